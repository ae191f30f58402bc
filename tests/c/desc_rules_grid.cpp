/*
 * desc_rules_grid.cpp -- xsknf_amd/csrc/desc_rules.h over a fixed grid, under
 * AddressSanitizer + UBSan (tests/test_desc_rules.py builds it with g++ and
 * compares every line with the numpy restatements of tests/copy_cases.py).
 * First line: "out_of_range <kOutOfRange>".  Then one line per case:
 *   <addr> <len> <size> <phase> <desc_offset> <in_umem> <chunk_count> <slot_bytes>
 * with the chunk count taken at byte address phase + offset (phase: the UMEM's
 * address mod 16).  UMEM sizes {16, 4096, 2^40}; offsets {0, 1, 15, 16,
 * size - 1, size, size + 1}, each as a plain address and, where it is large
 * enough, with 1 and with 65535 of it in address bits 48..63; lengths {0, 1, 15,
 * 16, 17, 33, size, 2^32 - 1} (size where a descriptor's 32 bits hold it);
 * every phase 0..15.  CPU only.
 */
#include <stdint.h>
#include <stdio.h>

#include "../../xsknf_amd/csrc/desc_rules.h"

int main()
{
	using namespace xsknf_gpu;
	printf("out_of_range %llu\n", (unsigned long long)kOutOfRange);
	const uint64_t sizes[] = {16, 4096, 1ull << 40};
	const uint64_t his[] = {0, 1, 65535};
	for (uint64_t size : sizes) {
		const uint64_t offs[] = {0, 1, 15, 16, size - 1, size, size + 1};
		const uint64_t lens[] = {0, 1, 15, 16, 17, 33, size, 0xffffffffull};
		for (uint64_t off : offs)
			for (uint64_t hi : his) {
				if (hi > off)
					continue;
				const uint64_t addr = (off - hi) | hi << XSKNF_GPU_UNALIGNED_BUF_OFFSET_SHIFT;
				for (uint64_t l : lens) {
					if (l > 0xffffffffull)
						continue;
					const uint32_t len = (uint32_t)l;
					for (uint64_t phase = 0; phase < 16; ++phase) {
						const uint64_t o = desc_offset(addr);
						printf("%llu %u %llu %llu %llu %d %llu %llu\n", (unsigned long long)addr, len,
						       (unsigned long long)size, (unsigned long long)phase, (unsigned long long)o,
						       in_umem(o, len, size) ? 1 : 0, (unsigned long long)chunk_count(phase + o, len),
						       (unsigned long long)slot_bytes(phase + o, len));
					}
				}
			}
	}
	return 0;
}

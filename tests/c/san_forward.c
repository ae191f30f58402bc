/*
 * san_forward.c -- the forwarding of routed frames on the host (xsknf_amd/csrc/
 * forward_host.cpp: xsknf_gpu_forward_host) under AddressSanitizer + UBSan, on
 * random sets: 1 to 32 interfaces, own, shared (NULL), rx-equal and smaller
 * destination UMEMs, empty lists, lengths 0 to 9000 at every address mod 16,
 * aligned- and unaligned-mode addresses, frames past the end and lengths of
 * 0xFFFFFFFF.  The UMEMs are heap blocks of exactly their size (aligned_alloc),
 * and in every case one frame ends at the last byte of the rx UMEM and of the
 * full-size destinations, so the sanitizer sees any byte read or written past a
 * frame's end there.  Checks every byte of every destination against a byte
 * loop of its own, and the stats; prints "ok <cases>".  CPU only
 * (tests/test_forward.py builds and runs it).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "xsknf_gpu.h"

static uint64_t st = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd(void)
{
	st ^= st >> 12;
	st ^= st << 25;
	st ^= st >> 27;
	return st * 0x2545F4914F6CDD1DULL;
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "case %d: %s failed (line %d)\n", cs, #c, __LINE__); return 1; } } while (0)

/* a heap block of exactly `size` bytes (a multiple of 16) at a 16-byte aligned address */
static uint8_t *block(uint64_t size, uint8_t **raw)
{
	*raw = aligned_alloc(16, size);
	return *raw;
}

int main(void)
{
	static const uint32_t lens[] = {0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1500, 9000};
	int cs;
	for (cs = 0; cs < 2000; cs++) {
		const uint32_t nif = cs % 3 == 0 ? 1 : (cs % 3 == 1 ? 2 + (uint32_t)(rnd() % 3) : 1 + (uint32_t)(rnd() % 32));
		/* sizes that are multiples of 16, so that the block's end is the UMEM's end */
		const uint64_t size = 16 * (640 + rnd() % 2048);
		uint8_t *rxraw, *rx = block(size, &rxraw);
		uint8_t *dst[32], *raw[32], *want[32];
		uint64_t sizes[32], counts[33] = {0}, total = 0, ws[3] = {0, 0, 0}, stats[3];
		CHECK(rx);
		for (uint64_t i = 0; i < size; i++)
			rx[i] = (uint8_t)(rnd() % 0xA5);
		for (uint32_t i = 0; i < nif; i++) {
			const int kind = (int)(rnd() % 5);
			raw[i] = want[i] = NULL;
			sizes[i] = kind == 2 ? 16 * (1 + rnd() % (size / 16)) : size;
			if (kind == 0) {
				dst[i] = NULL;
				sizes[i] = 0;
			} else if (kind == 1) {
				dst[i] = rx;
			} else {
				dst[i] = block(sizes[i], &raw[i]);
				want[i] = malloc(sizes[i]);
				CHECK(dst[i] && want[i]);
				memset(dst[i], 0xA5, sizes[i]);
				memset(want[i], 0xA5, sizes[i]);
			}
			counts[i] = cs % 11 == 0 ? 0 : rnd() % 12;
			total += counts[i];
		}
		struct xsknf_gpu_desc *tx = aligned_alloc(16, 16 * (total ? total : 1));
		CHECK(tx);
		uint64_t j = 0;
		for (uint32_t i = 0; i < nif; i++) {
			for (uint64_t k = 0; k < counts[i]; k++, j++) {
				uint32_t len = lens[rnd() % 13];
				uint64_t off;
				const int what = (int)(rnd() % 16);
				if (k == 0) {               /* ends at the last byte of the rx UMEM */
					off = size - len;
				} else if (what == 0) {     /* one byte too long for the rx UMEM */
					off = size - len + 1;
				} else if (what == 1) {     /* ends at / one past the end of this destination */
					len = len < sizes[i] ? len : 16;
					off = sizes[i] - len + (rnd() & 1);
				} else if (what == 2) {
					off = rnd() % size;
					len = 0xFFFFFFFFu;
				} else if (what == 3) {
					off = size + rnd() % 64;
				} else {
					off = rnd() % (size - len);
				}
				/* unaligned mode: part of the offset in bits 48 and up */
				const uint64_t delta = (rnd() & 1) && off >= 512 ? 256 + rnd() % 256 : 0;
				tx[j].addr = (off - delta) | delta << 48;
				tx[j].len = len;
				tx[j].options = 0;
				if (!want[i])
					continue;
				if (off <= size && len <= size - off && off <= sizes[i] && len <= sizes[i] - off) {
					for (uint32_t b = 0; b < len; b++)
						want[i][off + b] = rx[off + b];
					ws[0]++;
					ws[1] += len;
				} else {
					ws[2]++;
				}
			}
		}
		uint8_t *rxcopy = malloc(size);
		CHECK(rxcopy);
		memcpy(rxcopy, rx, size);
		CHECK(xsknf_gpu_forward_host(rx, size, dst, sizes, nif, tx, counts, NULL) == 0);
		CHECK(xsknf_gpu_forward_host(rx, size, dst, sizes, nif, tx, counts, stats) == 0);
		CHECK(stats[0] == ws[0] && stats[1] == ws[1] && stats[2] == ws[2]);
		CHECK(!memcmp(rx, rxcopy, size));
		for (uint32_t i = 0; i < nif; i++)
			CHECK(!want[i] || !memcmp(dst[i], want[i], sizes[i]));
		/* bad arguments are refused, not dereferenced */
		CHECK(xsknf_gpu_forward_host(rx, size, dst, sizes, 0, tx, counts, stats) < 0);
		CHECK(xsknf_gpu_forward_host(rx, size, dst, sizes, 33, tx, counts, stats) < 0);
		CHECK(xsknf_gpu_forward_host(rx, size, NULL, sizes, nif, tx, counts, stats) < 0);
		CHECK(xsknf_gpu_forward_host(rx, size, dst, NULL, nif, tx, counts, stats) < 0);
		CHECK(xsknf_gpu_forward_host(rx + 8, size - 8, dst, sizes, nif, tx, counts, stats) < 0);
		CHECK(total == 0 || xsknf_gpu_forward_host(NULL, size, dst, sizes, nif, tx, counts, stats) < 0);
		CHECK(total == 0 || xsknf_gpu_forward_host(rx, size, dst, sizes, nif, NULL, counts, stats) < 0);
		for (uint32_t i = 0; i < nif; i++) {
			free(raw[i]);
			free(want[i]);
		}
		free(tx); free(rxcopy); free(rxraw);
	}
	printf("ok %d\n", cs);
	return 0;
}

/*
 * san_macswap.c -- the macswap NF's host model (xsknf_amd/csrc/macswap_host.cpp:
 * xsknf_gpu_macswap_host) under AddressSanitizer + UBSan.  Every UMEM,
 * descriptor array and verdict array is a heap block of exactly its size, so a
 * read or write past a frame at the UMEM's end or past n verdicts is a heap
 * overflow.  Cases: random batches of frames of every length 0..40 packed with
 * gaps of 0..8 bytes, the last frame ending on the UMEM's last byte, descriptors
 * outside the UMEM, unaligned-mode addresses, every action and both swap
 * modes, 0 frames; and a 14-byte frame in the last 14 bytes of the UMEM.  The
 * result is checked against a byte-by-byte restatement of the header's rules;
 * prints "ok <cases>".  CPU only (tests/test_macswap_san.py builds and runs it).
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

/* a 14-byte frame in the UMEM's last 14 bytes, a short one at its start */
static int last_bytes_case(void)
{
	int cs = -1;
	for (uint64_t size = 14; size < 14 + 40; size++) {
		uint8_t *umem = malloc(size), *want = malloc(size);
		struct xsknf_gpu_desc *d = malloc(sizeof(*d) * 2);
		int32_t *v = malloc(sizeof(*v) * 2);
		CHECK(umem && want && d && v);
		for (uint64_t i = 0; i < size; i++)
			umem[i] = (uint8_t)rnd();
		memcpy(want, umem, size);
		memcpy(want + size - 14, umem + size - 8, 6);
		memcpy(want + size - 8, umem + size - 14, 6);
		d[0].addr = size - 14; d[0].len = 14; d[0].options = 0;
		d[1].addr = 0; d[1].len = size - 14 < 13 ? (uint32_t)(size - 14) : 13; d[1].options = 0;
		const struct xsknf_macswap_opts o = {XSKNF_MACSWAP_ACTION_PASS, 0, 3, 0};
		CHECK(xsknf_gpu_macswap_host(umem, size, d, 2, 0xffffffffu, &o, v) == 0);
		CHECK(v[0] == 0 && v[1] == -1 && !memcmp(umem, want, size));
		free(v); free(d); free(want); free(umem);
	}
	return 0;
}

int main(void)
{
	int cs;
	if (last_bytes_case())
		return 1;
	for (cs = 0; cs < 600; cs++) {
		const uint32_t nf = cs % 11 == 0 ? 0 : 1 + (uint32_t)(rnd() % 200);
		struct xsknf_gpu_desc *d = malloc(sizeof(*d) * nf);
		int32_t *v = malloc(sizeof(*v) * nf), *wv = malloc(sizeof(*wv) * nf);
		uint32_t *lens = malloc(sizeof(*lens) * nf), *gaps = malloc(sizeof(*gaps) * nf);
		uint64_t size = 0;
		CHECK(nf == 0 || (d && v && wv && lens && gaps));
		for (uint32_t i = 0; i < nf; i++) {
			lens[i] = rnd() % 3 ? 14 + (uint32_t)(rnd() % 4) : (uint32_t)(rnd() % 41);
			gaps[i] = rnd() % 2 ? 0 : (uint32_t)(rnd() % 9);   /* before frame i; the last frame ends the UMEM */
			size += gaps[i] + lens[i];
		}
		uint8_t *umem = malloc(size ? size : 1), *want = malloc(size ? size : 1);
		CHECK(umem && want);
		for (uint64_t i = 0; i < size; i++)
			umem[i] = (uint8_t)rnd();
		memcpy(want, umem, size);
		struct xsknf_macswap_opts o = {(uint32_t)(cs % 3), (uint32_t)(cs / 3 % 2) * (1 + (uint32_t)(rnd() % 9)),
					       cs % 3 == XSKNF_MACSWAP_ACTION_DROP ? (uint32_t)(rnd() % 2) : 1 + (uint32_t)(rnd() % 5), 0};
		const uint32_t ingress = cs % 7 == 0 ? 0xffffffffu : (uint32_t)(rnd() % 6);
		const int32_t fwd = o.action == XSKNF_MACSWAP_ACTION_DROP ? -1 : (int32_t)((ingress + 1u) % o.num_interfaces);
		uint64_t pos = 0;
		for (uint32_t i = 0; i < nf; i++) {
			pos += gaps[i];
			const uint64_t off48 = rnd() % ((pos < 0xffff ? pos : 0xffff) + 1);
			d[i].addr = (pos - off48) | off48 << 48;
			d[i].len = lens[i];
			d[i].options = (uint32_t)rnd();
			wv[i] = lens[i] >= 14 ? fwd : -1;
			if (rnd() % 10 == 0) {   /* outside the UMEM */
				switch (rnd() % 4) {
				case 0: d[i].addr = size; d[i].len = 1; break;
				case 1: d[i].addr = pos; d[i].len = (uint32_t)(size - pos) + 1; break;
				case 2: d[i].addr = 1ULL << 47; break;
				default: d[i].addr = 0xffffULL << 48 | 0xffffffffffffULL; d[i].len = 0xffffffffu; break;
				}
				wv[i] = -1;
			} else if (lens[i] >= 14 && !o.double_macswap) {
				memcpy(want + pos, umem + pos + 6, 6);
				memcpy(want + pos + 6, umem + pos, 6);
			}
			pos += lens[i];
		}
		CHECK(nf == 0 || pos == size);
		for (uint32_t i = 0; i < nf; i++)
			v[i] = 0x5a5a5a5a;
		CHECK(xsknf_gpu_macswap_host(umem, size, d, nf, ingress, &o, v) == 0);
		for (uint32_t i = 0; i < nf; i++)
			CHECK(v[i] == wv[i]);
		CHECK(!memcmp(umem, want, size));
		/* the argument errors touch nothing */
		o.action = 3;
		CHECK(xsknf_gpu_macswap_host(umem, size, d, nf, ingress, &o, v) == -22);
		o.action = XSKNF_MACSWAP_ACTION_REDIRECT;
		o.num_interfaces = 0;
		CHECK(xsknf_gpu_macswap_host(umem, size, d, nf, ingress, &o, v) == -22);
		CHECK(xsknf_gpu_macswap_host(umem, size, d, nf, ingress, NULL, v) == -22);
		CHECK(!memcmp(umem, want, size));
		free(want);
		free(umem);
		free(gaps);
		free(lens);
		free(wv);
		free(v);
		free(d);
	}
	printf("ok %d\n", cs);
	return 0;
}

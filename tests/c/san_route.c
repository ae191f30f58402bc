/*
 * san_route.c -- the routing of a checksummed batch on the host (xsknf_amd/csrc/
 * route_host.cpp: xsknf_gpu_route_host) under AddressSanitizer + UBSan, on
 * random and edge-case verdict sets: empty batches, one frame, every frame in
 * one bin, bins that stay empty, verdicts that name no interface (past the
 * count, negative, INT32_MIN / INT32_MAX, record-tagged words), 1 to 32
 * interfaces.  The tx and fill buffers are allocated at exactly ntx and the drop
 * count entries (counted here by the header's rule), so the sanitizer sees any
 * write past the totals.  Checks the lists entry by entry against `order` and
 * the stable-partition invariants; prints "ok <cases>".  CPU only
 * (tests/test_route.py builds and runs it).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "xsknf_gpu.h"

static uint64_t st = 0xD1B54A32D192ED03ULL;
static uint64_t rnd(void)
{
	st ^= st >> 12;
	st ^= st << 25;
	st ^= st >> 27;
	return st * 0x2545F4914F6CDD1DULL;
}

/* the header's rule, restated */
static uint32_t bin_of(int32_t v, uint32_t nif)
{
	if (nif == 1)
		return v == -1 ? 1 : 0;
	return (v < 0 || (uint32_t)v >= nif) ? nif : (uint32_t)v;
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "case %d: %s failed (line %d)\n", cs, #c, __LINE__); return 1; } } while (0)

int main(void)
{
	static const int32_t stray[] = {-2, INT32_MIN, INT32_MAX, 0x40000000, 0x404A1234, 32, 33, 0x7eadbeef};
	int cs;
	for (cs = 0; cs < 4000; cs++) {
		const uint32_t n = cs % 7 == 0 ? 0 : (cs % 5 == 0 ? 1 + (uint32_t)(rnd() % 4) : (uint32_t)(rnd() % 6000));
		const uint32_t nif = cs % 3 == 0 ? 1 : (cs % 3 == 1 ? 2 + (uint32_t)(rnd() % 3) : 1 + (uint32_t)(rnd() % 32));
		const int kind = cs % 6;
		struct xsknf_gpu_desc *d = malloc(sizeof(*d) * n);
		int32_t *v = malloc(sizeof(*v) * n);
		uint64_t want[33] = {0}, counts[33], ntx = 0;
		CHECK(n == 0 || (d && v));
		for (uint32_t i = 0; i < n; i++) {
			d[i].addr = rnd();
			d[i].len = (uint32_t)rnd();
			d[i].options = (uint32_t)rnd() | 1;
			switch (kind) {
			case 0: v[i] = (int32_t)(rnd() % (nif + 1)) - 1; break;          /* uniform */
			case 1: v[i] = -1; break;                                       /* all dropped */
			case 2: v[i] = (int32_t)(nif - 1); break;                       /* all on one interface */
			case 3: v[i] = rnd() % 4 ? (int32_t)(rnd() % (nif + 1)) - 1     /* strays among them */
						 : stray[rnd() % (sizeof(stray) / sizeof(stray[0]))]; break;
			case 4: v[i] = (int32_t)((i / 97) % (nif + 1)) - 1; break;      /* runs */
			default: v[i] = (int32_t)(rnd() % nif); break;                  /* no drop at all */
			}
			want[bin_of(v[i], nif)]++;
		}
		for (uint32_t k = 0; k < nif; k++)
			ntx += want[k];
		/* exactly as long as the lists (a size of 0 leaves no byte to write) */
		struct xsknf_gpu_desc *tx = malloc(sizeof(*tx) * ntx);
		uint64_t *fill = malloc(sizeof(*fill) * want[nif]);
		uint32_t *order = malloc(sizeof(*order) * n);
		CHECK(tx && fill && order);
		CHECK(xsknf_gpu_route_host(d, v, n, nif, tx, fill, cs % 2 ? order : NULL, NULL) == 0);
		CHECK(xsknf_gpu_route_host(d, v, n, nif, tx, fill, order, counts) == 0);
		CHECK(ntx + want[nif] == n);
		uint64_t at = 0;
		for (uint32_t k = 0; k <= nif; k++) {
			CHECK(counts[k] == want[k]);
			for (uint64_t r = 0; r < want[k]; r++, at++) {
				const uint32_t f = order[at];
				CHECK(f < n && bin_of(v[f], nif) == k);
				CHECK(r == 0 || order[at - 1] < f);           /* receive order within the list */
				if (k < nif)
					CHECK(tx[at].addr == d[f].addr && tx[at].len == d[f].len && tx[at].options == 0);
				else
					CHECK(fill[r] == d[f].addr);
			}
		}
		CHECK(at == n);
		/* bad arguments are refused, not dereferenced */
		CHECK(xsknf_gpu_route_host(d, v, n, 0, tx, fill, order, counts) < 0);
		CHECK(xsknf_gpu_route_host(d, v, n, 33, tx, fill, order, counts) < 0);
		CHECK(n == 0 || xsknf_gpu_route_host(NULL, v, n, nif, tx, fill, order, counts) < 0);
		CHECK(n == 0 || xsknf_gpu_route_host(d, NULL, n, nif, tx, fill, order, counts) < 0);
		CHECK(n == 0 || xsknf_gpu_route_host(d, v, n, nif, NULL, fill, order, counts) < 0);
		CHECK(n == 0 || xsknf_gpu_route_host(d, v, n, nif, tx, NULL, order, counts) < 0);
		free(d); free(v); free(tx); free(fill); free(order);
	}
	printf("ok %d\n", cs);
	return 0;
}

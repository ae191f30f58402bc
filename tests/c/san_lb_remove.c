/*
 * san_lb_remove.c -- removing sessions from the load balancer's host table
 * (xsknf_amd/csrc/lb.cpp, built with XSKNF_LB_HOST_ONLY: no GPU call;
 * xsknf_gpu_lb_sessions_remove_host, _drain_backend_host, _sessions_clear)
 * under AddressSanitizer + UBSan.  Random sequences of put / batch / remove /
 * drain / clear on small tables (64 slots, so that rebuilds happen all the
 * time) against a model: an array of sessions on which a removal is decided
 * from a copy taken before the call (the header's set semantics).  Addresses
 * and ports come from a handful of values, so that stored sessions are each
 * other's partners by design and by accident, in both directions, and so that
 * lists hold duplicates and keys beside their partners.  Every key list, result
 * and dump buffer is a heap block of exactly its size.  After every step the
 * dump equals the model and the count is right; after a batch (which creates
 * sessions as the NF does) the model is read back from the dump.  Prints
 * "ok <cases>".  CPU only (tests/test_lb_remove_san.py builds and runs it).
 */
#include <errno.h>
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

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "case %d step %d: %s failed (line %d)\n", cs, step, #c, __LINE__); return 1; } } while (0)

typedef struct xsknf_gpu_lb_session_key K;
typedef struct xsknf_gpu_lb_session_value V;

#define MAXS 24
#define SLOTS 64
static K mk[MAXS];
static V mv[MAXS];
static uint32_t mn, tombs;

static int same(const K *x, const K *y)
{
	return x->saddr == y->saddr && x->daddr == y->daddr && x->sport == y->sport && x->dport == y->dport &&
	       x->proto == y->proto;
}
static int at(const K *k, const K *tab, uint32_t n)
{
	for (uint32_t i = 0; i < n; i++)
		if (same(&tab[i], k)) return (int)i;
	return -1;
}
static K partner(const K *k, const V *v)
{
	K p;
	memset(&p, 0, sizeof(p));
	p.proto = k->proto;
	if (v->dir == XSKNF_GPU_LB_TO_BACKEND) {
		p.saddr = v->addr; p.daddr = k->saddr; p.sport = v->port; p.dport = k->sport;
	} else {
		p.saddr = k->daddr; p.daddr = v->addr; p.sport = k->dport; p.dport = v->port;
	}
	return p;
}
/* gone[i] of the model's sessions leave; returns the expected COMPACTED */
static uint64_t settle(const uint8_t *gone, uint64_t *removed)
{
	uint32_t w = 0;
	*removed = 0;
	for (uint32_t i = 0; i < mn; i++) {
		if (gone[i]) { ++*removed; continue; }
		mk[w] = mk[i];
		mv[w++] = mv[i];
	}
	mn = w;
	tombs += (uint32_t)*removed;
	if (tombs <= SLOTS / 4) return 0;
	tombs = 0;
	return 1;
}
static K small_key(void)
{
	K k;
	memset(&k, 0, sizeof(k));
	k.saddr = 1 + rnd() % 4; k.daddr = 1 + rnd() % 4; k.sport = (uint16_t)(1 + rnd() % 2); k.dport = (uint16_t)(1 + rnd() % 2);
	k.proto = rnd() & 1 ? 6 : 17;
	return k;
}
static int cmp_key(const K *x, const K *y)
{
	uint32_t xc = x->sport | (uint32_t)x->dport << 16, yc = y->sport | (uint32_t)y->dport << 16;
	if (x->saddr != y->saddr) return x->saddr < y->saddr ? -1 : 1;
	if (x->daddr != y->daddr) return x->daddr < y->daddr ? -1 : 1;
	if (xc != yc) return xc < yc ? -1 : 1;
	return x->proto < y->proto ? -1 : x->proto > y->proto;
}

int main(void)
{
	int cs, step = 0;
	uint64_t rebuilds = 0, pairs = 0;
	for (cs = 0; cs < 300; cs++) {
		struct xsknf_gpu_lb_backend bk[3];
		memset(bk, 0, sizeof(bk));
		for (uint32_t i = 0; i < 3; i++) {
			bk[i].vaddr = 9; bk[i].vport = 9; bk[i].proto = 17;
			bk[i].addr = 1 + i; bk[i].port = (uint16_t)(1 + i % 2); bk[i].ifindex = (uint16_t)i;
		}
		struct xsknf_gpu_lb *lb = NULL;
		CHECK(xsknf_gpu_lb_create(&lb, bk, 3, MAXS, SLOTS) == 0);
		mn = tombs = 0;
		for (step = 0; step < 40; step++) {
			uint32_t op = rnd() % 10;
			uint64_t *res = malloc(sizeof(uint64_t) * XSKNF_GPU_LB_REMOVE_RESULT), want_removed = 0, want_compacted = 0;
			int counted = 0;
			res[0] = res[1] = 77;
			if (op < 3) {   /* put */
				uint32_t n = rnd() % 6;
				K *k = malloc(sizeof(K) * (n ? n : 1));
				V *v = malloc(sizeof(V) * (n ? n : 1));
				int full = 0;
				for (uint32_t i = 0; i < n; i++) {
					k[i] = small_key();
					memset(&v[i], 0, sizeof(V));
					v[i].addr = 1 + rnd() % 4; v[i].port = (uint16_t)(1 + rnd() % 2); v[i].dir = (uint8_t)(rnd() & 1);
					if (rnd() % 3 == 0 && mn) {   /* the partner of a stored session, aimed back at it */
						uint32_t j = rnd() % mn;
						k[i] = partner(&mk[j], &mv[j]);
						v[i].dir = !mv[j].dir;
						if (v[i].dir == XSKNF_GPU_LB_TO_BACKEND) { v[i].addr = mk[j].saddr; v[i].port = mk[j].sport; }
						else { v[i].addr = mk[j].daddr; v[i].port = mk[j].dport; }
					}
					int j = at(&k[i], mk, mn);
					if (full) continue;
					if (j >= 0) mv[j] = v[i];
					else if (mn == MAXS) full = 1;
					else { mk[mn] = k[i]; mv[mn++] = v[i]; }
				}
				CHECK(xsknf_gpu_lb_sessions_put(lb, n ? k : NULL, n ? v : NULL, n) == (full ? -ENOSPC : 0));
				free(k); free(v);
			} else if (op == 3) {   /* a batch of new flows and of frames of stored sessions; then read the model back */
				uint32_t n = 1 + rnd() % 6;
				uint8_t *umem = malloc(64 * n);
				struct xsknf_gpu_desc *d = malloc(sizeof(*d) * n);
				int32_t *verd = malloc(sizeof(int32_t) * n);
				for (uint32_t i = 0; i < n; i++) {
					uint8_t *f = umem + 64 * i;
					K k = small_key();
					if (rnd() & 1) { k.daddr = 9; k.dport = 9; k.proto = 17; }
					for (int b = 0; b < 64; b++) f[b] = (uint8_t)rnd();
					f[12] = 8; f[13] = 0; f[14] = 0x45; f[23] = k.proto;
					memcpy(f + 26, &k.saddr, 4); memcpy(f + 30, &k.daddr, 4);
					memcpy(f + 34, &k.sport, 2); memcpy(f + 36, &k.dport, 2);
					d[i].addr = 64ull * i; d[i].len = 64; d[i].options = 0;
				}
				uint64_t stats[XSKNF_GPU_LB_STATS];
				CHECK(xsknf_gpu_lb_host(umem, 64 * n, d, n, 1, 4, lb, verd, stats) == 0);
				CHECK(stats[4] + mn <= MAXS);
				uint32_t cnt = 0;
				CHECK(xsknf_gpu_lb_sessions_dump(lb, XSKNF_GPU_LB_HOST_TABLE, mk, mv, MAXS, &cnt) == 0);
				CHECK(cnt == mn + stats[4]);
				mn = cnt;
				free(umem); free(d); free(verd);
			} else if (op < 8) {   /* remove */
				uint32_t n = rnd() % 9, flags = rnd() & 1 ? XSKNF_GPU_LB_REMOVE_PAIR : 0;
				K *k = malloc(sizeof(K) * (n ? n : 1));
				uint8_t gone[MAXS];
				memset(gone, 0, sizeof(gone));
				for (uint32_t i = 0; i < n; i++) {
					uint32_t how = rnd() % 5;
					if (how == 0 || !mn) k[i] = small_key();
					else if (how == 1 && i) k[i] = k[rnd() % i];                      /* a duplicate */
					else if (how == 2) { uint32_t j = rnd() % mn; k[i] = partner(&mk[j], &mv[j]); }
					else k[i] = mk[rnd() % mn];
					if (rnd() % 16 == 0) k[i].proto = (uint8_t)rnd();
					k[i].pad[0] = (uint8_t)rnd();
				}
				for (uint32_t i = 0; i < n; i++) {
					int j = k[i].proto == 6 || k[i].proto == 17 ? at(&k[i], mk, mn) : -1;
					if (j < 0) continue;
					gone[j] = 1;
					if (!flags) continue;
					K p = partner(&mk[j], &mv[j]);
					int q = at(&p, mk, mn);
					if (q < 0 || mv[q].dir == mv[j].dir) continue;
					K back = partner(&mk[q], &mv[q]);
					if (same(&back, &mk[j])) { pairs += !gone[q]; gone[q] = 1; }
				}
				want_compacted = settle(gone, &want_removed);
				CHECK(xsknf_gpu_lb_sessions_remove_host(lb, n ? k : NULL, n, flags, res) == 0);
				counted = 1;
				free(k);
			} else if (op == 8) {   /* drain */
				uint32_t addr = 1 + rnd() % 4, port = 1 + rnd() % 2, proto = rnd() & 1 ? 6 : 17;
				uint8_t gone[MAXS];
				for (uint32_t i = 0; i < mn; i++)
					gone[i] = mk[i].proto == proto &&
					          (mv[i].dir == XSKNF_GPU_LB_TO_BACKEND ? mv[i].addr == addr && mv[i].port == port
					                                                : mk[i].saddr == addr && mk[i].sport == port);
				want_compacted = settle(gone, &want_removed);
				CHECK(xsknf_gpu_lb_drain_backend_host(lb, addr, (uint16_t)port, (uint8_t)proto, res) == 0);
				counted = 1;
			} else if (rnd() % 4 == 0) {   /* clear */
				CHECK(xsknf_gpu_lb_sessions_clear(lb, XSKNF_GPU_LB_HOST_TABLE, NULL) == 0);
				mn = tombs = 0;
			}
			if (counted) {
				CHECK(res[XSKNF_GPU_LB_REMOVED] == want_removed && res[XSKNF_GPU_LB_COMPACTED] == want_compacted);
				rebuilds += want_compacted;
			}
			free(res);
			/* the dump is the model, sorted */
			struct xsknf_gpu_lb_info info;
			CHECK(xsknf_gpu_lb_info(lb, &info) == 0 && info.host_sessions == mn);
			uint32_t cnt = 0;
			K *dk = malloc(sizeof(K) * (mn ? mn : 1));
			V *dv = malloc(sizeof(V) * (mn ? mn : 1));
			CHECK(xsknf_gpu_lb_sessions_dump(lb, XSKNF_GPU_LB_HOST_TABLE, dk, dv, mn, &cnt) == 0 && cnt == mn);
			for (uint32_t i = 0; i < cnt; i++) {
				int j = at(&dk[i], mk, mn);
				CHECK(j >= 0 && mv[j].addr == dv[i].addr && mv[j].port == dv[i].port && mv[j].dir == dv[i].dir &&
				      mv[j].ifindex == dv[i].ifindex);
				CHECK(i == 0 || cmp_key(&dk[i - 1], &dk[i]) < 0);
			}
			free(dk); free(dv);
		}
		CHECK(xsknf_gpu_lb_sessions_remove(lb, NULL, 0, 0, NULL, NULL) == -ENODEV);
		CHECK(xsknf_gpu_lb_destroy(lb) == 0);
	}
	if (rebuilds < 100 || pairs < 100) {
		fprintf(stderr, "too few rebuilds (%llu) or partners (%llu) to mean anything\n", (unsigned long long)rebuilds,
		        (unsigned long long)pairs);
		return 1;
	}
	printf("ok %d\n", cs);
	return 0;
}

/*
 * san_lb_age.c -- ageing of the load balancer's host table (xsknf_amd/csrc/lb.cpp,
 * built with XSKNF_LB_HOST_ONLY: no GPU call, and lb_host.cpp;
 * xsknf_gpu_lb_aging_enable, _clock, _sessions_expire_host, _sessions_ages) under
 * AddressSanitizer + UBSan.  Random sequences of put / batch / clock / expire /
 * remove on small tables (64 slots, so that rebuilds happen all the time and
 * carry stamps) against a model: an array of sessions, each with its stamp, on
 * which an expiry is decided from the table as it stood before the call (the
 * header's set semantics and pair rule).  One service with one backend, so a
 * flow's backward key is known here without jhash; addresses and ports come
 * from a handful of values, so that put entries are partners of stored sessions
 * by design and by accident.  Half the objects enable ageing on a table that
 * already holds sessions, some after a removal has made the rebuild's scratch.
 * Every buffer is a heap block of exactly its size.  After every step the ages
 * dump equals the model.  Prints "ok <cases>".  CPU only
 * (tests/test_lb_age_san.py builds and runs it).
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
#define BK_ADDR 2u
#define BK_PORT 1u
static K mk[MAXS];
static V mv[MAXS];
static uint32_t ms[MAXS];   /* the stamps */
static uint32_t mn, tombs, clk;

static int same(const K *x, const K *y)
{
	return x->saddr == y->saddr && x->daddr == y->daddr && x->sport == y->sport && x->dport == y->dport &&
	       x->proto == y->proto;
}
static int at(const K *k)
{
	for (uint32_t i = 0; i < mn; i++)
		if (same(&mk[i], k)) return (int)i;
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
static uint64_t settle(const uint8_t *gone, uint64_t *removed)
{
	uint32_t w = 0;
	*removed = 0;
	for (uint32_t i = 0; i < mn; i++) {
		if (gone[i]) { ++*removed; continue; }
		mk[w] = mk[i];
		ms[w] = ms[i];
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
	k.proto = 17;
	return k;
}
/* the model's insert: 1 stored or replaced (and stamped), 0 refused */
static int store(const K *k)
{
	int j = at(k);
	if (j < 0) {
		if (mn == MAXS) return 0;
		j = (int)mn++;
		mk[j] = *k;
		memset(&mv[j], 0, sizeof(V));
	}
	ms[j] = clk;
	return 1;
}
/* the values of the model's keys, from a dump */
static int read_values(struct xsknf_gpu_lb *lb)
{
	K *dk = malloc(sizeof(K) * (mn ? mn : 1));
	V *dv = malloc(sizeof(V) * (mn ? mn : 1));
	uint32_t cnt = 0;
	int ok = xsknf_gpu_lb_sessions_dump(lb, XSKNF_GPU_LB_HOST_TABLE, dk, dv, mn, &cnt) == 0 && cnt == mn;
	for (uint32_t i = 0; ok && i < cnt; i++) {
		int j = at(&dk[i]);
		if (j < 0) ok = 0;
		else mv[j] = dv[i];
	}
	free(dk); free(dv);
	return ok;
}

int main(void)
{
	int cs, step = 0;
	uint64_t rebuilds = 0, expired = 0, kept_by_partner = 0;
	for (cs = 0; cs < 300; cs++) {
		struct xsknf_gpu_lb_backend bk;
		memset(&bk, 0, sizeof(bk));
		bk.vaddr = 9; bk.vport = 9; bk.proto = 17; bk.addr = BK_ADDR; bk.port = BK_PORT; bk.ifindex = 2;
		struct xsknf_gpu_lb *lb = NULL;
		CHECK(xsknf_gpu_lb_create(&lb, &bk, 1, MAXS, SLOTS) == 0);
		mn = tombs = clk = 0;
		step = -1;
		CHECK(xsknf_gpu_lb_clock(lb, XSKNF_GPU_LB_HOST_TABLE, 1, NULL) == -EINVAL);
		CHECK(xsknf_gpu_lb_sessions_expire_host(lb, 0, NULL) == -EINVAL);
		if (cs & 1) {   /* sessions from before ageing: stamp 0 */
			uint32_t n = 1 + rnd() % 8;
			K *k = malloc(sizeof(K) * n);
			V *v = malloc(sizeof(V) * n);
			for (uint32_t i = 0; i < n; i++) {
				k[i] = small_key();
				memset(&v[i], 0, sizeof(V));
				v[i].addr = 1 + rnd() % 4; v[i].port = (uint16_t)(1 + rnd() % 2); v[i].dir = (uint8_t)(rnd() & 1);
				store(&k[i]);
			}
			CHECK(xsknf_gpu_lb_sessions_put(lb, k, v, n) == 0);
			if (cs & 2) {   /* and the rebuild's scratch from before ageing */
				uint8_t gone[MAXS] = {1};
				uint64_t removed;
				CHECK(xsknf_gpu_lb_sessions_remove_host(lb, &mk[0], 1, 0, NULL) == 0);
				(void)settle(gone, &removed);
			}
			free(k); free(v);
			CHECK(read_values(lb));
		}
		CHECK(xsknf_gpu_lb_aging_enable(lb) == 0);
		for (step = 0; step < 40; step++) {
			uint32_t op = rnd() % 10;
			if (op < 2) {   /* put */
				uint32_t n = 1 + rnd() % 5;
				K *k = malloc(sizeof(K) * n);
				V *v = malloc(sizeof(V) * n);
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
					if (!full && !store(&k[i])) full = 1;
				}
				CHECK(xsknf_gpu_lb_sessions_put(lb, k, v, n) == (full ? -ENOSPC : 0));
				free(k); free(v);
				CHECK(read_values(lb));
			} else if (op < 5) {   /* a batch: rule 11 frame by frame */
				uint32_t n = 1 + rnd() % 6;
				uint8_t *umem = malloc(64 * n);
				struct xsknf_gpu_desc *d = malloc(sizeof(*d) * n);
				int32_t *verd = malloc(sizeof(int32_t) * n);
				uint64_t failed = 0;
				for (uint32_t i = 0; i < n; i++) {
					uint8_t *f = umem + 64 * i;
					K k = small_key();
					if (rnd() & 1) { k.daddr = 9; k.dport = 9; }
					else if (mn && rnd() & 1) k = mk[rnd() % mn];
					for (int b = 0; b < 64; b++) f[b] = (uint8_t)rnd();
					f[12] = 8; f[13] = 0; f[14] = 0x45; f[23] = k.proto;
					if (rnd() % 8 == 0) f[12] = 0x86;   /* passes: nothing stamped */
					memcpy(f + 26, &k.saddr, 4); memcpy(f + 30, &k.daddr, 4);
					memcpy(f + 34, &k.sport, 2); memcpy(f + 36, &k.dport, 2);
					d[i].addr = 64ull * i; d[i].len = 64; d[i].options = 0;
					if (f[12] != 8) continue;
					int j = at(&k);
					if (j >= 0) { ms[j] = clk; continue; }                    /* rule 7 */
					if (k.daddr != 9 || k.dport != 9) continue;               /* rule 8 */
					if (!store(&k)) { failed++; continue; }                   /* rule 9; a failed insert stamps nothing */
					K back;
					memset(&back, 0, sizeof(back));
					back.saddr = BK_ADDR; back.daddr = k.saddr; back.sport = BK_PORT; back.dport = k.sport; back.proto = 17;
					if (!store(&back)) failed++;
				}
				uint64_t stats[XSKNF_GPU_LB_STATS];
				CHECK(xsknf_gpu_lb_host(umem, 64 * n, d, n, 1, 4, lb, verd, stats) == 0);
				CHECK(stats[5] == failed);
				free(umem); free(d); free(verd);
				CHECK(read_values(lb));
			} else if (op < 7) {   /* clock: mostly forward, sometimes across the wrap */
				clk = rnd() % 16 == 0 ? 0xfffffff8u + (uint32_t)(rnd() % 16) : clk + (uint32_t)(rnd() % 6);
				CHECK(xsknf_gpu_lb_clock(lb, XSKNF_GPU_LB_HOST_TABLE, clk, NULL) == 0);
			} else {   /* expire (or, one time in four, a plain removal: its rebuild carries stamps too) */
				uint64_t *res = malloc(sizeof(uint64_t) * XSKNF_GPU_LB_REMOVE_RESULT), want_removed = 0, want_compacted;
				uint8_t gone[MAXS];
				memset(gone, 0, sizeof(gone));
				res[0] = res[1] = 77;
				if (rnd() % 4 == 0 && mn) {
					K k = mk[rnd() % mn];
					gone[at(&k)] = 1;
					want_compacted = settle(gone, &want_removed);
					CHECK(xsknf_gpu_lb_sessions_remove_host(lb, &k, 1, 0, res) == 0);
				} else {
					uint32_t max_idle = rnd() % 8 == 0 ? 0xffffffffu : (uint32_t)(rnd() % 6);
					for (uint32_t i = 0; i < mn; i++) {
						if ((uint32_t)(clk - ms[i]) <= max_idle) continue;
						K p = partner(&mk[i], &mv[i]);
						int q = at(&p);
						if (q >= 0 && mv[q].dir != mv[i].dir) {
							K back = partner(&mk[q], &mv[q]);
							if (same(&back, &mk[i]) && (uint32_t)(clk - ms[q]) <= max_idle) { kept_by_partner++; continue; }
						}
						gone[i] = 1;
					}
					want_compacted = settle(gone, &want_removed);
					CHECK(xsknf_gpu_lb_sessions_expire_host(lb, max_idle, res) == 0);
					expired += want_removed;
				}
				CHECK(res[XSKNF_GPU_LB_REMOVED] == want_removed && res[XSKNF_GPU_LB_COMPACTED] == want_compacted);
				rebuilds += want_compacted;
				free(res);
			}
			/* the ages dump is the model's */
			struct xsknf_gpu_lb_info info;
			CHECK(xsknf_gpu_lb_info(lb, &info) == 0 && info.host_sessions == mn);
			uint32_t cnt = 0, now = 77;
			K *dk = malloc(sizeof(K) * (mn ? mn : 1));
			uint32_t *da = malloc(sizeof(uint32_t) * (mn ? mn : 1));
			CHECK(xsknf_gpu_lb_sessions_ages(lb, XSKNF_GPU_LB_HOST_TABLE, dk, da, mn, &cnt, &now) == 0);
			CHECK(cnt == mn && now == clk);
			for (uint32_t i = 0; i < cnt; i++) {
				int j = at(&dk[i]);
				CHECK(j >= 0 && da[i] == (uint32_t)(clk - ms[j]));
			}
			free(dk); free(da);
		}
		CHECK(xsknf_gpu_lb_aging_enable(lb) == 0);   /* idempotent */
		CHECK(xsknf_gpu_lb_sessions_expire(lb, 0, NULL, NULL) == -ENODEV);
		CHECK(xsknf_gpu_lb_clock(lb, XSKNF_GPU_LB_DEVICE_TABLE, 1, NULL) == -ENODEV);
		CHECK(xsknf_gpu_lb_destroy(lb) == 0);
	}
	if (rebuilds < 50 || expired < 500 || kept_by_partner < 50) {
		fprintf(stderr, "too few rebuilds (%llu), expiries (%llu) or kept pairs (%llu) to mean anything\n",
		        (unsigned long long)rebuilds, (unsigned long long)expired, (unsigned long long)kept_by_partner);
		return 1;
	}
	printf("ok %d\n", cs);
	return 0;
}

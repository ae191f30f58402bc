/*
 * san_lb_backends.c -- the services and backends of a live load balancer and
 * the list drain on the host copy and the host table (xsknf_amd/csrc/lb.cpp,
 * built with XSKNF_LB_HOST_ONLY: no GPU call; xsknf_gpu_lb_backends_update,
 * _backends_dump, _drain_backends_host) under AddressSanitizer + UBSan.
 * Random sequences of update / batch / put / list drain / dump on small tables
 * against a model in C: the services as arrays edited by the header's rules, the
 * sessions as an array on which a drain is decided from the state before the
 * call.  Services, addresses and ports come from a handful of values, so that
 * updates hit existing backends, duplicates and absent ones, and services come
 * and go.  Every op list, id list, result and dump buffer is a heap block of
 * exactly its size.  After every step both dumps equal the model; a batch's
 * frames towards a service the model holds are rewritten, and the model's
 * sessions are read back from the dump.  Three cases also walk the capacity
 * edges (1024 services, 131072 records, one more of each).  Prints
 * "ok <cases>".  CPU only (tests/test_lb_backends_san.py builds and runs it).
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
typedef struct xsknf_gpu_lb_backend B;
typedef struct xsknf_gpu_lb_backend_op OP;
typedef struct xsknf_gpu_lb_backend_id ID;

#define MAXS 24
#define SLOTS 64
#define MAXSVC 12   /* 3 addresses x 2 ports x 2 protocols */
#define MAXB 64
static K mk[MAXS];
static V mv[MAXS];
static uint32_t mn, tombs;
/* the services: ms[s] holds nb[s] records (the service's key in every one), in backend order */
static B ms[MAXSVC][MAXB];
static uint32_t nb[MAXSVC], nsvc;

static int same_svc(const B *x, const B *y) { return x->vaddr == y->vaddr && x->vport == y->vport && x->proto == y->proto; }
static int same_bk(const B *x, const B *y) { return x->addr == y->addr && x->port == y->port; }
static int svc_at(const B *r)
{
	for (uint32_t s = 0; s < nsvc; s++)
		if (same_svc(&ms[s][0], r)) return (int)s;
	return -1;
}
static void model_update(const OP *ops, uint32_t n)
{
	for (uint32_t i = 0; i < n; i++) {
		const B *r = &ops[i].backend;
		int s = svc_at(r);
		if (ops[i].op == XSKNF_GPU_LB_BACKEND_REMOVE) {
			if (s < 0) continue;
			uint32_t w = 0;
			for (uint32_t k = 0; k < nb[s]; k++)
				if (!same_bk(&ms[s][k], r)) ms[s][w++] = ms[s][k];
			nb[s] = w;
			if (w) continue;
			for (uint32_t t = (uint32_t)s; t + 1 < nsvc; t++) {
				memcpy(ms[t], ms[t + 1], sizeof(ms[t]));
				nb[t] = nb[t + 1];
			}
			--nsvc;
			continue;
		}
		if (s < 0) {
			ms[nsvc][0] = *r;
			nb[nsvc++] = 1;
			continue;
		}
		int found = 0;
		for (uint32_t k = 0; k < nb[s]; k++)
			if (same_bk(&ms[s][k], r)) { ms[s][k] = *r; found = 1; }
		if (!found) ms[s][nb[s]++] = *r;
	}
}
static uint32_t model_total(void)
{
	uint32_t t = 0;
	for (uint32_t s = 0; s < nsvc; s++) t += nb[s];
	return t;
}
static int svc_less(const B *x, const B *y)
{
	uint32_t xv = x->vport | (uint32_t)x->proto << 16, yv = y->vport | (uint32_t)y->proto << 16;
	return x->vaddr != y->vaddr ? x->vaddr < y->vaddr : xv < yv;
}
static int same_rec(const B *x, const B *y)
{
	return same_svc(x, y) && same_bk(x, y) && x->ifindex == y->ifindex && !memcmp(x->mac, y->mac, 6);
}

static B small_rec(void)
{
	B r;
	memset(&r, 0, sizeof(r));
	r.vaddr = 9 + rnd() % 3; r.vport = (uint16_t)(9 + rnd() % 2); r.proto = rnd() & 1 ? 6 : 17;
	r.addr = 1 + rnd() % 4; r.port = (uint16_t)(1 + rnd() % 2); r.ifindex = (uint16_t)(rnd() % 4);
	for (int b = 0; b < 6; b++) r.mac[b] = (uint8_t)rnd();
	r.pad = (uint8_t)rnd(); r.pad2[0] = (uint8_t)rnd();
	return r;
}
static K small_key(void)
{
	K k;
	memset(&k, 0, sizeof(k));
	k.saddr = 1 + rnd() % 4; k.daddr = 1 + rnd() % 4; k.sport = (uint16_t)(1 + rnd() % 2); k.dport = (uint16_t)(1 + rnd() % 2);
	k.proto = rnd() & 1 ? 6 : 17;
	return k;
}
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

/* the capacity edges, on exactly sized buffers */
static int edges(int cs)
{
	int step = -1;
	const uint32_t S = XSKNF_GPU_LB_MAX_SERVICES, N = XSKNF_GPU_LB_MAX_BACKENDS;
	B *r = calloc(S - 1, sizeof(B));
	for (uint32_t i = 0; i < S - 1; i++) { r[i].vaddr = 100 + i; r[i].vport = 1; r[i].proto = 6; r[i].addr = 1; r[i].port = 1; }
	struct xsknf_gpu_lb *lb = NULL;
	CHECK(xsknf_gpu_lb_create(&lb, r, S - 1, 4, 64) == 0);
	OP *o = calloc(2, sizeof(OP));
	o[0].backend = r[0]; o[0].backend.vaddr = 50;
	o[1].backend = r[0]; o[1].backend.vaddr = 51;
	CHECK(xsknf_gpu_lb_backends_update(lb, o, 2, NULL) == -ENOSPC);        /* 1025 */
	CHECK(xsknf_gpu_lb_backends_update(lb, o, 1, NULL) == 0);              /* exactly 1024 */
	CHECK(xsknf_gpu_lb_backends_update(lb, o + 1, 1, NULL) == -ENOSPC);
	o[0].op = XSKNF_GPU_LB_BACKEND_REMOVE;
	CHECK(xsknf_gpu_lb_backends_update(lb, o, 2, NULL) == 0);              /* one out, one in */
	uint32_t cnt = 0;
	B *d = calloc(S, sizeof(B));
	CHECK(xsknf_gpu_lb_backends_dump(lb, XSKNF_GPU_LB_HOST_TABLE, d, S, &cnt) == 0 && cnt == S);
	CHECK(d[0].vaddr == 51 && d[1].vaddr == 100 && d[S - 1].vaddr == 100 + S - 2);
	free(d); free(r);
	CHECK(xsknf_gpu_lb_destroy(lb) == 0);
	r = calloc(N - 1, sizeof(B));
	for (uint32_t i = 0; i < N - 1; i++) { r[i].vaddr = 7; r[i].vport = 1; r[i].proto = 17; r[i].addr = 1 + i; r[i].port = 1; }
	CHECK(xsknf_gpu_lb_create(&lb, r, N - 1, 4, 64) == 0);
	o[0].op = o[1].op = XSKNF_GPU_LB_BACKEND_ADD;
	o[0].backend = r[0]; o[0].backend.addr = N;
	o[1].backend = r[0]; o[1].backend.addr = N + 1;
	CHECK(xsknf_gpu_lb_backends_update(lb, o, 2, NULL) == -ENOSPC);        /* 131073 */
	CHECK(xsknf_gpu_lb_backends_update(lb, o, 1, NULL) == 0);              /* exactly 131072 */
	d = calloc(N, sizeof(B));
	CHECK(xsknf_gpu_lb_backends_dump(lb, XSKNF_GPU_LB_HOST_TABLE, d, N - 1, &cnt) == -ENOSPC && cnt == N);
	CHECK(xsknf_gpu_lb_backends_dump(lb, XSKNF_GPU_LB_HOST_TABLE, d, N, &cnt) == 0 && d[N - 1].addr == N && d[0].addr == 1);
	ID *ids = calloc(N, sizeof(ID));
	for (uint32_t i = 0; i < N; i++) { ids[i].addr = i; ids[i].port = 1; ids[i].proto = 17; }
	CHECK(xsknf_gpu_lb_drain_backends_host(lb, ids, N, NULL) == 0);        /* the longest list */
	free(ids); free(d); free(r); free(o);
	CHECK(xsknf_gpu_lb_destroy(lb) == 0);
	return 0;
}

int main(void)
{
	int cs, step = 0;
	uint64_t rebuilds = 0, drained = 0, vanished = 0, replaced = 0;
	for (cs = 0; cs < 300; cs++) {
		if (cs % 100 == 0 && edges(cs)) return 1;
		/* creation: 0..5 records, duplicates among them */
		uint32_t n0 = rnd() % 6;
		B *bk = malloc(sizeof(B) * (n0 ? n0 : 1));
		OP *asops = malloc(sizeof(OP) * (n0 ? n0 : 1));
		for (uint32_t i = 0; i < n0; i++) { bk[i] = small_rec(); asops[i].backend = bk[i]; asops[i].op = XSKNF_GPU_LB_BACKEND_ADD; }
		struct xsknf_gpu_lb *lb = NULL;
		CHECK(xsknf_gpu_lb_create(&lb, n0 ? bk : NULL, n0, MAXS, SLOTS) == 0);
		mn = tombs = nsvc = 0;
		memset(nb, 0, sizeof(nb));
		/* (creation appends every record: duplicates stay) */
		for (uint32_t i = 0; i < n0; i++) {
			int s = svc_at(&bk[i]);
			if (s < 0) { s = (int)nsvc++; nb[s] = 0; }
			ms[s][nb[s]++] = bk[i];
		}
		free(bk); free(asops);
		for (step = 0; step < 40; step++) {
			uint32_t op = rnd() % 10;
			if (op < 4) {   /* update */
				uint32_t n = rnd() % 7;
				OP *ops = malloc(sizeof(OP) * (n ? n : 1));
				for (uint32_t i = 0; i < n; i++) {
					ops[i].backend = small_rec();
					ops[i].op = rnd() % 5 < 2 ? XSKNF_GPU_LB_BACKEND_REMOVE : XSKNF_GPU_LB_BACKEND_ADD;
					if (nsvc && rnd() % 3 == 0) {   /* aimed at a record the model holds */
						uint32_t s = rnd() % nsvc;
						B t = ms[s][rnd() % nb[s]];
						memcpy(t.mac, ops[i].backend.mac, 6);
						t.ifindex = ops[i].backend.ifindex;
						ops[i].backend = t;
						replaced += ops[i].op == XSKNF_GPU_LB_BACKEND_ADD;
					}
				}
				int bad = n && rnd() % 8 == 0;
				if (bad) {   /* nothing may change */
					uint32_t i = rnd() % n;
					if (rnd() & 1) ops[i].op = 2 + (uint32_t)rnd() % 5; else ops[i].backend.proto = 1;
					CHECK(xsknf_gpu_lb_backends_update(lb, ops, n, NULL) == -EINVAL);
				} else {
					uint32_t before = nsvc;
					/* (the model's arrays are large enough: 12 services of 8 backends exist by name, plus creation's duplicates) */
					model_update(ops, n);
					vanished += nsvc < before;
					CHECK(xsknf_gpu_lb_backends_update(lb, n ? ops : NULL, n, NULL) == 0);
				}
				free(ops);
			} else if (op < 6) {   /* a batch; then read the sessions back */
				uint32_t n = 1 + rnd() % 6, must = 0;
				uint8_t *umem = malloc(64 * n);
				struct xsknf_gpu_desc *d = malloc(sizeof(*d) * n);
				int32_t *verd = malloc(sizeof(int32_t) * n);
				for (uint32_t i = 0; i < n; i++) {
					uint8_t *f = umem + 64 * i;
					K k = small_key();
					B as;
					memset(&as, 0, sizeof(as));
					if (rnd() & 1) { k.daddr = 9 + rnd() % 3; k.dport = (uint16_t)(9 + rnd() % 2); }
					as.vaddr = k.daddr; as.vport = k.dport; as.proto = k.proto;
					must += svc_at(&as) >= 0;
					for (int b = 0; b < 64; b++) f[b] = (uint8_t)rnd();
					f[12] = 8; f[13] = 0; f[14] = 0x45; f[23] = k.proto;
					memcpy(f + 26, &k.saddr, 4); memcpy(f + 30, &k.daddr, 4);
					memcpy(f + 34, &k.sport, 2); memcpy(f + 36, &k.dport, 2);
					d[i].addr = 64ull * i; d[i].len = 64; d[i].options = 0;
				}
				uint64_t stats[XSKNF_GPU_LB_STATS];
				CHECK(xsknf_gpu_lb_host(umem, 64 * n, d, n, 1, 4, lb, verd, stats) == 0);
				CHECK(stats[1] >= must && stats[1] + stats[2] == n);
				uint32_t cnt = 0;
				CHECK(xsknf_gpu_lb_sessions_dump(lb, XSKNF_GPU_LB_HOST_TABLE, mk, mv, MAXS, &cnt) == 0);
				CHECK(cnt == mn + stats[4]);
				mn = cnt;
				free(umem); free(d); free(verd);
			} else if (op < 7) {   /* put */
				uint32_t n = rnd() % 5;
				K *k = malloc(sizeof(K) * (n ? n : 1));
				V *v = malloc(sizeof(V) * (n ? n : 1));
				int full = 0;
				for (uint32_t i = 0; i < n; i++) {
					k[i] = small_key();
					memset(&v[i], 0, sizeof(V));
					v[i].addr = 1 + rnd() % 4; v[i].port = (uint16_t)(1 + rnd() % 2); v[i].dir = (uint8_t)(rnd() & 1);
					int j = at(&k[i], mk, mn);
					if (full) continue;
					if (j >= 0) mv[j] = v[i];
					else if (mn == MAXS) full = 1;
					else { mk[mn] = k[i]; mv[mn++] = v[i]; }
				}
				CHECK(xsknf_gpu_lb_sessions_put(lb, n ? k : NULL, n ? v : NULL, n) == (full ? -ENOSPC : 0));
				free(k); free(v);
			} else if (op < 9) {   /* list drain */
				uint32_t n = rnd() % 12;
				ID *ids = malloc(sizeof(ID) * (n ? n : 1));
				uint64_t *res = malloc(sizeof(uint64_t) * XSKNF_GPU_LB_REMOVE_RESULT), want = 0, compacted = 0;
				uint32_t w = 0;
				res[0] = res[1] = 77;
				for (uint32_t i = 0; i < n; i++) {
					ids[i].addr = 1 + rnd() % 4; ids[i].port = (uint16_t)(1 + rnd() % 2); ids[i].proto = rnd() & 1 ? 6 : 17;
					ids[i].pad = (uint8_t)rnd();
					if (i && rnd() % 4 == 0) ids[i] = ids[rnd() % i];   /* a duplicate */
				}
				for (uint32_t i = 0; i < mn; i++) {
					int hit = 0;
					for (uint32_t j = 0; j < n; j++)
						hit |= mk[i].proto == ids[j].proto &&
						       (mv[i].dir == XSKNF_GPU_LB_TO_BACKEND ? mv[i].addr == ids[j].addr && mv[i].port == ids[j].port
						                                              : mk[i].saddr == ids[j].addr && mk[i].sport == ids[j].port);
					if (hit) { ++want; continue; }
					mk[w] = mk[i];
					mv[w++] = mv[i];
				}
				mn = w;
				tombs += (uint32_t)want;
				if (tombs > SLOTS / 4) { tombs = 0; compacted = 1; }
				CHECK(xsknf_gpu_lb_drain_backends_host(lb, n ? ids : NULL, n, res) == 0);
				CHECK(res[XSKNF_GPU_LB_REMOVED] == want && res[XSKNF_GPU_LB_COMPACTED] == compacted);
				rebuilds += compacted;
				drained += want;
				free(ids); free(res);
			}
			/* both dumps are the model */
			struct xsknf_gpu_lb_info info;
			const uint32_t total = model_total();
			CHECK(xsknf_gpu_lb_info(lb, &info) == 0 && info.host_sessions == mn && info.services == nsvc && info.backends == total);
			uint32_t cnt = 0;
			B *db = malloc(sizeof(B) * (total ? total : 1));
			if (total) CHECK(xsknf_gpu_lb_backends_dump(lb, XSKNF_GPU_LB_HOST_TABLE, db, total - 1, &cnt) == -ENOSPC && cnt == total);
			CHECK(xsknf_gpu_lb_backends_dump(lb, XSKNF_GPU_LB_HOST_TABLE, total ? db : NULL, total, &cnt) == 0 && cnt == total);
			for (uint32_t i = 0; i < total;) {
				int s = svc_at(&db[i]);
				CHECK(s >= 0 && i + nb[s] <= total && (i == 0 || svc_less(&db[i - 1], &db[i])));
				for (uint32_t k = 0; k < nb[s]; k++) {
					B want = ms[s][k];
					CHECK(same_rec(&db[i + k], &want) && db[i + k].pad == 0 && db[i + k].pad2[0] == 0 && db[i + k].pad2[1] == 0);
				}
				i += nb[s];
			}
			free(db);
			K *dk = malloc(sizeof(K) * (mn ? mn : 1));
			V *dv = malloc(sizeof(V) * (mn ? mn : 1));
			CHECK(xsknf_gpu_lb_sessions_dump(lb, XSKNF_GPU_LB_HOST_TABLE, dk, dv, mn, &cnt) == 0 && cnt == mn);
			for (uint32_t i = 0; i < cnt; i++) {
				int j = at(&dk[i], mk, mn);
				CHECK(j >= 0 && mv[j].addr == dv[i].addr && mv[j].port == dv[i].port && mv[j].dir == dv[i].dir);
			}
			free(dk); free(dv);
		}
		uint32_t none = 0;
		CHECK(xsknf_gpu_lb_backends_dump(lb, XSKNF_GPU_LB_DEVICE_TABLE, NULL, 0, &none) == -ENODEV);
		CHECK(xsknf_gpu_lb_drain_backends(lb, NULL, 0, NULL, NULL) == -ENODEV);
		CHECK(xsknf_gpu_lb_destroy(lb) == 0);
	}
	if (rebuilds < 20 || drained < 300 || vanished < 100 || replaced < 300) {
		fprintf(stderr, "too few rebuilds (%llu), drained sessions (%llu), vanished services (%llu) or replaced records (%llu)\n",
		        (unsigned long long)rebuilds, (unsigned long long)drained, (unsigned long long)vanished,
		        (unsigned long long)replaced);
		return 1;
	}
	printf("ok %d\n", cs);
	return 0;
}

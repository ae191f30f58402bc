/*
 * san_acl_update.c -- xsknf_gpu_acl_update and xsknf_gpu_acl_dump
 * (xsknf_amd/csrc/acl.cpp, built with XSKNF_ACL_HOST_ONLY: no GPU call) under
 * AddressSanitizer + UBSan, with xsknf_gpu_firewall_host (firewall_host.cpp) as
 * the lookup.  The model is open-coded: an array of the universe's keys with a
 * live flag and an action.  Cases: churn on 64 slots (17 keys deleted and 17
 * others put, over and over: the rebuild in place fires again and again),
 * capacity (slots - 1 live keys: one more is refused and leaves no trace, a
 * replace and a swap succeed), and random ops in calls of random size on tables
 * of 64 to 1024 slots, a bad op or a protocol the table never holds among them.
 * Every ops, rule and frame buffer is a heap block of exactly its size.  After
 * every call the dump must be the model's live keys, ascending, and every key of
 * the universe must look up as the model says.  Prints "ok <calls>".  CPU only
 * (tests/test_acl_update_san.py builds and runs it).
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

static int calls;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "call %d: %s failed (line %d)\n", calls, #c, __LINE__); return 1; } } while (0)

#define MAXU 1100

struct model {
	struct xsknf_gpu_acl_rule key[MAXU];   /* the universe; action = the live key's action */
	int live[MAXU];
	uint32_t n;
};

static void universe(struct model *m, uint32_t n)
{
	memset(m, 0, sizeof(*m));
	m->n = n;
	for (uint32_t i = 0; i < n; i++) {
		m->key[i].saddr = (uint32_t)rnd();
		m->key[i].daddr = i;   /* distinct */
		m->key[i].sport = (uint16_t)rnd();
		m->key[i].dport = (uint16_t)rnd();
		m->key[i].proto = rnd() % 2 ? 6 : 17;
	}
}

static int before(const struct xsknf_gpu_acl_rule *x, const struct xsknf_gpu_acl_rule *y)
{
	const uint32_t xc = x->sport | (uint32_t)x->dport << 16, yc = y->sport | (uint32_t)y->dport << 16;
	if (x->saddr != y->saddr)
		return x->saddr < y->saddr;
	if (x->daddr != y->daddr)
		return x->daddr < y->daddr;
	if (xc != yc)
		return xc < yc;
	return x->proto < y->proto;
}

/* the dump and every key's lookup against the model */
static int verify(const struct xsknf_gpu_acl *acl, const struct model *m)
{
	uint32_t live = 0, n = 0;
	for (uint32_t i = 0; i < m->n; i++)
		live += m->live[i];
	struct xsknf_gpu_acl_info info;
	CHECK(xsknf_gpu_acl_info(acl, &info) == 0 && info.rules == live && info.rules + info.tombstones < info.slots);
	CHECK(info.tombstones <= info.slots / 4 && info.max_probe <= info.rules + info.tombstones);
	CHECK((live == 0) == (info.max_probe == 0));
	struct xsknf_gpu_acl_rule *out = malloc(sizeof(*out) * (live ? live : 1));
	CHECK(out);
	if (live) {
		struct xsknf_gpu_acl_rule *small = malloc(sizeof(*small) * (live - 1 ? live - 1 : 1));
		CHECK(small && xsknf_gpu_acl_dump(acl, XSKNF_GPU_ACL_HOST_TABLE, small, live - 1, &n) == -28 && n == live);
		free(small);
	}
	CHECK(xsknf_gpu_acl_dump(acl, XSKNF_GPU_ACL_HOST_TABLE, out, live, &n) == 0 && n == live);
	CHECK(xsknf_gpu_acl_dump(acl, XSKNF_GPU_ACL_DEVICE_TABLE, out, live, &n) == -19);
	for (uint32_t i = 0; i < live; i++) {
		CHECK(i == 0 || before(&out[i - 1], &out[i]));
		const uint32_t u = out[i].daddr;
		CHECK(u < m->n && m->live[u] && out[i].saddr == m->key[u].saddr && out[i].sport == m->key[u].sport &&
		      out[i].dport == m->key[u].dport && out[i].proto == m->key[u].proto && out[i].action == m->key[u].action);
		CHECK(!out[i].pad[0] && !out[i].pad[1] && !out[i].pad[2]);
	}
	free(out);
	/* one 64-byte frame per key of the universe, the last on the UMEM's last byte */
	const uint32_t nf = m->n;
	uint8_t *umem = malloc(64 * (size_t)nf);
	struct xsknf_gpu_desc *d = malloc(sizeof(*d) * nf);
	int32_t *v = malloc(sizeof(*v) * nf);
	CHECK(umem && d && v);
	for (uint32_t i = 0; i < nf; i++) {
		uint8_t *f = umem + 64 * (size_t)i;
		for (int b = 0; b < 64; b++)
			f[b] = (uint8_t)rnd();
		f[12] = 8; f[13] = 0; f[14] = 0x45; f[23] = m->key[i].proto;
		memcpy(f + 26, &m->key[i].saddr, 4);
		memcpy(f + 30, &m->key[i].daddr, 4);
		memcpy(f + 34, &m->key[i].sport, 2);
		memcpy(f + 36, &m->key[i].dport, 2);
		d[i].addr = 64 * (uint64_t)i;
		d[i].len = 64;
		d[i].options = 0;
	}
	CHECK(xsknf_gpu_firewall_host(umem, 64 * (uint64_t)nf, d, nf, acl, v) == 0);
	for (uint32_t i = 0; i < nf; i++)
		CHECK(v[i] == (m->live[i] ? m->key[i].action : 0));
	free(v);
	free(d);
	free(umem);
	return 0;
}

/* one call of n ops (an exact heap block) drawn by pick(); returns the call's rc */
static int update(struct xsknf_gpu_acl *acl, struct model *m, uint32_t n, const uint32_t *who, const uint32_t *op,
		  int expect)
{
	struct xsknf_gpu_acl_op *ops = malloc(sizeof(*ops) * (n ? n : 1));
	struct model *after = malloc(sizeof(*after));
	CHECK(ops && after);
	*after = *m;
	for (uint32_t i = 0; i < n; i++) {
		memset(&ops[i], 0x5a, sizeof(ops[i]));
		ops[i].rule = m->key[who[i]];
		ops[i].rule.action = (int32_t)(rnd() % 40) - 1;
		ops[i].op = op[i];
		if (op[i] == XSKNF_GPU_ACL_PUT) {
			after->live[who[i]] = 1;
			after->key[who[i]].action = ops[i].rule.action;
		} else {
			after->live[who[i]] = 0;
		}
	}
	const int rc = xsknf_gpu_acl_update(acl, n ? ops : NULL, n, NULL);
	calls++;
	CHECK(rc == expect);
	if (rc == 0)
		*m = *after;
	free(after);
	free(ops);
	return verify(acl, m);
}

static int churn(void)
{
	struct model *m = malloc(sizeof(*m));
	uint32_t who[34], op[34];
	struct xsknf_gpu_acl *acl = NULL;
	CHECK(m);
	universe(m, 47 + 17 * 3);
	struct xsknf_gpu_acl_rule *init = malloc(sizeof(*init) * 47);
	CHECK(init);
	for (uint32_t i = 0; i < 47; i++) {
		m->live[i] = 1;
		m->key[i].action = (int32_t)i - 1;
		init[i] = m->key[i];
	}
	CHECK(xsknf_gpu_acl_create(&acl, init, 47, 64) == 0);
	free(init);
	CHECK(verify(acl, m) == 0);
	/* sets of 17 keys: 30..46 live at first, then each round deletes the live set and puts the next */
	for (int round = 0; round < 40; round++) {
		const uint32_t out = 30 + 17 * (round % 4), in = 30 + 17 * ((round + 1) % 4);
		for (uint32_t i = 0; i < 17; i++) {
			who[i] = out + i; op[i] = XSKNF_GPU_ACL_DELETE;
			who[17 + i] = in + i; op[17 + i] = XSKNF_GPU_ACL_PUT;
		}
		if (round % 2) {   /* as two calls: the deletes alone pass the bound, tombstones drop to 0 */
			struct xsknf_gpu_acl_info info;
			CHECK(update(acl, m, 17, who, op, 0) == 0);
			CHECK(xsknf_gpu_acl_info(acl, &info) == 0 && info.tombstones == 0);
			CHECK(update(acl, m, 17, who + 17, op + 17, 0) == 0);
		} else {
			CHECK(update(acl, m, 34, who, op, 0) == 0);
		}
	}
	CHECK(xsknf_gpu_acl_destroy(acl) == 0);
	free(m);
	return 0;
}

static int capacity(void)
{
	struct model *m = malloc(sizeof(*m));
	uint32_t who[4], op[4];
	struct xsknf_gpu_acl *acl = NULL;
	CHECK(m);
	universe(m, 70);
	struct xsknf_gpu_acl_rule *init = malloc(sizeof(*init) * 63);
	CHECK(init);
	for (uint32_t i = 0; i < 63; i++) {
		m->live[i] = 1;
		m->key[i].action = (int32_t)i;
		init[i] = m->key[i];
	}
	CHECK(xsknf_gpu_acl_create(&acl, init, 63, 64) == 0);
	free(init);
	who[0] = 65; op[0] = XSKNF_GPU_ACL_PUT;
	CHECK(update(acl, m, 1, who, op, -28) == 0);             /* one more new key */
	who[0] = 5;
	CHECK(update(acl, m, 1, who, op, 0) == 0);               /* a replace at full capacity */
	who[0] = 6; who[1] = 66; op[1] = XSKNF_GPU_ACL_PUT;
	CHECK(update(acl, m, 2, who, op, -28) == 0);             /* nothing of a refused call is kept */
	who[0] = 7; op[0] = XSKNF_GPU_ACL_DELETE;
	CHECK(update(acl, m, 2, who, op, 0) == 0);               /* one out, one in */
	who[0] = 67; op[0] = XSKNF_GPU_ACL_PUT; who[1] = 67; op[1] = XSKNF_GPU_ACL_DELETE;
	CHECK(update(acl, m, 2, who, op, 0) == 0);               /* put and deleted again: nothing more at the end */
	who[0] = 8; op[0] = 2;
	CHECK(update(acl, m, 1, who, op, -22) == 0);
	CHECK(update(acl, m, 0, who, op, 0) == 0);
	CHECK(xsknf_gpu_acl_update(NULL, NULL, 0, NULL) == -22 && xsknf_gpu_acl_update(acl, NULL, 1, NULL) == -22);
	CHECK(xsknf_gpu_acl_destroy(acl) == 0);
	free(m);
	return 0;
}

static int random_ops(void)
{
	static const uint32_t slot_choices[4] = {64, 128, 256, 1024};
	struct model *m = malloc(sizeof(*m));
	CHECK(m);
	for (int t = 0; t < 12; t++) {
		const uint32_t slots = slot_choices[t % 4];
		/* a universe that fits (t even) or overflows the table now and then (t odd) */
		const uint32_t nu = t % 2 ? slots + slots / 16 : slots - slots / 4;
		struct xsknf_gpu_acl *acl = NULL;
		universe(m, nu);
		CHECK(xsknf_gpu_acl_create(&acl, NULL, 0, slots) == 0);
		for (int c = 0; c < 60; c++) {
			const uint32_t n = (uint32_t)(rnd() % (c % 7 == 0 ? 3 : slots / 2));
			uint32_t *who = malloc(sizeof(*who) * (n ? n : 1)), *op = malloc(sizeof(*op) * (n ? n : 1));
			CHECK(who && op);
			const uint32_t del_share = 2 + (uint32_t)(rnd() % 5);
			for (uint32_t i = 0; i < n; i++) {
				who[i] = (uint32_t)(rnd() % nu);
				op[i] = rnd() % 8 < del_share ? XSKNF_GPU_ACL_DELETE : XSKNF_GPU_ACL_PUT;
			}
			/* what the model says the map would hold */
			int *live = malloc(sizeof(*live) * nu);
			CHECK(live);
			memcpy(live, m->live, sizeof(*live) * nu);
			for (uint32_t i = 0; i < n; i++)
				live[who[i]] = op[i] == XSKNF_GPU_ACL_PUT;
			uint32_t count = 0;
			for (uint32_t i = 0; i < nu; i++)
				count += (uint32_t)live[i];
			free(live);
			int expect = count >= slots ? -28 : 0;
			if (n && c % 13 == 5) {
				op[rnd() % n] = 7;
				expect = -22;
			}
			CHECK(update(acl, m, n, who, op, expect) == 0);
			free(op);
			free(who);
		}
		/* a protocol the table never holds: the PUT is left out, the DELETE does nothing */
		struct xsknf_gpu_acl_op odd[2];
		memset(odd, 0, sizeof(odd));
		odd[0].rule = m->key[0];
		odd[0].rule.proto = 1;
		odd[0].op = XSKNF_GPU_ACL_PUT;
		odd[1] = odd[0];
		odd[1].op = XSKNF_GPU_ACL_DELETE;
		CHECK(xsknf_gpu_acl_update(acl, odd, 1, NULL) == 0 && xsknf_gpu_acl_update(acl, odd + 1, 1, NULL) == 0);
		calls += 2;
		CHECK(verify(acl, m) == 0);
		CHECK(xsknf_gpu_acl_destroy(acl) == 0);
	}
	free(m);
	return 0;
}

int main(void)
{
	if (churn() || capacity() || random_ops())
		return 1;
	printf("ok %d\n", calls);
	return 0;
}

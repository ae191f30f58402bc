/*
 * san_acl_counters.c -- the ACL's hit counters on the host
 * (xsknf_gpu_acl_counters_enable / _dump / _clear: xsknf_amd/csrc/acl.cpp built
 * with XSKNF_ACL_HOST_ONLY, no GPU call; the counting in firewall_host.cpp)
 * under AddressSanitizer + UBSan.  The model is open-coded: the universe's keys,
 * each with a live flag, an action and its packets and bytes, and four totals.
 * On tables of 64 to 1024 slots: random calls of random size -- puts, replaces
 * and deletes, the same key several times in a call, so that rebuilds past the
 * tombstone bound and for want of an empty slot come again and again -- with a
 * batch between them: frames of the universe's keys (a few take most), of keys
 * nobody holds, frames too short to reach the map and descriptors outside the
 * UMEM.  Now and then the set is cleared.  After every step the dump must be the
 * model's live keys, ascending, with the model's counters and totals.  Every
 * ops, rule, counter, descriptor, verdict and frame buffer is a heap block of
 * exactly its size.  Prints "ok <steps>".  CPU only
 * (tests/test_acl_counters_san.py builds and runs it).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "xsknf_gpu.h"

static uint64_t st = 0xD1B54A32D192ED03ULL;
static uint64_t rnd(void)
{
	st ^= st >> 12;
	st ^= st << 25;
	st ^= st >> 27;
	return st * 0x2545F4914F6CDD1DULL;
}

static int steps;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "step %d: %s failed (line %d)\n", steps, #c, __LINE__); return 1; } } while (0)

#define MAXU 1100

struct model {
	struct xsknf_gpu_acl_rule key[MAXU];   /* the universe; action = the live key's action */
	int live[MAXU];
	uint64_t packets[MAXU], bytes[MAXU];
	uint64_t totals[XSKNF_GPU_ACL_TOTALS];
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

static int verify(const struct xsknf_gpu_acl *acl, const struct model *m)
{
	uint32_t live = 0, n = 0;
	uint64_t hits = 0;
	for (uint32_t i = 0; i < m->n; i++)
		live += (uint32_t)m->live[i];
	struct xsknf_gpu_acl_rule *out = malloc(sizeof(*out) * (live ? live : 1));
	struct xsknf_gpu_acl_counter *ctr = malloc(sizeof(*ctr) * (live ? live : 1));
	uint64_t *tot = malloc(sizeof(*tot) * XSKNF_GPU_ACL_TOTALS);
	CHECK(out && ctr && tot);
	if (live) {
		struct xsknf_gpu_acl_rule *small = malloc(sizeof(*small) * (live - 1 ? live - 1 : 1));
		struct xsknf_gpu_acl_counter *csmall = malloc(sizeof(*csmall) * (live - 1 ? live - 1 : 1));
		CHECK(small && csmall);
		CHECK(xsknf_gpu_acl_counters_dump(acl, XSKNF_GPU_ACL_HOST_TABLE, small, csmall, live - 1, &n, NULL) == -28 && n == live);
		free(small);
		free(csmall);
	}
	CHECK(xsknf_gpu_acl_counters_dump(acl, XSKNF_GPU_ACL_HOST_TABLE, out, ctr, live, &n, tot) == 0 && n == live);
	CHECK(xsknf_gpu_acl_counters_dump(acl, XSKNF_GPU_ACL_DEVICE_TABLE, out, ctr, live, &n, tot) == -19);
	for (uint32_t i = 0; i < live; i++) {
		const uint32_t u = out[i].daddr;
		CHECK(u < m->n && m->live[u] && out[i].saddr == m->key[u].saddr && out[i].action == m->key[u].action);
		CHECK(i == 0 || out[i - 1].saddr < out[i].saddr || (out[i - 1].saddr == out[i].saddr && out[i - 1].daddr < out[i].daddr));
		CHECK(ctr[i].packets == m->packets[u] && ctr[i].bytes == m->bytes[u]);
		hits += ctr[i].packets;
	}
	for (int t = 0; t < XSKNF_GPU_ACL_TOTALS; t++)
		CHECK(tot[t] == m->totals[t]);
	CHECK(tot[0] == tot[1] + tot[2] + tot[3] && hits <= tot[1]);
	free(tot);
	free(ctr);
	free(out);
	return 0;
}

/* one batch of nf frames, each in a heap UMEM that ends on the last frame's last byte */
static int batch(const struct xsknf_gpu_acl *acl, struct model *m, uint32_t nf)
{
	uint64_t size = 0;
	uint32_t *len = malloc(sizeof(*len) * (nf ? nf : 1)), *who = malloc(sizeof(*who) * (nf ? nf : 1));
	CHECK(len && who);
	for (uint32_t i = 0; i < nf; i++) {
		const uint32_t kind = (uint32_t)(rnd() % 16);
		/* 0: too short for the map; 1: outside; 2, 3: a key nobody holds; else a key of the universe, skewed */
		who[i] = kind < 2 ? m->n + kind : kind < 4 ? m->n + 2 : (uint32_t)(rnd() % (rnd() % 4 ? 8 : m->n));
		len[i] = kind == 0 ? (uint32_t)(rnd() % 34) : 54 + (uint32_t)(rnd() % 40);
		size += len[i];
	}
	uint8_t *umem = malloc(size ? size : 1);
	struct xsknf_gpu_desc *d = malloc(sizeof(*d) * (nf ? nf : 1));
	int32_t *v = malloc(sizeof(*v) * (nf ? nf : 1));
	CHECK(umem && d && v);
	uint64_t pos = 0;
	for (uint32_t i = 0; i < nf; i++) {
		uint8_t *f = umem + pos;
		for (uint32_t b = 0; b < len[i]; b++)
			f[b] = (uint8_t)rnd();
		d[i].addr = pos;
		d[i].len = len[i];
		d[i].options = 0;
		int32_t want = 0;
		m->totals[0]++;
		if (who[i] == m->n + 1) {   /* one byte past the end */
			d[i].addr = size - len[i] + 1;
			want = -1;
			m->totals[3]++;
		} else if (who[i] == m->n) {
			if (len[i] >= 14) {
				f[12] = 8; f[13] = 0;
			}
			want = -1;
			m->totals[3]++;
		} else {
			struct xsknf_gpu_acl_rule k;
			if (who[i] < m->n) {
				k = m->key[who[i]];
			} else {
				memset(&k, 0, sizeof(k));
				k.saddr = (uint32_t)rnd();
				k.daddr = m->n + (uint32_t)(rnd() % 1000);   /* no key of the universe */
				k.proto = 6;
			}
			f[12] = 8; f[13] = 0; f[14] = 0x45; f[23] = k.proto;
			memcpy(f + 26, &k.saddr, 4);
			memcpy(f + 30, &k.daddr, 4);
			memcpy(f + 34, &k.sport, 2);
			memcpy(f + 36, &k.dport, 2);
			if (who[i] < m->n && m->live[who[i]]) {
				want = k.action;
				m->packets[who[i]]++;
				m->bytes[who[i]] += len[i];
				m->totals[1]++;
			} else {
				m->totals[2]++;
			}
		}
		v[i] = want;   /* kept in who[] below: v is the call's output */
		who[i] = (uint32_t)want;
		pos += len[i];
	}
	CHECK(xsknf_gpu_firewall_host(umem, size, d, nf, acl, v) == 0);
	for (uint32_t i = 0; i < nf; i++)
		CHECK(v[i] == (int32_t)who[i]);
	steps++;
	free(v);
	free(d);
	free(umem);
	free(who);
	free(len);
	return verify(acl, m);
}

/* one call of n random ops over the universe, in an exact heap block */
static int update(struct xsknf_gpu_acl *acl, struct model *m, uint32_t n, uint32_t slots)
{
	struct xsknf_gpu_acl_op *ops = malloc(sizeof(*ops) * (n ? n : 1));
	struct model *after = malloc(sizeof(*after));
	CHECK(ops && after);
	*after = *m;
	const uint32_t del_share = 2 + (uint32_t)(rnd() % 5);
	for (uint32_t i = 0; i < n; i++) {
		const uint32_t u = (uint32_t)(rnd() % m->n);
		memset(&ops[i], 0x5a, sizeof(ops[i]));
		ops[i].rule = m->key[u];
		ops[i].rule.action = (int32_t)(rnd() % 40) - 1;
		ops[i].op = rnd() % 8 < del_share ? XSKNF_GPU_ACL_DELETE : XSKNF_GPU_ACL_PUT;
		if (ops[i].op == XSKNF_GPU_ACL_PUT) {
			if (!after->live[u])
				after->packets[u] = after->bytes[u] = 0;   /* a new rule */
			after->live[u] = 1;
			after->key[u].action = ops[i].rule.action;
		} else {
			after->live[u] = 0;
			after->packets[u] = after->bytes[u] = 0;
		}
	}
	uint32_t count = 0;
	for (uint32_t i = 0; i < m->n; i++)
		count += (uint32_t)after->live[i];
	const int rc = xsknf_gpu_acl_update(acl, n ? ops : NULL, n, NULL);
	steps++;
	CHECK(rc == (count >= slots ? -28 : 0));
	if (rc == 0)
		*m = *after;
	free(after);
	free(ops);
	return verify(acl, m);
}

int main(void)
{
	static const uint32_t slot_choices[4] = {64, 128, 256, 1024};
	struct model *m = malloc(sizeof(*m));
	uint32_t n = 0;
	CHECK(m);
	CHECK(xsknf_gpu_acl_counters_enable(NULL) == -22 && xsknf_gpu_acl_counters_clear(NULL, 0, NULL) == -22);
	for (int t = 0; t < 8; t++) {
		const uint32_t slots = slot_choices[t % 4];
		const uint32_t nu = t % 2 ? slots + slots / 16 : slots - slots / 4;
		struct xsknf_gpu_acl *acl = NULL;
		universe(m, nu);
		CHECK(xsknf_gpu_acl_create(&acl, NULL, 0, slots) == 0);
		CHECK(xsknf_gpu_acl_counters_dump(acl, XSKNF_GPU_ACL_HOST_TABLE, NULL, NULL, 0, &n, NULL) == -22);
		CHECK(xsknf_gpu_acl_counters_clear(acl, XSKNF_GPU_ACL_HOST_TABLE, NULL) == -22);
		CHECK(xsknf_gpu_acl_counters_enable(acl) == 0 && xsknf_gpu_acl_counters_enable(acl) == 0);
		CHECK(xsknf_gpu_acl_counters_dump(acl, 2, NULL, NULL, 0, &n, NULL) == -22);
		CHECK(xsknf_gpu_acl_counters_dump(acl, XSKNF_GPU_ACL_HOST_TABLE, NULL, NULL, 0, NULL, NULL) == -22);
		CHECK(xsknf_gpu_acl_counters_clear(acl, XSKNF_GPU_ACL_DEVICE_TABLE, NULL) == -19);
		for (int c = 0; c < 40; c++) {
			CHECK(update(acl, m, (uint32_t)(rnd() % (c % 7 == 0 ? 3 : slots / 2)), slots) == 0);
			CHECK(batch(acl, m, (uint32_t)(rnd() % (c % 5 == 0 ? 2 : 300))) == 0);
			if (c % 11 == 10) {
				CHECK(xsknf_gpu_acl_counters_clear(acl, XSKNF_GPU_ACL_HOST_TABLE, NULL) == 0);
				memset(m->packets, 0, sizeof(m->packets));
				memset(m->bytes, 0, sizeof(m->bytes));
				memset(m->totals, 0, sizeof(m->totals));
				steps++;
				CHECK(verify(acl, m) == 0);
			}
		}
		CHECK(xsknf_gpu_acl_destroy(acl) == 0);
	}
	free(m);
	printf("ok %d\n", steps);
	return 0;
}

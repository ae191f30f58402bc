/*
 * san_lbfw.c -- the lbfw NF's host model (xsknf_amd/csrc/lbfw_host.cpp:
 * xsknf_gpu_lbfw_host) with the objects it works on (acl.cpp built with
 * XSKNF_ACL_HOST_ONLY, lb.cpp with XSKNF_LB_HOST_ONLY: no GPU call) and
 * lb_host.cpp under AddressSanitizer + UBSan.  Every UMEM, descriptor array,
 * verdict array and rule array is a heap block of exactly its size, so a read
 * or write past a frame at the UMEM's end, past n verdicts or past the ACL's
 * last slot is a heap overflow.  Cases: random services and session tables as
 * in san_lb.c, ACLs from no rule (and a single slot) to a table with one empty
 * slot, rules that are the frames' own keys (actions 0, -1, positive, INT32
 * extremes), one-bit neighbours and unrelated ones, frames of every length
 * 0..120 with every ihl, the last frame ending on the UMEM's last byte,
 * descriptors outside the UMEM, num_interfaces 1..4 and 0 (-EINVAL, nothing
 * written), acl NULL, lbfw and lb calls alternating on one object.  Checked:
 * [0] = [1] + [2] + [3] + [7], a frame whose key the ACL holds has the rule's
 * action and its bytes unchanged, every other verdict is -1, PASS or an ifindex
 * that exists, the session count never exceeds max_sessions; prints
 * "ok <cases>".  CPU only (tests/test_lbfw_san.py builds and runs it).
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

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "case %d: %s failed (line %d)\n", cs, #c, __LINE__); return 1; } } while (0)

static const int32_t acts[] = { 0, -1, 1, 3, INT32_MAX, INT32_MIN, 0, 2 };

/* the key the parse reads from f, 1 if it reaches the gate */
static int key_of(const uint8_t *f, uint32_t len, struct xsknf_gpu_acl_rule *r)
{
	if (len < 34 || f[12] != 8 || f[13] != 0) return 0;
	uint32_t next = 14 + 4 * (f[14] & 15u);
	if (f[23] != 6 && f[23] != 17) return 0;
	if (next + (f[23] == 6 ? 20u : 8u) > len) return 0;
	memset(r, 0, sizeof(*r));
	memcpy(&r->saddr, f + 26, 4);
	memcpy(&r->daddr, f + 30, 4);
	memcpy(&r->sport, f + next, 2);
	memcpy(&r->dport, f + next + 2, 2);
	r->proto = f[23];
	return 1;
}

int main(void)
{
	int cs;
	for (cs = 0; cs < 400; cs++) {
		uint32_t nb = rnd() % 12, nsvc = 1 + rnd() % 3, maxs = cs % 5 == 0 ? rnd() % 4 : 4 + rnd() % 60;
		struct xsknf_gpu_lb_backend *bk = malloc(sizeof(*bk) * (nb ? nb : 1));
		memset(bk, 0, sizeof(*bk) * (nb ? nb : 1));
		for (uint32_t i = 0; i < nb; i++) {
			uint32_t s = rnd() % nsvc;
			bk[i].vaddr = 0x0a000001 + s;
			bk[i].vport = (uint16_t)(0x5000 + s);
			bk[i].proto = s & 1 ? 6 : 17;
			bk[i].addr = (uint32_t)rnd();
			bk[i].port = (uint16_t)rnd();
			for (int k = 0; k < 6; k++) bk[i].mac[k] = (uint8_t)rnd();
			bk[i].ifindex = (uint16_t)(rnd() % 4);
		}
		struct xsknf_gpu_lb *lb = NULL;
		CHECK(xsknf_gpu_lb_create(&lb, nb ? bk : NULL, nb, maxs, cs % 3 == 0 ? 128 : 0) == 0);

		uint32_t n = rnd() % 70;
		uint32_t *lens = malloc(sizeof(uint32_t) * (n + 1)), total = 0;
		for (uint32_t i = 0; i < n; i++) {
			lens[i] = rnd() % 4 ? 34 + rnd() % 87 : rnd() % 121;
			total += lens[i];
		}
		uint8_t *umem = malloc(total ? total : 1), *before = malloc(total ? total : 1);
		struct xsknf_gpu_desc *d = malloc(sizeof(*d) * (n ? n : 1));
		struct xsknf_gpu_lb_session_key *pk = malloc(sizeof(*pk) * (n ? n : 1));
		struct xsknf_gpu_lb_session_value *pv = malloc(sizeof(*pv) * (n ? n : 1));
		/* the ACL: up to one rule per frame (its key, a neighbour or noise); held[i]: frame i's key is a rule */
		struct xsknf_gpu_acl_rule *rules = malloc(sizeof(*rules) * (n ? n : 1));
		int32_t *held = malloc(sizeof(int32_t) * (n ? n : 1));
		uint8_t *is_held = malloc(n ? n : 1);
		uint32_t npre = 0, nrules = 0, pos = 0;
		for (uint32_t i = 0; i < total; i++) umem[i] = (uint8_t)rnd();
		for (uint32_t i = 0; i < n; i++) {
			uint32_t len = lens[i], ihl = rnd() % 16, next = 14 + 4 * ihl;
			uint8_t *f = umem + pos;
			is_held[i] = 0;
			if (len >= 14 && rnd() % 8) { f[12] = 8; f[13] = 0; }
			if (len > 23) { f[14] = (uint8_t)(f[14] & 0xf0) | (uint8_t)ihl; f[23] = rnd() % 6 ? (rnd() & 1 ? 6 : 17) : 1; }
			if (len >= 34 && nb && rnd() % 2) {   /* towards a service */
				const struct xsknf_gpu_lb_backend *b = &bk[rnd() % nb];
				memcpy(f + 30, &b->vaddr, 4);
				f[23] = b->proto;
				if (next + 4 <= len) memcpy(f + next + 2, &b->vport, 2);
			}
			if (len >= 34 && next + 4 <= len && rnd() % 4 == 0 && (f[23] == 6 || f[23] == 17)) {   /* a stored session */
				memset(&pk[npre], 0, sizeof(*pk));
				memset(&pv[npre], 0, sizeof(*pv));
				memcpy(&pk[npre].saddr, f + 26, 4);
				memcpy(&pk[npre].daddr, f + 30, 4);
				memcpy(&pk[npre].sport, f + next, 2);
				memcpy(&pk[npre].dport, f + next + 2, 2);
				pk[npre].proto = f[23];
				pv[npre].addr = (uint32_t)rnd();
				pv[npre].port = (uint16_t)rnd();
				pv[npre].ifindex = (uint16_t)(rnd() % 4);
				pv[npre].dir = (uint8_t)(rnd() & 1);
				npre++;
			}
			uint64_t o = rnd() % ((pos < 0xffff ? pos : 0xffff) + 1);
			d[i].addr = (pos - o) | o << 48;
			d[i].len = len;
			d[i].options = (uint32_t)rnd();
			int outside = rnd() % 9 == 0;
			struct xsknf_gpu_acl_rule r;
			if (!outside && cs % 7 != 0 && key_of(f, len, &r)) {
				uint32_t how = rnd() % 3;
				if (how == 1) r.saddr ^= 1u << (rnd() % 32);          /* a neighbour */
				if (how < 2) {
					r.action = acts[rnd() % 8];
					rules[nrules++] = r;
				}
				if (how == 0) { is_held[i] = 1; held[i] = r.action; }
			}
			if (outside) { d[i].addr = rnd() % 3 ? total - len / 2 : 1ull << 47; if (len < 2) d[i].addr = total + 1ull; }
			pos += len;   /* back to back: the last frame ends on the UMEM's last byte */
		}
		/* a later rule of the same key wins, and a neighbour may be another frame's key: settle held[] by the table's own order */
		for (uint32_t i = 0, p = 0; i < n; p += lens[i], i++) {
			struct xsknf_gpu_acl_rule r;
			uint64_t off = (d[i].addr & ((1ull << 48) - 1)) + (d[i].addr >> 48);
			if (off != p || !key_of(umem + p, lens[i], &r)) { is_held[i] = 0; continue; }
			is_held[i] = 0;
			for (uint32_t k = 0; k < nrules; k++)
				if (rules[k].saddr == r.saddr && rules[k].daddr == r.daddr && rules[k].sport == r.sport &&
				    rules[k].dport == r.dport && rules[k].proto == r.proto) { is_held[i] = 1; held[i] = rules[k].action; }
		}
		/* slots: the default, a table with exactly one empty slot, or (no rule) a single slot */
		uint32_t slots = 0;
		if (nrules == 0 && cs % 2) slots = 1;
		struct xsknf_gpu_acl *acl = NULL;
		CHECK(xsknf_gpu_acl_create(&acl, nrules ? rules : NULL, nrules, slots) == 0);
		struct xsknf_gpu_acl_info ai;
		CHECK(xsknf_gpu_acl_info(acl, &ai) == 0 && ai.device_bytes == 0 && ai.rules <= nrules);
		if (nrules && cs % 4 == 1) {   /* rebuild as full as a table may be */
			uint32_t full = 1;
			while (full <= ai.rules) full *= 2;
			if (full == ai.rules + 1) {
				CHECK(xsknf_gpu_acl_destroy(acl) == 0);
				CHECK(xsknf_gpu_acl_create(&acl, rules, nrules, full) == 0);
			}
		}
		int rc = xsknf_gpu_lb_sessions_put(lb, pk, pv, npre);
		CHECK(rc == 0 || rc == -ENOSPC);
		int32_t *v = malloc(sizeof(int32_t) * (n ? n : 1));
		uint64_t stats[XSKNF_GPU_LB_STATS];
		struct xsknf_gpu_lb_info info;
		for (int round = 0; round < 4; round++) {
			memcpy(before, umem, total);
			uint32_t ingress = rnd() % 4, nif = 1 + rnd() % 4;
			const struct xsknf_gpu_acl *use = round == 2 ? NULL : acl;
			for (uint32_t i = 0; i < n; i++) v[i] = 0x5eadbeef;
			CHECK(xsknf_gpu_lbfw_host(umem, total, d, n, ingress, 0, use, lb, v, stats) == -EINVAL);
			for (uint32_t i = 0; i < n; i++) CHECK(v[i] == 0x5eadbeef);
			CHECK(memcmp(before, umem, total) == 0);
			if (round == 3) {   /* the load balancer itself on the same object */
				CHECK(xsknf_gpu_lb_host(umem, total, d, n, ingress, nif, lb, v, stats) == 0);
				CHECK(stats[0] == n && stats[1] + stats[2] + stats[3] == n && stats[7] == 0);
				continue;
			}
			CHECK(xsknf_gpu_lbfw_host(umem, total, d, n, ingress, nif, use, lb, v, stats) == 0);
			CHECK(stats[0] == n && stats[1] + stats[2] + stats[3] + stats[7] == n && stats[6] == 0);
			if (!use) CHECK(stats[7] == 0);
			int32_t pass = (int32_t)((ingress + 1) % nif);
			uint64_t gated = 0;
			for (uint32_t i = 0, p = 0; i < n; p += lens[i], i++) {
				/* (round 0 only: later rounds see rewritten frames, whose keys moved) */
				if (round == 0 && is_held[i]) {
					CHECK(v[i] == held[i] && memcmp(before + p, umem + p, lens[i]) == 0);
					gated++;
				} else if (round == 0 || !use) {
					CHECK(v[i] == -1 || v[i] == pass || (v[i] >= 0 && v[i] < 4));
				}
			}
			if (round == 0) CHECK(stats[7] == gated);
			CHECK(xsknf_gpu_lb_info(lb, &info) == 0 && info.host_sessions <= maxs);
			if (stats[1] == 0) CHECK(memcmp(before, umem, total) == 0);
		}
		CHECK(xsknf_gpu_acl_destroy(acl) == 0);
		CHECK(xsknf_gpu_lb_destroy(lb) == 0);
		free(v); free(pk); free(pv); free(d); free(umem); free(before); free(lens); free(bk);
		free(rules); free(held); free(is_held);
	}
	printf("ok %d\n", cs);
	return 0;
}

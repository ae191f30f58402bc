/*
 * san_firewall.c -- the ACL parser and table builder (xsknf_amd/csrc/acl.cpp,
 * built with XSKNF_ACL_HOST_ONLY: no GPU call) and the firewall's host model
 * (firewall_host.cpp: xsknf_gpu_firewall_host) under AddressSanitizer + UBSan.
 * Every UMEM, descriptor array and verdict array is a heap block of exactly
 * its size, so a read past a frame at the UMEM's end or a write past n verdicts
 * is a heap overflow.  Cases: random ACLs from 0 rules to tables with one empty
 * slot, frames of every length 0..120 with every ihl and TCP / UDP / other
 * protocols, the last frame ending on the UMEM's last byte, descriptors outside
 * the UMEM, unaligned-mode addresses; ACL files good, bad and cut short at every
 * byte.  The verdicts are checked against a linear search of the rules (the last
 * equal rule wins); prints "ok <cases>".  CPU only (tests/test_firewall_san.py
 * builds and runs it).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

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

/* the header's rules 1-7 by a linear search over the rules, the last match winning */
static int32_t want_of(const uint8_t *f, uint32_t len, const struct xsknf_gpu_acl_rule *r, uint32_t nr)
{
	if (len < 14)
		return -1;
	if (f[12] != 8 || f[13] != 0)
		return 0;
	if (len < 34)
		return -1;
	uint32_t next = 14 + 4 * (f[14] & 15);
	if (f[23] == 6) {
		if (next + 20 > len)
			return -1;
	} else if (f[23] == 17) {
		if (next + 8 > len)
			return -1;
	} else {
		return 0;
	}
	int32_t v = 0;
	for (uint32_t i = 0; i < nr; i++)
		if (!memcmp(&r[i].saddr, f + 26, 4) && !memcmp(&r[i].daddr, f + 30, 4) && !memcmp(&r[i].sport, f + next, 2) &&
		    !memcmp(&r[i].dport, f + next + 2, 2) && r[i].proto == f[23])
			v = r[i].action;
	return v;
}

static int parse_cases(void)
{
	static const char good[] = "3\n10.0.0.1 10.0.0.2 80 443 TCP DROP\n1.2.3.4 5.6.7.8 65536 70000 UDP 12\n"
				   "255.255.255.255 0.0.0.0 0 0 UDP abc\n";
	char path[] = "/tmp/san_firewall_XXXXXX";
	int cs = -1, fd = mkstemp(path);
	CHECK(fd >= 0);
	close(fd);
	/* the file cut short at every byte: parsed or refused, never overrun */
	for (size_t cut = 0; cut <= sizeof(good) - 1; cut++) {
		FILE *f = fopen(path, "w");
		CHECK(f && fwrite(good, 1, cut, f) == cut);
		fclose(f);
		uint32_t n = 99;
		struct xsknf_gpu_acl_rule *out = malloc(sizeof(*out) * 3);
		int rc = xsknf_gpu_acl_parse(path, out, 3, &n);
		CHECK(rc == 0 || rc == -22);
		if (cut >= sizeof(good) - 4) {   /* whole, or only a piece of the last word missing (atoi reads the rest) */
			CHECK(rc == 0 && n == 3 && out[0].action == -1 && out[1].action == 12 && out[2].action == 0);
			CHECK(out[1].sport == 0 && out[1].proto == 17 && out[0].proto == 6);
		}
		/* a buffer of one rule for three */
		struct xsknf_gpu_acl_rule *one = malloc(sizeof(*one));
		int rc1 = xsknf_gpu_acl_parse(path, one, 1, &n);
		CHECK(rc1 == (rc == 0 ? -28 : -22));
		free(one);
		free(out);
	}
	unlink(path);
	uint32_t n;
	CHECK(xsknf_gpu_acl_parse(path, NULL, 0, &n) == -2);
	return 0;
}

int main(void)
{
	int cs;
	if (parse_cases())
		return 1;
	for (cs = 0; cs < 600; cs++) {
		const uint32_t nr = cs % 9 == 0 ? 0 : (cs % 4 == 0 ? 1 + (uint32_t)(rnd() % 3) : (uint32_t)(rnd() % 300));
		const uint32_t nf = cs % 11 == 0 ? 0 : 1 + (uint32_t)(rnd() % 200);
		struct xsknf_gpu_acl_rule *r = malloc(sizeof(*r) * nr);
		struct xsknf_gpu_desc *d = malloc(sizeof(*d) * nf);
		int32_t *v = malloc(sizeof(*v) * nf), *want = malloc(sizeof(*want) * nf);
		uint32_t *lens = malloc(sizeof(*lens) * nf), *gaps = malloc(sizeof(*gaps) * nf);
		uint64_t size = 0;
		CHECK((nr == 0 || r) && (nf == 0 || (d && v && want && lens && gaps)));
		for (uint32_t i = 0; i < nf; i++) {
			lens[i] = (uint32_t)(rnd() % 121);
			gaps[i] = (uint32_t)(rnd() % 9);   /* before frame i; the last frame ends the UMEM */
			size += gaps[i] + lens[i];
		}
		uint8_t *umem = malloc(size ? size : 1);
		CHECK(umem);
		for (uint64_t i = 0; i < size; i++)
			umem[i] = (uint8_t)rnd();
		uint64_t pos = 0;
		for (uint32_t i = 0; i < nf; i++) {
			pos += gaps[i];
			uint8_t *f = umem + pos;
			const uint32_t len = lens[i];
			if (len >= 14 && rnd() % 8) { f[12] = 8; f[13] = 0; }
			if (len > 14 && rnd() % 2) f[14] = 0x45;
			if (len > 23) f[23] = rnd() % 5 == 0 ? (uint8_t)rnd() : (rnd() % 2 ? 6 : 17);
			const uint64_t o = rnd() % ((pos < 0xffff ? pos : 0xffff) + 1);
			d[i].addr = (pos - o) | o << 48;
			d[i].len = len;
			d[i].options = (uint32_t)rnd();
			want[i] = -2;
			if (rnd() % 10 == 0) {   /* outside the UMEM */
				switch (rnd() % 4) {
				case 0: d[i].addr = size; d[i].len = 1; break;
				case 1: d[i].addr = pos; d[i].len = (uint32_t)(size - pos) + 1; break;
				case 2: d[i].addr = 1ULL << 47; break;
				default: d[i].addr = 0xffffULL << 48 | 0xffffffffffffULL; d[i].len = 0xffffffffu; break;
				}
				want[i] = -1;
			}
			pos += len;
		}
		CHECK(nf == 0 || pos == size);
		/* rules: keys taken from frames (hits), their one-bit neighbours, random ones, repeats */
		for (uint32_t i = 0; i < nr; i++) {
			memset(&r[i], 0xa5, sizeof(r[i]));
			r[i].saddr = (uint32_t)rnd();
			r[i].daddr = (uint32_t)rnd();
			r[i].sport = (uint16_t)rnd();
			r[i].dport = (uint16_t)rnd();
			r[i].proto = rnd() % 7 == 0 ? (uint8_t)rnd() : (rnd() % 2 ? 6 : 17);
			r[i].action = cs % 5 == 0 ? (int32_t)rnd() : (int32_t)(rnd() % 34) - 1;
			if (nf && rnd() % 3) {
				const uint32_t k = (uint32_t)(rnd() % nf);
				const uint64_t off = (d[k].addr & XSKNF_GPU_UNALIGNED_BUF_ADDR_MASK) + (d[k].addr >> 48);
				if (want[k] == -2 && d[k].len >= 34) {
					const uint8_t *f = umem + off;
					const uint32_t next = 14 + 4 * (f[14] & 15);
					if (next + 4 <= d[k].len) {
						memcpy(&r[i].saddr, f + 26, 4);
						memcpy(&r[i].daddr, f + 30, 4);
						memcpy(&r[i].sport, f + next, 2);
						memcpy(&r[i].dport, f + next + 2, 2);
						r[i].proto = f[23];
						if (rnd() % 4 == 0)
							r[i].saddr ^= 1u << (rnd() % 32);
					}
				}
			} else if (i && rnd() % 4 == 0) {
				const int32_t a = r[i].action;
				r[i] = r[rnd() % i];
				r[i].action = a;
			}
		}
		for (uint32_t i = 0; i < nf; i++)
			if (want[i] == -2)
				want[i] = want_of(umem + ((d[i].addr & XSKNF_GPU_UNALIGNED_BUF_ADDR_MASK) + (d[i].addr >> 48)),
						  d[i].len, r, nr);
		/* distinct matchable keys, for the tightest table */
		uint32_t distinct = 0;
		for (uint32_t i = 0; i < nr; i++) {
			int dup = r[i].proto != 6 && r[i].proto != 17;
			for (uint32_t j = 0; j < i && !dup; j++)
				dup = r[j].saddr == r[i].saddr && r[j].daddr == r[i].daddr && r[j].sport == r[i].sport &&
				      r[j].dport == r[i].dport && r[j].proto == r[i].proto;
			distinct += !dup;
		}
		uint32_t tight = 1;
		while (tight <= distinct)
			tight *= 2;
		const uint32_t slot_choices[3] = {0, tight, tight * 4};
		for (int s = 0; s < 3; s++) {
			struct xsknf_gpu_acl *acl = NULL;
			struct xsknf_gpu_acl_info info;
			CHECK(xsknf_gpu_acl_create(&acl, r, nr, slot_choices[s]) == 0 && acl);
			CHECK(xsknf_gpu_acl_info(acl, &info) == 0 && info.rules == distinct && info.slots > info.rules);
			CHECK(info.device_bytes == 0 && info.max_probe <= info.slots && (info.slots & (info.slots - 1)) == 0);
			for (uint32_t i = 0; i < nf; i++)
				v[i] = 0x5a5a5a5a;
			CHECK(xsknf_gpu_firewall_host(umem, size, d, nf, acl, v) == 0);
			for (uint32_t i = 0; i < nf; i++)
				CHECK(v[i] == want[i]);
			CHECK(xsknf_gpu_acl_destroy(acl) == 0);
		}
		if (tight > 1) {   /* one slot too few */
			struct xsknf_gpu_acl *acl = NULL;
			CHECK(xsknf_gpu_acl_create(&acl, r, nr, tight / 2) == (distinct >= tight / 2 ? -22 : 0));
			if (acl)
				xsknf_gpu_acl_destroy(acl);
		}
		free(umem);
		free(lens);
		free(gaps);
		free(want);
		free(v);
		free(d);
		free(r);
	}
	printf("ok %d\n", cs);
	return 0;
}

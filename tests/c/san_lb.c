/*
 * san_lb.c -- the load balancer's object (xsknf_amd/csrc/lb.cpp, built with
 * XSKNF_LB_HOST_ONLY: no GPU call) and its host model (lb_host.cpp:
 * xsknf_gpu_lb_host) under AddressSanitizer + UBSan.  Every UMEM, descriptor
 * array, verdict array and dump buffer is a heap block of exactly its size, so
 * a read or write past a frame at the UMEM's end, past n verdicts or past the
 * dump's cap is a heap overflow.  Cases: random services (0 backends to
 * several per service), session tables from max_sessions 0 to ones that fill
 * during the batch, frames of every length 0..120 with every ihl and TCP / UDP /
 * other protocols aimed at services, at stored sessions and at nothing, the
 * last frame ending on the UMEM's last byte, descriptors outside the UMEM,
 * unaligned-mode addresses, two batches per object.  Checked: the counters add
 * up, every verdict is -1, PASS or an ifindex that exists, the dump is sorted
 * and as long as the count says, bytes outside the frames are untouched; prints
 * "ok <cases>".  CPU only (tests/test_lb_san.py builds and runs it).
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
		struct xsknf_gpu_lb_info info;
		CHECK(xsknf_gpu_lb_info(lb, &info) == 0 && info.device_bytes == 0 && info.backends == nb);
		CHECK((info.slots & (info.slots - 1)) == 0 && info.slots >= 2 * maxs);

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
		uint32_t npre = 0, pos = 0;
		for (uint32_t i = 0; i < total; i++) umem[i] = (uint8_t)rnd();
		for (uint32_t i = 0; i < n; i++) {
			uint32_t len = lens[i], ihl = rnd() % 16, next = 14 + 4 * ihl;
			uint8_t *f = umem + pos;
			if (len >= 14 && rnd() % 8) { f[12] = 8; f[13] = 0; }
			if (len > 23) { f[14] = (uint8_t)(f[14] & 0xf0) | (uint8_t)ihl; f[23] = rnd() % 6 ? (rnd() & 1 ? 6 : 17) : 1; }
			if (len >= 34 && nb && rnd() % 2) {   /* towards a service */
				const struct xsknf_gpu_lb_backend *b = &bk[rnd() % nb];
				memcpy(f + 30, &b->vaddr, 4);
				f[23] = b->proto;
				if (next + 4 <= len) memcpy(f + next + 2, &b->vport, 2);
				if (rnd() % 2) { memset(f + 26, 7, 4); if (next + 2 <= len) memset(f + next, 9, 2); }   /* one repeated flow */
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
			if (rnd() % 9 == 0) { d[i].addr = rnd() % 3 ? total - len / 2 : 1ull << 47; if (len < 2) d[i].addr = total + 1ull; }
			pos += len;   /* back to back: the last frame ends on the UMEM's last byte */
		}
		int rc = xsknf_gpu_lb_sessions_put(lb, pk, pv, npre);
		CHECK(rc == 0 || rc == -ENOSPC);
		int32_t *v = malloc(sizeof(int32_t) * (n ? n : 1));
		uint64_t stats[XSKNF_GPU_LB_STATS];
		for (int round = 0; round < 2; round++) {
			memcpy(before, umem, total);
			uint32_t ingress = rnd() % 4, nif = rnd() % 5;
			CHECK(xsknf_gpu_lb_host(umem, total, d, n, ingress, nif, lb, v, stats) == 0);
			CHECK(stats[0] == n && stats[1] + stats[2] + stats[3] == n && stats[6] == 0 && stats[7] == 0);
			int32_t pass = nif > 1 ? (int32_t)((ingress + 1) % nif) : -1;
			for (uint32_t i = 0; i < n; i++) CHECK(v[i] == -1 || v[i] == pass || (v[i] >= 0 && v[i] < 4));
			CHECK(xsknf_gpu_lb_info(lb, &info) == 0 && info.host_sessions <= maxs);
			if (stats[1] == 0) CHECK(memcmp(before, umem, total) == 0);
		}
		uint32_t cnt = 0;
		rc = xsknf_gpu_lb_sessions_dump(lb, XSKNF_GPU_LB_HOST_TABLE, NULL, NULL, 0, &cnt);
		CHECK((rc == 0 && cnt == 0) || rc == -ENOSPC);
		CHECK(cnt == info.host_sessions);
		struct xsknf_gpu_lb_session_key *dk = malloc(sizeof(*dk) * (cnt ? cnt : 1));
		struct xsknf_gpu_lb_session_value *dv = malloc(sizeof(*dv) * (cnt ? cnt : 1));
		CHECK(xsknf_gpu_lb_sessions_dump(lb, XSKNF_GPU_LB_HOST_TABLE, dk, dv, cnt, &cnt) == 0);
		for (uint32_t i = 1; i < cnt; i++)
			CHECK(dk[i - 1].saddr < dk[i].saddr || (dk[i - 1].saddr == dk[i].saddr && memcmp(&dk[i - 1], &dk[i], sizeof(*dk)) != 0));
		CHECK(xsknf_gpu_lb_sessions_dump(lb, XSKNF_GPU_LB_DEVICE_TABLE, dk, dv, cnt, &cnt) == -ENODEV);
		CHECK(xsknf_gpu_lb_destroy(lb) == 0);
		free(dk); free(dv); free(v); free(pk); free(pv); free(d); free(umem); free(before); free(lens); free(bk);
	}
	printf("ok %d\n", cs);
	return 0;
}

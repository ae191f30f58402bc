"""Record tests/golden/lb_golden.npz from the reference's own load balancer.

    python3 tests/golden/make_lb_golden.py REFERENCE_CHECKOUT [OUT.npz]

Not run by the tests.  In a scratch directory it assembles a C harness from
VERBATIM line ranges of the reference checkout, each checked against an anchor
line first (as oracle/ref_extract.sh does), compiles it together with the
reference's own examples/common/khashmap.c against its headers/ (jhash.h,
list_nulls.h) and load_balancer.h, and runs three consecutive batches through
the reference's xsknf_packet_processor():

    src/xsknf.h:4,11-12,25-40                        struct xsknf_config
    examples/load_balancer/load_balancer_user.c:1-2  load_balancer.h, khashmap.h
    ...:31                                           struct xsknf_config config;
    ...:49-50,57                                     the three khashmaps
    ...:396-553                                      xsknf_packet_processor()

Around them the harness (this file's own text) fills the three maps through
khashmap_update_elem -- services and backends as load_services does, with the
record's ifindex where the reference leaves it uninitialised -- applies rule 0
(a frame outside the UMEM is -1 and never handed over), and writes what the
function left.  The function is built with -fno-strict-aliasing: for ihl < 5
it reads through uint16_t pointers what it wrote through uint32_t fields, and
the contract is the order of its lines.  Nothing of the reference's text is
kept: only the data below and the sources' SHA-256 go into the fixture.
"""
import hashlib
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import firewall_cases as FC   # noqa: E402
from tests import lb_cases as LC         # noqa: E402
from xsknf_amd import lb                 # noqa: E402

LBU = "examples/load_balancer/load_balancer_user.c"
XH = "src/xsknf.h"
ANCHORS = [
    (XH, 4, "#include <stdint.h>"), (XH, 11, "#define XSKNF_MAX_INTERFACES"), (XH, 25, "struct xsknf_config {"),
    (XH, 40, "};"),
    (LBU, 1, '#include "load_balancer.h"'), (LBU, 2, '#include "../common/khashmap.h"'),
    (LBU, 31, "struct xsknf_config config;"), (LBU, 49, "struct khashmap services;"),
    (LBU, 50, "struct khashmap backends;"), (LBU, 57, "struct khashmap active_sessions;"),
    (LBU, 396, "int xsknf_packet_processor(void *pkt, unsigned len, unsigned ingress_ifindex)"),
    (LBU, 520, "UPDATE:;"), (LBU, 553, "}"),
    ("examples/load_balancer/load_balancer.h", 54, "static inline uint16_t csum_fold(uint32_t csum)"),
    ("examples/common/khashmap.c", 130, "int khashmap_update_elem(struct khashmap *map, void *key, void *value,"),
    ("headers/linux/jhash.h", 93, "static inline uint32_t jhash(const void *key, uint32_t length, uint32_t initval)"),
]
RANGES = [(XH, 4, 4), (XH, 11, 12), (XH, 25, 40), (LBU, 1, 2), (LBU, 31, 31), (LBU, 49, 50), (LBU, 57, 57),
          (LBU, 396, 553)]
SOURCES = [LBU, XH, "examples/load_balancer/load_balancer.h", "examples/common/khashmap.c", "examples/common/khashmap.h",
           "headers/linux/jhash.h", "headers/linux/list_nulls.h"]

PRELUDE = r"""
#include <arpa/inet.h>
#include <linux/ip.h>
#include <linux/jhash.h>
#include <linux/tcp.h>
#include <linux/udp.h>
#include <net/ethernet.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
"""

HARNESS = r"""
/* ---- the harness: maps filled through khashmap_update_elem, batches in order ---- */
struct rec_backend { uint32_t vaddr; uint16_t vport; uint8_t proto, pad; uint32_t addr; uint16_t port; uint8_t mac[6];
                     uint16_t ifindex; uint8_t pad2[2]; };
struct rec_key { uint32_t saddr, daddr; uint16_t sport, dport; uint8_t proto, pad[3]; };
struct rec_val { uint32_t addr; uint16_t port, ifindex; uint8_t mac[6]; uint8_t dir, pad; };
struct rec_desc { uint64_t addr; uint32_t len, options; };

static void rd(void *p, size_t n, FILE *f) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } }

int main(int argc, char **argv)
{
	if (argc != 3) return 2;
	FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
	if (!in || !out) return 2;
	uint32_t nb, ns, nbatch;
	rd(&nb, 4, in); rd(&ns, 4, in); rd(&nbatch, 4, in);
	khashmap_init(&active_sessions, sizeof(struct session_id), sizeof(struct replace_info), 1 << 16);
	khashmap_init(&services, sizeof(struct service_id), sizeof(struct service_info), MAX_SERVICES);
	khashmap_init(&backends, sizeof(struct backend_id), sizeof(struct backend_info), 1 << 14);
	for (uint32_t i = 0; i < nb; i++) {
		struct rec_backend r;
		rd(&r, sizeof(r), in);
		struct backend_id bid;
		memset(&bid, 0, sizeof(bid));
		bid.service.vaddr = r.vaddr; bid.service.vport = r.vport; bid.service.proto = r.proto;
		struct service_info *si = khashmap_lookup_elem(&services, &bid.service), fresh = { 0 };
		bid.index = si ? si->backends : 0;
		fresh.backends = bid.index + 1;
		if (khashmap_update_elem(&services, &bid.service, &fresh, 0)) return 3;
		struct backend_info bi;
		memset(&bi, 0, sizeof(bi));
		bi.addr = r.addr; bi.port = r.port; memcpy(bi.mac_addr, r.mac, 6); bi.ifindex = r.ifindex;
		if (khashmap_update_elem(&backends, &bid, &bi, 0)) return 3;
	}
	for (uint32_t i = 0; i < ns; i++) {
		struct rec_key k; struct rec_val v;
		rd(&k, sizeof(k), in); rd(&v, sizeof(v), in);
		struct session_id sid;
		memset(&sid, 0, sizeof(sid));
		sid.saddr = k.saddr; sid.daddr = k.daddr; sid.sport = k.sport; sid.dport = k.dport; sid.proto = k.proto;
		struct replace_info rep;
		memset(&rep, 0, sizeof(rep));
		rep.dir = v.dir; rep.addr = v.addr; rep.port = v.port; memcpy(rep.mac_addr, v.mac, 6); rep.ifindex = v.ifindex;
		if (khashmap_update_elem(&active_sessions, &sid, &rep, 0)) return 3;
	}
	for (uint32_t b = 0; b < nbatch; b++) {
		uint64_t size; uint32_t n, ingress, nif;
		rd(&size, 8, in); rd(&n, 4, in); rd(&ingress, 4, in); rd(&nif, 4, in);
		uint8_t *umem = malloc(size + 1);
		struct rec_desc *d = malloc(sizeof(*d) * (n + 1));
		rd(umem, size, in); rd(d, sizeof(*d) * n, in);
		config.num_interfaces = nif;
		for (uint32_t i = 0; i < n; i++) {
			uint64_t off = (d[i].addr & ((1ull << 48) - 1)) + (d[i].addr >> 48);
			int32_t v = -1;
			if (off <= size && d[i].len <= size - off) v = xsknf_packet_processor(umem + off, d[i].len, ingress);
			fwrite(&v, 4, 1, out);
		}
		fwrite(umem, 1, size, out);
		free(umem); free(d);
	}
	uint32_t count = (uint32_t)(((char *)active_sessions.next_free - (char *)active_sessions.elems) / active_sessions.elem_size);
	fwrite(&count, 4, 1, out);
	for (uint32_t i = 0; i < count; i++) {
		struct khashmap_elem *e = (void *)((char *)active_sessions.elems + (size_t)i * active_sessions.elem_size);
		fwrite(e->key, 1, sizeof(struct session_id), out);
		fwrite(e->key + 16, 1, sizeof(struct replace_info), out);
	}
	fclose(out);
	return 0;
}
"""


def lines(ref, rel):
    return open(os.path.join(ref, rel)).read().split("\n")


def build_harness(ref, work):
    for rel, ln, want in ANCHORS:
        got = lines(ref, rel)[ln - 1]
        if not got.startswith(want):
            raise SystemExit(f"{rel}:{ln} is {got!r}, expected {want!r}...: the reference's lines moved")
    parts = [PRELUDE]
    for rel, lo, hi in RANGES:
        parts.append(f'#line {lo} "{rel}"')
        parts += lines(ref, rel)[lo - 1:hi]
    parts.append('#line 1 "harness"')
    parts.append(HARNESS)
    src = os.path.join(work, "lb_ref.c")
    open(src, "w").write("\n".join(parts) + "\n")
    exe = os.path.join(work, "lb_ref")
    subprocess.run(["gcc", "-O1", "-fno-strict-aliasing", "-w", "-std=gnu11", "-I", os.path.join(ref, "headers"),
                    "-I", os.path.join(ref, "examples", "load_balancer"), "-I", os.path.join(ref, "examples", "common"),
                    "-o", exe, src, os.path.join(ref, "examples", "common", "khashmap.c"), "-pthread"], check=True)
    return exe


def make_inputs():
    """The backends, the pre-populated sessions and three batches (see the
    fixture's `about`)."""
    rng = np.random.default_rng(20261020)
    base = LC.make_backends(rng, services=5)
    cause = {c: LC.ordered_cause(rng, c, salt=0x100 * (i + 1)) for i, c in enumerate(("existing_b", "shared_b", "vip_client"))}
    # batch 0: every branch; per ihl and protocol a session hit in each direction,
    # a new flow towards a service made from the frame's own key (for ihl < 5 the
    # key fields overlap), and a frame that matches nothing
    b0, ph0 = FC.decision_frames(rng, phases=(0,))
    ph0 = [int(rng.integers(16)) for _ in b0]
    extra, svc_recs, pre_k, pre_v = [], [], [], []
    ports = [0x0000, 0xffff, 0x8000, 0x0100, 0x00ff]
    for ihl in range(16):
        for proto in (6, 17):
            for kind in range(5):
                sid = (int(rng.integers(1 << 32)), int(rng.integers(1 << 32)), ports[int(rng.integers(5))],
                       ports[int(rng.integers(5))], proto)
                f = LC.frame(rng, sid, ihl=ihl, zero_check=kind == 0)
                key = LC.frame_sid(f)
                extra.append(f)
                if kind < 2:
                    k, v = LC.session(LC._u32(key, 0), LC._u32(key, 4), LC._u16(key, 8), LC._u16(key, 10), proto, kind,
                                      int(rng.integers(1 << 32)), ports[int(rng.integers(5))],
                                      rng.integers(0, 256, 6).tolist(), int(rng.integers(4)))
                    pre_k.append(k)
                    pre_v.append(v)
                elif kind < 4:
                    for _ in range(kind):
                        svc_recs.append((LC._u32(key, 4), LC._u16(key, 10), proto, 0, int(rng.integers(1, 1 << 32)),
                                         ports[int(rng.integers(5))], tuple(rng.integers(0, 256, 6).tolist()),
                                         int(rng.integers(4)), (0, 0)))
                    extra.append(f[:6] + bytes(rng.integers(0, 256, 6).tolist()) + f[12:])   # the flow's second frame
    b0 += extra
    ph0 += [int(rng.integers(16)) for _ in extra]
    backends = np.concatenate([base, np.array(svc_recs, dtype=lb.BACKEND_DTYPE)] + [cause[c][0] for c in cause])
    # (only existing_b brings a session)
    pre_k += list(cause["existing_b"][1][0])
    pre_v += list(cause["existing_b"][1][1])
    # batch 1: flows of several frames with their backward traffic before and
    # after the creator, then each ordered-path cause
    b1 = LC.flows_batch(rng, base, flows=120, filler=60)
    b1 += cause["existing_b"][2] + cause["shared_b"][2]
    # batch 2: the same flows again (every session is found), more new ones, and
    # the third cause
    b2 = [b1[i] for i in rng.permutation(len(b1))[:300]] + LC.flows_batch(rng, base, flows=40, filler=20)
    b2 += cause["vip_client"][2]
    batches = []
    for fl, ph, ingress, nif in ((b0, ph0, 0, 4), (b1, None, 1, 4), (b2, None, 2, 1)):
        umem, descs = LC.pack_packed(fl, rng, ph)
        batches.append((umem, FC.with_outside(umem, descs, rng), ingress, nif))
    return backends, np.array(pre_k, dtype=lb.KEY_DTYPE), np.array(pre_v, dtype=lb.VALUE_DTYPE), batches


def main():
    ref = sys.argv[1]
    out_path = sys.argv[2] if len(sys.argv) > 2 else LC.GOLDEN
    backends, pre_k, pre_v, batches = make_inputs()
    with tempfile.TemporaryDirectory() as work:
        exe = build_harness(ref, work)
        blob = struct.pack("<III", backends.shape[0], pre_k.shape[0], len(batches))
        blob += backends.tobytes()
        blob += b"".join(k.tobytes() + v.tobytes() for k, v in zip(pre_k, pre_v))
        for umem, descs, ingress, nif in batches:
            blob += struct.pack("<QIII", umem.size, descs.shape[0], ingress, nif) + umem.tobytes() + descs.tobytes()
        open(os.path.join(work, "in.bin"), "wb").write(blob)
        subprocess.run([exe, os.path.join(work, "in.bin"), os.path.join(work, "out.bin")], check=True)
        res = open(os.path.join(work, "out.bin"), "rb").read()
    data = {"backends": backends, "pre_keys": pre_k, "pre_values": pre_v}
    pos = 0
    for b, (umem, descs, ingress, nif) in enumerate(batches):
        n = descs.shape[0]
        data[f"umem{b}"] = umem
        data[f"descs{b}"] = descs
        data[f"params{b}"] = np.array([ingress, nif], dtype=np.uint32)
        data[f"verdicts{b}"] = np.frombuffer(res, dtype="<i4", count=n, offset=pos).copy()
        pos += 4 * n
        data[f"after{b}"] = np.frombuffer(res, dtype=np.uint8, count=umem.size, offset=pos).copy()
        pos += umem.size
    (count,) = struct.unpack_from("<I", res, pos)
    pos += 4
    rows = np.frombuffer(res, dtype=np.uint8, count=count * 31, offset=pos).reshape(count, 31)
    assert pos + count * 31 == len(res)
    # struct session_id (13 bytes) and struct replace_info (4 dir, 4 addr, 2 port, 6 mac, 2 ifindex), in the
    # order the reference's pool holds them
    data["final_keys"] = rows[:, :13].copy()
    data["final_values"] = rows[:, 13:].copy()
    data["sources_sha256"] = np.array([f"{hashlib.sha256(open(os.path.join(ref, s), 'rb').read()).hexdigest()}  {s}"
                                       for s in SOURCES])
    data["about"] = np.array(
        "three consecutive batches through the reference's xsknf_packet_processor "
        "(load_balancer_user.c:396-553 with khashmap.c, jhash.h, load_balancer.h), -fno-strict-aliasing; "
        "batch 0: every parse branch x ihl 0..15 x protocol, session hits in both directions, new flows and misses per "
        "ihl and protocol, UDP checks of 0, ports 0000 ffff 8000 0100 00ff; batch 1: flows of 1-5 frames with backward "
        "traffic before and after their creator, a pre-existing backward key, two flows sharing a backward key; "
        "batch 2: the sessions found again, new flows, a service address as a client; nif 1 (PASS = -1)")
    np.savez_compressed(out_path, **data)
    print(out_path, os.path.getsize(out_path), "bytes;", sum(b[1].shape[0] for b in batches), "frames;", count, "sessions")


if __name__ == "__main__":
    main()

"""Record tests/golden/lbfw_golden.npz from the reference's own lbfw NF.

    python3 tests/golden/make_lbfw_golden.py REFERENCE_CHECKOUT [OUT.npz]

Not run by the tests.  As make_lb_golden.py does, it assembles a C harness in a
scratch directory from VERBATIM line ranges of the reference checkout, each
checked against an anchor line first, compiles it together with the reference's
own examples/common/khashmap.c against its headers/ and lbfw.h, and runs the
same consecutive batches through the reference's xsknf_packet_processor() twice,
each time from the same pre-populated table:

    src/xsknf.h:4,11-12,15-17,25-40          MODE_*, struct xsknf_config
    examples/lbfw/lbfw_user.c:1-2            lbfw.h, khashmap.h
    ...:28                                   struct xsknf_config config;
    ...:45-46,53-54                          the four khashmaps
    ...:420-594                              xsknf_packet_processor()

once with config.working_mode = MODE_AF_XDP (the ACL gate runs: "afxdp") and
once with MODE_COMBINED (the function skips it: "combined", what acl == NULL
gives here).  The harness (this file's own text) fills the maps through
khashmap_update_elem, applies rule 0 and writes the verdicts, the UMEM and the
session pool after every batch.  num_interfaces is never 0 (the function would
divide by zero).  Built with -fno-strict-aliasing, as make_lb_golden.py says.
Nothing of the reference's text is kept: only the data below and the sources'
SHA-256 go into the fixture.
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
from tests import lbfw_cases as WC       # noqa: E402
from xsknf_amd import lb                 # noqa: E402

LFU = "examples/lbfw/lbfw_user.c"
XH = "src/xsknf.h"
ANCHORS = [
    (XH, 4, "#include <stdint.h>"), (XH, 11, "#define XSKNF_MAX_INTERFACES"), (XH, 15, "#define MODE_AF_XDP 0x1"),
    (XH, 17, "#define MODE_COMBINED (MODE_AF_XDP | MODE_XDP)"), (XH, 25, "struct xsknf_config {"), (XH, 40, "};"),
    (LFU, 1, '#include "lbfw.h"'), (LFU, 2, '#include "../common/khashmap.h"'),
    (LFU, 28, "struct xsknf_config config;"), (LFU, 45, "struct khashmap services;"),
    (LFU, 46, "struct khashmap backends;"), (LFU, 53, "struct khashmap active_sessions;"),
    (LFU, 54, "struct khashmap acl;"),
    (LFU, 420, "int xsknf_packet_processor(void *pkt, unsigned len, unsigned ingress_ifindex)"),
    (LFU, 435, "\t\treturn (ingress_ifindex + 1) % config.num_interfaces;"),
    (LFU, 486, "\tif (config.working_mode == MODE_AF_XDP) {"), (LFU, 561, "UPDATE:;"), (LFU, 594, "}"),
    ("examples/lbfw/lbfw.h", 3, "#define MAX_ACL_SIZE"),
    ("examples/common/khashmap.c", 130, "int khashmap_update_elem(struct khashmap *map, void *key, void *value,"),
    ("headers/linux/jhash.h", 93, "static inline uint32_t jhash(const void *key, uint32_t length, uint32_t initval)"),
]
RANGES = [(XH, 4, 4), (XH, 11, 12), (XH, 15, 17), (XH, 25, 40), (LFU, 1, 2), (LFU, 28, 28), (LFU, 45, 46), (LFU, 53, 54),
          (LFU, 420, 594)]
SOURCES = [LFU, XH, "examples/lbfw/lbfw.h", "examples/common/khashmap.c", "examples/common/khashmap.h",
           "headers/linux/jhash.h", "headers/linux/list_nulls.h"]
MODES = {"afxdp": 1, "combined": 3}

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
struct rec_rule { uint32_t saddr, daddr; uint16_t sport, dport; uint8_t proto, pad[3]; int32_t action; };
struct rec_desc { uint64_t addr; uint32_t len, options; };

static void rd(void *p, size_t n, FILE *f) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } }

int main(int argc, char **argv)
{
	if (argc != 3) return 2;
	FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
	if (!in || !out) return 2;
	uint32_t mode, nb, ns, nr, nbatch;
	rd(&mode, 4, in); rd(&nb, 4, in); rd(&ns, 4, in); rd(&nr, 4, in); rd(&nbatch, 4, in);
	config.working_mode = mode;
	khashmap_init(&active_sessions, sizeof(struct session_id), sizeof(struct replace_info), 1 << 16);
	khashmap_init(&services, sizeof(struct service_id), sizeof(struct service_info), MAX_SERVICES);
	khashmap_init(&backends, sizeof(struct backend_id), sizeof(struct backend_info), 1 << 14);
	khashmap_init(&acl, sizeof(struct session_id), sizeof(int), 1 << 14);
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
	for (uint32_t i = 0; i < nr; i++) {
		struct rec_rule r;
		rd(&r, sizeof(r), in);
		struct session_id sid;
		memset(&sid, 0, sizeof(sid));
		sid.saddr = r.saddr; sid.daddr = r.daddr; sid.sport = r.sport; sid.dport = r.dport; sid.proto = r.proto;
		int action = r.action;
		if (khashmap_update_elem(&acl, &sid, &action, 0)) return 3;
	}
	for (uint32_t b = 0; b < nbatch; b++) {
		uint64_t size; uint32_t n, ingress, nif;
		rd(&size, 8, in); rd(&n, 4, in); rd(&ingress, 4, in); rd(&nif, 4, in);
		if (nif == 0) return 4;
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
		uint32_t count = (uint32_t)(((char *)active_sessions.next_free - (char *)active_sessions.elems) / active_sessions.elem_size);
		fwrite(&count, 4, 1, out);
		for (uint32_t i = 0; i < count; i++) {
			struct khashmap_elem *e = (void *)((char *)active_sessions.elems + (size_t)i * active_sessions.elem_size);
			fwrite(e->key, 1, sizeof(struct session_id), out);
			fwrite(e->key + 16, 1, sizeof(struct replace_info), out);
		}
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
    src = os.path.join(work, "lbfw_ref.c")
    open(src, "w").write("\n".join(parts) + "\n")
    exe = os.path.join(work, "lbfw_ref")
    subprocess.run(["gcc", "-O1", "-fno-strict-aliasing", "-w", "-std=gnu11", "-I", os.path.join(ref, "headers"),
                    "-I", os.path.join(ref, "examples", "lbfw"), "-I", os.path.join(ref, "examples", "common"),
                    "-o", exe, src, os.path.join(ref, "examples", "common", "khashmap.c"), "-pthread"], check=True)
    return exe


ACTIONS = (0, -1, 2, 0, 3, 9999, -1, 1)


def make_inputs():
    """The backends, the pre-populated sessions, the ACL and three batches (see
    the fixture's `about`)."""
    rng = np.random.default_rng(20261021)
    base = LC.make_backends(rng, services=5)
    cause = {c: LC.ordered_cause(rng, c, salt=0x100 * (i + 1)) for i, c in enumerate(("existing_b", "shared_b"))}
    acl_keys = []   # every ACL'd key, in order; the actions cycle
    # batch 0: a sample of the parse's branches; per ihl and protocol a session hit
    # in each direction, two new flows towards services made from the frame's own
    # key, and a frame that matches nothing.  A third of each kind is ACL'd.
    dec, _ = FC.decision_frames(rng, phases=(0,))
    b0 = [dec[i] for i in range(0, len(dec), 4)]
    svc_recs, pre_k, pre_v = [], [], []
    ports = [0x0000, 0xffff, 0x8000, 0x0100, 0x00ff]
    for ihl in range(16):
        for proto in (6, 17):
            for kind in range(5):
                sid = (int(rng.integers(1 << 32)), int(rng.integers(1 << 32)), ports[int(rng.integers(5))],
                       ports[int(rng.integers(5))], proto)
                f = LC.frame(rng, sid, ihl=ihl, zero_check=kind == 0)
                key = LC.frame_sid(f)
                b0.append(f)
                if (ihl + kind + (proto == 6)) % 3 == 0:
                    acl_keys.append(key)
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
                    b0.append(f[:6] + bytes(rng.integers(0, 256, 6).tolist()) + f[12:])   # the flow's second frame
    backends = np.concatenate([base, np.array(svc_recs, dtype=lb.BACKEND_DTYPE)] + [cause[c][0] for c in cause])
    pre_k += list(cause["existing_b"][1][0])
    pre_v += list(cause["existing_b"][1][1])
    # batch 1: flows of several frames with their backward traffic; of the flows a
    # third has its forward key in the ACL and a sixth its backward key; a
    # pre-existing backward key (not ACL'd: the reference's loop replaces it)
    b1 = LC.flows_batch(rng, base, flows=90, filler=40) + cause["existing_b"][2]
    # batch 2, one interface: frames of batch 1 again, new flows, and two flows
    # that share a backward key, the second of them ACL'd
    b2 = [b1[i] for i in rng.permutation(len(b1))[:220]] + LC.flows_batch(rng, base, flows=30, filler=20)
    b2 += cause["shared_b"][2]
    services = {(int(r["vaddr"]), int(r["vport"]), int(r["proto"])) for r in base}
    j = 0
    for key in WC.frame_keys(b1 + b2):
        sid = (LC._u32(key, 0), LC._u32(key, 4), LC._u16(key, 8), LC._u16(key, 10), key[12])
        if (sid[1], sid[3], sid[4]) not in services:
            continue
        j += 1
        if j % 3 == 0:
            acl_keys.append(key)
        elif j % 6 == 1:
            acl_keys.append(WC.sid_key(LC.backward_sid(base, sid)))
    acl_keys.append(WC.frame_keys(cause["shared_b"][2])[2])   # s2, the second flow of the shared backward key
    held = set(acl_keys)
    actions = [ACTIONS[i % len(ACTIONS)] for i in range(len(acl_keys))]
    # one-bit neighbours of keys the ACL does not hold: they must not match
    near = [k for k in WC.frame_keys(b0 + b1 + b2) if k not in held][::7]
    for i, k in enumerate(near):
        nb = WC.flip(k, (11 * i) % 96)
        if nb not in held:
            acl_keys.append(nb)
            actions.append(5)
    rules = FC.rules_from_keys(acl_keys, actions)
    batches = []
    for fl, ingress, nif in ((b0, 0, 4), (b1, 1, 4), (b2, 2, 1)):
        umem, descs = LC.pack_packed(fl, rng, [int(rng.integers(16)) for _ in fl] if fl is b0 else None)
        batches.append((umem, FC.with_outside(umem, descs, rng), ingress, nif))
    return backends, np.array(pre_k, dtype=lb.KEY_DTYPE), np.array(pre_v, dtype=lb.VALUE_DTYPE), rules, batches


def main():
    ref = sys.argv[1]
    out_path = sys.argv[2] if len(sys.argv) > 2 else WC.GOLDEN
    backends, pre_k, pre_v, rules, batches = make_inputs()
    assert all(nif > 0 for _, _, _, nif in batches)
    data = {"backends": backends, "pre_keys": pre_k, "pre_values": pre_v, "rules": rules,
            "batches": np.array(len(batches), dtype=np.uint32)}
    for b, (umem, descs, ingress, nif) in enumerate(batches):
        data[f"umem{b}"] = umem
        data[f"descs{b}"] = descs
        data[f"params{b}"] = np.array([ingress, nif], dtype=np.uint32)
    with tempfile.TemporaryDirectory() as work:
        exe = build_harness(ref, work)
        for mode, value in MODES.items():
            blob = struct.pack("<IIIII", value, backends.shape[0], pre_k.shape[0], rules.shape[0], len(batches))
            blob += backends.tobytes()
            blob += b"".join(k.tobytes() + v.tobytes() for k, v in zip(pre_k, pre_v))
            blob += rules.tobytes()
            for umem, descs, ingress, nif in batches:
                blob += struct.pack("<QIII", umem.size, descs.shape[0], ingress, nif) + umem.tobytes() + descs.tobytes()
            open(os.path.join(work, "in.bin"), "wb").write(blob)
            subprocess.run([exe, os.path.join(work, "in.bin"), os.path.join(work, "out.bin")], check=True)
            res = open(os.path.join(work, "out.bin"), "rb").read()
            pos = 0
            for b, (umem, descs, ingress, nif) in enumerate(batches):
                n = descs.shape[0]
                data[f"{mode}_verdicts{b}"] = np.frombuffer(res, dtype="<i4", count=n, offset=pos).copy()
                pos += 4 * n
                data[f"{mode}_after{b}"] = np.frombuffer(res, dtype=np.uint8, count=umem.size, offset=pos).copy()
                pos += umem.size
                (count,) = struct.unpack_from("<I", res, pos)
                pos += 4
                # struct session_id (13 bytes) and struct replace_info (4 dir, 4 addr, 2 port, 6 mac, 2 ifindex),
                # in the order the reference's pool holds them
                data[f"{mode}_sessions{b}"] = np.frombuffer(res, dtype=np.uint8, count=count * 31,
                                                            offset=pos).reshape(count, 31).copy()
                pos += count * 31
            assert pos == len(res)
    data["sources_sha256"] = np.array([f"{hashlib.sha256(open(os.path.join(ref, s), 'rb').read()).hexdigest()}  {s}"
                                       for s in SOURCES])
    data["about"] = np.array(
        "three consecutive batches through the reference's xsknf_packet_processor (lbfw_user.c:420-594 with khashmap.c, "
        "jhash.h, lbfw.h), -fno-strict-aliasing, twice from the same pre-populated table: afxdp_* with working_mode "
        "MODE_AF_XDP (the ACL gate), combined_* with MODE_COMBINED (no gate: acl == NULL); *_sessions<b> is the session "
        "pool after batch b.  ACL actions 0, -1, 1, 2, 3, 9999 on service flows, on flows with pre-put sessions and on "
        "backward keys, plus one-bit neighbours (action 5) of keys it does not hold.  batch 0: a sample of the parse's "
        "branches, ihl 0..15 x protocol with session hits in both directions, new flows and misses; batch 1: flows of "
        "1-5 frames with backward traffic, a pre-existing backward key; batch 2: nif 1 (PASS = 0), batch 1's frames "
        "again, new flows, two flows sharing a backward key of which the second is ACL'd.  nif is never 0")
    np.savez_compressed(out_path, **data)
    print(out_path, os.path.getsize(out_path), "bytes;", sum(b[1].shape[0] for b in batches), "frames;",
          {m: int(data[f"{m}_sessions{len(batches) - 1}"].shape[0]) for m in MODES}, "sessions;", rules.shape[0], "rules")


if __name__ == "__main__":
    main()

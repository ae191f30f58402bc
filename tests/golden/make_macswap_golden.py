"""Record tests/golden/macswap_golden.npz from the reference's own macswap.

    python3 tests/golden/make_macswap_golden.py REFERENCE_CHECKOUT [OUT.npz]

Not run by the tests.  In a scratch directory it assembles a C harness from
VERBATIM line ranges of the reference checkout, each checked against an anchor
line first (as oracle/ref_extract.sh does), compiles it and runs every batch of
tests/macswap_cases.py golden_batches() through the reference's
xsknf_packet_processor():

    src/xsknf.h:4,11-12,25-40               struct xsknf_config
    examples/macswap/macswap.h              whole (the two swap functions)
    examples/macswap/macswap_user.c:18-22   enum action
    ...:28-29                               opt_action, opt_double_macswap
    ...:34-50                               xsknf_packet_processor()

Around them the harness (this file's own text) declares `config`, sets the three
globals per batch, applies rule 0 (a frame outside the UMEM is -1 and never
handed over), and writes the verdicts and what the function left of the UMEM.
Built with -O2 as the reference's Makefile builds it: macswap.h's plain `inline`
functions have no out-of-line definition and do not link at -O0.  Nothing of the
reference's text is kept: only the data below and the sources' SHA-256 go into
the fixture.
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

from tests import macswap_cases as MC   # noqa: E402

MSU = "examples/macswap/macswap_user.c"
MSH = "examples/macswap/macswap.h"
XH = "src/xsknf.h"
ANCHORS = [
    (XH, 4, "#include <stdint.h>"), (XH, 11, "#define XSKNF_MAX_INTERFACES"), (XH, 25, "struct xsknf_config {"),
    (XH, 40, "};"),
    (MSH, 1, "struct global_data {"), (MSH, 6, "void inline swap_mac_addresses(void *data)"),
    (MSH, 26, "void inline swap_mac_addresses_v2(void *data)"), (MSH, 36, "}"),
    (MSU, 18, "enum action {"), (MSU, 22, "};"),
    (MSU, 28, "static enum action opt_action = ACTION_REDIRECT;"), (MSU, 29, "static int opt_double_macswap = 0;"),
    (MSU, 34, "int xsknf_packet_processor(void *pkt, unsigned len, unsigned ingress_ifindex)"),
    (MSU, 50, "}"),
]
SOURCES = [MSU, MSH, XH]

PRELUDE = r"""
#include <linux/if_ether.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
"""

HARNESS = r"""
/* ---- the harness: the globals set per batch, rule 0 around the call ---- */
struct rec_desc { uint64_t addr; uint32_t len, options; };

static void rd(void *p, size_t n, FILE *f) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } }

int main(int argc, char **argv)
{
	if (argc != 3) return 2;
	FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
	if (!in || !out) return 2;
	uint32_t nbatch;
	rd(&nbatch, 4, in);
	for (uint32_t b = 0; b < nbatch; b++) {
		uint64_t size; uint32_t n, ingress, action, twice, nif;
		rd(&size, 8, in); rd(&n, 4, in); rd(&ingress, 4, in); rd(&action, 4, in); rd(&twice, 4, in); rd(&nif, 4, in);
		uint8_t *umem = malloc(size + 1);
		struct rec_desc *d = malloc(sizeof(*d) * (n + 1));
		rd(umem, size, in); rd(d, sizeof(*d) * n, in);
		config.num_interfaces = nif;
		opt_action = (enum action)action;
		opt_double_macswap = (int)twice;
		for (uint32_t i = 0; i < n; i++) {
			uint64_t off = (d[i].addr & ((1ull << 48) - 1)) + (d[i].addr >> 48);
			int32_t v = -1;
			if (off <= size && d[i].len <= size - off) v = xsknf_packet_processor(umem + off, d[i].len, ingress);
			fwrite(&v, 4, 1, out);
		}
		fwrite(umem, 1, size, out);
		free(umem); free(d);
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
    whole = len(lines(ref, MSH))
    parts = [PRELUDE]
    for rel, lo, hi in ((XH, 4, 4), (XH, 11, 12), (XH, 25, 40), (MSH, 1, whole), (MSU, 18, 22), (MSU, 28, 29)):
        parts.append(f'#line {lo} "{rel}"')
        parts += lines(ref, rel)[lo - 1:hi]
    parts.append('#line 1 "harness"')
    parts.append("struct xsknf_config config;")
    parts.append(f'#line 34 "{MSU}"')
    parts += lines(ref, MSU)[33:50]
    parts.append('#line 3 "harness"')
    parts.append(HARNESS)
    src = os.path.join(work, "macswap_ref.c")
    open(src, "w").write("\n".join(parts) + "\n")
    exe = os.path.join(work, "macswap_ref")
    subprocess.run(["gcc", "-O2", "-w", "-std=gnu11", "-o", exe, src], check=True)
    return exe


def main():
    ref = sys.argv[1]
    out_path = sys.argv[2] if len(sys.argv) > 2 else MC.GOLDEN
    batches = MC.golden_batches()
    with tempfile.TemporaryDirectory() as work:
        exe = build_harness(ref, work)
        blob = struct.pack("<I", len(batches))
        for umem, descs, ingress, action, double, nif in batches:
            blob += struct.pack("<QIIIII", umem.size, descs.shape[0], ingress, action, int(double), nif)
            blob += umem.tobytes() + descs.tobytes()
        open(os.path.join(work, "in.bin"), "wb").write(blob)
        subprocess.run([exe, os.path.join(work, "in.bin"), os.path.join(work, "out.bin")], check=True)
        res = open(os.path.join(work, "out.bin"), "rb").read()
    data = {"batches": np.array(len(batches), dtype=np.uint32)}
    pos = 0
    for b, (umem, descs, ingress, action, double, nif) in enumerate(batches):
        n = descs.shape[0]
        data[f"umem{b}"] = umem
        data[f"descs{b}"] = descs
        # ingress_ifindex, action, double_macswap, num_interfaces
        data[f"params{b}"] = np.array([ingress, action, int(double), nif], dtype=np.uint32)
        data[f"verdicts{b}"] = np.frombuffer(res, dtype="<i4", count=n, offset=pos).copy()
        pos += 4 * n
        data[f"after{b}"] = np.frombuffer(res, dtype=np.uint8, count=umem.size, offset=pos).copy()
        pos += umem.size
    assert pos == len(res)
    data["sources_sha256"] = np.array([f"{hashlib.sha256(open(os.path.join(ref, s), 'rb').read()).hexdigest()}  {s}"
                                       for s in SOURCES])
    data["about"] = np.array(
        "batches through the reference's xsknf_packet_processor (macswap_user.c:34-50 with macswap.h), gcc -O2, rule 0 "
        "applied around the call; params = ingress_ifindex, action, double_macswap, num_interfaces; batch 0: every "
        "length 0..20 at every start phase 0..15 and 59..1514 bytes, outside descriptors among them; batch 1: 14-byte "
        "frames back to back from offset 1, then lengths 14 15 17 13, PASS, ingress 0xffffffff; batches 2..25: "
        "action x swap mode x 1..4 interfaces, the ingress cycling 0 1 2 3 7fffffff fffffffe ffffffff")
    np.savez_compressed(out_path, **data)
    print(out_path, os.path.getsize(out_path), "bytes;", sum(b[1].shape[0] for b in batches), "frames;",
          len(batches), "batches")


if __name__ == "__main__":
    main()

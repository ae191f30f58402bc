"""xsknf_amd/csrc/desc_rules.h -- the one C++ statement of what a descriptor
means -- against the numpy restatements the copy sweeps use (tests/copy_cases.py
offsets() / chunks()), over a fixed grid (tests/c/desc_rules_grid.cpp, built
with g++ under AddressSanitizer + UBSan and run as a child process); and a
guard that the rules are stated nowhere else in xsknf_amd/csrc.  CPU only."""
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import copy_cases as CC
from tests.route_cases import CSRC
from xsknf_amd import frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (16, 4096, 1 << 40)

# Kernels that keep a rule written out, each under a one-line comment naming the
# rule.  Through the shared function the compiler emits other instructions for
# them (tools/asm_same.py against the commit before desc_rules.h); timed on the
# MI355X against that commit, five alternating runs each, the new build's median
# lay outside the old one's min..max (profiles/desc_rules/kernel_times.json), so
# they got their expression back.  slot_len of kernel_plan.h changed three
# planner kernels the same way, passed that measurement and calls slot_bytes.
# file -> (the expression, the reason).
WRITTEN_OUT = {
    "kernel_pack.h": ("off <= span && d.len <= span - off",
                      "in_umem: shard_counters 455 -> 457 instructions; 46.00 us against 44.56..45.80"),
    "kernel_forward.h": ("nch = ((off & 15) + len + 15) >> 4;",
                         "chunk_count: forward_frames reordered; config 4, three interfaces: 1123.89 us against "
                         "1118.85..1123.81 (inside the range in the three other cases)"),
}


@pytest.fixture(scope="module")
def grid(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ missing")
    exe = str(tmp_path_factory.mktemp("desc_rules") / "desc_rules_grid")
    subprocess.run(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-std=c++17", "-Iinclude", "tests/c/desc_rules_grid.cpp",
                    "-o", exe], cwd=ROOT, check=True)
    r = subprocess.run([exe], cwd=ROOT, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    head, *lines = r.stdout.splitlines()
    # (Python ints: addresses with bits 48..63 set do not fit an int64)
    return head, np.array([[int(x) for x in ln.split()] for ln in lines], dtype=object)


def test_out_of_range_marker(grid):
    assert grid[0] == f"out_of_range {1 << 47}"
    outside = np.zeros(1, dtype=frames.DESC_DTYPE)
    outside["len"] = 1                      # one byte in a UMEM of none: the restated layout marks it
    assert int(CC.packed_layout(outside, [0, 1], 0, 0)[0][0]) == 1 << 47


def test_grid_is_the_stated_one(grid):
    addr, ln, size, phase = (grid[1][:, k] for k in range(4))
    assert set(size) == set(SIZES) and set(phase) == set(range(16))
    for s in SIZES:
        m = size == s
        offs = {int((a & ((1 << 48) - 1)) + (a >> 48)) for a in addr[m]}
        assert offs == {0, 1, 15, 16, s - 1, s, s + 1}
        assert set(ln[m]) == {x for x in (0, 1, 15, 16, 17, 33, s, (1 << 32) - 1) if x < 1 << 32}
        his = {int(a >> 48) for a in addr[m]}
        assert his == {h for h in (0, 1, 65535) if h <= s + 1}        # (65535 needs an offset that large)
        # every offset that can hold it comes with and without a part in bits 48..63
        assert all({int(a >> 48) for a in addr[m] if (a & ((1 << 48) - 1)) + (a >> 48) == o} >= {0, 1}
                   for o in offs if o >= 1)


def test_every_line_matches_the_numpy_restatement(grid):
    rows = grid[1]
    for s in SIZES:
        for ph in range(16):
            r = rows[(rows[:, 2] == s) & (rows[:, 3] == ph)]
            d = np.zeros(r.shape[0], dtype=frames.DESC_DTYPE)
            d["addr"] = r[:, 0].astype(np.uint64)
            d["len"] = r[:, 1].astype(np.uint32)
            off, ln, inr, nch = CC.chunks(d, s, ph)
            assert np.array_equal(off, CC.offsets(d))
            assert np.array_equal(r[:, 4].astype(np.int64), off)
            assert np.array_equal(r[:, 5].astype(bool), inr)
            # chunks() counts no chunk for an entry of no bytes or outside the
            # UMEM, as the callers of chunk_count decide before they ask
            live = inr & (ln > 0)
            assert live.any() and (~live).any()
            assert np.array_equal(r[:, 6].astype(np.int64)[live], nch[live])
            assert np.array_equal(r[:, 7].astype(np.int64), 16 * r[:, 6].astype(np.int64))


def test_the_rules_are_stated_once():
    """The address translation and the marker occur in desc_rules.h alone; the
    kernels that keep a rule written out are the listed ones, once each, under a
    comment that names the rule."""
    src = {os.path.basename(p): open(p).read()
           for ext in ("h", "hip", "cpp") for p in glob.glob(os.path.join(CSRC, "*." + ext))}
    for text in ("XSKNF_GPU_UNALIGNED_BUF_OFFSET_SHIFT", "1ull << 47"):
        assert [f for f in sorted(src) if text in src[f]] == ["desc_rules.h"], text
    for f, (expr, reason) in WRITTEN_OUT.items():
        assert src[f].count(expr) == 1 and "// desc_rules.h " in src[f].split(expr)[0].splitlines()[-2], (f, reason)

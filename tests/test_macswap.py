"""The macswap NF on the CPU (include/xsknf_gpu.h "the macswap NF"):
xsknf_gpu_macswap_host (xsknf_amd/csrc/macswap_host.cpp), the model the device
call is held to -- against the numpy model of tests/macswap_cases.py and against
what the reference's own function left (tests/golden/macswap_golden.npz) -- and
the argument checks of both calls that come before any GPU call."""
import ctypes
import errno

import numpy as np
import pytest

from tests import macswap_cases as MC
from xsknf_amd import _lib, frames, macswap


def _same(umem, descs, ingress=0, action=MC.REDIRECT, double=False, nif=1, what=""):
    """macswap_host == the model on every byte and verdict; returns both."""
    before = umem.copy()
    hu, hv = macswap.macswap_host(umem, descs, ingress, action=action, double_macswap=double, num_interfaces=nif)
    assert np.array_equal(umem, before), "macswap_host wrote its input"
    mu, mv = MC.model(umem, descs, ingress, action, double, nif)
    assert np.array_equal(hv, mv), f"{what}: verdicts differ at {np.nonzero(hv != mv)[0][:8]}"
    assert np.array_equal(hu, mu), f"{what}: UMEM bytes differ at {np.nonzero(hu != mu)[0][:8]}"
    return hu, hv


def test_names_and_constants():
    import xsknf_amd
    assert (macswap.ACTION_REDIRECT, macswap.ACTION_DROP, macswap.ACTION_PASS) == (0, 1, 2)
    assert (xsknf_amd.MACSWAP_ACTION_REDIRECT, xsknf_amd.MACSWAP_ACTION_DROP, xsknf_amd.MACSWAP_ACTION_PASS) == (0, 1, 2)
    assert xsknf_amd.macswap_host is macswap.macswap_host and xsknf_amd.macswap_batch is macswap.macswap_batch
    assert ctypes.sizeof(_lib.MacswapOpts) == 16
    hdr = open(MC.ROOT + "/include/xsknf_gpu.h").read()
    for name, val in (("REDIRECT", 0), ("DROP", 1), ("PASS", 2)):
        assert f"#define XSKNF_MACSWAP_ACTION_{name} {val}" in hdr


def test_host_equals_the_model_on_the_builders_cases():
    rng = np.random.default_rng(31)
    for base in range(4):
        _same(*MC.packed(rng, 300, base), what=f"packed from {base}")
        _same(*MC.packed(rng, 300, base, lens=(14, 15, 17, 13)), ingress=1, nif=3, what=f"cycling from {base}")
    u, d = MC.phase_sweep(rng)
    hu, hv = _same(u, d, ingress=2, action=MC.PASS, nif=4, what="phases")
    assert (hv == 3).all() and np.count_nonzero(hu != u) > 11 * d.shape[0]
    _same(u, MC.unaligned_form(d, rng), what="phases, unaligned mode")
    _same(*MC.bounds_case(rng), nif=2, what="bounds")
    _same(*MC.uniform(rng, 1000), what="uniform")
    _same(*MC.mixed(rng), ingress=5, nif=7, what="mixed")


def test_host_equals_the_reference_fixture():
    """Frames and verdicts byte for byte what the reference's function left."""
    g = np.load(MC.GOLDEN)
    nb = int(g["batches"])
    assert nb == 26 and len(g["sources_sha256"]) == 3 and all(len(str(s).split()[0]) == 64 for s in g["sources_sha256"])
    seen, frames_in = set(), 0
    for b in range(nb):
        ingress, action, double, nif = (int(x) for x in g[f"params{b}"])
        descs = g[f"descs{b}"]
        assert descs.dtype == frames.DESC_DTYPE
        hu, hv = macswap.macswap_host(g[f"umem{b}"], descs, ingress, action=action, double_macswap=double,
                                      num_interfaces=nif)
        assert np.array_equal(hv, g[f"verdicts{b}"]), b
        assert np.array_equal(hu, g[f"after{b}"]), b
        mu, mv = MC.model(g[f"umem{b}"], descs, ingress, action, bool(double), nif)
        assert np.array_equal(mv, g[f"verdicts{b}"]) and np.array_equal(mu, g[f"after{b}"]), b
        seen.add((action, double, nif))
        frames_in += descs.shape[0]
    assert seen >= {(a, d, n) for a in MC.ACTIONS for d in (0, 1) for n in (1, 2, 3, 4)}
    assert 300 <= frames_in <= 1000
    # batch 0 holds every length 0..20 at every start phase, inside the UMEM
    d0 = g["descs0"]
    off = MC.offsets(d0)
    inside = off + d0["len"] <= g["umem0"].size
    assert {(int(ln), int(o) % 16) for ln, o in zip(d0["len"][inside], off[inside])} >= \
        {(ln, p) for ln in range(21) for p in range(16)}
    assert int(d0["len"][inside].max()) == 1514 and not inside.all()
    # ingress 0xffffffff wraps to interface 0 (batch 1: PASS, 3 interfaces)
    assert int(g["params1"][0]) == 0xffffffff and set(g["verdicts1"].tolist()) == {-1, 0}


def test_pass_is_a_redirect():
    """The reference's quirk on the AF_XDP path: only DROP is tested for."""
    rng = np.random.default_rng(32)
    u, d = MC.mixed(rng)
    for ingress, nif in ((0, 1), (0, 2), (6, 4), (0xffffffff, 5), (0xfffffffd, 0xffffffff)):
        ru, rv = macswap.macswap_host(u, d, ingress, action=macswap.ACTION_REDIRECT, num_interfaces=nif)
        pu, pv = macswap.macswap_host(u, d, ingress, action=macswap.ACTION_PASS, num_interfaces=nif)
        assert np.array_equal(rv, pv) and np.array_equal(ru, pu)
        assert set(rv.tolist()) == {-1, MC.verdict(MC.REDIRECT, ingress, nif)}
    assert MC.verdict(MC.PASS, 0xffffffff, 5) == 0 and MC.verdict(MC.PASS, 0xfffffffd, 0xffffffff) == -2
    du, dv = macswap.macswap_host(u, d, 0, action=macswap.ACTION_DROP, num_interfaces=0)
    assert (dv == -1).all() and np.array_equal(du, ru)   # DROP still swaps


def test_double_swap_leaves_the_umem_unchanged():
    rng = np.random.default_rng(33)
    for u, d in (MC.packed(rng, 200, 1), MC.mixed(rng), MC.bounds_case(rng)):
        hu, hv = _same(u, d, ingress=0, double=True, nif=2)
        assert np.array_equal(hu, u)
        su, sv = macswap.macswap_host(u, d, 0, num_interfaces=2)
        assert np.array_equal(hv, sv) and not np.array_equal(su, u)
        # twice through the single swap is the same thing
        assert np.array_equal(macswap.macswap_host(su, d, 0, num_interfaces=2)[0], u)


def test_length_13_against_14():
    rng = np.random.default_rng(34)
    u = rng.integers(0, 256, 64, dtype=np.uint8)
    for action in MC.ACTIONS:
        d = MC.descs_of([3, 20], [13, 14])
        hu, hv = _same(u, d, action=action, nif=2)
        assert hv.tolist() == [-1, -1 if action == MC.DROP else 1]
        assert np.array_equal(hu[:20], u[:20]) and np.array_equal(hu[32:], u[32:])
        assert np.array_equal(hu[20:26], u[26:32]) and np.array_equal(hu[26:32], u[20:26])


def test_rule_0_edges():
    rng = np.random.default_rng(35)
    size = 100
    u = rng.integers(0, 256, size, dtype=np.uint8)
    # a frame ending exactly at umem_size; one byte longer; starting at the end
    d = MC.descs_of([size - 14, size - 14, size - 20, size, size, size + 1], [14, 15, 21, 0, 1, 0])
    hu, hv = _same(u, d, nif=2)
    assert hv.tolist() == [1, -1, -1, -1, -1, -1]
    assert np.array_equal(hu[:size - 14], u[:size - 14]) and np.array_equal(hu[size - 14:size - 8], u[size - 8:size - 2])
    # unaligned-mode addresses: base | offset << 48
    d = MC.descs_of([10 | (30 << 48), (size - 14) | (1 << 48), ((1 << 48) - 1) | (0xffff << 48), 0 | (86 << 48)],
                    [14, 14, 14, 14])
    hu, hv = _same(u, d, nif=2)
    assert hv.tolist() == [1, -1, -1, 1]
    assert np.array_equal(hu[40:46], u[46:52]) and np.array_equal(hu[86:92], u[92:98])
    # every outside descriptor the builders know
    out = MC.outside_descs(size)
    hu, hv = _same(u, out)
    assert (hv == -1).all() and np.array_equal(hu, u)
    # an empty UMEM: every descriptor is outside it but the 0-byte one at 0, which is short
    e = np.zeros(0, dtype=np.uint8)
    hu, hv = _same(e, MC.descs_of([0, 0, 1], [0, 14, 0]))
    assert hv.tolist() == [-1, -1, -1] and hu.size == 0


def _opts(action=0, double=0, nif=1, reserved=0):
    return _lib.MacswapOpts(action, double, nif, reserved)


def test_argument_errors_and_empty_batches():
    lib = _lib.load()
    host, batch = lib.xsknf_gpu_macswap_host, lib.xsknf_gpu_macswap_batch
    u = np.zeros(64, dtype=np.uint8)
    d = MC.descs_of([0, 20], [14, 14])
    v = np.full(2, 99, dtype=np.int32)
    up, dp, vp = u.ctypes.data, d.ctypes.data, v.ctypes.data
    EINVAL = -errno.EINVAL
    bad_opts = [None, _opts(action=3), _opts(action=0xffffffff), _opts(action=MC.REDIRECT, nif=0),
                _opts(action=MC.PASS, nif=0), _opts(reserved=1)]
    for o in bad_opts:
        ref = None if o is None else ctypes.byref(o)
        assert host(up, 64, dp, 2, 0, ref, vp) == EINVAL
        assert host(None, 0, None, 0, 0, ref, None) == EINVAL          # the options come first, n == 0 included
        assert batch(None, 0, None, 0, 0, ref, None, None) == EINVAL
        assert batch(ctypes.c_void_p(16), 64, ctypes.c_void_p(16), 2, 0, ref, ctypes.c_void_p(16), None) == EINVAL
    assert (v == 99).all() and not u.any()
    good = ctypes.byref(_opts(nif=2))
    # DROP needs no interface (the reference never divides in DROP mode)
    drop0 = ctypes.byref(_opts(action=MC.DROP, nif=0))
    assert host(up, 64, dp, 2, 0, drop0, vp) == 0 and v.tolist() == [-1, -1]
    assert batch(None, 0, None, 0, 0, drop0, None, None) == 0
    # NULL buffers with n > 0
    v[:] = 99
    assert host(None, 64, dp, 2, 0, good, vp) == EINVAL
    assert host(up, 64, None, 2, 0, good, vp) == EINVAL
    assert host(up, 64, dp, 2, 0, good, None) == EINVAL
    assert (v == 99).all()
    # n == 0 succeeds, whatever the pointers
    assert host(None, 0, None, 0, 0, good, None) == 0
    assert host(up, 64, dp, 0, 7, good, vp) == 0 and (v == 99).all()
    hu, hv = macswap.macswap_host(u, d[:0])
    assert hv.size == 0 and np.array_equal(hu, u)
    # the device call's checks that come before any GPU call: n == 0, misaligned and NULL pointers
    p16 = ctypes.c_void_p(16)
    assert batch(None, 0, None, 0, 0, good, None, None) == 0
    assert batch(p16, 64, p16, 0, 0, good, p16, None) == 0
    assert batch(ctypes.c_void_p(8), 0, None, 0, 0, good, None, None) == EINVAL
    assert batch(None, 0, ctypes.c_void_p(8), 0, 0, good, None, None) == EINVAL
    assert batch(None, 0, None, 0, 0, good, ctypes.c_void_p(2), None) == EINVAL
    assert batch(None, 64, p16, 2, 0, good, p16, None) == EINVAL
    assert batch(p16, 64, None, 2, 0, good, p16, None) == EINVAL
    assert batch(p16, 64, p16, 2, 0, good, None, None) == EINVAL
    # the Python forms raise
    with pytest.raises(_lib.XsknfGpuError):
        macswap.macswap_host(u, d, action=3)
    with pytest.raises(_lib.XsknfGpuError):
        macswap.macswap_host(u, d, num_interfaces=0)
    with pytest.raises(ValueError):
        macswap.macswap_host(u.astype(np.int8), d)
    with pytest.raises(ValueError):
        macswap.macswap_host(u, np.zeros(4, dtype=np.uint64))


def test_options_are_read_at_the_call():
    """opts may be changed after the call returns: the host call keeps no pointer."""
    rng = np.random.default_rng(36)
    u, d = MC.packed(rng, 16, 1)
    o = _opts(action=MC.REDIRECT, nif=4)
    a, b = u.copy(), u.copy()
    va, vb = np.zeros(16, dtype=np.int32), np.zeros(16, dtype=np.int32)
    host = _lib.load().xsknf_gpu_macswap_host
    assert host(a.ctypes.data, a.size, d.ctypes.data, 16, 2, ctypes.byref(o), va.ctypes.data) == 0
    o.action, o.double_macswap = MC.DROP, 1
    assert host(b.ctypes.data, b.size, d.ctypes.data, 16, 2, ctypes.byref(o), vb.ctypes.data) == 0
    assert (va == 3).all() and (vb == -1).all() and np.array_equal(b, u) and not np.array_equal(a, u)

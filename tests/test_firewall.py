"""The firewall NF on the CPU (include/xsknf_gpu.h "the firewall NF"): the ACL
file parser and table builder (xsknf_amd/csrc/acl.cpp) and
xsknf_gpu_firewall_host (firewall_host.cpp), the model the device lookup is held
to -- against the dict model of tests/firewall_cases.py and against the recorded
verdicts of the reference's own function (tests/golden/firewall_golden.npz)."""
import errno
import json
import time

import numpy as np
import pytest

from tests import firewall_cases as FC
from xsknf_amd import _lib, firewall, frames


@pytest.fixture(scope="module")
def golden():
    g = np.load(FC.GOLDEN)
    return {k: g[k] for k in g.files}


def _golden_case(golden, tmp_path):
    p = tmp_path / "acl.txt"
    p.write_bytes(golden["acl_text"].tobytes())
    descs = golden["descs"].copy().view(frames.DESC_DTYPE).reshape(-1)
    return golden["umem"], descs, str(p)


def test_model_host_and_fixture_agree(golden, tmp_path):
    """The reference function's recorded verdicts, the dict model and
    xsknf_gpu_firewall_host over the parsed ACL file: equal on every frame."""
    umem, descs, path = _golden_case(golden, tmp_path)
    rules = firewall.parse_acl(path)
    want = golden["verdicts"]
    assert np.array_equal(FC.model(umem, descs, FC.acl_dict(rules)), want)
    with firewall.Acl.from_file(path) as acl:
        assert np.array_equal(firewall.firewall_host(umem, descs, acl), want)
    meta = json.loads(golden["meta"].tobytes())
    assert len(meta["sha256"]) == 6 and all(len(h) == 64 for h in meta["sha256"].values())


def test_fixture_holds_every_branch(golden):
    """Every way out of rules 1-7 occurs in the fixture, ihl 0..15 reach the map,
    and among the lookups are hits of every action, near misses and misses."""
    umem = golden["umem"]
    descs = golden["descs"].copy().view(frames.DESC_DTYPE).reshape(-1)
    assert descs.shape[0] <= 3000 and int(descs["len"].max()) <= 130
    buf = umem.tobytes()
    seen, ihls = set(), set()
    for addr, ln in zip(descs["addr"].tolist(), descs["len"].tolist()):
        off = (addr & ((1 << 48) - 1)) + (addr >> 48)
        f = buf[off:off + ln]
        v, key = FC.frame_key(f)
        if ln < 14:
            seen.add("short-eth")
        elif f[12:14] != b"\x08\x00":
            seen.add("not-ip")
        elif ln < 34:
            seen.add("short-ip")
        elif f[23] not in (6, 17):
            seen.add("other-proto")
        elif key is None:
            seen.add("short-tcp" if f[23] == 6 else "short-udp")
        else:
            seen.add("tcp" if f[23] == 6 else "udp")
            ihls.add(f[14] & 15)
    assert seen == {"short-eth", "not-ip", "short-ip", "other-proto", "short-tcp", "short-udp", "tcp", "udp"}
    assert ihls == set(range(16))
    assert set(np.unique(golden["verdicts"]).tolist()) == {-7, -1, 0, 1, 2, 31, 9999}


def test_decision_sweep_on_the_host():
    """ihl x protocol x ethertype x length x start phase, with descriptors
    outside the UMEM among them and the last frame ending on the UMEM's last
    byte: firewall_host equals the model."""
    rng = np.random.default_rng(5)
    fl, ph = FC.decision_frames(rng, phases=(0, 7, 15))
    umem, descs = FC.pack_unaligned(fl, rng, ph)
    last = descs[-1]
    assert (int(last["addr"]) & ((1 << 48) - 1)) + (int(last["addr"]) >> 48) + int(last["len"]) == umem.size
    rules = FC.hit_miss_acl(FC.keys_of(umem, descs), rng)
    descs = FC.with_outside(umem, descs, rng)
    want = FC.model(umem, descs, FC.acl_dict(rules))
    assert {-1, 0, 1, 2, 31, 0x7fffffff, -7} <= set(want.tolist())
    with firewall.Acl.from_rules(rules) as acl:
        assert np.array_equal(firewall.firewall_host(umem, descs, acl), want)
    au, ad = FC.pack_aligned(fl[::7], rng)
    rules = FC.hit_miss_acl(FC.keys_of(au, ad), rng)
    with firewall.Acl.from_rules(rules) as acl:
        assert np.array_equal(firewall.firewall_host(au, ad, acl), FC.model(au, ad, FC.acl_dict(rules)))


# ---- the parser ----------------------------------------------------------------

def _parse_text(tmp_path, text):
    p = tmp_path / "a.txt"
    p.write_text(text)
    return firewall.parse_acl(str(p))


def _rc(tmp_path, text):
    p = tmp_path / "bad.txt"
    p.write_bytes(text if isinstance(text, bytes) else text.encode())
    n = __import__("ctypes").c_uint32(0)
    return _lib.load().xsknf_gpu_acl_parse(str(p).encode(), None, 0, n)


def test_parser_round_trips_the_reference_format(tmp_path):
    rng = np.random.default_rng(9)
    rules = FC.random_rules(rng, 500)
    rules["action"][::5] = -1
    rules["action"][1::5] = rng.integers(-999, 9999, 100)
    got = _parse_text(tmp_path, FC.acl_text(rules))
    assert got.tobytes() == rules.tobytes()
    # any white space separates, as fscanf's
    txt = FC.acl_text(rules[:3]).replace(" ", "\t \n", 4)
    assert _parse_text(tmp_path, "  " + txt + "\n\n").tobytes() == rules[:3].tobytes()
    assert _parse_text(tmp_path, "0\n").size == 0


def test_parser_actions_ports_and_addresses(tmp_path):
    r = _parse_text(tmp_path, "6\n"
                              "10.0.0.1 10.0.0.2 80 443 TCP DROP\n"
                              "10.0.0.1 10.0.0.2 80 443 UDP 3\n"
                              "10.0.0.1 10.0.0.2 65536 131073 UDP abc\n"      # atoi -> 0; ports -> 0, 1
                              "10.0.0.1 10.0.0.2 4294967295 70000 TCP -12\n"  # ports -> 65535, 4464
                              "1.2.3 0x7f.1 1 2 TCP 7x\n"                     # inet_aton's short and hex forms; atoi -> 7
                              "255.255.255.255 0.0.0.0 0 0 UDP drop\n")       # only DROP drops
    assert r["action"].tolist() == [-1, 3, 0, -12, 7, 0]
    assert r["proto"].tolist() == [6, 17, 17, 6, 6, 17]
    assert bytes(r[0:1].view(np.uint8)[:12]) == bytes([10, 0, 0, 1, 10, 0, 0, 2, 0, 80, 1, 187])
    assert [int.from_bytes(int(x).to_bytes(2, "little"), "big") for x in r["sport"]] == [80, 80, 0, 65535, 1, 0]
    assert [int.from_bytes(int(x).to_bytes(2, "little"), "big") for x in r["dport"]] == [443, 443, 1, 4464, 2, 0]
    assert bytes(r[4:5].view(np.uint8)[:8]) == bytes([1, 2, 0, 3, 127, 0, 0, 1])
    assert not r["pad"].any()


def test_parser_duplicates_the_last_wins(tmp_path):
    r = _parse_text(tmp_path, "3\n1.1.1.1 2.2.2.2 5 6 TCP 4\n9.9.9.9 2.2.2.2 5 6 TCP 1\n1.1.1.1 2.2.2.2 5 6 TCP DROP\n")
    assert r.size == 3
    u, d = FC.frames_for_rules(r, np.random.default_rng(1))
    with firewall.Acl.from_rules(r) as acl:
        assert acl.info["rules"] == 2
        assert firewall.firewall_host(u, d, acl).tolist() == [-1, 1, -1]
    with firewall.Acl.from_rules(r[::-1]) as acl:
        assert firewall.firewall_host(u, d, acl).tolist() == [4, 1, 4]


@pytest.mark.parametrize("text", [
    "2\n1.1.1.1 2.2.2.2 5 6 TCP 4\n",                                   # fewer records than the count
    "1\n1.1.1.1 2.2.2.2 5 6 TCP 4\n1.1.1.1 2.2.2.2 5 7 TCP 4\n",        # more
    "1\n1.1.1.1 2.2.2.2 5 6 ICMP 4\n",                                  # unknown protocol
    "1\n1.1.1.1 2.2.2.2 5 6 tcp 4\n",
    "1\n1.1.1.1 2.2.2.2 5 6 TCPX 4\n",                                  # longer than proto[4]
    "1\n1.1.1.256 2.2.2.2 5 6 TCP 4\n",                                 # inet_aton rejects
    "1\n1.1.1.1 example 5 6 TCP 4\n",
    "1\n100.100.100.1000 2.2.2.2 5 6 TCP 4\n",                          # longer than saddr[16]
    "1\n1.1.1.1 2.2.2.2 5 6 TCP 12345\n",                               # longer than action[5]
    "1\n1.1.1.1 2.2.2.2 5x 6 TCP 4\n",                                  # not a decimal port
    "1\n1.1.1.1 2.2.2.2 -5 6 TCP 4\n",
    "1\n1.1.1.1 2.2.2.2 5 4294967296 TCP 4\n",
    "1\n1.1.1.1 2.2.2.2 5 6 TCP\n",                                     # a record cut short
    "x\n", "", "-1\n",
    "1000001\n",                                                        # more than MAX_ACL_SIZE
    b"1\n1.1.1.1 2.2.2.2 5 6 TCP 4\x00\n",
])
def test_parser_rejects(tmp_path, text):
    assert _rc(tmp_path, text) == -errno.EINVAL


def test_parser_files_and_arguments(tmp_path):
    import ctypes
    lib = _lib.load()
    n = ctypes.c_uint32(7)
    assert lib.xsknf_gpu_acl_parse(str(tmp_path / "missing.txt").encode(), None, 0, n) == -errno.ENOENT
    assert lib.xsknf_gpu_acl_parse(str(tmp_path).encode(), None, 0, n) in (-errno.EISDIR, -errno.EINVAL)
    with pytest.raises(_lib.XsknfGpuError):
        firewall.parse_acl(str(tmp_path / "missing.txt"))
    p = tmp_path / "two.txt"
    p.write_text("2\n1.1.1.1 2.2.2.2 5 6 TCP 4\n1.1.1.1 2.2.2.2 5 6 UDP 4\n")
    assert lib.xsknf_gpu_acl_parse(None, None, 0, n) == -errno.EINVAL
    assert lib.xsknf_gpu_acl_parse(str(p).encode(), None, 0, None) == -errno.EINVAL
    assert lib.xsknf_gpu_acl_parse(str(p).encode(), None, 1, n) == -errno.EINVAL
    # a buffer too small: the count comes back, the first `cap` rules are written
    one = np.zeros(2, dtype=firewall.RULE_DTYPE)
    assert lib.xsknf_gpu_acl_parse(str(p).encode(), one.ctypes.data, 1, n) == -errno.ENOSPC and n.value == 2
    assert one["proto"].tolist() == [6, 0]


# ---- the table -----------------------------------------------------------------

def test_table_finds_every_key_and_info_is_consistent():
    rng = np.random.default_rng(11)
    rules = FC.random_rules(rng, 5000)
    rules[4000:] = rules[:1000]              # duplicates, with new actions
    rules["action"][4000:] = 77
    u, d = FC.frames_for_rules(rules, rng)
    want = FC.model(u, d, FC.acl_dict(rules))
    assert (want[:1000] == 77).all()
    for slots in (0, 4096, 8192, 1 << 16):
        with firewall.Acl.from_rules(rules, slots) as acl:
            i = acl.info
            assert i["rules"] == 4000 and i["slots"] == (slots or 16384) and 1 <= i["max_probe"] < i["slots"]
            assert i["device_bytes"] in (0, 20 * i["slots"])
            assert np.array_equal(firewall.firewall_host(u, d, acl), want)
    # deterministic: the same probes in another run
    with firewall.Acl.from_rules(rules) as a, firewall.Acl.from_rules(rules.copy()) as b:
        assert a.info == b.info


def test_slots_validation():
    rng = np.random.default_rng(12)
    rules = FC.random_rules(rng, 64)
    lib = _lib.load()
    import ctypes
    h = ctypes.c_void_p()
    for bad in (1, 3, 48, 63, 64, 100, (1 << 24) + 1, 1 << 25, 0xffffffff):   # no power of two, not > 64 keys, too large
        assert lib.xsknf_gpu_acl_create(ctypes.byref(h), rules.ctypes.data, 64, bad) == -errno.EINVAL, bad
    assert lib.xsknf_gpu_acl_create(None, rules.ctypes.data, 64, 0) == -errno.EINVAL
    assert lib.xsknf_gpu_acl_create(ctypes.byref(h), None, 64, 0) == -errno.EINVAL
    assert lib.xsknf_gpu_acl_info(None, None) == -errno.EINVAL and lib.xsknf_gpu_acl_destroy(None) == -errno.EINVAL
    with firewall.Acl.from_rules(rules, 128) as acl:
        assert acl.info["slots"] == 128
    rules[1:] = rules[0]                     # 64 rules of one key fit 2 slots
    with firewall.Acl.from_rules(rules, 2) as acl:
        assert acl.info["rules"] == 1 and acl.info["slots"] == 2
    with firewall.Acl.from_rules(rules, 1 << 10) as acl:
        acl.close()
        acl.close()
        with pytest.raises(ValueError):
            acl.info


def test_empty_acl_and_rules_that_cannot_match():
    rng = np.random.default_rng(13)
    rules = FC.random_rules(rng, 10)
    u, d = FC.frames_for_rules(rules, rng)
    with firewall.Acl.from_rules(rules[:0]) as acl:
        assert acl.info["rules"] == 0 and acl.info["slots"] == 64 and acl.info["max_probe"] == 0
        assert not firewall.firewall_host(u, d, acl).any()
        assert firewall.firewall_host(u, d[:0], acl).size == 0
    other = rules.copy()
    other["proto"] = [0, 1, 2, 5, 7, 16, 18, 47, 255, 6]
    with firewall.Acl.from_rules(other) as acl:
        assert acl.info["rules"] == 1
    # pad bytes are ignored
    padded = rules.copy()
    padded["pad"] = 0xa5
    with firewall.Acl.from_rules(padded) as acl:
        assert np.array_equal(firewall.firewall_host(u, d, acl), rules["action"])


def test_full_table_on_the_host():
    """1023 rules in 1024 slots: clusters wrap past the last slot and a miss
    probes to the one empty slot."""
    rules, u, d = FC.full_table_case()
    want = FC.model(u, d, FC.acl_dict(rules))
    assert np.array_equal(want[:1023], rules["action"]) and not want[1023:].any()
    with firewall.Acl.from_rules(rules, 1024) as acl:
        assert acl.info["rules"] == 1023 and acl.info["max_probe"] > 64
        assert np.array_equal(firewall.firewall_host(u, d, acl), want)


def test_a_million_rules():
    """The reference harness's largest ACL: 1,000,000 random rules, 65,536 hits
    and 65,536 near misses against the dict."""
    rules, u, d, want = FC.million_case()
    assert np.count_nonzero(want[:65536]) > 60000   # (action 0 is one of 33)
    t0 = time.perf_counter()
    acl = firewall.Acl.from_rules(rules)
    dt = time.perf_counter() - t0
    with acl:
        i = acl.info
        print(f"1M-rule ACL: built in {dt:.3f} s, {i}")
        assert i["slots"] == 1 << 21 and i["rules"] == len(FC.rules_dict_fast(rules)) and i["max_probe"] < 200
        assert np.array_equal(firewall.firewall_host(u, d, acl), want)
    assert not want[65536:].any()


def test_firewall_host_arguments():
    import ctypes
    lib = _lib.load()
    v = np.zeros(4, dtype=np.int32)
    d = np.zeros(4, dtype=frames.DESC_DTYPE)
    u = np.zeros(64, dtype=np.uint8)
    with firewall.Acl.from_rules(np.zeros(0, dtype=firewall.RULE_DTYPE)) as acl:
        h = acl.handle
        assert lib.xsknf_gpu_firewall_host(u.ctypes.data, 64, d.ctypes.data, 4, None, v.ctypes.data) == -errno.EINVAL
        assert lib.xsknf_gpu_firewall_host(None, 64, d.ctypes.data, 4, h, v.ctypes.data) == -errno.EINVAL
        assert lib.xsknf_gpu_firewall_host(u.ctypes.data, 64, None, 4, h, v.ctypes.data) == -errno.EINVAL
        assert lib.xsknf_gpu_firewall_host(u.ctypes.data, 64, d.ctypes.data, 4, h, None) == -errno.EINVAL
        assert lib.xsknf_gpu_firewall_host(None, 0, None, 0, h, None) == 0
        # the device call's checks that come before any GPU call
        f = lib.xsknf_gpu_firewall_batch
        assert f(None, 0, None, 0, None, None, None) == -errno.EINVAL
        assert f(None, 0, None, 0, h, None, None) == 0
        assert f(ctypes.c_void_p(8), 0, None, 0, h, None, None) == -errno.EINVAL
        assert f(None, 0, ctypes.c_void_p(8), 0, h, None, None) == -errno.EINVAL
        assert f(None, 0, None, 0, h, ctypes.c_void_p(2), None) == -errno.EINVAL
        assert f(None, 64, ctypes.c_void_p(16), 4, h, ctypes.c_void_p(16), None) == -errno.EINVAL
        assert f(ctypes.c_void_p(16), 64, None, 4, h, ctypes.c_void_p(16), None) == -errno.EINVAL
        assert f(ctypes.c_void_p(16), 64, ctypes.c_void_p(16), 4, h, None, None) == -errno.EINVAL

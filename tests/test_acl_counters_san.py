"""The ACL's hit counters under AddressSanitizer + UBSan, as a stand-alone
program (tests/c/san_acl_counters.c) -- CPU only, nothing preloaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_acl_counters_are_sanitizer_clean(tmp_path):
    """xsknf_amd/csrc/acl.cpp (built without its device side: XSKNF_ACL_HOST_ONLY)
    and firewall_host.cpp through random updates and batches against an
    open-coded model, every buffer exactly as long as its contents."""
    if not shutil.which("g++"):
        pytest.skip("g++ missing")
    exe = str(tmp_path / "san_acl_counters")
    subprocess.run(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-Iinclude", "-DXSKNF_ACL_HOST_ONLY", "-x", "c",
                    "tests/c/san_acl_counters.c", "-x", "c++", "-std=c++17", "xsknf_amd/csrc/acl.cpp",
                    "xsknf_amd/csrc/firewall_host.cpp", "-o", exe], cwd=ROOT, check=True)
    r = subprocess.run([exe], cwd=ROOT, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip() == "ok 664"

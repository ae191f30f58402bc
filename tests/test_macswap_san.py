"""The macswap NF's host model under AddressSanitizer + UBSan, as a stand-alone
program (tests/c/san_macswap.c) -- CPU only, nothing preloaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_macswap_host_is_sanitizer_clean(tmp_path):
    """xsknf_amd/csrc/macswap_host.cpp on 600 random batches, every buffer
    exactly as long as its contents, and a 14-byte frame in the UMEM's last 14
    bytes."""
    if not shutil.which("g++"):
        pytest.skip("g++ missing")
    exe = str(tmp_path / "san_macswap")
    subprocess.run(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-Iinclude", "-x", "c", "tests/c/san_macswap.c", "-x", "c++",
                    "-std=c++17", "xsknf_amd/csrc/macswap_host.cpp", "-o", exe], cwd=ROOT, check=True)
    r = subprocess.run([exe], cwd=ROOT, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip() == "ok 600"

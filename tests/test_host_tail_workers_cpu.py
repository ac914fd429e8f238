"""The host tail's hash workers under the host sanitizers: tools/host_tail_check.cpp (its own
main; producer threads raise the ready flags out of order) built with the workers' source, once
with AddressSanitizer + UBSan and once with ThreadSanitizer, and run directly. Nothing is loaded
into Python. No GPU needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("san", ["address,undefined", "thread"])
def test_workers_under_sanitizer(san, tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "host_tail_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", f"-fsanitize={san}", "-fno-sanitize-recover=all",
                    "-pthread", os.path.join(ROOT, "tools", "host_tail_check.cpp"),
                    os.path.join(ROOT, "bs_amd", "csrc", "host_sha256.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host_tail_check: ok" in r.stdout

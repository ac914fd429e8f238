"""The library's own host SHA-256 (bs_amd/csrc/host_sha256.cpp), both implementations, against
hashlib: the padding edges, a multi-block length, unaligned starts and the FIPS vectors. The x86
SHA-extension implementation is skipped where cpuid lacks it. No GPU needed."""
import ctypes
import hashlib

import numpy as np
import pytest

from conftest import load_json

PORTABLE, X86 = 0, 1
LENGTHS = [0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128, 64 * 37 + 29]


@pytest.fixture(scope="module")
def sha():
    from bs_amd import build, bsgpu
    build.build()
    L = bsgpu.lib()

    def run(impl, buf: np.ndarray, start: int, n: int):
        out = (ctypes.c_uint8 * 32)()
        rc = L.bsg_host_sha256_debug(buf.ctypes.data + start, n, impl, out)
        if rc == 1:
            pytest.skip("cpuid reports no SHA extensions on this host")
        assert rc == 0
        return bytes(out).hex()
    return run


def _bytes(n, seed=7):
    return np.random.default_rng(seed).integers(0, 256, size=n + 8, dtype=np.uint8)


@pytest.mark.parametrize("impl", [PORTABLE, X86], ids=["portable", "x86"])
def test_lengths_and_unaligned_starts(sha, impl):
    for n in LENGTHS:
        buf = _bytes(n, seed=n + 1)
        for start in range(4):
            want = hashlib.sha256(buf[start:start + n].tobytes()).hexdigest()
            assert sha(impl, buf, start, n) == want, (n, start)


@pytest.mark.parametrize("impl", [PORTABLE, X86], ids=["portable", "x86"])
def test_fips_vectors(sha, impl):
    kat = load_json("sha256_kat.json")
    for msg, want in kat["fips"].items():
        buf = np.frombuffer(msg.encode() + b"\0" * 8, dtype=np.uint8).copy()
        assert sha(impl, buf, 0, len(msg)) == want, msg
    buf = np.full(1_000_000 + 8, ord("a"), dtype=np.uint8)
    assert sha(impl, buf, 0, 1_000_000) == kat["million_a"]

"""One bsg_pool_put_blobs and one bsg_pool_get past a single pass of every grid, past the prefix
sum's two-parts-per-thread point and past one hash batch (65,535 blobs), against the model of
blob_cases.py: the pool in full, where[], the refs; idx, out_off and the output's bytes."""
import numpy as np
import pytest

import blob_cases as B
import dedup_cases as DC
import pool_cases as P
from bs_amd.synth import splitmix_array
from test_gpu_pool_merge import _is
from test_gpu_tier_counts import cus  # noqa: F401  (the device's CU count, a fixture)

pytestmark = pytest.mark.gpu


def test_put_and_get_past_one_pass(gpu, cus):  # noqa: F811
    t, n0 = DC.wide_counts(cus)
    n = n0 + 3001
    # item i: 1 - 25 splitmix bytes at 32 i; every fifth item coincides with an earlier one
    src = np.concatenate([splitmix_array(0xB10B, 32 * n), np.zeros(256, np.uint8)])
    i = np.arange(n, dtype=np.int64)
    at = np.where(i % 5 == 4, (i * 2654435761 >> 11) % np.maximum(i, 1), i)
    at -= at % 5 == 4                                              # (an original, not a repeat)
    off, lens = 32 * at, 1 + (at * 2654435761 >> 7) % 25
    # (four items in five are new: with n barely past t that is fewer than t, so it is the items,
    # the requests and the table that pass a grid's single trip, not the new blobs)
    assert (at <= i).all() and n > t and int((at != i).sum()) > n // 6
    assert n > 8 * 65535 and lens.min() == 1 and lens.max() == 25

    cap = (32 * n, n)
    m, pool, eng = P.Model(*cap), gpu.Pool(*cap), gpu.Engine()
    buf = gpu.DeviceBuffer(len(src))
    try:
        buf.from_host(src)
        rc, info, refs = pool.put_blobs(eng, buf, off, lens)
        want = B.put_blobs(m, src, off, lens)
        assert rc == want[0] == B.OK and info == want[1], (rc, info, want[1])
        assert info["added"] > 6 * 65535 and info["repeats"] > n // 6 and info["known"] == 0
        assert refs.tobytes() == b"".join(want[2])
        _is(gpu, pool, m)
        assert pool.where().tobytes() == m.where.tobytes()

        # every ref in reversed order, every seventh replaced by one the pool lacks
        ask = np.frombuffer(refs.tobytes(), dtype=np.uint8).reshape(n, 32)[::-1].copy()
        ask[::7] = splitmix_array(0x5EED, 32 * len(ask[::7])).reshape(-1, 32)
        rc, winfo, widx, woff, _ = B.get(m, [r.tobytes() for r in ask], None)
        assert winfo["missing"] == len(ask[::7]) and len(ask) > t
        out = gpu.DeviceBuffer(winfo["need_bytes"] + 64)
        try:
            out.from_host(np.full(out.nbytes, 0xA5, dtype=np.uint8))
            rc, ginfo, idx, out_off = pool.get(eng, ask, out.ptr, out_cap=winfo["need_bytes"])
            assert rc == B.OK and ginfo == winfo, (rc, ginfo, winfo)
            assert idx.tobytes() == widx.tobytes() and out_off.tobytes() == woff.tobytes()
            got = out.to_host()
            assert got[:-64].tobytes() == B.get_gather(m, widx, woff).tobytes()
            assert (got[-64:] == 0xA5).all()
        finally:
            out.free()
        _is(gpu, pool, m)
    finally:
        buf.free()
        pool.free()
        eng.close()

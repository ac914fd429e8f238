"""bsg_engine_pool_put past one pass of its grids, against the model of pool_cases.py, every
result for equality.

A launch is capped at T = 8 x CUs x 256 threads (engine_grid), read from the source and the device
as tests/test_gpu_dedup_wide.py reads it; N0 = max(T, 256 x kSumTile) is the count from which
k_sum_mid also sums several parts per thread. The run is dedup_cases.wide_run: more than N0 records
of at most some 25 bytes, more than T of them new, so one put has more than T new blobs (the second
trip of the first-occurrence pass, of k_pool_plan, k_pool_append and its index inserts and of
k_pool_where; the aligned prefix with several parts per thread; seg_find over more than T segments
in k_pool_gather), and a second put of the same run looks more than T items up among more than T
keys and adds nothing."""
import numpy as np
import pytest

import dedup_cases as DC
import pool_cases as P
from test_gpu_dedup import _records, _run
from test_gpu_tier_counts import cus  # noqa: F401  (the device's CU count, a fixture)

pytestmark = pytest.mark.gpu


def _equal(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert len(got) == len(want), (name, len(got), len(want))
    bad = np.flatnonzero(got != want)
    assert not len(bad), (name, len(bad), int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))


def _same(pool, m):
    st = pool.stat()
    assert st == m.stat(), (st, m.stat())
    table, want = pool.table(), m.blobs()
    for f in ("off", "len"):
        _equal(f, table[f], want[f])
    assert table["ref"].tobytes() == want["ref"].tobytes()
    _equal("bytes", pool.to_host(P.align16(st["bytes"])), m.buf)   # in full, padding included
    _equal("where", pool.where(), m.where)


def test_wide_put_and_again(gpu, oracle, table, cus):  # noqa: F811
    t, n0 = DC.wide_counts(cus)
    case, want_recs = DC.wide_run(oracle, table, cus)
    streams, bits, mn = case
    host, off, lens = DC.place(streams)
    eng = gpu.Engine()
    buf = pool = None
    try:
        buf = _run(gpu, eng, host, off, lens, bits, mn)
        recs = _records(gpu, oracle, table, eng, streams, bits, mn)
        _, _, nodes, arena = eng.trees()
        run = (recs, streams, nodes, arena)
        items = len(recs) + len(nodes)
        cap = (int(((recs["len"].astype(np.int64) + 15) & ~15).sum()) + len(arena), items)
        pool, m = gpu.Pool(*cap), P.Model(*cap)
        rc, want = m.put(run)
        assert rc == P.OK and want["added"] > t + 100 and want["items"] > n0 + 100
        assert want["repeats"] >= 1000 and len(nodes) > 1000
        info = eng.pool_put(pool)
        assert info == want, (info, want)
        _same(pool, m)
        rc, want = m.put(run)
        assert rc == P.OK and want["added"] == 0 and want["known"] == items
        before = (pool.table().tobytes(), pool.to_host().tobytes())
        info = eng.pool_put(pool)
        assert info == want, (info, want)
        assert (pool.table().tobytes(), pool.to_host().tobytes()) == before
        _same(pool, m)
    finally:
        eng.close()
        for x in (buf, pool):
            if x is not None:
                x.free()

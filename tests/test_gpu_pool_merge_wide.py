"""bsg_pool_merge past one pass of its grids, against the model of merge_cases.py, every result
for equality.

A launch is capped at T = 8 x CUs x 256 threads (engine_grid). The source is
tests/test_gpu_pool_collect_wide.py's pool: dedup_cases.wide_run put once, more than T blobs of at
most some 25 bytes and a few thousand nodes, fewer than 2 T in all, so one merge cannot both
append and know more than T of them. Two merges share the work. The first goes into a pool that
holds what the 80 excerpts' and the copy's Roots reach and selects the main stream's Root: more
than T selected, more than T appended, new and dead blobs on both sides of the pass boundary. The
excerpts' streams come first in the run, so the chunks they share with the main stream, the known
ones, are some 26,000 entries at the table's start. The second
goes into a pool that holds what the main stream's Root reaches and selects every blob: more than
T selected, more than T known on both sides of the boundary, and the blobs only the other Roots
reach (chunks at the excerpts' cut ends at the table's start, their nodes at its end) appended
from both sides of it. In both, k_pool_probe, k_pool_merge_end and
k_pool_merge_append make a second trip and the gather's seg_find runs over more than a grid of
segments."""
import numpy as np
import pytest

import collect_cases as C
import dedup_cases as DC
import gc_cases as G
import merge_cases as M
import pool_cases as P
import walk_cases as W
from test_gpu_dedup import _records, _run
from test_gpu_pool_wide import _equal
from test_gpu_tier_counts import cus  # noqa: F401  (the device's CU count, a fixture)

pytestmark = pytest.mark.gpu


def _held(gpu, eng, src, m, roots, cap, marked):
    """A pool that holds what `roots` reach of src, by a collect, and its model (a merge into an
    empty pool, which tests/test_merge_cases_cpu.py holds to collect_cases.collect)."""
    rc, _, _, md, _ = M.merge(m, P.Model(*cap), roots, marked=marked)
    assert rc == M.OK
    dst = gpu.Pool(*cap)
    assert eng.pool_collect(src, dst, W.roots_array(roots))[0] == C.OK
    return dst, md


def _check(dst, want):
    rc, status, info, md, remap = want
    st = dst.stat()
    assert st == md.stat(), (st, md.stat())
    tb, wt = dst.table(), md.blobs()
    for f in ("off", "len"):
        _equal(f, tb[f], wt[f])
    assert tb["ref"].tobytes() == wt["ref"].tobytes()
    _equal("bytes", dst.to_host(P.align16(st["bytes"])), md.buf)      # in full, padding included
    _equal("remap", dst.remap(), remap)


def test_wide_merge(gpu, oracle, table, cus):  # noqa: F811
    t, _ = DC.wide_counts(cus)
    case, _ = DC.wide_run(oracle, table, cus)
    streams, bits, mn = case
    host, off, lens = DC.place(streams)
    eng = gpu.Engine()
    buf = src = d1 = d2 = None
    try:
        buf = _run(gpu, eng, host, off, lens, bits, mn)
        recs = _records(gpu, oracle, table, eng, streams, bits, mn)
        roots, _, nodes, arena = eng.trees()
        run = (recs, streams, nodes, arena)
        cap = (int(((recs["len"].astype(np.int64) + 15) & ~15).sum()) + len(arena) + 16,
               len(recs) + len(nodes))
        src, m = gpu.Pool(*cap), P.Model(*cap)
        rc, put = m.put(run)
        assert rc == P.OK and eng.pool_put(src) == put
        main = [roots[DC.WIDE_EXCERPTS].tobytes()]
        rest = [r.tobytes() for k, r in enumerate(roots) if k != DC.WIDE_EXCERPTS]
        before = (src.stat(), src.table().tobytes())
        n = len(m.table)
        assert t < n < 2 * t

        # 1. the main stream's Root into a pool that holds the other streams
        blobs, pb = m.blobs(), m.stat()["pool_bytes"]
        mk_main = G.mark(m.blob_bytes, blobs, main, pb)         # each mark once: they take seconds
        mk_rest = G.mark(m.blob_bytes, blobs, rest, pb)
        d1, m1 = _held(gpu, eng, src, m, rest, cap, mk_rest)
        want = M.merge(m, m1, main, marked=mk_main)
        info, remap = want[2], want[4]
        assert want[0] == M.OK and info["selected"] > t and info["added"] > t, (info, t)
        known = np.flatnonzero((remap != M.NONE) & (remap < len(m1.table)))
        new = np.flatnonzero((remap != M.NONE) & (remap >= len(m1.table)))
        dead = np.flatnonzero(remap == M.NONE)
        assert len(known) >= 1000 and len(new) == info["added"]
        assert new[0] < t < new[-1], (new[0], new[-1], t)
        assert len(dead) >= 1000 and dead[0] < t < dead[-1], (len(dead), t)
        got = eng.pool_merge(src, d1, W.roots_array(main))
        assert got[0] == M.OK and got[1] == info and got[2].tolist() == want[1].tolist()
        _check(d1, want)

        # 2. every blob into a pool that holds the main stream
        d2, m2 = _held(gpu, eng, src, m, main, cap, mk_main)
        want = M.merge(m, m2, None, M.ALL)
        info, remap = want[2], want[4]
        assert want[0] == M.OK and info["selected"] == n and info["known"] > t, (info, t)
        new = np.flatnonzero(remap >= len(m2.table))
        assert len(new) == info["added"] >= 1000 and new[0] < t < new[-1], (len(new), t)
        got = eng.pool_merge(src, d2, all=True, verify=True)
        want[2]["verified"] = info["added_bytes"]
        assert got[0] == M.OK and got[1] == want[2] and len(got[2]) == 0
        _check(d2, want)
        assert (src.stat(), src.table().tobytes()) == before

        # the main stream walks the same on both destinations and on the source
        res = []
        for pool in (d1, d2, src):
            rc, winfo, wstatus = eng.pool_walk(pool, W.roots_array(main))
            assert rc == W.OK, (rc, winfo)
            res.append((winfo, wstatus.tolist(), [x.tobytes() for x in eng.copy_walk()]))
        assert res[0] == res[1] == res[2]
    finally:
        eng.close()
        for x in (buf, src, d1, d2):
            if x is not None:
                x.free()

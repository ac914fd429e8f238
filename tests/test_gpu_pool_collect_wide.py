"""bsg_pool_collect past one pass of its grids, against the model of collect_cases.py, every result
for equality.

A launch is capped at T = 8 x CUs x 256 threads (engine_grid), read from the source and the device
as tests/test_gpu_pool_wide.py reads it. The source is that file's pool: dedup_cases.wide_run put
once, more than T blobs of at most some 25 bytes and a few thousand nodes. The collect keeps the
main stream's Root and drops the 80 excerpts' and the copy's, whose nodes (and the chunks at
their cut ends) die: at least 1,000 dead blobs spread over the table while more than T stay live.
So k_pool_adopt and every grid-stride pass of the mark make a second trip, k_gc_compact's seg_find
runs over more than a grid of segments, and the destination's index takes more than a grid of
inserts. Then the kept Root walks the same on both pools."""
import numpy as np
import pytest

import collect_cases as C
import dedup_cases as DC
import pool_cases as P
import walk_cases as W
from test_gpu_dedup import _records, _run
from test_gpu_pool_wide import _equal
from test_gpu_tier_counts import cus  # noqa: F401  (the device's CU count, a fixture)

pytestmark = pytest.mark.gpu


def test_wide_collect(gpu, oracle, table, cus):  # noqa: F811
    t, _ = DC.wide_counts(cus)
    assert t == 8 * cus * 256
    case, _ = DC.wide_run(oracle, table, cus)
    streams, bits, mn = case
    host, off, lens = DC.place(streams)
    eng = gpu.Engine()
    buf = src = dst = None
    try:
        buf = _run(gpu, eng, host, off, lens, bits, mn)
        recs = _records(gpu, oracle, table, eng, streams, bits, mn)
        roots, _, nodes, arena = eng.trees()
        run = (recs, streams, nodes, arena)
        cap = (int(((recs["len"].astype(np.int64) + 15) & ~15).sum()) + len(arena),
               len(recs) + len(nodes))
        src, m = gpu.Pool(*cap), P.Model(*cap)
        rc, put = m.put(run)
        assert rc == P.OK and eng.pool_put(src) == put
        kept = [roots[DC.WIDE_EXCERPTS].tobytes()]          # the main stream's
        before = (src.stat(), src.table().tobytes())

        rc, status, info, md, remap = C.collect(m, kept, *cap)
        assert rc == C.OK
        assert info["gc"]["ndead"] >= 1000 and info["gc"]["nlive"] > t, (info, t)
        dead = np.flatnonzero(remap == C.NONE)
        assert dead[0] < len(remap) // 2 < dead[-1]        # dead blobs on both sides of the table
        dst = gpu.Pool(*cap)
        got = eng.pool_collect(src, dst, W.roots_array(kept))
        assert got[0] == C.OK and got[1] == info and got[2].tolist() == status.tolist()
        st = dst.stat()
        assert st == md.stat(), (st, md.stat())
        tb, want = dst.table(), md.blobs()
        for f in ("off", "len"):
            _equal(f, tb[f], want[f])
        assert tb["ref"].tobytes() == want["ref"].tobytes()
        _equal("bytes", dst.to_host(P.align16(st["bytes"])), md.buf)   # in full, padding included
        _equal("remap", dst.remap(), remap)
        assert (src.stat(), src.table().tobytes()) == before

        # the kept Root walks the same on the destination and on the source
        res = []
        for pool in (dst, src):
            rc, winfo, wstatus = eng.pool_walk(pool, W.roots_array(kept))
            assert rc == W.OK, (rc, winfo)
            res.append((winfo, wstatus.tolist(), [x.tobytes() for x in eng.copy_walk()]))
        assert res[0] == res[1]
        main = recs[recs["stream"] == DC.WIDE_EXCERPTS]
        walked = np.frombuffer(res[0][2][0], dtype=gpu.CHUNK_DTYPE)
        assert len(walked) == len(main) and walked["ref"].tobytes() == main["ref"].tobytes()
    finally:
        eng.close()
        for x in (buf, src, dst):
            if x is not None:
                x.free()

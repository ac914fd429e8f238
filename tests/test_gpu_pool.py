"""bsg_pool / bsg_engine_pool_put on the device against the model of pool_cases.py, every
comparison an equality: one put, two runs in one pool, the same run twice, a full pool, flags and
states, what a put leaves alone, gc on a pool, an index whose cluster wraps, two threads."""
import ctypes
import threading

import numpy as np
import pytest

import dedup_cases as DC
import gc_cases as G
import pool_cases as P
import walk_cases as W
from bs_amd.bsgpu import BsgError
from bs_amd.synth import edit_stream, splitmix_array
from test_gpu_engine_trees import _run

pytestmark = pytest.mark.gpu

PARAMS = [(4, 64, 2), (6, 64, 3), (16, 1024, 8)]
CAP = (8 << 20, 1 << 16)


@pytest.fixture()
def eng(gpu):
    e = gpu.Engine()
    yield e
    e.close()


def _streams(bits, edited=False):
    """A, a copy of A, a prefix of A, an empty stream, a one-chunk stream and B; `edited`: the
    second run's streams, the first run's with a few KB edited, plus a new stream."""
    na, nb, one = (9107, 30000, 40) if bits < 16 else (187986, 1 << 21, 500)
    a, b = splitmix_array(1, na), splitmix_array(2, nb)
    out = [a, a.copy(), a[:na // 2].copy(), np.zeros(0, np.uint8), splitmix_array(3, one), b]
    if edited:
        out[0] = edit_stream(a, 5, sites=3, span=256)
        out[5] = edit_stream(b, 6, sites=8, span=256)
        out.append(splitmix_array(4, na + 77))
    return out


def _start(gpu, eng, streams, bits, mn, fanout, trees=True):
    """One finished run (and its trees) on `eng`: (the input's device buffer, the run as the
    model takes it, the Roots)."""
    buf = _run(gpu, eng, streams, bits, mn, fanout)
    try:
        recs = eng.chunks()
        if not trees:
            return buf, (recs, streams, np.zeros(0, gpu.TREE_NODE_DTYPE), np.zeros(0, np.uint8)), []
        roots, _, nodes, arena = eng.trees()
        return buf, (recs, streams, nodes, arena), [r.tobytes() for r in roots]
    except BaseException:
        buf.free()
        raise


def _state(pool):
    st = pool.stat()
    return st, pool.table().tobytes(), pool.to_host(P.align16(st["bytes"])).tobytes()


def _same(pool, m, where=True):
    """The pool's counters, table, bytes (up to the end of the last blob's padding) and where[]
    are the model's."""
    st, table, raw = _state(pool)
    assert st == m.stat(), (st, m.stat())
    assert table == m.blobs().tobytes()
    assert raw == m.buf.tobytes()
    if where:
        assert pool.where().tolist() == m.where.tolist()


def _put(eng, pool, m, run, chunks=True, nodes=True, expect=P.OK):
    """One put on the device and in the model; the return code and every info field equal."""
    rc, want = m.put(run, (P.CHUNKS if chunks else 0) | (P.NODES if nodes else 0))
    assert rc == expect, (rc, expect, want)
    try:
        info = eng.pool_put(pool, chunks=chunks, nodes=nodes)
        got = P.OK
    except BsgError as e:  # the code and the info of the failed call
        got, info = e.code, e.info
    assert got == rc and info == want, (got, rc, info, want)
    return info


def _walk_and_restore(gpu, eng, pool, m, roots, recs, streams, verify=True):
    """The Roots walk over pool.table() to the records, and restore_walk gives the bytes back."""
    blobs = pool.table()
    W.check(gpu, eng, pool, m.blob_bytes, blobs, roots, pool.pool_bytes, expect=W.OK)
    got, sizes, _ = eng.copy_walk()
    for f in ("stream", "offset", "len", "ref"):
        assert (got[f] == recs[f]).all(), f
    assert sizes.tolist() == [len(d) for d in streams]
    rc, info, off, out = W.restore_walk(gpu, eng, pool, pool.pool_bytes, blobs, sizes,
                                        verify=verify)
    assert rc == W.OK and info["bytes"] == sum(len(d) for d in streams), (rc, info)
    for s, d in enumerate(streams):
        assert out[off[s]:off[s] + len(d)].tobytes() == bytes(d), s


def _restream(recs, s0):
    """Records as a walk of Roots [s0 ..) numbers them."""
    r = recs.copy()
    r["stream"] += s0
    return r


# ---- 1. one put --------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,mn,fanout", PARAMS)
def test_one_put(gpu, eng, bits, mn, fanout):
    streams = _streams(bits)
    pool, m = gpu.Pool(*CAP), P.Model(*CAP)
    buf, run, roots = _start(gpu, eng, streams, bits, mn, fanout)
    try:
        assert pool.stat() == m.stat() and len(pool.table()) == 0
        info = _put(eng, pool, m, run)
        _same(pool, m)
        recs, _, nodes, _ = run
        assert info["repeats"] > 0 and info["known"] == 0 and info["added"] == len(m.table)
        # the copy of A adds no node
        at = len(recs) + np.flatnonzero(nodes["stream"] == 1)
        assert len(at) and (m.where[at] == m.where[len(recs) + np.flatnonzero(nodes["stream"] == 0)]
                            ).all()
        assert (pool.table()["off"] % 16 == 0).all()
        _walk_and_restore(gpu, eng, pool, m, roots, recs, streams)
        _walk_and_restore(gpu, eng, pool, m, roots, recs, streams, verify=False)
    finally:
        buf.free()
        pool.free()


# ---- 2. two runs, one pool; 3. the same run twice ----------------------------------------------
@pytest.mark.parametrize("bits,mn,fanout", PARAMS)
def test_two_runs_one_pool(gpu, eng, bits, mn, fanout):
    s1, s2 = _streams(bits), _streams(bits, edited=True)
    pool, m = gpu.Pool(*CAP), P.Model(*CAP)
    try:
        buf, run1, roots1 = _start(gpu, eng, s1, bits, mn, fanout)
        try:
            _put(eng, pool, m, run1)
            st1, table1, raw1 = _state(pool)
            again = _put(eng, pool, m, run1)              # the same run twice
            assert again["added"] == 0 and again["known"] == again["items"]
            assert _state(pool) == (st1, table1, raw1)
            _same(pool, m)
        finally:
            buf.free()
        buf, run2, roots2 = _start(gpu, eng, s2, bits, mn, fanout)
        try:
            info = _put(eng, pool, m, run2)
            _same(pool, m)
            assert info["known"] > 0 and info["added"] > 0
            assert info["first_blob"] == st1["nblobs"]
            st2, table2, raw2 = _state(pool)
            assert table2[:len(table1)] == table1
            assert raw2[:len(raw1)] == raw1 and len(raw1) == P.align16(st1["bytes"])
            # the Roots of both runs walk and restore from the one pool
            recs = np.concatenate([run1[0], _restream(run2[0], len(s1))])
            _walk_and_restore(gpu, eng, pool, m, roots1 + roots2, recs, s1 + s2)
        finally:
            buf.free()
    finally:
        pool.free()


# ---- 4. full -----------------------------------------------------------------------------------
def test_full(gpu, eng):
    bits, mn, fanout = 6, 64, 3
    streams = _streams(bits)
    small = [splitmix_array(8, 3000)]
    buf, run, roots = _start(gpu, eng, streams, bits, mn, fanout)
    pools = []
    try:
        need = P.Model(*CAP).put(run)[1]
        for cb, cn in ((need["need_bytes"] - 1, need["need_blobs"]),
                       (need["need_bytes"], need["need_blobs"] - 1)):
            pool, m = gpu.Pool(cb, cn), P.Model(cb, cn)
            pools.append((pool, m))
            before = _state(pool)
            info = _put(eng, pool, m, run, expect=P.ENOMEM)
            assert info == need and _state(pool) == before
            assert gpu.lib().bsg_pool_copy_where(pool.h, None, 0) == P.ESTATE   # no put yet
        exact, me = gpu.Pool(need["need_bytes"], need["need_blobs"]), P.Model(
            need["need_bytes"], need["need_blobs"])
        pools.append((exact, me))
        _put(eng, exact, me, run)
        _same(exact, me)
        _walk_and_restore(gpu, eng, exact, me, roots, run[0], streams)
        # full after a put: where[] too stays the earlier put's
        where = exact.where().tobytes()
        buf.free()
        buf, run_s, roots_s = _start(gpu, eng, small, bits, mn, fanout)
        before = _state(exact)
        _put(eng, exact, me, run_s, expect=P.ENOMEM)
        assert _state(exact) == before and exact.where().tobytes() == where
        # a smaller run then fits the pools that were one short
        for pool, m in pools[:2]:
            _put(eng, pool, m, run_s)
            _same(pool, m)
            _walk_and_restore(gpu, eng, pool, m, roots_s, run_s[0], small)
    finally:
        buf.free()
        for pool, _ in pools:
            pool.free()


# ---- 5. flags and state ------------------------------------------------------------------------
def test_flags(gpu, eng):
    bits, mn, fanout = 4, 64, 2
    streams = _streams(bits)
    buf, run, roots = _start(gpu, eng, streams, bits, mn, fanout)
    both, split, only = gpu.Pool(*CAP), gpu.Pool(*CAP), gpu.Pool(*CAP)
    mb, ms, mo = P.Model(*CAP), P.Model(*CAP), P.Model(*CAP)
    try:
        _put(eng, both, mb, run)
        i1 = _put(eng, split, ms, run, nodes=False)
        _same(split, ms)
        i2 = _put(eng, split, ms, run, chunks=False)
        _same(split, ms)
        assert _state(split) == _state(both) and i2["first_blob"] == i1["added"]
        # nodes only into an empty pool: the leaves are simply absent
        _put(eng, only, mo, run, chunks=False)
        _same(only, mo)
        blobs = only.table()
        want = G.mark(mo.blob_bytes, blobs, roots, only.pool_bytes, G.GC_MISSING_LEAVES)
        rc, info, status = eng.gc_mark(only.ptr, blobs, W.roots_array(roots),
                                       pool_bytes=only.pool_bytes, flags=gpu.GC_MISSING_LEAVES)
        assert rc == want[0] == G.OK and info == want[2]
        assert info["missing_leaves"] == len({r.tobytes() for r in run[0]["ref"]}) > 0
        rc, info, status = eng.gc_mark(only.ptr, blobs, W.roots_array(roots),
                                       pool_bytes=only.pool_bytes)
        assert rc == G.ENOTFOUND
    finally:
        buf.free()
        for p in (both, split, only):
            p.free()


def test_states_and_arguments(gpu, eng):
    L = gpu.lib()
    info = gpu.POOL_PUT_INFO()
    err = ctypes.c_int(0)
    assert not L.bsg_pool_new(L.bsg_device_count() + 3, 1 << 20, 16, ctypes.byref(err))
    assert err.value == P.ENODEV
    pool = gpu.Pool(1 << 20, 1 << 12)
    streams = [splitmix_array(5, 9107)]
    try:
        put = lambda e, p, f: L.bsg_engine_pool_put(e, p, f, ctypes.byref(info))  # noqa: E731
        for e, p, f in ((None, pool.h, 3), (eng.h, None, 3), (eng.h, pool.h, 0),
                        (eng.h, pool.h, 4), (eng.h, pool.h, 7)):
            assert put(e, p, f) == P.EINVAL
        assert L.bsg_pool_stat(None, None) == P.EINVAL
        assert L.bsg_pool_copy_table(pool.h, None, 1, 0) == P.EINVAL       # first > nblobs
        assert not L.bsg_pool_bytes_device(None) and not L.bsg_pool_where_device(pool.h)
        assert pool.ptr % 16 == 0 and L.bsg_pool_table_device(pool.h)
        assert put(eng.h, pool.h, 1) == P.ESTATE                           # no run
        buf = _run(gpu, eng, streams, 6, 64, 3)
        try:
            assert put(eng.h, pool.h, 2) == P.ESTATE                       # no trees
            assert put(eng.h, pool.h, 3) == P.ESTATE
            assert put(eng.h, pool.h, 1) == P.OK and info.added > 0
            eng.trees()
            assert put(eng.h, pool.h, 3) == P.OK and info.known > 0
            assert L.bsg_pool_where_device(pool.h)
            n = pool.stat()["nblobs"]
            # a new run: the earlier run's tree is not this run's
            eng.run(buf.ptr, [0], [len(streams[0])], bits=4, min_size=64, fanout=2)
            assert put(eng.h, pool.h, 1) == P.ESTATE                       # unfinished
            eng.finish()
            assert put(eng.h, pool.h, 2) == P.ESTATE
            eng.hash(buf.ptr, [0], [3000])
            eng.finish()
            assert put(eng.h, pool.h, 1) == P.ESTATE                       # a hash run
            assert pool.stat()["nblobs"] == n
            # a run over the pool's own bytes
            eng.run(pool.ptr, [0], [4096], bits=6, min_size=64, fanout=3)
            eng.finish()
            assert put(eng.h, pool.h, 1) == P.EINVAL
        finally:
            buf.free()
    finally:
        pool.free()


# ---- 6. the put leaves the run alone -----------------------------------------------------------
def test_put_leaves_the_run_alone(gpu, eng):
    bits, mn, fanout = 6, 64, 3
    streams = _streams(bits)
    pool, m = gpu.Pool(*CAP), P.Model(*CAP)
    buf, run, roots = _start(gpu, eng, streams, bits, mn, fanout)
    try:
        L = gpu.lib()

        def snapshot():
            n, nu = len(run[0]), eng.nunique
            first, uniq = np.zeros(n, np.uint64), np.zeros(max(nu, 1), np.uint64)
            pack_off = np.zeros(nu + 1, np.uint64)
            assert L.bsg_engine_copy_dedup(eng.h, first.ctypes.data, n, uniq.ctypes.data,
                                           pack_off.ctypes.data, nu) == 0
            nn, ar = np.zeros(len(run[2]), gpu.TREE_NODE_DTYPE), np.zeros(len(run[3]), np.uint8)
            assert L.bsg_engine_copy_tree_nodes(eng.h, nn.ctypes.data, len(nn), ar.ctypes.data,
                                                len(ar)) == 0
            rt = np.zeros((len(streams), 32), np.uint8)
            assert L.bsg_engine_copy_roots(eng.h, rt.ctypes.data, None, len(streams)) == 0
            return [x.tobytes() for x in (eng.chunks(), first, uniq, pack_off, nn, ar, rt,
                                          *eng.copy_walk())]

        _put(eng, pool, m, run)
        eng.dedup()
        _walk_and_restore(gpu, eng, pool, m, roots, run[0], streams)
        before = snapshot()
        other, mo = gpu.Pool(*CAP), P.Model(*CAP)
        try:
            _put(eng, other, mo, run)
            _put(eng, pool, m, run, chunks=False)
        finally:
            other.free()
        assert snapshot() == before
    finally:
        buf.free()
        pool.free()


# ---- 7. gc on a pool ---------------------------------------------------------------------------
def test_gc_on_a_pool(gpu, eng):
    bits, mn, fanout = 6, 64, 3
    s1, s2 = _streams(bits), _streams(bits, edited=True)
    pool, m = gpu.Pool(*CAP), P.Model(*CAP)
    swept = None
    try:
        buf, run1, _ = _start(gpu, eng, s1, bits, mn, fanout)
        _put(eng, pool, m, run1)
        buf.free()
        buf, run2, roots2 = _start(gpu, eng, s2, bits, mn, fanout)
        try:
            _put(eng, pool, m, run2)
            blobs = pool.table()
            want = G.mark(m.blob_bytes, blobs, roots2, pool.pool_bytes)
            rc, info, status = eng.gc_mark(pool.ptr, blobs, W.roots_array(roots2),
                                           pool_bytes=pool.pool_bytes)
            assert rc == want[0] == G.OK and info == want[2] and info["ndead"] > 0
            live, table = eng.copy_gc(align16=True)
            assert live.tolist() == want[3].tolist()
            wtable, end = G.layout(blobs, want[3], True)
            assert table.tobytes() == wtable.tobytes()
            swept = gpu.DeviceBuffer(P.align16(end))
            rc, n = eng.gc_compact(pool.ptr, swept, align16=True, pool_bytes=pool.pool_bytes)
            assert rc == G.OK and n == end
            assert swept.to_host(0, end).tobytes() == G.compacted(m.buf, blobs, want[3],
                                                                  True).tobytes()
            # the compacted pool walks and restores run 2
            sm = P.Model(*CAP)
            sm.table = [(int(t["off"]), int(t["len"]), t["ref"].tobytes()) for t in table]
            sm.buf = swept.to_host(0, end)
            pb = swept.nbytes + gpu.READ_SLACK
            W.check(gpu, eng, swept, sm.blob_bytes, table, roots2, pb, expect=W.OK)
            got, sizes, _ = eng.copy_walk()
            assert got["ref"].tobytes() == run2[0]["ref"].tobytes()
            rc, info, off, out = W.restore_walk(gpu, eng, swept, pb, table, sizes, verify=True)
            assert rc == W.OK
            for s, d in enumerate(s2):
                assert out[off[s]:off[s] + len(d)].tobytes() == bytes(d), s
        finally:
            buf.free()
    finally:
        pool.free()
        if swept is not None:
            swept.free()


# ---- 8. the index wraps ------------------------------------------------------------------------
def _wrap_case(oracle, table, cap_blobs=8):
    """A one-stream run of at most cap_blobs blobs (chunks and nodes) whose index cluster at the
    table's last slots steps on to slot 0, by the model alone: (streams, the run, the model after
    the put). The seed is searched on the CPU."""
    for seed in range(100, 400):
        streams = [splitmix_array(seed, 600)]
        run = P.oracle_run(oracle, table, streams, 6, 64, 3)
        m = P.Model(1 << 16, cap_blobs)
        rc, _ = m.put(run)
        if rc == P.OK and m.wrapped():
            return streams, run, m
    raise AssertionError("no seed wraps")


def test_index_wraps(gpu, eng, oracle, table):
    streams, want_run, m0 = _wrap_case(oracle, table)
    slots = P.slots_of(8)
    assert slots == 16 and m0.wrapped() and len(m0.table) <= 8
    k = m0.wrapped()[0]
    assert m0.homes()[k] > DC.probe_slots([r for _, _, r in m0.table], slots)[m0.table[k][2]]
    pool, m = gpu.Pool(1 << 16, 8), P.Model(1 << 16, 8)
    buf, run, roots = _start(gpu, eng, streams, 6, 64, 3)
    try:
        assert run[0].tobytes() == want_run[0].tobytes()
        assert run[2]["ref"].tobytes() == want_run[2]["ref"].tobytes()
        _put(eng, pool, m, run)
        _same(pool, m)
        assert m.table == m0.table
        again = _put(eng, pool, m, run)                   # every ref is found
        assert again["added"] == 0 and again["known"] == again["items"]
        _same(pool, m)
        _walk_and_restore(gpu, eng, pool, m, roots, run[0], streams)
    finally:
        buf.free()
        pool.free()


# ---- 9. two threads, one pool ------------------------------------------------------------------
def test_two_threads_one_pool(gpu):
    bits, mn, fanout = 6, 64, 3
    groups, _, _ = DC.shared_halves()
    groups = [g[:6] for g in groups]                      # 4 common streams, 2 of their own
    pool = gpu.Pool(*CAP)
    engs = [gpu.Engine(), gpu.Engine()]
    runs, bufs, errs = [None, None], [None, None], []
    for t in range(2):
        bufs[t], run, roots = _start(gpu, engs[t], groups[t], bits, mn, fanout)
        runs[t] = (run, roots)
    go = threading.Barrier(2)

    def work(t):
        try:
            go.wait()
            engs[t].pool_put(pool, nodes=False)
            engs[t].pool_put(pool)
        except BaseException as e:  # noqa: BLE001
            errs.append(e)

    try:
        th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not errs, errs
        table = pool.table()
        got = [(int(t["len"]), t["ref"].tobytes()) for t in table]
        want = set()
        for run, _ in runs:
            want |= {(int(r["len"]), r["ref"].tobytes()) for r in run[0]}
            want |= {(int(n["blob_len"]), n["ref"].tobytes()) for n in run[2]}
        assert len(got) == len(set(r for _, r in got)) and set(got) == want
        assert (table["off"] % 16 == 0).all()
        st = pool.stat()
        m = P.Model(*CAP)
        m.table = [(int(t["off"]), int(t["len"]), t["ref"].tobytes()) for t in table]
        m.buf = pool.to_host(P.align16(st["bytes"]))
        for t in range(2):
            run, roots = runs[t]
            _walk_and_restore(gpu, engs[t], pool, m, roots, run[0], groups[t])
    finally:
        for b in bufs:
            if b is not None:
                b.free()
        for e in engs:
            e.close()
        pool.free()


# ---- 10. a pool made where another one was, and a run without items ----------------------------
def test_new_pools_in_freed_memory_and_an_empty_run(gpu, eng):
    """Pools made, filled and freed in turn: the next one lies where the last one lay, and its
    index and bytes are empty whatever that one left behind. A run of one empty stream puts
    nothing."""
    bits, mn, fanout = 6, 64, 3
    streams = _streams(bits)
    buf, run, roots = _start(gpu, eng, streams, bits, mn, fanout)
    try:
        need = P.Model(*CAP).put(run)[1]
        cap = (need["need_bytes"] + 4096, need["need_blobs"] + 5)
        for _ in range(4):
            pool, m = gpu.Pool(*cap), P.Model(*cap)
            try:
                assert not pool.to_host(cap[0]).any()
                assert _put(eng, pool, m, run) == need
                _same(pool, m)
            finally:
                pool.free()
        buf.free()
        buf, run0, roots0 = _start(gpu, eng, [np.zeros(0, np.uint8)], bits, mn, fanout)
        pool, m = gpu.Pool(*cap), P.Model(*cap)
        try:
            info = _put(eng, pool, m, run0)
            assert info["items"] == 0 and roots0 == [bytes(32)]
            _same(pool, m)
            assert not gpu.lib().bsg_pool_where_device(pool.h)
            _put(eng, pool, m, run0, chunks=False)
        finally:
            pool.free()
    finally:
        buf.free()

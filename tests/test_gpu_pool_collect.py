"""bsg_pool_collect, bsg_pool_reset, bsg_pool_walk and bsg_pool_restore_walk on the device against
the model of collect_cases.py, every comparison an equality and the destination's bytes in full:
a collect with one run's Roots, with all, none and repeated Roots, missing leaves, failed marks,
capacity, states and arguments, puts after a collect, the engine's gc result after a collect,
reset, an index cluster that wraps, two threads, and the pool-native walk and restore against the
host-table forms."""
import ctypes
import threading

import numpy as np
import pytest

import collect_cases as C
import gc_cases as G
import pool_cases as P
import walk_cases as W
from bs_amd.synth import edit_stream, splitmix_array
from test_gpu_engine_trees import _run
from test_gpu_pool import _wrap_case

pytestmark = pytest.mark.gpu

BITS, MN, FANOUT = 8, 64, 3
CAP = (4 << 20, 1 << 14)


def _streams(second=False):
    """Run 1: A, a prefix of A and B. Run 2: A with a few KB edited, B again and a new stream."""
    a, b = splitmix_array(1, 300_007), splitmix_array(2, 200_000)
    if not second:
        return [a, a[:150_001].copy(), b]
    return [edit_stream(a, 5, sites=3, span=256), b, splitmix_array(4, 120_077)]


def _start(gpu, eng, streams, fanout=FANOUT):
    """One finished run and its trees on `eng`: (the input's device buffer, the run as the model
    takes it, the Roots)."""
    buf = _run(gpu, eng, streams, BITS, MN, fanout)
    try:
        recs = eng.chunks()
        roots, _, nodes, arena = eng.trees()
        return buf, (recs, streams, nodes, arena), [r.tobytes() for r in roots]
    except BaseException:
        buf.free()
        raise


def _put(eng, pool, m, run, chunks=True, nodes=True):
    rc, want = m.put(run, (P.CHUNKS if chunks else 0) | (P.NODES if nodes else 0))
    assert rc == P.OK
    info = eng.pool_put(pool, chunks=chunks, nodes=nodes)
    assert info == want, (info, want)
    return info


class Base:
    """Two runs put into one pool, once for the module: the pool, its model, the runs (as the
    model takes them), their Roots and streams. No test writes the pool."""


@pytest.fixture(scope="module")
def base(gpu):
    b, eng = Base(), gpu.Engine()
    b.src, b.m = gpu.Pool(*CAP), P.Model(*CAP)
    b.runs, b.roots, b.streams = [], [], []
    try:
        for second in (False, True):
            streams = _streams(second)
            buf, run, roots = _start(gpu, eng, streams)
            try:
                _put(eng, b.src, b.m, run)
            finally:
                buf.free()
            b.runs.append(run)
            b.roots.append(roots)
            b.streams.append(streams)
        depth = G.mark(b.m.blob_bytes, b.m.blobs(), b.roots[0], b.src.pool_bytes)[2]["depth"]
        assert depth >= 2, depth                           # at least three levels of nodes
        b.state = _state(b.src)
        yield b
        assert _state(b.src) == b.state, "a test wrote the source"
    finally:
        eng.close()
        b.src.free()


@pytest.fixture()
def eng(gpu):
    e = gpu.Engine()
    yield e
    e.close()


def _state(pool):
    st = pool.stat()
    return st, pool.table().tobytes(), pool.to_host(P.align16(st["bytes"])).tobytes()


def _raw(gpu, pool):
    """Everything a failed collect must leave as it was: the counters, the whole allocation, every
    table entry up to the capacity, and the remap and where[] pointers."""
    st = pool.stat()
    table = np.zeros(max(st["cap_blobs"], 1), dtype=gpu.POOL_BLOB_DTYPE)
    rc = gpu.lib().bsg_memcpy(pool.device, table.ctypes.data,
                              gpu.lib().bsg_pool_table_device(pool.h), table.nbytes, 1)
    assert rc == 0
    return (st, pool.to_host(st["pool_bytes"]).tobytes(), table.tobytes(), pool.remap_device(),
            pool.where_device())


def _same(pool, m):
    st, table, raw = _state(pool)
    assert st == m.stat(), (st, m.stat())
    assert table == m.blobs().tobytes()
    assert raw == m.buf.tobytes()


def _collect(gpu, eng, b_src, m_src, dst, roots, flags=0, expect=C.OK):
    """One collect on the device and in the model: the return code, every Root's status, the info
    and, on success, the destination's counters, table, bytes and remap equal; on failure the
    destination is as it was. Returns the model's tuple."""
    st = dst.stat()
    want = C.collect(m_src, roots, st["cap_bytes"], st["cap_blobs"], flags)
    assert want[0] == expect, (want[0], expect, want[2])
    before = _raw(gpu, dst)
    rc, info, status = eng.pool_collect(b_src, dst, W.roots_array(roots), flags)
    assert rc == want[0], (rc, want[0], info, want[2])
    assert info == want[2], (info, want[2])
    assert status.tolist() == want[1].tolist()
    if rc != C.OK:
        assert _raw(gpu, dst) == before
        return want
    _same(dst, want[3])
    assert dst.remap().tolist() == want[4].tolist()
    assert (dst.remap_device() != 0) == (len(want[4]) > 0)
    return want


def _restored(gpu, eng, pool, roots, streams, verify):
    """bsg_pool_walk of the Roots, then bsg_pool_restore_walk: the streams bit for bit."""
    rc, info, status = eng.pool_walk(pool, W.roots_array(roots))
    assert rc == W.OK and not status.any(), (rc, info, status)
    _, sizes, _ = eng.copy_walk()
    assert sizes.tolist() == [len(d) for d in streams]
    off, cap = W.out_layout(sizes)
    obuf = gpu.DeviceBuffer(W.GUARD + cap + W.GUARD)
    try:
        obuf.from_host(np.full(obuf.nbytes, W.FILL, dtype=np.uint8))
        rc, info = eng.pool_restore_walk(pool, obuf.ptr + W.GUARD, off, verify=verify, out_cap=cap)
        got = obuf.to_host()
    finally:
        obuf.free()
    assert rc == W.OK and info["bytes"] == sum(len(d) for d in streams), (rc, info)
    assert (got[:W.GUARD] == W.FILL).all() and (got[W.GUARD + cap:] == W.FILL).all()
    for s, d in enumerate(streams):
        o = W.GUARD + off[s]
        assert got[o:o + len(d)].tobytes() == bytes(d), s


# ---- 1. one run's Roots ------------------------------------------------------------------------
def test_collect_run_one(gpu, eng, base):
    dst = gpu.Pool(*CAP)
    try:
        want = _collect(gpu, eng, base.src, base.m, dst, base.roots[0])
        gi = want[2]["gc"]
        assert gi["ndead"] > 0 and gi["nlive"] > 0 and gi["depth"] >= 2
        assert (dst.table()["off"] % 16 == 0).all() and not dst.where_device()
        _restored(gpu, eng, dst, base.roots[0], base.streams[0], verify=True)
        _restored(gpu, eng, dst, base.roots[0], base.streams[0], verify=False)
        # run 2's own Roots are gone
        rc, info, status = eng.pool_walk(dst, W.roots_array(base.roots[1]))
        assert rc == W.ENOTFOUND and status[0] == W.ENOTFOUND
    finally:
        dst.free()


# ---- 2. all, none and repeated Roots -----------------------------------------------------------
def test_all_roots_is_the_source(gpu, eng, base):
    dst = gpu.Pool(*CAP)
    try:
        want = _collect(gpu, eng, base.src, base.m, dst, base.roots[0] + base.roots[1])
        assert want[2]["gc"]["ndead"] == 0
        assert _state(dst) == base.state
        assert dst.remap().tolist() == list(range(base.state[0]["nblobs"]))
    finally:
        dst.free()


def test_no_roots_is_an_empty_pool(gpu, eng, base):
    for roots in ([], [bytes(32)] * 5):
        dst = gpu.Pool(1 << 12, 4)
        try:
            fresh = _raw(gpu, dst)
            _collect(gpu, eng, base.src, base.m, dst, roots)
            got = _raw(gpu, dst)
            assert got[:3] == fresh[:3] and dst.stat()["nblobs"] == 0
            assert (dst.remap() == gpu.NONE64).all()
        finally:
            dst.free()
    # an empty source: nothing to map
    empty, dst = gpu.Pool(1 << 12, 4), gpu.Pool(1 << 12, 4)
    try:
        _collect(gpu, eng, empty, P.Model(1 << 12, 4), dst, [])
        assert not dst.remap_device()
        _collect(gpu, eng, empty, P.Model(1 << 12, 4), dst, [base.roots[0][0]],
                 expect=C.ENOTFOUND)
    finally:
        empty.free()
        dst.free()


def test_one_root_many_times(gpu, eng, base):
    one, many = gpu.Pool(*CAP), gpu.Pool(*CAP)
    try:
        r = base.roots[0][0]
        _collect(gpu, eng, base.src, base.m, one, [r])
        _collect(gpu, eng, base.src, base.m, many, [r] * 700 + [bytes(32)] + [r] * 3)
        assert _state(one) == _state(many)
        assert one.remap().tobytes() == many.remap().tobytes()
    finally:
        one.free()
        many.free()


# ---- 3. missing leaves -------------------------------------------------------------------------
def test_missing_leaves(gpu, eng, base):
    only, mo, dst = gpu.Pool(*CAP), P.Model(*CAP), gpu.Pool(*CAP)
    buf, run, roots = _start(gpu, eng, base.streams[0])
    try:
        _put(eng, only, mo, run, chunks=False)
        before = _state(only)
        _collect(gpu, eng, only, mo, dst, roots, expect=C.ENOTFOUND)
        want = _collect(gpu, eng, only, mo, dst, roots, flags=gpu.GC_MISSING_LEAVES)
        assert want[2]["gc"]["missing_leaves"] == len({r.tobytes() for r in run[0]["ref"]}) > 0
        assert want[2]["gc"]["ndead"] == 0 and _state(dst) == before == _state(only)
    finally:
        buf.free()
        for p in (only, dst):
            p.free()


# ---- 4. failed marks and capacity: the destination stays as it was -------------------------------
def test_failed_marks_leave_the_destination(gpu, eng, base):
    dst, md = gpu.Pool(*CAP), P.Model(*CAP)
    small = [splitmix_array(8, 3000)]
    try:
        gone = bytes(range(1, 33))
        chunk = base.runs[0][0][7]["ref"].tobytes()
        for roots, rc, st in (([base.roots[0][0], gone, base.roots[0][2]], C.ENOTFOUND,
                               [0, C.ENOTFOUND, 0]),
                              ([base.roots[0][1], chunk], C.ECORRUPT, [0, C.ECORRUPT])):
            want = _collect(gpu, eng, base.src, base.m, dst, roots, expect=rc)
            assert want[1].tolist() == st and want[2]["gc"]["bad_root"] == 1
            assert gpu.lib().bsg_engine_copy_gc(eng.h, None, 0, None, 0, 0) == C.ESTATE
            assert gpu.lib().bsg_pool_copy_remap(dst.h, None, 0) == C.ESTATE
        # an earlier collect's remap and an (empty) put's where[] stay through a failed collect
        _collect(gpu, eng, base.src, base.m, dst, [])
        buf, run0, _ = _start(gpu, eng, [np.zeros(0, np.uint8)])
        buf.free()
        _put(eng, dst, md, run0)
        remap = dst.remap().tobytes()
        _collect(gpu, eng, base.src, base.m, dst, [gone], expect=C.ENOTFOUND)
        assert dst.remap().tobytes() == remap and dst.remap_device()
        # and the destination is still a pool
        buf, run, roots = _start(gpu, eng, small)
        try:
            _put(eng, dst, md, run)
            _same(dst, md)
        finally:
            buf.free()
    finally:
        dst.free()


def test_capacity(gpu, eng, base):
    need = C.collect(base.m, base.roots[0], *CAP)[2]
    nb, nn = need["need_bytes"], need["need_blobs"]
    assert nn == need["gc"]["nlive"] > 1
    for cb, cn in ((nb, nn - 1), (nb - 1, nn)):
        dst = gpu.Pool(cb, cn)
        try:
            want = _collect(gpu, eng, base.src, base.m, dst, base.roots[0], expect=C.ENOMEM)
            assert want[2] == need
            assert gpu.lib().bsg_pool_copy_remap(dst.h, None, 0) == C.ESTATE
            # the mark stands although nothing was appended
            live, table = eng.copy_gc(align16=True)
            assert int(live.sum()) == nn == len(table)
        finally:
            dst.free()
    exact = gpu.Pool(nb, nn)
    try:
        _collect(gpu, eng, base.src, base.m, exact, base.roots[0])
        _restored(gpu, eng, exact, base.roots[0], base.streams[0], verify=True)
    finally:
        exact.free()


# ---- 5. states and arguments -------------------------------------------------------------------
def test_states_and_arguments(gpu, eng, base):
    L = gpu.lib()
    dst, other = gpu.Pool(*CAP), gpu.Pool(1 << 16, 64)
    roots = W.roots_array(base.roots[0])
    info = gpu.PoolCollectInfo()
    try:
        def call(e, s, d, r=roots.ctypes.data, n=len(roots), f=0):
            return L.bsg_pool_collect(e, s, d, r, n, f, None, ctypes.byref(info))

        for args in ((None, base.src.h, dst.h), (eng.h, None, dst.h), (eng.h, base.src.h, None),
                     (eng.h, dst.h, dst.h)):
            assert call(*args) == C.EINVAL, args
        assert call(eng.h, base.src.h, dst.h, f=2) == C.EINVAL
        assert call(eng.h, base.src.h, dst.h, f=3) == C.EINVAL
        assert call(eng.h, base.src.h, dst.h, r=None) == C.EINVAL
        assert call(eng.h, base.src.h, dst.h, n=1 << 32) == C.EINVAL
        assert L.bsg_pool_collect(eng.h, base.src.h, dst.h, None, 0, 0, None, None) == C.OK
        assert L.bsg_pool_reset(None) == C.EINVAL and not L.bsg_pool_remap_device(None)
        assert L.bsg_pool_copy_remap(None, None, 0) == C.EINVAL
        assert L.bsg_pool_copy_remap(dst.h, None, 1) == C.EINVAL
        # EINVAL before ESTATE: a non-empty destination and an unknown flag
        assert call(eng.h, dst.h, base.src.h, f=2) == C.EINVAL
        assert call(eng.h, dst.h, base.src.h) == C.ESTATE                  # not empty
        # an unfinished run
        buf = gpu.DeviceBuffer(1 << 16)
        try:
            buf.from_host(splitmix_array(5, 1 << 16))
            eng.run(buf.ptr, [0], [1 << 16], bits=BITS, min_size=MN, fanout=FANOUT)
            assert call(eng.h, base.src.h, other.h) == C.ESTATE
            assert L.bsg_pool_walk(eng.h, None, roots.ctypes.data, len(roots), 0, None,
                                   None) == C.EINVAL
            eng.finish()
        finally:
            buf.free()
        assert other.stat()["nblobs"] == 0 and not other.remap_device()
        assert call(eng.h, base.src.h, other.h) == C.ENOMEM and info.need_blobs > 64
        assert L.bsg_pool_restore_walk(eng.h, None, None, 0, None, 0, 0, None) == C.EINVAL
    finally:
        dst.free()
        other.free()


# ---- 6. puts after a collect -------------------------------------------------------------------
def test_puts_after_a_collect(gpu, eng, base):
    dst = gpu.Pool(*CAP)
    try:
        md = _collect(gpu, eng, base.src, base.m, dst, base.roots[0])[3]
        dead = base.state[0]["nblobs"] - len(md.table)
        buf, run1, _ = _start(gpu, eng, base.streams[0])
        try:
            again = _put(eng, dst, md, run1)
            assert again["added"] == 0 and again["known"] == again["items"]
            _same(dst, md)
        finally:
            buf.free()
        buf, run2, roots2 = _start(gpu, eng, base.streams[1])
        try:
            info = _put(eng, dst, md, run2)
            assert info["added"] == dead > 0 and info["first_blob"] == len(md.table) - dead
            _same(dst, md)
            assert dst.where().tolist() == md.where.tolist()
            _restored(gpu, eng, dst, base.roots[0] + roots2, base.streams[0] + base.streams[1],
                      verify=True)
        finally:
            buf.free()
    finally:
        dst.free()


# ---- 7. the engine's gc result after a collect -------------------------------------------------
def test_copy_gc_after_a_collect(gpu, eng, base):
    dst = swept = None
    try:
        dst = gpu.Pool(*CAP)
        want = _collect(gpu, eng, base.src, base.m, dst, base.roots[1])
        blobs = base.m.blobs()
        wlive = G.mark(base.m.blob_bytes, blobs, base.roots[1], base.src.pool_bytes)[3]
        assert eng.gc_live_device() != 0
        live, table = eng.copy_gc(align16=True)
        assert live.tobytes() == wlive.tobytes()
        assert table.tobytes() == dst.table().tobytes() == want[3].blobs().tobytes()
        live, tight = eng.copy_gc(align16=False)
        assert tight.tobytes() == G.layout(blobs, wlive, False)[0].tobytes()
        # bsg_engine_gc_compact on the source's pointers still works
        end = want[2]["need_bytes"]
        swept = gpu.DeviceBuffer(P.align16(end))
        rc, n = eng.gc_compact(base.src.ptr, swept, align16=True, pool_bytes=base.src.pool_bytes)
        assert rc == G.OK and n == end
        assert swept.to_host(0, end).tobytes() == dst.to_host(end).tobytes()
    finally:
        for x in (dst, swept):
            if x is not None:
                x.free()


# ---- 8. reset ----------------------------------------------------------------------------------
def test_reset_alternates_two_pools(gpu, eng, base):
    a, b = gpu.Pool(*CAP), gpu.Pool(*CAP)
    ma = P.Model(*CAP)
    try:
        for second in (False, True):
            buf, run, _ = _start(gpu, eng, base.streams[second])
            try:
                _put(eng, a, ma, run)
            finally:
                buf.free()
        roots = base.roots[1]
        mb = _collect(gpu, eng, a, ma, b, roots)[3]
        assert a.where_device()
        a.reset()
        assert a.stat() == P.Model(*CAP).stat() and not a.where_device() and not a.remap_device()
        assert gpu.lib().bsg_pool_copy_where(a.h, None, 0) == C.ESTATE
        want = _collect(gpu, eng, b, mb, a, roots)
        assert want[2]["gc"]["ndead"] == 0
        assert _state(a) == _state(b)
        # and once more round: B is a put target again after its reset
        b.reset()
        _collect(gpu, eng, a, want[3], b, roots[:1])
    finally:
        a.free()
        b.free()


def test_reset_pool_is_a_new_pool(gpu, eng, base):
    cap = (1 << 20, 1 << 12)
    used, fresh = gpu.Pool(*cap), gpu.Pool(*cap)
    m = P.Model(*cap)
    small = [splitmix_array(8, 30_000), splitmix_array(9, 4_001)]
    try:
        _collect(gpu, eng, base.src, base.m, used, base.roots[0][1:2])
        buf, run, _ = _start(gpu, eng, small, fanout=2)
        try:
            _put(eng, used, C.collect(base.m, base.roots[0][1:2], *cap)[3], run)
            used.reset()
            empty = _raw(gpu, used)
            assert empty[:3] == _raw(gpu, fresh)[:3] and not empty[3] and not empty[4]
            want = m.put(run)[1]
            assert eng.pool_put(used) == want and eng.pool_put(fresh) == want
            _same(used, m)
            assert _raw(gpu, used)[:3] == _raw(gpu, fresh)[:3]
            assert used.where().tobytes() == fresh.where().tobytes()
        finally:
            buf.free()
    finally:
        used.free()
        fresh.free()


# ---- 9. the destination's index wraps ----------------------------------------------------------
def test_index_wraps(gpu, eng, oracle, table):
    streams, want_run, m0 = _wrap_case(oracle, table)
    assert P.slots_of(8) == 16 and m0.wrapped() and len(m0.table) <= 8
    src, ms, dst = gpu.Pool(1 << 16, 64), P.Model(1 << 16, 64), gpu.Pool(1 << 16, 8)
    buf = _run(gpu, eng, streams, 6, 64, 3)
    try:
        recs = eng.chunks()
        roots, _, nodes, arena = eng.trees()
        run = (recs, streams, nodes, arena)
        assert recs.tobytes() == want_run[0].tobytes()
        _put(eng, src, ms, run)
        md = _collect(gpu, eng, src, ms, dst, [r.tobytes() for r in roots])[3]
        assert md.table == m0.table and md.wrapped() == m0.wrapped()
        assert 0 in C.taken_slots(md) and 15 in C.taken_slots(md)
        again = _put(eng, dst, md, run)                   # every ref is found, past the last slot
        assert again["added"] == 0 and again["known"] == again["items"]
        _same(dst, md)
        _restored(gpu, eng, dst, [r.tobytes() for r in roots], streams, verify=True)
    finally:
        buf.free()
        for p in (src, dst):
            p.free()


# ---- 10. two threads ---------------------------------------------------------------------------
def _in_threads(jobs):
    go, errs = threading.Barrier(len(jobs)), []

    def work(job):
        try:
            go.wait()
            job()
        except BaseException as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(j,)) for j in jobs]
    for x in th:
        x.start()
    for x in th:
        x.join(60)
    assert not any(x.is_alive() for x in th), "deadlock"
    assert not errs, errs


def test_two_engines_collect_one_source(gpu, base):
    engs = [gpu.Engine(), gpu.Engine()]
    dsts = [gpu.Pool(*CAP), gpu.Pool(*CAP)]
    out = [None, None]
    roots = W.roots_array(base.roots[1])
    try:
        def job(t):
            return lambda: out.__setitem__(t, engs[t].pool_collect(base.src, dsts[t], roots))

        _in_threads([job(0), job(1)])
        want = C.collect(base.m, base.roots[1], *CAP)
        for t in range(2):
            assert out[t][0] == C.OK and out[t][1] == want[2]
            _same(dsts[t], want[3])
            assert dsts[t].remap().tolist() == want[4].tolist()
    finally:
        for x in engs:
            x.close()
        for p in dsts:
            p.free()


def test_a_to_b_beside_c_to_a(gpu, base):
    engs = [gpu.Engine(), gpu.Engine()]
    a, b, c = gpu.Pool(*CAP), gpu.Pool(*CAP), gpu.Pool(*CAP)
    out = [None, None]
    try:
        # C: run 1's blobs. A -> B with a zero Root gives an empty B whether C -> A came first
        # or not; what matters is that the two calls, which both lock A, end.
        mc = C.collect(base.m, base.roots[0], *CAP)[3]
        assert engs[0].pool_collect(base.src, c, W.roots_array(base.roots[0]))[0] == C.OK
        r0 = W.roots_array(base.roots[0][:1])
        rz = W.roots_array([bytes(32)])
        jobs = [lambda: out.__setitem__(0, engs[0].pool_collect(a, b, rz)),
                lambda: out.__setitem__(1, engs[1].pool_collect(c, a, r0))]
        _in_threads(jobs)
        assert out[0][0] == C.OK and out[1][0] == C.OK
        _same(a, C.collect(mc, base.roots[0][:1], *CAP)[3])
        assert b.stat()["nblobs"] == 0
        # now the other way round at once: A -> B beside B -> A with B empty and A not
        ma = C.collect(mc, base.roots[0][:1], *CAP)[3]
        jobs = [lambda: out.__setitem__(0, engs[0].pool_collect(a, b, r0)),
                lambda: out.__setitem__(1, engs[1].pool_collect(b, a, rz))]
        _in_threads(jobs)
        assert out[1][0] == C.ESTATE                       # A is not empty, whoever came first
        assert out[0][0] == C.OK
        _same(b, ma)
        _same(a, ma)
    finally:
        for x in engs:
            x.close()
        for p in (a, b, c):
            p.free()


# ---- 11. the walk and the restore on a pool against the host-table forms -----------------------
def _both_walks(gpu, eng, pool, roots):
    """bsg_engine_walk fed bsg_pool_copy_table, then bsg_pool_walk: equal in everything. Returns
    (rc, sizes)."""
    blobs, ra = pool.table(), W.roots_array(roots)
    rc0, info0, st0 = eng.walk(pool.ptr, blobs, ra, pool_bytes=pool.pool_bytes)
    res0 = [x.tobytes() for x in eng.copy_walk()] if rc0 == W.OK else None
    rc1, info1, st1 = eng.pool_walk(pool, ra)
    assert (rc1, info1, st1.tolist()) == (rc0, info0, st0.tolist())
    if rc1 != W.OK:
        assert gpu.lib().bsg_engine_copy_walk(eng.h, None, 0, None, None, 0) == W.ESTATE
        assert eng.walk_records_device() == 0
        return rc1, None
    recs, sizes, counts = eng.copy_walk()
    assert [x.tobytes() for x in (recs, sizes, counts)] == res0
    assert eng.walk_records_device() != 0
    return rc1, sizes


def test_pool_walk_and_restore_against_the_host_table_forms(gpu, eng, base):
    pool = base.src
    good = base.roots[0] + base.roots[1]
    chunk = base.runs[1][0][3]["ref"].tobytes()
    rc, sizes = _both_walks(gpu, eng, pool, good)
    assert rc == W.OK
    gone = bytes(range(2, 34))
    assert _both_walks(gpu, eng, pool, good[:2] + [gone] + good[2:])[0] == W.ENOTFOUND
    assert _both_walks(gpu, eng, pool, [good[0], chunk])[0] == W.ECORRUPT
    rc, sizes = _both_walks(gpu, eng, pool, [good[1], bytes(32), good[4]])
    assert rc == W.OK and sizes[1] == 0
    streams = [base.streams[0][1], np.zeros(0, np.uint8), base.streams[1][1]]
    off, cap = W.out_layout(sizes)
    blobs = pool.table()
    for verify in (False, True):
        outs = []
        for native in (False, True):
            obuf = gpu.DeviceBuffer(W.GUARD + cap + W.GUARD)
            try:
                obuf.from_host(np.full(obuf.nbytes, W.FILL, dtype=np.uint8))
                if native:
                    res = eng.pool_restore_walk(pool, obuf.ptr + W.GUARD, off, verify=verify,
                                                out_cap=cap)
                else:
                    res = eng.restore_walk(pool.ptr, blobs, obuf.ptr + W.GUARD, off, verify=verify,
                                           pool_bytes=pool.pool_bytes, out_cap=cap)
                outs.append((res, obuf.to_host().tobytes()))
            finally:
                obuf.free()
        assert outs[0] == outs[1] and outs[1][0][0] == W.OK
        got = np.frombuffer(outs[1][1], dtype=np.uint8)
        for s, d in enumerate(streams):
            o = W.GUARD + off[s]
            assert got[o:o + len(d)].tobytes() == bytes(d), s
    # an output range inside the pool, and the wrong stream count
    for native in (False, True):
        at = pool.ptr + 4096
        if native:
            res = eng.pool_restore_walk(pool, at, off, out_cap=cap)
        else:
            res = eng.restore_walk(pool.ptr, blobs, at, off, pool_bytes=pool.pool_bytes,
                                   out_cap=cap)
        assert res[0] == W.EINVAL, (native, res)
    assert eng.pool_restore_walk(pool, pool.ptr, off[:2], out_cap=cap)[0] == W.EINVAL
    assert base.state == _state(pool)

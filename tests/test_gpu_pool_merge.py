"""bsg_pool_merge and bsg_pool_sync on the device against the model of merge_cases.py, every
comparison an equality and the destination's allocation in full: merges with one run's Roots,
all, none and repeated Roots into a destination that holds the other run, the same run or
nothing, ALL over dead blobs, an unaligned end, a known ref with another len, failed marks,
capacity, BSG_MERGE_VERIFY with a planted flip, the merged pool in use, an index cluster that
wraps, states and arguments, two threads, and sync."""
import ctypes

import numpy as np
import pytest

import collect_cases as C
import merge_cases as M
import pool_cases as P
import walk_cases as W
from bs_amd.synth import splitmix_array
from test_gpu_engine_trees import _run
from test_gpu_pool import _wrap_case
from test_gpu_pool_collect import (BITS, CAP, FANOUT, MN, _in_threads, _put, _raw, _restored,
                                   _start, _streams, eng)  # noqa: F401  (eng: a fixture)

pytestmark = pytest.mark.gpu


class Base:
    """Pools that no test writes: one (run 1), two (run 2), both (run 1 then run 2), with their
    models, the runs, their Roots and their streams. The runs share stream B whole and most of
    stream A, so chunks and nodes repeat across the pools."""


@pytest.fixture(scope="module")
def base(gpu):
    b, e = Base(), gpu.Engine()
    b.pools = {k: gpu.Pool(*CAP) for k in ("one", "two", "both")}
    b.m = {k: P.Model(*CAP) for k in b.pools}
    b.runs, b.roots, b.streams = [], [], []
    try:
        for i, second in enumerate((False, True)):
            streams = _streams(second)
            buf, run, roots = _start(gpu, e, streams)
            try:
                for k in (("one", "two")[i], "both"):
                    _put(e, b.pools[k], b.m[k], run)
            finally:
                buf.free()
            b.runs.append(run)
            b.roots.append(roots)
            b.streams.append(streams)
        state = {k: _whole(gpu, p) for k, p in b.pools.items()}
        yield b
        assert {k: _whole(gpu, p) for k, p in b.pools.items()} == state, "a test wrote a source"
    finally:
        e.close()
        for p in b.pools.values():
            p.free()


def _whole(gpu, pool):
    """The counters, the whole allocation and every table entry up to the capacity."""
    return _raw(gpu, pool)[:3]


def _is(gpu, pool, m):
    """The pool equals the model: counters, table, and the bytes over the whole allocation (zero
    behind the model's last padding)."""
    st, raw, table = _whole(gpu, pool)
    assert st == m.stat(), (st, m.stat())
    want = np.zeros(st["pool_bytes"], dtype=np.uint8)
    want[:len(m.buf)] = m.buf
    assert raw == want.tobytes()
    tb = np.zeros(max(st["cap_blobs"], 1), dtype=gpu.POOL_BLOB_DTYPE)
    tb[:len(m.table)] = m.blobs()
    assert table == tb.tobytes()


def _holding(gpu, eng, base, which, cap=CAP):
    """A fresh pool (and its model) that holds what base.pools[which] holds, by a collect of all
    its Roots (no blob of these pools is dead)."""
    roots = {"one": base.roots[0], "two": base.roots[1], "both": base.roots[0] + base.roots[1]}
    rc, _, info, m, _ = C.collect(base.m[which], roots[which], *cap)
    assert rc == C.OK and info["gc"]["ndead"] == 0
    p = gpu.Pool(*cap)
    assert eng.pool_collect(base.pools[which], p, W.roots_array(roots[which]))[0] == C.OK
    return p, m


def _merge(gpu, eng, src, m_src, dst, m_dst, roots=None, flags=0, expect=M.OK):
    """One merge on the device and in the model: the return code, the status, the info and, on
    success, the destination in full and the remap equal; on failure the destination is as it
    was. Returns the model's tuple."""
    want = M.merge(m_src, m_dst, roots, flags)
    assert want[0] == expect, (want[0], expect, want[2])
    before = _raw(gpu, dst)
    rc, info, status = eng.pool_merge(src, dst, None if flags & M.ALL else W.roots_array(roots),
                                      all=bool(flags & M.ALL), verify=bool(flags & M.VERIFY),
                                      missing_leaves=bool(flags & M.MISSING_LEAVES))
    print("merge", rc, info)
    assert rc == want[0], (rc, want[0], info, want[2])
    assert info == want[2], (info, want[2])
    assert status.tolist() == ([] if want[1] is None else want[1].tolist())
    if rc != M.OK:
        assert _raw(gpu, dst) == before
        return want
    _is(gpu, dst, want[3])
    assert dst.remap().tolist() == want[4].tolist()
    assert (dst.remap_device() != 0) == (len(want[4]) > 0)
    assert before[4] == dst.where_device()
    return want


def _read_all(gpu, eng, pool, roots, streams):
    """bsg_pool_read of every Root's whole stream, verified: the streams bit for bit."""
    off, cap = W.out_layout([len(d) for d in streams])
    out = gpu.DeviceBuffer(cap + 16)
    try:
        rc, status, got, info = pool.read(eng, [(r, 0, len(d)) for r, d in zip(roots, streams)],
                                          out, off, flags=gpu.READ_VERIFY)
        assert rc == W.OK and not status.any(), (rc, status, info)
        host = out.to_host()
        for s, d in enumerate(streams):
            assert int(got[s]) == len(d) and host[off[s]:off[s] + len(d)].tobytes() == bytes(d), s
    finally:
        out.free()


# ---- 1. Roots of every kind into a destination that holds the other run, the same run, nothing --
@pytest.mark.parametrize("held", ["two", "one", None])
def test_roots_into(gpu, eng, base, held):
    r1 = base.roots[0]
    for roots in (r1, r1 + base.roots[1], [], [bytes(32)] * 3,
                  [r1[0]] * 300 + [bytes(32)] + [r1[2]] * 3):
        if held:
            dst, md = _holding(gpu, eng, base, held)
        else:
            dst, md = gpu.Pool(*CAP), P.Model(*CAP)
        other = gpu.Pool(*CAP)
        try:
            want = _merge(gpu, eng, base.pools["both"], base.m["both"], dst, md, roots)
            info = want[2]
            if held == "two" and roots and any(roots[0]):
                assert info["added"] > 0 and info["known"] > 0            # partial overlap
            if held == "one" and roots == r1:
                assert info["added"] == 0 and info["need_bytes"] == md.bytes
                assert info["known"] == info["selected"] > 0
            if held is None:                                             # a collect, directly
                got = eng.pool_collect(base.pools["both"], other, W.roots_array(roots))
                assert got[0] == C.OK and got[1]["gc"] == info["gc"]
                assert _whole(gpu, other) == _whole(gpu, dst)
                assert other.remap().tobytes() == dst.remap().tobytes()
        finally:
            dst.free()
            other.free()


# ---- 2. ALL on a source that also holds dead blobs; an unaligned end ----------------------------
def test_all_takes_dead_blobs_too(gpu, eng, base):
    dst, md = _holding(gpu, eng, base, "one")
    try:
        assert md.bytes % 16 != 0, md.bytes                      # the base is rounded up
        live = M.merge(base.m["both"], md, base.roots[0])[2]
        assert live["gc"]["ndead"] > 0
        want = _merge(gpu, eng, base.pools["both"], base.m["both"], dst, md, None, M.ALL)
        assert want[2]["added"] == live["gc"]["ndead"] and want[2]["selected"] == len(want[4])
        base_off = P.align16(md.bytes)
        raw = dst.to_host(want[3].bytes)
        assert not raw[md.bytes:base_off].any() and want[3].table[len(md.table)][0] == base_off
        for o, n, _ in want[3].table[len(md.table):]:
            assert o % 16 == 0 and not raw[o + n:P.align16(o + n)].any()
        # the engine's gc result is left as it was: the collect's, of _holding
        live, _ = eng.copy_gc()
        assert len(live) == len(base.m["one"].table)
    finally:
        dst.free()


# ---- 3. a known ref with another len ------------------------------------------------------------
def test_known_ref_with_another_len_stays(gpu, eng, base):
    """No call gives a pool a ref over another len (a ref is the hash of the bytes a put stores),
    so the destination's table entry is edited where it lies: one byte shorter."""
    dst, md = _holding(gpu, eng, base, "one")
    try:
        ms = base.m["two"]
        j = next(j for j, (_, n, r) in enumerate(md.table) if r in ms.index and n > 1)
        o, n, r = md.table[j]
        md.table[j] = (o, n - 1, r)
        at = gpu.lib().bsg_pool_table_device(dst.h) + 48 * j + 8
        assert gpu.lib().bsg_memcpy(dst.device, at, np.array([n - 1], dtype="<u8").ctypes.data,
                                    8, 0) == 0
        _is(gpu, dst, md)
        want = _merge(gpu, eng, base.pools["two"], ms, dst, md, None, M.ALL)
        assert want[3].table[j] == (o, n - 1, r) and int(want[4][ms.index[r]]) == j
        assert want[2]["known"] > 0 and want[2]["added"] > 0
        assert ms.table[ms.index[r]][1] == n
    finally:
        dst.free()


# ---- 4. failed marks and capacity: the destination stays as it was ------------------------------
def test_failed_marks_leave_the_destination(gpu, eng, base):
    dst, md = _holding(gpu, eng, base, "one")
    only, mo = gpu.Pool(*CAP), P.Model(*CAP)
    buf, run, roots = _start(gpu, eng, base.streams[1])
    try:
        gone = bytes(range(1, 33))
        chunk = base.runs[1][0][7]["ref"].tobytes()
        src, ms = base.pools["two"], base.m["two"]
        r2 = base.roots[1]
        want = _merge(gpu, eng, src, ms, dst, md, [r2[0], gone, r2[2]], expect=M.ENOTFOUND)
        assert want[1].tolist() == [0, M.ENOTFOUND, 0] and want[2]["gc"]["bad_root"] == 1
        want = _merge(gpu, eng, src, ms, dst, md, [r2[1], chunk], expect=M.ECORRUPT)
        assert want[1].tolist() == [0, M.ECORRUPT]
        assert gpu.lib().bsg_engine_copy_gc(eng.h, None, 0, None, 0, 0) == M.ESTATE
        # a missing leaf, without and with the flag
        _put(eng, only, mo, run, chunks=False)
        _merge(gpu, eng, only, mo, dst, md, roots, expect=M.ENOTFOUND)
        want = _merge(gpu, eng, only, mo, dst, md, roots, M.MISSING_LEAVES)
        assert want[2]["gc"]["missing_leaves"] > 0 and want[2]["added"] > 0
    finally:
        buf.free()
        only.free()
        dst.free()


def test_capacity(gpu, eng, base):
    src, ms, roots = base.pools["two"], base.m["two"], base.roots[1]
    need = M.merge(ms, base.m["one"], roots)[2]
    nb, nn = need["need_bytes"], need["need_blobs"]
    assert need["added"] > 1
    for cb, cn in ((nb, nn - 1), (nb - 1, nn), (nb, nn)):
        dst, md = _holding(gpu, eng, base, "one", (cb, cn))
        try:
            fits = (cb, cn) == (nb, nn)
            want = _merge(gpu, eng, src, ms, dst, md, roots, expect=M.OK if fits else M.ENOMEM)
            assert want[2] == need
            if not fits:
                live, _ = eng.copy_gc()                            # the mark stands
                assert int(live.sum()) == need["selected"]
            else:
                _restored(gpu, eng, dst, base.roots[0] + roots,
                          base.streams[0] + base.streams[1], verify=True)
        finally:
            dst.free()


# ---- 5. BSG_MERGE_VERIFY -------------------------------------------------------------------------
def _flipped(gpu, eng, base, stream, at):
    """A pool of run 2 whose input had one byte flipped after the refs were taken, with its
    model, and the index of the blob that holds the flipped byte."""
    src, ms = gpu.Pool(*CAP), P.Model(*CAP)
    streams = [d.copy() for d in base.streams[1]]
    buf, run, roots = _start(gpu, eng, streams)
    try:
        off = [0]
        for d in streams:
            off.append(off[-1] + P.align16(len(d)))
        streams[stream][at] ^= 0x40
        buf.from_host(streams[stream][at:at + 1], off[stream] + at)
        _put(eng, src, ms, (run[0], streams, run[2], run[3]))
        recs = run[0]
        i = next(i for i in range(len(recs)) if recs[i]["stream"] == stream
                 and recs[i]["offset"] <= at < recs[i]["offset"] + recs[i]["len"])
        return src, ms, int(src.where()[i]), roots
    except BaseException:
        src.free()
        raise
    finally:
        buf.free()


def test_verify(gpu, eng, base):
    dst, md = _holding(gpu, eng, base, "one")
    try:
        # a clean merge
        want = _merge(gpu, eng, base.pools["two"], base.m["two"], dst, md, base.roots[1],
                      M.VERIFY)
        assert want[2]["verified"] == want[2]["added_bytes"] > 0
        assert want[2]["bad_blob"] == M.NONE
    finally:
        dst.free()
    # stream 2 of run 2 is new to run 1: a flip there is in a blob to append
    src, ms, k, roots = _flipped(gpu, eng, base, 2, 60_000)
    dst, md = _holding(gpu, eng, base, "one")
    try:
        assert ms.table[k][2] not in md.index
        want = _merge(gpu, eng, src, ms, dst, md, roots, M.VERIFY, expect=M.ECORRUPT)
        assert want[2]["bad_blob"] == k
        want = _merge(gpu, eng, src, ms, dst, md, None, M.ALL | M.VERIFY, expect=M.ECORRUPT)
        assert want[2]["bad_blob"] == k
        # the same blob dead: Roots that do not reach it
        want = _merge(gpu, eng, src, ms, dst, md, roots[:2], M.VERIFY)
        assert want[4][k] == M.NONE and want[2]["added"] > 0
    finally:
        src.free()
        dst.free()
    # stream 1 of run 2 is run 1's stream B: a flip there is in a blob the destination knows
    src, ms, k, roots = _flipped(gpu, eng, base, 1, 60_000)
    dst, md = _holding(gpu, eng, base, "one")
    try:
        assert ms.table[k][2] in md.index
        want = _merge(gpu, eng, src, ms, dst, md, roots, M.VERIFY)
        assert want[4][k] == md.index[ms.table[k][2]] and want[2]["added"] > 0
    finally:
        src.free()
        dst.free()


# ---- 6. the merged pool in use -------------------------------------------------------------------
def test_the_merged_pool_is_a_pool(gpu, eng, base):
    dst, md = _holding(gpu, eng, base, "one")
    third = [splitmix_array(11, 130_001), base.streams[1][2]]
    coll, more = gpu.Pool(*CAP), gpu.Pool(*CAP)
    try:
        md = _merge(gpu, eng, base.pools["two"], base.m["two"], dst, md, base.roots[1])[3]
        roots = base.roots[0] + base.roots[1]
        streams = base.streams[0] + base.streams[1]
        buf, run3, roots3 = _start(gpu, eng, third)
        try:
            info = _put(eng, dst, md, run3)
            assert info["added"] > 0 and info["known"] > 0
            _is(gpu, dst, md)
        finally:
            buf.free()
        _restored(gpu, eng, dst, roots + roots3, streams + third, verify=True)
        _read_all(gpu, eng, dst, roots + roots3, streams + third)
        # a collect out of it, and a further merge of it into that
        want = C.collect(md, base.roots[1], *CAP)
        got = eng.pool_collect(dst, coll, W.roots_array(base.roots[1]))
        assert got[0] == C.OK and got[1] == want[2]
        _is(gpu, coll, want[3])
        _merge(gpu, eng, dst, md, coll, want[3], roots3 + base.roots[0][:1])
        # every ref is known to a put of the runs
        mm = _merge(gpu, eng, dst, md, more, P.Model(*CAP), None, M.ALL)[3]
        buf, run1, _ = _start(gpu, eng, base.streams[0])
        try:
            again = _put(eng, more, mm, run1)
            assert again["added"] == 0 and again["known"] == again["items"]
        finally:
            buf.free()
    finally:
        for p in (dst, coll, more):
            p.free()


# ---- 7. the destination's index wraps ------------------------------------------------------------
def test_index_wraps(gpu, eng, oracle, table):
    streams, want_run, m0 = _wrap_case(oracle, table)
    assert P.slots_of(8) == 16 and m0.wrapped() and len(m0.table) <= 8
    src, ms = gpu.Pool(1 << 16, 64), P.Model(1 << 16, 64)
    dst, md = gpu.Pool(1 << 16, 8), P.Model(1 << 16, 8)
    buf = _run(gpu, eng, streams, 6, 64, 3)
    try:
        recs = eng.chunks()
        roots, _, nodes, arena = eng.trees()
        run = (recs, streams, nodes, arena)
        assert recs.tobytes() == want_run[0].tobytes()
        _put(eng, src, ms, run)
        _put(eng, dst, md, run, nodes=False)               # the chunks; the merge adds the nodes
        rl = [r.tobytes() for r in roots]
        out = _merge(gpu, eng, src, ms, dst, md, rl)[3]
        assert out.table == m0.table and out.wrapped() == m0.wrapped()
        assert 0 in C.taken_slots(out) and 15 in C.taken_slots(out)
        assert len(out.table) > len(md.table) > 0
        again = _put(eng, dst, out, run)                   # every ref is found, past the last slot
        assert again["added"] == 0 and again["known"] == again["items"]
        again = _merge(gpu, eng, src, ms, dst, out, rl)
        assert again[2]["added"] == 0 and again[2]["known"] == len(out.table)
        _restored(gpu, eng, dst, rl, streams, verify=True)
    finally:
        buf.free()
        for p in (src, dst):
            p.free()


# ---- 8. states and arguments, in the order of the header ----------------------------------------
def test_states_and_arguments(gpu, eng, base):
    L = gpu.lib()
    src = base.pools["two"]
    dst, _ = _holding(gpu, eng, base, "one")
    small = gpu.Pool(1 << 12, 4)
    roots = W.roots_array(base.roots[1])
    info = gpu.PoolMergeInfo()
    pair = (gpu.PoolMergeInfo * 2)()
    try:
        def call(e, s, d, r=roots.ctypes.data, n=len(roots), f=0):
            return L.bsg_pool_merge(e, s, d, r, n, f, None, ctypes.byref(info))

        before = _raw(gpu, dst)
        for args in ((None, src.h, dst.h), (eng.h, None, dst.h), (eng.h, src.h, None),
                     (eng.h, dst.h, dst.h)):
            assert call(*args) == M.EINVAL, args
        assert call(eng.h, src.h, dst.h, f=8) == M.EINVAL
        assert call(eng.h, src.h, dst.h, f=M.ALL) == M.EINVAL                # ALL with Roots
        assert call(eng.h, src.h, dst.h, r=None, n=0, f=M.ALL | 1) == M.EINVAL
        assert call(eng.h, src.h, dst.h, n=1 << 32) == M.EINVAL
        assert call(eng.h, src.h, dst.h, r=None) == M.EINVAL
        for args in ((None, src.h, dst.h), (eng.h, None, dst.h), (eng.h, src.h, None),
                     (eng.h, dst.h, dst.h)):
            assert L.bsg_pool_sync(*args, 0, pair) == M.EINVAL, args
        for f in (1, 2, 8):
            assert L.bsg_pool_sync(eng.h, src.h, dst.h, f, pair) == M.EINVAL
        # dead pools, either side; EINVAL comes first
        for dead, args in ((small, (small.h, dst.h)), (small, (src.h, small.h))):
            assert L.bsg_pool_kill_debug(dead.h) == 0
            assert call(eng.h, *args, f=8) == M.EINVAL
            assert call(eng.h, *args) == M.ESTATE
            assert L.bsg_pool_sync(eng.h, *args, 0, None) == M.ESTATE
            dead.reset()
        # an unfinished run
        buf = gpu.DeviceBuffer(1 << 16)
        try:
            buf.from_host(splitmix_array(5, 1 << 16))
            eng.run(buf.ptr, [0], [1 << 16], bits=BITS, min_size=MN, fanout=FANOUT)
            assert call(eng.h, src.h, dst.h) == M.ESTATE
            assert L.bsg_pool_sync(eng.h, src.h, dst.h, 0, pair) == M.ESTATE
            eng.finish()
        finally:
            buf.free()
        assert _raw(gpu, dst) == before
        # the mark's code before the capacity's
        gone = W.roots_array([bytes(range(1, 33))])
        assert call(eng.h, src.h, small.h, r=gone.ctypes.data, n=1) == M.ENOTFOUND
        assert call(eng.h, src.h, small.h) == M.ENOMEM and info.need_blobs > 4
        assert small.stat()["nblobs"] == 0 and not small.remap_device()
        # null info and status; an empty source; no Roots
        assert L.bsg_pool_merge(eng.h, small.h, dst.h, None, 0, M.ALL, None, None) == M.OK
        assert not dst.remap_device() and L.bsg_pool_copy_remap(dst.h, None, 0) == M.OK
        assert L.bsg_pool_merge(eng.h, src.h, dst.h, None, 0, 0, None, None) == M.OK
        assert _raw(gpu, dst)[:3] == before[:3]
        dst._nremap = src.stat()["nblobs"]
        assert len(dst.remap()) > 0 and (dst.remap() == gpu.NONE64).all()
    finally:
        dst.free()
        small.free()


# ---- 9. two threads: A -> B beside B -> A --------------------------------------------------------
def test_a_to_b_beside_b_to_a(gpu, base):
    engs = [gpu.Engine(), gpu.Engine()]
    a, ma = _holding(gpu, engs[0], base, "one")
    b, mb = _holding(gpu, engs[0], base, "two")
    out = [None, None]
    try:
        jobs = [lambda: out.__setitem__(0, engs[0].pool_merge(a, b, all=True)),
                lambda: out.__setitem__(1, engs[1].pool_merge(b, a, all=True))]
        _in_threads(jobs)
        assert out[0][0] == M.OK and out[1][0] == M.OK
        # A -> B first, then B -> A; or the other way round
        ab = M.merge(ma, mb, None, M.ALL)
        ab_ba = M.merge(ab[3], ma, None, M.ALL)
        ba = M.merge(mb, ma, None, M.ALL)
        ba_ab = M.merge(ba[3], mb, None, M.ALL)
        first = (out[0][1], out[1][1]) == (ab[2], ab_ba[2])
        assert first or (out[0][1], out[1][1]) == (ba_ab[2], ba[2])
        wa, wb = (ab_ba[3], ab[3]) if first else (ba[3], ba_ab[3])
        _is(gpu, a, wa)
        _is(gpu, b, wb)
        assert {r for _, _, r in wa.table} == {r for _, _, r in wb.table}
    finally:
        for x in engs:
            x.close()
        a.free()
        b.free()


# ---- 10. sync ------------------------------------------------------------------------------------
def _sync(gpu, eng, a, ma, b, mb, flags=0, expect=M.OK):
    want = M.sync(ma, mb, flags)
    assert want[0] == expect, (want[0], expect, want[1])
    before = _raw(gpu, a), _raw(gpu, b)
    rc, info, status = eng.pool_sync(a, b, verify=bool(flags & M.VERIFY))
    print("sync", rc, info)
    assert rc == want[0] and info == want[1], (rc, info, want[1])
    assert len(status) == 0
    if rc != M.OK:
        assert (_raw(gpu, a), _raw(gpu, b)) == before
        return want
    _is(gpu, a, want[2])
    _is(gpu, b, want[3])
    assert b.remap().tolist() == want[4].tolist() and a.remap().tolist() == want[5].tolist()
    assert {r for _, _, r in want[2].table} == {r for _, _, r in want[3].table}
    return want


def test_sync(gpu, eng, base):
    roots = base.roots[0] + base.roots[1]
    streams = base.streams[0] + base.streams[1]
    third = [splitmix_array(11, 130_001)]
    made = []

    def pools(ka, kb):
        out = []
        for k in (ka, kb):
            out += list(_holding(gpu, eng, base, k) if k else (gpu.Pool(*CAP), P.Model(*CAP)))
            made.append(out[-2])
        return out

    try:
        # overlapping pools, with the verification; both are readable for every Root afterwards
        a, ma, b, mb = pools("one", "two")
        want = _sync(gpu, eng, a, ma, b, mb, M.VERIFY)
        assert all(i["added"] > 0 and i["known"] > 0 for i in want[1])
        assert want[1][0]["verified"] == want[1][0]["added_bytes"]
        for p in (a, b):
            _restored(gpu, eng, p, roots, streams, verify=True)
            _read_all(gpu, eng, p, roots, streams)
        again = _sync(gpu, eng, a, want[2], b, want[3])               # both equal as sets
        assert [i["added"] for i in again[1]] == [0, 0]
        # disjoint pools
        c, mc = gpu.Pool(*CAP), P.Model(*CAP)
        made.append(c)
        buf, run3, roots3 = _start(gpu, eng, third)
        try:
            _put(eng, c, mc, run3)
        finally:
            buf.free()
        a, ma, _, _ = pools("one", None)
        want = _sync(gpu, eng, a, ma, c, mc)
        assert [i["known"] for i in want[1]] == [0, 0]
        _restored(gpu, eng, a, base.roots[0] + roots3, base.streams[0] + third, verify=True)
        _restored(gpu, eng, c, base.roots[0] + roots3, base.streams[0] + third, verify=True)
        # one empty, either side; both the same
        a, ma, b, mb = pools("both", None)
        _sync(gpu, eng, a, ma, b, mb)
        a, ma, b, mb = pools(None, "two")
        _sync(gpu, eng, a, ma, b, mb)
        a, ma, b, mb = pools("two", "two")
        want = _sync(gpu, eng, a, ma, b, mb)
        assert want[4].tolist() == want[5].tolist() == list(range(len(ma.table)))
    finally:
        for p in made:
            p.free()


def test_sync_is_all_or_nothing(gpu, eng, base):
    need = M.sync(base.m["one"], base.m["two"])[1]
    caps = {"first": ((need[1]["need_bytes"], need[1]["need_blobs"]),
                      (need[0]["need_bytes"], need[0]["need_blobs"] - 1)),
            "second": ((need[1]["need_bytes"] - 1, need[1]["need_blobs"]),
                       (need[0]["need_bytes"], need[0]["need_blobs"])),
            "fits": ((need[1]["need_bytes"], need[1]["need_blobs"]),
                     (need[0]["need_bytes"], need[0]["need_blobs"]))}
    for name, (ca, cb) in caps.items():
        a, ma = _holding(gpu, eng, base, "one", ca)
        b, mb = _holding(gpu, eng, base, "two", cb)
        try:
            want = _sync(gpu, eng, a, ma, b, mb, expect=M.OK if name == "fits" else M.ENOMEM)
            assert want[1] == need, name
        finally:
            a.free()
            b.free()

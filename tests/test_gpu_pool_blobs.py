"""bsg_pool_put_blobs and bsg_pool_get on the device against the model of blob_cases.py, every
comparison an equality and the pool's allocation and table in full after every call: the length
edges with scattered, descending, coinciding and empty blobs, known refs, a run's chunks and nodes
against bsg_engine_pool_put, capacity, gets of every kind, BSG_GET_VERIFY with a planted flip,
arguments and states, two threads."""
import ctypes
import hashlib

import numpy as np
import pytest

import blob_cases as B
import pool_cases as P
from bs_amd.synth import splitmix_array
from test_gpu_pool_collect import (BITS, FANOUT, MN, _in_threads, _raw, _restored, _start,
                                   _streams, eng)  # noqa: F401  (eng: a fixture)
from test_gpu_pool_merge import _is, _whole

pytestmark = pytest.mark.gpu

CAP = (1 << 20, 256)
FILL = 0xA5
MISS = [hashlib.sha256(b"no such blob %d" % i).digest() for i in range(4)]


def _device(gpu, src):
    buf = gpu.DeviceBuffer(len(src))
    buf.from_host(src)
    return buf


def _put(gpu, eng, pool, m, src, off, lens, expect=B.OK):
    """One put on the device and in the model: the return code, the info and the refs; on success
    the pool in full and where[], on failure the pool as it was."""
    before = _raw(gpu, pool)
    buf = _device(gpu, src)
    try:
        rc, info, refs = pool.put_blobs(eng, buf, off, lens)
    finally:
        buf.free()
    want = B.put_blobs(m, src, off, lens)
    print("put_blobs", rc, info)
    assert want[0] == expect and rc == want[0], (rc, want[0], info, want[1])
    assert info == want[1], (info, want[1])
    assert refs.tobytes() == b"".join(want[2])
    if rc != B.OK:
        assert _raw(gpu, pool) == before
        return info
    _is(gpu, pool, m)
    assert pool.where().tolist() == m.where.tolist()
    assert (pool.where_device() != 0) == (len(off) > 0)
    return info


def _get(gpu, eng, pool, m, refs, cap="fit", verify=False, expect=B.OK):
    """One get on the device and in the model: the return code, the info, idx and out_off; the
    output's first out_off[n] bytes on success and its fill everywhere else; the pool as it was."""
    if cap == "fit":
        cap = max(B.get(m, refs, None)[1]["need_bytes"], 16)
    want = B.get(m, refs, cap, verify)
    before = _raw(gpu, pool)
    out = gpu.DeviceBuffer((cap or 0) + 64)
    try:
        out.from_host(np.full(out.nbytes, FILL, dtype=np.uint8))
        rc, info, idx, out_off = pool.get(eng, refs, None if cap is None else out.ptr,
                                          verify=verify, out_cap=cap or 0)
        got = out.to_host()
    finally:
        out.free()
    print("get", rc, info)
    assert want[0] == expect and rc == want[0], (rc, want[0], info, want[1])
    assert info == want[1], (info, want[1])
    assert idx.tolist() == want[2].tolist() and out_off.tolist() == want[3].tolist()
    wrote = 0 if want[4] is None else len(want[4])
    if wrote:
        assert got[:wrote].tobytes() == want[4].tobytes()
    assert (got[wrote:] == FILL).all()
    assert _raw(gpu, pool) == before
    return want


@pytest.fixture()
def edges(gpu, eng):
    """A pool that holds the length edges, and its model."""
    src, off, lens, _ = B.edge_case()
    pool, m = gpu.Pool(*CAP), P.Model(*CAP)
    _put(gpu, eng, pool, m, src, off, lens)
    yield pool, m
    pool.free()


# ---- 1. the length edges; known refs ---------------------------------------------------------------
def test_length_edges_and_known_refs(gpu, eng):
    src, off, lens, facts = B.edge_case()
    assert off[:15] == sorted(off[:15], reverse=True) and 40_000 > 32768  # descending; > one tile
    pool, m = gpu.Pool(*CAP), P.Model(*CAP)
    try:
        info = _put(gpu, eng, pool, m, src, off, lens)
        assert info["added"] == facts["distinct"] and info["repeats"] == facts["repeats"]
        raw = src.tobytes()
        assert [r for _, _, r in m.table][:3] == \
            [hashlib.sha256(raw[o:o + n]).digest() for o, n in zip(off[:3], lens[:3])]
        # the same put again: nothing new, the same where[]
        where, used = pool.where().tolist(), pool.stat()["bytes"]
        info = _put(gpu, eng, pool, m, src, off, lens)
        assert info["added"] == 0 and info["known"] == facts["items"]
        assert pool.where().tolist() == where and pool.stat()["bytes"] == used
        # some known, some new, an unaligned end before them; then an empty blob alone
        more = [splitmix_array(90 + i, n) for i, n in enumerate((7, 300, 33))]
        src2, off2, lens2 = B.place([src[off[0]:off[0] + lens[0]]] + more + [more[1]])
        info = _put(gpu, eng, pool, m, src2, off2, lens2)
        assert (info["known"], info["added"], info["repeats"]) == (1, 3, 1)
        assert (pool.where() >= info["first_blob"]).tolist() == [False, True, True, True, True]
        fresh, mf = gpu.Pool(64, 2), P.Model(64, 2)
        try:
            _put(gpu, eng, fresh, mf, *B.place([b"abcde"]))
            info = _put(gpu, eng, fresh, mf, np.zeros(256 + 32, np.uint8), [16], [0])
            assert info["added"] == 1 and mf.table[1][:2] == (16, 0) and mf.bytes == 16
            _put(gpu, eng, fresh, mf, np.zeros(256, np.uint8), [], [])
            assert not fresh.where_device()
        finally:
            fresh.free()
    finally:
        pool.free()


# ---- 2. a run's chunks and nodes: bsg_engine_pool_put's pool, raw for raw --------------------------
def test_a_runs_chunks_then_nodes_is_its_put(gpu, eng):
    streams = _streams()
    buf, run, roots = _start(gpu, eng, streams)
    by_put, by_blobs = gpu.Pool(4 << 20, 1 << 14), gpu.Pool(4 << 20, 1 << 14)
    try:
        recs, _, nodes, arena = run
        info = eng.pool_put(by_put)
        chunks = [streams[int(r["stream"])][int(r["offset"]):int(r["offset"] + r["len"])]
                  for r in recs]
        blobs = [arena[int(t["blob_off"]):int(t["blob_off"]) + int(t["blob_len"])] for t in nodes]
        src, off, lens = B.place(chunks + blobs)
        d = _device(gpu, src)
        try:
            rc, got, refs = by_blobs.put_blobs(eng, d, off, lens)
        finally:
            d.free()
        assert rc == B.OK and got == info, (got, info)
        assert refs.tobytes() == recs["ref"].tobytes() + nodes["ref"].tobytes()
        assert _whole(gpu, by_blobs) == _whole(gpu, by_put)
        assert by_blobs.where().tobytes() == by_put.where().tobytes()
        # the engine's run is as it was, and the pool serves a walk and a restore
        assert eng.chunks().tobytes() == recs.tobytes()
        _restored(gpu, eng, by_blobs, roots, streams, verify=True)
    finally:
        buf.free()
        by_put.free()
        by_blobs.free()


# ---- 3. capacity -------------------------------------------------------------------------------------
def test_capacity_is_all_or_nothing(gpu, eng):
    src, off, lens, _ = B.edge_case()
    big = P.Model(*CAP)
    assert B.put_blobs(big, src, off, lens)[0] == B.OK
    fit = (big.bytes, len(big.table))
    for cap in (fit, (fit[0] - 1, fit[1]), (fit[0], fit[1] - 1)):
        pool, m = gpu.Pool(*cap), P.Model(*cap)
        try:
            info = _put(gpu, eng, pool, m, src, off, lens,
                        expect=B.OK if cap == fit else B.ENOMEM)
            assert (info["need_bytes"], info["need_blobs"]) == fit
            if cap != fit:
                assert not pool.where_device() and pool.stat()["nblobs"] == 0
        finally:
            pool.free()


# ---- 4. get ------------------------------------------------------------------------------------------
def test_get_of_every_kind(gpu, eng, edges):
    pool, m = edges
    refs = [r for _, _, r in m.table]
    empty = hashlib.sha256(b"").digest()
    assert empty in m.index
    want = _get(gpu, eng, pool, m, refs)
    assert want[1]["missing"] == 0 and want[1]["found"] == len(refs)
    want = _get(gpu, eng, pool, m, [MISS[0]] + refs[:5] + [MISS[1]] + refs[5:] + [MISS[2]])
    assert want[1]["missing"] == 3 and int(want[2][0]) == int(want[2][-1]) == B.NONE64
    k = next(k for k, (_, n, _) in enumerate(m.table) if n == 4096)
    want = _get(gpu, eng, pool, m, [refs[k], empty, refs[k], MISS[3], refs[k]])
    assert want[1]["bytes"] == 3 * 4096 and want[3].tolist() == [0, 4096, 4096, 8192, 8192, 12288]
    _get(gpu, eng, pool, m, [empty])
    _get(gpu, eng, pool, m, MISS)
    _get(gpu, eng, pool, m, [])
    _get(gpu, eng, pool, m, [], cap=None)
    # the stat form; an exact capacity, and 16 less
    want = _get(gpu, eng, pool, m, refs, cap=None)
    need = want[1]["need_bytes"]
    assert need == sum(P.align16(n) for _, n, _ in m.table) > 32768
    _get(gpu, eng, pool, m, refs, cap=need)
    want = _get(gpu, eng, pool, m, refs, cap=need - 16, expect=B.ENOMEM)
    assert want[1]["need_bytes"] == need and want[1]["found"] == len(refs)
    # padding zero: every found blob's tail
    for q, (_, n, _) in enumerate(m.table):
        o = int(want[3][q])
        assert int(want[3][q + 1]) - o == P.align16(n)


def test_a_gets_output_is_a_puts_source(gpu, eng, edges):
    pool, m = edges
    refs = [r for _, _, r in m.table][::-1] + [MISS[0]]
    want = B.get(m, refs, None)
    out, fresh = gpu.DeviceBuffer(want[1]["need_bytes"]), gpu.Pool(*CAP)
    try:
        rc, info, idx, out_off = pool.get(eng, refs, out)
        assert rc == B.OK and info == want[1]
        lens = [m.table[int(k)][1] if int(k) != B.NONE64 else 0 for k in idx]
        rc, info, got = fresh.put_blobs(eng, out, out_off[:-1], lens)
        assert rc == B.OK and info["added"] == len(m.table)
        assert got.tobytes()[:-32] == b"".join(refs[:-1])
        assert got.tobytes()[-32:] == hashlib.sha256(b"").digest()    # the missing ref: no bytes
        mf = P.Model(*CAP)
        assert B.put_blobs(mf, out.to_host(), out_off[:-1], lens)[0] == B.OK
        _is(gpu, fresh, mf)
    finally:
        out.free()
        fresh.free()


# ---- 5. BSG_GET_VERIFY -------------------------------------------------------------------------------
def test_verify_and_a_planted_flip(gpu, eng, edges):
    pool, m = edges
    refs = [r for _, _, r in m.table]
    want = _get(gpu, eng, pool, m, refs + refs[:3], verify=True)
    assert want[1]["verified"] == sum(n for _, n, _ in m.table) and want[1]["bad_blob"] == B.NONE64
    k = next(k for k, (_, n, _) in enumerate(m.table) if n == 65)
    at = m.table[k][0] + 64
    m.buf[at] ^= 1
    assert gpu.lib().bsg_memcpy(pool.device, pool.ptr + at, m.buf[at:at + 1].ctypes.data, 1, 0) == 0
    _is(gpu, pool, m)
    want = _get(gpu, eng, pool, m, refs, verify=True, expect=B.ECORRUPT)
    assert want[1]["bad_blob"] == k
    _get(gpu, eng, pool, m, [refs[k]], cap=None, verify=True, expect=B.ECORRUPT)
    _get(gpu, eng, pool, m, refs)                                   # unverified: the bytes as held
    rest = refs[:k] + refs[k + 1:] + refs[:2] + [MISS[0]]
    want = _get(gpu, eng, pool, m, rest, verify=True)
    assert want[1]["verified"] == sum(n for j, (_, n, _) in enumerate(m.table) if j != k)


# ---- 6. arguments and states -------------------------------------------------------------------------
def test_arguments_and_states(gpu, eng, edges):
    pool, m = edges
    L = gpu.lib()
    src, off, lens = B.place([b"x" * 40, b"y" * 5])
    buf, out = _device(gpu, src), gpu.DeviceBuffer(1 << 16)
    oo, ll = gpu._u64(off), gpu._u64(lens)
    pinfo, ginfo = gpu.POOL_PUT_INFO(), gpu.PoolGetInfo()
    refs = np.frombuffer(m.table[1][2] + m.table[2][2], dtype=np.uint8).copy()
    out.from_host(np.full(out.nbytes, FILL, dtype=np.uint8))
    before = _raw(gpu, pool)

    def put(e=eng.h, p=pool.h, s=buf.ptr, o=oo, n=ll, count=2, f=0):
        op = None if o is None else gpu._p(gpu._u64(o), ctypes.c_uint64)
        np_ = None if n is None else gpu._p(gpu._u64(n), ctypes.c_uint64)
        return L.bsg_pool_put_blobs(e, p, s, op, np_, count, f, None, ctypes.byref(pinfo))

    def get(e=eng.h, p=pool.h, r=refs.ctypes.data, n=2, o=out.ptr, cap=1 << 16, f=0, info=ginfo):
        return L.bsg_pool_get(e, p, r, n, o, cap, f, None, None,
                              None if info is None else ctypes.byref(info))

    try:
        assert put(e=None) == put(p=None) == put(f=1) == B.EINVAL
        assert put(s=None) == put(o=None) == put(n=None) == put(count=1 << 32) == B.EINVAL
        assert put(s=buf.ptr + 8) == put(o=[0, 8]) == put(n=[40, 1 << 40]) == B.EINVAL
        assert put(o=[0, (1 << 64) - 16], n=[40, 32]) == B.EINVAL           # wraps
        assert put(o=[0, len(src) - 16], n=[40, 32]) == B.EINVAL            # no read slack
        assert put(s=pool.ptr) == B.EINVAL                                  # inside the pool
        assert get(e=None) == get(p=None) == get(info=None) == get(r=None) == B.EINVAL
        assert get(f=2) == get(n=1 << 32) == get(o=out.ptr + 8) == B.EINVAL
        assert get(o=None) == get(cap=0) == get(o=pool.ptr, cap=64) == B.EINVAL
        assert get(o=pool.ptr + pool.pool_bytes - 16, cap=64) == B.EINVAL
        if gpu.device_count() > 1:
            other = gpu.Engine(device=1)
            try:
                assert put(e=other.h) == get(e=other.h) == B.EINVAL
            finally:
                other.close()
        # an unfinished run; the run's records stay as they are through both calls
        run = gpu.DeviceBuffer(1 << 16)
        try:
            run.from_host(splitmix_array(5, 1 << 16))
            eng.run(run.ptr, [0], [1 << 16], bits=BITS, min_size=MN, fanout=FANOUT)
            assert put(f=1) == B.EINVAL and put() == B.ESTATE and get() == B.ESTATE
            eng.finish()
            recs = eng.chunks().tobytes()
            assert get() == B.OK and ginfo.found == 2 and put(count=0, s=None, o=None, n=None) == 0
            assert eng.chunks().tobytes() == recs and len(recs) > 0
        finally:
            run.free()
        got = out.to_host()
        n1, n2 = m.table[1][1], m.table[2][1]
        assert got[:n1].tobytes() == m.blob_bytes(1)
        assert got[P.align16(n1):P.align16(n1) + n2].tobytes() == m.blob_bytes(2)
        assert (got[P.align16(n1) + P.align16(n2):] == FILL).all()
        # a dead pool; EINVAL comes first
        dead = gpu.Pool(1 << 12, 4)
        try:
            assert L.bsg_pool_kill_debug(dead.h) == 0
            assert put(p=dead.h, f=1) == B.EINVAL and put(p=dead.h) == B.ESTATE
            assert get(p=dead.h, f=2) == B.EINVAL and get(p=dead.h) == B.ESTATE
            dead.reset()
            assert put(p=dead.h) == B.OK and pinfo.added == 2
        finally:
            dead.free()
        assert _raw(gpu, pool)[:3] == before[:3]
        assert L.bsg_pool_put_blobs(eng.h, pool.h, buf.ptr, gpu._p(oo, ctypes.c_uint64),
                                    gpu._p(ll, ctypes.c_uint64), 2, 0, None, None) == B.OK
        assert B.put_blobs(m, src, off, lens)[0] == B.OK
        _is(gpu, pool, m)
    finally:
        buf.free()
        out.free()


# ---- 7. two threads, their own engines, one pool -------------------------------------------------------
def test_two_threads_put_into_one_pool(gpu):
    blobs = [splitmix_array(300 + i, 1 + 37 * i) for i in range(60)]
    parts = [blobs[:40], blobs[20:]]                               # 20 shared, 20 each alone
    placed = [B.place(p) for p in parts]
    engs = [gpu.Engine(), gpu.Engine()]
    bufs = [_device(gpu, s) for s, _, _ in placed]
    pool = gpu.Pool(*CAP)
    got = [None, None]
    try:
        def job(t):
            def run():
                got[t] = pool.put_blobs(engs[t], bufs[t], placed[t][1], placed[t][2])
            return run
        _in_threads([job(0), job(1)])
        assert got[0][0] == got[1][0] == B.OK
        state, orders = _whole(gpu, pool), []
        for first in (0, 1):
            m = P.Model(*CAP)
            infos = {}
            for t in (first, 1 - first):
                rc, infos[t], _ = B.put_blobs(m, *placed[t])
            if [got[0][1], got[1][1]] == [infos[0], infos[1]]:
                _is(gpu, pool, m)
                orders.append(first)
        assert len(orders) == 1, (got[0][1], got[1][1])
        assert _whole(gpu, pool) == state
    finally:
        for e in engs:
            e.close()
        for b in bufs:
            b.free()
        pool.free()

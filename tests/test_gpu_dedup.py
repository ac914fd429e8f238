"""bsg_engine_dedup, bsg_refset and bsg_engine_pack_unique on the device, against the dict model
of dedup_cases.py over the oracle's records of the same bytes (the GPU records are held to those
first): first / uniq / pack_off / nunique / unique_bytes exactly, packed bytes exactly, guard
bytes around the packed output intact."""
import ctypes
import threading

import numpy as np
import pytest

import dedup_cases as DC
import layouts as L

pytestmark = pytest.mark.gpu

IN_SET = DC.IN_SET


def _run(gpu, eng, host, off, lens, bits, mn):
    buf = gpu.DeviceBuffer(host.size)
    buf.from_host(host)
    eng.run(buf.ptr, off, lens, bits=bits, min_size=mn)
    eng.finish()
    return buf


def _records(gpu, oracle, table, eng, streams, bits, mn):
    """The oracle's records, after holding the engine's to them."""
    want = DC.oracle_records(oracle, table, streams, bits, mn)
    got = eng.chunks()
    assert len(got) == len(want)
    for f in ("offset", "len", "stream", "ref"):
        assert (got[f] == want[f]).all(), f
    return want


def _check(eng, res, recs, seen=frozenset()):
    first, uniq, pack_off = res
    wf, wu, wp = DC.expected(recs, seen)
    assert first.tolist() == wf.tolist()
    assert uniq.tolist() == wu.tolist()
    assert pack_off.tolist() == wp.tolist()
    assert eng.nunique == len(wu) and eng.unique_bytes == int(wp[-1])
    return wu


def _pack(gpu, eng, streams, recs, uniq, guard=256):
    """pack_unique into the middle of a buffer poisoned 0xA5; the bytes and the guards."""
    n = eng.unique_bytes
    size = guard + ((n + 15) & ~15) + guard
    out = gpu.DeviceBuffer(size)
    try:
        out.from_host(np.full(size, 0xA5, dtype=np.uint8))
        eng.pack_unique(out, offset=guard, cap=n)
        got = out.to_host()
    finally:
        out.free()
    assert got[guard:guard + n].tobytes() == DC.packed(streams, recs, uniq)
    assert (got[:guard] == 0xA5).all() and (got[guard + n:] == 0xA5).all()


def _case(gpu, oracle, table, case, pack=True, funnel=0):
    streams, bits, mn = case
    host, off, lens = DC.place(streams)
    eng = gpu.Engine()
    try:
        # k_pack's other load variant (aligned loads and a byte funnel; measurement tooling)
        assert gpu.lib().bsg_engine_pack_mode_debug(eng.h, funnel) == 0
        buf = _run(gpu, eng, host, off, lens, bits, mn)
        recs = _records(gpu, oracle, table, eng, streams, bits, mn)
        uniq = _check(eng, eng.dedup(), recs)
        if pack:
            _pack(gpu, eng, streams, recs, uniq)
        buf.free()
        return recs, uniq
    finally:
        eng.close()


# ---- 1. edited copies --------------------------------------------------------------------------
def test_edited_copies(gpu, oracle, table):
    recs, uniq = _case(gpu, oracle, table, DC.edited_copies())
    assert len(uniq) < len(recs)


# ---- 2. aliased, shuffled and descending layouts ----------------------------------------------
@pytest.mark.parametrize("name", ["aliased", "shuffled", "descending"])
def test_layouts(gpu, oracle, table, name):
    layout = L.build(name)
    host = L.fill(layout, 0)
    off = [o for o, _, _ in layout[1]]
    lens = [n for _, n, _ in layout[1]]
    streams = [host[o:o + n] for o, n in zip(off, lens)]
    eng = gpu.Engine()
    try:
        buf = _run(gpu, eng, host, off, lens, 6, 64)
        recs = _records(gpu, oracle, table, eng, streams, 6, 64)
        first, uniq, pack_off = res = eng.dedup()
        wu = _check(eng, res, recs)
        if name == "aliased":  # the second stream on the same bytes: all duplicates of stream 9's
            s0, s1 = L.ALIAS_SAME
            i0 = int(np.flatnonzero(recs["stream"] == s0)[0])
            idx1 = np.flatnonzero(recs["stream"] == s1)
            assert first[idx1].tolist() == list(range(i0, i0 + len(idx1)))
            assert not set(idx1.tolist()) & set(uniq.tolist())
        _pack(gpu, eng, streams, recs, wu)
        buf.free()
    finally:
        eng.close()


# ---- 3. degenerate runs ------------------------------------------------------------------------
def test_no_streams_and_empty_streams(gpu):
    buf = gpu.DeviceBuffer(4096)
    out = gpu.DeviceBuffer(4096)
    eng = gpu.Engine()
    try:
        for off, lens in (([], []), ([0, 16, 16], [0, 0, 0])):
            eng.run(buf.ptr, off, lens, bits=6, min_size=64)
            assert eng.finish() == 0
            first, uniq, pack_off = eng.dedup()
            assert len(first) == 0 and len(uniq) == 0 and pack_off.tolist() == [0]
            assert eng.nunique == 0 and eng.unique_bytes == 0
            eng.pack_unique(out, cap=0)
    finally:
        eng.close()
        buf.free()
        out.free()


def test_one_chunk(gpu, oracle, table):
    from bs_amd.synth import splitmix_array
    recs, uniq = _case(gpu, oracle, table, ([splitmix_array(3, 777)], 33, 64))
    assert len(recs) == 1 and uniq.tolist() == [0]


def test_zeros(gpu, oracle, table):
    recs, uniq = _case(gpu, oracle, table, DC.zeros())
    assert len(recs) > 100 and len(uniq) <= 2


def test_one_chunk_streams(gpu, oracle, table):
    recs, uniq = _case(gpu, oracle, table, DC.one_chunk_streams())
    assert len(recs) == 3000 and len(uniq) == 2000


# ---- 4. planted collisions through bsg_refset_add ---------------------------------------------
def test_planted_collisions(gpu):
    refs = DC.planted_refs()
    want_first, want_new = DC.first_index([r.tobytes() for r in refs])
    rs = gpu.RefSet()
    try:
        added = rs.add(refs)
        want = np.zeros(len(refs), dtype=np.uint8)
        want[want_new] = 1
        assert added.tolist() == want.tolist()
        assert rs.count() == len(want_new)
        assert not rs.add(refs).any() and rs.count() == len(want_new)   # all known now
        # neighbours of the planted ones are still absent: the whole key is compared
        near = refs[[0, 64, 128, 128 + 4096]].copy()
        near[:, 20] ^= 1
        assert rs.add(near).tolist() == [1, 1, 1, 1]
        assert rs.count() == len(want_new) + 4
    finally:
        rs.free()


# ---- 5. growth ---------------------------------------------------------------------------------
def test_growth(gpu):
    p0, p1 = DC.doubling_points(2)
    refs = DC.random_refs(21, p1 + 64)
    rs = gpu.RefSet()
    try:
        have = 0
        for target in (p0 - 1, p0, p0 + 1, p1 - 1, p1, p1 + 1):
            assert rs.add(refs[have:target]).all()       # fresh refs: every one added
            have = target
            assert rs.count() == have
            sample = refs[np.linspace(0, have - 1, 97).astype(np.int64)]   # ends included
            assert not rs.add(sample).any() and rs.count() == have
        assert rs.add(refs[have:]).all()                 # (the refs not yet added were absent)
        have = len(refs)
        # a single call across several doublings, repeats inside it
        big = DC.random_refs(22, 10_000)
        both = np.concatenate([big, big[::-1]])
        added = rs.add(both)
        assert added[:10_000].all() and not added[10_000:].any()
        assert rs.count() == have + 10_000
        assert not rs.add(refs[:have]).any()
    finally:
        rs.free()


# ---- 6. a set and runs together ----------------------------------------------------------------
def test_set_and_runs(gpu, oracle, table):
    from bs_amd.synth import splitmix_array
    a = [splitmix_array(1, 90_000), splitmix_array(2, 50_001)]
    b = [a[1], splitmix_array(3, 40_000), a[0][:30_000]]   # shares content with run 1
    eng, rs = gpu.Engine(), gpu.RefSet()
    try:
        host, off, lens = DC.place(a)
        buf_a = _run(gpu, eng, host, off, lens, 7, 64)
        ra = _records(gpu, oracle, table, eng, a, 7, 64)
        plain = eng.dedup()
        again = eng.dedup()
        for x, y in zip(plain, again):      # set == NULL: identical arrays
            assert x.tobytes() == y.tobytes()
        half = DC.ref_list(ra)[::2]
        assert rs.add(half).sum() == len(set(half))
        seen = set(half)
        res = eng.dedup(rs)
        wu = _check(eng, res, ra, frozenset(seen))
        assert ((res[0] >> np.uint64(63)) == 1).tolist() == [r in seen for r in DC.ref_list(ra)]
        _pack(gpu, eng, a, ra, wu)
        seen |= set(DC.ref_list(ra))
        assert rs.count() == len(seen)
        res = eng.dedup(rs)                 # the same run, the same set: nothing is new
        assert eng.nunique == 0 and eng.unique_bytes == 0 and len(res[1]) == 0
        assert ((res[0] >> np.uint64(63)) == 1).all()

        host, off, lens = DC.place(b)
        buf_b = _run(gpu, eng, host, off, lens, 7, 64)
        rb = _records(gpu, oracle, table, eng, b, 7, 64)
        res = eng.dedup(rs)
        wu = _check(eng, res, rb, frozenset(seen))
        assert 0 < len(wu) < len(rb)
        assert set(DC.ref_list(rb[wu.astype(np.int64)])).isdisjoint(seen)
        _pack(gpu, eng, b, rb, wu)
        seen |= set(DC.ref_list(rb))
        assert rs.count() == len(seen)
        buf_a.free()
        buf_b.free()
    finally:
        eng.close()
        rs.free()


# ---- 7. state and arguments --------------------------------------------------------------------
def test_states_and_arguments(gpu, oracle, table):
    from bs_amd.synth import splitmix_array
    Lb = gpu.lib()
    nu, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
    streams = [splitmix_array(8, 70_000), splitmix_array(9, 5_000), splitmix_array(8, 70_000)]
    host, off, lens = DC.place(streams)
    eng, fresh = gpu.Engine(), gpu.Engine()
    out = gpu.DeviceBuffer(host.size + 64)
    try:
        def dedup_rc():
            return Lb.bsg_engine_dedup(eng.h, None, ctypes.byref(nu), ctypes.byref(nb))
        assert dedup_rc() == -71                                        # no run yet
        assert Lb.bsg_engine_dedup(eng.h, None, None, ctypes.byref(nb)) == -22
        assert Lb.bsg_engine_dedup(eng.h, None, ctypes.byref(nu), None) == -22
        assert Lb.bsg_engine_pack_unique(eng.h, out.ptr, out.nbytes) == -71
        assert Lb.bsg_engine_dedup_first_device(eng.h) is None
        buf = gpu.DeviceBuffer(host.size)
        buf.from_host(host)
        eng.hash(buf.ptr, off, lens)
        eng.finish()
        assert dedup_rc() == -71                                        # a hash run
        eng.run(buf.ptr, off, lens, bits=6, min_size=64, fanout=2)
        assert dedup_rc() == -71                                        # run without finish
        eng.finish()
        assert Lb.bsg_engine_pack_unique(eng.h, out.ptr, out.nbytes) == -71   # before dedup
        assert Lb.bsg_engine_copy_dedup(eng.h, None, 0, None, None, 0) == -71
        recs = _records(gpu, oracle, table, eng, streams, 6, 64)
        res = eng.dedup()
        wu = _check(eng, res, recs)
        assert Lb.bsg_engine_dedup_first_device(eng.h) and Lb.bsg_engine_dedup_uniq_device(eng.h)
        assert Lb.bsg_engine_dedup_pack_off_device(eng.h)
        n = eng.unique_bytes
        assert Lb.bsg_engine_pack_unique(eng.h, None, n) == -22
        assert Lb.bsg_engine_pack_unique(eng.h, out.ptr + 8, n) == -22
        assert Lb.bsg_engine_pack_unique(eng.h, out.ptr, n - 1) == -22
        assert Lb.bsg_engine_pack_unique(eng.h, buf.ptr + 4096, n) == -22   # inside the input
        assert Lb.bsg_engine_pack_unique(eng.h, out.ptr, n) == 0
        assert out.to_host(0, n).tobytes() == DC.packed(streams, recs, wu)
        # caps below the totals: no more than asked is written
        f = np.full(len(recs), 7, dtype=np.uint64)
        u = np.full(len(wu), 7, dtype=np.uint64)
        p = np.full(len(wu) + 1, 7, dtype=np.uint64)
        assert Lb.bsg_engine_copy_dedup(eng.h, f.ctypes.data, 5, u.ctypes.data, p.ctypes.data, 3) == 0
        assert f[:5].tolist() == res[0][:5].tolist() and (f[5:] == 7).all()
        assert u[:3].tolist() == res[1][:3].tolist() and (u[3:] == 7).all()
        assert p[:4].tolist() == res[2][:4].tolist() and (p[4:] == 7).all()

        # dedup, then trees, then chunks: Roots and records as a fresh engine's
        roots = eng.trees()[0]
        fresh.run(buf.ptr, off, lens, bits=6, min_size=64, fanout=2)
        fresh.finish()
        assert roots.tobytes() == fresh.trees()[0].tobytes()
        assert eng.chunks().tobytes() == fresh.chunks().tobytes()
        for x, y in zip(eng.dedup(), res):     # and dedup after trees: the same again
            assert x.tobytes() == y.tobytes()
        # a new run drops the result
        eng.run(buf.ptr, off, lens, bits=6, min_size=64)
        assert Lb.bsg_engine_dedup_first_device(eng.h) is None
        eng.finish()
        assert Lb.bsg_engine_pack_unique(eng.h, out.ptr, out.nbytes) == -71
        buf.free()
    finally:
        eng.close()
        fresh.close()
        out.free()


# ---- 8. pack, every residue --------------------------------------------------------------------
@pytest.mark.parametrize("funnel", [0, 1])
def test_pack_residues(gpu, oracle, table, funnel):
    recs, uniq = _case(gpu, oracle, table, DC.residues(), funnel=funnel)
    assert len(uniq) > 4000


@pytest.mark.parametrize("funnel", [0, 1])
def test_pack_tiny_chunks(gpu, oracle, table, funnel):
    recs, uniq = _case(gpu, oracle, table, DC.tiny_chunks(), funnel=funnel)
    assert (recs["len"] == 1).any() and len(uniq) < len(recs)


# ---- 9. pack, long segments --------------------------------------------------------------------
def test_pack_long_segment(gpu, oracle, table):
    recs, uniq = _case(gpu, oracle, table, DC.long_segment())
    assert len(recs) == 1 and int(recs["len"][0]) > DC.constants()["kPackTile"]


def test_pack_long_among_short(gpu, oracle, table):
    recs, uniq = _case(gpu, oracle, table, DC.long_among_short())
    assert len(uniq) == 4001


# ---- 10. two engines, one set, two threads -----------------------------------------------------
def test_two_engines_one_set(gpu, oracle, table):
    groups, bits, mn = DC.shared_halves()
    want = [DC.oracle_records(oracle, table, g, bits, mn) for g in groups]
    rs = gpu.RefSet()
    results, errors = [None, None], []

    def work(t):
        try:
            host, off, lens = DC.place(groups[t])
            eng = gpu.Engine()
            try:
                buf = _run(gpu, eng, host, off, lens, bits, mn)
                recs = _records(gpu, oracle, table, eng, groups[t], bits, mn)
                first, uniq, _ = eng.dedup(rs)
                results[t] = [recs["ref"][int(i)].tobytes() for i in uniq]
                buf.free()
            finally:
                eng.close()
        except Exception as e:  # noqa: BLE001 (reported by the main thread)
            errors.append(e)

    try:
        threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        distinct = set(DC.ref_list(want[0])) | set(DC.ref_list(want[1]))
        new = results[0] + results[1]
        assert len(new) == len(set(new)) and set(new) == distinct   # each new exactly once
        assert rs.count() == len(distinct)
    finally:
        rs.free()

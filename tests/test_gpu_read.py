"""bsg_engine_read and bsg_pool_read on the device against the model of read_cases.py, every
comparison an equality and the output compared over its whole allocation: ranges that start and end
at and around every kind of boundary, every source residue in a tight pool, many ranges in one
call, pruning made visible by pools that lack what a range does not need, verification of the
touched blobs alone, every layout rule, the states, and two threads on one pool."""
import ctypes
import threading

import numpy as np
import pytest

import pool_cases as P
import read_cases as R
import walk_cases as W
from bs_amd.synth import splitmix_array
from test_gpu_pool_collect import BITS, CAP, FANOUT, MN, _put, _start, _streams

pytestmark = pytest.mark.gpu
FILL, GUARD = W.FILL, W.GUARD


class Host:
    """A pool in device memory with its table on the host (bsg_engine_read's form)."""

    def __init__(self, gpu, pool, blobs):
        self.pool, self.blobs, self.pool_bytes = pool, blobs, len(pool)
        self.buf = gpu.DeviceBuffer(len(pool))
        self.buf.from_host(pool)
        self.blob_bytes = W.getter(pool, blobs)

    def free(self):
        self.buf.free()


class Lying:
    """A bsg_pool with its model."""

    def __init__(self, pool, m):
        self.pool, self.blobs, self.pool_bytes = pool, m.blobs(), m.stat()["pool_bytes"]
        self.blob_bytes = m.blob_bytes


@pytest.fixture(scope="module")
def base(gpu):
    """Two runs of three streams put into one bsg_pool, once for the module: the pool, the same
    pool as a host-table pool (aligned, with read slack) and as a tight one (every blob after the
    other from byte 1 on), the Roots and the streams. No test writes any of them."""
    class B:
        pass
    b, eng = B(), gpu.Engine()
    src, m = gpu.Pool(*CAP), P.Model(*CAP)
    b.roots, b.streams, b.hosts = [], [], []
    try:
        for second in (False, True):
            streams = _streams(second)
            buf, run, roots = _start(gpu, eng, streams)
            try:
                _put(eng, src, m, run)
            finally:
                buf.free()
            b.roots += roots
            b.streams += [bytes(d) for d in streams]
        b.lying = Lying(src, m)
        b.m = m
        b.aligned_pool = np.concatenate([m.buf, np.zeros(256, np.uint8)])
        b.aligned = Host(gpu, b.aligned_pool, m.blobs())
        tight, tb = W.pool_of({r: m.blob_bytes(k) for k, (_, _, r) in enumerate(m.table)})
        b.tight = Host(gpu, np.concatenate([tight, np.zeros(256, np.uint8)]), tb)
        b.hosts = [b.aligned, b.tight]
        b.index = {r: k for k, (_, _, r) in enumerate(m.table)}
        b.nodes = [k for k in range(len(m.table)) if W.parse_node(m.blob_bytes(k)) is not None]
        b.cuts = [R.boundaries(m.blob_bytes, b.lying.blobs, r) for r in b.roots]
        assert all(c[3] == len(d) for c, d in zip(b.cuts, b.streams))
        yield b
    finally:
        eng.close()
        src.free()
        for h in b.hosts:
            h.free()


@pytest.fixture()
def eng(gpu):
    e = gpu.Engine()
    yield e
    e.close()


def _layout(ranges, want):
    """out_off and out_cap: room for a range's len (below 2^63) and for what the model says it
    gets, 16-aligned with a gap."""
    off, o = [], 16
    for (_, _, n), g in zip(ranges, want[2]):
        off.append(o)
        o += (max(g, n if n < 1 << 63 else 0) + 15 & ~15) + 32
    return off, o


def _call(gpu, eng, t, ranges, off, cap, flags=0):
    """One read into a FILL-ed buffer with GUARD bytes at both ends: (rc, status, got, info, the
    whole buffer)."""
    obuf = gpu.DeviceBuffer(GUARD + cap + GUARD)
    try:
        obuf.from_host(np.full(obuf.nbytes, FILL, dtype=np.uint8))
        if isinstance(t, Lying):
            res = t.pool.read(eng, ranges, obuf.ptr + GUARD, off, flags=flags, out_cap=cap)
        else:
            res = eng.read(t.buf.ptr, t.blobs, ranges, obuf.ptr + GUARD, off, flags=flags,
                           pool_bytes=t.pool_bytes, out_cap=cap)
        return res + (obuf.to_host(),)
    finally:
        obuf.free()


def _held(gpu, eng, t, ranges, flags=0, expect=R.OK, blobs=None):
    """One read on the device and in the model: the return code, every range's status and byte
    count, the info and every byte of the output's allocation. Returns the model's tuple."""
    if blobs is not None:
        t = _view(t, blobs)
    off, cap = _layout(ranges, R.model(t.blob_bytes, t.blobs, ranges, t.pool_bytes, flags=flags))
    want = R.model(t.blob_bytes, t.blobs, ranges, t.pool_bytes, off, cap, flags)
    assert want[0] == expect, (want[0], expect, want[3])
    rc, status, got, info, out = _call(gpu, eng, t, ranges, off, cap, flags)
    assert rc == want[0], (rc, want[0], info, want[3])
    assert info == want[3], (info, want[3])
    assert got.tolist() == want[2]
    if want[1] is not None:
        assert status.tolist() == want[1].tolist()
    exp = np.full(GUARD + cap + GUARD, FILL, dtype=np.uint8)
    if rc == R.OK:
        for o, d in zip(off, want[4]):
            exp[GUARD + o:GUARD + o + len(d)] = np.frombuffer(d, dtype=np.uint8)
    assert out.tobytes() == exp.tobytes()
    return want


def _view(t, blobs):
    """Host pool t under another table (its bytes on the device are shared)."""
    v = Host.__new__(Host)
    v.pool, v.blobs, v.pool_bytes, v.buf = t.pool, blobs, t.pool_bytes, t.buf
    v.blob_bytes = W.getter(t.pool, blobs)
    return v


def _edited(gpu, t, edits, blobs=None):
    """A new host pool: t's bytes with {position: byte values} written over them."""
    pool = t.pool.copy()
    for at, b in edits.items():
        pool[at:at + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
    return Host(gpu, pool, t.blobs if blobs is None else blobs)


# ---- 1. edge ranges ------------------------------------------------------------------------------
def _points(cuts):
    chunks, leaf_nodes, top, size = cuts
    mid = [chunks[len(chunks) // 3], leaf_nodes[len(leaf_nodes) // 2], top[1]]
    assert len(set(mid)) == 3 and all(0 < x < size for x in mid)
    pts = {x + d for x in mid for d in (-1, 0, 1)} | {0, size - 1, size, size + 1}
    return sorted(pts)


@pytest.mark.parametrize("form", ("lying", "aligned"))
def test_edge_ranges(gpu, eng, base, form):
    t = getattr(base, form)
    root, cuts = base.roots[0], base.cuts[0]
    size, pts = cuts[3], _points(cuts)
    ranges = [(root, a, b - a) for a in pts for b in pts if a <= b]
    inside = cuts[0][5] + 3  # a range inside one chunk
    assert cuts[0][6] - cuts[0][5] > 8
    ranges += [(root, inside, 0), (root, inside, 1), (root, inside, 4), (root, 0, size),
               (root, size - 1, R.U64), (root, size, R.U64), (root, size + 1, 7),
               (root, R.U64, 1), (root, R.U64, R.U64), (root, size - 3, R.U64 - 5),
               (root, 5, R.U64 - 4), (bytes(32), 0, 100), (bytes(32), 7, 0)]
    want = _held(gpu, eng, t, ranges)
    assert want[2][-2:] == [0, 0] and want[2][-3] == size - 5
    for (r, a, n), d in zip(ranges, want[4]):
        assert d == (base.streams[0][a:a + n] if r == root else b"")


def test_whole_streams_are_restore_walk(gpu, eng, base):
    """Every stream whole: the bytes bsg_pool_restore_walk writes, and the walk's counts."""
    ranges = [(r, 0, len(d)) for r, d in zip(base.roots, base.streams)]
    want = _held(gpu, eng, base.lying, ranges, flags=R.VERIFY)
    rc, winfo, status = eng.pool_walk(base.lying.pool, W.roots_array(base.roots))
    assert rc == W.OK
    assert (want[3]["nnodes"], want[3]["nleaves"], want[3]["depth"]) == \
        (winfo["nnodes"], winfo["nrecs"], winfo["depth"])
    off, cap = _layout(ranges, want)
    obuf = gpu.DeviceBuffer(GUARD + cap + GUARD)
    try:
        obuf.from_host(np.full(obuf.nbytes, FILL, dtype=np.uint8))
        rc, info = eng.pool_restore_walk(base.lying.pool, obuf.ptr + GUARD, off, out_cap=cap)
        walked = obuf.to_host()
    finally:
        obuf.free()
    assert rc == W.OK
    _, _, _, _, out = _call(gpu, eng, base.lying, ranges, off, cap)
    assert out.tobytes() == walked.tobytes()


# ---- 2. alignment --------------------------------------------------------------------------------
def test_every_source_residue(gpu, eng, base):
    """All 16 values of offset mod 16 against chunks that start at differing residues in the tight
    pool, with lens that end in every residue too."""
    t, root, chunks = base.tight, base.roots[0], base.cuts[0][0]
    raw = np.ascontiguousarray(t.blobs["ref"]).tobytes()
    where = {raw[32 * k:32 * k + 32]: int(t.blobs[k]["off"]) for k in range(len(t.blobs))}
    data, picked, seen = base.streams[0], [], set()
    for c0, c1 in zip(chunks, chunks[1:]):
        res = where[W.sha(data[c0:c1])] % 16
        if res not in seen and c0 > 0:
            seen.add(res)
            picked.append(c0)
        if len(picked) == 6:
            break
    assert len(picked) == 6
    ranges = [(root, c0 - 8 + d, 3000 + 7 * d + j) for j, c0 in enumerate(picked)
              for d in range(16)]
    assert {a % 16 for _, a, _ in ranges} == set(range(16))
    want = _held(gpu, eng, t, ranges)
    for (_, a, n), d in zip(ranges, want[4]):
        assert d == data[a:a + n]


# ---- 3. many ranges ------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("lying", "tight"))
def test_many_ranges_of_many_streams(gpu, eng, base, form):
    rng = np.random.default_rng(12)
    ranges = []
    for i in range(240):  # the streams interleaved, every Root many times, a zero Root among them
        s = i % 7
        if s == 6:
            ranges.append((bytes(32), int(rng.integers(0, 50)), int(rng.integers(0, 50))))
            continue
        size = len(base.streams[s])
        a = int(rng.integers(0, size + 20))
        ranges.append((base.roots[s], a, int(rng.integers(0, 20_000))))
    ranges += [ranges[3]] * 3
    want = _held(gpu, eng, getattr(base, form), ranges)
    for (r, a, n), d in zip(ranges, want[4]):
        if r != bytes(32):
            assert d == base.streams[base.roots.index(r)][a:a + n]


# ---- 4. pruning, observable ----------------------------------------------------------------------
def test_what_a_range_does_not_need_may_be_missing(gpu, eng, base):
    t, root = base.aligned, base.roots[0]
    chunks, leaf_nodes, top, size = base.cuts[0]
    data = base.streams[0]
    # a chunk, and a whole leaf-node subtree, far from the window
    gone_chunk = base.index[W.sha(data[chunks[40]:chunks[41]])]
    ln = next(k for k in base.nodes
              if (nd := W.parse_node(base.m.blob_bytes(k)))[0] == 2 and nd[2] == leaf_nodes[30])
    kids = W.parse_node(base.m.blob_bytes(ln))[1]
    subtree = [ln] + [base.index[r] for r, _ in kids]
    sub_end = leaf_nodes[31]
    window = (root, top[1] + 11, 9000)
    assert chunks[41] < window[1] and sub_end < window[1]
    full = _held(gpu, eng, t, [window])
    for gone in ([gone_chunk], subtree):
        few = np.delete(t.blobs, gone)
        want = _held(gpu, eng, t, [window], blobs=few)
        assert (want[2], want[3], want[4]) == (full[2], full[3], full[4])
    # the same blobs under the window: not found, the right range named, nothing written
    for gone, at in (([gone_chunk], chunks[40]), (subtree, leaf_nodes[30]), (subtree, sub_end - 1)):
        few = np.delete(t.blobs, gone)
        ranges = [window, (root, at, 1), (root, 0, 10)]
        want = _held(gpu, eng, t, ranges, expect=R.ENOTFOUND, blobs=few)
        assert want[1].tolist() == [R.OK, R.ENOTFOUND, R.OK] and want[3]["bad_range"] == 1
    # the byte before the subtree and the byte after it do not need it
    few = np.delete(t.blobs, subtree)
    _held(gpu, eng, t, [(root, leaf_nodes[30] - 1, 1), (root, sub_end, 1)], blobs=few)


def test_garbage_beside_the_path_and_on_it(gpu, eng, base):
    t, root = base.aligned, base.roots[0]
    window = (root, base.cuts[0][2][1] + 5, 5000)
    full = R.model(t.blob_bytes, t.blobs, [window], t.pool_bytes)
    on = [k for k in base.nodes if k in full[5]]
    beside = [k for k in base.nodes if k not in full[5]]
    assert len(on) >= 3 and len(beside) > 10
    junk = lambda k: {int(t.blobs[k]["off"]): b"\xff" * int(t.blobs[k]["len"])}  # noqa: E731
    e = {}
    for k in beside:
        e.update(junk(k))
    h = _edited(gpu, t, e)
    try:
        want = _held(gpu, eng, h, [window])
        assert (want[2], want[3], want[4]) == (full[2], full[3], full[4])
    finally:
        h.free()
    for k in (on[0], on[len(on) // 2], on[-1]):
        h = _edited(gpu, t, junk(k))
        try:
            want = _held(gpu, eng, h, [(root, 0, 1), window], expect=R.ECORRUPT)
            assert want[1][1] == R.ECORRUPT and want[3]["bad_range"] in (0, 1)
        finally:
            h.free()


# ---- 5. verify -----------------------------------------------------------------------------------
def test_verify_hashes_what_the_read_touches(gpu, eng, base):
    t, root = base.aligned, base.roots[3]
    chunks, leaf_nodes, top, size = base.cuts[3]
    window = (root, top[0] + 100, 7000)  # inside the Root's first child
    assert window[1] + window[2] < top[1]
    full = _held(gpu, eng, t, [window], flags=R.VERIFY)
    touched = full[5]
    assert 0 < full[3]["verified"] == sum(int(t.blobs[k]["len"]) for k in touched)
    assert full[3]["verified"] * 20 < int(t.blobs["len"].sum())
    _held(gpu, eng, base.lying, [window], flags=R.VERIFY)
    flip = lambda at: {at: bytes([int(t.pool[at]) ^ 0x10])}  # noqa: E731
    # an untouched blob: not seen
    far = next(k for k in range(len(t.blobs)) if k not in touched and k not in base.nodes)
    h = _edited(gpu, t, flip(int(t.blobs[far]["off"]) + 1))
    try:
        want = _held(gpu, eng, h, [window], flags=R.VERIFY)
        assert (want[2], want[3], want[4]) == (full[2], full[3], full[4])
    finally:
        h.free()
    # a touched leaf
    leaf = max(k for k in touched if k not in base.nodes)
    h = _edited(gpu, t, flip(int(t.blobs[leaf]["off"]) + int(t.blobs[leaf]["len"]) - 1))
    try:
        want = _held(gpu, eng, h, [window], flags=R.VERIFY, expect=R.ECORRUPT)
        assert want[3]["bad_blob"] == leaf and want[3]["verified"] == full[3]["verified"]
        _held(gpu, eng, h, [window])  # (without the flag the bytes are trusted)
    finally:
        h.free()
    # the Root: one byte of the ref of a child the window does not follow. The node still parses
    # and the walk never looks the ref up, so only the hash catches it.
    rk = base.index[root]
    kind, kids, _, _ = W.parse_node(t.blob_bytes(rk))
    assert kind == 1 and len(kids) >= 2
    at = int(t.blobs[rk]["off"]) + t.blob_bytes(rk).index(kids[-1][0]) + 9
    h = _edited(gpu, t, flip(at))
    try:
        assert W.parse_node(h.blob_bytes(rk)) is not None
        want = _held(gpu, eng, h, [window], flags=R.VERIFY, expect=R.ECORRUPT)
        assert want[3]["bad_blob"] == rk
        plain = _held(gpu, eng, h, [window])
        assert plain[4] == full[4]
    finally:
        h.free()
    # a misaligned touched blob: the flag alone minds
    _held(gpu, eng, base.tight, [window], flags=R.VERIFY, expect=R.EINVAL)
    _held(gpu, eng, base.tight, [window])


# ---- 6. errors and states ------------------------------------------------------------------------
def test_layout_rules(gpu, eng, base):
    L, t = gpu.lib(), base.aligned
    root, size = base.roots[1], len(base.streams[1])
    rg = gpu.read_ranges([(root, 10, 100), (root, 50, 100)])
    oo = np.array([0, 112], dtype=np.uint64)
    st, got, info = np.zeros(2, np.int32), np.zeros(2, np.uint64), gpu.ReadInfo()
    obuf = gpu.DeviceBuffer(GUARD + 4096 + GUARD)
    try:
        obuf.from_host(np.full(obuf.nbytes, FILL, dtype=np.uint8))
        out = obuf.ptr + GUARD

        def call(e=eng.h, pool=t.buf.ptr, pb=t.pool_bytes, bl=t.blobs.ctypes.data,
                 nb=len(t.blobs), r=rg.ctypes.data, n=2, o=out, cap=4096, off=oo.ctypes.data, f=0):
            got[:] = 77
            rc = L.bsg_engine_read(e, pool, pb, bl, nb, r, n, o, cap, off, f, st.ctypes.data,
                                   got.ctypes.data, ctypes.byref(info))
            # (beyond 65,535 ranges the arrays' lengths are not known to be nranges)
            assert rc == R.OK or n > 2 or (got.tolist() == [0, 0] and info.bytes == 0), (rc, got)
            return rc

        assert call() == R.OK and got.tolist() == [100, 100]
        for kw in (dict(e=None), dict(pool=None), dict(bl=None), dict(r=None), dict(off=None),
                   dict(o=None), dict(n=65536), dict(f=2), dict(f=3), dict(o=out + 8),
                   dict(cap=211), dict(pb=int(t.blobs["off"].max()) + 1)):
            assert call(**kw) == R.EINVAL, kw
        for bad in ([8, 112], [0, 104], [0, 4000], [0, 4112], [0, 96], [16, 0]):
            oo[:] = bad
            assert call() == R.EINVAL, bad
        oo[:] = [0, 112]
        # a len of 2^63 and more is held to the stream's size, once it is known
        big = gpu.read_ranges([(root, size - 40, 1 << 63), (root, size - 9, R.U64)])
        assert call(r=big.ctypes.data, cap=112 + 9) == R.OK and got.tolist() == [40, 9]
        obuf.from_host(np.full(obuf.nbytes, FILL, dtype=np.uint8))
        assert call(r=big.ctypes.data, cap=112 + 8) == R.EINVAL
        oo[:] = [0, 32]
        assert call(r=big.ctypes.data) == R.EINVAL                        # 40 bytes at 0 reach 32
        oo[:] = [0, 112]
        # the output inside the pool
        inside = (t.buf.ptr + 4096 + 15) & ~15
        assert call(o=inside) == R.EINVAL
        assert L.bsg_pool_read(eng.h, base.lying.pool.h, rg.ctypes.data, 2, base.lying.pool.ptr,
                               4096, oo.ctypes.data, 0, None, None, None) == R.EINVAL
        assert L.bsg_pool_read(eng.h, None, rg.ctypes.data, 2, out, 4096, oo.ctypes.data, 0, None,
                               None, None) == R.EINVAL
        assert L.bsg_pool_read(None, base.lying.pool.h, rg.ctypes.data, 2, out, 4096,
                               oo.ctypes.data, 0, None, None, None) == R.EINVAL
        # nothing to read is no fault, and the optional pointers are optional
        assert call(n=0, r=None, off=None) == R.OK
        assert L.bsg_engine_read(eng.h, t.buf.ptr, t.pool_bytes, t.blobs.ctypes.data,
                                 len(t.blobs), rg.ctypes.data, 2, out, 4096, oo.ctypes.data, 0,
                                 None, None, None) == R.OK
        assert (obuf.to_host(0, GUARD) == FILL).all()
        assert (obuf.to_host(GUARD + 4096, GUARD) == FILL).all()
    finally:
        obuf.free()


def test_states(gpu, eng, base):
    L, t = gpu.lib(), base.aligned
    root = base.roots[2]
    window = [(root, 1000, 3000)]
    # a dead pool, and a pool on another device, come before everything but a null handle
    small = gpu.Pool(1 << 12, 4)
    try:
        rc, status, got, info, out = _call(gpu, eng, Lying(small, P.Model(1 << 12, 4)), window,
                                           [0], 3008)
        assert rc == R.ENOTFOUND and status.tolist() == [R.ENOTFOUND]
        assert L.bsg_pool_kill_debug(small.h) == R.OK
        rc, status, got, info, out = _call(gpu, eng, Lying(small, P.Model(1 << 12, 4)), window,
                                           [0], 3008, flags=2)
        assert rc == R.ESTATE and info == R.fresh_info() and (out == FILL).all()
        small.reset()
    finally:
        small.free()
    if gpu.device_count() > 1:
        other = gpu.Pool(1 << 12, 4, device=1)
        try:
            rc, *_ = _call(gpu, eng, Lying(other, P.Model(1 << 12, 4)), window, [0], 3008)
            assert rc == R.EINVAL
        finally:
            other.free()
    # an unfinished run: ranked after every verdict, and nothing is written
    h = _edited(gpu, t, {int(t.blobs[base.index[root]]["off"]): b"\xff"})
    buf = gpu.DeviceBuffer(1 << 16)
    try:
        buf.from_host(splitmix_array(5, 1 << 16))
        eng.run(buf.ptr, [0], [1 << 16], bits=BITS, min_size=MN, fanout=FANOUT)
        _held(gpu, eng, h, window, expect=R.ECORRUPT)
        _held(gpu, eng, t, [(b"\x01" * 32, 0, 5)], expect=R.ENOTFOUND)
        for flags in (0, R.VERIFY):
            rc, status, got, info, out = _call(gpu, eng, t, window, [0], 3008, flags)
            assert rc == R.ESTATE and got.tolist() == [0] and info["bytes"] == 0
            assert status.tolist() == [R.OK] and (out == FILL).all()
        eng.finish()
        _held(gpu, eng, t, window)
    finally:
        buf.free()
        h.free()


def test_earlier_results_stay(gpu, eng, base):
    """The engine's run, dedup result, tree, walk and gc results are what they were after reads
    with and without the flag, failed ones among them."""
    t = base.aligned
    buf, run, roots = _start(gpu, eng, _streams())
    try:
        first, uniq, pack_off = eng.dedup()
        rc, winfo, _ = eng.walk(t.buf.ptr, t.blobs, W.roots_array(base.roots[:3]),
                                pool_bytes=t.pool_bytes)
        assert rc == W.OK
        rc, ginfo, _ = eng.gc_mark(t.buf.ptr, t.blobs, W.roots_array(base.roots[:3]),
                                   pool_bytes=t.pool_bytes)
        assert rc == W.OK

        def state():
            recs, sizes, counts = eng.copy_walk()
            live, table = eng.copy_gc(align16=True)
            L = gpu.lib()
            f2 = np.zeros(len(first), np.uint64)
            assert L.bsg_engine_copy_dedup(eng.h, f2.ctypes.data, len(f2), None, None, 0) == 0
            return (eng.chunks().tobytes(), recs.tobytes(), sizes.tolist(), counts.tolist(),
                    live.tobytes(), table.tobytes(), f2.tobytes(), eng.walk_records_device(),
                    eng.gc_live_device(), L.bsg_engine_roots_device(eng.h))

        before = state()
        assert before[6] == first.tobytes() and before[9]
        _held(gpu, eng, t, [(base.roots[4], 5, 70_000)], flags=R.VERIFY)
        _held(gpu, eng, base.lying, [(base.roots[0], 100_000, 64)])
        _held(gpu, eng, t, [(b"\x02" * 32, 0, 5)], expect=R.ENOTFOUND)
        assert state() == before
    finally:
        buf.free()


# ---- 7. threads ----------------------------------------------------------------------------------
def test_two_threads_read_one_pool(gpu, base):
    engs = [gpu.Engine(), gpu.Engine()]
    rng = np.random.default_rng(3)
    jobs = []
    for i in range(2):
        ranges = [(base.roots[(i + j) % 6], int(rng.integers(0, 100_000)),
                   int(rng.integers(1, 40_000))) for j in range(12)]
        jobs.append((ranges, R.model(base.lying.blob_bytes, base.lying.blobs, ranges,
                                     base.lying.pool_bytes, flags=i)))
    errs = []

    def work(i):
        try:
            ranges, want = jobs[i]
            off, cap = _layout(ranges, want)
            for _ in range(4):
                rc, status, got, info, out = _call(gpu, engs[i], base.lying, ranges, off, cap, i)
                assert rc == R.OK and info == want[3] and got.tolist() == want[2]
                for o, d in zip(off, want[4]):
                    assert out[GUARD + o:GUARD + o + len(d)].tobytes() == d
        except BaseException as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    try:
        for x in th:
            x.start()
        for x in th:
            x.join(120)
        assert not any(x.is_alive() for x in th), "deadlock"
        assert not errs, errs
    finally:
        for e in engs:
            e.close()

"""bsg_engine_gc_mark's and bsg_engine_gc_compact's refusals on the device against the model of
gc_cases.py: what the pool lacks, nodes that break their form, which blob is blamed, the order of
the return codes, a failed mark after a good one, and every argument check."""
import ctypes

import numpy as np
import pytest

import gc_cases as G
import walk_cases as W
from bs_amd.bsgpu import GC_MISSING_LEAVES

pytestmark = pytest.mark.gpu


@pytest.fixture()
def eng(gpu):
    e = gpu.Engine()
    yield e
    e.close()


def _without(store, ref):
    return {r: b for r, b in store.items() if r != ref}


# ---- misses --------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, GC_MISSING_LEAVES])
def test_missing_root_nodes_child_and_leaves_child(gpu, eng, flags):
    trees, store = W.two_streams()
    roots = [t.root for t in trees]
    index = lambda blobs, ref: G.index_of(blobs)[ref]  # noqa: E731
    # a Root the pool lacks: its status alone, no blob to blame
    pool, blobs = W.pool_of(store)
    want = G.check_host_pool(gpu, eng, pool, blobs, roots + [W.sha(b"no such root")],
                             G.ENOTFOUND, flags=flags)
    assert want[1].tolist() == [0, 0, G.ENOTFOUND] and want[2]["bad_blob"] == G.NONE
    assert want[2]["bad_root"] == 2
    # a `nodes` child: the parent is blamed, with or without the flag
    gone = trees[1].nodes[2][3]
    pool, blobs = W.pool_of(_without(store, gone["ref"]))
    want = G.check_host_pool(gpu, eng, pool, blobs, roots, G.ENOTFOUND, flags=flags)
    assert want[2]["bad_blob"] == index(blobs, trees[1].nodes[1][1]["ref"])
    assert want[1].tolist() == [0, 0]
    # `leaves` children: two distinct refs, one of them named by two nodes
    a, b = trees[0].nodes[2][0]["kids"][1][0], trees[1].nodes[2][8]["kids"][2][0]
    less = _without(_without(store, a), b)
    extra = G.node(leaves=[(a, 0), (trees[0].nodes[2][0]["kids"][0][0], 9)], size=20)
    less[W.sha(extra)] = extra
    pool, blobs = W.pool_of(less)
    want = G.check_host_pool(gpu, eng, pool, blobs, roots + [W.sha(extra)],
                             G.OK if flags else G.ENOTFOUND, flags=flags)
    if flags:
        assert want[2]["missing_leaves"] == 2 and want[2]["ndead"] == 0
    else:
        assert want[2]["bad_blob"] == min(index(blobs, trees[0].nodes[2][0]["ref"]),
                                          index(blobs, trees[1].nodes[2][8]["ref"]),
                                          index(blobs, W.sha(extra)))


# ---- form faults ---------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["root", "middle", "leaf"])
@pytest.mark.parametrize("name", ["padded", "both_kinds", "size0", "descending", "flip_marker"])
def test_form_faults(gpu, eng, name, where):
    pool, blobs, roots, want_rc = W.mutated(name, where, 1)
    want = G.check_host_pool(gpu, eng, pool, blobs, roots, want_rc)
    d, i = W.WHERE[where]
    assert want[2]["bad_blob"] == G.index_of(blobs)[W.two_streams()[0][1].nodes[d][i]["ref"]]
    assert want[1].tolist() == [0, G.ECORRUPT if where == "root" else 0]


@pytest.mark.parametrize("name,where", [("own_offset", "root"), ("own_size", "middle"),
                                        ("own_offset", "leaf")])
def test_cover_faults_pass(gpu, eng, name, where):
    pool, blobs, roots, _ = W.mutated(name, where, 0)
    want = G.check_host_pool(gpu, eng, pool, blobs, roots, G.OK)
    assert want[2]["ndead"] == 0


def test_smallest_bad_blob_and_the_order_of_codes(gpu, eng):
    trees, store = W.two_streams()
    roots = [t.root for t in trees]
    bad = [trees[0].nodes[2][7], trees[1].nodes[1][2], trees[1].nodes[2][0]]
    for n in bad:
        store[n["ref"]] = W.FAMILIES["truncated"][0](n)
    pool, blobs = W.pool_of(store)
    index = G.index_of(blobs)
    for order in (roots, roots[::-1]):
        want = G.check_host_pool(gpu, eng, pool, blobs, order, G.ECORRUPT)
        assert want[2]["bad_blob"] == min(index[n["ref"]] for n in bad)
    # a miss beside them: not found outranks corrupt, and the blob blamed is still the malformed
    gone = trees[0].nodes[2][2]
    pool, blobs = W.pool_of(_without(store, gone["ref"]))
    index = G.index_of(blobs)
    want = G.check_host_pool(gpu, eng, pool, blobs, roots, G.ENOTFOUND)
    assert want[2]["bad_blob"] == min(index[n["ref"]] for n in bad)
    # two misses alone: the smaller parent
    trees, store = W.two_streams()
    for n in (trees[0].nodes[2][8], trees[1].nodes[2][1]):
        store = _without(store, n["ref"])
    pool, blobs = W.pool_of(store)
    index = G.index_of(blobs)
    want = G.check_host_pool(gpu, eng, pool, blobs, roots, G.ENOTFOUND)
    assert want[2]["bad_blob"] == min(index[trees[0].nodes[1][2]["ref"]],
                                      index[trees[1].nodes[1][0]["ref"]])


def test_a_failed_mark_drops_the_good_one(gpu, eng):
    pool, blobs, roots, _ = W.mutated("padded", "leaf", 0)
    good = W.pool_of(W.two_streams()[1])
    G.check_host_pool(gpu, eng, good[0], good[1], roots, G.OK)
    G.check_host_pool(gpu, eng, pool, blobs, roots, G.ECORRUPT)  # (check: ESTATE afterwards)
    G.check_host_pool(gpu, eng, good[0], good[1], roots, G.OK)
    # an argument fault drops it too
    rc, _, _ = eng.gc_mark(0, good[1], W.roots_array(roots), pool_bytes=0, flags=2)
    assert rc == G.EINVAL
    assert gpu.lib().bsg_engine_copy_gc(eng.h, None, 0, None, 0, 0) == G.ESTATE


# ---- argument checks -----------------------------------------------------------------------------
def test_mark_einval_and_estate(gpu, eng):
    trees, store = W.two_streams()
    pool, blobs = W.pool_of(store)
    roots = W.roots_array([t.root for t in trees])
    L, info = gpu.lib(), gpu.GcInfo()
    pbuf = gpu.DeviceBuffer(len(pool))
    try:
        pbuf.from_host(pool)
        args = lambda **kw: [kw.get("pool", pbuf.ptr), kw.get("pool_bytes", len(pool)),  # noqa: E731
                             kw.get("blobs", blobs.ctypes.data), kw.get("nblobs", len(blobs)),
                             kw.get("roots", roots.ctypes.data), kw.get("nroots", len(roots)),
                             kw.get("flags", 0), None, ctypes.byref(info)]
        assert L.bsg_engine_gc_mark(eng.h, *args()) == G.OK
        assert L.bsg_engine_gc_mark(None, *args()) == G.EINVAL
        for kw in ({"pool": None}, {"blobs": None}, {"roots": None}, {"flags": 2}, {"flags": -1},
                   {"pool_bytes": int(blobs[-1]["off"]) + int(blobs[-1]["len"]) - 1},
                   {"nroots": 1 << 32}):
            assert L.bsg_engine_gc_mark(eng.h, *args(**kw)) == G.EINVAL, kw
            assert info.bad_root == G.NONE and info.nlive == 0
            assert eng.gc_live_device() == 0
        # null pointers with zero counts are fine
        assert L.bsg_engine_gc_mark(eng.h, *args(pool=None, pool_bytes=0, blobs=None, nblobs=0,
                                                 roots=None, nroots=0)) == G.OK
        # the model agrees on the layout faults
        assert G.run_model(pool, blobs, [], pool_bytes=len(pool) - 1)[0] == G.EINVAL
        assert G.run_model(pool, blobs, [], flags=2)[0] == G.EINVAL
        # an unfinished run: after the verdicts, before anything is published
        data = gpu.DeviceBuffer(1 << 16)
        try:
            data.from_host(np.arange(1 << 16, dtype=np.uint32).view(np.uint8)[:1 << 16])
            eng.run(data.ptr, [0], [1 << 16], bits=6, min_size=64, fanout=3)
            assert L.bsg_engine_gc_mark(eng.h, *args()) == G.ESTATE
            assert eng.gc_live_device() == 0
            eng.finish()
            assert L.bsg_engine_gc_mark(eng.h, *args()) == G.OK
        finally:
            data.free()
    finally:
        pbuf.free()


def test_compact_refusals_leave_the_output_alone(gpu, eng):
    pool, blobs, roots = G.len_mix("LLD")
    nbytes = (len(pool) + 15) & ~15
    buf = gpu.DeviceBuffer(2 * nbytes + 8192)  # the pool, then room for the output
    try:
        image = np.full(buf.nbytes, G.FILL, dtype=np.uint8)
        image[:len(pool)] = pool
        buf.from_host(image)
        out = buf.ptr + nbytes
        rc, info, _ = eng.gc_mark(buf.ptr, blobs, W.roots_array(roots), pool_bytes=len(pool))
        assert rc == G.OK
        live = G.run_model(pool, blobs, roots)[3]
        tight, al16 = (G.layout(blobs, live, a)[1] for a in (False, True))
        assert tight == info["live_bytes"] and al16 > tight
        kw = dict(pool_bytes=len(pool))
        refused = [
            eng.gc_compact(buf.ptr, out, cap=tight - 1, **kw),               # one byte short
            eng.gc_compact(buf.ptr, out, cap=al16 - 1, align16=True, **kw),
            eng.gc_compact(buf.ptr, buf.ptr + ((len(pool) - 1) & ~15), cap=1 << 20, **kw),  # overlap
            eng.gc_compact(buf.ptr, buf.ptr, cap=1 << 20, **kw),
            eng.gc_compact(buf.ptr, out + 8, cap=1 << 20, **kw),              # not 16-aligned
            eng.gc_compact(buf.ptr, 0, cap=1 << 20, **kw),                    # null
            eng.gc_compact(buf.ptr + 16, out, cap=1 << 20, **kw),             # not the mark's pool
            eng.gc_compact(buf.ptr, out, cap=1 << 20, pool_bytes=len(pool) - 1),
        ]
        assert refused == [(G.EINVAL, 0)] * len(refused)
        n = ctypes.c_uint64(7)
        assert gpu.lib().bsg_engine_gc_compact(eng.h, buf.ptr, len(pool), out, 1 << 20, 2,
                                               ctypes.byref(n)) == G.EINVAL and n.value == 0
        assert gpu.lib().bsg_engine_copy_gc(eng.h, None, 0, None, 0, 2) == G.EINVAL
        assert buf.to_host().tobytes() == image.tobytes()
        # the mark survives a refusal: the exact cap passes
        rc, n = eng.gc_compact(buf.ptr, out, cap=tight, **kw)
        assert rc == G.OK and n == tight
        got = buf.to_host()
        assert got[nbytes:nbytes + tight].tobytes() == G.compacted(pool, blobs, live, False).tobytes()
        image[nbytes:nbytes + tight] = got[nbytes:nbytes + tight]
        assert got.tobytes() == image.tobytes()
    finally:
        buf.free()

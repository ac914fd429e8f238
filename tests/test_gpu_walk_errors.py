"""bsg_engine_walk's refusals on the device, every one against the model of walk_cases.py: the
mutation families on a Root, a middle node and a leaf node, missing blobs, the status ranking,
the depth bound and the layout faults. No test here provokes a fault: every address the walk
forms is range-checked, and a refused walk publishes nothing."""
import numpy as np
import pytest

import walk_cases as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(gpu):
    e = gpu.Engine()
    yield e
    e.close()


def _refused(gpu, eng, pool, blobs, roots, expect):
    """The walk is refused as the model says, publishes nothing, and a restore_walk after it
    returns BSG_ESTATE with d_out untouched."""
    pbuf = gpu.DeviceBuffer(max(len(pool), 16))
    try:
        pbuf.from_host(pool)
        want = W.check(gpu, eng, pbuf, W.getter(pool, blobs), blobs, roots, len(pool), expect)
        rc, info, off, out = W.restore_walk(gpu, eng, pbuf, len(pool), blobs, [64] * len(roots))
        assert rc == W.ESTATE and (out == W.FILL).all() and info["bytes"] == 0
    finally:
        pbuf.free()
    return want


@pytest.mark.parametrize("name", sorted(W.FAMILIES))
def test_families(gpu, eng, name):
    for where in W.WHERE:
        for stream in (0, 1):
            pool, blobs, roots, want = W.mutated(name, where, stream)
            got = _refused(gpu, eng, pool, blobs, roots, want)
            assert got[1][stream] == want and got[1][1 - stream] == W.OK
            assert got[2]["bad_stream"] == stream


def test_leaf_blob_of_the_wrong_len(gpu, eng):
    trees, store = W.two_streams()
    roots = [t.root for t in trees]
    pool, blobs = W.pool_of(store)
    for stream in (0, 1):
        leaf = trees[stream].nodes[2][4]["kids"][1][0]
        k = next(i for i in range(len(blobs)) if blobs[i]["ref"].tobytes() == leaf)
        for d in (-1, 1):
            t = blobs.copy()
            t["len"][k] = int(t["len"][k]) + d
            got = _refused(gpu, eng, pool, t, roots, W.ECORRUPT)
            assert got[2]["bad_stream"] == stream


def test_missing_and_ranking(gpu, eng):
    trees, store = W.two_streams()
    roots = [t.root for t in trees]
    leaf = trees[1].nodes[2][4]["kids"][1][0]
    for gone in (trees[1].root, trees[1].nodes[1][1]["ref"], leaf):
        s = {r: b for r, b in store.items() if r != gone}
        got = _refused(gpu, eng, *W.pool_of(s), roots, W.ENOTFOUND)
        assert got[1].tolist() == [W.OK, W.ENOTFOUND]
    # a missing child and a malformed node in one stream: not found
    s = {r: b for r, b in store.items() if r != leaf}
    s[trees[1].nodes[2][0]["ref"]] = W.FAMILIES["padded"][0](trees[1].nodes[2][0])
    got = _refused(gpu, eng, *W.pool_of(s), roots, W.ENOTFOUND)
    assert got[1].tolist() == [W.OK, W.ENOTFOUND]
    # one corrupt and one missing stream: not found, both statuses right
    s[trees[0].nodes[1][2]["ref"]] = W.FAMILIES["size0"][0](trees[0].nodes[1][2])
    got = _refused(gpu, eng, *W.pool_of(s), roots, W.ENOTFOUND)
    assert got[1].tolist() == [W.ECORRUPT, W.ENOTFOUND] and got[2]["bad_stream"] == 0
    # a Root that is a chunk, not a node
    got = _refused(gpu, eng, *W.pool_of(store), [roots[0], leaf], W.ECORRUPT)
    assert got[1].tolist() == [W.OK, W.ECORRUPT]


def test_cycles_end(gpu, eng):
    """A node labelled with a ref that it lists as its own child: with one child the cover fits
    and the depth bound ends the walk, with two the cover rule does."""
    from oracle import oracle as O
    leaf = b"0123456789"
    me = W.sha(b"a label, since nothing is hashed")
    one = O.proto_node([(me, 0)], [], 0, 10)
    pool, blobs = W.pool_of({W.sha(leaf): leaf, me: one})
    got = _refused(gpu, eng, pool, blobs, [me], W.ECORRUPT)
    assert got[2]["depth"] == W.WALK_MAX_DEPTH and got[2]["nnodes"] == W.WALK_MAX_DEPTH + 1
    two = O.proto_node([(me, 0), (me, 4)], [], 0, 10)
    pool, blobs = W.pool_of({W.sha(leaf): leaf, me: two})
    got = _refused(gpu, eng, pool, blobs, [bytes(32), me], W.ECORRUPT)
    assert got[2]["depth"] == 1 and got[2]["nnodes"] == 3 and got[2]["bad_stream"] == 1


def test_depth_bound(gpu, eng):
    """The deepest node allowed lies at depth 64 (Root = 0): a chain down to it is read, a chain
    one node longer is refused at the node that names the 65th level."""
    pool, blobs, roots = W.chain(W.WALK_MAX_DEPTH)
    want = W.check_host_pool(gpu, eng, pool, blobs, roots, W.OK)
    assert want[2]["depth"] == 64 and want[2]["nrecs"] == 1
    pool, blobs, roots = W.chain(W.WALK_MAX_DEPTH + 1)
    got = _refused(gpu, eng, pool, blobs, roots, W.ECORRUPT)
    assert got[2]["depth"] == 64 and got[2]["nnodes"] == 65


def test_layout_faults(gpu, eng):
    pool, blobs, roots, _ = W.mixed_depth()
    L = gpu.lib()
    pbuf = gpu.DeviceBuffer(len(pool))
    try:
        pbuf.from_host(pool)
        W.check(gpu, eng, pbuf, W.getter(pool, blobs), blobs, roots, len(pool), W.OK)
        ra = W.roots_array(roots)
        st = np.zeros(1, dtype=np.int32)
        args = (pbuf.ptr, len(pool), blobs.ctypes.data, len(blobs), ra.ctypes.data, 1)
        assert L.bsg_engine_walk(None, *args, 0, st.ctypes.data, None) == W.EINVAL
        for bad in ((None, len(pool)) + args[2:], args[:2] + (None, len(blobs)) + args[4:],
                    args[:4] + (None, 1)):
            assert L.bsg_engine_walk(eng.h, *bad, 0, st.ctypes.data, None) == W.EINVAL
        # (each of these is a walk, and the one before them is gone)
        assert eng.walk_records_device() == 0
        W.check(gpu, eng, pbuf, W.getter(pool, blobs), blobs, roots, len(pool), W.EINVAL, flags=1)
        W.check(gpu, eng, pbuf, W.getter(pool, blobs), blobs, roots, len(pool) - 1, W.EINVAL)
        W.check(gpu, eng, pbuf, W.getter(pool, blobs), blobs, [bytes(32)] * 65536, len(pool),
                W.EINVAL)
        # null status and info are fine, and 65,535 streams are not too many
        assert L.bsg_engine_walk(eng.h, *args, 0, None, None) == W.OK
        W.check(gpu, eng, pbuf, W.getter(pool, blobs), blobs, [bytes(32)] * 65534 + roots,
                len(pool), W.OK)
        recs, sizes, counts = eng.copy_walk()
        assert counts[-1] == len(recs) == 7 and (recs["stream"] == 65534).all()
        # copy_walk: fewer streams than the walk's, more is a fault
        s2 = np.zeros(2, dtype=np.uint64)
        assert L.bsg_engine_copy_walk(eng.h, None, 0, s2.ctypes.data, None, 2) == W.OK
        assert L.bsg_engine_copy_walk(eng.h, None, 0, None, None, 65536) == W.EINVAL
        rc, info = eng.restore_walk(pbuf.ptr, blobs, 0, [0], pool_bytes=len(pool), out_cap=0)
        assert rc == W.EINVAL  # nstreams is not the walk's
    finally:
        pbuf.free()

"""bsg_engine_gc_mark where no accepted walk can go and past one pass of its grids, against the
model of gc_cases.py bit for bit.

Offsets up to 2^64 - 2 (entries of 45, 46 and 47 bytes, varints of 8, 9 and 10 bytes): a mark holds
no child to a cover, so a tiny pool carries them through the lanes' parse of k_wk_count, wk_entry
and the ref reads of k_gc_emit and k_gc_missing; and the faults of the 10-byte form, each on lane 0
and on a later lane of a 64-entry group, through the mark and the walk alike.

More than one grid pass: a launch is capped at T = 8 x CUs x 256 threads (engine_grid) and the
count pass at N = 64 x CUs x 4 waves (launch_walk_count), both read from the source and the device,
so every kernel's grid-stride loop makes a second trip here: k_wk_count (N + 3 nodes in a level),
k_gc_roots and k_gc_status (T + 5 Roots), k_gc_emit and k_gc_missing (T + 7 entries in a node),
k_dd_insert as the pool's index and k_gc_offsets (more than 2 T blobs), and k_sum_mid with several
parts per thread. None of these inputs is malformed beyond what a parse verdict answers."""
import numpy as np
import pytest

import gc_cases as G
import walk_cases as W
from test_gpu_tier_counts import cus  # noqa: F401  (the device's CU count, a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture()
def eng(gpu):
    e = gpu.Engine()
    yield e
    e.close()


# ---- offsets up to 2^64 - 1 --------------------------------------------------------------------
def test_every_entry_length_and_offsets_up_to_2_64(gpu, eng):
    """Five Roots: all eleven entry lengths in one node, the changes on lanes 0, 32 and 63; size
    2^64 - 1 at offset 0; offset 2^63 with size 2^63 - 1. The leaves that entries of 45, 46 and
    47 bytes alone name are live."""
    pool, blobs, roots = G.edge_pool()
    want = G.check_host_pool(gpu, eng, pool, blobs, roots, G.OK)
    index = G.index_of(blobs)
    for e in (45, 46, 47):
        assert want[3][index[W.sha(W.only_leaf(e))]] == 1, e
    assert want[2]["nnodes"] == 5 and want[2]["ndead"] == 1 and want[2]["depth"] == 0


@pytest.mark.parametrize("name,lane", W.WIDE_CASES)
def test_ten_byte_varint_faults(gpu, eng, name, lane):
    """The lanes' rules for a varint of ten bytes. Only the mark's verdict depends on the form:
    the node as it was passes the mark (test_gc_cases_cpu.py), while the walk refuses it for its
    covers too, so the walk's call shows no more than that the fault does it no harm. Lane 0's
    fault is found by the step that starts there, a later lane's by the ballot. ends_02 and
    ends_00 would also fall to the ascending rule if the parser kept the low 64 bits; the _alone
    families (lane 0 only: a later lane's elder is at 2^63 at least) leave the offsets ascending,
    so the tenth byte's own rule is all that refuses them."""
    pool, blobs, roots, k = W.wide_mutated(name, lane)
    want = G.check_host_pool(gpu, eng, pool, blobs, roots, G.ECORRUPT)
    assert want[2]["bad_blob"] == k and want[1].tolist() == [0, G.ECORRUPT]
    want = W.check_host_pool(gpu, eng, pool, blobs, roots, W.ECORRUPT)
    assert want[1].tolist() == [0, W.ECORRUPT] and want[2]["bad_stream"] == 1


def test_the_leaf_of_the_47_byte_entries_is_missing(gpu, eng):
    """Four entries of 47 bytes name it; with BSG_GC_MISSING_LEAVES it counts once."""
    pool, blobs, roots = G.edge_pool(drop=[W.sha(W.only_leaf(47))])
    want = G.check_host_pool(gpu, eng, pool, blobs, roots, G.OK, flags=G.GC_MISSING_LEAVES)
    assert want[2]["missing_leaves"] == 1 and want[2]["nnodes"] == 5
    G.check_host_pool(gpu, eng, pool, blobs, roots, G.ENOTFOUND)


# ---- more than one grid pass -------------------------------------------------------------------
def test_more_nodes_than_a_count_pass(gpu, eng, cus):  # noqa: F811
    """A level of N + 3 leaf nodes: each is expanded only if its own wave's trip ran."""
    n = W.count_waves(cus)
    pool, blobs, roots = G.wide(n + 3)
    want = G.check_host_pool(gpu, eng, pool, blobs, roots, G.OK)
    assert want[2]["nnodes"] == n + 4 and want[2]["ndead"] == 0 and want[2]["depth"] == 1


def test_more_roots_than_a_grid_pass(gpu, eng, cus):  # noqa: F811
    """T + 5 Roots; the last two alone name the second and the third tree. Then the third tree's
    Root blob malformed: the status of exactly that Root is corrupt."""
    t = W.grid_threads(cus)
    pool, blobs, roots, own = G.many_roots(t + 5)
    want = G.check_host_pool(gpu, eng, pool, blobs, roots, G.OK)
    assert want[3][own[1]].all() and want[3][own[2]].all() and want[2]["nnodes"] == 39
    assert len(want[1]) == t + 5 and want[2]["ndead"] == 0
    pool, blobs, roots, own = G.many_roots(t + 5, malformed=True)
    want = G.check_host_pool(gpu, eng, pool, blobs, roots, G.ECORRUPT)
    assert want[1][-1] == G.ECORRUPT and not want[1][:-1].any()
    assert want[2]["bad_root"] == t + 4 and want[2]["bad_blob"] == G.index_of(blobs)[roots[-1]]


def test_more_children_and_blobs_than_a_grid_pass(gpu, eng, cus):  # noqa: F811
    """A leaf node of T + 7 entries in a pool of 2 (T + 7) blobs, compacted tight and 16-aligned;
    then, with BSG_GC_MISSING_LEAVES, without the last 100 live leaves in the table."""
    t, tile = W.grid_threads(cus), W.grid_caps()["kSumTile"]
    nblobs = 2 * (t + 7)
    assert -(-nblobs // tile) > 256  # k_sum_mid: more than one part per thread
    pool, blobs, roots, flags = G.sized_pool(nblobs)
    root_k = int(np.flatnonzero((blobs["ref"] == np.frombuffer(roots[0], np.uint8)).all(axis=1))[0])
    pbuf = gpu.DeviceBuffer(len(pool))
    try:
        pbuf.from_host(pool)
        want = G.check(gpu, eng, pbuf, pool, blobs, roots, expect=G.OK, flags=flags)
        assert want[2]["nlive"] == t + 8 and want[2]["ndead"] == t + 6 and want[2]["nnodes"] == 1
        gone = [k for k in np.flatnonzero(want[3]).tolist() if k != root_k][-100:]
        fewer = np.delete(blobs, gone)
        want = G.mark(W.getter(pool, fewer), fewer, roots, len(pool), G.GC_MISSING_LEAVES)
        rc, info, status = eng.gc_mark(pbuf.ptr, fewer, W.roots_array(roots), pool_bytes=len(pool),
                                       flags=G.GC_MISSING_LEAVES)
        assert rc == want[0] == G.OK and info == want[2], (rc, info, want[2])
        assert info["missing_leaves"] == 100 and info["nlive"] == t + 8 - 100
        assert status.tolist() == [0]
        assert eng.copy_gc()[0].tobytes() == want[3].tobytes()
    finally:
        pbuf.free()

"""bsg_engine_walk, bsg_engine_restore_walk and bsg_engine_restore past one pass of their grids,
against the model of walk_cases.py bit for bit.

A launch is capped at T = 8 x CUs x 256 threads (engine_grid) and the count pass at N = 64 x CUs x
4 waves (launch_walk_count), both read from the source and the device. Here a level holds more
than N nodes (k_wk_count's second trip), more than T leaf children over many nodes and within one
node (k_wk_emit, k_wk_records), a level more than T nodes (k_wk_nrec, k_wk_rbase) and a walk more
than T records (k_rs_resolve), and offsets cross 2^49: entries of 45 bytes, varints of 8. Every
pool, table and Root is valid."""
import numpy as np
import pytest

import gc_cases as G
import walk_cases as W
from test_gpu_tier_counts import cus  # noqa: F401  (the device's CU count, a fixture)
from test_gpu_walk import _stride_case

pytestmark = pytest.mark.gpu


@pytest.fixture()
def eng(gpu):
    e = gpu.Engine()
    yield e
    e.close()


def test_stride_changes_across_2_49(gpu, eng, cus):  # noqa: F811
    """test_stride_changes_large_offsets' scheme with 2^49 as a seventh threshold: three streams of
    2^19 and a few leaves, nearly all the unwritten 1 GiB blob, the change to entries of 45 bytes
    on lanes 0, 32 and 63. Each stream is one leaf node of more than T children, so one node's
    children take k_wk_emit's and k_wk_records' second trip. Varints of 9 and 10 bytes (offsets
    of 2^56 and more) cannot be reached by an accepted walk: they would need 2^26 leaves of
    1 GiB. test_gpu_gc_wide.py reaches them through the mark and through the walk's refusals."""
    t = W.grid_threads(cus)
    tail = max(40, t - (1 << 19) + 40)
    want = _stride_case(gpu, eng, [1 << (7 * j) for j in range(1, 8)], 1 << 30, tail,
                        gmax=1 << 20)
    assert int(want[5].min()) > t, (want[5], t)
    recs = want[3]
    for s in range(3):
        far = recs[(recs["stream"] == s) & (recs["offset"] >= 1 << 49)]
        assert len(far) >= tail and (far["len"] == 1 << 30).all(), s
    assert int(want[4].min()) > 1 << 49


def test_more_nodes_children_and_records_than_a_grid_pass(gpu, eng, cus):  # noqa: F811
    """T // 27 + 2 three_level streams of three distinct trees, with empty streams and mixed_depth
    trees among them and as the last three: more than N nodes at depth 2 and more than T leaf
    children and records. Walked, restored from the walk's records on the device, and restored
    once more from the same records given by the host."""
    t, n = W.grid_threads(cus), W.count_waves(cus)
    n3 = t // 27 + 2
    pool, blobs, roots, kinds, data = W.many_streams(n3)
    assert 9 * n3 > n and 27 * n3 > t
    pbuf = gpu.DeviceBuffer(len(pool))
    try:
        pbuf.from_host(pool)
        want = W.check(gpu, eng, pbuf, W.getter(pool, blobs), blobs, roots, len(pool), W.OK)
        assert want[2]["nrecs"] == 27 * n3 + 3 * 7 and want[2]["depth"] == 2
        assert want[5].tolist() == [len(W.mixed_depth()[3]) if k == "m" else 0 if k == "z" else 27
                                    for k in kinds]
        recs, sizes, counts = eng.copy_walk()
        rc, info, off, out = W.restore_walk(gpu, eng, pbuf, len(pool), blobs, sizes)
        assert rc == W.OK and info["bytes"] == sum(len(data[k]) for k in kinds), (rc, info)
        for s, k in enumerate(kinds):
            assert out[off[s]:off[s] + len(data[k])].tobytes() == data[k], (s, k)
        obuf = gpu.DeviceBuffer(len(out))
        try:
            obuf.from_host(np.full(len(out), W.FILL, dtype=np.uint8))
            # (restore raises on any return code but OK and gives its info back)
            again = eng.restore(pbuf.ptr, blobs, recs, obuf, off, sizes, pool_bytes=len(pool))
            assert again["bytes"] == info["bytes"], (again, info)
            assert obuf.to_host().tobytes() == out.tobytes()
        finally:
            obuf.free()
    finally:
        pbuf.free()


def test_more_nodes_in_a_level_than_a_grid_pass(gpu, eng, cus):  # noqa: F811
    """One stream whose Root names T + 3 leaf nodes of one leaf each (gc_cases.wide): a `nodes`
    node of more than T entries, and a level of more than T nodes, so every thread of k_wk_nrec
    and k_wk_rbase makes a second trip. Walked and restored from the walk's records."""
    t = W.grid_threads(cus)
    pool, blobs, roots = G.wide(t + 3)
    pbuf = gpu.DeviceBuffer(len(pool))
    try:
        pbuf.from_host(pool)
        want = W.check(gpu, eng, pbuf, W.getter(pool, blobs), blobs, roots, len(pool), W.OK)
        assert want[2]["nnodes"] == t + 4 and want[2]["nrecs"] == t + 3 and want[2]["depth"] == 1
        rc, info, off, out = W.restore_walk(gpu, eng, pbuf, len(pool), blobs, want[4])
        assert rc == W.OK and info["bytes"] == 10 * (t + 3), (rc, info)
        assert out[off[0]:off[0] + 10 * (t + 3)].tobytes() == b"0123456789" * (t + 3)
    finally:
        pbuf.free()

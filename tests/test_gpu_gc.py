"""bsg_engine_gc_mark, bsg_engine_copy_gc and bsg_engine_gc_compact on the device against the model
of gc_cases.py, bit for bit: sharing and races for a blob, the pool's rules, the count and depth
limits, the compaction's edges, what a mark must leave alone, and an engine run swept and read
back."""
import numpy as np
import pytest

import gc_cases as G
import walk_cases as W
from bs_amd.synth import splitmix_array
from test_gpu_walk import RunPool

pytestmark = pytest.mark.gpu


@pytest.fixture()
def eng(gpu):
    e = gpu.Engine()
    yield e
    e.close()


# ---- sharing and races ---------------------------------------------------------------------------
def test_two_roots_share_a_subtree(gpu, eng):
    pool, blobs, roots, nodes = G.shared_subtree()
    want = G.check_host_pool(gpu, eng, pool, blobs, roots, G.OK)
    assert want[2]["nnodes"] == nodes and want[2]["ndead"] == 0
    # one Root alone leaves the other's own subtree dead
    want = G.check_host_pool(gpu, eng, pool, blobs, roots[:1], G.OK)
    assert want[2]["nnodes"] == 1 + 3 * 4 and want[2]["ndead"] == 1 + 4 + 9


def test_one_root_a_thousand_times(gpu, eng):
    t, lstore = W.three_level(4)
    pool, blobs = W.pool_of({**lstore, **t.store()})
    want = G.check_host_pool(gpu, eng, pool, blobs, [t.root] * 1000, G.OK)
    assert want[2]["nnodes"] == 13 and want[1].tolist() == [0] * 1000


def test_4096_entries_for_one_child(gpu, eng):
    pool, blobs, roots = G.same_child_level(64)
    want = G.check_host_pool(gpu, eng, pool, blobs, roots, G.OK)
    assert want[2]["nnodes"] == 1 + 64 + 1 and want[2]["depth"] == 2 and want[2]["ndead"] == 0


def test_a_label_cycle_ends(gpu, eng):
    pool, blobs, roots = G.cycle()
    want = G.check_host_pool(gpu, eng, pool, blobs, roots, G.OK)
    assert want[3].tolist() == [1, 1] and want[2]["nnodes"] == 2


@pytest.mark.parametrize("order", [(0, 1), (1, 0), (0,)])
def test_named_under_leaves_and_under_nodes(gpu, eng, order):
    pool, blobs, roots, leaf = G.both_ways()
    want = G.check_host_pool(gpu, eng, pool, blobs, [roots[j] for j in order], G.OK)
    assert want[3][leaf] == (len(order) == 2)


# ---- the pool's rules ----------------------------------------------------------------------------
def test_duplicate_refs_and_zero_roots(gpu, eng):
    t, lstore = W.three_level(6)
    ent = list({**lstore, **t.store()}.items())
    n = t.nodes[1][1]
    k = [r for r, _ in ent].index(n["ref"])
    # a malformed twin after the good blob is dead; a good twin before a malformed one is used
    ent.append((n["ref"], W.FAMILIES["padded"][0](n)))
    ent.append((ent[0][0], b"another blob under the first leaf's ref"))
    pool, blobs = G.pool_from(ent)
    roots = [bytes(32), t.root, bytes(32)]
    want = G.check_host_pool(gpu, eng, pool, blobs, roots, G.OK)
    assert want[3][k] == 1 and want[3][-2:].tolist() == [0, 0] and want[2]["ndead"] == 2
    ent.insert(0, ent.pop(-2))
    pool, blobs = G.pool_from(ent)
    want = G.check_host_pool(gpu, eng, pool, blobs, roots, G.ECORRUPT)
    assert want[2]["bad_blob"] == 0


def test_no_roots_everything_is_dead(gpu, eng):
    t, lstore = W.three_level(7)
    pool, blobs = W.pool_of({**lstore, **t.store()})
    for roots in ([], [bytes(32)] * 3):
        want = G.check_host_pool(gpu, eng, pool, blobs, roots, G.OK)
        assert want[2]["nlive"] == 0 and want[2]["ndead"] == len(blobs)
    # and an empty pool
    G.check_host_pool(gpu, eng, np.zeros(0, np.uint8), blobs[:0], [], G.OK)


@pytest.mark.parametrize("nblobs", [1, 63, 64, 65, 2049])
def test_nblobs(gpu, eng, nblobs):
    pool, blobs, roots, flags = G.sized_pool(nblobs)
    want = G.check_host_pool(gpu, eng, pool, blobs, roots, G.OK, flags=flags)
    assert want[2]["nlive"] == nblobs // 2 + 1 and want[2]["missing_leaves"] == (nblobs == 1)


# ---- limits --------------------------------------------------------------------------------------
def test_2049_children_and_a_level_of_2049(gpu, eng):
    pool, blobs, roots = G.wide(2049)
    want = G.check_host_pool(gpu, eng, pool, blobs, roots, G.OK)
    assert want[2]["nnodes"] == 2050 and want[2]["depth"] == 1


def test_70000_roots(gpu, eng):
    t, lstore = W.three_level(8)
    store = {r: lstore[r] for r, _ in t.nodes[2][0]["kids"]}
    mid = W.Tree._node(1, [(t.nodes[2][0]["ref"], 0)], 0, t.nodes[2][0]["size"])
    top = W.Tree._node(1, [(mid["ref"], 0)], 0, mid["size"])
    for n in (t.nodes[2][0], mid, top):
        store[n["ref"]] = n["bytes"]
    pool, blobs = W.pool_of(store)
    refs = [top["ref"], mid["ref"], t.nodes[2][0]["ref"], bytes(32)]
    roots = [refs[(r * 7) % 4] for r in range(70000)]
    want = G.check_host_pool(gpu, eng, pool, blobs, roots, G.OK)
    assert want[2]["nnodes"] == 3 and want[2]["depth"] == 0 and len(want[1]) == 70000


def test_chains(gpu, eng):
    pool, blobs, roots = W.chain(69)  # 70 nodes: the one at depth 64 names a node
    want = G.check_host_pool(gpu, eng, pool, blobs, roots, G.ECORRUPT)
    assert want[2]["depth"] == 64 and want[1].tolist() == [0]
    pool, blobs, roots = W.chain(99)
    want = G.check_host_pool(gpu, eng, pool, blobs, roots + [blobs[50]["ref"].tobytes()], G.OK)
    assert want[2]["depth"] == 49 and want[2]["nnodes"] == 100


# ---- compact -------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["L", "DL", "LD", "DDLLDDL", "LLDDDDLD", "D"])
def test_compact_lens_and_dead_runs(gpu, eng, pattern):
    """Lens 0, 1, 15, 16, 17 and 4,097 at odd pool offsets; dead blobs first, last, in runs, none
    and all. check() compacts tight and 16-aligned into a pre-filled buffer with guards."""
    pool, blobs, roots = G.len_mix(pattern)
    want = G.check_host_pool(gpu, eng, pool, blobs, roots, G.OK)
    assert want[2]["nlive"] == (0 if pattern == "D" else 1 + sum(
        pattern[i % len(pattern)] == "L" for i in range(12)))


def test_compact_larger_than_a_tile(gpu, eng):
    """Several output tiles, blobs that straddle them, and dead blobs between."""
    rng = np.random.default_rng(3)
    lens = [40000, 1, 33000, 70001, 17, 32768, 5]
    data = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    refs = [W.sha(d) for d in data]
    offs = np.cumsum([0] + lens).tolist()
    ln = G.node(leaves=[(refs[i], offs[i]) for i in (0, 2, 3, 4, 6)], size=offs[-1])
    pool, blobs = G.pool_from(list(zip(refs, data)) + [(W.sha(ln), ln)], first=5)
    G.check_host_pool(gpu, eng, pool, blobs, [W.sha(ln)], G.OK)


# ---- non-interference and determinism ------------------------------------------------------------
def test_mark_twice(gpu, eng):
    pool, blobs, roots, _ = G.shared_subtree()
    pbuf = gpu.DeviceBuffer(len(pool))
    try:
        pbuf.from_host(pool)
        got = []
        for _ in range(2):
            rc, info, status = eng.gc_mark(pbuf.ptr, blobs, W.roots_array(roots),
                                           pool_bytes=len(pool))
            assert rc == G.OK
            got.append([info, status.tobytes()] + [x.tobytes() for al in (False, True)
                                                   for x in eng.copy_gc(align16=al)])
        assert got[0] == got[1]
    finally:
        pbuf.free()


def _streams():
    a = splitmix_array(1, 30000)
    b = np.concatenate([a[:20000], splitmix_array(2, 9000)])
    return [a, b, splitmix_array(3, 9107), splitmix_array(4, 12000)]


def test_mark_and_compact_leave_the_run_alone(gpu, eng):
    streams = _streams()[:3]
    rp = RunPool(gpu, eng, streams, 4, 64, 2)
    try:
        roots = [r.tobytes() for r in rp.roots]
        W.check(gpu, eng, rp.pbuf, rp.blob_bytes, rp.blobs, roots, rp.pool_bytes, expect=W.OK)
        walked = [x.tobytes() for x in eng.copy_walk()]
        pool = rp.pbuf.to_host(0, rp.pool_bytes)
        G.check(gpu, eng, rp.pbuf, pool, rp.blobs, roots[:2], rp.pool_bytes, G.OK)
        assert eng.chunks().tobytes() == rp.recs.tobytes()
        first = np.zeros(len(rp.recs), dtype=np.uint64)
        uniq = np.zeros(eng.nunique, dtype=np.uint64)
        pack_off = np.zeros(eng.nunique + 1, dtype=np.uint64)
        assert gpu.lib().bsg_engine_copy_dedup(eng.h, first.ctypes.data, len(first),
                                               uniq.ctypes.data, pack_off.ctypes.data,
                                               len(uniq)) == 0
        assert (first.tobytes(), uniq.tobytes(), pack_off.tobytes()) == rp.dedup
        nn = np.zeros(len(rp.nodes), dtype=gpu.TREE_NODE_DTYPE)
        ar = np.zeros(len(rp.arena), dtype=np.uint8)
        assert gpu.lib().bsg_engine_copy_tree_nodes(eng.h, nn.ctypes.data, len(nn),
                                                    ar.ctypes.data, len(ar)) == 0
        assert nn.tobytes() == rp.nodes.tobytes() and ar.tobytes() == rp.arena.tobytes()
        rr = np.zeros((len(streams), 32), dtype=np.uint8)
        assert gpu.lib().bsg_engine_copy_roots(eng.h, rr.ctypes.data, None, len(streams)) == 0
        assert rr.tobytes() == rp.roots.tobytes()
        assert [x.tobytes() for x in eng.copy_walk()] == walked
    finally:
        rp.free()


def test_gc_on_a_fresh_engine(gpu):
    e = gpu.Engine()
    try:
        assert e.gc_live_device() == 0
        assert gpu.lib().bsg_engine_copy_gc(e.h, None, 0, None, 0, 0) == G.ESTATE
        pool, blobs, roots, _ = W.mixed_depth()
        G.check_host_pool(gpu, e, pool, blobs, roots, G.OK)
    finally:
        e.close()


# ---- end to end ----------------------------------------------------------------------------------
def test_run_sweep_walk_restore(gpu, eng):
    """Four streams, two sharing a long prefix, taken apart into one pool; the fourth Root is
    dropped, the pool swept 16-aligned, and the three kept streams read back from the swept pool
    with every blob verified."""
    streams = _streams()
    rp = RunPool(gpu, eng, streams, 4, 64, 2)
    try:
        assert len({int(n["height"]) for n in rp.nodes}) >= 3
        roots = [r.tobytes() for r in rp.roots]
        pool = rp.pbuf.to_host(0, rp.pool_bytes)
        want = G.check(gpu, eng, rp.pbuf, pool, rp.blobs, roots[:3], rp.pool_bytes, G.OK)
        live, index = want[3], G.index_of(rp.blobs)
        own = [set(rp.recs["ref"][rp.recs["stream"] == s].tobytes()[i:i + 32]
                   for i in range(0, 32 * int(rp.counts[s]), 32)) for s in range(4)]
        kept = own[0] | own[1] | own[2]
        assert own[0] & own[1] and own[3] - kept
        assert all(live[index[r]] == 0 for r in own[3] - kept)
        assert all(live[index[r]] == 1 for r in kept)
        nodes_of = np.split(np.arange(len(rp.nodes)), np.cumsum(rp.ncounts.astype(np.int64))[:-1])
        for s in range(4):
            for i in nodes_of[s]:
                assert live[index[rp.nodes[i]["ref"].tobytes()]] == (s < 3), (s, i)
        assert live[index[roots[3]]] == 0 and want[2]["ndead"] > 0

        _, table = eng.copy_gc(align16=True)
        end = G.layout(rp.blobs, live, True)[1]
        obuf = gpu.DeviceBuffer(end)  # (a DeviceBuffer has BSG_READ_SLACK readable bytes after it)
        try:
            obuf.from_host(np.zeros(end + gpu.READ_SLACK, dtype=np.uint8))
            rc, n = eng.gc_compact(rp.pbuf.ptr, obuf, align16=True, pool_bytes=rp.pool_bytes)
            assert rc == G.OK and n == end
            nbytes = end + gpu.READ_SLACK
            rc, info, status = eng.walk(obuf.ptr, table, W.roots_array(roots), pool_bytes=nbytes)
            assert rc == W.ENOTFOUND and status.tolist() == [0, 0, 0, W.ENOTFOUND]
            rc, info, status = eng.walk(obuf.ptr, table, W.roots_array(roots[:3]),
                                        pool_bytes=nbytes)
            assert rc == W.OK, (rc, info)
            _, sizes, _ = eng.copy_walk()
            assert sizes.tolist() == [len(d) for d in streams[:3]]
            rc, info, off, out = W.restore_walk(gpu, eng, obuf, nbytes, table, sizes, verify=True)
            assert rc == W.OK and info["verified"] > 0, (rc, info)
            for s, d in enumerate(streams[:3]):
                assert out[off[s]:off[s] + len(d)].tobytes() == d.tobytes(), s
        finally:
            obuf.free()
    finally:
        rp.free()

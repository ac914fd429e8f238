"""bsg_engine_walk on the device against the model of walk_cases.py: engine runs taken apart
(trees, dedup, pack) and read back from their Roots, tall and wide trees, changes of the entry
length inside one node, leaf nodes at mixed depths, and what a walk must leave alone."""
import numpy as np
import pytest

import tree_cases as TC
import tree_form as TF
import walk_cases as W
from bs_amd.synth import splitmix_array
from test_gpu_engine_trees import _run

pytestmark = pytest.mark.gpu


@pytest.fixture()
def eng(gpu):
    e = gpu.Engine()
    yield e
    e.close()


class RunPool:
    """An engine run taken apart: run -> trees -> dedup -> pack, and the pool of the packed
    chunks with the tree arena's node blobs appended."""

    def __init__(self, gpu, eng, streams, bits, mn, fanout):
        self.src = _run(gpu, eng, streams, bits, mn, fanout)
        self.recs, self.counts = eng.chunks(), eng.counts()
        self.roots, self.ncounts, self.nodes, self.arena = eng.trees()
        first, uniq, pack_off = eng.dedup()
        self.dedup = (first.tobytes(), uniq.tobytes(), pack_off.tobytes())
        nu, ub = eng.nunique, eng.unique_bytes
        self.base = (ub + 15) & ~15
        self.pool_bytes = self.base + len(self.arena) + gpu.READ_SLACK
        self.pbuf = gpu.DeviceBuffer(self.pool_bytes)
        self.pbuf.from_host(np.zeros(self.pool_bytes, dtype=np.uint8))
        if ub:
            eng.pack_unique(self.pbuf, 0, cap=ub)
        if len(self.arena):
            self.pbuf.from_host(self.arena, offset=self.base)
        u = uniq.astype(np.int64)
        ent = [(int(pack_off[k]), int(self.recs["len"][i]), self.recs["ref"][i].tobytes())
               for k, i in enumerate(u)]
        ent += [(self.base + int(n["blob_off"]), int(n["blob_len"]), n["ref"].tobytes())
                for n in self.nodes]
        self.blobs = W.table_of(ent)
        self.nchunk_blobs = nu

    def blob_bytes(self, k):
        assert k >= self.nchunk_blobs, "the model read a chunk as a node"
        o = int(self.blobs[k]["off"]) - self.base
        return self.arena[o:o + int(self.blobs[k]["len"])].tobytes()

    def free(self):
        self.src.free()
        self.pbuf.free()


def _round_trip(gpu, eng, streams, bits, mn, fanout, verify=False):
    rp = RunPool(gpu, eng, streams, bits, mn, fanout)
    try:
        roots = [r.tobytes() for r in rp.roots]
        want = W.check(gpu, eng, rp.pbuf, rp.blob_bytes, rp.blobs, roots, rp.pool_bytes,
                       expect=W.OK)
        recs, sizes, counts = eng.copy_walk()
        for f in ("stream", "offset", "len", "ref"):
            assert (recs[f] == rp.recs[f]).all(), f
        assert (recs["level"] == 0).all()
        assert sizes.tolist() == [len(d) for d in streams]
        assert counts.tolist() == rp.counts.tolist()
        assert want[2]["nnodes"] == len(rp.nodes)
        rc, info, off, out = W.restore_walk(gpu, eng, rp.pbuf, rp.pool_bytes, rp.blobs, sizes,
                                            verify=verify)
        assert rc == W.OK and info["bytes"] == sum(len(d) for d in streams), (rc, info)
        for s, d in enumerate(streams):
            assert out[off[s]:off[s] + len(d)].tobytes() == bytes(d), s
        return rp, want
    except BaseException:
        rp.free()
        raise


# ---- 1. round trip -----------------------------------------------------------------------------
@pytest.mark.parametrize("bits,mn,fanout", [(4, 64, 2), (6, 64, 3), (16, 1024, 8)])
def test_round_trip(gpu, eng, bits, mn, fanout):
    """A 0-byte stream, a one-chunk stream, the fixture streams (a pruned would-be root among
    them) and streams of different Root heights in one run."""
    lens = [820, 0, 40, 979, 9107, 30000] if bits < 16 else [187986, 0, 500, 1 << 21]
    streams = [splitmix_array(1 + (s > 4), n) if n else np.zeros(0, np.uint8)
               for s, n in enumerate(lens)]
    rp, want = _round_trip(gpu, eng, streams, bits, mn, fanout)
    try:
        assert rp.counts[1] == 0 and rp.counts[2] == 1 and not rp.roots[1].any()
        if bits < 16:
            heights = {int(n["height"]) for n in rp.nodes}
            roots_h = {int(rp.nodes[int(rp.ncounts[:s + 1].sum()) - 1]["height"])
                       for s in range(len(lens)) if rp.ncounts[s]}
            assert len(heights) >= 2 and len(roots_h) >= 2
            assert want[2]["depth"] == max(heights)
    finally:
        rp.free()


# ---- 2. tall and many --------------------------------------------------------------------------
def test_tallest_tree(gpu, eng, table):
    """Fanout 1 at Bits 1: 32 heights, the Root 31 levels above its first leaf node."""
    lists = [[0, 2, 0, 1], TC.TALL_LEVELS, [], [31]]
    R, _ = TF.stream_heights(TC.TALL_LEVELS, 1)
    assert R == 31
    rp, want = _round_trip(gpu, eng, TC.streams_of(table, TC.TALL_BITS, lists), TC.TALL_BITS, 64, 1)
    rp.free()
    assert want[2]["depth"] == 31


def test_many_streams_and_a_wide_node(gpu, eng):
    """3,000 one-chunk streams in one walk, and one stream whose leaf node holds more than
    64 x 64 children."""
    store, roots, datas = {}, [], []
    for s in range(3000):
        d = b"stream %d" % s + bytes(s % 7)
        store[W.sha(d)] = d
        n = W.Tree([(W.sha(d), len(d))])
        store.update(n.store())
        roots.append(n.root)
        datas.append(d)
    wide = [bytes([i % 251]) * (1 + i % 3) for i in range(64 * 64 + 77)]
    for d in wide:
        store[W.sha(d)] = d
    t = W.Tree([(W.sha(d), len(d)) for d in wide], arity=len(wide))
    store.update(t.store())
    roots.insert(1500, t.root)
    datas.insert(1500, b"".join(wide))
    pool, blobs = W.pool_of(store)
    pbuf = gpu.DeviceBuffer(len(pool))
    try:
        pbuf.from_host(pool)
        want = W.check(gpu, eng, pbuf, W.getter(pool, blobs), blobs, roots, len(pool), W.OK)
        assert want[2]["nnodes"] == 3001 and want[5][1500] == len(wide)
        rc, info, off, out = W.restore_walk(gpu, eng, pbuf, len(pool), blobs, want[4])
        assert rc == W.OK
        for s in (0, 1499, 1500, 1501, 3000):
            assert out[off[s]:off[s] + len(datas[s])].tobytes() == datas[s], s
    finally:
        pbuf.free()


# ---- 3. stride changes inside one node ---------------------------------------------------------
def _stride_case(gpu, eng, thresholds, bmax, tail, gmax=1 << 14):
    """One walk of three streams, the entry length changing first (lane 0), in the middle (32)
    and last (63) of a 64-entry group. The leaves all alias one unwritten stretch of bmax bytes
    after the node blobs: the walk reads no leaf byte."""
    nodes, roots, ent, lanes = [], [], {}, []
    for lane in (0, 32, 63):
        lens = W.crossing_lens(thresholds, bmax, lane, tail, gmax)
        ch = W.stride_lanes(lens)
        assert len(ch) == 1 + len(thresholds) and all(ln == lane for _, ln in ch[1:])
        b, root, leaves = W.stride_node(lens, 0)
        nodes.append((root, b))
        roots.append(root)
        ent.update({r: n for _, n, r in leaves})
        lanes.append(len(lens))
    head = b"".join(b for _, b in nodes)
    at = (len(head) + 15) & ~15
    entries, o = [], 0
    for root, b in nodes:
        entries.append((o, len(b), root))
        o += len(b)
    entries += [(at, n, r) for r, n in ent.items()]
    blobs = W.table_of(entries)
    pool_bytes = at + bmax
    pbuf = gpu.DeviceBuffer(pool_bytes)
    try:
        pbuf.from_host(np.frombuffer(head, dtype=np.uint8))
        want = W.check(gpu, eng, pbuf, lambda k: nodes[k][1], blobs, roots, pool_bytes, W.OK)
        assert want[5].tolist() == lanes
        return want
    finally:
        pbuf.free()


def test_stride_changes_small_offsets(gpu, eng):
    """Offsets cross 2^7, 2^14, 2^21 and 2^28: a 1 MiB blob repeated 300 times and more."""
    want = _stride_case(gpu, eng, [1 << 7, 1 << 14, 1 << 21, 1 << 28], 1 << 20, 60)
    assert (want[3]["len"] == 1 << 20).sum() >= 3 * 300


def test_stride_changes_large_offsets(gpu, eng):
    """Offsets cross 2^35 and 2^42 as well: a 1 GiB blob, left unwritten, repeated 4,100 times.
    (2^49 is crossed in test_gpu_walk_wide.py; varints of 9 and 10 bytes: DESIGN §4.10.)"""
    want = _stride_case(gpu, eng, [1 << 7, 1 << 14, 1 << 21, 1 << 28, 1 << 35, 1 << 42],
                        1 << 30, 40)
    assert (want[3]["len"] == 1 << 30).sum() >= 3 * 4100 and int(want[4].max()) > 1 << 42


# ---- 4. mixed depth ----------------------------------------------------------------------------
def test_mixed_depth(gpu, eng):
    pool, blobs, roots, leaves = W.mixed_depth()
    # twice in one walk, around an empty stream, so a later stream's places depend on it too
    want = W.check_host_pool(gpu, eng, pool, blobs, [roots[0], bytes(32), roots[0]], W.OK)
    one = W.chunk_records(leaves)
    two = W.chunk_records(leaves, stream=2)
    assert want[3].tobytes() == one.tobytes() + two.tobytes()
    assert want[2]["depth"] == 2 and want[2]["nnodes"] == 10


# ---- 6. independence and determinism -----------------------------------------------------------
def test_two_walks_and_two_blobs_under_one_ref(gpu, eng):
    trees, store = W.two_streams()
    roots = [t.root for t in trees]
    pool, blobs = W.pool_of(store)
    W.check_host_pool(gpu, eng, pool, blobs, roots, W.OK)
    a = [x.tobytes() for x in eng.copy_walk()]
    W.check_host_pool(gpu, eng, pool, blobs, roots, W.OK)
    assert [x.tobytes() for x in eng.copy_walk()] == a
    # a second, malformed blob under a node's ref after the good one: unused; before it: used
    n = trees[1].nodes[1][0]
    k = next(i for i in range(len(blobs)) if blobs[i]["ref"].tobytes() == n["ref"])
    bad = W.FAMILIES["padded"][0](n)
    pool2 = np.concatenate([pool, np.frombuffer(bad, dtype=np.uint8)])
    extra = W.table_of([(len(pool), len(bad), n["ref"])])
    W.check_host_pool(gpu, eng, pool2, np.concatenate([blobs, extra]), roots, W.OK)
    assert [x.tobytes() for x in eng.copy_walk()] == a
    first = np.concatenate([blobs[:k], extra, blobs[k:]])
    W.check_host_pool(gpu, eng, pool2, first, roots, W.ECORRUPT)


def test_walk_leaves_the_run_alone(gpu, eng, oracle, table):
    streams = [splitmix_array(3, 9107), np.zeros(0, np.uint8), splitmix_array(4, 30000)]
    rp, _ = _round_trip(gpu, eng, streams, 4, 64, 2)
    try:
        assert eng.chunks().tobytes() == rp.recs.tobytes()
        roots, ncounts, nodes, arena = (x.copy() for x in (rp.roots, rp.ncounts, rp.nodes,
                                                            rp.arena))
        first = np.zeros(len(rp.recs), dtype=np.uint64)
        uniq = np.zeros(eng.nunique, dtype=np.uint64)
        pack_off = np.zeros(eng.nunique + 1, dtype=np.uint64)
        assert gpu.lib().bsg_engine_copy_dedup(eng.h, first.ctypes.data, len(first),
                                               uniq.ctypes.data, pack_off.ctypes.data,
                                               len(uniq)) == 0
        assert (first.tobytes(), uniq.tobytes(), pack_off.tobytes()) == rp.dedup
        nn = np.zeros(len(nodes), dtype=gpu.TREE_NODE_DTYPE)
        ar = np.zeros(len(arena), dtype=np.uint8)
        assert gpu.lib().bsg_engine_copy_tree_nodes(eng.h, nn.ctypes.data, len(nn),
                                                    ar.ctypes.data, len(ar)) == 0
        assert nn.tobytes() == nodes.tobytes() and ar.tobytes() == arena.tobytes()
        # restore with copy_walk's records handed in from the host: the same bytes
        recs, sizes, counts = eng.copy_walk()
        rc, info, off, out = W.restore_walk(gpu, eng, rp.pbuf, rp.pool_bytes, rp.blobs, sizes)
        obuf = gpu.DeviceBuffer(len(out))
        obuf.from_host(np.full(len(out), W.FILL, dtype=np.uint8))
        eng.restore(rp.pbuf.ptr, rp.blobs, recs, obuf, off, sizes, pool_bytes=rp.pool_bytes)
        assert obuf.to_host().tobytes() == out.tobytes()
        obuf.free()
        # a later run gives the oracle's records
        buf = _run(gpu, eng, streams, 6, 64, 3)
        got = eng.chunks()
        buf.free()
        for s, d in enumerate(streams):
            want = oracle.split(table, d, bits=6, min_size=64)
            mine = got[got["stream"] == s]
            assert len(mine) == len(want) and (mine["ref"] == want["ref"]).all()
    finally:
        rp.free()


def test_walk_on_a_fresh_engine(gpu):
    e = gpu.Engine()
    try:
        assert e.walk_records_device() == 0
        rc, info = e.restore_walk(0, np.zeros(0, gpu.POOL_BLOB_DTYPE), 0, [], pool_bytes=0,
                                  out_cap=0)
        assert rc == W.ESTATE
        pool, blobs, roots, leaves = W.mixed_depth()
        W.check_host_pool(gpu, e, pool, blobs, roots, W.OK)
        # no stream at all is a valid walk
        W.check_host_pool(gpu, e, pool, blobs, [], W.OK)
    finally:
        e.close()

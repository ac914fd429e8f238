"""bsg_engine_trees at its limits: more nodes at one height than a hash batch takes
(kTreeHashBatch), more items than one tile per thread of the prefix sums' middle pass
(256 x kTreeTile), both sides of the wave-ticket switch (kTreeWaveNodes), the tallest tree there is
(below kTreeMaxHeights), chosen tree shapes, runs without a chunk, and the entry points the first
tests left out. The inputs are tree_cases.py's (64-byte windows of chosen levels back to back;
test_engine_trees_cpu.py holds each to its claim with the oracle); every Root is compared with the
C Writer's, every node list with the closed form (tree_form.check_listing) and every arena with
check_arena. The limits are read from the source, so a changed constant moves the sizes."""
import ctypes

import numpy as np
import pytest

import tree_cases as TC
import tree_form as TF
from bs_amd.synth import splitmix_array
from test_gpu_engine_trees import _run

pytestmark = pytest.mark.gpu

LIM = TC.limits()
BATCH, WAVE, TILE, SCAN = (LIM["kTreeHashBatch"], LIM["kTreeWaveNodes"], LIM["kTreeTile"],
                           LIM["scan_items"])


class Result:
    """One bsg_engine_trees call, split by stream."""

    def __init__(self, eng):
        self.roots, self.counts, self.nodes, self.arena = eng.trees()
        recs, rc = eng.chunks(), eng.counts()
        cs = np.concatenate([[0], np.cumsum(rc)]).astype(np.int64)
        ns = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        assert ns[-1] == len(self.nodes)
        self.recs = [recs[cs[s]:cs[s + 1]] for s in range(len(rc))]
        self.snodes = [self.nodes[ns[s]:ns[s + 1]] for s in range(len(rc))]
        for s, part in enumerate(self.snodes):  # stream-major
            assert (part["stream"] == s).all()

    def same_as(self, other):
        return all(getattr(self, f).tobytes() == getattr(other, f).tobytes()
                   for f in ("roots", "counts", "nodes", "arena"))


def _sha_many(oracle, table):
    """SHA-256 of many pieces of one buffer with the oracle's C code on 16 threads: each piece a
    stream of a split that cannot cut (Bits 33), whose one record carries the piece's ref."""
    def f(buf, starts, lens):
        ch, counts = oracle.split_streams(table, buf, starts, lens, bits=33, min_size=64,
                                          threads=16)
        assert (counts == 1).all() and (ch["len"] == np.asarray(lens)).all()
        return ch["ref"]
    return f


def _check(oracle, table, res, streams, bits, fanout, node_by_node=True):
    """Roots against the C Writer, per-stream counts and the per-height histogram against the
    closed form, the arena's gaps and size; node by node: every listed node (check_listing)."""
    assert len(res.roots) == len(streams)
    sha = _sha_many(oracle, table)
    for s, d in enumerate(streams):
        want = oracle.writer_root(table, d, bits=bits, min_size=64, fanout=fanout)[0]
        assert res.roots[s].tobytes() == want, s
        lv = res.recs[s]["level"]
        assert int(res.counts[s]) == int(TF.height_histogram(lv, fanout, 40).sum()), s
        if node_by_node:
            TF.check_listing(res.recs[s], fanout, want, res.snodes[s], res.arena, sha)
    hist = TC.run_histogram([r["level"] for r in res.recs], fanout)
    if len(res.nodes):
        assert np.bincount(res.nodes["height"], minlength=len(hist)).tolist() == hist.tolist()
    TF.check_arena(res.nodes, res.arena)
    return hist


def _planned_run(gpu, oracle, table, eng, level_lists, bits, fanout, node_by_node=True):
    streams = TC.streams_of(table, bits, level_lists)
    buf = _run(gpu, eng, streams, bits, 64, fanout)
    try:
        res = Result(eng)
        for r, lv in zip(res.recs, level_lists):  # the run is the planned one
            assert len(r) == len(lv) and (r["level"] == np.asarray(lv)).all()
        hist = _check(oracle, table, res, streams, bits, fanout, node_by_node)
    finally:
        buf.free()
    return res, hist


# ---- a. shape families ------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["declared", "descending", "shuffled"])
@pytest.mark.parametrize("fanout", [1, 2, 3, 8])
def test_shape_families(gpu, oracle, table, fanout, order):
    """Highest level first, in the middle and last, stairs, equal consecutive q, one and two
    chunks, with levels at k f - 1, k f and k f + 1, empty streams in between, in one run."""
    fams = TC.family_levels(fanout, order)
    lists = [lv for _, lv in fams]
    if order == "declared":
        TC.assert_family_properties(fams, fanout)
    eng = gpu.Engine()
    try:
        res, hist = _planned_run(gpu, oracle, table, eng, lists, TC.FAMILY_BITS, fanout)
    finally:
        eng.close()
    # streams of different Root heights, and an unpruned single-child node above height 0
    R = [int(n["height"][-1]) for n in res.snodes if len(n)]
    assert len(hist) == max(R) + 1 and min(R) == 0 and len(set(R)) >= 3
    single = 0
    for lv in lists:
        r, k = TF.stream_heights(lv, fanout)
        for h in range(1, r + 1):  # a close at h right after a close at h: one child
            c = np.nonzero(k > h - 1)[0]
            single += int((np.diff(np.nonzero(k[c] > h)[0]) == 1).sum())
    assert single >= 1


# ---- b. exact thresholds ------------------------------------------------------------------------
@pytest.mark.parametrize("nodes0", [WAVE, WAVE + 1])
def test_wave_ticket_switch(gpu, oracle, table, nodes0):
    lists = TC.node_threshold_run(nodes0, nodes0)
    assert TC.run_histogram(lists, TC.THRESHOLD_FANOUT)[0] == nodes0
    assert 0 < TF.height_histogram(lists[0], TC.THRESHOLD_FANOUT, 1)[0] < WAVE
    eng = gpu.Engine()
    try:
        _planned_run(gpu, oracle, table, eng, lists, TC.THRESHOLD_BITS, TC.THRESHOLD_FANOUT)
    finally:
        eng.close()


@pytest.mark.parametrize("nodes0", [BATCH, BATCH + 1, BATCH + 2, 2 * BATCH + 1])
def test_hash_batch_border(gpu, oracle, table, nodes0):
    """Height 0 of the run fills one hash batch exactly, spills one and two nodes into a second,
    and one into a third; heights 1 and 2 hold thousands of nodes whose children lie on both
    sides of the border. Every node is checked."""
    f = TC.THRESHOLD_FANOUT
    lists = TC.node_threshold_run(nodes0, nodes0, (3000, 1500))
    hist = TC.run_histogram(lists, f)
    assert hist[0] == nodes0 and len(hist) == 4 and (hist[1:3] >= 1000).all()
    assert 0 < TF.height_histogram(lists[0], f, 1)[0] < BATCH  # the border: inside the last stream
    eng = gpu.Engine()
    try:
        _planned_run(gpu, oracle, table, eng, lists, TC.THRESHOLD_BITS, f)
    finally:
        eng.close()


@pytest.mark.parametrize("chunks", [TILE - 1, TILE, TILE + 1])
def test_scan_one_tile(gpu, oracle, table, chunks):
    lists = TC.chunk_threshold_run(chunks, chunks, 600)
    assert sum(len(x) for x in lists) == chunks and 0 < len(lists[0]) < TILE - 1
    eng = gpu.Engine()
    try:
        _planned_run(gpu, oracle, table, eng, lists, TC.THRESHOLD_BITS, TC.THRESHOLD_FANOUT)
    finally:
        eng.close()


@pytest.mark.parametrize("chunks", [SCAN - 1, SCAN, SCAN + 1])
def test_scan_middle_pass_second_step(gpu, oracle, table, chunks):
    """The run's chunks fill 256 tiles of the prefix sums less one item, exactly, and one more:
    with the 257th tile k_sum_mid sums two tiles per thread. Roots, per-stream counts,
    the per-height histogram and the arena's gaps (32 MiB per run: not node by node)."""
    lists = TC.chunk_threshold_run(chunks, chunks, 6000)
    assert sum(len(x) for x in lists) == chunks and 0 < len(lists[0]) < SCAN - 1
    assert (chunks + TILE - 1) // TILE == (257 if chunks > SCAN else 256)
    eng = gpu.Engine()
    try:
        res, hist = _planned_run(gpu, oracle, table, eng, lists, TC.THRESHOLD_BITS,
                                 TC.THRESHOLD_FANOUT, node_by_node=False)
        assert hist[0] == 6000 and len(hist) == 4
    finally:
        eng.close()


# ---- c. one random wide tree --------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide(oracle, table):
    """12 MiB at Bits 2 / MinSize 64 / fanout 1 and the oracle's records and Root of it."""
    d = splitmix_array(21, 12 << 20)
    recs = oracle.split(table, d, bits=2, min_size=64, with_refs=False)
    assert int((recs["level"] >= 1).sum()) + 1 > BATCH  # height-0 nodes, from the oracle
    assert int((recs["level"] >= 2).sum()) + 1 > WAVE
    return d, recs, oracle.writer_root(table, d, bits=2, min_size=64, fanout=1)[0]


@pytest.mark.parametrize("what", ["root_counts_arena", "node_by_node"])
def test_wide_random_tree(gpu, oracle, table, wide, what):
    """187,813 chunks, heights 0 and 1 past one hash batch. Two cases, each a run of its own, to
    stay under the tree tests' time ceiling: the Root, the count, the per-height histogram and
    the arena's gaps; every one of the 186,929 nodes against the closed form.
    Measured on an MI355X box: 0.79 s and 0.93 s, against 0.50 s for test_past_2_28 in the same
    session, so both cases are still above that ceiling. The time is in the run and bsg_engine_trees
    themselves (Bits 2 makes a candidate of every fourth byte, 3 M for 12 MiB, and the tree has
    18 heights), not in the checks: checking all nodes adds 0.14 s. One case doing both took
    1.07 s."""
    d, want, root = wide
    eng = gpu.Engine()
    try:
        buf = _run(gpu, eng, [d], 2, 64, 1)
        res = Result(eng)
        assert len(res.recs[0]) == len(want) and (res.recs[0]["level"] == want["level"]).all()
        assert res.roots[0].tobytes() == root
        if what == "node_by_node":
            TF.check_listing(res.recs[0], 1, root, res.snodes[0], res.arena,
                             _sha_many(oracle, table))
        else:
            hist = TC.run_histogram([want["level"]], 1)
            assert hist[0] > BATCH and len(hist) == int(want["level"][:-1].max()) + 1
            assert int(res.counts[0]) == int(hist.sum()) == len(res.nodes)
            assert np.bincount(res.nodes["height"]).tolist() == hist.tolist()
            TF.check_arena(res.nodes, res.arena)
        buf.free()
    finally:
        eng.close()


# ---- d. the tallest tree ------------------------------------------------------------------------
def test_tallest_tree(gpu, oracle, table):
    """Bits 1 (0 means the default 13) and fanout 1: a zero hash is level 31, so H = 32, the most
    TrailingZeros32 can give; next to it a stream of three heights and an empty one."""
    lists = [[0, 2, 0, 1], TC.TALL_LEVELS, [], [31]]
    R, _ = TF.stream_heights(TC.TALL_LEVELS, 1)
    assert R + 1 == 32 <= LIM["kTreeMaxHeights"]
    eng = gpu.Engine()
    try:
        res, hist = _planned_run(gpu, oracle, table, eng, lists, TC.TALL_BITS, 1)
        assert len(hist) == 32 and int(res.snodes[1]["height"][-1]) == 31
        assert [int(n["height"][-1]) for n in (res.snodes[0], res.snodes[3])] == [2, 0]
    finally:
        eng.close()


# ---- e. no chunks -------------------------------------------------------------------------------
def test_runs_without_chunks_and_stale_buffers(gpu, oracle, table):
    """Runs of one and of three empty streams; then, on the same engine, the family run, a tall
    run, a shallow one, an empty one and the tall one again: each as on a fresh engine (what an
    earlier, larger run left in rmax, close, meta and hoff is not read)."""
    fam = [lv for _, lv in TC.family_levels(2)]
    tall = [[0, 2, 0, 1], TC.TALL_LEVELS, [], [31]]
    shallow = [[0, 0, 0], [], [1]]
    fresh = {}
    for name, lists, bits, fan in (("fam", fam, TC.FAMILY_BITS, 2), ("tall", tall, TC.TALL_BITS, 1),
                                   ("shallow", shallow, TC.TALL_BITS, 1)):
        eng = gpu.Engine()
        try:
            fresh[name] = _planned_run(gpu, oracle, table, eng, lists, bits, fan)[0]
        finally:
            eng.close()
    assert len(fresh["shallow"].nodes) == 2

    def empty(eng, ns):
        buf = _run(gpu, eng, [np.zeros(0, dtype=np.uint8)] * ns, TC.FAMILY_BITS, 64, 2)
        nn, nb = ctypes.c_uint64(7), ctypes.c_uint64(7)
        assert gpu.lib().bsg_engine_trees(eng.h, ctypes.byref(nn), ctypes.byref(nb)) == 0
        assert nn.value == 0 and nb.value == 0
        roots, counts, nodes, arena = eng.trees()
        assert len(nodes) == 0 and len(arena) == 0
        assert roots.shape == (ns, 32) and not roots.any() and not counts.any()
        buf.free()

    eng = gpu.Engine()
    try:
        empty(eng, 1)
        empty(eng, 3)
        assert _planned_run(gpu, oracle, table, eng, fam, TC.FAMILY_BITS, 2)[0].same_as(fresh["fam"])
        assert _planned_run(gpu, oracle, table, eng, tall, TC.TALL_BITS, 1)[0].same_as(fresh["tall"])
        assert _planned_run(gpu, oracle, table, eng, shallow, TC.TALL_BITS, 1)[0].same_as(
            fresh["shallow"])
        empty(eng, 3)
        assert _planned_run(gpu, oracle, table, eng, tall, TC.TALL_BITS, 1)[0].same_as(fresh["tall"])
    finally:
        eng.close()


# ---- f. entry points ------------------------------------------------------------------------------
def test_device_pointers_and_copy_roots(gpu, oracle, table):
    L = gpu.lib()
    lists = [lv for _, lv in TC.family_levels(3)]
    ns = len(lists)
    eng = gpu.Engine()
    try:
        assert not L.bsg_engine_tree_nodes_device(eng.h)  # no tree yet
        streams = TC.streams_of(table, TC.FAMILY_BITS, lists)
        buf = _run(gpu, eng, streams, TC.FAMILY_BITS, 64, 3)
        assert not L.bsg_engine_roots_device(eng.h)       # a finished run, bsg_engine_trees not called
        res = Result(eng)
        _check(oracle, table, res, streams, TC.FAMILY_BITS, 3)

        def d2h(ptr, n):
            assert ptr
            out = np.full(n, 0xEE, dtype=np.uint8)
            assert L.bsg_memcpy(0, out.ctypes.data, ptr, n, 1) == 0
            return out

        assert d2h(L.bsg_engine_tree_nodes_device(eng.h), 56 * len(res.nodes)).tobytes() == \
            res.nodes.tobytes()
        assert d2h(L.bsg_engine_tree_arena_device(eng.h), len(res.arena)).tobytes() == \
            res.arena.tobytes()
        assert d2h(L.bsg_engine_roots_device(eng.h), 32 * ns).tobytes() == res.roots.tobytes()

        # node_counts: the closed form's; without it only the Roots are written
        counts = np.full(ns, 0xEEEE, dtype=np.uint64)
        roots = np.full(32 * ns, 0xEE, dtype=np.uint8)
        assert L.bsg_engine_copy_roots(eng.h, roots.ctypes.data,
                                       counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                       ns) == 0
        assert roots.tobytes() == res.roots.tobytes()
        assert counts.tolist() == [int(TF.height_histogram(lv, 3, 40).sum()) for lv in lists]
        assert counts.sum() == len(res.nodes)
        # fewer streams than the run's: no more than asked is written; more: BSG_EINVAL
        k = 5
        assert res.roots[k].any() and counts[k]
        counts2 = np.full(ns, 0xEEEE, dtype=np.uint64)
        roots2 = np.full(32 * ns, 0xEE, dtype=np.uint8)
        assert L.bsg_engine_copy_roots(eng.h, roots2.ctypes.data,
                                       counts2.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                       k) == 0
        assert roots2[:32 * k].tobytes() == res.roots[:k].tobytes() and (roots2[32 * k:] == 0xEE).all()
        assert (counts2[:k] == counts[:k]).all() and (counts2[k:] == 0xEEEE).all()
        assert L.bsg_engine_copy_roots(eng.h, roots2.ctypes.data, None, 0) == 0
        assert (roots2[32 * k:] == 0xEE).all()
        assert L.bsg_engine_copy_roots(eng.h, roots2.ctypes.data, None, ns + 1) == -22

        eng.hash(buf.ptr, [0], [64])
        eng.finish()
        assert not L.bsg_engine_tree_nodes_device(eng.h)
        assert not L.bsg_engine_tree_arena_device(eng.h)
        assert not L.bsg_engine_roots_device(eng.h)
        buf.free()
    finally:
        eng.close()

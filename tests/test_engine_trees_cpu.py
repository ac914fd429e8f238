"""bsg_engine_trees without a GPU: the closed form the kernels follow (tests/tree_form.py) against
the oracle's literal TreeBuilder (py_tree_root), the node record's layout, and the null-argument
errors."""
import ctypes
import hashlib

import numpy as np
import pytest

import planting as P
import tree_cases as TC
import tree_form as TF
from bs_amd.synth import splitmix_array

FANOUTS = (1, 2, 3, 8)


def _sequences(fanout: int, count: int):
    """Seeded (length, level) sequences: up to 200 chunks, levels up to 20, lengths that put
    offsets on both sides of the 1-, 2- and 3-byte varint edges."""
    rng = np.random.default_rng(1000 + fanout)
    for k in range(count):
        n = int(rng.integers(1, 201)) if k % 7 else int(rng.integers(1, 5))
        top = int(rng.integers(0, 21))
        # geometric levels (as trailing zeros are), capped, with a few forced high ones
        lv = np.minimum(rng.geometric(0.5, n) - 1, top)
        if k % 3 == 0:
            lv[rng.integers(0, n, max(1, n // 16))] = top
        if k % 4 == 1:
            lv[-1] = 20  # the last chunk alone reaches the top: the single-child prune
        ln = rng.integers(1, 120, n)
        if k % 5 == 0:
            ln[rng.integers(0, n, 2)] = rng.integers(16_000, 40_000, 2)
        yield [int(x) for x in ln], [int(x) for x in lv]


@pytest.mark.parametrize("fanout", FANOUTS)
def test_closed_form_matches_tree_builder(oracle, fanout):
    rng = np.random.default_rng(fanout)
    seen_prune = seen_deep = 0
    for lens, levels in _sequences(fanout, 150):
        data = [rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for ln in lens]
        store = {}
        root = oracle.py_tree_root(list(zip(data, levels)), fanout=fanout, store=store)
        want = TF.walk(oracle, store, root)
        chunks = [(hashlib.sha256(d).digest(), len(d), lv) for d, lv in zip(data, levels)]
        got_root, nodes = TF.closed_form(chunks, fanout)
        assert got_root == root
        assert {nd["ref"]: (nd["blob"], nd["height"]) for nd in nodes} == want
        assert len(nodes) == len(want)  # no blob listed twice
        # listed order: height ascending, then offset ascending; the Root last
        keys = [(nd["height"], nd["offset"]) for nd in nodes]
        assert keys == sorted(keys) and nodes[-1]["ref"] == root
        # the kernels' count of the same rule: Root height and closes per chunk
        R, k = TF.kernel_heights(levels, fanout)
        assert R == nodes[-1]["height"] and sum(k) == len(nodes)
        for h in range(R + 1):
            assert [i for i, ki in enumerate(k) if ki > h] == \
                [nd["close"] for nd in nodes if nd["height"] == h]
        seen_prune += max(lv // fanout for lv in levels) > R
        seen_deep += R >= 2
    # the prune and trees of three and more heights were exercised
    assert seen_prune >= 5 and seen_deep >= 5, (seen_prune, seen_deep)


def test_closed_form_empty_and_single():
    assert TF.closed_form([], 8) == (bytes(32), [])
    ref = hashlib.sha256(b"x" * 10).digest()
    root, nodes = TF.closed_form([(ref, 10, 5)], 1)  # its own level is pruned away
    assert len(nodes) == 1 and nodes[0]["height"] == 0
    assert nodes[0]["blob"] == b"\x12\x22\x0a\x20" + ref + b"\x20\x0a"  # one leaf, no offset
    assert root == hashlib.sha256(nodes[0]["blob"]).digest()


def _same_nodes(a, b):
    assert a[0] == b[0] and len(a[1]) == len(b[1])
    for x, y in zip(a[1], b[1]):
        assert x == y


@pytest.mark.parametrize("fanout", FANOUTS)
def test_linear_closed_form_equals_first_statement(fanout):
    """closed_form with one pointer per height against the quadratic statement it replaces, on
    the sequences above and on 300 short lists with many equal and many high levels."""
    rng = np.random.default_rng(50 + fanout)
    cases = list(_sequences(fanout, 60))
    for _ in range(300):
        n = int(rng.integers(1, 40))
        cases.append(([int(x) for x in rng.integers(1, 300, n)],
                      [int(x) for x in rng.integers(0, rng.integers(1, 33), n)]))
    for lens, levels in cases:
        chunks = [(hashlib.sha256(b"%d-%d" % (i, ln)).digest(), ln, lv)
                  for i, (ln, lv) in enumerate(zip(lens, levels))]
        _same_nodes(TF.closed_form(chunks, fanout), TF._closed_form_slow(chunks, fanout))


def _listing_of(chunks, fanout):
    refs = np.frombuffer(b"".join(c[0] for c in chunks), dtype=np.uint8).reshape(-1, 32)
    return TF.listing(refs, [c[1] for c in chunks], [c[2] for c in chunks], fanout)


def _assert_listing_is_closed_form(chunks, fanout):
    root, nodes = TF.closed_form(chunks, fanout)
    got = _listing_of(chunks, fanout)
    assert len(got["height"]) == len(nodes)
    for f in ("height", "offset", "size", "close"):
        assert got[f].tolist() == [nd[f] for nd in nodes], f
    assert got["blob_len"].tolist() == [len(nd["blob"]) for nd in nodes]
    assert got["buf"].tobytes() == b"".join(nd["blob"] for nd in nodes)
    assert got["ref"].tobytes() == b"".join(nd["ref"] for nd in nodes)
    assert got["blob_start"].tolist() == list(np.cumsum([0] + [len(nd["blob"]) for nd in nodes])[:-1])
    return root, nodes, got


@pytest.mark.parametrize("fanout", FANOUTS)
def test_listing_equals_closed_form(fanout):
    """listing(), the closed form in numpy that check_listing compares an engine's nodes with,
    gives closed_form()'s nodes: order, heights, ranges, blob bytes and refs. Lengths put offsets
    and sizes on both sides of the 1- to 4-byte varint edges."""
    for k, (lens, levels) in enumerate(_sequences(fanout, 80)):
        if k % 9 == 0:
            lens[0] = 1 << 21
        chunks = [(hashlib.sha256(b"%d" % i).digest(), ln, lv)
                  for i, (ln, lv) in enumerate(zip(lens, levels))]
        _assert_listing_is_closed_form(chunks, fanout)
    assert len(TF.listing(np.zeros((0, 32), np.uint8), [], [], fanout)["height"]) == 0


def test_limits_read_from_source():
    lim = TC.limits()
    assert lim["kTreeHashBatch"] == 65535       # bsg_engine_hash takes no more blobs
    assert lim["kTreeWaveNodes"] < lim["kTreeHashBatch"]
    assert lim["kTreeTile"] == 256 * 8           # k_sum_part: 256 threads x 8 items
    # levels are at most 32 (TrailingZeros32), so q <= 32 and a tree has at most 33 heights;
    # kcnt is a uint8_t
    assert 33 <= lim["kTreeMaxHeights"] - 1 and lim["kTreeMaxHeights"] <= 255


def _planned(oracle, table, bits, level_lists):
    """The streams of the level lists; the oracle cuts each into exactly the planned chunks."""
    streams = TC.streams_of(table, bits, level_lists)
    for d, lv in zip(streams, level_lists):
        r = oracle.split(table, d, bits=bits, min_size=64, with_refs=False)
        assert len(r) == len(lv) and (r["len"] == 64).all()
        assert (r["level"] == np.asarray(lv)).all()
    return streams


def test_level_windows_pool(table):
    pool = P.level_windows(table, 1, range(32))
    for lv, wins in pool.items():
        assert len(wins) >= 2 and not (wins[0] == wins[1]).all()
        for w in wins:
            assert int(P._tz(P.window_hashes(table, w, 63, 64))[0]) == 1 + lv


@pytest.mark.parametrize("fanout", FANOUTS)
def test_family_streams_hold_their_claims(oracle, table, fanout):
    """The shape families of test_gpu_tree_limits.py: the oracle cuts each stream into the
    planned levels, closed_form's Root is the C Writer's and its nodes are the walk through
    py_tree_root's store; listing() agrees; the run has what it is there for."""
    fams = TC.family_levels(fanout)
    streams = _planned(oracle, table, TC.FAMILY_BITS, [lv for _, lv in fams])
    for order in ("descending", "shuffled"):
        assert sorted(map(str, TC.family_levels(fanout, order))) == sorted(map(str, fams))
    single_child = 0
    for (name, lv), d in zip(fams, streams):
        recs = oracle.split(table, d, bits=TC.FAMILY_BITS, min_size=64)
        chunks = [(r["ref"].tobytes(), int(r["len"]), int(r["level"])) for r in recs]
        root, nodes, got = _assert_listing_is_closed_form(chunks, fanout)
        assert root == oracle.writer_root(table, d, bits=TC.FAMILY_BITS, min_size=64,
                                          fanout=fanout)[0], name
        data = bytes(d)
        store = {}
        pieces = [(data[64 * i:64 * i + 64], x) for i, x in enumerate(lv)]
        assert oracle.py_tree_root(pieces, fanout=fanout, store=store) == root
        assert {nd["ref"]: (nd["blob"], nd["height"]) for nd in nodes} == \
            TF.walk(oracle, store, root)
        single_child += sum(nd["height"] >= 1 and nd["nkids"] == 1 for nd in nodes)
    assert single_child >= 1
    TC.assert_family_properties(fams, fanout)


def test_family_levels_sit_on_both_sides_of_a_multiple():
    for fanout in FANOUTS:
        lv = {x for _, l in TC.family_levels(fanout) for x in l}
        for k in (1, 2, 3):
            assert {k * fanout - 1, k * fanout} <= lv, (fanout, k)
        assert {fanout + 1, 2 * fanout + 1} <= lv


def _threshold_runs():
    lim = TC.limits()
    B, W, S = lim["kTreeHashBatch"], lim["kTreeWaveNodes"], lim["scan_items"]
    for n0 in (W, W + 1):
        yield "nodes", n0, TC.node_threshold_run(n0, n0)
    for n0 in (B, B + 1, B + 2, 2 * B + 1):
        yield "nodes", n0, TC.node_threshold_run(n0, n0, (3000, 1500))
    for m in (lim["kTreeTile"] - 1, lim["kTreeTile"], lim["kTreeTile"] + 1):
        yield "chunks", m, TC.chunk_threshold_run(m, m, 600)
    for m in (S - 1, S, S + 1):
        yield "chunks", m, TC.chunk_threshold_run(m, m, 6000)


def test_threshold_runs_hold_their_claims(oracle, table):
    """Every threshold run has exactly the planned chunks; its height-0 node count or chunk
    count is the limit it is named for, inside a stream; listing()'s Root is the C Writer's."""
    f = TC.THRESHOLD_FANOUT
    for kind, want, lists in _threshold_runs():
        streams = _planned(oracle, table, TC.THRESHOLD_BITS, lists)
        hist = TC.run_histogram(lists, f)
        if kind == "nodes":
            assert hist[0] == want
            if want > 60000:
                assert len(hist) == 4 and (hist[1:3] >= 1000).all()  # a few thousand
        else:
            assert sum(len(x) for x in lists) == want
        assert len(lists) >= 2 and 0 < len(lists[0]) < want and len(lists[-1]) > 0
        for d, lv in zip(streams, lists):
            if len(lv) == 0 or (want > 70000 and kind == "nodes" and want != 65536):
                continue  # Roots of three sizes per kind are enough here; the GPU test has all
            recs = oracle.split(table, d, bits=TC.THRESHOLD_BITS, min_size=64)
            got = TF.listing(recs["ref"], recs["len"], recs["level"], f)
            assert got["ref"][-1].tobytes() == \
                oracle.writer_root(table, d, bits=TC.THRESHOLD_BITS, min_size=64, fanout=f)[0]
            assert len(got["height"]) == int(TF.height_histogram(lv, f, 8).sum())


def test_wide_random_tree_listing(oracle, table):
    """12 MiB at Bits 2 / fanout 1: more than kTreeHashBatch nodes at height 0 and at height 1.
    listing() gives the C Writer's Root over its 186,929 nodes."""
    d = splitmix_array(21, 12 << 20)
    recs = oracle.split(table, d, bits=2, min_size=64)
    assert len(recs) == 187_813 and int(recs["level"].max()) == 17
    assert int((recs["level"] >= 1).sum()) == 93_617
    got = TF.listing(recs["ref"], recs["len"], recs["level"], 1)

    def sha_many(buf, starts, lens):  # as test_gpu_tree_limits.py hashes: the oracle's C code
        ch, counts = oracle.split_streams(table, buf, starts, lens, bits=33, min_size=64, threads=4)
        assert (counts == 1).all()
        return ch["ref"]
    fast = TF.listing(recs["ref"], recs["len"], recs["level"], 1, sha_many)
    assert fast["ref"].tobytes() == got["ref"].tobytes()
    assert fast["buf"].tobytes() == got["buf"].tobytes()
    assert len(got["height"]) == 186_929
    assert int((got["height"] == 0).sum()) > TC.limits()["kTreeHashBatch"]
    assert got["ref"][-1].tobytes() == oracle.writer_root(table, d, bits=2, min_size=64,
                                                          fanout=1)[0]


def test_tallest_tree_stream(oracle, table):
    streams = _planned(oracle, table, TC.TALL_BITS, [TC.TALL_LEVELS])
    recs = oracle.split(table, streams[0], bits=TC.TALL_BITS, min_size=64)
    chunks = [(r["ref"].tobytes(), int(r["len"]), int(r["level"])) for r in recs]
    root, nodes, got = _assert_listing_is_closed_form(chunks, 1)
    assert nodes[-1]["height"] + 1 == 32 <= TC.limits()["kTreeMaxHeights"]
    assert root == oracle.writer_root(table, streams[0], bits=TC.TALL_BITS, min_size=64,
                                      fanout=1)[0]


def test_check_listing_and_arena_notice(oracle, table):
    """check_listing and check_arena fail on a wrong height, a swapped pair, a flipped blob byte,
    a wrong ref and a dirty gap (they are the GPU tests' only judge of a node list)."""
    from bs_amd import bsgpu
    d = TC.streams_of(table, TC.FAMILY_BITS, [dict(TC.family_levels(2))["equal_q"]])[0]
    recs = oracle.split(table, d, bits=TC.FAMILY_BITS, min_size=64)
    want = TF.listing(recs["ref"], recs["len"], recs["level"], 2)
    n = len(want["height"])
    nodes = np.zeros(n, dtype=bsgpu.TREE_NODE_DTYPE)
    al = (want["blob_len"] + 15) & ~15
    nodes["blob_off"] = np.cumsum(al) - al
    nodes["blob_len"], nodes["height"], nodes["ref"] = want["blob_len"], want["height"], want["ref"]
    arena = np.zeros(int(al.sum()), dtype=np.uint8)
    for i in range(n):
        o, s, ln = int(nodes["blob_off"][i]), int(want["blob_start"][i]), int(want["blob_len"][i])
        arena[o:o + ln] = want["buf"][s:s + ln]
    root = want["ref"][-1].tobytes()
    TF.check_listing(recs, 2, root, nodes, arena)
    TF.check_arena(nodes, arena)

    def broken(fn):
        nd, ar = nodes.copy(), arena.copy()
        fn(nd, ar)
        with pytest.raises(AssertionError):
            TF.check_listing(recs, 2, root, nd, ar)
            TF.check_arena(nd, ar)

    def swap(nd, ar):
        nd[[0, 1]] = nd[[1, 0]]

    def height(nd, ar):
        nd["height"][n - 1] += 1

    def byte(nd, ar):
        ar[int(nd["blob_off"][2]) + 5] ^= 1

    def ref(nd, ar):
        nd["ref"][1, 0] ^= 1

    def gap(nd, ar):
        ar[int(nd["blob_off"][0]) + int(nd["blob_len"][0])] = 7

    assert int(nodes["blob_len"][0]) % 16  # there is a gap after blob 0
    for fn in (swap, height, byte, ref, gap):
        broken(fn)
    with pytest.raises(AssertionError):
        TF.check_listing(recs, 2, bytes(32), nodes, arena)
    with pytest.raises(AssertionError):
        TF.check_arena(nodes, np.concatenate([arena, np.zeros(16, np.uint8)]))


def test_tree_node_layout():
    from bs_amd import bsgpu

    class TreeNode(ctypes.Structure):
        _fields_ = [("blob_off", ctypes.c_uint64), ("blob_len", ctypes.c_uint32),
                    ("stream", ctypes.c_uint32), ("height", ctypes.c_uint32),
                    ("reserved", ctypes.c_uint32), ("ref", ctypes.c_uint8 * 32)]
    assert ctypes.sizeof(TreeNode) == 56
    assert bsgpu.TREE_NODE_DTYPE.itemsize == 56
    for name, _ in TreeNode._fields_:
        assert bsgpu.TREE_NODE_DTYPE.fields[name][1] == getattr(TreeNode, name).offset


def test_trees_null_arguments():
    from bs_amd import bsgpu
    L = bsgpu.lib()
    a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert L.bsg_engine_trees(None, ctypes.byref(a), ctypes.byref(b)) == -22
    buf = np.zeros(64, dtype=np.uint8)
    assert L.bsg_engine_copy_roots(None, buf.ctypes.data, None, 1) == -22
    assert L.bsg_engine_copy_tree_nodes(None, buf.ctypes.data, 1, buf.ctypes.data, 1) == -22
    assert not L.bsg_engine_tree_nodes_device(None)
    assert not L.bsg_engine_tree_arena_device(None)
    assert not L.bsg_engine_roots_device(None)

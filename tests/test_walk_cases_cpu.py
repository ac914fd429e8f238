"""The model of bsg_engine_walk (walk_cases.py) held to the oracle, without a GPU: it accepts
every tree oracle.py_tree_root builds and gives the chunks back as records, it refuses every
mutation family with the status the family predicts, and its records, concatenated, are what the
C++ split::Reader reads from the same store."""
import numpy as np
import pytest

import walk_cases as W
from bs_amd.synth import splitmix_array
from conftest import load_json
from oracle import oracle as O

FANOUTS = (1, 2, 3, 8)
COUNTS = (0, 1, 2, 3, 7, 50, 400)


def _accepts(chunks, root, store, fanout):
    pool, blobs = W.pool_of(store)
    rc, status, info, recs, sizes, counts = W.run_model(pool, blobs, [root])
    assert rc == W.OK and status.tolist() == [W.OK], (rc, info)
    want = W.chunk_records([c for c, _ in chunks])
    assert recs.tobytes() == want.tobytes()
    assert sizes.tolist() == [sum(len(c) for c, _ in chunks)] and counts.tolist() == [len(chunks)]
    assert info["nnodes"] == W.reachable_nodes(store, root)
    assert info["nrecs"] == len(chunks) and info["bytes"] == int(sizes[0])
    return pool, blobs, recs


@pytest.mark.parametrize("fanout", FANOUTS)
def test_model_accepts_oracle_trees(fanout):
    for n in COUNTS:
        data, chunks, root, store = W.oracle_tree(7, n, fanout)
        assert (root == bytes(32)) == (n == 0)
        _accepts(chunks, root, store, fanout)


def test_model_accepts_fixture_streams(oracle, table):
    cases = load_json("tree_root_variants.json")["cases"]
    assert len(cases) == 5
    for c in cases:
        data = splitmix_array(c["seed"], c["length"])
        ch = oracle.split(table, data, bits=c["bits"], min_size=c["min_size"])
        raw = data.tobytes()
        chunks = [(raw[int(r["offset"]):int(r["offset"]) + int(r["len"])], int(r["level"]))
                  for r in ch]
        store = {}
        root = O.py_tree_root(chunks, fanout=c["fanout"], store=store)
        assert root.hex() == c["root_nonempty"], c["name"]
        _accepts(chunks, root, store, c["fanout"])


def test_strict_parser_is_the_canonical_form():
    """parse_node accepts a node's bytes exactly when re-encoding its fields gives them back."""
    trees, _ = W.two_streams()
    for t in trees:
        for lv in t.nodes:
            for n in lv:
                kind, kids, off, size = W.parse_node(n["bytes"])
                assert (kind, kids, off, size) == (n["kind"], n["kids"], n["offset"], n["size"])
                assert W.encode(n) == n["bytes"]


@pytest.mark.parametrize("name", sorted(W.FAMILIES))
def test_model_refuses_every_family(name):
    for where in W.WHERE:
        for stream in (0, 1):
            pool, blobs, roots, want = W.mutated(name, where, stream)
            rc, status, info, recs, sizes, counts = W.run_model(pool, blobs, roots)
            other = 1 - stream
            assert rc == want and status[stream] == want and status[other] == W.OK, \
                (name, where, stream, rc, status)
            assert info["bad_stream"] == stream and recs is None and info["nrecs"] == 0


def test_model_missing_and_ranking():
    trees, store = W.two_streams()
    roots = [t.root for t in trees]
    leaf = trees[1].nodes[2][4]["kids"][1][0]
    for gone in (trees[1].root, trees[1].nodes[1][1]["ref"], leaf):
        s = {r: b for r, b in store.items() if r != gone}
        rc, status, info, *_ = W.run_model(*W.pool_of(s), roots)
        assert rc == W.ENOTFOUND and status.tolist() == [W.OK, W.ENOTFOUND]
    # a missing child and a malformed node in one stream: not found; one stream of each: not found
    s = {r: b for r, b in store.items() if r != leaf}
    s[trees[1].nodes[2][0]["ref"]] = W.FAMILIES["padded"][0](trees[1].nodes[2][0])
    rc, status, info, *_ = W.run_model(*W.pool_of(s), roots)
    assert rc == W.ENOTFOUND and status.tolist() == [W.OK, W.ENOTFOUND]
    s[trees[0].nodes[1][2]["ref"]] = W.FAMILIES["size0"][0](trees[0].nodes[1][2])
    rc, status, info, *_ = W.run_model(*W.pool_of(s), roots)
    assert rc == W.ENOTFOUND and status.tolist() == [W.ECORRUPT, W.ENOTFOUND]
    assert info["bad_stream"] == 0


def test_model_depth_bound_and_mixed_depth():
    rc, status, info, recs, *_ = W.run_model(*W.chain(W.WALK_MAX_DEPTH))
    assert rc == W.OK and info["depth"] == 64 and info["nnodes"] == 65 and len(recs) == 1
    rc, status, info, *_ = W.run_model(*W.chain(W.WALK_MAX_DEPTH + 1))
    assert rc == W.ECORRUPT and info["depth"] == 64 and info["nnodes"] == 65
    pool, blobs, roots, leaves = W.mixed_depth()
    rc, status, info, recs, sizes, counts = W.run_model(pool, blobs, roots)
    assert rc == W.OK and info["depth"] == 2 and info["nnodes"] == 5
    assert recs.tobytes() == W.chunk_records(leaves).tobytes()


def test_model_layout_faults():
    pool, blobs, roots, _ = W.mixed_depth()
    assert W.run_model(pool, blobs, roots, flags=1)[0] == W.EINVAL
    assert W.run_model(pool, blobs, roots, pool_bytes=len(pool) - 1)[0] == W.EINVAL
    assert W.run_model(pool, blobs, [bytes(32)] * 65536)[0] == W.EINVAL


@pytest.mark.parametrize("fanout,n", [(1, 50), (2, 400), (8, 400), (3, 7)])
def test_reader_reads_the_models_records(fanout, n):
    """Canonical trees through the C++ Reader (store/mem, PutWithRef; no kernel runs): the bytes
    it reads are the model's records, blob after blob."""
    from bs_amd import bsgpu
    data, chunks, root, store = W.oracle_tree(11, n, fanout)
    pool, blobs, recs = _accepts(chunks, root, store, fanout)
    st = bsgpu.MemStore()
    for r, b in store.items():
        st.put_ref(r, b)
    rd = bsgpu.Reader(st, root)
    assert rd.size == len(data)
    got = rd.read_all()
    rd.free()
    st.free()
    assert got == b"".join(store[r["ref"].tobytes()] for r in recs) == data


# ---- the builders of test_gpu_walk_wide.py and test_gpu_gc_wide.py -------------------------------
SMALL = ([1 << 7, 1 << 14, 1 << 21, 1 << 28], 1 << 20, 60)
LARGE = ([1 << 7, 1 << 14, 1 << 21, 1 << 28, 1 << 35, 1 << 42], 1 << 30, 40)
# (entries, the first 16 hex digits of the SHA-256 of the lens as uint64) per lane 0, 32, 63, as
# crossing_lens gave them before it took gmax
CROSSING_PINS = {
    "small": [(509, "4a4c58abc7dae640"), (445, "ef300b8aba8a7771"), (505, "565e3647c81d79f5")],
    "large": [(4457, "2e692d79cf2fd08a"), (4265, "6beb4afebd96c526"), (4451, "b9d92e7b540ca834")],
}


def test_crossing_lens_gives_what_it_gave():
    for name, (th, bmax, tail) in (("small", SMALL), ("large", LARGE)):
        for lane, (n, digest) in zip((0, 32, 63), CROSSING_PINS[name]):
            lens = W.crossing_lens(th, bmax, lane, tail)
            assert len(lens) == n
            assert W.sha(np.array(lens, dtype=np.uint64).tobytes()).hex()[:16] == digest
            assert lens == W.crossing_lens(th, bmax, lane, tail, 1 << 20)


@pytest.mark.parametrize("lane", [0, 32, 63])
def test_crossing_lens_across_2_49(lane):
    """The seventh threshold needs 2^19 - 2^12 leaves of 1 GiB in one stretch: past gmax's
    default, and with the stretches before it more than 2^19 entries in the node."""
    th = LARGE[0] + [1 << 49]
    with pytest.raises(AssertionError):
        W.crossing_lens(th, 1 << 30, lane, 40)
    lens = W.crossing_lens(th, 1 << 30, lane, 40, gmax=1 << 20)
    before = W.crossing_lens(*LARGE[:2], lane, 0)  # up to 2^42: the same stretches
    assert lens[:len(before)] == before
    ch = W.stride_lanes(lens)
    assert len(ch) == 8 and ch[0] == (1, 1) and all(ln == lane for _, ln in ch[1:])
    offs = np.cumsum([0] + lens[:-1], dtype=np.uint64)
    assert ch[-1][0] == len(lens) - 40 and int(offs[ch[-1][0]]) == 1 << 49
    assert len(lens) > 1 << 19 and max(lens) == 1 << 30 and set(lens[-40:]) == {1 << 30}
    # the node's last 50 entries as a node of their own: 44 bytes up to 2^49 - 1, then 45
    b, root, leaves = W.stride_node(lens[-50:], 0, first=int(offs[-50]))
    kind, kids, noff, size = W.parse_node(b)
    assert [W.entry_len(o) for _, o in kids] == [44] * 10 + [45] * 40


def _canonical(b: bytes) -> bool:
    """By the oracle's decoder (what test_strict_parser_is_the_canonical_form holds parse_node to):
    b decodes, every number is below 2^64, re-encoding the decoded fields gives b back, and the
    node's rules hold."""
    try:
        nodes, leaves, off, size = O._unwrap({b"": b}, b"")
    except IndexError:
        return False
    kids = nodes or leaves
    if (nodes and leaves) or not kids or max([off, size] + [o for _, o in kids]) >= 1 << 64:
        return False
    if O.proto_node(nodes, leaves, off, size) != b or any(len(r) != 32 for r, _ in kids):
        return False
    offs = [o for _, o in kids]
    return offs[0] == off and all(x < y for x, y in zip(offs, offs[1:])) and size > 0 and \
        off + size < 1 << 64


@pytest.mark.parametrize("lane", [0, 32, 63])
def test_all_lengths_offsets(lane):
    offs = W.all_lengths_offsets(lane)
    lens = [W.entry_len(o) for o in offs]
    assert sorted(set(lens)) == W.ENTRY_LENS and lens == sorted(lens)
    ch = W.offset_lanes(offs)
    assert len(ch) == 10 and ch[0] == (1, 1) and all(ln == lane for _, ln in ch[1:])
    for t in W.THRESHOLDS:
        assert t - 1 in offs and t in offs
    assert offs[0] == 0 and offs[-1] == (1 << 64) - 2 and offs == sorted(set(offs))
    # stride_lanes means the same lane
    assert W.stride_lanes([1, 126, 1, 5]) == W.offset_lanes([0, 1, 127, 128])


def test_edge_nodes_are_what_they_say():
    nodes = W.edge_nodes()
    for n in nodes:
        got = W.parse_node(n["bytes"])
        assert got == (2, n["kids"], n["offset"], n["size"]) and _canonical(n["bytes"])
        assert O._unwrap({b"": n["bytes"]}, b"") == ([], n["kids"], n["offset"], n["size"])
    for n in nodes[:3]:
        assert n["bytes"].endswith(b"\x20\x01") and n["offset"] == 0
        assert n["bytes"][-49:-2] == W._entries(n)[-1] and b"\x18" != n["bytes"][-4:-3]
    assert nodes[3]["bytes"][-11:] == b"\x20" + b"\xff" * 9 + b"\x01" and len(nodes[3]["kids"]) == 1
    assert nodes[4]["bytes"][-21:] == b"\x18" + b"\x80" * 9 + b"\x01\x20" + b"\xff" * 8 + b"\x7f"
    assert nodes[4]["offset"] + nodes[4]["size"] == (1 << 64) - 1
    # who names which leaf: only_leaf(e) by entries of e bytes alone, the common leaf by the rest
    named = {}
    for n in nodes:
        for r, o in n["kids"]:
            named.setdefault(r, set()).add(W.entry_len(o))
    for e in (45, 46, 47):
        assert named[W.sha(W.only_leaf(e))] == {e}
    assert named[W.sha(W.COMMON_LEAF)] == set(W.ENTRY_LENS) and set(named) == set(W.wide_leaves())


@pytest.mark.parametrize("name,lane", W.WIDE_CASES)
def test_model_refuses_every_wide_family(name, lane):
    pool, blobs, roots, k = W.wide_mutated(name, lane)
    bad = W.getter(pool, blobs)(k)
    # the decoder-based criterion refuses it, so a parser that let it pass (one that took a tenth
    # byte of 2, say) fails here
    assert not _canonical(bad) and W.parse_node(bad) is None
    if name != "wrap_2_63":
        n, at = W.wide_target(name, lane)
        first = W.offset_lanes([o for _, o in n["kids"]])[-1][0]
        assert _canonical(n["bytes"]) and len(W._entries(n)[at]) == 47
        assert (at - first) % 64 == lane and at >= first
        pos = sum(map(len, W._entries(n)[:at]))
        assert bad[:pos] == n["bytes"][:pos]  # nothing before entry `at` has changed
    if name == "ends_02":
        sub = bad[pos:pos + 47]
        assert sub[-1] == 2 and all(c & 0x80 for c in sub[37:46])  # 2^64 and more
    if name in ("ends_02", "ends_00") or name in W.WIDE_ALONE:
        # what a parser that kept the low 64 bits and had no rule for the tenth byte would see
        sub = bad[pos:pos + 47]
        spelt = sum((c & 0x7F) << (7 * j) for j, c in enumerate(sub[37:47]))
        low = spelt % (1 << 64)
        elder, younger = n["kids"][at - 1][1], n["kids"][at + (name not in W.WIDE_ALONE)][1]
        kids = n["kids"][:at] + [(n["kids"][0][0], low)] + \
            n["kids"][at + (name not in W.WIDE_ALONE):]
        as_read = O.proto_node([], kids, n["offset"], n["size"])
        if name in W.WIDE_ALONE:
            # only the tenth byte's rule can refuse: the offsets ascend, the rest is a valid node
            assert (elder, low, younger) == ((1 << 63) - 2, (1 << 63) - 1, 1 << 63)
            assert spelt >= 1 << 64 if name == "ends_02_alone" else spelt == low
            assert _canonical(as_read) and W.parse_node(as_read) is not None
            assert len(as_read) == len(bad) - 1 and as_read[:pos] == bad[:pos]
        else:
            # these the ascending rule refuses as well (why the _alone families exist)
            assert low <= elder and not _canonical(as_read)
    rc, status, info, recs, sizes, counts = W.run_model(pool, blobs, roots)
    assert rc == W.ECORRUPT and status.tolist() == [W.OK, W.ECORRUPT]
    assert info["bad_stream"] == 1 and recs is None


def test_grid_caps_and_many_streams():
    caps = W.grid_caps()
    assert set(caps) == {"grid_wgs_per_cu", "count_wgs_per_cu", "kSumTile"} and min(caps.values()) > 0
    t, n = W.grid_threads(1), W.count_waves(1)
    assert t == caps["grid_wgs_per_cu"] * 256 and n == caps["count_wgs_per_cu"] * 4
    n3 = t // 27 + 2
    assert 9 * n3 > n and 27 * n3 > t
    pool, blobs, roots, kinds, data = W.many_streams(40)
    assert len(roots) == len(kinds) == 45 and kinds[7] == "z" and kinds[11] == "m"
    assert kinds[-3:] == ["m", "z", "m"] and {0, 1, 2} <= set(kinds) and roots[7] == bytes(32)
    assert len({roots[kinds.index(k)] for k in (0, 1, 2, "m", "z")}) == 5
    rc, status, info, recs, sizes, counts = W.run_model(pool, blobs, roots)
    assert rc == W.OK and info["depth"] == 2 and info["nrecs"] == 27 * 40 + 3 * 7
    assert counts.tolist() == [7 if k == "m" else 0 if k == "z" else 27 for k in kinds]
    assert sizes.tolist() == [len(data[k]) for k in kinds]
    get = {r: b for r, b in zip((bytes(x) for x in blobs["ref"]), map(W.getter(pool, blobs),
                                                                     range(len(blobs))))}
    for s, k in enumerate(kinds):
        mine = recs[recs["stream"] == s]
        assert b"".join(get[r.tobytes()] for r in mine["ref"]) == data[k]
        # a stream's records are not those of the streams before it
        for back in (1, 2):
            if s >= back and kinds[s - back] != k:
                other = recs[recs["stream"] == s - back]
                assert mine["ref"].tobytes() != other["ref"].tobytes()

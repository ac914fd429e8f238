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

"""The model of gc_cases.py pinned on the CPU: against walk_cases.model where the two must agree,
where they must differ, against the recursive gc.Protect, and on its own determinism."""
import numpy as np
import pytest

import gc_cases as G
import walk_cases as W

NODE_FORM = [n for n in W.FAMILIES if n not in ("flip_ref", "own_offset", "own_size")]
# (family, where) whose fault lies in the node's own form; "wrap" at a Root (offset 0) wraps
# nothing and only outgrows the children's covers
FORM_AT = [(n, w) for n in NODE_FORM + ["flip_ref"] for w in ("root", "middle", "leaf")
           if (n, w) != ("wrap", "root")]
COVER_AT = [(n, w) for n in ("own_offset", "own_size") for w in ("root", "middle", "leaf")] + \
    [("wrap", "root")]


def _single_root_cases():
    t, lstore = W.three_level(2)
    pool, blobs = W.pool_of({**lstore, **t.store()})
    yield "three_level", pool, blobs, [t.root]
    pool, blobs, roots, _ = W.mixed_depth()
    yield "mixed_depth", pool, blobs, roots
    pool, blobs, roots = W.chain(5)
    yield "chain", pool, blobs, roots
    for nchunks, fanout in ((1, 2), (40, 2), (200, 3)):
        data, chunks, root, store = W.oracle_tree(7, nchunks, fanout)
        store = dict(store)
        for c, _ in chunks:
            store.setdefault(W.sha(c), c)
        pool, blobs = W.pool_of(store)
        yield "oracle_%d_%d" % (nchunks, fanout), pool, blobs, [root]


@pytest.mark.parametrize("case", list(_single_root_cases()), ids=lambda c: c[0])
def test_live_is_what_the_walk_visits_and_its_records(case):
    _, pool, blobs, roots = case
    visited = set()
    get = W.getter(pool, blobs)

    def blob_bytes(k):
        visited.add(k)
        return get(k)

    rc, _, winfo, recs, _, _ = W.model(blob_bytes, blobs, roots, len(pool))
    assert rc == W.OK
    index = G.index_of(blobs)
    want = visited | {index[r.tobytes()] for r in recs["ref"]}
    rc, status, info, live = G.run_model(pool, blobs, roots)
    assert rc == G.OK and status.tolist() == [0]
    assert set(np.flatnonzero(live).tolist()) == want
    assert info["nnodes"] == len(visited) and info["depth"] == winfo["depth"]
    assert info["nlive"] + info["ndead"] == len(blobs)
    # the recursive gc.Protect keeps the same refs
    view = {}
    for k in range(len(blobs)):
        view.setdefault(blobs[k]["ref"].tobytes(), get(k))
    assert {index[r] for r in G.protect(view, roots)} == want


@pytest.mark.parametrize("name,where", FORM_AT)
def test_node_form_faults_give_the_walks_verdict(name, where):
    pool, blobs, roots, want = W.mutated(name, where, 1)
    wrc = W.run_model(pool, blobs, roots)[0]
    rc, status, info, live = G.run_model(pool, blobs, roots)
    assert rc == wrc == want and live is None
    d, i = W.WHERE[where]
    trees, _ = W.two_streams()
    k = G.index_of(blobs)[trees[1].nodes[d][i]["ref"]]
    assert info["bad_blob"] == k
    # the status speaks of a Root's own blob alone
    assert status.tolist() == [0, want if where == "root" and want == G.ECORRUPT else 0]
    assert info["bad_root"] == (1 if where == "root" and want == G.ECORRUPT else G.NONE)


@pytest.mark.parametrize("name,where", COVER_AT)
def test_a_cover_fault_passes_the_mark(name, where):
    """The difference from the walk, on purpose: split.Protect follows refs and nothing else."""
    pool, blobs, roots, want = W.mutated(name, where, 0)
    assert W.run_model(pool, blobs, roots)[0] == want == W.ECORRUPT
    rc, status, info, live = G.run_model(pool, blobs, roots)
    assert rc == G.OK and status.tolist() == [0, 0] and info["bad_blob"] == G.NONE
    clean = W.pool_of(W.two_streams()[1])
    assert live.tolist() == G.run_model(clean[0], clean[1], roots)[3].tolist()


def test_bad_blob_does_not_depend_on_the_root_order():
    trees, store = W.two_streams()
    for s, (d, i) in ((0, (2, 7)), (1, (1, 2)), (1, (2, 0))):
        n = trees[s].nodes[d][i]
        store[n["ref"]] = W.FAMILIES["padded"][0](n)
    pool, blobs = W.pool_of(store)
    roots = [t.root for t in trees] + [trees[0].nodes[1][1]["ref"], bytes(32)]
    first = G.run_model(pool, blobs, roots)
    assert first[0] == G.ECORRUPT and first[2]["bad_blob"] != G.NONE
    rng = np.random.default_rng(1)
    for _ in range(5):
        order = rng.permutation(len(roots))
        got = G.run_model(pool, blobs, [roots[j] for j in order])
        assert got[0] == first[0]
        assert {k: v for k, v in got[2].items() if k != "bad_root"} == \
            {k: v for k, v in first[2].items() if k != "bad_root"}


def test_layout_and_compacted_bytes():
    pool, blobs, roots = G.len_mix("LDLLDL")
    rc, _, info, live = G.run_model(pool, blobs, roots)
    assert rc == G.OK and info["nlive"] == 1 + 8
    for al in (False, True):
        table, end = G.layout(blobs, live, al)
        out = G.compacted(pool, blobs, live, al)
        assert len(out) == end and len(table) == info["nlive"]
        if al:
            assert (table["off"] % 16 == 0).all()
        else:
            assert end == info["live_bytes"]
        for t in table:
            k = G.index_of(blobs)[t["ref"].tobytes()]
            o, n, so = int(t["off"]), int(t["len"]), int(blobs[k]["off"])
            assert out[o:o + n].tobytes() == pool[so:so + n].tobytes()


def test_case_builders_mean_what_they_say():
    pool, blobs, roots, nodes = G.shared_subtree()
    assert G.run_model(pool, blobs, roots)[2]["nnodes"] == nodes
    pool, blobs, roots = G.same_child_level(8)
    assert G.run_model(pool, blobs, roots)[2]["nnodes"] == 1 + 8 + 1
    pool, blobs, roots = G.cycle()
    rc, _, info, live = G.run_model(pool, blobs, roots)
    assert rc == G.OK and live.tolist() == [1, 1] and info["nnodes"] == 2
    pool, blobs, roots, leaf = G.both_ways()
    assert G.run_model(pool, blobs, roots[:1])[3][leaf] == 0
    assert G.run_model(pool, blobs, roots)[3][leaf] == 1
    assert G.run_model(pool, blobs, roots[::-1])[3][leaf] == 1
    for n in (1, 2, 63, 64, 65):
        pool, blobs, roots, flags = G.sized_pool(n)
        rc, _, info, _ = G.run_model(pool, blobs, roots, flags=flags)
        assert rc == G.OK and len(blobs) == n and info["nlive"] == n // 2 + 1
    pool, blobs, roots = W.chain(69)
    assert G.run_model(pool, blobs, roots)[0] == G.ECORRUPT
    pool, blobs, roots = W.chain(99)
    rc, _, info, live = G.run_model(pool, blobs, roots + [blobs[50]["ref"].tobytes()])
    assert rc == G.OK and info["depth"] == 49 and live.all()


# ---- the builders of test_gpu_gc_wide.py -----------------------------------------------------------
def test_edge_pool():
    pool, blobs, roots = G.edge_pool()
    rc, status, info, live = G.run_model(pool, blobs, roots)
    assert rc == G.OK and status.tolist() == [0] * 5 and info["nnodes"] == 5
    assert info["ndead"] == 1 and info["depth"] == 0
    index = G.index_of(blobs)
    for e in (45, 46, 47):
        assert live[index[W.sha(W.only_leaf(e))]] == 1
    view = {blobs[k]["ref"].tobytes(): W.getter(pool, blobs)(k) for k in range(len(blobs))}
    assert {index[r] for r in G.protect(view, roots)} == set(np.flatnonzero(live).tolist())
    # the walk holds every child to its cover: it refuses these nodes, which is why the mark
    # carries them
    assert W.run_model(pool, blobs, roots[:1])[0] == W.ECORRUPT
    # each only_leaf is live through its own entries: without the three all_lengths nodes and the
    # node at 2^63, none is
    assert G.run_model(pool, blobs, roots[3:4])[2]["nlive"] == 2
    gone = W.sha(W.only_leaf(47))
    pool, blobs, roots = G.edge_pool(drop=[gone])
    assert G.run_model(pool, blobs, roots)[0] == G.ENOTFOUND
    rc, status, info, live = G.run_model(pool, blobs, roots, flags=G.GC_MISSING_LEAVES)
    assert rc == G.OK and info["missing_leaves"] == 1
    assert sum(r == gone for n in W.edge_nodes() for r, _ in n["kids"]) == 4


@pytest.mark.parametrize("name,lane", W.WIDE_CASES)
def test_wide_faults_give_the_walks_verdict(name, lane):
    pool, blobs, roots, k = W.wide_mutated(name, lane)
    wrc = W.run_model(pool, blobs, roots)[0]
    rc, status, info, live = G.run_model(pool, blobs, roots)
    assert rc == wrc == G.ECORRUPT and live is None
    assert info["bad_blob"] == k and info["bad_root"] == 1 and status.tolist() == [0, G.ECORRUPT]
    # the node as it was passes the mark
    n = W.wide_target(name, lane)[0] if name != "wrap_2_63" else W.edge_nodes()[4]
    assert n["ref"] == roots[1]
    pool, blobs = G.pool_from(list(W.wide_leaves().items()) + [(n["ref"], n["bytes"])])
    assert G.run_model(pool, blobs, roots[1:])[0] == G.OK


def test_grid_pass_builders_mean_what_they_say():
    t, n = W.grid_threads(1), W.count_waves(1)
    pool, blobs, roots = G.wide(n + 3)
    rc, _, info, live = G.run_model(pool, blobs, roots)
    assert rc == G.OK and info["nnodes"] == n + 4 and live.all()
    # the walk accepts wide() as well: a level of t + 3 nodes under a `nodes` node of t + 3 entries
    pool, blobs, roots = G.wide(t + 3)
    rc, _, info, recs, sizes, counts = W.run_model(pool, blobs, roots)
    assert rc == W.OK and info["nnodes"] == t + 4 and info["depth"] == 1
    assert counts.tolist() == [t + 3] and sizes.tolist() == [10 * (t + 3)]
    assert len(W.parse_node(W.getter(pool, blobs)(len(blobs) - 1))[1]) == t + 3
    pool, blobs, roots, own = G.many_roots(t + 5)
    assert len(roots) == t + 5 and set(roots[:-2]) == {roots[0], bytes(32)}
    assert len({roots[0], roots[-2], roots[-1]}) == 3 and not set(own[1]) & set(own[2])
    rc, status, info, live = G.run_model(pool, blobs, roots)
    assert rc == G.OK and live.all() and info["nnodes"] == 39
    live = G.run_model(pool, blobs, roots[:-2])[3]
    assert not live[own[1]].any() and not live[own[2]].any() and live[own[0]].all()
    pool, blobs, roots, own = G.many_roots(t + 5, malformed=True)
    rc, status, info, live = G.run_model(pool, blobs, roots)
    assert rc == G.ECORRUPT and status[-1] == G.ECORRUPT and not status[:-1].any()
    assert info["bad_root"] == t + 4 and info["bad_blob"] == G.index_of(blobs)[roots[-1]]
    nblobs = 2 * (t + 7)
    pool, blobs, roots, flags = G.sized_pool(nblobs)
    rc, _, info, live = G.run_model(pool, blobs, roots, flags=flags)
    k = G.index_of(blobs)[roots[0]]
    assert rc == G.OK and len(blobs) == nblobs > 2 * t and info["nlive"] == t + 8
    assert len(W.parse_node(W.getter(pool, blobs)(k))[1]) == t + 7 and info["nnodes"] == 1
    assert -(-nblobs // W.grid_caps()["kSumTile"]) > 2

"""The host tail at its list, ring, bucket and gather edges, on the planted runs of
tests/tail_cases.py (held to their claims by test_tail_cases_cpu.py). Every run's records are
compared field for field (offset, len, level, ref, stream) and its counts per stream with the
oracle's split of the same bytes, and the plan diag()["host_tail"] reports (chunks, bytes,
host_blocks, longest_blocks, longest_left_blocks, cut_blocks) with tail_cases.model exactly.

(1) many_chunks, the list limits: k_offload_gather's 64 workgroups each copy three chunks and more,
    up to 64 at a full list;
(2) gather_ends: every start residue modulo 16 and final chunks shorter than, as long as and just
    longer than the bytes before the first whole vector;
(3) gather_loop: vector counts at the edges of the 4x-unrolled loop;
(4) list limits: a bucket that would pass 4,096 chunks is left whole, 4,096 chunks of one bucket
    are all taken, 4,097 none, and the full list follows the empty one on one engine;
(5) ring limits: a ring of exactly two buckets' slots, one byte less, and three buckets' slots and
    a slot more;
(6) floors inside a bucket;
(7) a run whose candidates overflow the first estimate: the tail stands down, the re-run has one;
(8) the plan's numbers, in every test; and the cost model's own cut, whatever it is, takes exactly
    the records longer than what it reports as left."""
import pytest

import tail_cases as T

pytestmark = pytest.mark.gpu


def _want(oracle, table, name):
    case = T.get(table, name)
    return case, T.expect(case, oracle, table)


def _plan(tail, m, what):
    print(what, tail)
    got = {f: tail[f] for f in T.PLAN_FIELDS}
    assert got == {f: m[f] for f in T.PLAN_FIELDS}, what


def _forced(gpu, case, want, force_cut, ring_bytes, what, **kw):
    got = T.split(gpu, case, force_cut=force_cut, ring_bytes=ring_bytes, **kw)
    T.check(got, want, what)
    m = T.model(T.rec_lens(want), force_cut, ring_bytes)
    _plan(got["tail"], m, what)
    return got, m


@pytest.mark.parametrize("portable", [False, True], ids=["best", "portable"])
def test_gather_ends(gpu, oracle, table, portable):
    """(2)"""
    case, want = _want(oracle, table, "tail-gather-ends")
    with T.device(gpu, case) as buf:
        assert buf.ptr % 16 == 0           # the case's residues are the device's
    got, m = _forced(gpu, case, want, 1, case.note["ring_bytes"], "gather ends", portable=portable)
    assert m["chunks"] == len(want["records"])
    assert portable is False or got["tail"]["impl"] == "portable"


@pytest.mark.parametrize("portable", [False, True], ids=["best", "portable"])
def test_gather_loop(gpu, oracle, table, portable):
    """(3)"""
    case, want = _want(oracle, table, "tail-gather-loop")
    got, m = _forced(gpu, case, want, 1, case.note["ring_bytes"], "gather loop", portable=portable)
    assert m["chunks"] == len(want["records"])
    assert portable is False or got["tail"]["impl"] == "portable"


def test_many_chunks(gpu, oracle, table):
    """(1)"""
    case, want = _want(oracle, table, "tail-many-chunks")
    _, m = _forced(gpu, case, want, 1, case.note["ring_bytes"], "many chunks")
    assert m["chunks"] == len(want["records"]) >= 3 * T.GATHER_WGS


def test_list_limit_bucket_left_whole(gpu, oracle, table):
    """(4a)"""
    case, want = _want(oracle, table, "tail-list-a")
    _, m = _forced(gpu, case, want, 1, case.note["ring_bytes"], "list a")
    assert 0 < m["chunks"] <= T.MAX_ITEMS < len(want["records"])


def test_list_limit_at_equality(gpu, oracle, table):
    """(4b)"""
    case, want = _want(oracle, table, "tail-list-b")
    _, m = _forced(gpu, case, want, 1, case.note["ring_bytes"], "list b")
    assert m["chunks"] == T.MAX_ITEMS == len(want["records"])


def test_list_limit_full_after_empty(gpu, oracle, table):
    """(4c), then (4b) on the same engine: the full list follows the empty one."""
    c, wc = _want(oracle, table, "tail-list-c")
    b, wb = _want(oracle, table, "tail-list-b")
    ring = c.note["ring_bytes"]
    with T.device(gpu, c) as bc, T.device(gpu, b) as bb:
        eng = gpu.Engine()
        try:
            eng.set_host_tail(0, force_cut=1, ring_bytes=ring)
            T.run(eng, bc, c)
            eng.finish()
            none = T.result(eng)
            T.run(eng, bb, b)
            eng.finish()
            full = T.result(eng)
        finally:
            eng.close()
    T.check(none, wc, "list c")
    mc = T.model(T.rec_lens(wc), 1, ring)
    _plan(none["tail"], mc, "list c")
    assert mc["chunks"] == 0 and mc["longest_left_blocks"] == mc["longest_blocks"]
    T.check(full, wb, "list b after c")
    mb = T.model(T.rec_lens(wb), 1, ring)
    _plan(full["tail"], mb, "list b after c")
    assert mb["chunks"] == T.MAX_ITEMS


@pytest.mark.parametrize("which", ["equal", "one-less", "three-and-a-slot"])
def test_ring_limit(gpu, oracle, table, which):
    """(5)"""
    case, want = _want(oracle, table, "tail-ring")
    ring, nbuckets = T.ring_values(T.rec_lens(want))[which]
    _, m = _forced(gpu, case, want, case.note["force_cut"], ring, ("ring", which))
    assert m["chunks"] == sum(len(g) for g in T.RING_BUCKETS[:nbuckets])
    assert which != "equal" or m["bytes"] == ring


@pytest.mark.parametrize("cut", T.FLOOR_CUTS)
def test_floor_in_bucket(gpu, oracle, table, cut):
    """(6)"""
    case, want = _want(oracle, table, "tail-floor")
    _, m = _forced(gpu, case, want, cut, case.note["ring_bytes"], ("floor", cut))
    assert m["chunks"] == sum(1 for n in T.rec_lens(want) if T.blocks(n) >= cut)
    assert m["longest_left_blocks"] == cut - 1


def test_overflow_rerun(gpu, oracle, table):
    """(7): the records and the tail are the re-run's; the engine's next ordinary run is right."""
    case, want = _want(oracle, table, "tail-overflow")
    three, w3 = _want(oracle, table, "tail-three")
    fc, ring = case.note["force_cut"], case.note["ring_bytes"]
    assert want["ncand"] > 65536
    with T.device(gpu, case) as bo, T.device(gpu, three) as b3:
        eng = gpu.Engine()
        try:
            eng.set_host_tail(0, force_cut=fc, ring_bytes=ring)
            T.run(eng, bo, case)
            eng.finish()
            ncand = int(eng.candidates)
            first = T.result(eng)
            T.run(eng, b3, three)
            eng.finish()
            again = T.result(eng)
        finally:
            eng.close()
    assert ncand == want["ncand"]
    T.check(first, want, "overflow")
    _plan(first["tail"], T.model(T.rec_lens(want), fc, ring), "overflow")
    assert first["tail"]["chunks"] == 3
    T.check(again, w3, "tail-three after the re-run")
    _plan(again["tail"], T.model(T.rec_lens(w3), fc, ring), "tail-three after the re-run")
    assert again["tail"]["chunks"] == 3


@pytest.mark.parametrize("name", ["tail-many-chunks", "tail-three"])
def test_model_cut_takes_whole_buckets(gpu, oracle, table, name):
    """(8): nothing forced. The cut depends on a host rate measured at run time, so no count is
    asserted: whatever is taken is exactly the records of at least 256 blocks that are longer
    than the longest one reported as left."""
    case, want = _want(oracle, table, name)
    got = T.split(gpu, case, ring_bytes=T.RING)
    tail = got["tail"]
    print(name, tail)
    T.check(got, want, name)
    lens = T.rec_lens(want)
    taken = [n for n in lens if T.blocks(n) > tail["longest_left_blocks"]
             and T.blocks(n) >= T.MIN_BLOCKS]
    assert tail["chunks"] == len(taken) <= T.MAX_ITEMS
    assert tail["bytes"] == sum(T.slot(n) for n in taken) <= T.RING
    assert tail["host_blocks"] == sum(T.blocks(n) for n in taken)
    assert tail["longest_blocks"] == max(T.blocks(n) for n in lens)

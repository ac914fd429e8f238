"""tests/tail_cases.py held to its claims against the oracle (no GPU): what keeps
test_gpu_host_tail_edges.py from passing vacuously.

For every case the oracle cuts exactly the planned chunks. Per case: gather_ends covers every start
residue and every relation of a final chunk's length to its head; gather_loop meets its nvec list;
the chunk counts are over 64 and over, at and one over 4,096; the three rings take 2, 1 and 3
buckets; the floors fall inside a bucket; the overflow run has more than 65,536 candidates. The
model is held to a restatement from the definition on random length lists, and to the numbers
test_gpu_host_tail.py asserts on tail-three."""
import numpy as np
import pytest

import early_cases as C
import tail_cases as T


def _want(oracle, table, name):
    c = T.get(table, name)
    return c, T.expect(c, oracle, table)


def _planned(c):
    """The chunk lengths the plans ask for, stream by stream ("z" runs left out)."""
    return [[int(seg[1]) for seg in pl] for pl in c.plans]


@pytest.mark.parametrize("name", [n for n in T.CASES if n != "tail-overflow"])
def test_oracle_cuts_the_planned_chunks(oracle, table, name):
    c, x = _want(oracle, table, name)
    k = 0
    for s, lens in enumerate(_planned(c)):
        got = x["records"][k:k + x["counts"][s]]
        k += x["counts"][s]
        assert [r[1] for r in got] == lens, (name, s)
        assert [r[4] for r in got] == [s] * len(lens)
        assert c.off[s] % 16 == 0
    assert k == len(x["records"])
    assert max(o + n for o, n in zip(c.off, c.lens)) + C.SLACK < 6_000_000
    print(name, "bytes", sum(c.lens), "records", len(x["records"]))


def test_gather_ends_cover(oracle, table):
    c, x = _want(oracle, table, "tail-gather-ends")
    recs = x["records"]
    m = T.model(T.rec_lens(x), c.note["force_cut"], c.note["ring_bytes"])
    assert m["chunks"] == len(recs) == 2 * len(c.plans) > T.GATHER_WGS      # every chunk goes
    addr = T.starts(c, recs)
    finals = [(a % 16, r[1]) for a, r in zip(addr, recs) if r[0] != 0]
    assert len(finals) == len(c.plans)
    assert [(a, t) for a, _, t in c.note["finals"]] == finals
    assert {a for a, _ in finals} == set(range(16))
    assert {a % 16 for a, r in zip(addr, recs) if r[0] == 0} == {0}
    kinds, mods = set(), set()
    for a, n in finals:
        head, nvec, tail = T.gather_split(a, n)
        full = (16 - a) & 15
        assert head == min(n, full) and head + 16 * nvec + tail == n and tail < 16
        if n < full:
            kinds.add("below head")
        elif n == full:
            kinds.add("head")
        elif n < full + 16:
            assert nvec == 0 and tail
            kinds.add("no vector")
        elif n == full + 16:
            assert nvec == 1 and not tail
            kinds.add("one vector")
        if n >= full:
            mods.add((n - full) % 16)
    assert kinds == {"below head", "head", "no vector", "one vector"}
    assert mods == set(range(16))
    assert any(n == 1 for _, n in finals)
    # the first chunks: a whole number of vectors and every tail but for the head
    assert {T.gather_split(a, r[1])[2] for a, r in zip(addr, recs) if r[0] == 0} == set(range(16))


def test_gather_loop_nvec(oracle, table):
    c, x = _want(oracle, table, "tail-gather-loop")
    recs = x["records"]
    addr = T.starts(c, recs)
    split = {r[0]: T.gather_split(a, r[1]) for a, r in zip(addr, recs)}
    longs = c.note["longs"]
    assert [split[o][1] for o, _, _ in longs] == list(T.LOOP_NVEC) == [v for _, _, v in longs]
    assert T.LOOP_NVEC == (1023, 1024, 1025, 3071, 3072, 3073, 4095, 4096, 4097, 7169)
    assert sum(1 for o, _, _ in longs if (c.off[0] + o) % 16) >= 3
    assert sum(1 for o, _, _ in longs if split[o][2]) >= 3 and any(not split[o][2] for o, _, _ in longs)
    others = [v[1] for o, v in split.items() if o not in {o for o, _, _ in longs}]
    assert others and max(others) < 100              # short chunks between them
    m = T.model(T.rec_lens(x), 1, c.note["ring_bytes"])
    assert m["chunks"] == len(recs) == 2 * len(T.LOOP_NVEC) + 1


def test_many_chunks_counts(oracle, table):
    c, x = _want(oracle, table, "tail-many-chunks")
    lens = T.rec_lens(x)
    assert len(lens) >= 200 + 1 and len(lens) >= 3 * T.GATHER_WGS
    planted = lens[:-1]
    assert min(planted) >= 1100 and max(planted) <= 3000 and max(planted) - min(planted) > 1500
    assert len(set(planted)) < len(planted)
    m = T.model(lens, 1, c.note["ring_bytes"])
    assert m["chunks"] == len(lens) and m["bytes"] <= c.note["ring_bytes"]
    assert max(T.blocks(n) for n in lens) < T.MIN_BLOCKS       # the cost model takes none of them


def test_list_limit_counts(oracle, table):
    c, x = _want(oracle, table, "tail-list-a")
    lens = T.rec_lens(x)
    nb = [T.blocks(n) for n in lens]
    assert len(lens) > T.MAX_ITEMS and T.width(max(nb)) == 1
    per = {b: nb.count(b) for b in set(nb)}
    assert sorted(per) == list(T.LIST_BLOCKS) and len(per) >= 36
    assert all(v in (T.LIST_PER, T.LIST_PER + 1) for v in per.values())
    m = T.model(lens, 1, c.note["ring_bytes"])
    assert m["chunks"] == len(lens) - per[min(per)] <= T.MAX_ITEMS < len(lens)
    assert m["longest_left_blocks"] == min(per) and m["cut_blocks"] == min(per) + 1
    assert m["taken"] == {i for i, b in enumerate(nb) if b > min(per)}
    assert T.model(lens, 1, 1 << 40)["chunks"] == m["chunks"]           # the ring does not limit
    assert len({x["records"][i][3] for i in range(len(lens))}) == len(lens)   # distinct content

    for name, count in (("tail-list-b", T.MAX_ITEMS), ("tail-list-c", T.MAX_ITEMS + 1)):
        c, x = _want(oracle, table, name)
        lens = T.rec_lens(x)
        assert len(lens) == count and {T.blocks(n) for n in lens} == {18}
        assert len(set(lens)) > 32 and len({r[3] for r in x["records"]}) == count
        m = T.model(lens, 1, c.note["ring_bytes"])
        if count == T.MAX_ITEMS:
            assert m["chunks"] == count and m["longest_left_blocks"] == 0
            assert m["cut_blocks"] == 18 and m["bytes"] < c.note["ring_bytes"]
        else:
            assert m["chunks"] == 0 and m["longest_left_blocks"] == m["longest_blocks"] == 18
            assert m["cut_blocks"] == 0 and m["bytes"] == 0


def test_ring_values(oracle, table):
    c, x = _want(oracle, table, "tail-ring")
    lens = T.rec_lens(x)
    nb = [T.blocks(n) for n in lens]
    fc = c.note["force_cut"]
    assert max(nb) == 520 and T.width(520) == 3
    per = {}
    for b in nb:
        if b >= fc:
            per.setdefault(T.bucket(520, b), []).append(b)
    assert sorted(per, reverse=True) == [173, 170, 165, 160]
    assert [sorted(per[k]) for k in (173, 170, 165, 160)] == [sorted(g) for g in T.RING_BUCKETS]
    assert all(3 <= len(g) <= 5 for g in per.values())
    rings = T.ring_values(lens)
    edges = {2: 170 * 3, 1: 173 * 3, 3: 165 * 3}
    left = {2: 497, 1: 512, 3: 482}
    for name, (ring, nbuckets) in rings.items():
        m = T.model(lens, fc, ring)
        assert m["chunks"] == sum(len(g) for g in T.RING_BUCKETS[:nbuckets]), name
        assert m["cut_blocks"] == edges[nbuckets] and m["longest_left_blocks"] == left[nbuckets]
        assert m["bytes"] <= ring
        if name == "equal":
            assert m["bytes"] == ring
    assert rings["equal"][0] - rings["one-less"][0] == 1
    three = T.model(lens, fc, rings["three-and-a-slot"][0])
    assert rings["three-and-a-slot"][0] - three["bytes"] == min(
        T.slot(n) for n in lens if T.bucket(520, T.blocks(n)) == 160)


def test_floor_in_bucket(oracle, table):
    c, x = _want(oracle, table, "tail-floor")
    lens = T.rec_lens(x)
    nb = [T.blocks(n) for n in lens]
    assert max(nb) == 2050 and T.width(2050) == 9
    assert sorted(b for b in nb if 900 < b < 2050) == list(T.FLOOR_BLOCKS)
    assert {T.bucket(2050, b) for b in range(999, 1008)} == {111} and T.bucket(2050, 1008) == 112
    for fc, chunks in zip(T.FLOOR_CUTS, (6, 3, 2)):
        m = T.model(lens, fc, c.note["ring_bytes"])
        assert m["chunks"] == chunks and m["cut_blocks"] == fc
        assert m["longest_left_blocks"] == fc - 1 and fc - 1 in nb
        assert m["taken"] == {i for i, b in enumerate(nb) if b >= fc}
    # chunks on both sides of the floor in one bucket
    assert T.bucket(2050, 1003) == T.bucket(2050, 1004) and T.bucket(2050, 1006) == T.bucket(2050, 1007)


def test_overflow_rerun_candidates(oracle, table):
    c, x = _want(oracle, table, "tail-overflow")
    assert x["ncand"] > 65536 and 200 << 10 < sum(c.lens) < 1 << 20
    lens = T.rec_lens(x)
    m = T.model(lens, c.note["force_cut"], c.note["ring_bytes"])
    assert m["chunks"] == 3 and sorted(T.blocks(lens[i]) for i in m["taken"]) == [1333, 1705, 2050]
    got = [int(p) for p in x["cands"][0]]
    assert got == c.cands[0]


def test_model_on_tail_three(oracle, table):
    """The numbers test_gpu_host_tail.py asserts."""
    c, x = _want(oracle, table, "tail-three")
    lens = T.rec_lens(x)
    for cut, chunks in ((5000, 0), (2000, 1), (1000, 3), (1, 9)):
        m = T.model(lens, cut, 1 << 20)
        assert m["chunks"] == chunks == sum(1 for n in lens if T.blocks(n) >= cut)
        assert m["host_blocks"] == sum(T.blocks(n) for n in lens if T.blocks(n) >= cut)
    small = T.model(lens, 1000, C.L(2050, 55) + 4096)
    assert small["chunks"] == 1 and small["longest_left_blocks"] == 1705
    assert small["longest_blocks"] == 2050 and small["cut_blocks"] == 227 * 9


# ---------------------------------------------------------------------------------------------
# The model against the definition
# ---------------------------------------------------------------------------------------------
def brute(lens, force_cut, ring_bytes, max_items):
    """From the definition: the candidates sorted by bucket, longest bucket first; of the
    prefixes that end where a bucket ends, the longest one that the list and the ring hold and
    whose shorter such prefixes they hold too."""
    nb = [T.blocks(n) for n in lens]
    mx = max(nb)
    w = mx // 256 + 1
    cand = sorted((i for i in range(len(lens)) if nb[i] >= force_cut),
                  key=lambda i: -min(nb[i] // w, 255))
    best = 0
    for k in range(1, len(cand) + 1):
        if k < len(cand) and min(nb[cand[k]] // w, 255) == min(nb[cand[k - 1]] // w, 255):
            continue                                   # inside a bucket
        if k > max_items or sum(T.slot(lens[i]) for i in cand[:k]) > ring_bytes:
            break
        best = k
    taken, rest = cand[:best], cand[best:]
    if not taken:
        left, cut = mx, 0
    else:
        left = max(nb[i] for i in rest) if rest else min(force_cut - 1, mx)
        cut = max(min(min(nb[i] // w, 255) for i in taken) * w, force_cut)
    return {"taken": set(taken), "chunks": len(taken),
            "bytes": sum(T.slot(lens[i]) for i in taken),
            "host_blocks": sum(nb[i] for i in taken), "longest_blocks": mx,
            "longest_left_blocks": left, "cut_blocks": cut}


@pytest.mark.parametrize("seed", range(6))
def test_model_against_the_definition(seed):
    rng = np.random.default_rng([505, seed])
    lists = stops = 0
    for _ in range(50):
        count = int(rng.integers(1, 60))
        top = int(rng.choice([300, 5000, 40000, 200000]))
        lens = [int(v) for v in rng.integers(1, top, count)]
        lens += [int(rng.choice(lens)) for _ in range(int(rng.integers(0, 10)))]      # ties
        nb = [T.blocks(n) for n in lens]
        fc = int(rng.choice([1, max(nb) // 2 + 1, max(nb), max(nb) + 1, int(rng.choice(nb))]))
        free = T.model(lens, fc, 1 << 40, 1 << 30)
        assert free == brute(lens, fc, 1 << 40, 1 << 30)
        assert free["taken"] == {i for i, b in enumerate(nb) if b >= fc}
        # a ring, then a list, that stops the cut below every bucket (and one short of it)
        per = {}
        for i in free["taken"]:
            per.setdefault(T.bucket(max(nb), nb[i]), []).append(i)
        n = nbytes = 0
        for b in sorted(per, reverse=True):
            n += len(per[b])
            nbytes += sum(T.slot(lens[i]) for i in per[b])
            for ring, items in ((nbytes, 1 << 30), (nbytes - 1, 1 << 30), (1 << 40, n),
                                (1 << 40, n - 1), (nbytes, n)):
                m = T.model(lens, fc, ring, items)
                assert m == brute(lens, fc, ring, items), (lens, fc, ring, items)
                assert m["chunks"] <= items and m["bytes"] <= ring
                if (ring, items) == (nbytes, n):
                    assert m["chunks"] == n and m["bytes"] == nbytes
                stops += 1
        lists += 1
    assert lists == 50 and stops > 500

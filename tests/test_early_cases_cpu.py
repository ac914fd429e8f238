"""tests/early_cases.py held to its claims against the oracle (no GPU): what keeps
test_gpu_early_small.py from passing vacuously.

For every case: the oracle finds exactly the planned candidates and cuts exactly the chunks
planting.greedy_walk cuts from them; every chunk the case is about is (or, where the case says so,
is not) a record and a sure chunk; the model's picks over the oracle's candidates are the intended
ones. Per family: the candidate indices of (j) fall in the intended thread, wave and workgroup
classes, (k) covers every (blocks, tail), (l) every start residue, (m) its levels. The model is
checked once against the definition applied chunk by chunk (early_cases.brute_picks) on random
streams at low Bits with the floor lowered."""
import numpy as np
import pytest

import early_cases as C
import planting as P
import sha_edges as E


def _case(table, name):
    return C.get(table, name)


@pytest.mark.parametrize("name", C.NAMES)
def test_case_holds_its_claims(oracle, table, name):
    c = _case(table, name)
    x = C.expect(c, oracle, table)
    assert sum(c.lens) + 16 * len(c.lens) <= (2 << 20) + (128 << 10)
    recs, flat = x["records"], C.run_candidates(x["cands"], c.lens)
    k = 0
    for s, d in enumerate(c.streams):
        got = [int(p) for p in x["cands"][s]]
        assert got == c.cands[s], (name, s, "candidates", sorted(set(got) ^ set(c.cands[s]))[:8])
        ends = P.greedy_walk(got, len(d), c.min_size)
        mine = recs[k:k + x["counts"][s]]
        k += x["counts"][s]
        assert [o + n - 1 for o, n, *_ in mine] == ends, (name, s)
        assert [r[4] for r in mine] == [s] * len(mine)
    # the chunks the case is about
    spans = c.note.get("spans")
    for stream, start, length, sure in c.longs:
        assert E.nblocks(length) >= 1023, (name, start, length)
        is_rec = any(r[4] == stream and r[0] == start and r[1] == length for r in recs)
        if spans and start > spans[1] and start < spans[1] + spans[2]:
            assert not is_rec and any(r[4] == spans[0] and r[0] == spans[1] and r[1] == spans[2]
                                      for r in recs), (name, spans)
        else:
            assert is_rec, (name, stream, start, length)
        at = [i for i, (s, p, f) in enumerate(flat) if s == stream and p == start - 1 and not f]
        verdict = bool(at) and C.sure_chunk(flat, at[0], c.min_size) == (stream, start, length)
        assert verdict == sure, (name, stream, start, length, sure)
    # no other chunk reaches the floor, so the picks are among the chunks above
    known = {(s, o, n) for s, o, n, _ in c.longs}
    for o, n, _, _, s in recs:
        assert E.nblocks(n) < C.FLOOR or (s, o, n) in known or (spans and (s, o, n) == spans), \
            (name, s, o, n)
    # the model's picks are the intended ones
    picks = x["picks"]
    want = C.intended(c)
    assert len(picks) == len(want) <= 2, (name, picks, want)
    for (blocks, i, rec), (s, start, length) in zip(picks, want):
        assert blocks == E.nblocks(length) >= C.FLOOR
        assert flat[i][:2] == (s, start - 1) and not flat[i][2]
        assert recs[rec][0] == start and recs[rec][1] == length and recs[rec][4] == s
    if len(picks) == 2:
        assert picks[0][:2] > picks[1][:2]
    print(name, "bytes", sum(c.lens), "candidates", x["ncand"], "picks", picks)


def test_floor_lengths():
    assert E.nblocks(65464) == 1024 == E.nblocks(65472) and E.nblocks(65463) == 1023
    assert C.FLOOR == 1024


def test_double_end_candidate(oracle, table):
    """e-forced-natural: the last byte is a natural candidate (the forced one follows it at the
    same position), and the oracle's last record has the planted window's level."""
    c = _case(table, "e-forced-natural")
    x = C.expect(c, oracle, table)
    assert int(x["cands"][0][-1]) == c.lens[0] - 1
    flat = C.run_candidates(x["cands"], c.lens)
    assert flat[-2][:2] == flat[-1][:2] and (flat[-2][2], flat[-1][2]) == (False, True)
    assert x["ncand"] == len(flat) == P.expected_candidates(oracle, table, c.streams[0], c.bits)
    assert x["records"][-1][2] == 3
    plain = C.expect(_case(table, "e-forced"), oracle, table)
    assert int(plain["cands"][0][-1]) != _case(table, "e-forced").lens[0] - 1


def test_stream_edges_layout(table):
    c = _case(table, "f-stream-edges")
    o = c.off
    assert all(x > 0 and x % 16 == 0 for x in o) and o[2] < o[0] < o[1]
    iv = sorted((a, a + n) for a, n in zip(o, c.lens))
    assert all(iv[k][1] + 16 <= iv[k + 1][0] for k in range(2))      # gaps between the streams
    buf = c.buffer()
    assert all((buf[a:a + n] == d).all() for a, n, d in zip(o, c.lens, c.streams))
    assert len(buf) == iv[-1][1] + C.SLACK


def test_tie_cases(oracle, table):
    for name in ("g-ties", "g-ties-streams", "b-floor"):
        c = _case(table, name)
        tied = [x for x in c.longs if E.nblocks(x[2]) == E.nblocks(c.longs[c.picks[0]][2])]
        assert len(tied) >= (3 if name.startswith("g") else 2)
        assert len({x[2] for x in tied}) == len(tied)                # different byte lengths
        picks = C.expect(c, oracle, table)["picks"]
        assert picks[0][0] == picks[1][0] and picks[0][1] > picks[1][1]
    assert len({x[0] for x in _case(table, "g-ties-streams").longs
                if E.nblocks(x[2]) == 1100}) == 3


def test_adjacent_picks_share_a_candidate(oracle, table):
    p = C.expect(_case(table, "h-adjacent"), oracle, table)["picks"]
    assert p[0][1] + 1 == p[1][1] and p[0][2] + 1 == p[1][2]


def test_one_and_none(oracle, table):
    assert len(C.expect(_case(table, "i-one"), oracle, table)["picks"]) == 1
    for name in ("i-none", "b-below", "e-one-chunk"):
        assert C.expect(_case(table, name), oracle, table)["picks"] == []


def _place(i):
    t = i % C.GRID
    return t, t // 64, t // 1024          # thread, wave, workgroup of k_pick's 64 x 1,024 grid


def test_reduction_positions(oracle, table):
    kinds = set()
    for name in [n for n in C.NAMES if n.startswith("j-")]:
        c = _case(table, name)
        x = C.expect(c, oracle, table)
        ia, ib, ic = c.note["index"]
        mirror = name.endswith("-mirror")
        picks = x["picks"]
        assert [p[1] for p in picks] == ([ib, ia] if mirror else [ia, ib]), (name, picks)
        assert picks[1][0] > E.nblocks(c.longs[2][2]) >= C.FLOOR     # C is eligible and third
        third = C.model_picks(x["cands"], c.lens, slots=3)[2]
        assert third[1] == ic and third[0] == E.nblocks(c.longs[2][2])
        (ta, wa, ga), (tb, wb, gb), (tc, wc, gc) = _place(ia), _place(ib), _place(ic)
        kind = c.note["kind"]
        if kind == "wave":
            assert wa == wb and ta != tb
        elif kind == "waves":
            assert ga == gb and wa != wb
        elif kind == "workgroups":
            assert ga != gb
        else:
            assert ta == tb and ib - ia == C.GRID
            assert x["ncand"] > 65536       # more than the first candidate estimate: a re-run
        assert gc not in (ga, gb)           # the third chunk's key comes from another workgroup
        kinds.add((kind, mirror))
    assert kinds == {(k, m) for k in C.J_PAIRS for m in (False, True)}


def test_chain_edges_cover(table):
    seen = []
    for name in [n for n in C.NAMES if n.startswith("k-")]:
        c = _case(table, name)
        for (b, t), (_, _, length, _) in zip(c.note["edges"], c.longs):
            assert E.nblocks(length) == b and length % 64 == t
            seen.append((b, t))
    assert sorted(seen) == sorted((b, t) for b in C.K_BLOCKS for t in E.TAILS)
    assert set(C.K_BLOCKS) == {64 * f + d for f in (16, 17, 18) for d in (-1, 0, 1)} - {1023}
    assert sorted(E.TAILS) == [0, 1, 55, 56, 63]


def test_start_residues_cover(table):
    seen = []
    for name in [n for n in C.NAMES if n.startswith("l-")]:
        c = _case(table, name)
        assert 140_000 <= sum(c.lens) <= 300_000
        got = tuple((c.off[0] + start) % 64 for _, start, _, _ in c.longs)
        assert got == c.note["residues"]
        seen += got
    assert sorted(seen) == list(range(64))
    assert len({_case(table, n).off[0] for n in C.NAMES if n.startswith("l-")}) == 4


def test_levels(oracle, table):
    a = C.expect(_case(table, "m-levels"), oracle, table)
    assert sorted(a["records"][p[2]][2] for p in a["picks"]) == [0, 5]
    b = C.expect(_case(table, "m-level-top-forced"), oracle, table)
    assert b["records"][b["picks"][0][2]][2] == 31 - C.BITS
    assert b["picks"][1][2] == len(b["records"]) - 1                 # the forced final chunk
    assert 2 in [r[2] for r in b["records"]]


@pytest.mark.parametrize("bits,min_size,floor,seed", [(6, 64, 2, 1), (6, 64, 3, 2), (7, 100, 2, 3),
                                                      (7, 64, 1, 4), (8, 64, 2, 5)])
def test_model_against_the_definition(oracle, table, bits, min_size, floor, seed):
    rng = np.random.default_rng([404, seed])
    streams = [rng.integers(0, 256, int(n), dtype=np.uint8) for n in (6000, 0, 4097, 64, 9000)]
    if seed == 4:   # a stream whose last byte is a natural candidate as well
        d = streams[0]
        last = int(P.candidate_positions(oracle, table, d, bits)[-1])
        streams[0] = d[:last + 1]
    cands = [P.candidate_positions(oracle, table, d, bits) for d in streams]
    lens = [len(d) for d in streams]
    for s, d in enumerate(streams):   # hashes() is the oracle's rolling hash
        assert np.array_equal(np.nonzero(C.cand_mask(C.hashes(table, d), bits))[0], cands[s])
    for slots in (2, 10_000):
        model = C.model_picks(cands, lens, min_size, floor, slots)
        brute = C.brute_picks(cands, lens, min_size, floor, slots)
        assert model == brute and (len(model) == 2 or slots > 2)
    assert len(model) >= 10   # many sure chunks, of more than one stream
    assert len({C.run_candidates(cands, lens)[i][0] for _, i, _ in model}) >= 3

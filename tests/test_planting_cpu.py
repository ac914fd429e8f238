"""The planted layouts of tests/planting.py do what they claim, checked against the oracle
alone (no GPU): every planted end is a chunk end where the layout says so, the tails and
flushes of C have their level and length, D's strips hold exactly their counts, F's boundaries
are a plain greedy walk's, the rejected windows of (20, 16) end nothing, and A and B cover
every (nfull, block, parity) and every byte."""
import numpy as np
import pytest

import planting as P


def _ends(oracle, table, d, bits, min_size):
    return set(P.chunk_ends(oracle.split(table, d, bits=bits, min_size=min_size, with_refs=False)))


def test_zero_windows_exact_tz(oracle, table):
    for low, tz in ((12, None), (16, None), (20, None), (22, None), (16, 16), (12, 15), (20, 23)):
        for w in P.windows(table, low, tz):
            d = np.concatenate([np.zeros(100, np.uint8), w])
            h = int(oracle.rolling_sums(table, d)[-1])
            assert h & ((1 << low) - 1) == 0
            if tz is not None:
                assert h >> tz & 1 and h & ((1 << tz) - 1) == 0
            assert int(P.window_hashes(table, d, 163, 164)[0]) == h
    # the closed form agrees with the oracle at a stream's head too (zero history)
    d = np.random.default_rng(5).integers(0, 256, 300, dtype=np.uint8)
    assert P.window_hashes(table, d, 0, 300).tolist() == oracle.rolling_sums(table, d).tolist()


def test_plant_rejects_overlap_and_short():
    d = np.zeros(500, np.uint8)
    w = [np.ones(64, np.uint8)] * 2
    P.plant(d, [63, 127], w)
    with pytest.raises(AssertionError):
        P.plant(d, [100, 163], w)
    with pytest.raises(AssertionError):
        P.plant(d, [62], w[:1])


def test_coverage_a_b():
    a = P.a_cases()
    want = {(nf, b, par) for nf in range(1, 33) for b in range(nf) for par in (0, 1)}
    assert {(nf, b, k & 1) for nf, b, k in a} == want and len(a) == len(want) == 1056
    for c in range(4):
        assert {k for _, b, k in a if b % 4 == c} == set(range(64)), c
    # neighbours differ in nfull while more than one nfull has cases left
    same = sum(x[0] == y[0] for x, y in zip(a, a[1:]))
    assert same <= 64, same
    b = P.b_cases()
    assert len(b) == 640
    for nf in P.B_NFULL:
        assert sorted(k for n2, blk, k in b if n2 == nf and blk == nf - 1) == list(range(64))


@pytest.mark.parametrize("bits,low", P.PARAMS)
@pytest.mark.parametrize("layout", ["a", "b"])
def test_last_strip_layouts(oracle, table, layout, bits, low):
    streams, ends, cases = (P.layout_a if layout == "a" else P.layout_b)(table, bits, low)
    assert (1080 <= len(streams) <= 1120) if layout == "a" else len(streams) == 640
    for d, e, c in zip(streams, ends, cases):
        if c is None:
            assert len(d) % P.STRIP == 0 and not e
            continue
        nfull, b, k = c
        last = len(d) - (len(d) - 1) // P.STRIP * P.STRIP     # bytes in the last strip
        assert (last >> 6, last & 63) == (nfull, 0)
        assert e == [len(d) - last + 64 * b + k]
        assert set(e) <= _ends(oracle, table, d, bits, 64), c


@pytest.mark.parametrize("layout", ["a", "b", "d"])
def test_rejected_windows_end_nothing(oracle, table, layout):
    bits, low = P.REJECT
    streams, ends = {"a": P.layout_a, "b": P.layout_b, "d": P.layout_d}[layout](table, bits, low)[:2]
    for d, e in zip(streams, ends):
        sums = oracle.rolling_sums(table, d)
        for p in e:   # the 16-bit pre-filter fires, the exact test rejects
            assert int(sums[p]) & 0xFFFF == 0 and int(sums[p]) & 0xFFFFF != 0
        got = _ends(oracle, table, d, bits, 64)
        assert not (set(e) - {len(d) - 1}) & got


@pytest.mark.parametrize("bits,low", P.PARAMS)
def test_tails_and_flush(oracle, table, bits, low):
    streams, ends, cases = P.layout_c_tails(table, bits)
    assert len(streams) == 3 * (1 + sum(P.C_REM))
    seen = set()
    for d, e, (rem, n, t) in zip(streams, ends, cases):
        assert len(d) & 63 == rem and ((len(d) - 1) % P.STRIP + 1) >> 6 in (n, 32)
        ch = oracle.split(table, d, bits=bits, min_size=64)
        assert e[0] in P.chunk_ends(ch), (rem, n, t)
        seen.add((rem, n, len(d) - 1 - e[0]))
        if e[0] == len(d) - 1:   # the last byte: emitted by the per-byte rule, level 3
            assert int(ch[-1]["level"]) == P.C_LEVEL and int(ch[-1]["len"]) >= 64
    for rem in P.C_REM:   # every tail offset, the last byte included
        for n in P.C_N:
            assert {x for r, m, x in seen if (r, m) == (rem, n)} == set(range(rem))
    streams, ends, cases = P.layout_c_close(table, bits)
    assert len(streams) == 2 * 3 * (1 + len(P.C_REM))
    for d, e, (rem, n, kind) in zip(streams, ends, cases):
        assert len(d) & 63 == rem and e[-1] == len(d) - 1
        ch = oracle.split(table, d, bits=bits, min_size=P.C_CLOSE_MIN)
        assert int(ch[-1]["level"]) == P.C_LEVEL, (rem, n, kind)
        assert set(e) <= set(P.chunk_ends(ch))
        if kind == "long":
            assert int(ch[-1]["len"]) >= P.C_CLOSE_MIN
        else:   # below MinSize: only Close's flush emits it
            assert int(ch[-1]["len"]) == 128 < P.C_CLOSE_MIN


@pytest.mark.parametrize("bits,low", P.PARAMS)
def test_slot_limit_counts(oracle, table, bits, low):
    for build, over in ((P.layout_d, 4), (P.layout_d_control, 0)):
        (d,), (ends,), per_strip = build(table, bits, low)
        pos = P.candidate_positions(oracle, table, d, bits)
        assert pos.tolist() == sorted(ends)
        counts = np.bincount(pos // P.STRIP, minlength=len(per_strip)).tolist()
        assert counts == per_strip
        assert all(b - a >= 64 for a, b in zip(ends, ends[1:]))
        assert len(d) % P.STRIP == P.D_SHORT
        counts[-1] += 1   # the forced final candidate
        assert sum(c > 4 for c in counts) == over
        assert P.expected_candidates(oracle, table, d, bits) == len(ends) + 1
        assert set(ends) <= _ends(oracle, table, d, bits, 64)
        if over:   # MinSize 1024 drops most of them
            assert len(_ends(oracle, table, d, bits, 1024)) < len(ends) // 3


@pytest.mark.parametrize("bits,low", [(16, 16), (12, 12)])
@pytest.mark.parametrize("tile", [4096, 5000])
def test_tile_heads(oracle, table, tile, bits, low):
    (d,), (ends,), tile, writes, heads = P.layout_e(table, bits, low, tile)
    assert sum(writes) == len(d) and len(d) % tile and set(writes) - {writes[-1]} <= set(P.E_WRITES)
    assert {s for _, s in heads} == set(range(65)) and ends == [e for e, _ in heads]
    for e, s in heads:   # s bytes of the window lie in the tile before
        assert ((e - 63) + s) % tile == 0 and (e - 63) + s >= tile
    assert set(ends) <= _ends(oracle, table, d, bits, 64)


@pytest.mark.parametrize("tile", [4096, 5000])
def test_tile_heads_min_size(oracle, table, tile):
    """min_size = 1024 with a helper window before every tile head: the head's end is kept or
    dropped by the start of the open chunk, which lies in the tile before."""
    (d,), (ends,), tile, _, heads = P.layout_e(table, 16, 16, tile, helpers=True)
    assert len(ends) == 2 * len(heads)
    ch = oracle.split(table, d, bits=16, min_size=1024, with_refs=False)
    got = set(P.chunk_ends(ch))
    starts = sorted(int(c["offset"]) for c in ch)
    kept = dropped = 0
    for e, s in heads:
        first = e - 63 + s                              # the tile's first byte
        open_start = max(o for o in starts if o <= e)   # start of the chunk that holds e
        assert open_start < first
        if e in got:
            kept += 1
            assert e + 1 - open_start >= 1024
        else:
            dropped += 1
            assert e + 1 - open_start < 1024
    assert kept >= 20 and dropped >= 20, (kept, dropped)


@pytest.mark.parametrize("bits,low", P.PARAMS)
@pytest.mark.parametrize("min_size", [128, 1024])
def test_exact_spacing_is_a_greedy_walk(oracle, table, min_size, bits, low):
    (d,), (ends,) = P.layout_f(table, bits, low, min_size)
    gaps = np.diff(ends).tolist()
    assert {min_size - 1, min_size, min_size + 1} <= set(gaps) and min(gaps) >= 64
    pos = P.candidate_positions(oracle, table, d, bits)
    assert set(ends) <= set(pos.tolist())
    ch = oracle.split(table, d, bits=bits, min_size=min_size, with_refs=False)
    assert P.greedy_walk(pos, len(d), min_size) == P.chunk_ends(ch)
    kept = set(P.chunk_ends(ch)) & set(ends)   # the spacing both keeps and drops planted ends
    assert len(ends) // 4 < len(kept) < len(ends)

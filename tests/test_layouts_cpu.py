"""tests/layouts.py held to its claims (no GPU): alignment, declared overlaps, poison outside the
streams only, expected_region against a brute-force rule at the region borders, and the sparse
layouts' chunk counts (C oracle) on the intended side of the jobs-per-region threshold."""
import numpy as np
import pytest

import layouts as LY
from bs_amd.synth import splitmix_array


@pytest.mark.parametrize("name", LY.SMALL)
def test_small_layouts_shape(name):
    size, streams, desc = LY.build(name)
    assert desc and size <= 4 << 20
    assert all(o % 16 == 0 for o, _, _ in streams)
    assert max(o + n for o, n, _ in streams) + LY.READ_SLACK == size
    assert set(LY.LENS) <= {n for _, n, _ in streams}
    assert len(streams) <= 65535


def _overlap(a, b):
    return max(0, min(a[0] + a[1], b[0] + b[1]) - max(a[0], b[0]))


def test_gaps_and_orders():
    _, g, _ = LY.gaps()
    offs = [o for o, _, _ in g]
    assert offs == sorted(offs)
    seen = [g[i + 1][0] - LY.align16(g[i][0] + g[i][1]) for i in range(len(g) - 1)]
    assert set(seen) == set(LY.GAPS) and [n for _, n, _ in g] == LY.LENS
    for i in range(len(g)):
        for j in range(i + 1, len(g)):
            assert _overlap(g[i], g[j]) == 0
    _, d, _ = LY.descending()
    assert d == g[::-1] and [o for o, _, _ in d] == sorted(offs, reverse=True)
    _, s, _ = LY.shuffled()
    assert sorted(s) == sorted(g) and s != g and s != d


def test_aliased_relations_are_real():
    _, s, _ = LY.aliased()
    a, b = (s[i] for i in LY.ALIAS_SAME)
    assert a[:2] == b[:2] and a[1] == 70_001
    a, b = (s[i] for i in LY.ALIAS_PREFIX)
    assert a[0] == b[0] and 0 < b[1] < a[1]
    a, b = (s[i] for i in LY.ALIAS_INTERIOR)
    assert a[0] < b[0] and b[0] + b[1] < a[0] + a[1] and (b[0] - a[0]) % 16 == 0
    a, b = (s[i] for i in LY.ALIAS_TAIL)
    assert a[0] < b[0] < a[0] + a[1] < b[0] + b[1]
    assert _overlap(a, b) == a[0] + a[1] - b[0]
    # every LENS length also lies on aliased bytes
    o = a[0]
    assert {n for p, n, _ in s[14:] if p == o} == set(LY.LENS[:-1])


def test_empties_positions():
    _, s, _ = LY.empties()
    e = [s[i] for i in LY.EMPTY_AT]
    assert all(n == 0 for _, n, _ in e)
    nonempty = [x for x in s if x[1]]
    assert e[0][0] == 0 and LY.EMPTY_AT[0] == 0                      # at the start
    assert any(e[1][0] == o for o, _, _ in nonempty)                  # on a non-empty one's off
    assert all(not (o <= e[2][0] < o + n) for o, n, _ in nonempty)    # in a gap ...
    assert min(o for o, _, _ in nonempty) < e[2][0] < max(o for o, _, _ in nonempty)
    last = max(nonempty, key=lambda x: x[0] + x[1])
    assert e[3][0] == LY.align16(last[0] + last[1])                   # at the last one's end
    assert LY.EMPTY_AT[-1] == len(s) - 1


@pytest.mark.parametrize("name", LY.SMALL)
def test_fill_streams_and_poison(name):
    lay = LY.build(name)
    size, streams, _ = lay
    inside = LY.covered(lay)
    assert inside.any() and not inside[-LY.READ_SLACK:].any()
    bufs = {p: LY.fill(lay, p) for p in LY.POISONS}
    for p, buf in bufs.items():
        assert buf.dtype == np.uint8 and buf.size == size
        for o, n, seed in streams:  # the poison never lands inside a stream, aliases agree
            assert (buf[o:o + n] == splitmix_array(seed, n)).all(), (name, p, o, n)
    assert (bufs[0x00][~inside] == 0).all() and (bufs[0xFF][~inside] == 0xFF).all()
    assert (bufs[0x00][inside] == bufs[0xFF][inside]).all()
    assert (bufs["random"][inside] == bufs[0xFF][inside]).all()
    r = bufs["random"][~inside]
    assert len(np.unique(r)) > 200  # neither constant


def test_pieces_match_fill():
    lay = LY.build("aliased")
    for p in LY.POISONS:
        full = LY.fill(lay, p)
        got = np.full(lay[0], 0x5A, dtype=np.uint8)
        touched = np.zeros(lay[0], dtype=bool)
        for lo, b in LY.pieces(lay, p):
            got[lo:lo + len(b)] = b
            assert not touched[lo:lo + len(b)].any()
            touched[lo:lo + len(b)] = True
        assert (got[touched] == full[touched]).all()
        for o, n, _ in lay[1]:
            assert touched[o:o + n + LY.READ_SLACK].all()


def test_sub_seed():
    a = splitmix_array(77, 4096)
    for k in (0, 8, 16, 2048, 4000):
        assert (splitmix_array(LY.sub_seed(77, k), 4096 - k) == a[k:]).all()


def _brute_region(o, R, span):
    """job_region restated the slow way: the last r whose border ceil(r * span / R) is <= o."""
    if o <= 0 or R <= 1:
        return 0
    r = 0
    while r + 1 < R and -(-(r + 1) * span // R) <= o:
        r += 1
    return r


@pytest.mark.parametrize("span", [LY.REGION_BYTES + 1, 3 * LY.GIB // 2, 2581174672,
                                  (1 << 32) + (4 << 20) + 7, LY.SPARSE_SIZE])
def test_expected_region_at_borders(span):
    for R in (1, 2, 3, 5, 7, 64):
        assert LY.expected_region(0, R, span) == 0
        assert LY.expected_region(-16, R, span) == 0
        assert LY.expected_region(span - 1, R, span) == R - 1
        assert LY.expected_region(span, R, span) == R - 1      # the clamp
        assert LY.expected_region(span + 4096, R, span) == R - 1
        for r in range(1, R):
            b = -(-r * span // R)  # the first offset of region r
            for o in (b - 17, b - 16, b - 1, b, b + 1, b + 16):
                want = _brute_region(o, R, span)
                assert LY.expected_region(o, R, span) == want, (o, R, span)
            assert LY.expected_region(b - 1, R, span) == r - 1
            assert LY.expected_region(b, R, span) == r


def test_expected_nregions():
    assert LY.expected_nregions(LY.REGION_BYTES, 10**6) == 1
    assert LY.expected_nregions(LY.REGION_BYTES + 1, 8191) == 1
    assert LY.expected_nregions(LY.REGION_BYTES + 1, 8192) == 2
    assert LY.expected_nregions(5 * LY.GIB, 4096 * 5 - 1) == 4
    assert LY.expected_nregions(300 * LY.GIB, 10**7) == 64
    assert LY.expected_nregions(300 * LY.GIB, 10**7, waves=16 * 300) == 256


SPARSE_R = {"three_groups": 3, "empty_region": 3, "last_region": 3, "border_inside": 2,
            "past_4gib": 5, "few_jobs": 1}


@pytest.mark.parametrize("case", LY.SPARSE)
def test_sparse_layouts_sides_of_the_threshold(case, oracle, table):
    """The oracle's chunk counts put every sparse case on the intended side of the 4,096 jobs
    per region threshold, with no chunk long enough for the wave path (64 KiB)."""
    size, streams, _ = LY.sparse(case)
    assert all(o % 16 == 0 for o, _, _ in streams)
    span = LY.span_of(streams)
    assert span > LY.REGION_BYTES and span + LY.READ_SLACK <= size
    jobs, longest = 0, 0
    for o, n, seed in streams:
        ch = oracle.split(table, splitmix_array(seed, n), bits=8, min_size=64, with_refs=False)
        jobs += len(ch)
        longest = max(longest, int(ch["len"].max()))
    assert longest + 9 <= 1023 * 64
    R = LY.expected_nregions(span, jobs)
    assert R == SPARSE_R[case], (jobs, span)
    if case == "few_jobs":
        assert jobs < 2 * LY.MIN_REGION_JOBS
    else:  # enough jobs: the span alone sets R
        assert jobs // LY.MIN_REGION_JOBS >= R == -(-span // LY.REGION_BYTES)

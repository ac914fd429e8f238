"""k_scan and k_select against the oracle with candidates planted at chosen positions
(tests/planting.py; test_planting_cpu.py shows that the layouts hold what they claim).

Random input at Bits = 16 has one candidate per 64 KiB, so the places where the scan can be
subtly wrong never hold one in the suite's small inputs. Here every such place does:

  A  every (nfull, block, byte parity) of a last strip, block counts mixed within a wave (the
     WIDE asm pass's exec-mask drop-out, its hit bit (1 << i) << b, the paired 16-bit pre-filter)
  B  every byte of the last block
  C  every offset of a tail (exact_block's non-FULL branch) and Close's flush, level 3
  D  strips of 3, 4, 5, 6 and 31 candidates: kSlotCap slots, k_compact, k_rescan
  E  windows with 0..64 bytes in the previous streaming tile (StreamDesc::hist, open_start)
  F  gaps of MinSize - 1, MinSize, MinSize + 1 (k_select's sync points), across tiles too

Each case compares the records (offset, len, level, ref, stream) with oracle.split's, stream
by stream; Engine runs also compare Engine.candidates (Counters::ncand) with the oracle's count,
so that a phantom or doubled candidate that selection happens to drop still shows. (12, 12)
runs the narrow compiled loop (the control), (20, 16) has the pre-filter fire and the exact
test reject.
"""
import numpy as np
import pytest

import planting as P

pytestmark = pytest.mark.gpu

ALL = P.PARAMS + [P.REJECT]
_CACHE = {}


def _layout(key, build):
    """Each layout is built once, and its oracle records and counts computed once, per session."""
    if key not in _CACHE:
        _CACHE[key] = {"L": build(), "want": {}, "ncand": {}}
    return _CACHE[key]


def _tuples(ch, stream):
    return [(int(c["offset"]), int(c["len"]), int(c["level"]), bytes(c["ref"]).hex(), stream)
            for c in ch]


def _got_tuples(ch):
    return [(int(c["offset"]), int(c["len"]), int(c["level"]), bytes(c["ref"]).hex(),
             int(c["stream"])) for c in ch]


def _want(ent, oracle, table, bits, min_size):
    k = (bits, min_size)
    if k not in ent["want"]:
        ent["want"][k] = [_tuples(oracle.split(table, d, bits=bits, min_size=min_size), i)
                          for i, d in enumerate(ent["L"][0])]
    return ent["want"][k]


def _ncand(ent, oracle, table, bits):
    if bits not in ent["ncand"]:
        ent["ncand"][bits] = sum(P.expected_candidates(oracle, table, d, bits)
                                 for d in ent["L"][0])
    return ent["ncand"][bits]


def _compare(got, counts, want, cases, what):
    k = 0
    for i, w in enumerate(want):
        g = got[k:k + int(counts[i])]
        k += int(counts[i])
        assert g == w, (what, "stream", i, "case", cases[i] if cases else None,
                        "wanted", w[-3:], "got", g[-3:])
    assert k == len(got)


def _run_batch(gpu, streams, bits, min_size):
    ch, counts = gpu.split_hash_batch(streams, bits=bits, min_size=min_size)
    return _got_tuples(ch), counts


def _run_engine(gpu, streams, bits, min_size):
    """Device-resident run: streams packed at 16-byte aligned offsets of one buffer. Returns
    (records, counts, Engine.candidates, strips sent to k_rescan)."""
    off, o = [], 0
    for d in streams:
        off.append(o)
        o += (len(d) + 15) & ~15
    host = np.zeros(max(o, 16), dtype=np.uint8)
    for d, p in zip(streams, off):
        host[p:p + len(d)] = d
    buf = gpu.DeviceBuffer(host.size)
    eng = gpu.Engine()
    try:
        buf.from_host(host)
        eng.run(buf.ptr, off, [len(d) for d in streams], bits=bits, min_size=min_size)
        eng.finish()
        return _got_tuples(eng.chunks()), eng.counts(), int(eng.candidates), eng.rescan_strips
    finally:
        eng.close()
        buf.free()


def _run_streaming(gpu, data, bits, min_size, tile, carry_cap, writes):
    w = gpu.StreamingSplitter(bits=bits, min_size=min_size, tile=tile, carry_cap=carry_cap)
    try:
        got, p = [], 0
        for n in writes:
            w.write(data[p:p + n])
            p += n
            got.append(w.drain())
        assert p == len(data)
        w.close()
        got.append(w.drain())
    finally:
        w.free()
    return _got_tuples(np.concatenate(got))


def _check_both(gpu, oracle, table, ent, path, bits, min_size, what):
    streams, _, cases = ent["L"][:3]
    want = _want(ent, oracle, table, bits, min_size)
    if path == "batch":
        got, counts = _run_batch(gpu, streams, bits, min_size)
    else:
        got, counts, ncand, _ = _run_engine(gpu, streams, bits, min_size)
    _compare(got, counts, want, cases, what)
    if path == "engine":
        assert ncand == _ncand(ent, oracle, table, bits), what


# --------------------------------------------------------------------------------------------
# A, B: the last strip
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["batch", "engine"])
@pytest.mark.parametrize("bits,low", ALL)
def test_a_mixed_nfull(gpu, oracle, table, bits, low, path):
    """cases: (nfull, b, k), the window ends at byte k of block b of a last strip of nfull blocks."""
    ent = _layout(("a", bits, low), lambda: P.layout_a(table, bits, low))
    _check_both(gpu, oracle, table, ent, path, bits, 64, ("A", bits, low, path))


@pytest.mark.parametrize("path", ["batch", "engine"])
@pytest.mark.parametrize("bits,low", ALL)
def test_b_last_block_bytes(gpu, oracle, table, bits, low, path):
    ent = _layout(("b", bits, low), lambda: P.layout_b(table, bits, low))
    _check_both(gpu, oracle, table, ent, path, bits, 64, ("B", bits, low, path))


# --------------------------------------------------------------------------------------------
# C: tails and the final flush
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,low", P.PARAMS)
def test_c_tail_offsets(gpu, oracle, table, bits, low):
    """cases: (rem, n, t), the window ends at offset t of the rem-byte tail (t = -1, rem = 0: on
    the last byte of a stream without a tail)."""
    ent = _layout(("c1", bits), lambda: P.layout_c_tails(table, bits))
    want = _want(ent, oracle, table, bits, 64)
    for w, e, d in zip(want, ent["L"][1], ent["L"][0]):
        if e[0] == len(d) - 1:   # the oracle's final record: level 3, at least MinSize
            assert w[-1][2] == P.C_LEVEL and w[-1][1] >= 64
    _check_both(gpu, oracle, table, ent, "engine", bits, 64, ("C tails", bits))


@pytest.mark.parametrize("bits,low", P.PARAMS)
def test_c_close_flush(gpu, oracle, table, bits, low):
    """cases: (rem, n, kind): "long", the per-byte rule emits the final chunk; "short", the
    final chunk is below MinSize and only Close emits it, its level from the same hash."""
    ent = _layout(("c2", bits), lambda: P.layout_c_close(table, bits))
    want = _want(ent, oracle, table, bits, P.C_CLOSE_MIN)
    for w, (rem, n, kind) in zip(want, ent["L"][2]):
        assert w[-1][2] == P.C_LEVEL
        assert (w[-1][1] >= P.C_CLOSE_MIN) == (kind == "long")
    _check_both(gpu, oracle, table, ent, "engine", bits, P.C_CLOSE_MIN, ("C close", bits))
    _check_both(gpu, oracle, table, ent, "batch", bits, P.C_CLOSE_MIN, ("C close", bits))


# --------------------------------------------------------------------------------------------
# D: the slot limit
# --------------------------------------------------------------------------------------------
D_CASES = [(b, l, m) for b, l in P.PARAMS for m in (64, 1024)] + [P.REJECT + (64,)]


@pytest.mark.parametrize("bits,low,min_size", D_CASES)
def test_d_slot_limit(gpu, oracle, table, bits, low, min_size):
    """Strips of 3, 4, 5, 6, 31 and (short, with the forced final candidate) 5 + 1 candidates.
    The four strips above kSlotCap = 4 go through k_rescan<WRITE>: the run's candidates (55)
    are far below the engine's smallest candidate buffer (65,536 entries, plan_split), so it is
    not the overflow re-run that finds them."""
    ent = _layout(("d", bits, low), lambda: P.layout_d(table, bits, low))
    streams, _, per_strip = ent["L"]
    want = _want(ent, oracle, table, bits, min_size)
    got, counts, ncand, rescan = _run_engine(gpu, streams, bits, min_size)
    _compare(got, counts, want, None, ("D", bits, low, min_size, per_strip))
    assert ncand == _ncand(ent, oracle, table, bits)
    if low >= bits:
        assert ncand == sum(per_strip) + 1 < 65536
        assert rescan == 4
    else:
        assert ncand == 1 and rescan == 0
    got, counts = _run_batch(gpu, streams, bits, min_size)
    _compare(got, counts, want, None, ("D batch", bits, low, min_size))


@pytest.mark.parametrize("bits,low", [(16, 16), (12, 12)])
def test_d_control_no_rescan(gpu, oracle, table, bits, low):
    """At most kSlotCap candidates in every strip: nothing is scanned again."""
    ent = _layout(("d0", bits, low), lambda: P.layout_d_control(table, bits, low))
    streams, _, per_strip = ent["L"]
    want = _want(ent, oracle, table, bits, 64)
    got, counts, ncand, rescan = _run_engine(gpu, streams, bits, 64)
    _compare(got, counts, want, None, ("D control", bits, per_strip))
    assert ncand == sum(per_strip) + 1 == _ncand(ent, oracle, table, bits)
    assert rescan == 0


# --------------------------------------------------------------------------------------------
# E: tile heads and tile ends, streaming
# --------------------------------------------------------------------------------------------
E_CASES = [(16, t, c, 64) for t in (4096, 5000) for c in (None, 0, 3000)] + \
          [(16, 4096, None, 1024), (16, 5000, 0, 1024), (12, 4096, None, 64)]


@pytest.mark.parametrize("bits,tile,carry_cap,min_size", E_CASES)
def test_e_tile_heads(gpu, oracle, table, bits, tile, carry_cap, min_size):
    """Tile j holds a window with (j - 1) mod 65 of its bytes in tile j - 1. min_size 1024: one
    more window before each (layout_e's helpers), so whether the end at the tile head is kept
    depends on open_start carried from the tile before."""
    helpers = min_size != 64
    ent = _layout(("e", bits, tile, helpers),
                  lambda: P.layout_e(table, bits, bits, tile, helpers=helpers))
    (d,), (ends,), tile, writes, heads = ent["L"]
    want = _want(ent, oracle, table, bits, min_size)[0]
    want_ends = {o + n - 1 for o, n, *_ in want}
    if min_size == 64:
        assert set(ends) <= want_ends
    else:   # the helper windows make the oracle keep some tile-head ends and drop others
        kept = sum(e in want_ends for e, _ in heads)
        assert 20 <= kept <= len(heads) - 20
    got = _run_streaming(gpu, d, bits, min_size, tile, carry_cap, writes)
    bad = next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
    assert got == want, ("E", bits, tile, carry_cap, min_size, "first difference at record", bad,
                         "wanted", want[bad:bad + 2], "got", got[bad:bad + 2])


# --------------------------------------------------------------------------------------------
# F: exact MinSize spacing
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_size", [128, 1024])
@pytest.mark.parametrize("bits,low", P.PARAMS)
def test_f_exact_spacing(gpu, oracle, table, bits, low, min_size):
    ent = _layout(("f", bits, low, min_size), lambda: P.layout_f(table, bits, low, min_size))
    streams = ent["L"][0]
    want = _want(ent, oracle, table, bits, min_size)
    got, counts, ncand, _ = _run_engine(gpu, streams, bits, min_size)
    _compare(got, counts, want, None, ("F", bits, min_size))
    assert ncand == _ncand(ent, oracle, table, bits)
    got, counts = _run_batch(gpu, streams, bits, min_size)
    _compare(got, counts, want, None, ("F batch", bits, min_size))


@pytest.mark.parametrize("carry_cap", [0, None])
def test_f_exact_spacing_streaming(gpu, oracle, table, carry_cap):
    """The min_size = 128 stream in 4,096-byte tiles: walks cross tile boundaries."""
    ent = _layout(("f", 16, 16, 128), lambda: P.layout_f(table, 16, 16, 128))
    (d,) = ent["L"][0]
    want = _want(ent, oracle, table, 16, 128)[0]
    got = _run_streaming(gpu, d, 16, 128, 4096, carry_cap, P.write_sizes(len(d), 31))
    assert got == want, ("F streaming", carry_cap)

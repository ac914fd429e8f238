"""The early chains (k_pick, k_early, k_early_fix, k_lens's match) on small planted
runs: which chunks are picked, and the chains at their edges.

An engine takes early chains from 256 MiB on; Engine.set_early_min(0) (test tooling) lets the runs
of tests/early_cases.py, a few hundred KiB each, take them. test_early_cases_cpu.py shows that
every case holds what it claims. For every case here, with exact equality throughout:

  * the records, the counts per stream and Engine.candidates equal the oracle's with KNOB_EARLY on
    and off;
  * with the knob on, Engine.early_picks() equals the model's picks (early_cases.model_picks over
    the oracle's candidates): the block count and the candidate index k_pick left in Early::top,
    and the record index k_lens left in Early::idx; Engine.tiers()["early"] has the same slots;
  * with the knob off, or with the engine's own threshold, there are no picks.

The families: (a) the two longest of five; (b) the 1,024-block floor; (c) a start that is a
boundary but not a sure one, at gaps MinSize - 1, MinSize, MinSize + 1; (d) a candidate just
inside the chunk; (e) the forced end, with and without a natural candidate on the last byte, a
one-chunk stream, a first chunk; (f) three streams at descending, gapped offsets; (g) ties;
(h) adjacent picks; (i) one pick and none; (j) the two winners in one wave, two waves, two
workgroups and one thread of k_pick's grid, and mirrored; (k) chains of 1,024 to 1,153 blocks
with every tail; (l) every start residue mod 64; (m) levels 0, 5 and tz = 31."""
import contextlib
import ctypes

import numpy as np
import pytest

import early_cases as C

pytestmark = pytest.mark.gpu
C_U64P = ctypes.POINTER(ctypes.c_uint64)


def _tuples(ch):
    return [(int(c["offset"]), int(c["len"]), int(c["level"]), bytes(c["ref"]).hex(),
             int(c["stream"])) for c in ch]


def _result(eng):
    return {"records": _tuples(eng.chunks()), "counts": [int(x) for x in eng.counts()],
            "ncand": int(eng.candidates), "picks": eng.early_picks(),
            "early": eng.tiers()["early"]}


def _split(eng, buf, case):
    eng.run(buf.ptr, case.off, case.lens, bits=case.bits, min_size=case.min_size)
    eng.finish()
    return _result(eng)


@contextlib.contextmanager
def _device(gpu, case):
    host = case.buffer()
    buf = gpu.DeviceBuffer(host.size)
    try:
        buf.from_host(host)
        yield buf
    finally:
        buf.free()


def _fresh(gpu, buf, case, early_min=0):
    eng = gpu.Engine()
    try:
        if early_min is not None:
            eng.set_early_min(early_min)
        return _split(eng, buf, case)
    finally:
        eng.close()


def _check(got, want, picks, what):
    bad = next((i for i, (g, w) in enumerate(zip(got["records"], want["records"])) if g != w),
               min(len(got["records"]), len(want["records"])))
    assert got["records"] == want["records"], (what, "first difference at record", bad,
                                               want["records"][bad:bad + 1],
                                               got["records"][bad:bad + 1])
    assert got["counts"] == want["counts"], what
    assert got["ncand"] == want["ncand"], what
    assert got["picks"] == picks, (what, "picks", got["picks"], "model", picks)
    assert got["early"] == (len(picks) >= 1, len(picks) >= 2), what


def _run_case(gpu, oracle, table, name, light=None):
    case = C.get(table, name)
    want = C.expect(case, oracle, table)
    stack = contextlib.ExitStack()
    with stack, _device(gpu, case) as buf:
        if light is not None:
            stack.enter_context(gpu.debug_knob(gpu.KNOB_LIGHT_BYTES, light))
        with gpu.debug_knob(gpu.KNOB_EARLY, 1):
            on = _fresh(gpu, buf, case)
            default = _fresh(gpu, buf, case, early_min=None)
        with gpu.debug_knob(gpu.KNOB_EARLY, 0):
            off = _fresh(gpu, buf, case)
    print(name, "bytes", sum(case.lens), "candidates", on["ncand"], "picks", on["picks"])
    _check(on, want, want["picks"], (name, "early on"))
    _check(off, want, [], (name, "early off"))
    _check(default, want, [], (name, "default threshold"))
    assert on["records"] == off["records"] == default["records"]
    return on


@pytest.mark.parametrize("name", C.NAMES)
def test_case(gpu, oracle, table, name):
    on = _run_case(gpu, oracle, table, name)
    case = C.get(table, name)
    # the picks are the chunks the case intends (the CPU tests tie the model to them)
    assert [on["records"][r][:2] + (on["records"][r][4],) for _, _, r in on["picks"]] == \
        [(start, length, s) for s, start, length in C.intended(case)]


@pytest.mark.parametrize("name", ["a-basic", "f-stream-edges"])
def test_case_loaded_schedule(gpu, oracle, table, name):
    """KNOB_LIGHT_BYTES 0: the chains on the second stream, selection on the engine's."""
    _run_case(gpu, oracle, table, name, light=0)


def test_engine_reuse(gpu, oracle, table):
    """One engine: a run with picks, one without, a hash run, the first again. Each equals a
    fresh engine's result and the oracle's; nothing of an earlier run's Early record shows."""
    a, none = C.get(table, "a-basic"), C.get(table, "i-none")
    wa, wn = C.expect(a, oracle, table), C.expect(none, oracle, table)
    assert len(wa["picks"]) == 2 and wn["picks"] == []
    with gpu.debug_knob(gpu.KNOB_EARLY, 1), _device(gpu, a) as ba, _device(gpu, none) as bn:
        fresh_a, fresh_n = _fresh(gpu, ba, a), _fresh(gpu, bn, none)
        eng = gpu.Engine()
        try:
            eng.set_early_min(0)
            first = _split(eng, ba, a)
            second = _split(eng, bn, none)
            eng.hash(ba.ptr, a.off, a.lens)
            assert eng.finish() == len(a.lens)
            hashed = [bytes(c["ref"]) for c in eng.chunks()]
            after_hash = (eng.early_picks(), eng.tiers()["early"])
            again = _split(eng, ba, a)
        finally:
            eng.close()
    _check(fresh_a, wa, wa["picks"], "fresh a")
    _check(fresh_n, wn, [], "fresh none")
    _check(first, wa, wa["picks"], "reused: a")
    _check(second, wn, [], "reused: none after a")
    _check(again, wa, wa["picks"], "reused: a after a hash run")
    assert first == fresh_a == again and second == fresh_n
    assert hashed == [oracle.sha256(d) for d in a.streams]
    assert after_hash == ([], (False, False))


def test_early_min_while_enqueued(gpu, table):
    """bsg_engine_early_min_debug and bsg_engine_early_picks_debug refuse a null engine and an
    engine with a run enqueued."""
    L = gpu.lib()
    out = np.zeros(4, dtype=np.uint64)
    assert L.bsg_engine_early_min_debug(None, 0) == -22
    assert L.bsg_engine_early_picks_debug(None, out.ctypes.data_as(C_U64P)) == -22
    case = C.get(table, "i-one")
    with _device(gpu, case) as buf:
        eng = gpu.Engine()
        try:
            eng.run(buf.ptr, case.off, case.lens, bits=case.bits, min_size=case.min_size)
            assert L.bsg_engine_early_min_debug(eng.h, 0) == -22
            assert L.bsg_engine_early_picks_debug(eng.h, out.ctypes.data_as(C_U64P)) == -22
            eng.finish()
            assert eng.early_picks() == []          # the engine's own threshold held
            eng.set_early_min(0)
        finally:
            eng.close()


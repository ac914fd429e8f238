"""The host tail (k_offload_pick, k_offload_gather, the hash workers, k_offload_fix) on
small planted runs. An engine hands chunks to the host from 512 MiB on; Engine.set_host_tail
(test tooling) lowers that to 0 and forces the cut, so runs of a few hundred KiB, built like the
early-chain cases (tests/early_cases.py), go through every kernel of the path. Every run's records
are compared field for field (offset, len, level, ref, stream) with the oracle's split of the same
bytes, and the counts per stream with the oracle's.

(a) three chunks far longer than the rest, the cut forced so that 0, 1, 3 and all chunks go to the
host; (b) with all chunks offloaded that includes the stream's first chunk, its forced final chunk
and chunks starting at offsets that are no multiple of 16; (c) offloaded lengths of 64k-9, 64k-8,
64k and 64k+1 bytes; (d) four streams with the offloaded chunks in streams 1 and 3; (e) a run that
would also take early chains: the tail takes their chunks, no early pick is made, every record is
written once; (f) the portable hash; (g) two runs without a finish between them; (h) the knob
off; (i) a ring that holds only the longest candidate; (j) a hash run behind an unfinished run with
a tail; (k) the cost model's own cut on a 512 MiB stream, the engine's own threshold."""
import pytest

import early_cases as C
import tail_cases as T

pytestmark = pytest.mark.gpu
L, _c = C.L, C._c
SHORT, _plan = T.SHORT, T.plan
_tuples, _device, _run, _result, _split, _check, _blocks = (T.tuples, T.device, T.run, T.result,
                                                            T.split, T.check, T.blocks)


def _cases():
    return {
        "three": T.three(),
        "edges": C.Case("tail-edges", [_plan([L(1200, 55), L(1300, 56), L(1400, 0), L(1500, 1)])],
                        102),
        "streams": C.Case("tail-streams", [_plan([]), _plan([L(1600, 7), L(1250, 56)]), _plan([]),
                                           _plan([L(1900, 0)], tail=("r", L(1100, 33)))], 103),
        "other": C.Case("tail-other", [_plan([L(1450, 9), L(1150, 63)])], 104),
    }


_BUILT = {}


@pytest.fixture(scope="module")
def cases(table, oracle):
    if not _BUILT:
        for k, c in _cases().items():
            c.build(table)
            _BUILT[k] = (c, C.expect(c, oracle, table))
    return _BUILT


@pytest.mark.parametrize("cut,chunks", [(5000, 0), (2000, 1), (1000, 3), (1, None)])
def test_forced_cut(gpu, cases, cut, chunks):
    """(a), (b)"""
    case, want = cases["three"]
    got = _split(gpu, case, force_cut=cut)
    print(cut, got["tail"])
    _check(got, want, ("cut", cut))
    lens = [r[1] for r in want["records"]]
    taken = [n for n in lens if _blocks(n) >= cut]
    assert got["tail"]["chunks"] == (len(lens) if chunks is None else chunks) == len(taken)
    assert got["tail"]["host_blocks"] == sum(_blocks(n) for n in taken)
    if chunks is None:     # the first chunk, the forced final one, starts off the 16-byte grid
        assert any(r[0] % 16 for r in want["records"])


def test_padding_edges(gpu, cases):
    """(c)"""
    case, want = cases["edges"]
    got = _split(gpu, case, force_cut=1000)
    _check(got, want, "edges")
    assert got["tail"]["chunks"] == 4
    assert sorted(r[1] % 64 for r in want["records"] if _blocks(r[1]) >= 1000) == [0, 1, 55, 56]


def test_four_streams(gpu, cases):
    """(d)"""
    case, want = cases["streams"]
    got = _split(gpu, case, force_cut=1000)
    _check(got, want, "streams")
    assert got["tail"]["chunks"] == 4
    assert {r[4] for r in want["records"] if _blocks(r[1]) >= 1000} == {1, 3}


def test_early_picks_above_cut(gpu, cases):
    """(e): with both thresholds at 0 the run's two early picks are chunks the host takes. The
    tail makes no early picks, so each record is written once, by k_offload_fix."""
    case, want = cases["three"]
    with gpu.debug_knob(gpu.KNOB_EARLY, 1):
        got = _split(gpu, case, early=True, force_cut=1000)
    _check(got, want, "early and tail")
    assert got["tail"]["chunks"] == 3 and got["early"] == (False, False)


def test_portable(gpu, cases):
    """(f)"""
    case, want = cases["three"]
    got = _split(gpu, case, force_cut=1000, portable=True)
    _check(got, want, "portable")
    assert got["tail"]["chunks"] == 3 and got["tail"]["impl"] == "portable"


def test_model_cut(gpu, cases):
    """The cost model's own cut on the planted run: whatever it takes, the records hold."""
    case, want = cases["three"]
    got = _split(gpu, case)
    print(got["tail"])
    _check(got, want, "model")


def test_back_to_back(gpu, cases):
    """(g): a second run enqueued before the first is finished completes the first one's tail;
    then a third the second one's. Each finish sees its own run's records."""
    a, wa = cases["three"]
    b, wb = cases["other"]
    with _device(gpu, a) as ba, _device(gpu, b) as bb:
        eng = gpu.Engine()
        try:
            eng.set_host_tail(0, force_cut=1000)
            _run(eng, ba, a)
            _run(eng, bb, b)
            eng.finish()
            second = _result(eng)
            _run(eng, bb, b)
            _run(eng, ba, a)
            eng.finish()
            first = _result(eng)
        finally:
            eng.close()
    _check(second, wb, "b after an unfinished a")
    _check(first, wa, "a after an unfinished b")
    assert second["tail"]["chunks"] == 2 and first["tail"]["chunks"] == 3


def test_knob_off(gpu, cases):
    """(h)"""
    case, want = cases["three"]
    with gpu.debug_knob(gpu.KNOB_HOST_TAIL, 0):
        got = _split(gpu, case, force_cut=1000)
    _check(got, want, "knob off")
    assert got["tail"]["chunks"] == 0 and got["tail"]["bytes"] == 0


def test_small_ring(gpu, cases):
    """(i): the ring holds the longest candidate alone; the other two stay on the GPU."""
    case, want = cases["three"]
    got = _split(gpu, case, force_cut=1000, ring_bytes=L(2050, 55) + 4096)
    _check(got, want, "small ring")
    assert got["tail"]["chunks"] == 1
    assert got["tail"]["longest_left_blocks"] == 1705


def test_hash_behind_unfinished_tail(gpu, oracle, cases):
    """(j): bsg_engine_hash enqueued behind a split run with a tail that was not finished. The
    hash run's refs are the blobs' own, nothing of the earlier tail is written over them or
    reported for them, and the engine's next split run is right again."""
    a, wa = cases["three"]
    b, _ = cases["streams"]
    with _device(gpu, a) as ba, _device(gpu, b) as bb:
        eng = gpu.Engine()
        try:
            eng.set_host_tail(0, force_cut=1000)
            _run(eng, ba, a)
            eng.hash(bb.ptr, b.off, b.lens)
            assert eng.finish() == len(b.lens)
            hashed = [bytes(c["ref"]) for c in eng.chunks()]
            tail = eng.diag()["host_tail"]
            _run(eng, ba, a)
            eng.hash(ba.ptr, a.off, a.lens)
            assert eng.finish() == len(a.lens)
            hashed_a = [bytes(c["ref"]) for c in eng.chunks()]
            _run(eng, ba, a)
            eng.finish()
            again = _result(eng)
        finally:
            eng.close()
    assert hashed == [oracle.sha256(d) for d in b.streams]
    assert hashed_a == [oracle.sha256(d) for d in a.streams]
    assert tail["chunks"] == 0 and tail["bytes"] == 0
    _check(again, wa, "a split run after the hash runs")
    assert again["tail"]["chunks"] == 3


def test_model_cut_512mib(gpu, oracle, table):
    """(k): one 512 MiB stream of random bytes, the engine's own threshold and the cost model's
    own cut (nothing forced). Its chunk lengths are near exponential with a mean of 64 KiB, so
    the longest (several hundred KB) is far above what the model leaves on the GPU: chunks go to
    the host, within the ring (1/8 of the run), the longest chunk left on the GPU is shorter than
    the run's longest, and the records equal the oracle's."""
    from bs_amd.synth import splitmix_array
    n, seed = 512 << 20, 0x7A11
    want = oracle.split(table, splitmix_array(seed, n))
    buf = gpu.DeviceBuffer(n)
    eng = gpu.Engine()
    try:
        gpu.fill_splitmix(buf.ptr, n, seed, stream=eng.stream)
        eng.run(buf.ptr, [0], [n])
        eng.finish()
        ch, tail = eng.chunks(), eng.diag()["host_tail"]
    finally:
        eng.close()
        buf.free()
    print(tail)
    assert len(ch) == len(want)
    for f in ("offset", "len", "level", "ref"):
        assert (ch[f] == want[f]).all(), f
    assert (ch["stream"] == 0).all()
    longest = _blocks(int(want["len"].max()))
    assert tail["longest_blocks"] == longest
    assert tail["chunks"] > 0 and 0 < tail["bytes"] <= n // 8
    assert tail["longest_left_blocks"] < longest
    taken = want["len"][(want["len"] + 8) // 64 + 1 > tail["longest_left_blocks"]]
    assert tail["chunks"] == len(taken)
    assert tail["host_blocks"] == int(((taken + 8) // 64 + 1).sum())

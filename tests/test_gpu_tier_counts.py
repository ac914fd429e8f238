"""k_sha's tier split and job queues at their count edges (k_lens, k_thresh, k_order,
k_bucket_scan, the ticket arithmetic of sha_wave_job), on the censuses of
tests/tier_cases.py. test_tier_cases_cpu.py shows that every case holds what it claims.

Per case: a fresh engine, a first run of the same layout over the complemented bytes (so the ref
a dropped job would leave behind is a wrong one), then the case. Every ref equals hashlib's
(cases I and J: every record the oracle's); `len` and `stream` are as given; Engine.diag() and
Engine.tiers() equal the model at waves = 4 x the device's CU count, and on a 256-CU part the
literals the case states; no early chain runs."""
import contextlib
import subprocess
import sys

import numpy as np
import pytest

import dedup_cases as D
import sha_edges as E
import tier_cases as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cus(gpu):
    """The device's CU count, from torch's device properties. Asked in a child process: torch
    ships its own HIP runtime, which a process that runs libbsgpu does not initialise."""
    out = subprocess.run(
        [sys.executable, "-c", "import torch; "
         "print(torch.cuda.get_device_properties(0).multi_processor_count)"],
        capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    n = int(out.stdout.split()[-1])
    assert 1 <= n <= 4096, out.stdout
    return n


@pytest.fixture(scope="module")
def bufs(gpu):
    """tier_cases.buffer() and its complement on the device."""
    host = T.buffer()
    plain, flipped = gpu.DeviceBuffer(T.BUF_BYTES), gpu.DeviceBuffer(T.BUF_BYTES)
    try:
        plain.from_host(host)
        flipped.from_host(~host)
        yield plain, flipped
    finally:
        plain.free()
        flipped.free()


def _hash_case(gpu, bufs, case):
    """(records, diag, tiers, the first run's refs) of `case` on a fresh engine."""
    plain, flipped = bufs
    eng = gpu.Engine()
    try:
        eng.hash(flipped.ptr, case.off, case.lens)
        assert eng.finish() == len(case.lens)
        stale = eng.chunks()["ref"].copy()
        eng.hash(plain.ptr, case.off, case.lens)
        assert eng.finish() == len(case.lens)
        return eng.chunks(), eng.diag(), eng.tiers(), stale
    finally:
        eng.close()


def _check_refs(case, ch, stale, m):
    want = np.frombuffer(b"".join(case.refs()), dtype=np.uint8).reshape(-1, 32)
    bad = np.nonzero((ch["ref"] != want).any(axis=1))[0]
    assert bad.size == 0, (case.name, len(bad), "wrong refs; (index, nblocks, tier by the model)",
                           [(int(i), case.blocks[i], m["tier"][i]) for i in bad[:12]])
    assert ch["len"].tolist() == case.lens
    assert ch["stream"].tolist() == list(range(len(case.lens)))
    assert not ch["offset"].any()
    # the first run left another ref in every record
    assert (stale != want).any(axis=1).all(), case.name


def _check_counts(name, diag, tiers, m, want, cus):
    got = T.reported(diag, tiers)
    print(name, "CUs", cus, got, "light" if m["light"] else "loaded")
    assert got == T.expected_report(m), (name, "device", got, "model", T.expected_report(m))
    assert diag["wave_tickets"] == tiers["wave_tickets"]
    if cus == T.constants()["num_cus"]:
        assert {k: got[k] for k in T.COUNTS} == want, (name, "literals", want)
    assert tiers["early"] == (False, False)


@pytest.mark.parametrize("name", T.NAMES)
def test_case(gpu, bufs, cus, name):
    case = T.get(name)
    m = T.model(case.blocks, T.waves(cus))
    ch, diag, tiers, stale = _hash_case(gpu, bufs, case)
    _check_refs(case, ch, stale, m)
    _check_counts(name, diag, tiers, m, case.want, cus)


@pytest.mark.parametrize("mode", sorted(T.H_MODE_WANT))
def test_sort_under_long_mode(gpu, bufs, cus, mode):
    """Case H with every job on a lane (KNOB_LONG_MODE 1) and every job on a solo or group
    ticket (2): 2,500 jobs of 2,500 different ranks in one queue."""
    case = T.get("H-sort")
    m = T.model(case.blocks, T.waves(cus), long_mode=mode)
    with gpu.debug_knob(gpu.KNOB_LONG_MODE, mode):
        ch, diag, tiers, stale = _hash_case(gpu, bufs, case)
    _check_refs(case, ch, stale, m)
    assert diag["nlong"] == (0 if mode == 1 else len(case.blocks))
    _check_counts(f"H-sort mode {mode}", diag, tiers, m, T.H_MODE_WANT[mode], cus)


# ---------------------------------------------------------------------------------------------
# Split runs
# ---------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _placed(gpu, streams):
    """The streams at 16-byte offsets on the device, and their complement: (plain, flipped, off,
    lens)."""
    host, off, lens = D.place(streams)
    plain, flipped = gpu.DeviceBuffer(host.size), gpu.DeviceBuffer(host.size)
    try:
        plain.from_host(host)
        flipped.from_host(~host)
        yield plain, flipped, off, lens
    finally:
        plain.free()
        flipped.free()


def _split_case(gpu, oracle, table, streams, bits, min_size, cus, what):
    want = D.oracle_records(oracle, table, streams, bits, min_size)
    with _placed(gpu, streams) as (plain, flipped, off, lens):
        eng = gpu.Engine()
        try:
            eng.run(flipped.ptr, off, lens, bits=bits, min_size=min_size)
            eng.finish()
            eng.run(plain.ptr, off, lens, bits=bits, min_size=min_size)
            assert eng.finish() == len(want), what
            got, counts, diag, tiers = eng.chunks(), eng.counts(), eng.diag(), eng.tiers()
        finally:
            eng.close()
    nb = [E.nblocks(n) for n in want["len"]]
    m = T.model(nb, T.waves(cus))
    bad = np.nonzero((got["ref"] != want["ref"]).any(axis=1))[0]
    assert bad.size == 0, (what, len(bad), "wrong refs; (record, nblocks, tier by the model)",
                           [(int(i), nb[i], m["tier"][i]) for i in bad[:12]])
    for f in ("offset", "len", "level", "stream"):
        assert (got[f] == want[f]).all(), (what, f)
    assert counts.tolist() == [int((want["stream"] == s).sum()) for s in range(len(streams))]
    return diag, tiers, m


@pytest.mark.parametrize("passes", T.I_PASSES)
def test_more_slots_than_a_grid_pass(gpu, oracle, table, cus, passes):
    """Case I: a split run whose job slots (records + streams) are one more than `passes` grid
    passes of k_lens / k_order: the last slot, the stream's, is alone in a pass of its own, and
    the last record is the last thread's of the pass before."""
    data, want = T.slots_stream(oracle, table, passes, cus)
    assert len(want) + 1 == passes * T.grid_slots(cus) + 1
    diag, tiers, m = _split_case(gpu, oracle, table, [data], T.I_BITS, T.I_MIN, cus,
                                 f"I passes {passes}")
    _check_counts(f"I-{passes}", diag, tiers, m, T._want(0, 0, 0, 0, len(want), 0), cus)


def test_planted_split_run(gpu, oracle, table, cus):
    """Case J: the split path's job list (43 records, then three stream slots without a job)
    with three helped solo chains and no group or pair ticket."""
    streams, lens = T.planted_run()
    diag, tiers, m = _split_case(gpu, oracle, table, streams, T.J_BITS, T.J_MIN, cus, "J")
    assert m["max_nblocks"] == max(T.J_LONG)
    _check_counts("J", diag, tiers, m, T.J_WANT, cus)

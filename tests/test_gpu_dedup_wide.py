"""bsg_engine_dedup, bsg_refset / bsg_refset_add and bsg_engine_pack_unique past one pass of their
grids and at the end of their tables, against the dict model of dedup_cases.py (and, for the pool's
index, the model of restore_cases.py), every result for equality.

A launch is capped at T = 8 x CUs x 256 threads (engine_grid), read from the source and the device;
N0 = max(T, 256 x kSumTile) is the count from which k_sum_mid also sums two parts per thread. Here
a run has more than N0 new records (the second trip of k_dd_insert, k_dd_first and k_dd_compact,
k_sum_mid under DvNew and DvNewBytes, seg_find over more than T segments in k_pack), a set takes
more than T keys in one call and is asked for more than T (k_set_add, ref_lookup in k_dd_first), a
table of more than T keys doubles (k_set_rehash), and T + 9 items share one ref. The last tests
put a cluster on the last slot of every table, so that the probe `(h + p) & mask` of k_dd_insert,
k_dd_first, set_insert, ref_lookup and pool_lookup has to go on from slot 0. Every input is valid,
or is answered with a return code."""
import numpy as np
import pytest

import dedup_cases as DC
import restore_cases as RC
from test_gpu_dedup import _records, _run
from test_gpu_tier_counts import cus  # noqa: F401  (the device's CU count, a fixture)

pytestmark = pytest.mark.gpu

BIT63 = np.uint64(63)


@pytest.fixture(scope="module")
def wide(oracle, table, cus):  # noqa: F811
    """dedup_cases.wide_run for this device, the oracle's records of it and the model's results,
    computed once and left unchanged."""
    t, n0 = DC.wide_counts(cus)
    case, recs = DC.wide_run(oracle, table, cus)
    want = DC.expected(recs)
    assert len(recs) > n0 + 100 and len(want[1]) > t + 100
    return {"case": case, "recs": recs, "want": want, "seen": frozenset(DC.ref_list(recs)),
            "packed": DC.packed_gather(case[0], recs, want[1])}


def _equal(name, got, want):
    assert len(got) == len(want), (name, len(got), len(want))
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    assert not len(bad), (name, len(bad), int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))


def _check(eng, res, want):
    for name, g, w in zip(("first", "uniq", "pack_off"), res, want):
        _equal(name, g, w)
    assert eng.nunique == len(want[1]) and eng.unique_bytes == int(want[2][-1])


def _pack(gpu, eng, want: bytes, funnel=0, guard=256):
    """pack_unique into the middle of a buffer poisoned 0xA5: the bytes and the guards."""
    n = eng.unique_bytes
    assert n == len(want)
    size = guard + ((n + 15) & ~15) + guard
    out = gpu.DeviceBuffer(size)
    try:
        assert gpu.lib().bsg_engine_pack_mode_debug(eng.h, funnel) == 0
        out.from_host(np.full(size, 0xA5, dtype=np.uint8))
        eng.pack_unique(out, offset=guard, cap=n)
        got = out.to_host()
    finally:
        out.free()
        gpu.lib().bsg_engine_pack_mode_debug(eng.h, 0)
    _equal("packed", got[guard:guard + n], np.frombuffer(want, dtype=np.uint8))
    assert (got[:guard] == 0xA5).all() and (got[guard + n:] == 0xA5).all()


def _start(gpu, oracle, table, eng, case):
    """The case run on `eng`; (the input's device buffer, the oracle's records, held to)."""
    streams, bits, mn = case
    host, off, lens = DC.place(streams)
    buf = _run(gpu, eng, host, off, lens, bits, mn)
    try:
        return buf, _records(gpu, oracle, table, eng, streams, bits, mn)
    except BaseException:
        buf.free()
        raise


def _added(n, new):
    want = np.zeros(n, dtype=np.uint8)
    want[new] = 1
    return want


# ---- 1. a run with more than N0 new records ----------------------------------------------------
def test_wide_run(gpu, oracle, table, wide):
    """first, uniq, pack_off and the totals of more than N0 records, more than T of them new, with
    duplicates early in the run and others more than T records after their first occurrence;
    the packed bytes through both of k_pack's load variants."""
    eng = gpu.Engine()
    try:
        buf, recs = _start(gpu, oracle, table, eng, wide["case"])
        try:
            assert recs.tobytes() == wide["recs"].tobytes()
            _check(eng, eng.dedup(), wide["want"])
            for funnel in (0, 1):
                _pack(gpu, eng, wide["packed"], funnel)
        finally:
            buf.free()
    finally:
        eng.close()


# ---- 2. the same run against a set -------------------------------------------------------------
def test_wide_run_and_a_set(gpu, oracle, table, wide, cus):  # noqa: F811
    """An empty set takes the run's new refs, more than T, in one call (k_set_add's second trip,
    several doublings from a new set's table); asked again, every record is in the set
    (ref_lookup for more than T records among more than T keys) and nothing is new; a small run
    with shared content sees exactly the wide run's refs as known."""
    t, _ = DC.wide_counts(cus)
    nu = len(wide["want"][1])
    assert nu > t and nu > DC.doubling_points(4)[3]     # more than three doublings in one call
    eng, rs = gpu.Engine(), gpu.RefSet()
    try:
        buf, recs = _start(gpu, oracle, table, eng, wide["case"])
        try:
            _check(eng, eng.dedup(rs), wide["want"])        # an empty set: as without one
            assert rs.count() == nu
            first, uniq, pack_off = eng.dedup(rs)
            assert eng.nunique == 0 and eng.unique_bytes == 0
            assert len(uniq) == 0 and pack_off.tolist() == [0]
            _equal("first", first, wide["want"][0] | np.uint64(DC.IN_SET))
            assert rs.count() == nu
        finally:
            buf.free()
        small = DC.wide_small(wide["case"][0][DC.WIDE_EXCERPTS])
        buf, rb = _start(gpu, oracle, table, eng, small)
        try:
            want = DC.expected(rb, wide["seen"])
            known = int((want[0] >> BIT63).sum())
            assert 1000 < known < len(rb) - 1000 and len(want[1]) > 1000
            _check(eng, eng.dedup(rs), want)
            _pack(gpu, eng, DC.packed(small[0], rb, want[1]))
            assert rs.count() == nu + len(want[1])
        finally:
            buf.free()
    finally:
        eng.close()
        rs.free()


# ---- 3. bsg_refset_add past T, and a rehash of more than T keys --------------------------------
def test_refset_add_past_a_grid_pass(gpu, cus):  # noqa: F811
    """T + 101 refs into an empty set; then, in one call, the refs that bring the count to the
    doubling point P exactly, among repeats of known refs and repeats inside the call more than T
    entries back; then one ref more, which rehashes P > T keys (k_set_rehash's second trip). No
    key is lost: a sample over all of them and then every one of them is known."""
    t, _ = DC.wide_counts(cus)
    a, b, c, p = DC.past_grid_refs(cus)
    assert len(a) == t + 101 and p >= len(a) and p in DC.doubling_points(50)
    first, new = DC.first_index([r.tobytes() for r in b], frozenset(r.tobytes() for r in a))
    assert len(a) + len(new) == p
    rs = gpu.RefSet()
    try:
        assert rs.add(a).all() and rs.count() == len(a)
        _equal("added", rs.add(b), _added(len(b), new))
        assert rs.count() == p
        assert rs.add(c).tolist() == [1] and rs.count() == p + 1
        keys = np.concatenate([a, b[new], c])
        assert len(keys) == p + 1
        sample = keys[np.linspace(0, p, 997).astype(np.int64)]   # ends included
        assert not rs.add(sample).any() and rs.count() == p + 1
        assert not rs.add(keys).any() and rs.count() == p + 1
    finally:
        rs.free()


# ---- 4. one ref T + 9 times --------------------------------------------------------------------
def test_one_ref_more_often_than_a_grid_pass(gpu, cus):  # noqa: F811
    """Every thread's atomicMin lands on one slot, some on their second trip."""
    t, _ = DC.wide_counts(cus)
    refs = DC.same_ref(t + 9)
    rs = gpu.RefSet()
    try:
        _equal("added", rs.add(refs), _added(t + 9, [0]))
        assert rs.count() == 1
        assert not rs.add(refs).any() and rs.count() == 1
    finally:
        rs.free()


def test_two_refs_in_more_records_than_a_grid_pass(gpu, oracle, table, cus):  # noqa: F811
    """T + 9 chunks of 64 bytes with two distinct refs in turn: first is 0 or 1 everywhere, and
    pack_unique writes those two chunks' 128 bytes and nothing else."""
    t, _ = DC.wide_counts(cus)
    case = DC.two_ref_stream(table, t + 9)
    eng = gpu.Engine()
    try:
        buf, recs = _start(gpu, oracle, table, eng, case)
        try:
            assert len(recs) == t + 9
            want = DC.expected(recs)
            _check(eng, eng.dedup(), want)
            assert eng.nunique == 2 and eng.unique_bytes == 128
            _pack(gpu, eng, DC.packed(case[0], recs, want[1]))
        finally:
            buf.free()
    finally:
        eng.close()


# ---- 5. clusters that step off the table's last slot -------------------------------------------
def test_wrap_through_refset_add(gpu):
    """The pass's own table (k_dd_insert, k_dd_first) and the set's (set_insert, ref_lookup), at a
    new set's size and after each of two doublings (k_set_rehash): the cluster lies at the end of
    every one of them."""
    refs = DC.wrap_refs()
    _, new = DC.first_index([r.tobytes() for r in refs])
    assert len(new) == 96
    rs = gpu.RefSet()
    try:
        _equal("added", rs.add(refs), _added(len(refs), new))
        assert rs.count() == 96
        assert not rs.add(refs[::-1]).any() and rs.count() == 96
        near = DC.wrap_base()
        near[:, 20] ^= 1
        assert rs.add(near).all() and rs.count() == 192
        assert not rs.add(refs).any() and not rs.add(near[::-1]).any()
        have = 192
        points = [x for x in DC.doubling_points(50) if x >= have][:2]
        fill = DC.random_refs(62, points[1] + 1)
        for point in points:
            assert rs.add(fill[have:point + 1]).all()     # one key past the point: a doubling
            have = point + 1
            assert rs.count() == have
            assert not rs.add(refs).any() and not rs.add(near).any() and rs.count() == have
        assert not rs.add(fill[192:have]).any()
        assert rs.add(DC.wrap_absent()[None, :]).tolist() == [1]
    finally:
        rs.free()


def test_wrap_through_engine_dedup(gpu, oracle, table):
    """A run's records looked up (k_dd_first's ref_lookup) in a set that holds the wrap refs, the
    refs that take the 8 slots before the table's last, and those of the run's own refs whose
    home is one of these 9 slots: their keys lie past the table's end, from slot 95 on, and a
    lookup that did not go on from slot 0 would call them new. Bit 63 of every record is the
    model's; then, in the grown set, every record is known."""
    case = DC.wrap_run()
    slots = DC.constants()["kRefSetSlots0"]
    eng, rs = gpu.Engine(), gpu.RefSet()
    try:
        buf, recs = _start(gpu, oracle, table, eng, case)
        try:
            at = DC.near_end(recs, slots)
            chosen = sorted({recs["ref"][i].tobytes() for i in at})
            held = [r.tobytes() for r in np.concatenate([DC.wrap_base(), DC.end_fillers()])]
            assert len(chosen) >= 10 and len(held) + len(chosen) <= DC.doubling_points(1)[0]
            assert rs.add(DC.wrap_refs()).sum() == 96 and rs.add(DC.end_fillers()).all()
            assert rs.add(chosen).all()                  # (the table is still a new set's)
            seen = frozenset(held) | frozenset(chosen)
            assert rs.count() == len(seen)
            want = DC.expected(recs, seen)
            res = eng.dedup(rs)
            _check(eng, res, want)
            inset = (res[0] >> BIT63) == 1
            assert inset.tolist() == [r in seen for r in DC.ref_list(recs)]
            assert inset[at].all() and int(inset.sum()) == len(at)
            assert rs.count() == len(seen | frozenset(DC.ref_list(recs)))
            first, uniq, _ = eng.dedup(rs)
            assert len(uniq) == 0 and ((first >> BIT63) == 1).all()
            assert not rs.add(DC.wrap_refs()).any() and not rs.add(DC.end_fillers()).any()
        finally:
            buf.free()
    finally:
        eng.close()
        rs.free()


def test_wrap_through_the_pool_index(gpu):
    """bsg_engine_restore from blobs labelled with the wrap refs: every one is found (pool_lookup
    over k_dd_insert's table), every output byte and guard is the model's; a ref with the same
    head that no blob carries is BSG_ENOTFOUND at its record and leaves the output untouched."""
    eng = gpu.Engine()
    try:
        c = RC.wrap_pool()
        rc, info, out = RC.run(gpu, eng, c, expect=RC.OK)
        RC.check_streams(c, out)
        assert info["bytes"] == sum(c["out_len"]) and info["bad_record"] == RC.NONE
        bad, k = RC.wrap_pool_absent()
        rc, info, out = RC.run(gpu, eng, bad, expect=RC.ENOTFOUND)
        assert info["bad_record"] == k and info["bytes"] == 0 and (out == RC.FILL).all()
    finally:
        eng.close()

"""Chunk dedup without a GPU: the dict model against a brute-force comparison, the new entry
points on null handles, and every input builder of dedup_cases.py held to what it claims (with the
oracle's records, which are what the GPU tests derive their expectations from)."""
import ctypes

import numpy as np
import pytest

import dedup_cases as DC
import layouts as L


@pytest.mark.parametrize("seed", range(6))
def test_model_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 120))
    pool = [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(max(1, n // 3))]
    refs = [pool[int(k)] for k in rng.integers(0, len(pool), n)]
    seen = frozenset(pool[:: 4]) if seed % 2 else frozenset()
    assert DC.first_index(refs, seen) == DC.brute_first(refs, seen)
    first, new = DC.first_index(refs, seen)
    assert len(set(refs) - seen) == len(new)            # every distinct unseen ref new once
    assert all(first[i] == i for i in new)
    assert all((f & DC.IN_SET != 0) == (r in seen) for f, r in zip(first, refs))


def test_null_handles():
    from bs_amd import bsgpu
    Lb = bsgpu.lib()
    nu, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert Lb.bsg_engine_dedup(None, None, ctypes.byref(nu), ctypes.byref(nb)) == -22
    assert Lb.bsg_engine_pack_unique(None, None, 0) == -22
    assert Lb.bsg_engine_copy_dedup(None, None, 0, None, None, 0) == -22
    assert Lb.bsg_engine_dedup_first_device(None) is None
    assert Lb.bsg_engine_dedup_uniq_device(None) is None
    assert Lb.bsg_engine_dedup_pack_off_device(None) is None
    assert Lb.bsg_refset_count(None) == 0
    refs = np.zeros(32, dtype=np.uint8)
    assert Lb.bsg_refset_add(None, refs.ctypes.data, 1, None) == -22
    Lb.bsg_refset_free(None)
    err = ctypes.c_int(0)
    h = Lb.bsg_refset_new(Lb.bsg_device_count() + 3, ctypes.byref(err))
    assert not h and err.value == -19


def test_constants():
    c = DC.constants()
    assert c["kRefSetSlots0"] <= 4096 and c["kRefSetSlots0"] & (c["kRefSetSlots0"] - 1) == 0
    assert 0 < c["kRefSetLoadPct"] < 100
    assert c["kPackTile"] % 16 == 0
    p = DC.doubling_points()
    assert p[1] == 2 * p[0] > 0


def test_edited_copies(oracle, table):
    streams, bits, mn = DC.edited_copies()
    assert [len(s) for s in streams][0] == DC.MIB and abs(len(streams[1]) - DC.MIB) < 16 * 256
    recs = DC.oracle_records(oracle, table, streams, bits, mn)
    first, uniq, _ = DC.expected(recs)
    nb = int((recs["stream"] == 1).sum())
    na = len(recs) - nb
    assert na > 2000 and nb > 2000
    dup_of_a = sum(1 for i in range(na, len(recs)) if int(first[i]) < na)
    assert dup_of_a * 2 > nb, (dup_of_a, nb)
    assert 0 < len(uniq) < len(recs)


def test_residue_coverage(oracle, table):
    streams, bits, mn = DC.residues()
    recs = DC.oracle_records(oracle, table, streams, bits, mn)
    _, uniq, pack_off = DC.expected(recs)
    # streams start at multiples of 16 of a 16-byte aligned base: the source residue is offset's
    pairs = {(int(recs["offset"][int(i)]) % 16, int(pack_off[k]) % 16) for k, i in enumerate(uniq)}
    assert len(pairs) == 256


def test_tiny_chunks(oracle, table):
    streams, bits, mn = DC.tiny_chunks()
    recs = DC.oracle_records(oracle, table, streams, bits, mn)
    first, uniq, _ = DC.expected(recs)
    assert (recs["len"] == 1).sum() > 100
    dups = len(recs) - len(uniq)
    assert dups * 3 >= len(recs)
    # new records after duplicates: packing skips segments in the middle of the run
    assert any(int(uniq[k + 1]) - int(uniq[k]) > 1 for k in range(len(uniq) - 1))
    # some 16-byte vector of the output holds bytes of at least four segments
    new_lens = recs["len"][uniq.astype(np.int64)]
    assert any(int(new_lens[k:k + 4].sum()) <= 16 for k in range(len(uniq) - 4))


def test_zeros_and_one_chunk_streams(oracle, table):
    streams, bits, mn = DC.zeros()
    recs = DC.oracle_records(oracle, table, streams, bits, mn)
    assert len(recs) > 100 and len(DC.expected(recs)[1]) <= 2
    streams, bits, mn = DC.one_chunk_streams()
    assert len(streams) == 3000
    recs = DC.oracle_records(oracle, table, streams, bits, mn)
    assert len(recs) == 3000                       # one chunk each
    first, uniq, _ = DC.expected(recs)
    assert all(int(first[s]) == s - 2 for s in range(2, 3000, 3))
    assert len(uniq) == 2000


def test_long_segments(oracle, table):
    tile = DC.constants()["kPackTile"]
    streams, bits, mn = DC.long_segment()
    recs = DC.oracle_records(oracle, table, streams, bits, mn)
    assert len(recs) == 1 and int(recs["len"][0]) > 64 * tile
    streams, bits, mn = DC.long_among_short()
    assert len(streams) == 4001
    lens = [len(s) for s in streams]
    assert max(lens) == lens[2000] > tile and all(64 <= n <= 200 for n in lens[:2000] + lens[2001:])
    recs = DC.oracle_records(oracle, table, streams, bits, mn)
    assert len(recs) == 4001 and len(DC.expected(recs)[1]) == 4001


def test_shared_halves(oracle, table):
    groups, bits, mn = DC.shared_halves()
    ra, rb = (DC.oracle_records(oracle, table, g, bits, mn) for g in groups)
    sa, sb = set(DC.ref_list(ra)), set(DC.ref_list(rb))
    assert len(sa & sb) * 3 >= len(sa) and len(sa - sb) * 3 >= len(sa) and len(sb - sa) > 0


def test_planted_refs():
    r = DC.planted_refs()
    a, b, c = r[:64], r[64:128], r[128:128 + 4096]
    assert len({x[:31].tobytes() for x in a}) == 1 and len({int(x[31]) for x in a}) == 64
    assert len({x[:8].tobytes() for x in b}) == 1 and len({x[9:].tobytes() for x in b}) == 1
    assert len({int(x[8]) for x in b}) == 64
    assert len({x[:2].tobytes() for x in c}) == 1 and len({x.tobytes() for x in c}) == 4096
    assert not r[128 + 4096].any() and (r[128 + 4097] == 0xFF).all()
    refs = [x.tobytes() for x in r]
    first, new = DC.first_index(refs)
    assert len(new) == 64 + 64 + 4096 + 2 and len(refs) == len(new) + 200
    assert all(first[i] < i for i in range(len(new), len(refs)))   # exact repeats in one call


def test_layout_duplicates(oracle, table):
    """The aliased layout of tests/layouts.py: the second stream on the same bytes repeats the
    first chunk for chunk, the prefix stream shares its leading chunks."""
    layout = L.build("aliased")
    buf = L.fill(layout, 0)
    streams = [buf[o:o + n] for o, n, _ in layout[1]]
    recs = DC.oracle_records(oracle, table, streams, 6, 64)
    first, _, _ = DC.expected(recs)
    s0, s1 = L.ALIAS_SAME
    i0 = int(np.flatnonzero(recs["stream"] == s0)[0])
    idx1 = np.flatnonzero(recs["stream"] == s1)
    assert len(idx1) > 100
    assert [int(first[i]) for i in idx1] == list(range(i0, i0 + len(idx1)))
    p0, p1 = L.ALIAS_PREFIX
    idxp = np.flatnonzero(recs["stream"] == p1)
    assert len(idxp) > 3 and all(int(first[i]) < int(idxp[0]) for i in idxp[:-1])


# ---- the builders of tests/test_gpu_dedup_wide.py, at the 256 CUs of an MI355X -----------------
CUS = 256


def test_wide_counts():
    import walk_cases as W
    t, n0 = DC.wide_counts(CUS)
    assert t == W.grid_threads(CUS) and n0 >= t and n0 >= 256 * W.grid_caps()["kSumTile"]
    assert n0 in (t, 256 * W.grid_caps()["kSumTile"])
    # from N0 + 1 items on the prefix sums have more than 256 parts: two for some thread
    assert -(-(n0 + 1) // W.grid_caps()["kSumTile"]) > 256


def test_wide_run(oracle, table):
    t, n0 = DC.wide_counts(CUS)
    (streams, bits, mn), recs = DC.wide_run(oracle, table, CUS)
    assert (bits, mn) == (1, 8) and len(streams) == DC.WIDE_EXCERPTS + 2
    main = DC.WIDE_EXCERPTS
    assert all(len(s) == 2000 for s in streams[:main]) and len(streams[main + 1]) >= 64 << 10
    assert abs(len(streams[main]) - 10.5 * n0) <= 1      # no growth was needed at this size
    assert recs.tobytes() == DC.oracle_records(oracle, table, streams, bits, mn).tobytes()
    first, uniq, pack_off = DC.expected(recs)
    f = first.astype(np.int64)
    i = np.arange(len(recs))
    assert len(recs) > n0 + 100
    assert len(uniq) > t + 100
    assert int((f < i - t).sum()) >= 1000
    in_main = recs["stream"] == main
    assert int(((f < i) & in_main).sum()) >= 1000
    assert len(set(recs["len"].tolist())) >= 16
    # the duplicates inside the main stream are scattered: some in each of its eight parts
    at = np.flatnonzero((f < i) & in_main)
    lo, n = int(np.flatnonzero(in_main)[0]), int(in_main.sum())
    assert len(set(((at - lo) * 8 // n).tolist())) == 8
    # the last stream's far duplicates are copies of records of the main stream's first quarter
    far = np.flatnonzero((f < i - t) & (recs["stream"] == main + 1))
    assert len(far) >= 1000 and (f[far] < lo + n // 4).all()
    assert DC.wide_facts(recs, first, uniq, t, main) == {
        "nrec": len(recs), "nunique": len(uniq), "far": int((f < i - t).sum()),
        "dups_in_main": len(at), "nlens": len(set(recs["len"].tolist()))}
    # the gathered pack of this run: its length, and every new record's bytes at its offset
    got = DC.packed_gather(streams, recs, uniq)
    assert len(got) == int(pack_off[-1])
    for k in np.linspace(0, len(uniq) - 1, 500).astype(np.int64):
        assert got[int(pack_off[k]):int(pack_off[k + 1])] == DC.packed(streams, recs, uniq[k:k + 1])
    # the small run shares records with this one and has records of its own
    small, sb, sm = DC.wide_small(streams[main])
    assert (sb, sm) == (bits, mn)
    rs = DC.oracle_records(oracle, table, small, sb, sm)
    seen = set(DC.ref_list(recs))
    shared = sum(r in seen for r in DC.ref_list(rs))
    assert shared > 1000 and len(rs) - shared > 1000


@pytest.mark.parametrize("name", ["residues", "tiny_chunks", "zeros", "long_among_short"])
def test_packed_gather(oracle, table, name):
    """The vectorised twin of packed(), on small cases of every kind of segment."""
    streams, bits, mn = getattr(DC, name)()
    recs = DC.oracle_records(oracle, table, streams, bits, mn)
    _, uniq, _ = DC.expected(recs)
    assert DC.packed_gather(streams, recs, uniq) == DC.packed(streams, recs, uniq)
    assert DC.packed_gather(streams, recs, uniq[:0]) == b""


def test_past_grid_refs():
    t, _ = DC.wide_counts(CUS)
    a, b, c, p = DC.past_grid_refs(CUS)
    assert len(a) == t + 101 and p == 1 << 20 and len(c) == 1
    pts = DC.doubling_points(50)
    assert p in pts and pts[pts.index(p) - 1] < len(a) <= p
    sa = {r.tobytes() for r in a}
    assert len(sa) == len(a) and c[0].tobytes() not in sa
    refs = [r.tobytes() for r in b]
    first, new = DC.first_index(refs, frozenset(sa))
    assert len(a) + len(new) == p and c[0].tobytes() not in set(refs)
    assert len(b) > t + 2 * 4096
    f = np.array([x & ~DC.IN_SET for x in first], dtype=np.int64)
    inset = np.array([x & DC.IN_SET != 0 for x in first])
    i = np.arange(len(b))
    assert int((~inset & (f < i - t)).sum()) == 4096       # repeats inside the call, far back
    assert int(inset.sum()) >= len(new) // 4               # repeats of the first call's refs
    # interleaved: fresh refs, old ones and repeats all occur after entry T
    tail = slice(t, len(b))
    assert (f[tail] == i[tail])[~inset[tail]].any() and inset[tail].any()
    assert inset[4096:t].any() and (~inset[4096:t]).any()


def test_same_ref_and_two_ref_stream(oracle, table):
    t, _ = DC.wide_counts(CUS)
    r = DC.same_ref(t + 9)
    assert r.shape == (t + 9, 32) and (r == r[0]).all()
    streams, bits, mn = DC.two_ref_stream(table, t + 9)
    assert (bits, mn) == (8, 64) and len(streams[0]) == 64 * (t + 9)
    recs = DC.oracle_records(oracle, table, streams, bits, mn)
    assert len(recs) == t + 9 and (recs["len"] == 64).all()
    first, uniq, pack_off = DC.expected(recs)
    assert uniq.tolist() == [0, 1] and pack_off.tolist() == [0, 64, 128]
    assert set(first.tolist()) == {0, 1}


def test_wrap_refs():
    base, refs = DC.wrap_base(), DC.wrap_refs()
    assert len(base) == 96 and len({r.tobytes() for r in base}) == 96
    ff, lo = base[:DC.WRAP_HEAD], base[DC.WRAP_HEAD:]
    assert (ff[:, :8] == 0xFF).all()
    assert len({r[:31].tobytes() for r in ff[:16]}) == 1 and len({int(r[31]) for r in ff[:16]}) == 16
    assert [int.from_bytes(r[:8].tobytes(), "little") for r in lo] == list(range(48))
    keys = [r.tobytes() for r in refs]
    assert len(keys) == 126 and set(keys) == {r.tobytes() for r in base}
    first, new = DC.first_index(keys)
    again = [keys[i] for i in range(len(keys)) if first[i] < i]
    assert len(again) == 30 and len(set(again)) == 30
    assert sum(k[:8] == b"\xff" * 8 for k in again) == 15
    absent = DC.wrap_absent()
    assert (absent[:8] == 0xFF).all() and absent.tobytes() not in set(keys)
    # the sizes these refs meet: a pass's own table, a new set's and its doublings, a pool's index
    c = DC.constants()
    for slots in (256, c["kRefSetSlots0"], 2 * c["kRefSetSlots0"], 4 * c["kRefSetSlots0"]):
        assert all(DC.home(r, slots) == slots - 1 for r in ff)
        assert [DC.home(r, slots) for r in lo] == list(range(48))
        where = DC.probe_slots(refs, slots)
        assert len(where) == 96 and len(set(where.values())) == 96
        below = [k for k, s in where.items() if s < DC.home(np.frombuffer(k, np.uint8), slots)]
        assert len(below) >= 40 and all(k[:8] == b"\xff" * 8 for k in below)
        # the wrapped sequence passes the homes of the low refs: both kinds share slots 0 .. 94
        assert sorted(where.values()) == list(range(95)) + [slots - 1]


def test_wrap_run(oracle, table):
    """Enough of the run's own refs have their home in a new set's last 9 slots, which wrap_base
    and end_fillers take: inserted after those, every one of them ends below its home, past the
    wrapped cluster."""
    slots = DC.constants()["kRefSetSlots0"]
    fill = DC.end_fillers()
    for s in (slots, 4 * slots):
        assert [DC.home(r, s) for r in fill] == [s - 2 - j for j in range(DC.WRAP_FILL)]
    streams, bits, mn = DC.wrap_run()
    recs = DC.oracle_records(oracle, table, streams, bits, mn)
    at = DC.near_end(recs, slots)
    assert at.tolist() == [i for i, r in enumerate(recs["ref"])
                           if DC.home(r, slots) >= slots - DC.WRAP_FILL - 1]
    chosen = sorted({recs["ref"][i].tobytes() for i in at})
    assert len(chosen) >= 10
    held = list(DC.wrap_base()) + list(fill)
    assert len(held) + len(chosen) <= DC.doubling_points(1)[0]      # the table does not double
    where = DC.probe_slots(held + [np.frombuffer(k, np.uint8) for k in chosen], slots)
    assert sorted(where[k] for k in chosen) == list(range(95, 95 + len(chosen)))


def test_wrap_pool():
    import restore_cases as RC
    c = RC.wrap_pool()
    blobs, recs = c["blobs"], c["recs"]
    assert {b["ref"].tobytes() for b in blobs} == {r.tobytes() for r in DC.wrap_base()}
    assert sorted(blobs["len"].tolist()) == list(range(1, 97)) and not c["verify"]
    assert sorted(r.tobytes() for r in recs["ref"]) == sorted(b.tobytes() for b in blobs["ref"])
    assert set(recs["stream"].tolist()) == {0, 1}
    label = [b.tobytes() for b in blobs["ref"]]
    named = [label.index(r.tobytes()) for r in recs["ref"]]
    assert named != sorted(named)
    out0 = np.full(c["cap"], RC.FILL, dtype=np.uint8)
    rc, info, out = RC.expected(c["pool"], blobs, recs, c["out_off"], c["out_len"], out0, False)
    assert rc == RC.OK and info["bytes"] == sum(range(1, 97))
    RC.check_streams(c, out)
    bad, k = RC.wrap_pool_absent()
    assert (bad["recs"][k]["ref"][:8] == 0xFF).all()
    assert bad["recs"][k]["ref"].tobytes() not in set(label)
    rc, info, out = RC.expected(bad["pool"], blobs, bad["recs"], bad["out_off"], bad["out_len"],
                                out0, False)
    assert rc == RC.ENOTFOUND and info["bad_record"] == k and (out == RC.FILL).all()

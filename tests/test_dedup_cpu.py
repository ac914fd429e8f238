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

"""merge_cases held to what it claims, on runs built from the oracle and tree_form.listing: the
merged destination against a copy of it into which the new blobs are put one by one, a merge into
an empty pool against collect_cases.collect, overlap none, partial and total, ALL against every
Root, a repeated merge, sync against its two merges and its all-or-nothing capacity rule. No GPU
needed."""
import numpy as np
import pytest

import collect_cases as C
import gc_cases as G
import merge_cases as M
import pool_cases as P
from bs_amd.synth import edit_stream, splitmix_array

PARAMS = [(4, 64, 2), (6, 64, 3)]
CAP = (1 << 22, 1 << 14)


class Case:
    pass


@pytest.fixture(scope="module", params=PARAMS, ids=lambda p: "b%d_m%d_f%d" % p)
def case(request, oracle, table):
    """Three runs that share streams: run 2 is an edit of run 1's first stream, run 1's last
    stream again and a new one; run 3 shares nothing. Pools: one (run 1), two (run 2), both (1
    then 2), other (run 3)."""
    bits, mn, fanout = request.param
    a, b = splitmix_array(1, 9107), splitmix_array(2, 30000)
    s1 = [a, a[:5000].copy(), np.zeros(0, np.uint8), splitmix_array(3, 40), b]
    s2 = [edit_stream(a, 5, sites=3, span=256), b, splitmix_array(9, 7001)]
    s3 = [splitmix_array(21, 12345)]
    c = Case()
    c.runs = [P.oracle_run(oracle, table, s, bits, mn, fanout) for s in (s1, s2, s3)]
    c.roots = [P.roots_of(r) for r in c.runs]

    def pool(*which):
        m = P.Model(*CAP)
        for w in which:
            assert m.put(c.runs[w])[0] == P.OK
        return m

    c.one, c.two, c.both, c.other = pool(0), pool(1), pool(0, 1), pool(2)
    return c


def _same(a: P.Model, b: P.Model):
    assert a.table == b.table and a.bytes == b.bytes and a.index == b.index
    assert a.buf.tobytes() == b.buf.tobytes()


def _frozen(m: P.Model):
    return list(m.table), m.bytes, m.buf.tobytes(), dict(m.index)


def _merge(src, dst, roots=None, flags=0):
    """One merge held to the brute form and to the remap rule; neither argument is written."""
    before = _frozen(src), _frozen(dst)
    rc, status, info, out, remap = M.merge(src, dst, roots, flags)
    assert rc == M.OK
    assert (_frozen(src), _frozen(dst)) == before
    if flags & M.ALL:
        live = np.ones(len(src.table), dtype=np.uint8)
        assert info["gc"] == M.GC_ZERO and status is None
    else:
        live = G.mark(src.blob_bytes, src.blobs(), roots, src.stat()["pool_bytes"])[3]
    new = M.new_of(src, dst, live)
    _same(out, M.brute(src, dst, new))
    assert out.table[:len(dst.table)] == dst.table
    assert info["selected"] == int(live.sum()) == info["known"] + info["added"]
    assert info["added"] == int(new.sum()) == len(out.table) - len(dst.table)
    assert info["first_blob"] == len(dst.table) and info["need_blobs"] == len(out.table)
    assert info["need_bytes"] == out.bytes
    assert info["added_bytes"] == sum(src.table[k][1] for k in np.flatnonzero(new))
    for k in range(len(src.table)):
        if not live[k]:
            assert remap[k] == M.NONE
        else:
            j = int(remap[k])
            assert out.table[j][2] == src.table[k][2]
            assert (j >= len(dst.table)) == bool(new[k])
    at = remap[np.flatnonzero(new)].tolist()
    assert at == list(range(len(dst.table), len(out.table)))      # src's index order
    assert len(C.taken_slots(out)) == len(out.table)
    return info, out, remap


def test_into_an_empty_pool_is_a_collect(case):
    for roots in (case.roots[0], case.roots[1], case.roots[0] + case.roots[1], []):
        info, out, remap = _merge(case.both, P.Model(*CAP), roots)
        rc, status, ci, cd, cremap = C.collect(case.both, roots, *CAP)
        assert rc == C.OK
        _same(out, cd)
        assert remap.tolist() == cremap.tolist() and info["gc"] == ci["gc"]
        assert (info["need_bytes"], info["need_blobs"]) == (ci["need_bytes"], ci["need_blobs"])


def test_overlap_none_partial_and_total(case):
    # none: run 3 shares nothing with run 1
    info, out, _ = _merge(case.other, case.one, case.roots[2])
    assert info["known"] == 0 and info["added"] == len(case.other.table)
    # partial: run 2's streams share chunks and nodes with run 1
    info, out, _ = _merge(case.two, case.one, case.roots[1])
    assert info["known"] > 0 and info["added"] > 0
    assert set(out.index) == set(case.both.index)
    assert case.one.bytes % 16 != 0 or case.two.bytes % 16 != 0
    # total: everything selected is known, and nothing changes
    info, out, remap = _merge(case.one, case.both, case.roots[0])
    assert info["added"] == 0 and info["known"] == info["selected"] == len(case.one.table)
    _same(out, case.both)
    assert info["need_bytes"] == case.both.bytes
    assert remap.tolist() == list(range(len(case.one.table)))


def test_all_is_every_root_of_a_pool_without_dead_blobs(case):
    a = _merge(case.both, case.other, None, M.ALL)
    b = _merge(case.both, case.other, case.roots[0] + case.roots[1])
    _same(a[1], b[1])
    assert a[2].tolist() == b[2].tolist()
    assert {k: v for k, v in a[0].items() if k != "gc"} == \
           {k: v for k, v in b[0].items() if k != "gc"}
    assert b[0]["gc"]["ndead"] == 0


def test_a_second_merge_adds_nothing(case):
    _, out, remap = _merge(case.two, case.one, case.roots[1])
    info, again, remap2 = _merge(case.two, out, case.roots[1])
    assert info["added"] == 0 and info["added_bytes"] == 0 and info["need_bytes"] == out.bytes
    _same(again, out)
    assert remap2.tolist() == remap.tolist()


def test_a_known_ref_with_another_len_stays(case):
    src = M.clone(case.other)
    o, n, r = case.one.table[3]
    assert src.put(C.one_blob_run(b"not the blob", r), P.CHUNKS)[1]["added"] == 1
    info, out, remap = _merge(src, case.one, None, M.ALL)
    assert out.table[3] == (o, n, r) and int(remap[-1]) == 3
    assert info["known"] == 1 and info["added"] == len(case.other.table)


def test_verify_sees_the_blobs_to_append_only(case):
    assert M.merge(case.two, case.one, case.roots[1], M.VERIFY)[2]["verified"] > 0
    live = G.mark(case.two.blob_bytes, case.two.blobs(), case.roots[1],
                  case.two.stat()["pool_bytes"])[3]
    new = M.new_of(case.two, case.one, live)
    k_new = int(np.flatnonzero(new & (case.two.blobs()["len"] > 0))[1])
    k_known = int(np.flatnonzero(~new)[0])
    for k, rc in ((k_new, M.ECORRUPT), (k_known, M.OK)):
        src = M.clone(case.two)
        src.buf[src.table[k][0]] ^= 1
        got = M.merge(src, case.one, case.roots[1] if rc == M.OK else None,
                      M.VERIFY | (0 if rc == M.OK else M.ALL))
        assert got[0] == rc, (k, got[0])
        assert got[2]["bad_blob"] == (k if rc != M.OK else M.NONE)
        assert got[2]["verified"] == got[2]["added_bytes"] > 0
        assert (got[3] is None) == (rc != M.OK)


def test_failed_marks_and_capacity(case):
    gone = bytes(range(32))
    rc, status, info, out, remap = M.merge(case.two, case.one, [case.roots[1][0], gone])
    assert rc == M.ENOTFOUND and status.tolist() == [0, M.ENOTFOUND] and out is None
    assert info["gc"]["bad_root"] == 1 and info["added"] == 0
    need = M.merge(case.two, case.one, case.roots[1])[2]
    for cb, cn in ((need["need_bytes"] - 1, need["need_blobs"]),
                   (need["need_bytes"], need["need_blobs"] - 1)):
        dst = M.clone(case.one)
        dst.cap_bytes, dst.cap_blobs = cb, cn
        rc, _, info, out, remap = M.merge(case.two, dst, case.roots[1])
        assert rc == M.ENOMEM and info == need and out is None and remap is None
    dst = M.clone(case.one)
    dst.cap_bytes, dst.cap_blobs = need["need_bytes"], need["need_blobs"]
    assert M.merge(case.two, dst, case.roots[1])[0] == M.OK


def test_sync_is_the_two_merges(case):
    for a, b in ((case.one, case.two), (case.one, case.other), (case.one, P.Model(*CAP)),
                 (case.both, M.clone(case.both))):
        fa, fb = _frozen(a), _frozen(b)
        rc, info, a2, b2, remap_b, remap_a = M.sync(a, b)
        assert rc == M.OK and (_frozen(a), _frozen(b)) == (fa, fb)
        _, _, i0, b1, r0 = M.merge(a, b, None, M.ALL)
        _, _, i1, a1, r1 = M.merge(b1, a, None, M.ALL)
        _same(b2, b1)
        _same(a2, a1)
        assert set(a2.index) == set(b2.index) == set(a.index) | set(b.index)
        assert info[0] == i0 and remap_b.tolist() == r0.tolist()
        assert remap_a.tolist() == r1[:len(b.table)].tolist()       # b's blobs at the call
        for k in ("added", "added_bytes", "first_blob", "need_bytes", "need_blobs"):
            assert info[1][k] == i1[k], k
        assert info[1]["selected"] == len(b.table)


def test_sync_is_all_or_nothing(case):
    a, b = M.clone(case.one), M.clone(case.two)
    need = M.sync(a, b)[1]
    assert need[0]["added"] > 0 and need[1]["added"] > 0
    b.cap_bytes, b.cap_blobs = need[0]["need_bytes"], need[0]["need_blobs"]      # a -> b fits
    a.cap_bytes, a.cap_blobs = need[1]["need_bytes"], need[1]["need_blobs"] - 1  # b -> a does not
    fa, fb = _frozen(a), _frozen(b)
    rc, info, a2, b2, _, _ = M.sync(a, b)
    assert rc == M.ENOMEM and info == need and a2 is None and b2 is None
    assert (_frozen(a), _frozen(b)) == (fa, fb)
    assert M.merge(a, b, None, M.ALL)[0] == M.OK       # the first direction alone would fit
    a.cap_blobs += 1
    assert M.sync(a, b)[0] == M.OK

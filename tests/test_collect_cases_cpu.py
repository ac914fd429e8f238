"""collect_cases held to what it claims, on runs built from the oracle and tree_form.listing: its
numpy layout and gather against gc_cases, the collected pool against a fresh Model into which the
live blobs are put one by one, and two invariants (every Root: the source again; no Root: an
empty pool). No GPU needed."""
import numpy as np
import pytest

import collect_cases as C
import gc_cases as G
import pool_cases as P
from bs_amd.synth import edit_stream, splitmix_array

PARAMS = [(4, 64, 2), (6, 64, 3)]
CAP = (1 << 22, 1 << 14)


def _streams():
    a, b = splitmix_array(1, 9107), splitmix_array(2, 30000)
    return [a, a.copy(), a[:5000].copy(), np.zeros(0, np.uint8), splitmix_array(3, 40), b]


@pytest.fixture(scope="module", params=PARAMS, ids=lambda p: "b%d_m%d_f%d" % p)
def pool(request, oracle, table):
    """A pool of two runs, the second an edit of the first plus a new stream: (the model, the
    Roots of run 1, the Roots of run 2)."""
    bits, mn, fanout = request.param
    s1 = _streams()
    s2 = [edit_stream(s1[0], 5, sites=3, span=256), s1[5], splitmix_array(9, 7001)]
    r1 = P.oracle_run(oracle, table, s1, bits, mn, fanout)
    r2 = P.oracle_run(oracle, table, s2, bits, mn, fanout)
    m = P.Model(*CAP)
    assert m.put(r1)[0] == P.OK and m.put(r2)[0] == P.OK
    return m, P.roots_of(r1), P.roots_of(r2)


def _same(a: P.Model, b: P.Model):
    assert a.table == b.table and a.bytes == b.bytes and a.index == b.index
    assert a.buf.tobytes() == b.buf.tobytes()


@pytest.mark.parametrize("which", [1, 2])
def test_collect_is_the_live_blobs_put_one_by_one(pool, which):
    m, roots1, roots2 = pool
    roots = roots1 if which == 1 else roots2
    before = (list(m.table), m.buf.copy(), m.bytes)
    rc, status, info, dst, remap = C.collect(m, roots, *CAP)
    assert rc == C.OK and status.tolist() == [0] * len(roots)
    assert (m.table, m.bytes) == (before[0], before[2]) and (m.buf == before[1]).all()
    blobs = m.blobs()
    live = G.mark(m.blob_bytes, blobs, roots, m.stat()["pool_bytes"])[3]
    assert 0 < info["gc"]["ndead"] and info["gc"]["nlive"] == int(live.sum()) == len(dst.table)
    # the restated layout and gather are gc_cases' own
    wt, end = G.layout(blobs, live, True)
    t16, end16 = C.layout16(blobs, live)
    assert t16.tobytes() == wt.tobytes() and end16 == end
    swept = G.compacted(m.buf, blobs, live, True)
    assert C.gathered(m.buf, blobs, live).tobytes() == swept.tobytes()
    assert dst.blobs().tobytes() == wt.tobytes() and dst.bytes == end == info["need_bytes"]
    assert info["need_blobs"] == len(wt)
    _same(dst, C.brute(m, live, *CAP))
    # remap: live blobs count up in index order, every entry is its source's
    at = np.flatnonzero(live)
    assert remap[at].tolist() == list(range(len(at))) and (remap[live == 0] == C.NONE).all()
    for k in at:
        j = int(remap[k])
        assert dst.table[j][1:] == m.table[k][1:] and dst.blob_bytes(j) == m.blob_bytes(int(k))
    assert len(C.taken_slots(dst)) == len(dst.table)


def test_every_root_is_the_source_again(pool):
    m, roots1, roots2 = pool
    rc, _, info, dst, remap = C.collect(m, roots1 + roots2, *CAP)
    assert rc == C.OK and info["gc"]["ndead"] == 0
    _same(dst, m)
    assert remap.tolist() == list(range(len(m.table)))
    assert C.taken_slots(dst) == C.taken_slots(m)


def test_no_root_is_an_empty_pool(pool):
    m = pool[0]
    for roots in ([], [bytes(32)] * 3):
        rc, status, info, dst, remap = C.collect(m, roots, 0, 0)
        assert rc == C.OK and len(status) == len(roots)
        assert info["need_bytes"] == info["need_blobs"] == info["gc"]["nlive"] == 0
        assert info["gc"]["ndead"] == len(m.table)
        _same(dst, P.Model(0, 0))
        assert (remap == C.NONE).all() and len(remap) == len(m.table)


def test_verdicts_and_capacity(pool):
    m, roots1, _ = pool
    gone = bytes(range(32))
    rc, status, info, dst, remap = C.collect(m, [roots1[0], gone], *CAP)
    assert rc == C.ENOTFOUND and status.tolist() == [0, C.ENOTFOUND] and dst is None
    assert info["gc"]["bad_root"] == 1 and info["need_blobs"] == 0
    chunk = next(r for _, n, r in m.table if G.W.parse_node(m.blob_bytes(m.index[r])) is None)
    rc, status, info, dst, remap = C.collect(m, [chunk], *CAP)
    assert rc == C.ECORRUPT and status.tolist() == [C.ECORRUPT] and dst is None
    need = C.collect(m, roots1, *CAP)[2]
    for cb, cn in ((need["need_bytes"] - 1, need["need_blobs"]),
                   (need["need_bytes"], need["need_blobs"] - 1)):
        rc, _, info, dst, remap = C.collect(m, roots1, cb, cn)
        assert rc == C.ENOMEM and info == need and dst is None and remap is None
    assert C.collect(m, roots1, need["need_bytes"], need["need_blobs"])[0] == C.OK

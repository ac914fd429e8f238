"""pool_cases.Model held to what it claims, on runs built from the oracle (its split and
py_tree_root) and tree_form.listing: no GPU needed."""
import numpy as np
import pytest

import dedup_cases as DC
import pool_cases as P
from bs_amd.synth import edit_stream, splitmix_array

PARAMS = [(4, 64, 2), (6, 64, 3)]


def _streams():
    a, b = splitmix_array(1, 9107), splitmix_array(2, 30000)
    return [a, a.copy(), a[:5000].copy(), np.zeros(0, np.uint8), splitmix_array(3, 40), b]


@pytest.fixture(scope="module", params=PARAMS, ids=lambda p: "b%d_m%d_f%d" % p)
def run(request, oracle, table):
    bits, mn, fanout = request.param
    return P.oracle_run(oracle, table, _streams(), bits, mn, fanout), request.param


def test_oracle_run_is_the_writer_tree(run, oracle):
    """The listed nodes' last one per stream is py_tree_root's Root, every node's ref is the
    SHA-256 of its arena bytes, and the arena's blobs start at multiples of 16."""
    (recs, streams, nodes, arena), (bits, mn, fanout) = run
    import hashlib
    roots = P.roots_of((recs, streams, nodes, arena))
    for s, d in enumerate(streams):
        r = recs[recs["stream"] == s]
        pieces = [(bytes(d[int(c["offset"]):int(c["offset"]) + int(c["len"])]), int(c["level"]))
                  for c in r]
        assert roots[s] == oracle.py_tree_root(pieces, fanout=fanout), s
    assert roots[3] == bytes(32) and (recs["stream"] == 4).sum() == 1
    assert (nodes["blob_off"] % 16 == 0).all()
    for n in nodes:
        o, ln = int(n["blob_off"]), int(n["blob_len"])
        assert hashlib.sha256(arena[o:o + ln].tobytes()).digest() == n["ref"].tobytes()


def test_one_put(run):
    r, _ = run
    recs, streams, nodes, arena = r
    m = P.Model(1 << 22, 1 << 14)
    rc, info = m.put(r)
    assert rc == P.OK
    new = P.brute_put([], r)
    nrec = len(recs)
    # duplicates collapse: the copy of A and the prefix of A add (next to) nothing
    assert info["items"] == nrec + len(nodes) and info["added"] == len(new) == len(m.table)
    assert info["repeats"] == info["items"] - info["added"] > 0 and info["known"] == 0
    refs = [x for _, _, x in m.table]
    assert len(set(refs)) == len(refs)
    # a node equal to an earlier node is not added: none of the copy's nodes is
    a_nodes = {n["ref"].tobytes() for n in nodes[nodes["stream"] == 0]}
    copy_at = nrec + np.flatnonzero(nodes["stream"] == 1)
    assert len(copy_at) == len(a_nodes) > 0 and not set(copy_at.tolist()) & set(new)
    # order: chunks, then nodes, each in item order
    kinds = [i >= nrec for i in new]
    assert kinds == sorted(kinds) and new == sorted(new) and any(kinds) and not all(kinds)
    # offsets: multiples of 16, each blob right after the one before, padding zero
    o = 0
    cover = np.zeros(len(m.buf), dtype=bool)
    for (off, ln, ref), i in zip(m.table, new):
        assert off == o and off % 16 == 0 and ln > 0
        cover[off:off + ln] = True
        o = P.align16(off + ln)
    assert len(m.buf) == o and not m.buf[~cover].any()
    assert m.bytes == m.table[-1][0] + m.table[-1][1] == info["need_bytes"]
    assert info["added_bytes"] == sum(ln for _, ln, _ in m.table) == int(cover.sum())
    # the bytes are the items' bytes
    host, soff, _ = DC.place(streams)
    for (off, ln, ref), i in zip(m.table, new):
        if i < nrec:
            c = recs[i]
            at = soff[int(c["stream"])] + int(c["offset"])
            want = host[at:at + ln]
            assert ln == int(c["len"]) and ref == c["ref"].tobytes()
        else:
            n = nodes[i - nrec]
            want = arena[int(n["blob_off"]):int(n["blob_off"]) + ln]
            assert ln == int(n["blob_len"]) and ref == n["ref"].tobytes()
        assert m.buf[off:off + ln].tobytes() == want.tobytes()
    # where: every item's ref sits in the blob it names
    allrefs = [x.tobytes() for x in recs["ref"]] + [x.tobytes() for x in nodes["ref"]]
    assert [m.table[int(k)][2] for k in m.where] == allrefs


def test_second_put_and_flags(run, oracle, table):
    r, (bits, mn, fanout) = run
    m = P.Model(1 << 22, 1 << 14)
    m.put(r)
    before = (list(m.table), m.buf.copy(), m.bytes)
    rc, info = m.put(r)                                   # the same run: nothing new
    assert rc == P.OK and info["added"] == 0 and info["known"] == info["items"]
    assert (m.table, m.bytes) == (before[0], before[2]) and (m.buf == before[1]).all()
    assert info["need_bytes"] == m.bytes and info["need_blobs"] == len(m.table)
    s2 = [edit_stream(r[1][0], 5, sites=3, span=256), r[1][5], splitmix_array(9, 7001)]
    r2 = P.oracle_run(oracle, table, s2, bits, mn, fanout)
    held = list(m.table)
    rc, info = m.put(r2)
    assert rc == P.OK and 0 < info["known"] and info["added"] == len(P.brute_put(held, r2)) > 0
    assert m.table[:len(held)] == held and (m.buf[:len(before[1])] == before[1]).all()
    assert info["first_blob"] == len(held) and m.table[len(held)][0] == P.align16(before[2])
    # chunks only, then nodes only, is both at once
    one, two = P.Model(1 << 22, 1 << 14), P.Model(1 << 22, 1 << 14)
    one.put(r)
    i1 = two.put(r, P.CHUNKS)[1]
    i2 = two.put(r, P.NODES)[1]
    assert two.table == one.table and (two.buf == one.buf).all()
    assert i1["added"] + i2["added"] == len(one.table) and i2["first_blob"] == i1["added"]


def test_full_is_all_or_nothing(run):
    r, _ = run
    need = P.Model(1 << 22, 1 << 14).put(r)[1]
    for cb, cn in ((need["need_bytes"] - 1, need["need_blobs"]),
                   (need["need_bytes"], need["need_blobs"] - 1)):
        m = P.Model(cb, cn)
        rc, info = m.put(r)
        assert rc == P.ENOMEM and info == need
        assert m.table == [] and m.bytes == 0 and len(m.buf) == 0 and m.where is None
    m = P.Model(need["need_bytes"], need["need_blobs"])
    assert m.put(r) == (P.OK, need)


def test_home_rule():
    assert [P.slots_of(c) for c in (0, 1, 2, 3, 8, 9, 1000)] == [2, 2, 4, 8, 16, 32, 2048]
    ref = bytes(range(1, 33))
    assert DC.home(ref, 16) == 1 and DC.home(ref, 1 << 12) == 0x201
    m = P.Model(1 << 10, 8)
    # three refs at home 15 and one at home 0 of 16 slots: two of them wrap
    for k, head in enumerate((15, 31, 47, 0)):
        m.table.append((16 * k, 1, head.to_bytes(8, "little") + bytes([k]) * 24))
    assert m.homes() == [15, 15, 15, 0] and m.wrapped() == [1, 2]

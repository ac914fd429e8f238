"""blob_cases held to what it claims: put_blobs and get against a brute-force dict store on the
GPU tests' length edges, known refs and capacity; put_blobs of an oracle run's chunks and then its
nodes against pool_cases.Model.put of the run; the header declares both calls. No GPU needed."""
import hashlib

import numpy as np
import pytest

import blob_cases as B
import dedup_cases as DC
import pool_cases as P
from bs_amd import bsgpu
from bs_amd.synth import splitmix_array

CAP = (1 << 20, 256)


class Brute:
    """A store that compares every pair: blobs in the order of their first Put."""

    def __init__(self):
        self.blobs = []  # (ref, bytes)

    def put(self, data: bytes) -> bool:
        r = hashlib.sha256(data).digest()
        if any(r == h for h, _ in self.blobs):
            return False
        self.blobs.append((r, data))
        return True

    def get(self, ref: bytes):
        return next((d for h, d in self.blobs if h == ref), None)


def _held(m: P.Model, store: Brute):
    """The model holds the store's blobs in the store's order, 16-aligned, zero padded, packed."""
    assert [r for _, _, r in m.table] == [r for r, _ in store.blobs]
    at = 0
    for k, (o, n, _) in enumerate(m.table):
        assert o == P.align16(at) and m.blob_bytes(k) == store.blobs[k][1]
        assert not m.buf[o + n:P.align16(o + n)].any() and not m.buf[at:o].any()
        at = o + n
    assert m.bytes == at and m.index == {r: k for k, (r, _) in enumerate(store.blobs)}


def _put(m, store, src, off, lens):
    first = len(store.blobs)
    raw = src.tobytes()
    added = [store.put(raw[o:o + n]) for o, n in zip(off, lens)]
    rc, info, refs = B.put_blobs(m, src, off, lens)
    assert rc == B.OK and refs == [hashlib.sha256(raw[o:o + n]).digest() for o, n in zip(off, lens)]
    _held(m, store)
    # PutMulti's map[Ref]bool: a ref is new iff its where is at or past first_blob, and the item
    # that brought it is the first with that where
    w = m.where.tolist()
    assert [x >= first for x in w] == [store.blobs[x][0] not in
                                       [r for r, _ in store.blobs[:first]] for x in w]
    assert [i for i in range(len(w)) if w[i] >= first and w.index(w[i]) == i] == \
        [i for i, a in enumerate(added) if a]
    assert info["items"] == len(off) and info["added"] == sum(added)
    assert info["first_blob"] == first and info["need_blobs"] == len(store.blobs)
    assert info["added_bytes"] == sum(len(d) for _, d in store.blobs[first:])
    assert info["need_bytes"] == m.bytes
    return info


def _get(m, store, refs, cap=1 << 20, verify=False):
    rc, info, idx, out_off, out = B.get(m, refs, cap, verify)
    assert rc == B.OK
    got = [store.get(r) for r in refs]
    assert info["found"] == sum(g is not None for g in got)
    assert info["missing"] == len(refs) - info["found"]
    assert info["bytes"] == sum(len(g) for g in got if g is not None)
    at = 0
    for q, g in enumerate(got):
        assert int(out_off[q]) == at
        if g is None:
            assert int(idx[q]) == B.NONE64
            continue
        assert m.table[int(idx[q])][2] == refs[q]
        assert out[at:at + len(g)].tobytes() == g and not out[at + len(g):P.align16(len(g))].any()
        at += P.align16(len(g))
    assert int(out_off[-1]) == at == info["need_bytes"] == len(out)
    assert out.tobytes() == B.get_gather(m, idx, out_off).tobytes()
    return info


def test_edges_known_and_get():
    src, off, lens, facts = B.edge_case()
    m, store = P.Model(*CAP), Brute()
    info = _put(m, store, src, off, lens)
    assert info["added"] == facts["distinct"] and info["repeats"] == facts["repeats"]
    assert info["known"] == 0 and sorted(n for _, n, _ in m.table) == \
        sorted(B.EDGE_LENS + (1234,))
    # the same put again: nothing is new, where is the same
    where = m.where.tolist()
    info = _put(m, store, src, off, lens)
    assert info["added"] == 0 and info["known"] == facts["items"] and m.where.tolist() == where
    # some known, some new
    more = [splitmix_array(90 + i, n) for i, n in enumerate((7, 0, 300))]
    src2, off2, lens2 = B.place(more + [src[off[0]:off[0] + lens[0]]])
    info = _put(m, store, src2, off2, lens2)
    assert info["known"] == 2 and info["added"] == 2

    refs = [r for _, _, r in m.table]
    miss = [hashlib.sha256(b"no such blob %d" % i).digest() for i in range(3)]
    empty = hashlib.sha256(b"").digest()
    _get(m, store, refs)
    _get(m, store, [miss[0]] + refs[:4] + [miss[1]] + refs[4:] + [miss[2]])
    _get(m, store, [refs[5], refs[5], empty, refs[5]], verify=True)
    _get(m, store, [])
    _get(m, store, miss)
    # the stat form, the capacity rule and a planted flip
    rc, info, idx, out_off, out = B.get(m, refs, None)
    assert rc == B.OK and out is None and info["need_bytes"] == int(out_off[-1])
    need = info["need_bytes"]
    assert B.get(m, refs, need)[0] == B.OK and B.get(m, refs, need - 16)[0] == B.ENOMEM
    k = next(k for k, (_, n, _) in enumerate(m.table) if n == 65)
    m.buf[m.table[k][0] + 64] ^= 1
    rc, info, _, _, out = B.get(m, refs, need, verify=True)
    assert rc == B.ECORRUPT and info["bad_blob"] == k and out is None
    assert info["verified"] == sum(n for _, n, _ in m.table)
    rc, info, _, _, _ = B.get(m, refs[:k] + refs[:k], 2 * need, verify=True)
    assert rc == B.OK and info["verified"] == sum(n for _, n, _ in m.table[:k])


def test_capacity_is_all_or_nothing():
    src, off, lens, _ = B.edge_case()
    big = P.Model(*CAP)
    assert B.put_blobs(big, src, off, lens)[0] == B.OK
    for cap in ((big.bytes, len(big.table)), (big.bytes - 1, len(big.table)),
                (big.bytes, len(big.table) - 1)):
        m = P.Model(*cap)
        rc, info, refs = B.put_blobs(m, src, off, lens)
        assert rc == (B.OK if cap == (big.bytes, len(big.table)) else B.ENOMEM)
        assert info["need_bytes"] == big.bytes and info["need_blobs"] == len(big.table)
        assert refs == B.refs_of(src, off, lens)
        if rc:
            assert not m.table and m.bytes == 0 and m.where is None


@pytest.mark.parametrize("bits,mn,fanout", [(4, 64, 2), (6, 64, 3)])
def test_a_runs_chunks_then_nodes_is_its_put(oracle, table, bits, mn, fanout):
    a = splitmix_array(1, 9107)
    streams = [a, a[:5000].copy(), np.zeros(0, np.uint8), splitmix_array(3, 40)]
    run = P.oracle_run(oracle, table, streams, bits, mn, fanout)
    recs, _, nodes, arena = run
    want = P.Model(*CAP)
    rc, winfo = want.put(run)
    assert rc == P.OK and winfo["repeats"] > 0

    host, soff, _ = DC.place(streams)
    src = np.concatenate([host, np.asarray(arena, dtype=np.uint8), np.zeros(256, np.uint8)])
    off = (np.asarray(soff, dtype=np.int64)[recs["stream"]] + recs["offset"].astype(np.int64)) \
        .tolist() + (len(host) + nodes["blob_off"].astype(np.int64)).tolist()
    lens = recs["len"].tolist() + nodes["blob_len"].tolist()
    # (a chunk starts anywhere in its stream; the model takes any offset, the device call wants
    # multiples of 16, so the GPU test repacks)
    m = P.Model(*CAP)
    rc, info, refs = B.put_blobs(m, src, off, lens)
    assert rc == B.OK and info == winfo
    assert refs == [r.tobytes() for r in recs["ref"]] + [r.tobytes() for r in nodes["ref"]]
    assert m.table == want.table and m.bytes == want.bytes and m.index == want.index
    assert m.buf.tobytes() == want.buf.tobytes() and m.where.tolist() == want.where.tolist()


def test_header_declares_both_calls():
    names = bsgpu.exported_symbols_from_header()
    assert "bsg_pool_put_blobs" in names and "bsg_pool_get" in names
    assert "bsg_pool_blobs_ms_debug" not in names

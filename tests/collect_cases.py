"""The model for bsg_pool_collect / bsg_pool_reset.

It is composed from what is already pinned: gc_cases.mark over a pool_cases.Model gives the
verdicts, the info and live[]; the layout is gc_cases.layout(align16=True) and the bytes are
gc_cases.compacted, both restated here as numpy prefix sums so that a pool of several hundred
thousand blobs costs no Python loop (tests/test_collect_cases_cpu.py holds the restatement to
gc_cases, and the whole model to a fresh Model into which the live blobs are put one by one).
The result is a pool_cases.Model, so Model.put continues it and Model.wrapped / homes speak of
its index. tests/test_gpu_pool_collect*.py hold the device to it."""
from __future__ import annotations

import numpy as np

import dedup_cases as DC
import gc_cases as G
import pool_cases as P
from bs_amd.bsgpu import CHUNK_DTYPE, TREE_NODE_DTYPE

OK, EINVAL, ENOMEM, ESTATE, ENOTFOUND, ECORRUPT = P.OK, P.EINVAL, P.ENOMEM, P.ESTATE, \
    G.ENOTFOUND, G.ECORRUPT
NONE = G.NONE


def layout16(blobs, live):
    """gc_cases.layout(blobs, live, True) without a loop: (table, end16)."""
    at = np.flatnonzero(live)
    t = blobs[at].copy()
    n = t["len"].astype(np.uint64)
    pad = (n + np.uint64(15)) & ~np.uint64(15)
    t["off"] = np.cumsum(pad) - pad
    return t, int(t["off"][-1] + n[-1]) if len(at) else 0


def gathered(buf, blobs, live) -> np.ndarray:
    """gc_cases.compacted(buf, blobs, live, True) without a loop."""
    t, end = layout16(blobs, live)
    n = t["len"].astype(np.int64)
    out = np.zeros(end, dtype=np.uint8)
    run0 = np.cumsum(n) - n
    j = np.arange(int(n.sum()), dtype=np.int64)
    so = blobs["off"][np.flatnonzero(live)].astype(np.int64)
    out[np.repeat(t["off"].astype(np.int64) - run0, n) + j] = buf[np.repeat(so - run0, n) + j]
    return out


def collect(src: P.Model, roots, cap_bytes: int, cap_blobs: int, flags: int = 0):
    """(rc, status, info, dst, remap) of bsg_pool_collect of `src` into an empty pool of the given
    capacity: info is the bsg_pool_collect_info as a dict, dst the pool afterwards as a
    pool_cases.Model and remap one uint64 per blob of src; both None unless rc is OK."""
    blobs = src.blobs()
    rc, status, gi, live = G.mark(src.blob_bytes, blobs, roots, src.stat()["pool_bytes"], flags)
    info = {"gc": gi, "need_bytes": 0, "need_blobs": 0}
    if rc != OK:
        return rc, status, info, None, None
    table, end = layout16(blobs, live)
    info["need_bytes"], info["need_blobs"] = end, len(table)
    if end > cap_bytes or len(table) > cap_blobs:
        return ENOMEM, status, info, None, None
    dst = P.Model(cap_bytes, cap_blobs)
    raw = np.ascontiguousarray(table["ref"]).tobytes()
    dst.table = [(o, n, raw[32 * j:32 * j + 32])
                 for j, (o, n) in enumerate(zip(table["off"].tolist(), table["len"].tolist()))]
    dst.index = {r: j for j, (_, _, r) in enumerate(dst.table)}
    dst.bytes = end
    dst.buf = np.zeros(P.align16(end), dtype=np.uint8)
    dst.buf[:end] = gathered(src.buf, blobs, live)
    remap = np.full(len(blobs), NONE, dtype=np.uint64)
    remap[np.flatnonzero(live)] = np.arange(len(table), dtype=np.uint64)
    return OK, status, info, dst, remap


def taken_slots(m: P.Model) -> set:
    """The index slots a pool's entries hold. Which ref sits in which slot of a cluster depends on
    the order of the inserts; the set of taken slots does not."""
    return set(DC.probe_slots([r for _, _, r in m.table], P.slots_of(m.cap_blobs)).values())


def one_blob_run(data: bytes, ref: bytes):
    """A run whose one item is a record of stream 0 that carries `data` under `ref`: what
    Model.put takes to append exactly this blob."""
    rec = np.zeros(1, dtype=CHUNK_DTYPE)
    rec[0]["len"] = len(data)
    rec[0]["ref"] = np.frombuffer(ref, dtype=np.uint8)
    return (rec, [np.frombuffer(data, dtype=np.uint8)], np.zeros(0, dtype=TREE_NODE_DTYPE),
            np.zeros(0, dtype=np.uint8))


def brute(src: P.Model, live, cap_bytes: int, cap_blobs: int) -> P.Model:
    """The collected pool restated: a fresh Model into which exactly the live blobs are put, one
    by one, in index order."""
    m = P.Model(cap_bytes, cap_blobs)
    for k in np.flatnonzero(live):
        rc, info = m.put(one_blob_run(src.blob_bytes(int(k)), src.table[int(k)][2]), P.CHUNKS)
        assert rc == OK and info["added"] == 1, (k, rc, info)
    return m

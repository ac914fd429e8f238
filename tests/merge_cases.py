"""The model for bsg_pool_merge / bsg_pool_sync.

It is composed from what is already pinned: gc_cases.mark over a pool_cases.Model selects (or
every blob, with ALL), a search of the destination's sorted refs says which selected blobs are
new, collect_cases.layout16 / gathered give the new blobs' places and bytes from the base
align16(dst.bytes), and BSG_MERGE_VERIFY is hashlib over the new blobs' bytes. The result is a
pool_cases.Model, so Model.put, collect_cases.collect and a further merge continue it.
tests/test_merge_cases_cpu.py holds the model to a destination into which the new blobs are put
one by one; tests/test_gpu_pool_merge*.py hold the device to it."""
from __future__ import annotations

import copy
import hashlib

import numpy as np

import collect_cases as C
import gc_cases as G
import pool_cases as P

OK, EINVAL, ENOMEM, ESTATE, ENOTFOUND, ECORRUPT = C.OK, C.EINVAL, C.ENOMEM, C.ESTATE, \
    C.ENOTFOUND, C.ECORRUPT
NONE = C.NONE
MISSING_LEAVES, ALL, VERIFY = 1, 2, 4
GC_ZERO = dict.fromkeys(("bad_root", "bad_blob", "nlive", "live_bytes", "ndead", "dead_bytes",
                         "nnodes", "missing_leaves", "depth"), 0)


def clone(m: P.Model) -> P.Model:
    out = P.Model(m.cap_bytes, m.cap_blobs)
    out.table, out.index, out.bytes = list(m.table), dict(m.index), m.bytes
    out.buf = m.buf.copy()
    out.where = None if m.where is None else m.where.copy()
    return out


def probe(sblobs, dblobs):
    """(found, at) per entry of the table sblobs: the table dblobs holds an entry under its ref
    (whatever len that entry has: refs are trusted labels), and that entry's index. No loop over
    the blobs: the refs compare as 32-byte strings, dblobs' sorted once."""
    s = np.ascontiguousarray(sblobs["ref"]).view("S32").reshape(-1)
    d = np.ascontiguousarray(dblobs["ref"]).view("S32").reshape(-1)
    if not len(s) or not len(d):
        return np.zeros(len(s), dtype=bool), np.zeros(len(s), dtype=np.uint64)
    order = np.argsort(d, kind="stable")
    pos = np.minimum(np.searchsorted(d[order], s), len(d) - 1)
    return d[order][pos] == s, order[pos].astype(np.uint64)


def new_of(src: P.Model, dst: P.Model, live) -> np.ndarray:
    """new[k]: blob k of src is selected and dst holds no entry under its ref."""
    return (np.asarray(live) != 0) & ~probe(src.blobs(), dst.blobs())[0]


def merge(src: P.Model, dst: P.Model, roots=None, flags: int = 0, marked=None):
    """(rc, status, info, dst', remap) of bsg_pool_merge of `src` into `dst`: info is the
    bsg_pool_merge_info as a dict, dst' the destination afterwards as a new pool_cases.Model
    (`dst` itself is never changed) and remap one uint64 per blob of src; both None unless rc is
    OK. status is None with ALL. marked: what gc_cases.mark returned for these arguments, if the
    caller has it already (a mark of several hundred thousand blobs takes seconds)."""
    blobs, n = src.blobs(), len(src.table)
    info = dict(gc=dict(GC_ZERO), selected=0, added=0, added_bytes=0, known=0,
                first_blob=0, need_bytes=0, need_blobs=0, bad_blob=NONE, verified=0)
    if flags & ALL:
        assert not roots and not flags & MISSING_LEAVES
        status, live = None, np.ones(n, dtype=np.uint8)
    else:
        rc, status, gi, live = marked or G.mark(src.blob_bytes, blobs, roots or [],
                                                src.stat()["pool_bytes"], flags & MISSING_LEAVES)
        info["gc"] = dict(gi)
        if rc != OK:
            return rc, status, info, None, None
    found, at = probe(blobs, dst.blobs())
    new = (np.asarray(live) != 0) & ~found
    first, base = len(dst.table), P.align16(dst.bytes)
    t, end = C.layout16(blobs, new)
    info.update(selected=int(np.count_nonzero(live)), added=len(t),
                added_bytes=int(t["len"].sum()), first_blob=first, need_blobs=first + len(t),
                need_bytes=base + end if len(t) else dst.bytes)
    info["known"] = info["selected"] - info["added"]
    if flags & VERIFY:
        info["verified"] = info["added_bytes"]
        bad = [int(k) for k in np.flatnonzero(new)
               if hashlib.sha256(src.blob_bytes(int(k))).digest() != src.table[int(k)][2]]
        if bad:
            info["bad_blob"] = bad[0]
            return ECORRUPT, status, info, None, None
    if info["need_bytes"] > dst.cap_bytes or info["need_blobs"] > dst.cap_blobs:
        return ENOMEM, status, info, None, None
    out = clone(dst)
    remap = np.full(n, NONE, dtype=np.uint64)
    known = (np.asarray(live) != 0) & found
    remap[known] = at[known]
    remap[np.flatnonzero(new)] = first + np.arange(len(t), dtype=np.uint64)
    if len(t):
        raw = np.ascontiguousarray(t["ref"]).tobytes()
        for j, (o, ln) in enumerate(zip(t["off"].tolist(), t["len"].tolist())):
            r = raw[32 * j:32 * j + 32]
            out.table.append((base + o, ln, r))
            out.index[r] = first + j
        out.bytes = base + end
        buf = np.zeros(P.align16(out.bytes), dtype=np.uint8)
        buf[:len(dst.buf)] = dst.buf
        buf[base:base + end] = C.gathered(src.buf, blobs, new)
        out.buf = buf
    return OK, status, info, out, remap


def sync(a: P.Model, b: P.Model, flags: int = 0):
    """(rc, info[2], a', b', remap_b, remap_a) of bsg_pool_sync: each direction is merge(ALL)
    against the other pool as it stands at the call, and nothing is written unless both fit.
    remap_b (b's) covers a's blobs, remap_a (a's) b's. The pools and remaps are None unless rc
    is OK; `a` and `b` themselves are never changed."""
    assert not flags & ~VERIFY
    ab = merge(a, b, None, ALL | flags)
    ba = merge(b, a, None, ALL | flags)
    info = [ab[2], ba[2]]
    for rc in (ECORRUPT, ENOMEM):                 # both verifications, then both capacities
        for res in (ab, ba):
            if res[0] == rc:
                return rc, info, None, None, None, None
    assert ab[0] == OK and ba[0] == OK
    return OK, info, ba[3], ab[3], ab[4], ba[4]


def brute(src: P.Model, dst: P.Model, new) -> P.Model:
    """The merged destination restated: a copy of dst into which exactly the new blobs are put,
    one by one, in src's index order."""
    m = copy.deepcopy(dst)
    for k in np.flatnonzero(new):
        rc, info = m.put(C.one_blob_run(src.blob_bytes(int(k)), src.table[int(k)][2]), P.CHUNKS)
        assert rc == OK and info["added"] == 1, (k, rc, info)
    return m

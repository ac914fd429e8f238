"""The model for bsg_pool_put_blobs / bsg_pool_get, in plain Python over pool_cases.Model.

put_blobs hashes with hashlib and applies bsg_engine_pool_put's rules to the blobs in the place of
records and nodes (include/bsgpu.h); get applies GetMulti's: a partial result, every found blob at
the exclusive prefix sum of the padded lens in request order. tests/test_blob_cases_cpu.py holds
both to a brute-force dict store, tests/test_gpu_pool_blobs*.py hold the device to them."""
from __future__ import annotations

import hashlib

import numpy as np

import pool_cases as P
from bs_amd.bsgpu import GET_VERIFY as VERIFY, PoolGetInfo

OK, EINVAL, ENOMEM, ESTATE, ECORRUPT = P.OK, P.EINVAL, P.ENOMEM, P.ESTATE, -74
NONE64 = (1 << 64) - 1
GET_FIELDS = tuple(k for k, _ in PoolGetInfo._fields_)
assert VERIFY == 1 and GET_FIELDS == ("found", "missing", "bytes", "need_bytes", "bad_blob",
                                      "verified")


def place(blobs, gap=0):
    """Blobs packed at 16-byte offsets with `gap` spare vectors between them, and the read slack
    behind: (src, off, lens)."""
    off, o = [], 0
    for b in blobs:
        off.append(o)
        o += P.align16(len(b)) + 16 * gap
    src = np.zeros(o + 256, dtype=np.uint8)
    for b, p in zip(blobs, off):
        src[p:p + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
    return src, off, [len(b) for b in blobs]


def refs_of(src, off, lens) -> list:
    raw = np.ascontiguousarray(src, dtype=np.uint8).tobytes()
    return [hashlib.sha256(raw[o:o + n]).digest() for o, n in zip(off, lens)]


def put_blobs(m: P.Model, src, off, lens):
    """(rc, info, refs) of one bsg_pool_put_blobs of src[off[i] .. off[i] + lens[i]) into `m`,
    which is written on success only."""
    src = np.ascontiguousarray(src, dtype=np.uint8)
    off, lens = [int(o) for o in off], [int(n) for n in lens]
    refs = refs_of(src, off, lens)
    first_blob = len(m.table)
    info = dict.fromkeys(P.INFO_FIELDS, 0)
    info.update(items=len(refs), first_blob=first_blob)
    mine, new, where = {}, [], []
    for i, r in enumerate(refs):
        if r in m.index:
            info["known"] += 1
        if r in mine:
            info["repeats"] += 1
        elif r in m.index:
            mine[r] = m.index[r]
        else:
            mine[r] = first_blob + len(new)
            new.append(i)
        where.append(mine[r])
    base = P.align16(m.bytes)
    nl = np.array([lens[i] for i in new], dtype=np.int64)
    pad = (nl + 15) & ~15
    dst = base + np.cumsum(pad) - pad
    info["added"], info["added_bytes"] = len(new), int(nl.sum())
    info["need_blobs"] = first_blob + len(new)
    info["need_bytes"] = int(dst[-1] + nl[-1]) if new else m.bytes
    if info["need_bytes"] > m.cap_bytes or info["need_blobs"] > m.cap_blobs:
        return ENOMEM, info, refs
    if new:
        buf = np.zeros(int(dst[-1] + pad[-1]), dtype=np.uint8)
        buf[:len(m.buf)] = m.buf
        sat = np.array([off[i] for i in new], dtype=np.int64)
        run0 = np.cumsum(nl) - nl
        j = np.arange(int(nl.sum()), dtype=np.int64)
        buf[np.repeat(dst - run0, nl) + j] = src[np.repeat(sat - run0, nl) + j]
        m.buf = buf
        for k, i in enumerate(new):
            m.table.append((int(dst[k]), lens[i], refs[i]))
            m.index[refs[i]] = first_blob + k
        m.bytes = info["need_bytes"]
    m.where = np.array(where, dtype=np.uint64)
    return OK, info, refs


def get(m: P.Model, refs, cap, verify=False):
    """(rc, info, idx, out_off, out) of one bsg_pool_get of `refs` (a list of 32-byte refs) with
    an output of `cap` bytes (None: the stat form, no output). out is the output's first
    out_off[n] bytes, or None where the call writes none."""
    idx = [m.index.get(bytes(r), NONE64) for r in refs]
    lens = [m.table[k][1] if k != NONE64 else 0 for k in idx]
    out_off = [0]
    for k, n in zip(idx, lens):
        out_off.append(out_off[-1] + (P.align16(n) if k != NONE64 else 0))
    info = dict.fromkeys(GET_FIELDS, 0)
    found = [k for k in idx if k != NONE64]
    info.update(found=len(found), missing=len(idx) - len(found), bytes=sum(lens),
                need_bytes=out_off[-1], bad_blob=NONE64)
    idx, out_off = np.array(idx, dtype=np.uint64), np.array(out_off, dtype=np.uint64)
    if cap is not None and info["need_bytes"] > cap:
        return ENOMEM, info, idx, out_off, None
    if verify:
        for k in sorted(set(found)):
            info["verified"] += m.table[k][1]
            if hashlib.sha256(m.blob_bytes(k)).digest() != m.table[k][2] \
                    and info["bad_blob"] == NONE64:
                info["bad_blob"] = k
        if info["bad_blob"] != NONE64:
            return ECORRUPT, info, idx, out_off, None
    if cap is None:
        return OK, info, idx, out_off, None
    out = np.zeros(info["need_bytes"], dtype=np.uint8)
    for q, k in enumerate(idx.tolist()):
        if k != NONE64:
            o, n, _ = m.table[k]
            out[int(out_off[q]):int(out_off[q]) + n] = m.buf[o:o + n]
    return OK, info, idx, out_off, out


def get_gather(m: P.Model, idx, out_off) -> np.ndarray:
    """get()'s output as one numpy gather, for requests of several hundred thousand refs."""
    idx = np.asarray(idx, dtype=np.uint64)
    hit = np.nonzero(idx != np.uint64(NONE64))[0]
    t = m.blobs()
    src = t["off"][idx[hit].astype(np.int64)].astype(np.int64)
    n = t["len"][idx[hit].astype(np.int64)].astype(np.int64)
    dst = np.asarray(out_off, dtype=np.uint64)[hit].astype(np.int64)
    out = np.zeros(int(out_off[-1]), dtype=np.uint8)
    run0 = np.cumsum(n) - n
    j = np.arange(int(n.sum()), dtype=np.int64)
    out[np.repeat(dst - run0, n) + j] = m.buf[np.repeat(src - run0, n) + j]
    return out


# ---- the length edges of the GPU tests -------------------------------------------------------------
EDGE_LENS = (0, 1, 15, 16, 17, 55, 56, 63, 64, 65, 119, 120, 4096, 40_000, 70_001)


def edge_case(seed=11):
    """(src, off, lens, facts): one blob of every length in EDGE_LENS from distinct splitmix bytes,
    laid out with gaps and put in descending order of offset; then an item that coincides with
    the 4,096-byte one (a repeat), one that is a prefix of the 40,000-byte one (another ref) and
    a second empty blob at another offset (a repeat of the first)."""
    from bs_amd.synth import splitmix_array
    blobs = [splitmix_array(seed + i, n) for i, n in enumerate(EDGE_LENS)]
    src, off, lens = place(blobs, gap=2)
    order = list(range(len(blobs)))[::-1]
    o = [off[i] for i in order] + [off[EDGE_LENS.index(4096)], off[EDGE_LENS.index(40_000)],
                                   off[3] + 16]
    n = [lens[i] for i in order] + [4096, 1234, 0]
    facts = {"items": len(o), "distinct": len(EDGE_LENS) + 1, "repeats": 2}
    return src, o, n, facts

"""The model for bsg_engine_read / bsg_pool_read.

A pruned breadth-first read in plain Python over walk_cases.parse_node, with the rules of
include/bsgpu.h: the Root is always visited, a child is followed if and only if its cover has a
byte in the range, a child that is not followed is neither looked up nor read, and with
BSG_READ_VERIFY exactly the touched blobs are hashed. tests/test_read_cases_cpu.py holds it to the
oracle's trees and to walk_cases.model; tests/test_gpu_read*.py hold the device to it."""
from __future__ import annotations

import numpy as np

import walk_cases as W
from bs_amd.bsgpu import READ_SLACK, WALK_MAX_DEPTH

OK, EINVAL, ENOTFOUND, ECORRUPT, ESTATE = W.OK, W.EINVAL, W.ENOTFOUND, W.ECORRUPT, W.ESTATE
NONE = W.NONE
VERIFY = 1
U64 = (1 << 64) - 1
_RANK = {0: OK, 1: ECORRUPT, 2: ENOTFOUND}


def fresh_info() -> dict:
    return {"bad_range": NONE, "bad_blob": NONE, "nnodes": 0, "nleaves": 0, "bytes": 0,
            "verified": 0, "depth": 0}


def got_of(size: int, offset: int, n: int) -> int:
    return min(n, size - min(offset, size))


def model(blob_bytes, blobs, ranges, pool_bytes, out_off=None, out_cap=None, flags=0):
    """(rc, status, got, info, data, touched) of bsg_engine_read. blob_bytes(k): the bytes of pool
    blob k (asked for touched blobs only); blobs: the POOL_BLOB_DTYPE table; ranges: (root, offset,
    len) triples; out_off / out_cap: where the ranges go (default: one after the other, each at a
    multiple of 16). status is None for a fault of the first group of rules; got is all zero,
    data (the bytes of every range) None and touched (the set of blob indices) None unless rc is
    OK."""
    nr = len(ranges)
    info, got0 = fresh_info(), [0] * nr
    if out_off is None:
        out_off, out_cap = out_layout(ranges)
    offs, lens = blobs["off"].tolist(), blobs["len"].tolist()
    if (flags & ~VERIFY) or nr > 65535 or any(o + n > pool_bytes for o, n in zip(offs, lens)):
        return EINVAL, None, got0, info, None, None
    for (_, _, n), oo in zip(ranges, out_off):
        if oo % 16 or oo > out_cap or (n < 1 << 63 and oo + n > out_cap):
            return EINVAL, None, got0, info, None, None
    raw, index = np.ascontiguousarray(blobs["ref"]).tobytes(), {}
    for k in range(len(blobs)):
        index.setdefault(raw[32 * k:32 * k + 32], k)
    rank, sizes = [0] * nr, [0] * nr
    leaves = [[] for _ in range(nr)]  # (offset, len, blob)
    touched = set()

    def fail(q, r):
        rank[q] = max(rank[q], r)

    win = [(off, min(off + n, U64)) for _, off, n in ranges]
    frontier = []  # (range, blob, expected offset, expected size or None)
    for q, (root, _, _) in enumerate(ranges):
        if bytes(root) == bytes(32):
            continue
        k = index.get(bytes(root))
        if k is None:
            fail(q, 2)
        else:
            touched.add(k)
            frontier.append((q, k, 0, None))
    depth = 0
    while frontier:
        nxt = []
        for q, k, eoff, esize in frontier:
            info["nnodes"] += 1
            info["depth"] = max(info["depth"], depth)
            nd = W.parse_node(blob_bytes(k))
            if nd is None or nd[2] != eoff or (esize is not None and nd[3] != esize):
                fail(q, 1)
                continue
            kind, kids, noff, size = nd
            if depth == 0:
                sizes[q] = size
            w0, w1 = win[q]
            ends = [o for _, o in kids[1:]] + [noff + size]
            for (ref, off), end in zip(kids, ends):
                if off >= end:  # an empty cover: the listing node's fault, whatever the range
                    fail(q, 1)
                    continue
                if not (w0 < w1 and off < w1 and w0 < end):
                    continue  # not followed: neither looked up nor read
                if kind == 1 and depth == WALK_MAX_DEPTH:
                    fail(q, 1)
                    continue
                c = index.get(ref)
                if c is None:
                    fail(q, 2)
                elif kind == 1:
                    touched.add(c)
                    nxt.append((q, c, off, end - off))
                elif lens[c] != end - off:
                    fail(q, 1)
                else:
                    leaves[q].append((off, end - off, c))
        frontier = nxt
        depth += 1

    want = [got_of(sizes[q], off, n) for q, (_, off, n) in enumerate(ranges)]
    spans = sorted((oo, oo + g) for oo, g in zip(out_off, want) if g)
    if any(oo + g > out_cap for oo, g in zip(out_off, want)) or \
            any(b[0] < a[1] for a, b in zip(spans, spans[1:])):
        return EINVAL, None, got0, fresh_info(), None, None
    status = np.array([_RANK[r] for r in rank], dtype=np.int32)
    bad = [q for q in range(nr) if rank[q]]
    if bad:
        info["bad_range"] = bad[0]
        return (ENOTFOUND if 2 in rank else ECORRUPT), status, got0, info, None, None
    info["nleaves"] = sum(len(x) for x in leaves)
    for x in leaves:
        touched.update(c for _, _, c in x)
    if flags & VERIFY:
        order = sorted(touched)
        if any(offs[k] % 16 or lens[k] >= 1 << 40 or pool_bytes - offs[k] - lens[k] < READ_SLACK
               for k in order):
            return EINVAL, status, got0, info, None, None
        info["verified"] = sum(lens[k] for k in order)
        wrong = [k for k in order if W.sha(blob_bytes(k)) != raw[32 * k:32 * k + 32]]
        if wrong:
            info["bad_blob"] = wrong[0]
            return ECORRUPT, status, got0, info, None, None
    data = []
    for q, (_, off, _) in enumerate(ranges):
        x = sorted(leaves[q])
        whole = b"".join(blob_bytes(c) for _, _, c in x)
        skip = off - x[0][0] if x else 0
        data.append(whole[skip:skip + want[q]])
        assert len(data[-1]) == want[q]
    info["bytes"] = sum(want)
    return OK, status, want, info, data, touched


def run_model(pool, blobs, ranges, pool_bytes=None, **kw):
    return model(W.getter(pool, blobs), blobs, ranges,
                 len(pool) if pool_bytes is None else pool_bytes, **kw)


def out_layout(ranges, sizes=None):
    """Every range's place in one output, one after the other at multiples of 16 with a gap
    between them: (out_off, out_cap). A range takes min(len, 2^20) bytes of room, or with `sizes`
    (one per range) what it gets."""
    off, o = [], 0
    for q, (_, offset, n) in enumerate(ranges):
        off.append(o)
        room = min(n, 1 << 20) if sizes is None else got_of(sizes[q], offset, n)
        o += (room + 15 & ~15) + 16
    return off, o


# ---- where a tree's boundaries lie ---------------------------------------------------------------
def boundaries(blob_bytes, blobs, root):
    """The stream offsets at which the chunks, the leaf nodes and the Root's children under `root`
    start (each list ascending, 0 included), and the stream's size: (chunks, leaf_nodes, top,
    size). The pool must hold the whole tree."""
    raw, index = np.ascontiguousarray(blobs["ref"]).tobytes(), {}
    for k in range(len(blobs)):
        index.setdefault(raw[32 * k:32 * k + 32], k)
    chunks, leaf_nodes, top, size = [], [], [], 0
    todo = [(index[bytes(root)], 0)]
    while todo:
        k, depth = todo.pop()
        kind, kids, noff, sz = W.parse_node(blob_bytes(k))
        if depth == 0:
            size, top = sz, [o for _, o in kids]
        if kind == 2:
            leaf_nodes.append(noff)
            chunks += [o for _, o in kids]
        else:
            todo += [(index[r], depth + 1) for r, _ in kids]
    return sorted(chunks), sorted(leaf_nodes), top, size

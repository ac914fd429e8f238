"""Inputs and the model for bsg_pool / bsg_engine_pool_put.

The model is plain Python with the rules of include/bsgpu.h: a dict from ref to blob index, the
offset rule (every blob at a multiple of 16, the k-th appended item right after the one before
it, padding zero) and the index's home rule (a ref's first 8 bytes, little-endian,
masked to the smallest power of two >= 2 x max(cap_blobs, 1) slots). A run is given as
(records, the streams' bytes, tree nodes, tree arena); tests/test_pool_cases_cpu.py holds the
model to what it claims on runs built from the oracle and tree_form.listing,
tests/test_gpu_pool*.py hold the device to it."""
from __future__ import annotations

import numpy as np

import dedup_cases as DC
import tree_form as TF
from bs_amd.bsgpu import CHUNK_DTYPE, POOL_BLOB_DTYPE, TREE_NODE_DTYPE

OK, EINVAL, ENOMEM, ESTATE, ENODEV = 0, -22, -12, -71, -19
CHUNKS, NODES = 1, 2
INFO_FIELDS = ("items", "added", "added_bytes", "known", "repeats", "first_blob", "need_bytes",
               "need_blobs")


def align16(x: int) -> int:
    return (x + 15) & ~15


def slots_of(cap_blobs: int) -> int:
    """The index's size: the smallest power of two >= 2 x max(cap_blobs, 1)."""
    s = 1
    while s < 2 * max(cap_blobs, 1):
        s <<= 1
    return s


# ---- runs --------------------------------------------------------------------------------------
def oracle_run(O, table, streams, bits, min_size, fanout):
    """(records, streams, nodes, arena) of one run from the oracle's split and the closed form of
    split.Writer's tree (tree_form.listing): what bsg_engine_chunks_device and
    bsg_engine_tree_nodes_device / _arena_device hold after bsg_engine_trees. Every blob of the
    arena starts at a multiple of 16."""
    recs = DC.oracle_records(O, table, streams, bits, min_size)
    rows, parts, o = [], [], 0
    for s in range(len(streams)):
        r = recs[recs["stream"] == s]
        L = TF.listing(r["ref"], r["len"], r["level"], fanout)
        for i in range(len(L["height"])):
            b0, bl = int(L["blob_start"][i]), int(L["blob_len"][i])
            rows.append((o, bl, s, int(L["height"][i]), 0, L["ref"][i]))
            parts.append((o, L["buf"][b0:b0 + bl]))
            o += align16(bl)
    nodes = np.zeros(len(rows), dtype=TREE_NODE_DTYPE)
    for i, row in enumerate(rows):
        nodes[i] = row
    arena = np.zeros(o, dtype=np.uint8)
    for at, b in parts:
        arena[at:at + len(b)] = b
    return recs, streams, nodes, arena


def roots_of(run) -> list:
    """Every stream's Root: its last listed node's ref, 32 zero bytes for an empty stream."""
    recs, streams, nodes, _ = run
    out = []
    for s in range(len(streams)):
        mine = nodes[nodes["stream"] == s]
        out.append(mine[-1]["ref"].tobytes() if len(mine) else bytes(32))
    return out


# ---- the model ---------------------------------------------------------------------------------
class Model:
    """The pool after a sequence of puts: table (a list of (off, len, ref)), buf (its bytes up to
    the end of the last blob's padding), bytes (the end of the last blob's last byte), index
    (ref -> blob index) and where (of the last successful put)."""

    def __init__(self, cap_bytes: int, cap_blobs: int):
        self.cap_bytes, self.cap_blobs = cap_bytes, cap_blobs
        self.table, self.index, self.bytes = [], {}, 0
        self.buf = np.zeros(0, dtype=np.uint8)
        self.where = None

    def stat(self) -> dict:
        return {"nblobs": len(self.table), "bytes": self.bytes, "cap_blobs": self.cap_blobs,
                "cap_bytes": self.cap_bytes, "pool_bytes": align16(self.cap_bytes) + 256}

    def blobs(self) -> np.ndarray:
        t = np.zeros(len(self.table), dtype=POOL_BLOB_DTYPE)
        if self.table:
            t["off"] = [o for o, _, _ in self.table]
            t["len"] = [n for _, n, _ in self.table]
            t["ref"] = np.frombuffer(b"".join(r for _, _, r in self.table),
                                     dtype=np.uint8).reshape(-1, 32)
        return t

    def blob_bytes(self, k: int) -> bytes:
        o, n, _ = self.table[k]
        return self.buf[o:o + n].tobytes()

    def put(self, run, flags: int = CHUNKS | NODES):
        """(rc, info) of one bsg_engine_pool_put of `run` into this pool."""
        recs, streams, nodes, arena = run
        host, off, _ = DC.place(streams)
        src = np.concatenate([host, np.asarray(arena, dtype=np.uint8)])
        refs, lens, at = [], [], []
        if flags & CHUNKS:
            raw = np.ascontiguousarray(recs["ref"]).tobytes()
            refs += [raw[32 * i:32 * i + 32] for i in range(len(recs))]
            lens += recs["len"].astype(np.int64).tolist()
            at += (np.asarray(off, dtype=np.int64)[recs["stream"]]
                   + recs["offset"].astype(np.int64)).tolist() if len(recs) else []
        if flags & NODES:
            raw = np.ascontiguousarray(nodes["ref"]).tobytes()
            refs += [raw[32 * i:32 * i + 32] for i in range(len(nodes))]
            lens += nodes["blob_len"].astype(np.int64).tolist()
            at += (len(host) + nodes["blob_off"].astype(np.int64)).tolist()
        first_blob = len(self.table)
        info = dict.fromkeys(INFO_FIELDS, 0)
        info.update(items=len(refs), first_blob=first_blob)
        mine, new, where = {}, [], []
        for i, r in enumerate(refs):
            if r in self.index:
                info["known"] += 1
            if r in mine:
                info["repeats"] += 1
            elif r in self.index:
                mine[r] = self.index[r]
            else:
                mine[r] = first_blob + len(new)
                new.append(i)
            where.append(mine[r])
        base = align16(self.bytes)
        nl = np.array([lens[i] for i in new], dtype=np.int64)
        pad = (nl + 15) & ~15
        dst = base + np.cumsum(pad) - pad
        info["added"], info["added_bytes"] = len(new), int(nl.sum())
        info["need_blobs"] = first_blob + len(new)
        info["need_bytes"] = int(dst[-1] + nl[-1]) if new else self.bytes
        if info["need_bytes"] > self.cap_bytes or info["need_blobs"] > self.cap_blobs:
            return ENOMEM, info
        if new:
            buf = np.zeros(int(dst[-1] + pad[-1]), dtype=np.uint8)
            buf[:len(self.buf)] = self.buf
            sat = np.array([at[i] for i in new], dtype=np.int64)
            run0 = np.cumsum(nl) - nl
            j = np.arange(int(nl.sum()), dtype=np.int64)
            buf[np.repeat(dst - run0, nl) + j] = src[np.repeat(sat - run0, nl) + j]
            self.buf = buf
            for k, i in enumerate(new):
                self.table.append((int(dst[k]), lens[i], refs[i]))
                self.index[refs[i]] = first_blob + k
            self.bytes = info["need_bytes"]
        self.where = np.array(where, dtype=np.uint64)
        return OK, info

    # the index ----------------------------------------------------------------------------------
    def homes(self) -> list:
        """Every table entry's home slot."""
        s = slots_of(self.cap_blobs)
        return [DC.home(r, s) for _, _, r in self.table]

    def wrapped(self) -> list:
        """The blobs whose index slot, under plain linear probing in table order, lies before
        their home: their probe sequence stepped off the last slot and went on from slot 0.
        (Which refs sit in which slots of a cluster depends on the order of the inserts; the set
        of taken slots, and so whether the cluster at the table's end wraps, does not.)"""
        s = slots_of(self.cap_blobs)
        where = DC.probe_slots([r for _, _, r in self.table], s)
        return [k for k, (_, _, r) in enumerate(self.table) if where[r] < DC.home(r, s)]


def brute_put(table, run, flags=CHUNKS | NODES):
    """Which items a put appends, by comparing every pair: the indices of the new items for a pool
    whose table (a list of (off, len, ref)) is given."""
    recs, _, nodes, _ = run
    refs = ([r.tobytes() for r in recs["ref"]] if flags & CHUNKS else []) + \
           ([r.tobytes() for r in nodes["ref"]] if flags & NODES else [])
    held = [r for _, _, r in table]
    return [i for i, r in enumerate(refs)
            if not any(r == h for h in held) and not any(r == refs[j] for j in range(i))]


def empty_records() -> np.ndarray:
    return np.zeros(0, dtype=CHUNK_DTYPE)

"""Inputs and the model for bsg_engine_walk.

The model is a plain breadth-first walk in Python with the acceptance rules of include/bsgpu.h:
a strict parser of PutProto's bytes (parse_node), the cover rules, the depth bound and the
per-stream status ranking. tests/test_walk_cases_cpu.py holds it to the oracle's trees
(oracle.py_tree_root) and to the C++ Reader; tests/test_gpu_walk*.py hold the device to it."""
from __future__ import annotations

import hashlib
import os
import re

import numpy as np

from bs_amd.bsgpu import CHUNK_DTYPE, POOL_BLOB_DTYPE, WALK_MAX_DEPTH
from oracle import oracle as O

OK, EINVAL, ENOTFOUND, ECORRUPT, ESTATE = 0, -22, -2, -74, -71
NONE = (1 << 64) - 1
FILL, GUARD = 0xA5, 256
_RANK = {0: OK, 1: ECORRUPT, 2: ENOTFOUND}


def sha(b) -> bytes:
    return hashlib.sha256(bytes(b)).digest()


# ---- the model ---------------------------------------------------------------------------------
def _varint(b: bytes, i: int):
    """A minimal, non-zero varint below 2^64 at b[i:]: (value, next index) or None."""
    v = 0
    for j in range(10):
        if i >= len(b):
            return None
        c = b[i]
        i += 1
        v |= (c & 0x7F) << (7 * j)
        if not c & 0x80:
            if c == 0 or (j == 9 and c > 1):
                return None
            return v, i
    return None


def parse_node(b: bytes):
    """(kind, [(ref, offset)], offset, size) if b is exactly what PutProto emits for a Node with
    children of one kind (1 nodes, 2 leaves), at least one, the first child's offset equal to the
    node's, strictly ascending offsets, size > 0 and offset + size < 2^64; else None."""
    i, kids, tag0 = 0, [], None
    while i < len(b) and b[i] in (0x0A, 0x12):
        tag = b[i]
        if tag0 is None:
            tag0 = tag
        if tag != tag0 or i + 2 > len(b):
            return None
        n = b[i + 1]
        e = b[i + 2:i + 2 + n]
        if n < 34 or len(e) != n or e[0] != 0x0A or e[1] != 0x20:
            return None
        off = 0
        if n > 34:
            if e[34] != 0x10:
                return None
            got = _varint(e, 35)
            if got is None or got[1] != n:
                return None
            off = got[0]
        if kids and off <= kids[-1][1]:
            return None
        kids.append((bytes(e[2:34]), off))
        i += 2 + n
    noff = 0
    if i < len(b) and b[i] == 0x18:
        got = _varint(b, i + 1)
        if got is None:
            return None
        noff, i = got
    if not (i < len(b) and b[i] == 0x20):
        return None
    got = _varint(b, i + 1)
    if got is None:
        return None
    size, i = got
    if i != len(b) or not kids or kids[0][1] != noff or noff + size >= 1 << 64:
        return None
    return (1 if tag0 == 0x0A else 2), kids, noff, size


def model(blob_bytes, blobs, roots, pool_bytes, flags=0):
    """(rc, status, info, records, sizes, counts) of bsg_engine_walk. blob_bytes(k): the bytes of
    pool blob k (asked for node blobs only); blobs: the POOL_BLOB_DTYPE table; roots: a list of
    32-byte refs. status is None for a layout fault; records, sizes and counts are None unless
    rc is OK."""
    ns = len(roots)
    info = {"bad_stream": NONE, "nrecs": 0, "nnodes": 0, "bytes": 0, "depth": 0}
    if flags != 0 or ns > 65535 or any(
            o + n > pool_bytes for o, n in zip(blobs["off"].tolist(), blobs["len"].tolist())):
        return EINVAL, None, info, None, None, None
    raw, index = np.ascontiguousarray(blobs["ref"]).tobytes(), {}
    for k in range(len(blobs)):
        index.setdefault(raw[32 * k:32 * k + 32], k)
    rank, sizes, recs = [0] * ns, [0] * ns, []

    def fail(s, r):
        rank[s] = max(rank[s], r)

    frontier = []  # (stream, blob, expected offset, expected size or None)
    for s, r in enumerate(roots):
        if bytes(r) == bytes(32):
            continue
        k = index.get(bytes(r))
        if k is None:
            fail(s, 2)
        else:
            frontier.append((s, k, 0, None))
    depth = 0
    while frontier:
        nxt = []
        for s, k, eoff, esize in frontier:
            info["nnodes"] += 1
            info["depth"] = max(info["depth"], depth)
            nd = parse_node(blob_bytes(k))
            if nd is None or nd[2] != eoff or (esize is not None and nd[3] != esize):
                fail(s, 1)
                continue
            kind, kids, noff, size = nd
            if depth == 0:
                sizes[s] = size
            ends = [o for _, o in kids[1:]] + [noff + size]
            for (ref, off), end in zip(kids, ends):
                if kind == 1 and depth == WALK_MAX_DEPTH:
                    fail(s, 1)
                    continue
                c = index.get(ref)
                if c is None:
                    fail(s, 2)
                elif off >= end:
                    fail(s, 1)
                elif kind == 1:
                    nxt.append((s, c, off, end - off))
                elif int(blobs[c]["len"]) != end - off:
                    fail(s, 1)
                else:
                    recs.append((s, off, end - off, ref))
        frontier = nxt
        depth += 1
    status = np.array([_RANK[r] for r in rank], dtype=np.int32)
    bad = [s for s in range(ns) if rank[s]]
    if bad:
        info["bad_stream"] = bad[0]
        return (ENOTFOUND if 2 in rank else ECORRUPT), status, info, None, None, None
    recs.sort(key=lambda r: (r[0], r[1]))
    out = np.zeros(len(recs), dtype=CHUNK_DTYPE)
    for i, (s, off, ln, ref) in enumerate(recs):
        out[i] = (off, ln, 0, s, np.frombuffer(ref, dtype=np.uint8))
    counts = np.bincount(out["stream"], minlength=ns).astype(np.uint64)[:ns]
    info["nrecs"], info["bytes"] = len(recs), int(sum(sizes))
    return OK, status, info, out, np.array(sizes, dtype=np.uint64), counts


# ---- pools -------------------------------------------------------------------------------------
def table_of(entries) -> np.ndarray:
    """A bsg_pool_blob table from (off, len, ref) triples."""
    t = np.zeros(len(entries), dtype=POOL_BLOB_DTYPE)
    if len(entries):
        assert all(len(ref) == 32 for _, _, ref in entries)
        t["off"] = np.array([off for off, _, _ in entries], dtype=np.uint64)
        t["len"] = np.array([ln for _, ln, _ in entries], dtype=np.uint64)
        t["ref"] = np.frombuffer(b"".join(bytes(ref) for _, _, ref in entries),
                                 dtype=np.uint8).reshape(-1, 32)
    return t


def pool_of(store: dict, first: int = 1):
    """The store's blobs packed tight from byte `first` on (so they start at odd and even
    addresses alike), in insertion order: (pool bytes, table)."""
    entries, parts, o = [], [bytes(first)], first
    for ref, b in store.items():
        entries.append((o, len(b), ref))
        parts.append(bytes(b))
        o += len(b)
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), table_of(entries)


def getter(pool, blobs):
    """blob_bytes for a pool held in host memory."""
    def f(k):
        o, n = int(blobs[k]["off"]), int(blobs[k]["len"])
        return pool[o:o + n].tobytes()
    return f


def run_model(pool, blobs, roots, pool_bytes=None, flags=0):
    return model(getter(pool, blobs), blobs, roots,
                 len(pool) if pool_bytes is None else pool_bytes, flags)


# ---- trees -------------------------------------------------------------------------------------
def oracle_tree(seed: int, nchunks: int, fanout: int):
    """A stream of nchunks random chunks through the oracle's TreeBuilder: (data, chunks, root,
    store), chunks being the (bytes, level) pairs."""
    rng = np.random.default_rng([seed, nchunks, fanout])
    chunks = [(rng.integers(0, 256, int(rng.integers(1, 200)), dtype=np.uint8).tobytes(),
               int(rng.choice([0, 0, 0, 1, 1, 2, 3, 5, 9]))) for _ in range(nchunks)]
    store = {}
    root = O.py_tree_root(chunks, fanout=fanout, store=store)
    return b"".join(c for c, _ in chunks), chunks, root, store


def chunk_records(chunks, stream=0) -> np.ndarray:
    """The records a walk must give for chunks (byte strings) in stream order."""
    out = np.zeros(len(chunks), dtype=CHUNK_DTYPE)
    o = 0
    for i, c in enumerate(chunks):
        out[i] = (o, len(c), 0, stream, np.frombuffer(sha(c), dtype=np.uint8))
        o += len(c)
    return out


def reachable_nodes(store, root) -> int:
    """Node blobs reachable from root, each visit counted (split.Protect's traversal)."""
    if root == bytes(32):
        return 0
    nodes, _, _, _ = O._unwrap(store, root)
    return 1 + sum(reachable_nodes(store, r) for r, _ in nodes)


class Tree:
    """A hand-made tree over leaf blobs: leaves (ref, len) in stream order grouped `arity` to a
    leaf node, nodes `arity` to a node, up to one Root. Every node is kept as its fields, so a
    test can change one and re-serialise: nodes[d] lists depth d's nodes (Root: nodes[0][0]) as
    dicts {ref, kind, kids [(ref, offset)], offset, size}; a node's ref is the SHA-256 of its
    unchanged bytes and stays its label whatever the bytes become."""

    def __init__(self, leaves, arity=3):
        level, o = [], 0
        for i in range(0, len(leaves), arity):
            kids, o0 = [], o
            for ref, ln in leaves[i:i + arity]:
                kids.append((ref, o))
                o += ln
            level.append(self._node(2, kids, o0, o - o0))
        self.nodes = [level]
        while len(level) > 1:
            up = []
            for i in range(0, len(level), arity):
                grp = level[i:i + arity]
                up.append(self._node(1, [(n["ref"], n["offset"]) for n in grp], grp[0]["offset"],
                                     sum(n["size"] for n in grp)))
            level = up
            self.nodes.insert(0, level)
        self.root = level[0]["ref"]
        self.size = level[0]["size"]

    @staticmethod
    def _node(kind, kids, offset, size):
        b = O.proto_node(kids if kind == 1 else [], kids if kind == 2 else [], offset, size)
        return {"ref": sha(b), "kind": kind, "kids": kids, "offset": offset, "size": size,
                "bytes": b}

    def store(self) -> dict:
        return {n["ref"]: n["bytes"] for lv in self.nodes for n in lv}


def leaf_blobs(seed: int, lens):
    """Random leaf blobs of the given lengths: ([(ref, len)], {ref: bytes})."""
    rng = np.random.default_rng(seed)
    out, store = [], {}
    for n in lens:
        b = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        store[sha(b)] = b
        out.append((sha(b), n))
    return out, store


def encode(n, tags=None, kids=None, offset=None, size=None, first_zero=False) -> bytes:
    """Node n's bytes with some fields replaced; tags: one wire tag per child (0x0a nodes, 0x12
    leaves) in the order given; first_zero: the first child's offset written out as `10 00`."""
    kids = n["kids"] if kids is None else kids
    offset = n["offset"] if offset is None else offset
    size = n["size"] if size is None else size
    tags = [0x0A if n["kind"] == 1 else 0x12] * len(kids) if tags is None else tags
    out = bytearray()
    for k, ((ref, off), tag) in enumerate(zip(kids, tags)):
        c = O.proto_child(ref, off)
        if k == 0 and first_zero:
            c = O.proto_child(ref, 0) + b"\x10\x00"
        out += bytes([tag]) + O._varint(len(c)) + c
    if offset:
        out += b"\x18" + O._varint(offset)
    if size:
        out += b"\x20" + O._varint(size)
    return bytes(out)


def _nonminimal(n):
    b = bytearray(n["bytes"])
    b[-1] |= 0x80  # the size's last byte gets a continuation bit and a zero byte after it
    return bytes(b) + b"\x00"


def _swap01(n):
    k = list(n["kids"])
    k[0], k[1] = (k[0][0], k[1][1]), (k[1][0], k[0][1])
    return k


# name -> (node -> new bytes, the status the family must give). Every target has two children
# at least. The node's label (its ref in the blob table) is unchanged.
FAMILIES = {
    "flip_marker": (lambda n: n["bytes"][:2] + bytes([n["bytes"][2] ^ 1]) + n["bytes"][3:],
                    ECORRUPT),
    "flip_ref": (lambda n: n["bytes"][:10] + bytes([n["bytes"][10] ^ 0x40]) + n["bytes"][11:],
                 ENOTFOUND),
    "truncated": (lambda n: n["bytes"][:-1], ECORRUPT),
    "padded": (lambda n: n["bytes"] + b"\x00", ECORRUPT),
    "ref31": (lambda n: encode(n, kids=[(n["kids"][0][0][:31], n["kids"][0][1])] + n["kids"][1:]),
              ECORRUPT),
    "nonminimal": (_nonminimal, ECORRUPT),
    "explicit_zero": (lambda n: encode(n, first_zero=True), ECORRUPT),
    "unknown_field": (lambda n: n["bytes"] + b"\x28\x01", ECORRUPT),
    "leaves_before_nodes": (lambda n: encode(n, tags=[0x12] + [0x0A] * (len(n["kids"]) - 1)),
                            ECORRUPT),
    "both_kinds": (lambda n: encode(n, tags=[0x0A] * (len(n["kids"]) - 1) + [0x12]), ECORRUPT),
    "no_child": (lambda n: encode(n, kids=[]), ECORRUPT),
    "first_offset": (lambda n: encode(n, kids=[(n["kids"][0][0], n["kids"][0][1] + 1)]
                                      + n["kids"][1:]), ECORRUPT),
    "equal_offsets": (lambda n: encode(n, kids=[n["kids"][0], (n["kids"][1][0], n["kids"][0][1])]
                                       + n["kids"][2:]), ECORRUPT),
    "descending": (lambda n: encode(n, kids=_swap01(n) + n["kids"][2:]), ECORRUPT),
    "size0": (lambda n: encode(n, size=0), ECORRUPT),
    "wrap": (lambda n: encode(n, size=(1 << 64) - max(n["offset"], 1)), ECORRUPT),
    "own_offset": (lambda n: encode(n, offset=n["offset"] + 1,
                                    kids=[(r, o + 1) for r, o in n["kids"]]), ECORRUPT),
    "own_size": (lambda n: encode(n, size=n["size"] + 1), ECORRUPT),
}


def three_level(seed: int):
    """A Tree of three levels (Root, 3 middle nodes, 9 leaf nodes of 3 leaves) with its leaf
    store: every node has the two children the families need."""
    leaves, lstore = leaf_blobs(seed, [5 + (7 * i) % 23 for i in range(27)])
    t = Tree(leaves, 3)
    assert [len(lv) for lv in t.nodes] == [1, 3, 9]
    return t, lstore


def two_streams(seed: int = 1):
    """Two three_level trees (the second over other leaves): (trees, store) with the store in
    insertion order leaves, then nodes."""
    a, sa = three_level(seed)
    b, sb = three_level(seed + 50)
    store = {**sa, **sb, **a.store(), **b.store()}
    return [a, b], store


WHERE = {"root": (0, 0), "middle": (1, 1), "leaf": (2, 4)}


def mutated(name: str, where: str, stream: int, seed: int = 1):
    """(pool, blobs, roots, predicted status of `stream`): two_streams with family `name` applied
    to the Root, a middle node or a leaf node of `stream`."""
    trees, store = two_streams(seed)
    d, i = WHERE[where]
    n = trees[stream].nodes[d][i]
    fn, want = FAMILIES[name]
    store[n["ref"]] = fn(n)
    pool, blobs = pool_of(store)
    return pool, blobs, [t.root for t in trees], want


def chain(depth: int):
    """One stream whose Root has a single `nodes` child, and so on, down to a leaf node at
    `depth` (Root = 0) over one 9-byte leaf: (pool, blobs, roots)."""
    leaf = b"nine byte"
    store = {sha(leaf): leaf}
    b = O.proto_node([], [(sha(leaf), 0)], 0, len(leaf))
    store[sha(b)] = b
    for _ in range(depth):
        b = O.proto_node([(sha(b), 0)], [], 0, len(leaf))
        store[sha(b)] = b
    pool, blobs = pool_of(store)
    return pool, blobs, [sha(b)]


def mixed_depth(seed: int = 3):
    """A Root whose first child is a leaf node and whose second is a node with two leaf nodes
    under it: (pool, blobs, roots, the leaves' bytes in stream order)."""
    leaves, lstore = leaf_blobs(seed, [11, 3, 40, 7, 19, 64, 1])
    a = Tree(leaves[:3], 3)              # one leaf node over [0, 54)
    o = a.size
    kids, nodes = [], []
    for grp in (leaves[3:5], leaves[5:]):
        ks, o0 = [], o
        for ref, ln in grp:
            ks.append((ref, o))
            o += ln
        nodes.append(Tree._node(2, ks, o0, o - o0))
    mid = Tree._node(1, [(n["ref"], n["offset"]) for n in nodes], a.size, o - a.size)
    root = Tree._node(1, [(a.root, 0), (mid["ref"], a.size)], 0, o)
    store = dict(lstore)
    for n in [a.nodes[0][0]] + nodes + [mid, root]:
        store[n["ref"]] = n["bytes"]
    pool, blobs = pool_of(store)
    return pool, blobs, [root["ref"]], [lstore[r] for r, _ in leaves]


# ---- stride changes inside one node --------------------------------------------------------------
def varint_len(v: int) -> int:
    return len(O._varint(v))


def stride_lanes(lens):
    """For a leaf node over leaves of `lens`: [(child index, lane)] of every change of entry
    length, lane being the child's distance from the previous change modulo 64 (the place in a
    64-entry group that starts where the stride last changed)."""
    out, start, prev, o = [], 0, None, 0
    for i, n in enumerate(lens):
        e = 36 if o == 0 else 37 + varint_len(o)
        if prev is not None and e != prev:
            out.append((i, (i - start) % 64))
            start = i
        prev = e
        o += n
    return out


def crossing_lens(thresholds, bmax: int, lane: int, tail: int, gmax: int = 1 << 14):
    """Leaf lengths (each at most bmax) of one leaf node whose children's offsets reach every
    threshold exactly, so that the entry length changes there, each change `lane` entries (modulo
    64) after the one before; then `tail` more leaves of bmax bytes. A stretch is as many bmax
    leaves as fit, one leaf for the rest and 1-byte leaves to make up the count, fewer than gmax
    entries in all."""
    lens, at = [1], 1  # child 0 at offset 0 (36 bytes), child 1 at offset 1: the first change
    for t in thresholds:
        d = t - at
        for g in range(1, gmax):
            k = min((d - 1) // bmax, g - 1)
            rest = d - k * bmax - (g - k - 1)  # what the one odd leaf must hold
            if g % 64 == lane and (g == k and rest == 0 or g > k and 1 <= rest <= bmax):
                lens += [bmax] * k + ([rest] + [1] * (g - k - 1) if g > k else [])
                break
        else:
            raise AssertionError((t, bmax, lane))
        at = t
    return lens + [bmax] * tail


def stride_node(lens, pool_off: int, first: int = 0):
    """One stream: a leaf node over len(lens) leaves that all lie at pool_off (a leaf of n bytes
    is the blob (pool_off, n), labelled by n alone, so the pool stays small and is never read).
    Returns (node bytes, root ref, leaf table entries)."""
    labels = {n: sha(b"leaf of %d" % n) for n in set(lens)}
    kids, o = [], first
    for n in lens:
        kids.append((labels[n], o))
        o += n
    b = O.proto_node([], kids, first, o - first)
    return b, sha(b), [(pool_off, n, r) for n, r in sorted(labels.items())]


# ---- entries of 45 to 47 bytes: offsets up to 2^64 - 1 -------------------------------------------
# An accepted walk cannot reach them all (a leaf is at most the pool, so offsets of 2^56 and more
# need 2^26 leaves of 1 GiB); a mark holds no child to a cover, so there a tiny pool can.
THRESHOLDS = [1 << (7 * j) for j in range(10)]  # the offsets at which an entry grows by a byte
ENTRY_LENS = [36] + list(range(38, 48))
COMMON_LEAF = b"the common leaf"


def entry_len(off: int) -> int:
    return 36 if off == 0 else 37 + varint_len(off)


def offset_lanes(offsets):
    """stride_lanes for a node given by its children's offsets."""
    out, start, prev = [], 0, None
    for i, o in enumerate(offsets):
        e = entry_len(o)
        if prev is not None and e != prev:
            out.append((i, (i - start) % 64))
            start = i
        prev = e
    return out


def all_lengths_offsets(lane: int, tail: int = 2):
    """Ascending child offsets of a node with all eleven entry lengths (36, 38 .. 47): child 0 at
    0, then for every threshold t = 2^(7j) a run from t on that ends at the next threshold - 1
    (the last one at 2^64 - 2), so both sides of every varint edge are present. Every run but the
    last holds `lane` entries modulo 64 (at least two), so every change of the entry length after
    the first (child 1, lane 1) lies on `lane` of its 64-entry group; the last run holds `tail`."""
    assert 0 <= lane < 64 and tail >= 2
    g = lane if lane >= 2 else lane + 64
    offs = [0]
    for j, t in enumerate(THRESHOLDS):
        n = g if j < 9 else tail
        end = THRESHOLDS[j + 1] - 1 if j < 9 else (1 << 64) - 2
        offs += [t + i for i in range(n - 1)] + [end]
    return offs


def only_leaf(elen: int) -> bytes:
    """The leaf blob that offsets_node's entries of elen bytes (45, 46 or 47) alone name."""
    return b"named by entries of %d bytes alone" % elen


def offsets_node(offsets, size: int = 1):
    """A leaf node over children at `offsets` (its own offset: the first child's), in Tree._node's
    form. Every child names COMMON_LEAF, but the last entry of each run of 45, 46 and 47 bytes
    names only_leaf(its length), so that leaf is live only if that very entry was read."""
    kids = []
    for i, o in enumerate(offsets):
        e = entry_len(o)
        last = i + 1 == len(offsets) or entry_len(offsets[i + 1]) != e
        kids.append((sha(only_leaf(e)) if e >= 45 and last else sha(COMMON_LEAF), o))
    return Tree._node(2, kids, offsets[0], size)


def wide_leaves() -> dict:
    """{ref: bytes} of the leaves offsets_node names."""
    return {sha(b): b for b in [COMMON_LEAF] + [only_leaf(e) for e in (45, 46, 47)]}


def edge_nodes():
    """The accepted nodes of the offsets' upper edge: all_lengths_offsets on lanes 0, 32 and 63
    with size 1 (`20 01`); one child at offset 0 with size 2^64 - 1 (a 10-byte varint whose last
    byte is 1); and a node at its own offset 2^63 (an `18` field of 10 bytes) with size 2^63 - 1,
    so that offset + size is 2^64 - 1."""
    out = [offsets_node(all_lengths_offsets(lane)) for lane in (0, 32, 63)]
    out.append(offsets_node([0], size=(1 << 64) - 1))
    out.append(offsets_node([(1 << 63) + i for i in range(3)], size=(1 << 63) - 1))
    return out


def _entries(n):
    return [b"\x12" + O._varint(len(c)) + c for c in (O.proto_child(r, o) for r, o in n["kids"])]


def _respliced(n, k: int, new: bytes, insert: bool = False) -> bytes:
    e = _entries(n)
    assert len(e[k]) == 47
    e[k:k + (0 if insert else 1)] = [new]
    tail = (b"\x18" + O._varint(n["offset"]) if n["offset"] else b"") + b"\x20" + \
        O._varint(n["size"])
    return b"".join(e) + tail


def _e47(n, k: int) -> bytes:
    return _entries(n)[k]


# name -> ((node, k) -> new bytes): entry k, one of 47 bytes, made a fault of the 10-byte varint's
# rules. Every one is ECORRUPT by the node's form alone. Only the mark's verdict shows it: the
# walk refuses these nodes for their covers anyway.
WIDE_FAMILIES = {
    # the tenth byte 2: an offset of 2^64 and more
    "ends_02": lambda n, k: _respliced(n, k, _e47(n, k)[:-1] + b"\x02"),
    # the tenth byte goes on, and an eleventh follows the entry's 47 bytes
    "continues": lambda n, k: _respliced(n, k, _e47(n, k)[:-1]
                                         + bytes([_e47(n, k)[-1] | 0x80, 0x01])),
    # the tenth byte 0: not minimal
    "ends_00": lambda n, k: _respliced(n, k, _e47(n, k)[:-1] + b"\x00"),
    # length byte 46, an entry of 48 bytes with a varint of eleven
    "len_byte_46": lambda n, k: _respliced(n, k, b"\x12\x2e" + _e47(n, k)[2:-1]
                                           + bytes([_e47(n, k)[-1] | 0x80, 0x01])),
    # an entry of 46 bytes after those of 47: the lengths fall, and so do the offsets
    "len_47_then_46": lambda n, k: _respliced(
        n, k, b"\x12" + O._varint(44) + O.proto_child(sha(COMMON_LEAF), (1 << 56) + k), True),
}
WIDE_LANES = (0, 5)


def _alone(last: int):
    """An entry of 47 bytes put in before entry k, its varint nine bytes of ff and then `last`:
    the low 64 bits of what it spells are 2^63 - 1 whether `last` is 2 or 0."""
    return lambda n, k: _respliced(n, k, b"\x12" + O._varint(45) + O.proto_child(
        sha(COMMON_LEAF), 1)[:-1] + b"\xff" * 9 + bytes([last]), True)


# ends_02 and ends_00 above sit in a run that starts at 2^63 after a child at 2^63 - 1, so a
# parser that kept the low 64 bits alone (0, or 5 on lane 5) would still refuse them, by the
# ascending rule. These two can be refused by the tenth byte's own rule alone: the child before
# is at 2^63 - 2, the low 64 bits of the entry are 2^63 - 1 and the next child is at 2^63, so the
# offsets ascend and the rest of the node is valid. Lane 0 only: a later lane's elder in a run of
# 47-byte entries is at 2^63 at least.
WIDE_ALONE = {"ends_02_alone": _alone(0x02), "ends_00_alone": _alone(0x00)}
WIDE_FAMILIES.update(WIDE_ALONE)


def wide_target(name: str, lane: int):
    """(node, k): all_lengths_offsets(0, 70)'s node and the entry the family `name` changes so
    that the fault lies on `lane` of a 64-entry group of 47-byte entries: the run's first entry
    (for the entry put in after the 47-byte ones: after 64 of them) or `lane` later. For the
    WIDE_ALONE families the node's child at 2^63 - 1 lies at 2^63 - 2 instead, and k is the first
    47-byte entry, which the new one goes before."""
    offs = all_lengths_offsets(0, 70)
    if name in WIDE_ALONE:
        assert lane == 0
        offs[offs.index((1 << 63) - 1)] -= 1
    n = offsets_node(offs)
    first = offset_lanes([o for _, o in n["kids"]])[-1][0]
    return n, first + lane + (64 if name == "len_47_then_46" and lane == 0 else 0)


def wide_mutated(name: str, lane: int, seed: int = 1):
    """(pool, blobs, roots, the changed blob's index): a three_level tree as Root 0 and, as Root
    1, wide_target's node with the family applied (or, for "wrap_2_63", the node at offset 2^63
    with size 2^63), under its unchanged label."""
    t, lstore = three_level(seed)
    store = {**lstore, **t.store(), **wide_leaves()}
    if name == "wrap_2_63":
        n = offsets_node([(1 << 63) + i for i in range(3)], size=(1 << 63) - 1)
        bad = encode(n, tags=[0x12] * 3, size=1 << 63)
    else:
        n, k = wide_target(name, lane)
        bad = WIDE_FAMILIES[name](n, k)
    assert n["ref"] not in store and bad != n["bytes"]
    store[n["ref"]] = bad
    pool, blobs = pool_of(store)
    return pool, blobs, [t.root, n["ref"]], len(store) - 1


WIDE_CASES = [(name, lane) for name in sorted(WIDE_FAMILIES) for lane in WIDE_LANES
              if lane == 0 or name not in WIDE_ALONE] + [("wrap_2_63", 0)]


# ---- more than one grid pass -------------------------------------------------------------------
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bs_amd", "csrc")


def grid_caps() -> dict:
    """What caps a launch of the walk's, the mark's, the restore's and the dedup's grid-stride
    kernels, read from the source: engine_grid's workgroups per CU (of 256 threads),
    launch_walk_count's (of 4 waves, a node each) and the prefix sum's tile."""
    out = {}

    def one(fn, pattern, name):
        with open(os.path.join(CSRC, fn)) as f:
            m = re.findall(pattern, f.read(), re.M)
        assert len(m) == 1, (name, m)
        out[name] = int(m[0])

    one("bsgpu_engine_common.inc",
        r"^\s*return grid_for\(items, 256, (\d+)u \* \(uint32_t\)num_cus\);", "grid_wgs_per_cu")
    one("bsgpu_walk.inc", r"cap = (\d+)ull \* \(uint32_t\)num_cus;", "count_wgs_per_cu")
    one("bsgpu_engine_common.inc", r"^constexpr\s+uint32_t\s+kSumTile\s*=\s*(\d+)\s*;", "kSumTile")
    return out


def grid_threads(cus: int) -> int:
    """T: the threads of one pass of an engine_grid launch; item T is a thread's second trip."""
    return grid_caps()["grid_wgs_per_cu"] * cus * 256


def count_waves(cus: int) -> int:
    """N: the waves of one pass of k_wk_count; node N is a wave's second trip."""
    return grid_caps()["count_wgs_per_cu"] * cus * 4


def many_streams(n3: int):
    """n3 streams that cycle three distinct three_level trees, with an empty stream (a zero Root)
    put in at place 7, a mixed_depth tree at place 11, and mixed_depth, empty, mixed_depth as the
    last three: (pool, blobs, roots, kinds, data), kinds[s] in 0, 1, 2, "m", "z" naming stream
    s's tree and data[kind] its bytes."""
    assert n3 >= 12
    trees, store, data = [], {}, {"z": b""}
    for j in range(3):
        t, lstore = three_level(20 + j)
        trees.append(t)
        store.update(lstore)
        store.update(t.store())
        data[j] = b"".join(lstore[r] for lv in t.nodes[2:] for n in lv for r, _ in n["kids"])
    mpool, mblobs, mroots, mleaves = mixed_depth()
    get = getter(mpool, mblobs)
    store.update({mblobs[k]["ref"].tobytes(): get(k) for k in range(len(mblobs))})
    data["m"] = b"".join(mleaves)
    kinds = [s % 3 for s in range(n3)]
    kinds.insert(7, "z")
    kinds.insert(11, "m")
    kinds += ["m", "z", "m"]
    assert len(kinds) <= 65535
    root = {0: trees[0].root, 1: trees[1].root, 2: trees[2].root, "m": mroots[0], "z": bytes(32)}
    pool, blobs = pool_of(store)
    return pool, blobs, [root[k] for k in kinds], kinds, data


# ---- the device against the model (tests/test_gpu_walk*.py) ------------------------------------
def roots_array(roots) -> np.ndarray:
    return np.frombuffer(b"".join(bytes(r) for r in roots), dtype=np.uint8).reshape(-1, 32)


def check(gpu, eng, pbuf, blob_bytes, blobs, roots, pool_bytes, expect=None, flags=0):
    """One bsg_engine_walk held to the model: the return code, every stream's status, the info
    and, on success, the records, sizes and counts (else: nothing published). pbuf: the pool on
    the device; blob_bytes(k): its node blobs' bytes on the host. Returns the model's tuple."""
    want = model(blob_bytes, blobs, roots, pool_bytes, flags)
    rc, info, status = eng.walk(pbuf.ptr, blobs, roots_array(roots), pool_bytes=pool_bytes,
                                flags=flags)
    assert rc == want[0], (rc, want[0], info, want[2])
    if expect is not None:
        assert rc == expect, (rc, expect)
    assert info == want[2], (info, want[2])
    if want[1] is not None:
        assert status.tolist() == want[1].tolist()
    if rc == OK:
        recs, sizes, counts = eng.copy_walk()
        assert recs.tobytes() == want[3].tobytes()
        assert sizes.tolist() == want[4].tolist() and counts.tolist() == want[5].tolist()
        assert eng.walk_records_device() != 0
    else:
        assert gpu.lib().bsg_engine_copy_walk(eng.h, None, 0, None, None, 0) == ESTATE
        assert eng.walk_records_device() == 0
    return want


def check_host_pool(gpu, eng, pool, blobs, roots, expect=None, pool_bytes=None, flags=0):
    """check() for a pool given as host bytes (uploaded for the call)."""
    pbuf = gpu.DeviceBuffer(max(len(pool), 16))
    try:
        pbuf.from_host(pool)
        return check(gpu, eng, pbuf, getter(pool, blobs), blobs, roots,
                     len(pool) if pool_bytes is None else pool_bytes, expect, flags)
    finally:
        pbuf.free()


def out_layout(sizes, gap=48):
    """16-aligned output offsets for streams of `sizes` with `gap` spare bytes between them."""
    off, o = [], 16
    for n in sizes:
        off.append(o)
        o = ((o + int(n) + 15) & ~15) + gap
    return off, o


def restore_walk(gpu, eng, pbuf, pool_bytes, blobs, sizes, verify=False):
    """bsg_engine_restore_walk into a FILL-ed buffer with GUARD bytes at both ends, which must
    stay; returns (rc, info, out_off, the out_cap bytes at d_out)."""
    off, cap = out_layout(sizes)
    obuf = gpu.DeviceBuffer(GUARD + cap + GUARD)
    try:
        obuf.from_host(np.full(obuf.nbytes, FILL, dtype=np.uint8))
        rc, info = eng.restore_walk(pbuf.ptr, blobs, obuf.ptr + GUARD, off, verify=verify,
                                    pool_bytes=pool_bytes, out_cap=cap)
        got = obuf.to_host()
    finally:
        obuf.free()
    assert (got[:GUARD] == FILL).all() and (got[GUARD + cap:] == FILL).all(), "guards"
    return rc, info, off, got[GUARD:GUARD + cap]

"""Inputs and the model for bsg_engine_gc_mark / bsg_engine_copy_gc / bsg_engine_gc_compact.

The model is plain Python with the rules of include/bsgpu.h: `protect` is gc.Protect with
split.Protect, literally recursive over a {ref: bytes} view of the pool (the smallest index per
ref); `mark` is the same reachability breadth first, which is what gives a node its depth, with
the walk's per-node parser (walk_cases.parse_node), the verdicts and the totals; `layout` and
`compacted` are the new offsets, the table and the swept pool. tests/test_gc_cases_cpu.py holds
the model to walk_cases.model; tests/test_gpu_gc*.py hold the device to it."""
from __future__ import annotations

import numpy as np

import walk_cases as W
from bs_amd.bsgpu import GC_MISSING_LEAVES, POOL_BLOB_DTYPE, WALK_MAX_DEPTH
from oracle import oracle as O

OK, EINVAL, ENOTFOUND, ECORRUPT, ESTATE = W.OK, W.EINVAL, W.ENOTFOUND, W.ECORRUPT, W.ESTATE
NONE = W.NONE
FILL, GUARD = 0x5A, 256
_RANK = {0: OK, 1: ECORRUPT, 2: ENOTFOUND}


# ---- the model ---------------------------------------------------------------------------------
def index_of(blobs) -> dict:
    """ref -> the smallest blob index that carries it."""
    raw = np.ascontiguousarray(blobs["ref"]).tobytes()
    index = {}
    for k in range(len(blobs)):
        index.setdefault(raw[32 * k:32 * k + 32], k)
    return index


def protect(view: dict, roots) -> set:
    """gc.Protect (gc/gc.go) with split.Protect (split/split.go) as its traversal, recursive over
    view = {ref: bytes}: the refs kept. gc.Protect returns at once for a ref it already keeps; here
    that check is on the refs already expanded, so that a blob first kept as somebody's leaf and
    later named under `nodes` is still expanded (include/bsgpu.h: a blob named both ways is
    expanded). A kept blob that is no well-formed node has no children."""
    keep, expanded = set(), set()

    def rec(ref):
        if ref not in view or ref in expanded:
            return
        keep.add(ref)
        expanded.add(ref)
        nd = W.parse_node(view[ref])
        if nd is None:
            return
        for child, _ in nd[1]:
            if nd[0] == 1:
                rec(child)
            elif child in view:
                keep.add(child)

    for r in roots:
        if bytes(r) != bytes(32):
            rec(bytes(r))
    return keep


def mark(blob_bytes, blobs, roots, pool_bytes, flags=0):
    """(rc, status, info, live) of bsg_engine_gc_mark. blob_bytes(k): the bytes of pool blob k
    (asked for expanded blobs only). status is None for a layout fault; live (uint8 per blob) is
    None unless rc is OK."""
    nr = len(roots)
    info = {"bad_root": NONE, "bad_blob": NONE, "nlive": 0, "live_bytes": 0, "ndead": 0,
            "dead_bytes": 0, "nnodes": 0, "missing_leaves": 0, "depth": 0}
    if flags & ~GC_MISSING_LEAVES or nr >= 1 << 32 or \
            any(o + n > pool_bytes for o, n in zip(blobs["off"].tolist(), blobs["len"].tolist())):
        return EINVAL, None, info, None
    index = index_of(blobs)
    live, claimed, failed, missing = set(), set(), set(), set()
    rank, rblob, frontier = [0] * nr, [None] * nr, []
    bad_form, bad_miss, verdict = [], [], 0
    for r, ref in enumerate(roots):
        if bytes(ref) == bytes(32):
            continue
        k = index.get(bytes(ref))
        if k is None:
            rank[r], verdict = 2, 2
            continue
        rblob[r] = k
        live.add(k)
        if k not in claimed:
            claimed.add(k)
            frontier.append(k)
    depth = 0
    while frontier:
        nxt = []
        for k in frontier:
            info["nnodes"] += 1
            info["depth"] = max(info["depth"], depth)
            nd = W.parse_node(blob_bytes(k))
            if nd is None:
                failed.add(k)
                bad_form.append(k)
                verdict = max(verdict, 1)
                continue
            for ref, _ in nd[1]:
                if nd[0] == 1 and depth == WALK_MAX_DEPTH:
                    bad_form.append(k)
                    verdict = max(verdict, 1)
                    continue
                c = index.get(ref)
                if c is not None:
                    live.add(c)
                    if nd[0] == 1 and c not in claimed:
                        claimed.add(c)
                        nxt.append(c)
                elif nd[0] == 2 and flags & GC_MISSING_LEAVES:
                    missing.add(ref)
                else:
                    bad_miss.append(k)
                    verdict = 2
        frontier = nxt
        depth += 1
    for r in range(nr):
        if rblob[r] in failed:
            rank[r] = max(rank[r], 1)
    status = np.array([_RANK[x] for x in rank], dtype=np.int32)
    bad = [r for r in range(nr) if rank[r]]
    info["bad_root"] = bad[0] if bad else NONE
    info["bad_blob"] = min(bad_form) if bad_form else min(bad_miss) if bad_miss else NONE
    if verdict:
        return _RANK[verdict], status, info, None
    lv = np.zeros(len(blobs), dtype=np.uint8)
    lv[sorted(live)] = 1
    lens = blobs["len"].astype(np.uint64)
    info["nlive"], info["ndead"] = len(live), len(blobs) - len(live)
    info["live_bytes"] = int(lens[lv == 1].sum())
    info["dead_bytes"] = int(lens[lv == 0].sum())
    info["missing_leaves"] = len(missing)
    return OK, status, info, lv


def layout(blobs, live, align16: bool):
    """(table of the live blobs at their new offsets, out_bytes)."""
    ent, o, end = [], 0, 0
    for k in np.flatnonzero(live):
        n = int(blobs[k]["len"])
        ent.append((o, n, blobs[k]["ref"].tobytes()))
        end = o + n
        o += (n + 15) & ~15 if align16 else n
    return W.table_of(ent), end


def compacted(pool, blobs, live, align16: bool) -> np.ndarray:
    """The swept pool's out_bytes bytes: every live blob at its new offset, padding zero."""
    table, end = layout(blobs, live, align16)
    out = np.zeros(end, dtype=np.uint8)
    for t, k in zip(table, np.flatnonzero(live)):
        o, n, so = int(t["off"]), int(t["len"]), int(blobs[k]["off"])
        out[o:o + n] = pool[so:so + n]
    return out


def run_model(pool, blobs, roots, pool_bytes=None, flags=0):
    return mark(W.getter(pool, blobs), blobs, roots,
                len(pool) if pool_bytes is None else pool_bytes, flags)


# ---- case builders -----------------------------------------------------------------------------
def node(nodes=(), leaves=(), offset=0, size=1) -> bytes:
    return O.proto_node(list(nodes), list(leaves), offset, size)


def pool_from(entries, first: int = 1):
    """A pool from (ref, bytes) pairs in order (refs may repeat): blobs packed tight from byte
    `first`, so they start at odd and even addresses alike. (pool bytes, table)."""
    ent, parts, o = [], [bytes(first)], first
    for ref, b in entries:
        ent.append((o, len(b), ref))
        parts.append(bytes(b))
        o += len(b)
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), W.table_of(ent)


def shared_subtree(seed: int = 5):
    """Two Roots over the same two middle nodes plus one of their own each: (pool, blobs, roots,
    distinct node blobs)."""
    leaves, lstore = W.leaf_blobs(seed, [7 + (5 * i) % 19 for i in range(36)])
    t = [W.Tree(leaves[9 * i:9 * i + 9], 3) for i in range(4)]  # Root over 3 leaf nodes each
    tops = []
    for own in (2, 3):
        kids, o = [], 0
        for x in (t[0], t[1], t[own]):
            kids.append((x.root, o))
            o += x.size
        tops.append(W.Tree._node(1, kids, 0, o))
    store = dict(lstore)
    for x in t:
        store.update(x.store())
    for n in tops:
        store[n["ref"]] = n["bytes"]
    pool, blobs = W.pool_of(store)
    return pool, blobs, [n["ref"] for n in tops], 2 + 4 * 4


def same_child_level(width: int = 64):
    """A Root over `width` middle nodes, each with `width` `nodes` entries that all name one leaf
    node: width * width frontier entries for one blob. (pool, blobs, roots)."""
    leaf = b"the one leaf"
    ln = node(leaves=[(W.sha(leaf), 0)], size=len(leaf))
    ent = [(W.sha(leaf), leaf), (W.sha(ln), ln)]
    mids = []
    for m in range(width):
        b = node(nodes=[(W.sha(ln), 1000 * m + j) for j in range(width)], offset=1000 * m,
                 size=1000)
        mids.append((W.sha(b), 1000 * m))
        ent.append((W.sha(b), b))
    root = node(nodes=mids, size=1000 * width)
    ent.append((W.sha(root), root))
    pool, blobs = pool_from(ent)
    return pool, blobs, [W.sha(root)]


def wide(n: int = 2049):
    """A Root with n `nodes` children, each a leaf node over the same leaf: a node wider than the
    prefix sum's tile, and a level of n nodes. (pool, blobs, roots)."""
    leaf = b"0123456789"
    ent, kids = [(W.sha(leaf), leaf)], []
    for i in range(n):
        b = node(leaves=[(W.sha(leaf), 10 * i)], offset=10 * i, size=10)
        kids.append((W.sha(b), 10 * i))
        ent.append((W.sha(b), b))
    root = node(nodes=kids, size=10 * n)
    ent.append((W.sha(root), root))
    pool, blobs = pool_from(ent)
    return pool, blobs, [W.sha(root)]


def cycle():
    """Two node blobs whose labels name each other: (pool, blobs, roots)."""
    ra, rb = W.sha(b"label a"), W.sha(b"label b")
    pool, blobs = pool_from([(ra, node(nodes=[(rb, 0)], size=5)),
                             (rb, node(nodes=[(ra, 0)], size=5))])
    return pool, blobs, [ra]


def both_ways():
    """A leaf node X named under `leaves` by the first Root and under `nodes` by the second:
    (pool, blobs, roots, X's leaf's blob index)."""
    leaf = b"below x"
    x = node(leaves=[(W.sha(leaf), 0)], size=len(leaf))
    a = node(leaves=[(W.sha(x), 0)], size=len(x))
    b = node(nodes=[(W.sha(x), 0)], size=len(leaf))
    pool, blobs = pool_from([(W.sha(leaf), leaf), (W.sha(x), x), (W.sha(a), a), (W.sha(b), b)])
    return pool, blobs, [W.sha(a), W.sha(b)], 0


def sized_pool(nblobs: int, seed: int = 9):
    """A pool of exactly nblobs blobs: one leaf node over half of them, the others dead filler in
    between. (pool, blobs, roots, flags): a pool of one blob is a leaf node whose leaf is missing."""
    if nblobs == 1:
        b = node(leaves=[(W.sha(b"gone"), 0)], size=4)
        pool, blobs = pool_from([(W.sha(b), b)])
        return pool, blobs, [W.sha(b)], GC_MISSING_LEAVES
    nl = nblobs // 2
    fillers = nblobs - nl - 1
    data = [b"leaf %d " % i + bytes((seed + 3 * i) % 40) for i in range(nl)]  # (all distinct)
    leaves, lstore = [(W.sha(d), len(d)) for d in data], {W.sha(d): d for d in data}
    t = W.Tree(leaves, arity=nl)
    ent = []
    for i, (ref, _) in enumerate(leaves):
        ent.append((ref, lstore[ref]))
        if i < fillers:
            d = b"dead %d " % i + bytes(i % 29)
            ent.append((W.sha(d), d))
    ent.insert(len(ent) // 2, (t.root, t.nodes[0][0]["bytes"]))
    assert len(ent) == nblobs
    pool, blobs = pool_from(ent)
    return pool, blobs, [t.root], 0


def len_mix(pattern: str, seed: int = 11):
    """Blobs of lens 0, 1, 15, 16, 17 and 4,097 (twice over) at odd pool offsets under one leaf
    node; pattern: one character per blob and round, 'L' live or 'D' dead. (pool, blobs, roots)."""
    lens = [0, 1, 15, 16, 17, 4097] * 2
    rng = np.random.default_rng(seed)
    data = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    refs = [W.sha(b"blob %d" % i) for i in range(len(lens))]  # labels (two blobs are empty)
    offs = np.cumsum([0] + [max(n, 1) for n in lens]).tolist()
    keep = [(refs[i], offs[i]) for i in range(len(lens)) if pattern[i % len(pattern)] == "L"]
    ent = list(zip(refs, data))
    roots = []
    if keep:
        ln = node(leaves=keep, offset=keep[0][1], size=1 << 20)
        ent.insert(3, (W.sha(ln), ln))
        roots = [W.sha(ln)]
    pool, blobs = pool_from(ent, first=3)
    return pool, blobs, roots


def edge_pool(drop=()):
    """walk_cases.edge_nodes as five Roots of one tiny pool, offsets up to 2^64 - 2 and every
    entry length in it: (pool, blobs, roots). The leaves they name lie between the nodes, a blob
    nobody names among them; the leaves whose refs are in `drop` are left out."""
    nodes = W.edge_nodes()
    dead = b"named by nobody"
    ent = [(r, b) for r, b in W.wide_leaves().items() if r not in drop] + [(W.sha(dead), dead)]
    for i, n in enumerate(nodes):
        ent.insert(2 * i, (n["ref"], n["bytes"]))
    pool, blobs = pool_from(ent)
    return pool, blobs, [n["ref"] for n in nodes]


def many_roots(nroots: int, malformed: bool = False):
    """nroots Roots over three three_level trees: all but the last two repeat the first tree's
    Root or are zero (every fifth), the last two name the second and the third tree, which are
    live through them alone. malformed: the third tree's Root blob is padded by a byte.
    (pool, blobs, roots, [the blob indices of tree j])."""
    assert nroots >= 3
    trees, store = [], {}
    for j in range(3):
        t, lstore = W.three_level(30 + j)
        trees.append(t)
        store.update(lstore)
        store.update(t.store())
    if malformed:
        n = trees[2].nodes[0][0]
        store[n["ref"]] = W.FAMILIES["padded"][0](n)
    pool, blobs = W.pool_of(store)
    index = index_of(blobs)
    own = [sorted({index[n["ref"]] for lv in t.nodes for n in lv}
                  | {index[r] for n in t.nodes[2] for r, _ in n["kids"]}) for t in trees]
    roots = [bytes(32) if r % 5 == 4 else trees[0].root for r in range(nroots - 2)]
    return pool, blobs, roots + [trees[1].root, trees[2].root], own


# ---- the device against the model (tests/test_gpu_gc*.py) --------------------------------------
def compact_once(gpu, eng, pbuf, pool_bytes, align16, want_bytes):
    """bsg_engine_gc_compact into a FILL-ed buffer with GUARD bytes at both ends: everything but
    the out_bytes bytes at d_out must stay, those must be want_bytes."""
    cap = len(want_bytes) + 64
    obuf = gpu.DeviceBuffer(GUARD + cap + GUARD)
    try:
        obuf.from_host(np.full(obuf.nbytes, FILL, dtype=np.uint8))
        rc, n = eng.gc_compact(pbuf.ptr, obuf.ptr + GUARD, align16=align16,
                               pool_bytes=pool_bytes, cap=len(want_bytes))
        got = obuf.to_host()
    finally:
        obuf.free()
    assert rc == OK and n == len(want_bytes), (rc, n, len(want_bytes))
    assert got[GUARD:GUARD + n].tobytes() == want_bytes.tobytes(), "compacted bytes"
    assert (got[:GUARD] == FILL).all() and (got[GUARD + n:] == FILL).all(), "bytes outside"


def check(gpu, eng, pbuf, pool, blobs, roots, pool_bytes=None, expect=None, flags=0):
    """One bsg_engine_gc_mark held to the model, bit for bit: the return code, every Root's
    status, the info and, on success, live, both tables and both compacted pools (else: nothing
    published). pbuf: the pool on the device; pool: the same bytes on the host. Returns the
    model's tuple."""
    pool_bytes = len(pool) if pool_bytes is None else pool_bytes
    want = mark(W.getter(pool, blobs), blobs, roots, pool_bytes, flags)
    rc, info, status = eng.gc_mark(pbuf.ptr, blobs, W.roots_array(roots), pool_bytes=pool_bytes,
                                   flags=flags)
    assert rc == want[0], (rc, want[0], info, want[2])
    if expect is not None:
        assert rc == expect, (rc, expect)
    assert info == want[2], (info, want[2])
    if want[1] is not None:
        assert status.tolist() == want[1].tolist()
    if rc != OK:
        assert gpu.lib().bsg_engine_copy_gc(eng.h, None, 0, None, 0, 0) == ESTATE
        assert eng.gc_compact(pbuf.ptr, pbuf.ptr, pool_bytes=pool_bytes, cap=0)[0] == ESTATE
        assert eng.gc_live_device() == 0
        return want
    assert eng.gc_live_device() != 0
    for al in (False, True):
        live, table = eng.copy_gc(align16=al)
        assert live.tobytes() == want[3].tobytes()
        wt, end = layout(blobs, want[3], al)
        assert table.tobytes() == wt.tobytes(), al
        compact_once(gpu, eng, pbuf, pool_bytes, al, compacted(pool, blobs, want[3], al))
    return want


def check_host_pool(gpu, eng, pool, blobs, roots, expect=None, pool_bytes=None, flags=0):
    """check() for a pool given as host bytes (uploaded for the call)."""
    pbuf = gpu.DeviceBuffer(max(len(pool), 16))
    try:
        pbuf.from_host(pool)
        return check(gpu, eng, pbuf, pool, blobs, roots, pool_bytes, expect, flags)
    finally:
        pbuf.free()

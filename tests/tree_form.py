"""split.Writer's tree in closed form, restated in Python from (ref, len, level) lists, and the
walk through py_tree_root's store it is compared with (shared by test_engine_trees_cpu.py and
test_gpu_engine_trees.py; no test in here).

closed_form() is the specification bsg_engine_trees follows ("Trees on the device"):
  q_i = level_i / fanout, Q = max q_i, then q_{n-1} = Q (TreeBuilder.Root folds every non-empty
  level: the last chunk closes every level below the top). A node of height L < Q closes after
  every chunk with q_i > L, the one node of height Q after the last chunk; a node covers the
  chunks after the previous close at its height up to its closing chunk. From the height-Q node,
  while the node has exactly one `nodes` child, move to that child: the node reached is the Root,
  and only it and the nodes below it are listed (stream-major, height, offset).
kernel_heights() is the same rule the way the kernels count it: Root height R = max q_i over every
chunk but the last, chunk i closes heights 0 .. q_i - 1 and the last chunk 0 .. R.
listing() is closed_form() once more, in numpy, for streams of any size (test_engine_trees_cpu.py
holds the two to each other); check_listing() and check_arena() compare an engine's node list and
arena with it."""
import hashlib

import numpy as np


def varint(v: int) -> bytes:
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def child(ref: bytes, offset: int, tag: int) -> bytes:
    c = b"\x0a\x20" + ref + (b"\x10" + varint(offset) if offset else b"")
    return bytes([tag]) + varint(len(c)) + c


def node_blob(nodes, leaves, offset: int, size: int) -> bytes:
    out = b"".join(child(r, o, 0x0A) for r, o in nodes)
    out += b"".join(child(r, o, 0x12) for r, o in leaves)
    if offset:
        out += b"\x18" + varint(offset)
    if size:
        out += b"\x20" + varint(size)
    return out


def closed_form(chunks, fanout: int):
    """chunks: [(ref, len, level)] of one stream. Returns (root, nodes): nodes in listed order,
    each a dict(height, offset, size, blob, ref, close) with close = its closing chunk.
    Linear in the nodes: the closes at height L are a subsequence of the closes at L - 1, so a
    row's children are taken from the row below with one pointer."""
    n = len(chunks)
    if n == 0:
        return bytes(32), []
    starts, o = [], 0
    for _, ln, _ in chunks:
        starts.append(o)
        o += ln
    ends = [s + c[1] for s, c in zip(starts, chunks)]
    q = [c[2] // fanout for c in chunks]
    Q = max(q)
    q[-1] = Q
    by_height = []
    closes = list(range(n))  # of the row below; height 0's children are the chunks themselves
    for L in range(Q + 1):
        below = by_height[L - 1] if L else None
        closes = [i for i in closes if q[i] > L] if L < Q else [n - 1]
        row, first, p = [], 0, 0
        for e in closes:
            off, size = starts[first], ends[e] - starts[first]
            if L == 0:
                kids, leaves = [], [(chunks[i][0], starts[i]) for i in range(first, e + 1)]
            else:
                p0 = p
                while p < len(below) and below[p]["close"] <= e:
                    p += 1
                kids, leaves = [(c["ref"], c["offset"]) for c in below[p0:p]], []
            blob = node_blob(kids, leaves, off, size)
            row.append(dict(height=L, offset=off, size=size, blob=blob, close=e,
                            ref=hashlib.sha256(blob).digest(), nkids=len(kids)))
            first = e + 1
        by_height.append(row)
    top = Q
    while by_height[top][0]["nkids"] == 1:  # the single-child prune
        top -= 1
    assert len(by_height[top]) == 1
    nodes = [nd for L in range(top + 1) for nd in by_height[L]]
    return nodes[-1]["ref"], nodes


def _closed_form_slow(chunks, fanout: int):
    """The first statement of closed_form (every node filters the whole row below it: quadratic),
    kept to compare the linear one with."""
    n = len(chunks)
    if n == 0:
        return bytes(32), []
    starts, o = [], 0
    for _, ln, _ in chunks:
        starts.append(o)
        o += ln
    ends = [s + c[1] for s, c in zip(starts, chunks)]
    q = [c[2] // fanout for c in chunks]
    Q = max(q)
    q[-1] = Q
    by_height = []
    for L in range(Q + 1):
        closes = [i for i in range(n) if q[i] > L] if L < Q else [n - 1]
        row, first = [], 0
        for e in closes:
            off, size = starts[first], ends[e] - starts[first]
            if L == 0:
                kids, leaves = [], [(chunks[i][0], starts[i]) for i in range(first, e + 1)]
            else:
                kids = [(c["ref"], c["offset"]) for c in by_height[L - 1]
                        if first <= c["close"] <= e]
                leaves = []
            blob = node_blob(kids, leaves, off, size)
            row.append(dict(height=L, offset=off, size=size, blob=blob, close=e,
                            ref=hashlib.sha256(blob).digest(), nkids=len(kids)))
            first = e + 1
        by_height.append(row)
    top = Q
    while by_height[top][0]["nkids"] == 1:  # the single-child prune
        top -= 1
    assert len(by_height[top]) == 1
    nodes = [nd for L in range(top + 1) for nd in by_height[L]]
    return nodes[-1]["ref"], nodes


def kernel_heights(levels, fanout: int):
    """(R, k): the Root height and the number of nodes each chunk closes, as the kernels count."""
    q = [lv // fanout for lv in levels]
    R = max(q[:-1], default=0)
    return R, q[:-1] + [R + 1]


def walk(O, store: dict, root: bytes):
    """Every node blob reachable from root in py_tree_root's store: {ref: (blob, height)}."""
    out = {}
    if root == bytes(32):
        return out

    def rec(ref):
        nodes, _leaves, _off, _size = O._unwrap(store, ref)
        h = 1 + max(rec(r) for r, _ in nodes) if nodes else 0
        out[ref] = (store[ref], h)
        return h
    rec(root)
    return out


# ---------------------------------------------------------------------------------------------
# The closed form in numpy: one pass per height, no Python loop over nodes but the SHA-256 calls
# ---------------------------------------------------------------------------------------------
def _vlen(v):
    v = np.asarray(v, dtype=np.uint64)
    n = np.ones(v.shape, dtype=np.int64)
    for k in range(1, 10):
        n += v >= np.uint64(1 << (7 * k))
    return n


def _put_varint(buf, pos, v):
    """varint(v[i]) at buf[pos[i] ...]."""
    v = np.asarray(v, dtype=np.uint64)
    vl = _vlen(v)
    for b in range(int(vl.max()) if len(vl) else 0):
        m = vl > b
        x = (v[m] >> np.uint64(7 * b)) & np.uint64(0x7F)
        buf[pos[m] + b] = (x | np.where(vl[m] > b + 1, 0x80, 0).astype(np.uint64)).astype(np.uint8)


def stream_heights(levels, fanout: int):
    """kernel_heights in numpy: (R, k) of one stream's levels (k empty for an empty stream)."""
    q = np.asarray(levels, dtype=np.int64) // fanout
    if len(q) == 0:
        return 0, q
    R = int(q[:-1].max()) if len(q) > 1 else 0
    k = q.copy()
    k[-1] = R + 1
    return R, k


def height_histogram(levels, fanout: int, heights: int):
    """Listed nodes of one stream per height 0 .. heights - 1."""
    R, k = stream_heights(levels, fanout)
    return np.array([int((k > h).sum()) for h in range(heights)], dtype=np.int64)


def _sha_each(buf, starts, lens):
    raw = buf.tobytes()
    return np.frombuffer(b"".join(hashlib.sha256(raw[a:a + b]).digest()
                                  for a, b in zip(starts.tolist(), lens.tolist())),
                         dtype=np.uint8).reshape(-1, 32)


def listing(refs, lens, levels, fanout: int, sha_many=None):
    """The listed nodes of one stream, in listed order, as arrays: dict(height, offset, size,
    close, blob_start, blob_len, ref [n, 32], buf) with node i's blob
    buf[blob_start[i] : blob_start[i] + blob_len[i]]. refs: [n, 32] uint8 chunk refs.
    sha_many(buf, starts, lens) -> [n, 32]: SHA-256 of many pieces of buf at once (hashlib one
    by one if None)."""
    n = len(lens)
    empty = np.zeros(0, dtype=np.int64)
    if n == 0:
        return dict(height=empty, offset=empty, size=empty, close=empty, blob_start=empty,
                    blob_len=empty, ref=np.zeros((0, 32), dtype=np.uint8),
                    buf=np.zeros(0, dtype=np.uint8))
    lens = np.asarray(lens, dtype=np.int64)
    ends = np.cumsum(lens)
    starts = ends - lens
    R, k = stream_heights(levels, fanout)
    c_ref = np.ascontiguousarray(refs, dtype=np.uint8).reshape(n, 32)
    c_off, c_close, tag = starts, np.arange(n, dtype=np.int64), 0x12
    rows, base = [], 0
    for h in range(R + 1):
        close = np.nonzero(k > h)[0]
        first = np.concatenate([[0], close[:-1] + 1])
        off, size = starts[first], ends[close] - starts[first]
        # every child of the row below belongs to a node here; node j takes those up to close[j]
        c1 = np.searchsorted(c_close, close, side="right")
        c0 = np.concatenate([[0], c1[:-1]])
        assert c1[-1] == len(c_close) and (c1 > c0).all()
        nc = c1 - c0
        el = 36 + np.where(c_off > 0, 1 + _vlen(c_off), 0)
        tl = np.where(off > 0, 1 + _vlen(off), 0) + np.where(size > 0, 1 + _vlen(size), 0)
        blen = np.add.reduceat(el, c0) + tl
        bstart = np.cumsum(blen) - blen
        pos = np.cumsum(el) - el + np.repeat(np.cumsum(tl) - tl, nc)
        buf = np.zeros(int(blen.sum()), dtype=np.uint8)
        buf[pos] = tag
        buf[pos + 1] = el - 2
        buf[pos + 2] = 0x0A
        buf[pos + 3] = 0x20
        buf[pos[:, None] + 4 + np.arange(32)[None, :]] = c_ref
        m = c_off > 0
        buf[pos[m] + 36] = 0x10
        _put_varint(buf, pos[m] + 37, c_off[m])
        t = bstart + blen - tl
        m = off > 0
        buf[t[m]] = 0x18
        _put_varint(buf, t[m] + 1, off[m])
        t = t + np.where(m, 1 + _vlen(off), 0)
        m = size > 0
        buf[t[m]] = 0x20
        _put_varint(buf, t[m] + 1, size[m])
        ref = (sha_many or _sha_each)(buf, bstart, blen)
        rows.append(dict(height=np.full(len(close), h, dtype=np.int64), offset=off, size=size,
                         close=close, blob_start=bstart + base, blob_len=blen, ref=ref, buf=buf))
        base += len(buf)
        c_ref, c_off, c_close, tag = ref, off, close, 0x0A
    return {f: np.concatenate([r[f] for r in rows]) for f in rows[0]}


def gather_blobs(arena, blob_off, blob_len):
    """The listed blobs' bytes, one after the other."""
    blob_off = np.asarray(blob_off, dtype=np.int64)
    blob_len = np.asarray(blob_len, dtype=np.int64)
    assert (blob_off >= 0).all() and (blob_off + blob_len <= len(arena)).all()
    start = np.cumsum(blob_len) - blob_len
    idx = np.repeat(blob_off - start, blob_len) + np.arange(int(blob_len.sum()), dtype=np.int64)
    return arena[idx]


def check_listing(recs, fanout: int, root: bytes, snodes, arena, sha_many=None):
    """One stream's listed nodes (snodes, TREE_NODE_DTYPE) against the closed form over its
    chunk records: the number of nodes, their order, height, blob length and blob bytes, the
    ref = sha256(blob) of every node, the Root last, blob_off 16-byte aligned and ascending.
    Returns the closed form (listing())."""
    want = listing(recs["ref"], recs["len"], recs["level"], fanout, sha_many)
    assert len(snodes) == len(want["height"]), (len(snodes), len(want["height"]))
    if len(snodes) == 0:
        assert root == bytes(32)
        return want
    assert (snodes["height"] == want["height"]).all()
    assert (snodes["blob_len"] == want["blob_len"]).all()
    off = snodes["blob_off"].astype(np.int64)
    assert (off % 16 == 0).all()
    assert (np.diff(off) > 0).all()
    got = gather_blobs(arena, off, snodes["blob_len"])
    assert got.tobytes() == want["buf"].tobytes()   # order: height, then stream offset
    # want["ref"] is sha256 of the closed form's blobs, which the listed blobs equal
    assert snodes["ref"].tobytes() == want["ref"].tobytes()
    assert snodes["ref"][-1].tobytes() == root == want["ref"][-1].tobytes()
    return want


def check_arena(nodes, arena):
    """arena_bytes is the sum of the blobs' 16-byte aligned lengths, no two blobs overlap, and
    every arena byte outside a listed blob is zero."""
    ln = nodes["blob_len"].astype(np.int64)
    assert len(arena) == int(((ln + 15) & ~15).sum()), (len(arena), int(((ln + 15) & ~15).sum()))
    if len(nodes) == 0:
        return
    off = nodes["blob_off"].astype(np.int64)
    assert (off + ln <= len(arena)).all()
    cover = np.bincount(off, minlength=len(arena) + 1) - \
        np.bincount(off + ln, minlength=len(arena) + 1)
    inside = np.cumsum(cover[:-1])
    assert inside.max() <= 1  # no byte in two blobs
    assert not arena[inside == 0].any()

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
chunk but the last, chunk i closes heights 0 .. q_i - 1 and the last chunk 0 .. R."""
import hashlib


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
    each a dict(height, offset, size, blob, ref, close) with close = its closing chunk."""
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

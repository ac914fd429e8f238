"""bsg_engine_trees without a GPU: the closed form the kernels follow (tests/tree_form.py) against
the oracle's literal TreeBuilder (py_tree_root), the node record's layout, and the null-argument
errors."""
import ctypes
import hashlib

import numpy as np
import pytest

import tree_form as TF

FANOUTS = (1, 2, 3, 8)


def _sequences(fanout: int, count: int):
    """Seeded (length, level) sequences: up to 200 chunks, levels up to 20, lengths that put
    offsets on both sides of the 1-, 2- and 3-byte varint edges."""
    rng = np.random.default_rng(1000 + fanout)
    for k in range(count):
        n = int(rng.integers(1, 201)) if k % 7 else int(rng.integers(1, 5))
        top = int(rng.integers(0, 21))
        # geometric levels (as trailing zeros are), capped, with a few forced high ones
        lv = np.minimum(rng.geometric(0.5, n) - 1, top)
        if k % 3 == 0:
            lv[rng.integers(0, n, max(1, n // 16))] = top
        if k % 4 == 1:
            lv[-1] = 20  # the last chunk alone reaches the top: the single-child prune
        ln = rng.integers(1, 120, n)
        if k % 5 == 0:
            ln[rng.integers(0, n, 2)] = rng.integers(16_000, 40_000, 2)
        yield [int(x) for x in ln], [int(x) for x in lv]


@pytest.mark.parametrize("fanout", FANOUTS)
def test_closed_form_matches_tree_builder(oracle, fanout):
    rng = np.random.default_rng(fanout)
    seen_prune = seen_deep = 0
    for lens, levels in _sequences(fanout, 150):
        data = [rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for ln in lens]
        store = {}
        root = oracle.py_tree_root(list(zip(data, levels)), fanout=fanout, store=store)
        want = TF.walk(oracle, store, root)
        chunks = [(hashlib.sha256(d).digest(), len(d), lv) for d, lv in zip(data, levels)]
        got_root, nodes = TF.closed_form(chunks, fanout)
        assert got_root == root
        assert {nd["ref"]: (nd["blob"], nd["height"]) for nd in nodes} == want
        assert len(nodes) == len(want)  # no blob listed twice
        # listed order: height ascending, then offset ascending; the Root last
        keys = [(nd["height"], nd["offset"]) for nd in nodes]
        assert keys == sorted(keys) and nodes[-1]["ref"] == root
        # the kernels' count of the same rule: Root height and closes per chunk
        R, k = TF.kernel_heights(levels, fanout)
        assert R == nodes[-1]["height"] and sum(k) == len(nodes)
        for h in range(R + 1):
            assert [i for i, ki in enumerate(k) if ki > h] == \
                [nd["close"] for nd in nodes if nd["height"] == h]
        seen_prune += max(lv // fanout for lv in levels) > R
        seen_deep += R >= 2
    # the prune and trees of three and more heights were exercised
    assert seen_prune >= 5 and seen_deep >= 5, (seen_prune, seen_deep)


def test_closed_form_empty_and_single():
    assert TF.closed_form([], 8) == (bytes(32), [])
    ref = hashlib.sha256(b"x" * 10).digest()
    root, nodes = TF.closed_form([(ref, 10, 5)], 1)  # its own level is pruned away
    assert len(nodes) == 1 and nodes[0]["height"] == 0
    assert nodes[0]["blob"] == b"\x12\x22\x0a\x20" + ref + b"\x20\x0a"  # one leaf, no offset
    assert root == hashlib.sha256(nodes[0]["blob"]).digest()


def test_tree_node_layout():
    from bs_amd import bsgpu

    class TreeNode(ctypes.Structure):
        _fields_ = [("blob_off", ctypes.c_uint64), ("blob_len", ctypes.c_uint32),
                    ("stream", ctypes.c_uint32), ("height", ctypes.c_uint32),
                    ("reserved", ctypes.c_uint32), ("ref", ctypes.c_uint8 * 32)]
    assert ctypes.sizeof(TreeNode) == 56
    assert bsgpu.TREE_NODE_DTYPE.itemsize == 56
    for name, _ in TreeNode._fields_:
        assert bsgpu.TREE_NODE_DTYPE.fields[name][1] == getattr(TreeNode, name).offset


def test_trees_null_arguments():
    from bs_amd import bsgpu
    L = bsgpu.lib()
    a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert L.bsg_engine_trees(None, ctypes.byref(a), ctypes.byref(b)) == -22
    buf = np.zeros(64, dtype=np.uint8)
    assert L.bsg_engine_copy_roots(None, buf.ctypes.data, None, 1) == -22
    assert L.bsg_engine_copy_tree_nodes(None, buf.ctypes.data, 1, buf.ctypes.data, 1) == -22
    assert not L.bsg_engine_tree_nodes_device(None)
    assert not L.bsg_engine_tree_arena_device(None)
    assert not L.bsg_engine_roots_device(None)

"""Inputs of the tree limit tests (test_engine_trees_cpu.py holds every one of them to its claim
with the oracle, test_gpu_tree_limits.py runs them; no test in here).

Every stream is planting.level_stream(): 64-byte windows back to back, which Bits / MinSize 64
cut into chunks of exactly the planned levels, so the node count of every height of a run is
chosen, not drawn: height h of a stream has #{i not last : level_i // fanout > h} nodes, plus one
while h <= R."""
import os
import re

import numpy as np

import planting as P
import tree_form as TF

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bs_amd", "csrc")
_LIMITS = {"kTreeHashBatch": "bsgpu_host.cpp", "kTreeWaveNodes": "bsgpu_host.cpp",
           "kTreeTile": "bsgpu_tree.inc", "kTreeMaxHeights": "bsgpu_internal.h"}


def limits() -> dict:
    """The four constants the tree code switches on, read from the source."""
    out = {}
    for name, fn in _LIMITS.items():
        with open(os.path.join(CSRC, fn)) as f:
            m = re.findall(r"^constexpr\s+uint(?:32|64)_t\s+%s\s*=\s*(\d+)\s*;" % name, f.read(),
                           re.M)
        assert len(m) == 1, (name, fn, m)
        out[name] = int(m[0])
    out["scan_items"] = 256 * out["kTreeTile"]  # k_sum_mid: 256 threads, one tile each
    return out


# ---------------------------------------------------------------------------------------------
# a. shape families: (k, d) stands for level k * fanout + d, on either side of a multiple
# ---------------------------------------------------------------------------------------------
FAMILY_BITS = 8
Z = (0, 0)
FAMILIES = [
    ("level0", [Z] * 7 + [(2, 0)]),                       # every non-last chunk level 0: R = 0
    ("highest_first", [(3, 0), (1, -1), (1, 0), (1, 1), (2, -1), Z, (2, 0), Z]),
    ("highest_last_zero", [Z, (1, -1), Z, (1, -1), Z, (3, 0)]),   # the others q = 0
    ("highest_middle", [(1, 0), Z, (2, -1), (3, 0), (1, 1), (2, 0), Z, (1, -1), Z]),
    ("highest_last_lower", [(1, 0), Z, (2, -1), Z, (1, 1), (3, 0)]),
    ("descending", [(3, 0), (3, -1), (2, 1), (2, 0), (2, -1), (1, 1), (1, 0), (1, -1), Z, Z]),
    ("ascending", [Z, (1, -1), (1, 0), (1, 1), (2, -1), (2, 0), (2, 1), (3, -1), (3, 0), Z]),
    ("equal_q", [(1, 0), (2, 0), (2, 0), (2, 1), Z, (3, 0), (3, 0), (1, 0), Z]),
    ("two_chunks", [(3, 0), Z]),
    ("one_chunk", [(2, 0)]),
]
# declared order: empty streams between the families, the tallest neither first nor last
FAMILY_ORDER = ["level0", None, "highest_first", None, "highest_last_zero", "highest_middle", None,
                None, "highest_last_lower", "descending", "ascending", None, "equal_q",
                "two_chunks", None, "one_chunk"]


def family_levels(fanout: int, order: str = "declared"):
    """[(name or None, levels)] of one family run; order: declared, descending (Root height) or
    shuffled."""
    fam = dict(FAMILIES)
    out = []
    for name in FAMILY_ORDER:
        lv = [max(0, k * fanout + d) for k, d in fam[name]] if name else []
        assert all(FAMILY_BITS + x <= 32 for x in lv)
        out.append((name, lv))
    if order == "descending":
        out.sort(key=lambda x: -(TF.stream_heights(x[1], fanout)[0] + (1 if x[1] else 0)))
    elif order == "shuffled":
        perm = np.random.default_rng(100 + fanout).permutation(len(out))
        out = [out[i] for i in perm]
    else:
        assert order == "declared"
    return out


def assert_family_properties(fams, fanout: int):
    """What a family run is there for, from the closed form alone: streams of different Root
    heights with a lower one before and after the tallest, the tallest neither first nor last,
    empty streams in between."""
    R = [TF.stream_heights(lv, fanout)[0] if lv else None for _, lv in fams]
    H = 1 + max(r for r in R if r is not None)
    assert H >= 3
    tall = [s for s, r in enumerate(R) if r == H - 1]
    assert 0 < tall[0] and tall[-1] < len(fams) - 1
    assert any(r is not None and r < H - 1 for r in R[:tall[0]])
    assert any(r is not None and r < H - 1 for r in R[tall[-1] + 1:])
    assert any(r is None for r in R)
    return H


# ---------------------------------------------------------------------------------------------
# b. exact thresholds
# ---------------------------------------------------------------------------------------------
THRESHOLD_BITS = 8
THRESHOLD_FANOUT = 2


def mixed_levels(seed, chunks: int, nodes0: int, upper=(0, 0), fanout: int = THRESHOLD_FANOUT):
    """Levels of one stream of `chunks` chunks with exactly nodes0 nodes of height 0: nodes0 - 1
    chunks other than the last have q >= 1, upper[0] of them q >= 2 and upper[1] of those q = 3,
    at seeded positions; the level within a q is seeded too."""
    assert 1 <= nodes0 <= chunks and upper[1] <= upper[0] <= nodes0 - 1
    rng = np.random.default_rng(seed)
    q = np.zeros(chunks, dtype=np.int64)
    a = rng.permutation(chunks - 1)[:nodes0 - 1]
    q[a] = 1
    q[a[:upper[0]]] = 2
    q[a[:upper[1]]] = 3
    lv = q * fanout + rng.integers(0, fanout, chunks)
    lv[-1] = rng.integers(0, 4 * fanout)
    return lv


def split_plan(total: int, parts):
    """`total` split by the fractions `parts` into positive integers."""
    out = [max(1, int(total * p)) for p in parts[:-1]]
    out.append(total - sum(out))
    assert out[-1] >= 1
    return out


def node_threshold_run(nodes0: int, seed: int, upper=(0, 0)):
    """Level lists of a run of three streams (the second empty) with nodes0 height-0 nodes in
    all, about 1.5 chunks per node; a limit below nodes0 falls inside the last stream."""
    n = split_plan(nodes0, (0.37, 0.63))
    u = [split_plan(x, (0.37, 0.63)) if x >= 2 else [0, x] for x in upper]
    return [mixed_levels([seed, 0], n[0] * 3 // 2 + 1, n[0], (u[0][0], u[1][0])),
            np.zeros(0, dtype=np.int64),
            mixed_levels([seed, 1], n[1] * 3 // 2 + 2, n[1], (u[0][1], u[1][1]))]


def chunk_threshold_run(chunks: int, seed: int, nodes0: int):
    """Level lists of a run of three streams (the second empty) with `chunks` chunks in all."""
    m = split_plan(chunks, (0.41, 0.59))
    n = split_plan(nodes0, (0.41, 0.59))
    return [mixed_levels([seed, 0], m[0], n[0], (n[0] // 8, n[0] // 16)),
            np.zeros(0, dtype=np.int64),
            mixed_levels([seed, 1], m[1], n[1], (n[1] // 8, n[1] // 16))]


def run_histogram(level_lists, fanout: int):
    """Listed nodes per height of a whole run, up to its tallest tree."""
    H = 1 + max((TF.stream_heights(lv, fanout)[0] for lv in level_lists if len(lv)), default=0)
    return sum(TF.height_histogram(lv, fanout, H) for lv in level_lists)


def streams_of(table, bits, level_lists):
    return [P.level_stream(table, bits, lv) if len(lv) else np.zeros(0, dtype=np.uint8)
            for lv in level_lists]


# ---------------------------------------------------------------------------------------------
# d. the tallest tree: every level Bits = 1 can give, 31 (a zero hash) first among them
# ---------------------------------------------------------------------------------------------
TALL_BITS = 1
TALL_LEVELS = [3, 31, 0, 30, 31, 31, 17, 0, 29, 1, 16, 15, 31, 2, 8, 30, 0, 7, 24, 23, 31, 0, 5,
               9, 31, 30, 4, 0, 12, 31, 6, 0]

"""bsg_engine_read past one pass of its grids, every comparison an equality.

A launch is capped at T = 8 x CUs x 256 threads (engine_grid), read from the source and the device.
One stream whose Root names T + 3 leaf nodes is read whole and over its middle third in one call:
the pruned emit has more than T children of one node, the placement more than T nodes in a level
and more than T followed leaves, the resolve more than T records, so every thread of each makes a
second trip, and the middle third's dead frontier entries lie on both sides of its live ones. Then
65,535 ranges of a few bytes each over two small streams: second trips of the per-range kernels
(the Roots, the tiling check's per-range pass). The expected bytes and counts are closed forms."""
import numpy as np
import pytest

import gc_cases as G
import read_cases as R
import walk_cases as W
from test_gpu_tier_counts import cus  # noqa: F401  (the device's CU count, a fixture)

pytestmark = pytest.mark.gpu
FILL, GUARD = W.FILL, W.GUARD


@pytest.fixture()
def eng(gpu):
    e = gpu.Engine()
    yield e
    e.close()


def _read(gpu, eng, pool, blobs, ranges, off, cap, flags=0):
    pbuf, obuf = gpu.DeviceBuffer(len(pool)), gpu.DeviceBuffer(GUARD + cap + GUARD)
    try:
        pbuf.from_host(pool)
        obuf.from_host(np.full(obuf.nbytes, FILL, dtype=np.uint8))
        res = eng.read(pbuf.ptr, blobs, ranges, obuf.ptr + GUARD, off, flags=flags,
                       pool_bytes=len(pool), out_cap=cap)
        return res + (obuf.to_host(),)
    finally:
        pbuf.free()
        obuf.free()


def test_a_node_wider_than_a_grid_pass(gpu, eng, cus):  # noqa: F811
    t = W.grid_threads(cus)
    n = t + 3
    pool, blobs, roots = G.wide(n)
    a, ln = 10 * (n // 3) + 4, 10 * (n // 3)
    m = (a + ln - 1) // 10 - a // 10 + 1       # the leaf nodes under the middle third
    assert m + n > t and 0 < a // 10 and (a + ln) // 10 < n - 1
    ranges = gpu.read_ranges([(roots[0], 0, 10 * n), (roots[0], a, ln)])
    off = [0, (10 * n + 15 & ~15) + 16]
    cap = off[1] + ln + 16
    rc, status, got, info, out = _read(gpu, eng, pool, blobs, ranges, off, cap)
    assert rc == R.OK and status.tolist() == [R.OK, R.OK] and got.tolist() == [10 * n, ln]
    assert info == {"bad_range": R.NONE, "bad_blob": R.NONE, "nnodes": 2 + n + m,
                    "nleaves": n + m, "bytes": 10 * n + ln, "verified": 0, "depth": 1}
    stream = np.frombuffer(b"0123456789" * n, dtype=np.uint8)
    exp = np.full(GUARD + cap + GUARD, FILL, dtype=np.uint8)
    exp[GUARD:GUARD + 10 * n] = stream
    exp[GUARD + off[1]:GUARD + off[1] + ln] = stream[a:a + ln]
    assert out.tobytes() == exp.tobytes()


def test_more_ranges_than_a_grid_pass(gpu, eng, cus):  # noqa: F811
    trees, store = W.two_streams()
    pool, blobs = W.pool_of(store)
    pool = np.concatenate([pool, np.zeros(256, np.uint8)])
    nr = 65535
    assert nr > 0 and W.grid_threads(cus) > 0
    whole = R.run_model(pool, blobs, [(x.root, 0, x.size) for x in trees])
    assert whole[0] == R.OK
    data = [np.frombuffer(d, dtype=np.uint8) for d in whole[4]]
    starts = []  # per stream: the node offsets of every depth, then the chunks'
    for x in trees:
        lv = [np.array([nd["offset"] for nd in lvl]) for lvl in x.nodes]
        lv.append(np.array([o for nd in x.nodes[-1] for _, o in nd["kids"]]))
        starts.append(lv)
    rng = np.random.default_rng(65535)
    which = rng.integers(0, 3, nr)              # 2: a zero Root
    at = rng.integers(0, trees[0].size + 6, nr)
    ln = rng.integers(0, 9, nr)
    rg = np.zeros(nr, dtype=gpu.READ_RANGE_DTYPE)
    rg["offset"], rg["len"] = at, ln
    for s, x in enumerate(trees):
        rg["root"][which == s] = np.frombuffer(x.root, dtype=np.uint8)
    off = 16 * np.arange(nr, dtype=np.uint64)
    cap = 16 * nr
    exp = np.full(GUARD + cap + GUARD, FILL, dtype=np.uint8)
    want_got = np.zeros(nr, dtype=np.uint64)
    nnodes = nleaves = 0
    for q in range(nr):
        s = int(which[q])
        if s == 2:
            continue
        a, size = int(at[q]), trees[s].size
        b = min(a + int(ln[q]), size)
        nnodes += 1
        if a >= b:
            continue
        want_got[q] = b - a
        exp[GUARD + 16 * q:GUARD + 16 * q + b - a] = data[s][a:b]
        under = [int(np.searchsorted(v, b, "left") - np.searchsorted(v, a, "right") + 1)
                 for v in starts[s]]
        nnodes += sum(under[1:-1])
        nleaves += under[-1]
    for flags in (0, R.VERIFY):
        rc, status, got, info, out = _read(gpu, eng, pool if flags == 0 else _aligned(store)[0],
                                           blobs if flags == 0 else _aligned(store)[1], rg, off,
                                           cap, flags)
        assert rc == R.OK and not status.any(), (rc, info)
        assert got.tolist() == want_got.tolist()
        assert (info["nnodes"], info["nleaves"], info["bytes"], info["depth"]) == \
            (nnodes, nleaves, int(want_got.sum()), 2)
        assert info["verified"] == (int(_aligned(store)[1]["len"].sum()) if flags else 0)
        assert out.tobytes() == exp.tobytes()


def _aligned(store):
    """The store's blobs at multiples of 16 with read slack after them: (pool, table)."""
    entries, parts, o = [], [], 0
    for ref, b in store.items():
        entries.append((o, len(b), ref))
        parts.append(bytes(b) + bytes(-len(b) % 16))
        o += len(parts[-1])
    return (np.frombuffer(b"".join(parts) + bytes(256), dtype=np.uint8).copy(),
            W.table_of(entries))

"""The model of bsg_engine_read (read_cases.py) held to the oracle's trees and to the walk's model,
without a GPU: every range's bytes are the stream's, a range of the whole stream visits what the
walk visits, a 1-byte range visits one node per level of its path, and the blobs the model did not
touch can be taken out of the pool without changing anything."""
import numpy as np
import pytest

import read_cases as R
import walk_cases as W

FANOUTS = (1, 2, 3, 8)
COUNTS = (1, 2, 3, 7, 50, 400)


def _ranges_of(root, size, cuts, rng):
    """Ranges that start and end at, just before and just after the cuts, and seeded ones."""
    pts = sorted({min(max(c + d, 0), size + 2) for c in cuts for d in (-1, 0, 1)} | {0, size})
    picks = [pts[i] for i in rng.choice(len(pts), min(len(pts), 12), replace=False)]
    out = [(root, a, b - a) for a in picks for b in picks if a <= b]
    out += [(root, int(a), int(n)) for a, n in zip(rng.integers(0, size + 3, 8),
                                                   rng.integers(0, size + 3, 8))]
    return out + [(root, 0, size), (root, 0, R.U64), (root, size - 1, R.U64), (root, R.U64, 5),
                  (root, size, 1), (root, 3, 0)]


@pytest.mark.parametrize("fanout", FANOUTS)
def test_bytes_are_the_streams(fanout):
    rng = np.random.default_rng(fanout)
    for n in COUNTS:
        data, chunks, root, store = W.oracle_tree(11, n, fanout)
        pool, blobs = W.pool_of(store)
        cuts, leaf_nodes, top, size = R.boundaries(W.getter(pool, blobs), blobs, root)
        assert size == len(data) and cuts == np.cumsum([0] + [len(c) for c, _ in chunks[:-1]]).tolist()
        ranges = _ranges_of(root, size, cuts[::max(1, len(cuts) // 6)] + leaf_nodes[:4] + top, rng)
        for rg in ranges:  # one by one, so the outputs need no room beside each other
            rc, status, got, info, out, touched = R.run_model(pool, blobs, [rg])
            _, off, ln = rg
            assert rc == R.OK and status.tolist() == [R.OK], (rg[1:], rc, info)
            assert out[0] == data[off:off + ln] and got == [len(out[0])], rg[1:]
            assert info["bytes"] == got[0] and info["bad_range"] == R.NONE


def test_empty_stream_and_no_ranges():
    pool, blobs = W.pool_of({})
    rc, status, got, info, out, touched = R.run_model(pool, blobs, [(bytes(32), 0, 10)])
    assert (rc, status.tolist(), got, out, touched) == (R.OK, [R.OK], [0], [b""], set())
    assert info == R.fresh_info()
    rc, status, got, info, out, touched = R.run_model(pool, blobs, [])
    assert (rc, got, out, info) == (R.OK, [], [], R.fresh_info())


@pytest.mark.parametrize("fanout", FANOUTS)
def test_whole_stream_is_the_walk(fanout):
    for n in COUNTS:
        data, chunks, root, store = W.oracle_tree(5, n, fanout)
        pool, blobs = W.pool_of(store)
        visited = []

        def seen(k, f=W.getter(pool, blobs)):
            visited.append(k)
            return f(k)

        wrc, _, winfo, recs, sizes, _ = W.model(seen, blobs, [root], len(pool))
        assert wrc == W.OK
        rc, status, got, info, out, touched = R.run_model(pool, blobs, [(root, 0, len(data))])
        assert rc == R.OK and out == [data]
        assert info["nnodes"] == winfo["nnodes"] and info["depth"] == winfo["depth"]
        assert info["nleaves"] == winfo["nrecs"] == len(chunks)
        index = {bytes(r): k for k, r in reversed(list(enumerate(blobs["ref"])))}
        leaves = {index[bytes(r)] for r in recs["ref"]}
        assert touched == set(visited) | leaves
        # ... and gives its records: the touched leaves in stream order are the walk's
        order = sorted(leaves, key=lambda k: min(int(r["offset"]) for r in recs
                                                 if index[bytes(r["ref"])] == k))
        assert [W.getter(pool, blobs)(k) for k in order] == \
            [c for c in dict.fromkeys(c for c, _ in chunks)]


@pytest.mark.parametrize("fanout", (2, 3, 8))
def test_one_byte_visits_one_node_per_level(fanout):
    from oracle import oracle as O
    data, chunks, root, store = W.oracle_tree(3, 400, fanout)
    pool, blobs = W.pool_of(store)
    for at in (0, 1, len(data) // 3, len(data) // 2, len(data) - 1):
        height, ref = 0, root  # the path's length, by the oracle's own unwrap
        while True:
            nodes, leaves, _, _ = O._unwrap(store, ref)
            height += 1
            if not nodes:
                break
            ref = [r for r, o in nodes if o <= at][-1]
        rc, status, got, info, out, touched = R.run_model(pool, blobs, [(root, at, 1)])
        assert rc == R.OK and out == [data[at:at + 1]]
        assert info["nnodes"] == height and info["depth"] == height - 1 and info["nleaves"] == 1
        assert len(touched) == height + 1


@pytest.mark.parametrize("fanout", (2, 3))
def test_untouched_blobs_may_go(fanout):
    data, chunks, root, store = W.oracle_tree(9, 400, fanout)
    pool, blobs = W.pool_of(store)
    rng = np.random.default_rng(fanout)
    for _ in range(6):
        off, ln = int(rng.integers(0, len(data))), int(rng.integers(1, 3000))
        for flags in (0,):
            full = R.run_model(pool, blobs, [(root, off, ln)], flags=flags)
            assert full[0] == R.OK and 0 < len(full[5]) < len(blobs)
            kept = sorted(full[5])
            few = blobs[kept]
            rc, status, got, info, out, touched = R.run_model(pool, few, [(root, off, ln)],
                                                              flags=flags)
            assert (rc, status.tolist(), got, info, out) == \
                (full[0], full[1].tolist(), full[2], full[3], full[4])
            assert touched == set(range(len(kept)))
            # and each of them is needed: without it the range is not found
            for gone in (0, len(kept) // 2, len(kept) - 1):
                rc, status, got, info, out, touched = R.run_model(
                    pool, np.delete(few, gone), [(root, off, ln)])
                assert rc == R.ENOTFOUND and status.tolist() == [R.ENOTFOUND] and got == [0]


def test_layout_rules():
    data, chunks, root, store = W.oracle_tree(2, 50, 3)
    pool, blobs = W.pool_of(store)
    ok = [(root, 0, 100), (root, 10, 100)]
    assert R.run_model(pool, blobs, ok, out_off=[0, 112], out_cap=212)[0] == R.OK
    for out_off, out_cap in (([0, 96], 300), ([0, 120], 300), ([0, 112], 211), ([0, 304], 300)):
        rc, status, got, info, out, touched = R.run_model(pool, blobs, ok, out_off=out_off,
                                                          out_cap=out_cap)
        assert rc == R.EINVAL and got == [0, 0] and info == R.fresh_info()
    # a len of 2^63 or more is held to the stream's size
    big = [(root, len(data) - 5, 1 << 63)]
    assert R.run_model(pool, blobs, big, out_off=[0], out_cap=5)[0] == R.OK
    assert R.run_model(pool, blobs, big, out_off=[0], out_cap=4)[0] == R.EINVAL
    assert R.run_model(pool, blobs, ok, flags=2)[0] == R.EINVAL
    # the tight pool is misaligned: only the flag minds
    rc, status, got, info, out, touched = R.run_model(pool, blobs, ok, flags=R.VERIFY)
    assert rc == R.EINVAL and status.tolist() == [R.OK, R.OK] and info["nleaves"] > 0


def test_verify_hashes_the_touched_alone():
    data, chunks, root, store = W.oracle_tree(4, 120, 3)
    refs = list(store)
    entries, parts, o = [], [], 0
    for ref in refs:  # an aligned pool
        b = store[ref]
        entries.append((o, len(b), ref))
        parts.append(b + bytes(-len(b) % 16))
        o += len(parts[-1])
    pool = np.frombuffer(b"".join(parts) + bytes(256), dtype=np.uint8).copy()
    blobs = W.table_of(entries)
    rg = [(root, len(data) // 2, 700)]
    rc, status, got, info, out, touched = R.run_model(pool, blobs, rg, flags=R.VERIFY)
    assert rc == R.OK and info["verified"] == sum(int(blobs[k]["len"]) for k in touched)
    assert 0 < info["verified"] < int(blobs["len"].sum())
    for k in range(len(blobs)):
        p = pool.copy()
        p[int(blobs[k]["off"])] ^= 1
        rc2, _, got2, info2, out2, _ = R.run_model(p, blobs, rg, flags=R.VERIFY)
        if k in touched and W.parse_node(W.getter(p, blobs)(k)) is None and \
                W.parse_node(W.getter(pool, blobs)(k)) is not None:
            assert rc2 in (R.ECORRUPT, R.ENOTFOUND)  # the structure gave way first
        elif k in touched:
            assert rc2 in (R.ECORRUPT, R.ENOTFOUND) and got2 == [0] and out2 is None
            if info2["bad_blob"] != R.NONE:
                assert info2["bad_blob"] == k
        else:
            assert (rc2, got2, info2, out2) == (rc, got, info, out)

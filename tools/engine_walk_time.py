"""Times bsg_engine_walk and bsg_engine_restore_walk in one process, with HIP events on the
engine stream (bsg_engine_profile), median of --reps after one warm-up:
  c1   the configs[1] shape (1 x 1 GiB, SplitMix) at the default parameters
  c2   the configs[2] shape (256 x 64 MiB)
  c4   configs[4] at full size: stream B = stream A (1 GiB) with 1,024 edits
Each shape is split, its trees built (bsg_engine_trees), deduplicated and packed; the pool is the
packed chunks with the tree arena's node blobs after them. The walk starts from the run's Roots
(walk_index_ms / walk_levels_ms / walk_placement_ms, beside trees_ms, the whole
bsg_engine_trees call of the same run) and its records are held to the run's; then the streams
are restored with the records handed in from the host (restore_ms = resolve + scatter) and with
bsg_engine_restore_walk (restore_walk_ms), and the restored bytes are split again once.

Usage: python tools/engine_walk_time.py [--reps 3] [--shapes c1,c2,c4]
Prints one JSON line per shape."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bs_amd import bsgpu  # noqa: E402
from engine_restore_time import blob_array, shape  # noqa: E402


def measure(name, reps):
    buf, off, lens = shape(name)
    eng, heng = bsgpu.Engine(), bsgpu.Engine()
    bufs = [buf]
    try:
        eng.profile(1)
        eng.run(buf.ptr, off, lens)
        n = eng.finish()
        recs = eng.chunks()
        trees_ms = []
        for rep in range(reps + 1):
            roots, ncounts, nodes, arena = eng.trees()
            if rep:
                trees_ms.append(eng.trees_ms()["total"])
        _, uniq, pack_off = eng.dedup()
        ub = eng.unique_bytes
        base = (ub + 15) & ~15
        pool = bsgpu.DeviceBuffer(base + len(arena))
        bufs.append(pool)
        eng.pack_unique(pool, 0, cap=ub)
        bsgpu._check(bsgpu.lib().bsg_memcpy(0, pool.ptr + base,
                                            bsgpu.lib().bsg_engine_tree_arena_device(eng.h),
                                            len(arena), 2), "bsg_memcpy")
        u = uniq.astype(np.int64)
        blobs = np.concatenate([
            blob_array(pack_off[:-1], recs["len"][u], recs["ref"][u]),
            blob_array(nodes["blob_off"] + np.uint64(base), nodes["blob_len"], nodes["ref"])])
        pool_bytes = base + len(arena)

        total = int(sum(lens))
        out = bsgpu.DeviceBuffer(buf.nbytes)
        bufs.append(out)
        rows = []
        for rep in range(reps + 1):  # the first is the warm-up (buffers, kernel load)
            row = {}
            rc, info, status = eng.walk(pool, blobs, roots, pool_bytes=pool_bytes)
            assert rc == 0 and info["nrecs"] == n and info["nnodes"] == len(nodes), (rc, info)
            for k, v in eng.walk_ms().items():
                row[f"walk_{k}_ms"] = v
            row["walk_ms"] = sum(eng.walk_ms().values())
            r = eng.restore(pool, blobs, recs, out, off, lens, pool_bytes=pool_bytes)
            assert r["bytes"] == total
            ms = eng.restore_ms()
            row["restore_ms"] = ms["resolve"] + ms["scatter"]
            rc, r = eng.restore_walk(pool, blobs, out, off, pool_bytes=pool_bytes)
            assert rc == 0 and r["bytes"] == total, (rc, r)
            ms = eng.restore_ms()
            row["restore_walk_ms"] = ms["resolve"] + ms["scatter"]
            if rep:
                rows.append(row)
        got, sizes, counts = eng.copy_walk()
        for f in ("stream", "offset", "len", "ref"):
            assert (got[f] == recs[f]).all(), f
        assert sizes.tolist() == list(lens)
        # the restored bytes split as the input did
        heng.run(out.ptr, off, lens)
        assert heng.finish() == n and heng.chunks().tobytes() == recs.tobytes()

        res = {"shape": name, "streams": len(off), "bytes": total, "n": int(n),
               "nodes": int(len(nodes)), "depth": info["depth"], "nblobs": int(len(blobs)),
               "trees_ms": round(statistics.median(trees_ms), 3)}
        for k in rows[0]:
            res[k] = round(statistics.median(r[k] for r in rows), 3)
        res["walk_over_trees"] = round(res["walk_ms"] / res["trees_ms"], 3)
        res["restore_walk_over_restore"] = round(res["restore_walk_ms"] / res["restore_ms"], 3)
        return res
    finally:
        eng.close()
        heng.close()
        for b in bufs:
            b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="c1,c2,c4")
    a = ap.parse_args()
    for name in a.shapes.split(","):
        print(json.dumps(measure(name, a.reps)), flush=True)


if __name__ == "__main__":
    main()

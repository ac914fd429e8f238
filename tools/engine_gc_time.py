"""Times bsg_engine_gc_mark and bsg_engine_gc_compact in one process, with HIP events on the
engine stream (bsg_engine_profile), median of --reps after one warm-up, beside the two yardsticks
the engine already has on the same pool: bsg_engine_walk's level time over the same Roots and
bsg_engine_restore_walk's scatter over the same streams.
  c2   the configs[2] shape (256 x 64 MiB): the pool is its unique chunks plus its tree nodes
  c1   the configs[1] shape (1 x 1 GiB)
Each shape is split, its trees built, deduplicated and packed as tools/engine_walk_time.py does.
The mark runs from all Roots and from the first half of them; the swept pool (16-aligned) is
walked from the same Roots with bsg_engine_copy_gc's table and must give the same records.
gc_compact_gbs and scatter_gbs count the bytes read plus the bytes written.

Usage: python tools/engine_gc_time.py [--reps 3] [--shapes c2]
Prints one JSON line per shape and set of Roots."""
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
    eng = bsgpu.Engine()
    bufs = [buf]
    try:
        eng.profile(1)
        eng.run(buf.ptr, off, lens)
        eng.finish()
        recs = eng.chunks()
        roots, ncounts, nodes, arena = eng.trees()
        _, uniq, pack_off = eng.dedup()
        ub = eng.unique_bytes
        base = (ub + 15) & ~15
        pool_bytes = base + len(arena)
        pool = bsgpu.DeviceBuffer(pool_bytes)
        bufs.append(pool)
        eng.pack_unique(pool, 0, cap=ub)
        bsgpu._check(bsgpu.lib().bsg_memcpy(0, pool.ptr + base,
                                            bsgpu.lib().bsg_engine_tree_arena_device(eng.h),
                                            len(arena), 2), "bsg_memcpy")
        u = uniq.astype(np.int64)
        blobs = np.concatenate([
            blob_array(pack_off[:-1], recs["len"][u], recs["ref"][u]),
            blob_array(nodes["blob_off"] + np.uint64(base), nodes["blob_len"], nodes["ref"])])
        out = bsgpu.DeviceBuffer(buf.nbytes)
        swept = bsgpu.DeviceBuffer(pool_bytes + 16 * len(blobs))
        bufs += [out, swept]

        ns = len(off)
        for label, k in (("all", ns), ("half", max(ns // 2, 1))):
            rows = []
            for rep in range(reps + 1):  # the first is the warm-up (buffers, kernel load)
                row = {}
                rc, winfo, _ = eng.walk(pool, blobs, roots[:k], pool_bytes=pool_bytes)
                assert rc == 0, (rc, winfo)
                row["walk_levels_ms"] = eng.walk_ms()["levels"]
                rc, r = eng.restore_walk(pool, blobs, out, off[:k], pool_bytes=pool_bytes)
                assert rc == 0, (rc, r)
                row["scatter_ms"] = eng.restore_ms()["scatter"]
                rc, info, status = eng.gc_mark(pool, blobs, roots[:k], pool_bytes=pool_bytes)
                assert rc == 0 and not status.any(), (rc, info)
                rc, nout = eng.gc_compact(pool, swept, align16=True, pool_bytes=pool_bytes)
                assert rc == 0, rc
                for key, v in eng.gc_ms().items():
                    row[f"gc_{key}_ms"] = v
                if rep:
                    rows.append(row)
            want = eng.copy_walk()[0]
            _, table = eng.copy_gc(align16=True)
            rc, winfo2, _ = eng.walk(swept, table, roots[:k], pool_bytes=nout)
            assert rc == 0 and eng.copy_walk()[0].tobytes() == want.tobytes(), (rc, winfo2)
            res = {"shape": name, "roots": label, "nroots": int(k), "nblobs": int(len(blobs)),
                   "pool_bytes": int(pool_bytes), "nlive": info["nlive"],
                   "live_bytes": info["live_bytes"], "ndead": info["ndead"],
                   "nnodes": info["nnodes"], "depth": info["depth"],
                   "restored_bytes": r["bytes"]}
            for key in rows[0]:
                res[key] = round(statistics.median(x[key] for x in rows), 3)
            res["gc_mark_ms"] = round(res["gc_index_ms"] + res["gc_levels_ms"] +
                                      res["gc_offsets_ms"], 3)
            res["gc_compact_gbs"] = round(2 * info["live_bytes"] / res["gc_compact_ms"] / 1e6, 1)
            res["scatter_gbs"] = round(2 * r["bytes"] / res["scatter_ms"] / 1e6, 1)
            res["mark_levels_over_walk_levels"] = round(res["gc_levels_ms"] /
                                                        res["walk_levels_ms"], 3)
            print(json.dumps(res), flush=True)
    finally:
        eng.close()
        for b in bufs:
            b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="c2")
    a = ap.parse_args()
    for name in a.shapes.split(","):
        measure(name, a.reps)


if __name__ == "__main__":
    main()

"""Times bsg_pool_read beside bsg_pool_walk + bsg_pool_restore_walk of the whole streams and one
hipMemcpyDtoDAsync of the bytes read, in one process, with HIP events on the engine stream
(bsg_engine_profile), median of --reps after one warm-up. The shapes are those of
tools/engine_dedup_time.py (c1, c2, c4): the run is put, chunks and nodes, into a pool once; then
three workloads are read out of it, with and without BSG_READ_VERIFY:

  * small: one 4 KiB range per stream at a seeded offset;
  * mib:   one 1 MiB range per stream at a seeded offset;
  * whole: every stream whole.

Per row: the read's six stages (index + Roots, levels, placement, resolve + tiling, verify,
scatter), the host's wall time of the call, the walk's three stages and the restore's three for
the whole streams, the copy, and `verified` over the pool's bytes.

Usage: python tools/pool_read_time.py [--reps 3] [--shapes c1,c2,c4]
Prints one JSON line per shape, workload and flag."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bs_amd import bsgpu  # noqa: E402
from tools.engine_dedup_time import shape  # noqa: E402


def wall(f):
    t0 = time.perf_counter()
    out = f()
    return out, (time.perf_counter() - t0) * 1e3


def measure(name, reps):
    buf, off, lens = shape(name)
    eng = bsgpu.Engine()
    pool = out = None
    try:
        eng.profile(1)
        eng.run(buf.ptr, off, lens)
        n = eng.finish()
        roots, _, nodes, arena = eng.trees()
        nblobs = int(n) + len(nodes)
        pool = bsgpu.Pool(int(sum(lens)) + len(arena) + 16 * nblobs, nblobs)
        eng.pool_put(pool)
        st = pool.stat()
        sizes = [int(x) for x in lens]
        ooff, o = [], 0
        for x in sizes:
            ooff.append(o)
            o += (x + 15 & ~15) + 16
        out = bsgpu.DeviceBuffer(o + 16)
        rng = np.random.default_rng(4096)
        work = {
            "small": [(r.tobytes(), int(rng.integers(0, max(x - 4096, 1))), 4096)
                      for r, x in zip(roots, sizes)],
            "mib": [(r.tobytes(), int(rng.integers(0, max(x - (1 << 20), 1))), 1 << 20)
                    for r, x in zip(roots, sizes)],
            "whole": [(r.tobytes(), 0, x) for r, x in zip(roots, sizes)],
        }
        for label, ranges in work.items():
            for flags in (0, bsgpu.READ_VERIFY):
                rows = []
                for rep in range(reps + 1):  # the first is the warm-up (buffers, kernel load)
                    row = {}
                    (rc, status, got, info), row["read_wall"] = wall(
                        lambda: pool.read(eng, ranges, out, ooff, flags=flags))
                    assert rc == 0, (rc, info)
                    for k, v in eng.read_ms().items():
                        row["read_" + k] = v
                    # the yardsticks: the whole streams walked and restored, and one copy
                    (rc, winfo, _), row["walk_wall"] = wall(lambda: eng.pool_walk(pool, roots))
                    assert rc == 0, rc
                    for k, v in eng.walk_ms().items():
                        row["walk_" + k] = v
                    (rc, rinfo), row["restore_wall"] = wall(
                        lambda: eng.pool_restore_walk(pool, out, ooff, verify=bool(flags)))
                    assert rc == 0, rc
                    for k, v in eng.restore_ms().items():
                        row["restore_" + k] = v
                    t = ctypes.c_float(0)
                    bsgpu._check(bsgpu.lib().bsg_engine_d2d_ms_debug(
                        eng.h, out.ptr, pool.ptr, max(min(info["bytes"], st["bytes"]), 16),
                        ctypes.byref(t)), "d2d")
                    row["d2d_ms"] = t.value
                    if rep:
                        rows.append(row)
                res = {"shape": name, "work": label, "verify": bool(flags), "ranges": len(ranges),
                       "blobs": st["nblobs"], "pool_bytes": st["bytes"], "bytes": info["bytes"],
                       "nnodes": info["nnodes"], "nleaves": info["nleaves"],
                       "depth": info["depth"], "verified": info["verified"],
                       "walk_nnodes": winfo["nnodes"], "walk_nrecs": winfo["nrecs"]}
                for k in sorted(rows[0]):
                    res[k] = round(statistics.median(r[k] for r in rows), 3)
                stages = ("index", "levels", "placement", "resolve", "verify", "scatter")
                res["read_ms"] = round(sum(res["read_" + p] for p in stages), 3)
                res["walk_ms"] = round(sum(res["walk_" + p]
                                           for p in ("index", "levels", "placement")), 3)
                res["restore_ms"] = round(sum(res["restore_" + p]
                                              for p in ("resolve", "verify", "scatter")), 3)

                def ratio(a, b):
                    return round(a / b, 3) if b else None

                res["read_over_walk_restore"] = ratio(res["read_ms"],
                                                      res["walk_ms"] + res["restore_ms"])
                res["read_levels_over_walk_levels"] = ratio(res["read_levels"], res["walk_levels"])
                res["scatter_over_d2d"] = ratio(res["read_scatter"], res["d2d_ms"])
                res["verified_over_pool"] = ratio(res["verified"], st["bytes"])
                print(json.dumps(res), flush=True)
    finally:
        eng.close()
        for x in (buf, pool, out):
            if x is not None:
                x.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="c1,c2,c4")
    a = ap.parse_args()
    for name in a.shapes.split(","):
        measure(name, a.reps)


if __name__ == "__main__":
    main()

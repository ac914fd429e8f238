"""Times bsg_engine_pool_put beside bsg_engine_dedup + bsg_engine_pack_unique of the same run and
one hipMemcpyDtoDAsync of added_bytes, in one process, with HIP events on the engine stream
(bsg_engine_profile), median of --reps after one warm-up. The shapes are those of
tools/engine_dedup_time.py (c1, c1s, c2, c4). Every repetition runs the engine, builds the trees
and then, alternating, dedup + pack and a put of chunks and nodes into a new, empty pool (made and
zero-filled outside the timed parts), so both see the same run in the same state of the device.
The put's parts: first occurrence and offsets, table append and index, gather, where[].

Usage: python tools/engine_pool_time.py [--reps 3] [--shapes c1,c1s,c2,c4]
Prints one JSON line per shape."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bs_amd import bsgpu  # noqa: E402
from tools.engine_dedup_time import shape  # noqa: E402


def measure(name, reps):
    buf, off, lens = shape(name)
    eng = bsgpu.Engine()
    out = None
    try:
        eng.profile(1)
        rows = []
        for rep in range(reps + 1):  # the first is the warm-up (buffers, kernel load)
            eng.run(buf.ptr, off, lens)
            n = eng.finish()
            _, _, nodes, arena = eng.trees()
            row = {}
            for what in (("dedup", "put") if rep % 2 else ("put", "dedup")):
                if what == "dedup":
                    eng.dedup()
                    if out is None:
                        out = bsgpu.DeviceBuffer(max(eng.unique_bytes, 16))
                    eng.pack_unique(out)
                    ms = eng.dedup_ms()
                    row["dedup_ms"], row["pack_ms"] = ms["dedup"], ms["pack"]
                else:
                    nblobs = int(n) + len(nodes)
                    pool = bsgpu.Pool(int(sum(lens)) + len(arena) + 16 * nblobs, nblobs)
                    try:
                        info = eng.pool_put(pool)
                        ms = pool.put_ms()
                    finally:
                        pool.free()
                    row.update(first_ms=ms["first"], append_ms=ms["append"],
                               gather_ms=ms["gather"], where_ms=ms["where"])
            t = ctypes.c_float(0)
            bsgpu._check(bsgpu.lib().bsg_engine_d2d_ms_debug(eng.h, out.ptr, buf.ptr,
                                                             min(info["added_bytes"], buf.nbytes,
                                                                 out.nbytes),
                                                             ctypes.byref(t)), "d2d")
            row["d2d_ms"] = t.value
            if rep:
                rows.append(row)
        res = {"shape": name, "streams": len(off), "bytes": int(sum(lens)), "n": int(n),
               "nodes": len(nodes), "added": info["added"], "added_bytes": info["added_bytes"],
               "repeats": info["repeats"], "unique_bytes": int(eng.unique_bytes)}
        for k in sorted(rows[0]):
            res[k] = round(statistics.median(r[k] for r in rows), 3)
        rest = res["first_ms"] + res["append_ms"] + res["where_ms"]
        res["put_ms"] = round(rest + res["gather_ms"], 3)
        res["gather_over_d2d"] = round(res["gather_ms"] / res["d2d_ms"], 3) if res["d2d_ms"] else None
        res["gather_over_pack"] = round(res["gather_ms"] / res["pack_ms"], 3) if res["pack_ms"] else None
        res["rest_over_dedup"] = round(rest / res["dedup_ms"], 3) if res["dedup_ms"] else None
        return res
    finally:
        eng.close()
        buf.free()
        if out is not None:
            out.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="c1,c1s,c2,c4")
    a = ap.parse_args()
    for name in a.shapes.split(","):
        print(json.dumps(measure(name, a.reps)), flush=True)


if __name__ == "__main__":
    main()

"""Times bsg_pool_collect and bsg_pool_walk beside the host-table forms they stand next to, in one
process, with HIP events on the engine stream (bsg_engine_profile), median of --reps after one
warm-up. The shapes are those of tools/engine_dedup_time.py (c1, c2, c4): the run is put, chunks
and nodes, into a source pool once; then, with all Roots and with every second Root:

  * the pool-native mark (inside bsg_pool_collect) against bsg_engine_gc_mark fed
    bsg_pool_copy_table of the same pool: the three event-timed stages of each, and the host's
    wall time of the whole call (the table's copy out, the host loop over the blobs and the upload
    lie outside the events; a collect's wall time holds its adopt and gather too);
  * the collect's gather against bsg_engine_gc_compact (BSG_GC_ALIGN16) of the same mark into a
    plain buffer and one hipMemcpyDtoDAsync of the live bytes;
  * k_pool_adopt, beside the source put's k_pool_append over its items;
  * bsg_pool_walk against bsg_pool_copy_table + bsg_engine_walk.

Every repetition collects into a new, empty pool (made and zero-filled outside the timed parts).

Usage: python tools/pool_collect_time.py [--reps 3] [--shapes c1,c2,c4]
Prints one JSON line per shape and Root set."""
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
    src = plain = None
    try:
        eng.profile(1)
        eng.run(buf.ptr, off, lens)
        n = eng.finish()
        roots, _, nodes, arena = eng.trees()
        nblobs = int(n) + len(nodes)
        cap = (int(sum(lens)) + len(arena) + 16 * nblobs, nblobs)
        src = bsgpu.Pool(*cap)
        put = eng.pool_put(src)
        append_ms = src.put_ms()["append"]
        st = src.stat()
        plain = bsgpu.DeviceBuffer(st["bytes"] + 16)
        for label, keep in (("all", roots), ("half", roots[::2])):
            keep = np.ascontiguousarray(keep)
            rows = []
            for rep in range(reps + 1):  # the first is the warm-up (buffers, kernel load)
                row = {}
                # today's code: the table out, the mark over it, the compaction into a buffer
                blobs, row["copy_table_wall"] = wall(src.table)
                (rc, ginfo, _), row["mark_host_wall"] = wall(
                    lambda: eng.gc_mark(src.ptr, blobs, keep, pool_bytes=st["pool_bytes"]))
                assert rc == 0, rc
                rc, end = eng.gc_compact(src.ptr, plain, align16=True,
                                         pool_bytes=st["pool_bytes"])
                assert rc == 0, rc
                ms = eng.gc_ms()
                row.update(mark_host_index=ms["index"], mark_host_levels=ms["levels"],
                           mark_host_offsets=ms["offsets"], compact_ms=ms["compact"])
                # the collect
                dst = bsgpu.Pool(*cap)
                try:
                    (rc, info, _), row["collect_wall"] = wall(
                        lambda: eng.pool_collect(src, dst, keep))
                    assert rc == 0 and info["gc"] == ginfo, (rc, info, ginfo)
                    ms = eng.gc_ms()
                    row.update(mark_pool_index=ms["index"], mark_pool_levels=ms["levels"],
                               mark_pool_offsets=ms["offsets"], gather_ms=ms["compact"],
                               adopt_ms=dst.collect_ms())
                    t = ctypes.c_float(0)
                    bsgpu._check(bsgpu.lib().bsg_engine_d2d_ms_debug(
                        eng.h, plain.ptr, src.ptr, min(info["gc"]["live_bytes"], plain.nbytes),
                        ctypes.byref(t)), "d2d")
                    row["d2d_ms"] = t.value
                    # the walks, on the source
                    (rc, winfo, _), row["walk_pool_wall"] = wall(lambda: eng.pool_walk(src, keep))
                    assert rc == 0, rc
                    row["walk_pool_ms"] = sum(eng.walk_ms().values())
                    (rc, hinfo, _), row["walk_host_wall"] = wall(
                        lambda: eng.walk(src.ptr, src.table(), keep, pool_bytes=st["pool_bytes"]))
                    assert rc == 0 and hinfo == winfo, (rc, hinfo, winfo)
                    row["walk_host_ms"] = sum(eng.walk_ms().values())
                finally:
                    dst.free()
                if rep:
                    rows.append(row)
            res = {"shape": name, "roots": label, "nroots": len(keep), "blobs": st["nblobs"],
                   "bytes": st["bytes"], "nlive": info["gc"]["nlive"],
                   "live_bytes": info["gc"]["live_bytes"], "put_items": put["items"],
                   "put_added": put["added"], "put_append_ms": round(append_ms, 3)}
            for k in sorted(rows[0]):
                res[k] = round(statistics.median(r[k] for r in rows), 3)
            for who in ("host", "pool"):
                res["mark_%s_ms" % who] = round(sum(res["mark_%s_%s" % (who, p)]
                                                    for p in ("index", "levels", "offsets")), 3)
            res["mark_host_wall"] = round(res["mark_host_wall"] + res["copy_table_wall"], 3)

            def ratio(a, b):
                return round(res[a] / res[b], 3) if res[b] else None

            res["mark_pool_over_host"] = ratio("mark_pool_ms", "mark_host_ms")
            res["gather_over_compact"] = ratio("gather_ms", "compact_ms")
            res["gather_over_d2d"] = ratio("gather_ms", "d2d_ms")
            res["walk_pool_over_host"] = ratio("walk_pool_ms", "walk_host_ms")
            res["walk_wall_pool_over_host"] = ratio("walk_pool_wall", "walk_host_wall")
            print(json.dumps(res), flush=True)
    finally:
        eng.close()
        for x in (buf, src, plain):
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

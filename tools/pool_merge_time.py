"""Times bsg_pool_merge beside what stands next to it, in one process, with HIP events on the
engine stream (bsg_engine_profile), median of --reps after one warm-up. The shapes are those of
tools/engine_dedup_time.py (c1, c2): the run is put, chunks and nodes, into a source pool once.

  (a) a merge into an empty pool against bsg_pool_collect into an empty pool, with all Roots and
      with every second Root: the mark's three stages of each, then adopt + gather against
      probe + plan + append + gather;
  (b) a merge, with all Roots, into a pool that already holds every second stream, against the
      host route: bsg_pool_copy_table of both pools, a host diff of the refs and a collect of the
      other Roots into a new pool. Wall time and event-timed device time of both; the merge runs
      with BSG_MERGE_VERIFY, so its wall time holds the verify stage, which is reported apart and
      left out of its device time;
  (c) k_pool_probe and k_pool_merge_append per blob beside k_pool_adopt;
  (d) BSG_MERGE_VERIFY's event-timed cost per appended byte, on (b)'s merge.

Every repetition writes into new pools (made and zero-filled outside the timed parts).

Usage: python tools/pool_merge_time.py [--reps 3] [--shapes c1,c2]
Prints one JSON line per shape and Root set."""
import argparse
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


def mark_ms(eng):
    ms = eng.gc_ms()
    return ms["index"] + ms["levels"] + ms["offsets"], ms["compact"]


def measure(name, reps):
    buf, off, lens = shape(name)
    eng = bsgpu.Engine()
    src = None
    try:
        eng.profile(1)
        eng.run(buf.ptr, off, lens)
        n = eng.finish()
        roots, _, nodes, arena = eng.trees()
        nblobs = int(n) + len(nodes)
        cap = (int(sum(lens)) + len(arena) + 16 * nblobs, nblobs)
        src = bsgpu.Pool(*cap)
        eng.pool_put(src)
        st = src.stat()
        for label, keep in (("all", roots), ("half", roots[::2])):
            keep = np.ascontiguousarray(keep)
            rest = np.ascontiguousarray(roots[1::2])
            rows = []
            for rep in range(reps + 1):  # the first is the warm-up (buffers, kernel load)
                row = {}
                pools = [bsgpu.Pool(*cap) for _ in range(4)]
                try:
                    # (a) into an empty pool
                    (rc, cinfo, _), row["collect_wall"] = wall(
                        lambda: eng.pool_collect(src, pools[0], keep))
                    assert rc == 0, rc
                    row["collect_mark"], row["collect_gather"] = mark_ms(eng)
                    row["collect_adopt"] = pools[0].collect_ms()
                    (rc, minfo, _), row["merge_wall"] = wall(
                        lambda: eng.pool_merge(src, pools[1], keep))
                    assert rc == 0 and minfo["added"] == cinfo["gc"]["nlive"], (rc, minfo)
                    row["merge_mark"], _ = mark_ms(eng)
                    ms = eng.pool_merge_ms()
                    for k in ("probe", "plan", "append", "gather"):
                        row["merge_" + k] = ms[k]
                    # (b) with overlap: the destination holds every second stream
                    assert eng.pool_collect(src, pools[2],
                                            np.ascontiguousarray(roots[::2]))[0] == 0

                    def host_route():
                        a, b = src.table(), pools[2].table()
                        va = np.ascontiguousarray(a["ref"]).view("V32").reshape(-1)
                        vb = np.ascontiguousarray(b["ref"]).view("V32").reshape(-1)
                        missing = ~np.isin(va, vb)
                        return int(missing.sum()), eng.pool_collect(src, pools[3], rest)

                    (nmiss, (rc, _, _)), row["host_route_wall"] = wall(host_route)
                    assert rc == 0, rc
                    hm, hg = mark_ms(eng)
                    row["host_route_device"] = hm + hg + pools[3].collect_ms()
                    (rc, oinfo, _), row["overlap_wall"] = wall(
                        lambda: eng.pool_merge(src, pools[2], roots, verify=True))
                    assert rc == 0 and oinfo["verified"] == oinfo["added_bytes"], (rc, oinfo)
                    ms = eng.pool_merge_ms()
                    row["overlap_verify"] = ms["verify"]
                    row["overlap_device"] = (mark_ms(eng)[0] + ms["probe"] + ms["plan"]
                                             + ms["append"] + ms["gather"])
                    row["overlap_added"], row["overlap_added_bytes"] = (oinfo["added"],
                                                                        oinfo["added_bytes"])
                    row["overlap_known"] = oinfo["known"]
                finally:
                    for p in pools:
                        p.free()
                if rep:
                    rows.append(row)
            res = {"shape": name, "roots": label, "nroots": len(keep), "blobs": st["nblobs"],
                   "bytes": st["bytes"], "nlive": cinfo["gc"]["nlive"],
                   "live_bytes": cinfo["gc"]["live_bytes"]}
            for k in sorted(rows[0]):
                res[k] = round(statistics.median(r[k] for r in rows), 3)
            res["collect_device"] = round(res["collect_mark"] + res["collect_adopt"]
                                          + res["collect_gather"], 3)
            res["merge_device"] = round(res["merge_mark"] + res["merge_probe"] + res["merge_plan"]
                                        + res["merge_append"] + res["merge_gather"], 3)

            def ratio(a, b):
                return round(res[a] / res[b], 3) if res[b] else None

            res["merge_over_collect_device"] = ratio("merge_device", "collect_device")
            res["merge_over_collect_wall"] = ratio("merge_wall", "collect_wall")
            res["merge_gather_over_collect_gather"] = ratio("merge_gather", "collect_gather")
            res["overlap_over_host_route_wall"] = ratio("overlap_wall", "host_route_wall")
            res["probe_ns_per_blob"] = round(1e6 * res["merge_probe"] / max(st["nblobs"], 1), 3)
            res["append_ns_per_blob"] = round(1e6 * res["merge_append"] / max(res["nlive"], 1), 3)
            res["adopt_ns_per_blob"] = round(1e6 * res["collect_adopt"] / max(st["nblobs"], 1), 3)
            res["verify_ns_per_byte"] = (round(1e6 * res["overlap_verify"]
                                               / res["overlap_added_bytes"], 4)
                                         if res["overlap_added_bytes"] else None)
            print(json.dumps(res), flush=True)
    finally:
        eng.close()
        for x in (buf, src):
            if x is not None:
                x.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="c1,c2")
    a = ap.parse_args()
    for name in a.shapes.split(","):
        measure(name, a.reps)


if __name__ == "__main__":
    main()

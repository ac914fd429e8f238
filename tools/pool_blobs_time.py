"""Times bsg_pool_put_blobs beside bsg_engine_pool_put of the same blobs, and bsg_pool_get beside
one hipMemcpyDtoDAsync of the same byte count, in one process, with HIP events on the engine
stream (bsg_engine_profile), median of --reps after one warm-up. The blobs are the chunks and tree
nodes of one run over --mib MiB of splitmix bytes, repacked at 16-byte offsets for put_blobs; each
repetition puts into a pool emptied outside the timed parts. The get asks for every ref of the
pool in table order.

Usage: python tools/pool_blobs_time.py [--reps 5] [--mib 128]
Prints one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from bs_amd import bsgpu  # noqa: E402
from bs_amd.synth import splitmix_array  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mib", type=int, default=128)
    a = ap.parse_args()
    data = splitmix_array(0xB10B5, a.mib << 20)
    eng = bsgpu.Engine()
    buf = bsgpu.DeviceBuffer(len(data))
    buf.from_host(data)
    eng.profile(1)
    eng.run(buf.ptr, [0], [len(data)])
    eng.finish()
    recs = eng.chunks()
    _, _, nodes, arena = eng.trees()
    parts = [data[int(r["offset"]):int(r["offset"] + r["len"])] for r in recs] + \
            [arena[int(t["blob_off"]):int(t["blob_off"]) + int(t["blob_len"])] for t in nodes]
    lens = [len(p) for p in parts]
    off = (np.cumsum([(n + 15) & ~15 for n in lens]) - [(n + 15) & ~15 for n in lens]).tolist()
    packed = np.zeros(off[-1] + lens[-1] + 16, dtype=np.uint8)
    for p, o in zip(parts, off):
        packed[o:o + len(p)] = p
    src = bsgpu.DeviceBuffer(len(packed))
    src.from_host(packed)
    pool = bsgpu.Pool(len(packed) + 16, len(parts))
    out = bsgpu.DeviceBuffer(len(packed) + 16)
    rows = []
    try:
        for rep in range(a.reps + 1):  # the first is the warm-up (buffers, kernel load)
            row = {}
            pool.reset()
            info = eng.pool_put(pool)
            ms = pool.put_ms()
            row["run_append_ms"], row["run_gather_ms"] = ms["append"], ms["gather"]
            pool.reset()
            rc, binfo, _ = pool.put_blobs(eng, src, off, lens)
            assert rc == 0 and binfo == info, (rc, binfo, info)
            ms = pool.blobs_ms(eng)
            row.update(hash_ms=ms["hash"], plan_ms=ms["plan"], append_gather_ms=ms["append"])
            refs = pool.table()["ref"]
            rc, ginfo, _, out_off = pool.get(eng, refs, out)
            assert rc == 0 and ginfo["missing"] == 0, (rc, ginfo)
            ms = pool.blobs_ms(eng)
            row.update(probe_ms=ms["probe"], get_gather_ms=ms["gather"])
            rc, _, _, _ = pool.get(eng, refs, out, verify=True)
            assert rc == 0
            row["verify_ms"] = pool.blobs_ms(eng)["verify"]
            t = ctypes.c_float(0)
            bsgpu._check(bsgpu.lib().bsg_engine_d2d_ms_debug(eng.h, out.ptr, src.ptr,
                                                             int(out_off[-1]), ctypes.byref(t)),
                         "d2d")
            row["d2d_ms"] = t.value
            if rep:
                rows.append(row)
        res = {"bytes": len(data), "blobs": len(parts), "added": info["added"],
               "added_bytes": info["added_bytes"], "get_bytes": int(out_off[-1])}
        for k in sorted(rows[0]):
            res[k] = round(statistics.median(r[k] for r in rows), 3)
        run = res["run_append_ms"] + res["run_gather_ms"]
        res["append_gather_over_run"] = round(res["append_gather_ms"] / run, 3) if run else None
        res["get_gather_over_d2d"] = round(res["get_gather_ms"] / res["d2d_ms"], 3) \
            if res["d2d_ms"] else None
        print(json.dumps(res), flush=True)
    finally:
        eng.close()
        for b in (buf, src, out):
            b.free()
        pool.free()


if __name__ == "__main__":
    main()

"""Times bsg_engine_restore in one process, with HIP events on the engine stream
(bsg_engine_profile), median of --reps after one warm-up:
  c1   the configs[1] shape (1 x 1 GiB, SplitMix) at the default parameters
  c2   the configs[2] shape (256 x 64 MiB)
  c4   configs[4] at full size: stream B = stream A (1 GiB) with 1,024 edits
Each shape is split, deduplicated and packed (bsg_engine_pack_unique); its streams are then
restored from that packed pool (scatter_ms) and, with BSG_RESTORE_VERIFY, from a pool that
holds the same blobs at 16-byte aligned offsets (verify_ms). Beside them, the same way: one
hipMemcpyDtoDAsync of the restored byte count (d2d_ms) and bsg_engine_hash of the aligned pool
in batches of 65,535 blobs (hash_ms, the sum of the runs' stages). The restored bytes are split
again once and their records held to the first run's.

Usage: python tools/engine_restore_time.py [--reps 3] [--shapes c1,c2,c4]
Prints one JSON line per shape."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bs_amd import bsgpu  # noqa: E402
from bs_amd.synth import BASE_SEED, edit_stream, splitmix_array  # noqa: E402

HASH_BATCH = 65535


def shape(name):
    """(device buffer, off, lens) of a shape, built in device memory."""
    if name in ("c1", "c2"):
        ns, each = (256, 64 << 20) if name == "c2" else (1, 1 << 30)
        buf = bsgpu.DeviceBuffer(ns * each)
        bsgpu.fill_splitmix(buf.ptr, ns * each, BASE_SEED)
        bsgpu.synchronize()
        return buf, [i * each for i in range(ns)], [each] * ns
    a = splitmix_array(BASE_SEED, 1 << 30)
    b = edit_stream(a, BASE_SEED + 1)
    ob = (len(a) + 15) & ~15
    buf = bsgpu.DeviceBuffer(ob + len(b))
    buf.from_host(a)
    buf.from_host(b, ob)
    return buf, [0, ob], [len(a), len(b)]


def blob_array(off, lens, refs):
    b = np.zeros(len(off), dtype=bsgpu.POOL_BLOB_DTYPE)
    b["off"], b["len"], b["ref"] = off, lens, refs
    return b


def measure(name, reps):
    buf, off, lens = shape(name)
    eng, heng = bsgpu.Engine(), bsgpu.Engine()
    bufs = [buf]
    try:
        eng.profile(1)
        heng.profile(1)
        eng.run(buf.ptr, off, lens)
        n = eng.finish()
        recs = eng.chunks()
        _, uniq, pack_off = eng.dedup()
        packed = bsgpu.DeviceBuffer(max(eng.unique_bytes, 16))
        bufs.append(packed)
        eng.pack_unique(packed)
        u = uniq.astype(np.int64)
        blen = recs["len"][u]
        tight = blob_array(pack_off[:-1], blen, recs["ref"][u])

        # the same blobs at 16-byte aligned offsets, written by a restore of one stream per blob
        a_off = np.concatenate([[0], np.cumsum((blen + 15) & ~np.uint64(15))]).astype(np.uint64)
        apool = bsgpu.DeviceBuffer(int(a_off[-1]) + bsgpu.READ_SLACK)
        bufs.append(apool)
        one = np.zeros(len(u), dtype=bsgpu.CHUNK_DTYPE)
        one["len"], one["stream"], one["ref"] = blen, np.arange(len(u)), recs["ref"][u]
        eng.restore(packed, tight, one, apool, a_off[:-1], blen, pool_bytes=eng.unique_bytes)
        aligned = blob_array(a_off[:-1], blen, recs["ref"][u])

        total = int(sum(lens))
        out = bsgpu.DeviceBuffer(buf.nbytes)
        bufs.append(out)
        rows = []
        for rep in range(reps + 1):  # the first is the warm-up (buffers, kernel load)
            row = {}
            info = eng.restore(packed, tight, recs, out, off, lens, pool_bytes=eng.unique_bytes)
            assert info["bytes"] == total
            ms = eng.restore_ms()
            row["resolve_ms"], row["scatter_ms"] = ms["resolve"], ms["scatter"]
            info = eng.restore(apool, aligned, recs, out, off, lens, verify=True,
                               pool_bytes=apool.nbytes)
            assert info["verified"] == int(blen.sum()) and info["bad_blob"] == bsgpu.NONE64
            ms = eng.restore_ms()
            row["verify_ms"], row["scatter_aligned_ms"] = ms["verify"], ms["scatter"]
            row["hash_ms"] = 0.0
            for b0 in range(0, len(u), HASH_BATCH):
                heng.hash(apool.ptr, aligned["off"][b0:b0 + HASH_BATCH],
                          blen[b0:b0 + HASH_BATCH])
                heng.finish()
                row["hash_ms"] += sum(heng.stage_ms())
            t = ctypes.c_float(0)
            bsgpu._check(bsgpu.lib().bsg_engine_d2d_ms_debug(eng.h, out.ptr, buf.ptr, total,
                                                             ctypes.byref(t)), "d2d")
            row["d2d_ms"] = t.value
            if rep:
                rows.append(row)
        # the restored bytes split as the input did
        eng.restore(packed, tight, recs, out, off, lens, pool_bytes=eng.unique_bytes)
        heng.run(out.ptr, off, lens)
        assert heng.finish() == n and heng.chunks().tobytes() == recs.tobytes()

        res = {"shape": name, "streams": len(off), "bytes": total, "n": int(n),
               "nblobs": int(len(u)), "pool_bytes": int(eng.unique_bytes)}
        for k in rows[0]:
            res[k] = round(statistics.median(r[k] for r in rows), 3)
        res["scatter_over_d2d"] = round(res["scatter_ms"] / res["d2d_ms"], 3)
        res["verify_over_hash"] = round(res["verify_ms"] / res["hash_ms"], 3)
        res["scatter_gibs"] = round(total / 2**30 / (res["scatter_ms"] / 1e3), 1)
        res["pool_share_of_bytes"] = round(res["pool_bytes"] / max(total, 1), 4)
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

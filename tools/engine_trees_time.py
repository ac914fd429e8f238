"""Times bsg_engine_trees (split.Writer's tree and Root per stream, built on the device) beside
the engine run it follows, in one process, with HIP events on the engine stream
(bsg_engine_profile): the configs[1] shape (1 x 1 GiB) and the configs[2] shape (256 x 64 MiB) at
the default parameters, and the one-wide-node case (Bits 4 / MinSize 64 / Fanout 1000, one
stream) whose single node's hash is compared with bsg_engine_hash of a blob of the same length.

Usage: python tools/engine_trees_time.py [--reps 3] [--shapes c1,c2,wide] [--wide-mib 1024]
Prints one JSON line per shape."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bs_amd import bsgpu  # noqa: E402


def measure(ns, each, bits, mn, fan, reps):
    n = ns * each
    buf = bsgpu.DeviceBuffer(n)
    eng = bsgpu.Engine()
    try:
        bsgpu.fill_splitmix(buf.ptr, n, 0xB5B52026)
        bsgpu.synchronize()
        off = [i * each for i in range(ns)]
        lens = [each] * ns
        eng.profile(1)
        rows = []
        for rep in range(reps + 1):  # the first is the warm-up (buffers, kernel load)
            t0 = time.perf_counter()
            eng.run(buf.ptr, off, lens, bits=bits, min_size=mn, fanout=fan)
            nchunks = eng.finish()
            t1 = time.perf_counter()
            nn, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
            bsgpu._check(bsgpu.lib().bsg_engine_trees(eng.h, ctypes.byref(nn),
                                                      ctypes.byref(nb)), "bsg_engine_trees")
            t2 = time.perf_counter()
            if rep:
                ms = eng.trees_ms()
                rows.append({"step_wall_ms": (t1 - t0) * 1e3, "step_stage_ms": sum(eng.stage_ms()),
                             "trees_wall_ms": (t2 - t1) * 1e3, **{"trees_" + k: v for k, v in ms.items()}})
        out = {"streams": ns, "stream_mib": each >> 20, "bits": bits, "min_size": mn, "fanout": fan,
               "chunks": int(nchunks), "nodes": int(nn.value), "arena_bytes": int(nb.value)}
        for k in rows[0]:
            out[k] = round(statistics.median(r[k] for r in rows), 3)
        return out, eng, buf
    except Exception:
        eng.close()
        buf.free()
        raise


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="c1,c2,wide")
    ap.add_argument("--wide-mib", type=int, default=1024)
    a = ap.parse_args()
    for shape in a.shapes.split(","):
        if shape == "c1":
            out, eng, buf = measure(1, 1 << 30, 16, 1024, 8, a.reps)
        elif shape == "c2":
            out, eng, buf = measure(256, 64 << 20, 16, 1024, 8, a.reps)
        else:
            out, eng, buf = measure(1, a.wide_mib << 20, 4, 64, 1000, a.reps)
            # the same number of SHA-256 blocks as one blob through bsg_engine_hash
            blob = min(out["arena_bytes"], buf.nbytes)
            assert out["nodes"] == 1
            ts = []
            for _ in range(a.reps + 1):
                eng.hash(buf.ptr, [0], [blob])
                eng.finish()
                ts.append(eng.stage_ms()[2])
            out["hash_blob_bytes"] = int(blob)
            out["engine_hash_sha_ms"] = round(statistics.median(ts[1:]), 3)
            out["node_hash_over_engine_hash"] = round(out["trees_hash"] / statistics.median(ts[1:]), 3) \
                if blob == out["arena_bytes"] else None
        out["shape"] = shape
        print(json.dumps(out), flush=True)
        eng.close()
        buf.free()


if __name__ == "__main__":
    main()

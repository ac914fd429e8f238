"""Times bsg_engine_dedup and bsg_engine_pack_unique beside the engine run they follow, in one
process, with HIP events on the engine stream (bsg_engine_profile), median of --reps after one
warm-up:
  c1   the configs[1] shape (1 x 1 GiB, SplitMix) at the default parameters
  c1s  the same after one 69-byte stream, so every packed byte's source address differs from its
       destination's by 5 mod 16 (c1 alone copies at equal residues)
  c2   the configs[2] shape (256 x 64 MiB)
  c4   configs[4] at full size: stream B = stream A (1 GiB) with 1,024 edits
Each shape packs with both load variants of k_pack (unaligned 16-byte loads; aligned loads and a
byte funnel) and times one hipMemcpyDtoDAsync of unique_bytes the same way.

Usage: python tools/engine_dedup_time.py [--reps 3] [--shapes c1,c1s,c2,c4]
Prints one JSON line per shape."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bs_amd import bsgpu  # noqa: E402
from bs_amd.synth import BASE_SEED, edit_stream, splitmix_array  # noqa: E402


def shape(name):
    """(device buffer, off, lens) of a shape, built in device memory."""
    if name in ("c1", "c1s", "c2"):
        ns, each = (256, 64 << 20) if name == "c2" else (1, 1 << 30)
        lead = 256 if name == "c1s" else 0
        buf = bsgpu.DeviceBuffer(lead + ns * each)
        bsgpu.fill_splitmix(buf.ptr, lead + ns * each, BASE_SEED)
        bsgpu.synchronize()
        off = [lead + i * each for i in range(ns)]
        lens = [each] * ns
        if lead:
            off, lens = [0] + off, [69] + lens
        return buf, off, lens
    a = splitmix_array(BASE_SEED, 1 << 30)
    b = edit_stream(a, BASE_SEED + 1)
    ob = (len(a) + 15) & ~15
    buf = bsgpu.DeviceBuffer(ob + len(b))
    buf.from_host(a)
    buf.from_host(b, ob)
    return buf, [0, ob], [len(a), len(b)]


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
            step = sum(eng.stage_ms())
            eng.dedup()
            if out is None:
                out = bsgpu.DeviceBuffer(max(eng.unique_bytes, 16))
            row = {"step_ms": step}
            for mode, key in ((0, "pack_ms"), (1, "pack_funnel_ms")):
                bsgpu._check(bsgpu.lib().bsg_engine_pack_mode_debug(eng.h, mode), "pack mode")
                eng.pack_unique(out)
                ms = eng.dedup_ms()
                row["dedup_ms"] = ms["dedup"]
                row[key] = ms["pack"]
            t = ctypes.c_float(0)
            bsgpu._check(bsgpu.lib().bsg_engine_d2d_ms_debug(eng.h, out.ptr, buf.ptr,
                                                             min(eng.unique_bytes, buf.nbytes),
                                                             ctypes.byref(t)), "d2d")
            row["d2d_ms"] = t.value
            if rep:
                rows.append(row)
        res = {"shape": name, "streams": len(off), "bytes": int(sum(lens)), "n": int(n),
               "nunique": int(eng.nunique), "unique_bytes": int(eng.unique_bytes)}
        for k in rows[0]:
            res[k] = round(statistics.median(r[k] for r in rows), 3)
        res["dedup_over_step"] = round(res["dedup_ms"] / res["step_ms"], 4)
        res["pack_over_d2d"] = round(res["pack_ms"] / res["d2d_ms"], 3) if res["d2d_ms"] else None
        res["unique_share_of_bytes"] = round(res["unique_bytes"] / max(res["bytes"], 1), 4)
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

"""bench.py's one-line JSON contract, on a small workload (the driver runs the full default).

Checks the keys and types the round-end driver and the judge read: the metric and unit of
BASELINE.json, the whole-job value, the roofline object (bound, achieved, peak, unit, frac,
traffic) and the cpu_baseline object (value, unit, cores, kind, sample). The legs beside the
headline figure run under --full; a plain run carries the headline alone and --dump-outputs
writes the last timed step's records.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_json_line():
    cmd = [sys.executable, "bench.py", "--full", "--steps", "2", "--warmup", "1", "--streams", "2",
           "--stream-mib", "64", "--cpu-sample-mib", "8", "--e2e-mib", "64"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    with open(os.path.join(ROOT, "BASELINE.json")) as f:
        base = json.load(f)
    assert d["metric"] == base["metric"]
    assert d["unit"] == "GiB/s" and d["higher_is_better"] is True
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["dtype"] == "u8" and "synthetic" in d["data"]
    assert d["config"]["workload"] and d["config"]["streams_per_gpu"] == 2
    rf = d["roofline"]
    # the bound that binds; the graded fraction stays the HBM roof's
    assert rf["bound"] and rf["roof"] in ("hbm", "mfma") and rf["unit"] == "GB/s"
    assert rf["peak"] > 0 and rf["achieved"] > 0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    assert "traffic" in rf
    cb = d["cpu_baseline"]
    assert cb["value"] > 0 and cb["unit"] == "GiB/s" and cb["cores"] >= 1
    assert cb["kind"] in ("port", "reference") and cb["sample"]
    assert d["end_to_end"]["value"] > 0
    assert d["chain_roofline"]["frac"] > 0
    assert d["oracle_check"] is True and d["oracle_checked"]  # parity on the bench's own bytes


@pytest.mark.gpu
def test_bench_default_carries_configs2():
    """Under --full the default workload (configs[1]) also carries the nested configs[2] record."""
    cmd = [sys.executable, "bench.py", "--full", "--steps", "2", "--warmup", "1",
           "--configs2-steps", "1",
           "--cpu-sample-mib", "64", "--e2e-mib", "0"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["config"]["workload"].startswith("configs[1]")
    c2 = d["configs2"]
    assert c2["workload"].startswith("configs[2]") and c2["steps"] == 1
    assert c2["value"] > d["value"] and c2["ms_per_step"] > 0
    assert c2["roofline"]["kernel"].startswith("k_sha") and c2["roofline"]["frac"] > 0
    assert c2["roofline"]["k_scan"]["frac"] > 0
    assert c2["cpu_baseline"]["cores"] >= 1 and c2["cpu_baseline"]["full_writer"]["value"] > 0
    assert set(c2["stage_ms"]) == set(d["stage_ms"])
    assert d["oracle_check"] is True and c2["oracle_check"] is True


def _plain_run(extra):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--streams", "3", "--stream-mib", "8"] + extra
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_run_and_dump_outputs(tmp_path, oracle):
    """A plain run times its steps and nothing else: the legs beside the headline are null.
    --dump-outputs writes the last timed step's records as float .npy files, the same from run
    to run, and they are the oracle's chunks of the same seeded streams."""
    import numpy as np
    from bs_amd.synth import splitmix_array
    import bench
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    d = _plain_run(["--dump-outputs", a])
    _plain_run(["--dump-outputs", b])
    assert d["full"] is False and d["steps"] == 2 and d["warmup"] == 1
    assert d["unit"] == "GiB/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    for leg in ("cpu_baseline", "end_to_end", "writer_e2e", "configs2", "oracle_check"):
        assert d[leg] is None, leg
    # value and ms_per_step are the same measurement: 3 x 8 MiB per step
    assert d["ms_per_step"] > 0
    assert abs(d["value"] - (24 / 1024) / (d["ms_per_step"] * 1e-3)) <= 0.02 * d["value"]
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and "ref.npy" in names and "offset.npy" in names
    got = {n[:-4]: np.load(os.path.join(a, n)) for n in names}
    assert sum(v.nbytes for v in got.values()) <= 64 * 10**6
    for n in names:
        assert got[n[:-4]].dtype in (np.float32, np.float64), n
        assert np.array_equal(got[n[:-4]], np.load(os.path.join(b, n))), n
    table = oracle.buzhash32_table(1)
    k = 0
    assert len(got["counts"]) == 3 and got["nchunks"][0] == got["counts"].sum() == len(got["ref"])
    for s in range(3):
        ref = oracle.split(table, splitmix_array(bench.BASE_SEED + s, 8 << 20))
        c = int(got["counts"][s])
        assert c == len(ref)
        for f in ("offset", "len", "level", "ref"):
            assert np.array_equal(got[f][k:k + c], ref[f].astype(got[f].dtype)), (s, f)
        assert (got["stream"][k:k + c] == s).all()
        k += c

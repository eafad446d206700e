"""bench.py's command line: --dump-outputs (float64 arrays, a seeded sample above the size cap,
identical from run to run) and the plain run's line (the headline alone; the passes that take
runs of their own only with --full)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("hbm_resident_ms_per_step", "latency_ms_per_step", "device_resident_ms_per_step",
             "kernels_ms_per_partition", "roofline", "cpu_baseline")


def test_dump_outputs_whole_arrays(tmp_path):
    a = np.arange(7, dtype=np.int32)
    w = np.linspace(1.0, 0.0, 7)
    bench.dump_outputs(str(tmp_path / "d"), {"a": a, "w": w})
    ga, gw = np.load(tmp_path / "d" / "a.npy"), np.load(tmp_path / "d" / "w.npy")
    assert ga.dtype == np.float64 and gw.dtype == np.float64
    assert np.array_equal(ga, a) and np.array_equal(gw, w)


def test_dump_outputs_samples_above_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 8 * 100)
    a, b, lab = np.arange(300), np.arange(300) * 2.0, np.arange(150)
    for d in ("d1", "d2"):
        bench.dump_outputs(str(tmp_path / d), {"a": a, "b": b, "lab": lab})
    got = {k: np.load(tmp_path / "d1" / (k + ".npy")) for k in ("a", "b", "lab")}
    assert sum(v.nbytes for v in got.values()) <= 8 * 100
    assert all(v.shape[0] > 0 and np.all(np.diff(v) > 0) for v in got.values())  # ascending picks, no repeats
    assert np.array_equal(got["b"], got["a"] * 2.0)  # equal-length columns keep the same rows
    assert np.isin(got["lab"], lab).all()
    for k, v in got.items():  # the same entries in every run
        assert np.array_equal(v, np.load(tmp_path / "d2" / (k + ".npy")))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps(tmp_path):
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--n", "20000", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120,
                       cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert all(k in line for k in HEADLINE) and not any(k in line for k in FULL_ONLY)
    assert line["steps"] == 2 and line["full"] is False and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(20000 / (line["ms_per_step"] * 1e-3))
    n = 20000
    va, vb, w, lab = (np.load(out / (k + ".npy")) for k in ("merged_vertex_a", "merged_vertex_b", "merged_weight", "labels"))
    assert all(x.dtype == np.float64 for x in (va, vb, w, lab))
    assert va.shape == vb.shape == w.shape == (2 * n - 1,) and lab.shape == (n,)
    assert np.all(w[:-1] >= w[1:]) and int((va != vb).sum()) == n - 1
    assert lab.min() >= 0 and lab.max() == line["n_clusters"]

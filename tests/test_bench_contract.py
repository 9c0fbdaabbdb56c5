"""The bench.py contract, checked without a GPU: the CLI the driver calls exists, and the JSON lines this tree produced on hardware
(committed under profiles/) carry every field the contract names, with the metric / unit BASELINE.json prescribes."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
       "roofline", "cpu_baseline"}
ROOFLINE = {"bound", "achieved", "peak", "unit", "frac", "traffic"}
CPU = {"value", "unit", "cores", "kind", "sample"}


def test_cli_flags_of_the_contract():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert flag in out.stdout



@pytest.mark.timeout(300)
def test_plain_run_is_lean_counts_its_steps_and_dumps_the_last_step(tmp_path):
    """a plain run (no --full) times exactly --steps steps, prints the headline fields and nothing that needs extra steps or runs, and --dump-outputs
    writes the last timed step's outputs as float32 / float64 .npy files; that step starts from the seeded initial state, so two runs with the same
    arguments write the same arrays (bit for bit on the host simulator).
    No GPU here: --simulate, one process"""
    import numpy as np
    env = dict(os.environ, MAED_SYNTHETIC_SMPL_OK="1", OMP_NUM_THREADS="2")
    runs = []
    for i in range(2):
        out_dir = tmp_path / f"dump{i}"
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--simulate", "--dtype", "f32",
               "--dump-outputs", str(out_dir)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        d = json.loads(lines[0])
        assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(d)
        assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["step_time"]["how"] and d["first_step_loss"] is not None
        assert not {"host_enqueue_ms", "roofline", "kernels", "cpu_baseline", "parity_mode", "graph", "value_at_1e3"} & set(d), sorted(d)
        files = sorted(os.listdir(out_dir))
        assert {"loss.npy", "theta.npy", "kp_2d.npy", "kp_3d.npy", "params.npy"} <= set(files), files
        arrays = {f: np.load(out_dir / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        # the dumped step starts from the seeded initial state: it recomputes the very first step's objective
        assert float(arrays["loss.npy"]) == d["first_step_loss"], (float(arrays["loss.npy"]), d["first_step_loss"])
        runs.append((d, arrays))
    assert runs[0][0]["first_step_loss"] == runs[1][0]["first_step_loss"]
    assert runs[0][1].keys() == runs[1][1].keys()
    for name, a in runs[0][1].items():
        assert a.shape == runs[1][1][name].shape and np.array_equal(a, runs[1][1][name]), name


@pytest.mark.parametrize("path", [os.path.join(ROOT, "profiles", "r02_bench_train.json"), os.path.join(ROOT, "profiles", "r02_bench_torchrun_world1_forced_collectives.json"),
                                  os.path.join(ROOT, "profiles", "r01_bench_v10_train_27.6ms.json")])
def test_committed_bench_lines_carry_the_contract_fields(path):
    d = json.loads(open(path).read().strip().split("\n")[-1])
    assert TOP <= set(d), TOP - set(d)
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert d["unit"] == "video-clips/sec" and base["metric"].startswith(d["unit"]) and d["metric"].startswith(d["unit"])
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["data"] == "synthetic" and d["vs_baseline"] is None
    assert d["n_gpus"] == 1 and d["steps"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - 8 * d["n_gpus"] * 1e3 / d["ms_per_step"]) < 0.02 * d["value"]       # whole-job clips/s = clips per step / step time
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert ROOFLINE <= set(r) and r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    if d["cpu_baseline"] is not None:                                                         # (absent in --no-cpu-baseline A/B runs)
        c = d["cpu_baseline"]
        assert CPU <= set(c) and c["kind"] in ("port", "reference") and c["cores"] >= 1
    if "step_time" in d:                                                                      # round 2 on: per-step hipEvent statistics
        st = d["step_time"]
        assert st["p10_ms"] <= st["median_ms"] <= st["p90_ms"] and abs(st["median_ms"] - d["ms_per_step"]) < 0.1 * d["ms_per_step"]


def test_committed_pmc_traffic_is_stamped_with_a_source_hash():
    """bench.py quotes roofline.traffic only from a PMC file measured on the running build: the committed file names the hash of the kernel sources it
    was collected on and the per-launch bytes of the three roofline kernels"""
    t = json.load(open(os.path.join(ROOT, "profiles", "r02_pmc", "traffic.json")))
    assert len(t["source_hash"]) == 16 and set(t["kernels"]) == {"attn_spatial_fwd", "gemm_nt", "gemm_tn"}
    assert all(isinstance(v, int) and v > 0 for v in t["kernels"].values())
    # the attention forward moves its algorithmic bytes and nothing more (4*M*C*2 + lse at cfg3 = 103.6 MB)
    assert abs(t["kernels"]["attn_spatial_fwd"] - 103.6e6) < 0.02 * 103.6e6

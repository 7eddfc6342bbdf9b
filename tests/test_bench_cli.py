"""bench.py's command-line contract on the CPU (no GPU here): the RCCL
launch refuses more ranks than visible GPUs before any process group exists,
and the BASELINE configs[0] line (the CPU PyTorch path) prints one JSON line.
On the GPU: a plain run's headline line and --dump-outputs files, and the
fields --full adds, each on a small workload."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _run(args, env_over=None, timeout=300):
    env = dict(os.environ, **(env_over or {}))
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=timeout)


def test_nccl_refuses_more_ranks_than_gpus():
    """WORLD_SIZE=2 under --backend nccl with fewer visible GPUs (none here):
    exit code 3 and a message, before init_process_group (no MASTER_PORT is
    listening, so reaching the rendezvous would hang until the timeout)."""
    r = _run(["--gpus", "2", "--backend", "nccl"],
             dict(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="1",
                  HIP_VISIBLE_DEVICES=""), timeout=120)
    assert r.returncode == 3, (r.returncode, r.stderr[-2000:])
    assert "one GPU per rank" in r.stderr


def test_config1_cpu_line():
    """--config 1: the oracle's training step on the host (precrop window,
    TV, RAdam), one JSON line naming BASELINE configs[0]; a reduced batch
    keeps the test short."""
    r = _run(["--config", "1", "--steps", "1", "--n-rand", "64"])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert "BASELINE configs[0]" in line["config"]["workload"]
    assert line["n_gpus"] == 0 and line["value"] > 0 and line["unit"] == "rays/s"


def test_dump_outputs_is_for_the_hip_trainer():
    """--dump-outputs with the CPU path (--config 1) is refused before any work."""
    r = _run(["--config", "1", "--steps", "1", "--n-rand", "64", "--dump-outputs", "unused"], timeout=120)
    assert r.returncode != 0 and "--dump-outputs" in r.stderr


HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("roofline", "kernels", "mfma", "host_enqueue_ms", "sparsity", "cpu_baseline")
# a small workload: no untimed training, 300 rays (not a multiple of the 32-sample tile rows)
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--pretrain", "0", "--scene", "uniform", "--n-rand", "300"]


@pytest.mark.gpu
def test_plain_run_headline_and_dump(tmp_path):
    """A plain run prints the headline fields only, and --dump-outputs writes
    the last timed step's outputs as float32 .npy files under 64 MB in all:
    finite, per-ray arrays with one row per ray, the table sample with
    DUMP_TABLE_ROWS rows per level."""
    out = tmp_path / "dump"
    r = _run(SMALL + ["--dump-outputs", str(out)])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert all(k in line for k in HEADLINE) and not any(k in line for k in FULL_ONLY)
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["unit"] == "rays/s"
    assert abs(line["value"] - 300 * 1e3 / line["ms_per_step"]) <= 0.01 * line["value"]
    files = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert {"loss", "mse", "table_rows", "z_coarse", "z_fine", "raw_c", "raw_f", "coarse_sigma0",
            "fine_color2"} <= set(files) and len(files) == 17
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 * 10 ** 6
    assert files["raw_f"].shape == (300, 192, 4) and files["z_coarse"].shape == (300, 64)
    assert files["table_rows"].shape == (16, 1 << 16, 2)
    assert abs(float(files["loss"][0]) - line["loss"]) <= 1e-6


@pytest.mark.gpu
def test_full_run_adds_the_other_fields():
    """--full: the same headline plus the launch-time, roofline and sparsity
    fields (the CPU baseline left out here: it takes the oracle's full batch)."""
    r = _run(SMALL + ["--full", "--no-cpu-baseline", "--kernel-steps", "2"])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert all(k in line for k in HEADLINE)
    assert all(k in line for k in FULL_ONLY if k != "cpu_baseline") and "cpu_baseline" not in line
    assert line["kernels"]["render_fwd_ms"] > 0 and line["roofline"]["launch_ms"] > 0

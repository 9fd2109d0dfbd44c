"""GPU test: what a run of bench.py does besides its timed steps.  A plain run prints the result line with the headline
fields and the figures sampled inside the timed region, and none of the legs that take runs of their own; --full adds
those legs to the same line.  Small batch and few steps: the legs are checked for being there, not for their numbers.
(The CPU baseline and the other configurations are --full legs too; they take tens of seconds at any size, so the
--full case here trims them with their own flags.)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "4", "--warmup", "2", "--batch", "256"]
FULL_ONLY = ("configs", "cpu_baseline", "speedup_vs_cpu")


def _bench(*extra):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + list(extra), cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines                    # ONE JSON result line on stdout
    return json.loads(lines[0])


def _check_headline(out):
    assert out["metric"].startswith("utterances/sec fwd+bwd")
    assert out["unit"] == "utterances/s" and out["higher_is_better"] is True and out["dtype"].startswith("f32")
    assert out["steps"] == 4 and out["warmup"] == 2 and out["n_gpus"] == 1
    assert out["ms_per_step"] > 0
    assert abs(out["value"] - 256 / (out["ms_per_step"] * 1e-3)) <= 1e-6 * out["value"]
    # sampled inside the timed region: no run of their own, so both kinds of run carry them
    assert out["roofline"]["avg_launch_ms"] > 0 and out["forward_kernel"]["avg_launch_ms"] > 0
    assert out["roofline_mfma"]["achieved"] > 0


def test_a_plain_run_prints_the_headline_and_runs_no_other_leg(tmp_path):
    out = _bench("--dump-outputs", str(tmp_path / "dump"))
    _check_headline(out)
    assert out["full"] is False
    assert out["graph_replay"] is None and out["ms_per_step_median_of_blocks"] is None
    assert not [k for k in FULL_ONLY if k in out]
    hs = np.load(tmp_path / "dump" / "hs_sample.npy")
    assert hs.shape == (99, 256, 128) and hs.dtype == np.float32 and np.isfinite(hs).all()
    assert np.load(tmp_path / "dump" / "grad_U.npy").shape == (128, 128)


def test_full_adds_the_block_median_and_the_graph_replay_leg():
    out = _bench("--full", "--no-cpu-baseline", "--no-extra-configs")
    _check_headline(out)
    assert out["full"] is True
    assert out["ms_per_step_median_of_blocks"] > 0
    assert "error" not in out["graph_replay"], out["graph_replay"]
    assert out["graph_replay"]["ms_per_step"] > 0 and out["graph_replay"]["steps"] == 4
    assert not [k for k in FULL_ONLY if k in out]   # trimmed by their own flags

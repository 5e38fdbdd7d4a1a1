"""bench.py end to end on the MI355X: a plain run times exactly --steps steps, reports ms_per_step consistently with value,
runs none of the --full measurements, and --dump-outputs writes what its last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    from policy_gradient_asr_amd.model import Seq2Seq
    import bench
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and "for 3 steps" in r.stderr
    assert d["metric"] == bench.METRIC and d["unit"] == "utterances/sec" and d["higher_is_better"] is True and d["dtype"].startswith("f32")
    assert abs(d["value"] - bench.B_PER_GPU / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    for leg in ("long_run", "inputs_resident", "bucketed", "precision_variants", "max_rel_err_vs_fp64", "cpu_baseline"):
        assert leg not in d, leg
    assert d["roofline_gemm"] is None and "leg " not in r.stderr
    arrays = {p.name[:-len(".npy")]: np.load(p) for p in out.iterdir()}
    assert sorted(arrays) == ["grads", "loss", "nll", "params", "reward_greedy", "reward_sampled"]
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= bench.DUMP_LIMIT_BYTES
    assert float(arrays["loss"]) == d["loss"]                              # the loss of the last timed step
    n_params = sum(p.numel() for p in Seq2Seq(bench.V, n_feats=bench.F).parameters())
    assert arrays["params"].shape == arrays["grads"].shape == (n_params,) and np.abs(arrays["grads"]).max() > 0
    assert arrays["nll"].shape == arrays["reward_sampled"].shape == arrays["reward_greedy"].shape == (bench.B_PER_GPU,)

"""GPU: a plain ``bench.py`` run (no ``--full``) times exactly ``--steps`` steps, prints the headline line only, and
``--dump-outputs`` writes the last timed step's outputs, identical from run to run (seeded inputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    # 13 steps after a 4-step warm-up: the timed region starts mid-chunk and crosses a chunk end (PER insert)
    cmd = [sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "13", "--warmup", "4",
           "--envs", "256", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_plain_run_headline_only_and_dump_is_reproducible(tmp_path):
    lines = [_plain_run(tmp_path / d) for d in ("a", "b")]
    for line in lines:
        assert line["full"] is False and line["steps"] == 13 and line["warmup"] == 4 and line["repeats"] == 1
        assert line["unit"] == "agent-env-steps/s" and line["higher_is_better"] is True and line["errors"] == 0
        assert line["ms_per_step"] > 0 and line["ms_per_step_min"] == line["ms_per_step"] == line["ms_per_step_max"]
        assert np.isclose(line["value"], 256 * 8 / (line["ms_per_step"] * 1e-3), rtol=2e-2)   # (ms rounded to 1e-4)
        for moved in ("learner", "train_loop", "cfg1_vdn", "mappo", "offpolicy_qmix", "cfg5_forward", "roofline",
                      "cpu_baseline"):
            assert moved not in line
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"act.npy", "q_taken.npy", "target_max_q.npy", "reward.npy", "done.npy", "next_obs.npy",
            "hidden_behavior.npy", "hidden_target.npy", "per_tree.npy"} <= set(names)
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
        np.testing.assert_array_equal(a, b, err_msg=n)
        total += a.nbytes
    assert total <= 64 * 1000 * 1000
    act, hid = np.load(tmp_path / "a" / "act.npy"), np.load(tmp_path / "a" / "hidden_behavior.npy")
    assert act.shape == (256, 8) and set(np.unique(act)) <= {0.0, 1.0, 2.0, 3.0, 4.0}
    assert hid.shape == (8, 64, 256) and np.abs(hid).max() > 0

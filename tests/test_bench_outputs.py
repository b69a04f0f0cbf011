"""bench.py --dump-outputs: the files a run leaves for comparing two builds.
CPU: dump_outputs on a stand-in model.  GPU: one short plain run of the bench
itself -- the result line's headline keys, --steps honoured, no --full leg in
the line, the dumped arrays finite and float32."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

NAMES = ["losses", "weights", "gradients", "adam_m", "adam_v"]


class StandIn:
    def __init__(self):
        r = np.random.default_rng(0)
        self.w = [r.standard_normal((3, 4)), r.standard_normal(4)]
        self.g = [r.standard_normal((3, 4)).astype(np.float32), r.standard_normal(4).astype(np.float32)]
        self.m, self.v = r.standard_normal(16), r.random(16)

    def get_weights(self):
        return self.w

    def get_gradients(self):
        return self.g

    def get_optimizer_state(self):
        return self.m, self.v, 7


def test_dump_outputs_writes_float32_arrays(tmp_path):
    s = StandIn()
    d = tmp_path / "sub" / "out"
    bench.dump_outputs(str(d), s, np.array([3.0, 2.0], np.float64))
    assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in NAMES)
    got = {n: np.load(d / (n + ".npy"), allow_pickle=False) for n in NAMES}
    assert all(a.dtype == np.float32 for a in got.values())
    np.testing.assert_array_equal(got["losses"], np.float32([3.0, 2.0]))
    np.testing.assert_array_equal(got["weights"], np.concatenate([w.ravel() for w in s.w]).astype(np.float32))
    np.testing.assert_array_equal(got["gradients"], np.concatenate([g.ravel() for g in s.g]))
    np.testing.assert_array_equal(got["adam_m"], s.m.astype(np.float32))
    np.testing.assert_array_equal(got["adam_v"], s.v.astype(np.float32))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--dump-outputs", str(d)], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 2 and out["full"] is False
    assert out["unit"] == "image*samples/s" and out["higher_is_better"] is True and "fp32" in out["dtype"]
    assert out["ms_per_step"] > 0
    # value = sample rows of the 3 timed steps over their time
    assert out["value"] == pytest.approx(bench.B_PER_GPU * bench.K / (out["ms_per_step"] * 1e-3), rel=1e-3)
    for leg in ("nll", "large_batch", "roofline", "cpu_baseline", "train_step_calls", "configs0_train"):
        assert leg not in out
    got = {n: np.load(d / (n + ".npy"), allow_pickle=False) for n in NAMES}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert got["losses"].shape == (3,)
    assert out["loss"] == pytest.approx(float(got["losses"][-1]), abs=1e-3)
    assert got["weights"].shape == got["gradients"].shape == got["adam_m"].shape == got["adam_v"].shape == (bench.N_PARAMS,)
    assert np.abs(got["gradients"]).max() > 0 and (got["adam_v"] >= 0).all()

"""bench.py's plain / --full split and --dump-outputs, in process on a reduced cfg 2 shape (64^2, K = 20).

A plain run prints the headline figure and nothing that takes a run of its own; --full adds the forward /
backward split, the per-kernel times and the roofline.  --dump-outputs writes the last timed step's arrays
(float32), and two runs with the same arguments write the same values: the last step starts from the
initial pose and Adam state (Workload.reset_state), its Philox key is that of its ordinal."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import pertrenderer_amd as pa

pytestmark = pytest.mark.gpu

SHAPE = ["--image-size", "64", "--faces-per-pixel", "20"]
MOVED = ("ms_forward", "ms_backward", "kernels", "roofline", "roofline_dense", "cpu_baseline", "strong_scaling")
ARRAYS = {"image": (1, 64, 64, 4), "loss": (1,), "log_rot": (1, 3), "grad_log_rot": (1, 3), "grad_sigma": (1,),
          "grad_gamma": (1,), "grad_alpha": (1,)}


def _bench(argv, monkeypatch, capsys):
    """bench.main() with `argv`; the process-wide state it sets (torch's seeds, the DeviceSeed routing) is
    put back."""
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1"] + argv)
    cpu_state, gpu_state = torch.random.get_rng_state(), torch.cuda.get_rng_state()
    try:
        bench.main()
    finally:
        pa.noise.use_device_seed(None)
        torch.random.set_rng_state(cpu_state)
        torch.cuda.set_rng_state(gpu_state)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.parametrize("mode", ["graph", "eager"])
def test_plain_run_dumps_repeatable_outputs(mode, tmp_path, monkeypatch, capsys):
    runs = []
    for name in ("a", "b"):
        d = str(tmp_path / name)
        line = _bench(["--steps", "4", "--warmup", "2", "--mode", mode, "--dump-outputs", d] + SHAPE, monkeypatch, capsys)
        assert line["steps"] == 4 and line["warmup"] == 2 and line["config"]["execution"] == mode
        assert line["value"] > 0 and line["ms_per_step"] > 0 and line["full"] is False
        assert abs(line["value"] * line["ms_per_step"] / 1e3 - 1.0) < 1e-2  # one frame per step
        assert not [k for k in MOVED if k in line], line.keys()
        assert {k: tuple(v) for k, v in line["outputs"]["arrays"].items()} == ARRAYS
        arrs = {k: np.load(os.path.join(d, k + ".npy")) for k in ARRAYS}
        for k, a in arrs.items():
            assert a.dtype == np.float32 and a.shape == ARRAYS[k] and np.isfinite(a).all(), k
        assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
        assert arrs["image"][..., :3].max() > 0 and np.abs(arrs["grad_log_rot"]).sum() > 0
        runs.append(arrs)
    a, b = runs
    # the forward and the loss sum in a fixed order; one Adam step from zero moments moves each pose
    # component by lr * g / (|g| + eps): a few ulp.  A flipped perturbed-argmax winner would be O(1)
    for k in ("image", "loss", "log_rot"):
        np.testing.assert_allclose(a[k], b[k], rtol=0, atol=1e-6, err_msg=k)
    # the backward scatters with float atomics: fp32 summation order, the suite's 1e-4 bar for such sums
    for k in ("grad_log_rot", "grad_sigma", "grad_gamma", "grad_alpha"):
        np.testing.assert_allclose(a[k], b[k], rtol=1e-4, atol=1e-4 * np.abs(b[k]).max(), err_msg=k)


def test_full_run_adds_the_kernel_report(monkeypatch, capsys):
    line = _bench(["--steps", "4", "--warmup", "2", "--full", "--no-cpu-baseline", "--no-dense"] + SHAPE,
                  monkeypatch, capsys)
    assert line["full"] is True and line["steps"] == 4 and line["ms_per_step"] > 0
    assert line["ms_forward"] > 0 and line["ms_backward"] > 0
    assert {"rast_fwd", "rast_bwd", "blend_fwd", "blend_bwd"} <= set(line["kernels"])
    assert line["roofline"]["kernel"] and 0 < line["roofline"]["frac"] < 1
    assert "outputs" not in line

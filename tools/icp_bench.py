"""Timing of iterative_closest_point (renderer/alignment.py) on the GPU; prints one JSON line.

    python tools/icp_bench.py [--clouds 4] [--points 5000] [--target 20000] [--iterations 20]
                              [--repeats 5] [--steps 5] [--out FILE]

One case: `clouds` clouds of `points` points (a noisy, shifted, rotated subset of the target, the
scene recipe of tests/icp_cases.py) against `target` points each, `iterations` ICP iterations with
relative_rmse_thr = -1 so that the count is fixed, on the native kernels and on the torch composition
(NATIVE_ICP off) in the same process: kernels and copies of one call, the native kernels' device
times one by one (from a torch.profiler trace), ms per call, and the largest difference of the two
results.

Every timing is a host clock around `steps` calls that end in a device synchronise, after a warm-up
of the same shape, repeated `repeats` times: the median, the minimum and the maximum are reported
(the composition runs one call per window)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from meshloss_bench import count_launches, kernel_times, spread, timed  # noqa: E402
from pertrenderer_amd.renderer import alignment as AL  # noqa: E402


def scene(clouds, points, target, seed=0):
    rng = np.random.RandomState(seed)
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(12.0)
    R = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K
    Y = rng.uniform(-1, 1, (clouds, target, 3))
    X = np.stack([(Y[n][rng.permutation(target)[:points]] + 0.01 * rng.randn(points, 3) - 0.03) @ R for n in range(clouds)])
    return torch.from_numpy(X.astype(np.float32)), torch.from_numpy(Y.astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=4)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--target", type=int, default=20000)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("icp_bench needs a ROCm device: a CPU run gives no timing")
    device = torch.device("cuda:0")
    X, Y = (t.to(device) for t in scene(args.clouds, args.points, args.target))
    out = {}

    def call():
        out["sol"] = AL.iterative_closest_point(X, Y, max_iterations=args.iterations, relative_rmse_thr=-1.0)

    res = dict(device=torch.cuda.get_device_name(0), clouds=args.clouds, points=args.points, target=args.target,
               iterations=args.iterations, check_every=int(os.environ.get("PR_ICP_CHECK_EVERY", "8")))
    sols = {}
    for name, native, steps in (("native", True, args.steps), ("composition", False, 1)):
        AL.NATIVE_ICP = native
        try:
            for _ in range(2):
                call()
            row = count_launches(call)
            total, per = kernel_times(call)
            row["kernel_us"] = total
            if native:
                row["native_kernels_us"] = {k: v for k, v in per.items() if k.startswith(("icp_", "centroid_"))}
            row["ms"] = spread(timed(call, steps, args.repeats))
            assert len(out["sol"].t_history) == args.iterations and out["sol"].converged is False
            sols[name] = out["sol"]
            res[name] = row
        finally:
            AL.NATIVE_ICP = True
    a, b = sols["native"], sols["composition"]
    res["max_abs_difference"] = dict(R=float((a.RTs.R - b.RTs.R).abs().max()), T=float((a.RTs.T - b.RTs.T).abs().max()),
                                     rmse=float((a.rmse - b.rmse).abs().max()), Xt=float((a.Xt - b.Xt).abs().max()))
    res["rmse"] = [round(v, 6) for v in a.rmse.tolist()]
    res["speedup"] = round(res["composition"]["ms"]["median"] / res["native"]["ms"]["median"], 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

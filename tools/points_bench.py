"""Timing of the point-cloud renderer (renderer/points.py) on the GPU; prints one JSON line.

    python tools/points_bench.py [--clouds 4] [--points 20000] [--size 256] [--k 8] [--radius 0.02]
                                 [--repeats 5] [--steps 20] [--out FILE]

One case: forward + backward of PointsRenderer (FoVPerspectiveCameras, AlphaCompositor) on `clouds`
clouds of `points` coloured points each on a unit sphere, to the world points and the features,
on the native kernels and on the torch composition (NATIVE_POINTS off) in the same process: kernels
and copies of one call, the native kernels' device times one by one (from a torch.profiler trace)
and ms per call.  The native step is also replayed from a captured graph.

Every timing is a host clock around `steps` calls that end in a device synchronise, after a warm-up
of the same shape, repeated `repeats` times: the median, the minimum and the maximum are reported
(the composition, seconds per call, runs `steps` / 10 calls per window)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from meshloss_bench import count_launches, kernel_times, spread, timed  # noqa: E402
from pertrenderer_amd.renderer import (AlphaCompositor, FoVPerspectiveCameras, Pointclouds,  # noqa: E402
                                       PointsRasterizationSettings, PointsRasterizer, PointsRenderer,
                                       look_at_view_transform)
from pertrenderer_amd.renderer import points as PT  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=4)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--radius", type=float, default=0.02)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("points_bench needs a ROCm device: a CPU run gives no timing")
    device = torch.device("cuda:0")
    g = torch.Generator().manual_seed(args.points)
    pts = torch.nn.functional.normalize(torch.randn((args.clouds, args.points, 3), generator=g), dim=2).to(device)
    cols = (0.5 + 0.5 * pts).contiguous()
    pts.requires_grad_(True)
    cols.requires_grad_(True)
    R, T = look_at_view_transform(2.7, 20.0, 40.0, device=device)
    rs = PointsRasterizationSettings(image_size=args.size, radius=args.radius, points_per_pixel=args.k)
    renderer = PointsRenderer(PointsRasterizer(FoVPerspectiveCameras(R=R, T=T, device=device), rs), AlphaCompositor((0.0, 0.0, 0.0)))
    target = torch.rand((args.clouds, args.size, args.size, 3), generator=g).to(device)

    def call():
        pts.grad = cols.grad = None
        ((renderer(Pointclouds(pts, features=cols)) - target) ** 2).sum().backward()

    res = dict(device=torch.cuda.get_device_name(0), clouds=args.clouds, points=args.points, size=args.size, K=args.k,
               radius=args.radius)
    grads = {}
    for name, native, steps in (("native", True, args.steps), ("composition", False, max(args.steps // 10, 1))):
        PT.NATIVE_POINTS = native
        try:
            for _ in range(2):
                call()
            row = count_launches(call)
            total, per = kernel_times(call)
            row["kernel_us"] = total
            if native:
                row["native_kernels_us"] = {k: v for k, v in per.items() if k.startswith("points_")}
            row["ms"] = spread(timed(call, steps, args.repeats))
            grads[name] = (pts.grad.clone(), cols.grad.clone())
            res[name] = row
        finally:
            PT.NATIVE_POINTS = True
    res["max_abs_grad_difference"] = [float((a - b).abs().max()) for a, b in zip(grads["native"], grads["composition"])]
    # the native step replayed from a captured graph
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    pts.grad = cols.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(3):
        graph.replay()
    res["native"]["captured_ms"] = spread(timed(graph.replay, args.steps, args.repeats))
    res["speedup"] = round(res["composition"]["ms"]["median"] / res["native"]["ms"]["median"], 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

"""Timing of the mesh-loss module (renderer/loss.py) on the GPU; prints one JSON line.

    python tools/meshloss_bench.py [--repeats 7] [--steps 200] [--out FILE]

(a) "regulariser_step": one deformation step on tests/golden/sphere_642.obj, forward + backward +
    in-place SGD update of mesh_laplacian_smoothing("cot") + mesh_edge_loss + mesh_normal_consistency
    (DESIGN.md "Mesh regularisers", "Launch count"): kernels and copies of one step under
    torch.profiler, ms/step eager and replayed from a captured graph.
(b) "chamfer": chamfer_distance forward + backward at N = 1, P = Q = 5000 and 20000 (uniform clouds,
    seeded): ms per call and peak allocated memory above the inputs.

    python tools/meshloss_bench.py --sweep [--out FILE]

"chamfer_sweep": chamfer_distance forward alone and forward + backward at 5000 x 5000, 20000 x 20000
and 642 x 20000 points over PR_CHAMFER_SPLITS (the library's own choice, then 1 ... 64 ranges), for
the library that is loaded.  The LDS tile is a compile-time constant: build variants with
`python -m pertrenderer_amd.build_native --out pertrenderer_amd/libpertrender_tile256.so -D PR_CHAMFER_TILE=256`
and select one with PR_NATIVE_LIB; the line names the library it timed
(profiles/meshloss_native/chamfer_sweep_tile*.json).

Every timing is a host clock around `steps` calls that end in a device synchronise, after a
warm-up of the same shape, repeated `repeats` times: the median, the minimum and the maximum are
reported.  It uses the module's public functions only, so the same file runs on any commit that
has them (compare a branch with its parent on the same machine, in the same session)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pertrenderer_amd.renderer import Meshes, load_obj  # noqa: E402
from pertrenderer_amd.renderer import loss as L  # noqa: E402


def spread(ms):
    return dict(median=round(statistics.median(ms), 5), min=round(min(ms), 5), max=round(max(ms), 5), repeats=len(ms))


def timed(fn, steps, repeats):
    """ms per call: `repeats` windows of `steps` calls, each ended by a synchronise."""
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / steps)
    return out


def count_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    with tempfile.TemporaryDirectory() as td:
        tr = os.path.join(td, "t.json")
        prof.export_chrome_trace(tr)
        ev = [e for e in json.load(open(tr))["traceEvents"] if e.get("ph") == "X"]
    return dict(kernels=sum(e.get("cat") == "kernel" for e in ev),
                copies=sum(e.get("cat") in ("gpu_memcpy", "gpu_memset") for e in ev))


def regulariser_step(device, steps, repeats):
    v, f, _ = load_obj(os.path.join(ROOT, "tests", "golden", "sphere_642.obj"))
    base = Meshes([(v.float() * torch.tensor([1.0, 0.7, 1.3])).to(device)], [f.verts_idx.to(device)])
    start = (0.02 * torch.randn(v.shape, generator=torch.Generator().manual_seed(3))).to(device)

    def step(deform):
        mesh = base.offset_verts(deform)
        loss = L.mesh_laplacian_smoothing(mesh, "cot") + L.mesh_edge_loss(mesh) + L.mesh_normal_consistency(mesh)
        deform.grad = None
        loss.backward()
        with torch.no_grad():
            deform.add_(deform.grad, alpha=-1e-4)
        return loss

    d = start.clone().requires_grad_(True)
    for _ in range(10):
        step(d)
    out = count_launches(lambda: step(d))
    out["eager_ms"] = spread(timed(lambda: step(d), steps, repeats))

    d = start.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(d)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(d)
    for _ in range(10):
        graph.replay()
    out["captured_ms"] = spread(timed(graph.replay, steps, repeats))
    return out


def chamfer(device, P, steps, repeats):
    g = torch.Generator().manual_seed(P)
    x = torch.rand((1, P, 3), generator=g).to(device).requires_grad_(True)
    y = torch.rand((1, P, 3), generator=g).to(device).requires_grad_(True)

    def call():
        x.grad = y.grad = None
        L.chamfer_distance(x, y)[0].backward()

    for _ in range(3):
        call()
    torch.cuda.synchronize()
    x.grad = y.grad = None
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    call()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    out = count_launches(call)
    out.update(P=P, Q=P, ms=spread(timed(call, steps, repeats)), peak_bytes=int(peak))
    return out


def chamfer_sweep(device, steps, repeats):
    from pertrenderer_amd import _native as nat
    out = dict(library=os.path.basename(nat.LIB_PATH), cases=[])
    keep = os.environ.pop("PR_CHAMFER_SPLITS", None)
    for P, Q in ((5000, 5000), (20000, 20000), (642, 20000)):
        g = torch.Generator().manual_seed(P)
        x = torch.rand((1, P, 3), generator=g).to(device).requires_grad_(True)
        y = torch.rand((1, Q, 3), generator=g).to(device).requires_grad_(True)

        def fwd_bwd():
            x.grad = y.grad = None
            L.chamfer_distance(x, y)[0].backward()

        def fwd():
            with torch.no_grad():
                L.chamfer_distance(x, y)

        for s in ("default", "1", "2", "5", "10", "20", "40", "64"):
            os.environ.pop("PR_CHAMFER_SPLITS", None)
            if s != "default":
                os.environ["PR_CHAMFER_SPLITS"] = s  # read by the library on every call
            row = dict(P=P, Q=Q, splits=s)
            for name, fn in (("fwd_ms", fwd), ("fwd_bwd_ms", fwd_bwd)):
                for _ in range(5):
                    fn()
                row[name] = spread(timed(fn, steps, repeats))
            out["cases"].append(row)
    os.environ.pop("PR_CHAMFER_SPLITS", None)
    if keep is not None:
        os.environ["PR_CHAMFER_SPLITS"] = keep
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out")
    ap.add_argument("--sweep", action="store_true", help="chamfer over PR_CHAMFER_SPLITS instead of (a) and (b)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meshloss_bench needs a ROCm device: a CPU run gives no timing")
    device = torch.device("cuda:0")
    if args.sweep:
        res = dict(device=torch.cuda.get_device_name(0),
                   chamfer_sweep=chamfer_sweep(device, max(args.steps // 4, 10), min(args.repeats, 5)))
    else:
        res = _default_run(device, args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


def _default_run(device, args):
    return dict(device=torch.cuda.get_device_name(0), native_meshloss=L.NATIVE_MESHLOSS,
                native_chamfer=hasattr(L, "_ChamferFn"),
                regulariser_step=regulariser_step(device, args.steps, args.repeats),
                chamfer=[chamfer(device, 5000, max(args.steps // 4, 10), args.repeats),
                         chamfer(device, 20000, max(args.steps // 20, 5), args.repeats)])


if __name__ == "__main__":
    main()

"""Timing of the mesh-loss module (renderer/loss.py) on the GPU; prints one JSON line.

    python tools/meshloss_bench.py [--repeats 7] [--steps 200] [--out FILE]

(a) "regulariser_step": one deformation step on tests/golden/sphere_642.obj, forward + backward +
    in-place SGD update of mesh_laplacian_smoothing("cot") + mesh_edge_loss + mesh_normal_consistency
    (DESIGN.md "Mesh regularisers", "Launch count"): kernels and copies of one step under
    torch.profiler, ms/step eager and replayed from a captured graph.
(b) "chamfer": chamfer_distance forward + backward at N = 1, P = Q = 5000 and 20000 (uniform clouds,
    seeded): ms per call and peak allocated memory above the inputs.

(c) "sampling": sample_points_from_meshes with normals, forward + backward, and (d)
    "deformation_step": sample -> chamfer_distance with normals + mesh_edge_loss +
    mesh_normal_consistency + mesh_laplacian_smoothing -> backward -> SGD update, at 4 x sphere_642
    with S = 5000 and at the 3x subdivided sphere (81 920 faces) with S = 10 000: kernels and copies
    of one call, ms per call on the native kernels and on the torch composition
    (NATIVE_MESHLOSS off) in the same process, and the native step replayed from a captured graph
    with a DeviceSeed.  `--sampling` runs (c) and (d) alone.

(e) "point_mesh": point_mesh_face_distance and point_mesh_edge_distance, forward + backward to the
    vertices and the points, 4 x sphere_642 against 5000 points each: kernels and copies of one call,
    the device time of its kernels (their durations in a torch.profiler trace, summed; the native
    kernels also one by one) and ms per call, on the native kernels and on the torch composition.
    `--pointmesh` runs (e) alone.

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


def kernel_times(fn):
    """(total device time of fn()'s kernels in us, {kernel name: us}) from a torch.profiler trace."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    with tempfile.TemporaryDirectory() as td:
        tr = os.path.join(td, "t.json")
        prof.export_chrome_trace(tr)
        ev = [e for e in json.load(open(tr))["traceEvents"] if e.get("ph") == "X" and e.get("cat") == "kernel"]
    per = {}
    for e in ev:
        name = e["name"].replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].split("::")[-1].split(" ")[-1]
        per[name] = round(per.get(name, 0.0) + float(e["dur"]), 2)
    return round(sum(float(e["dur"]) for e in ev), 2), per


def point_mesh(device, steps, repeats):
    """point_mesh_face_distance / point_mesh_edge_distance, forward + backward, 4 x sphere_642 against
    5000 points each (on a sphere a little larger than the meshes)."""
    from pertrenderer_amd.renderer import Pointclouds
    _, src, S = _sampling_shapes(device)[0]
    N = len(src)
    g = torch.Generator().manual_seed(S)
    pts = (torch.nn.functional.normalize(torch.randn((N, S, 3), generator=g), dim=2) * 1.1 + 0.05).to(device)
    pts.requires_grad_(True)
    cloud = Pointclouds(pts)
    d = torch.zeros((src.verts_packed().shape[0], 3), device=device, requires_grad=True)
    rows = []
    for name, fn in (("faces", L.point_mesh_face_distance), ("edges", L.point_mesh_edge_distance)):
        def call():
            d.grad = pts.grad = None
            fn(src.offset_verts(d), cloud).backward()

        def measure():
            for _ in range(3):
                call()
            row = count_launches(call)
            total, per = kernel_times(call)
            row["kernel_us"] = total
            if L.NATIVE_MESHLOSS:
                row["native_kernels_us"] = {k: v for k, v in per.items()
                                            if k.startswith(("prim_", "point", "vert_gather"))}
            row["ms"] = spread(timed(call, steps, repeats))
            return row

        rows.append(dict(prims=name, shape="4xsphere_642", points_per_cloud=S, **_both_paths(measure)))
    return rows


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


def _sampling_shapes(device):
    """(name, source Meshes, S): 4 x sphere_642 at S = 5000 and fine_sphere(3) (81 920 faces) at S = 10 000."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import meshgen
    v0, f0 = meshgen.load_sphere()
    v3, f3 = meshgen.fine_sphere(3)
    scale = torch.tensor([1.0, 0.7, 1.3])
    small = Meshes([(torch.tensor(v0) * scale).to(device) for _ in range(4)], [torch.tensor(f0).to(device) for _ in range(4)])
    fine = Meshes([(torch.tensor(v3) * scale).to(device)], [torch.tensor(f3).to(device)])
    return [("4xsphere_642", small, 5000), ("fine_sphere3", fine, 10000)]


def _both_paths(fn):
    """fn() under the native kernels and under the torch composition (NATIVE_MESHLOSS off)."""
    out = {}
    keep = L.NATIVE_MESHLOSS
    for name, native in (("native", True), ("composition", False)):
        L.NATIVE_MESHLOSS = native
        try:
            out[name] = fn()
        finally:
            L.NATIVE_MESHLOSS = keep
    return out


def sampling(device, steps, repeats):
    """sample_points_from_meshes with normals, forward + backward to the vertices."""
    from pertrenderer_amd.renderer import sample_points_from_meshes
    rows = []
    for name, src, S in _sampling_shapes(device):
        d = torch.zeros((src.verts_packed().shape[0], 3), device=device, requires_grad=True)

        def call():
            d.grad = None
            p, n = sample_points_from_meshes(src.offset_verts(d), S, return_normals=True)
            (p.sum() + n[..., 0].sum()).backward()

        def measure():
            for _ in range(5):
                call()
            row = count_launches(call)
            row["ms"] = spread(timed(call, steps, repeats))
            return row

        rows.append(dict(shape=name, S=S, faces=int(src.faces_packed().shape[0]), **_both_paths(measure)))
    return rows


def deformation_step(device, steps, repeats):
    """sample -> Chamfer with normals + edge + normal consistency + Laplacian -> backward: ms per step
    eager on both paths, and replayed from a captured graph with a DeviceSeed on the native path."""
    from pertrenderer_amd import noise
    from pertrenderer_amd.renderer import sample_points_from_meshes
    rows = []
    for name, src, S in _sampling_shapes(device):
        N = len(src)
        g = torch.Generator().manual_seed(S)
        tgt = torch.nn.functional.normalize(torch.randn((N, S, 3), generator=g), dim=2).to(device)
        tgt_n = tgt.clone()
        tgt = tgt * 1.1 + 0.05
        start = (0.02 * torch.randn(src.verts_packed().shape, generator=g)).to(device)

        def step(d):
            m = src.offset_verts(d)
            p, n = sample_points_from_meshes(m, S, return_normals=True)
            cd, cn = L.chamfer_distance(p, tgt, x_normals=n, y_normals=tgt_n)
            loss = (cd + 0.1 * cn + L.mesh_edge_loss(m) + 0.01 * L.mesh_normal_consistency(m)
                    + 0.1 * L.mesh_laplacian_smoothing(m, "uniform"))
            d.grad = None
            loss.backward()
            with torch.no_grad():
                d.add_(d.grad, alpha=-1e-4)

        def measure():
            d = start.clone().requires_grad_(True)
            for _ in range(5):
                step(d)
            row = count_launches(lambda: step(d))
            row["eager_ms"] = spread(timed(lambda: step(d), steps, repeats))
            if not L.NATIVE_MESHLOSS:  # the captured step is the native path's claim
                return row
            ds = noise.DeviceSeed(device, seed=1)
            noise.use_device_seed(ds)
            try:
                d = start.clone().requires_grad_(True)
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    ds.advance()
                    step(d)
                torch.cuda.current_stream().wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    ds.advance()
                    step(d)
                for _ in range(5):
                    graph.replay()
                row["captured_ms"] = spread(timed(graph.replay, steps, repeats))
            finally:
                noise.use_device_seed(None)
            return row

        rows.append(dict(shape=name, S=S, faces=int(src.faces_packed().shape[0]), **_both_paths(measure)))
    return rows


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
    ap.add_argument("--sampling", action="store_true", help="(c) and (d) only")
    ap.add_argument("--pointmesh", action="store_true", help="(e) only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meshloss_bench needs a ROCm device: a CPU run gives no timing")
    device = torch.device("cuda:0")
    if args.sweep:
        res = dict(device=torch.cuda.get_device_name(0),
                   chamfer_sweep=chamfer_sweep(device, max(args.steps // 4, 10), min(args.repeats, 5)))
    elif args.sampling:
        res = dict(device=torch.cuda.get_device_name(0), **_sampling_run(device, args))
    elif args.pointmesh:
        res = dict(device=torch.cuda.get_device_name(0), point_mesh=point_mesh(device, max(args.steps // 10, 5), args.repeats))
    else:
        res = _default_run(device, args)
        res.update(_sampling_run(device, args))
        res["point_mesh"] = point_mesh(device, max(args.steps // 10, 5), args.repeats)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


def _sampling_run(device, args):
    return dict(sampling=sampling(device, max(args.steps // 4, 10), args.repeats),
                deformation_step=deformation_step(device, max(args.steps // 10, 5), args.repeats))


def _default_run(device, args):
    return dict(device=torch.cuda.get_device_name(0), native_meshloss=L.NATIVE_MESHLOSS,
                native_chamfer=hasattr(L, "_ChamferFn"),
                regulariser_step=regulariser_step(device, args.steps, args.repeats),
                chamfer=[chamfer(device, 5000, max(args.steps // 4, 10), args.repeats),
                         chamfer(device, 20000, max(args.steps // 20, 5), args.repeats)])


if __name__ == "__main__":
    main()

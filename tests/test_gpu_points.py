"""Native point-cloud renderer (csrc/pr_points.hip behind renderer/points.py) on the GPU against the
float64 restatement of points_cases.py: fragments, the three compositors' images and every
gradient under random cotangents; against the torch composition on the device; bitwise
reproducibility; the K cap; an all-behind cloud; PointsRenderer end to end; capture in a HIP graph.

Every scene runs with the default chunk size and with PR_POINTS_CHUNK=16 (the 70-point clouds then
cross four chunk boundaries, the 1000-point clouds sixty-two).

Rules.  idx exact (the scenes keep float32's selection equal to float64's, and the planted ties
resolve to the lowest index), zbuf bitwise, dists and images at conftest.assert_close's defaults.
Gradients: max-abs over max-abs (points_cases.grad_error) against float64 at the kernel's own
indices, bounded by 4x the float32 composition's own error on that case, floored at 1e-5 (the rule
of test_gpu_point_mesh.py); points_cases.references asserts that the composition's error stays
<= 2e-5, so the rule cannot loosen.  One exception to the plain metric (points_cases.grad_scale):
in one_k1 every pixel has one slot, the norm-weighted d alphas cancels to 4e-16 in float64 and has
no magnitude to divide by; there, and only there, the error is taken against the size of the
cancelling terms (the weighted mode's d alphas).

Measured on an MI355X (float32 composition error / native error, the largest over all scenes and both
chunk settings): d points 1.64e-07 / 1.64e-07 (one_k1); alpha d alphas 1.47e-07 / 1.47e-07, d features
1.60e-07 / 1.15e-07 (c1000_k50); norm d alphas 1.29e-06 / 6.53e-07 (empty_k8; the composition's own
largest is 5.38e-06 on per_point_k8, native 1.58e-07 there), d features 1.68e-07 / 1.37e-07; weighted
d alphas 1.20e-07 / 1.20e-07, d features 1.65e-07 / 1.35e-07; PointsRenderer
d projected points 1.67e-07 / 1.67e-07, d features 1.40e-07 / 1.40e-07.  Everything is below the
1e-5 floor."""
import os

import pytest
import torch

import points_cases as C
from conftest import ROOT, assert_close
from pertrenderer_amd import _native as nat
from pertrenderer_amd.renderer import (AlphaCompositor, FoVPerspectiveCameras, Meshes, NormWeightedCompositor,
                                       Pointclouds, PointsRasterizationSettings, PointsRasterizer, PointsRenderer,
                                       load_obj, look_at_view_transform, rasterize_points, sample_points_from_meshes)
from pertrenderer_amd.renderer import points as PT

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[None, "16"], ids=["chunk-default", "chunk-16"])
def chunk(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("PR_POINTS_CHUNK", raising=False)
    else:
        monkeypatch.setenv("PR_POINTS_CHUNK", request.param)
    return request.param


def _run(name, device, native=True):
    """Everything one scene produces: fragments, d points, and per mode the image, d alphas, d features."""
    s, ref = C.scene(name), C.references(name)
    keep = PT.NATIVE_POINTS
    PT.NATIVE_POINTS = native
    try:
        clouds = [c.to(device).requires_grad_(True) for c in s["clouds"]]
        rad = s["radius"].to(device) if torch.is_tensor(s["radius"]) else s["radius"]
        idx, zbuf, dists = rasterize_points(Pointclouds(clouds), (s["H"], s["W"]), rad, s["K"])
        loss = (zbuf * ref["cot_z"].float().to(device)).sum() + (dists * ref["cot_d"].float().to(device)).sum()
        gp = torch.autograd.grad(loss, clouds, allow_unused=True)
        out = dict(idx=idx, zbuf=zbuf.detach(), dists=dists.detach(),
                   d_points=torch.cat([torch.zeros_like(c) if g is None else g for g, c in zip(gp, clouds)]))
        feats = torch.cat(s["features"]).to(device)
        for m in C.MODES:
            a, f = ref["alphas"].to(device).requires_grad_(True), feats.clone().requires_grad_(True)
            img = PT._composite_rows(idx, a, f, PT._MODES[m])
            out[f"image_{m}"] = img.detach()
            out[f"d_alphas_{m}"], out[f"d_features_{m}"] = torch.autograd.grad((img * ref["cot_img"].float().to(device)).sum(), (a, f))
    finally:
        PT.NATIVE_POINTS = keep
    return out


@pytest.mark.parametrize("name", list(C.SCENES))
def test_native_matches_float64(name, chunk, device):
    ref = C.references(name)
    got = _run(name, device)
    assert got["idx"].dtype == torch.int64 and got["zbuf"].dtype == got["dists"].dtype == torch.float32
    assert torch.equal(got["idx"].cpu(), ref["idx"]), "selection (or a planted tie) differs from float64"
    assert torch.equal(got["zbuf"].cpu().double(), ref["zbuf"]), "zbuf is not the chosen z bit for bit"
    assert_close(got["dists"], ref["dists"], name="dists")
    for m in C.MODES:
        assert_close(got[f"image_{m}"], ref[f"image_{m}"], name=f"image {m}")
    err = {k: C.grad_error(k, got[k], ref) for k in C.GRAD_KEYS}
    print(f"{name} chunk={chunk}: gradient error composition(fp32) / native: "
          + ", ".join(f"{k} {ref['err32'][k]:.2e} / {err[k]:.2e}" for k in C.GRAD_KEYS))
    for k in C.GRAD_KEYS:
        assert err[k] <= max(4.0 * ref["err32"][k], 1e-5), (k, err[k], ref["err32"][k])


def test_planted_ties_resolve_to_the_lowest_index(chunk, device):
    idx = _run("c70_k8", device)["idx"].cpu()
    first, second = C.PLANT_DUP
    pos = (idx == second).nonzero()
    assert len(pos) and (pos[:, 3] > 0).all()
    assert (idx[pos[:, 0], pos[:, 1], pos[:, 2], pos[:, 3] - 1] == first).all()
    lo, hi = C.PLANT_EQUAL_Z
    both = ((idx == lo).any(-1) & (idx == hi).any(-1)).nonzero()
    assert len(both)
    for n, r, c in both.tolist():
        row = idx[n, r, c].tolist()
        assert row.index(lo) + 1 == row.index(hi)
    for p in C.PLANT_BEHIND + C.PLANT_OUTSIDE + (C.PLANT_NAN,):
        assert not (idx == p).any(), p


@pytest.mark.parametrize("name", ["c70_k50", "batch2_k8", "per_point_k8"])
def test_native_calls_are_bitwise_reproducible(name, chunk, device):
    a, b = _run(name, device), _run(name, device)
    assert all(torch.equal(a[k], b[k]) for k in a), [k for k in a if not torch.equal(a[k], b[k])]


@pytest.mark.parametrize("name", ["c70_k8", "c1000_k50", "empty_k8", "per_point_k8"])
def test_native_matches_torch_composition(name, chunk, device):
    """Both are float32 statements of the same formulas.  The fragments are equal bit for bit (the
    exact test and d2 are one float32 expression without contraction on either path); images and
    gradients are each within the rule above of float64, so against each other twice that."""
    ref = C.references(name)
    a, b = _run(name, device), _run(name, device, native=False)
    assert torch.equal(a["idx"], b["idx"]) and torch.equal(a["zbuf"], b["zbuf"]) and torch.equal(a["dists"], b["dists"])
    for m in C.MODES:
        assert_close(a[f"image_{m}"], b[f"image_{m}"], name=f"image {m}")
    for k in C.GRAD_KEYS:
        assert (a[k] - b[k]).abs().max().item() / C.grad_scale(k, ref) <= max(8.0 * ref["err32"][k], 2e-5), k


@pytest.mark.parametrize("K", [16, 17])
def test_fragments_on_both_sides_of_the_tile_switch(K, chunk, device):
    """K = 16 is the last size of the 16 x 16 tiles, K = 17 the first of the 8 x 8 ones: the same
    fragments as the composition, bit for bit (the 1000-point cloud fills more than 17 slots)."""
    s = C.scene("c1000_k50")
    pc = Pointclouds([c.to(device) for c in s["clouds"]])
    a = rasterize_points(pc, (s["H"], s["W"]), s["radius"], K)
    PT.NATIVE_POINTS = False
    try:
        b = rasterize_points(pc, (s["H"], s["W"]), s["radius"], K)
    finally:
        PT.NATIVE_POINTS = True
    assert (a[0][..., K - 1] >= 0).any() and all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.equal(a[0].cpu(), C.references("c1000_k50")["idx"][..., :K])


def test_k_above_the_native_cap_takes_the_composition(device, monkeypatch):
    s = C.scene("c70_k50")
    pc = Pointclouds([c.to(device) for c in s["clouds"]])
    at_cap = rasterize_points(pc, (s["H"], s["W"]), s["radius"], PT.MAX_K)  # native
    calls = []
    real = nat.call
    monkeypatch.setattr(nat, "call", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])
    over = rasterize_points(pc, (s["H"], s["W"]), s["radius"], PT.MAX_K + 1)
    assert not [c for c in calls if c.startswith("pr_points")]
    assert tuple(over[0].shape)[-1] == PT.MAX_K + 1 and PT.MAX_K >= 64
    # 70 points: slot 64 exists only where more than 64 candidates do; the first 64 slots are the native ones
    assert all(torch.equal(o[..., :PT.MAX_K], n) for o, n in zip(over, at_cap))
    rasterize_points(pc, (s["H"], s["W"]), s["radius"], PT.MAX_K)
    assert calls == ["pr_points_rast_fwd"]
    with pytest.raises(nat.NativeError):
        PT._RastFn.apply(s["clouds"][0], torch.zeros(1, dtype=torch.int64), torch.ones(1, dtype=torch.int64), None, 0.1, 8, 8, 2,
                         PT._FragmentCSR(70))


def test_an_all_behind_cloud_gives_empty_fragments_and_the_background(device):
    g = torch.Generator().manual_seed(2)
    pts = torch.rand((2, 40, 3), generator=g) * 2 - 1
    pts[0, :, 2] = -pts[0, :, 2].abs() - 0.1  # cloud 0: all behind
    pts[1, :, 2] = pts[1, :, 2].abs() + 0.5
    feats = torch.rand((2, 40, 3), generator=g)
    bg = (0.25, 0.5, 0.75)
    for comp in (AlphaCompositor(background_color=bg), NormWeightedCompositor(background_color=bg)):
        p, f = pts.to(device).requires_grad_(True), feats.to(device).requires_grad_(True)
        pc = Pointclouds(p, features=f)
        idx, zbuf, dists = rasterize_points(pc, 16, 0.3, 4)
        assert (idx[0] == -1).all() and (zbuf[0] == -1).all() and (dists[0] == -1).all() and (idx[1] >= 0).any()
        img = comp._rows(idx, 1 - dists / 0.09, pc.features_packed())
        assert torch.equal(img[0].cpu(), torch.tensor(bg).expand(16, 16, 3))
        gp, gf = torch.autograd.grad(img.sum(), (p, f))
        assert not gp[0].any() and not gf[0].any() and gp[1].any() and gf[1].any()


def _sphere_cloud(device, S=1500):
    verts, faces, _ = load_obj(os.path.join(ROOT, "tests", "golden", "sphere_642.obj"))
    mesh = Meshes([verts.to(device)], [faces.verts_idx.to(device)])
    pts = sample_points_from_meshes(mesh, S, seed=11).detach()
    return pts, (0.5 + 0.5 * pts / pts.norm(dim=-1, keepdim=True)).contiguous()  # colours from the direction


def test_points_renderer_end_to_end(device):
    """sample_points_from_meshes of the sphere with per-point colours through FoVPerspectiveCameras:
    the gradient reaches the world points and the features.  The cameras are float32 on every path,
    so float64 starts from the projected points: the image, d features and d projected points of the
    native path against the float64 restatement at the kernel's indices, under the rule above; the
    world-space gradients against the composition's."""
    H, W = 40, 56
    pts, cols = _sphere_cloud(device)
    R, T = look_at_view_transform(2.7, 20.0, 40.0, device=device)
    rs = PointsRasterizationSettings(image_size=(H, W), radius=0.06, points_per_pixel=6)
    renderer = PointsRenderer(PointsRasterizer(FoVPerspectiveCameras(R=R, T=T, device=device), rs), AlphaCompositor((0.0, 0.0, 0.0)))
    cot = torch.randn((1, H, W, 3), generator=torch.Generator().manual_seed(1)).to(device)
    res = {}
    for native in (True, False):
        PT.NATIVE_POINTS = native
        try:
            p, f = pts.clone().requires_grad_(True), cols.clone().requires_grad_(True)
            pc = Pointclouds(p, features=f)
            img = renderer(pc)
            gp, gf = torch.autograd.grad((img * cot).sum(), (p, f))
            # the same image from the projected points as a leaf: d image / d projected points
            ndc = renderer.rasterizer.transform(pc).points_padded().detach().requires_grad_(True)
            idx, _, dists = rasterize_points(Pointclouds(ndc), (H, W), rs.radius, rs.points_per_pixel)
            img2 = renderer.compositor._rows(idx, 1 - dists / (rs.radius * rs.radius), pc.features_packed())
            assert torch.equal(img2, img)
            (gn,) = torch.autograd.grad((img2 * cot).sum(), ndc)
            res[native] = dict(img=img.detach(), gp=gp, gf=gf, gn=gn[0], idx=idx, ndc=ndc.detach()[0])
        finally:
            PT.NATIVE_POINTS = True
    a, b = res[True], res[False]
    assert tuple(a["img"].shape) == (1, H, W, 3) and (a["idx"][..., 0] >= 0).float().mean() > 0.2
    for g in (a["gp"], a["gf"]):
        assert torch.isfinite(g).all() and g.abs().sum() > 0
    assert torch.equal(a["idx"], b["idx"]) and torch.equal(a["ndc"], b["ndc"])
    assert_close(a["img"], b["img"], name="image")
    idx = a["idx"].cpu()
    n64, f64 = a["ndc"].cpu().double().requires_grad_(True), cols[0].cpu().double().requires_grad_(True)
    zero = torch.zeros(idx.shape, dtype=torch.float64)
    _, d64, _ = C.raster_loss64(n64, idx, zero, zero, H, W)
    r2 = float(torch.tensor(rs.radius, dtype=torch.float32).double() ** 2)
    img64 = C.composite64(idx, 1 - d64 / r2, f64, "alpha")
    assert_close(a["img"], img64.detach(), name="image vs float64")
    gn64, gf64 = torch.autograd.grad((img64 * cot.cpu().double()).sum(), (n64, f64))
    for key, want in (("gn", gn64), ("gf", gf64)):
        native, comp = C.rel_err(a[key].reshape(want.shape), want), C.rel_err(b[key].reshape(want.shape), want)
        print(f"renderer {key}: error composition(fp32) / native: {comp:.2e} / {native:.2e}")
        assert native <= max(4.0 * comp, 1e-5), (key, native, comp)
    # world space: each path within the rule of float64 from the projected points on, the transform shared
    assert C.rel_err(a["gp"], b["gp"]) <= 2e-5 and C.rel_err(a["gf"], b["gf"]) <= 2e-5


def test_one_sort_serves_both_backward_passes(device, monkeypatch):
    """The point -> (pixel, slot) CSR is built once per fragments object: one device sort in a
    renderer backward, shared by the compositor's and the rasterizer's gathers."""
    pts, cols = _sphere_cloud(device, 300)
    p, f = pts.clone().requires_grad_(True), cols.clone().requires_grad_(True)
    idx, _, dists = rasterize_points(Pointclouds(p * torch.tensor([0.5, 0.5, 0.0], device=device) + torch.tensor([0, 0, 1.0], device=device)),
                                     24, 0.1, 4)
    img = AlphaCompositor()._rows(idx, 1 - dists / 0.01, f[0])
    sorts = []
    real = torch.argsort
    monkeypatch.setattr(torch, "argsort", lambda *a, **k: (sorts.append(1), real(*a, **k))[1])
    gp, gf = torch.autograd.grad((img ** 2).sum(), (p, f))
    assert len(sorts) == 1 and gp.abs().sum() > 0 and gf.abs().sum() > 0


def test_render_step_is_captured_in_a_graph(device):
    """Forward + backward of PointsRenderer in one captured graph after a warm-up call; replayed with
    changed point values it equals the eager result bitwise."""
    pts, cols = _sphere_cloud(device, 800)
    R, T = look_at_view_transform(2.7, 10.0, 20.0, device=device)
    rs = PointsRasterizationSettings(image_size=32, radius=0.08, points_per_pixel=5)
    renderer = PointsRenderer(PointsRasterizer(FoVPerspectiveCameras(R=R, T=T, device=device), rs),
                              NormWeightedCompositor((1.0, 1.0, 1.0)))
    target = torch.rand((1, 32, 32, 3), generator=torch.Generator().manual_seed(3)).to(device)

    def step(p, f):
        loss = ((renderer(Pointclouds(p, features=f)) - target) ** 2).sum()
        gp, gf = torch.autograd.grad(loss, (p, f))
        return loss, gp, gf

    moved = pts * 1.1 + 0.05
    eager = [[t.clone() for t in step(x.clone().requires_grad_(True), cols.clone().requires_grad_(True))] for x in (pts, moved)]
    p_g, f_g = pts.clone().requires_grad_(True), cols.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the one call before the capture
        step(p_g, f_g)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(p_g, f_g)
    for x, want in zip((pts, moved), eager):
        with torch.no_grad():
            p_g.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(o, w) for o, w in zip(out, want))
    assert not torch.equal(eager[0][0], eager[1][0]) and eager[0][1].abs().sum() > 0

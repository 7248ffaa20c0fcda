"""Native mesh regularisers (csrc/pr_meshloss.hip behind renderer/loss.py) on the GPU: values and
d verts against the dense float64 restatement of the formulas (mesh_loss_cases.py), against the
torch composition (NATIVE_MESHLOSS = False), bitwise reproducibility, capture in a HIP graph, and
composition with the rendered loss of eval.py's deformation step.

Tolerances.  Loss values: conftest.assert_close's defaults (1e-5).  Gradients: the formulas cancel
in float32 (|l_i| is ~1e-2 of |v_i| on a smooth mesh), so each case measures the error of the
float32 run of the restatement itself against its float64 run (max-abs over max-abs) and allows the
native result 4x that (the CSR gather sums in another order than the dense mm), floored at 1e-5.

Measured on an MI355X (sphere_642, reference error / native error, max-abs over max-abs):
    uniform 1.39e-05 / 1.34e-05, cot 3.92e-04 / 4.18e-04, cotcurv 4.15e-05 / 4.91e-05, edge 5.92e-07 / 5.35e-07.
Next largest: hub70 cot 1.09e-05 / 1.33e-05, cotcurv 1.06e-05 / 1.67e-05; grid3 cot 8.76e-06 / 9.77e-06,
cotcurv 6.05e-06 / 7.53e-06; batch2 cot 7.46e-07 / 1.75e-06.  Every other case is below 1e-6 on
both sides.  The native error is 0.3x to 2.4x the reference's own, inside the factor 4; loss values
agree with float64 to 2.5e-06 relative (sphere_642 uniform; every other case 6e-07 or better)."""
import functools
import math

import pytest
import torch

import pertrenderer_amd as pa
from conftest import assert_close
from mesh_loss_cases import LOSS_CASES_GPU, case, ref_edge, ref_laplacian, rel_err
from pertrenderer_amd import _native as nat
from pertrenderer_amd.renderer import (FoVPerspectiveCameras, MeshRasterizer, MeshRenderer, Meshes,
                                       RasterizationSettings, TexturesVertex, look_at_view_transform)
from pertrenderer_amd.renderer import loss as L

pytestmark = pytest.mark.gpu

KINDS = ["uniform", "cot", "cotcurv", "edge"]
TARGET = 0.3  # edge loss target length


@functools.lru_cache(maxsize=None)
def _reference(name, kind):
    """(loss64, grad64, float32 restatement's gradient error), computed once per case."""
    verts, faces = case(name)
    run = (lambda dt: ref_edge(verts, faces, TARGET, dt)) if kind == "edge" else \
        (lambda dt: ref_laplacian(verts, faces, kind, dt))
    loss64, g64 = run(torch.float64)
    _, g32 = run(torch.float32)
    return loss64, g64, rel_err(g32, g64)


def _fn(kind):
    return (lambda m: L.mesh_edge_loss(m, TARGET)) if kind == "edge" else (lambda m: L.mesh_laplacian_smoothing(m, kind))


def _run(name, kind, device, native=True):
    verts, faces = case(name)
    keep = L.NATIVE_MESHLOSS
    L.NATIVE_MESHLOSS = native
    try:
        vs = [v.to(device).requires_grad_(True) for v in verts]
        out = _fn(kind)(Meshes(vs, [f.to(device) for f in faces]))
        g = torch.cat(torch.autograd.grad(out, vs))
    finally:
        L.NATIVE_MESHLOSS = keep
    return out.detach(), g


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", LOSS_CASES_GPU)
def test_native_matches_float64_restatement(name, kind, device):
    loss64, g64, ref_err = _reference(name, kind)
    loss, g = _run(name, kind, device)
    err = rel_err(g, g64)
    print(f"{name} {kind}: loss {loss.item():.8e} vs {loss64.item():.8e}; gradient error "
          f"reference(fp32) {ref_err:.2e} native {err:.2e}")
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert_close(loss, loss64, name="loss")
    assert err <= max(4.0 * ref_err, 1e-5), (err, ref_err)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", LOSS_CASES_GPU)
def test_native_matches_torch_composition(name, kind, device, monkeypatch):
    """PR_NATIVE_MESHLOSS=0 (the module flag) restores the torch composition; same tolerance.  The
    composition's edge loss is the global mean over edges, which is the per-mesh definition only
    for equal edge counts: the unequal batch is left to the float64 check above."""
    if kind == "edge" and name == "batch2":
        verts, faces = case(name)
        loss, _ = _run(name, kind, device)
        assert_close(loss, ref_edge(verts, faces, TARGET, per_mesh=True)[0], name="per-mesh edge loss")
        assert abs(loss.item() - ref_edge(verts, faces, TARGET, per_mesh=False)[0].item()) > 1e-3 * loss.item()
        return
    _, _, ref_err = _reference(name, kind)
    loss, g = _run(name, kind, device)
    monkeypatch.setattr(L, "NATIVE_MESHLOSS", False)
    loss_t, g_t = _run(name, kind, device, native=False)
    assert_close(loss, loss_t, name="loss")
    assert rel_err(g, g_t) <= max(4.0 * ref_err, 1e-5)


@pytest.mark.parametrize("kind", KINDS)
def test_native_calls_are_bitwise_reproducible(kind, device):
    for name in ("sphere_642", "batch2"):
        a, b = _run(name, kind, device), _run(name, kind, device)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), name


def test_raw_ops_refuse_cpu_tensors():
    verts, faces = case("tetrahedron")
    m = Meshes(verts, faces)
    with pytest.raises(nat.NativeError):
        L._LaplacianFn.apply(m.verts_packed(), m._topo, nat.PR_MESH_LAP_COT)
    with pytest.raises(nat.NativeError):
        L._EdgeLossFn.apply(m.verts_packed(), m._topo, 0.0)


def _regularisers(mesh):
    return L.mesh_laplacian_smoothing(mesh, "cot") + L.mesh_edge_loss(mesh) + L.mesh_normal_consistency(mesh)


def test_regulariser_step_is_captured_in_a_graph(device):
    """Forward, backward and an in-place SGD update of the vertex offsets in one captured graph:
    three replays equal three eager steps from the same start, bitwise (every sum on the path is
    in a fixed order).  Nothing on the path may synchronise or build an index tensor once the
    topology caches exist (one call before the capture)."""
    verts, faces = case("sphere_642")
    base = Meshes([verts[0].to(device)], [faces[0].to(device)])
    start = (0.02 * torch.randn(verts[0].shape, generator=torch.Generator().manual_seed(3))).to(device)
    lr = 0.05

    def step(deform):
        loss = _regularisers(base.offset_verts(deform))
        loss.backward()
        with torch.no_grad():
            deform.add_(deform.grad, alpha=-lr)
        return loss

    d_e = start.clone().requires_grad_(True)
    eager = []
    for _ in range(3):
        d_e.grad = None
        eager.append(step(d_e).detach().clone())

    d_g = start.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the one call before the capture: caches, autograd warm-up
        _regularisers(base.offset_verts(d_g)).backward()
    torch.cuda.current_stream().wait_stream(side)
    d_g.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step(d_g)
    replayed = []
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        replayed.append(loss.detach().clone())
    for i, (a, b) in enumerate(zip(eager, replayed)):
        assert torch.equal(a, b), (i, a.item(), b.item())
    assert torch.equal(d_e.detach(), d_g.detach())
    assert not torch.equal(d_g.detach(), start) and eager[2].item() < eager[0].item()


def test_laplacian_gradient_adds_to_the_render_gradient(device):
    """One eager deformation step of eval.py:448-457: d (L1 + 5e-3 laplacian) / d deform equals the
    sum of the two gradients taken separately.  The renderer's noise is the torch draw, reseeded
    before every render, and its backward runs in deterministic order, so the rendered gradient is
    the same in both runs and the comparison sees the regulariser's contribution alone."""
    verts, faces = case("sphere_642")
    g = torch.Generator().manual_seed(11)
    v = verts[0] - verts[0].mean(0)
    v = (v / (2 * v.abs().max())).to(device)
    colors = torch.rand((1, v.shape[0], 3), generator=g).to(device)
    base = Meshes([v], [faces[0].to(device)], TexturesVertex(colors))
    target = torch.rand((48, 48, 3), generator=g).to(device)
    start = (0.01 * torch.randn(v.shape, generator=g)).to(device)
    sigma, gamma = 1e-3, 1e-2
    R, T = look_at_view_transform(2.7, 30.0, 120.0, device=device)
    cams = FoVPerspectiveCameras(R=R, T=T, device=device)
    rs = RasterizationSettings(image_size=48, blur_radius=math.log(1e4 - 1) * sigma, faces_per_pixel=50)
    shader = pa.RandomSimpleShader(device=device, cameras=cams, smoothrast=pa.GaussianRast(nb_samples=8, sigma=sigma),
                                   smoothagg=pa.GaussianAgg(nb_samples=8, gamma=gamma))
    renderer = MeshRenderer(MeshRasterizer(cameras=cams, raster_settings=rs), shader)

    def grad(w_rgb, w_lap):
        deform = start.clone().requires_grad_(True)
        mesh = base.offset_verts(deform)
        total = 0.0
        if w_rgb:
            torch.manual_seed(7)
            total = total + w_rgb * (renderer(mesh)[..., :3] - target).abs().mean()
        if w_lap:
            total = total + w_lap * L.mesh_laplacian_smoothing(mesh, method="uniform")
        total.backward()
        return deform.grad

    old_noise, old_det = pa.noise.get_noise_source(), torch.are_deterministic_algorithms_enabled()
    pa.set_noise_source("torch")
    torch.use_deterministic_algorithms(True)
    try:
        both, rgb, lap = grad(1.0, 5e-3), grad(1.0, 0.0), grad(0.0, 5e-3)
    finally:
        torch.use_deterministic_algorithms(old_det)
        pa.set_noise_source(old_noise)
    assert rgb.abs().max() > 0 and lap.abs().max() > 0
    assert_close(both, rgb + lap, name="d deform")

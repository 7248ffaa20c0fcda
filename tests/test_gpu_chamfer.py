"""Native chamfer_distance (csrc/pr_chamfer.hip behind renderer/loss.py) on the GPU, against the
float64 brute-force restatement of chamfer_cases.py: nearest indices (the lowest index on exact
ties), distances, losses under every reduction, weights and lengths, loss_normals, all gradients;
against the torch composition on the device; bitwise reproducibility; capture in a HIP graph.

Every shape runs with the split count the library picks and with PR_CHAMFER_SPLITS=3 (the database
cut into three ranges and merged), with full clouds and with per-cloud lengths.  The clouds are
seeded so that every query's best and second-best d^2 differ by >= 1e-6 in float64
(chamfer_cases.clouds asserts it): float32 cannot pick another neighbour.  The planted exact
duplicates (five copies of one database point, in the first, the middle and the last range of a
split database, and one query on top of them) are checked for the lowest-index rule, within a
range and in the merge of the ranges, and for d = 0 exactly.

Tolerances.  Values: conftest.assert_close's defaults.  Gradients: the native max-abs error over
max-abs may be 4x the float32 restatement's own error against float64, floored at 1e-5 (the rule
of test_gpu_mesh_losses.py); the gradient is 2 g (x_i - y_j), so both are a few 1e-8 and the floor
decides.

Measured on an MI355X (float32 restatement error / native error, max-abs over max-abs, the
largest over all cases and both split settings): d x 1.06e-07 / 2.02e-07, d y 8.84e-08 / 8.84e-08.
The worst native case is (2,64,65) with cut lengths, None / sum, no weights: 8.44e-08 / 2.02e-07
(a point with several incoming neighbours sums them in another order than autograd's
index_add); everything is more than an order below the 1e-5 floor."""
import functools

import pytest
import torch

from chamfer_cases import DUP, clouds, lengths, planted, ref_chamfer
from conftest import assert_close
from mesh_loss_cases import case, rel_err
from pertrenderer_amd import _native as nat
from pertrenderer_amd.renderer import Meshes
from pertrenderer_amd.renderer import loss as L

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 3, 70), (2, 64, 65), (2, 257, 1025)]
# (batch_reduction, point_reduction, weights)
CONFIGS = [("mean", "mean", False), ("sum", "sum", True), ("mean", "sum", True), (None, "mean", True),
           (None, "sum", False)]
COT = torch.tensor([1.0, -0.7])
WEIGHTS = torch.tensor([0.5, 2.0])


@functools.lru_cache(maxsize=None)
def _reference(shape, cut, config):
    """(float64 restatement, the float32 restatement's gradient errors (x, y)), once per case."""
    x, y, xn, yn = clouds(shape)
    xl, yl = lengths(shape, cut)
    br, pr, weighted = config
    w = WEIGHTS[: shape[0]] if weighted else None
    cot = COT[: shape[0]] if br is None else None
    r64 = ref_chamfer(x, y, br, pr, xl, yl, xn, yn, w, cot=cot)
    r32 = ref_chamfer(x, y, br, pr, xl, yl, None, None, w, dtype=torch.float32, cot=cot)
    return r64, (rel_err(r32["grad_x"], r64["grad_x"]), rel_err(r32["grad_y"], r64["grad_y"]))


def _run(shape, cut, config, device, native=True):
    x, y, xn, yn = clouds(shape)
    xl, yl = lengths(shape, cut)
    br, pr, weighted = config
    dev = lambda t: None if t is None else t.to(device)  # noqa: E731
    keep = L.NATIVE_MESHLOSS
    L.NATIVE_MESHLOSS = native
    try:
        xr, yr = x.to(device).requires_grad_(True), y.to(device).requires_grad_(True)
        loss, ln = L.chamfer_distance(xr, yr, br, pr, x_lengths=dev(xl), y_lengths=dev(yl), x_normals=dev(xn),
                                      y_normals=dev(yn), weights=dev(WEIGHTS[: shape[0]]) if weighted else None)
        out = loss if br is not None else loss * COT[: shape[0]].to(device)
        gx, gy = torch.autograd.grad(out.sum(), (xr, yr))
    finally:
        L.NATIVE_MESHLOSS = keep
    return loss.detach(), ln.detach(), gx, gy


@pytest.fixture(params=[None, "3"], ids=["splits-default", "splits-3"])
def splits(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("PR_CHAMFER_SPLITS", raising=False)
    else:
        monkeypatch.setenv("PR_CHAMFER_SPLITS", request.param)
    return request.param


@pytest.mark.parametrize("cut", [False, True], ids=["full", "cut"])
@pytest.mark.parametrize("shape", SHAPES)
def test_nearest_neighbours_match_float64(shape, cut, splits, device):
    x, y, _, _ = clouds(shape)
    xl, yl = lengths(shape, cut)
    want, _ = _reference(shape, cut, CONFIGS[0])
    dev = lambda t: None if t is None else t.to(device)  # noqa: E731
    dx, dy, ix, iy = L._ChamferFn.apply(x.to(device), y.to(device), dev(xl), dev(yl))
    assert dx.dtype == dy.dtype == torch.float32 and ix.dtype == iy.dtype == torch.int32
    assert torch.equal(ix.cpu().long(), want["idx_x"]) and torch.equal(iy.cpu().long(), want["idx_y"])
    assert_close(dx, want["dist_x"], name="dist_x")
    assert_close(dy, want["dist_y"], name="dist_y")
    for n in range(shape[0] if planted(shape) else 0):
        nx, ny = (shape[1], shape[2]) if xl is None else (int(xl[n]), int(yl[n]))
        live = [j for j in planted(shape) if j < ny]
        if nx < 2 or len(live) < 2:
            continue
        # the query on top of the copies (which lie in different ranges of the split database): the
        # lowest copy, at exactly 0; and each copy's own nearest is that query, at exactly 0
        assert ix[n, 1].item() == DUP[0] and dx[n, 1].item() == 0.0
        assert [iy[n, j].item() for j in live] == [1] * len(live) and not dy[n, live].any()
    if xl is not None:
        for n in range(shape[0]):
            assert (ix[n, int(xl[n]):] == -1).all() and not dx[n, int(xl[n]):].any()
            assert (iy[n, int(yl[n]):] == -1).all() and not dy[n, int(yl[n]):].any()
            assert ix[n, :int(xl[n])].max() < int(yl[n]) and iy[n, :int(yl[n])].max() < int(xl[n])


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: f"{c[0]}-{c[1]}-{'w' if c[2] else 'nw'}")
@pytest.mark.parametrize("cut", [False, True], ids=["full", "cut"])
@pytest.mark.parametrize("shape", SHAPES)
def test_losses_and_gradients_match_float64(shape, cut, config, splits, device):
    want, (ex, ey) = _reference(shape, cut, config)
    loss, ln, gx, gy = _run(shape, cut, config, device)
    err_x, err_y = rel_err(gx, want["grad_x"]), rel_err(gy, want["grad_y"])
    print(f"{shape} cut={cut} {config}: gradient error restatement(fp32) x {ex:.2e} y {ey:.2e}, "
          f"native x {err_x:.2e} y {err_y:.2e}")
    assert loss.dtype == torch.float32
    assert_close(loss, want["loss"], name="loss")
    assert_close(ln, want["loss_normals"], name="loss_normals")
    assert err_x <= max(4.0 * ex, 1e-5) and err_y <= max(4.0 * ey, 1e-5), (err_x, ex, err_y, ey)
    xl, yl = lengths(shape, cut)
    if xl is not None:  # padded points get gradient 0
        for n in range(shape[0]):
            assert not gx[n, int(xl[n]):].any() and not gy[n, int(yl[n]):].any()


@pytest.mark.parametrize("cut", [False, True], ids=["full", "cut"])
@pytest.mark.parametrize("shape", SHAPES)
def test_native_matches_torch_composition(shape, cut, splits, device):
    config = CONFIGS[2]
    _, (ex, ey) = _reference(shape, cut, config)
    loss, ln, gx, gy = _run(shape, cut, config, device)
    loss_t, ln_t, gx_t, gy_t = _run(shape, cut, config, device, native=False)
    assert_close(loss, loss_t, name="loss")
    assert_close(ln, ln_t, name="loss_normals")
    assert rel_err(gx, gx_t) <= max(4.0 * ex, 1e-5) and rel_err(gy, gy_t) <= max(4.0 * ey, 1e-5)


def test_call_without_keywords_returns_loss_and_none(device):
    x, y, _, _ = clouds((2, 64, 65))
    want, _ = _reference((2, 64, 65), False, CONFIGS[0])
    loss, ln = L.chamfer_distance(x.to(device), y.to(device))
    assert ln is None
    assert_close(loss, want["loss"], name="loss")


def test_empty_database_gives_zero_and_minus_one(device):
    x, y, _, _ = clouds((2, 64, 65))
    xl, yl = torch.tensor([5, 0], device=device), torch.tensor([0, 7], device=device)
    xr, yr = x.to(device).requires_grad_(True), y.to(device).requires_grad_(True)
    dx, dy, ix, iy = L._ChamferFn.apply(xr, yr, xl, yl)
    assert not dx.any() and not dy.any() and (ix == -1).all() and (iy == -1).all()
    gx, gy = torch.autograd.grad(dx.sum() + dy.sum(), (xr, yr))
    assert not gx.any() and not gy.any()


def test_points_without_a_finite_neighbour_are_not_silenced(splits, device):
    """A NaN query, and finite queries facing a database of NaN points only, get a non-finite
    distance (NaN / +inf), idx -1 and gradient 0: the loss shows the divergence.  A NaN database
    point among finite ones is never chosen."""
    x, y, _, _ = clouds((1, 3, 70))
    x, y = x.to(device).clone(), y.to(device).clone()
    x[0, 2, 1] = float("nan")
    y[0, 9] = float("nan")
    xr, yr = x.requires_grad_(True), y.requires_grad_(True)
    dx, dy, ix, iy = L._ChamferFn.apply(xr, yr, None, None)
    assert torch.isnan(dx[0, 2]) and ix[0, 2] == -1 and torch.isfinite(dx[0, :2]).all() and (ix[0, :2] != 9).all()
    assert torch.isnan(dy[0, 9]) and iy[0, 9] == -1
    rest = [j for j in range(70) if j != 9]
    assert torch.isfinite(dy[0, rest]).all() and (iy[0, rest] >= 0).all() and (iy[0, rest] != 2).all()
    gx, gy = torch.autograd.grad(dx[0, :2].sum() + dy[0, rest].sum(), (xr, yr))
    assert not gx[0, 2].any() and not gy[0, 9].any() and torch.isfinite(gx).all() and torch.isfinite(gy).all()
    assert not torch.isfinite(L.chamfer_distance(x, y)[0])
    dx, _, ix, _ = L._ChamferFn.apply(x.detach()[:, :2], torch.full_like(y.detach(), float("nan")), None, None)
    assert torch.isinf(dx).all() and (dx > 0).all() and (ix == -1).all()


def test_other_point_dimensions_take_the_composition(device):
    """(N,P,2) clouds worked before the native op (torch.cdist takes any dimension) and still do."""
    g = torch.Generator().manual_seed(2)
    x, y = torch.rand((2, 9, 2), generator=g), torch.rand((2, 11, 2), generator=g)
    want = L.chamfer_distance(x.double(), y.double())[0]
    assert_close(L.chamfer_distance(x.to(device), y.to(device))[0], want, name="loss")
    with pytest.raises(ValueError):
        L._ChamferFn.apply(x.to(device), y.to(device), None, None)


def test_native_calls_are_bitwise_reproducible(splits, device):
    for shape in ((2, 64, 65), (2, 257, 1025)):
        a, b = _run(shape, True, CONFIGS[1], device), _run(shape, True, CONFIGS[1], device)
        assert all(torch.equal(p, q) for p, q in zip(a, b)), shape


def test_raw_op_refuses_cpu_tensors():
    x, y, _, _ = clouds((1, 3, 70))
    with pytest.raises(nat.NativeError):
        L._ChamferFn.apply(x, y, None, None)


def test_fitting_step_is_captured_in_a_graph(device):
    """chamfer(verts, cloud) + mesh_normal_consistency, backward and an in-place SGD update of the
    vertex offsets in one captured graph, after one warm-up call: three replays equal three eager
    steps from the same start, bitwise."""
    verts, faces = case("sphere_642")
    base = Meshes([verts[0].to(device)], [faces[0].to(device)])
    g = torch.Generator().manual_seed(5)
    cloud = (1.2 * torch.rand((1, 500, 3), generator=g) - 0.6).to(device)
    start = (0.02 * torch.randn(verts[0].shape, generator=g)).to(device)
    lr = 0.05

    def objective(deform):
        mesh = base.offset_verts(deform)
        return L.chamfer_distance(mesh.verts_padded(), cloud)[0] + 0.1 * L.mesh_normal_consistency(mesh)

    def step(deform):
        loss = objective(deform)
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
        objective(d_g).backward()
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

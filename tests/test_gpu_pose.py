"""Native pose ops (pr_so3_exp_*, pr_rotate_*) against the torch formulas of
PyTorch3D 0.4.0's so3_exponential_map / Rotate.transform_points (evaluated on CPU)."""
import numpy as np
import pytest
import torch

import pose_cases
from conftest import assert_close
from pertrenderer_amd import host_layer
from pertrenderer_amd.renderer.transforms import Rotate, so3_exponential_map

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("scale", [1e-4, 0.3, 2.5])
def test_so3_exponential_map_fwd_bwd(scale, device):
    g = torch.Generator().manual_seed(3)
    w = (scale * torch.randn((7, 3), generator=g))
    w[0] = 0.0  # below the clamp: zero gradient through the norm
    gR = torch.randn((7, 3, 3), generator=g)
    wc = w.clone().requires_grad_(True)
    Rc = so3_exponential_map(wc)
    (Rc * gR).sum().backward()
    wg = w.to(device).requires_grad_(True)
    Rg = so3_exponential_map(wg)
    (Rg * gR.to(device)).sum().backward()
    torch.testing.assert_close(Rg.detach().cpu(), Rc.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(wg.grad.cpu(), wc.grad, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("N,P,shared", [(1, 642, True), (3, 1000, False), (4, 17, True)])
def test_rotate_transform_points_fwd_bwd(N, P, shared, device):
    g = torch.Generator().manual_seed(N * P)
    pts = torch.randn((N, P, 3), generator=g)
    R = torch.randn((1 if shared else N, 3, 3), generator=g)
    gout = torch.randn((N, P, 3), generator=g)
    pc, Rc = pts.clone().requires_grad_(True), R.clone().requires_grad_(True)
    oc = Rotate(Rc).transform_points(pc)
    (oc * gout).sum().backward()
    pg, Rg = pts.to(device).requires_grad_(True), R.to(device).requires_grad_(True)
    og = Rotate(Rg).transform_points(pg)
    (og * gout.to(device)).sum().backward()
    torch.testing.assert_close(og.detach().cpu(), oc.detach(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(pg.grad.cpu(), pc.grad, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(Rg.grad.cpu(), Rc.grad, rtol=1e-4, atol=1e-4)


# ---- float64 parity at launch and branch edges (tests/pose_cases.py), on both autograd layers
pc = pose_cases  # (test_rotate_transform_points_fwd_bwd above has a local of this name)


@pytest.fixture(params=pc.LAYERS)
def layer(request):
    with pc.autograd_layer(request.param) as ok:
        if not ok:
            pytest.skip(f"C++ autograd layer not built: {host_layer.error()}")
        yield request.param


def _so3_gpu(w, G, eps, device):
    wg = torch.from_numpy(np.ascontiguousarray(w)).to(device).requires_grad_(True)
    R = so3_exponential_map(wg, eps) if eps is not None else so3_exponential_map(wg)
    R.backward(torch.from_numpy(np.ascontiguousarray(G)).to(device))
    return R.detach().cpu().numpy(), wg.grad.cpu().numpy()


def _check_so3(Rg, gg, w, G, ang, eps):
    """Rows >= 0.02 at the standing bar, the rows below at 4x the float32 composition's own error."""
    R, gw = pc.so3_ref(w, eps, G)
    big = ang >= pc.SO3_SMALL
    assert_close(Rg[big], R[big], name="R")
    assert_close(gg[big], gw[big], name="d log_rot")
    if (~big).any():
        Rc, gc = pc.so3_fp32_composition(w, eps, G)
        fr = pc.assert_small_angle_rows(Rg[~big], R[~big], Rc[~big], "R, small angles")
        fg = pc.assert_small_angle_rows(gg[~big], gw[~big], gc[~big], "d log_rot, small angles")
        print(f"so3 rows below {pc.SO3_SMALL}, rel. to the row's largest |ref| (fp32 composition, kernel): "
              f"R {fr[0]:.2e} {fr[1]:.2e}; d log_rot {fg[0]:.2e} {fg[1]:.2e}")


def test_so3_130_rows_match_float64(layer, device):
    """Three blocks and a tail; zero, either side of the clamp, near pi and 2 pi, beyond a turn.
    Measured on an MI355X, rows below 0.02, error relative to the row's largest reference component,
    float32 CPU composition / kernel: R 3.78e-08 / 3.78e-08, d log_rot 1.59e-06 / 1.60e-06 (both
    layers the same)."""
    w, G, ang = pc.so3_inputs()
    Rg, gg = _so3_gpu(w, G, None, device)
    _check_so3(Rg, gg, w, G, ang, pc.SO3_EPS)
    # below the clamp the angle is sqrt(eps) for every row: R - 1 is linear in w there
    assert np.array_equal(Rg[0], np.eye(3, dtype=np.float32))


@pytest.mark.parametrize("N", [0, 1, 64, 65])
def test_so3_block_edges(N, layer, device):
    w, G, ang = pc.so3_inputs()
    Rg, gg = _so3_gpu(w[:N], G[:N], None, device)
    assert Rg.shape == (N, 3, 3) and gg.shape == (N, 3)
    if N:
        _check_so3(Rg, gg, w[:N], G[:N], ang[:N], pc.SO3_EPS)


def test_so3_other_eps(layer, device):
    """eps = 1e-2 through the wrapper, forward and backward: rows either side of |w| = 0.1."""
    w, G, ang, eps = pc.so3_inputs_eps()
    Rg, gg = _so3_gpu(w, G, eps, device)
    _check_so3(Rg, gg, w, G, ang, eps)
    _, gw = pc.so3_ref(w, eps, G)
    _, g4 = pc.so3_ref(w, pc.SO3_EPS, G)  # the default eps gives another answer on the clamped rows
    assert np.abs(g4 - gw)[ang < 0.1].max() > 1e-3 * np.abs(gw).max()


def test_so3_on_the_clamp_boundary(layer, device):
    """|w|^2 == eps exactly (eps = 2^-4): the gradient passes through the norm (the backward's >=)."""
    w, G, ang, eps = pc.so3_boundary_inputs()
    Rg, gg = _so3_gpu(w, G, eps, device)
    _check_so3(Rg, gg, w, G, ang, eps)


def test_so3_strided_input(layer, device):
    w, G, ang = pc.so3_inputs()
    leaf = torch.zeros((w.shape[0], 6), device=device)
    leaf[:, ::2] = torch.from_numpy(w).to(device)
    leaf[:, 1::2] = 7.0
    leaf.requires_grad_(True)
    view = leaf[:, ::2]
    assert not view.is_contiguous()
    R = so3_exponential_map(view)
    R.backward(torch.from_numpy(G).to(device))
    g = leaf.grad.cpu().numpy()
    _check_so3(R.detach().cpu().numpy(), g[:, ::2], w, G, ang, pc.SO3_EPS)
    assert np.array_equal(g[:, 1::2], np.zeros((w.shape[0], 3), np.float32))


ROTATE_SHAPES = [(2, 600000, False),  # > 4096 * 256 points: the forward's grid-stride loop repeats
                 (1, 70000, True),  # one workgroup, 274 iterations
                 (5, 1, True), (1, 1, True), (3, 257, False)]


@pytest.fixture(scope="module")
def rotate_refs():
    cache = {}

    def get(N, P, shared):
        k = (N, P, shared)
        if k not in cache:
            inp = pc.rotate_inputs(N, P, shared, 100 + N * P)
            cache[k] = (inp, pc.rotate_ref(*inp))
        return cache[k]
    return get


@pytest.mark.parametrize("N,P,shared", ROTATE_SHAPES)
def test_rotate_matches_float64(N, P, shared, layer, device, rotate_refs):
    (pts, R, gout), (o, gp, gR) = rotate_refs(N, P, shared)
    pg, Rg = pts.to(device).clone().requires_grad_(True), R.to(device).clone().requires_grad_(True)
    out = Rotate(Rg).transform_points(pg)
    out.backward(gout.to(device))
    assert_close(out, o, name="out")
    assert_close(pg.grad, gp, name="d points")
    assert_close(Rg.grad, gR, name="d R")
    first = Rg.grad.clone()  # the R reduction has a fixed order: bitwise the same again
    pg.grad = Rg.grad = None
    Rotate(Rg).transform_points(pg).backward(gout.to(device))
    assert torch.equal(Rg.grad, first)


@pytest.mark.parametrize("mode", ["points", "R"])
@pytest.mark.parametrize("N,P,shared", [(3, 257, False), (1, 70000, True)])
def test_rotate_backward_single_gradient(N, P, shared, mode, layer, device, rotate_refs):
    """Only one input requires grad: the kernel gets a NULL for the other gradient."""
    (pts, R, gout), (o, gp, gR) = rotate_refs(N, P, shared)
    pg, Rg = pts.to(device).clone(), R.to(device).clone()
    want, other = (pg, Rg) if mode == "points" else (Rg, pg)
    want.requires_grad_(True)
    sentinel = torch.full_like(other, -123.0)
    other.grad = sentinel.clone()
    Rotate(Rg).transform_points(pg).backward(gout.to(device))
    assert_close(want.grad, gp if mode == "points" else gR, name="d " + mode)
    assert torch.equal(other.grad, sentinel) and torch.equal(other, (R if mode == "points" else pts).to(device))


def test_rotate_views(layer, device, rotate_refs):
    """R given as a transposed view, the points as a permuted view: gradients on the leaves."""
    (pts, R, gout), (o, gp, gR) = rotate_refs(3, 257, False)
    R0 = R.transpose(1, 2).contiguous().to(device).requires_grad_(True)  # R0^T = R
    p0 = pts.permute(1, 0, 2).contiguous().to(device).requires_grad_(True)  # (P,N,3)
    Rv, pv = R0.transpose(1, 2), p0.permute(1, 0, 2)
    assert not Rv.is_contiguous() and not pv.is_contiguous()
    out = Rotate(Rv).transform_points(pv)
    out.backward(gout.to(device))
    assert_close(out, o, name="out")
    assert_close(p0.grad, gp.transpose(1, 0, 2), name="d points leaf")
    assert_close(R0.grad, gR.transpose(0, 2, 1), name="d R leaf")

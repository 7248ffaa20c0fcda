"""knn_points / knn_gather on the GPU (the torch composition of renderer/ops.py, on the device),
against the float64 brute force of knn_cases.py: neighbour indices (ascending index on exact ties),
distances, padding, gradients, bitwise reproducibility, return_nn / knn_gather, non-finite points,
K and D beyond 64 and 32, and that the forward never synchronises with the host.

Every shape runs with full clouds and with per-cloud lengths.  The clouds are seeded so that
float32 cannot reorder neighbours except the planted ties (knn_cases.clouds asserts a 16-fold
margin over float32's rounding).  The planted exact duplicates (five copies of one database point
and one query on top of them) are checked for the ascending-index rule and for d = 0 exactly.

Tolerances.  Values: conftest.assert_close's defaults.  Gradients: the max-abs error over max-abs
may be 4x the float32 restatement's own error against float64, floored at 1e-5 (the rule of
test_gpu_mesh_losses.py, through mesh_loss_cases.rel_err).

Measured on an MI355X (float32 restatement error / the composition's error on the device, max-abs
over max-abs, the largest over all cases): d p1 1.30e-07 / 8.93e-08, d p2 1.10e-07 / 1.87e-07 (the
latter at (1,70,300,3,64) with cut lengths: a database point with many incoming neighbours is summed
by index_put_ in another order than autograd's float64 reference).  Everything is more than an
order below the 1e-5 floor, which decides."""
import pytest
import torch

from conftest import assert_close
from knn_cases import DUP, SHAPES, clouds, cotangent, lengths, planted, ref_knn, reference
from mesh_loss_cases import rel_err
from pertrenderer_amd.renderer import ops

pytestmark = pytest.mark.gpu

IDS = ["-".join(map(str, s)) for s in SHAPES]
shapes = pytest.mark.parametrize("shape", SHAPES, ids=IDS)
cuts = pytest.mark.parametrize("cut", [False, True], ids=["full", "cut"])


def _dev(t, device):
    return None if t is None else t.to(device)


@cuts
@shapes
def test_forward_matches_float64(shape, cut, device):
    x, y = clouds(shape)
    xl, yl = lengths(shape, cut)
    want = reference(shape, cut)
    d, raw = ops._knn_points_torch(x.to(device), y.to(device), _dev(xl, device), _dev(yl, device), shape[4])
    assert d.dtype == torch.float32 and raw.dtype == torch.int64 and d.device.type == raw.device.type == "cuda"
    assert tuple(d.shape) == tuple(raw.shape) == (shape[0], shape[1], shape[4])
    assert torch.equal(raw.cpu(), want["idx"])
    assert_close(d, want["dists"], name="dists")
    r = ops.knn_points(x.to(device), y.to(device), _dev(xl, device), _dev(yl, device), K=shape[4])
    assert r.idx.dtype == torch.int64 and torch.equal(r.idx, raw.clamp(min=0)) and torch.equal(r.dists, d)
    assert r.knn is None


@cuts
@pytest.mark.parametrize("shape", [s for s in SHAPES if planted(s)], ids=lambda s: "-".join(map(str, s)))
def test_planted_ties(shape, cut, device):
    x, y = clouds(shape)
    xl, yl = lengths(shape, cut)
    d, raw = ops._knn_points_torch(x.to(device), y.to(device), _dev(xl, device), _dev(yl, device), shape[4])
    seen = 0
    for n in range(shape[0]):
        nx, ny = (shape[1], shape[2]) if xl is None else (int(xl[n]), int(yl[n]))
        live = [c for c in planted(shape) if c < ny][:shape[4]]
        if nx < 2 or len(live) < 2:
            continue
        seen += 1
        assert raw[n, 1, :len(live)].tolist() == live and live[0] == DUP[0]
        assert (d[n, 1, :len(live)] == 0.0).all()
    assert seen > 0


@shapes
def test_padding(shape, device):
    x, y = clouds(shape)
    xl, yl = lengths(shape, True)
    N, _, P2, _, K = shape
    d, raw = ops._knn_points_torch(x.to(device), y.to(device), xl.to(device), yl.to(device), K)
    for n in range(N):
        nx, k = int(xl[n]), min(K, int(yl[n]))
        assert (raw[n, nx:] == -1).all() and not d[n, nx:].any()
        assert (raw[n, :, k:] == -1).all() and not d[n, :, k:].any()
        assert (raw[n, :nx, :k] >= 0).all() and (raw[n, :nx, :k] < int(yl[n])).all()
    if K > P2:  # without lengths: the slots past P2
        r = ops.knn_points(x.to(device), y.to(device), K=K)
        assert not r.dists[:, :, P2:].any() and not r.idx[:, :, P2:].any()


@cuts
@shapes
def test_gradients_match_float64(shape, cut, device):
    x, y = clouds(shape)
    xl, yl = lengths(shape, cut)
    want = reference(shape, cut)
    e1, e2 = want["err"]
    xr, yr = x.to(device).requires_grad_(True), y.to(device).requires_grad_(True)
    r = ops.knn_points(xr, yr, _dev(xl, device), _dev(yl, device), K=shape[4])
    assert not r.idx.requires_grad
    g1, g2 = torch.autograd.grad((r.dists * cotangent(shape).to(device)).sum(), (xr, yr))
    n1, n2 = rel_err(g1, want["grad_p1"]), rel_err(g2, want["grad_p2"])
    print(f"{shape} cut={cut}: gradient error restatement(fp32) p1 {e1:.2e} p2 {e2:.2e}, device p1 {n1:.2e} p2 {n2:.2e}")
    assert n1 <= max(4.0 * e1, 1e-5) and n2 <= max(4.0 * e2, 1e-5), (n1, e1, n2, e2)
    if xl is not None:  # padded points get gradient 0
        for n in range(shape[0]):
            assert not g1[n, int(xl[n]):].any() and not g2[n, int(yl[n]):].any()


def test_points_without_a_finite_neighbour_are_not_silenced(device):
    x, y = clouds((1, 3, 70, 3, 8))
    x, y = x.to(device).clone(), y.to(device).clone()
    x[0, 2, 1] = float("nan")
    y[0, 9] = float("nan")
    xr, yr = x.requires_grad_(True), y.requires_grad_(True)
    d, raw = ops._knn_points_torch(xr, yr, None, None, 8)
    assert torch.isnan(d[0, 2]).all() and (raw[0, 2] == -1).all()
    assert torch.isfinite(d[0, :2]).all() and (raw[0, :2] != 9).all() and (raw[0, :2] >= 0).all()
    g1, g2 = torch.autograd.grad(d[0, :2].sum(), (xr, yr))
    assert torch.isfinite(g1).all() and torch.isfinite(g2).all() and not g1[0, 2].any() and not g2[0, 9].any()
    # four database points of which the last is NaN, K = 4: the last slot finds nothing below +inf
    d, raw = ops._knn_points_torch(x.detach()[:, :2], y.detach()[:, 6:10], None, None, 4)
    assert torch.isfinite(d[0, :, :3]).all() and (raw[0, :, :3] >= 0).all() and (raw[0, :, :3] != 3).all()
    assert torch.isinf(d[0, :, 3]).all() and (raw[0, :, 3] == -1).all()


def test_return_nn_and_knn_gather(device):
    shape = (2, 33, 70, 5, 8)
    x, y = clouds(shape)
    xl, yl = lengths(shape, True)
    xr, yr = x.to(device).requires_grad_(True), y.to(device).requires_grad_(True)
    r = ops.knn_points(xr, yr, xl.to(device), yl.to(device), K=8, return_nn=True)
    assert tuple(r.knn.shape) == (2, 33, 8, 5)
    idx = r.idx.cpu()
    for n in range(2):
        k = min(8, int(yl[n]))
        assert torch.equal(r.knn[n, :, :k].cpu(), y[n][idx[n, :, :k]]) and not r.knn[n, :, k:].any()
    assert torch.equal(ops.knn_gather(yr, r.idx, yl.to(device)), r.knn)
    assert torch.equal(ops.knn_gather(yr, r.idx).cpu(), y[torch.arange(2)[:, None, None], idx])
    # gradient reaches p2 through dists and through knn
    (gd,) = torch.autograd.grad(r.dists.sum(), yr, retain_graph=True)
    (gk,) = torch.autograd.grad(r.knn.sum(), yr, retain_graph=True)
    assert gd.any() and gk.any()
    count = torch.zeros((2, 70))
    for n in range(2):
        k = min(8, int(yl[n]))
        count[n] = torch.bincount(idx[n, :, :k].reshape(-1), minlength=70).float()
    assert torch.equal(gk.cpu(), count[:, :, None].expand(2, 70, 5))


def test_float64_on_the_device(device):
    shape = (2, 64, 65, 3, 4)
    x, y = clouds(shape)
    want = reference(shape, False)
    r = ops.knn_points(x.to(device).double(), y.to(device).double(), K=4)
    assert r.dists.dtype == torch.float64 and torch.equal(r.idx.cpu(), want["idx"])
    assert_close(r.dists, want["dists"], rtol=1e-12, atol_rel=1e-13, name="dists64")


def test_calls_are_bitwise_reproducible(device):
    """Two forward + backward runs: identical bits for dists, idx, grad_p1 and grad_p2 (the
    neighbours are indexed, so autograd's backward is a sorted index_put_, not float atomics)."""
    for shape in ((2, 64, 65, 3, 4), (2, 257, 1025, 3, 16), (2, 33, 70, 5, 8)):
        x, y = clouds(shape)
        xl, yl = lengths(shape, True)
        runs = []
        for _ in range(2):
            xr, yr = x.to(device).requires_grad_(True), y.to(device).requires_grad_(True)
            r = ops.knn_points(xr, yr, xl.to(device), yl.to(device), K=shape[4])
            g1, g2 = torch.autograd.grad((r.dists * cotangent(shape).to(device)).sum(), (xr, yr))
            runs.append((r.dists.detach(), r.idx, g1, g2))
        assert all(torch.equal(a, b) for a, b in zip(*runs)), shape


@pytest.mark.parametrize("size", [(1, 6, 80, 3, 65), (2, 6, 20, 33, 4)], ids=["K65", "D33"])
def test_large_k_and_d_match_float64(size, device):
    N, P1, P2, D, K = size
    g = torch.Generator().manual_seed(11)
    x, y = torch.rand((N, P1, D), generator=g), torch.rand((N, P2, D), generator=g)
    want_d, want_j = ref_knn(x, y, None, None, K)
    r = ops.knn_points(x.to(device), y.to(device), K=K)
    assert r.dists.dtype == torch.float32 and r.dists.device.type == "cuda"
    assert torch.equal(r.idx.cpu(), want_j.clamp(min=0))
    assert_close(r.dists, want_d, name="dists")


def test_the_forward_does_not_synchronise_with_the_host(device):
    """Forward with lengths and return_nn under torch's sync debug mode: a host read (of a length, a
    count, an index) would raise.  The backward is autograd's own and is not covered."""
    shape = (2, 257, 1025, 3, 16)
    x, y = clouds(shape)
    xl, yl = lengths(shape, True)
    xr, yr = x.to(device).requires_grad_(True), y.to(device).requires_grad_(True)
    xl, yl = xl.to(device), yl.to(device)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r = ops.knn_points(xr, yr, xl, yl, K=16, return_nn=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert r.dists.any() and r.knn.any()

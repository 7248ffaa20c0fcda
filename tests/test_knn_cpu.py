"""knn_points / knn_gather without a GPU: the torch composition (_knn_points_torch, what CPU tensors
take) against the float64 brute force of knn_cases.py on every shape and both length settings, the
lowest-index rule on the planted ties, the padding rules, knn_gather, return_nn, gradients against
float64 autograd, argument validation and the pytorch3d.ops shim."""
import os

import pytest
import torch

from conftest import assert_close
from knn_cases import DUP, SHAPES, clouds, cotangent, lengths, planted, ref_knn, reference
from mesh_loss_cases import rel_err
from pertrenderer_amd import build_native
from pertrenderer_amd.renderer import ops

IDS = ["-".join(map(str, s)) for s in SHAPES]


@pytest.mark.parametrize("cut", [False, True], ids=["full", "cut"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_composition_matches_float64(shape, cut):
    x, y = clouds(shape)
    xl, yl = lengths(shape, cut)
    want = reference(shape, cut)
    d, j = ops._knn_points_torch(x, y, xl, yl, shape[4])
    assert d.dtype == torch.float32 and j.dtype == torch.int64 and tuple(d.shape) == (shape[0], shape[1], shape[4])
    assert torch.equal(j, want["idx"])
    assert_close(d, want["dists"], name="dists")
    assert (d[:, :, 1:] >= d[:, :, :-1]).logical_or(j[:, :, 1:] < 0).all()  # ascending over the live slots


@pytest.mark.parametrize("cut", [False, True], ids=["full", "cut"])
@pytest.mark.parametrize("shape", [s for s in SHAPES if planted(s)], ids=lambda s: "-".join(map(str, s)))
def test_planted_ties_come_out_in_ascending_index(shape, cut):
    x, y = clouds(shape)
    xl, yl = lengths(shape, cut)
    r = ops.knn_points(x, y, xl, yl, K=shape[4])
    for n in range(shape[0]):
        nx, ny = (shape[1], shape[2]) if xl is None else (int(xl[n]), int(yl[n]))
        live = [c for c in planted(shape) if c < ny][:shape[4]]
        if nx < 2 or len(live) < 2:
            continue
        assert r.idx[n, 1, :len(live)].tolist() == live and live[0] == DUP[0]
        assert not r.dists[n, 1, :len(live)].any()  # exactly 0.0


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_padding(shape):
    x, y = clouds(shape)
    xl, yl = lengths(shape, True)
    N, P1, P2, _, K = shape
    d, raw = ops._knn_points_torch(x, y, xl, yl, K)
    r = ops.knn_points(x, y, xl, yl, K=K)
    assert r.idx.dtype == torch.int64 and torch.equal(r.idx, raw.clamp(min=0)) and torch.equal(r.dists, d)
    for n in range(N):
        nx, k = int(xl[n]), min(K, int(yl[n]))
        assert (raw[n, nx:] == -1).all() and not d[n, nx:].any() and not r.idx[n, nx:].any()
        assert (raw[n, :, k:] == -1).all() and not d[n, :, k:].any() and not r.idx[n, :, k:].any()
        assert (raw[n, :nx, :k] >= 0).all() and (raw[n, :nx, :k] < int(yl[n])).all()
    # K > P2 without lengths: the slots past P2 are padding
    if K > P2:
        d, raw = ops._knn_points_torch(x, y, None, None, K)
        assert (raw[:, :, P2:] == -1).all() and not d[:, :, P2:].any() and (raw[:, :, :P2] >= 0).all()


def test_lengths_are_clamped():
    x, y = clouds((2, 5, 3, 3, 5))
    a = ops._knn_points_torch(x, y, torch.tensor([9, -2]), torch.tensor([-1, 7]), 5)
    b = ops._knn_points_torch(x, y, torch.tensor([5, 0]), torch.tensor([0, 3]), 5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert (a[1][0] == -1).all() and (a[1][1] == -1).all()  # an empty database, an empty query cloud


def test_non_finite_points():
    """A NaN database point is never chosen; a slot that finds nothing below +inf gets NaN for a NaN
    query, else +inf, raw idx -1 and no gradient."""
    x, y = clouds((1, 3, 70, 3, 8))
    x, y = x.clone(), y.clone()
    x[0, 2, 1] = float("nan")
    y[0, 9] = float("nan")
    xr, yr = x.requires_grad_(True), y.requires_grad_(True)
    d, raw = ops._knn_points_torch(xr, yr, None, None, 8)
    assert torch.isnan(d[0, 2]).all() and (raw[0, 2] == -1).all()
    assert torch.isfinite(d[0, :2]).all() and (raw[0, :2] != 9).all() and (raw[0, :2] >= 0).all()
    g1, g2 = torch.autograd.grad(d[0, :2].sum(), (xr, yr))
    assert torch.isfinite(g1).all() and torch.isfinite(g2).all() and not g1[0, 2].any() and not g2[0, 9].any()
    d, raw = ops._knn_points_torch(x.detach()[:, :2], torch.full_like(y.detach(), float("nan")), None, None, 2)
    assert torch.isinf(d).all() and (d > 0).all() and (raw == -1).all()


def test_knn_gather_with_and_without_lengths():
    g = torch.Generator().manual_seed(3)
    x = torch.rand((2, 7, 4), generator=g)
    idx = torch.randint(0, 7, (2, 5, 3), generator=g)
    out = ops.knn_gather(x, idx)
    assert tuple(out.shape) == (2, 5, 3, 4)
    for n in range(2):
        for l in range(5):
            for k in range(3):
                assert torch.equal(out[n, l, k], x[n, idx[n, l, k]])
    cut = ops.knn_gather(x, idx, torch.tensor([2, 0]))
    assert torch.equal(cut[0, :, :2], out[0, :, :2]) and not cut[0, :, 2:].any() and not cut[1].any()
    assert torch.equal(ops.knn_gather(x, idx.to(torch.int32)), out)
    xr = x.clone().requires_grad_(True)
    ops.knn_gather(xr, idx, torch.tensor([2, 3])).sum().backward()
    want = torch.zeros_like(x)
    for n, k_live in enumerate((2, 3)):
        for l in range(5):
            for k in range(k_live):
                want[n, idx[n, l, k]] += 1.0
    assert torch.equal(xr.grad, want)
    for bad in (lambda: ops.knn_gather(x[0], idx), lambda: ops.knn_gather(x, idx[:1]),
                lambda: ops.knn_gather(x, idx.float()), lambda: ops.knn_gather(x, idx, torch.tensor([1]))):
        with pytest.raises(ValueError):
            bad()


def test_return_nn_equals_direct_indexing():
    shape = (2, 33, 70, 5, 8)
    x, y = clouds(shape)
    xl, yl = lengths(shape, True)
    r = ops.knn_points(x, y, xl, yl, K=8, return_nn=True)
    assert ops.knn_points(x, y, xl, yl, K=8).knn is None
    assert tuple(r.knn.shape) == (2, 33, 8, 5)
    for n in range(2):
        k = min(8, int(yl[n]))
        assert torch.equal(r.knn[n, :, :k], y[n][r.idx[n, :, :k]]) and not r.knn[n, :, k:].any()
    assert r._fields == ("dists", "idx", "knn")


@pytest.mark.parametrize("cut", [False, True], ids=["full", "cut"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gradients_match_float64_autograd(shape, cut):
    x, y = clouds(shape)
    xl, yl = lengths(shape, cut)
    want = reference(shape, cut)
    xr, yr = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    r = ops.knn_points(xr, yr, xl, yl, K=shape[4])
    assert not r.idx.requires_grad
    g1, g2 = torch.autograd.grad((r.dists * cotangent(shape)).sum(), (xr, yr))
    e1, e2 = want["err"]
    assert rel_err(g1, want["grad_p1"]) <= max(4.0 * e1, 1e-5) and rel_err(g2, want["grad_p2"]) <= max(4.0 * e2, 1e-5)
    if xl is not None:
        for n in range(shape[0]):
            assert not g1[n, int(xl[n]):].any() and not g2[n, int(yl[n]):].any()
    # float64 inputs: the composition in float64 is the restatement
    r = ops.knn_points(x.double(), y.double(), xl, yl, K=shape[4])
    assert r.dists.dtype == torch.float64 and torch.equal(r.idx, want["idx"].clamp(min=0))
    assert_close(r.dists, want["dists"], rtol=1e-12, atol_rel=1e-13, name="dists64")


def test_gradient_reaches_p2_through_knn():
    x, y = clouds((2, 33, 70, 5, 8))
    yr = y.clone().requires_grad_(True)
    r = ops.knn_points(x, yr, K=8, return_nn=True)
    (g,) = torch.autograd.grad(r.knn.sum(), yr)
    count = torch.zeros((2, 70))
    for n in range(2):
        count[n] = torch.bincount(r.idx[n].reshape(-1), minlength=70).float()
    assert torch.equal(g, count[:, :, None].expand(2, 70, 5))


def test_chunked_queries_agree(monkeypatch):
    shape = (2, 64, 65, 3, 4)
    x, y = clouds(shape)
    whole = ops._knn_points_torch(x, y, None, None, 4)
    monkeypatch.setattr(ops, "_TORCH_CHUNK", 65 * 7)  # 7 queries per chunk
    parts = ops._knn_points_torch(x, y, None, None, 4)
    assert torch.equal(whole[0], parts[0]) and torch.equal(whole[1], parts[1])


def test_arguments_are_validated():
    x, y = clouds((2, 5, 3, 3, 5))
    ok = torch.tensor([1, 2])
    bad_calls = [
        lambda: ops.knn_points(x[0], y),                                  # not 3-D
        lambda: ops.knn_points(x, y[0]),
        lambda: ops.knn_points(x.long(), y.long()),                        # not floating point
        lambda: ops.knn_points(x, y.double()),                             # dtypes differ
        lambda: ops.knn_points(x, y.to("meta")),                           # devices differ
        lambda: ops.knn_points(x, y[:1]),                                  # N differs
        lambda: ops.knn_points(x, y[:, :, :2]),                            # D differs
        lambda: ops.knn_points(x, y, K=0),
        lambda: ops.knn_points(x, y, K=-1),
        lambda: ops.knn_points(x, y, K=2.0),
        lambda: ops.knn_points(x, y, K=True),
        lambda: ops.knn_points(x, y, lengths1=torch.tensor([1])),          # shape
        lambda: ops.knn_points(x, y, lengths2=torch.tensor([[1, 2]])),
        lambda: ops.knn_points(x, y, lengths1=torch.tensor([1.0, 2.0])),   # dtype
        lambda: ops.knn_points(x, y, lengths2=torch.tensor([True, False])),
        lambda: ops.knn_points(x, y, lengths1=ok.to("meta")),              # device
        lambda: ops.knn_points(x, y, lengths2=ok.to("meta")),
        lambda: ops.knn_points(x, y, lengths2=[1, 2]),
        lambda: ops.knn_points(x, y, version=4),
        lambda: ops.knn_points(x, y, version=-2),
        lambda: ops.knn_points(x, y, version="1"),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {i} was accepted")


def test_version_and_return_sorted_are_accepted_and_ignored():
    x, y = clouds((1, 3, 70, 3, 8))
    base = ops.knn_points(x, y, K=8)
    for v in (-1, 0, 1, 2, 3):
        r = ops.knn_points(x, y, K=8, version=v, return_sorted=False)
        assert torch.equal(r.dists, base.dists) and torch.equal(r.idx, base.idx)
    r = ops.knn_points(x, y, torch.tensor([3], dtype=torch.int32), torch.tensor([70], dtype=torch.int32), 8)
    assert torch.equal(r.idx, base.idx)  # any integer dtype for the lengths


def test_ref_knn_is_the_documented_order():
    """The restatement itself on a hand-made case: ties by index, padding."""
    x = torch.tensor([[[0.0, 0.0], [1.0, 0.0]]])
    y = torch.tensor([[[1.0, 0.0], [0.0, 1.0], [1.0, 0.0], [5.0, 5.0]]])
    d, j = ref_knn(x, y, torch.tensor([2]), torch.tensor([3]), 4)
    assert j.tolist() == [[[0, 1, 2, -1], [0, 2, 1, -1]]]
    assert d.tolist() == [[[1.0, 1.0, 1.0, 0.0], [0.0, 0.0, 2.0, 0.0]]]


def test_shim_exports():
    import pytorch3d.ops
    assert pytorch3d.ops.knn_points is ops.knn_points and pytorch3d.ops.knn_gather is ops.knn_gather
    from pytorch3d.ops import knn_gather, knn_points, sample_points_from_meshes  # noqa: F401


def test_chamfer_uses_the_shared_d2():
    with open(os.path.join(build_native.CSRC, "pr_chamfer.hip")) as fh:
        assert "dist2_3(" in fh.read()


@pytest.mark.parametrize("size", [(1, 6, 80, 3, 65), (2, 6, 20, 33, 4), (1, 4, 9, 2, 9)], ids=["K65", "D33", "K-eq-P2"])
def test_large_k_and_d_match_float64(size):
    """K and D beyond what a tiled kernel would cap (64, 32), and K = P2."""
    N, P1, P2, D, K = size
    g = torch.Generator().manual_seed(11)
    x, y = torch.rand((N, P1, D), generator=g), torch.rand((N, P2, D), generator=g)
    y[:, 5] = y[:, 2]  # a tie
    want_d, want_j = ref_knn(x, y, None, None, K)
    r = ops.knn_points(x, y, K=K)
    assert torch.equal(r.idx, want_j.clamp(min=0))
    assert_close(r.dists, want_d, name="dists")

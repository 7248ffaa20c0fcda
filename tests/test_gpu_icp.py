"""The native iterative_closest_point / corresponding_points_alignment (csrc/pr_icp.hip) against
the float64 restatement of tests/icp_cases.py, the torch composition on the device, bitwise
reproducibility over PR_ICP_CHECK_EVERY and PR_ICP_SPLITS, the NaN / empty-cloud / tie rules, and no
host read inside a batch of iterations.

Tolerances.  The neighbour indices of every iteration equal float64's (icp_cases asserts a margin
float32 cannot cross).  R, T, s of every history entry, rmse and Xt: max-abs over max-abs against the
float64 restatement, at most 4x the error of the restatement's own float32 run on that case, floored
at 1e-5 (the rule of test_gpu_mesh_losses.py; icp_cases asserts the float32 run stays under 2e-5).

Measured on an MI355X (float32 restatement / native, max-abs over max-abs; the native figures are the
same bits for the default split count, PR_ICP_SPLITS=1 and PR_ICP_SPLITS=3):
    one-65-513    R 1.31e-07 / 2.96e-08, T 5.14e-07 / 5.04e-08, s 0 / 0, rmse 1.31e-07 / 2.46e-08, Xt 1.19e-07 / 8.89e-08
    batch-64-512  R 1.66e-07 / 2.96e-08, T 6.57e-07 / 4.17e-08, s 0 / 0, rmse 7.33e-07 / 3.53e-08, Xt 1.96e-07 / 1.13e-07
    two-257-1025  R 1.39e-07 / 2.84e-08, T 3.01e-06 / 3.37e-08, s 0 / 0, rmse 3.34e-07 / 2.14e-08, Xt 2.07e-07 / 1.34e-07
    two-257-1025, estimate_scale
                  R 1.51e-07 / 2.95e-08, T 3.83e-06 / 2.89e-08, s 2.72e-07 / 2.96e-08, rmse 3.27e-07 / 3.04e-08, Xt 4.22e-07 / 1.22e-07
    weighted alignment (3 x 300, lengths 300 / 257 / 40, weights in [0, 2]; the composition on the device third)
                  R 4.16e-07 / 2.80e-08 / 5.53e-07, T 7.28e-08 / 1.89e-08 / 1.41e-07, with scale s 2.18e-08 / 7.02e-09 / 2.30e-08
All below the 1e-5 floor."""
import warnings

import numpy as np
import pytest
import torch

import icp_cases as ic
from pertrenderer_amd.renderer import Pointclouds
from pertrenderer_amd.renderer import alignment as AL

pytestmark = pytest.mark.gpu


def _lengths(lens, full, device):
    return None if all(k == full for k in lens) else torch.tensor(lens, dtype=torch.int64, device=device)


def _native(scene, device, iters, thr, **kw):
    X, Y, lx, ly = scene
    x, y = torch.from_numpy(X).to(device), torch.from_numpy(Y).to(device)
    return AL._icp_native(x, y, _lengths(lx, X.shape[1], device), _lengths(ly, Y.shape[1], device), None, iters, thr,
                          kw.get("estimate_scale", False), False, False, keep_indices=True)


def _as_numpy(out):
    conv, rmse, Xt, RTs, hist, idx = out
    return dict(converged=conv, rmse=rmse.cpu().numpy(), Xt=Xt.cpu().numpy(), idx=idx.cpu().numpy(),
                R=np.stack([t.R.cpu().numpy() for t in hist]), T=np.stack([t.T.cpu().numpy() for t in hist]),
                s=np.stack([t.s.cpu().numpy() for t in hist]))


@pytest.mark.parametrize("splits", [None, "1", "3"], ids=["default", "unsplit", "3-ranges"])
@pytest.mark.parametrize("name", list(ic.SHAPES))
def test_fixed_count_matches_float64(name, splits, device, monkeypatch):
    if splits is None:
        monkeypatch.delenv("PR_ICP_SPLITS", raising=False)
    else:
        monkeypatch.setenv("PR_ICP_SPLITS", splits)
    scene, ref, err32 = ic.reference(name)
    got = _as_numpy(_native(scene, device, ic.FIXED_ITERATIONS, -1.0))
    assert got["converged"] is False and got["idx"].shape == ref["idx"].shape
    assert np.array_equal(got["idx"], ref["idx"])
    for q in ic.QUANTITIES:
        e = ic.rel_err(got[q], ref[q])
        print(f"{name} splits={splits} {q}: reference(fp32) {err32[q]:.2e} native {e:.2e}")
        assert e <= max(4.0 * err32[q], 1e-5), (q, e, err32[q])
    assert got["Xt"].dtype == np.float32 and got["rmse"].shape == (scene[0].shape[0],)


def test_estimate_scale_matches_float64(device, monkeypatch):
    monkeypatch.delenv("PR_ICP_SPLITS", raising=False)
    scene, ref, err32 = ic.reference("two-257-1025", True)
    got = _as_numpy(_native(scene, device, ic.FIXED_ITERATIONS, -1.0, estimate_scale=True))
    assert np.array_equal(got["idx"], ref["idx"])
    for q in ic.QUANTITIES:
        e = ic.rel_err(got[q], ref[q])
        print(f"scale {q}: reference(fp32) {err32[q]:.2e} native {e:.2e}")
        assert e <= max(4.0 * err32[q], 1e-5), (q, e, err32[q])
    assert np.abs(ref["s"] - 1).max() > 1e-4  # the scale is estimated, not 1


def _bits(sol):
    return [sol.rmse, sol.Xt if torch.is_tensor(sol.Xt) else sol.Xt.points_padded(), sol.RTs.R, sol.RTs.T, sol.RTs.s] + \
           [t for h in sol.t_history for t in h]


def test_early_exit_count_and_batch_size_independence(device, monkeypatch):
    monkeypatch.delenv("PR_ICP_SPLITS", raising=False)
    (X, Y, lx, ly), ref = ic.early_reference()
    Xp = Pointclouds([torch.from_numpy(X[n, :k]).to(device) for n, k in enumerate(lx)])
    Yp = Pointclouds([torch.from_numpy(Y[n, :k]).to(device) for n, k in enumerate(ly)])
    kw = dict(max_iterations=ic.EARLY["max_iterations"], relative_rmse_thr=ic.EARLY["thr"])
    runs = []
    for every in ("1", "3", "8", str(ic.EARLY["max_iterations"]), "8"):
        monkeypatch.setenv("PR_ICP_CHECK_EVERY", every)
        sol = AL.iterative_closest_point(Xp, Yp, **kw)
        assert sol.converged is True and ref["converged"] and len(sol.t_history) == len(ref["R"])
        assert isinstance(sol.Xt, Pointclouds) and sol.Xt.npoints == lx
        runs.append(_bits(sol))
    assert 3 < len(ref["R"]) < 8  # the batch of 3 stops in its third batch, the batch of 8 in its first
    for other in runs[1:]:
        assert len(other) == len(runs[0]) and all(torch.equal(a, b) for a, b in zip(runs[0], other))
    assert ic.rel_err(runs[0][0].cpu().numpy(), ref["rmse"]) <= 1e-5
    assert ic.rel_err(runs[0][2].cpu().numpy(), ref["R"][-1]) <= 1e-5
    # the composition on the device stops at the same count
    monkeypatch.setattr(AL, "NATIVE_ICP", False)
    comp = AL.iterative_closest_point(Xp, Yp, **kw)
    assert comp.converged is True and len(comp.t_history) == len(ref["R"])
    assert ic.rel_err(comp.RTs.T.cpu().numpy(), runs[0][3].cpu().numpy()) <= 1e-5


def test_max_iterations_reached_and_init_transform(device):
    X, Y, _, _ = ic.scene(1, 65, 513, 0)
    x, y = torch.from_numpy(X).to(device), torch.from_numpy(Y).to(device)
    R0 = torch.from_numpy(ic.rotation((1, 2, 3), -10.0)).float()[None].to(device)
    init = AL.SimilarityTransform(R0, torch.full((1, 3), 0.02, device=device), torch.ones(1, device=device))
    sol = AL.iterative_closest_point(x, y, init_transform=init, max_iterations=4, relative_rmse_thr=-1.0)
    ref = ic.icp(X.astype(np.float64), Y.astype(np.float64), init=[t.cpu().numpy() for t in init], max_iterations=4, thr=-1.0)
    assert sol.converged is False and len(sol.t_history) == 4
    assert ic.rel_err(sol.RTs.R.cpu().numpy(), ref["R"][-1]) <= 1e-5 and ic.rel_err(sol.Xt.cpu().numpy(), ref["Xt"]) <= 1e-5
    zero = AL.iterative_closest_point(x, y, init_transform=init, max_iterations=0)
    assert zero.rmse is None and zero.t_history == [] and torch.equal(zero.Xt, AL._apply_similarity_transform(x, *init))


@pytest.mark.parametrize("scale", [1.0, 1.3])
def test_alignment_recovers_a_copy(scale, device):
    X, Y, R, T = ic.rigid_copy(scale=scale)
    out = AL.corresponding_points_alignment(torch.from_numpy(X).to(device), torch.from_numpy(Y).to(device), estimate_scale=scale != 1.0)
    Rn = out.R.double().cpu()
    assert out.R.dtype == torch.float32 and out.R.shape == (2, 3, 3) and out.T.shape == (2, 3) and out.s.shape == (2,)
    assert np.abs(Rn.numpy() - R).max() <= 2e-6 and np.abs(out.T.cpu().numpy() - T).max() <= 2e-6
    assert np.abs(out.s.cpu().numpy() - scale).max() <= 2e-6
    assert (Rn @ Rn.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max() <= 1e-6
    assert (torch.det(Rn) - 1).abs().max() <= 1e-6


def test_alignment_reflection(device):
    X, Y, R, _ = ic.rigid_copy(mirror=True)
    x, y = torch.from_numpy(X).to(device), torch.from_numpy(Y).to(device)
    free = AL.corresponding_points_alignment(x, y, allow_reflection=True).R.double().cpu()
    assert np.abs(free.numpy() - R).max() <= 2e-6 and (torch.det(free) + 1).abs().max() <= 1e-6
    proper = AL.corresponding_points_alignment(x, y).R.double().cpu()
    assert (torch.det(proper) - 1).abs().max() <= 1e-6
    assert np.abs(proper.numpy() - ic.align(X.astype(np.float64), Y.astype(np.float64))[0]).max() <= 1e-5


def test_alignment_weights_and_lengths(device, monkeypatch):
    rng = np.random.RandomState(3)
    X, Y = rng.uniform(-1, 1, (3, 300, 3)).astype(np.float32), rng.uniform(-1, 1, (3, 300, 3)).astype(np.float32)
    w = rng.uniform(0, 2, (3, 300)).astype(np.float32)
    lengths = [300, 257, 40]
    Xp = Pointclouds([torch.from_numpy(X[n, :k]).to(device) for n, k in enumerate(lengths)])
    Yp = Pointclouds([torch.from_numpy(Y[n, :k]).to(device) for n, k in enumerate(lengths)])
    wl = [torch.from_numpy(w[n, :k]).to(device) for n, k in enumerate(lengths)]
    for scale in (False, True):
        ref = ic.align(X.astype(np.float64), Y.astype(np.float64), w.astype(np.float64), estimate_scale=scale, lengths=lengths)
        ref32 = ic.align(X, Y, w, estimate_scale=scale, lengths=lengths)
        nat_out = AL.corresponding_points_alignment(Xp, Yp, weights=wl, estimate_scale=scale)
        monkeypatch.setattr(AL, "NATIVE_ICP", False)
        comp = AL.corresponding_points_alignment(Xp, Yp, weights=wl, estimate_scale=scale)
        monkeypatch.setattr(AL, "NATIVE_ICP", True)
        for a, c, b, b32, q in zip(nat_out, comp, ref, ref32, "RTs"):
            e, e32, ec = ic.rel_err(a.cpu().numpy(), b), ic.rel_err(b32, b), ic.rel_err(c.cpu().numpy(), b)
            print(f"weights scale={scale} {q}: reference(fp32) {e32:.2e} native {e:.2e} composition {ec:.2e}")
            assert e <= max(4.0 * e32, 1e-5), (q, e, e32)
            assert ec <= max(4.0 * e32, 1e-5), (q, ec, e32)
        # w^2 in the covariance: the restatement with sqrt(w) is another rotation
        assert np.abs(ic.align(X.astype(np.float64), Y.astype(np.float64), np.sqrt(w.astype(np.float64)), lengths=lengths)[0] - ref[0]).max() > 1e-3
    # no weights, ragged lengths: the rows past a length carry weight 0
    ref = ic.align(X.astype(np.float64), Y.astype(np.float64), None, lengths=lengths)
    out = AL.corresponding_points_alignment(Xp, Yp)
    assert ic.rel_err(out.R.cpu().numpy(), ref[0]) <= 1e-5 and ic.rel_err(out.T.cpu().numpy(), ref[1]) <= 1e-5
    again = AL.corresponding_points_alignment(Xp, Yp)
    assert all(torch.equal(a, b) for a, b in zip(out, again))


def _run(X, Y, lx, ly, device, iters=3):
    x, y = torch.from_numpy(X).to(device), torch.from_numpy(Y).to(device)
    return AL._icp_native(x, y, _lengths(lx, X.shape[1], device), _lengths(ly, Y.shape[1], device), None, iters, -1.0, False, False,
                          False, keep_indices=True)


@pytest.mark.parametrize("splits", ["1", "2"])
def test_empty_cloud_tie_and_nan_rules(splits, device, monkeypatch):
    monkeypatch.setenv("PR_ICP_SPLITS", splits)
    X, Y, lx, ly = ic.scene(2, 16, 40, 0)
    eye = torch.eye(3, device=device)
    # an X cloud of length 0: finite orthonormal R, T = 0, s = 1, rmse 0; the other cloud as without it
    conv, rmse, Xt, RTs, hist, idx = _run(X, Y, [16, 0], ly, device)
    ref = ic.icp(X, Y, [16, 0], ly, max_iterations=3, thr=-1.0, check_margin=False)
    assert torch.isfinite(RTs.R[1]).all() and (RTs.R[1] @ RTs.R[1].T - eye).abs().max() <= 1e-6
    assert torch.equal(RTs.T[1], torch.zeros(3, device=device)) and RTs.s[1] == 1 and rmse[1] == 0
    assert ic.rel_err(RTs.R[0].cpu().numpy(), ref["R"][-1][0]) <= 1e-5 and conv is False and len(hist) == 3
    assert np.array_equal(idx.cpu().numpy(), ref["idx"]) and (idx[:, 1] == -1).all()
    # an empty Y cloud: its X cloud's live queries find no neighbour -> NaN, not dropped silently
    conv, rmse, Xt, RTs, hist, idx = _run(X, Y, lx, [40, 0], device)
    assert torch.isnan(RTs.R[1]).all() and torch.isnan(RTs.T[1]).all() and torch.isnan(RTs.s[1]) and torch.isnan(rmse[1])
    assert torch.isfinite(RTs.R[0]).all() and torch.isfinite(rmse[0]) and (idx[:, 1] == -1).all() and conv is False
    # a NaN point of Y is never chosen
    Yn = Y.copy()
    Yn[0, 3] = np.nan
    idx = _run(X, Yn, lx, ly, device, 2)[5]
    assert not (idx[:, 0] == 3).any() and (idx[:, 0, :lx[0]] >= 0).all()
    # a NaN query poisons its cloud only
    Xn = X.copy()
    Xn[1, 2, 0] = np.nan
    RTs = _run(Xn, Y, lx, ly, device)[3]
    assert torch.isnan(RTs.R[1]).all() and torch.isfinite(RTs.R[0]).all()
    # a planted tie: two copies of a Y point that is some query's neighbour, 20 apart (in different
    # ranges when split): the lowest index wins
    j = int(ic.icp(X, Y, lx, ly, max_iterations=1, thr=-1.0, check_margin=False)["idx"][0, 0, 0])
    lo, hi = sorted((j, (j + 20) % 40))
    Yt = Y.copy()
    Yt[0, lo] = Yt[0, hi] = Y[0, j]
    idx = _run(X, Yt, lx, ly, device)[5].cpu().numpy()
    ref = ic.icp(X, Yt, lx, ly, max_iterations=3, thr=-1.0, check_margin=False)
    assert np.array_equal(idx, ref["idx"]) and (idx[:, 0] == lo).any() and not (idx[:, 0] == hi).any()


def test_tiny_clouds(device):
    one = AL.iterative_closest_point(torch.tensor([[[0.1, 0.2, 0.3]]], device=device), torch.tensor([[[0.5, -0.2, 0.1]]], device=device),
                                     max_iterations=3, relative_rmse_thr=-1.0)
    assert torch.allclose(one.Xt.cpu(), torch.tensor([[[0.5, -0.2, 0.1]]]), atol=1e-6) and one.rmse.abs().max() <= 1e-6
    R = one.RTs.R[0].cpu()
    assert torch.allclose(R @ R.T, torch.eye(3), atol=1e-6) and len(one.t_history) == 3
    X, Y, _, _ = ic.scene(1, 4, 4, 0)
    four = AL.iterative_closest_point(torch.from_numpy(X).to(device), torch.from_numpy(Y).to(device), max_iterations=3, relative_rmse_thr=-1.0)
    ref = ic.icp(X.astype(np.float64), Y.astype(np.float64), max_iterations=3, thr=-1.0, check_margin=False)
    assert ic.rel_err(four.Xt.cpu().numpy(), ref["Xt"]) <= 1e-4 and ic.rel_err(four.rmse.cpu().numpy(), ref["rmse"]) <= 1e-4


def test_no_host_read_in_a_batch(device):
    X, Y, _, _ = ic.scene(1, 65, 513, 0)
    x, y = torch.from_numpy(X).to(device), torch.from_numpy(Y).to(device)
    w = torch.rand((1, 65), device=device)
    run = AL._IcpRun(x, y, None, None, None, 8, -1.0, False, False)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        run.enqueue(8)
        out = AL.corresponding_points_alignment(x, y[:, :65], weights=w, estimate_scale=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert run.flags.tolist() == [0, 8] and torch.isfinite(out.R).all()


def test_an_input_that_requires_grad_takes_the_composition(device):
    X, Y, _, _ = ic.scene(1, 16, 40, 0)
    x, y = torch.from_numpy(X).to(device).requires_grad_(True), torch.from_numpy(Y).to(device)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sol = AL.iterative_closest_point(x, y, max_iterations=2, relative_rmse_thr=-1.0)
        # (sum Xt itself is P Ymu, which does not depend on X)
        (sol.Xt ** 2).sum().backward()
        out = AL.corresponding_points_alignment(x, y[:, :16])
    assert sol.Xt.requires_grad and x.grad is not None and torch.isfinite(x.grad).all() and x.grad.abs().sum() > 0
    assert out.R.requires_grad
    with torch.no_grad():  # grad mode off: the native path, the same numbers
        nat_sol = AL.iterative_closest_point(x, y, max_iterations=2, relative_rmse_thr=-1.0)
    assert not nat_sol.Xt.requires_grad and ic.rel_err(nat_sol.Xt.cpu().numpy(), sol.Xt.detach().cpu().numpy()) <= 1e-5

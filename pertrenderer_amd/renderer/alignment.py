"""PyTorch3D 0.4.0 ``pytorch3d.ops.corresponding_points_alignment`` and ``iterative_closest_point``:
the rigid (or similarity) transform that takes one point cloud onto another, from given
correspondences (Umeyama) or by iterating nearest neighbours (ICP).  Row vectors: X R ~ Y.

On a ROCm device with float32 points of dimension 3, when no input requires grad (or grad mode is
off), both run on the native kernels (csrc/pr_icp.hip).  An ICP iteration is two or three launches
(the K = 1 search with the moments fused in, its merge when the database is cut into ranges, one
3 x 3 Jacobi solve per cloud in float64) and reads nothing on the host; iterations are enqueued in
batches of PR_ICP_CHECK_EVERY (default 8), the host reads the 4-byte converged flag once per batch,
and the kernels of the iterations after convergence return at once, so the result does not depend
on the batch size.  Everything else (CPU tensors, other dtypes, other dimensions, inputs that
require grad, PR_NATIVE_ICP=0 or NATIVE_ICP = False) takes the torch composition of the same
formulas with torch.linalg.svd, through which gradients flow as they do in PyTorch3D; there is no
native backward through the SVD.  Parity with PyTorch3D is unpinned (not installable here)."""
import collections
import os
import warnings

import torch

from . import ops as _ops
from .pointclouds import Pointclouds

# read at import, like loss.NATIVE_MESHLOSS; tests/test_gpu_icp.py compares the two paths
NATIVE_ICP = os.environ.get("PR_NATIVE_ICP", "1") == "1"
AMBIGUOUS_ROT_SINGULAR_THR = 1e-15
_MAX_CLOUDS = 65535
_INT32_MAX = 2 ** 31 - 1

SimilarityTransform = collections.namedtuple("SimilarityTransform", "R T s")
ICPSolution = collections.namedtuple("ICPSolution", "converged rmse Xt RTs t_history")


def wmean(x, weight=None, dim=-2, keepdim=True, eps=1e-9):
    """The weighted mean of x (*, P, D) over `dim` with weight (*, P):
    (x w[..., None]).sum(dim) / w[..., None].sum(dim).clamp(eps); weight None: all ones
    (pytorch3d.ops.utils.wmean)."""
    if weight is None:
        weight = torch.ones(x.shape[:-1], dtype=x.dtype, device=x.device)
    if any(xd != wd and xd != 1 and wd != 1 for xd, wd in zip(x.shape[-2::-1], weight.shape[::-1])):
        raise ValueError("wmean: weights are not compatible with the tensor")
    w = weight[..., None]
    return (x * w).sum(dim=dim, keepdim=keepdim) / w.sum(dim=dim, keepdim=keepdim).clamp(eps)


def convert_pointclouds_to_tensor(pcl):
    """(padded (N,P,D), num_points (N,) int64 on the device) of a Pointclouds or a tensor
    (pytorch3d.ops.utils.convert_pointclouds_to_tensor)."""
    if isinstance(pcl, Pointclouds):
        return pcl.points_padded(), pcl.num_points_per_cloud()
    if torch.is_tensor(pcl):
        if pcl.dim() != 3:
            raise ValueError(f"expected a (N,P,D) tensor, got {tuple(pcl.shape)}")
        return pcl, torch.full((pcl.shape[0],), pcl.shape[1], dtype=torch.int64, device=pcl.device)
    raise ValueError(f"The inputs have to be either tensors or Pointclouds objects, got {type(pcl).__name__}")


def _lengths(pcl):
    """The clouds' lengths as Python ints (no host read), and whether any is shorter than the padding."""
    if isinstance(pcl, Pointclouds):
        n = list(pcl.npoints)
        return n, any(k != max(n, default=0) for k in n)
    return [pcl.shape[1]] * pcl.shape[0], False


def _apply_similarity_transform(X, R, T, s):
    return s[:, None, None] * torch.bmm(X, R) + T[:, None, :]


def _native_ok(*tensors):
    t = tensors[0]
    if not (NATIVE_ICP and t.is_cuda and t.shape[2] == 3 and 0 < t.shape[0] <= _MAX_CLOUDS):
        return False
    if any(x.dtype != torch.float32 or x.device != t.device or not 0 < x.shape[1] <= _INT32_MAX for x in tensors):
        return False
    return not (torch.is_grad_enabled() and any(x.requires_grad for x in tensors))


def _align_torch(X, Y, weights, estimate_scale, allow_reflection, eps, num_points=None):
    """The composition: (R, T, s) from padded X, Y (N,P,D) and weights (N,P) or None (then every row
    counts and total = clamp(num_points, 1)).  A cloud whose covariance is not finite gets NaN."""
    N, P, D = X.shape
    Xmu, Ymu = wmean(X, weights, eps=eps), wmean(Y, weights, eps=eps)
    Xc, Yc = X - Xmu, Y - Ymu
    if weights is not None:
        Xc, Yc = Xc * weights[:, :, None], Yc * weights[:, :, None]
        total = weights.sum(1).clamp(eps)
    else:
        n = torch.full((N,), P, dtype=X.dtype, device=X.device) if num_points is None else num_points.to(X.dtype)
        total = n.clamp(1)
    C = torch.bmm(Xc.transpose(1, 2), Yc) / total[:, None, None]
    bad = ~torch.isfinite(C).all(dim=2).all(dim=1)
    eye = torch.eye(D, dtype=X.dtype, device=X.device)[None]
    U, S, Vh = torch.linalg.svd(torch.where(bad[:, None, None], eye, C))
    V = Vh.transpose(1, 2)
    if not X.is_cuda:  # both need a host read
        if num_points is not None and bool((num_points < D + 1).any()):
            warnings.warn("The size of one of the point clouds is <= dim+1. corresponding_points_alignment cannot "
                          "return a unique rotation.")
        if bool((S.abs() <= AMBIGUOUS_ROT_SINGULAR_THR).any()):
            warnings.warn("Excessively low rank of cross-correlation between aligned point clouds. "
                          "corresponding_points_alignment cannot return a unique rotation.")
    E = eye.repeat(N, 1, 1)
    if not allow_reflection:
        E[:, -1, -1] = torch.det(torch.bmm(U, V.transpose(1, 2)))
    R = torch.bmm(torch.bmm(U, E), V.transpose(1, 2))
    if estimate_scale:
        s = (torch.diagonal(E, dim1=1, dim2=2) * S).sum(1) / ((Xc * Xc).sum((1, 2)) / total).clamp(eps)
    else:
        s = total.new_ones(N)
    T = Ymu[:, 0, :] - s[:, None] * torch.bmm(Xmu, R)[:, 0, :]
    nan = float("nan")
    return SimilarityTransform(R.masked_fill(bad[:, None, None], nan), T.masked_fill(bad[:, None], nan),
                               s.masked_fill(bad, nan))


def _align_native(X, Y, weights, lengths, estimate_scale, allow_reflection, eps):
    """pr_align_fwd on float32 device tensors: no host read."""
    from .. import _native as nat
    N, P = X.shape[0], X.shape[1]
    x, y = nat.dense(X, torch.float32), nat.dense(Y, torch.float32)
    w = None if weights is None else nat.dense(weights, torch.float32)
    a = nat.PRAlignArgs()
    a.x, a.y, a.weights, a.x_len = nat.ptr(x), nat.ptr(y), nat.ptr(w), nat.ptr(lengths)
    a.N, a.P, a.estimate_scale, a.allow_reflection, a.eps = N, P, int(bool(estimate_scale)), int(bool(allow_reflection)), float(eps)
    R, T, s = (torch.empty(shape, dtype=torch.float32, device=x.device) for shape in ((N, 3, 3), (N, 3), (N,)))
    nbytes = nat.load().pr_align_workspace(N, P)
    ws = nat.workspace(nbytes, x.device)
    a.R, a.T, a.s, a.workspace, a.workspace_bytes = nat.ptr(R), nat.ptr(T), nat.ptr(s), nat.ptr(ws), nbytes
    nat.call("pr_align_fwd", "pr_align_fwd", x, a)
    return SimilarityTransform(R, T, s)


def corresponding_points_alignment(X, Y, weights=None, estimate_scale=False, allow_reflection=False, eps=1e-9):
    """The similarity transform (R, T, s) that minimises sum_i w_i |s X_i R + T - Y_i|^2 over
    corresponding points (PyTorch3D 0.4.0 corresponding_points_alignment; Umeyama's solution): a
    SimilarityTransform namedtuple of R (N,D,D), T (N,D), s (N,) (ones unless estimate_scale).

    X and Y are (N,P,D) tensors or Pointclouds of equal shapes and lengths; weights (N,P) a tensor or
    a list of (P_i,) tensors; rows past a cloud's length get weight 0.  As in the library, the
    centred clouds are both multiplied by the weights, so the covariance carries w^2.  R has
    determinant +1 unless allow_reflection.  The library's two warnings (a cloud with fewer than D+1
    points, a singular value <= 1e-15) need a host read: they are issued for CPU tensors only.

    Float32 device tensors with D = 3 that do not require grad run on the native kernels (no host
    read); everything else on the torch composition, which is differentiable."""
    Xt, num_points = convert_pointclouds_to_tensor(X)
    Yt, _ = convert_pointclouds_to_tensor(Y)
    nx, ragged = _lengths(X)
    ny, _ = _lengths(Y)
    if Xt.shape != Yt.shape or nx != ny:
        raise ValueError("Point sets X and Y have to have the same number of batches, points and dimensions.")
    if not Xt.is_floating_point() or Xt.dtype != Yt.dtype or Xt.device != Yt.device:
        raise ValueError(f"X and Y must be floating point of one dtype on one device, got {Xt.dtype} on {Xt.device} "
                         f"and {Yt.dtype} on {Yt.device}")
    if weights is not None:
        if isinstance(weights, (list, tuple)):
            if [tuple(w.shape) for w in weights] != [(k,) for k in nx]:
                raise ValueError("weights should have the same first two dimensions as X.")
            pad = Xt.new_zeros(Xt.shape[:2])
            for i, w in enumerate(weights):
                pad[i, :w.shape[0]] = w
            weights = pad
        if not torch.is_tensor(weights) or tuple(weights.shape) != tuple(Xt.shape[:2]):
            raise ValueError("weights should have the same first two dimensions as X.")
        weights = weights.to(device=Xt.device, dtype=Xt.dtype)
    lengths = num_points if ragged else None
    if _native_ok(Xt, Yt) and (weights is None or not (torch.is_grad_enabled() and weights.requires_grad)):
        return _align_native(Xt, Yt, weights, lengths, estimate_scale, allow_reflection, eps)
    if ragged:
        mask = (torch.arange(Xt.shape[1], device=Xt.device)[None] < num_points[:, None]).to(Xt.dtype)
        weights = mask if weights is None else mask * weights
    return _align_torch(Xt, Yt, weights, estimate_scale, allow_reflection, eps, num_points)


def _check_icp_inputs(Xt, Yt, init_transform):
    if Xt.dim() != 3 or Yt.dim() != 3 or Xt.shape[0] != Yt.shape[0] or Xt.shape[2] != Yt.shape[2]:
        raise ValueError("Point sets X and Y have to have the same batch size and data dimension.")
    if not Xt.is_floating_point() or Xt.dtype != Yt.dtype or Xt.device != Yt.device:
        raise ValueError(f"X and Y must be floating point of one dtype on one device, got {Xt.dtype} on {Xt.device} "
                         f"and {Yt.dtype} on {Yt.device}")
    if init_transform is None:
        return None
    N, D = Xt.shape[0], Xt.shape[2]
    try:
        R, T, s = init_transform
        ok = tuple(R.shape) == (N, D, D) and tuple(T.shape) == (N, D) and tuple(s.shape) == (N,)
    except Exception:
        ok = False
    if not ok:
        raise ValueError("The initial transformation init_transform has to be a named tuple SimilarityTransform with "
                         "elements (R, T, s). R are dim x dim orthonormal matrices of shape (minibatch, dim, dim), T is a "
                         "batch of dim-dimensional translations of shape (minibatch, dim) and s is a batch of scalars of "
                         "shape (minibatch,).")
    return SimilarityTransform(*(t.to(device=Xt.device, dtype=Xt.dtype) for t in (R, T, s)))


def _icp_torch(Xp, Yp, lx, ly, init, max_iterations, thr, estimate_scale, allow_reflection, verbose, trace=None):
    """The composition.  lx / ly: (N,) int64 lengths on the device.  `trace`: a list that receives
    every iteration's neighbour indices (N,P1) int64, -1 where a row has none."""
    N, P1 = Xp.shape[0], Xp.shape[1]
    live = torch.arange(P1, device=Xp.device)[None] < lx[:, None]
    mask_X = live.to(Xp.dtype)
    Xt = Xp if init is None else _apply_similarity_transform(Xp, *init)
    rows = torch.arange(N, device=Xp.device)[:, None]
    nan, zero = Xp.new_full((), float("nan")), Xp.new_zeros(())
    t_history, converged, rmse, prev, RTs = [], False, None, None, init
    if RTs is None:
        RTs = SimilarityTransform(torch.eye(Xp.shape[2], dtype=Xp.dtype, device=Xp.device)[None].repeat(N, 1, 1),
                                  Xp.new_zeros((N, Xp.shape[2])), Xp.new_ones(N))
    for it in range(max_iterations):
        idx = _ops._knn_points_torch(Xt.detach(), Yp.detach(), lx, ly, 1)[1][..., 0]
        if trace is not None:
            trace.append(idx)
        # a live row without a neighbour poisons its cloud; padded rows carry weight 0
        nn = torch.where((idx >= 0)[..., None], Yp[rows, idx.clamp(min=0)], torch.where(live[..., None], nan, zero))
        RTs = _align_torch(Xp, nn, mask_X, estimate_scale, allow_reflection, 1e-9, lx)
        Xt = _apply_similarity_transform(Xp, *RTs)
        t_history.append(RTs)
        rmse = wmean(((Xt - nn) ** 2).sum(2)[:, :, None], mask_X).sqrt()[:, 0, 0]
        rel = torch.ones_like(rmse) if prev is None else (prev - rmse) / prev
        if verbose:
            print(f"ICP iteration {it}: mean/max rmse = {rmse.mean().item():1.2e}/{rmse.max().item():1.2e}; "
                  f"mean relative rmse = {rel.mean().item():1.2e}")
        if bool((rel <= thr).all()):
            converged = True
            break
        prev = rmse
    return converged, rmse, Xt, RTs, t_history


class _IcpRun:
    """One native ICP run: the device buffers and the argument struct of pr_icp_run.  enqueue(k)
    launches k iterations and reads nothing on the host."""

    def __init__(self, Xp, Yp, lx, ly, init, max_iterations, thr, estimate_scale, allow_reflection, keep_indices=False):
        from .. import _native as nat
        self.nat = nat
        N, P, Q = Xp.shape[0], Xp.shape[1], Yp.shape[1]
        dev = Xp.device
        self.x, self.y = nat.dense(Xp, torch.float32), nat.dense(Yp, torch.float32)
        self.lx, self.ly = lx, ly
        if init is None:
            state = torch.cat([torch.eye(3, dtype=torch.float32, device=dev).reshape(1, 9).expand(N, 9),
                               torch.zeros((N, 3), dtype=torch.float32, device=dev),
                               torch.ones((N, 1), dtype=torch.float32, device=dev)], dim=1)
        else:
            state = torch.cat([init.R.detach().reshape(N, 9), init.T.detach(), init.s.detach()[:, None]], dim=1)
        self.state = state.to(torch.float32).contiguous()
        new = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)  # noqa: E731
        self.history = new((max_iterations, N, nat.PR_ICP_STATE))
        self.rmse, self.idx, self.xt = new((N,)), new((N, P), torch.int32), new((N, P, 3))
        self.idx_history = new((max_iterations, N, P), torch.int32) if keep_indices else None
        self.flags = torch.zeros((2,), dtype=torch.int32, device=dev)
        nbytes = nat.load().pr_icp_workspace(N, P, Q)
        self.ws = nat.workspace(nbytes, dev)
        a = self.args = nat.PRIcpArgs()
        a.x, a.y, a.x_len, a.y_len = nat.ptr(self.x), nat.ptr(self.y), nat.ptr(lx), nat.ptr(ly)
        a.N, a.P, a.Q, a.max_iterations = N, P, Q, max_iterations
        a.estimate_scale, a.allow_reflection, a.relative_rmse_thr = int(bool(estimate_scale)), int(bool(allow_reflection)), float(thr)
        a.state, a.history, a.rmse, a.idx = (nat.ptr(t) for t in (self.state, self.history, self.rmse, self.idx))
        a.idx_history, a.flags, a.xt = nat.ptr(self.idx_history), nat.ptr(self.flags), nat.ptr(self.xt)
        a.workspace, a.workspace_bytes = nat.ptr(self.ws), nbytes
        self.max_iterations, self.enqueued, self.started = max_iterations, 0, False

    def enqueue(self, k, end=False):
        nat = self.nat
        self.args.phase = (0 if self.started else nat.PR_ICP_BEGIN) | (nat.PR_ICP_END if end else 0)
        nat.call("pr_icp_run", "pr_icp_run", self.x, self.args, int(k))
        self.started = True
        self.enqueued += k


def _icp_native(Xp, Yp, lx, ly, init, max_iterations, thr, estimate_scale, allow_reflection, verbose, keep_indices=False):
    """(converged, rmse, Xt, RTs, t_history, idx_history or None) on the native kernels."""
    run = _IcpRun(Xp, Yp, lx, ly, init, max_iterations, thr, estimate_scale, allow_reflection, keep_indices)
    every = 1 if verbose else max(1, int(os.environ.get("PR_ICP_CHECK_EVERY", "8")))
    while run.enqueued < max_iterations:
        run.enqueue(min(every, max_iterations - run.enqueued))
        if verbose:
            conv, it = run.flags.tolist()
            if it == run.enqueued:  # this iteration was executed
                r = run.rmse.tolist()
                print(f"ICP iteration {it - 1}: mean/max rmse = {sum(r) / len(r):1.2e}/{max(r):1.2e}")
        if run.enqueued < max_iterations and run.flags[0].item():  # the batch's only host read
            break
    run.enqueue(0, end=True)
    conv, iters = run.flags.tolist()
    h = run.history
    t_history = [SimilarityTransform(h[i, :, :9].reshape(-1, 3, 3), h[i, :, 9:12], h[i, :, 12]) for i in range(iters)]
    st = run.state
    RTs = SimilarityTransform(st[:, :9].reshape(-1, 3, 3), st[:, 9:12], st[:, 12])
    return bool(conv), run.rmse, run.xt, RTs, t_history, (run.idx_history[:iters] if keep_indices else None)


def iterative_closest_point(X, Y, init_transform=None, max_iterations=100, relative_rmse_thr=1e-6, estimate_scale=False,
                            allow_reflection=False, verbose=False):
    """Iterative closest point (PyTorch3D 0.4.0 iterative_closest_point): the similarity transform
    that takes X (N,P1,D) onto Y (N,P2,D), tensors or Pointclouds, found by alternating the nearest
    point of Y to every transformed point of X (K = 1, squared distances summed coordinate by
    coordinate, the lowest index on ties, points past a cloud's length and NaN points never chosen)
    with corresponding_points_alignment of the initial X against those neighbours.  Returns an
    ICPSolution namedtuple: converged (a Python bool), rmse (N,) of the last iteration (None with
    max_iterations = 0), Xt the transformed X (padded; a Pointclouds for a Pointclouds X), RTs the
    last SimilarityTransform and t_history, one transform per executed iteration.

    rmse is that of the new transform against the neighbours it was solved from; the loop stops when
    (prev - rmse) / prev <= relative_rmse_thr for every cloud of the batch (never on the first
    iteration unless the threshold is >= 1; 0 / 0 is NaN and never converges).  A live query without
    a neighbour (a NaN point, an empty Y cloud) makes its cloud's R, T, s and rmse NaN.

    Float32 device tensors with D = 3 that do not require grad run on the native kernels: no host
    read inside a batch of PR_ICP_CHECK_EVERY iterations (default 8; verbose reads every
    iteration), bitwise reproducible, and the same result for every batch size.  Everything else
    takes the torch composition.  Arguments are checked (ValueError) before anything is launched."""
    Xp, lx = convert_pointclouds_to_tensor(X)
    Yp, ly = convert_pointclouds_to_tensor(Y)
    init = _check_icp_inputs(Xp, Yp, init_transform)
    if isinstance(max_iterations, bool) or not isinstance(max_iterations, int) or max_iterations < 0:
        raise ValueError(f"max_iterations must be an int >= 0, got {max_iterations!r}")
    if max_iterations == 0:
        Xt = Xp if init is None else _apply_similarity_transform(Xp, *init)
        if init is None:
            D = Xp.shape[2]
            init = SimilarityTransform(torch.eye(D, dtype=Xp.dtype, device=Xp.device)[None].repeat(Xp.shape[0], 1, 1),
                                       Xp.new_zeros((Xp.shape[0], D)), Xp.new_ones(Xp.shape[0]))
        converged, rmse, RTs, t_history = False, None, init, []
    elif _native_ok(Xp, Yp) and (init is None or not (torch.is_grad_enabled() and any(t.requires_grad for t in init))):
        ragged_x, ragged_y = _lengths(X)[1], _lengths(Y)[1]
        converged, rmse, Xt, RTs, t_history, _ = _icp_native(
            Xp, Yp, lx if ragged_x else None, ly if ragged_y else None, init, max_iterations, relative_rmse_thr,
            estimate_scale, allow_reflection, verbose)
    else:
        converged, rmse, Xt, RTs, t_history = _icp_torch(Xp, Yp, lx, ly, init, max_iterations, relative_rmse_thr,
                                                          estimate_scale, allow_reflection, verbose)
    if isinstance(X, Pointclouds):
        Xt = X.update_padded(Xt)
    return ICPSolution(converged, rmse, Xt, RTs, t_history)

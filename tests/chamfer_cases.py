"""Shared by the Chamfer tests (not a test module): seeded clouds with planted exact duplicates,
and the brute-force restatement of PyTorch3D 0.4.0's chamfer_distance as the issue documents it:
a dense (P,Q) matrix of d^2 = sum of squared coordinate differences per cloud, argmin (the first
minimum: the lowest index), explicit per-cloud reductions.  Run in float64 on float32 inputs it is
the reference; run in float32 it measures float32's own gradient error (the 4x rule of
test_gpu_mesh_losses.py)."""
import functools

import torch

# seeds at which every query's best and second-best d^2 differ by >= 1e-6 in float64 (asserted by
# clouds()), found by trying 0, 1, 2, ... on the CPU
SEEDS = {(1, 1, 1): 0, (1, 3, 70): 0, (2, 64, 65): 0, (2, 257, 1025): 1}
# database points y[:, 4] = y[:, 6] = y[:, Q // 2] = y[:, Q - 1] = y[:, 1], and the query x[:, 1] = y[:, 1]:
# with the database cut into three ranges the copies lie in the first, the second (also under the cut
# lengths, which keep 2 Q / 3 points) and the last, so the merge of the ranges sees exact ties
DUP = (1, 4, 6)
MIN_GAP = 1e-6


def planted(shape):
    """The indices of the copies in y (ascending; () for a shape too small to hold them)."""
    _, P, Q = shape
    return DUP + (Q // 2, Q - 1) if P >= 2 and Q // 2 > max(DUP) else ()


def lengths(shape, cut):
    """(x_len, y_len) int64 (N,) or (None, None): cuts inside a block and inside a tile, and a
    cloud of length 1."""
    if not cut:
        return None, None
    N, P, Q = shape
    xl, yl = [max(1, P * 3 // 5), 1], [max(1, Q * 2 // 3), Q]
    if N == 1:
        xl, yl = [max(1, P - 1)], yl[:1]
    return torch.tensor(xl), torch.tensor(yl)


def _gaps(q, db, nq, ndb, skip):
    """best and second-best d^2 of every live query, float64, the columns in `skip` left out."""
    d = ((q[:nq, None].double() - db[None, :ndb].double()) ** 2).sum(-1)
    keep = [j for j in range(ndb) if j not in skip]
    if nq == 0 or len(keep) < 2:
        return None
    two = d[:, keep].topk(2, dim=1, largest=False).values
    return two[:, 1] - two[:, 0]


def make_clouds(shape, seed):
    """x (N,P,3), y (N,Q,3), unit normals of both; float32, uniform in [0,1]^3."""
    N, P, Q = shape
    g = torch.Generator().manual_seed(seed)
    x, y = torch.rand((N, P, 3), generator=g), torch.rand((N, Q, 3), generator=g)
    for j in planted(shape)[1:]:
        y[:, j] = y[:, DUP[0]]
    if planted(shape):
        x[:, 1] = y[:, DUP[0]]
    xn, yn = torch.randn((N, P, 3), generator=g), torch.randn((N, Q, 3), generator=g)
    return x, y, xn, yn


def min_gap(shape, seed):
    """The smallest best-to-second-best gap over both directions and both length settings; the
    later copies of the planted duplicate are left out (they tie by construction)."""
    x, y, _, _ = make_clouds(shape, seed)
    N, P, Q = shape
    copies = planted(shape)[1:]
    worst = float("inf")
    for cut in (False, True):
        xl, yl = lengths(shape, cut)
        for n in range(N):
            nx, ny = (P, Q) if xl is None else (int(xl[n]), int(yl[n]))
            for gap in (_gaps(x[n], y[n], nx, ny, copies), _gaps(y[n], x[n], ny, nx, ())):
                if gap is not None:
                    worst = min(worst, gap.min().item())
    return worst


@functools.lru_cache(maxsize=None)
def clouds(shape):
    assert min_gap(shape, SEEDS[shape]) >= MIN_GAP, (shape, min_gap(shape, SEEDS[shape]))
    return make_clouds(shape, SEEDS[shape])


def ref_nn(x, y, xl, yl, dtype=torch.float64):
    """(dist_x (N,P), dist_y (N,Q), idx_x, idx_y) by brute force; padded points and points facing an
    empty cloud: 0 and -1.  Differentiable in x and y."""
    N, P, Q = x.shape[0], x.shape[1], y.shape[1]
    dx, dy, ix, iy = [], [], [], []
    for n in range(N):
        nx, ny = (P, Q) if xl is None else (int(xl[n]), int(yl[n]))
        d = ((x[n, :nx, None].to(dtype) - y[n, None, :ny].to(dtype)) ** 2).sum(-1)
        for dist, idx, dd, cnt, full in ((dx, ix, d, nx, P), (dy, iy, d.t(), ny, Q)):
            if dd.shape[0] == 0 or dd.shape[1] == 0:
                dist.append(torch.zeros(full, dtype=dtype))
                idx.append(torch.full((full,), -1, dtype=torch.int64))
                continue
            j = dd.argmin(dim=1)  # the first minimum
            v = dd.gather(1, j[:, None])[:, 0]
            dist.append(torch.cat([v, torch.zeros(full - cnt, dtype=dtype)]))
            idx.append(torch.cat([j, torch.full((full - cnt,), -1, dtype=torch.int64)]))
    return torch.stack(dx), torch.stack(dy), torch.stack(ix), torch.stack(iy)


def _reduce(cx, cy, xl, yl, w, batch_reduction, point_reduction):
    per = []
    for n in range(cx.shape[0]):
        nx, ny = (cx.shape[1], cy.shape[1]) if xl is None else (int(xl[n]), int(yl[n]))
        sx, sy = cx[n, :nx].sum(), cy[n, :ny].sum()
        if w is not None:
            sx, sy = sx * w[n].to(cx.dtype), sy * w[n].to(cx.dtype)
        if point_reduction == "mean":
            sx, sy = sx / max(nx, 1), sy / max(ny, 1)
        per.append(sx + sy)
    per = torch.stack(per)
    if batch_reduction == "mean":
        return per.sum() / (w.to(cx.dtype).sum() if w is not None else cx.shape[0])
    return per.sum() if batch_reduction == "sum" else per


def _normal_terms(n, other, idx, dtype):
    out = torch.zeros(idx.shape, dtype=dtype)
    for b in range(idx.shape[0]):
        live = idx[b] >= 0
        p, q = n[b][live].to(dtype), other[b][idx[b][live]].to(dtype)
        cos = (p * q).sum(1) / (p.norm(dim=1).clamp(min=1e-6) * q.norm(dim=1).clamp(min=1e-6))
        out[b, live] = 1.0 - cos.abs()
    return out


def ref_chamfer(x, y, batch_reduction="mean", point_reduction="mean", xl=None, yl=None, xn=None, yn=None, w=None,
                dtype=torch.float64, cot=None):
    """dict(loss, loss_normals, dist_x, dist_y, idx_x, idx_y, grad_x, grad_y): the gradients are those
    of (loss * cot).sum(), cot a (N,) cotangent for batch_reduction None."""
    xr, yr = x.to(dtype).requires_grad_(True), y.to(dtype).requires_grad_(True)
    dx, dy, ix, iy = ref_nn(xr, yr, xl, yl, dtype)
    loss = _reduce(dx, dy, xl, yl, w, batch_reduction, point_reduction)
    ln = None
    if xn is not None:
        ln = _reduce(_normal_terms(xn, yn, ix, dtype), _normal_terms(yn, xn, iy, dtype), xl, yl, w, batch_reduction,
                     point_reduction)
    out = loss if cot is None else loss * cot.to(dtype)
    gx, gy = torch.autograd.grad(out.sum(), (xr, yr))
    return dict(loss=loss.detach(), loss_normals=ln, dist_x=dx.detach(), dist_y=dy.detach(), idx_x=ix, idx_y=iy,
                grad_x=gx, grad_y=gy)

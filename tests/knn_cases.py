"""Shared by the K-nearest-neighbour tests (not a test module): seeded clouds with planted exact
duplicates, and the brute-force restatement of PyTorch3D 0.4.0's knn_points as the project documents
it: per cloud a dense (P1,P2) matrix of d^2 = sum of squared coordinate differences, a stable sort
by (d^2, index), the first K, the padding rules.  Run in float64 on float32 inputs it is the
reference; run in float32 it measures float32's own gradient error (the 4x rule of
test_gpu_mesh_losses.py)."""
import functools

import torch

# (N, P1, P2, D, K): small shapes around the sizes at which a tiled search changes path
SHAPES = [
    (1, 1, 1, 3, 1),
    (2, 5, 3, 3, 5),        # K > P2; the cut lengths leave a database of 1
    (1, 3, 70, 3, 8),
    (2, 64, 65, 3, 4),
    (2, 257, 1025, 3, 16),  # several query blocks and database tiles; copies in the first, middle and last third
    (1, 70, 300, 3, 64),    # the largest K
    (1, 40, 130, 1, 3),
    (2, 33, 70, 5, 8),      # D no multiple of 4
    (1, 3, 70, 32, 8),      # the largest D
]
# seeds at which float32 cannot reorder neighbours except the planted ties (asserted by clouds()),
# found by trying 0, 1, 2, ... on the CPU
SEEDS = {s: 0 for s in SHAPES}
SEEDS[(2, 257, 1025, 3, 16)] = 9
SEEDS[(1, 70, 300, 3, 64)] = 3
# database points y[:, 4] = y[:, 6] = y[:, Q // 2] = y[:, Q - 1] = y[:, 1], and the query x[:, 1] = y[:, 1]
DUP = (1, 4, 6)


def planted(shape):
    """The indices of the copies in y (ascending; () for a shape too small to hold them)."""
    _, P, Q = shape[:3]
    return DUP + (Q // 2, Q - 1) if P >= 2 and Q // 2 > max(DUP) else ()


def lengths(shape, cut):
    """(lengths1, lengths2) int64 (N,) or (None, None): cuts inside a block and inside a tile, and a
    cloud of length 1 (chamfer_cases.lengths)."""
    if not cut:
        return None, None
    N, P, Q = shape[:3]
    xl, yl = [max(1, P * 3 // 5), 1], [max(1, Q * 2 // 3), Q]
    if N == 1:
        xl, yl = [max(1, P - 1)], yl[:1]
    return torch.tensor(xl), torch.tensor(yl)


def make_clouds(shape, seed):
    """x (N,P1,D), y (N,P2,D): float32, uniform in [0,1]^D, x drawn before y."""
    N, P, Q, D, _ = shape
    g = torch.Generator().manual_seed(seed)
    x, y = torch.rand((N, P, D), generator=g), torch.rand((N, Q, D), generator=g)
    for j in planted(shape)[1:]:
        y[:, j] = y[:, DUP[0]]
    if planted(shape):
        x[:, 1] = y[:, DUP[0]]
    return x, y


def bound(shape):
    """The relative gap below which float32 might reorder two d^2: 16 times the worst-case rounding
    of two sums of D squared differences ((D + 2) 2^-24 each)."""
    return 32.0 * (shape[3] + 2) * 2.0 ** -24


def margin(shape, seed):
    """The smallest relative gap between consecutive values among every live query's K + 1 smallest
    float64 d^2, over both length settings, the later copies of the planted point left out (they
    tie by construction), as a multiple of bound(shape)."""
    x, y = make_clouds(shape, seed)
    N, P, Q, D, K = shape
    copies = planted(shape)[1:]
    worst = float("inf")
    for cut in (False, True):
        xl, yl = lengths(shape, cut)
        for n in range(N):
            nx, ny = (P, Q) if xl is None else (int(xl[n]), int(yl[n]))
            keep = [j for j in range(ny) if j not in copies]
            if len(keep) < 2:
                continue
            d = ((x[n, :nx, None].double() - y[n, None, keep].double()) ** 2).sum(-1)
            v = d.sort(dim=1).values[:, :K + 1]
            rel = (v[:, 1:] - v[:, :-1]) / v[:, 1:].clamp(min=1e-300)
            worst = min(worst, rel.min().item())
    return worst / bound(shape)


@functools.lru_cache(maxsize=None)
def clouds(shape):
    m = margin(shape, SEEDS[shape])
    assert m >= 1.0, (shape, SEEDS[shape], m)
    return make_clouds(shape, SEEDS[shape])


def ref_knn(x, y, xl, yl, K, dtype=torch.float64):
    """(dists (N,P1,K), idx (N,P1,K) int64) by brute force: ascending (d^2, index); rows at or past
    lengths1 and slots at or past min(K, lengths2) hold 0 and -1.  Differentiable in x and y."""
    N, P, Q = x.shape[0], x.shape[1], y.shape[1]
    dists, idx = [], []
    for n in range(N):
        nx, ny = (P, Q) if xl is None else (int(xl[n]), int(yl[n]))
        d = ((x[n, :nx, None].to(dtype) - y[n, None, :ny].to(dtype)) ** 2).sum(-1)  # (nx, ny)
        k = min(K, ny)
        order = torch.sort(d.detach(), dim=1, stable=True).indices[:, :k]
        jn = torch.full((P, K), -1, dtype=torch.int64)
        dn = torch.cat([torch.cat([d.gather(1, order), torch.zeros((nx, K - k), dtype=dtype)], dim=1),
                        torch.zeros((P - nx, K), dtype=dtype)], dim=0)
        jn[:nx, :k] = order
        dists.append(dn)
        idx.append(jn)
    return torch.stack(dists), torch.stack(idx)


def cotangent(shape):
    """A fixed random cotangent (N,P1,K) for the distances."""
    N, P, _, _, K = shape
    return torch.randn((N, P, K), generator=torch.Generator().manual_seed(1234))


@functools.lru_cache(maxsize=None)
def reference(shape, cut):
    """dict(dists, idx, grad_p1, grad_p2) of the float64 restatement with the gradients of
    (dists * cotangent).sum(), and err = the float32 restatement's gradient errors (p1, p2) against
    it (max-abs over max-abs); computed once per case and shared."""
    from mesh_loss_cases import rel_err
    x, y = clouds(shape)
    xl, yl = lengths(shape, cut)
    out = {}
    for dtype in (torch.float64, torch.float32):
        xr, yr = x.to(dtype).requires_grad_(True), y.to(dtype).requires_grad_(True)
        d, j = ref_knn(xr, yr, xl, yl, shape[4], dtype)
        g1, g2 = torch.autograd.grad((d * cotangent(shape).to(dtype)).sum(), (xr, yr), allow_unused=True)
        g1 = torch.zeros_like(xr) if g1 is None else g1
        g2 = torch.zeros_like(yr) if g2 is None else g2
        out[dtype] = dict(dists=d.detach(), idx=j, grad_p1=g1, grad_p2=g2)
    r64, r32 = out[torch.float64], out[torch.float32]
    r64["err"] = (rel_err(r32["grad_p1"], r64["grad_p1"]), rel_err(r32["grad_p2"], r64["grad_p2"]))
    return r64

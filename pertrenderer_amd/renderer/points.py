"""Point-cloud renderer (PyTorch3D 0.4.0's rasterize_points, PointsRasterizer, the point
compositors and PointsRenderer) on the native kernels of csrc/pr_points.hip.

Semantics.  The points are NDC x, y with view-space z.  Pixel (row, col) of an (H, W) image has the
mesh rasterizer's centre (xf, yf) = (ndc(W-1-col, W, H), ndc(H-1-row, H, W)).  Point p of cloud n is
a candidate of a pixel of image n when z >= 0 and d2 = (xf - x)^2 + (yf - y)^2 < r^2 (strict; a
comparison with NaN is false), r the scalar radius or the point's entry of a (P,) tensor in packed
order; no gradient goes to the radius.  Each pixel keeps the K candidates smallest in (z, packed
index), ascending: exact z ties go to the lowest index (PyTorch3D leaves them unspecified).
idx (int64 packed indices), zbuf (the chosen z, bit for bit) and dists (d2) are (N,H,W,K); unused
slots hold -1.  bin_size and max_points_per_bin are accepted and never change the fragments.

The compositors skip slots with idx < 0 (they are no stop).  With a_k, f_k the alpha and feature
column of valid slot k:
    alpha_composite    out = sum_k a_k prod_{j<k valid}(1 - a_j) f_k
    norm_weighted_sum  out = sum_k a_k f_k / max(sum_k a_k, 1e-4)
    weighted_sum       out = sum_k a_k f_k
and the gradients are the exact derivatives of these formulas (the alpha chain from prefix and
suffix products: PyTorch3D's quotient by (1 - a_t + eps) is not reproduced).

On a ROCm device with float32 inputs, K <= 64 and int32-sized images everything runs on the native
kernels (no atomics, bitwise reproducible, no host read: capturable in a HIP graph); both backward
passes gather over one point -> (pixel, slot) CSR that is sorted on the device once per fragments
object and shared between the rasterizer's and the compositor's backward.  Otherwise (CPU tensors,
other dtypes, larger K or sizes, PR_NATIVE_POINTS=0) a chunked torch composition of the same
formulas runs: brute force per cloud over pixel-row chunks, a stable sort of the masked z."""
import os
from typing import NamedTuple

import torch

from .. import _native as nat
from .pointclouds import Pointclouds

NATIVE_POINTS = os.environ.get("PR_NATIVE_POINTS", "1") != "0"
MAX_K = nat.PR_POINTS_MAX_K
_PAIRS_PER_CHUNK = 1 << 22  # (pixel, point) pairs per block of the composition's search
_MODES = {"alpha": nat.PR_POINTS_ALPHA, "norm": nat.PR_POINTS_NORM, "weighted": nat.PR_POINTS_WEIGHTED}
_INT32 = 2 ** 31 - 1


class PointFragments(NamedTuple):
    idx: torch.Tensor
    zbuf: torch.Tensor
    dists: torch.Tensor


class PointsRasterizationSettings:
    __slots__ = ["image_size", "radius", "points_per_pixel", "bin_size", "max_points_per_bin"]

    def __init__(self, image_size=256, radius=0.01, points_per_pixel=8, bin_size=None, max_points_per_bin=None):
        self.image_size = image_size
        self.radius = radius
        self.points_per_pixel = points_per_pixel
        self.bin_size = bin_size
        self.max_points_per_bin = max_points_per_bin


def pixel_centres(H, W, dtype=torch.float32, device="cpu"):
    """(xs (W,), ys (H,)): the NDC centre of every pixel column and row, csrc/pr_common.h's ndc()
    operation by operation in `dtype` (+X points left, +Y up).  Every operand is a tensor: torch
    turns a division by a Python scalar into a multiplication by its reciprocal on the device, which
    rounds differently from ndc()'s division."""
    def axis(S1, S2):
        i = torch.arange(S1 - 1, -1, -1, dtype=dtype, device=device)
        two, s1, s2 = (torch.full((), float(v), dtype=dtype, device=device) for v in (2, S1, S2))
        rng = (s1 * two) / s2 if S1 > S2 else two
        off = rng / two
        return -off + (rng * i + off) / s1
    return axis(W, H), axis(H, W)


class _FragmentCSR:
    """point -> its (pixel, slot) entries e = ((n H + row) W + col) K + k of one idx tensor, ascending:
    a stable device sort, built by the first backward that asks and shared with the others.  The
    holder belongs to one version of the tensor: after an in-place edit of idx, _csr_of gives the
    next compositor call a new one."""

    def __init__(self, P, version=0):
        self.P, self.version, self._csr = P, version, None

    def get(self, idx):
        if self._csr is None:
            flat = idx.reshape(-1)
            key = flat.masked_fill((flat < 0) | (flat >= self.P), self.P)
            order = torch.argsort(key, stable=True)
            start = torch.searchsorted(key[order].contiguous(), torch.arange(self.P + 1, dtype=torch.int64, device=idx.device))
            self._csr = (start.contiguous(), order.contiguous())
        return self._csr


def _csr_of(idx, P):
    csr = getattr(idx, "_pr_csr", None)
    if csr is None or csr.P != P or csr.version != idx._version:
        csr = _FragmentCSR(P, idx._version)
        try:
            idx._pr_csr = csr
        except AttributeError:
            pass
    return csr


def _fits(N, H, W, K, P, C=1):
    return (0 < N <= 65535 and 0 < H <= 65535 * 8 and W > 0 and K > 0 and P > 0 and N * H * W * max(K, C) <= _INT32
            and P * max(C, 3) <= _INT32)


# ------------------------------------------------------------------ rasterizer
class _RastFn(torch.autograd.Function):
    """points (P,3) packed -> (idx int64, zbuf, dists) (N,H,W,K): pr_points_rast_fwd / _bwd."""

    @staticmethod
    def forward(ctx, points, cloud_first, cloud_count, radius, radius_scalar, H, W, K, csr):
        nat.require_device(points, cloud_first, cloud_count, radius)
        p = nat.dense(points, torch.float32)
        cf, cc = nat.dense(cloud_first, torch.int64), nat.dense(cloud_count, torch.int64)
        rad = None if radius is None else nat.dense(radius, torch.float32)
        N, P = cf.shape[0], p.shape[0]
        idx = torch.empty((N, H, W, K), dtype=torch.int64, device=p.device)
        zbuf = torch.empty((N, H, W, K), dtype=torch.float32, device=p.device)
        dists = torch.empty_like(zbuf)
        a = nat.PRPointsRastArgs()
        a.points, a.cloud_first, a.cloud_count, a.radius = nat.ptr(p), nat.ptr(cf), nat.ptr(cc), nat.ptr(rad)
        a.radius_scalar, a.N, a.H, a.W, a.K, a.P = float(radius_scalar), N, H, W, K, P
        a.idx, a.zbuf, a.dists = nat.ptr(idx), nat.ptr(zbuf), nat.ptr(dists)
        nat.call("pr_points_rast_fwd", "pr_points_rast_fwd", p, a)
        ctx.save_for_backward(p, idx)
        ctx.csr = csr
        ctx.mark_non_differentiable(idx)
        return idx, zbuf, dists

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, _g_idx, g_zbuf, g_dists):
        p, idx = ctx.saved_tensors
        N, H, W, K = idx.shape
        g_zbuf = torch.zeros(idx.shape, dtype=torch.float32, device=p.device) if g_zbuf is None else nat.dense(g_zbuf, torch.float32)
        g_dists = torch.zeros(idx.shape, dtype=torch.float32, device=p.device) if g_dists is None else nat.dense(g_dists, torch.float32)
        start, entries = ctx.csr.get(idx)
        gp = torch.empty_like(p)
        a = nat.PRPointsRastArgs()
        a.points, a.idx, a.N, a.H, a.W, a.K, a.P = nat.ptr(p), nat.ptr(idx), N, H, W, K, p.shape[0]
        a.point_start, a.point_entries = nat.ptr(start), nat.ptr(entries)
        a.grad_zbuf, a.grad_dists, a.grad_points = nat.ptr(g_zbuf), nat.ptr(g_dists), nat.ptr(gp)
        nat.call("pr_points_rast_bwd", "pr_points_rast_bwd", p, a)
        return gp, None, None, None, None, None, None, None, None


def _rasterize_points_torch(points, ranges, radius, H, W, K):
    """The torch composition on packed points in their dtype; `ranges` are Python (first, count) pairs
    per cloud.  The search runs without autograd per cloud over blocks of pixel rows; the chosen
    points are then evaluated once more with autograd."""
    dev, dt, N = points.device, points.dtype, len(ranges)
    xs, ys = pixel_centres(H, W, dt, dev)
    idx = torch.full((N, H, W, K), -1, dtype=torch.int64, device=dev)
    with torch.no_grad():
        pd = points.detach()
        if torch.is_tensor(radius):
            r = radius.detach().to(device=dev, dtype=dt)
        else:
            r = torch.full((), float(radius), dtype=dt, device=dev)
        r2 = r * r
        for n, (first, count) in enumerate(ranges):
            if count == 0:
                continue
            x, y, z = pd[first:first + count].unbind(1)
            r2n = r2[first:first + count] if r2.dim() else r2
            front = z >= 0
            rows = max(1, _PAIRS_PER_CHUNK // (W * count))
            dx = xs[None, :, None] - x[None, None, :]
            dx2 = dx * dx
            for r0 in range(0, H, rows):
                dy = ys[r0:r0 + rows, None, None] - y[None, None, :]
                d2 = dx2 + dy * dy
                cand = (d2 < r2n) & front
                # ascending z, NaN (no candidate) last; stable: the lowest index among equal z
                order = torch.argsort(torch.where(cand, z, torch.full_like(z, float("nan"))), dim=-1, stable=True)[..., :K]
                sel = torch.where(cand.gather(-1, order), order + first, torch.full_like(order, -1))
                idx[n, r0:r0 + rows, :, :sel.shape[-1]] = sel
    valid = idx >= 0
    g = points[idx.clamp(min=0)] if points.shape[0] else points.new_zeros((N, H, W, K, 3))
    dx, dy = xs.view(1, 1, W, 1) - g[..., 0], ys.view(1, H, 1, 1) - g[..., 1]
    minus = torch.full((), -1.0, dtype=dt, device=dev)
    return idx, torch.where(valid, g[..., 2], minus), torch.where(valid, dx * dx + dy * dy, minus)


def _image_size(image_size):
    if isinstance(image_size, (tuple, list)):
        if len(image_size) != 2:
            raise ValueError("image_size must be an int or (H, W)")
        H, W = int(image_size[0]), int(image_size[1])
    else:
        H = W = int(image_size)
    if H <= 0 or W <= 0:
        raise ValueError(f"image_size must be positive, got {image_size}")
    return H, W


def rasterize_points(pointclouds, image_size=256, radius=0.01, points_per_pixel=8, bin_size=None,
                     max_points_per_bin=None):
    """(idx, zbuf, dists), each (N,H,W,K): see the module docstring.  `radius` is a float or a (P,)
    tensor in packed order."""
    if not isinstance(pointclouds, Pointclouds):
        raise ValueError(f"pointclouds must be a Pointclouds, got {type(pointclouds).__name__}")
    N = len(pointclouds)
    if N == 0:
        raise ValueError("pointclouds is empty")
    H, W = _image_size(image_size)
    K = int(points_per_pixel)
    if K <= 0:
        raise ValueError(f"points_per_pixel must be positive, got {points_per_pixel}")
    points = pointclouds.points_packed()
    if not points.is_floating_point():
        raise ValueError(f"points must be floating point, got {points.dtype}")
    P = points.shape[0]
    if torch.is_tensor(radius):
        if tuple(radius.shape) != (P,):
            raise ValueError(f"a radius tensor must have shape ({P},) (packed order), got {tuple(radius.shape)}")
        if radius.device != points.device:
            raise ValueError(f"radius is on {radius.device}, the points on {points.device}")
    native = NATIVE_POINTS and points.is_cuda and points.dtype == torch.float32 and K <= MAX_K and _fits(N, H, W, K, P)
    if native:
        csr = _FragmentCSR(P)
        tensor_radius = torch.is_tensor(radius)
        idx, zbuf, dists = _RastFn.apply(points, pointclouds.cloud_to_packed_first_idx(), pointclouds.num_points_per_cloud(),
                                         radius if tensor_radius else None, 0.0 if tensor_radius else float(radius),
                                         H, W, K, csr)
        csr.version = idx._version
        idx._pr_csr = csr
        return idx, zbuf, dists
    ranges, off = [], 0
    for n in pointclouds.npoints:
        ranges.append((off, n))
        off += n
    return _rasterize_points_torch(points, ranges, radius, H, W, K)


class PointsRasterizer(torch.nn.Module):
    def __init__(self, cameras=None, raster_settings=None):
        super().__init__()
        self.cameras = cameras
        self.raster_settings = raster_settings if raster_settings is not None else PointsRasterizationSettings()

    def to(self, device):
        if self.cameras is not None:
            self.cameras = self.cameras.to(device)
        return self

    def transform(self, point_clouds, **kwargs):
        cameras = kwargs.get("cameras", self.cameras)
        if cameras is None:
            raise ValueError("Cameras must be specified either at initialization or in the forward pass "
                             "of PointsRasterizer")
        w2v, proj = cameras.get_world_to_view_transform(**kwargs), cameras.get_projection_transform(**kwargs)

        def project(pts_world, w2v, proj):
            pts_view = w2v.transform_points(pts_world)
            pts_ndc = proj.transform_points(pts_view)
            return torch.cat([pts_ndc[..., :2], pts_view[..., 2:3]], dim=-1)  # view-space z

        n = point_clouds.npoints
        if all(c == n[0] for c in n):
            return point_clouds.update_padded(project(point_clouds.points_padded(), w2v, proj))
        # clouds of unequal sizes: cloud by cloud under its own camera.  The zero rows that pad the
        # shorter clouds never reach the cameras (a row on the camera plane would put 0 * inf = NaN
        # into the camera parameters' gradients).
        nth = lambda t, i: type(t)(t.matrix[i:i + 1]) if getattr(t, "matrix", None) is not None and t.matrix.shape[0] > 1 else t  # noqa: E731
        return point_clouds._with_points([project(p[None], nth(w2v, i), nth(proj, i))[0]
                                          for i, p in enumerate(point_clouds.points_list())])

    def forward(self, point_clouds, **kwargs) -> PointFragments:
        rs = kwargs.get("raster_settings", self.raster_settings)
        idx, zbuf, dists = rasterize_points(self.transform(point_clouds, **kwargs), image_size=rs.image_size,
                                            radius=rs.radius, points_per_pixel=rs.points_per_pixel, bin_size=rs.bin_size,
                                            max_points_per_bin=rs.max_points_per_bin)
        return PointFragments(idx=idx, zbuf=zbuf, dists=dists)


# ------------------------------------------------------------------ compositors
class _CompositeFn(torch.autograd.Function):
    """(idx (N,H,W,K) int64, alphas (N,H,W,K), features (P,C)) -> (N,H,W,C): pr_points_composite_fwd / _bwd."""

    @staticmethod
    def forward(ctx, idx, alphas, features, mode, csr):
        nat.require_device(idx, alphas, features)
        i, al, f = nat.dense(idx, torch.int64), nat.dense(alphas, torch.float32), nat.dense(features, torch.float32)
        N, H, W, K = i.shape
        out = torch.empty((N, H, W, f.shape[1]), dtype=torch.float32, device=f.device)
        a = _CompositeFn._args(i, al, f, mode)
        a.out = nat.ptr(out)
        nat.call("pr_points_composite_fwd", "pr_points_composite_fwd", f, a)
        ctx.save_for_backward(i, al, f)
        ctx.mode, ctx.csr = mode, csr  # the fragments' own CSR holder: one sort, shared with the rasterizer's backward
        return out

    @staticmethod
    def _args(i, al, f, mode):
        a = nat.PRPointsCompositeArgs()
        a.idx, a.alphas, a.features = nat.ptr(i), nat.ptr(al), nat.ptr(f)
        a.N, a.H, a.W, a.K = i.shape
        a.C, a.mode, a.P = f.shape[1], mode, f.shape[0]
        return a

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        i, al, f = ctx.saved_tensors
        N, H, W, K = i.shape
        g = nat.dense(g_out, torch.float32)
        start, entries = ctx.csr.get(i)
        ga, gf = torch.empty_like(al), torch.empty_like(f)
        a = _CompositeFn._args(i, al, f, ctx.mode)
        nbytes = nat.load().pr_points_workspace(N, H, W, K)
        ws = nat.workspace(nbytes, f.device)
        a.workspace, a.workspace_bytes = nat.ptr(ws), nbytes
        a.point_start, a.point_entries = nat.ptr(start), nat.ptr(entries)
        a.grad_out, a.grad_alphas, a.grad_features = nat.ptr(g), nat.ptr(ga), nat.ptr(gf)
        nat.call("pr_points_composite_bwd", "pr_points_composite_bwd", f, a)
        return None, ga, gf, None, None


def _composite_torch(idx, alphas, features, mode):
    """The torch composition on the rasterizer's layouts: idx, alphas (N,H,W,K), features (P,C) -> (N,H,W,C)."""
    P, C = features.shape
    valid = (idx >= 0) & (idx < P)
    zero = torch.zeros((), dtype=alphas.dtype, device=alphas.device)
    a = torch.where(valid, alphas, zero)
    if P == 0:
        return alphas.new_zeros(idx.shape[:3] + (C,)) + 0.0 * a.sum()
    f = torch.where(valid[..., None], features[idx.clamp(0, P - 1)], zero.to(features.dtype))
    if mode == nat.PR_POINTS_ALPHA:
        T = torch.cumprod(1.0 - a, dim=-1)
        T = torch.cat([torch.ones_like(T[..., :1]), T[..., :-1]], dim=-1)
        return ((a * T)[..., None] * f).sum(dim=-2)
    out = (a[..., None] * f).sum(dim=-2)
    if mode == nat.PR_POINTS_NORM:
        out = out / torch.clamp(a.sum(dim=-1, keepdim=True), min=1e-4)
    return out


def _composite_rows(idx, alphas, features, mode):
    """Compositor on the rasterizer's layouts, native where it can be: (N,H,W,C)."""
    if idx.dim() != 4 or alphas.shape != idx.shape or features.dim() != 2:
        raise ValueError("the compositors take idx and alphas of one 4-d shape and 2-d features, got "
                         f"{tuple(idx.shape)}, {tuple(alphas.shape)}, {tuple(features.shape)}")
    if idx.dtype != torch.int64:
        idx = idx.long()
    N, H, W, K = idx.shape
    P, C = features.shape
    if (NATIVE_POINTS and alphas.is_cuda and alphas.dtype == torch.float32 and features.dtype == torch.float32
            and C > 0 and _fits(N, H, W, K, P, C)):
        return _CompositeFn.apply(idx, alphas, features, mode, _csr_of(idx, P))
    return _composite_torch(idx, alphas, features, mode)


def _composite_public(pointsidx, alphas, pt_clds, mode):
    if pointsidx.dim() != 4 or pt_clds.dim() != 2:
        raise ValueError("pointsidx and alphas must be (N,K,H,W) and pt_clds (C,P)")
    out = _composite_rows(pointsidx.permute(0, 2, 3, 1), alphas.permute(0, 2, 3, 1), pt_clds.t(), mode)
    return out.permute(0, 3, 1, 2)


def alpha_composite(pointsidx, alphas, pt_clds):
    """(N,C,H,W) from pointsidx, alphas (N,K,H,W) and pt_clds (C,P): front-to-back alpha compositing."""
    return _composite_public(pointsidx, alphas, pt_clds, nat.PR_POINTS_ALPHA)


def norm_weighted_sum(pointsidx, alphas, pt_clds):
    """(N,C,H,W): the alpha-weighted mean of the features, the weight sum clamped at 1e-4."""
    return _composite_public(pointsidx, alphas, pt_clds, nat.PR_POINTS_NORM)


def weighted_sum(pointsidx, alphas, pt_clds):
    """(N,C,H,W): the alpha-weighted sum of the features."""
    return _composite_public(pointsidx, alphas, pt_clds, nat.PR_POINTS_WEIGHTED)


class _Compositor(torch.nn.Module):
    _mode = None

    def __init__(self, background_color=None):
        super().__init__()
        self.background_color = background_color
        self._bg = {}

    def _background(self, bc, C, dtype, device):
        """(C,) tensor of the background colour `bc`.  The module's own colour is cached per device (no
        host copy in a captured step); a colour given for one call is built for that call."""
        own = bc is self.background_color
        key = (C, dtype, str(device))
        bg = self._bg.get(key) if own else None
        if bg is None:
            bc = bc.detach().to("cpu", torch.float64).reshape(-1).tolist() if torch.is_tensor(bc) else [float(v) for v in bc]
            if len(bc) == 3 and C == 4:
                bc = bc + [1.0]  # an alpha channel: opaque
            if len(bc) != C:
                raise ValueError(f"background_color has {len(bc)} channels, the features have {C}")
            bg = torch.tensor(bc, dtype=dtype).to(device)
            if own:
                self._bg[key] = bg
        return bg

    def _rows(self, idx, alphas, features, **kwargs):
        """idx, alphas (N,H,W,K) and features (P,C) rows -> (N,H,W,C): PointsRenderer's path, no permutes.
        Of the keywords only `background_color` is read, for this call (the module keeps its own)."""
        out = _composite_rows(idx, alphas, features, self._mode)
        bc = kwargs.get("background_color", self.background_color)
        if bc is not None:
            out = torch.where((idx[..., 0] < 0)[..., None], self._background(bc, out.shape[-1], out.dtype, out.device), out)
        return out

    def forward(self, fragments, alphas, ptclds, **kwargs):
        """PyTorch3D's layouts: fragments (idx) and alphas (N,K,H,W), ptclds (C,P) -> (N,C,H,W)."""
        return self._rows(fragments.permute(0, 2, 3, 1), alphas.permute(0, 2, 3, 1), ptclds.t(), **kwargs).permute(0, 3, 1, 2)


class AlphaCompositor(_Compositor):
    """Front-to-back alpha compositing; `background_color` fills the pixels whose slot 0 is empty."""
    _mode = nat.PR_POINTS_ALPHA


class NormWeightedCompositor(_Compositor):
    """The alpha-weighted mean of the features; `background_color` fills the pixels whose slot 0 is empty."""
    _mode = nat.PR_POINTS_NORM


class PointsRenderer(torch.nn.Module):
    """rasterizer (PointsRasterizer) + compositor: (N,H,W,C) images of a Pointclouds with features,
    weights = 1 - dists / r^2."""

    def __init__(self, rasterizer, compositor):
        super().__init__()
        self.rasterizer = rasterizer
        self.compositor = compositor

    def to(self, device):
        self.rasterizer = self.rasterizer.to(device)
        return self

    def forward(self, point_clouds, **kwargs):
        features = point_clouds.features_packed()
        if features is None:
            raise ValueError("PointsRenderer needs a Pointclouds with features")
        fragments = self.rasterizer(point_clouds, **kwargs)
        r = kwargs.get("raster_settings", self.rasterizer.raster_settings).radius
        if torch.is_tensor(r):  # per-point radii: the radius of every slot's point
            r = r.detach().to(fragments.dists.dtype)[fragments.idx.clamp(min=0)]
        weights = 1 - fragments.dists / (r * r)
        # fragments and feature rows straight through: no (N,K,H,W) / (C,P) round trip
        return self.compositor._rows(fragments.idx, weights, features, **kwargs)

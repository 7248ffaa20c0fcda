"""Seeded scenes for the point-cloud renderer tests and a float64 restatement of rasterize_points
and the three compositors, written with numpy / dense torch and independent of
pertrenderer_amd/renderer/points.py.

Pixel centres.  The contract takes the mesh rasterizer's pixel centres "exactly": the centre of a
pixel IS the float32 value of ndc() (csrc/pr_common.h).  centres() mirrors ndc() operation by
operation in numpy float32 and widens the result; everything after it (d2, the candidate test, the
selection, the compositors, every gradient) is float64.

Scenes.  Points are float32 values (widened exactly), so z comparisons, and with them the (z, index)
order, are the same in both precisions; scene() additionally asserts
  * |d2 - r^2| >= 1e-6 for every (pixel, point) pair with finite coordinates, and
  * the K-th and (K+1)-th candidate of every pixel differ by >= 1e-6 in z unless they are exactly
    equal (a planted tie, which the lowest-index rule decides in any precision),
so the float32 selection cannot legitimately differ from float64's.  Seeds are searched in a fixed
order until both hold.

Planted in every cloud of >= 30 points: z < 0 (3, 4), outside the image (5, 6), exactly on a pixel
centre (7: d2 = 0, weight exactly 1, so the alpha chain has a factor 1 - a = 0), a duplicated point
(8, 9), two overlapping points of equal z (20, 21), a NaN point (11).

references() also runs the float32 torch composition of renderer/points.py on the CPU and asserts
that it meets the value tolerance (conftest.assert_close defaults) and a gradient error <= 2e-5
against float64: the bars of the GPU tests are ones the formulas alone satisfy in float32."""
import functools

import numpy as np
import torch

from conftest import assert_close

MODES = ("alpha", "norm", "weighted")
PLANT_BEHIND, PLANT_OUTSIDE, PLANT_CENTRE, PLANT_DUP, PLANT_EQUAL_Z, PLANT_NAN = (3, 4), (5, 6), 7, (8, 9), (20, 21), 11
CENTRE_PIXEL = (10, 12)  # (row, col) of the point planted on a pixel centre

# name -> (image (H, W), cloud sizes, K, radius: a float or "per-point", seed)
SCENES = {
    "one_k1": ((32, 32), (1,), 1, 0.1, 1),
    "c70_k8": ((32, 32), (70,), 8, 0.2, 2),
    "c70_k50": ((24, 40), (70,), 50, 0.3, 3),
    "c1000_k8": ((24, 40), (1000,), 8, 0.05, 4),
    "c1000_k50": ((32, 32), (1000,), 50, 0.2, 5),
    "batch2_k8": ((24, 40), (70, 1000), 8, 0.1, 6),
    "empty_k8": ((32, 32), (70, 0, 1), 8, 0.3, 7),
    "per_point_k8": ((24, 40), (70, 30), 8, "per-point", 8),
}
GRAD_KEYS = ("d_points",) + tuple(f"d_{w}_{m}" for m in MODES for w in ("alphas", "features"))


def rel_err(a, b, floor=0.0):
    """max |a - b| / max(max |b|, floor) (b the float64 reference)."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).abs().max() / b.abs().max().clamp(min=max(floor, 1e-30))).item() if b.numel() else 0.0


DEGENERATE = 1e-9  # a reference gradient this far below its own terms has cancelled to rounding


def grad_scale(key, ref):
    """The denominator of grad_error: max |ref[key]|, plainly.  One exception: the norm-weighted
    d alphas is the difference (G_t - q) / D of two terms of the size of G_t = the weighted mode's
    d alphas, and in a scene whose pixels all have one valid slot (one_k1) they cancel exactly
    (out = f whatever a is): float64 leaves about 4e-16, which is no magnitude to divide by.  Only
    there (max |ref| <= 1e-9 max |G_t|) the scale is max |G_t|, the size of the terms float32 rounds."""
    scale = ref[key].abs().max().item()
    if key == "d_alphas_norm":
        terms = ref["d_alphas_weighted"].abs().max().item()
        if scale <= DEGENERATE * terms:
            scale = terms
    return max(scale, 1e-30)


def grad_error(key, got, ref):
    """The gradient error of GRAD_KEYS entry `key` against the float64 reference dict `ref`:
    max-abs over max-abs (grad_scale)."""
    return (got.detach().cpu().double() - ref[key]).abs().max().item() / grad_scale(key, ref)


def _ndc32(i, S1, S2):
    f = np.float32
    rng = f(2.0)
    if S1 > S2:
        rng = (f(S1) * rng) / f(S2)
    off = rng / f(2.0)
    return -off + (rng * i.astype(np.float32) + off) / f(S1)


def centres(H, W):
    """(xs (W,), ys (H,)) float64: the float32 pixel centres, widened (+X left, +Y up)."""
    xs = _ndc32(np.arange(W - 1, -1, -1), W, H)
    ys = _ndc32(np.arange(H - 1, -1, -1), H, W)
    assert xs.dtype == ys.dtype == np.float32
    return xs.astype(np.float64), ys.astype(np.float64)


def _make(name, seed):
    (H, W), sizes, K, radius, _ = SCENES[name]
    g = torch.Generator().manual_seed(seed)
    xs, ys = centres(H, W)
    clouds = []
    for n in sizes:
        p = torch.empty((n, 3))
        p[:, :2] = torch.rand((n, 2), generator=g) * 2.3 - 1.15
        p[:, 2] = torch.rand((n,), generator=g) * 2.5 + 0.5
        if n == 1:
            p[0, 0], p[0, 1] = float(xs[CENTRE_PIXEL[1]]), float(ys[CENTRE_PIXEL[0]])
        if n >= 30:
            p[PLANT_BEHIND[0], 2], p[PLANT_BEHIND[1], 2] = -0.5, -1e-3
            p[PLANT_OUTSIDE[0], 0], p[PLANT_OUTSIDE[1], 1] = 3.0, -2.5
            p[PLANT_CENTRE, 0], p[PLANT_CENTRE, 1] = float(xs[CENTRE_PIXEL[1]]), float(ys[CENTRE_PIXEL[0]])
            p[PLANT_DUP[0], 2] = 0.3
            p[PLANT_DUP[1]] = p[PLANT_DUP[0]]
            p[PLANT_EQUAL_Z[0], 2] = 0.4
            p[PLANT_EQUAL_Z[1], :2] = p[PLANT_EQUAL_Z[0], :2] + 0.03
            p[PLANT_EQUAL_Z[1], 2] = 0.4
            p[PLANT_NAN, 0] = float("nan")
        clouds.append(p)
    P = sum(sizes)
    rad = torch.rand((P,), generator=g) * 0.25 + 0.05 if radius == "per-point" else radius
    feats = [torch.rand((n, 3), generator=g) for n in sizes]
    return clouds, rad, feats


def _radius32(rad, P):
    """(P,) float64 of the float32 radii."""
    if torch.is_tensor(rad):
        return rad.double().numpy()
    return np.full((P,), np.float64(np.float32(rad)))


def rasterize64(clouds, rad, H, W, K, check=False):
    """float64 (idx int64, zbuf, dists), each (N,H,W,K) numpy; with `check` returns instead whether the two scene
    conditions hold."""
    xs, ys = centres(H, W)
    N, P = len(clouds), sum(c.shape[0] for c in clouds)
    r_all = _radius32(rad, P)
    idx = np.full((N, H, W, K), -1, np.int64)
    zbuf, dists = np.full((N, H, W, K), -1.0), np.full((N, H, W, K), -1.0)
    first = 0
    for n, c in enumerate(clouds):
        cn = c.shape[0]
        if cn == 0:
            continue
        p = c.double().numpy()
        r2 = r_all[first:first + cn] ** 2
        with np.errstate(invalid="ignore"):
            d2 = (xs[None, :, None] - p[None, None, :, 0]) ** 2 + (ys[:, None, None] - p[None, None, :, 1]) ** 2
            cand = (p[:, 2] >= 0)[None, None, :] & (d2 < r2)
        if check and not (np.abs(d2 - r2)[np.isfinite(d2)] >= 1e-6).all():
            return False
        zm = np.where(cand, p[None, None, :, 2], np.inf)
        order = np.argsort(zm, axis=-1, kind="stable")  # ascending z, the lowest index among equal z
        if check and cn > K:
            zs = np.take_along_axis(zm, order[..., K - 1:K + 1], -1)
            both = np.isfinite(zs).all(-1)
            gap = zs[both][:, 1] - zs[both][:, 0]
            if not ((gap >= 1e-6) | (gap == 0)).all():
                return False
        order = order[..., :K]
        ok = np.take_along_axis(cand, order, -1)
        k = order.shape[-1]
        idx[n, ..., :k] = np.where(ok, order + first, -1)
        zbuf[n, ..., :k] = np.where(ok, np.take_along_axis(zm, order, -1), -1.0)
        dists[n, ..., :k] = np.where(ok, np.take_along_axis(d2, order, -1), -1.0)
        first += cn
    return True if check else (idx, zbuf, dists)


@functools.lru_cache(maxsize=None)
def scene(name):
    """dict(clouds [float32 (P_i,3)], radius (float or float32 (P,)), features [float32 (P_i,3)], H, W, K)."""
    (H, W), sizes, K, _, seed = SCENES[name]
    for t in range(64):
        clouds, rad, feats = _make(name, seed + 1000 * t)
        if rasterize64(clouds, rad, H, W, K, check=True):
            return dict(clouds=clouds, radius=rad, features=feats, H=H, W=W, K=K)
    raise AssertionError(f"{name}: no seed meets the scene conditions")


def raster_loss64(points, idx, cot_z, cot_d, H, W):
    """(zbuf, dists, loss) in float64 torch at the given indices (autograd reaches `points`)."""
    xs, ys = (torch.from_numpy(v) for v in centres(H, W))
    valid = idx >= 0
    g = points[idx.clamp(min=0)]
    d2 = (xs.view(1, 1, W, 1) - g[..., 0]) ** 2 + (ys.view(1, H, 1, 1) - g[..., 1]) ** 2
    minus = torch.tensor(-1.0, dtype=torch.float64)
    zbuf, dists = torch.where(valid, g[..., 2], minus), torch.where(valid, d2, minus)
    return zbuf, dists, (zbuf * cot_z).sum() + (dists * cot_d).sum()


def composite64(idx, alphas, feats, mode):
    """(N,H,W,C) float64 by a plain loop over the K slots; idx, alphas (N,H,W,K), feats (P,C)."""
    N, H, W, K = idx.shape
    out = torch.zeros((N, H, W, feats.shape[1]), dtype=torch.float64)
    T, total = torch.ones((N, H, W), dtype=torch.float64), torch.zeros((N, H, W), dtype=torch.float64)
    for k in range(K):
        v = idx[..., k] >= 0
        a = torch.where(v, alphas[..., k], torch.zeros((), dtype=torch.float64))
        f = feats[idx[..., k].clamp(min=0)] * v[..., None]
        if mode == "alpha":
            out = out + (a * T)[..., None] * f
            T = T * (1 - a)
        else:
            out = out + a[..., None] * f
            total = total + a
    if mode == "norm":
        out = out / torch.clamp(total, min=1e-4)[..., None]
    return out


def slot_radius2(rad, idx):
    """(N,H,W,K) float64 r^2 of every slot's point (1 for an empty slot)."""
    if torch.is_tensor(rad):
        return torch.where(idx >= 0, rad.double()[idx.clamp(min=0)] ** 2, torch.ones((), dtype=torch.float64))
    return torch.full(idx.shape, float(np.float64(np.float32(rad)) ** 2), dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def references(name):
    """float64 reference of scene `name`, computed once and shared:
    idx, zbuf, dists; the compositor inputs alphas (float32: the renderer's weights 1 - d2 / r^2 of the
    valid slots, 0.5 elsewhere) and cotangents; per mode the image; every gradient of GRAD_KEYS under
    the cotangents; and err32: the float32 composition's own gradient errors (asserted <= 2e-5)."""
    s = scene(name)
    H, W, K = s["H"], s["W"], s["K"]
    idx, zbuf, dists = (torch.from_numpy(v) for v in rasterize64(s["clouds"], s["radius"], H, W, K))
    packed = torch.cat(s["clouds"])
    feats = torch.cat(s["features"])
    g = torch.Generator().manual_seed(SCENES[name][4] + 77)
    cot_z, cot_d = (torch.randn(idx.shape, generator=g, dtype=torch.float64) for _ in range(2))
    cot_img = torch.randn(idx.shape[:3] + (3,), generator=g, dtype=torch.float64)
    alphas = torch.where(idx >= 0, 1.0 - dists / slot_radius2(s["radius"], idx), torch.full((), 0.5, dtype=torch.float64)).float()
    ref = dict(idx=idx, zbuf=zbuf, dists=dists, alphas=alphas, cot_z=cot_z, cot_d=cot_d, cot_img=cot_img)
    p64 = packed.double().requires_grad_(True)
    z2, d2, loss = raster_loss64(p64, idx, cot_z, cot_d, H, W)
    assert torch.equal(z2, zbuf) and torch.equal(d2.detach(), dists)
    (ref["d_points"],) = torch.autograd.grad(loss, p64)
    nan_rows = torch.isnan(packed).any(dim=1)
    assert not ref["d_points"][nan_rows].any()  # a NaN point is never chosen
    for m in MODES:
        a64, f64 = alphas.double().requires_grad_(True), feats.double().requires_grad_(True)
        img = composite64(idx, a64, f64, m)
        ref[f"image_{m}"] = img.detach()
        ref[f"d_alphas_{m}"], ref[f"d_features_{m}"] = torch.autograd.grad((img * cot_img).sum(), (a64, f64))
    ref["err32"] = _composition_errors(s, ref)
    return ref


def _composition_errors(s, ref):
    """The float32 torch composition (renderer/points.py) on the CPU against `ref`: values at the
    tests' tolerance, gradient errors (max-abs over max-abs) <= 2e-5; returns the errors."""
    from pertrenderer_amd.renderer import Pointclouds
    from pertrenderer_amd.renderer import points as PT
    clouds = [c.clone().requires_grad_(True) for c in s["clouds"]]
    idx, zbuf, dists = PT.rasterize_points(Pointclouds(clouds), (s["H"], s["W"]), s["radius"], s["K"])
    assert torch.equal(idx, ref["idx"]) and torch.equal(zbuf.detach().double(), ref["zbuf"])
    assert_close(dists, ref["dists"], name="composition dists")
    gp = torch.autograd.grad((zbuf * ref["cot_z"].float()).sum() + (dists * ref["cot_d"].float()).sum(), clouds, allow_unused=True)
    err = dict(d_points=grad_error("d_points", torch.cat([torch.zeros_like(c) if x is None else x for x, c in zip(gp, clouds)]), ref))
    feats = torch.cat(s["features"])
    for m in MODES:
        a, f = ref["alphas"].clone().requires_grad_(True), feats.clone().requires_grad_(True)
        img = PT._composite_rows(ref["idx"], a, f, PT._MODES[m])
        assert_close(img, ref[f"image_{m}"], name=f"composition image {m}")
        ga, gf = torch.autograd.grad((img * ref["cot_img"].float()).sum(), (a, f))
        err[f"d_alphas_{m}"], err[f"d_features_{m}"] = grad_error(f"d_alphas_{m}", ga, ref), grad_error(f"d_features_{m}", gf, ref)
    assert max(err.values()) <= 2e-5, err
    return err

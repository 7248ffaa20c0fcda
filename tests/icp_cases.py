"""A numpy restatement of corresponding_points_alignment and iterative_closest_point
(renderer/alignment.py's docstrings are the specification) in float64 or float32, and the scenes the
ICP tests share.

The restatement asserts, at every iteration, that each live query's nearest and second-nearest d^2
differ by >= MARGIN relative: a float32 transform (error <= 1e-6 on these scenes, clouds in [-1,1]^3,
neighbour distances ~1e-2) moves a d^2 by ~1e-4 relative, so float32 cannot change an assignment, and
the indices of the float32 and float64 runs are asserted equal.  reference() also asserts that the
float32 run of the restatement stays within 2e-5 (max-abs over max-abs) of the float64 run, which
bounds the 4x rule the GPU tests apply."""
import functools

import numpy as np

MARGIN = 1e-3
REF32_BOUND = 2e-5


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(degrees)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def apply(X, R, T, s):
    """s (X R) + T, batched, in X's dtype."""
    return s[:, None, None] * np.einsum("npj,njk->npk", X, R) + T[:, None, :]


def align(X, Y, w=None, estimate_scale=False, allow_reflection=False, eps=1e-9, lengths=None):
    """(R (N,3,3), T (N,3), s (N,)) in X's dtype.  w (N,P) or None; rows past lengths[n] get weight 0."""
    dt = X.dtype
    N, P, D = X.shape
    R, T, s = np.zeros((N, D, D), dt), np.zeros((N, D), dt), np.zeros((N,), dt)
    for n in range(N):
        L = P if lengths is None else int(lengths[n])
        mask = (np.arange(P) < L).astype(dt)
        ww = None if (w is None and L == P) else (mask if w is None else mask * w[n].astype(dt))
        wv = np.ones(P, dt) if ww is None else ww
        den = max(wv.sum(dtype=dt), dt.type(eps))
        xmu = (X[n] * wv[:, None]).sum(0, dtype=dt) / den
        ymu = (Y[n] * wv[:, None]).sum(0, dtype=dt) / den
        xc, yc = X[n] - xmu, Y[n] - ymu
        if ww is not None:
            xc, yc = xc * ww[:, None], yc * ww[:, None]
            total = max(ww.sum(dtype=dt), dt.type(eps))
        else:
            total = dt.type(max(L, 1))
        C = (xc.T @ yc) / total
        if not np.isfinite(C).all():
            R[n], T[n], s[n] = np.nan, np.nan, np.nan
            continue
        U, S, Vh = np.linalg.svd(C)
        E = np.eye(D, dtype=dt)
        if not allow_reflection:
            E[-1, -1] = np.linalg.det(U @ Vh)
        R[n] = U @ E @ Vh
        s[n] = (np.diag(E) * S).sum() / max((xc * xc).sum(dtype=dt) / total, dt.type(eps)) if estimate_scale else 1
        T[n] = ymu - s[n] * (xmu @ R[n])
    return R, T, s


def nearest(Xt, Y, lx, ly, check_margin):
    """idx (P1,) int64 (-1: none / padding) of one cloud; d^2 summed coordinate by coordinate in
    Xt's dtype, NaN and dead columns at +inf, the lowest index on ties."""
    P1, P2 = Xt.shape[0], Y.shape[0]
    d = np.zeros((P1, P2), Xt.dtype)
    with np.errstate(invalid="ignore"):
        for c in range(Xt.shape[1]):
            diff = Xt[:, None, c] - Y[None, :, c]
            d = d + diff * diff
    d[np.isnan(d)] = np.inf
    d[:, ly:] = np.inf
    idx = d.argmin(1)
    best = d[np.arange(P1), idx]
    idx[~(best < np.inf)] = -1
    idx[lx:] = -1
    margin = np.inf
    if check_margin and P2 >= 2 and lx > 0:
        two = np.partition(d[:lx], 1, axis=1)[:, :2]
        ok = np.isfinite(two[:, 1])
        if ok.any():
            margin = float(((two[ok, 1] - two[ok, 0]) / two[ok, 1]).min())
        assert margin >= MARGIN, f"nearest / second-nearest margin {margin:.2e} < {MARGIN}"
    return idx, margin


def icp(X, Y, lx=None, ly=None, init=None, max_iterations=100, thr=1e-6, estimate_scale=False, allow_reflection=False,
        check_margin=True, rel_gap=None):
    """A dict: converged, rmse (N,), Xt (N,P1,3), R / T / s (iterations, N, ...), idx (iterations, N, P1),
    margin (the smallest seen), rel (iterations, N).  rel_gap: assert every rel after the first
    iteration is >= rel_gap thr or <= thr / rel_gap."""
    dt = X.dtype
    N, P1, _ = X.shape
    lx = [P1] * N if lx is None else list(lx)
    ly = [Y.shape[1]] * N if ly is None else list(ly)
    mask = (np.arange(P1)[None] < np.asarray(lx)[:, None]).astype(dt)
    Xt = X if init is None else apply(X, *(np.asarray(t, dt) for t in init))
    out = dict(R=[], T=[], s=[], idx=[], rel=[], margin=np.inf, converged=False, rmse=None)
    prev = None
    for it in range(max_iterations):
        nn, idx = np.zeros_like(X), np.zeros((N, P1), np.int64)
        for n in range(N):
            idx[n], m = nearest(Xt[n], Y[n], lx[n], ly[n], check_margin)
            out["margin"] = min(out["margin"], m)
            nn[n] = Y[n][np.clip(idx[n], 0, None)]
            nn[n][(idx[n] < 0) & (mask[n] > 0)] = np.nan  # a live query without a neighbour poisons its cloud
            nn[n][mask[n] == 0] = 0
        with np.errstate(invalid="ignore", divide="ignore"):
            R, T, s = align(X, nn, mask, estimate_scale, allow_reflection)
            Xt = apply(X, R, T, s)
            sq = ((Xt - nn) ** 2).sum(2, dtype=dt) * mask
            rmse = np.sqrt(sq.sum(1, dtype=dt) / np.maximum(mask.sum(1, dtype=dt), dt.type(1e-9)))
            rel = np.ones_like(rmse) if prev is None else (prev - rmse) / prev
        for k, v in (("R", R), ("T", T), ("s", s), ("idx", idx), ("rel", rel)):
            out[k].append(v)
        out["rmse"] = rmse
        if rel_gap is not None and it > 0:
            assert ((rel >= rel_gap * thr) | (rel <= thr / rel_gap)).all(), f"rel {rel} too close to {thr} at iteration {it}"
        if (rel <= thr).all():
            out["converged"] = True
            break
        prev = rmse
    for k in ("R", "T", "s", "idx", "rel"):
        out[k] = np.stack(out[k]) if out[k] else np.zeros((0,))
    out["Xt"] = Xt
    return out


def scene(N, P1, P2, seed):
    """X (N,P1,3), Y (N,P2,3) float32 (zero rows past the lengths) and the lengths: Y uniform in
    [-1,1]^3; X a random subset of Y's live rows plus 0.01 N(0,1), minus 0.03, rotated 12 degrees about
    (1,2,3); the clouds after the first cut to max(4, P1 // 2) and P2 - 7."""
    rng = np.random.RandomState(seed)
    Rm = rotation((1, 2, 3), 12.0)
    X, Y = np.zeros((N, P1, 3), np.float32), np.zeros((N, P2, 3), np.float32)
    lx, ly = [], []
    for n in range(N):
        a, b = (P1, P2) if n == 0 else (max(4, P1 // 2), P2 - 7)
        y = rng.uniform(-1, 1, (b, 3))
        x = (y[rng.permutation(b)[:a]] + 0.01 * rng.randn(a, 3) - 0.03) @ Rm
        X[n, :a], Y[n, :b] = x, y
        lx.append(a)
        ly.append(b)
    return X, Y, lx, ly


# name -> (N, P1, P2, seed); the seeds pass the margin assertion through FIXED_ITERATIONS iterations
SHAPES = {"one-65-513": (1, 65, 513, 0), "batch-64-512": (3, 64, 512, 1), "two-257-1025": (2, 257, 1025, 2)}
FIXED_ITERATIONS = 6
EARLY = dict(shape=(2, 65, 513, 2), thr=1e-3, max_iterations=30)


def rel_err(a, b):
    """max-abs over max-abs of a against the reference b."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


QUANTITIES = ("R", "T", "s", "rmse", "Xt")


@functools.lru_cache(maxsize=None)
def reference(name, estimate_scale=False):
    """(scene, float64 run, {quantity: error of the float32 run}) of the fixed-count case `name`."""
    X, Y, lx, ly = scene(*SHAPES[name])
    kw = dict(lx=lx, ly=ly, max_iterations=FIXED_ITERATIONS, thr=-1.0, estimate_scale=estimate_scale)
    r64 = icp(X.astype(np.float64), Y.astype(np.float64), **kw)
    r32 = icp(X, Y, **kw)
    assert np.array_equal(r64["idx"], r32["idx"]), "float32 and float64 disagree on a neighbour"
    err = {q: rel_err(r32[q], r64[q]) for q in QUANTITIES}
    assert max(err.values()) <= REF32_BOUND, err
    return (X, Y, lx, ly), r64, err


@functools.lru_cache(maxsize=None)
def early_reference():
    X, Y, lx, ly = scene(*EARLY["shape"])
    r64 = icp(X.astype(np.float64), Y.astype(np.float64), lx=lx, ly=ly, max_iterations=EARLY["max_iterations"],
              thr=EARLY["thr"], rel_gap=10.0)
    return (X, Y, lx, ly), r64


def rigid_copy(P=40, seed=5, scale=1.0, mirror=False):
    """X (2,P,3) float32 and Y = scale (X R) + T (mirrored through the x = 0 plane first when asked),
    formed in float64 and rounded: (X, Y, R, T)."""
    rng = np.random.RandomState(seed)
    X = rng.uniform(-1, 1, (2, P, 3)).astype(np.float32)
    R = np.stack([rotation((1, 2, 3), 12.0), rotation((-2, 1, 0.5), 75.0)])
    if mirror:
        R = np.diag([-1.0, 1.0, 1.0])[None] @ R
    T = rng.uniform(-1, 1, (2, 3))
    Y = apply(X.astype(np.float64), R, T, np.full(2, float(scale))).astype(np.float32)
    return X, Y, R, T

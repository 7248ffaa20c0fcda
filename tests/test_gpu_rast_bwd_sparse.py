"""pr_rast_bwd on sparse upstream gradients and on every tile shape of its kernel, against the C oracle
(oracle.rast_ref.rast_bwd) at the bar of tests/test_gpu_rast.py's backward tests (conftest.assert_close,
1e-5 relative) and, under torch's deterministic switch (PR_DETERMINISTIC), bit for bit.

The tile kernel sorts each round's valid slots into those whose d dists is not +-0 (they run the
distance term) and the others (they skip it: the term would add +-0), so the patterns below put the
split at chosen lanes of a round, and the frames cover one round, several rounds (a full 8x2 tile at
K = 50 has 800 valid slots), more faces per tile than the LDS reduction holds (128: global atomics),
partial tiles, and a frame whose only non-empty tile is the last.  A face with a non-finite vertex
never skips; its gradient is compared with the one recorded from the commit before the split
(tests/golden/rast_bwd_nonfinite.npz), not with the oracle, which may differ on NaN."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_close
from oracle import rast_ref

pytestmark = pytest.mark.gpu

BLUR = 2e-2


def _soup(F, seed, spread, size, zmin=0.5):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-spread, spread, (F, 1, 2))
    xy = c + rng.uniform(-size, size, (F, 3, 2))
    z = rng.uniform(zmin, 5.0, (F, 3, 1))
    return np.concatenate([xy, z], -1).astype(np.float32)


def _cover(F, seed):
    """F faces that each cover the whole image, at depths that cross: every pixel holds min(F, K) slots."""
    rng = np.random.default_rng(seed)
    tri = np.array([[-4.0, -3.0], [4.0, -3.0], [0.0, 5.0]])
    xy = tri[None] + rng.uniform(-0.5, 0.5, (F, 3, 2))
    z = rng.uniform(0.5, 5.0, (F, 3, 1))
    return np.concatenate([xy, z], -1).astype(np.float32)


# name -> (face_verts, faces per mesh, H, W, K, perspective_correct, clip)
FRAMES = {
    "16x16_k1": lambda: (_soup(60, 21, 0.9, 0.5), [60], 16, 16, 1, False, True),
    "16x16_k7_n2": lambda: (np.concatenate([_soup(70, 22, 0.9, 0.4), _soup(40, 23, 0.9, 0.4)]), [70, 40], 16, 16, 7,
                            True, True),
    "24x20_k50": lambda: (_soup(300, 24, 0.9, 0.6), [300], 24, 20, 50, False, True),
    "24x20_k64_n2": lambda: (np.concatenate([_soup(200, 25, 0.9, 0.6), _soup(150, 26, 0.9, 0.6)]), [200, 150], 24, 20,
                             64, False, False),
    "24x20_k7_n2": lambda: (np.concatenate([_soup(90, 27, 0.9, 0.4), _soup(50, 28, 0.9, 0.4)]), [90, 50], 24, 20, 7,
                            False, True),
    # every 8x2 tile: 16 pixels x 50 slots = 800 valid slots (four rounds of 256)
    "full_800": lambda: (_cover(60, 29), [60], 16, 16, 50, False, True),
    # more than 128 distinct faces in one 8x2 tile
    "many_faces": lambda: (_soup(1500, 30, 1.0, 0.12), [1500], 16, 16, 64, False, True),
    # one small face under the last tile (row H - 1 and column W - 1 are the most negative NDC)
    "last_tile": lambda: (np.array([[[-0.95, -0.99, 1.0], [-0.75, -0.99, 2.0], [-0.85, -0.93, 1.5]]], np.float32), [1],
                          16, 16, 7, False, True),
}

_cache = {}


def _frame(name, device):
    """The frame's forward on the device (once per session): leaf, outputs, host pix_to_face."""
    if name not in _cache:
        from pertrenderer_amd.renderer.rasterizer import _rasterize
        fv, nf, H, W, K, persp, clip = FRAMES[name]()
        first = np.concatenate([[0], np.cumsum(nf)[:-1]]).astype(np.int64)
        fvt = torch.tensor(fv, device=device, requires_grad=True)
        p2f, zbuf, bary, dists = _rasterize(fvt, torch.tensor(first, device=device),
                                            torch.tensor(np.asarray(nf, np.int64), device=device), H, W, K, BLUR, persp,
                                            clip, False)
        _cache[name] = (fv, fvt, (zbuf, bary, dists), p2f.cpu().numpy(), persp, clip)
    return _cache[name]


def _backward(fvt, outs, gz, gb, gd, device, det=False):
    """d face_verts through the autograd wrapper over pr_rast_bwd; a None upstream is passed as absent."""
    pairs = [(o, torch.tensor(g, device=device)) for o, g in zip(outs, (gz, gb, gd)) if g is not None]
    old = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(det)
    try:
        (g,) = torch.autograd.grad([o for o, _ in pairs], fvt, [g for _, g in pairs], retain_graph=True)
    finally:
        torch.use_deterministic_algorithms(old)
    return g.cpu().numpy()


def _check(name, gz, gb, gd, device, det):
    fv, fvt, outs, p2f, persp, clip = _frame(name, device)
    got = _backward(fvt, outs, gz, gb, gd, device, det)
    assert np.isfinite(got).all(), "non-finite gradient"
    ref = rast_ref.rast_bwd(fv, p2f, gz, gb, gd, persp, clip)
    if det:
        np.testing.assert_array_equal(got, ref)
    else:
        assert_close(got, ref, name=f"grad_face_verts[{name}]")
    return got


def _tile_mask(shape, rows=slice(0, 2), cols=slice(0, 8)):
    m = np.zeros(shape, bool)
    m[:, rows, cols] = True
    return m


def _upstream(pattern, p2f):
    """(d zbuf, d bary, d dists) of a pattern; shapes (N,H,W,K), (N,H,W,K,3), (N,H,W,K)."""
    rng = np.random.default_rng(31)
    s = p2f.shape
    gz = rng.standard_normal(s).astype(np.float32)
    gb = rng.standard_normal(s + (3,)).astype(np.float32)
    gd = rng.standard_normal(s).astype(np.float32)
    zero = lambda a: np.zeros_like(a)
    if pattern == "zero":
        return zero(gz), zero(gb), zero(gd)
    if pattern == "only_zbuf":
        return gz, zero(gb), zero(gd)
    if pattern == "only_dists":
        return zero(gz), zero(gb), gd
    if pattern == "only_bary":
        return zero(gz), gb, zero(gd)
    if pattern == "absent_dists":  # no d dists tensor at all
        return gz, gb, None
    if pattern in ("rand70", "negzero"):
        gd[rng.random(s) < 0.7] = 0.0
        gz[rng.random(s) < 0.1] = 0.0
        gb[rng.random(s) < 0.8] = 0.0
        if pattern == "negzero":
            for a in (gz, gb, gd):
                a[a == 0.0] = -0.0
            assert np.signbit(gd[gd == 0.0]).all()
        return gz, gb, gd
    if pattern == "tile_all_zero":  # every d dists of the first 8x2 tile is zero, the others are random
        gd[_tile_mask(s)] = 0.0
        return gz, gb, gd
    if pattern == "tile_none_zero":  # no d dists is zero anywhere
        gd[gd == 0.0] = 1.0
        return gz, gb, gd
    raise KeyError(pattern)


@pytest.mark.parametrize("det", [False, True], ids=["fast", "deterministic"])
@pytest.mark.parametrize("name", list(FRAMES))
def test_frames_random_sparse_upstream(name, det, device):
    """Every frame with d dists 70 % zeros (d zbuf 10 %, d bary 80 %)."""
    fv, fvt, outs, p2f, persp, clip = _frame(name, device)
    valid = p2f >= 0
    if name == "full_800":
        assert (valid[0, :2, :8].sum(), valid.all()) == (800, True)
    if name == "many_faces":
        per_tile = max(len(np.unique(p2f[0, r:r + 2, c:c + 8][valid[0, r:r + 2, c:c + 8]]))
                       for r in range(0, 16, 2) for c in (0, 8))
        assert per_tile > 128, per_tile
    if name == "last_tile":
        assert valid[0, 14:, 8:].any() and valid.sum() == valid[0, 14:, 8:].sum()
    if name.startswith("24x20"):
        assert valid[:, :, 16:].any() and valid[:, 22:, :].any()  # the partial column tile, the last rows
    _check(name, *_upstream("rand70", p2f), device, det)


@pytest.mark.parametrize("det", [False, True], ids=["fast", "deterministic"])
@pytest.mark.parametrize("pattern", ["zero", "only_zbuf", "only_dists", "only_bary", "absent_dists", "negzero",
                                     "tile_all_zero", "tile_none_zero"])
@pytest.mark.parametrize("name", ["full_800", "24x20_k7_n2"])
def test_upstream_patterns(name, pattern, det, device):
    p2f = _frame(name, device)[3]
    got = _check(name, *_upstream(pattern, p2f), device, det)
    if pattern == "zero":
        np.testing.assert_array_equal(got, np.zeros_like(got))


@pytest.mark.parametrize("det", [False, True], ids=["fast", "deterministic"])
@pytest.mark.parametrize("m,rows", [(0, None), (1, None), (63, None), (64, None), (100, None), (255, None),
                                    (256, None), (63, "1"), (100, "4"), (63, "8")])
def test_split_position_in_a_round(m, rows, det, device, monkeypatch):
    """A full frame (every tile's walk is pixel-major, 50 slots per pixel): d dists is non-zero at the
    walk entries i of each 8x2 tile with i % 256 < m, so each 256-slot round has m entries with a
    distance term: the split falls at lane 0 of a wave (m = 0, 64, 256), at lane 63 (m = 63, 255, whose
    last front lane is 62), and inside a wave (m = 1, 100).  Other tile heights (PR_RAST_BWD_ROWS)
    walk the pixels in another order, which moves the split without changing the result."""
    if rows is not None:
        monkeypatch.setenv("PR_RAST_BWD_ROWS", rows)
    p2f = _frame("full_800", device)[3]
    gz, gb, gd = _upstream("tile_none_zero", p2f)
    N, H, W, K = p2f.shape
    r, c, k = np.meshgrid(np.arange(H), np.arange(W), np.arange(K), indexing="ij")
    walk = ((r % 2) * 8 + c % 8) * K + k  # entry of slot (r, c, k) in its 8x2 tile's walk
    gd[0][walk % 256 >= m] = 0.0
    _check("full_800", gz, gb, gd, device, det)


def nonfinite_case(device, det):
    """One face of the 16x16 K = 7 frame gets an infinite x after the forward (so it keeps its slots);
    d dists is zero everywhere, d zbuf and d bary are random.  -> (face index, d face_verts)."""
    from pertrenderer_amd.renderer.rasterizer import _rasterize
    fv = _soup(70, 22, 0.9, 0.4)
    fvt = torch.tensor(fv, device=device, requires_grad=True)
    p2f, zbuf, bary, dists = _rasterize(fvt, torch.tensor([0], device=device), torch.tensor([70], device=device), 16, 16,
                                        7, BLUR, False, True, False)
    pc = p2f.cpu().numpy()
    face = int(np.bincount(pc[pc >= 0]).argmax())  # the face with the most slots
    fvt.data[face, 1, 0] = float("inf")  # .data: the saved tensor's version stays
    rng = np.random.default_rng(32)
    gz = rng.standard_normal(pc.shape).astype(np.float32)
    gb = rng.standard_normal(pc.shape + (3,)).astype(np.float32)
    gd = np.zeros(pc.shape, np.float32)
    return face, _backward(fvt, (zbuf, bary, dists), gz, gb, gd, device, det)


@pytest.mark.parametrize("det", [False, True], ids=["fast", "deterministic"])
def test_nonfinite_vertex_matches_recorded_parent(det, device):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "rast_bwd_nonfinite.npz"))
    face, got = nonfinite_case(device, det)
    exp = gold["deterministic" if det else "fast"]
    assert face == int(gold["face"])
    assert not np.isfinite(exp[face]).all()  # the face's own gradient is where the non-finite values land
    np.testing.assert_array_equal(np.isnan(got), np.isnan(exp))
    fin = np.isfinite(exp)
    np.testing.assert_array_equal(got[~fin & ~np.isnan(exp)], exp[~fin & ~np.isnan(exp)])  # infinities, by sign
    others = np.arange(len(exp)) != face
    assert np.isfinite(got[others]).all()
    if det:
        np.testing.assert_array_equal(got[fin], exp[fin])
    else:
        assert_close(np.where(fin, got, 0.0), np.where(fin, exp, 0.0), name="grad_face_verts")

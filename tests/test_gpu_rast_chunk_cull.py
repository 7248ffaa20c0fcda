"""The rasterizer forward's two-level tile cull (pr_rast.hip: one union box per chunk of
consecutive packed faces, tested before the chunk's face boxes are loaded) lists exactly the
faces of the flat scan of every face box.  Each case compares the fragments (pix_to_face, zbuf,
bary, dists and the valid counts) of the default path bit for bit with the same call under
PR_RAST_CHUNK_CULL=0 (the flat scan) and with the C oracle (oracle/rast_oracle.c), with and
without perspective correction and with clip_barycentric_coords on and off.

A face box gets a NaN bound only when all three corners' x (or y) are NaN: the box is built with
fminf / fmaxf, which drop a single NaN.  What the oracle does with such a face, checked on the CPU:
  * if the face lies off screen along the other axis it is never listed, and the fragments are
    those of the mesh without it (no NaN anywhere): compared with the oracle in every mode;
  * if it lies on screen along the other axis the oracle lists it (160 fragments in the case
    below: like PyTorch3D it skips a face on `dist >= blur`, false for a NaN distance).  The
    rasterizer does not: its per-pixel test keeps a face on `dist < blur`, so a NaN-distance face
    yields no fragment -- measured: 0 fragments of that face in all four modes, two-level and flat,
    and the same 0 with the build before this change.  That difference lies in the per-pixel
    test, which this cull does not touch, so this input is compared with the flat scan only.
So on the GPU a face with a NaN box never yields a fragment, and whether its chunk was kept cannot
be read from the fragments: test_chunk_boxes_in_the_workspace reads the chunk boxes themselves
(all-covering for a chunk with a NaN box, where fminf / fmaxf alone would leave the finite
off-screen union; empty for a chunk of culled faces; the exact union of the members' fp16 boxes
otherwise)."""
import functools

import numpy as np
import pytest
import torch

from oracle import rast_ref

pytestmark = pytest.mark.gpu

BLUR = float(np.log(1.0 / 1e-4 - 1.0) * 1e-3)  # the headline configuration's blur radius
MODES = [(False, False), (False, True), (True, False), (True, True)]  # (perspective_correct, clip)


def _tris(F, seed, spread=0.9, size=0.15, centre=(0.0, 0.0)):
    """F random small triangles in front of the camera around `centre` (NDC)."""
    rng = np.random.default_rng(seed)
    c = np.asarray(centre) + rng.uniform(-spread, spread, (F, 1, 2))
    xy = c + rng.uniform(-size, size, (F, 3, 2))
    z = rng.uniform(0.5, 5.0, (F, 3, 1))
    return np.concatenate([xy, z], -1).astype(np.float32)


def _native(fv, first, nf, H, W, K, persp, clip, device):
    from pertrenderer_amd.renderer.rasterizer import _rasterize, valid_counts
    p2f, zbuf, bary, dists = _rasterize(torch.tensor(fv, device=device), torch.tensor(first, device=device),
                                        torch.tensor(nf, device=device), H, W, K, BLUR, persp, clip, False)
    return tuple(t.detach().cpu().numpy() for t in (p2f, zbuf, bary, dists, valid_counts(p2f)))


def _bits(x):
    return x.view(np.int32) if x.dtype == np.float32 else x


def _both(fv, first, nf, H, W, K, persp, clip, device, monkeypatch):
    """Fragments of the two-level cull, after checking them bit for bit against the flat scan's."""
    monkeypatch.delenv("PR_RAST_CHUNK_CULL", raising=False)
    got = _native(fv, first, nf, H, W, K, persp, clip, device)
    monkeypatch.setenv("PR_RAST_CHUNK_CULL", "0")
    flat = _native(fv, first, nf, H, W, K, persp, clip, device)
    monkeypatch.delenv("PR_RAST_CHUNK_CULL")
    for name, a, b in zip(("pix_to_face", "zbuf", "bary", "dists", "pix_count"), got, flat):
        np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=f"{name}: two-level cull vs flat scan")
    return got


def _check_oracle(got, fv, first, nf, H, W, K, persp, clip):
    rp, rz, rb, rd = rast_ref.rast_fwd(fv, first, nf, H, W, K, BLUR, persp, clip, False)
    p2f, zbuf, bary, dists, cnt = got
    np.testing.assert_array_equal(p2f, rp)
    np.testing.assert_array_equal(cnt, (rp >= 0).sum(-1))
    np.testing.assert_array_equal(zbuf, rz)
    np.testing.assert_array_equal(dists, rd)
    np.testing.assert_array_equal(bary, rb)
    return rp


@functools.lru_cache(maxsize=None)
def _mesh129():
    """Faces ordered left to right, so that a chunk of consecutive faces covers a strip of the image."""
    fv = _tris(129, 21)
    return fv[np.argsort(fv[:, :, 0].mean(1), kind="stable")]


@pytest.mark.parametrize("F", [1, 63, 64, 65, 129])
def test_chunk_edges(F, device, monkeypatch):
    """Face counts around the 64-face chunk size: the last chunk's lanes past the mesh are masked."""
    fv = _mesh129()[:F]
    first, nf = np.array([0]), np.array([F])
    seen = 0
    for persp, clip in MODES:
        got = _both(fv, first, nf, 32, 32, 8, persp, clip, device, monkeypatch)
        seen += (_check_oracle(got, fv, first, nf, 32, 32, 8, persp, clip) >= 0).sum()
    assert seen > 0


@pytest.mark.parametrize("sizes", [(70, 5), (5, 70)])
def test_chunk_straddles_mesh_boundary(sizes, device, monkeypatch):
    """Two meshes in one batch: the chunk that holds faces of both is tested by both images' tiles,
    and each lists only its own mesh's faces."""
    a, b = sizes
    fv = np.concatenate([_tris(a, 31), _tris(b, 32, spread=0.5)])
    first, nf = np.array([0, a]), np.array([a, b])
    for persp, clip in MODES:
        got = _both(fv, first, nf, 32, 32, 8, persp, clip, device, monkeypatch)
        rp = _check_oracle(got, fv, first, nf, 32, 32, 8, persp, clip)
        for n, (lo, hi) in enumerate(((0, a), (a, a + b))):
            hit = rp[n][rp[n] >= 0]
            assert hit.size > 0 and hit.min() >= lo and hit.max() < hi


def _empty_then_visible():
    """Chunk 0: faces behind the camera or of zero area (every box empty); chunk 1: visible faces;
    chunk 2: faces far off screen."""
    dead = _tris(64, 41)
    dead[:32, :, 2] -= 8.0                # behind the camera
    dead[32:, 2, :2] = dead[32:, 1, :2]   # two equal corners: zero area
    return np.concatenate([dead, _tris(64, 42), _tris(64, 43, spread=0.3, centre=(6.0, 5.0))])


def test_empty_chunk_next_to_visible_chunk(device, monkeypatch):
    fv = _empty_then_visible()
    first, nf = np.array([0]), np.array([len(fv)])
    for persp, clip in MODES:
        got = _both(fv, first, nf, 32, 32, 8, persp, clip, device, monkeypatch)
        rp = _check_oracle(got, fv, first, nf, 32, 32, 8, persp, clip)
        hit = rp[rp >= 0]
        assert hit.size > 100 and hit.min() >= 64 and hit.max() < 128


def _nan_box_mesh(face, axis):
    """_empty_then_visible with one face whose box has NaN bounds: all three corners' x or y NaN."""
    fv = _empty_then_visible()
    fv[face, :, axis] = np.nan
    return fv


@pytest.mark.parametrize("face,axis", [(150, 0), (150, 1), (128, 0)])
def test_nan_box_face(face, axis, device, monkeypatch):
    """A box with a NaN bound passes the flat scan's tile test (every comparison is false), so the
    chunk that holds one is never rejected.  Face 150 sits inside the off-screen chunk, 128 is that
    chunk's first face (its slot holds the chunk box; the cull takes its record's box).  Off screen
    along the other axis, the face is never listed: same bits as the flat scan and as the oracle."""
    fv = _nan_box_mesh(face, axis)
    first, nf = np.array([0]), np.array([len(fv)])
    for persp, clip in MODES:
        got = _both(fv, first, nf, 32, 32, 8, persp, clip, device, monkeypatch)
        rp = _check_oracle(got, fv, first, nf, 32, 32, 8, persp, clip)
        assert (rp >= 0).sum() > 100 and not (rp == face).any()


@pytest.mark.parametrize("face", [150, 128])
def test_nan_box_face_on_screen_along_the_other_axis(face, device, monkeypatch):
    """The same face with every y NaN and the x of a visible face, the rest of its chunk off
    screen.  Flat scan only: the oracle lists this face and the rasterizer's per-pixel test never
    does, before this cull as after it (module docstring)."""
    fv = _empty_then_visible()
    fv[face, :, 0] = fv[70, :, 0]
    fv[face, :, 1] = np.nan
    first, nf = np.array([0]), np.array([len(fv)])
    for persp, clip in MODES:
        got = _both(fv, first, nf, 32, 32, 8, persp, clip, device, monkeypatch)
        assert (got[0] >= 0).sum() > 100


def _half_down(x):
    h = x.astype(np.float16)
    return np.where(h.astype(np.float32) > x, np.nextafter(h, np.float16(-np.inf)), h)


def _half_up(x):
    h = x.astype(np.float16)
    return np.where(h.astype(np.float32) < x, np.nextafter(h, np.float16(np.inf)), h)


def _fp16_boxes(fv):
    """(F, 4) float16 [xmin, xmax, ymin, ymax]: the blur-grown boxes rounded outward, valid faces only."""
    r = np.sqrt(np.float32(BLUR))
    x, y = fv[:, :, 0], fv[:, :, 1]
    return np.stack([_half_down(x.min(1) - r), _half_up(x.max(1) + r), _half_down(y.min(1) - r), _half_up(y.max(1) + r)], 1)


@pytest.mark.parametrize("nan_face", [150, 128])
def test_chunk_boxes_in_the_workspace(nan_face, device):
    """The chunk boxes the face pass leaves in the workspace (the box array behind the F 96-byte
    records; a chunk's box in its first face's slot, every other slot the face's own fp16 box):
    chunk 0 (culled faces only) empty, chunk 1 the exact union of its 64 faces' fp16 boxes, chunk 2
    (one face with a NaN box among off-screen faces) all-covering -- fminf / fmaxf alone would have
    dropped the NaN and left the finite off-screen union, which every tile rejects."""
    from pertrenderer_amd import _native as nat
    fv = _nan_box_mesh(nan_face, 0)
    F = len(fv)
    lib = nat.load()
    fvt = torch.tensor(fv, device=device)
    first, nf = torch.tensor([0], device=device), torch.tensor([F], device=device)
    H = W = 32
    K = 8
    a = nat.PRRastArgs()
    a.face_verts, a.mesh_first_face, a.mesh_num_faces = nat.ptr(fvt), nat.ptr(first), nat.ptr(nf)
    a.F, a.N, a.H, a.W, a.K = F, 1, H, W, K
    a.blur_radius, a.perspective_correct, a.clip_barycentric_coords, a.cull_backfaces = BLUR, 0, 1, 0
    p2f = torch.empty((1, H, W, K), dtype=torch.int64, device=device)
    zbuf, dists = (torch.empty((1, H, W, K), dtype=torch.float32, device=device) for _ in range(2))
    bary = torch.empty((1, H, W, K, 3), dtype=torch.float32, device=device)
    a.pix_to_face, a.zbuf, a.bary, a.dists = nat.ptr(p2f), nat.ptr(zbuf), nat.ptr(bary), nat.ptr(dists)
    ws = torch.zeros(lib.pr_rast_fwd_workspace_size(a), dtype=torch.uint8, device=device)
    assert ws.numel() == F * (96 + 8)
    a.workspace, a.workspace_bytes = nat.ptr(ws), ws.numel()
    nat.call("pr_rast_fwd", "pr_rast_fwd", fvt, a)
    torch.cuda.synchronize()
    box = ws.cpu().numpy()[F * 96:].view(np.float16).reshape(F, 4)  # [xmin, xmax, ymin, ymax]
    inf = np.float16(np.inf)
    want = _fp16_boxes(fv)
    np.testing.assert_array_equal(box[0], [inf, -inf, inf, -inf])       # chunk 0: nothing but culled faces
    np.testing.assert_array_equal(box[1:64], np.tile([inf, -inf, inf, -inf], (63, 1)).astype(np.float16))
    np.testing.assert_array_equal(box[65:128], want[65:128])            # faces' own boxes
    m = want[64:128]
    np.testing.assert_array_equal(box[64], [m[:, 0].min(), m[:, 1].max(), m[:, 2].min(), m[:, 3].max()])
    np.testing.assert_array_equal(box[128], [-inf, inf, -inf, inf])     # chunk 2: holds a NaN box
    own = [f for f in range(129, 192) if f != nan_face]
    np.testing.assert_array_equal(box[own], want[own])
    assert box[own, 0].min() > 1.5                                      # ... among off-screen faces
    if nan_face != 128:
        assert np.isnan(box[nan_face, :2]).all()


@pytest.mark.parametrize("K", [4, 140])
def test_list_overflow_rounds(K, device, monkeypatch):
    """600 stacked triangles over every tile of an 8x8 image: more than one round's list (128 faces
    at 4 and 8 slices), so a pass of 64 faces that would overflow it starts the next round."""
    rng = np.random.default_rng(51)
    F = 600
    fv = np.empty((F, 3, 3), np.float32)
    fv[:, 0, :2], fv[:, 1, :2], fv[:, 2, :2] = (-3.0, -2.5), (3.0, -2.5), (0.0, 3.5)
    fv[:, :, :2] += rng.uniform(-0.2, 0.2, (F, 3, 2)).astype(np.float32)
    fv[:, :, 2] = rng.uniform(0.5, 5.0, (F, 1)).astype(np.float32) + rng.uniform(0, 0.1, (F, 3)).astype(np.float32)
    first, nf = np.array([0]), np.array([F])
    for persp, clip in MODES:
        got = _both(fv, first, nf, 8, 8, K, persp, clip, device, monkeypatch)
        rp = _check_oracle(got, fv, first, nf, 8, 8, K, persp, clip)
        assert ((rp >= 0).sum(-1) == K).all()


def test_chunk_boxes_that_cover_everything(device, monkeypatch):
    """The 129-face mesh in shuffled face order: every chunk's union box spans the image, so no
    chunk is rejected and the second level does all the culling."""
    fv = _mesh129()[np.random.default_rng(61).permutation(129)]
    first, nf = np.array([0]), np.array([129])
    for persp, clip in MODES:
        got = _both(fv, first, nf, 32, 32, 8, persp, clip, device, monkeypatch)
        assert (_check_oracle(got, fv, first, nf, 32, 32, 8, persp, clip) >= 0).sum() > 100


def test_more_surviving_chunks_than_one_group_of_passes(device, monkeypatch):
    """24 chunks of small triangles scattered over the image: every chunk box covers every tile, so
    each tile walks all 24 chunks -- more than the 16 passes in flight at once, i.e. a second group
    of passes in the same window -- while most tiles keep fewer than 64 faces.  (A chunk visited
    twice would put a face into a list twice.)"""
    F = 24 * 64
    fv = _tris(F, 71, spread=0.95, size=0.03)
    first, nf = np.array([0]), np.array([F])
    for persp, clip in MODES:
        got = _both(fv, first, nf, 64, 64, 8, persp, clip, device, monkeypatch)
        assert (_check_oracle(got, fv, first, nf, 64, 64, 8, persp, clip) >= 0).sum() > 1000

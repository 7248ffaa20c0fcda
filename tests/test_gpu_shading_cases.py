"""The Phong shading kernels (pr_shade_fwd / pr_shade_bwd, csrc/pr_shade.hip and pr_phong.h) against
the float64 composition on hand-built fragments (shading_cases.py; pinned on the CPU by
test_shading_cases_cpu.py): colours and every gradient -- barycentrics, vertices (through positions
and normals), texture (map, vertex colours or given texels), light and camera -- on both autograd
layers and the three kernel paths, at the frames where the layouts change: pixel blocks that hold
two images and a tail block, 16-byte padded stores over a live / padded pair of slots, K = 1, 3, 5,
10, 12, 64, 65, the four accumulator layouts of the backward, more images than the padded-terms
table holds, deterministic batches that end inside a pixel, and a face whose normals are exactly 0.

Bars: |err| <= 5e-6 max|ref| on colours, 2e-4 max|ref| on each gradient (test_gpu_shading.py's), with
nothing left out of a comparison; a reference gradient that is identically zero asks for exact
zeros.  Every test prints err / bar per output."""
import os

import pytest
import torch

import pose_cases
import shading_cases as sc
from pertrenderer_amd import host_layer
from pertrenderer_amd.renderer import shading as sh

pytestmark = pytest.mark.gpu

# counts attached: the pixel-block kernels / PR_SHADE_PIX=0: the chunk kernels reading the counts /
# nothing attached: the chunk kernels reading pix_to_face.  Given texels always take the chunk kernels.
PATHS = ("pixel-blocks", "chunks-counts", "chunks-faces")


def _paths(spec):
    return PATHS[1:] if spec.tex == "given" else PATHS


@pytest.fixture(params=pose_cases.LAYERS)
def layer(request):
    with pose_cases.autograd_layer(request.param) as ok:
        if not ok:
            pytest.skip(f"C++ autograd layer not built: {host_layer.error()}")
        yield request.param


def _shade(c, device, path, monkeypatch, live_only=False):
    """The library's colours of case c on `path` and the leaves they depend on."""
    if path == "chunks-counts":
        monkeypatch.setenv("PR_SHADE_PIX", "0")
    else:
        monkeypatch.delenv("PR_SHADE_PIX", raising=False)
    meshes, frag, lights, cams, mats, leaves, texels = sc.scene(c, device, torch.float32,
                                                                "plain" if path == "chunks-faces" else "counts")
    if c.spec.tex == "given":
        out = sh.phong_shading(meshes, frag, lights, cams, mats, texels)
    else:
        out = sh.textured_phong_shading(meshes, frag, lights, cams, mats, live_only=live_only)
    assert bool(getattr(out, "_pr_live_only", False)) == live_only
    return out, leaves


def _check(got, ref, what, inside=None):
    """Every output of `got` against `ref` at the bars; `inside`: the slots compared for colours and
    d bary (live_only leaves the others unwritten)."""
    bad = []
    for name, a, b in zip(sc.Ref._fields, got, ref):
        r = sc.ratio(a, b, sc.COLOUR_BAR if name == "colours" else sc.GRAD_BAR,
                     inside if name in ("colours", "d_bary") else None)
        print(f"{what} {name}: err / bar = {r:.3g}")
        if not r <= 1.0:
            bad.append((name, r))
    assert not bad, (what, bad)


def _run(spec, device, path, monkeypatch, live_only=False):
    c = sc.build(spec)
    out, leaves = _shade(c, device, path, monkeypatch, live_only)
    got = sc.grads_of(out, leaves, c.G.to(device))
    _check(got, sc.shade_ref64(spec), f"{sc.spec_id(spec)} {path}{' live-only' if live_only else ''}",
           c.inside if live_only else None)
    return c, got


LIVE_ONLY = [(s, p) for s in sc.FULL_CROSS + sc.OTHER_GEOMETRIES if s.tex != "given" for p in PATHS[:2]]


@pytest.mark.parametrize("spec,path", [(s, p) for s in sc.FULL_CROSS for p in _paths(s)],
                         ids=lambda v: sc.spec_id(v) if isinstance(v, sc.Spec) else v)
def test_textures_and_lights(spec, path, layer, device, monkeypatch):
    """Every texture and light kind at 3 x 5 x 7 x 5: 105 pixels, one full pixel block that holds an
    image boundary and a 41-pixel tail; every per-image row differs."""
    _run(spec, device, path, monkeypatch)


@pytest.mark.parametrize("spec,path", [(s, p) for s in sc.OTHER_GEOMETRIES for p in PATHS],
                         ids=lambda v: sc.spec_id(v) if isinstance(v, sc.Spec) else v)
def test_geometries(spec, path, layer, device, monkeypatch):
    """K = 1, 3, 10, 12, 64, 65: the padded stores' phases against the pixel size (K = 12 and 64 are the
    multiple-of-4 controls) and the chunk kernels' 64-slot walk (q64 = 64, r64 = 0, q64 = 0)."""
    _run(spec, device, path, monkeypatch)


@pytest.mark.parametrize("spec,path", LIVE_ONLY, ids=lambda v: sc.spec_id(v) if isinstance(v, sc.Spec) else v)
def test_live_only(spec, path, layer, device, monkeypatch):
    """live_only: colours and d bary compared inside the counts only (the rest is unwritten), every
    other gradient in full."""
    _run(spec, device, path, monkeypatch, live_only=True)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(sc.ACCUMULATORS))
def test_accumulator_layouts(name, path, layer, device, monkeypatch):
    """The backward's per-vertex and per-image sums in the LDS table or as global atomics, all four
    combinations, and N = 257: past the padded-terms table and the pixel-block kernels."""
    spec, expected = sc.ACCUMULATORS[name]
    c = sc.build(spec)
    V, N = c.verts.shape[0], spec.N
    assert (V * 9 + N * 6 <= 8192, N * 6 <= 2048) == expected  # pr_shade_bwd's Tab.useV, Tab.useB
    _run(spec, device, path, monkeypatch)


@pytest.mark.parametrize("spec", sc.DETERMINISTIC, ids=sc.spec_id)
def test_deterministic_batches(spec, layer, device, monkeypatch):
    """The ordered-sum backward in batches of 37 slots (a batch ends inside a pixel of 5 slots): the
    reference's values, and two runs agree bit for bit on every gradient."""
    assert sc.DET_BATCH % spec.K and sc.DET_BATCH < spec.N * spec.H * spec.W * spec.K
    ref = sc.shade_ref64(spec)  # (before the switch: the reference's own backward is torch's)
    runs = []
    old_mode, old = torch.are_deterministic_algorithms_enabled(), os.environ.get("PR_DET_BATCH")
    os.environ["PR_DET_BATCH"] = str(sc.DET_BATCH)
    torch.use_deterministic_algorithms(True)
    try:
        for _ in range(2):
            runs.append(_run(spec, device, "pixel-blocks", monkeypatch)[1])
    finally:
        torch.use_deterministic_algorithms(old_mode)
        if old is None:
            os.environ.pop("PR_DET_BATCH", None)
        else:
            os.environ["PR_DET_BATCH"] = old
    assert ref is sc.shade_ref64(spec)
    for name, a, b in zip(sc.Ref._fields, *runs):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("spec,path", [(s, p) for s in sc.DEGENERATE for p in _paths(s)],
                         ids=lambda v: sc.spec_id(v) if isinstance(v, sc.Spec) else v)
def test_degenerate_normals(spec, path, layer, device, monkeypatch):
    """Slots on an isolated collinear face: vertex normals and interpolated normal exactly 0
    (normalize's and normalize_bwd's <= eps branch).  Everything is finite and at the bars; for a
    cotangent on those slots alone the colour is ambient * texel and every gradient but the texture's
    (and d bary through it) is exactly zero."""
    c = sc.build(spec)
    out, leaves = _shade(c, device, path, monkeypatch)
    what = f"{sc.spec_id(spec)} {path}"
    got = sc.grads_of(out, leaves, c.G.to(device), retain=True)
    for name, t in zip(sc.Ref._fields, got):
        assert bool(torch.isfinite(t).all()), name
    _check(got, sc.shade_ref64(spec), what)
    ref = sc.degenerate_ref64(spec)
    for name in ("d_verts", "d_light", "d_T"):
        assert not bool(getattr(ref, name).any()), name
    assert bool(ref.d_tex.any())
    only = sc.grads_of(out, leaves, (c.G * c.degenerate[..., None]).to(device))
    _check(only, ref, what + " isolated face only")
    d = c.degenerate
    texel = {"uv": None, "vertex": None, "given": c.tex}[spec.tex]
    if texel is not None:  # given texels: the colour is the float32 product itself
        exp = (c.ambient[:, None, None, None, :] * texel)[d]
        assert torch.equal(got.colours.cpu()[d], exp)

"""The perturbed blend against the CPU oracle on every launch geometry of pr_blend.hip.

The host picks the geometry from (K, Sa, P): pixels per block PB, record capacity cap (MULTI: several
passes per block), lanes per pixel lpp (8 / 16 / 32), the forward's argmax stripes NC, the backward's
B2 register or LDS path and its B6 lane split nch (1..16), PR_FOR_SLOTS over Sa with qS = 256 / Sa
(0 past 256 samples), partial last blocks and blocks that straddle two images.  The default frames
of the other oracle tests reach lpp 8 / 16 and nch = 1 only; here PR_BLEND_PB_FWD / _BWD (read per
call) bring the geometries of large frames -- the cfg 3 backward (PB 32, MULTI, lpp 8) and the cfg 4
backward (the same with nch = 4) among them -- down to frames of under 150 pixels.

Every case first asserts, through pr_blend_geometry, the path it was written for (a retune of the LDS
targets then fails here instead of silently emptying the sweep), then compares image, d dists,
d zbuf, d colours (or d bary / d vertex colours; or the weights and d prob of the standalone
aggregate) and d sigma, d gamma, d alpha with oracle/blend_oracle.py under injected noise.

Tolerances are the project's: conftest.assert_close defaults (1e-5 relative + 1e-6 of the largest
element) for images and per-element gradients, rtol 1e-4 for the scalars
(test_fused_blend_matches_oracle_random).  The alpha channel 1 - prod(1 - prob) and the Monte-Carlo
weights are compared exactly: prob is a count / Sr with Sr <= 4, so every factor is a multiple of
1/4 and the product is exact in fp32 in any order (a zero factor, or at most 15 factors of 3/4);
the weights are counts / Sa.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import assert_close
from oracle import blend_oracle as bo
from pertrenderer_amd import Noise, perturbed_aggregate, perturbed_blend
from pertrenderer_amd import _native as nat
from pertrenderer_amd.blend import perturbed_blend_vertex
from pertrenderer_amd.renderer.rasterizer import attach_valid_counts
from test_gpu_batch_grid_parity import _texels
from test_gpu_blend import _leaf, _oracle, _run_fused, _synthetic

gpu = pytest.mark.gpu
ENV = ("PR_BLEND_PB_FWD", "PR_BLEND_PB_BWD", "PR_BLEND_LDS_KB_FWD", "PR_BLEND_LDS_KB_BWD")
FIELDS = ("PB", "cap", "lds_bytes", "lpp", "multi", "NC", "nch", "b2_regs", "interleaved")

# name: (N, H, W, K, Sr, Sa), {PR_BLEND_PB_<FWD|BWD>}, expected forward fields, expected backward
# fields, edge (MULTI cases: a second input whose first block mixes empty, full and ordinary pixels).
# Cases with enough slots also run "thin" fragments (_thin).
CASES = {
    "k1_partial": ((1, 3, 3, 1, 2, 2), {}, dict(multi=0), dict(multi=0, nch=1, b2_regs=1), False),
    "nch2_lpp8": ((2, 5, 7, 63, 4, 29), {}, dict(multi=1), dict(lpp=8, multi=1, nch=2, b2_regs=0), True),
    "nch2_lpp16": ((2, 5, 7, 64, 4, 30), {}, dict(multi=1), dict(lpp=16, multi=1, nch=2, b2_regs=0), True),
    "nch4": ((1, 6, 6, 129, 4, 61), {}, dict(multi=1), dict(multi=1, nch=4), True),
    "nch8": ((1, 4, 5, 40, 4, 128), {}, dict(multi=0, NC=1), dict(multi=1, nch=8), True),
    "sa257": ((1, 3, 3, 16, 2, 257), {}, dict(multi=0), dict(multi=1, nch=16), True),
    "sa4096": ((1, 2, 2, 8, 2, 4096), {}, dict(multi=0), dict(PB=2, multi=1, nch=16), True),
    "cfg3_bwd": ((1, 8, 9, 100, 4, 16), dict(BWD=32), dict(multi=1),
                 dict(PB=32, lpp=8, multi=1, nch=1, b2_regs=0), True),
    "cfg4_bwd": ((2, 9, 7, 150, 4, 64), dict(BWD=32), dict(multi=1),
                 dict(PB=32, lpp=8, multi=1, nch=4, b2_regs=0), True),
    "pb4_lpp32": ((1, 6, 6, 150, 4, 8), dict(FWD=4, BWD=4), dict(PB=4, lpp=32, multi=0, NC=32),
                  dict(PB=4, lpp=32, multi=0, b2_regs=1), False),
    "pb8_lpp16": ((2, 5, 5, 127, 4, 8), dict(FWD=8, BWD=8), dict(PB=8, lpp=16, multi=0),
                  dict(PB=8, lpp=16, multi=1, b2_regs=0), True),
    "pb8_lpp32": ((2, 5, 5, 128, 4, 8), dict(FWD=8, BWD=8), dict(PB=8, lpp=32, multi=0),
                  dict(PB=8, lpp=32, multi=1, b2_regs=0), True),
    "regs_lpp16": ((1, 5, 5, 100, 4, 8), dict(BWD=8), dict(multi=1), dict(PB=8, lpp=16, multi=0, b2_regs=1), True),
    "pb1": ((1, 6, 6, 12, 4, 8), dict(FWD=1, BWD=1), dict(PB=1, multi=0), dict(PB=1, multi=0, b2_regs=1), False),
    "pb2": ((1, 6, 6, 12, 4, 8), dict(FWD=2, BWD=2), dict(PB=2, multi=0), dict(PB=2, multi=0, b2_regs=1), False),
}
# blocks that straddle two images (and so look up the second image's planes) / partial last blocks
STRADDLE = ("nch2_lpp8", "nch2_lpp16", "cfg4_bwd", "pb8_lpp16", "pb8_lpp32")
PARTIAL = ("k1_partial", "nch2_lpp8", "nch2_lpp16", "cfg4_bwd")
THIN = tuple(n for n, c in CASES.items() if c[0][3] >= 12 and c[0][2] * c[0][1] * c[0][3] > 200)  # enough slots for hits
TEXEL = [(n, v) for n, c in CASES.items()
         for v in ("random",) + (("edge",) if c[4] else ()) + (("thin",) if n in THIN else ())]


def _set_env(monkeypatch, name):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in CASES[name][1].items():
        monkeypatch.setenv("PR_BLEND_PB_" + k, str(v))


def _query(name):
    """(forward, backward) geometry of a case under the current environment (host only)."""
    N, H, W, K, Sr, Sa = CASES[name][0]
    p = nat.PRBlendParams()
    p.N, p.H, p.W, p.K, p.Sr, p.Sa = N, H, W, K, Sr, Sa
    out = []
    for bwd in (0, 1):
        g = nat.PRBlendGeometry()
        nat.check(nat.load().pr_blend_geometry(p, bwd, g), "pr_blend_geometry")
        out.append({k: getattr(g, k) for k in FIELDS})
    return out


def _assert_geometry(monkeypatch, name):
    """Set the case's environment and assert it lands on the geometry it was written for."""
    _set_env(monkeypatch, name)
    (N, H, W, K, Sr, Sa), _, want_f, want_b, edge = CASES[name]
    gf, gb = _query(name)
    for got, want, which in ((gf, want_f, "forward"), (gb, want_b, "backward")):
        for k, v in want.items():
            assert got[k] == v, f"{name} {which}: {k} = {got[k]}, written for {v} ({got})"
        assert got["multi"] == int(got["cap"] < got["PB"] * (K + 1))
    if edge:
        assert gf["multi"] or gb["multi"], name
    if name in STRADDLE:
        assert N > 1 and (H * W) % gb["PB"] != 0, name
    if name in PARTIAL:
        assert (N * H * W) % gb["PB"] != 0 and (N * H * W) % gf["PB"] != 0, name
    return gf, gb


def test_every_case_lands_on_its_geometry(monkeypatch):
    for name in CASES:
        _assert_geometry(monkeypatch, name)


def test_cases_cover_every_geometry(monkeypatch):
    """The union of the geometries the cases report holds every path the kernels have."""
    fwd, bwd = [], []
    for name in CASES:
        gf, gb = _assert_geometry(monkeypatch, name)
        fwd.append(gf), bwd.append(gb)
    assert {g["lpp"] for g in fwd} >= {8, 16, 32} and {g["lpp"] for g in bwd} >= {8, 16, 32}
    assert {g["nch"] for g in bwd} == {1, 2, 4, 8, 16}
    for lpp in (16, 32):
        assert {g["b2_regs"] for g in bwd if g["lpp"] == lpp} == {0, 1}, lpp
    assert {g["multi"] for g in fwd} == {0, 1} and {g["multi"] for g in bwd} == {0, 1}
    assert {g["PB"] for g in bwd} == {1, 2, 4, 8, 16, 32}
    assert {g["NC"] for g in fwd} >= {1, 32}


def _edge_block(f, seed, npix=32):
    """The first `npix` pixels (the first block of either kernel) cycle through no valid slot, all K
    slots valid, and the pixel as drawn: passes then end on pixels of 1 and of K + 1 entries."""
    g = torch.Generator().manual_seed(seed)
    K = f["pix_to_face"].shape[-1]
    p2f, d, z = (f[k].reshape(-1, K) for k in ("pix_to_face", "dists", "zbuf"))  # views: edited in place
    for i in range(min(npix, p2f.shape[0])):
        if i % 3 == 2:
            continue
        cnt = 0 if i % 3 == 0 else K
        p2f[i] = np.where(np.arange(K) < cnt, torch.randint(0, 5000, (K,), generator=g).numpy(), -1)
        d[i] = np.where(np.arange(K) < cnt, ((torch.rand(K, generator=g) - 0.5) * 6 * float(f["sigma"])).numpy(), -1.0)
        z[i] = np.where(np.arange(K) < cnt, (5.0 + torch.rand(K, generator=g)).numpy(), -1.0)
    cnt = (f["pix_to_face"].reshape(-1, K)[:npix] >= 0).sum(-1)
    assert (cnt == 0).any() and (cnt == K).any() and ((cnt > 0) & (cnt < K)).any()


def _thin(f, seed):
    """Every valid slot 2.0 to 2.6 sigma outside its face: a few percent of the slots draw a hit, so
    prod(1 - prob) has a handful of factors below 1 and none that is 0 -- the exclusive products of
    the alpha gradient are non-zero across every lane chunk (with _synthetic's distances nearly
    every pixel of a large K holds a slot of probability 1, which zeroes them), and most slots
    have probability 0: logit -inf."""
    g = torch.Generator().manual_seed(seed)
    valid = f["pix_to_face"] >= 0
    d = (2.0 + 0.6 * torch.rand(valid.shape, generator=g)).numpy() * f["sigma"]
    f["dists"] = np.where(valid, d, np.float32(-1.0)).astype(np.float32)


def _planes(N):
    """Each image its own znear / zfar (test_gpu_planes._planes), as constants."""
    return torch.linspace(1.5, 2.0, N).reshape(N, 1, 1, 1), torch.linspace(40.0, 50.0, N).reshape(N, 1, 1, 1)


T = lambda a: torch.from_numpy(np.asarray(a))


@functools.lru_cache(maxsize=None)
def _inputs(name, variant):
    shape = CASES[name][0]
    f = _synthetic(*shape, seed=sum(shape) + len(name))
    if variant == "edge":
        _edge_block(f, seed=sum(shape))
    if variant == "thin":
        _thin(f, seed=sum(shape))
    return f


@functools.lru_cache(maxsize=None)
def _reference(name, variant):
    """Oracle image, gradients and saved state of a case (computed once, shared, never modified)."""
    f = _inputs(name, variant)
    N = CASES[name][0][0]
    if N == 1:
        img, og, s = _oracle(f)
    else:
        zn, zf = _planes(N)
        img, s = bo.blend_forward(T(f["pix_to_face"]), T(f["dists"]), T(f["zbuf"]), T(f["colors"]), T(f["noise_r"]),
                                  T(f["noise_a"]), T(f["sigma"]), T(f["gamma"]), T(f["alpha"]), float(f["eps"]),
                                  T(f["background"]), zn, zf)
        og = bo.blend_backward(T(f["grad_image"]), s)
    # the alpha channel is exact in any order (module docstring): the exact comparison below rests on it
    om = s["one_minus"]
    assert f["Sr"] <= 4 and bool(((om == 0).any(-1) | ((om == 0.75).sum(-1) <= 15)).all())
    return img, og, s


def _frag_tensors(f, dev, counts):
    p2f = torch.tensor(f["pix_to_face"], device=dev)
    if counts:
        attach_valid_counts(p2f, (p2f >= 0).sum(-1).to(torch.int32))
    d = torch.tensor(f["dists"], device=dev, requires_grad=True)
    z = torch.tensor(f["zbuf"], device=dev, requires_grad=True)
    noise = Noise.injected(torch.tensor(f["noise_r"], device=dev), torch.tensor(f["noise_a"], device=dev))
    N = p2f.shape[0]
    zn, zf = _planes(N) if N > 1 else (torch.full((1, 1, 1, 1), float(f["znear"])), torch.full((1, 1, 1, 1), float(f["zfar"])))
    kw = dict(eps=float(f["eps"]), background=tuple(f["background"]), znear=zn.to(dev), zfar=zf.to(dev), noise=noise)
    return p2f, d, z, kw


def _run(f, dev, counts):
    """test_gpu_blend._run_fused, with per-image planes on batches."""
    if f["pix_to_face"].shape[0] == 1:
        return _run_fused(f, dev, counts=counts)
    p2f, d, z, kw = _frag_tensors(f, dev, counts)
    c = torch.tensor(f["colors"], device=dev, requires_grad=True)
    s, g, a = _leaf(f["sigma"]), _leaf(f["gamma"]), _leaf(f["alpha"])
    img = perturbed_blend(c, p2f, d, z, s, g, a, int(f["Sr"]), int(f["Sa"]), **kw)
    (img * torch.tensor(f["grad_image"], device=dev)).sum().backward()
    return img, dict(dists=d.grad, zbuf=z.grad, colors=c.grad, sigma=s.grad, gamma=g.grad, alpha=a.grad)


def _compare(img, g, oimg, og, keys):
    assert torch.isfinite(img).all()
    assert torch.equal(img[..., 3].detach().cpu(), oimg[..., 3]), "alpha channel"
    assert_close(img, oimg, name="image")
    # K = 1: a pixel's one slot is its own z_max, so its logit (gamma / alpha) log P lies far above
    # the background's eps - z_max at gamma = 1e-2: every sample picks the unperturbed argmax and the
    # aggregation's gradients (d zbuf, d gamma, d alpha) are exactly 0 in the oracle -- and must be here
    flat =() if oimg.shape[:3] + (1,) != og["zbuf"].shape else ("zbuf", "gamma", "alpha")
    for k in keys:
        assert k in flat or float(og[k].abs().max()) > 0, k  # a real signal to compare
        assert_close(g[k], og[k], name="d " + k)
    for k in ("sigma", "gamma", "alpha"):
        assert k in flat or float(og[k].abs()) > 0, k
        assert_close(g[k], og[k], rtol=1e-4, atol_rel=0, name="d " + k)


@gpu
@pytest.mark.parametrize("counts", [False, True])
@pytest.mark.parametrize("name,variant", TEXEL)
def test_texel_blend_matches_oracle(name, variant, counts, device, monkeypatch):
    """Colour mode 1 on every geometry; counts=True walks the valid prefix only."""
    _assert_geometry(monkeypatch, name)
    f = _inputs(name, variant)
    oimg, og, _ = _reference(name, variant)
    img, g = _run(f, device, counts)
    _compare(img, g, oimg, og, ("dists", "zbuf", "colors"))


# ------------------------------------------------------------------ fused TexturesVertex blend
V_, F_ = 1600, 5000  # (_synthetic draws face ids below 5000)


@functools.lru_cache(maxsize=None)
def _vertex_reference(name):
    f = _inputs(name, "random")
    g = torch.Generator().manual_seed(7 + len(name))
    valid = T(f["pix_to_face"]) >= 0
    b = torch.rand(valid.shape + (3,), generator=g) + 0.05
    v = dict(p2f=T(f["pix_to_face"]), faces=torch.randint(0, V_, (F_, 3), generator=g), vc=torch.rand((V_, 3), generator=g),
             bary=torch.where(valid[..., None], b / b.sum(-1, keepdim=True), torch.full_like(b, -1.0)))
    bary, vc = v["bary"].clone().requires_grad_(True), v["vc"].clone().requires_grad_(True)
    colors = _texels(dict(v, bary=bary, vc=vc))
    N = valid.shape[0]
    zn, zf = _planes(N) if N > 1 else (torch.full((1, 1, 1, 1), float(f["znear"])), torch.full((1, 1, 1, 1), float(f["zfar"])))
    oimg, s = bo.blend_forward(v["p2f"], T(f["dists"]), T(f["zbuf"]), colors.detach(), T(f["noise_r"]), T(f["noise_a"]),
                               T(f["sigma"]), T(f["gamma"]), T(f["alpha"]), float(f["eps"]), T(f["background"]), zn, zf)
    og = bo.blend_backward(T(f["grad_image"]), s)
    colors.backward(og["colors"])  # d bary, d vertex colours: torch autograd of the gather from the oracle's d colours
    og["bary"] = torch.where(valid[..., None], bary.grad, torch.zeros_like(bary.grad))
    og["vc"] = vc.grad
    return v, oimg, og


@gpu
@pytest.mark.parametrize("counts", [False, True])
@pytest.mark.parametrize("name", ["cfg3_bwd", "cfg4_bwd", "pb4_lpp32"])
def test_vertex_blend_matches_oracle(name, counts, device, monkeypatch):
    """Colour mode 2: slot colours interpolated in the kernels from per-vertex colours."""
    _assert_geometry(monkeypatch, name)
    f = _inputs(name, "random")
    v, oimg, og = _vertex_reference(name)
    p2f, d, z, kw = _frag_tensors(f, device, counts)
    b = v["bary"].to(device).requires_grad_(True)
    vc = v["vc"].to(device).requires_grad_(True)
    s, gm, a = _leaf(f["sigma"]), _leaf(f["gamma"]), _leaf(f["alpha"])
    img = perturbed_blend_vertex(vc, v["faces"].to(device), p2f, b, d, z, s, gm, a, int(f["Sr"]), int(f["Sa"]), **kw)
    (img * torch.tensor(f["grad_image"], device=device)).sum().backward()
    g = dict(dists=d.grad, zbuf=z.grad, bary=b.grad, vc=vc.grad, sigma=s.grad, gamma=gm.grad, alpha=a.grad)
    _compare(img, g, oimg, og, ("dists", "zbuf", "bary", "vc"))


# ------------------------------------------------------------------ standalone aggregate
@gpu
@pytest.mark.parametrize("name", ["cfg4_bwd", "sa257"])
def test_aggregate_matches_oracle(name, device, monkeypatch):
    """Colour mode 0 (probabilities in, weights out), as test_gpu_planes'
    test_aggregate_plane_gradients_match_oracle: W exact (counts / Sa), gradients at the bar."""
    _assert_geometry(monkeypatch, name)
    N, H, W, K, Sr, Sa = CASES[name][0]
    f = _inputs(name, "random")
    zn, zf = (t.to(device).requires_grad_(True) for t in _planes(N))
    z = torch.tensor(f["zbuf"], device=device, requires_grad=True)
    prob = torch.rand((N, H, W, K), generator=torch.Generator().manual_seed(2)) * 0.9 + 0.05
    pr = prob.to(device).requires_grad_(True)
    mask = torch.tensor(f["pix_to_face"], device=device) >= 0
    gW = torch.randn((N, H, W, K + 1), generator=torch.Generator().manual_seed(3))
    g, a = _leaf(f["gamma"]), _leaf(f["alpha"])
    Wt = perturbed_aggregate(z, zf, zn, pr, mask, g, a, Sa, eps=float(f["eps"]),
                             noise=Noise.injected(noise_a=torch.tensor(f["noise_a"], device=device)))
    (Wt * gW.to(device)).sum().backward()
    out = bo.aggregate_forward_backward(T(f["zbuf"]), zf.detach().cpu(), zn.detach().cpu(), prob, mask.cpu(),
                                        T(f["noise_a"]), T(f["gamma"]), T(f["alpha"]), float(f["eps"]), gW, planes=True)
    assert torch.equal(Wt.detach().cpu(), out[0]), "W"
    assert_close(z.grad, out[1], name="d zbuf")
    assert_close(pr.grad, out[2], name="d prob")
    assert_close(g.grad, out[3], rtol=1e-4, atol_rel=0, name="d gamma")
    assert_close(a.grad, out[4], rtol=1e-4, atol_rel=0, name="d alpha")
    assert_close(zn.grad, out[5], rtol=1e-4, atol_rel=1e-6, name="d znear")
    assert_close(zf.grad, out[6], rtol=1e-4, atol_rel=1e-6, name="d zfar")

"""PR_BLEND_PHONG's sparse colour buffer: the forward and the backward agree on the slots it holds.

The fused Phong forward writes `colors` only at the slots that won a sample and at its own
unperturbed argmax j0 (found among the argmax candidates); the PR_BLEND_COLOR_SPARSE backward
recomputes that argmax in B2 -- its register path or its LDS path, per lane chunk, then merged over
the pixel's lanes -- and reads colors[j0].  The buffer comes from torch.empty, so a disagreement
would build dW from uninitialised memory.  Hand-built fragments put the two searches on their edges
(exact logit ties inside a lane chunk, across lane chunks and on pixels at pass boundaries, a slot
tied with the background, no finite slot logit, every z_inv negative, empty and full pixels, an
argmax that wins no sample), at K = 12 (single pass, register path) and at K = 150 on the default
geometry and with PR_BLEND_PB_BWD=32 (multi-pass, LDS path, 10- and 19-entry chunks):

* through RandomPhongShader, the image, d dists, d zbuf and d bary equal the unfused shade -> blend
  path bit for bit and every gradient is finite, with torch (injected) and Philox draws;
* through the C ABI with `colors` pre-filled with NaN, the slots the forward wrote are exactly the
  winners and the oracle's unperturbed argmax (first index on ties; oracle/blend_oracle.py logits on
  the forward's own probabilities), and the backward's outputs are finite.
"""
import numpy as np
import pytest
import torch

import pertrenderer_amd as pa
import pertrenderer_amd.blend as pb
import pertrenderer_amd.random_rasterizer as rr
from conftest import assert_close
from oracle import blend_oracle as bo
from pertrenderer_amd import Noise, noise
from pertrenderer_amd import _native as nat
from pertrenderer_amd.renderer.rasterizer import Fragments, attach_valid_counts
from pertrenderer_amd.renderer.shading import phong_inputs
from test_gpu_shading import _scene

pytestmark = pytest.mark.gpu

H = W = 8
S = 4
SIG, GAM, EPS, ZN, ZF = 1e-3, 1e-2, 2.0 ** -10, 1.0, 2.0
BG = (0.2, 0.3, 0.4)
# (K, PR_BLEND_PB_BWD, the backward geometry the case is written for)
CONFIGS = {
    "k12": (12, None, dict(PB=16, lpp=8, multi=0, b2_regs=1)),
    "k150": (150, None, dict(PB=16, lpp=16, multi=1, b2_regs=0)),
    "k150_pb32": (150, "32", dict(PB=32, lpp=8, multi=1, b2_regs=0)),
}
# special pixels of the first block (the others of pixels 0..31 hold exact ties)
BG_TIE, ALL_OUT, ALL_NEG, EMPTY, FULL, CROWD = 3, 7, 12, 17, 20, range(22, 28)


def _geometry(K, bwd):
    p = nat.PRBlendParams()
    p.N, p.H, p.W, p.K, p.Sr, p.Sa = 1, H, W, K, S, S
    g = nat.PRBlendGeometry()
    nat.check(nat.load().pr_blend_geometry(p, bwd, g), "pr_blend_geometry")
    return g


def _setup(name, monkeypatch):
    K, pb_bwd, want = CONFIGS[name]
    for k in ("PR_BLEND_PB_FWD", "PR_BLEND_PB_BWD", "PR_BLEND_LDS_KB_FWD", "PR_BLEND_LDS_KB_BWD"):
        monkeypatch.delenv(k, raising=False)
    if pb_bwd:
        monkeypatch.setenv("PR_BLEND_PB_BWD", pb_bwd)
    g = _geometry(K, 1)
    for k, v in want.items():
        assert getattr(g, k) == v, f"{name}: backward {k} = {getattr(g, k)}, written for {v}"
    return K, g


def _pass_starts(entries, PB, cap):
    """Pixels that begin a second or later pass (block_entries' greedy passes)."""
    out = []
    for b0 in range(0, len(entries), PB):
        ex = np.concatenate([[0], np.cumsum(entries[b0:b0 + PB])])
        est = 0
        for pl in range(1, len(ex) - 1) if ex[-1] > cap else ():
            if ex[pl + 1] - est > cap:
                out.append(b0 + pl)
                est = ex[pl]
    return out


def _fragments(K, F, ckp, seed=5):
    """8 x 8 packed fragments.  Pixels 0..31 hold all K slots; apart from the special pixels each has
    two or three slots of probability exactly 1 (dists = -10 sigma) and one zbuf, above every other
    slot's logit: an exact tie the lowest slot must win -- three slots a few apart (one or two lane
    chunks), slots 0 and ckp = ceil((K + 1) / lpp) (the first entries of two lane chunks), or slots
    ckp - 1 and ckp (either side of a chunk boundary).  Returns the tensors and the expected
    unperturbed argmax of the crafted pixels."""
    g = torch.Generator().manual_seed(seed)
    P = H * W
    cnt = torch.randint(0, K + 1, (P,), generator=g)
    cnt[:32] = K
    cnt[ALL_NEG], cnt[EMPTY] = K // 2, 0
    dists = (torch.rand((P, K), generator=g) - 0.5) * 6 * SIG
    zbuf = 1.3 + 0.5 * torch.rand((P, K), generator=g)  # z_inv = 2 - zbuf in [0.2, 0.7]
    near, far = -10 * SIG, 10 * SIG  # probability exactly 1 / exactly 0
    expect = {}
    for i in range(32):
        if i in (BG_TIE, ALL_OUT, ALL_NEG, EMPTY, FULL) or i in CROWD:
            continue
        a = i % (K - 8)
        tied = ((a, a + 3, a + 7), (0, ckp), (ckp - 1, ckp))[i % 3]
        for j in tied:
            dists[i, j], zbuf[i, j] = near, 1.25  # z_inv = 0.75 = z_max: logit exactly 0
        expect[i] = tied[0]
    # a slot tied with the background: z_inv = z_max = eps = 2^-10 and probability 1, so the slot's and
    # the background's logits are both exactly 0 (every other slot: probability 0, z_inv < 0)
    dists[BG_TIE], zbuf[BG_TIE] = far, 2.0 + 0.25 * torch.rand(K, generator=g)
    dists[BG_TIE, 4], zbuf[BG_TIE, 4] = near, 2.0 - 2.0 ** -10
    expect[BG_TIE] = 4
    dists[ALL_OUT] = far  # every slot logit -inf: the background
    expect[ALL_OUT] = K
    zbuf[ALL_NEG] = 2.1 + 0.4 * torch.rand(K, generator=g)  # every z_inv < 0 < the masked slots' 0: z_max = 0
    expect[ALL_NEG] = K
    expect[EMPTY] = K
    for i in CROWD:  # K near-tied slots of probability 1: slot 0 is the argmax and rarely wins a sample
        dists[i], zbuf[i] = near, 1.5 + 1e-6 * torch.arange(K)
        expect[i] = 0
    valid = torch.arange(K) < cnt[:, None]
    p2f = torch.where(valid, torch.randint(0, F, (P, K), generator=g), torch.full((P, K), -1))
    b = torch.rand((P, K, 3), generator=g) + 0.05
    shape = (1, H, W, K)
    return dict(p2f=p2f.reshape(shape), cnt=cnt.to(torch.int32).reshape(1, H, W), valid=valid.reshape(shape),
                dists=torch.where(valid, dists, torch.full((P, K), -1.0)).reshape(shape),
                zbuf=torch.where(valid, zbuf, torch.full((P, K), -1.0)).reshape(shape),
                bary=torch.where(valid[..., None], b / b.sum(-1, keepdim=True), torch.full_like(b, -1.0)).reshape(shape + (3,)),
                gimg=torch.randn((1, H, W, 4), generator=g)), expect


@pytest.fixture(scope="module")
def scene(device):
    return _scene(device, "vertex", size=H, K=4)


def _case(name, scene, monkeypatch):
    K, g = _setup(name, monkeypatch)
    ckp = (K + 1 + g.lpp - 1) // g.lpp
    fr, expect = _fragments(K, scene[0].faces_packed().shape[0], ckp)
    if g.multi:  # ties sit on both sides of a pass boundary of either kernel
        gf = _geometry(K, 0)
        full, compact = np.full(H * W, K + 1), fr["cnt"].reshape(-1).numpy() + 1
        for entries, PB, cap in ((full, g.PB, g.cap), (compact, g.PB, g.cap), (compact, gf.PB, gf.cap)):
            starts = _pass_starts(entries, PB, cap)
            tie = [s for s in starts if s < 32 and s not in CROWD and s - 1 not in CROWD
                   and expect.get(s, K) < K and expect.get(s - 1, K) < K]
            assert tie, (name, starts)
    return K, fr, expect


def _leaves(fr, device):
    p2f = fr["p2f"].to(device)
    attach_valid_counts(p2f, fr["cnt"].to(device))
    d, z, b = (fr[k].to(device).requires_grad_(True) for k in ("dists", "zbuf", "bary"))
    return p2f, d, z, b


def _shade_blend(scene, fr, fused, source, device):
    mesh, _, lights, cams, mats, verts, loc, extra = scene
    sr = pa.GaussianRast(nb_samples=S, sigma=SIG)
    sa = pa.GaussianAgg(nb_samples=S, gamma=GAM, eps=EPS)
    shader = pa.RandomPhongShader(device=device, cameras=cams, lights=lights, materials=mats, smoothrast=sr,
                                  smoothagg=sa, blend_params=rr.BlendParams(1e-4, 1e-4, BG))
    p2f, d, z, b = _leaves(fr, device)
    old, old_src = rr.FUSE_PHONG, noise.get_noise_source()
    rr.FUSE_PHONG = fused
    noise.set_noise_source(source)
    try:
        torch.manual_seed(19)
        img = shader(Fragments(p2f, z, b, d), mesh, znear=ZN, zfar=ZF)
        leaves = [d, z, b, verts, extra, loc, sr.sigma, sa.gamma, sa.alpha]
        gs = torch.autograd.grad((img * fr["gimg"].to(device)).sum(), leaves, allow_unused=True)
    finally:
        rr.FUSE_PHONG = old
        noise.set_noise_source(old_src)
    return img.detach(), [torch.zeros_like(l) if g is None else g for g, l in zip(gs, leaves)]


@pytest.mark.parametrize("source", ["torch", "philox"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_fused_phong_equals_unfused_on_crafted_pixels(name, source, scene, device, monkeypatch):
    K, fr, _ = _case(name, scene, monkeypatch)
    img_f, g_f = _shade_blend(scene, fr, True, source, device)
    img_u, g_u = _shade_blend(scene, fr, False, source, device)
    names = ["d dists", "d zbuf", "d bary", "verts", "vertex colours", "light", "sigma", "gamma", "alpha"]
    for n, a in zip(names, g_f):
        assert torch.isfinite(a).all(), n
    assert torch.isfinite(img_f).all() and torch.equal(img_f, img_u)
    for n, a, b in zip(names, g_f, g_u):
        if n.startswith("d "):
            assert float(b.abs().max()) > 0, n
            assert torch.equal(a, b), n  # per slot, the same operations
        else:
            assert_close(a, b, rtol=1e-5, atol_rel=1e-6, name=n)  # float-atomic sums


def _oracle_j0(fr, prob):
    """First index of the largest unperturbed logit (smoothagg.py:197-202 in fp32), and its margin
    over the best logit of another value."""
    pl = torch.full((1, 1, 1, 1), 1.0)
    z, _ = bo.logits(fr["zbuf"], pl * ZF, pl * ZN, prob * fr["valid"], fr["valid"], torch.tensor(GAM),
                     torch.tensor(1.0), EPS)
    zm = z.max(-1, keepdim=True).values
    K1 = z.shape[-1]
    j0 = torch.where(z == zm, torch.arange(K1), torch.full_like(z, K1, dtype=torch.int64)).min(-1).values
    second = torch.where(z == zm, torch.full_like(z, -float("inf")), z).max(-1).values
    return j0.reshape(-1), (zm[..., 0] - second).reshape(-1)


@pytest.mark.parametrize("mode", ["injected", "philox"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_forward_writes_exactly_the_slots_the_backward_reads(name, mode, scene, device, monkeypatch):
    K, fr, expect = _case(name, scene, monkeypatch)
    mesh, _, lights, cams, mats = scene[:5]
    P = H * W
    p2f, d, z, b = _leaves(fr, device)
    sh = phong_inputs(mesh, Fragments(p2f, z, b, d), lights, cams, mats)
    assert sh is not None and sh["counts"] is not None
    p2f_c, d_c, z_c = nat.dense(p2f, torch.int64), nat.dense(d, torch.float32), nat.dense(z, torch.float32)
    t = {k: nat.dense(v, torch.float32) for k, v in dict(bary=b, verts=sh["verts"], normals=sh["normals"], tex=sh["tex"],
                                                       light=sh["light"], camera=sh["camera"]).items()}
    g = torch.Generator().manual_seed(23)
    nz = (Noise.injected(torch.randn((S, 1, H, W, K), generator=g), torch.randn((S, 1, H, W, K + 1), generator=g))
          if mode == "injected" else Noise.philox(seed_r=0x51, seed_a=0x52)).to(device)
    zn, zf = pb._planes(ZN, 1, device), pb._planes(ZF, 1, device)
    flags = nat.PR_BLEND_RAST | nat.PR_BLEND_COLOR | nat.PR_BLEND_PHONG
    p = pb._params((1, H, W, K), S, S, (SIG, GAM, 1.0), None, EPS, list(BG), nz, zn, zf, flags)
    image = torch.empty((1, H, W, 4), device=device)
    winners = torch.empty((P, S), dtype=torch.uint8, device=device)
    cache = torch.zeros((1, H, W, K, 2), device=device)
    colors = torch.full((1, H, W, K, 3), float("nan"), device=device)
    sync = pb._sync(device)
    shade = pb._phong_args(sh, p2f_c, t)
    a = nat.PRBlendFwdArgs()
    a.p = p
    a.pix_to_face, a.zbuf, a.dists, a.bary = nat.ptr(p2f_c), nat.ptr(z_c), nat.ptr(d_c), nat.ptr(t["bary"])
    a.colors, a.image, a.winners, a.rast_cache = nat.ptr(colors), nat.ptr(image), nat.ptr(winners), nat.ptr(cache)
    a.pix_count, a.sync, a.shade = nat.ptr(sh["counts"]), nat.ptr(sync), nat.C.addressof(shade)
    nat.call("pr_blend_fwd", "pr_blend_fwd", image, a)
    # the backward on that buffer: NaN wherever the forward did not write
    q = nat.PRBlendParams.from_buffer_copy(p)
    q.flags = (flags & ~nat.PR_BLEND_PHONG) | nat.PR_BLEND_COLOR_SPARSE
    gimg = fr["gimg"].to(device)
    gd, gz, gc = torch.empty_like(d_c), torch.empty_like(z_c), torch.empty_like(colors)
    gsc = torch.empty(3, device=device)
    bw = nat.PRBlendBwdArgs()
    bw.p = q
    bw.pix_to_face, bw.zbuf, bw.dists, bw.colors = nat.ptr(p2f_c), nat.ptr(z_c), nat.ptr(d_c), nat.ptr(colors)
    bw.winners, bw.grad_image, bw.rast_cache = nat.ptr(winners), nat.ptr(gimg), nat.ptr(cache)
    bw.grad_dists, bw.grad_zbuf, bw.grad_colors, bw.grad_scalars = nat.ptr(gd), nat.ptr(gz), nat.ptr(gc), nat.ptr(gsc)
    bw.pix_count, bw.sync = nat.ptr(sh["counts"]), nat.ptr(sync)
    ws = nat.workspace(nat.load().pr_blend_bwd_workspace_size(bw), device)
    bw.workspace, bw.workspace_bytes = nat.ptr(ws), ws.numel()
    nat.call("pr_blend_bwd", "pr_blend_bwd", gimg, bw)
    torch.cuda.synchronize()

    win = winners.cpu().long()
    assert int(win.max()) <= K
    prob = torch.where(fr["valid"], cache[..., 0].cpu(), torch.zeros(()))
    j0, margin = _oracle_j0(fr, prob)
    for i, j in expect.items():  # the construction gives the intended argmax
        assert int(j0[i]) == j, (i, int(j0[i]), j)
    want = torch.zeros((P, K + 1), dtype=torch.bool)
    want.scatter_(1, win, True)
    want.scatter_(1, j0[:, None], True)
    want = want[:, :K]
    got = ~torch.isnan(colors.cpu()).reshape(P, K, 3)
    assert torch.equal(got.all(-1), got.any(-1))
    got = got.all(-1)
    # outside the crafted pixels a near-tie may resolve differently in the oracle's libm
    sure = torch.tensor([i in expect for i in range(P)]) | (margin > 1e-6)
    assert int(sure.sum()) >= P - 2
    bad = (got != want).any(-1) & sure
    assert not bad.any(), f"pixels {bad.nonzero().reshape(-1).tolist()}: written slots differ from winners + argmax"
    # the argmax that wins no sample is written too, and that case occurred
    lone = (j0 < K) & ~(win == j0[:, None]).any(-1)
    assert lone[list(CROWD)].any() and got[lone & sure, j0[lone & sure]].all()
    assert not (win[ALL_OUT] != K).any() and not got[ALL_OUT].any() and not got[EMPTY].any()
    for n, x in (("image", image), ("d dists", gd), ("d zbuf", gz), ("d colours", gc), ("d scalars", gsc)):
        assert torch.isfinite(x).all(), n
    assert float(gd.abs().max()) > 0 and float(gz.abs().max()) > 0

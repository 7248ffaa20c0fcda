"""The blend kernels' shortened block chain (pr_blend.hip; profiles/blend_chain/README.md) computes
what the longer chain computed.

Forward, vertex colours, single-pass template: the image and the winners are compared with the
texel path (colours sampled first by pr_interp_fwd, the same operation order) and with the
multi-pass template (PR_BLEND_LDS_KB_FWD=8), the rast cache with the multi-pass template's, and
image and weights with oracle/blend_oracle.py under injected draws.  (The checks were written for
two restructurings of the single-pass forward that were measured and not kept; they hold for
any rewrite of its phases 1a and 4.)

Backward, PR_BLEND_CHAIN bit 2 (value 2): B2 resolves a won slot's colour gather once, one thread
per entry, and writes its d bary (and d vertex colours) there.  d dists, d zbuf, d bary and the
smoothing scalars must be bitwise those of PR_BLEND_CHAIN=0, d vertex colours equal up to their
float atomics' order; with and without valid-prefix counts, with and without d vertex colours
asked for, under PR_BLEND_LIVE_ONLY (valid rows), and against the oracle.  Bit 1 (value 1, wave
priority of heavy forward blocks) changes no output.

Synthetic fragments, K = 40, Sr = Sa = 8: per-pixel valid prefixes from {0, 1, 7, 33, 40}, so the
forward's 32-pixel blocks fall on both sides of 1024 entries (a second round of phase 1a's walk), one
block built to hold exactly 1024 entries and one 1025; gamma = 0.5 spreads a pixel's 8 samples over
several slots; one pixel row has no fragment and one only fragments outside every sample, so the
background wins each sample; crafted pixels whose unperturbed argmax wins no sample (injected
draws of ordinary size: a draw far in the tail would leave d zbuf of that slot to fp32 cancellation
in kernel and oracle alike)."""
import os

import pytest
import torch

import pertrenderer_amd.blend as pb
from conftest import assert_close
from oracle import blend_oracle as bo
from pertrenderer_amd import Noise
from pertrenderer_amd import _native as nat
from pertrenderer_amd.renderer.interp import interpolate_vertex_attributes

pytestmark = pytest.mark.gpu
K, S = 40, 8
SIG, GAM, ALP, EPS = 1e-3, 0.5, 1.0, 1e-10
BG = (0.1, 0.2, 0.3)
ZN, ZF = 1.0, 100.0
SCALAR_RTOL = 2e-5  # tests/test_gpu_batch_grid_parity.py's
SHAPES = {"64": (1, 64, 64), "50": (1, 50, 50), "2x32": (2, 32, 32)}
PREFIXES = torch.tensor([0, 1, 7, 33, 40])
# the 64 x 64 frame's crafted rows (a forward block is 32 consecutive pixels: half a row)
ROW_1024, ROW_EMPTY, ROW_OUTSIDE, ROW_LONE = 3, 5, 6, 9
LONE_X = (2, 11, 40)


def _frags(name):
    N, H, W = SHAPES[name]
    g = torch.Generator().manual_seed(77 + N * H)
    # per 32-pixel block either a uniform draw from PREFIXES or one weighted to the deep values, whose
    # blocks scatter around 1024 entries (32 x 32.65 slots + 32 background entries = 1077 +- 70)
    P = N * H * W
    light = torch.randint(0, 5, (P,), generator=g)
    deep = torch.multinomial(torch.tensor([0.05, 0.05, 0.05, 0.25, 0.6]), P, replacement=True, generator=g)
    dense = torch.rand(((P + 31) // 32,), generator=g) < 0.5
    cnt = PREFIXES[torch.where(dense.repeat_interleave(32)[:P], deep, light)].reshape(N, H, W)
    if name == "64":
        # 1024 entries = 992 slots + 32 background entries: 23 x 40 + 2 x 33 + 6 x 1 + 0; 1025 = 993 + 32:
        # 23 x 40 + 2 x 33 + 7 + 6 x 0
        cnt[0, ROW_1024, :32] = torch.tensor([40] * 23 + [33] * 2 + [1] * 6 + [0])
        cnt[0, ROW_1024, 32:] = torch.tensor([40] * 23 + [33] * 2 + [7] + [0] * 6)
        cnt[0, ROW_EMPTY] = 0
        for x in LONE_X:
            cnt[0, ROW_LONE, x] = 33
    valid = torch.arange(K) < cnt[..., None]
    shape = (N, H, W, K)
    F_, V = 900, 500
    p2f = torch.where(valid, torch.randint(0, F_, shape, generator=g), torch.full(shape, -1))
    dists = torch.where(valid, (torch.rand(shape, generator=g) - 0.5) * 1.6e-2, torch.full(shape, -1.0))
    zbuf = torch.where(valid, (5.0 + 2.0 * torch.rand(shape, generator=g)).sort(-1).values, torch.full(shape, -1.0))
    nr = torch.randn((S,) + shape, generator=g)
    na = torch.randn((S, N, H, W, K + 1), generator=g)
    if name == "64":
        dists[0, ROW_OUTSIDE] = torch.where(valid[0, ROW_OUTSIDE], torch.tensor(1.0), torch.tensor(-1.0))
        for x in LONE_X:  # slots 0 and 1 deep inside, slot 0 nearer: the unperturbed argmax; every sample's
            dists[0, ROW_LONE, x, :2] = -1.0  # draws (-3 against +3, gamma = 0.5) put slot 1 above it
            na[:, 0, ROW_LONE, x, 0] = -3.0
            na[:, 0, ROW_LONE, x, 1] = 3.0
    b = torch.rand(shape + (3,), generator=g) + 0.05
    f = dict(p2f=p2f, dists=dists, zbuf=zbuf, cnt=cnt.to(torch.int32), valid=valid, nr=nr, na=na,
             bary=torch.where(valid[..., None], b / b.sum(-1, keepdim=True), torch.full_like(b, -1.0)),
             faces=torch.randint(0, V, (F_, 3), generator=g), vc=torch.rand((V, 3), generator=g),
             gimg=torch.randn((N, H, W, 4), generator=g))
    return f


def _noise(f, mode, dev):
    if mode == "injected":
        return Noise.injected(f["nr"], f["na"]).to(dev)
    return Noise.philox(seed_r=0x71, seed_a=0x72).to(dev)


class _Env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        for k, v in self.kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(f, dev, mode, *, texels=False, counts=True, want_vc=True, live_only=False, backward=True):
    """pr_blend_fwd (+ pr_blend_bwd) on the C ABI: every output, gradient buffers pre-filled with NaN."""
    N, H, W, _ = f["p2f"].shape
    shape = (N, H, W, K)
    t = {k: f[k].to(dev).contiguous() for k in ("p2f", "dists", "zbuf", "bary", "faces", "vc", "gimg")}
    cnt = f["cnt"].to(dev).contiguous() if counts else None
    nz = _noise(f, mode, dev)
    zn, zf = pb._planes(ZN, N, dev), pb._planes(ZF, N, dev)
    flags = nat.PR_BLEND_RAST | nat.PR_BLEND_COLOR | (0 if texels else nat.PR_BLEND_VERTEX)
    if live_only:
        flags |= nat.PR_BLEND_LIVE_ONLY
    p = pb._params(shape, S, S, (SIG, GAM, ALP), None, EPS, list(BG), nz, zn, zf, flags)
    colors = interpolate_vertex_attributes(t["p2f"], t["bary"], t["vc"], t["faces"]).contiguous() if texels else None
    image = torch.full((N, H, W, 4), float("nan"), device=dev)
    winners = torch.full((N * H * W, S), 255, dtype=torch.uint8, device=dev)
    cache = torch.zeros(shape + (2,), device=dev)
    sync = pb._sync(dev)
    a = nat.PRBlendFwdArgs()
    a.p = p
    a.pix_to_face, a.zbuf, a.dists = nat.ptr(t["p2f"]), nat.ptr(t["zbuf"]), nat.ptr(t["dists"])
    if texels:
        a.colors = nat.ptr(colors)
    else:
        a.bary, a.faces, a.vert_colors = nat.ptr(t["bary"]), nat.ptr(t["faces"]), nat.ptr(t["vc"])
    a.image, a.winners, a.rast_cache = nat.ptr(image), nat.ptr(winners), nat.ptr(cache)
    a.pix_count, a.sync = nat.ptr(cnt), nat.ptr(sync)
    nat.call("pr_blend_fwd", "pr_blend_fwd", image, a)
    out = dict(image=image, winners=winners, cache=cache)
    if backward:
        nan = lambda *s: torch.full(s, float("nan"), device=dev)
        gd, gz, gb, gsc = nan(*shape), nan(*shape), nan(*shape, 3), nan(3)
        gv = torch.zeros_like(t["vc"]) if want_vc else None
        bw = nat.PRBlendBwdArgs()
        bw.p = p
        bw.pix_to_face, bw.zbuf, bw.dists = nat.ptr(t["p2f"]), nat.ptr(t["zbuf"]), nat.ptr(t["dists"])
        bw.bary, bw.faces, bw.vert_colors = nat.ptr(t["bary"]), nat.ptr(t["faces"]), nat.ptr(t["vc"])
        bw.winners, bw.grad_image, bw.rast_cache = nat.ptr(winners), nat.ptr(t["gimg"]), nat.ptr(cache)
        bw.grad_dists, bw.grad_zbuf, bw.grad_bary = nat.ptr(gd), nat.ptr(gz), nat.ptr(gb)
        bw.grad_vert_colors, bw.grad_scalars = nat.ptr(gv), nat.ptr(gsc)
        bw.pix_count, bw.sync = nat.ptr(cnt), nat.ptr(sync)
        ws = nat.workspace(nat.load().pr_blend_bwd_workspace_size(bw), dev)
        bw.workspace, bw.workspace_bytes = nat.ptr(ws), ws.numel()
        nat.call("pr_blend_bwd", "pr_blend_bwd", t["gimg"], bw)
        out.update(dists=gd, zbuf=gz, bary=gb, vc=gv, scalars=gsc)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def frags():
    return {name: _frags(name) for name in SHAPES}


def _oracle(f):
    sig, gam, alp = (torch.tensor(v) for v in (SIG, GAM, ALP))
    bary = f["bary"].clone().requires_grad_(True)
    vc = f["vc"].clone().requires_grad_(True)
    pc = vc[f["faces"]][f["p2f"].clamp(min=0)]
    colors = torch.where(f["valid"][..., None], (bary[..., None] * pc).sum(-2), torch.zeros(()))
    N = f["p2f"].shape[0]
    pl = torch.ones((N, 1, 1, 1))
    img, saved = bo.blend_forward(f["p2f"], f["dists"], f["zbuf"], colors.detach(), f["nr"], f["na"], sig, gam, alp,
                                  EPS, torch.tensor(BG), pl * ZN, pl * ZF)
    g = bo.blend_backward(f["gimg"], saved)
    colors.backward(g["colors"])
    g["bary"] = torch.where(f["valid"][..., None], bary.grad, torch.zeros(()))
    g["vc"] = vc.grad
    return img, saved["W"], g


@pytest.fixture(scope="module")
def oracle64(frags):
    return _oracle(frags["64"])


def _weights(winners, shape):
    N, H, W = shape
    w = torch.zeros((N * H * W, K + 1))
    w.scatter_add_(1, winners.cpu().long(), torch.ones((N * H * W, S)))
    return (w / S).reshape(N, H, W, K + 1)


def test_frame_exercises_the_cases(frags, device):
    f = frags["64"]
    lds = nat.PRBlendGeometry()
    nz = _noise(f, "philox", device)
    p = pb._params((1, 64, 64, K), S, S, (SIG, GAM, ALP), None, EPS, list(BG), nz, pb._planes(ZN, 1, device),
                   pb._planes(ZF, 1, device), nat.PR_BLEND_RAST | nat.PR_BLEND_COLOR | nat.PR_BLEND_VERTEX)
    assert nat.load().pr_blend_geometry(p, 0, lds) == 0
    assert lds.PB == 32 and not lds.multi
    ent = f["cnt"].reshape(-1, 32).sum(1) + 32  # a block's entries: slots + one background entry per pixel
    row = ROW_1024 * 2
    assert int(ent[row]) == 1024 and int(ent[row + 1]) == 1025
    assert int((ent > 1024).sum()) > 10 and int((ent <= 1024).sum()) > 10
    with _Env(PR_BLEND_LDS_KB_FWD=8):
        assert nat.load().pr_blend_geometry(p, 0, lds) == 0
        assert lds.multi
    for mode in ("philox", "injected"):
        win = _run(f, device, mode, backward=False)["winners"].cpu().long().reshape(64, 64, S)
        distinct = torch.zeros((64, 64, K + 1)).scatter_(2, win, 1.0)
        assert int((distinct.sum(-1) >= 3).sum()) > 100, mode  # samples spread over >= 3 slots
        # a lane of the pixel's 8 meets two won slots (k = l, l + 8, ...)
        per_lane = distinct[..., :K].reshape(64, 64, K // 8, 8).sum(2)
        assert int((per_lane >= 2).sum()) > 20, mode
        assert bool((win[ROW_EMPTY] == K).all()) and bool((win[ROW_OUTSIDE] == K).all()), mode
    for x in LONE_X:  # injected draws: the unperturbed argmax (slot 0) wins no sample
        assert not bool((win[ROW_LONE, x] == 0).any())


@pytest.mark.parametrize("mode", ["philox", "injected"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_matches_texel_path_and_multi_pass_bitwise(name, mode, frags, device):
    f = frags[name]
    a = _run(f, device, mode, backward=False)
    assert bool(torch.isfinite(a["image"]).all()) and int(a["winners"].max()) <= K
    t = _run(f, device, mode, texels=True, backward=False)
    with _Env(PR_BLEND_LDS_KB_FWD=8):
        m = _run(f, device, mode, backward=False)
    for other, what in ((t, "texel path"), (m, "multi-pass")):
        assert torch.equal(a["image"], other["image"]), what
        assert torch.equal(a["winners"], other["winners"]), what
    valid = f["valid"].to(device)
    assert torch.equal(a["cache"][valid], m["cache"][valid])
    assert float(a["cache"][valid][:, 1].abs().max()) > 0


def test_forward_matches_oracle(frags, oracle64, device):
    f = frags["64"]
    oimg, oW, _ = oracle64
    a = _run(f, device, "injected", backward=False)
    assert_close(a["image"], oimg, name="image")
    assert_close(_weights(a["winners"], SHAPES["64"]), oW, name="weights")


def test_priority_bit_changes_no_output(frags, device):
    f = frags["64"]
    with _Env(PR_BLEND_CHAIN=0):
        a = _run(f, device, "philox")
    with _Env(PR_BLEND_CHAIN=1):
        b = _run(f, device, "philox")
    for k in ("image", "winners", "cache", "dists", "zbuf", "bary", "scalars"):
        assert torch.equal(a[k], b[k]), k
    assert_close(b["vc"], a["vc"], name="d vertex colours")


@pytest.mark.parametrize("want_vc", [True, False], ids=["vc", "novc"])
@pytest.mark.parametrize("counts", [True, False], ids=["counts", "nocounts"])
@pytest.mark.parametrize("mode", ["philox", "injected"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_backward_gather_once_is_bitwise(name, mode, counts, want_vc, frags, device):
    f = frags[name]
    with _Env(PR_BLEND_CHAIN=0):
        a = _run(f, device, mode, counts=counts, want_vc=want_vc)
    with _Env(PR_BLEND_CHAIN=2):
        b = _run(f, device, mode, counts=counts, want_vc=want_vc)
    with _Env(PR_BLEND_CHAIN=None):
        c = _run(f, device, mode, counts=counts, want_vc=want_vc)
    for o in (b, c):
        for k in ("image", "winners", "dists", "zbuf", "bary", "scalars"):
            assert bool(torch.isfinite(o[k].float()).all()), k
            assert torch.equal(a[k], o[k]), k
        if want_vc:
            assert_close(o["vc"], a["vc"], name="d vertex colours")
    assert float(a["bary"].abs().max()) > 0 and float(a["dists"].abs().max()) > 0


def test_backward_gather_once_live_only_valid_rows_bitwise(frags, device):
    f = frags["64"]
    valid = f["valid"].to(device)
    with _Env(PR_BLEND_CHAIN=0):
        full = _run(f, device, "philox")
        a = _run(f, device, "philox", live_only=True)
    with _Env(PR_BLEND_CHAIN=2):
        b = _run(f, device, "philox", live_only=True)
    for k in ("dists", "zbuf", "bary"):
        assert bool(torch.isfinite(b[k][valid]).all()), k
        assert torch.equal(a[k][valid], b[k][valid]), k
        assert torch.equal(full[k][valid], b[k][valid]), k
    assert torch.equal(a["scalars"], b["scalars"])
    assert_close(b["vc"], a["vc"], name="d vertex colours")


@pytest.mark.parametrize("chain", [0, 2])
def test_backward_matches_oracle(chain, frags, oracle64, device):
    f = frags["64"]
    _, _, og = oracle64
    with _Env(PR_BLEND_CHAIN=chain):
        a = _run(f, device, "injected")
    assert_close(a["dists"], og["dists"], name="d dists")
    assert_close(a["zbuf"], og["zbuf"], name="d zbuf")
    assert_close(a["bary"], og["bary"], name="d bary")
    assert_close(a["vc"], og["vc"], name="d vertex colours")
    for i, k in enumerate(("sigma", "gamma", "alpha")):
        assert_close(a["scalars"][i], og[k], rtol=SCALAR_RTOL, name=k)
    # the crafted pixels' unperturbed argmax won nothing: B2 reads its colour, nobody writes a d bary
    for x in LONE_X:
        assert bool((a["bary"][0, ROW_LONE, x, 0] == 0).all())

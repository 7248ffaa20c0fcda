"""The blend kernels' rotated block order (PR_BLEND_ORDER=12: pr_blend.hip rotated_block) against the
linear order (PR_BLEND_ORDER=0) in one process.

Only which workgroup takes which pixel block changes: partials are indexed by pixel block and
Philox counters by physical pixel, so the image, d dists, d zbuf, d colours (d bary on the fused
vertex path) and d sigma / d gamma / d alpha are bitwise equal.  d vertex colours is a float-atomic
scatter whose summation order is that of the workgroups' arrival, different from run to run even
in one order: it compares at conftest.assert_close's 1e-5, as in tests/test_gpu_interleave.py.

Frames: the smallest that reach each branch of the permutation, with small blocks forced by
PR_BLEND_PB_FWD / _BWD -- more than one 256-block dealing cycle at 16 blocks per row, a row count
of blocks that is no power of two, a batch (the order restarts per image), blocks that tile the
image but not its rows and a partial last block (both fall back to linear).  Each runs with
Philox and injected noise, with the valid counts attached (empty-block shortcut, live-only
backward) and without, and with the fused scalar reduction on and off; pr_blend_geometry names
the order every case takes.  One frame is captured in a HIP graph and replayed twice.
"""
import contextlib
import os

import pytest
import torch

import pertrenderer_amd as pa
import pertrenderer_amd.blend as pb
from conftest import assert_close
from pertrenderer_amd import _native as nat
from pertrenderer_amd.blend import Noise
from pertrenderer_amd.renderer.rasterizer import attach_valid_counts

pytestmark = pytest.mark.gpu

LINEAR, ROTATED = "0", "12"
SR, SA = 4, 4
# name: (N, H, W, K), forced pixels per block (None: the default), order the rotated request takes
FRAMES = {
    "two_cycles": ((1, 24, 32, 3), 2, nat.BLEND_ORDER_ROTATED),   # 384 blocks, 16 per row
    "six_per_row": ((1, 50, 24, 3), 4, nat.BLEND_ORDER_ROTATED),  # 300 blocks, 6 per row
    "batch": ((3, 20, 32, 5), 2, nat.BLEND_ORDER_ROTATED),        # 320 blocks per image
    "not_rows": ((1, 6, 10, 4), 4, nat.BLEND_ORDER_LINEAR),       # 15 blocks tile the image, not its rows
    "partial": ((1, 5, 7, 4), None, nat.BLEND_ORDER_LINEAR),      # 35 pixels: a partial last block
}
ENV = ("PR_BLEND_ORDER", "PR_BLEND_PB_FWD", "PR_BLEND_PB_BWD")


@contextlib.contextmanager
def blend_env(order, PB, fused=True):
    old = {k: os.environ.get(k) for k in ENV}
    old_fused = pb._FUSED_FINALIZE
    new = {"PR_BLEND_ORDER": order, "PR_BLEND_PB_FWD": PB and str(PB), "PR_BLEND_PB_BWD": PB and str(PB)}
    try:
        for k, v in new.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        pb._FUSED_FINALIZE = fused
        yield
    finally:
        pb._FUSED_FINALIZE = old_fused
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _orders(shape, PB):
    """(forward, backward) order pr_blend_geometry reports under the current environment."""
    p = nat.PRBlendParams()
    p.N, p.H, p.W, p.K, p.Sr, p.Sa = shape + (SR, SA)
    out = []
    for bwd in (0, 1):
        g = nat.PRBlendGeometry()
        nat.check(nat.load().pr_blend_geometry(p, bwd, g), "pr_blend_geometry")
        assert PB is None or g.PB == PB
        assert not g.interleaved
        out.append(g.order)
    return tuple(out)


_CACHE = {}


def _frame(device, name):
    """Fragments with an empty band, empty pixels and full pixels (valid prefixes), colours, a mesh's
    worth of vertex colours / faces / bary, injected noise and an upstream gradient; made once."""
    if name in _CACHE:
        return _CACHE[name]
    N, H, W, K = FRAMES[name][0]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    cnt = torch.randint(0, K + 1, (N, H, W), generator=g)
    cnt[:, : H // 3] = 0
    cnt[:, H // 2, ::3] = K
    valid = torch.arange(K) < cnt[..., None]
    f = dict(
        p2f=torch.where(valid, torch.randint(0, 40, (N, H, W, K), generator=g), -1),
        dists=torch.where(valid, (torch.rand((N, H, W, K), generator=g) - 0.5) * 6e-3, -1.0),
        zbuf=torch.where(valid, (5.0 + 2.0 * torch.rand((N, H, W, K), generator=g)).sort(-1).values, -1.0),
        colors=torch.rand((N, H, W, K, 3), generator=g),
        bary=torch.where(valid[..., None], torch.rand((N, H, W, K, 3), generator=g), -1.0),
        vc=torch.rand((30, 3), generator=g), faces=torch.randint(0, 30, (40, 3), generator=g),
        nr=torch.randn((SR, N, H, W, K), generator=g), na=torch.randn((SA, N, H, W, K + 1), generator=g),
        gimg=torch.randn((N, H, W, 4), generator=g), cnt=cnt.to(torch.int32))
    _CACHE[name] = {k: v.to(device) for k, v in f.items()}
    return _CACHE[name]


def _noise(f, injected):
    return Noise.injected(f["nr"], f["na"]) if injected else Noise.philox(seed_r=11, seed_a=13)


def _run(device, f, injected, counts, vertex):
    p2f = f["p2f"].clone()  # a fresh tensor: the counts ride on it
    if counts:
        attach_valid_counts(p2f, f["cnt"])
    dists, zbuf = (f[k].clone().requires_grad_(True) for k in ("dists", "zbuf"))
    sig, gam, alp = (torch.tensor(v, device=device, requires_grad=True) for v in (1e-3, 1e-2, 1.2))
    kw = dict(background=(0.2, 0.4, 0.6), noise=_noise(f, injected), live_only=counts)
    if vertex:
        bary, vc = f["bary"].clone().requires_grad_(True), f["vc"].clone().requires_grad_(True)
        img = pa.blend.perturbed_blend_vertex(vc, f["faces"], p2f, bary, dists, zbuf, sig, gam, alp, SR, SA, **kw)
        extra, names = (bary, vc), ("d bary", "d vertex colours")
    else:
        colors = f["colors"].clone().requires_grad_(True)
        img = pa.perturbed_blend(colors, p2f, dists, zbuf, sig, gam, alp, SR, SA, **kw)
        extra, names = (colors,), ("d colours",)
    img.backward(f["gimg"])
    torch.cuda.synchronize()
    out = [img.detach(), dists.grad, zbuf.grad] + [t.grad for t in extra] + [sig.grad, gam.grad, alp.grad]
    if counts:  # live-only: the masked slots' gradients (d dists, d zbuf, d colours / d bary) are not written
        live = f["p2f"] >= 0
        for i in (1, 2, 3):
            out[i] = torch.where(live if out[i].dim() == 4 else live[..., None], out[i], torch.zeros_like(out[i]))
    return out, ("image", "d dists", "d zbuf") + names + ("d sigma", "d gamma", "d alpha")


def _compare(a, b, names):
    for x, y, n in zip(a, b, names):
        if n == "d vertex colours":
            assert_close(x, y, rtol=1e-5, name=n)
        else:
            assert torch.equal(x, y), n


@pytest.mark.parametrize("vertex", [False, True], ids=["texel", "vertex"])
@pytest.mark.parametrize("counts", [True, False], ids=["counts", "nocounts"])
@pytest.mark.parametrize("injected", [False, True], ids=["philox", "injected"])
@pytest.mark.parametrize("name", list(FRAMES))
def test_rotated_order_is_bitwise_linear(device, name, injected, counts, vertex):
    shape, PB, want = FRAMES[name]
    f = _frame(device, name)
    for fused in (True, False):
        with blend_env(LINEAR, PB, fused):
            assert _orders(shape, PB) == (nat.BLEND_ORDER_LINEAR,) * 2
            a, names = _run(device, f, injected, counts, vertex)
        with blend_env(ROTATED, PB, fused):
            assert _orders(shape, PB) == (want, want)
            b, _ = _run(device, f, injected, counts, vertex)
        assert torch.isfinite(a[0]).all() and int((a[1] != 0).sum()) > 0
        _compare(a, b, names)


def test_order_is_selected_per_kernel():
    shape, PB, _ = FRAMES["two_cycles"]
    lin, co, rot = nat.BLEND_ORDER_LINEAR, nat.BLEND_ORDER_CENTRE_OUT, nat.BLEND_ORDER_ROTATED
    for value, want in (("0", (lin, lin)), ("1", (co, lin)), ("2", (lin, co)), ("3", (co, co)), ("4", (rot, lin)),
                        ("8", (lin, rot)), ("12", (rot, rot)), ("6", (rot, co)), ("9", (co, rot)), ("15", (rot, rot))):
        with blend_env(value, PB):
            assert _orders(shape, PB) == want, value


def test_rotated_order_in_a_captured_graph(device):
    shape, PB, want = FRAMES["two_cycles"]
    f = _frame(device, "two_cycles")
    with blend_env(LINEAR, PB):
        ref, _ = _run(device, f, False, False, False)
    with blend_env(ROTATED, PB):
        assert _orders(shape, PB) == (want, want)
        dists, zbuf, colors = (f[k].clone().requires_grad_(True) for k in ("dists", "zbuf", "colors"))
        sig, gam, alp = (torch.tensor(v, device=device, requires_grad=True) for v in (1e-3, 1e-2, 1.2))
        leaves = (dists, zbuf, colors, sig, gam, alp)

        def step():
            img = pa.perturbed_blend(colors, f["p2f"], dists, zbuf, sig, gam, alp, SR, SA, background=(0.2, 0.4, 0.6),
                                     noise=_noise(f, False))
            img.backward(f["gimg"])
            return img
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        for t in leaves:
            t.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            img = step()
    for _ in range(2):  # replays need no environment: the order is in the captured launches
        for t in leaves:
            t.grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = [img.detach()] + [t.grad for t in leaves]
        for x, y in zip(got, ref):
            assert torch.equal(x, y)

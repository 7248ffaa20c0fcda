"""Native deterministic SoftRast + SoftAgg blend (PR_BLEND_SOFT, csrc/pr_softblend.hip) against the
CPU oracle (oracle/blend_oracle.py: the reference composition, bitwise-pinned by soft_blend.npz and,
on these inputs, by tests/test_softblend_cases_cpu.py) on the frames of tests/softblend_cases.py:

* plain: random fragments with |u| = |d / sigma| <= 4, K up to 150, z ties between slots 0 and 1,
  P = 1 on slot 0 of a tenth of the pixels, packed and scattered valid slots, with and without the
  rasterizer's valid-prefix counts;
* saturated: valid slots with P == 0 (log P = -inf: the inf / nan conventions of log_corrected and
  prod_corrected), one, two and three P == 1 slots per pixel on every arrangement of the 16 lanes
  (torch.prod's exclusive-product backward), all-masked and one-slot pixels, z ties between slots
  k, k + 5 and k + 16, at K = 1, 15, 16, 17, 63, 64 (lanes kernels) and 65, 70 (scalar kernels);
* clamped: the four regimes of clamp(min=eps) on zmax, planes that differ per image, alpha 0.5 / 1 / 1.3;
* large plain frames: more than 256 backward workgroups (the finalize kernel's strided loop) in both
  kernel families, and more pixels than the lanes kernels' 8192 workgroups x 16 (their grid-stride
  loop, with a partly dead last group).

The scalar kernels' own grid-stride loop needs more than 4096 x 256 = 1 048 576 pixels at K >= 65:
out of reach for a test of a few seconds, so it is not run.  Which branch each frame reaches is
asserted on the CPU (test_softblend_cases_cpu.py), from the coverage counts of softblend_cases.py.
The golden-vector check through the public classes is tests/test_public_api_parity.py."""
import numpy as np
import pytest
import torch

import softblend_cases as sc
from conftest import assert_close
from oracle import blend_oracle as bo
from pertrenderer_amd import soft_blend
from pertrenderer_amd.renderer.rasterizer import attach_valid_counts

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape,packed,counts", [((1, 16, 20, 50), True, True), ((2, 9, 7, 12), False, False),
                                                 ((1, 6, 5, 150), True, False), ((1, 8, 8, 3), True, True)])
def test_soft_blend_matches_oracle(shape, packed, counts, device):
    N, H, W, K = shape
    sigma, gamma, alpha, eps, bg = 1e-3, 1e-2, 1.3, 1e-10, (0.1, 0.2, 0.3)
    p2f, d, z, cols, gimg, valid = sc.plain(shape, sum(shape), packed, sigma)[:6]
    zn, zf = torch.ones((N, 1, 1, 1)), torch.full((N, 1, 1, 1), 100.0)
    oimg, og = bo.soft_blend_forward_backward(p2f, d, z, cols, sigma, gamma, alpha, eps, bg, zn, zf, gimg)
    P = p2f.to(device)
    if counts:
        attach_valid_counts(P, valid.sum(-1).to(torch.int32).to(device))
    dd, zz, cc = (t.to(device).requires_grad_(True) for t in (d, z, cols))
    s, gm, al = (torch.tensor(v, requires_grad=True) for v in (sigma, gamma, alpha))
    img = soft_blend(cc, P, dd, zz, s, gm, al, eps=eps, background=bg, znear=zn.to(device), zfar=zf.to(device))
    (img * gimg.to(device)).sum().backward()
    for k, t in (("image", img), ("dists", dd.grad), ("zbuf", zz.grad), ("colors", cc.grad), ("sigma", s.grad),
                 ("gamma", gm.grad), ("alpha", al.grad)):
        assert torch.isfinite(t).all(), f"{k} is not finite"
    assert_close(img, oimg, name="image")
    for k, t in (("dists", dd), ("colors", cc)):
        assert_close(t.grad, og[k], name=k)
    # d zbuf of a pixel's nearest slot carries d zmax = -(sum of all K+1 logit gradients), which
    # is exactly 0 in real arithmetic (a softmax is shift-invariant): both sides hold only its
    # fp32 rounding residue (~K ulp of the largest term), so that slot's bar is 1e-4 of the max
    assert_close(zz.grad, og["zbuf"], atol_rel=1e-4, name="zbuf")
    # the smoothing scalars are sums over all N*H*W*K slots of signed terms, reduced by the kernel's
    # workgroup tree and by the oracle's torch.sum: fp32 summation order alone moves them by ~1e-5
    # relative on the larger frames (measured 1.4e-5), so their bar is 5e-5
    for k, t in (("sigma", s), ("gamma", gm), ("alpha", al)):
        assert t.grad.device.type == "cpu"
        assert_close(t.grad, og[k], rtol=5e-5, name=k)


def _run(c, counts, device):
    """The native forward and backward on a softblend_cases.Case -> (image, gradients) on the CPU."""
    p = c.params
    P = c.p2f.to(device)
    if counts:
        attach_valid_counts(P, c.valid.sum(-1).to(torch.int32).to(device))
    dd, zz, cc = (t.to(device).requires_grad_(True) for t in (c.dists, c.zbuf, c.colors))
    s, gm, al = (torch.tensor(p[k], requires_grad=True) for k in ("sigma", "gamma", "alpha"))
    img = soft_blend(cc, P, dd, zz, s, gm, al, eps=p["eps"], background=p["background"], znear=c.znear.to(device),
                     zfar=c.zfar.to(device))
    (img * c.grad_image.to(device)).sum().backward()
    for k, t in (("sigma", s), ("gamma", gm), ("alpha", al)):
        assert t.grad.device.type == "cpu", k
    return img.detach().cpu(), dict(dists=dd.grad.cpu(), zbuf=zz.grad.cpu(), colors=cc.grad.cpu(), sigma=s.grad,
                                    gamma=gm.grad, alpha=al.grad)


def _compare(img, g, oimg, og):
    """Finite first (assert_close lets a NaN through: NaN > tol is false), then the bars of
    test_soft_blend_matches_oracle, for the reasons written there.  The scalars' 5e-5 holds on every
    frame, the large ones included (measured there: 7.3e-6 at worst, d gamma of the 260-workgroup
    frame; over the whole battery 3.2e-5, d alpha of the packed (1,4,5,70) frame, whose terms cancel
    to a tenth: rho = 11); what it needs is a sum that does not cancel altogether, which
    test_softblend_cases_cpu.py asserts of every frame (softblend_cases.conditioning)."""
    assert torch.isfinite(img).all(), "image is not finite"
    for k, t in g.items():
        assert torch.isfinite(t).all(), f"d {k} is not finite"
    assert_close(img, oimg, name="image")
    for k in ("dists", "zbuf", "colors"):
        assert_close(g[k], og[k], atol_rel=1e-4 if k == "zbuf" else 1e-6, name=k)
    for k in ("sigma", "gamma", "alpha"):
        print(f"d {k}: kernel {g[k].item():.9g} oracle {og[k].item():.9g} "
              f"rel {abs(g[k].item() - og[k].item()) / max(abs(og[k].item()), 1e-30):.3g}")
    for k in ("sigma", "gamma", "alpha"):
        assert_close(g[k], og[k], rtol=5e-5, name=k)


# lanes kernels: packed with counts, packed by pix_to_face, scattered; scalar kernels: packed with
# counts and scattered (soft_pixel's search for the first masked slot)
SAT_RUNS = ([(("saturated", s, True), True) for s in sc.SAT_LANES + sc.SAT_SCALAR]
            + [(("saturated", s, True), False) for s in sc.SAT_LANES]
            + [(("saturated", s, False), False) for s in sc.SAT_LANES + sc.SAT_SCALAR])


@pytest.mark.parametrize("entry,counts", SAT_RUNS, ids=[sc.case_id(e) + ("-counts" if n else "") for e, n in SAT_RUNS])
def test_saturated(entry, counts, device):
    """P == 0 and P == 1 slots at every K boundary of both kernel families."""
    c = sc.build(*entry)
    img, g = _run(c, counts, device)
    _compare(img, g, *sc.oracle(*entry))
    sc.check_hand_derived(c, img, g)


@pytest.mark.parametrize("entry", sc.CLAMPED, ids=sc.case_id)
def test_clamped(entry, device):
    """clamp(min=eps) on zmax: no d zmax below eps, a masked slot's z_inv = 0 as the maximum, and
    the first-index rule between a masked slot and a valid slot at zbuf == zfar (eps = 0).  The
    frame without a masked slot runs with counts (every count is K)."""
    c = sc.build(*entry)
    img, g = _run(c, bool(c.valid.all()), device)
    _compare(img, g, *sc.oracle(*entry))
    sc.check_hand_derived(c, img, g)


@pytest.mark.parametrize("entry", sc.LARGE, ids=sc.case_id)
def test_large_frames(entry, device):
    """More than 256 backward workgroups (260 lanes, 257 scalar) and the lanes kernels' second
    grid-stride trip: every per-slot gradient and the workgroup-reduced scalars."""
    c = sc.build(*entry)
    img, g = _run(c, entry[2][0], device)
    _compare(img, g, *sc.oracle(*entry))
    sc.check_hand_derived(c, img, g)


def test_soft_blend_device_scalars_and_capture(device):
    """Device smoothing leaves are read by pointer: the step captures into a HIP graph and
    replays to the eager result."""
    p2f, d, z, cols, gimg, _ = sc.plain((1, 12, 12, 20), 3, True, 1e-3)[:6]
    P, cc, gi, zz = p2f.to(device), cols.to(device), gimg.to(device), z.to(device)
    s, gm, al = (torch.tensor(v, device=device, requires_grad=True) for v in (1e-3, 1e-2, 1.0))
    de = d.to(device).requires_grad_(True)
    eager = soft_blend(cc, P, de, zz, s, gm, al, background=(0, 0, 0))
    (eager * gi).sum().backward()
    ref_img, ref_g = eager.detach().clone(), de.grad.clone()
    del eager
    # a fresh leaf: its gradient accumulator must be created on the capture's side of the stream
    dd = d.to(device).requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        (soft_blend(cc, P, dd, zz, s, gm, al, background=(0, 0, 0)) * gi).sum().backward()
    torch.cuda.current_stream().wait_stream(side)
    dd.grad.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        img = soft_blend(cc, P, dd, zz, s, gm, al, background=(0, 0, 0))
        (img * gi).sum().backward()
    dd.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(img, ref_img)
    torch.testing.assert_close(dd.grad, ref_g, rtol=0, atol=0)

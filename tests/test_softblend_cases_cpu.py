"""The soft-blend battery of tests/softblend_cases.py on the CPU, for every frame that
tests/test_gpu_softblend.py runs: the builders reach the branches they claim (coverage counts),
the oracle (oracle/blend_oracle.py) stays finite on them and meets the values that follow from the
formulas alone, and it agrees with the product's own torch classes (SoftRast / SoftAgg through
smooth_rgb_blend, which test_public_api_parity.py pins bitwise to the reference's soft_blend.npz):
this pins the oracle on the saturated and clamped inputs, which that golden file does not hold."""
import pytest
import torch

import pertrenderer_amd as pa
import softblend_cases as sc
from pertrenderer_amd.random_rasterizer import BlendParams, smooth_rgb_blend
from pertrenderer_amd.renderer.rasterizer import Fragments

GRADS = ("dists", "zbuf", "colors", "sigma", "gamma", "alpha")


@pytest.mark.parametrize("entry", sc.BATTERY, ids=sc.case_id)
def test_oracle_is_finite(entry):
    img, g = sc.oracle(*entry)
    assert torch.isfinite(img).all(), "image"
    for k in GRADS:
        assert torch.isfinite(g[k]).all(), k


@pytest.mark.parametrize("entry", sc.BATTERY, ids=sc.case_id)
def test_no_slot_in_a_forbidden_range(entry):
    c = sc.build(*entry)
    cov = sc.coverage(c)
    assert cov["forbidden"] == 0, cov
    # every valid slot is ordinary (|u| <= 8) or saturated (|u| >= 200)
    assert cov["ordinary_slots"] + cov["saturated_slots"] == cov["slots"], cov


@pytest.mark.parametrize("entry", sc.SATURATED, ids=sc.case_id)
def test_saturated_coverage(entry):
    _, shape, packed = entry
    c = sc.build(*entry)
    cov = sc.coverage(c)
    for key in sc.required_saturated(shape[-1]):
        assert cov[key] > 0, (key, cov)
    assert cov["p0_any"] >= 0.2 * cov["pixels"], cov
    if packed:  # a prefix, as attach_valid_counts needs
        K = shape[-1]
        assert torch.equal(c.valid, torch.arange(K).expand(c.valid.shape) < c.valid.sum(-1, keepdim=True))
    assert (sc.bwd_blocks(shape)[1] == sc.LANES_PIX) == (shape in sc.SAT_LANES)  # the kernel family by K


@pytest.mark.parametrize("entry", sc.BATTERY, ids=sc.case_id)
def test_scalar_gradients_are_well_conditioned(entry):
    """The relative bar on d sigma, d gamma, d alpha is a bar on the kernel only where the sum does
    not cancel (softblend_cases.conditioning)."""
    for k, rho in sc.conditioning(*entry).items():
        assert rho <= sc.RHO_MAX, (k, rho)


def test_k_boundaries():
    """One or two slots per lane (15 / 16 / 17), the last lane's last slot (63 / 64), one slot, and
    the first K of the scalar kernels."""
    assert {s[-1] for s in sc.SAT_LANES} == {1, 15, 16, 17, 63, 64}
    assert sc.SAT_SCALAR[0][-1] == 65 and all(s[-1] > 64 for s in sc.SAT_SCALAR)
    assert {s[-1] > 64 for s in sc.CLAMP_SHAPES} == {False, True}


@pytest.mark.parametrize("entry", sc.CLAMPED, ids=sc.case_id)
def test_clamped_coverage(entry):
    _, shape, case = entry
    c = sc.build(*entry)
    cov = sc.coverage(c)
    for key in sc.REQUIRED_CLAMPED[case]:
        assert cov[key] > 0, (key, cov)
    if case in ("beyond", "masked_wins", "big_eps"):  # zmax_grad == false at every pixel
        assert cov["zmax_off"] == cov["pixels"] and cov["zmax_on"] == 0, cov
    if case == "beyond":
        assert bool(c.valid.all()) and cov["all_behind"] == cov["pixels"], cov
        assert bool((c.zbuf > c.zfar).all()) and bool((c.zbuf <= 50 * c.zfar).all())
    if case == "masked_wins":
        assert cov["masked_max"] + cov["all_masked"] == cov["pixels"] - int(c.valid.all(-1).sum()), cov
    if case == "eps0":
        assert c.params["eps"] == 0.0 and cov["zmax_on"] > 0, cov
    assert c.znear[0].item() != c.znear[1].item() and c.zfar[0].item() != c.zfar[1].item()
    assert {sc.build("clamped", shape, k).params["alpha"] for k in sc.CLAMP_CASES} == {0.5, 1.0, 1.3}


def test_large_frames_reach_the_strided_loops():
    """nblk > 256 enters soft_finalize_kernel's strided loop in both kernel families; more pixels
    than 8192 workgroups x 16 enter the lanes kernels' second grid-stride trip, whose last group of
    16 is partly dead."""
    nb, per = sc.bwd_blocks(sc.STRIDE_LANES)
    assert per == sc.LANES_PIX and sc.THREADS < nb == 260 < sc.LANES_MAX_BLOCKS
    nb, per = sc.bwd_blocks(sc.STRIDE_SCALAR)
    assert per == sc.THREADS and nb == 257 > sc.THREADS
    N, H, W, K = sc.GRID_LANES
    nb, per = sc.bwd_blocks(sc.GRID_LANES)
    assert per == sc.LANES_PIX and nb == sc.LANES_MAX_BLOCKS and N * H * W > nb * per and (N * H * W) % per != 0
    cov = sc.coverage(sc.build(*sc.PLAIN_STRIDE_LANES))
    assert cov["p1_with_p0"] >= (sc.STRIDE_LANES[1] * sc.STRIDE_LANES[2] + 96) // 97, cov


@pytest.mark.parametrize("entry", sc.SATURATED + sc.CLAMPED + (sc.PLAIN_STRIDE_LANES,), ids=sc.case_id)
def test_hand_derived_values(entry):
    c = sc.build(*entry)
    img, g = sc.oracle(*entry)
    dark, multi = sc.check_hand_derived(c, img, g)
    if entry[0] == "saturated":
        assert dark > 0 and (multi > 0 or entry[1][-1] < 2)


@pytest.mark.parametrize("entry", sc.BATTERY, ids=sc.case_id)
def test_oracle_matches_product_classes(entry):
    """The oracle restates the graph that smooth_rgb_blend builds from SoftRast and SoftAgg, op for
    op, so on the CPU the two agree bit for bit: image and all six gradients."""
    c = sc.build(*entry)
    p = c.params
    d, z, col = (t.clone().requires_grad_(True) for t in (c.dists, c.zbuf, c.colors))
    rast = pa.SoftRast(sigma=p["sigma"])
    agg = pa.SoftAgg(gamma=p["gamma"], alpha=p["alpha"], eps=p["eps"])
    bary = torch.zeros(tuple(c.p2f.shape) + (3,))  # not read by the blend
    bp = BlendParams(p["sigma"], p["gamma"], p["background"])
    img = smooth_rgb_blend(col, Fragments(c.p2f, z, bary, d), rast, agg, bp, znear=c.znear, zfar=c.zfar)
    (img * c.grad_image).sum().backward()
    oimg, og = sc.oracle(*entry)
    assert torch.equal(img.detach(), oimg), "image"
    got = dict(dists=d.grad, zbuf=z.grad, colors=col.grad, sigma=rast.sigma.grad, gamma=agg.gamma.grad,
               alpha=agg.alpha.grad)
    for k in GRADS:
        assert torch.equal(got[k], og[k]), k

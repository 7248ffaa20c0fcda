"""The point-cloud renderer on the CPU (the torch composition of renderer/points.py): against the
float64 restatement of points_cases.py on every scene (indices exact, zbuf bitwise, dists and images
at conftest.assert_close's defaults; gradients within the 2e-5 the cases module asserts), gradcheck
in float64, known answers, the shim's names and the Pointclouds feature views.  No GPU."""
import pytest
import torch

import points_cases as C
from conftest import assert_close
from pertrenderer_amd.renderer import FoVPerspectiveCameras, Pointclouds
from pertrenderer_amd.renderer import points as PT


@pytest.mark.parametrize("name", list(C.SCENES))
def test_composition_matches_float64(name):
    ref = C.references(name)  # asserts the float32 composition's values and gradient errors
    s = C.scene(name)
    assert max(ref["err32"].values()) <= 2e-5
    # the float64 composition picks the same fragments and gives the restatement's numbers
    rad = s["radius"].double() if torch.is_tensor(s["radius"]) else s["radius"]
    idx, zbuf, dists = PT.rasterize_points(Pointclouds([c.double() for c in s["clouds"]]), (s["H"], s["W"]), rad, s["K"])
    assert idx.dtype == torch.int64 and zbuf.dtype == dists.dtype == torch.float64
    assert tuple(idx.shape) == (len(s["clouds"]), s["H"], s["W"], s["K"])
    assert torch.equal(idx, ref["idx"]) and torch.equal(zbuf, ref["zbuf"])
    assert_close(dists, ref["dists"], name="float64 composition dists")
    assert ((idx < 0) == (zbuf == -1)).all() and ((idx < 0) == (dists == -1)).all()


def test_planted_cases_behave():
    s, ref = C.scene("c70_k8"), C.references("c70_k8")
    idx = ref["idx"]
    for p in C.PLANT_BEHIND + C.PLANT_OUTSIDE + (C.PLANT_NAN,):
        assert not (idx == p).any(), p
    # the duplicated point: wherever the second copy appears the first sits in the slot before it
    first, second = C.PLANT_DUP
    pos = (idx == second).nonzero()
    assert len(pos) and (pos[:, 3] > 0).all()
    assert (idx[pos[:, 0], pos[:, 1], pos[:, 2], pos[:, 3] - 1] == first).all()
    # two points of equal z: where both are kept the lower index comes first
    lo, hi = C.PLANT_EQUAL_Z
    both = ((idx == lo).any(-1) & (idx == hi).any(-1)).nonzero()
    assert len(both)
    for n, r, c in both.tolist():
        row = idx[n, r, c].tolist()
        assert row.index(lo) + 1 == row.index(hi)
    # the point on a pixel centre: d2 exactly 0 there
    r, c = C.CENTRE_PIXEL
    k = idx[0, r, c].tolist().index(C.PLANT_CENTRE)
    assert ref["dists"][0, r, c, k] == 0 and ref["alphas"][0, r, c, k] == 1
    # slots are a sorted prefix
    z = torch.where(idx >= 0, ref["zbuf"], torch.full_like(ref["zbuf"], float("inf")))
    assert (z[..., 1:] >= z[..., :-1]).all()
    assert s["K"] == 8


def test_one_point_on_a_pixel_centre():
    s = C.scene("one_k1")
    idx, zbuf, dists = PT.rasterize_points(Pointclouds(s["clouds"]), 32, 0.1, 1)
    r, c = C.CENTRE_PIXEL
    assert idx[0, r, c, 0] == 0 and dists[0, r, c, 0] == 0 and zbuf[0, r, c, 0] == s["clouds"][0][0, 2]
    # pixel pitch 2/32 = 0.0625 < r = 0.1 < 0.125: the centre pixel, its 4 neighbours and (0.0884 < 0.1) its 4 diagonals
    assert (idx >= 0).sum() == 9
    assert_close(dists[0, r, c + 1, 0], (2.0 / 32) ** 2)
    # image_size (H, W), bin knobs accepted and without effect
    a = PT.rasterize_points(Pointclouds(s["clouds"]), (32, 32), 0.1, 1, bin_size=0, max_points_per_bin=5)
    assert all(torch.equal(x, y) for x, y in zip(a, (idx, zbuf, dists)))


def test_two_slot_alpha_chain_norm_clamp_and_weighted_by_hand():
    idx = torch.tensor([[[[0, -1, 1]]]])  # (N,H,W,K) = (1,1,1,3): an empty slot in the middle is skipped, not a stop
    alphas = torch.tensor([[[[0.25, 0.9, 0.5]]]], requires_grad=True)
    feats = torch.tensor([[1.0, 2.0], [10.0, 20.0]], requires_grad=True)  # (P,C)
    out = PT._composite_rows(idx, alphas, feats, PT._MODES["alpha"])
    assert_close(out, [[[[0.25 * 1 + 0.75 * 0.5 * 10, 0.25 * 2 + 0.75 * 0.5 * 20]]]])
    ga, gf = torch.autograd.grad(out[..., 0].sum(), (alphas, feats))
    assert_close(ga, [[[[1.0 - 0.5 * 10, 0.0, 0.75 * 10]]]])
    assert_close(gf, [[0.25, 0.0], [0.375, 0.0]])
    # a_0 = 1: the chain's factor is 0, the derivative stays finite and exact (no division by 1 - a)
    one = torch.tensor([[[[1.0, 0.9, 0.5]]]], requires_grad=True)
    (g1,) = torch.autograd.grad(PT._composite_rows(idx, one, feats.detach(), PT._MODES["alpha"])[..., 0].sum(), one)
    assert_close(g1, [[[[1.0 - 0.5 * 10, 0.0, 0.0]]]])
    out = PT._composite_rows(idx, alphas, feats, PT._MODES["weighted"])
    assert_close(out, [[[[0.25 + 5.0, 0.5 + 10.0]]]])
    out = PT._composite_rows(idx, alphas, feats, PT._MODES["norm"])
    assert_close(out, [[[[5.25 / 0.75, 10.5 / 0.75]]]])
    tiny = torch.tensor([[[[2e-5, 0.9, 3e-5]]]])  # sum 5e-5 < 1e-4: the clamp divides
    out = PT._composite_rows(idx, tiny, feats, PT._MODES["norm"])
    assert_close(out, [[[[(2e-5 * 1 + 3e-5 * 10) / 1e-4, (2e-5 * 2 + 3e-5 * 20) / 1e-4]]]])
    # the public functions take PyTorch3D's layouts
    pub = PT.alpha_composite(idx.permute(0, 3, 1, 2), alphas.permute(0, 3, 1, 2), feats.t())
    assert tuple(pub.shape) == (1, 2, 1, 1) and torch.equal(pub[0, :, 0, 0], PT._composite_rows(idx, alphas, feats, 0)[0, 0, 0])
    assert tuple(PT.norm_weighted_sum(idx.permute(0, 3, 1, 2), alphas.permute(0, 3, 1, 2), feats.t()).shape) == (1, 2, 1, 1)
    assert tuple(PT.weighted_sum(idx.permute(0, 3, 1, 2), alphas.permute(0, 3, 1, 2), feats.t()).shape) == (1, 2, 1, 1)


def test_background_fills_the_pixels_whose_first_slot_is_empty():
    idx = torch.tensor([[[[0, -1], [-1, 0]]]])  # (1,1,2,2): pixel 1 has an empty slot 0
    alphas = torch.full((1, 1, 2, 2), 0.5)
    feats = torch.tensor([[1.0, 1.0, 1.0]])
    for cls in (PT.AlphaCompositor, PT.NormWeightedCompositor):
        plain = cls()(idx.permute(0, 3, 1, 2), alphas.permute(0, 3, 1, 2), feats.t())
        out = cls(background_color=(0.1, 0.2, 0.3))(idx.permute(0, 3, 1, 2), alphas.permute(0, 3, 1, 2), feats.t())
        assert tuple(out.shape) == (1, 3, 1, 2)
        assert torch.equal(out[0, :, 0, 0], plain[0, :, 0, 0])
        assert_close(out[0, :, 0, 1], [0.1, 0.2, 0.3])
        assert plain[0, :, 0, 1].abs().sum() > 0  # the skipped slot did not stop the second one


def test_gradcheck_float64():
    g = torch.Generator().manual_seed(4)  # generic points: no exact ties, whose order a perturbation would flip
    pts = torch.rand((20, 3), generator=g, dtype=torch.float64) * torch.tensor([2.2, 2.2, 2.0]) - torch.tensor([1.1, 1.1, -0.5])
    pts[3, 2] = -0.5
    pts.requires_grad_(True)

    def frag(p):
        _, zbuf, dists = PT.rasterize_points(Pointclouds([p]), (6, 9), 0.35, 4)
        return zbuf, dists
    assert torch.autograd.gradcheck(frag, (pts,), eps=1e-7, atol=1e-6)
    idx = PT.rasterize_points(Pointclouds([pts.detach()]), (6, 9), 0.35, 4)[0]
    assert (idx >= 0).any() and (idx < 0).any()
    alphas = torch.rand(idx.shape, generator=g, dtype=torch.float64).requires_grad_(True)
    feats = torch.rand((pts.shape[0], 3), generator=g, dtype=torch.float64).requires_grad_(True)
    for mode in C.MODES:
        assert torch.autograd.gradcheck(lambda a, f: PT._composite_rows(idx, a, f, PT._MODES[mode]), (alphas, feats)), mode


def test_renderer_on_the_cpu_reaches_points_features_and_camera():
    s = C.scene("batch2_k8")
    # (world points in front of the camera; the NaN point is made finite: it would reach T through the transform)
    pts = [(torch.nan_to_num(c) * torch.tensor([0.5, 0.5, 0.1]) + torch.tensor([0, 0, 2.0])).requires_grad_(True) for c in s["clouds"]]
    feats = [f.clone().requires_grad_(True) for f in s["features"]]
    # the camera at the origin: the zero rows that pad the shorter cloud would lie on the camera plane and
    # put 0 * inf = NaN into T's gradient; clouds of unequal sizes are projected cloud by cloud instead
    T = torch.zeros((1, 3), requires_grad=True)
    cams = FoVPerspectiveCameras(T=T)
    rs = PT.PointsRasterizationSettings(image_size=(12, 20), radius=0.1, points_per_pixel=4)
    renderer = PT.PointsRenderer(PT.PointsRasterizer(cameras=cams, raster_settings=rs), PT.AlphaCompositor(background_color=(0, 0, 1)))
    img = renderer(Pointclouds(pts, features=feats))
    assert tuple(img.shape) == (2, 12, 20, 3)
    frags = renderer.rasterizer(Pointclouds(pts, features=feats))
    assert isinstance(frags, PT.PointFragments) and tuple(frags.idx.shape) == (2, 12, 20, 4)
    empty = frags.idx[..., 0] < 0
    assert empty.any() and (~empty).any()
    assert torch.equal(img[empty], torch.tensor([0.0, 0.0, 1.0]).expand(int(empty.sum()), 3))
    # the layout-permuting public route gives the same image
    w = 1 - frags.dists / (0.1 * 0.1)
    pub = PT.alpha_composite(frags.idx.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), torch.cat(feats).t()).permute(0, 2, 3, 1)
    assert torch.equal(pub[~empty], img[~empty])
    grads = torch.autograd.grad((img ** 2).sum(), pts + feats + [T])
    assert all(torch.isfinite(g).all() and g.abs().sum() > 0 for g in grads)
    with pytest.raises(ValueError):
        PT.PointsRasterizer()(Pointclouds(pts))
    with pytest.raises(ValueError):
        renderer(Pointclouds(pts))  # no features
    # cameras from kwargs
    assert torch.equal(PT.PointsRasterizer(raster_settings=rs)(Pointclouds(pts), cameras=cams).idx, frags.idx)


def test_arguments_are_checked():
    pc = Pointclouds([torch.rand((5, 3))])
    for bad in (dict(points_per_pixel=0), dict(image_size=0), dict(image_size=(4, 5, 6)), dict(radius=torch.rand(4))):
        with pytest.raises(ValueError):
            PT.rasterize_points(pc, **{**dict(image_size=8), **bad})
    with pytest.raises(ValueError):
        PT.rasterize_points(torch.rand((1, 5, 3)))
    idx, zbuf, dists = PT.rasterize_points(Pointclouds([torch.zeros((0, 3))]), 4, 0.1, 2)
    assert (idx == -1).all() and (zbuf == -1).all() and (dists == -1).all()


def test_shim_imports_resolve():
    from pytorch3d.renderer import (AlphaCompositor, NormWeightedCompositor, PointsRasterizationSettings,  # noqa: F401
                                    PointsRasterizer, PointsRenderer, alpha_composite, norm_weighted_sum,
                                    rasterize_points, weighted_sum)
    import pertrenderer_amd.renderer as R
    for n in ("AlphaCompositor", "NormWeightedCompositor", "PointsRasterizationSettings", "PointsRasterizer",
              "PointsRenderer", "rasterize_points", "alpha_composite", "norm_weighted_sum", "weighted_sum"):
        assert n in R.__all__ and getattr(R, n) is getattr(PT, n)
    assert PointsRenderer is PT.PointsRenderer
    rs = PointsRasterizationSettings()
    assert (rs.image_size, rs.radius, rs.points_per_pixel, rs.bin_size, rs.max_points_per_bin) == (256, 0.01, 8, None, None)


def test_pointclouds_feature_views():
    a, b = torch.rand((4, 3)), torch.rand((2, 3))
    fa, fb = torch.rand((4, 5)), torch.rand((2, 5))
    pc = Pointclouds([a, b], features=[fa, fb])
    assert pc.features_list()[1] is fb and torch.equal(pc.features_packed(), torch.cat([fa, fb]))
    pad = pc.features_padded()
    assert tuple(pad.shape) == (2, 4, 5) and torch.equal(pad[1, :2], fb) and not pad[1, 2:].any()
    assert Pointclouds([a, b]).features_packed() is None and Pointclouds([a, b]).features_padded() is None
    first = pc.cloud_to_packed_first_idx()
    new = pc.update_padded(pc.points_padded() + 1.0)
    assert torch.equal(new.points_packed(), torch.cat([a, b]) + 1.0) and new.features_list() is pc.features_list()
    assert new.cloud_to_packed_first_idx() is first and new.npoints == [4, 2]
    # padded form
    P, F = torch.rand((2, 3, 3)), torch.rand((2, 3, 4))
    pp = Pointclouds(P, features=F)
    assert torch.equal(pp.features_packed(), F.reshape(-1, 4)) and pp.features_padded() is F
    q = pp.update_padded(P * 2)
    assert torch.equal(q.points_packed(), (P * 2).reshape(-1, 3)) and q.features_padded() is F
    for bad in ([fa], [fa, torch.rand((3, 5))], [fa, torch.rand((2, 4))], torch.rand((2, 4))):
        with pytest.raises(ValueError):
            Pointclouds([a, b], features=bad)
    with pytest.raises(ValueError):
        pc.update_padded(torch.rand((2, 5, 3)))


def test_renderer_with_per_point_radii_weighs_every_slot_by_its_own_radius():
    s, ref = C.scene("per_point_k8"), C.references("per_point_k8")
    rs = PT.PointsRasterizationSettings(image_size=(s["H"], s["W"]), radius=s["radius"], points_per_pixel=s["K"])

    class Identity:  # the scene's points are NDC already
        def get_world_to_view_transform(self, **kwargs):
            return self

        get_projection_transform = get_world_to_view_transform

        def transform_points(self, p):
            return p

    pts = [torch.nan_to_num(c, nan=5.0) for c in s["clouds"]]  # (the NaN point moved out of the image: same fragments)
    img = PT.PointsRenderer(PT.PointsRasterizer(Identity(), rs), PT.NormWeightedCompositor())(Pointclouds(pts, features=s["features"]))
    assert_close(img, ref["image_norm"], name="image")  # ref's alphas are 1 - d2 / r_p^2 with the slot's own radius


def test_a_background_given_for_one_call_leaves_the_module_alone():
    idx = torch.tensor([[[[-1]]]])
    alphas, feats = torch.ones((1, 1, 1, 1)), torch.ones((1, 3))
    comp = PT.AlphaCompositor(background_color=(0.1, 0.2, 0.3))
    assert_close(comp._rows(idx, alphas, feats)[0, 0, 0], [0.1, 0.2, 0.3])
    # other keywords (PointsRenderer forwards the rasterizer's) are ignored
    assert_close(comp._rows(idx, alphas, feats, background_color=(0.9, 0.8, 0.7), cameras=None)[0, 0, 0], [0.9, 0.8, 0.7])
    assert comp.background_color == (0.1, 0.2, 0.3)
    assert_close(comp._rows(idx, alphas, feats)[0, 0, 0], [0.1, 0.2, 0.3])
    plain = PT.NormWeightedCompositor()
    assert_close(plain._rows(idx, alphas, feats, background_color=(0.9, 0.8, 0.7))[0, 0, 0], [0.9, 0.8, 0.7])
    assert plain.background_color is None and not plain._rows(idx, alphas, feats).any()


def test_the_cached_sort_belongs_to_one_version_of_idx():
    idx = torch.tensor([[[[0, 1, -1]]]])
    csr = PT._csr_of(idx, 2)
    assert PT._csr_of(idx, 2) is csr and PT._csr_of(idx, 3) is not csr
    csr = PT._csr_of(idx, 2)
    start, entries = csr.get(idx)
    assert start.tolist() == [0, 1, 2] and entries.tolist()[:2] == [0, 1]
    idx[0, 0, 0, 2] = 1  # an in-place edit: the sort above is stale
    fresh = PT._csr_of(idx, 2)
    assert fresh is not csr and fresh.get(idx)[0].tolist() == [0, 1, 3]

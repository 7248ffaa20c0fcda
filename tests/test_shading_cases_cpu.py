"""The shading cases (shading_cases.py) pinned on the CPU, before any kernel is judged by them: the
float64 reference against the library's torch composition and against a hand evaluation in Python
floats, the conditioning of the cases (torch's float32 composition sits well inside the GPU tests'
bars), and the builder's conditions on every case test_gpu_shading_cases.py runs."""
import math

import pytest
import torch

import shading_cases as sc
from pertrenderer_amd.renderer import shading as sh

F32, F64 = torch.float32, torch.float64

# every texture and light kind at N = 3 (per-image shininess), N = 1, and N == H == 3: an (N,) shininess
# reshaped to (N,1,1) broadcast against (N,H,W,K) along H without an error (the _bc regression)
BC_REGRESSION = sc.Spec(3, 3, 5, 2, "given", "point")
COMPOSITION = list(sc.FULL_CROSS) + [sc.Spec(1, 8, 8, 12, "uv", "point"), sc.Spec(1, 8, 8, 12, "vertex", "point"),
                                     sc.Spec(1, 5, 7, 5, "given", "directional"), BC_REGRESSION] + list(sc.DEGENERATE)


def _library_composition(spec, dtype):
    """shading.phong_shading_reference on the case's CPU Meshes / Fragments in `dtype`, the texels
    from the same-dtype torch lookup: Ref of the colours and the gradients for the case's cotangent."""
    c = sc.build(spec)
    meshes, frag, lights, cams, mats, leaves, _ = sc.scene(c, "cpu", dtype, "plain")
    if dtype == F64:  # the ambient row the kernel is given is the float32 product of the two colours
        mats.ambient_color, lights.ambient_color = c.ambient.to(F64), torch.ones((1, 3), dtype=F64)
    z = sc.composition(c, leaves["verts"], leaves["bary"], leaves["tex"], leaves["light"], leaves["T"])
    out = sh.phong_shading_reference(meshes, frag, lights, cams, mats, z.texels)
    return sc.grads_of(out, leaves, c.G)


@pytest.mark.parametrize("spec", COMPOSITION, ids=sc.spec_id)
def test_reference_is_the_library_composition_in_float64(spec):
    c = sc.build(spec)
    assert len(set(c.shininess.tolist())) == min(spec.N, 4) and c.shininess.shape == (spec.N,)
    ref, lib = sc.shade_ref64(spec), _library_composition(spec, F64)
    for name, a, b in zip(sc.Ref._fields, lib, ref):
        assert a.dtype == F64 and a.shape == b.shape
        assert sc.ratio(a, b, 1e-12) <= 1.0, name


def test_per_image_shininess_broadcasts_over_images():
    """N == H: with the shininess along H instead of N the colours of images 1 and 2 change."""
    c = sc.build(BC_REGRESSION)
    assert c.spec.N == c.spec.H == 3 and len(set(c.shininess.tolist())) == 3
    assert tuple(sh._bc(c.shininess, torch.zeros(3, 3, 5, 2)).shape) == (3, 1, 1, 1)
    meshes, frag, lights, cams, mats, leaves, texels = sc.scene(c, "cpu", F64, "plain")
    out = sh.phong_shading_reference(meshes, frag, lights, cams, mats, texels).detach()
    for n in range(3):  # image n alone, its shininess as the scalar Materials() takes
        mats.shininess = c.shininess[n:n + 1].to(F64)
        one = sh.phong_shading_reference(meshes, frag, lights, cams, mats, texels).detach()
        assert torch.equal(one[n], out[n])
        assert any(not torch.equal(one[m], out[m]) for m in range(3) if m != n)


# ------------------------------------------------------------------ one slot in Python floats
def _normalize(x):
    r = max(math.sqrt(sum(v * v for v in x)), 1e-6)
    return [v / r for v in x]


def _vertex_normal(c, vi):
    acc = [0.0, 0.0, 0.0]
    for f in c.faces.tolist():
        if vi not in f:
            continue
        p0, p1, p2 = ([float(t) for t in c.verts[j]] for j in f)
        a, b = [p1[i] - p0[i] for i in range(3)], [p2[i] - p0[i] for i in range(3)]
        cr = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
        acc = [acc[i] + cr[i] for i in range(3)]
    return _normalize(acc)


def _hand_colour(c, n, y, x, k):
    dot = lambda a, b: sum(p * q for p, q in zip(a, b))
    row = lambda t: [float(v) for v in t[n]]
    live = bool(c.live[n, y, x, k])
    P, Nn, uv, vc = [0.0] * 3, [0.0] * 3, [0.0, 0.0], [0.0] * 3
    if live:
        corners = c.faces[int(c.p2f[n, y, x, k])].tolist()
        b = [float(v) for v in c.bary[n, y, x, k]]
        mix = lambda rows: [sum(b[i] * float(rows[i][a]) for i in range(3)) for a in range(len(rows[0]))]
        P = mix([c.verts[j] for j in corners])
        Nn = mix([_vertex_normal(c, j) for j in corners])
        if c.spec.tex == "uv":
            uv = mix([c.verts_uvs[j] for j in corners])
        elif c.spec.tex == "vertex":
            vc = mix([c.tex[j] for j in corners])
    if c.spec.tex == "uv":
        ix = min(max(uv[0] * (sc.WM - 1), 0.0), sc.WM - 1.0)
        iy = min(max(uv[1] * (sc.HM - 1), 0.0), sc.HM - 1.0)
        x0, y0 = math.floor(ix), math.floor(iy)
        tex = [0.0] * 3
        for cx, cy, w in ((x0, y0, (x0 + 1 - ix) * (y0 + 1 - iy)), (x0 + 1, y0, (ix - x0) * (y0 + 1 - iy)),
                          (x0, y0 + 1, (x0 + 1 - ix) * (iy - y0)), (x0 + 1, y0 + 1, (ix - x0) * (iy - y0))):
            if 0 <= cx < sc.WM and 0 <= cy < sc.HM:  # v = 0 is the map's bottom row
                tex = [tex[i] + w * float(c.tex[n, sc.HM - 1 - cy, cx, i]) for i in range(3)]
    elif c.spec.tex == "vertex":
        tex = vc
    else:
        tex = [float(v) for v in c.tex[n, y, x, k]]
    L = row(c.light)
    d = _normalize(L if c.spec.light == "directional" else [L[i] - P[i] for i in range(3)])
    nh = _normalize(Nn)
    cos = dot(nh, d)
    R, T = c.R[n].tolist(), row(c.T)
    centre = [-sum(T[i] * R[j][i] for i in range(3)) for j in range(3)]
    view = _normalize([centre[i] - P[i] for i in range(3)])
    reflect = [-d[i] + 2.0 * cos * nh[i] for i in range(3)]
    alpha = max(dot(view, reflect), 0.0) * (1.0 if cos > 0 else 0.0)
    spec = alpha ** float(c.shininess[n])
    amb, ld, ls, md, ms = row(c.ambient), row(c.light_diffuse), row(c.light_specular), row(c.mat_diffuse), row(c.mat_specular)
    return [(amb[i] + md[i] * ld[i] * max(cos, 0.0)) * tex[i] + ms[i] * ls[i] * spec for i in range(3)], cos, alpha


@pytest.mark.parametrize("spec", [sc.FULL_CROSS[0], sc.FULL_CROSS[2], sc.FULL_CROSS[4]], ids=sc.spec_id)
def test_reference_matches_a_hand_evaluation(spec):
    """One lit slot with a specular term, one back-lit slot and one padded slot (of the last image:
    its rows, not image 0's), in plain Python floats."""
    c, ref = sc.build(spec), sc.shade_ref64(spec)
    cond = sc.conditions(c)
    n = spec.N - 1
    generic = c.live[n] & ~c.exact[n]
    picks = dict(lit=generic & (cond["cos"][n] > 0) & (cond["dotvr"][n] > 0.3), backlit=generic & (cond["cos"][n] < 0),
                 padded=~c.inside[n])
    for name, mask in picks.items():
        y, x, k = torch.nonzero(mask)[0].tolist()
        col, cos, alpha = _hand_colour(c, n, y, x, k)
        assert {"lit": cos > 0 and alpha > 0, "backlit": cos < 0 and alpha == 0, "padded": cos == 0 and alpha == 0}[name]
        got = ref.colours[n, y, x, k].tolist()
        assert max(abs(a - b) for a, b in zip(col, got)) <= 1e-12 * max(1.0, max(map(abs, got))), name


def test_camera_centres_are_the_library_s():
    from pertrenderer_amd.renderer import FoVPerspectiveCameras
    c = sc.build(sc.FULL_CROSS[0])
    lib = FoVPerspectiveCameras(R=c.R, T=c.T).get_camera_center()
    torch.testing.assert_close(sc.camera_centers(c.R, c.T), lib, rtol=1e-5, atol=1e-6)
    assert len({tuple(r) for r in lib.tolist()}) == c.spec.N


# --------------------------------------------------------------------------- conditioning
@pytest.mark.parametrize("spec", COMPOSITION, ids=sc.spec_id)
def test_float32_composition_is_inside_the_bars(spec):
    """The sanity bound on the cases' conditioning: torch's float32 composition of the same inputs
    holds the bars the kernels are held to (measured far inside: the GPU tests' bars are not what a
    float32 evaluation of these inputs needs)."""
    ref, f32 = sc.shade_ref64(spec), _library_composition(spec, F32)
    for name, a, b in zip(sc.Ref._fields, f32, ref):
        bar = sc.COLOUR_BAR if name == "colours" else sc.GRAD_BAR
        r = sc.ratio(a, b, bar)
        print(f"{sc.spec_id(spec)} float32 composition {name}: err / bar = {r:.3g}")
        assert r <= 1.0, (name, r)


@pytest.mark.parametrize("spec", sc.all_specs(), ids=sc.spec_id)
def test_case_conditions_hold(spec):
    """Every condition and share of the builder, on every case the GPU file runs."""
    c = sc.build(spec)
    N, H, W, K = spec.N, spec.H, spec.W, spec.K
    cond = sc.conditions(c)
    assert not cond["bad"].any()
    for name, share in cond["shares"].items():
        assert share >= sc.share_floor(name), (name, share)
    live = c.live & ~c.degenerate
    assert float(cond["cos"][live].abs().min()) >= sc.MIN_COS and float(cond["dotvr"][live].abs().min()) >= sc.MIN_COS
    # counts, the hole, poison
    assert c.counts.dtype == torch.int32 and int(c.counts.min()) == 0 and int(c.counts.max()) == K
    assert int(c.hole.sum()) == 1 and bool((c.hole & c.inside).any()) and bool((c.p2f_counts[c.hole] == -1).all())
    past = ~c.inside
    assert bool(torch.isnan(c.bary_counts[past]).all()) and bool(torch.isfinite(c.bary_counts[c.live]).all())
    assert bool((c.p2f_counts[past] >= 0).any()) and bool((c.p2f_counts[past] == -1).any())
    assert bool((c.p2f_counts[past] < c.faces.shape[0]).all())
    assert bool((c.p2f_plain[~c.live] == -1).all()) and bool((c.bary_plain[~c.live] == 0).all())
    # image n's live slots point into mesh n's faces only
    if not spec.shared:
        nF = c.faces_list[0].shape[0]
        img = torch.arange(N)[:, None, None, None].expand(N, H, W, K)
        assert bool((c.p2f_plain[c.live] // nF == img[c.live]).all())
    b = c.bary[c.live]
    assert bool((b >= 0).all()) and float((b.sum(-1) - 1).abs().max()) < 1e-6
    # the cotangent: exact zeros on a fair part of the live slots; padded slots by texture kind
    assert 0.25 < float(c.zero_bwd.sum()) / float(c.live.sum()) < 0.75
    assert bool((c.G[c.zero_bwd] == 0).all())
    assert bool((c.G[~c.live] == 0).all()) != (spec.tex == "given")
    # fill_padded's mixed 16-byte stores, from the counts
    mixed = sc.mixed_float4s(c.counts, K)
    assert mixed == c.mixed
    if K % 4:
        assert mixed["pixel"] > 0
    if K > 1:
        assert mixed["within"] > 0
    if spec[:4] == sc.MAIN:
        assert mixed["image"] > 0 and mixed["split"] > 0 and N * H * W == 105  # both kinds over an image boundary
    if spec.mesh == "sphere+line":
        assert int(c.degenerate.sum()) == 4 * N and bool((c.G[c.degenerate] != 0).any())


@pytest.mark.parametrize("name", list(sc.ACCUMULATORS))
def test_accumulator_cases_mean_what_they_say(name):
    spec, expected = sc.ACCUMULATORS[name]
    c = sc.build(spec)
    assert sc.accumulator_layout(c.verts.shape[0], spec.N) == expected
    assert (spec.N > sc.PAD_IMGS) == (name in ("lds-verts+atomic-batch", "atomic-verts+atomic-batch", "past-pad-table"))
    assert {e for _, e in sc.ACCUMULATORS.values()} == {(True, True), (True, False), (False, True), (False, False)}


@pytest.mark.parametrize("spec", [s for s in sc.all_specs() if s.tex == "uv"], ids=sc.spec_id)
def test_exact_slots_sit_on_texels_in_float32(spec):
    """The exact slots' map coordinates are integers in float32 too, computed the kernel's way
    (pr_phong.h src_coord), and reach the low clamp, a texel line and the high clamp on both axes."""
    c = sc.build(spec)
    assert int(c.exact.sum()) >= 6
    assert bool((c.bary[c.exact] == torch.tensor([1.0, 0.0, 0.0])).all()) and bool((c.G[c.exact] != 0).any())
    fv = c.faces[c.p2f[c.exact]]
    b = c.bary[c.exact]
    uv = (b[:, 0:1] * c.verts_uvs[fv[:, 0]] + b[:, 1:2] * c.verts_uvs[fv[:, 1]]) + b[:, 2:3] * c.verts_uvs[fv[:, 2]]
    assert uv.dtype == F32
    for axis, size in ((0, sc.WM), (1, sc.HM)):
        g = uv[:, axis] * 2.0 - 1.0
        x = ((g + 1.0) / 2.0) * float(size - 1)
        assert x.dtype == F32 and bool((x == x.round()).all())
        assert bool((x == 0).any()) and bool((x == size - 1).any()) and bool(((x > 0) & (x < size - 1)).any())

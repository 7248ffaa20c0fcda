"""Native point_mesh_face_distance / point_mesh_edge_distance (csrc/pr_pointmesh.hip behind
renderer/loss.py) on the GPU, against the float64 restatement of point_mesh_cases.py: distances,
selection, the planted exact ties, the gradients of the loss and of the raw outputs under a random
cotangent; against the torch composition on the device; bitwise reproducibility; the NaN rule;
padded, list-built and tensor-with-lengths clouds; capture in a HIP graph.

Every scene runs for faces and for edges, with the split count the library picks and with
PR_POINTMESH_SPLITS=3 (the other side cut into three ranges and merged).

Selection.  The scenes are seeded so that every primitive's best and second-best point differ by
>= 1e-6 in float64 d^2 (point_mesh_cases.scene asserts it): the primitive -> point indices must equal
float64's.  Point -> primitive indices are not compared: a point whose closest point lies on an edge
or vertex shared by several faces ties exactly across them; instead the float64 distance to the
primitive the kernel chose must meet assert_close against the float64 minimum.  The planted ties
(a face copied into the first, a middle and the last range, a duplicated point) must resolve to
the lowest index.

Tolerances.  Values: conftest.assert_close's defaults.  Gradients: against the float64 restatement
evaluated at the kernel's own indices, max-abs over max-abs; the bound is 4x the float32
restatement's own error on that case, floored at 1e-5 (the rule of test_gpu_mesh_losses.py), and
point_mesh_cases.float32_errors asserts that the restatement's error stays <= 2e-5, so the rule
cannot loosen.

Measured on an MI355X (float32 restatement error / native error, max-abs over max-abs, the largest
over all cases, kinds and both split settings): loss d points 1.54e-06 / 2.28e-06 (sphere_642, 1
point, edges), d verts 1.60e-06 / 1.19e-06 (hub70, 257 points, faces); raw outputs under the
cotangent d points 8.60e-07 / 9.63e-07, d verts 1.85e-06 / 1.96e-06 (hub70, 70 points, faces).
Everything is below the 1e-5 floor.

Known answers.  The hand-built table of point_mesh_cases.py (the seven Voronoi regions, a point in
the face and on a vertex, a collinear and an all-equal triangle, a zero-length edge, a segment's
interior and ends) goes through the kernel as single calls and as one batch with non-zero packed
offsets, with the library's ranges and with three (a single face cut into three ranges, two of them
empty): dist, idx and the weight outputs w_p / w_m are compared bitwise, since every intermediate is
a dyadic number of a few bits and the library is built without contraction.  A point in the face or
on a vertex gives a distance and gradients of exactly 0.  The table cannot reach the third segment
(c a) of a degenerate triangle: the three segments of collinear corners overlap, so (c a) is never
strictly nearer than the first two in exact arithmetic and wins by rounding only; the collapsed
scenes below reach it.

Collapsed meshes (point_mesh_cases.collapsed_scene: hub70 with face 3, sphere_642 with faces 5 and
700 collapsed to a point; 3 / 8 degenerate faces, 3 / 6 zero-length edges; 70 and 1025 points; the
library's ranges, 1 and 3) follow the rules above with one change: d verts is compared after the rows
of bitwise-equal vertex positions have been summed on both sides (point_mesh_cases.merged_rows),
because on an (a, b, b) face rounding decides whether the gradient goes to id b or to id c.  Also:
everything finite, weight rows non-negative and summing to 1 within 1e-6, w_m of an all-equal face
exactly (1, 0, 0), two calls bitwise equal.  Collinear faces with three distinct positions are left
out: the same closest point is expressed over (a, b), (b, c) or (c, a), so there is no unique
d verts to compare with (the float32 restatement is 2e-2 from float64 there); the table covers
their values.  Measured on an MI355X (as above, d verts through merged_rows; the largest over all
cases, kinds and split settings): loss d points 4.81e-07 / 6.31e-07, d verts 1.60e-06 (sphere_642,
70 points, faces) / 6.93e-07 (hub70, 1025 points, faces); raw outputs d points 6.28e-07 / 6.28e-07,
d verts 4.81e-06 / 4.56e-06 (hub70, 1025 points, faces).  Below the 1e-5 floor.

Point tiles.  sphere_642, hub70 and batch2 (its second cloud one point) with 513 and 1025 points run
the same body with PR_POINTMESH_SPLITS unset, 1, 2 and 3: a primitive then walks tiles of 512, 512
and 1 points in one range, ranges of 513 and 512, or the library's own unequal numbers of ranges for
the two directions; a duplicated point whose copies are two tiles apart resolves to the first copy
within a range and across the merge.  Measured on an MI355X (as above): loss d points 4.77e-07 /
5.44e-07, d verts 1.21e-06 (sphere_642, 1025 points, faces) / 8.02e-07 (hub70, 513 points, faces);
raw outputs d points 6.28e-07 / 6.28e-07, d verts 4.81e-06 / 4.56e-06 (hub70, 1025 points, faces)."""
import functools

import pytest
import torch

import point_mesh_cases as C
from conftest import assert_close
from mesh_loss_cases import rel_err
from pertrenderer_amd import _native as nat
from pertrenderer_amd.renderer import Meshes, Pointclouds, sample_points_from_meshes
from pertrenderer_amd.renderer import loss as L

pytestmark = pytest.mark.gpu

FN = {"faces": L.point_mesh_face_distance, "edges": L.point_mesh_edge_distance}


@pytest.fixture(params=[None, "3"], ids=["splits-default", "splits-3"])
def splits(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("PR_POINTMESH_SPLITS", raising=False)
    else:
        monkeypatch.setenv("PR_POINTMESH_SPLITS", request.param)
    return request.param


def _grads(out, c, v):
    """(d out / d packed points, d out / d packed verts) from one backward pass."""
    g = torch.autograd.grad(out, c + v, allow_unused=True)
    cat = lambda gs, xs: torch.cat([torch.zeros_like(x) if y is None else y for y, x in zip(gs, xs)])  # noqa: E731
    return cat(g[:len(c)], c), cat(g[len(c):], v)


def _run(verts, faces, clouds, kind, device, cot=None, native=True):
    """dict(dist_p, dist_m, idx_p, idx_m, w_p, w_m, loss, grad_points, grad_verts[, raw_grad_points, raw_grad_verts])."""
    keep = L.NATIVE_MESHLOSS
    L.NATIVE_MESHLOSS = native
    try:
        v = [x.to(device).requires_grad_(True) for x in verts]
        c = [x.to(device).requires_grad_(True) for x in clouds]
        mesh, pcl = Meshes(v, [f.to(device) for f in faces]), Pointclouds(c)
        loss = FN[kind](mesh, pcl)
        gp, gv = _grads(loss, c, v)
        out = dict(loss=loss.detach(), grad_points=gp, grad_verts=gv)
        dist_p, dist_m, idx_p, idx_m, w_p, w_m = L._point_mesh_nn(mesh, pcl, kind)[:6]
        out.update(dist_p=dist_p.detach(), dist_m=dist_m.detach(), idx_p=idx_p, idx_m=idx_m, w_p=w_p, w_m=w_m)
        if cot is not None:
            raw = (dist_p * cot[0].to(device)).sum() + (dist_m * cot[1].to(device)).sum()
            gp, gv = _grads(raw, c, v)
            out.update(raw_grad_points=gp, raw_grad_verts=gv)
    finally:
        L.NATIVE_MESHLOSS = keep
    return out


@functools.lru_cache(maxsize=None)
def _float64_minima(name, count, kind, collapsed=False):
    return C.dense_d2(*C.scene(name, count, collapsed), kind)


def _set_splits(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("PR_POINTMESH_SPLITS", raising=False)
    else:
        monkeypatch.setenv("PR_POINTMESH_SPLITS", value)


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("count", C.COUNTS)
@pytest.mark.parametrize("name", C.MESHES)
def test_native_matches_float64(name, count, kind, splits, device):
    _check_against_float64(name, count, kind, splits, device)


def _check_against_float64(name, count, kind, splits, device, collapsed=False):
    """The rules of the module docstring on one scene; on a collapsed scene d verts is compared
    after the rows of bitwise-equal vertex positions have been summed, on both sides.  Returns the
    kernel's outputs."""
    verts, faces, clouds = C.scene(name, count, collapsed)
    want, cot = C.references(name, count, kind, collapsed)
    got = _run(verts, faces, clouds, kind, device, cot)
    assert got["dist_p"].dtype == got["dist_m"].dtype == got["loss"].dtype == torch.float32
    assert got["idx_p"].dtype == got["idx_m"].dtype == torch.int32 and got["loss"].dim() == 0
    # values
    assert_close(got["dist_p"], want["dist_p"], name="dist_p")
    assert_close(got["dist_m"], want["dist_m"], name="dist_m")
    assert_close(got["loss"], want["loss"], name="loss")
    # selection: primitive -> point exactly; point -> primitive through its float64 distance
    idx_p, idx_m = got["idx_p"].cpu().long(), got["idx_m"].cpu().long()
    assert torch.equal(idx_m, want["idx_m"])
    poff = moff = 0
    for d in _float64_minima(name, count, kind, collapsed):
        P, M = d.shape
        local = idx_p[poff:poff + P] - moff
        assert ((local >= 0) & (local < M)).all(), "a point chose a primitive of another mesh"
        assert_close(d.gather(1, local[:, None])[:, 0], d.min(dim=1).values, name="d64 of the chosen primitive")
        poff, moff = poff + P, moff + M
    # gradients, at the kernel's own indices
    r64, ref_err = C.float32_errors(name, count, kind, (idx_p, idx_m), collapsed)
    err = {k: C.grad_error(got[k], r64[k], k, verts if collapsed else None) for k in C.GRAD_KEYS}
    print(f"{name}{' collapsed' if collapsed else ''} {count} {kind} splits={splits}: "
          "gradient error restatement(fp32) / native: "
          + ", ".join(f"{k} {ref_err[k]:.2e} / {err[k]:.2e}" for k in C.GRAD_KEYS))
    for k in C.GRAD_KEYS:
        assert err[k] <= max(4.0 * ref_err[k], 1e-5), (k, err[k], ref_err[k])
    return got


@pytest.mark.parametrize("kind", C.KINDS)
def test_planted_ties_resolve_to_the_lowest_index(kind, splits, device):
    verts, faces, clouds, copies, dup = C.tie_scene()
    want = C.reference(verts, faces, clouds, kind)
    got = _run(verts, faces, clouds, kind, device)
    idx_p, idx_m = got["idx_p"].cpu().long(), got["idx_m"].cpu().long()
    # the duplicated point: the first copy wins for every primitive that is nearest to it
    assert torch.equal(idx_m, want["idx_m"]) and (idx_m == dup[0]).any() and not (idx_m == dup[1]).any()
    assert_close(got["dist_p"], want["dist_p"], name="dist_p")
    assert got["dist_p"][dup[0]].item() == got["dist_p"][dup[1]].item() and idx_p[dup[0]] == idx_p[dup[1]]
    if kind == "faces":
        # the copies of the face lie in different ranges: within a range and across the merge the lowest wins
        assert idx_p[C.TIE_POINT].item() == copies[0] == want["idx_p"][C.TIE_POINT].item()
        assert not any((idx_p == c).any() for c in copies[1:])
        assert idx_m[list(copies)].unique().numel() == 1 and got["dist_m"][list(copies)].unique().numel() == 1


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("name", C.MESHES)
def test_native_matches_torch_composition(name, kind, splits, device):
    """Both paths are float32 statements of the same formulas, each within 4x the float32
    restatement's error of float64 (floored at 1e-5) by the rule above: against each other twice
    that.  Where the two chose different primitives for a point (an exact tie in float64 across a
    shared edge or vertex that float32 breaks either way) the closest points differ by the
    rounding of d^2, about sqrt(eps) = 3e-4 of the distance: 2e-3 then."""
    verts, faces, clouds = C.scene(name, 70)
    _, cot = C.references(name, 70, kind)
    a = _run(verts, faces, clouds, kind, device, cot)
    b = _run(verts, faces, clouds, kind, device, cot, native=False)
    assert torch.equal(a["idx_m"].long(), b["idx_m"])
    for k in ("dist_p", "dist_m", "loss"):
        assert_close(a[k], b[k], name=k)
    _, ref_err = C.float32_errors(name, 70, kind, (a["idx_p"].cpu().long(), a["idx_m"].cpu().long()))
    same = torch.equal(a["idx_p"].long(), b["idx_p"])
    for k in C.GRAD_KEYS:
        # where the two paths chose other faces of a tie the gradients differ by about sqrt(eps)
        assert rel_err(a[k], b[k]) <= (max(8.0 * ref_err[k], 2e-5) if same else 2e-3), (k, same)


def test_native_calls_are_bitwise_reproducible(splits, device):
    for name, kind in (("sphere_642", "faces"), ("batch2", "edges"), ("hub70", "faces")):
        verts, faces, clouds = C.scene(name, 257)
        _, cot = C.references(name, 257, kind)
        a, b = _run(verts, faces, clouds, kind, device, cot), _run(verts, faces, clouds, kind, device, cot)
        assert all(torch.equal(a[k], b[k]) for k in a), (name, kind)


@pytest.mark.parametrize("kind", C.KINDS)
def test_padded_list_and_length_forms_agree_bitwise(kind, splits, device):
    verts, faces, clouds = C.scene("batch2", 70)
    mesh = Meshes([v.to(device) for v in verts], [f.to(device) for f in faces])
    # full clouds: a padded tensor, a Pointclouds of it, a Pointclouds of its rows
    g = torch.Generator().manual_seed(3)
    full = torch.stack([clouds[0][:9], clouds[0][9:18] + 0.1 * torch.rand((9, 3), generator=g)]).to(device)
    outs = []
    for make in (lambda t: t, lambda t: Pointclouds(t), lambda t: Pointclouds([t[0], t[1]])):
        t = full.clone().requires_grad_(True)
        loss = FN[kind](mesh, make(t))
        outs.append((loss.detach(), torch.autograd.grad(loss, t)[0]))
    assert all(torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]) for o in outs[1:])
    # cut lengths: a padded tensor with device lengths against the list
    padded = torch.full((2, 70, 3), 7.0)
    padded[0], padded[1, :1] = clouds[0], clouds[1]
    pr = padded.to(device).requires_grad_(True)
    lengths = torch.tensor([70, 1], device=device)
    loss = FN[kind](mesh, pr, lengths=lengths)
    cl = [c.to(device).requires_grad_(True) for c in clouds]
    want = FN[kind](mesh, Pointclouds(cl))
    assert torch.equal(loss, want)
    (gp,) = torch.autograd.grad(loss, pr)
    gl = torch.autograd.grad(want, cl)
    assert torch.equal(gp[0], gl[0]) and torch.equal(gp[1, :1], gl[1]) and not gp[1, 1:].any()
    dist_p, _, idx_p, _, w_p = L._point_mesh_nn(mesh, pr, kind, lengths)[:5]
    assert not dist_p[71:].any() and (idx_p[71:] == -1).all() and not w_p[71:].any() and (idx_p[:71] >= 0).all()


def test_an_empty_cloud_contributes_nothing(splits, device):
    verts, faces, clouds = C.scene("batch2", 3)
    v = [x.to(device).requires_grad_(True) for x in verts]
    mesh = Meshes(v, [f.to(device) for f in faces])
    pcl = Pointclouds([clouds[0].to(device), torch.zeros((0, 3), device=device)])
    one = FN["faces"](Meshes(v[:1], [faces[0].to(device)]), Pointclouds([clouds[0].to(device)]))
    loss = FN["faces"](mesh, pcl)
    assert_close(loss, 0.5 * one, name="loss")
    gv = torch.autograd.grad(loss, v)
    assert gv[0].any() and not gv[1].any()
    dist_m, idx_m = L._point_mesh_nn(mesh, pcl, "faces")[1:4:2]
    F0 = faces[0].shape[0]
    assert (idx_m[F0:] == -1).all() and not dist_m[F0:].any() and (idx_m[:F0] >= 0).all()


@pytest.mark.parametrize("kind", C.KINDS)
def test_nan_points_are_never_chosen_and_not_silenced(kind, splits, device):
    """A NaN point gets a NaN distance, idx -1 and gradient 0 and is nobody's nearest point; points
    facing NaN primitives only get +inf: the loss shows the divergence."""
    verts, faces, clouds = C.scene("tetrahedron", 70)
    pts = clouds[0].clone()
    pts[5, 1] = float("nan")
    p = pts.to(device).requires_grad_(True)
    mesh = Meshes([verts[0].to(device)], [faces[0].to(device)])
    dist_p, dist_m, idx_p, idx_m = L._point_mesh_nn(mesh, Pointclouds([p]), kind)[:4]
    rest = [i for i in range(70) if i != 5]
    assert torch.isnan(dist_p[5]) and idx_p[5] == -1 and torch.isfinite(dist_p[rest]).all() and (idx_p[rest] >= 0).all()
    assert torch.isfinite(dist_m).all() and (idx_m != 5).all() and (idx_m >= 0).all()
    (g,) = torch.autograd.grad(dist_p[rest].sum() + dist_m.sum(), p)
    assert not g[5].any() and torch.isfinite(g).all()
    assert not torch.isfinite(FN[kind](mesh, Pointclouds([pts.to(device)])))
    bad = Meshes([torch.full_like(verts[0], float("nan")).to(device)], [faces[0].to(device)])
    dist_p, dist_m, idx_p, idx_m = L._point_mesh_nn(bad, Pointclouds([clouds[0].to(device)]), kind)[:4]
    assert torch.isinf(dist_p).all() and (dist_p > 0).all() and (idx_p == -1).all()
    assert torch.isnan(dist_m).all() and (idx_m == -1).all()


def test_raw_op_refuses_cpu_tensors():
    verts, faces, clouds = C.scene("tetrahedron", 3)
    mesh = Meshes(verts, faces)
    with pytest.raises(nat.NativeError):
        L._PointMeshFn.apply(clouds[0], verts[0], mesh._topo, "faces", None, None, 3)


def test_fitting_step_is_captured_in_a_graph(device):
    """Sample a target cloud, point_mesh_face_distance + point_mesh_edge_distance + mesh_edge_loss,
    backward and an in-place SGD update of the vertex offsets in one captured graph, after one
    warm-up call: three replays equal three eager steps from the same start, bitwise."""
    verts, faces, _ = C.scene("sphere_642", 1)
    base = Meshes([verts[0].to(device)], [faces[0].to(device)])
    target = Meshes([(1.15 * verts[0] + 0.03).to(device)], [faces[0].to(device)])
    start = (0.02 * torch.randn(verts[0].shape, generator=torch.Generator().manual_seed(5))).to(device)
    lr = 0.05

    def objective(deform):
        mesh = base.offset_verts(deform)
        cloud = Pointclouds(sample_points_from_meshes(target, 500, seed=11))
        return (L.point_mesh_face_distance(mesh, cloud) + 0.5 * L.point_mesh_edge_distance(mesh, cloud)
                + 0.1 * L.mesh_edge_loss(mesh))

    def step(deform):
        loss = objective(deform)
        loss.backward()
        with torch.no_grad():
            deform.add_(deform.grad, alpha=-lr)
        return loss

    d_e = start.clone().requires_grad_(True)
    eager = []
    for _ in range(3):
        d_e.grad = None
        eager.append(step(d_e).detach().clone())

    d_g = start.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the one call before the capture: caches, autograd warm-up
        objective(d_g).backward()
    torch.cuda.current_stream().wait_stream(side)
    d_g.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step(d_g)
    replayed = []
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        replayed.append(loss.detach().clone())
    for i, (a, b) in enumerate(zip(eager, replayed)):
        assert torch.equal(a, b), (i, a.item(), b.item())
    assert torch.equal(d_e.detach(), d_g.detach())
    assert not torch.equal(d_g.detach(), start) and eager[2].item() < eager[0].item()


# ---- known answers through the kernel: the table of point_mesh_cases.py, bitwise


def _nn(verts, faces, clouds, kind, device):
    """The six outputs of _point_mesh_nn on the CPU, from float32 lists moved to the device."""
    mesh = Meshes([torch.tensor(v).to(device) for v in verts], [torch.tensor(f).to(device) for f in faces])
    out = L._point_mesh_nn(mesh, Pointclouds([torch.tensor(c).to(device) for c in clouds]), kind)[:6]
    return [o.detach().cpu() for o in out]


def _expect(got, want, label):
    """Bitwise: every value of the table is exact in float32 and the library is built without contraction."""
    for name, g, w in zip(("dist_p", "dist_m", "idx_p", "idx_m", "w_p", "w_m"), got, want):
        w = torch.tensor(w, dtype=g.dtype).reshape(g.shape)
        assert torch.equal(g, w), (label, name, g.tolist(), w.tolist())


ONE_FACE = [[0, 1, 2]]  # three distinct vertex ids, whatever their positions


def test_known_answers_of_the_regions_through_the_kernel(splits, device):
    points = [p for p, _, _ in C.REGIONS.values()]
    d2 = [d for _, d, _ in C.REGIONS.values()]
    w = [x for _, _, x in C.REGIONS.values()]
    near = list(C.REGIONS).index("on the triangle")
    assert near == 7 and d2[near] == d2[near + 1] == 0.0  # the first of the two points at distance 0
    # the regular triangle with its nine points
    got = _nn([C.TRI], [ONE_FACE], [points], "faces", device)
    _expect(got, (d2, [0.0], [0] * 9, [7], w, [[0.25, 0.25, 0.5]]), "nine points")
    # one point at a time: the primitive -> point direction sees every region too
    for label, (p, d, x) in C.REGIONS.items():
        _expect(_nn([C.TRI], [ONE_FACE], [[p]], "faces", device), ([d], [d], [0], [0], [x], [x]), label)
    # the degenerate triangles, alone
    for label, (t, p, d, x) in C.DEGENERATE_TRIANGLES.items():
        _expect(_nn([t], [ONE_FACE], [[p]], "faces", device), ([d], [d], [0], [0], [x], [x]), label)
    assert C.DEGENERATE_TRIANGLES["collinear"][2:] == (1.0, [0.0, 0.5, 0.5])
    assert C.DEGENERATE_TRIANGLES["all equal"][2:] == (4.0, [1.0, 0.0, 0.0])
    # one batch: the packed offsets of the second and third element are not 0
    deg = list(C.DEGENERATE_TRIANGLES.values())
    got = _nn([C.TRI] + [t for t, _, _, _ in deg], [ONE_FACE] * 3, [points] + [[p] for _, p, _, _ in deg], "faces", device)
    _expect(got, (d2 + [d for _, _, d, _ in deg], [0.0] + [d for _, _, d, _ in deg], [0] * 9 + [1, 2], [7, 9, 10],
                  w + [x for _, _, _, x in deg], [[0.25, 0.25, 0.5]] + [x for _, _, _, x in deg]), "batch")


def test_known_answers_of_the_edges_through_the_kernel(splits, device):
    cases = C.known_edge_cases()
    assert cases[0][3:] == (4.0, [1.0, 0.0, 0.0]) and cases[-1][3] == 4.0625
    for label, tri, p, d, x in cases:  # edge 0 = (0 1) is the segment under test
        dist_p, dist_m, idx_p, idx_m, w_p, w_m = _nn([tri], [ONE_FACE], [[p]], "edges", device)
        assert dist_m.shape == (3,) and (idx_m == 0).all()
        _expect((dist_p, dist_m[:1], idx_p, idx_m[:1], w_p, w_m[:1]), ([d], [d], [0], [0], [x], [x]), label)
    # one batch, one point per mesh
    got = _nn([t for _, t, _, _, _ in cases], [ONE_FACE] * len(cases), [[p] for _, _, p, _, _ in cases], "edges", device)
    dist_p, dist_m, idx_p, idx_m, w_p, w_m = got
    n = len(cases)
    _expect((dist_p, dist_m[::3], idx_p, idx_m[::3], w_p, w_m[::3]),
            ([d for *_, d, _ in cases], [d for *_, d, _ in cases], [3 * i for i in range(n)], list(range(n)),
             [x for *_, x in cases], [x for *_, x in cases]), "batch")


@pytest.mark.parametrize("where", ["on the triangle", "on a vertex"])
def test_a_point_on_the_face_has_distance_and_gradients_of_exactly_zero(where, splits, device):
    p, d, _ = C.REGIONS[where]
    assert d == 0.0
    for verts, clouds in (([C.TRI], [[p]]), ([C.DEGENERATE_TRIANGLES["all equal"][0], C.TRI], [[[1.0, 2.0, 3.0]], [p]])):
        v = [torch.tensor(x, device=device, requires_grad=True) for x in verts]
        c = [torch.tensor(x, device=device, requires_grad=True) for x in clouds]
        mesh = Meshes(v, [torch.tensor(ONE_FACE, device=device)] * len(v))
        dist_p, dist_m = L._point_mesh_nn(mesh, Pointclouds(c), "faces")[:2]
        assert not dist_p.any() and not dist_m.any()
        cot_p, cot_m = torch.full_like(dist_p, 3.0), torch.full_like(dist_m, -5.0)
        gp, gv = _grads((dist_p * cot_p).sum() + (dist_m * cot_m).sum(), c, v)
        assert not gp.any() and not gv.any() and torch.isfinite(gp).all() and torch.isfinite(gv).all()


# ---- collapsed meshes: degenerate faces and zero-length edges against float64, gradients included


@pytest.mark.parametrize("nsplits", [None, "1", "3"], ids=["splits-default", "splits-1", "splits-3"])
@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("count", C.COLLAPSED_COUNTS)
@pytest.mark.parametrize("name", list(C.COLLAPSED))
def test_collapsed_meshes_match_float64(name, count, kind, nsplits, monkeypatch, device):
    _set_splits(monkeypatch, nsplits)
    got = _check_against_float64(name, count, kind, nsplits, device, collapsed=True)
    assert all(torch.isfinite(got[k]).all() for k in got if got[k].is_floating_point())
    for w, idx in ((got["w_p"], got["idx_p"]), (got["w_m"], got["idx_m"])):
        assert (idx >= 0).all() and (w >= 0).all()
        assert ((w.double().sum(dim=1) - 1).abs() <= 1e-6).all()
    if kind == "faces":  # three ids at one position: the first segment's first endpoint
        w = got["w_m"][list(C.COLLAPSED[name])].cpu()
        assert torch.equal(w, torch.tensor([[1.0, 0.0, 0.0]]).expand_as(w))
    verts, faces, clouds = C.scene(name, count, True)
    _, cot = C.references(name, count, kind, True)
    again = _run(verts, faces, clouds, kind, device, cot)
    assert all(torch.equal(got[k], again[k]) for k in got)


# ---- clouds longer than the 512-point tile: the tiles and the ranges a primitive walks


@pytest.mark.parametrize("nsplits", [None, "1", "2", "3"], ids=["splits-default", "splits-1", "splits-2", "splits-3"])
@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("count", C.TILE_COUNTS)
@pytest.mark.parametrize("name", C.TILE_MESHES)
def test_native_matches_float64_across_point_tiles(name, count, kind, nsplits, monkeypatch, device):
    """1025 points: one range is tiles of 512, 512 and 1; two ranges are 513 and 512 (a tile and one
    point); the library's own choice cuts the points and the primitives into unequal numbers of ranges."""
    _set_splits(monkeypatch, nsplits)
    _check_against_float64(name, count, kind, nsplits, device)


@pytest.mark.parametrize("nsplits", [None, "1", "2", "3"], ids=["splits-default", "splits-1", "splits-2", "splits-3"])
@pytest.mark.parametrize("kind", C.KINDS)
def test_far_duplicate_resolves_to_the_lowest_index(kind, nsplits, monkeypatch, device):
    """The duplicated point's copies are two tiles apart: the first wins across a tile boundary
    within a range and across the merge of two or three ranges."""
    _set_splits(monkeypatch, nsplits)
    verts, faces, clouds, copies, dup = C.tie_scene(C.TIE_COUNT_FAR)
    assert dup[1] - dup[0] > 512
    want = C.reference(verts, faces, clouds, kind)
    got = _run(verts, faces, clouds, kind, device)
    idx_p, idx_m = got["idx_p"].cpu().long(), got["idx_m"].cpu().long()
    assert torch.equal(idx_m, want["idx_m"]) and (idx_m == dup[0]).any() and not (idx_m == dup[1]).any()
    assert_close(got["dist_p"], want["dist_p"], name="dist_p")
    assert_close(got["dist_m"], want["dist_m"], name="dist_m")
    assert got["dist_p"][dup[0]].item() == got["dist_p"][dup[1]].item() and idx_p[dup[0]] == idx_p[dup[1]]
    if kind == "faces":
        assert idx_p[C.TIE_POINT].item() == copies[0] and not any((idx_p == c).any() for c in copies[1:])
        assert idx_m[list(copies)].unique().numel() == 1 and got["dist_m"][list(copies)].unique().numel() == 1


@pytest.mark.parametrize("nsplits", [None, "2"], ids=["splits-default", "splits-2"])
def test_native_calls_are_bitwise_reproducible_across_point_tiles(nsplits, monkeypatch, device):
    _set_splits(monkeypatch, nsplits)
    for name, kind in (("sphere_642", "faces"), ("batch2", "edges")):
        verts, faces, clouds = C.scene(name, 1025)
        _, cot = C.references(name, 1025, kind)
        a, b = _run(verts, faces, clouds, kind, device, cot), _run(verts, faces, clouds, kind, device, cot)
        assert all(torch.equal(a[k], b[k]) for k in a), (name, kind)

"""point_mesh_face_distance / point_mesh_edge_distance on the CPU (the torch composition of
renderer/loss.py) and the Pointclouds structure: hand known-answer cases of the closest-point
arithmetic (the seven Voronoi regions, degenerate primitives), the composition against the
restatement of point_mesh_cases.py, gradcheck in float64, argument checks, the shim's exports."""
import pytest
import torch

import point_mesh_cases as C
from conftest import assert_close
from mesh_loss_cases import brute_edges, case, packed, rel_err
from pertrenderer_amd import renderer
from pertrenderer_amd.renderer import Meshes, Pointclouds
from pertrenderer_amd.renderer import loss as L
# the known-answer table, shared with the device tests (test_gpu_point_mesh.py)
from point_mesh_cases import DEGENERATE_TRIANGLES as DEGENERATE, REGIONS, SEGMENT, SEGMENT_CASES, TRI, ZERO_LENGTH

FN = {"faces": L.point_mesh_face_distance, "edges": L.point_mesh_edge_distance}


def _closest_fns():
    return {"composition": lambda p, pv: L._closest(p, pv)[:2], "restatement": C.closest}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("which", ["composition", "restatement"])
def test_known_answers_of_the_voronoi_regions(which, dtype):
    fn = _closest_fns()[which]
    tri = torch.tensor(TRI, dtype=dtype)
    for name, (p, d2, w) in REGIONS.items():
        d, got = fn(torch.tensor([p], dtype=dtype), tri[None])
        assert d.item() == d2, (name, d.item())
        assert torch.equal(got[0], torch.tensor(w, dtype=dtype)), (name, got)
    for name, (t, p, d2, w) in DEGENERATE.items():
        d, got = fn(torch.tensor([p], dtype=dtype), torch.tensor([t], dtype=dtype))
        assert d.item() == d2 and torch.equal(got[0], torch.tensor(w, dtype=dtype)), (name, d.item(), got)
    # a zero-length edge is its endpoint
    s, p, d2, w = ZERO_LENGTH
    d, got = fn(torch.tensor([p], dtype=dtype), torch.tensor([s], dtype=dtype))
    assert d.item() == d2 == 4.0 and torch.equal(got[0], torch.tensor(w, dtype=dtype)) and w == [1.0, 0.0, 0.0]
    # a segment's interior and its two ends
    seg = torch.tensor([SEGMENT], dtype=dtype)
    for p, d2, w in SEGMENT_CASES:
        d, got = fn(torch.tensor([p], dtype=dtype), seg)
        assert d.item() == d2 and torch.equal(got[0], torch.tensor(w, dtype=dtype)), (p, d.item(), got)


def test_known_answers_through_the_public_functions():
    pts = torch.tensor([p for p, _, _ in REGIONS.values()])
    want = torch.tensor([d for _, d, _ in REGIONS.values()])
    mesh = Meshes([torch.tensor(TRI)], [torch.tensor([[0, 1, 2]])])
    dist_p, dist_m, idx_p, idx_m = L._point_mesh_nn(mesh, Pointclouds([pts]), "faces")[:4]
    assert torch.equal(dist_p, want) and (idx_p == 0).all()
    assert dist_m.item() == 0.0 and idx_m.item() == 7  # the first of the two points at distance 0
    loss = L.point_mesh_face_distance(mesh, Pointclouds([pts]))
    assert loss.dim() == 0 and loss.item() == pytest.approx(want.mean().item(), rel=1e-6)
    # the edges of the triangle: the point above the interior is nearest to (a b), at (0.25, 0, 0)
    p, d2, w = C.ABOVE_INTERIOR_TO_EDGES
    assert p == REGIONS["interior"][0] and d2 == 4.0625
    dist_p, _, idx_p, _, w_p = L._point_mesh_nn(mesh, Pointclouds([torch.tensor([p])]), "edges")[:5]
    assert dist_p.item() == d2 and idx_p.item() == 0 and torch.equal(w_p[0], torch.tensor(w))


def test_known_answers_of_the_edges_through_the_public_functions():
    """The hand-built edge meshes of the device tests: the composition gives the table's values at edge 0."""
    for label, tri, p, d2, w in C.known_edge_cases():
        mesh = Meshes([torch.tensor(tri)], [torch.tensor([[0, 1, 2]])])
        dist_p, dist_m, idx_p, idx_m, w_p, w_m = L._point_mesh_nn(mesh, Pointclouds([torch.tensor([p])]), "edges")[:6]
        assert dist_p.item() == d2 and idx_p.item() == 0 and torch.equal(w_p[0], torch.tensor(w)), (label, dist_p, w_p)
        assert dist_m[0].item() == d2 and (idx_m == 0).all() and torch.equal(w_m[0], torch.tensor(w)), (label, dist_m, w_m)


# every scene the device tests add: (mesh, count, collapsed)
DEVICE_SCENES = ([(n, c, False) for n in C.TILE_MESHES for c in C.TILE_COUNTS]
                 + [(n, c, True) for n in C.COLLAPSED for c in C.COLLAPSED_COUNTS])


@pytest.mark.parametrize("name,count,collapsed", DEVICE_SCENES)
def test_conditions_of_the_device_scenes(name, count, collapsed):
    """What the device tests rely on, checked without a device: the gap rule (asserted by the
    builder, stated again here), the float32 restatement's gradient error at float64's indices
    within MAX_RESTATEMENT_ERROR (on a collapsed mesh with the d verts rows of equal positions
    summed), and on the collapsed hub70 a degenerate face among the points' float64 choices."""
    verts, faces, clouds = C.scene(name, count, collapsed)
    assert [c.shape[0] for c in clouds] == C.lengths_of(name, count)
    assert C.min_gap(verts, faces, clouds) >= C.MIN_GAP
    for kind in C.KINDS:
        want, _ = C.references(name, count, kind, collapsed)
        _, err = C.float32_errors(name, count, kind, (want["idx_p"], want["idx_m"]), collapsed)
        assert max(err.values()) <= C.MAX_RESTATEMENT_ERROR, (kind, err)
        print(f"{name} {count} collapsed={collapsed} {kind}: restatement(fp32) "
              + ", ".join(f"{k} {e:.2e}" for k, e in err.items()))
    if collapsed:
        assert len(C.degenerate_faces(verts[0], faces[0])) >= 3 * len(C.COLLAPSED[name])
        if name == "hub70":
            assert C.degenerate_choices(verts, faces, clouds) > 0


def test_merged_rows_sums_equal_positions_per_mesh():
    v = torch.tensor([[1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [1.0, 2.0, 3.0]])
    g = torch.tensor([[1.0, 0.0, 0.0], [0.0, 5.0, 0.0], [0.0, 0.0, 2.0]])
    got = C.merged_rows(g, [v])
    assert got.shape == (2, 3) and sorted(got.tolist()) == [[0.0, 5.0, 0.0], [1.0, 0.0, 2.0]]
    # equal positions of different meshes stay apart; a swap between coincident ids of one mesh is not seen
    assert C.merged_rows(torch.cat([g, g]), [v, v]).shape == (4, 3)
    assert C.grad_error(g[[2, 1, 0]], g, "grad_verts", [v]) == 0.0 and C.grad_error(g[[2, 1, 0]], g, "grad_verts") > 0.0


def test_far_tie_scene_splits_the_duplicates_over_tiles_and_ranges():
    verts, faces, clouds, copies, dup = C.tie_scene(C.TIE_COUNT_FAR)
    assert C.tie_scene()[4] == (1, C.TIE_COUNT - 1)  # the scene of the 70-point tests is what it was
    assert clouds[0].shape[0] == 1025 and dup[1] == 1024 and torch.equal(clouds[0][dup[0]], clouds[0][1024])
    assert dup[1] - dup[0] > 512 and dup[0] // 512 == 0 and dup[1] // 512 == 2  # one range: the first and the third tile
    assert all(dup[0] // -(-1025 // s) == 0 and dup[1] // -(-1025 // s) == s - 1 for s in (2, 3))  # first and last range
    for kind in C.KINDS:
        want = C.reference(verts, faces, clouds, kind)
        assert (want["idx_m"] == dup[0]).any() and not (want["idx_m"] == dup[1]).any()


def _grads(out, c, v):
    """(d out / d packed points, d out / d packed verts) from one backward pass."""
    g = torch.autograd.grad(out, c + v, allow_unused=True)
    cat = lambda gs, xs: torch.cat([torch.zeros_like(x) if y is None else y for y, x in zip(gs, xs)])  # noqa: E731
    return cat(g[:len(c)], c), cat(g[len(c):], v)


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("count", [3, 70])
@pytest.mark.parametrize("name", C.MESHES)
def test_composition_matches_the_restatement(name, count, kind):
    verts, faces, clouds = C.scene(name, count)
    want, cot = C.references(name, count, kind)
    for dtype, tol in ((torch.float64, 1e-12), (torch.float32, None)):
        v = [x.to(dtype).clone().requires_grad_(True) for x in verts]  # the scene's tensors are shared: never marked
        c = [x.to(dtype).clone().requires_grad_(True) for x in clouds]
        mesh, pcl = Meshes(v, faces), Pointclouds(c)
        dist_p, dist_m, idx_p, idx_m = L._point_mesh_nn(mesh, pcl, kind)[:4]
        assert torch.equal(idx_m, want["idx_m"])  # the gap rule: float32 cannot pick another point
        loss = FN[kind](mesh, pcl)
        if tol is not None:
            assert torch.equal(idx_p, want["idx_p"])
            for got, key in ((dist_p, "dist_p"), (dist_m, "dist_m"), (loss, "loss")):
                assert (got - want[key]).abs().max() <= tol * want[key].abs().max(), key
            gp, gv = _grads(loss, c, v)
            assert rel_err(gp, want["grad_points"]) <= tol and rel_err(gv, want["grad_verts"]) <= tol
            gp, gv = _grads((dist_p * cot[0].to(dtype)).sum() + (dist_m * cot[1].to(dtype)).sum(), c, v)
            assert rel_err(gp, want["raw_grad_points"]) <= tol and rel_err(gv, want["raw_grad_verts"]) <= tol
        else:
            assert loss.dtype == torch.float32
            assert_close(dist_p, want["dist_p"], name="dist_p")
            assert_close(dist_m, want["dist_m"], name="dist_m")
            assert_close(loss, want["loss"], name="loss")
            r64, err = C.float32_errors(name, count, kind, (idx_p, idx_m))
            gp, gv = _grads(loss, c, v)
            assert rel_err(gp, r64["grad_points"]) <= max(4 * err["grad_points"], 1e-5)
            assert rel_err(gv, r64["grad_verts"]) <= max(4 * err["grad_verts"], 1e-5)


@pytest.mark.parametrize("kind", C.KINDS)
def test_gradcheck_in_float64(kind):
    verts, faces, clouds = C.scene("tetrahedron", 3)

    def fn(p, v):
        return FN[kind](Meshes([v], faces), Pointclouds([p]))

    p, v = clouds[0].double().requires_grad_(True), verts[0].double().requires_grad_(True)
    assert torch.autograd.gradcheck(fn, (p, v), eps=1e-6, atol=1e-7, rtol=1e-5)
    verts, faces, clouds = C.scene("batch2", 3)

    def fn2(p0, p1, v0, v1):
        dist_p, dist_m = L._point_mesh_nn(Meshes([v0, v1], faces), Pointclouds([p0, p1]), kind)[:2]
        return torch.cat([dist_p, dist_m])

    leaves = [x.double().requires_grad_(True) for x in clouds + verts]
    assert torch.autograd.gradcheck(fn2, leaves, eps=1e-6, atol=1e-7, rtol=1e-5)


def test_composition_resolves_planted_ties_to_the_lowest_index(monkeypatch):
    verts, faces, clouds, copies, dup = C.tie_scene()
    monkeypatch.setattr(L, "_PAIRS_PER_CHUNK", 20 * faces[0].shape[0])  # blocks of 20 points: the duplicate is in another block
    dist_p, dist_m, idx_p, idx_m = L._point_mesh_nn(Meshes(verts, faces), Pointclouds(clouds), "faces")[:4]
    want = C.reference(verts, faces, clouds, "faces")
    assert idx_p[C.TIE_POINT].item() == copies[0] == want["idx_p"][C.TIE_POINT].item()
    assert torch.equal(idx_m, want["idx_m"]) and (idx_m == dup[0]).any() and not (idx_m == dup[1]).any()
    assert idx_m[list(copies)].unique().numel() == 1 and dist_m[list(copies)].unique().numel() == 1
    assert_close(dist_p, want["dist_p"], name="dist_p")


def test_padded_tensor_with_lengths_equals_the_list():
    verts, faces, clouds = C.scene("batch2", 70)
    padded = torch.zeros((2, 70, 3))
    padded[0], padded[1, :1] = clouds[0], clouds[1]
    padded[1, 1:] = 7.0  # padding is never read
    lengths = torch.tensor([70, 1])
    mesh = Meshes(verts, faces)
    for kind in C.KINDS:
        want = FN[kind](mesh, Pointclouds(clouds))
        pr = padded.clone().requires_grad_(True)
        got = FN[kind](mesh, pr, lengths=lengths)
        assert torch.equal(got, want)
        (g,) = torch.autograd.grad(got, pr)
        assert not g[1, 1:].any() and g[1, 0].any()
        dist_p, _, idx_p = L._point_mesh_nn(mesh, padded, kind, lengths)[:3]
        assert not dist_p[71:].any() and (idx_p[71:] == -1).all() and (idx_p[:71] >= 0).all()
        # full clouds: the padded tensor, a Pointclouds of it and of its rows agree
        full = FN[kind](mesh, padded[:, :3])
        assert torch.equal(full, FN[kind](mesh, Pointclouds(padded[:, :3])))
        assert torch.equal(full, FN[kind](mesh, Pointclouds([padded[0, :3], padded[1, :3]])))


def test_nothing_on_the_other_side_contributes_zero():
    verts, faces, clouds = C.scene("batch2", 3)
    mesh = Meshes(verts, faces)
    one = L.point_mesh_face_distance(Meshes(verts[:1], faces[:1]), Pointclouds(clouds[:1]))
    v = [x.clone().requires_grad_(True) for x in verts]
    loss = L.point_mesh_face_distance(Meshes(v, faces), Pointclouds([clouds[0], torch.zeros((0, 3))]))
    assert loss.item() == pytest.approx(0.5 * one.item(), rel=1e-6)
    gv = torch.autograd.grad(loss, v, allow_unused=True)
    assert gv[0].any() and (gv[1] is None or not gv[1].any())
    dist_p, dist_m, idx_p, idx_m = L._point_mesh_nn(mesh, Pointclouds([clouds[0], torch.zeros((0, 3))]), "edges")[:4]
    E0 = len(brute_edges(faces[0]))
    assert (idx_m[E0:] == -1).all() and not dist_m[E0:].any() and (idx_m[:E0] >= 0).all()
    empty = L.point_mesh_edge_distance(mesh, Pointclouds([torch.zeros((0, 3)), torch.zeros((0, 3))]))
    assert empty.dim() == 0 and empty.item() == 0.0


def test_nan_candidates_are_never_chosen():
    verts, faces, clouds = C.scene("tetrahedron", 3)
    pts = clouds[0].clone()
    pts[1, 2] = float("nan")
    for kind in C.KINDS:
        p = pts.clone().requires_grad_(True)
        dist_p, dist_m, idx_p, idx_m = L._point_mesh_nn(Meshes(verts, faces), Pointclouds([p]), kind)[:4]
        assert torch.isnan(dist_p[1]) and idx_p[1] == -1 and torch.isfinite(dist_p[[0, 2]]).all()
        assert torch.isfinite(dist_m).all() and (idx_m != 1).all() and (idx_m >= 0).all()
        (g,) = torch.autograd.grad(dist_p[[0, 2]].sum() + dist_m.sum(), p)
        assert not g[1].any() and torch.isfinite(g).all()
        assert not torch.isfinite(FN[kind](Meshes(verts, faces), Pointclouds([pts])))
    bad = [torch.full_like(verts[0], float("nan"))]
    dist_p, dist_m, idx_p, idx_m = L._point_mesh_nn(Meshes(bad, faces), Pointclouds(clouds), "faces")[:4]
    assert torch.isinf(dist_p).all() and (idx_p == -1).all() and torch.isnan(dist_m).all() and (idx_m == -1).all()


def test_arguments_are_checked():
    verts, faces, clouds = C.scene("batch2", 3)
    mesh = Meshes(verts, faces)
    pad = torch.zeros((2, 4, 3))
    for fn in FN.values():
        with pytest.raises(ValueError, match="batch size"):
            fn(mesh, Pointclouds(clouds[:1]))
        with pytest.raises(ValueError, match="batch size"):
            fn(mesh, torch.zeros((3, 4, 3)))
        with pytest.raises(ValueError, match="Pointclouds or a padded"):
            fn(mesh, torch.zeros((2, 4, 2)))
        with pytest.raises(ValueError, match="Pointclouds or a padded"):
            fn(mesh, clouds)
        with pytest.raises(ValueError, match="Meshes"):
            fn(verts, Pointclouds(clouds))
        with pytest.raises(ValueError, match="lengths"):
            fn(mesh, pad, lengths=torch.tensor([1.0, 2.0]))
        with pytest.raises(ValueError, match="lengths"):
            fn(mesh, pad, lengths=torch.tensor([1, 2, 3]))
        with pytest.raises(ValueError, match="lengths"):
            fn(mesh, Pointclouds(clouds), lengths=torch.tensor([1, 1]))
        with pytest.raises(ValueError, match="is on"):
            fn(mesh, torch.zeros((2, 4, 3), device="meta"))
    with pytest.raises(ValueError):
        Pointclouds(torch.zeros((2, 3)))
    with pytest.raises(ValueError):
        Pointclouds([torch.zeros((2, 3)), torch.zeros((4, 2))])
    with pytest.raises(ValueError, match="normals"):
        Pointclouds([torch.zeros((2, 3))], normals=[torch.zeros((3, 3))])


def test_pointclouds_accessors():
    g = torch.Generator().manual_seed(1)
    a, b, c = (torch.rand((n, 3), generator=g, requires_grad=True) for n in (4, 1, 6))
    pc = Pointclouds([a, b, c])
    assert len(pc) == 3 and pc.device == a.device
    assert pc.points_list()[1] is b
    assert torch.equal(pc.points_packed(), torch.cat([a, b, c]))
    assert pc.num_points_per_cloud().tolist() == [4, 1, 6] and pc.num_points_per_cloud().dtype == torch.int64
    assert pc.cloud_to_packed_first_idx().tolist() == [0, 4, 5]
    assert pc.packed_to_cloud_idx().tolist() == [0] * 4 + [1] + [2] * 6
    padded = pc.points_padded()
    assert padded.shape == (3, 6, 3) and torch.equal(padded[0, :4], a) and not padded[1, 1:].any()
    # gradients flow to the tensors it was given, through the packed and the padded view
    ga = torch.autograd.grad(pc.points_packed().sum() + 2 * pc.points_padded().sum(), [a, b, c])
    assert all(torch.equal(x, torch.full_like(x, 3.0)) for x in ga)
    # the index tables are built once
    assert pc.num_points_per_cloud() is pc.num_points_per_cloud()
    assert pc.cloud_to_packed_first_idx() is pc.cloud_to_packed_first_idx()
    assert pc.packed_to_cloud_idx() is pc.packed_to_cloud_idx() and pc.loss_weights() is pc.loss_weights()
    assert torch.allclose(pc.loss_weights(), torch.tensor([1 / 12] * 4 + [1 / 3] + [1 / 18] * 6))
    # a padded tensor: every cloud has P points, the views are the tensor itself
    t = torch.rand((2, 5, 3), generator=g, requires_grad=True)
    n = torch.rand((2, 5, 3), generator=g)
    pt = Pointclouds(t, normals=n)
    assert pt.points_padded() is t and pt.normals_padded() is n and pt.num_points_per_cloud().tolist() == [5, 5]
    assert torch.equal(pt.points_packed(), t.reshape(10, 3)) and torch.equal(pt.normals_packed(), n.reshape(10, 3))
    assert torch.equal(pt.points_list()[1], t[1]) and torch.equal(pt.normals_list()[1], n[1])
    (gt,) = torch.autograd.grad(pt.points_packed().sum(), t)
    assert torch.equal(gt, torch.ones_like(t))
    moved = pt.to(torch.device("cpu"))
    assert len(moved) == 2 and torch.equal(moved.points_padded(), t) and pc.to("cpu").points_list()[2].shape == (6, 3)
    assert Pointclouds([a]).normals_packed() is None and Pointclouds([torch.zeros((0, 3))]).points_packed().shape == (0, 3)


@pytest.mark.parametrize("name", ["triangle", "fan3", "batch2", "sphere_642"])
def test_edge_end_csr_and_primitive_tables(name):
    verts, faces = case(name)
    mesh = Meshes(verts, faces)
    topo = mesh._topo
    edges = torch.tensor(brute_edges(packed(verts, faces)[1]))
    start, ends = topo.edge_end_csr()
    assert topo.edge_end_csr()[0] is start  # cached
    assert start.shape == (sum(v.shape[0] for v in verts) + 1,) and ends.shape == (2 * edges.shape[0],)
    flat = edges.reshape(-1)
    for v in range(start.shape[0] - 1):
        row = ends[start[v]:start[v + 1]]
        assert row.tolist() == (flat == v).nonzero()[:, 0].tolist(), v  # every end of v, ascending
    for kind in C.KINDS:
        tab = topo.prim_tables(kind)
        per_mesh = C.prims_of(verts, faces, kind)
        assert topo.prim_tables(kind) is tab
        assert tab["counts"] == [p.shape[0] for p in per_mesh] == tab["count"].tolist()
        assert tab["first"].tolist() == [sum(tab["counts"][:i]) for i in range(len(verts))]
        off = torch.tensor([0] + [v.shape[0] for v in verts]).cumsum(0)
        assert torch.equal(tab["prims"], torch.cat([p + off[i] for i, p in enumerate(per_mesh)]))
        w = topo.prim_loss_weights(kind)
        assert w is topo.prim_loss_weights(kind) and w.sum().item() == pytest.approx(1.0, rel=1e-5)


def test_exports_and_shims():
    from pytorch3d.loss import point_mesh_edge_distance, point_mesh_face_distance
    from pytorch3d.structures import Pointclouds as P3DPointclouds
    assert point_mesh_face_distance is L.point_mesh_face_distance and point_mesh_edge_distance is L.point_mesh_edge_distance
    assert P3DPointclouds is Pointclouds is renderer.Pointclouds
    for name in ("Pointclouds", "point_mesh_face_distance", "point_mesh_edge_distance"):
        assert name in renderer.__all__ and hasattr(renderer, name)

"""The mesh regularisers' torch composition (renderer/loss.py on CPU tensors) against the dense
float64 restatement of their formulas (mesh_loss_cases.py), and against the per-call code the
cached version replaced.

The edge loss's torch composition keeps its global mean over all edges; that equals the per-mesh
definition whenever the meshes have equal edge counts (every single mesh), so on the two-mesh
batch with different counts it is held to the restatement of the global mean and the per-mesh
definition is the native kernels' (tests/test_gpu_mesh_losses.py)."""
import pytest
import torch

from conftest import assert_close
from mesh_loss_cases import LOSS_CASES_CPU, case, packed, ref_edge, ref_laplacian, rel_err
from pertrenderer_amd.renderer import Meshes
from pertrenderer_amd.renderer import loss as L

METHODS = ["uniform", "cot", "cotcurv"]


def _run(fn, verts, faces, dtype=torch.float64):
    """(loss, d loss / d packed verts) of a loss.py function on a CPU mesh."""
    vs = [v.to(dtype).requires_grad_(True) for v in verts]
    out = fn(Meshes(vs, [f.clone() for f in faces]))
    return out.detach(), torch.cat(torch.autograd.grad(out, vs))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", LOSS_CASES_CPU)
def test_laplacian_matches_dense_restatement(name, method):
    verts, faces = case(name)
    want, gwant = ref_laplacian(verts, faces, method)
    got, ggot = _run(lambda m: L.mesh_laplacian_smoothing(m, method), verts, faces)
    assert_close(got, want, name="loss")
    assert rel_err(ggot, gwant) <= 1e-9  # float64 against float64
    # float32 inputs take the same composition: loss at the fp32 bar
    got32, _ = _run(lambda m: L.mesh_laplacian_smoothing(m, method), verts, faces, torch.float32)
    assert got32.dtype == torch.float32
    assert_close(got32, want, name="loss fp32")


@pytest.mark.parametrize("target", [0.0, 0.3])
@pytest.mark.parametrize("name", LOSS_CASES_CPU)
def test_edge_loss_matches_dense_restatement(name, target):
    verts, faces = case(name)
    want, gwant = ref_edge(verts, faces, target, per_mesh=name != "batch2")
    got, ggot = _run(lambda m: L.mesh_edge_loss(m, target), verts, faces)
    assert_close(got, want, name="loss")
    assert rel_err(ggot, gwant) <= 1e-9


# ---- the code at the parent commit (per-call unique / argsort), restated
def _old_edges(f):
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    e, _ = e.sort(dim=1)
    return torch.unique(e, dim=0)


def _old_uniform(verts, faces):
    v, f = packed(verts, faces)
    V = v.shape[0]
    e = _old_edges(f)
    deg = torch.zeros(V, dtype=v.dtype)
    deg.index_add_(0, e[:, 0], torch.ones(e.shape[0], dtype=v.dtype))
    deg.index_add_(0, e[:, 1], torch.ones(e.shape[0], dtype=v.dtype))
    s = torch.zeros_like(v)
    s.index_add_(0, e[:, 0], v[e[:, 1]])
    s.index_add_(0, e[:, 1], v[e[:, 0]])
    lap = s / deg.clamp(min=1.0)[:, None] - v
    nv = torch.tensor([x.shape[0] for x in verts])
    w = (1.0 / nv.to(torch.float32))[torch.repeat_interleave(torch.arange(len(nv)), nv)]
    return (lap.norm(dim=1) * w).sum() / len(nv)


def _old_edge(verts, faces, target):
    v, f = packed(verts, faces)
    e = _old_edges(f)
    return ((v[e[:, 0]] - v[e[:, 1]]).norm(dim=1) - target).pow(2).mean()


def _old_normal_consistency(verts, faces):
    v, f = packed(verts, faces)
    n = torch.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]], dim=1)
    n = torch.nn.functional.normalize(n, dim=1, eps=1e-6)
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0).sort(dim=1).values
    fid = torch.arange(f.shape[0]).repeat(3)
    key = e[:, 0] * (v.shape[0] + 1) + e[:, 1]
    order = key.argsort()
    k, fo = key[order], fid[order]
    same = k[1:] == k[:-1]
    if not bool(same.any()):
        return v.sum() * 0.0
    a, b = fo[:-1][same], fo[1:][same]
    return (1.0 - (n[a] * n[b]).sum(dim=1)).mean()


@pytest.mark.parametrize("name", LOSS_CASES_CPU)
def test_values_unchanged_from_the_per_call_code(name):
    verts, faces = case(name)
    m = Meshes([v.clone() for v in verts], [f.clone() for f in faces])
    assert_close(L.mesh_laplacian_smoothing(m), _old_uniform(verts, faces), name="uniform")
    assert_close(L.mesh_laplacian_smoothing(m, "uniform"), _old_uniform(verts, faces), name="uniform")
    assert_close(L.mesh_edge_loss(m, 0.2), _old_edge(verts, faces, 0.2), name="edge")  # the global mean, batch too
    assert_close(L.mesh_normal_consistency(m), _old_normal_consistency(verts, faces), name="normal consistency")


def test_normal_consistency_without_shared_edges_is_a_differentiable_zero():
    verts, faces = case("triangle")
    got, g = _run(L.mesh_normal_consistency, verts, faces)
    assert got.item() == 0.0 and torch.equal(g, torch.zeros_like(g))


def test_bad_method_raises_value_error():
    verts, faces = case("tetrahedron")
    with pytest.raises(ValueError):
        L.mesh_laplacian_smoothing(Meshes(verts, faces), "cotangent")


@pytest.mark.parametrize("method", METHODS)
def test_zero_area_face_gives_finite_loss_and_gradient(method):
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.3, 1.0, 0.2]])  # 0, 1, 2 collinear
    f = torch.tensor([[0, 1, 2], [0, 1, 3]])
    for dtype in (torch.float32, torch.float64):
        loss, g = _run(lambda m: L.mesh_laplacian_smoothing(m, method), [v], [f], dtype)
        assert torch.isfinite(loss) and torch.isfinite(g).all()
    loss, g = _run(lambda m: L.mesh_edge_loss(m, 0.1), [torch.zeros((3, 3))], [torch.tensor([[0, 1, 2]])])
    assert torch.isfinite(loss) and torch.isfinite(g).all()  # zero-length edges

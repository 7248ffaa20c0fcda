"""Native vertex normals (pr_vert_normals_fwd/bwd behind Meshes.verts_normals_packed) against the
torch composition of PyTorch3D's formula (three corner crosses index-added per vertex, then
F.normalize with eps 1e-6): forward and the gradient of a random linear functional, on the
reference's sphere and cube meshes and on a mesh with an isolated vertex (zero normal)."""
import os

import numpy as np
import pytest
import torch

import pose_cases as pc
from conftest import ROOT, assert_close
from pertrenderer_amd import host_layer
from pertrenderer_amd.renderer import Meshes, load_obj
from pertrenderer_amd.renderer import mesh as mesh_mod

pytestmark = pytest.mark.gpu


def _both(verts, faces):
    out, keep = [], mesh_mod.NATIVE_NORMALS
    for native in (True, False):
        mesh_mod.NATIVE_NORMALS = native
        try:
            v = verts.clone().requires_grad_(True)
            n = Meshes([v], [faces]).verts_normals_packed()
            g = torch.randn(n.shape, generator=torch.Generator().manual_seed(5)).to(n.device)
            (gv,) = torch.autograd.grad((n * g).sum(), v)
            out.append((n.detach(), gv))
        finally:
            mesh_mod.NATIVE_NORMALS = keep
    return out


@pytest.mark.parametrize("name", ["sphere_642.obj", "cube2.obj"])
def test_native_normals_match_torch(name, device):
    verts, faces, _ = load_obj(os.path.join(ROOT, "tests", "golden", name))
    v = (verts * torch.tensor([1.0, 0.7, 1.3])).to(device)  # non-uniform scale: uneven face areas
    (n1, g1), (n0, g0) = _both(v, faces.verts_idx.to(device))
    assert_close(n1, n0, name="normals")
    assert_close(g1, g0, name="d verts")


def test_isolated_vertex_has_zero_normal_and_gradient(device):
    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], device=device)
    f = torch.tensor([[0, 1, 2]], device=device)
    (n1, g1), (n0, g0) = _both(v, f)
    torch.testing.assert_close(n1, n0, rtol=1e-6, atol=1e-7)
    assert torch.equal(n1[3], torch.zeros(3, device=device))
    torch.testing.assert_close(g1, g0, rtol=1e-5, atol=1e-6)


# ---- float64 parity (tests/pose_cases.py): the CSR path through Meshes on both autograd layers, the
# atomic path (no corner CSR) through the C ABI
CASES = ["sphere", "cube", "batch", "exact"]


@pytest.fixture(params=pc.LAYERS)
def layer(request):
    with pc.autograd_layer(request.param) as ok:
        if not ok:
            pytest.skip(f"C++ autograd layer not built: {host_layer.error()}")
        yield request.param


@pytest.fixture(scope="module")
def refs():
    return {name: pc.normals_ref(*pc.mesh_case(name)) for name in CASES}


def _csr_path(vs, fs, g, device):
    leaves = [v.to(device).requires_grad_(True) for v in vs]
    n = Meshes(leaves, [f.to(device) for f in fs]).verts_normals_packed()
    gv = torch.autograd.grad((n * g.to(device)).sum(), leaves)
    return n.detach(), torch.cat(gv, 0)


def _atomic_path(vs, fs, g, device):
    """pr_vert_normals_fwd / _bwd with vert_corner_start = vert_corners = NULL: face_cross, normalize,
    normalize_bwd and face_cross_bwd (float atomics)."""
    from pertrenderer_amd import _native as nat
    v64, f = pc.pack(vs, fs)
    v, f, gn = v64.to(torch.float32).to(device), f.to(device).contiguous(), g.to(device).contiguous()
    n, raw, graw, gv = (torch.full_like(v, float("nan")) for _ in range(4))
    a = nat.PRNormalsArgs()
    a.verts, a.faces, a.V, a.F = nat.ptr(v), nat.ptr(f) if f.numel() else None, v.shape[0], f.shape[0]
    a.normals, a.raw = nat.ptr(n), nat.ptr(raw)
    nat.call("pr_vert_normals_fwd", "pr_vert_normals_fwd", v, a)
    a.grad_normals, a.grad_raw, a.grad_verts = nat.ptr(gn), nat.ptr(graw), nat.ptr(gv)
    nat.call("pr_vert_normals_bwd", "pr_vert_normals_bwd", v, a)
    torch.cuda.synchronize()
    return n, gv


def _check_case(name, n, gv, refs):
    vs, fs, g = pc.mesh_case(name)
    rn, rg = refs[name]
    assert_close(n, rn, name=name + " normals")
    assert_close(gv, rg, name=name + " d verts")
    n, gv = n.cpu().numpy(), gv.cpu().numpy()
    if name == "batch":
        (s0, s1), (c0, c1), (t0, t1) = pc.batch_ranges(vs)
        assert np.array_equal(n[c1 - 1], np.zeros(3)) and np.array_equal(gv[c1 - 1], np.zeros(3))  # isolated
        # the 1e-4 sphere (F.normalize's clamp branch) against its own maxima, not the batch's
        assert_close(n[t0:t1], rn[t0:t1], name="clamped normals")
        assert_close(gv[t0:t1], rg[t0:t1], name="clamped d verts")
        assert 1e-4 < np.abs(rn[t0:t1]).max() < 1e-2 and 50 < np.abs(rg[t0:t1]).max() < 1000
    if name == "exact":
        pair = list(pc.C_PAIR)
        assert np.array_equal(n[pair], np.zeros((3, 3))), n[pair]
        assert np.array_equal(gv[pair], np.zeros((3, 3))), gv[pair]


@pytest.mark.parametrize("name", CASES)
def test_normals_csr_path_matches_float64(name, layer, device, refs):
    vs, fs, g = pc.mesh_case(name)
    n, gv = _csr_path(vs, fs, g, device)
    _check_case(name, n, gv, refs)
    n2, gv2 = _csr_path(vs, fs, g, device)  # gathers in a fixed order: bitwise the same again
    assert torch.equal(n, n2) and torch.equal(gv, gv2)


@pytest.mark.parametrize("name", CASES)
def test_normals_atomic_path_matches_float64(name, device, refs):
    n, gv = _atomic_path(*pc.mesh_case(name), device)
    _check_case(name, n, gv, refs)


def test_normals_without_faces(layer, device):
    """V > 0, F = 0: zero normals and a zero gradient, through Meshes and through the C ABI."""
    v = torch.rand((5, 3), generator=torch.Generator().manual_seed(1))
    f = torch.zeros((0, 3), dtype=torch.int64)
    g = torch.ones(5, 3)
    for n, gv in (_csr_path([v], [f], g, device), _atomic_path([v], [f], g, device)):
        assert torch.equal(n, torch.zeros(5, 3, device=device)) and torch.equal(gv, torch.zeros(5, 3, device=device))

"""sample_points_from_meshes on the CPU: the torch composition (renderer/ops.py
_sample_points_torch) in float32 against itself in float64 from the uniforms of the documented
Philox layout (seed 1234, oracle/philox_ref.py), the distribution of the picks, the exact dyadic
grid, and the public function's argument checks, dead rows, shim and seeding.

Measured on the CPU (printed by the tests).  Composition, sphere_cube: picks identical at S = 257
and S = 5000; vertex gradient float32 against float64, max-abs over max-abs, 1.7e-07 at S = 257 and
6.9e-07 at S = 5000.  Distribution (chi^2 / dof / bound dof + 6 sqrt(2 dof)): sphere 1369 / 1279 /
1582 at S = 257 and 1236 / 1279 / 1582 at S = 5000; cube 9.8 and 11.8 / 11 / 39.  Dyadic grid (the
four zero-area faces listed in sample_points_cases.py give F = 128 + 1 + 4 = 133), total 9.0, the
float32 and float64 tables bitwise equal, 0 mismatching picks at S = 4096."""
import math

import pytest
import torch

from conftest import assert_close
from mesh_loss_cases import rel_err
from sample_points_cases import (BIG_FACE, DEGENERATE, LAST_LIVE, SEED, chi_square, face_areas, mesh, meshes,
                                 philox_uniforms, reference, uniforms)
from pertrenderer_amd import noise
from pertrenderer_amd.renderer import ops


def test_torch_philox_matches_the_reference_generator():
    for N, S, seed in ((2, 257, SEED), (1, 5, 2 ** 62 - 3), (3, 1, 0)):
        assert torch.equal(ops._philox_uniforms(seed, N, S, "cpu"), philox_uniforms(N, S, seed))
    u = philox_uniforms(2, 5000)
    assert u.min() > 0 and u.max() < 1


@pytest.mark.parametrize("S", [257, 5000])
def test_composition_float32_against_float64(S):
    r32, r64 = reference("sphere_cube", S, torch.float32), reference("sphere_cube", S)
    assert r32["samples"].dtype == torch.float32 and r32["face"].dtype == torch.int64
    assert torch.equal(r32["face"], r64["face"])
    assert_close(r32["cdf"], r64["cdf"], name="cdf")
    assert_close(r32["samples"], r64["samples"], name="samples")
    assert_close(r32["normals"], r64["normals"], name="normals")
    assert_close(r32["w"], r64["w"], name="w")
    err = rel_err(r32["grad"], r64["grad"])
    print(f"S={S}: vertex gradient float32 vs float64 {err:.2e}")
    # a vertex sums the terms of its ~6 faces' samples (about 25 x 3 at S = 5000), each within a few
    # float32 roundings (6e-8) of float64: below 1e-5, the floor of the mesh losses' gradient rule
    assert err <= 1e-5
    # every point lies on its face's plane and every normal is the face's unit normal
    v = torch.cat(mesh("sphere_cube")[0]).double()
    f = torch.cat([mesh("sphere_cube")[1][0], mesh("sphere_cube")[1][1] + mesh("sphere_cube")[0][0].shape[0]])
    fv = v[f[r64["face"]]]
    assert ((r64["samples"] - fv[..., 0, :]) * r64["normals"]).sum(-1).abs().max() < 1e-12
    assert_close(r64["normals"].norm(dim=-1), torch.ones(r64["face"].shape, dtype=torch.float64), name="|n|")
    assert (r64["w"] >= 0).all()
    assert_close(r64["w"].sum(-1), torch.ones(r64["face"].shape, dtype=torch.float64), name="sum w")


@pytest.mark.parametrize("S", [257, 5000])
def test_picks_follow_the_areas(S):
    face, areas = reference("sphere_cube", S, torch.float32)["face"], face_areas("sphere_cube")
    first = 0
    for n, f in enumerate(mesh("sphere_cube")[1]):
        nf = f.shape[0]
        assert (face[n] >= first).all() and (face[n] < first + nf).all()
        chi, dof = chi_square(face[n], areas, first, nf, S)
        bound = dof + 6.0 * math.sqrt(2.0 * dof)
        print(f"mesh {n} S={S}: chi^2 {chi:.1f} dof {dof} bound {bound:.0f}")
        assert chi < bound
        first += nf


def test_dyadic_grid_is_exact():
    S = 4096
    r32, r64 = reference("dyadic", S, torch.float32), reference("dyadic", S)
    assert r32["cdf"].shape == (133,) and r32["cdf"][-1].item() == 9.0
    assert torch.equal(r32["cdf"], r64["cdf"].float()) and torch.equal(r32["cdf"].double(), r64["cdf"])
    assert torch.equal(r32["face"], r64["face"])  # every sample, no exclusions
    face = r32["face"][0]
    assert not any((face == d).any() for d in DEGENERATE)
    assert face[0].item() == 0 and face[2].item() == LAST_LIVE and face[1].item() in (LAST_LIVE - 1, LAST_LIVE)
    share = (face == BIG_FACE).double().mean().item()
    assert abs(share - 8.0 / 9.0) < 0.02, share
    assert_close(r32["samples"], r64["samples"], name="samples")
    assert_close(r32["normals"], r64["normals"], name="normals")
    chi, dof = chi_square(face, face_areas("dyadic"), 0, 133, S)
    assert chi < dof + 6.0 * math.sqrt(2.0 * dof)


def test_dead_rows_are_zero_without_gradient():
    m = meshes("dead", requires_grad=True)
    S = 64
    p, nrm, face, w, _ = ops._sample_points_torch(m, philox_uniforms(4, S), True)
    assert (face[1] == -1).all() and (face[2] == -1).all() and (face[0] >= 0).all() and (face[3] >= 12 + 2).all()
    assert not p[1:3].any() and not nrm[1:3].any() and not w[1:3].any()
    got, gn = ops.sample_points_from_meshes(m, S, True, uniforms=philox_uniforms(4, S))
    assert torch.equal(got, p) and torch.equal(gn, nrm)
    grads = torch.autograd.grad(got.sum() + gn.sum(), m.verts_list(), allow_unused=True)
    assert grads[0].abs().sum() > 0 and grads[3].abs().sum() > 0
    assert all(g is None or not g.any() for g in grads[1:3])
    # a batch without any face
    from pertrenderer_amd.renderer import Meshes
    none = Meshes([torch.rand(3, 3)], [torch.zeros((0, 3), dtype=torch.int64)])
    assert not ops.sample_points_from_meshes(none, 5).any()


def test_argument_checks():
    from pertrenderer_amd.renderer import Meshes
    m = meshes("sphere_cube")
    with pytest.raises(ValueError):
        ops.sample_points_from_meshes(Meshes([], []), 4)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            ops.sample_points_from_meshes(m, bad)
    u = philox_uniforms(2, 8)
    for bad in (u[:1], u[:, :7], u[..., :2], u.double(), u.tolist()):
        with pytest.raises(ValueError):
            ops.sample_points_from_meshes(m, 8, uniforms=bad)
    with pytest.raises(ValueError):
        ops.sample_points_from_meshes(m, 8, uniforms=u, seed=3)
    for bad in (-1, 2 ** 64, 1.5):
        with pytest.raises(ValueError):
            ops.sample_points_from_meshes(m, 8, seed=bad)
    with pytest.raises(ValueError):
        ops.sample_points_from_meshes(Meshes([torch.zeros((3, 3), dtype=torch.int64)], [torch.tensor([[0, 1, 2]])]), 8)
    assert ops.sample_points_from_meshes(m, 8).shape == (2, 8, 3)
    p, n = ops.sample_points_from_meshes(m, 8, return_normals=True)
    assert p.shape == n.shape == (2, 8, 3)
    assert ops.sample_points_from_meshes(meshes("sphere_cube", dtype=torch.float64), 8).dtype == torch.float64


def test_shim_and_package_export_the_function():
    import pytorch3d.ops
    from pertrenderer_amd import renderer
    assert pytorch3d.ops.sample_points_from_meshes is ops.sample_points_from_meshes
    assert renderer.sample_points_from_meshes is ops.sample_points_from_meshes
    assert "sample_points_from_meshes" in renderer.__all__


def test_seeding():
    m = meshes("sphere_cube")
    S = 257
    want = reference("sphere_cube", S, torch.float32)
    # seed= is the documented Philox stream
    p, n = ops.sample_points_from_meshes(m, S, True, seed=SEED)
    assert torch.equal(p, want["samples"]) and torch.equal(n, want["normals"])
    assert not torch.equal(ops.sample_points_from_meshes(m, S, seed=SEED + 1), p)
    # the default key comes from torch's CPU generator
    torch.manual_seed(11)
    a = ops.sample_points_from_meshes(m, S)
    b = ops.sample_points_from_meshes(m, S)
    torch.manual_seed(11)
    assert torch.equal(ops.sample_points_from_meshes(m, S), a) and not torch.equal(a, b)
    torch.manual_seed(11)
    assert torch.equal(ops.sample_points_from_meshes(m, S, seed=noise.draw_key()), a)
    # the "torch" source: torch.rand((N,S,3)) through the injected path
    noise.set_noise_source("torch")
    try:
        torch.manual_seed(5)
        c = ops.sample_points_from_meshes(m, S)
        torch.manual_seed(5)
        u = torch.rand((2, S, 3))
    finally:
        noise.set_noise_source("philox")
    assert torch.equal(c, ops.sample_points_from_meshes(m, S, uniforms=u)) and not torch.equal(c, a)

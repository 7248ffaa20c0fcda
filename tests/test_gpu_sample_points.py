"""Native sample_points_from_meshes (csrc/pr_samplepoints.hip behind renderer/ops.py) on the GPU:
injected uniforms against the torch composition on the device (cdf, picks, points, normals), the
Philox mode against the injected run of the documented counter layout (oracle/philox_ref.py),
gradients against the composition's autograd in float64, bitwise reproducibility, and the
deformation step captured in a HIP graph with a DeviceSeed.

Shapes: the dyadic grid alone (exact in float32: picks must agree for every sample; face 60 holds
about 89 % of the samples, one backward segment far longer than a wave) and {sphere_642, cube}
together (two lengths in one launch, the sphere's 1280 faces are more than one scan chunk), at
S = 1, 257 and 5000, with and without normals; a batch with a face-less mesh and a zero-area mesh.

Tolerances.  cdf: rtol 1e-6.  Picks on the sphere batch: equal for every sample whose r = u0 total
lies farther than 1e-6 total from every entry of the composition's own table (the two tables differ
by float32 roundings of the areas); the other samples (below 1 %) pick the same or an index-adjacent
face.  Points, normals, weights of equal picks: conftest.assert_close's defaults.  Gradients: the
native max-abs error over max-abs may be 4x the float32 composition's own error against float64,
floored at 1e-5 (the rule of test_gpu_mesh_losses.py).

Measured on an MI355X (float32 composition error / native error, max-abs over max-abs):
sphere_cube S = 1 7.23e-08 / 8.83e-08, S = 257 1.63e-07 / 1.67e-07, S = 5000 5.53e-07 / 1.17e-07;
dyadic S = 5000 1.59e-06 / 9.13e-08; dead S = 257 3.56e-07 / 9.41e-08: the 1e-5 floor decides.
Picks within 1e-6 total of a table entry: 0 of 2, 0 of 514 and 10 of 10000 (0.1 %), none of which
differs from the composition's."""
import pytest
import torch

from conftest import assert_close
from mesh_loss_cases import rel_err
from sample_points_cases import (BIG_FACE, DEGENERATE, LAST_LIVE, SEED, cotangents, mesh, meshes, philox_uniforms,
                                 reference, uniforms)
from pertrenderer_amd import noise
from pertrenderer_amd.renderer import Meshes, ops
from pertrenderer_amd.renderer import loss as L

pytestmark = pytest.mark.gpu

SAMPLES = [1, 257, 5000]


def _native(m, S, normals, u=None, seed=None):
    """(samples, normals, face_idx, w, cdf) of the native op."""
    return ops._SamplePointsFn.apply(m.verts_packed(), m._topo, S, normals, seed, None, u)


def _composition(name, S, normals, device):
    with torch.no_grad():
        return ops._sample_points_torch(meshes(name, device), uniforms(name, S).to(device), normals)


def _check_rows(got, want, same, normals):
    p, n, _, w, _ = got
    assert p.dtype == w.dtype == torch.float32 and got[2].dtype == torch.int32
    assert_close(p[same], want[0][same], name="samples")
    assert_close(w[same], want[3][same], name="w")
    if normals:
        assert_close(n[same], want[1][same], name="normals")
    else:
        assert n is None


@pytest.mark.parametrize("normals", [True, False], ids=["normals", "points"])
@pytest.mark.parametrize("S", SAMPLES)
def test_dyadic_grid_matches_composition_exactly(S, normals, device):
    want = _composition("dyadic", S, normals, device)
    got = _native(meshes("dyadic", device), S, normals, uniforms("dyadic", S).to(device))
    assert torch.equal(got[4], want[4]) and got[4][-1].item() == 9.0  # the table: exact sums
    assert torch.equal(got[4].cpu(), reference("dyadic", S)["cdf"].float())
    face = got[2].long()
    assert torch.equal(face, want[2])  # every sample, no exclusions
    assert torch.equal(face.cpu(), reference("dyadic", S)["face"])
    assert not any((face == d).any() for d in DEGENERATE)
    if S >= 3:  # u0 = 2^-24, 1 - 2^-24, 1.0
        assert face[0, 0].item() == 0 and face[0, 2].item() == LAST_LIVE and face[0, 1].item() >= LAST_LIVE - 1
    if S == 5000:
        assert abs((face == BIG_FACE).float().mean().item() - 8.0 / 9.0) < 0.02
    _check_rows(got, want, torch.ones_like(face, dtype=torch.bool), normals)


@pytest.mark.parametrize("normals", [True, False], ids=["normals", "points"])
@pytest.mark.parametrize("S", SAMPLES)
def test_sphere_batch_matches_composition(S, normals, device):
    want = _composition("sphere_cube", S, normals, device)
    u = uniforms("sphere_cube", S).to(device)
    got = _native(meshes("sphere_cube", device), S, normals, u)
    assert_close(got[4], want[4], rtol=1e-6, atol_rel=0.0, name="cdf")
    face, cface, cdf = got[2].long(), want[2], want[4]
    near = torch.zeros_like(face, dtype=torch.bool)
    first = 0
    for n, f in enumerate(mesh("sphere_cube")[1]):
        nf = f.shape[0]
        c = cdf[first:first + nf]
        r = u[n, :, 0] * c[-1]
        near[n] = ((r[:, None] - c[None, :]).abs().min(dim=1).values <= 1e-6 * c[-1])
        assert (face[n] >= first).all() and (face[n] < first + nf).all()
        first += nf
    share = near.float().mean().item()
    print(f"S={S}: {int(near.sum())} of {near.numel()} picks within 1e-6 total of a table entry, "
          f"{int((face != cface)[near].sum())} of them differ")
    assert share < 0.01
    assert torch.equal(face[~near], cface[~near])
    assert ((face - cface).abs() <= 1).all()
    _check_rows(got, want, face == cface, normals)


def test_dead_rows(device):
    S = 257
    m = meshes("dead", device, requires_grad=True)
    u = philox_uniforms(4, S).to(device)
    got = _native(m, S, True, u)
    with torch.no_grad():
        want = ops._sample_points_torch(meshes("dead", device), u, True)
    face = got[2].long()
    assert (face[1] == -1).all() and (face[2] == -1).all() and torch.equal(face, want[2])
    for t in (got[0], got[1], got[3]):
        assert not t[1:3].any()
    _check_rows(got, want, torch.ones_like(face, dtype=torch.bool), True)
    grads = torch.autograd.grad(got[0].sum() + got[1].sum(), m.verts_list())
    assert grads[0].abs().sum() > 0 and grads[3].abs().sum() > 0 and not grads[1].any() and not grads[2].any()


@pytest.mark.parametrize("name,S", [("sphere_cube", 1), ("sphere_cube", 5000), ("dyadic", 257)])
def test_philox_mode_reproduces_the_documented_stream(name, S, device):
    m = meshes(name, device)
    inj = _native(m, S, True, philox_uniforms(len(m), S).to(device))
    phi = _native(m, S, True, None, SEED)
    assert torch.equal(phi[2], inj[2]) and torch.equal(phi[3], inj[3])  # picks and weights, bitwise
    assert torch.equal(phi[0], inj[0]) and torch.equal(phi[1], inj[1])
    pub = ops.sample_points_from_meshes(m, S, True, seed=SEED)
    assert torch.equal(pub[0], inj[0]) and torch.equal(pub[1], inj[1])
    assert not torch.equal(_native(m, S, True, None, SEED + 1)[3], inj[3])


def _native_grad(name, S, device, with_normals=True):
    m = meshes(name, device, requires_grad=True)
    gs, gn = (t.to(device) for t in cotangents(len(m), S))
    p, n, face, _, _ = _native(m, S, with_normals, uniforms(name, S).to(device))
    out = (p * gs).sum() + ((n * gn).sum() if with_normals else 0.0)
    return torch.cat(torch.autograd.grad(out, m.verts_list())), face.long().cpu()


@pytest.mark.parametrize("name,S", [("sphere_cube", 1), ("sphere_cube", 257), ("sphere_cube", 5000), ("dyadic", 5000),
                                    ("dead", 257)])
def test_gradients_match_float64(name, S, device):
    """d (sum samples . g_s + sum normals . g_n) / d verts against the composition's autograd in
    float64.  On "dyadic" face 60 holds about 89 % of the samples (a segment of ~4450 entries for
    one wave); "dead" has rows without a face."""
    want, own = reference(name, S), reference(name, S, torch.float32)
    e32 = rel_err(own["grad"], want["grad"])
    grad, face = _native_grad(name, S, device)
    err = rel_err(grad, want["grad"])
    print(f"{name} S={S}: gradient error composition(fp32) {e32:.2e}, native {err:.2e}")
    assert torch.equal(face, want["face"])  # the same picks: the gradients are comparable
    assert err <= max(4.0 * e32, 1e-5), (err, e32)
    if name == "dead":
        nv = [v.shape[0] for v in mesh(name)[0]]
        assert not grad[nv[0]:nv[0] + nv[1] + nv[2]].any()
    # samples alone (no grad_normals): the float64 composition without the normals' term
    m64 = meshes(name, dtype=torch.float64, requires_grad=True)
    p = ops._sample_points_torch(m64, uniforms(name, S))[0]
    ref = torch.autograd.grad((p * cotangents(len(m64), S)[0].double()).sum(), m64.verts_list(), allow_unused=True)
    ref = torch.cat([torch.zeros_like(v) if g is None else g for g, v in zip(ref, m64.verts_list())])
    assert rel_err(_native_grad(name, S, device, False)[0], ref) <= max(4.0 * e32, 1e-5)


def test_native_calls_are_bitwise_reproducible(device):
    for name in ("sphere_cube", "dyadic"):
        runs = []
        for _ in range(2):
            m = meshes(name, device, requires_grad=True)
            p, n, face, w, cdf = _native(m, 5000, True, None, 99)
            g = torch.autograd.grad((p * p).sum() + (n[..., 0] * p[..., 1]).sum(), m.verts_list())
            runs.append((p.detach(), n.detach(), face, w, cdf) + tuple(g))
        assert all(torch.equal(a, b) for a, b in zip(*runs)), name


def test_raw_op_refuses_cpu_tensors_and_bad_uniforms(device):
    from pertrenderer_amd import _native as nat
    m = meshes("sphere_cube")
    with pytest.raises(nat.NativeError):
        _native(m, 4, False, None, 1)
    with pytest.raises(ValueError):
        _native(meshes("sphere_cube", device), 4, False, torch.rand((2, 5, 3), device=device))
    with pytest.raises(ValueError):
        ops.sample_points_from_meshes(meshes("sphere_cube", device), 4, uniforms=torch.rand((2, 4, 3)))


def test_torch_source_and_composition_switch(device):
    m = meshes("sphere_cube", device)
    noise.set_noise_source("torch")
    try:
        torch.manual_seed(3)
        a = ops.sample_points_from_meshes(m, 257)
        torch.manual_seed(3)
        u = torch.rand((2, 257, 3), device=device)
    finally:
        noise.set_noise_source("philox")
    assert torch.equal(a, ops.sample_points_from_meshes(m, 257, uniforms=u))
    keep = L.NATIVE_MESHLOSS
    L.NATIVE_MESHLOSS = False  # the composition on the device, from the same Philox stream
    try:
        c = ops.sample_points_from_meshes(m, 257, seed=SEED)
    finally:
        L.NATIVE_MESHLOSS = keep
    n = ops.sample_points_from_meshes(m, 257, seed=SEED)
    assert_close(n, c, name="samples")


def test_deformation_step_is_captured_in_a_graph(device):
    """sample -> Chamfer with normals + edge + normal consistency + Laplacian -> backward in one
    captured graph with a DeviceSeed, after one warm-up call: every replay draws fresh samples, the
    last replay equals an eager step with the same key base bitwise, and the capture meets no host
    synchronisation (torch's sync debug mode raises on one; so does the capture itself)."""
    v, f = mesh("sphere_cube")
    base = Meshes([v[0].to(device)], [f[0].to(device)])
    g = torch.Generator().manual_seed(5)
    tgt = torch.randn((1, 700, 3), generator=g)
    tgt = (1.1 * tgt / tgt.norm(dim=2, keepdim=True) + 0.1).to(device)
    tgt_n = torch.nn.functional.normalize(tgt - 0.1, dim=2)
    start = (0.02 * torch.randn(v[0].shape, generator=g)).to(device)
    S = 1000

    def step(deform):
        m = base.offset_verts(deform)
        p, n = ops.sample_points_from_meshes(m, S, return_normals=True)
        cd, cn = L.chamfer_distance(p, tgt, x_normals=n, y_normals=tgt_n)
        loss = (cd + 0.1 * cn + L.mesh_edge_loss(m) + 0.01 * L.mesh_normal_consistency(m)
                + 0.1 * L.mesh_laplacian_smoothing(m, "uniform"))
        loss.backward()
        return p.detach(), loss.detach()

    ds = noise.DeviceSeed(device, seed=4242)
    noise.use_device_seed(ds)
    try:
        d = start.clone().requires_grad_(True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # the one call before the capture: caches, autograd warm-up
            ds.advance()
            step(d)
        torch.cuda.current_stream().wait_stream(side)
        d.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            torch.cuda.set_sync_debug_mode("error")
            try:
                ds.advance()
                p, loss = step(d)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        outs, grads, bases = [], [], []
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            outs.append(p.clone())
            grads.append(d.grad.clone())
            bases.append(int(ds.tensor.item()))
        assert bases[0] != bases[1] and not torch.equal(outs[0], outs[1])
        # an eager step with the last replay's base (the stream id is 1 again)
        eager = noise.DeviceSeed(device, seed=0)
        eager.tensor.fill_(bases[-1])
        noise.use_device_seed(eager)
        d2 = start.clone().requires_grad_(True)
        p2, loss2 = step(d2)
        assert torch.equal(p2, outs[-1]) and torch.equal(loss2, loss) and torch.equal(d2.grad, grads[-1])
        assert d2.grad.abs().sum() > 0
    finally:
        noise.use_device_seed(None)

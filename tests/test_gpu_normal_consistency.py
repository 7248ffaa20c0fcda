"""Native mesh_normal_consistency (pr_mesh_normal_consistency_fwd/bwd behind renderer/loss.py) on the
GPU: value and d verts against the float64 run of the torch composition, against the composition
on the device (NATIVE_MESHLOSS = False), bitwise reproducibility, the P = 0 case, and the launch
count of one forward + backward.

Tolerances, as in test_gpu_mesh_losses.py.  Loss: conftest.assert_close's defaults.  Gradient: each
case measures the float32 composition's own error against its float64 run (max-abs over max-abs,
on the CPU) and allows the native result 4x that, floored at 1e-5.

Measured on an MI355X (float32 composition error / native error, max-abs over max-abs):
    sphere_642 7.24e-06 / 7.57e-06, hub70 9.24e-07 / 1.13e-06, grid3 8.15e-07 / 9.94e-07,
    tetrahedron 2.73e-07 / 3.03e-07, batch2 2.71e-07 / 3.50e-07, fan3 1.04e-07 / 6.47e-08,
    sliver 9.92e-08 / 6.89e-08.
The native error is 0.6x to 1.3x the composition's own; loss values agree with float64 to 3.3e-06
relative (grid3; sphere_642 1.4e-06, every other case 3e-07 or better)."""
import functools
import json

import pytest
import torch

from conftest import assert_close
from mesh_loss_cases import LOSS_CASES_GPU, case, rel_err
from pertrenderer_amd import _native as nat
from pertrenderer_amd.renderer import Meshes
from pertrenderer_amd.renderer import loss as L

pytestmark = pytest.mark.gpu

# face 0 has |c| = 5.1e-7 < 1e-6: its normal is c / 1e-6 and its gradient takes the clamped branch
_SLIVER = ([torch.tensor([[0.0, 0.0, 0.0], [1e-3, 0.0, 0.0], [2e-4, 5e-4, 1e-4], [0.5, -1.0, 0.2], [0.4, 0.8, 0.9]])],
           [torch.tensor([[0, 1, 2], [1, 0, 3], [1, 2, 4]])])
CASES = LOSS_CASES_GPU + ["sliver"]


def _case(name):
    return _SLIVER if name == "sliver" else case(name)


def _run(name, device, dtype=torch.float32, native=True):
    verts, faces = _case(name)
    keep = L.NATIVE_MESHLOSS
    L.NATIVE_MESHLOSS = native
    try:
        vs = [v.to(device=device, dtype=dtype).requires_grad_(True) for v in verts]
        out = L.mesh_normal_consistency(Meshes(vs, [f.to(device) for f in faces]))
        g = torch.cat(torch.autograd.grad(out, vs))
    finally:
        L.NATIVE_MESHLOSS = keep
    return out.detach(), g


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(loss64, grad64, the float32 composition's gradient error), on the CPU, once per case."""
    loss64, g64 = _run(name, "cpu", torch.float64)
    _, g32 = _run(name, "cpu", torch.float32)
    return loss64, g64, rel_err(g32, g64)


def test_sliver_case_is_clamped():
    v, f = _SLIVER[0][0].double(), _SLIVER[1][0]
    c = torch.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]], dim=1).norm(dim=1)
    assert 0 < c[0] < 1e-6 and (c[1:] > 1e-3).all()


@pytest.mark.parametrize("name", CASES)
def test_native_matches_float64_composition(name, device):
    loss64, g64, ref_err = _reference(name)
    loss, g = _run(name, device)
    err = rel_err(g, g64)
    print(f"{name}: loss {loss.item():.8e} vs {loss64.item():.8e}; gradient error "
          f"composition(fp32) {ref_err:.2e} native {err:.2e}")
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert_close(loss, loss64, name="loss")
    if name == "triangle":  # P = 0: a differentiable zero, nothing launched
        assert loss.item() == 0.0 and torch.equal(g, torch.zeros_like(g))
        return
    assert err <= max(4.0 * ref_err, 1e-5), (err, ref_err)


@pytest.mark.parametrize("name", CASES)
def test_native_matches_torch_composition(name, device):
    _, _, ref_err = _reference(name)
    loss, g = _run(name, device)
    loss_t, g_t = _run(name, device, native=False)
    assert_close(loss, loss_t, name="loss")
    if name != "triangle":
        assert rel_err(g, g_t) <= max(4.0 * ref_err, 1e-5)


def test_native_calls_are_bitwise_reproducible(device):
    for name in ("sphere_642", "batch2", "fan3"):
        a, b = _run(name, device), _run(name, device)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), name


def test_raw_op_refuses_cpu_tensors():
    verts, faces = case("tetrahedron")
    m = Meshes(verts, faces)
    with pytest.raises(nat.NativeError):
        L._NormalConsistencyFn.apply(m.verts_packed(), m._topo)


def test_forward_and_backward_take_at_most_8_launches(device, tmp_path):
    """3 kernels forward (face normals, pair gather, finalize) and 2 backward (faces, vertices); the
    cap leaves room for autograd's fill of the incoming gradient.  The composition takes ~100."""
    from torch.profiler import ProfilerActivity, profile
    verts, faces = case("sphere_642")
    v = verts[0].to(device).requires_grad_(True)
    m = Meshes([v], [faces[0].to(device)])
    L.mesh_normal_consistency(m).backward()  # topology caches, library load
    v.grad = None
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        L.mesh_normal_consistency(m).backward()
        torch.cuda.synchronize()
    tr = str(tmp_path / "nc.json")
    prof.export_chrome_trace(tr)
    names = [e.get("name", "") for e in json.load(open(tr))["traceEvents"]
             if e.get("ph") == "X" and e.get("cat") == "kernel"]
    print(len(names), names)
    for k in ("face_normal_kernel", "normal_pairs_kernel", "mesh_finalize_kernel", "normal_face_bwd_kernel",
              "normal_vert_bwd_kernel"):
        assert sum(k in n for n in names) == 1, (k, names)
    assert len(names) <= 8, names

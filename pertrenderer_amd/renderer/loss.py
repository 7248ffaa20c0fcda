"""PyTorch3D 0.4.0 mesh losses that experiments/eval.py imports (eval.py:26-31) and uses
in its vertex-deformation task (mesh_laplacian_smoothing, eval.py:455).

The index structures (unique edges, neighbour CSR, face pairs, per-vertex weights) come from the
mesh's cached topology record (mesh.py _Topology), so a call builds no index tensor and does not
synchronise: after one call a deformation step can be captured in a HIP graph.  On a ROCm device
with float32 vertices the Laplacian and the edge loss run on the native kernels
(csrc/pr_meshloss.hip: per-vertex CSR gathers, no atomics, bitwise reproducible);
PR_NATIVE_MESHLOSS=0 (or NATIVE_MESHLOSS = False), CPU tensors and other dtypes take the torch
composition of the same formulas.  Parity with PyTorch3D is unpinned (not installable here)."""
import os

import torch

# read at import, like mesh.NATIVE_NORMALS; tests/test_gpu_mesh_losses.py compares the two paths
NATIVE_MESHLOSS = os.environ.get("PR_NATIVE_MESHLOSS", "1") == "1"

_METHODS = {"uniform": 0, "cot": 1, "cotcurv": 2}


def _native(v):
    return NATIVE_MESHLOSS and v.is_cuda and v.dtype == torch.float32


def _vert_weights(meshes, dtype):
    """1/num_verts of the mesh a packed vertex belongs to (PyTorch3D's per-mesh averaging)."""
    nv = meshes.num_verts_per_mesh().to(dtype)
    return (1.0 / nv)[meshes._topo.mesh_of_vert()], len(meshes)


def _mesh_args(nat, v, topo):
    a = nat.PRMeshLossArgs()
    a.verts, a.V, a.F = nat.ptr(v), v.shape[0], topo.faces_packed().shape[0]
    return a


class _LaplacianFn(torch.autograd.Function):
    """verts -> the Laplacian smoothing loss (pr_mesh_laplacian_fwd/bwd) over the topology's cached
    CSRs.  The backward runs on the forward's saved per-vertex terms: once-differentiable."""

    @staticmethod
    def forward(ctx, verts, topo, method):
        from .. import _native as nat
        nat.require_device(verts)
        v = nat.dense(verts, torch.float32)
        a = _mesh_args(nat, v, topo)
        a.method = method
        a.weight = nat.ptr(topo.loss_weights("verts"))  # the topology record owns the index tensors
        cot = None
        if method == nat.PR_MESH_LAP_UNIFORM:
            a.nbr_start, a.nbr = (nat.ptr(t) for t in topo.neighbour_csr())
        else:
            cot = torch.empty((max(int(a.F), 1), 4), dtype=torch.float32, device=v.device)
            a.faces, a.face_cot = nat.ptr(topo.faces_packed()), nat.ptr(cot)
            a.vert_corner_start, a.vert_corners = (nat.ptr(t) for t in topo.corner_csr("gather"))
        gather, diag = torch.empty_like(v), torch.empty_like(v)
        part = torch.empty(nat.load().pr_mesh_loss_workspace(a.V), dtype=torch.float32, device=v.device)
        loss = torch.empty((), dtype=torch.float32, device=v.device)
        a.gather, a.diag, a.partials, a.loss = nat.ptr(gather), nat.ptr(diag), nat.ptr(part), nat.ptr(loss)
        nat.call("pr_mesh_laplacian_fwd", "pr_mesh_laplacian_fwd", v, a)
        ctx.save_for_backward(gather, diag)
        ctx.cot, ctx.topo, ctx.method = cot, topo, method
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from .. import _native as nat
        gather, diag = ctx.saved_tensors
        topo = ctx.topo
        gl = nat.dense(g, torch.float32)
        gv = torch.empty_like(gather)
        a = nat.PRMeshLossArgs()
        a.V, a.F, a.method = gather.shape[0], topo.faces_packed().shape[0], ctx.method
        if ctx.method == nat.PR_MESH_LAP_UNIFORM:
            a.nbr_start, a.nbr = (nat.ptr(t) for t in topo.neighbour_csr())
        else:
            a.faces, a.face_cot = nat.ptr(topo.faces_packed()), nat.ptr(ctx.cot)
            a.vert_corner_start, a.vert_corners = (nat.ptr(t) for t in topo.corner_csr("gather"))
        a.gather, a.diag, a.grad_loss, a.grad_verts = nat.ptr(gather), nat.ptr(diag), nat.ptr(gl), nat.ptr(gv)
        nat.call("pr_mesh_laplacian_bwd", "pr_mesh_laplacian_bwd", gather, a)
        return gv, None, None


class _EdgeLossFn(torch.autograd.Function):
    """verts -> the edge-length loss (pr_mesh_edge_fwd/bwd) over the cached neighbour CSR."""

    @staticmethod
    def _args(nat, v, topo, target):
        a = _mesh_args(nat, v, topo)
        a.target_length = target
        a.weight = nat.ptr(topo.loss_weights("edges"))
        a.nbr_start, a.nbr = (nat.ptr(t) for t in topo.neighbour_csr())
        return a

    @staticmethod
    def forward(ctx, verts, topo, target):
        from .. import _native as nat
        nat.require_device(verts)
        v = nat.dense(verts, torch.float32)
        a = _EdgeLossFn._args(nat, v, topo, target)
        part = torch.empty(nat.load().pr_mesh_loss_workspace(a.V), dtype=torch.float32, device=v.device)
        loss = torch.empty((), dtype=torch.float32, device=v.device)
        a.partials, a.loss = nat.ptr(part), nat.ptr(loss)
        nat.call("pr_mesh_edge_fwd", "pr_mesh_edge_fwd", v, a)
        ctx.save_for_backward(v)
        ctx.topo, ctx.target = topo, target
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from .. import _native as nat
        (v,) = ctx.saved_tensors
        gl = nat.dense(g, torch.float32)
        gv = torch.empty_like(v)
        a = _EdgeLossFn._args(nat, v, ctx.topo, ctx.target)
        a.grad_loss, a.grad_verts = nat.ptr(gl), nat.ptr(gv)
        nat.call("pr_mesh_edge_bwd", "pr_mesh_edge_bwd", v, a)
        return gv, None, None


def _cot_weights(v, f):
    """Per-face corner cotangents (3 x (F,)) and Heron areas (F,), constants of the backward."""
    with torch.no_grad():
        v0, v1, v2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        A, B, C = (v1 - v2).norm(dim=1), (v0 - v2).norm(dim=1), (v0 - v1).norm(dim=1)
        s = 0.5 * (A + B + C)
        area = (s * (s - A) * (s - B) * (s - C)).clamp(min=1e-12).sqrt()
        A2, B2, C2 = A * A, B * B, C * C
        d = 4.0 * area
        return ((B2 + C2 - A2) / d, (A2 + C2 - B2) / d, (A2 + B2 - C2) / d), area


def _laplacian_torch(meshes, method):
    v = meshes.verts_packed()
    topo = meshes._topo
    if method == "uniform":
        e = topo.edges_packed()
        start = topo.neighbour_csr()[0]
        deg = (start[1:] - start[:-1]).to(v.dtype)
        s = torch.zeros_like(v)
        s.index_add_(0, e[:, 0], v[e[:, 1]])
        s.index_add_(0, e[:, 1], v[e[:, 0]])
        lap = s / deg.clamp(min=1.0)[:, None] - v
    else:
        f = topo.faces_packed()
        cot, area = _cot_weights(v, f)
        # the cot at corner c weighs the edge opposite to it: (f1,f2), (f2,f0), (f0,f1)
        ii = torch.cat([f[:, 1], f[:, 2], f[:, 0]])
        jj = torch.cat([f[:, 2], f[:, 0], f[:, 1]])
        c = torch.cat(cot)
        s = torch.zeros_like(v).index_add_(0, ii, c[:, None] * v[jj]).index_add_(0, jj, c[:, None] * v[ii])
        r = torch.zeros(v.shape[0], dtype=v.dtype, device=v.device).index_add_(0, ii, c).index_add_(0, jj, c)
        if method == "cot":
            lap = s * torch.where(r > 0, 1.0 / r, r)[:, None] - v
        else:
            a = torch.zeros_like(r).index_add_(0, torch.cat([f[:, 0], f[:, 1], f[:, 2]]), area.repeat(3))
            lap = (s - r[:, None] * v) * (0.25 * torch.where(a > 0, 1.0 / a, a))[:, None]
    w, n = _vert_weights(meshes, v.dtype)
    return (lap.norm(dim=1) * w).sum() / n


def mesh_laplacian_smoothing(meshes, method="uniform"):
    """Laplacian smoothing, loss = mean over meshes of the per-mesh mean |l_i| with (PyTorch3D's
    methods) "uniform": l_i = mean of neighbours - v_i; "cot": l_i = sum_j L_ij v_j / r_i - v_i;
    "cotcurv": l_i = (sum_j L_ij v_j - r_i v_i) / (4 a_i), L the cotangent weights (constants of
    the backward), r_i their row sum, a_i the area sum of i's faces."""
    if method not in _METHODS:
        raise ValueError(f"method must be one of {sorted(_METHODS)}, got {method!r}")
    v = meshes.verts_packed()
    if _native(v):
        return _LaplacianFn.apply(v, meshes._topo, _METHODS[method])
    return _laplacian_torch(meshes, method)


def mesh_edge_loss(meshes, target_length=0.0):
    """mean over meshes of the per-mesh mean (|e| - target)^2 over unique edges."""
    v = meshes.verts_packed()
    if _native(v):
        return _EdgeLossFn.apply(v, meshes._topo, float(target_length))
    e = meshes._topo.edges_packed()
    return ((v[e[:, 0]] - v[e[:, 1]]).norm(dim=1) - target_length).pow(2).mean()


def mesh_normal_consistency(meshes):
    """mean over interior edges of 1 - cos(angle between the two adjacent face normals)."""
    v, f = meshes.verts_packed(), meshes.faces_packed()
    n = torch.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]], dim=1)
    n = torch.nn.functional.normalize(n, dim=1, eps=1e-6)
    a, b, npairs = meshes._topo.face_pairs()
    if npairs == 0:
        return v.sum() * 0.0
    return (1.0 - (n[a] * n[b]).sum(dim=1)).mean()


def chamfer_distance(x, y, batch_reduction="mean", point_reduction="mean"):
    """Symmetric squared Chamfer distance between point clouds (N,P,3) and (N,Q,3);
    returns (loss, None) like PyTorch3D (no normals)."""
    d = torch.cdist(x, y).pow(2)
    cx, cy = d.min(dim=2).values, d.min(dim=1).values
    red = (lambda t: t.mean(1)) if point_reduction == "mean" else (lambda t: t.sum(1))
    loss = red(cx) + red(cy)
    if batch_reduction == "mean":
        loss = loss.mean()
    elif batch_reduction == "sum":
        loss = loss.sum()
    return loss, None

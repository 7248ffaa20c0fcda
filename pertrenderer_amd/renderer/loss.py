"""PyTorch3D 0.4.0 mesh losses that experiments/eval.py imports (eval.py:26-31) and uses
in its vertex-deformation task (mesh_laplacian_smoothing, eval.py:455).

The index structures (unique edges, neighbour CSR, face pairs, per-vertex weights) come from the
mesh's cached topology record (mesh.py _Topology), so a call builds no index tensor and does not
synchronise: after one call a deformation step can be captured in a HIP graph.  On a ROCm device
with float32 inputs all four losses run on the native kernels (the Laplacian, the edge loss and
normal consistency in csrc/pr_meshloss.hip: per-vertex / per-face CSR gathers; chamfer_distance's
nearest neighbours in csrc/pr_chamfer.hip; no atomics, bitwise reproducible);
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


class _NormalConsistencyFn(torch.autograd.Function):
    """verts -> mesh_normal_consistency (pr_mesh_normal_consistency_fwd/bwd) over the cached face-pair
    CSR; needs at least one pair.  The backward runs on the forward's saved per-face terms."""

    @staticmethod
    def _args(nat, v, topo, fn, fs):
        a = nat.PRNormalConsistencyArgs()
        a.verts, a.faces = nat.ptr(v), nat.ptr(topo.faces_packed())
        a.V, a.F, a.P = v.shape[0], topo.faces_packed().shape[0], topo.face_pairs()[2]
        a.face_normal, a.face_sum = nat.ptr(fn), nat.ptr(fs)
        return a

    @staticmethod
    def forward(ctx, verts, topo):
        from .. import _native as nat
        nat.require_device(verts)
        v = nat.dense(verts, torch.float32)
        F = topo.faces_packed().shape[0]
        fn = torch.empty((F, 4), dtype=torch.float32, device=v.device)
        fs = torch.empty((F, 3), dtype=torch.float32, device=v.device)
        a = _NormalConsistencyFn._args(nat, v, topo, fn, fs)
        a.pair_start, a.pair_partner = (nat.ptr(t) for t in topo.face_pair_csr())
        part = torch.empty(nat.load().pr_mesh_loss_workspace(F), dtype=torch.float32, device=v.device)
        loss = torch.empty((), dtype=torch.float32, device=v.device)
        a.partials, a.loss = nat.ptr(part), nat.ptr(loss)
        nat.call("pr_mesh_normal_consistency_fwd", "pr_mesh_normal_consistency_fwd", v, a)
        ctx.save_for_backward(v, fn, fs)
        ctx.topo = topo
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from .. import _native as nat
        v, fn, fs = ctx.saved_tensors
        gl = nat.dense(g, torch.float32)
        fg, gv = torch.empty_like(fs), torch.empty_like(v)
        a = _NormalConsistencyFn._args(nat, v, ctx.topo, fn, fs)
        a.vert_corner_start, a.vert_corners = (nat.ptr(t) for t in ctx.topo.corner_csr("gather"))
        a.face_grad, a.grad_loss, a.grad_verts = nat.ptr(fg), nat.ptr(gl), nat.ptr(gv)
        nat.call("pr_mesh_normal_consistency_bwd", "pr_mesh_normal_consistency_bwd", v, a)
        return gv, None


def mesh_normal_consistency(meshes):
    """mean over interior edges of 1 - cos(angle between the two adjacent face normals): the global
    mean over the face pairs of the packed batch (_Topology.face_pairs), with
    n_f = c_f / max(|c_f|, 1e-6); not PyTorch3D's per-edge, orientation-free formula."""
    v, f = meshes.verts_packed(), meshes.faces_packed()
    a, b, npairs = meshes._topo.face_pairs()
    if npairs == 0:
        return v.sum() * 0.0
    if _native(v):
        return _NormalConsistencyFn.apply(v, meshes._topo)
    n = torch.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]], dim=1)
    n = torch.nn.functional.normalize(n, dim=1, eps=1e-6)
    return (1.0 - (n[a] * n[b]).sum(dim=1)).mean()


class _ChamferFn(torch.autograd.Function):
    """(x (N,P,3), y (N,Q,3), x_len, y_len) -> (dist_x (N,P), dist_y (N,Q), idx_x, idx_y): squared
    nearest-neighbour distances both ways and the int32 nearest indices (pr_chamfer_fwd/bwd).  The
    lengths are (N,) int64 device tensors or None (full); they are read on the device."""

    @staticmethod
    def _args(nat, x, y, x_len, y_len, idx_x, idx_y):
        a = nat.PRChamferArgs()
        a.x, a.y, a.x_len, a.y_len = nat.ptr(x), nat.ptr(y), nat.ptr(x_len), nat.ptr(y_len)
        a.N, a.P, a.Q = x.shape[0], x.shape[1], y.shape[1]
        a.idx_x, a.idx_y = nat.ptr(idx_x), nat.ptr(idx_y)
        return a

    @staticmethod
    def _workspace(nat, a, x):
        nbytes = nat.load().pr_chamfer_workspace(a.N, a.P, a.Q)
        ws = nat.workspace(nbytes, x.device) if nbytes else None
        a.workspace, a.workspace_bytes = nat.ptr(ws), nbytes
        return ws  # kept alive by the caller's frame until the launch is enqueued (stream-ordered free)

    @staticmethod
    def forward(ctx, x, y, x_len, y_len):
        from .. import _native as nat
        # the kernels index every cloud as (n, i, 3) and every length as [n]: nothing else may reach them
        if x.dim() != 3 or y.dim() != 3 or x.shape[2] != 3 or y.shape[2] != 3 or x.shape[0] != y.shape[0]:
            raise ValueError(f"expected x (N,P,3) and y (N,Q,3), got {tuple(x.shape)} and {tuple(y.shape)}")
        for t, name in ((x_len, "x_lengths"), (y_len, "y_lengths")):
            if t is not None and (tuple(t.shape) != (x.shape[0],) or t.is_floating_point() or t.dtype == torch.bool):
                raise ValueError(f"{name} must be an integer tensor of shape ({x.shape[0]},), got {t.dtype} {tuple(t.shape)}")
        nat.require_device(x, y, x_len, y_len)
        for t, name in ((y, "y"), (x_len, "x_lengths"), (y_len, "y_lengths")):
            if t is not None and t.device != x.device:
                raise ValueError(f"{name} is on {t.device}, x on {x.device}")
        xd, yd = nat.dense(x, torch.float32), nat.dense(y, torch.float32)
        xl = None if x_len is None else nat.dense(x_len, torch.int64)
        yl = None if y_len is None else nat.dense(y_len, torch.int64)
        N, P, Q = xd.shape[0], xd.shape[1], yd.shape[1]
        dist_x = torch.empty((N, P), dtype=torch.float32, device=xd.device)
        dist_y = torch.empty((N, Q), dtype=torch.float32, device=xd.device)
        idx_x = torch.empty((N, P), dtype=torch.int32, device=xd.device)
        idx_y = torch.empty((N, Q), dtype=torch.int32, device=xd.device)
        a = _ChamferFn._args(nat, xd, yd, xl, yl, idx_x, idx_y)
        a.dist_x, a.dist_y = nat.ptr(dist_x), nat.ptr(dist_y)
        ws = _ChamferFn._workspace(nat, a, xd)  # noqa: F841
        nat.call("pr_chamfer_fwd", "pr_chamfer_fwd", xd, a)
        ctx.save_for_backward(xd, yd, idx_x, idx_y)
        ctx.lens = (xl, yl)
        ctx.mark_non_differentiable(idx_x, idx_y)
        return dist_x, dist_y, idx_x, idx_y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_dx, g_dy, _gix, _giy):
        from .. import _native as nat
        xd, yd, idx_x, idx_y = ctx.saved_tensors
        gx, gy = torch.empty_like(xd), torch.empty_like(yd)
        g_dx = torch.zeros(idx_x.shape, dtype=torch.float32, device=xd.device) if g_dx is None else nat.dense(g_dx, torch.float32)
        g_dy = torch.zeros(idx_y.shape, dtype=torch.float32, device=xd.device) if g_dy is None else nat.dense(g_dy, torch.float32)
        a = _ChamferFn._args(nat, xd, yd, *ctx.lens, idx_x, idx_y)
        a.grad_dist_x, a.grad_dist_y, a.grad_x, a.grad_y = nat.ptr(g_dx), nat.ptr(g_dy), nat.ptr(gx), nat.ptr(gy)
        ws = _ChamferFn._workspace(nat, a, xd)  # noqa: F841
        nat.call("pr_chamfer_bwd", "pr_chamfer_bwd", xd, a)
        return gx, gy, None, None


def _chamfer_nn_torch(x, y, x_len, y_len):
    """The torch composition of _ChamferFn: a dense (N,P,Q) matrix and two mins."""
    d = torch.cdist(x, y).pow(2)
    if x_len is None and y_len is None:
        mx, my = d.min(dim=2), d.min(dim=1)
        return mx.values, my.values, mx.indices, my.indices
    N, P, Q = d.shape
    inf = float("inf")
    x_pad = torch.arange(P, device=d.device)[None] >= (x_len[:, None] if x_len is not None else P)
    y_pad = torch.arange(Q, device=d.device)[None] >= (y_len[:, None] if y_len is not None else Q)
    mx, my = d.masked_fill(y_pad[:, None, :], inf).min(dim=2), d.masked_fill(x_pad[:, :, None], inf).min(dim=1)
    # padded points, and every point of a cloud whose other side is empty: distance 0, index -1
    dead_x, dead_y = x_pad | y_pad.all(dim=1, keepdim=True), y_pad | x_pad.all(dim=1, keepdim=True)
    return (mx.values.masked_fill(dead_x, 0.0), my.values.masked_fill(dead_y, 0.0),
            mx.indices.masked_fill(dead_x, -1), my.indices.masked_fill(dead_y, -1))


def _chamfer_reduce(cx, cy, x_len, y_len, weights, batch_reduction, point_reduction):
    """PyTorch3D 0.4.0's reductions of the per-point terms (N,P), (N,Q) (0 at padded points)."""
    if weights is not None:
        cx, cy = cx * weights[:, None], cy * weights[:, None]
    if point_reduction == "mean":
        rx = cx.mean(1) if x_len is None else cx.sum(1) / x_len.clamp(min=1).to(cx.dtype)
        ry = cy.mean(1) if y_len is None else cy.sum(1) / y_len.clamp(min=1).to(cy.dtype)
    else:
        rx, ry = cx.sum(1), cy.sum(1)
    loss = rx + ry
    if batch_reduction == "mean":
        loss = loss.mean() if weights is None else loss.sum() / weights.sum()
    elif batch_reduction == "sum":
        loss = loss.sum()
    return loss


def _normal_terms(n, n_other, idx):
    """1 - |cos(n_i, n_other[idx_i])| (N,P); 0 where idx is -1."""
    # indexed, not gathered: the backward is a sorted index_put_(accumulate=True), the same bits on
    # every call (gather's is a scatter_add on float atomics)
    near = n_other[torch.arange(idx.shape[0], device=idx.device)[:, None], idx.clamp(min=0).to(torch.int64)]
    c = 1.0 - torch.nn.functional.cosine_similarity(n, near, dim=2, eps=1e-6).abs()
    return c.masked_fill(idx < 0, 0.0)


def chamfer_distance(x, y, batch_reduction="mean", point_reduction="mean", *, x_lengths=None, y_lengths=None,
                     x_normals=None, y_normals=None, weights=None):
    """Symmetric squared Chamfer distance between padded point clouds x (N,P,3) and y (N,Q,3);
    returns (loss, loss_normals) like PyTorch3D 0.4.0, loss_normals None without normals.

    x_lengths / y_lengths (N,) int64: the points at index >= length are padding, contribute 0 and
    are never a nearest neighbour.  weights (N,) multiplies the per-cloud sums.  point_reduction
    "mean" divides a cloud's sum by its length (an empty cloud gives 0), "sum" does not;
    batch_reduction "mean" divides the batch sum by N, or by weights.sum() when weights are given,
    "sum" adds, None returns the (N,) per-cloud values.  With x_normals (N,P,3) and y_normals
    (N,Q,3), loss_normals is built the same way from 1 - |cos(x_normal_i, y_normal_nn(i))| and its
    mirror, in torch on the nearest indices.  On a ROCm device with float32 clouds the nearest
    neighbours and their gradient run on the native kernels (csrc/pr_chamfer.hip: no (N,P,Q)
    matrix, the lowest index wins on equal distances, bitwise reproducible, capturable);
    otherwise (CPU, other dtypes, a point dimension other than 3, PR_NATIVE_MESHLOSS=0) a torch.cdist
    composition.  The two differ on non-finite input: torch.min propagates a NaN point into its
    neighbours' distances, the kernels never choose one, and a point that can choose nothing gets a
    non-finite distance (NaN if it is NaN itself, else +inf) and no gradient, so the loss still shows
    it.  Shapes, devices and integer lengths are checked (ValueError) before anything is launched.
    Parity with PyTorch3D is unpinned (not installable here)."""
    if (x_normals is None) != (y_normals is None):
        raise ValueError("x_normals and y_normals must be given together")
    # the shape the native op takes; the composition also serves what torch.cdist has always taken
    # here (another point dimension, a batch of 1 broadcast against N)
    regular = x.dim() == 3 and y.dim() == 3 and x.shape[0] == y.shape[0] and x.shape[2] == y.shape[2]
    if x_lengths is not None or y_lengths is not None or weights is not None or x_normals is not None:
        if not regular:
            raise ValueError(f"expected x (N,P,D) and y (N,Q,D), got {tuple(x.shape)} and {tuple(y.shape)}")
        N = x.shape[0]
        for t, name, shape in ((x_lengths, "x_lengths", (N,)), (y_lengths, "y_lengths", (N,)), (weights, "weights", (N,)),
                               (x_normals, "x_normals", tuple(x.shape)), (y_normals, "y_normals", tuple(y.shape))):
            if t is None:
                continue
            if tuple(t.shape) != shape:
                raise ValueError(f"{name} must have shape {shape}, got {tuple(t.shape)}")
            if t.device != x.device:
                raise ValueError(f"{name} is on {t.device}, x on {x.device}")
        if any(t is not None and (t.is_floating_point() or t.dtype == torch.bool) for t in (x_lengths, y_lengths)):
            raise ValueError("x_lengths and y_lengths must be integer tensors")
    if x.device != y.device:
        raise ValueError(f"x is on {x.device}, y on {y.device}")
    if (_native(x) and y.dtype == torch.float32 and regular and x.shape[2] == 3 and 0 < x.shape[0] <= 32767
            and x.shape[1] > 0 and y.shape[1] > 0):
        cx, cy, ix, iy = _ChamferFn.apply(x, y, x_lengths, y_lengths)
    else:
        cx, cy, ix, iy = _chamfer_nn_torch(x, y, x_lengths, y_lengths)
    args = (x_lengths, y_lengths, weights, batch_reduction, point_reduction)
    loss = _chamfer_reduce(cx, cy, *args)
    if x_normals is None:
        return loss, None
    return loss, _chamfer_reduce(_normal_terms(x_normals, y_normals, ix), _normal_terms(y_normals, x_normals, iy), *args)

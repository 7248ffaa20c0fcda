"""PyTorch3D 0.4.0 mesh losses that experiments/eval.py imports (eval.py:26-31) and uses
in its vertex-deformation task (mesh_laplacian_smoothing, eval.py:455).

The index structures (unique edges, neighbour CSR, face pairs, per-vertex weights) come from the
mesh's cached topology record (mesh.py _Topology), so a call builds no index tensor and does not
synchronise: after one call a deformation step can be captured in a HIP graph.  On a ROCm device
with float32 inputs all four losses run on the native kernels (the Laplacian, the edge loss and
normal consistency in csrc/pr_meshloss.hip: per-vertex / per-face CSR gathers; chamfer_distance's
nearest neighbours in csrc/pr_chamfer.hip; no atomics, bitwise reproducible);
PR_NATIVE_MESHLOSS=0 (or NATIVE_MESHLOSS = False), CPU tensors and other dtypes take the torch
composition of the same formulas.  point_mesh_face_distance and point_mesh_edge_distance (the
losses between a mesh and a Pointclouds, csrc/pr_pointmesh.hip) follow the same rules.  Parity
with PyTorch3D is unpinned (not installable here)."""
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


# ------------------------------------------------------------------ point-to-mesh distances
# The closest point of a primitive (csrc/pr_pointmesh.hip states the same arithmetic): the Voronoi
# region of p from the signs of the edge dot products (Ericson's closest-point-on-triangle tests, in
# his order) gives the weights w of the closest point; in a vertex or edge region
# r = sum w_i (p - v_i); in the interior the point is projected first, n = (v1 - v0) x (v2 - v0),
# t = n . (p - v0) / |n|^2, r = t n, and w comes from the projected point's cross products against n;
# d^2 = |r|^2.  A triangle with |n|^2 <= _DEGENERATE is evaluated as its three segments, a
# zero-length segment as its first endpoint.  Choosing the region by comparing squared distances
# would lose half of float32's digits.
_DEGENERATE = 1e-30
_PAIRS_PER_CHUNK = 1 << 19  # (point, primitive) pairs per block of the composition: ~400 B of float32 temporaries each, ~200 MB
_PRIMS = {"faces": 0, "edges": 1}


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _ratio(num, den):
    return torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(num))


def _closest_on_segment(p, a, b):
    """(d^2, w (...,3) = (1 - v, v, 0), r) of the points p against the segments (a, b), broadcast."""
    ab, ap, bp = b - a, p - a, p - b
    d1, d3 = _dot(ab, ap), _dot(ab, bp)
    v = torch.where(d1 <= 0, torch.zeros_like(d1), torch.where(d3 >= 0, torch.ones_like(d1), d1 / (d1 - d3)))
    w = torch.stack([1 - v, v, torch.zeros_like(v)], -1)
    r = ap * w[..., 0:1] + bp * w[..., 1:2]
    return _dot(r, r), w, r


def _closest_on_triangle(p, a, b, c):
    """(d^2, w (...,3), r) of the points p against the triangles (a, b, c), broadcast."""
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    n = torch.cross(ab.expand_as(ap), ac.expand_as(ap), dim=-1)
    n2 = _dot(n, n)
    flat = ~(n2 > _DEGENERATE)
    inv = torch.where(flat, torch.zeros_like(n2), 1.0 / torch.where(flat, torch.ones_like(n2), n2))
    t = _dot(n, ap) * inv
    r_in = n * t[..., None]
    q = ap - r_in
    w1, w2 = _dot(n, torch.cross(q, ac.expand_as(q), dim=-1)) * inv, _dot(n, torch.cross(ab.expand_as(q), q, dim=-1)) * inv
    one, zero = torch.ones_like(d1), torch.zeros_like(d1)
    st = lambda x, y, z: torch.stack([x, y, z], -1)  # noqa: E731
    vab, vac, vbc = _ratio(d1, d1 - d3), _ratio(d2, d2 - d6), _ratio(d4 - d3, (d4 - d3) + (d5 - d6))
    regions = [((d1 <= 0) & (d2 <= 0), st(one, zero, zero)),
               ((d3 >= 0) & (d4 <= d3), st(zero, one, zero)),
               ((d1 * d4 - d3 * d2 <= 0) & (d1 >= 0) & (d3 <= 0), st(1 - vab, vab, zero)),
               ((d6 >= 0) & (d5 <= d6), st(zero, zero, one)),
               ((d5 * d2 - d1 * d6 <= 0) & (d2 >= 0) & (d6 <= 0), st(1 - vac, zero, vac)),
               ((d3 * d6 - d5 * d4 <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), st(zero, 1 - vbc, vbc))]
    w, inside = st(1 - w1 - w2, w1, w2), torch.ones_like(d1, dtype=torch.bool)
    for cond, wr in reversed(regions):  # applied last to first: the earliest test of Ericson's order wins
        w = torch.where(cond[..., None], wr, w)
        inside = inside & ~cond
    r = torch.where(inside[..., None], r_in, ap * w[..., 0:1] + bp * w[..., 1:2] + cp * w[..., 2:3])
    d = _dot(r, r)
    if bool(flat.any()):  # the first of the three segments that is nearest
        ds, ws, rs = _closest_on_segment(p, a, b)
        for (x, y), perm in (((b, c), (2, 0, 1)), ((c, a), (1, 2, 0))):
            d2_, w2_, r2_ = _closest_on_segment(p, x, y)
            less = d2_ < ds
            ds, rs = torch.where(less, d2_, ds), torch.where(less[..., None], r2_, rs)
            ws = torch.where(less[..., None], w2_[..., list(perm)], ws)
        d, w, r = torch.where(flat, ds, d), torch.where(flat[..., None], ws, w), torch.where(flat[..., None], rs, r)
    return d, w, r


def _closest(p, pv):
    """p (...,3) against the primitives pv (...,K,3): triangles (K = 3) or segments (K = 2)."""
    if pv.shape[-2] == 3:
        return _closest_on_triangle(p, pv[..., 0, :], pv[..., 1, :], pv[..., 2, :])
    return _closest_on_segment(p, pv[..., 0, :], pv[..., 1, :])


def _is_nan_row(t):
    return (t != t).reshape(t.shape[0], -1).any(dim=1)


def _missed(dist, found, query_nan, searched):
    """A query that chose nothing: 0 when it had nothing to search, else NaN if it is NaN itself, +inf otherwise."""
    miss = torch.where(query_nan, torch.full_like(dist, float("nan")), torch.full_like(dist, float("inf")))
    return torch.where(found, dist, miss if searched else torch.zeros_like(dist))


def _point_mesh_nn_torch(points, verts, prims, cloud_ranges, mesh_ranges):
    """The torch composition of _PointMeshFn on packed inputs, in the points' dtype: (dist_p (P),
    dist_m (M), idx_p, idx_m int64, w_p (P,3), w_m (M,3)).  The ranges are Python (first, count)
    pairs per batch element.  The search runs without autograd in blocks of at most
    _PAIRS_PER_CHUNK pairs; the chosen pairs are evaluated once more, and the gradient is attached
    in envelope form: d d^2 / d p = 2 r, d d^2 / d v_i = -2 w_i r, r and w constants."""
    P, M = points.shape[0], prims.shape[0]
    dev, inf = points.device, float("inf")
    dist_p, dist_m = points.new_zeros(P), points.new_zeros(M)
    idx_p = torch.full((P,), -1, dtype=torch.int64, device=dev)
    idx_m = torch.full((M,), -1, dtype=torch.int64, device=dev)
    with torch.no_grad():
        pd, pv_all = points.detach(), verts.detach()[prims]
        for (pf, pc), (mf, mc) in zip(cloud_ranges, mesh_ranges):
            if pc == 0 or mc == 0:
                continue
            pv = pv_all[mf:mf + mc]
            best_m = torch.full((mc,), inf, dtype=points.dtype, device=dev)
            arg_m = torch.full((mc,), -1, dtype=torch.int64, device=dev)
            step = max(1, _PAIRS_PER_CHUNK // mc)
            for c0 in range(pf, pf + pc, step):
                c1 = min(c0 + step, pf + pc)
                d = _closest(pd[c0:c1, None], pv[None])[0]
                d = torch.where(d != d, torch.full_like(d, inf), d)  # a NaN candidate is never chosen
                mp, mm = d.min(dim=1), d.min(dim=0)  # the first minimum: the lowest index
                dist_p[c0:c1] = mp.values
                idx_p[c0:c1] = torch.where(mp.values < inf, mp.indices + mf, torch.full_like(mp.indices, -1))
                less = mm.values < best_m  # strict, blocks in ascending order: the lowest index
                best_m, arg_m = torch.where(less, mm.values, best_m), torch.where(less, mm.indices + c0, arg_m)
            dist_m[mf:mf + mc], idx_m[mf:mf + mc] = best_m, arg_m
            dist_p[pf:pf + pc] = _missed(dist_p[pf:pf + pc], idx_p[pf:pf + pc] >= 0, _is_nan_row(pd[pf:pf + pc]), True)
            dist_m[mf:mf + mc] = _missed(best_m, arg_m >= 0, _is_nan_row(pv), True)
        _, w_p, r_p = _closest(pd, pv_all[idx_p.clamp(min=0)])
        _, w_m, r_m = _closest(pd[idx_m.clamp(min=0)], pv_all)
        live_p, live_m = idx_p >= 0, idx_m >= 0
        zero = torch.zeros((), dtype=points.dtype, device=dev)
        w_p, r_p = torch.where(live_p[:, None], w_p, zero), torch.where(live_p[:, None], r_p, zero)
        w_m, r_m = torch.where(live_m[:, None], w_m, zero), torch.where(live_m[:, None], r_m, zero)
    K = prims.shape[1]
    pv_all = verts[prims]

    def attach(dist, live, p, pv, w, r):
        # value dist, gradient 2 r . d (p - sum w_i v_i): the difference below is exactly 0 (a query
        # that chose nothing is left out: its coordinates may be NaN)
        delta = p - (pv * w[:, :K, None]).sum(dim=1)
        return dist + torch.where(live, 2.0 * (r * (delta - delta.detach())).sum(dim=-1), zero)

    dist_p = attach(dist_p, live_p, points, pv_all[idx_p.clamp(min=0)], w_p, r_p)
    dist_m = attach(dist_m, live_m, points[idx_m.clamp(min=0)], pv_all, w_m, r_m)
    return dist_p, dist_m, idx_p, idx_m, w_p, w_m


class _PointMeshFn(torch.autograd.Function):
    """(points (P,3) packed, verts (V,3)) -> (dist_p (P), dist_m (M), idx_p (P), idx_m (M) int32 packed
    or -1, w_p (P,3), w_m (M,3)) for the topology's faces or edges (pr_point_mesh_fwd/bwd).  The
    clouds are given by device tables (cloud_first, cloud_count) and the host bound max_points;
    cloud_first None is a padded batch of max_points rows per cloud.  The backward sorts idx_p and
    idx_m on the device into the two CSRs of the call: once-differentiable, no host read."""

    @staticmethod
    def _args(nat, p, v, tab, kind, cloud_first, cloud_count, max_points, idx_p, idx_m, w_p, w_m):
        a = nat.PRPointMeshArgs()
        a.points, a.cloud_first, a.cloud_count = nat.ptr(p), nat.ptr(cloud_first), nat.ptr(cloud_count)
        a.verts, a.prims, a.mesh_first, a.mesh_count = nat.ptr(v), nat.ptr(tab["prims"]), nat.ptr(tab["first"]), nat.ptr(tab["count"])
        a.N, a.P, a.V, a.M = len(tab["counts"]), p.shape[0], v.shape[0], tab["prims"].shape[0]
        a.max_points, a.max_prims, a.prim = max_points, max(tab["counts"]), _PRIMS[kind]
        a.idx_p, a.idx_m, a.w_p, a.w_m = nat.ptr(idx_p), nat.ptr(idx_m), nat.ptr(w_p), nat.ptr(w_m)
        nbytes = nat.load().pr_point_mesh_workspace(a.prim, a.N, a.P, a.M, a.max_points, a.max_prims)
        ws = nat.workspace(nbytes, p.device)
        a.workspace, a.workspace_bytes = nat.ptr(ws), nbytes
        return a, ws  # ws: kept alive by the caller's frame until the launch is enqueued

    @staticmethod
    def forward(ctx, points, verts, topo, kind, cloud_first, cloud_count, max_points):
        from .. import _native as nat
        nat.require_device(points, verts, cloud_first, cloud_count)
        p, v = nat.dense(points, torch.float32), nat.dense(verts, torch.float32)
        cf = None if cloud_first is None else nat.dense(cloud_first, torch.int64)
        cc = None if cloud_count is None else nat.dense(cloud_count, torch.int64)
        tab = topo.prim_tables(kind)
        P, M = p.shape[0], tab["prims"].shape[0]
        new = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=p.device)  # noqa: E731
        dist_p, dist_m, w_p, w_m = new((P,)), new((M,)), new((P, 3)), new((M, 3))
        idx_p, idx_m = new((P,), torch.int32), new((M,), torch.int32)
        a, ws = _PointMeshFn._args(nat, p, v, tab, kind, cf, cc, max_points, idx_p, idx_m, w_p, w_m)  # noqa: F841
        a.dist_p, a.dist_m = nat.ptr(dist_p), nat.ptr(dist_m)
        nat.call("pr_point_mesh_fwd", "pr_point_mesh_fwd", p, a)
        ctx.save_for_backward(p, v, idx_p, idx_m, w_p, w_m)
        ctx.topo, ctx.kind, ctx.clouds = topo, kind, (cf, cc, max_points)
        ctx.mark_non_differentiable(idx_p, idx_m, w_p, w_m)
        return dist_p, dist_m, idx_p, idx_m, w_p, w_m

    @staticmethod
    def _csr(idx, rows, arange):
        """rows -> the entries of idx that name them, ascending (a stable device sort; -1 last)."""
        key = torch.where(idx < 0, rows, idx)
        order = torch.argsort(key, stable=True)
        return torch.searchsorted(key[order].contiguous(), arange), order

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_p, g_m, *_unused):
        from .. import _native as nat
        p, v, idx_p, idx_m, w_p, w_m = ctx.saved_tensors
        topo, kind = ctx.topo, ctx.kind
        tab = topo.prim_tables(kind)
        P, M = p.shape[0], tab["prims"].shape[0]
        g_p = torch.zeros_like(w_p[:, 0]) if g_p is None else nat.dense(g_p, torch.float32)
        g_m = torch.zeros_like(w_m[:, 0]) if g_m is None else nat.dense(g_m, torch.float32)
        gp, gv = torch.empty_like(p), torch.empty_like(v)
        a, ws = _PointMeshFn._args(nat, p, v, tab, kind, *ctx.clouds, idx_p, idx_m, w_p, w_m)  # noqa: F841
        prim_start, prim_points = _PointMeshFn._csr(idx_p, M, tab["arange"])
        point_start, point_prims = _PointMeshFn._csr(idx_m, P, torch.arange(P + 1, dtype=torch.int32, device=p.device))
        a.prim_point_start, a.prim_points = nat.ptr(prim_start), nat.ptr(prim_points)
        a.point_prim_start, a.point_prims = nat.ptr(point_start), nat.ptr(point_prims)
        csr = topo.corner_csr("gather") if kind == "faces" else topo.edge_end_csr()
        a.vert_corner_start, a.vert_corners = nat.ptr(csr[0]), nat.ptr(csr[1])
        a.grad_dist_p, a.grad_dist_m, a.grad_points, a.grad_verts = nat.ptr(g_p), nat.ptr(g_m), nat.ptr(gp), nat.ptr(gv)
        nat.call("pr_point_mesh_bwd", "pr_point_mesh_bwd", p, a)
        return gp, gv, None, None, None, None, None


def _point_mesh_inputs(meshes, pcls, lengths):
    """Checked inputs of the point-to-mesh losses: (points (P,3) packed, cloud_first, cloud_count
    (device tensors or None), max_points, host (first, count) pairs or None, dtype -> the per-point
    weights 1 / (N P_n) as a (P,) tensor or a float)."""
    from .mesh import Meshes
    from .pointclouds import Pointclouds
    if not isinstance(meshes, Meshes):
        raise ValueError(f"meshes must be a Meshes, got {type(meshes).__name__}")
    N = len(meshes)
    if N == 0:
        raise ValueError("meshes is empty")
    v = meshes.verts_packed()
    if not v.is_floating_point() or v.dim() != 2 or v.shape[1] != 3:
        raise ValueError(f"vertices must be floating point (V,3), got {v.dtype} {tuple(v.shape)}")
    if isinstance(pcls, Pointclouds):
        if lengths is not None:
            raise ValueError("lengths goes with a padded (N,P,3) tensor, not with a Pointclouds")
        if len(pcls) != N:
            raise ValueError(f"meshes and pcls must have the same batch size, got {N} and {len(pcls)}")
        points = pcls.points_packed()
        if points.device != v.device:
            raise ValueError(f"pcls is on {points.device}, the meshes on {v.device}")
        ranges, off = [], 0
        for n in pcls.npoints:
            ranges.append((off, n))
            off += n
        return (points, pcls.cloud_to_packed_first_idx(), pcls.num_points_per_cloud(), max(pcls.npoints), ranges,
                pcls.loss_weights)
    if not torch.is_tensor(pcls) or pcls.dim() != 3 or pcls.shape[2] != 3:
        raise ValueError("pcls must be a Pointclouds or a padded (N,P,3) tensor, got "
                         f"{tuple(pcls.shape) if torch.is_tensor(pcls) else type(pcls).__name__}")
    if pcls.shape[0] != N:
        raise ValueError(f"meshes and pcls must have the same batch size, got {N} and {pcls.shape[0]}")
    if pcls.device != v.device:
        raise ValueError(f"pcls is on {pcls.device}, the meshes on {v.device}")
    P = pcls.shape[1]
    if lengths is None:
        return pcls.reshape(-1, 3), None, None, P, [(n * P, P) for n in range(N)], lambda dtype: 1.0 / (N * max(P, 1))
    if not torch.is_tensor(lengths) or tuple(lengths.shape) != (N,) or lengths.is_floating_point() or lengths.dtype == torch.bool:
        raise ValueError(f"lengths must be an integer tensor of shape ({N},)")
    if lengths.device != v.device:
        raise ValueError(f"lengths is on {lengths.device}, the meshes on {v.device}")
    count = lengths.to(torch.int64).clamp(0, P)  # read on the device, as chamfer_distance's lengths
    return (pcls.reshape(-1, 3), None, count, P, None,
            lambda dtype: (1.0 / (N * count.clamp(min=1).to(torch.float64))).to(dtype)[:, None].expand(N, P).reshape(-1))


def _point_mesh_nn(meshes, pcls, kind, lengths=None):
    """(dist_p (P), dist_m (M), idx_p, idx_m, w_p (P,3), w_m (M,3), the points' and the primitives'
    loss weights 1 / (N P_n), 1 / (N M_n)) on packed points and primitives ("faces" / "edges"); a padded tensor is packed row by row, its
    padding rows get 0 and -1.  Native on a ROCm device with float32 inputs, else the composition."""
    points, cloud_first, cloud_count, max_points, ranges, wp = _point_mesh_inputs(meshes, pcls, lengths)
    v, topo = meshes.verts_packed(), meshes._topo
    tab = topo.prim_tables(kind)
    P, M, N = points.shape[0], tab["prims"].shape[0], len(meshes)
    if P == 0 or M == 0:  # nothing on one side: every term is 0
        z = points.sum() * 0.0 + v.sum() * 0.0
        return (z + points.new_zeros(P), z + points.new_zeros(M), torch.full((P,), -1, dtype=torch.int64, device=v.device),
                torch.full((M,), -1, dtype=torch.int64, device=v.device), points.new_zeros((P, 3)), points.new_zeros((M, 3)),
                wp(points.dtype), topo.prim_loss_weights(kind, points.dtype))
    if (_native(v) and points.dtype == torch.float32 and N <= 32767 and P <= 2 ** 31 - 1 and 16 * M <= 2 ** 31 - 1):
        out = _PointMeshFn.apply(points, v, topo, kind, cloud_first, cloud_count, max_points)
    else:
        if ranges is None:  # the composition slices on the host: one read of the lengths
            ranges = [(n * max_points, int(c)) for n, c in enumerate(cloud_count.tolist())]
        mesh_ranges, off = [], 0
        for c in tab["counts"]:
            mesh_ranges.append((off, c))
            off += c
        out = _point_mesh_nn_torch(points, v.to(points.dtype), tab["prims"], ranges, mesh_ranges)
    return (*out, wp(out[0].dtype), topo.prim_loss_weights(kind, out[0].dtype))


def _point_mesh_distance(meshes, pcls, kind, lengths):
    dist_p, dist_m, _, _, _, _, wp, wm = _point_mesh_nn(meshes, pcls, kind, lengths)
    return (dist_p * wp).sum() + (dist_m * wm).sum()


def point_mesh_face_distance(meshes, pcls, *, lengths=None):
    """Squared point-to-face distance between meshes and point clouds, both ways (PyTorch3D 0.4.0
    point_mesh_face_distance's reductions): a 0-d loss
        (1/N) sum_n [ (1/P_n) sum_{p in cloud n} d^2(p, mesh n) + (1/F_n) sum_{f in mesh n} d^2(f, cloud n) ],
    d^2(p, mesh) the minimum over the mesh's triangles of the squared distance to the triangle,
    d^2(f, cloud) the minimum over the cloud's points; the lowest index wins on equal values.

    `pcls` is a Pointclouds, or a padded (N,P,3) tensor with `lengths` (N,) int64 (read on the
    device; None: full).  A cloud or mesh with nothing on the other side contributes 0.  The
    closest point comes from the Voronoi region of the point (the signs of the edge dot products,
    Ericson's order); in the interior the point is projected on the plane first; a triangle with
    |n|^2 <= 1e-30 is evaluated as its three segments.  Gradients are the envelope form
    d d^2 / d p = 2 r, d d^2 / d v_i = -2 w_i r with the closest point's weights as constants.

    On a ROCm device with float32 inputs the search and its backward run on the native kernels
    (csrc/pr_pointmesh.hip: no (P,F) matrix, no atomics, bitwise reproducible, capturable after one
    call on the topology); otherwise (CPU, other dtypes, PR_NATIVE_MESHLOSS=0) a torch composition
    of the same formulas, in blocks over the points.  On non-finite input both paths follow
    chamfer_distance's kernels: a NaN candidate is never chosen, and a query that can choose
    nothing gets a non-finite distance and no gradient.  Arguments are checked (ValueError) before
    anything is launched.  Parity with PyTorch3D is unpinned (not installable here)."""
    return _point_mesh_distance(meshes, pcls, "faces", lengths)


def point_mesh_edge_distance(meshes, pcls, *, lengths=None):
    """point_mesh_face_distance with the meshes' unique edges (edges_packed(): segments) in place of
    their faces: (1/N) sum_n [ (1/P_n) sum_p d^2(p, edges of mesh n) + (1/E_n) sum_e d^2(e, cloud n) ].
    A zero-length edge is evaluated as its first endpoint."""
    return _point_mesh_distance(meshes, pcls, "edges", lengths)

"""PyTorch3D 0.4.0 ``pytorch3d.ops.sample_points_from_meshes``: area-weighted points (and face
normals) on the surface of every mesh of a batch, differentiable with respect to the vertices.  It
feeds loss.chamfer_distance in the deformation loop.

On a ROCm device with float32 vertices the sampler runs on the native kernels
(csrc/pr_samplepoints.hip: a face pass, a per-mesh float64 scan of the areas, one lane per sample;
the backward a per-face segment sum and a per-vertex gather: no atomics, bitwise reproducible).
The per-mesh face tables are read on the device and the backward's face -> samples index is a
device sort, so after one call on a topology a call builds nothing on the host and does not
synchronise: the deformation step can be captured in a HIP graph.  PR_NATIVE_MESHLOSS=0 (or
loss.NATIVE_MESHLOSS = False), CPU tensors and other dtypes take the torch composition of the same
formulas (_sample_points_torch).  Parity with PyTorch3D is unpinned (not installable here).

``knn_points`` / ``knn_gather`` (PyTorch3D 0.4.0, same module) are here as torch compositions on every
device: chunked over the queries, a stable lowest-index tie rule, lengths read on the device."""
import collections

import torch

from .. import noise as _noise
from . import loss as _loss

_TAG_SAMP = 0x53414D50  # "SAMP", the 4th counter word of the sampler's Philox stream
_NORMAL_EPS = 2.220446049250313e-16
_INT32_MAX = 2 ** 31 - 1
_MAX_MESHES = 65535


def _philox_uniforms(key, N, S, device):
    """(N,S,3) float32 uniforms of the sampler's Philox stream, in torch integer ops: one
    Philox4x32-7 block per (n, s), counter (s, n, 0, "SAMP"), key split low / high, u_i = u01 of
    word i (csrc/pr_common.h philox_block / u01).  What the kernels draw in Philox mode."""
    m32 = 0xFFFFFFFF
    s = torch.arange(S, dtype=torch.int64, device=device)[None, :].expand(N, S)
    n = torch.arange(N, dtype=torch.int64, device=device)[:, None].expand(N, S)
    c = [s, n, torch.zeros_like(s), torch.full_like(s, _TAG_SAMP)]
    k0, k1 = int(key) & m32, (int(key) >> 32) & m32
    for _ in range(7):
        # 32 x 32 -> 64 bit products; int64 wraps modulo 2^64, the masks take the two halves
        p0, p1 = c[0] * 0xD2511F53, c[2] * 0xCD9E8D57
        c = [((p1 >> 32) & m32) ^ c[1] ^ k0, p1 & m32, ((p0 >> 32) & m32) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & m32, (k1 + 0xBB67AE85) & m32
    words = torch.stack(c[:3], dim=-1)
    return ((words >> 8) | 1).to(torch.float32) * 5.9604644775390625e-08


def _sample_points_torch(meshes, uniforms, return_normals=False):
    """The torch composition of the sampler from given uniforms (N,S,3), in the vertices' dtype:
    (samples (N,S,3), normals (N,S,3) or None, face_idx (N,S) int64 packed or -1, w (N,S,3),
    cdf (F,)).  Per mesh: areas 0.5 |(v1 - v0) x (v2 - v0)|, cdf = areas.double().cumsum(0) rounded to
    the dtype, r = u0 cdf[-1], the first face with cdf > r, else the first with cdf >= cdf[-1].  The
    meshes' face counts are the topology's Python ints: no host read."""
    v, f, topo = meshes.verts_packed(), meshes.faces_packed(), meshes._topo
    N, S = uniforms.shape[0], uniforms.shape[1]
    u = uniforms.to(v.dtype)
    F = f.shape[0]
    if F == 0:
        z = v.sum() * 0.0 + torch.zeros((N, S, 3), dtype=v.dtype, device=v.device)
        return (z, z.clone() if return_normals else None, torch.full((N, S), -1, dtype=torch.int64, device=v.device),
                torch.zeros_like(z), torch.zeros(0, dtype=v.dtype, device=v.device))
    with torch.no_grad():
        vd = v.detach()
        a0, a1, a2 = vd[f[:, 0]], vd[f[:, 1]], vd[f[:, 2]]
        area = 0.5 * torch.cross(a1 - a0, a2 - a0, dim=1).norm(dim=1)
        cdf = torch.zeros_like(area)
        picks, off = [], 0
        for n, nf in enumerate(topo.nfaces):
            if nf == 0:
                picks.append(torch.full((S,), -1, dtype=torch.int64, device=v.device))
                continue
            c = area[off:off + nf].double().cumsum(0).to(v.dtype)
            cdf[off:off + nf] = c
            total = c[-1]
            k = torch.searchsorted(c, (u[n, :, 0] * total).contiguous(), right=True)
            k = torch.where(k >= nf, torch.searchsorted(c, total.reshape(1)).expand(S), k)
            picks.append(torch.where(total > 0, k + off, torch.full_like(k, -1)))
            off += nf
        face = torch.stack(picks)
        live = face >= 0
        su = u[..., 1].sqrt()
        w = torch.stack([1.0 - su, su * (1.0 - u[..., 2]), su * u[..., 2]], dim=-1) * live[..., None].to(v.dtype)
    fv = v[f[face.clamp(min=0)]]  # (N,S,3,3)
    v0, v1, v2 = fv[..., 0, :], fv[..., 1, :], fv[..., 2, :]
    dead = ~live[..., None]
    p = (w[..., 0:1] * v0 + w[..., 1:2] * v1 + w[..., 2:3] * v2).masked_fill(dead, 0.0)
    nrm = None
    if return_normals:
        c = torch.cross(v1 - v0, v2 - v1, dim=-1)
        nrm = (c / c.norm(dim=-1, keepdim=True).clamp(min=_NORMAL_EPS)).masked_fill(dead, 0.0)
    return p, nrm, face, w, cdf


class _SamplePointsFn(torch.autograd.Function):
    """verts -> (samples (N,S,3), normals (N,S,3) or None, face_idx (N,S) int32, w (N,S,3), cdf (F,))
    over the topology's device tables (pr_sample_points_fwd/bwd).  Noise: `uniforms` (N,S,3), or the
    Philox key `seed` (the stream id of the device key base `seeds` when that is given).  The
    backward sorts face_idx on the device into the face -> samples CSR and runs on the forward's
    picks and weights: once-differentiable."""

    @staticmethod
    def _args(nat, v, topo, S):
        a = nat.PRSamplePointsArgs()
        f = topo.faces_packed()
        a.verts, a.faces = nat.ptr(v), nat.ptr(f)
        a.N, a.S, a.V, a.F = len(topo.nfaces), S, v.shape[0], f.shape[0]
        nbytes = nat.load().pr_sample_points_workspace(a.F)
        ws = nat.workspace(nbytes, v.device)
        a.workspace, a.workspace_bytes = nat.ptr(ws), nbytes
        return a, ws  # ws: kept alive by the caller's frame until the launch is enqueued

    @staticmethod
    def forward(ctx, verts, topo, S, want_normals, seed, seeds, uniforms):
        from .. import _native as nat
        nat.require_device(verts, seeds, uniforms)
        v = nat.dense(verts, torch.float32)
        N = len(topo.nfaces)
        a, ws = _SamplePointsFn._args(nat, v, topo, S)  # noqa: F841
        idx = topo.index_tensors()
        a.mesh_first_face, a.mesh_num_faces = nat.ptr(idx["first"]), nat.ptr(idx["nfaces"])
        u = None
        if uniforms is not None:
            if tuple(uniforms.shape) != (N, S, 3) or uniforms.device != v.device:
                raise ValueError(f"uniforms must be ({N},{S},3) on {v.device}, got {tuple(uniforms.shape)} on {uniforms.device}")
            u = nat.dense(uniforms, torch.float32)
            a.noise_mode, a.uniforms = nat.PR_NOISE_INJECTED, nat.ptr(u)
        else:
            a.noise_mode, a.seed, a.seeds = nat.PR_NOISE_PHILOX, int(seed), nat.ptr(seeds)
        new = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=v.device)  # noqa: E731
        samples, w, cdf = new((N, S, 3)), new((N, S, 3)), new((int(a.F),))
        normals = new((N, S, 3)) if want_normals else None
        face_idx = new((N, S), torch.int32)
        a.cdf, a.samples, a.normals, a.face_idx, a.w = (nat.ptr(t) for t in (cdf, samples, normals, face_idx, w))
        nat.call("pr_sample_points_fwd", "pr_sample_points_fwd", v, a)
        ctx.save_for_backward(v, face_idx, w)
        ctx.topo = topo
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(face_idx, w, cdf)
        return samples, normals, face_idx, w, cdf

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_s, g_n, _gf, _gw, _gc):
        from .. import _native as nat
        v, face_idx, w = ctx.saved_tensors
        topo = ctx.topo
        N, S = face_idx.shape
        gv = torch.empty_like(v)
        if g_s is None and g_n is None:
            return gv.zero_(), None, None, None, None, None, None
        g_s = torch.zeros_like(w) if g_s is None else nat.dense(g_s, torch.float32)
        g_n = None if g_n is None else nat.dense(g_n, torch.float32)
        a, ws = _SamplePointsFn._args(nat, v, topo, S)  # noqa: F841
        # the face -> samples CSR of this call: a stable sort (ascending sample order within a face),
        # dead rows keyed F; built on the device, no sync (like _Topology.corner_csr)
        key = face_idx.reshape(-1)
        key = torch.where(key < 0, int(a.F), key)
        order = torch.argsort(key, stable=True)
        start = torch.searchsorted(key[order].contiguous(), topo.face_arange())
        a.w, a.face_sample_start, a.face_samples = nat.ptr(w), nat.ptr(start), nat.ptr(order)
        a.vert_corner_start, a.vert_corners = (nat.ptr(t) for t in topo.corner_csr("gather"))
        a.grad_samples, a.grad_normals, a.grad_verts = nat.ptr(g_s), nat.ptr(g_n), nat.ptr(gv)
        nat.call("pr_sample_points_bwd", "pr_sample_points_bwd", v, a)
        return gv, None, None, None, None, None, None


def _native_ok(meshes, v, S):
    N, F = len(meshes), sum(meshes._topo.nfaces)
    return (_loss._native(v) and 0 < N <= _MAX_MESHES and N * S <= _INT32_MAX and 0 < 3 * F <= _INT32_MAX
            and v.shape[0] > 0)


def sample_points_from_meshes(meshes, num_samples=10000, return_normals=False, *, seed=None, uniforms=None):
    """num_samples points on the surface of every mesh, chosen in proportion to face area
    (PyTorch3D 0.4.0 sample_points_from_meshes; no return_textures): samples (N,S,3), or
    (samples, normals) with return_normals.  Gradients flow to the vertices through the points and
    the face normals; the areas and the choice of faces are constants of the backward.

    Sample s of mesh n comes from three uniforms u in (0,1).  Face: the mesh's inclusive prefix sum
    of the float32 areas 0.5 |(v1 - v0) x (v2 - v0)|, accumulated in float64 and rounded once per
    entry; r = u0 total; the first face whose entry exceeds r (a zero-area face is never picked).
    Point: su = sqrt(u1), w = (1 - su, su (1 - u2), su u2), p = w0 v0 + w1 v1 + w2 v2.  Normal:
    c / max(|c|, 2.2e-16), c = (v1 - v0) x (v2 - v1).  A mesh without faces, or whose areas sum to 0,
    gives zero rows and no gradient; PyTorch3D's multinomial raises on the latter, which would need
    a host read of the total.

    Noise (noise.py).  Default: one Philox4x32-7 block per (n, s), counter (s, n, 0, "SAMP"), keyed
    by noise.draw_key() from torch's CPU generator (torch.manual_seed reproduces a run), or by
    `seed`.  With an active noise.DeviceSeed the native path keys the block by the seed's device
    base and a fresh stream id, so a captured step draws fresh samples on every replay without host
    work (an explicit `seed`, and the torch composition, ignore the device seed).  `uniforms`
    (N,S,3) float32 in [0,1] on the meshes' device are used as given.
    noise.set_noise_source("torch") draws torch.rand((N,S,3)) on the device instead; PyTorch3D's
    own stream (a multinomial, then rand(2,N,S)) is not reproduced by any source.

    On a ROCm device with float32 vertices the native kernels run (csrc/pr_samplepoints.hip;
    float32 out, bitwise reproducible, capturable); otherwise the torch composition, in the
    vertices' dtype.  Arguments are checked (ValueError) before anything is launched."""
    if len(meshes) == 0:
        raise ValueError("meshes is empty")
    if isinstance(num_samples, bool) or not isinstance(num_samples, int) or num_samples <= 0:
        raise ValueError(f"num_samples must be a positive int, got {num_samples!r}")
    v = meshes.verts_packed()
    if not v.is_floating_point() or v.dim() != 2 or v.shape[1] != 3:
        raise ValueError(f"vertices must be floating point (V,3), got {v.dtype} {tuple(v.shape)}")
    N, S = len(meshes), num_samples
    if uniforms is not None:
        if seed is not None:
            raise ValueError("give seed or uniforms, not both")
        if not torch.is_tensor(uniforms) or tuple(uniforms.shape) != (N, S, 3):
            raise ValueError(f"uniforms must be a tensor of shape ({N},{S},3), got "
                             f"{tuple(uniforms.shape) if torch.is_tensor(uniforms) else type(uniforms).__name__}")
        if uniforms.dtype != torch.float32:
            raise ValueError(f"uniforms must be float32, got {uniforms.dtype}")
        if uniforms.device != v.device:
            raise ValueError(f"uniforms is on {uniforms.device}, the meshes on {v.device}")
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64):
        raise ValueError(f"seed must be an int in [0, 2^64), got {seed!r}")
    native = _native_ok(meshes, v, S)
    seeds = None
    if uniforms is None:
        if _noise.get_noise_source() == "torch" and seed is None:
            uniforms = torch.rand((N, S, 3), dtype=torch.float32, device=v.device)
        elif seed is None:
            ds = _noise._DEVICE_SEED
            if native and ds is not None and ds.tensor.device == v.device:
                seed, seeds = ds.stream_id(), ds.tensor
            else:
                seed = _noise.draw_key()
    if native:
        samples, normals = _SamplePointsFn.apply(v, meshes._topo, S, bool(return_normals), seed, seeds, uniforms)[:2]
    else:
        if uniforms is None:
            uniforms = _philox_uniforms(seed, N, S, v.device)
        samples, normals = _sample_points_torch(meshes, uniforms, bool(return_normals))[:2]
    return (samples, normals) if return_normals else samples


# ------------------------------------------------------------------ K nearest neighbours
_KNN = collections.namedtuple("_KNN", "dists idx knn")
_TORCH_CHUNK = 1 << 22  # entries of the (queries, P2) d^2 block the torch composition holds at once


def _check_knn_inputs(p1, p2, lengths1, lengths2, K):
    if not torch.is_tensor(p1) or not torch.is_tensor(p2) or p1.dim() != 3 or p2.dim() != 3:
        raise ValueError("expected p1 (N,P1,D) and p2 (N,P2,D) tensors, got "
                         f"{tuple(p1.shape) if torch.is_tensor(p1) else type(p1).__name__} and "
                         f"{tuple(p2.shape) if torch.is_tensor(p2) else type(p2).__name__}")
    if not p1.is_floating_point() or p1.dtype != p2.dtype:
        raise ValueError(f"p1 and p2 must be floating point of one dtype, got {p1.dtype} and {p2.dtype}")
    if p1.device != p2.device:
        raise ValueError(f"p1 is on {p1.device}, p2 on {p2.device}")
    if p1.shape[0] != p2.shape[0] or p1.shape[2] != p2.shape[2]:
        raise ValueError(f"p1 and p2 must agree in N and D, got {tuple(p1.shape)} and {tuple(p2.shape)}")
    if isinstance(K, bool) or not isinstance(K, int) or K < 1:
        raise ValueError(f"K must be an int >= 1, got {K!r}")
    for t, name in ((lengths1, "lengths1"), (lengths2, "lengths2")):
        if t is None:
            continue
        if not torch.is_tensor(t) or tuple(t.shape) != (p1.shape[0],) or t.is_floating_point() or t.is_complex() \
                or t.dtype == torch.bool:
            raise ValueError(f"{name} must be an integer tensor of shape ({p1.shape[0]},), got "
                             f"{(t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__}")
        if t.device != p1.device:
            raise ValueError(f"{name} is on {t.device}, p1 on {p1.device}")


def _knn_points_torch(p1, p2, lengths1=None, lengths2=None, K=1):
    """knn_points in torch ops, in the inputs' dtype: (dists (N,P1,K), idx (N,P1,K) int64, -1
    where a slot holds no neighbour).  Per cloud and per chunk of queries (no (N,P1,P2) tensor):
    d^2 summed coordinate by coordinate, NaN and padded columns at +inf, the K smallest by topk's
    kth value with the lowest indices among the entries equal to it, then a stable sort of those K
    (the lowest index first on equal d^2; topk's tie order is not relied on).  The distances are then
    formed again from the chosen points, which is what autograd differentiates; the lengths are
    read on the device."""
    N, P1, D = p1.shape
    P2, Kc = p2.shape[1], min(K, p2.shape[1])
    dev, inf = p1.device, float("inf")
    with torch.no_grad():
        l1 = torch.full((N,), P1, dtype=torch.int64, device=dev) if lengths1 is None else lengths1.to(torch.int64).clamp(0, P1)
        l2 = torch.full((N,), P2, dtype=torch.int64, device=dev) if lengths2 is None else lengths2.to(torch.int64).clamp(0, P2)
        idx = torch.full((N, P1, K), -1, dtype=torch.int64, device=dev)
        cols = torch.arange(P2, device=dev)
        step = max(1, _TORCH_CHUNK // max(P2, 1))
        for n in range(N if Kc > 0 else 0):
            dead = (cols >= l2[n])[None, :]
            for c0 in range(0, P1, step):
                q = p1[n, c0:c0 + step]
                d = torch.zeros((q.shape[0], P2), dtype=p1.dtype, device=dev)
                for c in range(D):
                    diff = q[:, c, None] - p2[n, None, :, c]
                    d = d + diff * diff
                d = torch.where(dead | torch.isnan(d), inf, d)
                # the K smallest under (d^2, index) without sorting the row: topk gives the kth value t
                # (its choice among equal values is not used); everything below t is in, and of the
                # entries equal to t the lowest indices fill the rest
                t = torch.topk(d, Kc, dim=1, largest=False).values[:, -1:]
                below, equal = d < t, d == t
                chosen = below | (equal & (equal.cumsum(1) <= Kc - below.sum(1, keepdim=True)))
                # exactly Kc per row; their indices in ascending order, as the Kc largest of P2 - j
                j = P2 - torch.topk(torch.where(chosen, P2 - cols, 0), Kc, dim=1).values
                val, order = torch.sort(d.gather(1, j), dim=1, stable=True)  # ascending index within equal d^2
                j = j.gather(1, order)
                idx[n, c0:c0 + step, :Kc] = torch.where(val < inf, j, -1)
        slot = torch.arange(K, device=dev)[None, None, :] < l2.clamp(max=K)[:, None, None]
        live = (torch.arange(P1, device=dev)[None, :] < l1[:, None])[:, :, None] & slot
        idx = torch.where(live, idx, -1)
        found = idx >= 0
        miss = torch.where(torch.isnan(p1).any(dim=2, keepdim=True), float("nan"), inf).to(p1.dtype).expand(N, P1, K)
        fill = torch.where(live, miss, torch.zeros((), dtype=p1.dtype, device=dev))
    near = p2[torch.arange(N, device=dev)[:, None, None], idx.clamp(min=0)]  # (N,P1,K,D), indexed: see loss._normal_terms
    diff = (p1[:, :, None, :] - near).masked_fill(~found[..., None], 0.0)
    d = torch.zeros((N, P1, K), dtype=p1.dtype, device=dev)
    for c in range(D):
        d = d + diff[..., c] * diff[..., c]
    return torch.where(found, d, fill), idx


def knn_gather(x, idx, lengths=None):
    """out[n,l,k] = x[n, idx[n,l,k]] for x (N,M,U) and idx (N,L,K): (N,L,K,U) (PyTorch3D 0.4.0
    knn_gather).  With lengths (N,), the slots k >= lengths[n] are zero.  Torch index ops on the
    device, no host read; the backward is autograd's index backward."""
    if not torch.is_tensor(x) or not torch.is_tensor(idx) or x.dim() != 3 or idx.dim() != 3 or x.shape[0] != idx.shape[0]:
        raise ValueError("expected x (N,M,U) and idx (N,L,K)")
    if idx.is_floating_point() or idx.dtype == torch.bool:
        raise ValueError(f"idx must be an integer tensor, got {idx.dtype}")
    N, K = idx.shape[0], idx.shape[2]
    out = x[torch.arange(N, device=x.device)[:, None, None], idx.to(torch.int64)]
    if lengths is not None:
        if not torch.is_tensor(lengths) or tuple(lengths.shape) != (N,) or lengths.is_floating_point() or lengths.dtype == torch.bool:
            raise ValueError(f"lengths must be an integer tensor of shape ({N},)")
        pad = torch.arange(K, device=x.device)[None, None, :] >= lengths.to(x.device)[:, None, None]
        out = out.masked_fill(pad.expand(idx.shape)[..., None], 0.0)
    return out


def knn_points(p1, p2, lengths1=None, lengths2=None, K=1, version=-1, return_nn=False, return_sorted=True):
    """The K nearest neighbours in p2 (N,P2,D) of every point of p1 (N,P1,D) (PyTorch3D 0.4.0
    knn_points): a namedtuple (dists (N,P1,K), idx (N,P1,K) int64, knn (N,P1,K,D) or None).

    dists are the squared Euclidean distances, ascending; neighbours are ordered by (d^2, index), so
    equal distances come out lowest index first.  d^2 is the sum over the coordinates, in order, of
    the squared differences: a point on top of its neighbour gives exactly 0.  lengths1 / lengths2
    (N,) integer tensors give the clouds' lengths (read on the device, clamped to [0, P]); rows
    i >= lengths1[n] and slots k >= min(K, lengths2[n]) have dists 0 and idx 0 (_knn_points_torch's
    own idx holds -1 there, and the gradient skips such entries).  K > P2 is allowed.  A NaN database
    point is never chosen; a live slot that finds no neighbour below +inf gets NaN if its query is
    NaN, else +inf, and no gradient.  dists is differentiable in p1 and p2, and so is knn
    (return_nn=True: knn_gather(p2, idx, lengths2)).  `version` (-1..3) is accepted and ignored, and
    return_sorted=False still returns the sorted order.

    Every device and dtype takes the torch composition of these formulas (_knn_points_torch): per
    cloud and per chunk of queries, so no (N,P1,P2) tensor is held at once, with no host read of the
    lengths in the forward; capture in a HIP graph is untested.  There is no native kernel for this
    op yet.  Arguments are checked (ValueError) before
    anything is launched.  Parity with PyTorch3D is unpinned (not installable here)."""
    _check_knn_inputs(p1, p2, lengths1, lengths2, K)
    if isinstance(version, bool) or not isinstance(version, int) or not -1 <= version <= 3:
        raise ValueError(f"version must be an int in -1..3, got {version!r}")
    dists, raw = _knn_points_torch(p1, p2, lengths1, lengths2, K)
    idx = raw.clamp(min=0)
    return _KNN(dists, idx, knn_gather(p2, idx, lengths2) if return_nn else None)

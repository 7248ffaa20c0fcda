"""Shared by the mesh-regulariser tests (not a test module): the small meshes, brute-force
topology, and the dense restatement of the losses' formulas.

The restatement builds a dense (V,V) weight matrix L with index_put_(accumulate=True), forms
L.mm(v) and lets autograd supply the gradients.  Run in float64 on float32 inputs it is the
reference; run in float32 it measures how far float32 itself is from float64 on a case, which is
what the native kernels' gradient tolerance is derived from (tests/test_gpu_mesh_losses.py)."""
import functools
import os

import torch

from conftest import GOLDEN


def _grid(n, seed):
    """Open n x n quad grid (two triangles per quad), jittered off the plane."""
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(n + 1.0), torch.arange(n + 1.0), indexing="ij")
    v = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.zeros((n + 1) ** 2)], 1)
    v = v + 0.2 * torch.rand(v.shape, generator=g)
    f = []
    for y in range(n):
        for x in range(n):
            a = y * (n + 1) + x
            f += [[a, a + 1, a + n + 2], [a, a + n + 2, a + n + 1]]
    return v, torch.tensor(f)


def _hub(n, seed):
    """A closed fan: vertex 0 with n neighbours on a jittered ring (a CSR row longer than a wave)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n) * (2 * torch.pi / n)
    ring = torch.stack([torch.cos(t), torch.sin(t), torch.zeros(n)], 1) + 0.05 * torch.rand((n, 3), generator=g)
    v = torch.cat([torch.tensor([[0.03, -0.02, 0.4]]), ring])
    f = torch.tensor([[0, 1 + i, 1 + (i + 1) % n] for i in range(n)])
    return v, f


_TRI = (torch.tensor([[0.1, 0.0, 0.2], [1.0, 0.1, 0.0], [0.2, 0.9, -0.1]]), torch.tensor([[0, 1, 2]]))
_TET = (torch.tensor([[0.0, 0.0, 0.1], [1.1, 0.0, 0.0], [0.1, 0.9, 0.0], [0.2, 0.3, 1.2]]),
        torch.tensor([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]]))
# edge (0,1) is shared by three faces
_FAN = (torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.4, 1.0, 0.1], [0.5, -0.9, 0.3], [0.6, 0.1, 1.1]]),
        torch.tensor([[0, 1, 2], [1, 0, 3], [0, 1, 4]]))
_ISOLATED = (torch.cat([_TET[0], torch.tensor([[3.0, 2.0, 1.0]])]), _TET[1])


@functools.lru_cache(maxsize=None)
def case(name):
    """(list of (V_i,3) float32 verts, list of (F_i,3) int64 faces)."""
    if name == "sphere_642":
        from pertrenderer_amd.renderer import load_obj
        v, f, _ = load_obj(os.path.join(GOLDEN, "sphere_642.obj"))
        return [v.float() * torch.tensor([1.0, 0.7, 1.3])], [f.verts_idx]
    single = {"triangle": _TRI, "tetrahedron": _TET, "grid3": _grid(3, 1), "fan3": _FAN, "isolated": _ISOLATED,
              "hub70": _hub(70, 2)}
    if name in single:
        v, f = single[name]
        return [v.float()], [f]
    if name == "batch2":  # different V and E
        return [_TET[0].float(), _grid(3, 3)[0].float()], [_TET[1], _grid(3, 3)[1]]
    raise KeyError(name)


TOPOLOGY_CASES = ["triangle", "tetrahedron", "grid3", "fan3", "isolated", "batch2"]
LOSS_CASES_CPU = TOPOLOGY_CASES + ["sphere_642"]
LOSS_CASES_GPU = ["triangle", "tetrahedron", "grid3", "fan3", "batch2", "sphere_642", "hub70"]


def packed(verts, faces):
    offs, out = 0, []
    for v, f in zip(verts, faces):
        out.append(f + offs)
        offs += v.shape[0]
    return torch.cat(verts), torch.cat(out)


def brute_edges(faces_packed):
    """Sorted list of the unique undirected edges (a < b), from Python sets."""
    s = set()
    for a, b, c in faces_packed.tolist():
        for x, y in ((a, b), (b, c), (c, a)):
            s.add((min(x, y), max(x, y)))
    return sorted(s)


def _vert_mesh(verts):
    return torch.cat([torch.full((v.shape[0],), i, dtype=torch.int64) for i, v in enumerate(verts)])


def _cots(v, f):
    with torch.no_grad():
        v0, v1, v2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        A, B, C = (v1 - v2).norm(dim=1), (v0 - v2).norm(dim=1), (v0 - v1).norm(dim=1)
        s = (A + B + C) / 2
        area = (s * (s - A) * (s - B) * (s - C)).clamp(min=1e-12).sqrt()
        cot = torch.stack([B * B + C * C - A * A, A * A + C * C - B * B, A * A + B * B - C * C], 1) / (4 * area)[:, None]
    return cot, area


def ref_laplacian(verts, faces, method, dtype=torch.float64):
    """(loss, d loss / d packed verts) of the dense restatement in `dtype`."""
    v32, f = packed(verts, faces)
    v = v32.to(dtype).requires_grad_(True)
    V = v.shape[0]
    L = torch.zeros((V, V), dtype=dtype)
    if method == "uniform":
        e = torch.tensor(brute_edges(f)).reshape(-1, 2)
        L.index_put_((e[:, 0], e[:, 1]), torch.ones(e.shape[0], dtype=dtype), accumulate=True)
        L = L + L.t()
        lap = L.mm(v) / L.sum(1).clamp(min=1.0)[:, None] - v
    else:
        cot, area = _cots(v, f)
        # the cot at corner c weighs the edge opposite to it
        ii, jj = f[:, [1, 2, 0]].reshape(-1), f[:, [2, 0, 1]].reshape(-1)
        L.index_put_((ii, jj), cot.reshape(-1), accumulate=True)
        L = L + L.t()
        r = L.sum(1)
        if method == "cot":
            lap = L.mm(v) * torch.where(r > 0, 1 / r, r)[:, None] - v
        else:
            a = torch.zeros(V, dtype=dtype).index_put_((f.reshape(-1),), area.repeat_interleave(3), accumulate=True)
            lap = (L.mm(v) - r[:, None] * v) * (0.25 * torch.where(a > 0, 1 / a, a))[:, None]
    w = torch.tensor([1.0 / x.shape[0] for x in verts], dtype=dtype)[_vert_mesh(verts)]
    loss = (lap.norm(dim=1) * w).sum() / len(verts)
    (g,) = torch.autograd.grad(loss, v)
    return loss.detach(), g


def ref_edge(verts, faces, target, dtype=torch.float64, per_mesh=True):
    """(1/N) sum_m (1/E_m) sum_e (|e| - target)^2 (per_mesh) or the mean over all edges, with its gradient;
    the edges are the non-zeros of the upper triangle of the dense adjacency matrix."""
    v32, f = packed(verts, faces)
    v = v32.to(dtype).requires_grad_(True)
    V = v.shape[0]
    A = torch.zeros((V, V), dtype=dtype)
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    A.index_put_((e.min(1).values, e.max(1).values), torch.ones(e.shape[0], dtype=dtype), accumulate=True)
    e = torch.triu(A, 1).nonzero()
    sq = ((v[e[:, 0]] - v[e[:, 1]]).norm(dim=1) - target) ** 2
    if per_mesh:
        m = _vert_mesh(verts)[e[:, 0]]
        ne = torch.bincount(m, minlength=len(verts)).to(dtype)
        loss = (sq / ne[m]).sum() / len(verts)
    else:
        loss = sq.mean()
    (g,) = torch.autograd.grad(loss, v)
    return loss.detach(), g


def rel_err(a, b):
    """max |a - b| over max |b|."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-300)).item()

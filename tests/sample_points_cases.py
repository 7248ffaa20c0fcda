"""Shared by the sample_points_from_meshes tests (not a test module): the meshes, the expected
uniforms of the documented Philox layout (oracle/philox_ref.py), and the reference runs of the
torch composition (renderer/ops.py _sample_points_torch), computed once and never modified.

Meshes.
  "sphere_cube": sphere_642 scaled 1.3 and shifted 0.1 (1280 faces: more than one chunk of the
      kernels' per-mesh scan) and a 12-face cube: two lengths in one launch.
  "dyadic": an 8 x 8 grid of 2^-3 squares split into 128 right triangles (area 2^-7 each), one
      triangle with legs 4 (area 8 of a total 9) at face index 60, and four zero-area faces: index 5
      (a repeated vertex), a collinear one and one with all corners on one vertex before the last
      two grid triangles, and a trailing one at the very end (F = 133).  Every area and every prefix
      sum is exact in float32, so float32 and float64 must pick the same face for every sample.
  "dead": the cube, a mesh without faces, a mesh whose faces all have zero area, the cube again."""
import functools
import os

import numpy as np
import torch

from conftest import GOLDEN
from oracle import philox_ref

TAG_SAMP = 0x53414D50
SEED = 1234
BIG_FACE = 60
DEGENERATE = (5, 128, 129, 132)  # face indices of "dyadic"
LAST_LIVE = 131


def _cube():
    v = torch.tensor([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)]) * torch.tensor([1.0, 0.8, 1.5]) - 0.4
    f = torch.tensor([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6],
                      [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])
    return v.float(), f


def _dyadic():
    n, h = 8, 0.125
    v = [[x * h, y * h, 0.0] for y in range(n + 1) for x in range(n + 1)]
    f = []
    for y in range(n):
        for x in range(n):
            a = y * (n + 1) + x
            f += [[a, a + 1, a + n + 2], [a, a + n + 2, a + n + 1]]
    b = len(v)
    v += [[0.0, 0.0, 1.0], [4.0, 0.0, 1.0], [0.0, 4.0, 1.0]]
    f.insert(5, [3, 3, 12])               # a repeated vertex
    f.insert(BIG_FACE, [b, b + 1, b + 2])  # legs 4: area 8
    f[-2:-2] = [[0, 1, 2], [40, 40, 40]]  # collinear; all corners on one vertex
    f.append([80, 80, 80])                # trailing
    return torch.tensor(v, dtype=torch.float32), torch.tensor(f)


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(list of (V_i,3) float32 verts, list of (F_i,3) int64 faces)."""
    if name == "sphere_cube":
        from pertrenderer_amd.renderer import load_obj
        v, f, _ = load_obj(os.path.join(GOLDEN, "sphere_642.obj"))
        cv, cf = _cube()
        return [v.float() * 1.3 + 0.1, cv], [f.verts_idx, cf]
    if name == "dyadic":
        v, f = _dyadic()
        return [v], [f]
    if name == "dead":
        cv, cf = _cube()
        flat = torch.tensor([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0]])
        return ([cv, cv[:3].clone(), flat, cv + 2.0],
                [cf, torch.zeros((0, 3), dtype=torch.int64), torch.tensor([[0, 1, 2], [1, 1, 2]]), cf])
    raise KeyError(name)


def meshes(name, device="cpu", dtype=torch.float32, requires_grad=False):
    from pertrenderer_amd.renderer import Meshes
    v, f = mesh(name)
    return Meshes([x.to(device=device, dtype=dtype).requires_grad_(requires_grad) for x in v], [x.to(device) for x in f])


@functools.lru_cache(maxsize=None)
def philox_uniforms(N, S, seed=SEED):
    """(N,S,3) float32: counter (s, n, 0, "SAMP"), key = seed, u01 of words 0, 1, 2."""
    w = philox_ref.block(seed, np.arange(S)[None, :], np.arange(N)[:, None], 0, TAG_SAMP)
    return torch.from_numpy(philox_ref.u01(w[..., :3]).astype(np.float32))


@functools.lru_cache(maxsize=None)
def uniforms(name, S):
    """The Philox uniforms of seed 1234; on "dyadic" (S >= 3) the first three u0 are planted:
    2^-24, 1 - 2^-24 and 1.0 (the last must land on the last face with area, LAST_LIVE)."""
    u = philox_uniforms(len(mesh(name)[0]), S).clone()
    if name == "dyadic" and S >= 3:
        u[0, :3, 0] = torch.tensor([2.0 ** -24, 1.0 - 2.0 ** -24, 1.0])
    return u


def cotangents(N, S, seed=7):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((N, S, 3), generator=g), torch.randn((N, S, 3), generator=g)


@functools.lru_cache(maxsize=None)
def reference(name, S, dtype=torch.float64):
    """The composition on the CPU in `dtype` from uniforms(name, S): dict(samples, normals, face, w,
    cdf, grad) with grad = d (sum samples . gs + sum normals . gn) / d packed verts."""
    from pertrenderer_amd.renderer.ops import _sample_points_torch
    m = meshes(name, dtype=dtype, requires_grad=True)
    p, nrm, face, w, cdf = _sample_points_torch(m, uniforms(name, S), True)
    gs, gn = cotangents(p.shape[0], S)
    grads = torch.autograd.grad((p * gs.to(dtype)).sum() + (nrm * gn.to(dtype)).sum(), m.verts_list(), allow_unused=True)
    grads = [torch.zeros_like(v) if g is None else g for g, v in zip(grads, m.verts_list())]
    return dict(samples=p.detach(), normals=nrm.detach(), face=face, w=w, cdf=cdf, grad=torch.cat(grads))


def chi_square(face, areas, first, nf, S):
    """The chi^2 statistic of one mesh's face counts against S a_f / total over the faces with area."""
    a = areas[first:first + nf].double()
    cnt = torch.bincount(face[face >= 0] - first, minlength=nf).double()
    exp = S * a / a.sum()
    live = exp > 0
    assert cnt[~live].sum() == 0
    return (((cnt - exp) ** 2)[live] / exp[live]).sum().item(), int(live.sum()) - 1


def face_areas(name):
    v, f = mesh(name)
    out = []
    for x, t in zip(v, f):
        x = x.double()
        out.append(0.5 * torch.cross(x[t[:, 1]] - x[t[:, 0]], x[t[:, 2]] - x[t[:, 0]], dim=1).norm(dim=1))
    return torch.cat(out)

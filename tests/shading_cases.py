"""Hand-built fragments and the float64 reference of the Phong shading kernels' tests (pr_shade_fwd /
pr_shade_bwd, csrc/pr_shade.hip and pr_phong.h): test_shading_cases_cpu.py pins the reference and the
cases' conditioning on the CPU, test_gpu_shading_cases.py compares the kernels with it.

The shading functions take pix_to_face, the barycentrics and the attached valid-prefix counts as plain
inputs, so a case needs no rasterizer: every slot's face, barycentrics and liveness are drawn (from a
seeded generator) to reach the kernels' layout and arithmetic branches at frames of a few dozen pixels
-- pixel blocks that hold two images, 16-byte stores that cover a live and a padded slot, per-image
lights / materials / maps that all differ, UVs beyond the map, slots exactly on a texel line, poisoned
padding, slots whose d colour is exactly zero, a face whose normals are exactly zero.

shade_ref64 widens the float32 inputs the kernel sees to float64 and evaluates PyTorch3D's
phong_shading composition there, so the only difference left is the kernel's own float32 arithmetic.
The builder keeps every live slot away from the composition's branch points (`conditions`), so that
float32 and float64 take the same branch: it redraws inputs, it never masks outputs.  Importing this
module needs no GPU."""
import collections
import functools
import types

import numpy as np
import torch
import torch.nn.functional as Fn

import meshgen

F32, F64 = torch.float32, torch.float64

HM, WM = 5, 9  # map size: k/4 and k/8 are exact texel coordinates
SHININESS = (1.0, 4.0, 32.0, 64.0)
EXACT_U = (0.0, 0.125, 0.5, 1.0)  # low clamp, texel lines 1 and 4 of 0..8, high clamp
EXACT_V = (0.0, 0.25, 0.5, 1.0)   # low clamp, texel lines 1 and 2 of 0..4, high clamp
BLK_PIX = 64  # pr_shade.hip kBlkPix
PAD_IMGS = 256  # pr_shade.hip kPadImgs
LDS_FLOATS = 8192  # pr_phong.h kLdsFloats

# the builder's conditions (float64) on every live slot ...
MIN_COS = 1e-3      # |cos angle| and |view . reflect|
MIN_TEXEL = 1e-3    # map coordinates from a texel line, from 0 and from size - 1 (texels)
MIN_NORMAL = 0.1    # |interpolated normal|
# ... and the shares of the live slots on each side of a branch
SHARE_COS, SHARE_REFLECT, SHARE_UV = 0.20, 0.10, 0.05

COLOUR_BAR, GRAD_BAR = 5e-6, 2e-4  # |err| <= bar * max|ref| (test_gpu_shading.py's bars)

Spec = collections.namedtuple("Spec", "N H W K tex light mesh shared seed", defaults=("sphere", False, 0))


def spec_id(s):
    return f"{s.N}x{s.H}x{s.W}x{s.K}-{s.tex}-{s.light}-{s.mesh}{'-shared' if s.shared else ''}"


# the geometry cross of test_gpu_shading_cases.py (N, H, W, K): (3,5,7,5) is 105 pixels, one full block
# that holds an image boundary and a 41-pixel tail; K = 12 is the multiple-of-4 control; K = 1, 64, 65 are
# the chunk kernels' step64 edges (q64 = 64; r64 = 0; q64 = 0)
MAIN = (3, 5, 7, 5)
GEOMETRIES = (MAIN, (3, 5, 7, 1), (3, 5, 7, 3), (2, 9, 9, 10), (1, 8, 8, 12), (2, 3, 5, 64), (3, 5, 7, 65))
FULL_CROSS = tuple(Spec(*MAIN, tex, light) for tex, light in
                   (("uv", "point"), ("vertex", "point"), ("given", "point"), ("uv", "directional"),
                    ("vertex", "directional")))
OTHER_GEOMETRIES = tuple(Spec(*g, tex, "point") for g in GEOMETRIES[1:] for tex in ("uv", "vertex"))
# the backward's accumulator layouts (pr_shade_bwd's Tab): name -> (spec, (useV, useB))
ACCUMULATORS = collections.OrderedDict([
    ("lds-verts+lds-batch", (Spec(3, 5, 7, 5, "vertex", "point", "sphere", True), (True, True))),
    ("atomic-verts+lds-batch-1", (Spec(1, 5, 7, 5, "vertex", "point", "sphere2562"), (False, True))),
    ("atomic-verts+lds-batch-3", (Spec(3, 5, 7, 5, "vertex", "point", "sphere2562"), (False, True))),
    ("lds-verts+atomic-batch", (Spec(342, 1, 2, 3, "vertex", "point", "sphere", True), (True, False))),
    ("atomic-verts+atomic-batch", (Spec(342, 1, 2, 3, "vertex", "point", "sphere2562", True), (False, False))),
    ("past-pad-table", (Spec(257, 1, 2, 3, "vertex", "point", "sphere", True), (True, True))),
])
DETERMINISTIC = tuple(Spec(*MAIN, tex, "point") for tex in ("uv", "vertex"))
DEGENERATE = tuple(Spec(*MAIN, tex, "point", "sphere+line") for tex in ("uv", "vertex", "given"))
DET_BATCH = 37  # slots per deterministic batch: no multiple of K = 5, a batch boundary inside a pixel


def all_specs():
    """Every case test_gpu_shading_cases.py runs (test_shading_cases_cpu.py checks the same list)."""
    out = list(FULL_CROSS) + list(OTHER_GEOMETRIES) + [s for s, _ in ACCUMULATORS.values()]
    out += list(DETERMINISTIC) + list(DEGENERATE)
    return list(collections.OrderedDict.fromkeys(out))


def accumulator_layout(V, N):
    """(useV, useB) of pr_shade_bwd: per-vertex / per-image sums in the LDS table or global atomics."""
    return V * 9 + N * 6 <= LDS_FLOATS, N * 6 <= LDS_FLOATS // 4


# ------------------------------------------------------------------------------------ meshes
@functools.lru_cache(maxsize=None)
def _sphere(level):
    v, f = meshgen.load_sphere()
    if level:
        v, f = meshgen.subdivide(v, f, level)
    v = torch.from_numpy(v).to(F64)
    return (v - v.mean(0)).to(F32), torch.from_numpy(f).to(torch.int64)


# the isolated face of the degenerate case: collinear, small integers, so the corner crosses, the
# vertex normals and every interpolated normal are exactly 0 in float32 and float64
LINE = ((2.0, 2.0, 2.0), (3.0, 3.0, 3.0), (5.0, 5.0, 5.0))


def _mesh(kind, n):
    """Image n's mesh (V,3) float32, (F,3) int64: the sphere under a per-image scale, so that a face
    id of another image's mesh shades differently."""
    v, f = _sphere(1 if kind == "sphere2562" else 0)
    scale = torch.tensor([1.0 + 0.11 * n, 1.0 - 0.07 * n, 1.0 + 0.05 * n]) / (1.0 + 0.04 * n)
    v = (v * scale).to(F32)
    if kind == "sphere+line":
        f = torch.cat([f, torch.tensor([[v.shape[0], v.shape[0] + 1, v.shape[0] + 2]])], 0)
        v = torch.cat([v, torch.tensor(LINE, dtype=F32)], 0)
    return v, f


# ------------------------------------------------------------------------------------ cameras
def camera_centers(R, T):
    """Centres (N,3) of world -> view X R + T: -T R^T (cameras.get_camera_center's values)."""
    return -torch.bmm(T[:, None, :], R.transpose(1, 2))[:, 0]


def _cameras(N):
    from pertrenderer_amd.renderer import look_at_view_transform
    n = torch.arange(N, dtype=F32)
    dist, elev, azim = 2.4 + 0.35 * (n % 5), -30.0 + 17.0 * (n % 7), (20.0 + 47.0 * n) % 360.0
    R, T = look_at_view_transform(dist, elev, azim)
    return R.to(F32), T.to(F32), dist, elev, azim


def _lights(N, kind, dist, elev, azim, g):
    """Per-image light rows: 35 to 75 degrees of azimuth and 10 to 40 of elevation from the camera,
    so that a fair part of what the light reaches reflects towards the camera and a fair part away."""
    da = 35.0 + 40.0 * torch.rand(N, generator=g)
    de = 10.0 + 30.0 * torch.rand(N, generator=g)
    az, el = torch.deg2rad(azim + da), torch.deg2rad(elev + de)
    d = torch.stack([torch.cos(el) * torch.sin(az), torch.sin(el), torch.cos(el) * torch.cos(az)], 1)
    r = (3.0 + 3.0 * torch.rand(N, generator=g))[:, None] if kind == "point" else 0.5 + torch.rand((N, 1), generator=g)
    return (d * r).to(F32)


# -------------------------------------------------------------------------------- the builder
def _bary(g, n):
    """Positive, normalised barycentrics; cubed uniforms, so that one corner often dominates and the
    interpolated UVs keep most of the vertices' spread."""
    r = torch.rand((n, 3), generator=g, dtype=F64) ** 3 + 1e-3
    return (r / r.sum(1, keepdim=True)).to(F32)


def mixed_float4s(counts, K):
    """The 16-byte stores of fill_padded (pr_shade.hip) that cover one padded and one live slot, from the
    counts (N,H,W): float4 q of a 64-pixel block holds floats of block slots 4q // 3 and 4q // 3 + 1.
    Returns dict(within=.., pixel=.., image=.., split=..): mixed float4s whose two slots share a pixel /
    lie in two pixels of one image / in two images, and `split`: float4s whose two slots are both
    padded but of two images (written component by component as well)."""
    N, H, W = counts.shape
    c = counts.reshape(-1).tolist()
    P, HW = N * H * W, H * W
    out = dict(within=0, pixel=0, image=0, split=0)
    for p0 in range(0, P, BLK_PIX):
        npix = min(BLK_PIX, P - p0)
        nf = npix * K * 3
        for q in range((nf + 3) // 4):
            sa = 4 * q // 3
            if sa + 1 >= npix * K:
                continue
            pa, ka = divmod(sa, K)
            pb, kb = divmod(sa + 1, K)
            pad_a, pad_b = ka >= c[p0 + pa], kb >= c[p0 + pb]
            na, nb = (p0 + pa) // HW, (p0 + pb) // HW
            if pad_a != pad_b:
                out["within" if pa == pb else ("pixel" if na == nb else "image")] += 1
            elif pad_a and na != nb:
                out["split"] += 1
    return out


def composition(c, v, b, tex_leaf, light, T, live=None):
    """The composition on tensors of one dtype (float64: the reference; float32: torch's own float32
    composition), leaves or not; returns a namespace of the colours, the texels and the intermediates
    the conditions are stated on."""
    dt = v.dtype
    live = c.live if live is None else live
    m = live[..., None]
    faces = c.faces
    fv = faces[torch.where(live, c.p2f, torch.zeros_like(c.p2f))]  # (N,H,W,K,3)
    # area-weighted vertex normals (Meshes.verts_normals_packed)
    tri = v[faces]
    raw = torch.zeros_like(v)
    raw = raw.index_add(0, faces[:, 1], torch.cross(tri[:, 2] - tri[:, 1], tri[:, 0] - tri[:, 1], dim=1))
    raw = raw.index_add(0, faces[:, 2], torch.cross(tri[:, 0] - tri[:, 2], tri[:, 1] - tri[:, 2], dim=1))
    raw = raw.index_add(0, faces[:, 0], torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1))
    vn = Fn.normalize(raw, eps=1e-6, dim=1)
    zero = torch.zeros((), dtype=dt)

    def interp(attr, corners=fv):
        o = (b[..., 0:1] * attr[corners[..., 0]] + b[..., 1:2] * attr[corners[..., 1]]) + b[..., 2:3] * attr[corners[..., 2]]
        return torch.where(m, o, zero)

    z = types.SimpleNamespace()
    z.P, z.Nn = interp(v), interp(vn)
    rows = lambda t: t.to(dt)[:, None, None, None, :]
    L = light[:, None, None, None, :]
    direction = L.expand_as(z.P) if c.spec.light == "directional" else L - z.P
    n, d = Fn.normalize(z.Nn, eps=1e-6, dim=-1), Fn.normalize(direction, eps=1e-6, dim=-1)
    z.cos = (n * d).sum(-1)
    diffuse = rows(c.light_diffuse) * Fn.relu(z.cos)[..., None]
    centre = camera_centers(c.R.to(dt), T)[:, None, None, None, :]
    view = Fn.normalize(centre - z.P, eps=1e-6, dim=-1)
    reflect = -d + 2 * (z.cos[..., None] * n)
    z.dotvr = (view * reflect).sum(-1)
    alpha = Fn.relu(z.dotvr) * (z.cos > 0).to(dt)
    specular = rows(c.light_specular) * torch.pow(alpha, c.shininess.to(dt)[:, None, None, None])[..., None]
    if c.spec.tex == "uv":
        fuv = c.verts_uvs.to(dt)  # per-vertex UVs, packed like the vertices (faces_uvs = faces)
        z.uv = interp(fuv)
        N, H, W, K = c.p2f.shape
        grid = z.uv.reshape(N, H, W * K, 2) * 2.0 - 1.0
        t = Fn.grid_sample(torch.flip(tex_leaf.permute(0, 3, 1, 2), [2]), grid, align_corners=True, padding_mode="border")
        z.texels = t.reshape(N, 3, H, W, K).permute(0, 2, 3, 4, 1)
    elif c.spec.tex == "vertex":
        z.texels = interp(tex_leaf)
    else:
        z.texels = tex_leaf
    ambient = rows(c.ambient)  # the float32 product the kernel is given
    z.colours = (ambient + rows(c.mat_diffuse) * diffuse) * z.texels + rows(c.mat_specular) * specular
    return z


def leaves(c, dtype=F64):
    """The differentiable inputs of the composition as fresh `dtype` leaves (padded slots: zero bary)."""
    w = lambda t: t.detach().to(dtype).clone().requires_grad_(True)
    live = c.live
    b = torch.where(live[..., None], c.bary, torch.zeros((), dtype=F32))
    return dict(bary=w(b), verts=w(c.verts), tex=w(c.tex), light=w(c.light), T=w(c.T))


def conditions(c):
    """The conditions the builder enforces, evaluated in float64: a dict of per-slot boolean masks
    (`bad`: live slots that break one) and the shares of the live slots on each side of a branch."""
    with torch.no_grad():
        l = {k: t.detach() for k, t in leaves(c).items()}
        z = composition(c, l["verts"], l["bary"], l["tex"], l["light"], l["T"])
    live = c.live & ~c.degenerate
    bad = live & ((z.cos.abs() < MIN_COS) | (z.dotvr.abs() < MIN_COS) | (z.Nn.norm(dim=-1) < MIN_NORMAL))
    out = dict(cos=z.cos, dotvr=z.dotvr)
    n = max(int(live.sum()), 1)
    lit = live & (z.cos > 0)
    shares = dict(lit=float(lit.sum()) / n, unlit=float((live & (z.cos < 0)).sum()) / n,
                  reflect=float((lit & (z.dotvr > 0)).sum()) / max(int(lit.sum()), 1),
                  no_reflect=float((lit & (z.dotvr < 0)).sum()) / max(int(lit.sum()), 1))
    if c.spec.tex == "uv":
        for axis, size, name in ((0, WM, "u"), (1, HM, "v")):
            x = z.uv[..., axis] * (size - 1)  # unclamped map coordinate, texels
            inside = (x > 0) & (x < size - 1)
            near = torch.where(inside, (x - x.round()).abs(), torch.minimum(x.abs(), (x - (size - 1)).abs())) < MIN_TEXEL
            bad = bad | (live & ~c.exact & near)
            out["i" + name] = x
            gen = live & ~c.exact
            g = max(int(gen.sum()), 1)
            shares.update({name + "_low": float((gen & (x < 0)).sum()) / g, name + "_high": float((gen & (x > size - 1)).sum()) / g,
                           name + "_inside": float((gen & inside).sum()) / g})
    out.update(bad=bad, shares=shares)
    return out


def share_floor(name):
    return SHARE_COS if name in ("lit", "unlit") else SHARE_REFLECT if name.endswith("reflect") else SHARE_UV


@functools.lru_cache(maxsize=None)
def build(spec):
    """The case of `spec` as a namespace of CPU tensors (float32 / int64 / int32), deterministic under
    the seeded generator; see the module docstring and `conditions`."""
    N, H, W, K = spec.N, spec.H, spec.W, spec.K
    g = torch.Generator().manual_seed(1000 + spec.seed)
    c = types.SimpleNamespace(spec=spec)
    meshes = [_mesh(spec.mesh, 0)] if spec.shared else [_mesh(spec.mesh, n) for n in range(N)]
    c.verts_list = [v for v, _ in meshes]
    c.faces_list = [f for _, f in meshes]
    nV, nF = meshes[0][0].shape[0], meshes[0][1].shape[0]
    c.verts = torch.cat(c.verts_list, 0)
    c.faces = torch.cat([f + i * nV for i, (_, f) in enumerate(meshes)], 0)
    first = torch.tensor([0 if spec.shared else n * nF for n in range(N)])  # image n's first packed face
    line_face = nF - 1 if spec.mesh == "sphere+line" else None
    draw_faces = nF - 1 if line_face is not None else nF  # the isolated face is placed, not drawn

    # lights, materials, cameras: every per-image row differs
    c.R, c.T, dist, elev, azim = _cameras(N)
    c.light = _lights(N, spec.light, dist, elev, azim, g)
    col = lambda lo, hi: (lo + (hi - lo) * torch.rand((N, 3), generator=g)).to(F32)
    c.light_ambient, c.light_diffuse, c.light_specular = col(0.3, 0.7), col(0.4, 1.0), col(0.4, 1.0)
    c.mat_ambient, c.mat_diffuse, c.mat_specular = col(0.5, 1.0), col(0.5, 1.0), col(0.5, 1.0)
    c.ambient = c.mat_ambient * c.light_ambient
    c.shininess = torch.tensor([SHININESS[(n + spec.seed) % 4] for n in range(N)], dtype=F32)

    # counts from {0..K}, both ends present; one pixel with a -1 inside its counted prefix
    counts = torch.randint(0, K + 1, (N, H, W), generator=g, dtype=torch.int32)
    flat = counts.reshape(-1)
    # the 16-byte store over an image boundary writes the next image's colour pattern: image 0 ends and
    # image 1 starts on padded slots (both padded, two images); image 1 ends on a live slot and image 2
    # starts on a padded one (the second slot alone is padded)
    fixed = {}
    if N > 1:
        fixed.update({H * W - 1: min(int(flat[H * W - 1]), K - 1), H * W: 0})
    if N > 2:
        fixed.update({2 * H * W - 1: K, 2 * H * W: 0})
    for i, v in fixed.items():
        flat[i] = v
    spots = [i for i in torch.randperm(flat.numel(), generator=g).tolist() if i not in fixed][:3]
    flat[spots[0]], flat[spots[1]], flat[spots[2]] = 0, K, max(K - 1, 1)
    hole_pixel, hole_k = spots[2], int(torch.randint(0, max(K - 1, 1), (1,), generator=g))
    c.counts = counts
    k = torch.arange(K)
    inside = k[None, None, None, :] < counts[..., None]
    c.inside = inside
    hole = torch.zeros((N * H * W, K), dtype=torch.bool)
    hole[hole_pixel, hole_k] = True
    c.hole = hole.reshape(N, H, W, K)
    c.live = inside & ~c.hole
    c.degenerate = torch.zeros_like(c.live)
    c.exact = torch.zeros_like(c.live)
    img = torch.arange(N)[:, None, None, None].expand(N, H, W, K)

    # textures
    if spec.tex == "uv":
        c.tex = torch.rand((N, HM, WM, 3), generator=g).to(F32)
        uvs = (-0.3 + 1.6 * torch.rand((len(meshes), nV, 2), generator=g)).to(F32)
        # 16 faces per mesh with distinct first corners take the exact UVs
        c.exact_faces = []
        for i, (_, f) in enumerate(meshes):
            seen, picked = set(), []
            for j in torch.randperm(draw_faces, generator=g).tolist():
                v0 = int(f[j, 0])
                if v0 not in seen and not (set(f[j].tolist()) & seen):
                    seen.update(f[j].tolist())
                    picked.append(j)
                if len(picked) == 16:
                    break
            assert len(picked) == 16
            for e, j in enumerate(picked):
                uvs[i, f[j, 0], 0], uvs[i, f[j, 0], 1] = EXACT_U[e % 4], EXACT_V[e // 4]
            c.exact_faces.append(torch.tensor(picked))
        c.verts_uvs_list = [u for u in uvs]
        c.verts_uvs = uvs.reshape(-1, 2)
        # up to 16 exact slots per image, on live slots
        for n in range(N):
            idx = torch.nonzero(c.live[n].reshape(-1))[:, 0]
            take = idx[torch.randperm(idx.numel(), generator=g)[: min(16, idx.numel() // 3)]]
            c.exact[n].reshape(-1)[take] = True
    elif spec.tex == "vertex":
        c.tex = torch.rand((c.verts.shape[0], 3), generator=g).to(F32)
    else:
        c.tex = torch.rand((N, H, W, K, 3), generator=g).to(F32)

    # slots: live ones hold a random face of their image's mesh, padded ones poison
    S = N * H * W * K
    p2f = first[img] + torch.randint(0, draw_faces, (N, H, W, K), generator=g)
    bary = _bary(g, S).reshape(N, H, W, K, 3)
    if line_face is not None:  # a few live slots per image on the isolated face
        for n in range(N):
            idx = torch.nonzero((c.live[n] & ~c.exact[n]).reshape(-1))[:, 0]
            take = idx[torch.randperm(idx.numel(), generator=g)[:4]]
            c.degenerate[n].reshape(-1)[take] = True
        p2f = torch.where(c.degenerate, first[img] + line_face, p2f)
    exact_order = torch.randperm(S, generator=g).reshape(N, H, W, K) % 16
    if spec.tex == "uv":
        ef = torch.stack([c.exact_faces[0 if spec.shared else n][exact_order[n]] for n in range(N)])
        p2f = torch.where(c.exact, first[img] + ef, p2f)
        bary = torch.where(c.exact[..., None], torch.tensor([1.0, 0.0, 0.0]), bary)
    c.p2f, c.bary = p2f, bary

    # redraw the slots that break a condition until none does
    for _ in range(200):
        bad = conditions(c)["bad"]
        if not bad.any():
            break
        nb = int(bad.sum())
        nf = torch.randint(0, draw_faces, (nb,), generator=g)
        if spec.tex == "uv":
            ex = c.exact[bad]
            alt = torch.stack([c.exact_faces[0 if spec.shared else int(n)][int(j)]
                               for n, j in zip(img[bad].tolist(), torch.randint(0, 16, (nb,), generator=g).tolist())])
            nf = torch.where(ex, alt, nf)
            nbary = torch.where(ex[:, None], torch.tensor([1.0, 0.0, 0.0]), _bary(g, nb))
        else:
            nbary = _bary(g, nb)
        c.p2f[bad] = first[img[bad]] + nf
        c.bary[bad] = nbary
    else:
        raise AssertionError(f"{spec_id(spec)}: conditions not reached")
    cond = conditions(c)
    for name, share in cond["shares"].items():
        assert share >= share_floor(name), f"{spec_id(spec)}: share {name} = {share:.3f}"
    if spec.tex == "uv":  # the exact slots reach the low clamp, a texel line and the high clamp on both axes
        for axis, vals in ((0, EXACT_U), (1, EXACT_V)):
            u = c.verts_uvs[c.faces[c.p2f[c.exact], 0], axis]
            assert (u == vals[0]).any() and (u == vals[3]).any() and ((u == vals[1]) | (u == vals[2])).any()

    # the two fragment variants: counts attached (poisoned padding) / no counts (-1 and zero bary)
    live = c.live
    c.p2f_plain = torch.where(live, c.p2f, torch.full_like(c.p2f, -1))
    c.bary_plain = torch.where(live[..., None], c.bary, torch.zeros((), dtype=F32))
    other = (first[(img + 1) % N] if N > 1 and not spec.shared else first[img]) + torch.randint(0, nF, (N, H, W, K), generator=g)
    poison = torch.where(torch.rand((N, H, W, K), generator=g) < 0.5, other, torch.full_like(other, -1))
    c.p2f_counts = torch.where(inside, c.p2f_plain, poison)  # (the hole keeps its -1)
    c.bary_counts = torch.where(live[..., None], c.bary, torch.full((), float("nan"), dtype=F32))
    c.p2f = c.p2f_plain  # what the reference indexes

    # cotangent: exactly zero on about half of the live slots; on padded slots zero (uv / vertex: the
    # kernel gives them no gradient) or random (given: d texel = ambient * g)
    G = torch.randn((N, H, W, K, 3), generator=g).to(F32)
    keep = (torch.rand((N, H, W, K), generator=g) < 0.5) | c.exact | c.degenerate
    keep = torch.where(live, keep, torch.full_like(keep, spec.tex == "given"))
    c.G = G * keep[..., None]
    c.zero_bwd = live & ~keep

    c.mixed = mixed_float4s(c.counts, K)
    assert int(counts.min()) == 0 and int(counts.max()) == K
    if K % 4:
        assert c.mixed["pixel"] > 0, spec_id(spec)
    if K > 1:
        assert c.mixed["within"] > 0, spec_id(spec)
    if N > 1 and (H * W * K * 3) % 4:  # 16-byte stores over the first two image boundaries
        assert c.mixed["split"] > 0 and (N == 2 or (2 * H * W * K * 3) % 4 == 0 or c.mixed["image"] > 0), spec_id(spec)
    return c


# ------------------------------------------------------------------------------ the reference
Ref = collections.namedtuple("Ref", "colours d_bary d_verts d_tex d_light d_T")


def _grads64(c, G, live=None):
    l = leaves(c)
    z = composition(c, l["verts"], l["bary"], l["tex"], l["light"], l["T"], live)
    gs = torch.autograd.grad(z.colours, [l["bary"], l["verts"], l["tex"], l["light"], l["T"]],
                             grad_outputs=G.to(F64), allow_unused=True)
    gs = [torch.zeros_like(x) if gr is None else gr for gr, x in zip(gs, (l["bary"], l["verts"], l["tex"], l["light"], l["T"]))]
    return Ref(z.colours.detach(), *gs)


@functools.lru_cache(maxsize=None)
def shade_ref64(spec):
    """PyTorch3D's phong_shading (+ the texel lookup) in float64 on the case's float32 inputs: the
    colours (N,H,W,K,3) and, for the cotangent c.G, d bary, d verts (packed), d texture (maps, vertex
    colours or texels), d light and d T (the camera centre's gradient taken through cameras.T).
    Liveness is k < count and face >= 0, which is face >= 0 of the no-counts variant.  Computed once
    per case; treat the result as read-only."""
    c = build(spec)
    return _grads64(c, c.G)


@functools.lru_cache(maxsize=None)
def degenerate_ref64(spec):
    """The reference for a cotangent on the isolated face's slots alone: every gradient but d texture
    (and d bary through the texture) is identically zero."""
    c = build(spec)
    return _grads64(c, c.G * c.degenerate[..., None])


# ---------------------------------------------------------------- library objects of a case
def scene(c, device="cpu", dtype=F32, variant="counts"):
    """The case as the library's objects on `device`: (meshes, fragments, lights, cameras, materials,
    leaves, texels).  leaves: dict(bary, verts (packed), tex, light, T) of tensors that require
    grad; texels: the `given` tensor (else None).  variant: "counts" (poisoned padding, counts
    attached), "plain" (-1 / zero padding, nothing attached).  dtype float64 (CPU only) serves the
    torch composition: cameras are then a stand-in that returns float64 centres."""
    from pertrenderer_amd.renderer import (FoVPerspectiveCameras, Materials, Meshes, PointLights, TexturesUV,
                                           TexturesVertex)
    from pertrenderer_amd.renderer.rasterizer import Fragments
    from pertrenderer_amd.renderer.renderer import DirectionalLights
    spec = c.spec
    to = lambda t: t.to(device=device, dtype=dtype)
    leaf = lambda t: to(t).clone().requires_grad_(True)
    p2f = (c.p2f_counts if variant == "counts" else c.p2f_plain).to(device).clone()
    bary = leaf(c.bary_counts if variant == "counts" else c.bary_plain)
    if variant == "counts":
        p2f._pr_valid_counts = (p2f._version, c.counts.to(device).clone())
    shape = tuple(p2f.shape)
    frag = Fragments(p2f, torch.zeros(shape, dtype=dtype, device=device), bary, torch.zeros(shape, dtype=dtype, device=device))
    verts = leaf(c.verts)
    sizes = [v.shape[0] for v in c.verts_list]
    faces = [f.to(device) for f in c.faces_list]
    texels = None
    if spec.tex == "uv":
        tex = leaf(c.tex)
        textures = TexturesUV(tex, faces, [to(u) for u in c.verts_uvs_list])
    elif spec.tex == "vertex":
        tex = leaf(c.tex)
        textures = TexturesVertex(list(tex.split(sizes)))
    else:
        tex = texels = leaf(c.tex)
        textures = None
    meshes = Meshes(list(verts.split(sizes)), faces, textures)
    light = leaf(c.light)
    lights = (DirectionalLights if spec.light == "directional" else PointLights)(device=device)
    lights.location = light
    lights.ambient_color, lights.diffuse_color, lights.specular_color = to(c.light_ambient), to(c.light_diffuse), to(c.light_specular)
    mats = Materials(device=device)
    mats.ambient_color, mats.diffuse_color, mats.specular_color = to(c.mat_ambient), to(c.mat_diffuse), to(c.mat_specular)
    mats.shininess = to(c.shininess)  # (N,): Materials() takes a scalar only
    T = leaf(c.T)
    if dtype == F32:
        cams = FoVPerspectiveCameras(R=c.R.to(device), T=T, device=device)
    else:
        R = to(c.R)
        cams = types.SimpleNamespace(get_camera_center=lambda: camera_centers(R, T))
    return meshes, frag, lights, cams, mats, dict(bary=bary, verts=verts, tex=tex, light=light, T=T), texels


def grads_of(out, leaves, G, retain=False):
    """Ref-shaped gradients of the library's colours `out` for cotangent G (nothing here reads out's
    values: it may be unwritten where G is zero)."""
    order = ("bary", "verts", "tex", "light", "T")
    gs = torch.autograd.grad(out, [leaves[k] for k in order], grad_outputs=G.to(out.dtype), allow_unused=True,
                             retain_graph=retain)
    return Ref(out.detach(), *[torch.zeros_like(leaves[k]) if gr is None else gr for gr, k in zip(gs, order)])


def ratio(actual, ref, bar, where=None):
    """max|actual - ref| / (bar * max|ref|): at most 1 passes.  `where` (a mask broadcast over the
    last axis) restricts the comparison, and the scale, to its slots.  A reference that is identically zero
    asks for exact zeros (ratio 0 or inf)."""
    a, r = actual.detach().to("cpu", F64), ref.detach().to("cpu", F64)
    if where is not None:
        a, r = a[where], r[where]
    scale = float(r.abs().max()) if r.numel() else 0.0
    if scale == 0.0:
        return 0.0 if not a.numel() or bool((a == 0).all()) else float("inf")
    err = float((a - r).abs().max())
    return err / (bar * scale) if np.isfinite(err) else float("inf")

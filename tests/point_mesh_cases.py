"""Shared by the point-to-mesh tests (not a test module): seeded scenes (meshes of
mesh_loss_cases.py with point clouds around them), a scene with planted exact ties, and the
restatement of the documented arithmetic of point_mesh_face_distance / point_mesh_edge_distance.

Arithmetic.  The Voronoi region of the point comes from the signs of the edge dot products
(Ericson's closest-point-on-triangle tests, in his order) and gives the weights w of the closest
point.  In a vertex or edge region r = sum w_i (p - v_i); in the interior n = e0 x e1,
t = n . (p - v0) / |n|^2 and r = t n; d^2 = |r|^2.  A triangle with |n|^2 <= 1e-30 is its three
segments, a zero-length segment its first endpoint.  The restatement forms a dense (P_n, M_n)
matrix of d^2 per batch element, takes the first minimum of every row and column (the lowest
index), evaluates the chosen pairs again and lets autograd supply the gradients: the weights of a
vertex or edge region are held constant (the envelope form), the interior's t n is differentiated
as written.  Run in float64 on float32 inputs it is the reference; run in float32 it measures
float32's own error (the 4x rule of test_gpu_mesh_losses.py); both can be evaluated at given
indices, since float32 may pick the other of two faces that share the closest point.

Scenes.  Points are drawn in the mesh's bounding box grown by 20 % per side and kept when their
float64 distance to the mesh is at least 2 % of the box diagonal.  scene() asserts that every
primitive's best and second-best point differ by >= MIN_GAP in float64 d^2 (faces and edges), so
the primitive -> point indices of float32 must equal float64's.

Known answers.  TRI / REGIONS / DEGENERATE_TRIANGLES / SEGMENT_CASES / ZERO_LENGTH are the hand-built
table of the closest-point arithmetic: every value is exact in float32 (dyadic numbers of a few
bits, every divisor a power of two), so equality is asked for, on the CPU and on the device.

Collapsed scenes.  collapsed_scene() copies a face's first vertex position onto its other two
vertices: that face becomes a point (three ids, one position), its neighbours become (a, a, b) /
(a, b, b) faces, three of its edges get length 0.  On an (a, b, b) face the segments (a b) and (c a)
coincide and rounding decides which of them is "nearest first", so the vertex gradient goes to id b
or to id c: d verts is only well-posed after the rows of bitwise-equal vertex positions have been
summed (merged_rows, grad_error).  Collinear faces with three distinct positions are left out of
these scenes: the same closest point is expressed over (a, b), (b, c) or (c, a), so there is no
unique d verts at all (the float32 restatement's own error reaches 2e-2); the table above covers
their values."""
import functools

import torch

from mesh_loss_cases import brute_edges, case

MESHES = ["triangle", "tetrahedron", "fan3", "hub70", "batch2", "sphere_642"]
COUNTS = [1, 3, 70, 257]
# a separate, smaller matrix: clouds that cross the kernel's 512-point tile (one point into the next
# tile, two tiles and one point); under batch2 the second cloud stays at one point
TILE_MESHES = ["sphere_642", "hub70", "batch2"]
TILE_COUNTS = [513, 1025]
MIN_GAP = 1e-6
SEEDS = {}  # (mesh, count) -> seed where 0 does not give the gap; found by trying 0, 1, 2, ... on the CPU
DEGENERATE = 1e-30
KINDS = ["faces", "edges"]

# ---- the known-answer table
TRI = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
# (point, d^2, weights): every value is exact in float32
REGIONS = {
    "vertex a": ([-1.0, -1.0, 1.0], 3.0, [1.0, 0.0, 0.0]),
    "vertex b": ([2.0, -0.5, 0.0], 1.25, [0.0, 1.0, 0.0]),
    "vertex c": ([-0.5, 2.0, 0.0], 1.25, [0.0, 0.0, 1.0]),
    "edge ab": ([0.5, -1.0, 0.5], 1.25, [0.5, 0.5, 0.0]),
    "edge ac": ([-1.0, 0.25, 0.0], 1.0, [0.75, 0.0, 0.25]),
    "edge bc, in the plane": ([1.0, 1.0, 0.0], 0.5, [0.0, 0.5, 0.5]),
    "interior": ([0.25, 0.25, 2.0], 4.0, [0.5, 0.25, 0.25]),
    "on the triangle": ([0.25, 0.5, 0.0], 0.0, [0.25, 0.25, 0.5]),
    "on a vertex": ([1.0, 0.0, 0.0], 0.0, [0.0, 1.0, 0.0]),
}
# (triangle, point, d^2, weights)
DEGENERATE_TRIANGLES = {
    # collinear: the segments (a b), (b c), (c a) give 1.25, 1, 1: the first of the equal ones
    "collinear": ([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0]], [1.5, 1.0, 0.0], 1.0, [0.0, 0.5, 0.5]),
    "all equal": ([[1.0, 2.0, 3.0]] * 3, [1.0, 2.0, 5.0], 4.0, [1.0, 0.0, 0.0]),
}
# a zero-length segment is its first endpoint: (segment, point, d^2, weights)
ZERO_LENGTH = ([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0]], [1.0, 0.0, 3.0], 4.0, [1.0, 0.0, 0.0])
# a segment's interior and its two ends: (point, d^2, weights)
SEGMENT = [[0.0, 0.0, 0.0], [2.0, 0.0, 0.0]]
SEGMENT_CASES = [([0.5, 1.0, 0.0], 1.0, [0.75, 0.25, 0.0]), ([-1.0, 0.0, 0.0], 1.0, [1.0, 0.0, 0.0]),
                 ([3.0, 0.0, 1.0], 2.0, [0.0, 1.0, 0.0])]
# the point above TRI's interior against TRI's edges: nearest to (a b), at (0.25, 0, 0)
ABOVE_INTERIOR_TO_EDGES = ([0.25, 0.25, 2.0], 4.0625, [0.75, 0.25, 0.0])


def known_edge_cases():
    """[(label, three vertex positions, point, d^2, weights)] for point_mesh_edge_distance on a mesh of
    one face (0, 1, 2): its unique edges are (0 1), (0 2), (1 2), the segment under test is (0 1) and
    the third vertex lies where no other edge is strictly nearer to the point, so edge 0 is chosen
    (where another edge ends in the same closest vertex it ties exactly and the lowest index wins).
    The zero-length edge is two ids at one position."""
    far = [0.0, -8.0, 0.0]
    out = [("zero-length edge", ZERO_LENGTH[0] + [[1.0, 10.0, 3.0]], *ZERO_LENGTH[1:])]
    out += [(f"segment case {i}", SEGMENT + [far], p, d2, w) for i, (p, d2, w) in enumerate(SEGMENT_CASES)]
    return out + [("above the interior", TRI, *ABOVE_INTERIOR_TO_EDGES)]


def _dot(a, b):
    return (a * b).sum(-1)


def _safe(num, den):
    return torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(num))


def segment_weights(p, a, b):
    """(..., 3) weights (1 - v, v, 0) of the closest point of segment (a, b)."""
    ab = b - a
    d1, d3 = _dot(ab, p - a), _dot(ab, p - b)
    v = torch.where(d1 <= 0, torch.zeros_like(d1), torch.where(d3 >= 0, torch.ones_like(d1), _safe(d1, d1 - d3)))
    return torch.stack([1 - v, v, torch.zeros_like(v)], -1)


def triangle_weights(p, a, b, c):
    """(weights (...,3), interior (...) bool) of the closest point of triangle (a, b, c)."""
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    ab, ac = ab.expand_as(ap), ac.expand_as(ap)
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    n = torch.cross(ab, ac, dim=-1)
    n2 = _dot(n, n)
    flat = ~(n2 > DEGENERATE)
    inv = torch.where(flat, torch.zeros_like(n2), 1 / torch.where(flat, torch.ones_like(n2), n2))
    q = ap - n * (_dot(n, ap) * inv)[..., None]
    w1, w2 = _dot(n, torch.cross(q, ac, dim=-1)) * inv, _dot(n, torch.cross(ab, q, dim=-1)) * inv
    one, zero = torch.ones_like(d1), torch.zeros_like(d1)
    w = torch.stack([1 - w1 - w2, w1, w2], -1)
    interior = torch.ones_like(d1, dtype=torch.bool)
    vab, vac, vbc = _safe(d1, d1 - d3), _safe(d2, d2 - d6), _safe(d4 - d3, (d4 - d3) + (d5 - d6))
    tests = [((d1 <= 0) & (d2 <= 0), (one, zero, zero)),
             ((d3 >= 0) & (d4 <= d3), (zero, one, zero)),
             ((d1 * d4 - d3 * d2 <= 0) & (d1 >= 0) & (d3 <= 0), (1 - vab, vab, zero)),
             ((d6 >= 0) & (d5 <= d6), (zero, zero, one)),
             ((d5 * d2 - d1 * d6 <= 0) & (d2 >= 0) & (d6 <= 0), (1 - vac, zero, vac)),
             ((d3 * d6 - d5 * d4 <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), (zero, 1 - vbc, vbc))]
    for cond, wr in reversed(tests):  # the earliest test that holds wins
        w = torch.where(cond[..., None], torch.stack(wr, -1), w)
        interior = interior & ~cond
    if flat.any():
        def seg(x, y, perm):
            ws = segment_weights(p, x, y)
            r = ws[..., 0:1] * (p - x) + ws[..., 1:2] * (p - y)
            return _dot(r, r), ws[..., perm]
        ds, ws = seg(a, b, [0, 1, 2])
        for x, y, perm in ((b, c, [2, 0, 1]), (c, a, [1, 2, 0])):
            d_, w_ = seg(x, y, perm)
            ws, ds = torch.where((d_ < ds)[..., None], w_, ws), torch.minimum(d_, ds)
        w = torch.where(flat[..., None], ws, w)
    return w, interior & ~flat


def closest(p, pv):
    """(d^2, w) of points p (...,3) against primitives pv (...,K,3), broadcast; differentiable in p and pv."""
    a, b = pv[..., 0, :], pv[..., 1, :]
    if pv.shape[-2] == 2:
        with torch.no_grad():
            w = segment_weights(p, a, b)
        r = w[..., 0:1] * (p - a) + w[..., 1:2] * (p - b)
        return _dot(r, r), w
    c = pv[..., 2, :]
    with torch.no_grad():
        w, interior = triangle_weights(p, a, b, c)
    r = w[..., 0:1] * (p - a) + w[..., 1:2] * (p - b) + w[..., 2:3] * (p - c)
    n = torch.cross((b - a).expand_as(r), (c - a).expand_as(r), dim=-1)
    n2 = _dot(n, n)
    t = _dot(n, p - a) / torch.where(interior, n2, torch.ones_like(n2))
    r = torch.where(interior[..., None], n * t[..., None], r)
    return _dot(r, r), w


def prims_of(verts, faces, kind):
    """Per mesh (M_i, K) int64 local vertex ids: the faces, or the sorted unique edges."""
    if kind == "faces":
        return list(faces)
    return [torch.tensor(brute_edges(f), dtype=torch.int64).reshape(-1, 2) for f in faces]


def reference(verts, faces, clouds, kind, dtype=torch.float64, idx=None, cot=None):
    """The restatement in `dtype` on lists of verts, faces and clouds.  dict(dist_p (P), dist_m (M),
    idx_p, idx_m (packed, -1: nothing to choose), loss, grad_points, grad_verts (of the loss, packed) and,
    with cot = (cot_p (P), cot_m (M)), raw_grad_points, raw_grad_verts of
    (dist_p cot_p).sum() + (dist_m cot_m).sum()).  idx = (idx_p, idx_m) evaluates at given indices."""
    prims = prims_of(verts, faces, kind)
    v = [x.to(dtype).clone().requires_grad_(True) for x in verts]
    c = [x.to(dtype).clone().requires_grad_(True) for x in clouds]
    dp, dm, ip, im = [], [], [], []
    poff = moff = 0
    loss = torch.zeros((), dtype=dtype)
    for n in range(len(v)):
        P, M = c[n].shape[0], prims[n].shape[0]
        pv = v[n][prims[n]]
        if P == 0 or M == 0:
            jp, jm = torch.full((P,), -1, dtype=torch.int64), torch.full((M,), -1, dtype=torch.int64)
            d_p, d_m = torch.zeros(P, dtype=dtype), torch.zeros(M, dtype=dtype)
        else:
            if idx is None:
                with torch.no_grad():
                    d = closest(c[n][:, None], pv[None])[0]
                    jp, jm = d.argmin(dim=1), d.argmin(dim=0)  # the first minimum
            else:
                jp = idx[0][poff:poff + P].long() - moff
                jm = idx[1][moff:moff + M].long() - poff
                assert ((jp >= 0) & (jp < M)).all() and ((jm >= 0) & (jm < P)).all(), "index outside its batch element"
            d_p, d_m = closest(c[n], pv[jp])[0], closest(c[n][jm], pv)[0]
            loss = loss + d_p.mean() + d_m.mean()
            jp, jm = jp + moff, jm + poff
        dp.append(d_p), dm.append(d_m), ip.append(jp), im.append(jm)
        poff, moff = poff + P, moff + M
    loss = loss / len(v)
    dp, dm = torch.cat(dp), torch.cat(dm)
    out = dict(dist_p=dp.detach(), dist_m=dm.detach(), idx_p=torch.cat(ip), idx_m=torch.cat(im), loss=loss.detach())
    g = torch.autograd.grad(loss, c + v, retain_graph=cot is not None, allow_unused=True)
    fill = lambda gs, xs: torch.cat([torch.zeros_like(x) if y is None else y for y, x in zip(gs, xs)])  # noqa: E731
    out["grad_points"], out["grad_verts"] = fill(g[:len(c)], c), fill(g[len(c):], v)
    if cot is not None:
        raw = (dp * cot[0].to(dtype)).sum() + (dm * cot[1].to(dtype)).sum()
        g = torch.autograd.grad(raw, c + v, allow_unused=True)
        out["raw_grad_points"], out["raw_grad_verts"] = fill(g[:len(c)], c), fill(g[len(c):], v)
    return out


def dense_d2(verts, faces, clouds, kind, dtype=torch.float64):
    """Per batch element the (P_n, M_n) matrix of d^2 in `dtype`, without autograd."""
    prims = prims_of(verts, faces, kind)
    with torch.no_grad():
        return [closest(c.to(dtype)[:, None], v.to(dtype)[p][None])[0] for v, c, p in zip(verts, clouds, prims)]


def _draw(v, f, count, g):
    """`count` float32 points around the mesh (v, f), each at least 2 % of the box diagonal from it."""
    lo, hi = v.min(0).values, v.max(0).values
    diag = (hi - lo).norm().double()
    pts = torch.zeros((0, 3))
    while pts.shape[0] < count:  # a CPU rejection loop
        c = lo + (hi - lo) * (torch.rand((4 * count + 8, 3), generator=g) * 1.4 - 0.2)
        d = dense_d2([v], [f], [c], "faces")[0].min(dim=1).values.sqrt()
        pts = torch.cat([pts, c[d >= 0.02 * diag]])
    return pts[:count].contiguous()


def lengths_of(name, count):
    """Points per cloud: `count`, and under batch2 a second cloud of length 1."""
    return [count, 1] if name == "batch2" else [count]


def make_scene(name, count, seed):
    verts, faces = case(name)
    verts = [v.detach() for v in verts]  # case() is shared: another test may have marked its tensors
    g = torch.Generator().manual_seed(seed)
    clouds = [_draw(v, f, n, g) for v, f, n in zip(verts, faces, lengths_of(name, count))]
    return list(verts), list(faces), clouds


# ---- collapsed meshes: the faces whose first vertex position is copied onto their other two vertices
COLLAPSED = {"hub70": (3,), "sphere_642": (5, 700)}
COLLAPSED_COUNTS = [70, 1025]
PLANT_RADII = (0.04, 0.05, 0.06)  # of the box diagonal; unequal: equal ones tie exactly on the point-like faces


def degenerate_faces(v, f):
    """Indices of the faces with |n|^2 <= DEGENERATE in float64."""
    pv = v.double()[f]
    n = torch.cross(pv[:, 1] - pv[:, 0], pv[:, 2] - pv[:, 0], dim=-1)
    return (~(_dot(n, n) > DEGENERATE)).nonzero()[:, 0]


def make_collapsed_scene(name, count, seed):
    verts, faces = case(name)
    v, f = verts[0].detach().clone(), faces[0]
    centre = v.mean(0)
    diag = (v.max(0).values - v.min(0).values).norm()
    planted = []
    for i in COLLAPSED[name]:
        a, b, c = f[i].tolist()
        v[b] = v[c] = v[a]
        out = (v[a] - centre) / (v[a] - centre).norm()  # outwards: the meshes are centred at their mean
        planted += [v[a] + r * diag * out for r in PLANT_RADII]
    g = torch.Generator().manual_seed(seed)
    pts = torch.cat([_draw(v, f, count - len(planted), g), torch.stack(planted)])
    return [v], [f], [pts.contiguous()]


def merged_rows(grad, verts):
    """A packed (V,3) vertex gradient with the rows of bitwise-equal vertex positions (of one mesh)
    summed, in float64 on the CPU: what d verts is compared as on a collapsed mesh."""
    mesh = torch.cat([torch.full((v.shape[0], 1), float(i), dtype=torch.float64) for i, v in enumerate(verts)])
    key = torch.cat([torch.cat(list(verts)).double().cpu(), mesh], 1)
    uniq, inverse = torch.unique(key, dim=0, return_inverse=True)
    return torch.zeros((uniq.shape[0], 3), dtype=torch.float64).index_add_(0, inverse, grad.detach().double().cpu())


def grad_error(got, want, key, merge=None):
    """max-abs over max-abs; with merge = the verts list a vertex gradient is compared through merged_rows."""
    from mesh_loss_cases import rel_err
    if merge is not None and key.endswith("verts"):
        got, want = merged_rows(got, merge), merged_rows(want, merge)
    return rel_err(got, want)


def min_gap(verts, faces, clouds, skip=()):
    """The smallest best-to-second-best gap in float64 d^2 over every primitive (faces and edges) of
    every batch element with at least two points; the packed-to-local point columns in `skip` are left out."""
    worst = float("inf")
    for kind in KINDS:
        for d in dense_d2(verts, faces, clouds, kind):
            keep = [j for j in range(d.shape[0]) if j not in skip]
            if len(keep) < 2 or d.shape[1] == 0:
                continue
            two = d[keep].t().topk(2, dim=1, largest=False).values
            worst = min(worst, (two[:, 1] - two[:, 0]).min().item())
    return worst


def scene(name, count, collapsed=False):
    """(verts list, faces list, clouds list), float32 on the CPU; the gap rule is asserted."""
    return collapsed_scene(name, count) if collapsed else _clean_scene(name, count)


@functools.lru_cache(maxsize=None)
def _clean_scene(name, count):
    s = make_scene(name, count, SEEDS.get((name, count), 0))
    assert min_gap(*s) >= MIN_GAP, (name, count, min_gap(*s))
    return s


@functools.lru_cache(maxsize=None)
def collapsed_scene(name, count):
    """scene() on the collapsed mesh of `name`, with three points planted outwards of every collapsed
    vertex.  Asserted: the degenerate primitives are there, the gap rule, and on hub70 that a
    degenerate face is some point's float64 choice (degenerate_choices)."""
    s = make_collapsed_scene(name, count, SEEDS.get((name, count, "collapsed"), 0))
    v, f = s[0][0], s[1][0]
    flat = degenerate_faces(v, f)
    assert set(COLLAPSED[name]) <= set(flat.tolist()) and len(flat) >= 3 * len(COLLAPSED[name])
    for i in COLLAPSED[name]:
        assert torch.equal(v[f[i]], v[f[i, :1]].expand(3, 3)), "three ids, one position"
    e = torch.tensor(brute_edges(f))
    assert (v[e[:, 0]] == v[e[:, 1]]).all(dim=1).sum() == 3 * len(COLLAPSED[name]), "zero-length edges"
    assert min_gap(*s) >= MIN_GAP, (name, count, min_gap(*s))
    assert name != "hub70" or degenerate_choices(*s) > 0, (name, count)
    return s


def degenerate_choices(verts, faces, clouds):
    """How many points have a degenerate face as their float64 choice (the first minimum)."""
    chosen = dense_d2(verts, faces, clouds, "faces")[0].argmin(dim=1)
    return torch.isin(chosen, degenerate_faces(verts[0], faces[0])).sum().item()


# ---- planted exact ties: face TIE_FACE of sphere_642 copied into the middle and to the end of the
# face list (with the faces cut into three ranges, or into eleven, the copies lie in the first, a
# middle and the last range); point TIE_POINT sits above that face's centroid, so the copies are its
# nearest faces at exactly equal d^2; the first point (after point 0, not TIE_POINT) that is the
# nearest point of some face and of some edge is duplicated as the last point: point 1 with TIE_COUNT
# points.  With TIE_COUNT_FAR points the two copies are two 512-point tiles apart: in the first and
# the third tile of one range, or in the first and the last of two or three ranges.
TIE_FACE, TIE_POINT, TIE_COUNT, TIE_COUNT_FAR = 5, 2, 70, 1025


@functools.lru_cache(maxsize=None)
def tie_scene(count=TIE_COUNT):
    """(verts list, faces list, clouds list, copies (face indices, ascending), duplicates (point indices))."""
    verts, faces = case("sphere_642")
    v, f = verts[0].detach(), faces[0]
    mid = f.shape[0] // 2
    f = torch.cat([f[:mid], f[TIE_FACE:TIE_FACE + 1], f[mid:], f[TIE_FACE:TIE_FACE + 1]])
    copies = (TIE_FACE, mid, f.shape[0] - 1)
    pts = _draw(v, f, count, torch.Generator().manual_seed(SEEDS.get(("tie", count), 0))).clone()
    a, b, c = (v[i] for i in f[TIE_FACE])
    n = torch.cross(b - a, c - a, dim=0)
    n = n / n.norm()
    centre = (a + b + c) / 3
    n = n if (n * centre).sum() > 0 else -n  # outwards: the sphere is centred at the origin
    pts[TIE_POINT] = centre + 0.05 * (v.max(0).values - v.min(0).values).norm() * n
    nearest = [d[:-1].argmin(dim=0) for d in (dense_d2([v], [f], [pts], k)[0] for k in KINDS)]
    first = min(j for j in range(1, count - 1) if j != TIE_POINT and all((n == j).any() for n in nearest))
    pts[-1] = pts[first]
    dup = (first, count - 1)
    assert min_gap([v], [f], [pts], skip=(dup[1],)) >= MIN_GAP, (count, min_gap([v], [f], [pts], skip=(dup[1],)))
    return [v], [f], [pts], copies, dup


def random_cotangent(P, M, seed=7):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(P, generator=g), torch.randn(M, generator=g)


def references(name, count, kind, collapsed=False):
    """(float64 restatement with the loss's and the raw outputs' gradients, the cotangent), once per case."""
    return _references(name, count, kind, bool(collapsed))


@functools.lru_cache(maxsize=None)
def _references(name, count, kind, collapsed):
    verts, faces, clouds = scene(name, count, collapsed)
    M = sum(p.shape[0] for p in prims_of(verts, faces, kind))
    cot = random_cotangent(sum(c.shape[0] for c in clouds), M)
    return reference(verts, faces, clouds, kind, cot=cot), cot


GRAD_KEYS = ("grad_points", "grad_verts", "raw_grad_points", "raw_grad_verts")
MAX_RESTATEMENT_ERROR = 2e-5  # of the float32 restatement's gradients; keeps the 4x rule from loosening


def float32_errors(name, count, kind, idx, collapsed=False):
    """{key: max-abs over max-abs error} of the float32 restatement against float64, both evaluated at
    the packed indices idx = (idx_p, idx_m); asserted to stay below MAX_RESTATEMENT_ERROR.  On a
    collapsed scene the vertex gradients are compared through merged_rows."""
    verts, faces, clouds = scene(name, count, collapsed)
    _, cot = references(name, count, kind, collapsed)
    r64 = reference(verts, faces, clouds, kind, idx=idx, cot=cot)
    r32 = reference(verts, faces, clouds, kind, dtype=torch.float32, idx=idx, cot=cot)
    err = {k: grad_error(r32[k], r64[k], k, verts if collapsed else None) for k in GRAD_KEYS}
    assert max(err.values()) <= MAX_RESTATEMENT_ERROR, (name, count, kind, err)
    return r64, err

"""Float64 references and shared inputs of the pose-step kernels' tests (pr_so3_exp_*, pr_rotate_*,
pr_rgb_mse_*, pr_pose_step, pr_vert_normals_*): test_pose_cases_cpu.py pins the references on the
CPU, test_gpu_pose.py / test_gpu_pose_opt.py / test_gpu_normals.py compare the kernels with them.

Every reference takes the float32 inputs the kernel sees, widens them to float64 and evaluates the
plain formula there, so the only difference left is the kernel's own float32 arithmetic.  Importing
this module needs no GPU."""
import contextlib
import functools
import math
import os

import numpy as np
import torch

from oracle import philox_ref

HERE = os.path.dirname(os.path.abspath(__file__))
F64 = torch.float64

LAYERS = ("python", "c++")


@contextlib.contextmanager
def autograd_layer(name):
    """Run the block on the Python autograd Functions ("python") or on the C++ layer ("c++").
    Yields False without running anything native when the C++ layer is asked for and not loadable
    (the caller skips with host_layer.error() as the reason)."""
    from pertrenderer_amd import host_layer
    if name == "python":
        with host_layer.disabled():
            assert host_layer.get() is None
            yield True
    elif host_layer.layer() != "c++":
        yield False
    else:
        assert host_layer.get() is not None, "the C++ layer is loaded but not selected"
        yield True


# ------------------------------------------------------------------------------------ so3
SO3_EPS = 1e-4
# the fixed angles: zero, far below / either side of the clamp at sqrt(eps) = 0.01, just above it,
# generic, around pi and 2 pi (fac1 -> 0), and beyond one turn
SO3_ANGLES = (0.0, 1e-6, 1e-3, 0.0099, 0.0101, 0.02, 0.5, math.pi - 1e-3, math.pi, math.pi + 1e-3,
              2 * math.pi - 1e-3, 2 * math.pi, 7.5, 20.0)
SO3_ROWS = 130  # three 64-thread blocks and a tail of 2
SO3_SMALL = 0.02  # rows below it are ill-conditioned in float32 (1 - cos(angle) cancels)


def hat64(w):
    h = w.new_zeros(w.shape[0], 3, 3)
    x, y, z = w.unbind(1)
    h[:, 0, 1], h[:, 0, 2] = -z, y
    h[:, 1, 0], h[:, 1, 2] = z, -x
    h[:, 2, 0], h[:, 2, 1] = -y, x
    return h


def so3_ref(w, eps, G):
    """PyTorch3D's so3_exponential_map (clamp(|w|^2, eps).sqrt(), Rodrigues with fac1 = sin / angle,
    fac2 = (1 - cos) / angle^2) in float64 on the float32-rounded w (N,3), eps and cotangent G (N,3,3):
    (R (N,3,3), d w (N,3)) as float64 numpy arrays."""
    w64 = torch.as_tensor(np.asarray(w, np.float32)).to(F64).reshape(-1, 3).requires_grad_(True)
    G64 = torch.as_tensor(np.asarray(G, np.float32)).to(F64).reshape(-1, 3, 3)
    nrms = (w64 * w64).sum(1)
    angles = torch.clamp(nrms, float(np.float32(eps))).sqrt()
    inv = 1.0 / angles
    fac1 = inv * angles.sin()
    fac2 = inv * inv * (1.0 - angles.cos())
    S = hat64(w64)
    R = fac1[:, None, None] * S + fac2[:, None, None] * torch.bmm(S, S) + torch.eye(3, dtype=F64)[None]
    if w64.shape[0]:
        (gw,) = torch.autograd.grad((R * G64).sum(), w64)
    else:
        gw = torch.zeros_like(w64)
    return R.detach().numpy(), gw.numpy()


def so3_rows(angles, seed, eps, clearance=1e-6):
    """(w (N,3) float32, G (N,3,3) float32, the rows' float32 angles) for log-rotations of the given
    angles along random unit directions.  Asserts that no row's float32 |w|^2 is within `clearance`
    of eps, so the kernel's float32 compare and the reference's float64 compare take the same side."""
    rng = np.random.RandomState(seed)
    a = np.asarray(angles, np.float64)
    d = rng.randn(a.size, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    w = (a[:, None] * d).astype(np.float32)
    G = rng.randn(a.size, 3, 3).astype(np.float32)
    nrms = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]  # the kernel's float32 sum
    assert nrms.dtype == np.float32
    assert (np.abs(nrms.astype(np.float64) - float(np.float32(eps))) > clearance).all(), "a row sits on the clamp boundary"
    return w, G, np.sqrt(nrms.astype(np.float64))


@functools.lru_cache(maxsize=None)
def so3_inputs():
    """The 130-row case: SO3_ANGLES, then random angles in [0, 6.5)."""
    rng = np.random.RandomState(11)
    angles = list(SO3_ANGLES) + list(rng.uniform(0.0, 6.5, SO3_ROWS - len(SO3_ANGLES)))
    w, G, ang = so3_rows(angles, 12, SO3_EPS)
    assert w.shape == (SO3_ROWS, 3)
    return w, G, ang


@functools.lru_cache(maxsize=None)
def so3_inputs_eps():
    """eps = 1e-2 (clamp at |w| = 0.1): rows either side of it, far below and generic ones."""
    return so3_rows((0.0, 0.03, 0.099, 0.101, 0.11, 0.5, 2.0, 3.0), 13, 1e-2, clearance=1e-4) + (1e-2,)


@functools.lru_cache(maxsize=None)
def so3_boundary_inputs():
    """Rows with |w|^2 == eps exactly, in float32 and in float64 alike (eps = 2^-4, w = +-2^-2 along an
    axis), between rows either side: torch.clamp passes the gradient where |w|^2 >= eps, so on these
    rows the backward's compare must be >= while the forward's choice of branch does not matter.
    (w, G, angles, eps)."""
    eps = 0.0625
    w = np.array([[0.25, 0, 0], [0, -0.25, 0], [0, 0, 0.25], [-0.25, 0, 0], [0.2, 0.1, 0.05], [0.2, 0.15, 0.05]], np.float32)
    G = np.random.RandomState(14).randn(w.shape[0], 3, 3).astype(np.float32)
    nr32 = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]
    nr64 = (w.astype(np.float64) ** 2).sum(1)
    assert (nr32[:4] == np.float32(eps)).all() and (nr64[:4] == eps).all() and nr64[4] < eps - 1e-3 and nr64[5] > eps + 1e-3
    return w, G, np.sqrt(nr64), eps


def so3_fp32_composition(w, eps, G):
    """The float32 torch composition of the same formula on the CPU (transforms.so3_exponential_map's
    CPU branch): (R, d w) float64 numpy arrays of its float32 results.  Its distance from so3_ref
    is what float32 costs on the ill-conditioned rows."""
    from pertrenderer_amd.renderer.transforms import so3_exponential_map
    w32 = torch.as_tensor(np.asarray(w, np.float32)).clone().requires_grad_(True)
    R = so3_exponential_map(w32, eps)
    (gw,) = torch.autograd.grad((R * torch.as_tensor(np.asarray(G, np.float32))).sum(), w32)
    return R.detach().numpy().astype(np.float64), gw.numpy().astype(np.float64)


def row_err(a, ref):
    """Per-row max-abs error of a against ref (first axis = rows)."""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(ref, np.float64))
    return d.reshape(d.shape[0], -1).max(1) if d.shape[0] else np.zeros(0)


def assert_small_angle_rows(actual, ref, comp, name, margin=4.0, atol_rel=1e-6):
    """The bar of the rows below SO3_SMALL: per row, max|actual - ref| <= margin * max|comp - ref| +
    atol_rel * max|ref| (comp: the float32 CPU composition; the margin covers the kernel's other
    order of the same terms and the hardware sinf / cosf being a few ulp from the CPU's).  Returns
    (worst composition error, worst kernel error), each relative to its row's largest |ref|."""
    ref = np.asarray(ref, np.float64)
    ea, ec = row_err(actual, ref), row_err(comp, ref)
    tol = margin * ec + atol_rel * np.abs(ref).max()
    bad = ea > tol
    assert not bad.any(), f"{name}: rows {np.nonzero(bad)[0]} off by {ea[bad]} (allowed {tol[bad]})"
    scale = np.abs(ref).reshape(ref.shape[0], -1).max(1)
    return float((ec / scale).max()), float((ea / scale).max())


# --------------------------------------------------------------------------------- rotate
def rotate_ref(points, R, gout):
    """points (N,P,3) @ R ((1 or N),3,3) in float64 with both gradients for cotangent gout:
    (out, d points, d R); a shared R's gradient is summed over the batch."""
    p, r, g = (np.asarray(x, np.float32).astype(np.float64) for x in (points, R, gout))
    rb = np.broadcast_to(r, (p.shape[0], 3, 3))
    out = np.einsum("npi,nij->npj", p, rb)
    gp = np.einsum("npj,nij->npi", g, rb)
    gR = np.einsum("npi,npj->nij", p, g)
    return out, gp, (gR if r.shape[0] == p.shape[0] and p.shape[0] > 1 else gR.sum(0, keepdims=True))


def rotate_inputs(N, P, shared, seed):
    g = torch.Generator().manual_seed(seed)
    pts = torch.randn((N, P, 3), generator=g)
    R = torch.randn((1 if shared else N, 3, 3), generator=g)
    gout = torch.randn((N, P, 3), generator=g)
    return pts, R, gout


# -------------------------------------------------------------------------------- rgb_mse
MSE_THREADS, MSE_BLOCKS = 256, 512  # pr_pose.hip: kThreads, kMseBlocks


def rgb_mse_ref(img, target, gscale=1.0):
    """((img[..., :3] - target) ** 2).mean() in float64 and gscale times its image gradient
    (zero on the channels past 3)."""
    x = np.asarray(img, np.float32).astype(np.float64)
    t = np.asarray(target, np.float32).astype(np.float64)
    d = x[..., :3] - t
    g = np.zeros_like(x)
    g[..., :3] = float(gscale) * 2.0 * d / d.size
    return float((d * d).mean()), g


def mse_home_block(p, P):
    """The workgroup of rgb_mse_partial_kernel that sums pixel p of P: the grid is
    min(ceil(P / 256), 512) workgroups and pixel p = b 256 + tid + k 512 256 belongs to b."""
    nb = max(1, min((P + MSE_THREADS - 1) // MSE_THREADS, MSE_BLOCKS))
    return (np.asarray(p) % (nb * MSE_THREADS)) // MSE_THREADS, nb


def mse_late_block_case():
    """(img (3,256,256,4), target (256,256,3), region) float32: 768 pixel tiles on 512 workgroups.
    The image equals the target except on `region` (flat pixel indices), where it is target + 1;
    every pixel of the region is summed by a workgroup >= 256, which the finalize kernel reads in its
    second round only.  Targets are multiples of 1/256, so target + 1 is exact and the loss is
    |region| / P = 1/3; the fourth channel is random."""
    rng = np.random.RandomState(21)
    t = (rng.randint(0, 256, (256, 256, 3)) / 256.0).astype(np.float32)
    img = np.empty((3, 256, 256, 4), np.float32)
    img[..., :3] = t
    img[..., 3] = rng.rand(3, 256, 256)
    P = 3 * 256 * 256
    region = np.arange(MSE_BLOCKS // 2 * MSE_THREADS, MSE_BLOCKS * MSE_THREADS)  # the second image
    home, nb = mse_home_block(region, P)
    assert nb == MSE_BLOCKS and (home >= MSE_THREADS).all() and MSE_BLOCKS > MSE_THREADS
    img.reshape(P, 4)[region, :3] += 1.0
    assert np.array_equal(img.reshape(P, 4)[region, :3] - np.tile(t.reshape(-1, 3), (3, 1))[region], np.ones((region.size, 3)))
    return img, t, region


# ------------------------------------------------------------------------------ pose_step
GUARD_TAG = 0x706F7365  # "pose"
GUARD_KEY = 0x67756172645F706F  # "guard_po"


def guard_draws(seed, t, n, tag=GUARD_TAG):
    """The gradient pr_pose_step writes when the gradient norm exceeds 1000: 1e-5 times Box-Muller
    normals of Philox4x32-10 blocks with counter (t & 0xffffffff, t >> 32, i, tag) for i = 0, 4, 8,
    ... and key (seed or 0) ^ GUARD_KEY split (low, high); the first n values, float64."""
    key = ((0 if seed is None else int(seed)) ^ GUARD_KEY) & 0xFFFFFFFFFFFFFFFF
    i = np.arange(0, n, 4, dtype=np.uint32)
    ctr = np.stack([np.full(i.shape, t & 0xFFFFFFFF, np.uint32), np.full(i.shape, (t >> 32) & 0xFFFFFFFF, np.uint32), i,
                    np.full(i.shape, tag, np.uint32)], -1)
    k = np.broadcast_to(np.array([key & 0xFFFFFFFF, key >> 32], np.uint32), (i.size, 2))
    e = np.stack(philox_ref._bm4(philox_ref.philox4x32_10(ctr, k)), -1).reshape(-1)[:n]
    return 1e-5 * e


def guard_tol(draws):
    """test_philox_kat.py's gauss4 bar (2e-5 max(1, |normal|)) scaled by the guard's 1e-5."""
    return 2e-5 * 1e-5 * np.maximum(1.0, np.abs(draws) / 1e-5)


def pose_step_ref(state, inputs, dtype=np.float32):
    """One pr_pose_step call restated over `dtype` scalars.  state: dict(it, losses, gnorms, best_loss,
    best (n), v (3) / acc (3) or None, and with Adam exp_avg (n), exp_avg_sq (n), step).  inputs:
    dict(loss, log_rot (n), grad (n), niter, leaf (three values or None each; default none), post,
    seed (int or None), adam (bool), lr).  Returns (state', log_rot', grad') as new objects; when
    `it` is outside [0, niter) they equal the inputs (the kernel writes nothing)."""
    f = dtype
    st = {k: (None if v is None else (int(v) if k == "it" else np.array(v, f).copy())) for k, v in state.items()}
    log_rot, grad = np.array(inputs["log_rot"], f).reshape(-1).copy(), np.array(inputs["grad"], f).reshape(-1).copy()
    t, n = st["it"], grad.size
    if t < 0 or t >= inputs["niter"]:
        return st, log_rot, grad
    loss = f(inputs["loss"])
    st["losses"][t] = loss
    if loss < st["best_loss"]:  # False for a NaN loss
        st["best_loss"] = np.array(loss, f)
        st["best"] = log_rot.copy().reshape(st["best"].shape)
    ss = f(0)
    for g in grad:
        ss = f(ss + f(g * g))
    gn = f(np.sqrt(ss))
    st["gnorms"][t] = gn
    if gn > f(1000):
        grad = guard_draws(inputs.get("seed"), t, n).astype(f)
    if st.get("acc") is not None:
        leaf = inputs.get("leaf") or (None, None, None)
        for i in range(3):
            g = st["acc"][i]
            if leaf[i] is not None:
                g = f(g + f(leaf[i]))
            if inputs.get("post"):
                st["v"][i] = f(f(f(0.9) * st["v"][i]) + f(f(0.1) * g))
                g = f(0)
            st["acc"][i] = g
    if inputs.get("adam"):  # torch.optim.Adam's adam_math: double hyper-parameters, `dtype` state
        b1, b2, eps = 0.9, 0.999, 1e-8
        step = f(st["step"] + f(1))
        st["step"] = np.array(step, f)
        bc1, bc2 = 1.0 - b1 ** float(step), 1.0 - b2 ** float(step)
        step_size, bc2_sqrt = float(f(inputs["lr"])) / bc1, math.sqrt(bc2)
        for i in range(n):
            g = float(grad[i])
            m = f(b1 * float(st["exp_avg"].reshape(-1)[i]) + (1 - b1) * g)
            s = f(b2 * float(st["exp_avg_sq"].reshape(-1)[i]) + (1 - b2) * g * g)
            st["exp_avg"].reshape(-1)[i], st["exp_avg_sq"].reshape(-1)[i] = m, s
            denom = float(f(np.sqrt(s))) / bc2_sqrt + eps
            log_rot[i] = f(float(log_rot[i]) - step_size * float(m) / denom)
    st["it"] = t + 1
    return st, log_rot, grad


# -------------------------------------------------------------------------------- normals
def pack(verts_list, faces_list):
    """Packed (V,3) float64 vertices and (F,3) int64 faces (vertex offsets added) of a batch."""
    offs, fs = 0, []
    for v, f in zip(verts_list, faces_list):
        fs.append(torch.as_tensor(f).to(torch.int64).reshape(-1, 3).cpu() + offs)
        offs += v.shape[0]
    v = torch.cat([torch.as_tensor(v).detach().cpu().to(torch.float32).to(F64) for v in verts_list], 0)
    return v, torch.cat(fs, 0)


def _raw64(v, f):
    fv = v[f]  # (F,3,3)
    n = torch.zeros_like(v)
    n = n.index_add(0, f[:, 1], torch.cross(fv[:, 2] - fv[:, 1], fv[:, 0] - fv[:, 1], dim=1))
    n = n.index_add(0, f[:, 2], torch.cross(fv[:, 0] - fv[:, 2], fv[:, 1] - fv[:, 2], dim=1))
    return n.index_add(0, f[:, 0], torch.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=1))


def normals_raw(verts_list, faces_list):
    """(V,3) float64 unnormalised corner-cross sums of the packed batch."""
    return _raw64(*pack(verts_list, faces_list)).numpy()


def normals_ref(verts_list, faces_list, g):
    """PyTorch3D's verts_normals_packed (three index_adds of the corner crosses, then
    F.normalize(eps=1e-6)) in float64 on the float32-rounded vertices: (normals (V,3), d verts (V,3))
    for cotangent g (V,3), float64 numpy arrays."""
    v, f = pack(verts_list, faces_list)
    v.requires_grad_(True)
    n = torch.nn.functional.normalize(_raw64(v, f), eps=1e-6, dim=1)
    g64 = torch.as_tensor(np.asarray(g, np.float32)).to(F64)
    (gv,) = torch.autograd.grad((n * g64).sum(), v)
    return n.detach().numpy(), gv.numpy()


NONUNIFORM = (1.0, 0.7, 1.3)  # uneven face areas (test_gpu_normals.py's scale)
ISOLATED = (5.0, 5.0, 5.0)


def _golden_mesh(name):
    from pertrenderer_amd.renderer import load_obj
    verts, faces, _ = load_obj(os.path.join(HERE, "golden", name))
    return (verts * torch.tensor(NONUNIFORM)).to(torch.float32), faces.verts_idx.to(torch.int64)


def _cotangent(V, seed):
    return torch.randn((V, 3), generator=torch.Generator().manual_seed(seed))


# the hand-made mesh of case (c), coordinates in eighths: products of differences are exact in float32
_C_VERTS = np.array([[0, 0, 0], [8, 0, 1], [2, 8, 0], [4, 3, 7], [-5, 4, 2],  # a small fan
                     [16, 1, 0], [20, 2, 3], [17, 8, 4]], np.float32) / 8.0  # the coincident pair's own vertices
_C_FACES = np.array([[0, 1, 2], [0, 2, 4], [0, 3, 1], [1, 3, 2], [2, 3, 4],
                     [3, 3, 4],  # a repeated vertex
                     [5, 6, 7], [5, 7, 6]], np.int64)  # coincident, opposite winding
C_PAIR = (5, 6, 7)


@functools.lru_cache(maxsize=None)
def mesh_case(name):
    """(verts_list, faces_list, g) float32 / int64 CPU tensors of a normals case:
    "sphere", "cube": the golden meshes under the non-uniform scale (case a);
    "batch": the sphere, the cube with an isolated vertex appended, the sphere scaled by 1e-4, whose
       ||raw|| ~ 1e-9 is deep in F.normalize's clamp branch (case b);
    "exact": the hand-made mesh (case c).  Its cotangent on the coincident pair's vertices is
       3e-6, 5e-6, ... (float32 products of 1e-6 and small integers): d raw = g / 1e-6 is then a small integer there, every
       term of those vertices' gradient is exact and the terms cancel to zero in any order.  With a
       random cotangent those gradients are sums of terms ~1e6 |g| that cancel, and any float32
       order leaves a residue (the float32 torch composition: 0.03 to 0.25 over 20 random cotangents), which
       no bar relative to the other vertices' gradients of about 2 can hold."""
    if name in ("sphere", "cube"):
        v, f = _golden_mesh("sphere_642.obj" if name == "sphere" else "cube2.obj")
        return [v], [f], _cotangent(v.shape[0], 5)
    if name == "batch":
        (sv, sf), (cv, cf) = _golden_mesh("sphere_642.obj"), _golden_mesh("cube2.obj")
        vs = [sv, torch.cat([cv, torch.tensor([ISOLATED])], 0), (sv * 1e-4).to(torch.float32)]
        return vs, [sf, cf, sf], _cotangent(sum(v.shape[0] for v in vs), 6)
    if name == "exact":
        v, f = torch.from_numpy(_C_VERTS.copy()), torch.from_numpy(_C_FACES.copy())
        g = _cotangent(v.shape[0], 7)
        ints = torch.tensor([[3.0, -5.0, 7.0], [-9.0, 11.0, 3.0], [5.0, 13.0, -7.0]])
        g[list(C_PAIR)] = torch.tensor(1e-6, dtype=torch.float32) * ints
        assert torch.equal(g[list(C_PAIR)] / torch.tensor(1e-6, dtype=torch.float32), ints)
        return [v], [f], g
    raise KeyError(name)


def batch_ranges(verts_list):
    """Packed [start, end) of every mesh of a batch."""
    out, o = [], 0
    for v in verts_list:
        out.append((o, o + v.shape[0]))
        o += v.shape[0]
    return out

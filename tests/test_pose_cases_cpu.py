"""The float64 references of tests/pose_cases.py pinned on the CPU: against torch.matrix_exp, finite
differences, Meshes' own float64 composition, torch.optim.Adam, and the conditions the GPU tests rely
on (clamp-branch membership, the exact zero of the coincident pair, the so3 rows' clearance from the
clamp, the workgroup mapping of the rgb_mse case).  No GPU is needed."""
import numpy as np
import pytest
import torch

import pose_cases as pc
from pertrenderer_amd.renderer import Meshes


def _fd(fun, x, h):
    """Central finite difference of the scalar fun at x (numpy float64), component by component."""
    g = np.zeros_like(x)
    for i in np.ndindex(x.shape):
        xp, xm = x.copy(), x.copy()
        xp[i] += h
        xm[i] -= h
        g[i] = (fun(xp) - fun(xm)) / (2 * h)
    return g


def test_so3_ref_matches_matrix_exp_and_finite_difference():
    w, G, ang = pc.so3_inputs()
    R, gw = pc.so3_ref(w, pc.SO3_EPS, G)
    big = ang >= pc.SO3_SMALL
    assert big.sum() >= 100 and (~big).sum() >= 5
    E = torch.matrix_exp(pc.hat64(torch.from_numpy(w).double())).numpy()
    np.testing.assert_allclose(R[big], E[big], rtol=0, atol=1e-13)
    # R^T R = 1 wherever the clamp is not active
    off = ang > 0.0101 - 1e-6
    np.testing.assert_allclose(np.einsum("nji,njk->nik", R[off], R[off]), np.broadcast_to(np.eye(3), R[off].shape), atol=1e-13)
    rows = [0, 1, 3, 4, 5, 8, 11, 13, 40, 129]  # zero, below / above the clamp, pi, 2 pi, 20, random
    G64 = G.astype(np.float64)
    for n in rows:
        # the functional of row n alone; the inputs are float32 values, so w + h is formed in float64
        def fun(x, n=n):
            w64 = torch.from_numpy(x[None])
            nr = (w64 * w64).sum(1)
            a = torch.clamp(nr, float(np.float32(pc.SO3_EPS))).sqrt()
            S = pc.hat64(w64)
            Rn = (a.sin() / a)[:, None, None] * S + ((1 - a.cos()) / (a * a))[:, None, None] * (S @ S) + torch.eye(3, dtype=pc.F64)
            return float((Rn[0] * torch.from_numpy(G64[n])).sum())
        fd = _fd(fun, w[n].astype(np.float64), 1e-7 if ang[n] < pc.SO3_SMALL else 1e-6)
        np.testing.assert_allclose(gw[n], fd, rtol=1e-6, atol=1e-7, err_msg=f"row {n} angle {ang[n]}")


def test_so3_rows_keep_clear_of_the_clamp_and_cover_both_sides():
    w, _, ang = pc.so3_inputs()
    nrms = (w.astype(np.float64) ** 2).sum(1)
    assert (np.abs(nrms - 1e-4) > 1e-6).all()
    assert nrms[3] < 1e-4 < nrms[4] and abs(ang[3] - 0.0099) < 1e-6 and abs(ang[4] - 0.0101) < 1e-6
    np.testing.assert_allclose(ang[: len(pc.SO3_ANGLES)], pc.SO3_ANGLES, rtol=1e-6, atol=1e-9)
    w2, _, ang2, eps2 = pc.so3_inputs_eps()
    n2 = (w2.astype(np.float64) ** 2).sum(1)
    assert (n2 < eps2).sum() >= 3 and (n2 > eps2).sum() >= 3 and (np.abs(n2 - eps2) > 1e-4).all()
    with pytest.raises(AssertionError):
        pc.so3_rows((0.01,), 0, 1e-4)


def test_so3_ref_passes_the_gradient_on_the_clamp_boundary():
    """|w|^2 == eps exactly: the reference (torch.clamp's x >= min) differentiates through the norm
    there, as with a slightly smaller eps and unlike a slightly larger one."""
    w, G, ang, eps = pc.so3_boundary_inputs()
    R, gw = pc.so3_ref(w, eps, G)
    Rb, gb = pc.so3_ref(w, eps * (1 - 2.0 ** -20), G)
    Ra, ga = pc.so3_ref(w, eps * (1 + 2.0 ** -20), G)
    on = slice(0, 4)
    np.testing.assert_allclose(gw[on], gb[on], rtol=0, atol=1e-14)
    assert row_min_gap(gw[on], ga[on]) > 1e-3 * np.abs(gw).max()
    np.testing.assert_allclose(R[on], Rb[on], rtol=0, atol=1e-14)
    _, gc = pc.so3_fp32_composition(w, eps, G)  # and so does the float32 composition
    np.testing.assert_allclose(gc, gw, rtol=1e-5, atol=1e-6 * np.abs(gw).max())


def row_min_gap(a, b):
    return np.abs(a - b).max(1).min()


def test_so3_fp32_composition_error_is_what_the_small_rows_bar_measures():
    """The float32 composition is within the standing bar of so3_ref on the rows >= 0.02 and visibly
    off it (~1e-5 of a row's gradient) next to the clamp: the reason those rows have their own bar."""
    w, G, ang = pc.so3_inputs()
    R, gw = pc.so3_ref(w, pc.SO3_EPS, G)
    Rc, gc = pc.so3_fp32_composition(w, pc.SO3_EPS, G)
    small = ang < pc.SO3_SMALL
    rel = pc.row_err(gc, gw) / np.abs(gw).max(1)
    print("fp32 composition, d w rel. error: small rows", rel[small], "largest of the others", rel[~small].max())
    assert rel[small].max() < 1e-3 and pc.row_err(Rc, R).max() < 1e-5


def test_rotate_and_mse_refs_match_torch_float64():
    pts, R, gout = pc.rotate_inputs(3, 17, False, 1)
    p64, R64 = pts.double().requires_grad_(True), R.double().requires_grad_(True)
    out = torch.bmm(p64, R64)
    (out * gout.double()).sum().backward()
    o, gp, gR = pc.rotate_ref(pts, R, gout)
    np.testing.assert_allclose(o, out.detach().numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(gp, p64.grad.numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(gR, R64.grad.numpy(), rtol=1e-13, atol=1e-13)
    pts, R, gout = pc.rotate_inputs(4, 5, True, 2)
    R64 = R.double().requires_grad_(True)
    (torch.bmm(pts.double(), R64.expand(4, 3, 3)) * gout.double()).sum().backward()
    assert pc.rotate_ref(pts, R, gout)[2].shape == (1, 3, 3)
    np.testing.assert_allclose(pc.rotate_ref(pts, R, gout)[2], R64.grad.numpy(), rtol=1e-13, atol=1e-13)
    img = torch.rand((2, 5, 4, 5))
    for t in (torch.rand((5, 4, 3)), torch.rand((2, 5, 4, 3))):
        x = img.double().requires_grad_(True)
        val = ((x[..., :3] - t.double()) ** 2).mean()
        (g,) = torch.autograd.grad(3.0 * val, x)
        rv, rg = pc.rgb_mse_ref(img, t, 3.0)
        assert abs(rv - float(val.detach())) <= 1e-15 and np.abs(rg - g.numpy()).max() <= 1e-16
        assert np.abs(rg[..., 3:]).max() == 0.0


def test_mse_late_block_case_needs_the_finalize_kernels_second_round():
    img, t, region = pc.mse_late_block_case()
    P = img.shape[0] * img.shape[1] * img.shape[2]
    home, nb = pc.mse_home_block(np.arange(P), P)
    assert nb == 512 and P == 768 * 256
    assert np.array_equal(np.bincount(home, minlength=512), np.r_[np.full(256, 512), np.full(256, 256)])  # grid-stride
    d = (img[..., :3].astype(np.float64) - t.astype(np.float64)).reshape(P, 3)
    nz = np.nonzero(np.abs(d).max(1))[0]
    assert np.array_equal(nz, region) and (home[nz] >= 256).all()  # only partials 256..511 are non-zero
    val, _ = pc.rgb_mse_ref(img, t)
    assert abs(val - 1.0 / 3.0) < 1e-15
    assert pc.mse_home_block(np.arange(2 * 65536), 2 * 65536)[1] == 512  # (2,256,256,.): exactly 512 workgroups
    assert pc.mse_home_block([0], 1) == (0, 1)


def test_guard_draws_stream():
    a = pc.guard_draws(12345, 4, 8)
    assert np.array_equal(a, pc.guard_draws(12345, 4, 8)) and a.shape == (8,)
    assert np.array_equal(pc.guard_draws(12345, 4, 6), a[:6])
    for other in (pc.guard_draws(12345, 5, 8), pc.guard_draws(None, 4, 8), pc.guard_draws(12346, 4, 8),
                  pc.guard_draws(12345, 4 + 2 ** 32, 8), pc.guard_draws(12345, 4, 8, tag=pc.GUARD_TAG ^ 1)):
        assert np.abs(other - a).min() > 0
    assert np.array_equal(pc.guard_draws(None, 4, 8), pc.guard_draws(0, 4, 8))
    big = pc.guard_draws(7, 0, 64)
    assert big.shape == (64,) and len(np.unique(big)) == 64
    assert 0.5e-5 < big.std() < 1.5e-5 and np.abs(big).max() < 6e-5  # 1e-5 * N(0,1)
    # the key is the seed xor "guard_po", the tag "pose"
    assert pc.GUARD_KEY.to_bytes(8, "big") == b"guard_po" and pc.GUARD_TAG.to_bytes(4, "big") == b"pose"


@pytest.mark.parametrize("dtype,rtol", [(np.float64, 1e-12), (np.float32, 1e-6)])
def test_pose_step_ref_adam_matches_torch_adam(dtype, rtol):
    tdt = torch.float64 if dtype is np.float64 else torch.float32
    g = torch.Generator().manual_seed(7)
    p = torch.randn(1, 64, generator=g, dtype=tdt).requires_grad_(True)
    opt = torch.optim.Adam([p], lr=5e-2)
    lr = float(np.float32(5e-2)) if dtype is np.float32 else 5e-2
    z = np.zeros(64, dtype)
    st = dict(it=0, losses=np.zeros(8, dtype), gnorms=np.zeros(8, dtype), best_loss=np.inf, best=z, v=None, acc=None,
              exp_avg=z, exp_avg_sq=z, step=0.0)
    log_rot = p.detach().numpy().reshape(-1).copy()
    for k in range(5):
        gr = torch.randn(1, 64, generator=g, dtype=tdt)
        p.grad = gr.clone()
        opt.step()
        st, log_rot, gout = pc.pose_step_ref(st, dict(loss=1.0 - 0.1 * k, log_rot=log_rot, grad=gr.numpy(), niter=8,
                                                      adam=True, lr=lr), dtype)
        assert np.array_equal(gout, gr.numpy().reshape(-1))  # |grad| < 1000: no guard
    o = opt.state[p]
    np.testing.assert_allclose(log_rot, p.detach().numpy().reshape(-1), rtol=rtol, atol=rtol * 0.1)
    np.testing.assert_allclose(st["exp_avg"], o["exp_avg"].numpy().reshape(-1), rtol=rtol, atol=rtol * 1e-2)
    np.testing.assert_allclose(st["exp_avg_sq"], o["exp_avg_sq"].numpy().reshape(-1), rtol=rtol, atol=rtol * 1e-4)
    assert st["it"] == 5 and float(st["step"]) == float(o["step"]) == 5.0
    assert float(st["best_loss"]) == dtype(1.0 - 0.1 * 4) and st["losses"][5] == 0


def test_pose_step_ref_bookkeeping():
    z3 = np.zeros(3, np.float32)
    base = dict(it=4, losses=np.zeros(8), gnorms=np.zeros(8), best_loss=0.5, best=z3, v=[0.1, -0.2, 0.3], acc=[1, 2, 3])
    inp = dict(loss=0.25, log_rot=[0.1, 0.2, 0.3], grad=[3, 4, 0], niter=8, leaf=[0.5, None, 2.0], post=False, seed=12345)
    st, lr, gr = pc.pose_step_ref(base, inp)
    assert st["it"] == 5 and st["losses"][4] == np.float32(0.25) and st["gnorms"][4] == 5.0
    assert st["best_loss"] == np.float32(0.25) and np.array_equal(st["best"], np.float32([0.1, 0.2, 0.3]))
    assert np.array_equal(st["acc"], np.float32([1.5, 2.0, 5.0])) and np.array_equal(st["v"], np.float32([0.1, -0.2, 0.3]))
    assert np.array_equal(gr, np.float32([3, 4, 0])) and base["it"] == 4 and base["losses"][4] == 0  # inputs untouched
    # equal and NaN losses leave the best pose; the guard is strict; post folds acc into v and clears it
    st2, _, gr2 = pc.pose_step_ref(st, dict(inp, loss=0.25, log_rot=[9, 9, 9], grad=[1000, 0, 0], post=True))
    assert np.array_equal(st2["best"], st["best"]) and np.array_equal(gr2, np.float32([1000, 0, 0]))
    assert np.array_equal(st2["acc"], z3) and st2["v"][0] == np.float32(np.float32(0.9) * np.float32(0.1) + np.float32(0.1) * np.float32(2.0))
    nxt = np.nextafter(np.float32(1000), np.float32(np.inf))
    st3, _, gr3 = pc.pose_step_ref(st2, dict(inp, loss=float("nan"), grad=[nxt, 0, 0]))
    assert np.isnan(st3["losses"][6]) and st3["best_loss"] == np.float32(0.25) and st3["gnorms"][6] > 1000
    np.testing.assert_array_equal(gr3, pc.guard_draws(12345, 6, 3).astype(np.float32))
    for t in (-1, 8):
        st4, lr4, gr4 = pc.pose_step_ref(dict(st3, it=t), dict(inp, grad=[5000, 0, 0]))
        assert st4["it"] == t and np.array_equal(gr4, np.float32([5000, 0, 0]))
        assert all(np.array_equal(st4[k], np.float32(st3[k]), equal_nan=True) for k in st3 if k != "it")


def _meshes64(vs, fs):
    return Meshes([v.double().requires_grad_(True) for v in vs], fs)


@pytest.mark.parametrize("name", ["sphere", "cube", "batch", "exact"])
def test_normals_ref_matches_meshes_float64(name):
    vs, fs, g = pc.mesh_case(name)
    n, gv = pc.normals_ref(vs, fs, g)
    m = _meshes64(vs, fs)
    nm = m.verts_normals_packed()
    assert nm.dtype == torch.float64
    gm = torch.cat(torch.autograd.grad((nm * g.double()).sum(), m.verts_list()), 0)
    np.testing.assert_allclose(n, nm.detach().numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(gv, gm.numpy(), rtol=1e-10, atol=1e-10 * np.abs(gv).max())


@pytest.mark.parametrize("name", ["sphere", "cube"])
def test_normals_ref_gradient_matches_finite_difference(name):
    vs, fs, g = pc.mesh_case(name)
    _, gv = pc.normals_ref(vs, fs, g)
    v0, f = pc.pack(vs, fs)
    g64 = g.double()

    def fun(x):
        return float((torch.nn.functional.normalize(pc._raw64(x, f), eps=1e-6, dim=1) * g64).sum())

    rng = np.random.RandomState(3)
    for _ in range(4):  # directional derivatives along random directions (every vertex moves)
        d = torch.from_numpy(rng.randn(*v0.shape))
        fd = (fun(v0 + 1e-6 * d) - fun(v0 - 1e-6 * d)) / 2e-6
        an = float((torch.from_numpy(gv) * d).sum())
        assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)), (fd, an)
    i = int(np.abs(gv).max(1).argmax())  # and one vertex component by component
    e = np.zeros((3,) + tuple(v0.shape))
    for c in range(3):
        e[c, i, c] = 1.0
    fd = [(fun(v0 + 1e-6 * torch.from_numpy(e[c])) - fun(v0 - 1e-6 * torch.from_numpy(e[c]))) / 2e-6 for c in range(3)]
    np.testing.assert_allclose(gv[i], fd, rtol=1e-6, atol=1e-7)


def test_batch_case_sits_in_the_clamp_branch_far_from_its_boundary():
    vs, fs, g = pc.mesh_case("batch")
    raw = np.linalg.norm(pc.normals_raw(vs, fs), axis=1)
    (s0, s1), (c0, c1), (t0, t1) = pc.batch_ranges(vs)
    assert t1 == raw.size and ((raw[t0:t1] > 0) & (raw[t0:t1] < 1e-7)).all()
    print("scaled sphere ||raw||:", raw[t0:t1].min(), raw[t0:t1].max())
    assert raw[c1 - 1] == 0.0  # the isolated vertex
    assert (raw[s0:s1] > 1e-4).all() and (raw[c0:c1 - 1] > 1e-4).all()
    n, gv = pc.normals_ref(vs, fs, g)
    assert np.array_equal(n[c1 - 1], np.zeros(3)) and np.array_equal(gv[c1 - 1], np.zeros(3))
    np.testing.assert_allclose(n[t0:t1], pc.normals_raw(vs, fs)[t0:t1] / 1e-6, rtol=1e-12)  # x / eps
    assert 50 < np.abs(gv[t0:t1]).max() < 1000  # the clamp's gradient g / eps: ~200


def test_exact_case_gives_an_exact_zero_at_the_coincident_pair():
    vs, fs, g = pc.mesh_case("exact")
    v8 = vs[0].numpy() * 8
    assert np.array_equal(v8, np.round(v8)) and np.abs(v8).max() <= 20
    f = fs[0].numpy()
    pair = list(pc.C_PAIR)
    touching = [row for row in f if set(row) & set(pair)]
    assert len(touching) == 2 and sorted(touching[0]) == sorted(touching[1]) == pair  # no other face
    assert any(len(set(row)) == 2 for row in f)  # the repeated vertex
    raw = pc.normals_raw(vs, fs)
    n, gv = pc.normals_ref(vs, fs, g)
    assert np.array_equal(raw[pair], np.zeros((3, 3))) and np.array_equal(n[pair], np.zeros((3, 3)))
    assert (np.linalg.norm(raw[:5], axis=1) > 0.1).all()
    # the float32 CPU composition too (every product exact): zero normals and zero gradient there
    m = Meshes([vs[0].clone().requires_grad_(True)], fs)
    n32 = m.verts_normals_packed()
    (g32,) = torch.autograd.grad((n32 * g).sum(), m.verts_list())
    assert torch.equal(n32[pair].detach(), torch.zeros(3, 3))
    assert np.abs(gv[pair]).max() <= 1e-12 and float(g32[pair].abs().max()) == 0.0


def test_normals_ref_without_faces():
    v = torch.rand(5, 3)
    f = torch.zeros((0, 3), dtype=torch.int64)
    n, gv = pc.normals_ref([v], [f], torch.ones(5, 3))
    assert np.array_equal(n, np.zeros((5, 3))) and np.array_equal(gv, np.zeros((5, 3)))
    assert torch.equal(Meshes([v], [f]).verts_normals_packed(), torch.zeros(5, 3))

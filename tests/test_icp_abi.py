"""PRAlignArgs / PRIcpArgs: the ctypes layouts against gcc's offsetof on include/pertrender.h, the
host-side argument validation of pr_align_fwd / pr_icp_run (rejected before any launch, with a
pr_last_error() text), the workspace formulas, and the solve the kernels run on a cloud's moment
record (pr_align_solve_host: the float64 Jacobi SVD, the reflection fix, the scale and the
closed-form rmse) against the numpy restatement.  No GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import icp_cases as ic
from conftest import ROOT
from pertrenderer_amd import _native as nat
from pertrenderer_amd import build_native

HEADER = os.path.join(ROOT, "include", "pertrender.h")


@pytest.mark.parametrize("name", ["PRAlignArgs", "PRIcpArgs"])
def test_args_layout_matches_c_header(name):
    cls = getattr(nat, name)
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             f'printf("size %zu\\n", sizeof({name}));',
             'printf("consts %d %d %d %d\\n", PR_ICP_STATE, PR_ICP_BEGIN, PR_ICP_END, PR_ALIGN_RECORD);']
    for fname, _ in cls._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof({name}, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "l.c")
        with open(c, "w") as fh:
            fh.write("\n".join(lines))
        exe = os.path.join(td, "l")
        subprocess.check_call(["gcc", "-o", exe, c])
        got = dict(l.split(None, 1) for l in subprocess.check_output([exe]).decode().split("\n") if l)
    assert int(got["size"]) == C.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(got[fname]) == getattr(cls, fname).offset, fname
    assert got["consts"] == f"{nat.PR_ICP_STATE} {nat.PR_ICP_BEGIN} {nat.PR_ICP_END} {nat.PR_ALIGN_RECORD}"


def test_the_kernels_are_part_of_the_build():
    assert "pr_icp.hip" in build_native.SOURCES
    assert os.path.exists(os.path.join(build_native.CSRC, "pr_icp.hip"))
    assert nat.ABI_VERSION == 21 and nat.load().pr_abi_version() == 21  # additive
    for sym in ("pr_align_workspace", "pr_align_fwd", "pr_align_solve_host", "pr_icp_workspace", "pr_icp_run"):
        assert sym in nat.EXPORTS
    with open(os.path.join(build_native.CSRC, "pr_icp.hip")) as fh:
        src = fh.read()
    assert "dist2_3(" in src and "float dist2_3" not in src  # the one d^2 of pr_common.h, not a copy
    assert "atomic" not in src.lower().replace("no atomics", "")


def _filled(cls, buf, **over):
    """Every pointer set (to a host buffer that is never read: the calls below are all rejected)."""
    a = cls()
    for fname, t in cls._fields_:
        if t is C.c_void_p:
            setattr(a, fname, C.addressof(buf))
    sizes = dict(N=2, P=300, eps=1e-9) if cls is nat.PRAlignArgs else dict(N=2, P=300, Q=700, max_iterations=5)
    for k, v in {**sizes, **over}.items():
        setattr(a, k, v)
    lib = nat.load()
    a.workspace_bytes = lib.pr_align_workspace(a.N, a.P) if cls is nat.PRAlignArgs else lib.pr_icp_workspace(a.N, a.P, a.Q)
    return a


def test_argument_validation_without_gpu(monkeypatch):
    monkeypatch.delenv("PR_ICP_SPLITS", raising=False)
    lib = nat.load()
    buf = C.create_string_buffer(64)
    align, run = lib.pr_align_fwd, lambda a, k=1: lib.pr_icp_run(a, k, None)
    assert align(None, None) == -1 and b"align_fwd" in lib.pr_last_error()
    assert lib.pr_icp_run(None, 1, None) == -1 and b"icp_run" in lib.pr_last_error()
    assert align(nat.PRAlignArgs(), None) == -1 and run(nat.PRIcpArgs()) == -1
    for size in ("N", "P"):
        for bad in (0, -3):
            assert align(_filled(nat.PRAlignArgs, buf, **{size: bad}), None) == -1 and b"must be positive" in lib.pr_last_error()
    for size in ("N", "P", "Q", "max_iterations"):
        for bad in (0, -3):
            assert run(_filled(nat.PRIcpArgs, buf, **{size: bad})) == -1 and b"must be positive" in lib.pr_last_error(), size
    assert align(_filled(nat.PRAlignArgs, buf, N=65536), None) == -1 and b"65535" in lib.pr_last_error()
    assert run(_filled(nat.PRIcpArgs, buf, N=65536)) == -1 and b"65535" in lib.pr_last_error()
    assert align(_filled(nat.PRAlignArgs, buf, P=2 ** 31), None) == -1 and b"int32" in lib.pr_last_error()
    for over in (dict(P=2 ** 31), dict(Q=2 ** 31)):
        assert run(_filled(nat.PRIcpArgs, buf, **over)) == -1 and b"int32" in lib.pr_last_error()
    assert align(_filled(nat.PRAlignArgs, buf, eps=0.0), None) == -1 and b"eps" in lib.pr_last_error()
    for k in (-1, 6):
        assert run(_filled(nat.PRIcpArgs, buf), k) == -1 and b"iterations must be" in lib.pr_last_error()
    assert run(_filled(nat.PRIcpArgs, buf, phase=4)) == -1 and b"phase" in lib.pr_last_error()
    for fname in ("x", "y", "R", "T", "s"):
        a = _filled(nat.PRAlignArgs, buf)
        setattr(a, fname, None)
        assert align(a, None) == -1 and b"missing" in lib.pr_last_error(), fname
    for fname in ("x", "y", "state", "history", "rmse", "idx", "flags"):
        a = _filled(nat.PRIcpArgs, buf)
        setattr(a, fname, None)
        assert run(a) == -1 and b"missing" in lib.pr_last_error(), fname
    a = _filled(nat.PRIcpArgs, buf, phase=nat.PR_ICP_END)
    a.xt = None
    assert run(a, 0) == -1 and b"xt missing" in lib.pr_last_error()
    for cls, fn in ((nat.PRAlignArgs, lambda a: align(a, None)), (nat.PRIcpArgs, run)):
        a = _filled(cls, buf)
        a.workspace_bytes -= 1
        assert fn(a) == -3 and b"workspace" in lib.pr_last_error()  # PR_ERR_WORKSPACE
        a = _filled(cls, buf)
        a.workspace = None
        assert fn(a) == -3
    # the optional buffers (weights, lengths, idx_history) may be missing: such a call passes the
    # validation (not made here: it would launch)


def _icp_bytes(N, P, Q, splits=None):
    blocks = -(-P // 256)
    if splits is None:
        splits = max(1, min(-(-2048 // (N * blocks)), -(-Q // 512), 64))
    return 8 * (5 * N + 18 * N * blocks) + (8 * N * splits * P if splits > 1 else 0)


def test_workspace_formulas(monkeypatch):
    lib = nat.load()
    monkeypatch.delenv("PR_ICP_SPLITS", raising=False)
    # (Xmu, sum w) and the previous rmse per cloud, one 18-double record per 256 queries, and with
    # S > 1 database ranges a (d^2, index) pair per query and range
    for N, P, Q in ((1, 65, 513), (3, 64, 512), (4, 5000, 20000), (2, 257, 1025), (64, 100000, 100), (1, 1, 1)):
        assert lib.pr_icp_workspace(N, P, Q) == _icp_bytes(N, P, Q), (N, P, Q)
        assert lib.pr_align_workspace(N, P) == 8 * (5 * N + 18 * N * -(-P // 256))
    assert _icp_bytes(4, 5000, 20000) == 8 * (20 + 18 * 4 * 20) + 8 * 4 * 26 * 5000  # 26 ranges
    assert _icp_bytes(64, 100000, 100) == 8 * (5 * 64 + 18 * 64 * 391)  # enough queries: unsplit
    for s, want in (("3", 3), ("1", 1), ("1000", 64), ("0", None), ("x", None)):
        monkeypatch.setenv("PR_ICP_SPLITS", s)  # read per call
        assert lib.pr_icp_workspace(2, 257, 1025) == _icp_bytes(2, 257, 1025, want), s
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (65536, 4, 4), (1, 2 ** 31, 4), (1, 4, 2 ** 31)):
        assert lib.pr_icp_workspace(*bad) == 0, bad
    for bad in ((0, 4), (1, 0), (65536, 4), (1, 2 ** 31)):
        assert lib.pr_align_workspace(*bad) == 0, bad


def _record(X, Y, w):
    """The record the kernels sum (include/pertrender.h) in float64 numpy, and (Xmu, sum w)."""
    ws = w.sum()
    xmu = (X * w[:, None]).sum(0) / max(ws, 1e-9)
    a, d, w2 = X - xmu, Y - xmu, w * w
    m = np.concatenate([[ws], (w[:, None] * d).sum(0), np.einsum("p,pj,pk->jk", w2, a, d).ravel(), [(w2 * (a * a).sum(1)).sum()],
                        [(w * (d * d).sum(1)).sum()], (w2[:, None] * a).sum(0)])
    return m, np.concatenate([xmu, [ws]])


def _solve(X, Y, w, weighted=True, scale=False, reflect=False):
    m, xmu = _record(np.asarray(X, np.float64), np.asarray(Y, np.float64), np.asarray(w, np.float64))
    out = np.zeros(14)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    assert nat.load().pr_align_solve_host(dp(m), dp(xmu), int(weighted), 1e-9, int(scale), int(reflect), dp(out)) == 0
    return out[:9].reshape(3, 3), out[9:12], out[12], out[13]


@pytest.mark.parametrize("scale", [False, True])
@pytest.mark.parametrize("reflect", [False, True])
def test_host_solve_matches_restatement(scale, reflect):
    rng = np.random.RandomState(0)
    X, Y, w = rng.uniform(-1, 1, (1, 30, 3)), rng.uniform(-1, 1, (1, 30, 3)), rng.uniform(0, 2, (1, 30))
    R, T, s, _ = _solve(X[0], Y[0], w[0], True, scale, reflect)
    ref = ic.align(X, Y, w, scale, reflect)
    assert np.abs(R - ref[0][0]).max() <= 1e-13 and np.abs(T - ref[1][0]).max() <= 1e-13 and abs(s - ref[2][0]) <= 1e-13
    R, T, s, _ = _solve(X[0], Y[0], np.ones(30), False, scale, reflect)  # no weights: total = the count
    ref = ic.align(X, Y, None, scale, reflect)
    assert np.abs(R - ref[0][0]).max() <= 1e-13 and np.abs(T - ref[1][0]).max() <= 1e-13 and abs(s - ref[2][0]) <= 1e-13


def test_host_solve_copies_reflection_and_rmse():
    X, Y, R0, T0 = ic.rigid_copy(scale=1.3)
    R, T, s, rmse = _solve(X[0], Y[0], np.ones(40), scale=True)
    assert np.abs(R - R0[0]).max() <= 1e-6 and np.abs(T - T0[0]).max() <= 1e-6 and abs(s - 1.3) <= 1e-6  # Y is rounded to float32
    assert abs(np.linalg.det(R) - 1) <= 1e-14 and np.abs(R @ R.T - np.eye(3)).max() <= 1e-14 and rmse <= 1e-6
    X, Y, R0, _ = ic.rigid_copy(mirror=True)
    R, _, _, _ = _solve(X[0], Y[0], np.ones(40), reflect=True)
    assert np.abs(R - R0[0]).max() <= 1e-6 and abs(np.linalg.det(R) + 1) <= 1e-14
    R, _, _, rmse = _solve(X[0], Y[0], np.ones(40))
    ref = ic.align(X[:1].astype(np.float64), Y[:1].astype(np.float64))
    assert abs(np.linalg.det(R) - 1) <= 1e-14 and np.abs(R - ref[0][0]).max() <= 1e-13 and rmse > 0.1
    # the closed-form rmse against the residual of the transformed points, on an ICP iteration's pairs
    Xs, Ys, _, _ = ic.scene(1, 65, 513, 0)
    one = ic.icp(Xs.astype(np.float64), Ys.astype(np.float64), max_iterations=1, thr=-1.0)
    R, T, s, rmse = _solve(Xs[0], Ys[0][one["idx"][0][0]], np.ones(65))
    assert abs(rmse - one["rmse"][0]) <= 1e-12 * one["rmse"][0] and np.abs(R - one["R"][0][0]).max() <= 1e-13


def test_host_solve_degenerate_inputs():
    eye = np.eye(3)
    R, T, s, rmse = _solve(np.zeros((5, 3)), np.zeros((5, 3)), np.zeros(5))  # an empty cloud: all weights 0
    assert np.array_equal(R, eye) and np.array_equal(T, np.zeros(3)) and s == 1 and rmse == 0
    assert _solve(np.zeros((5, 3)), np.zeros((5, 3)), np.zeros(5), scale=True)[2] == 0  # the formula's value
    line = np.linspace(0, 1, 8)[:, None] * np.array([1.0, 0.0, 0.0])
    R, T, _, _ = _solve(line, line + 1.0, np.ones(8))  # rank 1: some orthonormal R that maps the line
    assert np.abs(R @ R.T - eye).max() <= 1e-14 and abs(np.linalg.det(R) - 1) <= 1e-14
    assert np.abs(line @ R + T - (line + 1.0)).max() <= 1e-14
    rng = np.random.RandomState(1)
    plane = rng.uniform(-1, 1, (10, 3))
    plane[:, 2] = 0
    Rz = ic.rotation((0, 0, 1), 30.0)
    R, _, _, _ = _solve(plane, plane @ Rz, np.ones(10))  # rank 2: the rotation is still unique
    assert np.abs(R - Rz).max() <= 1e-14
    bad = plane.copy()
    bad[0, 0] = np.nan
    for X, Y in ((bad, plane), (plane, bad)):
        R, T, s, rmse = _solve(X, Y, np.ones(10))
        assert np.isnan(R).all() and np.isnan(T).all() and np.isnan(s) and np.isnan(rmse)
    tiny = rng.uniform(-1, 1, (10, 3)) * 1e-150  # squares underflow without the solve's scaling
    R, _, _, _ = _solve(tiny, tiny @ Rz, np.ones(10))
    assert np.abs(R - Rz).max() <= 1e-12

"""PRNormalConsistencyArgs and PRChamferArgs: the ctypes layouts against gcc's offsetof on
include/pertrender.h, the host-side argument validation of their entry points (rejected before any
launch), and pr_chamfer_workspace.  No GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from conftest import ROOT
from pertrenderer_amd import _native as nat

HEADER = os.path.join(ROOT, "include", "pertrender.h")


@pytest.mark.parametrize("name", ["PRNormalConsistencyArgs", "PRChamferArgs"])
def test_args_layout_matches_c_header(name):
    cls = getattr(nat, name)
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             f'printf("size %zu\\n", sizeof({name}));']
    for fname, _ in cls._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof({name}, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "l.c")
        with open(c, "w") as fh:
            fh.write("\n".join(lines))
        exe = os.path.join(td, "l")
        subprocess.check_call(["gcc", "-o", exe, c])
        got = dict(l.split() for l in subprocess.check_output([exe]).decode().split("\n") if l)
    assert int(got["size"]) == C.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(got[fname]) == getattr(cls, fname).offset, fname


def _filled(cls, buf, **sizes):
    """Every pointer set (to a host buffer that is never read: the calls below are all rejected)."""
    a = cls()
    for fname, t in cls._fields_:
        if t is C.c_void_p:
            setattr(a, fname, C.addressof(buf))
    for k, v in sizes.items():
        setattr(a, k, v)
    return a


def test_normal_consistency_argument_validation_without_gpu():
    lib = nat.load()
    buf = C.create_string_buffer(64)
    cls = nat.PRNormalConsistencyArgs
    required = {
        "pr_mesh_normal_consistency_fwd": ["verts", "faces", "pair_start", "pair_partner", "face_normal", "face_sum",
                                           "partials", "loss"],
        "pr_mesh_normal_consistency_bwd": ["verts", "faces", "vert_corner_start", "vert_corners", "face_normal",
                                           "face_sum", "face_grad", "grad_loss", "grad_verts"],
    }
    for name, fields in required.items():
        fn = getattr(lib, name)
        assert fn(None, None) == -1 and name[3:].encode() in lib.pr_last_error()
        assert fn(cls(), None) == -1
        for size in ("V", "F", "P"):  # P = 0 is the caller's case: nothing to launch
            for bad in (0, -2):
                a = _filled(cls, buf, V=4, F=2, P=1)
                setattr(a, size, bad)
                assert fn(a, None) == -1 and b"must be positive" in lib.pr_last_error(), (name, size)
        for fname in fields:
            a = _filled(cls, buf, V=4, F=2, P=1)
            setattr(a, fname, None)
            assert fn(a, None) == -1, (name, fname)
            assert b"missing" in lib.pr_last_error(), (name, fname)


def test_chamfer_argument_validation_without_gpu(monkeypatch):
    monkeypatch.delenv("PR_CHAMFER_SPLITS", raising=False)  # the workspace cases below need the shape's own ranges
    lib = nat.load()
    buf = C.create_string_buffer(64)
    cls = nat.PRChamferArgs
    required = {
        "pr_chamfer_fwd": ["x", "y", "dist_x", "dist_y", "idx_x", "idx_y"],
        "pr_chamfer_bwd": ["x", "y", "idx_x", "idx_y", "grad_dist_x", "grad_dist_y", "grad_x", "grad_y"],
    }
    for name, fields in required.items():
        fn = getattr(lib, name)
        assert fn(None, None) == -1 and name[3:].encode() in lib.pr_last_error()
        assert fn(cls(), None) == -1
        for size in ("N", "P", "Q"):
            for bad in (0, -1):
                a = _filled(cls, buf, N=1, P=3, Q=5)
                setattr(a, size, bad)
                assert fn(a, None) == -1 and b"must be positive" in lib.pr_last_error(), (name, size)
        a = _filled(cls, buf, N=1, P=2 ** 31, Q=5)
        assert fn(a, None) == -1 and b"int32" in lib.pr_last_error()
        a = _filled(cls, buf, N=32768, P=3, Q=5)  # 2 N workgroups along gridDim.z
        assert fn(a, None) == -1 and b"32767" in lib.pr_last_error()
        a = _filled(cls, buf, N=1, P=3, Q=2 ** 31)
        assert fn(a, None) == -1 and b"int32" in lib.pr_last_error()
        for fname in fields:
            a = _filled(cls, buf, N=1, P=3, Q=5)
            setattr(a, fname, None)
            assert fn(a, None) == -1, (name, fname)
            assert b"missing" in lib.pr_last_error(), (name, fname)
    # a split shape needs its workspace, both ways: none, or one that is too small, is rejected before the launch
    need = lib.pr_chamfer_workspace(1, 5000, 5000)
    for ws, nbytes in ((None, need), (C.addressof(buf), need - 1)):
        a = _filled(cls, buf, N=1, P=5000, Q=5000)
        a.workspace, a.workspace_bytes = ws, nbytes
        for fn in (lib.pr_chamfer_fwd, lib.pr_chamfer_bwd):
            assert fn(a, None) == -1 and b"workspace" in lib.pr_last_error()


def test_chamfer_workspace(monkeypatch):
    lib = nat.load()
    monkeypatch.delenv("PR_CHAMFER_SPLITS", raising=False)
    # 2 x 1 workgroups of queries, one tile of database points: one range, no workspace
    assert lib.pr_chamfer_workspace(2, 64, 65) == 0
    assert lib.pr_chamfer_workspace(0, 64, 65) == 0 and lib.pr_chamfer_workspace(1, -1, 5) == 0
    # 20 workgroups of queries against 10 tiles of 512 points: min(ceil(2048 / 20), 10) = 10 ranges
    # each way, 12 bytes per point and range (forward: distance and index; backward: a partial gradient)
    assert lib.pr_chamfer_workspace(1, 5000, 5000) == 2 * 5000 * 10 * 12
    # only the 257 queries are split (over the 3 tiles of 1025 points); 1025 queries face one tile
    assert lib.pr_chamfer_workspace(2, 257, 1025) == 2 * 257 * 3 * 12
    monkeypatch.setenv("PR_CHAMFER_SPLITS", "3")  # read per call
    assert lib.pr_chamfer_workspace(2, 64, 65) == 2 * (64 + 65) * 3 * 12
    monkeypatch.setenv("PR_CHAMFER_SPLITS", "1")
    assert lib.pr_chamfer_workspace(1, 5000, 5000) == 0

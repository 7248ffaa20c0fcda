"""PRMeshLossArgs: the ctypes layout against gcc's offsetof on include/pertrender.h, and the
host-side argument validation of the pr_mesh_* entry points (rejected before any launch).  No GPU."""
import ctypes as C
import os
import subprocess
import tempfile

from conftest import ROOT
from pertrenderer_amd import _native as nat

HEADER = os.path.join(ROOT, "include", "pertrender.h")


def test_mesh_loss_args_layout_matches_c_header():
    cls = nat.PRMeshLossArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(PRMeshLossArgs));']
    for fname, _ in cls._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(PRMeshLossArgs, {fname}));')
    lines.append('printf("methods %d %d %d\\n", PR_MESH_LAP_UNIFORM, PR_MESH_LAP_COT, PR_MESH_LAP_COTCURV);')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "l.c")
        with open(c, "w") as fh:
            fh.write("\n".join(lines))
        exe = os.path.join(td, "l")
        subprocess.check_call(["gcc", "-o", exe, c])
        out = [l.split() for l in subprocess.check_output([exe]).decode().split("\n") if l]
    got = {l[0]: l[1:] for l in out}
    assert int(got["size"][0]) == C.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(got[fname][0]) == getattr(cls, fname).offset, fname
    assert [int(x) for x in got["methods"]] == [nat.PR_MESH_LAP_UNIFORM, nat.PR_MESH_LAP_COT, nat.PR_MESH_LAP_COTCURV]


def _filled(buf):
    """Every pointer set (to a host buffer that is never read: the calls below are all rejected)."""
    a = nat.PRMeshLossArgs()
    for fname, t in nat.PRMeshLossArgs._fields_:
        if t is C.c_void_p:
            setattr(a, fname, C.addressof(buf))
    a.V, a.F = 4, 2
    return a


def test_mesh_loss_argument_validation_without_gpu():
    lib = nat.load()
    buf = C.create_string_buffer(64)
    fns = {"pr_mesh_laplacian_fwd": lib.pr_mesh_laplacian_fwd, "pr_mesh_laplacian_bwd": lib.pr_mesh_laplacian_bwd,
           "pr_mesh_edge_fwd": lib.pr_mesh_edge_fwd, "pr_mesh_edge_bwd": lib.pr_mesh_edge_bwd}
    for name, fn in fns.items():
        assert fn(None, None) == -1 and name[3:].encode() in lib.pr_last_error()
        assert fn(nat.PRMeshLossArgs(), None) == -1  # all zero: V <= 0
        a = _filled(buf)
        a.V = 0
        assert fn(a, None) == -1 and b"V must be positive" in lib.pr_last_error()
        a = _filled(buf)
        a.V = -3
        assert fn(a, None) == -1
    # an unknown method
    for fn in (lib.pr_mesh_laplacian_fwd, lib.pr_mesh_laplacian_bwd):
        a = _filled(buf)
        a.method = 3
        assert fn(a, None) == -1 and b"unknown method 3" in lib.pr_last_error()
    # null required pointers, per entry point and method
    required = {
        ("pr_mesh_laplacian_fwd", nat.PR_MESH_LAP_UNIFORM): ["verts", "weight", "nbr_start", "nbr", "gather", "diag",
                                                              "partials", "loss"],
        ("pr_mesh_laplacian_fwd", nat.PR_MESH_LAP_COT): ["verts", "weight", "faces", "vert_corner_start", "vert_corners",
                                                          "face_cot", "gather", "diag", "partials", "loss"],
        ("pr_mesh_laplacian_bwd", nat.PR_MESH_LAP_UNIFORM): ["nbr_start", "nbr", "gather", "diag", "grad_loss",
                                                              "grad_verts"],
        ("pr_mesh_laplacian_bwd", nat.PR_MESH_LAP_COTCURV): ["faces", "vert_corner_start", "vert_corners", "face_cot",
                                                              "gather", "diag", "grad_loss", "grad_verts"],
        ("pr_mesh_edge_fwd", 0): ["verts", "weight", "nbr_start", "nbr", "partials", "loss"],
        ("pr_mesh_edge_bwd", 0): ["verts", "weight", "nbr_start", "nbr", "grad_loss", "grad_verts"],
    }
    for (name, method), fields in required.items():
        for fname in fields:
            a = _filled(buf)
            a.method = method
            setattr(a, fname, None)
            assert fns[name](a, None) == -1, (name, fname)
            assert b"missing" in lib.pr_last_error(), (name, fname)
    assert lib.pr_mesh_loss_workspace(642) == 3 and lib.pr_mesh_loss_workspace(0) == 1
    assert lib.pr_mesh_loss_workspace(10 ** 7) == 512

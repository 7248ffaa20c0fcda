"""PRPointMeshArgs: the ctypes layout against gcc's offsetof on include/pertrender.h, the host-side
argument validation of pr_point_mesh_fwd / _bwd (rejected before any launch), and
pr_point_mesh_workspace.  No GPU."""
import ctypes as C
import os
import subprocess
import tempfile

from conftest import ROOT
from pertrenderer_amd import _native as nat
from pertrenderer_amd import build_native

HEADER = os.path.join(ROOT, "include", "pertrender.h")


def test_args_layout_matches_c_header():
    name, cls = "PRPointMeshArgs", nat.PRPointMeshArgs
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


def test_the_kernels_are_part_of_the_build():
    assert "pr_pointmesh.hip" in build_native.SOURCES
    assert os.path.exists(os.path.join(build_native.CSRC, "pr_pointmesh.hip"))
    assert nat.ABI_VERSION == 21  # additive


SIZES = dict(N=2, P=14, V=9, M=5, max_points=9, max_prims=3)


def _filled(buf, **over):
    """Every pointer set (to a host buffer that is never read: the calls below are all rejected)."""
    cls = nat.PRPointMeshArgs
    a = cls()
    for fname, t in cls._fields_:
        if t is C.c_void_p:
            setattr(a, fname, C.addressof(buf))
    for k, v in {**SIZES, **over}.items():
        setattr(a, k, v)
    a.workspace_bytes = nat.load().pr_point_mesh_workspace(a.prim, a.N, a.P, a.M, a.max_points, a.max_prims)
    return a


REQUIRED = {
    "pr_point_mesh_fwd": ["points", "verts", "prims", "mesh_first", "mesh_count", "dist_p", "idx_p", "w_p", "dist_m",
                          "idx_m", "w_m", "workspace"],
    "pr_point_mesh_bwd": ["points", "verts", "prims", "idx_p", "w_p", "idx_m", "w_m", "workspace", "prim_point_start",
                          "prim_points", "point_prim_start", "point_prims", "vert_corner_start", "vert_corners",
                          "grad_dist_p", "grad_dist_m", "grad_points", "grad_verts"],
}


def test_argument_validation_without_gpu(monkeypatch):
    monkeypatch.delenv("PR_POINTMESH_SPLITS", raising=False)
    lib = nat.load()
    buf = C.create_string_buffer(64)
    for name, fields in REQUIRED.items():
        fn = getattr(lib, name)
        assert fn(None, None) == -1 and name[3:].encode() in lib.pr_last_error()
        assert fn(nat.PRPointMeshArgs(), None) == -1
        for size in SIZES:
            for bad in (0, -3):
                a = _filled(buf)
                setattr(a, size, bad)
                assert fn(a, None) == -1, (name, size)
                assert b"must be positive" in lib.pr_last_error(), (name, size)
        for prim in (2, -1):
            a = _filled(buf)
            a.prim = prim
            assert fn(a, None) == -1 and b"prim must be 0 (faces) or 1 (edges)" in lib.pr_last_error()
        a = _filled(buf)
        a.N = 32768
        assert fn(a, None) == -1 and b"32767" in lib.pr_last_error()
        for size, big in (("P", 2 ** 31), ("V", 2 ** 31), ("M", 2 ** 27)):
            a = _filled(buf)
            setattr(a, size, big)
            assert fn(a, None) == -1 and b"int32" in lib.pr_last_error(), size
        for size, other in (("max_points", "P"), ("max_prims", "M")):
            a = _filled(buf)
            setattr(a, size, SIZES[other] + 1)
            assert fn(a, None) == -1 and b"exceed" in lib.pr_last_error(), size
        # a padded batch (no cloud_first) must be N max_points rows long
        a = _filled(buf)
        a.cloud_first = None
        assert fn(a, None) == -1 and b"padded batch" in lib.pr_last_error()
        for fname in fields:
            a = _filled(buf)
            setattr(a, fname, None)
            assert fn(a, None) == -1, (name, fname)
            assert b"missing" in lib.pr_last_error(), (name, fname)
        a = _filled(buf)
        a.workspace_bytes -= 1
        assert fn(a, None) == -1 and b"workspace" in lib.pr_last_error()
    # cloud_count is optional, and cloud_first with P = N max_points (a padded batch): such calls pass
    # the validation; they are not made here (they would launch)


def test_workspace_size(monkeypatch):
    lib = nat.load()
    monkeypatch.setenv("PR_POINTMESH_SPLITS", "1")
    # no ranges: the forward's records (16 floats per triangle, 8 per segment); the backward's corner
    # gradients (3 x 3 or 2 x 3 floats) fit into them
    assert lib.pr_point_mesh_workspace(0, 1, 5000, 1280, 5000, 1280) == 1280 * 16 * 4
    assert lib.pr_point_mesh_workspace(1, 1, 5000, 1920, 5000, 1920) == 1920 * 8 * 4
    monkeypatch.setenv("PR_POINTMESH_SPLITS", "3")
    # three ranges each way: (d^2, index) pairs per range and query, on both sides
    assert lib.pr_point_mesh_workspace(0, 1, 5000, 1280, 5000, 1280) == 1280 * 16 * 4 + 3 * 8 * (5000 + 1280)
    monkeypatch.delenv("PR_POINTMESH_SPLITS")
    # the library's choice: one point against 1280 faces is cut into one range per tile of 128 triangles,
    # 1280 faces against one point are not cut
    assert lib.pr_point_mesh_workspace(0, 1, 1, 1280, 1, 1280) == 1280 * 16 * 4 + 10 * 8 * 1
    for bad in ((2, 1, 5, 5, 5, 5), (0, 0, 5, 5, 5, 5), (0, 1, 0, 5, 1, 5), (0, 1, 5, 0, 5, 1), (0, 1, 5, 5, 6, 5),
                (0, 1, 5, 5, 5, 0), (0, 40000, 5, 5, 5, 5)):
        assert lib.pr_point_mesh_workspace(*bad) == 0, bad

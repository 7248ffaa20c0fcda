"""PRSamplePointsArgs: the ctypes layout against gcc's offsetof on include/pertrender.h, the
host-side argument validation of pr_sample_points_fwd / _bwd (rejected before any launch), and
pr_sample_points_workspace.  No GPU."""
import ctypes as C
import os
import subprocess
import tempfile

from conftest import ROOT
from pertrenderer_amd import _native as nat

HEADER = os.path.join(ROOT, "include", "pertrender.h")


def test_args_layout_matches_c_header():
    name, cls = "PRSamplePointsArgs", nat.PRSamplePointsArgs
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


SIZES = dict(N=2, S=7, V=9, F=5)


def _filled(buf, **over):
    """Every pointer set (to a host buffer that is never read: the calls below are all rejected)."""
    cls = nat.PRSamplePointsArgs
    a = cls()
    for fname, t in cls._fields_:
        if t is C.c_void_p:
            setattr(a, fname, C.addressof(buf))
    a.noise_mode = nat.PR_NOISE_INJECTED
    a.workspace_bytes = nat.load().pr_sample_points_workspace(SIZES["F"])
    for k, v in {**SIZES, **over}.items():
        setattr(a, k, v)
    return a


REQUIRED = {
    "pr_sample_points_fwd": ["verts", "faces", "mesh_first_face", "mesh_num_faces", "uniforms", "cdf", "samples",
                             "face_idx", "w", "workspace"],
    "pr_sample_points_bwd": ["verts", "faces", "w", "workspace", "face_sample_start", "face_samples",
                             "vert_corner_start", "vert_corners", "grad_samples", "grad_verts"],
}


def test_argument_validation_without_gpu():
    lib = nat.load()
    buf = C.create_string_buffer(64)
    for name, fields in REQUIRED.items():
        fn = getattr(lib, name)
        assert fn(None, None) == -1 and name[3:].encode() in lib.pr_last_error()
        assert fn(nat.PRSamplePointsArgs(), None) == -1
        for size in SIZES:
            for bad in (0, -3):
                assert fn(_filled(buf, **{size: bad}), None) == -1, (name, size)
                assert b"must be positive" in lib.pr_last_error(), (name, size)
        assert fn(_filled(buf, N=65536), None) == -1 and b"65535" in lib.pr_last_error()
        assert fn(_filled(buf, N=2, S=2 ** 30), None) == -1 and b"int32" in lib.pr_last_error()  # N S = 2^31
        assert fn(_filled(buf, N=1, S=2 ** 31), None) == -1 and b"int32" in lib.pr_last_error()
        for fname in fields:
            a = _filled(buf)
            setattr(a, fname, None)
            assert fn(a, None) == -1, (name, fname)
            assert b"missing" in lib.pr_last_error(), (name, fname)
        a = _filled(buf)
        a.workspace_bytes -= 1
        assert fn(a, None) == -1 and b"workspace" in lib.pr_last_error()
    # the optional pointers: no normals, no grad_normals, no device key base; Philox needs no uniforms.
    # Such a call passes the validation; it is not made here (it would launch).
    a = _filled(buf, noise_mode=7)
    assert lib.pr_sample_points_fwd(a, None) == -1 and b"noise_mode" in lib.pr_last_error()


def test_workspace_size():
    lib = nat.load()
    # the backward's (F,3,3) float corner gradients; the forward's F areas fit into it
    assert lib.pr_sample_points_workspace(1280) == 1280 * 9 * 4
    assert lib.pr_sample_points_workspace(0) == 0 and lib.pr_sample_points_workspace(-4) == 0

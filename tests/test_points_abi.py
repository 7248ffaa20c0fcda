"""PRPointsRastArgs / PRPointsCompositeArgs: the ctypes layouts against gcc's offsetof on
include/pertrender.h, the host-side argument validation of the pr_points_* entry points (rejected
before any launch, with a pr_last_error() text) and pr_points_workspace.  No GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from conftest import ROOT
from pertrenderer_amd import _native as nat
from pertrenderer_amd import build_native

HEADER = os.path.join(ROOT, "include", "pertrender.h")


@pytest.mark.parametrize("name", ["PRPointsRastArgs", "PRPointsCompositeArgs"])
def test_args_layout_matches_c_header(name):
    cls = getattr(nat, name)
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             f'printf("size %zu\\n", sizeof({name}));', 'printf("maxk %d\\n", PR_POINTS_MAX_K);',
             'printf("modes %d%d%d\\n", PR_POINTS_ALPHA, PR_POINTS_NORM, PR_POINTS_WEIGHTED);']
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
    assert int(got["maxk"]) == nat.PR_POINTS_MAX_K >= 64
    assert got["modes"] == f"{nat.PR_POINTS_ALPHA}{nat.PR_POINTS_NORM}{nat.PR_POINTS_WEIGHTED}"


def test_the_kernels_are_part_of_the_build():
    assert "pr_points.hip" in build_native.SOURCES
    assert os.path.exists(os.path.join(build_native.CSRC, "pr_points.hip"))
    assert nat.ABI_VERSION == 21 and nat.load().pr_abi_version() == 21  # additive
    for sym in ("pr_points_workspace", "pr_points_rast_fwd", "pr_points_rast_bwd", "pr_points_composite_fwd",
                "pr_points_composite_bwd"):
        assert sym in nat.EXPORTS


def test_ndc_is_shared_not_copied():
    """One definition of the pixel-centre function, in pr_common.h, used by both rasterizers."""
    count = {}
    for f in os.listdir(build_native.CSRC):
        if not f.endswith((".hip", ".h", ".cpp")):
            continue
        with open(os.path.join(build_native.CSRC, f)) as fh:
            count[f] = fh.read().count("float ndc(int")
    assert count.pop("pr_common.h") == 1 and not any(count.values()), count


SIZES = dict(N=2, H=5, W=7, K=3, P=11)


def _filled(cls, buf, **over):
    """Every pointer set (to a host buffer that is never read: the calls below are all rejected)."""
    a = cls()
    for fname, t in cls._fields_:
        if t is C.c_void_p:
            setattr(a, fname, C.addressof(buf))
    for k, v in {**SIZES, **over}.items():
        setattr(a, k, v)
    if cls is nat.PRPointsCompositeArgs:
        a.C = over.get("C", 3)
        a.workspace_bytes = nat.load().pr_points_workspace(a.N, a.H, a.W, a.K)
    return a


REQUIRED = {
    "pr_points_rast_fwd": (nat.PRPointsRastArgs, ["points", "cloud_first", "cloud_count", "idx", "zbuf", "dists"]),
    "pr_points_rast_bwd": (nat.PRPointsRastArgs, ["points", "idx", "point_start", "point_entries", "grad_zbuf", "grad_dists",
                                                  "grad_points"]),
    "pr_points_composite_fwd": (nat.PRPointsCompositeArgs, ["idx", "alphas", "features", "out"]),
    "pr_points_composite_bwd": (nat.PRPointsCompositeArgs, ["idx", "alphas", "features", "workspace", "point_start",
                                                            "point_entries", "grad_out", "grad_alphas", "grad_features"]),
}


def test_argument_validation_without_gpu():
    lib = nat.load()
    buf = C.create_string_buffer(64)
    for name, (cls, fields) in REQUIRED.items():
        fn = getattr(lib, name)
        assert fn(None, None) == -1 and name[3:].encode() in lib.pr_last_error()
        assert fn(cls(), None) == -1
        for size in SIZES:
            for bad in (0, -3):
                a = _filled(cls, buf, **{size: bad})
                assert fn(a, None) == -1, (name, size)
                assert b"must be positive" in lib.pr_last_error(), (name, size)
        a = _filled(cls, buf, N=65536)
        assert fn(a, None) == -1 and b"65535" in lib.pr_last_error()
        a = _filled(cls, buf, H=65535 * 8 + 1, W=1, K=1, N=1)  # grid.y of the forward's 8 x 8 tiles
        assert fn(a, None) == -1 and b"H must fit the grid" in lib.pr_last_error()
        for over in (dict(H=40000, W=40000), dict(P=2 ** 31)):
            a = _filled(cls, buf, **over)
            assert fn(a, None) == -1 and b"int32" in lib.pr_last_error(), over
        for fname in fields:
            a = _filled(cls, buf)
            setattr(a, fname, None)
            assert fn(a, None) == -1, (name, fname)
            assert b"missing" in lib.pr_last_error(), (name, fname)
    for name in ("pr_points_rast_fwd", "pr_points_rast_bwd"):
        a = _filled(nat.PRPointsRastArgs, buf, K=nat.PR_POINTS_MAX_K + 1)
        assert getattr(lib, name)(a, None) == -1 and b"PR_POINTS_MAX_K" in lib.pr_last_error()
    for name in ("pr_points_composite_fwd", "pr_points_composite_bwd"):
        fn = getattr(lib, name)
        for mode in (3, -1):
            a = _filled(nat.PRPointsCompositeArgs, buf)
            a.mode = mode
            assert fn(a, None) == -1 and b"mode must be" in lib.pr_last_error()
        a = _filled(nat.PRPointsCompositeArgs, buf, C=0)
        assert fn(a, None) == -1 and b"C must be positive" in lib.pr_last_error()
    a = _filled(nat.PRPointsCompositeArgs, buf)
    a.workspace_bytes -= 1
    assert lib.pr_points_composite_bwd(a, None) == -1 and b"workspace" in lib.pr_last_error()
    # the per-point radius tensor is optional: a forward without it passes the validation (not called: it would launch)


def test_workspace_size():
    lib = nat.load()
    assert lib.pr_points_workspace(4, 256, 256, 8) == 4 * 256 * 256 * 8 * 4  # one float per fragment slot
    assert lib.pr_points_workspace(1, 1, 1, 100) == 400  # the compositors take any K
    assert lib.pr_points_workspace(1, 65535 * 8, 1, 1) == 65535 * 8 * 4
    for bad in ((0, 4, 4, 1), (1, 0, 4, 1), (1, 4, 0, 1), (1, 4, 4, 0), (65536, 4, 4, 1), (4, 40000, 40000, 1),
                (1, 65535 * 8 + 1, 1, 1)):
        assert lib.pr_points_workspace(*bad) == 0, bad

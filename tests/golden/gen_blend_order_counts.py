"""Fixture generator for tests/test_blend_order_cpu.py: the bench frame's valid slots per pixel.

The frame is bench.WorkloadCPU's (sphere_642, 256 x 256, faces_per_pixel = 50, the pose of step 0),
rasterized by the project's own CPU oracle (oracle/rast_ref.rast_fwd); the fixture keeps only the
number of valid slots of every pixel, 256 x 256 uint8, in tests/golden/blend_order_counts.npz.
Re-run with::

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_blend_order_counts.py
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, ROOT)


def bench_frame_counts():
    import bench
    from oracle import rast_ref
    wl = bench.WorkloadCPU()
    H, K = wl.H, wl.K
    R = bench.so3_exponential_map(wl.log_rot)
    v = bench.Rotate(R).transform_points(wl.verts[None])
    vv = wl.cams.get_world_to_view_transform().transform_points(v)
    vn = wl.cams.get_projection_transform().transform_points(vv)
    vn = np.concatenate([vn[..., :2].numpy(), vv[..., 2:3].numpy()], -1)[0]
    fv = vn[wl.faces.numpy()]
    p2f = rast_ref.rast_fwd(fv, [0], [fv.shape[0]], H, H, K, wl.blur, False, True, False)[0]
    return (p2f[0] >= 0).sum(-1).astype(np.uint8)


if __name__ == "__main__":
    counts = bench_frame_counts()
    assert counts.shape == (256, 256) and counts.max() <= 50
    np.savez_compressed(os.path.join(OUT, "blend_order_counts.npz"), counts=counts)
    print("wrote blend_order_counts", counts.shape, "valid slots", int(counts.sum()),
          "non-empty pixels", int((counts > 0).sum()))

"""ctypes binding of libpertrender.so (the C ABI declared in include/pertrender.h).

The library is the product: every public op of this package calls into it and
raises if it is missing or the tensors are not on a ROCm device.  There is no
CPU fallback.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# PR_NATIVE_LIB selects a diagnostic build (e.g. the -DPR_RAST_PROFILE variant)
LIB_PATH = os.environ.get("PR_NATIVE_LIB") or os.path.join(_HERE, "libpertrender.so")

PR_NOISE_PHILOX = 0
PR_NOISE_INJECTED = 1
PR_BLEND_RAST = 1
PR_BLEND_COLOR = 2
PR_BLEND_VERTEX = 4
PR_BLEND_RAST_CAUCHY = 8
PR_BLEND_AGG_CAUCHY = 16
PR_BLEND_AGG_UNIFORM = 256
PR_BLEND_WINNERS_IN = 512
PR_BLEND_LIVE_ONLY = 1024
PR_BLEND_PHONG = 2048  # forward: RandomPhongShader's shading on demand (PRBlendFwdArgs.shade)
PR_BLEND_COLOR_SPARSE = 4096  # backward of PR_BLEND_PHONG: colours valid at the slots it reads only
PR_BLEND_RAST_WOVR = 32
PR_BLEND_AGG_WOVR = 64
PR_BLEND_SOFT = 128
PR_GRAD_PREZEROED = 1
PR_BLEND_SYNC_BYTES = 1024
PR_DETERMINISTIC = 2
PR_RAST_VALID_ONLY = 8  # pr_rast_fwd: only the valid prefix of the fragments is written (needs pix_count)
PR_SHADE_LIVE_ONLY = 4  # pr_shade_*: padded slots' colours / d bary left unwritten (needs pix_count)

_vp = C.c_void_p


class PRBlendParams(C.Structure):
    _fields_ = [("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("K", C.c_int32),
                ("Sr", C.c_int32), ("Sa", C.c_int32),
                ("sample_offset_r", C.c_int32), ("sample_offset_a", C.c_int32),
                ("sigma", C.c_float), ("gamma", C.c_float), ("alpha", C.c_float), ("eps", C.c_float),
                ("background", C.c_float * 3), ("noise_mode", C.c_int32),
                ("seed_r", C.c_uint64), ("seed_a", C.c_uint64),
                ("noise_r", _vp), ("noise_a", _vp), ("znear", _vp), ("zfar", _vp),
                ("flags", C.c_int32), ("scalars", _vp * 3), ("seeds", _vp)]


class PRBlendFwdArgs(C.Structure):
    _fields_ = [("p", PRBlendParams), ("pix_to_face", _vp), ("mask", _vp), ("dists", _vp),
                ("prob", _vp), ("zbuf", _vp), ("colors", _vp), ("image", _vp), ("weights", _vp),
                ("winners", _vp), ("rast_cache", _vp), ("bary", _vp), ("faces", _vp), ("vert_colors", _vp),
                ("pix_count", _vp), ("plan", _vp), ("sync", _vp), ("shade", _vp)]


class PRBlendBwdArgs(C.Structure):
    _fields_ = [("p", PRBlendParams), ("pix_to_face", _vp), ("mask", _vp), ("dists", _vp),
                ("prob", _vp), ("zbuf", _vp), ("colors", _vp), ("winners", _vp),
                ("grad_image", _vp), ("grad_weights", _vp), ("grad_dists", _vp), ("grad_prob", _vp),
                ("grad_zbuf", _vp), ("grad_colors", _vp), ("grad_scalars", _vp),
                ("workspace", _vp), ("workspace_bytes", C.c_size_t), ("rast_cache", _vp), ("bary", _vp),
                ("faces", _vp), ("vert_colors", _vp), ("grad_bary", _vp), ("grad_vert_colors", _vp),
                ("pix_count", _vp), ("plan", _vp), ("sync", _vp)]


class PRBlendGeometry(C.Structure):
    _fields_ = [("PB", C.c_int32), ("cap", C.c_int32), ("lds_bytes", C.c_int32), ("lpp", C.c_int32),
                ("multi", C.c_int32), ("NC", C.c_int32), ("nch", C.c_int32), ("b2_regs", C.c_int32),
                ("interleaved", C.c_int32), ("order", C.c_int32)]


# PRBlendGeometry.order / pr_blend_block_order: which pixel block a dispatch index takes
BLEND_ORDER_LINEAR, BLEND_ORDER_CENTRE_OUT, BLEND_ORDER_ROTATED = 0, 1, 2


class PRHeavisideArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("K", C.c_int32),
                ("Sr", C.c_int32), ("sample_offset_r", C.c_int32), ("noise_mode", C.c_int32),
                ("sigma", C.c_float), ("seed_r", C.c_uint64), ("noise_r", _vp), ("dists", _vp),
                ("prob", _vp), ("grad_prob", _vp), ("grad_dists", _vp), ("grad_sigma", _vp),
                ("workspace", _vp), ("workspace_bytes", C.c_size_t), ("sigma_dev", _vp), ("seeds", _vp),
                ("flags", C.c_int32)]


class PRRastArgs(C.Structure):
    _fields_ = [("face_verts", _vp), ("mesh_first_face", _vp), ("mesh_num_faces", _vp),
                ("F", C.c_int64), ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("K", C.c_int32), ("blur_radius", C.c_float), ("perspective_correct", C.c_int32),
                ("clip_barycentric_coords", C.c_int32), ("cull_backfaces", C.c_int32),
                ("pix_to_face", _vp), ("zbuf", _vp), ("bary", _vp), ("dists", _vp),
                ("grad_zbuf", _vp), ("grad_bary", _vp), ("grad_dists", _vp),
                ("grad_face_verts", _vp), ("workspace", _vp), ("workspace_bytes", C.c_size_t),
                ("pix_count", _vp), ("flags", C.c_int32), ("bin_size", C.c_int32),
                ("max_faces_per_bin", C.c_int32), ("blur_radius_dev", _vp)]


class PRInterpArgs(C.Structure):
    _fields_ = [("pix_to_face", _vp), ("bary", _vp), ("face_attr", _vp), ("PK", C.c_int64),
                ("F", C.c_int64), ("D", C.c_int32), ("out", _vp), ("grad_out", _vp),
                ("grad_bary", _vp), ("grad_face_attr", _vp), ("faces", _vp), ("V", C.c_int64)]


class PRProjectArgs(C.Structure):
    _fields_ = [("verts", _vp), ("faces", _vp), ("mesh_first_face", _vp), ("mesh_num_faces", _vp),
                ("world_to_view", _vp), ("proj", _vp), ("V", C.c_int64), ("F", C.c_int64), ("N", C.c_int32),
                ("face_verts", _vp), ("grad_face_verts", _vp), ("grad_verts", _vp), ("flags", C.c_int32),
                ("vert_corner_start", _vp), ("vert_corners", _vp), ("seed_advance", _vp),
                ("seed_advance_n", C.c_int32)]


class PRSO3Args(C.Structure):
    _fields_ = [("N", C.c_int32), ("eps", C.c_float), ("log_rot", _vp), ("R", _vp), ("grad_R", _vp),
                ("grad_log_rot", _vp)]


class PRRotateArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("P", C.c_int32), ("R_batched", C.c_int32), ("points", _vp), ("R", _vp),
                ("out", _vp), ("grad_out", _vp), ("grad_points", _vp), ("grad_R", _vp)]


class PRRgbMseArgs(C.Structure):
    _fields_ = [("P", C.c_int64), ("C", C.c_int32), ("HW", C.c_int32), ("target_batched", C.c_int32),
                ("image", _vp), ("target", _vp), ("loss", _vp), ("partials", _vp), ("grad_loss", _vp),
                ("grad_image", _vp)]


class PRPoseStepArgs(C.Structure):
    _fields_ = [("loss", _vp), ("log_rot", _vp), ("grad", _vp), ("it", _vp), ("losses", _vp), ("gnorms", _vp),
                ("best_loss", _vp), ("best", _vp), ("v", _vp), ("acc", _vp), ("leaf_grad", _vp * 3), ("seed", _vp),
                ("exp_avg", _vp), ("exp_avg_sq", _vp), ("step", _vp), ("lr", _vp),
                ("niter", C.c_int64), ("n", C.c_int32), ("post", C.c_int32), ("adam", C.c_int32)]


PR_TEX_GIVEN = 0
PR_TEX_UV = 1
PR_TEX_VERTEX = 2


class PRShadeArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("K", C.c_int32),
                ("pix_to_face", _vp), ("pix_count", _vp), ("bary", _vp), ("faces", _vp), ("verts", _vp),
                ("flags", C.c_int32), ("workspace", _vp), ("workspace_bytes", C.c_size_t), ("normals", _vp), ("V", C.c_int64), ("F", C.c_int64), ("texture", C.c_int32), ("texels", _vp),
                ("vert_colors", _vp), ("face_uvs", _vp), ("maps", _vp), ("Hm", C.c_int32), ("Wm", C.c_int32),
                ("directional", C.c_int32), ("light", _vp), ("ambient", _vp), ("diffuse_color", _vp),
                ("specular_color", _vp), ("mat_diffuse", _vp), ("mat_specular", _vp), ("shininess", _vp),
                ("camera", _vp), ("colors", _vp), ("grad_colors", _vp), ("grad_bary", _vp), ("grad_verts", _vp),
                ("grad_normals", _vp), ("grad_texels", _vp), ("grad_vert_colors", _vp), ("grad_maps", _vp),
                ("grad_light", _vp), ("grad_camera", _vp)]


class PRNormalsArgs(C.Structure):
    _fields_ = [("verts", _vp), ("faces", _vp), ("V", C.c_int64), ("F", C.c_int64), ("normals", _vp),
                ("raw", _vp), ("grad_normals", _vp), ("grad_raw", _vp), ("grad_verts", _vp),
                ("vert_corner_start", _vp), ("vert_corners", _vp)]


PR_MESH_LAP_UNIFORM = 0
PR_MESH_LAP_COT = 1
PR_MESH_LAP_COTCURV = 2


class PRMeshLossArgs(C.Structure):
    _fields_ = [("verts", _vp), ("faces", _vp), ("V", C.c_int64), ("F", C.c_int64), ("method", C.c_int32),
                ("target_length", C.c_float), ("weight", _vp), ("nbr_start", _vp), ("nbr", _vp),
                ("vert_corner_start", _vp), ("vert_corners", _vp), ("face_cot", _vp), ("gather", _vp),
                ("diag", _vp), ("partials", _vp), ("loss", _vp), ("grad_loss", _vp), ("grad_verts", _vp)]


class PRNormalConsistencyArgs(C.Structure):
    _fields_ = [("verts", _vp), ("faces", _vp), ("V", C.c_int64), ("F", C.c_int64), ("P", C.c_int64),
                ("pair_start", _vp), ("pair_partner", _vp), ("vert_corner_start", _vp), ("vert_corners", _vp),
                ("face_normal", _vp), ("face_sum", _vp), ("face_grad", _vp), ("partials", _vp), ("loss", _vp),
                ("grad_loss", _vp), ("grad_verts", _vp)]


class PRChamferArgs(C.Structure):
    _fields_ = [("x", _vp), ("y", _vp), ("x_len", _vp), ("y_len", _vp), ("N", C.c_int64), ("P", C.c_int64),
                ("Q", C.c_int64), ("dist_x", _vp), ("dist_y", _vp), ("idx_x", _vp), ("idx_y", _vp),
                ("workspace", _vp), ("workspace_bytes", C.c_size_t), ("grad_dist_x", _vp), ("grad_dist_y", _vp),
                ("grad_x", _vp), ("grad_y", _vp)]


class PRSamplePointsArgs(C.Structure):
    _fields_ = [("verts", _vp), ("faces", _vp), ("mesh_first_face", _vp), ("mesh_num_faces", _vp),
                ("N", C.c_int64), ("S", C.c_int64), ("V", C.c_int64), ("F", C.c_int64),
                ("noise_mode", C.c_int32), ("pad0", C.c_int32), ("seed", C.c_uint64), ("seeds", _vp),
                ("uniforms", _vp), ("cdf", _vp), ("samples", _vp), ("normals", _vp), ("face_idx", _vp), ("w", _vp),
                ("workspace", _vp), ("workspace_bytes", C.c_size_t), ("face_sample_start", _vp),
                ("face_samples", _vp), ("vert_corner_start", _vp), ("vert_corners", _vp), ("grad_samples", _vp),
                ("grad_normals", _vp), ("grad_verts", _vp)]


class PRPointMeshArgs(C.Structure):
    _fields_ = [("points", _vp), ("cloud_first", _vp), ("cloud_count", _vp), ("verts", _vp), ("prims", _vp),
                ("mesh_first", _vp), ("mesh_count", _vp), ("N", C.c_int64), ("P", C.c_int64), ("V", C.c_int64),
                ("M", C.c_int64), ("max_points", C.c_int64), ("max_prims", C.c_int64), ("prim", C.c_int32),
                ("pad0", C.c_int32), ("dist_p", _vp), ("idx_p", _vp), ("w_p", _vp), ("dist_m", _vp), ("idx_m", _vp),
                ("w_m", _vp), ("workspace", _vp), ("workspace_bytes", C.c_size_t), ("prim_point_start", _vp),
                ("prim_points", _vp), ("point_prim_start", _vp), ("point_prims", _vp), ("vert_corner_start", _vp),
                ("vert_corners", _vp), ("grad_dist_p", _vp), ("grad_dist_m", _vp), ("grad_points", _vp),
                ("grad_verts", _vp)]


PR_POINTS_MAX_K = 64  # the largest points_per_pixel pr_points_rast_fwd serves
PR_POINTS_ALPHA, PR_POINTS_NORM, PR_POINTS_WEIGHTED = 0, 1, 2


class PRPointsRastArgs(C.Structure):
    _fields_ = [("points", _vp), ("cloud_first", _vp), ("cloud_count", _vp), ("radius", _vp),
                ("radius_scalar", C.c_float), ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("K", C.c_int32),
                ("P", C.c_int64), ("idx", _vp), ("zbuf", _vp), ("dists", _vp), ("point_start", _vp),
                ("point_entries", _vp), ("grad_zbuf", _vp), ("grad_dists", _vp), ("grad_points", _vp)]


class PRPointsCompositeArgs(C.Structure):
    _fields_ = [("idx", _vp), ("alphas", _vp), ("features", _vp), ("N", C.c_int32), ("H", C.c_int32),
                ("W", C.c_int32), ("K", C.c_int32), ("C", C.c_int32), ("mode", C.c_int32), ("P", C.c_int64),
                ("out", _vp), ("workspace", _vp), ("workspace_bytes", C.c_size_t), ("point_start", _vp),
                ("point_entries", _vp), ("grad_out", _vp), ("grad_alphas", _vp), ("grad_features", _vp)]


PR_ICP_STATE = 13  # floats per cloud of a transform: R row-major (9), T (3), s
PR_ICP_BEGIN, PR_ICP_END = 1, 2
PR_ALIGN_RECORD = 18  # doubles of a cloud's moment record (pr_align_solve_host)


class PRAlignArgs(C.Structure):
    _fields_ = [("x", _vp), ("y", _vp), ("weights", _vp), ("x_len", _vp), ("N", C.c_int64), ("P", C.c_int64),
                ("estimate_scale", C.c_int32), ("allow_reflection", C.c_int32), ("eps", C.c_double), ("R", _vp),
                ("T", _vp), ("s", _vp), ("workspace", _vp), ("workspace_bytes", C.c_size_t)]


class PRIcpArgs(C.Structure):
    _fields_ = [("x", _vp), ("y", _vp), ("x_len", _vp), ("y_len", _vp), ("N", C.c_int64), ("P", C.c_int64),
                ("Q", C.c_int64), ("max_iterations", C.c_int32), ("estimate_scale", C.c_int32),
                ("allow_reflection", C.c_int32), ("phase", C.c_int32), ("relative_rmse_thr", C.c_float),
                ("pad0", C.c_int32), ("state", _vp), ("history", _vp), ("rmse", _vp), ("idx", _vp), ("idx_history", _vp),
                ("flags", _vp), ("xt", _vp), ("workspace", _vp), ("workspace_bytes", C.c_size_t)]


# every symbol include/pertrender.h declares, with its argument struct (None = no args)
EXPORTS = {
    "pr_abi_version": (C.c_int, []),
    "pr_last_error": (C.c_char_p, []),
    "pr_ktimer_arm": (C.c_int, [C.c_int32]),
    "pr_blend_plan_size": (C.c_size_t, [C.POINTER(PRBlendParams)]),
    "pr_ktimer_read": (C.c_int, [C.c_int32, C.POINTER(C.c_float), C.c_char_p, C.c_int32]),
    "pr_blend_fwd": (C.c_int, [C.POINTER(PRBlendFwdArgs), _vp]),
    "pr_blend_bwd_workspace_size": (C.c_size_t, [C.POINTER(PRBlendBwdArgs)]),
    "pr_blend_bwd": (C.c_int, [C.POINTER(PRBlendBwdArgs), _vp]),
    "pr_blend_geometry": (C.c_int, [C.POINTER(PRBlendParams), C.c_int, C.POINTER(PRBlendGeometry)]),
    "pr_blend_block_order": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int64,
                                       C.POINTER(C.c_int32)]),
    "pr_heaviside_fwd": (C.c_int, [C.POINTER(PRHeavisideArgs), _vp]),
    "pr_heaviside_bwd_workspace_size": (C.c_size_t, [C.POINTER(PRHeavisideArgs)]),
    "pr_heaviside_bwd": (C.c_int, [C.POINTER(PRHeavisideArgs), _vp]),
    "pr_rast_fwd_workspace_size": (C.c_size_t, [C.POINTER(PRRastArgs)]),
    "pr_rast_fwd": (C.c_int, [C.POINTER(PRRastArgs), _vp]),
    "pr_rast_bwd_workspace_size": (C.c_size_t, [C.POINTER(PRRastArgs)]),
    "pr_rast_bwd": (C.c_int, [C.POINTER(PRRastArgs), _vp]),
    "pr_interp_fwd": (C.c_int, [C.POINTER(PRInterpArgs), _vp]),
    "pr_interp_bwd": (C.c_int, [C.POINTER(PRInterpArgs), _vp]),
    "pr_seed_advance": (C.c_int, [_vp, C.c_int32, _vp]),
    "pr_project_fwd": (C.c_int, [C.POINTER(PRProjectArgs), _vp]),
    "pr_project_bwd": (C.c_int, [C.POINTER(PRProjectArgs), _vp]),
    "pr_project_rast_fwd": (C.c_int, [C.POINTER(PRProjectArgs), C.POINTER(PRRastArgs), _vp]),
    "pr_pose_step": (C.c_int, [C.POINTER(PRPoseStepArgs), _vp]),
    "pr_rgb_mse_workspace": (C.c_size_t, [C.c_int64]),
    "pr_rgb_mse_fwd": (C.c_int, [C.POINTER(PRRgbMseArgs), _vp]),
    "pr_rgb_mse_bwd": (C.c_int, [C.POINTER(PRRgbMseArgs), _vp]),
    "pr_so3_exp_fwd": (C.c_int, [C.POINTER(PRSO3Args), _vp]),
    "pr_so3_exp_bwd": (C.c_int, [C.POINTER(PRSO3Args), _vp]),
    "pr_rotate_fwd": (C.c_int, [C.POINTER(PRRotateArgs), _vp]),
    "pr_rotate_bwd": (C.c_int, [C.POINTER(PRRotateArgs), _vp]),
    "pr_philox": (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, _vp, C.c_int32, _vp]),
    "pr_shade_fwd": (C.c_int, [C.POINTER(PRShadeArgs), _vp]),
    "pr_shade_bwd_workspace_size": (C.c_size_t, [C.POINTER(PRShadeArgs)]),
    "pr_shade_bwd": (C.c_int, [C.POINTER(PRShadeArgs), _vp]),
    "pr_vert_normals_fwd": (C.c_int, [C.POINTER(PRNormalsArgs), _vp]),
    "pr_vert_normals_bwd": (C.c_int, [C.POINTER(PRNormalsArgs), _vp]),
    "pr_mesh_loss_workspace": (C.c_size_t, [C.c_int64]),
    "pr_mesh_laplacian_fwd": (C.c_int, [C.POINTER(PRMeshLossArgs), _vp]),
    "pr_mesh_laplacian_bwd": (C.c_int, [C.POINTER(PRMeshLossArgs), _vp]),
    "pr_mesh_edge_fwd": (C.c_int, [C.POINTER(PRMeshLossArgs), _vp]),
    "pr_mesh_edge_bwd": (C.c_int, [C.POINTER(PRMeshLossArgs), _vp]),
    "pr_mesh_normal_consistency_fwd": (C.c_int, [C.POINTER(PRNormalConsistencyArgs), _vp]),
    "pr_mesh_normal_consistency_bwd": (C.c_int, [C.POINTER(PRNormalConsistencyArgs), _vp]),
    "pr_chamfer_workspace": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int64]),
    "pr_chamfer_fwd": (C.c_int, [C.POINTER(PRChamferArgs), _vp]),
    "pr_chamfer_bwd": (C.c_int, [C.POINTER(PRChamferArgs), _vp]),
    "pr_sample_points_workspace": (C.c_size_t, [C.c_int64]),
    "pr_sample_points_fwd": (C.c_int, [C.POINTER(PRSamplePointsArgs), _vp]),
    "pr_sample_points_bwd": (C.c_int, [C.POINTER(PRSamplePointsArgs), _vp]),
    "pr_point_mesh_workspace": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64]),
    "pr_point_mesh_fwd": (C.c_int, [C.POINTER(PRPointMeshArgs), _vp]),
    "pr_point_mesh_bwd": (C.c_int, [C.POINTER(PRPointMeshArgs), _vp]),
    "pr_points_workspace": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "pr_points_rast_fwd": (C.c_int, [C.POINTER(PRPointsRastArgs), _vp]),
    "pr_points_rast_bwd": (C.c_int, [C.POINTER(PRPointsRastArgs), _vp]),
    "pr_points_composite_fwd": (C.c_int, [C.POINTER(PRPointsCompositeArgs), _vp]),
    "pr_points_composite_bwd": (C.c_int, [C.POINTER(PRPointsCompositeArgs), _vp]),
    "pr_align_solve_host": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32, C.c_double, C.c_int32,
                                      C.c_int32, C.POINTER(C.c_double)]),
    "pr_align_workspace": (C.c_size_t, [C.c_int64, C.c_int64]),
    "pr_align_fwd": (C.c_int, [C.POINTER(PRAlignArgs), _vp]),
    "pr_icp_workspace": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int64]),
    "pr_icp_run": (C.c_int, [C.POINTER(PRIcpArgs), C.c_int32, _vp]),
}
ABI_VERSION = 21

_lib = None


class NativeError(RuntimeError):
    pass


def load(path=LIB_PATH):
    """Load (once) and type the native library.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise NativeError(
            f"libpertrender.so not found at {path}; build it with "
            "`python -m pertrenderer_amd.build_native` (hipcc, gfx950)")
    lib = C.CDLL(path)
    for name, (res, args) in EXPORTS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.pr_abi_version() != ABI_VERSION:
        raise NativeError(f"libpertrender ABI {lib.pr_abi_version()} != {ABI_VERSION}")
    _lib = lib
    return lib


def check(code, what):
    if code != 0:
        msg = load().pr_last_error().decode(errors="replace")
        raise NativeError(f"{what} failed ({code}): {msg}")


def blend_block_order(N, H, W, PB, order):
    """(blocks, taken): the pixel block of every dispatch index of a static blend grid under
    `order` (BLEND_ORDER_*) as an int32 array, and the order in effect (linear where the shape
    cannot take the one asked for).  Host only: pr_blend_block_order."""
    import numpy as np
    blocks = np.empty((N * H * W + PB - 1) // PB if min(N, H, W, PB) > 0 else 1, dtype=np.int32)
    taken = C.c_int32(-1)
    check(load().pr_blend_block_order(N, H, W, PB, order, blocks.ctypes.data, blocks.size, C.byref(taken)),
          "pr_blend_block_order")
    return blocks, taken.value


def ptr(t):
    """Device address of `t` (None for a missing optional buffer).  A plain int: ctypes takes it
    for c_void_p fields and arguments without a wrapper object per pointer."""
    return None if t is None else t.data_ptr()


def dense(t, dtype):
    """`t` detached as a contiguous `dtype` tensor: `t.detach().to(dtype).contiguous()`, without
    the two no-op dispatcher calls when it already is one (the eager step makes ~30 of these)."""
    if t.dtype is dtype and t.is_contiguous():
        return t.detach()
    return t.detach().to(dtype).contiguous()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_of(t):
    """The current torch stream of `t`'s device, as the hipStream_t handle (a plain int: ctypes
    passes it for the c_void_p argument)."""
    if _raw_stream is not None:
        return _raw_stream(t.device.index if t.device.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(t.device).cuda_stream


_get_device = getattr(torch._C, "_cuda_getDevice", None) or torch.cuda.current_device
_FNS = {}


def call(name, what, t, *args):
    """Run C-ABI entry `name`(*args, stream) on `t`'s device: the stream is that device's current
    torch stream, and when `t` lives on another device than the current one (in-process sample
    sharding over devices, multidevice.py) the call runs under a device guard, so every launch,
    memset and error query of the library addresses `t`'s device.  Raises NativeError on a
    non-zero status."""
    fn = _FNS.get(name)
    if fn is None:
        fn = _FNS[name] = getattr(load(), name)
    idx = t.device.index
    if idx is not None and idx != _get_device():
        with torch.cuda.device(idx):
            code = fn(*args, stream_of(t))
    else:
        code = fn(*args, stream_of(t))
    if code != 0:
        check(code, what)


def deterministic():
    """Deterministic-order backward passes (PR_DETERMINISTIC), switched with torch's own
    ``torch.use_deterministic_algorithms(True)``: the sums the fast kernels scatter with float
    atomics (rasterizer, shading) are formed by a stable sort and in-order sums instead, and the
    rasterizer backward then reproduces the CPU oracle's (PyTorch3D's CPU) accumulation bit for
    bit.  Gathers over the mesh topology (projection, vertex normals) are deterministic always."""
    return torch.are_deterministic_algorithms_enabled()


def workspace(nbytes, device):
    """A caller-owned scratch buffer for a native call (the library allocates nothing)."""
    return torch.empty(max(1, int(nbytes)), dtype=torch.uint8, device=device)


def require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise NativeError(
                "pertrenderer_amd native ops run on ROCm devices only (got a "
                f"{t.device} tensor); there is no CPU fallback")

"""ctypes binding of libpmn_hip.so (C ABI declared in include/pmn_hip.h).

The library is built in-tree (``patchmatchnet_amd/csrc/libpmn_hip.so``) by ``build()`` / ``make -C patchmatchnet_amd/csrc``
so that it travels with the source snapshot.  There is no fallback: if the library is missing or a symbol is absent
the product raises, it never silently runs something else.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from typing import Optional

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB_PATH = os.path.join(_CSRC, "libpmn_hip.so")
ABI_VERSION = 25
MLP_FLOATS = 340
MAX_DEPTH = 64
MAX_NEIGHBORS = 17
MAX_FUSE_SRC = 32
TSDF_MAX_VIEWS = 16
TSDF_MARK_SPAN = 8
RASTER_MAX_DIM = 16384
RASTER_MAX_BOX = 64
SPLAT_MAX_RADIUS = 32
ICP_SUMS = 17
ICP_LIMBS = 5
ICP_BLOCK_POINTS = 256
VOXEL_LONG_RUN = 256
VOXEL_MAX_CHANNELS = 8
CROP_MAX_VERTICES = 4096
MESH_PLACE_LONG_RUN = 256
MESH_SIMPLIFY_MAX_FACES = 715827882
MESH_SMOOTH_LONG_ROW = 256
MESH_SMOOTH_MAX_STEPS = 65536
NORMAL_SWEEPS = 6
NORMAL_MAX_VIEWPOINTS = 4096
PLANE_MAX_HYPOTHESES = 4096
PLANE_SUMS = 10
PLANE_LIMBS = 5
PLANE_BLOCK_POINTS = 1024
MLS_QUADRIC_MIN = 6
MLS_PIVOT_MIN = 1e-10

_fp = ctypes.c_void_p  # device float* (passed as integer address)
_ip = ctypes.c_void_p
_hp = ctypes.c_void_p  # host pointer
_i = ctypes.c_int
_f = ctypes.c_float
_s = ctypes.c_void_p   # hipStream_t

# name -> argtypes; mirrors include/pmn_hip.h one to one (tests/test_abi.py checks the header against this table)
SIGNATURES = {
    "pmn_abi_version": [],
    "pmn_error_string": [_i],
    "pmn_nchw_to_nhwc": [_fp, _fp, _i, _i, _i, _i, _s],
    "pmn_feature_weight": [_fp, _fp, _hp, _fp, _i, _i, _i, _i, _i, _i, _fp, _s],
    "pmn_init_hypotheses": [_fp, _fp, _i, _fp, _fp, _i, _f, _fp, _hp, _i, _i, _i, _i, _fp, _fp, _s],
    "pmn_warp_correlate": [_fp, _fp, _fp, _fp, _fp, _i, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _fp, _fp, _ip,
                           _fp, _s],
    "pmn_warp_correlate_views": [_fp, _fp, _fp, _fp, _fp, _i, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _fp, _fp, _ip,
                                 _fp, _s],
    "pmn_aggregate_regress": [_fp, _fp, _fp, _fp, _fp, _hp, _i, _f, _i, _i, _i, _i, _i, _fp, _fp, _s],
    "pmn_confidence": [_fp, _i, _i, _i, _i, _i, _i, _fp, _ip, _s],
    "pmn_conv2d": [_fp, _fp, _fp, _fp, _fp] + [_i] * 14 + [_s],
    "pmn_fpn_tail": [_fp] * 6 + [_i] * 6 + [_s],
    "pmn_fpn_level": [_fp] * 6 + [_i] * 6 + [_s],
    "pmn_conv2d_f16s": [_fp] * 4 + [_i] * 8 + [_s],
    "pmn_offset_heads_f16s": [_fp] * 5 + [_i] * 7 + [_s],
    "pmn_conv2d_f16s_pair": [_fp] * 6 + [_i] * 5 + [_s],
    "pmn_refine_front": [_fp] * 7 + [_i] * 3 + [_s],
    "pmn_refine_tail": [_fp] * 8 + [_i] * 3 + [_s],
    "pmn_refine_fused": [_fp] * 13 + [_i] * 3 + [_s],
    "pmn_conv2d_mfma": [_fp] * 5 + [_i] * 12 + [_s],
    "pmn_deconv3x3s2": [_fp] * 4 + [_i] * 6 + [_s],
    "pmn_stage_projections": [_fp, _fp, _i, _i, _i, _f, _fp, _s],
    "pmn_stem": [_fp] * 6 + [_i] * 3 + [_s],
    "pmn_stem_f16s": [_fp] * 6 + [_i] * 3 + [_s],
    "pmn_stem_f16s_views": [_fp, _i] + [_fp] * 5 + [_i] * 3 + [_s],
    "pmn_stem_conv2_f16s": [_fp] * 8 + [_i] * 3 + [_s],
    "pmn_stem_conv2_f16s_views": [_fp, _i] + [_fp] * 7 + [_i] * 3 + [_s],
    "pmn_differentiable_warping": [_fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _fp, _s],
    "pmn_fuse_view": [_fp, ctypes.c_longlong, _i, _hp, _hp, _i, _fp, _i, _i, _f, _f, _i, _f, _fp, _fp, _fp, _ip, _s],
    "pmn_fuse_view_merged": [_fp, ctypes.c_longlong, _i, _hp, _hp, _i, _fp, _i, _i, _f, _f, _i, _f, _fp, _fp, _fp, _ip, _fp,
                             ctypes.c_longlong, _fp, _s],
    "pmn_pack_points": [_fp, _fp, _fp, _i, _i, _i, _fp, ctypes.c_longlong, _fp, _ip, _fp, _s],
    "pmn_pack_points_normals": [_fp, _fp, _fp, _fp, _i, _fp, _i, _i, _i, _fp, ctypes.c_longlong, _fp, _ip, _fp, _s],
    "pmn_depth_normals": [_fp, _i, _i, _hp, _i, _f, _fp, _s],
    "pmn_normalize_depth": [_fp, _fp, _fp, _i, _i, _fp, _s],
    "pmn_check_f16_domain": [_fp, ctypes.c_longlong, _ip, _s],
    "pmn_plan_create": [ctypes.POINTER(ctypes.c_void_p)],
    "pmn_plan_begin": [_hp],
    "pmn_plan_end": [_hp],
    "pmn_plan_count": [_hp],
    "pmn_plan_kernel_name": [_hp, _i],
    "pmn_plan_launch": [_hp, _s],
    "pmn_plan_destroy": [_hp],
    "pmn_plan_fork": [_hp],
    "pmn_plan_switch": [_hp, _i],
    "pmn_plan_join": [_hp],
    "pmn_plan_entry_branch": [_hp, _i],
    "pmn_plan_launch_part": [_hp, _i, _s],
    "pmn_view_scores": [_fp] * 6 + [_i, _i, ctypes.c_longlong, ctypes.c_longlong] + [ctypes.c_double] * 3 + [_fp, _s],
    "pmn_depth_metrics": [_fp, _fp, _hp, _hp, _hp, _i, _hp, _i, _i, _i, _i, _fp, ctypes.c_longlong, _fp, _s],
    "pmn_nn_distance": [_fp, _ip, ctypes.c_longlong, _hp, ctypes.c_double, _hp, _fp, _ip, ctypes.c_longlong, ctypes.c_double, _fp, _ip,
                        _s],
    "pmn_reduce_round": [_fp, _ip, ctypes.c_longlong, _hp, ctypes.c_double, _hp, ctypes.c_double, _ip, _ip, _ip, _s],
    "pmn_tsdf_integrate": [_fp] * 4 + [_hp, _hp, _f, _f, _fp, ctypes.c_longlong] + [_hp] * 5 + [_i, _s],
    "pmn_mt_count": [_fp, _fp, _hp, _f, _ip, _ip, _s],
    "pmn_mt_emit": [_fp] * 4 + [_hp, _hp, _f, _f] + [_ip] * 4 + [_fp, _ip, _fp, _ip, _s],
    "pmn_tsdf_mark_blocks": [_ip, _ip, _hp, _hp, _f, _f, _fp, ctypes.c_longlong] + [_hp] * 4 + [_i, _s],
    "pmn_tsdf_integrate_blocks": [_fp] * 4 + [_ip, _i, _hp, _hp, _f, _f, _fp, ctypes.c_longlong] + [_hp] * 5 + [_i, _s],
    "pmn_mt_count_blocks": [_fp, _fp, _ip, _ip, _i, _hp, _f, _ip, _ip, _s],
    "pmn_mt_emit_blocks": [_fp] * 4 + [_ip, _ip, _i, _hp, _hp, _f, _f] + [_ip] * 4 + [_fp, _ip, _fp, _ip, _s],
    "pmn_raster_triangles": [_fp, _i, _ip, _i, _hp, _i, _i, ctypes.c_longlong, _ip, _ip, _ip, _s],
    "pmn_splat_points": [_fp, ctypes.c_longlong, _hp, _i, _i, _f, _f, _ip, _ip, _s],
    "pmn_raster_resolve": [_ip, _i, _i, _hp, _fp, ctypes.c_longlong, _ip, ctypes.c_longlong, _ip, _fp, _i, _fp, _ip, _ip, _fp, _s],
    "pmn_icp_accumulate": [_fp, _ip, ctypes.c_longlong, _hp, ctypes.c_double, _hp, _fp, _ip, ctypes.c_longlong, _hp, _hp, ctypes.c_double,
                           _fp, ctypes.c_longlong, _fp, _s],
    "pmn_voxel_mean": [_fp, _fp, _i, ctypes.c_longlong, _ip, ctypes.c_longlong, _fp, _fp, _s],
    "pmn_crop_prism": [_fp, ctypes.c_longlong, _fp, _i, _i, ctypes.c_double, ctypes.c_double, _hp, _ip, _s],
    "pmn_mesh_components": [_ip, _i, _i, _ip, _ip, _s],
    "pmn_mesh_face_samples": [_fp, _i, _ip, _i, ctypes.c_double, ctypes.c_ulonglong, _ip, _ip, _s],
    "pmn_mesh_sample": [_fp, _i, _ip, _i, _ip, _ip, ctypes.c_longlong, ctypes.c_ulonglong, _fp, _ip, _ip, _s],
    "pmn_undistort_image": [_fp, _i, _i, _i, _i, _hp, _hp, _i, _i, _fp, _fp, _fp, _s],
    "pmn_knn_distance": [_fp, _ip, ctypes.c_longlong, _hp, ctypes.c_double, _hp, _fp, _ip, ctypes.c_longlong, _i, ctypes.c_double, _i,
                         _fp, _ip, _fp, _s],
    "pmn_radius_count": [_fp, _ip, ctypes.c_longlong, _hp, ctypes.c_double, _hp, _fp, _ip, ctypes.c_longlong, ctypes.c_double, _i, _ip,
                         _s],
    "pmn_knn_normals": [_fp, _ip, ctypes.c_longlong, _hp, ctypes.c_double, _hp, _fp, _ip, ctypes.c_longlong, _i, ctypes.c_double, _i,
                        _fp, _i, ctypes.c_double, _fp, _fp, _ip, _s],
    "pmn_cloud_core": [_fp, _ip, ctypes.c_longlong, _hp, ctypes.c_double, _hp, ctypes.c_double, ctypes.c_longlong, _ip, _s],
    "pmn_cloud_dbscan": [_fp, _ip, ctypes.c_longlong, _hp, ctypes.c_double, _hp, ctypes.c_double, _ip, _ip, _ip, _ip, _s],
    "pmn_plane_score": [_fp, _fp, _ip, ctypes.c_longlong, _fp, _i, ctypes.c_double, ctypes.c_double, _ip, _s],
    "pmn_plane_inliers": [_fp, _fp, _ip, ctypes.c_longlong, _hp, ctypes.c_double, ctypes.c_double, _hp, _hp, _fp, ctypes.c_longlong, _ip,
                          _fp, _s],
    "pmn_cloud_sdf_blocks": [_fp, _ip, ctypes.c_longlong, _hp, ctypes.c_double, _hp, _fp, _ip, _ip, _i, _hp, _hp, _f, _f, _i,
                             ctypes.c_double, ctypes.c_double, _fp, _fp, _fp, _fp, _s],
    "pmn_knn_mls": [_fp, _ip, ctypes.c_longlong, _hp, ctypes.c_double, _hp, _fp, _ip, ctypes.c_longlong, _i, ctypes.c_double, _i, _i,
                    ctypes.c_double, _fp, _fp, _fp, _ip, _ip, _s],
    "pmn_mesh_distance": [_fp, _ip, ctypes.c_longlong, _hp, ctypes.c_double, _hp, _ip, ctypes.c_double, _fp, _i, _ip, _i, _fp, _ip,
                          ctypes.c_longlong, ctypes.c_double, _fp, _ip, _fp, _ip, _s],
    "pmn_mesh_remap_faces": [_ip, _i, _i, _ip, _i, _ip, _ip, _ip, _ip, _s],
    "pmn_mesh_cluster_place": [_fp, _i, _ip, _i, _ip, _ip, _ip, _i, _fp, _hp, ctypes.c_double, _hp, ctypes.c_double, _fp, _s],
    "pmn_mesh_smooth": [_fp, _i, _ip, _ip, ctypes.c_longlong, _ip, _hp, _i, _fp, _fp, _ip, _s],
    "pmn_mesh_vertex_normals": [_fp, _i, _ip, _i, _ip, _ip, _i, _fp, _ip, _s],
}

# pmn_depth_metrics' row layout and scratch size (the PMN_METRICS_* macros of include/pmn_hip.h; tests/test_validate_io.py checks them)
PLAN_PART_PRE, PLAN_PART_SIDE, PLAN_PART_MAIN, PLAN_PART_POST = 0, 1, 2, 3  # pmn_plan_launch_part (PMN_PLAN_PART_*)

METRICS_MAX_STAGES = 4
METRICS_MAX_ITERS = 5
METRICS_MAX_THRESHOLDS = 8
METRICS_COUNT, METRICS_ABS, METRICS_THR, METRICS_SL1 = 0, 4, 8, 16
METRICS_ROW = 36
METRICS_PIXELS_PER_BLOCK = 4096
METRICS_MAX_BLOCKS = 128


def metrics_scratch(B: int, H: int, W: int) -> int:
    """PMN_METRICS_SCRATCH(B, H, W): float64 elements of pmn_depth_metrics' per-workgroup partial rows."""
    return B * min(METRICS_MAX_BLOCKS, -(-H * W // METRICS_PIXELS_PER_BLOCK)) * METRICS_ROW

def icp_scratch(n: int) -> int:
    """PMN_ICP_SCRATCH(n): 8-byte words of pmn_icp_accumulate's per-workgroup digit sums."""
    return -(-n // ICP_BLOCK_POINTS) * ICP_SUMS * ICP_LIMBS

def plane_scratch(n: int) -> int:
    """PMN_PLANE_SCRATCH(n): 8-byte words of pmn_plane_inliers' per-workgroup digit sums."""
    return -(-n // PLANE_BLOCK_POINTS) * PLANE_SUMS * PLANE_LIMBS


# libpmn_hip_experimental.so only (include/pmn_hip_experimental.h; `make -C patchmatchnet_amd/csrc EXPERIMENTAL=1`)
EXPERIMENTAL_SIGNATURES = {"pmn_set_tuning": [_i, _i],
                           "pmn_conv3x3_wino": [_fp] * 4 + [_i] * 5 + [_s],
                           "pmn_conv5x5s2_wino": [_fp] * 4 + [_i] * 6 + [_s]}
EXPERIMENTAL_LIB_PATH = os.path.join(_CSRC, "libpmn_hip_experimental.so")


def experimental() -> bool:
    """True when this process opted into the research build (PMN_EXPERIMENTAL=1): the product never sets it."""
    return os.environ.get("PMN_EXPERIMENTAL", "") == "1"


_LIB: Optional[ctypes.CDLL] = None


class PmnError(RuntimeError):
    pass


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile the HIP sources for gfx950 (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", _CSRC, "-j4"] + (["-B"] if force else []) + (["EXPERIMENTAL=1"] if experimental() else [])
    if not verbose:
        args.insert(1, "-s")
    subprocess.check_call(args)
    return LIB_PATH


def lib() -> ctypes.CDLL:
    """Loads libpmn_hip.so; raises PmnError when it is missing (the product has no other compute path)."""
    global _LIB
    if _LIB is None:
        path, sigs = LIB_PATH, SIGNATURES
        if experimental():
            path, sigs = EXPERIMENTAL_LIB_PATH, {**SIGNATURES, **EXPERIMENTAL_SIGNATURES}
        if not os.path.isfile(path):
            raise PmnError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           f"or `make -C patchmatchnet_amd/csrc` -- patchmatchnet_amd has no fallback path")
        # PyDLL: the entry points only enqueue kernels (microseconds, never a synchronisation), so they are called WITHOUT
        # releasing the GIL.  With CDLL each of the ~55 launches of a forward is a release/re-acquire, and every one of them is
        # an opening for eval.py's writer threads to take the GIL away from the launch thread (PMN_CTYPES=cdll restores that).
        L = (ctypes.CDLL if os.environ.get("PMN_CTYPES", "") == "cdll" else ctypes.PyDLL)(path)
        for name, argtypes in sigs.items():
            try:
                fn = getattr(L, name)
            except AttributeError as e:
                raise PmnError(f"libpmn_hip.so does not export {name}") from e
            fn.argtypes = argtypes
            fn.restype = ctypes.c_char_p if name in ("pmn_error_string", "pmn_plan_kernel_name") else ctypes.c_int
        if L.pmn_abi_version() != ABI_VERSION:
            raise PmnError(f"libpmn_hip.so ABI {L.pmn_abi_version()} != expected {ABI_VERSION}: rebuild")
        _LIB = L
    return _LIB


def check(code: int, what: str) -> None:
    if code != 0:
        raise PmnError(f"{what} failed: {lib().pmn_error_string(code).decode()} (code {code})")

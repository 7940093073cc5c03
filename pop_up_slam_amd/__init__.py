"""pop_up_slam_amd -- MI355X-native plane-SLAM backend (graph solve + pop-up).

The product is the C-ABI shared library ``libpps.so`` (HIP kernels for gfx950,
``include/pps.h``).  This module is only the thin Python binding used by the
tests and ``bench.py``; a C++ host reaches the same entry points through
``include/pps_isam.hpp``.  There is no CPU fallback: if the library is
missing, importing :class:`Graph` users fail loudly.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PPS_LIB selects another build of the same library (e.g. the diagnostic libpps_nofma.so of `make nofma`)
LIB_PATH = os.environ.get("PPS_LIB") or os.path.join(_HERE, "libpps.so")

PPS_OK, PPS_EINVAL, PPS_ENOTPD, PPS_EHIP, PPS_ENOMEM, PPS_ESTATE = range(6)
JAC_NUMERIC, JAC_ANALYTIC = 0, 1
COST_NONE, COST_HUBER, COST_PSEUDO_HUBER, COST_CAUCHY = range(4)      # enum pps_cost_kind

_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int)


PPS_VERSION = 305      # include/pps.h: the struct layouts mirrored below


class PpsProps(C.Structure):
    _fields_ = [
        ("epsilon2", C.c_double), ("epsilon_abs", C.c_double), ("epsilon_rel", C.c_double),
        ("max_iterations", C.c_int), ("lm_lambda0", C.c_double), ("lm_lambda_factor", C.c_double),
        ("jacobian_mode", C.c_int), ("device", C.c_int), ("verbose", C.c_int),
    ]


class PpsStats(C.Structure):
    _fields_ = [
        ("n_poses", C.c_int), ("n_planes", C.c_int), ("n_factors", C.c_int),
        ("dim_nodes", C.c_int), ("dim_measure", C.c_int),
        ("n_fronts", C.c_int), ("n_levels", C.c_int), ("max_front", C.c_int),
        ("nnz_L", C.c_int64),
        ("lm_iterations", C.c_int), ("lm_trials_accepted", C.c_int), ("lm_trials_rejected", C.c_int),
        ("chi2_initial", C.c_double), ("chi2_final", C.c_double), ("lambda_final", C.c_double),
        ("last_delta_norm", C.c_double),
        ("t_total", C.c_double), ("t_analysis", C.c_double), ("t_upload", C.c_double),
        ("t_linearize", C.c_double), ("t_assemble", C.c_double), ("t_factor", C.c_double),
        ("t_backsolve", C.c_double), ("t_retract_chi2", C.c_double),
        ("n_linearize", C.c_int), ("n_factorize", C.c_int), ("lm_trials_notpd", C.c_int), ("n_launches", C.c_int),
    ]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PpsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"pps error {code}: {msg}")
        self.code = code


_LIB = None

# every symbol include/pps.h declares (checked by tests/test_cabi.py)
def edge_ray(invK, seg2d):
    """Pose3d_Plane3d_Factor2::precompute_edge_ray: fp32 invK * (u,v,1) per end point, as 6 doubles."""
    k = np.ascontiguousarray(invK, dtype=np.float32).reshape(9); sg = np.ascontiguousarray(seg2d, dtype=np.float32).reshape(4)
    out = np.zeros(6)
    rc = lib().pps_edge_ray(k.ctypes.data_as(_fp), sg.ctypes.data_as(_fp), out.ctypes.data_as(_dp))
    if rc != PPS_OK:
        raise PpsError(rc, "pps_edge_ray")
    return out


class PpsEdgeParams(C.Structure):
    """pps_edge_params (include/pps.h): popup_plane.h:82,184-200."""
    _fields_ = [("downsample_contour", C.c_int), ("dilation_distance", C.c_int), ("erosion_distance", C.c_int)] + [
        (k, C.c_double) for k in ("pre_vertical_thre", "pre_minium_len", "pre_contour_close_thre", "interval_overlap_thre",
                                  "post_short_thre", "post_bind_dist_thre", "post_merge_dist_thre", "post_merge_angle_thre",
                                  "post_extend_thre", "pre_boundary_thre", "pre_merge_angle_thre", "pre_merge_dist_thre",
                                  "pre_proj_angle_thre", "pre_proj_cover_thre", "pre_proj_cover_large_thre",
                                  "pre_proj_dist_thre")]


class PpsAssocParams(C.Structure):
    """pps_assoc_params (include/pps.h); defaults = Mapping.h:70-77 via pps_assoc_default_params."""
    _fields_ = [("edge_asso_2ddist", C.c_double), ("edge_asso_planedist", C.c_double), ("edge_asso_proj", C.c_double),
                ("edge_asso_angle", C.c_double), ("assoc_near_frames", C.c_int)]


class PpsMapChunk(C.Structure):
    """pps_map_chunk (include/pps.h): the points of one plane of one frame."""
    _fields_ = [("frame", C.c_int32), ("frame_seq_id", C.c_int32), ("frame_plane", C.c_int32), ("plane_id", C.c_int32),
                ("offset", C.c_int64), ("count", C.c_int64)]


class PpsMapTotals(C.Structure):
    _fields_ = [("capacity", C.c_int64), ("n_points", C.c_int64), ("built_points", C.c_int64),
                ("n_frames", C.c_int32), ("n_chunks", C.c_int32), ("built_chunks", C.c_int32), ("reserved", C.c_int32)]


class PpsMapSelect(C.Structure):
    """pps_map_select (include/pps.h): the thinning of main_3d.cpp:544-562; defaults via pps_map_default_select."""
    _fields_ = [("counter", C.c_int32), ("every_frame", C.c_int32), ("old_age", C.c_int32), ("old_every", C.c_int32),
                ("new_every", C.c_int32), ("age", C.c_int32 * 3), ("min_tracked", C.c_int32 * 3)]


CHUNK_DTYPE = np.dtype([("frame", "<i4"), ("frame_seq_id", "<i4"), ("frame_plane", "<i4"), ("plane_id", "<i4"),
                        ("offset", "<i8"), ("count", "<i8")])


FRAME_DTYPE = np.dtype([("frame", "<i4"), ("frame_seq_id", "<i4"), ("pose_id", "<i4"), ("reserved", "<i4"), ("T_wc", "<f4", (4, 4))])   # pps_map_frame


GRID_NEWEST, GRID_OLDEST = 0, 1                                      # enum pps_grid_rule


class PpsMapGridParams(C.Structure):
    """pps_map_grid_params (include/pps.h); defaults via pps_map_grid_default_params."""
    _fields_ = [("cell", C.c_double), ("rule", C.c_int32), ("min_count", C.c_int32), ("max_cells", C.c_int64)]


class PpsMapGridPlane(C.Structure):
    """pps_map_grid_plane (include/pps.h): one landmark of the grid map."""
    _fields_ = [("plane_id", C.c_int32), ("n_chunks", C.c_int32), ("i0", C.c_int32), ("j0", C.c_int32), ("ni", C.c_int32), ("nj", C.c_int32),
                ("offset", C.c_int64), ("count", C.c_int64), ("n_in", C.c_int64),
                ("n", C.c_double * 3), ("e1", C.c_double * 3), ("e2", C.c_double * 3)]


class PpsMapGridTotals(C.Structure):
    _fields_ = [("n_points", C.c_int64), ("n_cells", C.c_int64), ("n_in", C.c_int64), ("n_dropped", C.c_int64), ("n_passed_through", C.c_int64),
                ("n_planes", C.c_int32), ("launches", C.c_int32), ("cell", C.c_double), ("inv_cell", C.c_double), ("sec", C.c_double * 4)]


GRID_PLANE_DTYPE = np.dtype([("plane_id", "<i4"), ("n_chunks", "<i4"), ("i0", "<i4"), ("j0", "<i4"), ("ni", "<i4"), ("nj", "<i4"),
                             ("offset", "<i8"), ("count", "<i8"), ("n_in", "<i8"), ("n", "<f8", 3), ("e1", "<f8", 3), ("e2", "<f8", 3)])


class PpsMapView(C.Structure):
    """pps_map_view (include/pps.h): the camera of pps_map_render; defaults via pps_map_default_view."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("reach", C.c_int32), ("reserved", C.c_int32),
                ("invK", C.c_float * 9), ("T_wc", C.c_float * 16), ("z_near", C.c_double), ("z_far", C.c_double)]


class PpsMapRenderTotals(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("n_planes", C.c_int32), ("launches", C.c_int32),
                ("n_hit", C.c_int64), ("sec", C.c_double)]


class PpsMapCompareTotals(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("nplanes", C.c_int32), ("n_rows", C.c_int32),
                ("n_both", C.c_int64), ("n_frame_only", C.c_int64), ("n_view_only", C.c_int64), ("n_neither", C.c_int64),
                ("n_bad_id", C.c_int64), ("n_pairs", C.c_int64), ("launches", C.c_int32), ("reserved", C.c_int32),
                ("tol", C.c_double), ("sec", C.c_double)]


MAP_COMPARE_PLANE_DTYPE = np.dtype([("n_valid", "<i8"), ("n_new", "<i8"), ("best_row", "<i4"), ("best_plane_id", "<i4"),
                                    ("best_n", "<i8"), ("best_agree", "<i8")])                                    # pps_map_compare_plane
MAP_COMPARE_ROW_DTYPE = np.dtype([("n_view", "<i8"), ("n_unseen", "<i8")])                                         # pps_map_compare_row
MAP_COMPARE_PAIR_DTYPE = np.dtype([("frame_plane", "<i4"), ("row", "<i4"), ("plane_id", "<i4"), ("reserved", "<i4"),
                                   ("n", "<i8"), ("n_agree", "<i8"), ("sum_q", "<i8"), ("sum_q2", "<i8")])        # pps_map_compare_pair


SYMBOLS = [
    "pps_default_props", "pps_version", "pps_last_error", "pps_graph_create", "pps_graph_destroy",
    "pps_get_props", "pps_set_props", "pps_add_pose", "pps_add_plane", "pps_add_pose_prior",
    "pps_add_odometry", "pps_add_plane_obs", "pps_add_plane_prior", "pps_set_measurement",
    "pps_set_measurements", "pps_remove_factor", "pps_remove_node", "pps_update", "pps_batch_optimize",
    "pps_chi2", "pps_num_nodes", "pps_num_factors", "pps_get_pose", "pps_get_plane", "pps_set_pose",
    "pps_set_plane", "pps_get_poses", "pps_get_planes", "pps_get_stats", "pps_get_trace",
    "pps_set_profiling", "pps_factor_shape", "pps_eval_factor", "pps_analyze", "pps_analysis_dump",
    "pps_bench_sweep", "pps_save_state", "pps_restore_state",
    "pps_popup_planes", "pps_popup_create", "pps_popup_destroy", "pps_popup_last_error", "pps_popup_set_image",
    "pps_popup_run", "pps_popup_run_async", "pps_popup_planes_wait", "pps_popup_wait", "pps_popup_download", "pps_popup_last_kernel_time",
    "pps_frames_set_calibration", "pps_frames_add", "pps_refresh_measurements", "pps_get_measurement",
    "pps_popup_download_segments3d", "pps_assoc_default_params", "pps_landmark_update", "pps_landmark_set_merged",
    "pps_find_closest_planes", "pps_graph_save", "pps_graph_load", "pps_add_plane_obs2", "pps_edge_ray",
    "pps_time_linearize", "pps_debug_front_factor", "pps_debug_front_factor_w", "pps_debug_exmap", "pps_debug_solve", "pps_reproject_points", "pps_popup_set_outputs",
    "pps_edge_default_params", "pps_edges_create", "pps_edges_destroy", "pps_edges_last_error", "pps_edges_select",
    "pps_edges_download_label", "pps_edges_contour", "pps_edges_last_kernel_time", "pps_edges_host_contour",
    "pps_edges_host_select", "pps_popup_fill_depth", "pps_popup_plane_info", "pps_popup_mask_host",
    "pps_multi_create", "pps_multi_destroy", "pps_multi_last_error", "pps_multi_optimize", "pps_multi_rounds", "pps_multi_save_state", "pps_multi_restore_state", "pps_multi_set_profiling", "pps_multi_phase_times", "pps_popup_polygons_simple", "pps_analysis_reuse", "pps_analysis_kept",
    "pps_cov_recover", "pps_cov_marginals", "pps_cov_access", "pps_cov_joint", "pps_cov_last_times",
    "pps_cov_factor", "pps_debug_cov_path_form", "pps_cov_select", "pps_debug_cov_select_form",
    "pps_cov_block", "pps_cov_block_last", "pps_assoc_gate", "pps_assoc_gate_last", "pps_debug_assoc_gate_records",
    "pps_merge_gate", "pps_merge_gate_last", "pps_debug_merge_gate_records",
    "pps_factor_gate", "pps_factor_gate_last", "pps_debug_factor_gate_records",
    "pps_loop_gate", "pps_loop_gate_last", "pps_debug_loop_gate_records",
    "pps_map_default_select", "pps_map_create", "pps_map_destroy", "pps_map_last_error", "pps_map_add_frame", "pps_map_redirect",
    "pps_map_info", "pps_map_chunks", "pps_map_built_chunks", "pps_map_select_host", "pps_map_build", "pps_map_download",
    "pps_map_last_times", "pps_debug_map_add_points",
    "pps_map_grid_default_params", "pps_map_build_grid", "pps_map_grid_planes", "pps_map_grid_info", "pps_map_grid_download",
    "pps_map_grid_frame_host", "pps_map_grid_cell_host",
    "pps_map_default_view", "pps_map_render", "pps_map_render_download", "pps_map_render_info", "pps_map_grid_plane_eq",
    "pps_map_render_ray_host", "pps_map_render_hit_host",
    "pps_map_compare", "pps_debug_map_compare_points", "pps_map_compare_info", "pps_map_compare_rows", "pps_map_compare_pairs",
    "pps_map_compare_point_host",
    "pps_map_set_frame_pose", "pps_map_frames", "pps_map_build_posed", "pps_map_build_grid_posed", "pps_map_frame_motions",
    "pps_map_posed_last", "pps_map_motion_host", "pps_map_move_point_host",
    "pps_set_cost_function", "pps_get_cost_function",
]


def lib():
    """Load libpps.so (no fallback)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or make -C pop_up_slam_amd/csrc).  There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        # the struct mirrors below (PpsProps, PpsStats, ...) are written by hand against ONE layout of include/pps.h: a stale
        # library -- or another one selected through PPS_LIB -- would write past the end of a Python struct, or into a shorter one
        L.pps_version.restype = C.c_int
        if L.pps_version() != PPS_VERSION:
            raise ImportError(f"{LIB_PATH} reports PPS_VERSION {L.pps_version()}, this binding mirrors {PPS_VERSION}: rebuild the library")
        L.pps_last_error.restype = C.c_char_p
        L.pps_last_error.argtypes = [C.c_void_p]
        L.pps_default_props.argtypes = [C.POINTER(PpsProps)]
        L.pps_default_props.restype = None
        L.pps_graph_create.argtypes = [C.POINTER(PpsProps), C.POINTER(C.c_void_p)]
        L.pps_graph_destroy.argtypes = [C.c_void_p]
        L.pps_get_props.argtypes = [C.c_void_p, C.POINTER(PpsProps)]
        L.pps_set_props.argtypes = [C.c_void_p, C.POINTER(PpsProps)]
        L.pps_add_pose.argtypes = [C.c_void_p, _dp, _ip]
        L.pps_add_plane.argtypes = [C.c_void_p, _dp, _ip]
        L.pps_add_pose_prior.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _ip]
        L.pps_add_odometry.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _ip]
        L.pps_add_plane_obs.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _ip]
        L.pps_add_plane_prior.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _ip]
        L.pps_set_measurement.argtypes = [C.c_void_p, C.c_int, _dp]
        L.pps_set_measurements.argtypes = [C.c_void_p, C.c_int, _ip, _dp]
        L.pps_remove_factor.argtypes = [C.c_void_p, C.c_int]
        L.pps_remove_node.argtypes = [C.c_void_p, C.c_int]
        L.pps_update.argtypes = [C.c_void_p]
        L.pps_batch_optimize.argtypes = [C.c_void_p, _ip]
        L.pps_chi2.argtypes = [C.c_void_p, _dp]
        L.pps_num_nodes.argtypes = [C.c_void_p, _ip]
        L.pps_num_factors.argtypes = [C.c_void_p, _ip]
        L.pps_get_pose.argtypes = [C.c_void_p, C.c_int, _dp]
        L.pps_get_plane.argtypes = [C.c_void_p, C.c_int, _dp]
        L.pps_set_pose.argtypes = [C.c_void_p, C.c_int, _dp]
        L.pps_set_plane.argtypes = [C.c_void_p, C.c_int, _dp]
        L.pps_get_poses.argtypes = [C.c_void_p, C.c_int, _ip, _dp]
        L.pps_get_planes.argtypes = [C.c_void_p, C.c_int, _ip, _dp]
        L.pps_save_state.argtypes = [C.c_void_p]
        L.pps_restore_state.argtypes = [C.c_void_p]
        L.pps_get_stats.argtypes = [C.c_void_p, C.POINTER(PpsStats)]
        L.pps_get_trace.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _ip, _ip]
        L.pps_set_profiling.argtypes = [C.c_void_p, C.c_int]
        L.pps_factor_shape.argtypes = [C.c_void_p, C.c_int, _ip, _ip]
        L.pps_eval_factor.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp]
        L.pps_analyze.argtypes = [C.c_void_p]
        L.pps_analysis_dump.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
        L.pps_bench_sweep.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, C.POINTER(C.c_int64),
                                      C.POINTER(C.c_int64)]
        _u8 = C.POINTER(C.c_ubyte)
        L.pps_popup_planes.argtypes = [C.c_int, _fp, C.c_int, _fp, _fp, _fp]
        L.pps_popup_create.argtypes = [C.c_int, C.c_int, C.c_int, _fp, C.POINTER(C.c_void_p)]
        L.pps_popup_destroy.argtypes = [C.c_void_p]
        L.pps_popup_last_error.argtypes = [C.c_void_p]
        L.pps_popup_last_error.restype = C.c_char_p
        L.pps_popup_set_image.argtypes = [C.c_void_p, _u8]
        L.pps_popup_run.argtypes = [C.c_void_p, _fp, C.c_int, _fp, _fp, _ip, C.c_int, C.c_int, C.c_float, C.c_float, _ip]
        L.pps_popup_run_async.argtypes = L.pps_popup_run.argtypes[:-1]
        L.pps_popup_planes_wait.argtypes = [C.c_void_p, _fp]
        L.pps_popup_wait.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.pps_popup_download.argtypes = [C.c_void_p, _fp, C.c_void_p, _fp, C.POINTER(C.c_int32)]
        L.pps_popup_last_kernel_time.argtypes = [C.c_void_p, _dp]
        L.pps_popup_mask_host.argtypes = [_fp, _ip, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]
        L.pps_popup_polygons_simple.argtypes = [_fp, _fp, _fp, C.c_int, C.c_int, _fp, C.c_int, _fp, C.c_int, _ip, _ip]
        L.pps_multi_create.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.pps_multi_destroy.argtypes = [C.c_void_p]
        L.pps_multi_last_error.argtypes = [C.c_void_p]
        L.pps_multi_last_error.restype = C.c_char_p
        L.pps_multi_optimize.argtypes = [C.c_void_p, _ip, _ip]
        L.pps_multi_rounds.argtypes = [C.c_void_p, _ip]
        L.pps_multi_save_state.argtypes = [C.c_void_p]; L.pps_multi_restore_state.argtypes = [C.c_void_p]
        L.pps_multi_set_profiling.argtypes = [C.c_void_p, C.c_int]
        L.pps_multi_phase_times.argtypes = [C.c_void_p, _dp, C.POINTER(C.c_longlong)]
        L.pps_popup_fill_depth.argtypes = [C.c_void_p]
        L.pps_popup_plane_info.argtypes = [C.c_void_p, C.c_float, _ip, C.c_int, _fp, _ip]
        L.pps_frames_set_calibration.argtypes = [C.c_void_p, _fp]
        L.pps_frames_add.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, _ip, _ip]
        L.pps_refresh_measurements.argtypes = [C.c_void_p]
        L.pps_get_measurement.argtypes = [C.c_void_p, C.c_int, _dp]
        L.pps_popup_download_segments3d.argtypes = [C.c_void_p, _fp]
        L.pps_popup_set_outputs.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.pps_assoc_default_params.argtypes = [C.POINTER(PpsAssocParams)]
        L.pps_edge_default_params.argtypes = [C.POINTER(PpsEdgeParams)]; L.pps_edge_default_params.restype = None
        L.pps_edges_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.pps_edges_destroy.argtypes = [C.c_void_p]
        L.pps_edges_last_error.argtypes = [C.c_void_p]; L.pps_edges_last_error.restype = C.c_char_p
        L.pps_edges_select.argtypes = [C.c_void_p, C.c_void_p, C.c_int, _fp, C.c_int, C.POINTER(PpsEdgeParams), _fp, _ip, _fp, _ip, _fp]
        L.pps_edges_download_label.argtypes = [C.c_void_p, C.POINTER(C.c_ubyte), _ip, _ip]
        L.pps_edges_contour.argtypes = [C.c_void_p, _fp, C.c_int, _ip, _ip, _ip]
        L.pps_edges_last_kernel_time.argtypes = [C.c_void_p, _dp]
        L.pps_edges_host_contour.argtypes = [C.POINTER(C.c_int16), C.c_int, C.c_float, _fp, C.c_int, _ip, _ip, _ip]
        L.pps_edges_host_select.argtypes = [_fp, C.c_int, C.c_int, C.c_int, _fp, C.c_int, C.POINTER(PpsEdgeParams), _fp, _ip, _fp, _ip, _fp]
        L.pps_assoc_default_params.restype = None
        L.pps_landmark_update.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _fp, _fp]
        L.pps_landmark_set_merged.argtypes = [C.c_void_p, C.c_int]
        L.pps_add_plane_obs2.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, _ip]
        L.pps_edge_ray.argtypes = [_fp, _fp, _dp]
        L.pps_time_linearize.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.pps_debug_front_factor.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, C.POINTER(C.c_double)]
        if hasattr(L, "pps_debug_front_factor_w"):      # (an older library selected through PPS_LIB for an A/B run does not export it)
            L.pps_debug_front_factor_w.argtypes = L.pps_debug_front_factor.argtypes + [C.c_int]
        L.pps_debug_exmap.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp]
        L.pps_debug_solve.argtypes = [C.c_void_p, C.c_double, C.c_double, _dp, _dp, C.POINTER(C.c_int), C.POINTER(C.c_double)]
        L.pps_reproject_points.argtypes = [C.c_void_p, C.c_int, _ip, _fp, _fp]
        L.pps_graph_save.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.pps_graph_load.argtypes = [C.c_char_p, C.POINTER(PpsProps), C.POINTER(C.c_void_p)]
        L.pps_find_closest_planes.argtypes = [C.c_void_p, _dp, C.c_int, C.c_int, _dp, _ip, _fp, _fp, C.POINTER(PpsAssocParams), _ip, _dp]
        _i64p = C.POINTER(C.c_int64)
        L.pps_cov_recover.argtypes = [C.c_void_p]
        L.pps_cov_marginals.argtypes = [C.c_void_p, C.c_int, _ip, _dp, _i64p]
        L.pps_cov_access.argtypes = [C.c_void_p, C.c_int, _ip, _ip, _dp, _i64p, _ip]
        L.pps_cov_joint.argtypes = [C.c_void_p, C.c_int, _ip, _dp]
        L.pps_cov_last_times.argtypes = [C.c_void_p, _dp]
        L.pps_cov_factor.argtypes = [C.c_void_p]
        L.pps_debug_cov_path_form.argtypes = [C.c_void_p, C.c_int]
        L.pps_cov_select.argtypes = [C.c_void_p]
        L.pps_debug_cov_select_form.argtypes = [C.c_void_p, C.c_int]
        L.pps_cov_block.argtypes = [C.c_void_p, C.c_int, _ip, C.c_int, _ip, _dp]
        L.pps_cov_block_last.argtypes = [C.c_void_p, _dp, _ip]
        L.pps_assoc_gate.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, C.c_int, _ip, _dp, _ip]
        L.pps_assoc_gate_last.argtypes = [C.c_void_p, _dp, _ip]
        L.pps_debug_assoc_gate_records.argtypes = [C.c_void_p, C.c_int64, _dp, C.POINTER(C.c_int64)]
        L.pps_merge_gate.argtypes = [C.c_void_p, C.c_int, _ip, C.c_double, C.c_double, _dp, _ip, C.c_int, _ip, _ip]
        L.pps_merge_gate_last.argtypes = [C.c_void_p, _dp, _ip, _ip]
        L.pps_debug_merge_gate_records.argtypes = [C.c_void_p, C.c_int64, _dp, C.POINTER(C.c_int64)]
        L.pps_loop_gate.argtypes = [C.c_void_p, C.c_int, _ip, _ip, _dp, _dp, C.c_double, _dp, _dp, C.c_int, _ip, _ip]
        L.pps_loop_gate_last.argtypes = [C.c_void_p, _dp, _ip, _ip]
        L.pps_debug_loop_gate_records.argtypes = [C.c_void_p, C.c_int64, _dp, C.POINTER(C.c_int64)]
        L.pps_factor_gate.argtypes = [C.c_void_p, C.c_int, _ip, C.c_double, C.c_double, _dp, _dp, C.c_int, _ip, _ip]
        L.pps_factor_gate_last.argtypes = [C.c_void_p, _dp, _ip, _ip]
        L.pps_debug_factor_gate_records.argtypes = [C.c_void_p, C.c_int64, _dp, C.POINTER(C.c_int64)]
        L.pps_set_cost_function.argtypes = [C.c_void_p, C.c_int, C.c_double]
        L.pps_get_cost_function.argtypes = [C.c_void_p, _ip, _dp]
        _i32p = C.POINTER(C.c_int32)
        L.pps_map_default_select.argtypes = [C.POINTER(PpsMapSelect), C.c_int]; L.pps_map_default_select.restype = None
        L.pps_map_create.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
        L.pps_map_destroy.argtypes = [C.c_void_p]
        L.pps_map_last_error.argtypes = [C.c_void_p]; L.pps_map_last_error.restype = C.c_char_p
        L.pps_map_add_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, _ip, _ip]
        L.pps_debug_map_add_points.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, _ip, _ip]
        L.pps_map_redirect.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.pps_map_info.argtypes = [C.c_void_p, C.POINTER(PpsMapTotals)]
        L.pps_map_chunks.argtypes = [C.c_void_p, C.c_int, C.c_void_p, _ip]
        L.pps_map_built_chunks.argtypes = [C.c_void_p, C.c_int, C.c_void_p, _ip]
        L.pps_map_select_host.argtypes = [C.c_void_p, C.c_int, C.POINTER(PpsMapSelect), _i32p, _ip]
        L.pps_map_build.argtypes = [C.c_void_p, C.POINTER(PpsMapSelect), _i64p, _ip]
        L.pps_map_download.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p]
        L.pps_map_last_times.argtypes = [C.c_void_p, _dp]
        L.pps_map_grid_default_params.argtypes = [C.POINTER(PpsMapGridParams)]; L.pps_map_grid_default_params.restype = None
        L.pps_map_build_grid.argtypes = [C.c_void_p, C.POINTER(PpsMapSelect), C.POINTER(PpsMapGridParams), _i64p, _ip]
        L.pps_map_grid_planes.argtypes = [C.c_void_p, C.c_int, C.c_void_p, _ip]
        L.pps_map_grid_info.argtypes = [C.c_void_p, C.POINTER(PpsMapGridTotals)]
        L.pps_map_grid_download.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.pps_map_grid_frame_host.argtypes = [_dp, _dp, _dp, _dp]
        L.pps_map_grid_cell_host.argtypes = [_dp, C.c_double, _fp, _i64p, _ip]
        L.pps_map_default_view.argtypes = [C.POINTER(PpsMapView), C.c_int, C.c_int, _fp, _fp]; L.pps_map_default_view.restype = None
        L.pps_map_render.argtypes = [C.c_void_p, C.POINTER(PpsMapView), _i64p]
        L.pps_map_render_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.pps_map_render_info.argtypes = [C.c_void_p, C.POINTER(PpsMapRenderTotals)]
        L.pps_map_grid_plane_eq.argtypes = [C.c_void_p, C.c_int, _dp, _ip]
        L.pps_map_render_ray_host.argtypes = [C.POINTER(PpsMapView), C.c_int, C.c_int, _dp, _dp, _dp]
        L.pps_map_render_hit_host.argtypes = [_dp, _dp, _dp, _dp, C.c_double, C.c_double, C.c_double, _dp, _fp, _i64p]
        L.pps_map_compare.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p]
        L.pps_debug_map_compare_points.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_void_p]
        L.pps_map_compare_info.argtypes = [C.c_void_p, C.POINTER(PpsMapCompareTotals)]
        L.pps_map_compare_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p, _ip]
        L.pps_map_compare_pairs.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
        L.pps_map_compare_point_host.argtypes = [_dp, _fp, C.c_double, _dp, _i64p]
        L.pps_map_set_frame_pose.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp]
        L.pps_map_frames.argtypes = [C.c_void_p, C.c_int, C.c_void_p, _ip]
        L.pps_map_build_posed.argtypes = [C.c_void_p, C.POINTER(PpsMapSelect), _i64p, _ip]
        L.pps_map_build_grid_posed.argtypes = [C.c_void_p, C.POINTER(PpsMapSelect), C.POINTER(PpsMapGridParams), _i64p, _ip]
        L.pps_map_frame_motions.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, _ip]
        L.pps_map_posed_last.argtypes = [C.c_void_p, _dp, _ip, _ip]
        L.pps_map_motion_host.argtypes = [_fp, _dp, _dp]
        L.pps_map_move_point_host.argtypes = [_dp, _dp, _fp, _fp]
        _LIB = L
    return _LIB


def _d(a, n=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if n is not None and a.size != n:
        raise ValueError(f"expected {n} doubles, got {a.size}")
    return a, a.ctypes.data_as(_dp)


def default_props(**kw):
    p = PpsProps()
    lib().pps_default_props(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class Graph:
    """Python mirror of the ``isam::Slam`` surface the mapper uses (Slam.h:82-215 of the
    reference): add_node / add_factor / update / batch_optimization / chi2, ids instead of pointers."""

    def __init__(self, **props):
        self.L = lib()
        self.props = default_props(**props)
        h = C.c_void_p()
        rc = self.L.pps_graph_create(C.byref(self.props), C.byref(h))
        if rc != PPS_OK:
            raise PpsError(rc, "pps_graph_create failed")
        self.h = h

    @classmethod
    def load(cls, path, **props):
        """Read a graph written by save() (Slam::save text format) into a new handle."""
        self = cls.__new__(cls)
        self.L = lib()
        self.props = default_props(**props)
        h = C.c_void_p()
        rc = self.L.pps_graph_load(os.fsencode(path), C.byref(self.props), C.byref(h))
        if rc != PPS_OK:
            raise PpsError(rc, f"pps_graph_load({path}) failed")
        self.h = h
        return self

    def save(self, path, precision=0):
        """Slam::save (Slam.cpp:84-89); precision 0 = the reference's 6 significant digits, 17 = lossless."""
        self._ck(self.L.pps_graph_save(self.h, os.fsencode(path), int(precision)))

    def close(self):
        if getattr(self, "h", None):
            self.L.pps_graph_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != PPS_OK:
            raise PpsError(rc, self.L.pps_last_error(self.h).decode())

    def set_props(self, **kw):
        for k, v in kw.items():
            setattr(self.props, k, v)
        self._ck(self.L.pps_set_props(self.h, C.byref(self.props)))

    def get_props(self):
        p = PpsProps(); self._ck(self.L.pps_get_props(self.h, C.byref(p))); return p

    # ---- nodes / factors ----
    def add_pose(self, tq):
        a, p = _d(tq, 7); i = C.c_int(); self._ck(self.L.pps_add_pose(self.h, p, C.byref(i))); return i.value

    def add_plane(self, abcd):
        a, p = _d(abcd, 4); i = C.c_int(); self._ck(self.L.pps_add_plane(self.h, p, C.byref(i))); return i.value

    def add_pose_prior(self, pose, meas6, ut21):
        a, p = _d(meas6, 6); b, q = _d(ut21, 21); i = C.c_int()
        self._ck(self.L.pps_add_pose_prior(self.h, pose, p, q, C.byref(i))); return i.value

    def add_odometry(self, p1, p2, meas6, ut21):
        a, p = _d(meas6, 6); b, q = _d(ut21, 21); i = C.c_int()
        self._ck(self.L.pps_add_odometry(self.h, p1, p2, p, q, C.byref(i))); return i.value

    def add_plane_obs(self, pose, plane, meas4, ut6):
        a, p = _d(meas4, 4); b, q = _d(ut6, 6); i = C.c_int()
        self._ck(self.L.pps_add_plane_obs(self.h, pose, plane, p, q, C.byref(i))); return i.value

    def add_plane_obs2(self, pose, plane, meas4, ray6, ut6):
        """Pose3d_Plane3d_Factor2: the measurement is re-popped from the ground-edge rays at every evaluation."""
        a, p = _d(meas4, 4); r, pr = _d(ray6, 6); b, q = _d(ut6, 6); i = C.c_int()
        self._ck(self.L.pps_add_plane_obs2(self.h, pose, plane, p, pr, q, C.byref(i))); return i.value

    def add_plane_prior(self, plane, meas4, ut6):
        a, p = _d(meas4, 4); b, q = _d(ut6, 6); i = C.c_int()
        self._ck(self.L.pps_add_plane_prior(self.h, plane, p, q, C.byref(i))); return i.value

    def set_measurement(self, fid, meas4):
        a, p = _d(meas4, 4); self._ck(self.L.pps_set_measurement(self.h, fid, p))

    def set_measurements(self, fids, meas):
        f = np.ascontiguousarray(fids, dtype=np.int32); a, p = _d(meas, 4 * len(f))
        self._ck(self.L.pps_set_measurements(self.h, len(f), f.ctypes.data_as(_ip), p))

    def remove_factor(self, fid):
        self._ck(self.L.pps_remove_factor(self.h, fid))

    def remove_node(self, nid):
        self._ck(self.L.pps_remove_node(self.h, nid))

    # ---- solve ----
    def update(self):
        self._ck(self.L.pps_update(self.h))

    def batch_optimize(self):
        it = C.c_int(); self._ck(self.L.pps_batch_optimize(self.h, C.byref(it))); return it.value

    def chi2(self):
        v = C.c_double(); self._ck(self.L.pps_chi2(self.h, C.byref(v))); return v.value

    # ---- robust cost function (Slam::set_cost_function) ----
    def set_cost_function(self, kind, b=1.0):
        """COST_HUBER / COST_PSEUDO_HUBER / COST_CAUCHY with parameter b, or COST_NONE: every whitened residual component becomes
        sign(r) sqrt(rho(r)) in batch_optimize, update, chi2, eval_factor and cov_recover (pps_set_cost_function, include/pps.h)."""
        self._ck(self.L.pps_set_cost_function(self.h, int(kind), float(b)))

    def cost_function(self):
        """(kind, b) as set; (COST_NONE, 1.0) on a handle that has none"""
        k = C.c_int(); b = C.c_double()
        self._ck(self.L.pps_get_cost_function(self.h, C.byref(k), C.byref(b)))
        return k.value, b.value

    # ---- marginal covariances (Slam::covariances() -> isam::Covariances) ----
    def _node_dims(self, ids):
        # 6 for a pose, 3 for a plane; an unknown id raises PPS_EINVAL through the bulk getters' id check
        dims = []
        for i in ids:
            try:
                self.get_pose(int(i)); dims.append(6)
            except PpsError:
                self.get_plane(int(i)); dims.append(3)
        return dims

    def cov_recover(self):
        """Relinearise at the estimate, factor H = J'J (lambda = 0) and recover the selected inverse on the device; valid until the
        estimate, the measurements or the topology change."""
        self._ck(self.L.pps_cov_recover(self.h))

    def cov_factor(self):
        """The factor-only recovery (pps_cov_factor): relinearise at the estimate and factor H = J'J (lambda = 0) in the form the graph is
        solved in, band or dense-front.  All that cov_block and assoc_gate read; cov_marginals / cov_access / cov_joint need cov_recover."""
        self._ck(self.L.pps_cov_factor(self.h))

    def cov_select(self):
        """The selected inverse in whatever form the graph is solved in (pps_cov_select): cov_recover on a band graph, the factor of cov_factor
        and a root -> leaves pass over the dense fronts on a loop-closure graph.  cov_marginals / cov_access / cov_joint answer afterwards,
        cov_block and assoc_gate as after cov_factor."""
        self._ck(self.L.pps_cov_select(self.h))

    def debug_cov_select_form(self, form):
        """diagnostics: 1 = cov_select takes the dense-front pass on a band graph too, 0 = cov_recover there"""
        self._ck(self.L.pps_debug_cov_select_form(self.h, int(form)))

    def debug_cov_path_form(self, form):
        """diagnostics: 0 = cov_block / assoc_gate choose their path-walk kernel by the graph's fronts, 1 = always the kernel for wide fronts"""
        self._ck(self.L.pps_debug_cov_path_form(self.h, int(form)))

    def cov_marginals(self, ids=None):
        """Diagonal blocks of Sigma (6 x 6 per pose, 3 x 3 per plane) as a list of arrays; ids None = every live node in insertion order."""
        if ids is None:
            n = self.num_nodes(); ptr = None
        else:
            i = np.ascontiguousarray(ids, dtype=np.int32); n = len(i); ptr = i.ctypes.data_as(_ip)
        out = np.zeros(36 * max(n, 1)); off = np.zeros(n + 1, dtype=np.int64)
        self._ck(self.L.pps_cov_marginals(self.h, n, ptr, out.ctypes.data_as(_dp), off.ctypes.data_as(C.POINTER(C.c_int64))))
        blocks = []
        for k in range(n):
            d = int(round(np.sqrt(off[k + 1] - off[k])))
            blocks.append(out[off[k]:off[k + 1]].reshape(d, d).copy())
        return blocks

    def cov_access(self, pairs):
        """Cross blocks Sigma(row, col) for (row, col) node-id pairs: a list with one array per pair, None where the pair lies outside
        the pattern of the factor."""
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2); n = len(pr)
        rows = np.ascontiguousarray(pr[:, 0]); cols = np.ascontiguousarray(pr[:, 1])
        out = np.full(36 * max(n, 1), np.nan); off = np.zeros(n + 1, dtype=np.int64); inp = np.zeros(max(n, 1), dtype=np.int32)
        self._ck(self.L.pps_cov_access(self.h, n, rows.ctypes.data_as(_ip), cols.ctypes.data_as(_ip), out.ctypes.data_as(_dp),
                                       off.ctypes.data_as(C.POINTER(C.c_int64)), inp.ctypes.data_as(_ip)))
        res = []
        for k in range(n):
            if not inp[k]:
                res.append(None); continue
            size = int(off[k + 1] - off[k])
            dr = 6 if size == 36 else 3 if size == 9 else self._node_dims([pr[k, 0]])[0]       # (18 values: 6 x 3 or 3 x 6)
            res.append(out[off[k]:off[k + 1]].reshape(dr, size // dr).copy())
        return res

    def cov_joint(self, ids):
        """Joint marginal over a list of distinct nodes (Covariances::marginal(list)), nodes in list order."""
        i = np.ascontiguousarray(ids, dtype=np.int32); n = len(i)
        N = sum(self._node_dims(i))
        out = np.zeros((N, N))
        self._ck(self.L.pps_cov_joint(self.h, n, i.ctypes.data_as(_ip), out.ctypes.data_as(_dp)))
        return out

    def _records(self, fn):
        """the records of a query's last call (pps_debug_*_records): one call for the size, one for the doubles; the flat array"""
        n = C.c_int64(0)
        self._ck(fn(self.h, 0, None, C.byref(n)))
        rec = np.zeros(n.value)
        self._ck(fn(self.h, n.value, rec.ctypes.data_as(_dp), C.byref(n)))
        return rec

    def _last(self, fn, n_ints):
        """the figures of a query's last call (pps_*_last): (device seconds, n_ints ints)"""
        s = C.c_double(); k = [C.c_int() for _ in range(n_ints)]
        self._ck(fn(self.h, C.byref(s), *[C.byref(i) for i in k]))
        return (s.value,) + tuple(i.value for i in k)

    def cov_block(self, rows, cols=None):
        """Sigma(rows, cols) for ANY node ids, inside the pattern of the factor or not: a (sum dim(rows)) x (sum dim(cols)) array, nodes in
        the order given.  cols None: the joint marginal of rows (exactly symmetric).  One root-path solve per distinct node on the factor
        of the last cov_recover or cov_factor."""
        r = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
        c = r if cols is None else np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
        # (sized for poses: the ids are checked by the library, before and not after a size is derived from them)
        out = np.full(36 * max(len(r), 1) * max(len(c), 1), np.nan)
        self._ck(self.L.pps_cov_block(self.h, len(r), r.ctypes.data_as(_ip), len(c), None if cols is None else c.ctypes.data_as(_ip),
                                      out.ctypes.data_as(_dp)))
        nr, nc = sum(self._node_dims(r)), sum(self._node_dims(c))
        return out[:nr * nc].reshape(nr, nc).copy()

    def cov_block_last(self):
        """(device seconds around the two kernels, kernel launches) of the last cov_block"""
        return self._last(self.L.pps_cov_block_last, 1)

    def assoc_gate(self, pose_id, meas4, sqrtinf_ut, plane_ids=None):
        """Mahalanobis gate of plane association (pps_assoc_gate): meas4 (M x 4) plane measurements of pose `pose_id` in its sensor frame,
        sqrtinf_ut (M x 6) their packed upper-triangular sqrt information, plane_ids the L candidate landmarks (None: all live planes in
        insertion order).  Returns (d2, best): d2 (M x L) = r' (I + Jw Sigma Jw')^-1 r of every pairing at the estimate, Sigma from the
        last cov_recover; best (M) = index into plane_ids of the smallest finite d2 per measurement (-1: none).  A pairing passes the
        usual gate when d2 <= 7.815 (chi-square, 3 degrees of freedom, 0.95)."""
        m = np.ascontiguousarray(meas4, dtype=np.float64).reshape(-1, 4)
        w = np.ascontiguousarray(sqrtinf_ut, dtype=np.float64).reshape(-1, 6)
        if len(m) != len(w):
            raise ValueError("assoc_gate: one sqrtinf row per measurement")
        ids = None if plane_ids is None else np.ascontiguousarray(plane_ids, dtype=np.int32).reshape(-1)
        n_pl = self.stats()["n_planes"] if ids is None else len(ids)
        d2 = np.full((len(m), n_pl), np.nan); best = np.full(len(m), -1, dtype=np.int32)
        self._ck(self.L.pps_assoc_gate(self.h, int(pose_id), len(m), m.ctypes.data_as(_dp), w.ctypes.data_as(_dp), n_pl,
                                       None if ids is None else ids.ctypes.data_as(_ip), d2.ctypes.data_as(_dp), best.ctypes.data_as(_ip)))
        return d2, best

    def assoc_gate_records(self):
        """diagnostics: (Jw, r) of every candidate of the last assoc_gate as the kernel evaluated them -- Jw (M*L, 3, 9) over pose 6 | plane 3,
        r (M*L, 3), candidates in row-major (measurement, plane) order; the values pps_eval_factor gives for the same factor"""
        rec = self._records(self.L.pps_debug_assoc_gate_records).reshape(-1, 30)
        return np.concatenate([rec[:, :18].reshape(-1, 3, 6), rec[:, 18:27].reshape(-1, 3, 3)], axis=2), rec[:, 27:].copy()

    def assoc_gate_last(self):
        """(device seconds around the two kernels, kernel launches) of the last assoc_gate"""
        return self._last(self.L.pps_assoc_gate_last, 1)

    def merge_gate(self, plane_ids=None, floor_var=0.0, threshold=7.815, want_d2=True):
        """Mahalanobis merge gate between plane landmarks (pps_merge_gate): are two landmarks the same wall?  plane_ids: the n planes
        (None: all live planes in insertion order).  Returns (d2, best, pairs): d2 (n x n, exactly symmetric, zero diagonal; None with
        want_d2=False -- nothing n x n is then copied from the device) = e' S^-1 e of every pair, e the plane-prior residual of the
        first-listed plane against the other's estimate, S its covariance under their joint marginal from the last recovery plus
        floor_var I (rad^2); best (n) = index into plane_ids of the smallest finite off-diagonal d2 per row (-1: none); pairs (m x 2) =
        all (i, j), i < j, with finite d2 < threshold, ascending.  A pair whose S is not positive definite has d2 = NaN, is never
        best and never in pairs (merge_gate_last counts them).  The Jacobians are central differences whatever jacobian_mode."""
        ids = None if plane_ids is None else np.ascontiguousarray(plane_ids, dtype=np.int32).reshape(-1)
        n = self.stats()["n_planes"] if ids is None else len(ids)
        d2 = np.zeros((n, n)) if want_d2 else None
        best = np.full(max(n, 1), -1, dtype=np.int32)
        cap = min(max(n * (n - 1) // 2, 1), 4096)
        while True:
            pairs = np.zeros((cap, 2), dtype=np.int32); cnt = C.c_int(0)
            self._ck(self.L.pps_merge_gate(self.h, n, None if ids is None else ids.ctypes.data_as(_ip), float(floor_var), float(threshold),
                                           None if d2 is None else d2.ctypes.data_as(_dp), best.ctypes.data_as(_ip), cap, pairs.ctypes.data_as(_ip),
                                           C.byref(cnt)))
            if cnt.value <= cap:
                return d2, best[:n].copy(), pairs[:cnt.value].copy()
            cap = cnt.value                                  # (more pairs than the first guess: once more with room for all)

    def merge_gate_records(self):
        """diagnostics: (J_a, J_b, e) of every pair of the last merge_gate as the kernel evaluated them -- (P, 3, 3), (P, 3, 3), (P, 3), pair
        (i < j) at index i n - i (i + 1) / 2 + (j - i - 1); J_a and e are pps_eval_factor's of a plane prior on a with measurement pi_b,
        J_b the negated Jacobian of the mirrored prior"""
        rec = self._records(self.L.pps_debug_merge_gate_records).reshape(-1, 21)
        return rec[:, :9].reshape(-1, 3, 3).copy(), rec[:, 9:18].reshape(-1, 3, 3).copy(), rec[:, 18:].copy()

    def merge_gate_last(self):
        """(device seconds around the two kernels, kernel launches, pairs whose S was not positive definite) of the last merge_gate"""
        return self._last(self.L.pps_merge_gate_last, 2)

    def loop_gate(self, pose_a, pose_b, meas6, sqrtinf_ut, threshold=12.592, want_S=False):
        """Mahalanobis gate for loop-closure candidates between poses (pps_loop_gate): may this relative-pose measurement be added as a
        loop closure?  Candidate k is the factor add_odometry(pose_a[k], pose_b[k], meas6[k], sqrtinf_ut[k]) would add; meas6 (n x 6),
        sqrtinf_ut (n x 21).  Returns (d2, S, accepted): d2 (n) = r' S^-1 r with S = I + Jw Sigma Jw', r and Jw the candidate's whitened
        residual and Jacobian at the estimate in the handle's jacobian_mode, Sigma the joint marginal of its two poses from the last
        recovery; S (n x 6 x 6, exactly symmetric; None without want_S -- nothing n x 36 is then copied from the device); accepted =
        indices into the list, ascending, of the entries with finite d2 < threshold.  d2 is chi-square with 6 degrees of freedom for a
        correct closure.  A pose may be in any number of candidates; every entry is answered on its own.  A candidate whose S is not
        positive definite has d2 = NaN and is never accepted (loop_gate_last counts them).  Nothing is added to the graph."""
        ia = np.ascontiguousarray(pose_a, dtype=np.int32).reshape(-1); ib = np.ascontiguousarray(pose_b, dtype=np.int32).reshape(-1)
        n = len(ia)
        m = np.ascontiguousarray(meas6, dtype=np.float64).reshape(-1, 6); w = np.ascontiguousarray(sqrtinf_ut, dtype=np.float64).reshape(-1, 21)
        if len(ib) != n or len(m) != n or len(w) != n:
            raise ValueError("loop_gate: pose_a, pose_b, meas6 and sqrtinf_ut must have one entry per candidate")
        d2 = np.full(n, np.nan); S = np.zeros((n, 6, 6)) if want_S else None
        acc = np.zeros(max(n, 1), dtype=np.int32); cnt = C.c_int(0)
        self._ck(self.L.pps_loop_gate(self.h, n, ia.ctypes.data_as(_ip), ib.ctypes.data_as(_ip), m.ctypes.data_as(_dp), w.ctypes.data_as(_dp), float(threshold),
                                      d2.ctypes.data_as(_dp), None if S is None else S.ctypes.data_as(_dp), n, acc.ctypes.data_as(_ip), C.byref(cnt)))
        return d2, S, acc[:cnt.value].copy()

    def loop_gate_records(self):
        """diagnostics: (Jw, r) of every candidate of the last loop_gate as the kernel evaluated them -- (n, 6, 12) and (n, 6), columns of
        pose a then of pose b: what pps_eval_factor gives for the candidate added as an odometry factor"""
        rec = self._records(self.L.pps_debug_loop_gate_records).reshape(-1, 78)
        return rec[:, :72].reshape(-1, 6, 12).copy(), rec[:, 72:].copy()

    def loop_gate_last(self):
        """(device seconds around the two kernels, kernel launches, candidates whose S was not positive definite) of the last loop_gate"""
        return self._last(self.L.pps_loop_gate_last, 2)

    def factor_gate(self, fids=None, thr3=7.815, thr6=12.592):
        """Leave-one-out chi-square test of the graph's own factors (pps_factor_gate): which factor already in the graph is wrong?  fids:
        the n factor ids (None: all live factors in insertion order; an id may repeat).  Returns (d2, lev, flagged): d2 (n) =
        r' (I - P)^-1 r, lev (n) = trace(P), P = J Sigma_ff J' with r, J of the factor at the estimate and Sigma_ff the joint marginal of
        its nodes from the last cov_recover / cov_select; flagged = indices into the list, ascending, of the entries whose finite d2
        exceeds thr3 (3 rows) or thr6 (6 rows).  d2 is chi-square with as many degrees of freedom as the factor has rows when the factor
        is right.  A factor that alone constrains a direction (the gauge prior) has d2 = NaN and is never flagged (factor_gate_last
        counts them)."""
        ids = None if fids is None else np.ascontiguousarray(fids, dtype=np.int32).reshape(-1)
        n = self.num_factors() if ids is None else len(ids)
        d2 = np.full(n, np.nan); lev = np.full(n, np.nan)
        flagged = np.zeros(max(n, 1), dtype=np.int32); cnt = C.c_int(0)
        self._ck(self.L.pps_factor_gate(self.h, n, None if ids is None else ids.ctypes.data_as(_ip), float(thr3), float(thr6), d2.ctypes.data_as(_dp),
                                        lev.ctypes.data_as(_dp), n, flagged.ctypes.data_as(_ip), C.byref(cnt)))
        return d2, lev, flagged[:cnt.value].copy()

    def factor_gate_records(self):
        """diagnostics: J and r of every entry of the last factor_gate as the kernel evaluated them -- (n, 78), one slot per entry holding
        [J m x c row-major, packed | r m] (the rest of the slot unspecified), columns of the factor's first node, then of its second:
        slot[:m * c].reshape(m, c) and slot[m * c:m * c + m] are what pps_eval_factor gives for the factor"""
        return self._records(self.L.pps_debug_factor_gate_records).reshape(-1, 78)

    def factor_gate_last(self):
        """(device seconds around the kernel, kernel launches, untestable entries) of the last factor_gate"""
        return self._last(self.L.pps_factor_gate_last, 2)

    def cov_last_times(self):
        """device seconds of the last cov_recover or cov_select: (whole call, root -> leaves pass alone); of the last cov_factor: (whole call, 0)"""
        s = (C.c_double * 2)(); self._ck(self.L.pps_cov_last_times(self.h, s)); return float(s[0]), float(s[1])

    # ---- state ----
    def num_nodes(self):
        n = C.c_int(); self._ck(self.L.pps_num_nodes(self.h, C.byref(n))); return n.value

    def num_factors(self):
        n = C.c_int(); self._ck(self.L.pps_num_factors(self.h, C.byref(n))); return n.value

    def get_pose(self, nid):
        out = np.zeros(7); self._ck(self.L.pps_get_pose(self.h, nid, out.ctypes.data_as(_dp))); return out

    def get_plane(self, nid):
        out = np.zeros(4); self._ck(self.L.pps_get_plane(self.h, nid, out.ctypes.data_as(_dp))); return out

    def set_pose(self, nid, tq):
        a, p = _d(tq, 7); self._ck(self.L.pps_set_pose(self.h, nid, p))

    def set_plane(self, nid, abcd):
        a, p = _d(abcd, 4); self._ck(self.L.pps_set_plane(self.h, nid, p))

    def get_poses(self, ids=None, n=None):
        if ids is not None:
            i = np.ascontiguousarray(ids, dtype=np.int32); n = len(i); ptr = i.ctypes.data_as(_ip)
        else:
            ptr = None
            if n is None:
                n = self.stats()["n_poses"]
        out = np.zeros((n, 7)); self._ck(self.L.pps_get_poses(self.h, n, ptr, out.ctypes.data_as(_dp))); return out

    def get_planes(self, ids=None, n=None):
        if ids is not None:
            i = np.ascontiguousarray(ids, dtype=np.int32); n = len(i); ptr = i.ctypes.data_as(_ip)
        else:
            ptr = None
            if n is None:
                n = self.stats()["n_planes"]
        out = np.zeros((n, 4)); self._ck(self.L.pps_get_planes(self.h, n, ptr, out.ctypes.data_as(_dp))); return out

    # ---- pop-up feeding the graph (Mapper_mono::update_plane_measurement) ----
    def frames_set_calibration(self, invK):
        k = np.ascontiguousarray(invK, dtype=np.float32).reshape(9)
        self._ck(self.L.pps_frames_set_calibration(self.h, k.ctypes.data_as(_fp)))

    def frames_add(self, pose_id, seg2d, fids):
        seg = np.ascontiguousarray(seg2d, dtype=np.float32).reshape(-1, 4)
        f = np.ascontiguousarray(fids, dtype=np.int32)
        assert len(f) == len(seg) + 1
        out = C.c_int()
        self._ck(self.L.pps_frames_add(self.h, pose_id, len(seg), seg.ctypes.data_as(_fp), f.ctypes.data_as(_ip), C.byref(out)))
        return out.value

    def refresh_measurements(self):
        self._ck(self.L.pps_refresh_measurements(self.h))

    def get_measurement(self, fid):
        out = np.zeros(4); self._ck(self.L.pps_get_measurement(self.h, fid, out.ctypes.data_as(_dp))); return out

    # ---- data association (Mapper_mono::findClosestPlane) ----
    def landmark_update(self, plane_id, frame_plane_indice, frame_seq_id, seg2d=None, seg3d_xy=None):
        s2 = None if seg2d is None else np.ascontiguousarray(seg2d, dtype=np.float32).reshape(4)
        s3 = None if seg3d_xy is None else np.ascontiguousarray(seg3d_xy, dtype=np.float32).reshape(4)
        self._ck(self.L.pps_landmark_update(self.h, int(plane_id), int(frame_plane_indice), int(frame_seq_id),
                                            None if s2 is None else s2.ctypes.data_as(_fp),
                                            None if s3 is None else s3.ctypes.data_as(_fp)))

    def landmark_set_merged(self, plane_id):
        self._ck(self.L.pps_landmark_set_merged(self.h, int(plane_id)))

    def find_closest_planes(self, est_pose, frame_seq_id, planes_local, frame_plane_indice, seg2d, seg3d_xy, **params):
        """One launch for all query planes of a frame.  Returns (plane ids or -1, scores)."""
        prm = PpsAssocParams(); self.L.pps_assoc_default_params(C.byref(prm))
        for k, v in params.items():
            setattr(prm, k, v)
        pl = np.ascontiguousarray(planes_local, dtype=np.float64).reshape(-1, 4); n = len(pl)
        fpi = np.ascontiguousarray(frame_plane_indice, dtype=np.int32).reshape(n)
        s2 = np.ascontiguousarray(seg2d, dtype=np.float32).reshape(n, 4)
        s3 = np.ascontiguousarray(seg3d_xy, dtype=np.float32).reshape(n, 4)
        pose = np.ascontiguousarray(est_pose, dtype=np.float64).reshape(7)
        best = np.full(n, -1, dtype=np.int32); err = np.full(n, -1.0)
        self._ck(self.L.pps_find_closest_planes(self.h, pose.ctypes.data_as(_dp), int(frame_seq_id), n, pl.ctypes.data_as(_dp),
                                                fpi.ctypes.data_as(_ip), s2.ctypes.data_as(_fp), s3.ctypes.data_as(_fp),
                                                C.byref(prm), best.ctypes.data_as(_ip), err.ctypes.data_as(_dp)))
        return best, err

    def time_linearize(self, mode=JAC_NUMERIC, iters=200):
        """seconds per K1 launch, back-to-back launches on the solver's stream between two HIP events"""
        s = C.c_double(); self._ck(self.L.pps_time_linearize(self.h, int(mode), int(iters), C.byref(s))); return s.value

    def reproject_points(self, plane_ids, pts):
        """Mapper_mono::reproj_to_newplane: fp32 points projected onto the current estimate of their landmark planes."""
        ids = np.ascontiguousarray(plane_ids, dtype=np.int32); p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
        assert len(ids) == len(p)
        out = np.zeros_like(p)
        self._ck(self.L.pps_reproject_points(self.h, len(ids), ids.ctypes.data_as(_ip), p.ctypes.data_as(_fp), out.ctypes.data_as(_fp)))
        return out

    def save_state(self):
        self._ck(self.L.pps_save_state(self.h))

    def restore_state(self):
        self._ck(self.L.pps_restore_state(self.h))

    # ---- introspection ----
    def stats(self):
        s = PpsStats(); self._ck(self.L.pps_get_stats(self.h, C.byref(s))); return s.asdict()

    def trace(self):
        n = C.c_int(); self._ck(self.L.pps_get_trace(self.h, 0, None, None, None, C.byref(n)))
        lam = np.zeros(n.value); chi = np.zeros(n.value); acc = np.zeros(n.value, dtype=np.int32)
        self._ck(self.L.pps_get_trace(self.h, n.value, lam.ctypes.data_as(_dp), chi.ctypes.data_as(_dp),
                                      acc.ctypes.data_as(_ip), C.byref(n)))
        return [(float(l), float(c), bool(a)) for l, c, a in zip(lam, chi, acc)]

    def set_profiling(self, level=2):
        self._ck(self.L.pps_set_profiling(self.h, int(level)))

    def eval_factor(self, fid, mode=JAC_NUMERIC):
        m, c = C.c_int(), C.c_int(); self._ck(self.L.pps_factor_shape(self.h, fid, C.byref(m), C.byref(c)))
        J = np.zeros((m.value, c.value)); r = np.zeros(m.value)
        self._ck(self.L.pps_eval_factor(self.h, fid, mode, J.ctypes.data_as(_dp), r.ctypes.data_as(_dp)))
        return J, r

    def debug_solve(self, lam, lam2=-1.0):
        """pps_debug_solve: the step the shipped K3 launches solve for at the current estimate, without applying it.  Returns
        (delta, delta2 | None, form, not_pd): delta indexed by node_voff of analysis_dump(), delta2 the step for lam2 when lam2 >= 0
        (both damping values in one launch, band forms only), form 0 band per stage / 1 band whole tree / 2 dense fronts / 3 level form."""
        n = self.analysis_dump()["n_scalars"] if self.h and float(lam) >= 0 else 0
        dual = float(lam2) >= 0
        delta = np.zeros(max(n, 1)); delta2 = np.zeros(max(n, 1)) if dual else None
        form, bad = C.c_int(-1), C.c_double(0.0)
        self._ck(self.L.pps_debug_solve(self.h, float(lam), float(lam2), delta.ctypes.data_as(_dp),
                                        delta2.ctypes.data_as(_dp) if dual else None, C.byref(form), C.byref(bad)))
        return delta[:n], (delta2[:n] if dual else None), form.value, bad.value

    def analysis_reuse(self):
        """(fronts kept from the previous analysis, fronts in total) of the last analysis"""
        a, b = C.c_int(), C.c_int()
        self._ck(self.L.pps_analysis_reuse(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def analysis_kept(self):
        """leading entries of the index arrays the last analysis took over unchanged: dict fronts / fronts_lists / blocks / segs / contribs / nd_segs"""
        k = (C.c_int * 6)()
        self._ck(self.L.pps_analysis_kept(self.h, k))
        return dict(zip(("fronts", "fronts_lists", "blocks", "segs", "contribs", "nd_segs"), [int(x) for x in k]))

    def analyze(self):
        self._ck(self.L.pps_analyze(self.h))

    def analysis_dump(self):
        need = C.c_int64(); self._ck(self.L.pps_analysis_dump(self.h, 0, None, C.byref(need)))
        buf = np.zeros(need.value, dtype=np.int32)
        self._ck(self.L.pps_analysis_dump(self.h, need.value, buf.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(need)))
        return parse_analysis_dump(buf)

    def bench_sweep(self, mode=JAC_NUMERIC, replicas=1, iters=10):
        sec = (C.c_double * 3)(); npl = C.c_int64(); nod = C.c_int64()
        self._ck(self.L.pps_bench_sweep(self.h, mode, replicas, iters, sec, C.byref(npl), C.byref(nod)))
        return tuple(sec), npl.value, nod.value


_DUMP_SCALARS = ["n_nodes", "n_scalars", "n_fronts", "n_levels", "max_front", "n_blocks", "n_segs", "L_size",
                 "U_size", "H_size", "J_size"]
_DUMP_VECTORS = ["node_pos", "node_voff", "order", "f_p", "f_b", "f_poff", "f_parent", "f_level", "f_Loff", "f_Uoff",
                 "f_bidx_off", "bidx", "f_child_off", "child", "f_cmap_off", "cmap", "level_off", "level_fronts",
                 "f_asm_off", "asm_blk", "asm_lrow", "asm_lcol", "blk_rows", "blk_cols", "blk_size", "blk_nseg",
                 "blk_hoff", "seg_blk", "seg_c0", "seg_cnt", "seg_hoff", "contrib", "node_compact", "factor_joff"]


def parse_analysis_dump(buf):
    out = {}
    k = 0
    for name in _DUMP_SCALARS:
        out[name] = int(buf[k]); k += 1
    def vec():
        nonlocal k
        n = int(buf[k]); k += 1
        v = np.array(buf[k:k + n], dtype=np.int64); k += n
        return v
    for name in _DUMP_VECTORS[:-2]:
        out[name] = vec()
    for name in ("n_stages", "n_groups", "n_glevels"):
        out[name] = int(buf[k]); k += 1
    for name in ("stage_grp_off", "grp_lvl_off", "glvl_front_off", "glvl_fronts", "stage_max_front", "stage_max_width",
                 "f_el_off", "el_src", "el_tgt", "f_ea_off", "ea_tgt", "blk_doff", "blk_dst", "frec", "crec", "srec",
                 "pidx", "obs_dir", "nd_segs"):
        out[name] = vec()
    for name in _DUMP_VECTORS[-2:]:
        out[name] = vec()
    out["factor_poff"] = vec()                       # offset of every factor's product record (round 4)
    out["P_size"] = int(buf[k]); k += 1
    assert k == len(buf), (k, len(buf))
    return out


POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgba", "<u4")])


def popup_planes(seg2d, invK, T_wc, device=0):
    """popup_plane::update_plane_equation_from_seg on the device; returns (n+1) x 4 fp32."""
    seg = np.ascontiguousarray(seg2d, dtype=np.float32).reshape(-1, 4)
    k = np.ascontiguousarray(invK, dtype=np.float32).reshape(9)
    t = np.ascontiguousarray(T_wc, dtype=np.float32).reshape(16)
    out = np.zeros((len(seg) + 1, 4), dtype=np.float32)
    rc = lib().pps_popup_planes(device, seg.ctypes.data_as(_fp), len(seg), k.ctypes.data_as(_fp), t.ctypes.data_as(_fp),
                                out.ctypes.data_as(_fp))
    if rc != PPS_OK:
        raise PpsError(rc, "pps_popup_planes failed")
    return out


class Popup:
    """Per-camera pop-up context (popup_plane object of the reference, image-size bound)."""

    def __init__(self, width, height, invK, device=0):
        self.L = lib()
        self.w, self.h_ = width, height
        k = np.ascontiguousarray(invK, dtype=np.float32).reshape(9)
        h = C.c_void_p()
        rc = self.L.pps_popup_create(device, width, height, k.ctypes.data_as(_fp), C.byref(h))
        if rc != PPS_OK:
            raise PpsError(rc, "pps_popup_create failed")
        self.h = h
        self.n = 0

    def close(self):
        if getattr(self, "h", None):
            self.L.pps_popup_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != PPS_OK:
            raise PpsError(rc, self.L.pps_popup_last_error(self.h).decode())

    def plane_info(self, plane_cam_dist_thre=10.0, actual_plane_indices=None):
        """all_plane_dist_to_cam and the good-plane flags of the last run (n+1 entries, plane 0 = ground)"""
        dist = np.zeros(self.n + 1, dtype=np.float32); good = np.zeros(self.n + 1, dtype=np.int32)
        act = np.ascontiguousarray(actual_plane_indices if actual_plane_indices is not None else [], dtype=np.int32)
        self._ck(self.L.pps_popup_plane_info(self.h, float(plane_cam_dist_thre), act.ctypes.data_as(_ip) if len(act) else None, len(act),
                                             dist.ctypes.data_as(_fp), good.ctypes.data_as(_ip)))
        return dist, good

    def fill_depth(self):
        """after run(step=2): spread the even-pixel depth map over the full frame (get_depth_map_good's resize chain)"""
        self._ck(self.L.pps_popup_fill_depth(self.h))

    def set_image(self, bgr):
        if bgr is None:
            self._ck(self.L.pps_popup_set_image(self.h, None))
            return
        a = np.ascontiguousarray(bgr, dtype=np.uint8)
        assert a.size == self.w * self.h_ * 3
        self._ck(self.L.pps_popup_set_image(self.h, a.ctypes.data_as(C.POINTER(C.c_ubyte))))

    def run_async(self, seg2d, T_wc, polys, step=1, depth_thre=10.0, ceiling_thre=2.5):
        """pps_popup_run_async: the run is enqueued and not waited for; planes_wait() / wait() collect its results"""
        return self.run(seg2d, T_wc, polys, step, depth_thre, ceiling_thre, _async=True)

    def planes_wait(self):
        """the (n + 1) x 4 plane equations of the run in flight, as soon as the kernel has published them"""
        planes = np.zeros((self.n + 1, 4), dtype=np.float32)
        self._ck(self.L.pps_popup_planes_wait(self.h, planes.ctypes.data_as(_fp)))
        return planes

    def wait(self):
        """the end of the run in flight: points of its cloud"""
        nv = C.c_int(); self._ck(self.L.pps_popup_wait(self.h, C.byref(nv))); return nv.value

    def run(self, seg2d, T_wc, polys, step=1, depth_thre=10.0, ceiling_thre=2.5, _async=False):
        """polys: list of (k_i x 2) vertex arrays, one per plane (plane 0 = ground); may be empty arrays."""
        seg = np.ascontiguousarray(seg2d, dtype=np.float32).reshape(-1, 4)
        t = np.ascontiguousarray(T_wc, dtype=np.float32).reshape(16)
        off = np.zeros(len(polys) + 1, dtype=np.int32)
        for i, p in enumerate(polys):
            off[i + 1] = off[i] + len(p)
        flat = np.zeros((max(1, off[-1]), 2), dtype=np.float32)
        for i, p in enumerate(polys):
            if len(p):
                flat[off[i]:off[i + 1]] = np.asarray(p, dtype=np.float32).reshape(-1, 2)
        if _async:
            self._ck(self.L.pps_popup_run_async(self.h, seg.ctypes.data_as(_fp), len(seg), t.ctypes.data_as(_fp),
                                                flat.ctypes.data_as(_fp), off.ctypes.data_as(_ip), len(polys), step, depth_thre, ceiling_thre))
            self.n = len(seg)
            return None
        nv = C.c_int()
        self._ck(self.L.pps_popup_run(self.h, seg.ctypes.data_as(_fp), len(seg), t.ctypes.data_as(_fp),
                                      flat.ctypes.data_as(_fp), off.ctypes.data_as(_ip), len(polys), step,
                                      depth_thre, ceiling_thre, C.byref(nv)))
        self.n = len(seg)
        return nv.value

    def download(self):
        planes = np.zeros((self.n + 1, 4), dtype=np.float32)
        cloud = np.zeros(self.w * self.h_, dtype=POINT_DTYPE)
        depth = np.zeros((self.h_, self.w), dtype=np.float32)
        pid = np.zeros((self.h_, self.w), dtype=np.int32)
        self._ck(self.L.pps_popup_download(self.h, planes.ctypes.data_as(_fp), cloud.ctypes.data_as(C.c_void_p),
                                           depth.ctypes.data_as(_fp), pid.ctypes.data_as(C.POINTER(C.c_int32))))
        return planes, cloud.reshape(self.h_, self.w), depth, pid

    def set_outputs(self, depth=True, plane_id=True):
        """optional per-pixel outputs of run(): the cloud alone is 16 B per pixel, depth and plane id add 4 B each"""
        self._ck(self.L.pps_popup_set_outputs(self.h, int(depth), int(plane_id)))

    def segments3d(self):
        """ground_seg3d_lines_world of the last run: (n,6) world ground end points."""
        out = np.zeros((self.n, 6), dtype=np.float32)
        self._ck(self.L.pps_popup_download_segments3d(self.h, out.ctypes.data_as(_fp)))
        return out

    def last_kernel_time(self):
        s = C.c_double(); self._ck(self.L.pps_popup_last_kernel_time(self.h, C.byref(s))); return s.value


def map_select(counter, **kw):
    """pps_map_select with the reference's gates (main_3d.cpp:544-562) for a map published at frame `counter`; fields by keyword
    (age / min_tracked: sequences of 3)."""
    s = PpsMapSelect(); lib().pps_map_default_select(C.byref(s), int(counter))
    for k, v in kw.items():
        if not hasattr(s, k):
            raise KeyError(k)
        if k in ("age", "min_tracked"):
            v = (C.c_int32 * 3)(*[int(x) for x in v])
        setattr(s, k, v)
    return s


def map_select_host(chunks, sel=None):
    """pps_map_select_host: keep flag per row of a chunk table (CHUNK_DTYPE array); sel None keeps all.  No device needed."""
    c = np.ascontiguousarray(chunks, dtype=CHUNK_DTYPE); n = len(c)
    keep = np.zeros(max(n, 1), dtype=np.int32); nk = C.c_int()
    rc = lib().pps_map_select_host(c.ctypes.data_as(C.c_void_p), n, C.byref(sel) if sel is not None else None,
                                   keep.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nk))
    if rc != PPS_OK:
        raise PpsError(rc, "pps_map_select_host")
    assert nk.value == int(keep[:n].sum())
    return keep[:n].astype(bool)


class Map:
    """pps_map: the per-plane clouds of every frame kept on the device (tracking_frame::partplane_clouds), and the final map built from
    them -- every point projected onto the current estimate of its landmark (main_3d.cpp:535-588)."""

    def __init__(self, graph, capacity_points):
        self.L = lib()
        self.graph = graph                              # keeps the graph alive: the map reads its plane estimates
        h = C.c_void_p()
        rc = self.L.pps_map_create(graph.h, int(capacity_points), C.byref(h))
        if rc != PPS_OK:
            raise PpsError(rc, "pps_map_create failed")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.pps_map_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != PPS_OK:
            raise PpsError(rc, self.L.pps_map_last_error(self.h).decode())

    def add_frame(self, popup, frame_seq_id, plane_node_ids):
        """the last run of `popup` as a frame: one chunk per plane with plane_node_ids[k] >= 0 (-1 skips); returns the points per plane"""
        ids = np.ascontiguousarray(plane_node_ids, dtype=np.int32).reshape(-1)
        cnt = np.zeros(max(len(ids), 1), dtype=np.int32)
        self._ck(self.L.pps_map_add_frame(self.h, popup.h if popup is not None else None, int(frame_seq_id), len(ids),
                                          ids.ctypes.data_as(_ip), cnt.ctypes.data_as(_ip)))
        return cnt[:len(ids)].copy()

    def debug_add_points(self, cloud, plane_id, frame_seq_id, plane_node_ids):
        """pps_debug_map_add_points: add_frame fed host arrays (cloud: POINT_DTYPE, plane_id: int32, one record per pixel in raster
        order -- what Popup.download returns) in place of a pop-up run; returns the points per plane"""
        cloud = np.ascontiguousarray(cloud, dtype=POINT_DTYPE).reshape(-1)
        pid = np.ascontiguousarray(plane_id, dtype=np.int32).reshape(-1)
        if len(cloud) != len(pid):
            raise ValueError("debug_add_points: cloud and plane_id differ in length")
        ids = np.ascontiguousarray(plane_node_ids, dtype=np.int32).reshape(-1)
        cnt = np.zeros(max(len(ids), 1), dtype=np.int32)
        self._ck(self.L.pps_debug_map_add_points(self.h, cloud.ctypes.data_as(C.c_void_p), pid.ctypes.data_as(C.c_void_p), len(cloud),
                                                 int(frame_seq_id), len(ids), ids.ctypes.data_as(_ip), cnt.ctypes.data_as(_ip)))
        return cnt[:len(ids)].copy()

    def redirect(self, from_plane, to_plane):
        self._ck(self.L.pps_map_redirect(self.h, int(from_plane), int(to_plane)))

    def info(self):
        t = PpsMapTotals(); self._ck(self.L.pps_map_info(self.h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in t._fields_ if k != "reserved"}

    def _table(self, fn):
        n = C.c_int(); self._ck(fn(self.h, 0, None, C.byref(n)))
        out = np.zeros(n.value, dtype=CHUNK_DTYPE)
        if n.value:
            self._ck(fn(self.h, n.value, out.ctypes.data_as(C.c_void_p), C.byref(n)))
        return out

    def chunks(self):
        """chunk table of the store (CHUNK_DTYPE rows, insertion order)"""
        return self._table(self.L.pps_map_chunks)

    def built_chunks(self):
        """chunk table of the last build: offsets into the built map"""
        return self._table(self.L.pps_map_built_chunks)

    def build(self, sel=None, posed=False):
        """-> (points, chunks) of the map just built; sel: a PpsMapSelect (map_select) or None = every chunk.  posed: pps_map_build_posed,
        every point first moved with the correction of its frame's pose (set_frame_pose)"""
        npt = C.c_int64(); nch = C.c_int()
        fn = self.L.pps_map_build_posed if posed else self.L.pps_map_build
        self._ck(fn(self.h, C.byref(sel) if sel is not None else None, C.byref(npt), C.byref(nch)))
        return npt.value, nch.value

    def set_frame_pose(self, frame, pose_node_id, T_wc=None):
        """pps_map_set_frame_pose: frame (insertion index) was captured at T_wc (4x4 fp32; None: the T_wc of the pop-up run it was added
        from) and follows the estimate of pose_node_id from now on; pose_node_id = -1 clears the record.  No device needed."""
        T = None
        if T_wc is not None:
            T = np.ascontiguousarray(T_wc, dtype=np.float32).reshape(16)
        self._ck(self.L.pps_map_set_frame_pose(self.h, int(frame), int(pose_node_id), T.ctypes.data_as(_fp) if T is not None else None))

    def frames(self):
        """the frame table (FRAME_DTYPE rows: frame, frame_seq_id, pose_id (-1: no record), T_wc).  No device needed."""
        n = C.c_int(); self._ck(self.L.pps_map_frames(self.h, 0, None, C.byref(n)))
        out = np.zeros(n.value, dtype=FRAME_DTYPE)
        if n.value:
            self._ck(self.L.pps_map_frames(self.h, n.value, out.ctypes.data_as(C.c_void_p), C.byref(n)))
        return out

    def frame_motions(self):
        """motion table of the last posed build / posed grid, read from the device -> (D (n, 12): R_D row-major then t_D, moved (n,) int32),
        one row per frame with a point in the selection, in frame order"""
        n = C.c_int(); self._ck(self.L.pps_map_frame_motions(self.h, 0, None, None, C.byref(n)))
        D = np.zeros((n.value, 12)); moved = np.zeros(n.value, dtype=np.int32)
        if n.value:
            self._ck(self.L.pps_map_frame_motions(self.h, n.value, D.ctypes.data_as(C.c_void_p), moved.ctypes.data_as(C.c_void_p), C.byref(n)))
        return D, moved

    def posed_last(self):
        """of the last posed call: dict(sec=(motion kernel, posed build kernel) device seconds, launches, n_unposed_frames)"""
        s = (C.c_double * 2)(); nl = C.c_int(); nu = C.c_int()
        self._ck(self.L.pps_map_posed_last(self.h, s, C.byref(nl), C.byref(nu)))
        return dict(sec=(float(s[0]), float(s[1])), launches=nl.value, n_unposed_frames=nu.value)

    def download(self, which=0, first=0, n=None):
        """points [first, first + n) of the store (which = 0) or the built map (which = 1) as a POINT_DTYPE array"""
        if n is None:
            i = self.info(); n = (i["n_points"] if which == 0 else i["built_points"]) - first
        out = np.zeros(max(int(n), 0), dtype=POINT_DTYPE)
        self._ck(self.L.pps_map_download(self.h, int(which), int(first), int(n), out.ctypes.data_as(C.c_void_p)))
        return out

    def last_times(self):
        """device seconds: (kernels of the last add_frame, kernel of the last build)"""
        s = (C.c_double * 2)(); self._ck(self.L.pps_map_last_times(self.h, s)); return float(s[0]), float(s[1])

    def build_grid(self, sel=None, cell=0.02, rule=GRID_NEWEST, min_count=1, max_cells=1 << 26, posed=False):
        """pps_map_build_grid: one point per cell (edge `cell` metres) of every landmark plane, of the map build(sel) would write
        (posed: pps_map_build_grid_posed, of the map build(sel, posed=True) would write); -> (cells emitted, rows of the plane table)"""
        prm = PpsMapGridParams(float(cell), int(rule), int(min_count), int(max_cells))
        npt = C.c_int64(); npl = C.c_int()
        fn = self.L.pps_map_build_grid_posed if posed else self.L.pps_map_build_grid
        self._ck(fn(self.h, C.byref(sel) if sel is not None else None, C.byref(prm), C.byref(npt), C.byref(npl)))
        return npt.value, npl.value

    def grid_planes(self):
        """plane table of the last grid (GRID_PLANE_DTYPE rows, ascending plane node id)"""
        n = C.c_int(); self._ck(self.L.pps_map_grid_planes(self.h, 0, None, C.byref(n)))
        out = np.zeros(n.value, dtype=GRID_PLANE_DTYPE)
        if n.value:
            self._ck(self.L.pps_map_grid_planes(self.h, n.value, out.ctypes.data_as(C.c_void_p), C.byref(n)))
        return out

    def grid_info(self):
        """pps_map_grid_totals of the last grid as a dict (sec: 4-tuple); all zeros after a call that failed"""
        t = PpsMapGridTotals(); self._ck(self.L.pps_map_grid_info(self.h, C.byref(t)))
        d = {k: getattr(t, k) for k, _ in t._fields_ if k != "sec"}
        d["sec"] = tuple(float(v) for v in t.sec)
        return d

    def grid_download(self, first=0, n=None):
        """cells [first, first + n) of the last grid -> (points POINT_DTYPE, counts uint32, ij int32 (n, 2), src int64: the winner's index
        in the map build() writes for the same selection)"""
        if n is None:
            n = self.grid_info()["n_cells"] - first
        k = max(int(n), 0)
        pts = np.zeros(k, dtype=POINT_DTYPE); cnt = np.zeros(k, dtype=np.uint32); ij = np.zeros((k, 2), dtype=np.int32); src = np.zeros(k, dtype=np.int64)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        self._ck(self.L.pps_map_grid_download(self.h, int(first), int(n), vp(pts), vp(cnt), vp(ij), vp(src)))
        return pts, cnt, ij, src

    def grid_plane_eq(self):
        """pps_map_grid_plane_eq: (rows of grid_planes, 4) doubles, the plane equations the last grid was built with"""
        n = C.c_int(); self._ck(self.L.pps_map_grid_plane_eq(self.h, 0, None, C.byref(n)))
        out = np.zeros((n.value, 4))
        if n.value:
            self._ck(self.L.pps_map_grid_plane_eq(self.h, n.value, out.ctypes.data_as(_dp), C.byref(n)))
        return out

    def render(self, width, height, invK, T_wc, reach=1, z_near=0.0, z_far=float("inf")):
        """pps_map_render: the last grid seen by a pinhole camera at T_wc (4x4 fp32, sensor -> world) -> dict(cloud POINT_DTYPE, depth
        float32, plane_id int32, cell int64: (height, width) each; n_hit; totals: pps_map_render_totals as a dict)"""
        v = map_view(width, height, invK, T_wc, reach, z_near, z_far)
        n_hit = C.c_int64()
        self._ck(self.L.pps_map_render(self.h, C.byref(v), C.byref(n_hit)))
        out = self.render_download()
        out["n_hit"] = n_hit.value
        out["totals"] = self.render_info()
        return out

    def render_download(self):
        """the four images of the last render as a dict"""
        t = self.render_info()
        shape = (t["height"], t["width"])
        out = dict(cloud=np.zeros(shape, dtype=POINT_DTYPE), depth=np.zeros(shape, dtype=np.float32), plane_id=np.zeros(shape, dtype=np.int32),
                   cell=np.zeros(shape, dtype=np.int64))
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        self._ck(self.L.pps_map_render_download(self.h, vp(out["cloud"]), vp(out["depth"]), vp(out["plane_id"]), vp(out["cell"])))
        return out

    def render_info(self):
        """pps_map_render_totals of the last render as a dict"""
        t = PpsMapRenderTotals(); self._ck(self.L.pps_map_render_info(self.h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in t._fields_}


    def compare(self, popup, nplanes, tol=0.05):
        """pps_map_compare: the last run of `popup` against the last render, pixel for pixel -> MAP_COMPARE_PLANE_DTYPE (nplanes,): per
        frame plane its valid pixels, those without a view, and the landmark most of its pixels agree with (-1: none)"""
        out = np.zeros(max(int(nplanes), 0), dtype=MAP_COMPARE_PLANE_DTYPE)
        self._ck(self.L.pps_map_compare(self.h, popup.h if popup is not None else None, int(nplanes), float(tol), out.ctypes.data_as(C.c_void_p)))
        return out

    def debug_compare(self, cloud, plane_id, nplanes, tol=0.05):
        """pps_debug_map_compare_points: compare fed host arrays (cloud: POINT_DTYPE, plane_id: int32, one record per pixel of the
        rendered view in raster order -- what Popup.download returns) in place of a pop-up run"""
        cloud = np.ascontiguousarray(cloud, dtype=POINT_DTYPE).reshape(-1)
        pid = np.ascontiguousarray(plane_id, dtype=np.int32).reshape(-1)
        if len(cloud) != len(pid):
            raise ValueError("debug_compare: cloud and plane_id differ in length")
        out = np.zeros(max(int(nplanes), 0), dtype=MAP_COMPARE_PLANE_DTYPE)
        self._ck(self.L.pps_debug_map_compare_points(self.h, cloud.ctypes.data_as(C.c_void_p), pid.ctypes.data_as(C.c_void_p), len(cloud),
                                                     int(nplanes), float(tol), out.ctypes.data_as(C.c_void_p)))
        return out

    def compare_info(self):
        """pps_map_compare_totals of the last comparison as a dict"""
        t = PpsMapCompareTotals(); self._ck(self.L.pps_map_compare_info(self.h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in t._fields_ if k != "reserved"}

    def compare_rows(self):
        """per row of the grid's plane table (MAP_COMPARE_ROW_DTYPE): the pixels of the view that show it, and those without a frame point"""
        n = C.c_int(); self._ck(self.L.pps_map_compare_rows(self.h, 0, None, C.byref(n)))
        out = np.zeros(n.value, dtype=MAP_COMPARE_ROW_DTYPE)
        if n.value:
            self._ck(self.L.pps_map_compare_rows(self.h, n.value, out.ctypes.data_as(C.c_void_p), C.byref(n)))
        return out

    def compare_pairs(self, first=0, n=None):
        """entries [first, first + n) of the pair list (MAP_COMPARE_PAIR_DTYPE; by frame plane, then row): n, n_agree, sum_q, sum_q2 of
        every (frame plane, landmark) that shares a pixel"""
        if n is None:
            n = self.compare_info()["n_pairs"] - first
        out = np.zeros(max(int(n), 0), dtype=MAP_COMPARE_PAIR_DTYPE)
        self._ck(self.L.pps_map_compare_pairs(self.h, int(first), int(n), out.ctypes.data_as(C.c_void_p)))
        return out


def map_compare_point_host(abcd, xyz, tol):
    """pps_map_compare_point_host: one fp32 point against one plane -> (agree, e: signed distance in metres, q: e in 1/4096 m, rounded
    and saturated).  No device needed."""
    p = np.ascontiguousarray(abcd, dtype=np.float64).reshape(4); x = np.ascontiguousarray(xyz, dtype=np.float32).reshape(3)
    e = C.c_double(); q = C.c_int64()
    rc = lib().pps_map_compare_point_host(p.ctypes.data_as(_dp), x.ctypes.data_as(_fp), float(tol), C.byref(e), C.byref(q))
    if rc < 0:
        raise PpsError(PPS_EINVAL, "pps_map_compare_point_host")
    return bool(rc), e.value, q.value


def map_view(width, height, invK, T_wc, reach=1, z_near=0.0, z_far=float("inf")):
    """a PpsMapView: pps_map_default_view, then the three optional fields"""
    iK = np.ascontiguousarray(invK, dtype=np.float32).reshape(9); T = np.ascontiguousarray(T_wc, dtype=np.float32).reshape(16)
    v = PpsMapView(); lib().pps_map_default_view(C.byref(v), int(width), int(height), iK.ctypes.data_as(_fp), T.ctypes.data_as(_fp))
    v.reach, v.z_near, v.z_far = int(reach), float(z_near), float(z_far)
    return v


def map_render_ray_host(view, col, row):
    """pps_map_render_ray_host: (o, ds, dw) of pixel (col, row) of a PpsMapView.  No device needed."""
    o, ds, dw = np.zeros(3), np.zeros(3), np.zeros(3)
    rc = lib().pps_map_render_ray_host(C.byref(view), int(col), int(row), o.ctypes.data_as(_dp), ds.ctypes.data_as(_dp), dw.ctypes.data_as(_dp))
    if rc != PPS_OK:
        raise PpsError(rc, "pps_map_render_ray_host")
    return o, ds, dw


def map_render_hit_host(o, ds, dw, abcd, inv_cell, z_near=0.0, z_far=float("inf")):
    """pps_map_render_hit_host: one ray against one landmark plane -> (hit, z, xyz float32 (3,), (i, j)).  No device needed."""
    a = [np.ascontiguousarray(x, dtype=np.float64).reshape(n) for x, n in ((o, 3), (ds, 3), (dw, 3), (abcd, 4))]
    z = C.c_double(); xyz = np.zeros(3, dtype=np.float32); ij = np.zeros(2, dtype=np.int64)
    rc = lib().pps_map_render_hit_host(*[x.ctypes.data_as(_dp) for x in a], float(inv_cell), float(z_near), float(z_far), C.byref(z),
                                       xyz.ctypes.data_as(_fp), ij.ctypes.data_as(C.POINTER(C.c_int64)))
    if rc < 0:
        raise PpsError(PPS_EINVAL, "pps_map_render_hit_host")
    return bool(rc), z.value, xyz, (int(ij[0]), int(ij[1]))


def map_grid_frame_host(abcd):
    """pps_map_grid_frame_host: (n, e1, e2) of a plane's four doubles, the frame its grid cells are counted in.  No device needed."""
    p = np.ascontiguousarray(abcd, dtype=np.float64).reshape(4)
    n, e1, e2 = np.zeros(3), np.zeros(3), np.zeros(3)
    rc = lib().pps_map_grid_frame_host(p.ctypes.data_as(_dp), n.ctypes.data_as(_dp), e1.ctypes.data_as(_dp), e2.ctypes.data_as(_dp))
    if rc != PPS_OK:
        raise PpsError(rc, "pps_map_grid_frame_host")
    return n, e1, e2


def map_grid_cell_host(e, inv_cell, xyz):
    """pps_map_grid_cell_host: (cell index along the axis e, dropped flag) of one fp32 point.  No device needed."""
    ax = np.ascontiguousarray(e, dtype=np.float64).reshape(3); p = np.ascontiguousarray(xyz, dtype=np.float32).reshape(3)
    cell = C.c_int64(); dropped = C.c_int()
    rc = lib().pps_map_grid_cell_host(ax.ctypes.data_as(_dp), float(inv_cell), p.ctypes.data_as(_fp), C.byref(cell), C.byref(dropped))
    if rc != PPS_OK:
        raise PpsError(rc, "pps_map_grid_cell_host")
    return cell.value, bool(dropped.value)


def map_motion_host(T_wc, tq):
    """pps_map_motion_host: the 12 doubles (R_D row-major, t_D) that carry points captured at T_wc (4x4 fp32) to the pose tq (layout of
    Graph.get_pose).  No device needed."""
    T = np.ascontiguousarray(T_wc, dtype=np.float32).reshape(16); p = np.ascontiguousarray(tq, dtype=np.float64).reshape(7)
    D = np.zeros(12)
    rc = lib().pps_map_motion_host(T.ctypes.data_as(_fp), p.ctypes.data_as(_dp), D.ctypes.data_as(_dp))
    if rc != PPS_OK:
        raise PpsError(rc, "pps_map_motion_host")
    return D


def map_move_point_host(D, abcd, xyz):
    """pps_map_move_point_host: one fp32 point of the posed map -- moved by D (None: not moved), projected onto abcd (None: not
    projected), cast to fp32 once.  No device needed."""
    d = np.ascontiguousarray(D, dtype=np.float64).reshape(12) if D is not None else None
    pl = np.ascontiguousarray(abcd, dtype=np.float64).reshape(4) if abcd is not None else None
    p = np.ascontiguousarray(xyz, dtype=np.float32).reshape(3); out = np.zeros(3, dtype=np.float32)
    rc = lib().pps_map_move_point_host(d.ctypes.data_as(_dp) if d is not None else None, pl.ctypes.data_as(_dp) if pl is not None else None,
                                       p.ctypes.data_as(_fp), out.ctypes.data_as(_fp))
    if rc != PPS_OK:
        raise PpsError(rc, "pps_map_move_point_host")
    return out


class Multi:
    """pps_multi: independent graphs solved side by side, every kernel of an LM trial launched once for all of them"""

    def __init__(self, graphs):
        self.L = lib()
        self.graphs = list(graphs)                       # keeps the handles alive
        arr = (C.c_void_p * len(self.graphs))(*[g.h for g in self.graphs])
        self.h = C.c_void_p()
        rc = self.L.pps_multi_create(len(self.graphs), arr, C.byref(self.h))
        if rc != 0:
            # (PPS_ESTATE: a member has a robust cost function set; the refusal's text is on that graph's handle)
            why = [g.L.pps_last_error(g.h).decode() for g in self.graphs if rc == PPS_ESTATE and g.cost_function()[0] != COST_NONE][:1]
            raise PpsError(rc, "pps_multi_create" + "".join(": " + w for w in why))

    def close(self):
        if getattr(self, "h", None):
            self.L.pps_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def optimize(self, check=True):
        """-> (iterations per graph, status per graph)"""
        n = len(self.graphs)
        it = np.zeros(n, dtype=np.int32); st = np.zeros(n, dtype=np.int32)
        rc = self.L.pps_multi_optimize(self.h, it.ctypes.data_as(_ip), st.ctypes.data_as(_ip))
        if rc != 0 and check:
            raise PpsError(rc, (self.L.pps_multi_last_error(self.h) or b"").decode())
        return it, st

    def rounds(self):
        r = C.c_int(); self.L.pps_multi_rounds(self.h, C.byref(r)); return r.value

    def save_state(self):
        rc = self.L.pps_multi_save_state(self.h)
        if rc != 0:
            raise PpsError(rc, (self.L.pps_multi_last_error(self.h) or b"").decode())

    def restore_state(self):
        """every graph back to its snapshot, one launch"""
        rc = self.L.pps_multi_restore_state(self.h)
        if rc != 0:
            raise PpsError(rc, (self.L.pps_multi_last_error(self.h) or b"").decode())

    def set_profiling(self, level=1):
        self.L.pps_multi_set_profiling(self.h, level)

    def phase_times(self):
        """device seconds of the last optimize (profiling on): dict of K1 / K2 / factor / backsolve / trial + relinearisations, solves"""
        t = np.zeros(5); c = (C.c_longlong * 4)()
        self.L.pps_multi_phase_times(self.h, t.ctypes.data_as(_dp), c)
        return {"linearize": t[0], "assemble": t[1], "factor": t[2], "backsolve": t[3], "trial": t[4],
                "n_relinearized": int(c[0]), "n_solves": int(c[1]), "n_chunks": int(c[2]),
                "thread_form": bool(c[3] & 1), "level_form": bool(c[3] & 2)}        # the forms the last solve's chunks took


def _flatten_polys(polys):
    off = np.zeros(len(polys) + 1, dtype=np.int32)
    for i, p in enumerate(polys):
        off[i + 1] = off[i] + len(p)
    flat = np.zeros((max(1, off[-1]), 2), dtype=np.float32)
    for i, p in enumerate(polys):
        if len(p):
            flat[off[i]:off[i + 1]] = np.asarray(p, dtype=np.float32).reshape(-1, 2)
    return flat, off


def popup_polygons_simple(seg2d, K, T_wc, width, height):
    """pps_popup_polygons_simple: list of n + 1 closed wall polygons (k_i x 2 float32; plane 0 = ground: empty)"""
    seg = np.ascontiguousarray(seg2d, dtype=np.float32).reshape(-1, 4); n = len(seg)
    k = np.ascontiguousarray(K, dtype=np.float32).reshape(9)
    ik = np.ascontiguousarray(np.linalg.inv(k.reshape(3, 3)).astype(np.float32)).reshape(9)
    t = np.ascontiguousarray(T_wc, dtype=np.float32).reshape(16)
    verts = np.zeros((8 * max(1, n), 2), dtype=np.float32); off = np.zeros(n + 2, dtype=np.int32); nv = C.c_int()
    rc = lib().pps_popup_polygons_simple(k.ctypes.data_as(_fp), ik.ctypes.data_as(_fp), t.ctypes.data_as(_fp), width, height,
                                         seg.ctypes.data_as(_fp), n, verts.ctypes.data_as(_fp), len(verts), off.ctypes.data_as(_ip), C.byref(nv))
    if rc != 0:
        raise PpsError(rc, "pps_popup_polygons_simple")
    return [verts[off[i]:off[i + 1]].copy() for i in range(n + 1)]


def popup_mask_host(polys, width, height, step=1):
    """pps_popup_mask_host: the kernel's polygon -> pixel-set interval code run on the host (no device needed)"""
    flat, off = _flatten_polys(polys)
    pid = np.zeros((height, width), dtype=np.int32)
    rc = lib().pps_popup_mask_host(flat.ctypes.data_as(_fp), off.ctypes.data_as(_ip), len(polys), width, height, step,
                                   pid.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise PpsError(rc, "pps_popup_mask_host")
    return pid


def edge_params(**kw):
    """pps_edge_params with the reference's defaults, fields overridden by keyword."""
    p = PpsEdgeParams(); lib().pps_edge_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


class Edges:
    """Ground-edge selection context (popup_plane::get_ground_edges after the LSD detector), label-map-size bound."""

    def __init__(self, width, height, device=0):
        self.L = lib()
        self.w, self.h_ = int(width), int(height)
        h = C.c_void_p()
        rc = self.L.pps_edges_create(device, self.w, self.h_, C.byref(h))
        if rc != PPS_OK:
            raise PpsError(rc, "pps_edges_create failed")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.pps_edges_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != PPS_OK:
            raise PpsError(rc, self.L.pps_edges_last_error(self.h).decode())

    def select(self, label_map, lsd_lines, prm=None, device_ptr=None):
        """edge_get_polygons: -> (open segments (n, 4), closed polyline (m, 4), row of each open segment in the closed list).
        label_map: (height, width) u8 array with ground = 255, or pass device_ptr (int) for a map already in HBM."""
        l = np.ascontiguousarray(lsd_lines, dtype=np.float32).reshape(-1, 4); n = l.shape[0]
        cap = 2 * n + 2
        o = np.zeros((cap, 4), dtype=np.float32); cl = np.zeros((cap, 4), dtype=np.float32); idx = np.zeros(cap, dtype=np.float32)
        no = C.c_int(); ncl = C.c_int()
        if device_ptr is None:
            lab = np.ascontiguousarray(label_map, dtype=np.uint8)
            if lab.shape != (self.h_, self.w):
                raise ValueError("label map shape %r != (%d, %d)" % (lab.shape, self.h_, self.w))
            src, on_dev = lab.ctypes.data_as(C.c_void_p), 0
        else:
            src, on_dev = C.c_void_p(int(device_ptr)), 1
        self._ck(self.L.pps_edges_select(self.h, src, on_dev, l.ctypes.data_as(_fp), n, C.byref(prm) if prm is not None else None,
                                         o.ctypes.data_as(_fp), C.byref(no), cl.ctypes.data_as(_fp), C.byref(ncl),
                                         idx.ctypes.data_as(_fp)))
        return o[:no.value].copy(), cl[:ncl.value].copy(), idx[:no.value].copy()

    def label(self):
        """pre-processed label map of the last select (ground = 0)"""
        out = np.zeros(self.w * self.h_, dtype=np.uint8); w = C.c_int(); h = C.c_int()
        self._ck(self.L.pps_edges_download_label(self.h, out.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(w), C.byref(h)))
        return out[:w.value * h.value].reshape(h.value, w.value).copy()

    def contour(self):
        """-> (sub-sampled ground contour (n, 2) as (x, y), contours found, points of the chosen contour)"""
        cap = 4 * (self.w + self.h_) + 64
        xy = np.zeros((cap, 2), dtype=np.float32); n = C.c_int(); nc = C.c_int(); npnt = C.c_int()
        self._ck(self.L.pps_edges_contour(self.h, xy.ctypes.data_as(_fp), cap, C.byref(n), C.byref(nc), C.byref(npnt)))
        return xy[:min(n.value, cap)].copy(), nc.value, npnt.value

    def last_kernel_time(self):
        s = C.c_double(); self._ck(self.L.pps_edges_last_kernel_time(self.h, C.byref(s))); return s.value


def edges_host_contour(cell_segs, scale=1.0):
    """host stage 1 of Edges.select: cell segments (n, 4) int16 -> (sub-sampled contour (m, 2), contours, points)"""
    sg = np.ascontiguousarray(cell_segs, dtype=np.int16).reshape(-1, 4); L = lib()
    cap = 1 + sg.shape[0] // 10 + 64
    xy = np.zeros((cap, 2), dtype=np.float32); n = C.c_int(); nc = C.c_int(); npnt = C.c_int()
    rc = L.pps_edges_host_contour(sg.ctypes.data_as(C.POINTER(C.c_int16)), sg.shape[0], float(scale), xy.ctypes.data_as(_fp), cap,
                                  C.byref(n), C.byref(nc), C.byref(npnt))
    if rc != PPS_OK:
        raise PpsError(rc, "pps_edges_host_contour")
    return xy[:min(n.value, cap)].copy(), nc.value, npnt.value


def edges_host_select(contour_xy, width, height, lsd_lines, prm=None):
    """host stage 2 of Edges.select: contour + LSD lines -> (open, closed, open_in_closed)"""
    c = np.ascontiguousarray(contour_xy, dtype=np.float32).reshape(-1, 2)
    l = np.ascontiguousarray(lsd_lines, dtype=np.float32).reshape(-1, 4); n = l.shape[0]; L = lib()
    cap = 2 * n + 2
    o = np.zeros((cap, 4), dtype=np.float32); cl = np.zeros((cap, 4), dtype=np.float32); idx = np.zeros(cap, dtype=np.float32)
    no = C.c_int(); ncl = C.c_int()
    rc = L.pps_edges_host_select(c.ctypes.data_as(_fp), c.shape[0], int(width), int(height), l.ctypes.data_as(_fp), n,
                                 C.byref(prm) if prm is not None else None, o.ctypes.data_as(_fp), C.byref(no),
                                 cl.ctypes.data_as(_fp), C.byref(ncl), idx.ctypes.data_as(_fp))
    if rc != PPS_OK:
        raise PpsError(rc, "pps_edges_host_select")
    return o[:no.value].copy(), cl[:ncl.value].copy(), idx[:no.value].copy()


def debug_front_factor(A_tri, p, b, tiles=0, strip=False, width=8):
    """One frontal matrix (packed lower triangle, p pivot rows + b boundary rows + the rhs row) through the register-tile
    elimination of the band kernels: returns (L (p+b+1) x p, U packed triangle of b+1 rows, not_pd).  width: pivot columns per panel
    step, 8 (the level and wide kernels) or 4 (the register-only band kernels: at most 64 rows, no strip)."""
    L_ = lib()
    fa = p + b + 1
    a = np.ascontiguousarray(A_tri, dtype=np.float64)
    assert a.size == fa * (fa + 1) // 2
    Lp = np.zeros((fa, p)); U = np.zeros((b + 1) * (b + 2) // 2 + (b + 1) * (b + 1)); bad = C.c_double()
    args = (int(tiles), int(bool(strip)), int(p), int(b), a.ctypes.data_as(_dp), Lp.ctypes.data_as(_dp), U.ctypes.data_as(_dp), C.byref(bad))
    if width == 8:
        rc = L_.pps_debug_front_factor(*args)
    else:
        rc = L_.pps_debug_front_factor_w(*args, int(width))
    if rc != 0:
        raise PpsError(rc, "pps_debug_front_factor(tiles=%d, strip=%d, p=%d, b=%d, width=%d)" % (tiles, strip, p, b, width))
    return Lp, U[:(b + 1) * (b + 2) // 2], bad.value


def debug_exmap(kind, x, delta):
    """pps_debug_exmap: the device's pose_exmap (kind 0; x n x 7, delta n x 6) / plane_exmap (kind 1; x n x 4, delta n x 3)."""
    L_ = lib()
    x = np.ascontiguousarray(np.atleast_2d(np.asarray(x, dtype=np.float64)))
    d = np.ascontiguousarray(np.atleast_2d(np.asarray(delta, dtype=np.float64)))
    assert x.shape == (len(d), 7 if kind == 0 else 4) and d.shape[1] == (6 if kind == 0 else 3)
    out = np.empty_like(x)
    rc = L_.pps_debug_exmap(int(kind), len(x), x.ctypes.data_as(_dp), d.ctypes.data_as(_dp), out.ctypes.data_as(_dp))
    if rc != PPS_OK:
        raise PpsError(rc, "pps_debug_exmap(kind=%d, n=%d)" % (kind, len(x)))
    return out

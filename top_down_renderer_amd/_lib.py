"""ctypes binding of libtdr_hip.so (include/tdr.h).  There is no CPU fallback: if the library is missing or no HIP
device is present, the product path raises."""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("TDR_LIB_PATH") or os.path.join(_PKG, "libtdr_hip.so")   # override: tuning variants only

TDR_ST_FIELDS = 7
TDR_MAX_CLASSES = 15
TDR_SVG_NO_KEY = 0xFFFFFFFF


class FilterParamsC(C.Structure):
    _fields_ = [
        ("pos_cov", C.c_float), ("theta_cov", C.c_float), ("regularization", C.c_float),
        ("init_pos_px_x", C.c_float), ("init_pos_px_y", C.c_float), ("init_pos_px_cov", C.c_float),
        ("init_pos_m_x", C.c_float), ("init_pos_m_y", C.c_float),
        ("init_pos_deg_theta", C.c_float), ("init_pos_deg_cov", C.c_float),
        ("force_on_map", C.c_int32),
        ("fixed_scale", C.c_float), ("scale_log_min", C.c_float), ("scale_log_max", C.c_float),
        ("num_classes", C.c_int32),
        ("class_weights", C.c_float * 16),
    ]


class MapDescC(C.Structure):
    _fields_ = [("rec", C.c_void_p), ("ncls", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32),
                ("rec_floats", C.c_int32), ("resolution", C.c_float),
                ("cwords", C.c_int32), ("dict_n", C.c_int32), ("crec", C.c_void_p), ("dict", C.c_void_p),
                ("rec16", C.c_void_p)]


class BatchInputC(C.Structure):
    """tdr_batch_input: one filter's share of a tdr_batch_step."""
    _fields_ = [("scan_imgs", C.c_void_p), ("renderer", C.c_void_p), ("res", C.c_float), ("tx", C.c_float),
                ("ty", C.c_float), ("omega", C.c_float), ("n_target", C.c_int64)]


class GmmJobC(C.Structure):
    """tdr_gmm_job (include/tdr.h): one device fit."""
    _fields_ = [("samples", C.c_void_p), ("m", C.c_int32), ("k", C.c_int32), ("max_iter", C.c_int32), ("pad", C.c_int32),
                ("out", C.c_void_p), ("workspace", C.c_void_p)]


class GmmPickJobC(C.Structure):
    """tdr_gmm_pick_job (include/tdr.h): one filter's cluster-count decision over its candidate fits."""
    _fields_ = [("cand", C.c_void_p * 3), ("k", C.c_int32), ("pad", C.c_int32), ("record", C.c_void_p)]


GMM_MAX_K = 32
GMM_RECORD_DOUBLES = 2 + 8 * GMM_MAX_K


class BatchCloudC(C.Structure):
    """tdr_batch_cloud: one renderer's cloud in a tdr_batch_render_polar."""
    _fields_ = [("pts", C.c_void_p), ("stride", C.c_int), ("ioff", C.c_int), ("n", C.c_int64), ("res", C.c_float)]


class VizJobC(C.Structure):
    """tdr_viz_job: one picture of a batched particle-picture launch."""
    _fields_ = [("st", C.c_void_p), ("cap", C.c_int64), ("n", C.c_int64), ("H", C.c_int32), ("W", C.c_int32),
                ("planes", C.c_void_p), ("background", C.c_void_p), ("segs", C.c_void_p), ("best", C.c_void_p),
                ("n_segs", C.c_int32), ("pad", C.c_int32), ("out_h", C.c_int32), ("out_w", C.c_int32), ("out", C.c_void_p)]


class VizRequestC(C.Structure):
    """tdr_viz_request: one filter's share of a tdr_batch_visualize."""
    _fields_ = [("extra_arrows", C.c_void_p), ("m", C.c_int32), ("pad", C.c_int32), ("out_bgr_host", C.c_void_p),
                ("capacity", C.c_int64), ("out_h", C.c_int32), ("out_w", C.c_int32)]


class ScanPictureJobC(C.Structure):
    """tdr_scan_picture_job: one picture of a batched scan / analog picture launch."""
    _fields_ = [("imgs", C.c_void_p), ("ncls", C.c_int32), ("pad", C.c_int32), ("npix", C.c_int64), ("out_bgr", C.c_void_p)]


class LabelPictureJobC(C.Structure):
    """tdr_label_picture_job: one picture of a batched label picture launch."""
    _fields_ = [("labels", C.c_void_p), ("npix", C.c_int64), ("out_bgr", C.c_void_p)]


class FuseJobC(C.Structure):
    """tdr_fuse_job: one scan of a batched vote launch."""
    _fields_ = [("scan", C.c_void_p), ("rows", C.c_int32), ("cols", C.c_int32), ("polar", C.c_int32), ("pad", C.c_int32),
                ("cx", C.c_float), ("cy", C.c_float), ("theta", C.c_float), ("scale", C.c_float), ("res", C.c_float),
                ("pad2", C.c_float)]


class KldParamsC(C.Structure):
    """tdr_kld_params (include/tdr.h, "KLD-sampling count")."""
    _fields_ = [("bin_xy_px", C.c_float), ("theta_bins", C.c_int32), ("scale_bits", C.c_int32), ("epsilon", C.c_double),
                ("z", C.c_double), ("n_min", C.c_int64)]


class KldJobC(C.Structure):
    """tdr_kld_job: one filter of a batched count."""
    _fields_ = [("st", C.c_void_p), ("cap", C.c_int64), ("n", C.c_int64), ("table", C.c_void_p), ("table_slots", C.c_int64),
                ("out2", C.c_void_p)]


KLD_NO_KEY = 0xFFFFFFFFFFFFFFFF


class InjectJobC(C.Structure):
    """tdr_inject_job (include/tdr.h, "recovery injection"): one filter of a batched injection."""
    _fields_ = [("st", C.c_void_p), ("cap", C.c_int64), ("n", C.c_int64), ("slot_begin", C.c_int64), ("road", C.c_void_p),
                ("n_road", C.c_int64), ("cols", C.c_int32), ("resolution", C.c_float), ("seed", C.c_uint64),
                ("draw", C.c_uint64), ("threshold24", C.c_uint32), ("heading_mode", C.c_int32), ("injected", C.c_void_p)]


class RecoveryStateC(C.Structure):
    """tdr_recovery_state: the slow and the fast average of the updates' mean raw weight."""
    _fields_ = [("w_slow", C.c_double), ("w_fast", C.c_double)]


class RecoveryParamsC(C.Structure):
    """tdr_recovery_params."""
    _fields_ = [("alpha_slow", C.c_double), ("alpha_fast", C.c_double), ("p_max", C.c_double), ("heading_mode", C.c_int32),
                ("seed", C.c_uint64)]


class GridSpecC(C.Structure):
    """tdr_grid_spec (include/tdr.h, "pose-grid search"): the lattice, its headings and the candidates' scale."""
    _fields_ = [("c0", C.c_int32), ("r0", C.c_int32), ("step", C.c_int32), ("nx", C.c_int32), ("ny", C.c_int32),
                ("road_only", C.c_int32), ("heading_mode", C.c_int32), ("n_headings", C.c_int32), ("theta0", C.c_float),
                ("dtheta", C.c_float), ("scale", C.c_float)]


class GridPeakC(C.Structure):
    """tdr_grid_peak: lattice point, map cell r * cols + c, weight and heading of one peak."""
    _fields_ = [("g", C.c_int32), ("cell", C.c_uint32), ("w", C.c_float), ("theta", C.c_float)]


GRID_PEAK_DTYPE = np.dtype([("g", "<i4"), ("cell", "<u4"), ("w", "<f4"), ("theta", "<f4")])   # tdr_grid_peak


def grid_spec(c0, r0, step, nx, ny, road_only=1, heading_mode=0, n_headings=1, theta0=0.0, dtheta=0.0, scale=1.0):
    """A GridSpecC from plain numbers (include/tdr.h, "pose-grid search")."""
    return GridSpecC(int(c0), int(r0), int(step), int(nx), int(ny), int(road_only), int(heading_mode), int(n_headings),
                     float(theta0), float(dtheta), float(scale))


class PoseStatsC(C.Structure):
    """tdr_pose_stats: one filter's result of a tdr_batch_pose."""
    _fields_ = [("mean", C.c_float * 4), ("cov", C.c_float * 16), ("scale", C.c_float), ("n", C.c_int64)]


# name -> (restype, argtypes); every symbol include/tdr.h declares
_vp, _i, _i64, _f, _u64, _u32 = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_uint64, C.c_uint32
SIGNATURES = {
    "tdr_last_error": (C.c_char_p, []),
    "tdr_version": (_i, []),
    "tdr_device_count": (_i, []),
    "tdr_rec_floats": (_i, [_i]),
    "tdr_map_rec_floats_total": (C.c_size_t, [_i, _i, _i]),
    "tdr_map_rec16_bytes": (C.c_size_t, [_i, _i, _i]),
    "tdr_config_rec16_min_particles": (_i64, [_i64]),
    "tdr_config_compact": (_i, [_i]),
    "tdr_config_shift_uniform": (_i, [_i]),
    "tdr_config_shift_uniform_span": (C.c_float, [C.c_float]),
    "tdr_config_ray_split": (_i, [_i]),
    "tdr_config_cart_skip": (_i, [_i]),
    "tdr_config_init_mfma": (_i, [_i]),
    "tdr_config_uw_waves": (_i, [_i]),
    "tdr_config_prefix_small": (_i, [_i]),
    "tdr_shift_uniform_launches": (_i64, []),
    "tdr_cmap_words": (_i, [_i]),
    "tdr_cmap_words_total": (C.c_size_t, [_i, _i, _i]),
    "tdr_cmap_tile_words": (C.c_size_t, [_i, _i, _i]),
    "tdr_cmap_plane_offset_words": (C.c_size_t, [_i, _i, _i]),
    "tdr_cmap_plane_words": (C.c_size_t, [_i, _i, _i]),
    "tdr_cmap_cmask_words": (C.c_size_t, [_i, _i, _i]),
    "tdr_k_compact_map": (_i, [C.POINTER(MapDescC), _vp, _vp, _vp, _vp]),
    "tdr_cmap_wide_words_total": (C.c_size_t, [_i, _i, _i]),
    "tdr_k_compact_map_wide": (_i, [C.POINTER(MapDescC), _vp, _vp, _vp, _vp]),
    "tdr_k_unpack_compact_map": (_i, [C.POINTER(MapDescC), _vp, _vp]),
    "tdr_k_selftest_atan2": (_i, [_vp, _vp, _i64, _vp, _vp]),
    "tdr_libm_variant": (_i, []),
    "tdr_libm_force_variant": (_i, [_i]),
    "tdr_sincosf_host": (_i, [_vp, _i64, _i, _vp, _vp]),
    "tdr_k_selftest_sincos": (_i, [_vp, _i64, _vp, _vp, _vp]),
    "tdr_k_selftest_round": (_i, [_vp, _i64, _f, _vp, _vp]),
    "tdr_k_pack_map": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "tdr_map_ingest_workspace_bytes": (C.c_size_t, [_i, _i, _i]),
    "tdr_map_ingest_shape": (_i, [_i, _i, _f, C.POINTER(_i), C.POINTER(_i)]),
    "tdr_k_map_from_labels": (_i, [_vp, _i, _i, _vp, _i, _i, _f, _vp, _vp, _vp]),
    "tdr_k_map_from_rasters": (_i, [_vp, _i, _i, _i, _f, _vp, _vp, _vp]),
    "tdr_map_incr_tiles": (_i, [_i, _i]),
    "tdr_map_incr_workspace_bytes": (C.c_size_t, [_i, _i]),
    "tdr_k_map_update_labels": (_i, [_vp, _i, _i, _vp, _i, C.POINTER(MapDescC), _vp, _vp, _i64, _vp, _vp,
                                     C.POINTER(_i), C.POINTER(_i64), C.POINTER(_i), _vp]),
    "tdr_k_map_dict_counts": (_i, [C.POINTER(MapDescC), _vp, _vp]),
    "tdr_k_map_gather_tiles": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "tdr_map_save_rasters": (_i, [_vp, C.c_char_p]),
    "tdr_png_read_gray8_host": (_i, [C.c_char_p, _vp, _i64, _vp, _vp]),
    "tdr_png_write_gray8_host": (_i, [C.c_char_p, _vp, _i, _i]),
    "tdr_map_load_rasters": (_i, [_vp, C.c_char_p, _i, _f, _i, _i]),
    "tdr_svg_parse_host": (_i, [C.c_char_p, _vp, C.POINTER(_i64), C.POINTER(_i64), _vp, _vp, _vp]),
    "tdr_map_load_polygons": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _vp, _i, _f, _i, _i, _vp]),
    "tdr_map_load_svg": (_i, [_vp, C.c_char_p, _vp, _vp, _i, _i, _vp, _i, _f, _i, _i]),
    "tdr_k_map_from_color": (_i, [_vp, _i, _i, _vp, _vp, _i, _i, _f, _vp, _vp, _vp]),
    "tdr_k_color_index": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp]),
    "tdr_png_read_color_host": (_i, [C.c_char_p, _vp, _i64, _vp, _vp]),
    "tdr_map_load_color_image": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _i, _f, _i, _i]),
    "tdr_map_load_color_png": (_i, [_vp, C.c_char_p, _vp, _vp, _i, _i, _f, _i, _i]),
    "tdr_polygon_planes": (_i, [_vp, _vp, _vp, _i64, _i, _i, _i, _vp, _i, _f, _vp]),
    "tdr_k_unpack_map": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp]),
    "tdr_polar_table_host": (_i, [_i, _i, _f, _f, _vp]),
    "tdr_raster_workspace_bytes": (_i64, [_i64]),
    "tdr_k_raster_polar": (_i, [_vp, _i, _i, _i64, _f, _f, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "tdr_k_raster_cart": (_i, [_vp, _i, _i, _i64, _f, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "tdr_raster_geo_workspace_bytes": (_i64, [_i64]),
    "tdr_k_raster_geo_polar": (_i, [_vp, _i, _i64, _i64, _f, _f, _i, _i, _vp, _vp, _vp]),
    "tdr_k_raster_geo_cart": (_i, [_vp, _i, _i64, _i64, _f, _i, _i, _vp, _vp]),
    "tdr_k_pack_scan": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "tdr_score_workspace_floats": (C.c_size_t, [_i, _i, _i, _i64, _i64]),
    "tdr_k_score_polar": (_i, [C.POINTER(MapDescC), _vp, _vp, _i, _i, _f, C.POINTER(FilterParamsC), _vp, _i64, _i64,
                               _i64, _vp, _f, _i, _vp, _vp, _vp]),
    "tdr_k_active_diffs": (_i, [C.POINTER(MapDescC), _vp, _i, _i, _f, _vp, _vp, _i, _i, _vp, _vp]),
    "tdr_active_candidates_host": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, C.POINTER(_i), C.POINTER(_i)]),
    "tdr_logf_host": (_i, [_vp, _i64, _vp]),
    "tdr_k_selftest_logf": (_i, [_vp, _i64, _vp, _vp]),
    "tdr_rng_pipe_create": (_i, [_i64, C.POINTER(_vp)]),
    "tdr_rng_pipe_destroy": (None, [_vp]),
    "tdr_rng_pipe_on_device": (_i, [_vp]),
    "tdr_rng_pipe_from_host": (_i, [_vp, _vp, _vp]),
    "tdr_rng_pipe_to_host": (_i, [_vp, _vp, _vp]),
    "tdr_rng_pipe_normals": (_i, [_vp, _i64, _i64, _i64, _i, C.POINTER(_vp), _vp]),
    "tdr_rng_pipe_uniform": (_i, [_vp, C.POINTER(_vp), _vp]),
    "tdr_rng_dev_workspace_bytes": (C.c_size_t, [_i64]),
    "tdr_k_rng_propagate_normals": (_i, [_vp, _i64, _i64, _i64, _i, _vp, _vp, _vp]),
    "tdr_k_rng_uniform": (_i, [_vp, _vp, _vp]),
    "tdr_rng_get_state_host": (_i, [_vp, _vp]),
    "tdr_rng_set_state_host": (_i, [_vp, _vp]),
    "tdr_k_resample_dev": (_i, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp]),
    "tdr_score_ctx_create": (_i, [C.POINTER(_vp)]),
    "tdr_score_ctx_destroy": (None, [_vp]),
    "tdr_score_ctx_span": (C.c_float, [_vp]),
    "tdr_score_ctx_trial_calls": (_i64, [_vp]),
    "tdr_config_tuning": (_i64, [C.c_char_p, _i64]),
    "tdr_su_tail_plan": (_i, [_i, _i, _i, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "tdr_k_su_order_workspace_ints": (C.c_size_t, [_i64, _i]),
    "tdr_k_su_order_slots": (_i64, [_i64, _i]),
    "tdr_k_su_order": (_i, [_vp, _i64, _i64, _vp, _i, _f, _vp, _vp, _vp, _vp, C.POINTER(_i), _vp]),
    "tdr_k_score_prep": (_i, [_vp, _vp, _vp, _i, _i, _f, _vp, _i64, _i64, _i64, _vp, _f, _f, _vp, _vp, C.POINTER(_i64),
                              C.POINTER(_vp), _vp]),
    "tdr_selftest_score": (_i, []),
    # out[16]: [0..11] the dense kernels' loop variants, [12..15] the init search's passes — half records, on the fly,
    # wide, vector kernel: 64-particle batches whose results the pass wrote (include/tdr.h)
    "tdr_profile_variants": (_i, [C.POINTER(_i64)]),
    "tdr_profile_ray_gate": (_i, [C.POINTER(_i64)]),
    # out[2]: steps the dense polar kernel's assembly loop handed back, bins its list pass scored (include/tdr.h)
    "tdr_profile_su_list": (_i, [C.POINTER(_i64)]),
    "tdr_k_score_prep_full_mask": (_i, [_vp, _i, _i, _i64, _i64, _vp, _vp, C.POINTER(_i64), _vp]),
    "tdr_score_ctx_set_polar_factors": (_i, [_vp, _vp, _i, _i]),
    "tdr_polar_factors_host": (_i, [_i, _i, _f, _f, _vp]),
    "tdr_k_score_polar_ctx": (_i, [C.POINTER(MapDescC), _vp, _vp, _i, _i, _f, C.POINTER(FilterParamsC), _vp, _i64, _i64,
                                   _i64, _vp, _f, _i, _vp, _vp, _vp, _vp]),
    "tdr_score_geo_workspace_floats": (C.c_size_t, [_i, _i, _i, _i64, _i64]),
    "tdr_k_score_polar_geo": (_i, [C.POINTER(MapDescC), C.POINTER(MapDescC), _vp, _vp, _vp, _f, _f, _i, _i, _f,
                                   C.POINTER(FilterParamsC), _vp, _i64, _i64, _i64, _vp, _f, _i, _vp, _vp, _vp]),
    "tdr_score_cart_workspace_floats": (C.c_size_t, [_i, _i, _i, _i64, _i64]),
    "tdr_k_score_cart": (_i, [C.POINTER(MapDescC), _vp, _i, _i, _f, C.POINTER(FilterParamsC), _vp, _i64, _i64, _i64,
                              _vp, _vp, _vp, _vp]),
    "tdr_score_cart_init_workspace_floats": (C.c_size_t, [_i, _i, _i, _i64, _i64]),
    "tdr_k_score_cart_init": (_i, [C.POINTER(MapDescC), _vp, _i, _i, _f, C.POINTER(FilterParamsC), _vp, _i64, _i64, _i64,
                                   _vp, _vp]),
    "tdr_k_propagate": (_i, [_vp, _i64, _i64, _vp, _f, _f, _f, _i, _f, _f, _vp, _u64, _u64, _i64, _vp]),
    "tdr_rng_create": (_vp, [_u32]),
    "tdr_rng_destroy": (None, [_vp]),
    "tdr_rng_uniform_host": (_f, [_vp]),
    "tdr_propagate_normals_host": (_i, [_vp, _i64, _i, _vp]),
    "tdr_k_update_weights": (_i, [_vp, _vp, _i64, _vp, _vp, _vp]),
    "tdr_prefix_workspace_bytes": (_i64, [_i64]),
    "tdr_k_prefix": (_i, [_vp, _i64, _vp, _vp, _vp]),
    "tdr_k_prefix_mode": (_i, [_vp, _i64, _i, _vp, _vp, _vp, _vp]),
    "tdr_k_resample": (_i, [_vp, _i64, _i64, _f, _i64, _i64, _vp, _vp]),
    "tdr_k_gather_states": (_i, [_vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp]),
    "tdr_init_particles_host": (_i, [_vp, _vp, _i, _i, _i, _f, C.POINTER(FilterParamsC), _i, _vp, C.POINTER(C.c_int64)]),
    "tdr_init_particles_count": (_i64, [C.POINTER(FilterParamsC), _i]),
    "tdr_init_workspace_bytes": (C.c_size_t, []),
    "tdr_k_init_particles": (_i, [_vp, C.POINTER(MapDescC), C.POINTER(FilterParamsC), _i, _i64, _i64, _vp, _i64,
                                  C.POINTER(C.c_int64), _vp, _vp]),
    "tdr_rng_pipe_init_particles": (_i, [_vp, C.POINTER(MapDescC), C.POINTER(FilterParamsC), _i, _i64, _i64, _vp, _i64,
                                         C.POINTER(C.c_int64), _vp, _vp]),
    "tdr_k_mean_cov": (_i, [_vp, _i64, _i64, _vp, _vp, _vp]),
    "tdr_k_sample_ml_states": (_i, [_vp, _i64, _i64, _i, _vp, _vp]),
    "tdr_gmm_fit_host": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "tdr_gmm_select_host": (_i, [_vp, _i, _i64, _vp, _i, _vp, _vp]),
    "tdr_adaptive_count_host": (_i64, [_vp, _i, _i64, _i64]),
    "tdr_filter_compute_gmm": (_i, [_vp]),
    "tdr_filter_get_gmm": (_i, [_vp, _i, _vp, _vp, _vp]),
    "tdr_filter_adaptive_count": (_i64, [_vp]),
    "tdr_filter_step_count": (_i64, [_vp]),
    "tdr_filter_num_gaussians": (_i, [_vp]),
    "tdr_filter_set_num_gaussians": (_i, [_vp, _i]),
    "tdr_gmm_workspace_bytes": (C.c_size_t, [_i, _i]),
    "tdr_gmm_out_doubles": (_i, [_i]),
    "tdr_k_gmm_samples": (_i, [_vp, _i, _vp, _vp]),
    "tdr_k_gmm_fit": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp]),
    "tdr_k_gmm_fit_jobs": (_i, [_vp, _i, _vp]),
    "tdr_k_gmm_pick": (_i, [_vp, _i, _vp]),
    "tdr_gmm_candidates_host": (_i, [_i, _i64, _i, _i, _vp]),
    "tdr_filter_compute_gmm_device": (_i, [_vp]),
    "tdr_batch_compute_gmm": (_i, [_vp, _i, _vp]),
    "tdr_k_save_ml_state": (_i, [_vp, _vp, _i64, _i64, _i64, _vp, _vp]),
    "tdr_k_resample_gather": (_i, [_vp, _i64, _i64, _vp, _f, _i64, _i64, _vp, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp]),
    "tdr_k_shard_pack2": (_i, [_vp, _vp, _i64, _vp, _vp]),
    "tdr_k_shard_unpack2": (_i, [_vp, _i, _i64, _vp, _vp, _vp]),
    "tdr_k_unshard_states": (_i, [_vp, _i, _i64, _vp, _i64, _vp]),
    "tdr_comm_rccl_unique_id": (_i, [_vp]),
    "tdr_comm_create_rccl": (_i, [_i, _i, _vp, C.POINTER(_vp)]),
    "tdr_comm_create": (_i, [_i, _i, _vp, C.POINTER(_vp)]),
    "tdr_comm_destroy": (None, [_vp]),
    "tdr_comm_world": (_i, [_vp]),
    "tdr_comm_rank": (_i, [_vp]),
    "tdr_comm_all_gather": (_i, [_vp, _vp, _vp, C.c_size_t, _vp]),
    "tdr_comm_broadcast": (_i, [_vp, _vp, C.c_size_t, _i, _vp]),
    "tdr_filter_create_sharded": (_i, [_vp, _i, C.POINTER(FilterParamsC), _u32, _vp, C.POINTER(_vp)]),
    "tdr_filter_num_local": (_i64, [_vp]),
    "tdr_k_set_scale": (_i, [_vp, _i64, _i64, _vp, _vp]),
    "tdr_k_shift_init": (_i, [_vp, _i64, _i64, _f, _f, _vp]),
    "tdr_k_states_aos_to_soa": (_i, [_vp, _i64, _vp, _i64, _vp]),
    "tdr_k_states_soa_to_aos": (_i, [_vp, _i64, _i64, _vp, _vp]),
    "tdr_profile_enable": (_i, [_i]),
    "tdr_profile_score_ms": (_i, [C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "tdr_profile_shares": (_i, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    # handle layer (csrc/tdr_host_*.cpp)
    "tdr_map_create": (_i, [C.POINTER(_vp)]),
    "tdr_map_destroy": (None, [_vp]),
    "tdr_map_set": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _i, _i]),
    "tdr_map_set_labels": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _f, _i, _i]),
    "tdr_filter_update_map_labels": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _f, _i, _i]),
    "tdr_map_update_labels_incremental": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _f, _i, _i, C.POINTER(_i64)]),
    "tdr_map_patch_labels": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, C.POINTER(_i64)]),
    "tdr_map_get_desc": (_i, [_vp, C.POINTER(MapDescC)]),
    "tdr_filter_update_map_labels_incremental": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _f, _i, _i, C.POINTER(_i64)]),
    "tdr_filter_patch_map_labels": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, C.POINTER(_i64)]),
    "tdr_map_sample_pts_polar": (_i, [_vp, _i, _i, _f]),
    "tdr_map_polar_shape": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "tdr_map_set_window": (_i, [_vp, _i, _i]),
    "tdr_map_window_shape": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "tdr_map_info": (_i, [_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_f), C.POINTER(_i)]),
    "tdr_map_center": (_i, [_vp, _vp, _vp]),
    "tdr_map_local_map": (_i, [_vp, _i, _f, _f, _f, _f, _i, _i, _vp, _vp]),
    "tdr_k_local_map_polar": (_i, [_vp, _vp, _i, _i, _f, _f, _f, _f, _vp, _vp, _vp]),
    "tdr_k_local_map_cart": (_i, [_vp, _i, _i, _f, _f, _f, _f, _vp, _vp, _vp]),
    "tdr_map_local_geo_map": (_i, [_vp, _i, _f, _f, _f, _f, _i, _i, _vp]),
    "tdr_map_load_cache": (_i, [_vp, C.c_char_p, C.c_char_p, _i, _f, _i, _i, C.POINTER(_i)]),
    "tdr_map_save_cache": (_i, [_vp, C.c_char_p, C.c_char_p]),
    "tdr_k_geo_map_from_map": (_i, [C.POINTER(MapDescC), _i, _vp, _vp, _vp]),
    "tdr_map_classes_at_point": (_i, [_vp, _i, _i, C.POINTER(_u32)]),
    "tdr_map_best_rel_pos": (_i, [_vp, _vp, _i, _vp, _vp]),
    "tdr_renderer_create": (_i, [_vp, C.POINTER(_vp)]),
    "tdr_renderer_destroy": (None, [_vp]),
    "tdr_renderer_render": (_i, [_vp, _i, _vp, _i, _i, _i64, _f, _f, _i, _i, _i, _vp]),
    "tdr_renderer_render_geo": (_i, [_vp, _i, _vp, _i, _i64, _i64, _f, _f, _i, _i, _vp]),
    "tdr_filter_create": (_i, [_vp, _i, C.POINTER(FilterParamsC), _u32, C.POINTER(_vp)]),
    "tdr_filter_create_cart": (_i, [_vp, _i, C.POINTER(FilterParamsC), _u32, C.POINTER(_vp)]),
    "tdr_filter_destroy": (None, [_vp]),
    "tdr_filter_configure": (_i, [_vp, _i, _i]),
    "tdr_filter_initialize_particles": (_i, [_vp]),
    "tdr_filter_set_states": (_i, [_vp, _vp, _i64]),
    "tdr_filter_get_states": (_i, [_vp, _vp, _i64]),
    "tdr_filter_propagate": (_i, [_vp, _f, _f, _f]),
    "tdr_filter_update": (_i, [_vp, _vp, _vp, _f, _i64]),
    "tdr_filter_update_geo": (_i, [_vp, _vp, _vp, _f, _i64]),
    "tdr_filter_compute_weights": (_i, [_vp, _vp, _vp, _f]),
    "tdr_filter_get_raw_weights": (_i, [_vp, _vp, _i64]),
    "tdr_filter_get_last_dist": (_i, [_vp, _vp, _i64]),
    "tdr_filter_propagate_freeze": (_i, [_vp, _f, _f, _f, _i]),
    "tdr_filter_init_one": (_i, [_vp]),
    "tdr_filter_share_rng": (_i, [_vp, _vp]),
    "tdr_init_particle_host": (_i, [_vp, _vp, _i, _i, _i, _f, _vp, _vp]),
    "tdr_filter_get_weights": (_i, [_vp, _vp, _i64]),
    "tdr_filter_get_resample_indices": (_i, [_vp, _vp, _i64]),
    "tdr_filter_mean_cov": (_i, [_vp, _i, _vp, _vp]),
    "tdr_filter_freeze_scale": (_i, [_vp]),
    "tdr_filter_is_scale_frozen": (_i, [_vp]),
    "tdr_filter_scale": (_f, [_vp]),
    "tdr_filter_num_particles": (_i64, [_vp]),
    "tdr_filter_update_map": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _i, _i]),
    "tdr_batch_step": (_i, [_vp, _i, _vp, _vp]),
    "tdr_batch_last_stats": (_i, [_vp, _vp]),
    "tdr_batch_render_polar": (_i, [_vp, _i, _vp, _f, _i, _i, _i, _vp]),
    "tdr_renderer_get_render": (_i, [_vp, _vp, _vp]),
    "tdr_batch_pose": (_i, [_vp, _i, _vp, _vp]),
    "tdr_viz_plane_words": (C.c_size_t, [_i, _i]),
    "tdr_viz_arrow_host": (_i, [_i, _i, _vp]),
    "tdr_viz_overlay_host": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _vp, _i, C.POINTER(_i)]),
    "tdr_k_viz_particles": (_i, [_vp, _i64, _i64, _i, _i, _vp, _vp]),
    "tdr_k_viz_segments": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "tdr_k_viz_compose": (_i, [_vp, _i, _i, _vp, _i, _i, _vp, _vp]),
    "tdr_filter_set_viz_background": (_i, [_vp, _vp, _i, _i]),
    "tdr_filter_visualize": (_i, [_vp, _f, _vp, _i, _vp, _i64, C.POINTER(_i), C.POINTER(_i)]),
    "tdr_k_viz_particles_jobs": (_i, [_vp, _i, _i64, _vp]),
    "tdr_k_viz_segments_jobs": (_i, [_vp, _i, _i, _vp]),
    "tdr_k_viz_compose_jobs": (_i, [_vp, _i, _i64, _vp]),
    "tdr_batch_visualize": (_i, [_vp, _i, _f, _vp, _vp]),
    "tdr_k_viz_compose_fleet": (_i, [_vp, _i, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp]),
    "tdr_map_set_viz_background": (_i, [_vp, _vp, _i, _i]),
    "tdr_map_set_viz_background_labels": (_i, [_vp, _vp, _i, _i, _vp]),
    "tdr_batch_visualize_fleet": (_i, [_vp, _i, _f, _vp, _vp, _i, _vp, _i64, C.POINTER(_i), C.POINTER(_i), _vp]),
    "tdr_k_scan_picture": (_i, [_vp, _i, _i64, _vp, _vp, _vp, _vp]),
    "tdr_k_analog_picture": (_i, [_vp, _i64, _f, _vp, _vp]),
    "tdr_k_label_picture": (_i, [_vp, _i64, _vp, _vp, _vp]),
    "tdr_k_scan_picture_jobs": (_i, [_vp, _i, _i64, _vp, _i, _vp, _vp]),
    "tdr_k_analog_picture_jobs": (_i, [_vp, _i, _i64, _f, _vp]),
    "tdr_k_label_picture_jobs": (_i, [_vp, _i, _i64, _vp, _vp]),
    "tdr_renderer_visualize": (_i, [_vp, _vp, _vp, _vp, _i64, C.POINTER(_i), C.POINTER(_i)]),
    "tdr_renderer_visualize_analog": (_i, [_vp, _i, _f, _vp, _i64, C.POINTER(_i), C.POINTER(_i)]),
    "tdr_scan_picture_host": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp]),
    "tdr_filter_set_viz_background_labels": (_i, [_vp, _vp, _i, _i, _vp]),
    "tdr_batch_scan_pictures": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    # map fusion (csrc/tdr_fuse.hip, csrc/tdr_host_fuse.cpp)
    "tdr_k_fuse_votes_jobs": (_i, [_vp, _vp, _i, _i, _vp, _i, _i64, _vp, _vp, _vp, _vp]),
    "tdr_k_fuse_votes": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _i, _f, _f, _f, _f, _f, _vp, _vp, _vp, _vp]),
    "tdr_k_fuse_labels": (_i, [_vp, _i, _i, _i, _i, _i, _f, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _i, _vp, _vp]),
    "tdr_k_fuse_decay": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "tdr_fuser_create": (_i, [_vp, _vp, _u32, _u32, _u32, C.POINTER(_vp)]),
    "tdr_fuser_destroy": (None, [_vp]),
    "tdr_fuser_add": (_i, [_vp, _vp, _f, _f, _f, _f, _f, C.POINTER(_u64), C.POINTER(_u64)]),
    "tdr_fuser_add_batch": (_i, [_vp, _vp, _i, _vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "tdr_fuser_add_images": (_i, [_vp, _vp, _i, _i, _i, _f, _f, _f, _f, _f, C.POINTER(_u64), C.POINTER(_u64)]),
    "tdr_fuser_apply": (_i, [_vp, _vp, _i, C.POINTER(_i64)]),
    "tdr_fuser_decay": (_i, [_vp, _i]),
    "tdr_fuser_reset": (_i, [_vp]),
    "tdr_fuser_rebase": (_i, [_vp, C.POINTER(_i)]),
    "tdr_fuser_get_votes": (_i, [_vp, _vp]),
    "tdr_fuser_get_labels": (_i, [_vp, _vp]),
    "tdr_fuser_stats": (_i, [_vp, _vp]),
    # KLD-sampling count (csrc/tdr_kld.hip, csrc/tdr_host_kld.cpp)
    "tdr_kld_workspace_bytes": (C.c_size_t, [_i64]),
    "tdr_k_kld_keys": (_i, [_vp, _i64, _i64, C.POINTER(KldParamsC), _vp, _vp]),
    "tdr_k_kld_count": (_i, [_vp, _i64, _i64, C.POINTER(KldParamsC), _vp, _vp, _vp]),
    "tdr_k_kld_count_jobs": (_i, [_vp, _i, C.POINTER(KldParamsC), _vp]),
    "tdr_kld_bound_host": (_i64, [_i64, C.c_double, C.c_double]),
    "tdr_kld_target_host": (_i64, [_i64, _i64, _i64, _i64]),
    "tdr_filter_kld_count": (_i, [_vp, C.POINTER(KldParamsC), C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    "tdr_batch_kld_count": (_i, [_vp, _i, C.POINTER(KldParamsC), _vp, _vp, _vp, _vp]),
    # recovery injection (csrc/tdr_recover.hip, csrc/tdr_host_recover.cpp)
    "tdr_philox4x32_host": (None, [_vp, _vp, _vp]),
    "tdr_inject_threshold_host": (_u32, [C.c_double]),
    "tdr_recovery_track_host": (C.c_double, [C.POINTER(RecoveryStateC), C.c_double, C.POINTER(RecoveryParamsC)]),
    "tdr_recovery_reset_host": (None, [C.POINTER(RecoveryStateC)]),
    "tdr_map_road_workspace_bytes": (C.c_size_t, [_i, _i]),
    "tdr_k_map_road_cells": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "tdr_k_inject": (_i, [_vp, _i64, _i64, _i64, _vp, _vp, _i64, _u64, _u64, _u32, _i, _vp, _vp]),
    "tdr_k_inject_jobs": (_i, [_vp, _i, _vp]),
    "tdr_map_road_cells": (_i, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "tdr_map_read_road_cells": (_i, [_vp, _vp, _i64, C.POINTER(_i64)]),
    "tdr_filter_get_weight_stats": (_i, [_vp, _vp]),
    "tdr_filter_inject": (_i, [_vp, C.c_double, _i, _u64, C.POINTER(_i64)]),
    "tdr_filter_recovery_step": (_i, [_vp, C.POINTER(RecoveryStateC), C.POINTER(RecoveryParamsC), C.POINTER(C.c_double),
                                      C.POINTER(_i64)]),
    "tdr_batch_inject": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp]),
    # sensor resetting (csrc/tdr_recover_sensor.hip, csrc/tdr_host_recover.cpp)
    "tdr_inject_list_workspace_bytes": (C.c_size_t, [_i64]),
    "tdr_k_inject_list": (_i, [_i64, _i64, _u64, _u64, _u32, _vp, _vp, _vp, _i, _vp]),
    "tdr_k_inject_candidates": (_i, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _i, _vp, _vp, _i64, _u64, _u64, _i, _vp, _i64, _vp]),
    "tdr_k_inject_select": (_i, [_vp, _i64, _i64, _vp, _i64, _i64, _i, _vp, _i64, _vp, _vp, _vp, _vp]),
    "tdr_filter_inject_sensor": (_i, [_vp, _vp, _vp, _f, C.c_double, _i, _i, _u64, C.POINTER(_i64)]),
    "tdr_filter_recovery_step_sensor": (_i, [_vp, C.POINTER(RecoveryStateC), C.POINTER(RecoveryParamsC), _i, _vp, _vp, _f,
                                             C.POINTER(C.c_double), C.POINTER(_i64)]),
    # pose-grid search (csrc/tdr_grid.hip, csrc/tdr_host_grid.cpp)
    "tdr_grid_list_workspace_bytes": (C.c_size_t, [_i, _i]),
    "tdr_k_grid_list": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "tdr_k_grid_candidates": (_i, [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp]),
    "tdr_k_grid_reduce": (_i, [_vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "tdr_grid_peaks_workspace_bytes": (C.c_size_t, [_i, _i]),
    "tdr_k_grid_peaks": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "tdr_filter_grid_search": (_i, [_vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _i, _i, _vp, C.POINTER(_i64), C.POINTER(_i64)]),
    "tdr_filter_inject_cells": (_i, [_vp, _vp, _i64, C.c_double, _i, _u64, C.POINTER(_i64)]),
    "tdr_set_error": (_i, [_i, C.c_char_p]),
    "tdr_locality_tmp_ints": (C.c_size_t, [_i64, _i, _i]),
    "tdr_locality_pose_tmp_ints": (C.c_size_t, [_i64]),
    "tdr_k_locality_order_pose": (_i, [_vp, _i64, _i64, _i, _i, _f, _vp, _vp, _vp]),
    "tdr_k_locality_order": (_i, [_vp, _i64, _i64, _i, _i, _vp, _vp, _vp]),
}

_lib = None


class TdrError(RuntimeError):
    pass


def load():
    """Loads libtdr_hip.so and binds every entry point; raises TdrError if the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise TdrError(
            f"{SO_PATH} is missing: build the HIP extension first (python -m top_down_renderer_amd.build, or "
            "__graft_entry__.build()).  There is no CPU fallback.")
    L = C.CDLL(SO_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)  # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise TdrError(f"libtdr_hip error {rc}: {load().tdr_last_error().decode()}")

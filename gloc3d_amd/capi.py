"""ctypes binding of the C ABI in include/gloc3d.h (gloc3d_amd/lib/libgloc3d.so).

This is the same binding a reference-side maintainer would write.  It fails loudly
when the HIP extension is missing or no gfx950 device is usable: there is no CPU fallback.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GLOC3D_LIB_PATH") or os.path.join(HERE, "lib", "libgloc3d.so")  # (override: dev builds)

GLOC_OK = 0
ERR_NAMES = {1: "GLOC_ERR_INVALID", 2: "GLOC_ERR_HIP", 3: "GLOC_ERR_NOMEM", 4: "GLOC_ERR_NODEVICE",
             5: "GLOC_ERR_STATE"}
ALGO_AUTO, ALGO_EXACT, ALGO_MFMA, ALGO_MFMA_FP32 = 0, 1, 2, 3   # include/gloc3d.h GLOC_KNN_ALGO_*
KNN_OPT_ALGO, KNN_OPT_CANDIDATES, KNN_OPT_PROFILE = 1, 2, 3
REG_OPT_PROFILE, REG_OPT_NN_MODE, REG_OPT_NN_SRC_PER_LANE, REG_OPT_NN_JOB_GROUP, REG_OPT_TEMP_TARGET_INDEX = 1, 2, 3, 4, 5
REG_OPT_NN_SPLIT_HELPERS, REG_OPT_NN_SPLIT_THRESH, REG_OPT_NN_SUB_JOBS, REG_OPT_NN_HEAVY_THRESH, REG_OPT_SUB_BATCHES = 6, 7, 8, 9, 10
REG_OPT_NN_CHAIN = 11
REG_OPT_PAIRGRAPH_BUDGET = 12
REG_NN_CULLED, REG_NN_EXHAUSTIVE = 0, 1
NO_SCAN = 0xFFFFFFFF
SIZE_MAX = C.c_size_t(-1).value


class GlocError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{ERR_NAMES.get(code, code)}: {msg}")
        self.code = code


class RaycastParams(C.Structure):
    _fields_ = [("n_beams", C.c_uint32), ("n_az", C.c_uint32), ("max_range", C.c_double), ("noise_sigma", C.c_double),
                ("fov_lo_deg", C.c_double), ("fov_hi_deg", C.c_double)]


class KnnStats(C.Structure):
    _fields_ = [("searches_exact", C.c_uint64), ("searches_mfma", C.c_uint64),
                ("queries_total", C.c_uint64), ("queries_fallback", C.c_uint64),
                ("last_n_tile", C.c_uint32), ("last_k_split", C.c_uint32),
                ("last_candidates", C.c_uint32)]


class RegParams(C.Structure):
    _fields_ = [("ransac_iters", C.c_uint32), ("inlier_thresh", C.c_float),
                ("min_inlier_ratio", C.c_float), ("icp_iters", C.c_uint32),
                ("max_corr_dist", C.c_float), ("seed", C.c_uint64),
                ("ransac_confidence", C.c_float), ("max_rmse", C.c_float), ("max_final_step", C.c_float)]


class NdtParams(C.Structure):
    _fields_ = [("source_leaf", C.c_float), ("resolution", C.c_float), ("step_size", C.c_float), ("trans_eps", C.c_float),
                ("max_iters", C.c_uint32), ("outlier_ratio", C.c_float), ("min_points_per_cell", C.c_uint32),
                ("min_covar_eigvalue_mult", C.c_float)]


class SubmapParams(C.Structure):
    _fields_ = [("leaf", C.c_float), ("min_points", C.c_uint32), ("min_scans", C.c_uint32), ("max_range", C.c_float),
                ("group_points", C.c_uint32)]


class SubmapInfo(C.Structure):
    _fields_ = [("points_in", C.c_uint64), ("points_used", C.c_uint64), ("cells", C.c_uint32), ("kept", C.c_uint32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class P2lParams(C.Structure):
    _fields_ = [("max_iters", C.c_uint32), ("max_corr_dist", C.c_float), ("trans_eps", C.c_float), ("rot_eps", C.c_float),
                ("normal_k", C.c_uint32), ("reserved_", C.c_uint32)]


class GicpParams(C.Structure):
    _fields_ = [("max_iters", C.c_uint32), ("max_corr_dist", C.c_float), ("trans_eps", C.c_float), ("rot_eps", C.c_float),
                ("normal_k", C.c_uint32), ("plane_eps", C.c_float)]


class VgicpParams(C.Structure):
    _fields_ = [("max_iters", C.c_uint32), ("max_corr_dist", C.c_float), ("trans_eps", C.c_float), ("rot_eps", C.c_float),
                ("normal_k", C.c_uint32), ("plane_eps", C.c_float), ("resolution", C.c_float), ("neighbors", C.c_uint32),
                ("min_points", C.c_uint32), ("reserved_", C.c_uint32)]


class VmapParams(C.Structure):
    _fields_ = [("resolution", C.c_float), ("capacity", C.c_uint32), ("normal_k", C.c_uint32), ("reserved_", C.c_uint32)]


class VmapInfo(C.Structure):
    _fields_ = [("n_voxels", C.c_uint32), ("capacity", C.c_uint32), ("n_inserts", C.c_uint32), ("resolution", C.c_float),
                ("n_points", C.c_uint64)]


class RobustParams(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("scale", C.c_float), ("scale_start", C.c_float), ("anneal", C.c_float)]


ROBUST_NONE, ROBUST_HUBER, ROBUST_CAUCHY, ROBUST_TUKEY, ROBUST_GEMAN_MCCLURE = range(5)


class PgoParams(C.Structure):
    _fields_ = [("max_iters", C.c_uint32), ("pcg_max_iters", C.c_uint32), ("lambda_init", C.c_double), ("pcg_tol", C.c_double),
                ("rot_eps", C.c_double), ("trans_eps", C.c_double), ("grad_eps", C.c_double), ("reserved_", C.c_uint32 * 2)]


class PgoResult(C.Structure):
    _fields_ = [("iters", C.c_uint32), ("accepted", C.c_uint32), ("pcg_iters", C.c_uint32), ("status", C.c_int32),
                ("cost_initial", C.c_double), ("cost_final", C.c_double), ("lam", C.c_double), ("grad_inf", C.c_double)]


class PgoConsistencyParams(C.Structure):
    _fields_ = [("chi2", C.c_double), ("drift_rot", C.c_double), ("drift_trans", C.c_double), ("n_seeds", C.c_uint32),
                ("min_clique", C.c_uint32), ("reserved_", C.c_uint32 * 2)]


class FpfhParams(C.Structure):
    _fields_ = [("normal_k", C.c_uint32), ("feature_k", C.c_uint32), ("mutual", C.c_uint32), ("ransac_iters", C.c_uint32),
                ("inlier_thresh", C.c_float), ("min_inlier_ratio", C.c_float), ("ransac_confidence", C.c_float),
                ("reserved_", C.c_uint32), ("seed", C.c_uint64)]


class FpfhGraphParams(C.Structure):
    _fields_ = [("normal_k", C.c_uint32), ("feature_k", C.c_uint32), ("mutual", C.c_uint32), ("n_seeds", C.c_uint32),
                ("compat_thresh", C.c_float), ("inlier_thresh", C.c_float), ("min_inlier_ratio", C.c_float),
                ("theta_num", C.c_uint32), ("theta_den", C.c_uint32), ("reserved_", C.c_uint32)]


class FgrParams(C.Structure):
    _fields_ = [("normal_k", C.c_uint32), ("feature_k", C.c_uint32), ("mutual", C.c_uint32), ("tuple_tries", C.c_uint32),
                ("max_tuples", C.c_uint32), ("tuple_scale", C.c_float), ("max_iters", C.c_uint32), ("anneal_every", C.c_uint32),
                ("anneal_div", C.c_float), ("max_corr_dist", C.c_float), ("inlier_thresh", C.c_float), ("min_inlier_ratio", C.c_float),
                ("seed", C.c_uint64)]


class EvalParams(C.Structure):
    _fields_ = [("max_corr_dist", C.c_float), ("reserved_", C.c_uint32)]


class FpfhRadiusParams(C.Structure):
    _fields_ = [("normal_radius", C.c_float), ("normal_max_nn", C.c_uint32), ("normal_min_nn", C.c_uint32),
                ("feature_radius", C.c_float), ("feature_max_nn", C.c_uint32), ("reserved_", C.c_uint32)]


class IssParams(C.Structure):
    _fields_ = [("salient_radius", C.c_float), ("max_nn", C.c_uint32), ("min_nn", C.c_uint32), ("non_max_radius", C.c_float),
                ("gamma_21", C.c_float), ("gamma_32", C.c_float)]


class ClusterParams(C.Structure):
    _fields_ = [("tolerance", C.c_float), ("min_size", C.c_uint32), ("max_size", C.c_uint32), ("reserved_", C.c_uint32)]


class ScanFilterParams(C.Structure):
    _fields_ = [("min_range", C.c_float), ("max_range", C.c_float), ("ror_radius", C.c_float), ("ror_min_neighbors", C.c_uint32),
                ("sor_mean_k", C.c_uint32), ("sor_std_mul", C.c_float), ("cluster", ClusterParams)]


class ScanFilterInfo(C.Structure):
    _fields_ = [("points_in", C.c_uint32), ("after_range", C.c_uint32), ("after_ror", C.c_uint32), ("after_sor", C.c_uint32),
                ("after_cluster", C.c_uint32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class Clusters:
    """What ScanStore.cluster returns (E1 - E4 of include/gloc3d.h): root, cluster [n] uint32 in upload order (0xFFFFFFFF: a
    non-finite point / a point of no kept cluster); size, cluster_root [n_kept] uint32, centroid [n_kept, 3] float64, lo, hi
    [n_kept, 3] float32 in rank order; n_components, n_kept."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


FPFH_DIM = 33          # floats per feature row
FPFH_MATCH_TILE = 128  # target rows per tile of the matcher (csrc/fpfh.hpp MATCH_TILE_ROWS)


class BevParams(C.Structure):
    _fields_ = [("resolution", C.c_float), ("max_range", C.c_float), ("out_width", C.c_uint32),
                ("out_height", C.c_uint32), ("format", C.c_uint32), ("pad_bgr", C.c_uint8 * 3),
                ("reserved_", C.c_uint8)]


class BevInfo(C.Structure):
    _fields_ = [("min_ix", C.c_int32), ("min_iy", C.c_int32), ("max_ix", C.c_int32),
                ("max_iy", C.c_int32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("n_returns", C.c_uint32), ("empty", C.c_uint32), ("ox", C.c_double),
                ("oy", C.c_double), ("resolution", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


BEV_U8_HWC3, BEV_F32_CHW = 0, 1


class PillarParams(C.Structure):
    _fields_ = [("xbound", C.c_float * 3), ("ybound", C.c_float * 3), ("zbound", C.c_float * 3),
                ("num_points", C.c_uint32), ("mask_mode", C.c_uint32)]

    def grid(self):
        """(gx, gy, gz) as the library and voxel.py:40-45 compute them."""
        return tuple(int((float(b[1]) - float(b[0])) / float(b[2])) for b in (self.xbound, self.ybound, self.zbound))


PILLAR_MASK_INPUT, PILLAR_MASK_VALID = 0, 1   # include/gloc3d.h GLOC_PILLAR_MASK_*
PILLAR_FEATURES = 64
GROUND_OPT_KNN_EXHAUSTIVE = 1


class CoarseParams(C.Structure):
    _fields_ = [("resolution", C.c_float), ("cell_px", C.c_uint32), ("n_yaw", C.c_uint32), ("max_shift", C.c_uint32),
                ("top_yaw", C.c_uint32), ("refine", C.c_uint32), ("min_overlap", C.c_float), ("reserved_", C.c_uint32)]


class ScParams(C.Structure):
    _fields_ = [("n_rings", C.c_uint32), ("n_sectors", C.c_uint32), ("max_radius", C.c_float), ("sensor_height", C.c_float),
                ("min_common_columns", C.c_uint32), ("reserved_", C.c_uint32)]


class M2dpParams(C.Structure):
    _fields_ = [("n_azimuth", C.c_uint32), ("n_elevation", C.c_uint32), ("n_rings", C.c_uint32), ("n_sectors", C.c_uint32),
                ("max_range", C.c_float), ("min_points", C.c_uint32), ("reserved_", C.c_uint32)]


class GroundParams(C.Structure):
    _fields_ = [("near_range2", C.c_float), ("knn", C.c_uint32), ("plane_thresh", C.c_float),
                ("ransac_iters", C.c_uint32), ("ransac_conf", C.c_float), ("reserved_", C.c_uint32),
                ("seed", C.c_uint64)]


class GroundInfo(C.Structure):
    _fields_ = [("n_near", C.c_uint32), ("hist", C.c_uint32 * 18), ("ground_bin", C.c_int32),
                ("n_ground", C.c_uint32), ("best_hyp", C.c_uint32), ("inliers", C.c_uint32),
                ("iters_used", C.c_uint32), ("plane", C.c_float * 4), ("found", C.c_int32)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["hist"] = np.array(list(self.hist), np.uint32)
        d["plane"] = np.array(list(self.plane), np.float32)
        return d


# every symbol include/gloc3d.h declares: (name, restype, argtypes)
_vp, _sz, _u64, _i, _u32 = C.c_void_p, C.c_size_t, C.c_uint64, C.c_int, C.c_uint32
_PROTOS = [
    ("gloc_last_error", C.c_char_p, []),
    ("gloc_abi_version", _i, []),
    ("gloc_device_count", _i, []),
    ("gloc_knn_create", _i, [_i, _sz, C.POINTER(_vp)]),
    ("gloc_knn_create_view", _i, [_vp, C.POINTER(_vp)]),
    ("gloc_knn_destroy", _i, [_vp]),
    ("gloc_knn_set_stream", _i, [_vp, _vp]),
    ("gloc_knn_synchronize", _i, [_vp]),
    ("gloc_knn_set_option", _i, [_vp, _i, C.c_int64]),
    ("gloc_knn_add", _i, [_vp, _vp, _sz]),
    ("gloc_knn_add_device", _i, [_vp, _vp, _sz]),
    ("gloc_knn_reserve", _i, [_vp, _sz]),
    ("gloc_knn_clear", _i, [_vp]),
    ("gloc_knn_size", _i, [_vp, C.POINTER(_sz)]),
    ("gloc_knn_dim", _i, [_vp, C.POINTER(_sz)]),
    ("gloc_knn_device_rows", _i, [_vp, C.POINTER(_vp)]),
    ("gloc_knn_save", _i, [_vp, C.c_char_p]),
    ("gloc_knn_load", _i, [_vp, C.c_char_p]),
    ("gloc_knn_search", _i, [_vp, _vp, _sz, _sz, _sz, _sz, _vp, _vp]),
    ("gloc_knn_search_device", _i, [_vp, _vp, _sz, _sz, _sz, _sz, _u64, _vp, _vp]),
    ("gloc_topk_merge_device", _i, [_i, _vp, _vp, _vp, _sz, _sz, _sz, _vp, _vp]),
    ("gloc_comm_unique_id", _i, [_vp]),
    ("gloc_comm_create", _i, [_i, _i, _i, _vp, C.POINTER(_vp)]),
    ("gloc_comm_destroy", _i, [_vp]),
    ("gloc_comm_rank", _i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    ("gloc_comm_all_gather_device", _i, [_vp, _vp, _vp, _sz, _vp]),
    ("gloc_knn_search_sharded", _i, [_vp, _vp, _vp, _sz, _sz, _u64, _u64, _vp, _vp]),
    ("gloc_knn_search_sharded_host", _i, [_vp, _vp, _vp, _sz, _sz, _u64, _u64, _vp, _vp]),
    ("gloc_comm_all_gather_host", _i, [_vp, _vp, _vp, _sz]),
    ("gloc_knn_get_stats", _i, [_vp, C.POINTER(KnnStats)]),
    ("gloc_knn_profile", _i, [_vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(_u64)]),
    ("gloc_knn_profile_reset", _i, [_vp]),
    ("gloc_reg_default_params", None, [C.POINTER(RegParams)]),
    ("gloc_reg_create", _i, [_i, C.POINTER(_vp)]),
    ("gloc_reg_destroy", _i, [_vp]),
    ("gloc_reg_set_stream", _i, [_vp, _vp]),
    ("gloc_reg_synchronize", _i, [_vp]),
    ("gloc_reg_set_option", _i, [_vp, _i, C.c_int64]),
    ("gloc_scan_store_create", _i, [_i, C.POINTER(_vp)]),
    ("gloc_scan_store_destroy", _i, [_vp]),
    ("gloc_scan_store_add", _i, [_vp, _vp, _sz, _sz, C.POINTER(_u32)]),
    ("gloc_scan_store_add_device", _i, [_vp, _vp, _sz, _sz, C.POINTER(_u32)]),
    ("gloc_scan_store_add_variant", _i, [_vp, _u32, _vp, C.c_float, _u64, C.POINTER(_u32)]),
    ("gloc_scan_store_add_raycast_batch", _i, [_vp, _sz, _vp, _vp, _vp, C.c_double, _vp, _vp, _vp, _vp]),
    ("gloc_scan_store_build_target_index", _i, [_vp, _u32]),
    ("gloc_scan_store_build_target_index_batch", _i, [_vp, _vp, _sz]),
    ("gloc_scan_store_add_batch", _i, [_vp, _vp, _vp, _sz, _sz, _vp]),
    ("gloc_scan_store_release", _i, [_vp, _u32]),
    ("gloc_scan_store_clear", _i, [_vp]),
    ("gloc_scan_store_count", _i, [_vp, C.POINTER(_sz)]),
    ("gloc_scan_store_bytes", _i, [_vp, C.POINTER(_sz), C.POINTER(_sz)]),
    ("gloc_scan_store_points", _i, [_vp, _u32, C.POINTER(_sz)]),
    ("gloc_scan_store_download", _i, [_vp, _u32, _vp, _sz]),
    ("gloc_reg_attach_store", _i, [_vp, _vp]),
    ("gloc_reg_scan_upload", _i, [_vp, _vp, _sz, _sz, C.POINTER(_u32)]),
    ("gloc_reg_scan_build_target_index", _i, [_vp, _u32]),
    ("gloc_reg_scan_release", _i, [_vp, _u32]),
    ("gloc_reg_scan_count", _i, [_vp, C.POINTER(_sz)]),
    ("gloc_reg_scan_clear", _i, [_vp]),
    ("gloc_reg_batch_multi", _i, [_vp, _sz, _vp, _vp, _sz, _vp, _vp, C.POINTER(RegParams), _vp, _vp, _vp,
                                  _vp]),
    ("gloc_reg_batch_multi_begin", _i, [_vp, _sz, _vp, _vp, _sz, _vp, _vp, C.POINTER(RegParams)]),
    ("gloc_reg_batch_multi_end", _i, [_vp, _vp, _vp, _vp, _vp]),
    ("gloc_reg_batch", _i, [_vp, _vp, _sz, C.POINTER(_vp), C.POINTER(_sz), _sz, _vp, _vp,
                            C.POINTER(RegParams), _vp, _vp, _vp, _vp]),
    ("gloc_reg_batch_ids", _i, [_vp, _u32, _vp, _sz, _vp, _vp, C.POINTER(RegParams), _vp, _vp, _vp,
                                _vp]),
    ("gloc_reg_first_success_multi", _i, [_vp, _sz, _vp, _vp, _sz, _vp, C.POINTER(RegParams), _vp, _vp, _vp, _vp,
                                          C.POINTER(_u64)]),
    ("gloc_reg_select_first_ok", _i, [_vp, _sz]),
    ("gloc_reg_final_steps", _i, [_vp, _vp, _sz]),
    ("gloc_reg_nn", _i, [_vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp]),
    ("gloc_reg_ransac_hypotheses", _i, [_vp, _vp, _vp, _vp, _sz, _u64, _u32, _u32, _vp, _vp, _vp,
                                        C.c_float]),
    ("gloc_reg_profile", _i, [_vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(_u64)]),
    ("gloc_reg_profile_reset", _i, [_vp]),
    ("gloc_reg_nn_stats", _i, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    ("gloc_ndt_default_params", None, [C.POINTER(NdtParams)]),
    ("gloc_scan_store_build_normals", _i, [_vp, _u32, _u32]),
    ("gloc_scan_store_normals", _i, [_vp, _u32, _vp, _sz]),
    ("gloc_p2l_default_params", None, [C.POINTER(P2lParams)]),
    ("gloc_reg_p2l_batch_ids", _i, [_vp, _u32, _vp, _sz, _vp, C.POINTER(P2lParams), _vp, _vp, _vp, _vp]),
    ("gloc_reg_p2l_system", _i, [_vp, _u32, _u32, _vp, C.POINTER(P2lParams), _vp, _vp, C.POINTER(C.c_double),
                             C.POINTER(C.c_uint64)]),
    ("gloc_gicp_default_params", None, [C.POINTER(GicpParams)]),
    ("gloc_reg_gicp_batch_ids", _i, [_vp, _u32, _vp, _sz, _vp, C.POINTER(GicpParams), _vp, _vp, _vp, _vp]),
    ("gloc_reg_gicp_system", _i, [_vp, _u32, _u32, _vp, C.POINTER(GicpParams), _vp, _vp, C.POINTER(C.c_double),
                              C.POINTER(C.c_uint64)]),
    ("gloc_vgicp_default_params", None, [C.POINTER(VgicpParams)]),
    ("gloc_reg_vgicp_batch_ids", _i, [_vp, _u32, _vp, _sz, _vp, C.POINTER(VgicpParams), _vp, _vp, _vp, _vp]),
    ("gloc_reg_vgicp_system", _i, [_vp, _u32, _u32, _vp, C.POINTER(VgicpParams), _vp, _vp, C.POINTER(C.c_double),
                               C.POINTER(C.c_uint64)]),
    ("gloc_reg_vgicp_voxels", _i, [_vp, _u32, C.POINTER(VgicpParams), _sz, _vp, _vp, _vp, _vp, C.POINTER(_sz)]),
    ("gloc_robust_default_params", None, [C.POINTER(RobustParams)]),
    ("gloc_robust_scale", _i, [C.POINTER(RobustParams), _u32, C.POINTER(C.c_double)]),
    ("gloc_robust_weight", _i, [C.POINTER(RobustParams), _u32, C.c_double, C.POINTER(C.c_double)]),
    ("gloc_reg_p2l_batch_ids_robust", _i, [_vp, _u32, _vp, _sz, _vp, C.POINTER(P2lParams), C.POINTER(RobustParams), _vp, _vp, _vp, _vp, _vp]),
    ("gloc_reg_gicp_batch_ids_robust", _i, [_vp, _u32, _vp, _sz, _vp, C.POINTER(GicpParams), C.POINTER(RobustParams), _vp, _vp, _vp, _vp, _vp]),
    ("gloc_reg_vgicp_batch_ids_robust", _i, [_vp, _u32, _vp, _sz, _vp, C.POINTER(VgicpParams), C.POINTER(RobustParams), _vp, _vp, _vp, _vp, _vp]),
    ("gloc_reg_p2l_pairs", _i, [_vp, _vp, _vp, _sz, _vp, C.POINTER(P2lParams), C.POINTER(RobustParams), _vp, _vp, _vp, _vp, _vp]),
    ("gloc_reg_gicp_pairs", _i, [_vp, _vp, _vp, _sz, _vp, C.POINTER(GicpParams), C.POINTER(RobustParams), _vp, _vp, _vp, _vp, _vp]),
    ("gloc_reg_vgicp_pairs", _i, [_vp, _vp, _vp, _sz, _vp, C.POINTER(VgicpParams), C.POINTER(RobustParams), _vp, _vp, _vp, _vp, _vp]),
    ("gloc_reg_p2l_system_robust", _i, [_vp, _u32, _u32, _vp, C.POINTER(P2lParams), C.POINTER(RobustParams), _u32, _vp, _vp, C.POINTER(C.c_double),
                                    C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    ("gloc_reg_gicp_system_robust", _i, [_vp, _u32, _u32, _vp, C.POINTER(GicpParams), C.POINTER(RobustParams), _u32, _vp, _vp, C.POINTER(C.c_double),
                                     C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    ("gloc_reg_vgicp_system_robust", _i, [_vp, _u32, _u32, _vp, C.POINTER(VgicpParams), C.POINTER(RobustParams), _u32, _vp, _vp, C.POINTER(C.c_double),
                                      C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    ("gloc_fpfh_default_params", None, [C.POINTER(FpfhParams)]),
    ("gloc_scan_store_build_fpfh", _i, [_vp, _u32, _u32, _u32]),
    ("gloc_scan_store_fpfh", _i, [_vp, _u32, _vp, _sz]),
    ("gloc_scan_store_spfh", _i, [_vp, _u32, _u32, _vp, _vp, _sz]),
    ("gloc_reg_fpfh_match", _i, [_vp, _vp, _sz, _vp, _sz, _u32, _vp, _vp]),
    ("gloc_reg_fpfh_batch_ids", _i, [_vp, _u32, _vp, _sz, _vp, C.POINTER(FpfhParams), _vp, _vp, _vp, _vp]),
    ("gloc_fpfh_graph_default_params", None, [C.POINTER(FpfhGraphParams)]),
    ("gloc_reg_fpfh_graph_batch_ids", _i, [_vp, _u32, _vp, _sz, C.POINTER(FpfhGraphParams), _vp, _vp, _vp, _vp]),
    ("gloc_reg_pair_graph", _i, [_vp, _vp, _vp, _sz, C.POINTER(FpfhGraphParams), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("gloc_fpfh_radius_default_params", None, [C.POINTER(FpfhRadiusParams)]),
    ("gloc_scan_store_radius_neighbors", _i, [_vp, _u32, C.c_float, _u32, _vp, _vp, _vp, _sz]),
    ("gloc_scan_store_build_normals_radius", _i, [_vp, _u32, C.c_float, _u32, _u32]),
    ("gloc_scan_store_build_fpfh_radius", _i, [_vp, _u32, C.POINTER(FpfhRadiusParams)]),
    ("gloc_scan_store_spfh_radius", _i, [_vp, _u32, C.c_float, _u32, _vp, _vp, _sz]),
    ("gloc_reg_fpfh_batch_ids_radius", _i, [_vp, _u32, _vp, _sz, _vp, C.POINTER(FpfhParams), C.POINTER(FpfhRadiusParams), _vp, _vp, _vp, _vp]),
    ("gloc_reg_fpfh_graph_batch_ids_radius", _i, [_vp, _u32, _vp, _sz, C.POINTER(FpfhGraphParams), C.POINTER(FpfhRadiusParams), _vp, _vp, _vp, _vp]),
    ("gloc_iss_default_params", None, [C.POINTER(IssParams)]),
    ("gloc_scan_store_iss_saliency", _i, [_vp, _u32, C.POINTER(IssParams), _vp, _vp, _sz]),
    ("gloc_scan_store_build_keypoints", _i, [_vp, _u32, C.POINTER(IssParams)]),
    ("gloc_scan_store_keypoint_count", _i, [_vp, _u32, C.POINTER(C.c_size_t)]),
    ("gloc_scan_store_keypoints", _i, [_vp, _u32, _vp, _sz]),
    ("gloc_scan_store_keypoint_fpfh", _i, [_vp, _u32, _vp, _sz]),
    ("gloc_reg_fpfh_batch_ids_keypoints", _i, [_vp, _u32, _vp, _sz, _vp, C.POINTER(FpfhParams), C.POINTER(FpfhRadiusParams), C.POINTER(IssParams),
                                           _vp, _vp, _vp, _vp]),
    ("gloc_reg_fpfh_graph_batch_ids_keypoints", _i, [_vp, _u32, _vp, _sz, C.POINTER(FpfhGraphParams), C.POINTER(FpfhRadiusParams),
                                                 C.POINTER(IssParams), _vp, _vp, _vp, _vp]),
    ("gloc_cluster_default_params", None, [C.POINTER(ClusterParams)]),
    ("gloc_scan_store_cluster", _i, [_vp, _u32, C.POINTER(ClusterParams), _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    ("gloc_scan_filter_default_params", None, [C.POINTER(ScanFilterParams)]),
    ("gloc_scan_store_add_filtered", _i, [_vp, _u32, C.POINTER(ScanFilterParams), _vp, _vp]),
    ("gloc_scan_store_add_subset", _i, [_vp, _u32, _vp, _sz, _vp]),
    ("gloc_fgr_default_params", None, [C.POINTER(FgrParams)]),
    ("gloc_reg_fpfh_fgr_batch_ids", _i, [_vp, _u32, _vp, _sz, _vp, C.POINTER(FgrParams), _vp, _vp, _vp, _vp]),
    ("gloc_reg_fpfh_fgr_batch_ids_radius", _i, [_vp, _u32, _vp, _sz, _vp, C.POINTER(FgrParams), C.POINTER(FpfhRadiusParams), _vp, _vp, _vp, _vp]),
    ("gloc_reg_fpfh_fgr_batch_ids_keypoints", _i, [_vp, _u32, _vp, _sz, _vp, C.POINTER(FgrParams), C.POINTER(FpfhRadiusParams),
                                               C.POINTER(IssParams), _vp, _vp, _vp, _vp]),
    ("gloc_reg_fgr_pairs", _i, [_vp, _vp, _vp, _sz, _u32, C.POINTER(FgrParams), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("gloc_reg_p2l_pairs_system", _i, [_vp, _vp, _vp, _sz, _vp, C.POINTER(P2lParams), C.POINTER(RobustParams), _u32, _vp, _vp, _vp, _vp, _vp]),
    ("gloc_reg_gicp_pairs_system", _i, [_vp, _vp, _vp, _sz, _vp, C.POINTER(GicpParams), C.POINTER(RobustParams), _u32, _vp, _vp, _vp, _vp, _vp]),
    ("gloc_reg_vgicp_pairs_system", _i, [_vp, _vp, _vp, _sz, _vp, C.POINTER(VgicpParams), C.POINTER(RobustParams), _u32, _vp, _vp, _vp, _vp, _vp]),
    ("gloc_vmap_default_params", None, [C.POINTER(VmapParams)]),
    ("gloc_reg_vmap_create", _i, [_vp, C.POINTER(VmapParams), C.POINTER(_u32)]),
    ("gloc_reg_vmap_destroy", _i, [_vp, _u32]),
    ("gloc_reg_vmap_insert", _i, [_vp, _u32, _vp, _sz, _vp]),
    ("gloc_reg_vmap_prune", _i, [_vp, _u32, _vp, C.c_float, _u32, C.POINTER(_u32)]),
    ("gloc_reg_vmap_info", _i, [_vp, _u32, C.POINTER(VmapInfo)]),
    ("gloc_reg_vmap_voxels", _i, [_vp, _u32, _sz, _vp, _vp, _vp, _vp, _vp, C.POINTER(_sz)]),
    ("gloc_reg_vgicp_vmap", _i, [_vp, _vp, _vp, _sz, _vp, C.POINTER(VgicpParams), C.POINTER(RobustParams), _vp, _vp, _vp, _vp, _vp]),
    ("gloc_reg_vgicp_vmap_system", _i, [_vp, _vp, _vp, _sz, _vp, C.POINTER(VgicpParams), C.POINTER(RobustParams), _u32, _vp, _vp, _vp, _vp, _vp]),
    ("gloc_eval_default_params", None, [C.POINTER(EvalParams)]),
    ("gloc_reg_evaluate_pairs", _i, [_vp, _vp, _vp, _sz, _vp, C.POINTER(EvalParams), _vp, _vp, _vp, _vp, _vp]),
    ("gloc_reg_ndt_batch_ids", _i, [_vp, _u32, _vp, _sz, _vp, C.POINTER(NdtParams), _vp, _vp, _vp, _vp]),
    ("gloc_reg_ndt_derivatives", _i, [_vp, _u32, _u32, _vp, C.POINTER(NdtParams), _vp, _vp, _vp]),
    ("gloc_reg_ndt_cells", _i, [_vp, _u32, C.POINTER(NdtParams), _sz, _vp, _vp, _vp, _vp, C.POINTER(_sz)]),
    ("gloc_scan_store_add_approx_voxel", _i, [_vp, _u32, C.c_float, C.POINTER(_u32)]),
    ("gloc_submap_default_params", None, [C.POINTER(SubmapParams)]),
    ("gloc_scan_store_add_submap", _i, [_vp, _vp, _vp, _sz, C.POINTER(SubmapParams), C.POINTER(_u32), _vp]),
    ("gloc_scan_store_add_submaps", _i, [_vp, _vp, _vp, _vp, _sz, C.POINTER(SubmapParams), _vp, _vp]),
    ("gloc_reg_scan_add_submaps", _i, [_vp, _vp, _vp, _vp, _sz, C.POINTER(SubmapParams), _vp, _vp]),
    ("gloc_vlad_create", _i, [_i, _sz, _sz, _sz, _vp, _vp, _vp, _vp, _i, C.POINTER(_vp)]),
    ("gloc_vlad_set_gating", _i, [_vp, _vp, _vp, _vp]),
    ("gloc_vlad_destroy", _i, [_vp]),
    ("gloc_vlad_set_stream", _i, [_vp, _vp]),
    ("gloc_vlad_forward", _i, [_vp, _vp, _sz, _sz, _vp]),
    ("gloc_vlad_forward_device", _i, [_vp, _vp, _sz, _sz, _vp]),
    ("gloc_vlad_set_profile", _i, [_vp, _i]),
    ("gloc_vlad_profile", _i, [_vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(_u64)]),
    ("gloc_bev_default_params", _i, [_vp]),
    ("gloc_bev_create", _i, [_i, C.POINTER(_vp)]),
    ("gloc_bev_destroy", _i, [_vp]),
    ("gloc_bev_set_stream", _i, [_vp, _vp]),
    ("gloc_bev_synchronize", _i, [_vp]),
    ("gloc_bev_project", _i, [_vp, _vp, _sz, _sz, _vp, _vp, _vp]),
    ("gloc_bev_project_batch_device", _i, [_vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp]),
    ("gloc_bev_raw_image", _i, [_vp, _sz, _vp, _sz]),
    ("gloc_bev_set_profile", _i, [_vp, _i]),
    ("gloc_bev_profile", _i, [_vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(_u64)]),
    ("gloc_bev_device_flags", _i, [_vp, _sz, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_i)]),
    ("gloc_pillar_default_params", _i, [C.POINTER(PillarParams)]),
    ("gloc_pillar_create", _i, [_i, C.POINTER(_vp)]),
    ("gloc_pillar_destroy", _i, [_vp]),
    ("gloc_pillar_set_stream", _i, [_vp, _vp]),
    ("gloc_pillar_synchronize", _i, [_vp]),
    ("gloc_pillar_set_pointnet", _i, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_float]),
    ("gloc_pillar_inputs", _i, [_vp, _vp, _vp, _sz, _sz, C.POINTER(PillarParams), _vp]),
    ("gloc_pillar_inputs_device", _i, [_vp, _vp, _vp, _sz, _sz, C.POINTER(PillarParams), _vp]),
    ("gloc_pillar_canvas", _i, [_vp, _vp, _vp, _sz, _sz, C.POINTER(PillarParams), _vp]),
    ("gloc_pillar_canvas_device", _i, [_vp, _vp, _vp, _sz, _sz, C.POINTER(PillarParams), _vp]),
    ("gloc_pillar_backbone_layer_shape", _i, [_i, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_i), C.POINTER(_i)]),
    ("gloc_pillar_set_backbone_layer", _i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, C.c_float]),
    ("gloc_pillar_backbone_device", _i, [_vp, _vp, _sz, _u32, _u32, _vp]),
    ("gloc_pillar_backbone_layer_device", _i, [_vp, _i, _vp, _sz, _u32, _u32, _vp]),
    ("gloc_pillar_upsample_device", _i, [_vp, _vp, _sz, _u32, _u32, _u32, _u32, _vp]),
    ("gloc_pillar_features", _i, [_vp, _vp, _vp, _sz, _sz, C.POINTER(PillarParams), _vp]),
    ("gloc_pillar_features_device", _i, [_vp, _vp, _vp, _sz, _sz, C.POINTER(PillarParams), _vp]),
    ("gloc_pillar_set_profile", _i, [_vp, _i]),
    ("gloc_pillar_profile", _i, [_vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(_u64)]),
    ("gloc_pillar_profile_reset", _i, [_vp]),
    ("gloc_vgg_create", _i, [_i, C.POINTER(_vp)]),
    ("gloc_vgg_destroy", _i, [_vp]),
    ("gloc_vgg_set_stream", _i, [_vp, _vp]),
    ("gloc_vgg_synchronize", _i, [_vp]),
    ("gloc_vgg_layer_shape", _i, [_i, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_i), C.POINTER(_i)]),
    ("gloc_vgg_set_layer", _i, [_vp, _i, _vp, _vp]),
    ("gloc_vgg_forward", _i, [_vp, _vp, _sz, _u32, _u32, _vp]),
    ("gloc_vgg_forward_device", _i, [_vp, _vp, _sz, _u32, _u32, _vp]),
    ("gloc_vgg_forward_layer", _i, [_vp, _i, _vp, _sz, _u32, _u32, _vp]),
    ("gloc_vgg_set_profile", _i, [_vp, _i]),
    ("gloc_vgg_profile", _i, [_vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(_u64)]),
    ("gloc_vgg_profile_reset", _i, [_vp]),
    ("gloc_coarse_default_params", _i, [_vp]),
    ("gloc_coarse_create", _i, [_i, C.POINTER(_vp)]),
    ("gloc_coarse_destroy", _i, [_vp]),
    ("gloc_coarse_add_image", _i, [_vp, _vp, _u32, _u32, C.c_float, C.c_float, C.c_float, _vp, C.POINTER(_u32)]),
    ("gloc_coarse_add_scan", _i, [_vp, _vp, _sz, _sz, _vp, C.POINTER(_u32)]),
    ("gloc_coarse_add_store_scan", _i, [_vp, _vp, _u32, _vp, C.POINTER(_u32)]),
    ("gloc_coarse_add_store_scans", _i, [_vp, _vp, _vp, _sz, _vp, _vp]),
    ("gloc_coarse_match_pairs", _i, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    ("gloc_coarse_release", _i, [_vp, _u32]),
    ("gloc_coarse_cells", _i, [_vp, _u32, C.POINTER(_u32), _vp, _sz]),
    ("gloc_coarse_match", _i, [_vp, _u32, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    ("gloc_pgo_default_params", None, [C.POINTER(PgoParams)]),
    ("gloc_pgo_create", _i, [_i, C.POINTER(_vp)]),
    ("gloc_pgo_destroy", _i, [_vp]),
    ("gloc_pgo_set_stream", _i, [_vp, _vp]),
    ("gloc_pgo_synchronize", _i, [_vp]),
    ("gloc_pgo_set_profile", _i, [_vp, _i]),
    ("gloc_pgo_profile", _i, [_vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(_u64)]),
    ("gloc_pgo_profile_reset", _i, [_vp]),
    ("gloc_pgo_linearize", _i, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz, C.POINTER(PgoParams), C.POINTER(RobustParams),
                            _vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_double)]),
    ("gloc_pgo_optimize", _i, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz, C.POINTER(PgoParams), C.POINTER(RobustParams),
                           _vp, _vp, _vp, C.POINTER(PgoResult)]),
    ("gloc_pgo_consistency_default_params", None, [C.POINTER(PgoConsistencyParams)]),
    ("gloc_pgo_consistency", _i, [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz, C.POINTER(PgoConsistencyParams),
                              _vp, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32), _vp, _vp, _vp, _vp, _vp, _vp]),
    ("gloc_sc_default_params", _i, [C.POINTER(ScParams)]),
    ("gloc_sc_create", _i, [_i, C.POINTER(ScParams), C.POINTER(_vp)]),
    ("gloc_sc_destroy", _i, [_vp]),
    ("gloc_sc_set_stream", _i, [_vp, _vp]),
    ("gloc_sc_synchronize", _i, [_vp]),
    ("gloc_sc_describe", _i, [_vp, _vp, _sz, _sz, _vp]),
    ("gloc_sc_describe_store_scans", _i, [_vp, _vp, _vp, _sz, _vp]),
    ("gloc_sc_add", _i, [_vp, _vp, _sz]),
    ("gloc_sc_add_scan", _i, [_vp, _vp, _sz, _sz, C.POINTER(_u64)]),
    ("gloc_sc_add_store_scans", _i, [_vp, _vp, _vp, _sz, C.POINTER(_u64)]),
    ("gloc_sc_size", _i, [_vp, C.POINTER(_sz)]),
    ("gloc_sc_clear", _i, [_vp]),
    ("gloc_sc_reserve", _i, [_vp, _sz]),
    ("gloc_sc_rows", _i, [_vp, _sz, _sz, _vp]),
    ("gloc_sc_ring_keys", _i, [_vp, _sz, _sz, _vp]),
    ("gloc_sc_save", _i, [_vp, C.c_char_p]),
    ("gloc_sc_load", _i, [_vp, C.c_char_p]),
    ("gloc_sc_search", _i, [_vp, _vp, _sz, _sz, _sz, _sz, _vp, _vp, _vp]),
    ("gloc_sc_search_store_scans", _i, [_vp, _vp, _vp, _sz, _sz, _sz, _sz, _vp, _vp, _vp]),
    ("gloc_sc_distances", _i, [_vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    ("gloc_sc_shift_to_yaw", _i, [C.POINTER(ScParams), _u32, C.POINTER(C.c_float)]),
    ("gloc_sc_set_profile", _i, [_vp, _i]),
    ("gloc_sc_profile", _i, [_vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(_u64)]),
    ("gloc_sc_profile_reset", _i, [_vp]),
    ("gloc_m2dp_default_params", _i, [C.POINTER(M2dpParams)]),
    ("gloc_m2dp_dim", _i, [C.POINTER(M2dpParams), C.POINTER(_sz)]),
    ("gloc_m2dp_create", _i, [_i, C.POINTER(M2dpParams), C.POINTER(_vp)]),
    ("gloc_m2dp_destroy", _i, [_vp]),
    ("gloc_m2dp_set_stream", _i, [_vp, _vp]),
    ("gloc_m2dp_synchronize", _i, [_vp]),
    ("gloc_m2dp_describe", _i, [_vp, _vp, _sz, _sz, _vp, _vp, _vp]),
    ("gloc_m2dp_describe_store_scans", _i, [_vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    ("gloc_m2dp_describe_store_scans_device", _i, [_vp, _vp, _vp, _sz, _vp]),
    ("gloc_m2dp_signature_svd", _i, [_vp, _vp, _vp, _sz, _vp, _vp]),
    ("gloc_m2dp_frame_to_seed", _i, [_vp, _vp, _vp]),
    ("gloc_m2dp_set_profile", _i, [_vp, _i]),
    ("gloc_m2dp_profile", _i, [_vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(_u64)]),
    ("gloc_m2dp_profile_reset", _i, [_vp]),
    ("gloc_ground_default_params", _i, [_vp]),
    ("gloc_ground_create", _i, [_i, C.POINTER(_vp)]),
    ("gloc_ground_destroy", _i, [_vp]),
    ("gloc_ground_set_stream", _i, [_vp, _vp]),
    ("gloc_ground_set_option", _i, [_vp, _i, C.c_int64]),
    ("gloc_ground_estimate", _i, [_vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp]),
    ("gloc_ground_estimate_device", _i, [_vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp]),
    ("gloc_ground_knn", _i, [_vp, _vp, _sz, _u32, _vp, _vp]),
    ("gloc_ground_normals", _i, [_vp, _vp, _sz, _u32, _vp, _vp]),
    ("gloc_ground_transform_from_plane", _i, [_vp, _vp]),
    ("gloc_ground_set_profile", _i, [_vp, _i]),
    ("gloc_ground_profile", _i, [_vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(_u64)]),
    ("gloc_knn_add_synthetic", _i, [_vp, _i, _u64, _u64, _sz, _u64]),
    ("gloc_synth_fill_device", _i, [_i, _vp, _i, _u64, _u64, _sz, _sz, _u64, _vp]),
]
EXPORTED_SYMBOLS = [p[0] for p in _PROTOS]

_lib = None


def _preload_hip_runtime():
    """libgloc3d.so carries no NEEDED entry for the HIP runtime: exactly one must be in the process.
    PyTorch bundles its own libamdhip64; when torch is installed we run on that copy so that torch
    tensors, torch.distributed (RCCL) and our kernels share one runtime.  GLOC3D_HIP_RUNTIME
    overrides the choice."""
    cands = []
    if os.environ.get("GLOC3D_HIP_RUNTIME"):
        cands.append(os.environ["GLOC3D_HIP_RUNTIME"])
    try:
        import torch  # noqa: F401  (loads its bundled runtime)
        cands.append(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    except ImportError:
        pass
    cands += ["/opt/rocm/lib/libamdhip64.so", "libamdhip64.so"]
    for p in cands:
        try:
            C.CDLL(p, mode=C.RTLD_GLOBAL)
            return p
        except OSError:
            continue
    raise RuntimeError("no HIP runtime (libamdhip64.so) found: " + ", ".join(cands))


def lib():
    """Load libgloc3d.so (no compute; safe without a GPU).  Raises if it was never built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build the HIP extension first "
                "(python -m gloc3d_amd.build or __graft_entry__.build()); there is no CPU fallback")
        _preload_hip_runtime()
        L = C.CDLL(LIB_PATH)
        for name, res, args in _PROTOS:
            fn = getattr(L, name)  # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != GLOC_OK:
        raise GlocError(rc, lib().gloc_last_error().decode("utf-8", "replace"))


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class _Handle:
    """A C handle of prefix gloc_<_C>_: close() destroys it once (GlocError if the library refuses: live views, attached
    handles) and garbage collection tries the same.  The plumbing entry points every module forwards to one shared
    implementation are wrapped once below; a class takes the ones its part of the C ABI has."""
    _C = None

    def _fn(self, name):
        return getattr(lib(), f"gloc_{self._C}_{name}")

    def close(self):
        if self._h:
            check(self._fn("destroy")(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _set_stream(self, stream_ptr):
    check(self._fn("set_stream")(self._h, C.c_void_p(stream_ptr or 0)))


def _synchronize(self):
    check(self._fn("synchronize")(self._h))


def _set_profile(self, on=True):
    check(self._fn("set_profile")(self._h, 1 if on else 0))


def _profile(self, kernel):
    ms, n = C.c_double(), C.c_uint64()
    check(self._fn("profile")(self._h, kernel.encode(), C.byref(ms), C.byref(n)))
    return ms.value, n.value


def _profile_reset(self):
    check(self._fn("profile_reset")(self._h))


class KnnIndex(_Handle):
    """Resident descriptor database + exact L2 top-k (the reference's InvKeyTree / IndexFlatL2)."""

    _C = "knn"
    synchronize, profile, profile_reset = _synchronize, _profile, _profile_reset

    def __init__(self, dim, device=0):
        self._h = C.c_void_p()
        self.dim = int(dim)
        self.device = device
        check(lib().gloc_knn_create(device, self.dim, C.byref(self._h)))

    def close(self):
        _Handle.close(self)
        self._parent = None

    def view(self):
        """A second search handle over this index's rows (gloc_knn_create_view): own stream and workspace, so that a search
        on it runs beside a search on this handle.  Close it before its parent."""
        v = KnnIndex.__new__(KnnIndex)
        v._h = C.c_void_p()
        v.dim, v.device = self.dim, self.device
        check(lib().gloc_knn_create_view(self._h, C.byref(v._h)))
        v._parent = self          # (keeps the parent alive as long as the view)
        return v

    def __len__(self):
        n = C.c_size_t()
        check(lib().gloc_knn_size(self._h, C.byref(n)))
        return n.value

    def set_option(self, option, value):
        check(lib().gloc_knn_set_option(self._h, option, int(value)))

    def set_stream(self, hip_stream):
        _set_stream(self, hip_stream)

    def reserve(self, n):
        check(lib().gloc_knn_reserve(self._h, n))

    def clear(self):
        check(lib().gloc_knn_clear(self._h))

    def add(self, rows):
        rows = np.ascontiguousarray(rows, np.float32).reshape(-1, self.dim)
        check(lib().gloc_knn_add(self._h, _np_ptr(rows), rows.shape[0]))

    def add_device(self, dev_ptr, n):
        check(lib().gloc_knn_add_device(self._h, C.c_void_p(dev_ptr), n))

    def add_synthetic(self, kind, seed, first_row, n, row_stride=1):
        check(lib().gloc_knn_add_synthetic(self._h, kind, seed, first_row, n, row_stride))

    def save(self, path):
        check(lib().gloc_knn_save(self._h, str(path).encode()))

    def load(self, path):
        check(lib().gloc_knn_load(self._h, str(path).encode()))

    def device_rows(self):
        p = C.c_void_p()
        check(lib().gloc_knn_device_rows(self._h, C.byref(p)))
        return p.value

    def search(self, queries, k, first_row=0, last_row=None):
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, self.dim)
        nq = q.shape[0]
        idx = np.empty((nq, k), np.uint64)
        d2 = np.empty((nq, k), np.float32)
        last = SIZE_MAX if last_row is None else last_row
        check(lib().gloc_knn_search(self._h, _np_ptr(q), nq, k, first_row, last, _np_ptr(idx),
                                    _np_ptr(d2)))
        return idx, d2

    def search_device(self, q_ptr, nq, k, idx_ptr, d2_ptr, first_row=0, last_row=None,
                      index_offset=0):
        last = SIZE_MAX if last_row is None else last_row
        check(lib().gloc_knn_search_device(self._h, C.c_void_p(q_ptr), nq, k, first_row, last,
                                           index_offset, C.c_void_p(idx_ptr), C.c_void_p(d2_ptr)))

    def search_sharded(self, comm, q_ptr, nq, k, idx_ptr, d2_ptr, index_stride=1, index_offset=0):
        """Collective: top-k over the whole row-sharded database (RCCL all-gather + merge on the device)."""
        check(lib().gloc_knn_search_sharded(self._h, comm._h, C.c_void_p(q_ptr), nq, k, index_stride, index_offset,
                                            C.c_void_p(idx_ptr), C.c_void_p(d2_ptr)))

    def stats(self):
        s = KnnStats()
        check(lib().gloc_knn_get_stats(self._h, C.byref(s)))
        return {f[0]: getattr(s, f[0]) for f in KnnStats._fields_}


class Comm(_Handle):
    """RCCL communicator of this process's GPU (gloc_comm_*).  `exchange(id_bytes or None) -> id_bytes`
    broadcasts rank 0's 128-byte id to every rank (e.g. over torch.distributed or a shared file)."""

    _C = "comm"

    def __init__(self, device, rank, world, exchange):
        uid = (C.c_uint8 * 128)()
        err = None
        if rank == 0:
            try:
                check(lib().gloc_comm_unique_id(uid))
            except Exception as e:      # the other ranks are waiting in exchange(): hand them a null id, then fail
                err, uid = e, (C.c_uint8 * 128)()
        data = exchange(bytes(uid) if rank == 0 else None)
        if err is not None:
            raise err
        assert len(data) == 128
        if not any(data):
            raise GlocError(5, "rank 0 could not create the RCCL id")
        uid = (C.c_uint8 * 128).from_buffer_copy(data)
        self._h = C.c_void_p()
        self.rank, self.world = rank, world
        check(lib().gloc_comm_create(device, rank, world, uid, C.byref(self._h)))

    def rank_world(self):
        """(rank, world) as the communicator itself reports them (gloc_comm_rank)."""
        r, w = C.c_int(), C.c_int()
        check(lib().gloc_comm_rank(self._h, C.byref(r), C.byref(w)))
        return r.value, w.value

    def all_gather_device(self, send_ptr, recv_ptr, bytes_per_rank, stream=0):
        check(lib().gloc_comm_all_gather_device(self._h, C.c_void_p(send_ptr), C.c_void_p(recv_ptr), bytes_per_rank,
                                                C.c_void_p(stream or 0)))


def topk_merge_device(device, stream, idx_ptr, d2_ptr, n_lists, nq, k, out_idx_ptr, out_d2_ptr):
    check(lib().gloc_topk_merge_device(device, C.c_void_p(stream or 0), C.c_void_p(idx_ptr),
                                       C.c_void_p(d2_ptr), n_lists, nq, k,
                                       C.c_void_p(out_idx_ptr), C.c_void_p(out_d2_ptr)))


def synth_fill_device(device, stream, kind, seed, first_row, n, dim, out_ptr, row_stride=1):
    check(lib().gloc_synth_fill_device(device, C.c_void_p(stream or 0), kind, seed, first_row, n,
                                       dim, row_stride, C.c_void_p(out_ptr)))


def default_reg_params(**over):
    p = RegParams()
    lib().gloc_reg_default_params(C.byref(p))
    if os.environ.get("GLOC3D_MAX_FINAL_STEP"):          # developer override of the convergence check's threshold
        p.max_final_step = float(os.environ["GLOC3D_MAX_FINAL_STEP"])
    for k_, v in over.items():
        setattr(p, k_, v)
    return p


def default_ndt_params(**over):
    """gloc_ndt_params with the reference's constants (ndt_match_3d) and PCL's defaults for the rest, then `over`."""
    p = NdtParams()
    lib().gloc_ndt_default_params(C.byref(p))
    for k_, v in over.items():
        setattr(p, k_, v)
    return p


def default_submap_params(**over):
    """gloc_submap_params as gloc_submap_default_params leaves them (leaf 0.2 m, every occupied cell kept, no range limit),
    then `over`."""
    p = SubmapParams()
    lib().gloc_submap_default_params(C.byref(p))
    for k_, v in over.items():
        setattr(p, k_, v)
    return p


def _submap_args(submaps):
    """[(member ids, poses [n, 4, 4])] -> the flat arrays of gloc_scan_store_add_submaps: ids, poses [sum n, 16], first."""
    ids = [np.ascontiguousarray(m[0], np.uint32).reshape(-1) for m in submaps]
    Ts = [np.ascontiguousarray(m[1], np.float32).reshape(-1, 16) for m in submaps]
    for i, t in zip(ids, Ts):
        if i.shape[0] != t.shape[0]:
            raise ValueError(f"{i.shape[0]} member ids but {t.shape[0]} poses")
    first = np.zeros(len(submaps) + 1, np.uint32)
    first[1:] = np.cumsum([i.shape[0] for i in ids])
    cat_i = np.ascontiguousarray(np.concatenate(ids + [np.zeros(0, np.uint32)]))
    cat_T = np.ascontiguousarray(np.concatenate(Ts + [np.zeros((0, 16), np.float32)]))
    return cat_i, cat_T, first


def _add_submaps(fn, handle, submaps, params, want_info):
    ids, T, first = _submap_args(submaps)
    n = len(submaps)
    prm = params or default_submap_params()
    new = np.empty(n, np.uint32)
    info = (SubmapInfo * max(n, 1))()
    check(fn(handle, _np_ptr(ids), _np_ptr(T), _np_ptr(first), n, C.byref(prm), _np_ptr(new), C.cast(info, C.c_void_p)))
    out = [int(i) for i in new]
    return (out, [info[i].as_dict() for i in range(n)]) if want_info else out


def default_p2l_params(**over):
    """gloc_p2l_params as gloc_p2l_default_params leaves them (30 passes, no rejection, no early stop, k = 10), then `over`."""
    p = P2lParams()
    lib().gloc_p2l_default_params(C.byref(p))
    for k_, v in over.items():
        setattr(p, k_, v)
    return p


def default_gicp_params(**over):
    """gloc_gicp_params as gloc_gicp_default_params leaves them (30 passes, no rejection, no early stop, k = 10,
    plane_eps = 1e-3), then `over`."""
    p = GicpParams()
    lib().gloc_gicp_default_params(C.byref(p))
    for k_, v in over.items():
        setattr(p, k_, v)
    return p


def default_vgicp_params(**over):
    """gloc_vgicp_params as gloc_vgicp_default_params leaves them (generalized ICP's, 1 m voxels, 7 neighbours, voxels of
    one point and more), then `over`."""
    p = VgicpParams()
    lib().gloc_vgicp_default_params(C.byref(p))
    for k_, v in over.items():
        setattr(p, k_, v)
    return p


def default_vmap_params(**over):
    """gloc_vmap_params as gloc_vmap_default_params leaves them (1 m voxels, 2^18 of them, normal_k 10), then `over`."""
    p = VmapParams()
    lib().gloc_vmap_default_params(C.byref(p))
    for k_, v in over.items():
        setattr(p, k_, v)
    return p


def default_robust_params(**over):
    """gloc_robust_params as gloc_robust_default_params leaves them (kind NONE, zeros), then `over`."""
    p = RobustParams()
    lib().gloc_robust_default_params(C.byref(p))
    for k_, v in over.items():
        setattr(p, k_, v)
    return p


def robust_scale(robust, k):
    """c(k) of the block's schedule, as the device uses it (gloc_robust_scale)."""
    c = C.c_double()
    check(lib().gloc_robust_scale(C.byref(robust), int(k), C.byref(c)))
    return c.value


def robust_weight(robust, k, s2):
    """The weight of a squared residual s2 at c(k), as the device computes it (gloc_robust_weight)."""
    w = C.c_double()
    check(lib().gloc_robust_weight(C.byref(robust), int(k), float(s2), C.byref(w)))
    return w.value


def default_fpfh_params(**over):
    """gloc_fpfh_params as gloc_fpfh_default_params leaves them (normal_k = 10, feature_k = 16, mutual matches, 3000
    hypotheses at most, 0.6 m inliers, confidence 0.99, seed 1234), then `over`."""
    p = FpfhParams()
    lib().gloc_fpfh_default_params(C.byref(p))
    for k_, v in over.items():
        setattr(p, k_, v)
    return p


def default_fpfh_graph_params(**over):
    """gloc_fpfh_graph_params as gloc_fpfh_graph_default_params leaves them (normal_k = 10, feature_k = 16, mutual matches,
    64 seeds, 0.6 m compatibility and inlier thresholds, theta = 1 / 2), then `over`."""
    p = FpfhGraphParams()
    lib().gloc_fpfh_graph_default_params(C.byref(p))
    for k_, v in over.items():
        setattr(p, k_, v)
    return p


def default_fgr_params(**over):
    """gloc_fgr_params as gloc_fgr_default_params leaves them (normal_k = 10, feature_k = 16, mutual matches, 10 000 tuple
    tries of which the first 1000 passing at scale 0.9 are kept, 64 updates, mu divided by 1.4 every 4, 0.6 m match distance
    and inlier threshold, seed 1234), then `over`."""
    p = FgrParams()
    lib().gloc_fgr_default_params(C.byref(p))
    for k_, v in over.items():
        setattr(p, k_, v)
    return p


def default_eval_params(**over):
    """gloc_eval_params as gloc_eval_default_params leaves them (0.6 m correspondence distance), then `over`."""
    p = EvalParams()
    lib().gloc_eval_default_params(C.byref(p))
    for k_, v in over.items():
        setattr(p, k_, v)
    return p


def default_fpfh_radius_params(**over):
    """gloc_fpfh_radius_params as gloc_fpfh_radius_default_params leaves them (normals from 30 neighbours within 1.0 m, at
    least 5; features from 100 within 2.5 m), then `over`."""
    p = FpfhRadiusParams()
    lib().gloc_fpfh_radius_default_params(C.byref(p))
    for k_, v in over.items():
        setattr(p, k_, v)
    return p


def default_iss_params(**over):
    """gloc_iss_params as gloc_iss_default_params leaves them (saliency from 128 neighbours within 3.0 m, at least 5;
    suppression within 2.0 m; both eigenvalue ratios below 0.975), then `over`."""
    p = IssParams()
    lib().gloc_iss_default_params(C.byref(p))
    for k_, v in over.items():
        setattr(p, k_, v)
    return p


def default_cluster_params(**over):
    """gloc_cluster_params as gloc_cluster_default_params leaves them (tolerance 0.5 m, min_size 1, no max_size), then `over`."""
    p = ClusterParams()
    lib().gloc_cluster_default_params(C.byref(p))
    for k_, v in over.items():
        setattr(p, k_, v)
    return p


def default_scan_filter_params(**over):
    """gloc_scan_filter_params as gloc_scan_filter_default_params leaves them -- every stage off --, then `over`; a key
    cluster_<field> sets that field of the cluster block (cluster_tolerance = 0.5 switches the cluster stage on)."""
    p = ScanFilterParams()
    lib().gloc_scan_filter_default_params(C.byref(p))
    for k_, v in over.items():
        if k_.startswith("cluster_"):
            setattr(p.cluster, k_[len("cluster_"):], v)
        else:
            setattr(p, k_, v)
    return p


class ScanStore(_Handle):
    """Resident scans + their search index, shared by any number of Registrars."""

    _C = "scan_store"

    def __init__(self, device=0):
        self._h = C.c_void_p()
        self.device = device
        check(lib().gloc_scan_store_create(device, C.byref(self._h)))

    def add(self, pts):
        pts = np.ascontiguousarray(pts, np.float32)
        assert pts.ndim == 2 and 3 <= pts.shape[1] <= 16
        sid = C.c_uint32()
        check(lib().gloc_scan_store_add(self._h, _np_ptr(pts), pts.shape[0], pts.shape[1], C.byref(sid)))
        return sid.value

    def add_device(self, dev_ptr, n, stride_floats=3):
        sid = C.c_uint32()
        check(lib().gloc_scan_store_add_device(self._h, C.c_void_p(dev_ptr), n, stride_floats, C.byref(sid)))
        return sid.value

    def add_variant(self, base_id, T=None, noise_sigma=0.0, seed=0):
        Tp = None if T is None else np.ascontiguousarray(T, np.float32).reshape(16)
        sid = C.c_uint32()
        check(lib().gloc_scan_store_add_variant(self._h, int(base_id), None if Tp is None else _np_ptr(Tp),
                                                float(noise_sigma), int(seed), C.byref(sid)))
        return sid.value

    def add_raycast(self, world, poses, seeds, n_beams=64, n_az=2000, max_range=80.0, noise=0.02, fov=(-24.8, 2.0),
                    reach_margin=1.0):
        """Ray-cast len(poses) scans on the device (gloc_scan_store_add_raycast_batch; the device twin of
        synth.lidar_scan): world = dict(lo [n,3], hi [n,3], ground), poses = world <- sensor 4x4 matrices.  Every pose is
        given the boxes whose footprint comes within max_range (+ margin) of it.  Returns the scan ids."""
        poses = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 4, 4))
        lo, hi = np.asarray(world["lo"], np.float64).reshape(-1, 3), np.asarray(world["hi"], np.float64).reshape(-1, 3)
        ids = []
        for a in range(0, len(poses), 64):
            P = poses[a:a + 64]
            o = P[:, :2, 3]                                              # [k, 2]
            gap = np.maximum(np.maximum(lo[None, :, :2] - o[:, None, :], o[:, None, :] - hi[None, :, :2]), 0.0)
            near = np.hypot(gap[..., 0], gap[..., 1]) <= max_range + reach_margin        # [k, n_boxes]
            first = np.zeros(len(P) + 1, np.uint32)
            first[1:] = np.cumsum(near.sum(axis=1))
            sel = [np.nonzero(near[i])[0] for i in range(len(P))]
            cat = np.concatenate(sel) if sel else np.zeros(0, np.int64)
            blo, bhi = np.ascontiguousarray(lo[cat]), np.ascontiguousarray(hi[cat])
            prm = RaycastParams(int(n_beams), int(n_az), float(max_range), float(noise), float(fov[0]), float(fov[1]))
            sd = np.ascontiguousarray(np.asarray(seeds[a:a + 64], np.uint64))
            out = np.empty(len(P), np.uint32)
            check(lib().gloc_scan_store_add_raycast_batch(self._h, len(P), _np_ptr(blo) if len(cat) else None,
                                                          _np_ptr(bhi) if len(cat) else None, _np_ptr(first), float(world["ground"]),
                                                          _np_ptr(P), _np_ptr(sd), C.byref(prm), _np_ptr(out)))
            ids.extend(int(i) for i in out)
        return ids

    def add_batch(self, scans):
        """Several scans ([n_i, c] float32 arrays with the same number of columns) in one launch sequence."""
        arrs = [np.ascontiguousarray(p, np.float32) for p in scans]
        cols = arrs[0].shape[1]
        assert all(a.ndim == 2 and a.shape[1] == cols for a in arrs) and 3 <= cols <= 16
        k = len(arrs)
        ptrs = (C.c_void_p * k)(*[a.ctypes.data for a in arrs])
        cnts = (C.c_size_t * k)(*[a.shape[0] for a in arrs])
        ids = np.empty(k, np.uint32)
        check(lib().gloc_scan_store_add_batch(self._h, ptrs, cnts, k, cols, _np_ptr(ids)))
        return [int(i) for i in ids]

    def build_target_index(self, scan_id):
        """Re-sort the scan's index into kd order: for scans that serve as registration targets (database places)."""
        check(lib().gloc_scan_store_build_target_index(self._h, int(scan_id)))
        return scan_id

    def debug_index(self, scan_id):
        """Test aid: the scan's index as the search sees it -- dict(perm, keys, kpos, order2, kd)."""
        f = lib().gloc_scan_store_debug_index
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        n = self.points(scan_id)
        perm, keys, kpos = np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, np.uint32)
        order2 = np.empty((n + 127) // 128, np.uint32)
        kd = C.c_int()
        check(f(self._h, int(scan_id), _np_ptr(perm), _np_ptr(keys), _np_ptr(kpos), _np_ptr(order2), C.byref(kd)))
        return dict(perm=perm, keys=keys, kpos=kpos, order2=order2, kd=bool(kd.value))

    def debug_boxes(self, scan_id, cs=2):
        """Test aid: the rest of the scan's index as the search sees it now -- dict(lo, hi: the header's box as
        order-preserving integers [3]; ox, oy, oz, inv_cell: the key grid (float32); box_lo, box_hi [nchunks, 4]: the chunk
        boxes' centres and negated half extents / 64; sb2 [n_pad / 32, 3, 4]: the paired sub-block boxes as interleaved;
        sup_lo, sup_hi [nsup, 4]; pad [n_pad - n, 4]: the padding points; order: the launch order for cs sources per lane).
        An empty scan has a header and empty arrays."""
        f = lib().gloc_scan_store_debug_boxes
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_uint32, C.c_int] + [C.c_void_p] * 9
        n = self.points(scan_id)
        nch = (n + 127) // 128
        n_pad, nsup, group = nch * 128, (nch + 63) // 64, 64 * int(cs)
        hb, hg = np.empty(6, np.uint32), np.empty(4, np.float32)
        box_lo, box_hi = np.empty((nch, 4), np.float32), np.empty((nch, 4), np.float32)
        sb2 = np.empty((n_pad // 32, 3, 4), np.float32)
        sup_lo, sup_hi = np.empty((nsup, 4), np.float32), np.empty((nsup, 4), np.float32)
        pad = np.empty((n_pad - n, 4), np.float32)
        order = np.empty((n + group - 1) // group if group else 0, np.uint32)
        check(f(self._h, int(scan_id), int(cs), *[_np_ptr(a) for a in (hb, hg, box_lo, box_hi, sb2, sup_lo, sup_hi, pad, order)]))
        return dict(lo=hb[:3].copy(), hi=hb[3:].copy(), ox=hg[0], oy=hg[1], oz=hg[2], inv_cell=hg[3], box_lo=box_lo,
                    box_hi=box_hi, sb2=sb2, sup_lo=sup_lo, sup_hi=sup_hi, pad=pad, order=order)

    def debug_kd_table(self, scan_id):
        """Test aid: the split planes of a target index -- dict(rounds: record levels on a path, split [records, 7]
        float32, axes [records] uint32: 2 bits per node in heap order); rounds = 0 and empty arrays without a table."""
        f = lib().gloc_scan_store_debug_kd_table
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_size_t), C.c_void_p, C.c_size_t]
        rounds, n_rec = C.c_uint32(), C.c_size_t()
        check(f(self._h, int(scan_id), C.byref(rounds), C.byref(n_rec), None, 0))
        rec = np.empty((n_rec.value, 8), np.uint32)
        if n_rec.value:
            check(f(self._h, int(scan_id), C.byref(rounds), C.byref(n_rec), _np_ptr(rec), rec.shape[0]))
        return dict(rounds=int(rounds.value), split=rec[:, :7].copy().view(np.float32), axes=rec[:, 7].copy())

    def build_target_index_batch(self, scan_ids):
        ids = np.ascontiguousarray(scan_ids, np.uint32).reshape(-1)
        check(lib().gloc_scan_store_build_target_index_batch(self._h, _np_ptr(ids), ids.shape[0]))

    def release(self, scan_id):
        check(lib().gloc_scan_store_release(self._h, int(scan_id)))

    def clear(self):
        check(lib().gloc_scan_store_clear(self._h))

    def __len__(self):
        n = C.c_size_t()
        check(lib().gloc_scan_store_count(self._h, C.byref(n)))
        return n.value

    def bytes(self):
        a, b = C.c_size_t(), C.c_size_t()
        check(lib().gloc_scan_store_bytes(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def points(self, scan_id):
        n = C.c_size_t()
        check(lib().gloc_scan_store_points(self._h, int(scan_id), C.byref(n)))
        return n.value

    def add_approx_voxel(self, base_id, leaf=0.2):
        """A new scan: the approximate voxel filter of scan base_id (NDT's source filter).  Returns its id."""
        sid = C.c_uint32()
        check(lib().gloc_scan_store_add_approx_voxel(self._h, int(base_id), float(leaf), C.byref(sid)))
        return sid.value

    def add_submap(self, ids, T, params=None, want_info=False):
        """A new scan: the member scans `ids` brought into one frame by the poses T [n, 4, 4] (member -> submap frame) and
        thinned by an exact voxel grid (gloc_scan_store_add_submap).  One id with the identity pose is the exact voxel-grid
        filter of a scan.  Returns its id, with want_info (id, dict(points_in, points_used, cells, kept))."""
        ids = np.ascontiguousarray(np.atleast_1d(ids), np.uint32).reshape(-1)
        Tp = np.ascontiguousarray(T, np.float32).reshape(-1, 16)
        if ids.shape[0] != Tp.shape[0]:
            raise ValueError(f"{ids.shape[0]} member ids but {Tp.shape[0]} poses")
        prm = params or default_submap_params()
        sid, info = C.c_uint32(), SubmapInfo()
        check(lib().gloc_scan_store_add_submap(self._h, _np_ptr(ids), _np_ptr(Tp), ids.shape[0], C.byref(prm), C.byref(sid),
                                               C.cast(C.pointer(info), C.c_void_p)))
        return (sid.value, info.as_dict()) if want_info else sid.value

    def add_submaps(self, submaps, params=None, want_info=False):
        """Several submaps, [(ids, T [n, 4, 4]), ...], in one batch call (gloc_scan_store_add_submaps): each equals its
        add_submap, bit for bit.  Returns the ids, with want_info (ids, [info dict])."""
        return _add_submaps(lib().gloc_scan_store_add_submaps, self._h, submaps, params, want_info)

    def cluster(self, scan_id, params=None, figures=True):
        """The Euclidean clusters of a resident scan (gloc_scan_store_cluster; default_cluster_params when None): a Clusters
        object.  figures=False leaves out the centroids and corners (and the device work behind them)."""
        prm = params or default_cluster_params()
        n = self.points(scan_id)
        root, label = np.empty(n, np.uint32), np.empty(n, np.uint32)
        nc, nk = C.c_uint32(), C.c_uint32()
        # (one call: no scan has more clusters than points)
        size, croot = np.empty(n, np.uint32), np.empty(n, np.uint32)
        cent, lo, hi = np.empty((n, 3), np.float64), np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
        f3 = [_np_ptr(cent), _np_ptr(lo), _np_ptr(hi)] if figures else [None, None, None]
        check(lib().gloc_scan_store_cluster(self._h, int(scan_id), C.byref(prm), _np_ptr(root), _np_ptr(label), n, _np_ptr(size), _np_ptr(croot),
                                            *f3, n, C.byref(nc), C.byref(nk)))
        K = nk.value
        out = Clusters(root=root, cluster=label, size=size[:K].copy(), cluster_root=croot[:K].copy(), n_components=int(nc.value), n_kept=K)
        if figures:
            out.centroid, out.lo, out.hi = cent[:K].copy(), lo[:K].copy(), hi[:K].copy()
        return out

    def add_filtered(self, base_id, params=None, want_info=False, **over):
        """A new scan: what the stages of `params` (default_scan_filter_params(**over) when None) leave of scan base_id --
        range crop, radius outlier removal, statistical outlier removal, clusters, one after the other
        (gloc_scan_store_add_filtered).  Returns its id, with want_info (id, dict(points_in, after_range, after_ror,
        after_sor, after_cluster))."""
        prm = params or default_scan_filter_params(**over)
        sid, info = C.c_uint32(), ScanFilterInfo()
        check(lib().gloc_scan_store_add_filtered(self._h, int(base_id), C.byref(prm), C.cast(C.pointer(sid), C.c_void_p),
                                                 C.cast(C.pointer(info), C.c_void_p)))
        return (sid.value, info.as_dict()) if want_info else sid.value

    def add_subset(self, base_id, idx):
        """A new scan: rows idx of scan base_id in the order given, gathered on the device (gloc_scan_store_add_subset)."""
        idx = np.ascontiguousarray(idx, np.uint32).reshape(-1)
        sid = C.c_uint32()
        check(lib().gloc_scan_store_add_subset(self._h, int(base_id), _np_ptr(idx) if idx.shape[0] else None, idx.shape[0],
                                               C.cast(C.pointer(sid), C.c_void_p)))
        return sid.value

    def download(self, scan_id):
        n = self.points(scan_id)
        out = np.empty((n, 3), np.float32)
        check(lib().gloc_scan_store_download(self._h, int(scan_id), _np_ptr(out), n))
        return out

    def build_normals(self, scan_id, k=10):
        """Per-point normals of a resident scan from its k nearest neighbours (gloc_scan_store_build_normals)."""
        check(lib().gloc_scan_store_build_normals(self._h, int(scan_id), int(k)))

    def normals(self, scan_id):
        """The scan's normals [n, 3] float32 in original order; a zero row means "no normal"."""
        n = self.points(scan_id)
        out = np.empty((n, 3), np.float32)
        check(lib().gloc_scan_store_normals(self._h, int(scan_id), _np_ptr(out), n))
        return out


    def build_fpfh(self, scan_id, normal_k=10, feature_k=16):
        """FPFH features of a resident scan (gloc_scan_store_build_fpfh); builds the normals too if the scan has none."""
        check(lib().gloc_scan_store_build_fpfh(self._h, int(scan_id), int(normal_k), int(feature_k)))

    def fpfh(self, scan_id):
        """The scan's features [n, 33] float32 in original order; a zero row means "no feature"."""
        n = self.points(scan_id)
        out = np.empty((n, FPFH_DIM), np.float32)
        check(lib().gloc_scan_store_fpfh(self._h, int(scan_id), _np_ptr(out), n))
        return out

    def _spfh(self, fn, scan_id, *support):
        n = self.points(scan_id)
        counts, used = np.empty((n, FPFH_DIM), np.uint16), np.empty(n, np.uint32)
        check(fn(self._h, int(scan_id), *support, _np_ptr(counts), _np_ptr(used), n))
        return counts, used

    def spfh(self, scan_id, feature_k=16):
        """Diagnostic: the SPFH counts [n, 33] uint16 and the pairs counted [n] uint32 (0: no SPFH) from the scan's normals."""
        return self._spfh(lib().gloc_scan_store_spfh, scan_id, int(feature_k))

    def radius_neighbors(self, scan_id, radius, max_nn):
        """The scan's radius lists (gloc_scan_store_radius_neighbors): idx [n, max_nn] uint32 and d2 [n, max_nn] float32, the
        max_nn nearest points within `radius` of each point in ascending (d2, index), padded with 0xFFFFFFFF / FLT_MAX, and
        count [n] uint32, the size of the whole neighbourhood."""
        n = self.points(scan_id)
        idx, d2, cnt = np.empty((n, int(max_nn)), np.uint32), np.empty((n, int(max_nn)), np.float32), np.empty(n, np.uint32)
        check(lib().gloc_scan_store_radius_neighbors(self._h, int(scan_id), float(radius), int(max_nn), _np_ptr(idx), _np_ptr(d2), _np_ptr(cnt), n))
        return idx, d2, cnt

    def build_normals_radius(self, scan_id, radius=1.0, max_nn=30, min_nn=5):
        """Per-point normals from the neighbours within `radius` (gloc_scan_store_build_normals_radius): at most max_nn of
        them, no normal below min_nn."""
        check(lib().gloc_scan_store_build_normals_radius(self._h, int(scan_id), float(radius), int(max_nn), int(min_nn)))

    def build_fpfh_radius(self, scan_id, support=None):
        """FPFH features over a metric support (gloc_scan_store_build_fpfh_radius; default_fpfh_radius_params when None)."""
        prm = support or default_fpfh_radius_params()
        check(lib().gloc_scan_store_build_fpfh_radius(self._h, int(scan_id), C.byref(prm)))

    def spfh_radius(self, scan_id, radius=2.5, max_nn=100):
        """Diagnostic: spfh() over the radius list of (radius, max_nn)."""
        return self._spfh(lib().gloc_scan_store_spfh_radius, scan_id, float(radius), int(max_nn))

    def iss_saliency(self, scan_id, params=None):
        """Diagnostic: the ISS saliency [n] float32 (0: not salient) and the sorted covariance eigenvalues [n, 3] float64 of
        every point (gloc_scan_store_iss_saliency), in original order; nothing is kept."""
        prm = params or default_iss_params()
        n = self.points(scan_id)
        sal, eig = np.empty(n, np.float32), np.empty((n, 3), np.float64)
        check(lib().gloc_scan_store_iss_saliency(self._h, int(scan_id), C.byref(prm), _np_ptr(sal), _np_ptr(eig), n))
        return sal, eig

    def build_keypoints(self, scan_id, params=None):
        """Give a resident scan its ISS keypoints (gloc_scan_store_build_keypoints; default_iss_params when None)."""
        prm = params or default_iss_params()
        check(lib().gloc_scan_store_build_keypoints(self._h, int(scan_id), C.byref(prm)))

    def keypoints(self, scan_id):
        """The scan's keypoints [K] uint32: original indices in ascending order (gloc_scan_store_keypoints)."""
        k = C.c_size_t(0)
        check(lib().gloc_scan_store_keypoint_count(self._h, int(scan_id), C.byref(k)))
        out = np.empty(k.value, np.uint32)
        check(lib().gloc_scan_store_keypoints(self._h, int(scan_id), _np_ptr(out) if k.value else None, k.value))
        return out

    def keypoint_fpfh(self, scan_id):
        """Diagnostic: the keypoints' feature rows [K, 33] float32 as the keypoint matcher reads them
        (gloc_scan_store_keypoint_fpfh)."""
        k = C.c_size_t(0)
        check(lib().gloc_scan_store_keypoint_count(self._h, int(scan_id), C.byref(k)))
        out = np.empty((k.value, FPFH_DIM), np.float32)
        check(lib().gloc_scan_store_keypoint_fpfh(self._h, int(scan_id), _np_ptr(out) if k.value else None, k.value))
        return out


class Registrar(_Handle):
    """Batched candidate registration (RANSAC-SVD + ICP) over a resident scan store (its own, or a
    shared ScanStore passed in / attached later)."""

    _C = "reg"
    synchronize, profile, profile_reset = _synchronize, _profile, _profile_reset

    def __init__(self, device=0, store=None):
        self._h = C.c_void_p()
        self.device = device
        self._store = None
        check(lib().gloc_reg_create(device, C.byref(self._h)))
        if store is not None:
            self.attach_store(store)

    def close(self):
        _Handle.close(self)
        self._store = None

    def attach_store(self, store):
        check(lib().gloc_reg_attach_store(self._h, store._h if store is not None else None))
        self._store = store  # keeps the store alive as long as this handle uses it

    def scan_release(self, scan_id):
        check(lib().gloc_reg_scan_release(self._h, int(scan_id)))

    def batch_multi(self, q_ids, cand_ids, init_T=None, params=None, stream_ids=None):
        """q_ids [Q]; cand_ids [Q, n] (NO_SCAN = no candidate).  Returns arrays with leading [Q, n]."""
        q = np.ascontiguousarray(q_ids, np.uint32).reshape(-1)
        ids = np.ascontiguousarray(cand_ids, np.uint32).reshape(q.shape[0], -1)
        Q, n = ids.shape
        prm = params or default_reg_params()
        it = None if init_T is None else np.ascontiguousarray(init_T, np.float32).reshape(Q * n, 16)
        T, rmse, inl, ok = self._outs(Q * n)
        sid = None if stream_ids is None else np.ascontiguousarray(stream_ids, np.uint32).reshape(Q * n)
        check(lib().gloc_reg_batch_multi(self._h, Q, _np_ptr(q), _np_ptr(ids), n,
                                         None if sid is None else _np_ptr(sid),
                                         None if it is None else _np_ptr(it), C.byref(prm),
                                         _np_ptr(T), _np_ptr(rmse), _np_ptr(inl), _np_ptr(ok)))
        return dict(T=T.reshape(Q, n, 4, 4), rmse=rmse.reshape(Q, n), inliers=inl.reshape(Q, n),
                    ok=ok.astype(bool).reshape(Q, n))

    def batch_multi_begin(self, q_ids, cand_ids, init_T=None, params=None, stream_ids=None):
        """Enqueue a batch and return at once; batch_multi_end() waits for it and returns what batch_multi returns."""
        q = np.ascontiguousarray(q_ids, np.uint32).reshape(-1)
        ids = np.ascontiguousarray(cand_ids, np.uint32).reshape(q.shape[0], -1)
        Q, n = ids.shape
        prm = params or default_reg_params()
        it = None if init_T is None else np.ascontiguousarray(init_T, np.float32).reshape(Q * n, 16)
        sid = None if stream_ids is None else np.ascontiguousarray(stream_ids, np.uint32).reshape(Q * n)
        check(lib().gloc_reg_batch_multi_begin(self._h, Q, _np_ptr(q), _np_ptr(ids), n,
                                               None if sid is None else _np_ptr(sid),
                                               None if it is None else _np_ptr(it), C.byref(prm)))
        self._pending_shape = (Q, n)

    def batch_multi_end(self):
        Q, n = getattr(self, "_pending_shape", None) or (1, 1)     # (end without a begin: the library says so, GLOC_ERR_STATE)
        self._pending_shape = None
        T, rmse, inl, ok = self._outs(Q * n)
        check(lib().gloc_reg_batch_multi_end(self._h, _np_ptr(T), _np_ptr(rmse), _np_ptr(inl), _np_ptr(ok)))
        return dict(T=T.reshape(Q, n, 4, 4), rmse=rmse.reshape(Q, n), inliers=inl.reshape(Q, n),
                    ok=ok.astype(bool).reshape(Q, n))

    def set_option(self, option, value):
        check(lib().gloc_reg_set_option(self._h, option, int(value)))

    def set_stream(self, hip_stream):
        _set_stream(self, hip_stream)

    def scan_upload(self, pts):
        pts = np.ascontiguousarray(pts, np.float32)
        assert pts.ndim == 2 and 3 <= pts.shape[1] <= 16
        sid = C.c_uint32()
        check(lib().gloc_reg_scan_upload(self._h, _np_ptr(pts), pts.shape[0], pts.shape[1],
                                         C.byref(sid)))
        return sid.value

    def scan_build_target_index(self, scan_id):
        check(lib().gloc_reg_scan_build_target_index(self._h, int(scan_id)))
        return scan_id

    def scan_add_submaps(self, submaps, params=None, want_info=False):
        """ScanStore.add_submaps over the handle's current store (gloc_reg_scan_add_submaps)."""
        return _add_submaps(lib().gloc_reg_scan_add_submaps, self._h, submaps, params, want_info)

    def scan_count(self):
        n = C.c_size_t()
        check(lib().gloc_reg_scan_count(self._h, C.byref(n)))
        return n.value

    def scan_clear(self):
        check(lib().gloc_reg_scan_clear(self._h))

    @staticmethod
    def _outs(n):
        return (np.empty((n, 4, 4), np.float32), np.empty(n, np.float32), np.empty(n, np.uint32),
                np.empty(n, np.int32))

    def batch(self, q_xyz, cands, init_T=None, params=None, stream_ids=None):
        q = np.ascontiguousarray(q_xyz, np.float32).reshape(-1, 3)
        cs = [np.ascontiguousarray(c, np.float32).reshape(-1, 3) for c in cands]
        n = len(cs)
        ptrs = (C.c_void_p * n)(*[c.ctypes.data for c in cs])
        cnts = (C.c_size_t * n)(*[c.shape[0] for c in cs])
        prm = params or default_reg_params()
        it = None if init_T is None else np.ascontiguousarray(init_T, np.float32).reshape(n, 16)
        T, rmse, inl, ok = self._outs(n)
        sid = None if stream_ids is None else np.ascontiguousarray(stream_ids, np.uint32)
        check(lib().gloc_reg_batch(self._h, _np_ptr(q), q.shape[0], ptrs, cnts, n,
                                   None if sid is None else _np_ptr(sid),
                                   None if it is None else _np_ptr(it), C.byref(prm), _np_ptr(T),
                                   _np_ptr(rmse), _np_ptr(inl), _np_ptr(ok)))
        return dict(T=T, rmse=rmse, inliers=inl, ok=ok.astype(bool))

    def batch_ids(self, q_id, cand_ids, init_T=None, params=None, stream_ids=None):
        ids = np.ascontiguousarray(cand_ids, np.uint32)
        n = ids.shape[0]
        prm = params or default_reg_params()
        it = None if init_T is None else np.ascontiguousarray(init_T, np.float32).reshape(n, 16)
        T, rmse, inl, ok = self._outs(n)
        sid = None if stream_ids is None else np.ascontiguousarray(stream_ids, np.uint32)
        check(lib().gloc_reg_batch_ids(self._h, int(q_id), _np_ptr(ids), n,
                                       None if sid is None else _np_ptr(sid),
                                       None if it is None else _np_ptr(it), C.byref(prm),
                                       _np_ptr(T), _np_ptr(rmse), _np_ptr(inl), _np_ptr(ok)))
        return dict(T=T, rmse=rmse, inliers=inl, ok=ok.astype(bool))

    def ndt_batch(self, src_id, tgt_ids, init_T=None, params=None):
        """NDT of scan src_id against each of tgt_ids (gloc_reg_ndt_batch_ids): returns T [n, 4, 4] float32, trans
        probability [n] float64, iterations [n], converged [n] bool."""
        ids = np.ascontiguousarray(np.atleast_1d(tgt_ids), np.uint32)
        n = ids.shape[0]
        prm = params or default_ndt_params()
        it = None if init_T is None else np.ascontiguousarray(init_T, np.float32).reshape(n, 16)
        T = np.empty((n, 4, 4), np.float32)
        prob, iters, conv = np.empty(n, np.float64), np.empty(n, np.uint32), np.empty(n, np.int32)
        check(lib().gloc_reg_ndt_batch_ids(self._h, int(src_id), _np_ptr(ids), n, None if it is None else _np_ptr(it),
                                           C.byref(prm), _np_ptr(T), _np_ptr(prob), _np_ptr(iters), _np_ptr(conv)))
        return T, prob, iters, conv.astype(bool)

    def _refine_batch(self, method, prm, src_id, tgt_ids, init_T, robust):
        """A single-source entry of a Gauss-Newton refinement: gloc_reg_<method>_batch_ids, or its _robust form with the robust
        block behind the method's own and the weights behind the other outputs."""
        ids = np.ascontiguousarray(np.atleast_1d(tgt_ids), np.uint32)
        n = ids.shape[0]
        it = None if init_T is None else np.ascontiguousarray(init_T, np.float32).reshape(n, 16)
        out = [np.empty((n, 4, 4), np.float32), np.empty(n, np.float32), np.empty(n, np.uint32), np.empty(n, np.int32)]
        blocks = [C.byref(prm)]
        if robust is not None:
            out.append(np.empty(n, np.float32))
            blocks.append(C.byref(robust))
        fn = getattr(lib(), "gloc_reg_%s_batch_ids%s" % (method, "" if robust is None else "_robust"))
        check(fn(self._h, int(src_id), _np_ptr(ids), n, None if it is None else _np_ptr(it), *blocks, *[_np_ptr(o) for o in out]))
        return tuple(out)

    def _refine_system(self, method, prm, src_id, tgt_id, T, robust, robust_pass):
        """One evaluation of a refinement's normal equations: gloc_reg_<method>_system, or its _robust form with the robust
        block and the pass behind the method's own block and the weights' sum behind the other outputs."""
        t = None if T is None else np.ascontiguousarray(T, np.float32).reshape(16)
        H, g, s, c, ws = np.empty((6, 6), np.float64), np.empty(6, np.float64), C.c_double(), C.c_uint64(), C.c_double()
        head = (self._h, int(src_id), int(tgt_id), None if t is None else _np_ptr(t), C.byref(prm))
        if robust is not None:
            check(getattr(lib(), "gloc_reg_%s_system_robust" % method)(*head, C.byref(robust), int(robust_pass), _np_ptr(H), _np_ptr(g),
                                                                       C.byref(s), C.byref(c), C.byref(ws)))
            return H, g, s.value, c.value, ws.value
        check(getattr(lib(), "gloc_reg_%s_system" % method)(*head, _np_ptr(H), _np_ptr(g), C.byref(s), C.byref(c)))
        return H, g, s.value, c.value

    def p2l_batch(self, src_id, tgt_ids, init_T=None, params=None, robust=None):
        """Point-to-plane ICP of scan src_id against each of tgt_ids (gloc_reg_p2l_batch_ids): returns T [n, 4, 4] float32,
        rmse [n] float32 (point-to-plane, at the final pose), iterations [n], status [n] (0 cap, 1 converged, 2 degenerate).
        robust: a RobustParams -- every pair weighted by its residual (gloc_reg_p2l_batch_ids_robust); then also weight [n]
        float32, the mean weight of the final evaluation."""
        return self._refine_batch("p2l", params or default_p2l_params(), src_id, tgt_ids, init_T, robust)

    def p2l_system(self, src_id, tgt_id, T=None, params=None, robust=None, robust_pass=0):
        """One evaluation of the point-to-plane normal equations at T: H [6, 6], g [6], sum r^2, pairs used.  robust: as
        p2l_batch, weighted at c(robust_pass) (gloc_reg_p2l_system_robust); then also the weights' sum."""
        return self._refine_system("p2l", params or default_p2l_params(), src_id, tgt_id, T, robust, robust_pass)

    def gicp_batch(self, src_id, tgt_ids, init_T=None, params=None, robust=None):
        """Generalized ICP of scan src_id against each of tgt_ids (gloc_reg_gicp_batch_ids): returns T [n, 4, 4] float32,
        rmse [n] float32 (sqrt of the mean e^T M e at the final pose), iterations [n], status [n] (0 cap, 1 converged,
        2 degenerate).  robust: a RobustParams (gloc_reg_gicp_batch_ids_robust); then also weight [n] float32, the mean
        weight of the final evaluation."""
        return self._refine_batch("gicp", params or default_gicp_params(), src_id, tgt_ids, init_T, robust)

    def gicp_system(self, src_id, tgt_id, T=None, params=None, robust=None, robust_pass=0):
        """One evaluation of the generalized ICP normal equations at T: H [6, 6], g [6], sum e^T M e, pairs used.  robust: as
        gicp_batch, weighted at c(robust_pass) (gloc_reg_gicp_system_robust); then also the weights' sum."""
        return self._refine_system("gicp", params or default_gicp_params(), src_id, tgt_id, T, robust, robust_pass)

    def fpfh_match(self, src_feat, tgt_feat, mutual=True):
        """Nearest feature of every source row among the target rows (gloc_reg_fpfh_match): idx [n_src] uint32
        (0xFFFFFFFF: none kept), d2 [n_src] float32 (+inf there)."""
        a = np.ascontiguousarray(src_feat, np.float32).reshape(-1, FPFH_DIM)
        b = np.ascontiguousarray(tgt_feat, np.float32).reshape(-1, FPFH_DIM)
        idx, d2 = np.empty(a.shape[0], np.uint32), np.empty(a.shape[0], np.float32)
        check(lib().gloc_reg_fpfh_match(self._h, _np_ptr(a) if a.size else None, a.shape[0], _np_ptr(b) if b.size else None,
                                        b.shape[0], 1 if mutual else 0, _np_ptr(idx) if idx.size else _np_ptr(np.empty(1, np.uint32)),
                                        _np_ptr(d2) if d2.size else None))
        return idx, d2

    def _fpfh_jobs(self, entry, src_id, ids, blocks, support, keypoints=None):
        """What fpfh_batch and fpfh_graph_batch share: entry(handle, source, targets, n, *blocks, T, inliers, n_pairs, ok), or
        its _radius form with the support block behind the others, or its _keypoints form with the support block (or null)
        and the keypoint block behind them."""
        n = ids.shape[0]
        T = np.empty((n, 4, 4), np.float32)
        inl, npairs, ok = np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, np.int32)
        if keypoints is not None:
            fn = getattr(lib(), entry + "_keypoints")
            blocks = blocks + [None if support is None else C.byref(support), C.byref(keypoints)]
        else:
            fn = getattr(lib(), entry if support is None else entry + "_radius")
            blocks = blocks if support is None else blocks + [C.byref(support)]
        check(fn(self._h, int(src_id), _np_ptr(ids), n, *blocks, _np_ptr(T), _np_ptr(inl), _np_ptr(npairs), _np_ptr(ok)))
        return dict(T=T, inliers=inl, n_pairs=npairs, ok=ok.astype(bool))

    def fpfh_batch(self, src_id, tgt_ids, stream_ids=None, params=None, support=None, keypoints=None):
        """Feature-based global registration of scan src_id against each of tgt_ids (gloc_reg_fpfh_batch_ids), no initial
        guess: returns dict(T [n, 4, 4] float32 source -> target, inliers [n], n_pairs [n], ok [n] bool).  T is a start for
        p2l_batch / gicp_batch / batch_ids(init_T=...), not a refined pose.  support: a FpfhRadiusParams -- features over
        that metric support (gloc_reg_fpfh_batch_ids_radius) instead of the k-NN lists of params.  keypoints: an IssParams --
        match the scans' ISS keypoints alone (gloc_reg_fpfh_batch_ids_keypoints); None: every point, today's calls."""
        ids = np.ascontiguousarray(np.atleast_1d(tgt_ids), np.uint32)
        prm = params or default_fpfh_params()
        sid = None if stream_ids is None else np.ascontiguousarray(stream_ids, np.uint32).reshape(ids.shape[0])
        return self._fpfh_jobs("gloc_reg_fpfh_batch_ids", src_id, ids, [None if sid is None else _np_ptr(sid), C.byref(prm)], support, keypoints)

    def fpfh_graph_batch(self, src_id, tgt_ids, params=None, support=None, keypoints=None):
        """Feature-based global registration through the correspondence graph (gloc_reg_fpfh_graph_batch_ids): the matches of
        fpfh_batch, the pose from their second-order compatibility instead of RANSAC.  Returns dict(T [n, 4, 4] float32
        source -> target, inliers [n], n_pairs [n], ok [n] bool); T is a start for a refinement, as fpfh_batch's.  support: as
        fpfh_batch's (gloc_reg_fpfh_graph_batch_ids_radius); keypoints: as fpfh_batch's (gloc_reg_fpfh_graph_batch_ids_keypoints)."""
        ids = np.ascontiguousarray(np.atleast_1d(tgt_ids), np.uint32)
        prm = params or default_fpfh_graph_params()
        return self._fpfh_jobs("gloc_reg_fpfh_graph_batch_ids", src_id, ids, [C.byref(prm)], support, keypoints)

    def fpfh_fgr_batch(self, src_id, tgt_ids, params=None, support=None, keypoints=None, stream_ids=None):
        """Feature-based global registration by Fast Global Registration (gloc_reg_fpfh_fgr_batch_ids): the matches of
        fpfh_batch, the pose from one graduated-non-convexity optimisation over them instead of RANSAC.  Returns dict(T [n, 4,
        4] float32 source -> target, inliers [n], n_pairs [n], ok [n] bool); T is a start for a refinement, as fpfh_batch's.
        support, keypoints, stream_ids: as fpfh_batch's (the _radius and _keypoints entries)."""
        ids = np.ascontiguousarray(np.atleast_1d(tgt_ids), np.uint32)
        prm = params or default_fgr_params()
        sid = None if stream_ids is None else np.ascontiguousarray(stream_ids, np.uint32).reshape(ids.shape[0])
        return self._fpfh_jobs("gloc_reg_fpfh_fgr_batch_ids", src_id, ids, [None if sid is None else _np_ptr(sid), C.byref(prm)], support, keypoints)

    def fgr_pairs(self, P, Q, params=None, stream_id=0):
        """Fast Global Registration of a pair list P, Q [m, 3] (gloc_reg_fgr_pairs): dict(mult [m] uint32, n_tuples, d2,
        system [27] float64 (H's upper triangle, then g, of the last update formed), T [4, 4] float32, inliers, status (0: all
        updates ran, 2: degenerate), ok)."""
        P = np.ascontiguousarray(P, np.float32).reshape(-1, 3)
        Q = np.ascontiguousarray(Q, np.float32).reshape(-1, 3)
        m = P.shape[0]
        assert Q.shape[0] == m
        prm = params or default_fgr_params()
        mult, system = np.empty(max(m, 1), np.uint32), np.empty(27, np.float64)
        T = np.empty((4, 4), np.float32)
        nt, inl, d2, status, ok = C.c_uint32(), C.c_uint32(), C.c_double(), C.c_int(), C.c_int()
        check(lib().gloc_reg_fgr_pairs(self._h, _np_ptr(P) if m else None, _np_ptr(Q) if m else None, m, int(stream_id), C.byref(prm),
                                       _np_ptr(mult), C.byref(nt), C.byref(d2), _np_ptr(system), _np_ptr(T), C.byref(inl), C.byref(status),
                                       C.byref(ok)))
        return dict(mult=mult[:m], n_tuples=nt.value, d2=d2.value, system=system, T=T, inliers=inl.value, status=status.value,
                    ok=bool(ok.value))

    def pair_graph(self, P, Q, params=None):
        """The correspondence graph of a pair list P, Q [m, 3] (gloc_reg_pair_graph): dict(degree [m] uint32, score [m] uint64,
        seeds, set_sizes, seed_inliers [n_seeds] uint32, T [4, 4] float32, inliers, winner_rank (0xFFFFFFFF: none), ok)."""
        P = np.ascontiguousarray(P, np.float32).reshape(-1, 3)
        Q = np.ascontiguousarray(Q, np.float32).reshape(-1, 3)
        m = P.shape[0]
        assert Q.shape[0] == m
        prm = params or default_fpfh_graph_params()
        S = int(prm.n_seeds)
        deg, score = np.empty(max(m, 1), np.uint32), np.empty(max(m, 1), np.uint64)
        seeds, sizes, sinl = np.empty(S, np.uint32), np.empty(S, np.uint32), np.empty(S, np.uint32)
        T = np.empty((4, 4), np.float32)
        inl, rank, ok = C.c_uint32(), C.c_uint32(), C.c_int()
        check(lib().gloc_reg_pair_graph(self._h, _np_ptr(P) if m else None, _np_ptr(Q) if m else None, m, C.byref(prm), _np_ptr(deg),
                                        _np_ptr(score), _np_ptr(seeds), _np_ptr(sizes), _np_ptr(sinl), _np_ptr(T), C.byref(inl),
                                        C.byref(rank), C.byref(ok)))
        return dict(degree=deg[:m], score=score[:m], seeds=seeds, set_sizes=sizes, seed_inliers=sinl, T=T, inliers=inl.value,
                    winner_rank=rank.value, ok=bool(ok.value))

    def vgicp_batch(self, src_id, tgt_ids, init_T=None, params=None, robust=None):
        """Voxelized generalized ICP of scan src_id against each of tgt_ids (gloc_reg_vgicp_batch_ids): returns
        T [n, 4, 4] float32, rmse [n] float32 (sqrt of the weighted e^T M e per pair at the final pose), iterations [n],
        status [n] (0 cap, 1 converged, 2 degenerate).  robust: a RobustParams (gloc_reg_vgicp_batch_ids_robust); then also
        weight [n] float32, the mean weight of the final evaluation."""
        return self._refine_batch("vgicp", params or default_vgicp_params(), src_id, tgt_ids, init_T, robust)

    def _pairs(self, fn, prm, src_ids, tgt_ids, init_T, robust):
        """A pair-list entry (gloc_reg_<m>_pairs): row c is (src_ids[c], tgt_ids[c]); None in tgt_ids is "no target"."""
        src, tgt = self._pair_ids(src_ids, tgt_ids)
        n = src.shape[0]
        it = None if init_T is None else np.ascontiguousarray(init_T, np.float32).reshape(n, 16)
        T = np.empty((n, 4, 4), np.float32)
        rmse, iters, status = np.empty(n, np.float32), np.empty(n, np.uint32), np.empty(n, np.int32)
        weight = None if robust is None else np.empty(n, np.float32)
        check(fn(self._h, _np_ptr(src), _np_ptr(tgt), n, None if it is None else _np_ptr(it), C.byref(prm),
                 None if robust is None else C.byref(robust), _np_ptr(T), _np_ptr(rmse), _np_ptr(iters), _np_ptr(status),
                 None if weight is None else _np_ptr(weight)))
        return (T, rmse, iters, status) if robust is None else (T, rmse, iters, status, weight)

    def p2l_pairs(self, src_ids, tgt_ids, init_T=None, params=None, robust=None):
        """Point-to-plane ICP of a list of (source, target) pairs in one call (gloc_reg_p2l_pairs): what p2l_batch returns,
        row c that of p2l_batch(src_ids[c], [tgt_ids[c]]) bit for bit.  None in tgt_ids: no target (the row of an empty one)."""
        return self._pairs(lib().gloc_reg_p2l_pairs, params or default_p2l_params(), src_ids, tgt_ids, init_T, robust)

    def gicp_pairs(self, src_ids, tgt_ids, init_T=None, params=None, robust=None):
        """Generalized ICP of a list of (source, target) pairs in one call (gloc_reg_gicp_pairs): as p2l_pairs."""
        return self._pairs(lib().gloc_reg_gicp_pairs, params or default_gicp_params(), src_ids, tgt_ids, init_T, robust)

    def vgicp_pairs(self, src_ids, tgt_ids, init_T=None, params=None, robust=None):
        """Voxelized generalized ICP of a list of (source, target) pairs in one call (gloc_reg_vgicp_pairs): as p2l_pairs."""
        return self._pairs(lib().gloc_reg_vgicp_pairs, params or default_vgicp_params(), src_ids, tgt_ids, init_T, robust)

    @staticmethod
    def _pair_ids(src_ids, tgt_ids):
        """The id arrays of a pair list: None in tgt_ids is "no target"."""
        src = np.ascontiguousarray(np.atleast_1d(src_ids), np.uint32)
        tgt = np.ascontiguousarray([NO_SCAN if t is None else t for t in np.atleast_1d(np.asarray(tgt_ids, dtype=object))], np.uint32)
        if tgt.shape[0] != src.shape[0]:
            raise ValueError("src_ids and tgt_ids differ in length")
        return src, tgt

    def _pairs_system(self, fn, prm, src_ids, tgt_ids, T, robust, robust_pass):
        """The system form of a pair list (gloc_reg_<m>_pairs_system): row c is <m>_system(src_ids[c], tgt_ids[c], T[c]) bit
        for bit.  Returns H [n, 6, 6], g [n, 6], sum [n], count [n] uint64, and with a robust block the weights' sums [n]."""
        src, tgt = self._pair_ids(src_ids, tgt_ids)
        n = src.shape[0]
        t = None if T is None else np.ascontiguousarray(T, np.float32).reshape(n, 16)
        H, g, s, c = np.empty((n, 6, 6), np.float64), np.empty((n, 6), np.float64), np.empty(n, np.float64), np.empty(n, np.uint64)
        ws = None if robust is None else np.empty(n, np.float64)
        check(fn(self._h, _np_ptr(src), _np_ptr(tgt), n, None if t is None else _np_ptr(t), C.byref(prm),
                 None if robust is None else C.byref(robust), int(robust_pass), _np_ptr(H), _np_ptr(g), _np_ptr(s), _np_ptr(c),
                 None if ws is None else _np_ptr(ws)))
        return (H, g, s, c) if robust is None else (H, g, s, c, ws)

    def p2l_pairs_system(self, src_ids, tgt_ids, T=None, params=None, robust=None, robust_pass=0):
        """The point-to-plane normal equations of a list of (source, target, pose) rows in one call
        (gloc_reg_p2l_pairs_system): what p2l_system returns, stacked.  None in tgt_ids: no target (a zero row)."""
        return self._pairs_system(lib().gloc_reg_p2l_pairs_system, params or default_p2l_params(), src_ids, tgt_ids, T, robust, robust_pass)

    def gicp_pairs_system(self, src_ids, tgt_ids, T=None, params=None, robust=None, robust_pass=0):
        """The generalized ICP normal equations of a list of rows in one call (gloc_reg_gicp_pairs_system): as p2l_pairs_system."""
        return self._pairs_system(lib().gloc_reg_gicp_pairs_system, params or default_gicp_params(), src_ids, tgt_ids, T, robust, robust_pass)

    def vgicp_pairs_system(self, src_ids, tgt_ids, T=None, params=None, robust=None, robust_pass=0):
        """The voxelized generalized ICP normal equations of a list of rows in one call (gloc_reg_vgicp_pairs_system): as
        p2l_pairs_system."""
        return self._pairs_system(lib().gloc_reg_vgicp_pairs_system, params or default_vgicp_params(), src_ids, tgt_ids, T, robust, robust_pass)

    def evaluate_pairs(self, src_ids, tgt_ids, T=None, params=None, symmetric=False):
        """The point-to-point evaluation of a list of (source, target, pose) rows in one call (gloc_reg_evaluate_pairs):
        dict(fitness [n] float32 = counted pairs / source points, rmse [n] float32 over the counted pairs, count [n] uint32,
        info [n, 6, 6] float64 = sum J^T J with J = [-[p]x, I], g [n, 6] = sum J^T e).  A pair counts within
        params.max_corr_dist (0.6 m).  None in tgt_ids: no target (a zero row).
        symmetric: the reversed rows (tgt, src, T^-1 -- inverted in float64, rounded to fp32) are evaluated in the same call;
        adds fitness_rev, rmse_rev, count_rev and overlap = min(fitness, fitness_rev).  Every target then has to be a scan."""
        prm = params or default_eval_params()
        src, tgt = self._pair_ids(src_ids, tgt_ids)
        n = src.shape[0]
        t = None if T is None else np.ascontiguousarray(T, np.float32).reshape(n, 16)
        if symmetric:
            if (tgt == NO_SCAN).any():
                raise ValueError("symmetric evaluation needs a target in every row")
            if t is not None:
                inv = np.linalg.inv(t.reshape(n, 4, 4).astype(np.float64)).astype(np.float32).reshape(n, 16)
                t = np.ascontiguousarray(np.concatenate([t, inv]))
            src, tgt = np.concatenate([src, tgt]), np.concatenate([tgt, src])
        m = src.shape[0]
        fit, rmse, cnt = np.empty(m, np.float32), np.empty(m, np.float32), np.empty(m, np.uint32)
        info, g = np.empty((m, 6, 6), np.float64), np.empty((m, 6), np.float64)
        check(lib().gloc_reg_evaluate_pairs(self._h, _np_ptr(src), _np_ptr(tgt), m, None if t is None else _np_ptr(t), C.byref(prm),
                                            _np_ptr(fit), _np_ptr(rmse), _np_ptr(cnt), _np_ptr(info), _np_ptr(g)))
        out = dict(fitness=fit[:n], rmse=rmse[:n], count=cnt[:n], info=info[:n], g=g[:n])
        if symmetric:
            out.update(fitness_rev=fit[n:], rmse_rev=rmse[n:], count_rev=cnt[n:], overlap=np.minimum(fit[:n], fit[n:]))
        return out

    def vgicp_system(self, src_id, tgt_id, T=None, params=None, robust=None, robust_pass=0):
        """One evaluation of the voxelized generalized ICP normal equations at T: H [6, 6], g [6], the weighted sum of
        e^T M e, pairs used.  robust: as vgicp_batch, weighted at c(robust_pass) (gloc_reg_vgicp_system_robust); then also
        the weights' sum."""
        return self._refine_system("vgicp", params or default_vgicp_params(), src_id, tgt_id, T, robust, robust_pass)

    def vgicp_voxels(self, scan_id, params=None):
        """The voxels of a scan, sorted by key: dict(key3 [m, 3] int32, count [m], mean [m, 3], nn6 [m, 6] = the mean of the
        members' n n^T as xx xy xz yy yz zz)."""
        prm = params or default_vgicp_params()
        m = C.c_size_t()
        check(lib().gloc_reg_vgicp_voxels(self._h, int(scan_id), C.byref(prm), 0, None, None, None, None, C.byref(m)))
        k = m.value
        key, cnt = np.empty((k, 3), np.int32), np.empty(k, np.uint32)
        mean, nn6 = np.empty((k, 3), np.float64), np.empty((k, 6), np.float64)
        if k:
            check(lib().gloc_reg_vgicp_voxels(self._h, int(scan_id), C.byref(prm), k, _np_ptr(key), _np_ptr(cnt), _np_ptr(mean),
                                              _np_ptr(nn6), C.byref(m)))
        return dict(key3=key, count=cnt, mean=mean, nn6=nn6)

    # ---- resident voxel maps (include/gloc3d.h: M1 - M8) ----
    def vmap_create(self, params=None):
        """A resident voxel map owned by this handle (gloc_reg_vmap_create): its id."""
        prm = params or default_vmap_params()
        mid = C.c_uint32()
        check(lib().gloc_reg_vmap_create(self._h, C.byref(prm), C.byref(mid)))
        return mid.value

    def vmap_destroy(self, map_id):
        check(lib().gloc_reg_vmap_destroy(self._h, int(map_id)))

    def vmap_insert(self, map_id, scan_ids, T=None):
        """Merges the scans into the map in order, scan i under T[i] (scan -> map, [n, 4, 4]); T None: as they are
        (gloc_reg_vmap_insert).  GlocError with code 3 (GLOC_ERR_NOMEM) at the first scan that does not fit."""
        ids = np.ascontiguousarray(np.atleast_1d(scan_ids), np.uint32)
        n = ids.shape[0]
        t = None if T is None else np.ascontiguousarray(T, np.float32).reshape(n, 16)
        check(lib().gloc_reg_vmap_insert(self._h, int(map_id), _np_ptr(ids), n, None if t is None else _np_ptr(t)))

    def vmap_prune(self, map_id, center=None, max_dist=0.0, max_age=0):
        """Removes the voxels farther than max_dist from center (None: rule off) or older than max_age inserts (0: off)
        (gloc_reg_vmap_prune): how many went."""
        c = None if center is None else np.ascontiguousarray(center, np.float32).reshape(3)
        removed = C.c_uint32()
        check(lib().gloc_reg_vmap_prune(self._h, int(map_id), None if c is None else _np_ptr(c), float(max_dist), int(max_age),
                                        C.byref(removed)))
        return removed.value

    def vmap_info(self, map_id):
        """dict(n_voxels, capacity, n_inserts, resolution, n_points) (gloc_reg_vmap_info)."""
        o = VmapInfo()
        check(lib().gloc_reg_vmap_info(self._h, int(map_id), C.byref(o)))
        return dict(n_voxels=o.n_voxels, capacity=o.capacity, n_inserts=o.n_inserts, resolution=o.resolution, n_points=o.n_points)

    def vmap_voxels(self, map_id):
        """The map's voxels, sorted by key: vgicp_voxels' dict and stamp [m] uint32, the insert that last touched each."""
        m = C.c_size_t()
        check(lib().gloc_reg_vmap_voxels(self._h, int(map_id), 0, None, None, None, None, None, C.byref(m)))
        k = m.value
        key, cnt, stamp = np.empty((k, 3), np.int32), np.empty(k, np.uint32), np.empty(k, np.uint32)
        mean, nn6 = np.empty((k, 3), np.float64), np.empty((k, 6), np.float64)
        if k:
            check(lib().gloc_reg_vmap_voxels(self._h, int(map_id), k, _np_ptr(key), _np_ptr(cnt), _np_ptr(mean), _np_ptr(nn6),
                                             _np_ptr(stamp), C.byref(m)))
        return dict(key3=key, count=cnt, mean=mean, nn6=nn6, stamp=stamp)

    def vgicp_vmap(self, src_ids, map_ids, init_T=None, params=None, robust=None):
        """Voxelized generalized ICP of a list of (source scan, resident map) rows in one call (gloc_reg_vgicp_vmap): what
        vgicp_pairs returns.  None in map_ids: no target.  params.resolution must be the maps', params.min_points 1."""
        return self._pairs(lib().gloc_reg_vgicp_vmap, params or default_vgicp_params(), src_ids, map_ids, init_T, robust)

    def vgicp_vmap_system(self, src_ids, map_ids, T=None, params=None, robust=None, robust_pass=0):
        """The normal equations of a list of (source scan, resident map, pose) rows (gloc_reg_vgicp_vmap_system): what
        vgicp_pairs_system returns."""
        return self._pairs_system(lib().gloc_reg_vgicp_vmap_system, params or default_vgicp_params(), src_ids, map_ids, T, robust, robust_pass)

    def ndt_derivatives(self, src_id, tgt_id, p6, params=None):
        """score, gradient [6], Hessian [6, 6] of the filtered source against the target's cells at p6."""
        p = np.ascontiguousarray(p6, np.float64).reshape(6)
        prm = params or default_ndt_params()
        s, g, H = C.c_double(), np.empty(6, np.float64), np.empty((6, 6), np.float64)
        check(lib().gloc_reg_ndt_derivatives(self._h, int(src_id), int(tgt_id), _np_ptr(p), C.byref(prm), C.byref(s),
                                             _np_ptr(g), _np_ptr(H)))
        return s.value, g, H

    def ndt_cells(self, scan_id, params=None):
        """The valid NDT cells of a scan, sorted by key: dict(key3 [m, 3] int32, count [m], mean [m, 3], icov [m, 3, 3])."""
        prm = params or default_ndt_params()
        m = C.c_size_t()
        check(lib().gloc_reg_ndt_cells(self._h, int(scan_id), C.byref(prm), 0, None, None, None, None, C.byref(m)))
        k = m.value
        key, cnt = np.empty((k, 3), np.int32), np.empty(k, np.uint32)
        mean, icov = np.empty((k, 3), np.float64), np.empty((k, 3, 3), np.float64)
        if k:
            check(lib().gloc_reg_ndt_cells(self._h, int(scan_id), C.byref(prm), k, _np_ptr(key), _np_ptr(cnt), _np_ptr(mean),
                                           _np_ptr(icov), C.byref(m)))
        return dict(key3=key, count=cnt, mean=mean, icov=icov)

    def first_success_multi(self, q_ids, cand_ids, init_T=None, params=None):
        """The reference's stop-at-the-first-success loop for several queries: returns rank [Q] (-1: none),
        T [Q, 4, 4], rmse [Q], inliers [Q] and the number of registrations actually run."""
        q = np.ascontiguousarray(q_ids, np.uint32).reshape(-1)
        ids = np.ascontiguousarray(cand_ids, np.uint32).reshape(q.shape[0], -1)
        Q, n = ids.shape
        prm = params or default_reg_params()
        it = None if init_T is None else np.ascontiguousarray(init_T, np.float32).reshape(Q * n, 16)
        rank = np.empty(Q, np.int32)
        T, rmse, inl = np.empty((Q, 4, 4), np.float32), np.empty(Q, np.float32), np.empty(Q, np.uint32)
        jobs = C.c_uint64()
        check(lib().gloc_reg_first_success_multi(self._h, Q, _np_ptr(q), _np_ptr(ids), n,
                                                 None if it is None else _np_ptr(it), C.byref(prm), _np_ptr(rank),
                                                 _np_ptr(T), _np_ptr(rmse), _np_ptr(inl), C.byref(jobs)))
        return dict(rank=rank, T=T, rmse=rmse, inliers=inl, jobs_run=jobs.value)

    def nn(self, src, tgt, T=None):
        s = np.ascontiguousarray(src, np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(tgt, np.float32).reshape(-1, 3)
        idx = np.empty(s.shape[0], np.uint32)
        d2 = np.empty(s.shape[0], np.float32)
        Tp = None if T is None else np.ascontiguousarray(T, np.float32).reshape(16)
        check(lib().gloc_reg_nn(self._h, _np_ptr(s), s.shape[0], _np_ptr(t), t.shape[0],
                                None if Tp is None else _np_ptr(Tp), _np_ptr(idx), _np_ptr(d2)))
        return idx, d2

    def ransac_hypotheses(self, src, tgt, corr, seed, cand, n_hyp, inlier_thresh):
        s = np.ascontiguousarray(src, np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(tgt, np.float32).reshape(-1, 3)
        c = np.ascontiguousarray(corr, np.uint32)
        Rt = np.empty((n_hyp, 12), np.float32)
        valid = np.empty(n_hyp, np.uint32)
        inl = np.empty(n_hyp, np.uint32)
        check(lib().gloc_reg_ransac_hypotheses(self._h, _np_ptr(s), _np_ptr(t), _np_ptr(c),
                                               s.shape[0], seed, cand, n_hyp, _np_ptr(Rt),
                                               _np_ptr(valid), _np_ptr(inl), inlier_thresh))
        return Rt, valid, inl

    def final_steps(self, n_jobs):
        """Per job of the last batch: RMS displacement of the last ICP update (what max_final_step gates)."""
        out = np.empty(n_jobs, np.float32)
        check(lib().gloc_reg_final_steps(self._h, _np_ptr(out), n_jobs))
        return out

    def nn_stats(self):
        c, n = C.c_uint64(), C.c_uint64()
        check(lib().gloc_reg_nn_stats(self._h, C.byref(c), C.byref(n)))
        return c.value, n.value

    def debug_chain(self):
        """Test aid: (chained launches enqueued, chained launches that timed out) -- GLOC_REG_OPT_NN_CHAIN."""
        f = lib().gloc_reg_debug_chain
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        n, t = C.c_uint64(), C.c_uint64()
        check(f(self._h, C.byref(n), C.byref(t)))
        return n.value, t.value

    def debug_needed_iters(self, inl, n, conf, max_iters):
        """Test aid: the adaptive RANSAC stop's iteration count as the device computes it."""
        f = lib().gloc_reg_debug_needed_iters
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p]
        a, b = np.ascontiguousarray(inl, np.uint32), np.ascontiguousarray(n, np.uint32)
        out = np.empty(a.shape[0], np.uint32)
        check(f(self._h, _np_ptr(a), _np_ptr(b), a.shape[0], conf, max_iters, _np_ptr(out)))
        return out

    def debug_chain_stall(self, on):
        """Test aid: make the chained launch's solvers wait for a wave that never comes (the bounded waits)."""
        f = lib().gloc_reg_debug_chain_stall
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_int]
        check(f(self._h, 1 if on else 0))

    def debug_corr(self, job, n_src):
        """Test aid: correspondences of the last 1-NN pass of the last batch (caller's index space)."""
        f = lib().gloc_reg_debug_corr
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        idx, d2 = np.empty(n_src, np.uint32), np.empty(n_src, np.float32)
        check(f(self._h, job, n_src, _np_ptr(idx), _np_ptr(d2)))
        return idx, d2


def reg_select_first_ok(ok):
    a = np.ascontiguousarray(ok, np.int32)
    return lib().gloc_reg_select_first_ok(_np_ptr(a), a.shape[0])


class NetVladFC(_Handle):
    """NetVLAD-FC pooling head (model/netvlad_fc.py NetVLAD.forward without gating)."""

    _C = "vlad"
    set_stream, set_profile, profile = _set_stream, _set_profile, _profile

    def __init__(self, conv_w, centroids, fc_w, conv_b=None, normalize_input=True, device=0):
        cw = np.ascontiguousarray(conv_w, np.float32)
        ce = np.ascontiguousarray(centroids, np.float32)
        fw = np.ascontiguousarray(fc_w, np.float32)
        cb = None if conv_b is None else np.ascontiguousarray(conv_b, np.float32)
        self.K, self.C = cw.shape
        self.out_dim = fw.shape[1]
        assert ce.shape == (self.K, self.C) and fw.shape[0] == self.K * self.C
        self._h = C.c_void_p()
        check(lib().gloc_vlad_create(device, self.C, self.K, self.out_dim, _np_ptr(cw),
                                     None if cb is None else _np_ptr(cb), _np_ptr(ce), _np_ptr(fw),
                                     1 if normalize_input else 0, C.byref(self._h)))

    def set_gating(self, gating_w=None, scale=None, shift=None):
        """GatingContext after the FC: y * sigmoid((y W) * scale + shift); None switches it off."""
        if gating_w is None:
            check(lib().gloc_vlad_set_gating(self._h, None, None, None))
            return
        gw = np.ascontiguousarray(gating_w, np.float32)
        sc = np.ascontiguousarray(scale, np.float32)
        sh = np.ascontiguousarray(shift, np.float32)
        assert gw.shape == (self.out_dim, self.out_dim) and sc.shape == (self.out_dim,) == sh.shape
        check(lib().gloc_vlad_set_gating(self._h, _np_ptr(gw), _np_ptr(sc), _np_ptr(sh)))

    def forward(self, feat):
        x = np.ascontiguousarray(feat, np.float32)
        n = x.shape[0]
        x = x.reshape(n, self.C, -1)
        out = np.empty((n, self.out_dim), np.float32)
        check(lib().gloc_vlad_forward(self._h, _np_ptr(x), n, x.shape[2], _np_ptr(out)))
        return out

    def forward_device(self, feat_ptr, n, hw, out_ptr):
        check(lib().gloc_vlad_forward_device(self._h, C.c_void_p(feat_ptr), n, hw, C.c_void_p(out_ptr)))


def default_bev_params(**over):
    p = BevParams()
    check(lib().gloc_bev_default_params(C.byref(p)))
    for k, v in over.items():
        if k == "pad_bgr":
            for i in range(3):
                p.pad_bgr[i] = v[i]
        else:
            setattr(p, k, v)
    return p


class BevProjector(_Handle):
    """BEV occupancy projection (RpyPCLoopDetector::get_projected_grid + crop_pad_occupancy,
    registration/loop_detector.cpp:83-106,122-151)."""

    _C = "bev"
    set_stream, synchronize, set_profile, profile = _set_stream, _synchronize, _set_profile, _profile

    def __init__(self, device=0):
        self._h = C.c_void_p()
        check(lib().gloc_bev_create(device, C.byref(self._h)))

    @staticmethod
    def _out_array(p, n_scans=None):
        shape = (p.out_height, p.out_width, 3) if p.format == BEV_U8_HWC3 else (3, p.out_height, p.out_width)
        if n_scans is not None:
            shape = (n_scans,) + shape
        return np.empty(shape, np.uint8 if p.format == BEV_U8_HWC3 else np.float32)

    def project(self, points, params=None):
        """points [n, 3 or more] float32 -> (image, info dict)."""
        p = params or default_bev_params()
        pts = np.ascontiguousarray(points, np.float32)
        if pts.ndim != 2:
            pts = pts.reshape(-1, 3)
        out, info = self._out_array(p), BevInfo()
        check(lib().gloc_bev_project(self._h, _np_ptr(pts), pts.shape[0], pts.shape[1], C.byref(p),
                                     _np_ptr(out), C.byref(info)))
        return out, info.as_dict()

    def project_batch_device(self, xyz_ptr, offsets, stride_floats, out_ptr, params=None, want_info=True):
        """Device buffers: scans back to back at xyz_ptr, host `offsets` (n_scans + 1, in points)."""
        p = params or default_bev_params()
        off = np.ascontiguousarray(offsets, np.uint64)
        n = off.shape[0] - 1
        infos = (BevInfo * n)() if want_info else None
        check(lib().gloc_bev_project_batch_device(self._h, C.c_void_p(xyz_ptr), _np_ptr(off), n, stride_floats,
                                                  C.byref(p), C.c_void_p(out_ptr),
                                                  C.cast(infos, C.c_void_p) if want_info else None))
        return [i.as_dict() for i in infos] if want_info else None

    def raw_image(self, info, scan=0):
        """The uncropped [height, width] u8 image (occupancy_grid) of a scan of the last projection."""
        out = np.empty((info["height"], info["width"]), np.uint8)
        check(lib().gloc_bev_raw_image(self._h, scan, _np_ptr(out), out.size))
        return out


def default_pillar_params(**over):
    """gloc_pillar_params with the reference's grid and P (gen_libtorch_pointpillar.py:25-34), then `over`
    (xbound / ybound / zbound as [lo, hi, res])."""
    p = PillarParams()
    check(lib().gloc_pillar_default_params(C.byref(p)))
    for k, v in over.items():
        if k in ("xbound", "ybound", "zbound"):
            for i in range(3):
                getattr(p, k)[i] = v[i]
        else:
            setattr(p, k, v)
    return p


def _scan_batch(scans):
    """A scan [n, >=4] or a list of them -> (points [sum n, stride] float32, offsets [B + 1] uint64)."""
    if isinstance(scans, np.ndarray) and scans.ndim == 2:
        scans = [scans]
    arrs = [np.asarray(s, np.float32).reshape(-1, np.shape(s)[-1] if np.ndim(s) == 2 else 4) for s in scans]
    stride = max([a.shape[1] for a in arrs] + [4])
    assert all(a.shape[1] == stride for a in arrs if a.shape[0]), "scans of one batch share their row width"
    off = np.zeros(len(arrs) + 1, np.uint64)
    off[1:] = np.cumsum([a.shape[0] for a in arrs])
    pts = np.ascontiguousarray(np.concatenate([a.reshape(-1, stride) for a in arrs]) if arrs else np.zeros((0, stride)),
                               np.float32)
    return pts, off


PILLAR_BACKBONE_LAYERS = 13


def pillar_backbone_layer_shape(layer):
    """(Cin, Cout, stride, relu) of PointPillar backbone layer `layer` (0..12), from the library's own table."""
    ci, co, st, r = C.c_uint32(), C.c_uint32(), C.c_int(), C.c_int()
    check(lib().gloc_pillar_backbone_layer_shape(layer, C.byref(ci), C.byref(co), C.byref(st), C.byref(r)))
    return ci.value, co.value, st.value, bool(r.value)


class PillarEncoder(_Handle):
    """PointPillar scan front end: points_to_voxels + the traced model's [P, 16] input (model/voxel.py:23-133,
    gen_libtorch_pointpillar.py:47-62) and the PointNet + scatter-mean canvas [64, gx * gy * gz]
    (model/s2s_merged.py:113-127,204-218)."""

    _C = "pillar"
    set_stream, synchronize = _set_stream, _synchronize
    set_profile, profile, profile_reset = _set_profile, _profile, _profile_reset

    def __init__(self, device=0):
        self._h = C.c_void_p()
        self.device = device
        check(lib().gloc_pillar_create(device, C.byref(self._h)))

    def set_pointnet(self, w, bn_weight, bn_bias, bn_mean, bn_var, eps=1e-5):
        """w [64, 14] (or the Conv1d's [64, 14, 1]); BatchNorm1d weight, bias, running mean, running var [64]."""
        a = [np.ascontiguousarray(x, np.float32).reshape(-1) for x in (w, bn_weight, bn_bias, bn_mean, bn_var)]
        assert a[0].size == PILLAR_FEATURES * 14 and all(x.size == PILLAR_FEATURES for x in a[1:])
        check(lib().gloc_pillar_set_pointnet(self._h, *[_np_ptr(x) for x in a], float(eps)))

    def inputs(self, scans, params=None):
        """A scan [n, 4+] or a list of them -> [B, P, 16] float32."""
        p = params or default_pillar_params()
        pts, off = _scan_batch(scans)
        out = np.empty((len(off) - 1, p.num_points, 16), np.float32)
        check(lib().gloc_pillar_inputs(self._h, _np_ptr(pts), _np_ptr(off), len(off) - 1, pts.shape[1], C.byref(p),
                                       _np_ptr(out)))
        return out

    def canvas(self, scans, params=None):
        """A scan [n, 4+] or a list of them -> [B, 64, gx * gy * gz] float32."""
        p = params or default_pillar_params()
        pts, off = _scan_batch(scans)
        gx, gy, gz = p.grid()
        out = np.empty((len(off) - 1, PILLAR_FEATURES, gx * gy * gz), np.float32)
        check(lib().gloc_pillar_canvas(self._h, _np_ptr(pts), _np_ptr(off), len(off) - 1, pts.shape[1], C.byref(p),
                                       _np_ptr(out)))
        return out

    def inputs_device(self, pts_ptr, offsets, stride_floats, out_ptr, params=None):
        """Device buffers on the handle's stream: scans back to back at pts_ptr, host `offsets` (B + 1, in points)."""
        p = params or default_pillar_params()
        off = np.ascontiguousarray(offsets, np.uint64)
        check(lib().gloc_pillar_inputs_device(self._h, C.c_void_p(pts_ptr), _np_ptr(off), off.shape[0] - 1,
                                              stride_floats, C.byref(p), C.c_void_p(out_ptr)))

    def canvas_device(self, pts_ptr, offsets, stride_floats, out_ptr, params=None):
        p = params or default_pillar_params()
        off = np.ascontiguousarray(offsets, np.uint64)
        check(lib().gloc_pillar_canvas_device(self._h, C.c_void_p(pts_ptr), _np_ptr(off), off.shape[0] - 1,
                                              stride_floats, C.byref(p), C.c_void_p(out_ptr)))

    def set_backbone_layer(self, layer, w, bn_weight, bn_bias, bn_mean, bn_var, eps=1e-5):
        """w [Cout, Cin, 3, 3] (torch's Conv2d weight); BatchNorm2d weight, bias, running mean, running var [Cout]."""
        ci, co, _, _ = pillar_backbone_layer_shape(layer)
        wa = np.ascontiguousarray(w, np.float32)
        bn = [np.ascontiguousarray(x, np.float32).reshape(-1) for x in (bn_weight, bn_bias, bn_mean, bn_var)]
        assert wa.shape == (co, ci, 3, 3) and all(x.size == co for x in bn), (layer, wa.shape)
        check(lib().gloc_pillar_set_backbone_layer(self._h, layer, _np_ptr(wa), *[_np_ptr(x) for x in bn], float(eps)))

    def backbone_device(self, canvas_ptr, n, gx, gy, out_ptr):
        """Device buffers on the handle's stream: canvas [n, 64, gx * gy] -> [n, 128, gy * gx]."""
        check(lib().gloc_pillar_backbone_device(self._h, C.c_void_p(canvas_ptr), n, gx, gy, C.c_void_p(out_ptr)))

    def backbone_layer_device(self, layer, in_ptr, n, H, W, out_ptr):
        """One backbone layer with its BatchNorm (+ ReLU), NCHW [n, Cin, H, W] -> [n, Cout, Ho, Wo] (layers 9 and 10:
        the input before the upsample)."""
        check(lib().gloc_pillar_backbone_layer_device(self._h, layer, C.c_void_p(in_ptr), n, H, W, C.c_void_p(out_ptr)))

    def upsample_device(self, in_ptr, n, ch, H, W, factor, out_ptr):
        """The backbone's bilinear upsample (align_corners=True), NCHW [n, ch, H, W] -> [n, ch, factor H, factor W]."""
        check(lib().gloc_pillar_upsample_device(self._h, C.c_void_p(in_ptr), n, ch, H, W, factor, C.c_void_p(out_ptr)))

    def features(self, scans, params=None):
        """A scan [n, 4+] or a list of them -> backbone features [B, 128, gy * gx] float32 (canvas + backbone)."""
        p = params or default_pillar_params()
        pts, off = _scan_batch(scans)
        gx, gy, gz = p.grid()
        out = np.empty((len(off) - 1, 128, gx * gy * gz), np.float32)
        check(lib().gloc_pillar_features(self._h, _np_ptr(pts), _np_ptr(off), len(off) - 1, pts.shape[1], C.byref(p),
                                         _np_ptr(out)))
        return out

    def features_device(self, pts_ptr, offsets, stride_floats, out_ptr, params=None):
        p = params or default_pillar_params()
        off = np.ascontiguousarray(offsets, np.uint64)
        check(lib().gloc_pillar_features_device(self._h, C.c_void_p(pts_ptr), _np_ptr(off), off.shape[0] - 1,
                                                stride_floats, C.byref(p), C.c_void_p(out_ptr)))

VGG_LAYERS = 13


def vgg_layer_shape(layer):
    """(Cin, Cout, relu, pool) of encoder layer `layer` (0..12), from the library's own table."""
    ci, co, r, p = C.c_uint32(), C.c_uint32(), C.c_int(), C.c_int()
    check(lib().gloc_vgg_layer_shape(layer, C.byref(ci), C.byref(co), C.byref(r), C.byref(p)))
    return ci.value, co.value, bool(r.value), bool(p.value)


class VggEncoder(_Handle):
    """VGG16 features[:-2], the i2i model's encoder (s2s_libtorch/gen_libtorch_i2i.py:36-60): [n, 3, H, W] ->
    [n, 512, H / 16, W / 16], fp32 NCHW in and out (split-bf16 matrix cores inside, include/gloc3d.h)."""

    _C = "vgg"
    set_stream, synchronize = _set_stream, _synchronize
    set_profile, profile, profile_reset = _set_profile, _profile, _profile_reset

    def __init__(self, device=0):
        self._h = C.c_void_p()
        self.device = device
        check(lib().gloc_vgg_create(device, C.byref(self._h)))

    def set_layer(self, layer, w, b):
        """w [Cout, Cin, 3, 3] (torch's Conv2d weight), b [Cout]."""
        ci, co, _, _ = vgg_layer_shape(layer)
        wa = np.ascontiguousarray(w, np.float32)
        ba = np.ascontiguousarray(b, np.float32)
        assert wa.shape == (co, ci, 3, 3) and ba.shape == (co,), (layer, wa.shape, ba.shape)
        check(lib().gloc_vgg_set_layer(self._h, layer, _np_ptr(wa), _np_ptr(ba)))

    def set_layers(self, layers):
        """layers: 13 (w, b) pairs in network order."""
        assert len(layers) == VGG_LAYERS
        for i, (w, b) in enumerate(layers):
            self.set_layer(i, w, b)

    def forward(self, images):
        """Host [n, 3, H, W] (or [3, H, W]) -> [n, 512, H / 16, W / 16]."""
        x = np.ascontiguousarray(images, np.float32)
        if x.ndim == 3:
            x = x[None]
        n, _, H, W = x.shape
        out = np.empty((n, 512, H // 16, W // 16), np.float32)
        check(lib().gloc_vgg_forward(self._h, _np_ptr(x), n, H, W, _np_ptr(out)))
        return out

    def forward_device(self, images_ptr, n, H, W, out_ptr):
        check(lib().gloc_vgg_forward_device(self._h, C.c_void_p(images_ptr), n, H, W, C.c_void_p(out_ptr)))

    def forward_layer_device(self, layer, in_ptr, n, H, W, out_ptr):
        """One layer with its epilogue on device buffers, NCHW [n, Cin, H, W] -> [n, Cout, Ho, Wo]."""
        check(lib().gloc_vgg_forward_layer(self._h, layer, C.c_void_p(in_ptr), n, H, W, C.c_void_p(out_ptr)))


def default_coarse_params(**over):
    p = CoarseParams()
    check(lib().gloc_coarse_default_params(C.byref(p)))
    for k, v in over.items():
        setattr(p, k, v)
    return p


class CoarseMatcher(_Handle):
    """Coarse global (x, y, yaw) match on BEV occupancy grids (RpyPCLoopDetector::match on two
    OccupancyGrids, registration/loop_detector.cpp:186-288)."""

    _C = "coarse"

    def __init__(self, device=0, params=None):
        self._h = C.c_void_p()
        check(lib().gloc_coarse_create(device, C.byref(self._h)))
        self.params = params or default_coarse_params()

    def add_image(self, occupancy, ox, oy, resolution):
        img = np.ascontiguousarray(occupancy, np.uint8)
        gid = C.c_uint32()
        check(lib().gloc_coarse_add_image(self._h, _np_ptr(img), img.shape[1], img.shape[0], ox, oy, resolution,
                                          C.byref(self.params), C.byref(gid)))
        return gid.value

    def add_scan(self, pts):
        pts = np.ascontiguousarray(pts, np.float32)
        gid = C.c_uint32()
        check(lib().gloc_coarse_add_scan(self._h, _np_ptr(pts), pts.shape[0], pts.shape[1], C.byref(self.params),
                                         C.byref(gid)))
        return gid.value

    def add_store_scan(self, store, scan_id):
        gid = C.c_uint32()
        check(lib().gloc_coarse_add_store_scan(self._h, store._h, int(scan_id), C.byref(self.params), C.byref(gid)))
        return gid.value

    def add_store_scans(self, store, scan_ids):
        ids = np.ascontiguousarray(scan_ids, np.uint32).reshape(-1)
        out = np.empty(ids.shape[0], np.uint32)
        check(lib().gloc_coarse_add_store_scans(self._h, store._h, _np_ptr(ids), ids.shape[0], C.byref(self.params), _np_ptr(out)))
        return out

    def match_pairs(self, q_grids, db_grids):
        qs = np.ascontiguousarray(q_grids, np.uint32).reshape(-1)
        ds = np.ascontiguousarray(db_grids, np.uint32).reshape(-1)
        n = qs.shape[0]
        assert ds.shape[0] == n
        xyyaw, ratio, ok = np.empty((n, 3), np.float32), np.empty(n, np.float32), np.empty(n, np.int32)
        self.last_scale = np.empty(n, np.float32)     # the reference's `scale` output of the same match
        check(lib().gloc_coarse_match_pairs(self._h, _np_ptr(qs), _np_ptr(ds), n, C.byref(self.params), _np_ptr(xyyaw),
                                            _np_ptr(ratio), _np_ptr(ok), _np_ptr(self.last_scale)))
        return xyyaw, ratio, ok.astype(bool)

    def release(self, grid_id):
        check(lib().gloc_coarse_release(self._h, int(grid_id)))

    def cells(self, grid_id):
        n = C.c_uint32()
        check(lib().gloc_coarse_cells(self._h, int(grid_id), C.byref(n), None, 0))
        out = np.empty(n.value, np.uint32)
        check(lib().gloc_coarse_cells(self._h, int(grid_id), C.byref(n), _np_ptr(out), n.value))
        return out

    def match(self, q_grid, db_grids):
        ids = np.ascontiguousarray(db_grids, np.uint32)
        n = ids.shape[0]
        xyyaw, ratio, ok = np.empty((n, 3), np.float32), np.empty(n, np.float32), np.empty(n, np.int32)
        self.last_scale = np.empty(n, np.float32)     # the reference's `scale` output of the same match
        check(lib().gloc_coarse_match(self._h, int(q_grid), _np_ptr(ids), n, C.byref(self.params), _np_ptr(xyyaw),
                                      _np_ptr(ratio), _np_ptr(ok), _np_ptr(self.last_scale)))
        return xyyaw, ratio, ok.astype(bool)


def default_pgo_params(**over):
    """gloc_pgo_params as gloc_pgo_default_params leaves them, then `over`."""
    p = PgoParams()
    lib().gloc_pgo_default_params(C.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


class PoseGraphOptimizer(_Handle):
    """Levenberg-Marquardt over the node poses of a pose graph on the device (gloc_pgo_* of include/gloc3d.h): poses
    [n, 4, 4] float64 (node -> map), edges (src, tgt, Z [m, 4, 4] float32 source -> target, info [m, 6, 6] float64)."""

    _C = "pgo"
    set_stream, synchronize = _set_stream, _synchronize
    set_profile, profile, profile_reset = _set_profile, _profile, _profile_reset

    def __init__(self, device=0):
        self._h = C.c_void_p()
        check(lib().gloc_pgo_create(device, C.byref(self._h)))

    @staticmethod
    def _graph(poses, fixed, src, tgt, Z, info, mask):
        P = np.ascontiguousarray(poses, np.float64).reshape(-1, 16)
        fx = np.ascontiguousarray(fixed, np.uint8).reshape(-1)
        s, t = np.ascontiguousarray(src, np.uint32).reshape(-1), np.ascontiguousarray(tgt, np.uint32).reshape(-1)
        Zf = np.ascontiguousarray(Z, np.float32).reshape(-1, 16)
        Om = np.ascontiguousarray(info, np.float64).reshape(-1, 36)
        mk = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(-1)
        assert fx.shape[0] == P.shape[0] and t.shape[0] == s.shape[0] == Zf.shape[0] == Om.shape[0]
        assert mk is None or mk.shape[0] == s.shape[0]
        return P, fx, s, t, Zf, Om, mk

    def linearize(self, poses, fixed, src, tgt, Z, info, mask=None, params=None, robust=None):
        """One linearisation at `poses`: dict(r [m, 6], s2 [m], weight [m], g [n, 6], Hdiag [n, 6, 6], cost)."""
        P, fx, s, t, Zf, Om, mk = self._graph(poses, fixed, src, tgt, Z, info, mask)
        prm = params or default_pgo_params()
        n, m = P.shape[0], s.shape[0]
        r, s2, w = np.empty((m, 6)), np.empty(m), np.empty(m)
        g, H, cost = np.empty((n, 6)), np.empty((n, 6, 6)), C.c_double()
        check(lib().gloc_pgo_linearize(self._h, _np_ptr(P), _np_ptr(fx), n, _np_ptr(s), _np_ptr(t), _np_ptr(Zf), _np_ptr(Om),
                                       None if mk is None else _np_ptr(mk), m, C.byref(prm), None if robust is None else C.byref(robust),
                                       _np_ptr(r), _np_ptr(s2), _np_ptr(w), _np_ptr(g), _np_ptr(H), C.byref(cost)))
        return dict(r=r, s2=s2, weight=w, g=g, Hdiag=H, cost=cost.value)

    def optimize(self, poses, fixed, src, tgt, Z, info, mask=None, params=None, robust=None):
        """(poses [n, 4, 4] float64, s2 [m], weight [m], PgoResult)."""
        P, fx, s, t, Zf, Om, mk = self._graph(poses, fixed, src, tgt, Z, info, mask)
        prm = params or default_pgo_params()
        n, m = P.shape[0], s.shape[0]
        out, s2, w, res = np.empty((n, 4, 4)), np.empty(m), np.empty(m), PgoResult()
        check(lib().gloc_pgo_optimize(self._h, _np_ptr(P), _np_ptr(fx), n, _np_ptr(s), _np_ptr(t), _np_ptr(Zf), _np_ptr(Om),
                                      None if mk is None else _np_ptr(mk), m, C.byref(prm), None if robust is None else C.byref(robust),
                                      _np_ptr(out), _np_ptr(s2), _np_ptr(w), C.byref(res)))
        return out, s2, w, res

    def consistency(self, poses, src, tgt, Z, info, path=None, params=None, want_s2=False):
        """The largest mutually consistent set of the L candidate closures at `poses` (gloc_pgo_consistency, C1 - C6):
        dict(mask [L] bool, clique_size, winner_rank, ok, status [L], degree [L], score [L], seeds [n_seeds], clique_sizes
        [n_seeds]) and, with want_s2, s2 [L, L].  path [n]: a coordinate along the trajectory, None for all zeros."""
        P = np.ascontiguousarray(poses, np.float64).reshape(-1, 16)
        s, t = np.ascontiguousarray(src, np.uint32).reshape(-1), np.ascontiguousarray(tgt, np.uint32).reshape(-1)
        Zf = np.ascontiguousarray(Z, np.float32).reshape(-1, 16)
        Om = np.ascontiguousarray(info, np.float64).reshape(-1, 36)
        pth = None if path is None else np.ascontiguousarray(path, np.float64).reshape(-1)
        n, L = P.shape[0], s.shape[0]
        assert t.shape[0] == L and Zf.shape[0] == L and Om.shape[0] == L and (pth is None or pth.shape[0] == n)
        prm = params or default_pgo_consistency_params()
        S = max(1, min(int(prm.n_seeds), 1024))          # (an n_seeds out of range is refused by the call; the arrays just exist)
        mask, status, degree, score = np.zeros(L, np.uint8), np.zeros(L, np.uint8), np.zeros(L, np.uint32), np.zeros(L, np.uint64)
        seeds, sizes = np.zeros(S, np.uint32), np.zeros(S, np.uint32)
        s2 = np.empty((L, L)) if want_s2 else None
        size, rank, ok = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib().gloc_pgo_consistency(self._h, _np_ptr(P), n, _np_ptr(s), _np_ptr(t), _np_ptr(Zf), _np_ptr(Om),
                                         None if pth is None else _np_ptr(pth), L, C.byref(prm), _np_ptr(mask), C.byref(size), C.byref(rank),
                                         C.byref(ok), _np_ptr(status), _np_ptr(degree), _np_ptr(score), _np_ptr(seeds), _np_ptr(sizes),
                                         None if s2 is None else _np_ptr(s2)))
        out = dict(mask=mask.astype(bool), clique_size=size.value, winner_rank=rank.value, ok=bool(ok.value), status=status, degree=degree,
                   score=score, seeds=seeds, clique_sizes=sizes)
        if want_s2:
            out["s2"] = s2
        return out


def default_pgo_consistency_params(**over):
    """gloc_pgo_consistency_params as gloc_pgo_consistency_default_params leaves them, then `over`."""
    p = PgoConsistencyParams()
    lib().gloc_pgo_consistency_default_params(C.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def default_sc_params(**over):
    p = ScParams()
    check(lib().gloc_sc_default_params(C.byref(p)))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def sc_shift_to_yaw(params, shift):
    """The yaw (radians, in (-pi, pi]) of a query in the frame of the place it matched at `shift`."""
    yaw = C.c_float()
    check(lib().gloc_sc_shift_to_yaw(C.byref(params), int(shift), C.byref(yaw)))
    return yaw.value


class ScanContext(_Handle):
    """Scan Context place descriptors (Kim & Kim, IROS 2018): built from host or resident scans, kept as a resident
    database, searched exhaustively with the column shift that aligns the two scans' yaw (gloc_sc_* of include/gloc3d.h)."""

    _C = "sc"
    set_stream, synchronize = _set_stream, _synchronize
    set_profile, profile, profile_reset = _set_profile, _profile, _profile_reset

    def __init__(self, device=0, params=None):
        self._h = C.c_void_p()
        self.params = params or default_sc_params()
        check(lib().gloc_sc_create(device, C.byref(self.params), C.byref(self._h)))
        self.shape = (int(self.params.n_rings), int(self.params.n_sectors))

    def _desc(self, d, n=None):
        d = np.ascontiguousarray(d, np.float32).reshape((-1,) + self.shape)
        assert n is None or d.shape[0] == n
        return d

    @staticmethod
    def _ids(scan_ids):
        return np.ascontiguousarray(scan_ids, np.uint32).reshape(-1)

    def describe(self, pts):
        pts = np.ascontiguousarray(pts, np.float32)
        out = np.empty(self.shape, np.float32)
        check(lib().gloc_sc_describe(self._h, _np_ptr(pts), pts.shape[0], pts.shape[1], _np_ptr(out)))
        return out

    def describe_store_scans(self, store, scan_ids):
        ids = self._ids(scan_ids)
        out = np.empty((ids.shape[0],) + self.shape, np.float32)
        check(lib().gloc_sc_describe_store_scans(self._h, store._h, _np_ptr(ids), ids.shape[0], _np_ptr(out)))
        return out

    def add(self, desc):
        d = self._desc(desc)
        check(lib().gloc_sc_add(self._h, _np_ptr(d), d.shape[0]))

    def add_scan(self, pts):
        pts = np.ascontiguousarray(pts, np.float32)
        row = C.c_uint64()
        check(lib().gloc_sc_add_scan(self._h, _np_ptr(pts), pts.shape[0], pts.shape[1], C.byref(row)))
        return row.value

    def add_store_scans(self, store, scan_ids):
        """Returns the row index of the first of the scans; the others follow it in order."""
        ids = self._ids(scan_ids)
        first = C.c_uint64()
        check(lib().gloc_sc_add_store_scans(self._h, store._h, _np_ptr(ids), ids.shape[0], C.byref(first)))
        return first.value

    def __len__(self):
        n = C.c_size_t()
        check(lib().gloc_sc_size(self._h, C.byref(n)))
        return n.value

    def clear(self):
        check(lib().gloc_sc_clear(self._h))

    def reserve(self, n):
        check(lib().gloc_sc_reserve(self._h, n))

    def rows(self, first=0, n=None):
        n = len(self) - first if n is None else n
        out = np.empty((n,) + self.shape, np.float32)
        check(lib().gloc_sc_rows(self._h, first, n, _np_ptr(out)))
        return out

    def ring_keys(self, first=0, n=None):
        n = len(self) - first if n is None else n
        out = np.empty((n, self.shape[0]), np.float32)
        check(lib().gloc_sc_ring_keys(self._h, first, n, _np_ptr(out)))
        return out

    def save(self, path):
        check(lib().gloc_sc_save(self._h, os.fsencode(path)))

    def load(self, path):
        check(lib().gloc_sc_load(self._h, os.fsencode(path)))

    @staticmethod
    def _search_outs(nq, k):
        return np.empty((nq, k), np.uint64), np.empty((nq, k), np.float32), np.empty((nq, k), np.uint32)

    def search(self, q_desc, k, row_begin=0, row_end=None):
        """(row indices, distances, shifts), each [nq, k], ascending by (distance, row index)."""
        q = self._desc(q_desc)
        idx, dist, shift = self._search_outs(q.shape[0], k)
        check(lib().gloc_sc_search(self._h, _np_ptr(q), q.shape[0], k, row_begin, SIZE_MAX if row_end is None else row_end,
                                   _np_ptr(idx), _np_ptr(dist), _np_ptr(shift)))
        return idx, dist, shift

    def search_store_scans(self, store, q_scan_ids, k, row_begin=0, row_end=None):
        ids = self._ids(q_scan_ids)
        idx, dist, shift = self._search_outs(ids.shape[0], k)
        check(lib().gloc_sc_search_store_scans(self._h, store._h, _np_ptr(ids), ids.shape[0], k, row_begin,
                                               SIZE_MAX if row_end is None else row_end, _np_ptr(idx), _np_ptr(dist),
                                               _np_ptr(shift)))
        return idx, dist, shift

    def distances(self, q_desc, rows, by_shift=False):
        """One descriptor against the listed rows: (distances, shifts[, the distance at every shift [n, n_sectors]])."""
        q = self._desc(q_desc, 1)
        r = np.ascontiguousarray(rows, np.uint64).reshape(-1)
        dist, shift = np.empty(r.shape[0], np.float32), np.empty(r.shape[0], np.uint32)
        by = np.empty((r.shape[0], self.shape[1]), np.float32) if by_shift else None
        check(lib().gloc_sc_distances(self._h, _np_ptr(q), _np_ptr(r), r.shape[0], _np_ptr(dist), _np_ptr(shift),
                                      _np_ptr(by) if by_shift else None))
        return (dist, shift, by) if by_shift else (dist, shift)

    def shift_to_yaw(self, shift):
        return sc_shift_to_yaw(self.params, shift)


def default_m2dp_params(**over):
    p = M2dpParams()
    check(lib().gloc_m2dp_default_params(C.byref(p)))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def m2dp_dim(params):
    n = C.c_size_t()
    check(lib().gloc_m2dp_dim(C.byref(params), C.byref(n)))
    return n.value


def m2dp_frame_to_seed(frame_q, frame_db):
    """The 4 x 4 float32 pose query -> place of two M2DP frames [12] (gloc_m2dp_frame_to_seed; host only)."""
    fq, fd = (np.ascontiguousarray(f, np.float64).reshape(12) for f in (frame_q, frame_db))
    T = np.empty((4, 4), np.float32)
    check(lib().gloc_m2dp_frame_to_seed(_np_ptr(fq), _np_ptr(fd), _np_ptr(T)))
    return T


class M2dp(_Handle):
    """M2DP place descriptors (He, Wang & Zhang, IROS 2016): plain L2 vectors for KnnIndex, built from host or resident
    scans together with the PCA frame they are built in (gloc_m2dp_* of include/gloc3d.h)."""

    _C = "m2dp"
    set_stream, synchronize = _set_stream, _synchronize
    set_profile, profile, profile_reset = _set_profile, _profile, _profile_reset

    def __init__(self, device=0, params=None):
        self._h = C.c_void_p()
        self.params = params or default_m2dp_params()
        check(lib().gloc_m2dp_create(device, C.byref(self.params), C.byref(self._h)))
        self.n_planes = int(self.params.n_azimuth * self.params.n_elevation)
        self.n_bins = int(self.params.n_rings * self.params.n_sectors)
        self.dim = self.n_planes + self.n_bins

    def _outs(self, n, counts):
        return (np.empty((n, self.dim), np.float32), np.empty((n, 12), np.float64),
                np.empty((n, self.n_planes, self.n_bins), np.uint32) if counts else None)

    def describe(self, pts, counts=False):
        """(descriptor [dim], frame [12][, counts [planes, bins]]) of one host scan [n, 3..16]."""
        pts = np.ascontiguousarray(pts, np.float32)
        d, f, c = self._outs(1, counts)
        check(lib().gloc_m2dp_describe(self._h, _np_ptr(pts), pts.shape[0], pts.shape[1], _np_ptr(d), _np_ptr(f),
                                       _np_ptr(c) if counts else None))
        return (d[0], f[0], c[0]) if counts else (d[0], f[0])

    def describe_store_scans(self, store, scan_ids, counts=False):
        """(descriptors [n, dim], frames [n, 12][, counts [n, planes, bins]]) of resident scans, one launch sequence."""
        ids = np.ascontiguousarray(scan_ids, np.uint32).reshape(-1)
        d, f, c = self._outs(ids.shape[0], counts)
        check(lib().gloc_m2dp_describe_store_scans(self._h, store._h, _np_ptr(ids), ids.shape[0], _np_ptr(d), _np_ptr(f),
                                                   _np_ptr(c) if counts else None))
        return (d, f, c) if counts else (d, f)

    def describe_store_scans_device(self, store, scan_ids, out_ptr):
        """The rows [n, dim] float32 into device memory at out_ptr, enqueued on the handle's stream."""
        ids = np.ascontiguousarray(scan_ids, np.uint32).reshape(-1)
        check(lib().gloc_m2dp_describe_store_scans_device(self._h, store._h, _np_ptr(ids), ids.shape[0], C.c_void_p(out_ptr)))

    def signature_svd(self, counts, n_points):
        """(descriptors [n, dim], sigma [n, 2]) of given count matrices [n, planes, bins] (the SVD kernel alone)."""
        c = np.ascontiguousarray(counts, np.uint32).reshape(-1, self.n_planes, self.n_bins)
        n = np.ascontiguousarray(n_points, np.uint32).reshape(-1)
        assert n.shape[0] == c.shape[0]
        d, s = np.empty((c.shape[0], self.dim), np.float32), np.empty((c.shape[0], 2), np.float64)
        check(lib().gloc_m2dp_signature_svd(self._h, _np_ptr(c), _np_ptr(n), c.shape[0], _np_ptr(d), _np_ptr(s)))
        return d, s


def default_ground_params(**over):
    p = GroundParams()
    check(lib().gloc_ground_default_params(C.byref(p)))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def ground_transform_from_plane(plane):
    T = np.empty(16, np.float32)
    check(lib().gloc_ground_transform_from_plane(_np_ptr(np.ascontiguousarray(plane, np.float32)), _np_ptr(T)))
    return T.reshape(4, 4)


class GroundEstimator(_Handle):
    """Ground pre-alignment (GroundEstimator::EsitmateGroundAndTransform,
    registration/ground_estimator.cpp:196-228)."""

    _C = "ground"
    set_profile, profile = _set_profile, _profile

    def __init__(self, device=0):
        self._h = C.c_void_p()
        check(lib().gloc_ground_create(device, C.byref(self._h)))

    def set_option(self, option, value):
        check(lib().gloc_ground_set_option(self._h, option, value))

    def estimate(self, points, params=None, want_cloud=False):
        """points [n, 3 or more] float32 -> (T_l2g 4x4, info dict[, transformed cloud])."""
        p = params or default_ground_params()
        pts = np.ascontiguousarray(points, np.float32)
        T, info = np.empty(16, np.float32), GroundInfo()
        out = np.empty_like(pts) if want_cloud else None
        check(lib().gloc_ground_estimate(self._h, _np_ptr(pts), pts.shape[0], pts.shape[1], C.byref(p), _np_ptr(T),
                                         C.byref(info), _np_ptr(out) if want_cloud else None))
        return (T.reshape(4, 4), info.as_dict(), out) if want_cloud else (T.reshape(4, 4), info.as_dict())

    def estimate_device(self, xyz_ptr, n, stride_floats, out_ptr=None, params=None):
        p = params or default_ground_params()
        T, info = np.empty(16, np.float32), GroundInfo()
        check(lib().gloc_ground_estimate_device(self._h, C.c_void_p(xyz_ptr), n, stride_floats, C.byref(p), _np_ptr(T),
                                                C.byref(info), C.c_void_p(out_ptr) if out_ptr else None))
        return T.reshape(4, 4), info.as_dict()

    def knn(self, xyz, k=10):
        p = np.ascontiguousarray(xyz, np.float32)
        idx = np.empty((p.shape[0], k), np.uint32)
        d2 = np.empty((p.shape[0], k), np.float32)
        check(lib().gloc_ground_knn(self._h, _np_ptr(p), p.shape[0], k, _np_ptr(idx), _np_ptr(d2)))
        return idx, d2

    def normals(self, xyz, k=10):
        p = np.ascontiguousarray(xyz, np.float32)
        nrm = np.empty((p.shape[0], 3), np.float32)
        bins = np.empty(p.shape[0], np.uint8)
        check(lib().gloc_ground_normals(self._h, _np_ptr(p), p.shape[0], k, _np_ptr(nrm), _np_ptr(bins)))
        return nrm, bins

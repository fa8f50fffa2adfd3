"""ctypes binding of the C ABI in include/vbnn_hip.h (vbnn_amd/lib/libvbnn_hip.so).

There is NO fallback: if the shared library is missing, or a call returns a non-zero status,
this module raises. The product path never routes through oracle/ or through PyTorch math.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# VBNN_HIP_LIB: another build of the same library (A/B builds; the name lua/vbnn_ffi.lua reads too)
LIB_PATH = os.environ.get("VBNN_HIP_LIB") or os.path.join(_HERE, "lib", "libvbnn_hip.so")
CSRC = os.path.join(_HERE, "csrc")

OK = 0
F32, BF16 = 0, 1
CHAIN_DX_FIRST, CHAIN_DW_FIRST = 0, 1      # VBNN_CHAIN_DX_FIRST, VBNN_CHAIN_DW_FIRST (vbnn_backward_chain's order)
DEBUG_LAST_CHAINED, DEBUG_CHAIN_OFF = 15, 16   # VBNN_DEBUG_LAST_CHAINED (vbnn_debug_get), VBNN_DEBUG_CHAIN_OFF (vbnn_debug_set)
PACK_COPY, PACK_EXP, PACK_SQUARE, PACK_MUL, PACK_RELU, PACK_RELU_SQUARE = range(6)
KPAD = 64
STREAM_EPS, STREAM_ZETA, STREAM_INIT, STREAM_DATA, STREAM_HEINIT, STREAM_ACQUIRE = 1, 2, 3, 4, 5, 6

_vp, _i64, _u64, _u32, _f, _i = C.c_void_p, C.c_int64, C.c_uint64, C.c_uint32, C.c_float, C.c_int


class VbnnError(RuntimeError):
    pass


class FwdArgs(C.Structure):
    _fields_ = [("w", _vp), ("w2", _vp), ("x", _vp), ("x2", _vp), ("ld_w", _i64), ("ld_x", _i64),
                ("N", _i64), ("I", _i64), ("O", _i64), ("bias", _vp),
                ("seed", _u64), ("layer", _u32), ("draw", _u32), ("row0", _i64),
                ("y", _vp), ("ld_y", _i64), ("r", _vp), ("ld_r", _i64), ("r_packed", _i), ("relu", _i),
                ("h", _vp), ("h2", _vp), ("ld_h", _i64), ("hT", _vp), ("h2T", _vp), ("ld_hT", _i64), ("rows_per_draw", _i64),
                ("draw_dev", _vp), ("head_w3", _vp), ("head_ld_w", _i64), ("head_C", _i64), ("head_slots", _vp)]


class DxArgs(C.Structure):
    _fields_ = [("wT", _vp), ("w2T", _vp), ("g", _vp), ("gv", _vp), ("ld_wT", _i64), ("ld_g", _i64),
                ("N", _i64), ("I", _i64), ("O", _i64), ("x", _vp), ("ld_x", _i64),
                ("gx", _vp), ("ld_gx", _i64), ("relu_mask", _i), ("r_prev", _vp), ("ld_r_prev", _i64), ("r_prev_packed", _i),
                ("g_prev", _vp), ("gv_prev", _vp), ("ld_gp", _i64),
                ("gT_prev", _vp), ("gvT_prev", _vp), ("ld_gpT", _i64),
                ("w", _vp), ("w2", _vp), ("ld_w", _i64)]


class PrepDesc(C.Structure):          # vbnn_prep_desc
    _fields_ = [("means", _vp), ("lvars", _vp), ("O", _i64), ("I", _i64), ("mu_s", _vp), ("var_s", _vp), ("ld_w", _i64),
                ("muT_s", _vp), ("varT_s", _vp), ("ld_wT", _i64), ("stats", _vp)]


class PackDesc(C.Structure):          # vbnn_pack_desc
    _fields_ = [("src", _vp), ("rows", _i64), ("cols", _i64), ("ld_src", _i64), ("dst", _vp), ("ld_dst", _i64),
                ("dstT", _vp), ("ld_dstT", _i64)]


class AdamCfg(C.Structure):           # vbnn_adam_cfg
    _fields_ = [("lr", _f), ("beta1", _f), ("beta2", _f), ("eps", _f), ("lambda_", _f), ("t", _i64)]


class UpdateDesc(C.Structure):        # vbnn_update_desc
    _fields_ = [("means", _vp), ("lvars", _vp), ("O", _i64), ("I", _i64), ("mu_s", _vp), ("var_s", _vp), ("ld_w", _i64),
                ("muT_s", _vp), ("varT_s", _vp), ("ld_wT", _i64), ("stats", _vp), ("grad_mu", _vp), ("grad_lv", _vp),
                ("m_mu", _vp), ("v_mu", _vp), ("m_lv", _vp), ("v_lv", _vp), ("mu", AdamCfg), ("lv", AdamCfg),
                ("bias", _vp), ("grad_bias", _vp), ("lr_bias", _f), ("B", _f), ("log14", _vp), ("kl_add", _f)]


class DwArgs(C.Structure):
    _fields_ = [("xT", _vp), ("x2T", _vp), ("gT", _vp), ("gvT", _vp), ("ld_n", _i64),
                ("N", _i64), ("I", _i64), ("O", _i64), ("scale", _f), ("accumulate", _i),
                ("gradWeight", _vp), ("gradSum", _vp), ("seed", _u64), ("layer", _u32), ("draw", _u32),
                ("lvars", _vp), ("grad_mu", _vp), ("grad_lv", _vp), ("means", _vp), ("stats", _vp),
                ("B", _f), ("S", _f), ("kl_scale", _f), ("gradBias", _vp),
                ("x", _vp), ("x2", _vp), ("g", _vp), ("gv", _vp), ("ld_x", _i64), ("ld_g", _i64),
                ("mu_s", _vp), ("var_s", _vp), ("ld_w", _i64), ("part", _i), ("draw_dev", _vp)]


class BoxInfo(C.Structure):           # vbnn_box_info
    _fields_ = [("mfma_clock_ghz", C.c_double), ("mfma_tflops", C.c_double), ("mfma_ms", C.c_double), ("hbm_TBps", C.c_double),
                ("hbm_ms", C.c_double), ("hbm_bytes", _i64), ("cus", _i), ("reserved", _i)]


class HeadArgs(C.Structure):          # vbnn_head_args
    _fields_ = [("h", _vp), ("ld_h", _i64), ("w3", _vp), ("ld_w", _i64), ("bias", _vp), ("target", _vp),
                ("N", _i64), ("H", _i64), ("C", _i64), ("rows_per_draw", _i64), ("inv_n", _f), ("accumulate", _i),
                ("logits", _vp), ("out", _vp), ("g_logits", _vp), ("loss_sum_dev", _vp), ("correct_dev", _vp),
                ("gradWeight", _vp), ("gradBias", _vp), ("gradBias_prev", _vp), ("relu_mask", _i), ("r_prev_packed", _i),
                ("r_prev", _vp), ("ld_r_prev", _i64), ("g_prev", _vp), ("gv_prev", _vp), ("ld_gp", _i64),
                ("gT_prev", _vp), ("gvT_prev", _vp), ("ld_gpT", _i64), ("logit_slots", _vp), ("n_slots", _i64)]


class PredictArgs(C.Structure):       # vbnn_predict_args
    _fields_ = [("h", _vp), ("ld_h", _i64), ("w3", _vp), ("ld_w", _i64), ("bias", _vp), ("target", _vp),
                ("R", _i64), ("H", _i64), ("C", _i64), ("S", _i64), ("form", _i), ("first", _i), ("final", _i),
                ("state", _vp), ("probs", _vp), ("log_probs", _vp), ("entropy", _vp), ("expected_entropy", _vp),
                ("mutual_info", _vp), ("pred", _vp), ("totals", _vp)]


PREDICT_STACKED, PREDICT_ACCUMULATE = 0, 1


class MomentsArgs(C.Structure):       # vbnn_moments_args
    _fields_ = [("y", _vp), ("ld_y", _i64), ("target", _vp), ("ld_t", _i64), ("R", _i64), ("D", _i64), ("S", _i64),
                ("form", C.c_int32), ("draw", C.c_int32), ("noise_var", _f), ("state", _vp), ("mean", _vp), ("var", _vp),
                ("ld_out", _i64), ("row_var", _vp), ("row_sq_err", _vp), ("row_log_lik", _vp), ("totals", _vp)]


MOMENTS_STACKED, MOMENTS_ACCUMULATE = 0, 1
MOMENTS_STACKED_MAX_D = 4096          # VBNN_MOMENTS_STACKED_MAX_D


class GaussMomentsArgs(C.Structure):  # vbnn_gauss_moments_args
    _fields_ = [("y", _vp), ("ld_y", _i64), ("target", _vp), ("ld_t", _i64), ("R", _i64), ("D", _i64), ("S", _i64),
                ("form", C.c_int32), ("draw", C.c_int32), ("s_min", _f), ("s_max", _f), ("state", _vp),
                ("mean", _vp), ("var", _vp), ("noise_var", _vp), ("ld_out", _i64), ("row_var", _vp), ("row_noise_var", _vp),
                ("row_sq_err", _vp), ("row_log_lik", _vp), ("totals", _vp)]


GAUSS_MOMENTS_STACKED_MAX_D = 8192    # VBNN_GAUSS_MOMENTS_STACKED_MAX_D


class ClassMomentsArgs(C.Structure):  # vbnn_class_moments_args
    _fields_ = [("y", _vp), ("ld_y", _i64), ("target", _vp), ("R", _i64), ("C", _i64), ("S", _i64),
                ("form", C.c_int32), ("draw", C.c_int32), ("K", _i64), ("state", _vp), ("ld_state", _i64),
                ("probs", _vp), ("log_probs", _vp), ("ld_out", _i64), ("entropy", _vp), ("expected_entropy", _vp),
                ("mutual_info", _vp), ("pred", _vp), ("topk_idx", _vp), ("topk_prob", _vp), ("totals", _vp)]


CLASS_MOMENTS_STACKED_MAX_C = 4096    # VBNN_CLASS_MOMENTS_STACKED_MAX_C
CLASS_MOMENTS_MAX_K = 8               # VBNN_CLASS_MOMENTS_MAX_K


class LabelMomentsArgs(C.Structure):  # vbnn_label_moments_args
    _fields_ = [("y", _vp), ("ld_y", _i64), ("target", _vp), ("ld_t", _i64), ("R", _i64), ("D", _i64), ("S", _i64),
                ("form", C.c_int32), ("draw", C.c_int32), ("state", _vp), ("probs", _vp), ("entropy", _vp), ("mutual_info", _vp),
                ("ld_out", _i64), ("row_entropy", _vp), ("row_mutual_info", _vp), ("row_log_lik", _vp), ("row_marg_log_lik", _vp),
                ("row_hits", _vp), ("totals", _vp)]


LABEL_MOMENTS_STACKED_MAX_D = 4096    # VBNN_LABEL_MOMENTS_STACKED_MAX_D


class QuantilesArgs(C.Structure):     # vbnn_quantiles_args
    _fields_ = [("y", _vp), ("ld_y", _i64), ("draw_stride", _i64), ("target", _vp), ("ld_t", _i64), ("R", _i64), ("D", _i64),
                ("S", _i64), ("kind", C.c_int32), ("Q", C.c_int32), ("p", _f * 8), ("noise_var", _f), ("s_min", _f), ("s_max", _f),
                ("q", _vp), ("ld_q", _i64), ("plane_stride", _i64), ("pit", _vp), ("ld_pit", _i64), ("row_le", _vp),
                ("count_le", _vp)]


QUANT_EMPIRICAL, QUANT_FIXED_NOISE, QUANT_GAUSS = 0, 1, 2
QUANTILES_MAX_S = 128                 # VBNN_QUANTILES_MAX_S
QUANTILES_MAX_Q = 8                   # VBNN_QUANTILES_MAX_Q


class CalibrationArgs(C.Structure):   # vbnn_calibration_args
    _fields_ = [("probs", _vp), ("ld", _i64), ("pred", _vp), ("target", _vp), ("R", _i64), ("C", _i64), ("bins", C.c_int32),
                ("reserved", C.c_int32), ("conf", _vp), ("hit", _vp), ("brier", _vp), ("bin", _vp), ("acc", _vp)]


CALIBRATION_MAX_BINS = 64             # VBNN_CALIBRATION_MAX_BINS


class SelectiveArgs(C.Structure):     # vbnn_selective_args
    _fields_ = [("score", _vp), ("hit", _vp), ("R", _i64), ("Q", C.c_int32), ("reserved", C.c_int32), ("k", _i64 * 32),
                ("tau", _vp), ("counts", _vp)]


SELECTIVE_MAX_Q = 32                  # VBNN_SELECTIVE_MAX_Q


class TopRowsArgs(C.Structure):       # vbnn_top_rows_args
    _fields_ = [("score", _vp), ("exclude", _vp), ("R", _i64), ("k", C.c_int32), ("largest", C.c_int32),
                ("stochastic", C.c_int32), ("beta", _f), ("seed", _u64), ("draw", _u32), ("row0", _i64),
                ("index", _vp), ("value", _vp), ("key", _vp), ("counts", _vp), ("workspace", _vp), ("workspace_bytes", C.c_size_t)]


TOP_ROWS_MAX_K = 4096                 # VBNN_TOP_ROWS_MAX_K


class KcentreArgs(C.Structure):       # vbnn_kcentre_args
    _fields_ = [("feat", _vp), ("ld", _i64), ("weight", _vp), ("exclude", _vp), ("centres", _vp), ("R", _i64), ("D", _i64),
                ("n_centres", C.c_int32), ("k", C.c_int32), ("resume", C.c_int32), ("reserved", C.c_int32),
                ("index", _vp), ("key", _vp), ("dist", _vp), ("min_dist", _vp), ("counts", _vp), ("workspace", _vp),
                ("workspace_bytes", C.c_size_t)]


KCENTRE_MAX_K = 4096                  # VBNN_KCENTRE_MAX_K
KCENTRE_MAX_D = 8192                  # VBNN_KCENTRE_MAX_D


class RankMetricsArgs(C.Structure):   # vbnn_rank_metrics_args
    _fields_ = [("score", _vp), ("ld", _i64), ("target", _vp), ("ld_t", _i64), ("target_class", _vp), ("R", _i64), ("D", _i64),
                ("Q", C.c_int32), ("reserved", C.c_int32), ("tau", _f * 16), ("out", _vp), ("workspace", _vp),
                ("workspace_bytes", C.c_size_t)]


RANK_MAX_Q = 16                       # VBNN_RANK_MAX_Q


class ConformalArgs(C.Structure):     # vbnn_conformal_args
    _fields_ = [("probs", _vp), ("ld", _i64), ("target", _vp), ("R", _i64), ("C", _i64), ("kind", C.c_int32), ("Q", C.c_int32),
                ("qhat", _vp), ("score", _vp), ("size", _vp), ("cut_index", _vp), ("cut_prob", _vp), ("covered", _vp),
                ("member", _vp), ("acc", _vp)]


CONFORMAL_MAX_Q = 8                   # VBNN_CONFORMAL_MAX_Q
CONFORMAL_LAC, CONFORMAL_APS = 0, 1


class ConformalIntervalArgs(C.Structure):     # vbnn_conformal_interval_args
    _fields_ = [("lower", _vp), ("upper", _vp), ("ld", _i64), ("plane_stride", _i64), ("P", C.c_int32), ("Q", C.c_int32),
                ("scale", _vp), ("scale2", _vp), ("ld_s", _i64), ("scale_add", _f), ("scale_is_variance", C.c_int32),
                ("w_min", _f), ("per_column", C.c_int32), ("target", _vp), ("ld_t", _i64), ("R", _i64), ("D", _i64),
                ("qhat", _vp), ("ld_qhat", _i64), ("score", _vp), ("row_score", _vp), ("lo", _vp), ("hi", _vp),
                ("covered", _vp), ("row_covered", _vp), ("acc", _vp)]


class SelectColumnsArgs(C.Structure):         # vbnn_select_columns_args
    _fields_ = [("x", _vp), ("ld", _i64), ("R", _i64), ("D", _i64), ("Q", C.c_int32), ("reserved", C.c_int32), ("k", _i64 * 8),
                ("tau", _vp), ("ld_tau", _i64), ("counts", _vp), ("n_nan", _vp)]


SELECT_COLUMNS_MAX_Q = 8              # VBNN_SELECT_COLUMNS_MAX_Q


class ReluMomentsArgs(C.Structure):   # vbnn_relu_moments_args
    _fields_ = [("m", _vp), ("ld_m", _i64), ("v1", _vp), ("v2", _vp), ("ld_v", _i64), ("N", _i64), ("O", _i64),
                ("a", _vp), ("q", _vp), ("c", _vp), ("ld_out", _i64)]


class LogitDrawsArgs(C.Structure):    # vbnn_logit_draws_args
    _fields_ = [("m", _vp), ("ld_m", _i64), ("v", _vp), ("ld_v", _i64), ("R", _i64), ("C", _i64), ("S", _i64),
                ("seed", _u64), ("layer", _u32), ("draw", _u32), ("row0", _i64), ("y", _vp), ("ld_y", _i64), ("draw_stride", _i64)]


class PruneDesc(C.Structure):         # vbnn_prune_desc
    _fields_ = [("means", _vp), ("lvars", _vp), ("O", _i64), ("I", _i64), ("mu_p", _vp), ("var_p", _vp), ("ld_w", _i64),
                ("stats", _vp), ("mask", _vp)]


class SparseDesc(C.Structure):        # vbnn_sparse_desc
    _fields_ = [("row_ptr", _vp), ("cols", _vp), ("mu_v", _vp), ("var_v", _vp), ("O", _i64), ("I", _i64), ("nnz_cap", _i64),
                ("nnz_dev", _vp), ("idx_bytes", C.c_int32), ("reserved", C.c_int32)]


class SparseFwdArgs(C.Structure):     # vbnn_sparse_fwd_args
    _fields_ = [("row_ptr", _vp), ("cols", _vp), ("mu_v", _vp), ("var_v", _vp), ("idx_bytes", _i64),
                ("xT", _vp), ("x2T", _vp), ("ld_xT", _i64), ("N", _i64), ("I", _i64), ("O", _i64), ("bias", _vp),
                ("seed", _u64), ("layer", _u32), ("draw", _u32), ("row0", _i64), ("y", _vp), ("ld_y", _i64), ("relu", _i64),
                ("h", _vp), ("h2", _vp), ("ld_h", _i64), ("hT", _vp), ("h2T", _vp), ("ld_hT", _i64), ("rows_per_draw", _i64)]


class UnitDesc(C.Structure):          # vbnn_unit_desc
    _fields_ = [("means", _vp), ("lvars", _vp), ("O", _i64), ("I", _i64), ("key", _vp), ("keep", _vp), ("n_keep", _vp)]


class UnitGatherArgs(C.Structure):    # vbnn_unit_gather_args
    _fields_ = [("means", _vp), ("lvars", _vp), ("bias", _vp), ("O", _i64), ("I", _i64), ("rows", _vp), ("n_rows", _i64),
                ("cols", _vp), ("n_cols", _i64), ("dst_means", _vp), ("dst_lvars", _vp), ("dst_bias", _vp)]


_SIGS = {
    "vbnn_abi_version": ([], _i),
    "vbnn_last_error": ([], C.c_char_p),
    "vbnn_debug_set": ([_i, _i], _i),
    "vbnn_debug_get": ([_i], _i),
    "vbnn_kmajor_supported": ([_i64, _i64, _i64], _i),
    "vbnn_kmajor_supported_dw": ([_i64, _i64, _i64, _i], _i),
    "vbnn_ctx_kmajor_supported": ([_vp, _i64, _i64, _i64], _i),
    "vbnn_ctx_kmajor_supported_dw": ([_vp, _i64, _i64, _i64, _i], _i),
    "vbnn_ctx_create": ([_i, _vp, C.POINTER(_vp)], _i),
    "vbnn_ctx_create_cu_budget": ([_i, _i, C.POINTER(_vp)], _i),
    "vbnn_ctx_stream": ([_vp, C.POINTER(_vp), C.POINTER(_i)], _i),
    "vbnn_ctx_destroy": ([_vp], _i),
    "vbnn_ctx_set_stream": ([_vp, _vp], _i),
    "vbnn_sync": ([_vp], _i),
    "vbnn_buf_alloc": ([_vp, C.c_size_t, C.POINTER(_vp)], _i),
    "vbnn_buf_free": ([_vp, _vp], _i),
    "vbnn_buf_zero": ([_vp, _vp, C.c_size_t], _i),
    "vbnn_buf_upload": ([_vp, _vp, _vp, C.c_size_t], _i),
    "vbnn_buf_download": ([_vp, _vp, _vp, C.c_size_t], _i),
    "vbnn_fill_normal": ([_vp, _vp, _i64, _i64, _i64, _u64, _u32, _u32, _u32, _i64, _f], _i),
    "vbnn_fill_normal_hw": ([_vp, _vp, _i64, _i64, _i64, _u64, _u32, _u32, _u32, _i64, _f], _i),
    "vbnn_box_muller_forms": ([_vp, _vp, _vp, _vp, _vp, _i64], _i),
    "vbnn_compute_prior": ([_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp], _i),
    "vbnn_wn_sample": ([_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _u64, _u32, _u32], _i),
    "vbnn_pack": ([_vp, _i, _i, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _i64], _i),
    "vbnn_forward": ([_vp, _i, C.POINTER(FwdArgs)], _i),
    "vbnn_forward_head_slots": ([_vp, _i, _i64, _i64, _i64, _i64], _i),
    "vbnn_head_forward_slots": ([_vp, _vp, _i64, _vp, _vp, _i64, _i64, _f, _vp, _vp, _vp, _i, _vp, _vp, _i64], _i),
    "vbnn_grad_input": ([_vp, _i, C.POINTER(DxArgs)], _i),
    "vbnn_acc_grad_parameters": ([_vp, _i, C.POINTER(DwArgs)], _i),
    "vbnn_backward_pair": ([_vp, _i, C.POINTER(DxArgs), C.POINTER(DwArgs)], _i),
    "vbnn_backward_chain": ([_vp, _i, C.POINTER(DxArgs), C.POINTER(DwArgs), _i], _i),
    "vbnn_head_forward_backward": ([_vp, _i, C.POINTER(HeadArgs)], _i),
    "vbnn_head_predict": ([_vp, _i, C.POINTER(PredictArgs)], _i),
    "vbnn_predict_moments": ([_vp, C.POINTER(MomentsArgs)], _i),
    "vbnn_acc_grad_bias": ([_vp, _i, _vp, _i64, _i64, _i64, _f, _i, _vp], _i),
    "vbnn_prep_layer": ([_vp, _i, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _vp], _i),
    "vbnn_compute_mugrads": ([_vp, _vp, _vp, _f, _f, _vp, _vp, _i64], _i),
    "vbnn_compute_vargrads": ([_vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp, _i64], _i),
    "vbnn_calc_lc": ([_vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _i64], _i),
    "vbnn_pack_input": ([_vp, _i, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _i64], _i),
    "vbnn_adam_step": ([_vp, _vp, _vp, _vp, _vp, _vp, _i64, _f, _f, _f, _f, _f, _i64, _vp], _i),
    "vbnn_sgd_step": ([_vp, _vp, _vp, _i64, _f], _i),
    "vbnn_update": ([_vp, _i, _i, _vp, _vp], _i),
    "vbnn_prepare_masked": ([_vp, _i, _i, _vp, _vp, _vp], _i),
    "vbnn_update_masked": ([_vp, _i, _i, _vp, _vp, _vp], _i),
    "vbnn_calc_lc_masked": ([_vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _i64], _i),
    "vbnn_comm_unique_id": ([_vp], _i),
    "vbnn_comm_create": ([_vp, _i, _i, _vp, C.POINTER(_vp)], _i),
    "vbnn_comm_destroy": ([_vp], _i),
    "vbnn_comm_info": ([_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)], _i),
    "vbnn_allreduce_grads": ([_vp, _vp, _i64], _i),
    "vbnn_comm_finish": ([_vp], _i),
    "vbnn_allreduce_grads_bf16": ([_vp, _vp, _i64], _i),
    "vbnn_cast_grads": ([_vp, _i, _vp, _vp, _i64], _i),
    "vbnn_comm_allgather_u64": ([_vp, _vp, _vp], _i),
    "vbnn_stats_combine": ([_vp, _i, _i, _vp, _vp], _i),
    "vbnn_transpose_packed": ([_vp, _i, _vp, _i64, _i64, _i64, _vp, _i64], _i),
    "vbnn_comm_reduce_scatter": ([_vp, _vp, _i64], _i),
    "vbnn_comm_all_gather": ([_vp, _vp, _i64], _i),
    "vbnn_p2p_reduce_scatter": ([_vp, C.c_size_t, _i64], _i),
    "vbnn_p2p_all_gather": ([_vp, C.c_size_t, _i64], _i),
    "vbnn_p2p_create": ([_vp, _i, _i, C.c_size_t, C.POINTER(_vp), C.POINTER(_vp), _vp], _i),
    "vbnn_p2p_connect": ([_vp, _vp], _i),
    "vbnn_p2p_allreduce": ([_vp, C.c_size_t, _i64], _i),
    "vbnn_p2p_finish": ([_vp], _i),
    "vbnn_p2p_status": ([_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(C.c_uint)], _i),
    "vbnn_p2p_set_timeout": ([_vp, C.c_double], _i),
    "vbnn_p2p_clear_status": ([_vp], _i),
    "vbnn_p2p_destroy": ([_vp], _i),
    "vbnn_p2p_set_grid": ([_vp, _i, _i], _i),
    "vbnn_p2p_standin": ([_vp, _i, C.c_double], _i),
    "vbnn_box_calibrate": ([_vp, C.POINTER(BoxInfo)], _i),
    "vbnn_sample": ([_vp, _vp, _u32], _i),
    "vbnn_capture_begin": ([_vp], _i),
    "vbnn_capture_end": ([_vp, C.POINTER(_vp)], _i),
    "vbnn_graph_launch": ([_vp], _i),
    "vbnn_graph_info": ([_vp, C.POINTER(_i), C.POINTER(_i)], _i),
    "vbnn_graph_destroy": ([_vp], _i),
    "vbnn_relu_forward": ([_vp, _vp, _vp, _i64], _i),
    "vbnn_relu_backward": ([_vp, _vp, _vp, _vp, _i64], _i),
    "vbnn_logsoftmax_nll": ([_vp, _vp, _i64, _vp, _i64, _i64, _f, _vp, _vp, _vp, _vp], _i),
    "vbnn_prepare": ([_vp, _i, _i, _vp, _vp], _i),
    "vbnn_head_forward": ([_vp, _i, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i64, _i64, _f, _vp, _vp, _vp, _i, _vp, _vp, _i64], _i),
    "vbnn_head_backward": ([_vp, _i, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _i, _vp, _vp, _vp, _i, _vp, _i64, _i, _vp,
                           _vp, _i64, _vp, _vp, _i64], _i),
    "vbnn_mse_forward": ([_vp, _vp, _i64, _vp, _i64, _i64, _i64, _f, _vp, _i64, _i, _vp], _i),
    "vbnn_mse_backward": ([_vp, _vp, _i64, _vp, _i64, _i64, _i64, _f, _vp, _i64], _i),
    "vbnn_gauss_nll_forward": ([_vp, _vp, _i64, _vp, _i64, _i64, _i64, _f, _f, _f, _vp, _i64, _i, _vp], _i),
    "vbnn_gauss_nll_backward": ([_vp, _vp, _i64, _vp, _i64, _i64, _i64, _f, _f, _f, _vp, _i64], _i),
    "vbnn_predict_gauss_moments": ([_vp, C.POINTER(GaussMomentsArgs)], _i),
    "vbnn_bce_forward": ([_vp, _vp, _i64, _vp, _i64, _i64, _i64, _f, _vp, _i64, _i, _vp, _vp], _i),
    "vbnn_bce_backward": ([_vp, _vp, _i64, _vp, _i64, _i64, _i64, _f, _vp, _i64], _i),
    "vbnn_predict_label_moments": ([_vp, C.POINTER(LabelMomentsArgs)], _i),
    "vbnn_predict_class_moments": ([_vp, C.POINTER(ClassMomentsArgs)], _i),
    "vbnn_predict_quantiles": ([_vp, C.POINTER(QuantilesArgs)], _i),
    "vbnn_predict_calibration": ([_vp, C.POINTER(CalibrationArgs)], _i),
    "vbnn_selective": ([_vp, C.POINTER(SelectiveArgs)], _i),
    "vbnn_conformal": ([_vp, C.POINTER(ConformalArgs)], _i),
    "vbnn_conformal_interval": ([_vp, C.POINTER(ConformalIntervalArgs)], _i),
    "vbnn_select_columns": ([_vp, C.POINTER(SelectColumnsArgs)], _i),
    "vbnn_top_rows_workspace_bytes": ([_i64, C.c_int32, C.POINTER(C.c_size_t)], _i),
    "vbnn_top_rows": ([_vp, C.POINTER(TopRowsArgs)], _i),
    "vbnn_kcentre_workspace_bytes": ([_i64, _i64, C.c_int32, C.POINTER(C.c_size_t)], _i),
    "vbnn_kcentre": ([_vp, C.POINTER(KcentreArgs)], _i),
    "vbnn_rank_metrics_workspace_bytes": ([_i64, _i64, C.POINTER(C.c_size_t)], _i),
    "vbnn_rank_metrics": ([_vp, C.POINTER(RankMetricsArgs)], _i),
    "vbnn_relu_moments": ([_vp, _i, C.POINTER(ReluMomentsArgs)], _i),
    "vbnn_square_shadow": ([_vp, _i, _vp, _i64, _i64, _i64, _vp, _i64], _i),
    "vbnn_logit_draws": ([_vp, C.POINTER(LogitDrawsArgs)], _i),
    "vbnn_snr": ([_vp, _vp, _vp, _i64, _vp], _i),
    "vbnn_prune_workspace_bytes": ([_i, _vp, C.POINTER(C.c_size_t)], _i),
    "vbnn_prune_select": ([_vp, _i, _vp, _i64, _vp, _vp, C.c_size_t], _i),
    "vbnn_prune_pack": ([_vp, _i, _i, _vp, _vp, _f], _i),
    "vbnn_prune_compress": ([_vp, _i, _i, _vp, _vp, _vp, _f], _i),
    "vbnn_forward_sparse": ([_vp, _i, C.POINTER(SparseFwdArgs)], _i),
    "vbnn_unit_snr": ([_vp, _i, _vp], _i),
    "vbnn_unit_select": ([_vp, _i, _vp, _i64, _vp], _i),
    "vbnn_unit_index": ([_vp, _i, _vp, _vp, _f, _i64], _i),
    "vbnn_unit_gather": ([_vp, C.POINTER(UnitGatherArgs)], _i),
    "vbnn_digest": ([_vp, _vp, _u64, _u64, _vp], _i),
    "vbnn_nll_forward": ([_vp, _vp, _i64, _vp, _i64, _i64, _f, _vp, _vp], _i),
    "vbnn_nll_backward": ([_vp, _vp, _i64, _i64, _f, _vp], _i),
    "vbnn_logsoftmax_backward": ([_vp, _vp, _vp, _vp, _i64, _i64], _i),
}


def exported_symbols():
    """Every symbol include/vbnn_hip.h declares (kept in step by tests/test_abi.py)."""
    return sorted(_SIGS)


def build(verbose=False):
    """Compile libvbnn_hip.so for gfx950 with hipcc (vbnn_amd/csrc/Makefile)."""
    cmd = ["make", "-C", CSRC, "-j4"] + ([] if verbose else ["-s"])
    subprocess.check_call(cmd)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise VbnnError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU or PyTorch fallback.")
        L = C.CDLL(LIB_PATH)
        for name, (args, res) in _SIGS.items():
            fn = getattr(L, name)       # AttributeError if the library does not export it
            fn.argtypes = args
            fn.restype = res
        _lib = L
    return _lib


def check(status):
    if status != OK:
        msg = lib().vbnn_last_error()
        raise VbnnError(f"libvbnn_hip status {status}: {msg.decode() if msg else '?'}")


def pad_ld(k):
    return (int(k) + KPAD - 1) // KPAD * KPAD

"""ctypes binding of librcdm_hip.so (include/rcdm.h).  Thin: tensors stay owned by torch, only
`data_ptr()` integers and the current HIP stream handle cross the boundary.  There is NO CPU
fallback: if the library is missing or a call fails this module raises."""
import ctypes as C
import os
import sys

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RCDM_LIB") or os.path.join(_HERE, "lib", "librcdm_hip.so")  # RCDM_LIB: kernel experiments

EPI_BIAS, EPI_ROWVEC, EPI_RESIDUAL, EPI_GEGLU, EPI_GELU, EPI_QUICK_GELU, EPI_RELU = 1, 2, 4, 8, 16, 32, 64

_ERR = {-1: "RCDM_EINVAL", -2: "RCDM_ESHAPE", -3: "RCDM_ELAUNCH", -4: "RCDM_EWORKSPACE", -5: "RCDM_ECOMM"}


class RcdmError(RuntimeError):
    pass


class GemmDesc(C.Structure):
    _fields_ = [("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("lda", C.c_int32), ("ldc", C.c_int32), ("ldr", C.c_int32),
                ("epilogue", C.c_int32), ("rows_per_sample", C.c_int32), ("ldt", C.c_int32),
                ("out_scale", C.c_float), ("split_k", C.c_int32), ("dup_rows", C.c_int32)]


class LnFuse(C.Structure):
    _fields_ = [("gamma", C.c_void_p), ("beta", C.c_void_p), ("pe", C.c_void_p), ("out", C.c_void_p), ("ld", C.c_int32),
                ("rows_per_frame", C.c_int32), ("frames", C.c_int32), ("eps", C.c_float)]


class Lnx(C.Structure):
    _fields_ = [("stat_out", C.c_void_p), ("stat_parts", C.c_int32), ("stat_out_rows", C.c_int32), ("stat_in", C.c_void_p),
                ("parts_in", C.c_int32), ("stat_in_rows", C.c_int32), ("colsum", C.c_void_p), ("eps", C.c_float), ("C", C.c_int32)]


class ConvDesc(C.Structure):
    _fields_ = [("n_img", C.c_int32), ("h_in", C.c_int32), ("w_in", C.c_int32),
                ("c_in", C.c_int32), ("c_out", C.c_int32), ("stride", C.c_int32),
                ("upsample", C.c_int32), ("lda", C.c_int32), ("ldc", C.c_int32), ("ldr", C.c_int32),
                ("epilogue", C.c_int32), ("rows_per_sample", C.c_int32), ("ldt", C.c_int32),
                ("out_scale", C.c_float), ("split_k", C.c_int32), ("pad_after_only", C.c_int32),
                ("dup_rows", C.c_int32), ("c_in2", C.c_int32), ("lda2", C.c_int32)]


class GroupNormDesc(C.Structure):
    _fields_ = [("samples", C.c_int32), ("rows_per_sample", C.c_int32), ("C", C.c_int32),
                ("groups", C.c_int32), ("ldx", C.c_int32), ("ldy", C.c_int32),
                ("eps", C.c_float), ("silu", C.c_int32)]


class LayerNormDesc(C.Structure):
    _fields_ = [("M", C.c_int32), ("C", C.c_int32), ("ldx", C.c_int32), ("ldy", C.c_int32),
                ("eps", C.c_float), ("rows_per_frame", C.c_int32), ("frames", C.c_int32)]


class FFDesc(C.Structure):
    _fields_ = [("M", C.c_int32), ("C", C.c_int32), ("ldx", C.c_int32), ("ldo", C.c_int32), ("eps", C.c_float)]


class RowChainDesc(C.Structure):
    _fields_ = [("M", C.c_int32), ("C", C.c_int32), ("lda", C.c_int32), ("ldr", C.c_int32), ("ldt", C.c_int32),
                ("ldo", C.c_int32), ("tail", C.c_int32), ("rows_per_frame", C.c_int32), ("frames", C.c_int32),
                ("eps", C.c_float), ("gn_groups", C.c_int32), ("gn_rows", C.c_int32), ("ldz", C.c_int32)]


class AttnDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("heads", C.c_int32), ("Lq", C.c_int32), ("Lk", C.c_int32),
                ("d", C.c_int32), ("ldq", C.c_int32), ("ldk", C.c_int32), ("ldv", C.c_int32),
                ("ldo", C.c_int32), ("scale", C.c_float), ("flags", C.c_int32)]


ATTN_WIDE_RANGE = 1   # AttnDesc.flags: scores not bounded below 2^15 -> never the matrix-pipe-softmax (MSUB) kernel


class TemporalAttnDesc(C.Structure):
    _fields_ = [("samples", C.c_int32), ("frames", C.c_int32), ("pixels", C.c_int32),
                ("heads", C.c_int32), ("d", C.c_int32), ("ldqkv", C.c_int32), ("ldo", C.c_int32),
                ("scale", C.c_float)]


class ResampleDesc(C.Structure):
    _fields_ = [("src_pitch", C.c_int64), ("src_stride", C.c_int64), ("dst_pitch", C.c_int64), ("dst_stride", C.c_int64),
                ("n", C.c_int32), ("channels", C.c_int32), ("in_h", C.c_int32), ("in_w", C.c_int32),
                ("out_h", C.c_int32), ("out_w", C.c_int32), ("taps_x", C.c_int32), ("taps_y", C.c_int32),
                ("tile_rows", C.c_int32), ("flip_channels", C.c_int32), ("mode", C.c_int32), ("ld", C.c_int32),
                ("c_pad", C.c_int32), ("mean", C.c_float * 3), ("std", C.c_float * 3)]


class FramesU8Desc(C.Structure):
    _fields_ = [("dst_pitch", C.c_int64), ("dst_stride", C.c_int64), ("n", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("channels", C.c_int32), ("src_kind", C.c_int32), ("ld", C.c_int32)]


class Conv2dDesc(C.Structure):
    _fields_ = [("n_img", C.c_int32), ("h_in", C.c_int32), ("w_in", C.c_int32), ("c_in", C.c_int32), ("c_out", C.c_int32),
                ("kh", C.c_int32), ("kw", C.c_int32), ("stride_h", C.c_int32), ("stride_w", C.c_int32),
                ("pad_h", C.c_int32), ("pad_w", C.c_int32), ("lda", C.c_int32), ("ldc", C.c_int32), ("epilogue", C.c_int32)]


class Pool2dDesc(C.Structure):
    _fields_ = [("n_img", C.c_int32), ("h_in", C.c_int32), ("w_in", C.c_int32), ("c", C.c_int32),
                ("kh", C.c_int32), ("kw", C.c_int32), ("stride_h", C.c_int32), ("stride_w", C.c_int32),
                ("pad_h", C.c_int32), ("pad_w", C.c_int32), ("ld_in", C.c_int32), ("ld_out", C.c_int32), ("mode", C.c_int32)]


class BilinearDesc(C.Structure):
    _fields_ = [("src_pitch", C.c_int64), ("src_stride", C.c_int64), ("n", C.c_int32), ("channels", C.c_int32),
                ("in_h", C.c_int32), ("in_w", C.c_int32), ("out_h", C.c_int32), ("out_w", C.c_int32),
                ("flip_channels", C.c_int32), ("ld", C.c_int32), ("c_pad", C.c_int32),
                ("scale", C.c_float * 3), ("shift", C.c_float * 3)]


class LpipsHeadDesc(C.Structure):
    _fields_ = [("lda", C.c_int64), ("ldb", C.c_int64), ("pairs", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("c", C.c_int32),
                ("blocks", C.c_int32), ("reserved", C.c_int32)]


class LpipsInputDesc(C.Structure):
    _fields_ = [("src_pitch", C.c_int64), ("src_stride", C.c_int64), ("n", C.c_int32), ("in_h", C.c_int32), ("in_w", C.c_int32),
                ("space_to_depth", C.c_int32), ("ld", C.c_int32), ("mul", C.c_float * 3), ("add", C.c_float * 3)]


class PngDesc(C.Structure):
    _fields_ = [("src_pitch", C.c_int64), ("src_stride", C.c_int64), ("dst_stride", C.c_int64), ("n", C.c_int32),
                ("h", C.c_int32), ("w", C.c_int32), ("channels", C.c_int32), ("filter", C.c_int32)]


class PngFile(C.Structure):
    _fields_ = [("src_offset", C.c_uint64), ("src_bytes", C.c_uint64), ("dst_offset", C.c_uint64), ("ws_offset", C.c_uint64),
                ("zlib_bytes", C.c_uint64), ("dst_pitch", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32),
                ("color_type", C.c_uint32), ("idat_first", C.c_uint32), ("idat_count", C.c_uint32), ("plte_offset", C.c_uint32),
                ("plte_entries", C.c_uint32)]


class PngIdat(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("bytes", C.c_uint32), ("reserved", C.c_uint32)]


class MetricsDesc(C.Structure):
    _fields_ = [("a_pitch", C.c_int64), ("a_stride", C.c_int64), ("b_pitch", C.c_int64), ("b_stride", C.c_int64),
                ("n", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("channels", C.c_int32), ("window", C.c_int32),
                ("sample_covariance", C.c_int32)]


class FStatsDesc(C.Structure):
    _fields_ = [("ld", C.c_int64), ("n", C.c_int32), ("d", C.c_int32), ("dtype", C.c_int32), ("reserved", C.c_int32)]


class JacobiDesc(C.Structure):
    _fields_ = [("ld", C.c_int64), ("rows", C.c_int32), ("len", C.c_int32), ("dim", C.c_int32), ("reserved", C.c_int32)]


class CholeskyDesc(C.Structure):
    _fields_ = [("ld", C.c_int64), ("ldf", C.c_int64), ("d", C.c_int32), ("nb", C.c_int32)]


class MmdDesc(C.Structure):
    _fields_ = [("ldx", C.c_int64), ("ldy", C.c_int64), ("nx", C.c_int32), ("ny", C.c_int32), ("d", C.c_int32),
                ("subsets", C.c_int32), ("m", C.c_int32), ("degree", C.c_int32), ("dtype", C.c_int32),
                ("gamma", C.c_double), ("coef0", C.c_double), ("flags", C.c_uint32)]


class KnnDesc(C.Structure):
    _fields_ = [("ld", C.c_int64), ("n", C.c_int32), ("d", C.c_int32), ("k", C.c_int32), ("dtype", C.c_int32),
                ("col_chunks", C.c_int32), ("flags", C.c_uint32)]


class PrdcDesc(C.Structure):
    _fields_ = [("ldx", C.c_int64), ("ldy", C.c_int64), ("nx", C.c_int32), ("ny", C.c_int32), ("d", C.c_int32),
                ("dtype", C.c_int32), ("col_chunks", C.c_int32), ("flags", C.c_uint32)]


class LabelDesc(C.Structure):
    _fields_ = [("ld_logits", C.c_int64), ("ld_labels", C.c_int64), ("n", C.c_int32), ("classes", C.c_int32), ("dtype", C.c_int32),
                ("flags", C.c_uint32)]


class IscDesc(C.Structure):
    _fields_ = [("ld", C.c_int64), ("n", C.c_int32), ("classes", C.c_int32), ("splits", C.c_int32), ("dtype", C.c_int32),
                ("chunks_per_block", C.c_int32), ("flags", C.c_uint32)]


class TokAdded(C.Structure):
    _fields_ = [("text", C.c_uint8 * 32), ("len", C.c_int32), ("id", C.c_int32), ("special", C.c_int32), ("reserved", C.c_int32)]


class TokenizeDesc(C.Structure):
    _fields_ = [("ld", C.c_int64), ("text_bytes", C.c_int64), ("n", C.c_int32), ("max_length", C.c_int32), ("truncation", C.c_int32),
                ("bos_id", C.c_int32), ("eos_id", C.c_int32), ("pad_id", C.c_int32), ("n_added", C.c_int32),
                ("pair_slots", C.c_uint32)]


TOK_MAX_CAPTION, TOK_MAX_ADDED, TOK_MAX_ROWS, TOK_MAX_ADDED_LEN, TOK_MAX_RANK, TOK_MAX_CAPTIONS = 1024, 64, 66, 32, 1 << 22, 1 << 20
FSTATS_F32, FSTATS_F16 = 0, 1                            # FStatsDesc.dtype
FRECHET_MAX_DIM = 4096
KID_MAX_M, KID_MAX_SUBSETS, KID_MAX_DEGREE = 65536, 65535, 8   # kid::MAX_M, MAX_SUBSETS, MAX_DEGREE (d: FRECHET_MAX_DIM)
PRDC_MAX_K, PRDC_MAX_N, PRDC_MAX_CHUNKS = 16, 65536, 1024      # prdc::MAX_K, MAX_N, MAX_CHUNKS (d: FRECHET_MAX_DIM)
SCORES_MAX_LABEL_CLASSES, SCORES_MIN_CLASSES, SCORES_MAX_CLASSES = 64, 2, 4096    # sc::MAX_LABEL_CLASSES, MIN_CLASSES, MAX_CLASSES
SCORES_MAX_SPLITS, SCORES_MAX_N, SCORES_MAX_CHUNKS_PER_BLOCK = 65535, 1 << 30, 64  # sc::MAX_SPLITS, MAX_N, MAX_CHUNKS_PER_BLOCK
CHOLESKY_NB = 16                                          # fr::CHOL_NB, the panel width CholeskyDesc.nb = 0 stands for
SSIM_UNIFORM7, SSIM_GAUSS11 = 0, 1                        # MetricsDesc.window
PNG_BLOCK, PNG_SLOT, PNG_ADAPTIVE = 32768, 41728, -1      # RCDM_PNG_*
PNG_RGB, PNG_BGR = 0, 1
PNG_STATUS = {1: "RCDM_PNG_EZLIB", 2: "RCDM_PNG_ETRUNC", 3: "RCDM_PNG_EBLOCK", 4: "RCDM_PNG_ESTORED", 5: "RCDM_PNG_ECODES",
              6: "RCDM_PNG_ESYMBOL", 7: "RCDM_PNG_EDISTANCE", 8: "RCDM_PNG_EOVERRUN", 9: "RCDM_PNG_EUNDERRUN",
              10: "RCDM_PNG_EADLER", 11: "RCDM_PNG_EFILTER"}
IMAGE_TILE = 32                                         # RCDM_IMAGE_TILE
IMAGE_U8, IMAGE_F32_NCHW, IMAGE_F16_ROWS = 0, 1, 2      # ResampleDesc.mode
FRAMES_F16_ROWS, FRAMES_F32_NCHW = 0, 1                 # FramesU8Desc.src_kind
POOL_MAX, POOL_AVG_INCLUDE_PAD, POOL_AVG_EXCLUDE_PAD = 0, 1, 2   # Pool2dDesc.mode
LPIPS_MAX_C, LPIPS_TILE, LPIPS_MAX_PAIRS = 512, 64, 65535       # lp::MAX_C, TILE, MAX_PAIRS

# every symbol include/rcdm.h declares: name -> (restype, argtypes)
_P, _I, _F, _SZ = C.c_void_p, C.c_int32, C.c_float, C.c_size_t
SYMBOLS = {
    "rcdm_version": (C.c_int, []),
    "rcdm_last_hip_error": (C.c_int, []),
    "rcdm_last_hip_error_string": (C.c_char_p, []),
    "rcdm_gemm_ln": (C.c_int, [C.POINTER(GemmDesc), C.POINTER(LnFuse), _P, _P, _P, _P, _P, _P]),
    "rcdm_gemm_stat_parts": (C.c_int, [C.POINTER(GemmDesc)]),
    "rcdm_gemm_lnx_stat_parts": (C.c_int, [C.POINTER(GemmDesc), _I]),
    "rcdm_gemm_lnx_parts_ok": (C.c_int, [C.POINTER(GemmDesc), _I, _I]),
    "rcdm_gemm_plan_query": (C.c_int, [C.POINTER(GemmDesc), _I, _I, C.POINTER(C.c_int32)]),
    "rcdm_conv3x3_plan_query": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(C.c_int32)]),
    "rcdm_gemm_lnx_workspace_bytes": (C.c_size_t, [C.POINTER(GemmDesc), _I, _I]),
    "rcdm_set_groupnorm_fold": (C.c_int, [_I]),
    "rcdm_gemm_lnx": (C.c_int, [C.POINTER(GemmDesc), C.POINTER(Lnx), _P, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "rcdm_gemm_workspace_bytes": (_SZ, [C.POINTER(GemmDesc)]),
    "rcdm_set_igemm_variant": (C.c_int, [_I]),
    "rcdm_set_shape_rules": (C.c_int, [C.c_char_p]),
    "rcdm_set_igemm_pingpong": (C.c_int, [_I]),
    "rcdm_debug_set_igemm_trace": (C.c_int, [_P]),
    "rcdm_debug_set_attn_trace": (C.c_int, [_P]),
    "rcdm_debug_mfma_peak": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P]),
    "rcdm_gemm": (C.c_int, [C.POINTER(GemmDesc), _P, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "rcdm_conv3x3_workspace_bytes": (_SZ, [C.POINTER(ConvDesc)]),
    "rcdm_conv3x3": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "rcdm_conv3x3_add1x1": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "rcdm_conv3x3_add1x1_gnstat": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(GroupNormDesc), _P, _P, _P, _P, _P, _P, _P, _P, _SZ, _P, _SZ, _P]),
    "rcdm_groupnorm_workspace_bytes": (_SZ, [C.POINTER(GroupNormDesc)]),
    "rcdm_groupnorm_silu": (C.c_int, [C.POINTER(GroupNormDesc), _P, _P, _P, _P, _P, _SZ, _P]),
    "rcdm_groupnorm_stats": (C.c_int, [C.POINTER(GroupNormDesc), _P, _P, _P, _SZ, _P]),
    "rcdm_groupnorm_stats_prestat": (C.c_int, [C.POINTER(GroupNormDesc), _P, _P, _SZ, _P]),
    "rcdm_groupnorm_prestat_ok": (C.c_int, [C.POINTER(GroupNormDesc)]),
    "rcdm_groupnorm_silu_prestat": (C.c_int, [C.POINTER(GroupNormDesc), _P, _P, _P, _P, _P, _SZ, _P]),
    "rcdm_gemm_gnstat_ok": (C.c_int, [C.POINTER(GemmDesc), C.POINTER(GroupNormDesc)]),
    "rcdm_gemm_gnstat": (C.c_int, [C.POINTER(GemmDesc), C.POINTER(GroupNormDesc), _P, _P, _P, _P, _P, _P, _P, _SZ, _P, _SZ, _P]),
    "rcdm_conv3x3_gnstat_ok": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(GroupNormDesc)]),
    "rcdm_conv3x3_gnstat": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(GroupNormDesc), _P, _P, _P, _P, _P, _P, _P, _SZ, _P, _SZ, _P]),
    "rcdm_softmax_rows": (C.c_int, [_I, _I, _I, _I, C.c_float, _P, _P, _P]),
    "rcdm_layernorm": (C.c_int, [C.POINTER(LayerNormDesc), _P, _P, _P, _P, _P, _P]),
    "rcdm_flash_attn": (C.c_int, [C.POINTER(AttnDesc), _P, _P, _P, _P, _P]),
    "rcdm_flash_attn_masked": (C.c_int, [C.POINTER(AttnDesc), _P, _P, _P, _P, _I, _P, _P]),
    "rcdm_temporal_attn": (C.c_int, [C.POINTER(TemporalAttnDesc), _P, _P, _P]),
    "rcdm_ff_stream_bytes": (_SZ, [_I]),
    "rcdm_ff_fused_supported": (C.c_int, [_I]),
    "rcdm_pack_ff_stream": (C.c_int, [_P, _P, _P, _I, _P, _P, _P]),
    "rcdm_ff_fused": (C.c_int, [C.POINTER(FFDesc), _P, _P, _P, _P, _P, _P, _P, _P]),
    "rcdm_rowchain_supported": (C.c_int, [_I]),
    "rcdm_rowchain_config_supported": (C.c_int, [_I, _I, _I]),
    "rcdm_rowchain_stream_bytes": (_SZ, [_I, _I]),
    "rcdm_pack_rowchain": (C.c_int, [_P, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "rcdm_rowchain": (C.c_int, [C.POINTER(RowChainDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "rcdm_timestep_embed": (C.c_int, [_P, _I, _I, _P, _P]),
    "rcdm_small_linear": (C.c_int, [_P, _I, _I, _P, _P, _I, _I, _I, _P, _P]),
    "rcdm_assemble_input": (C.c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _I, _P]),
    "rcdm_ncfhw_to_rows": (C.c_int, [_P, _I, _I, _I, _I, _I, _P, _I, _I, _P]),
    "rcdm_rows_to_ncfhw": (C.c_int, [_P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "rcdm_cfg_ddim_step": (C.c_int, [_P, _I, _P, _I, _I, _I, _I, _I, _F, _P, _P, _P]),
    "rcdm_cfg_pndm_step": (C.c_int, [_P, _I, _P, _P, _I, _I, _I, _I, _I, _F, _P, _P, _P]),
    "rcdm_cfg_sigma_step": (C.c_int, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _P, _P, _P]),
    "rcdm_cfg_rescale_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "rcdm_cfg_rescale_factor": (C.c_int, [_P, _I, _I, _I, _I, _I, _F, _F, _P, _SZ, _P, _P]),
    "rcdm_cfg_ddim_step_scaled": (C.c_int, [_P, _I, _P, _I, _I, _I, _I, _I, _F, _P, _P, _P, _P]),
    "rcdm_cfg_pndm_step_scaled": (C.c_int, [_P, _I, _P, _P, _I, _I, _I, _I, _I, _F, _P, _P, _P, _P]),
    "rcdm_cfg_sigma_step_scaled": (C.c_int, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _P, _P, _P, _P]),
    "rcdm_prior_assemble": (C.c_int, [_P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _P]),
    "rcdm_cfg_unclip_step": (C.c_int, [_P, _I, _P, _I, _I, _I, C.c_float, C.c_float, _P, _P, _P, _P]),
    "rcdm_embed_tokens": (C.c_int, [_P, _I, _I, _P, _I, _P, _I, _P, _I, _P]),
    "rcdm_patch_rows": (C.c_int, [_P, _I, _I, _I, _I, _P, _I, _P]),
    "rcdm_load_timestep": (C.c_int, [_P, _P, _P, _I, _P]),
    "rcdm_image_resample_lds_bytes": (_SZ, [C.POINTER(ResampleDesc)]),
    "rcdm_image_resample": (C.c_int, [C.POINTER(ResampleDesc), _P, _P, _P, _P, _P, _P, _P]),
    "rcdm_frames_to_u8": (C.c_int, [C.POINTER(FramesU8Desc), _P, _P, _P]),
    "rcdm_conv2d": (C.c_int, [C.POINTER(Conv2dDesc), _P, _P, _P, _P, _P]),
    "rcdm_pool2d": (C.c_int, [C.POINTER(Pool2dDesc), _P, _P, _P]),
    "rcdm_global_avgpool": (C.c_int, [_I, _I, _I, _P, C.c_int64, _P, C.c_int64, _P]),
    "rcdm_image_bilinear_rows": (C.c_int, [C.POINTER(BilinearDesc), _P, _P, _P]),
    "rcdm_lpips_head_workspace_bytes": (_SZ, [C.POINTER(LpipsHeadDesc)]),
    "rcdm_lpips_head": (C.c_int, [C.POINTER(LpipsHeadDesc), _P, _P, _P, _P, _P, _SZ, _P]),
    "rcdm_lpips_input_sides": (C.c_int, [C.POINTER(LpipsInputDesc), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rcdm_lpips_input_rows": (C.c_int, [C.POINTER(LpipsInputDesc), _P, _P, _P]),
    "rcdm_png_bound": (_SZ, [C.POINTER(PngDesc)]),
    "rcdm_png_workspace_bytes": (_SZ, [C.POINTER(PngDesc)]),
    "rcdm_png_encode": (C.c_int, [C.POINTER(PngDesc), _P, _P, _P, _P, _P]),
    "rcdm_png_match_workspace_bytes": (_SZ, [C.POINTER(PngDesc)]),
    "rcdm_png_encode_match": (C.c_int, [C.POINTER(PngDesc), _P, _P, _P, _P, _P]),
    "rcdm_png_decode_workspace_bytes": (_SZ, [_P, C.c_int]),
    "rcdm_png_decode": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    "rcdm_frame_metrics_workspace_bytes": (_SZ, [C.POINTER(MetricsDesc)]),
    "rcdm_frame_metrics": (C.c_int, [C.POINTER(MetricsDesc), _P, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "rcdm_feature_stats_update": (C.c_int, [C.POINTER(FStatsDesc), _P, _P, _P, _P, _P]),
    "rcdm_gemm_tn_f64": (C.c_int, [_I, _I, _I, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, _P]),
    "rcdm_feature_stats_finalize": (C.c_int, [_I, C.c_int64, _P, _P, _P, _P, _P, _P, _P]),
    "rcdm_frechet_trace": (C.c_int, [_I, _P, _P, _P]),
    "rcdm_frechet_mean_term": (C.c_int, [_I, _P, _P, _P, _P]),
    "rcdm_jacobi_workspace_bytes": (_SZ, [C.POINTER(JacobiDesc)]),
    "rcdm_jacobi_sweep": (C.c_int, [C.POINTER(JacobiDesc), _P, _P, _P, _SZ, _P]),
    "rcdm_jacobi_norm_sum": (C.c_int, [C.POINTER(JacobiDesc), _P, _P, _P, _SZ, _P]),
    "rcdm_frechet_factor": (C.c_int, [C.POINTER(JacobiDesc), _P, _P, C.c_int64, _P, _P, _SZ, _P]),
    "rcdm_cholesky_workspace_bytes": (_SZ, [C.POINTER(CholeskyDesc)]),
    "rcdm_cholesky_pivoted_f64": (C.c_int, [C.POINTER(CholeskyDesc), _P, _P, _P, _P, _SZ, _P]),
    "rcdm_poly_mmd_workspace_bytes": (_SZ, [C.POINTER(MmdDesc)]),
    "rcdm_poly_mmd": (C.c_int, [C.POINTER(MmdDesc), _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "rcdm_poly_gram_f64": (C.c_int, [C.POINTER(MmdDesc), _P, _P, _P, _P, _P, C.c_int64, _P]),
    "rcdm_row_norms2_f64": (C.c_int, [_P, _I, _I, C.c_int64, _I, _P, _P]),
    "rcdm_knn_radii2_workspace_bytes": (_SZ, [C.POINTER(KnnDesc)]),
    "rcdm_knn_radii2": (C.c_int, [C.POINTER(KnnDesc), _P, _P, _P, _SZ, _P]),
    "rcdm_prdc_counts_workspace_bytes": (_SZ, [C.POINTER(PrdcDesc)]),
    "rcdm_prdc_counts": (C.c_int, [C.POINTER(PrdcDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "rcdm_label_state_len": (C.c_int64, [_I]),
    "rcdm_label_counts_workspace_bytes": (_SZ, [C.POINTER(LabelDesc)]),
    "rcdm_label_counts": (C.c_int, [C.POINTER(LabelDesc), _P, _P, _P, _P, _P, _SZ, _P]),
    "rcdm_inception_score_workspace_bytes": (_SZ, [C.POINTER(IscDesc)]),
    "rcdm_inception_score": (C.c_int, [C.POINTER(IscDesc), _P, _P, _P, _P, _P, _SZ, _P]),
    "rcdm_diffuse_assemble": (C.c_int, [_P, _P, _P, _F, _P, _P, _I, _P, _P, _I, _I, _I, _I, _P, _I, _I, _P]),
    "rcdm_eps_sqerr_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "rcdm_eps_sqerr": (C.c_int, [_P, _I, _P, _P, _F, _I, _I, _I, _I, _I, _P, _P, _SZ, _P]),
    "rcdm_tok_pair_hash": (C.c_uint32, [C.c_uint32, C.c_uint32]),
    "rcdm_clip_tokenize_workspace_bytes": (_SZ, [C.POINTER(TokenizeDesc)]),
    "rcdm_clip_tokenize": (C.c_int, [C.POINTER(TokenizeDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "rcdm_xattn_image_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "rcdm_xattn_pack_kv": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "rcdm_xattn": (C.c_int, [C.POINTER(AttnDesc), _P, _P, _P, _P]),
    "rcdm_advance_step": (C.c_int, [_P, _P]),
    "rcdm_load_table_row": (C.c_int, [_P, _P, _P, C.c_size_t, _P]),
    "rcdm_pack_f16": (C.c_int, [_P, _P, _SZ, _P]),
    "rcdm_mish": (C.c_int, [_P, _P, _SZ, _P]),
    "rcdm_pack_conv3x3": (C.c_int, [_P, _I, _I, _I, _P, _P]),
    "rcdm_pack_conv3x3_up2": (C.c_int, [_P, _I, _I, _P, _P]),
    "rcdm_matmul_f32": (C.c_int, [_P, _P, _P, _I, _I, _I, _P]),
    "rcdm_conv3x3_up2_supported": (C.c_int, [C.POINTER(ConvDesc)]),
    "rcdm_conv3x3_wino_supported": (C.c_int, [C.POINTER(ConvDesc)]),
    "rcdm_conv3x3_wino_workspace_bytes": (_SZ, [C.POINTER(ConvDesc)]),
    "rcdm_conv3x3_wino_plan_query": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(C.c_int32)]),
    "rcdm_pack_conv3x3_wino": (C.c_int, [_P, _I, _I, _P, _P]),
    "rcdm_set_wino_slab_f16": (C.c_int, [_I]),
    "rcdm_upsample_taps_gather": (C.c_int, [_P, _I, _I, _I, _I, _I, _P, _P, _I, _P]),
    "rcdm_conv_taps_gather": (C.c_int, [_P, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P]),
    "rcdm_set_splitk_slab_f16": (C.c_int, [_I]),
    "rcdm_conv3x3_wino": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(GroupNormDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _SZ,
                                    C.POINTER(GroupNormDesc), _P, _P]),
    "rcdm_groupnorm_finalize": (C.c_int, [_I, _I, _I, C.c_float, _P, _P, _P]),
    "rcdm_groupnorm_apply": (C.c_int, [C.POINTER(GroupNormDesc), _P, _P, _P, _P, _P, _P]),
    "rcdm_pack_geglu_rows": (C.c_int, [_P, _P, _I, _I, _P, _P, _P]),
    "rcdm_graph_begin_capture": (C.c_int, [_P]),
    "rcdm_graph_end_capture": (C.c_int, [_P, C.POINTER(C.c_void_p)]),
    "rcdm_graph_launch": (C.c_int, [_P, _P]),
    "rcdm_graph_destroy": (C.c_int, [_P]),
    "rcdm_event_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "rcdm_event_record": (C.c_int, [_P, _P]),
    "rcdm_event_elapsed_ms": (C.c_int, [_P, _P, C.POINTER(C.c_float)]),
    "rcdm_event_destroy": (C.c_int, [_P]),
    "rcdm_stream_synchronize": (C.c_int, [_P]),
    "rcdm_comm_unique_id": (C.c_int, [_P]),
    "rcdm_comm_create": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(_P)]),
    "rcdm_comm_destroy": (C.c_int, [_P]),
    "rcdm_bcast": (C.c_int, [_P, _P, C.c_size_t, C.c_int32, _P]),
    "rcdm_allgather": (C.c_int, [_P, _P, _P, C.c_size_t, _P]),
    "rcdm_comm_last_error": (C.c_int, []),
}

_lib = None


def load():
    """Load the shared library (once) and type every declared symbol.  Raises if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RcdmError(
            f"{LIB_PATH} not found: the HIP extension is not built (run `python -m rcdms_amd.build`); "
            "rcdms_amd has no CPU fallback by design")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _check(rc, what):
    if rc != 0:
        lib = load()
        extra = ""
        if rc == -3:
            extra = f" (hip error {lib.rcdm_last_hip_error()}: {lib.rcdm_last_hip_error_string().decode()})"
        if rc == -5:
            extra = f" (ncclResult {lib.rcdm_comm_last_error()}; 0 = librccl could not be opened)"
        raise RcdmError(f"{what} failed: {_ERR.get(rc, rc)}{extra}")


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return 0 if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------
# thin typed wrappers (all enqueue on torch's current stream unless `stream` is given)

def set_shape_rules(rules):
    """Per-shape tile rules "taps,M,N,Cin,variant,split;..." ("off": no table; None: back to RCDM_SHAPE_RULES)."""
    _check(load().rcdm_set_shape_rules(None if rules is None else rules.encode()), "rcdm_set_shape_rules")


def set_igemm_variant(v):
    _check(load().rcdm_set_igemm_variant(v), "rcdm_set_igemm_variant")


def set_igemm_pingpong(on):
    _check(load().rcdm_set_igemm_pingpong(int(bool(on))), "rcdm_set_igemm_pingpong")


def gemm_workspace_bytes(desc):
    return load().rcdm_gemm_workspace_bytes(C.byref(desc))


def gemm(desc, A, W, bias, rowvec, residual, out, ws_ptr=0, ws_bytes=0, stream=None):
    _check(load().rcdm_gemm(C.byref(desc), A, W, bias, rowvec, residual, out, ws_ptr, ws_bytes,
                            stream_ptr() if stream is None else stream), "rcdm_gemm")


def conv3x3_workspace_bytes(desc):
    return load().rcdm_conv3x3_workspace_bytes(C.byref(desc))


def conv3x3(desc, x, W, bias, rowvec, residual, out, ws_ptr=0, ws_bytes=0, stream=None):
    _check(load().rcdm_conv3x3(C.byref(desc), x, W, bias, rowvec, residual, out, ws_ptr, ws_bytes,
                               stream_ptr() if stream is None else stream), "rcdm_conv3x3")


def conv3x3_add1x1(desc, x, x2, W, bias, rowvec, residual, out, ws_ptr=0, ws_bytes=0, stream=None):
    _check(load().rcdm_conv3x3_add1x1(C.byref(desc), x, x2, W, bias, rowvec, residual, out, ws_ptr, ws_bytes,
                                      stream_ptr() if stream is None else stream), "rcdm_conv3x3_add1x1")


def groupnorm_workspace_bytes(desc):
    return load().rcdm_groupnorm_workspace_bytes(C.byref(desc))


def groupnorm_silu(desc, x, gamma, beta, y, ws_ptr, ws_bytes, stream=None):
    _check(load().rcdm_groupnorm_silu(C.byref(desc), x, gamma, beta, y, ws_ptr, ws_bytes,
                                      stream_ptr() if stream is None else stream), "rcdm_groupnorm_silu")


def groupnorm_silu_prestat(desc, x, gamma, beta, y, ws_ptr, ws_bytes, stream=None):
    _check(load().rcdm_groupnorm_silu_prestat(C.byref(desc), x, gamma, beta, y, ws_ptr, ws_bytes,
                                              stream_ptr() if stream is None else stream), "rcdm_groupnorm_silu_prestat")


def groupnorm_prestat_ok(desc):
    return bool(load().rcdm_groupnorm_prestat_ok(C.byref(desc)))


def gemm_gnstat_ok(desc, gn):
    return bool(load().rcdm_gemm_gnstat_ok(C.byref(desc), C.byref(gn)))


def gemm_gnstat(desc, gn, A, W, bias, rowvec, residual, out, ws_ptr, ws_bytes, gn_ws_ptr, gn_ws_bytes, stream=None):
    _check(load().rcdm_gemm_gnstat(C.byref(desc), C.byref(gn), A, W, bias, rowvec, residual, out, ws_ptr, ws_bytes, gn_ws_ptr,
                                   gn_ws_bytes, stream_ptr() if stream is None else stream), "rcdm_gemm_gnstat")


def conv3x3_gnstat_ok(desc, gn):
    return bool(load().rcdm_conv3x3_gnstat_ok(C.byref(desc), C.byref(gn)))


def conv3x3_gnstat(desc, gn, x, W, bias, rowvec, residual, out, ws_ptr, ws_bytes, gn_ws_ptr, gn_ws_bytes, stream=None):
    _check(load().rcdm_conv3x3_gnstat(C.byref(desc), C.byref(gn), x, W, bias, rowvec, residual, out, ws_ptr, ws_bytes, gn_ws_ptr,
                                      gn_ws_bytes, stream_ptr() if stream is None else stream), "rcdm_conv3x3_gnstat")


def conv3x3_add1x1_gnstat(desc, gn, x, x2, W, bias, rowvec, residual, out, ws_ptr, ws_bytes, gn_ws_ptr, gn_ws_bytes, stream=None):
    _check(load().rcdm_conv3x3_add1x1_gnstat(C.byref(desc), C.byref(gn), x, x2, W, bias, rowvec, residual, out, ws_ptr, ws_bytes,
                                             gn_ws_ptr, gn_ws_bytes, stream_ptr() if stream is None else stream),
           "rcdm_conv3x3_add1x1_gnstat")


def groupnorm_stats(desc, x, stat, ws_ptr, ws_bytes, stream=None):
    _check(load().rcdm_groupnorm_stats(C.byref(desc), x, stat, ws_ptr, ws_bytes,
                                       stream_ptr() if stream is None else stream), "rcdm_groupnorm_stats")


def groupnorm_stats_prestat(desc, stat, ws_ptr, ws_bytes, stream=None):
    _check(load().rcdm_groupnorm_stats_prestat(C.byref(desc), stat, ws_ptr, ws_bytes,
                                               stream_ptr() if stream is None else stream), "rcdm_groupnorm_stats_prestat")


def layernorm(desc, x, gamma, beta, pe, y, stream=None):
    _check(load().rcdm_layernorm(C.byref(desc), x, gamma, beta, pe, y,
                                 stream_ptr() if stream is None else stream), "rcdm_layernorm")


def softmax_rows(M, N, ldx, ldy, scale, x, y, stream=None):
    _check(load().rcdm_softmax_rows(M, N, ldx, ldy, scale, x, y, stream_ptr() if stream is None else stream),
           "rcdm_softmax_rows")


def gemm_ln(desc, ln, a, w, bias, residual, out, stream=None):
    _check(load().rcdm_gemm_ln(C.byref(desc), C.byref(ln), a, w, bias, residual, out,
                               stream_ptr() if stream is None else stream), "rcdm_gemm_ln")


def set_groupnorm_fold(on):
    _check(load().rcdm_set_groupnorm_fold(int(on)), "rcdm_set_groupnorm_fold")


def gemm_stat_parts(desc, consumer=False):
    """Column-tile count (= statistics slots per row) of a statistics-producing launch of this shape; consumer: the launch
    also consumes a deferred LayerNorm (both flags steer the tile choice: rcdm_gemm_lnx_stat_parts)."""
    if consumer:
        return int(load().rcdm_gemm_lnx_stat_parts(C.byref(desc), 1))
    return int(load().rcdm_gemm_stat_parts(C.byref(desc)))


_PLAN_FIELDS = ("variant", "bm", "bn", "tiles_m", "tiles_n", "splits", "blocks_per_cu", "k_steps")


def gemm_plan_query(desc, producer=False, consumer=False):
    out = (C.c_int32 * 8)()
    _check(load().rcdm_gemm_plan_query(C.byref(desc), int(bool(producer)), int(bool(consumer)), out), "rcdm_gemm_plan_query")
    return dict(zip(_PLAN_FIELDS, out))


def conv3x3_plan_query(desc):
    out = (C.c_int32 * 8)()
    _check(load().rcdm_conv3x3_plan_query(C.byref(desc), out), "rcdm_conv3x3_plan_query")
    return dict(zip(_PLAN_FIELDS, out))


def gemm_lnx_parts_ok(desc, parts, consumer=False):
    return bool(load().rcdm_gemm_lnx_parts_ok(C.byref(desc), int(parts), int(bool(consumer))))


def gemm_lnx_workspace_bytes(desc, producer=False, consumer=False):
    return int(load().rcdm_gemm_lnx_workspace_bytes(C.byref(desc), int(bool(producer)), int(bool(consumer))))


def gemm_lnx(desc, lnx, a, w, bias, rowvec, residual, out, workspace, workspace_bytes, stream=None):
    _check(load().rcdm_gemm_lnx(C.byref(desc), C.byref(lnx), a, w, bias, rowvec, residual, out, workspace, workspace_bytes,
                                stream_ptr() if stream is None else stream), "rcdm_gemm_lnx")


def flash_attn(desc, q, k, v, out, stream=None):
    _check(load().rcdm_flash_attn(C.byref(desc), q, k, v, out,
                                  stream_ptr() if stream is None else stream), "rcdm_flash_attn")


def flash_attn_masked(desc, q, k, v, key_valid, causal, out, stream=None):
    _check(load().rcdm_flash_attn_masked(C.byref(desc), q, k, v, key_valid, int(causal), out,
                                         stream_ptr() if stream is None else stream), "rcdm_flash_attn_masked")


def temporal_attn(desc, qkv, out, stream=None):
    _check(load().rcdm_temporal_attn(C.byref(desc), qkv, out,
                                     stream_ptr() if stream is None else stream), "rcdm_temporal_attn")


def ff_stream_bytes(Cc):
    return load().rcdm_ff_stream_bytes(Cc)


def ff_fused_supported(Cc):
    return bool(load().rcdm_ff_fused_supported(Cc))


def rowchain_supported(Cc):
    return bool(load().rcdm_rowchain_supported(Cc))


def rowchain_config_supported(Cc, tail, pe_frames=0):
    return bool(load().rcdm_rowchain_config_supported(Cc, tail, pe_frames))


def rowchain_stream_bytes(Cc, tail):
    return load().rcdm_rowchain_stream_bytes(Cc, tail)


def pack_rowchain(wa, Cc, tail, wt, w1, b1, w2, wstream, b1p, stream=None):
    _check(load().rcdm_pack_rowchain(wa, Cc, tail, wt, w1, b1, w2, wstream, b1p,
                                     stream_ptr() if stream is None else stream), "rcdm_pack_rowchain")


def rowchain(desc, a_in, res, tok, a_bias, ln_g, ln_b, pe, wstream, b1p, b2, out, stream=None, gn_stat=None, gn_g=None,
             gn_b=None, z_res=None, z_bias=None):
    _check(load().rcdm_rowchain(C.byref(desc), a_in, res, tok, a_bias, ln_g, ln_b, pe, wstream, b1p, b2, out,
                                gn_stat, gn_g, gn_b, z_res, z_bias, stream_ptr() if stream is None else stream), "rcdm_rowchain")


def pack_ff_stream(w1, b1, w2, Cc, wstream, b1p, stream=None):
    _check(load().rcdm_pack_ff_stream(w1, b1, w2, Cc, wstream, b1p, stream_ptr() if stream is None else stream),
           "rcdm_pack_ff_stream")


def ff_fused(desc, x, ln_g, ln_b, wstream, b1p, b2, out, stream=None):
    _check(load().rcdm_ff_fused(C.byref(desc), x, ln_g, ln_b, wstream, b1p, b2, out,
                                stream_ptr() if stream is None else stream), "rcdm_ff_fused")


def timestep_embed(t, rows, dim, out, stream=None):
    _check(load().rcdm_timestep_embed(t, rows, dim, out, stream_ptr() if stream is None else stream),
           "rcdm_timestep_embed")


def small_linear(x, rows, K, W, bias, N, silu_in, silu_out, out, stream=None):
    _check(load().rcdm_small_linear(x, rows, K, W, bias, N, silu_in, silu_out, out,
                                    stream_ptr() if stream is None else stream), "rcdm_small_linear")


def prior_assemble(base, temb, latents, n_lat, tok, x16, B, L, Cc, E, time_row, stream=None):
    _check(load().rcdm_prior_assemble(base, temb, latents, n_lat, tok, x16, B, L, Cc, E, time_row,
                                      stream_ptr() if stream is None else stream), "rcdm_prior_assemble")


def cfg_unclip_step(pred, ld, latents, n, reps, E, guidance_scale, clip_range, coef, noise, step_counter, stream=None):
    _check(load().rcdm_cfg_unclip_step(pred, ld, latents, n, reps, E, guidance_scale, clip_range, coef, noise,
                                       step_counter, stream_ptr() if stream is None else stream), "rcdm_cfg_unclip_step")


def embed_tokens(ids, n_rows, L, table, vocab, pos, Cc, out, ldo, stream=None):
    _check(load().rcdm_embed_tokens(ids, n_rows, L, table, vocab, pos, Cc, out, ldo,
                                    stream_ptr() if stream is None else stream), "rcdm_embed_tokens")


def patch_rows(pixels, B, H, W, patch, out, ldk, stream=None):
    _check(load().rcdm_patch_rows(pixels, B, H, W, patch, out, ldk, stream_ptr() if stream is None else stream),
           "rcdm_patch_rows")


def image_resample_lds_bytes(desc):
    return int(load().rcdm_image_resample_lds_bytes(C.byref(desc)))


def image_resample(desc, src, kx, bx, ky, by, dst, stream=None):
    _check(load().rcdm_image_resample(C.byref(desc), src, kx, bx, ky, by, dst, stream_ptr() if stream is None else stream),
           "rcdm_image_resample")


def frames_to_u8(desc, src, dst, stream=None):
    _check(load().rcdm_frames_to_u8(C.byref(desc), src, dst, stream_ptr() if stream is None else stream), "rcdm_frames_to_u8")


def conv2d(desc, x, W, bias, out, stream=None):
    _check(load().rcdm_conv2d(C.byref(desc), x, W, bias, out, stream_ptr() if stream is None else stream), "rcdm_conv2d")


def pool2d(desc, x, out, stream=None):
    _check(load().rcdm_pool2d(C.byref(desc), x, out, stream_ptr() if stream is None else stream), "rcdm_pool2d")


def global_avgpool(n_img, rows_per_img, c, x, ld, out, ldo, stream=None):
    _check(load().rcdm_global_avgpool(n_img, rows_per_img, c, x, ld, out, ldo, stream_ptr() if stream is None else stream),
           "rcdm_global_avgpool")


def image_bilinear_rows(desc, src, dst, stream=None):
    _check(load().rcdm_image_bilinear_rows(C.byref(desc), src, dst, stream_ptr() if stream is None else stream),
           "rcdm_image_bilinear_rows")


def lpips_head_workspace_bytes(desc):
    return load().rcdm_lpips_head_workspace_bytes(C.byref(desc))


def lpips_head(desc, a, b, lin, out, workspace, workspace_bytes, stream=None):
    _check(load().rcdm_lpips_head(C.byref(desc), a, b, lin, out, workspace, workspace_bytes,
                                  stream_ptr() if stream is None else stream), "rcdm_lpips_head")


def lpips_input_sides(desc):
    """-> (out_h, out_w, channels) of the rows rcdm_lpips_input_rows writes for this descriptor."""
    h, w, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _check(load().rcdm_lpips_input_sides(C.byref(desc), C.byref(h), C.byref(w), C.byref(c)), "rcdm_lpips_input_sides")
    return h.value, w.value, c.value


def lpips_input_rows(desc, src, dst, stream=None):
    _check(load().rcdm_lpips_input_rows(C.byref(desc), src, dst, stream_ptr() if stream is None else stream),
           "rcdm_lpips_input_rows")


def png_bound(desc):
    return int(load().rcdm_png_bound(C.byref(desc)))


def png_workspace_bytes(desc):
    return int(load().rcdm_png_workspace_bytes(C.byref(desc)))


def png_encode(desc, src, workspace, dst, sizes, stream=None):
    _check(load().rcdm_png_encode(C.byref(desc), src, workspace, dst, sizes, stream_ptr() if stream is None else stream),
           "rcdm_png_encode")


def png_file_workspace(zlib_bytes, raw_bytes):
    """RCDM_PNG_FILE_WORKSPACE: the bytes of one file's workspace region."""
    return ((zlib_bytes + 15) & ~15) + ((raw_bytes + 15) & ~15)


def png_decode_workspace_bytes(files, n):
    """files: a host (PngFile * n) array."""
    return int(load().rcdm_png_decode_workspace_bytes(C.addressof(files), n))


def png_decode(files, idats, n, n_idat, order, src, workspace, dst, status, stream=None):
    """files / idats / status: device pointers."""
    _check(load().rcdm_png_decode(files, idats, n, n_idat, order, src, workspace, dst, status,
                                  stream_ptr() if stream is None else stream), "rcdm_png_decode")


def png_match_workspace_bytes(desc):
    return int(load().rcdm_png_match_workspace_bytes(C.byref(desc)))


def png_encode_match(desc, src, workspace, dst, sizes, stream=None):
    _check(load().rcdm_png_encode_match(C.byref(desc), src, workspace, dst, sizes, stream_ptr() if stream is None else stream),
           "rcdm_png_encode_match")


def clip_tokenize_workspace_bytes(desc):
    return int(load().rcdm_clip_tokenize_workspace_bytes(C.byref(desc)))


def clip_tokenize(desc, text, offsets, byte_ids, added, pairs, input_ids, attention_mask, lengths, pool_index, workspace=0,
                  workspace_bytes=0, stream=None):
    _check(load().rcdm_clip_tokenize(C.byref(desc), text, offsets, byte_ids, added, pairs, input_ids, attention_mask, lengths,
                                     pool_index, workspace, workspace_bytes, stream_ptr() if stream is None else stream),
           "rcdm_clip_tokenize")


def _st(stream):
    return stream_ptr() if stream is None else stream


def feature_stats_update(desc, x, shift, sum_, outer, stream=None):
    _check(load().rcdm_feature_stats_update(C.byref(desc), x, shift, sum_, outer, _st(stream)), "rcdm_feature_stats_update")


def gemm_tn_f64(m, n, k, a, lda, b, ldb, c, ldc, stream=None):
    _check(load().rcdm_gemm_tn_f64(m, n, k, a, lda, b, ldb, c, ldc, _st(stream)), "rcdm_gemm_tn_f64")


def feature_stats_finalize(d, n, shift, sum_, outer, mean, cov, trace, stream=None):
    _check(load().rcdm_feature_stats_finalize(d, n, shift, sum_, outer, mean, cov, trace, _st(stream)), "rcdm_feature_stats_finalize")


def frechet_trace(d, a, out, stream=None):
    _check(load().rcdm_frechet_trace(d, a, out, _st(stream)), "rcdm_frechet_trace")


def frechet_mean_term(d, mu_a, mu_b, out, stream=None):
    _check(load().rcdm_frechet_mean_term(d, mu_a, mu_b, out, _st(stream)), "rcdm_frechet_mean_term")


def jacobi_workspace_bytes(desc):
    return int(load().rcdm_jacobi_workspace_bytes(C.byref(desc)))


def jacobi_sweep(desc, w, count, workspace, workspace_bytes, stream=None):
    _check(load().rcdm_jacobi_sweep(C.byref(desc), w, count, workspace, workspace_bytes, _st(stream)), "rcdm_jacobi_sweep")


def jacobi_norm_sum(desc, w, out, workspace, workspace_bytes, stream=None):
    _check(load().rcdm_jacobi_norm_sum(C.byref(desc), w, out, workspace, workspace_bytes, _st(stream)), "rcdm_jacobi_norm_sum")


def frechet_factor(desc, w, f, ldf, rank, workspace, workspace_bytes, stream=None):
    _check(load().rcdm_frechet_factor(C.byref(desc), w, f, ldf, rank, workspace, workspace_bytes, _st(stream)), "rcdm_frechet_factor")


def cholesky_workspace_bytes(desc):
    return int(load().rcdm_cholesky_workspace_bytes(C.byref(desc)))


def cholesky_pivoted_f64(desc, a, f, rank, workspace, workspace_bytes, stream=None):
    _check(load().rcdm_cholesky_pivoted_f64(C.byref(desc), a, f, rank, workspace, workspace_bytes, _st(stream)),
           "rcdm_cholesky_pivoted_f64")


def poly_mmd_workspace_bytes(desc):
    return int(load().rcdm_poly_mmd_workspace_bytes(C.byref(desc)))


def poly_mmd(desc, x, y, ix, iy, out, workspace, workspace_bytes, stream=None):
    _check(load().rcdm_poly_mmd(C.byref(desc), x, y, ix, iy, out, workspace, workspace_bytes, _st(stream)), "rcdm_poly_mmd")


def poly_gram_f64(desc, x, y, ix, iy, out, ldo, stream=None):
    _check(load().rcdm_poly_gram_f64(C.byref(desc), x, y, ix, iy, out, ldo, _st(stream)), "rcdm_poly_gram_f64")


def row_norms2_f64(x, n, d, ld, dtype, out, stream=None):
    _check(load().rcdm_row_norms2_f64(x, n, d, ld, dtype, out, _st(stream)), "rcdm_row_norms2_f64")


def knn_radii2_workspace_bytes(desc):
    return int(load().rcdm_knn_radii2_workspace_bytes(C.byref(desc)))


def knn_radii2(desc, x, r2, workspace, workspace_bytes, stream=None):
    _check(load().rcdm_knn_radii2(C.byref(desc), x, r2, workspace, workspace_bytes, _st(stream)), "rcdm_knn_radii2")


def prdc_counts_workspace_bytes(desc):
    return int(load().rcdm_prdc_counts_workspace_bytes(C.byref(desc)))


def prdc_counts(desc, x, y, rx2, ry2, out, fake_count, real_hit, real_min2, workspace, workspace_bytes, stream=None):
    _check(load().rcdm_prdc_counts(C.byref(desc), x, y, rx2, ry2, out, fake_count, real_hit, real_min2, workspace, workspace_bytes,
                                   _st(stream)), "rcdm_prdc_counts")


def label_state_len(classes):
    return int(load().rcdm_label_state_len(classes))


def label_counts_workspace_bytes(desc):
    return int(load().rcdm_label_counts_workspace_bytes(C.byref(desc)))


def label_counts(desc, logits, labels, thresholds, state, workspace, workspace_bytes, stream=None):
    _check(load().rcdm_label_counts(C.byref(desc), logits, labels, thresholds, state, workspace, workspace_bytes, _st(stream)),
           "rcdm_label_counts")


def inception_score_workspace_bytes(desc):
    return int(load().rcdm_inception_score_workspace_bytes(C.byref(desc)))


def inception_score(desc, logits, order, kl_out, row_h, workspace, workspace_bytes, stream=None):
    _check(load().rcdm_inception_score(C.byref(desc), logits, order, kl_out, row_h, workspace, workspace_bytes, _st(stream)),
           "rcdm_inception_score")


def diffuse_assemble(x0, noise, offs, offs_scale, t, table, T, mask, masked, B, frames, H, W, out, ld, c_pad, stream=None):
    """offs: 0 (no noise offset) or the address of the fp32 (B,4,f) draw; t: int64[B] on the device."""
    _check(load().rcdm_diffuse_assemble(x0, noise, offs, offs_scale, t, table, T, mask, masked, B, frames, H, W, out, ld, c_pad,
                                        _st(stream)), "rcdm_diffuse_assemble")


def eps_sqerr_workspace_bytes(B, frames, H, W):
    return int(load().rcdm_eps_sqerr_workspace_bytes(B, frames, H, W))


def eps_sqerr(eps, ld, noise, offs, offs_scale, B, frames, H, W, out, workspace, workspace_bytes, blocks=0, stream=None):
    _check(load().rcdm_eps_sqerr(eps, ld, noise, offs, offs_scale, B, frames, H, W, blocks, out, workspace, workspace_bytes,
                                 _st(stream)), "rcdm_eps_sqerr")


def frame_metrics_workspace_bytes(desc):
    return int(load().rcdm_frame_metrics_workspace_bytes(C.byref(desc)))


def frame_metrics(desc, a, b, win, ssim, sse, sad, workspace, workspace_bytes, stream=None):
    _check(load().rcdm_frame_metrics(C.byref(desc), a, b, win, ssim, sse, sad, workspace, workspace_bytes,
                                     stream_ptr() if stream is None else stream), "rcdm_frame_metrics")


def assemble_input(lat, mask, masked, S, reps, frames, H, W, out, ld, c_pad, stream=None):
    _check(load().rcdm_assemble_input(lat, mask, masked, S, reps, frames, H, W, out, ld, c_pad,
                                      stream_ptr() if stream is None else stream), "rcdm_assemble_input")


def ncfhw_to_rows(x, b, Cc, frames, H, W, out, ld, c_pad, stream=None):
    _check(load().rcdm_ncfhw_to_rows(x, b, Cc, frames, H, W, out, ld, c_pad,
                                     stream_ptr() if stream is None else stream), "rcdm_ncfhw_to_rows")


def rows_to_ncfhw(rows, ld, b, Cc, frames, H, W, out, stream=None):
    _check(load().rcdm_rows_to_ncfhw(rows, ld, b, Cc, frames, H, W, out,
                                     stream_ptr() if stream is None else stream), "rcdm_rows_to_ncfhw")


def cfg_pndm_step(eps, ld, lat, hist, S, reps, frames, H, W, gs, table, step, stream=None):
    _check(load().rcdm_cfg_pndm_step(eps, ld, lat, hist, S, reps, frames, H, W, gs, table, step,
                                     stream_ptr() if stream is None else stream), "rcdm_cfg_pndm_step")


def cfg_sigma_step(eps, ld, lat, model_in, hist, noise, S, reps, frames, H, W, gs, table, step, stream=None):
    _check(load().rcdm_cfg_sigma_step(eps, ld, lat, model_in, hist, noise, S, reps, frames, H, W, gs, table, step,
                                      stream_ptr() if stream is None else stream), "rcdm_cfg_sigma_step")


def cfg_rescale_workspace_bytes(S, frames, H, W):
    return load().rcdm_cfg_rescale_workspace_bytes(S, frames, H, W)


def cfg_rescale_factor(eps, ld, S, frames, H, W, gs, phi, ws, ws_bytes, factor, stream=None):
    """factor[s] = phi * std(eps_c) / std(eps_u + gs (eps_c - eps_u)) + 1 - phi per story (guidance rescale), two launches."""
    _check(load().rcdm_cfg_rescale_factor(eps, ld, S, frames, H, W, gs, phi, ws, ws_bytes, factor,
                                          stream_ptr() if stream is None else stream), "rcdm_cfg_rescale_factor")


def cfg_pndm_step_scaled(eps, ld, lat, hist, S, reps, frames, H, W, gs, table, step, factor, stream=None):
    _check(load().rcdm_cfg_pndm_step_scaled(eps, ld, lat, hist, S, reps, frames, H, W, gs, table, step, factor or None,
                                            stream_ptr() if stream is None else stream), "rcdm_cfg_pndm_step_scaled")


def cfg_sigma_step_scaled(eps, ld, lat, model_in, hist, noise, S, reps, frames, H, W, gs, table, step, factor, stream=None):
    _check(load().rcdm_cfg_sigma_step_scaled(eps, ld, lat, model_in, hist, noise, S, reps, frames, H, W, gs, table, step,
                                             factor or None, stream_ptr() if stream is None else stream),
           "rcdm_cfg_sigma_step_scaled")


def cfg_ddim_step_scaled(eps, ld, lat, S, reps, frames, H, W, gs, coef, step, factor, stream=None):
    _check(load().rcdm_cfg_ddim_step_scaled(eps, ld, lat, S, reps, frames, H, W, gs, coef, step, factor or None,
                                            stream_ptr() if stream is None else stream), "rcdm_cfg_ddim_step_scaled")


def cfg_ddim_step(eps, ld, lat, S, reps, frames, H, W, gs, coef, step, stream=None):
    _check(load().rcdm_cfg_ddim_step(eps, ld, lat, S, reps, frames, H, W, gs, coef, step,
                                     stream_ptr() if stream is None else stream), "rcdm_cfg_ddim_step")


def load_timestep(ts, step, t_out, rows, stream=None):
    _check(load().rcdm_load_timestep(ts, step, t_out, rows, stream_ptr() if stream is None else stream),
           "rcdm_load_timestep")


def xattn_image_bytes(batch, heads, d):
    return load().rcdm_xattn_image_bytes(batch, heads, d)


def xattn_pack_kv(k, v, batch, Lk, heads, d, ldk, ldv, image, stream=None):
    _check(load().rcdm_xattn_pack_kv(k, v, batch, Lk, heads, d, ldk, ldv, image,
                                     stream_ptr() if stream is None else stream), "rcdm_xattn_pack_kv")


def xattn(desc, q, image, out, stream=None):
    _check(load().rcdm_xattn(C.byref(desc), q, image, out, stream_ptr() if stream is None else stream), "rcdm_xattn")


def load_table_row(table, step, dst, row_floats, stream=None):
    _check(load().rcdm_load_table_row(table, step, dst, row_floats, stream_ptr() if stream is None else stream),
           "rcdm_load_table_row")


def advance_step(step, stream=None):
    _check(load().rcdm_advance_step(step, stream_ptr() if stream is None else stream), "rcdm_advance_step")


def pack_f16(src, dst, n, stream=None):
    _check(load().rcdm_pack_f16(src, dst, n, stream_ptr() if stream is None else stream), "rcdm_pack_f16")


def mish(x, y, n, stream=None):
    _check(load().rcdm_mish(x, y, n, stream_ptr() if stream is None else stream), "rcdm_mish")


def matmul_f32(a, b):
    """a [n][k] @ b [k][m] (or b [k]) in fp32 on the library's own kernel (rcdm_matmul_f32): weight composition at pack time."""
    import torch
    a = a.contiguous().float()
    vec = b.dim() == 1
    b2 = (b[:, None] if vec else b).contiguous().float()
    n, k = a.shape
    m = b2.shape[1]
    assert b2.shape[0] == k and a.is_cuda and b2.is_cuda
    c = torch.empty(n, m, dtype=torch.float32, device=a.device)
    _check(load().rcdm_matmul_f32(a.data_ptr(), b2.data_ptr(), c.data_ptr(), n, k, m, stream_ptr()), "rcdm_matmul_f32")
    return c[:, 0].contiguous() if vec else c


def pack_conv3x3_up2(w, c_out, c_in, dst, stream=None):
    _check(load().rcdm_pack_conv3x3_up2(w, c_out, c_in, dst, stream_ptr() if stream is None else stream),
           "rcdm_pack_conv3x3_up2")


def conv3x3_up2_supported(desc):
    return bool(load().rcdm_conv3x3_up2_supported(C.byref(desc)))


def upsample_taps_gather(P, ldp, n_img, h, w, c_out, bias, out, ldc, stream=None):
    _check(load().rcdm_upsample_taps_gather(P, ldp, n_img, h, w, c_out, bias, out, ldc, stream_ptr() if stream is None else stream),
           "rcdm_upsample_taps_gather")


def conv_taps_gather(P, ldp, n_img, h, w, c_out, upsample, bias, out, ldc, stream=None):
    _check(load().rcdm_conv_taps_gather(P, ldp, n_img, h, w, c_out, upsample, bias, out, ldc, stream_ptr() if stream is None else stream),
           "rcdm_conv_taps_gather")


def set_splitk_slab_f16(on):
    _check(load().rcdm_set_splitk_slab_f16(on), "rcdm_set_splitk_slab_f16")


def set_wino_slab_f16(on):
    _check(load().rcdm_set_wino_slab_f16(on), "rcdm_set_wino_slab_f16")


def conv3x3_wino_supported(desc):
    return bool(load().rcdm_conv3x3_wino_supported(C.byref(desc)))


def conv3x3_wino_workspace_bytes(desc):
    return load().rcdm_conv3x3_wino_workspace_bytes(C.byref(desc))


def conv3x3_wino_plan_query(desc):
    out = (C.c_int32 * 8)()
    _check(load().rcdm_conv3x3_wino_plan_query(C.byref(desc), out), "rcdm_conv3x3_wino_plan_query")
    return list(out)


def pack_conv3x3_wino(w, c_out, c_in, dst, stream=None):
    _check(load().rcdm_pack_conv3x3_wino(w, c_out, c_in, dst, stream_ptr() if stream is None else stream),
           "rcdm_pack_conv3x3_wino")


def conv3x3_wino(desc, x, U, bias, rowvec, residual, out, ws_ptr, ws_bytes, x2=0, W2=0, gn=None, gn_stat=0, gn_gamma=0, gn_beta=0,
                 gn_out=None, gn_out_partial=0, stream=None):
    """rcdm_conv3x3_wino: gn = GroupNormDesc of the norm (+ SiLU) the input transform applies to x (None: x as it is);
    gn_out = GroupNormDesc of the norm that reads `out` next, its per-tile partial statistics go to gn_out_partial."""
    _check(load().rcdm_conv3x3_wino(C.byref(desc), C.byref(gn) if gn is not None else None, gn_stat, gn_gamma, gn_beta, x, x2, U, W2,
                                    bias, rowvec, residual, out, ws_ptr, ws_bytes, C.byref(gn_out) if gn_out is not None else None,
                                    gn_out_partial, stream_ptr() if stream is None else stream),
           "rcdm_conv3x3_wino")


def groupnorm_apply(desc, x, stat, gamma, beta, y, stream=None):
    _check(load().rcdm_groupnorm_apply(C.byref(desc), x, stat, gamma, beta, y, stream_ptr() if stream is None else stream),
           "rcdm_groupnorm_apply")


def groupnorm_finalize(samples, groups, splits, eps, partial, stat, stream=None):
    _check(load().rcdm_groupnorm_finalize(samples, groups, splits, eps, partial, stat, stream_ptr() if stream is None else stream),
           "rcdm_groupnorm_finalize")


def pack_conv3x3(w, c_out, c_in, cin_pad, dst, stream=None):
    _check(load().rcdm_pack_conv3x3(w, c_out, c_in, cin_pad, dst, stream_ptr() if stream is None else stream),
           "rcdm_pack_conv3x3")


def pack_geglu_rows(w, bias, n_out, K, w_dst, bias_dst, stream=None):
    _check(load().rcdm_pack_geglu_rows(w, bias, n_out, K, w_dst, bias_dst,
                                       stream_ptr() if stream is None else stream), "rcdm_pack_geglu_rows")


class Graph:
    """One captured hipGraph (rcdm_graph_*).  Capture on torch's current stream."""

    def __init__(self):
        self.exec = C.c_void_p(0)
        self.stream = None

    def begin(self):
        self.stream = stream_ptr()
        _check(load().rcdm_graph_begin_capture(self.stream), "rcdm_graph_begin_capture")

    def end(self):
        _check(load().rcdm_graph_end_capture(self.stream, C.byref(self.exec)), "rcdm_graph_end_capture")

    def launch(self, stream=None):
        _check(load().rcdm_graph_launch(self.exec, stream_ptr() if stream is None else stream), "rcdm_graph_launch")

    def __del__(self):
        try:
            if self.exec and _lib is not None:
                _lib.rcdm_graph_destroy(self.exec)
        except Exception:
            pass


class Comm:
    """An RCCL communicator behind the C-ABI (rcdm_comm_*): broadcast / all-gather of raw device bytes on the current
    (or a given) HIP stream.  `unique_id()` on one rank, ship the 128 bytes to the others, then every rank constructs
    Comm(id, nranks, rank) — a collective call."""

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        _check(load().rcdm_comm_unique_id(buf), "rcdm_comm_unique_id")
        return buf.raw

    def __init__(self, unique_id, nranks, rank):
        if len(unique_id) != 128:
            raise ValueError("an RCCL unique id is 128 bytes")
        self.nranks, self.rank = int(nranks), int(rank)
        self.comm = C.c_void_p(0)
        _check(load().rcdm_comm_create(C.create_string_buffer(bytes(unique_id), 128), self.nranks, self.rank,
                                       C.byref(self.comm)), "rcdm_comm_create")

    def bcast(self, ptr, nbytes, root=0, stream=None):
        _check(load().rcdm_bcast(self.comm, ptr, nbytes, root, stream_ptr() if stream is None else stream), "rcdm_bcast")

    def allgather(self, send_ptr, recv_ptr, bytes_per_rank, stream=None):
        _check(load().rcdm_allgather(self.comm, send_ptr, recv_ptr, bytes_per_rank,
                                     stream_ptr() if stream is None else stream), "rcdm_allgather")

    def close(self):
        """Destroy the communicator (collective: every rank of it should close).  Call it explicitly, while the peers
        are alive and after every graph that captured a collective on it is gone."""
        if self.comm:
            load().rcdm_comm_destroy(self.comm)
            self.comm = C.c_void_p(0)

    def __del__(self):
        # never at interpreter teardown: ncclCommDestroy can block on a peer that has already exited
        try:
            if _lib is not None and not sys.is_finalizing():
                self.close()
        except Exception:
            pass


class Event:
    def __init__(self):
        self.ev = C.c_void_p(0)
        _check(load().rcdm_event_create(C.byref(self.ev)), "rcdm_event_create")

    def record(self, stream=None):
        _check(load().rcdm_event_record(self.ev, stream_ptr() if stream is None else stream), "rcdm_event_record")

    def elapsed_ms(self, stop):
        ms = C.c_float(0)
        _check(load().rcdm_event_elapsed_ms(self.ev, stop.ev, C.byref(ms)), "rcdm_event_elapsed_ms")
        return ms.value

    def __del__(self):
        try:
            if self.ev and _lib is not None:
                _lib.rcdm_event_destroy(self.ev)
        except Exception:
            pass

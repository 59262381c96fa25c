"""The C ABI of libstego_corr.so as ctypes declares it: what include/*.h says, and nothing that calls.

Per unit (one header each): the descriptor structures, the error codes, limits and kinds, and in SIGNATURES the return and argument
types of every export.  stego_amd.capi re-exports all of it and holds the calls.  tests/test_abi_table_host.py compares every line
here with the headers: signatures type by type, structure layouts through the host C compiler, constants by value.
"""
import ctypes
from ctypes import POINTER, Structure, c_float, c_int32, c_int64, c_size_t, c_void_p

ABI_VERSION = 7
FLAG_SHARED_DEVICE = 1          # StegoCorrDesc.flags
PREC_F32 = 0
PREC_F16X3 = 1
PREC_BF16X3 = PREC_F16X3        # old name of the split mode (it used bf16 halves until round 1, third design)


class StegoMap(Structure):
    _fields_ = [("data", c_void_p), ("stride_n", c_int64), ("stride_c", c_int64),
                ("stride_h", c_int64), ("stride_w", c_int64)]


class StegoCorrDesc(Structure):
    _fields_ = [("B", c_int32), ("C", c_int32), ("K", c_int32), ("H", c_int32), ("W", c_int32),
                ("S", c_int32), ("n_neg", c_int32), ("pointwise", c_int32), ("zero_clamp", c_int32),
                ("stabalize", c_int32), ("pos_intra_shift", c_float), ("pos_inter_shift", c_float),
                ("neg_inter_shift", c_float), ("precision", c_int32), ("flags", c_int32)]


class StegoVitDesc(Structure):
    """include/stego_vit.h"""
    _fields_ = [(n, c_int32) for n in ("B", "H", "W", "patch", "D", "depth", "heads", "hidden", "precision")]


VIT_F16, VIT_F16X3 = 0, 1


class StegoHeadDesc(Structure):
    """include/stego_head.h"""
    _fields_ = [("B", c_int32), ("HW", c_int32), ("C", c_int32), ("K", c_int32), ("nonlinear", c_int32),
                ("tok_stride", c_int64), ("img_stride", c_int64), ("tokens_amax", c_void_p)]


class StegoCrfDesc(Structure):
    """include/stego_crf.h"""
    _fields_ = [("B", c_int32), ("C", c_int32), ("H", c_int32), ("W", c_int32), ("n_iter", c_int32), ("pos_w", c_float),
                ("pos_xy_std", c_float), ("bi_w", c_float), ("bi_xy_std", c_float), ("bi_rgb_std", c_float)]


CRF_ERR_LIMITS, CRF_ERR_RANGE = 20, 21


class StegoDataItem(Structure):
    """include/stego_data.h: one stored crop of the device image store"""
    _fields_ = [("img_offset", c_int64), ("label_offset", c_int64)] + \
        [(n, c_int32) for n in ("h", "w", "nh", "nw", "row_map", "col_map", "center_top", "center_left")]


class StegoDataDesc(Structure):
    """include/stego_data.h"""
    _fields_ = [("N", c_int32), ("R", c_int32), ("n_items", c_int64), ("img_arena_bytes", c_int64), ("label_arena_bytes", c_int64),
                ("map_pool_len", c_int64)]


DATA_ERR_RES, DATA_ERR_COUNT, DATA_ERR_ITEM, DATA_ERR_RANGE, DATA_ERR_ORIGIN = 30, 31, 32, 33, 34
DATA_MAX_RES, DATA_MAX_N = 2048, 65535


class StegoProbeDesc(Structure):
    """include/stego_probe.h"""
    _fields_ = [(n, c_int32) for n in ("B", "K", "h", "w", "H", "W", "n_lin", "n_clu", "lin_kind", "clu_kind")] + [("alpha", c_float)]


PROBE_ERR_DIM, PROBE_ERR_SIZE, PROBE_ERR_OUTPUT = 40, 41, 42
PROBE_SKIP, PROBE_LOG_PROBS, PROBE_PROBS, PROBE_ARGMAX = 0, 1, 2, 3
PROBE_KINDS = {None: PROBE_SKIP, "log_probs": PROBE_LOG_PROBS, "probs": PROBE_PROBS, "argmax": PROBE_ARGMAX}
PROBE_MAX_K, PROBE_MAX_N, PROBE_MAX_OUT = 128, 64, 2048


class StegoWindowLayout(Structure):
    """include/stego_stitch.h"""
    _fields_ = [(n, c_int32) for n in ("H", "W", "win", "stride")]


class StegoStitchDesc(Structure):
    """include/stego_stitch.h"""
    _fields_ = [("layout", StegoWindowLayout)] + \
        [(n, c_int32) for n in ("T", "K", "hc", "wc", "n_lin", "n_clu", "lin_kind", "clu_kind")] + [("alpha", c_float)]


STITCH_ERR_DIM, STITCH_ERR_SIZE, STITCH_ERR_LAYOUT, STITCH_ERR_WINDOWS, STITCH_ERR_OUTPUT, STITCH_ERR_RANGE = 120, 121, 122, 123, 124, 125
STITCH_MAX_SIDE = 32768


class StegoProbeConfusionDesc(Structure):
    """include/stego_confusion.h"""
    _fields_ = [(n, c_int32) for n in ("B", "K", "h", "w", "H", "W", "n_lin", "n_clu", "lin_on", "clu_on")] + \
        [("alpha", c_float), ("n_classes", c_int32)]


class StegoConfusionDesc(Structure):
    """include/stego_confusion.h"""
    _fields_ = [(n, c_int32) for n in ("B", "n", "H", "W", "n_classes", "pred_kind")]


CONF_ERR_DIM, CONF_ERR_SIZE, CONF_ERR_PROBES, CONF_ERR_KIND = 100, 101, 102, 103
CONF_LABELS, CONF_SCORES = 0, 1
CONF_KINDS = {"labels": CONF_LABELS, "scores": CONF_SCORES}
CONF_MAX_N, CONF_MAX_PIXELS = 64, 1 << 40


class StegoPrDesc(Structure):
    """include/stego_pr.h"""
    _fields_ = [(n, c_int32) for n in ("B", "C", "h", "w", "HL", "WL", "N1", "N2", "n_bins", "n_classes", "flags")]


PR_ERR_DIM, PR_ERR_POINTS, PR_ERR_BINS, PR_ERR_CLASSES, PR_ERR_SIZE, PR_ERR_FLAGS = 50, 51, 52, 53, 54, 55
PR_RAW, PR_SKIP_UNLABELED = 1, 2
PR_MAX_C, PR_MAX_POINTS, PR_MIN_BINS, PR_MAX_BINS, PR_MAX_CLASSES, PR_MAX_SIDE = 768, 4096, 64, 8192, 255, 16384


class StegoProbeTrainDesc(Structure):
    """include/stego_probe_train.h"""
    _fields_ = [(n, c_int32) for n in ("B", "K", "h", "w", "H", "W", "n_lin", "n_clu")]


PTRAIN_ERR_DIM, PTRAIN_ERR_SIZE, PTRAIN_ERR_PROBES = 60, 61, 62
PTRAIN_MAX_K, PTRAIN_MAX_N, PTRAIN_MAX_OUT, PTRAIN_MAX_CODE = 128, 64, 2048, 65535


class StegoHeatDesc(Structure):
    """include/stego_heat.h"""
    _fields_ = [(n, c_int32) for n in ("B", "C", "hs", "ws", "h", "w", "N", "H", "W", "flags")]


HEAT_ERR_DIM, HEAT_ERR_POINTS, HEAT_ERR_SIZE, HEAT_ERR_OUTPUT, HEAT_ERR_FLAGS = 70, 71, 72, 73, 74
HEAT_NO_CENTER, HEAT_NO_CLAMP = 1, 2
HEAT_MAX_C, HEAT_MAX_POINTS, HEAT_MAX_SIDE, HEAT_MAX_CELLS, HEAT_MAX_OUT = 768, 4096, 16384, 16384, 2048


class StegoCrfLossDesc(Structure):
    """include/stego_crf_loss.h"""
    _fields_ = [(n, c_int32) for n in ("B", "K", "G", "h", "w", "hg", "wg", "H", "W", "N")] + \
               [(n, c_float) for n in ("alpha", "beta", "gamma", "w1", "w2", "shift")] + [("flags", c_int32)]


CRFLOSS_ERR_DIM, CRFLOSS_ERR_POINTS, CRFLOSS_ERR_SIZE, CRFLOSS_ERR_PARAM, CRFLOSS_ERR_FLAGS = 80, 81, 82, 83, 84
CRFLOSS_NORMALIZE = 1
CRFLOSS_MAX_K, CRFLOSS_MAX_G, CRFLOSS_MAX_POINTS, CRFLOSS_MAX_SIDE, CRFLOSS_LAUNCHES = 128, 8, 4096, 2048, 3


class StegoAugParams(Structure):
    """include/stego_aug.h: one image's draws (64 bytes)"""
    _fields_ = [(n, c_int32) for n in ("flip", "top", "left", "ch", "cw")] + [("order", c_int32 * 4), ("factor", c_float * 4),
                                                                              ("gray", c_int32), ("blur_sigma", c_float), ("reserved", c_int32)]


class StegoAugDesc(Structure):
    """include/stego_aug.h"""
    _fields_ = [(n, c_int32) for n in ("B", "H", "W", "R")]


class StegoAugAlignDesc(Structure):
    """include/stego_aug.h"""
    _fields_ = [(n, c_int32) for n in ("B", "K", "h", "w", "S", "Rh", "Rw")]


AUG_ERR_SIZE, AUG_ERR_PARAM, AUGALIGN_ERR_DIM, AUGALIGN_ERR_SIZE = 90, 91, 92, 93
AUG_BRIGHTNESS, AUG_CONTRAST, AUG_SATURATION, AUG_HUE, AUG_NONE = 0, 1, 2, 3, 4
AUG_MAX_SIDE, AUG_MIN_RES, AUG_LAUNCHES, AUGALIGN_MAX_K, AUGALIGN_MAX_SIDE, AUGALIGN_LAUNCHES = 2048, 3, 2, 128, 256, 2


class StegoAdamSegment(Structure):
    """include/stego_optim.h: one record of the segment table (40 bytes)"""
    _fields_ = [("param", c_void_p), ("count", c_int64), ("grad_offset", c_int64), ("state_offset", c_int64), ("group", c_int32),
                ("reserved", c_int32)]


class StegoAdamGroup(Structure):
    """include/stego_optim.h"""
    _fields_ = [(n, ctypes.c_double) for n in ("lr", "beta1", "beta2", "eps")] + [("active", c_int32), ("reserved", c_int32)]


OPTIM_ERR_COUNT, OPTIM_ERR_SEGMENT, OPTIM_ERR_PARAM, OPTIM_ERR_FLAGS = 110, 111, 112, 113
ADAM_MAX_SEGMENTS, ADAM_MAX_GROUPS, ADAM_MAX_ELEMS, ADAM_CHUNK, ADAM_MAX_GRID = 256, 8, 1 << 31, 1024, 2048


class StegoAdamDesc(Structure):
    """include/stego_optim.h"""
    _fields_ = [(n, c_int32) for n in ("n_segments", "n_groups", "zero_grads", "reserved")] + \
        [("grad_elems", c_int64), ("state_elems", c_int64), ("groups", StegoAdamGroup * ADAM_MAX_GROUPS)]


class StegoStatsDesc(Structure):
    """include/stego_stats.h"""
    _fields_ = [("n_tensors", c_int32), ("n_scalars", c_int32), ("with_hist", c_int32), ("ring_slots", c_int32), ("counts", c_int64 * 4)]


STATS_PLAN_FIELDS = ("grid", "chunk", "record_bytes", "off_step", "off_with_hist", "off_n_tensors", "off_tensors", "tensor_stride",
                     "t_n_finite", "t_n_nan", "t_n_out", "t_sum", "t_sum_sq", "t_min", "t_max", "off_scalars", "off_hist", "hist_stride",
                     "ring_bytes", "state_bytes", "workspace_bytes")


class StegoStatsPlan(Structure):
    """include/stego_stats.h: the launch and the record layout (byte offsets)"""
    _fields_ = [(name, c_int64) for name in STATS_PLAN_FIELDS]


STATS_ERR_COUNT, STATS_ERR_RING, STATS_ERR_FLAGS = 160, 161, 162
STATS_MAX_TENSORS, STATS_MAX_SCALARS, STATS_MAX_ELEMS, STATS_MAX_SLOTS, STATS_BUCKETS, STATS_LIMITS = 4, 16, 1 << 31, 65536, 1548, 1549


class StegoSalienceDesc(Structure):
    """include/stego_salience.h"""
    _fields_ = [(n, c_int32) for n in ("B", "H", "W", "S", "mask_dtype")]


SALIENCE_ERR_SIZE, SALIENCE_ERR_SAMPLES, SALIENCE_ERR_DTYPE = 130, 131, 132
SALIENCE_U8, SALIENCE_F32 = 0, 1
SALIENCE_MAX_PIXELS, SALIENCE_MAX_S, SALIENCE_MAX_B = 1 << 20, 16, 65535


class StegoRecDesc(Structure):
    """include/stego_rec.h"""
    _fields_ = [(n, c_int32) for n in ("B", "K", "C", "h", "w")]


REC_ERR_DIM, REC_ERR_SIZE = 140, 141
REC_MAX_K, REC_MAX_C, REC_MAX_B, REC_MAX_SIDE, REC_MAX_TOKENS = 128, 1024, 65535, 2048, 1 << 24
REC_TILE, REC_MAX_WORKGROUPS, REC_LAUNCHES = 32, 64, 2


class StegoRenderDesc(Structure):
    """include/stego_render.h"""
    _fields_ = [(n, c_int32) for n in ("B", "H", "W", "n_lut", "label_dtype", "flags")] + \
        [("alpha", c_float), ("mean", c_float * 3), ("std", c_float * 3), ("ignore_rgb", ctypes.c_uint8 * 4), ("edge_rgb", ctypes.c_uint8 * 4)] + \
        [(n, c_int64) for n in ("label_stride_n", "label_stride_h", "label_stride_w", "out_stride_n", "out_stride_h")]


RENDER_ERR_SIZE, RENDER_ERR_LUT, RENDER_ERR_DTYPE, RENDER_ERR_FLAGS, RENDER_ERR_PARAM, RENDER_ERR_SELECT = 150, 151, 152, 153, 154, 155
RENDER_IMAGE, RENDER_LABELS, RENDER_EDGES, RENDER_BLEND, RENDER_RESCALE = 1, 2, 4, 8, 16
RENDER_I64, RENDER_I32, RENDER_U8 = 0, 1, 2
RENDER_MAX_LUT, RENDER_MAX_B = 512, 65535


class StegoPcaDesc(Structure):
    """include/stego_pca.h"""
    _fields_ = [(n, c_int32) for n in ("B", "C", "h", "w", "H", "W", "group", "n_iter", "resize", "scale")] + \
        [(n, c_int64) for n in ("out_stride_n", "out_stride_h")]


PCA_ERR_DIM, PCA_ERR_SIZE, PCA_ERR_ITER, PCA_ERR_MODE = 170, 171, 172, 173
PCA_PER_IMAGE, PCA_JOINT = 0, 1
PCA_BILINEAR, PCA_NEAREST = 0, 1
PCA_UNIT, PCA_RANGE = 0, 1
PCA_RESIZES = {"bilinear": PCA_BILINEAR, "nearest": PCA_NEAREST}
PCA_SCALES = {"unit": PCA_UNIT, "range": PCA_RANGE}
PCA_MIN_C, PCA_MAX_C, PCA_MAX_B, PCA_MAX_SIDE, PCA_MAX_TOKENS, PCA_MIN_TOKENS = 3, 768, 65535, 4096, 1 << 28, 4
PCA_MAX_ITER, PCA_DEFAULT_ITER, PCA_FOLD = 256, 32, 1024


class StegoKmeansDesc(Structure):
    """include/stego_kmeans.h"""
    _fields_ = [(n, c_int32) for n in ("B", "K", "h", "w", "n")]


KMEANS_ERR_DIM, KMEANS_ERR_SIZE, KMEANS_ERR_DRAW = 180, 181, 182
KMEANS_MAX_K, KMEANS_MAX_N, KMEANS_MAX_B, KMEANS_MAX_TOKENS = 128, 64, 65535, (1 << 31) - 1
KMEANS_FOLD, KMEANS_TILE, KMEANS_MAX_WORKGROUPS = 1024, 128, 512


class StegoRegionsDesc(Structure):
    """include/stego_regions.h"""
    _fields_ = [(n, c_int32) for n in ("B", "H", "W", "connectivity", "label_dtype")]


REGIONS_ERR_SIZE, REGIONS_ERR_CONN, REGIONS_ERR_DTYPE, REGIONS_ERR_LABELS, REGIONS_ERR_RANGE = 190, 191, 192, 193, 194
REGIONS_I64, REGIONS_I32, REGIONS_U8 = 0, 1, 2
REGIONS_TILE, REGIONS_CHUNK, REGIONS_MAX_LABELS, REGIONS_LAUNCHES, REGIONS_MAX_B, REGIONS_MAX_PIXELS = 32, 2048, 256, 6, 65535, (1 << 31) - 1
REGIONS_COLS32 = ("area", "y0", "x0", "y1", "x1", "first")
REGIONS_COLS64 = ("label", "sum_y", "sum_x")


class StegoRegionPoolDesc(Structure):
    """include/stego_region_pool.h"""
    _fields_ = [(n, c_int32) for n in ("B", "C", "h", "w", "H", "W")] + [("rows", c_int64)]


REGION_POOL_ERR_SIZE, REGION_POOL_ERR_DIM, REGION_POOL_ERR_RANGE = 200, 201, 202
REGION_POOL_MAX_C, REGION_POOL_CB, REGION_POOL_PARTIALS, REGION_POOL_LAUNCHES = 2048, 128, 1024, 3

# name -> (restype, argtypes); every symbol the headers of include/ declare
_P = c_void_p
_H = POINTER(StegoHeadDesc)
_D = POINTER(StegoCorrDesc)
_M = POINTER(StegoMap)
_V = POINTER(StegoVitDesc)
SIGNATURES = {
    "stego_vit_param_count": (c_int32, [_V]),
    "stego_vit_weights_bytes": (c_size_t, [_V]),
    "stego_vit_workspace_bytes": (c_size_t, [_V]),
    "stego_vit_pack_weights": (c_int32, [_V, POINTER(ctypes.c_void_p), c_int32, _P, c_size_t, _P]),
    "stego_vit_forward": (c_int32, [_V, _P, _P, _P, _P, c_size_t, _P]),
    "stego_vit_forward_keys": (c_int32, [_V, _P, _P, _P, _P, c_size_t, _P]),
    "stego_vit_forward_attn": (c_int32, [_V, _P, _P, _P, _P, _P, c_size_t, _P]),
    "stego_attn_salience": (c_int32, [_P] + [c_int32] * 5 + [c_float, _P, _P, _P]),
    "stego_head_fwd_workspace_bytes": (c_size_t, [_H]),
    "stego_head_bwd_workspace_bytes": (c_size_t, [_H]),
    "stego_head_fwd": (c_int32, [_H] + [_P] * 10 + [_P] * 3 + [_P, c_size_t, _P]),
    "stego_head_bwd": (c_int32, [_H] + [_P] * 6 + [_P] * 6 + [_P, c_size_t, _P]),
    "stego_crf_workspace_bytes": (c_size_t, [POINTER(StegoCrfDesc)]),
    "stego_crf_run": (c_int32, [POINTER(StegoCrfDesc), _P, _P, _P, _P, c_size_t, _P]),
    "stego_crf_lattice_info": (c_int32, [POINTER(StegoCrfDesc), _P, c_size_t, c_int32, c_int32, POINTER(c_int32), _P, c_int32, _P]),
    "stego_data_check_items": (c_int32, [POINTER(StegoDataDesc), _P, POINTER(c_int64)]),
    "stego_data_prepare": (c_int32, [POINTER(StegoDataDesc)] + [_P] * 10 + [_P]),
    "stego_data_prepare_dir": (c_int32, [POINTER(StegoDataDesc)] + [_P] * 10 + [_P]),
    "stego_salience_coords": (c_int32, [POINTER(StegoSalienceDesc)] + [_P] * 8 + [_P]),
    "stego_probe_head": (c_int32, [POINTER(StegoProbeDesc), _M, _M] + [_P] * 5 + [_P]),
    "stego_probe_head_plan": (c_size_t, [POINTER(StegoProbeDesc), POINTER(c_int32), POINTER(c_int32)]),
    "stego_stitch_probe": (c_int32, [POINTER(StegoStitchDesc), _M, _M] + [_P] * 5 + [_P]),
    "stego_stitch_probe_plan": (c_size_t, [POINTER(StegoStitchDesc)] + [POINTER(c_int32)] * 4),
    "stego_window_gather": (c_int32, [POINTER(StegoWindowLayout), _M, c_int32, c_int32, _P, _P, _P]),
    "stego_image_range_workspace_bytes": (c_size_t, [POINTER(StegoRenderDesc)]),
    "stego_image_range": (c_int32, [POINTER(StegoRenderDesc), _M, _P, _P, c_size_t, _P]),
    "stego_render": (c_int32, [POINTER(StegoRenderDesc), _M, _P, _P, _P, _P, _P]),
    "stego_pca_workspace_bytes": (c_size_t, [POINTER(StegoPcaDesc)]),
    "stego_pca_fit": (c_int32, [POINTER(StegoPcaDesc), _M, _P, _P, _P, _P, _P, c_size_t, _P]),
    "stego_pca_scores": (c_int32, [POINTER(StegoPcaDesc), _M, _P, _P, _P, _P, _P, c_size_t, _P]),
    "stego_pca_paint": (c_int32, [POINTER(StegoPcaDesc), _P, _P, _P, _P]),
    "stego_kmeans_workspace_bytes": (c_size_t, [POINTER(StegoKmeansDesc)]),
    "stego_kmeans_plan": (c_size_t, [POINTER(StegoKmeansDesc), POINTER(c_int32)]),
    "stego_kmeans_step": (c_int32, [POINTER(StegoKmeansDesc), _M, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "stego_kmeans_seed": (c_int32, [POINTER(StegoKmeansDesc), _M, _P, _P, _P, _P, c_size_t, _P]),
    "stego_regions_workspace_bytes": (c_size_t, [POINTER(StegoRegionsDesc)]),
    "stego_regions_plan": (c_int32, [POINTER(StegoRegionsDesc), POINTER(c_int32), POINTER(c_size_t), POINTER(c_int64)]),
    "stego_regions_label": (c_int32, [POINTER(StegoRegionsDesc), _P, _P, _P, _P, _P, c_size_t, _P]),
    "stego_regions_table": (c_int32, [POINTER(StegoRegionsDesc), _P, _P, _P, c_int64, _P, _P, _P]),
    "stego_regions_votes": (c_int32, [POINTER(StegoRegionsDesc), _P, _P, _P, c_int64, _P, c_int64, c_int64, c_int32, _P, _P]),
    "stego_regions_relabel": (c_int32, [POINTER(StegoRegionsDesc), _P, _P, _P, _P, c_int64, _P, _P, c_int64, c_int64, c_int32, _P, _P, _P]),
    "stego_region_pool_workspace_bytes": (c_size_t, [POINTER(StegoRegionPoolDesc)]),
    "stego_region_pool_plan": (c_int32, [POINTER(StegoRegionPoolDesc), POINTER(c_int32), POINTER(c_int32), POINTER(c_size_t), POINTER(c_int64)]),
    "stego_region_pool": (c_int32, [POINTER(StegoRegionPoolDesc), _M, _P, _P, _P, c_int64, c_int64, c_int64, _P, _P, c_size_t, _P]),
    "stego_probe_confusion": (c_int32, [POINTER(StegoProbeConfusionDesc), _M, _M] + [_P] * 6 + [_P]),
    "stego_probe_confusion_plan": (c_size_t, [POINTER(StegoProbeConfusionDesc), POINTER(c_int32), POINTER(c_int32)]),
    "stego_confusion": (c_int32, [POINTER(StegoConfusionDesc), _P, _P, _P, _P]),
    "stego_adam_step": (c_int32, [POINTER(StegoAdamDesc), _P, _P, _P, _P, _P, _P, _P, _P]),
    "stego_adam_plan": (c_int32, [POINTER(StegoAdamDesc), _P, POINTER(c_int32), POINTER(c_int32), POINTER(c_int64)]),
    "stego_step_stats": (c_int32, [POINTER(StegoStatsDesc), _P, _P, _P, _P, _P, _P]),
    "stego_step_stats_plan": (c_int32, [POINTER(StegoStatsDesc), POINTER(StegoStatsPlan)]),
    "stego_step_stats_edges": (c_int32, [_P, _P]),
    "stego_pr_accumulate": (c_int32, [POINTER(StegoPrDesc), _M, _M] + [_P] * 6 + [_P]),
    "stego_pr_plan": (c_size_t, [POINTER(StegoPrDesc), POINTER(c_int32), POINTER(c_int32)]),
    "stego_probe_train_workspace_bytes": (c_size_t, [POINTER(StegoProbeTrainDesc)]),
    "stego_probe_train": (c_int32, [POINTER(StegoProbeTrainDesc), _M] + [_P] * 9 + [_P, c_size_t, _P]),
    "stego_probe_train_plan": (c_size_t, [POINTER(StegoProbeTrainDesc), POINTER(c_int32)]),
    "stego_heat_workspace_bytes": (c_size_t, [POINTER(StegoHeatDesc)]),
    "stego_heat_plan": (c_size_t, [POINTER(StegoHeatDesc), POINTER(c_int32), POINTER(c_int32), POINTER(c_size_t), POINTER(c_int32)]),
    "stego_corr_heatmaps": (c_int32, [POINTER(StegoHeatDesc), _M, _M] + [_P] * 5 + [_P, c_size_t, _P]),
    "stego_crf_loss_workspace_bytes": (c_size_t, [POINTER(StegoCrfLossDesc)]),
    "stego_crf_loss_plan": (c_int32, [POINTER(StegoCrfLossDesc), POINTER(c_size_t), POINTER(c_int64)]),
    "stego_crf_loss": (c_int32, [POINTER(StegoCrfLossDesc), _M, _M, _P, _P, _P, _M, _P, c_size_t, _P]),
    "stego_augment_check_params": (c_int32, [POINTER(StegoAugDesc), _P, POINTER(c_int64), POINTER(c_int32)]),
    "stego_augment_workspace_bytes": (c_size_t, [POINTER(StegoAugDesc)]),
    "stego_augment_plan": (c_int32, [POINTER(StegoAugDesc), POINTER(c_size_t), POINTER(c_int64)]),
    "stego_augment": (c_int32, [POINTER(StegoAugDesc), _M, _P, _P, _P, _P, _P, c_size_t, _P]),
    "stego_aug_align_workspace_bytes": (c_size_t, [POINTER(StegoAugAlignDesc)]),
    "stego_aug_align_plan": (c_int32, [POINTER(StegoAugAlignDesc), POINTER(c_size_t), POINTER(c_int64)]),
    "stego_aug_align": (c_int32, [POINTER(StegoAugAlignDesc), _M, _M, _P, _P, _M, _M, _P, c_size_t, _P]),
    "stego_rec_loss_workspace_bytes": (c_size_t, [POINTER(StegoRecDesc)]),
    "stego_rec_loss_plan": (c_int32, [POINTER(StegoRecDesc), POINTER(c_size_t), POINTER(c_int64)]),
    "stego_rec_loss": (c_int32, [POINTER(StegoRecDesc), _M, _M, _P, _P, _P, _M, _P, _P, _P, c_size_t, _P]),
    "stego_abi_version": (c_int32, []),
    "stego_debug_set": (c_int32, [c_int32, c_int32]),
    "stego_debug_occupy": (c_int32, [c_int32, c_int32, c_int32, _P]),
    "stego_error_string": (ctypes.c_char_p, [c_int32]),
    "stego_corr_workspace_bytes": (c_size_t, [_D]),
    "stego_corr_saved_ctx_bytes": (c_size_t, [_D]),
    "stego_corr_helper_workspace_bytes": (c_size_t, [_D]),
    "stego_corr_helper_saved_ctx_bytes": (c_size_t, [_D]),
    "stego_dense_corr_workspace_bytes": (c_size_t, [c_int32] * 6),
    "stego_dense_corr": (c_int32, [_M, _M] + [c_int32] * 7 + [_P, _P, c_size_t, _P]),
    "stego_dense_corr_kernel": (c_int32, [_M, _M] + [c_int32] * 6),
    "stego_sample": (c_int32, [_M, _P, c_int32, c_int32, c_int32, c_int32, _P, c_int32, c_int32, _P, _P]),
    "stego_sample_bwd": (c_int32, [_P, _M, _P, c_int32, c_int32, c_int32, c_int32, _P, c_int32, c_int32, _P]),
    "stego_sample_bwd_rows": (c_int32, [_P, _P, _P, _M, _P, c_int32, c_int32, c_int32, c_int32, _P, c_int32, c_int32, _P]),
    "stego_panel_image_bytes": (c_size_t, [c_int32, c_int32]),
    "stego_sample_panels": (c_int32, [_M, _P, c_int32, c_int32, c_int32, c_int32, _P, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P]),
    "stego_dense_corr_panels": (c_int32, [_P, _P, c_int32, _P, _P, c_int32, c_int32, c_int32, c_int32, _P, _P, _P]),
    "stego_rowsum": (c_int32, [_P, ctypes.c_int64, c_int32, _P, _P]),
    "stego_loss_pointwise_fwd": (c_int32, [_P] * 4 + [c_int32] * 3 + [POINTER(c_float), c_float, c_float, c_int32, _P, _P, _P]),
    "stego_loss_pointwise_bwd": (c_int32, [_P] * 4 + [c_int32] * 3 + [POINTER(c_float), c_float, c_float, c_int32, _P, _P, _P, _P, _P]),
    "stego_knn_workspace_bytes": (c_size_t, [ctypes.c_int64, c_int32, c_int32, ctypes.c_int64]),
    "stego_knn_topk": (c_int32, [_P, ctypes.c_int64, c_int32, ctypes.c_int64, c_int32, c_int32, ctypes.c_int64, ctypes.c_int64,
                                 _P, _P, _P, c_size_t, _P]),
    "stego_corr_fwd": (c_int32, [_D] + [_M] * 4 + [_P] * 3 + [_P] * 8 + [_P, c_size_t, _P]),
    "stego_corr_fwd_prepared": (c_int32, [_D] + [_M] * 4 + [_P] * 3 + [_P] * 8 + [_P, c_size_t, _P]),
    "stego_corr_workspace_prepare": (c_int32, [_D, _P, c_size_t, _P]),
    "stego_corr_workspace_prepare_now": (c_int32, [_D, _P, c_size_t]),
    "stego_corr_fwd_launches": (c_int32, [_D] + [_M] * 4),
    "stego_corr_event_counters": (c_void_p, [_D, _P, c_size_t]),
    "stego_ref_draws": (c_int32, [ctypes.c_uint64, ctypes.c_uint64, c_int32, c_int64, c_int32, c_int32, _P, _P, _P, _P]),
    "stego_ref_draws_advance": (ctypes.c_uint64, [c_int64, c_int32, c_int32, c_int32]),
    "stego_tokens_from_cache": (c_int32, [_P, _P, c_int32, c_int32, c_int32, c_int32, _P, _P, _P]),
    "stego_ref_dropout_masks": (c_int32, [ctypes.c_uint64, ctypes.c_uint64, _P, _P, c_int32, c_int32, c_int64, c_float, _P, _P]),
    "stego_ref_dropout_masks_advance": (ctypes.c_uint64, [c_int64, c_int32, c_int32]),
    "stego_ref_draws_indirect": (c_int32, [_P, _P, ctypes.c_uint64, c_int32, c_int64, c_int32, c_int32, _P, _P, _P, _P]),
    "stego_fast_draws": (c_int32, [_P, ctypes.c_int64, c_int32, c_int32, _P, _P, _P, _P]),
    "stego_finish_draws": (c_int32, [_P, _P, ctypes.c_int64, POINTER(ctypes.c_void_p), c_int32, c_int32, _P, _P, _P, _P]),
    "stego_corr_fwd_profile": (c_int32, [_D] + [_M] * 4 + [_P] * 3 + [_P] * 8 + [_P, c_size_t, _P]
                               + [c_int32, POINTER(c_float)]),
    "stego_corr_bwd_workspace_bytes": (c_size_t, [_D]),
    "stego_corr_helper_bwd_workspace_bytes": (c_size_t, [_D]),
    "stego_corr_bwd": (c_int32, [_D] + [_P] + [_P] * 3 + [_P] * 3 + [_P, _P, _P, c_int32] + [_P] * 3
                       + [_P, _P] + [_P, c_size_t, _P]),
    "stego_corr_helper_fwd": (c_int32, [_D] + [_M] * 4 + [_P] * 5 + [_P, c_size_t, _P]),
    "stego_corr_helper_bwd": (c_int32, [_D] + [_P] * 6 + [_P, _P] + [_P, c_size_t, _P]),
}

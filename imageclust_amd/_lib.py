"""ctypes binding of libimageclust_hip.so (the C-ABI declared in include/imageclust.h).

This module is plumbing only: it loads the in-tree shared object built by `__graft_entry__.build()` (or
`make -C imageclust_amd/csrc`) and fails loudly when it is missing -- there is no CPU or PyTorch fallback.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("ICL_SO_PATH") or os.path.join(_HERE, "libimageclust_hip.so")  # (ICL_SO_PATH: scratch A/B builds of the same library)

ICL_OK = 0
ICL_ERR_ARG, ICL_ERR_CONSTRAINT, ICL_ERR_HIP, ICL_ERR_NOMODEL, ICL_ERR_IO, ICL_ERR_UNSUPPORTED, ICL_ERR_OVERSIZE, ICL_ERR_NOMEM = range(1, 9)
HEAD_POOLED, HEAD_DENSE0 = 2048, 1000
PREC_FP32, PREC_BF16, PREC_BF16X3 = 0, 1, 2  # PREC_BF16X3: split bf16 (hi + lo pairs, three bf16 MFMAs per product), within the fp32 parity bound
UPDATE_EXACT, UPDATE_LW = 0, 1
SYNTH_NOISE, SYNTH_STRUCTURED = 0, 1
TILES_AUTO, TILES_LOCAL, TILES_DISTRIBUTED = 0, 1, 2
MERGE_GPU0, MERGE_SHARDED = 0, 1
CONV_P8_OFF, CONV_P8_AUTO, CONV_P8_ALL = 0, 1, 2
CONV_SPLIT = 16
ROWS_SINGLE, ROWS_EXACT_BATCH, ROWS_LW_BOUND, ROWS_LW_FAST, ROWS_SINGLE_APART = 0, 1, 2, 3, 4
FILE_FAIL_NEXT_LEADER = 0x100
MANY_MID_AUTO, MANY_MID_OFF, MANY_MID_ON = 0, 1, 2  # icl_set_many_options: the mid-size route (257 to 2048 rows) of icl_cluster_many
PNG_HOST, PNG_GPU = 0, 1  # icl_set_png_options: where a qualifying PNG of a batched file call is inflated and unfiltered
ENTROPY_HOST, ENTROPY_GPU = 0, 1  # icl_set_ingest_options: where the Huffman decoder of a qualifying baseline JPEG runs
K_CONV, K_DIST_EXACT, K_DIST_MFMA, K_ROWMIN, K_UPDATE, K_EMBED_OTHER, K_CONV64 = range(7)
K_NAMES = ["conv_igemm_kernel<*,128>", "ward_dist_exact_kernel", "dist_mfma_kernel", "row_argmin_*_kernel",
           "ward_update_exact_kernel", "embed_other", "conv_igemm_kernel<*,64>"]
IMG_BYTES = 224 * 224 * 3
MAX_IMAGE_SIZE, MAX_IMAGE_DIM = 5 * 1024 * 1024, 2048  # rekognition.go: MaxImageSize, and the box resizeImageIfNeeded resizes into

# every symbol include/imageclust.h declares: (name, restype, argtypes)
_vp, _i64, _i32, _int = C.c_void_p, C.c_int64, C.c_int32, C.c_int
_pi64, _pi32 = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
_pd = C.POINTER(C.c_double)
_ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # a host array's address; None (NULL) for no array or an empty one
_as_vp = lambda p: p if isinstance(p, _vp) or p is None else _vp(p)  # a device address as the argument type of a *_dev entry point
SYMBOLS = [
    ("icl_create", _int, [_int, C.POINTER(_vp)]),
    ("icl_destroy", None, [_vp]),
    ("icl_last_error", C.c_char_p, [_vp]),
    ("icl_stream", _vp, [_vp]),
    ("icl_sync", _int, [_vp]),
    ("icl_device_info", _int, [_vp, C.c_char_p, _int, C.POINTER(_int), _pi64]),
    ("icl_dev_malloc", _int, [_vp, _i64, C.POINTER(_vp)]),
    ("icl_dev_free", _int, [_vp, _vp]),
    ("icl_memcpy_h2d", _int, [_vp, _vp, _vp, _i64]),
    ("icl_memcpy_d2h", _int, [_vp, _vp, _vp, _i64]),
    ("icl_model_load_onnx", _int, [_vp, C.c_char_p]),
    ("icl_onnx_to_blob_file", _int, [C.c_char_p, _vp, _i64, _pi64]),
    ("icl_model_load_blob", _int, [_vp, _vp, _i64]),
    ("icl_model_load_synthetic", _int, [_vp, C.c_uint64]),
    ("icl_synthetic_blob_bytes", _i64, []),
    ("icl_synthetic_blob", _int, [C.c_uint64, _vp, _i64]),
    ("icl_embed_u8", _int, [_vp, _vp, _i64, _int, _int, _vp]),
    ("icl_embed_u8_dev", _int, [_vp, _vp, _i64, _int, _int, _vp]),
    ("icl_embed_file", _int, [_vp, C.c_char_p, _int, _vp]),
    ("icl_set_file_options", _int, [_vp, _int, _int, _int]),
    ("icl_file_batch_stats", _int, [_vp, _pi64, _pi64]),
    ("icl_preprocess_u8", _int, [_vp, _vp]),
    ("icl_preprocess_file", _int, [C.c_char_p, _vp]),
    ("icl_resize_u8", _int, [_vp, _i32, _i32, _vp, _i32, _i32]),
    ("icl_decode_image_file", _int, [C.c_char_p, _vp, _i64, _pi32, _pi32]),
    ("icl_load_image_224", _int, [C.c_char_p, _vp]),
    ("icl_load_images_224_dev", _int, [_vp, _vp, _i64, _i32, _vp, _vp]),
    ("icl_embed_files", _int, [_vp, _vp, _i64, _int, _int, _i32, _vp, _vp]),
    ("icl_embed_files_dev", _int, [_vp, _vp, _i64, _int, _int, _i32, _vp, _vp]),
    ("icl_last_ingest_stats", _int, [_vp, _pi64, _pi64, _pi64, _pd]),
    ("icl_set_ingest_options", _int, [_vp, _int]),
    ("icl_last_entropy_stats", _int, [_vp, _pi64, _pi64, _pi64, _pi64]),
    ("icl_jpeg_coefs_files", _int, [_vp, _vp, _i64, _int, _vp, _i64, _vp, _vp]),
    ("icl_jpeg_coefs_file_host", _int, [C.c_char_p, _int, _vp, _i64, _pi64, _vp]),
    ("icl_set_png_options", _int, [_vp, _int]),
    ("icl_last_png_stats", _int, [_vp, _pi64, _pi64, _pi64, _pi64]),
    ("icl_png_raw_files", _int, [_vp, _vp, _i64, _int, _vp, _i64, _vp, _vp]),
    ("icl_png_raw_file_host", _int, [C.c_char_p, _int, _vp, _i64, _pi64, _vp]),
    ("icl_png_raw_mem_host", _int, [_vp, _i64, _int, _vp, _i64, _pi64, _vp]),
    ("icl_decode_image_mem", _int, [_vp, _i64, _vp, _i64, _pi32, _pi32]),
    ("icl_load_image_224_mem", _int, [_vp, _i64, _vp]),
    ("icl_preprocess_mem", _int, [_vp, _i64, _vp]),
    ("icl_embed_image_mem", _int, [_vp, _vp, _i64, _int, _vp]),
    ("icl_load_images_224_mem_dev", _int, [_vp, _vp, _vp, _i64, _i32, _vp, _vp]),
    ("icl_embed_images_mem", _int, [_vp, _vp, _vp, _i64, _int, _int, _i32, _vp, _vp]),
    ("icl_embed_images_mem_dev", _int, [_vp, _vp, _vp, _i64, _int, _int, _i32, _vp, _vp]),
    ("icl_cluster_requests_mem", _int, [_vp, _i32] + [_vp] * 8 + [_int, _int, _i32] + [_vp] * 8),
    ("icl_jpeg_coefs_mem", _int, [_vp, _vp, _vp, _i64, _int, _vp, _i64, _vp, _vp]),
    ("icl_jpeg_encode_bound", _i64, [_i32, _i32]),
    ("icl_jpeg_encode_rgb", _int, [_vp, _i32, _i32, _i32, _vp, _i64, _pi64]),
    ("icl_jpeg_encode_rgb_dev", _int, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _i64, _vp]),
    ("icl_downsize_image_file", _int, [C.c_char_p, _i64, _i32, _vp, _i64, _pi64, _vp]),
    ("icl_downsize_image_mem", _int, [_vp, _i64, _i64, _i32, _vp, _i64, _pi64, _vp]),
    ("icl_downsize_images", _int, [_vp, _vp, _i64, _i64, _i32, _i32, _vp, _i64, _vp, _vp]),
    ("icl_downsize_images_mem", _int, [_vp, _vp, _vp, _i64, _i64, _i32, _i32, _vp, _i64, _vp, _vp]),
    ("icl_last_downsize_stats", _int, [_vp, _pi64, _pi64, _pi64, _pi64, _pi64, _pi64, _vp]),
    ("icl_set_batch", _int, [_vp, _int]),
    ("icl_set_conv_options", _int, [_vp, _int]),
    ("icl_conv_stats", _int, [_vp, _vp, _vp]),
    ("icl_set_forward_prune", _int, [_vp, _int]),
    ("icl_forward_prune_stats", _int, [_vp, _vp]),
    ("icl_set_forward_prune_fused", _int, [_vp, _int]),
    ("icl_forward_prune_fused_stats", _int, [_vp, _vp]),
    ("icl_set_stem_max_blocks", _int, [_vp, _int]),
    ("icl_bottleneck56_sub", _int, [_vp, _vp, _int, _int, _int] + [_vp] * 9 + [_int, _int, _vp]),
    ("icl_conv1x1_mapped", _int, [_vp, _vp, _int, _int, _int, _int, _vp, _int, _vp, _vp, _vp, _int, _vp]),
    ("icl_conv_split_launches", _int, [_vp, _vp]),
    ("icl_conv2d_fused", _int, [_vp, _int, _vp, _int, _int, _int, _vp, _int, _int, _int, _int, _vp, _vp, _vp, _int, _vp]),
    ("icl_conv2d_dual", _int, [_vp, _int, _vp, _int, _int, _int, _vp, _vp, _int, _int, _vp, _int, _int, _vp, _vp, _int, _vp]),
    ("icl_embed_taps", _int, [_vp, _int, _vp, _int, _int, _vp]),
    ("icl_stem_pool", _int, [_vp, _int, _vp, _int, _vp]),
    ("icl_bottleneck56", _int, [_vp, _vp, _int, _int, _int, _int] + [_vp] * 13),
    ("icl_calc_optimal_clusters", _int, [_i64, _i64, _i64, _pi64]),
    ("icl_ward_distance_matrix", _int, [_vp, _vp, _vp, _i64, _i32, _vp, _i64]),
    ("icl_ward_distance_matrix_dev", _int, [_vp, _vp, _vp, _i64, _i32, _vp, _i64]),
    ("icl_merge_centroid", _int, [_vp, _vp, _i64, _vp, _i64, _i32, _vp]),
    ("icl_update_distance_matrix", _int, [_vp, _vp, _i64, _i64, _vp, _vp, _i32, _i64, _i64, _vp, _i64]),
    ("icl_find_closest", _int, [_vp, _vp, _i64, _i64, _pi64, _pi64]),
    ("icl_find_closest_dev", _int, [_vp, _vp, _i64, _i64, _pi64, _pi64]),
    ("icl_group_create", _int, [_pi32, _i32, C.POINTER(_vp)]),
    ("icl_group_destroy", None, [_vp]),
    ("icl_group_size", _i32, [_vp]),
    ("icl_group_ctx", _vp, [_vp, _i32]),
    ("icl_group_last_error", C.c_char_p, [_vp]),
    ("icl_group_load_onnx", _int, [_vp, C.c_char_p]),
    ("icl_group_load_blob", _int, [_vp, _vp, _i64]),
    ("icl_group_load_synthetic", _int, [_vp, C.c_uint64]),
    ("icl_group_embed_u8", _int, [_vp, _vp, _i64, _int, _int, _vp]),
    ("icl_group_cluster", _int, [_vp, _vp, _i64, _i32, _i32, _i32, _int, _vp, _vp, _pi32]),
    ("icl_set_ward_options", _int, [_vp, _int]),
    ("icl_embed_cluster_dev", _int, [_vp, _vp, _i64, _int, _i32, _i32, _int, _int, _vp, _vp, _vp, _pi32]),
    ("icl_group_embed_cluster", _int, [_vp, _vp, _i64, _int, _i32, _i32, _int, _vp, _vp, _vp, _pi32]),
    ("icl_ward_rows_partition", _int, [_i64, _i32, _i32, _pi64, _pi64]),
    ("icl_ward_span", _int, [_i64, _i64, _pi64, _pi64]),
    ("icl_ward_distance_rows_dev", _int, [_vp, _vp, _i64, _i32, _i64, _i64, _vp]),
    ("icl_ward_rows_hold_bounds", _int, [_vp, _i64, _int]),
    ("icl_ward_prepare", _int, [_vp, _i64, _i32]),
    ("icl_ward_unpack_spans_dev", _int, [_vp, _i32, _pi64, _pi64, C.POINTER(_vp)]),
    ("icl_group_set_options", _int, [_vp, _int, _int]),
    ("icl_cluster_prefilled_dev", _int, [_vp, _vp, _i64, _i32, _i32, _i32, _int, _i64, _i64, _vp, _vp, _pi32]),
    ("icl_cluster", _int, [_vp, _vp, _i64, _i32, _i32, _i32, _int, _vp, _vp, _pi32]),
    ("icl_cluster_dev", _int, [_vp, _vp, _i64, _i32, _i32, _i32, _int, _vp, _vp, _pi32]),
    ("icl_cluster_many", _int, [_vp, _i32, _vp, _i64] + [_vp] * 11),
    ("icl_cluster_many_dev", _int, [_vp, _i32, _vp, _i64] + [_vp] * 11),
    ("icl_cluster_many_seeded", _int, [_vp, _i32, _vp, _i64] + [_vp] * 14),
    ("icl_cluster_many_seeded_dev", _int, [_vp, _i32, _vp, _i64] + [_vp] * 14),
    ("icl_cluster_many_apart", _int, [_vp, _i32, _vp, _i64] + [_vp] * 17),
    ("icl_cluster_many_apart_dev", _int, [_vp, _i32, _vp, _i64] + [_vp] * 17),
    ("icl_cluster_seeded", _int, [_vp, _vp, _i64, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _pi32, _vp]),
    ("icl_cluster_seeded_dev", _int, [_vp, _vp, _i64, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _pi32, _vp]),
    ("icl_cluster_seeded_fast", _int, [_vp, _vp, _i64, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _pi32, _vp]),
    ("icl_cluster_seeded_fast_dev", _int, [_vp, _vp, _i64, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _pi32, _vp]),
    ("icl_cluster_apart", _int, [_vp, _vp, _i64, _i32, _vp, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _vp, _pi32, _vp]),
    ("icl_cluster_apart_dev", _int, [_vp, _vp, _i64, _i32, _vp, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _vp, _pi32, _vp]),
    ("icl_seeded_assign_ids", _int, [_i32, _vp, _i32, _vp, _i32, _vp, _vp, _pi32]),
    ("icl_nearest", _int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp]),
    ("icl_nearest_dev", _int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp]),
    ("icl_nearest_from_matrix", _int, [_vp, _i64, _i64, _i64, _vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    ("icl_set_nearest_options", _int, [_vp, _i32]),
    ("icl_last_nearest_stats", _int, [_vp, _pi64]),
    ("icl_cluster_fit", _int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _i32] + [_vp] * 6),
    ("icl_cluster_fit_dev", _int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _i32] + [_vp] * 6),
    ("icl_cluster_fit_from_matrix", _int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _i32, _i32] + [_vp] * 6),
    ("icl_last_fit_stats", _int, [_vp, _pi64]),
    ("icl_ward_values_at", _int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _i32, _vp, _vp, _i64, _vp]),
    ("icl_ward_values_at_dev", _int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _i32, _vp, _vp, _i64, _vp]),
    ("icl_fold_centroids", _int, [_vp, _vp, _vp, _i64, _i32, _vp, _vp, _i64, _vp, _vp]),
    ("icl_fold_centroids_dev", _int, [_vp, _vp, _vp, _i64, _i32, _vp, _vp, _i64, _vp, _vp]),
    ("icl_last_fold_stats", _int, [_vp, _pi64]),
    ("icl_pairs_within", _int, [_vp, _vp, _vp, _i64, _i32, C.c_float, _vp, _vp, _vp, _i64, _pi64]),
    ("icl_pairs_within_dev", _int, [_vp, _vp, _vp, _i64, _i32, C.c_float, _vp, _vp, _vp, _i64, _pi64]),
    ("icl_pairs_within_from_matrix", _int, [_vp, _i64, _i64, C.c_float, _vp, _vp, _vp, _i64, _pi64]),
    ("icl_pair_groups", _int, [_i64, _vp, _vp, _vp, _pi64]),
    ("icl_last_pairs_stats", _int, [_vp, _pi64]),
    ("icl_pairs_between", _int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _i32, C.c_float, _vp, _vp, _vp, _vp, _i64, _pi64]),
    ("icl_pairs_between_dev", _int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _i32, C.c_float, _vp, _vp, _vp, _vp, _i64, _pi64]),
    ("icl_pairs_between_from_matrix", _int, [_vp, _i64, _i64, _i64, C.c_float, _vp, _vp, _vp, _vp, _i64, _pi64]),
    ("icl_last_pairs_between_stats", _int, [_vp, _pi64]),
    ("icl_set_many_options", _int, [_vp, _int]),
    ("icl_last_many_stats", _int, [_vp, _pi64, _pi64, _pi64, _pi64]),
    ("icl_requests_layout", _int, [_i32, _vp, _vp, _int, _vp, _vp, _pi64]),
    ("icl_cluster_requests", _int, [_vp, _i32] + [_vp] * 7 + [_int, _int, _i32] + [_vp] * 8),
    ("icl_last_requests_ms", _int, [_vp, _pd, _pd, _pd]),
    ("icl_last_merges", _i64, [_vp, _vp, _i64]),
    ("icl_last_merge_values", _i64, [_vp, _vp, _i64]),
    ("icl_distance_mfma_dev", _int, [_vp, _vp, _i64, _i32, _vp, _i64]),
    ("icl_distance_mfma_seeded_dev", _int, [_vp, _vp, _i64, _i32, _vp, _vp, _i64]),
    ("icl_synth_images", _int, [C.c_uint64, _i64, _i64, _int, _vp]),
    ("icl_synth_images_dev", _int, [_vp, C.c_uint64, _i64, _i64, _int, _vp]),
    ("icl_prof_enable", _int, [_vp, _int]),
    ("icl_prof_reset", _int, [_vp]),
    ("icl_prof_query", _int, [_vp, _int, _pd, _pi64, _pd, _pd]),
    ("icl_last_stage_ms", _int, [_vp, _pd, _pd, _pd]),
    ("icl_last_ward_stats", _int, [_vp, _vp, _vp, _vp, _vp]),
    ("icl_last_ward_mode", _int, [_vp, _vp, _vp]),
    ("icl_last_ward_layout", _int, [_vp, _vp, _vp, _vp]),
    ("icl_distance_bounds_check_dev", _int, [_vp, _vp, C.c_int64, C.c_int32, _int, _vp, _vp, _vp, _vp, _vp]),
    ("icl_last_ward_bound_violations", _i64, [_vp]),
    ("icl_ward_dump_pairs_dev", _int, [_vp, _vp, C.c_int64, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("icl_version", C.c_char_p, []),
]

_lib = None


class ICLError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("icl error %d: %s" % (code, msg))
        self.code = code


def load():
    """Load the HIP engine.  Raises (never falls back) if the shared object is absent or lacks a symbol."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise ImportError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950); imageclust_amd has no CPU fallback" % SO_PATH)
    try:
        # Share ONE HIP runtime with PyTorch when both live in a process: torch bundles its own libamdhip64
        # (same soname), so import it first and let the dynamic loader reuse that copy.
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(SO_PATH)
    for name, res, args in SYMBOLS:
        fn = getattr(L, name)  # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(ctx_handle, rc):
    if rc != ICL_OK:
        msg = load().icl_last_error(ctx_handle)
        raise ICLError(rc, msg.decode() if msg else "")


def _many_outputs(pk, want_merges):
    """The output arrays of a many-call over pk's problems: cluster_id, rank, n_clusters, n_merges, status, merge log (or None), in
    _unpack_many's order.  The statuses stay -1 when the call fails before the problems run (with a code that is no problem's own)."""
    nprob, rows = len(pk["n"]), int(pk["img_off"][-1])
    cid = np.full(max(rows, 1), -1, np.int32)
    rank = np.full(max(rows, 1), -1, np.int32)
    nc, nm = np.zeros(max(nprob, 1), np.int32), np.zeros(max(nprob, 1), np.int32)
    st = np.full(max(nprob, 1), -1, np.int32)
    mg = np.zeros(max(2 * rows, 1), np.int32) if want_merges else None
    return cid, rank, nc, nm, st, mg


def _unpack_many(pk, cid, rank, nc, nm, st, mg):
    out = []
    for p in range(len(pk["n"])):
        a, b = int(pk["img_off"][p]), int(pk["img_off"][p + 1])
        r = (cid[a:b].copy(), rank[a:b].copy(), int(nc[p]), int(st[p]))
        if mg is not None:
            r += (mg[2 * a:2 * a + 2 * int(nm[p])].reshape(-1, 2).copy(),)
        out.append(r)
    return out


def pack_many(problems):
    """The arguments of icl_cluster_many for problems = [(E, min_size, max_size), ...]: one float32 buffer holding every problem's rows,
    each problem starting on a 16-byte boundary (the kernels' float4 loads then read its rows in place) -> dict(E, e_off, n, d, min_size,
    max_size, img_off); problem p's images are [img_off[p], img_off[p + 1]) of the outputs."""
    mats, off, pos = [], [], 0
    for E, _, _ in problems:
        E = np.asarray(E, np.float32)
        if E.ndim != 2:
            raise ValueError("each problem's E must be 2-D, got shape %s" % (E.shape,))
        off.append(pos)
        mats.append(E)
        pos += (E.size + 3) // 4 * 4
    if len(mats) == 1 and mats[0].size and mats[0].flags.c_contiguous:
        buf = mats[0].reshape(-1)  # one problem: its own rows, not a copy
    else:
        buf = np.zeros(max(pos, 1), np.float32)
        for E, o in zip(mats, off):
            buf[o:o + E.size] = E.ravel()
    n = np.array([E.shape[0] for E in mats], np.int32)
    return dict(E=buf, e_off=np.array(off, np.int64), n=n, d=np.array([E.shape[1] for E in mats], np.int32),
                min_size=np.array([int(p[1]) for p in problems], np.int32), max_size=np.array([int(p[2]) for p in problems], np.int32),
                img_off=np.concatenate([[0], np.cumsum(n, dtype=np.int64)]))


def _nearest_side(n, size, what):
    """A size array of icl_nearest as contiguous int32[n], or None."""
    if size is None:
        return None
    a = np.ascontiguousarray(np.asarray(size).reshape(-1), np.int32)
    if len(a) != n:
        raise ValueError("%d %s entries for %d rows" % (len(a), what, n))
    return a


def _nearest_exclude(nq, exclude):
    if exclude is None:
        return None
    a = np.ascontiguousarray(np.asarray(exclude).reshape(-1), np.int64)
    if len(a) != nq:
        raise ValueError("%d exclude entries for %d query rows" % (len(a), nq))
    return a


def nearest_from_matrix(D, k, q_size=None, e_size=None, max_size=0, exclude=None, n=None):
    """icl_nearest_from_matrix (host only, no GPU): the leave-out and order rules of Context.nearest applied to values the caller holds ->
    (idx int32[nq][k], val float32[nq][k]).  D is nq x ld float32; n (default ld) columns of each row are pairs.  Raises ICLError(ICL_ERR_ARG)."""
    D = np.asarray(D, np.float32)
    if D.ndim != 2:
        raise ValueError("D must be 2-D")
    if not D.flags.c_contiguous:
        D = np.ascontiguousarray(D)
    nq, ld = D.shape
    n = ld if n is None else int(n)
    qs, es, ex = _nearest_side(nq, q_size, "q_size"), _nearest_side(n, e_size, "e_size"), _nearest_exclude(nq, exclude)
    kk = max(int(k), 1)
    idx, val = np.empty((nq, kk), np.int32), np.empty((nq, kk), np.float32)
    rc = load().icl_nearest_from_matrix(_ptr(D), nq, n, ld, _ptr(qs), _ptr(es), int(k), int(max_size), _ptr(ex), idx.ctypes.data, val.ctypes.data)
    if rc != ICL_OK:
        raise ICLError(rc, "icl_nearest_from_matrix: bad argument")
    return idx, val


def _fold_lists(row_ptr, member):
    """row_ptr of icl_fold_centroids as contiguous int64[K + 1]; its last entry must be the length of member (the library cannot see that)."""
    rp = np.ascontiguousarray(np.asarray(row_ptr).reshape(-1), np.int64)
    if len(rp) < 1:
        raise ValueError("row_ptr must hold K + 1 entries")
    if int(rp[-1]) != np.asarray(member).size:
        raise ValueError("row_ptr ends at %d for %d members" % (int(rp[-1]), np.asarray(member).size))
    return rp


def groups_as_csr(groups):
    """Lists of row indices -> (row_ptr int64[K + 1], member int32[total]), the member-list form of Context.fold_centroids."""
    rp = np.zeros(len(groups) + 1, np.int64)
    np.cumsum(np.array([len(g) for g in groups], np.int64), out=rp[1:])
    return rp, np.array([i for g in groups for i in g], np.int64).astype(np.int32).reshape(-1)


def _fit_outputs(nq, K, k_alt):
    """The output arrays of the icl_cluster_fit family, in argument order: own, alt_idx, alt_val, listed, rep, worst."""
    kk = max(int(k_alt), 0)
    return (np.empty(nq, np.float32), np.empty((nq, kk), np.int32), np.empty((nq, kk), np.float32), np.empty(K, np.int32), np.empty(K, np.int32),
            np.empty(K, np.int32))


def _fit_result(out):
    return dict(zip(("own", "alt_idx", "alt_val", "listed", "rep", "worst"), out))


def cluster_fit_from_matrix(D, cluster_of, k_alt, q_size=None, c_size=None, max_size=0, K=None):
    """icl_cluster_fit_from_matrix (host only, no GPU): the rules of Context.cluster_fit applied to values the caller holds -> the same
    dict.  D is nq x ld float32; K (default ld) columns of each row are clusters.  Raises ICLError(ICL_ERR_ARG)."""
    D = np.asarray(D, np.float32)
    if D.ndim != 2:
        raise ValueError("D must be 2-D")
    if not D.flags.c_contiguous:
        D = np.ascontiguousarray(D)
    nq, ld = D.shape
    K = ld if K is None else int(K)
    qs, cs, cof = _nearest_side(nq, q_size, "q_size"), _nearest_side(K, c_size, "c_size"), _nearest_side(nq, cluster_of, "cluster_of")
    out = _fit_outputs(nq, max(K, 0), k_alt)
    rc = load().icl_cluster_fit_from_matrix(_ptr(D), nq, K, ld, _ptr(qs), _ptr(cof), _ptr(cs), int(k_alt), int(max_size), *[_ptr(a) for a in out])
    if rc != ICL_OK:
        raise ICLError(rc, "icl_cluster_fit_from_matrix: bad argument")
    return _fit_result(out)


def _pairs_two_calls(n, call, what, cap=None):
    """The size query and the call proper of the icl_pairs_within family -> (row_ptr int64[n + 1], col int32[total], val float32[total]).
    call(row_ptr_address, col_address, val_address, cap, total) -> code; total is a ctypes int64 to pass by reference.  With a cap hint the
    first call already carries buffers, and a second one follows only when they were too small; ICL_ERR_ARG with total left at -1 is
    a bad argument."""
    row_ptr = np.zeros(max(int(n), 0) + 1, np.int64)
    cap = 0 if cap is None else max(int(cap), 0)
    while True:
        col, val, total = np.empty(cap, np.int32), np.empty(cap, np.float32), _i64(-1)
        rc = call(row_ptr.ctypes.data, col.ctypes.data if cap else None, val.ctypes.data if cap else None, cap, total)
        if rc == ICL_OK and total.value <= cap:
            return row_ptr, col[:total.value], val[:total.value]
        if rc not in (ICL_OK, ICL_ERR_ARG) or total.value <= cap:
            raise ICLError(rc, "%s: bad argument" % what)
        cap = total.value  # the size query's answer, or a hint that was too small


def _pairs_matrix(D):
    """The value matrix of a *_from_matrix call -> (C-contiguous 2-D float32 array, its address or None when it is empty)."""
    D = np.asarray(D, np.float32)
    if D.ndim != 2:
        raise ValueError("D must be 2-D")
    if not D.flags.c_contiguous:
        D = np.ascontiguousarray(D)
    return D, (D.ctypes.data if D.size else None)


def pairs_within_from_matrix(D, threshold, n=None):
    """icl_pairs_within_from_matrix (host only, no GPU): Context.pairs_within's rule and layout applied to values the caller holds: the
    strict lower triangle of the first n (default: all) rows and columns of D -> (row_ptr, col, val).  Raises ICLError(ICL_ERR_ARG)."""
    D, Dp = _pairs_matrix(D)
    ld = D.shape[1]
    n = D.shape[0] if n is None else int(n)
    if n > D.shape[0]:
        raise ValueError("n = %d rows asked of a matrix of %d" % (n, D.shape[0]))
    L = load()
    return _pairs_two_calls(n, lambda rp, c, v, cap, tot: L.icl_pairs_within_from_matrix(Dp, n, ld, float(threshold), rp, c, v, cap, C.byref(tot)),
                            "icl_pairs_within_from_matrix")


def pairs_between_from_matrix(D, threshold, exclude=None, n=None):
    """icl_pairs_between_from_matrix (host only, no GPU): Context.pairs_between's rule and layout applied to values the caller holds: D
    is nq x ld float32, n (default ld) columns of each row are pairs, exclude[i] (None / -1: none) is left out of row i ->
    (row_ptr int64[nq + 1], col, val).  Raises ICLError(ICL_ERR_ARG)."""
    D, Dp = _pairs_matrix(D)
    nq, ld = D.shape
    n = ld if n is None else int(n)
    ex = _nearest_exclude(nq, exclude)
    L = load()
    return _pairs_two_calls(nq, lambda rp, c, v, cap, tot: L.icl_pairs_between_from_matrix(Dp, nq, n, ld, float(threshold), _ptr(ex), rp, c, v, cap,
                                                                                          C.byref(tot)), "icl_pairs_between_from_matrix")


def pair_groups(row_ptr, col):
    """icl_pair_groups (host only): the connected components of the pair graph of a CSR list -> (group int32[n], n_groups): group[i] is the
    smallest index of i's component, n_groups the number of components of two or more.  Raises ICLError(ICL_ERR_ARG) for a malformed list."""
    rp = np.ascontiguousarray(np.asarray(row_ptr).reshape(-1), np.int64)
    if len(rp) < 1:
        raise ValueError("row_ptr needs n + 1 entries")
    cl = np.ascontiguousarray(np.asarray(col).reshape(-1), np.int32)
    n = len(rp) - 1
    if len(cl) < max(int(rp[-1]), 0):
        raise ValueError("%d col entries for row_ptr[n] = %d" % (len(cl), rp[-1]))
    group, ng = np.empty(n, np.int32), _i64(0)
    rc = load().icl_pair_groups(n, rp.ctypes.data, cl.ctypes.data if cl.size else None, group.ctypes.data if n else None, C.byref(ng))
    if rc != ICL_OK:
        raise ICLError(rc, "icl_pair_groups: bad argument")
    return group, int(ng.value)


def _byte_view(buf):
    """(address, length, keep-alive) of an encoded image held as bytes / bytearray / memoryview / contiguous numpy.uint8, or of None (an
    empty source: address 0).  Nothing is copied: the address is the object's own buffer, and the keep-alive reference is held by the
    caller for as long as the library may read it."""
    if buf is None:
        return 0, 0, None
    if isinstance(buf, np.ndarray):
        if buf.dtype != np.uint8 or not buf.flags.c_contiguous:
            raise TypeError("an image buffer must be contiguous uint8")
        a = buf
    else:
        m = buf if isinstance(buf, memoryview) else memoryview(buf)
        if not m.c_contiguous or m.itemsize != 1:
            raise TypeError("an image buffer must be contiguous bytes")
        if m.nbytes == 0:
            return 0, 0, None
        a = np.frombuffer(m, np.uint8)  # a view of the same memory (read-only for bytes)
    return (a.ctypes.data if a.size else 0), int(a.size), a


def _byte_arrays(bufs):
    """The data / bytes arrays of a batched memory call -> (void*[n], int64[n], n, keep-alive list)."""
    views = [_byte_view(b) for b in bufs]
    n = len(views)
    data = (C.c_void_p * max(1, n))(*[v[0] or None for v in views])
    size = (C.c_int64 * max(1, n))(*[v[1] for v in views])
    return data, size, n, [v[2] for v in views]


def requests_layout(n, n_labels, head=HEAD_DENSE0):
    """icl_requests_layout (host only): where each request's combined rows live -> (e_off int64[nreq], d int32[nreq], e_len):
    d[r] = head + n_labels[r], e_off[r] = sum of n[q] * d[q] over q < r."""
    n = np.ascontiguousarray(n, np.int32)
    n_labels = np.ascontiguousarray(n_labels, np.int32)
    if n.shape != n_labels.shape or n.ndim != 1:
        raise ValueError("n and n_labels must be 1-D and of one length")
    e_off, d, e_len = np.zeros(max(len(n), 1), np.int64), np.zeros(max(len(n), 1), np.int32), _i64()
    rc = load().icl_requests_layout(len(n), n.ctypes.data, n_labels.ctypes.data, head, e_off.ctypes.data, d.ctypes.data, C.byref(e_len))
    if rc != ICL_OK:
        raise ICLError(rc, "icl_requests_layout: bad argument")
    return e_off[:len(n)], d[:len(n)], int(e_len.value)


def pack_requests(requests, head=HEAD_DENSE0):
    """The arguments of icl_cluster_requests (host only) for requests = [(paths, labels_per_image, n_labels, min_size, max_size), ...],
    labels_per_image[i] being image i's list of column indices within the request's label set (-1: a label the set does not hold; an empty
    list and duplicates are fine) -> dict(paths, n, n_labels, label_off, label_idx, min_size, max_size, img_off, e_off, d, e_len)."""
    paths, n, nl, off, idx, mn, mx = [], [], [], [0], [], [], []
    for r, (ps, labels, n_labels, lo, hi) in enumerate(requests):
        if len(labels) != len(ps):
            raise ValueError("request %d: %d images, %d label lists" % (r, len(ps), len(labels)))
        paths += list(ps)
        n.append(len(ps))
        nl.append(int(n_labels))
        for li in labels:
            li = [int(j) for j in li]
            if any(j < -1 or j >= int(n_labels) for j in li):
                raise ValueError("request %d: label index outside [-1, %d)" % (r, n_labels))
            idx += li
            off.append(len(idx))
        mn.append(int(lo))
        mx.append(int(hi))
    n = np.array(n, np.int32)
    e_off, d, e_len = requests_layout(n, nl, head)
    return dict(paths=paths, n=n, n_labels=np.array(nl, np.int32), label_off=np.array(off, np.int64), label_idx=np.array(idx, np.int32),
                min_size=np.array(mn, np.int32), max_size=np.array(mx, np.int32),
                img_off=np.concatenate([[0], np.cumsum(n, dtype=np.int64)]), e_off=e_off, d=d, e_len=e_len)


class Context:
    """One GPU, one stream (icl_ctx)."""

    def __init__(self, device=0):
        L = load()
        h = _vp()
        rc = L.icl_create(device, C.byref(h))
        if rc != ICL_OK:
            msg = L.icl_last_error(None)
            raise ICLError(rc, msg.decode() if msg else "")
        self.h = h
        self.L = L
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.L.icl_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- memory ---------------------------------------------------------------------------------------
    def malloc(self, nbytes):
        p = _vp()
        check(self.h, self.L.icl_dev_malloc(self.h, int(nbytes), C.byref(p)))
        return p.value or 0

    def free(self, p):
        check(self.h, self.L.icl_dev_free(self.h, _vp(p)))

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        check(self.h, self.L.icl_memcpy_h2d(self.h, _vp(dptr), arr.ctypes.data, arr.nbytes))

    def d2h(self, arr, dptr):
        assert arr.flags["C_CONTIGUOUS"]
        check(self.h, self.L.icl_memcpy_d2h(self.h, arr.ctypes.data, _vp(dptr), arr.nbytes))

    def sync(self):
        check(self.h, self.L.icl_sync(self.h))

    def _on_device_copies(self, ins, outs, call):
        """The dev=True forms of the host methods: call(*device pointers) on device buffers of the arrays ins (uploaded) and outs
        (downloaded once the call's work has finished); an empty array gets a buffer of 16 bytes and no copy."""
        bufs = []
        try:
            for a in tuple(ins) + tuple(outs):
                bufs.append(self.malloc(max(a.nbytes, 16)))
            for p, a in zip(bufs, ins):
                if a.size:
                    self.h2d(p, a)
            call(*bufs)
            self.sync()
            for p, a in zip(bufs[len(ins):], outs):
                if a.size:
                    self.d2h(a, p)
        finally:
            for p in bufs:
                self.free(p)

    def device_info(self):
        buf = C.create_string_buffer(256)
        ncu = _int()
        hbm = _i64()
        check(self.h, self.L.icl_device_info(self.h, buf, 256, C.byref(ncu), C.byref(hbm)))
        return buf.value.decode(), ncu.value, hbm.value

    # -- profiling ------------------------------------------------------------------------------------
    def prof_enable(self, mask=-1):
        """mask: bit k brackets kernel class k with HIP events (True/-1 = all, False/0 = off)."""
        if mask is True:
            mask = -1
        check(self.h, self.L.icl_prof_enable(self.h, int(mask)))

    def prof_reset(self):
        check(self.h, self.L.icl_prof_reset(self.h))

    def prof_query(self, k):
        ms, fl, by = C.c_double(), C.c_double(), C.c_double()
        n = _i64()
        check(self.h, self.L.icl_prof_query(self.h, k, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)))
        return dict(ms=ms.value, launches=n.value, flops=fl.value, bytes=by.value)

    def last_stage_ms(self):
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        check(self.h, self.L.icl_last_stage_ms(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(embed_ms=a.value, dist_ms=b.value, merge_ms=c.value)

    def last_ward_stats(self):
        v = [_i64() for _ in range(4)]
        check(self.h, self.L.icl_last_ward_stats(self.h, *[C.byref(x) for x in v]))
        return dict(merges=v[0].value, steps=v[1].value, single_pick_steps=v[2].value, sum_live=v[3].value)

    def last_ward_bound_violations(self):
        """Exact values the last merge loop found below the lower bound they replaced (must be 0)."""
        return int(self.L.icl_last_ward_bound_violations(self.h))

    def last_ward_mode(self):
        """(row_mode, init_bounds) of the last merge loop: include/imageclust.h ICL_ROWS_*."""
        a, b = C.c_int32(0), C.c_int32(0)
        check(self.h, self.L.icl_last_ward_mode(self.h, C.byref(a), C.byref(b)))
        return a.value, bool(b.value)

    def last_ward_layout(self):
        """(complete_rows, row_pitch, int8_bounds) of the last merge loop's distance matrix: include/imageclust.h icl_last_ward_layout."""
        a, b, c = C.c_int32(0), C.c_int64(0), C.c_int32(0)
        check(self.h, self.L.icl_last_ward_layout(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return bool(a.value), int(b.value), bool(c.value)

    def distance_bounds_check(self, E, kind=0):
        """Every pair's distance bound against its exact value (include/imageclust.h icl_distance_bounds_check_dev):
        dict(below, above, unflagged, mean_gap, mean_val, sum_gap, sum_val).  E: float32 [n][d] (host array or CUDA tensor)."""
        import numpy as np
        import torch

        t = E if isinstance(E, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(E, dtype=np.float32))
        t = t.to("cuda:%d" % self.device, dtype=torch.float32).contiguous()
        n, d = t.shape
        a, b, u = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        g, v = C.c_double(0), C.c_double(0)
        check(self.h, self.L.icl_distance_bounds_check_dev(self.h, C.c_void_p(t.data_ptr()), n, d, kind, C.byref(a), C.byref(b), C.byref(u), C.byref(g), C.byref(v)))
        pairs = n * (n - 1) / 2
        return {"below": a.value, "above": b.value, "unflagged": u.value, "mean_gap": g.value / pairs, "mean_val": v.value / pairs, "sum_gap": g.value, "sum_val": v.value}

    def ward_dump_pairs(self, ids, d):
        """The working matrix of the last cluster() call for the pairs of the creation ids `ids` (include/imageclust.h icl_ward_dump_pairs_dev):
        dict(ids, sizes [L], centroids [L][d], row_filled [L], entries / mirror [L][L] uint32 (raw bits, sign bit = lower bound), lb_g1, lb_delta2
        (float32), row_mode, complete_rows, n, d, merges, max_size)."""
        import numpy as np

        ids = np.ascontiguousarray(ids, np.int32)
        L = len(ids)
        sizes, filled, info = np.zeros(L, np.int32), np.zeros(L, np.int32), np.zeros(6, np.int32)
        cent = np.zeros((L, d), np.float32)
        ent, mir = np.zeros((L, L), np.uint32), np.zeros((L, L), np.uint32)
        g1, d2 = C.c_float(0), C.c_float(0)
        check(self.h, self.L.icl_ward_dump_pairs_dev(self.h, ids.ctypes.data, L, d, sizes.ctypes.data, cent.ctypes.data, filled.ctypes.data, ent.ctypes.data,
                                                     mir.ctypes.data, C.byref(g1), C.byref(d2), info.ctypes.data))
        return {"ids": ids, "sizes": sizes, "centroids": cent, "row_filled": filled.astype(bool), "entries": ent, "mirror": mir,
                "lb_g1": np.float32(g1.value), "lb_delta2": np.float32(d2.value), "row_mode": int(info[0]), "complete_rows": bool(info[1]),
                "n": int(info[2]), "d": int(info[3]), "merges": int(info[4]), "max_size": int(info[5])}

    # -- model / embed --------------------------------------------------------------------------------
    def load_synthetic(self, seed=1):
        check(self.h, self.L.icl_model_load_synthetic(self.h, seed))

    def load_blob(self, blob):
        buf = np.frombuffer(blob, np.uint8)
        check(self.h, self.L.icl_model_load_blob(self.h, buf.ctypes.data, buf.nbytes))

    def load_onnx(self, path):
        check(self.h, self.L.icl_model_load_onnx(self.h, os.fsencode(path)))

    def set_batch(self, b):
        check(self.h, self.L.icl_set_batch(self.h, b))

    def conv_stats(self):
        """(launches on conv_p8_kernel, launches on the other convolution kernels) since the context was created."""
        a, b = C.c_int64(0), C.c_int64(0)
        check(self.h, self.L.icl_conv_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def conv_split_launches(self):
        """launches of conv_p8_kernel's split form (two workgroups per tile: the 7 x 7 layers) since the context was created."""
        a = C.c_int64(0)
        check(self.h, self.L.icl_conv_split_launches(self.h, C.byref(a)))
        return a.value

    def set_conv_options(self, p8_mode=1):
        """0 never, 1 auto, 2 every supported shape on the deep-pipelined 256x256x64 convolution kernel (include/imageclust.h ICL_CONV_P8_*)."""
        check(self.h, self.L.icl_set_conv_options(self.h, p8_mode))

    def set_forward_prune(self, on=True):
        """bf16 forward pass: compute only the pixels the next stage's stride reads (icl_set_forward_prune; results are bit-identical)."""
        check(self.h, self.L.icl_set_forward_prune(self.h, 1 if on else 0))

    def forward_prune_stats(self):
        """bottlenecks run in the pruned form since the context was created."""
        a = C.c_int64(0)
        check(self.h, self.L.icl_forward_prune_stats(self.h, C.byref(a)))
        return a.value

    def set_forward_prune_fused(self, on=True):
        """The same for stage 1's last block, which runs as one fused launch (icl_set_forward_prune_fused; only with set_forward_prune on)."""
        check(self.h, self.L.icl_set_forward_prune_fused(self.h, 1 if on else 0))

    def set_stem_max_blocks(self, max_blocks=0):
        """Tests only: cap the persistent grid of the stem kernels (icl_set_stem_max_blocks; 0 = no cap, the default)."""
        check(self.h, self.L.icl_set_stem_max_blocks(self.h, int(max_blocks)))

    def forward_prune_fused_stats(self):
        """launches of the fused bottleneck's pruned instantiation by the forward pass since the context was created."""
        a = C.c_int64(0)
        check(self.h, self.L.icl_forward_prune_fused_stats(self.h, C.byref(a)))
        return a.value

    def embed_u8(self, imgs, head=HEAD_POOLED, prec=PREC_FP32):
        imgs = np.ascontiguousarray(imgs, np.uint8).reshape(-1, IMG_BYTES)
        n = imgs.shape[0]
        out = np.empty((n, head), np.float32)
        check(self.h, self.L.icl_embed_u8(self.h, imgs.ctypes.data, n, head, prec, out.ctypes.data))
        return out

    def embed_u8_dev(self, d_imgs, n, d_out, head=HEAD_POOLED, prec=PREC_BF16):
        check(self.h, self.L.icl_embed_u8_dev(self.h, _vp(d_imgs), n, head, prec, _vp(d_out)))

    def embed_file(self, path, head=HEAD_DENSE0):
        out = np.empty(head, np.float32)
        check(self.h, self.L.icl_embed_file(self.h, os.fsencode(path), head, out.ctypes.data))
        return out

    def _files_call(self, fn, paths, *args):
        """Runs a batched file entry point; per-file failures come back in status (the call's code names the lowest failed index)."""
        enc = [os.fsencode(p) for p in paths]
        arr = (C.c_char_p * max(1, len(enc)))(*enc)
        status = np.zeros(len(enc), np.int32)
        rc = fn(self.h, arr, len(enc), *args, status.ctypes.data)
        failed = np.flatnonzero(status)
        if rc != ICL_OK and not (failed.size and status[failed[0]] == rc):
            check(self.h, rc)
        return status

    def embed_image_mem(self, data, head=HEAD_DENSE0):
        """icl_embed_image_mem: embed_file for an image held in memory (the same coalescing queue)."""
        p, n, keep = _byte_view(data)
        out = np.empty(head, np.float32)
        check(self.h, self.L.icl_embed_image_mem(self.h, _vp(p), n, head, out.ctypes.data))
        del keep
        return out

    def _mem_call(self, fn, bufs, *args):
        """_files_call for the memory twins: bufs are the encoded images (bytes / bytearray / memoryview / contiguous numpy.uint8; None or
        an empty buffer is that image's own failure).  The buffers are read in place and stay referenced until the call has returned."""
        data, size, n, keep = _byte_arrays(bufs)
        status = np.zeros(n, np.int32)
        rc = fn(self.h, data, size, n, *args, status.ctypes.data)
        del keep
        failed = np.flatnonzero(status)
        if rc != ICL_OK and not (failed.size and status[failed[0]] == rc):
            check(self.h, rc)
        return status

    def load_images_224_mem_dev(self, bufs, d_out, threads=0):
        """icl_load_images_224_mem_dev: load_images_224_dev for images held in memory."""
        return self._mem_call(self.L.icl_load_images_224_mem_dev, bufs, threads, _vp(d_out))

    def load_images_224_mem(self, bufs, threads=0):
        """icl_load_images_224_mem_dev through a device buffer -> (n x 224 x 224 x 3 u8, status)."""
        n = len(bufs)
        out = np.zeros((n, 224, 224, 3), np.uint8)
        d = self.malloc(max(1, n) * IMG_BYTES)
        try:
            status = self.load_images_224_mem_dev(bufs, d, threads)
            if n:
                self.d2h(out, d)
        finally:
            self.free(d)
        return out, status

    def embed_images_mem(self, bufs, head=HEAD_POOLED, prec=PREC_BF16, threads=0):
        """icl_embed_images_mem -> (E n x head fp32, status int32[n]); rows of failed images are NaN."""
        out = np.empty((len(bufs), head), np.float32)
        status = self._mem_call(self.L.icl_embed_images_mem, bufs, head, prec, threads, out.ctypes.data)
        return out, status

    def embed_images_mem_dev(self, bufs, d_out, head=HEAD_POOLED, prec=PREC_BF16, threads=0):
        """icl_embed_images_mem_dev: n x head fp32 rows into device memory d_out -> status (int32[n])."""
        return self._mem_call(self.L.icl_embed_images_mem_dev, bufs, head, prec, threads, _vp(d_out))

    def jpeg_coefs_mem(self, bufs, entropy=ENTROPY_HOST):
        """icl_jpeg_coefs_mem (test hook): jpeg_coefs_files for JPEGs held in memory."""
        data, size, n, keep = _byte_arrays(bufs)
        off = np.zeros(n + 1, np.int64)
        state = np.zeros(n, np.int32)
        check(self.h, self.L.icl_jpeg_coefs_mem(self.h, data, size, n, entropy, None, 0, off.ctypes.data, state.ctypes.data))
        buf = np.zeros(max(1, int(off[-1])), np.int16)
        check(self.h, self.L.icl_jpeg_coefs_mem(self.h, data, size, n, entropy, buf.ctypes.data, buf.size, off.ctypes.data, state.ctypes.data))
        del keep
        return [buf[off[i]:off[i + 1]] for i in range(n)], state

    # ---- the label service's downsizer and its JPEG encoder (rekognition.go:173-259) ----
    def jpeg_encode(self, rgb, quality=95):
        """icl_jpeg_encode_rgb (host): h x w x 3 u8 RGB -> the bytes of the JPEG file libjpeg's defaults write at this quality."""
        return jpeg_encode(rgb, quality)

    def jpeg_encode_dev(self, images, quality=95):
        """icl_jpeg_encode_rgb_dev: a list of h x w x 3 u8 RGB images of any sizes, uploaded and encoded in one call -> list of bytes."""
        imgs = [np.ascontiguousarray(a, np.uint8) for a in images]
        n = len(imgs)
        w = np.array([a.shape[1] for a in imgs], np.int32)
        h = np.array([a.shape[0] for a in imgs], np.int32)
        offs = np.zeros(n + 1, np.int64)
        for i, a in enumerate(imgs):
            offs[i + 1] = offs[i] + ((a.nbytes + 15) & ~15)
        flat = np.zeros(max(16, int(offs[-1])), np.uint8)
        for i, a in enumerate(imgs):
            flat[offs[i]:offs[i] + a.nbytes] = a.reshape(-1)
        cap = sum(int(self.L.icl_jpeg_encode_bound(int(w[i]), int(h[i]))) for i in range(n))
        out = np.zeros(max(1, cap), np.uint8)
        out_off = np.zeros(n + 1, np.int64)
        d = self.malloc(flat.nbytes)
        try:
            self.h2d(d, flat)
            check(self.h, self.L.icl_jpeg_encode_rgb_dev(self.h, _vp(d), offs.ctypes.data, w.ctypes.data, h.ctypes.data, n, quality,
                                                         out.ctypes.data, 0, out.nbytes, out_off.ctypes.data))
        finally:
            self.free(d)
        return [out[out_off[i]:out_off[i + 1]].tobytes() for i in range(n)]

    def downsize_image(self, path, max_bytes=MAX_IMAGE_SIZE, max_dim=MAX_IMAGE_DIM):
        return downsize_image(path, max_bytes, max_dim)

    def downsize_image_mem(self, data, max_bytes=MAX_IMAGE_SIZE, max_dim=MAX_IMAGE_DIM):
        return downsize_image_mem(data, max_bytes, max_dim)

    def _downsize_many(self, call, n, sizes_in):
        status = np.zeros(n, np.int32)
        out_off = np.zeros(n + 1, np.int64)
        cap = max(1, int(sum(sizes_in)))  # (an output is never larger than... only a guess: the call says what it needs)
        for _ in range(2):
            out = np.zeros(cap, np.uint8)
            rc = call(out.ctypes.data, out.nbytes, out_off.ctypes.data, status.ctypes.data)
            if rc == ICL_ERR_ARG and int(out_off[-1]) > cap:
                cap = int(out_off[-1])
                continue
            break
        failed = np.flatnonzero(status)
        if rc != ICL_OK and not (failed.size and status[failed[0]] == rc):
            check(self.h, rc)
        return [out[out_off[i]:out_off[i + 1]].tobytes() for i in range(n)], status

    def downsize_images(self, paths, max_bytes=MAX_IMAGE_SIZE, max_dim=MAX_IMAGE_DIM, threads=0):
        """icl_downsize_images -> (list of bytes, status int32[n]); a failed image has an empty entry."""
        enc = [os.fsencode(p) for p in paths]
        arr = (C.c_char_p * max(1, len(enc)))(*enc)
        sizes = [os.path.getsize(p) if os.path.exists(p) else 0 for p in paths]
        return self._downsize_many(lambda o, c, oo, st: self.L.icl_downsize_images(self.h, arr, len(enc), max_bytes, max_dim, threads, o, c, oo, st),
                                   len(enc), sizes)

    def downsize_images_mem(self, bufs, max_bytes=MAX_IMAGE_SIZE, max_dim=MAX_IMAGE_DIM, threads=0):
        """icl_downsize_images_mem: downsize_images for images held in memory."""
        data, size, n, keep = _byte_arrays(bufs)
        r = self._downsize_many(lambda o, c, oo, st: self.L.icl_downsize_images_mem(self.h, data, size, n, max_bytes, max_dim, threads, o, c, oo, st),
                                n, [int(size[i]) for i in range(n)])
        del keep
        return r

    def last_downsize_stats(self):
        """icl_last_downsize_stats of the last batched downsize call."""
        v = [C.c_int64(0) for _ in range(6)]
        ms = np.zeros(3, np.float64)
        check(self.h, self.L.icl_last_downsize_stats(self.h, *[C.byref(x) for x in v], ms.ctypes.data))
        keys = ["passthrough", "gpu_rebuilt", "host_decoded", "second_attempts", "bytes_in", "bytes_out"]
        d = {k: x.value for k, x in zip(keys, v)}
        d["stage_ms"] = {"host_decode": float(ms[0]), "gpu": float(ms[1]), "download": float(ms[2])}
        return d

    def load_images_224_dev(self, paths, d_out, threads=0):
        """icl_load_images_224_dev: n x 224x224x3 u8 rows into device memory d_out -> status (int32[n]); failed rows are zero."""
        return self._files_call(self.L.icl_load_images_224_dev, paths, threads, _vp(d_out))

    def load_images_224(self, paths, threads=0):
        """icl_load_images_224_dev through a device buffer -> (n x 224 x 224 x 3 u8, status)."""
        n = len(paths)
        out = np.zeros((n, 224, 224, 3), np.uint8)
        d = self.malloc(max(1, n) * IMG_BYTES)
        try:
            status = self.load_images_224_dev(paths, d, threads)
            if n:
                self.d2h(out, d)
        finally:
            self.free(d)
        return out, status

    def embed_files(self, paths, head=HEAD_POOLED, prec=PREC_BF16, threads=0):
        """icl_embed_files -> (E n x head fp32, status int32[n]); rows of failed files are NaN."""
        out = np.empty((len(paths), head), np.float32)
        status = self._files_call(self.L.icl_embed_files, paths, head, prec, threads, out.ctypes.data)
        return out, status

    def embed_files_dev(self, paths, d_out, head=HEAD_POOLED, prec=PREC_BF16, threads=0):
        """icl_embed_files_dev: n x head fp32 rows into device memory d_out -> status (int32[n])."""
        return self._files_call(self.L.icl_embed_files_dev, paths, head, prec, threads, _vp(d_out))

    def last_ingest_stats(self):
        g, h, u, s = _i64(), _i64(), _i64(), C.c_double()
        check(self.h, self.L.icl_last_ingest_stats(self.h, C.byref(g), C.byref(h), C.byref(u), C.byref(s)))
        return {"gpu_jpegs": g.value, "host_files": h.value, "upload_bytes": u.value, "host_decode_s": s.value}

    def set_ingest_options(self, entropy=ENTROPY_HOST):
        """icl_set_ingest_options: ENTROPY_GPU decodes qualifying baseline JPEGs' Huffman streams on the GPU (same rows, statuses, messages)."""
        check(self.h, self.L.icl_set_ingest_options(self.h, entropy))

    def last_entropy_stats(self):
        a, b, c, d = _i64(), _i64(), _i64(), _i64()
        check(self.h, self.L.icl_last_entropy_stats(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return {"gpu_entropy_jpegs": a.value, "host_entropy_jpegs": b.value, "redone_on_host": c.value, "stream_bytes": d.value}

    def jpeg_coefs_files(self, paths, entropy=ENTROPY_HOST):
        """icl_jpeg_coefs_files (test hook) -> ([int16 coefficients of file i, components 0, 1, 2 in natural order], state int32[n]):
        state 1 = decoded (and, on the GPU, accepted), 0 = rejected by the GPU check, -1 = does not qualify for the GPU decoder."""
        enc = [os.fsencode(p) for p in paths]
        arr = (C.c_char_p * max(1, len(enc)))(*enc)
        off = np.zeros(len(enc) + 1, np.int64)
        state = np.zeros(len(enc), np.int32)
        check(self.h, self.L.icl_jpeg_coefs_files(self.h, arr, len(enc), entropy, None, 0, off.ctypes.data, state.ctypes.data))
        buf = np.zeros(max(1, int(off[-1])), np.int16)
        check(self.h, self.L.icl_jpeg_coefs_files(self.h, arr, len(enc), entropy, buf.ctypes.data, buf.size, off.ctypes.data, state.ctypes.data))
        return [buf[off[i]:off[i + 1]] for i in range(len(enc))], state

    def set_png_options(self, png=PNG_HOST):
        """icl_set_png_options: PNG_GPU inflates and unfilters qualifying PNGs of the batched file calls on the GPU (same rows, statuses, messages)."""
        check(self.h, self.L.icl_set_png_options(self.h, png))

    def last_png_stats(self):
        a, b, c, d = _i64(), _i64(), _i64(), _i64()
        check(self.h, self.L.icl_last_png_stats(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return {"gpu_pngs": a.value, "host_pngs": b.value, "redone_on_host": c.value, "stream_bytes": d.value}

    def png_raw_files(self, paths, stage=0):
        """icl_png_raw_files (test hook) -> ([uint8 bytes of file i: the inflated stream (stage 0) or the unfiltered scanlines (stage 1)],
        state int32[n]): state 1 = accepted, 0 = rejected by the GPU check, -1 = does not qualify for the GPU route."""
        enc = [os.fsencode(p) for p in paths]
        arr = (C.c_char_p * max(1, len(enc)))(*enc)
        off = np.zeros(len(enc) + 1, np.int64)
        state = np.zeros(len(enc), np.int32)
        check(self.h, self.L.icl_png_raw_files(self.h, arr, len(enc), stage, None, 0, off.ctypes.data, state.ctypes.data))
        buf = np.zeros(max(1, int(off[-1])), np.uint8)
        check(self.h, self.L.icl_png_raw_files(self.h, arr, len(enc), stage, buf.ctypes.data, buf.size, off.ctypes.data, state.ctypes.data))
        return [buf[off[i]:off[i + 1]] for i in range(len(enc))], state

    def last_error(self):
        msg = self.L.icl_last_error(self.h)
        return msg.decode() if msg else ""

    def set_file_options(self, prec=PREC_FP32, window_us=2000, max_batch=256):
        """How icl_embed_file coalesces concurrent callers (workflow.go:156-175: one goroutine per image)."""
        check(self.h, self.L.icl_set_file_options(self.h, prec, window_us, max_batch))

    def file_batch_stats(self):
        b, i = _i64(), _i64()
        check(self.h, self.L.icl_file_batch_stats(self.h, C.byref(b), C.byref(i)))
        return {"batches": b.value, "images": i.value}

    def update_distance_matrix(self, D, centroids, sizes, r1, r2):
        """UpdateDistanceMatrix (clustering.go:76-96): D n x n before the merge; centroids / sizes of the n-1 clusters after
        RemoveClusters + append (new cluster last) -> (n-1) x (n-1)."""
        D = np.ascontiguousarray(D, np.float32)
        Cm = np.ascontiguousarray(centroids, np.float32)
        sz = np.ascontiguousarray(sizes, np.int32)
        n = D.shape[0]
        out = np.zeros((n - 1, n - 1), np.float32)
        check(self.h, self.L.icl_update_distance_matrix(self.h, D.ctypes.data, n, D.shape[1], Cm.ctypes.data, sz.ctypes.data,
                                                        Cm.shape[1] if Cm.ndim == 2 else 0, int(r1), int(r2), out.ctypes.data, n - 1))
        return out

    def conv2d_fused(self, x_nhwc, w_oihw, scale, shift, stride=1, pad=0, residual=None, relu=True, prec=PREC_FP32):
        x = np.ascontiguousarray(x_nhwc, np.float32)
        w = np.ascontiguousarray(w_oihw, np.float32)
        B, H, _, Cin = x.shape
        Cout, _, k, _ = w.shape
        Ho = (H + 2 * pad - k) // stride + 1
        y = np.empty((B, Ho, Ho, Cout), np.float32)
        sc = np.ascontiguousarray(scale, np.float32)
        sh = np.ascontiguousarray(shift, np.float32)
        r = None if residual is None else np.ascontiguousarray(residual, np.float32)
        check(self.h, self.L.icl_conv2d_fused(self.h, prec, x.ctypes.data, B, H, Cin, w.ctypes.data, Cout, k, stride, pad,
                                              sc.ctypes.data, sh.ctypes.data, None if r is None else r.ctypes.data,
                                              1 if relu else 0, y.ctypes.data))
        return y

    def conv1x1_mapped(self, x_nhwc, w, scale, shift, y_full, sub, residual=None, relu=True):
        """The mapped 1x1 launch of a pruned bottleneck's c3 (icl_conv1x1_mapped, bf16): x [B][Ho][Ho][Cin] compact, w [Cout][Cin],
        residual / y_full [B][H][H][Cout].  Returns a copy of y_full in which the pixels (sub * oy, sub * ox) hold the result."""
        f = lambda a: np.ascontiguousarray(a, np.float32)
        x, w, sc, sh = f(x_nhwc), f(w), f(scale), f(shift)
        y = np.array(y_full, np.float32, order="C", copy=True)
        B, H, _, Cout = y.shape
        Ho = (H - 1) // int(sub) + 1
        Cin = x.shape[3]
        assert x.shape == (B, Ho, Ho, Cin) and w.shape == (Cout, Cin) and sc.shape == (Cout,) and sh.shape == (Cout,)
        r = None if residual is None else f(residual)
        assert r is None or r.shape == y.shape
        check(self.h, self.L.icl_conv1x1_mapped(self.h, x.ctypes.data, B, H, int(sub), Cin, w.ctypes.data, Cout, sc.ctypes.data, sh.ctypes.data,
                                                None if r is None else r.ctypes.data, 1 if relu else 0, y.ctypes.data))
        return y

    def conv2d_dual(self, x_nhwc, w1, x2_nhwc, w2, stride2, scale, shift, relu=True, prec=PREC_FP32):
        """The dual-operand launch of block 0 of stages 2-4 (icl_conv2d_dual): x [B][Ho][Ho][Cin] . w1 [Cout][Cin] +
        x2[:, ::stride2, ::stride2] [B][H2][H2][Cin2] . w2 [Cout][Cin2], then scale, shift and ReLU -> [B][Ho][Ho][Cout]."""
        f = lambda a: np.ascontiguousarray(a, np.float32)
        x, x2, w1, w2, sc, sh = f(x_nhwc), f(x2_nhwc), f(w1), f(w2), f(scale), f(shift)
        B, Ho, _, Cin = x.shape
        _, H2, _, Cin2 = x2.shape
        Cout = w1.shape[0]
        assert x2.shape[0] == B and w1.shape == (Cout, Cin) and w2.shape == (Cout, Cin2) and sc.shape == (Cout,) and sh.shape == (Cout,)
        y = np.empty((B, Ho, Ho, Cout), np.float32)
        check(self.h, self.L.icl_conv2d_dual(self.h, prec, x.ctypes.data, B, Ho, Cin, w1.ctypes.data, x2.ctypes.data, H2, Cin2, w2.ctypes.data,
                                             int(stride2), Cout, sc.ctypes.data, sh.ctypes.data, 1 if relu else 0, y.ctypes.data))
        return y

    def embed_taps(self, imgs, tap, prec=PREC_FP32):
        """The forward pass of the loaded model on one batch, ended at a tap (icl_embed_taps): the tensor after the stem + maxpool
        (tap 0) or after bottleneck tap (1..16) as fp32 NHWC."""
        a = np.ascontiguousarray(imgs, np.uint8).reshape(-1, IMG_BYTES)
        out = np.empty((a.shape[0],) + tap_shape(tap), np.float32)
        check(self.h, self.L.icl_embed_taps(self.h, prec, a.ctypes.data, a.shape[0], int(tap), out.ctypes.data))
        return out

    def stem_pool(self, imgs, prec=PREC_FP32):
        """conv0 + BN + ReLU + maxpool of the loaded model in one launch: [B][56][56][64] fp32."""
        a = np.ascontiguousarray(imgs, np.uint8).reshape(-1, IMG_BYTES)
        out = np.empty((a.shape[0], 56, 56, 64), np.float32)
        check(self.h, self.L.icl_stem_pool(self.h, prec, a.ctypes.data, a.shape[0], out.ctypes.data))
        return out

    def bottleneck56(self, x_nhwc, w1, bn1, w2_oihw, bn2, w3, bn3, wds=None, bnds=None):
        """One fused stage-1 bottleneck (bf16): bnK = (scale, shift).  wds / bnds select the downsample-branch form."""
        f = lambda a: np.ascontiguousarray(a, np.float32)
        x = f(x_nhwc)
        B, H, W, Cin = x.shape
        y = np.empty((B, H, W, 256), np.float32)
        keep = [x, f(w1), f(bn1[0]), f(bn1[1]), f(w2_oihw), f(bn2[0]), f(bn2[1]), f(w3), f(bn3[0]), f(bn3[1])]
        keep += [None, None, None] if wds is None else [f(wds), f(bnds[0]), f(bnds[1])]
        ptr = [None if a is None else a.ctypes.data for a in keep]
        check(self.h, self.L.icl_bottleneck56(self.h, ptr[0], B, H, W, Cin, *ptr[1:], y.ctypes.data))
        return y

    def bottleneck56_sub(self, x_nhwc, w1, bn1, w2_oihw, bn2, w3, bn3, sub, fill):
        """bottleneck56's identity form with the launch's sub (1: whole, 2: the pruned instantiation, pixels (2 oy, 2 ox) only) on an output
        tensor preset to the 16-bit pattern `fill`: what the launch does not write comes back as fill << 16 (fp32 bits)."""
        f = lambda a: np.ascontiguousarray(a, np.float32)
        x = f(x_nhwc)
        B, H, W, Cin = x.shape
        assert Cin == 256
        y = np.empty((B, H, W, 256), np.float32)
        keep = [x, f(w1), f(bn1[0]), f(bn1[1]), f(w2_oihw), f(bn2[0]), f(bn2[1]), f(w3), f(bn3[0]), f(bn3[1])]
        ptr = [a.ctypes.data for a in keep]
        check(self.h, self.L.icl_bottleneck56_sub(self.h, ptr[0], B, H, W, *ptr[1:], int(sub), int(fill), y.ctypes.data))
        return y

    def synth_images_dev(self, seed, first, n, mode, d_out):
        check(self.h, self.L.icl_synth_images_dev(self.h, seed, first, n, mode, _vp(d_out)))

    # -- Ward -----------------------------------------------------------------------------------------
    def ward_distance_matrix(self, centroids, sizes=None):
        Cm = np.ascontiguousarray(centroids, np.float32)
        n, d = Cm.shape
        D = np.zeros((n, n), np.float32)
        sp = None
        if sizes is not None:
            sizes = np.ascontiguousarray(sizes, np.int32)
            sp = sizes.ctypes.data
        check(self.h, self.L.icl_ward_distance_matrix(self.h, Cm.ctypes.data, sp, n, d, D.ctypes.data, n))
        return D

    def nearest(self, Q, E, k, q_size=None, e_size=None, max_size=0, exclude=None, dev=False):
        """icl_nearest: for each row of Q the k rows of E of smallest WardDistance (sizes q_size / e_size, None: all 1), bit for bit the
        reference's values, ascending by (value, j), NaN last -> (idx int32[nq][k], val float32[nq][k]); short rows end in idx -1, val
        MaxFloat32.  exclude[i] (-1: none) names a column row i skips (a self-join passes arange(n)); max_size > 0 leaves out every pair
        whose sizes add up to more.  dev=True runs icl_nearest_dev on device copies instead of the host entry point."""
        Qm, Em = np.ascontiguousarray(Q, np.float32), np.ascontiguousarray(E, np.float32)
        if Qm.ndim != 2 or Em.ndim != 2 or Qm.shape[1] != Em.shape[1]:
            raise ValueError("Q and E must be 2-D with rows of one length, got %s and %s" % (Qm.shape, Em.shape))
        (nq, d), n = Qm.shape, Em.shape[0]
        qs, es, ex = _nearest_side(nq, q_size, "q_size"), _nearest_side(n, e_size, "e_size"), _nearest_exclude(nq, exclude)
        kk = max(int(k), 1)
        idx, val = np.empty((nq, kk), np.int32), np.empty((nq, kk), np.float32)
        if not dev:
            check(self.h, self.L.icl_nearest(self.h, _ptr(Qm), _ptr(qs), nq, _ptr(Em), _ptr(es), n, d, int(k), int(max_size), _ptr(ex),
                                             idx.ctypes.data, val.ctypes.data))
            return idx, val
        self._on_device_copies((Qm, Em), (idx, val), lambda dQ, dE, dI, dV: self.nearest_dev(dQ, nq, dE, n, d, k, dI, dV, qs, es, max_size, ex))
        return idx, val

    def nearest_dev(self, d_Q, nq, d_E, n, d, k, d_idx, d_val, q_size=None, e_size=None, max_size=0, exclude=None):
        """icl_nearest_dev: Q (nq x d), E (n x d), idx and val (nq x k) are device pointers; q_size, e_size and exclude host arrays
        or None.  Enqueued on the context's stream: sync() before reading the outputs through another stream."""
        qs, es, ex = _nearest_side(nq, q_size, "q_size"), _nearest_side(n, e_size, "e_size"), _nearest_exclude(nq, exclude)
        check(self.h, self.L.icl_nearest_dev(self.h, _as_vp(d_Q), _ptr(qs), nq, _as_vp(d_E), _ptr(es), n, d, int(k), int(max_size), _ptr(ex),
                                             _as_vp(d_idx), _as_vp(d_val)))

    def set_nearest_options(self, column_splits=0):
        """icl_set_nearest_options: workgroups per band of 128 query rows the library's column tiles are split over (0: the engine decides
        from nq, n and the CU count).  Same results for every count."""
        check(self.h, self.L.icl_set_nearest_options(self.h, int(column_splits)))

    def last_nearest_stats(self):
        """The last nearest[_dev]: column splits used, 128 x 128 tiles run, pairs evaluated, workspace bytes."""
        info = (C.c_int64 * 4)()
        check(self.h, self.L.icl_last_nearest_stats(self.h, info))
        return {"splits": info[0], "tiles": info[1], "pairs": info[2], "workspace_bytes": info[3]}

    def cluster_fit(self, Q, cluster_of, C, k_alt=1, q_size=None, c_size=None, max_size=0, dev=False):
        """icl_cluster_fit: for each row of Q (sizes q_size, None: all 1) its exact WardDistance to its own cluster cluster_of[i] of C
        (sizes c_size; negative: frozen; -1 in cluster_of: none, cost MaxFloat32) and its k_alt nearest other clusters -- frozen ones
        and, with max_size > 0, those it would push above max_size left out --, and per cluster the number of rows that name it, the row
        of smallest own cost and the row of largest -> dict(own float32[nq], alt_idx int32[nq][k_alt], alt_val float32[nq][k_alt],
        listed, rep, worst int32[K]).  dev=True runs icl_cluster_fit_dev on device copies instead of the host entry point."""
        Qm, Cm = np.ascontiguousarray(Q, np.float32), np.ascontiguousarray(C, np.float32)
        if Qm.ndim != 2 or Cm.ndim != 2 or Qm.shape[1] != Cm.shape[1]:
            raise ValueError("Q and C must be 2-D with rows of one length, got %s and %s" % (Qm.shape, Cm.shape))
        (nq, d), K = Qm.shape, Cm.shape[0]
        qs, cs, cof = _nearest_side(nq, q_size, "q_size"), _nearest_side(K, c_size, "c_size"), _nearest_side(nq, cluster_of, "cluster_of")
        out = _fit_outputs(nq, K, k_alt)
        if not dev:
            check(self.h, self.L.icl_cluster_fit(self.h, _ptr(Qm), _ptr(qs), _ptr(cof), nq, _ptr(Cm), _ptr(cs), K, d, int(k_alt), int(max_size),
                                                 *[_ptr(a) for a in out]))
            return _fit_result(out)
        self._on_device_copies((Qm, Cm), out, lambda dQ, dC, *d_out: self.cluster_fit_dev(dQ, cof, nq, dC, K, d, k_alt, *d_out, q_size=qs, c_size=cs,
                                                                                        max_size=max_size))
        return _fit_result(out)

    def cluster_fit_dev(self, d_Q, cluster_of, nq, d_C, K, d, k_alt, d_own, d_alt_idx, d_alt_val, d_listed=None, d_rep=None, d_worst=None,
                        q_size=None, c_size=None, max_size=0):
        """icl_cluster_fit_dev: Q (nq x d), C (K x d) and the six outputs are device pointers (the per-cluster ones may be None);
        cluster_of, q_size and c_size host arrays.  Enqueued on the context's stream: sync() before reading the outputs."""
        qs, cs, cof = _nearest_side(nq, q_size, "q_size"), _nearest_side(K, c_size, "c_size"), _nearest_side(nq, cluster_of, "cluster_of")
        check(self.h, self.L.icl_cluster_fit_dev(self.h, _as_vp(d_Q), _ptr(qs), _ptr(cof), nq, _as_vp(d_C), _ptr(cs), K, d, int(k_alt), int(max_size),
                                                 _as_vp(d_own), _as_vp(d_alt_idx), _as_vp(d_alt_val), _as_vp(d_listed), _as_vp(d_rep), _as_vp(d_worst)))

    def last_fit_stats(self):
        """The last cluster_fit[_dev]: column splits used, 128 x 128 tiles run, pairs evaluated, workspace bytes."""
        info = (C.c_int64 * 4)()
        check(self.h, self.L.icl_last_fit_stats(self.h, info))
        return {"splits": info[0], "tiles": info[1], "pairs": info[2], "workspace_bytes": info[3]}

    def ward_values_at(self, Q, E, qi, ej, q_size=None, e_size=None, dev=False):
        """icl_ward_values_at: the exact WardDistance of each listed pair (row qi[p] of Q, row ej[p] of E; sizes None: all 1, a negative
        e_size a frozen cluster's item count) -> float32[np].  dev=True runs icl_ward_values_at_dev on device copies."""
        Qm, Em = np.ascontiguousarray(Q, np.float32), np.ascontiguousarray(E, np.float32)
        if Qm.ndim != 2 or Em.ndim != 2 or Qm.shape[1] != Em.shape[1]:
            raise ValueError("Q and E must be 2-D with rows of one length, got %s and %s" % (Qm.shape, Em.shape))
        (nq, d), n = Qm.shape, Em.shape[0]
        a, b = np.ascontiguousarray(np.asarray(qi).reshape(-1), np.int32), np.ascontiguousarray(np.asarray(ej).reshape(-1), np.int32)
        if len(a) != len(b):
            raise ValueError("%d row indices for %d column indices" % (len(a), len(b)))
        qs, es = _nearest_side(nq, q_size, "q_size"), _nearest_side(n, e_size, "e_size")
        val = np.empty(len(a), np.float32)
        if not dev:
            check(self.h, self.L.icl_ward_values_at(self.h, _ptr(Qm), _ptr(qs), nq, _ptr(Em), _ptr(es), n, d, _ptr(a), _ptr(b), len(a), _ptr(val)))
            return val
        self._on_device_copies((Qm, Em), (val,), lambda dQ, dE, dV: self.ward_values_at_dev(dQ, nq, dE, n, d, a, b, dV, q_size=qs, e_size=es))
        return val

    def ward_values_at_dev(self, d_Q, nq, d_E, n, d, qi, ej, d_val, q_size=None, e_size=None):
        """icl_ward_values_at_dev: Q (nq x d), E (n x d) and val (len(qi) floats) are device pointers; the pair list and the sizes host
        arrays.  Enqueued on the context's stream."""
        a, b = np.ascontiguousarray(np.asarray(qi).reshape(-1), np.int32), np.ascontiguousarray(np.asarray(ej).reshape(-1), np.int32)
        qs, es = _nearest_side(nq, q_size, "q_size"), _nearest_side(n, e_size, "e_size")
        check(self.h, self.L.icl_ward_values_at_dev(self.h, _as_vp(d_Q), _ptr(qs), nq, _as_vp(d_E), _ptr(es), n, d, _ptr(a), _ptr(b), len(a), _as_vp(d_val)))

    def fold_centroids(self, E, row_ptr, member, size=None, dev=False):
        """icl_fold_centroids: the centroid of each group of rows of E -- group g is the rows member[row_ptr[g]:row_ptr[g + 1]], in that
        order, with item counts size (None: all 1) -- as the reference holds it after merging the members one at a time (MergeClusters,
        clustering.go:29-47, bit for bit) -> (C float32[K][d], size_out int32[K]); an empty group gives a row of +0.0 and size 0.
        dev=True runs icl_fold_centroids_dev on device copies instead of the host entry point."""
        Em = np.ascontiguousarray(E, np.float32)
        if Em.ndim != 2:
            raise ValueError("E must be 2-D, got %s" % (Em.shape,))
        n, d = Em.shape
        rp, mb, sz = _fold_lists(row_ptr, member), np.ascontiguousarray(np.asarray(member).reshape(-1), np.int32), _nearest_side(n, size, "size")
        K = len(rp) - 1
        Cm, so = np.empty((K, d), np.float32), np.empty(K, np.int32)
        if not dev:
            check(self.h, self.L.icl_fold_centroids(self.h, _ptr(Em), _ptr(sz), n, d, _ptr(rp), _ptr(mb), K, _ptr(Cm), _ptr(so)))
            return Cm, so
        self._on_device_copies((Em,), (Cm,), lambda dE, dC: so.__setitem__(slice(None), self.fold_centroids_dev(dE, n, d, rp, mb, dC, size=sz)))
        return Cm, so

    def fold_centroids_dev(self, d_E, n, d, row_ptr, member, d_C, size=None):
        """icl_fold_centroids_dev: E (n x d) and C (K x d) are device pointers; row_ptr, member and size host arrays -> size_out int32[K].
        Enqueued on the context's stream: sync() before reading C through another stream."""
        rp, mb, sz = _fold_lists(row_ptr, member), np.ascontiguousarray(np.asarray(member).reshape(-1), np.int32), _nearest_side(n, size, "size")
        K = len(rp) - 1
        so = np.empty(K, np.int32)
        check(self.h, self.L.icl_fold_centroids_dev(self.h, _as_vp(d_E), _ptr(sz), n, d, _ptr(rp), _ptr(mb), K, _as_vp(d_C), _ptr(so)))
        return so

    def last_fold_stats(self):
        """The last fold_centroids[_dev]: groups, member rows read, the longest group's length, workspace bytes."""
        info = (C.c_int64 * 4)()
        check(self.h, self.L.icl_last_fold_stats(self.h, info))
        return {"groups": info[0], "rows": info[1], "longest": info[2], "workspace_bytes": info[3]}

    def pairs_within(self, E, threshold, size=None, cap=None):
        """icl_pairs_within: EVERY pair of rows of E whose WardDistance (sizes `size`, None: all 1) is at most threshold, bit for bit the
        reference's values, as a CSR list over the strict lower triangle -> (row_ptr int64[n + 1], col int32[total], val float32[total]):
        row i's partners j < i, ascending in j, are col[row_ptr[i]:row_ptr[i + 1]].  NaN values are never listed.  The size query and the
        call proper are both made here; cap, a guess of the total, saves the query when it is large enough."""
        Em = np.ascontiguousarray(E, np.float32)
        if Em.ndim != 2:
            raise ValueError("E must be 2-D, got %s" % (Em.shape,))
        n, d = Em.shape
        sz = _nearest_side(n, size, "size")
        return self._pairs_calls(n, cap, lambda rp, c, v, cp, tot: self.L.icl_pairs_within(self.h, _ptr(Em), _ptr(sz), n, d, float(threshold),
                                                                                          rp, c, v, cp, C.byref(tot)))

    def pairs_within_dev(self, d_E, n, d, threshold, size=None, cap=None):
        """icl_pairs_within_dev on rows that are on the device already (d_E: n x d floats) -> (row_ptr, col, val) on the host, as
        pairs_within.  col and val live on the device during the call and are downloaded here."""
        sz = _nearest_side(n, size, "size")
        return self._pairs_calls(n, cap, self._pairs_dev_call(lambda rp, dc, dv, cp, tot: self.L.icl_pairs_within_dev(
            self.h, _as_vp(d_E), _ptr(sz), n, d, float(threshold), rp, dc, dv, cp, C.byref(tot))))

    def pairs_between(self, Q, L, threshold, q_size=None, l_size=None, exclude=None, cap=None):
        """icl_pairs_between: EVERY pair (row i of Q, row j of L) whose WardDistance (sizes q_size / l_size, None: all 1) is at most
        threshold, nearest()'s values bit for bit, as a CSR list over the queries -> (row_ptr int64[nq + 1], col int32[total],
        val float32[total]): query i's library partners, ascending in j, are col[row_ptr[i]:row_ptr[i + 1]].  exclude[i] (None / -1: none)
        is left out of row i; NaN values are never listed; there is no cap on a query's partners and no max_size ban.  The size query
        and the call proper are both made here; cap, a guess of the total, saves the query when it is large enough."""
        Qm, Lm = np.ascontiguousarray(Q, np.float32), np.ascontiguousarray(L, np.float32)
        if Qm.ndim != 2 or Lm.ndim != 2 or Qm.shape[1] != Lm.shape[1]:
            raise ValueError("Q and L must be 2-D with rows of one length, got %s and %s" % (Qm.shape, Lm.shape))
        (nq, d), n = Qm.shape, Lm.shape[0]
        qs, ls, ex = _nearest_side(nq, q_size, "q_size"), _nearest_side(n, l_size, "l_size"), _nearest_exclude(nq, exclude)
        return self._pairs_calls(nq, cap, lambda rp, c, v, cp, tot: self.L.icl_pairs_between(
            self.h, _ptr(Qm), _ptr(qs), nq, _ptr(Lm), _ptr(ls), n, d, float(threshold), _ptr(ex), rp, c, v, cp, C.byref(tot)), "icl_pairs_between")

    def pairs_between_dev(self, d_Q, nq, d_L, n, d, threshold, q_size=None, l_size=None, exclude=None, cap=None):
        """icl_pairs_between_dev on rows that are on the device already (d_Q: nq x d floats, d_L: n x d) -> (row_ptr, col, val) on the
        host, as pairs_between.  col and val live on the device during the call and are downloaded here."""
        qs, ls, ex = _nearest_side(nq, q_size, "q_size"), _nearest_side(n, l_size, "l_size"), _nearest_exclude(nq, exclude)
        return self._pairs_calls(nq, cap, self._pairs_dev_call(lambda rp, dc, dv, cp, tot: self.L.icl_pairs_between_dev(
            self.h, _as_vp(d_Q), _ptr(qs), nq, _as_vp(d_L), _ptr(ls), n, d, float(threshold), _ptr(ex), rp, dc, dv, cp, C.byref(tot))),
            "icl_pairs_between_dev")

    def last_pairs_between_stats(self):
        """The last pairs_between[_dev]: column splits used, 128 x 128 tiles the count pass ran, tiles with a hit (the fill pass's), pairs
        evaluated in both passes, workspace bytes."""
        info = (C.c_int64 * 5)()
        check(self.h, self.L.icl_last_pairs_between_stats(self.h, info))
        return {"splits": info[0], "tiles": info[1], "hit_tiles": info[2], "pairs": info[3], "workspace_bytes": info[4]}

    def _pairs_dev_call(self, dev_call):
        """A _dev entry point as _pairs_two_calls' call: dev_call(row_ptr, d_col, d_val, cap, total) -> code gets device buffers of cap
        entries, and what it lists is downloaded into the host arrays of the same length."""
        def call(rp, c, v, cp, tot):
            bufs = [self.malloc(cp * 4), self.malloc(cp * 4)] if cp else [None, None]
            try:
                rc = dev_call(rp, bufs[0], bufs[1], cp, tot)
                if rc == ICL_OK and 0 < tot.value <= cp:
                    self.sync()
                    check(self.h, self.L.icl_memcpy_d2h(self.h, c, _vp(bufs[0]), tot.value * 4))
                    check(self.h, self.L.icl_memcpy_d2h(self.h, v, _vp(bufs[1]), tot.value * 4))
                return rc
            finally:
                for p in bufs:
                    if p is not None:
                        self.free(p)

        return call

    def _pairs_calls(self, n, cap, call, what="icl_pairs_within"):
        try:
            return _pairs_two_calls(n, call, what, cap)
        except ICLError as e:
            msg = self.L.icl_last_error(self.h)
            raise ICLError(e.code, msg.decode() if msg else "") from None

    def last_pairs_stats(self):
        """The last pairs_within[_dev]: 128 x 128 tiles the count pass ran, tiles with a hit (the fill pass's), pairs evaluated in both
        passes, workspace bytes."""
        info = (C.c_int64 * 4)()
        check(self.h, self.L.icl_last_pairs_stats(self.h, info))
        return {"tiles": info[0], "hit_tiles": info[1], "pairs": info[2], "workspace_bytes": info[3]}

    def merge_centroid(self, ca, sa, cb, sb):
        ca = np.ascontiguousarray(ca, np.float32)
        cb = np.ascontiguousarray(cb, np.float32)
        out = np.empty_like(ca)
        check(self.h, self.L.icl_merge_centroid(self.h, ca.ctypes.data, int(sa), cb.ctypes.data, int(sb), ca.shape[0],
                                                out.ctypes.data))
        return out

    def find_closest(self, D):
        D = np.ascontiguousarray(D, np.float32)
        n = D.shape[0]
        i, j = _i64(), _i64()
        check(self.h, self.L.icl_find_closest(self.h, D.ctypes.data if n else None, n, D.shape[1] if n else 0,
                                              C.byref(i), C.byref(j)))
        return i.value, j.value

    def cluster(self, E, min_size, max_size, update=UPDATE_EXACT):
        """-> (cluster_id[n], member_rank[n], n_clusters); raises ICLError(ICL_ERR_CONSTRAINT) for (nil,false)."""
        E = np.ascontiguousarray(E, np.float32)
        n, d = E.shape
        cid = np.full(max(n, 1), -1, np.int32)
        rank = np.full(max(n, 1), -1, np.int32)
        nc = _i32()
        check(self.h, self.L.icl_cluster(self.h, E.ctypes.data if E.size else None, n, d, min_size, max_size, update,
                                         cid.ctypes.data, rank.ctypes.data, C.byref(nc)))
        return cid[:n], rank[:n], nc.value

    def cluster_many(self, problems, want_merges=False, raise_on_error=False):
        """Many independent exact-mode cluster() calls in one (icl_cluster_many): problems = [(E, min_size, max_size), ...] -> a list of
        (cluster_id, member_rank, n_clusters, status) per problem, each equal to what cluster() gives for that problem alone (status:
        ICL_OK or the problem's error code, with rows of -1); want_merges=True appends the problem's merge log (n_merges x 2 creation
        ids, as last_merges()).  raise_on_error=True raises the lowest failed problem's error instead."""
        pk = pack_many(problems)
        nprob = len(problems)
        outs = cid, rank, nc, nm, st, mg = _many_outputs(pk, want_merges)
        rc = self.L.icl_cluster_many(self.h, nprob, pk["E"].ctypes.data, pk["E"].size, pk["e_off"].ctypes.data, pk["n"].ctypes.data,
                                     pk["d"].ctypes.data, pk["min_size"].ctypes.data, pk["max_size"].ctypes.data, cid.ctypes.data,
                                     rank.ctypes.data, nc.ctypes.data, nm.ctypes.data, mg.ctypes.data if want_merges else None, st.ctypes.data)
        return self._many_results(rc, pk, outs, raise_on_error)

    def _many_results(self, rc, pk, outs, raise_on_error=False):
        """What a many-call returns (_unpack_many), from its code and its _many_outputs.  Raises when the code is not a problem's own -- an
        argument or device error: no per-problem status was written -- or, with raise_on_error, for the lowest failed problem."""
        if rc != ICL_OK and (raise_on_error or (outs[4][:len(pk["n"])] < 0).any()):
            check(self.h, rc)
        return _unpack_many(pk, *outs)

    def set_many_options(self, mid_mode=MANY_MID_AUTO):
        """icl_set_many_options: whether cluster_many runs problems of 257 to 2048 rows one workgroup each (MANY_MID_ON), never
        (MANY_MID_OFF), or when the call holds enough of them for that to win (MANY_MID_AUTO).  Same results in every mode."""
        check(self.h, self.L.icl_set_many_options(self.h, mid_mode))

    def last_many_stats(self):
        """Problems of the last cluster_many[_dev] call by route, and the number of groups its mid-size problems ran in."""
        a, b, c, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        check(self.h, self.L.icl_last_many_stats(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return {"small": a.value, "mid": b.value, "large": c.value, "mid_groups": d.value}

    def cluster_requests(self, requests, head=HEAD_DENSE0, prec=PREC_FP32, threads=0, want_merges=False, want_E=False):
        """icl_cluster_requests: workflow.Run for many requests in one call, requests as pack_requests() takes them -> a list of
        (cluster_id, member_rank, n_clusters, status[, merge log][, E]) per request, as cluster_many() gives them; status is ICL_OK,
        ICL_ERR_CONSTRAINT or the code of the request's lowest failed file (rows of -1 then).  want_E=True appends the request's combined
        rows (n x d float32).  self.last_file_status holds every image's code afterwards and self.last_requests_rc the call's own (the lowest
        failed request's; last_error() names it).  Raises for an argument or device error."""
        pk = pack_requests(requests, head)
        enc = [os.fsencode(p) for p in pk["paths"]]
        arr = (C.c_char_p * max(1, len(enc)))(*enc)
        return self._requests_call(self.L.icl_cluster_requests, pk, (arr,), head, prec, threads, want_merges, want_E)

    def cluster_requests_mem(self, requests, head=HEAD_DENSE0, prec=PREC_FP32, threads=0, want_merges=False, want_E=False):
        """icl_cluster_requests_mem: cluster_requests with each request's images held in memory -- requests = [(buffers, labels_per_image,
        n_labels, min_size, max_size), ...], buffers as embed_images_mem takes them.  Same return value and attributes."""
        pk = pack_requests(requests, head)
        data, size, _, keep = _byte_arrays(pk["paths"])
        try:
            return self._requests_call(self.L.icl_cluster_requests_mem, pk, (data, size), head, prec, threads, want_merges, want_E)
        finally:
            del keep

    def _requests_call(self, fn, pk, images, head, prec, threads, want_merges, want_E):
        nreq, rows = len(pk["n"]), int(pk["img_off"][-1])
        outs = cid, rank, nc, nm, st, mg = _many_outputs(pk, want_merges)
        fst = np.zeros(max(rows, 1), np.int32)
        E = np.zeros(max(pk["e_len"], 1), np.float32) if want_E else None
        ptr = lambda a: a.ctypes.data
        rc = fn(self.h, nreq, *images, ptr(pk["n"]), ptr(pk["n_labels"]), ptr(pk["label_off"]), ptr(pk["label_idx"]),
                                         ptr(pk["min_size"]), ptr(pk["max_size"]), head, prec, threads, ptr(cid), ptr(rank), ptr(nc), ptr(nm),
                                         ptr(mg) if want_merges else None, ptr(st), ptr(fst), ptr(E) if want_E else None)
        out = self._many_results(rc, pk, outs)
        self.last_file_status, self.last_requests_rc = fst[:rows].copy(), rc
        if want_E:
            out = [r + (E[int(o):int(o) + int(k) * int(w)].reshape(int(k), int(w)).copy(),)
                   for r, o, k, w in zip(out, pk["e_off"], pk["n"], pk["d"])]
        return out

    def last_requests_ms(self):
        """Stage wall times of the last cluster_requests: files -> embedding rows, assembly, clustering (ms)."""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        check(self.h, self.L.icl_last_requests_ms(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return {"embed_ms": a.value, "assemble_ms": b.value, "cluster_ms": c.value}

    def cluster_many_dev(self, d_E, e_len, e_off, n, d, min_size, max_size, want_merges=False):
        """icl_cluster_many_dev on a device buffer of e_len floats; per-problem arrays as pack_many() gives them.  Same result as cluster_many()."""
        pk = dict(e_off=np.ascontiguousarray(e_off, np.int64), n=np.ascontiguousarray(n, np.int32), d=np.ascontiguousarray(d, np.int32),
                  min_size=np.ascontiguousarray(min_size, np.int32), max_size=np.ascontiguousarray(max_size, np.int32))
        nprob = len(pk["n"])
        pk["img_off"] = np.concatenate([[0], np.cumsum(pk["n"], dtype=np.int64)])
        outs = cid, rank, nc, nm, st, mg = _many_outputs(pk, want_merges)
        rc = self.L.icl_cluster_many_dev(self.h, nprob, _vp(d_E), int(e_len), pk["e_off"].ctypes.data, pk["n"].ctypes.data, pk["d"].ctypes.data,
                                         pk["min_size"].ctypes.data, pk["max_size"].ctypes.data, cid.ctypes.data, rank.ctypes.data,
                                         nc.ctypes.data, nm.ctypes.data, mg.ctypes.data if want_merges else None, st.ctypes.data)
        return self._many_results(rc, pk, outs)

    def cluster_many_apart(self, problems, want_merges=False, want_centroids=False, raise_on_error=False, dev=False):
        """icl_cluster_many_apart: cluster_many_seeded with keep-apart constraints.  problems = [(C, seed_size, min_size, max_size, k_target,
        apart_class | None, apart_pairs | None), ...]: apart_class holds one int per seed (0: none; two seeds of one non-zero class are never
        merged into one cluster), apart_pairs (i, j) seed indices that stay apart; a merged cluster inherits the bans of both parents.
        Arguments and return value are cluster_many_seeded's; a malformed constraint raises ICLError(ICL_ERR_ARG)."""
        classes, pairs, off = [], [], [0]
        for p, pr in enumerate(problems):
            m = len(np.asarray(pr[1]).reshape(-1))
            cl = np.zeros(m, np.int32) if len(pr) < 6 or pr[5] is None else np.asarray(pr[5], np.int32).reshape(-1)
            if len(cl) != m:
                raise ValueError("problem %d: %d apart_class entries for %d seeds" % (p, len(cl), m))
            pa = np.zeros((0, 2), np.int32) if len(pr) < 7 or pr[6] is None else np.asarray(pr[6], np.int32).reshape(-1, 2)
            classes.append(cl)
            pairs.append(pa)
            off.append(off[-1] + len(pa))
        cls = np.ascontiguousarray(np.concatenate(classes + [np.zeros(1, np.int32)]), np.int32)
        par = np.ascontiguousarray(np.concatenate(pairs + [np.zeros((1, 2), np.int32)]), np.int32)
        apart = (cls, np.array(off, np.int64), par)
        return self.cluster_many_seeded(problems, want_merges, want_centroids, raise_on_error, dev, _apart=apart)

    def cluster_many_seeded(self, problems, want_merges=False, want_centroids=False, raise_on_error=False, dev=False, _apart=None):
        """icl_cluster_many_seeded: the clustering loop started from existing clusters.  problems = [(C, seed_size, min_size, max_size[,
        k_target]), ...]: C holds one centroid row per seed, seed_size[i] its item count (negative: frozen, never merged), k_target > 0
        the number of clusters to stop at (else CalculateOptimalClusters of the item total) -> a list of (cluster_id, seed_rank,
        n_clusters, status) per problem at seed granularity, as cluster_many() gives them per image; want_merges appends the merge log
        (seed i has id i, merge t id m + t), want_centroids then appends C_out (m x d: the row of each final cluster's rank-0 seed is
        the cluster's centroid, every other row zero).  dev=True runs icl_cluster_many_seeded_dev on a device copy (the same result).
        (_apart: cluster_many_apart's constraint arrays; the call is then icl_cluster_many_apart[_dev].)"""
        pk = pack_many([(pr[0], pr[2], pr[3]) for pr in problems])
        nprob = len(problems)
        sizes = [np.asarray(pr[1], np.int32).reshape(-1) for pr in problems]
        for p, sz in enumerate(sizes):
            if len(sz) != int(pk["n"][p]):
                raise ValueError("problem %d: %d seed sizes for %d centroid rows" % (p, len(sz), int(pk["n"][p])))
        ss = np.ascontiguousarray(np.concatenate(sizes + [np.zeros(0, np.int32)]), np.int32)
        ss = ss if ss.size else np.zeros(1, np.int32)
        kt = np.array([int(pr[4]) if len(pr) > 4 else 0 for pr in problems] + ([] if nprob else [0]), np.int32)
        outs = cid, rank, nc, nm, st, mg = _many_outputs(pk, want_merges)
        co = np.zeros(pk["E"].size, np.float32) if want_centroids else None
        ptr = lambda a: a.ctypes.data if a is not None else None
        tail = (ptr(pk["e_off"]), ptr(pk["n"]), ptr(pk["d"]), ptr(ss), ptr(pk["min_size"]), ptr(pk["max_size"]), ptr(kt)) + \
               (tuple(ptr(a) for a in _apart) if _apart is not None else ()) + (ptr(cid), ptr(rank), ptr(nc), ptr(nm), ptr(mg), ptr(st))
        fn_host = self.L.icl_cluster_many_seeded if _apart is None else self.L.icl_cluster_many_apart
        fn_dev = self.L.icl_cluster_many_seeded_dev if _apart is None else self.L.icl_cluster_many_apart_dev
        if dev:
            dE, dC = self.malloc(max(pk["E"].nbytes, 4)), self.malloc(max(pk["E"].nbytes, 4)) if want_centroids else None
            try:
                self.h2d(dE, pk["E"])
                if want_centroids:
                    self.h2d(dC, co)
                rc = fn_dev(self.h, nprob, _vp(dE), pk["E"].size, *tail, _vp(dC) if want_centroids else None)
                if want_centroids:
                    self.d2h(co, dC)
            finally:
                self.free(dE)
                if dC is not None:
                    self.free(dC)
        else:
            rc = fn_host(self.h, nprob, ptr(pk["E"]), pk["E"].size, *tail, ptr(co))
        out = self._many_results(rc, pk, outs, raise_on_error)
        if want_centroids:
            out = [r + (co[int(o):int(o) + int(k) * int(w)].reshape(int(k), int(w)).copy(),)
                   for r, o, k, w in zip(out, pk["e_off"], pk["n"], pk["d"])]
        return out

    @staticmethod
    def _apart_args(m, apart_class, apart_pairs):
        """the constraint arguments of icl_cluster_apart[_dev] -> (the arrays to keep alive, (apart_class, n_pairs, apart_pairs))"""
        cl = None if apart_class is None else np.ascontiguousarray(np.asarray(apart_class, np.int32).reshape(-1))
        if cl is not None and len(cl) != m:
            raise ValueError("%d apart_class entries for %d seeds" % (len(cl), m))
        pa = np.zeros((0, 2), np.int32) if apart_pairs is None else np.ascontiguousarray(np.asarray(apart_pairs, np.int32).reshape(-1, 2))
        return (cl, pa), (cl.ctypes.data if cl is not None and m else None, len(pa), pa.ctypes.data if len(pa) else None)

    def cluster_apart(self, C_, seed_size, min_size, max_size, k_target=0, apart_class=None, apart_pairs=None, want_centroids=True, dev=False):
        """icl_cluster_apart: ONE constrained seeded problem (cluster_many_apart's semantics: apart_class one int per seed, apart_pairs (i, j)
        seed indices, merged clusters inherit both parents' bans) on the large-N engine, any number of seeds.  Arguments and return value
        are cluster_seeded's; a malformed constraint raises ICLError(ICL_ERR_ARG).  dev=True runs icl_cluster_apart_dev on a device copy."""
        m = len(np.asarray(seed_size).reshape(-1))
        return self.cluster_seeded(C_, seed_size, min_size, max_size, k_target, want_centroids, dev, _apart=self._apart_args(m, apart_class, apart_pairs))

    def cluster_apart_dev(self, d_C, m, d, seed_size, min_size, max_size, k_target=0, apart_class=None, apart_pairs=None, d_C_out=None):
        """icl_cluster_apart_dev on m x d device floats: cluster_seeded_dev with the constraints of cluster_apart (host arrays)."""
        return self.cluster_seeded_dev(d_C, m, d, seed_size, min_size, max_size, k_target, d_C_out, _apart=self._apart_args(m, apart_class, apart_pairs))

    def _seeded_fns(self, update, _apart):
        """(host call, _dev call) of a seeded problem: icl_cluster_seeded, icl_cluster_seeded_fast for UPDATE_LW, icl_cluster_apart under constraints"""
        if update not in (UPDATE_EXACT, UPDATE_LW):
            raise ValueError("unknown update mode %r" % (update,))
        if _apart:
            if update == UPDATE_LW:
                raise ICLError(ICL_ERR_UNSUPPORTED, "FAST mode (UPDATE_LW) keeps no keep-apart constraints")
            return self.L.icl_cluster_apart, self.L.icl_cluster_apart_dev
        if update == UPDATE_LW:
            return self.L.icl_cluster_seeded_fast, self.L.icl_cluster_seeded_fast_dev
        return self.L.icl_cluster_seeded, self.L.icl_cluster_seeded_dev

    def cluster_seeded(self, C_, seed_size, min_size, max_size, k_target=0, want_centroids=True, dev=False, _apart=None, update=UPDATE_EXACT):
        """icl_cluster_seeded: ONE seeded problem (cluster_many_seeded's semantics) on the large-N engine, any number of seeds -> (cluster_id,
        seed_rank, n_clusters, status, merges, C_out); C_out is None without want_centroids.  status is ICL_OK, ICL_ERR_CONSTRAINT or
        ICL_ERR_UNSUPPORTED (rows of -1, C_out zero); every other error raises.  dev=True runs icl_cluster_seeded_dev on a device copy.
        update=UPDATE_LW: icl_cluster_seeded_fast[_dev], the same problem in FAST mode (MFMA matrix scaled by the sizes, Lance-Williams rows).
        (_apart: cluster_apart's constraint arguments; the call is then icl_cluster_apart[_dev], exact only.)"""
        Cs = np.ascontiguousarray(C_, np.float32)
        m, d = Cs.shape
        ss = np.ascontiguousarray(np.asarray(seed_size, np.int32).reshape(-1))
        if len(ss) != m:
            raise ValueError("%d seed sizes for %d centroid rows" % (len(ss), m))
        cid, rank = np.full(max(m, 1), -1, np.int32), np.full(max(m, 1), -1, np.int32)
        nc = _i32()
        co = np.zeros((m, d), np.float32) if want_centroids else None
        args = (m, d, _ptr(ss), int(min_size), int(max_size), int(k_target)) + (_apart[1] if _apart else ()) + (cid.ctypes.data, rank.ctypes.data, C.byref(nc))
        fn_host, fn_dev = self._seeded_fns(update, _apart)
        if dev:
            dE = self.malloc(max(Cs.nbytes, 16))
            dC = self.malloc(max(Cs.nbytes, 16)) if want_centroids else None
            try:
                self.h2d(dE, Cs)
                rc = fn_dev(self.h, _vp(dE), *args, _vp(dC) if want_centroids else None)
                if want_centroids and Cs.size and rc in (ICL_OK, ICL_ERR_CONSTRAINT, ICL_ERR_UNSUPPORTED):
                    self.d2h(co, dC)
            finally:
                self.free(dE)
                if dC is not None:
                    self.free(dC)
        else:
            rc = fn_host(self.h, Cs.ctypes.data if m else None, *args, _ptr(co))
        if rc not in (ICL_OK, ICL_ERR_CONSTRAINT, ICL_ERR_UNSUPPORTED):
            check(self.h, rc)
        merges = self.last_merges() if rc == ICL_OK else np.zeros((0, 2), np.int32)
        return cid[:m], rank[:m], nc.value, rc, merges, co

    def cluster_seeded_dev(self, d_C, m, d, seed_size, min_size, max_size, k_target=0, d_C_out=None, _apart=None, update=UPDATE_EXACT):
        """icl_cluster_seeded_dev on m x d device floats (d_C_out: m x d device floats, or None) -> (cluster_id, seed_rank, n_clusters,
        status); the log is last_merges().  update=UPDATE_LW: icl_cluster_seeded_fast_dev.  (_apart: as cluster_seeded's.)"""
        ss = np.ascontiguousarray(np.asarray(seed_size, np.int32).reshape(-1))
        cid, rank = np.full(max(m, 1), -1, np.int32), np.full(max(m, 1), -1, np.int32)
        nc = _i32()
        fn = self._seeded_fns(update, _apart)[1]
        rc = fn(self.h, _vp(d_C), m, d, ss.ctypes.data if m else None, int(min_size), int(max_size), int(k_target), *(_apart[1] if _apart else ()),
                cid.ctypes.data, rank.ctypes.data, C.byref(nc), _vp(d_C_out) if d_C_out is not None else None)
        if rc not in (ICL_OK, ICL_ERR_CONSTRAINT, ICL_ERR_UNSUPPORTED):
            check(self.h, rc)
        return cid[:m], rank[:m], nc.value, rc

    def cluster_dev(self, d_E, n, d, min_size, max_size, update=UPDATE_EXACT):
        cid = np.full(max(n, 1), -1, np.int32)
        rank = np.full(max(n, 1), -1, np.int32)
        nc = _i32()
        check(self.h, self.L.icl_cluster_dev(self.h, _vp(d_E), n, d, min_size, max_size, update, cid.ctypes.data,
                                             rank.ctypes.data, C.byref(nc)))
        return cid[:n], rank[:n], nc.value

    def set_ward_options(self, dist_mode=0):
        """0 auto, 1 exact distances everywhere, 2 (= 3) distance bounds in the initial matrix + on-demand exact evaluation, 4 the rows of new clusters as Lance-Williams lower bounds too (include/imageclust.h ICL_DIST_*)."""
        check(self.h, self.L.icl_set_ward_options(self.h, dist_mode))

    def embed_cluster_dev(self, d_imgs, n, d_E, min_size, max_size, prec=PREC_BF16, update=UPDATE_EXACT, overlap=True):
        """workflow.go:84-94 on one GPU: embed n resident images into d_E (n x 2048, device) and cluster them; overlap=True runs
        the distance rows of already-embedded images beside the later forward passes."""
        cid = np.full(max(n, 1), -1, np.int32)
        rank = np.full(max(n, 1), -1, np.int32)
        nc = _i32()
        check(self.h, self.L.icl_embed_cluster_dev(self.h, _vp(d_imgs), n, prec, min_size, max_size, update, 1 if overlap else 0, _vp(d_E),
                                                   cid.ctypes.data, rank.ctypes.data, C.byref(nc)))
        return cid[:n], rank[:n], nc.value

    # ---- distance tiles over several GPUs (building blocks; imageclust_amd/distributed.py and Group use them) ----
    def ward_prepare(self, n, d):
        check(self.h, self.L.icl_ward_prepare(self.h, n, d))

    def ward_distance_rows_dev(self, d_E, n, d, row_lo, row_hi, d_span):
        check(self.h, self.L.icl_ward_distance_rows_dev(self.h, _vp(d_E), n, d, row_lo, row_hi, _vp(d_span)))

    def ward_unpack_spans_dev(self, spans):
        """spans: [(row_lo, row_hi, device pointer readable from this GPU)]: packed rows -> the rows of the distance matrix."""
        k = len(spans)
        lo = (C.c_int64 * k)(*[int(t[0]) for t in spans])
        hi = (C.c_int64 * k)(*[int(t[1]) for t in spans])
        pp = (C.c_void_p * k)(*[int(t[2]) for t in spans])
        check(self.h, self.L.icl_ward_unpack_spans_dev(self.h, k, lo, hi, pp))

    def cluster_prefilled_dev(self, d_E, n, d, min_size, max_size, own_lo, own_hi, update=UPDATE_EXACT):
        cid = np.full(max(n, 1), -1, np.int32)
        rank = np.full(max(n, 1), -1, np.int32)
        nc = _i32()
        check(self.h, self.L.icl_cluster_prefilled_dev(self.h, _vp(d_E), n, d, min_size, max_size, update, own_lo, own_hi,
                                                       cid.ctypes.data, rank.ctypes.data, C.byref(nc)))
        return cid[:n], rank[:n], nc.value

    def distance_mfma(self, E):
        """MFMA distance tile (K6): lower triangle (incl. zero diagonal) of 0.5*|e_i-e_j|^2, n x n fp32."""
        E = np.ascontiguousarray(E, np.float32)
        n, d = E.shape
        dE, dD = self.malloc(max(E.nbytes, 16)), self.malloc(max(n * n * 4, 16))
        try:
            self.h2d(dE, E)
            check(self.h, self.L.icl_distance_mfma_dev(self.h, _vp(dE), n, d, _vp(dD), n))
            out = np.zeros((n, n), np.float32)
            self.d2h(out, dD)
        finally:
            self.free(dE)
            self.free(dD)
        return np.tril(out)

    def distance_mfma_seeded_dev(self, d_C, m, d, seed_size, d_D, ld=None):
        """icl_distance_mfma_seeded_dev: the matrix icl_cluster_seeded_fast clusters -- distance_mfma's entries scaled by the two seeds' item
        counts (seed_size: host, sign ignored) -- into m rows of pitch ld (default m) of device floats; lower triangle and zero diagonal."""
        ss = np.ascontiguousarray(np.asarray(seed_size, np.int32).reshape(-1))
        if len(ss) != m:
            raise ValueError("%d seed sizes for %d rows" % (len(ss), m))
        check(self.h, self.L.icl_distance_mfma_seeded_dev(self.h, _vp(d_C), m, d, ss.ctypes.data if m else None, _vp(d_D), m if ld is None else ld))

    def distance_mfma_seeded(self, C_, seed_size):
        """distance_mfma_seeded_dev on host rows -> m x m fp32, lower triangle incl. the zero diagonal."""
        Cs = np.ascontiguousarray(C_, np.float32)
        m, d = Cs.shape
        dC, dD = self.malloc(max(Cs.nbytes, 16)), self.malloc(max(m * m * 4, 16))
        try:
            self.h2d(dC, Cs)
            self.distance_mfma_seeded_dev(dC, m, d, seed_size, dD)
            out = np.zeros((m, m), np.float32)
            self.d2h(out, dD)
        finally:
            self.free(dC)
            self.free(dD)
        return np.tril(out)

    def last_merges(self):
        n = self.L.icl_last_merges(self.h, None, 0)
        out = np.zeros((max(n, 1), 2), np.int32)
        self.L.icl_last_merges(self.h, out.ctypes.data, n)
        return out[:n]

    def last_merge_values(self):
        """Ward distance of the pair joined by each merge of last_merges() (the dendrogram heights)."""
        n = self.L.icl_last_merge_values(self.h, None, 0)
        out = np.zeros(max(n, 1), np.float32)
        self.L.icl_last_merge_values(self.h, out.ctypes.data, n)
        return out[:n]


def ward_rows_partition(n, parts, part):
    """Rows [lo, hi) of the initial distance matrix that part `part` of `parts` computes: whole 128-row tile rows, equal AREA."""
    lo, hi = _i64(), _i64()
    rc = load().icl_ward_rows_partition(n, parts, part, C.byref(lo), C.byref(hi))
    if rc:
        raise ICLError(rc, "icl_ward_rows_partition")
    return lo.value, hi.value


def ward_span(row_lo, row_hi):
    """(float offset, float count) of rows [row_lo, row_hi) in the packed lower triangle (rows padded to 4 floats)."""
    off, cnt = _i64(), _i64()
    rc = load().icl_ward_span(row_lo, row_hi, C.byref(off), C.byref(cnt))
    if rc:
        raise ICLError(rc, "icl_ward_span")
    return off.value, cnt.value


class Group:
    """Several GPUs behind one handle (icl_group_*): one process, one context + host thread per GPU."""

    def __init__(self, devices):
        self.L = load()
        self.g = _vp()
        dv = (C.c_int32 * len(devices))(*devices)
        rc = self.L.icl_group_create(dv, len(devices), C.byref(self.g))
        if rc:
            raise ICLError(rc, (self.L.icl_last_error(None) or b"").decode())

    def _check(self, rc):
        if rc:
            raise ICLError(rc, (self.L.icl_group_last_error(self.g) or b"").decode())

    def close(self):
        if self.g:
            self.L.icl_group_destroy(self.g)
            self.g = _vp()

    def set_options(self, tiles_mode=0, merge_mode=0):
        """Who builds the initial distance matrix: TILES_AUTO (GPU 0 alone below 6 GPUs), TILES_LOCAL, TILES_DISTRIBUTED; where the
        merge loop runs: MERGE_GPU0, MERGE_SHARDED (every GPU a replica of the state, the new rows' blocks dealt out)."""
        self._check(self.L.icl_group_set_options(self.g, tiles_mode, merge_mode))

    def size(self):
        return self.L.icl_group_size(self.g)

    def load_synthetic(self, seed=1):
        self._check(self.L.icl_group_load_synthetic(self.g, seed))

    def load_blob(self, blob: bytes):
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        self._check(self.L.icl_group_load_blob(self.g, C.addressof(buf), len(blob)))

    def embed_u8(self, imgs, head=HEAD_POOLED, prec=PREC_BF16):
        imgs = np.ascontiguousarray(imgs, np.uint8).reshape(-1, IMG_BYTES)
        out = np.empty((imgs.shape[0], head), np.float32)
        self._check(self.L.icl_group_embed_u8(self.g, imgs.ctypes.data, imgs.shape[0], head, prec, out.ctypes.data))
        return out

    def cluster(self, E, min_size, max_size, update=UPDATE_EXACT):
        E = np.ascontiguousarray(E, np.float32)
        n, d = E.shape
        cid = np.full(max(n, 1), -1, np.int32)
        rank = np.full(max(n, 1), -1, np.int32)
        nc = _i32()
        self._check(self.L.icl_group_cluster(self.g, E.ctypes.data, n, d, min_size, max_size, update, cid.ctypes.data, rank.ctypes.data, C.byref(nc)))
        return cid[:n], rank[:n], nc.value

    def last_merges(self, i=0):
        """Merge log (creation ids) / Ward values of the last cluster call, from the context of GPU i (icl_group_ctx)."""
        h = self.L.icl_group_ctx(self.g, i)
        n = self.L.icl_last_merges(h, None, 0)
        m = np.zeros((max(n, 1), 2), np.int32)
        self.L.icl_last_merges(h, m.ctypes.data, n)
        k = self.L.icl_last_merge_values(h, None, 0)
        v = np.zeros(max(k, 1), np.float32)
        self.L.icl_last_merge_values(h, v.ctypes.data, k)
        return m[:n], v[:k]

    def embed_cluster(self, imgs, min_size, max_size, prec=PREC_BF16, update=UPDATE_EXACT, want_E=True):
        """workflow.go:84-94 in one call: embed (2048-d pooled) on all GPUs, E assembled on the devices, clustered on GPU 0.
        -> (E or None, cluster_id, member_rank, n_clusters)"""
        imgs = np.ascontiguousarray(imgs, np.uint8).reshape(-1, IMG_BYTES)
        n = imgs.shape[0]
        E = np.empty((n, HEAD_POOLED), np.float32) if want_E else None
        cid = np.full(max(n, 1), -1, np.int32)
        rank = np.full(max(n, 1), -1, np.int32)
        nc = _i32()
        self._check(self.L.icl_group_embed_cluster(self.g, imgs.ctypes.data, n, prec, min_size, max_size, update,
                                                   E.ctypes.data if want_E else None, cid.ctypes.data, rank.ctypes.data, C.byref(nc)))
        return E, cid[:n], rank[:n], nc.value


def calc_optimal_clusters(total, min_size, max_size):
    k = _i64()
    rc = load().icl_calc_optimal_clusters(total, min_size, max_size, C.byref(k))
    return (k.value, None) if rc == ICL_OK else (0, rc)


def seeded_assign_ids(seed_size, min_size, merges):
    """icl_seeded_assign_ids (host only): seed sizes, minSize and a merge log (pairs of creation ids: seed i is i, merge t is m + t) ->
    (cluster_id[m], seed_rank[m], n_clusters) by the final-list rule of the seeded call."""
    ss = np.ascontiguousarray(seed_size, np.int32).reshape(-1)
    mg = np.ascontiguousarray(merges, np.int32).reshape(-1, 2)
    m = len(ss)
    cid, rank, nc = np.full(max(m, 1), -1, np.int32), np.full(max(m, 1), -1, np.int32), _i32()
    rc = load().icl_seeded_assign_ids(m, ss.ctypes.data if m else None, int(min_size), mg.ctypes.data if len(mg) else None, len(mg),
                                      cid.ctypes.data, rank.ctypes.data, C.byref(nc))
    if rc != ICL_OK:
        msg = load().icl_last_error(None)
        raise ICLError(rc, msg.decode() if msg else "")
    return cid[:m], rank[:m], nc.value


def decode_image_file(path):
    """IMRead (embeddings.go:50) for baseline or progressive JPEG / PNG / binary PPM -> h x w x 3 u8 RGB."""
    L = load()
    w, h = _i32(), _i32()
    rc = L.icl_decode_image_file(os.fsencode(path), None, 0, C.byref(w), C.byref(h))
    if rc:
        raise ICLError(rc, (L.icl_last_error(None) or b"").decode())
    out = np.empty((h.value, w.value, 3), np.uint8)
    rc = L.icl_decode_image_file(os.fsencode(path), out.ctypes.data, out.nbytes, C.byref(w), C.byref(h))
    if rc:
        raise ICLError(rc, (L.icl_last_error(None) or b"").decode())
    return out


def onnx_to_blob(path):
    """The ONNX reader's conversion alone (host only): file -> ICLW blob as a uint8 array."""
    L = load()
    n = _i64()
    rc = L.icl_onnx_to_blob_file(os.fsencode(path), None, 0, C.byref(n))
    if rc:
        raise ICLError(rc, (L.icl_last_error(None) or b"").decode())
    out = np.empty(n.value, np.uint8)
    rc = L.icl_onnx_to_blob_file(os.fsencode(path), out.ctypes.data, out.nbytes, C.byref(n))
    if rc:
        raise ICLError(rc, (L.icl_last_error(None) or b"").decode())
    return out


def decode_image_mem(data):
    """icl_decode_image_mem: decode_image_file for an image held in memory -> h x w x 3 u8 RGB."""
    L = load()
    p, n, keep = _byte_view(data)
    w, h = _i32(), _i32()
    rc = L.icl_decode_image_mem(_vp(p), n, None, 0, C.byref(w), C.byref(h))
    if rc:
        raise ICLError(rc, (L.icl_last_error(None) or b"").decode())
    out = np.empty((h.value, w.value, 3), np.uint8)
    rc = L.icl_decode_image_mem(_vp(p), n, out.ctypes.data, out.nbytes, C.byref(w), C.byref(h))
    del keep
    if rc:
        raise ICLError(rc, (L.icl_last_error(None) or b"").decode())
    return out


def jpeg_encode(rgb, quality=95):
    """icl_jpeg_encode_rgb (no GPU): h x w x 3 u8 RGB -> the bytes of the JPEG file libjpeg's defaults write at this quality."""
    L = load()
    a = np.ascontiguousarray(rgb, np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("jpeg_encode wants an h x w x 3 array")
    h, w = a.shape[:2]
    n = _i64()
    rc = L.icl_jpeg_encode_rgb(a.ctypes.data, w, h, quality, None, 0, C.byref(n))
    if rc:
        raise ICLError(rc, (L.icl_last_error(None) or b"").decode())
    out = np.empty(n.value, np.uint8)
    rc = L.icl_jpeg_encode_rgb(a.ctypes.data, w, h, quality, out.ctypes.data, out.nbytes, C.byref(n))
    if rc:
        raise ICLError(rc, (L.icl_last_error(None) or b"").decode())
    return out.tobytes()


def jpeg_encode_bound(w, h):
    return int(load().icl_jpeg_encode_bound(w, h))


def _downsize_one(call, want_info, guess):
    """One call into a buffer of the input's size (a downsized image is rarely larger than its source); a second only if it was too small."""
    L = load()
    n = _i64()
    info = np.zeros(6, np.int32)
    out = np.empty(max(1, guess), np.uint8)
    rc = call(out.ctypes.data, out.nbytes, C.byref(n), info.ctypes.data)
    if rc == ICL_ERR_ARG and n.value > out.nbytes:
        out = np.empty(n.value, np.uint8)
        rc = call(out.ctypes.data, out.nbytes, C.byref(n), info.ctypes.data)
    if rc:
        raise ICLError(rc, (L.icl_last_error(None) or b"").decode())
    data = out[:n.value].tobytes()
    if not want_info:
        return data
    keys = ["passthrough", "width", "height", "new_width", "new_height", "attempts"]
    return data, {k: int(v) for k, v in zip(keys, info)}


def downsize_image(path, max_bytes=MAX_IMAGE_SIZE, max_dim=MAX_IMAGE_DIM, want_info=False):
    """icl_downsize_image_file (no GPU): resizeImageIfNeeded (rekognition.go:173-259) with its limits as arguments -> bytes."""
    L = load()
    guess = os.path.getsize(path) if os.path.exists(path) else 0
    return _downsize_one(lambda o, c, n, i: L.icl_downsize_image_file(os.fsencode(path), max_bytes, max_dim, o, c, n, i), want_info, guess)


def downsize_image_mem(data, max_bytes=MAX_IMAGE_SIZE, max_dim=MAX_IMAGE_DIM, want_info=False):
    """icl_downsize_image_mem: downsize_image for an image held in memory."""
    L = load()
    p, nb, keep = _byte_view(data)
    r = _downsize_one(lambda o, c, n, i: L.icl_downsize_image_mem(_vp(p), nb, max_bytes, max_dim, o, c, n, i), want_info, nb)
    del keep
    return r


def load_image_224_mem(data):
    """icl_load_image_224_mem: load_image_224 for an image held in memory."""
    p, n, keep = _byte_view(data)
    out = np.empty((224, 224, 3), np.uint8)
    rc = load().icl_load_image_224_mem(_vp(p), n, out.ctypes.data)
    del keep
    if rc:
        raise ICLError(rc, (load().icl_last_error(None) or b"").decode())
    return out


def preprocess_mem(data):
    """icl_preprocess_mem: preprocess_file for an image held in memory -> (1, 3, 224, 224) fp32 NCHW."""
    p, n, keep = _byte_view(data)
    out = np.empty((1, 3, 224, 224), np.float32)
    rc = load().icl_preprocess_mem(_vp(p), n, out.ctypes.data)
    del keep
    if rc:
        raise ICLError(rc, (load().icl_last_error(None) or b"").decode())
    return out


def preprocess_file(path):
    """PreprocessImage(imagePath) (embeddings.go:46-116) -> (1, 3, 224, 224) fp32 NCHW."""
    out = np.empty((1, 3, 224, 224), np.float32)
    rc = load().icl_preprocess_file(os.fsencode(path), out.ctypes.data)
    if rc:
        raise ICLError(rc, (load().icl_last_error(None) or b"").decode())
    return out


def resize_u8(img, dw, dh):
    """cv::resize(img, (dw, dh), INTER_LINEAR) on an h x w x 3 u8 image (embeddings.go:69)."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    out = np.empty((dh, dw, 3), np.uint8)
    rc = load().icl_resize_u8(img.ctypes.data, w, h, out.ctypes.data, dw, dh)
    if rc:
        raise ICLError(rc, "icl_resize_u8")
    return out


def jpeg_coefs_file_host(path, sub_bits=0):
    """icl_jpeg_coefs_file_host (no GPU): the quantised coefficients of a JPEG by host stage A (sub_bits == 0) or by stage A0 and the GPU
    entropy decoder's schedule run as a host loop over subsequences of sub_bits bits -> (int16 array, info dict); info["state"]: 1 =
    decoded / accepted, 0 = rejected, -1 = does not qualify."""
    L = load()
    need = _i64()
    info = np.zeros(8, np.int32)
    rc = L.icl_jpeg_coefs_file_host(os.fsencode(path), sub_bits, None, 0, C.byref(need), info.ctypes.data)
    check(None, rc)
    out = np.zeros(max(1, need.value), np.int16)
    check(None, L.icl_jpeg_coefs_file_host(os.fsencode(path), sub_bits, out.ctypes.data, out.size, C.byref(need), info.ctypes.data))
    keys = ["state", "ncomp", "blocks0", "blocks1", "blocks2", "rounds", "nsub", "nintervals"]
    return out[:need.value], dict(zip(keys, (int(v) for v in info)))


PNG_INFO_KEYS = ["state", "w", "h", "depth", "ctype", "stored", "fixed", "dynamic", "max_code_len", "max_dist", "overlaps", "ring_wraps"]


def png_raw_file_host(path, stage=0):
    """icl_png_raw_file_host (no GPU): the GPU PNG route's schedule run as a host loop -> (uint8 array, info dict).  stage 0: the inflated
    stream, 1: the unfiltered scanlines (filter bytes kept), 2: RGB by the sample-to-RGB rule.  info["state"]: 1 = accepted, 0 = rejected
    (no bytes), -1 = does not qualify (no bytes)."""
    L = load()
    need = _i64()
    info = np.zeros(12, np.int32)
    check(None, L.icl_png_raw_file_host(os.fsencode(path), stage, None, 0, C.byref(need), info.ctypes.data))
    out = np.zeros(max(1, need.value), np.uint8)
    check(None, L.icl_png_raw_file_host(os.fsencode(path), stage, out.ctypes.data, out.size, C.byref(need), info.ctypes.data))
    return out[:need.value], dict(zip(PNG_INFO_KEYS, (int(v) for v in info)))


def load_image_224(path):
    out = np.empty((224, 224, 3), np.uint8)
    rc = load().icl_load_image_224(os.fsencode(path), out.ctypes.data)
    if rc:
        raise ICLError(rc, (load().icl_last_error(None) or b"").decode())
    return out


def tap_shape(tap):
    """(H, W, C) of the tensor icl_embed_taps returns for a tap: 56 x 56 x 64 after the stem, then [3, 4, 6, 3] bottlenecks per stage."""
    if not 0 <= tap <= 16:
        raise ValueError("tap must be 0..16")
    if tap == 0:
        return (56, 56, 64)
    stage = sum(tap > e for e in (3, 7, 13))
    return (56 >> stage, 56 >> stage, 256 << stage)


def synth_images(seed, first, n, mode=SYNTH_NOISE):
    out = np.empty((n, 224, 224, 3), np.uint8)
    rc = load().icl_synth_images(seed, first, n, mode, out.ctypes.data)
    if rc:
        raise ICLError(rc, "icl_synth_images")
    return out


def synthetic_blob(seed=1):
    L = load()
    nb = L.icl_synthetic_blob_bytes()
    buf = np.empty(nb, np.uint8)
    rc = L.icl_synthetic_blob(seed, buf.ctypes.data, nb)
    if rc:
        raise ICLError(rc, "icl_synthetic_blob")
    return buf

"""ctypes binding of libbayesod_hip.so (include/bayesod.h).  cffi is not installed in the target
image; the ABI is plain C so a cffi ABI-mode binding is the same declarations."""
import ctypes as C
import os

import numpy as np

# (GPU_MAX_HW_QUEUES: a handle drives up to five HIP streams -- a training handle seven -- which the runtime multiplexes onto that many
# hardware queues (default 4).  Only the training step gains from 8 (docs/DESIGN_HISTORY.md A.1), and the variable changes queue
# multiplexing for every HIP user of the process: it is a default of the ENTRY POINTS that benefit -- run_training.py, bench.py,
# which records the effective value in its JSON line -- not of importing this package.)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libbayesod_hip.so")
# development aid (tests/tools/ab_lib.sh): same-box A/B of two BUILDS of the library -- the override must name an existing file
if os.environ.get("BOD_LIB_OVERRIDE"):
    LIB_PATH = os.path.abspath(os.environ["BOD_LIB_OVERRIDE"])

BOD_OK, BOD_ERR_INVALID_ARG, BOD_ERR_HIP, BOD_ERR_OOM, BOD_ERR_NOT_READY, BOD_ERR_NO_DEVICE = range(6)
BOD_PARTS_COVARIANCE, BOD_PARTS_CLASS = 1, 2      # bits of bod_config.covariance_parts
BOD_MERGE_BAYES, BOD_MERGE_CENTRE, BOD_MERGE_MIXTURE = 0, 1, 2      # bod_set_merge_method
MERGE_METHODS = {"bayes": BOD_MERGE_BAYES, "centre": BOD_MERGE_CENTRE, "mixture": BOD_MERGE_MIXTURE}
BOD_METHOD_BAYES_OD, BOD_METHOD_BLACK_BOX = 0, 1                   # bod_set_uncertainty_method
UNCERTAINTY_METHODS = {"bayes_od": BOD_METHOD_BAYES_OD, "black_box": BOD_METHOD_BLACK_BOX}
BOD_VIEW_IDENTITY, BOD_VIEW_HFLIP = 0, 1         # views of a statistics handle (bod_stat_forward_view / bod_stat_merge_view)


class BodBlackBoxOptions(C.Structure):
    """Mirror of ``bod_blackbox_options`` (include/bayesod.h)."""
    _fields_ = [("min_score", C.c_float), ("min_members", C.c_int32), ("affinity_threshold", C.c_float), ("reserved", C.c_int32)]


class BodAcquisitionOptions(C.Structure):
    """Mirror of ``bod_acquisition_options`` (include/bayesod.h)."""
    _fields_ = [("min_foreground", C.c_float), ("top_k", C.c_int32), ("reserved", C.c_int32 * 2)]


class BodConfig(C.Structure):
    _fields_ = [
        ("device", C.c_int32), ("image_h", C.c_int32), ("image_w", C.c_int32), ("batch", C.c_int32),
        ("mc_samples", C.c_int32), ("num_classes", C.c_int32), ("anchors_per_location", C.c_int32),
        ("min_level", C.c_int32), ("max_level", C.c_int32), ("dropout_rate", C.c_float),
        ("use_full_covar", C.c_int32), ("dirichlet_non_informative", C.c_int32),
        ("gaussian_isotropic", C.c_int32), ("isotropic_variance", C.c_float),
        ("ranking_method", C.c_int32), ("nms_max_output_size", C.c_int32),
        ("nms_iou_threshold", C.c_float), ("nms_soft_sigma", C.c_float), ("nms_variant", C.c_int32),
        ("num_categorical_draws", C.c_int32), ("has_covar_head", C.c_int32),
        ("kitti_scale_h", C.c_float), ("kitti_scale_w", C.c_float), ("precision", C.c_int32),
        ("mc_sample_base", C.c_int32),
        ("mc_ensemble_size", C.c_int32),
        ("training", C.c_int32),
        ("backbone_depth", C.c_int32),
        ("pipeline_overlap", C.c_int32),
        ("mc_statistics", C.c_int32),
        ("covariance_parts", C.c_int32),         # (the last reserved int of include/bayesod.h)
    ]


class BodAugment(C.Structure):
    """bod_augment: one frame's augmentation record (``engine.AUGMENT_DTYPE`` is the same layout as a NumPy dtype)."""
    _fields_ = [("flip", C.c_int32), ("scale", C.c_float), ("off_y", C.c_float), ("off_x", C.c_float),
                ("gain", C.c_float), ("bias", C.c_float)]


class BodLossOptions(C.Structure):
    """bod_loss_options: the energy score's sample count and the key of its normals."""
    _fields_ = [("energy_samples", C.c_int32), ("seed", C.c_uint64), ("first_image_id", C.c_uint32), ("reserved", C.c_int32 * 4)]


class BodJpegInfo(C.Structure):
    """struct bod_jpeg_info: what a JPEG file's header says."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("components", C.c_int32), ("h_samp", C.c_int32), ("v_samp", C.c_int32),
                ("restart_interval", C.c_int32), ("supported", C.c_int32), ("coef_count", C.c_int64)]


class BodPngInfo(C.Structure):
    """struct bod_png_info: what a PNG file's header says."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("bit_depth", C.c_int32), ("color_type", C.c_int32), ("channels", C.c_int32),
                ("interlace", C.c_int32), ("supported", C.c_int32), ("raw_bytes", C.c_int64)]


class BodCorruptOp(C.Structure):
    """bod_corrupt_op: one op of a frame's corruption chain (``corruptions.OP_DTYPE`` is the same layout as a NumPy dtype)."""
    _fields_ = [("kind", C.c_int32), ("f0", C.c_float), ("u0", C.c_uint32), ("tap_offset", C.c_int32), ("ksize", C.c_int32),
                ("table", C.c_int32), ("reserved", C.c_int32 * 2)]


class BodRenderOptions(C.Structure):
    """bod_render_options: view, line width, labels and contour radius of bod_render_frames_u8."""
    _fields_ = [("view", C.c_int32), ("line_width", C.c_int32), ("labels", C.c_int32), ("r2", C.c_float), ("reserved", C.c_int32 * 4)]


BOD_RENDER_OVERLAY, BOD_RENDER_HEAT = 0, 1


class BodFoldLayer(C.Structure):
    """bod_fold_layer: one layer of bod_stage_fold_pack (inputs, geometry, host output arrays)."""
    _fields_ = [("kernel", C.POINTER(C.c_float)), ("bias", C.POINTER(C.c_float)), ("gamma", C.POINTER(C.c_float)),
                ("beta", C.POINTER(C.c_float)), ("mean", C.POINTER(C.c_float)), ("var", C.POINTER(C.c_float)),
                ("taps", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32), ("cout_pad", C.c_int32),
                ("w_fwd", C.POINTER(C.c_uint16)), ("w_bwd", C.POINTER(C.c_uint16)), ("w_flip", C.POINTER(C.c_uint16)),
                ("w_fwd32", C.POINTER(C.c_float)), ("b_fwd", C.POINTER(C.c_float))]


BOD_DGRAD_FLIP, BOD_DGRAD_ROWS, BOD_DGRAD_COL2IM = 0, 1, 2       # routes of bod_stage_conv_dgrad

# forms of bod_stage_stem
(BOD_STEM_AUTO, BOD_STEM_F32_POOL_F32, BOD_STEM_F32_POOL_SPLIT, BOD_STEM_SEG64_POOL, BOD_STEM_ROW_POOL, BOD_STEM_FUSED_8,
 BOD_STEM_FUSED_4, BOD_STEM_FUSED_SPLIT) = range(8)

BOD_LOSS_ONE_IMAGE_ID = 1                          # flag in bod_loss_options.reserved[0]


def loss_options(energy_samples=64, seed=0, first_image_id=0, one_image_id=False):
    flags = (C.c_int32 * 4)(BOD_LOSS_ONE_IMAGE_ID if one_image_id else 0, 0, 0, 0)
    return BodLossOptions(int(energy_samples), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_image_id) & 0xFFFFFFFF, flags)


class BodSizes(C.Structure):
    _fields_ = [
        ("num_pixels", C.c_int32), ("num_anchors", C.c_int32), ("level_h", C.c_int32 * 8),
        ("level_w", C.c_int32 * 8), ("num_levels", C.c_int32), ("max_detections", C.c_int32),
        ("device_bytes", C.c_int64),
    ]


_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)
_D = C.POINTER(C.c_double)
_H = C.c_void_p

# name -> (restype, argtypes); must list every symbol include/bayesod.h declares
SIGNATURES = {
    "bod_version": (C.c_char_p, []),
    "bod_last_error": (C.c_char_p, [_H]),
    "bod_create": (C.c_int, [C.POINTER(BodConfig), C.POINTER(_H)]),
    "bod_destroy": (C.c_int, [_H]),
    "bod_query_sizes": (C.c_int, [_H, C.POINTER(BodSizes)]),
    "bod_update_config": (C.c_int, [_H, C.POINTER(BodConfig)]),
    "bod_load_weight": (C.c_int, [_H, C.c_char_p, C.c_int32, C.POINTER(C.c_int64), C.c_int32, _F]),
    "bod_finalize_weights": (C.c_int, [_H]),
    "bod_set_anchors": (C.c_int, [_H, _F, C.c_int32]),
    "bod_forward": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_uint64, C.c_uint32]),
    "bod_get_raw": (C.c_int, [_H, _F, _F, _F]),
    "bod_set_raw": (C.c_int, [_H, _F, _F, _F]),
    "bod_get_pyramid": (C.c_int, [_H, C.c_int32, _F]),
    "bod_posterior": (C.c_int, [_H, C.c_uint64, C.c_uint32]),
    "bod_validation_post": (C.c_int, [_H]),
    "bod_get_num_kept": (C.c_int, [_H, _I]),
    "bod_get_posterior": (C.c_int, [_H, C.c_int32, _F, _F, _F, _F, _F, _I]),
    "bod_set_posterior": (C.c_int, [_H, C.c_int32, C.c_int32, _F, _F, _F, _F]),
    "bod_nms": (C.c_int, [_H]),
    "bod_get_nms": (C.c_int, [_H, C.c_int32, _I, _I]),
    "bod_set_nms": (C.c_int, [_H, C.c_int32, _I, C.c_int32]),
    "bod_get_iou_matrix": (C.c_int, [_H, C.c_int32, _F]),
    "bod_cluster_fuse": (C.c_int, [_H]),
    "bod_set_affinity": (C.c_int, [_H, C.c_int32, _F, C.c_int32, C.c_int32]),
    "bod_get_detections": (C.c_int, [_H, C.c_int32, _I, _F, _F, _F, _F]),
    "bod_get_detections_batch": (C.c_int, [_H, _I, _F, _F, _F, _F]),
    "bod_device_detections": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_void_p)]),
    "bod_device_raw": (C.c_int, [_H, C.POINTER(C.c_void_p), C.c_int32]),
    "bod_infer": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_uint64, C.c_uint32]),
    "bod_infer_async": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_uint64, C.c_uint32, _I]),
    "bod_collect": (C.c_int, [_H, C.c_int32, _I, _F, _F, _F, _F]),
    "bod_upload_images": (C.c_int, [_H, _F]),
    "bod_upload_frames_u8": (C.c_int, [_H, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, _F, C.c_int32]),
    "bod_upload_frames_u8_async": (C.c_int, [_H, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, _F, C.c_int32, C.c_int32]),
    "bod_upload_frames_u8_ragged": (C.c_int, [_H, C.POINTER(C.c_uint8), _I, _F, C.c_int32]),
    "bod_upload_frames_u8_ragged_async": (C.c_int, [_H, C.POINTER(C.c_uint8), _I, _F, C.c_int32, C.c_int32]),
    "bod_upload_frames_u8_augmented": (C.c_int, [_H, C.POINTER(C.c_uint8), _I, _F, C.c_int32, C.POINTER(BodAugment)]),
    "bod_upload_frames_u8_augmented_async": (C.c_int, [_H, C.POINTER(C.c_uint8), _I, _F, C.c_int32, C.POINTER(BodAugment), C.c_int32]),
    "bod_augment_boxes": (C.c_int, [C.c_int32, _I, C.c_int32, C.c_int32, C.c_int32, C.POINTER(BodAugment), _I, _F, _F, C.c_int32,
                                    C.c_float, _I, _F, _F]),
    "bod_jpeg_info": (C.c_int, [C.c_char_p, C.c_int64, C.POINTER(BodJpegInfo)]),
    "bod_jpeg_entropy_decode": (C.c_int, [C.c_char_p, C.c_int64, C.POINTER(C.c_int16), C.c_int64, C.POINTER(C.c_uint16)]),
    "bod_jpeg_decode_rgb": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_int32,
                                      C.POINTER(C.c_uint8), C.c_int64, _I]),
    "bod_upload_frames_jpeg": (C.c_int, [_H, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), _F, C.c_int32, C.POINTER(BodAugment),
                                         C.c_int32, _I]),
    "bod_upload_frames_jpeg_async": (C.c_int, [_H, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), _F, C.c_int32, C.POINTER(BodAugment),
                                               C.c_int32, _I, C.c_int32]),
    "bod_corrupt_frames_u8": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_uint8), _I, C.POINTER(BodCorruptOp), C.c_int32,
                                        C.POINTER(C.c_uint32), C.POINTER(C.c_uint16), C.c_int32, C.POINTER(C.c_uint8), C.c_int32,
                                        C.POINTER(C.c_uint16), C.c_int32, C.c_uint64, C.POINTER(C.c_uint8)]),
    "bod_set_upload_corruption": (C.c_int, [_H, C.POINTER(BodCorruptOp), C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint16),
                                            C.c_int32, C.POINTER(C.c_uint8), C.c_int32, C.POINTER(C.c_uint16), C.c_int32, C.c_uint64]),
    "bod_render_frames_u8": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_uint8), _I, _I, _I, _F, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8),
                                       _I, _I, C.POINTER(BodRenderOptions), C.POINTER(C.c_uint8), _I]),
    "bod_render_font": (C.c_int, [C.POINTER(C.c_uint8), _I]),
    "bod_png_info": (C.c_int, [C.c_char_p, C.c_int64, C.POINTER(BodPngInfo)]),
    "bod_png_inflate": (C.c_int, [C.c_char_p, C.c_int64, C.POINTER(C.c_uint8), C.c_int64]),
    "bod_png_decode_rgb": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_int32,
                                     C.POINTER(C.c_uint8), C.c_int64, _I]),
    "bod_bench_png_decode": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_int32, C.c_int32,
                                       C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "bod_upload_frames_png": (C.c_int, [_H, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), _F, C.c_int32, C.POINTER(BodAugment),
                                        C.c_int32, _I]),
    "bod_upload_frames_png_async": (C.c_int, [_H, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), _F, C.c_int32, C.POINTER(BodAugment),
                                              C.c_int32, _I, C.c_int32]),
    "bod_device_images_buffer": (C.c_void_p, [_H, C.c_int32]),
    "bod_device_images": (C.c_void_p, [_H]),
    "bod_synchronize": (C.c_int, [_H]),
    "bod_stage_conv_wgrad": (C.c_int, [C.c_int32, _F, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F, C.c_int32, C.c_int32,
                                       C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F, _F]),
    "bod_stage_act_backward": (C.c_int, [C.c_int32, C.c_int32, _F, _F, _F, C.c_int64, _I, _I, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_float, C.c_int32, _F, C.c_int64, _F, _F, _F, _I]),
    "bod_stage_conv_dgrad": (C.c_int, [C.c_int32, C.c_int32, _F, _F, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F, _I]),
    "bod_stage_stem_pool_backward": (C.c_int, [C.c_int32, C.c_int32, _F, _F, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _F]),
    "bod_stage_stem": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _F, C.c_int32, C.c_int32, C.c_int32, _F, _F, C.c_int32, C.c_int32,
                                 C.c_float, _F, _F, _I]),
    "bod_stage_stem_pool": (C.c_int, [C.c_int32, C.c_int32, _F, C.c_int32, C.c_int32, C.c_int32, C.c_float, _F]),
    "bod_stage_fold_pack": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(BodFoldLayer)]),
    "bod_stage_conv": (C.c_int, [C.c_int32, _F, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F, _F,
                                 C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F,
                                 C.c_float, C.c_uint64, C.c_int32, C.c_uint32, C.c_int32, C.c_int32, _F]),
    "bod_loss_forward": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F, _F, _F, _F, _F, _F,
                                   C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_float,
                                   C.POINTER(C.c_double)]),
    "bod_loss_forward_ex": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F, _F, _F, _F, _F, _F,
                                      C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_float,
                                      C.POINTER(C.c_double), C.POINTER(BodLossOptions)]),
    "bod_set_loss_options": (C.c_int, [_H, C.POINTER(BodLossOptions)]),
    "bod_train_step": (C.c_int, [_H, C.c_void_p, C.c_int32, _F, _F, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_uint64, C.c_uint32,
                                 C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32, C.POINTER(C.c_double)]),
    "bod_train_step_boxes": (C.c_int, [_H, C.c_void_p, C.c_int32, _I, _F, _F, C.c_float, C.c_float, C.c_uint64, C.c_uint32,
                                       C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32, C.POINTER(C.c_double)]),
    "bod_train_get_targets": (C.c_int, [_H, _F, _F, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]),
    "bod_train_gradients": (C.c_int, [_H, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "bod_train_apply": (C.c_int, [_H, C.c_float, C.POINTER(C.c_double)]),
    "bod_train_get": (C.c_int, [_H, C.c_char_p, C.c_int32, C.c_int32, _F, C.c_int64]),
    "bod_train_set": (C.c_int, [_H, C.c_char_p, C.c_int32, C.c_int32, _F, C.c_int64]),
    "bod_train_step_count": (C.c_int, [_H, C.POINTER(C.c_int64), C.c_int64]),
    "bod_loss_backward": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F, _F, _F, _F, _F, _F,
                                    C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_float,
                                    C.c_float, C.c_float, C.POINTER(C.c_double), _F, _F, _F]),
    "bod_loss_backward_ex": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F, _F, _F, _F, _F, _F,
                                       C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_float,
                                       C.c_float, C.c_float, C.POINTER(C.c_double), _F, _F, _F, C.POINTER(BodLossOptions)]),
    "bod_anchor_targets": (C.c_int, [C.c_int32, C.c_int32, _F, C.c_int32, _I, _F, _F, C.c_int32, C.c_float, C.c_float, _F, _F,
                                     C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), _I, _F]),
    "bod_validation_losses_boxes": (C.c_int, [_H, _I, _F, _F, C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_float, _D]),
    "bod_get_validation_detections_batch": (C.c_int, [_H, _I, _F, _F]),
    "bod_validate_boxes": (C.c_int, [_H, C.c_void_p, C.c_int32, _I, _F, _F, C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_float, _D,
                                     _I, _F, _F]),
    "bod_pdq_corner_heatmaps": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _D, _D, _I, _F]),
    "bod_pdq_frames": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _I, _I, _I, _I, _D, _D, _D, _D, _F]),
    "bod_score_pairs": (C.c_int, [C.c_int32, C.c_int64, _D, _D, _D, C.c_int32, C.c_uint64, C.c_uint64, _D, _I]),
    "bod_bench_head_conv": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "bod_profile_begin": (C.c_int, [_H]),
    "bod_profile_select": (C.c_int, [_H, C.c_int32]),
    "bod_plan_info": (C.c_int, [_H, C.POINTER(C.c_int32)]),
    "bod_plan_info_n": (C.c_int, [_H, C.POINTER(C.c_int32), C.c_int32]),
    "bod_stat_reset": (C.c_int, [_H]),
    "bod_stat_forward": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_uint64, C.c_uint32, C.c_int32]),
    "bod_stat_merge_from": (C.c_int, [_H, _H]),
    "bod_stat_merge": (C.c_int, [_H, C.POINTER(C.c_void_p), C.c_int32]),
    "bod_stat_device": (C.c_int, [_H, C.POINTER(C.c_void_p), _I]),
    "bod_stat_get": (C.c_int, [_H, _F, _F, _F, _I]),
    "bod_stat_set": (C.c_int, [_H, _F, _F, _F, C.c_int32]),
    "bod_stat_posterior": (C.c_int, [_H, C.c_uint64, C.c_uint32]),
    "bod_stat_forward_view": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_uint64, C.c_uint32, C.c_int32, C.c_int32]),
    "bod_stat_merge_view": (C.c_int, [_H, C.POINTER(C.c_void_p), C.c_int32, C.c_int32]),
    "bod_record_width": (C.c_int32, [_H]),
    "bod_get_posterior_parts": (C.c_int, [_H, C.c_int32, _F]),
    "bod_set_posterior_parts": (C.c_int, [_H, C.c_int32, C.c_int32, _F]),
    "bod_get_detection_parts": (C.c_int, [_H, C.c_int32, _F]),
    "bod_get_detection_parts_batch": (C.c_int, [_H, _F]),
    "bod_collect_parts": (C.c_int, [_H, C.c_int32, _F]),
    "bod_device_detection_parts": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_void_p)]),
    "bod_get_posterior_class_parts": (C.c_int, [_H, C.c_int32, _F]),
    "bod_get_posterior_mean_probs": (C.c_int, [_H, C.c_int32, _F]),
    "bod_set_posterior_class_parts": (C.c_int, [_H, C.c_int32, C.c_int32, _F, _F]),
    "bod_get_detection_class_parts": (C.c_int, [_H, C.c_int32, _F]),
    "bod_get_detection_class_parts_batch": (C.c_int, [_H, _F]),
    "bod_collect_class_parts": (C.c_int, [_H, C.c_int32, _F]),
    "bod_device_detection_class_parts": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_void_p)]),
    "bod_set_merge_method": (C.c_int, [_H, C.c_int32]),
    "bod_get_merge_method": (C.c_int, [_H, _I]),
    "bod_get_detection_merge_terms": (C.c_int, [_H, C.c_int32, _F, _F, _I]),
    "bod_get_detection_merge_terms_batch": (C.c_int, [_H, C.c_int32, _F, _F, _I]),
    "bod_device_detection_merge_terms": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_void_p)]),
    "bod_set_uncertainty_method": (C.c_int, [_H, C.c_int32, C.POINTER(BodBlackBoxOptions)]),
    "bod_get_uncertainty_method": (C.c_int, [_H, _I]),
    "bod_blackbox_samples": (C.c_int, [_H]),
    "bod_blackbox_merge": (C.c_int, [_H]),
    "bod_get_sample_detections": (C.c_int, [_H, C.c_int32, C.c_int32, _I, _I, _F, _F, _F]),
    "bod_set_sample_detections": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, _I, _F, _F, _F]),
    "bod_stat_get_entropy": (C.c_int, [_H, _F]),
    "bod_stat_set_entropy": (C.c_int, [_H, _F]),
    "bod_stat_device_entropy": (C.c_int, [_H, C.POINTER(C.c_void_p)]),
    "bod_stat_merge_entropy": (C.c_int, [_H, C.c_void_p, C.c_int32]),
    "bod_stat_acquisition": (C.c_int, [_H, C.POINTER(BodAcquisitionOptions), _D, _D]),
    "bod_stat_acquisition_map": (C.c_int, [_H, _F]),
    "bod_gather_detections": (C.c_int, [_H, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "bod_profile_end": (C.c_int, [_H, C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                  C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
}

_lib = None


def load():
    """Loads the shared library; raises RuntimeError (never falls back) if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libbayesod_hip.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (there is no CPU fallback)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError => header / library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def fptr(a):
    return None if a is None else a.ctypes.data_as(_F)


def dptr(a):
    return None if a is None else a.ctypes.data_as(_D)


def iptr(a):
    return None if a is None else a.ctypes.data_as(_I)


def check(lib, handle, status):
    if status == BOD_OK:
        return
    msg = lib.bod_last_error(handle)
    msg = msg.decode() if msg else "status %d" % status
    if status in (BOD_ERR_INVALID_ARG, BOD_ERR_NOT_READY):
        raise ValueError(msg)
    if status == BOD_ERR_OOM:
        raise MemoryError(msg)
    raise RuntimeError(msg)


def as_f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)

/*
 * bayesod.h -- C ABI of libbayesod_hip.so, the MI355X (gfx950) BayesOD inference hot path.
 *
 * The reference (asharakeh/bayes-od-rc) is pure Python/TensorFlow and has no FFI or plugin
 * interface; its boundary for this path is the Python call surface.
 * Each entry point below names the reference interface it stands behind (paths relative to
 * the reference root).  Plain pointers and sizes only; no torch / HIP types.  All host
 * buffers are caller-owned; the library owns every device allocation.  A handle is not
 * thread-safe: one handle per GPU / host thread.  Every call returns BOD_OK or an error code;
 * bod_last_error() gives the message.  Empty results (M = 0 / K = 0) are not errors
 * (src/retina_net/experiments/run_inference.py:147-161).
 */
#ifndef BAYESOD_H
#define BAYESOD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bod_context* bod_handle;

typedef enum {
    BOD_OK = 0,
    BOD_ERR_INVALID_ARG = 1,   /* maps to ValueError in the Python mirror            */
    BOD_ERR_HIP = 2,           /* HIP runtime failure (message holds hipGetErrorString) */
    BOD_ERR_OOM = 3,
    BOD_ERR_NOT_READY = 4,     /* weights / anchors not loaded, or stage order violated */
    BOD_ERR_NO_DEVICE = 5
} bod_status;

enum { BOD_RANK_SCORE = 0, BOD_RANK_JOINT_ENTROPY = 1 };
enum { BOD_NMS_VARIANT_A = 0, BOD_NMS_VARIANT_B = 1 };      /* SURVEY.md App. A.8 */
enum { BOD_HEAD_CLS = 0, BOD_HEAD_REG = 1, BOD_HEAD_COV = 2 };
enum { BOD_PRECISION_BF16 = 0, BOD_PRECISION_FP32 = 1, BOD_PRECISION_BF16X3 = 2, BOD_PRECISION_F16MX = 3, BOD_PRECISION_F16MX4 = 4 };

/* Mirrors model_config / testing_config of src/retina_net/configs/retinanet_bdd_covar.yaml
 * (:61-143) plus the geometry the reference derives at run time. */
typedef struct {
    int32_t device;              /* HIP device ordinal (--gpu_device, run_inference.py:267)           */
    int32_t image_h, image_w;    /* network input size                                                */
    int32_t batch;               /* images per call (reference: 1, run_inference.py:68)               */
    int32_t mc_samples;          /* model_config.mc_dropout_samples (yaml :66)                        */
    int32_t num_classes;         /* header.num_classes + 1 background (multitask_headers.py:86-88)    */
    int32_t anchors_per_location;/* len(scales)*len(aspect_ratios) (config_utils.py:81-86)            */
    int32_t min_level, max_level;/* anchor_generator.layers (yaml :53) -> 3..7                         */
    float   dropout_rate;        /* header.dropout_rate (yaml :82)                                    */
    int32_t use_full_covar;      /* testing_config.use_full_covar (yaml :125)                         */
    int32_t dirichlet_non_informative; /* bayes_od_config.dirichlet_prior.type == 'non_informative'   */
    int32_t gaussian_isotropic;  /* bayes_od_config.gaussian_prior.type == 'isotropic'                */
    float   isotropic_variance;  /* yaml :141                                                         */
    int32_t ranking_method;      /* BOD_RANK_*  (yaml :133)                                           */
    int32_t nms_max_output_size; /* nms_config.max_output_size (yaml :128)                            */
    float   nms_iou_threshold;   /* nms_config.iou_threshold, also the clustering affinity threshold
                                    (run_inference.py:148-149)                                        */
    float   nms_soft_sigma;      /* nms_config.soft_nms_sigma                                         */
    int32_t nms_variant;         /* BOD_NMS_VARIANT_*                                                 */
    int32_t num_categorical_draws; /* Categorical.sample(30) (inference_utils.py:42)                  */
    int32_t has_covar_head;      /* 'regression_covar' in output_names (retinanet_model.py:50)        */
    float   kitti_scale_h, kitti_scale_w; /* orig/net size; 0 => dataset != 'kitti'
                                    (inference_utils.py:147-167)                                      */
    int32_t precision;           /* BOD_PRECISION_BF16 (default, throughput path: bf16 storage + bf16 MFMA),
                                    BOD_PRECISION_FP32 (fp32 storage + exact-fp32 MFMA: the reference's fp32
                                    arithmetic end to end; ~1/10 of the speed) or BOD_PRECISION_BF16X3 (every value a
                                    (hi, lo) bf16 pair, products hi*hi + hi*lo + lo*hi on the bf16 MFMA with fp32
                                    accumulation: within 1e-3 of the float64 reference END TO END at about a third
                                    of the bf16 rate -- the parity mode of the throughput path) or
                                    BOD_PRECISION_F16MX (the parity mode with the head towers -- 80 % of its time --
                                    on one f16 product + half a block-scaled e2m3 product per multiplication instead of
                                    three bf16 products: x = f16 hi + lo, hi*hi exact, the two cross terms on the MX
                                    pipe; everything else as in BF16X3.  END TO END against the fp32 CPU forward with the same
                                    dropout masks: raw head outputs <= 2e-4 of |ref| + rms(ref); final detections, apart from
                                    at most one discrete flip per frame (a categorical draw at a CDF edge, a cluster member at
                                    the affinity threshold): box means <= 2e-5, scores <= 1e-7, covariance entries <= 1e-3 of
                                    |entry| + rms(matrix) -- bench.py's `meets_1e-3` states it per run) or
                                    BOD_PRECISION_F16MX4 (F16MX with the cross terms as block-scaled e2m1 (fp4) products of
                                    twice the channels: three quarters of the tower bytes and K-tiles, ~4x F16MX's
                                    rounding error: raw outputs 6e-4, boxes and scores inside 1e-3, fused covariance
                                    entries up to 4e-3 -- an opt-in mode BETWEEN bf16 and F16MX, not a parity mode)    */
    int32_t mc_sample_base;      /* index of this handle's first MC sample in the dropout RNG streams (default 0).
                                    A handle with mc_samples = n and base = r*n computes samples r*n .. r*n+n-1 of
                                    a larger ensemble bit-identically: the MC-sample-sharded multi-GPU mode
                                    (second mode).  May change on a live handle.        */
    int32_t mc_ensemble_size;    /* total MC samples of the ensemble this handle contributes to; 0 = mc_samples.
                                    MC dropout is on iff max(mc_ensemble_size, mc_samples) > 1
                                    (retinanet_model.py:74-77 decides on the ensemble size), so a rank holding a
                                    single sample of a sharded ensemble still applies its dropout masks.       */
    int32_t training;            /* 1: the handle also runs training steps (bod_train_step):
                                    every layer keeps its activation, dropout is on with mc_samples = 1
                                    (retinanet_model.py:113-147, training branch), fp32 master weights, gradients
                                    and Adam moments live on the device.  precision = BOD_PRECISION_BF16 (the product) or
                                    BOD_PRECISION_FP32 (the gradient-verification mode: same executor on fp32 tensors and
                                    the exact-fp32 MFMA kernel; meets float64 autograd element-wise).           */
    int32_t backbone_depth;      /* 0 / 50: ResNet-50, the reference's only backbone (feature_extractor.py:6-9).  101: stage 4 with
                                    1 ConvBlock + 22 IdentityBlocks (layer names res4a .. res4w) -- BASELINE config 5's
                                    "ResNet-101", which has no counterpart in the reference.             */
    int32_t pipeline_overlap;    /* 1: bod_infer_async overlaps the memory-bound front of batch i+1 (stem, backbone, FPN) with the
                                    MFMA-bound back of batch i (fan-out layer, towers, posterior) on two CU-partitioned streams
                                    (hipExtStreamCreateWithCUMask: the front owns the last 4 CU slots of every XCD, 32 of 256 CUs,
                                    the back the other 224; the pyramid is double-buffered).  EXPERIMENTAL: measured 8.5 % SLOWER
                                    than one stream (the chip is power-bound: DESIGN.md 8.3), and it runs kernels of the library
                                    beside each other by design, which until round 6 was not reproducible bit for bit (DESIGN.md
                                    8.4: packed fp32 results of a wave are corrupted in lanes 48-63 beside a wave that interleaves
                                    VALU work with MFMAs -- a gfx950 erratum; the library is built without packed fp32
                                    instructions since, and no difference has been seen after that).  bod_create refuses the
                                    mode unless BOD_OVERLAP_EXPERIMENTAL=1 is set in the environment.  Every other entry point
                                    keeps the whole chip.  Inference handles only.  0 (default): one stream: no kernel of the
                                    library runs beside another.                                                  */
    int32_t mc_statistics;       /* 1: a STATISTICS handle (inference only; training / pipeline_overlap are refused): the handle owns
                                    an accumulator of mergeable per-anchor MC statistics beside the ones of its last forward, and a
                                    sample count K -- the bod_stat_* entry points below.  Its aggregating plan, where the conditions
                                    for one hold (also with mc_ensemble_size > mc_samples), is the DENSE one: no keep stage, no
                                    sparse tail or halo, because the kept set depends on the merged class statistics and every
                                    anchor's box / covariance statistics must exist before the merge.  0 (default): plans, kernels,
                                    buffers and results exactly as without the field.                                    */
    union {                      /* the last reserved int under both names: the size and every offset are unchanged, and a caller
                                    that zeroes reserved[0] asks for the default                                        */
        int32_t covariance_parts; /* A bit set (BOD_PARTS_* below).  BOD_PARTS_COVARIANCE = 1: the handle also reports, for every
                                    posterior row and every detection, the three terms
                                    its covariance is the sum of -- epistemic, aleatoric, prior (the bod_*_parts entry points
                                    below).  Inference and statistics handles; refused with training = 1.  Two
                                    more launches per pass, 30 floats per anchor + 48 per detection slot of HBM; record rows
                                    widen by 48 floats.  BOD_PARTS_CLASS = 2: ... and the entropy of the MC class distribution
                                    split into aleatoric, epistemic (mutual information) and spatial parts (the
                                    bod_*_class_parts / bod_stat_*entropy entry points below): one more float
                                    per anchor from the classification head's epilogue, two more launches per pass, 4 + C
                                    floats per anchor + 4 per detection slot of HBM; record rows widen by 4 floats.  3: both.
                                    0 (default): plans, kernels, buffers and results exactly as without the field.          */
        int32_t reserved[1];
    };
} bod_config;
enum { BOD_PARTS_COVARIANCE = 1, BOD_PARTS_CLASS = 2 };      /* bits of bod_config.covariance_parts */

/* Sizes the caller needs to allocate host buffers. */
typedef struct {
    int32_t num_pixels;          /* P: sum over levels of h*w            */
    int32_t num_anchors;         /* A = P * anchors_per_location         */
    int32_t level_h[8], level_w[8];
    int32_t num_levels;
    int32_t max_detections;      /* nms_max_output_size                  */
    int64_t device_bytes;        /* total HBM the handle holds           */
} bod_sizes;

const char* bod_version(void);
const char* bod_last_error(bod_handle h);         /* h may be NULL: last create() failure */

/* RetinaNetModel(model_config)  (src/retina_net/models/retinanet_model.py:19-65) */
bod_status bod_create(const bod_config* cfg, bod_handle* out);
bod_status bod_destroy(bod_handle h);
bod_status bod_query_sizes(bod_handle h, bod_sizes* out);
/* Change the testing_config-derived fields (use_full_covar, priors, ranking, nms_*, kitti scale,
 * num_categorical_draws) of a live handle; geometry / batch / mc_samples / heads must be unchanged. */
bod_status bod_update_config(bod_handle h, const bod_config* cfg);

/* ckpt.restore(...) (run_inference.py:120): one call per Keras variable, fp32 host data.
 * kind: 0 conv kernel HWIO [kh,kw,cin,cout]; 1 conv bias [cout]; 2..5 BN gamma/beta/mean/var.
 * name: Keras layer name ('conv1', 'bn_conv1', 'res2a_branch2a', 'C5_reduced', 'P3',
 * 'pyramid_classification_0', 'pyramid_classification', 'pyramid_regression', 'pyramid_cov' ...;
 * feature_extractor.py:154-155,231-232; feature_decoder.py:28-132; multitask_headers.py:30-314). */
bod_status bod_load_weight(bod_handle h, const char* name, int32_t kind,
                           const int64_t* shape, int32_t ndim, const float* data);
/* Folds frozen BN (feature_extractor.py:108 ... training=False), packs bf16 OHWI, uploads. */
bod_status bod_finalize_weights(bod_handle h);

/* sample_dict['anchors'] (src/core/constants.py:50; bdd_dataset_handler.py:183-186): [A,4] (v,u,h,w) */
bod_status bod_set_anchors(bod_handle h, const float* anchors_vuhw, int32_t num_anchors);

/* model(image, train_val_test='testing')  (retinanet_model.py:67-112).
 * images: [batch,H,W,3] fp32 normalised BGR (sample_dict['image_normalized']), host pointer or,
 * if images_on_device != 0, a device pointer already resident in HBM.
 * seed / first_image_id key the Philox dropout + categorical streams (DESIGN.md RNG contract).
 * On a handle created with training = 1 this is model(image, train_val_test='training') (retinanet_model.py:113-147):
 * one sample with dropout ON, batch-norm frozen, the current (trained) master weights. */
bod_status bod_forward(bod_handle h, const float* images, int32_t images_on_device,
                       uint64_t seed, uint32_t first_image_id);
/* prediction_dict tensors (src/core/constants.py:61-63), copied to host:
 * cls [batch,N,A,C], box [batch,N,A,4], covar params [batch,N,A,10] (pre fill_triangular).
 * Any pointer may be NULL. */
bod_status bod_get_raw(bod_handle h, float* cls, float* box, float* covar_params);
/* Replace the head outputs with caller-supplied ones (stage-level parity tests). */
bod_status bod_set_raw(bod_handle h, const float* cls, const float* box, const float* covar_params);
/* Backbone / FPN taps for parity tests: which = 0..4 -> p3..p7 ([batch,h,w,256] fp32 out). */
bod_status bod_get_pyramid(bod_handle h, int32_t level_index, float* out);

/* bayes_od_inference after the model call (src/retina_net/experiments/inference_utils.py:25-202):
 * decode, softmax, mean over MC, categorical sampling, filter, per-anchor mean / 4x4 covariance,
 * aleatoric L D L^T, mixing, Dirichlet + Gaussian prior fusion, ranking; compacted in anchor order. */
bod_status bod_posterior(bod_handle h, uint64_t seed, uint32_t first_image_id);
/* validation_utils.post_process_predictions (:10-77), the deterministic validation path: softmax of MC sample 0
 * of the raw class outputs, anchors whose arg-max class is background dropped, candidates ranked by their top
 * score.  Fills the same compacted buffers as bod_posterior (score = counts = softmax row, means = decoded
 * box, covs = 0), so bod_nms / bod_get_posterior / bod_get_nms follow as usual. */
bod_status bod_validation_post(bod_handle h);
/* Per image results of bod_posterior. num_kept[batch]; the arrays are [M,...] for image_index.
 * counts/score [M,C], means [M,4], covs [M,16], ranking [M], anchor_index [M]. NULLs skipped. */
bod_status bod_get_num_kept(bod_handle h, int32_t* num_kept);
bod_status bod_get_posterior(bod_handle h, int32_t image_index, float* counts, float* score,
                             float* means, float* covs, float* ranking, int32_t* anchor_index);
/* Inject a posterior (stage-level parity of NMS / clustering): arrays as above, M rows. */
bod_status bod_set_posterior(bod_handle h, int32_t image_index, int32_t m, const float* counts,
                             const float* means, const float* covs, const float* ranking);

/* tf.image.non_max_suppression_with_scores on vuhw_to_vuvu(means) (inference_utils.py:204-212). */
bod_status bod_nms(bod_handle h);
bod_status bod_get_nms(bod_handle h, int32_t image_index, int32_t* indices, int32_t* num_selected);
/* Inject cluster centres (the `cluster_centers` argument of bayes_od_clustering, :289). */
bod_status bod_set_nms(bod_handle h, int32_t image_index, const int32_t* indices, int32_t num_selected);
/* box_utils.bbox_iou_vuvu(corners, corners) (inference_utils.py:214-215): [M,M] fp32 to host. */
bod_status bod_get_iou_matrix(bod_handle h, int32_t image_index, float* iou);

/* bayes_od_clustering (inference_utils.py:285-364) on the device, affinity = the IoU above,
 * threshold = nms_iou_threshold; covariances x70. */
bod_status bod_cluster_fuse(bod_handle h);
/* The `affinity_matrix` argument of bayes_od_clustering (inference_utils.py:290,316) when the caller's affinity is
 * not the IoU of the posterior means: centre_columns [k][m] holds, for each of the image's k cluster centres (in
 * bod_set_nms / bod_get_nms order), the column affinity_matrix[:, centre] over the image's m boxes.  The NEXT
 * bod_cluster_fuse tests `centre_columns[k][i] > nms_iou_threshold` for that image instead of evaluating the IoU on
 * the fly, then the columns are dropped (one-shot).  k and m must equal the image's centre and box counts. */
bod_status bod_set_affinity(bod_handle h, int32_t image_index, const float* centre_columns, int32_t k, int32_t m);
/* Final detections of one image: K <= max_detections rows.
 * scores [K,C], means [K,4] (v,u,h,w), covs [K,16], counts [K,C]. */
bod_status bod_get_detections(bod_handle h, int32_t image_index, int32_t* num_detections,
                              float* scores, float* means, float* covs, float* counts);

/* All images of the batch in one call (one device->host copy per array, one sync):
 * num_detections [batch]; scores/counts [batch,max_detections,C]; means [batch,max_detections,4];
 * covs [batch,max_detections,16]; rows >= num_detections[b] are unspecified. NULLs skipped. */
bod_status bod_get_detections_batch(bod_handle h, int32_t* num_detections, float* scores, float* means,
                                    float* covs, float* counts);
/* Device addresses of the same five arrays of record slot 0/1 (order: num, scores, means, covs,
 * counts) for zero-copy hand-off to a collective library (the RCCL gather of SURVEY.md section
 * 8e).  Valid until bod_destroy; contents are defined once the batch that filled the slot has
 * completed (bod_synchronize, or bod_collect with NULL destinations). Synchronous calls use slot 0
 * until the first bod_infer_async. */
bod_status bod_device_detections(bod_handle h, int32_t slot, void** ptrs5);
/* Device addresses of the raw head outputs of bod_forward (order: cls [B,N,A,C], box [B,N,A,4],
 * cov [B,N,A,10] or NULL), fp32 -- the tensors RetinaNetModel.call returns (retinanet_model.py:99-112) --
 * for zero-copy exchange between handles / GPUs (MC-sample sharding gathers every rank's [1,n,A,.] slices
 * into one handle's buffers).  mark_ready != 0 declares the buffers filled by the caller (like bod_set_raw),
 * so bod_posterior may run on them; the caller orders its writes before that call (bod_synchronize or
 * its own stream/event ordering). */
bod_status bod_device_raw(bod_handle h, void** ptrs3, int32_t mark_ready);

/* The whole per-image body of run_inference.test_model's loop (:137-149) for `batch` images:
 * forward -> posterior -> nms -> cluster_fuse, one stream, no host round trip. */
bod_status bod_infer(bod_handle h, const float* images, int32_t images_on_device,
                     uint64_t seed, uint32_t first_image_id);

/* Pipelined form for sustained throughput: enqueue the whole pass and return at once, so that the host
 * enqueues batch i+1 while batch i runs and its records travel to pinned memory.  (Until round 5 the
 * soft-NMS + cluster-fuse of a batch ran on a side stream underneath the next batch's convolutions; they
 * follow the posterior on the main stream now -- DESIGN.md 8.4.)  Detection records are double-buffered ("slots").  *slot receives the
 * ticket to pass to bod_collect, which waits for that batch and copies its padded records
 * (layout as bod_get_detections_batch).  At most two batches may be in flight. */
bod_status bod_infer_async(bod_handle h, const float* images, int32_t images_on_device,
                           uint64_t seed, uint32_t first_image_id, int32_t* slot);
bod_status bod_collect(bod_handle h, int32_t slot, int32_t* num_detections, float* scores,
                       float* means, float* covs, float* counts);

/* Device buffer of [batch,H,W,3] fp32 owned by the handle (fill with bod_upload_images, then
 * pass to bod_forward/bod_infer with images_on_device=1). */
bod_status bod_upload_images(bod_handle h, const float* host_images);
/* Same destination, filled from decoded uint8 RGB frames [batch, src_h, src_w, 3]: the dataset handlers'
 * preprocessing runs on the device -- float conversion, mean subtraction (rgb_means[3], constants.py:12),
 * RGB->BGR (bdd_dataset_handler.py:128-139) and, with aspect_resize != 0, KITTI's
 * tf.image.resize(BILINEAR, preserve_aspect_ratio=True) + resize_with_crop_or_pad to the network size
 * (kitti_dataset_handler.py:120-148).  A quarter of the PCIe bytes of bod_upload_images. */
bod_status bod_upload_frames_u8(bod_handle h, const uint8_t* rgb, int32_t src_h, int32_t src_w,
                                const float* rgb_means, int32_t aspect_resize);
/* Pipelined form of the same upload: the host->device copy of `rgb` (pinned host memory for a truly asynchronous copy)
 * and the device preprocessing run on the handle's COPY stream into image buffer 0 or 1 and return at once, so the PCIe
 * transfer of batch i+1 overlaps the convolutions of batch i (the reference gets the same overlap from tf.data's
 * prefetch, run_inference.py:71-72).  Pass bod_device_images_buffer(h, buffer) with images_on_device = 1 to bod_forward /
 * bod_infer / bod_infer_async: the forward waits for the upload, and the next upload into the same buffer waits until the
 * stem of that forward has consumed the frames.  `rgb` must stay valid until that forward has been enqueued AND the copy
 * has completed (bod_synchronize, or a later bod_collect of that batch).  Buffer 0 is bod_device_images(). */
bod_status bod_upload_frames_u8_async(bod_handle h, const uint8_t* rgb, int32_t src_h, int32_t src_w,
                                      const float* rgb_means, int32_t aspect_resize, int32_t buffer);
/* The same two uploads for a batch whose frames differ in source size (KITTI: 370x1224 .. 376x1241 interleaved through every
 * split).  `rgb_packed` holds the frames back to back -- frame b starts at byte 3 * sum of h_i * w_i over i < b -- and
 * src_hw[batch][2] their (h, w).  Every frame gets the resize / crop / pad geometry of its own size and comes out as
 * bod_upload_frames_u8 of that size gives it, bit for bit; rgb_means are shared by the batch.  With aspect_resize != 0 on a
 * handle whose kitti_scale_h > 0, frame b also gets its own rescale factors float(h_b / image_h), float(w_b / image_w): they
 * belong to the image buffer filled, and the forward that consumes that buffer applies them in its posterior
 * (inference_utils.py:147-167, S = orig / net per sample) in place of kitti_scale_h / kitti_scale_w.  A uniform upload,
 * bod_upload_images or host float images into that buffer bring the handle's two scalars back.  BOD_ERR_INVALID_ARG, naming
 * the frame, for a size below 1, a degenerate resize, or aspect_resize == 0 with a frame not at the network size; the
 * handle and the frames it held stay as they were.  Staging, streams and the lifetime of `rgb_packed` as for the uniform
 * pair (src_hw is read before the call returns). */
bod_status bod_upload_frames_u8_ragged(bod_handle h, const uint8_t* rgb_packed, const int32_t* src_hw,
                                       const float* rgb_means, int32_t aspect_resize);
bod_status bod_upload_frames_u8_ragged_async(bod_handle h, const uint8_t* rgb_packed, const int32_t* src_hw,
                                             const float* rgb_means, int32_t aspect_resize, int32_t buffer);
/* Training-time augmentation of the same upload: every frame of the packed batch is shown in a form of its own -- mirrored,
 * resized by `scale`, placed off-centre in the network frame, its brightness / contrast changed.  The default routes above do
 * not change; this one is opt-in (run_training --augment).
 * Geometry of frame b (the function the two other upload routes take their centred geometry from):
 *   aspect_resize != 0: the resize target is (max(1, floor(scale*image_h + 0.5)), max(1, floor(scale*image_w + 0.5))), in double,
 *     in place of (image_h, image_w); (rh, rw) is the aspect-preserving size for that target by the rule above.
 *   aspect_resize == 0: the frame must be at the network size; (rh, rw) = (max(1, floor(scale*h + 0.5)), max(1, floor(scale*w + 0.5)))
 *     and the frame is resized by the same bilinear when that differs from (h, w).
 *   per axis, d = rh - image_h:  d > 0: crop = floor(off*d), no pad;  d < 0: pad = floor(off*(-d)), no crop (off widened to double).
 *     off = 0.5 is the centred d / 2 of every other upload.
 * Then, per output pixel: flip mirrors the SOURCE frame (the result is bit for bit the upload of the mirrored frame with flip = 0);
 * inside the visible region v' = min(max(gain*v + bias, 0), 255) on the interpolated 0..255 value, two fp32 operations; padding
 * stays 0 (so -mean after normalisation).  flip 0, scale 1, off 0.5, gain 1, bias 0 is bod_upload_frames_u8_ragged bit for bit.
 * On a handle whose kitti_scale_h > 0 the handle's two scalars apply, as after a uniform upload (detections of an augmented frame
 * are not mapped back to its source).  BOD_ERR_INVALID_ARG, naming the frame, for flip outside {0, 1}, a scale that is not finite
 * and positive, an off outside [0, 1], a gain or bias that is not finite, and the ragged uploads' errors; the handle and the
 * frames it held stay as they were.  Packing, staging, streams and lifetimes as for the ragged pair (aug is read before return). */
typedef struct bod_augment {   /* one per frame */
    int32_t flip;              /* 0 or 1 */
    float   scale;             /* > 0, finite; 1 = none */
    float   off_y, off_x;      /* in [0,1]; 0.5 = centred, as every other upload */
    float   gain, bias;        /* finite; 1, 0 = none */
} bod_augment;
bod_status bod_upload_frames_u8_augmented(bod_handle h, const uint8_t* rgb_packed, const int32_t* src_hw,
                                          const float* rgb_means, int32_t aspect_resize, const bod_augment* aug);
bod_status bod_upload_frames_u8_augmented_async(bod_handle h, const uint8_t* rgb_packed, const int32_t* src_hw,
                                                const float* rgb_means, int32_t aspect_resize, const bod_augment* aug,
                                                int32_t buffer);
/* Ground truth of B augmented frames, mapped through the same geometry: pure host code, no handle and no device.  gt_boxes_vuvu_src
 * holds sum(num_gt) rows (y1, x1, y2, x2) in SOURCE pixels, frame after frame, gt_classes the matching [.., C] rows.  In fp32, in
 * this order: flip (x1' = (w-1) - x2, x2' = (w-1) - x1); multiply by float(rh / h), float(rw / w); add pad - crop; clip to
 * [0, net_h-1] x [0, net_w-1].  A box is dropped when its clipped area is below min_visible times its unclipped transformed area or
 * its clipped height or width is below 1.  A frame left without a box gets the dataset handlers' placeholder row [0, 0, 1, 1] with
 * the background class (the last of C), so num_out[b] >= 1.  Outputs: num_out[B]; boxes_out / classes_out sized for
 * sum(max(num_gt[b], 1)) rows, packed frame after frame.
 * NOTE: this map differs on purpose from the KITTI handler's box * (net / orig) ratio (kitti_dataset_handler.py:132-135), which
 * ignores the pad of the aspect-preserving resize; that ratio stays what the non-augmented route uses.
 * Errors are reported through bod_last_error(NULL). */
bod_status bod_augment_boxes(int32_t B, const int32_t* src_hw, int32_t net_h, int32_t net_w, int32_t aspect_resize,
                             const bod_augment* aug, const int32_t* num_gt, const float* gt_boxes_vuvu_src,
                             const float* gt_classes, int32_t C, float min_visible,
                             int32_t* num_out, float* boxes_out, float* classes_out);
/* Baseline JPEG frames decoded inside the library.  Marker parsing and Huffman decoding run on host threads; the
 * dequantisation, the 8x8 inverse DCT (libjpeg's "islow"), the "fancy" chroma upsampling and YCbCr -> RGB run on the device and
 * write the uint8 RGB frames into the staging buffer the ragged / augmented preprocess kernels read: the decoded frame never
 * exists on the host.  The frames equal PIL's Image.open(..).convert('RGB') (libjpeg-turbo) byte for byte.
 * Supported: 8-bit baseline (SOF0) streams with one interleaved scan, 1 component (grayscale) or 3 (YCbCr) with luma sampling
 * 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0) and chroma 1x1; restart intervals; any Huffman tables.  Progressive, arithmetic, lossless
 * and 12-bit streams, several scans, DNL, 16-bit quantisation tables, 4 components, other samplings and Adobe RGB are well-formed
 * but NOT supported: bod_jpeg_info reports them with supported = 0 and the reason in bod_last_error(NULL) (so does a file without
 * an SOI marker: a PNG), the other entry points refuse them with BOD_ERR_INVALID_ARG.  A corrupt or truncated stream is
 * BOD_ERR_INVALID_ARG everywhere.
 * (The struct has no typedef: in C a typedef would share the function's name space.) */
struct bod_jpeg_info {
    int32_t width, height, components;
    int32_t h_samp, v_samp;          /* luma sampling; chroma is 1x1 */
    int32_t restart_interval;
    int32_t supported;               /* 0: well-formed but outside the supported subset (the message says why) */
    int64_t coef_count;              /* int16 coefficients bod_jpeg_entropy_decode writes */
};
/* Header and entropy stage alone: host only, no handle, no device (as bod_augment_boxes); errors through bod_last_error(NULL).
 * bod_jpeg_entropy_decode writes, per component, the coefficient blocks of the MCU-padded plane in raster block order, 64 int16
 * per block in natural (row-major) order, and the components' quantisation tables in natural order into quant3x64[3][64]. */
bod_status bod_jpeg_info(const uint8_t* data, int64_t len, struct bod_jpeg_info* out);
bod_status bod_jpeg_entropy_decode(const uint8_t* data, int64_t len, int16_t* coefs, int64_t coef_capacity,
                                   uint16_t* quant3x64);
/* The decoder alone (stand-alone device entry, as bod_score_pairs): n files -> packed RGB on the host (frame b at byte 3 * sum of
 * h_i * w_i over i < b) + src_hw[n][2].  `threads` host threads decode the scans (capped at 16 and at n; <= 0 means 1). */
bod_status bod_jpeg_decode_rgb(int32_t device, int32_t n, const uint8_t* const* data, const int64_t* len,
                               int32_t threads, uint8_t* rgb_packed, int64_t rgb_capacity, int32_t* src_hw);
/* The upload routes: data[batch] / len[batch] are the files.  The scans are decoded on `threads` host threads into pinned staging
 * the handle owns (one per image buffer; the host waits for the previous copy out of it first), then the copy, the two JPEG
 * kernels and the ragged (aug == NULL) or augmented preprocess kernel run on the upload's stream.  Everything else -- geometry
 * errors, the per-frame KITTI factors, which image buffer is filled, the ordering against the forward that consumes it -- is
 * bod_upload_frames_u8_ragged[_async] / bod_upload_frames_u8_augmented[_async] of the decoded frames, bit for bit.  The host
 * decode finishes before the call returns: `data` is free on return, in the async form as well.  src_hw_out[batch][2] (may be
 * NULL) receives the frames' sizes.  A corrupt or unsupported frame gives BOD_ERR_INVALID_ARG naming the frame and the reason;
 * nothing is enqueued, the handle and the frames it held stay as they were. */
bod_status bod_upload_frames_jpeg(bod_handle h, const uint8_t* const* data, const int64_t* len,
                                  const float* rgb_means, int32_t aspect_resize, const bod_augment* aug,
                                  int32_t threads, int32_t* src_hw_out);
bod_status bod_upload_frames_jpeg_async(bod_handle h, const uint8_t* const* data, const int64_t* len,
                                        const float* rgb_means, int32_t aspect_resize, const bod_augment* aug,
                                        int32_t threads, int32_t* src_hw_out, int32_t buffer);
/* Corruptions of the packed uint8 RGB source frames on the device: dataset shift for scoring uncertainty.  A
 * frame's corruption is a chain of ops_per_frame (1..4) ops applied in order to its h*w*3 bytes; ops[n][ops_per_frame] holds one
 * chain per frame (pad a shorter chain with BOD_CORRUPT_NONE, which leaves the bytes alone).  Every op but GAUSSIAN_NOISE is
 * integer arithmetic, or fp32 with a fixed operation order (no contraction): its result is defined to the bit.
 *   LUT            v' = luts[table][c][v]                                     (luts: uint8 [n_luts][3][256])
 *   CONTRAST       m_c = (float)((double)(sum of channel c over the frame) / (double)(h*w));
 *                  v' = rintf(min(max((v - m_c) * f0 + m_c, 0), 255)), subtract, multiply and add as three fp32 operations
 *   IMPULSE_NOISE  words x, y, z of the pixel's Philox call serve R, G, B: word < u0 ? ((word & 1) ? 255 : 0) : v
 *                  (u0 = min(floor(p * 2^32), 2^32 - 1) for a probability p)
 *   GAUSSIAN_NOISE u(t) = ((t >> 9) + 0.5) * 2^-23;  n0, n1 = sqrtf(-2 logf(u(x))) * (cosf, sinf)(6.2831855f * u(y)), n2 the cosine
 *                  branch of (z, w);  v'_c = rintf(min(max(v_c + f0 * n_c, 0), 255)), multiply and add as two fp32 operations
 *   CONV2D         v'(y, x) = (sum over ky, kx of taps[tap_offset + ky*ksize + kx] * v(clamp(y + ky - r), clamp(x + kx - r)) + 2^14) >> 15,
 *                  r = ksize / 2, coordinates clamped to the frame; ksize odd, 1..25; the ksize^2 uint16 taps sum to exactly 2^15
 *   PIXELATE       every u0 x u0 block anchored at (0, 0), ragged at the right / bottom edge, becomes (sum + n/2) / n over its n
 *                  pixels, per channel, integer division
 *   JPEG           8x8-block-local baseline round trip at 4:4:4: libjpeg's jccolor forward colour, edge blocks replicating the
 *                  last column then the last row, samples - 128, jfdctint ("islow") forward DCT, quantisation
 *                  sign(x) * ((|x| + (8q >> 1)) / 8q) by qtables[table] (uint16 [n_qtables][2][64], luma then chroma, natural
 *                  order), then the decoder's dequantisation, inverse DCT, clamp and YCbCr -> RGB.  Equal to libjpeg(-turbo)'s
 *                  save-then-load bytes at subsampling 4:4:4.
 *   FOG            octaves s = 7..2, lattice spacing S = 2^s; the lattice value v(s, iy, ix) is the top 16 bits of word x of a
 *                  Philox call; fx = x & (S-1), fy = y & (S-1), b_s = (v00*(S-fx) + v01*fx)*(S-fy) + (v10*(S-fx) + v11*fx)*fy;
 *                  F = sum over s of (b_s >> 2s) >> (7 - s);  t = (u0 * F) >> 17;  v' = (v*(256 - t) + 255*t + 128) >> 8
 * Random numbers: philox4x32_10 with key (seed low, seed high) and counter
 *   (x, y, BOD_CORRUPT_TAG | slot, frame id)                    IMPULSE_NOISE, GAUSSIAN_NOISE: pixel (y, x)
 *   (ix, iy, BOD_CORRUPT_TAG | slot | s << 4, frame id)         FOG: lattice point (iy, ix) of octave s
 * with BOD_CORRUPT_TAG = 0x00C02200 and slot = the op's index 0..3 in its chain: a frame's result depends on its bytes, its
 * chain, its id and the seed alone -- not on its place in the batch, the batch's other frames or how frames are split over calls
 * (a chain split over two calls keeps its slots when the other call's slots hold BOD_CORRUPT_NONE). */
enum { BOD_CORRUPT_NONE = 0, BOD_CORRUPT_LUT = 1, BOD_CORRUPT_CONTRAST = 2, BOD_CORRUPT_IMPULSE_NOISE = 3,
       BOD_CORRUPT_GAUSSIAN_NOISE = 4, BOD_CORRUPT_CONV2D = 5, BOD_CORRUPT_PIXELATE = 6, BOD_CORRUPT_JPEG = 7, BOD_CORRUPT_FOG = 8 };
typedef struct bod_corrupt_op {   /* 32 bytes */
    int32_t  kind;                /* BOD_CORRUPT_* */
    float    f0;                  /* CONTRAST: the factor k (finite); GAUSSIAN_NOISE: sigma in grey levels, 0..128; else unused */
    uint32_t u0;                  /* IMPULSE_NOISE: threshold T; PIXELATE: block size f, 2..64; FOG: strength a, 0..256; else unused */
    int32_t  tap_offset;          /* CONV2D: first tap of the kernel in `taps` */
    int32_t  ksize;               /* CONV2D: K (odd, 1..25) */
    int32_t  table;               /* LUT: index into luts; JPEG: index into qtables */
    int32_t  reserved[2];         /* 0 */
} bod_corrupt_op;
/* The stage alone (stand-alone device entry, as bod_jpeg_decode_rgb): n frames packed back to back (frame b at byte 3 * sum of
 * h_i * w_i over i < b) with sizes src_hw[n][2], their chains and ids frame_ids[n] (NULL: 0, 1, ..) -> rgb_packed_out, same
 * packing.  taps / luts / qtables may be NULL when their count is 0.  Errors through bod_last_error(NULL). */
bod_status bod_corrupt_frames_u8(int32_t device, int32_t n, const uint8_t* rgb_packed_in, const int32_t* src_hw,
                                 const bod_corrupt_op* ops, int32_t ops_per_frame, const uint32_t* frame_ids,
                                 const uint16_t* taps, int32_t n_taps, const uint8_t* luts, int32_t n_luts,
                                 const uint16_t* qtables, int32_t n_qtables, uint64_t seed, uint8_t* rgb_packed_out);
/* One-shot: the same description for the handle's `batch` frames, copied before return and consumed by the handle's NEXT packed
 * upload -- bod_upload_frames_u8_ragged[_async], bod_upload_frames_u8_augmented[_async] or bod_upload_frames_jpeg[_async].  The
 * stage runs on that upload's stream after the copy (or the JPEG colour kernel) and before the preprocess kernel, under the same
 * events and buffer ownership: the image buffer ends up bit for bit as after the upload of bod_corrupt_frames_u8's output.  The
 * corrupted frame never exists on the host.  ops == NULL clears a pending description.  A uniform bod_upload_frames_u8[_async]
 * with one pending fails with BOD_ERR_INVALID_ARG and consumes nothing; an upload that fails leaves it pending.
 * Both entries validate before anything is enqueued: BOD_ERR_INVALID_ARG naming the frame and the op for an unknown kind,
 * ops_per_frame outside 1..4, an even ksize or one outside 1..25, taps that do not sum to 2^15, tap_offset + ksize^2 past n_taps,
 * a block size outside 2..64, a table index past its table, a zero quantisation entry, a sigma that is not finite or
 * outside [0, 128], a contrast factor that is not finite, a fog strength above 256; the handle stays as it was. */
bod_status bod_set_upload_corruption(bod_handle h, const bod_corrupt_op* ops, int32_t ops_per_frame, const uint32_t* frame_ids,
                                     const uint16_t* taps, int32_t n_taps, const uint8_t* luts, int32_t n_luts,
                                     const uint16_t* qtables, int32_t n_qtables, uint64_t seed);
/* Rendering (render_kernels.hip): detections and their corner uncertainty drawn onto uint8 RGB frames on the device.
 * A stand-alone stage like bod_corrupt_frames_u8, with the same packing: frame b starts at byte 3 * sum of h_i * w_i over i < b, sizes
 * src_hw[n][2] (1..65535 each).  Frame f owns rows [sum of num_det[i] over i < f, + num_det[f]) of the det_* arrays and likewise of
 * gt_boxes.  The drawing rules are this library's own and are defined to the byte: tests/render_reference.py restates them in NumPy.
 *
 * Pixel (x, y) is the integer lattice point.  Every blend is v' = (v*(256 - A) + colour*A + 128) >> 8 per channel, A in 0..256.
 * Primitives are applied strictly in the order below, within a pass in ascending row index (painter's order), so a frame's result
 * depends on its bytes and its rows alone: not on the batch, the tiling or the launch shape.  Boxes may lie partly or wholly outside
 * the frame; drawing is clipped.
 *
 * BOD_RENDER_OVERLAY
 *   pass 0  every ground-truth box: the ring of width 1 in colour (0, 255, 0).
 *   pass A  per detection: the ring of width 1 in the detection's colour; if `labels` and the text has L > 0 glyphs (det_text row: up
 *           to 16 glyph indices, 0xFF ends it), a black filled rectangle over x in [x0, x0 + 6L], y in [y0, y0 + 8], then the set bit
 *           (row r, column j) of glyph i at (x0 + 1 + 6i + j, y0 + 1 + r) in the detection's colour.  All of pass A has A = 256.
 *   pass B  per detection: the top-left ellipse at centre (x0, y0), the bottom-right ellipse at centre (x1, y1), then the ring of
 *           width max(t - 1, 1), t = line_width.
 *   Ring of width w on (x0, y0, x1, y1), with a = w / 2 and b = (w + 1) / 2 (integer division): a pixel is covered (A = 256) iff
 *           x in [x0 - a, x1 + a] and y in [y0 - a, y1 + a] and not (x in [x0 + b, x1 - b] and y in [y0 + b, y1 - b]).  A box with
 *           x1 < x0 or y1 < y0 draws nothing.
 *   Ellipse of a corner covariance, a = S_xx, b = S_xy, c = S_yy (fp32): skipped, and counted in skipped_ellipses[frame], unless a, b, c
 *           are finite, a > 0, c > 0 and det = a*c - b*b > 0 (fp32, two products and a difference).  Extents, computed in double:
 *           ex = ceil(1.5 * sqrt(r2 * a)) + t + 1, ey = ceil(1.5 * sqrt(r2 * c)) + t + 1, each capped at 4096; the coverage is 0 by
 *           definition outside |dx| <= ex, |dy| <= ey (dx = x - centre x, dy = y - centre y).  Inside, in fp32 without contraction:
 *               gx = (c*dx - b*dy) / det;  gy = (a*dy - b*dx) / det;  q = dx*gx + dy*gy;
 *               if (!(q > 0)) A = 0; else { m = sqrtf(q); g = sqrtf(gx*gx + gy*gy); dist = fabsf(m - sqrtf(r2)) * m / g;
 *                                           cov = fminf(fmaxf((0.5f*t + 0.5f) - dist, 0), 1); A = (int)(cov * 256.0f); }
 *           (+, -, *, / and sqrtf only, all correctly rounded; fmaxf / fminf return the operand that is not a NaN), in the detection's
 *           colour.  dist is the first-order distance to the contour of squared Mahalanobis radius r2.
 * BOD_RENDER_HEAT
 *   A per-pixel index plane starts at 0.  Detections in ascending order: wherever the detection's box heatmap h -- exactly the float32
 *   map bod_pdq_frames(.., heatmaps) yields for that row on a frame of this size, made by the same device code -- is nonzero,
 *   index = (int)(h * 255.0f); the last nonzero write wins.  Colour of index i, with x = 4i: R = clip(min(x - 382, 1147 - x), 0, 255),
 *   G = clip(min(x - 127, 892 - x), 0, 255), B = clip(min(x + 128, 637 - x), 0, 255).  Output = (26*v + 230*colour + 128) >> 8.
 *   Rows bod_pdq_frames refuses (and a frame wider than 4000) are refused here the same way, before anything is drawn.  Detections are
 *   taken in chunks of at most 4096 rows whose heatmaps fit 64 MiB (at least one row): the device scratch of the view is at most
 *   3 * max(64 MiB, 4*h*w bytes) plus 1 KiB + 16*h + 8*w bytes per chunk row, whatever D is.
 * Font: 5x7 glyphs for a-z, 0-9, '.', ' ', '%', '-', '_' (41 glyphs, indices in this order).  bod_render_font writes them as
 *   glyph_rows[count][7], low 5 bits of a byte, bit 4 = the leftmost column (glyph_rows may be NULL to ask for count alone).
 * Errors through bod_last_error(NULL).  BOD_ERR_INVALID_ARG, naming the frame and the row where there is one: n < 0, a NULL array with
 * a nonzero count, a negative count, a frame size outside 1..65535, line_width outside 1..7, r2 not finite or not > 0, an unknown
 * view, a glyph index >= count that is not 0xFF.  n == 0 is BOD_OK.  opt == NULL: OVERLAY, line_width 2, labels on, r2 6.180074f. */
enum { BOD_RENDER_OVERLAY = 0, BOD_RENDER_HEAT = 1 };
typedef struct bod_render_options {   /* 32 bytes */
    int32_t view;          /* BOD_RENDER_* */
    int32_t line_width;    /* t, 1..7: ellipses use t, the second-pass box max(t-1,1), the first-pass box 1 */
    int32_t labels;        /* 0/1 */
    float   r2;            /* squared Mahalanobis radius of the contour; default 6.180074f
                              (= chi2.ppf(2*Phi(2)-1, 2): the 2-sigma contour the reference's demo draws) */
    int32_t reserved[4];   /* 0 */
} bod_render_options;
bod_status bod_render_frames_u8(int32_t device, int32_t n, const uint8_t* rgb_packed_in, const int32_t* src_hw,
                                const int32_t* num_det, const int32_t* det_boxes, const float* det_corner_covs,
                                const uint8_t* det_colors, const uint8_t* det_text, const int32_t* num_gt,
                                const int32_t* gt_boxes, const bod_render_options* opt, uint8_t* rgb_packed_out,
                                int32_t* skipped_ellipses);
bod_status bod_render_font(uint8_t* glyph_rows, int32_t* count);
/* PNG frames decoded inside the library, the JPEG entries' counterpart for KITTI's files.  Chunk parsing and the
 * zlib inflate run on host threads (no zlib is linked); the reconstruction of the filtered scanlines (PNG specification section 9:
 * None, Sub, Up, Average, Paeth) runs on the device and writes the uint8 RGB frames into the staging buffer the ragged / augmented
 * preprocess kernels read: the decoded frame never exists on the host.  PNG is lossless: the frames equal PIL's
 * Image.open(..).convert('RGB') byte for byte (RGBA loses its alpha, gray and gray + alpha give the gray byte three times).
 * Supported: bit depth 8, colour type 0 (gray), 2 (RGB), 4 (gray + alpha) or 6 (RGBA), interlace method 0, no tRNS and no acTL
 * chunk.  Palette images, bit depths 1, 2, 4 and 16, Adam7 interlacing and files with a tRNS or acTL chunk are well-formed but NOT
 * supported: bod_png_info reports them with supported = 0 and the reason in bod_last_error(NULL) (so does a file without the PNG
 * signature: a JPEG), the other entry points refuse them with BOD_ERR_INVALID_ARG.  A bad CRC-32 of a critical chunk or Adler-32,
 * a truncated file or stream, a stream that gives more or fewer bytes than height * (1 + width * channels), a filter-type byte
 * beyond 4, a width or height of 0 or beyond 65535 are BOD_ERR_INVALID_ARG (bod_png_info checks the header and the chunk layout;
 * what lies inside IDAT is checked where it is inflated).
 * (The struct has no typedef: in C a typedef would share the function's name space.) */
struct bod_png_info {
    int32_t width, height, bit_depth, color_type;
    int32_t channels;                /* bytes per pixel of the filtered scanlines: 1, 3, 2 or 4 for colour type 0, 2, 4, 6 */
    int32_t interlace;
    int32_t supported;               /* 0: well-formed but outside the supported subset (the message says why) */
    int64_t raw_bytes;               /* height * (1 + width * channels): what bod_png_inflate writes */
};
/* Header and inflate stage alone: host only, no handle, no device (as bod_jpeg_info); errors through bod_last_error(NULL).
 * bod_png_inflate writes the filtered scanlines: per row one filter-type byte (0..4), then width * channels bytes. */
bod_status bod_png_info(const uint8_t* data, int64_t len, struct bod_png_info* out);
bod_status bod_png_inflate(const uint8_t* data, int64_t len, uint8_t* raw, int64_t raw_capacity);
/* The decoder alone (as bod_jpeg_decode_rgb): n files -> packed RGB on the host (frame b at byte 3 * sum of h_i * w_i over i < b)
 * + src_hw[n][2].  `threads` host threads inflate the files (capped at 16 and at n; <= 0 means 1). */
bod_status bod_png_decode_rgb(int32_t device, int32_t n, const uint8_t* const* data, const int64_t* len,
                              int32_t threads, uint8_t* rgb_packed, int64_t rgb_capacity, int32_t* src_hw);
/* Measurement entry (as bod_bench_head_conv; tests/tools/bench_png.py): the decoder's two halves timed apart on n files.
 * host_ms[iters]: the host half as the uploads run it -- headers, layout, inflate on `threads` of the library's worker threads
 * into pinned staging -- by the host clock (the first iteration also allocates the staging).  kernel_ms[iters]:
 * png_unfilter_kernel alone on the batch, by events around each launch, after one launch that is not timed. */
bod_status bod_bench_png_decode(int32_t device, int32_t n, const uint8_t* const* data, const int64_t* len,
                                int32_t threads, int32_t iters, double* host_ms, double* kernel_ms);
/* The upload routes, word for word bod_upload_frames_jpeg[_async] with PNG files: inflated on `threads` host threads into pinned
 * staging the handle owns (one per image buffer; the host waits for the previous copy out of it first), then the copy, the
 * unfilter kernel and the ragged (aug == NULL) or augmented preprocess kernel run on the upload's stream.  Everything else is
 * bod_upload_frames_u8_ragged[_async] / bod_upload_frames_u8_augmented[_async] of the decoded frames, bit for bit (geometry
 * errors, per-frame KITTI factors, bod_set_upload_corruption).  The host stage finishes before the call returns: `data` is free
 * on return.  A corrupt or unsupported frame gives BOD_ERR_INVALID_ARG naming the frame and the reason; nothing is enqueued, the
 * handle and the frames it held stay as they were. */
bod_status bod_upload_frames_png(bod_handle h, const uint8_t* const* data, const int64_t* len,
                                 const float* rgb_means, int32_t aspect_resize, const bod_augment* aug,
                                 int32_t threads, int32_t* src_hw_out);
bod_status bod_upload_frames_png_async(bod_handle h, const uint8_t* const* data, const int64_t* len,
                                       const float* rgb_means, int32_t aspect_resize, const bod_augment* aug,
                                       int32_t threads, int32_t* src_hw_out, int32_t buffer);
const float* bod_device_images_buffer(bod_handle h, int32_t buffer);
const float* bod_device_images(bod_handle h);
bod_status bod_synchronize(bod_handle h);

/* Stage entry point for parity tests of the hot kernel: ONE convolution of the forward pass
 * (keras Conv2D semantics) through the same implicit-GEMM MFMA kernel and
 * epilogue the pipeline uses.  x [B,H,W,Cin] and w [KH,KW,Cin,Cout] (HWIO) are fp32 host arrays
 * and are rounded to bf16 exactly as stored activations / packed weights are; bias fp32 (may be
 * NULL); residual [B,OH,OW,Cout] optional (added before ReLU, like the bottleneck shortcut,
 * feature_extractor.py:210-212).  dropout_rate > 0 applies the head-tower epilogue
 * (multitask_headers.py:102-116): batch item b plays MC sample b, pixel index = y*OW+x.
 * out [B,OH,OW,Cout] fp32; round_output_bf16 != 0 rounds it like a stored activation.
 * precision = BOD_PRECISION_FP32 runs the fp32 twin of the kernel on unrounded fp32 operands.
 * precision = BOD_PRECISION_F16MX / BOD_PRECISION_F16MX4 (3x3, stride 1, SAME, 256 -> 256 only: a head-tower layer) runs that tower kernel on the
 * row-reuse loop; round_output_bf16 then selects the data path under test: 0 = hx rows in, (hi, lo) pairs out (a head's last
 * layer); 1 = hx rows in, hx rows out (a middle layer; `out` is the decoded hx row: f16 hi + e2m3 lo); 2 = (hi, lo) pairs in,
 * hx rows out (the first layer).
 * Errors are reported through bod_last_error(NULL). */
bod_status bod_stage_conv(int32_t device, const float* x, int32_t B, int32_t H, int32_t W, int32_t Cin,
                          const float* w, const float* bias, int32_t KH, int32_t KW, int32_t Cout,
                          int32_t stride, int32_t same_padding, int32_t relu, const float* residual,
                          float dropout_rate, uint64_t seed, int32_t layer_id, uint32_t image_id,
                          int32_t round_output_bf16, int32_t precision, float* out);

/* Stage entry point of the training step's hot kernel (run_training.py:208-247
 * tape.gradient): the WEIGHT GRADIENT of one Conv2D, dw[KH,KW,Cin,Cout] = dL/dW and db[Cout] = dL/db given the
 * layer input x [B,H,W,Cin] and the output gradient dy [B,OH,OW,Cout] (keras Conv2D geometry as in
 * bod_stage_conv; x and dy are rounded to bf16 like stored activations, accumulation is fp32).  Runs as a
 * pixel-reduction GEMM on the forward implicit-GEMM MFMA kernel: im2col^T of x through the forward row table,
 * dy transposed, reduction split over `ksplit` workgroups per tile (0 = chosen automatically).  The input
 * gradient as a forward convolution needs no entry point of its own: it is bod_stage_conv on dy with the spatially
 * flipped, cin/cout swapped weights (tests/test_gpu_train_blocks.py); the step's own three accumulating launches are
 * bod_stage_conv_dgrad below.  Errors via bod_last_error(NULL). */
bod_status bod_stage_conv_wgrad(int32_t device, const float* x, int32_t B, int32_t H, int32_t W, int32_t Cin,
                                const float* dy, int32_t KH, int32_t KW, int32_t Cout, int32_t stride,
                                int32_t same_padding, int32_t ksplit, float* dw, float* db);

/* Stage entry points of the backward kernels that only the bf16 training handle launches (DESIGN.md 9.12,
 * tests/test_gpu_train_backward_kernels.py).  Each one builds a throw-away context, calls the library's own launchers
 * the way the training step does and copies the results back.  Every offset and size a kernel would turn into an
 * address is checked on the host first: BOD_ERR_INVALID_ARG, nothing launched.  bf16 tensors cross the boundary as
 * fp32 host arrays (rounded to nearest even on the way in, widened exactly on the way out) unless stated otherwise.
 * Errors via bod_last_error(NULL).
 *
 * Activation backward of one layer (launch_relu_merge when dout_relu is given, then launch_act_backward_gather, then
 * launch_gather_transpose when dZ^T is wanted and the launch did not write it).  dout [out_elems] fp32 is the gradient
 * of the layer's output in the output buffer's own layout, out_act [out_elems] the stored output (NULL: no activation),
 * dout_relu [out_elems] the gradient of the output's ReLU'd copy (NULL: none).  Row m reads pixel out_off[m] (channel
 * stride out_cstride) and, with dres, adds into pixel res_off[m] (stride res_cstride) of dres [dres_elems], which is
 * read and written.  dz [M][cout_pad] is written; dzp [out_elems] and dzt [cout_pad][Kpad] are optional (NULL: not
 * wanted, the launcher then sees no such buffer), prefilled by the caller and written where the kernels write them.
 * *wrote_transpose: 1 when the tile kernel wrote dZ^T itself.  precision: BOD_PRECISION_BF16 or BOD_PRECISION_FP32. */
bod_status bod_stage_act_backward(int32_t device, int32_t precision, const float* dout, const float* out_act, const float* dout_relu,
                                  int64_t out_elems, const int32_t* out_off, const int32_t* res_off, int32_t M, int32_t cout,
                                  int32_t cout_pad, int32_t out_cstride, int32_t res_cstride, float scale, int32_t Kpad, float* dres,
                                  int64_t dres_elems, float* dz, float* dzp, float* dzt, int32_t* wrote_transpose);

/* Input gradient of one bf16 Conv2D through one of the training step's three launches, each with CONV_OUT_F32 and (the
 * first two) CONV_ACCUM: BOD_DGRAD_FLIP = convolution of the dZ plane with the flipped weights (3x3, stride 1, SAME),
 * BOD_DGRAD_ROWS = the 1x1 GEMM through the table of launch_make_dgrad_rows, BOD_DGRAD_COL2IM = dXcol + col2im.
 * dz [groups][B,OH,OW,Cout] and w [groups][KH,KW,Cin,Cout] (master layout, packed by launch_fold_pack without
 * batch-norm) are rounded to bf16; din [groups][B,H+2,W+2,Cin] is the fp32 gradient plane of the layer's input with
 * its one-pixel border, read and written.  ksplit 0 = the step's own rule, otherwise forced; groups 1..3 run as one
 * grouped launch (BOD_DGRAD_FLIP only).  info2 (may be NULL): {split-K factor used, 1 if the launch took the 256x256 tile}. */
enum { BOD_DGRAD_FLIP = 0, BOD_DGRAD_ROWS = 1, BOD_DGRAD_COL2IM = 2 };
bod_status bod_stage_conv_dgrad(int32_t device, int32_t route, const float* dz, const float* w, int32_t B, int32_t H, int32_t W,
                                int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t same_padding,
                                int32_t ksplit, int32_t groups, float* din, int32_t* info2);

/* Backward of ZeroPadding2D((1,2)) + MaxPool 3x3 s2 under the stem's ReLU (launch_stem_pool_backward): stem_out and dz
 * [B,ih,iw,64]; dpool is the pooled gradient on its bordered plane [B,oh+2,ow+2,64] fp32 with oh = (ih - 1) / 2 + 1 and
 * ow = (iw + 1) / 2 + 1 as handle creation derives them (dpool_elems must say exactly that). */
bod_status bod_stage_stem_pool_backward(int32_t device, int32_t precision, const float* stem_out, const float* dpool, int64_t dpool_elems,
                                        int32_t B, int32_t ih, int32_t iw, float* dz);

/* Stage entry points of the stem and stem-pool kernels (tests/test_gpu_stem_kernels.py), built like the
 * ones above: a throw-away context, host arrays in and out, the library's own launchers, every size, pointer and
 * precondition checked on the host before anything is launched (BOD_ERR_INVALID_ARG), errors via bod_last_error(NULL).
 *
 * bod_stage_stem runs ONE form of the stem on images [B,H,W,3] fp32, w [7][7][3][64] fp32 (folded) and bias [64].
 * Geometry as bod_create derives it: oh = (H-7)/2+1, ow = (W-7)/2+1, ph = (oh-1)/2+1, pw = (ow+1)/2+1.
 * form = BOD_STEM_AUTO follows the pipeline's rule for `precision` (BOD_PRECISION_FP32, _BF16 or _BF16X3): the fused
 * kernel where stem_pool_fused_applies says so for this image pointer, W, B and n_cu (the stream's compute-unit share,
 * as the forward pass passes it; <= 0: the rule's default of 256), else launch_stem_conv's choice and the pooling
 * launch.  An explicit form names the kernels and must fit `precision`:
 *   BOD_STEM_F32_POOL_F32     fp32 stem, stem_pool_f32_kernel                 (FP32)
 *   BOD_STEM_F32_POOL_SPLIT   fp32 stem, stem_pool_split_kernel               (BF16X3; pooled pixels are 128 slots)
 *   BOD_STEM_SEG64_POOL       64-pixel bf16 stem, stem_pool_kernel            (BF16)
 *   BOD_STEM_ROW_POOL         row bf16 stem, stem_pool_kernel                 (BF16; W % 4 == 0, aligned image)
 *   BOD_STEM_FUSED_8 / _4     stem + pool in one kernel on 8 / 4 waves        (BF16; as ROW, and ow <= 256)
 *   BOD_STEM_FUSED_SPLIT      the fused kernel of the (hi, lo) precisions     (BF16X3; as the fused forms; 128 slots)
 * An explicit form whose precondition does not hold is refused.  misalign != 0 places the device image 4 bytes past a
 * 16-byte boundary (BOD_STEM_AUTO then has to fall back to the 64-pixel kernel).  Requires H, W >= 7 and at most 2^22
 * input pixels.
 * stem_out [B,oh,ow,64] (may be NULL) receives the stem plane of the forms that write one (the fused forms leave it
 * untouched); pooled [B,ph+2,pw+2,64 or 128] (may be NULL) the pooled plane INCLUDING its one-pixel border, the 128
 * slots of a pair pixel in storage order.  bf16 values come back widened to fp32.  Both device planes are filled
 * with `sentinel` (a value bf16 holds exactly, e.g. -65536) before the launch and lie between two guard regions of the same
 * fill; a guard that changed is BOD_ERR_HIP.  *form_ran: the explicit form that ran. */
enum { BOD_STEM_AUTO = 0, BOD_STEM_F32_POOL_F32 = 1, BOD_STEM_F32_POOL_SPLIT = 2, BOD_STEM_SEG64_POOL = 3, BOD_STEM_ROW_POOL = 4,
       BOD_STEM_FUSED_8 = 5, BOD_STEM_FUSED_4 = 6, BOD_STEM_FUSED_SPLIT = 7 };
bod_status bod_stage_stem(int32_t device, int32_t form, int32_t precision, const float* images, int32_t B, int32_t H, int32_t W,
                          const float* w, const float* bias, int32_t misalign, int32_t n_cu, float sentinel, float* stem_out,
                          float* pooled, int32_t* form_ran);

/* launch_stem_pool alone on a caller-supplied stem plane stem [B,ih,iw,64]: mode 0 bf16 -> bf16 (the plane is rounded
 * to bf16 on the way in), 1 fp32 -> fp32, 2 fp32 -> (hi, lo) pairs.  pooled [B,oh+2,ow+2,64 (mode 2: 128)] with
 * oh = (ih-1)/2+1, ow = (iw+1)/2+1 comes back with its border; the device plane is prefilled with `sentinel` and guarded as
 * above.  At most 2^22 stem pixels. */
bod_status bod_stage_stem_pool(int32_t device, int32_t mode, const float* stem, int32_t B, int32_t ih, int32_t iw, float sentinel,
                               float* pooled);

/* Fold batch-norm into the master weights and pack them, all `count` layers in ONE launch_fold_pack_all launch, bf16
 * mode.  Inputs: kernel [taps][cin][cout], bias / gamma / beta / mean / var [cout] or NULL (the four batch-norm arrays
 * together).  Outputs, each optional except b_fwd: w_fwd [cout_pad][taps][cin], w_bwd [(tap, ci)][cout_pad] and w_flip
 * [cin][taps, flipped][cout_pad] as raw bf16 bits, w_fwd32 [taps*cin][cout] fp32 (the stem's), b_fwd [cout_pad] fp32. */
typedef struct bod_fold_layer {
    const float* kernel; const float* bias; const float* gamma; const float* beta; const float* mean; const float* var;
    int32_t taps, cin, cout, cout_pad;
    uint16_t* w_fwd; uint16_t* w_bwd; uint16_t* w_flip; float* w_fwd32; float* b_fwd;
} bod_fold_layer;
bod_status bod_stage_fold_pack(int32_t device, int32_t count, const bod_fold_layer* layers);

/* One training step, run_training.train_single_step (:208-247), on a handle created with training = 1:
 * forward in training mode (dropout on, batch-norm frozen), total loss = w_cls * focal + w_reg * regression
 * (reg_kind as in bod_loss_forward) + Keras l2(l2_rate) on the header tower kernels and cov_out, backward through
 * the whole network, tf.clip_by_global_norm(5.0) and keras Adam(epsilon = 1e-2) with `learning_rate` (the piecewise
 * schedule is the caller's, :48-61).  Targets as the dataset handler produces them: cls_targets [B,A,C],
 * box_targets [B,A,4], positive / negative anchor masks [B,A] (bytes).  apply_update = 0 stops after the
 * gradients (tests).  out6 = {total_loss, cls_loss, reg_loss, covariance_loss, regularization_loss, global
 * gradient norm before clipping}. */
bod_status bod_train_step(bod_handle h, const float* images, int32_t images_on_device, const float* cls_targets,
                          const float* box_targets, const uint8_t* positive_mask, const uint8_t* negative_mask,
                          uint64_t seed, uint32_t first_image_id, int32_t reg_kind, float label_smoothing,
                          float w_cls, float w_reg, float l2_rate, float learning_rate, int32_t apply_update,
                          double* out6);
/* The same step from what a dataset gives: per frame num_gt[b] >= 1 ground-truth rows (the handlers' placeholder row
 * [0,0,1,1] with a background class for a frame without boxes), gt_boxes_vuvu [sum G,4] corners (y1, x1, y2, x2) and
 * gt_classes [sum G,C] rows (C = the handle's num_classes).  The dense targets are assigned on the device against the
 * handle's anchors (bod_set_anchors) by the kernel of bod_anchor_targets, into the buffers bod_train_step copies its
 * targets to; everything after that is bod_train_step, arguments from `seed` on included. */
bod_status bod_train_step_boxes(bod_handle h, const float* images, int32_t images_on_device, const int32_t* num_gt,
                                const float* gt_boxes_vuvu, const float* gt_classes, float min_positive_iou,
                                float max_negative_iou, uint64_t seed, uint32_t first_image_id, int32_t reg_kind,
                                float label_smoothing, float w_cls, float w_reg, float l2_rate, float learning_rate,
                                int32_t apply_update, double* out6);
/* The targets the last step (either entry point) used, read back: cls_targets [B,A,C], box_targets [B,A,4], masks [B,A]. */
bod_status bod_train_get_targets(bod_handle h, float* cls_targets, float* box_targets, uint8_t* positive_mask,
                                 uint8_t* negative_mask);
/* Data-parallel training (one process per GPU): after bod_train_step(..., apply_update = 0) the gradients of ALL
 * trainable tensors lie in one contiguous fp32 device array -- bod_train_gradients returns its address and length
 * (the handle's stream is synchronised first) -- so the ranks need ONE all-reduce (RCCL) over it, then
 * bod_train_apply runs the clip + Adam update on whatever the array then holds (the mean gradient). */
bod_status bod_train_gradients(bod_handle h, void** device_ptr, int64_t* count);
bod_status bod_train_apply(bod_handle h, float learning_rate, double* grad_norm);
/* Read a trainable tensor of a training handle back: layer = Keras layer name (conv or batch-norm), kind 0 kernel
 * (HWIO) / 1 bias / 2 gamma / 3 beta, what 0 value / 1 gradient of the last step / 2, 3 Adam moments. */
bod_status bod_train_get(bod_handle h, const char* layer, int32_t kind, int32_t what, float* out, int64_t n);
/* Checkpoint / resume of the optimizer (tf.train.Checkpoint(step, optimizer, net) + ckpt.restore(manager.latest_checkpoint),
 * run_training.py:68-82): bod_train_set writes an Adam moment (what = 2 first, 3 second) of a trainable tensor back -- the
 * values themselves are restored through bod_load_weight before bod_finalize_weights -- and bod_train_step_count reads
 * (get != NULL) and / or sets (set >= 0) the number of updates applied so far, which enters Adam's bias correction. */
bod_status bod_train_set(bod_handle h, const char* layer, int32_t kind, int32_t what, const float* data, int64_t n);
bod_status bod_train_step_count(bod_handle h, int64_t* get, int64_t set);

/* model.get_loss(sample_dict, prediction_dict) forward (retinanet_model.py:151-328, core/losses.py:30-61;
 * BASELINE config 5's loss, forward only).  Host arrays: cls/cls_targets [B,A,C], box/box_targets [B,A,4],
 * covar_params [B,A,10] (pre fill_triangular; may be NULL unless reg_kind >= 2), anchors [A,4],
 * positive/negative masks [B,A] (bytes).  reg_kind: 0 none, 1 'regression', 2 'regression_var',
 * 3 'regression_covar', 4 'regression_nll', 5 'regression_energy' (the last two: below).
 * out4 = {sum of masked focal terms, sum of positive regression terms,
 * sum of positive 0.5*sum(log D) terms, number of positives}; the caller applies the
 * /max(num_pos,1) normalisation and the yaml loss weights. Errors via bod_last_error(NULL). */
bod_status bod_loss_forward(int32_t device, int32_t B, int32_t A, int32_t C, const float* cls,
                            const float* cls_targets, const float* box, const float* box_targets,
                            const float* covar_params, const float* anchors, const uint8_t* positive_mask,
                            const uint8_t* negative_mask, int32_t do_classification, int32_t reg_kind,
                            float label_smoothing, double* out4);

/* Proper scoring rules as training losses.  Per positive anchor, with pb / tb the decoded prediction and
 * target in vuhw pixels (the decode of reg_kind 2 / 3, clips and their zero gradient included), e = pb - tb, c[0..9] the raw
 * covariance parameters, ld = (c4, c9, c5, c0), A1 the unit-lower matrix with rows (1), (c8, 1), (c7, c6, 1), (c3, c2, c1, 1) and
 * Sigma = A1^-1 diag(exp ld) A1^-T -- the full covariance inference builds from the same ten numbers:
 *   reg_kind 4 'regression_nll':    regression term 0.5 sum_k exp(-ld_k) r_k^2 with r = A1 e, covariance term 0.5 sum_k ld_k
 *                                   (their sum + 2 ln 2pi is the Gaussian negative log-likelihood of tb);
 *   reg_kind 5 'regression_energy': regression term (1/M) sum_{i<M} |z_i - g| - 1/(2(M-1)) sum_{i<M-1} |z_i - z_{i+1}| with
 *                                   A1 y_i = exp(ld/2) o n_i, z_i = T (pb + y_i), g = T tb, T: vuhw -> (x1, y1, x2, y2);
 *                                   covariance term 0.
 * Normals of reg_kind 5: sample i of (image id, anchor a) is ONE call philox4x32_10(i, a, 0x0010555E, image id, seed &
 * 0xffffffff, seed >> 32) -> (x, y, z, w), u(t) = (t + 0.5) 2^-32, n0, n1 = sqrt(-2 ln u(x)) (cos, sin)(2 pi u(y)), n2, n3
 * likewise from (z, w); image id = first_image_id + frame.  A row's term and gradient depend on (seed, image id, anchor, M)
 * and the row's own tensors alone (bitwise), not on the batch around it.
 * energy_samples = M in [2, 1024]; anything else is BOD_ERR_INVALID_ARG.  reserved[0] holds flags: BOD_LOSS_ONE_IMAGE_ID = every
 * frame of the call is image `first_image_id` itself (validation: a frame's loss is then the one it has alone, whatever batch it
 * sits in and wherever; the training step ignores the flag).  reserved[1..3]: set to 0. */
#define BOD_LOSS_ONE_IMAGE_ID 1
typedef struct {
    int32_t energy_samples;
    uint64_t seed;
    uint32_t first_image_id;
    int32_t reserved[4];
} bod_loss_options;
/* bod_loss_forward / bod_loss_backward with the options of reg_kind 5; NULL = the defaults {64, 0, 0}, which is what the two
 * plain entries use.  reg_kind 0..4 ignore everything but the range check of energy_samples. */
bod_status bod_loss_forward_ex(int32_t device, int32_t B, int32_t A, int32_t C, const float* cls,
                               const float* cls_targets, const float* box, const float* box_targets,
                               const float* covar_params, const float* anchors, const uint8_t* positive_mask,
                               const uint8_t* negative_mask, int32_t do_classification, int32_t reg_kind,
                               float label_smoothing, double* out4, const bod_loss_options* options);
/* The options of a handle's entries (NULL = defaults).  bod_train_step / bod_train_step_boxes take energy_samples from here and
 * the seed and the first image id from their own arguments (a recorded step reads them from the device scalars its dropout
 * reads, so every replay draws new normals; another energy_samples re-records).  bod_validation_losses_boxes and
 * bod_validate_boxes take all three from here. */
bod_status bod_set_loss_options(bod_handle h, const bod_loss_options* options);

/* Anchor-target assignment (bbox_iou_vuvu + positive_negative_batching + generate_anchor_targets of the dataset handlers;
 * stateless, host arrays in and out): anchors_vuhw [A,4], per frame num_gt[b] >= 1 rows of gt_boxes_vuvu [sum G,4] and
 * gt_classes [sum G,C], C >= 2 with the background class last.  All fp32 in the host code's op order: IoU with the +1 pixel
 * convention and the reference's area expression, positive = any IoU >= min_positive_iou, negative = all IoU <=
 * max_negative_iou, best GT = first row of the largest IoU; box_targets [B,A,4] are written for every anchor, cls_targets
 * [B,A,C] hold the best GT's class row where positive and the background row elsewhere, masks [B,A] are bytes.  best_gt
 * [B,A] (row within the frame) and best_iou [B,A] may be NULL.  Degenerate boxes are not rejected (a non-finite target is
 * the caller's data).  Errors via bod_last_error(NULL). */
bod_status bod_anchor_targets(int32_t device, int32_t A, const float* anchors_vuhw, int32_t B, const int32_t* num_gt,
                              const float* gt_boxes_vuvu, const float* gt_classes, int32_t C, float min_positive_iou,
                              float max_negative_iou, float* cls_targets, float* box_targets, uint8_t* positive_mask,
                              uint8_t* negative_mask, int32_t* best_gt, float* best_iou);

/* ---- validation from ground-truth boxes (src/retina_net/experiments/run_validation.py:230-260 val_single_step, followed by
 * validation_utils.post_process_predictions, :10-77), for `batch` frames of an inference handle with mc_samples = 1; the raw head
 * outputs, the dense targets and the candidates never leave the device.  The three calls return BOD_ERR_INVALID_ARG for a
 * training handle, mc_samples != 1, reg_kind >= 2 without the covariance head, a class count other than 4 or 8 and
 * num_gt[b] < 1, and BOD_ERR_NOT_READY for missing anchors, a missing forward or a missing bod_nms.
 *
 * model.get_loss(sample_dict, prediction_dict) of val_single_step (:247-258) per frame: stage entry on the handle's current raw
 * outputs (after bod_forward or bod_set_raw; MC sample 0).  The ground truth is given as to bod_train_step_boxes: num_gt[b] >= 1
 * rows per frame (the placeholder row [0,0,1,1] with the background class for a frame without boxes), gt_boxes_vuvu [sum G,4],
 * gt_classes [sum G,C].  The dense targets are assigned on the device by the kernel of bod_anchor_targets into buffers the handle
 * allocates on its first validation call; the loss terms are those of bod_loss_forward (do_classification, reg_kind and
 * label_smoothing as there), summed per frame: sums4 [batch][4] = {sum of masked focal terms, sum of positive regression terms,
 * sum of positive 0.5*sum(log D) terms, number of positives}.  Block partials are added in double in a fixed order: a frame's four
 * sums are bitwise independent of the batch it sits in and of its position there. */
bod_status bod_validation_losses_boxes(bod_handle h, const int32_t* num_gt, const float* gt_boxes_vuvu, const float* gt_classes,
                                       float min_positive_iou, float max_negative_iou, int32_t do_classification,
                                       int32_t reg_kind, float label_smoothing, double* sums4);
/* The return value of validation_utils.post_process_predictions (:62-77) for every image, after bod_validation_post and bod_nms:
 * the class rows and the corners (y1, x1, y2, x2; network-input pixels) of the selected candidates in soft-NMS order, gathered on
 * the device and copied with one copy per array and one synchronise.  num_detections [batch]; scores [batch,max_detections,C];
 * corners [batch,max_detections,4]; rows >= num_detections[b] are zero.  NULLs skipped. */
bod_status bod_get_validation_detections_batch(bod_handle h, int32_t* num_detections, float* scores, float* corners);
/* The loop body of run_validation.py:108-204 for `batch` frames -- val_single_step, then post_process_predictions: forward, loss
 * sums, validation post, NMS, record gather on one stream, no host round trip until the final copies.  images as in bod_forward;
 * the other arguments and the results as in the two calls above, which it equals bit for bit. */
bod_status bod_validate_boxes(bod_handle h, const float* images, int32_t images_on_device, const int32_t* num_gt,
                              const float* gt_boxes_vuvu, const float* gt_classes, float min_positive_iou,
                              float max_negative_iou, int32_t do_classification, int32_t reg_kind, float label_smoothing,
                              double* sums4, int32_t* num_detections, float* scores, float* corners);

/* Gradient of  total = w_cls * S_cls / max(n_pos,1) + w_reg * (S_cmp + S_reg) / max(n_pos,1)  (the reference's
 * total_loss before the L2 term, retinanet_model.py:183-323) with respect to the raw head outputs: dcls [B,A,C],
 * dbox [B,A,4], dcov [B,A,10] (NULL = not wanted).  Arguments as bod_loss_forward; out4 receives the same sums.
 * First piece of the training step's backward pass. */
bod_status bod_loss_backward(int32_t device, int32_t B, int32_t A, int32_t C, const float* cls,
                             const float* cls_targets, const float* box, const float* box_targets,
                             const float* covar_params, const float* anchors, const uint8_t* positive_mask,
                             const uint8_t* negative_mask, int32_t do_cls, int32_t reg_kind, float label_smoothing,
                             float w_cls, float w_reg, double* out4, float* dcls, float* dbox, float* dcov);
/* The same with the options of reg_kind 5 (bod_loss_forward_ex); NULL = defaults. */
bod_status bod_loss_backward_ex(int32_t device, int32_t B, int32_t A, int32_t C, const float* cls,
                                const float* cls_targets, const float* box, const float* box_targets,
                                const float* covar_params, const float* anchors, const uint8_t* positive_mask,
                                const uint8_t* negative_mask, int32_t do_cls, int32_t reg_kind, float label_smoothing,
                                float w_cls, float w_reg, double* out4, float* dcls, float* dbox, float* dcov,
                                const bod_loss_options* options);

/* PDQ (Probability-based Detection Quality, prob_detection_quality.py) on the device; stateless, like bod_loss_forward.
 * Results match the CPU path's rules: corner regions, fp64 bivariate-normal CDFs stored as float32 heatmaps, NumPy slice
 * semantics for the boxes, per-pixel loss arguments formed in float32 and summed in fp64 (bitwise repeatable, independent
 * of how frames are split over calls).  Non-finite inputs, a non-positive variance, |correlation| > 1 or a corner whose
 * mean lies outside its region (where the CPU path raises) fail with BOD_ERR_INVALID_ARG.  Errors via bod_last_error(NULL).
 *
 * One Gaussian corner per row (stage entry for parity tests): means_yx [n,2], covs_yx [n,2,2];
 * rois [n,4] = x0 y0 x1 y1 (may be NULL), heatmaps [n,H,W] float32 (may be NULL). */
bod_status bod_pdq_corner_heatmaps(int32_t device, int32_t img_h, int32_t img_w, int32_t n, const double* means_yx,
                                   const double* covs_yx, int32_t* rois, float* heatmaps);
/* Frames of one image size: num_gt[F], gt_boxes [sum G,4] x1 y1 x2 y2; num_det[F], det_boxes [sum D,4] (PBoxDetInst.box),
 * det_corner_covs [sum D,2,2,2] (PBoxDetInst.covs: top-left then bottom-right, (x, y) order);
 * out: fg_loss / bg_loss [sum G_f*D_f] (per frame a row-major [G_f][D_f] block), det_bg_loss [sum D],
 * heatmaps [sum D,H,W] (may be NULL).  Image width at most 4000. */
bod_status bod_pdq_frames(int32_t device, int32_t img_h, int32_t img_w, int32_t num_frames, const int32_t* num_gt,
                          const int32_t* gt_boxes, const int32_t* num_det, const int32_t* det_boxes,
                          const double* det_corner_covs, double* fg_loss, double* bg_loss, double* det_bg_loss,
                          float* heatmaps);

/* Scoring rules of the box Gaussian on the device (score_kernels.hip, scoring_rules.py); stateless, fp64.
 * Row i pairs a 4-dimensional Gaussian (means [n,4], covs [n,4,4]) with a target (targets [n,4]).  L = lower Cholesky
 * factor of the covariance (Cholesky-Banachiewicz on the LOWER triangle; the upper one is not read).  out [n,8]:
 *   [0] nll = 0.5 (4 ln 2pi + ln det + m2)          [1] m2 = |L^-1 (g - mu)|^2 (squared Mahalanobis distance)
 *   [2] energy score (1/M) sum_{i<M} |z_i - g| - 1/(2(M-1)) sum_{i<M-1} |z_i - z_{i+1}|,  z_i = mu + L n_i,  M = num_samples
 *   [3..6] PIT_k = 0.5 erfc(-(g_k - mu_k) / sqrt(2 cov_kk))                              [7] ln det = 2 sum ln L_kk
 * status [n]: 2 = a non-finite input, 1 = a pivot <= 0 or non-finite, 0 otherwise; a row with status != 0 gets NaN in its
 * eight outputs, disturbs no other row and is no error of the call.
 * Normals: sample i of the row with id r = first_row_id + i_row is ONE call philox4x32_10(i, r & 0xffffffff, 0x005C04E5,
 * r >> 32, seed & 0xffffffff, seed >> 32) -> (x, y, z, w); u(t) = (t + 0.5) 2^-32; n0, n1 = sqrt(-2 ln u(x)) (cos, sin)
 * (2 pi u(y)), n2, n3 likewise from (z, w).  A row's result depends on its id alone: not on n, on its position, or on how
 * rows are split over calls (bitwise).  n = 0 is BOD_OK; n < 0, num_samples outside [2, 65536] or a NULL array with n > 0
 * fail with BOD_ERR_INVALID_ARG.  Errors via bod_last_error(NULL). */
bod_status bod_score_pairs(int32_t device, int64_t n, const double* means, const double* covs, const double* targets,
                           int32_t num_samples, uint64_t seed, uint64_t first_row_id, double* out, int32_t* status);

/* Kernel micro-benchmark (tests/tools): re-launches the `layer`-th head-tower launch of a bod_infer step
 * (0 = de-duplicated fan-out layer, 1 = tower layer 1; on plans with the fused MC aggregation 2 = layer 2 of the
 * heads that continue, 3 = layer 2 of the head that ends there (aggregating), 4 = layer 3; otherwise 2, 3 = layers
 * 2, 3) `iters` times on the handle's own buffers and returns the mean duration; `variant` selects an ablation
 * build of the kernel (0 = production). */
bod_status bod_bench_head_conv(bod_handle h, int32_t layer, int32_t variant, int32_t iters,
                               double* mean_ms, double* flops_per_launch);

/* Measurement hooks (bench.py): HIP-event timing of the dominant kernel on the handle's stream. */
bod_status bod_profile_begin(bod_handle h);
/* Which head 3x3 launches the hook times: 0 = all of them (default), 1 = only the launches of the row-reuse tower kernel
 * (tower layers 1..3 in bf16 mode: ONE kernel symbol, the one a rocprofv3 --kernel-trace summary lists first), 2 = the
 * others (the N-way fan-out launch of layer 0).  Stays in force until changed. */
bod_status bod_profile_select(bod_handle h, int32_t which);
/* total ms in head 3x3 conv launches since begin, number of launches, FLOPs (2*MACs) issued */
bod_status bod_profile_end(bod_handle h, double* head_conv_ms, int64_t* head_conv_launches,
                           double* head_conv_flops, double* posterior_ms, int64_t* posterior_launches);

/* ---- the path's ONE multi-GPU exchange for callers of the C ABI (no PyTorch in the loop) ----
 * Images shard across processes (one per GPU); per step every rank contributes the detection records of its batch and `root`
 * receives all of them.  A record row is W = bod_record_width() = 1 + 4 + 16 + 2C floats: [valid, mean (v,u,h,w), covariance
 * row-major, score[C], counts[C]] (BOD_PARTS_COVARIANCE handles: + 48, the three parts behind the counts; BOD_PARTS_CLASS handles: + 4, the class-entropy parts last); a rank's block is [batch][max_detections][W], rows beyond an image's detection count are zero.
 *
 * bod_gather_detections packs the records of `slot` (the ticket of bod_infer_async; pass -1 after a synchronous bod_infer) on the
 * device and issues ONE RCCL gather -- ncclGather(send, recv, batch*K*W, ncclFloat32, root, comm, stream).  For a ticket
 * (slot >= 0) both run on the stream that finished the slot's records -- the handle's MAIN stream -- behind its cluster-and-fuse
 * kernels and record copies, and the slot's event is re-recorded behind them: bod_collect(slot) and the next bod_infer_async that
 * reuses the slot wait for the send.  If the next bod_infer_async has already been enqueued, pack and gather run BEHIND its kernels
 * (one step of latency): since round 6 no kernel of this library runs beside another one by default (until then the
 * two ran on a side stream underneath the next batch's convolutions; BOD_SIDE_STREAM=1 restores that placement for reproduction
 * runs).  For slot == -1 both run on the handle's MAIN stream, behind the
 * synchronous bod_infer's own kernels: every later call on the handle (the next bod_infer, bod_synchronize, ...) is ordered behind
 * the pack and the gather by stream order.
 * `nccl_comm` is the caller's ncclComm_t (created with ncclCommInitRank on this handle's device; librccl.so is opened at run time,
 * the library does not link it); `world` / `rank` are the communicator's size and this process' rank.  nccl_comm == NULL is the
 * single-process form (world must be 1: the block is "gathered" by a device copy).
 * On `root`, `gathered_host` (may be NULL) receives [world][batch][K][W] floats, in rank order, after the copy has been waited
 * for (an event behind it, not the whole stream); *gathered_device (may be NULL) is set to the device copy, valid until the next gather: its contents are complete once
 * bod_collect(slot) has returned (slot >= 0) or after bod_synchronize (slot == -1) -- unless gathered_host was given, in which case
 * the call itself has waited.  Other ranks pass NULL for both (their call returns once the send is enqueued).  A pending slot is
 * NOT released: bod_collect still may. */
int32_t bod_record_width(bod_handle h);
bod_status bod_gather_detections(bod_handle h, int32_t slot, void* nccl_comm, int32_t world, int32_t rank, int32_t root,
                                 float* gathered_host, float** gathered_device);

/* ---- covariance parts (handles created with BOD_PARTS_COVARIANCE in bod_config.covariance_parts; every call below returns BOD_ERR_INVALID_ARG on
 * any other handle) ----
 * Both fusion steps are linear in the member means, so every covariance they store is exactly the sum of three terms: what the
 * fused mean inherits from the epistemic noise (the sample covariance over the MC samples), from the aleatoric noise (the
 * covariance head) and from the Gaussian prior.  Per kept anchor, with lik = (10 A + E) / 11, P = (lik^-1 + I / iso_var)^-1 and
 * the gain G = P lik^-1 = (I + lik / iso_var)^-1:  epi = G (E / 11) G^T,  ale = G (10 A / 11) G^T,  pri = P P / iso_var  (no Gaussian prior: G = I, pri = 0; no
 * covariance head: ale = 0; KITTI: each term rescaled like the covariance).  Per cluster, with P_i the inverse of member i's
 * covariance and F = (sum P_i)^-1:  X_out = 70 F (sum P_i X_i P_i) F.
 * `parts` is always [rows][3][16]: epistemic, aleatoric, prior, each a row-major 4x4 like `covs`.
 * bod_get_posterior_parts: the M rows of image_index, in bod_get_posterior's order (all zero after bod_validation_post).
 * bod_set_posterior_parts: the injection that goes with bod_set_posterior (m = the image's row count).  After bod_set_posterior on
 * an image WITHOUT it, bod_cluster_fuse still runs, and the detection-parts getters of that image return BOD_ERR_NOT_READY.
 * bod_get_detection_parts / _batch: [K][3][16] of one image / [batch][max_detections][3][16], rows as bod_get_detections[_batch].
 * bod_collect_parts: the parts of a bod_infer_async ticket (they are double-buffered with the records and travel to pinned memory
 * with them); it waits for the batch like bod_collect, does not release the slot, and may be called before bod_collect or after it,
 * until the next bod_infer_async that reuses the slot.
 * bod_device_detection_parts: device address of a slot's [batch][max_detections][3][16] array (see bod_device_detections).
 * On these handles bod_record_width() is 1 + 4 + 16 + 2C + 48: bod_gather_detections appends the parts behind the counts. */
bod_status bod_get_posterior_parts(bod_handle h, int32_t image_index, float* parts);
bod_status bod_set_posterior_parts(bod_handle h, int32_t image_index, int32_t m, const float* parts);
bod_status bod_get_detection_parts(bod_handle h, int32_t image_index, float* parts);
bod_status bod_get_detection_parts_batch(bod_handle h, float* parts);
bod_status bod_collect_parts(bod_handle h, int32_t slot, float* parts);
bod_status bod_device_detection_parts(bod_handle h, int32_t slot, void** ptr);

/* ---- class-entropy parts (handles created with BOD_PARTS_CLASS in bod_config.covariance_parts; every call below returns
 * BOD_ERR_INVALID_ARG on any other handle) ----
 * The MC predictive class distribution of an anchor is the mean pbar of its K samples' softmax rows p_n (the distribution the 30
 * Dirichlet counts are drawn from; NOT the reported `score`).  Its entropy splits into
 *   aleatoric = (1/K) sum_n H(p_n)      epistemic = H(pbar) - aleatoric, clamped at 0 (the mutual information of class and weights)
 * with H(p) = -sum_j p_j log p_j (natural log, 0 log 0 = 0).  sum_n H(p_n) is the statistic ent_sum [B,A] the classification head's
 * epilogue writes beside cls_sum: H_n = log(sden) - (sum_j v_j (l_j - mx)) / sden with mx = max_j l_j, v_j = exp(l_j - mx),
 * sden = sum_j v_j; fp32, j and n ascending, no fused multiply-add, log(sden) as the hardware log2 times ln 2; the raw route
 * computes the same bits.
 * Per detection the M cluster members count as M * K samples of one object: pbar_c = (sum_i pbar_i) / M, total = H(pbar_c),
 * aleatoric and epistemic_mc the members' means, epistemic_spatial = max(total - (aleatoric + epistemic_mc), 0) -- the disagreement
 * between the members' mean distributions.
 * bod_get_posterior_class_parts: rows [M][3] = total, aleatoric, epistemic of image_index, in bod_get_posterior's order (all
 * zero after bod_validation_post).
 * bod_get_posterior_mean_probs: the same rows' pbar [M][C], the other half of what bod_set_posterior_class_parts takes (a caller that
 * keeps a posterior on the host and injects it again, as inference_utils.bayes_od_clustering does, reads both).
 * bod_set_posterior_class_parts: the injection that goes with bod_set_posterior (m = the image's row count): mean_probs [m][C]
 * and rows [m][3].  After bod_set_posterior on an image WITHOUT it, bod_cluster_fuse still runs, and the detection getters of that
 * image return BOD_ERR_NOT_READY.
 * bod_get_detection_class_parts / _batch: [K][4] of one image / [batch][max_detections][4] (rows beyond an image's count zero) =
 * total, aleatoric, epistemic_mc, epistemic_spatial; the last three sum to the first.
 * bod_collect_class_parts: the rows of a bod_infer_async ticket, as bod_collect_parts.
 * bod_device_detection_class_parts: device address of a slot's [batch][max_detections][4] array (see bod_device_detections).
 * On these handles bod_record_width() grows by 4: bod_gather_detections appends the four values last. */
bod_status bod_get_posterior_class_parts(bod_handle h, int32_t image_index, float* rows);
bod_status bod_get_posterior_mean_probs(bod_handle h, int32_t image_index, float* mean_probs);
bod_status bod_set_posterior_class_parts(bod_handle h, int32_t image_index, int32_t m, const float* mean_probs, const float* rows);
bod_status bod_get_detection_class_parts(bod_handle h, int32_t image_index, float* rows);
bod_status bod_get_detection_class_parts_batch(bod_handle h, float* rows);
bod_status bod_collect_class_parts(bod_handle h, int32_t slot, float* rows);
bod_status bod_device_detection_class_parts(bod_handle h, int32_t slot, void** ptr);

/* ---- how a cluster becomes a detection: the Bayesian fuse, the NMS pick, or the equal-weight Gaussian mixture ----
 * bod_cluster_fuse multiplies the members' Gaussians and scales the result by 70 (BOD_MERGE_BAYES, the default and the method of
 * bayes_od_clustering).  The two other methods give the other side of that comparison on the same posterior and the same clusters.
 * Membership is the same for all three: the rows i < num_kept whose affinity to centre k is > nms_iou_threshold, the affinity being
 * the IoU of the posterior means evaluated on the fly or the one-shot columns of bod_set_affinity.
 * With n the member count, c the centre's row, mu_i / Sigma_i / counts_i the members' posterior rows and d_i = mu_i - mu_c (the
 * shift by the centre keeps the second moments well conditioned in fp32):
 *   BOD_MERGE_BAYES    today's kernel and results; nothing below is written.
 *   BOD_MERGE_CENTRE   what plain NMS reports, the centre's own posterior:  mean = mu_c, cov = Sigma_c (no factor 70),
 *                      counts = counts_c, scores_j = counts_cj / sum_j counts_cj (summed for j ascending).
 *                      Terms: within = Sigma_c, between = 0, members = n.
 *   BOD_MERGE_MIXTURE  the moment-matched mixture of the members with weight 1/n each:
 *                        dbar = (1/n) sum d_i,  mean = mu_c + dbar,
 *                        within  = (1/n) sum Sigma_i,
 *                        between = (1/n) sum d_i d_i^T - dbar dbar^T   (evaluated on the lower triangle and mirrored; within likewise),
 *                        cov = within + between (no factor 70),
 *                        scores = (1/n) sum counts_i / sum_j(counts_ij),  counts = (1/n) sum counts_i.
 *                      `between` is the spread of the members' means: the "output redundancy" spatial uncertainty.
 *   n == 0 (only under a caller's affinity whose column excludes every row, the centre included): both new methods return the
 *   centre's row as BOD_MERGE_CENTRE does, with members = 0.  (BOD_MERGE_BAYES divides by zero there, as before.)
 * fp32 throughout, no fused multiply-add; the sums over the members are re-associated (256 threads, wave butterflies).
 * bod_set_merge_method: takes effect with the next bod_cluster_fuse, bod_infer or bod_infer_async enqueued (so it also serves
 * statistics handles: bod_stat_posterior -> bod_nms -> bod_cluster_fuse).  BOD_ERR_INVALID_ARG, with a message, for an unknown
 * value, for a training = 1 handle, and for a non-default method on a handle whose covariance_parts is non-zero: the covariance and
 * class-entropy parts kernels are defined for the Bayesian fuse only, and extending them is out of scope.  After a refusal the
 * handle's method is unchanged.  The first non-default call allocates the term buffers (2 slots x batch x max_detections x 33 words).
 * bod_get_detection_merge_terms / _batch: within [K][16], between [K][16], members [K] of one image / the same with
 * [batch][max_detections] in front (rows beyond an image's count zero), rows as bod_get_detections[_batch]; NULLs skipped.
 * _batch's slot = -1 is the slot synchronous calls use; slot 0 / 1 is a bod_infer_async ticket: the call waits for that batch as
 * bod_collect does, does not release the slot, and may come before bod_collect or after it, until the next bod_infer_async that
 * reuses the slot.  BOD_ERR_NOT_READY when the slot's last cluster stage ran as BOD_MERGE_BAYES (or none has run).
 * bod_device_detection_merge_terms: device addresses {within, between, members} of a slot (see bod_device_detections); NULLs
 * before the first non-default bod_set_merge_method.
 * The five detection arrays, bod_record_width and bod_gather_detections do not know the method: the terms are not in the records. */
enum { BOD_MERGE_BAYES = 0, BOD_MERGE_CENTRE = 1, BOD_MERGE_MIXTURE = 2 };
bod_status bod_set_merge_method(bod_handle h, int32_t method);
bod_status bod_get_merge_method(bod_handle h, int32_t* method);
bod_status bod_get_detection_merge_terms(bod_handle h, int32_t image_index, float* within, float* between, int32_t* members);
bod_status bod_get_detection_merge_terms_batch(bod_handle h, int32_t slot, float* within, float* between, int32_t* members);
bod_status bod_device_detection_merge_terms(bod_handle h, int32_t slot, void** ptrs3);

/* ---- black-box MC dropout: per-sample NMS, then the detections merged ----
 * The baseline BayesOD is compared against: every stochastic pass goes through the detector's ordinary post-processing on its own,
 * the N detection sets of an image are grouped by overlap, and each group becomes one detection with the sample mean and the sample
 * covariance of its members.  Kmax = nms_max_output_size, theta = affinity_threshold (0: nms_iou_threshold).
 * Stage 1 (bod_blackbox_samples), for every image b and sample n -- bod_validation_post + bod_nms applied to sample n:
 *   1. softmax of the sample's class row; anchors whose arg-max is background (first maximum wins) are dropped; the rest are ranked
 *      by their top softmax score, their boxes decoded from the sample's own deltas;
 *   2. nms_kernel with the handle's nms_* settings, in network coordinates: up to Kmax indices;
 *   3. every selected candidate becomes a sample detection: score[C] = the softmax row (not the decayed NMS score), mean[4] (v,u,h,w),
 *      anchor_index, cov[16] = the sample's own aleatoric matrix -- L D L^T with L = inv(unit_lower(params)), D = exp(diag) when
 *      use_full_covar, else D; zeros when has_covar_head == 0 (bod_posterior's arithmetic on ONE sample's parameters);
 *   4. the KITTI rescale of bod_posterior (S mu, S Sigma S^T; a ragged upload's per-frame factors included) here, after the NMS;
 *   5. detections whose top score is below min_score are discarded; the others keep their order.
 * Stage 2 (bod_blackbox_merge), per image.  The pool holds the image's sample detections at pooled index n * Kmax + rank; the corners
 * of a detection are vuhw_to_vuvu of its (rescaled) mean.  Greedy:
 *   1. the unassigned detection with the highest top score becomes a centre c; ties go to the lower pooled index;
 *   2. its members are c itself (whatever its self-IoU under the reference's +1 formula) and every unassigned i with
 *      bbox_iou_vuvu(corners_c, corners_i) > theta (bod_cluster_fuse's affinity); all of them become assigned;
 *   3. with n members and d_i = mu_i - mu_c:  dbar = (1/n) sum d_i,  mean = mu_c + dbar,  within = (1/n) sum cov_i,
 *      between = (sum d_i d_i^T - n dbar dbar^T) / (n - 1) for n >= 2 -- the unbiased sample covariance, centred as in
 *      BOD_MERGE_MIXTURE -- and exactly 0 for n = 1,  cov = within + between (no factor 70, no 10:1 mix),
 *      counts = sum score_i,  scores = counts / n,  members = n;
 *   4. a cluster with n < min_members emits nothing; its members stay consumed;
 *   5. stop after Kmax emitted clusters or when the pool is empty; detections appear in emission order.
 * Clustering is class-agnostic.  fp32, no fused multiply-add; the sums over the members are re-associated (256 threads, wave
 * butterflies), deterministically.
 * bod_set_uncertainty_method(h, BOD_METHOD_BLACK_BOX, opt): opt == NULL means {0, 1, 0}.  The first switch allocates the stage's
 * buffers (B * N virtual images' worth of keep flags, top scores, block counts, ranking, corners, anchor indices and nms_kernel's
 * work arrays; the sample detections; the pool's work arrays; the merge-term buffers).  BOD_ERR_INVALID_ARG, with the reason, for
 * an unknown method, a training handle, a statistics handle, covariance_parts != 0, a merge method other than BOD_MERGE_BAYES,
 * min_members < 1, a min_score or affinity_threshold that is not finite or is negative, reserved != 0; the handle's method is
 * unchanged then.  While black box is on, bod_set_merge_method refuses a non-default method.  BOD_METHOD_BAYES_OD brings back the
 * default path: plans, buffers written and result bytes as on a handle that was never switched.
 * In black-box mode bod_infer / bod_infer_async run the forward with the per-sample head outputs, then the two stages into the
 * ticket's record slot, and mc_samples = 1 is allowed (the sampling-free baseline: members = 1, between = 0).  bod_collect,
 * bod_get_detections[_batch], bod_gather_detections and bod_get_detection_merge_terms[_batch] serve the result as they stand.
 * The stage entries work in either mode: bod_blackbox_samples needs the anchors and a forward / bod_set_raw
 * (BOD_ERR_NOT_READY), bod_blackbox_merge needs sample detections newer than the last forward / bod_set_raw: bod_blackbox_samples, or
 * bod_set_sample_detections (stage-level tests), which replaces ONE (image, sample) and leaves the others as they are -- empty on a
 * handle whose stage 1 never ran.  The stage entries need the buffers: BOD_ERR_NOT_READY before the first switch to black box.
 * bod_get_sample_detections: count, then anchor_index [count], scores [count][C], means [count][4], covs [count][16]; NULLs skipped. */
enum { BOD_METHOD_BAYES_OD = 0, BOD_METHOD_BLACK_BOX = 1 };
typedef struct bod_blackbox_options {   /* 16 bytes */
    float   min_score;           /* stage 1, rule 5; default 0 */
    int32_t min_members;         /* stage 2, rule 4; >= 1, default 1 */
    float   affinity_threshold;  /* theta; 0 = nms_iou_threshold */
    int32_t reserved;            /* 0 */
} bod_blackbox_options;
bod_status bod_set_uncertainty_method(bod_handle h, int32_t method, const bod_blackbox_options* options);
bod_status bod_get_uncertainty_method(bod_handle h, int32_t* method);
bod_status bod_blackbox_samples(bod_handle h);
bod_status bod_blackbox_merge(bod_handle h);
bod_status bod_get_sample_detections(bod_handle h, int32_t image_index, int32_t sample_index, int32_t* count, int32_t* anchor_index,
                                     float* scores, float* means, float* covs);
bod_status bod_set_sample_detections(bod_handle h, int32_t image_index, int32_t sample_index, int32_t count,
                                     const int32_t* anchor_index, const float* scores, const float* means, const float* covs);

/* What the handle's plan looks like (tests / bench report it; nothing on the hot path reads it).  info8[0] = 1 when the MC
 * statistics are reduced inside the last tower layers' tiles (no [B,N,A,.] tensors on the bod_infer path), [1] = 1 when the 1x1
 * head output convs are fused into the last tower layers' epilogues, [2] = 1 when the per-sample tower layers run on the
 * activation-row-reuse kernel, [3] = 1 when the fan-out layer does, [4] = number of ops of the forward plan, [5] = number of
 * backbone / FPN 3x3 layers planned on the row-reuse kernel, [6] = 1 / 2 when the head towers run the f16mx / f16mx4 arithmetic
 * (BOD_PRECISION_F16MX / BOD_PRECISION_F16MX4), [7] = 1 when the box / covariance heads' last layers run over the pixels with a kept
 * anchor only (the sparse tail; BOD_SPARSE_TAIL=0: dense). */
bod_status bod_plan_info(bod_handle h, int32_t* info8);
/* bod_plan_info with more slots: fills info[0 .. min(n, 11) - 1]; [0..7] as above, [8] = 1 when box layer 1 and covariance layer 2
 * also run only over the 3x3 dilation of the sparse tail's pixels (the sparse halo; BOD_SPARSE_HALO=0: dense, as before), [9] = rows
 * per tile of the sparse tail's launch: 192, or 256 with BOD_SPARSE_TAIL_ROWS=256 (0 without a sparse tail), [10] = the last block of
 * ResNet stages 2-4 on the pixels the next stage reads: 0 whole planes (training handles, BOD_STAGE_END_PIXELS=0), 1 the `2c` layers,
 * 2 the `2c` layers and stage 4's `2b`. */
bod_status bod_plan_info_n(bod_handle h, int32_t* info, int32_t n);

/* ---- mergeable MC statistics (handles created with mc_statistics = 1): ensembles of several weight sets, more samples than one
 * forward holds, sample sharding at 34 floats per anchor instead of 22 per anchor AND sample.  Every call below returns
 * BOD_ERR_INVALID_ARG for a handle without mc_statistics and BOD_ERR_NOT_READY for a stage-order violation.
 *
 * The statistics record of `samples` MC samples, fp32, per image b and anchor a (what the last tower layers' epilogues reduce
 * over the samples of one forward, and what bayes_od_inference needs of them, inference_utils.py:31-60, :220-244):
 *   cls_sum     [B,A,C]   sum over the samples of softmax(class logits)
 *   box_moments [B,A,16]  mean[4] of the decoded boxes (v,u,h,w); the lower triangle, row-major, of the co-moment sums
 *                         M2_ij = sum (x_i - mean_i)(x_j - mean_j): (0,0) (1,0) (1,1) (2,0) (2,1) (2,2) (3,0) .. (3,3) [10]; 0; 0
 *   cov_sum     [B,A,10]  sum over the samples of the raw covariance parameters (pre fill_triangular); absent (NULL) without
 *                         the covariance head
 * Two records of ka and kb samples merge (Chan's pairwise update; fp32, no fused multiply-add, in this order):
 *   cls_sum = a + b;  cov_sum = a + b;  d = mean_b - mean_a;  w = kb / (ka + kb);  mean = mean_a + d * w;
 *   M2_ij = (M2a_ij + M2b_ij) + (d_i * d_j) * (ka * w);  the two pad floats stay 0;  ka = 0 copies b.
 * The merge uses no atomics: the same calls in the same order give the same bits. */
/* K = 0: the accumulator is empty (its contents are not read by the next merge). */
bod_status bod_stat_reset(bod_handle h);
/* bod_forward for this handle's n = mc_samples samples with the ABSOLUTE sample indices sample_base .. sample_base + n - 1 in the
 * dropout streams (mc_sample_base of the call; the handle's own value is untouched), reduced to a statistics record -- inside the
 * last tower layers' tiles where the plan aggregates, else by a kernel over the raw head outputs (same operations in the same
 * order: identical bits) -- and folded into the accumulator: K += n.  One stream, no host round trip.  sample_base + n must not
 * exceed mc_ensemble_size when that is set.  Needs the weights and the anchors (the boxes are decoded). */
bod_status bod_stat_forward(bod_handle h, const float* images, int32_t images_on_device, uint64_t seed, uint32_t first_image_id,
                            int32_t sample_base);
/* dst's accumulator (+)= src's; src is unchanged.  Both handles on the same device with the same batch, anchors, classes and
 * covariance head (BOD_ERR_INVALID_ARG names the field).  dst's stream is ordered behind src's and src's next write behind the
 * merge.  An empty src (K = 0) is a no-op. */
bod_status bod_stat_merge_from(bod_handle dst, bod_handle src);
/* The same from device pointers {cls_sum, box_moments, cov_sum or NULL} of a record of `samples` >= 1 samples (buffers that
 * arrived through a collective; 16-byte aligned).  The caller orders its writes before the call as for bod_device_raw. */
bod_status bod_stat_merge(bod_handle h, const void* const* ptrs3, int32_t samples);
/* Device addresses of the accumulator (order as above; [2] = NULL without the covariance head) and K, for zero-copy exchange.
 * Valid until bod_destroy; the contents are complete after bod_synchronize.  Either output may be NULL. */
bod_status bod_stat_device(bod_handle h, void** ptrs3, int32_t* samples);
/* Host copies of the accumulator out and in (stage-level test hooks, like bod_get_raw / bod_set_raw).  NULL arrays are skipped;
 * bod_stat_set sets K = samples >= 0. */
bod_status bod_stat_get(bod_handle h, float* cls_sum, float* box_moments, float* cov_sum, int32_t* samples);
bod_status bod_stat_set(bod_handle h, const float* cls_sum, const float* box_moments, const float* cov_sum, int32_t samples);
/* bod_posterior on the accumulator with N = K (BOD_ERR_NOT_READY for K < 2: the sample covariance divides by N - 1); bod_nms,
 * bod_cluster_fuse, bod_get_posterior and bod_get_detections* follow as after bod_posterior.  Needs the anchors. */
bod_status bod_stat_posterior(bod_handle h, uint64_t seed, uint32_t first_image_id);

/* ---- test-time views of a statistics handle: the same frames mirrored left-right, counted in the SAME accumulator.  A forward
 * of the mirrored frames yields the record of the mirrored anchors; the fold reads it through the mirror map, which is exact in
 * fp32.  With K = anchors_per_location and the level table of bod_sizes, anchor a = off_l + (y * W_l + x) * K + k has the partner
 * a' = off_l + (y * W_l + (W_l - 1 - x)) * K + k, and the result at a' from the record at a is
 *   cls_sum      copied
 *   box_moments  mean (v, u, h, w) -> (v, float(image_w - 1) - u, h, w) (bod_augment_boxes' flip: x' = (w-1) - x); M2 entries with
 *                exactly one index equal to 1 -- stored positions 1, 4 and 7 -- negated; the rest and the pads copied
 *   cov_sum      parameters 8, 6 and 2 (fill_triangular's (1,0), (2,1), (3,1)) negated: Sigma -> S Sigma S^T, S = diag(1,-1,1,1)
 * and the merge formula above follows, operation for operation.  A mirrored view needs mirror-symmetric anchors: anchors[a']
 * must equal (v, float(image_w) - u, h, w) of anchors[a] bit for bit, which for the FPN anchor grid means image_w is a multiple of
 * 2^max_level (512x512, 720x1280, 384x1280; not KITTI's 384x1248, whose levels 6 and 7 overhang the frame).  Checked on the host
 * on the first mirrored call after bod_set_anchors; BOD_ERR_INVALID_ARG names the first level that fails. */
enum { BOD_VIEW_IDENTITY = 0, BOD_VIEW_HFLIP = 1 };
/* bod_stat_forward of a view of the frames.  view = BOD_VIEW_IDENTITY is bod_stat_forward.  BOD_VIEW_HFLIP mirrors the network-input
 * frames (host floats, either image buffer, a ragged upload: its per-frame factors stay in force) into a scratch buffer of the
 * handle -- the source is not modified --, runs the same forward with the same seed / sample_base semantics, reduces to a record
 * and folds it through the mirror map: K += n.  One stream, no host round trip.  The dropout streams do not know about views:
 * give the mirrored pass a sample_base of its own for independent masks.  BOD_ERR_INVALID_ARG for any other view and for
 * anchors that are not mirror-symmetric; after a refusal the accumulator and K are as before. */
bod_status bod_stat_forward_view(bod_handle h, const float* images, int32_t images_on_device, uint64_t seed, uint32_t first_image_id,
                                 int32_t sample_base, int32_t view);
/* bod_stat_merge of a record that is still in the frame of `view` (it arrived from a rank that ran mirrored forwards and did not
 * fold them).  BOD_VIEW_HFLIP needs the anchors (BOD_ERR_NOT_READY).  bod_stat_merge_from has no view: un-mirror where the
 * forward ran. */
bod_status bod_stat_merge_view(bod_handle h, const void* const* ptrs3, int32_t samples, int32_t view);

/* ---- the record's fourth array on BOD_PARTS_CLASS statistics handles: ent_sum [B,A], the sum over the samples of the entropy of
 * softmax(class logits).  Two records merge as ent_sum = a + b whatever their sample counts; the mirror map copies the value
 * from the partner anchor.  bod_stat_forward[_view] and bod_stat_merge_from fold it with the other three (bod_stat_merge_from
 * refuses a src without ent_sum when dst carries it: BOD_ERR_INVALID_ARG names the field).  The three-array entry points keep
 * their signatures; on these handles each of them is FOLLOWED by its entropy call, which brings ent_sum level with K:
 *   bod_stat_merge[_view]  then  bod_stat_merge_entropy(h, device pointer (16-byte aligned), view)
 *   bod_stat_set           then  bod_stat_set_entropy(h, host array)
 * Until then ent_sum is behind the record and bod_stat_posterior, a further fold and bod_stat_get_entropy return
 * BOD_ERR_NOT_READY.  bod_stat_device_entropy: device address of the accumulator's ent_sum, valid until bod_destroy. */
bod_status bod_stat_get_entropy(bod_handle h, float* ent_sum);
bod_status bod_stat_set_entropy(bod_handle h, const float* ent_sum);
bod_status bod_stat_device_entropy(bod_handle h, void** ptr);
bod_status bod_stat_merge_entropy(bod_handle h, const void* ent_sum, int32_t view);

/* ---- acquisition scores of a statistics handle: the accumulator of K >= 2 samples reduced, in one streaming pass
 * on the handle's stream, to a few numbers per frame for ranking unlabeled frames by the model's uncertainty (active learning).
 * Per anchor, fp32, with C classes of which the last is the background:
 *   bad     any non-finite float in the anchor's record; a bad anchor is counted in n_bad and enters nothing else
 *   W       the frame's foreground set: cls_sum[C-1] <= (float)((1.0 - (double)min_foreground) * K)
 *   H       -sum_j p_j ln p_j with p_j = cls_sum[j] / K (p_j <= 0 contributes 0);  Ha = ent_sum / K;  MI = max(H - Ha, 0)
 *   fg      1 - cls_sum[C-1] / K
 *   e_box   (M2_00 + M2_11 + M2_22 + M2_33) / (K - 1) / (h^2 + w^2) with h, w = box_moments[2], [3]: the box's epistemic spread
 *   lda     (x[0] + x[4] + x[5] + x[9]) / K, x the cov_sum row: the log-determinant of the aleatoric covariance
 *   cls     arg max_{j < C-1} cls_sum[j], the first maximum
 * frame_scores [B,12], fp64: n_fg = |W|, n_bad, entropy_mean (H over W), aleatoric_entropy_mean (Ha over W), mi_mean, mi_max (MI over
 * W), mi_soft (sum fg MI / sum fg over every good anchor), mi_topk (mean of the min(top_k, n_fg) largest MI of W), box_epistemic_mean,
 * box_epistemic_max (e_box over W), box_aleatoric_mean, box_aleatoric_max (lda over W).  per_class [B,C-1,3], fp64 (NULL: skipped):
 * for class j the number of W anchors with cls = j, their largest MI and their largest e_box.  A mean or maximum over an empty set
 * is NaN; columns 3-7 and per_class' MI are NaN without BOD_PARTS_CLASS (no ent_sum), columns 10-11 without the covariance head.
 * No atomics: the same record gives the same bits, and a frame's row depends on that frame's record alone.
 * The call is ordered behind whatever wrote the accumulator, copies the outputs to the host and returns when they are complete.
 * The accumulator, K and every posterior / record buffer are left as they are: bod_stat_posterior may follow, precede or not happen.
 * BOD_ERR_INVALID_ARG: no mc_statistics, min_foreground outside [0, 1], top_k outside 1..1024, non-zero reserved.
 * BOD_ERR_NOT_READY: K < 2, ent_sum behind the record.  options = NULL: min_foreground 0.05, top_k 16. */
typedef struct bod_acquisition_options {   /* 16 bytes */
    float min_foreground;
    int32_t top_k;
    int32_t reserved[2];
} bod_acquisition_options;
bod_status bod_stat_acquisition(bod_handle h, const bod_acquisition_options* options, double* frame_scores, double* per_class);
/* Test hook: the [B,A] scratch of the last bod_stat_acquisition -- every anchor's MI, NaN outside W, for bad anchors and without
 * ent_sum.  BOD_ERR_NOT_READY before any bod_stat_acquisition (the scratch is allocated by the first one). */
bod_status bod_stat_acquisition_map(bod_handle h, float* mi);

#ifdef __cplusplus
}
#endif
#endif /* BAYESOD_H */

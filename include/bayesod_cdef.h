/* GENERATED from include/bayesod.h by bayes_od_rc_amd.build.write_cdef(): the same declarations without
 * comments / preprocessor lines, for ffi.cdef(open('include/bayesod_cdef.h').read()).  Do not edit. */
typedef struct bod_context* bod_handle;
typedef enum {
    BOD_OK = 0,
    BOD_ERR_INVALID_ARG = 1,
    BOD_ERR_HIP = 2,
    BOD_ERR_OOM = 3,
    BOD_ERR_NOT_READY = 4,
    BOD_ERR_NO_DEVICE = 5
} bod_status;
enum { BOD_RANK_SCORE = 0, BOD_RANK_JOINT_ENTROPY = 1 };
enum { BOD_NMS_VARIANT_A = 0, BOD_NMS_VARIANT_B = 1 };
enum { BOD_HEAD_CLS = 0, BOD_HEAD_REG = 1, BOD_HEAD_COV = 2 };
enum { BOD_PRECISION_BF16 = 0, BOD_PRECISION_FP32 = 1, BOD_PRECISION_BF16X3 = 2, BOD_PRECISION_F16MX = 3, BOD_PRECISION_F16MX4 = 4 };
typedef struct {
    int32_t device;
    int32_t image_h, image_w;
    int32_t batch;
    int32_t mc_samples;
    int32_t num_classes;
    int32_t anchors_per_location;
    int32_t min_level, max_level;
    float   dropout_rate;
    int32_t use_full_covar;
    int32_t dirichlet_non_informative;
    int32_t gaussian_isotropic;
    float   isotropic_variance;
    int32_t ranking_method;
    int32_t nms_max_output_size;
    float   nms_iou_threshold;
    float   nms_soft_sigma;
    int32_t nms_variant;
    int32_t num_categorical_draws;
    int32_t has_covar_head;
    float   kitti_scale_h, kitti_scale_w;
    int32_t precision;
    int32_t mc_sample_base;
    int32_t mc_ensemble_size;
    int32_t training;
    int32_t backbone_depth;
    int32_t pipeline_overlap;
    int32_t mc_statistics;
    union {
        int32_t covariance_parts;
        int32_t reserved[1];
    };
} bod_config;
enum { BOD_PARTS_COVARIANCE = 1, BOD_PARTS_CLASS = 2 };
typedef struct {
    int32_t num_pixels;
    int32_t num_anchors;
    int32_t level_h[8], level_w[8];
    int32_t num_levels;
    int32_t max_detections;
    int64_t device_bytes;
} bod_sizes;
const char* bod_version(void);
const char* bod_last_error(bod_handle h);
bod_status bod_create(const bod_config* cfg, bod_handle* out);
bod_status bod_destroy(bod_handle h);
bod_status bod_query_sizes(bod_handle h, bod_sizes* out);
bod_status bod_update_config(bod_handle h, const bod_config* cfg);
bod_status bod_load_weight(bod_handle h, const char* name, int32_t kind,
                           const int64_t* shape, int32_t ndim, const float* data);
bod_status bod_finalize_weights(bod_handle h);
bod_status bod_set_anchors(bod_handle h, const float* anchors_vuhw, int32_t num_anchors);
bod_status bod_forward(bod_handle h, const float* images, int32_t images_on_device,
                       uint64_t seed, uint32_t first_image_id);
bod_status bod_get_raw(bod_handle h, float* cls, float* box, float* covar_params);
bod_status bod_set_raw(bod_handle h, const float* cls, const float* box, const float* covar_params);
bod_status bod_get_pyramid(bod_handle h, int32_t level_index, float* out);
bod_status bod_posterior(bod_handle h, uint64_t seed, uint32_t first_image_id);
bod_status bod_validation_post(bod_handle h);
bod_status bod_get_num_kept(bod_handle h, int32_t* num_kept);
bod_status bod_get_posterior(bod_handle h, int32_t image_index, float* counts, float* score,
                             float* means, float* covs, float* ranking, int32_t* anchor_index);
bod_status bod_set_posterior(bod_handle h, int32_t image_index, int32_t m, const float* counts,
                             const float* means, const float* covs, const float* ranking);
bod_status bod_nms(bod_handle h);
bod_status bod_get_nms(bod_handle h, int32_t image_index, int32_t* indices, int32_t* num_selected);
bod_status bod_set_nms(bod_handle h, int32_t image_index, const int32_t* indices, int32_t num_selected);
bod_status bod_get_iou_matrix(bod_handle h, int32_t image_index, float* iou);
bod_status bod_cluster_fuse(bod_handle h);
bod_status bod_set_affinity(bod_handle h, int32_t image_index, const float* centre_columns, int32_t k, int32_t m);
bod_status bod_get_detections(bod_handle h, int32_t image_index, int32_t* num_detections,
                              float* scores, float* means, float* covs, float* counts);
bod_status bod_get_detections_batch(bod_handle h, int32_t* num_detections, float* scores, float* means,
                                    float* covs, float* counts);
bod_status bod_device_detections(bod_handle h, int32_t slot, void** ptrs5);
bod_status bod_device_raw(bod_handle h, void** ptrs3, int32_t mark_ready);
bod_status bod_infer(bod_handle h, const float* images, int32_t images_on_device,
                     uint64_t seed, uint32_t first_image_id);
bod_status bod_infer_async(bod_handle h, const float* images, int32_t images_on_device,
                           uint64_t seed, uint32_t first_image_id, int32_t* slot);
bod_status bod_collect(bod_handle h, int32_t slot, int32_t* num_detections, float* scores,
                       float* means, float* covs, float* counts);
bod_status bod_upload_images(bod_handle h, const float* host_images);
bod_status bod_upload_frames_u8(bod_handle h, const uint8_t* rgb, int32_t src_h, int32_t src_w,
                                const float* rgb_means, int32_t aspect_resize);
bod_status bod_upload_frames_u8_async(bod_handle h, const uint8_t* rgb, int32_t src_h, int32_t src_w,
                                      const float* rgb_means, int32_t aspect_resize, int32_t buffer);
bod_status bod_upload_frames_u8_ragged(bod_handle h, const uint8_t* rgb_packed, const int32_t* src_hw,
                                       const float* rgb_means, int32_t aspect_resize);
bod_status bod_upload_frames_u8_ragged_async(bod_handle h, const uint8_t* rgb_packed, const int32_t* src_hw,
                                             const float* rgb_means, int32_t aspect_resize, int32_t buffer);
typedef struct bod_augment {
    int32_t flip;
    float   scale;
    float   off_y, off_x;
    float   gain, bias;
} bod_augment;
bod_status bod_upload_frames_u8_augmented(bod_handle h, const uint8_t* rgb_packed, const int32_t* src_hw,
                                          const float* rgb_means, int32_t aspect_resize, const bod_augment* aug);
bod_status bod_upload_frames_u8_augmented_async(bod_handle h, const uint8_t* rgb_packed, const int32_t* src_hw,
                                                const float* rgb_means, int32_t aspect_resize, const bod_augment* aug,
                                                int32_t buffer);
bod_status bod_augment_boxes(int32_t B, const int32_t* src_hw, int32_t net_h, int32_t net_w, int32_t aspect_resize,
                             const bod_augment* aug, const int32_t* num_gt, const float* gt_boxes_vuvu_src,
                             const float* gt_classes, int32_t C, float min_visible,
                             int32_t* num_out, float* boxes_out, float* classes_out);
struct bod_jpeg_info {
    int32_t width, height, components;
    int32_t h_samp, v_samp;
    int32_t restart_interval;
    int32_t supported;
    int64_t coef_count;
};
bod_status bod_jpeg_info(const uint8_t* data, int64_t len, struct bod_jpeg_info* out);
bod_status bod_jpeg_entropy_decode(const uint8_t* data, int64_t len, int16_t* coefs, int64_t coef_capacity,
                                   uint16_t* quant3x64);
bod_status bod_jpeg_decode_rgb(int32_t device, int32_t n, const uint8_t* const* data, const int64_t* len,
                               int32_t threads, uint8_t* rgb_packed, int64_t rgb_capacity, int32_t* src_hw);
bod_status bod_upload_frames_jpeg(bod_handle h, const uint8_t* const* data, const int64_t* len,
                                  const float* rgb_means, int32_t aspect_resize, const bod_augment* aug,
                                  int32_t threads, int32_t* src_hw_out);
bod_status bod_upload_frames_jpeg_async(bod_handle h, const uint8_t* const* data, const int64_t* len,
                                        const float* rgb_means, int32_t aspect_resize, const bod_augment* aug,
                                        int32_t threads, int32_t* src_hw_out, int32_t buffer);
enum { BOD_CORRUPT_NONE = 0, BOD_CORRUPT_LUT = 1, BOD_CORRUPT_CONTRAST = 2, BOD_CORRUPT_IMPULSE_NOISE = 3,
       BOD_CORRUPT_GAUSSIAN_NOISE = 4, BOD_CORRUPT_CONV2D = 5, BOD_CORRUPT_PIXELATE = 6, BOD_CORRUPT_JPEG = 7, BOD_CORRUPT_FOG = 8 };
typedef struct bod_corrupt_op {
    int32_t  kind;
    float    f0;
    uint32_t u0;
    int32_t  tap_offset;
    int32_t  ksize;
    int32_t  table;
    int32_t  reserved[2];
} bod_corrupt_op;
bod_status bod_corrupt_frames_u8(int32_t device, int32_t n, const uint8_t* rgb_packed_in, const int32_t* src_hw,
                                 const bod_corrupt_op* ops, int32_t ops_per_frame, const uint32_t* frame_ids,
                                 const uint16_t* taps, int32_t n_taps, const uint8_t* luts, int32_t n_luts,
                                 const uint16_t* qtables, int32_t n_qtables, uint64_t seed, uint8_t* rgb_packed_out);
bod_status bod_set_upload_corruption(bod_handle h, const bod_corrupt_op* ops, int32_t ops_per_frame, const uint32_t* frame_ids,
                                     const uint16_t* taps, int32_t n_taps, const uint8_t* luts, int32_t n_luts,
                                     const uint16_t* qtables, int32_t n_qtables, uint64_t seed);
enum { BOD_RENDER_OVERLAY = 0, BOD_RENDER_HEAT = 1 };
typedef struct bod_render_options {
    int32_t view;
    int32_t line_width;
    int32_t labels;
    float   r2;
    int32_t reserved[4];
} bod_render_options;
bod_status bod_render_frames_u8(int32_t device, int32_t n, const uint8_t* rgb_packed_in, const int32_t* src_hw,
                                const int32_t* num_det, const int32_t* det_boxes, const float* det_corner_covs,
                                const uint8_t* det_colors, const uint8_t* det_text, const int32_t* num_gt,
                                const int32_t* gt_boxes, const bod_render_options* opt, uint8_t* rgb_packed_out,
                                int32_t* skipped_ellipses);
bod_status bod_render_font(uint8_t* glyph_rows, int32_t* count);
struct bod_png_info {
    int32_t width, height, bit_depth, color_type;
    int32_t channels;
    int32_t interlace;
    int32_t supported;
    int64_t raw_bytes;
};
bod_status bod_png_info(const uint8_t* data, int64_t len, struct bod_png_info* out);
bod_status bod_png_inflate(const uint8_t* data, int64_t len, uint8_t* raw, int64_t raw_capacity);
bod_status bod_png_decode_rgb(int32_t device, int32_t n, const uint8_t* const* data, const int64_t* len,
                              int32_t threads, uint8_t* rgb_packed, int64_t rgb_capacity, int32_t* src_hw);
bod_status bod_bench_png_decode(int32_t device, int32_t n, const uint8_t* const* data, const int64_t* len,
                                int32_t threads, int32_t iters, double* host_ms, double* kernel_ms);
bod_status bod_upload_frames_png(bod_handle h, const uint8_t* const* data, const int64_t* len,
                                 const float* rgb_means, int32_t aspect_resize, const bod_augment* aug,
                                 int32_t threads, int32_t* src_hw_out);
bod_status bod_upload_frames_png_async(bod_handle h, const uint8_t* const* data, const int64_t* len,
                                       const float* rgb_means, int32_t aspect_resize, const bod_augment* aug,
                                       int32_t threads, int32_t* src_hw_out, int32_t buffer);
const float* bod_device_images_buffer(bod_handle h, int32_t buffer);
const float* bod_device_images(bod_handle h);
bod_status bod_synchronize(bod_handle h);
bod_status bod_stage_conv(int32_t device, const float* x, int32_t B, int32_t H, int32_t W, int32_t Cin,
                          const float* w, const float* bias, int32_t KH, int32_t KW, int32_t Cout,
                          int32_t stride, int32_t same_padding, int32_t relu, const float* residual,
                          float dropout_rate, uint64_t seed, int32_t layer_id, uint32_t image_id,
                          int32_t round_output_bf16, int32_t precision, float* out);
bod_status bod_stage_conv_wgrad(int32_t device, const float* x, int32_t B, int32_t H, int32_t W, int32_t Cin,
                                const float* dy, int32_t KH, int32_t KW, int32_t Cout, int32_t stride,
                                int32_t same_padding, int32_t ksplit, float* dw, float* db);
bod_status bod_stage_act_backward(int32_t device, int32_t precision, const float* dout, const float* out_act, const float* dout_relu,
                                  int64_t out_elems, const int32_t* out_off, const int32_t* res_off, int32_t M, int32_t cout,
                                  int32_t cout_pad, int32_t out_cstride, int32_t res_cstride, float scale, int32_t Kpad, float* dres,
                                  int64_t dres_elems, float* dz, float* dzp, float* dzt, int32_t* wrote_transpose);
enum { BOD_DGRAD_FLIP = 0, BOD_DGRAD_ROWS = 1, BOD_DGRAD_COL2IM = 2 };
bod_status bod_stage_conv_dgrad(int32_t device, int32_t route, const float* dz, const float* w, int32_t B, int32_t H, int32_t W,
                                int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t same_padding,
                                int32_t ksplit, int32_t groups, float* din, int32_t* info2);
bod_status bod_stage_stem_pool_backward(int32_t device, int32_t precision, const float* stem_out, const float* dpool, int64_t dpool_elems,
                                        int32_t B, int32_t ih, int32_t iw, float* dz);
enum { BOD_STEM_AUTO = 0, BOD_STEM_F32_POOL_F32 = 1, BOD_STEM_F32_POOL_SPLIT = 2, BOD_STEM_SEG64_POOL = 3, BOD_STEM_ROW_POOL = 4,
       BOD_STEM_FUSED_8 = 5, BOD_STEM_FUSED_4 = 6, BOD_STEM_FUSED_SPLIT = 7 };
bod_status bod_stage_stem(int32_t device, int32_t form, int32_t precision, const float* images, int32_t B, int32_t H, int32_t W,
                          const float* w, const float* bias, int32_t misalign, int32_t n_cu, float sentinel, float* stem_out,
                          float* pooled, int32_t* form_ran);
bod_status bod_stage_stem_pool(int32_t device, int32_t mode, const float* stem, int32_t B, int32_t ih, int32_t iw, float sentinel,
                               float* pooled);
typedef struct bod_fold_layer {
    const float* kernel; const float* bias; const float* gamma; const float* beta; const float* mean; const float* var;
    int32_t taps, cin, cout, cout_pad;
    uint16_t* w_fwd; uint16_t* w_bwd; uint16_t* w_flip; float* w_fwd32; float* b_fwd;
} bod_fold_layer;
bod_status bod_stage_fold_pack(int32_t device, int32_t count, const bod_fold_layer* layers);
bod_status bod_train_step(bod_handle h, const float* images, int32_t images_on_device, const float* cls_targets,
                          const float* box_targets, const uint8_t* positive_mask, const uint8_t* negative_mask,
                          uint64_t seed, uint32_t first_image_id, int32_t reg_kind, float label_smoothing,
                          float w_cls, float w_reg, float l2_rate, float learning_rate, int32_t apply_update,
                          double* out6);
bod_status bod_train_step_boxes(bod_handle h, const float* images, int32_t images_on_device, const int32_t* num_gt,
                                const float* gt_boxes_vuvu, const float* gt_classes, float min_positive_iou,
                                float max_negative_iou, uint64_t seed, uint32_t first_image_id, int32_t reg_kind,
                                float label_smoothing, float w_cls, float w_reg, float l2_rate, float learning_rate,
                                int32_t apply_update, double* out6);
bod_status bod_train_get_targets(bod_handle h, float* cls_targets, float* box_targets, uint8_t* positive_mask,
                                 uint8_t* negative_mask);
bod_status bod_train_gradients(bod_handle h, void** device_ptr, int64_t* count);
bod_status bod_train_apply(bod_handle h, float learning_rate, double* grad_norm);
bod_status bod_train_get(bod_handle h, const char* layer, int32_t kind, int32_t what, float* out, int64_t n);
bod_status bod_train_set(bod_handle h, const char* layer, int32_t kind, int32_t what, const float* data, int64_t n);
bod_status bod_train_step_count(bod_handle h, int64_t* get, int64_t set);
bod_status bod_loss_forward(int32_t device, int32_t B, int32_t A, int32_t C, const float* cls,
                            const float* cls_targets, const float* box, const float* box_targets,
                            const float* covar_params, const float* anchors, const uint8_t* positive_mask,
                            const uint8_t* negative_mask, int32_t do_classification, int32_t reg_kind,
                            float label_smoothing, double* out4);
typedef struct {
    int32_t energy_samples;
    uint64_t seed;
    uint32_t first_image_id;
    int32_t reserved[4];
} bod_loss_options;
bod_status bod_loss_forward_ex(int32_t device, int32_t B, int32_t A, int32_t C, const float* cls,
                               const float* cls_targets, const float* box, const float* box_targets,
                               const float* covar_params, const float* anchors, const uint8_t* positive_mask,
                               const uint8_t* negative_mask, int32_t do_classification, int32_t reg_kind,
                               float label_smoothing, double* out4, const bod_loss_options* options);
bod_status bod_set_loss_options(bod_handle h, const bod_loss_options* options);
bod_status bod_anchor_targets(int32_t device, int32_t A, const float* anchors_vuhw, int32_t B, const int32_t* num_gt,
                              const float* gt_boxes_vuvu, const float* gt_classes, int32_t C, float min_positive_iou,
                              float max_negative_iou, float* cls_targets, float* box_targets, uint8_t* positive_mask,
                              uint8_t* negative_mask, int32_t* best_gt, float* best_iou);
bod_status bod_validation_losses_boxes(bod_handle h, const int32_t* num_gt, const float* gt_boxes_vuvu, const float* gt_classes,
                                       float min_positive_iou, float max_negative_iou, int32_t do_classification,
                                       int32_t reg_kind, float label_smoothing, double* sums4);
bod_status bod_get_validation_detections_batch(bod_handle h, int32_t* num_detections, float* scores, float* corners);
bod_status bod_validate_boxes(bod_handle h, const float* images, int32_t images_on_device, const int32_t* num_gt,
                              const float* gt_boxes_vuvu, const float* gt_classes, float min_positive_iou,
                              float max_negative_iou, int32_t do_classification, int32_t reg_kind, float label_smoothing,
                              double* sums4, int32_t* num_detections, float* scores, float* corners);
bod_status bod_loss_backward(int32_t device, int32_t B, int32_t A, int32_t C, const float* cls,
                             const float* cls_targets, const float* box, const float* box_targets,
                             const float* covar_params, const float* anchors, const uint8_t* positive_mask,
                             const uint8_t* negative_mask, int32_t do_cls, int32_t reg_kind, float label_smoothing,
                             float w_cls, float w_reg, double* out4, float* dcls, float* dbox, float* dcov);
bod_status bod_loss_backward_ex(int32_t device, int32_t B, int32_t A, int32_t C, const float* cls,
                                const float* cls_targets, const float* box, const float* box_targets,
                                const float* covar_params, const float* anchors, const uint8_t* positive_mask,
                                const uint8_t* negative_mask, int32_t do_cls, int32_t reg_kind, float label_smoothing,
                                float w_cls, float w_reg, double* out4, float* dcls, float* dbox, float* dcov,
                                const bod_loss_options* options);
bod_status bod_pdq_corner_heatmaps(int32_t device, int32_t img_h, int32_t img_w, int32_t n, const double* means_yx,
                                   const double* covs_yx, int32_t* rois, float* heatmaps);
bod_status bod_pdq_frames(int32_t device, int32_t img_h, int32_t img_w, int32_t num_frames, const int32_t* num_gt,
                          const int32_t* gt_boxes, const int32_t* num_det, const int32_t* det_boxes,
                          const double* det_corner_covs, double* fg_loss, double* bg_loss, double* det_bg_loss,
                          float* heatmaps);
bod_status bod_score_pairs(int32_t device, int64_t n, const double* means, const double* covs, const double* targets,
                           int32_t num_samples, uint64_t seed, uint64_t first_row_id, double* out, int32_t* status);
bod_status bod_bench_head_conv(bod_handle h, int32_t layer, int32_t variant, int32_t iters,
                               double* mean_ms, double* flops_per_launch);
bod_status bod_profile_begin(bod_handle h);
bod_status bod_profile_select(bod_handle h, int32_t which);
bod_status bod_profile_end(bod_handle h, double* head_conv_ms, int64_t* head_conv_launches,
                           double* head_conv_flops, double* posterior_ms, int64_t* posterior_launches);
int32_t bod_record_width(bod_handle h);
bod_status bod_gather_detections(bod_handle h, int32_t slot, void* nccl_comm, int32_t world, int32_t rank, int32_t root,
                                 float* gathered_host, float** gathered_device);
bod_status bod_get_posterior_parts(bod_handle h, int32_t image_index, float* parts);
bod_status bod_set_posterior_parts(bod_handle h, int32_t image_index, int32_t m, const float* parts);
bod_status bod_get_detection_parts(bod_handle h, int32_t image_index, float* parts);
bod_status bod_get_detection_parts_batch(bod_handle h, float* parts);
bod_status bod_collect_parts(bod_handle h, int32_t slot, float* parts);
bod_status bod_device_detection_parts(bod_handle h, int32_t slot, void** ptr);
bod_status bod_get_posterior_class_parts(bod_handle h, int32_t image_index, float* rows);
bod_status bod_get_posterior_mean_probs(bod_handle h, int32_t image_index, float* mean_probs);
bod_status bod_set_posterior_class_parts(bod_handle h, int32_t image_index, int32_t m, const float* mean_probs, const float* rows);
bod_status bod_get_detection_class_parts(bod_handle h, int32_t image_index, float* rows);
bod_status bod_get_detection_class_parts_batch(bod_handle h, float* rows);
bod_status bod_collect_class_parts(bod_handle h, int32_t slot, float* rows);
bod_status bod_device_detection_class_parts(bod_handle h, int32_t slot, void** ptr);
enum { BOD_MERGE_BAYES = 0, BOD_MERGE_CENTRE = 1, BOD_MERGE_MIXTURE = 2 };
bod_status bod_set_merge_method(bod_handle h, int32_t method);
bod_status bod_get_merge_method(bod_handle h, int32_t* method);
bod_status bod_get_detection_merge_terms(bod_handle h, int32_t image_index, float* within, float* between, int32_t* members);
bod_status bod_get_detection_merge_terms_batch(bod_handle h, int32_t slot, float* within, float* between, int32_t* members);
bod_status bod_device_detection_merge_terms(bod_handle h, int32_t slot, void** ptrs3);
enum { BOD_METHOD_BAYES_OD = 0, BOD_METHOD_BLACK_BOX = 1 };
typedef struct bod_blackbox_options {
    float   min_score;
    int32_t min_members;
    float   affinity_threshold;
    int32_t reserved;
} bod_blackbox_options;
bod_status bod_set_uncertainty_method(bod_handle h, int32_t method, const bod_blackbox_options* options);
bod_status bod_get_uncertainty_method(bod_handle h, int32_t* method);
bod_status bod_blackbox_samples(bod_handle h);
bod_status bod_blackbox_merge(bod_handle h);
bod_status bod_get_sample_detections(bod_handle h, int32_t image_index, int32_t sample_index, int32_t* count, int32_t* anchor_index,
                                     float* scores, float* means, float* covs);
bod_status bod_set_sample_detections(bod_handle h, int32_t image_index, int32_t sample_index, int32_t count,
                                     const int32_t* anchor_index, const float* scores, const float* means, const float* covs);
bod_status bod_plan_info(bod_handle h, int32_t* info8);
bod_status bod_plan_info_n(bod_handle h, int32_t* info, int32_t n);
bod_status bod_stat_reset(bod_handle h);
bod_status bod_stat_forward(bod_handle h, const float* images, int32_t images_on_device, uint64_t seed, uint32_t first_image_id,
                            int32_t sample_base);
bod_status bod_stat_merge_from(bod_handle dst, bod_handle src);
bod_status bod_stat_merge(bod_handle h, const void* const* ptrs3, int32_t samples);
bod_status bod_stat_device(bod_handle h, void** ptrs3, int32_t* samples);
bod_status bod_stat_get(bod_handle h, float* cls_sum, float* box_moments, float* cov_sum, int32_t* samples);
bod_status bod_stat_set(bod_handle h, const float* cls_sum, const float* box_moments, const float* cov_sum, int32_t samples);
bod_status bod_stat_posterior(bod_handle h, uint64_t seed, uint32_t first_image_id);
enum { BOD_VIEW_IDENTITY = 0, BOD_VIEW_HFLIP = 1 };
bod_status bod_stat_forward_view(bod_handle h, const float* images, int32_t images_on_device, uint64_t seed, uint32_t first_image_id,
                                 int32_t sample_base, int32_t view);
bod_status bod_stat_merge_view(bod_handle h, const void* const* ptrs3, int32_t samples, int32_t view);
bod_status bod_stat_get_entropy(bod_handle h, float* ent_sum);
bod_status bod_stat_set_entropy(bod_handle h, const float* ent_sum);
bod_status bod_stat_device_entropy(bod_handle h, void** ptr);
bod_status bod_stat_merge_entropy(bod_handle h, const void* ent_sum, int32_t view);
typedef struct bod_acquisition_options {
    float min_foreground;
    int32_t top_k;
    int32_t reserved[2];
} bod_acquisition_options;
bod_status bod_stat_acquisition(bod_handle h, const bod_acquisition_options* options, double* frame_scores, double* per_class);
bod_status bod_stat_acquisition_map(bod_handle h, float* mi);

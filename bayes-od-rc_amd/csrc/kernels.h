// Internal launch interface between engine.hip and the kernel translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>
#include "../../include/bayesod.h"
#include "plan_tables.h"
#include "sparse_tables.h"

// ------------------------------------------------------------------------------------------------
// Implicit-GEMM convolution (conv_igemm.hip)
//
// D[cout][pixel] = sum_k W[cout][k] * X[pixel][k],  k = (tap, cin).   NHWC bf16 activations live
// in spatially zero-padded planes so the im2col gather never needs bounds checks; output "rows"
// (pixels) are described by a row table, which lets one launch cover all pyramid levels, MC
// samples and images at once.
// ------------------------------------------------------------------------------------------------
// struct RowEnt (32 B per output pixel) and XR_EXT_ROWS: plan_tables.h (plain C++, shared with the host sanitizer build)

struct ConvGroup {         // element type of in / w / res / out_relu: bf16 (default) or fp32 (fp32 precision mode)
    const void* in;        // activations
    const void* w;         // [Cout_pad][taps][Cin]
    const float* bias;     // fp32 [Cout_pad]
    void* out;             // activation type, or fp32 with CONV_OUT_F32
    const void* res;       // residual or nullptr
    void* out_relu;        // optional second output relu(out) (P6 -> P7 input) or nullptr
    int32_t in_coff;       // channel offset inside an input pixel
    int32_t layer_id;      // dropout stream id (head*4 + layer)
    // Fused head output conv (1x1, 256 -> cout2) applied to this group's finished output tile while it
    // is still in LDS; the tile itself is then not stored (nothing else reads the last tower layer).
    const void* w2;        // bf16 [cout2 rounded up to 32][256] or nullptr
    const float* bias2;    // fp32, padded like w2
    float* out2;           // fp32 [rows][out2_cstride]; row index = RowEnt.pad0
    int32_t cout2;         // real output channels (A*C, A*4, A*10)
    int32_t out2_cstride;
    // MC aggregation fused behind the 1x1 (inference_utils.py:31-60,220-244): when agg_kind != 0 the per-sample head outputs of
    // a tile never leave the CU -- the tile holds ALL agg_n samples of its pixels (row = pixel_slot * agg_n + sample, see the
    // "aggregated" row tables of engine.hip), the fp32 outputs go through LDS and one thread per (pixel, anchor) reduces over
    // the samples: AGG_CLS sum_n softmax(logits) [B,A,C]; AGG_BOX Welford mean + M2 of the decoded boxes [B,A,16] (mean 4, lower
    // triangle of M2 10, 2 pad); AGG_COV sum_n of the covariance parameters [B,A,10].  out2 is then unused, except by AGG_CLS_ENT
    // (BOD_PARTS_CLASS handles): AGG_CLS plus sum_n H(softmax(logits_n)), one float per (image, anchor), stored to out2 [B,A].
    int32_t agg_kind;
    int32_t agg_n;         // MC samples per pixel in a tile
    int32_t agg_P;         // pixels per image (RowEnt.pad0 = (image * agg_n + sample) * agg_P + pixel)
    int32_t agg_C;         // classes (AGG_CLS) -- 4 or 8
    float* agg_out;
    const float* anchors;  // [A,4] (v,u,h,w): box decode of AGG_BOX
    // Bottleneck chain (ResNet stages 2-3, bf16 inference; 64x128 / 128x128 tiles whose cout tile holds ALL couts of this 3x3 conv):
    // the finished tile of this group's conv -- a block's `2b` -- stays in LDS and feeds the block's 1x1 expansion `2c`
    // (ch_w2: [ch_c2][cout] bf16, + bias + shortcut ch_res + ReLU -> plane ch_out) and, on that result, the NEXT block's 1x1
    // reduction `2a` (ch_w3: [cout][ch_c2] bf16, + bias + ReLU -> plane ch_out3; optional).  All planes share this conv's output
    // geometry (pixel index = RowEnt.out_off); the 2b output itself is not stored.  feature_extractor.py:195-213,283-309.
    const void* ch_w2; const float* ch_b2; const void* ch_res; void* ch_out; int32_t ch_c2;
    const void* ch_w3; const float* ch_b3; void* ch_out3;
    // Pointwise kernel, next form (conv_pointwise.hip; ch_w3 without ch_w2): this group's conv is a block's `2c` itself (64 -> 256 of
    // stage 2, 128 -> 512 of stage 3) and ch_w3 / ch_b3 / ch_out3 the next block's `2a` (256 -> 64, 512 -> 128) on its finished tile.
    // Pointwise kernel, dual form (conv_pointwise.hip, NEXT = 2): ch_w3 / ch_b3 / ch_out3 describe a second 1x1 convolution (64 couts,
    // + bias + ReLU) of the SAME input tile -- a ConvBlock's `2a` riding on its projection shortcut `branch1` -- instead of one of
    // the finished output tile.
    int32_t ch_dual;
    // f16mx precision (ConvArgs.mx != 0): 1 = this group's output rows leave in the tower format "hx" (header of conv_igemm.hip: per 64
    // channels a 128-byte H chunk of 64 f16 hi and a 128-byte X chunk of four 32-byte slots -- 16 channels as 32 e2m3 (fp6) elements
    // {hi6, lo6'}, lo' = lo * 2^11, 24 bytes + the block's E8M0 scale at byte 28) for the next tower layer; 0 = (hi, lo) bf16 pairs (what
    // the fused 1x1 + aggregation and every other consumer read); 2 = "h4" rows (f16mx4: e2m1 cross terms, scale bytes in chunk 6)
    int32_t out_hx;
};
enum : int32_t { AGG_NONE = 0, AGG_CLS = 1, AGG_BOX = 2, AGG_COV = 3, AGG_CLS_ENT = 4 };

enum : int32_t { CONV_RELU = 1, CONV_DROPOUT = 2, CONV_OUT_F32 = 4,
                 CONV_ACCUM = 8,       // with CONV_OUT_F32: out += result (input gradients of 1x1 layers accumulate in place)
                 CONV_NT_OUT = 16 };   // bf16 outputs stored non-temporally (set by launch_conv_igemm: the bf16 fan-out launch)

struct ConvArgs {
    ConvGroup g[3];
    const RowEnt* rows;
    int32_t M;             // number of output pixels (rows)
    int32_t taps, KW;      // KH*KW, KW
    int32_t cin;           // channels reduced per tap (multiple of 64)
    int32_t in_cstride;    // channels per input pixel
    int32_t cout_pad;      // multiple of the cout tile
    int32_t cout_valid;    // real output channels
    int32_t out_cstride;   // channels per output pixel
    int32_t res_cstride;
    int32_t flags;
    int32_t fan_count;     // >1: write fan_count dropout variants (sample n at out_off + n*fan_stride)
    int32_t fan_stride;
    uint32_t seed_lo, seed_hi;
    uint32_t drop_threshold;
    float drop_scale;
    uint32_t image_base;   // global id of image 0 of the batch
    int32_t groups;
    int32_t variant;       // 0 = production kernel; >0 = ablation / experimental builds (tests/tools)
    // Activation row reuse (3x3 stride-1 convs, 256x256 tiles): `rows` is then organised in tiles of 256
    // slots (invalid slots have out_off = -1) and `ext` lists, per tile, the XR_EXT_ROWS "extended" input
    // pixels {pixel index for ky = 0, plane pitch}: every run of x-adjacent output pixels contributes its
    // pixels plus one on either side, so the three kx taps read the SAME staged rows at offsets 0/1/2
    // (RowEnt.pad1 = a pixel's extended-row index) and activations are staged once per (chunk, ky).
    const int2* ext;
    int32_t xreuse;        // 0 off; 2 on: compact-state loop, 32-bit byte offsets against the tile's first extended row
                           // (ext[tile * 320] must be the tile's smallest pixel index); 1: first-generation loop, 64-bit pointers
    // Split-K (small-M layers: P6, the stage-4/5 layers at batch 1): ksplit > 1 splits the input-channel chunks over
    // ksplit workgroups per tile (blockIdx.z = group * ksplit + split); every split writes its raw fp32 accumulators to
    // partial[(z * M + m) * cout_pad + co] and launch_conv_igemm runs the reduce kernel (sum, bias, residual, ReLU,
    // bf16 store through the row table) behind it.  cin / 64 must be divisible by ksplit.
    int32_t ksplit;
    float* partial;
    // Optional device copy of {seed_lo, seed_hi, image_base}: when set it overrides the three by-value fields, so a launch
    // recorded in a hipGraph (training step) can be replayed with a new dropout seed / image id (nullptr in inference).
    const uint32_t* dyn_rng;
    uint32_t sample_base;  // added to every MC sample index before it enters the dropout counter (sample sharding)
    // bf16x3 precision mode: activations / weights / residuals are (hi, lo) bf16 pairs, 32 hi then 32 lo per 64-slot group
    // (conv_igemm.hip); cin, in_cstride, res_cstride, in_coff and -- for non-fp32 outputs -- out_cstride count SLOTS (2 per
    // channel), cout_pad / cout_valid stay in channels.
    int32_t split;
    // Output plane geometry of a plane -> plane convolution whose row table is ordered (image, y, x): rows per image and pixels per
    // row (0 = unknown).  The sliding-window 3x3 kernel (conv_pointwise.hip) walks column strips with it.
    int32_t plane_h, plane_w;
    // Compute units the launch may fill (0 = unknown: the device's count).  The engine sets it per launch -- the whole chip, or the
    // CU partition of the stream the launch goes to (bod_config.pipeline_overlap) -- and the planner compares workgroup counts with it.
    int32_t n_cu;
    // Fan-out launch (first tower layer): the first workgroup of CU slot k of every XCD starts (k & 3) * stagger_ticks 100-MHz ticks
    // late, so that the ten-fold store bursts of the CUs' epilogues interleave with other CUs' main loops instead of all hitting HBM
    // at once (conv_igemm.hip).  0 = off.
    int32_t stagger_ticks;
    // Fan-out launch, order of the (pixel tile, head) work items in an XCD's range (set by launch_conv_igemm): 0 = interleaved (tile 0 heads
    // 0 1 2, tile 1 ...: a tile's heads share its input rows through L2); T > 0 = chunks of T tiles, head-major (one head's weights at a time in L2)
    int32_t fan_chunk;
    // f16mx precision, head towers on the row-reuse loop (with `split`: same slot counts, same 1 KiB pixel rows): 1 = activations and
    // weights in the hx format, one f16 product + half a block-scaled e2m3 (fp6) product (the two cross terms) per multiplication; 2 = (hi, lo)
    // bf16 pairs in (the bf16x3 loop), epilogue able to write hx rows (first tower layer); 3 = activations and weights in the h4 format
    // (f16mx4: the cross terms as e2m1 products of twice the channels; the weight buffer carries a compact copy of its scale bytes behind
    // the 256 rows).  0 = off.
    int32_t mx;
    int32_t mx_loader;     // f16mx loop: which waves issue the weight pieces (conv_igemm.hip; 0 all, 1 lower four, 2 upper four)
    // Rows per pixel tile of a launch with `tile_count`: 0 or 256 = the 256x256 tile; 192 = the 256-cout x 192-row build (three 16-row
    // pixel fragments per wave: the sparse tail, whose tiles close on their extended rows long before 256 rows are full).  `rows`
    // then holds M / 192 tiles of 192 rows; `ext` is XR_EXT_ROWS per tile either way.
    int32_t tile_rows;          // (in the padding in front of the pointer: the argument block keeps its size)
    // Row-reuse launch whose tile count is only known on the device (the sparse tail, launch_sparse_tail_rows): `rows` / `ext` hold
    // capacity for M / 256 tiles (M / tile_rows with `tile_rows`), the first *tile_count of them are valid (conv_igemm_kernel).  nullptr = M / 256 tiles.
    const int32_t* tile_count;
};

// hipFuncSetAttribute is per device: remember which devices of this process already have the attribute
struct PerDeviceOnce {
    bool done[64] = {false};
    bool* slot() { int d = 0; if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) d = 0; return &done[d]; }
};

// Compute units a launch may fill: ConvArgs.n_cu when the engine set it (the whole chip, or a CU-partitioned stream's share), else the
// current device's count (hipDeviceProp_t::multiProcessorCount, cached per device).  The planner's rules compare workgroup counts with it.
int device_cu_count();
inline int launch_cus(const ConvArgs& a) { return a.n_cu > 0 ? a.n_cu : device_cu_count(); }
hipError_t launch_conv_igemm(const ConvArgs& a, hipStream_t s);
bool conv_igemm_uses_full_cout_tile(const ConvArgs& a);   // true => 256-wide cout tile => 1x1 fusion possible
bool conv_igemm_uses_big_tile(const ConvArgs& a);         // true => the 256x256 tile (any cout); false => 128-pixel tiles
void conv_igemm_phase_cycles(unsigned long long* out16, bool reset);   // instrumented build (variant 90)
hipError_t launch_conv_igemm_f32(const ConvArgs& a, hipStream_t s);      // conv_igemm_f32.hip (fp32 planes / weights)
// f16mx precision: (hi, lo) bf16 pair rows [npix][2C] -> hx rows [npix][4C bytes] (conv_igemm.hip; C a multiple of 64)
hipError_t launch_pairs_to_hx(const void* in, void* out, long npix, int C, hipStream_t s, int fmt = 1);          // fmt 1: hx rows, 2: h4 rows (f16mx4)

// ------------------------------------------------------------------------------------------------
// Stem + pooling + small elementwise (aux_kernels.hip)
// ------------------------------------------------------------------------------------------------
// 7x7 s2 VALID conv (fp32 image, fp32 folded weights [7][7][3][64]) + bias + ReLU -> bf16 [B,oh,ow,64]
hipError_t launch_stem_conv(const float* img, const float* w, const float* bias, void* out, int out_f32,
                            int B, int H, int W, int oh, int ow, hipStream_t s);
// launch_stem_conv = the rule (stem_conv_form: precision, BOD_STEM_SEG64, row alignment) + the launch of that form.  fp32: exact fp32
// MFMA, 64-pixel tasks; SEG64 / ROW: the bf16 kernels on 64-pixel and on 256-pixel row tasks (bit-identical planes).  The row kernel
// needs W % 4 == 0 and a 16-byte aligned image (stem_conv_row_fits; hipErrorInvalidValue otherwise, nothing launched)
enum StemConvForm { STEM_CONV_F32 = 0, STEM_CONV_SEG64 = 1, STEM_CONV_ROW = 2 };
bool stem_conv_row_fits(const float* img, int W);
StemConvForm stem_conv_form(const float* img, int out_f32, int W);
hipError_t launch_stem_conv_form(StemConvForm form, const float* img, const float* w, const float* bias, void* out,
                                 int B, int H, int W, int oh, int ow, hipStream_t s);
// ZeroPadding2D((1,2)) + MaxPool 3x3 s2 VALID on [B,ih,iw,64] -> padded-plane output.  mode 0: bf16 -> bf16; 1: fp32 -> fp32;
// 2: fp32 -> (hi, lo) bf16 pairs (bf16x3 precision)
// stem + zero-pad + max-pool in one kernel (bf16 inference, stem rows of <= 256 pixels; aux_kernels.hip)
bool stem_pool_fused_applies(const float* img, int B, int W, int ow, int n_cu);
// split = 1: the (hi, lo) precisions -- three bf16 products, fp32 pooling, pooled pixels stored as pairs (aux_kernels.hip)
hipError_t launch_stem_pool_fused(const float* img, const float* w, const float* bias, void* pooled, int split, int B, int H, int W, int oh,
                                  int ow, int ph, int pw, int pool_pitch, int pool_plane, hipStream_t s);
// launch_stem_pool_fused = the rule (stem_pool_fused_form: split, BOD_STEM_WAVES) + the launch of that form.  Every form needs
// stem_pool_fused_fits: ow <= 256, W % 4 == 0, a 16-byte aligned image (hipErrorInvalidValue otherwise, nothing launched)
enum StemFusedForm { STEM_FUSED_8 = 0, STEM_FUSED_4 = 1, STEM_FUSED_SPLIT = 2 };
bool stem_pool_fused_fits(const float* img, int W, int ow);
StemFusedForm stem_pool_fused_form(int split);
hipError_t launch_stem_pool_fused_form(StemFusedForm form, const float* img, const float* w, const float* bias, void* pooled, int B, int H,
                                       int W, int oh, int ow, int ph, int pw, int pool_pitch, int pool_plane, hipStream_t s);
hipError_t launch_stem_pool(const void* in, void* out, int mode, int B, int ih, int iw, int oh, int ow,
                            int out_pitch, int out_plane, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// Bayesian post-processing (post_kernels.hip)
// ------------------------------------------------------------------------------------------------
struct PostCfg {
    int32_t B, N, A, C, draws;
    int32_t use_full_covar, has_covar, dirichlet, gaussian_iso, ranking_method;
    float iso_var;
    float kitti_sh, kitti_sw;       // 0 => off
    const float* kitti_frame;       // [B][2] (sh, sw) of every frame (a ragged upload's frames), used in place of the two scalars; nullptr => the scalars
    uint32_t seed_lo, seed_hi, image_base;
    int32_t aggregated;             // 1: the MC statistics come from the conv epilogue (PostBuffers.agg_*), not from raw [B,N,A,.]
};

struct PostBuffers {
    // inputs
    const float* cls;       // [B,N,A,C]
    const float* box;       // [B,N,A,4]
    const float* cov;       // [B,N,A,10]
    const float* anchors;   // [A,4]
    // PostCfg.aggregated: per-anchor MC statistics written by the last tower layers' epilogues (ConvGroup.agg_kind)
    const float* agg_cls;   // [B,A,C]   sum over samples of softmax(logits)
    const float* agg_box;   // [B,A,16]  Welford mean[4], lower triangle of M2[10], 2 pad
    const float* agg_cov;   // [B,A,10]  sum over samples of the covariance parameters
    // dense per-anchor scratch
    uint8_t* keep;          // [B,A]
    float* d_counts;        // [B,A,C]   sampled counts (likelihood)
    // compacted outputs, capacity A per image
    int32_t* block_counts;  // [B, nblocks]
    int32_t* num_kept;      // [B]
    float* counts;          // [B,A,C]   Dirichlet posterior counts
    float* score;           // [B,A,C]
    float* means;           // [B,A,4]
    float* covs;            // [B,A,16]
    float* ranking;         // [B,A]
    float* corners;         // [B,A,4]
    int32_t* anchor_index;  // [B,A]
};

hipError_t launch_posterior(const PostCfg& c, const PostBuffers& b, hipStream_t s);
// launch_posterior in two halves: the keep flags (sampling + per-image scan) and the rest (compaction + per-anchor fusion)
hipError_t launch_posterior_keep(const PostCfg& c, const PostBuffers& b, hipStream_t s);
hipError_t launch_posterior_fuse(const PostCfg& c, const PostBuffers& b, hipStream_t s);

// Sparse tail (engine.hip): the aggregating launches of the box and covariance heads run only over the pixels with at least one kept
// anchor, and (with `halo_rows`) the two layers that feed them -- box layer 1, covariance layer 2 -- only over the 3x3 dilation of
// those pixels.  One workgroup per image flags the pixels of both tables, lists their runs with prefix scans, packs the runs into
// sample-complete row-reuse tiles (one wave per table) and writes the rows (sparse_tables.h).  Every RowEnt is the one of the dense
// per-sample table (same dropout counters, same aggregation slot); `pix` is that table's image 0 / sample 0 part (P entries), the
// others differ by closed forms.
struct SparseTailArgs {
    const uint8_t* keep;        // [B, A] (post_sample_kernel)
    const RowEnt* pix;          // [P]
    RowEnt* rows;               // tail: [cap_tiles * tail_rows]
    int2* ext;                  // tail: [cap_tiles * XR_EXT_ROWS]
    RowEnt* halo_rows;          // halo: [cap_tiles * 256], or nullptr (tail only)
    int2* halo_ext;             // halo: [cap_tiles * XR_EXT_ROWS]
    int32_t* tile_count;        // [2]: tail, halo tiles; zeroed by the launcher
    int2* runs;                 // scratch [tables * B * P]: {first, last pixel} of every run
    StQuad* chunks;             // scratch [tables * B * P]: pieces (sparse_tables.h StPack)
    StQuad* tiles;              // scratch [tables * B * P]: tiles
    int32_t B, N, P, apl, cap_tiles;
    int32_t tail_rows;          // rows per tail tile: 192 or 256 (the halo table's tiles always have 256)
    int64_t Ppad;
    SparseLevels lv;
};
hipError_t launch_sparse_tail_rows(const SparseTailArgs& a, hipStream_t s);
hipError_t launch_joint_entropy_rank(const PostCfg& c, const PostBuffers& b, hipStream_t s);
hipError_t launch_validation_post(const PostCfg& c, const PostBuffers& b, hipStream_t s);   // validation_utils.py:10-77

struct NmsArgs {
    int32_t B, A;                 // per-image capacity A
    const int32_t* num_kept;      // [B]
    const float* corners;         // [B,A,4]
    const float* ranking;         // [B,A]
    float* work_scores;           // [B, A rounded up to 512] scratch (used when M exceeds the LDS capacity)
    int32_t* work_begin;          // same shape
    int32_t* selected;            // [B,max_out]
    int32_t* num_selected;        // [B]
    int32_t max_out;
    float iou_thr, sigma;
    int32_t variant;
};
hipError_t launch_nms(const NmsArgs& a, hipStream_t s);

// Records of the validation path: score rows and corners (y1, x1, y2, x2) of every image's selected candidates, in soft-NMS order
struct ValGatherArgs {
    int32_t B, A, C, max_out;
    const int32_t* num_kept;      // [B]
    const int32_t* selected;      // [B,max_out] indices into the image's compacted candidates
    const int32_t* num_selected;  // [B]
    const float* score;           // [B,A,C]
    const float* corners;         // [B,A,4]
    float* out_scores;            // [B,max_out,C]; rows beyond the image's count are zero
    float* out_corners;           // [B,max_out,4]
    int32_t* out_num;             // [B]
};
hipError_t launch_validation_gather(const ValGatherArgs& a, hipStream_t s);

struct ClusterArgs {
    int32_t B, A, C, max_out;
    const int32_t* num_kept;
    const int32_t* selected;      // [B,max_out]
    const int32_t* num_selected;  // [B]
    const float* corners;         // [B,A,4]
    const float* counts;          // [B,A,C]
    const float* means;           // [B,A,4]
    const float* covs;            // [B,A,16]
    float thr;
    // optional caller-supplied affinity (bayes_od_clustering's `affinity_matrix`, inference_utils.py:316): for image
    // `affinity_img`, row k = affinity_matrix[:, centre_k] ([max_out][A] floats); nullptr = IoU of the means on the fly
    const float* affinity; int32_t affinity_img;
    // outputs [B,max_out,...]
    float* out_scores; float* out_means; float* out_covs; float* out_counts;
};
hipError_t launch_cluster_fuse(const ClusterArgs& a, hipStream_t s);
// The other ways to merge a cluster (bayesod.h, bod_set_merge_method): method = BOD_MERGE_CENTRE or
// BOD_MERGE_MIXTURE in place of cluster_fuse_kernel, same ClusterArgs, grid and membership test.  Writes the five detection arrays
// and the terms: within / between [B,max_out,16], members [B,max_out].
struct MergeTerms { float* within; float* between; int32_t* members; };
hipError_t launch_cluster_merge(const ClusterArgs& a, int method, MergeTerms out, hipStream_t s);
// Black-box MC dropout (bayesod.h, bod_set_uncertainty_method): every (image b, sample n) is a virtual image
// v = b * N + n of the validation post-process and of nms_kernel, then the image's N detection sets are pooled and merged.
//   launch_blackbox_samples  bb_flag_kernel / post_scan_kernel / bb_compact_kernel over the B*N virtual images (every scratch array
//                            below has B*N images' worth), launch_nms on them, then bb_gather_kernel: the softmax row, the decoded
//                            box and the sample's own aleatoric matrix of the at most max_out selected rows, KITTI-rescaled, the
//                            rows below min_score dropped in order
//   launch_blackbox_merge    bb_merge_kernel, one workgroup per image: greedy centre pick (block arg-max), members by iou_plus1 against
//                            the centre, sample mean / within / between of the members; pooled index = n * max_out + rank
struct BlackBoxArgs {
    int32_t B, N, A, C, max_out;
    float min_score; int32_t min_members; float thr;
    // stage 1 scratch, per virtual image
    uint8_t* keep;            // [B*N,A]
    float* top;               // [B*N,A]   top softmax score per anchor (dense)
    int32_t* block_counts;    // [B*N,nblocks]
    int32_t* num_kept;        // [B*N]
    float* ranking;           // [B*N,A]   compacted
    float* corners;           // [B*N,A,4] compacted, network coordinates
    int32_t* anchor_index;    // [B*N,A]   compacted
    float* work_scores; int32_t* work_begin;      // nms_kernel's fallback, [B*N, A rounded up to 512]
    int32_t* selected; int32_t* num_selected;     // [B*N,max_out], [B*N]
    // sample detections
    float* sd_score;          // [B*N,max_out,C]
    float* sd_mean;           // [B*N,max_out,4]
    float* sd_cov;            // [B*N,max_out,16]
    int32_t* sd_anchor;       // [B*N,max_out]
    int32_t* sd_count;        // [B*N]
    // stage 2 work buffers for a pool beyond the LDS capacity
    float* pool_top;          // [B,N*max_out]
    float* pool_corners;      // [B,N*max_out,4]
    // outputs [B,max_out,...] (a record slot and its merge terms); out_centre: pooled index of every emitted cluster's centre
    int32_t* out_num; int32_t* out_centre;
    float* out_scores; float* out_means; float* out_covs; float* out_counts;
};
hipError_t launch_blackbox_samples(const PostCfg& c, const PostBuffers& in, const BlackBoxArgs& a, const NmsArgs& nms, hipStream_t s);
hipError_t launch_blackbox_merge(const BlackBoxArgs& a, MergeTerms terms, hipStream_t s);
hipError_t launch_iou_matrix(const float* corners, int M, float* out, hipStream_t s);
// Covariance parts (bod_config.covariance_parts): every covariance the two fusion steps store, split into what the fused
// mean inherits from the epistemic noise, from the aleatoric noise and from the prior -- three symmetric 4x4 terms that sum to it.
//   launch_posterior_parts  behind post_fuse_kernel, one thread per kept slot: parts [B,A,30] = the three lower triangles (row by row:
//                           00 10 11 20 21 22 30 31 32 33) of epi, ale, pri; writes nothing else
//   launch_cluster_parts    beside cluster_fuse_kernel (same ClusterArgs, same membership test): out_parts [B,max_out,3,16]
#define BOD_PARTS_TRI 30
hipError_t launch_posterior_parts(const PostCfg& c, const PostBuffers& b, float* parts, hipStream_t s);
hipError_t launch_cluster_parts(const ClusterArgs& a, const float* parts, float* out_parts, hipStream_t s);
// Class-entropy parts (bod_config.covariance_parts bit BOD_PARTS_CLASS): the entropy of the MC predictive class
// distribution split into its aleatoric part (mean of the samples' entropies), the mutual information between class and weights
// (epistemic) and, per detection, the disagreement between the members' mean distributions (spatial).
//   launch_posterior_class_parts  behind post_fuse_kernel, one thread per kept slot: cparts [B,A,3+C] = total, aleatoric, epistemic,
//                                 mean_probs[C].  ent_sum [B,A] = sum_n H(softmax(logits_n)) with PostCfg.aggregated (the epilogue's
//                                 AGG_CLS_ENT / the statistics record); otherwise it is summed here from raw cls, operation for
//                                 operation as agg_reduce_cls<C, true> does
//   launch_cluster_class_parts    beside cluster_fuse_kernel (same ClusterArgs, same membership test): out [B,max_out,4] = total,
//                                 aleatoric, epistemic_mc, epistemic_spatial
// log(sden) of a sample's entropy, sden = sum_j exp(l_j - max l) in [1, C]: the hardware log2 (v_log_f32, 1 ulp; no denormal
// input here) times ln 2.  Not logf: the library routine's inlined code differs between translation units built with and without
// -ffp-contract=off (its ln 2 multiply-add fuses in one and not in the other), and the three places that form ent_sum -- the
// head epilogue in conv_igemm.hip, post_kernels.hip, stat_kernels.hip -- must agree bit for bit.
#define BOD_LOG_SDEN(x) (__builtin_amdgcn_logf(x) * 0.693147180559945f)
hipError_t launch_posterior_class_parts(const PostCfg& c, const PostBuffers& b, const float* ent_sum, float* cparts, hipStream_t s);
hipError_t launch_cluster_class_parts(const ClusterArgs& a, const float* cparts, float* out_cparts, hipStream_t s);
// detection records [B][K][1 + 4 + 16 + 2C (+ 48 when parts != nullptr) (+ 4 when cparts != nullptr)] of the multi-GPU gather (zero rows
// beyond num[b]); the row's field offsets: record_fields (record_state.h)
hipError_t launch_pack_records(const int32_t* num, const float* scores, const float* means, const float* covs, const float* counts,
                               const float* parts, const float* cparts, float* rec, int B, int K, int C, hipStream_t s);

struct PreprocArgs {
    const uint8_t* src;        // [B, sh, sw, 3] uint8 RGB
    float* dst;                // [B, H, W, 3] fp32 BGR, mean-subtracted
    int32_t B, sh, sw;         // source size
    int32_t rh, rw;            // size after the (optional) aspect-preserving bilinear resize (= sh, sw without)
    int32_t H, W;              // network input size
    int32_t crop_y, crop_x, pad_y, pad_x, vis_h, vis_w;   // tf.image.resize_with_crop_or_pad geometry
    int32_t resize;
    float scale_y, scale_x;    // sh/rh, sw/rw as float32
    float mean[3];             // RGB order
};
hipError_t launch_preprocess(const PreprocArgs& a, hipStream_t s);

// Ragged form: frame b of the batch has its own source size and resize / pad geometry (one record of a device table), the frames
// lie back to back in one packed uint8 buffer.
struct PreprocFrame {
    int64_t offset;            // first byte of the frame in the packed buffer: 3 * sum of h_i * w_i over the frames in front of it
    int32_t sh, sw, rh, rw;    // as PreprocArgs, of this frame
    float scale_y, scale_x;
    int32_t crop_y, crop_x, pad_y, pad_x, vis_h, vis_w;
};
struct PreprocRaggedArgs {
    const uint8_t* src;              // packed uint8 RGB frames
    float* dst;                      // [B, H, W, 3] fp32 BGR, mean-subtracted
    const PreprocFrame* frames;      // [B], device memory
    int32_t B, H, W;
    int32_t resize;
    float mean[3];                   // RGB order, shared by the batch
};
hipError_t launch_preprocess_ragged(const PreprocRaggedArgs& a, hipStream_t s);

// Augmented form (training only): the ragged record drawn at random on the host -- crop / pad no longer centred, the resize target
// scaled -- plus a mirror bit and two photometric scalars.  flip mirrors the SOURCE frame (every source column c read becomes
// sw - 1 - c); gain / bias act on the interpolated 0..255 value inside the visible region, v' = clamp(gain * v + bias, 0, 255) as two
// fp32 operations; padding stays 0.  flip = 0, gain = 1, bias = 0 on a centred record is preprocess_ragged_kernel bit for bit.
struct PreprocAugFrame {
    PreprocFrame g;
    int32_t flip;              // 0 or 1
    int32_t resize;            // per frame: without aspect_resize a frame is resized only when its scale moves it off its source size
    float gain, bias;
};
struct PreprocAugArgs {
    const uint8_t* src;              // packed uint8 RGB frames
    float* dst;                      // [B, H, W, 3] fp32 BGR, mean-subtracted
    const PreprocAugFrame* frames;   // [B], device memory
    int32_t B, H, W;
    float mean[3];                   // RGB order, shared by the batch
};
hipError_t launch_preprocess_augment(const PreprocAugArgs& a, hipStream_t s);

// JPEG frames (jpeg_kernels.hip): the host's entropy decoder (jpeg_entropy.h) leaves each component's coefficient
// blocks, the two kernels turn them into the packed uint8 RGB frames the ragged / augmented preprocess kernels read.  One record per
// frame, written and validated on the host; every device address comes from it.
struct JpegFrame {             // 512 B
    int64_t coef_off[3];       // first int16 of each component in the batch's coefficient buffer (multiples of 64)
    int64_t plane_off[3];      // first byte of each component's MCU-padded uint8 plane in the scratch (multiples of 16)
    int64_t rgb_off;           // first byte of the frame in the packed RGB buffer (PreprocFrame::offset)
    int32_t bw[3], bh[3];      // blocks per row / column of each component's plane
    int32_t components;        // 1 (grayscale) or 3 (YCbCr)
    int32_t h_samp, v_samp;    // luma sampling: 1x1, 2x1 or 2x2; chroma is 1x1
    int32_t width, height;
    int32_t pad[7];
    uint16_t quant[3][64];     // natural order
};
static_assert(sizeof(JpegFrame) == 512 && offsetof(JpegFrame, quant) == 128, "JpegFrame layout (16-byte loads of the quantisation rows)");
struct JpegArgs {
    const JpegFrame* frames;   // [n], device memory
    const int16_t* coefs;      // 64 per block, natural order
    uint8_t* planes;           // scratch: the components' planes
    uint8_t* rgb;              // packed uint8 RGB frames
    int32_t n;
    // every frame gets the same number of workgroups, enough for the largest: the frame of a workgroup is wave-uniform
    int32_t idct_wgs_per_frame;    // ceil(max over the frames of their 8x8 blocks / 32)
    int32_t color_wgs_per_frame;   // ceil(max over the frames of their 4-pixel groups / 256)
};
hipError_t launch_jpeg_idct(const JpegArgs& a, hipStream_t s);
hipError_t launch_jpeg_color(const JpegArgs& a, hipStream_t s);

// PNG frames (png_kernels.hip): the host's inflate (png_inflate.h) leaves each frame's filtered scanlines -- per row a
// filter-type byte the host has checked to be 0..4, then width * channels bytes --, the kernel reconstructs them (PNG specification,
// section 9) into the packed uint8 RGB frames the ragged / augmented preprocess kernels read.  One record per frame, written and
// validated on the host; every device address and every loop bound comes from it.
struct PngFrame {              // 32 B
    int64_t raw_off;           // first byte of the frame's filtered scanlines in the batch's buffer
    int64_t rgb_off;           // first byte of the frame in the packed RGB buffer (PreprocFrame::offset)
    int32_t height, width;
    int32_t channels;          // 1 gray, 2 gray + alpha, 3 RGB, 4 RGBA (8 bits each): the filters' bytes per pixel
    int32_t pad;
};
static_assert(sizeof(PngFrame) == 32, "PngFrame layout");
struct PngArgs {
    const PngFrame* frames;    // [n], device memory
    const uint8_t* raw;        // the filtered scanlines of all frames
    uint8_t* rgb;              // packed uint8 RGB frames
    int32_t n;
    int32_t rows_per_band;     // threads of a workgroup, one per row of a band: a multiple of 64, at most PNG_MAX_BAND_ROWS
};
constexpr int PNG_MAX_BAND_ROWS = 1024;
hipError_t launch_png_unfilter(const PngArgs& a, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// Loss forward (loss_kernels.hip)
// ------------------------------------------------------------------------------------------------
struct LossArgs {
    int32_t B, A, C;
    int32_t do_cls;          // focal classification term
    int32_t reg_kind;        // 0 none, 1 'regression', 2 'regression_var', 3 'regression_covar', 4 'regression_nll', 5 'regression_energy'
    float label_smoothing;
    const float* cls; const float* cls_t;       // [B,A,C]
    const float* box; const float* box_t;       // [B,A,4]
    const float* cov;                           // [B,A,10] fill_triangular parameters
    const float* anchors;                       // [A,4]
    const uint8_t* pos; const uint8_t* neg;     // [B,A]
    const float* row_term;                      // [B,A] reg_kind 5: a positive row's energy-score term (launch_energy_forward), read as s_cmp
};
hipError_t launch_loss(const LossArgs& a, float* partial, int nblocks, hipStream_t s);
hipError_t launch_loss_reduce(const float* partial, int nblocks, float* sums4, hipStream_t s);
// Per-frame sums (validation from boxes): grid.y = frame; partial [B][ceil(A / 256)][4], then sums [B][4] in double, one block
// per frame, fixed order -- a frame's four sums do not depend on the batch around it
hipError_t launch_loss_frames(const LossArgs& a, float* partial, hipStream_t s);
hipError_t launch_loss_frames_reduce(const float* partial, int frames, int nblocks, double* sums, hipStream_t s);
hipError_t launch_loss_backward(const LossArgs& a, const float* sums4, float w_cls, float w_reg, float* dcls, float* dbox, float* dcov,
                                hipStream_t s);
// reg_kind 5, the sample-based energy score: one wave64 per positive row over a fixed grid that strides over the
// list launch_loss_compact writes (list[0] = number of positives, list[1..] = their flat indices b * A + a, ascending), so the
// launches can sit in a captured graph.  The forward writes row_term[idx] of every positive row -- launch_loss / launch_loss_frames
// then sum it as s_cmp -- and the backward overwrites the positive rows of dbox / dcov that launch_loss_backward has zeroed.
#define BOD_ENERGY_MIN_SAMPLES 2
#define BOD_ENERGY_MAX_SAMPLES 1024
#define BOD_ENERGY_DEFAULT_SAMPLES 64
struct EnergyArgs {
    int32_t B, A, M;                            // M samples per row
    const float* box; const float* box_t;       // [B,A,4]
    const float* cov;                           // [B,A,10]
    const float* anchors;                       // [A,4]
    const uint32_t* dyn;                        // device {seed low, seed high, first image id} (a replayed graph), or nullptr: the three below
    uint32_t seed_lo, seed_hi, first_image_id;
    int32_t id_stride;                          // image id of frame b = first image id + b * id_stride: 1, or 0 (BOD_LOSS_ONE_IMAGE_ID)
    const int32_t* list;                        // [B*A + 1]
    float* row_term;                            // [B,A]
};
hipError_t launch_loss_compact(const uint8_t* pos, long long n, int32_t* list, hipStream_t s);
hipError_t launch_energy_forward(const EnergyArgs& a, hipStream_t s);
hipError_t launch_energy_backward(const EnergyArgs& a, const float* sums4, float w_reg, float* dbox, float* dcov, hipStream_t s);
// out[c] = sum_r g[r * nch + c]: the output-bias gradient of a head from dbox / dcov [rows = B * positions][nch = anchors per location * width]
hipError_t launch_head_bias_grad(const float* g, long long rows, int nch, float* out, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// Anchor-target assignment (target_kernels.hip): IoU of every anchor with its frame's GT rows, positive / negative masks, the best
// GT per anchor and the dense class / box targets the loss reads -- one launch for all frames and pyramid levels
struct TargetArgs {
    int32_t A, B, C;
    float min_positive_iou, max_negative_iou;
    const float* anchors;                       // [A,4] (v, u, h, w)
    const int32_t* gt_off;                      // [B+1] first GT row of every frame (>= 1 row per frame)
    const float* gt_boxes;                      // [sum G,4] corners (y1, x1, y2, x2), 16-byte aligned
    const float* gt_classes;                    // [sum G,C], 16-byte aligned
    float* cls_t; float* box_t;                 // [B,A,C], [B,A,4]
    uint8_t* pos; uint8_t* neg;                 // [B,A]
    int32_t* best_gt; float* best_iou;          // [B,A] row within the frame / its IoU (nullptr = not wanted)
};
hipError_t launch_anchor_targets(const TargetArgs& a, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// Mergeable MC statistics (stat_kernels.hip; record layout: include/bayesod.h): the three per-anchor arrays of the fused
// epilogues (ConvGroup.agg_kind) from raw head outputs of n >= 1 samples, and the fold of one set of them into another
struct StatRawArgs {
    int32_t B, N, A, C;
    const float* cls; const float* box; const float* cov;      // raw [B,N,A,C], [B,N,A,4], [B,N,A,10] (cov: nullptr without the head)
    const float* anchors;                                       // [A,4] (v, u, h, w)
    float* cls_sum; float* box_moments; float* cov_sum;         // [B,A,C], [B,A,16], [B,A,10] (nullptr with cov)
    float* ent_sum;                                             // [B,A] sum_n H(softmax(logits_n)), or nullptr (records without the entropy)
};
hipError_t launch_stat_from_raw(const StatRawArgs& a, hipStream_t s);
struct StatMergeArgs {
    int64_t BA;                                                 // images * anchors
    int32_t C;
    int32_t ka, kb;                                             // samples in the accumulator (0: copy the source) / in the source (>= 1)
    float* acc_cls; float* acc_box; float* acc_cov;             // 16-byte aligned; acc_cov / src_cov both nullptr without the head
    const float* src_cls; const float* src_box; const float* src_cov;
};
hipError_t launch_stat_merge(const StatMergeArgs& a, hipStream_t s);
// The same fold with the source read through the mirror map of a record (stat_kernels.hip header): horizontal-flip views
struct StatMirrorArgs {
    StatMergeArgs m;
    int32_t A, K, nlev;                                         // anchors per image, anchors per location, pyramid levels (<= 8)
    int32_t lvl_off[9];                                         // first anchor of every level; lvl_off[nlev] = A
    int32_t lvl_w[8];                                           // columns of every level
    float u_flip;                                               // float(image_w - 1): u' = u_flip - u
};
hipError_t launch_stat_merge_mirror(const StatMirrorArgs& a, hipStream_t s);
// The record's fourth array (BOD_PARTS_CLASS handles): acc = acc + src (copy == 0) or acc = src, float4 accesses; with `mirror` the
// source is gathered from the partner anchor of mirror->'s level table (the value itself is unchanged under a mirror; mirror->m is
// not read).  acc and src 16-byte aligned.
hipError_t launch_stat_merge_entropy(float* acc, const float* src, int64_t BA, int copy, const StatMirrorArgs* mirror, hipStream_t s);
// out[b,y,x,:] = in[b,y,W-1-x,:], fp32 [B,H,W,3]; in != out
hipError_t launch_mirror_images(const float* in, float* out, int B, int H, int W, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// Acquisition scores of a statistics record (acq_kernels.hip; include/bayesod.h bod_stat_acquisition): one streaming
// pass over the accumulator, G = acq_groups(A) workgroups per frame, then one workgroup per frame that folds their partial rows and
// finds the top-k mean of the MI scratch by bisection.  Reads the record only; no atomics.
#define ACQ_MAX_GROUPS 64                                       // workgroups per frame at most
#define ACQ_ROW_MAX 33                                          // doubles per partial row (C = 8: 16 sums, 17 maxima)
struct AcqArgs {
    int32_t B, A, C, K;                                         // frames, anchors per frame, classes (4 or 8), samples in the record (>= 2)
    int32_t G;                                                  // acq_groups(A)
    int32_t top_k;
    float thr;                                                  // foreground gate: cls_sum[C-1] <= thr
    const float* cls_sum; const float* box_moments;             // [B,A,C], [B,A,16], 16-byte aligned
    const float* cov_sum;                                       // [B,A,10] or nullptr (no covariance head)
    const float* ent_sum;                                       // [B,A] or nullptr (no BOD_PARTS_CLASS)
    float* mi;                                                  // [B,A] scratch: every anchor's MI, NaN outside the foreground set
    double* partials;                                           // [B,G,ACQ_ROW_MAX] at most
    double* scores;                                             // [B,12]
    double* per_class;                                          // [B,C-1,3] or nullptr
};
int acq_groups(int A);
hipError_t launch_acquisition(const AcqArgs& a, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// Streaming pointwise (1x1) convolution for reductions of <= 256 channels (conv_pointwise.hip); launch_conv_igemm routes eligible
// launches there (BOD_POINTWISE=0: off)
bool conv_pointwise_eligible(const ConvArgs& a);
bool conv_pointwise_can_fuse_next(const ConvArgs& a);      // plan time: may a 64 -> 256 expansion carry the next block's 2a (ch_w3)?
bool conv_pointwise_can_fuse_next3(const ConvArgs& a);     // plan time: may a 128 -> 512 expansion (stage 3) carry the next block's 2a (512 -> 128)?  BOD_PW_FUSE_NEXT3=0: never
bool conv_pointwise_can_fuse_dual(const ConvArgs& a);     // plan time: may a 64 -> 256 projection shortcut carry its own block's 2a (ch_w3 + ch_dual)?
hipError_t launch_conv_pointwise(const ConvArgs& a, hipStream_t s);
// Sliding-window 3x3 stride-1 SAME convolution, 64 -> 64 channels (ResNet stage 2's `2b`; conv_pointwise.hip, BOD_SLIDE3X3=0: off)
bool conv_slide3x3_eligible(const ConvArgs& a);
hipError_t launch_conv_slide3x3(const ConvArgs& a, hipStream_t s);

// Training-step building blocks (train_kernels.hip)
// ------------------------------------------------------------------------------------------------
hipError_t launch_gather_transpose(const void* in, const RowEnt* rows, void* out, int M, int Kpad, int C, int cstride,
                                   int taps, int KW, bool append_ones_row, hipStream_t s, bool f32 = false);
hipError_t launch_fill_row_bf16(void* row, int n_set, int n_total, float value, hipStream_t s);

struct FoldArgs {
    const float* kernel;        // master [taps][cin][cout]
    const float* bias;          // master [cout] or nullptr
    const float *gamma, *beta, *mean, *var;   // BatchNorm (nullptr: no BN)
    float eps;
    int32_t taps, cin, cout, cout_pad;
    uint16_t* w_fwd;            // [cout_pad][taps][cin] bf16 (or nullptr)
    float* w_fwd32;             // stem: fp32 [taps*cin][cout] (or nullptr)
    uint16_t* w_bwd;            // [(tap, ci)][cout_pad] bf16 (or nullptr)
    uint16_t* w_flip;           // [cin][taps, flipped][cout_pad] bf16: the input gradient of a stride-1 SAME layer as a convolution (or nullptr)
    float* b_fwd;               // folded bias [cout_pad]
    int32_t f32;                // fp32 training handle: the three packings above hold float (same layouts)
};
struct ActBwdArgs {
    const float* dout;          // gradient of the layer output, laid out like the output buffer
    const uint16_t* out_bf16;   // stored output (mask source) or nullptr (no activation: fp32 raw head outputs)
    const RowEnt* rows;
    float* dres;                // gradient buffer of the residual input or nullptr
    uint16_t* dz;               // dense [M][cout_pad] bf16
    uint16_t* dzp;              // the same values in the output plane's own (zero-bordered) layout, or nullptr
    uint16_t* dzt;              // the same values transposed, [cout_pad][Kpad] (columns M..Kpad-1 zero), or nullptr
    int32_t M, cout, cout_pad, out_cstride, res_cstride, Kpad;
    float scale;                // dropout keep scale (1 without dropout)
    int32_t f32;                // fp32 training handle: out_bf16 / dz / dzp hold float, dzt is not written
};
struct UnfoldArgs {
    const float* dwp;           // [(taps*cin) + 1][cout]: folded-weight gradient, last row = folded-bias gradient
    const float* kernel; const float* bias;
    const float *gamma, *mean, *var;
    float eps;
    int32_t taps, cin, cout;
    float *d_kernel, *d_bias, *d_gamma, *d_beta;
    float* dot;                 // [cout] zero-initialised scratch for the gamma dot products (left zeroed)
    float l2;                   // Keras l2(rate) on the kernel: d_kernel += 2 rate K, *l2_loss += rate sum K^2 (0 = none)
    float* l2_loss;
};
hipError_t launch_fold_pack(const FoldArgs& a, hipStream_t s);
hipError_t launch_fold_pack_all(const FoldArgs* device_array, int count, long max_elems, hipStream_t s);
// *wrote_transpose tells the caller whether a.dzt was produced by the same launch (tile form) or still needs a transpose pass
hipError_t launch_act_backward_gather(const ActBwdArgs& a, hipStream_t s, bool* wrote_transpose = nullptr);
hipError_t launch_relu_merge(const float* dout_relu, const void* out, float* dout, long n, hipStream_t s, bool f32 = false);
hipError_t launch_col2im(const float* dxcol, const RowEnt* rows, float* din, int M, int taps, int KW, int cin, int in_cstride, hipStream_t s);
hipError_t launch_stem_pool_backward(const void* stem_out, const float* dpool, void* dz, int B, int ih, int iw, int oh, int ow, int pool_pitch,
                                     int pool_plane, hipStream_t s, bool f32 = false);
hipError_t launch_unfold_grad(const UnfoldArgs& a, hipStream_t s);
hipError_t launch_l2_grad(const float* w, float* g, long n, float rate, float* loss_acc, hipStream_t s);
hipError_t launch_sumsq(const float* g, long n, float* acc, float* partial1024, hipStream_t s);
hipError_t launch_adam(float* w, const float* g, float* m, float* v, long n, const float* sumsq, float clip, const float* lr_t, float beta1, float beta2,
                       float eps, hipStream_t s);
hipError_t launch_f32_to_bf16(const float* in, void* out, long n, hipStream_t s);
hipError_t launch_make_dgrad_rows(const RowEnt* fwd, RowEnt* out, int M, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// PDQ evaluation (pdq_kernels.hip): host drivers of bod_pdq_corner_heatmaps / bod_pdq_frames on the caller's stream and
// current device.  Return a bod_status value; on failure errbuf holds the message.
// ------------------------------------------------------------------------------------------------
int pdq_corner_heatmaps_run(int H, int W, int n, const double* means_yx, const double* covs_yx, int32_t* rois, float* heatmaps,
                            hipStream_t s, char* errbuf, size_t errcap);
int pdq_frames_run(int H, int W, int F, const int32_t* num_gt, const int32_t* gt_boxes, const int32_t* num_det, const int32_t* det_boxes,
                   const double* det_corner_covs, double* fg_loss, double* bg_loss, double* det_bg_loss, float* heatmaps, hipStream_t s,
                   char* errbuf, size_t errcap);
// bod_pdq_frames' box heatmaps of one frame's rows, left on the device in d_heat [nd][H][W] (NULL: validate only); *bad_row names a
// refused row.  The rendering stage's HEAT view composes them (render_kernels.hip).
int pdq_box_heatmaps_device(int H, int W, int nd, const int32_t* det_boxes, const float* det_corner_covs, float* d_heat, int* bad_row,
                            hipStream_t s, char* errbuf, size_t errcap);
// Rendering (render_kernels.hip): host drivers of bod_render_frames_u8, same conventions.  render_validate needs no
// device and runs first.
int render_validate(int32_t n, const uint8_t* rgb_in, const int32_t* src_hw, const int32_t* num_det, const int32_t* det_boxes,
                    const float* det_corner_covs, const uint8_t* det_colors, const uint8_t* det_text, const int32_t* num_gt,
                    const int32_t* gt_boxes, const bod_render_options* opt, uint8_t* rgb_out, char* errbuf, size_t errcap);
int render_frames_run(int32_t n, const uint8_t* rgb_in, const int32_t* src_hw, const int32_t* num_det, const int32_t* det_boxes,
                      const float* det_corner_covs, const uint8_t* det_colors, const uint8_t* det_text, const int32_t* num_gt,
                      const int32_t* gt_boxes, const bod_render_options* opt, uint8_t* rgb_out, int32_t* skipped_ellipses, hipStream_t s,
                      char* errbuf, size_t errcap);
// Scoring rules (score_kernels.hip): host driver of bod_score_pairs, same conventions; rows are staged in internal batches.
int score_pairs_run(long long n, const double* means, const double* covs, const double* targets, int num_samples, unsigned long long seed,
                    unsigned long long first_row_id, double* out, int32_t* status, hipStream_t s, char* errbuf, size_t errcap);

// ------------------------------------------------------------------------------------------------
// Frame corruptions (corrupt_kernels.hip): op chains on the packed uint8 RGB frames, between the copy (or the JPEG
// colour kernel) and the preprocess kernels.  The functions return a bod_status value; on failure errbuf holds the message.
// ------------------------------------------------------------------------------------------------
struct CorruptSpec {                       // a validated description, copied from the caller: n == 0 means none
    int32_t n = 0, ops_per_frame = 0;
    std::vector<bod_corrupt_op> ops;       // [n][ops_per_frame]
    std::vector<uint32_t> frame_ids;       // [n]
    std::vector<uint16_t> taps;
    std::vector<uint8_t> luts;             // [..][3][256]
    std::vector<uint16_t> qtables;         // [..][2][64]
    uint64_t seed = 0;
};
int corrupt_spec_make(const char* who, int32_t n, const bod_corrupt_op* ops, int32_t ops_per_frame, const uint32_t* frame_ids,
                      const uint16_t* taps, int32_t n_taps, const uint8_t* luts, int32_t n_luts, const uint16_t* qtables,
                      int32_t n_qtables, uint64_t seed, CorruptSpec* out, char* errbuf, size_t errcap);
struct CorruptSlot {                       // one route's device side: record / table blob, ping-pong scratch, both grow on demand
    std::vector<char> host;
    char* dev = nullptr; size_t dev_cap = 0;
    uint8_t* scratch = nullptr; size_t scratch_cap = 0;
    hipEvent_t copied = nullptr;           // the copy of `host` has left the host (its next rewrite waits for it)
    size_t sums_off = 0, sums_bytes = 0, taps_off = 0, luts_off = 0, q_off = 0, frame_bytes = 0;
    int32_t wgs[4][4] = {};                // per op slot: workgroups per frame of the pointwise, conv, pixelate and JPEG kernels
    uint32_t kinds[4] = {};                // per op slot: bit k set when a frame runs kind k there
    void release();
};
// Host half: lays the batch out for src_hw[n][2], rewrites slot.host and grows the device buffers (synchronising `stream` first when
// it has to free one).  Nothing is enqueued.
int corrupt_prepare(CorruptSlot& slot, const char* who, const CorruptSpec& spec, const int32_t* src_hw, hipStream_t stream,
                    char* errbuf, size_t errcap);
// Device half, after corrupt_prepare: the frames at `buf` run through their chains on `stream`; *result is where they end up
// (`buf` after an even number of op slots, slot.scratch after an odd one).
int corrupt_enqueue(CorruptSlot& slot, const char* who, const CorruptSpec& spec, uint8_t* buf, hipStream_t stream, uint8_t** result,
                    char* errbuf, size_t errcap);

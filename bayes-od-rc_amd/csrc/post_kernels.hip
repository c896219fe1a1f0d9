// Bayesian post-processing on the device: everything `bayes_od_inference` does after the model
// call and all of `bayes_od_clustering` (src/retina_net/experiments/inference_utils.py:25-215,
// :285-364).  fp32 throughout, like the reference.
//
//   K1 post_sample_kernel   softmax per MC sample -> mean -> Categorical.sample(30) via Philox
//                           uniforms -> counts -> background filter flag            (:31-51)
//   K2 post_scan_kernel     ordered compaction offsets (tf.boolean_mask keeps anchor order)
//   K3 post_fuse_kernel     per kept anchor: decode, mean / 4x4 sample covariance over MC,
//                           aleatoric L D L^T, mixing, Dirichlet + Gaussian prior fusion,
//                           KITTI rescale, score ranking, corners                    (:25-29,:53-202)
//   K4 nms_kernel           NonMaxSuppressionV5 (soft-NMS), one wavefront per image   (:204-212)
//   K5 cluster_fuse_kernel  bayes_od_clustering, one workgroup per (image, centre)   (:285-364)
//      cluster_merge_kernel in its place under bod_set_merge_method: the NMS pick / the Gaussian mixture (no reference counterpart)
//   K6 iou_matrix_kernel    box_utils.bbox_iou_vuvu (only for API compatibility)     (:214-215)
//   black-box MC dropout (bod_set_uncertainty_method, no reference counterpart in this release): bb_flag_kernel / bb_compact_kernel /
//      bb_gather_kernel beside the validation kernels -- K4 per (image, sample) -- and bb_merge_kernel behind cluster_merge_kernel
#include "kernels.h"
#include "philox.h"
#include "record_state.h"
#include <algorithm>
#include <math.h>

#define POST_BLOCK 256
#define MAXC 16

// ------------------------------------------------------------------------------------------------
// small dense helpers (all indices compile-time after unrolling)
// ------------------------------------------------------------------------------------------------
struct Mat4 { float m[4][4]; };

// inverse of a symmetric positive definite 4x4 through Cholesky A = G G^T, inv = G^-T G^-1
__device__ __forceinline__ Mat4 inv_spd4_once(const Mat4& a) {
    float g[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) g[i][j] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float d = a.m[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= g[j][k] * g[j][k];
        const float dj = sqrtf(d);
        g[j][j] = dj;
        const float inv = 1.0f / dj;
#pragma unroll
        for (int i = j + 1; i < 4; ++i) {
            float s = a.m[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= g[i][k] * g[j][k];
            g[i][j] = s * inv;
        }
    }
    // h = G^-1 (lower)
    float h[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) h[i][j] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        h[j][j] = 1.0f / g[j][j];
#pragma unroll
        for (int i = j + 1; i < 4; ++i) {
            float s = 0.f;
#pragma unroll
            for (int k = j; k < i; ++k) s += g[i][k] * h[k][j];
            h[i][j] = -s / g[i][i];
        }
    }
    Mat4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            float s = 0.f;
#pragma unroll
            for (int k = i; k < 4; ++k) s += h[k][i] * h[k][j];
            r.m[i][j] = s;
            r.m[j][i] = s;
        }
    return r;
}

// DESIGN.md 8.4 (round 6): this file -- like every source of the library -- is compiled WITHOUT the SLP vectoriser (bayes_od_rc_amd/build.py: -fno-slp-vectorize), i.e. without
// packed fp32 instructions (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32).  With them, post_fuse_kernel and cluster_fuse_kernel -- the 4x4
// inverses and matrix-vector products, which the vectoriser packs two floats at a time -- returned wrong results in lanes 48-63 of a wave
// whenever a convolution kernel of the library shared the compute unit (0.2-10 % of the waves in the self-check build,
// tests/tools/selfcheck_probe.py; never alone; never on disjoint CUs); without them: 0 of 56 million waves, and the canary test
// (tests/test_gpu_zz_canary.py) passes.  Same IEEE operations either way: results are bit-identical to the packed build's when nothing
// runs beside it.  (A round-6 interim form evaluated the inverse until two consecutive evaluations agreed: it removed 85 % of the events,
// not all -- the products behind the inverse are packed too.)
__device__ __forceinline__ Mat4 inv_spd4(const Mat4& a) { return inv_spd4_once(a); }

__device__ __forceinline__ void decode_box(const float4 anc, const float4 t, float o[4]) {
    // box_utils.box_from_anchor_and_target_bnms (:171-192): anchors (v,u,h,w)
    o[0] = anc.z * t.x / 10.0f + anc.x;
    o[1] = anc.w * t.y / 10.0f + anc.y;
    o[2] = anc.z * fminf(fmaxf(expf(t.z / 5.0f), 1e-4f), 1e4f);
    o[3] = anc.w * fminf(fmaxf(expf(t.w / 5.0f), 1e-4f), 1e4f);
}

// ------------------------------------------------------------------------------------------------
// K1: mean softmax + categorical sampling + filter flag
// ------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(POST_BLOCK) void post_sample_kernel(PostCfg c, PostBuffers pb, int nblocks) {
    const int a = blockIdx.x * POST_BLOCK + threadIdx.x;
    const int b = blockIdx.y;
    bool keep = false;
    if (a < c.A) {
        float mp[C];
#pragma unroll
        for (int j = 0; j < C; ++j) mp[j] = 0.f;
        if (c.aggregated) {                 // sum_n softmax from the head epilogue (conv_igemm.hip agg_reduce_cls: the loop below, fused)
            const float* l = pb.agg_cls + ((size_t)b * c.A + a) * C;
#pragma unroll
            for (int j = 0; j < C; ++j) mp[j] = l[j];
        }
        for (int n = 0; n < (c.aggregated ? 0 : c.N); ++n) {
            const float* l = pb.cls + (((size_t)b * c.N + n) * c.A + a) * C;
            float v[C];
            if (C % 4 == 0) {
#pragma unroll
                for (int q = 0; q < C / 4; ++q) {
                    const float4 t = reinterpret_cast<const float4*>(l)[q];
                    v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < C; ++j) v[j] = l[j];
            }
            float mx = v[0];
#pragma unroll
            for (int j = 1; j < C; ++j) mx = fmaxf(mx, v[j]);
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < C; ++j) { v[j] = expf(v[j] - mx); s += v[j]; }
#pragma unroll
            for (int j = 0; j < C; ++j) mp[j] += v[j] / s;
        }
        float cdf[C];
        float accum = 0.f;
#pragma unroll
        for (int j = 0; j < C; ++j) { mp[j] = mp[j] / (float)c.N; accum += mp[j]; cdf[j] = accum; }
        const float total = cdf[C - 1];
        int cnt[C];
#pragma unroll
        for (int j = 0; j < C; ++j) cnt[j] = 0;
        const int groups = (c.draws + 3) / 4;
        for (int g = 0; g < groups; ++g) {
            const Philox4 r = philox4x32_10((uint32_t)a, (uint32_t)g, BOD_CAT_TAG, c.image_base + b,
                                            c.seed_lo, c.seed_hi);
            const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (4 * g + q < c.draws) {
                    const float t = (float)(w[q] >> 8) * 5.9604644775390625e-8f * total;
                    int k = 0;
#pragma unroll
                    for (int j = 0; j < C; ++j) k += (cdf[j] <= t) ? 1 : 0;
                    k = k < C - 1 ? k : C - 1;
#pragma unroll
                    for (int j = 0; j < C; ++j) cnt[j] += (j == k) ? 1 : 0;
                }
            }
        }
        int best = 0, bestc = cnt[0];
#pragma unroll
        for (int j = 1; j < C; ++j)
            if (cnt[j] > bestc) { bestc = cnt[j]; best = j; }
        keep = best != C - 1;
        pb.keep[(size_t)b * c.A + a] = keep ? 1 : 0;
        float* dc = pb.d_counts + ((size_t)b * c.A + a) * C;
#pragma unroll
        for (int j = 0; j < C; ++j) dc[j] = (float)cnt[j];
    }
    const int n = __syncthreads_count(keep ? 1 : 0);
    if (threadIdx.x == 0) pb.block_counts[(size_t)b * nblocks + blockIdx.x] = n;
}

// K2: exclusive scan of block counts (in place), one block per image
__global__ __launch_bounds__(POST_BLOCK) void post_scan_kernel(PostBuffers pb, int nblocks) {
    __shared__ int part[POST_BLOCK];
    const int b = blockIdx.x, tid = threadIdx.x;
    int* bc = pb.block_counts + (size_t)b * nblocks;
    const int per = (nblocks + POST_BLOCK - 1) / POST_BLOCK;
    int local = 0;
    for (int i = 0; i < per; ++i) {
        const int idx = tid * per + i;
        if (idx < nblocks) local += bc[idx];
    }
    part[tid] = local;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < POST_BLOCK; ++i) { const int t = part[i]; part[i] = run; run += t; }
        pb.num_kept[b] = run;
    }
    __syncthreads();
    int run = part[tid];
    for (int i = 0; i < per; ++i) {
        const int idx = tid * per + i;
        if (idx < nblocks) { const int t = bc[idx]; bc[idx] = run; run += t; }
    }
}

// K3a (round 4): the ordered compaction alone -- every kept anchor writes its index to its slot.  The per-anchor work below then runs
// over the COMPACT list: with ~2 % of the anchors kept, a wave of the one-thread-per-anchor form ran the whole posterior (three 4x4
// inverses, the aleatoric L D L^T, the prior fusion) for one or two active lanes -- 0.61 ms per 512 frames on the main stream.
__global__ __launch_bounds__(POST_BLOCK) void post_compact_kernel(PostCfg c, PostBuffers pb, int nblocks) {
    __shared__ int wave_off[POST_BLOCK / 64 + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a = blockIdx.x * POST_BLOCK + tid;
    const int b = blockIdx.y;
    const bool keep = (a < c.A) && pb.keep[(size_t)b * c.A + a];
    const unsigned long long bal = __ballot(keep);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wave_off[wave + 1] = __popcll(bal);
    if (tid == 0) wave_off[0] = 0;
    __syncthreads();
    if (tid == 0)
        for (int w = 1; w <= POST_BLOCK / 64; ++w) wave_off[w] += wave_off[w - 1];
    __syncthreads();
    if (!keep) return;
    const int slot = pb.block_counts[(size_t)b * nblocks + blockIdx.x] + wave_off[wave] + before;
    pb.anchor_index[(size_t)b * c.A + slot] = a;
}

// K3: per kept anchor fusion, written straight to its compacted slot
// BOD_POST_SELFCHECK (development build, tests/tools/build_variant.sh + selfcheck_probe.py): every slot is computed TWICE
// in the same thread through ONE out-of-line copy of the code -- the same machine instructions on the same inputs -- and the two
// results are compared bit for bit; a difference is logged with where the wave ran (HW_REG_HW_ID: SIMD / CU / SE, HW_REG_XCC_ID).
#if defined(BOD_POST_SELFCHECK)
#define POST_FUSE_INLINE __noinline__
#if BOD_POST_SELFCHECK == 2
// variant 2: the slot's inputs are loaded ONCE by the kernel and handed to the out-of-line copy in registers; the copy neither loads nor
// stores (pure VALU between call and return) -- does the difference between two computations survive without memory operations?
struct FuseIn { float4 anc, ab[4]; float2 cv[5]; float dc[8]; };
#define POST_FUSE_OUT , float* __restrict__ out20, const FuseIn& fin
#else
#define POST_FUSE_OUT , float* __restrict__ out20
#endif
struct SelfcheckRec { uint32_t hw_id, xcc_id, image, slot, lane, elem; float first, second; };
__device__ unsigned int g_selfcheck_count;
__device__ unsigned long long g_selfcheck_waves;          // waves that ran the check (the rate's denominator)
__device__ SelfcheckRec g_selfcheck_recs[4096];
#else
#define POST_FUSE_INLINE __forceinline__
#define POST_FUSE_OUT
#endif
template <int C>
__device__ POST_FUSE_INLINE void post_fuse_anchor(const PostCfg& c, const PostBuffers& pb, const int b, const int slot POST_FUSE_OUT) {
    const size_t o = (size_t)b * c.A + slot;
#if defined(BOD_POST_SELFCHECK) && BOD_POST_SELFCHECK == 2
    const int a = 0; (void)a; (void)o;
    const float4 anc = fin.anc;
#else
    const int a = pb.anchor_index[o];

    const float4 anc = reinterpret_cast<const float4*>(pb.anchors)[a];
#endif
    // ---- epistemic: two-pass mean / unbiased covariance over MC samples (:220-244)
    float mu[4] = {0.f, 0.f, 0.f, 0.f};
    Mat4 epi;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) epi.m[i][j] = 0.f;
    const int n_raw = c.aggregated ? 0 : c.N;
    if (c.aggregated) {                     // Welford mean and co-moment sums from the head epilogue (agg_reduce_box)
#if defined(BOD_POST_SELFCHECK) && BOD_POST_SELFCHECK == 2
        const float4* ab = fin.ab;
#else
        const float4* ab = reinterpret_cast<const float4*>(pb.agg_box) + ((size_t)b * c.A + a) * 4;
#endif
        const float4 m = ab[0], q0 = ab[1], q1 = ab[2], q2 = ab[3];
        mu[0] = m.x; mu[1] = m.y; mu[2] = m.z; mu[3] = m.w;
        epi.m[0][0] = q0.x; epi.m[1][0] = q0.y; epi.m[1][1] = q0.z; epi.m[2][0] = q0.w;
        epi.m[2][1] = q1.x; epi.m[2][2] = q1.y; epi.m[3][0] = q1.z; epi.m[3][1] = q1.w;
        epi.m[3][2] = q2.x; epi.m[3][3] = q2.y;
    }
    for (int n = 0; n < n_raw; ++n) {
        const float4 t = reinterpret_cast<const float4*>(pb.box)[((size_t)b * c.N + n) * c.A + a];
        float bx[4];
        decode_box(anc, t, bx);
#pragma unroll
        for (int i = 0; i < 4; ++i) mu[i] += bx[i];
    }
    if (!c.aggregated) {
#pragma unroll
        for (int i = 0; i < 4; ++i) mu[i] = mu[i] / (float)c.N;
    }
    for (int n = 0; n < n_raw; ++n) {
        const float4 t = reinterpret_cast<const float4*>(pb.box)[((size_t)b * c.N + n) * c.A + a];
        float bx[4];
        decode_box(anc, t, bx);
#pragma unroll
        for (int i = 0; i < 4; ++i) bx[i] -= mu[i];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) epi.m[i][j] += bx[i] * bx[j];
    }
    const float nm1 = (float)c.N - 1.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) { epi.m[i][j] = epi.m[i][j] / nm1; epi.m[j][i] = epi.m[i][j]; }

#if defined(BOD_POST_SELFCHECK_PART) && BOD_POST_SELFCHECK_PART == 1          // (bisection of the self-check: stop behind the epistemic block)
    for (int i = 0; i < 4; ++i) { out20[i] = mu[i]; for (int j = 0; j < 4; ++j) out20[4 + i * 4 + j] = epi.m[i][j]; }
    return;
#endif
    // ---- aleatoric (:62-84): mean of the raw lower-triangular params, D = exp(diag), L = inv(unit lower)
    Mat4 al;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) al.m[i][j] = 0.f;
    if (c.has_covar) {
        float x[10];
#pragma unroll
        for (int q = 0; q < 10; ++q) x[q] = 0.f;
        if (c.aggregated) {                 // sum_n of the raw parameters from the head epilogue (agg_reduce_cov)
#if defined(BOD_POST_SELFCHECK) && BOD_POST_SELFCHECK == 2
            const float* p = reinterpret_cast<const float*>(fin.cv);
#else
            const float* p = pb.agg_cov + ((size_t)b * c.A + a) * 10;
#endif
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const float2 t = reinterpret_cast<const float2*>(p)[q];
                x[2 * q] = t.x; x[2 * q + 1] = t.y;
            }
        }
        for (int n = 0; n < n_raw; ++n) {
            const float* p = pb.cov + (((size_t)b * c.N + n) * c.A + a) * 10;
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const float2 t = reinterpret_cast<const float2*>(p)[q];
                x[2 * q] += t.x; x[2 * q + 1] += t.y;
            }
        }
#pragma unroll
        for (int q = 0; q < 10; ++q) x[q] = x[q] / (float)c.N;
        // tfp.math.fill_triangular (retinanet_model.py:110)
        const float d0 = expf(x[4]), d1 = expf(x[9]), d2 = expf(x[5]), d3 = expf(x[0]);
        if (c.use_full_covar) {
            const float l10 = x[8], l20 = x[7], l21 = x[6], l30 = x[3], l31 = x[2], l32 = x[1];
            // inverse of the unit lower matrix by forward substitution
            float li[4][4];
            li[0][0] = 1.f; li[0][1] = 0.f; li[0][2] = 0.f; li[0][3] = 0.f;
            li[1][0] = -l10; li[1][1] = 1.f; li[1][2] = 0.f; li[1][3] = 0.f;
            li[2][0] = -(l20 * 1.f + l21 * li[1][0]); li[2][1] = -l21; li[2][2] = 1.f; li[2][3] = 0.f;
            li[3][0] = -(l30 * 1.f + l31 * li[1][0] + l32 * li[2][0]);
            li[3][1] = -(l31 * 1.f + l32 * li[2][1]);
            li[3][2] = -l32; li[3][3] = 1.f;
            const float d[4] = {d0, d1, d2, d3};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j) {
                    float s = 0.f;
#pragma unroll
                    for (int k = 0; k <= j; ++k) s += li[i][k] * d[k] * li[j][k];
                    al.m[i][j] = s; al.m[j][i] = s;
                }
        } else {
            al.m[0][0] = d0; al.m[1][1] = d1; al.m[2][2] = d2; al.m[3][3] = d3;
        }
    }
#if defined(BOD_POST_SELFCHECK_PART) && BOD_POST_SELFCHECK_PART == 2          // ... behind the aleatoric block (exp, unit-lower inverse, L D L^T)
    for (int i = 0; i < 4; ++i) { out20[i] = mu[i]; for (int j = 0; j < 4; ++j) out20[4 + i * 4 + j] = al.m[i][j]; }
    return;
#endif
    Mat4 lik;                                                     // (:86-87)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) lik.m[i][j] = (10.0f * al.m[i][j] + 1.0f * epi.m[i][j]) / 11.0f;

    // ---- Dirichlet posterior (:90-97)
#if defined(BOD_POST_SELFCHECK) && BOD_POST_SELFCHECK == 2
    const float* dc = fin.dc;
#else
    const float* dc = pb.d_counts + ((size_t)b * c.A + a) * C;
#endif
    float pc[C];
    float csum = 0.f;
    const float alpha = c.dirichlet ? 1.0f / (float)C : 0.f;
#pragma unroll
    for (int j = 0; j < C; ++j) { pc[j] = dc[j] + alpha; csum += pc[j]; }
    float best = 0.f;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        const float s = pc[j] / csum;
#if !(defined(BOD_POST_SELFCHECK) && BOD_POST_SELFCHECK == 2)
        pb.counts[o * C + j] = pc[j];
        pb.score[o * C + j] = s;
#endif
        best = j == 0 ? s : fmaxf(best, s);
    }

#if defined(BOD_POST_SELFCHECK_PART) && BOD_POST_SELFCHECK_PART == 3          // ... behind the likelihood mix and the Dirichlet scores
    for (int i = 0; i < 4; ++i) { out20[i] = mu[i] + best; for (int j = 0; j < 4; ++j) out20[4 + i * 4 + j] = lik.m[i][j]; }
    return;
#endif
    // ---- Gaussian prior fusion (:100-145): prior mean = the anchor, prior cov = iso_var * I
    Mat4 pcov;
    float pm[4];
    if (c.gaussian_iso) {
        const Mat4 prec = inv_spd4(lik);
        const float pp = 1.0f / c.iso_var;
        Mat4 post_prec = prec;
#pragma unroll
        for (int i = 0; i < 4; ++i) post_prec.m[i][i] += pp;
        pcov = inv_spd4(post_prec);
        const float am[4] = {anc.x, anc.y, anc.z, anc.w};
        float inter[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) s += prec.m[i][k] * mu[k];
            inter[i] = pp * am[i] + s;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) s += pcov.m[i][k] * inter[k];
            pm[i] = s;
        }
    } else {
        pcov = lik;
#pragma unroll
        for (int i = 0; i < 4; ++i) pm[i] = mu[i];
    }
    if (c.kitti_sh > 0.f) {                                       // (:147-167) S mu, S Sigma S^T
        float ksh = c.kitti_sh, ksw = c.kitti_sw;
        if (c.kitti_frame) { ksh = c.kitti_frame[2 * b]; ksw = c.kitti_frame[2 * b + 1]; }      // the frame's own S = orig / net
        const float sc[4] = {ksh, ksw, ksh, ksw};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            pm[i] *= sc[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) pcov.m[i][j] = sc[i] * pcov.m[i][j] * sc[j];
        }
    }
#if !(defined(BOD_POST_SELFCHECK) && BOD_POST_SELFCHECK == 2)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        pb.means[o * 4 + i] = pm[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) pb.covs[o * 16 + i * 4 + j] = pcov.m[i][j];
    }
#endif
#if defined(BOD_POST_SELFCHECK)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        out20[i] = pm[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) out20[4 + i * 4 + j] = pcov.m[i][j];
    }
#endif
#if defined(BOD_POST_SELFCHECK) && BOD_POST_SELFCHECK == 2
    out20[0] += best * 0.f;
    return;
#else
    pb.ranking[o] = best;                                         // ranking_method 'score' (:202)
    // box_utils.vuhw_to_vuvu (:5-23)
    pb.corners[o * 4 + 0] = pm[0] - pm[2] / 2.0f;
    pb.corners[o * 4 + 1] = pm[1] - pm[3] / 2.0f;
    pb.corners[o * 4 + 2] = pm[0] + pm[2] / 2.0f;
    pb.corners[o * 4 + 3] = pm[1] + pm[3] / 2.0f;
#endif
}

// a few blocks per image walk its compact list (POST_FUSE_BLOCKS x 256 slots per pass: one pass up to 2 048 kept anchors)
#define POST_FUSE_BLOCKS 8
template <int C>
__global__ __launch_bounds__(POST_BLOCK) void post_fuse_kernel(PostCfg c, PostBuffers pb, int nblocks) {
    const int b = blockIdx.y;
    const int m = pb.num_kept[b];
#if defined(BOD_POST_SELFCHECK)
    for (int slot = blockIdx.x * POST_BLOCK + threadIdx.x; slot < m; slot += gridDim.x * POST_BLOCK) {
        float r1[20], r2[20];
#if BOD_POST_SELFCHECK == 2
        FuseIn fin;
        {
            const size_t o = (size_t)b * c.A + slot;
            const int a = pb.anchor_index[o];
            fin.anc = reinterpret_cast<const float4*>(pb.anchors)[a];
            for (int q = 0; q < 4; ++q) fin.ab[q] = (reinterpret_cast<const float4*>(pb.agg_box) + ((size_t)b * c.A + a) * 4)[q];
            for (int q = 0; q < 5; ++q) fin.cv[q] = reinterpret_cast<const float2*>(pb.agg_cov + ((size_t)b * c.A + a) * 10)[q];
            for (int q = 0; q < 8; ++q) fin.dc[q] = q < C ? pb.d_counts[((size_t)b * c.A + a) * C + q] : 0.f;
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        post_fuse_anchor<C>(c, pb, b, slot, r1, fin);
        post_fuse_anchor<C>(c, pb, b, slot, r2, fin);
#else
        post_fuse_anchor<C>(c, pb, b, slot, r1);
        post_fuse_anchor<C>(c, pb, b, slot, r2);
#endif
        if ((threadIdx.x & 63) == 0) atomicAdd(&g_selfcheck_waves, 1ull);
        int bad = -1;
        for (int i = 19; i >= 0; --i) if (__float_as_uint(r1[i]) != __float_as_uint(r2[i])) bad = i;
        if (bad >= 0) {
            const unsigned int k = atomicAdd(&g_selfcheck_count, 1u);
            if (k < 4096u) {
                SelfcheckRec r;
                r.hw_id = __builtin_amdgcn_s_getreg((31 << 11) | 4);          // HW_REG_HW_ID, all 32 bits
                r.xcc_id = __builtin_amdgcn_s_getreg((31 << 11) | 20);        // HW_REG_XCC_ID
                r.image = (uint32_t)b; r.slot = (uint32_t)slot; r.lane = threadIdx.x & 63; r.elem = (uint32_t)bad;
                r.first = r1[bad]; r.second = r2[bad];
                g_selfcheck_recs[k] = r;
            }
        }
    }
#else
    for (int slot = blockIdx.x * POST_BLOCK + threadIdx.x; slot < m; slot += gridDim.x * POST_BLOCK) post_fuse_anchor<C>(c, pb, b, slot);
#endif
}
#if defined(BOD_POST_SELFCHECK)
// (development builds only: not in include/bayesod.h)  count of mismatching slots since the last call, the waves that ran the check, up to
// `max` records of 8 dwords {hw_id, xcc_id, image, slot, lane, element, first, second}; resets the log.
extern "C" int bod_debug_selfcheck_read(unsigned int* count, unsigned long long* waves, void* recs, int max) {
    unsigned int n = 0;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_selfcheck_count), 4) != hipSuccess) return 1;
    if (hipMemcpyFromSymbol(waves, HIP_SYMBOL(g_selfcheck_waves), 8) != hipSuccess) return 1;
    const unsigned int m = n < (unsigned)max ? n : (unsigned)max;
    if (m && hipMemcpyFromSymbol(recs, HIP_SYMBOL(g_selfcheck_recs), (size_t)(m < 4096u ? m : 4096u) * sizeof(SelfcheckRec)) != hipSuccess) return 1;
    const unsigned int z = 0; const unsigned long long z8 = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_selfcheck_count), &z, 4) != hipSuccess || hipMemcpyToSymbol(HIP_SYMBOL(g_selfcheck_waves), &z8, 8) != hipSuccess) return 1;
    *count = n;
    return 0;
}
#endif

hipError_t launch_posterior_keep(const PostCfg& c, const PostBuffers& b, hipStream_t s) {
    const int nblocks = (c.A + POST_BLOCK - 1) / POST_BLOCK;
    dim3 grid(nblocks, c.B);
    if (c.C == 8) hipLaunchKernelGGL(post_sample_kernel<8>, grid, dim3(POST_BLOCK), 0, s, c, b, nblocks);
    else if (c.C == 4) hipLaunchKernelGGL(post_sample_kernel<4>, grid, dim3(POST_BLOCK), 0, s, c, b, nblocks);
    else return hipErrorInvalidValue;
    hipLaunchKernelGGL(post_scan_kernel, dim3(c.B), dim3(POST_BLOCK), 0, s, b, nblocks);
    return hipGetLastError();
}

hipError_t launch_posterior_fuse(const PostCfg& c, const PostBuffers& b, hipStream_t s) {
    const int nblocks = (c.A + POST_BLOCK - 1) / POST_BLOCK;
    dim3 grid(nblocks, c.B);
    if (c.C != 8 && c.C != 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(post_compact_kernel, grid, dim3(POST_BLOCK), 0, s, c, b, nblocks);
    if (c.C == 8) hipLaunchKernelGGL(post_fuse_kernel<8>, dim3(std::min(nblocks, POST_FUSE_BLOCKS), c.B), dim3(POST_BLOCK), 0, s, c, b, nblocks);
    else hipLaunchKernelGGL(post_fuse_kernel<4>, dim3(std::min(nblocks, POST_FUSE_BLOCKS), c.B), dim3(POST_BLOCK), 0, s, c, b, nblocks);
    return hipGetLastError();
}

hipError_t launch_posterior(const PostCfg& c, const PostBuffers& b, hipStream_t s) {
    const hipError_t e = launch_posterior_keep(c, b, s);
    return e != hipSuccess ? e : launch_posterior_fuse(c, b, s);
}

// ------------------------------------------------------------------------------------------------
// Covariance parts, per kept anchor (bod_config.covariance_parts; kernels.h).  post_fuse_anchor mixes
// lik = (10 A + E) / 11 and fuses the prior iso_var * I: P = (lik^-1 + I / iso_var)^-1.  The posterior mean is linear in the
// likelihood's mean with gain G = P lik^-1 = (I + lik / iso_var)^-1, so P = G (E / 11) G^T + G (10 A / 11) G^T + P P / iso_var exactly.
// This kernel runs behind post_fuse_kernel on parts handles only: it rebuilds E and A from the inputs post_fuse_anchor read, with
// its operations in its order (the two blocks below restate that function's; it is left as it was, so the default handle's bits
// cannot move) and writes the three lower triangles.
// ------------------------------------------------------------------------------------------------
// lower triangle of G X G^T (X symmetric) scaled like the covariance: out[t] = sc_i * (G X G^T)_ij * sc_j
__device__ __forceinline__ void parts_congruence(const Mat4& g, const Mat4& x, const float sc[4], float* __restrict__ out) {
    Mat4 t;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) s += g.m[i][k] * x.m[k][j];
            t.m[i][j] = s;
        }
    int q = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) s += t.m[i][k] * g.m[j][k];
            out[q++] = sc[i] * s * sc[j];
        }
}

__global__ __launch_bounds__(POST_BLOCK) void post_parts_kernel(PostCfg c, PostBuffers pb, float* __restrict__ parts) {
    const int b = blockIdx.y;
    const int m = pb.num_kept[b];
    for (int slot = blockIdx.x * POST_BLOCK + threadIdx.x; slot < m; slot += gridDim.x * POST_BLOCK) {
        const size_t o = (size_t)b * c.A + slot;
        const int a = pb.anchor_index[o];
        const float4 anc = reinterpret_cast<const float4*>(pb.anchors)[a];
        // ---- E: post_fuse_anchor's epistemic block
        float mu[4] = {0.f, 0.f, 0.f, 0.f};
        Mat4 epi;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) epi.m[i][j] = 0.f;
        const int n_raw = c.aggregated ? 0 : c.N;
        if (c.aggregated) {
            const float4* ab = reinterpret_cast<const float4*>(pb.agg_box) + ((size_t)b * c.A + a) * 4;
            const float4 q0 = ab[1], q1 = ab[2], q2 = ab[3];
            epi.m[0][0] = q0.x; epi.m[1][0] = q0.y; epi.m[1][1] = q0.z; epi.m[2][0] = q0.w;
            epi.m[2][1] = q1.x; epi.m[2][2] = q1.y; epi.m[3][0] = q1.z; epi.m[3][1] = q1.w;
            epi.m[3][2] = q2.x; epi.m[3][3] = q2.y;
        }
        for (int n = 0; n < n_raw; ++n) {
            const float4 t = reinterpret_cast<const float4*>(pb.box)[((size_t)b * c.N + n) * c.A + a];
            float bx[4];
            decode_box(anc, t, bx);
#pragma unroll
            for (int i = 0; i < 4; ++i) mu[i] += bx[i];
        }
        if (!c.aggregated) {
#pragma unroll
            for (int i = 0; i < 4; ++i) mu[i] = mu[i] / (float)c.N;
        }
        for (int n = 0; n < n_raw; ++n) {
            const float4 t = reinterpret_cast<const float4*>(pb.box)[((size_t)b * c.N + n) * c.A + a];
            float bx[4];
            decode_box(anc, t, bx);
#pragma unroll
            for (int i = 0; i < 4; ++i) bx[i] -= mu[i];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j) epi.m[i][j] += bx[i] * bx[j];
        }
        const float nm1 = (float)c.N - 1.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) { epi.m[i][j] = epi.m[i][j] / nm1; epi.m[j][i] = epi.m[i][j]; }
        // ---- A: post_fuse_anchor's aleatoric block
        Mat4 al;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) al.m[i][j] = 0.f;
        if (c.has_covar) {
            float x[10];
#pragma unroll
            for (int q = 0; q < 10; ++q) x[q] = 0.f;
            if (c.aggregated) {
                const float* p = pb.agg_cov + ((size_t)b * c.A + a) * 10;
#pragma unroll
                for (int q = 0; q < 5; ++q) {
                    const float2 t = reinterpret_cast<const float2*>(p)[q];
                    x[2 * q] = t.x; x[2 * q + 1] = t.y;
                }
            }
            for (int n = 0; n < n_raw; ++n) {
                const float* p = pb.cov + (((size_t)b * c.N + n) * c.A + a) * 10;
#pragma unroll
                for (int q = 0; q < 5; ++q) {
                    const float2 t = reinterpret_cast<const float2*>(p)[q];
                    x[2 * q] += t.x; x[2 * q + 1] += t.y;
                }
            }
#pragma unroll
            for (int q = 0; q < 10; ++q) x[q] = x[q] / (float)c.N;
            const float d0 = expf(x[4]), d1 = expf(x[9]), d2 = expf(x[5]), d3 = expf(x[0]);
            if (c.use_full_covar) {
                const float l10 = x[8], l20 = x[7], l21 = x[6], l30 = x[3], l31 = x[2], l32 = x[1];
                float li[4][4];
                li[0][0] = 1.f; li[0][1] = 0.f; li[0][2] = 0.f; li[0][3] = 0.f;
                li[1][0] = -l10; li[1][1] = 1.f; li[1][2] = 0.f; li[1][3] = 0.f;
                li[2][0] = -(l20 * 1.f + l21 * li[1][0]); li[2][1] = -l21; li[2][2] = 1.f; li[2][3] = 0.f;
                li[3][0] = -(l30 * 1.f + l31 * li[1][0] + l32 * li[2][0]);
                li[3][1] = -(l31 * 1.f + l32 * li[2][1]);
                li[3][2] = -l32; li[3][3] = 1.f;
                const float d[4] = {d0, d1, d2, d3};
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j <= i; ++j) {
                        float s = 0.f;
#pragma unroll
                        for (int k = 0; k <= j; ++k) s += li[i][k] * d[k] * li[j][k];
                        al.m[i][j] = s; al.m[j][i] = s;
                    }
            } else {
                al.m[0][0] = d0; al.m[1][1] = d1; al.m[2][2] = d2; al.m[3][3] = d3;
            }
        }
        // ---- the two likelihood terms: lik = e + a
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) { epi.m[i][j] = epi.m[i][j] / 11.0f; al.m[i][j] = 10.0f * al.m[i][j] / 11.0f; }
        // ---- the gain G = P lik^-1 = (I + lik / iso_var)^-1 and P = G lik.  I + lik / iso_var is SPD with every eigenvalue >= 1, so this
        // inverse is well conditioned whatever lik is -- also where lik^-1, and with it the stored P, is beyond fp32 (a rank-deficient
        // sample covariance without the covariance head) -- which is why P is formed here and not read back (nor unscaled on KITTI)
        float sc[4] = {1.f, 1.f, 1.f, 1.f};
        if (c.kitti_sh > 0.f) {
            float ksh = c.kitti_sh, ksw = c.kitti_sw;
            if (c.kitti_frame) { ksh = c.kitti_frame[2 * b]; ksw = c.kitti_frame[2 * b + 1]; }
            sc[0] = ksh; sc[1] = ksw; sc[2] = ksh; sc[3] = ksw;
        }
        Mat4 g, pp;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) { g.m[i][j] = i == j ? 1.f : 0.f; pp.m[i][j] = 0.f; }
        if (c.gaussian_iso) {
            Mat4 lik, t;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) { lik.m[i][j] = epi.m[i][j] + al.m[i][j]; t.m[i][j] = g.m[i][j] + lik.m[i][j] / c.iso_var; }
            g = inv_spd4(t);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float s = 0.f;
#pragma unroll
                    for (int k = 0; k < 4; ++k) s += g.m[i][k] * lik.m[k][j];
                    t.m[i][j] = s;                                  // P
                }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j) {
                    float s = 0.f;
#pragma unroll
                    for (int k = 0; k < 4; ++k) s += t.m[i][k] * t.m[j][k];
                    pp.m[i][j] = s / c.iso_var; pp.m[j][i] = pp.m[i][j];
                }
        }
        float* out = parts + o * BOD_PARTS_TRI;
        parts_congruence(g, epi, sc, out);
        if (c.has_covar) {
            parts_congruence(g, al, sc, out + 10);
        } else {
#pragma unroll
            for (int q = 0; q < 10; ++q) out[10 + q] = 0.f;
        }
        int q = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) out[20 + q++] = sc[i] * pp.m[i][j] * sc[j];
    }
}

hipError_t launch_posterior_parts(const PostCfg& c, const PostBuffers& b, float* parts, hipStream_t s) {
    if (!parts) return hipErrorInvalidValue;
    const int nblocks = (c.A + POST_BLOCK - 1) / POST_BLOCK;
    hipLaunchKernelGGL(post_parts_kernel, dim3(std::min(nblocks, POST_FUSE_BLOCKS), c.B), dim3(POST_BLOCK), 0, s, c, b, parts);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Class-entropy parts, per kept anchor (bod_config.covariance_parts bit BOD_PARTS_CLASS; kernels.h).  With K samples
// behind the class statistics and pbar = cls_sum / K (post_sample_kernel's mean):
//   aleatoric = ent_sum / K        total = -sum_j pbar_j log pbar_j  (0 log 0 = 0)        epistemic = max(total - aleatoric, 0)
// the mutual information between the class and the weights.  ent_sum = sum_n H(softmax(logits_n)) comes from the head epilogue
// (conv_igemm.hip agg_reduce_cls<C, true>) or the statistics record when the posterior is aggregated; on the raw route this kernel
// walks the samples itself with that function's operations in its order, so the two routes agree bit for bit.  One thread per kept
// slot behind post_fuse_kernel, which -- like post_sample_kernel -- is left as it was.
// ------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(POST_BLOCK) void post_class_parts_kernel(PostCfg c, PostBuffers pb, const float* __restrict__ ent_sum,
                                                                      float* __restrict__ cparts) {
    const int b = blockIdx.y;
    const int m = pb.num_kept[b];
    for (int slot = blockIdx.x * POST_BLOCK + threadIdx.x; slot < m; slot += gridDim.x * POST_BLOCK) {
        const size_t o = (size_t)b * c.A + slot;
        const int a = pb.anchor_index[o];
        float mp[C];
        float ent = 0.f;
#pragma unroll
        for (int j = 0; j < C; ++j) mp[j] = 0.f;
        if (c.aggregated) {
            const float4* l = reinterpret_cast<const float4*>(pb.agg_cls + ((size_t)b * c.A + a) * C);
#pragma unroll
            for (int k = 0; k < C / 4; ++k) {
                const float4 t = l[k];
                mp[4 * k] = t.x; mp[4 * k + 1] = t.y; mp[4 * k + 2] = t.z; mp[4 * k + 3] = t.w;
            }
            ent = ent_sum[(size_t)b * c.A + a];
        }
        for (int n = 0; n < (c.aggregated ? 0 : c.N); ++n) {
            const float* l = pb.cls + (((size_t)b * c.N + n) * c.A + a) * C;
            float v[C];
#pragma unroll
            for (int k = 0; k < C / 4; ++k) {
                const float4 t = reinterpret_cast<const float4*>(l)[k];
                v[4 * k] = t.x; v[4 * k + 1] = t.y; v[4 * k + 2] = t.z; v[4 * k + 3] = t.w;
            }
            float mx = v[0];
#pragma unroll
            for (int j = 1; j < C; ++j) mx = fmaxf(mx, v[j]);
            float sden = 0.f, dot = 0.f;
#pragma unroll
            for (int j = 0; j < C; ++j) { const float d = v[j] - mx; v[j] = expf(d); sden += v[j]; dot += v[j] * d; }
            ent += BOD_LOG_SDEN(sden) - dot / sden;
#pragma unroll
            for (int j = 0; j < C; ++j) mp[j] += v[j] / sden;
        }
        const float fk = (float)c.N;
        float total = 0.f;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            mp[j] = mp[j] / fk;
            if (mp[j] > 0.f) total -= mp[j] * logf(mp[j]);
        }
        const float ale = ent / fk;
        float* out = cparts + o * (3 + C);
        out[0] = total; out[1] = ale; out[2] = fmaxf(total - ale, 0.f);
#pragma unroll
        for (int j = 0; j < C; ++j) out[3 + j] = mp[j];
    }
}

hipError_t launch_posterior_class_parts(const PostCfg& c, const PostBuffers& b, const float* ent_sum, float* cparts, hipStream_t s) {
    if (!cparts || (c.aggregated && !ent_sum) || (c.C != 4 && c.C != 8)) return hipErrorInvalidValue;
    const int nblocks = (c.A + POST_BLOCK - 1) / POST_BLOCK;
    const dim3 grid(std::min(nblocks, POST_FUSE_BLOCKS), c.B);
    if (c.C == 8) hipLaunchKernelGGL(post_class_parts_kernel<8>, grid, dim3(POST_BLOCK), 0, s, c, b, ent_sum, cparts);
    else hipLaunchKernelGGL(post_class_parts_kernel<4>, grid, dim3(POST_BLOCK), 0, s, c, b, ent_sum, cparts);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Sparse tail and halo row tables (kernels.h SparseTailArgs, sparse_tables.h).  One workgroup per image:
//   1. the pixel flags go to LDS, one phase per flag (kept, tail, 3x3 dilation, halo), all threads;
//   2. every thread counts the run starts of both tables in its contiguous share of the pixels, a block scan places them, and the
//      threads list the runs {first, last} in pixel order;
//   3. one wave per table packs the runs into tiles: the packing is a serial recurrence (pieces cut by free slots and extended
//      rows), so all 64 lanes run it in lockstep on 64 runs loaded at a time (one global load per 64 runs, not one per pixel);
//   4. all threads write the pieces' rows and extended rows and pad the tiles.
// Tiles of different images land in the order the images reserve them (atomicAdd): each tile holds one image's pixels with all N
// samples, so the order changes no result.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sparse_tail_rows_kernel(SparseTailArgs a) {
    extern __shared__ uint8_t s_flag[];            // [P]: ST_* bits
    __shared__ int s_cnt[2][256];
    __shared__ int s_nrun[2], s_nchunk[2], s_ntile[2], s_base[2];
    const int b = blockIdx.x, tid = threadIdx.x, N = a.N, P = a.P, B = a.B;
    const int T = a.halo_rows ? 2 : 1;
    const SparseLevels& lv = a.lv;
    const uint8_t* keep = a.keep + (size_t)b * P * a.apl;
    for (int p = tid; p < P; p += blockDim.x) {
        uint8_t f = 0;
        for (int k = 0; k < a.apl; ++k) f |= keep[(size_t)p * a.apl + k];
        s_flag[p] = f ? ST_KEPT : 0;
    }
    __syncthreads();
    for (int p = tid; p < P; p += blockDim.x) if (st_member(s_flag, lv, p, ST_KEPT)) s_flag[p] |= ST_TAIL;
    if (T == 2) {
        __syncthreads();
        for (int p = tid; p < P; p += blockDim.x) if (st_dilated(s_flag, lv, p)) s_flag[p] |= ST_DIL;
        __syncthreads();
        for (int p = tid; p < P; p += blockDim.x) if (st_member(s_flag, lv, p, ST_DIL)) s_flag[p] |= ST_HALO;
    }
    __syncthreads();
    // 2. runs: contiguous shares, block scan of the start counts
    const int share = (P + 255) / 256, q0 = min(P, tid * share), q1 = min(P, q0 + share);
    int cnt[2] = {0, 0};
    for (int t = 0; t < T; ++t) {
        const uint8_t bit = t == 0 ? ST_TAIL : ST_HALO;
        for (int p = q0; p < q1; ++p) cnt[t] += st_run_edge(s_flag, lv, p, bit) & 1;
        s_cnt[t][tid] = cnt[t];
    }
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {             // inclusive Hillis-Steele scan
        int v[2] = {0, 0};
        for (int t = 0; t < T; ++t) v[t] = tid >= d ? s_cnt[t][tid - d] : 0;
        __syncthreads();
        for (int t = 0; t < T; ++t) s_cnt[t][tid] += v[t];
        __syncthreads();
    }
    for (int t = 0; t < T; ++t) {
        const uint8_t bit = t == 0 ? ST_TAIL : ST_HALO;
        int2* runs = a.runs + ((size_t)t * B + b) * P;
        int r = s_cnt[t][tid] - cnt[t];              // runs started in front of this share
        for (int p = q0; p < q1; ++p) {
            const int edge = st_run_edge(s_flag, lv, p, bit);
            if (edge & 1) runs[r++].x = p;
            if (edge & 2) runs[r - 1].y = p;         // (a run that ends here started here or in front)
        }
        if (tid == 255) s_nrun[t] = s_cnt[t][255];
    }
    __syncthreads();
    // 3. packing: wave t packs table t
    const int wave = tid >> 6, lane = tid & 63;
    if (wave < T) {
        const int t = wave;
        const int2* runs = a.runs + ((size_t)t * B + b) * P;
        StQuad* chunks = a.chunks + ((size_t)t * B + b) * P;
        StQuad* tiles = a.tiles + ((size_t)t * B + b) * P;
        const int nrun = s_nrun[t];
        const int R = t == 0 ? a.tail_rows : 256;       // rows per tile of this table
        StPack st{0, 0, 0, 0, 0, 0};
        for (int r0 = 0; r0 < nrun; r0 += 64) {
            const int2 mine = r0 + lane < nrun ? runs[r0 + lane] : make_int2(0, 0);
            const int n = min(64, nrun - r0);
            for (int j = 0; j < n; ++j) {
                const int p = __shfl(mine.x, j), q = __shfl(mine.y, j);
                st_pack_run(st, p, q - p + 1, N, chunks, tiles, lane == 0, R);
            }
        }
        st_pack_close(st, tiles, lane == 0);
        if (lane == 0) {
            s_nchunk[t] = st.nchunk; s_ntile[t] = st.ntile;
            s_base[t] = atomicAdd(a.tile_count + t, st.ntile);
        }
    }
    __syncthreads();
    // 4. rows, extended rows, padding
    const RowEnt invalid = st_invalid_row(a.pix[0]);
    for (int t = 0; t < T; ++t) {
        const int nchunk = s_nchunk[t], ntile = s_ntile[t], base = s_base[t];
        const int R = t == 0 ? a.tail_rows : 256;
        // Cannot happen.  A tile that closes before its image's end closes on its slots (R / N pixels) or because fewer than 3N
        // extended rows are free; k pixels cost at most 3N * k of them, so it holds more than (XR_EXT_ROWS - 3N) / 3N pixels: at
        // least m = st_min_pixels(N) either way.  An image's table with T tiles has at least (T - 1) * m + 1 member pixels of its P, so
        // T <= P / m + 1, the images' reservations sum to at most B * (P / m + 1) = cap_tiles, and base + ntile stays within it in
        // whatever order the images reserve.  (tests/test_sparse_tables_reference_host.py holds the bound on the worst masks,
        // tests/test_gpu_sparse_masks.py holds the device's counts against the capacity.)
        if (base + ntile > a.cap_tiles) continue;
        RowEnt* rows = t == 0 ? a.rows : a.halo_rows;
        ExtRow* ext = reinterpret_cast<ExtRow*>(t == 0 ? a.ext : a.halo_ext);
        const StQuad* chunks = a.chunks + ((size_t)t * B + b) * P;
        const StQuad* tiles = a.tiles + ((size_t)t * B + b) * P;
        for (int i = tid; i < nchunk * N; i += blockDim.x) {
            const int ci = i / N, n = i - ci * N;
            const StQuad c = chunks[ci];
            st_write_piece(c, n, b, base + c.y, a.pix, N, P, a.Ppad, rows, ext, R);
        }
        for (int i = tid; i < ntile * R; i += blockDim.x) {
            const int tt = i / R, r = i - tt * R;
            if (st_pad_row(tiles[tt], r, N)) rows[(size_t)(base + tt) * R + r] = invalid;
        }
        for (int i = tid; i < ntile * XR_EXT_ROWS; i += blockDim.x) {
            const int tt = i / XR_EXT_ROWS, r = i - tt * XR_EXT_ROWS;
            const StQuad ti = tiles[tt];
            if (r >= ti.z) ext[(size_t)(base + tt) * XR_EXT_ROWS + r] = st_pad_ext(ti, b, a.pix, N, P, a.Ppad);
        }
    }
}

hipError_t launch_sparse_tail_rows(const SparseTailArgs& a, hipStream_t s) {
    if (a.B <= 0 || a.P <= 0 || a.N < 1 || 256 / a.N < 1 || XR_EXT_ROWS / a.N - 2 < 1 || a.P > 65536 || a.lv.n < 1 || a.lv.n > 5)
        return hipErrorInvalidValue;
    if ((a.tail_rows != 192 && a.tail_rows != 256) || a.tail_rows / a.N < 1) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(a.tile_count, 0, 2 * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sparse_tail_rows_kernel, dim3(a.B), dim3(256), (size_t)a.P, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Validation post-processing (src/retina_net/experiments/validation_utils.py:10-77): deterministic single
// forward pass -> softmax -> drop anchors whose arg-max class is background -> rank by the top score -> the
// same soft-NMS kernel.  The compacted candidates land in the posterior buffers (score = counts = softmax row,
// means = decoded box, covs = 0), so bod_nms and the getters serve both paths.
// ------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(POST_BLOCK) void val_flag_kernel(PostCfg c, PostBuffers pb, int nblocks) {
    const int a = blockIdx.x * POST_BLOCK + threadIdx.x;
    const int b = blockIdx.y;
    bool keep = false;
    if (a < c.A) {
        const float* l = pb.cls + (((size_t)b * c.N) * c.A + a) * C;        // sample 0
        float v[C];
#pragma unroll
        for (int j = 0; j < C; ++j) v[j] = l[j];
        float mx = v[0];
#pragma unroll
        for (int j = 1; j < C; ++j) mx = fmaxf(mx, v[j]);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < C; ++j) { v[j] = expf(v[j] - mx); s += v[j]; }
        int best = 0; float bestp = v[0] / s;
        float* dc = pb.d_counts + ((size_t)b * c.A + a) * C;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const float pj = v[j] / s;
            dc[j] = pj;
            if (j > 0 && pj > bestp) { bestp = pj; best = j; }                // tf.argmax: first maximum
        }
        keep = best != C - 1;
        pb.keep[(size_t)b * c.A + a] = keep ? 1 : 0;
    }
    const int n = __syncthreads_count(keep ? 1 : 0);
    if (threadIdx.x == 0) pb.block_counts[(size_t)b * nblocks + blockIdx.x] = n;
}

template <int C>
__global__ __launch_bounds__(POST_BLOCK) void val_fuse_kernel(PostCfg c, PostBuffers pb, int nblocks) {
    __shared__ int wave_off[POST_BLOCK / 64 + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a = blockIdx.x * POST_BLOCK + tid;
    const int b = blockIdx.y;
    const bool keep = (a < c.A) && pb.keep[(size_t)b * c.A + a];
    const unsigned long long bal = __ballot(keep);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wave_off[wave + 1] = __popcll(bal);
    if (tid == 0) wave_off[0] = 0;
    __syncthreads();
    if (tid == 0)
        for (int w = 1; w <= POST_BLOCK / 64; ++w) wave_off[w] += wave_off[w - 1];
    __syncthreads();
    if (!keep) return;
    const int slot = pb.block_counts[(size_t)b * nblocks + blockIdx.x] + wave_off[wave] + before;
    const size_t o = (size_t)b * c.A + slot;
    const float4 anc = reinterpret_cast<const float4*>(pb.anchors)[a];
    const float4 t = reinterpret_cast<const float4*>(pb.box)[((size_t)b * c.N) * c.A + a];
    float bx[4];
    decode_box(anc, t, bx);                                                   // box_utils.box_from_anchor_and_target (:149-168)
    const float* dc = pb.d_counts + ((size_t)b * c.A + a) * C;
    float top = dc[0];
#pragma unroll
    for (int j = 0; j < C; ++j) { pb.counts[o * C + j] = dc[j]; pb.score[o * C + j] = dc[j]; top = fmaxf(top, dc[j]); }
#pragma unroll
    for (int i = 0; i < 4; ++i) pb.means[o * 4 + i] = bx[i];
#pragma unroll
    for (int i = 0; i < 16; ++i) pb.covs[o * 16 + i] = 0.f;
    pb.ranking[o] = top;
    // vuhw_to_vuvu (box_utils.py:5-23)
    reinterpret_cast<float4*>(pb.corners)[o] = make_float4(bx[0] - bx[2] / 2.0f, bx[1] - bx[3] / 2.0f, bx[0] + bx[2] / 2.0f, bx[1] + bx[3] / 2.0f);
    pb.anchor_index[o] = a;
}

hipError_t launch_validation_post(const PostCfg& c, const PostBuffers& b, hipStream_t s) {
    const int nblocks = (c.A + POST_BLOCK - 1) / POST_BLOCK;
    dim3 grid(nblocks, c.B);
    if (c.C == 8) {
        hipLaunchKernelGGL(val_flag_kernel<8>, grid, dim3(POST_BLOCK), 0, s, c, b, nblocks);
        hipLaunchKernelGGL(post_scan_kernel, dim3(c.B), dim3(POST_BLOCK), 0, s, b, nblocks);
        hipLaunchKernelGGL(val_fuse_kernel<8>, grid, dim3(POST_BLOCK), 0, s, c, b, nblocks);
    } else if (c.C == 4) {
        hipLaunchKernelGGL(val_flag_kernel<4>, grid, dim3(POST_BLOCK), 0, s, c, b, nblocks);
        hipLaunchKernelGGL(post_scan_kernel, dim3(c.B), dim3(POST_BLOCK), 0, s, b, nblocks);
        hipLaunchKernelGGL(val_fuse_kernel<4>, grid, dim3(POST_BLOCK), 0, s, c, b, nblocks);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// The records validation writes out (validation_utils.py:62-77: tf.gather of the class rows and the corners by the NMS indices):
// one thread per (image, output row).  An index outside the image's candidates (never produced by nms_kernel) yields a zero row.
__global__ __launch_bounds__(128) void val_gather_kernel(ValGatherArgs a) {
    const int k = blockIdx.x * 128 + threadIdx.x;
    const int b = blockIdx.y;
    if (k >= a.max_out) return;
    const int n = min(max(a.num_selected[b], 0), a.max_out);
    if (k == 0) a.out_num[b] = n;
    const size_t o = (size_t)b * a.max_out + k;
    const int src = k < n ? a.selected[o] : -1;
    const bool ok = src >= 0 && src < min(a.num_kept[b], a.A);
    const size_t i = (size_t)b * a.A + (ok ? src : 0);
    for (int j = 0; j < a.C; ++j) a.out_scores[o * a.C + j] = ok ? a.score[i * a.C + j] : 0.f;
    reinterpret_cast<float4*>(a.out_corners)[o] = ok ? reinterpret_cast<const float4*>(a.corners)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
}

hipError_t launch_validation_gather(const ValGatherArgs& a, hipStream_t s) {
    if (a.B < 1 || a.B > 65535 || a.A < 1 || a.C < 1 || a.max_out < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(val_gather_kernel, dim3((unsigned)((a.max_out + 127) / 128), (unsigned)a.B), dim3(128), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Black-box MC dropout, stage 1 (bayesod.h, bod_set_uncertainty_method): the validation post-process above for every
// (image, sample) instead of sample 0.  The callers pass PostCfg with B = batch * mc_samples and N = 1, so blockIdx.y is the virtual
// image v = b * N + n and the raw tensors [B,N,A,.] are indexed by v as they stand.  Same expressions as val_flag_kernel /
// val_fuse_kernel (the candidates, their order, ranking and corners are theirs bit for bit), but nothing of width C or 16 is stored
// per candidate: the dense scratch is the keep flag and the top score, the compacted rows are ranking, corners and the anchor index.
// bb_gather_kernel recomputes the softmax row and forms the aleatoric matrix for the rows nms_kernel selected.
// ------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(POST_BLOCK) void bb_flag_kernel(PostCfg c, PostBuffers pb, BlackBoxArgs bb, int nblocks) {
    const int a = blockIdx.x * POST_BLOCK + threadIdx.x;
    const int v = blockIdx.y;
    bool keep = false;
    if (a < c.A) {
        const float* l = pb.cls + ((size_t)v * c.A + a) * C;
        float e[C];
#pragma unroll
        for (int j = 0; j < C; ++j) e[j] = l[j];
        float mx = e[0];
#pragma unroll
        for (int j = 1; j < C; ++j) mx = fmaxf(mx, e[j]);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < C; ++j) { e[j] = expf(e[j] - mx); s += e[j]; }
        int best = 0; float bestp = e[0] / s;
#pragma unroll
        for (int j = 1; j < C; ++j) {
            const float pj = e[j] / s;
            if (pj > bestp) { bestp = pj; best = j; }                          // tf.argmax: first maximum
        }
        keep = best != C - 1;
        bb.keep[(size_t)v * c.A + a] = keep ? 1 : 0;
        bb.top[(size_t)v * c.A + a] = bestp;
    }
    const int n = __syncthreads_count(keep ? 1 : 0);
    if (threadIdx.x == 0) bb.block_counts[(size_t)v * nblocks + blockIdx.x] = n;
}

__global__ __launch_bounds__(POST_BLOCK) void bb_compact_kernel(PostCfg c, PostBuffers pb, BlackBoxArgs bb, int nblocks) {
    __shared__ int wave_off[POST_BLOCK / 64 + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a = blockIdx.x * POST_BLOCK + tid;
    const int v = blockIdx.y;
    const bool keep = (a < c.A) && bb.keep[(size_t)v * c.A + a];
    const unsigned long long bal = __ballot(keep);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wave_off[wave + 1] = __popcll(bal);
    if (tid == 0) wave_off[0] = 0;
    __syncthreads();
    if (tid == 0)
        for (int w = 1; w <= POST_BLOCK / 64; ++w) wave_off[w] += wave_off[w - 1];
    __syncthreads();
    if (!keep) return;
    const int slot = bb.block_counts[(size_t)v * nblocks + blockIdx.x] + wave_off[wave] + before;
    const size_t o = (size_t)v * c.A + slot;
    const float4 anc = reinterpret_cast<const float4*>(pb.anchors)[a];
    const float4 t = reinterpret_cast<const float4*>(pb.box)[(size_t)v * c.A + a];
    float bx[4];
    decode_box(anc, t, bx);
    bb.ranking[o] = bb.top[(size_t)v * c.A + a];
    reinterpret_cast<float4*>(bb.corners)[o] = make_float4(bx[0] - bx[2] / 2.0f, bx[1] - bx[3] / 2.0f, bx[0] + bx[2] / 2.0f, bx[1] + bx[3] / 2.0f);
    bb.anchor_index[o] = a;
}

// One wave per virtual image walks its selected rows 64 at a time: softmax row, decoded box, the sample's own aleatoric matrix
// (post_fuse_anchor's arithmetic on one sample's parameters), KITTI rescale, then the ordered compaction of the rows whose top score
// is not below min_score.  c.B / c.N are the real batch and sample counts here.
template <int C>
__global__ __launch_bounds__(64) void bb_gather_kernel(PostCfg c, PostBuffers pb, BlackBoxArgs bb) {
    const int v = blockIdx.x, lane = threadIdx.x;
    const int b = v / c.N;
    const int K = bb.max_out;
    const int nsel = min(max(bb.num_selected[v], 0), K);
    const int M = min(max(bb.num_kept[v], 0), c.A);
    int nout = 0;
    for (int k0 = 0; k0 < nsel; k0 += 64) {
        const int k = k0 + lane;
        const int slot = k < nsel ? bb.selected[(size_t)v * K + k] : -1;
        const bool valid = slot >= 0 && slot < M;
        const int a = valid ? bb.anchor_index[(size_t)v * c.A + slot] : 0;
        float p[C];
        const float* l = pb.cls + ((size_t)v * c.A + a) * C;
#pragma unroll
        for (int j = 0; j < C; ++j) p[j] = l[j];
        float mx = p[0];
#pragma unroll
        for (int j = 1; j < C; ++j) mx = fmaxf(mx, p[j]);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < C; ++j) { p[j] = expf(p[j] - mx); s += p[j]; }
        float top = 0.f;
#pragma unroll
        for (int j = 0; j < C; ++j) { p[j] = p[j] / s; top = j == 0 ? p[0] : fmaxf(top, p[j]); }
        const float4 anc = reinterpret_cast<const float4*>(pb.anchors)[a];
        const float4 t = reinterpret_cast<const float4*>(pb.box)[(size_t)v * c.A + a];
        float bx[4];
        decode_box(anc, t, bx);
        Mat4 al;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) al.m[i][j] = 0.f;
        if (c.has_covar) {
            float x[10];
            const float* q = pb.cov + ((size_t)v * c.A + a) * 10;
#pragma unroll
            for (int i = 0; i < 10; ++i) x[i] = q[i];
            // tfp.math.fill_triangular, as in post_fuse_anchor
            const float d[4] = {expf(x[4]), expf(x[9]), expf(x[5]), expf(x[0])};
            if (c.use_full_covar) {
                const float l10 = x[8], l20 = x[7], l21 = x[6], l30 = x[3], l31 = x[2], l32 = x[1];
                float li[4][4];
                li[0][0] = 1.f; li[0][1] = 0.f; li[0][2] = 0.f; li[0][3] = 0.f;
                li[1][0] = -l10; li[1][1] = 1.f; li[1][2] = 0.f; li[1][3] = 0.f;
                li[2][0] = -(l20 * 1.f + l21 * li[1][0]); li[2][1] = -l21; li[2][2] = 1.f; li[2][3] = 0.f;
                li[3][0] = -(l30 * 1.f + l31 * li[1][0] + l32 * li[2][0]);
                li[3][1] = -(l31 * 1.f + l32 * li[2][1]);
                li[3][2] = -l32; li[3][3] = 1.f;
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j <= i; ++j) {
                        float sm = 0.f;
#pragma unroll
                        for (int kk = 0; kk <= j; ++kk) sm += li[i][kk] * d[kk] * li[j][kk];
                        al.m[i][j] = sm; al.m[j][i] = sm;
                    }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) al.m[i][i] = d[i];
            }
        }
        if (c.kitti_sh > 0.f) {                                       // S mu, S Sigma S^T, as bod_posterior does
            float ksh = c.kitti_sh, ksw = c.kitti_sw;
            if (c.kitti_frame) { ksh = c.kitti_frame[2 * b]; ksw = c.kitti_frame[2 * b + 1]; }
            const float sc[4] = {ksh, ksw, ksh, ksw};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                bx[i] *= sc[i];
#pragma unroll
                for (int j = 0; j < 4; ++j) al.m[i][j] = sc[i] * al.m[i][j] * sc[j];
            }
        }
        const bool pass = valid && !(top < bb.min_score);
        const unsigned long long bal = __ballot(pass);
        if (pass) {
            const size_t o = (size_t)v * K + nout + __popcll(bal & ((1ull << lane) - 1ull));
#pragma unroll
            for (int j = 0; j < C; ++j) bb.sd_score[o * C + j] = p[j];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                bb.sd_mean[o * 4 + i] = bx[i];
#pragma unroll
                for (int j = 0; j < 4; ++j) bb.sd_cov[o * 16 + i * 4 + j] = al.m[i][j];
            }
            bb.sd_anchor[o] = a;
        }
        nout += __popcll(bal);
    }
    if (lane == 0) bb.sd_count[v] = nout;
}

// ------------------------------------------------------------------------------------------------
// joint-entropy ranking (:169-200): min-max normalised information gains, one block per image
// ------------------------------------------------------------------------------------------------
// log det of an SPD 4x4 (a posterior covariance) through its Cholesky factor, in double: the cofactor expansion in fp32 loses
// cond(Sigma) x 2^-24 of the determinant to cancellation, which the min-max normalisation over the image's M boxes then
// stretches to ~5e-3 of the ranking; log det = 2 sum log L_ii has no cancellation.  (M ~ 10^3 boxes per image: the cost is nil.)
__device__ __forceinline__ double logdet4_spd(const float* m) {
    double L[4][4];
    double ld = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double s = (double)m[i * 4 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
            if (i == j) { L[i][i] = sqrt(s); ld += log(s); }      // log L_ii^2
            else L[i][j] = s / L[j][j];
        }
    }
    return ld;
}

__global__ __launch_bounds__(POST_BLOCK) void joint_entropy_kernel(PostCfg c, PostBuffers pb) {
    __shared__ float red[4][POST_BLOCK];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int M = pb.num_kept[b];
    const float two_pi_term = 2.0f + 2.0f * logf(2.0f * 3.14159265358979323846f);
    const float iv = c.iso_var;
    const float prior_ent = two_pi_term + 0.5f * logf(iv * iv * iv * iv);
    const float cat_prior = logf((float)c.C);          // entropy of the uniform prior score
    float gmin = INFINITY, gmax = -INFINITY, cmin = INFINITY, cmax = -INFINITY;
    for (int m = tid; m < M; m += POST_BLOCK) {
        const size_t o = (size_t)b * c.A + m;
        const float g = (float)((double)prior_ent - ((double)two_pi_term + 0.5 * logdet4_spd(pb.covs + o * 16)));
        float ce = 0.f;
        for (int j = 0; j < c.C; ++j) { const float p = pb.score[o * c.C + j]; ce -= p * logf(p); }
        const float cg = cat_prior - ce;
        gmin = fminf(gmin, g); gmax = fmaxf(gmax, g);
        cmin = fminf(cmin, cg); cmax = fmaxf(cmax, cg);
    }
    red[0][tid] = gmin; red[1][tid] = gmax; red[2][tid] = cmin; red[3][tid] = cmax;
    __syncthreads();
    for (int s = POST_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red[0][tid] = fminf(red[0][tid], red[0][tid + s]);
            red[1][tid] = fmaxf(red[1][tid], red[1][tid + s]);
            red[2][tid] = fminf(red[2][tid], red[2][tid + s]);
            red[3][tid] = fmaxf(red[3][tid], red[3][tid + s]);
        }
        __syncthreads();
    }
    gmin = red[0][0]; gmax = red[1][0]; cmin = red[2][0]; cmax = red[3][0];
    const float gden = fmaxf(1.0f, gmax - gmin), cden = fmaxf(0.001f, cmax - cmin);
    for (int m = tid; m < M; m += POST_BLOCK) {
        const size_t o = (size_t)b * c.A + m;
        const float g = (float)((double)prior_ent - ((double)two_pi_term + 0.5 * logdet4_spd(pb.covs + o * 16)));
        float ce = 0.f;
        for (int j = 0; j < c.C; ++j) { const float p = pb.score[o * c.C + j]; ce -= p * logf(p); }
        const float cg = cat_prior - ce;
        pb.ranking[o] = (cg - cmin) / cden + (g - gmin) / gden;
    }
}

hipError_t launch_joint_entropy_rank(const PostCfg& c, const PostBuffers& b, hipStream_t s) {
    hipLaunchKernelGGL(joint_entropy_kernel, dim3(c.B), dim3(POST_BLOCK), 0, s, c, b);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// K4: soft-NMS (NonMaxSuppressionV5). One wavefront per image walks the exact greedy order of
// the TF op: pop the best live candidate, decay it by every box selected since it was last
// examined (newest first), select iff unchanged, else re-queue.  The priority queue is replaced
// by a per-lane cached arg-max over a strided slice + a 6-step wave butterfly (same order:
// score desc, index asc).
// ------------------------------------------------------------------------------------------------
#define NMS_LDS_CAP 6144
#define NMS_MAX_OUT 512

__device__ __forceinline__ float nms_iou(const float4 bi, const float4 bj) {
    const float ymin_i = fminf(bi.x, bi.z), xmin_i = fminf(bi.y, bi.w);
    const float ymax_i = fmaxf(bi.x, bi.z), xmax_i = fmaxf(bi.y, bi.w);
    const float ymin_j = fminf(bj.x, bj.z), xmin_j = fminf(bj.y, bj.w);
    const float ymax_j = fmaxf(bj.x, bj.z), xmax_j = fmaxf(bj.y, bj.w);
    const float area_i = (ymax_i - ymin_i) * (xmax_i - xmin_i);
    const float area_j = (ymax_j - ymin_j) * (xmax_j - xmin_j);
    if (area_i <= 0.f || area_j <= 0.f) return 0.f;
    const float iy0 = fmaxf(ymin_i, ymin_j), ix0 = fmaxf(xmin_i, xmin_j);
    const float iy1 = fminf(ymax_i, ymax_j), ix1 = fminf(xmax_i, xmax_j);
    const float inter = fmaxf(iy1 - iy0, 0.f) * fmaxf(ix1 - ix0, 0.f);
    return inter / ((area_i + area_j) - inter);
}

// Wave-wide arg-max of (score desc, index asc) without LDS traffic: 4 DPP steps reduce each row of 16
// lanes (quad xor 1, xor 2, half-row mirror, row mirror), then the four row results are read out through
// SGPRs.  idx < 0 marks "no candidate".
__device__ __forceinline__ bool nms_better(float os, int oi, float bs, int bi) {
    return (oi >= 0) && (bi < 0 || os > bs || (os == bs && oi < bi));
}
template <int CTRL>
__device__ __forceinline__ void nms_dpp_step(float& bs, int& bi) {
    const float os = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(bs), CTRL, 0xF, 0xF, false));
    const int oi = __builtin_amdgcn_update_dpp(0, bi, CTRL, 0xF, 0xF, false);
    if (nms_better(os, oi, bs, bi)) { bs = os; bi = oi; }
}
__device__ __forceinline__ void nms_wave_argmax(float& bs, int& bi) {
    nms_dpp_step<0xB1>(bs, bi);     // quad_perm [1,0,3,2]
    nms_dpp_step<0x4E>(bs, bi);     // quad_perm [2,3,0,1]
    nms_dpp_step<0x141>(bs, bi);    // row_half_mirror
    nms_dpp_step<0x140>(bs, bi);    // row_mirror
    float rs = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bs), 0));
    int ri = __builtin_amdgcn_readlane(bi, 0);
#pragma unroll
    for (int r = 16; r < 64; r += 16) {
        const float os = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bs), r));
        const int oi = __builtin_amdgcn_readlane(bi, r);
        if (nms_better(os, oi, rs, ri)) { rs = os; ri = oi; }
    }
    bs = rs; bi = ri;
}

#define NMS_BOX_CAP 4096
__global__ __launch_bounds__(64) void nms_kernel(NmsArgs a) {
    extern __shared__ __attribute__((aligned(16))) char nms_smem[];
    float4* s_box = reinterpret_cast<float4*>(nms_smem);                                  // [NMS_BOX_CAP]
    float4* s_selbox = s_box + NMS_BOX_CAP;                                               // [NMS_MAX_OUT]
    float* s_score = reinterpret_cast<float*>(s_selbox + NMS_MAX_OUT);                    // [NMS_LDS_CAP]
    int* s_begin = reinterpret_cast<int*>(s_score + NMS_LDS_CAP);                         // [NMS_LDS_CAP]
    const int b = blockIdx.x, lane = threadIdx.x;
    const int M = a.num_kept[b];
    const float4* gboxes = reinterpret_cast<const float4*>(a.corners) + (size_t)b * a.A;
    float* score = (M <= NMS_LDS_CAP) ? s_score : a.work_scores + (size_t)b * ((a.A + 511) & ~511);
    int* begin = (M <= NMS_LDS_CAP) ? s_begin : a.work_begin + (size_t)b * ((a.A + 511) & ~511);
    const bool box_lds = M <= NMS_BOX_CAP;
    int* sel = a.selected + (size_t)b * a.max_out;
    const float scale = a.sigma > 0.f ? -0.5f / a.sigma : 0.f;
    const bool soft = a.sigma > 0.f;
    const bool always_soft = a.variant == 1 && soft;
    const bool hard_drop = a.variant == 1 && !soft;      // TF >= 2.3 without soft-NMS: a box over the IoU threshold is dropped, never re-queued
    const float NEG_INF = -INFINITY;

    // score[] is padded to a multiple of 64*8 with -inf; a candidate that leaves the queue is marked by
    // score = -inf as well (the op never queues a -inf score: it only admits score > score_threshold = -inf),
    // so the lane-local rescan is a branch-free strided max with 8 independent LDS reads in flight.
    const int Mpad = (M + 511) & ~511;
    for (int i = lane; i < Mpad; i += 64) {
        score[i] = i < M ? a.ranking[(size_t)b * a.A + i] : NEG_INF;
        if (i < M) {
            begin[i] = 0;
            if (box_lds) s_box[i] = gboxes[i];
        }
    }
    __syncthreads();

    // lane-local best over its strided slice
    float lbest = NEG_INF; int lidx = -1;
    auto rescan = [&]() {
        lbest = NEG_INF; lidx = -1;
        for (int i0 = lane; i0 < Mpad; i0 += 512) {
            float v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = score[i0 + q * 64];
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (v[q] > lbest) { lbest = v[q]; lidx = i0 + q * 64; }    // ascending i => lowest index wins ties
        }
    };
    rescan();
    int nsel = 0;
    while (nsel < a.max_out) {
        float bs = lbest; int bi = lidx;
        nms_wave_argmax(bs, bi);
        if (bi < 0) break;
        const int idx = bi;
        const float original = bs;
        const int beg = begin[idx];
        const float4 cb = box_lds ? s_box[idx] : gboxes[idx];
        // Decay by every box selected since the candidate was last examined, newest first (the TF op's
        // loop order; fp32 products do not commute in rounding).  Weights are evaluated lane-parallel, 64
        // selected boxes at a time with lane l <-> j = hi-1-l; a factor of exactly 1.0f (no overlap) leaves
        // the product bit-identical, so only the lanes with w != 1 enter the serial chain.
        float s = original;
        bool dropped = false;
        for (int hi = nsel; hi > beg; hi -= 64) {
            const int j = hi - 1 - lane;
            float w = 1.0f;
            bool over = false;
            if (j >= beg) {
                const float sim = nms_iou(cb, s_selbox[j]);
                if (sim != 0.f) w = (float)exp((double)(scale * (sim * sim)));
                if (!always_soft && !(sim <= a.iou_thr)) w = 0.f;
                over = sim > a.iou_thr;
            }
            if (hard_drop && __ballot(over)) dropped = true;
            unsigned long long m = __ballot(w != 1.0f);
            while (m) {
                const int l = __builtin_ctzll(m);
                m &= m - 1;
                s = s * __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), l));
            }
        }
        const bool owner = (idx & 63) == lane;
        if (dropped) {
            if (owner) score[idx] = NEG_INF;
        } else if (s == original) {
            if (lane == 0) { sel[nsel] = idx; s_selbox[nsel] = cb; }
            if (owner) score[idx] = NEG_INF;
            ++nsel;
        } else if (s > NEG_INF) {
            if (owner) { score[idx] = s; begin[idx] = nsel; }
        } else {
            if (owner) score[idx] = NEG_INF;
        }
        __syncthreads();
        if (owner) rescan();
    }
    if (lane == 0) a.num_selected[b] = nsel;
}

hipError_t launch_nms(const NmsArgs& a, hipStream_t s) {
    if (a.max_out > NMS_MAX_OUT) return hipErrorInvalidValue;
    constexpr int LDS = (NMS_BOX_CAP + NMS_MAX_OUT) * 16 + NMS_LDS_CAP * 8;
    static PerDeviceOnce once;
    bool& attr_set = *once.slot();
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(nms_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    hipLaunchKernelGGL(nms_kernel, dim3(a.B), dim3(64), LDS, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// K5: cluster-and-fuse. One workgroup per (centre, image); the M x M affinity matrix of the
// reference (:214-215) is never built: IoU against the centre is evaluated on the fly.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float iou_plus1(const float4 p, const float4 q) {
    // box_utils.bbox_iou_vuvu (:117-146) including the (min-max+1) area quirk
    const float xi1 = fmaxf(p.y, q.y), yi1 = fmaxf(p.x, q.x);
    const float xi2 = fminf(p.w, q.w), yi2 = fminf(p.z, q.z);
    const float inter = fmaxf(xi2 - xi1 + 1.0f, 0.f) * fmaxf(yi2 - yi1 + 1.0f, 0.f);
    const float a1 = (p.y - p.w + 1.0f) * (p.x - p.z + 1.0f);
    const float a2 = (q.y - q.w + 1.0f) * (q.x - q.z + 1.0f);
    const float uni = (a1 + a2) - inter;
    return inter / (uni + 0.00001f);
}

#define CL_BLOCK 256
template <int C>
__global__ __launch_bounds__(CL_BLOCK) void cluster_fuse_kernel(ClusterArgs a) {
    __shared__ float red[CL_BLOCK];
    __shared__ float top_kl[4 * 3];              // the four waves' three best (kl, anchor) each
    __shared__ int top_ix[4 * 3];
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (k >= a.num_selected[b]) return;
    const int M = a.num_kept[b];
    const int centre = a.selected[(size_t)b * a.max_out + k];
    const size_t base = (size_t)b * a.A;
    const float4* boxes = reinterpret_cast<const float4*>(a.corners) + base;
    const float4 cbox = boxes[centre];
    float cs[C];
    {
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < C; ++j) { cs[j] = a.counts[(base + centre) * C + j]; sum += cs[j]; }
#pragma unroll
        for (int j = 0; j < C; ++j) cs[j] = cs[j] / sum;
        // scipy.stats.entropy renormalises pk
        float s2 = 0.f;
#pragma unroll
        for (int j = 0; j < C; ++j) s2 += cs[j];
#pragma unroll
        for (int j = 0; j < C; ++j) cs[j] = cs[j] / s2;
    }
    float psum[10], pmsum[4], ssum[C], csum[C];
#pragma unroll
    for (int q = 0; q < 10; ++q) psum[q] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) pmsum[q] = 0.f;
#pragma unroll
    for (int j = 0; j < C; ++j) { ssum[j] = 0.f; csum[j] = 0.f; }
    float tk[3] = {INFINITY, INFINITY, INFINITY};
    int ti[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff};
    int cnt = 0;
    const float* aff = (a.affinity && b == a.affinity_img) ? a.affinity + (size_t)k * a.A : nullptr;
    for (int i = tid; i < M; i += CL_BLOCK) {
        if (!((aff ? aff[i] : iou_plus1(boxes[i], cbox)) > a.thr)) continue;
        ++cnt;
        Mat4 cv;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) cv.m[r][q] = a.covs[(base + i) * 16 + r * 4 + q];
        const Mat4 pr = inv_spd4(cv);
        int t = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q <= r; ++q) psum[t++] += pr.m[r][q];
        float mu[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) mu[r] = a.means[(base + i) * 4 + r];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float s = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) s += pr.m[r][q] * mu[q];
            pmsum[r] += s;
        }
        float row[C], rs = 0.f;
#pragma unroll
        for (int j = 0; j < C; ++j) { row[j] = a.counts[(base + i) * C + j]; rs += row[j]; }
        float kl = 0.f, qs = 0.f;
        float sc[C];
#pragma unroll
        for (int j = 0; j < C; ++j) { sc[j] = row[j] / rs; qs += sc[j]; }
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const float q = sc[j] / qs;
            if (cs[j] > 0.f) kl += (q > 0.f) ? cs[j] * logf(cs[j] / q) : INFINITY;
            ssum[j] += sc[j];
            csum[j] += row[j];
        }
        // insert into this thread's sorted top-3 (kl asc, index asc)
        if (kl < tk[2] || (kl == tk[2] && i < ti[2])) {
            tk[2] = kl; ti[2] = i;
            if (tk[2] < tk[1] || (tk[2] == tk[1] && ti[2] < ti[1])) {
                float f = tk[1]; tk[1] = tk[2]; tk[2] = f; int g = ti[1]; ti[1] = ti[2]; ti[2] = g;
                if (tk[1] < tk[0] || (tk[1] == tk[0] && ti[1] < ti[0])) {
                    f = tk[0]; tk[0] = tk[1]; tk[1] = f; g = ti[0]; ti[0] = ti[1]; ti[1] = g;
                }
            }
        }
    }
    // ---- block reductions (round 4): wave-wide butterflies + one LDS exchange of the four waves' partials -- two barriers for all 15
    // sums (the tree reduction per value they replace: 140), the global top-3 as three rounds of wave-wide arg-min + a 12-entry merge
    // (replaced: one thread scanning 768 entries).  Sums are re-associated (fp32 round-off); the top-3 selection is exact.
    const int wave = tid >> 6, lane = tid & 63;
    auto wsum = [](float v) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        return v;
    };
    {
        float vals[15];
#pragma unroll
        for (int q = 0; q < 10; ++q) vals[q] = psum[q];
#pragma unroll
        for (int q = 0; q < 4; ++q) vals[10 + q] = pmsum[q];
        vals[14] = (float)cnt;                                  // (at most A < 2^24: exact)
#pragma unroll
        for (int q = 0; q < 15; ++q) {
            const float r = wsum(vals[q]);
            if (lane == 0) red[wave * 16 + q] = r;
        }
    }
    // this wave's three best (kl asc, index asc) of its threads' sorted candidates
    {
        int p = 0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float ck = p == 0 ? tk[0] : p == 1 ? tk[1] : p == 2 ? tk[2] : INFINITY;
            const int ci = p == 0 ? ti[0] : p == 1 ? ti[1] : p == 2 ? ti[2] : 0x7fffffff;
            float bk = ck; int bi = ci;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ok = __shfl_xor(bk, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (oi != 0x7fffffff && (bi == 0x7fffffff || ok < bk || (ok == bk && oi < bi))) { bk = ok; bi = oi; }
            }
            if (lane == 0) { top_kl[wave * 3 + r] = bk; top_ix[wave * 3 + r] = bi; }
            if (bi != 0x7fffffff && ci == bi) ++p;              // (an anchor belongs to exactly one thread: the winner advances)
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 10; ++q) psum[q] = (red[q] + red[16 + q]) + (red[32 + q] + red[48 + q]);
#pragma unroll
    for (int q = 0; q < 4; ++q) pmsum[q] = (red[10 + q] + red[26 + q]) + (red[42 + q] + red[58 + q]);
    const int total = (int)((red[14] + red[30]) + (red[46] + red[62]));
    if (total <= 3) {                                           // (block-uniform)
        __syncthreads();                                        // every thread has read the first exchange
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const float r0 = wsum(ssum[j]), r1 = wsum(csum[j]);
            if (lane == 0) { red[wave * 16 + j] = r0; red[64 + wave * 16 + j] = r1; }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < C; ++j) {
            ssum[j] = (red[j] + red[16 + j]) + (red[32 + j] + red[48 + j]);
            csum[j] = (red[64 + j] + red[80 + j]) + (red[96 + j] + red[112 + j]);
        }
    }
    if (tid != 0) return;
    const size_t ob = (size_t)b * a.max_out + k;
    // fused Gaussian: cov = inv(sum prec), mean = cov * sum(prec*mean)  (:321-331), x70 (:361)
    Mat4 ps;
    {
        int t = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q <= r; ++q) { ps.m[r][q] = psum[t]; ps.m[q][r] = psum[t]; ++t; }
    }
    const Mat4 fc = inv_spd4(ps);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) s += fc.m[r][q] * pmsum[q];
        a.out_means[ob * 4 + r] = s;
#pragma unroll
        for (int q = 0; q < 4; ++q) a.out_covs[ob * 16 + r * 4 + q] = fc.m[r][q] * 70.0f;
    }
    if (total > 3) {
        // global top-3 over the per-thread candidates (:338-349)
        float bk[3] = {INFINITY, INFINITY, INFINITY};
        int bx[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff};
        for (int t = 0; t < 4 * 3; ++t) {                       // the four waves' three best each
            const float kl = top_kl[t]; const int ix = top_ix[t];
            if (ix == 0x7fffffff) continue;
            if (kl < bk[2] || (kl == bk[2] && ix < bx[2])) {
                bk[2] = kl; bx[2] = ix;
                if (bk[2] < bk[1] || (bk[2] == bk[1] && bx[2] < bx[1])) {
                    float f = bk[1]; bk[1] = bk[2]; bk[2] = f; int g = bx[1]; bx[1] = bx[2]; bx[2] = g;
                    if (bk[1] < bk[0] || (bk[1] == bk[0] && bx[1] < bx[0])) {
                        f = bk[0]; bk[0] = bk[1]; bk[1] = f; g = bx[0]; bx[0] = bx[1]; bx[1] = g;
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < C; ++j) { ssum[j] = 0.f; csum[j] = 0.f; }
        for (int t = 0; t < 3; ++t) {
            float row[C], rs = 0.f;
#pragma unroll
            for (int j = 0; j < C; ++j) { row[j] = a.counts[(base + bx[t]) * C + j]; rs += row[j]; }
#pragma unroll
            for (int j = 0; j < C; ++j) { ssum[j] += row[j] / rs; csum[j] += row[j]; }
        }
    }
    const float denom = (float)(total > 3 ? 3 : total);
#pragma unroll
    for (int j = 0; j < C; ++j) {
        a.out_scores[ob * C + j] = ssum[j] / denom;
        a.out_counts[ob * C + j] = csum[j];
    }
}

hipError_t launch_cluster_fuse(const ClusterArgs& a, hipStream_t s) {
    dim3 grid(a.max_out, a.B);
    if (a.C == 8) hipLaunchKernelGGL(cluster_fuse_kernel<8>, grid, dim3(CL_BLOCK), 0, s, a);
    else if (a.C == 4) hipLaunchKernelGGL(cluster_fuse_kernel<4>, grid, dim3(CL_BLOCK), 0, s, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// Covariance parts of the fused detections (kernels.h): with P_i the precision of member i and F = (sum P_i)^-1 the
// fused mean is F sum P_i mu_i, linear in the members' means, so each part X of the fused covariance is 70 F (sum P_i X_i P_i) F
// and the three sum to 70 F, the covariance cluster_fuse_kernel stores.  Same grid, same membership expression and the same
// reduction as that kernel: wave butterflies, one LDS exchange, thread 0 finishes.
__global__ __launch_bounds__(CL_BLOCK) void cluster_parts_kernel(ClusterArgs a, const float* __restrict__ parts, float* __restrict__ out_parts) {
    __shared__ float red[4 * 40];
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (k >= a.num_selected[b]) return;
    const int M = a.num_kept[b];
    const int centre = a.selected[(size_t)b * a.max_out + k];
    const size_t base = (size_t)b * a.A;
    const float4* boxes = reinterpret_cast<const float4*>(a.corners) + base;
    const float4 cbox = boxes[centre];
    float acc[40];                                   // sum P_i X_i P_i: 3 x 10 (lower triangles), then sum P_i: 10
#pragma unroll
    for (int q = 0; q < 40; ++q) acc[q] = 0.f;
    const float* aff = (a.affinity && b == a.affinity_img) ? a.affinity + (size_t)k * a.A : nullptr;
    for (int i = tid; i < M; i += CL_BLOCK) {
        if (!((aff ? aff[i] : iou_plus1(boxes[i], cbox)) > a.thr)) continue;
        Mat4 cv;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) cv.m[r][q] = a.covs[(base + i) * 16 + r * 4 + q];
        const Mat4 pr = inv_spd4(cv);
        {
            int t = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int q = 0; q <= r; ++q) acc[30 + t++] += pr.m[r][q];
        }
        const float* x = parts + (base + i) * BOD_PARTS_TRI;
        const float one[4] = {1.f, 1.f, 1.f, 1.f};
#pragma unroll
        for (int part = 0; part < 3; ++part) {
            Mat4 xm;
            int t = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int q = 0; q <= r; ++q) { xm.m[r][q] = x[part * 10 + t]; xm.m[q][r] = xm.m[r][q]; ++t; }
            float pxp[10];
            parts_congruence(pr, xm, one, pxp);
#pragma unroll
            for (int q = 0; q < 10; ++q) acc[part * 10 + q] += pxp[q];
        }
    }
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int q = 0; q < 40; ++q) {
        float v = acc[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) red[wave * 40 + q] = v;
    }
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int q = 0; q < 40; ++q) acc[q] = (red[q] + red[40 + q]) + (red[80 + q] + red[120 + q]);
    Mat4 ps;
    {
        int t = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q <= r; ++q) { ps.m[r][q] = acc[30 + t]; ps.m[q][r] = acc[30 + t]; ++t; }
    }
    const Mat4 fc = inv_spd4(ps);
    const float one[4] = {1.f, 1.f, 1.f, 1.f};
    float* out = out_parts + ((size_t)b * a.max_out + k) * 48;
#pragma unroll
    for (int part = 0; part < 3; ++part) {
        Mat4 sm;
        int t = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q <= r; ++q) { sm.m[r][q] = acc[part * 10 + t]; sm.m[q][r] = sm.m[r][q]; ++t; }
        float fsf[10];
        parts_congruence(fc, sm, one, fsf);
        t = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q <= r; ++q) {
                const float v = fsf[t++] * 70.0f;
                out[part * 16 + r * 4 + q] = v; out[part * 16 + q * 4 + r] = v;
            }
    }
}

hipError_t launch_cluster_parts(const ClusterArgs& a, const float* parts, float* out_parts, hipStream_t s) {
    if (!parts || !out_parts) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cluster_parts_kernel, dim3(a.max_out, a.B), dim3(CL_BLOCK), 0, s, a, parts, out_parts);
    return hipGetLastError();
}

// Class-entropy parts of the fused detections (kernels.h).  The Dirichlet fusion adds the members' counts with equal
// weight, so the M members are M * K samples of one object: pbar_c = (sum_i pbar_i) / M, total = H(pbar_c), the aleatoric part and
// the members' own mutual information are the members' means, and what remains -- the disagreement between the members' mean
// distributions, >= 0 by Jensen's inequality -- is the spatial part.  Same grid, membership expression and reduction as
// cluster_fuse_kernel: wave butterflies, one LDS exchange, thread 0 finishes.
template <int C>
__global__ __launch_bounds__(CL_BLOCK) void cluster_class_parts_kernel(ClusterArgs a, const float* __restrict__ cparts, float* __restrict__ out_cparts) {
    constexpr int Q = C + 3;                          // sum pbar_i [C], sum aleatoric_i, sum epistemic_i, members
    __shared__ float red[4 * Q];
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (k >= a.num_selected[b]) return;
    const int M = a.num_kept[b];
    const int centre = a.selected[(size_t)b * a.max_out + k];
    const size_t base = (size_t)b * a.A;
    const float4* boxes = reinterpret_cast<const float4*>(a.corners) + base;
    const float4 cbox = boxes[centre];
    float acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = 0.f;
    const float* aff = (a.affinity && b == a.affinity_img) ? a.affinity + (size_t)k * a.A : nullptr;
    for (int i = tid; i < M; i += CL_BLOCK) {
        if (!((aff ? aff[i] : iou_plus1(boxes[i], cbox)) > a.thr)) continue;
        const float* x = cparts + (base + i) * Q;
#pragma unroll
        for (int j = 0; j < C; ++j) acc[j] += x[3 + j];
        acc[C] += x[1]; acc[C + 1] += x[2]; acc[C + 2] += 1.f;
    }
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        float v = acc[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) red[wave * Q + q] = v;
    }
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = (red[q] + red[Q + q]) + (red[2 * Q + q] + red[3 * Q + q]);
    const float fm = acc[C + 2];                      // >= 1 with the IoU (the centre is its own member); a caller's affinity may leave none
    float* out = out_cparts + ((size_t)b * a.max_out + k) * 4;
    if (!(fm > 0.f)) { out[0] = 0.f; out[1] = 0.f; out[2] = 0.f; out[3] = 0.f; return; }
    float total = 0.f;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        const float pj = acc[j] / fm;
        if (pj > 0.f) total -= pj * logf(pj);
    }
    const float ale = acc[C] / fm, emc = acc[C + 1] / fm;
    out[0] = total; out[1] = ale; out[2] = emc; out[3] = fmaxf(total - (ale + emc), 0.f);
}

hipError_t launch_cluster_class_parts(const ClusterArgs& a, const float* cparts, float* out_cparts, hipStream_t s) {
    if (!cparts || !out_cparts || (a.C != 4 && a.C != 8)) return hipErrorInvalidValue;
    if (a.C == 8) hipLaunchKernelGGL(cluster_class_parts_kernel<8>, dim3(a.max_out, a.B), dim3(CL_BLOCK), 0, s, a, cparts, out_cparts);
    else hipLaunchKernelGGL(cluster_class_parts_kernel<4>, dim3(a.max_out, a.B), dim3(CL_BLOCK), 0, s, a, cparts, out_cparts);
    return hipGetLastError();
}

// The NMS pick and the equal-weight Gaussian mixture of a cluster (bayesod.h, bod_set_merge_method), in place of
// cluster_fuse_kernel: same grid, same membership expression, the same reduction (wave butterflies, one LDS exchange of the four
// waves' partials, thread 0 finishes), and no 4x4 inverse.  The members' means enter shifted by the centre's, d_i = mu_i - mu_c.
// BOD_MERGE_CENTRE (uniform over the grid) only counts the members.
template <int C>
__global__ __launch_bounds__(CL_BLOCK) void cluster_merge_kernel(ClusterArgs a, int method, MergeTerms out) {
    constexpr int Q = 25 + 2 * C;                     // sum Sigma_i [10], sum d_i d_i^T [10], sum d_i [4], scores [C], counts [C], members
    __shared__ float red[4 * Q];
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (k >= a.num_selected[b]) return;
    const int M = a.num_kept[b];
    const int centre = a.selected[(size_t)b * a.max_out + k];
    const size_t base = (size_t)b * a.A;
    const float4* boxes = reinterpret_cast<const float4*>(a.corners) + base;
    const float4 cbox = boxes[centre];
    const bool mix = method == BOD_MERGE_MIXTURE;
    float mc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) mc[r] = a.means[(base + centre) * 4 + r];
    float acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = 0.f;
    const float* aff = (a.affinity && b == a.affinity_img) ? a.affinity + (size_t)k * a.A : nullptr;
    for (int i = tid; i < M; i += CL_BLOCK) {
        if (!((aff ? aff[i] : iou_plus1(boxes[i], cbox)) > a.thr)) continue;
        acc[Q - 1] += 1.f;                            // (at most A < 2^24: exact)
        if (!mix) continue;
        float d[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) d[r] = a.means[(base + i) * 4 + r] - mc[r];
        int t = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q <= r; ++q) {
                acc[t] += a.covs[(base + i) * 16 + r * 4 + q];
                acc[10 + t] += d[r] * d[q];
                ++t;
            }
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[20 + r] += d[r];
        float row[C], rs = 0.f;
#pragma unroll
        for (int j = 0; j < C; ++j) { row[j] = a.counts[(base + i) * C + j]; rs += row[j]; }
#pragma unroll
        for (int j = 0; j < C; ++j) { acc[24 + j] += row[j] / rs; acc[24 + C + j] += row[j]; }
    }
    const int wave = tid >> 6, lane = tid & 63;
    auto wsum = [](float v) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        return v;
    };
    if (mix) {                                        // (block-uniform)
#pragma unroll
        for (int q = 0; q < Q - 1; ++q) {
            const float r = wsum(acc[q]);
            if (lane == 0) red[wave * Q + q] = r;
        }
    }
    {
        const float r = wsum(acc[Q - 1]);
        if (lane == 0) red[wave * Q + Q - 1] = r;
    }
    __syncthreads();
    if (tid != 0) return;
    const size_t ob = (size_t)b * a.max_out + k;
    const float fn = (red[Q - 1] + red[2 * Q - 1]) + (red[3 * Q - 1] + red[4 * Q - 1]);
    out.members[ob] = (int)fn;
    if (!mix || !(fn > 0.f)) {
        // the centre's own posterior row; a caller's affinity may leave a mixture without members: the same row
        float row[C], rs = 0.f;
#pragma unroll
        for (int j = 0; j < C; ++j) { row[j] = a.counts[(base + centre) * C + j]; rs += row[j]; }
#pragma unroll
        for (int j = 0; j < C; ++j) { a.out_scores[ob * C + j] = row[j] / rs; a.out_counts[ob * C + j] = row[j]; }
#pragma unroll
        for (int r = 0; r < 4; ++r) a.out_means[ob * 4 + r] = mc[r];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float v = a.covs[(base + centre) * 16 + q];
            a.out_covs[ob * 16 + q] = v; out.within[ob * 16 + q] = v; out.between[ob * 16 + q] = 0.f;
        }
        return;
    }
#pragma unroll
    for (int q = 0; q < Q - 1; ++q) acc[q] = (red[q] + red[Q + q]) + (red[2 * Q + q] + red[3 * Q + q]);
    float dbar[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { dbar[r] = acc[20 + r] / fn; a.out_means[ob * 4 + r] = mc[r] + dbar[r]; }
    {
        int t = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q <= r; ++q) {
                const float w = acc[t] / fn;
                const float bt = acc[10 + t] / fn - dbar[r] * dbar[q];
                const float cv = w + bt;
                out.within[ob * 16 + r * 4 + q] = w; out.within[ob * 16 + q * 4 + r] = w;
                out.between[ob * 16 + r * 4 + q] = bt; out.between[ob * 16 + q * 4 + r] = bt;
                a.out_covs[ob * 16 + r * 4 + q] = cv; a.out_covs[ob * 16 + q * 4 + r] = cv;
                ++t;
            }
    }
#pragma unroll
    for (int j = 0; j < C; ++j) {
        a.out_scores[ob * C + j] = acc[24 + j] / fn;
        a.out_counts[ob * C + j] = acc[24 + C + j] / fn;
    }
}

hipError_t launch_cluster_merge(const ClusterArgs& a, int method, MergeTerms out, hipStream_t s) {
    if ((method != BOD_MERGE_CENTRE && method != BOD_MERGE_MIXTURE) || !out.within || !out.between || !out.members) return hipErrorInvalidValue;
    dim3 grid(a.max_out, a.B);
    if (a.C == 8) hipLaunchKernelGGL(cluster_merge_kernel<8>, grid, dim3(CL_BLOCK), 0, s, a, method, out);
    else if (a.C == 4) hipLaunchKernelGGL(cluster_merge_kernel<4>, grid, dim3(CL_BLOCK), 0, s, a, method, out);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// Black-box MC dropout, stage 2 (bayesod.h): one workgroup per image merges its pool of N * max_out sample detections.
// Pool entry i = n * max_out + rank; an entry past its sample's count, and an assigned one, has top score -inf.  Top scores and corners
// live in LDS up to BB_POOL_LDS_CAP entries, in the global work buffers beyond.  A thread only ever touches the entries i = tid (mod
// BB_BLOCK), in the arg-max and in the member pass alike, so the pool needs no barrier; the two LDS exchanges per centre do.
// Centre: block arg-max of (score desc, index asc) -- the lane's strided scan, nms_kernel's wave arg-max, the four waves' results
// compared in wave order.  Members: the centre plus every unassigned i with iou_plus1(centre, i) > thr.  Sums as cluster_merge_kernel
// forms them (d_i = mu_i - mu_c; per-thread chain, wave butterflies, (w0 + w1) + (w2 + w3)); thread 0 writes the row.
#define BB_BLOCK 256
#define BB_POOL_LDS_CAP 6144
template <int C>
__global__ __launch_bounds__(BB_BLOCK) void bb_merge_kernel(BlackBoxArgs a, MergeTerms terms) {
    constexpr int Q = 31 + C;                         // sum cov_i [16], sum d_i d_i^T [10], sum d_i [4], sum score_i [C], members
    extern __shared__ __attribute__((aligned(16))) char bb_smem[];
    __shared__ float red[4 * Q];
    __shared__ float s_ws[4];
    __shared__ int s_wi[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.max_out, P = a.N * K;
    const bool lds = P <= BB_POOL_LDS_CAP;
    float4* box = lds ? reinterpret_cast<float4*>(bb_smem) : reinterpret_cast<float4*>(a.pool_corners) + (size_t)b * P;
    float* score = lds ? reinterpret_cast<float*>(bb_smem + (size_t)BB_POOL_LDS_CAP * 16) : a.pool_top + (size_t)b * P;
    const size_t sd0 = (size_t)b * P;                 // the image's first sample-detection row: v * K + rank = b * P + i
    const float NEG_INF = -INFINITY;
    for (int i = tid; i < P; i += BB_BLOCK) {
        const int n = i / K, rank = i - n * K;
        const bool valid = rank < min(max(a.sd_count[b * a.N + n], 0), K);
        float top = NEG_INF;
        if (valid) {
            const float* sr = a.sd_score + (sd0 + i) * C;
            top = sr[0];
#pragma unroll
            for (int j = 1; j < C; ++j) top = fmaxf(top, sr[j]);
            const float4 m = reinterpret_cast<const float4*>(a.sd_mean)[sd0 + i];
            // box_utils.vuhw_to_vuvu
            box[i] = make_float4(m.x - m.z / 2.0f, m.y - m.w / 2.0f, m.x + m.z / 2.0f, m.y + m.w / 2.0f);
        }
        score[i] = top;
    }
    __syncthreads();                                  // every thread reads the centre's box
    int nout = 0;
    while (nout < K) {
        float bs = NEG_INF; int bi = -1;
        for (int i = tid; i < P; i += BB_BLOCK) {
            const float v = score[i];
            if (v > bs) { bs = v; bi = i; }           // ascending i: the lowest index wins a tie
        }
        nms_wave_argmax(bs, bi);
        if (lane == 0) { s_ws[wave] = bs; s_wi[wave] = bi; }
        __syncthreads();
        bs = s_ws[0]; bi = s_wi[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (nms_better(s_ws[w], s_wi[w], bs, bi)) { bs = s_ws[w]; bi = s_wi[w]; }
        if (bi < 0) break;                            // (block-uniform) the pool is empty
        const int centre = bi;
        const float4 cbox = box[centre];
        const float4 mcv = reinterpret_cast<const float4*>(a.sd_mean)[sd0 + centre];
        const float mc[4] = {mcv.x, mcv.y, mcv.z, mcv.w};
        float acc[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) acc[q] = 0.f;
        for (int i = tid; i < P; i += BB_BLOCK) {
            if (!(score[i] > NEG_INF)) continue;
            if (i != centre && !(iou_plus1(cbox, box[i]) > a.thr)) continue;
            score[i] = NEG_INF;
            acc[Q - 1] += 1.f;
            const float4 mv = reinterpret_cast<const float4*>(a.sd_mean)[sd0 + i];
            const float d[4] = {mv.x - mc[0], mv.y - mc[1], mv.z - mc[2], mv.w - mc[3]};
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[q] += a.sd_cov[(sd0 + i) * 16 + q];
            int t = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int q = 0; q <= r; ++q) { acc[16 + t] += d[r] * d[q]; ++t; }
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[26 + r] += d[r];
#pragma unroll
            for (int j = 0; j < C; ++j) acc[30 + j] += a.sd_score[(sd0 + i) * C + j];
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            float v = acc[q];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == 0) red[wave * Q + q] = v;
        }
        __syncthreads();
        const float fn = (red[Q - 1] + red[2 * Q - 1]) + (red[3 * Q - 1] + red[4 * Q - 1]);      // (block-uniform, exact: at most 15 360)
        if ((int)fn >= a.min_members) {
            if (tid == 0) {
                const size_t ob = (size_t)b * K + nout;
#pragma unroll
                for (int q = 0; q < Q - 1; ++q) acc[q] = (red[q] + red[Q + q]) + (red[2 * Q + q] + red[3 * Q + q]);
                float dbar[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) { dbar[r] = acc[26 + r] / fn; a.out_means[ob * 4 + r] = mc[r] + dbar[r]; }
                const bool single = !(fn > 1.f);
                float bt[16];
                int t = 0;
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int q = 0; q <= r; ++q) {
                        const float v = single ? 0.f : (acc[16 + t] - fn * (dbar[r] * dbar[q])) / (fn - 1.0f);
                        bt[r * 4 + q] = v; bt[q * 4 + r] = v;
                        ++t;
                    }
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const float w = acc[q] / fn;
                    terms.within[ob * 16 + q] = w;
                    terms.between[ob * 16 + q] = bt[q];
                    a.out_covs[ob * 16 + q] = w + bt[q];
                }
#pragma unroll
                for (int j = 0; j < C; ++j) { a.out_counts[ob * C + j] = acc[30 + j]; a.out_scores[ob * C + j] = acc[30 + j] / fn; }
                terms.members[ob] = (int)fn;
                a.out_centre[ob] = centre;
            }
            ++nout;
        }
        __syncthreads();                              // red / s_ws are rewritten by the next centre
    }
    if (tid == 0) a.out_num[b] = nout;
}

hipError_t launch_blackbox_samples(const PostCfg& c, const PostBuffers& in, const BlackBoxArgs& a, const NmsArgs& nms, hipStream_t s) {
    const long long V = (long long)a.B * a.N;
    if (V < 1 || V > 65535 || a.A < 1 || a.max_out < 1 || a.max_out > NMS_MAX_OUT) return hipErrorInvalidValue;
    PostCfg cv = c;                                   // the virtual images: B * N images of one sample each
    cv.B = (int32_t)V; cv.N = 1;
    PostBuffers scan{};
    scan.block_counts = a.block_counts; scan.num_kept = a.num_kept;
    const int nblocks = (a.A + POST_BLOCK - 1) / POST_BLOCK;
    dim3 grid(nblocks, (unsigned)V);
    if (a.C == 8) hipLaunchKernelGGL(bb_flag_kernel<8>, grid, dim3(POST_BLOCK), 0, s, cv, in, a, nblocks);
    else if (a.C == 4) hipLaunchKernelGGL(bb_flag_kernel<4>, grid, dim3(POST_BLOCK), 0, s, cv, in, a, nblocks);
    else return hipErrorInvalidValue;
    hipLaunchKernelGGL(post_scan_kernel, dim3((unsigned)V), dim3(POST_BLOCK), 0, s, scan, nblocks);
    hipLaunchKernelGGL(bb_compact_kernel, grid, dim3(POST_BLOCK), 0, s, cv, in, a, nblocks);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_nms(nms, s);
    if (e != hipSuccess) return e;
    if (a.C == 8) hipLaunchKernelGGL(bb_gather_kernel<8>, dim3((unsigned)V), dim3(64), 0, s, c, in, a);
    else hipLaunchKernelGGL(bb_gather_kernel<4>, dim3((unsigned)V), dim3(64), 0, s, c, in, a);
    return hipGetLastError();
}

hipError_t launch_blackbox_merge(const BlackBoxArgs& a, MergeTerms terms, hipStream_t s) {
    if (a.B < 1 || a.N < 1 || a.max_out < 1 || a.max_out > NMS_MAX_OUT || !terms.within || !terms.between || !terms.members) return hipErrorInvalidValue;
    const bool lds_pool = (long long)a.N * a.max_out <= BB_POOL_LDS_CAP;
    if (!lds_pool && (!a.pool_top || !a.pool_corners)) return hipErrorInvalidValue;
    constexpr int LDS = BB_POOL_LDS_CAP * 20;
    const size_t dyn = lds_pool ? LDS : 0;
    static PerDeviceOnce once8, once4;
    if (a.C == 8) {
        bool& attr_set = *once8.slot();
        if (!attr_set) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(bb_merge_kernel<8>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
            if (e != hipSuccess) return e;
            attr_set = true;
        }
        hipLaunchKernelGGL(bb_merge_kernel<8>, dim3(a.B), dim3(BB_BLOCK), dyn, s, a, terms);
    } else if (a.C == 4) {
        bool& attr_set = *once4.slot();
        if (!attr_set) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(bb_merge_kernel<4>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
            if (e != hipSuccess) return e;
            attr_set = true;
        }
        hipLaunchKernelGGL(bb_merge_kernel<4>, dim3(a.B), dim3(BB_BLOCK), dyn, s, a, terms);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

__global__ void iou_matrix_kernel(const float4* boxes, int M, float* out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    if (j < M) out[(size_t)i * M + j] = iou_plus1(boxes[i], boxes[j]);
}

// ------------------------------------------------------------------------------------------------
// Detection records for the path's one multi-GPU exchange: per image K padded rows of
// W = 1 + 4 + 16 + 2C floats -- [valid, mean (v,u,h,w), covariance row-major, score[C], counts[C]] -- zero beyond the image's
// detection count.  The layout of distributed.pack_records, written by one kernel instead of five torch ops.  A handle with
// covariance parts appends their 48 floats behind the counts, one with class-entropy parts its four last: `parts` / `cparts`
// are nullptr on a handle without them (record_fields, record_state.h: the row's field offsets).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pack_records_kernel(const int32_t* __restrict__ num, const float* __restrict__ scores,
                                                           const float* __restrict__ means, const float* __restrict__ covs,
                                                           const float* __restrict__ counts, const float* __restrict__ parts,
                                                           const float* __restrict__ cparts, float* __restrict__ rec, int B, int K, int C) {
    const RecordFields f = record_fields(C, parts != nullptr, cparts != nullptr);
    const int W = f.width;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * K * W) return;
    const int w = (int)(i % W);
    const long row = i / W;                      // b * K + k
    const int b = (int)(row / K), k = (int)(row % K);
    float v = 0.f;
    if (k < num[b]) {
        if (w < f.mean) v = 1.f;
        else if (w < f.cov) v = means[row * REC_MEAN + (w - f.mean)];
        else if (w < f.score) v = covs[row * REC_COV + (w - f.cov)];
        else if (w < f.count) v = scores[row * C + (w - f.score)];
        else if (w < f.parts) v = counts[row * C + (w - f.count)];
        else if (w < f.cparts) v = parts[row * REC_PARTS + (w - f.parts)];
        else v = cparts[row * REC_CPARTS + (w - f.cparts)];
    }
    rec[i] = v;
}

hipError_t launch_pack_records(const int32_t* num, const float* scores, const float* means, const float* covs, const float* counts,
                               const float* parts, const float* cparts, float* rec, int B, int K, int C, hipStream_t s) {
    const long n = (long)B * K * record_fields(C, parts != nullptr, cparts != nullptr).width;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(pack_records_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, num, scores, means, covs, counts, parts, cparts,
                       rec, B, K, C);
    return hipGetLastError();
}

hipError_t launch_iou_matrix(const float* corners, int M, float* out, hipStream_t s) {
    if (M <= 0) return hipSuccess;
    hipLaunchKernelGGL(iou_matrix_kernel, dim3((M + 255) / 256, M), dim3(256), 0, s,
                       reinterpret_cast<const float4*>(corners), M, out);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Frame preprocessing on the device (the dataset handlers' work between image decode and
// sample_dict['image_normalized']): uint8 RGB -> [optional KITTI bilinear resize + centred crop / zero pad]
// -> float32, mean subtraction, RGB -> BGR  (bdd_dataset_handler.py:128-139, kitti_dataset_handler.py:120-148).
// One thread per output pixel; fp32 operation order identical to oracle/preprocess.py (this file is built
// with -ffp-contract=off), so results are bit-exact.
// ------------------------------------------------------------------------------------------------
// One output pixel (y, x) of a frame whose source starts at `src`: the geometry fields are PreprocArgs' / PreprocFrame's.
// kAug (preprocess_augment_kernel only) adds the mirror of the source columns and the photometric step; without it flip, gain and
// bias are not read and the code is what the two plain kernels have always run.
template <bool kAug>
__device__ __forceinline__ void preprocess_pixel(const uint8_t* src, float* o, const int y, const int x, const int sh, const int sw,
                                                 const int rh, const int rw, const int crop_y, const int crop_x, const int pad_y,
                                                 const int pad_x, const int vis_h, const int vis_w, const int resize,
                                                 const float scale_y, const float scale_x, const float* mean, const int flip = 0,
                                                 const float gain = 1.f, const float bias = 0.f) {
    const int ry = y - pad_y + crop_y, rx = x - pad_x + crop_x;             // coordinates in the (resized) source
    float v[3] = {0.f, 0.f, 0.f};                                            // zero padding (before mean subtraction)
    const bool inside = y >= pad_y && x >= pad_x && ry < rh && rx < rw && ry >= 0 && rx >= 0 &&
                        y - pad_y < vis_h && x - pad_x < vis_w;
    if (inside) {
        if (!resize) {
            const uint8_t* p = src + ((size_t)ry * sw + (kAug && flip ? sw - 1 - rx : rx)) * 3;
            v[0] = (float)p[0]; v[1] = (float)p[1]; v[2] = (float)p[2];
        } else {
            const float fy = ((float)ry + 0.5f) * scale_y - 0.5f;
            const float fx = ((float)rx + 0.5f) * scale_x - 0.5f;
            const float fy0 = floorf(fy), fx0 = floorf(fx);
            const float ly = fy - fy0, lx = fx - fx0;
            const int y0 = min(max((int)fy0, 0), sh - 1), y1 = min(max((int)ceilf(fy), 0), sh - 1);
            int x0 = min(max((int)fx0, 0), sw - 1), x1 = min(max((int)ceilf(fx), 0), sw - 1);
            if (kAug && flip) { x0 = sw - 1 - x0; x1 = sw - 1 - x1; }      // the taps keep their roles in the lerp: lx is unchanged
            const uint8_t* p00 = src + ((size_t)y0 * sw + x0) * 3;
            const uint8_t* p01 = src + ((size_t)y0 * sw + x1) * 3;
            const uint8_t* p10 = src + ((size_t)y1 * sw + x0) * 3;
            const uint8_t* p11 = src + ((size_t)y1 * sw + x1) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float tl = (float)p00[c], tr = (float)p01[c], bl = (float)p10[c], br = (float)p11[c];
                const float top = tl + (tr - tl) * lx;
                const float bot = bl + (br - bl) * lx;
                v[c] = top + (bot - top) * ly;
            }
        }
        if (kAug) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float t = gain * v[c];
                t = t + bias;
                v[c] = fminf(fmaxf(t, 0.f), 255.f);
            }
        }
    }
    o[0] = v[2] - mean[2]; o[1] = v[1] - mean[1]; o[2] = v[0] - mean[0];
}

__global__ __launch_bounds__(256) void preprocess_kernel(PreprocArgs a) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y, b = blockIdx.z;
    if (x >= a.W) return;
    preprocess_pixel<false>(a.src + (size_t)b * a.sh * a.sw * 3, a.dst + (((size_t)b * a.H + y) * a.W + x) * 3, y, x, a.sh, a.sw, a.rh,
                            a.rw, a.crop_y, a.crop_x, a.pad_y, a.pad_x, a.vis_h, a.vis_w, a.resize, a.scale_y, a.scale_x, a.mean);
}

hipError_t launch_preprocess(const PreprocArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(preprocess_kernel, dim3((a.W + 255) / 256, a.H, a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

// The same pixel for a batch of frames of mixed source sizes: grid z = frame, whose record of the geometry table gives its
// 64-bit offset into the packed buffer and its own resize / crop / pad.  Same fp32 operations in the same order as above.
__global__ __launch_bounds__(256) void preprocess_ragged_kernel(PreprocRaggedArgs a) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y, b = blockIdx.z;
    if (x >= a.W) return;
    const PreprocFrame f = a.frames[b];
    preprocess_pixel<false>(a.src + f.offset, a.dst + (((size_t)b * a.H + y) * a.W + x) * 3, y, x, f.sh, f.sw, f.rh, f.rw,
                     f.crop_y, f.crop_x, f.pad_y, f.pad_x, f.vis_h, f.vis_w, a.resize, f.scale_y, f.scale_x, a.mean);
}

hipError_t launch_preprocess_ragged(const PreprocRaggedArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(preprocess_ragged_kernel, dim3((a.W + 255) / 256, a.H, a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

// The same pixel of a training frame shown in a random form: the record adds a per-frame resize switch, the mirror bit and the
// photometric pair (PreprocAugFrame).  The record is uniform over a workgroup (grid z = frame), so its loads are scalar.
__global__ __launch_bounds__(256) void preprocess_augment_kernel(PreprocAugArgs a) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y, b = blockIdx.z;
    if (x >= a.W) return;
    const PreprocAugFrame r = a.frames[b];
    const PreprocFrame& f = r.g;
    preprocess_pixel<true>(a.src + f.offset, a.dst + (((size_t)b * a.H + y) * a.W + x) * 3, y, x, f.sh, f.sw, f.rh, f.rw,
                           f.crop_y, f.crop_x, f.pad_y, f.pad_x, f.vis_h, f.vis_w, r.resize, f.scale_y, f.scale_x, a.mean, r.flip,
                           r.gain, r.bias);
}

hipError_t launch_preprocess_augment(const PreprocAugArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(preprocess_augment_kernel, dim3((a.W + 255) / 256, a.H, a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

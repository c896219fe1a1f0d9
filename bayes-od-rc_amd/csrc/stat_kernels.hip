// MC statistics that can be accumulated and merged (include/bayesod.h, "statistics handles"): the per-anchor record the last
// tower layers' epilogues reduce over the samples of ONE forward (conv_igemm.hip agg_reduce_cls / agg_reduce_box / agg_reduce_cov)
//
//   cls_sum     [B,A,C]   sum over samples of softmax(logits)
//   box_moments [B,A,16]  Welford mean[4] of the decoded boxes, lower triangle of the co-moment sums M2 row-major [10], 0, 0
//   cov_sum     [B,A,10]  sum over samples of the raw covariance parameters (absent without the covariance head)
//   ent_sum     [B,A]     sum over samples of H(softmax(logits)) (BOD_PARTS_CLASS handles only; agg_reduce_cls<C, true>)
//
// produced from raw [B,n,A,.] head outputs (stat_from_raw_kernel: handles without an aggregating plan) and folded into an
// accumulator of ka samples (stat_merge_kernel).  The file is built with -ffp-contract=off, the correctly rounded division and the
// library expf: stat_from_raw_kernel's results are compared with the fused epilogues' for equality, stat_merge_kernel's with a
// float64 statement of the same formula.
//
// The mirror map of a record (horizontal-flip test-time views): a forward of the frames mirrored left-right yields the record of
// the mirrored anchors; mapping it back is exact in fp32.  With K anchors per location and level l of W_l columns starting at
// anchor off_l, anchor a = off_l + (y * W_l + x) * K + k has the partner a' = off_l + (y * W_l + (W_l - 1 - x)) * K + k (a level
// of one column and the middle column of an odd width are their own partners), and the result at a' from the source record at a is
//   cls_sum      copied (and so is ent_sum)
//   mean         (v, u, h, w) -> (v, float(image_w - 1) - u, h, w): the flip of the augmented upload's ground truth, x' = (w-1) - x
//   M2           the entries with exactly one index equal to 1 -- stored positions 1 (1,0), 4 (2,1), 7 (3,1) -- negated; pads 0
//   cov_sum      the parameters fill_triangular_4 places at (1,0), (2,1), (3,1) -- indices 8, 6, 2 -- negated (S M S with
//                S = diag(1,-1,1,1) on the unit-diagonal factor gives Sigma -> S Sigma S^T; the diagonal D is untouched)
// stat_merge_mirror_kernel is stat_merge_kernel with the source read through this map: merge(acc, mirror(src)) operation for
// operation.  distributed.mirror_statistics_np is the same map in NumPy.
#include "kernels.h"
#include <math.h>
#include <algorithm>

#define STAT_BLOCK 256
#define STAT_MAX_GRID 2048          // memory-bound: grid-stride beyond 8 blocks per compute unit

// One thread per (image, anchor); the same operations in the same order as agg_reduce_cls / agg_reduce_box / agg_reduce_cov, whose
// tile holds the n samples of a pixel as LDS rows -- here they are rows of the raw tensors.
template <int C, bool ENT>
__global__ __launch_bounds__(STAT_BLOCK) void stat_from_raw_kernel(StatRawArgs a) {
    const size_t BA = (size_t)a.B * a.A;
    for (size_t idx = (size_t)blockIdx.x * STAT_BLOCK + threadIdx.x; idx < BA; idx += (size_t)gridDim.x * STAT_BLOCK) {
        const size_t b = idx / (size_t)a.A, an = idx - b * (size_t)a.A;
        const size_t row0 = b * (size_t)a.N * a.A + an;                  // sample 0; sample n at row0 + n * A
        {   // sum_n softmax(logits)
            float mp[C];
            float ent = 0.f;
#pragma unroll
            for (int j = 0; j < C; ++j) mp[j] = 0.f;
            for (int n = 0; n < a.N; ++n) {
                const float* l = a.cls + (row0 + (size_t)n * a.A) * C;
                float v[C];
#pragma unroll
                for (int k = 0; k < C / 4; ++k) {
                    const float4 t = reinterpret_cast<const float4*>(l)[k];
                    v[4 * k] = t.x; v[4 * k + 1] = t.y; v[4 * k + 2] = t.z; v[4 * k + 3] = t.w;
                }
                float mx = v[0];
#pragma unroll
                for (int j = 1; j < C; ++j) mx = fmaxf(mx, v[j]);
                float sden = 0.f;
                if constexpr (ENT) {
                    float dot = 0.f;
#pragma unroll
                    for (int j = 0; j < C; ++j) { const float d = v[j] - mx; v[j] = expf(d); sden += v[j]; dot += v[j] * d; }
                    ent += BOD_LOG_SDEN(sden) - dot / sden;
                } else {
#pragma unroll
                    for (int j = 0; j < C; ++j) { v[j] = expf(v[j] - mx); sden += v[j]; }
                }
#pragma unroll
                for (int j = 0; j < C; ++j) mp[j] += v[j] / sden;
            }
            float* o = a.cls_sum + idx * C;
#pragma unroll
            for (int k = 0; k < C / 4; ++k) reinterpret_cast<float4*>(o)[k] = make_float4(mp[4 * k], mp[4 * k + 1], mp[4 * k + 2], mp[4 * k + 3]);
            if constexpr (ENT) a.ent_sum[idx] = ent;
        }
        {   // Welford mean and co-moment sums of the decoded boxes
            const float4 anc = reinterpret_cast<const float4*>(a.anchors)[an];
            float mean[4] = {0.f, 0.f, 0.f, 0.f}, m2[10];
#pragma unroll
            for (int k = 0; k < 10; ++k) m2[k] = 0.f;
            for (int n = 0; n < a.N; ++n) {
                const float4 t = reinterpret_cast<const float4*>(a.box)[row0 + (size_t)n * a.A];
                float x[4];
                x[0] = anc.z * t.x / 10.0f + anc.x;
                x[1] = anc.w * t.y / 10.0f + anc.y;
                x[2] = anc.z * fminf(fmaxf(expf(t.z / 5.0f), 1e-4f), 1e4f);
                x[3] = anc.w * fminf(fmaxf(expf(t.w / 5.0f), 1e-4f), 1e4f);
                const float inv = 1.0f / (float)(n + 1);
                float d[4], e[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) { d[i] = x[i] - mean[i]; mean[i] += d[i] * inv; e[i] = x[i] - mean[i]; }
                int k = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j <= i; ++j) m2[k++] += d[i] * e[j];
            }
            float4* o = reinterpret_cast<float4*>(a.box_moments + idx * 16);
            o[0] = make_float4(mean[0], mean[1], mean[2], mean[3]);
            o[1] = make_float4(m2[0], m2[1], m2[2], m2[3]);
            o[2] = make_float4(m2[4], m2[5], m2[6], m2[7]);
            o[3] = make_float4(m2[8], m2[9], 0.f, 0.f);
        }
        if (a.cov) {   // sum_n of the covariance parameters (rows of 10 floats: 8-byte aligned)
            float acc[10];
#pragma unroll
            for (int k = 0; k < 10; ++k) acc[k] = 0.f;
            for (int n = 0; n < a.N; ++n) {
                const float2* p = reinterpret_cast<const float2*>(a.cov + (row0 + (size_t)n * a.A) * 10);
#pragma unroll
                for (int k = 0; k < 5; ++k) { const float2 t = p[k]; acc[2 * k] += t.x; acc[2 * k + 1] += t.y; }
            }
            float2* o = reinterpret_cast<float2*>(a.cov_sum + idx * 10);
#pragma unroll
            for (int k = 0; k < 5; ++k) o[k] = make_float2(acc[2 * k], acc[2 * k + 1]);
        }
    }
}

hipError_t launch_stat_from_raw(const StatRawArgs& a, hipStream_t s) {
    if (a.B < 1 || a.N < 1 || a.A < 1 || (a.C != 4 && a.C != 8) || !a.cls || !a.box || !a.anchors || !a.cls_sum || !a.box_moments ||
        ((a.cov != nullptr) != (a.cov_sum != nullptr)))
        return hipErrorInvalidValue;
    const size_t BA = (size_t)a.B * a.A;
    const unsigned grid = (unsigned)std::min<size_t>((BA + STAT_BLOCK - 1) / STAT_BLOCK, STAT_MAX_GRID);
    if (a.ent_sum) {
        if (a.C == 8) hipLaunchKernelGGL((stat_from_raw_kernel<8, true>), dim3(grid), dim3(STAT_BLOCK), 0, s, a);
        else hipLaunchKernelGGL((stat_from_raw_kernel<4, true>), dim3(grid), dim3(STAT_BLOCK), 0, s, a);
    } else {
        if (a.C == 8) hipLaunchKernelGGL((stat_from_raw_kernel<8, false>), dim3(grid), dim3(STAT_BLOCK), 0, s, a);
        else hipLaunchKernelGGL((stat_from_raw_kernel<4, false>), dim3(grid), dim3(STAT_BLOCK), 0, s, a);
    }
    return hipGetLastError();
}

// accumulator (ka samples) <- accumulator (+) source (kb samples), one pass, 16-byte loads and stores, no atomics.  The work items
// of the three arrays are laid end to end: [0, BA) one box record each, then the float4s of cls_sum, then those of cov_sum (whose
// last item may be a partial one: B*A*10 need not be a multiple of 4).  Operation order, per (image, anchor):
//   cls_sum, cov_sum:  acc = acc + src
//   d_i   = mean_b,i - mean_a,i            w = kb / (ka + kb)            kw = ka * w
//   mean_i = mean_a,i + d_i * w
//   M2_ij  = (M2a_ij + M2b_ij) + (d_i * d_j) * kw          for the 10 stored entries, i >= j
//   pads   = 0
// ka == 0: every array is a copy of the source (the accumulator's old contents are not read).
template <int C>
__global__ __launch_bounds__(STAT_BLOCK) void stat_merge_kernel(StatMergeArgs a) {
    const size_t n_box = a.BA, n_cls = a.BA * (C / 4), cov_f = a.acc_cov ? a.BA * 10 : 0, n_cov = (cov_f + 3) / 4;
    const size_t total = n_box + n_cls + n_cov;
    const bool copy = a.ka == 0;
    const float fka = (float)a.ka, fkb = (float)a.kb;
    const float w = fkb / (fka + fkb);
    const float kw = fka * w;
    for (size_t it = (size_t)blockIdx.x * STAT_BLOCK + threadIdx.x; it < total; it += (size_t)gridDim.x * STAT_BLOCK) {
        if (it < n_box) {
            const float4* sb = reinterpret_cast<const float4*>(a.src_box) + it * 4;
            float4* ab = reinterpret_cast<float4*>(a.acc_box) + it * 4;
            const float4 s0 = sb[0], s1 = sb[1], s2 = sb[2], s3 = sb[3];
            if (copy) {
                ab[0] = s0; ab[1] = s1; ab[2] = s2; ab[3] = make_float4(s3.x, s3.y, 0.f, 0.f);
                continue;
            }
            const float4 a0 = ab[0], a1 = ab[1], a2 = ab[2], a3 = ab[3];
            const float ma[4] = {a0.x, a0.y, a0.z, a0.w}, mb[4] = {s0.x, s0.y, s0.z, s0.w};
            const float qa[10] = {a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w, a3.x, a3.y};
            const float qb[10] = {s1.x, s1.y, s1.z, s1.w, s2.x, s2.y, s2.z, s2.w, s3.x, s3.y};
            float d[4], m[4], q[10];
#pragma unroll
            for (int i = 0; i < 4; ++i) { d[i] = mb[i] - ma[i]; m[i] = ma[i] + d[i] * w; }
            int k = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j) { q[k] = (qa[k] + qb[k]) + (d[i] * d[j]) * kw; ++k; }
            ab[0] = make_float4(m[0], m[1], m[2], m[3]);
            ab[1] = make_float4(q[0], q[1], q[2], q[3]);
            ab[2] = make_float4(q[4], q[5], q[6], q[7]);
            ab[3] = make_float4(q[8], q[9], 0.f, 0.f);
            continue;
        }
        size_t j = it - n_box;
        const float* src = a.src_cls;
        float* acc = a.acc_cls;
        size_t floats = n_cls * 4;
        if (j >= n_cls) { j -= n_cls; src = a.src_cov; acc = a.acc_cov; floats = cov_f; }
        if (j * 4 + 4 <= floats) {
            const float4 sv = reinterpret_cast<const float4*>(src)[j];
            float4 r = sv;
            if (!copy) {
                const float4 av = reinterpret_cast<const float4*>(acc)[j];
                r = make_float4(av.x + sv.x, av.y + sv.y, av.z + sv.z, av.w + sv.w);
            }
            reinterpret_cast<float4*>(acc)[j] = r;
        } else {
            for (size_t e = j * 4; e < floats; ++e) acc[e] = copy ? src[e] : acc[e] + src[e];
        }
    }
}

hipError_t launch_stat_merge(const StatMergeArgs& a, hipStream_t s) {
    if (a.BA < 1 || (a.C != 4 && a.C != 8) || a.ka < 0 || a.kb < 1 || !a.acc_cls || !a.acc_box || !a.src_cls || !a.src_box ||
        ((a.acc_cov != nullptr) != (a.src_cov != nullptr)))
        return hipErrorInvalidValue;
    const void* p[6] = {a.acc_cls, a.acc_box, a.acc_cov, a.src_cls, a.src_box, a.src_cov};
    for (const void* q : p)
        if ((reinterpret_cast<uintptr_t>(q) & 15u) != 0) return hipErrorInvalidValue;          // 16-byte loads and stores
    const size_t total = a.BA + a.BA * (size_t)a.C / 4 + (a.acc_cov ? (a.BA * 10 + 3) / 4 : 0);
    const unsigned grid = (unsigned)std::min<size_t>((total + STAT_BLOCK - 1) / STAT_BLOCK, STAT_MAX_GRID);
    if (a.C == 8) hipLaunchKernelGGL(stat_merge_kernel<8>, dim3(grid), dim3(STAT_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(stat_merge_kernel<4>, dim3(grid), dim3(STAT_BLOCK), 0, s, a);
    return hipGetLastError();
}

// accumulator (ka samples) <- accumulator (+) mirror(source) (kb samples): stat_merge_kernel's formula, indexed by DESTINATION
// anchor so that every write is a contiguous 16-byte (box, cls) or 8-byte (cov rows of 10 floats) store; the source is gathered
// from the partner anchor of the same pyramid row.  Work items end to end: [0, BA) one box record each, then the float4s of
// cls_sum, then one cov_sum row each.  No atomics, one pass.
__device__ __forceinline__ size_t stat_mirror_partner(const StatMirrorArgs& a, size_t idx) {
    const size_t b = idx / (size_t)a.A;
    const int an = (int)(idx - b * (size_t)a.A);
    int off = 0, w = a.lvl_w[0];                   // constant indices only: the table stays in scalar registers
#pragma unroll
    for (int l = 1; l < 8; ++l)
        if (l < a.nlev && an >= a.lvl_off[l]) { off = a.lvl_off[l]; w = a.lvl_w[l]; }
    const int x = ((an - off) / a.K) % w;
    return b * (size_t)a.A + (size_t)(an + (w - 1 - 2 * x) * a.K);
}

template <int C>
__global__ __launch_bounds__(STAT_BLOCK) void stat_merge_mirror_kernel(StatMirrorArgs a) {
    const StatMergeArgs& m = a.m;
    const size_t n_box = m.BA, n_cls = m.BA * (C / 4), n_cov = m.acc_cov ? m.BA : 0;
    const size_t total = n_box + n_cls + n_cov;
    const bool copy = m.ka == 0;
    const float fka = (float)m.ka, fkb = (float)m.kb;
    const float w = fkb / (fka + fkb);
    const float kw = fka * w;
    for (size_t it = (size_t)blockIdx.x * STAT_BLOCK + threadIdx.x; it < total; it += (size_t)gridDim.x * STAT_BLOCK) {
        if (it < n_box) {
            const float4* sb = reinterpret_cast<const float4*>(m.src_box) + stat_mirror_partner(a, it) * 4;
            float4* ab = reinterpret_cast<float4*>(m.acc_box) + it * 4;
            const float4 s0 = sb[0], s1 = sb[1], s2 = sb[2], s3 = sb[3];
            const float mb[4] = {s0.x, a.u_flip - s0.y, s0.z, s0.w};
            const float qb[10] = {s1.x, -s1.y, s1.z, s1.w, -s2.x, s2.y, s2.z, -s2.w, s3.x, s3.y};
            if (copy) {
                ab[0] = make_float4(mb[0], mb[1], mb[2], mb[3]);
                ab[1] = make_float4(qb[0], qb[1], qb[2], qb[3]);
                ab[2] = make_float4(qb[4], qb[5], qb[6], qb[7]);
                ab[3] = make_float4(qb[8], qb[9], 0.f, 0.f);
                continue;
            }
            const float4 a0 = ab[0], a1 = ab[1], a2 = ab[2], a3 = ab[3];
            const float ma[4] = {a0.x, a0.y, a0.z, a0.w};
            const float qa[10] = {a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w, a3.x, a3.y};
            float d[4], mn[4], q[10];
#pragma unroll
            for (int i = 0; i < 4; ++i) { d[i] = mb[i] - ma[i]; mn[i] = ma[i] + d[i] * w; }
            int k = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j) { q[k] = (qa[k] + qb[k]) + (d[i] * d[j]) * kw; ++k; }
            ab[0] = make_float4(mn[0], mn[1], mn[2], mn[3]);
            ab[1] = make_float4(q[0], q[1], q[2], q[3]);
            ab[2] = make_float4(q[4], q[5], q[6], q[7]);
            ab[3] = make_float4(q[8], q[9], 0.f, 0.f);
            continue;
        }
        size_t j = it - n_box;
        if (j < n_cls) {
            const size_t an = j / (C / 4), part = j - an * (C / 4);
            const float4 sv = reinterpret_cast<const float4*>(m.src_cls)[stat_mirror_partner(a, an) * (C / 4) + part];
            float4 r = sv;
            if (!copy) {
                const float4 av = reinterpret_cast<const float4*>(m.acc_cls)[j];
                r = make_float4(av.x + sv.x, av.y + sv.y, av.z + sv.z, av.w + sv.w);
            }
            reinterpret_cast<float4*>(m.acc_cls)[j] = r;
            continue;
        }
        j -= n_cls;
        const float2* sp = reinterpret_cast<const float2*>(m.src_cov + stat_mirror_partner(a, j) * 10);
        float2* ap = reinterpret_cast<float2*>(m.acc_cov + j * 10);
        float sv[10];
#pragma unroll
        for (int k = 0; k < 5; ++k) { const float2 t = sp[k]; sv[2 * k] = t.x; sv[2 * k + 1] = t.y; }
        sv[2] = -sv[2]; sv[6] = -sv[6]; sv[8] = -sv[8];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            float2 r = make_float2(sv[2 * k], sv[2 * k + 1]);
            if (!copy) { const float2 av = ap[k]; r = make_float2(av.x + r.x, av.y + r.y); }
            ap[k] = r;
        }
    }
}

hipError_t launch_stat_merge_mirror(const StatMirrorArgs& a, hipStream_t s) {
    const StatMergeArgs& m = a.m;
    if (m.BA < 1 || (m.C != 4 && m.C != 8) || m.ka < 0 || m.kb < 1 || !m.acc_cls || !m.acc_box || !m.src_cls || !m.src_box ||
        ((m.acc_cov != nullptr) != (m.src_cov != nullptr)))
        return hipErrorInvalidValue;
    const void* p[6] = {m.acc_cls, m.acc_box, m.acc_cov, m.src_cls, m.src_box, m.src_cov};
    for (const void* q : p)
        if ((reinterpret_cast<uintptr_t>(q) & 15u) != 0) return hipErrorInvalidValue;
    // the level table covers [0, A) in whole pyramid rows: every partner stays inside its own row
    if (a.A < 1 || a.K < 1 || a.nlev < 1 || a.nlev > 8 || m.BA % a.A != 0 || a.lvl_off[0] != 0 || a.lvl_off[a.nlev] != a.A) return hipErrorInvalidValue;
    for (int l = 0; l < a.nlev; ++l) {
        const int span = a.lvl_off[l + 1] - a.lvl_off[l];
        if (a.lvl_w[l] < 1 || span < 1 || span % (a.lvl_w[l] * a.K) != 0) return hipErrorInvalidValue;
    }
    const size_t total = (size_t)m.BA * (1 + (size_t)m.C / 4 + (m.acc_cov ? 1 : 0));
    const unsigned grid = (unsigned)std::min<size_t>((total + STAT_BLOCK - 1) / STAT_BLOCK, STAT_MAX_GRID);
    if (m.C == 8) hipLaunchKernelGGL(stat_merge_mirror_kernel<8>, dim3(grid), dim3(STAT_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(stat_merge_mirror_kernel<4>, dim3(grid), dim3(STAT_BLOCK), 0, s, a);
    return hipGetLastError();
}

// The record's fourth array, ent_sum [BA]: acc = acc + src (independent of the sample counts), or a copy of the source into an
// empty accumulator.  One float4 per work item (the last one may be partial), no atomics.  MIRROR: the source is gathered from the
// partner anchor of stat_merge_mirror_kernel's map; an entropy is unchanged under the mirror.
template <bool MIRROR>
__global__ __launch_bounds__(STAT_BLOCK) void stat_merge_entropy_kernel(float* __restrict__ acc, const float* __restrict__ src, size_t BA, int copy,
                                                                        StatMirrorArgs a) {
    const size_t total = (BA + 3) / 4;
    for (size_t it = (size_t)blockIdx.x * STAT_BLOCK + threadIdx.x; it < total; it += (size_t)gridDim.x * STAT_BLOCK) {
        const size_t e0 = it * 4;
        if (e0 + 4 <= BA) {
            float4 sv;
            if constexpr (MIRROR) {
                sv = make_float4(src[stat_mirror_partner(a, e0)], src[stat_mirror_partner(a, e0 + 1)], src[stat_mirror_partner(a, e0 + 2)],
                                 src[stat_mirror_partner(a, e0 + 3)]);
            } else {
                sv = reinterpret_cast<const float4*>(src)[it];
            }
            float4 r = sv;
            if (!copy) {
                const float4 av = reinterpret_cast<const float4*>(acc)[it];
                r = make_float4(av.x + sv.x, av.y + sv.y, av.z + sv.z, av.w + sv.w);
            }
            reinterpret_cast<float4*>(acc)[it] = r;
        } else {
            for (size_t e = e0; e < BA; ++e) {
                const float sv = MIRROR ? src[stat_mirror_partner(a, e)] : src[e];
                acc[e] = copy ? sv : acc[e] + sv;
            }
        }
    }
}

hipError_t launch_stat_merge_entropy(float* acc, const float* src, int64_t BA, int copy, const StatMirrorArgs* mirror, hipStream_t s) {
    if (!acc || !src || acc == src || BA < 1) return hipErrorInvalidValue;
    if (((reinterpret_cast<uintptr_t>(acc) | reinterpret_cast<uintptr_t>(src)) & 15u) != 0) return hipErrorInvalidValue;
    const size_t total = ((size_t)BA + 3) / 4;
    const unsigned grid = (unsigned)std::min<size_t>((total + STAT_BLOCK - 1) / STAT_BLOCK, STAT_MAX_GRID);
    if (mirror) {
        const StatMirrorArgs& a = *mirror;
        if (a.A < 1 || a.K < 1 || a.nlev < 1 || a.nlev > 8 || BA % a.A != 0 || a.lvl_off[0] != 0 || a.lvl_off[a.nlev] != a.A) return hipErrorInvalidValue;
        for (int l = 0; l < a.nlev; ++l) {
            const int span = a.lvl_off[l + 1] - a.lvl_off[l];
            if (a.lvl_w[l] < 1 || span < 1 || span % (a.lvl_w[l] * a.K) != 0) return hipErrorInvalidValue;
        }
        hipLaunchKernelGGL(stat_merge_entropy_kernel<true>, dim3(grid), dim3(STAT_BLOCK), 0, s, acc, src, (size_t)BA, copy, a);
    } else {
        hipLaunchKernelGGL(stat_merge_entropy_kernel<false>, dim3(grid), dim3(STAT_BLOCK), 0, s, acc, src, (size_t)BA, copy, StatMirrorArgs{});
    }
    return hipGetLastError();
}

// out[b,y,x,:] = in[b,y,W-1-x,:] for fp32 [B,H,W,3] frames: one thread per pixel (12 bytes in, 12 bytes out; a wave reads and
// writes 768 contiguous bytes).  in and out are different buffers.
struct Pixel3 { float c[3]; };
__global__ __launch_bounds__(STAT_BLOCK) void mirror_images_kernel(const Pixel3* __restrict__ in, Pixel3* __restrict__ out, size_t rows, int W) {
    const size_t total = rows * (size_t)W;
    for (size_t idx = (size_t)blockIdx.x * STAT_BLOCK + threadIdx.x; idx < total; idx += (size_t)gridDim.x * STAT_BLOCK) {
        const size_t row = idx / (size_t)W;
        const int x = (int)(idx - row * (size_t)W);
        out[idx] = in[row * (size_t)W + (size_t)(W - 1 - x)];
    }
}

hipError_t launch_mirror_images(const float* in, float* out, int B, int H, int W, hipStream_t s) {
    if (!in || !out || in == out || B < 1 || H < 1 || W < 1) return hipErrorInvalidValue;
    const size_t total = (size_t)B * H * W;
    const unsigned grid = (unsigned)std::min<size_t>((total + STAT_BLOCK - 1) / STAT_BLOCK, STAT_MAX_GRID);
    hipLaunchKernelGGL(mirror_images_kernel, dim3(grid), dim3(STAT_BLOCK), 0, s, reinterpret_cast<const Pixel3*>(in),
                       reinterpret_cast<Pixel3*>(out), (size_t)B * H, W);
    return hipGetLastError();
}

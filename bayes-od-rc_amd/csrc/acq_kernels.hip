// Acquisition scores of a statistics handle (include/bayesod.h, bod_stat_acquisition): the per-anchor record of
// K >= 2 merged MC samples (stat_kernels.hip: cls_sum [B,A,C], box_moments [B,A,16], cov_sum [B,A,10], ent_sum [B,A]) reduced to
// twelve numbers per frame and three per frame and foreground class, for ranking an unlabeled pool by the model's uncertainty.
//
// Per anchor, fp32, in this order (the file is built with -ffp-contract=off and the correctly rounded division, as stat_kernels.hip):
//   bad    any non-finite float in the anchor's record (C + 16 + 10 + 1 floats, less the arrays the handle does not carry)
//   bg     cls_sum[C-1]                     in W  iff  not bad and bg <= thr          (thr = (float)((1 - min_foreground) * K), host)
//   p_j    cls_sum[j] / K                   H  = -sum_j p_j ln p_j  (p_j <= 0 contributes 0; post_class_parts_kernel's total)
//   Ha     ent_sum / K                      MI = max(H - Ha, 0)                    fg = 1 - bg / K
//   e_box  (((M2_00 + M2_11) + M2_22) + M2_33) / (K - 1) / (h * h + w * w)          (stored positions 4, 6, 9, 13; h, w = mean[2], [3])
//   lda    (((x0 + x4) + x5) + x9) / K      (x = cov_sum row: the log-determinant of post_fuse_anchor's aleatoric covariance)
//   cls    arg max_{j < C-1} cls_sum[j], the first maximum
//
// acq_pass_kernel: grid (G, B), G workgroups of 256 threads per frame (acq_groups(A)); a thread walks the frame's anchors with the
// stride G * 256, writes each anchor's MI (NaN outside W) to the [B,A] scratch and keeps fp64 sums / integer counts / fp32 maxima;
// they are reduced by wave butterflies, one LDS exchange and written as one row of NV doubles per workgroup.  acq_finish_kernel: one
// workgroup per frame folds the G rows in order, finds the k-th largest MI of the scratch by bisection on the order-preserving
// integer image of the floats and writes the frame's outputs.  No atomics anywhere: the order of every sum is fixed by the launch
// shape, which depends on A alone, so a frame's outputs depend on that frame's record alone.
#include "kernels.h"
#include <math.h>
#include <algorithm>

#define ACQ_BLOCK 256
#define ACQ_WAVES (ACQ_BLOCK / 64)

int acq_groups(int A) { return std::max(1, std::min((A + ACQ_BLOCK - 1) / ACQ_BLOCK, ACQ_MAX_GROUPS)); }

// A partial row: the sums [NS] first, then the maxima [NM]
//   sums    0 H, 1 Ha, 2 MI, 3 fg * MI, 4 fg (3, 4: every good anchor), 5 e_box, 6 lda, 7 n_fg, 8 n_bad, 9 + j anchors of class j
//   maxima  NS + 0 MI, + 1 e_box, + 2 lda, NS + 3 + 2j MI of class j, NS + 4 + 2j e_box of class j
template <int C> struct AcqRow {
    static constexpr int NS = 9 + (C - 1), NM = 3 + 2 * (C - 1), NV = NS + NM;
};

__device__ __forceinline__ bool acq_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

template <int C, bool ENT, bool COV>
__global__ __launch_bounds__(ACQ_BLOCK) void acq_pass_kernel(AcqArgs a) {
    constexpr int NS = AcqRow<C>::NS, NV = AcqRow<C>::NV;
    static_assert(NV <= ACQ_ROW_MAX, "partial row");
    __shared__ double lds[ACQ_WAVES][NV];
    const int b = blockIdx.y;
    const size_t base = (size_t)b * a.A;
    const float fk = (float)a.K, fk1 = (float)(a.K - 1);
    const float nan = __uint_as_float(0x7fc00000u);
    double v[NV];
#pragma unroll
    for (int i = 0; i < NS; ++i) v[i] = 0.0;
#pragma unroll
    for (int i = NS; i < NV; ++i) v[i] = -INFINITY;
    for (int an = blockIdx.x * ACQ_BLOCK + threadIdx.x; an < a.A; an += gridDim.x * ACQ_BLOCK) {
        const size_t idx = base + an;
        float cs[C];
        bool good = true;
        {
            const float4* l = reinterpret_cast<const float4*>(a.cls_sum + idx * C);
#pragma unroll
            for (int k = 0; k < C / 4; ++k) {
                const float4 t = l[k];
                cs[4 * k] = t.x; cs[4 * k + 1] = t.y; cs[4 * k + 2] = t.z; cs[4 * k + 3] = t.w;
            }
#pragma unroll
            for (int j = 0; j < C; ++j) good = good && acq_finite(cs[j]);
        }
        const float4* bm = reinterpret_cast<const float4*>(a.box_moments + idx * 16);
        const float4 b0 = bm[0], b1 = bm[1], b2 = bm[2], b3 = bm[3];
        good = good && acq_finite(b0.x) && acq_finite(b0.y) && acq_finite(b0.z) && acq_finite(b0.w) && acq_finite(b1.x) && acq_finite(b1.y) &&
               acq_finite(b1.z) && acq_finite(b1.w) && acq_finite(b2.x) && acq_finite(b2.y) && acq_finite(b2.z) && acq_finite(b2.w) &&
               acq_finite(b3.x) && acq_finite(b3.y) && acq_finite(b3.z) && acq_finite(b3.w);
        float lda = 0.f;
        if constexpr (COV) {               // rows of 10 floats: 8-byte aligned
            const float2* p = reinterpret_cast<const float2*>(a.cov_sum + idx * 10);
            float x[10];
#pragma unroll
            for (int k = 0; k < 5; ++k) { const float2 t = p[k]; x[2 * k] = t.x; x[2 * k + 1] = t.y; }
#pragma unroll
            for (int k = 0; k < 10; ++k) good = good && acq_finite(x[k]);
            lda = (((x[0] + x[4]) + x[5]) + x[9]) / fk;
        }
        float es = 0.f;
        if constexpr (ENT) { es = a.ent_sum[idx]; good = good && acq_finite(es); }
        if (!good) {
            v[8] += 1.0;
            a.mi[idx] = nan;
            continue;
        }
        const float bg = cs[C - 1];
        float H = 0.f;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const float p = cs[j] / fk;
            if (p > 0.f) H -= p * logf(p);
        }
        const float Ha = es / fk;
        const float MI = fmaxf(H - Ha, 0.f);
        const float fg = 1.0f - bg / fk;
        if constexpr (ENT) { v[3] += (double)(fg * MI); v[4] += (double)fg; }
        const bool in_w = bg <= a.thr;
        a.mi[idx] = (ENT && in_w) ? MI : nan;
        if (!in_w) continue;
        const float ebox = (((b1.x + b1.z) + b2.y) + b3.y) / fk1 / (b0.z * b0.z + b0.w * b0.w);
        int cls = 0;
        float best = cs[0];
#pragma unroll
        for (int j = 1; j < C - 1; ++j)
            if (cs[j] > best) { best = cs[j]; cls = j; }
        v[0] += (double)H; v[5] += (double)ebox; v[7] += 1.0;
        v[NS + 1] = fmax(v[NS + 1], (double)ebox);
        if constexpr (ENT) { v[1] += (double)Ha; v[2] += (double)MI; v[NS] = fmax(v[NS], (double)MI); }
        if constexpr (COV) { v[6] += (double)lda; v[NS + 2] = fmax(v[NS + 2], (double)lda); }
#pragma unroll
        for (int j = 0; j < C - 1; ++j) {      // constant indices: the row stays in registers
            const bool me = j == cls;
            v[9 + j] += me ? 1.0 : 0.0;
            if constexpr (ENT) v[NS + 3 + 2 * j] = me ? fmax(v[NS + 3 + 2 * j], (double)MI) : v[NS + 3 + 2 * j];
            v[NS + 4 + 2 * j] = me ? fmax(v[NS + 4 + 2 * j], (double)ebox) : v[NS + 4 + 2 * j];
        }
    }
    // wave butterflies (every lane ends with the wave's value), one LDS exchange, the four waves in order
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int i = 0; i < NS; ++i) v[i] += __shfl_xor(v[i], off, 64);
#pragma unroll
        for (int i = NS; i < NV; ++i) v[i] = fmax(v[i], __shfl_xor(v[i], off, 64));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) lds[wave][i] = v[i];
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        const int i = threadIdx.x;
        double r = lds[0][i];
        for (int w = 1; w < ACQ_WAVES; ++w) r = i < NS ? r + lds[w][i] : fmax(r, lds[w][i]);
        a.partials[((size_t)b * gridDim.x + blockIdx.x) * NV + i] = r;
    }
}

// Sum of one int / one double per thread over the workgroup, to every thread; `slot` is reused by the next call (two barriers)
__device__ __forceinline__ int acq_block_sum(int x, int* slot) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = x;
    __syncthreads();
    const int r = (slot[0] + slot[1]) + (slot[2] + slot[3]);
    __syncthreads();
    return r;
}
__device__ __forceinline__ double acq_block_sum(double x, double* slot) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = x;
    __syncthreads();
    const double r = (slot[0] + slot[1]) + (slot[2] + slot[3]);
    __syncthreads();
    return r;
}

// float bits -> unsigned, order-preserving (NaN never gets here), and back; the scratch is read as bits: integer code up to the sum
__device__ __forceinline__ bool acq_is_nan(uint32_t u) { return (u & 0x7fffffffu) > 0x7f800000u; }
__device__ __forceinline__ uint32_t acq_key(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float acq_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

template <int C, bool ENT, bool COV>
__global__ __launch_bounds__(ACQ_BLOCK) void acq_finish_kernel(AcqArgs a) {
    constexpr int NS = AcqRow<C>::NS, NV = AcqRow<C>::NV;
    __shared__ double tot[NV];
    __shared__ int islot[ACQ_WAVES];
    __shared__ double dslot[ACQ_WAVES];
    const int b = blockIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (threadIdx.x < NV) {              // the G partial rows of the frame, in order
        const int i = threadIdx.x;
        const double* p = a.partials + (size_t)b * a.G * NV + i;
        double r = p[0];
        for (int g = 1; g < a.G; ++g) r = i < NS ? r + p[(size_t)g * NV] : fmax(r, p[(size_t)g * NV]);
        tot[i] = r;
    }
    __syncthreads();
    const int n_fg = (int)tot[7];
    double topk = nan;
    if constexpr (ENT) {
        const int k = min(a.top_k, n_fg);            // (uniform over the workgroup)
        if (k > 0) {
            const uint32_t* mi = reinterpret_cast<const uint32_t*>(a.mi) + (size_t)b * a.A;
            // the largest T with |{key >= T}| >= k is the k-th largest key: one bit per pass, from the top
            uint32_t T = 0;
            for (int bit = 31; bit >= 0; --bit) {
                const uint32_t cand = T | (1u << bit);
                int c = 0;
                for (int an = threadIdx.x; an < a.A; an += ACQ_BLOCK) {
                    const uint32_t u = mi[an];
                    c += (!acq_is_nan(u) && acq_key(u) >= cand) ? 1 : 0;
                }
                if (acq_block_sum(c, islot) >= k) T = cand;
            }
            const float t = acq_unkey(T);
            int c = 0;
            double s = 0.0;
            for (int an = threadIdx.x; an < a.A; an += ACQ_BLOCK) {
                const uint32_t u = mi[an];
                if (!acq_is_nan(u) && acq_key(u) > T) { c += 1; s += (double)__uint_as_float(u); }
            }
            const int count_gt = acq_block_sum(c, islot);
            const double sum_gt = acq_block_sum(s, dslot);
            topk = (sum_gt + (double)(k - count_gt) * (double)t) / (double)k;
        }
    }
    if (threadIdx.x == 0) {
        double* o = a.scores + (size_t)b * 12;
        const double n = tot[7];
        const bool any = n_fg > 0;
        o[0] = n;
        o[1] = tot[8];
        o[2] = any ? tot[0] / n : nan;
        o[3] = (ENT && any) ? tot[1] / n : nan;
        o[4] = (ENT && any) ? tot[2] / n : nan;
        o[5] = (ENT && any) ? tot[NS] : nan;
        o[6] = (ENT && tot[4] != 0.0) ? tot[3] / tot[4] : nan;
        o[7] = topk;
        o[8] = any ? tot[5] / n : nan;
        o[9] = any ? tot[NS + 1] : nan;
        o[10] = (COV && any) ? tot[6] / n : nan;
        o[11] = (COV && any) ? tot[NS + 2] : nan;
    }
    if (a.per_class && threadIdx.x < C - 1) {
        const int j = threadIdx.x;
        double* o = a.per_class + ((size_t)b * (C - 1) + j) * 3;
        const bool any = tot[9 + j] > 0.0;
        o[0] = tot[9 + j];
        o[1] = (ENT && any) ? tot[NS + 3 + 2 * j] : nan;
        o[2] = any ? tot[NS + 4 + 2 * j] : nan;
    }
}

template <int C, bool ENT, bool COV>
static void acq_launch(const AcqArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((acq_pass_kernel<C, ENT, COV>), dim3(a.G, a.B), dim3(ACQ_BLOCK), 0, s, a);
    hipLaunchKernelGGL((acq_finish_kernel<C, ENT, COV>), dim3(a.B), dim3(ACQ_BLOCK), 0, s, a);
}

hipError_t launch_acquisition(const AcqArgs& a, hipStream_t s) {
    if (a.B < 1 || a.B > 65535 || a.A < 1 || (a.C != 4 && a.C != 8) || a.K < 2 || a.top_k < 1 || a.G != acq_groups(a.A) || !a.cls_sum ||
        !a.box_moments || !a.mi || !a.partials || !a.scores)
        return hipErrorInvalidValue;
    if (((reinterpret_cast<uintptr_t>(a.cls_sum) | reinterpret_cast<uintptr_t>(a.box_moments)) & 15u) != 0 ||
        (reinterpret_cast<uintptr_t>(a.cov_sum) & 7u) != 0)
        return hipErrorInvalidValue;
    const int sel = (a.C == 8 ? 4 : 0) | (a.ent_sum ? 2 : 0) | (a.cov_sum ? 1 : 0);
    switch (sel) {
        case 0: acq_launch<4, false, false>(a, s); break;
        case 1: acq_launch<4, false, true>(a, s); break;
        case 2: acq_launch<4, true, false>(a, s); break;
        case 3: acq_launch<4, true, true>(a, s); break;
        case 4: acq_launch<8, false, false>(a, s); break;
        case 5: acq_launch<8, false, true>(a, s); break;
        case 6: acq_launch<8, true, false>(a, s); break;
        default: acq_launch<8, true, true>(a, s); break;
    }
    return hipGetLastError();
}

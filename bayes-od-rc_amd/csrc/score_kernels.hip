// Scoring rules of the box Gaussian on the device (scoring_rules.py): for n already-paired rows
// (mu[4], Sigma[4][4], target g[4]), all fp64,
//
//   out[0] nll    = 0.5 (4 ln 2pi + ln det Sigma + m2)
//   out[1] m2     = |L^-1 (g - mu)|^2                     L = lower Cholesky factor of Sigma
//   out[2] ES     = (1/M) sum_{i<M} |z_i - g| - 1/(2(M-1)) sum_{i<M-1} |z_i - z_{i+1}|,   z_i = mu + L n_i
//   out[3..6] PIT_k = 0.5 erfc(-(g_k - mu_k) / sqrt(2 Sigma_kk))
//   out[7] ln det Sigma = 2 sum ln L_kk
//
// L: Cholesky-Banachiewicz, row by row, in registers, on the LOWER triangle of the input (the upper one is not read).
// status 2 = a non-finite input (mu, g, lower triangle), 1 = a pivot <= 0 or non-finite, 0 otherwise; a row with status != 0
// gets NaN in all eight outputs and touches nothing else.
//
// Normals ("RNG contract"): sample i of the row with 64-bit id r = first_row_id + row is ONE call
// philox4x32_10(i, r & 0xffffffff, BOD_SCORE_TAG, r >> 32, seed_lo, seed_hi) -> (x, y, z, w), u(t) = (t + 0.5) 2^-32,
// n0, n1 = sqrt(-2 ln u(x)) (cos, sin)(2 pi u(y)), n2, n3 likewise from (z, w).  Nothing depends on n, on the row's
// position in the call or on how rows are split over calls.
//
// Shape: one wave64 per row, four rows per 256-thread workgroup; lane l takes samples l, l + 64, ...  The neighbour term
// is evaluated as |z_i - z_{i-1}| for i >= 1: lane l reads lane l-1's sample with one cross-lane read per coordinate, lane 0
// the sample lane 63 held one trip earlier -- a second Philox call plus Box-Muller per sample (two fp64 logs, two sincos)
// would cost several times the four reads.  Each lane adds its terms in sample order; the 64 partial sums are folded by
// __shfl_down at distances 32, 16, ..., 1.  No atomics, no LDS, no barrier: the result's bits are fixed.
#include "../../include/bayesod.h"
#include "host_call.h"
#include "kernels.h"
#include "philox.h"

#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>

namespace {

constexpr int SCORE_BLOCK = 256;
constexpr int SCORE_ROWS_PER_BLOCK = SCORE_BLOCK / 64;
constexpr int SCORE_BATCH_ROWS = 1 << 18;           // rows of one internal batch: 33 doubles + 1 int each, about 70 MB on the device
constexpr double SCORE_TWO_PI = 6.283185307179586;
constexpr double SCORE_LN_2PI = 1.8378770664093453;

__device__ __forceinline__ double score_uniform(uint32_t t) { return ((double)t + 0.5) * 2.3283064365386963e-10; }   // 2^-32

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;                                       // lane 0 holds the total
}

__global__ __launch_bounds__(SCORE_BLOCK) void score_pairs_kernel(const double* __restrict__ means, const double* __restrict__ covs,
                                                                  const double* __restrict__ targets, int n, int num_samples,
                                                                  uint32_t seed_lo, uint32_t seed_hi, unsigned long long first_row_id,
                                                                  double* __restrict__ out, int* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * SCORE_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= n) return;                           // (whole waves leave: nothing below waits for another wave)
    double mu[4], g[4], S[4][4], L[4][4];
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        mu[k] = means[(size_t)row * 4 + k];
        g[k] = targets[(size_t)row * 4 + k];
        finite = finite && isfinite(mu[k]) && isfinite(g[k]);
#pragma unroll
        for (int j = 0; j <= k; ++j) {
            S[k][j] = covs[(size_t)row * 16 + k * 4 + j];
            finite = finite && isfinite(S[k][j]);
        }
    }
    int st = finite ? 0 : 2;
    double logdet = 0.0;
    if (st == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int j = 0; j < k; ++j) {
                double s = S[k][j];
#pragma unroll
                for (int p = 0; p < j; ++p) s -= L[k][p] * L[j][p];
                L[k][j] = s / L[j][j];
            }
            double d = S[k][k];
#pragma unroll
            for (int p = 0; p < k; ++p) d -= L[k][p] * L[k][p];
            if (!(d > 0.0) || !isfinite(d)) { st = 1; d = 1.0; }        // (d = 1 keeps the remaining arithmetic defined; the row is dropped)
            L[k][k] = sqrt(d);
            logdet += log(L[k][k]);
        }
    }
    double* o = out + (size_t)row * 8;
    if (st != 0) {                                  // uniform over the wave
        if (lane < 8) o[lane] = __builtin_nan("");
        if (lane == 0) status[row] = st;
        return;
    }
    logdet *= 2.0;
    // m2: forward substitution L y = g - mu
    double y[4], m2 = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double s = g[k] - mu[k];
#pragma unroll
        for (int p = 0; p < k; ++p) s -= L[k][p] * y[p];
        y[k] = s / L[k][k];
        m2 += y[k] * y[k];
    }
    // energy score
    const uint32_t r_lo = (uint32_t)(first_row_id + (unsigned long long)row);
    const uint32_t r_hi = (uint32_t)((first_row_id + (unsigned long long)row) >> 32);
    const int from = (lane + 63) & 63;
    double sum_a = 0.0, sum_b = 0.0;
    double zl[4] = {0.0, 0.0, 0.0, 0.0};            // this lane's sample of the trip before
    for (int base = 0; base < num_samples; base += 64) {     // uniform trip count: every lane takes part in the cross-lane reads
        const int i = base + lane;
        const Philox4 w = philox4x32_10((uint32_t)i, r_lo, BOD_SCORE_TAG, r_hi, seed_lo, seed_hi);
        const double r0 = sqrt(-2.0 * log(score_uniform(w.x))), r1 = sqrt(-2.0 * log(score_uniform(w.z)));
        double s0, c0, s1, c1;
        sincos(SCORE_TWO_PI * score_uniform(w.y), &s0, &c0);
        sincos(SCORE_TWO_PI * score_uniform(w.w), &s1, &c1);
        const double nn[4] = {r0 * c0, r0 * s0, r1 * c1, r1 * s1};
        double z[4], da = 0.0, db = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double s = mu[k];
#pragma unroll
            for (int p = 0; p <= k; ++p) s += L[k][p] * nn[p];
            z[k] = s;
            // sample i - 1: lane l - 1 of this trip, or (lane 0) lane 63 of the trip before
            const double zp = __shfl(lane == 63 ? zl[k] : s, from);
            const double ea = s - g[k], eb = s - zp;
            da += ea * ea;
            db += eb * eb;
        }
        if (i < num_samples) {
            sum_a += sqrt(da);
            if (i >= 1) sum_b += sqrt(db);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) zl[k] = z[k];
    }
    sum_a = wave_sum(sum_a);
    sum_b = wave_sum(sum_b);
    if (lane == 0) {
        o[0] = 0.5 * (4.0 * SCORE_LN_2PI + logdet + m2);
        o[1] = m2;
        o[2] = sum_a / (double)num_samples - sum_b / (2.0 * (double)(num_samples - 1));
#pragma unroll
        for (int k = 0; k < 4; ++k) o[3 + k] = 0.5 * erfc(-(g[k] - mu[k]) / sqrt(2.0 * S[k][k]));
        o[7] = logdet;
        status[row] = 0;
    }
}

#define SCORE_HIP(expr)                                                                                     \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess) return err.fail(BOD_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

}  // namespace

int score_pairs_run(long long n, const double* means, const double* covs, const double* targets, int num_samples, unsigned long long seed,
                    unsigned long long first_row_id, double* out, int32_t* status, hipStream_t s, char* errbuf, size_t errcap) {
    Err err{errbuf, errcap};
    if (n < 0) return err.fail(BOD_ERR_INVALID_ARG, "bod_score_pairs: negative row count %lld", n);
    if (num_samples < 2 || num_samples > 65536)
        return err.fail(BOD_ERR_INVALID_ARG, "bod_score_pairs: num_samples %d outside [2, 65536]", num_samples);
    if (n == 0) return BOD_OK;
    if (!means || !covs || !targets || !out || !status) return err.fail(BOD_ERR_INVALID_ARG, "bod_score_pairs: a required array is NULL");
    const int cap = (int)std::min<long long>(n, SCORE_BATCH_ROWS);
    DevArena arena;
    double *d_mu, *d_cov, *d_g, *d_out; int* d_st;
    SCORE_HIP(arena.alloc(&d_mu, (size_t)cap * 4)); SCORE_HIP(arena.alloc(&d_cov, (size_t)cap * 16));
    SCORE_HIP(arena.alloc(&d_g, (size_t)cap * 4)); SCORE_HIP(arena.alloc(&d_out, (size_t)cap * 8));
    SCORE_HIP(arena.alloc(&d_st, (size_t)cap));
    for (long long r0 = 0; r0 < n; r0 += cap) {
        const int m = (int)std::min<long long>(n - r0, cap);
        SCORE_HIP(hipMemcpyAsync(d_mu, means + r0 * 4, sizeof(double) * 4 * m, hipMemcpyHostToDevice, s));
        SCORE_HIP(hipMemcpyAsync(d_cov, covs + r0 * 16, sizeof(double) * 16 * m, hipMemcpyHostToDevice, s));
        SCORE_HIP(hipMemcpyAsync(d_g, targets + r0 * 4, sizeof(double) * 4 * m, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(score_pairs_kernel, dim3((m + SCORE_ROWS_PER_BLOCK - 1) / SCORE_ROWS_PER_BLOCK), dim3(SCORE_BLOCK), 0, s, d_mu, d_cov,
                           d_g, m, num_samples, (uint32_t)seed, (uint32_t)(seed >> 32), first_row_id + (unsigned long long)r0, d_out, d_st);
        SCORE_HIP(hipGetLastError());
        SCORE_HIP(hipMemcpyAsync(out + r0 * 8, d_out, sizeof(double) * 8 * m, hipMemcpyDeviceToHost, s));
        SCORE_HIP(hipMemcpyAsync(status + r0, d_st, sizeof(int32_t) * m, hipMemcpyDeviceToHost, s));
        SCORE_HIP(hipStreamSynchronize(s));       // (the pageable copies above are synchronous anyway; the next batch reuses the buffers)
    }
    return BOD_OK;
}

// PDQ (Probability-based Detection Quality) on the device: the corner heatmaps of probabilistic boxes and the per-pair
// log-losses of prob_detection_quality.py, rule by rule:
//
//   * corner_roi: five-sigma box (int() truncation), singular shortcut |det| < 1e-8, Mahalanobis radius as scipy's cdist
//     computes it (sqrt((d VI) d), VI = inv(cov), fp64), the shift rule for rows above / columns left of the mean's cell,
//     threshold <= 3.439, the mean's cell forced on, bounding box of the mask;            -> pdq_roi_kernel
//   * corner_heatmap: P(corner <= (y + 1 - 1e-14, x + 1 - 1e-14)) on the region in fp64 (Genz's bivariate-normal
//     algorithm, Statistics and Computing 14:251-260, 2004 -- what scipy's mvnun evaluates in 2-D), stored as float32,
//     continued constant below / right of the region (1 in the far quadrant), minus the float32 masses left of / above
//     the image and plus the fp64 cdf(-1e-14, -1e-14) (NumPy 2: a float32 array plus a float64 scalar is computed in
//     float64), floored at 0.0027;                                                         -> pdq_cdf_kernel, corner_value
//   * PBoxDetInst.calc_heatmap: top-left corner times the bottom-right corner's map of the image turned by 180 degrees,
//     float32 product clipped at 1 and floored at 0.0027;                                 -> pdq_rows_kernel
//   * pair_qualities / image_quality: fg_loss[g,d] = sum log(heat + 1e-14) over mask[y1:y2, x1:x2], bg_loss[g,d] = sum
//     log(1 - heat + 1e-14) [heat > 0] outside [y1:y2+1, x1:x2+1], det_bg_loss[d] = the same over the whole frame.
//     Rectangles follow NumPy slice semantics.  Each per-pixel argument is formed in float32 like NumPy does; the log is
//     taken in fp64 of that float32 argument and the sums are fp64.                       -> pdq_rows_kernel, pdq_reduce_kernel
//
// Determinism: no floating-point atomics.  Each (detection, row) block scans its row in a fixed order (inclusive prefix
// sums in LDS) and writes per-(row, ground truth) segment sums; one thread per (ground truth, detection) adds them over the
// rows in order.  Nothing depends on which other frames share a launch, so one call of N frames and N calls of one frame
// give the same bits.  The only atomics are integer min / max of the region bounds.
#include "../../include/bayesod.h"
#include "host_call.h"
#include "kernels.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <climits>
#include <vector>

namespace {

constexpr double PDQ_TINY = 1e-14;
constexpr double PDQ_ROI_RADIUS = 3.439;
// heat[heat < 0.0027] = 0 on a float32 array: NumPy 2 casts the Python float to float32 and compares in float32
constexpr float PDQ_FLOOR = 0.0027f;
constexpr int PDQ_BLOCK = 256;
constexpr int PDQ_MAX_W = 4000;                   // two fp64 prefix rows of W entries in LDS (64 000 bytes)
constexpr size_t PDQ_BATCH_BYTES = (size_t)1 << 30;   // device memory of one internal batch of frames (at least one frame)
constexpr int PDQ_BATCH_FRAMES = 256;

struct PdqCorner {
    double my, mx;          // mean (y, x)
    double sy, sx;          // standard deviations
    double r;               // correlation (mvnun: covar(2,1) / stdev(2) / stdev(1))
    double vi[4];           // inv(cov), row-major (y, x)
    int ay0, ax0, nh, nw;   // the five-sigma box [ay0, ay0 + nh) x [ax0, ax0 + nw) (the region itself when singular)
    int iy, ix;             // the mean's cell in that box
    int shift_y, shift_x;   // 0 < iy < h - 1 (resp. ix): rows above / columns left of the cell take the next one's distance
    int singular;
    int pad;
    long long map_off;      // CDF values [nh][nw], then left [nh], then above [nw] (float32) in the map buffer
};

struct PdqGt {              // one ground-truth box, resolved to half-open pixel ranges
    int fy0, fy1, fx0, fx1; // foreground mask[y1:y2, x1:x2]
    int by0, by1, bx0, bx1; // the box the background term leaves out, [y1:y2+1, x1:x2+1]
};

struct PdqDet {             // one detection of a batch
    int frame;              // frame index inside the batch
    int local;              // detection index inside its frame
};

struct PdqFrame {
    int gt_off, G;          // ground truths [gt_off, gt_off + G) of the batch
    int det_off, D;         // detections [det_off, det_off + D) of the batch
    long long row_off;      // per-(detection, row, ground truth) segment sums: row_off + ((d * H) + y) * G + g
    long long pair_off;     // fg / bg outputs of the frame: pair_off + g * D + d
};

// ---- Genz's bivariate normal upper probability P(X > h, Y > k), correlation r ----------------------------------------
// Gauss-Legendre abscissas (negative half) and weights for 6, 12 and 20 points.
__constant__ double GL_X[3][10] = {
    {-0.93246951420315205, -0.66120938646626448, -0.23861918608319693},
    {-0.98156063424671924, -0.9041172563704748, -0.76990267419430469, -0.58731795428661748, -0.36783149899818018,
     -0.12523340851146891},
    {-0.99312859918509488, -0.96397192727791381, -0.91223442825132584, -0.83911697182221878, -0.7463319064601508,
     -0.63605368072651502, -0.51086700195082713, -0.37370608871541955, -0.2277858511416451, -0.076526521133497338}};
__constant__ double GL_W[3][10] = {
    {0.17132449237916975, 0.36076157304813894, 0.46791393457269137},
    {0.047175336386512022, 0.10693932599531888, 0.16007832854334611, 0.20316742672306565, 0.23349253653835464,
     0.24914704581340269},
    {0.017614007139153273, 0.040601429800386217, 0.062672048334109443, 0.083276741576704671, 0.10193011981724026,
     0.11819453196151825, 0.13168863844917653, 0.14209610931838187, 0.14917298647260366, 0.15275338713072578}};

__device__ __forceinline__ double norm_cdf(double x) { return 0.5 * erfc(-x * 0.70710678118654752440); }

__device__ double bvn_upper(double h, double k, double r) {
    const double two_pi = 6.283185307179586;
    const double ar = fabs(r);
    const int ng = ar < 0.3 ? 0 : (ar < 0.75 ? 1 : 2);
    const int lg = ng == 0 ? 3 : (ng == 1 ? 6 : 10);
    double hk = h * k;
    double bvn = 0.0;
    if (ar < 0.925) {
        // Sheppard's formula: integrate d/dr of the probability from 0 to r in the substitution sin(theta) = r
        const double hs = (h * h + k * k) / 2;
        const double asr = asin(r);
        for (int i = 0; i < lg; ++i) {
            double sn = sin(asr * (GL_X[ng][i] + 1) / 2);
            bvn += GL_W[ng][i] * exp((sn * hk - hs) / (1 - sn * sn));
            sn = sin(asr * (-GL_X[ng][i] + 1) / 2);
            bvn += GL_W[ng][i] * exp((sn * hk - hs) / (1 - sn * sn));
        }
        return bvn * asr / (2 * two_pi) + norm_cdf(-h) * norm_cdf(-k);
    }
    // |r| near 1: integrate from r to +-1 after subtracting the singular part of the integrand (Drezner & Wesolowsky)
    if (r < 0) { k = -k; hk = -hk; }
    if (ar < 1) {
        const double as = (1 - r) * (1 + r);
        double a = sqrt(as);
        const double bs = (h - k) * (h - k);
        const double c = (4 - hk) / 8;
        const double d = (12 - hk) / 16;
        bvn = a * exp(-(bs / as + hk) / 2) * (1 - c * (bs - as) * (1 - d * bs / 5) / 3 + c * d * as * as / 5);
        if (hk > -160) {
            const double b = sqrt(bs);
            bvn -= exp(-hk / 2) * sqrt(two_pi) * norm_cdf(-b / a) * b * (1 - c * bs * (1 - d * bs / 5) / 3);
        }
        a = a / 2;
        for (int i = 0; i < lg; ++i) {
            double xs = (a * (GL_X[ng][i] + 1)) * (a * (GL_X[ng][i] + 1));
            double rs = sqrt(1 - xs);
            bvn += a * GL_W[ng][i] * (exp(-bs / (2 * xs) - hk / (1 + rs)) / rs - exp(-(bs / xs + hk) / 2) * (1 + c * xs * (1 + d * xs)));
            xs = as * (-GL_X[ng][i] + 1) * (-GL_X[ng][i] + 1) / 4;
            rs = sqrt(1 - xs);
            bvn += a * GL_W[ng][i] * exp(-(bs / xs + hk) / 2) * (exp(-hk * (1 - rs) / (2 * (1 + rs))) / rs - (1 + c * xs * (1 + d * xs)));
        }
        bvn = -bvn / two_pi;
    }
    if (r > 0) return bvn + norm_cdf(-fmax(h, k));
    bvn = -bvn;
    if (k > h) bvn += h < 0 ? norm_cdf(k) - norm_cdf(h) : norm_cdf(-h) - norm_cdf(-k);
    return bvn;
}

// P(corner_y <= uy, corner_x <= ux): mvnun standardises the limits, BVNU(-b1, -b2, r)
__device__ __forceinline__ double corner_cdf(const PdqCorner& c, double uy, double ux) {
    return bvn_upper(-((uy - c.my) / c.sy), -((ux - c.mx) / c.sx), c.r);
}

// ---- region of interest: bounding box of {Mahalanobis radius <= 3.439} (integer atomics: order-free) ------------------
__global__ __launch_bounds__(PDQ_BLOCK) void pdq_roi_kernel(const PdqCorner* __restrict__ corners, int n, int* __restrict__ rois) {
    const int ci = blockIdx.y;
    if (ci >= n) return;
    const PdqCorner c = corners[ci];
    __shared__ int red[4][PDQ_BLOCK];
    int lo_r = INT_MAX, lo_c = INT_MAX, hi_r = INT_MIN, hi_c = INT_MIN;
    if (!c.singular) {
        const long long total = (long long)c.nh * c.nw;
        for (long long p = (long long)blockIdx.x * PDQ_BLOCK + threadIdx.x; p < total; p += (long long)gridDim.x * PDQ_BLOCK) {
            const int r = (int)(p / c.nw), q = (int)(p % c.nw);
            const int rr = r + ((c.shift_y && r < c.iy) ? 1 : 0);
            const int qq = q + ((c.shift_x && q < c.ix) ? 1 : 0);
            const double d0 = (double)(c.ay0 + rr) - c.my, d1 = (double)(c.ax0 + qq) - c.mx;
            const double t0 = d0 * c.vi[0] + d1 * c.vi[2];
            const double t1 = d0 * c.vi[1] + d1 * c.vi[3];
            double s = 0.0;
            s += t0 * d0;
            s += t1 * d1;
            if (sqrt(s) <= PDQ_ROI_RADIUS || (r == c.iy && q == c.ix)) {
                lo_r = min(lo_r, r); hi_r = max(hi_r, r); lo_c = min(lo_c, q); hi_c = max(hi_c, q);
            }
        }
    }
    red[0][threadIdx.x] = lo_r; red[1][threadIdx.x] = lo_c; red[2][threadIdx.x] = hi_r; red[3][threadIdx.x] = hi_c;
    __syncthreads();
    for (int s = PDQ_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red[0][threadIdx.x] = min(red[0][threadIdx.x], red[0][threadIdx.x + s]);
            red[1][threadIdx.x] = min(red[1][threadIdx.x], red[1][threadIdx.x + s]);
            red[2][threadIdx.x] = max(red[2][threadIdx.x], red[2][threadIdx.x + s]);
            red[3][threadIdx.x] = max(red[3][threadIdx.x], red[3][threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && !c.singular && red[2][0] >= 0) {
        atomicMin(&rois[ci * 4 + 0], c.ax0 + red[1][0]);
        atomicMin(&rois[ci * 4 + 1], c.ay0 + red[0][0]);
        atomicMax(&rois[ci * 4 + 2], c.ax0 + red[3][0]);
        atomicMax(&rois[ci * 4 + 3], c.ay0 + red[2][0]);
    }
}

// ---- CDF on the region, plus the left column / top row / corner masses when the region touches the image's edge -------
// thread (r, q) of [-1, nh) x [-1, nw): r = -1 is the row above the image, q = -1 the column left of it
__global__ __launch_bounds__(PDQ_BLOCK) void pdq_cdf_kernel(const PdqCorner* __restrict__ corners, int n, const int* __restrict__ rois,
                                                           float* __restrict__ maps, double* __restrict__ cconst) {
    const int ci = blockIdx.y;
    if (ci >= n) return;
    const PdqCorner c = corners[ci];
    const int rx0 = rois[ci * 4 + 0], ry0 = rois[ci * 4 + 1], rx1 = rois[ci * 4 + 2], ry1 = rois[ci * 4 + 3];
    float* map = maps + c.map_off;
    float* left = map + (long long)c.nh * c.nw;
    float* above = left + c.nh;
    const long long total = (long long)(c.nh + 1) * (c.nw + 1);
    for (long long p = (long long)blockIdx.x * PDQ_BLOCK + threadIdx.x; p < total; p += (long long)gridDim.x * PDQ_BLOCK) {
        const int r = (int)(p / (c.nw + 1)) - 1, q = (int)(p % (c.nw + 1)) - 1;
        const int y = c.ay0 + r, x = c.ax0 + q;
        const bool in_y = y >= ry0 && y <= ry1, in_x = x >= rx0 && x <= rx1;
        const double uy = (double)(y + 1) - PDQ_TINY, ux = (double)(x + 1) - PDQ_TINY;
        if (r >= 0 && q >= 0) {
            if (in_y && in_x) map[(long long)r * c.nw + q] = (float)corner_cdf(c, uy, ux);
        } else if (r >= 0) {
            if (rx0 == 0 && in_y) left[r] = (float)corner_cdf(c, uy, 0.0 - PDQ_TINY);
        } else if (q >= 0) {
            if (ry0 == 0 && in_x) above[q] = (float)corner_cdf(c, 0.0 - PDQ_TINY, ux);
        } else if (rx0 == 0 && ry0 == 0) {
            cconst[ci] = corner_cdf(c, 0.0 - PDQ_TINY, 0.0 - PDQ_TINY);
        }
    }
}

// corner_heatmap's value at pixel (y, x) of the corner's own image
__device__ __forceinline__ float corner_value(const PdqCorner& c, const int* roi, const float* maps, double cc, int y, int x) {
    const int rx0 = roi[0], ry0 = roi[1], rx1 = roi[2], ry1 = roi[3];
    const float* map = maps + c.map_off;
    const float* left = map + (long long)c.nh * c.nw;
    const float* above = left + c.nh;
    float v;
    if (y < ry0 || x < rx0) v = 0.f;
    else if (y > ry1 && x > rx1) v = 1.f;
    else v = map[(long long)(min(y, ry1) - c.ay0) * c.nw + (min(x, rx1) - c.ax0)];
    if (rx0 == 0) v = v - (y < ry0 ? 0.f : left[min(y, ry1) - c.ay0]);
    if (ry0 == 0) v = v - (x < rx0 ? 0.f : above[min(x, rx1) - c.ax0]);
    if (rx0 == 0 && ry0 == 0) v = (float)((double)v + cc);
    return v < PDQ_FLOOR ? 0.f : v;
}

__global__ __launch_bounds__(PDQ_BLOCK) void pdq_expand_kernel(const PdqCorner* __restrict__ corners, int n, const int* __restrict__ rois,
                                                              const float* __restrict__ maps, const double* __restrict__ cconst,
                                                              int H, int W, float* __restrict__ out) {
    const int ci = blockIdx.y;
    if (ci >= n) return;
    const PdqCorner c = corners[ci];
    const double cc = cconst[ci];
    const long long total = (long long)H * W;
    for (long long p = (long long)blockIdx.x * PDQ_BLOCK + threadIdx.x; p < total; p += (long long)gridDim.x * PDQ_BLOCK)
        out[(long long)ci * total + p] = corner_value(c, rois + ci * 4, maps, cc, (int)(p / W), (int)(p % W));
}

// ---- one block per (detection, row): heat, the two loss terms per pixel, their row prefix sums, the segment sums ------
__device__ __forceinline__ double wave_inclusive_scan(double v) {
    const int lane = threadIdx.x & (warpSize - 1);
    for (int o = 1; o < warpSize; o <<= 1) {
        const double u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

__global__ __launch_bounds__(PDQ_BLOCK) void pdq_rows_kernel(const PdqCorner* __restrict__ corners, const int* __restrict__ rois,
                                                            const float* __restrict__ maps, const double* __restrict__ cconst,
                                                            const PdqDet* __restrict__ dets, const PdqFrame* __restrict__ frames,
                                                            const PdqGt* __restrict__ gts, int H, int W, double* __restrict__ seg,
                                                            double* __restrict__ rowtot, float* __restrict__ heat_out) {
    extern __shared__ double pre[];                 // inclusive prefix sums: fg terms [W], bg terms [W]
    __shared__ double wtot[2][PDQ_BLOCK / 64];
    __shared__ double carry[2];
    const int y = blockIdx.x, di = blockIdx.y;
    const PdqDet det = dets[di];
    const PdqFrame fr = frames[det.frame];
    const PdqCorner ctl = corners[2 * di], cbr = corners[2 * di + 1];
    const int* roi_tl = rois + 8 * di;
    const int* roi_br = roi_tl + 4;
    const double cc_tl = cconst[2 * di], cc_br = cconst[2 * di + 1];
    double* pf = pre;
    double* pb = pre + W;
    // heat == 0: log(float32(0 + 1e-14)) (NumPy forms heat + 1e-14 in float32; the log is taken here in fp64)
    const double f_zero = log((double)1e-14f);
    const int wave = threadIdx.x / warpSize, lane = threadIdx.x & (warpSize - 1);
    if (threadIdx.x == 0) { carry[0] = 0.0; carry[1] = 0.0; }
    for (int x0 = 0; x0 < W; x0 += PDQ_BLOCK) {
        const int x = x0 + threadIdx.x;
        double f = 0.0, b = 0.0;
        if (x < W) {
            const float p_tl = corner_value(ctl, roi_tl, maps, cc_tl, y, x);
            const float p_br = corner_value(cbr, roi_br, maps, cc_br, H - 1 - y, W - 1 - x);
            float h = p_tl * p_br;
            if (h > 1.f) h = 1.f;
            if (h < PDQ_FLOOR) h = 0.f;
            if (heat_out) heat_out[((long long)di * H + y) * W + x] = h;
            f = h == 0.f ? f_zero : log((double)(h + 1e-14f));
            b = h > 0.f ? log((double)((1.0f - h) + 1e-14f)) : 0.0;
        }
        f = wave_inclusive_scan(f);
        b = wave_inclusive_scan(b);
        if (lane == warpSize - 1) { wtot[0][wave] = f; wtot[1][wave] = b; }
        __syncthreads();
        double of = carry[0], ob = carry[1];
        for (int w = 0; w < wave; ++w) { of += wtot[0][w]; ob += wtot[1][w]; }
        f += of;
        b += ob;
        if (x < W) { pf[x] = f; pb[x] = b; }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int last = min(x0 + PDQ_BLOCK, W) - 1;
            carry[0] = pf[last]; carry[1] = pb[last];
        }
        __syncthreads();
    }
    // sum over [a, b) of a row = P(b) - P(a), P(e) = inclusive prefix through e - 1 (0 for e = 0)
    const double tot_b = pb[W - 1];
    const long long base = fr.row_off + ((long long)det.local * H + y) * fr.G;
    for (int g = threadIdx.x; g < fr.G; g += PDQ_BLOCK) {
        const PdqGt t = gts[fr.gt_off + g];
        double fg = 0.0, bg = tot_b;
        if (y >= t.fy0 && y < t.fy1 && t.fx1 > t.fx0)
            fg = pf[t.fx1 - 1] - (t.fx0 > 0 ? pf[t.fx0 - 1] : 0.0);
        if (y >= t.by0 && y < t.by1 && t.bx1 > t.bx0)
            bg = (t.bx0 > 0 ? pb[t.bx0 - 1] : 0.0) + (tot_b - pb[t.bx1 - 1]);
        seg[2 * (base + g)] = fg;
        seg[2 * (base + g) + 1] = bg;
    }
    if (threadIdx.x == 0) rowtot[(long long)di * H + y] = tot_b;
}

// ---- one thread per (ground truth, detection) of a frame: the rows' segment sums in row order ------------------------
__global__ __launch_bounds__(PDQ_BLOCK) void pdq_reduce_kernel(const PdqFrame* __restrict__ frames, const double* __restrict__ seg,
                                                              const double* __restrict__ rowtot, int H, double* __restrict__ fg_out,
                                                              double* __restrict__ bg_out, double* __restrict__ dbg_out) {
    const PdqFrame fr = frames[blockIdx.y];
    const int p = blockIdx.x * PDQ_BLOCK + threadIdx.x;
    if (p < fr.G * fr.D) {
        const int g = p / fr.D, d = p % fr.D;
        double fg = 0.0, bg = 0.0;
        for (int y = 0; y < H; ++y) {
            const long long i = fr.row_off + ((long long)d * H + y) * fr.G + g;
            fg += seg[2 * i];
            bg += seg[2 * i + 1];
        }
        fg_out[fr.pair_off + p] = fg;
        bg_out[fr.pair_off + p] = bg;
    }
    if (p < fr.D) {
        double s = 0.0;
        for (int y = 0; y < H; ++y) s += rowtot[(long long)(fr.det_off + p) * H + y];
        dbg_out[fr.det_off + p] = s;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------
#define PDQ_HIP(expr)                                                                                       \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess) return err.fail(BOD_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// int(v) of Python for v clamped to [lo, hi] beforehand (truncation toward zero)
inline long long py_int(double v) { return (long long)std::max(std::min(v, 4e15), -4e15); }

// corner_roi's host-side part: validation, five-sigma box, singular shortcut, the mean's cell, inv(cov).  cov = (y, x)
// order row-major.  roi_init receives the region of a singular corner, or the identities of min / max otherwise.
int setup_corner(int H, int W, double my, double mx, const double* cov, PdqCorner* out, int* roi_init, Err& err, long long idx) {
    const double c00 = cov[0], c01 = cov[1], c10 = cov[2], c11 = cov[3];
    if (!std::isfinite(my) || !std::isfinite(mx) || !std::isfinite(c00) || !std::isfinite(c01) || !std::isfinite(c10) || !std::isfinite(c11))
        return err.fail(BOD_ERR_INVALID_ARG, "pdq corner %lld: non-finite mean or covariance", idx);
    if (!(c00 > 0) || !(c11 > 0))
        return err.fail(BOD_ERR_INVALID_ARG, "pdq corner %lld: non-positive variance", idx);
    PdqCorner c{};
    c.my = my; c.mx = mx;
    c.sy = sqrt(c00); c.sx = sqrt(c11);
    c.r = c10 / c.sy / c.sx;
    if (!(fabs(c.r) <= 1) || !(fabs(c01 / c.sy / c.sx) <= 1))
        return err.fail(BOD_ERR_INVALID_ARG, "pdq corner %lld: covariance is not positive semi-definite (|correlation| > 1)", idx);
    const double fx0 = std::max(mx - 5 * c.sx, 0.0), fy0 = std::max(my - 5 * c.sy, 0.0);
    if (fx0 >= W || fy0 >= H)            // its region would start outside the image (the CPU path raises)
        return err.fail(BOD_ERR_INVALID_ARG, "pdq corner %lld: mean (%g, %g) lies outside the image's reach", idx, my, mx);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const long long x1 = py_int(std::min(mx + 5 * c.sx, (double)(W - 1))), y1 = py_int(std::min(my + 5 * c.sy, (double)(H - 1)));
    // np.linalg.det: LU with partial pivoting
    const double det = fabs(c00) >= fabs(c10) ? c00 * (c11 - (c10 / c00) * c01) : -(c10 * (c01 - (c00 / c10) * c11));
    c.singular = fabs(det) < 1e-8;
    if (c.singular) {
        const long long rx1 = std::max(0LL, x1), ry1 = std::max(0LL, y1);
        if (x0 > rx1 || y0 > ry1)
            return err.fail(BOD_ERR_INVALID_ARG, "pdq corner %lld: singular covariance with an empty region", idx);
        c.ay0 = y0; c.ax0 = x0; c.nh = (int)(ry1 + 1 - y0); c.nw = (int)(rx1 + 1 - x0);
        roi_init[0] = x0; roi_init[1] = y0; roi_init[2] = (int)rx1; roi_init[3] = (int)ry1;
    } else {
        c.ay0 = y0; c.ax0 = x0;
        c.nh = (int)std::max(y1 + 1 - y0, 1LL); c.nw = (int)std::max(x1 + 1 - x0, 1LL);
        auto cell = [](double t, int n) -> int {      // max(min(int(t), n - 1), 0)
            if (t >= n) return n - 1;
            if (t <= -1) return 0;
            return std::max(std::min((int)t, n - 1), 0);
        };
        c.iy = cell(my - y0, H); c.ix = cell(mx - x0, W);
        if (c.iy >= c.nh || c.ix >= c.nw)    // the CPU path raises (IndexError / ValueError)
            return err.fail(BOD_ERR_INVALID_ARG, "pdq corner %lld: mean (%g, %g) lies outside its approximate region", idx, my, mx);
        c.shift_y = c.iy > 0 && c.iy < H - 1;
        c.shift_x = c.ix > 0 && c.ix < W - 1;
        // inv(cov) (np.linalg.inv: LU with partial pivoting, then the two unit columns)
        double a = c00, b = c01, cc = c10, d = c11;
        const bool swap = fabs(cc) > fabs(a);
        if (swap) { std::swap(a, cc); std::swap(b, d); }
        const double l = cc / a, u = d - l * b;
        double e[2][2] = {{1, 0}, {0, 1}};
        if (swap) { e[0][0] = 0; e[0][1] = 1; e[1][0] = 1; e[1][1] = 0; }      // rows of the identity permuted
        for (int j = 0; j < 2; ++j) {
            const double y0v = e[0][j], y1v = e[1][j] - l * y0v;
            const double xb = y1v / u, xa = (y0v - b * xb) / a;
            c.vi[0 * 2 + j] = xa; c.vi[1 * 2 + j] = xb;
        }
        roi_init[0] = INT_MAX; roi_init[1] = INT_MAX; roi_init[2] = INT_MIN; roi_init[3] = INT_MIN;
    }
    *out = c;
    return BOD_OK;
}

inline size_t corner_bytes(const PdqCorner& c) { return ((size_t)c.nh * c.nw + c.nh + c.nw) * 4 + 64; }

int grid_for(long long work) { return (int)std::max(1LL, std::min((work + PDQ_BLOCK - 1) / PDQ_BLOCK, 2048LL)); }

// region + CDF launches for corners [0, n) of a batch already on the device
int launch_corners(const PdqCorner* h_corners, int n, PdqCorner* d_corners, int* d_rois, float* d_maps, double* d_cc,
                   hipStream_t s, Err& err) {
    long long work_roi = 0, work_cdf = 0;
    for (int i = 0; i < n; ++i) {
        if (!h_corners[i].singular) work_roi = std::max(work_roi, (long long)h_corners[i].nh * h_corners[i].nw);
        work_cdf = std::max(work_cdf, (long long)(h_corners[i].nh + 1) * (h_corners[i].nw + 1));
    }
    for (int c0 = 0; c0 < n; c0 += 65535) {
        const int m = std::min(n - c0, 65535);
        if (work_roi > 0) {
            hipLaunchKernelGGL(pdq_roi_kernel, dim3(grid_for(work_roi), m), dim3(PDQ_BLOCK), 0, s, d_corners + c0, m, d_rois + 4 * c0);
            PDQ_HIP(hipGetLastError());
        }
    }
    for (int c0 = 0; c0 < n; c0 += 65535) {
        const int m = std::min(n - c0, 65535);
        hipLaunchKernelGGL(pdq_cdf_kernel, dim3(grid_for(work_cdf), m), dim3(PDQ_BLOCK), 0, s, d_corners + c0, m, d_rois + 4 * c0, d_maps,
                           d_cc + c0);
        PDQ_HIP(hipGetLastError());
    }
    return BOD_OK;
}

bool trace_on() {
    const char* t = getenv("BOD_PDQ_TRACE");
    return t && atoi(t) != 0;
}

}  // namespace

int pdq_corner_heatmaps_run(int H, int W, int n, const double* means_yx, const double* covs_yx, int32_t* rois, float* heatmaps,
                            hipStream_t s, char* errbuf, size_t errcap) {
    Err err{errbuf, errcap};
    if (H < 1 || W < 1 || n < 0 || (n > 0 && (!means_yx || !covs_yx)))
        return err.fail(BOD_ERR_INVALID_ARG, "bod_pdq_corner_heatmaps: bad argument");
    std::vector<PdqCorner> corners((size_t)n);
    std::vector<int> roi_init((size_t)n * 4);
    for (int i = 0; i < n; ++i) {
        const int st = setup_corner(H, W, means_yx[2 * i], means_yx[2 * i + 1], covs_yx + 4 * i, &corners[i], &roi_init[4 * i], err, i);
        if (st != BOD_OK) return st;
    }
    const size_t per_map = heatmaps ? (size_t)H * W * 4 : 0;
    int c0 = 0;
    while (c0 < n) {
        // a batch of corners within the memory budget (at least one)
        size_t bytes = 0, maps = 0;
        int c1 = c0;
        while (c1 < n && (c1 == c0 || bytes + corner_bytes(corners[c1]) + per_map <= PDQ_BATCH_BYTES) && c1 - c0 < 4096) {
            corners[c1].map_off = (long long)maps;
            maps += (size_t)corners[c1].nh * corners[c1].nw + corners[c1].nh + corners[c1].nw;
            bytes += corner_bytes(corners[c1]) + per_map;
            ++c1;
        }
        const int m = c1 - c0;
        DevArena arena;
        PdqCorner* d_corners; int* d_rois; float* d_maps; double* d_cc; float* d_heat = nullptr;
        PDQ_HIP(arena.alloc(&d_corners, m)); PDQ_HIP(arena.alloc(&d_rois, (size_t)4 * m));
        PDQ_HIP(arena.alloc(&d_maps, maps)); PDQ_HIP(arena.alloc(&d_cc, m));
        if (heatmaps) PDQ_HIP(arena.alloc(&d_heat, (size_t)m * H * W));
        PDQ_HIP(hipMemcpyAsync(d_corners, corners.data() + c0, sizeof(PdqCorner) * m, hipMemcpyHostToDevice, s));
        PDQ_HIP(hipMemcpyAsync(d_rois, roi_init.data() + 4 * c0, sizeof(int) * 4 * m, hipMemcpyHostToDevice, s));
        PDQ_HIP(hipMemsetAsync(d_cc, 0, sizeof(double) * m, s));
        int st = launch_corners(corners.data() + c0, m, d_corners, d_rois, d_maps, d_cc, s, err);
        if (st != BOD_OK) return st;
        if (heatmaps) {
            for (int k = 0; k < m; k += 65535) {
                const int mm = std::min(m - k, 65535);
                hipLaunchKernelGGL(pdq_expand_kernel, dim3(grid_for((long long)H * W), mm), dim3(PDQ_BLOCK), 0, s, d_corners + k, mm,
                                   d_rois + 4 * k, d_maps, d_cc + k, H, W, d_heat + (size_t)k * H * W);
                PDQ_HIP(hipGetLastError());
            }
            PDQ_HIP(hipMemcpyAsync(heatmaps + (size_t)c0 * H * W, d_heat, (size_t)m * H * W * 4, hipMemcpyDeviceToHost, s));
        }
        if (rois) PDQ_HIP(hipMemcpyAsync(rois + 4 * c0, d_rois, sizeof(int) * 4 * m, hipMemcpyDeviceToHost, s));
        PDQ_HIP(hipStreamSynchronize(s));
        c0 = c1;
    }
    return BOD_OK;
}

int pdq_frames_run(int H, int W, int F, const int32_t* num_gt, const int32_t* gt_boxes, const int32_t* num_det, const int32_t* det_boxes,
                   const double* det_corner_covs, double* fg_loss, double* bg_loss, double* det_bg_loss, float* heatmaps, hipStream_t s,
                   char* errbuf, size_t errcap) {
    Err err{errbuf, errcap};
    if (H < 1 || W < 1 || F < 0 || (F > 0 && (!num_gt || !num_det)))
        return err.fail(BOD_ERR_INVALID_ARG, "bod_pdq_frames: bad argument");
    if (W > PDQ_MAX_W) return err.fail(BOD_ERR_INVALID_ARG, "bod_pdq_frames: image width %d above %d", W, PDQ_MAX_W);
    long long sum_g = 0, sum_d = 0, sum_pairs = 0;
    for (int f = 0; f < F; ++f) {
        if (num_gt[f] < 0 || num_det[f] < 0) return err.fail(BOD_ERR_INVALID_ARG, "bod_pdq_frames: negative count in frame %d", f);
        sum_g += num_gt[f]; sum_d += num_det[f]; sum_pairs += (long long)num_gt[f] * num_det[f];
    }
    if ((sum_g && !gt_boxes) || (sum_d && (!det_boxes || !det_corner_covs || !det_bg_loss)) || (sum_pairs && (!fg_loss || !bg_loss)))
        return err.fail(BOD_ERR_INVALID_ARG, "bod_pdq_frames: a required array is NULL");
    // corners of every detection (validated before anything runs): top-left = (y1, x1) with covs[0] in (y, x) order; the
    // bottom-right corner lives on the image turned by 180 degrees: mean (h - (y2 + 1), w - (x2 + 1)), cov flip(covs[1]).T
    std::vector<PdqCorner> corners((size_t)(2 * sum_d));
    std::vector<int> roi_init((size_t)(8 * sum_d));
    for (long long d = 0; d < sum_d; ++d) {
        const int32_t* b = det_boxes + 4 * d;
        const double* cv = det_corner_covs + 8 * d;              // [2][2][2], (x, y) order
        const double tl[4] = {cv[3], cv[2], cv[1], cv[0]};       // flipud(fliplr(c))
        const double br[4] = {cv[7], cv[5], cv[6], cv[4]};       // flipud(fliplr(c)).T
        int st = setup_corner(H, W, (double)b[1], (double)b[0], tl, &corners[2 * d], &roi_init[8 * d], err, 2 * d);
        if (st != BOD_OK) return st;
        st = setup_corner(H, W, (double)H - ((double)b[3] + 1), (double)W - ((double)b[2] + 1), br, &corners[2 * d + 1], &roi_init[8 * d + 4],
                          err, 2 * d + 1);
        if (st != BOD_OK) return st;
    }
    // ground-truth rectangles with NumPy slice semantics
    auto norm = [](long long v, int n) -> int {
        if (v < 0) v += n;
        return (int)std::max(0LL, std::min(v, (long long)n));
    };
    std::vector<PdqGt> gts((size_t)sum_g);
    for (long long g = 0; g < sum_g; ++g) {
        const int32_t* b = gt_boxes + 4 * g;
        PdqGt t;
        t.fy0 = norm(b[1], H); t.fy1 = norm(b[3], H); t.fx0 = norm(b[0], W); t.fx1 = norm(b[2], W);
        t.by0 = norm(b[1], H); t.by1 = norm((long long)b[3] + 1, H); t.bx0 = norm(b[0], W); t.bx1 = norm((long long)b[2] + 1, W);
        gts[g] = t;
    }
    const bool trace = trace_on();
    double trace_ms[4] = {0, 0, 0, 0};
    int f0 = 0;
    long long g_base = 0, d_base = 0, pair_base = 0;
    while (f0 < F) {
        // frames [f0, f1) within the memory budget (at least one)
        size_t bytes = 0, maps = 0;
        long long seg_n = 0, nd = 0, ng = 0, npairs = 0;
        int f1 = f0;
        std::vector<PdqFrame> frames;
        std::vector<PdqDet> dets;
        while (f1 < F && (int)frames.size() < PDQ_BATCH_FRAMES) {
            const int G = num_gt[f1], D = num_det[f1];
            size_t fb = (size_t)D * H * G * 16 + (size_t)D * H * 8 + (heatmaps ? (size_t)D * H * W * 4 : 0);
            for (int k = 0; k < 2 * D; ++k) fb += corner_bytes(corners[2 * (d_base + nd) + k]);
            if (f1 > f0 && bytes + fb > PDQ_BATCH_BYTES) break;
            PdqFrame fr;
            fr.gt_off = (int)ng; fr.G = G; fr.det_off = (int)nd; fr.D = D; fr.row_off = seg_n; fr.pair_off = npairs;
            frames.push_back(fr);
            for (int k = 0; k < D; ++k) dets.push_back(PdqDet{(int)frames.size() - 1, k});
            for (int k = 0; k < 2 * D; ++k) {
                PdqCorner& c = corners[2 * (d_base + nd) + k];
                c.map_off = (long long)maps;
                maps += (size_t)c.nh * c.nw + c.nh + c.nw;
            }
            seg_n += (long long)D * H * G; nd += D; ng += G; npairs += (long long)G * D;
            bytes += fb;
            ++f1;
        }
        const int nb = (int)frames.size();
        if (nd > 0) {
            DevArena arena;
            PdqCorner* d_corners; int* d_rois; float* d_maps; double* d_cc; PdqDet* d_dets; PdqFrame* d_frames; PdqGt* d_gts;
            double *d_seg, *d_rowtot, *d_fg, *d_bg, *d_dbg; float* d_heat = nullptr;
            PDQ_HIP(arena.alloc(&d_corners, (size_t)2 * nd)); PDQ_HIP(arena.alloc(&d_rois, (size_t)8 * nd));
            PDQ_HIP(arena.alloc(&d_maps, maps)); PDQ_HIP(arena.alloc(&d_cc, (size_t)2 * nd));
            PDQ_HIP(arena.alloc(&d_dets, (size_t)nd)); PDQ_HIP(arena.alloc(&d_frames, (size_t)nb)); PDQ_HIP(arena.alloc(&d_gts, (size_t)ng));
            PDQ_HIP(arena.alloc(&d_seg, (size_t)2 * seg_n)); PDQ_HIP(arena.alloc(&d_rowtot, (size_t)nd * H));
            PDQ_HIP(arena.alloc(&d_fg, (size_t)npairs)); PDQ_HIP(arena.alloc(&d_bg, (size_t)npairs)); PDQ_HIP(arena.alloc(&d_dbg, (size_t)nd));
            if (heatmaps) PDQ_HIP(arena.alloc(&d_heat, (size_t)nd * H * W));
            PDQ_HIP(hipMemcpyAsync(d_corners, corners.data() + 2 * d_base, sizeof(PdqCorner) * 2 * nd, hipMemcpyHostToDevice, s));
            PDQ_HIP(hipMemcpyAsync(d_rois, roi_init.data() + 8 * d_base, sizeof(int) * 8 * nd, hipMemcpyHostToDevice, s));
            PDQ_HIP(hipMemsetAsync(d_cc, 0, sizeof(double) * 2 * nd, s));
            PDQ_HIP(hipMemcpyAsync(d_dets, dets.data(), sizeof(PdqDet) * nd, hipMemcpyHostToDevice, s));
            PDQ_HIP(hipMemcpyAsync(d_frames, frames.data(), sizeof(PdqFrame) * nb, hipMemcpyHostToDevice, s));
            if (ng) PDQ_HIP(hipMemcpyAsync(d_gts, gts.data() + g_base, sizeof(PdqGt) * ng, hipMemcpyHostToDevice, s));
            hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
            if (trace) { for (auto& e : ev) PDQ_HIP(hipEventCreate(&e)); PDQ_HIP(hipEventRecord(ev[0], s)); }
            int st = launch_corners(corners.data() + 2 * d_base, (int)(2 * nd), d_corners, d_rois, d_maps, d_cc, s, err);
            if (st != BOD_OK) return st;
            if (trace) PDQ_HIP(hipEventRecord(ev[1], s));
            if (trace) PDQ_HIP(hipEventRecord(ev[2], s));
            for (long long k = 0; k < nd; k += 65535) {
                const int m = (int)std::min(nd - k, 65535LL);
                hipLaunchKernelGGL(pdq_rows_kernel, dim3(H, m), dim3(PDQ_BLOCK), (size_t)2 * W * sizeof(double), s, d_corners + 2 * k, d_rois + 8 * k,
                                   d_maps, d_cc + 2 * k, d_dets + k, d_frames, d_gts, H, W, d_seg, d_rowtot + k * H,
                                   d_heat ? d_heat + (size_t)k * H * W : nullptr);
                PDQ_HIP(hipGetLastError());
            }
            if (trace) PDQ_HIP(hipEventRecord(ev[3], s));
            int max_pairs = 1;
            for (const auto& fr : frames) max_pairs = std::max(max_pairs, std::max(fr.G * fr.D, fr.D));
            hipLaunchKernelGGL(pdq_reduce_kernel, dim3((max_pairs + PDQ_BLOCK - 1) / PDQ_BLOCK, nb), dim3(PDQ_BLOCK), 0, s, d_frames, d_seg, d_rowtot, H,
                               d_fg, d_bg, d_dbg);
            PDQ_HIP(hipGetLastError());
            if (trace) PDQ_HIP(hipEventRecord(ev[4], s));
            if (npairs) {
                PDQ_HIP(hipMemcpyAsync(fg_loss + pair_base, d_fg, sizeof(double) * npairs, hipMemcpyDeviceToHost, s));
                PDQ_HIP(hipMemcpyAsync(bg_loss + pair_base, d_bg, sizeof(double) * npairs, hipMemcpyDeviceToHost, s));
            }
            PDQ_HIP(hipMemcpyAsync(det_bg_loss + d_base, d_dbg, sizeof(double) * nd, hipMemcpyDeviceToHost, s));
            if (heatmaps) PDQ_HIP(hipMemcpyAsync(heatmaps + (size_t)d_base * H * W, d_heat, sizeof(float) * nd * H * W, hipMemcpyDeviceToHost, s));
            PDQ_HIP(hipStreamSynchronize(s));
            if (trace) {
                for (int k = 0; k < 3; ++k) {
                    float ms = 0.f;
                    PDQ_HIP(hipEventElapsedTime(&ms, ev[k == 0 ? 0 : k + 1], ev[k == 0 ? 1 : k + 2]));
                    trace_ms[k] += ms;
                }
                for (auto& e : ev) hipEventDestroy(e);
            }
        }
        f0 = f1; g_base += ng; d_base += nd; pair_base += npairs;
    }
    if (trace)
        fprintf(stderr, "# pdq_frames %d frames %dx%d: device ms regions+cdf %.4f rows %.4f reduce %.4f\n", F, H, W, trace_ms[0], trace_ms[1],
                trace_ms[2]);
    return BOD_OK;
}

// The box heatmaps of pdq_frames_run alone, left on the device, for the rendering stage's HEAT view (render_kernels.hip): rows
// [0, nd) of one frame's detections (corner covariances as float32, widened exactly) -> d_heat [nd][H][W], made by the same
// setup_corner / launch_corners / pdq_rows_kernel as bod_pdq_frames' heatmaps (a frame without ground truths).  d_heat == NULL only
// validates.  On a refused row *bad_row names it.  Synchronises the stream before its scratch is freed.
int pdq_box_heatmaps_device(int H, int W, int nd, const int32_t* det_boxes, const float* det_corner_covs, float* d_heat, int* bad_row,
                            hipStream_t s, char* errbuf, size_t errcap) {
    Err err{errbuf, errcap};
    *bad_row = -1;
    if (H < 1 || W < 1 || nd < 0 || nd > 32767 || (nd > 0 && (!det_boxes || !det_corner_covs)))
        return err.fail(BOD_ERR_INVALID_ARG, "bad argument");
    if (W > PDQ_MAX_W) return err.fail(BOD_ERR_INVALID_ARG, "image width %d above %d", W, PDQ_MAX_W);
    if (nd == 0) return BOD_OK;
    std::vector<PdqCorner> corners((size_t)(2 * nd));
    std::vector<int> roi_init((size_t)(8 * nd));
    std::vector<PdqDet> dets((size_t)nd);
    size_t maps = 0;
    for (int d = 0; d < nd; ++d) {
        const int32_t* b = det_boxes + 4 * d;
        const float* cv = det_corner_covs + 8 * d;               // [2][2][2], (x, y) order: as pdq_frames_run
        const double tl[4] = {cv[3], cv[2], cv[1], cv[0]};
        const double br[4] = {cv[7], cv[5], cv[6], cv[4]};
        *bad_row = d;
        int st = setup_corner(H, W, (double)b[1], (double)b[0], tl, &corners[2 * d], &roi_init[8 * d], err, 2 * d);
        if (st != BOD_OK) return st;
        st = setup_corner(H, W, (double)H - ((double)b[3] + 1), (double)W - ((double)b[2] + 1), br, &corners[2 * d + 1], &roi_init[8 * d + 4],
                          err, 2 * d + 1);
        if (st != BOD_OK) return st;
        for (int k = 0; k < 2; ++k) {
            PdqCorner& c = corners[2 * d + k];
            c.map_off = (long long)maps;
            maps += (size_t)c.nh * c.nw + c.nh + c.nw;
        }
        dets[d] = PdqDet{0, d};
    }
    *bad_row = -1;
    if (!d_heat) return BOD_OK;
    const PdqFrame frame{0, 0, 0, nd, 0, 0};
    DevArena arena;
    PdqCorner* d_corners; int* d_rois; float* d_maps; double* d_cc; PdqDet* d_dets; PdqFrame* d_frames; PdqGt* d_gts;
    double *d_seg, *d_rowtot;
    PDQ_HIP(arena.alloc(&d_corners, (size_t)2 * nd)); PDQ_HIP(arena.alloc(&d_rois, (size_t)8 * nd));
    PDQ_HIP(arena.alloc(&d_maps, maps)); PDQ_HIP(arena.alloc(&d_cc, (size_t)2 * nd));
    PDQ_HIP(arena.alloc(&d_dets, (size_t)nd)); PDQ_HIP(arena.alloc(&d_frames, 1)); PDQ_HIP(arena.alloc(&d_gts, 1));
    PDQ_HIP(arena.alloc(&d_seg, 2)); PDQ_HIP(arena.alloc(&d_rowtot, (size_t)nd * H));
    PDQ_HIP(hipMemcpyAsync(d_corners, corners.data(), sizeof(PdqCorner) * 2 * nd, hipMemcpyHostToDevice, s));
    PDQ_HIP(hipMemcpyAsync(d_rois, roi_init.data(), sizeof(int) * 8 * nd, hipMemcpyHostToDevice, s));
    PDQ_HIP(hipMemsetAsync(d_cc, 0, sizeof(double) * 2 * nd, s));
    PDQ_HIP(hipMemcpyAsync(d_dets, dets.data(), sizeof(PdqDet) * nd, hipMemcpyHostToDevice, s));
    PDQ_HIP(hipMemcpyAsync(d_frames, &frame, sizeof(PdqFrame), hipMemcpyHostToDevice, s));
    int st = launch_corners(corners.data(), 2 * nd, d_corners, d_rois, d_maps, d_cc, s, err);
    if (st == BOD_OK) {
        hipLaunchKernelGGL(pdq_rows_kernel, dim3(H, nd), dim3(PDQ_BLOCK), (size_t)2 * W * sizeof(double), s, d_corners, d_rois, d_maps, d_cc,
                           d_dets, d_frames, d_gts, H, W, d_seg, d_rowtot, d_heat);
        if (hipGetLastError() != hipSuccess) st = err.fail(BOD_ERR_HIP, "the heatmap launch failed");
    }
    if (hipStreamSynchronize(s) != hipSuccess && st == BOD_OK) st = err.fail(BOD_ERR_HIP, "the heatmap kernels failed");
    return st;
}

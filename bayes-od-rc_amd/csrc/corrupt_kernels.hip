// Frame corruptions on the device (the ops and the random-number contract: include/bayesod.h).  A chain of 1..4 ops
// per frame runs slot by slot over the packed uint8 RGB frames, ping-ponging between the staging buffer and one scratch of the same
// size.  In one slot every frame is covered by exactly one kernel: each kind present in the slot is launched once over the whole
// batch with the workgroups of the batch's largest frame, and a workgroup whose frame runs another kind there leaves at once (its
// record is wave-uniform).  BOD_CORRUPT_NONE is the copy.
// Every op but GAUSSIAN_NOISE is integer arithmetic or fp32 with a fixed operation order (__fmul_rn / __fadd_rn / __fsub_rn, and the
// file is built with -ffp-contract=off): tests/corruption_reference.py restates them in NumPy and the results are equal.
// All addressing comes from the host-built records (frame offsets and sizes, validated table indices): no address depends on a
// pixel value.
#include "../../include/bayesod.h"
#include "host_call.h"
#include "jpeg_dct.h"
#include "kernels.h"
#include "philox.h"

#include <math.h>
#include <string.h>

namespace {

constexpr int POINT_THREADS = 256;                // one thread per 4 consecutive pixels of the frame (12 bytes)
constexpr int SUM_GROUPS = 16;                    // CONTRAST's sums: 4-pixel groups per thread
constexpr int CONV_TILE = 32;                     // output pixels per side of a CONV2D workgroup's tile
constexpr int CONV_KMAX = 25;
constexpr int CONV_TW = CONV_TILE + CONV_KMAX - 1;
constexpr int PIX_TILE = 64;                      // a PIXELATE workgroup covers (64 / f)^2 blocks: a tile of (64 / f) * f <= 64 pixels per side
constexpr int JPEG_THREADS = 256;                 // 8 lanes per 8x8 block (lane t: row t, then column t): 32 blocks per workgroup
constexpr int JPEG_PITCH = 9;

struct CorruptFrame {                             // 48 B: one frame's op of one slot
    int64_t offset;                               // first byte of the frame in the packed buffer
    int32_t h, w;
    uint32_t frame_id;
    int32_t kind;
    float f0;
    uint32_t u0;
    int32_t tap_offset, ksize, table, pad;
};
static_assert(sizeof(CorruptFrame) == 48, "CorruptFrame layout");

struct CorruptArgs {
    const CorruptFrame* frames;                   // [n], this slot's
    const uint8_t* src;
    uint8_t* dst;
    const uint16_t* taps;
    const uint8_t* luts;
    const uint16_t* qtables;
    unsigned long long* sums;                     // [n][3], this slot's: CONTRAST's per-channel sums
    uint32_t seed_lo, seed_hi, slot;
    int32_t n, wgs_per_frame;
};

// 4 consecutive pixels (npx of them inside the frame) as 12 bytes
__device__ __forceinline__ void load_group(const uint8_t* p, int npx, uint8_t px[12]) {
    if (npx == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        const uint32_t* p32 = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const uint32_t v = p32[j];
#pragma unroll
            for (int k = 0; k < 4; ++k) px[4 * j + k] = (uint8_t)(v >> (8 * k));
        }
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) px[j] = j < 3 * npx ? p[j] : (uint8_t)0;
    }
}
__device__ __forceinline__ void store_group(uint8_t* p, int npx, const uint8_t px[12]) {
    if (npx == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        uint32_t* p32 = reinterpret_cast<uint32_t*>(p);
#pragma unroll
        for (int j = 0; j < 3; ++j)
            p32[j] = (uint32_t)px[4 * j] | (uint32_t)px[4 * j + 1] << 8 | (uint32_t)px[4 * j + 2] << 16 | (uint32_t)px[4 * j + 3] << 24;
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j)
            if (j < 3 * npx) p[j] = px[j];
    }
}

__device__ __forceinline__ uint8_t round_level(float v) { return (uint8_t)(int)rintf(fminf(fmaxf(v, 0.0f), 255.0f)); }
__device__ __forceinline__ float unit_open(uint32_t t) { return ((float)(t >> 9) + 0.5f) * 1.1920928955078125e-07f; }    // exact in fp32

// CONTRAST, pass A: per-frame per-channel integer sums (order-independent: partial sums + integer atomics).  A thread adds up
// SUM_GROUPS groups, a workgroup issues one atomic per channel: same-address atomics serialise, so there must be few of them.
__global__ __launch_bounds__(POINT_THREADS) void corrupt_sum_kernel(CorruptArgs a) {
    __shared__ uint32_t part[POINT_THREADS / 64][3];
    const int f = blockIdx.x / a.wgs_per_frame;
    const CorruptFrame& fr = a.frames[f];
    if (fr.kind != BOD_CORRUPT_CONTRAST) return;
    const uint32_t npix = (uint32_t)fr.h * (uint32_t)fr.w;
    const uint32_t g0 = (uint32_t)(blockIdx.x % a.wgs_per_frame) * (SUM_GROUPS * POINT_THREADS) + threadIdx.x;
    uint32_t s[3] = {0, 0, 0};                    // (at most 16 * 4 * 255 per thread, 2^22 per workgroup)
    for (int it = 0; it < SUM_GROUPS; ++it) {
        const uint32_t g = g0 + (uint32_t)it * POINT_THREADS;
        if ((uint64_t)g * 4 >= npix) break;
        const int npx = (int)min(4u, npix - g * 4);
        uint8_t px[12];
        load_group(a.src + fr.offset + (int64_t)g * 12, npx, px);
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) s[c] += px[3 * k + c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s[c] += __shfl_down(s[c], d);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) part[threadIdx.x >> 6][c] = s[c];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < POINT_THREADS / 64; ++w) t += part[w][threadIdx.x];
        if (t) atomicAdd(a.sums + (size_t)f * 3 + threadIdx.x, (unsigned long long)t);
    }
}

// The pointwise ops: NONE (copy), LUT, CONTRAST (pass B), IMPULSE_NOISE, GAUSSIAN_NOISE, FOG
template <int KIND>
__global__ __launch_bounds__(POINT_THREADS) void corrupt_point_kernel(CorruptArgs a) {
    const int f = blockIdx.x / a.wgs_per_frame;                                 // (grid = n * wgs_per_frame: inside the table)
    const CorruptFrame& fr = a.frames[f];
    if (fr.kind != KIND) return;
    const uint32_t W = (uint32_t)fr.w, npix = (uint32_t)fr.h * W;               // (h * w <= 2^30: corrupt_prepare)
    const uint32_t g = (uint32_t)(blockIdx.x % a.wgs_per_frame) * POINT_THREADS + threadIdx.x;
    if ((uint64_t)g * 4 >= npix) return;
    const int npx = (int)min(4u, npix - g * 4);
    uint8_t px[12];
    load_group(a.src + fr.offset + (int64_t)g * 12, npx, px);
    uint32_t xs[4], ys[4];
    xs[0] = (g * 4) % W; ys[0] = (g * 4) / W;
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        xs[k] = xs[k - 1] + 1; ys[k] = ys[k - 1];
        if (xs[k] == W) { xs[k] = 0; ++ys[k]; }
    }
    const uint32_t tag = BOD_CORRUPT_TAG | a.slot;
    if constexpr (KIND == BOD_CORRUPT_LUT) {
        const uint8_t* lut = a.luts + (size_t)fr.table * 768;
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) px[3 * k + c] = lut[c * 256 + px[3 * k + c]];
    } else if constexpr (KIND == BOD_CORRUPT_CONTRAST) {
        float m[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) m[c] = (float)((double)a.sums[(size_t)f * 3 + c] / (double)npix);
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                px[3 * k + c] = round_level(__fadd_rn(__fmul_rn(__fsub_rn((float)px[3 * k + c], m[c]), fr.f0), m[c]));
    } else if constexpr (KIND == BOD_CORRUPT_IMPULSE_NOISE) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const Philox4 r = philox4x32_10(xs[k], ys[k], tag, fr.frame_id, a.seed_lo, a.seed_hi);
            const uint32_t wd[3] = {r.x, r.y, r.z};
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (wd[c] < fr.u0) px[3 * k + c] = (wd[c] & 1u) ? (uint8_t)255 : (uint8_t)0;
        }
    } else if constexpr (KIND == BOD_CORRUPT_GAUSSIAN_NOISE) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const Philox4 r = philox4x32_10(xs[k], ys[k], tag, fr.frame_id, a.seed_lo, a.seed_hi);
            const float r0 = sqrtf(__fmul_rn(-2.0f, logf(unit_open(r.x)))), t0 = __fmul_rn(6.2831855f, unit_open(r.y));
            const float r1 = sqrtf(__fmul_rn(-2.0f, logf(unit_open(r.z)))), t1 = __fmul_rn(6.2831855f, unit_open(r.w));
            const float nn[3] = {__fmul_rn(r0, cosf(t0)), __fmul_rn(r0, sinf(t0)), __fmul_rn(r1, cosf(t1))};
#pragma unroll
            for (int c = 0; c < 3; ++c) px[3 * k + c] = round_level(__fadd_rn((float)px[3 * k + c], __fmul_rn(fr.f0, nn[c])));
        }
    } else if constexpr (KIND == BOD_CORRUPT_FOG) {
        uint32_t F[4] = {0, 0, 0, 0};
#pragma unroll 1
        for (int s = 7; s >= 2; --s) {
            const uint32_t S = 1u << s, c2 = tag | ((uint32_t)s << 4);
            uint32_t lix = 0xFFFFFFFFu, liy = 0xFFFFFFFFu, v00 = 0, v01 = 0, v10 = 0, v11 = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t ix = xs[k] >> s, iy = ys[k] >> s, fx = xs[k] & (S - 1), fy = ys[k] & (S - 1);
                if (ix != lix || iy != liy) {                                   // (the 4 pixels of a group mostly share their cell)
                    v00 = philox4x32_10(ix, iy, c2, fr.frame_id, a.seed_lo, a.seed_hi).x >> 16;
                    v01 = philox4x32_10(ix + 1, iy, c2, fr.frame_id, a.seed_lo, a.seed_hi).x >> 16;
                    v10 = philox4x32_10(ix, iy + 1, c2, fr.frame_id, a.seed_lo, a.seed_hi).x >> 16;
                    v11 = philox4x32_10(ix + 1, iy + 1, c2, fr.frame_id, a.seed_lo, a.seed_hi).x >> 16;
                    lix = ix; liy = iy;
                }
                const uint32_t b = (v00 * (S - fx) + v01 * fx) * (S - fy) + (v10 * (S - fx) + v11 * fx) * fy;
                F[k] += (b >> (2 * s)) >> (7 - s);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t t = (fr.u0 * F[k]) >> 17;
#pragma unroll
            for (int c = 0; c < 3; ++c) px[3 * k + c] = (uint8_t)(((uint32_t)px[3 * k + c] * (256u - t) + 255u * t + 128u) >> 8);
        }
    }
    store_group(a.dst + fr.offset + (int64_t)g * 12, npx, px);
}

// CONV2D: the uint8 tile with its halo (coordinates clamped to the frame) and the taps are staged in LDS once per workgroup; a
// thread computes 4 horizontally adjacent pixels, sliding a 4-pixel window along each kernel row.
__global__ __launch_bounds__(256) void corrupt_conv_kernel(CorruptArgs a) {
    __shared__ uint8_t tile[CONV_TW * CONV_TW * 3];
    __shared__ uint16_t wt[CONV_KMAX * CONV_KMAX];
    const CorruptFrame& fr = a.frames[blockIdx.x / a.wgs_per_frame];
    if (fr.kind != BOD_CORRUPT_CONV2D) return;
    const int H = fr.h, W = fr.w, K = fr.ksize, r = K >> 1, TW = CONV_TILE + K - 1;      // (K odd, 1..25: corrupt_spec_make)
    const int tiles_x = (W + CONV_TILE - 1) / CONV_TILE, tiles_y = (H + CONV_TILE - 1) / CONV_TILE;
    const int l = blockIdx.x % a.wgs_per_frame;
    if (l >= tiles_x * tiles_y) return;
    const int y0 = (l / tiles_x) * CONV_TILE, x0 = (l % tiles_x) * CONV_TILE;
    const uint8_t* src = a.src + fr.offset;
    for (int i = threadIdx.x; i < K * K; i += 256) wt[i] = a.taps[fr.tap_offset + i];
    for (int i = threadIdx.x; i < TW * TW; i += 256) {
        const int ty = i / TW, tx = i % TW;
        const int gy = min(max(y0 - r + ty, 0), H - 1), gx = min(max(x0 - r + tx, 0), W - 1);
        const uint8_t* p = src + ((int64_t)gy * W + gx) * 3;
        tile[3 * i] = p[0]; tile[3 * i + 1] = p[1]; tile[3 * i + 2] = p[2];
    }
    __syncthreads();
    const int row = threadIdx.x >> 3, xq = (threadIdx.x & 7) * 4;
    uint32_t acc[4][3] = {};
    for (int ky = 0; ky < K; ++ky) {
        const uint8_t* rp = tile + ((row + ky) * TW + xq) * 3;
        uint32_t p[4][3];
#pragma unroll
        for (int j = 1; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) p[j][c] = rp[3 * (j - 1) + c];
        for (int kx = 0; kx < K; ++kx) {
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int c = 0; c < 3; ++c) p[j][c] = p[j + 1][c];
#pragma unroll
            for (int c = 0; c < 3; ++c) p[3][c] = rp[3 * (kx + 3) + c];         // (column xq + kx + 3 <= 28 + K + 2 = TW - 1)
            const uint32_t wv = wt[ky * K + kx];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[j][c] += wv * p[j][c];
        }
    }
    const int y = y0 + row;
    if (y >= H) return;
    uint8_t* dst = a.dst + fr.offset + ((int64_t)y * W + x0 + xq) * 3;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (x0 + xq + j < W) {
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[3 * j + c] = (uint8_t)((acc[j][c] + 16384u) >> 15);
        }
}

// PIXELATE: a workgroup owns nb x nb blocks (nb = 64 / f): column sums per block row, block means, then the tile's pixels
__global__ __launch_bounds__(256) void corrupt_pixelate_kernel(CorruptArgs a) {
    __shared__ uint32_t colsum[(PIX_TILE / 2) * PIX_TILE * 3];                  // [block row][x][c]: nb * T <= 32 * 64
    __shared__ uint8_t mean[(PIX_TILE / 2) * (PIX_TILE / 2) * 3];               // [block row][block column][c]
    const CorruptFrame& fr = a.frames[blockIdx.x / a.wgs_per_frame];
    if (fr.kind != BOD_CORRUPT_PIXELATE) return;
    const int H = fr.h, W = fr.w, f = (int)fr.u0, nb = PIX_TILE / f, T = nb * f;          // (f in 2..64: corrupt_spec_make)
    const int tiles_x = (W + T - 1) / T, tiles_y = (H + T - 1) / T;
    const int l = blockIdx.x % a.wgs_per_frame;
    if (l >= tiles_x * tiles_y) return;
    const int y0 = (l / tiles_x) * T, x0 = (l % tiles_x) * T;
    const uint8_t* src = a.src + fr.offset;
    for (int i = threadIdx.x; i < nb * T; i += 256) {
        const int by = i / T, gx = x0 + i % T;
        uint32_t s0 = 0, s1 = 0, s2 = 0;
        if (gx < W) {
            const int gy0 = y0 + by * f, rows = min(f, H - gy0);
            for (int rr = 0; rr < rows; ++rr) {
                const uint8_t* p = src + ((int64_t)(gy0 + rr) * W + gx) * 3;
                s0 += p[0]; s1 += p[1]; s2 += p[2];
            }
        }
        colsum[3 * i] = s0; colsum[3 * i + 1] = s1; colsum[3 * i + 2] = s2;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb * nb; i += 256) {
        const int by = i / nb, bx = i % nb;
        const int rows = min(f, H - (y0 + by * f)), cols = min(f, W - (x0 + bx * f));
        if (rows <= 0 || cols <= 0) continue;
        const uint32_t n = (uint32_t)rows * (uint32_t)cols;
        uint32_t s0 = 0, s1 = 0, s2 = 0;
        for (int xx = 0; xx < cols; ++xx) {
            const uint32_t* cs = colsum + (by * T + bx * f + xx) * 3;
            s0 += cs[0]; s1 += cs[1]; s2 += cs[2];
        }
        mean[3 * i] = (uint8_t)((s0 + n / 2) / n); mean[3 * i + 1] = (uint8_t)((s1 + n / 2) / n); mean[3 * i + 2] = (uint8_t)((s2 + n / 2) / n);
    }
    __syncthreads();
    uint8_t* dst = a.dst + fr.offset;
    for (int i = threadIdx.x; i < T * T; i += 256) {
        const int ty = i / T, tx = i % T, gy = y0 + ty, gx = x0 + tx;
        if (gy >= H || gx >= W) continue;
        const uint8_t* m = mean + ((ty / f) * nb + tx / f) * 3;
        uint8_t* p = dst + ((int64_t)gy * W + gx) * 3;
        p[0] = m[0]; p[1] = m[1]; p[2] = m[2];
    }
}

// jfdctint.c's 1-D forward transform (CONST_BITS = 13, PASS1_BITS = 2) on d[0..7] in place, with the pass's own scaling: the same
// twelve constants as jpeg_idct_1d
template <bool PASS2>
__device__ __forceinline__ void jpeg_fdct_1d(uint32_t d[8]) {
    const uint32_t t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const uint32_t t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int SH = PASS2 ? 15 : 11;
    uint32_t z1 = (t12 + t13) * 4433u;
    const uint32_t o0 = PASS2 ? (uint32_t)jpeg_descale(t10 + t11, 2) : (t10 + t11) << 2;
    const uint32_t o4 = PASS2 ? (uint32_t)jpeg_descale(t10 - t11, 2) : (t10 - t11) << 2;
    const uint32_t o2 = (uint32_t)jpeg_descale(z1 + t13 * 6270u, SH), o6 = (uint32_t)jpeg_descale(z1 - t12 * 15137u, SH);
    z1 = t4 + t7;
    uint32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const uint32_t z5 = (z3 + z4) * 9633u;
    const uint32_t a4 = t4 * 2446u, a5 = t5 * 16819u, a6 = t6 * 25172u, a7 = t7 * 12299u;
    z1 *= (uint32_t)-7373; z2 *= (uint32_t)-20995;
    z3 = z3 * (uint32_t)-16069 + z5; z4 = z4 * (uint32_t)-3196 + z5;
    d[0] = o0; d[4] = o4; d[2] = o2; d[6] = o6;
    d[7] = (uint32_t)jpeg_descale(a4 + z1 + z3, SH); d[5] = (uint32_t)jpeg_descale(a5 + z2 + z4, SH);
    d[3] = (uint32_t)jpeg_descale(a6 + z2 + z3, SH); d[1] = (uint32_t)jpeg_descale(a7 + z1 + z4, SH);
}

constexpr int32_t jfix(double x) { return (int32_t)(x * 65536.0 + 0.5); }

// JPEG: the 8x8-block-local round trip at 4:4:4.  Lane t of a block's 8 lanes holds row t of the three components through the colour
// conversion and the forward row pass, column t through the forward column pass, the quantisation and the decoder's column pass
// (jpeg_kernels.hip runs its first pass on columns too), and row t again for the decoder's row pass and the store.
__global__ __launch_bounds__(JPEG_THREADS) void corrupt_jpeg_kernel(CorruptArgs a) {
    __shared__ int32_t ws[JPEG_THREADS / 8][3][8 * JPEG_PITCH];
    const CorruptFrame& fr = a.frames[blockIdx.x / a.wgs_per_frame];
    if (fr.kind != BOD_CORRUPT_JPEG) return;
    const int H = fr.h, W = fr.w, t = threadIdx.x & 7, slot = threadIdx.x >> 3;
    const int bw = (W + 7) >> 3, bh = (H + 7) >> 3;
    const int l = (blockIdx.x % a.wgs_per_frame) * (JPEG_THREADS / 8) + slot;
    const bool live = l < bw * bh;
    const int by = live ? l / bw : 0, bx = live ? l % bw : 0;
    const uint16_t* qt = a.qtables + (size_t)fr.table * 128;
    uint32_t x[3][8];
    {   // colour conversion (jccolor.c) of row t, edge blocks replicating the last column / row; samples - 128; forward pass 1
        const uint8_t* rowp = a.src + fr.offset + (int64_t)min(by * 8 + t, H - 1) * W * 3;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint8_t* p = rowp + min(bx * 8 + j, W - 1) * 3;
            const int32_t R = p[0], G = p[1], B = p[2];
            x[0][j] = (uint32_t)(((jfix(0.299) * R + jfix(0.587) * G + jfix(0.114) * B + 32768) >> 16) - 128);
            x[1][j] = (uint32_t)(((-jfix(0.16874) * R - jfix(0.33126) * G + jfix(0.5) * B + (128 << 16) + 32767) >> 16) - 128);
            x[2][j] = (uint32_t)(((jfix(0.5) * R - jfix(0.41869) * G - jfix(0.08131) * B + (128 << 16) + 32767) >> 16) - 128);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            jpeg_fdct_1d<false>(x[c]);
#pragma unroll
            for (int j = 0; j < 8; ++j) ws[slot][c][t * JPEG_PITCH + j] = (int32_t)x[c][j];
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) {                 // column t: forward pass 2, quantise, dequantise, the decoder's pass 1
#pragma unroll
        for (int r = 0; r < 8; ++r) x[c][r] = (uint32_t)ws[slot][c][r * JPEG_PITCH + t];
        jpeg_fdct_1d<true>(x[c]);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const uint32_t q = qt[(c ? 64 : 0) + r * 8 + t], q8 = q * 8u;       // (q >= 1: corrupt_spec_make)
            const int32_t v = (int32_t)x[c][r];
            const uint32_t m = ((uint32_t)(v < 0 ? -v : v) + (q8 >> 1)) / q8;
            x[c][r] = (uint32_t)(v < 0 ? -(int32_t)m : (int32_t)m) * q;
        }
        jpeg_idct_1d(x[c]);
    }
    __syncthreads();                              // every lane has read its columns
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[slot][c][r * JPEG_PITCH + t] = jpeg_descale(x[c][r], 11);
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) {                 // row t: the decoder's pass 2
#pragma unroll
        for (int j = 0; j < 8; ++j) x[c][j] = (uint32_t)ws[slot][c][t * JPEG_PITCH + j];
        jpeg_idct_1d(x[c]);
#pragma unroll
        for (int j = 0; j < 8; ++j) x[c][j] = (uint32_t)min(max(jpeg_descale(x[c][j], 18) + 128, 0), 255);
    }
    const int y = by * 8 + t;
    if (!live || y >= H) return;
    uint8_t* dst = a.dst + fr.offset + ((int64_t)y * W + bx * 8) * 3;
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (bx * 8 + j < W) {
            int R, G, B;
            jpeg_ycc_to_rgb((int)x[0][j], (int)x[1][j] - 128, (int)x[2][j] - 128, R, G, B);
            dst[3 * j] = (uint8_t)R; dst[3 * j + 1] = (uint8_t)G; dst[3 * j + 2] = (uint8_t)B;
        }
}

template <typename KernelT>
hipError_t launch_one(KernelT kernel, CorruptArgs a, int32_t wgs, int threads, hipStream_t s) {
    if (wgs <= 0) return hipSuccess;
    a.wgs_per_frame = wgs;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((int64_t)a.n * wgs)), dim3(threads), 0, s, a);
    return hipGetLastError();
}

enum { WG_POINT = 0, WG_CONV = 1, WG_PIX = 2, WG_JPEG = 3 };

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace

void CorruptSlot::release() {
    if (dev) hipFree(dev);
    if (scratch) hipFree(scratch);
    if (copied) hipEventDestroy(copied);
    dev = nullptr; scratch = nullptr; copied = nullptr; dev_cap = scratch_cap = 0;
}

int corrupt_spec_make(const char* who, int32_t n, const bod_corrupt_op* ops, int32_t P, const uint32_t* frame_ids, const uint16_t* taps,
                      int32_t n_taps, const uint8_t* luts, int32_t n_luts, const uint16_t* qtables, int32_t n_qtables, uint64_t seed,
                      CorruptSpec* out, char* errbuf, size_t errcap) {
    Err err{errbuf, errcap};
    if (n < 1 || !ops) return err.fail(BOD_ERR_INVALID_ARG, "%s: no frame or no ops", who);
    if (P < 1 || P > 4) return err.fail(BOD_ERR_INVALID_ARG, "%s: ops_per_frame %d outside 1..4", who, P);
    if (n_taps < 0 || n_luts < 0 || n_qtables < 0 || (n_taps && !taps) || (n_luts && !luts) || (n_qtables && !qtables))
        return err.fail(BOD_ERR_INVALID_ARG, "%s: a table is NULL or its count negative", who);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < P; ++j) {
            const bod_corrupt_op& o = ops[(size_t)i * P + j];
            switch (o.kind) {
            case BOD_CORRUPT_NONE: case BOD_CORRUPT_IMPULSE_NOISE: break;
            case BOD_CORRUPT_LUT:
                if (o.table < 0 || o.table >= n_luts)
                    return err.fail(BOD_ERR_INVALID_ARG, "%s: frame %d op %d: LUT table %d outside the %d given", who, i, j, o.table, n_luts);
                break;
            case BOD_CORRUPT_CONTRAST:
                if (!isfinite(o.f0)) return err.fail(BOD_ERR_INVALID_ARG, "%s: frame %d op %d: contrast factor is not finite", who, i, j);
                break;
            case BOD_CORRUPT_GAUSSIAN_NOISE:
                if (!isfinite(o.f0) || o.f0 < 0.0f || o.f0 > 128.0f)
                    return err.fail(BOD_ERR_INVALID_ARG, "%s: frame %d op %d: sigma %g is not in [0, 128]", who, i, j, (double)o.f0);
                break;
            case BOD_CORRUPT_CONV2D: {
                if (o.ksize < 1 || o.ksize > CONV_KMAX || !(o.ksize & 1))
                    return err.fail(BOD_ERR_INVALID_ARG, "%s: frame %d op %d: kernel size %d is not odd and in 1..25", who, i, j, o.ksize);
                const int64_t kk = (int64_t)o.ksize * o.ksize;
                if (o.tap_offset < 0 || (int64_t)o.tap_offset + kk > n_taps)
                    return err.fail(BOD_ERR_INVALID_ARG, "%s: frame %d op %d: taps %d .. %lld lie past the table of %d", who, i, j, o.tap_offset,
                                    (long long)(o.tap_offset + kk), n_taps);
                uint64_t sum = 0;
                for (int64_t k = 0; k < kk; ++k) sum += taps[o.tap_offset + k];
                if (sum != 32768) return err.fail(BOD_ERR_INVALID_ARG, "%s: frame %d op %d: the taps sum to %llu, not 2^15", who, i, j, (unsigned long long)sum);
                break;
            }
            case BOD_CORRUPT_PIXELATE:
                if (o.u0 < 2 || o.u0 > 64) return err.fail(BOD_ERR_INVALID_ARG, "%s: frame %d op %d: block size %u outside 2..64", who, i, j, o.u0);
                break;
            case BOD_CORRUPT_JPEG:
                if (o.table < 0 || o.table >= n_qtables)
                    return err.fail(BOD_ERR_INVALID_ARG, "%s: frame %d op %d: quantisation table %d outside the %d given", who, i, j, o.table, n_qtables);
                for (int k = 0; k < 128; ++k)
                    if (qtables[(size_t)o.table * 128 + k] == 0)
                        return err.fail(BOD_ERR_INVALID_ARG, "%s: frame %d op %d: quantisation entry %d of table %d is zero", who, i, j, k, o.table);
                break;
            case BOD_CORRUPT_FOG:
                if (o.u0 > 256) return err.fail(BOD_ERR_INVALID_ARG, "%s: frame %d op %d: fog strength %u above 256", who, i, j, o.u0);
                break;
            default:
                return err.fail(BOD_ERR_INVALID_ARG, "%s: frame %d op %d: unknown kind %d", who, i, j, o.kind);
            }
        }
    try {
        CorruptSpec s;
        s.n = n; s.ops_per_frame = P; s.seed = seed;
        s.ops.assign(ops, ops + (size_t)n * P);
        s.frame_ids.resize((size_t)n);
        for (int i = 0; i < n; ++i) s.frame_ids[(size_t)i] = frame_ids ? frame_ids[i] : (uint32_t)i;
        if (n_taps) s.taps.assign(taps, taps + n_taps);
        if (n_luts) s.luts.assign(luts, luts + (size_t)n_luts * 768);
        if (n_qtables) s.qtables.assign(qtables, qtables + (size_t)n_qtables * 128);
        *out = std::move(s);
    } catch (const std::bad_alloc&) {
        return err.fail(BOD_ERR_OOM, "%s: out of host memory for the description", who);
    }
    return BOD_OK;
}

int corrupt_prepare(CorruptSlot& slot, const char* who, const CorruptSpec& spec, const int32_t* src_hw, hipStream_t stream, char* errbuf,
                    size_t errcap) {
    Err err{errbuf, errcap};
    const int n = spec.n, P = spec.ops_per_frame;
    std::vector<CorruptFrame> rec((size_t)n * P);
    int64_t off = 0;
    for (int j = 0; j < P; ++j) { slot.kinds[j] = 0; for (int k = 0; k < 4; ++k) slot.wgs[j][k] = 0; }
    for (int i = 0; i < n; ++i) {
        const int64_t h = src_hw[2 * i], w = src_hw[2 * i + 1];
        if (h < 1 || w < 1 || h * w > (1ll << 30)) return err.fail(BOD_ERR_INVALID_ARG, "%s: frame %d is %lldx%lld", who, i, (long long)h, (long long)w);
        for (int j = 0; j < P; ++j) {
            const bod_corrupt_op& o = spec.ops[(size_t)i * P + j];
            CorruptFrame& f = rec[(size_t)j * n + i];
            f = CorruptFrame{off, (int32_t)h, (int32_t)w, spec.frame_ids[(size_t)i], o.kind, o.f0, o.u0, o.tap_offset, o.ksize, o.table, 0};
            slot.kinds[j] |= 1u << o.kind;
            int64_t wg = 0; int which = WG_POINT;
            if (o.kind == BOD_CORRUPT_CONV2D) { which = WG_CONV; wg = ((h + CONV_TILE - 1) / CONV_TILE) * ((w + CONV_TILE - 1) / CONV_TILE); }
            else if (o.kind == BOD_CORRUPT_PIXELATE) { const int64_t T = (PIX_TILE / o.u0) * o.u0; which = WG_PIX; wg = ((h + T - 1) / T) * ((w + T - 1) / T); }
            else if (o.kind == BOD_CORRUPT_JPEG) { which = WG_JPEG; wg = (((h + 7) / 8) * ((w + 7) / 8) + JPEG_THREADS / 8 - 1) / (JPEG_THREADS / 8); }
            else wg = ((h * w + 3) / 4 + POINT_THREADS - 1) / POINT_THREADS;
            if (wg * n > 0x7FFFFFFF) return err.fail(BOD_ERR_INVALID_ARG, "%s: %d frames as large as frame %d are more than one launch covers", who, n, i);
            slot.wgs[j][which] = std::max(slot.wgs[j][which], (int32_t)wg);
        }
        off += 3 * h * w;
    }
    slot.frame_bytes = (size_t)off;
    const size_t rec_bytes = rec.size() * sizeof(CorruptFrame);
    slot.taps_off = align_up(rec_bytes, 16);
    slot.luts_off = align_up(slot.taps_off + spec.taps.size() * sizeof(uint16_t), 16);
    slot.q_off = align_up(slot.luts_off + spec.luts.size(), 16);
    const size_t host_bytes = align_up(slot.q_off + spec.qtables.size() * sizeof(uint16_t), 16);
    slot.sums_off = host_bytes;
    slot.sums_bytes = (size_t)P * n * 3 * sizeof(unsigned long long);
    const size_t dev_bytes = host_bytes + slot.sums_bytes;
    if (slot.copied && hipEventSynchronize(slot.copied) != hipSuccess) return err.fail(BOD_ERR_HIP, "%s: waiting for the previous table copy failed", who);
    try { slot.host.assign(host_bytes, 0); } catch (const std::bad_alloc&) { return err.fail(BOD_ERR_OOM, "%s: out of host memory for the op table", who); }
    memcpy(slot.host.data(), rec.data(), rec_bytes);
    if (!spec.taps.empty()) memcpy(slot.host.data() + slot.taps_off, spec.taps.data(), spec.taps.size() * sizeof(uint16_t));
    if (!spec.luts.empty()) memcpy(slot.host.data() + slot.luts_off, spec.luts.data(), spec.luts.size());
    if (!spec.qtables.empty()) memcpy(slot.host.data() + slot.q_off, spec.qtables.data(), spec.qtables.size() * sizeof(uint16_t));
    if (dev_bytes > slot.dev_cap || slot.frame_bytes > slot.scratch_cap) {
        if (hipStreamSynchronize(stream) != hipSuccess) return err.fail(BOD_ERR_HIP, "%s: hipStreamSynchronize failed", who);
        if (dev_bytes > slot.dev_cap) {
            if (slot.dev) hipFree(slot.dev);
            slot.dev = nullptr; slot.dev_cap = 0;
            if (hipMalloc(reinterpret_cast<void**>(&slot.dev), dev_bytes) != hipSuccess) { slot.dev = nullptr; return err.fail(BOD_ERR_OOM, "%s: %zu bytes of op table", who, dev_bytes); }
            slot.dev_cap = dev_bytes;
        }
        if (slot.frame_bytes > slot.scratch_cap) {
            if (slot.scratch) hipFree(slot.scratch);
            slot.scratch = nullptr; slot.scratch_cap = 0;
            if (hipMalloc(reinterpret_cast<void**>(&slot.scratch), slot.frame_bytes) != hipSuccess) { slot.scratch = nullptr; return err.fail(BOD_ERR_OOM, "%s: %zu bytes of corruption scratch", who, slot.frame_bytes); }
            slot.scratch_cap = slot.frame_bytes;
        }
    }
    if (!slot.copied && hipEventCreateWithFlags(&slot.copied, hipEventDisableTiming) != hipSuccess) { slot.copied = nullptr; return err.fail(BOD_ERR_HIP, "%s: hipEventCreate failed", who); }
    return BOD_OK;
}

int corrupt_enqueue(CorruptSlot& slot, const char* who, const CorruptSpec& spec, uint8_t* buf, hipStream_t stream, uint8_t** result, char* errbuf,
                    size_t errcap) {
    Err err{errbuf, errcap};
    const int n = spec.n, P = spec.ops_per_frame;
    hipError_t e = hipMemcpyAsync(slot.dev, slot.host.data(), slot.host.size(), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipEventRecord(slot.copied, stream);
    bool any_contrast = false;
    for (int j = 0; j < P; ++j) any_contrast |= (slot.kinds[j] >> BOD_CORRUPT_CONTRAST) & 1u;
    if (e == hipSuccess && any_contrast) e = hipMemsetAsync(slot.dev + slot.sums_off, 0, slot.sums_bytes, stream);
    uint8_t* cur = buf;
    uint8_t* other = slot.scratch;
    for (int j = 0; j < P && e == hipSuccess; ++j) {
        CorruptArgs a{};
        a.frames = reinterpret_cast<const CorruptFrame*>(slot.dev) + (size_t)j * n;
        a.src = cur; a.dst = other;
        a.taps = reinterpret_cast<const uint16_t*>(slot.dev + slot.taps_off);
        a.luts = reinterpret_cast<const uint8_t*>(slot.dev + slot.luts_off);
        a.qtables = reinterpret_cast<const uint16_t*>(slot.dev + slot.q_off);
        a.sums = reinterpret_cast<unsigned long long*>(slot.dev + slot.sums_off) + (size_t)j * n * 3;
        a.seed_lo = (uint32_t)spec.seed; a.seed_hi = (uint32_t)(spec.seed >> 32); a.slot = (uint32_t)j; a.n = n;
        const uint32_t kinds = slot.kinds[j];
        const int32_t pw = slot.wgs[j][WG_POINT];
        auto has = [&](int k) { return ((kinds >> k) & 1u) != 0; };
        if (e == hipSuccess && has(BOD_CORRUPT_NONE)) e = launch_one(corrupt_point_kernel<BOD_CORRUPT_NONE>, a, pw, POINT_THREADS, stream);
        if (e == hipSuccess && has(BOD_CORRUPT_LUT)) e = launch_one(corrupt_point_kernel<BOD_CORRUPT_LUT>, a, pw, POINT_THREADS, stream);
        if (e == hipSuccess && has(BOD_CORRUPT_CONTRAST)) {
            e = launch_one(corrupt_sum_kernel, a, (pw + SUM_GROUPS - 1) / SUM_GROUPS, POINT_THREADS, stream);
            if (e == hipSuccess) e = launch_one(corrupt_point_kernel<BOD_CORRUPT_CONTRAST>, a, pw, POINT_THREADS, stream);
        }
        if (e == hipSuccess && has(BOD_CORRUPT_IMPULSE_NOISE)) e = launch_one(corrupt_point_kernel<BOD_CORRUPT_IMPULSE_NOISE>, a, pw, POINT_THREADS, stream);
        if (e == hipSuccess && has(BOD_CORRUPT_GAUSSIAN_NOISE)) e = launch_one(corrupt_point_kernel<BOD_CORRUPT_GAUSSIAN_NOISE>, a, pw, POINT_THREADS, stream);
        if (e == hipSuccess && has(BOD_CORRUPT_FOG)) e = launch_one(corrupt_point_kernel<BOD_CORRUPT_FOG>, a, pw, POINT_THREADS, stream);
        if (e == hipSuccess && has(BOD_CORRUPT_CONV2D)) e = launch_one(corrupt_conv_kernel, a, slot.wgs[j][WG_CONV], 256, stream);
        if (e == hipSuccess && has(BOD_CORRUPT_PIXELATE)) e = launch_one(corrupt_pixelate_kernel, a, slot.wgs[j][WG_PIX], 256, stream);
        if (e == hipSuccess && has(BOD_CORRUPT_JPEG)) e = launch_one(corrupt_jpeg_kernel, a, slot.wgs[j][WG_JPEG], JPEG_THREADS, stream);
        std::swap(cur, other);
    }
    if (e != hipSuccess) return err.fail(BOD_ERR_HIP, "%s: the corruption stage failed: %s", who, hipGetErrorString(e));
    *result = cur;
    return BOD_OK;
}

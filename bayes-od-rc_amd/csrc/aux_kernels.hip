// Stem of the ResNet-50 backbone: 7x7 s2 VALID conv + folded BN + ReLU, then
// ZeroPadding2D((1,2)) + MaxPool 3x3 s2 VALID   (src/retina_net/models/feature_extractor.py:17-33,
// :107-111).  The 3-channel input is never rounded to bf16 (fp32 mode:
// exact fp32 MFMA; bf16 mode: hi + lo split); everything after is bf16 storage.
#include "kernels.h"

__device__ __forceinline__ uint32_t f32_to_bf16_a(float f) {
    uint32_t u = __float_as_uint(f);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return u >> 16;
}
__device__ __forceinline__ float bf16_to_f32_a(uint32_t v) { return __uint_as_float(v << 16); }

// Stem as an exact-fp32 implicit GEMM on v_mfma_f32_16x16x4_f32 (f32 in / f32 accumulate, bitwise an
// fmaf chain): D[cout 64][pixel] with K ordered (ky, kx*3+ci) and each ky row padded 21 -> 24, so the
// B operand of one k-step is 4 CONSECUTIVE floats of an input row.  Each wave keeps ALL weights as
// MFMA A fragments in registers (42 k-steps x 4 cout fragments = 168 VGPRs, one wave per SIMD, 4
// independent accumulators = the f32 MFMA issue rate) and the block walks (image,row,64-pixel
// segment) tasks persistently; the 7 x 133 x 3 input patch of the next task is prefetched into the
// other LDS buffer while the current one is multiplied.
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
constexpr int ST_SEG = 64;                      // output pixels per task (4 waves x 16)
constexpr int ST_ROWF = 2 * ST_SEG * 3 + 5 * 3 + 5;   // 404 floats: (2*63+7) pixels * 3 ch = 399, + the 3 zero-weight k slots, padded
constexpr int ST_KSTEPS = 42;                   // 7 rows x 24 (21 real + 3 zero) / 4

__global__ __launch_bounds__(256, 1) void stem_conv_kernel(const float* __restrict__ img,
                                                           const float* __restrict__ w,
                                                           const float* __restrict__ bias,
                                                           float* __restrict__ out,
                                                           int B, int H, int W, int oh, int ow) {
    __shared__ float patch[2][7][ST_ROWF];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lq = lane >> 4;
    // A fragments: a[s][f] = W[k = s*4+lq][cout = f*16+li], k -> (ky = s/6, t = (s%6)*4+lq), zero for t >= 21
    float a[ST_KSTEPS][4];
#pragma unroll
    for (int s = 0; s < ST_KSTEPS; ++s) {
        const int ky = s / 6, t = (s % 6) * 4 + lq;
#pragma unroll
        for (int f = 0; f < 4; ++f) a[s][f] = t < 21 ? w[(ky * 21 + t) * 64 + f * 16 + li] : 0.f;
    }
    float bv[4][4];
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) bv[f][r] = bias[f * 16 + lq * 4 + r];

    const int segs = (ow + ST_SEG - 1) / ST_SEG;
    const int ntasks = B * oh * segs;
    constexpr int ST_PER = (7 * ST_ROWF + 255) / 256;          // staged floats per thread
    float stage[ST_PER];
    auto fetch = [&](int task) {                               // global -> registers (in flight during the MFMAs)
        const int seg = task % segs, oy = (task / segs) % oh, b = task / (segs * oh);
        const float* src = img + ((size_t)b * H + 2 * oy) * W * 3 + (size_t)seg * ST_SEG * 2 * 3;
        const int valid = W * 3 - seg * ST_SEG * 2 * 3;           // floats left in the row
#pragma unroll
        for (int q = 0; q < ST_PER; ++q) {
            const int i = tid + q * 256;
            const int r = i / ST_ROWF, c = i % ST_ROWF;
            stage[q] = (i < 7 * ST_ROWF && c < valid) ? src[(size_t)r * W * 3 + c] : 0.f;
        }
    };
    auto commit = [&](int buf) {                               // registers -> LDS
#pragma unroll
        for (int q = 0; q < ST_PER; ++q) {
            const int i = tid + q * 256;
            if (i < 7 * ST_ROWF) (&patch[buf][0][0])[i] = stage[q];
        }
    };
    int task = blockIdx.x, buf = 0;
    if (task < ntasks) { fetch(task); commit(0); }
    __syncthreads();
    for (; task < ntasks; task += gridDim.x, buf ^= 1) {
        const int nxt = task + gridDim.x;
        if (nxt < ntasks) fetch(nxt);
        f32x4_t acc[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) acc[f] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        // B operand: lane (pixel li of this wave's 16, k offset lq): patch[ky][(wave*16+li)*6 + t]
        const float* pb = &patch[buf][0][(wave * 16 + li) * 6 + lq];
#pragma unroll
        for (int s = 0; s < ST_KSTEPS; ++s) {
            const float bq = pb[(s / 6) * ST_ROWF + (s % 6) * 4];
#pragma unroll
            for (int f = 0; f < 4; ++f)
                acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][f], bq, acc[f], 0, 0, 0);
        }
        const int seg = task % segs, oy = (task / segs) % oh, b = task / (segs * oh);
        const int ox = seg * ST_SEG + wave * 16 + li;
        if (ox < ow) {
            float* o = out + (((size_t)b * oh + oy) * ow + ox) * 64 + lq * 4;
#pragma unroll
            for (int f = 0; f < 4; ++f)
                *reinterpret_cast<float4*>(o + f * 16) =
                    make_float4(fmaxf(acc[f][0] + bv[f][0], 0.f), fmaxf(acc[f][1] + bv[f][1], 0.f),
                                fmaxf(acc[f][2] + bv[f][2], 0.f), fmaxf(acc[f][3] + bv[f][3], 0.f));
        }
        if (nxt < ntasks) commit(buf ^ 1);
        __syncthreads();
    }
}

// bf16 mode: the same implicit GEMM on v_mfma_f32_16x16x32_bf16.  The image stays exact to 2^-17: every staged
// pixel value is split x = hi + lo (two bf16) when it is written to LDS, and both halves are multiplied with the
// bf16-rounded folded weights (like every other layer of this mode, the stem's weights are bf16; fp32 accumulate).
// K per ky row = 24 slots (21 real + 3 zero-weight) = 3 chunks of 8; an MFMA k-step covers chunks (2s, 2s+1), its
// four k-blocks being (chunk 2s, hi), (2s+1, hi), (2s, lo), (2s+1, lo): 11 steps x 4 cout fragments = 44 MFMAs per
// 16 pixels x 64 channels (the fp32 kernel: 168 four-times-slower ones).  Weights live in LDS (one copy per block),
// so the kernel needs few registers and three blocks per CU keep enough loads in flight to stream the image.
typedef __attribute__((ext_vector_type(8))) __bf16 stem_bf16x8_t;
constexpr int SB_ROWE = 408;                    // uint16 per staged row (404 used)
constexpr int SB_WROW = 184;                    // uint16 per weight row: 22 chunks x 8 + 8 pad (368 B: conflict-free b128 reads)

__global__ __launch_bounds__(256) void stem_conv_bf16_kernel(const float* __restrict__ img, const float* __restrict__ w,
                                                             const float* __restrict__ bias, uint16_t* __restrict__ out,
                                                             int B, int H, int W, int oh, int ow) {
    __shared__ __attribute__((aligned(16))) uint16_t wl[64][SB_WROW];
    __shared__ __attribute__((aligned(16))) uint16_t patch[2][2][7][SB_ROWE];       // [buffer][hi / lo][ky][element]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lq = lane >> 4;
    for (int i = tid; i < 64 * SB_WROW; i += 256) {
        const int co = i / SB_WROW, kp = i % SB_WROW;
        const int c = kp >> 3, t = kp & 7, ky = c / 3, j = (c % 3) * 8 + t;
        wl[co][kp] = (c < 21 && j < 21) ? (uint16_t)f32_to_bf16_a(w[(ky * 21 + j) * 64 + co]) : (uint16_t)0;
    }
    float bv[4][4];
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) bv[f][r] = bias[f * 16 + lq * 4 + r];

    const int segs = (ow + ST_SEG - 1) / ST_SEG;
    const int ntasks = B * oh * segs;
    constexpr int ST_PER = (7 * ST_ROWF + 255) / 256;
    float stage[ST_PER];
    auto fetch = [&](int task) {
        const int seg = task % segs, oy = (task / segs) % oh, b = task / (segs * oh);
        const float* src = img + ((size_t)b * H + 2 * oy) * W * 3 + (size_t)seg * ST_SEG * 2 * 3;
        const int valid = W * 3 - seg * ST_SEG * 2 * 3;
#pragma unroll
        for (int q = 0; q < ST_PER; ++q) {
            const int i = tid + q * 256;
            const int r = i / ST_ROWF, c = i % ST_ROWF;
            stage[q] = (i < 7 * ST_ROWF && c < valid) ? src[(size_t)r * W * 3 + c] : 0.f;
        }
    };
    auto commit = [&](int buf) {                               // registers -> LDS as hi / lo bf16
#pragma unroll
        for (int q = 0; q < ST_PER; ++q) {
            const int i = tid + q * 256;
            if (i >= 7 * ST_ROWF) continue;
            const int r = i / ST_ROWF, c = i % ST_ROWF;
            const uint32_t hi = f32_to_bf16_a(stage[q]);
            const uint32_t lo = f32_to_bf16_a(stage[q] - bf16_to_f32_a(hi));
            patch[buf][0][r][c] = (uint16_t)hi;
            patch[buf][1][r][c] = (uint16_t)lo;
        }
    };
    // this lane's B source: plane (lq & 1), pixel wave*16 + li, chunk parity lq >> 1 (see SR_ROWE: the two planes of one chunk share a 32-lane LDS access)
    const int role = lq & 1, k1 = lq >> 1;
    int task = blockIdx.x, buf = 0;
    if (task < ntasks) { fetch(task); commit(0); }
    __syncthreads();
    for (; task < ntasks; task += gridDim.x, buf ^= 1) {
        const int nxt = task + gridDim.x;
        if (nxt < ntasks) fetch(nxt);
        f32x4_t acc[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) acc[f] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        const uint16_t* pb = &patch[buf][role][0][(wave * 16 + li) * 6];
#pragma unroll
        for (int s = 0; s < 11; ++s) {
            const int c = 2 * s + k1;
            const int cc = c < 21 ? c : 20;                    // chunk 21 has zero weights: any finite data will do
            const int ky = cc / 3, j0 = (cc - 3 * ky) * 8;
            union { uint32_t u[4]; stem_bf16x8_t v; } bq;
            const uint32_t* src = reinterpret_cast<const uint32_t*>(pb + ky * SB_ROWE + j0);
#pragma unroll
            for (int t = 0; t < 4; ++t) bq.u[t] = src[t];
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                const stem_bf16x8_t aq = *reinterpret_cast<const stem_bf16x8_t*>(&wl[f * 16 + li][c * 8]);
                acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aq, bq.v, acc[f], 0, 0, 0);
            }
        }
        const int seg = task % segs, oy = (task / segs) % oh, b = task / (segs * oh);
        const int ox = seg * ST_SEG + wave * 16 + li;
        if (ox < ow) {
            uint16_t* o = out + (((size_t)b * oh + oy) * ow + ox) * 64 + lq * 4;
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                uint2 pk;
                pk.x = f32_to_bf16_a(fmaxf(acc[f][0] + bv[f][0], 0.f)) | (f32_to_bf16_a(fmaxf(acc[f][1] + bv[f][1], 0.f)) << 16);
                pk.y = f32_to_bf16_a(fmaxf(acc[f][2] + bv[f][2], 0.f)) | (f32_to_bf16_a(fmaxf(acc[f][3] + bv[f][3], 0.f)) << 16);
                *reinterpret_cast<uint2*>(o + f * 16) = pk;
            }
        }
        if (nxt < ntasks) commit(buf ^ 1);
        __syncthreads();
    }
}

// Round 3: the same arithmetic (same MFMAs in the same order per accumulator: bit-identical outputs) with the operand reuse
// the kernel above lacks.  There every MFMA reads its weight fragment (1 KB) AND a quarter of a pixel fragment from LDS --
// 1.25 KB per MFMA against the 0.5 KB per MFMA slot the LDS pipe delivers to four SIMDs -- so the launch ran at the LDS issue
// rate (1.85 ms at 256 frames of 512x512, 167 TF/s).  Here a task is 256 pixels of one output row, a wave owns 64 of them x
// 64 channels = 4 x 4 fragments, ALL weights live in registers (11 k-steps x 4 cout fragments = 176 VGPRs, loaded once per
// block through LDS) and a pixel fragment read from LDS feeds four MFMAs: 0.25 KB of LDS per MFMA.  One block per CU (about
// 330 registers per lane); 16 independent accumulators per wave keep the matrix pipe issuing at one wave per SIMD.  The staging
// is vectorised (16-byte loads, hardware bf16 packs, 8-byte LDS writes) and the outputs leave as whole 128-byte pixel rows
// through a per-wave LDS tile.  Measured at 256 frames of 512x512: op trace 1.42-1.86 -> 1.19-1.39 ms; in the pipelined step
// the backbone stage moves by 0.2 ms (25.5 -> 25.3): the old kernel's steady-state time is the low end of its trace range.
constexpr int SR_SEG = 256;                               // output pixels per task (4 waves x 4 fragments x 16)
constexpr int SR_ROWF = 2 * SR_SEG * 3 + 5 * 3 + 5;       // 1556 floats: (2*255+7)*3 = 1551 real + 3 zero-weight k slots, padded
// uint16 per staged LDS row.  1568 = 784 dwords = 16 mod 32: the B fragments are read dword-wise (12-byte pixel stride), a 32-lane LDS
// access = 16 pixels x the (hi, lo) planes of ONE chunk, and with the planes 16 banks apart the two 3-dword-stride combs interleave
// without a collision (round 4: with 1560 and the planes in different accesses -- lanes paired by chunk parity instead -- four banks
// of every access were hit twice: 40 % of the fused kernel's LDS cycles, tests/tools/pmc_kernel.sh)
constexpr int SR_ROWE = 1568;
constexpr int SR_PLANE = 7 * SR_ROWE;                     // one (hi or lo) plane of a buffer
constexpr int SR_LDS_BYTES = 2 * 2 * SR_PLANE * 2;        // [buffer][hi / lo][ky][element] = 87 808 B; the weight table aliases buffer 1
constexpr int SR_LDS_TOTAL = SR_LDS_BYTES + 4 * 8192;     // + one 8 KB epilogue tile per wave

__global__ __launch_bounds__(256, 1) void stem_conv_bf16_row_kernel(const float* __restrict__ img, const float* __restrict__ w,
                                                                    const float* __restrict__ bias, uint16_t* __restrict__ out,
                                                                    int B, int H, int W, int oh, int ow) {
    extern __shared__ __attribute__((aligned(16))) uint16_t sr_smem[];
    uint16_t* patch = sr_smem;                                          // [buf][plane][ky][SR_ROWE]
    uint16_t (*wl)[SB_WROW] = reinterpret_cast<uint16_t (*)[SB_WROW]>(sr_smem + 2 * SR_PLANE);   // inside buffer 1, dead before its first use
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lq = lane >> 4;
    for (int i = tid; i < 64 * SB_WROW; i += 256) {
        const int co = i / SB_WROW, kp = i % SB_WROW;
        const int c = kp >> 3, t = kp & 7, ky = c / 3, j = (c % 3) * 8 + t;
        wl[co][kp] = (c < 21 && j < 21) ? (uint16_t)f32_to_bf16_a(w[(ky * 21 + j) * 64 + co]) : (uint16_t)0;
    }
    float bv[4][4];
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) bv[f][r] = bias[f * 16 + lq * 4 + r];

    const int segs = (ow + SR_SEG - 1) / SR_SEG;
    const int ntasks = B * oh * segs;
    // staging: 16-byte loads of four consecutive row floats (rows start 16-byte aligned and end on a multiple of four floats:
    // the launcher requires W % 4 == 0), the hi / lo split on the hardware pack v_cvt_pk_bf16_f32 (round-to-nearest-even, the
    // same values as f32_to_bf16_a on finite inputs), 8-byte LDS writes
    constexpr int ROWQ = SR_ROWF / 4;                                   // 389 quads per row
    constexpr int PER = (7 * ROWQ + 255) / 256;                         // 11 staged quads per thread
    static_assert(PER <= 11, "one staged quad per k-step");
    auto fetch = [&](int task, float4 (&stage)[PER]) {
        const int seg = task % segs, oy = (task / segs) % oh, b = task / (segs * oh);
        const float* src = img + ((size_t)b * H + 2 * oy) * W * 3 + (size_t)seg * SR_SEG * 2 * 3;
        const int valid = W * 3 - seg * SR_SEG * 2 * 3;
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int i = tid + q * 256;
            const int r = i / ROWQ, c = (i - r * ROWQ) * 4;
            stage[q] = (i < 7 * ROWQ && c < valid) ? *reinterpret_cast<const float4*>(src + (size_t)r * W * 3 + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto pk = [](float lo, float hi) { uint32_t r; asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi)); return r; };
    auto commit_piece = [&](int buf, int q, const float4 (&stage)[PER]) {      // one staged quad -> LDS as hi / lo bf16
        uint16_t* pb = patch + buf * 2 * SR_PLANE;
        const int i = tid + q * 256;
        if (i >= 7 * ROWQ) return;
        const int r = i / ROWQ, c = (i - r * ROWQ) * 4;
        const float4 v = stage[q];
        const uint32_t h0 = pk(v.x, v.y), h1 = pk(v.z, v.w);
        const uint32_t l0 = pk(v.x - __uint_as_float(h0 << 16), v.y - __uint_as_float(h0 & 0xFFFF0000u));
        const uint32_t l1 = pk(v.z - __uint_as_float(h1 << 16), v.w - __uint_as_float(h1 & 0xFFFF0000u));
        *reinterpret_cast<uint2*>(pb + r * SR_ROWE + c) = make_uint2(h0, h1);
        *reinterpret_cast<uint2*>(pb + SR_PLANE + r * SR_ROWE + c) = make_uint2(l0, l1);
    };
    const int role = lq & 1, k1 = lq >> 1;                              // this lane's B source: plane, chunk parity (see SR_ROWE)
    // (Measured and not kept: the next patch's conversion + LDS writes one quad per k-step behind that step's MFMAs, with one or
    // two register stages -- 1.95 ms against 1.39 ms for the plain order below: at one wave per SIMD the interleaved VALU / LDS
    // traffic delays the MFMA issue more than the overlap returns.)
    float4 stage[PER];
    int task = blockIdx.x, buf = 0;
    const int g = gridDim.x;
    if (task < ntasks) {
        fetch(task, stage);
#pragma unroll
        for (int q = 0; q < PER; ++q) commit_piece(0, q, stage);
    }
    __syncthreads();
    stem_bf16x8_t aqr[11][4];
#pragma unroll
    for (int s = 0; s < 11; ++s)
#pragma unroll
        for (int f = 0; f < 4; ++f) aqr[s][f] = *reinterpret_cast<const stem_bf16x8_t*>(&wl[f * 16 + li][(2 * s + k1) * 8]);
    __syncthreads();                                                    // the table's LDS becomes buffer 1
    for (; task < ntasks; task += g, buf ^= 1) {
        const int nxt = task + g;
        if (nxt < ntasks) fetch(nxt, stage);
        f32x4_t acc[4][4];
#pragma unroll
        for (int f = 0; f < 4; ++f)
#pragma unroll
            for (int p = 0; p < 4; ++p) acc[f][p] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        const uint16_t* pb = patch + (buf * 2 + role) * SR_PLANE + (wave * 64 + li) * 6;
        // (Measured and not kept: reading the four pixel fragments of k-step s+1 in front of the 16 MFMAs of step s, pinned with a
        // scheduling barrier -- 1.62 ms against 1.39 ms for the compiler's own order below.)
#pragma unroll
        for (int s = 0; s < 11; ++s) {
            const int c = 2 * s + k1;
            const int cc = c < 21 ? c : 20;                             // chunk 21 has zero weights: any finite data will do
            const int ky = cc / 3, j0 = (cc - 3 * ky) * 8;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                union { uint32_t u[4]; stem_bf16x8_t v; } bq;
                const uint32_t* src = reinterpret_cast<const uint32_t*>(pb + p * 96 + ky * SR_ROWE + j0);
#pragma unroll
                for (int t = 0; t < 4; ++t) bq.u[t] = src[t];
#pragma unroll
                for (int f = 0; f < 4; ++f) acc[f][p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aqr[s][f], bq.v, acc[f][p], 0, 0, 0);
            }
        }
        const int seg = task % segs, oy = (task / segs) % oh, b = task / (segs * oh);
        // epilogue through a per-wave LDS tile [64 pixels][128 B] (16-byte chunks XOR-swizzled by the pixel): a lane's 8-byte
        // pieces of four channels become whole 128-byte pixel rows, stored 16 B per lane = 1 KB contiguous per instruction
        // (the wave's 64 pixels are 8 KB contiguous in the NHWC plane; the accumulator layout gave 32-byte pieces per pixel)
        char* et = reinterpret_cast<char*>(sr_smem) + SR_LDS_BYTES + wave * 8192;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int px = p * 16 + li;
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                uint2 pkd;
                pkd.x = pk(fmaxf(acc[f][p][0] + bv[f][0], 0.f), fmaxf(acc[f][p][1] + bv[f][1], 0.f));
                pkd.y = pk(fmaxf(acc[f][p][2] + bv[f][2], 0.f), fmaxf(acc[f][p][3] + bv[f][3], 0.f));
                const int chunk = f * 2 + (lq >> 1);
                *reinterpret_cast<uint2*>(et + px * 128 + ((chunk ^ (px & 7)) << 4) + (lq & 1) * 8) = pkd;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        {
            const int ox0 = seg * SR_SEG + wave * 64;
            char* orow = reinterpret_cast<char*>(out + (((size_t)b * oh + oy) * ow + ox0) * 64);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int px = i * 8 + (lane >> 3), ch = lane & 7;
                const uint4 v = *reinterpret_cast<const uint4*>(et + px * 128 + ((ch ^ (px & 7)) << 4));
                if (ox0 + px < ow) *reinterpret_cast<uint4*>(orow + px * 128 + ch * 16) = v;
            }
        }
        if (nxt < ntasks) {
#pragma unroll
            for (int q = 0; q < PER; ++q) commit_piece(buf ^ 1, q, stage);
        }
        __syncthreads();
    }
}

// Round 3: stem + ZeroPadding2D((1,2)) + max-pool in ONE kernel (bf16 inference, stem rows of at most 256 pixels).  A workgroup owns
// an image and walks DOWN it: a stem row needs input rows 2r .. 2r+6, the next one two new rows -- an eight-slot LDS ring of (hi, lo)
// input rows, every input row loaded once instead of 3.5 times -- and every stem row is max-combined in registers (packed bf16, all
// values >= 0) into the pooling window it belongs to; every second row the window is finished through an LDS tile (the horizontal
// 3-window, stride 2) and ONLY the pooled row is stored: the 2.1 GB stem plane (at 256 frames of 512 x 512) is neither written nor
// re-read.  Same MFMAs in the same order as the row kernel above, the same packs and the same maxima as stem_pool_kernel:
// bit-identical pooled plane (tests/test_gpu_forward.py::test_fused_stem_pool_is_bit_identical; BOD_STEM_POOL_FUSED=0: separate).
constexpr int SF_RING = 8;
constexpr int SF_LDS_BYTES = SF_RING * 2 * SR_ROWE * 2 + 256 * 128;      // ring [8][hi / lo][SR_ROWE] uint16 + tile [256 px][64 ch]

__device__ __forceinline__ uint32_t sf_max(uint32_t a, uint32_t b) {
    uint32_t r;
    asm("v_pk_max_i16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// NCH = 1: four waves, each a 64-pixel quarter of the row x all 64 couts (176 weight registers, one wave per SIMD).  NCH = 2 (round 4):
// eight waves = pixel quarter x cout half -- 88 weight registers, TWO waves per SIMD, so one wave's LDS round trips, conversions and
// barriers hide behind the other's MFMAs; every B fragment is read by two waves.  Same MFMAs in the same order per accumulator.
template <int NCH>
__global__ __launch_bounds__(256 * NCH, 1) void stem_pool_fused_kernel(const float* __restrict__ img, const float* __restrict__ w,
                                                                 const float* __restrict__ bias, uint16_t* __restrict__ pooled,
                                                                 int B, int H, int W, int oh, int ow, int ph, int pw, int pool_pitch,
                                                                 int pool_plane) {
    extern __shared__ __attribute__((aligned(16))) uint16_t sf_smem[];
    uint16_t* const ring = sf_smem;                                     // slot s, plane h: ring + (s * 2 + h) * SR_ROWE
    char* const tile = reinterpret_cast<char*>(sf_smem + SF_RING * 2 * SR_ROWE);      // [256 px][128 B], 16-byte chunks swizzled by the pixel
    uint16_t (*wl)[SB_WROW] = reinterpret_cast<uint16_t (*)[SB_WROW]>(tile);          // the weight table lives in the tile until the loop starts
    constexpr int THREADS = 256 * NCH, FW = 4 / NCH;                    // cout fragments of 16 per wave
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pxq = wave & 3, chh = wave >> 2;                          // pixel quarter, cout half
    const int li = lane & 15, lq = lane >> 4;
    for (int i = tid; i < 64 * SB_WROW; i += THREADS) {
        const int co = i / SB_WROW, kp = i % SB_WROW;
        const int c = kp >> 3, t = kp & 7, ky = c / 3, j = (c % 3) * 8 + t;
        wl[co][kp] = (c < 21 && j < 21) ? (uint16_t)f32_to_bf16_a(w[(ky * 21 + j) * 64 + co]) : (uint16_t)0;
    }
    float bv[FW][4];
#pragma unroll
    for (int f = 0; f < FW; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) bv[f][r] = bias[(chh * FW + f) * 16 + lq * 4 + r];
    constexpr int ROWQ = SR_ROWF / 4;                                   // 389 quads per input row
    auto pk = [](float lo, float hi) { uint32_t r; asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi)); return r; };
    const int valid = W * 3;
    const float* const im = img + (size_t)blockIdx.x * H * W * 3;
    // quad q of input row ir: fetch / convert-and-store (hi, lo) into ring slot ir & 7
    auto fetch_quad = [&](int ir, int q) {
        const int c = q * 4;
        return (q < ROWQ && c < valid && ir < H) ? *reinterpret_cast<const float4*>(im + (size_t)ir * W * 3 + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    auto commit_quad = [&](int ir, int q, const float4 v) {
        if (q >= ROWQ) return;
        uint16_t* pb = ring + ((ir & (SF_RING - 1)) * 2) * SR_ROWE + q * 4;
        const uint32_t h0 = pk(v.x, v.y), h1 = pk(v.z, v.w);
        const uint32_t l0 = pk(v.x - __uint_as_float(h0 << 16), v.y - __uint_as_float(h0 & 0xFFFF0000u));
        const uint32_t l1 = pk(v.z - __uint_as_float(h1 << 16), v.w - __uint_as_float(h1 & 0xFFFF0000u));
        *reinterpret_cast<uint2*>(pb) = make_uint2(h0, h1);
        *reinterpret_cast<uint2*>(pb + SR_ROWE) = make_uint2(l0, l1);
    };
    // ---- prologue: input rows 0 .. 6, the weights into registers
    for (int ir = 0; ir < 7; ++ir)
        for (int q = tid; q < ROWQ; q += THREADS) commit_quad(ir, q, fetch_quad(ir, q));
    __syncthreads();
    const int role = lq & 1, k1 = lq >> 1;                              // this lane's B source: plane, chunk parity (see SR_ROWE)
    stem_bf16x8_t aqr[11][FW];
#pragma unroll
    for (int s = 0; s < 11; ++s)
#pragma unroll
        for (int f = 0; f < FW; ++f) aqr[s][f] = *reinterpret_cast<const stem_bf16x8_t*>(&wl[(chh * FW + f) * 16 + li][(2 * s + k1) * 8]);
    __syncthreads();                                                    // the table's LDS becomes the pooling tile
    uint2 vm[FW][4];                                                    // running maximum of the open pooling window: [cout frag][pixel frag]
#pragma unroll
    for (int f = 0; f < FW; ++f)
#pragma unroll
        for (int p = 0; p < 4; ++p) vm[f][p] = make_uint2(0u, 0u);
    uint16_t* const obase = pooled + (size_t)blockIdx.x * pool_plane * 64;

    for (int r = 0; r < oh; ++r) {
        // the two input rows the NEXT stem row adds (2r+7, 2r+8): four quads per thread, in flight during this row's MFMAs
        constexpr int NQ = 1024 / THREADS;
        float4 st[NQ];
#pragma unroll
        for (int i = 0; i < NQ; ++i) { const int q = i * THREADS + tid; st[i] = fetch_quad(2 * r + 7 + (q >= 512), q & 511); }
        f32x4_t acc[FW][4];
#pragma unroll
        for (int f = 0; f < FW; ++f)
#pragma unroll
            for (int p = 0; p < 4; ++p) acc[f][p] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 11; ++s) {
            const int c = 2 * s + k1;
            const int cc = c < 21 ? c : 20;                             // chunk 21 has zero weights: any finite data will do
            const int ky = cc / 3, j0 = (cc - 3 * ky) * 8;
            const uint16_t* pb = ring + ((((2 * r + ky) & (SF_RING - 1)) * 2) + role) * SR_ROWE + (pxq * 64 + li) * 6 + j0;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                union { uint32_t u[4]; stem_bf16x8_t v; } bq;
                const uint32_t* src = reinterpret_cast<const uint32_t*>(pb + p * 96);
#pragma unroll
                for (int t = 0; t < 4; ++t) bq.u[t] = src[t];
#pragma unroll
                for (int f = 0; f < FW; ++f) acc[f][p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aqr[s][f], bq.v, acc[f][p], 0, 0, 0);
            }
        }
        // this stem row joins the open pooling window (rows 2p-1, 2p, 2p+1): bias + ReLU + pack exactly like the stem kernels, then a
        // packed signed 16-bit maximum (every value is >= +0; a -0 from fmaxf can never win against the window's initial +0)
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int f = 0; f < FW; ++f) {
                const uint32_t x = pk(fmaxf(acc[f][p][0] + bv[f][0], 0.f), fmaxf(acc[f][p][1] + bv[f][1], 0.f));
                const uint32_t y = pk(fmaxf(acc[f][p][2] + bv[f][2], 0.f), fmaxf(acc[f][p][3] + bv[f][3], 0.f));
                vm[f][p].x = sf_max(vm[f][p].x, x); vm[f][p].y = sf_max(vm[f][p].y, y);
                acc[f][p][0] = __uint_as_float(x); acc[f][p][1] = __uint_as_float(y);      // (kept: an odd row opens the next window)
            }
        const bool closes = (r & 1) || r == oh - 1;                     // row 2p+1 closes window p; so does the last row of an odd-height plane
        if (closes) {
            const int prow = r >> 1;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int px = pxq * 64 + p * 16 + li;
#pragma unroll
                for (int f = 0; f < FW; ++f)
                    *reinterpret_cast<uint2*>(tile + px * 128 + ((((chh * FW + f) * 2 + (lq >> 1)) ^ (px & 7)) << 4) + (lq & 1) * 8) = vm[f][p];
            }
            __syncthreads();
            if (prow < ph) {
                // horizontal window: pooled column q = max over stem columns 2q-2, 2q-1, 2q (those inside the row)
                for (int i = tid; i < pw * 8; i += THREADS) {
                    const int q = i >> 3, ch = i & 7;
                    uint4 m = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const int px = 2 * q + kx - 2;
                        if (px < 0 || px >= ow) continue;
                        const uint4 v = *reinterpret_cast<const uint4*>(tile + px * 128 + ((ch ^ (px & 7)) << 4));
                        m.x = sf_max(m.x, v.x); m.y = sf_max(m.y, v.y); m.z = sf_max(m.z, v.z); m.w = sf_max(m.w, v.w);
                    }
                    *reinterpret_cast<uint4*>(obase + ((size_t)(prow + 1) * pool_pitch + (q + 1)) * 64 + ch * 8) = m;
                }
            }
            // the closing row (when it is row 2p+1) opens window p+1
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int f = 0; f < FW; ++f) vm[f][p] = make_uint2(__float_as_uint(acc[f][p][0]), __float_as_uint(acc[f][p][1]));
        }
        __syncthreads();                                                // every wave is done with input rows 2r, 2r+1 (and the tile)
        if (r + 1 < oh) {
#pragma unroll
            for (int i = 0; i < NQ; ++i) { const int q = i * THREADS + tid; commit_quad(2 * r + 7 + (q >= 512), q & 511, st[i]); }
        }
        __syncthreads();
    }
}

// Round 6: the same walk for the (hi, lo) precisions (bf16x3, f16mx, f16mx4: the backbone on pairs of bf16).  Until now those modes ran
// the exact fp32 stem (v_mfma_f32_32x32x2_f32, 75 TFLOP/s) and a separate pooling launch that split the maxima into pairs: 5.2 ms per
// 256 frames of 512 x 512 against 0.8 for the bf16 kernel above.  Here the stem is three bf16 products like every other conv of those
// modes -- w_hi x (x_hi + x_lo): the eleven k-steps of the kernel above on the hi weights; w_lo x x_hi: six more k-steps whose four
// lane groups read four hi chunks -- the running maximum of the pooling window is fp32 (the max itself is exact), the window leaves
// through an fp32 LDS tile, and the pooled pixel is stored as (hi, lo) pairs in the layout stem_pool_split_kernel writes (32 hi then
// 32 lo per 64-slot group).  Per-layer error of the three-product form: 4e-6 of the output RMS, the class of every other
// backbone conv of these modes.  BOD_STEM_POOL_FUSED=0 or a traced / training handle: the fp32 stem and the pooling launch as before.
constexpr int SB_WROW_LO = 200;                     // uint16 per lo-weight row: 24 chunks x 8 + 8 pad (400 B rows: 16-byte aligned reads)
constexpr int SFS_LDS_BYTES = SF_RING * 2 * SR_ROWE * 2 + 256 * 256;      // ring + fp32 tile [256 px][64 ch]
static_assert(64 * SB_WROW * 2 + 64 * SB_WROW_LO * 2 <= 256 * 256, "both weight tables live in the tile until the loop starts");

__global__ __launch_bounds__(512, 1) void stem_pool_fused_split_kernel(const float* __restrict__ img, const float* __restrict__ w,
                                                                       const float* __restrict__ bias, uint16_t* __restrict__ pooled,
                                                                       int B, int H, int W, int oh, int ow, int ph, int pw, int pool_pitch,
                                                                       int pool_plane) {
    extern __shared__ __attribute__((aligned(16))) uint16_t sf_smem[];
    uint16_t* const ring = sf_smem;
    char* const tile = reinterpret_cast<char*>(sf_smem + SF_RING * 2 * SR_ROWE);      // [256 px][256 B], 16-byte chunks swizzled by the pixel
    uint16_t (*wl)[SB_WROW] = reinterpret_cast<uint16_t (*)[SB_WROW]>(tile);
    uint16_t (*wlo)[SB_WROW_LO] = reinterpret_cast<uint16_t (*)[SB_WROW_LO]>(tile + 64 * SB_WROW * 2);
    constexpr int THREADS = 512, FW = 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pxq = wave & 3, chh = wave >> 2;
    const int li = lane & 15, lq = lane >> 4;
    for (int i = tid; i < 64 * SB_WROW_LO; i += THREADS) {
        const int co = i / SB_WROW_LO, kp = i % SB_WROW_LO;
        const int c = kp >> 3, t = kp & 7, ky = c / 3, j = (c % 3) * 8 + t;
        const float wv = (c < 21 && j < 21) ? w[(ky * 21 + j) * 64 + co] : 0.f;
        const uint32_t hi = f32_to_bf16_a(wv);
        if (kp < SB_WROW) wl[co][kp] = (uint16_t)hi;
        wlo[co][kp] = (uint16_t)f32_to_bf16_a(wv - bf16_to_f32_a(hi));
    }
    constexpr int ROWQ = SR_ROWF / 4;
    auto pk = [](float lo, float hi) { uint32_t r; asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi)); return r; };
    const int valid = W * 3;
    const float* const im = img + (size_t)blockIdx.x * H * W * 3;
    auto fetch_quad = [&](int ir, int q) {
        const int c = q * 4;
        return (q < ROWQ && c < valid && ir < H) ? *reinterpret_cast<const float4*>(im + (size_t)ir * W * 3 + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    auto commit_quad = [&](int ir, int q, const float4 v) {
        if (q >= ROWQ) return;
        uint16_t* pb = ring + ((ir & (SF_RING - 1)) * 2) * SR_ROWE + q * 4;
        const uint32_t h0 = pk(v.x, v.y), h1 = pk(v.z, v.w);
        const uint32_t l0 = pk(v.x - __uint_as_float(h0 << 16), v.y - __uint_as_float(h0 & 0xFFFF0000u));
        const uint32_t l1 = pk(v.z - __uint_as_float(h1 << 16), v.w - __uint_as_float(h1 & 0xFFFF0000u));
        *reinterpret_cast<uint2*>(pb) = make_uint2(h0, h1);
        *reinterpret_cast<uint2*>(pb + SR_ROWE) = make_uint2(l0, l1);
    };
    for (int ir = 0; ir < 7; ++ir)
        for (int q = tid; q < ROWQ; q += THREADS) commit_quad(ir, q, fetch_quad(ir, q));
    __syncthreads();
    const int role = lq & 1, k1 = lq >> 1;
    stem_bf16x8_t aqr[11][FW], alr[5][FW];
#pragma unroll
    for (int s = 0; s < 11; ++s)
#pragma unroll
        for (int f = 0; f < FW; ++f) aqr[s][f] = *reinterpret_cast<const stem_bf16x8_t*>(&wl[(chh * FW + f) * 16 + li][(2 * s + k1) * 8]);
#pragma unroll
    for (int t = 0; t < 5; ++t)
#pragma unroll
        for (int f = 0; f < FW; ++f) alr[t][f] = *reinterpret_cast<const stem_bf16x8_t*>(&wlo[(chh * FW + f) * 16 + li][(4 * t + lq) * 8]);
    // the last k-step of the first pass has a free slot: chunk 21 (k1 = 1) carries zero weights and reads chunk 20's data, plane `role` --
    // the lane group with role 0 (lq = 2) takes w_lo of chunk 20 there, so the second pass is five k-steps (chunks 0 .. 19), not six
    if (lq == 2) {
#pragma unroll
        for (int f = 0; f < FW; ++f) aqr[10][f] = *reinterpret_cast<const stem_bf16x8_t*>(&wlo[(chh * FW + f) * 16 + li][20 * 8]);
    }
    __syncthreads();                                                    // the tables' LDS becomes the pooling tile
    f32x4_t vm[FW][4];                                                  // running maximum of the open pooling window (fp32)
#pragma unroll
    for (int f = 0; f < FW; ++f)
#pragma unroll
        for (int p = 0; p < 4; ++p) vm[f][p] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    uint16_t* const obase = pooled + (size_t)blockIdx.x * pool_plane * 128;

    for (int r = 0; r < oh; ++r) {
        constexpr int NQ = 1024 / THREADS;
        float4 st[NQ];
#pragma unroll
        for (int i = 0; i < NQ; ++i) { const int q = i * THREADS + tid; st[i] = fetch_quad(2 * r + 7 + (q >= 512), q & 511); }
        f32x4_t acc[FW][4];
#pragma unroll
        for (int f = 0; f < FW; ++f)
#pragma unroll
            for (int p = 0; p < 4; ++p) acc[f][p] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        // w_hi x (x_hi, x_lo): the k-steps of the bf16 kernel
#pragma unroll
        for (int s = 0; s < 11; ++s) {
            const int c = 2 * s + k1;
            const int cc = c < 21 ? c : 20;
            const int ky = cc / 3, j0 = (cc - 3 * ky) * 8;
            const uint16_t* pb = ring + ((((2 * r + ky) & (SF_RING - 1)) * 2) + role) * SR_ROWE + (pxq * 64 + li) * 6 + j0;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                union { uint32_t u[4]; stem_bf16x8_t v; } bq;
                const uint32_t* src = reinterpret_cast<const uint32_t*>(pb + p * 96);
#pragma unroll
                for (int t = 0; t < 4; ++t) bq.u[t] = src[t];
#pragma unroll
                for (int f = 0; f < FW; ++f) acc[f][p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aqr[s][f], bq.v, acc[f][p], 0, 0, 0);
            }
        }
        // w_lo x x_hi: lane group lq reads hi chunk 4t + lq (chunk 20: see aqr[10] above)
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const int cc = 4 * t + lq;
            const int ky = cc / 3, j0 = (cc - 3 * ky) * 8;
            const uint16_t* pb = ring + (((2 * r + ky) & (SF_RING - 1)) * 2) * SR_ROWE + (pxq * 64 + li) * 6 + j0;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                union { uint32_t u[4]; stem_bf16x8_t v; } bq;
                const uint32_t* src = reinterpret_cast<const uint32_t*>(pb + p * 96);
#pragma unroll
                for (int u = 0; u < 4; ++u) bq.u[u] = src[u];
#pragma unroll
                for (int f = 0; f < FW; ++f) acc[f][p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(alr[t][f], bq.v, acc[f][p], 0, 0, 0);
            }
        }
        // bias + ReLU in fp32 (stem_conv_kernel's epilogue), then the window's running maximum
#pragma unroll
        for (int f = 0; f < FW; ++f) {
            const f32x4_t bv = *reinterpret_cast<const f32x4_t*>(bias + (chh * FW + f) * 16 + lq * 4);      // (per row: registers are short here)
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float v = fmaxf(acc[f][p][q] + bv[q], 0.f);
                    vm[f][p][q] = fmaxf(vm[f][p][q], v);
                    acc[f][p][q] = v;                                  // (kept: an odd row opens the next window)
                }
        }
        const bool closes = (r & 1) || r == oh - 1;
        if (closes) {
            const int prow = r >> 1;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int px = pxq * 64 + p * 16 + li;
#pragma unroll
                for (int f = 0; f < FW; ++f)
                    *reinterpret_cast<f32x4_t*>(tile + px * 256 + ((((chh * FW + f) * 4 + lq) ^ (px & 15)) << 4)) = vm[f][p];
            }
            __syncthreads();
            if (prow < ph) {
                // horizontal window as above; a thread = (pooled column, eight channels): maxima of two 16-byte chunks, split into pairs
                for (int i = tid; i < pw * 8; i += THREADS) {
                    const int q = i >> 3, ch = i & 7;
                    float m[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) m[e] = 0.f;
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const int px = 2 * q + kx - 2;
                        if (px < 0 || px >= ow) continue;
                        const f32x4_t v0 = *reinterpret_cast<const f32x4_t*>(tile + px * 256 + (((2 * ch) ^ (px & 15)) << 4));
                        const f32x4_t v1 = *reinterpret_cast<const f32x4_t*>(tile + px * 256 + (((2 * ch + 1) ^ (px & 15)) << 4));
#pragma unroll
                        for (int e = 0; e < 4; ++e) { m[e] = fmaxf(m[e], v0[e]); m[4 + e] = fmaxf(m[4 + e], v1[e]); }
                    }
                    uint32_t hi[4], lo[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        hi[e] = pk(m[2 * e], m[2 * e + 1]);
                        lo[e] = pk(m[2 * e] - __uint_as_float(hi[e] << 16), m[2 * e + 1] - __uint_as_float(hi[e] & 0xFFFF0000u));
                    }
                    const int c = ch * 8, slot = (c >> 5) * 64 + (c & 31);
                    uint16_t* o = obase + ((size_t)(prow + 1) * pool_pitch + (q + 1)) * 128 + slot;
                    *reinterpret_cast<uint4*>(o) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
                    *reinterpret_cast<uint4*>(o + 32) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
                }
            }
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int f = 0; f < FW; ++f) vm[f][p] = acc[f][p];
        }
        __syncthreads();
        if (r + 1 < oh) {
#pragma unroll
            for (int i = 0; i < NQ; ++i) { const int q = i * THREADS + tid; commit_quad(2 * r + 7 + (q >= 512), q & 511, st[i]); }
        }
        __syncthreads();
    }
}

// which fused kernel the pipeline runs: the rule (environment reads) apart from the launch, so that a test can name the form
StemFusedForm stem_pool_fused_form(int split) {
    if (split) return STEM_FUSED_SPLIT;
    // BOD_STEM_WAVES=4: the four-wave form (round 3), A/B aid -- bit-identical pooled plane
    static const bool eight = [] { const char* e = getenv("BOD_STEM_WAVES"); return !e || atoi(e) != 4; }();
    return eight ? STEM_FUSED_8 : STEM_FUSED_4;
}
// the shapes every fused kernel is built for (stem_pool_fused_applies adds the switches and the batch floor)
bool stem_pool_fused_fits(const float* img, int W, int ow) {
    return ow <= SR_SEG && (W & 3) == 0 && (reinterpret_cast<uintptr_t>(img) & 15) == 0;
}

hipError_t launch_stem_pool_fused_form(StemFusedForm form, const float* img, const float* w, const float* bias, void* pooled, int B, int H,
                                       int W, int oh, int ow, int ph, int pw, int pool_pitch, int pool_plane, hipStream_t s) {
    if (!stem_pool_fused_fits(img, W, ow)) return hipErrorInvalidValue;
    static PerDeviceOnce once;
    bool& attr_set = *once.slot();
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(stem_pool_fused_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, SF_LDS_BYTES);
        if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(stem_pool_fused_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, SF_LDS_BYTES);
        if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(stem_pool_fused_split_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, SFS_LDS_BYTES);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    if (form == STEM_FUSED_SPLIT)
        hipLaunchKernelGGL(stem_pool_fused_split_kernel, dim3(B), dim3(512), SFS_LDS_BYTES, s, img, w, bias, reinterpret_cast<uint16_t*>(pooled), B, H, W,
                           oh, ow, ph, pw, pool_pitch, pool_plane);
    else if (form == STEM_FUSED_8)
        hipLaunchKernelGGL(stem_pool_fused_kernel<2>, dim3(B), dim3(512), SF_LDS_BYTES, s, img, w, bias, reinterpret_cast<uint16_t*>(pooled), B, H, W, oh, ow,
                           ph, pw, pool_pitch, pool_plane);
    else
        hipLaunchKernelGGL(stem_pool_fused_kernel<1>, dim3(B), dim3(256), SF_LDS_BYTES, s, img, w, bias, reinterpret_cast<uint16_t*>(pooled), B, H, W, oh, ow,
                           ph, pw, pool_pitch, pool_plane);
    return hipGetLastError();
}
hipError_t launch_stem_pool_fused(const float* img, const float* w, const float* bias, void* pooled, int split, int B, int H, int W, int oh,
                                  int ow, int ph, int pw, int pool_pitch, int pool_plane, hipStream_t s) {
    return launch_stem_pool_fused_form(stem_pool_fused_form(split), img, w, bias, pooled, B, H, W, oh, ow, ph, pw, pool_pitch, pool_plane, s);
}
// the fused kernel's shapes: one 256-pixel segment per stem row, 16-byte aligned rows, enough images to fill the chip's CUs
// (one workgroup per image walks down its frame: with fewer images than CUs part of the chip idles for the whole launch -- measured
//  per N=1 forward at 512x512, tests/tools/planner_sweep.py: 128 frames on 256 CUs 19.02 ms fused vs 18.74 as two launches, 256 frames
//  35.9 vs 36.6 -- so the floor is one image per compute unit of the stream's share; BOD_STEM_POOL_FUSED_MIN_B overrides it)
bool stem_pool_fused_applies(const float* img, int B, int W, int ow, int n_cu) {
    static const bool on = [] { const char* e = getenv("BOD_STEM_POOL_FUSED"); return !e || atoi(e) != 0; }();
    static const int min_b = [] { const char* e = getenv("BOD_STEM_POOL_FUSED_MIN_B"); return e ? atoi(e) : 0; }();
    return on && stem_pool_fused_fits(img, W, ow) && B >= (min_b > 0 ? min_b : (n_cu > 0 ? n_cu : 256));
}

// which stem kernel the pipeline runs (the rule apart from the launch, as above)
bool stem_conv_row_fits(const float* img, int W) {                                      // (16-byte row loads: rows of W*3 floats from a 16-byte aligned base)
    return (W & 3) == 0 && (reinterpret_cast<uintptr_t>(img) & 15) == 0;
}
StemConvForm stem_conv_form(const float* img, int out_f32, int W) {
    if (out_f32) return STEM_CONV_F32;
    static const bool old_stem = getenv("BOD_STEM_SEG64") && atoi(getenv("BOD_STEM_SEG64")) == 1;   // A/B aid: the 64-pixel-task kernel (bit-identical outputs)
    return old_stem || !stem_conv_row_fits(img, W) ? STEM_CONV_SEG64 : STEM_CONV_ROW;
}

hipError_t launch_stem_conv_form(StemConvForm form, const float* img, const float* w, const float* bias, void* out,
                                 int B, int H, int W, int oh, int ow, hipStream_t s) {
    const int segs = (ow + ST_SEG - 1) / ST_SEG;
    const int ntasks = B * oh * segs;
    const int grid = ntasks < 1024 ? ntasks : 1024;
    if (form == STEM_CONV_F32) hipLaunchKernelGGL(stem_conv_kernel, dim3(grid), dim3(256), 0, s, img, w, bias, reinterpret_cast<float*>(out), B, H, W, oh, ow);
    else if (form == STEM_CONV_SEG64)
        hipLaunchKernelGGL(stem_conv_bf16_kernel, dim3(ntasks < 768 ? ntasks : 768), dim3(256), 0, s, img, w, bias,
                           reinterpret_cast<uint16_t*>(out), B, H, W, oh, ow);
    else {
        if (!stem_conv_row_fits(img, W)) return hipErrorInvalidValue;
        static PerDeviceOnce once;
        bool& attr_set = *once.slot();
        if (!attr_set) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(stem_conv_bf16_row_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, SR_LDS_TOTAL);
            if (e != hipSuccess) return e;
            attr_set = true;
        }
        const int rtasks = B * oh * ((ow + SR_SEG - 1) / SR_SEG);
        hipLaunchKernelGGL(stem_conv_bf16_row_kernel, dim3(rtasks < 256 ? rtasks : 256), dim3(256), SR_LDS_TOTAL, s, img, w, bias,
                           reinterpret_cast<uint16_t*>(out), B, H, W, oh, ow);
    }
    return hipGetLastError();
}
hipError_t launch_stem_conv(const float* img, const float* w, const float* bias, void* out, int out_f32,
                            int B, int H, int W, int oh, int ow, hipStream_t s) {
    return launch_stem_conv_form(stem_conv_form(img, out_f32, W), img, w, bias, out, B, H, W, oh, ow, s);
}

// fp32 variant of the pooling kernel below (thread = output pixel x 4-channel group)
__global__ __launch_bounds__(256) void stem_pool_f32_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                            int B, int ih, int iw, int oh, int ow, int out_pitch,
                                                            int out_plane) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    const int total = B * oh * ow * 16;
    if (gid >= total) return;
    const int cg = gid & 15;
    int p = gid >> 4;
    const int ox = p % ow; p /= ow;
    const int oy = p % oh;
    const int b = p / oh;
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * oy + ky - 1;
        if (iy < 0 || iy >= ih) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = 2 * ox + kx - 2;
            if (ix < 0 || ix >= iw) continue;
            const float4 v = *reinterpret_cast<const float4*>(in + (((size_t)b * ih + iy) * iw + ix) * 64 + cg * 4);
            m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
        }
    }
    const size_t opix = (size_t)b * out_plane + (size_t)(oy + 1) * out_pitch + (ox + 1);
    *reinterpret_cast<float4*>(out + opix * 64 + cg * 4) = m;
}

// bf16x3 precision: fp32 stem output in, (hi, lo) bf16 pairs out -- 32 hi then 32 lo per 64-slot group of the 128-slot
// pixel (conv_igemm.hip); the max itself is exact
__global__ __launch_bounds__(256) void stem_pool_split_kernel(const float* __restrict__ in, uint16_t* __restrict__ out,
                                                              int B, int ih, int iw, int oh, int ow, int out_pitch, int out_plane) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    const int total = B * oh * ow * 16;
    if (gid >= total) return;
    const int cg = gid & 15;
    int p = gid >> 4;
    const int ox = p % ow; p /= ow;
    const int oy = p % oh;
    const int b = p / oh;
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * oy + ky - 1;
        if (iy < 0 || iy >= ih) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = 2 * ox + kx - 2;
            if (ix < 0 || ix >= iw) continue;
            const float4 v = *reinterpret_cast<const float4*>(in + (((size_t)b * ih + iy) * iw + ix) * 64 + cg * 4);
            m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
        }
    }
    const float v[4] = {m.x, m.y, m.z, m.w};
    uint32_t hi[4], lo[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { hi[q] = f32_to_bf16_a(v[q]); lo[q] = f32_to_bf16_a(v[q] - bf16_to_f32_a(hi[q])); }
    const size_t opix = (size_t)b * out_plane + (size_t)(oy + 1) * out_pitch + (ox + 1);
    const int c = cg * 4, slot = (c >> 5) * 64 + (c & 31);
    uint16_t* o = out + opix * 128 + slot;
    *reinterpret_cast<uint2*>(o) = make_uint2(hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16));
    *reinterpret_cast<uint2*>(o + 32) = make_uint2(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16));
}

// thread = (output pixel, 8-channel group); 16-byte loads/stores. Pads are zeros: inputs are
// post-ReLU (>= 0) so a zero pad value is what ZeroPadding2D + max produces.
__global__ __launch_bounds__(256) void stem_pool_kernel(const uint16_t* __restrict__ in,
                                                        uint16_t* __restrict__ out, int B, int ih,
                                                        int iw, int oh, int ow, int out_pitch,
                                                        int out_plane) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    const int total = B * oh * ow * 8;
    if (gid >= total) return;
    const int cg = gid & 7;
    int p = gid >> 3;
    const int ox = p % ow; p /= ow;
    const int oy = p % oh;
    const int b = p / oh;
    float m[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) m[q] = 0.f;
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * oy + ky - 1;
        if (iy < 0 || iy >= ih) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = 2 * ox + kx - 2;
            if (ix < 0 || ix >= iw) continue;
            const uint4 v = *reinterpret_cast<const uint4*>(in + (((size_t)b * ih + iy) * iw + ix) * 64 + cg * 8);
            const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                m[2 * q] = fmaxf(m[2 * q], bf16_to_f32_a(u[q] & 0xFFFFu));
                m[2 * q + 1] = fmaxf(m[2 * q + 1], bf16_to_f32_a(u[q] >> 16));
            }
        }
    }
    uint4 o;
    o.x = f32_to_bf16_a(m[0]) | (f32_to_bf16_a(m[1]) << 16);
    o.y = f32_to_bf16_a(m[2]) | (f32_to_bf16_a(m[3]) << 16);
    o.z = f32_to_bf16_a(m[4]) | (f32_to_bf16_a(m[5]) << 16);
    o.w = f32_to_bf16_a(m[6]) | (f32_to_bf16_a(m[7]) << 16);
    const size_t opix = (size_t)b * out_plane + (size_t)(oy + 1) * out_pitch + (ox + 1);
    *reinterpret_cast<uint4*>(out + opix * 64 + cg * 8) = o;
}

hipError_t launch_stem_pool(const void* in, void* out, int mode, int B, int ih, int iw, int oh, int ow,
                            int out_pitch, int out_plane, hipStream_t s) {
    if (mode == 2) {
        const int total = B * oh * ow * 16;
        hipLaunchKernelGGL(stem_pool_split_kernel, dim3((total + 255) / 256), dim3(256), 0, s,
                           reinterpret_cast<const float*>(in), reinterpret_cast<uint16_t*>(out), B, ih, iw, oh, ow,
                           out_pitch, out_plane);
        return hipGetLastError();
    }
    if (mode == 1) {
        const int total = B * oh * ow * 16;
        hipLaunchKernelGGL(stem_pool_f32_kernel, dim3((total + 255) / 256), dim3(256), 0, s,
                           reinterpret_cast<const float*>(in), reinterpret_cast<float*>(out), B, ih, iw, oh, ow,
                           out_pitch, out_plane);
        return hipGetLastError();
    }
    const int total = B * oh * ow * 8;
    hipLaunchKernelGGL(stem_pool_kernel, dim3((total + 255) / 256), dim3(256), 0, s,
                       reinterpret_cast<const uint16_t*>(in), reinterpret_cast<uint16_t*>(out), B, ih,
                       iw, oh, ow, out_pitch, out_plane);
    return hipGetLastError();
}

// Device half of the JPEG decoder: what follows the host's Huffman decoding (jpeg_entropy.h).
//   jpeg_idct_kernel    dequantisation + libjpeg's "islow" 8x8 inverse DCT (jidctint.c) -> each component's MCU-padded uint8 plane
//   jpeg_color_kernel   libjpeg's "fancy" chroma upsampling (jdsample.c) + YCbCr -> RGB (jdcolor.c) -> packed uint8 RGB frames, the
//                       buffer preprocess_ragged_kernel / preprocess_augment_kernel read
// Integer arithmetic only; bit-equal to libjpeg(-turbo)'s default decode for encoder-made streams.  All addressing comes from the
// host-validated JpegFrame table: no address depends on a coefficient or a sample, so a hostile stream cannot move an access.
// Products and sums are formed in uint32 (two's complement, wrap-around defined) and read back as int32.
#include "jpeg_dct.h"
#include "kernels.h"

namespace {

constexpr int IDCT_THREADS = 256;                 // 8 lanes per block: 32 blocks per workgroup, 8 per wave
constexpr int IDCT_PITCH = 9;                     // int32 per row of a block's LDS tile (8 + 1: the column reads spread over the banks)
constexpr int COLOR_THREADS = 256;                // one thread per 4 horizontally adjacent pixels

__global__ __launch_bounds__(IDCT_THREADS) void jpeg_idct_kernel(JpegArgs a) {
    __shared__ int32_t tile[IDCT_THREADS / 8][8 * IDCT_PITCH];
    const int t = threadIdx.x & 7, slot = threadIdx.x >> 3;
    const JpegFrame& fr = a.frames[blockIdx.x / a.idct_wgs_per_frame];          // (grid = n * idct_wgs_per_frame: inside the table)
    int64_t l = (int64_t)(blockIdx.x % a.idct_wgs_per_frame) * (IDCT_THREADS / 8) + slot;
    int64_t frame_blocks = 0;
    for (int c = 0; c < fr.components; ++c) frame_blocks += (int64_t)fr.bw[c] * fr.bh[c];
    const bool live = l < frame_blocks;
    int32_t* ws = tile[slot];
    uint32_t x[8];
    uint8_t* out = nullptr;
    if (live) {
        int c = 0;
        for (; c < fr.components - 1; ++c) {
            const int64_t nb = (int64_t)fr.bw[c] * fr.bh[c];
            if (l < nb) break;
            l -= nb;
        }
        // lane t: row t of the block, 16 bytes of coefficients and 16 of the table
        const int4 cv = *reinterpret_cast<const int4*>(a.coefs + fr.coef_off[c] + l * 64 + t * 8);
        const int4 qv = *reinterpret_cast<const int4*>(&fr.quant[c][t * 8]);
        const int32_t cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ws[t * IDCT_PITCH + 2 * j] = (int32_t)((uint32_t)(int32_t)(int16_t)(cw[j] & 0xFFFF) * (uint32_t)(qw[j] & 0xFFFF));
            ws[t * IDCT_PITCH + 2 * j + 1] = (int32_t)((uint32_t)(cw[j] >> 16) * ((uint32_t)qw[j] >> 16));
        }
        const int64_t brow = l / fr.bw[c], bcol = l % fr.bw[c];
        out = a.planes + fr.plane_off[c] + (brow * 8 + t) * ((int64_t)fr.bw[c] * 8) + bcol * 8;
    }
    __syncthreads();
    if (live) {                                   // pass 1: column t
#pragma unroll
        for (int r = 0; r < 8; ++r) x[r] = (uint32_t)ws[r * IDCT_PITCH + t];
        jpeg_idct_1d(x);
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[r * IDCT_PITCH + t] = jpeg_descale(x[r], 11);
    }
    __syncthreads();
    if (live) {                                   // pass 2: row t
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = (uint32_t)ws[t * IDCT_PITCH + j];
        jpeg_idct_1d(x);
        uint32_t w[2] = {0, 0};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int32_t v = min(max(jpeg_descale(x[j], 18) + 128, 0), 255);
            w[j >> 2] |= (uint32_t)v << (8 * (j & 3));
        }
        *reinterpret_cast<uint2*>(out) = make_uint2(w[0], w[1]);
    }
}

// The chroma samples of output pixels x0 .. x0 + 3 (x0 a multiple of 4) of row y: jdsample.c's fancy upsampling, plain replication when
// the chroma plane is <= 2 wide.  Neighbour indices are clamped to the plane, which IS libjpeg's rule for the first and the last output
// column ((3 s + s + 1) >> 2 = s = (3 s + s + 2) >> 2;  (3 cs + cs + 8 or 7) >> 4 = (4 cs + 8 or 7) >> 4), and keeps the reads of a
// ragged last group inside it.
__device__ __forceinline__ void chroma_row4(const uint8_t* pl, int64_t pitch, int cw, int ch, int hs, int vs, int x0, int y, int out[4]) {
    if (hs == 1) {                                // full resolution: 4 aligned bytes, inside the MCU-padded row
        const uint32_t v = *reinterpret_cast<const uint32_t*>(pl + y * pitch + x0);
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] = (int)(v >> (8 * k) & 255);
        return;
    }
    const int i0 = x0 >> 1;
    const int r = vs == 2 ? y >> 1 : y;
    const uint8_t* in0 = pl + r * pitch;
    int j[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) j[k] = min(max(i0 - 1 + k, 0), cw - 1);
    if (cw <= 2) {
        out[0] = out[1] = in0[j[1]];
        out[2] = out[3] = in0[j[2]];
        return;
    }
    int s[4];
    if (vs == 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = in0[j[k]];
        out[0] = (3 * s[1] + s[0] + 1) >> 2; out[1] = (3 * s[1] + s[2] + 2) >> 2;
        out[2] = (3 * s[2] + s[1] + 1) >> 2; out[3] = (3 * s[2] + s[3] + 2) >> 2;
        return;
    }
    const int r1 = min(max((y & 1) ? r + 1 : r - 1, 0), ch - 1);
    const uint8_t* in1 = pl + r1 * pitch;
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = 3 * in0[j[k]] + in1[j[k]];
    out[0] = (3 * s[1] + s[0] + 8) >> 4; out[1] = (3 * s[1] + s[2] + 7) >> 4;
    out[2] = (3 * s[2] + s[1] + 8) >> 4; out[3] = (3 * s[2] + s[3] + 7) >> 4;
}

__global__ __launch_bounds__(COLOR_THREADS) void jpeg_color_kernel(JpegArgs a) {
    const JpegFrame& fr = a.frames[blockIdx.x / a.color_wgs_per_frame];         // (grid = n * color_wgs_per_frame: inside the table)
    const int W = fr.width, H = fr.height, hs = fr.h_samp, vs = fr.v_samp;
    const int64_t l = (int64_t)(blockIdx.x % a.color_wgs_per_frame) * COLOR_THREADS + threadIdx.x;
    const int gpr = (W + 3) >> 2;
    if (l >= (int64_t)H * gpr) return;
    const int y = (int)(l / gpr), x0 = (int)(l % gpr) * 4;
    const int npx = min(4, W - x0);
    const uint8_t* py = a.planes + fr.plane_off[0] + (int64_t)y * fr.bw[0] * 8;
    const bool color = fr.components == 3;
    const uint8_t* pcb = a.planes + fr.plane_off[color ? 1 : 0];
    const uint8_t* pcr = a.planes + fr.plane_off[color ? 2 : 0];
    const int64_t cpitch = (int64_t)fr.bw[color ? 1 : 0] * 8;
    const int cw = (W + hs - 1) / hs, ch = (H + vs - 1) / vs;
    const uint32_t y4 = *reinterpret_cast<const uint32_t*>(py + x0);             // 4 aligned bytes, inside the MCU-padded row
    int cb4[4] = {128, 128, 128, 128}, cr4[4] = {128, 128, 128, 128};
    if (color) {
        chroma_row4(pcb, cpitch, cw, ch, hs, vs, x0, y, cb4);
        chroma_row4(pcr, cpitch, cw, ch, hs, vs, x0, y, cr4);
    }
    uint8_t px[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {                 // (pixels past the frame's edge are computed from in-plane samples and not stored)
        const int Y = (int)(y4 >> (8 * k) & 255), cb = cb4[k] - 128, cr = cr4[k] - 128;
        int R = Y, G = Y, B = Y;
        if (color) jpeg_ycc_to_rgb(Y, cb, cr, R, G, B);
        px[3 * k] = (uint8_t)R; px[3 * k + 1] = (uint8_t)G; px[3 * k + 2] = (uint8_t)B;
    }
    uint8_t* dst = a.rgb + fr.rgb_off + ((int64_t)y * W + x0) * 3;
    if (npx == 4 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
        uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
        for (int j = 0; j < 3; ++j)
            d32[j] = (uint32_t)px[4 * j] | (uint32_t)px[4 * j + 1] << 8 | (uint32_t)px[4 * j + 2] << 16 | (uint32_t)px[4 * j + 3] << 24;
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j)
            if (j < 3 * npx) dst[j] = px[j];
    }
}

}  // namespace

hipError_t launch_jpeg_idct(const JpegArgs& a, hipStream_t s) {
    if (a.n <= 0 || a.idct_wgs_per_frame <= 0) return hipSuccess;
    const int64_t grid = (int64_t)a.n * a.idct_wgs_per_frame;
    if (grid > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)grid), dim3(IDCT_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_jpeg_color(const JpegArgs& a, hipStream_t s) {
    if (a.n <= 0 || a.color_wgs_per_frame <= 0) return hipSuccess;
    const int64_t grid = (int64_t)a.n * a.color_wgs_per_frame;
    if (grid > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)grid), dim3(COLOR_THREADS), 0, s, a);
    return hipGetLastError();
}

// Device half of the PNG decoder: what follows the host's inflate (png_inflate.h).
//   png_unfilter_kernel   reconstructs the filtered scanlines (PNG specification, section 9: None, Sub, Up, Average, Paeth) and writes
//                         packed uint8 RGB frames, the buffer preprocess_ragged_kernel / preprocess_augment_kernel read: RGB as it
//                         is, RGBA without its alpha, gray and gray + alpha with the gray byte three times (PIL's convert('RGB')).
// Integer arithmetic only.  All addressing and every loop bound come from the host-validated PngFrame table, and the host has checked
// every row's filter-type byte to be 0..4: no address and no trip count depends on a pixel.
//
// A pixel needs its left, upper and upper-left neighbours, so a frame is an anti-diagonal wavefront.  One workgroup per frame; thread
// t owns row band0 + t of a band of blockDim.x rows and, at step s, reconstructs chunk s - t (PNG_CHUNK pixels) of its row: left and
// upper-left stay in registers, "up" is the chunk thread t - 1 left in LDS one step earlier (two LDS buffers, alternating by step: one
// barrier per step).  The byte lanes of a pixel are independent under all five filters, so an alpha lane is never reconstructed.
// Bands run in sequence; the first row of a band reads the last row of the previous band from the output, a chunk ahead of its use as
// the filtered bytes are (a row of any width does not fit LDS).  LDS is sized by the launch: 32 bytes per row of a band.
#include "kernels.h"

namespace {

constexpr int PNG_CHUNK = 4;                      // pixels per thread and step

__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);       // (the tie order is the specification's)
}

// The filtered bytes of chunk c of a row (src: behind its filter-type byte), lanes 0 .. nl - 1 of each pixel packed into one word.
// Pixels past the row's end are not read.
__device__ __forceinline__ void load_chunk(const uint8_t* src, int c, int W, int bpp, int nl, uint32_t f[PNG_CHUNK]) {
#pragma unroll
    for (int k = 0; k < PNG_CHUNK; ++k) {
        const int x = c * PNG_CHUNK + k;
        uint32_t v = 0;
        if (x < W) {
            const uint8_t* p = src + (int64_t)x * bpp;
            v = p[0];
            if (nl == 3) v |= (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
        }
        f[k] = v;
    }
}

// The reconstructed pixels of chunk c of the output row `up_row`, lanes 0 .. nl - 1: what the first row of a band behind the first
// takes for "up".  Written by this workgroup before the band's fence and barrier; read past this compute unit's L1.
__device__ __forceinline__ void load_up_chunk(const uint8_t* up_row, int c, int W, int nl, uint32_t up[PNG_CHUNK]) {
#pragma unroll
    for (int k = 0; k < PNG_CHUNK; ++k) {
        const int x = c * PNG_CHUNK + k;
        uint32_t v = 0;
        if (x < W)
            for (int l = 0; l < nl; ++l)
                v |= (uint32_t)__hip_atomic_load(up_row + (int64_t)x * 3 + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) << (8 * l);
        up[k] = v;
    }
}

__global__ __launch_bounds__(PNG_MAX_BAND_ROWS) void png_unfilter_kernel(PngArgs a) {
    extern __shared__ __align__(16) uint32_t up_lds[];                  // [2][blockDim.x][PNG_CHUNK]: 32 bytes per row of a band
    const PngFrame fr = a.frames[blockIdx.x];                           // (grid = n: inside the table; uniform across the workgroup)
    const int H = fr.height, W = fr.width, bpp = fr.channels;
    const int nl = bpp >= 3 ? 3 : 1;                                    // lanes that reach the output
    const int R = (int)blockDim.x, t = (int)threadIdx.x;
    const int64_t stride = 1 + (int64_t)W * bpp;
    const uint8_t* raw = a.raw + fr.raw_off;
    uint8_t* out = a.rgb + fr.rgb_off;                                  // (read back at band boundaries: no __restrict__)
    const int nchunks = (W + PNG_CHUNK - 1) / PNG_CHUNK;
    for (int band0 = 0; band0 < H; band0 += R) {
        const int rows = min(R, H - band0);
        const int row = band0 + t;
        const bool have_row = t < rows;
        const uint8_t* src = raw + (have_row ? (int64_t)row * stride : 0);
        const int ftype = have_row ? src[0] : 0;
        ++src;
        uint8_t* dst_row = out + (int64_t)row * W * 3;
        const uint8_t* up_row = dst_row - (int64_t)W * 3;               // (dereferenced for t == 0 of a band behind the first only)
        const bool up_from_output = t == 0 && row > 0;
        int la[3] = {0, 0, 0}, ul[3] = {0, 0, 0};                       // left and upper-left pixel, per lane
        uint32_t nextf[PNG_CHUNK] = {0, 0, 0, 0};
        uint32_t nextup[PNG_CHUNK] = {0, 0, 0, 0};                      // thread 0: "up" of its next chunk; zeros in the frame's first row
        if (have_row) load_chunk(src, 0, W, bpp, nl, nextf);
        if (up_from_output) load_up_chunk(up_row, 0, W, nl, nextup);
        const int steps = nchunks + rows - 1;                           // uniform: every thread reaches every barrier
        for (int s = 0; s < steps; ++s) {
            const int c = s - t;
            if (have_row && c >= 0 && c < nchunks) {
                uint32_t filt[PNG_CHUNK], up[PNG_CHUNK];
#pragma unroll
                for (int k = 0; k < PNG_CHUNK; ++k) filt[k] = nextf[k];
                if (c + 1 < nchunks) load_chunk(src, c + 1, W, bpp, nl, nextf);   // the next step's bytes, in flight during this one
                if (t > 0) {
                    const uint4 v = *reinterpret_cast<const uint4*>(up_lds + ((size_t)(((s - 1) & 1) * R + t - 1)) * PNG_CHUNK);
                    up[0] = v.x; up[1] = v.y; up[2] = v.z; up[3] = v.w;
                } else {
#pragma unroll
                    for (int k = 0; k < PNG_CHUNK; ++k) up[k] = nextup[k];
                    if (up_from_output && c + 1 < nchunks) load_up_chunk(up_row, c + 1, W, nl, nextup);
                }
                uint32_t cur[PNG_CHUNK];
#pragma unroll
                for (int k = 0; k < PNG_CHUNK; ++k) {
                    // (pixels past the row's end are computed from zeros and not stored)
#pragma unroll
                    for (int l = 0; l < 3; ++l) {
                        if (l >= nl) continue;
                        const int f = (int)(filt[k] >> (8 * l) & 255), b = (int)(up[k] >> (8 * l) & 255);
                        const int av = la[l], cv = ul[l];
                        const int pred = ftype == 0 ? 0 : ftype == 1 ? av : ftype == 2 ? b : ftype == 3 ? (av + b) >> 1 : paeth(av, b, cv);
                        la[l] = (f + pred) & 255;
                        ul[l] = b;
                    }
                    cur[k] = (uint32_t)la[0] | (uint32_t)la[1] << 8 | (uint32_t)la[2] << 16;
                }
                *reinterpret_cast<uint4*>(up_lds + ((size_t)((s & 1) * R + t)) * PNG_CHUNK) = make_uint4(cur[0], cur[1], cur[2], cur[3]);
                uint8_t px[3 * PNG_CHUNK];
#pragma unroll
                for (int k = 0; k < PNG_CHUNK; ++k) {
                    const uint8_t r = (uint8_t)cur[k];
                    px[3 * k] = r;
                    px[3 * k + 1] = nl == 3 ? (uint8_t)(cur[k] >> 8) : r;
                    px[3 * k + 2] = nl == 3 ? (uint8_t)(cur[k] >> 16) : r;
                }
                const int npx = min(PNG_CHUNK, W - c * PNG_CHUNK);
                uint8_t* dst = dst_row + (int64_t)c * PNG_CHUNK * 3;
                if (npx == PNG_CHUNK && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
                    uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
                    for (int j = 0; j < 3; ++j)
                        d32[j] = (uint32_t)px[4 * j] | (uint32_t)px[4 * j + 1] << 8 | (uint32_t)px[4 * j + 2] << 16 | (uint32_t)px[4 * j + 3] << 24;
                } else {
#pragma unroll
                    for (int j = 0; j < 3 * PNG_CHUNK; ++j)
                        if (j < 3 * npx) dst[j] = px[j];
                }
            }
            __syncthreads();
        }
        // the band's last row has to have left this compute unit before the next band's first row reads it
        __threadfence();
        __syncthreads();
    }
}

}  // namespace

hipError_t launch_png_unfilter(const PngArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (a.rows_per_band < 64 || a.rows_per_band > PNG_MAX_BAND_ROWS || a.rows_per_band % 64) return hipErrorInvalidValue;
    const size_t lds = (size_t)2 * a.rows_per_band * PNG_CHUNK * sizeof(uint32_t);
    hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)a.n), dim3((unsigned)a.rows_per_band), lds, s, a);
    return hipGetLastError();
}

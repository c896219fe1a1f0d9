// Rendering on the device (the drawing contract: include/bayesod.h): boxes, labels and 2-sigma corner ellipses
// (OVERLAY) or the jet-coloured spatial-probability map (HEAT) drawn onto packed uint8 RGB frames.
//
// OVERLAY.  The host expands a frame's rows into a flat list of primitives in contract order (ground-truth rings; per detection its
// ring, label box and glyphs; per detection its two ellipses and second ring), each with its bounding rectangle clipped to the frame
// (a primitive that misses the frame is dropped there).  render_bin_kernel runs twice, one thread per 32x32 tile walking its frame's
// rectangles in ascending order: the first pass counts the primitives that meet the tile, render_scan_kernel turns the counts into
// offsets, the second pass writes the indices -- ascending per tile by construction, no atomics, and the list holds exactly the count
// pass's total (the host computes the same total from the rectangles to size it: nothing is ever dropped for capacity).
// render_paint_kernel is one workgroup per tile: a thread keeps 4 horizontally adjacent pixels in registers while the workgroup
// walks the tile's list, 64 primitive records at a time through LDS; a record is workgroup-uniform, so the branch on its kind is too.
// The ellipse coverage is fp32 with the operation order of the header (the file is built with -ffp-contract=off; divide and sqrtf
// are hipcc's correctly rounded ones): tests/render_reference.py restates it in NumPy and the bytes are equal.
// HEAT.  Per frame, chunks of detections: pdq_kernels.hip makes the chunk's box heatmaps on the device (the code bod_pdq_frames runs),
// render_heat_compose_kernel folds them into the uint8 index plane in ascending order, render_heat_colour_kernel blends the ramp.
// All addressing comes from host-built records: no address depends on a pixel value.
#include "../../include/bayesod.h"
#include "host_call.h"
#include "kernels.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "render_font.h"

namespace {

constexpr int TILE = 32;
constexpr int PAINT_THREADS = 256;                // thread t: row t / 8 of the tile, pixels 4 * (t % 8) .. + 3
constexpr int PRIM_CHUNK = 64;                    // primitive records staged in LDS at a time
constexpr int BIN_THREADS = 256;
constexpr int SCAN_THREADS = 256;
constexpr int64_t COORD_CLAMP = 1 << 20;          // box coordinates beyond it draw as if at it: frames are at most 65535 wide / high
constexpr int EXTENT_CAP = 4096;
constexpr size_t HEAT_CHUNK_BYTES = (size_t)64 << 20;
constexpr int HEAT_CHUNK_ROWS = 4096;

enum { PRIM_RING = 0, PRIM_FILL = 1, PRIM_GLYPH = 2, PRIM_ELLIPSE = 3 };

struct RenderPrim {                               // 48 B
    int32_t kind;
    int32_t rx0, ry0, rx1, ry1;                   // bounding rectangle inside the frame, inclusive: nothing is drawn outside it
    int32_t p[6];                                 // RING: x0 y0 x1 y1 a b; GLYPH: x y, bits 0..31, bits 32..34 (bit 5r + j: row r, column j);
                                                  // ELLIPSE: centre x y, then a b c det as fp32 bit patterns
    uint32_t colour;                              // R | G << 8 | B << 16
};
static_assert(sizeof(RenderPrim) == 48, "RenderPrim layout");

struct RenderFrame {                              // 32 B
    int64_t offset;                               // first byte of the frame in the packed buffers
    int32_t h, w;
    int32_t prim_off, prim_n;                     // its primitives, in contract order
    int32_t tile_off, tiles_x;                    // its tiles in the batch's tile numbering, row-major
};
static_assert(sizeof(RenderFrame) == 32, "RenderFrame layout");

struct RenderArgs {
    const RenderFrame* frames;
    const int32_t* tile_frame;                    // [n_tiles]: the frame a tile belongs to
    const RenderPrim* prims;
    const int4* rects;                            // [n_prims]: rx0 ry0 rx1 ry1 again, what the binning reads
    uint32_t* counts;                             // [n_tiles]
    uint32_t* offsets;                            // [n_tiles + 1]: exclusive scan of counts
    int32_t* list;                                // [list_cap]: per tile the ascending frame-local primitive indices
    const uint8_t* src;
    uint8_t* dst;
    uint32_t list_cap;
    int32_t n_tiles;
    float sqrt_r2, half_width;                    // sqrtf(r2), 0.5f * t + 0.5f
};

// 4 consecutive pixels (npx of them inside the row) as 12 byte values
__device__ __forceinline__ void load_group(const uint8_t* p, int npx, int v[12]) {
    if (npx == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        const uint32_t* p32 = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const uint32_t u = p32[j];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[4 * j + k] = (int)((u >> (8 * k)) & 255u);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) v[j] = j < 3 * npx ? (int)p[j] : 0;
    }
}
__device__ __forceinline__ void store_group(uint8_t* p, int npx, const int v[12]) {
    if (npx == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        uint32_t* p32 = reinterpret_cast<uint32_t*>(p);
#pragma unroll
        for (int j = 0; j < 3; ++j)
            p32[j] = (uint32_t)v[4 * j] | (uint32_t)v[4 * j + 1] << 8 | (uint32_t)v[4 * j + 2] << 16 | (uint32_t)v[4 * j + 3] << 24;
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j)
            if (j < 3 * npx) p[j] = (uint8_t)v[j];
    }
}

// count (fill == 0) or write (fill != 0) the primitives of the tile's frame whose rectangle meets the tile, in ascending order
__global__ __launch_bounds__(BIN_THREADS) void render_bin_kernel(RenderArgs a, int fill) {
    const int tile = blockIdx.x * BIN_THREADS + threadIdx.x;
    if (tile >= a.n_tiles) return;
    const RenderFrame fr = a.frames[a.tile_frame[tile]];
    const int l = tile - fr.tile_off;
    const int tx0 = (l % fr.tiles_x) * TILE, ty0 = (l / fr.tiles_x) * TILE;
    const uint32_t pos = fill ? a.offsets[tile] : 0u;
    uint32_t cnt = 0;
    for (int i = 0; i < fr.prim_n; ++i) {
        const int4 r = a.rects[fr.prim_off + i];
        if (r.x > tx0 + TILE - 1 || r.z < tx0 || r.y > ty0 + TILE - 1 || r.w < ty0) continue;
        if (fill && pos + cnt < a.list_cap) a.list[pos + cnt] = i;
        ++cnt;
    }
    if (!fill) a.counts[tile] = cnt;
}

// offsets = exclusive scan of counts, offsets[n_tiles] = the total: one workgroup, a contiguous run of tiles per thread
__global__ __launch_bounds__(SCAN_THREADS) void render_scan_kernel(RenderArgs a) {
    __shared__ uint32_t part[SCAN_THREADS];
    const int n = a.n_tiles, per = (n + SCAN_THREADS - 1) / SCAN_THREADS;
    const int lo = min((int)threadIdx.x * per, n), hi = min(lo + per, n);
    uint32_t s = 0;
    for (int i = lo; i < hi; ++i) s += a.counts[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int t = 0; t < SCAN_THREADS; ++t) { const uint32_t v = part[t]; part[t] = run; run += v; }
        a.offsets[n] = run;
    }
    __syncthreads();
    uint32_t run = part[threadIdx.x];
    for (int i = lo; i < hi; ++i) { a.offsets[i] = run; run += a.counts[i]; }
}

__device__ __forceinline__ void blend(int v[3], uint32_t colour, int alpha) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (v[c] * (256 - alpha) + (int)((colour >> (8 * c)) & 255u) * alpha + 128) >> 8;
}

// the header's coverage of the contour at offset (dx, dy) from the ellipse's centre, 0..256
__device__ __forceinline__ int ellipse_alpha(float a, float b, float c, float det, float sqrt_r2, float half_width, int idx, int idy) {
    const float dx = (float)idx, dy = (float)idy;
    const float gx = __fsub_rn(__fmul_rn(c, dx), __fmul_rn(b, dy)) / det;      // (hipcc's fp32 divide and sqrtf are correctly rounded)
    const float gy = __fsub_rn(__fmul_rn(a, dy), __fmul_rn(b, dx)) / det;
    const float q = __fadd_rn(__fmul_rn(dx, gx), __fmul_rn(dy, gy));
    if (!(q > 0.0f)) return 0;
    const float m = sqrtf(q);
    const float g = sqrtf(__fadd_rn(__fmul_rn(gx, gx), __fmul_rn(gy, gy)));
    const float dist = __fmul_rn(fabsf(__fsub_rn(m, sqrt_r2)), m) / g;
    const float cov = fminf(fmaxf(__fsub_rn(half_width, dist), 0.0f), 1.0f);
    return (int)__fmul_rn(cov, 256.0f);
}

__global__ __launch_bounds__(PAINT_THREADS) void render_paint_kernel(RenderArgs a) {
    __shared__ RenderPrim sp[PRIM_CHUNK];
    const int tile = blockIdx.x;                  // (grid = n_tiles)
    const RenderFrame fr = a.frames[a.tile_frame[tile]];
    const int l = tile - fr.tile_off;
    const int y = (l / fr.tiles_x) * TILE + (int)(threadIdx.x >> 3), x0 = (l % fr.tiles_x) * TILE + (int)(threadIdx.x & 7) * 4;
    const bool live = y < fr.h && x0 < fr.w;
    const int npx = live ? min(4, fr.w - x0) : 0;
    const int64_t at = fr.offset + ((int64_t)y * fr.w + x0) * 3;
    int v[12];
    if (live) load_group(a.src + at, npx, v);
    const uint32_t beg = a.offsets[tile], end = min(a.offsets[tile + 1], a.list_cap);
    for (uint32_t c0 = beg; c0 < end; c0 += PRIM_CHUNK) {
        const int m = (int)min((uint32_t)PRIM_CHUNK, end - c0);
        __syncthreads();                          // the previous chunk has been read
        for (int i = threadIdx.x; i < m * 12; i += PAINT_THREADS) {
            const int r = i / 12, wd = i % 12;
            const int idx = min(max(a.list[c0 + r], 0), fr.prim_n - 1);        // (the fill pass wrote 0 .. prim_n - 1: the clamp is a guard)
            reinterpret_cast<uint32_t*>(sp)[i] = reinterpret_cast<const uint32_t*>(a.prims + fr.prim_off + idx)[wd];
        }
        __syncthreads();
        if (!live) continue;
        for (int k = 0; k < m; ++k) {
            const RenderPrim& p = sp[k];
            if (y < p.ry0 || y > p.ry1 || x0 > p.rx1 || x0 + 3 < p.rx0) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = x0 + j;
                if (x < p.rx0 || x > p.rx1) continue;                           // (rx1 < w: pixels past the row's end never pass)
                int alpha = 256;
                if (p.kind == PRIM_RING) {
                    const int bb = p.p[5];
                    if (x >= p.p[0] + bb && x <= p.p[2] - bb && y >= p.p[1] + bb && y <= p.p[3] - bb) alpha = 0;
                } else if (p.kind == PRIM_GLYPH) {
                    const int bit = (y - p.p[1]) * 5 + (x - p.p[0]);             // 0..34 inside the rectangle
                    alpha = ((bit < 32 ? (uint32_t)p.p[2] >> bit : (uint32_t)p.p[3] >> (bit - 32)) & 1u) ? 256 : 0;
                } else if (p.kind == PRIM_ELLIPSE) {
                    alpha = ellipse_alpha(__int_as_float(p.p[2]), __int_as_float(p.p[3]), __int_as_float(p.p[4]), __int_as_float(p.p[5]),
                                          a.sqrt_r2, a.half_width, x - p.p[0], y - p.p[1]);
                }
                if (alpha) blend(v + 3 * j, p.colour, alpha);
            }
        }
    }
    if (live) store_group(a.dst + at, npx, v);
}

// HEAT: fold the heatmaps of m detections, in ascending order, into the index plane
__global__ __launch_bounds__(256) void render_heat_compose_kernel(const float* __restrict__ heat, int m, int64_t npix, uint8_t* __restrict__ index) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    int v = index[p];
    for (int d = 0; d < m; ++d) {
        const float h = heat[(int64_t)d * npix + p];
        if (h != 0.0f) v = (int)__fmul_rn(h, 255.0f);                           // (h <= 1: at most 255)
    }
    index[p] = (uint8_t)v;
}

__device__ __forceinline__ int clip255(int v) { return min(max(v, 0), 255); }

// HEAT: out = (26 * v + 230 * ramp(index) + 128) >> 8, a thread per 4 pixels
__global__ __launch_bounds__(256) void render_heat_colour_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ index, int64_t npix,
                                                                uint8_t* __restrict__ dst) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g * 4 >= npix) return;
    const int npx = (int)min((int64_t)4, npix - g * 4);
    int v[12];
    load_group(src + g * 12, npx, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j >= npx) continue;
        const int x = 4 * (int)index[g * 4 + j];
        const int ramp[3] = {clip255(min(x - 382, 1147 - x)), clip255(min(x - 127, 892 - x)), clip255(min(x + 128, 637 - x))};
#pragma unroll
        for (int c = 0; c < 3; ++c) v[3 * j + c] = (26 * v[3 * j + c] + 230 * ramp[c] + 128) >> 8;
    }
    store_group(dst + g * 12, npx, v);
}

#define RENDER_HIP(expr)                                                                                               \
    do {                                                                                                               \
        hipError_t _e = (expr);                                                                                        \
        if (_e != hipSuccess) return err.fail(BOD_ERR_HIP, "%s: %s failed: %s", WHO, #expr, hipGetErrorString(_e)); \
    } while (0)

const char* const WHO = "bod_render_frames_u8";

bod_render_options options_or_default(const bod_render_options* opt) {
    if (opt) return *opt;
    bod_render_options o{};
    o.view = BOD_RENDER_OVERLAY; o.line_width = 2; o.labels = 1; o.r2 = 6.180074f;
    return o;
}

inline uint32_t pack_colour(const uint8_t* c) { return (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16; }
inline int32_t clamp_coord(int64_t v) { return (int32_t)std::max(-COORD_CLAMP, std::min(v, COORD_CLAMP)); }
inline int32_t float_bits(float f) { int32_t u; memcpy(&u, &f, 4); return u; }

// one frame's primitives in contract order
struct PrimBuilder {
    std::vector<RenderPrim>& prims;
    int h, w;
    int64_t list_total = 0;                       // sum over the primitives of the tiles their rectangle meets
    // clips the rectangle to the frame; false when nothing is left
    bool add(RenderPrim p, int64_t x0, int64_t y0, int64_t x1, int64_t y1) {
        x0 = std::max<int64_t>(x0, 0); y0 = std::max<int64_t>(y0, 0);
        x1 = std::min<int64_t>(x1, w - 1); y1 = std::min<int64_t>(y1, h - 1);
        if (x1 < x0 || y1 < y0) return false;
        p.rx0 = (int32_t)x0; p.ry0 = (int32_t)y0; p.rx1 = (int32_t)x1; p.ry1 = (int32_t)y1;
        prims.push_back(p);
        list_total += (int64_t)(p.rx1 / TILE - p.rx0 / TILE + 1) * (p.ry1 / TILE - p.ry0 / TILE + 1);
        return true;
    }
    void ring(const int32_t* b, int width, uint32_t colour) {
        if (b[2] < b[0] || b[3] < b[1]) return;
        const int a = width / 2;
        RenderPrim p{};
        p.kind = PRIM_RING; p.colour = colour;
        for (int k = 0; k < 4; ++k) p.p[k] = clamp_coord(b[k]);
        p.p[4] = a; p.p[5] = (width + 1) / 2;
        add(p, (int64_t)b[0] - a, (int64_t)b[1] - a, (int64_t)b[2] + a, (int64_t)b[3] + a);
    }
    void label(const int32_t* b, const uint8_t* text, uint32_t colour) {
        int L = 0;
        while (L < 16 && text[L] != 0xFF) ++L;
        if (!L) return;
        RenderPrim f{};
        f.kind = PRIM_FILL; f.colour = 0;
        add(f, b[0], b[1], (int64_t)b[0] + 6 * L, (int64_t)b[1] + 8);
        for (int i = 0; i < L; ++i) {
            uint64_t bits = 0;
            for (int r = 0; r < RENDER_FONT_ROWS; ++r)
                for (int j = 0; j < 5; ++j)
                    if ((RENDER_FONT[text[i]][r] >> (4 - j)) & 1) bits |= (uint64_t)1 << (5 * r + j);
            if (!bits) continue;
            const int64_t gx = (int64_t)b[0] + 1 + 6 * i, gy = (int64_t)b[1] + 1;
            RenderPrim g{};
            g.kind = PRIM_GLYPH; g.colour = colour;
            g.p[0] = clamp_coord(gx); g.p[1] = clamp_coord(gy);                  // (a glyph that stays is within 6 pixels of the frame)
            g.p[2] = (int32_t)(uint32_t)bits; g.p[3] = (int32_t)(uint32_t)(bits >> 32);
            add(g, gx, gy, gx + 4, gy + 6);
        }
    }
    // false: the header's validity rule fails, the ellipse is skipped
    bool ellipse(int64_t cx, int64_t cy, const float* cov, const bod_render_options& o, uint32_t colour) {
        const float a = cov[0], b = cov[1], c = cov[3];
        if (!std::isfinite(a) || !std::isfinite(b) || !std::isfinite(c) || !(a > 0.0f) || !(c > 0.0f)) return false;
        const float ac = a * c, bb = b * b, det = ac - bb;
        if (!(det > 0.0f)) return false;
        auto extent = [&](float s) -> int64_t {
            const double e = ceil(1.5 * sqrt((double)o.r2 * (double)s)) + o.line_width + 1;
            return e < (double)EXTENT_CAP ? (int64_t)e : (int64_t)EXTENT_CAP;
        };
        const int64_t ex = extent(a), ey = extent(c);
        RenderPrim p{};
        p.kind = PRIM_ELLIPSE; p.colour = colour;
        p.p[0] = clamp_coord(cx); p.p[1] = clamp_coord(cy);                      // (an ellipse that stays is within 4096 pixels of the frame)
        p.p[2] = float_bits(a); p.p[3] = float_bits(b); p.p[4] = float_bits(c); p.p[5] = float_bits(det);
        add(p, cx - ex, cy - ey, cx + ex, cy + ey);
        return true;
    }
};

bool trace_on() {
    const char* t = getenv("BOD_RENDER_TRACE");
    return t && atoi(t) != 0;
}

int run_overlay(int32_t n, const uint8_t* rgb_in, const int32_t* src_hw, const int32_t* num_det, const int32_t* det_boxes,
                const float* det_corner_covs, const uint8_t* det_colors, const uint8_t* det_text, const int32_t* num_gt,
                const int32_t* gt_boxes, const bod_render_options& o, uint8_t* rgb_out, int32_t* skipped, hipStream_t s, Err& err) {
    std::vector<RenderPrim> prims;
    std::vector<RenderFrame> frames((size_t)n);
    std::vector<int32_t> tile_frame;
    int64_t bytes = 0, n_tiles = 0, list_total = 0, d0 = 0, g0 = 0;
    const uint32_t green = 255u << 8;
    const int second = std::max(o.line_width - 1, 1);
    for (int f = 0; f < n; ++f) {
        const int h = src_hw[2 * f], w = src_hw[2 * f + 1], D = num_det[f], G = num_gt ? num_gt[f] : 0;
        RenderFrame& fr = frames[(size_t)f];
        fr.offset = bytes; fr.h = h; fr.w = w; fr.prim_off = (int32_t)prims.size();
        fr.tile_off = (int32_t)n_tiles; fr.tiles_x = (w + TILE - 1) / TILE;
        PrimBuilder pb{prims, h, w};
        int skip = 0;
        for (int g = 0; g < G; ++g) pb.ring(gt_boxes + 4 * (g0 + g), 1, green);
        for (int d = 0; d < D; ++d) {
            const int32_t* b = det_boxes + 4 * (d0 + d);
            const uint32_t colour = pack_colour(det_colors + 3 * (d0 + d));
            pb.ring(b, 1, colour);
            if (o.labels && det_text) pb.label(b, det_text + 16 * (d0 + d), colour);
        }
        for (int d = 0; d < D; ++d) {
            const int32_t* b = det_boxes + 4 * (d0 + d);
            const float* cv = det_corner_covs + 8 * (d0 + d);
            const uint32_t colour = pack_colour(det_colors + 3 * (d0 + d));
            if (!pb.ellipse(b[0], b[1], cv, o, colour)) ++skip;
            if (!pb.ellipse(b[2], b[3], cv + 4, o, colour)) ++skip;
            pb.ring(b, second, colour);
        }
        if (skipped) skipped[f] = skip;
        const int64_t tiles = (int64_t)fr.tiles_x * ((h + TILE - 1) / TILE);
        fr.prim_n = (int32_t)(prims.size() - (size_t)fr.prim_off);
        tile_frame.insert(tile_frame.end(), (size_t)tiles, f);
        bytes += (int64_t)3 * h * w; n_tiles += tiles; list_total += pb.list_total; d0 += D; g0 += G;
        if (n_tiles > 0x7FFFFFFF / 2 || prims.size() > (size_t)0x7FFFFFFF / 2 || list_total > 0x7FFFFFFF)
            return err.fail(BOD_ERR_INVALID_ARG, "%s: the batch up to frame %d is more than one call covers (%lld tiles, %zu primitives, %lld list entries)",
                            WHO, f, (long long)n_tiles, prims.size(), (long long)list_total);
    }
    std::vector<int4> rects(prims.size());
    for (size_t i = 0; i < prims.size(); ++i) rects[i] = make_int4(prims[i].rx0, prims[i].ry0, prims[i].rx1, prims[i].ry1);

    DevArena arena;
    uint8_t *d_in, *d_out; RenderFrame* d_frames; int32_t* d_tile_frame; RenderPrim* d_prims; int4* d_rects;
    uint32_t *d_counts, *d_offsets; int32_t* d_list;
    RENDER_HIP(arena.alloc(&d_in, (size_t)bytes)); RENDER_HIP(arena.alloc(&d_out, (size_t)bytes));
    RENDER_HIP(arena.alloc(&d_frames, (size_t)n)); RENDER_HIP(arena.alloc(&d_tile_frame, (size_t)n_tiles));
    RENDER_HIP(arena.alloc(&d_prims, prims.size())); RENDER_HIP(arena.alloc(&d_rects, prims.size()));
    RENDER_HIP(arena.alloc(&d_counts, (size_t)n_tiles)); RENDER_HIP(arena.alloc(&d_offsets, (size_t)n_tiles + 1));
    RENDER_HIP(arena.alloc(&d_list, (size_t)list_total));
    RENDER_HIP(hipMemcpyAsync(d_in, rgb_in, (size_t)bytes, hipMemcpyHostToDevice, s));
    RENDER_HIP(hipMemcpyAsync(d_frames, frames.data(), sizeof(RenderFrame) * n, hipMemcpyHostToDevice, s));
    RENDER_HIP(hipMemcpyAsync(d_tile_frame, tile_frame.data(), sizeof(int32_t) * n_tiles, hipMemcpyHostToDevice, s));
    if (!prims.empty()) {
        RENDER_HIP(hipMemcpyAsync(d_prims, prims.data(), sizeof(RenderPrim) * prims.size(), hipMemcpyHostToDevice, s));
        RENDER_HIP(hipMemcpyAsync(d_rects, rects.data(), sizeof(int4) * rects.size(), hipMemcpyHostToDevice, s));
    }
    RenderArgs a{};
    a.frames = d_frames; a.tile_frame = d_tile_frame; a.prims = d_prims; a.rects = d_rects; a.counts = d_counts; a.offsets = d_offsets;
    a.list = d_list; a.src = d_in; a.dst = d_out; a.list_cap = (uint32_t)list_total; a.n_tiles = (int32_t)n_tiles;
    a.sqrt_r2 = sqrtf(o.r2); a.half_width = 0.5f * (float)o.line_width + 0.5f;
    const bool trace = trace_on();
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    if (trace) { for (auto& e : ev) RENDER_HIP(hipEventCreate(&e)); RENDER_HIP(hipEventRecord(ev[0], s)); }
    const unsigned bin_grid = (unsigned)((n_tiles + BIN_THREADS - 1) / BIN_THREADS);
    hipLaunchKernelGGL(render_bin_kernel, dim3(bin_grid), dim3(BIN_THREADS), 0, s, a, 0);
    RENDER_HIP(hipGetLastError());
    hipLaunchKernelGGL(render_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, a);
    RENDER_HIP(hipGetLastError());
    hipLaunchKernelGGL(render_bin_kernel, dim3(bin_grid), dim3(BIN_THREADS), 0, s, a, 1);
    RENDER_HIP(hipGetLastError());
    if (trace) RENDER_HIP(hipEventRecord(ev[1], s));
    hipLaunchKernelGGL(render_paint_kernel, dim3((unsigned)n_tiles), dim3(PAINT_THREADS), 0, s, a);
    RENDER_HIP(hipGetLastError());
    if (trace) RENDER_HIP(hipEventRecord(ev[2], s));
    uint32_t total = 0;
    RENDER_HIP(hipMemcpyAsync(&total, d_offsets + n_tiles, sizeof total, hipMemcpyDeviceToHost, s));
    RENDER_HIP(hipMemcpyAsync(rgb_out, d_out, (size_t)bytes, hipMemcpyDeviceToHost, s));
    RENDER_HIP(hipStreamSynchronize(s));
    if (trace) {
        float bin_ms = 0.f, paint_ms = 0.f;
        RENDER_HIP(hipEventElapsedTime(&bin_ms, ev[0], ev[1])); RENDER_HIP(hipEventElapsedTime(&paint_ms, ev[1], ev[2]));
        for (auto& e : ev) hipEventDestroy(e);
        fprintf(stderr, "# render_frames overlay %d frames %zu primitives %u list entries: device ms bin %.4f paint %.4f\n", n, prims.size(), total,
                bin_ms, paint_ms);
    }
    if ((int64_t)total != list_total)             // the count pass and the host's sizing are the same arithmetic: never silent
        return err.fail(BOD_ERR_HIP, "%s: the binning counted %u list entries, the host sized %lld", WHO, total, (long long)list_total);
    return BOD_OK;
}

int heat_chunk_rows(int h, int w) {
    const size_t per = (size_t)h * w * sizeof(float);
    return (int)std::max<size_t>(1, std::min<size_t>(HEAT_CHUNK_BYTES / per, HEAT_CHUNK_ROWS));
}

int run_heat(int32_t n, const uint8_t* rgb_in, const int32_t* src_hw, const int32_t* num_det, const int32_t* det_boxes,
             const float* det_corner_covs, uint8_t* rgb_out, hipStream_t s, Err& err) {
    char msg[512];
    // every row is validated before anything is drawn, by the code that bod_pdq_frames validates with
    for (int f = 0, d0 = 0; f < n; d0 += num_det[f], ++f) {
        const int h = src_hw[2 * f], w = src_hw[2 * f + 1], m = heat_chunk_rows(h, w);
        for (int c0 = 0; c0 < num_det[f]; c0 += m) {
            const int mm = std::min(m, num_det[f] - c0);
            int bad = -1;
            msg[0] = 0;
            const int st = pdq_box_heatmaps_device(h, w, mm, det_boxes + 4 * (size_t)(d0 + c0), det_corner_covs + 8 * (size_t)(d0 + c0), nullptr, &bad,
                                                   s, msg, sizeof msg);
            if (st != BOD_OK) return err.fail(st, "%s: frame %d row %d: %s", WHO, f, bad < 0 ? 0 : c0 + bad, msg);
        }
    }
    int64_t off = 0;
    const bool trace = trace_on();
    double trace_ms = 0.0;
    long long trace_rows = 0;
    for (int f = 0, d0 = 0; f < n; d0 += num_det[f], ++f) {
        const int h = src_hw[2 * f], w = src_hw[2 * f + 1], D = num_det[f], m = heat_chunk_rows(h, w);
        hipEvent_t ev[2] = {nullptr, nullptr};
        const int64_t npix = (int64_t)h * w;
        DevArena arena;
        uint8_t *d_in, *d_out, *d_index; float* d_heat = nullptr;
        RENDER_HIP(arena.alloc(&d_in, (size_t)npix * 3)); RENDER_HIP(arena.alloc(&d_out, (size_t)npix * 3));
        RENDER_HIP(arena.alloc(&d_index, (size_t)npix));
        if (D) RENDER_HIP(arena.alloc(&d_heat, (size_t)std::min(m, D) * (size_t)npix));
        RENDER_HIP(hipMemcpyAsync(d_in, rgb_in + off, (size_t)npix * 3, hipMemcpyHostToDevice, s));
        RENDER_HIP(hipMemsetAsync(d_index, 0, (size_t)npix, s));
        if (trace) { for (auto& e : ev) RENDER_HIP(hipEventCreate(&e)); RENDER_HIP(hipEventRecord(ev[0], s)); }
        for (int c0 = 0; c0 < D; c0 += m) {
            const int mm = std::min(m, D - c0);
            int bad = -1;
            msg[0] = 0;
            const int st = pdq_box_heatmaps_device(h, w, mm, det_boxes + 4 * (size_t)(d0 + c0), det_corner_covs + 8 * (size_t)(d0 + c0), d_heat, &bad, s,
                                                   msg, sizeof msg);
            if (st != BOD_OK) return err.fail(st, "%s: frame %d row %d: %s", WHO, f, bad < 0 ? c0 : c0 + bad, msg);
            hipLaunchKernelGGL(render_heat_compose_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, d_heat, mm, npix, d_index);
            RENDER_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(render_heat_colour_kernel, dim3((unsigned)(((npix + 3) / 4 + 255) / 256)), dim3(256), 0, s, d_in, d_index, npix, d_out);
        RENDER_HIP(hipGetLastError());
        if (trace) RENDER_HIP(hipEventRecord(ev[1], s));
        RENDER_HIP(hipMemcpyAsync(rgb_out + off, d_out, (size_t)npix * 3, hipMemcpyDeviceToHost, s));
        RENDER_HIP(hipStreamSynchronize(s));
        if (trace) {                              // (the span from the first heatmap launch to the colour kernel, the chunks' synchronisations included)
            float ms = 0.f;
            RENDER_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
            for (auto& e : ev) hipEventDestroy(e);
            trace_ms += ms; trace_rows += D;
        }
        off += npix * 3;
    }
    if (trace) fprintf(stderr, "# render_frames heat %d frames %lld detections: device ms heatmaps+compose+colour %.4f\n", n, trace_rows, trace_ms);
    return BOD_OK;
}

}  // namespace

int render_validate(int32_t n, const uint8_t* rgb_in, const int32_t* src_hw, const int32_t* num_det, const int32_t* det_boxes,
                    const float* det_corner_covs, const uint8_t* det_colors, const uint8_t* det_text, const int32_t* num_gt,
                    const int32_t* gt_boxes, const bod_render_options* opt, uint8_t* rgb_out, char* errbuf, size_t errcap) {
    Err err{errbuf, errcap};
    if (n < 0) return err.fail(BOD_ERR_INVALID_ARG, "%s: n = %d is negative", WHO, n);
    const bod_render_options o = options_or_default(opt);
    if (o.view != BOD_RENDER_OVERLAY && o.view != BOD_RENDER_HEAT) return err.fail(BOD_ERR_INVALID_ARG, "%s: unknown view %d", WHO, o.view);
    if (o.line_width < 1 || o.line_width > 7) return err.fail(BOD_ERR_INVALID_ARG, "%s: line_width %d outside 1..7", WHO, o.line_width);
    if (!std::isfinite(o.r2) || !(o.r2 > 0.0f)) return err.fail(BOD_ERR_INVALID_ARG, "%s: r2 = %g is not finite and greater than 0", WHO, (double)o.r2);
    if (n == 0) return BOD_OK;
    if (!rgb_in || !src_hw || !num_det || !rgb_out) return err.fail(BOD_ERR_INVALID_ARG, "%s: a frame array or num_det is NULL with n = %d", WHO, n);
    int64_t sum_d = 0, sum_g = 0;
    for (int f = 0; f < n; ++f) {
        const int64_t h = src_hw[2 * f], w = src_hw[2 * f + 1];
        if (h < 1 || w < 1 || h > 65535 || w > 65535) return err.fail(BOD_ERR_INVALID_ARG, "%s: frame %d is %lldx%lld", WHO, f, (long long)h, (long long)w);
        if (num_det[f] < 0 || (num_gt && num_gt[f] < 0)) return err.fail(BOD_ERR_INVALID_ARG, "%s: frame %d has a negative count", WHO, f);
        sum_d += num_det[f]; sum_g += num_gt ? num_gt[f] : 0;
    }
    if (sum_d > 0x7FFFFFFF / 16 || sum_g > 0x7FFFFFFF / 16) return err.fail(BOD_ERR_INVALID_ARG, "%s: more rows than one call covers", WHO);
    if (sum_d && (!det_boxes || !det_corner_covs || !det_colors))
        return err.fail(BOD_ERR_INVALID_ARG, "%s: det_boxes, det_corner_covs or det_colors is NULL with %lld detections", WHO, (long long)sum_d);
    if (sum_g && !gt_boxes) return err.fail(BOD_ERR_INVALID_ARG, "%s: gt_boxes is NULL with %lld ground-truth boxes", WHO, (long long)sum_g);
    if (det_text) {
        int64_t d0 = 0;
        for (int f = 0; f < n; d0 += num_det[f], ++f)
            for (int d = 0; d < num_det[f]; ++d) {
                const uint8_t* t = det_text + 16 * (d0 + d);
                for (int i = 0; i < 16 && t[i] != 0xFF; ++i)
                    if (t[i] >= RENDER_FONT_COUNT)
                        return err.fail(BOD_ERR_INVALID_ARG, "%s: frame %d row %d: glyph index %d at position %d is not below %d", WHO, f, d, (int)t[i], i,
                                        RENDER_FONT_COUNT);
            }
    }
    return BOD_OK;
}

int render_frames_run(int32_t n, const uint8_t* rgb_in, const int32_t* src_hw, const int32_t* num_det, const int32_t* det_boxes,
                      const float* det_corner_covs, const uint8_t* det_colors, const uint8_t* det_text, const int32_t* num_gt,
                      const int32_t* gt_boxes, const bod_render_options* opt, uint8_t* rgb_out, int32_t* skipped_ellipses, hipStream_t s,
                      char* errbuf, size_t errcap) {
    Err err{errbuf, errcap};
    const bod_render_options o = options_or_default(opt);
    if (o.view == BOD_RENDER_HEAT) {
        if (skipped_ellipses) memset(skipped_ellipses, 0, sizeof(int32_t) * (size_t)n);
        return run_heat(n, rgb_in, src_hw, num_det, det_boxes, det_corner_covs, rgb_out, s, err);
    }
    return run_overlay(n, rgb_in, src_hw, num_det, det_boxes, det_corner_covs, det_colors, det_text, num_gt, gt_boxes, o, rgb_out, skipped_ellipses, s,
                       err);
}

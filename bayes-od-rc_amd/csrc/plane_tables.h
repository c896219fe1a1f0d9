// Host-side row tables of the plane -> plane convolutions (backbone, FPN): plain C++ (no HIP), shared by engine.hip (make_table) and
// by the sanitizer build of tests/host/plane_tables_check.cpp (g++ -fsanitize=address,undefined; tests/test_host_plane_tables.py).
//   plane_row_table        one RowEnt per output pixel (b, y, x) of a convolution between two planes with a one-pixel zero border;
//                          with out_step = 2 only the output pixels (2y, 2x), y < ceil(h / 2), x < ceil(w / 2) -- the pixels a 1x1
//                          stride-2 VALID convolution over the output plane reads (the next ResNet stage's `2a` and `branch1`)
//   plane_rows_of_even_y   the rows of a dense table whose output y is even, all x (runs stay x-adjacent for xr_tile_rows)
#pragma once
#include "plan_tables.h"
#include <cmath>

struct PlaneGeom {         // a [B][h + 2][w + 2] plane inside a buffer, in pixels
    int64_t base;          // pixel offset of image 0's padded plane in its buffer
    int64_t bstride;       // padded pixels per image
    int pitch;             // padded row width
    int h, w;
};

inline int plane_step_count(int n, int step) { return (n + step - 1) / step; }

// Entry of output pixel (b, y, x).  (org_y, org_x) = padded coordinate of the window origin of output (0, 0); res optional
// (nearest-upsampled when its size differs).
inline RowEnt plane_row_entry(const PlaneGeom& in, const PlaneGeom& out, int stride, int org_y, int org_x, const PlaneGeom* res, int b, int y, int x) {
    RowEnt e{};
    e.in_off = (int32_t)(in.base + b * in.bstride + (int64_t)(y * stride + org_y) * in.pitch + (x * stride + org_x));
    e.in_pitch = in.pitch;
    e.out_off = (int32_t)(out.base + b * out.bstride + (int64_t)(y + 1) * out.pitch + (x + 1));
    if (res) {
        int ry = y, rx = x;
        if (res->h != out.h || res->w != out.w) {
            ry = std::min((int)std::floor((y + 0.5) * ((double)res->h / out.h)), res->h - 1);
            rx = std::min((int)std::floor((x + 0.5) * ((double)res->w / out.w)), res->w - 1);
        }
        e.res_off = (int32_t)(res->base + b * res->bstride + (int64_t)(ry + 1) * res->pitch + (rx + 1));
    }
    return e;
}

// out_step 1: every output pixel, B * h * w rows.  out_step 2: B * ceil(h / 2) * ceil(w / 2) rows, each the dense table's row of
// pixel (2y, 2x): same input, output and residual positions, the other pixels of the output plane are not written.
inline void plane_row_table(int B, const PlaneGeom& in, const PlaneGeom& out, int stride, int org_y, int org_x, const PlaneGeom* res,
                            int out_step, std::vector<RowEnt>& rows) {
    const int ny = plane_step_count(out.h, out_step), nx = plane_step_count(out.w, out_step);
    rows.resize((size_t)B * ny * nx);
    size_t r = 0;
    for (int b = 0; b < B; ++b)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) rows[r++] = plane_row_entry(in, out, stride, org_y, org_x, res, b, y * out_step, x * out_step);
}

// The step-2 table costs no memory of its own: it lives in the dense table of the same convolution shape.  The plane -> plane kernels
// read the first four fields of an entry only (in_off, in_pitch, out_off, res_off; the other four belong to the head towers: dropout
// counters, fused-output row, extended-row index -- never used between planes), so the SECOND half of dense entry i holds the first
// half of step-2 entry i, and the launch takes the table half an entry further on (plane_step_view): entry m of the view is bytes
// [32 m + 16, 32 m + 48) of the dense table.  A kernel that loads a whole entry of the view reads the next dense entry's first half
// behind it, so the view's last entry must end inside the dense table: step.size() < dense.size() (false: not embedded -- a 1 x 1
// plane, whose step-2 table IS the dense table).
constexpr size_t PLANE_STEP_VIEW_BYTES = 16;
static_assert(sizeof(RowEnt) == 32 && offsetof(RowEnt, rng_p) == PLANE_STEP_VIEW_BYTES, "the step-2 view starts at an entry's second half");

inline bool plane_embed_step_table(std::vector<RowEnt>& dense, const std::vector<RowEnt>& step) {
    if (step.size() >= dense.size()) return false;
    for (size_t i = 0; i < step.size(); ++i) {
        dense[i].rng_p = step[i].in_off; dense[i].rng_zs = step[i].in_pitch; dense[i].pad0 = step[i].out_off; dense[i].pad1 = step[i].res_off;
    }
    return true;
}

inline const RowEnt* plane_step_view(const RowEnt* dense) {
    return reinterpret_cast<const RowEnt*>(reinterpret_cast<const char*>(dense) + PLANE_STEP_VIEW_BYTES);
}

// dense [B][h][w] table -> its rows with even y, all x, in the same order
inline void plane_rows_of_even_y(const std::vector<RowEnt>& dense, int B, int h, int w, std::vector<RowEnt>& rows) {
    rows.clear();
    rows.reserve((size_t)B * plane_step_count(h, 2) * w);
    for (int b = 0; b < B; ++b)
        for (int y = 0; y < h; y += 2)
            for (int x = 0; x < w; ++x) rows.push_back(dense[((size_t)b * h + y) * w + x]);
}

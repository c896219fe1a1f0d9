// CPU check of the plane -> plane row tables with an output step (bayes-od-rc_amd/csrc/plane_tables.h), compiled with
// -fsanitize=address,undefined by tests/test_host_plane_tables.py.  The last block of ResNet stages 2-4 is read by the next stage's
// 1x1 stride-2 VALID convolutions alone, so its `2c` runs on the table of output pixels (2y, 2x).  For planes 128x128, 25x19, 13x10,
// 7x5 and 1x1, batch 1 and 3:
//   - the step-2 table has B * ceil(h / 2) * ceil(w / 2) rows;
//   - each row equals the dense table's row of pixel (2y, 2x) in all three offsets (input, output, shortcut) and the pitch;
//   - the pixels it writes are exactly those a stride-2 VALID 1x1 table over the same plane reads (add_conv: first_stride = 2,
//     same = false -> origin (1, 1) in padded coordinates), each once, and every one lies inside the plane's interior;
//   - embedded in the dense table (plane_embed_step_table / plane_step_view: no allocation of its own) the view shows the same rows,
//     the dense rows' first halves are untouched and the view's last entry ends inside the dense table; a 1x1 plane is not embedded;
//   - the even-row selection for stage 4's `2b` (plane_rows_of_even_y) keeps B * ceil(h / 2) * w rows, the dense rows of even y in
//     order, whose x-adjacent runs tile full (xr_tile_rows) and cover every pixel the step-2 `2c` table reads.
#include "plane_tables.h"
#include <cstdio>
#include <cstring>
#include <set>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } } } while (0)

static PlaneGeom plane(int h, int w, int64_t base = 0) { return PlaneGeom{base, (int64_t)(h + 2) * (w + 2), w + 2, h, w}; }

int main() {
    const int sizes[][2] = {{128, 128}, {25, 19}, {13, 10}, {7, 5}, {1, 1}};
    const int batches[] = {1, 3};
    long configs = 0;
    for (const auto& hw : sizes)
        for (int B : batches) {
            const int h = hw[0], w = hw[1], h2 = (h + 1) / 2, w2 = (w + 1) / 2;
            char what[64];
            std::snprintf(what, sizeof what, "%dx%d B=%d", h, w, B);
            // the block's planes: t2 (input of the 2c), x (shortcut), out; three buffers of the same geometry
            const PlaneGeom t2 = plane(h, w), x = plane(h, w), out = plane(h, w);
            std::vector<RowEnt> dense, step2;
            plane_row_table(B, t2, out, 1, 1, 1, &x, 1, dense);          // 1x1, stride 1, VALID: origin (1, 1)
            plane_row_table(B, t2, out, 1, 1, 1, &x, 2, step2);
            CHECK(dense.size() == (size_t)B * h * w, "%s: dense table has %zu rows", what, dense.size());
            CHECK(step2.size() == (size_t)B * h2 * w2, "%s: step-2 table has %zu rows, expected %d", what, step2.size(), B * h2 * w2);
            if (dense.size() != (size_t)B * h * w || step2.size() != (size_t)B * h2 * w2) continue;
            std::set<int32_t> written;
            for (int b = 0; b < B; ++b)
                for (int y = 0; y < h2; ++y)
                    for (int xx = 0; xx < w2; ++xx) {
                        const RowEnt& r = step2[((size_t)b * h2 + y) * w2 + xx];
                        const RowEnt& d = dense[((size_t)b * h + 2 * y) * w + 2 * xx];
                        CHECK(r.in_off == d.in_off && r.out_off == d.out_off && r.res_off == d.res_off && r.in_pitch == d.in_pitch,
                              "%s: row (%d, %d, %d) is (%d, %d, %d), dense (%d, %d, %d)", what, b, y, xx, r.in_off, r.out_off, r.res_off, d.in_off, d.out_off, d.res_off);
                        CHECK(std::memcmp(&r, &d, sizeof(RowEnt)) == 0, "%s: row (%d, %d, %d) differs from the dense row outside the offsets", what, b, y, xx);
                        // same pixel of t2, x and out; inside the interior of image b's plane
                        CHECK(r.in_off == r.out_off && r.res_off == r.out_off, "%s: row (%d, %d, %d) mixes pixels", what, b, y, xx);
                        const int64_t rel = (int64_t)r.out_off - b * out.bstride;
                        const int py = (int)(rel / out.pitch), px = (int)(rel % out.pitch);
                        CHECK(rel >= 0 && rel < out.bstride && py >= 1 && py <= h && px >= 1 && px <= w, "%s: row (%d, %d, %d) writes (%d, %d): border or outside", what, b, y, xx, py, px);
                        CHECK(written.insert(r.out_off).second, "%s: pixel %d written twice", what, r.out_off);
                    }
            // the step-2 table inside the dense table: the first half of the dense entries is untouched, entry m of the view (half an
            // entry further on) is the step-2 row in the four fields the plane kernels read, and a whole-entry load of the view's last
            // entry ends inside the dense table
            {
                std::vector<RowEnt> host = dense;
                const bool embedded = plane_embed_step_table(host, step2);
                CHECK(embedded == (step2.size() < dense.size()), "%s: embedded %d with %zu of %zu rows", what, (int)embedded, step2.size(), dense.size());
                if (!embedded) CHECK(h == 1 && w == 1 && std::memcmp(step2.data(), dense.data(), dense.size() * sizeof(RowEnt)) == 0, "%s: only a 1x1 plane's step-2 table is its dense table", what);
                if (embedded) {
                    const char* view = reinterpret_cast<const char*>(plane_step_view(host.data()));
                    const char* end = reinterpret_cast<const char*>(host.data() + host.size());
                    CHECK(view + step2.size() * sizeof(RowEnt) <= end, "%s: the view's last entry ends %td bytes behind the dense table", what, view + step2.size() * sizeof(RowEnt) - end);
                    for (size_t i = 0; i < dense.size(); ++i)
                        CHECK(std::memcmp(&host[i], &dense[i], PLANE_STEP_VIEW_BYTES) == 0, "%s: dense row %zu changed by the embedding", what, i);
                    for (size_t m = 0; m < step2.size() && view + (m + 1) * sizeof(RowEnt) <= end; ++m) {
                        RowEnt e;                                        // what a kernel sees at rows[m] of the view
                        std::memcpy(&e, view + m * sizeof(RowEnt), sizeof(RowEnt));
                        CHECK(e.in_off == step2[m].in_off && e.in_pitch == step2[m].in_pitch && e.out_off == step2[m].out_off && e.res_off == step2[m].res_off,
                              "%s: view row %zu is (%d, %d, %d, %d)", what, m, e.in_off, e.in_pitch, e.out_off, e.res_off);
                    }
                }
            }
            // the reader: the next stage's 2a / branch1 over `out`, 1x1 stride 2 VALID, onto a ceil(h / 2) x ceil(w / 2) plane
            const PlaneGeom next = plane(h2, w2);
            std::vector<RowEnt> reader;
            plane_row_table(B, out, next, 2, 1, 1, nullptr, 1, reader);
            CHECK(reader.size() == step2.size(), "%s: the reader has %zu rows, the step-2 table %zu", what, reader.size(), step2.size());
            std::set<int32_t> read;
            for (const RowEnt& r : reader) read.insert(r.in_off);
            CHECK(read == written, "%s: %zu pixels read, %zu written, sets differ", what, read.size(), written.size());
            for (size_t i = 0; i < reader.size() && i < step2.size(); ++i)
                CHECK(reader[i].in_off == step2[i].out_off, "%s: reader row %zu reads %d, the step-2 table's row writes %d", what, i, reader[i].in_off, step2[i].out_off);

            // stage 4's 2b: 3x3 stride 1 SAME (origin (0, 0)) from t1 to t2, even output rows, all x
            const PlaneGeom t1 = plane(h, w);
            std::vector<RowEnt> dense3, even;
            plane_row_table(B, t1, t2, 1, 0, 0, nullptr, 1, dense3);
            plane_rows_of_even_y(dense3, B, h, w, even);
            CHECK(even.size() == (size_t)B * h2 * w, "%s: %zu even rows, expected %d", what, even.size(), B * h2 * w);
            if (even.size() != (size_t)B * h2 * w) continue;
            std::set<int32_t> produced;
            for (int b = 0; b < B; ++b)
                for (int y = 0; y < h2; ++y)
                    for (int xx = 0; xx < w; ++xx) {
                        const RowEnt& r = even[((size_t)b * h2 + y) * w + xx];
                        CHECK(std::memcmp(&r, &dense3[((size_t)b * h + 2 * y) * w + xx], sizeof(RowEnt)) == 0, "%s: even row (%d, %d, %d) is not the dense row", what, b, y, xx);
                        produced.insert(r.out_off);
                    }
            for (const RowEnt& r : step2) CHECK(produced.count(r.in_off) == 1, "%s: the 2c reads pixel %d of t2, which the even-row 2b does not write", what, r.in_off);
            std::vector<RowEnt> tiled;
            std::vector<ExtRow> ext;
            CHECK(xr_tile_rows(even, tiled, ext), "%s: extended rows out of order", what);
            CHECK(tiled.size() % 256 == 0 && ext.size() == tiled.size() / 256 * XR_EXT_ROWS, "%s: %zu tiled rows, %zu extended rows", what, tiled.size(), ext.size());
            size_t valid = 0;
            const int64_t in_pixels = (int64_t)B * t1.bstride;
            for (size_t t = 0; t < tiled.size() / 256; ++t) {
                const ExtRow* e = &ext[t * XR_EXT_ROWS];
                for (int q = 0; q < XR_EXT_ROWS; ++q)
                    CHECK(e[q].x >= e[0].x && e[q].x >= 0 && (int64_t)e[q].x + 2 * (int64_t)e[q].y < in_pixels, "%s: tile %zu extended row %d out of the planes", what, t, q);
                for (int s = 0; s < 256; ++s) {
                    const RowEnt& r = tiled[t * 256 + s];
                    if (r.out_off < 0) continue;
                    ++valid;
                    CHECK(produced.count(r.out_off) == 1, "%s: tile %zu slot %d writes %d, not an even-row pixel", what, t, s, r.out_off);
                    CHECK(r.pad1 >= 0 && r.pad1 + 2 < XR_EXT_ROWS, "%s: extended-row index %d", what, r.pad1);
                    if (r.pad1 < 0 || r.pad1 + 2 >= XR_EXT_ROWS) continue;
                    for (int ky = 0; ky < 3; ++ky)
                        for (int kx = 0; kx < 3; ++kx)
                            CHECK((int64_t)e[r.pad1 + kx].x + (int64_t)ky * e[r.pad1 + kx].y == (int64_t)r.in_off + (int64_t)ky * r.in_pitch + kx,
                                  "%s: tile %zu slot %d tap (%d, %d)", what, t, s, ky, kx);
                }
            }
            CHECK(valid == even.size(), "%s: %zu valid tiled rows for %zu even rows", what, valid, even.size());
            // whole planes of 32-pixel rows: eight runs fill a tile (no emptier than the dense tiling)
            if (w == 128 && h == 128) CHECK(tiled.size() == (size_t)B * h2 * w, "%s: %zu tiled rows for %d pixels: tiles not full", what, tiled.size(), B * h2 * w);
            ++configs;
        }
    std::printf("plane_tables_check: %ld configurations, %d failures\n", configs, failures);
    return failures ? 1 : 0;
}

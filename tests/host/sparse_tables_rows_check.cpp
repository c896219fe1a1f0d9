// CPU replay of the sparse tail's row table at a tile height of R rows (bayes-od-rc_amd/csrc/sparse_tables.h: the `R` parameter of
// st_pack_run / st_write_piece / st_min_pixels; post_kernels.hip sparse_tail_rows_kernel with SparseTailArgs.tail_rows), compiled
// with -fsanitize=address,undefined by tests/test_host_sparse_tables_rows.py.  For R = 192 (three 16-row pixel fragments per wave of
// the tower kernel) and R = 256, on several geometries, sample counts and random keep sets, empty and full ones included:
//   - the table equals a serial walk with slot limit R / N, row for row and extended row for extended row;
//   - every row equals the dense per-sample table's row apart from its extended-row index, each (image, sample, pixel) of the tail
//     appears once, each tap's staged element is the gathered one, a tile's first extended row is its smallest, tiles hold all N
//     samples of their pixels, rows behind slot R / N are padding;
//   - tile counts stay within the closed-form capacity, which is the same for both heights (st_min_pixels);
//   - at the 0.18 density the 192-row table has at most 2 % more tiles than the 256-row one: per table for the three large
//     geometries (hundreds of tiles each), and per sample count summed over all five.  The two small geometries have 8 to 14 tiles
//     per table, where one tile more -- an image's last, partly filled tile -- is 8 to 12 %: quantisation, not the packing rule, so
//     they enter the sum only (their counts are printed).
#include "sparse_tables.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } } } while (0)

static PyramidGeometry geometry(int H, int W) {      // as tests/host/plan_tables_check.cpp
    auto cdiv = [](int a, int b) { return (a + b - 1) / b; };
    int lh[5], lw[5];
    int h = cdiv(cdiv(H, 2), 2), w = cdiv(cdiv(W, 2), 2);
    for (int l = 0; l < 3; ++l) { h = cdiv(h, 2); w = cdiv(w, 2); lh[l] = h; lw[l] = w; }
    lh[3] = (lh[2] + 1) / 2; lw[3] = (lw[2] + 1) / 2;
    lh[4] = (lh[3] + 1) / 2; lw[4] = (lw[3] + 1) / 2;
    return pyramid_geometry(lh, lw);
}

struct Tables { std::vector<RowEnt> rows; std::vector<ExtRow> ext; int tiles = 0; long valid_rows = 0; };

static bool same_row(const RowEnt& a, const RowEnt& b) { return std::memcmp(&a, &b, sizeof(RowEnt)) == 0; }

// a serial walk over the pixels of each image (adjacency from the row table), slot limit R / N
static void serial_tail(const std::vector<uint8_t>& kept, const std::vector<RowEnt>& pix, int B, int N, int P, int64_t Ppad, int R, Tables& out) {
    const int Qmax = R / N;
    const RowEnt invalid = st_invalid_row(pix[0]);
    for (int b = 0; b < B; ++b) {
        const uint8_t* flag = &kept[(size_t)b * P];
        auto adjacent = [&](int p) { return pix[p].in_off == pix[p - 1].in_off + 1 && pix[p].in_pitch == pix[p - 1].in_pitch; };
        std::vector<StQuad> chunks, tiles;
        int Q = 0, X = 0, first = 0;
        bool open = false;
        auto close_tile = [&]() { tiles.push_back(StQuad{first, Q, X, 0}); open = false; };
        int p = 0;
        while (p < P) {
            if (!flag[p]) { ++p; continue; }
            int L = 1;
            while (p + L < P && adjacent(p + L) && (flag[p + L] || (p + L + 1 < P && flag[p + L + 1] && adjacent(p + L + 1)))) ++L;
            while (L > 0) {
                if (!open) { first = p; Q = 0; X = 0; open = true; }
                const int take = std::min(std::min(L, Qmax - Q), (XR_EXT_ROWS - X) / N - 2);
                if (take < 1) { close_tile(); continue; }
                chunks.push_back(StQuad{p, (int)tiles.size(), Q, X | (take << 16)});
                X += N * (take + 2); Q += take; p += take; L -= take;
                if (Q == Qmax) close_tile();
            }
        }
        if (open) close_tile();
        const int base = out.tiles;
        out.tiles += (int)tiles.size();
        out.rows.resize((size_t)out.tiles * R);
        out.ext.resize((size_t)out.tiles * XR_EXT_ROWS);
        for (const StQuad& c : chunks) {
            const int p0 = c.x, Q0 = c.z, X0 = c.w & 0xFFFF, take = c.w >> 16, t = base + c.y;
            for (int n = 0; n < N; ++n) {
                const int x0 = X0 + n * (take + 2);
                const RowEnt f = st_row(pix[p0], b, n, p0, N, P, Ppad);
                for (int k = 0; k < take + 2; ++k) out.ext[(size_t)t * XR_EXT_ROWS + x0 + k] = ExtRow{f.in_off + k, f.in_pitch};
                for (int k = 0; k < take; ++k) {
                    RowEnt q = st_row(pix[p0 + k], b, n, p0 + k, N, P, Ppad);
                    q.pad1 = x0 + k;
                    out.rows[(size_t)t * R + (Q0 + k) * N + n] = q;
                }
            }
        }
        for (size_t t = 0; t < tiles.size(); ++t) {
            for (int r = tiles[t].y * N; r < R; ++r) out.rows[(base + t) * R + r] = invalid;
            const RowEnt f = st_row(pix[tiles[t].x], b, 0, tiles[t].x, N, P, Ppad);
            for (int r = tiles[t].z; r < XR_EXT_ROWS; ++r) out.ext[(base + t) * XR_EXT_ROWS + r] = ExtRow{f.in_off, f.in_pitch};
        }
    }
}

// the kernel's phases for the tail table (post_kernels.hip sparse_tail_rows_kernel, t = 0) at R rows per tile
static void parallel_tail(const std::vector<uint8_t>& kept, const std::vector<RowEnt>& pix, const SparseLevels& lv, int B, int N, int P,
                          int64_t Ppad, int R, Tables& o, std::vector<uint8_t>& flags) {
    flags.assign((size_t)B * P, 0);
    const RowEnt invalid = st_invalid_row(pix[0]);
    for (int b = 0; b < B; ++b) {
        uint8_t* f = &flags[(size_t)b * P];
        for (int p = 0; p < P; ++p) f[p] = kept[(size_t)b * P + p] ? ST_KEPT : 0;
        for (int p = 0; p < P; ++p) if (st_member(f, lv, p, ST_KEPT)) f[p] |= ST_TAIL;
        const int share = (P + 255) / 256;
        int cnt[256], incl[256];
        for (int tid = 0; tid < 256; ++tid) {
            const int q0 = std::min(P, tid * share), q1 = std::min(P, q0 + share);
            cnt[tid] = 0;
            for (int p = q0; p < q1; ++p) cnt[tid] += st_run_edge(f, lv, p, ST_TAIL) & 1;
        }
        for (int tid = 0, acc = 0; tid < 256; ++tid) { acc += cnt[tid]; incl[tid] = acc; }
        const int nrun = incl[255];
        std::vector<int32_t> rx((size_t)P, -1), ry((size_t)P, -1);
        for (int tid = 0; tid < 256; ++tid) {
            const int q0 = std::min(P, tid * share), q1 = std::min(P, q0 + share);
            int r = incl[tid] - cnt[tid];
            for (int p = q0; p < q1; ++p) {
                const int edge = st_run_edge(f, lv, p, ST_TAIL);
                if (edge & 1) { CHECK(r < P, "run index %d", r); rx[r++] = p; }
                if (edge & 2) { CHECK(r >= 1, "run end before a start at %d", p); if (r >= 1) ry[r - 1] = p; }
            }
        }
        std::vector<StQuad> chunks((size_t)P), tiles((size_t)P);
        StPack st{0, 0, 0, 0, 0, 0};
        for (int r = 0; r < nrun; ++r) {
            CHECK(rx[r] >= 0 && ry[r] >= rx[r], "run %d: [%d, %d]", r, rx[r], ry[r]);
            st_pack_run(st, rx[r], ry[r] - rx[r] + 1, N, chunks.data(), tiles.data(), true, R);
        }
        st_pack_close(st, tiles.data(), true);
        CHECK(st.nchunk <= P && st.ntile <= P, "scratch overflow: %d pieces, %d tiles for %d pixels", st.nchunk, st.ntile, P);
        const int base = o.tiles;
        o.tiles += st.ntile;
        o.rows.resize((size_t)o.tiles * R);
        o.ext.resize((size_t)o.tiles * XR_EXT_ROWS);
        for (int i = 0; i < st.nchunk * N; ++i) {
            const int ci = i / N, n = i - ci * N;
            st_write_piece(chunks[ci], n, b, base + chunks[ci].y, pix.data(), N, P, Ppad, o.rows.data(), o.ext.data(), R);
        }
        for (int i = 0; i < st.ntile * R; ++i) {
            const int tt = i / R, r = i - tt * R;
            if (st_pad_row(tiles[tt], r, N)) o.rows[(size_t)(base + tt) * R + r] = invalid;
        }
        for (int i = 0; i < st.ntile * XR_EXT_ROWS; ++i) {
            const int tt = i / XR_EXT_ROWS, r = i - tt * XR_EXT_ROWS;
            if (r >= tiles[tt].z) o.ext[(size_t)(base + tt) * XR_EXT_ROWS + r] = st_pad_ext(tiles[tt], b, pix.data(), N, P, Ppad);
        }
    }
}

int main() {
    const int sizes[][2] = {{512, 512}, {384, 1248}, {720, 1280}, {96, 160}, {100, 75}};
    const int samples[] = {2, 7, 10, 30, 64};
    const int heights[] = {192, 256};
    const double densities[] = {0.0, 0.002, 0.02, 0.18, 0.6, 1.0};
    std::mt19937 rng(4321);
    long configs = 0;
    for (int N : samples) {
        // the capacity rule: the fewest pixels of a closed tile do not depend on the height
        CHECK(st_min_pixels(N, 192) == st_min_pixels(N), "N=%d: st_min_pixels %d at 192 rows, %d at 256", N, st_min_pixels(N, 192), st_min_pixels(N));
        CHECK(st_min_pixels(N, 256) == st_min_pixels(N), "N=%d: the default height is 256", N);
        long tiles018[2] = {0, 0};
        for (const auto& hw : sizes)
            for (double dens : densities) {
                const int B = 2;
                const PyramidGeometry g = geometry(hw[0], hw[1]);
                const int P = g.P;
                std::vector<RowEnt> t1, t2, t3;
                head_row_tables(g, B, N, t1, t2, t3);
                const std::vector<RowEnt> pix(t2.begin(), t2.begin() + P);
                SparseLevels lv{};
                lv.n = 5;
                for (int l = 0; l < 5; ++l) { lv.lw[l] = g.lw[l]; lv.lh[l] = g.lh[l]; lv.p0[l] = (int32_t)g.lvl_p0[l]; }
                // kept pixels: independent draws, plus clusters (objects) at the middle densities
                std::vector<uint8_t> kept((size_t)B * P, 0);
                std::uniform_real_distribution<double> U(0.0, 1.0);
                for (auto& k : kept) k = U(rng) < dens ? 1 : 0;
                if (dens > 0 && dens < 1)
                    for (int b = 0; b < B; ++b)
                        for (int c = 0; c < 8; ++c) {
                            const int p = (int)(U(rng) * P), len = 1 + (int)(U(rng) * 12);
                            for (int k = 0; k < len && p + k < P; ++k) kept[(size_t)b * P + p + k] = 1;
                        }
                const int cap = B * (P / st_min_pixels(N) + 1);
                const int64_t in_pixels = (int64_t)B * N * g.Ppad;
                long geo018[2] = {0, 0};
                for (int hi = 0; hi < 2; ++hi) {
                    const int R = heights[hi], Qmax = R / N;
                    char what[128];
                    std::snprintf(what, sizeof what, "%dx%d N=%d density %.3f R=%d", hw[0], hw[1], N, dens, R);
                    Tables ref, got;
                    std::vector<uint8_t> flags;
                    serial_tail(kept, pix, B, N, P, g.Ppad, R, ref);
                    parallel_tail(kept, pix, lv, B, N, P, g.Ppad, R, got, flags);
                    CHECK(got.tiles == ref.tiles, "%s: %d tiles, serial walk %d", what, got.tiles, ref.tiles);
                    if (got.tiles == ref.tiles) {
                        for (size_t i = 0; i < ref.rows.size(); ++i) CHECK(same_row(got.rows[i], ref.rows[i]), "%s: row %zu differs", what, i);
                        for (size_t i = 0; i < ref.ext.size(); ++i)
                            CHECK(got.ext[i].x == ref.ext[i].x && got.ext[i].y == ref.ext[i].y, "%s: extended row %zu differs", what, i);
                    }
                    CHECK(got.tiles <= cap, "%s: %d tiles over the capacity %d", what, got.tiles, cap);
                    if (dens == 0.18) { tiles018[hi] += got.tiles; geo018[hi] = got.tiles; }
                    std::vector<int> seen((size_t)B * N * P, 0);
                    for (int tile = 0; tile < got.tiles; ++tile) {
                        const ExtRow* e = &got.ext[(size_t)tile * XR_EXT_ROWS];
                        for (int q = 0; q < XR_EXT_ROWS; ++q) {
                            CHECK(e[q].x >= e[0].x, "%s: tile %d extended row %d below the first", what, tile, q);
                            CHECK(e[q].x >= 0 && (int64_t)e[q].x + 2 * (int64_t)e[q].y < in_pixels, "%s: tile %d extended row %d outside the planes", what, tile, q);
                        }
                        for (int s = 0; s < R; ++s) {
                            const RowEnt& r = got.rows[(size_t)tile * R + s];
                            const int q = s / N, n = s - q * N;
                            if (r.out_off < 0) {
                                if (q < Qmax) CHECK(got.rows[(size_t)tile * R + q * N].out_off < 0, "%s: tile %d slot %d partly valid", what, tile, q);
                                continue;
                            }
                            CHECK(q < Qmax, "%s: tile %d row %d behind the last slot", what, tile, s);
                            const int b = r.rng_zs >> 16, p = r.rng_p;
                            CHECK((r.rng_zs & 0xFFFF) == n, "%s: tile %d row %d holds sample %d", what, tile, s, r.rng_zs & 0xFFFF);
                            CHECK(b >= 0 && b < B && p >= 0 && p < P, "%s: row (%d, %d)", what, b, p);
                            if (!(b >= 0 && b < B && p >= 0 && p < P)) continue;
                            RowEnt d = t2[((size_t)b * N + n) * P + p];
                            d.pad1 = r.pad1;
                            CHECK(same_row(r, d), "%s: tile %d row %d is not the dense table's", what, tile, s);
                            ++seen[((size_t)b * N + n) * P + p];
                            CHECK(r.pad1 >= 0 && r.pad1 + 2 < XR_EXT_ROWS, "%s: extended row index %d", what, r.pad1);
                            if (r.pad1 < 0 || r.pad1 + 2 >= XR_EXT_ROWS) continue;
                            for (int ky = 0; ky < 3; ++ky)
                                for (int kx = 0; kx < 3; ++kx)
                                    CHECK((int64_t)e[r.pad1 + kx].x + (int64_t)ky * e[r.pad1 + kx].y == (int64_t)r.in_off + (int64_t)ky * r.in_pitch + kx,
                                          "%s: tile %d row %d tap (%d,%d)", what, tile, s, ky, kx);
                        }
                    }
                    for (size_t i = 0; i < seen.size(); ++i) {
                        const int b = (int)(i / ((size_t)N * P)), p = (int)(i % P);
                        const bool member = (flags[(size_t)b * P + p] & ST_TAIL) != 0;
                        CHECK(seen[i] == (member ? 1 : 0), "%s: (image %d, pixel %d) computed %d times", what, b, p, seen[i]);
                    }
                    ++configs;
                }
                if (dens == 0.18) {
                    const bool large = (long)hw[0] * hw[1] >= 512L * 512L;
                    std::printf("  %dx%d N=%d density 0.18: %ld tiles of 192 rows, %ld of 256%s\n", hw[0], hw[1], N, geo018[0], geo018[1],
                                large ? "" : " (small geometry: in the sum only)");
                    if (large)
                        CHECK((double)geo018[0] <= 1.02 * (double)geo018[1], "%dx%d N=%d density 0.18: %ld tiles of 192 rows against %ld of 256: more than 2 %% more",
                              hw[0], hw[1], N, geo018[0], geo018[1]);
                }
            }
        std::printf("N=%d density 0.18: %ld tiles of 192 rows, %ld of 256 (%+.2f %%)\n", N, tiles018[0], tiles018[1],
                    100.0 * ((double)tiles018[0] / (double)tiles018[1] - 1.0));
        CHECK((double)tiles018[0] <= 1.02 * (double)tiles018[1], "N=%d density 0.18: %ld tiles of 192 rows against %ld of 256: more than 2 %% more",
              N, tiles018[0], tiles018[1]);
    }
    std::printf("sparse_tables_rows_check: %ld configurations, %d failures\n", configs, failures);
    return failures ? 1 : 0;
}

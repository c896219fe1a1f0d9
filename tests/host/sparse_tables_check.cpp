// CPU replay of the sparse tail / halo row-table builder (bayes-od-rc_amd/csrc/sparse_tables.h, post_kernels.hip
// sparse_tail_rows_kernel), compiled with -fsanitize=address,undefined by tests/test_host_sparse_tables.py.  The kernel's phases run
// here in the same order with the same helper functions (256 "threads" for the run lists and their scan, one packer per table).
// Checked against brute force on several geometries and random keep sets, empty and full ones included:
//   - the tail table equals the one of the serial walk it replaced, row for row and extended row for extended row;
//   - every halo pixel appears once per sample, and the halo contains the 3x3 dilation of the tail's pixels inside each level;
//   - every row equals the dense per-sample table's row (head_row_tables' t2), apart from its extended-row index;
//   - the row-reuse invariants hold: each tap's staged element is the gathered one, a tile's first extended row is its smallest,
//     tiles hold all N samples of their pixels, tile counts stay within the closed-form capacity.
#include "sparse_tables.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>

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

struct Tables { std::vector<RowEnt> rows; std::vector<ExtRow> ext; int tiles = 0; };

static bool same_row(const RowEnt& a, const RowEnt& b) { return std::memcmp(&a, &b, sizeof(RowEnt)) == 0; }

// the serial walk the parallel builder replaced (one thread per image, adjacency from the row table)
static void serial_tail(const std::vector<uint8_t>& kept, const std::vector<RowEnt>& pix, int B, int N, int P, int64_t Ppad, Tables& out) {
    const int Qmax = 256 / N;
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
        out.rows.resize((size_t)out.tiles * 256);
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
                    out.rows[(size_t)t * 256 + (Q0 + k) * N + n] = q;
                }
            }
        }
        for (size_t t = 0; t < tiles.size(); ++t) {
            for (int r = tiles[t].y * N; r < 256; ++r) out.rows[(base + t) * 256 + r] = invalid;
            const RowEnt f = st_row(pix[tiles[t].x], b, 0, tiles[t].x, N, P, Ppad);
            for (int r = tiles[t].z; r < XR_EXT_ROWS; ++r) out.ext[(base + t) * XR_EXT_ROWS + r] = ExtRow{f.in_off, f.in_pitch};
        }
    }
}

// the kernel, phase by phase (post_kernels.hip sparse_tail_rows_kernel)
static void parallel_tables(const std::vector<uint8_t>& kept, const std::vector<RowEnt>& pix, const SparseLevels& lv, int B, int N, int P,
                            int64_t Ppad, Tables out[2], std::vector<uint8_t>& flags) {
    flags.assign((size_t)B * P, 0);
    const RowEnt invalid = st_invalid_row(pix[0]);
    for (int b = 0; b < B; ++b) {
        uint8_t* f = &flags[(size_t)b * P];
        for (int p = 0; p < P; ++p) f[p] = kept[(size_t)b * P + p] ? ST_KEPT : 0;
        for (int p = 0; p < P; ++p) if (st_member(f, lv, p, ST_KEPT)) f[p] |= ST_TAIL;
        for (int p = 0; p < P; ++p) if (st_dilated(f, lv, p)) f[p] |= ST_DIL;
        for (int p = 0; p < P; ++p) if (st_member(f, lv, p, ST_DIL)) f[p] |= ST_HALO;
        const int share = (P + 255) / 256;
        for (int t = 0; t < 2; ++t) {
            const uint8_t bit = t == 0 ? ST_TAIL : ST_HALO;
            int cnt[256], incl[256];
            for (int tid = 0; tid < 256; ++tid) {
                const int q0 = std::min(P, tid * share), q1 = std::min(P, q0 + share);
                cnt[tid] = 0;
                for (int p = q0; p < q1; ++p) cnt[tid] += st_run_edge(f, lv, p, bit) & 1;
            }
            for (int tid = 0, acc = 0; tid < 256; ++tid) { acc += cnt[tid]; incl[tid] = acc; }
            const int nrun = incl[255];
            std::vector<int32_t> rx((size_t)P, -1), ry((size_t)P, -1);
            for (int tid = 0; tid < 256; ++tid) {
                const int q0 = std::min(P, tid * share), q1 = std::min(P, q0 + share);
                int r = incl[tid] - cnt[tid];
                for (int p = q0; p < q1; ++p) {
                    const int edge = st_run_edge(f, lv, p, bit);
                    if (edge & 1) { CHECK(r < P, "run index %d", r); rx[r++] = p; }
                    if (edge & 2) { CHECK(r >= 1, "run end before a start at %d", p); if (r >= 1) ry[r - 1] = p; }
                }
            }
            std::vector<StQuad> chunks((size_t)P), tiles((size_t)P);
            StPack st{0, 0, 0, 0, 0, 0};
            for (int r = 0; r < nrun; ++r) {
                CHECK(rx[r] >= 0 && ry[r] >= rx[r], "run %d: [%d, %d]", r, rx[r], ry[r]);
                st_pack_run(st, rx[r], ry[r] - rx[r] + 1, N, chunks.data(), tiles.data(), true);
            }
            st_pack_close(st, tiles.data(), true);
            CHECK(st.nchunk <= P && st.ntile <= P, "scratch overflow: %d pieces, %d tiles for %d pixels", st.nchunk, st.ntile, P);
            Tables& o = out[t];
            const int base = o.tiles;
            o.tiles += st.ntile;
            o.rows.resize((size_t)o.tiles * 256);
            o.ext.resize((size_t)o.tiles * XR_EXT_ROWS);
            for (int i = 0; i < st.nchunk * N; ++i) {
                const int ci = i / N, n = i - ci * N;
                st_write_piece(chunks[ci], n, b, base + chunks[ci].y, pix.data(), N, P, Ppad, o.rows.data(), o.ext.data());
            }
            for (int i = 0; i < st.ntile * 256; ++i) {
                const int tt = i >> 8, r = i & 255;
                if (st_pad_row(tiles[tt], r, N)) o.rows[(size_t)(base + tt) * 256 + r] = invalid;
            }
            for (int i = 0; i < st.ntile * XR_EXT_ROWS; ++i) {
                const int tt = i / XR_EXT_ROWS, r = i - tt * XR_EXT_ROWS;
                if (r >= tiles[tt].z) o.ext[(size_t)(base + tt) * XR_EXT_ROWS + r] = st_pad_ext(tiles[tt], b, pix.data(), N, P, Ppad);
            }
        }
    }
}

int main() {
    const int sizes[][2] = {{512, 512}, {384, 1248}, {720, 1280}, {96, 160}, {100, 75}};
    const int samples[] = {2, 10, 30};
    const double densities[] = {0.0, 0.002, 0.02, 0.18, 0.6, 1.0};
    std::mt19937 rng(1234);
    long configs = 0, halo_rows_total = 0, dense_rows_total = 0;
    for (const auto& hw : sizes)
        for (int N : samples)
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
                Tables ref, got[2];
                serial_tail(kept, pix, B, N, P, g.Ppad, ref);
                std::vector<uint8_t> flags;
                parallel_tables(kept, pix, lv, B, N, P, g.Ppad, got, flags);
                const int cap = B * (P / st_min_pixels(N) + 1);
                char what[128];
                std::snprintf(what, sizeof what, "%dx%d N=%d density %.3f", hw[0], hw[1], N, dens);
                // the tail: exactly the serial walk's table
                CHECK(got[0].tiles == ref.tiles, "%s: tail %d tiles, serial walk %d", what, got[0].tiles, ref.tiles);
                if (got[0].tiles == ref.tiles) {
                    for (size_t i = 0; i < ref.rows.size(); ++i) CHECK(same_row(got[0].rows[i], ref.rows[i]), "%s: tail row %zu differs", what, i);
                    for (size_t i = 0; i < ref.ext.size(); ++i)
                        CHECK(got[0].ext[i].x == ref.ext[i].x && got[0].ext[i].y == ref.ext[i].y, "%s: tail extended row %zu differs", what, i);
                }
                for (int t = 0; t < 2; ++t) CHECK(got[t].tiles <= cap, "%s: table %d: %d tiles over the capacity %d", what, t, got[t].tiles, cap);
                // brute force: tail pixels (from the serial table), their 3x3 dilation inside each level
                std::vector<uint8_t> tail((size_t)B * P, 0), dil((size_t)B * P, 0);
                for (const RowEnt& r : ref.rows)
                    if (r.out_off >= 0) tail[(size_t)(r.rng_zs >> 16) * P + r.rng_p] = 1;
                for (int b = 0; b < B; ++b)
                    for (int l = 0; l < 5; ++l)
                        for (int y = 0; y < g.lh[l]; ++y)
                            for (int x = 0; x < g.lw[l]; ++x) {
                                if (!tail[(size_t)b * P + g.lvl_p0[l] + y * g.lw[l] + x]) continue;
                                for (int yy = std::max(0, y - 1); yy <= std::min(g.lh[l] - 1, y + 1); ++yy)
                                    for (int xx = std::max(0, x - 1); xx <= std::min(g.lw[l] - 1, x + 1); ++xx)
                                        dil[(size_t)b * P + g.lvl_p0[l] + yy * g.lw[l] + xx] = 1;
                            }
                for (size_t i = 0; i < tail.size(); ++i) {
                    CHECK(!!(flags[i] & ST_TAIL) == !!tail[i], "%s: pixel %zu tail flag %d, serial walk %d", what, i, flags[i] & ST_TAIL, tail[i]);
                    CHECK(!!(flags[i] & ST_DIL) == !!dil[i], "%s: pixel %zu dilation flag %d, brute force %d", what, i, flags[i] & ST_DIL, dil[i]);
                }
                // both tables: every row the dense table's, each (image, sample, pixel) once, the row-reuse invariants
                const int64_t in_pixels = (int64_t)B * N * g.Ppad;
                for (int t = 0; t < 2; ++t) {
                    const Tables& T = got[t];
                    std::vector<int> seen((size_t)B * N * P, 0);
                    for (int tile = 0; tile < T.tiles; ++tile) {
                        const ExtRow* e = &T.ext[(size_t)tile * XR_EXT_ROWS];
                        for (int q = 0; q < XR_EXT_ROWS; ++q) {
                            CHECK(e[q].x >= e[0].x, "%s: table %d tile %d extended row %d below the first", what, t, tile, q);
                            CHECK(e[q].x >= 0 && (int64_t)e[q].x + 2 * (int64_t)e[q].y < in_pixels, "%s: table %d tile %d extended row %d outside the planes", what, t, tile, q);
                        }
                        for (int s = 0; s < 256; ++s) {
                            const RowEnt& r = T.rows[(size_t)tile * 256 + s];
                            const int q = s / N, n = s - q * N;
                            if (r.out_off < 0) {
                                if (q < 256 / N) CHECK(T.rows[(size_t)tile * 256 + q * N].out_off < 0, "%s: table %d tile %d slot %d partly valid", what, t, tile, q);
                                continue;
                            }
                            CHECK(q < 256 / N, "%s: table %d tile %d row %d behind the last slot", what, t, tile, s);
                            const int b = r.rng_zs >> 16, p = r.rng_p;
                            CHECK((r.rng_zs & 0xFFFF) == n, "%s: table %d tile %d row %d holds sample %d", what, t, tile, s, r.rng_zs & 0xFFFF);
                            CHECK(b >= 0 && b < B && p >= 0 && p < P, "%s: table %d row (%d, %d)", what, t, b, p);
                            if (!(b >= 0 && b < B && p >= 0 && p < P)) continue;
                            RowEnt d = t2[((size_t)b * N + n) * P + p];
                            d.pad1 = r.pad1;
                            CHECK(same_row(r, d), "%s: table %d tile %d row %d is not the dense table's", what, t, tile, s);
                            ++seen[((size_t)b * N + n) * P + p];
                            CHECK(r.pad1 >= 0 && r.pad1 + 2 < XR_EXT_ROWS, "%s: table %d extended row index %d", what, t, r.pad1);
                            if (r.pad1 < 0 || r.pad1 + 2 >= XR_EXT_ROWS) continue;
                            for (int ky = 0; ky < 3; ++ky)
                                for (int kx = 0; kx < 3; ++kx)
                                    CHECK((int64_t)e[r.pad1 + kx].x + (int64_t)ky * e[r.pad1 + kx].y == (int64_t)r.in_off + (int64_t)ky * r.in_pitch + kx,
                                          "%s: table %d tile %d row %d tap (%d,%d)", what, t, tile, s, ky, kx);
                        }
                    }
                    for (int b = 0; b < B; ++b)
                        for (int n = 0; n < N; ++n)
                            for (int p = 0; p < P; ++p) {
                                const int c = seen[((size_t)b * N + n) * P + p];
                                const bool member = t == 0 ? tail[(size_t)b * P + p] : (flags[(size_t)b * P + p] & ST_HALO);
                                CHECK(c == (member ? 1 : 0), "%s: table %d (%d, %d, %d) computed %d times", what, t, b, n, p, c);
                                if (t == 1 && dil[(size_t)b * P + p]) CHECK(c == 1, "%s: dilation pixel (%d, %d) not in the halo", what, b, p);
                            }
                }
                halo_rows_total += (long)got[1].tiles * 256;
                dense_rows_total += (long)B * N * P;
                ++configs;
            }
    std::printf("sparse_tables_check: %ld configurations, halo rows / dense rows %.3f, %d failures\n", configs,
                (double)halo_rows_total / (double)dense_rows_total, failures);
    return failures ? 1 : 0;
}

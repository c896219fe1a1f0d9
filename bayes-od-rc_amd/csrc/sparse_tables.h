// Device-built row tables of the sparse tail and its halo (kernels.h SparseTailArgs, post_kernels.hip sparse_tail_rows_kernel):
// the per-pixel rules and the per-piece writes, in plain C++ that the kernel and the host sanitizer build of
// tests/host/sparse_tables_check.cpp both run.
//
// One image at a time, over its P pyramid pixels in dense order (level, y, x) with one flag byte per pixel:
//   ST_KEPT  the pixel has a kept anchor
//   ST_TAIL  the tail computes it: kept, or an unkept pixel between two kept, x-adjacent ones (a run of three costs fewer extended
//            rows than two runs of one)
//   ST_DIL   the 3x3 dilation of the ST_TAIL pixels inside their pyramid level: the pixels the tail's windows read
//   ST_HALO  the halo launch computes it: ST_DIL, or a single pixel between two ST_DIL ones in a row (taken along as above)
// Each flag depends only on the flags before it, so a phase may set its bit while other threads read the older bits.
// A table is the list of maximal runs of x-adjacent member pixels, cut into pieces and packed, in pixel order, into sample-complete
// tiles of at most R / N pixel slots and XR_EXT_ROWS extended rows (the rules of xr_tile_rows_aggregated, plan_tables.h).  R is the
// tile height in rows: 256 (the halo table, and every call that does not name it) or 192 (the tail table: its tiles close on their
// extended rows at about 15 of 25 slots, so three 16-row pixel fragments per wave hold them as well as four).
#pragma once
#include "plan_tables.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define ST_HD __host__ __device__
#else
#define ST_HD
#endif

enum : uint8_t { ST_KEPT = 1, ST_TAIL = 2, ST_DIL = 4, ST_HALO = 8 };

struct SparseLevels {                     // the pyramid levels of one image in dense pixel order
    int32_t n;
    int32_t lw[5], lh[5];
    int32_t p0[5];                        // dense pixel index of each level's first pixel
};

struct alignas(16) StQuad { int32_t x, y, z, w; };      // the layout of HIP's int4

// pieces: {first pixel, tile (image-local), first slot, first extended row | pixels << 16}; tiles: {first pixel, slots used,
// extended rows used, -}
struct StPack { int32_t Q, X, first, open, nchunk, ntile; };

ST_HD inline void st_level_x(const SparseLevels& g, int p, int& l, int& y, int& x) {
    l = 0;
    while (l + 1 < g.n && p >= g.p0[l + 1]) ++l;
    const int q = p - g.p0[l];
    y = q / g.lw[l];
    x = q - y * g.lw[l];
}

// member of the table whose source flag is `bit`: the pixel itself, or a single gap between two x-adjacent ones
ST_HD inline bool st_member(const uint8_t* f, const SparseLevels& g, int p, uint8_t bit) {
    if (f[p] & bit) return true;
    int l, y, x;
    st_level_x(g, p, l, y, x);
    return x > 0 && x + 1 < g.lw[l] && (f[p - 1] & bit) && (f[p + 1] & bit);
}

ST_HD inline bool st_dilated(const uint8_t* f, const SparseLevels& g, int p) {
    int l, y, x;
    st_level_x(g, p, l, y, x);
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= g.lh[l]) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= g.lw[l]) continue;
            if (f[g.p0[l] + yy * g.lw[l] + xx] & ST_TAIL) return true;
        }
    }
    return false;
}

// run boundaries of the members flagged `bit`: 1 starts a run, 2 ends one (3: both)
ST_HD inline int st_run_edge(const uint8_t* f, const SparseLevels& g, int p, uint8_t bit) {
    if (!(f[p] & bit)) return 0;
    int l, y, x;
    st_level_x(g, p, l, y, x);
    return ((x == 0 || !(f[p - 1] & bit)) ? 1 : 0) | ((x + 1 == g.lw[l] || !(f[p + 1] & bit)) ? 2 : 0);
}

// the packing of one run [p, p + L): identical to the serial walk it replaced (pieces cut by free slots and free extended rows)
ST_HD inline void st_pack_run(StPack& s, int p, int L, int N, StQuad* chunks, StQuad* tiles, bool write, int R = 256) {
    const int Qmax = R / N;
    while (L > 0) {
        if (!s.open) { s.first = p; s.Q = 0; s.X = 0; s.open = 1; }
        int take = L < Qmax - s.Q ? L : Qmax - s.Q;
        const int room = (XR_EXT_ROWS - s.X) / N - 2;
        take = take < room ? take : room;
        if (take < 1) {
            if (write) tiles[s.ntile] = StQuad{s.first, s.Q, s.X, 0};
            ++s.ntile; s.open = 0;
            continue;
        }
        if (write) chunks[s.nchunk] = StQuad{p, s.ntile, s.Q, s.X | (take << 16)};
        ++s.nchunk;
        s.X += N * (take + 2); s.Q += take; p += take; L -= take;
        if (s.Q == Qmax) {
            if (write) tiles[s.ntile] = StQuad{s.first, s.Q, s.X, 0};
            ++s.ntile; s.open = 0;
        }
    }
}

ST_HD inline void st_pack_close(StPack& s, StQuad* tiles, bool write) {
    if (!s.open) return;
    if (write) tiles[s.ntile] = StQuad{s.first, s.Q, s.X, 0};
    ++s.ntile; s.open = 0;
}

// the dense per-sample table's row (head_row_tables' t2) of image b, sample n, pixel p; pix_p = that of image 0, sample 0
ST_HD inline RowEnt st_row(const RowEnt& pix_p, int b, int n, int p, int N, int P, int64_t Ppad) {
    RowEnt e = pix_p;
    const int32_t plane = (int32_t)(((int64_t)b * N + n) * Ppad);
    e.in_off += plane;
    e.out_off += plane;
    e.rng_zs = n | (b << 16);
    e.pad0 = (int32_t)(((int64_t)b * N + n) * P + p);
    return e;
}

// sample n of piece c: take + 2 extended rows and take rows of tile `tile` (global index; R rows per tile)
ST_HD inline void st_write_piece(const StQuad& c, int n, int b, int tile, const RowEnt* pix, int N, int P, int64_t Ppad,
                                 RowEnt* rows, ExtRow* ext, int R = 256) {
    const int p0 = c.x, Q0 = c.z, X0 = c.w & 0xFFFF, take = c.w >> 16;
    const int x0 = X0 + n * (take + 2);
    const RowEnt first = st_row(pix[p0], b, n, p0, N, P, Ppad);
    ExtRow* e = ext + (size_t)tile * XR_EXT_ROWS + x0;
    for (int k = 0; k < take + 2; ++k) e[k] = ExtRow{first.in_off + k, first.in_pitch};
    RowEnt* r = rows + (size_t)tile * R;
    for (int k = 0; k < take; ++k) {
        RowEnt q = st_row(pix[p0 + k], b, n, p0 + k, N, P, Ppad);
        q.pad1 = x0 + k;
        r[(Q0 + k) * N + n] = q;
    }
}

// padding of tile t (image-local tile info ti): rows behind the last slot are invalid, extended rows behind the last one repeat the
// tile's first (never read by a valid row, and it keeps the first entry the smallest)
ST_HD inline bool st_pad_row(const StQuad& ti, int r, int N) { return r >= ti.y * N; }
ST_HD inline RowEnt st_invalid_row(const RowEnt& pix0) {
    RowEnt e = pix0;
    e.out_off = -1; e.pad0 = 0; e.pad1 = 0;
    return e;
}
ST_HD inline ExtRow st_pad_ext(const StQuad& ti, int b, const RowEnt* pix, int N, int P, int64_t Ppad) {
    const RowEnt first = st_row(pix[ti.x], b, 0, ti.x, N, P, Ppad);
    return ExtRow{first.in_off, first.in_pitch};
}

// fewest pixels a tile closed before the image's end holds: closed when its slots are full or when a piece of one pixel (3N extended
// rows) no longer fits; a piece of k pixels costs N * (k + 2) <= 3N * k extended rows.  Bounds the tiles of both tables.
// (The extended-row term, about 106 / N, is below 192 / N for every N: 192-row tiles have the same bound -- the planner checks.)
inline int st_min_pixels(int N, int R = 256) {
    const int Qmax = R / N;
    return std::max(1, std::min(Qmax, (XR_EXT_ROWS - 3 * N) / (3 * N) + 1));
}

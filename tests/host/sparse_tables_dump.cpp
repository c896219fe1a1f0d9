// Prints what bayes-od-rc_amd/csrc/sparse_tables.h makes of given keep masks: the pixel flags, the pieces and the tiles of the tail and
// the halo table, by the header's own functions in the order sparse_tail_rows_kernel (post_kernels.hip) runs them -- flags, run edges,
// st_pack_run per run, st_pack_close.  tests/test_sparse_tables_reference_host.py compiles it with -fsanitize=address,undefined and
// holds the output against the Python restatement (tests/sparse_tables_reference.py).
//
// Input (a file, argv[1]): any number of cases, each
//   <levels> <N> <tail tile rows>   then <width> <height> per level   then the mask, one character 0 / 1 per pixel, as one word
// Output per case:
//   case <P> <st_min_pixels(N)> <st_min_pixels(N, tail rows)>
//   flags <one hex digit per pixel>
//   table <0 tail | 1 halo> <runs> <pieces> <tiles>
//   run <first pixel> <pixels>                                                 (per run)
//   piece <first pixel> <tile> <first slot> <first extended row> <pixels>      (per piece)
//   tile <first pixel> <slots used> <extended rows used>                       (per tile)
#include "sparse_tables.h"
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: sparse_tables_dump <cases file>\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    int nlev, N, R;
    while (in >> nlev >> N >> R) {
        if (nlev < 1 || nlev > 5 || N < 1 || XR_EXT_ROWS / N - 2 < 1 || (R != 192 && R != 256) || R / N < 1) { std::fprintf(stderr, "bad case header\n"); return 2; }
        SparseLevels lv{};
        lv.n = nlev;
        int P = 0;
        for (int l = 0; l < nlev; ++l) {
            if (!(in >> lv.lw[l] >> lv.lh[l]) || lv.lw[l] < 1 || lv.lh[l] < 1) { std::fprintf(stderr, "bad level\n"); return 2; }
            lv.p0[l] = P;
            P += lv.lw[l] * lv.lh[l];
        }
        std::string mask;
        if (!(in >> mask) || (int)mask.size() != P) { std::fprintf(stderr, "mask of %zu characters for %d pixels\n", mask.size(), P); return 2; }
        std::vector<uint8_t> f((size_t)P);
        for (int p = 0; p < P; ++p) f[p] = mask[p] == '1' ? ST_KEPT : 0;
        for (int p = 0; p < P; ++p) if (st_member(f.data(), lv, p, ST_KEPT)) f[p] |= ST_TAIL;
        for (int p = 0; p < P; ++p) if (st_dilated(f.data(), lv, p)) f[p] |= ST_DIL;
        for (int p = 0; p < P; ++p) if (st_member(f.data(), lv, p, ST_DIL)) f[p] |= ST_HALO;
        std::printf("case %d %d %d\nflags ", P, st_min_pixels(N), st_min_pixels(N, R));
        for (int p = 0; p < P; ++p) std::printf("%x", f[p]);
        std::printf("\n");
        for (int t = 0; t < 2; ++t) {
            const uint8_t bit = t == 0 ? ST_TAIL : ST_HALO;
            const int rows = t == 0 ? R : 256;
            std::vector<int> first, last;
            for (int p = 0; p < P; ++p) {
                const int edge = st_run_edge(f.data(), lv, p, bit);
                if (edge & 1) first.push_back(p);
                if (edge & 2) {
                    if (last.size() + 1 != first.size()) { std::fprintf(stderr, "run end at %d without a start\n", p); return 1; }
                    last.push_back(p);
                }
            }
            if (first.size() != last.size()) { std::fprintf(stderr, "a run without an end\n"); return 1; }
            std::vector<StQuad> chunks((size_t)P), tiles((size_t)P);       // the kernel's scratch: P entries per image and table
            StPack st{0, 0, 0, 0, 0, 0};
            for (size_t r = 0; r < first.size(); ++r) {
                // (st_pack_run writes without a bound: a run holds at least one pixel, a piece and a tile too, so P entries hold)
                st_pack_run(st, first[r], last[r] - first[r] + 1, N, chunks.data(), tiles.data(), true, rows);
                if (st.nchunk > P || st.ntile >= P + 1) { std::fprintf(stderr, "scratch overflow\n"); return 1; }
            }
            st_pack_close(st, tiles.data(), true);
            std::printf("table %d %zu %d %d\n", t, first.size(), st.nchunk, st.ntile);
            for (size_t r = 0; r < first.size(); ++r) std::printf("run %d %d\n", first[r], last[r] - first[r] + 1);
            for (int i = 0; i < st.nchunk; ++i)
                std::printf("piece %d %d %d %d %d\n", chunks[i].x, chunks[i].y, chunks[i].z, chunks[i].w & 0xFFFF, chunks[i].w >> 16);
            for (int i = 0; i < st.ntile; ++i) std::printf("tile %d %d %d\n", tiles[i].x, tiles[i].y, tiles[i].z);
        }
    }
    return 0;
}

// The two JPEG kernels alone, timed with events against their byte floors: 64 frames of 720x1280, 4:2:0, with
// random small coefficients (the kernels' work does not depend on the values).  Links against the built library:
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -Ibayes-od-rc_amd/csrc tests/tools/jpeg_kernel_time.hip \
//         -Lbayes-od-rc_amd/lib -lbayesod_hip -Wl,-rpath,'$ORIGIN/../bayes-od-rc_amd/lib' -o <dir beside the package>/jpeg_kernel_time
// Floors: jpeg_idct_kernel moves 128 B in + 64 B out per block; jpeg_color_kernel reads each plane byte once (1.5 B per pixel at
// 4:2:0) and writes 3 B per pixel; HBM at the 6.29 TB/s a float4 copy measures.
#include "kernels.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(e) do { hipError_t _e = (e); if (_e != hipSuccess) { fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(_e)); return 1; } } while (0)

int main() {
    const int n = 64, W = 1280, H = 720, hs = 2, vs = 2;
    const int mx = (W + 8 * hs - 1) / (8 * hs), my = (H + 8 * vs - 1) / (8 * vs);
    std::vector<JpegFrame> fr(n);
    int64_t coefs = 0, planes = 0, rgb = 0, blocks = 0, groups = 0;
    for (int i = 0; i < n; ++i) {
        JpegFrame& f = fr[i];
        f = JpegFrame{};
        for (int c = 0; c < 3; ++c) {
            f.bw[c] = mx * (c == 0 ? hs : 1); f.bh[c] = my * (c == 0 ? vs : 1);
            f.coef_off[c] = coefs; f.plane_off[c] = planes;
            coefs += (int64_t)f.bw[c] * f.bh[c] * 64; planes += (int64_t)f.bw[c] * f.bh[c] * 64;
            for (int k = 0; k < 64; ++k) f.quant[c][k] = (uint16_t)(3 + k / 4);
        }
        f.rgb_off = rgb;
        f.components = 3; f.h_samp = hs; f.v_samp = vs; f.width = W; f.height = H;
        blocks = coefs / 64; groups += (int64_t)H * ((W + 3) / 4); rgb += (int64_t)3 * W * H;
    }
    std::vector<int16_t> hc((size_t)coefs);
    srand(1);
    for (int64_t i = 0; i < coefs; ++i) hc[(size_t)i] = (i % 64 == 0) ? (int16_t)(rand() % 200 - 100) : (int16_t)((rand() % 8 == 0) ? rand() % 21 - 10 : 0);
    JpegFrame* d_fr; int16_t* d_c; uint8_t *d_p, *d_rgb;
    CHECK(hipMalloc(&d_fr, n * sizeof(JpegFrame))); CHECK(hipMalloc(&d_c, (size_t)coefs * 2));
    CHECK(hipMalloc(&d_p, (size_t)planes)); CHECK(hipMalloc(&d_rgb, (size_t)rgb));
    CHECK(hipMemcpy(d_fr, fr.data(), n * sizeof(JpegFrame), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_c, hc.data(), (size_t)coefs * 2, hipMemcpyHostToDevice));
    JpegArgs a{};
    a.frames = d_fr; a.coefs = d_c; a.planes = d_p; a.rgb = d_rgb; a.n = n;
    a.idct_wgs_per_frame = (int32_t)((blocks / n + 31) / 32); a.color_wgs_per_frame = (int32_t)((groups / n + 255) / 256);       // equal frames
    hipStream_t s; CHECK(hipStreamCreate(&s));
    hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    const double idct_bytes = (double)blocks * 192.0, color_bytes = (double)planes + (double)rgb, hbm = 6.29e12;
    const int iters = 20;
    for (int rep = 0; rep < 3; ++rep) {
        float ms_i = 0, ms_c = 0;
        CHECK(launch_jpeg_idct(a, s)); CHECK(launch_jpeg_color(a, s));
        CHECK(hipEventRecord(e0, s));
        for (int i = 0; i < iters; ++i) CHECK(launch_jpeg_idct(a, s));
        CHECK(hipEventRecord(e1, s)); CHECK(hipEventSynchronize(e1)); CHECK(hipEventElapsedTime(&ms_i, e0, e1));
        CHECK(hipEventRecord(e0, s));
        for (int i = 0; i < iters; ++i) CHECK(launch_jpeg_color(a, s));
        CHECK(hipEventRecord(e1, s)); CHECK(hipEventSynchronize(e1)); CHECK(hipEventElapsedTime(&ms_c, e0, e1));
        ms_i /= iters; ms_c /= iters;
        printf("rep %d  jpeg_idct_kernel  %.3f ms for %lld blocks: %.2f TB/s of its %.1f MB, floor %.3f ms (%.0f %% of it)\n", rep, ms_i, (long long)blocks,
               idct_bytes / ms_i / 1e9, idct_bytes / 1e6, idct_bytes / hbm * 1e3, 100.0 * idct_bytes / hbm * 1e3 / ms_i);
        printf("rep %d  jpeg_color_kernel %.3f ms for %d frames of %dx%d: %.2f TB/s of its %.1f MB, floor %.3f ms (%.0f %% of it)\n", rep, ms_c, n, H, W,
               color_bytes / ms_c / 1e9, color_bytes / 1e6, color_bytes / hbm * 1e3, 100.0 * color_bytes / hbm * 1e3 / ms_c);
    }
    (void)hipFree(d_fr); (void)hipFree(d_c); (void)hipFree(d_p); (void)hipFree(d_rgb);
    return 0;
}

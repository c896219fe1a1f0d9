// Host side of libbayesod_hip.so: handle, HBM plan, weight folding/packing, launch sequencing and
// the C ABI of include/bayesod.h.  Mirrors, stage for stage, the call stack of
// src/retina_net/experiments/run_inference.py:137-149 -> inference_utils.bayes_od_inference
// -> RetinaNetModel.call.
#include "../../include/bayesod.h"
#include "kernels.h"
#include "plane_tables.h"
#include "record_state.h"
#include "jpeg_entropy.h"
#include "png_inflate.h"
#include "render_font.h"

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <tuple>
#include <type_traits>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <system_error>
#include <vector>
#include <dlfcn.h>

namespace {

constexpr float BN_EPS = 1e-3f;   // keras BatchNormalization default

thread_local std::string g_create_error;

struct HostTensor { std::vector<int64_t> shape; std::vector<float> data; };

struct Plane {               // NHWC view (bf16, or fp32 in fp32 precision mode) with a 1-pixel zero border
    char* d = nullptr;
    int64_t base = 0;        // pixel offset of this view inside d
    int64_t bstride = 0;     // pixels between consecutive batch items
    int h = 0, w = 0, C = 0, pitch = 0;
};

struct PackedConv { char* w = nullptr; float* bias = nullptr; int cout = 0, cout_pad = 0, taps = 0, kw = 0, cin = 0; };

struct Op {
    enum Kind { STEM, POOL, CONV, KEEP } kind;      // KEEP: the posterior's keep flags + the sparse tail's row table (build_plan)
    ConvArgs conv;
    bool is_head3x3 = false;
    double flops = 0;
    std::string name;
    std::string wname[3], bnname[3];     // per group: conv / batch-norm layer names (training: parameter lookup)
    bool same_geom = false;              // 3x3 stride-1 SAME with identically laid-out input / output planes (training: input gradient as a convolution)
    // The last tower layers exist in two flavours when the MC aggregation is fused into their epilogue: FLAVOUR_RAW writes the
    // per-sample head outputs [B,N,A,.] (bod_forward, sample sharding, parity tests), FLAVOUR_AGG reduces them over the
    // samples inside the tile (bod_infer).  0 = the op belongs to both.
    int flavour = 0;
    int head[3] = {-1, -1, -1};          // per group: BOD_HEAD_* whose raw buffer the fused 1x1 writes (raw buffers are allocated lazily)
    bool hx_pyramid = false;             // f16mx: this launch (the first tower layer) reads the pyramid as hx rows -- converted right in front of it
    // Sparse halo (build_plan): a raw forward runs layers 1 and 2 as before (RAW_FORWARD: skipped by materialise_raw, whose
    // activations of the other heads are no longer the layers' inputs); materialise_raw re-runs only the two halo convs (RAW_RERUN)
    enum { ANY_RAW = 0, RAW_FORWARD = 1, RAW_RERUN = 2 };
    int raw_use = ANY_RAW;
};
enum { FLAVOUR_BOTH = 0, FLAVOUR_RAW = 1, FLAVOUR_AGG = 2 };

uint16_t f2bf(float f) {
    uint32_t u; std::memcpy(&u, &f, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
float bf2f(uint16_t v) { uint32_t u = (uint32_t)v << 16; float f; std::memcpy(&f, &u, 4); return f; }

// ---- f16mx precision: the "hx" row of conv_igemm.hip (header there), packed on the host for weights (and for the test entry
// point's activations): float -> IEEE half, round to nearest even, subnormals kept (the f16 MFMA honours them:
// profiles/round5_mx_probe.txt)
uint16_t f2h(float f) {
    uint32_t u; std::memcpy(&u, &f, 4);
    const uint32_t sign = (u >> 16) & 0x8000u;
    u &= 0x7FFFFFFFu;
    if (u >= 0x47800000u) return (uint16_t)(sign | (u > 0x7F800000u ? 0x7E00u : 0x7C00u));      // >= 65536: inf (NaN stays NaN)
    if (u < 0x38800000u) {                         // below 2^-14: subnormal half = round(|f| * 2^24)
        float a; std::memcpy(&a, &u, 4);
        return (uint16_t)(sign | (uint32_t)std::nearbyint(a * 16777216.0f));
    }
    u += 0xFFFu + ((u >> 13) & 1u);                // round the 13 dropped mantissa bits to nearest even
    return (uint16_t)(sign | ((u - 0x38000000u) >> 13));      // (a mantissa carry runs into the exponent, up to inf, correctly)
}
float h2f(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
    float f;
    if (e == 0) { f = (float)m * (1.0f / 16777216.0f); uint32_t u; std::memcpy(&u, &f, 4); u |= sign; std::memcpy(&f, &u, 4); return f; }
    const uint32_t u = sign | ((e == 31 ? 255u : e + 112u) << 23) | (m << 13);
    std::memcpy(&f, &u, 4);
    return f;
}
// e2m3 (OCP fp6, bias 1): round to nearest even, saturating at 7.5
uint32_t f2e2m3(float x) {
    const uint32_t sign = std::signbit(x) ? 32u : 0u;
    const float a = std::fabs(x);
    uint32_t code;
    if (a < 1.0f) code = (uint32_t)std::nearbyint(a * 8.0f);
    else if (a < 2.0f) code = 8u + (uint32_t)std::nearbyint((a - 1.0f) * 8.0f);
    else if (a < 4.0f) code = 16u + (uint32_t)std::nearbyint((a - 2.0f) * 4.0f);
    else code = 24u + (uint32_t)std::nearbyint((std::min(a, 7.5f) - 4.0f) * 2.0f);
    return sign | std::min(code, 31u);
}
float e2m3_to_f(uint32_t c) {
    const uint32_t e = (c >> 3) & 3u, m = c & 7u;
    const float r = e == 0 ? m / 8.0f : std::ldexp(1.0f + m / 8.0f, (int)e - 1);
    return (c & 32u) ? -r : r;
}
// One hx row: C channels (multiple of 64) -> 4 C bytes.  Per 64 channels: H chunk = 64 f16 hi; X chunk = four 32-byte slots (m, b),
// pieces at X offsets 64m + 16b and 64m + 32 + 16b; a slot = the 16 channels 32m + 8 g4 + 4b + r as 32 e2m3 elements under one scale
// 2^(eb - 127), eb = biased exponent of (max(|v|, 2^-14) * 16/15) - 2: element 2k = hi6 (weights: lo6'), 2k + 1 = lo6' (weights:
// hi6), lo' = (v - hi) * 2^11; scale byte at byte 28 of the slot (weights: eb - 11, which undoes the 2^11 of both cross products).
void pack_hx_row(const float* v, int C, uint8_t* dst, bool weights) {
    std::memset(dst, 0, (size_t)C * 4);
    for (int q = 0; q < C / 64; ++q) {
        uint8_t* H = dst + (size_t)q * 256;
        uint8_t* X = H + 128;
        for (int c = 0; c < 64; ++c) { const uint16_t hb = f2h(v[q * 64 + c]); std::memcpy(H + 2 * c, &hb, 2); }
        for (int m = 0; m < 2; ++m)
            for (int b = 0; b < 2; ++b) {
                float hi[16], lo[16], mx = 6.103515625e-05f;
                for (int k = 0; k < 16; ++k) {
                    const float x = v[q * 64 + 32 * m + 8 * (k >> 2) + 4 * b + (k & 3)];
                    hi[k] = h2f(f2h(x)); lo[k] = (x - hi[k]) * 2048.0f;
                    mx = std::max(mx, std::fabs(x));
                }
                const float mxs = mx * 1.0666667f;
                uint32_t ub; std::memcpy(&ub, &mxs, 4);
                const uint32_t eb = (ub >> 23) - 2u;
                const float inv = std::ldexp(1.0f, 127 - (int)eb);
                uint8_t slot[32] = {0};
                for (int k = 0; k < 16; ++k) {
                    const uint32_t h6 = f2e2m3(hi[k] * inv), l6 = f2e2m3(lo[k] * inv);
                    const uint32_t e0 = weights ? l6 : h6, e1 = weights ? h6 : l6;
                    const int bit0 = 12 * k;
                    for (int t = 0; t < 6; ++t) {
                        if ((e0 >> t) & 1u) slot[(bit0 + t) >> 3] |= (uint8_t)(1u << ((bit0 + t) & 7));
                        if ((e1 >> t) & 1u) slot[(bit0 + 6 + t) >> 3] |= (uint8_t)(1u << ((bit0 + 6 + t) & 7));
                    }
                }
                slot[28] = (uint8_t)(weights ? eb - 11u : eb);
                std::memcpy(X + 64 * m + 16 * b, slot, 16);
                std::memcpy(X + 64 * m + 32 + 16 * b, slot + 16, 16);
            }
    }
}
// ... and back (test entry point: the epilogue's hx output): value = hi + lo' * 2^-11 with lo' from the slot's odd elements
void unpack_hx_row(const uint8_t* src, int C, float* v) {
    for (int q = 0; q < C / 64; ++q) {
        const uint8_t* H = src + (size_t)q * 256;
        const uint8_t* X = H + 128;
        for (int m = 0; m < 2; ++m)
            for (int b = 0; b < 2; ++b) {
                uint8_t slot[32];
                std::memcpy(slot, X + 64 * m + 16 * b, 16);
                std::memcpy(slot + 16, X + 64 * m + 32 + 16 * b, 16);
                const float sc = std::ldexp(1.0f, (int)slot[28] - 127);
                for (int k = 0; k < 16; ++k) {
                    const int c = 32 * m + 8 * (k >> 2) + 4 * b + (k & 3);
                    uint16_t hb; std::memcpy(&hb, H + 2 * c, 2);
                    uint32_t l6 = 0;
                    for (int t = 0; t < 6; ++t) l6 |= (uint32_t)((slot[(12 * k + 6 + t) >> 3] >> ((12 * k + 6 + t) & 7)) & 1u) << t;
                    v[q * 64 + c] = h2f(hb) + e2m3_to_f(l6) * sc * (1.0f / 2048.0f);
                }
            }
    }
}

// e2m1 (OCP MX fp4): round to nearest even, saturating at 6; code = sign(1) exp(2) mant(1), bias 1, subnormal step 0.5
uint32_t f2e2m1(float x) {
    const uint32_t s = std::signbit(x) ? 8u : 0u;
    float a = std::fabs(x);
    if (!(a == a)) return s;
    if (a >= 6.0f) return s | 7u;
    static const float grid[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
    uint32_t best = 0;
    for (uint32_t c = 0; c < 7; ++c) {
        const float mid = 0.5f * (grid[c] + grid[c + 1]);
        if (a > mid || (a == mid && (c & 1u))) best = c + 1;          // ties to the even code
    }
    return s | best;
}
float e2m1_to_f(uint32_t c) {
    static const float grid[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
    return (c & 8u) ? -grid[c & 7u] : grid[c & 7u];
}
// One h4 row (f16mx4): C = 256 channels -> 1 024 bytes in eight 128-byte chunks: [H0 H1 X0 H2 H3 X1 S -].  Hq = the 64 f16 hi of channels
// 64q..; Xx = the cross-term elements of channels 128x..: piece 2 ks + half (16 bytes) = the MX block of the 16 channels
// 128x + 32 ks + 8 g4 + 4 half + r as 32 e2m1 nibbles, nibble 2k = hi4 (weights: lo4'), 2k + 1 = lo4' (weights: hi4), k = 4 g4 + r,
// lo' = (v - hi) * 2^11, under the block's scale 2^(eb - 127), eb = biased exponent of (max(|hi|, 2^-14) * 4/3) - 2; S: byte
// 8x + 4 half + ks = eb (weights: eb - 11).
void pack_h4_row(const float* v, int C, uint8_t* dst, bool weights) {
    std::memset(dst, 0, (size_t)C * 4);
    for (int q = 0; q < C / 64; ++q) {
        uint8_t* H = dst + (size_t)(3 * (q >> 1) + (q & 1)) * 128;
        for (int c = 0; c < 64; ++c) { const uint16_t hb = f2h(v[q * 64 + c]); std::memcpy(H + 2 * c, &hb, 2); }
    }
    for (int x = 0; x < C / 128; ++x)
        for (int ks = 0; ks < 4; ++ks)
            for (int b = 0; b < 2; ++b) {
                float hi[16], lo[16], mx = 6.103515625e-05f;
                for (int k = 0; k < 16; ++k) {
                    const float xv = v[128 * x + 32 * ks + 8 * (k >> 2) + 4 * b + (k & 3)];
                    hi[k] = h2f(f2h(xv)); lo[k] = (xv - hi[k]) * 2048.0f;
                    mx = std::max(mx, std::fabs(hi[k]));
                }
                const float mxs = mx * 1.3333334f;
                uint32_t ub; std::memcpy(&ub, &mxs, 4);
                const uint32_t eb = (ub >> 23) - 2u;
                const float inv = std::ldexp(1.0f, 127 - (int)eb);
                uint8_t* piece = dst + (size_t)(3 * x + 2) * 128 + (2 * ks + b) * 16;
                for (int k = 0; k < 16; ++k) {
                    const uint32_t h4 = f2e2m1(hi[k] * inv), l4 = f2e2m1(lo[k] * inv);
                    piece[k] = (uint8_t)(weights ? (l4 | (h4 << 4)) : (h4 | (l4 << 4)));
                }
                dst[6 * 128 + 8 * x + 4 * b + ks] = (uint8_t)(weights ? eb - 11u : eb);
            }
}
void unpack_h4_row(const uint8_t* src, int C, float* v) {
    for (int x = 0; x < C / 128; ++x)
        for (int ks = 0; ks < 4; ++ks)
            for (int b = 0; b < 2; ++b) {
                const uint8_t* piece = src + (size_t)(3 * x + 2) * 128 + (2 * ks + b) * 16;
                const float sc = std::ldexp(1.0f, (int)src[6 * 128 + 8 * x + 4 * b + ks] - 127);
                for (int k = 0; k < 16; ++k) {
                    const int c = 128 * x + 32 * ks + 8 * (k >> 2) + 4 * b + (k & 3);
                    const int q = c >> 6;
                    uint16_t hb; std::memcpy(&hb, src + (size_t)(3 * (q >> 1) + (q & 1)) * 128 + 2 * (c & 63), 2);
                    v[c] = h2f(hb) + e2m1_to_f((uint32_t)piece[k] >> 4) * sc * (1.0f / 2048.0f);
                }
            }
}

}  // namespace

// One batch of encoded frames in flight (upload_impl.inc: bod_upload_frames_{jpeg,png}[_async], bod_{jpeg,png}_decode_rgb; DESIGN.md 9.11,
// 9.15).  `pinned` holds the [n] frame records of the format (JpegFrame / PngFrame) and, 128-byte aligned behind them at `payload_base`,
// what the host threads decode: a JPEG batch's coefficients, a PNG batch's filtered scanlines.  One copy takes both to `dev`.
// `copied`: that copy has left `pinned` -- the next batch's host decode into it waits for the event.
enum DecodeKind { DECODE_JPEG = 0, DECODE_PNG = 1, DECODE_KINDS = 2 };
struct DecodeSlot {
    char* pinned = nullptr; size_t pinned_cap = 0;
    char* dev = nullptr; size_t dev_cap = 0;
    uint8_t* scratch = nullptr; size_t scratch_cap = 0;   // JPEG: the components' MCU-padded uint8 planes (device); PNG: none
    hipEvent_t copied = nullptr;
    // of the batch decoded last
    int32_t n = 0;
    size_t stage_bytes = 0, payload_base = 0, scratch_bytes = 0;
    int64_t rgb_bytes = 0;
    int32_t idct_wgs_per_frame = 0, color_wgs_per_frame = 0;     // JPEG: the two kernels' workgroups per frame
    int32_t rows_per_band = 0;                                   // PNG: rows a workgroup takes at a time
    void release() {
        if (pinned) hipHostFree(pinned);
        if (dev) hipFree(dev);
        if (scratch) hipFree(scratch);
        if (copied) hipEventDestroy(copied);
        *this = DecodeSlot();
    }
};

// One buffer of detection records and everything that belongs to it.  The device arrays are [B,K,.] (nms_nsel [B]); the pinned copy
// is laid out by RecordLayout (record_state.h).
struct RecordSlot {
    int32_t* nms_sel = nullptr; int32_t* nms_nsel = nullptr;           // cluster centres and their count per image
    float* scores = nullptr; float* means = nullptr; float* covs = nullptr; float* counts = nullptr;
    float* parts = nullptr; float* cparts = nullptr;                   // [B,K,3,16] / [B,K,4] on handles with covariance / class-entropy parts
    // merge terms, from the first non-default bod_set_merge_method on: within / between [B,K,16], members [B,K]; merge_terms_ok: the
    // slot's last cluster stage wrote them (it ran as CENTRE or MIXTURE)
    float* merge_within = nullptr; float* merge_between = nullptr; int32_t* merge_members = nullptr;
    bool merge_terms_ok = false;
    std::vector<char> parts_ok, cparts_ok;                             // per image: the handle's parts_ok / cparts_ok at the slot's cluster-fuse
    // a ticket of bod_infer_async
    char* host_stage = nullptr;                // pinned host copy of the records (filled on the stream that finished them)
    hipEvent_t done = nullptr;
    hipStream_t done_stream = nullptr;         // the stream that recorded `done`: a ticket's gather follows on it
    bool pending = false;                      // not collected yet
    bool parts_staged = false, cparts_staged = false;                  // host_stage holds the parts of a ticket
};

struct bod_context {
    bod_config cfg{};
    std::string err;
    hipStream_t stream = nullptr;
    std::vector<void*> allocs;
    std::map<const void*, size_t> alloc_bytes;
    int64_t device_bytes = 0;
    struct TrainState* train = nullptr;                 // training mode (train_impl.inc)
    struct ValState* val = nullptr;                     // validation from boxes (validate_impl.inc): allocated by its first call
    // reg_kind 5 (bod_set_loss_options): samples per row; seed / first image id of the validation entries (the
    // training step takes its own from the step's arguments).  The two buffers are allocated by the first kind-5 call.
    int32_t energy_samples = BOD_ENERGY_DEFAULT_SAMPLES;
    uint64_t loss_seed = 0; uint32_t loss_first_image_id = 0; int32_t loss_id_stride = 1;
    int32_t* energy_list = nullptr; float* energy_term = nullptr;    // [batch * A + 1] positive indices, [batch * A] row terms

    // geometry
    int sh = 0, sw = 0, ph = 0, pw = 0;                 // stem / pool output
    int ch[6] = {0}, cw[6] = {0};                       // stage 2..5 sizes (index = stage)
    int nlev = 0; int lh[8] = {0}, lw[8] = {0};         // pyramid levels p3..p7
    int64_t lvl_off[8] = {0};                           // padded pixel offset of each level
    int64_t lvl_p0[8] = {0};                            // dense pixel offset of each level
    int64_t Ppad = 0; int P = 0, A = 0;

    // weights
    std::map<std::string, HostTensor> host_w;           // "name/kind"
    std::map<std::string, PackedConv> packed;
    float* stem_w = nullptr; float* stem_b = nullptr;
    bool weights_ready = false, anchors_ready = false;
    StageState stage;                                   // which of forward / posterior / nms / cluster has run (record_state.h)

    // activations
    float* d_images = nullptr;
    float* splitk_partial = nullptr; size_t splitk_elems = 0;        // fp32 partial sums of the split-K layers
    uint8_t* d_frames_u8 = nullptr; size_t frames_u8_cap = 0;     // staging for bod_upload_frames_u8 (plain hipMalloc, grows)
    // pipelined input path (bod_upload_frames_u8_async): two image buffers (0 = d_images), their uint8 staging, a copy stream;
    // ev_img_ready: preprocess of a buffer finished (the forward waits on it); ev_img_free: the stem that read it finished
    // (the next upload into the same buffer waits on it)
    float* d_images_b[2] = {nullptr, nullptr}; uint8_t* d_u8_b[2] = {nullptr, nullptr}; size_t u8_cap_b[2] = {0, 0};
    hipStream_t copy = nullptr;
    hipEvent_t ev_img_ready[2] = {nullptr, nullptr}, ev_img_free[2] = {nullptr, nullptr};
    bool img_ready_pending[2] = {false, false}, img_free_pending[2] = {false, false};
    int cur_img_buf = -1;
    // ragged uploads (bod_upload_frames_u8_ragged[_async]): one table per route -- [batch] PreprocFrame records, then [batch][2] KITTI
    // factors -- filled on the host and copied on the upload's stream ahead of its kernel (plain hipMalloc on first use; the batch
    // fixes its size).  kscale_src[k]: where the factors of the frames in image buffer k lie (nullptr: uniform frames, the handle's
    // scalars apply).  The forward that consumes buffer k copies them into kscale_cur[i] on the stream of its stem, in front of
    // ev_img_free[k]: the copy stream may rewrite the table from then on, and the posterior reads the snapshot only.  Two
    // snapshots, alternated: at most two batches are in flight (bod_infer_async).
    struct RaggedTable { std::vector<char> host; char* dev = nullptr; };
    RaggedTable rag_sync, rag_b[2];
    RaggedTable aug_sync, aug_b[2];       // the augmented uploads' own (their records are PreprocAugFrame, without factors)
    DecodeSlot decode_slot[DECODE_KINDS][3];            // JPEG / PNG uploads: one per image buffer, [2] the synchronous route's
    // frame corruptions: the one-shot description bod_set_upload_corruption left for the next packed upload, and
    // each route's tables and scratch (indexed as decode_slot[kind])
    CorruptSpec corrupt_pending;
    CorruptSlot corrupt_slot[3];
    hipEvent_t ev_tab[2] = {nullptr, nullptr};          // the copy of rag_b[k].host has left the host (its next rewrite waits for it)
    const float* kscale_src[2] = {nullptr, nullptr};
    float* kscale_cur[2] = {nullptr, nullptr}; int kscale_i = 0;
    const float* kscale_now = nullptr;                  // snapshot of the batch the current call works on (nullptr: none)
    char* stem_out = nullptr;
    int es = 2;                                          // bytes per activation / weight CHANNEL (2 = bf16; 4 = fp32, or a (hi, lo) bf16 pair)
    bool split = false;                                  // bf16x3 precision: (hi, lo) bf16 pairs, three MFMA products (conv_igemm.hip)
    char* pyr_hx = nullptr;                              // f16mx: the pyramid as hx rows [B][Ppad][1 KiB] (pairs_to_hx_kernel in front of the first tower layer)
    int pyr_fmt = 1;                                     // format of `pyr_hx` (1 hx, 2 h4)
    int plan_mx = 0;                                     // ... and the plan really runs them that way (BOD_TOWER_MX=0 / BOD_CONV_XREUSE=0: bf16x3 towers)
    int mx = 0;                                          // 1 = f16mx, 2 = f16mx4 (the cross terms as ONE e2m1 product of twice the channels; h4 rows).  f16mx precision: bf16x3 everywhere but the head towers, which run one f16 + half a block-scaled e2m3 product per multiplication (conv_igemm.hip header)
    Plane pyramid;                                       // all levels, [B][Ppad][256]
    char* head_act[3][2] = {{nullptr}};              // [B][N][Ppad][256]
    char* head_act_t[3][4] = {{nullptr}};            // training: one buffer per tower layer
    float* raw[3] = {nullptr};                           // cls [B,N,P,9C] box [B,N,P,36] cov [B,N,P,90]
    // MC aggregation fused into the last tower layers (ConvGroup.agg_kind): per-anchor statistics instead of raw[]
    float* agg[3] = {nullptr};                           // sum softmax [B,A,C], Welford box [B,A,16], sum cov params [B,A,10]
    bool agg_plan = false;                               // the plan holds FLAVOUR_AGG ops
    bool plan_fused_out = false, plan_xreuse = false, plan_xreuse0 = false;     // bod_plan_info
    bool raw_valid = false, agg_valid = false;           // which of the two the last forward produced
    // Sparse tail (build_plan): the box and covariance heads' aggregating launches run after the keep flags, over the pixels with a
    // kept anchor only; their statistics [agg[1], agg[2]] then exist for the anchors kept at (keep_seed, keep_first) alone.
    bool plan_sparse = false;
    bool plan_halo = false;                              // ... and box layer 1 / covariance layer 2 over the tail's 3x3 halo
    SparseTailArgs sparse{};
    int plan_tail_rows = 0;                              // rows per tile of the sparse tail launch (bod_plan_info_n slot 9; 0: no sparse tail)
    int plan_stage_end = 0;                              // last block of stages 2-4 on the pixels the next stage reads (slot 10): 0 off, 1 the `2c`, 2 + stage 4's `2b`
    bool agg_sparse = false;                             // the last forward's agg[1] / agg[2] are sparse
    // Statistics handles (bod_config.mc_statistics): the accumulator of the bod_stat_* entry points -- a second set of the three
    // agg[] arrays holding the merged statistics of stat_k samples.  agg[] itself receives every bod_stat_forward's fresh record (from
    // the aggregating flavour, or from raw[] through stat_from_raw_kernel on plans without one) and is the merge's source.
    float* stat_acc[3] = {nullptr};
    int stat_k = 0;
    hipEvent_t ev_stat = nullptr;                        // bod_stat_merge_from: orders the two handles' streams
    // Mirrored views (bod_stat_forward_view / bod_stat_merge_view): the frames mirrored left-right, allocated by the first mirrored
    // forward, and the outcome of the host check that the uploaded anchors are mirror-symmetric (-1: not checked since
    // bod_set_anchors, 1: symmetric, 0: level mirror_bad_level is not)
    float* d_mirror = nullptr;
    int mirror_sym = -1, mirror_bad_level = 0;
    bool keep_ready = false;                             // pb.keep / d_counts / block_counts / num_kept hold the keep stage's output
    uint64_t keep_seed = 0; uint32_t keep_first = 0;
    uint64_t last_seed = 0; uint32_t last_first_image = 0;
    int32_t last_sample_base = 0;                        // mc_sample_base of the last forward (bod_stat_forward passes its own): materialise_raw re-runs with it
    std::map<std::string, RowEnt*> tables;
    struct XrTable { RowEnt* rows = nullptr; int2* ext = nullptr; int m = 0; };
    std::map<std::string, XrTable> xr_tables;          // row-reuse tilings of plane -> plane 3x3 layers (add_conv)
    std::vector<Op> ops;
    const float* cur_images = nullptr;

    // post
    float* d_anchors = nullptr;
    PostBuffers pb{};
    float* nms_scores = nullptr; int32_t* nms_begin = nullptr;
    // detection records are double-buffered ("slots") so the latency-bound NMS + cluster-fuse of one
    // batch can run on a side stream underneath the next batch's convolutions
    RecordSlot rec[2];
    int slot = 0;
    RecordSlot& cur() { return rec[slot]; }             // the slot run_nms / run_cluster write and the synchronous getters read
    // Covariance parts (bod_config.covariance_parts; nullptr / empty on every other handle): the per-anchor lower triangles behind
    // pb.covs, the detections' [B,K,3,16] double-buffered with the records.  parts_ok[img]: the image's rows of `parts` belong to its
    // posterior (false between bod_set_posterior and bod_set_posterior_parts); rec[slot].parts_ok[img]: ... at the slot's cluster-fuse.
    float* parts = nullptr;
    std::vector<char> parts_ok;
    // Class-entropy parts (bod_config.covariance_parts bit BOD_PARTS_CLASS; nullptr / empty on every other handle).  ent: the fresh
    // sum_n H(softmax) [B,A] of the last forward (AGG_CLS_ENT epilogue, or stat_from_raw_kernel); stat_ent: its accumulator on a
    // statistics handle, holding stat_ent_k of the record's stat_k samples; cparts: [B,A,3+C] per kept slot; the detections'
    // [B,K,4] double-buffered with the records; the *_ok flags as for the covariance parts.
    bool class_parts = false;
    float* ent = nullptr; float* stat_ent = nullptr; int stat_ent_k = 0;
    // bod_stat_acquisition, allocated by its first call: the [B,A] MI scratch, the workgroups' partial rows, the
    // outputs ([B,12] then [B,C-1,3] doubles)
    float* acq_mi = nullptr; double* acq_partials = nullptr; double* acq_out = nullptr;
    bool acq_ran = false;
    float* cparts = nullptr;
    std::vector<char> cparts_ok;
    // How run_cluster merges a cluster (bod_set_merge_method).  The slots' term buffers exist from the first
    // non-default setter call on.
    int merge_method = BOD_MERGE_BAYES;
    // Black-box MC dropout (bod_set_uncertainty_method).  bb holds the stage's buffers from the first switch to the
    // method on (bb.keep != nullptr); its outputs point at the record slot a call writes.  bb_samples_ok: the sample detections
    // belong to the last forward (bod_blackbox_samples ran, or bod_set_sample_detections since).
    int uncertainty_method = BOD_METHOD_BAYES_OD;
    bod_blackbox_options bb_opt{0.f, 1, 0.f, 0};
    BlackBoxArgs bb{};
    bool bb_samples_ok = false;
    hipStream_t side = nullptr;
    // ---- CU-partitioned pipeline overlap (bod_config.pipeline_overlap; bod_infer_async only).  The memory-bound front of batch i+1
    // (stem, backbone, FPN) runs on its own stream, masked to the last `ov_front_slots` CU slots of every XCD, while the MFMA-bound
    // back of batch i (fan-out layer, towers, posterior) runs on the other slots: `back` = the main stream of such a call (h->stream
    // points at it for the call's duration), `full` = the unmasked main stream every other entry point uses.  The only tensor that
    // crosses the partition is the pyramid, double-buffered (pyr_d); ev_front_done[p]: front of the batch with parity p finished,
    // ev_l0_done[p]: the fan-out layer that read pyramid p finished (the front two batches later waits for it).
    int overlap_mode = 0;                               // 0 off, 1 CU-masked streams, 2 plain streams (A/B)
    int ov_front_slots = 0, ov_slots = 0;
    hipStream_t full = nullptr, front = nullptr, back = nullptr;
    hipEvent_t ev_front_done[2] = {nullptr, nullptr}, ev_l0_done[2] = {nullptr, nullptr}, ev_join = nullptr;
    bool l0_pending[2] = {false, false};
    bool ov_dirty = false;                              // front / back hold work no `full`-stream call has been ordered behind yet
    char* pyr_d[2] = {nullptr, nullptr};                // pyr_d[0] == pyramid.d; [1] only on overlap handles
    int fwd_parity = 0, pyr_last = 0;
    int first_head_op = 0;                              // index of the first head launch in ops: everything before it is the front
    bool in_overlap_call = false;
    int n_cu = 256;                                     // compute units of the device (hipDeviceProp_t::multiProcessorCount)
    hipEvent_t ev_posterior = nullptr;
    int dev_op_lo = 0, dev_op_hi = 1 << 30;                   // BOD_FORWARD_OPS=lo:hi (development: tests/tools/selfcheck_probe.py): forward runs ops [lo, hi) only
    float* rec_send = nullptr; float* rec_recv = nullptr; size_t rec_recv_elems = 0;      // bod_gather_detections: packed records, gathered blocks
    hipEvent_t ev_gather = nullptr; hipStream_t gather_stream = nullptr;                  // last use of rec_send / rec_recv and the stream it went to
    float* iou_scratch = nullptr; int64_t iou_cap = 0;
    float* affinity = nullptr;                           // bod_set_affinity: centre columns of a caller-supplied affinity matrix (one-shot; stage.affinity_img)

    // profiling
    bool profiling = false; int prof_which = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_head, ev_post;
    double prof_flops = 0;

    bod_status fail(bod_status s, const char* fmt, ...) {
        char buf[1024];
        va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
        err = buf;
        return s;
    }
    template <typename T> bod_status dalloc(T** p, size_t n_elems, bool zero = true) {
        void* q = nullptr;
        const size_t bytes = std::max<size_t>(n_elems * sizeof(T), 256);
        hipError_t e = hipMalloc(&q, bytes);
        if (e != hipSuccess) return fail(BOD_ERR_OOM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        if (zero) {
            e = hipMemsetAsync(q, 0, bytes, stream);
            if (e != hipSuccess) return fail(BOD_ERR_HIP, "hipMemset: %s", hipGetErrorString(e));
        }
        allocs.push_back(q);
        alloc_bytes[q] = bytes;
        device_bytes += (int64_t)bytes;
        *p = reinterpret_cast<T*>(q);
        return BOD_OK;
    }
};

#define HIPCHK(h, expr)                                                                         \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess)                                                                   \
            return (h)->fail(BOD_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                             __FILE__, __LINE__);                                               \
    } while (0)
#define BODCHK(expr) do { bod_status _s = (expr); if (_s != BOD_OK) return _s; } while (0)

namespace {

// The throw-away context of the stateless entry points (bod_stage_*, bod_loss_*, bod_anchor_targets): it owns the call's stream and
// temporary device buffers; done() leaves the message where bod_last_error(NULL) finds it.
struct StageScope {
    bod_context ctx;
    bod_context* h = &ctx;
    bod_status done(bod_status s) {
        if (s != BOD_OK) g_create_error = h->err;
        if (h->stream) hipStreamSynchronize(h->stream);
        for (void* p : h->allocs) hipFree(p);
        if (h->stream) hipStreamDestroy(h->stream);
        h->allocs.clear(); h->stream = nullptr;
        return s;
    }
    bod_status open(int32_t device) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
            return h->fail(BOD_ERR_NO_DEVICE, "no HIP device %d: libbayesod_hip has no CPU fallback", device);
        if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess)
            return h->fail(BOD_ERR_HIP, "cannot set up device %d", device);
        return BOD_OK;
    }
};

// Forward row table of a convolution that reads a zero-bordered plane (pitch, bstride) -- one row per output pixel in (b, y, x)
// order, in_off = the pixel's window origin (conv_out_geometry: oy, ox).  The other fields are zero: a caller that needs them
// fills them in a second pass.
std::vector<RowEnt> forward_row_table(int B, int OH, int OW, int stride, int oy, int ox, int pitch, int64_t bstride) {
    std::vector<RowEnt> rows((size_t)B * OH * OW);
    size_t r = 0;
    for (int b = 0; b < B; ++b)
        for (int y = 0; y < OH; ++y)
            for (int xx = 0; xx < OW; ++xx) {
                RowEnt e{};
                e.in_off = (int32_t)(b * bstride + (int64_t)(y * stride + oy) * pitch + (xx * stride + ox));
                e.in_pitch = pitch;
                rows[r++] = e;
            }
    return rows;
}

// every batch still in a record slot finishes in front of what `st` gets next (the posterior's buffers are its readers' inputs)
bod_status wait_pending_slots(bod_context* h, hipStream_t st) {
    for (RecordSlot& r : h->rec)
        if (r.pending) HIPCHK(h, hipStreamWaitEvent(st, r.done, 0));
    return BOD_OK;
}

RecordLayout record_layout(const bod_context* h) {
    return RecordLayout((size_t)h->cfg.batch, (size_t)h->cfg.nms_max_output_size, h->cfg.num_classes,
                        (h->cfg.covariance_parts & BOD_PARTS_COVARIANCE) != 0, h->class_parts);
}

// A slot's pinned staging buffer, segment by segment, for every segment `ptr` names: filled from the device arrays there on `st`
// (from_device), or copied out to the caller's arrays there.
bod_status copy_staged(bod_context* h, const RecordSlot& r, void* const ptr[RecordLayout::SEGS], bool from_device, hipStream_t st) {
    const RecordLayout L = record_layout(h);
    for (int s = 0; s < RecordLayout::SEGS; ++s) {
        const size_t n = L.bytes((RecordLayout::Seg)s);
        if (!ptr[s] || n == 0) continue;
        if (from_device) HIPCHK(h, hipMemcpyAsync(r.host_stage + L.off[s], ptr[s], n, hipMemcpyDeviceToHost, st));
        else std::memcpy(ptr[s], r.host_stage + L.off[s], n);
    }
    return BOD_OK;
}

// the current slot's detection count of one image, on the host
bod_status slot_count(bod_context* h, int32_t img, int32_t* num) {
    HIPCHK(h, hipMemcpyAsync(num, h->cur().nms_nsel + img, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BOD_OK;
}

const char* kHeadPrefix[3] = {"pyramid_classification", "pyramid_regression", "pyramid_cov"};
const int kHeadConvs[3] = {4, 3, 4};     // RegHeader.call uses 3 towers convs (multitask_headers.py:209-230)

// CU mask of hipExtStreamCreateWithCUMask for CU slots [lo, hi) of every XCD.  On MI355X (8 XCDs x 32 CUs) mask bit i selects slot
// i / 8 of XCD i % 8 (tests/tools/cu_mask_probe.hip; an XCD without any bit set keeps all its CUs), so a slot range is symmetric
// over the XCDs and workgroup b still lands on XCD b % 8 -- what the tower kernel's XCD-aware tile order assumes.
void cu_slot_mask(int lo, int hi, uint32_t mask[8]) {
    for (int w = 0; w < 8; ++w) mask[w] = 0u;
    for (int slot = lo; slot < hi; ++slot)
        for (int xcd = 0; xcd < 8; ++xcd) { const int bit = slot * 8 + xcd; mask[bit >> 5] |= 1u << (bit & 31); }
}

bod_status new_plane(bod_context* h, Plane* p, int B, int hh, int ww, int C) {
    p->h = hh; p->w = ww; p->C = C; p->pitch = ww + 2; p->base = 0;
    p->bstride = (int64_t)(hh + 2) * (ww + 2);
    return h->dalloc(&p->d, (size_t)B * p->bstride * C * h->es);
}

// row table for plane -> plane convolutions (plane_tables.h). org_* = padded coordinate of the window origin of
// output (0,0); res optional (nearest-upsampled when its size differs); out_step 2: the output pixels
// (2y, 2x) only -- no allocation of its own: the table lives in the second halves of the dense table's entries (dense_key; built here
// if no conv has asked for it yet) and is taken half an entry further on (plane_tables.h, plane_step_view).  *M = rows of the table.
PlaneGeom plane_geom(const Plane& p) { return PlaneGeom{p.base, p.bstride, p.pitch, p.h, p.w}; }

bod_status make_table(bod_context* h, const std::string& key, const std::string& dense_key, int B, const Plane& in, const Plane& out,
                      int stride, int org_y, int org_x, const Plane* res, int out_step, const RowEnt** tbl, int* M) {
    *M = B * plane_step_count(out.h, out_step) * plane_step_count(out.w, out_step);
    auto it = h->tables.find(key);
    if (it != h->tables.end()) { *tbl = it->second; return BOD_OK; }
    std::vector<RowEnt> rows;
    const PlaneGeom gi = plane_geom(in), go = plane_geom(out), gr = res ? plane_geom(*res) : PlaneGeom{};
    plane_row_table(B, gi, go, stride, org_y, org_x, res ? &gr : nullptr, out_step, rows);
    if (out_step != 1) {
        const RowEnt* dense = nullptr;
        int Md = 0;
        BODCHK(make_table(h, dense_key, dense_key, B, in, out, stride, org_y, org_x, res, 1, &dense, &Md));
        RowEnt* view = const_cast<RowEnt*>(dense);          // (a 1 x 1 plane: the step-2 table is the dense table)
        if (rows.size() < (size_t)Md) {
            view = const_cast<RowEnt*>(plane_step_view(dense));
            HIPCHK(h, hipMemcpy2D(view, sizeof(RowEnt), rows.data(), sizeof(RowEnt), PLANE_STEP_VIEW_BYTES, rows.size(), hipMemcpyHostToDevice));
        }
        h->tables[key] = view;
        *tbl = view;
        return BOD_OK;
    }
    RowEnt* d = nullptr;
    BODCHK(h->dalloc(&d, rows.size(), false));
    HIPCHK(h, hipMemcpyAsync(d, rows.data(), rows.size() * sizeof(RowEnt), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->tables[key] = d;
    *tbl = d;
    return BOD_OK;
}

const HostTensor* find_w(bod_context* h, const std::string& name, int kind) {
    auto it = h->host_w.find(name + "/" + std::to_string(kind));
    return it == h->host_w.end() ? nullptr : &it->second;
}

// Fold BN (double), pack OHWI bf16 padded to cout_pad, upload.
bod_status pack_conv(bod_context* h, const std::string& name, const std::string& bn, int cout_pad_to,
                     PackedConv* out, int hx = 0) {          // hx: 0 = the data path's own form, 1 = hx rows (f16mx), 2 = h4 rows (f16mx4)
    const std::string ckey = hx == 2 ? name + ":h4" : hx ? name + ":hx" : name;             // (f16mx: tower layers 1.. are packed as hx rows, everything else as pairs)
    auto it = h->packed.find(ckey);
    if (it != h->packed.end()) { *out = it->second; return BOD_OK; }
    const HostTensor* k = find_w(h, name, 0);
    if (!k || k->shape.size() != 4) return h->fail(BOD_ERR_NOT_READY, "missing conv kernel '%s'", name.c_str());
    const int kh = (int)k->shape[0], kw = (int)k->shape[1], cin = (int)k->shape[2], cout = (int)k->shape[3];
    const HostTensor* b = find_w(h, name, 1);
    std::vector<double> scale(cout, 1.0), shift(cout, 0.0);
    for (int o = 0; o < cout; ++o) shift[o] = b ? (double)b->data[o] : 0.0;
    if (!bn.empty()) {
        const HostTensor *g = find_w(h, bn, 2), *be = find_w(h, bn, 3), *mu = find_w(h, bn, 4), *var = find_w(h, bn, 5);
        if (!g || !be || !mu || !var) return h->fail(BOD_ERR_NOT_READY, "missing batch-norm '%s'", bn.c_str());
        for (int o = 0; o < cout; ++o) {
            const double s = (double)g->data[o] / std::sqrt((double)var->data[o] + (double)BN_EPS);
            scale[o] = s;
            shift[o] = (shift[o] - (double)mu->data[o]) * s + (double)be->data[o];
        }
    }
    PackedConv pc;
    pc.cout = cout; pc.taps = kh * kw; pc.kw = kw; pc.cin = cin;
    pc.cout_pad = ((cout + cout_pad_to - 1) / cout_pad_to) * cout_pad_to;
    const size_t nw = (size_t)pc.cout_pad * pc.taps * cin;
    const bool as_f32 = h->es == 4 && !h->split;
    std::vector<uint16_t> w(as_f32 ? 0 : nw * (h->split ? 2 : 1), 0);
    std::vector<float> w32(as_f32 ? nw : 0, 0.f);
    std::vector<float> bias(pc.cout_pad, 0.f);
    for (int o = 0; o < cout; ++o) {
        bias[o] = (float)shift[o];
        for (int t = 0; t < pc.taps; ++t)
            for (int c = 0; c < cin; ++c) {
                const double v = (double)k->data[((size_t)t * cin + c) * cout + o] * scale[o];
                const size_t idx = ((size_t)o * pc.taps + t) * cin + c;
                if (h->split) {            // (hi, lo) pair of the fp32 weight: 32 hi then 32 lo per 64-slot group
                    const float f = (float)v;
                    const uint16_t hi = f2bf(f);
                    const size_t slot = ((size_t)o * pc.taps + t) * 2 * cin + (size_t)(c >> 5) * 64 + (c & 31);
                    w[slot] = hi; w[slot + 32] = f2bf(f - bf2f(hi));
                } else if (h->es == 2) w[idx] = f2bf((float)v);
                else w32[idx] = (float)v;
            }
    }
    if (hx) {                                  // one hx row per (cout, tap): same bytes as the pair form
        if (!h->split || cin % 64 != 0) return h->fail(BOD_ERR_INVALID_ARG, "hx weights need the (hi, lo) data path and cin %% 64 == 0");
        std::vector<float> row(cin);
        uint8_t* wb = reinterpret_cast<uint8_t*>(w.data());
        for (int o = 0; o < cout; ++o)
            for (int t = 0; t < pc.taps; ++t) {
                for (int c = 0; c < cin; ++c) row[c] = (float)((double)k->data[((size_t)t * cin + c) * cout + o] * scale[o]);
                if (hx == 2) {
                    if (cin != 256) return h->fail(BOD_ERR_INVALID_ARG, "h4 weights: 256 input channels");
                    pack_h4_row(row.data(), cin, wb + ((size_t)o * pc.taps + t) * cin * 4, true);
                } else pack_hx_row(row.data(), cin, wb + ((size_t)o * pc.taps + t) * cin * 4, true);
            }
    }
    size_t w_extra = 0;
    if (hx == 2) {          // ... + a compact copy of the scale bytes behind the rows: [tap][x][cout][half][ks], what the kernel's scale pieces read
        if (pc.cout_pad != 256) return h->fail(BOD_ERR_INVALID_ARG, "h4 weights: one 256-cout tile");
        w_extra = (size_t)pc.taps * 2 * 2048;
        w.resize(w.size() + w_extra / 2, 0);
        uint8_t* wb = reinterpret_cast<uint8_t*>(w.data());
        uint8_t* sc = wb + nw * h->es;
        for (int t = 0; t < pc.taps; ++t)
            for (int x = 0; x < 2; ++x)
                for (int o = 0; o < 256; ++o)
                    std::memcpy(sc + ((size_t)(t * 2 + x) * 256 + o) * 8, wb + ((size_t)o * pc.taps + t) * cin * 4 + 768 + 8 * x, 8);
    }
    BODCHK(h->dalloc(&pc.w, nw * h->es + w_extra, false));
    BODCHK(h->dalloc(&pc.bias, bias.size(), false));
    HIPCHK(h, hipMemcpyAsync(pc.w, as_f32 ? (const void*)w32.data() : (const void*)w.data(), nw * h->es + w_extra,
                             hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(pc.bias, bias.data(), bias.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->packed[ckey] = pc;
    *out = pc;
    return BOD_OK;
}

ConvArgs base_args(const PackedConv& pc, const RowEnt* rows, int M, int in_cstride, int out_cstride) {
    ConvArgs a{};
    a.rows = rows; a.M = M; a.taps = pc.taps; a.KW = pc.kw; a.cin = pc.cin;
    a.in_cstride = in_cstride; a.cout_pad = pc.cout_pad; a.cout_valid = pc.cout;
    a.out_cstride = out_cstride; a.res_cstride = out_cstride; a.groups = 1;
    a.fan_count = 1; a.fan_stride = 0;
    return a;
}

// bf16x3 precision: the kernel counts (hi, lo) SLOTS wherever the bf16 mode counts channels of a pixel (kernels.h, ConvArgs::split)
void to_split_args(ConvArgs* a) {
    a->split = 1;
    a->cin *= 2; a->in_cstride *= 2; a->res_cstride *= 2;
    if (!(a->flags & CONV_OUT_F32)) a->out_cstride *= 2;
    for (int g = 0; g < 3; ++g) a->g[g].in_coff *= 2;
}

// conv + folded BN (+residual) (+ReLU) between two planes
bod_status add_conv(bod_context* h, const std::string& name, const std::string& bn, const Plane& in,
                    const Plane& out, int stride, bool same, bool relu, const Plane* res,
                    char* out_relu = nullptr, int out_step = 1, bool even_rows = false) {
    PackedConv pc;
    BODCHK(pack_conv(h, name, bn, 64, &pc));
    if (pc.cin != in.C || pc.cout != out.C)
        return h->fail(BOD_ERR_INVALID_ARG, "conv '%s': weight shape [%d->%d] does not match planes [%d->%d]",
                       name.c_str(), pc.cin, pc.cout, in.C, out.C);
    const int kh = pc.taps / pc.kw;
    int OH, OW, oy, ox;                        // (the output plane is the caller's: only the window origin is taken from here)
    conv_out_geometry(in.h, in.w, kh, pc.kw, stride, same, &OH, &OW, &oy, &ox);
    // the table depends on plane geometry only (offsets are relative to each buffer's base)
    char key[256], dense_key[256];
    for (int k = 0; k < 2; ++k)
        snprintf(k ? dense_key : key, sizeof key, "pp:%lld,%lld,%d:%lld,%lld,%d,%d,%d:%d:%d:%d:%lld,%lld,%d,%d,%d:%d", (long long)in.base,
                 (long long)in.bstride, in.pitch, (long long)out.base, (long long)out.bstride, out.pitch, out.h, out.w,
                 stride, oy, ox, res ? (long long)res->base : -1LL, res ? (long long)res->bstride : 0LL,
                 res ? res->pitch : 0, res ? res->h : 0, res ? res->w : 0, k ? 1 : out_step);
    const RowEnt* tbl = nullptr;
    const int B = h->cfg.batch;
    int M = 0;
    BODCHK(make_table(h, key, dense_key, B, in, out, stride, oy, ox, res, out_step, &tbl, &M));
    Op op; op.kind = Op::CONV;
    op.conv = base_args(pc, tbl, M, in.C, out.C);
    op.conv.g[0] = ConvGroup{in.d, pc.w, pc.bias, out.d, res ? res->d : nullptr, out_relu, 0, 0, nullptr, nullptr, nullptr, 0, 0};
    op.conv.flags = relu ? CONV_RELU : 0;
    op.flops = 2.0 * op.conv.M * pc.cout * pc.taps * pc.cin;
    op.name = name; op.wname[0] = name; op.bnname[0] = bn;
    op.same_geom = stride == 1 && same && pc.taps == 9 && pc.kw == 3 && in.base == out.base && in.bstride == out.bstride && in.pitch == out.pitch &&
                   in.h == out.h && in.w == out.w;
    if (stride == 1 && same && pc.taps == 9 && pc.kw == 3 && in.h == out.h && in.w == out.w) { op.conv.plane_h = out.h; op.conv.plane_w = out.w; }
    // Split-K for layers with too few output tiles to fill the chip and a long reduction (P6 always; most of
    // stage 3-5 at batch 1): enough splits for >= ~256 workgroups, each keeping >= 4 K-tiles.
    static const bool splitk_on = [] { const char* e = getenv("BOD_CONV_SPLITK"); return !e || atoi(e) != 0; }();
    if (splitk_on && (h->es == 2 || h->split)) {
        // (counted on the whole plane also where the table holds a part of it -- out_step, even_rows: a pixel's summation order must
        //  not depend on BOD_STAGE_END_PIXELS)
        const long tiles = (long)((B * out.h * out.w + 127) / 128) * (pc.cout_pad % 128 == 0 ? pc.cout_pad / 128 : pc.cout_pad / 64);
        const int chunks = pc.cin * (h->split ? 2 : 1) / 64;          // K-tiles per tap (bf16x3: 32 channels per K-tile)
        int S = 1;
        while (tiles * S < 256 && S * 2 <= 16 && chunks % (S * 2) == 0 && (long)pc.taps * (chunks / (S * 2)) >= 4) S *= 2;
        if (S > 1) {
            op.conv.ksplit = S;
            h->splitk_elems = std::max(h->splitk_elems, (size_t)S * op.conv.M * pc.cout_pad);
        }
    }
    // Activation row reuse for the plane -> plane 3x3 stride-1 SAME convolutions of 256 -> 256 channels (stage 4's `2b` layers, P3-P5
    // of the FPN): the tower kernel's loop -- every (chunk, ky) staged once, the three kx taps read the same rows -- on this layer's own
    // tiles of x-adjacent runs (plan_tables.h).  Round 4, tests/tools/op_table.py: these launches ran the generic loop at 1 100-1 130
    // TFLOP/s against the towers' 1 270.  BOD_PLANE_XREUSE=0: the generic launches (different fp32 summation order: not bit-identical).
    static const bool plane_xr_on = [] { const char* e = getenv("BOD_PLANE_XREUSE"); return !e || atoi(e) != 0; }();
    static const bool xr_on = [] { const char* e = getenv("BOD_CONV_XREUSE"); return !e || atoi(e) != 0; }();
    if (plane_xr_on && xr_on && (h->es == 2 || h->split) && !h->cfg.training && op.conv.ksplit <= 1 && stride == 1 && same && pc.taps == 9 && pc.kw == 3 &&
        pc.cin == 256 && pc.cout == 256 && pc.cout_pad == 256 && !res && !out_relu && in.h == out.h && in.w == out.w) {
        ConvArgs probe = op.conv;
        if (conv_igemm_uses_full_cout_tile(probe)) {
            // even_rows (the `2b` of stage 4's last block, build_plan): tiles of the even output rows only, all x -- runs stay
            // x-adjacent and tiles full; the odd rows are read by nobody (plane_tables.h).  Only where the launch keeps the 256x256
            // tile with half the rows (the kernel's launch rule, conv_igemm.hip, sees the table's M): otherwise every row as before.
            bool even = even_rows;
            if (even) { ConvArgs half = op.conv; half.M = B * plane_step_count(out.h, 2) * out.w; even = conv_igemm_uses_full_cout_tile(half); }
            const std::string xkey = std::string(key) + (even ? ":xr:even" : ":xr");
            auto it = h->xr_tables.find(xkey);
            if (it == h->xr_tables.end()) {
                std::vector<RowEnt> rows((size_t)op.conv.M), tiled;
                std::vector<ExtRow> ext;
                HIPCHK(h, hipMemcpy(rows.data(), tbl, rows.size() * sizeof(RowEnt), hipMemcpyDeviceToHost));
                if (even) { std::vector<RowEnt> dense; dense.swap(rows); plane_rows_of_even_y(dense, B, out.h, out.w, rows); }
                if (!xr_tile_rows(rows, tiled, ext)) return h->fail(BOD_ERR_INVALID_ARG, "row-reuse tiling of '%s': extended rows out of order", name.c_str());
                bod_context::XrTable t;
                t.m = (int)tiled.size();
                BODCHK(h->dalloc(&t.rows, tiled.size(), false));
                BODCHK(h->dalloc(&t.ext, ext.size(), false));
                HIPCHK(h, hipMemcpy(t.rows, tiled.data(), tiled.size() * sizeof(RowEnt), hipMemcpyHostToDevice));
                HIPCHK(h, hipMemcpy(t.ext, ext.data(), ext.size() * sizeof(int2), hipMemcpyHostToDevice));
                it = h->xr_tables.emplace(xkey, t).first;
            }
            op.conv.rows = it->second.rows; op.conv.ext = it->second.ext; op.conv.M = it->second.m; op.conv.xreuse = 2;
            if (even) op.flops = 2.0 * B * plane_step_count(out.h, 2) * out.w * pc.cout * pc.taps * pc.cin;
        }
    }
    h->ops.push_back(op);
    return BOD_OK;
}

bod_status build_geometry(bod_context* h) {
    const bod_config& c = h->cfg;
    const int H = c.image_h, W = c.image_w;
    if (H < 64 || W < 64) return h->fail(BOD_ERR_INVALID_ARG, "image size %dx%d too small", H, W);
    h->sh = (H - 7) / 2 + 1; h->sw = (W - 7) / 2 + 1;
    h->ph = (h->sh + 2 - 3) / 2 + 1; h->pw = (h->sw + 4 - 3) / 2 + 1;
    h->ch[2] = h->ph; h->cw[2] = h->pw;
    for (int s = 3; s <= 5; ++s) { h->ch[s] = (h->ch[s - 1] - 1) / 2 + 1; h->cw[s] = (h->cw[s - 1] - 1) / 2 + 1; }
    if (c.min_level != 3 || c.max_level != 7)
        return h->fail(BOD_ERR_INVALID_ARG, "only pyramid levels 3..7 are supported (got %d..%d)", c.min_level, c.max_level);
    h->nlev = 5;
    h->lh[0] = h->ch[3]; h->lw[0] = h->cw[3];
    h->lh[1] = h->ch[4]; h->lw[1] = h->cw[4];
    h->lh[2] = h->ch[5]; h->lw[2] = h->cw[5];
    h->lh[3] = (h->lh[2] + 1) / 2; h->lw[3] = (h->lw[2] + 1) / 2;
    h->lh[4] = (h->lh[3] + 1) / 2; h->lw[4] = (h->lw[3] + 1) / 2;
    int64_t pp = 0; int p = 0;
    for (int l = 0; l < 5; ++l) {
        const int stride = 1 << (l + 3);
        const int ah = (H + stride - 1) / stride, aw = (W + stride - 1) / stride;   // anchor grid (fpn_anchor_generator.py:28-29)
        if (ah != h->lh[l] || aw != h->lw[l])
            return h->fail(BOD_ERR_INVALID_ARG,
                           "pyramid level p%d is %dx%d but the anchor grid is %dx%d for a %dx%d image "
                           "(the reference's tf.concat of head outputs with anchors would mismatch too)",
                           l + 3, h->lh[l], h->lw[l], ah, aw, H, W);
        h->lvl_off[l] = pp; h->lvl_p0[l] = p;
        pp += (int64_t)(h->lh[l] + 2) * (h->lw[l] + 2);
        p += h->lh[l] * h->lw[l];
    }
    h->Ppad = pp; h->P = p; h->A = p * c.anchors_per_location;
    return BOD_OK;
}

Plane level_view(bod_context* h, int l) {
    Plane v = h->pyramid;
    v.base = h->lvl_off[l]; v.h = h->lh[l]; v.w = h->lw[l]; v.pitch = h->lw[l] + 2;
    return v;
}

// Raw head outputs [B,N,A,.] fp32.  Allocated with the plan, or on first use by a handle that never loads
// weights (a "post-only" handle whose raw buffers are filled by bod_set_raw / through bod_device_raw).
bod_status ensure_raw(bod_context* h) {
    const bod_config& c = h->cfg;
    const int out_ch[3] = {c.anchors_per_location * c.num_classes, c.anchors_per_location * 4, c.anchors_per_location * 10};
    for (int hd = 0; hd < 3; ++hd) {
        if ((hd == 2 && !c.has_covar_head) || h->raw[hd]) continue;
        BODCHK(h->dalloc(&h->raw[hd], (size_t)c.batch * c.mc_samples * h->P * out_ch[hd]));
    }
    // plans with the fused MC aggregation allocate the raw tensors on first use: point the raw-flavour ops at them
    for (Op& o : h->ops)
        if (o.kind == Op::CONV && o.flavour == FLAVOUR_RAW)
            for (int g = 0; g < o.conv.groups; ++g)
                if (o.conv.g[g].w2 && o.head[g] >= 0) o.conv.g[g].out2 = h->raw[o.head[g]];
    return BOD_OK;
}

bod_status train_init(bod_context* h);          // train_impl.inc
bod_status train_forward_only(bod_context* h, const float* dev, uint64_t seed, uint32_t first_image_id);
const uint32_t* train_dyn_rng(bod_context* h);
void train_destroy(bod_context* h);
void val_destroy(bod_context* h);               // validate_impl.inc

// The accumulator of a statistics handle (34 floats per anchor and image): with the plan, or on the first bod_stat_* call of a
// handle that never gets weights (a merge-and-posterior handle, like the raw buffers of such a handle: ensure_raw)
bod_status ensure_stat(bod_context* h) {
    if (h->stat_acc[0]) return BOD_OK;
    const bod_config& c = h->cfg;
    const size_t BA = (size_t)c.batch * h->A;
    BODCHK(h->dalloc(&h->stat_acc[0], BA * c.num_classes));
    BODCHK(h->dalloc(&h->stat_acc[1], BA * 16));
    if (c.has_covar_head) BODCHK(h->dalloc(&h->stat_acc[2], BA * 10));
    if (c.covariance_parts & BOD_PARTS_CLASS) BODCHK(h->dalloc(&h->stat_ent, BA));
    return BOD_OK;
}

bod_status build_plan(bod_context* h) {
    const bod_config& c = h->cfg;
    const int B = c.batch, N = c.mc_samples;
    const bool train_mode = c.training != 0;
    h->ops.clear();
    // ---------------- stem
    {
        const HostTensor* k = find_w(h, "conv1", 0);
        if (!k || k->shape.size() != 4 || k->shape[0] != 7 || k->shape[2] != 3 || k->shape[3] != 64)
            return h->fail(BOD_ERR_NOT_READY, "missing / malformed stem kernel 'conv1' [7,7,3,64]");
        const HostTensor* b = find_w(h, "conv1", 1);
        const HostTensor *g = find_w(h, "bn_conv1", 2), *be = find_w(h, "bn_conv1", 3), *mu = find_w(h, "bn_conv1", 4), *var = find_w(h, "bn_conv1", 5);
        if (!g || !be || !mu || !var) return h->fail(BOD_ERR_NOT_READY, "missing batch-norm 'bn_conv1'");
        std::vector<float> w(7 * 7 * 3 * 64), bias(64);
        for (int o = 0; o < 64; ++o) {
            const double s = (double)g->data[o] / std::sqrt((double)var->data[o] + (double)BN_EPS);
            bias[o] = (float)((((b ? (double)b->data[o] : 0.0) - (double)mu->data[o]) * s) + (double)be->data[o]);
            for (int t = 0; t < 147; ++t) w[(size_t)t * 64 + o] = (float)((double)k->data[(size_t)t * 64 + o] * s);
        }
        BODCHK(h->dalloc(&h->stem_w, w.size(), false));
        BODCHK(h->dalloc(&h->stem_b, bias.size(), false));
        HIPCHK(h, hipMemcpyAsync(h->stem_w, w.data(), w.size() * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->stem_b, bias.data(), bias.size() * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        BODCHK(h->dalloc(&h->stem_out, (size_t)B * h->sh * h->sw * 64 * h->es));
        Op s; s.kind = Op::STEM; s.name = "conv1(stem)"; s.flops = 2.0 * B * h->sh * h->sw * 64.0 * 147.0; h->ops.push_back(s);
        Op p; p.kind = Op::POOL; p.name = "pool1"; h->ops.push_back(p);
    }
    // ---------------- ResNet-50 stages (feature_extractor.py:104-139)
    Plane x;
    BODCHK(new_plane(h, &x, B, h->ph, h->pw, 64));
    Plane pool_out = x;
    h->ops[1].conv.g[0].out = pool_out.d;   // remember pool destination
    const char* blocks[6] = {"", "", "abc", "abcd", c.backbone_depth == 101 ? "abcdefghijklmnopqrstuvw" : "abcdef", "abc"};
    const int f1s[6] = {0, 0, 64, 128, 256, 512};
    Plane taps[6];
    // The last block of stages 2, 3 and 4 (res2c, res3d, res4f / res4w) has ONE reader: the next stage's ConvBlock, whose `2a` and
    // `branch1` are 1x1, stride 2, VALID -- pixel (2y, 2x) and nothing else (the FPN taps are the block-'a' outputs, below).  Its `2c`
    // therefore runs on a table of those pixels alone (plane_tables.h, out_step = 2): a quarter of the rows, written to the same
    // positions of the same plane, so the next stage's launches are untouched; the other pixels keep stale values nobody reads.
    // Stage 4's `2b` (row-reuse tiles) computes the even rows only.  Inference handles; BOD_STAGE_END_PIXELS=0: the whole planes
    // (A/B, bit-identical downstream), =1: the `2c` alone.  bod_plan_info_n slot 10.
    int stage_end = train_mode ? 0 : 2;
    if (const char* e = getenv("BOD_STAGE_END_PIXELS")) stage_end = std::min(stage_end, std::max(atoi(e), 0));
    h->plan_stage_end = stage_end;
    for (int st = 2; st <= 5; ++st) {
        const int f1 = f1s[st], f3 = f1 * 4, hh = h->ch[st], ww = h->cw[st];
        const int first_stride = st == 2 ? 1 : 2;
        Plane t1, t2, sc, oa, ob;
        BODCHK(new_plane(h, &t1, B, hh, ww, f1));
        BODCHK(new_plane(h, &t2, B, hh, ww, f1));
        BODCHK(new_plane(h, &sc, B, hh, ww, f3));
        BODCHK(new_plane(h, &oa, B, hh, ww, f3));
        BODCHK(new_plane(h, &ob, B, hh, ww, f3));
        bool use_a = true;
        // Bottleneck chain (stages 2 and 3, bf16 inference): a block's 3x3 conv `2b` keeps its tile in LDS and runs the block's 1x1
        // expansion `2c` (+ shortcut + ReLU) and the NEXT block's 1x1 reduction `2a` on it (conv_igemm.hip, ConvGroup.ch_*): the two
        // narrow intermediates never reach HBM -- 1.3 KB instead of 2 KB per pixel and block, two launches fewer.  The 3x3 comes FIRST
        // in the fused chain, so only the narrow t1 plane is re-read with a halo; t1 is double-buffered (the fused launch reads one
        // t1 plane with halos while it writes the next block's).  BOD_CHAIN_FUSION=0: the three separate launches (A/B; bit-identical).
        // Measured per block at 256 frames of 512x512 (BOD_TRACE_OPS): stage 2 (64 -> 256 channels) 2.23 -> 1.99 ms, its last block
        // 1.67 -> 1.45; stage 3 (128 -> 512) 1.33 -> 1.59 ms -- four shortcut passes per 128-pixel tile, each opening with an exposed
        // LDS-DMA round trip, cost more than the bytes they save -- so stage 3 is chained only on request (BOD_CHAIN_FUSION=3).
        // Later in round 3 the separate launches got their own streaming kernels (conv_pointwise.hip: the 1x1 expansion with the next
        // tile's rows in flight, the 64 -> 64 3x3 as a sliding window): per 256-frame step the chained stage 2 measures 23.1-23.6 ms of
        // backbone against 22.4-23.1 unchained on the same boxes, so the chain is OFF by default now (BOD_CHAIN_FUSION=2: stage 2,
        // =3: stages 2 and 3; the kernel, its guard entries and its bit-identity test stay).
        int chain_stages = 0;
        if (const char* e = getenv("BOD_CHAIN_FUSION")) chain_stages = atoi(e);
        bool chain_ok = h->es == 2 && !h->split && !train_mode && ((st == 2 && chain_stages >= 1) || (st == 3 && chain_stages >= 3));
        Plane t1alt;
        if (chain_ok) BODCHK(new_plane(h, &t1alt, B, hh, ww, f1));
        bool t1_ready = false;                  // the previous block's fused launch already produced this block's t1
        bool pw_t1_ready = false;               // (same, through the pointwise kernel's fused 2a)
        for (const char* bl = blocks[st]; *bl; ++bl) {
            char cb[64], bb[64];
            snprintf(cb, sizeof cb, "res%d%c_branch", st, *bl);
            snprintf(bb, sizeof bb, "bn%d%c_branch", st, *bl);
            const std::string c_(cb), b_(bb);
            if (chain_ok) {
                Plane& out = use_a ? oa : ob;
                const bool first = *bl == 'a';
                if (!t1_ready) BODCHK(add_conv(h, c_ + "2a", b_ + "2a", x, t1, first ? first_stride : 1, false, true, nullptr));
                if (first) BODCHK(add_conv(h, c_ + "1", b_ + "1", x, sc, first_stride, false, false, nullptr));
                BODCHK(add_conv(h, c_ + "2b", b_ + "2b", t1, t2, 1, true, true, nullptr));
                Op& op2b = h->ops.back();
                const Plane& shortcut = first ? sc : x;
                const bool can = op2b.conv.ksplit <= 1 && !conv_igemm_uses_big_tile(op2b.conv) && op2b.conv.cout_pad == f1 && (f1 == 64 || f1 == 128);
                if (!can) {                      // (split-K at batch 1, ...): the separate launches
                    BODCHK(add_conv(h, c_ + "2c", b_ + "2c", t2, out, 1, false, true, &shortcut));
                    t1_ready = false;
                } else {
                    PackedConv p2c;
                    BODCHK(pack_conv(h, c_ + "2c", b_ + "2c", 64, &p2c));
                    if (p2c.cin != f1 || p2c.cout != f3 || p2c.taps != 1 || p2c.cout_pad != f3)
                        return h->fail(BOD_ERR_INVALID_ARG, "conv '%s2c' must be 1x1 %d->%d", cb, f1, f3);
                    ConvGroup& G = op2b.conv.g[0];
                    G.ch_w2 = p2c.w; G.ch_b2 = p2c.bias; G.ch_res = shortcut.d; G.ch_out = out.d; G.ch_c2 = f3;
                    op2b.flops += 2.0 * op2b.conv.M * (double)f3 * f1;
                    op2b.name += "+2c"; op2b.wname[1] = c_ + "2c"; op2b.bnname[1] = b_ + "2c";
                    t1_ready = false;
                    if (bl[1] != 0) {            // the next block of the stage: its 2a (stride 1) rides along, into the other t1 plane
                        char nb[64], nbb[64];
                        snprintf(nb, sizeof nb, "res%d%c_branch2a", st, bl[1]);
                        snprintf(nbb, sizeof nbb, "bn%d%c_branch2a", st, bl[1]);
                        PackedConv p2a;
                        BODCHK(pack_conv(h, nb, nbb, 64, &p2a));
                        if (p2a.cin != f3 || p2a.cout != f1 || p2a.taps != 1 || p2a.cout_pad != f1)
                            return h->fail(BOD_ERR_INVALID_ARG, "conv '%s' must be 1x1 %d->%d", nb, f3, f1);
                        G.ch_w3 = p2a.w; G.ch_b3 = p2a.bias; G.ch_out3 = t1alt.d;
                        op2b.flops += 2.0 * op2b.conv.M * (double)f1 * f3;
                        op2b.name += std::string("+") + nb; op2b.wname[2] = nb; op2b.bnname[2] = nbb;
                        std::swap(t1, t1alt);
                        t1_ready = true;
                    }
                }
                if (first && (st == 3 || st == 4)) {
                    taps[st] = out;
                    Plane fresh;
                    BODCHK(new_plane(h, &fresh, B, hh, ww, f3));
                    x = out;
                    if (use_a) oa = fresh; else ob = fresh;
                    use_a = !use_a;
                    continue;
                }
                x = out;
                use_a = !use_a;
                continue;
            }
            // Stage 2 on the streaming pointwise kernel (conv_pointwise.hip, BC = 256): the 1x1 expansion just added carries the NEXT
            // block's 1x1 reduction -- computed from the finished tile in LDS, written to the t1 plane this block's 3x3 has already
            // consumed -- when the launch is certain to run on that kernel (conv_pointwise_can_fuse_next).  BOD_PW_FUSE_NEXT=0: off.
            // Stage 3 (128 -> 512, the next 2a 512 -> 128) does the same on pw_conv512_next_kernel's 512-channel tile of 32 pixels
            // (conv_pointwise_can_fuse_next3; its own switch, BOD_PW_FUSE_NEXT3=0: off).
            auto fuse_next_2a = [&](const char* blk) -> bod_status {
                if ((st != 2 && st != 3) || blk[1] == 0 || train_mode || h->es != 2 || h->split) return BOD_OK;
                Op& op2c = h->ops.back();
                if (!(st == 2 ? conv_pointwise_can_fuse_next(op2c.conv) : conv_pointwise_can_fuse_next3(op2c.conv)) || op2c.conv.ksplit > 1) return BOD_OK;
                char nb[64], nbb[64];
                snprintf(nb, sizeof nb, "res%d%c_branch2a", st, blk[1]);
                snprintf(nbb, sizeof nbb, "bn%d%c_branch2a", st, blk[1]);
                PackedConv p2a;
                BODCHK(pack_conv(h, nb, nbb, 64, &p2a));
                if (p2a.cin != f3 || p2a.cout != f1 || p2a.taps != 1 || p2a.cout_pad != (st == 2 ? 64 : 128)) return BOD_OK;
                ConvGroup& G = op2c.conv.g[0];
                G.ch_w3 = p2a.w; G.ch_b3 = p2a.bias; G.ch_out3 = t1.d;
                op2c.flops += 2.0 * op2c.conv.M * (double)f1 * f3;
                op2c.name += std::string("+") + nb; op2c.wname[2] = nb; op2c.bnname[2] = nbb;
                pw_t1_ready = true;
                return BOD_OK;
            };
            if (train_mode) {                   // training keeps every activation: fresh planes per block
                BODCHK(new_plane(h, &t1, B, hh, ww, f1));
                BODCHK(new_plane(h, &t2, B, hh, ww, f1));
                BODCHK(new_plane(h, &sc, B, hh, ww, f3));
                BODCHK(new_plane(h, &oa, B, hh, ww, f3));
                BODCHK(new_plane(h, &ob, B, hh, ww, f3));
            }
            Plane& out = use_a ? oa : ob;
            if (*bl == 'a') {
                // Stage 2's ConvBlock: `branch1` (64 -> 256) and `2a` (64 -> 64 + ReLU) are both 1x1 over the pooled plane
                // (feature_extractor.py:283-309).  On the pointwise kernel's 256-channel tile the 2a rides on branch1's input tile
                // (conv_pointwise.hip, dual form): one launch, the plane read once.  BOD_PW_FUSE_DUAL=0: the two launches.
                bool dual = false;
                if (st == 2 && !train_mode && h->es == 2 && !h->split) {
                    BODCHK(add_conv(h, c_ + "1", b_ + "1", x, sc, first_stride, false, false, nullptr));
                    Op& op1 = h->ops.back();
                    PackedConv p2a;
                    BODCHK(pack_conv(h, c_ + "2a", b_ + "2a", 64, &p2a));
                    if (conv_pointwise_can_fuse_dual(op1.conv) && op1.conv.ksplit <= 1 && p2a.cin == 64 && p2a.cout == f1 && f1 == 64 &&
                        p2a.taps == 1 && p2a.cout_pad == 64) {
                        ConvGroup& G = op1.conv.g[0];
                        G.ch_w3 = p2a.w; G.ch_b3 = p2a.bias; G.ch_out3 = t1.d; G.ch_dual = 1;
                        op1.flops += 2.0 * op1.conv.M * (double)f1 * 64.0;
                        op1.name += std::string("+") + c_ + "2a"; op1.wname[2] = c_ + "2a"; op1.bnname[2] = b_ + "2a";
                        dual = true;
                    } else {
                        h->ops.pop_back();            // planned below in the reference's order
                    }
                }
                if (!dual) BODCHK(add_conv(h, c_ + "2a", b_ + "2a", x, t1, first_stride, false, true, nullptr));
                BODCHK(add_conv(h, c_ + "2b", b_ + "2b", t1, t2, 1, true, true, nullptr));
                if (!dual) BODCHK(add_conv(h, c_ + "1", b_ + "1", x, sc, first_stride, false, false, nullptr));
                BODCHK(add_conv(h, c_ + "2c", b_ + "2c", t2, out, 1, false, true, &sc));
                BODCHK(fuse_next_2a(bl));
                // the C3 / C4 taps are the block-'a' outputs (:119-120,:126-127): keep them alive
                if (st == 3 || st == 4) {
                    taps[st] = out;
                    Plane fresh;
                    BODCHK(new_plane(h, &fresh, B, hh, ww, f3));
                    x = out;
                    if (use_a) oa = fresh; else ob = fresh;
                    use_a = !use_a;
                    continue;
                }
            } else {
                if (!pw_t1_ready) BODCHK(add_conv(h, c_ + "2a", b_ + "2a", x, t1, 1, false, true, nullptr));
                pw_t1_ready = false;
                const bool stage_end_blk = bl[1] == 0 && st <= 4;          // read at the pixels (2y, 2x) only (above)
                BODCHK(add_conv(h, c_ + "2b", b_ + "2b", t1, t2, 1, true, true, nullptr, nullptr, 1, stage_end_blk && stage_end >= 2 && st == 4));
                BODCHK(add_conv(h, c_ + "2c", b_ + "2c", t2, out, 1, false, true, &x, nullptr, stage_end_blk && stage_end >= 1 ? 2 : 1));
                BODCHK(fuse_next_2a(bl));
            }
            x = out;
            use_a = !use_a;
        }
    }
    const Plane c5 = x, c4 = taps[4], c3 = taps[3];

    // ---------------- FPN (feature_decoder.py:136-171)
    h->pyramid.C = 256; h->pyramid.bstride = h->Ppad;
    BODCHK(h->dalloc(&h->pyramid.d, (size_t)B * h->Ppad * 256 * h->es));
    Plane c5r, m4, m3, p6relu;
    BODCHK(new_plane(h, &c5r, B, h->lh[2], h->lw[2], 256));
    BODCHK(new_plane(h, &m4, B, h->lh[1], h->lw[1], 256));
    BODCHK(new_plane(h, &m3, B, h->lh[0], h->lw[0], 256));
    // relu(P6) shares the pyramid layout so one row table serves both outputs of the P6 conv
    char* p6relu_buf = nullptr;
    BODCHK(h->dalloc(&p6relu_buf, (size_t)B * h->Ppad * 256 * h->es));
    p6relu = h->pyramid; p6relu.d = p6relu_buf;
    BODCHK(add_conv(h, "C5_reduced", "", c5, c5r, 1, false, false, nullptr));
    BODCHK(add_conv(h, "P5", "", c5r, level_view(h, 2), 1, true, false, nullptr));
    BODCHK(add_conv(h, "P6", "", c5, level_view(h, 3), 2, true, false, nullptr, p6relu_buf));
    {
        Plane v = p6relu; v.base = h->lvl_off[3]; v.h = h->lh[3]; v.w = h->lw[3]; v.pitch = h->lw[3] + 2;
        BODCHK(add_conv(h, "P7", "", v, level_view(h, 4), 2, true, false, nullptr));
    }
    BODCHK(add_conv(h, "C4_reduced", "", c4, m4, 1, false, false, &c5r));     // + nearest-up(c5r)
    BODCHK(add_conv(h, "P4", "", m4, level_view(h, 1), 1, true, false, nullptr));
    BODCHK(add_conv(h, "C3_reduced", "", c3, m3, 1, false, false, &m4));      // + nearest-up(m4) (:162-167)
    BODCHK(add_conv(h, "P3", "", m3, level_view(h, 0), 1, true, false, nullptr));

    // ---------------- heads (multitask_headers.py; retinanet_model.py:78-109)
    const size_t act_elems = (size_t)B * N * h->Ppad * 256 * h->es;
    for (int hd = 0; hd < 3; ++hd) {
        if (hd == 2 && !c.has_covar_head) continue;
        if (train_mode) {                       // every tower activation is kept for the backward pass
            for (int l = 0; l < kHeadConvs[hd]; ++l) BODCHK(h->dalloc(&h->head_act_t[hd][l], act_elems));
            continue;
        }
        BODCHK(h->dalloc(&h->head_act[hd][0], act_elems));
        BODCHK(h->dalloc(&h->head_act[hd][1], act_elems));
    }
    const int out_ch[3] = {c.anchors_per_location * c.num_classes, c.anchors_per_location * 4, c.anchors_per_location * 10};
    // row tables: layer 1 (pyramid -> N dropout variants), layers 2.. (per sample), output 1x1
    std::vector<RowEnt> t1, t2, t3;
    {
        PyramidGeometry pg = pyramid_geometry(h->lh, h->lw);      // (plan_tables.h; bod_create laid the planes out with the same function's formulas)
        if (pg.Ppad != h->Ppad || pg.P != h->P) return h->fail(BOD_ERR_INVALID_ARG, "pyramid geometry mismatch");
        head_row_tables(pg, B, N, t1, t2, t3);
    }
    RowEnt *d1 = nullptr, *d2 = nullptr, *d3 = nullptr;
    BODCHK(h->dalloc(&d1, t1.size(), false));
    BODCHK(h->dalloc(&d2, t2.size(), false));
    BODCHK(h->dalloc(&d3, t3.size(), false));
    HIPCHK(h, hipMemcpyAsync(d1, t1.data(), t1.size() * sizeof(RowEnt), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d2, t2.data(), t2.size() * sizeof(RowEnt), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d3, t3.data(), t3.size() * sizeof(RowEnt), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));

    // Activation row reuse for the per-sample 3x3 tower layers: re-pack the rows into 256-slot tiles made
    // of runs of x-adjacent pixels and list each tile's extended input rows (kernels.h, ConvArgs::ext).
    RowEnt* d2x = nullptr; int2* dext = nullptr; int m2x = 0;
    bool xreuse = (h->es == 2 || h->split) && !train_mode;      // bf16, bf16x3 and f16mx: the per-sample tower layers (and, `xreuse0` below, the fan-out layer) on the row-reuse loop
    if (const char* e = getenv("BOD_CONV_XREUSE")) xreuse = xreuse && atoi(e) != 0;
    // f16mx precision: the towers' arithmetic exists in the row-reuse kernel only, which therefore runs them at every size (the tile
    // heuristics below choose between kernels of equal results; here the kernel IS the arithmetic).  BOD_TOWER_MX=0: plain bf16x3 towers.
    bool mx_plan = h->mx != 0 && xreuse;
    const int mxf = h->mx;                 // tower row format: 1 = hx, 2 = h4
    if (const char* e = getenv("BOD_TOWER_MX")) mx_plan = mx_plan && atoi(e) != 0;
    {
        ConvArgs probe{};
        probe.M = B * N * h->P; probe.cout_pad = 256; probe.fan_count = 1; probe.flags = CONV_RELU;
        xreuse = xreuse && (mx_plan || conv_igemm_uses_full_cout_tile(probe));
    }
    // rows -> 256-slot tiles of x-adjacent runs + each tile's extended input rows (kernels.h, ConvArgs::ext)
    static_assert(sizeof(ExtRow) == sizeof(int2), "ExtRow is the host-side twin of int2");
    auto make_xr_tiles = [&](const std::vector<RowEnt>& src, RowEnt** d_rows, int2** d_ext, int* m_out) -> bod_status {
        std::vector<RowEnt> tiled;
        std::vector<ExtRow> ext;
        if (!xr_tile_rows(src, tiled, ext)) return h->fail(BOD_ERR_INVALID_ARG, "row-reuse tiling: extended rows out of order");
        *m_out = (int)tiled.size();
        BODCHK(h->dalloc(d_rows, tiled.size(), false));
        BODCHK(h->dalloc(d_ext, ext.size(), false));
        HIPCHK(h, hipMemcpyAsync(*d_rows, tiled.data(), tiled.size() * sizeof(RowEnt), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(*d_ext, ext.data(), ext.size() * sizeof(int2), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return BOD_OK;
    };
    if (xreuse) BODCHK(make_xr_tiles(t2, &d2x, &dext, &m2x));
    // the first tower layer (one convolution per image, N-way dropout fan-out epilogue) takes the row-reuse loop too once
    // its launch is on the 256x256 tile (conv_igemm.hip: from 1 024 tiles on): activation reads x4.5 -> x1.2 of the
    // algorithmic bytes (profiles/round1_head_conv_pmc.json, launch 0).
    RowEnt* d1x = nullptr; int2* dext1 = nullptr; int m1x = 0;
    bool xreuse0 = xreuse;          // (N = 1: no fan-out, a plain three-head launch over the pyramid -- on the same loop since round 4: 1.07 -> 1.23 PFLOP/s)
    {
        ConvArgs probe{};
        probe.M = B * h->P; probe.cout_pad = 256; probe.fan_count = N; probe.flags = CONV_RELU | CONV_DROPOUT; probe.groups = c.has_covar_head ? 3 : 2;
        xreuse0 = xreuse0 && conv_igemm_uses_full_cout_tile(probe);
    }
    if (mx_plan) xreuse0 = true;           // (the first tower layer writes the hx rows the next one reads)
    // ... and reads hx rows itself: the pyramid, which the FPN's kernels write as (hi, lo) pairs, is converted once per forward (1.5 GB
    // in, 1.5 GB out per 256 frames: 0.7 ms) so that the three first-layer convs run at 1.5 instead of 3 products too.  Not on overlap
    // handles (two pyramid buffers).  BOD_MX_LAYER0=0: the bf16x3 loop on the pair rows (conv_igemm_mx_kernel<2>).
    bool mx_l0 = mx_plan && !c.pipeline_overlap;
    if (const char* e = getenv("BOD_MX_LAYER0")) mx_l0 = mx_l0 && atoi(e) != 0;
    if (mx_l0) BODCHK(h->dalloc(&h->pyr_hx, (size_t)B * h->Ppad * 256 * 4));
    if (xreuse0) BODCHK(make_xr_tiles(t1, &d1x, &dext1, &m1x));

    const bool mc = train_mode || std::max(N, c.mc_ensemble_size) > 1;    // mc_dropout_enabled (retinanet_model.py:74-77); training: dropout on (:113-129)
    const uint32_t thr = (uint32_t)std::floor((double)c.dropout_rate * 65536.0);
    const float dscale = (float)(1.0 / (1.0 - (double)c.dropout_rate));
    const int nheads = c.has_covar_head ? 3 : 2;
    // which heads are still running a tower conv at `layer`
    // Fuse each head's 1x1 output conv into the epilogue of its last tower layer whenever that layer runs
    // with the full 256-channel cout tile (bf16 mode, enough rows): the last tower activation then never
    // goes to HBM and three launches disappear.  BOD_FUSE_HEAD_OUTPUT=0 keeps the separate launches.
    // (bf16x3: the fused form exists in the row-reuse kernel's epilogue only -- `xreuse` below -- with the same products in the
    // same order as the separate 1x1 launches: bit-identical head outputs either way)
    bool fuse_out = (h->es == 2 || (h->split && xreuse)) && !train_mode;
    if (const char* e = getenv("BOD_FUSE_HEAD_OUTPUT")) fuse_out = fuse_out && atoi(e) != 0;
    {
        ConvArgs probe{};
        probe.M = B * N * h->P; probe.cout_pad = 256; probe.fan_count = 1; probe.flags = CONV_RELU;
        fuse_out = fuse_out && (mx_plan || conv_igemm_uses_full_cout_tile(probe));
    }
    // ---- MC aggregation fused into the last tower layers' epilogues (inference_utils.py:31-60,
    // :220-244): a tile of those layers must hold ALL N samples of its pixels, so they get their own row table -- tiles of
    // Q <= 256 / N pixel slots, row = slot * N + sample, made of runs of x-adjacent pixels whose extended rows (run + 2,
    // once per sample) fit the 320 staged rows.  BOD_FUSE_AGGREGATION=0 keeps the raw tensors + the posterior's own loops.
    bool agg = xreuse && fuse_out && N >= 2 && 256 / N >= 1 && 320 / N - 2 >= 1 && (c.mc_ensemble_size <= N || c.mc_statistics);      // (a statistics handle's record is one part of a larger ensemble's by design)
    if (const char* e = getenv("BOD_FUSE_AGGREGATION")) agg = agg && atoi(e) != 0;
    RowEnt* d2a = nullptr; int2* dexta = nullptr; int m2a = 0;
    if (agg) {
        std::vector<RowEnt> tiled;
        std::vector<ExtRow> ext;
        const int rc = xr_tile_rows_aggregated(t2, B, N, h->P, tiled, ext);
        if (rc == 1) return h->fail(BOD_ERR_INVALID_ARG, "aggregated tiling: no pixel fits a tile (N = %d)", N);
        if (rc == 2) return h->fail(BOD_ERR_INVALID_ARG, "aggregated tiling: extended rows out of order");
        m2a = (int)tiled.size();
        BODCHK(h->dalloc(&d2a, tiled.size(), false));
        BODCHK(h->dalloc(&dexta, ext.size(), false));
        HIPCHK(h, hipMemcpyAsync(d2a, tiled.data(), tiled.size() * sizeof(RowEnt), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(dexta, ext.data(), ext.size() * sizeof(int2), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        const size_t BA = (size_t)B * h->A;
        BODCHK(h->dalloc(&h->agg[0], BA * c.num_classes));
        BODCHK(h->dalloc(&h->agg[1], BA * 16));
        if (c.has_covar_head) BODCHK(h->dalloc(&h->agg[2], BA * 10));
        if (h->class_parts) BODCHK(h->dalloc(&h->ent, BA));
    } else {
        BODCHK(ensure_raw(h));                 // the ops below reference the raw tensors directly
    }
    if (c.mc_statistics) {                     // the accumulator and, on plans without the aggregating flavour, stat_from_raw_kernel's output
        const size_t BA = (size_t)B * h->A;
        const size_t per[3] = {(size_t)c.num_classes, 16, 10};
        for (int k = 0; k < (c.has_covar_head ? 3 : 2); ++k)
            if (!h->agg[k]) BODCHK(h->dalloc(&h->agg[k], BA * per[k]));
        if (h->class_parts && !h->ent) BODCHK(h->dalloc(&h->ent, BA));
        BODCHK(ensure_stat(h));
    }
    // ---- Sparse tail: only the classification head's statistics decide which anchors are kept (post_sample_kernel), and everything
    // behind the filter reads the box and covariance statistics of kept anchors only (post_fuse_kernel, through anchor_index) -- about
    // 2 % of them at the reference's operating point.  So the launch of the heads that end at layer 2 (box regression) and at layer 3
    // (covariance) moves behind the classification head's last layer and the keep flags, and runs over the pixels with a kept anchor
    // (SparseTailArgs): the same rows, products and epilogue as the dense launch, for those pixels.  BOD_SPARSE_TAIL=0: the dense plan.
    // (Not on pipeline_overlap handles, the experimental CU-partitioned mode: they keep the dense plan.)
    // (Nor on statistics handles: the kept set depends on the MERGED class statistics, so every anchor's record must exist.)
    bool sparse = agg && h->es == 2 && !h->split && !mx_plan && !c.pipeline_overlap && !c.mc_statistics &&
                  h->A == h->P * c.anchors_per_location && h->P <= 65536;
    if (const char* e = getenv("BOD_SPARSE_TAIL")) sparse = sparse && atoi(e) != 0;
    // ---- Sparse halo: the tail's 3x3 windows read box layer 1's and covariance layer 2's outputs only around the tail's pixels, and
    // nothing else reads them in an aggregating forward.  So in aggregating forwards those two convs leave the dense launches of
    // layers 1 and 2 and run as one launch behind the keep stage, over the 3x3 dilation of the tail's pixels (sparse_tables.h
    // ST_HALO).  Raw forwards keep today's launches of layers 1 and 2; materialise_raw re-runs the two convs densely (Op::raw_use).
    // BOD_SPARSE_HALO=0: the tail alone.
    bool halo = sparse && !train_mode;
    if (const char* e = getenv("BOD_SPARSE_HALO")) halo = halo && atoi(e) != 0;
    if (sparse) {
        SparseTailArgs& sa = h->sparse;
        const int tables = halo ? 2 : 1;
        sa.B = B; sa.N = N; sa.P = h->P; sa.apl = c.anchors_per_location; sa.Ppad = h->Ppad;
        // both tables: B * (P / st_min_pixels + 1) tiles of 256 rows (8 KiB) + XR_EXT_ROWS extended rows (2.5 KiB) each; 512 frames
        // of 512x512 at N = 10: 279 552 tiles, 3.0 GB per table
        sa.cap_tiles = B * (h->P / st_min_pixels(N) + 1);
        // The tail's tiles have 192 rows -- three 16-row pixel fragments per wave instead of four: its tiles close on their extended
        // rows at 15 of 25 slots (N = 10), so the fourth fragment multiplied padding (conv_igemm.hip, BP = 192).  Same pixels in as
        // many tiles (+0.1 %), each with three quarters of the MFMAs.  BOD_SPARSE_TAIL_ROWS=256: the 256-row tiles, A/B twin.
        sa.tail_rows = 192;
        if (const char* e = getenv("BOD_SPARSE_TAIL_ROWS")) { if (atoi(e) == 256) sa.tail_rows = 256; }
        {
            // the launch needs the 256-cout tile for its M = cap_tiles * rows (launch_conv_igemm refuses it otherwise): cap_tiles is at
            // least 2.4 times the dense tile count, so 0.75 of it passes wherever the dense launch did -- checked, not assumed
            ConvArgs probe{};
            probe.M = sa.cap_tiles * sa.tail_rows; probe.cout_pad = 256; probe.fan_count = 1; probe.flags = CONV_RELU;
            if (!conv_igemm_uses_full_cout_tile(probe)) sa.tail_rows = 256;
        }
        // (the fewest pixels of a closed tile are set by the extended rows, about 106 / N < 192 / N: cap_tiles holds for either height)
        if (st_min_pixels(N, sa.tail_rows) != st_min_pixels(N))
            return h->fail(BOD_ERR_INVALID_ARG, "sparse tail: %d-row tiles change the tile bound at N = %d", sa.tail_rows, N);
        sa.lv.n = 5;
        {
            const PyramidGeometry pg = pyramid_geometry(h->lh, h->lw);
            for (int l = 0; l < 5; ++l) { sa.lv.lw[l] = pg.lw[l]; sa.lv.lh[l] = pg.lh[l]; sa.lv.p0[l] = (int32_t)pg.lvl_p0[l]; }
        }
        RowEnt* pix = nullptr;
        BODCHK(h->dalloc(&pix, (size_t)h->P, false));
        HIPCHK(h, hipMemcpyAsync(pix, t2.data(), (size_t)h->P * sizeof(RowEnt), hipMemcpyHostToDevice, h->stream));     // image 0, sample 0
        HIPCHK(h, hipStreamSynchronize(h->stream));
        sa.pix = pix;
        BODCHK(h->dalloc(&sa.rows, (size_t)sa.cap_tiles * sa.tail_rows, false));
        BODCHK(h->dalloc(&sa.ext, (size_t)sa.cap_tiles * XR_EXT_ROWS, false));
        if (halo) {
            BODCHK(h->dalloc(&sa.halo_rows, (size_t)sa.cap_tiles * 256, false));
            BODCHK(h->dalloc(&sa.halo_ext, (size_t)sa.cap_tiles * XR_EXT_ROWS, false));
        }
        BODCHK(h->dalloc(&sa.tile_count, 2));
        BODCHK(h->dalloc(&sa.runs, (size_t)tables * B * h->P, false));
        BODCHK(h->dalloc(&sa.chunks, (size_t)tables * B * h->P, false));
        BODCHK(h->dalloc(&sa.tiles, (size_t)tables * B * h->P, false));
    }
    h->plan_sparse = sparse;
    h->plan_halo = halo;
    h->plan_tail_rows = sparse ? h->sparse.tail_rows : 0;
    Op sparse_op; sparse_op.kind = Op::CONV; sparse_op.is_head3x3 = true; sparse_op.flavour = FLAVOUR_AGG;
    int sparse_groups = 0; PackedConv sparse_pc{};
    Op halo_op = sparse_op;
    int halo_groups = 0; PackedConv halo_pc{};
    h->agg_plan = agg; h->plan_fused_out = fuse_out; h->plan_xreuse = xreuse; h->plan_xreuse0 = xreuse0; h->plan_mx = mx_plan ? mxf : 0;
    // A layer's launch takes the sample-complete ("aggregated") tiling only for the heads that END there (fused 1x1 + MC aggregation): such
    // a tile holds 25 pixels x 10 samples = 250 of its 256 rows (240 at N = 30), so every other head's conv of that layer -- the
    // classification and covariance towers at layer 2 -- would pay 2.8 % (6 %) more MFMA work for nothing.  Round 4: those heads run the
    // layer as their own launch on the plain tiling (part 0); the ending heads' launch (part 1) exists in the two flavours.
    // f16mx4: all towers on h4 rows (e2m1 cross terms).  BOD_MX4_BOX_HX=1 keeps the box-regression tower on hx rows (e2m3) -- the epistemic
    // covariance is a sample variance of N nearly equal boxes and amplifies the box outputs' rounding error; measured on the BASELINE-size
    // frames: fused covariance entries 2.5e-3 -> 1.8e-3 (f16mx: 5e-4), 1 024 -> 1 000 frames/s (f16mx: 944) -- as separate launches from
    // layer 1 on; layer 0 then reads ONE pyramid (hx) and writes each head's format.
    int hfmt[3] = {mxf, mxf, mxf};
    if (mxf == 2) { const char* e = getenv("BOD_MX4_BOX_HX"); if (e && atoi(e) != 0) hfmt[1] = 1; }
    // f16mx, round 6: the CLASSIFICATION tower alone runs on h4 rows (e2m1 cross terms: three quarters of the staged bytes and K-tiles of 3
    // of the 8 per-sample convs) -- its logits go through a softmax and a 30-draw categorical and lose nothing measurable (raw class
    // logits 1.2e-4 against 9.3e-5 on hx rows; the bench line's gate: every clause unchanged, categorical draw flips 1 -> 5 of 1 600
    // detections), while the box and covariance towers, whose rounding reaches the fused covariance entries, stay on hx rows.  The same
    // mixed plan as above: the towers run as one launch per format from layer 1 on.  +1.6-2.1 % frames/s.  BOD_MX_CLS_H4=0: all on hx rows.
    if (mxf == 1) { static const bool cls_h4 = [] { const char* e = getenv("BOD_MX_CLS_H4"); return !e || atoi(e) != 0; }(); if (cls_h4) hfmt[0] = 2; }
    const bool mixed = mx_plan && hfmt[0] != hfmt[1];
    const int pyr_fmt = mixed ? 1 : mxf;
    h->pyr_fmt = pyr_fmt;
    for (int layer = 0; layer < 4; ++layer)
    for (int fpass = 0; fpass < 2; ++fpass)
    for (int part = 0; part < 2; ++part)
    for (int flav = (agg && layer >= 2) ? FLAVOUR_RAW : FLAVOUR_BOTH; flav <= ((agg && layer >= 2) ? FLAVOUR_AGG : FLAVOUR_BOTH); ++flav) {
        const bool split_launch = agg && layer >= 2;       // part 0: heads that continue, part 1: heads that end at this layer
        if (fpass == 1 && (!mixed || layer == 0)) continue;
        const int lfmt = !mx_plan ? 0 : layer == 0 ? pyr_fmt : mixed ? (fpass == 0 ? 2 : 1) : mxf;       // row format this launch READS
        if (!split_launch && part == 1) continue;
        if (split_launch && part == 0 && flav == FLAVOUR_AGG) continue;      // the continuing heads' launch is the same in both flavours: planned once
        const bool both = split_launch && part == 0;
        Op op; op.kind = Op::CONV; op.is_head3x3 = true; op.flavour = both ? FLAVOUR_BOTH : flav;
        int g = 0; PackedConv pc0{};
        double fused_flops = 0;
        const bool both_flav = op.flavour == FLAVOUR_BOTH;
        // the halo's dense twins: the layer's full launch for raw forwards, the halo conv alone for materialise_raw
        ConvGroup raw_cg{}; PackedConv raw_pc{}; std::string raw_wname; bool has_raw = false;
        ConvGroup full_cg[3]{}; std::string full_wname[3]; PackedConv full_pc{}; int nfull = 0;
        for (int hd = 0; hd < nheads; ++hd) {
            if (layer >= kHeadConvs[hd]) continue;
            if (split_launch && (part == 1) != (layer == kHeadConvs[hd] - 1)) continue;
            if (mixed && layer > 0 && hfmt[hd] != lfmt) continue;
            PackedConv pc;
            BODCHK(pack_conv(h, std::string(kHeadPrefix[hd]) + "_" + std::to_string(layer), "", 128, &pc, (mx_plan && (layer > 0 || mx_l0)) ? lfmt : 0));
            if (pc.cin != 256 || pc.cout != 256 || pc.taps != 9)
                return h->fail(BOD_ERR_INVALID_ARG, "head conv %s_%d must be 3x3 256->256", kHeadPrefix[hd], layer);
            op.wname[g] = std::string(kHeadPrefix[hd]) + "_" + std::to_string(layer);
            ConvGroup cg{};
            cg.in = layer == 0 ? (mx_l0 ? h->pyr_hx : h->pyramid.d) : (train_mode ? h->head_act_t[hd][layer - 1] : h->head_act[hd][(layer + 1) & 1]);
            cg.w = pc.w; cg.bias = pc.bias;
            cg.out = train_mode ? h->head_act_t[hd][layer] : h->head_act[hd][layer & 1];
            cg.layer_id = hd * 4 + layer;
            cg.out_hx = (mx_plan && layer < kHeadConvs[hd] - 1) ? hfmt[hd] : 0;      // read by the head's next tower layer: hx rows; a last layer feeds the 1x1: pairs
            if (fuse_out && layer == kHeadConvs[hd] - 1) {
                PackedConv po;
                BODCHK(pack_conv(h, kHeadPrefix[hd], "", 32, &po));
                if (po.cin != 256 || po.cout != out_ch[hd] || po.taps != 1)
                    return h->fail(BOD_ERR_INVALID_ARG, "head output conv %s must be 1x1 256->%d (got %d->%d)", kHeadPrefix[hd], out_ch[hd], po.cin, po.cout);
                cg.w2 = po.w; cg.bias2 = po.bias; cg.out2 = h->raw[hd]; cg.cout2 = po.cout; cg.out2_cstride = out_ch[hd];
                op.head[g] = hd;
                if (flav == FLAVOUR_AGG) {             // reduce over the MC samples inside the tile instead of writing [B,N,A,.]
                    cg.out2 = nullptr;
                    cg.agg_kind = hd == 0 ? AGG_CLS : hd == 1 ? AGG_BOX : AGG_COV;
                    cg.agg_n = N; cg.agg_P = h->P; cg.agg_C = c.num_classes; cg.agg_out = h->agg[hd]; cg.anchors = h->d_anchors;
                    if (hd == 0 && h->class_parts) { cg.agg_kind = AGG_CLS_ENT; cg.out2 = h->ent; }      // + sum_n H(softmax) [B,A]
                }
                fused_flops += 2.0 * ((double)B * N * h->P) * 256.0 * out_ch[hd];      // the 1x1 output conv runs inside this launch
            }
            if (halo && both_flav && ((layer == 1 && hd == 1) || (layer == 2 && hd == 2))) {
                // -> the halo launch, planned behind the keep stage; the dense launch stays, for the raw flavour alone
                halo_op.conv.g[halo_groups] = cg;
                halo_op.wname[halo_groups] = op.wname[g];
                if (halo_groups++ == 0) halo_pc = pc;
                halo_op.flops += 2.0 * ((double)B * N * h->P) * 256.0 * 2304.0;      // (the dense launch's algorithmic count, as the tail's)
                raw_cg = cg; raw_pc = pc; raw_wname = op.wname[g]; has_raw = true;
                if (nfull == 0) full_pc = pc;
                full_cg[nfull] = cg; full_wname[nfull++] = op.wname[g];
                op.wname[g].clear();
                continue;
            }
            if (sparse && flav == FLAVOUR_AGG && hd != 0) {          // -> the sparse tail's launch, planned behind the keep stage
                sparse_op.conv.g[sparse_groups] = cg;
                sparse_op.wname[sparse_groups] = op.wname[g];
                sparse_op.head[sparse_groups] = hd;
                if (sparse_groups++ == 0) sparse_pc = pc;
                // the dense launch's algorithmic count: the profiler's head-conv FLOPs stay those of the dense plan
                sparse_op.flops += 2.0 * ((double)B * N * h->P) * 256.0 * 2304.0 + 2.0 * ((double)B * N * h->P) * 256.0 * out_ch[hd];
                fused_flops -= 2.0 * ((double)B * N * h->P) * 256.0 * out_ch[hd];
                op.head[g] = -1; op.wname[g].clear();
                continue;
            }
            op.conv.g[g] = cg;
            if (g == 0) pc0 = pc;
            if (nfull == 0) full_pc = pc;
            full_cg[nfull] = cg; full_wname[nfull++] = op.wname[g];
            ++g;
        }
        if (g == 0 && !has_raw) continue;                    // (no head of this part at this layer)
        const int M = layer == 0 ? B * h->P : B * N * h->P;
        if (has_raw) op.flavour = FLAVOUR_AGG;               // the layer without the halo conv: aggregating forwards only
        for (int twin = 0; twin < 3; ++twin) {
            if (twin == 0 ? g == 0 : !has_raw) continue;
            if (twin > 0) {
                op = Op{}; op.kind = Op::CONV; op.is_head3x3 = true; op.flavour = FLAVOUR_RAW; fused_flops = 0;
                if (twin == 1) {                             // today's launch of the layer, for raw forwards
                    for (int q = 0; q < nfull; ++q) { op.conv.g[q] = full_cg[q]; op.wname[q] = full_wname[q]; }
                    pc0 = full_pc; g = nfull; op.raw_use = Op::RAW_FORWARD;
                } else {                                     // the halo conv densely, for materialise_raw
                    op.conv.g[0] = raw_cg; op.wname[0] = raw_wname;
                    pc0 = raw_pc; g = 1; op.raw_use = Op::RAW_RERUN;
                }
            }
            ConvArgs a = base_args(pc0, layer == 0 ? d1 : d2, M, 256, 256);
            for (int q = 0; q < g; ++q) a.g[q] = op.conv.g[q];
            a.groups = g;
            a.flags = CONV_RELU | (mc ? CONV_DROPOUT : 0);
            a.fan_count = layer == 0 ? N : 1;
            a.fan_stride = (int32_t)h->Ppad;
            a.drop_threshold = thr; a.drop_scale = dscale;
            a.mx = mx_plan ? ((layer == 0 && !mx_l0) ? 2 : (lfmt == 2 ? 3 : 1)) : 0;
            op.hx_pyramid = mx_l0 && layer == 0;
            // which waves of the f16mx loop issue the weight pieces (conv_igemm.hip: 0 all / 1 lower four / 2 upper four; same-box A/B at
            // 256 frames, two rounds each: towers 198.0 / 196.2 / 199.7 ms).  The bf16 tower loop keeps 0: the same pairing measured
            // 0.8 % SLOWER there (211.6 against 209.9 ms per 512 frames)
            a.mx_loader = mx_plan ? 1 : 0;
            if (xreuse0 && layer == 0) { a.rows = d1x; a.M = m1x; a.ext = dext1; a.xreuse = 2; }
            if (xreuse && layer > 0) {
                a.rows = d2x; a.M = m2x; a.ext = dext;
                if (split_launch && part == 1) { a.rows = d2a; a.M = m2a; a.ext = dexta; }       // sample-complete tiles (both flavours)
                a.xreuse = 2;       // 32-bit activation offsets against the tile's first extended row: any buffer size
            }
            op.conv = a;
            op.flops = 2.0 * M * 256.0 * 2304.0 * g + fused_flops;
            op.name = "head_tower_layer_" + std::to_string(layer) + (twin == 1 ? "(raw)" : twin == 2 ? "(rerun)" : has_raw ? "(aggregating)" :
                      both ? "" : flav == FLAVOUR_AGG ? "(aggregating)" : flav == FLAVOUR_RAW ? "(raw)" : "");
            op.same_geom = N == 1;            // pyramid [B][Ppad] and head planes [B*N][Ppad] coincide at N = 1
            h->ops.push_back(op);
        }
    }
    if (sparse_groups > 0) {
        Op keep; keep.kind = Op::KEEP; keep.flavour = FLAVOUR_AGG; keep.name = "head_tower_layer_3(keep)";
        h->ops.push_back(keep);
        const SparseTailArgs& sa = h->sparse;
        if (halo_groups > 0) {           // box layer 1 + covariance layer 2 over the halo table: plain epilogue, the tile count on the device
            ConvArgs a = base_args(halo_pc, sa.halo_rows, sa.cap_tiles * 256, 256, 256);
            for (int q = 0; q < halo_groups; ++q) a.g[q] = halo_op.conv.g[q];
            a.groups = halo_groups;
            a.flags = CONV_RELU | (mc ? CONV_DROPOUT : 0);
            a.fan_count = 1; a.fan_stride = (int32_t)h->Ppad;
            a.drop_threshold = thr; a.drop_scale = dscale;
            a.ext = sa.halo_ext; a.xreuse = 2; a.tile_count = sa.tile_count + 1;
            halo_op.conv = a;
            halo_op.name = "head_tower_layer_2(halo)";
            h->ops.push_back(halo_op);
        }
        ConvArgs a = base_args(sparse_pc, sa.rows, sa.cap_tiles * sa.tail_rows, 256, 256);
        a.tile_rows = sa.tail_rows;
        for (int q = 0; q < sparse_groups; ++q) a.g[q] = sparse_op.conv.g[q];
        a.groups = sparse_groups;
        a.flags = CONV_RELU | (mc ? CONV_DROPOUT : 0);
        a.fan_count = 1; a.fan_stride = (int32_t)h->Ppad;
        a.drop_threshold = thr; a.drop_scale = dscale;
        a.ext = sa.ext; a.xreuse = 2; a.tile_count = sa.tile_count;
        sparse_op.conv = a;
        sparse_op.name = "head_tower_layer_3(sparse)";
        h->ops.push_back(sparse_op);
    }
    for (int hd = 0; hd < nheads && !fuse_out; ++hd) {
        PackedConv pc;
        BODCHK(pack_conv(h, kHeadPrefix[hd], "", 64, &pc));
        if (pc.cin != 256 || pc.cout != out_ch[hd] || pc.taps != 1)
            return h->fail(BOD_ERR_INVALID_ARG, "head output conv %s must be 1x1 256->%d (got %d->%d)", kHeadPrefix[hd], out_ch[hd], pc.cin, pc.cout);
        Op op; op.kind = Op::CONV;
        ConvArgs a = base_args(pc, d3, B * N * h->P, 256, out_ch[hd]);
        a.g[0] = ConvGroup{train_mode ? h->head_act_t[hd][kHeadConvs[hd] - 1] : h->head_act[hd][(kHeadConvs[hd] - 1) & 1], pc.w, pc.bias, h->raw[hd], nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, 0, 0};
        a.flags = CONV_OUT_F32;
        op.conv = a;
        op.flops = 2.0 * a.M * pc.cout * 256.0;
        op.name = kHeadPrefix[hd]; op.wname[0] = kHeadPrefix[hd];
        h->ops.push_back(op);
    }
    if (h->splitk_elems) {
        BODCHK(h->dalloc(&h->splitk_partial, h->splitk_elems));
        for (Op& o : h->ops) if (o.kind == Op::CONV && o.conv.ksplit > 1) o.conv.partial = h->splitk_partial;
    }
    if (h->split) for (Op& o : h->ops) if (o.kind == Op::CONV) to_split_args(&o.conv);
    h->first_head_op = (int)h->ops.size();
    for (size_t i = 0; i < h->ops.size(); ++i) if (h->ops[i].is_head3x3) { h->first_head_op = (int)i; break; }
    h->pyr_d[0] = h->pyramid.d;
    // BOD_DUMP_OPS=1: the plan, one line per op on stderr, with the ALGORITHMIC bytes of the launch (input pixels read once, output and
    // shortcut once, weights once) -- tests/tools/op_table.py joins it with a rocprofv3 kernel trace into a per-op roofline table
    if (const char* e = getenv("BOD_DUMP_OPS")) if (atoi(e) != 0) {
        fprintf(stderr, "# ops: index name kind flavour M taps cin cout groups fan has_res fused_next flops bytes\n");
        for (size_t i = 0; i < h->ops.size(); ++i) {
            const Op& o = h->ops[i];
            const ConvArgs& a = o.conv;
            double bytes = 0;
            if (o.kind == Op::STEM)                    // fp32 frames in, pooled 64-channel plane out (the fused stem + pool kernel)
                bytes = (double)B * c.image_h * c.image_w * 3 * 4 + (double)B * h->ph * h->pw * 64 * h->es;
            if (o.kind == Op::CONV) {
                const double es = (a.flags & CONV_OUT_F32) ? 4.0 : (double)h->es;
                for (int g = 0; g < a.groups; ++g) {
                    bytes += (double)a.M * a.cin * h->es;                                                    // input pixels (stride-2 3x3: ~4x that)
                    bytes += (double)a.M * std::max(1, a.fan_count) * a.cout_valid * es;                     // output(s)
                    if (a.g[g].res) bytes += (double)a.M * a.cout_valid * h->es;
                    if (a.g[g].ch_w3) bytes += (double)a.M * (a.cin == 128 ? 128 : 64) * h->es;      // the fused 2a's plane (stage 3: 128 channels)
                    bytes += (double)a.taps * a.cin * a.cout_pad * h->es;
                }
            }
            fprintf(stderr, "# op %zu %s %d %d %d %d %d %d %d %d %d %d %.6g %.6g\n", i, o.name.c_str(), (int)o.kind, o.flavour, a.M, a.taps, a.cin,
                    a.cout_valid, a.groups, a.fan_count, o.kind == Op::CONV && a.g[0].res ? 1 : 0, o.kind == Op::CONV && a.g[0].ch_w3 ? 1 : 0, o.flops, bytes);
        }
    }
    if (h->overlap_mode) BODCHK(h->dalloc(&h->pyr_d[1], (size_t)B * h->Ppad * 256 * h->es));      // zero borders like the first
    return BOD_OK;
}

bod_status alloc_post(bod_context* h) {
    const bod_config& c = h->cfg;
    const size_t BA = (size_t)c.batch * h->A;
    const int nblocks = (h->A + 255) / 256;
    PostBuffers& p = h->pb;
    BODCHK(h->dalloc(&p.keep, BA));
    BODCHK(h->dalloc(&p.d_counts, BA * c.num_classes));
    BODCHK(h->dalloc(&p.block_counts, (size_t)c.batch * nblocks));
    BODCHK(h->dalloc(&p.num_kept, (size_t)c.batch));
    BODCHK(h->dalloc(&p.counts, BA * c.num_classes));
    BODCHK(h->dalloc(&p.score, BA * c.num_classes));
    BODCHK(h->dalloc(&p.means, BA * 4));
    BODCHK(h->dalloc(&p.covs, BA * 16));
    BODCHK(h->dalloc(&p.ranking, BA));
    BODCHK(h->dalloc(&p.corners, BA * 4));
    BODCHK(h->dalloc(&p.anchor_index, BA));
    BODCHK(h->dalloc(&h->d_anchors, (size_t)h->A * 4));
    const size_t BApad = (size_t)h->cfg.batch * ((h->A + 511) & ~(size_t)511);   // nms_kernel pads its queue to 512
    BODCHK(h->dalloc(&h->nms_scores, BApad));
    BODCHK(h->dalloc(&h->nms_begin, BApad));
    const size_t BK = (size_t)c.batch * c.nms_max_output_size;
    const bool cov_parts = (c.covariance_parts & BOD_PARTS_COVARIANCE) != 0;
    const size_t stage_bytes = record_layout(h).total();
    for (RecordSlot& r : h->rec) {
        BODCHK(h->dalloc(&r.nms_sel, BK));
        BODCHK(h->dalloc(&r.nms_nsel, (size_t)c.batch));
        BODCHK(h->dalloc(&r.scores, BK * c.num_classes));
        BODCHK(h->dalloc(&r.means, BK * REC_MEAN));
        BODCHK(h->dalloc(&r.covs, BK * REC_COV));
        BODCHK(h->dalloc(&r.counts, BK * c.num_classes));
        if (cov_parts) { BODCHK(h->dalloc(&r.parts, BK * REC_PARTS)); r.parts_ok.assign((size_t)c.batch, 0); }
        if (h->class_parts) { BODCHK(h->dalloc(&r.cparts, BK * REC_CPARTS)); r.cparts_ok.assign((size_t)c.batch, 0); }
        if (hipHostMalloc(reinterpret_cast<void**>(&r.host_stage), stage_bytes, hipHostMallocDefault) != hipSuccess)
            return h->fail(BOD_ERR_OOM, "pinned host staging buffer (%zu bytes)", stage_bytes);
    }
    if (cov_parts) {
        BODCHK(h->dalloc(&h->parts, BA * BOD_PARTS_TRI));
        h->parts_ok.assign((size_t)c.batch, 0);
    }
    if (h->class_parts) {
        BODCHK(h->dalloc(&h->cparts, BA * (3 + (size_t)c.num_classes)));
        h->cparts_ok.assign((size_t)c.batch, 0);
    }
    BODCHK(h->dalloc(&h->d_images, (size_t)c.batch * c.image_h * c.image_w * 3));
    h->d_images_b[0] = h->d_images;
    return BOD_OK;
}

PostCfg post_cfg(bod_context* h, uint64_t seed, uint32_t first_image) {
    const bod_config& c = h->cfg;
    PostCfg p{};
    p.B = c.batch; p.N = c.mc_samples; p.A = h->A; p.C = c.num_classes; p.draws = c.num_categorical_draws;
    p.use_full_covar = c.use_full_covar; p.has_covar = c.has_covar_head; p.dirichlet = c.dirichlet_non_informative;
    p.gaussian_iso = c.gaussian_isotropic; p.ranking_method = c.ranking_method; p.iso_var = c.isotropic_variance;
    p.kitti_sh = c.kitti_scale_h; p.kitti_sw = c.kitti_scale_w;
    p.kitti_frame = c.kitti_scale_h > 0.f ? h->kscale_now : nullptr;
    p.seed_lo = (uint32_t)seed; p.seed_hi = (uint32_t)(seed >> 32); p.image_base = first_image;
    return p;
}

// flavour: FLAVOUR_RAW = per-sample head outputs into raw[] (RetinaNetModel.call's tensors), FLAVOUR_AGG = MC statistics
// reduced inside the last tower layers' tiles (plans with agg_plan only).  only_flavoured: run just the ops that differ
// between the two (materialise_raw re-runs the raw flavour of the last layers on the activations still in HBM).
// ---- rocprofv3 markers (tracing): with BOD_ROCTX=1 every stage of a step is bracketed by a roctx range --
// bod:stem, bod:res2 .. bod:res5, bod:fpn, bod:head_tower_layer_k, bod:posterior, bod:nms, bod:cluster_fuse, bod:collect,
// bod:upload -- so that `rocprofv3 --marker-trace --kernel-trace` lays the kernels of a step out by stage.  The roctx library is
// opened at run time (no link dependency; without the variable not a single call is made).  The ranges bracket the ENQUEUE of a
// stage on the host; the stage timers of the C ABI (bod_profile_begin / bod_profile_end) are the device-side figures.
struct Markers {
    bool on = false;
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Markers() {
        const char* e = getenv("BOD_ROCTX");
        if (!e || !atoi(e)) return;
        void* lib = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) { fprintf(stderr, "bayesod: BOD_ROCTX=1 but no roctx library could be opened (%s)\n", dlerror()); return; }
        push = reinterpret_cast<int (*)(const char*)>(dlsym(lib, "roctxRangePushA"));
        pop = reinterpret_cast<int (*)()>(dlsym(lib, "roctxRangePop"));
        on = push && pop;
    }
};
static Markers& markers() { static Markers m; return m; }
struct MarkerRange {                    // scope = one range
    bool on;
    explicit MarkerRange(const char* name) : on(markers().on) { if (on) markers().push(name); }
    ~MarkerRange() { if (on) markers().pop(); }
    MarkerRange(const MarkerRange&) = delete;
    MarkerRange& operator=(const MarkerRange&) = delete;
};
// BOD_STEM_SPLIT_FUSED=0: the (hi, lo) precisions keep the fp32 stem and the pooling launch (read by the forward pass and bod_stage_stem)
static bool stem_split_fused_enabled() {
    static const bool on = [] { const char* e = getenv("BOD_STEM_SPLIT_FUSED"); return !e || atoi(e) != 0; }();
    return on;
}
// stage of a forward op, from its name: conv1 / pool1 -> stem, resK* -> resK, C?_reduced / P? -> fpn, head_tower_layer_k(...) -> itself
static std::string op_stage(const std::string& name) {
    if (name.rfind("conv1", 0) == 0 || name.rfind("pool1", 0) == 0) return "bod:stem";
    if (name.rfind("res", 0) == 0 && name.size() > 3) return "bod:" + name.substr(0, 4);
    if (name.rfind("head_tower_layer_", 0) == 0) return "bod:" + name.substr(0, name.find('(') == std::string::npos ? name.size() : name.find('('));
    if (name.rfind("pyramid_", 0) == 0) return "bod:head_outputs";      // separate 1x1 output convs (plans without the fused epilogue)
    return "bod:fpn";
}

// Records ev_img_free for the image buffer the current call reads (bod_device_images_buffer(k)): everything enqueued on the main
// stream so far has finished with the frames once the event fires; bod_upload_frames_u8_async makes the copy stream wait on it.
bod_status mark_images_consumed(bod_context* h, hipStream_t st = nullptr) {
    if (h->cur_img_buf >= 0 && h->copy) {
        HIPCHK(h, hipEventRecord(h->ev_img_free[h->cur_img_buf], st ? st : h->stream));
        h->img_free_pending[h->cur_img_buf] = true;
    }
    return BOD_OK;
}

// Every entry point but the pipelined ones (bod_infer_async, bod_collect, bod_gather_detections of a ticket, the asynchronous upload)
// works on the unmasked `full` stream: it first waits for whatever the partition's two streams still hold.
bod_status join_overlap(bod_context* h) {
    if (!h->ov_dirty) return BOD_OK;
    HIPCHK(h, hipStreamSynchronize(h->front));
    HIPCHK(h, hipStreamSynchronize(h->back));
    h->ov_dirty = false;
    return BOD_OK;
}

// overlapped (bod_infer_async on a pipeline_overlap handle; h->stream == h->back for the call): the ops in front of the first head
// launch go to h->front, the pyramid they write is buffer `fwd_parity` of two, and two events hand it to the back and take it back.
bod_status run_forward(bod_context* h, const float* dev_images, uint64_t seed, uint32_t first_image, int flavour = FLAVOUR_RAW,
                       bool only_flavoured = false, bool overlapped = false) {
    const bod_config& c = h->cfg;
    if (flavour == FLAVOUR_RAW && !only_flavoured) BODCHK(ensure_raw(h));
    const bool ov = overlapped && h->overlap_mode != 0 && !only_flavoured;
    hipStream_t fs = ov ? h->front : h->stream;
    int par = 0;
    if (ov) {
        par = h->fwd_parity; h->fwd_parity ^= 1;
        if (h->l0_pending[par]) { HIPCHK(h, hipStreamWaitEvent(fs, h->ev_l0_done[par], 0)); h->l0_pending[par] = false; }
    }
    if (!only_flavoured) { h->pyr_last = par; h->keep_ready = false; }
    // Kernel CHOICES (sliding-window / pointwise / fused-stem eligibility: launch_conv_igemm, workgroups against compute units) are made
    // against the WHOLE chip on every stream: a CU-masked front stream that chose by its own 32 CUs ran other kernels than bod_infer
    // and a serial handle at mid-size batches (64 frames at 512x512: 64 column strips >= 32 take slide3x3_c128, which re-associates one
    // fp32 add per output, < 256 do not) and broke the header's "bit-identical to the serial pipeline" (round-4 advisor finding).  The
    // overlap mode is an opt-in A/B switch that measured slower: the contract wins over its planner.
    const int cus_front = h->n_cu;
    const int cus_back = h->n_cu;
    // BOD_TRACE_OPS=k: the k-th forward call is traced op by op (HIP events on the engine stream) and a table
    // is printed to stderr -- a development aid (tests/tools), off by default.
    static const int trace_call = getenv("BOD_TRACE_OPS") ? atoi(getenv("BOD_TRACE_OPS")) : 0;
    static int call_no = 0;
    const bool trace = trace_call > 0 && ++call_no == trace_call && !ov;
    std::vector<hipEvent_t> tev;
    if (trace) {
        tev.resize(h->ops.size() + 1);
        for (hipEvent_t& e : tev) HIPCHK(h, hipEventCreate(&e));
        HIPCHK(h, hipEventRecord(tev[0], h->stream));
    }
    size_t op_i = 0;
    bool stem_pool_fused = false;
    std::string cur_stage;                                        // open marker range (BOD_ROCTX=1)
    struct StageCloser { std::string& s; ~StageCloser() { if (!s.empty()) markers().pop(); } } stage_closer{cur_stage};
    for (Op& op : h->ops) {
        if (trace && op_i > 0) HIPCHK(h, hipEventRecord(tev[op_i], h->stream));
        const bool is_front = (int)op_i < h->first_head_op;
        const bool first_back = (int)op_i == h->first_head_op;
        hipStream_t st = is_front ? fs : h->stream;
        ++op_i;
        if ((op.flavour != FLAVOUR_BOTH && op.flavour != flavour) || (only_flavoured && op.flavour == FLAVOUR_BOTH)) continue;
        if (op.raw_use == (only_flavoured ? Op::RAW_FORWARD : Op::RAW_RERUN)) continue;
        if ((int)op_i - 1 < h->dev_op_lo || (int)op_i - 1 >= h->dev_op_hi) continue;          // (BOD_FORWARD_OPS: development)
        if (ov && first_back) {                          // the pyramid is complete: hand it to the back
            HIPCHK(h, hipEventRecord(h->ev_front_done[par], fs));
            HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_front_done[par], 0));
        }
        if (markers().on) {
            std::string st = op_stage(op.name);
            if (st != cur_stage) {
                if (!cur_stage.empty()) markers().pop();
                markers().push(st.c_str());
                cur_stage.swap(st);
            }
        }
        switch (op.kind) {
            case Op::STEM: {
                // bf16 inference on rows of <= 256 stem pixels: stem + zero-pad + max-pool in one kernel (the stem plane is never
                // written; aux_kernels.hip, BOD_STEM_POOL_FUSED=0: the two launches).  Training handles keep the plane (pool backward).
                const Op* pool = op_i < h->ops.size() && h->ops[op_i].kind == Op::POOL ? &h->ops[op_i] : nullptr;
                // Round 6: the (hi, lo) precisions take the same walk on three bf16 products (their stem was the exact fp32 kernel + a
                // pooling launch: 5.2 ms per 256 frames against 0.8); BOD_STEM_SPLIT_FUSED=0: as before.
                stem_pool_fused = pool && !h->train && (h->split ? stem_split_fused_enabled() : h->es == 2) && !trace &&
                                  stem_pool_fused_applies(dev_images, c.batch, c.image_w, h->sw, is_front ? cus_front : cus_back);
                if (stem_pool_fused)
                    HIPCHK(h, launch_stem_pool_fused(dev_images, h->stem_w, h->stem_b, pool->conv.g[0].out, h->split ? 1 : 0, c.batch, c.image_h,
                                                     c.image_w, h->sh, h->sw, h->ph, h->pw, h->pw + 2, (h->ph + 2) * (h->pw + 2), st));
                else
                HIPCHK(h, launch_stem_conv(dev_images, h->stem_w, h->stem_b, h->stem_out, h->es == 4, c.batch, c.image_h,
                                           c.image_w, h->sh, h->sw, st));
                // the frames are consumed: the copy stream may refill this buffer.  (Training handles read the frames again in the
                // backward pass -- bf16 copy + stem weight gradient -- and record the event at the end of the step instead:
                // mark_images_consumed, train_impl.inc)
                if (!h->train) BODCHK(mark_images_consumed(h, st));
                break;
            }
            case Op::KEEP: {
                // the posterior's keep flags, then the sparse tail's row table from them -- on the device, no host round trip.  The
                // flags and counts are the posterior's buffers: ordered behind the readers of an earlier call as run_posterior is.
                BODCHK(wait_pending_slots(h, st));
                PostCfg pc = post_cfg(h, seed, first_image);
                pc.aggregated = 1;
                PostBuffers pb = h->pb;
                pb.agg_cls = h->agg[0];
                HIPCHK(h, launch_posterior_keep(pc, pb, st));
                SparseTailArgs sa = h->sparse;
                sa.keep = h->pb.keep;
                HIPCHK(h, launch_sparse_tail_rows(sa, st));
                // BOD_SPARSE_STATS=1 (diagnostic; it waits for the stream and reads the tail table back): how many tiles the tables got
                // and how full the tail's are
                static const bool sparse_stats = [] { const char* e = getenv("BOD_SPARSE_STATS"); return e && atoi(e) != 0; }();
                if (sparse_stats) {
                    HIPCHK(h, hipStreamSynchronize(st));
                    int32_t cnt[2] = {0, 0};
                    HIPCHK(h, hipMemcpy(cnt, sa.tile_count, sizeof cnt, hipMemcpyDeviceToHost));
                    const int R = sa.tail_rows;
                    long valid = 0, full = 0;
                    if (cnt[0] > 0 && cnt[0] <= sa.cap_tiles) {
                        std::vector<int32_t> off((size_t)cnt[0] * R);
                        HIPCHK(h, hipMemcpy2D(off.data(), sizeof(int32_t), &sa.rows[0].out_off, sizeof(RowEnt), sizeof(int32_t), off.size(), hipMemcpyDeviceToHost));
                        for (int t = 0; t < cnt[0]; ++t) {
                            int v = 0;
                            for (int r = 0; r < R; ++r) v += off[(size_t)t * R + r] >= 0 ? 1 : 0;
                            valid += v;
                            full += v == R ? 1 : 0;       // no padding row: the tile closed on its slots and R is a multiple of N
                        }
                    }
                    const long dense = ((long)sa.B * sa.N * sa.P + 255) / 256;
                    std::fprintf(stderr, "BOD_SPARSE_STATS: tail %d tiles of %d rows, %.1f valid rows per tile (%ld rows = %.3f of the dense launch's), %ld tiles with all %d rows valid; "
                                 "halo %d tiles of 256 rows; dense plain tiles %ld; capacity %d tiles\n", (int)cnt[0], R,
                                 cnt[0] > 0 ? (double)valid / cnt[0] : 0.0, valid, (double)valid / ((double)sa.B * sa.N * sa.P), full, R, (int)cnt[1], dense, (int)sa.cap_tiles);
                }
                h->keep_ready = true; h->keep_seed = seed; h->keep_first = first_image;
                break;
            }
            case Op::POOL:
                if (stem_pool_fused) break;
                HIPCHK(h, launch_stem_pool(h->stem_out, op.conv.g[0].out, h->split ? 2 : (h->es == 4 ? 1 : 0), c.batch,
                                           h->sh, h->sw, h->ph, h->pw, h->pw + 2, (h->ph + 2) * (h->pw + 2), st));
                break;
            case Op::CONV: {
                if (op.hx_pyramid) HIPCHK(h, launch_pairs_to_hx(h->pyramid.d, h->pyr_hx, (long)c.batch * h->Ppad, 256, st, h->pyr_fmt));
                op.conv.seed_lo = (uint32_t)seed; op.conv.seed_hi = (uint32_t)(seed >> 32);
                op.conv.image_base = first_image;
                op.conv.sample_base = (uint32_t)c.mc_sample_base;
                op.conv.dyn_rng = train_dyn_rng(h);              // training: device copy of {seed, image id} (graph replay)
                const bool is_tower = op.conv.xreuse != 0 && op.conv.fan_count <= 1;        // per-sample tower launches (one kernel symbol)
                const bool timed = h->profiling && op.is_head3x3 && (h->prof_which == 0 || (h->prof_which == 1) == is_tower);
                hipEvent_t e0 = nullptr, e1 = nullptr;
                if (timed) {
                    HIPCHK(h, hipEventCreate(&e0)); HIPCHK(h, hipEventCreate(&e1));
                    HIPCHK(h, hipEventRecord(e0, st));
                }
                op.conv.n_cu = is_front ? cus_front : cus_back;          // compute units this launch may fill (planner: workgroups vs CUs)
                if (par != 0) {                                  // the second pyramid buffer of an overlap handle
                    ConvArgs a = op.conv;
                    for (int g = 0; g < a.groups; ++g) {
                        if (a.g[g].in == h->pyr_d[0]) a.g[g].in = h->pyr_d[1];
                        if (a.g[g].out == h->pyr_d[0]) a.g[g].out = h->pyr_d[1];
                    }
                    HIPCHK(h, (h->es == 4 && !h->split) ? launch_conv_igemm_f32(a, st) : launch_conv_igemm(a, st));
                } else
                HIPCHK(h, (h->es == 4 && !h->split) ? launch_conv_igemm_f32(op.conv, st) : launch_conv_igemm(op.conv, st));
                if (timed) {
                    HIPCHK(h, hipEventRecord(e1, st));
                    h->ev_head.emplace_back(e0, e1);
                    h->prof_flops += op.flops;
                }
                if (ov && first_back) {                          // the fan-out layer has read pyramid `par`
                    HIPCHK(h, hipEventRecord(h->ev_l0_done[par], h->stream));
                    h->l0_pending[par] = true;
                }
                break;
            }
        }
    }
    if (trace) {
        HIPCHK(h, hipEventRecord(tev[h->ops.size()], h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        fprintf(stderr, "# op trace: name kind M taps cin cout_pad groups fan ms TFLOP/s\n");
        for (size_t i = 0; i < h->ops.size(); ++i) {
            float ms = 0.f;
            HIPCHK(h, hipEventElapsedTime(&ms, tev[i], tev[i + 1]));
            const Op& o = h->ops[i];
            fprintf(stderr, "%-28s %d %8d %2d %5d %5d %d %2d %9.4f %8.1f\n", o.name.c_str(), (int)o.kind, o.conv.M, o.conv.taps,
                    o.conv.cin, o.conv.cout_pad, o.conv.groups, o.conv.fan_count, ms, o.flops / (ms * 1e-3) / 1e12);
        }
        for (hipEvent_t& e : tev) hipEventDestroy(e);
    }
    h->stage.forward_ran();
    h->last_seed = seed; h->last_first_image = first_image;
    if (!only_flavoured) { h->last_sample_base = c.mc_sample_base; h->bb_samples_ok = false; }
    if (flavour == FLAVOUR_AGG) { h->agg_valid = true; h->raw_valid = false; h->agg_sparse = h->plan_sparse; }
    else { h->raw_valid = true; if (!only_flavoured) h->agg_valid = false; }
    return BOD_OK;
}

// The raw head outputs of the last forward, for callers that ask for them after an aggregating bod_infer: the last tower
// layers' raw flavour is re-run on the activations still in HBM (same seed, same Philox streams: exactly the tensors a
// raw-flavour forward would have produced).
bod_status materialise_raw(bod_context* h) {
    if (h->raw_valid || !h->agg_valid) { BODCHK(ensure_raw(h)); return BOD_OK; }
    BODCHK(ensure_raw(h));
    const bool prof = h->profiling;
    h->profiling = false;
    const StageState stage = h->stage;
    const int32_t base = h->cfg.mc_sample_base;
    h->cfg.mc_sample_base = h->last_sample_base;
    const bod_status st = run_forward(h, h->cur_images, h->last_seed, h->last_first_image, FLAVOUR_RAW, true);
    h->cfg.mc_sample_base = base;
    h->profiling = prof;
    h->stage = stage;
    return st;
}

bod_status run_posterior(bod_context* h, uint64_t seed, uint32_t first_image) {
    if (!h->anchors_ready) return h->fail(BOD_ERR_NOT_READY, "bod_set_anchors has not been called");
    BODCHK(wait_pending_slots(h, h->stream));
    MarkerRange mr("bod:posterior");
    PostCfg pc = post_cfg(h, seed, first_image);
    PostBuffers pb = h->pb;
    pb.cls = h->raw[0]; pb.box = h->raw[1]; pb.cov = h->raw[2]; pb.anchors = h->d_anchors;
    pc.aggregated = (h->agg_valid && !h->raw_valid) ? 1 : 0;        // statistics from the conv epilogue, no [B,N,A,.] tensors
    pb.agg_cls = h->agg[0]; pb.agg_box = h->agg[1]; pb.agg_cov = h->agg[2];
    // bod_infer: the forward's keep stage already sampled with this seed.  A posterior under another seed may keep other anchors,
    // whose box / covariance statistics the sparse tail did not compute: it takes the raw tensors (re-run on the activations in HBM).
    const bool keep_done = pc.aggregated && h->keep_ready && seed == h->keep_seed && first_image == h->keep_first;
    h->keep_ready = false;
    if (pc.aggregated && h->agg_sparse && (seed != h->keep_seed || first_image != h->keep_first)) {
        BODCHK(materialise_raw(h));
        pc.aggregated = 0;
        pb.cls = h->raw[0]; pb.box = h->raw[1]; pb.cov = h->raw[2];
    }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (h->profiling) {
        HIPCHK(h, hipEventCreate(&e0)); HIPCHK(h, hipEventCreate(&e1));
        HIPCHK(h, hipEventRecord(e0, h->stream));
    }
    HIPCHK(h, keep_done ? launch_posterior_fuse(pc, pb, h->stream) : launch_posterior(pc, pb, h->stream));
    if (h->parts) { HIPCHK(h, launch_posterior_parts(pc, pb, h->parts, h->stream)); std::fill(h->parts_ok.begin(), h->parts_ok.end(), 1); }
    if (h->cparts) { HIPCHK(h, launch_posterior_class_parts(pc, pb, h->ent, h->cparts, h->stream)); std::fill(h->cparts_ok.begin(), h->cparts_ok.end(), 1); }
    if (h->cfg.ranking_method == BOD_RANK_JOINT_ENTROPY && h->cfg.gaussian_isotropic && h->cfg.dirichlet_non_informative)
        HIPCHK(h, launch_joint_entropy_rank(pc, pb, h->stream));
    if (h->profiling) { HIPCHK(h, hipEventRecord(e1, h->stream)); h->ev_post.emplace_back(e0, e1); }
    h->stage.posterior_ran();
    return BOD_OK;
}

// validation_utils.post_process_predictions up to the NMS input, on MC sample 0 of the raw head outputs (bod_validation_post)
bod_status run_validation_post(bod_context* h) {
    BODCHK(materialise_raw(h));
    BODCHK(wait_pending_slots(h, h->stream));
    PostCfg pc = post_cfg(h, 0, 0);
    PostBuffers pb = h->pb;
    pb.cls = h->raw[0]; pb.box = h->raw[1]; pb.cov = h->raw[2]; pb.anchors = h->d_anchors;
    HIPCHK(h, launch_validation_post(pc, pb, h->stream));
    if (h->parts) {                                   // covs = 0: so are the three terms
        HIPCHK(h, hipMemsetAsync(h->parts, 0, (size_t)h->cfg.batch * h->A * BOD_PARTS_TRI * sizeof(float), h->stream));
        std::fill(h->parts_ok.begin(), h->parts_ok.end(), 1);
    }
    if (h->cparts) {                                  // one sample, no MC distribution: zero rows
        HIPCHK(h, hipMemsetAsync(h->cparts, 0, (size_t)h->cfg.batch * h->A * (3 + h->cfg.num_classes) * sizeof(float), h->stream));
        std::fill(h->cparts_ok.begin(), h->cparts_ok.end(), 1);
    }
    h->stage.posterior_ran();
    return BOD_OK;
}

bod_status run_nms(bod_context* h, hipStream_t st) {
    MarkerRange mr("bod:nms");
    const bod_config& c = h->cfg;
    NmsArgs a{};
    a.B = c.batch; a.A = h->A; a.num_kept = h->pb.num_kept; a.corners = h->pb.corners; a.ranking = h->pb.ranking;
    a.work_scores = h->nms_scores; a.work_begin = h->nms_begin; a.selected = h->cur().nms_sel; a.num_selected = h->cur().nms_nsel;
    a.max_out = c.nms_max_output_size; a.iou_thr = c.nms_iou_threshold; a.sigma = c.nms_soft_sigma; a.variant = c.nms_variant;
    HIPCHK(h, launch_nms(a, st));
    h->stage.nms_ran();
    return BOD_OK;
}

bod_status run_cluster(bod_context* h, hipStream_t st) {
    MarkerRange mr("bod:cluster_fuse");
    const bod_config& c = h->cfg;
    ClusterArgs a{};
    a.B = c.batch; a.A = h->A; a.C = c.num_classes; a.max_out = c.nms_max_output_size;
    RecordSlot& r = h->cur();
    a.num_kept = h->pb.num_kept; a.selected = r.nms_sel; a.num_selected = r.nms_nsel;
    a.corners = h->pb.corners; a.counts = h->pb.counts; a.means = h->pb.means; a.covs = h->pb.covs;
    a.thr = c.nms_iou_threshold;
    a.affinity = h->stage.affinity_img >= 0 ? h->affinity : nullptr; a.affinity_img = h->stage.affinity_img;
    h->stage.affinity_img = -1;                   // consumed by this call
    a.out_scores = r.scores; a.out_means = r.means; a.out_covs = r.covs; a.out_counts = r.counts;
    if (h->merge_method == BOD_MERGE_BAYES) {
        HIPCHK(h, launch_cluster_fuse(a, st));
    } else {
        const MergeTerms terms{r.merge_within, r.merge_between, r.merge_members};
        HIPCHK(h, launch_cluster_merge(a, h->merge_method, terms, st));
    }
    r.merge_terms_ok = h->merge_method != BOD_MERGE_BAYES;
    if (h->parts) { HIPCHK(h, launch_cluster_parts(a, h->parts, r.parts, st)); r.parts_ok = h->parts_ok; }
    if (h->cparts) { HIPCHK(h, launch_cluster_class_parts(a, h->cparts, r.cparts, st)); r.cparts_ok = h->cparts_ok; }
    h->stage.cluster_ran();
    return BOD_OK;
}

// ---- black-box MC dropout (bayesod.h) ----
// Every buffer of the two stages, on the first switch to the method: the per-image arrays of the validation post-process and of
// nms_kernel for batch * mc_samples virtual images, the sample detections, the pool's work arrays, and the slots' merge terms.
bod_status alloc_blackbox(bod_context* h) {
    if (h->bb.keep) return BOD_OK;
    const bod_config& c = h->cfg;
    const size_t V = (size_t)c.batch * c.mc_samples, VA = V * h->A, VK = V * c.nms_max_output_size, C = c.num_classes;
    const size_t nblocks = (h->A + 255) / 256;
    BlackBoxArgs& a = h->bb;
    uint8_t* keep = nullptr;
    BODCHK(h->dalloc(&keep, VA));
    BODCHK(h->dalloc(&a.top, VA));
    BODCHK(h->dalloc(&a.block_counts, V * nblocks));
    BODCHK(h->dalloc(&a.num_kept, V));
    BODCHK(h->dalloc(&a.ranking, VA));
    BODCHK(h->dalloc(&a.corners, VA * 4));
    BODCHK(h->dalloc(&a.anchor_index, VA));
    const size_t VApad = V * ((h->A + 511) & ~(size_t)511);
    BODCHK(h->dalloc(&a.work_scores, VApad));
    BODCHK(h->dalloc(&a.work_begin, VApad));
    BODCHK(h->dalloc(&a.selected, VK));
    BODCHK(h->dalloc(&a.num_selected, V));
    BODCHK(h->dalloc(&a.sd_score, VK * C));
    BODCHK(h->dalloc(&a.sd_mean, VK * 4));
    BODCHK(h->dalloc(&a.sd_cov, VK * 16));
    BODCHK(h->dalloc(&a.sd_anchor, VK));
    BODCHK(h->dalloc(&a.sd_count, V));
    BODCHK(h->dalloc(&a.pool_top, VK));
    BODCHK(h->dalloc(&a.pool_corners, VK * 4));
    if (!h->rec[1].merge_members) {
        const size_t BK = (size_t)c.batch * c.nms_max_output_size;
        for (RecordSlot& r : h->rec) {
            BODCHK(h->dalloc(&r.merge_within, BK * REC_COV));
            BODCHK(h->dalloc(&r.merge_between, BK * REC_COV));
            BODCHK(h->dalloc(&r.merge_members, BK));
        }
    }
    a.keep = keep;                                    // last: the mark that everything above exists
    return BOD_OK;
}

BlackBoxArgs blackbox_args(bod_context* h) {
    const bod_config& c = h->cfg;
    BlackBoxArgs a = h->bb;
    a.B = c.batch; a.N = c.mc_samples; a.A = h->A; a.C = c.num_classes; a.max_out = c.nms_max_output_size;
    a.min_score = h->bb_opt.min_score; a.min_members = h->bb_opt.min_members;
    a.thr = h->bb_opt.affinity_threshold > 0.f ? h->bb_opt.affinity_threshold : c.nms_iou_threshold;
    return a;
}

// stage 1: the validation post-process and the soft-NMS of every (image, sample), then the sample detections
bod_status run_blackbox_samples(bod_context* h) {
    if (!h->anchors_ready) return h->fail(BOD_ERR_NOT_READY, "bod_set_anchors has not been called");
    BODCHK(materialise_raw(h));
    BODCHK(wait_pending_slots(h, h->stream));
    MarkerRange mr("bod:blackbox_samples");
    const bod_config& c = h->cfg;
    const PostCfg pc = post_cfg(h, 0, 0);
    PostBuffers pb{};
    pb.cls = h->raw[0]; pb.box = h->raw[1]; pb.cov = h->raw[2]; pb.anchors = h->d_anchors;
    const BlackBoxArgs a = blackbox_args(h);
    NmsArgs n{};
    n.B = c.batch * c.mc_samples; n.A = h->A; n.num_kept = a.num_kept; n.corners = a.corners; n.ranking = a.ranking;
    n.work_scores = a.work_scores; n.work_begin = a.work_begin; n.selected = a.selected; n.num_selected = a.num_selected;
    n.max_out = c.nms_max_output_size; n.iou_thr = c.nms_iou_threshold; n.sigma = c.nms_soft_sigma; n.variant = c.nms_variant;
    HIPCHK(h, launch_blackbox_samples(pc, pb, a, n, h->stream));
    h->bb_samples_ok = true;
    return BOD_OK;
}

// stage 2: the image's pool merged into the current record slot; the detection getters follow as after bod_cluster_fuse
bod_status run_blackbox_merge(bod_context* h, hipStream_t st) {
    MarkerRange mr("bod:blackbox_merge");
    RecordSlot& r = h->cur();
    BlackBoxArgs a = blackbox_args(h);
    a.out_num = r.nms_nsel; a.out_centre = r.nms_sel;
    a.out_scores = r.scores; a.out_means = r.means; a.out_covs = r.covs; a.out_counts = r.counts;
    const MergeTerms terms{r.merge_within, r.merge_between, r.merge_members};
    HIPCHK(h, launch_blackbox_merge(a, terms, st));
    r.merge_terms_ok = true;
    h->stage.posterior_ran();                         // the slot's centres are pooled indices now: no bod_cluster_fuse on them
    h->stage.posterior = false;
    h->stage.cluster_ran();
    return BOD_OK;
}

bod_status stage_images(bod_context* h, const float* images, int on_device, const float** dev, hipStream_t st = nullptr) {
    if (!images) return h->fail(BOD_ERR_INVALID_ARG, "images is NULL");
    if (!st) st = h->stream;                            // the stream the stem will run on
    h->cur_img_buf = -1;
    h->kscale_now = nullptr;
    if (on_device) {
        for (int k = 0; k < 2; ++k)
            if (images == h->d_images_b[k] && h->d_images_b[k]) {
                h->cur_img_buf = k;
                if (h->img_ready_pending[k]) {           // filled by bod_upload_frames_u8_async on the copy stream
                    HIPCHK(h, hipStreamWaitEvent(st, h->ev_img_ready[k], 0));
                    h->img_ready_pending[k] = false;
                }
                if (h->kscale_src[k]) {                  // frames of a ragged upload: their factors become this call's (see kscale_src)
                    float* cur = h->kscale_cur[h->kscale_i];
                    h->kscale_i ^= 1;
                    HIPCHK(h, hipMemcpyAsync(cur, h->kscale_src[k], (size_t)h->cfg.batch * 2 * sizeof(float), hipMemcpyDeviceToDevice, st));
                    h->kscale_now = cur;
                }
            }
        *dev = images;
        return BOD_OK;
    }
    h->kscale_src[0] = nullptr;                         // host float frames replace whatever buffer 0 held
    const size_t bytes = (size_t)h->cfg.batch * h->cfg.image_h * h->cfg.image_w * 3 * sizeof(float);
    HIPCHK(h, hipMemcpyAsync(h->d_images, images, bytes, hipMemcpyHostToDevice, st));
    *dev = h->d_images;
    return BOD_OK;
}

// bod_infer reduces over the MC samples inside the conv epilogue whenever the plan has that flavour and this handle holds the
// whole ensemble (a handle computing a shard of a larger ensemble keeps the raw tensors: the exchange needs them)
int infer_flavour(bod_context* h) {
    const bod_config& c = h->cfg;
    const bool whole = c.mc_sample_base == 0 && (c.mc_ensemble_size == 0 || c.mc_ensemble_size == c.mc_samples);
    return (h->agg_plan && whole && h->anchors_ready) ? FLAVOUR_AGG : FLAVOUR_RAW;
}

template <typename T>
bod_status d2h(bod_context* h, T* dst, const T* src, size_t n) {
    if (!dst || n == 0) return BOD_OK;
    HIPCHK(h, hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, h->stream));
    return BOD_OK;
}

}  // namespace

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

const char* bod_version(void) { return "bayesod-hip 0.1.0 (gfx950)"; }

const char* bod_last_error(bod_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

bod_status bod_create(const bod_config* cfg, bod_handle* out) {
    if (!cfg || !out) { g_create_error = "bod_create: NULL argument"; return BOD_ERR_INVALID_ARG; }
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        g_create_error = "no HIP device visible: libbayesod_hip has no CPU fallback";
        return BOD_ERR_NO_DEVICE;
    }
    std::unique_ptr<bod_context> h(new bod_context());
    h->cfg = *cfg;
    auto bail = [&](bod_status s) { g_create_error = h->err; return s; };
    const bod_config& c = h->cfg;
    if (c.device < 0 || c.device >= ndev) return bail(h->fail(BOD_ERR_INVALID_ARG, "device %d out of range [0,%d)", c.device, ndev));
    if (c.batch < 1 || c.batch > 4096 || c.mc_samples < 1 || c.mc_samples > 4096)
        return bail(h->fail(BOD_ERR_INVALID_ARG, "batch=%d / mc_samples=%d out of range", c.batch, c.mc_samples));
    if (c.mc_sample_base < 0 || c.mc_sample_base + c.mc_samples > 65535 || c.mc_ensemble_size < 0 ||
        (c.mc_ensemble_size > 0 && c.mc_sample_base + c.mc_samples > c.mc_ensemble_size))
        return bail(h->fail(BOD_ERR_INVALID_ARG, "mc_sample_base=%d / mc_samples=%d / mc_ensemble_size=%d inconsistent",
                            c.mc_sample_base, c.mc_samples, c.mc_ensemble_size));
    if (c.training && ((c.precision != BOD_PRECISION_BF16 && c.precision != BOD_PRECISION_FP32) || c.mc_samples != 1))
        return bail(h->fail(BOD_ERR_INVALID_ARG, "training handles run in bf16 (or, for gradient verification, fp32) precision with mc_samples = 1 (dropout stays on)"));
    if (c.backbone_depth != 0 && c.backbone_depth != 50 && c.backbone_depth != 101)
        return bail(h->fail(BOD_ERR_INVALID_ARG, "backbone_depth must be 50 or 101, got %d", c.backbone_depth));
    if (c.num_classes != 4 && c.num_classes != 8)
        return bail(h->fail(BOD_ERR_INVALID_ARG, "num_classes (incl. background) must be 4 or 8, got %d", c.num_classes));
    if (c.anchors_per_location < 1 || (c.anchors_per_location * c.num_classes) % 4 != 0)
        return bail(h->fail(BOD_ERR_INVALID_ARG, "anchors_per_location=%d unsupported", c.anchors_per_location));
    if (!(c.dropout_rate >= 0.f && c.dropout_rate < 1.f)) return bail(h->fail(BOD_ERR_INVALID_ARG, "dropout_rate must be in [0,1)"));
    if (c.num_categorical_draws < 1 || c.num_categorical_draws > 1024) return bail(h->fail(BOD_ERR_INVALID_ARG, "num_categorical_draws out of range"));
    if (c.nms_max_output_size < 1 || c.nms_max_output_size > 512) return bail(h->fail(BOD_ERR_INVALID_ARG, "nms_max_output_size must be in [1,512]"));
    if (c.precision != BOD_PRECISION_BF16 && c.precision != BOD_PRECISION_FP32 && c.precision != BOD_PRECISION_BF16X3 && c.precision != BOD_PRECISION_F16MX && c.precision != BOD_PRECISION_F16MX4)
        return bail(h->fail(BOD_ERR_INVALID_ARG, "precision must be BOD_PRECISION_BF16 (0), BOD_PRECISION_FP32 (1), BOD_PRECISION_BF16X3 (2), BOD_PRECISION_F16MX (3) or BOD_PRECISION_F16MX4 (4)"));
    if (c.mc_statistics != 0 && c.mc_statistics != 1) return bail(h->fail(BOD_ERR_INVALID_ARG, "mc_statistics must be 0 or 1, got %d", c.mc_statistics));
    if (c.mc_statistics && (c.training || c.pipeline_overlap))
        return bail(h->fail(BOD_ERR_INVALID_ARG, "mc_statistics: statistics handles are inference handles on one stream (%s = 1 refused)",
                            c.training ? "training" : "pipeline_overlap"));
    if (c.covariance_parts < 0 || c.covariance_parts > (BOD_PARTS_COVARIANCE | BOD_PARTS_CLASS))
        return bail(h->fail(BOD_ERR_INVALID_ARG, "covariance_parts must be a set of BOD_PARTS_COVARIANCE (1) and BOD_PARTS_CLASS (2), got %d", c.covariance_parts));
    if (c.covariance_parts && c.training)
        return bail(h->fail(BOD_ERR_INVALID_ARG, "covariance_parts: the parts belong to inference and statistics handles (training = 1 refused)"));
    h->class_parts = (c.covariance_parts & BOD_PARTS_CLASS) != 0;
    h->es = c.precision == BOD_PRECISION_BF16 ? 2 : 4;
    h->split = c.precision == BOD_PRECISION_BF16X3 || c.precision == BOD_PRECISION_F16MX || c.precision == BOD_PRECISION_F16MX4;
    h->mx = c.precision == BOD_PRECISION_F16MX ? 1 : c.precision == BOD_PRECISION_F16MX4 ? 2 : 0;
    if (hipSetDevice(c.device) != hipSuccess) return bail(h->fail(BOD_ERR_HIP, "hipSetDevice(%d) failed", c.device));
    // Development switches of the section-8.4 probes (tests/tools/selfcheck_probe.py), read when the handle is created:
    //   BOD_CU_MASK_SLOTS=lo:hi  the handle's main stream may use CU slots [lo, hi) of every XCD only (hipExtStreamCreateWithCUMask);
    //   BOD_FORWARD_OPS=lo:hi    bod_forward runs ops [lo, hi) of the plan only (a company of chosen kernels; the outputs are garbage).
    if (const char* e = getenv("BOD_FORWARD_OPS")) { int lo = 0, hi = 0; if (sscanf(e, "%d:%d", &lo, &hi) == 2 && lo >= 0 && hi > lo) { h->dev_op_lo = lo; h->dev_op_hi = hi; } }
    bool masked_main = false;
    if (const char* e = getenv("BOD_CU_MASK_SLOTS")) {
        int lo = 0, hi = 0;
        hipDeviceProp_t prop;
        if (sscanf(e, "%d:%d", &lo, &hi) == 2 && hipGetDeviceProperties(&prop, c.device) == hipSuccess && prop.multiProcessorCount % 8 == 0 &&
            lo >= 0 && hi > lo && hi <= prop.multiProcessorCount / 8) {
            uint32_t m[8];
            cu_slot_mask(lo, hi, m);
            if (hipExtStreamCreateWithCUMask(&h->stream, 8, m) != hipSuccess) return bail(h->fail(BOD_ERR_HIP, "hipExtStreamCreateWithCUMask failed"));
            masked_main = true;
        } else return bail(h->fail(BOD_ERR_INVALID_ARG, "BOD_CU_MASK_SLOTS=%s: want lo:hi within the XCD's CU slots", e));
    }
    if (!masked_main && hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return bail(h->fail(BOD_ERR_HIP, "hipStreamCreate failed"));
    if (hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking) != hipSuccess) return bail(h->fail(BOD_ERR_HIP, "hipStreamCreate failed"));
    h->full = h->stream;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, c.device) != hipSuccess) return bail(h->fail(BOD_ERR_HIP, "hipGetDeviceProperties failed"));
        h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        // pipeline overlap: BOD_OVERLAP=0 forces it off, =1 on (CU-masked streams), =2 on with two plain streams (A/B aid).
        // The front owns 4 CU slots per XCD (the workgroup dispatcher balances over the four shader engines of an XCD, so only
        // multiples of 4 change anything: tests/tools/cu_mask_probe.hip)
        int want = c.pipeline_overlap ? 1 : 0;
        if (const char* e = getenv("BOD_OVERLAP")) want = atoi(e);
        if (c.training) want = 0;
        // Round 6: the mode runs kernels of this library beside each other by design, and those can miscompute a 16-lane row
        //  -- it is slower than one stream anyway (8.3).  An experiment, never a default: refused without the switch.
        if (want && !(getenv("BOD_OVERLAP_EXPERIMENTAL") && atoi(getenv("BOD_OVERLAP_EXPERIMENTAL")) == 1))
            return bail(h->fail(BOD_ERR_INVALID_ARG, "pipeline_overlap is experimental (slower than one stream and not bit-reproducible: include/bayesod.h, "
                                                     "DESIGN.md 8.3-8.4): set BOD_OVERLAP_EXPERIMENTAL=1 to create such a handle"));
        if (want) {
            const int slots = h->n_cu / 8;
            const int fs = std::max(1, std::min(4, slots - 1));
            const bool masks = want == 1 && h->n_cu % 8 == 0 && slots >= 8 && slots <= 32;
            if (masks) {
                uint32_t mf[8], mb[8];
                cu_slot_mask(slots - fs, slots, mf);
                cu_slot_mask(0, slots - fs, mb);
                if (hipExtStreamCreateWithCUMask(&h->front, 8, mf) != hipSuccess || hipExtStreamCreateWithCUMask(&h->back, 8, mb) != hipSuccess)
                    return bail(h->fail(BOD_ERR_HIP, "hipExtStreamCreateWithCUMask failed"));
                h->overlap_mode = 1; h->ov_front_slots = fs; h->ov_slots = slots;
            } else {
                if (hipStreamCreateWithFlags(&h->front, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithFlags(&h->back, hipStreamNonBlocking) != hipSuccess)
                    return bail(h->fail(BOD_ERR_HIP, "hipStreamCreate failed"));
                h->overlap_mode = 2; h->ov_front_slots = 0; h->ov_slots = slots;
            }
            for (int k = 0; k < 2; ++k)
                if (hipEventCreateWithFlags(&h->ev_front_done[k], hipEventDisableTiming) != hipSuccess ||
                    hipEventCreateWithFlags(&h->ev_l0_done[k], hipEventDisableTiming) != hipSuccess)
                    return bail(h->fail(BOD_ERR_HIP, "hipEventCreate failed"));
            if (hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess) return bail(h->fail(BOD_ERR_HIP, "hipEventCreate failed"));
        }
    }
    if (hipEventCreateWithFlags(&h->ev_posterior, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->rec[0].done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->rec[1].done, hipEventDisableTiming) != hipSuccess)
        return bail(h->fail(BOD_ERR_HIP, "hipEventCreate failed"));
    if (c.mc_statistics && hipEventCreateWithFlags(&h->ev_stat, hipEventDisableTiming) != hipSuccess)
        return bail(h->fail(BOD_ERR_HIP, "hipEventCreate failed"));
    bod_status s = build_geometry(h.get());
    if (s != BOD_OK) return bail(s);
    if ((int64_t)c.batch * c.mc_samples * h->Ppad >= (1LL << 31))
        return bail(h->fail(BOD_ERR_INVALID_ARG, "batch*mc_samples*pixels exceeds 2^31 rows"));
    s = alloc_post(h.get());
    if (s != BOD_OK) return bail(s);
    *out = h.release();
    return BOD_OK;
}

bod_status bod_destroy(bod_handle h) {
    if (!h) return BOD_OK;
    hipSetDevice(h->cfg.device);
    h->stream = h->full;
    if (h->front) { hipStreamSynchronize(h->front); hipStreamDestroy(h->front); }
    if (h->back) { hipStreamSynchronize(h->back); hipStreamDestroy(h->back); }
    for (int k = 0; k < 2; ++k) { if (h->ev_front_done[k]) hipEventDestroy(h->ev_front_done[k]); if (h->ev_l0_done[k]) hipEventDestroy(h->ev_l0_done[k]); }
    if (h->ev_join) hipEventDestroy(h->ev_join);
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->side) { hipStreamSynchronize(h->side); hipStreamDestroy(h->side); }
    if (h->ev_posterior) hipEventDestroy(h->ev_posterior);
    if (h->ev_stat) hipEventDestroy(h->ev_stat);
    for (RecordSlot& r : h->rec) if (r.done) hipEventDestroy(r.done);
    train_destroy(h);
    val_destroy(h);
    for (RecordSlot& r : h->rec) if (r.host_stage) hipHostFree(r.host_stage);
    if (h->rec_recv && h->rec_recv != h->rec_send) hipFree(h->rec_recv);
    if (h->rec_send) hipFree(h->rec_send);
    if (h->ev_gather) hipEventDestroy(h->ev_gather);
    for (void* p : h->allocs) hipFree(p);
    if (h->iou_scratch) hipFree(h->iou_scratch);
    if (h->affinity) hipFree(h->affinity);
    if (h->d_frames_u8) hipFree(h->d_frames_u8);
    if (h->rag_sync.dev) hipFree(h->rag_sync.dev);
    if (h->aug_sync.dev) hipFree(h->aug_sync.dev);
    for (int k = 0; k < 2; ++k) if (h->aug_b[k].dev) hipFree(h->aug_b[k].dev);
    for (int k = 0; k < 2; ++k) { if (h->rag_b[k].dev) hipFree(h->rag_b[k].dev); if (h->ev_tab[k]) hipEventDestroy(h->ev_tab[k]); if (h->kscale_cur[k]) hipFree(h->kscale_cur[k]); }
    if (h->copy) { hipStreamSynchronize(h->copy); hipStreamDestroy(h->copy); }
    for (auto& slots : h->decode_slot) for (DecodeSlot& s : slots) s.release();
    for (CorruptSlot& cs : h->corrupt_slot) cs.release();
    for (int k = 0; k < 2; ++k) {
        if (h->d_u8_b[k]) hipFree(h->d_u8_b[k]);
        if (h->ev_img_ready[k]) hipEventDestroy(h->ev_img_ready[k]);
        if (h->ev_img_free[k]) hipEventDestroy(h->ev_img_free[k]);
    }
    for (auto& e : h->ev_head) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
    for (auto& e : h->ev_post) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
    return BOD_OK;
}

bod_status bod_query_sizes(bod_handle h, bod_sizes* out) {
    if (!h || !out) return BOD_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof *out);
    out->num_pixels = h->P; out->num_anchors = h->A; out->num_levels = h->nlev;
    for (int l = 0; l < h->nlev; ++l) { out->level_h[l] = h->lh[l]; out->level_w[l] = h->lw[l]; }
    out->max_detections = h->cfg.nms_max_output_size;
    out->device_bytes = h->device_bytes;
    return BOD_OK;
}

bod_status bod_update_config(bod_handle h, const bod_config* cfg) {
    if (!h || !cfg) return BOD_ERR_INVALID_ARG;
    const bod_config& o = h->cfg;
    if (cfg->device != o.device || cfg->image_h != o.image_h || cfg->image_w != o.image_w || cfg->batch != o.batch ||
        cfg->mc_samples != o.mc_samples || cfg->num_classes != o.num_classes ||
        cfg->anchors_per_location != o.anchors_per_location || cfg->min_level != o.min_level ||
        cfg->max_level != o.max_level || cfg->has_covar_head != o.has_covar_head || cfg->dropout_rate != o.dropout_rate ||
        cfg->precision != o.precision || cfg->training != o.training || cfg->backbone_depth != o.backbone_depth || cfg->pipeline_overlap != o.pipeline_overlap || cfg->mc_statistics != o.mc_statistics || cfg->covariance_parts != o.covariance_parts || (std::max(cfg->mc_ensemble_size, cfg->mc_samples) > 1) != (std::max(o.mc_ensemble_size, o.mc_samples) > 1))
        return h->fail(BOD_ERR_INVALID_ARG, "bod_update_config: geometry / model fields cannot change on a live handle");
    if (cfg->nms_max_output_size != o.nms_max_output_size)
        return h->fail(BOD_ERR_INVALID_ARG, "bod_update_config: nms_max_output_size sizes device buffers and cannot change");
    if (cfg->num_categorical_draws < 1 || cfg->num_categorical_draws > 1024)
        return h->fail(BOD_ERR_INVALID_ARG, "num_categorical_draws out of range");
    if (cfg->mc_sample_base < 0 || cfg->mc_sample_base + cfg->mc_samples > 65535)
        return h->fail(BOD_ERR_INVALID_ARG, "mc_sample_base + mc_samples must stay below 65536 (16-bit sample field of the RNG counter)");
    h->cfg = *cfg;
    return BOD_OK;
}

bod_status bod_load_weight(bod_handle h, const char* name, int32_t kind, const int64_t* shape, int32_t ndim, const float* data) {
    if (!h) return BOD_ERR_INVALID_ARG;
    if (!name || !shape || !data || ndim < 1 || ndim > 4 || kind < 0 || kind > 5)
        return h->fail(BOD_ERR_INVALID_ARG, "bod_load_weight: bad argument");
    if ((kind == 0) != (ndim == 4)) return h->fail(BOD_ERR_INVALID_ARG, "bod_load_weight('%s'): kind %d needs ndim %d", name, kind, kind == 0 ? 4 : 1);
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) { if (shape[i] <= 0) return h->fail(BOD_ERR_INVALID_ARG, "non-positive dim"); t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
    t.data.assign(data, data + n);
    h->host_w[std::string(name) + "/" + std::to_string(kind)] = std::move(t);
    h->weights_ready = false;
    return BOD_OK;
}

bod_status bod_finalize_weights(bod_handle h) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (h->weights_ready) return BOD_OK;
    if (!h->ops.empty()) return h->fail(BOD_ERR_INVALID_ARG, "weights were already finalized; create a new handle to reload");
    BODCHK(build_plan(h));
    if (h->cfg.training) BODCHK(train_init(h));
    h->host_w.clear();
    h->weights_ready = true;
    return BOD_OK;
}

bod_status bod_set_anchors(bod_handle h, const float* anchors, int32_t n) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    if (!anchors || n != h->A) return h->fail(BOD_ERR_INVALID_ARG, "bod_set_anchors: expected %d anchors, got %d", h->A, n);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemcpyAsync(h->d_anchors, anchors, (size_t)n * 16, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->anchors_ready = true;
    h->mirror_sym = -1;
    return BOD_OK;
}

bod_status bod_upload_images(bod_handle h, const float* host_images) {
    if (!h || !host_images) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t bytes = (size_t)h->cfg.batch * h->cfg.image_h * h->cfg.image_w * 3 * sizeof(float);
    HIPCHK(h, hipMemcpyAsync(h->d_images, host_images, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->kscale_src[0] = nullptr;
    return BOD_OK;
}

// Header and inflate stage alone (bayesod.h): host only, no handle, no device.
bod_status bod_png_info(const uint8_t* data, int64_t len, struct bod_png_info* out) {
    if (!data || !out || len < 0) { g_create_error = "bod_png_info: NULL argument"; return BOD_ERR_INVALID_ARG; }
    std::memset(out, 0, sizeof *out);
    PngHeader h;
    if (png_parse(data, len, &h) != PNG_OK) { g_create_error = std::string("bod_png_info: ") + h.msg; return BOD_ERR_INVALID_ARG; }
    out->width = h.width; out->height = h.height; out->bit_depth = h.bit_depth; out->color_type = h.color_type;
    out->channels = h.channels; out->interlace = h.interlace; out->supported = h.supported; out->raw_bytes = h.raw_bytes;
    g_create_error = h.supported ? "" : std::string("bod_png_info: ") + h.msg;
    return BOD_OK;
}

bod_status bod_png_inflate(const uint8_t* data, int64_t len, uint8_t* raw, int64_t raw_capacity) {
    static const char* who = "bod_png_inflate";
    if (!data || !raw || len < 0) { g_create_error = std::string(who) + ": NULL argument"; return BOD_ERR_INVALID_ARG; }
    PngHeader h;
    if (png_parse(data, len, &h) != PNG_OK) { g_create_error = std::string(who) + ": " + h.msg; return BOD_ERR_INVALID_ARG; }
    if (!h.supported) { g_create_error = std::string(who) + ": not a supported PNG: " + h.msg; return BOD_ERR_INVALID_ARG; }
    if (h.raw_bytes > raw_capacity) {
        g_create_error = std::string(who) + ": the scanlines take " + std::to_string(h.raw_bytes) + " bytes, the buffer holds " + std::to_string(raw_capacity);
        return BOD_ERR_INVALID_ARG;
    }
    char msg[192] = {0};
    if (png_decode(data, len, h, raw, msg, sizeof msg) != PNG_OK) { g_create_error = std::string(who) + ": " + msg; return BOD_ERR_INVALID_ARG; }
    return BOD_OK;
}

// Header and entropy stage alone (bayesod.h): host only, no handle, no device.
bod_status bod_jpeg_info(const uint8_t* data, int64_t len, struct bod_jpeg_info* out) {
    if (!data || !out || len < 0) { g_create_error = "bod_jpeg_info: NULL argument"; return BOD_ERR_INVALID_ARG; }
    std::memset(out, 0, sizeof *out);
    std::unique_ptr<JpegHeader> h(new JpegHeader);
    if (jpeg_parse(data, len, h.get()) != JPEG_OK) { g_create_error = std::string("bod_jpeg_info: ") + h->msg; return BOD_ERR_INVALID_ARG; }
    out->width = h->width; out->height = h->height; out->components = h->components;
    out->h_samp = h->h_samp; out->v_samp = h->v_samp; out->restart_interval = h->restart_interval;
    out->supported = h->supported; out->coef_count = h->coef_count;
    g_create_error = h->supported ? "" : std::string("bod_jpeg_info: ") + h->msg;
    return BOD_OK;
}

bod_status bod_jpeg_entropy_decode(const uint8_t* data, int64_t len, int16_t* coefs, int64_t coef_capacity, uint16_t* quant3x64) {
    static const char* who = "bod_jpeg_entropy_decode";
    if (!data || !coefs || !quant3x64 || len < 0) { g_create_error = std::string(who) + ": NULL argument"; return BOD_ERR_INVALID_ARG; }
    std::unique_ptr<JpegHeader> h(new JpegHeader);
    if (jpeg_parse(data, len, h.get()) != JPEG_OK) { g_create_error = std::string(who) + ": " + h->msg; return BOD_ERR_INVALID_ARG; }
    if (!h->supported) { g_create_error = std::string(who) + ": not a supported JPEG: " + h->msg; return BOD_ERR_INVALID_ARG; }
    if (h->coef_count > coef_capacity) {
        g_create_error = std::string(who) + ": the stream has " + std::to_string(h->coef_count) + " coefficients, the buffer holds " + std::to_string(coef_capacity);
        return BOD_ERR_INVALID_ARG;
    }
    char msg[192] = {0};
    if (jpeg_decode(data, len, *h, coefs, quant3x64, msg, sizeof msg) != JPEG_OK) { g_create_error = std::string(who) + ": " + msg; return BOD_ERR_INVALID_ARG; }
    return BOD_OK;
}

const float* bod_device_images_buffer(bod_handle h, int32_t buffer) {
    return (h && buffer >= 0 && buffer <= 1) ? h->d_images_b[buffer] : nullptr;
}

const float* bod_device_images(bod_handle h) { return h ? h->d_images : nullptr; }

bod_status bod_synchronize(bod_handle h) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    if (h->copy) HIPCHK(h, hipStreamSynchronize(h->copy));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipStreamSynchronize(h->side));
    h->rec[0].pending = h->rec[1].pending = false;
    return BOD_OK;
}

bod_status bod_forward(bod_handle h, const float* images, int32_t on_device, uint64_t seed, uint32_t first_image_id) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    if (!h->weights_ready) return h->fail(BOD_ERR_NOT_READY, "weights not finalized");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const float* dev = nullptr;
    BODCHK(stage_images(h, images, on_device, &dev));
    h->cur_images = dev;
    if (h->train) return train_forward_only(h, dev, seed, first_image_id);     // model(x, 'training'): dropout on, N = 1
    return run_forward(h, dev, seed, first_image_id);
}

bod_status bod_get_raw(bod_handle h, float* cls, float* box, float* cov) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    if (!h->stage.forward) return h->fail(BOD_ERR_NOT_READY, "bod_forward has not run");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    BODCHK(materialise_raw(h));
    const bod_config& c = h->cfg;
    const size_t n = (size_t)c.batch * c.mc_samples * h->A;
    BODCHK(d2h(h, cls, h->raw[0], n * c.num_classes));
    BODCHK(d2h(h, box, h->raw[1], n * 4));
    if (cov) {
        if (!c.has_covar_head) return h->fail(BOD_ERR_INVALID_ARG, "model has no covariance head");
        BODCHK(d2h(h, cov, h->raw[2], n * 10));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BOD_OK;
}

bod_status bod_set_raw(bod_handle h, const float* cls, const float* box, const float* cov) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    HIPCHK(h, hipSetDevice(h->cfg.device));
    BODCHK(ensure_raw(h));
    const bod_config& c = h->cfg;
    const size_t n = (size_t)c.batch * c.mc_samples * h->A;
    h->kscale_now = nullptr;                            // outputs from outside: no ragged batch's factors belong to them
    if (cls) HIPCHK(h, hipMemcpyAsync(h->raw[0], cls, n * c.num_classes * 4, hipMemcpyHostToDevice, h->stream));
    if (box) HIPCHK(h, hipMemcpyAsync(h->raw[1], box, n * 16, hipMemcpyHostToDevice, h->stream));
    if (cov && c.has_covar_head) HIPCHK(h, hipMemcpyAsync(h->raw[2], cov, n * 40, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->stage.forward_ran();
    h->raw_valid = true; h->agg_valid = false; h->bb_samples_ok = false;
    return BOD_OK;
}

bod_status bod_get_pyramid(bod_handle h, int32_t l, float* out) {
    if (!h || !out) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    if (!h->stage.forward || !h->pyramid.d) return h->fail(BOD_ERR_NOT_READY, "bod_forward has not run");
    if (l < 0 || l >= h->nlev) return h->fail(BOD_ERR_INVALID_ARG, "level index %d out of range", l);
    const int B = h->cfg.batch;
    std::vector<char> tmp((size_t)B * h->Ppad * 256 * h->es);
    HIPCHK(h, hipMemcpyAsync(tmp.data(), h->pyr_d[h->pyr_last] ? h->pyr_d[h->pyr_last] : h->pyramid.d, tmp.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const int hh = h->lh[l], ww = h->lw[l], pitch = ww + 2;
    for (int b = 0; b < B; ++b)
        for (int y = 0; y < hh; ++y)
            for (int x = 0; x < ww; ++x) {
                const size_t pix = ((size_t)b * h->Ppad + h->lvl_off[l] + (size_t)(y + 1) * pitch + (x + 1)) * 256;
                float* d = out + (((size_t)b * hh + y) * ww + x) * 256;
                if (h->split) {
                    const uint16_t* s = reinterpret_cast<const uint16_t*>(tmp.data()) + pix * 2;
                    for (int ch = 0; ch < 256; ++ch) { const int slot = (ch >> 5) * 64 + (ch & 31); d[ch] = bf2f(s[slot]) + bf2f(s[slot + 32]); }
                } else if (h->es == 2) {
                    const uint16_t* s = reinterpret_cast<const uint16_t*>(tmp.data()) + pix;
                    for (int ch = 0; ch < 256; ++ch) d[ch] = bf2f(s[ch]);
                } else {
                    std::memcpy(d, reinterpret_cast<const float*>(tmp.data()) + pix, 256 * sizeof(float));
                }
            }
    return BOD_OK;
}

bod_status bod_posterior(bod_handle h, uint64_t seed, uint32_t first_image_id) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    if (!h->stage.forward) return h->fail(BOD_ERR_NOT_READY, "bod_forward / bod_set_raw has not run");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return run_posterior(h, seed, first_image_id);
}

bod_status bod_validation_post(bod_handle h) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    if (!h->stage.forward) return h->fail(BOD_ERR_NOT_READY, "bod_forward / bod_set_raw has not run");
    if (!h->anchors_ready) return h->fail(BOD_ERR_NOT_READY, "bod_set_anchors has not been called");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return run_validation_post(h);
}

bod_status bod_get_num_kept(bod_handle h, int32_t* out) {
    if (!h || !out) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    if (!h->stage.posterior) return h->fail(BOD_ERR_NOT_READY, "bod_posterior has not run");
    BODCHK(d2h(h, out, h->pb.num_kept, (size_t)h->cfg.batch));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BOD_OK;
}

static bod_status image_m(bod_handle h, int32_t img, int32_t* m) {
    if (img < 0 || img >= h->cfg.batch) return h->fail(BOD_ERR_INVALID_ARG, "image index %d out of range", img);
    HIPCHK(h, hipMemcpyAsync(m, h->pb.num_kept + img, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BOD_OK;
}

bod_status bod_get_posterior(bod_handle h, int32_t img, float* counts, float* score, float* means, float* covs, float* ranking, int32_t* anchor_index) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    if (!h->stage.posterior) return h->fail(BOD_ERR_NOT_READY, "bod_posterior has not run");
    int32_t m = 0;
    BODCHK(image_m(h, img, &m));
    const size_t o = (size_t)img * h->A, C = h->cfg.num_classes;
    BODCHK(d2h(h, counts, h->pb.counts + o * C, m * C));
    BODCHK(d2h(h, score, h->pb.score + o * C, m * C));
    BODCHK(d2h(h, means, h->pb.means + o * 4, (size_t)m * 4));
    BODCHK(d2h(h, covs, h->pb.covs + o * 16, (size_t)m * 16));
    BODCHK(d2h(h, ranking, h->pb.ranking + o, (size_t)m));
    BODCHK(d2h(h, anchor_index, h->pb.anchor_index + o, (size_t)m));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BOD_OK;
}

bod_status bod_set_posterior(bod_handle h, int32_t img, int32_t m, const float* counts, const float* means, const float* covs, const float* ranking) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    if (img < 0 || img >= h->cfg.batch || m < 0 || m > h->A) return h->fail(BOD_ERR_INVALID_ARG, "bod_set_posterior: bad image index / M");
    if (m > 0 && (!counts || !means || !covs || !ranking)) return h->fail(BOD_ERR_INVALID_ARG, "bod_set_posterior: NULL array");
    const size_t o = (size_t)img * h->A, C = h->cfg.num_classes;
    std::vector<float> corners((size_t)m * 4);
    for (int i = 0; i < m; ++i) {
        const float v = means[i * 4], u = means[i * 4 + 1], hh = means[i * 4 + 2], ww = means[i * 4 + 3];
        corners[i * 4] = v - hh / 2.0f; corners[i * 4 + 1] = u - ww / 2.0f;
        corners[i * 4 + 2] = v + hh / 2.0f; corners[i * 4 + 3] = u + ww / 2.0f;
    }
    if (m > 0) {
        HIPCHK(h, hipMemcpyAsync(h->pb.counts + o * C, counts, m * C * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->pb.means + o * 4, means, (size_t)m * 16, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->pb.covs + o * 16, covs, (size_t)m * 64, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->pb.ranking + o, ranking, (size_t)m * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->pb.corners + o * 4, corners.data(), (size_t)m * 16, hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(h, hipMemcpyAsync(h->pb.num_kept + img, &m, 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->stage.posterior_ran();
    if (h->parts) h->parts_ok[img] = 0;               // the rows' parts are the previous posterior's until bod_set_posterior_parts
    if (h->cparts) h->cparts_ok[img] = 0;             // ... until bod_set_posterior_class_parts
    return BOD_OK;
}

static bod_status parts_handle(bod_handle h, const char* who) {
    if (!h) return BOD_ERR_INVALID_ARG;
    if (!h->parts) return h->fail(BOD_ERR_INVALID_ARG, "%s: the handle was created without bod_config.covariance_parts", who);
    return BOD_OK;
}

// lower triangle rows [m][30] (kernels.h) <-> the ABI's [m][3][16]
static void parts_expand(const float* tri, size_t m, float* full) {
    for (size_t i = 0; i < m * 3; ++i) {
        int t = 0;
        for (int r = 0; r < 4; ++r)
            for (int q = 0; q <= r; ++q) { full[i * 16 + r * 4 + q] = full[i * 16 + q * 4 + r] = tri[i * 10 + t]; ++t; }
    }
}

bod_status bod_get_posterior_parts(bod_handle h, int32_t img, float* parts) {
    BODCHK(parts_handle(h, "bod_get_posterior_parts"));
    BODCHK(join_overlap(h));
    if (!h->stage.posterior) return h->fail(BOD_ERR_NOT_READY, "bod_posterior has not run");
    int32_t m = 0;
    BODCHK(image_m(h, img, &m));
    if (!h->parts_ok[img]) return h->fail(BOD_ERR_NOT_READY, "bod_get_posterior_parts: image %d was injected with bod_set_posterior; bod_set_posterior_parts has not followed", img);
    if (!parts || m == 0) return BOD_OK;
    std::vector<float> tri((size_t)m * BOD_PARTS_TRI);
    BODCHK(d2h(h, tri.data(), h->parts + (size_t)img * h->A * BOD_PARTS_TRI, tri.size()));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    parts_expand(tri.data(), (size_t)m, parts);
    return BOD_OK;
}

bod_status bod_set_posterior_parts(bod_handle h, int32_t img, int32_t m, const float* parts) {
    BODCHK(parts_handle(h, "bod_set_posterior_parts"));
    BODCHK(join_overlap(h));
    if (!h->stage.posterior) return h->fail(BOD_ERR_NOT_READY, "bod_posterior / bod_set_posterior has not run");
    int32_t mm = 0;
    BODCHK(image_m(h, img, &mm));
    if (m != mm || (m > 0 && !parts)) return h->fail(BOD_ERR_INVALID_ARG, "bod_set_posterior_parts: got %d rows, image %d has %d", m, img, mm);
    std::vector<float> tri((size_t)m * BOD_PARTS_TRI);
    for (size_t i = 0; i < (size_t)m * 3; ++i) {
        int t = 0;
        for (int r = 0; r < 4; ++r)
            for (int q = 0; q <= r; ++q) tri[i * 10 + t++] = parts[i * 16 + r * 4 + q];
    }
    if (m > 0) HIPCHK(h, hipMemcpyAsync(h->parts + (size_t)img * h->A * BOD_PARTS_TRI, tri.data(), tri.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->parts_ok[img] = 1; h->stage.parts_set();
    return BOD_OK;
}

bod_status bod_nms(bod_handle h) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    if (!h->stage.posterior) return h->fail(BOD_ERR_NOT_READY, "bod_posterior has not run");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return run_nms(h, h->stream);
}

bod_status bod_get_nms(bod_handle h, int32_t img, int32_t* indices, int32_t* num) {
    if (!h || !num) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    if (!h->stage.nms) return h->fail(BOD_ERR_NOT_READY, "bod_nms has not run");
    if (img < 0 || img >= h->cfg.batch) return h->fail(BOD_ERR_INVALID_ARG, "image index out of range");
    BODCHK(slot_count(h, img, num));
    BODCHK(d2h(h, indices, h->cur().nms_sel + (size_t)img * h->cfg.nms_max_output_size, (size_t)*num));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BOD_OK;
}

bod_status bod_set_nms(bod_handle h, int32_t img, const int32_t* indices, int32_t n) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    if (!h->stage.posterior) return h->fail(BOD_ERR_NOT_READY, "bod_posterior / bod_set_posterior has not run");
    if (img < 0 || img >= h->cfg.batch || n < 0 || n > h->cfg.nms_max_output_size || (n > 0 && !indices))
        return h->fail(BOD_ERR_INVALID_ARG, "bod_set_nms: bad image index or count (max %d)", h->cfg.nms_max_output_size);
    int32_t m = 0;
    BODCHK(image_m(h, img, &m));
    for (int i = 0; i < n; ++i)
        if (indices[i] < 0 || indices[i] >= m) return h->fail(BOD_ERR_INVALID_ARG, "cluster centre %d out of range [0,%d)", indices[i], m);
    if (n > 0)
        HIPCHK(h, hipMemcpyAsync(h->cur().nms_sel + (size_t)img * h->cfg.nms_max_output_size, indices, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->cur().nms_nsel + img, &n, 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->stage.nms_ran();
    return BOD_OK;
}

bod_status bod_get_iou_matrix(bod_handle h, int32_t img, float* iou) {
    if (!h || !iou) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    if (!h->stage.posterior) return h->fail(BOD_ERR_NOT_READY, "bod_posterior has not run");
    int32_t m = 0;
    BODCHK(image_m(h, img, &m));
    if (m == 0) return BOD_OK;
    const int64_t need = (int64_t)m * m;
    if (need > h->iou_cap) {
        if (h->iou_scratch) hipFree(h->iou_scratch);
        h->iou_scratch = nullptr; h->iou_cap = 0;
        if (hipMalloc((void**)&h->iou_scratch, (size_t)need * 4) != hipSuccess)
            return h->fail(BOD_ERR_OOM, "cannot allocate %lld-element IoU matrix", (long long)need);
        h->iou_cap = need;
    }
    HIPCHK(h, launch_iou_matrix(h->pb.corners + (size_t)img * h->A * 4, m, h->iou_scratch, h->stream));
    BODCHK(d2h(h, iou, h->iou_scratch, (size_t)need));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BOD_OK;
}

bod_status bod_set_affinity(bod_handle h, int32_t img, const float* centre_columns, int32_t k, int32_t m) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    if (!h->stage.nms) return h->fail(BOD_ERR_NOT_READY, "bod_nms / bod_set_nms has not run");
    if (img < 0 || img >= h->cfg.batch || !centre_columns) return h->fail(BOD_ERR_INVALID_ARG, "bod_set_affinity: bad image index / NULL");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int32_t mm = 0, kk = 0;
    BODCHK(image_m(h, img, &mm));
    BODCHK(slot_count(h, img, &kk));
    if (m != mm || k != kk)
        return h->fail(BOD_ERR_INVALID_ARG, "bod_set_affinity: got %d columns of %d rows, the image has %d centres and %d boxes", k, m, kk, mm);
    if (!h->affinity && hipMalloc((void**)&h->affinity, (size_t)h->cfg.nms_max_output_size * h->A * 4) != hipSuccess)
        return h->fail(BOD_ERR_OOM, "bod_set_affinity: %zu bytes", (size_t)h->cfg.nms_max_output_size * h->A * 4);
    for (int r = 0; r < k && m > 0; ++r)          // row r -> affinity[r][0..m): one plain copy per centre (k <= max_detections)
        HIPCHK(h, hipMemcpyAsync(h->affinity + (size_t)r * h->A, centre_columns + (size_t)r * m, (size_t)m * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->stage.affinity_set(img);
    return BOD_OK;
}

bod_status bod_cluster_fuse(bod_handle h) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    if (!h->stage.nms) return h->fail(BOD_ERR_NOT_READY, "bod_nms has not run");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return run_cluster(h, h->stream);
}

bod_status bod_get_detections(bod_handle h, int32_t img, int32_t* num, float* scores, float* means, float* covs, float* counts) {
    if (!h || !num) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    if (!h->stage.cluster) return h->fail(BOD_ERR_NOT_READY, "bod_cluster_fuse has not run");
    if (img < 0 || img >= h->cfg.batch) return h->fail(BOD_ERR_INVALID_ARG, "image index out of range");
    BODCHK(slot_count(h, img, num));
    const size_t k = (size_t)*num, o = (size_t)img * h->cfg.nms_max_output_size, C = h->cfg.num_classes;
    const RecordSlot& r = h->cur();
    BODCHK(d2h(h, scores, r.scores + o * C, k * C));
    BODCHK(d2h(h, means, r.means + o * REC_MEAN, k * REC_MEAN));
    BODCHK(d2h(h, covs, r.covs + o * REC_COV, k * REC_COV));
    BODCHK(d2h(h, counts, r.counts + o * C, k * C));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BOD_OK;
}

bod_status bod_get_detections_batch(bod_handle h, int32_t* num, float* scores, float* means, float* covs, float* counts) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    if (!h->stage.cluster) return h->fail(BOD_ERR_NOT_READY, "bod_cluster_fuse has not run");
    const size_t BK = (size_t)h->cfg.batch * h->cfg.nms_max_output_size, C = h->cfg.num_classes;
    const RecordSlot& r = h->cur();
    BODCHK(d2h(h, num, r.nms_nsel, (size_t)h->cfg.batch));
    BODCHK(d2h(h, scores, r.scores, BK * C));
    BODCHK(d2h(h, means, r.means, BK * REC_MEAN));
    BODCHK(d2h(h, covs, r.covs, BK * REC_COV));
    BODCHK(d2h(h, counts, r.counts, BK * C));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BOD_OK;
}

bod_status bod_get_detection_parts(bod_handle h, int32_t img, float* parts) {
    BODCHK(parts_handle(h, "bod_get_detection_parts"));
    BODCHK(join_overlap(h));
    if (!h->stage.cluster) return h->fail(BOD_ERR_NOT_READY, "bod_cluster_fuse has not run");
    if (img < 0 || img >= h->cfg.batch) return h->fail(BOD_ERR_INVALID_ARG, "image index out of range");
    if (!h->cur().parts_ok[img]) return h->fail(BOD_ERR_NOT_READY, "bod_get_detection_parts: image %d was fused without its posterior's parts (bod_set_posterior_parts)", img);
    int32_t num = 0;
    BODCHK(slot_count(h, img, &num));
    BODCHK(d2h(h, parts, h->cur().parts + (size_t)img * h->cfg.nms_max_output_size * REC_PARTS, (size_t)num * REC_PARTS));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BOD_OK;
}

bod_status bod_get_detection_parts_batch(bod_handle h, float* parts) {
    BODCHK(parts_handle(h, "bod_get_detection_parts_batch"));
    BODCHK(join_overlap(h));
    if (!h->stage.cluster) return h->fail(BOD_ERR_NOT_READY, "bod_cluster_fuse has not run");
    for (int img = 0; img < h->cfg.batch; ++img)
        if (!h->cur().parts_ok[img]) return h->fail(BOD_ERR_NOT_READY, "bod_get_detection_parts_batch: image %d was fused without its posterior's parts (bod_set_posterior_parts)", img);
    BODCHK(d2h(h, parts, h->cur().parts, (size_t)h->cfg.batch * h->cfg.nms_max_output_size * REC_PARTS));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BOD_OK;
}

bod_status bod_device_detection_parts(bod_handle h, int32_t sidx, void** p) {
    BODCHK(parts_handle(h, "bod_device_detection_parts"));
    if (!p || sidx < 0 || sidx > 1) return h->fail(BOD_ERR_INVALID_ARG, "bod_device_detection_parts: slot %d / NULL", sidx);
    *p = h->rec[sidx].parts;
    return BOD_OK;
}

static bod_status class_parts_handle(bod_handle h, const char* who) {
    if (!h) return BOD_ERR_INVALID_ARG;
    if (!h->class_parts) return h->fail(BOD_ERR_INVALID_ARG, "%s: the handle was created without BOD_PARTS_CLASS in bod_config.covariance_parts", who);
    return BOD_OK;
}

bod_status bod_get_posterior_class_parts(bod_handle h, int32_t img, float* rows) {
    BODCHK(class_parts_handle(h, "bod_get_posterior_class_parts"));
    BODCHK(join_overlap(h));
    if (!h->stage.posterior) return h->fail(BOD_ERR_NOT_READY, "bod_posterior has not run");
    int32_t m = 0;
    BODCHK(image_m(h, img, &m));
    if (!h->cparts_ok[img]) return h->fail(BOD_ERR_NOT_READY, "bod_get_posterior_class_parts: image %d was injected with bod_set_posterior; bod_set_posterior_class_parts has not followed", img);
    if (!rows || m == 0) return BOD_OK;
    const size_t Q = 3 + (size_t)h->cfg.num_classes;
    std::vector<float> tmp((size_t)m * Q);
    BODCHK(d2h(h, tmp.data(), h->cparts + (size_t)img * h->A * Q, tmp.size()));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < (size_t)m; ++i)
        for (int q = 0; q < 3; ++q) rows[i * 3 + q] = tmp[i * Q + q];
    return BOD_OK;
}

bod_status bod_get_posterior_mean_probs(bod_handle h, int32_t img, float* mean_probs) {
    BODCHK(class_parts_handle(h, "bod_get_posterior_mean_probs"));
    BODCHK(join_overlap(h));
    if (!h->stage.posterior) return h->fail(BOD_ERR_NOT_READY, "bod_posterior has not run");
    int32_t m = 0;
    BODCHK(image_m(h, img, &m));
    if (!h->cparts_ok[img]) return h->fail(BOD_ERR_NOT_READY, "bod_get_posterior_mean_probs: image %d was injected with bod_set_posterior; bod_set_posterior_class_parts has not followed", img);
    if (!mean_probs || m == 0) return BOD_OK;
    const size_t C = (size_t)h->cfg.num_classes, Q = 3 + C;
    std::vector<float> tmp((size_t)m * Q);
    BODCHK(d2h(h, tmp.data(), h->cparts + (size_t)img * h->A * Q, tmp.size()));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < (size_t)m; ++i)
        for (size_t j = 0; j < C; ++j) mean_probs[i * C + j] = tmp[i * Q + 3 + j];
    return BOD_OK;
}

bod_status bod_set_posterior_class_parts(bod_handle h, int32_t img, int32_t m, const float* mean_probs, const float* rows) {
    BODCHK(class_parts_handle(h, "bod_set_posterior_class_parts"));
    BODCHK(join_overlap(h));
    if (!h->stage.posterior) return h->fail(BOD_ERR_NOT_READY, "bod_posterior / bod_set_posterior has not run");
    int32_t mm = 0;
    BODCHK(image_m(h, img, &mm));
    if (m != mm || (m > 0 && (!mean_probs || !rows))) return h->fail(BOD_ERR_INVALID_ARG, "bod_set_posterior_class_parts: got %d rows, image %d has %d", m, img, mm);
    const size_t C = (size_t)h->cfg.num_classes, Q = 3 + C;
    std::vector<float> tmp((size_t)m * Q);
    for (size_t i = 0; i < (size_t)m; ++i) {
        for (int q = 0; q < 3; ++q) tmp[i * Q + q] = rows[i * 3 + q];
        for (size_t j = 0; j < C; ++j) tmp[i * Q + 3 + j] = mean_probs[i * C + j];
    }
    if (m > 0) HIPCHK(h, hipMemcpyAsync(h->cparts + (size_t)img * h->A * Q, tmp.data(), tmp.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->cparts_ok[img] = 1; h->stage.parts_set();
    return BOD_OK;
}

bod_status bod_get_detection_class_parts(bod_handle h, int32_t img, float* rows) {
    BODCHK(class_parts_handle(h, "bod_get_detection_class_parts"));
    BODCHK(join_overlap(h));
    if (!h->stage.cluster) return h->fail(BOD_ERR_NOT_READY, "bod_cluster_fuse has not run");
    if (img < 0 || img >= h->cfg.batch) return h->fail(BOD_ERR_INVALID_ARG, "image index out of range");
    if (!h->cur().cparts_ok[img]) return h->fail(BOD_ERR_NOT_READY, "bod_get_detection_class_parts: image %d was fused without its posterior's class parts (bod_set_posterior_class_parts)", img);
    int32_t num = 0;
    BODCHK(slot_count(h, img, &num));
    BODCHK(d2h(h, rows, h->cur().cparts + (size_t)img * h->cfg.nms_max_output_size * REC_CPARTS, (size_t)num * REC_CPARTS));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BOD_OK;
}

bod_status bod_get_detection_class_parts_batch(bod_handle h, float* rows) {
    BODCHK(class_parts_handle(h, "bod_get_detection_class_parts_batch"));
    BODCHK(join_overlap(h));
    if (!h->stage.cluster) return h->fail(BOD_ERR_NOT_READY, "bod_cluster_fuse has not run");
    for (int img = 0; img < h->cfg.batch; ++img)
        if (!h->cur().cparts_ok[img]) return h->fail(BOD_ERR_NOT_READY, "bod_get_detection_class_parts_batch: image %d was fused without its posterior's class parts (bod_set_posterior_class_parts)", img);
    // rows beyond an image's count are whatever an earlier batch left: zero them on the way out, like the record rows
    const size_t B = (size_t)h->cfg.batch, K = (size_t)h->cfg.nms_max_output_size;
    std::vector<int32_t> num(B);
    HIPCHK(h, hipMemcpyAsync(num.data(), h->cur().nms_nsel, B * 4, hipMemcpyDeviceToHost, h->stream));
    BODCHK(d2h(h, rows, h->cur().cparts, B * K * REC_CPARTS));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    zero_rows_past_count(rows, num.data(), B, K, REC_CPARTS);
    return BOD_OK;
}

bod_status bod_device_detection_class_parts(bod_handle h, int32_t sidx, void** p) {
    BODCHK(class_parts_handle(h, "bod_device_detection_class_parts"));
    if (!p || sidx < 0 || sidx > 1) return h->fail(BOD_ERR_INVALID_ARG, "bod_device_detection_class_parts: slot %d / NULL", sidx);
    *p = h->rec[sidx].cparts;
    return BOD_OK;
}

bod_status bod_set_merge_method(bod_handle h, int32_t method) {
    if (!h) return BOD_ERR_INVALID_ARG;
    if (method != BOD_MERGE_BAYES && method != BOD_MERGE_CENTRE && method != BOD_MERGE_MIXTURE)
        return h->fail(BOD_ERR_INVALID_ARG, "bod_set_merge_method: unknown method %d (BOD_MERGE_BAYES = 0, BOD_MERGE_CENTRE = 1, BOD_MERGE_MIXTURE = 2)", method);
    if (h->cfg.training) return h->fail(BOD_ERR_INVALID_ARG, "bod_set_merge_method: a training handle has no cluster stage");
    if (method != BOD_MERGE_BAYES && h->cfg.covariance_parts != 0)
        return h->fail(BOD_ERR_INVALID_ARG, "bod_set_merge_method: the handle was created with bod_config.covariance_parts = %d; the covariance and "
                       "class-entropy parts are defined for the Bayesian fuse (BOD_MERGE_BAYES) only", h->cfg.covariance_parts);
    if (method != BOD_MERGE_BAYES && h->uncertainty_method == BOD_METHOD_BLACK_BOX)
        return h->fail(BOD_ERR_INVALID_ARG, "bod_set_merge_method: the handle's uncertainty method is BOD_METHOD_BLACK_BOX, which merges the pooled "
                       "sample detections by its own rule; the merge methods belong to BOD_METHOD_BAYES_OD");
    if (method != BOD_MERGE_BAYES && !h->rec[1].merge_members) {
        HIPCHK(h, hipSetDevice(h->cfg.device));
        const size_t BK = (size_t)h->cfg.batch * h->cfg.nms_max_output_size;
        for (RecordSlot& r : h->rec) {
            BODCHK(h->dalloc(&r.merge_within, BK * REC_COV));
            BODCHK(h->dalloc(&r.merge_between, BK * REC_COV));
            BODCHK(h->dalloc(&r.merge_members, BK));
        }
    }
    h->merge_method = method;
    return BOD_OK;
}

bod_status bod_get_merge_method(bod_handle h, int32_t* method) {
    if (!h || !method) return BOD_ERR_INVALID_ARG;
    *method = h->merge_method;
    return BOD_OK;
}

bod_status bod_get_detection_merge_terms(bod_handle h, int32_t img, float* within, float* between, int32_t* members) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    if (!h->stage.cluster) return h->fail(BOD_ERR_NOT_READY, "bod_cluster_fuse has not run");
    if (img < 0 || img >= h->cfg.batch) return h->fail(BOD_ERR_INVALID_ARG, "image index out of range");
    if (!h->cur().merge_terms_ok) return h->fail(BOD_ERR_NOT_READY, "bod_get_detection_merge_terms: the last cluster stage ran as BOD_MERGE_BAYES, which has no merge terms");
    int32_t num = 0;
    BODCHK(slot_count(h, img, &num));
    const size_t k = (size_t)std::max(num, 0), o = (size_t)img * h->cfg.nms_max_output_size;
    BODCHK(d2h(h, within, h->cur().merge_within + o * REC_COV, k * REC_COV));
    BODCHK(d2h(h, between, h->cur().merge_between + o * REC_COV, k * REC_COV));
    BODCHK(d2h(h, members, h->cur().merge_members + o, k));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BOD_OK;
}

bod_status bod_get_detection_merge_terms_batch(bod_handle h, int32_t slot, float* within, float* between, int32_t* members) {
    if (!h) return BOD_ERR_INVALID_ARG;
    if (slot < -1 || slot > 1) return h->fail(BOD_ERR_INVALID_ARG, "bod_get_detection_merge_terms_batch: slot %d", slot);
    const size_t B = (size_t)h->cfg.batch, K = (size_t)h->cfg.nms_max_output_size;
    std::vector<int32_t> num(B);
    if (slot < 0) {
        BODCHK(join_overlap(h));
        if (!h->stage.cluster) return h->fail(BOD_ERR_NOT_READY, "bod_cluster_fuse has not run");
        const RecordSlot& r = h->cur();
        if (!r.merge_terms_ok) return h->fail(BOD_ERR_NOT_READY, "bod_get_detection_merge_terms_batch: the last cluster stage ran as BOD_MERGE_BAYES, which has no merge terms");
        HIPCHK(h, hipMemcpyAsync(num.data(), r.nms_nsel, B * 4, hipMemcpyDeviceToHost, h->stream));
        BODCHK(d2h(h, within, r.merge_within, B * K * REC_COV));
        BODCHK(d2h(h, between, r.merge_between, B * K * REC_COV));
        BODCHK(d2h(h, members, r.merge_members, B * K));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    } else {
        // a bod_infer_async ticket: wait for that batch as bod_collect does (its event, not a stream the next batch may be queued on),
        // then plain blocking copies -- the pinned staging of the records is sized at create and stays as it is
        const RecordSlot& r = h->rec[slot];
        if (!r.done_stream) return h->fail(BOD_ERR_NOT_READY, "bod_get_detection_merge_terms_batch: slot %d holds no batch of bod_infer_async", slot);
        if (!r.merge_terms_ok) return h->fail(BOD_ERR_NOT_READY, "bod_get_detection_merge_terms_batch: slot %d's cluster stage ran as BOD_MERGE_BAYES, which has no merge terms", slot);
        HIPCHK(h, hipSetDevice(h->cfg.device));
        HIPCHK(h, hipEventSynchronize(r.done));
        HIPCHK(h, hipMemcpy(num.data(), r.nms_nsel, B * 4, hipMemcpyDeviceToHost));
        if (within) HIPCHK(h, hipMemcpy(within, r.merge_within, B * K * REC_COV * 4, hipMemcpyDeviceToHost));
        if (between) HIPCHK(h, hipMemcpy(between, r.merge_between, B * K * REC_COV * 4, hipMemcpyDeviceToHost));
        if (members) HIPCHK(h, hipMemcpy(members, r.merge_members, B * K * 4, hipMemcpyDeviceToHost));
    }
    // rows beyond an image's count are whatever an earlier batch left: zero them on the way out, like the record rows
    zero_rows_past_count(within, num.data(), B, K, REC_COV);
    zero_rows_past_count(between, num.data(), B, K, REC_COV);
    zero_rows_past_count(members, num.data(), B, K, 1);
    return BOD_OK;
}

bod_status bod_device_detection_merge_terms(bod_handle h, int32_t sidx, void** p) {
    if (!h) return BOD_ERR_INVALID_ARG;
    if (!p || sidx < 0 || sidx > 1) return h->fail(BOD_ERR_INVALID_ARG, "bod_device_detection_merge_terms: slot %d / NULL", sidx);
    const RecordSlot& r = h->rec[sidx];
    p[0] = r.merge_within; p[1] = r.merge_between; p[2] = r.merge_members;
    return BOD_OK;
}

bod_status bod_set_uncertainty_method(bod_handle h, int32_t method, const bod_blackbox_options* options) {
    if (!h) return BOD_ERR_INVALID_ARG;
    if (method != BOD_METHOD_BAYES_OD && method != BOD_METHOD_BLACK_BOX)
        return h->fail(BOD_ERR_INVALID_ARG, "bod_set_uncertainty_method: unknown method %d (BOD_METHOD_BAYES_OD = 0, BOD_METHOD_BLACK_BOX = 1)", method);
    if (h->cfg.training) return h->fail(BOD_ERR_INVALID_ARG, "bod_set_uncertainty_method: a training handle has no detection stages");
    if (method == BOD_METHOD_BLACK_BOX) {
        if (h->cfg.mc_statistics)
            return h->fail(BOD_ERR_INVALID_ARG, "bod_set_uncertainty_method: a statistics handle (bod_config.mc_statistics = 1) holds merged per-anchor "
                           "statistics, not the samples' own head outputs that black-box MC dropout post-processes one by one");
        if (h->cfg.covariance_parts != 0)
            return h->fail(BOD_ERR_INVALID_ARG, "bod_set_uncertainty_method: the handle was created with bod_config.covariance_parts = %d; the covariance and "
                           "class-entropy parts are defined for BOD_METHOD_BAYES_OD only", h->cfg.covariance_parts);
        if (h->merge_method != BOD_MERGE_BAYES)
            return h->fail(BOD_ERR_INVALID_ARG, "bod_set_uncertainty_method: the handle's merge method is %d; black-box MC dropout merges by its own rule: "
                           "set BOD_MERGE_BAYES first", h->merge_method);
        const bod_blackbox_options o = options ? *options : bod_blackbox_options{0.f, 1, 0.f, 0};
        if (o.min_members < 1) return h->fail(BOD_ERR_INVALID_ARG, "bod_set_uncertainty_method: min_members %d must be >= 1", o.min_members);
        if (!std::isfinite(o.min_score) || o.min_score < 0.f || !std::isfinite(o.affinity_threshold) || o.affinity_threshold < 0.f)
            return h->fail(BOD_ERR_INVALID_ARG, "bod_set_uncertainty_method: min_score %g and affinity_threshold %g must be finite and >= 0",
                           (double)o.min_score, (double)o.affinity_threshold);
        if (o.reserved != 0) return h->fail(BOD_ERR_INVALID_ARG, "bod_set_uncertainty_method: reserved must be 0");
        BODCHK(join_overlap(h));
        HIPCHK(h, hipSetDevice(h->cfg.device));
        BODCHK(alloc_blackbox(h));
        h->bb_opt = o;
    }
    h->uncertainty_method = method;
    return BOD_OK;
}

bod_status bod_get_uncertainty_method(bod_handle h, int32_t* method) {
    if (!h || !method) return BOD_ERR_INVALID_ARG;
    *method = h->uncertainty_method;
    return BOD_OK;
}

bod_status bod_blackbox_samples(bod_handle h) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    if (!h->bb.keep) return h->fail(BOD_ERR_NOT_READY, "bod_blackbox_samples: bod_set_uncertainty_method(BOD_METHOD_BLACK_BOX) has not been called");
    if (!h->stage.forward) return h->fail(BOD_ERR_NOT_READY, "bod_forward / bod_set_raw has not run");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return run_blackbox_samples(h);
}

bod_status bod_blackbox_merge(bod_handle h) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    if (!h->bb.keep) return h->fail(BOD_ERR_NOT_READY, "bod_blackbox_merge: bod_set_uncertainty_method(BOD_METHOD_BLACK_BOX) has not been called");
    if (!h->bb_samples_ok) return h->fail(BOD_ERR_NOT_READY, "bod_blackbox_samples / bod_set_sample_detections has not run");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    BODCHK(wait_pending_slots(h, h->stream));
    return run_blackbox_merge(h, h->stream);
}

static bod_status sample_index_ok(bod_handle h, const char* who, int32_t img, int32_t sample) {
    if (!h->bb.keep) return h->fail(BOD_ERR_NOT_READY, "%s: bod_set_uncertainty_method(BOD_METHOD_BLACK_BOX) has not been called", who);
    if (img < 0 || img >= h->cfg.batch || sample < 0 || sample >= h->cfg.mc_samples)
        return h->fail(BOD_ERR_INVALID_ARG, "%s: image %d / sample %d out of range", who, img, sample);
    return BOD_OK;
}

bod_status bod_get_sample_detections(bod_handle h, int32_t img, int32_t sample, int32_t* count, int32_t* anchor_index, float* scores,
                                     float* means, float* covs) {
    if (!h || !count) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    BODCHK(sample_index_ok(h, "bod_get_sample_detections", img, sample));
    if (!h->bb_samples_ok) return h->fail(BOD_ERR_NOT_READY, "bod_blackbox_samples / bod_set_sample_detections has not run");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t v = (size_t)img * h->cfg.mc_samples + sample, K = (size_t)h->cfg.nms_max_output_size, C = h->cfg.num_classes;
    HIPCHK(h, hipMemcpyAsync(count, h->bb.sd_count + v, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const size_t k = (size_t)std::min<int64_t>(std::max<int64_t>(*count, 0), (int64_t)K);
    BODCHK(d2h(h, anchor_index, h->bb.sd_anchor + v * K, k));
    BODCHK(d2h(h, scores, h->bb.sd_score + v * K * C, k * C));
    BODCHK(d2h(h, means, h->bb.sd_mean + v * K * 4, k * 4));
    BODCHK(d2h(h, covs, h->bb.sd_cov + v * K * 16, k * 16));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BOD_OK;
}

bod_status bod_set_sample_detections(bod_handle h, int32_t img, int32_t sample, int32_t count, const int32_t* anchor_index,
                                     const float* scores, const float* means, const float* covs) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    BODCHK(sample_index_ok(h, "bod_set_sample_detections", img, sample));
    if (count < 0 || count > h->cfg.nms_max_output_size)
        return h->fail(BOD_ERR_INVALID_ARG, "bod_set_sample_detections: count %d outside 0..nms_max_output_size = %d", count, h->cfg.nms_max_output_size);
    if (count > 0 && (!scores || !means || !covs)) return h->fail(BOD_ERR_INVALID_ARG, "bod_set_sample_detections: scores, means and covs are needed");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    BODCHK(wait_pending_slots(h, h->stream));
    const size_t v = (size_t)img * h->cfg.mc_samples + sample, K = (size_t)h->cfg.nms_max_output_size, C = h->cfg.num_classes, k = (size_t)count;
    if (k) {
        if (anchor_index) HIPCHK(h, hipMemcpyAsync(h->bb.sd_anchor + v * K, anchor_index, k * 4, hipMemcpyHostToDevice, h->stream));
        else HIPCHK(h, hipMemsetAsync(h->bb.sd_anchor + v * K, 0, k * 4, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->bb.sd_score + v * K * C, scores, k * C * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->bb.sd_mean + v * K * 4, means, k * 16, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->bb.sd_cov + v * K * 16, covs, k * 64, hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(h, hipMemcpyAsync(h->bb.sd_count + v, &count, sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->bb_samples_ok = true;
    return BOD_OK;
}

bod_status bod_device_raw(bod_handle h, void** p, int32_t mark_ready) {
    if (!h || !p) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (mark_ready) BODCHK(ensure_raw(h)); else BODCHK(materialise_raw(h));
    p[0] = h->raw[0]; p[1] = h->raw[1]; p[2] = h->cfg.has_covar_head ? h->raw[2] : nullptr;
    if (mark_ready) { h->kscale_now = nullptr; h->stage.forward_ran(); h->raw_valid = true; h->agg_valid = false; h->bb_samples_ok = false; }
    return BOD_OK;
}

bod_status bod_device_detections(bod_handle h, int32_t sidx, void** p) {
    if (!h || !p || sidx < 0 || sidx > 1) return BOD_ERR_INVALID_ARG;
    const RecordSlot& r = h->rec[sidx];
    p[0] = r.nms_nsel; p[1] = r.scores; p[2] = r.means; p[3] = r.covs; p[4] = r.counts;
    return BOD_OK;
}

bod_status bod_infer(bod_handle h, const float* images, int32_t on_device, uint64_t seed, uint32_t first_image_id) {
    MarkerRange mr_api("bod:infer");
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    if (!h->weights_ready) return h->fail(BOD_ERR_NOT_READY, "weights not finalized");
    const bool black_box = h->uncertainty_method == BOD_METHOD_BLACK_BOX;
    if (!black_box && h->cfg.mc_samples < 2) return h->fail(BOD_ERR_INVALID_ARG, "bayes_od needs mc_samples >= 2 (sample covariance divides by N-1)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const float* dev = nullptr;
    BODCHK(stage_images(h, images, on_device, &dev));
    h->cur_images = dev;
    if (black_box) {                                  // per-sample head outputs, per-sample NMS, then the pooled detections merged
        BODCHK(run_forward(h, dev, seed, first_image_id, FLAVOUR_RAW));
        BODCHK(run_blackbox_samples(h));
        return run_blackbox_merge(h, h->stream);
    }
    BODCHK(run_forward(h, dev, seed, first_image_id, infer_flavour(h)));
    BODCHK(run_posterior(h, seed, first_image_id));
    BODCHK(run_nms(h, h->stream));
    return run_cluster(h, h->stream);
}

bod_status bod_infer_async(bod_handle h, const float* images, int32_t on_device, uint64_t seed, uint32_t first_image_id, int32_t* slot_out) {
    MarkerRange mr_api("bod:infer_async");
    if (!h || !slot_out) return BOD_ERR_INVALID_ARG;
    if (!h->weights_ready) return h->fail(BOD_ERR_NOT_READY, "weights not finalized");
    const bool black_box = h->uncertainty_method == BOD_METHOD_BLACK_BOX;
    if (!black_box && h->cfg.mc_samples < 2) return h->fail(BOD_ERR_INVALID_ARG, "bayes_od needs mc_samples >= 2 (sample covariance divides by N-1)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int sidx = h->slot ^ 1;
    RecordSlot& r = h->rec[sidx];
    if (r.pending)
        return h->fail(BOD_ERR_NOT_READY, "slot %d still holds uncollected detections: call bod_collect first", sidx);
    // pipeline_overlap handles: this call's front goes to h->front, everything else to h->back (h->stream for the call's duration);
    // both are first ordered behind whatever the full-chip stream still holds (an upload, a synchronous call's tail)
    const bool ov = h->overlap_mode != 0;
    struct MainStream { bod_context* h; ~MainStream() { h->stream = h->full; h->in_overlap_call = false; } } restore_main{h};
    if (ov) {
        HIPCHK(h, hipEventRecord(h->ev_join, h->full));
        HIPCHK(h, hipStreamWaitEvent(h->front, h->ev_join, 0));
        HIPCHK(h, hipStreamWaitEvent(h->back, h->ev_join, 0));
        h->stream = h->back; h->in_overlap_call = true; h->ov_dirty = true;
    }
    const float* dev = nullptr;
    BODCHK(stage_images(h, images, on_device, &dev, ov ? h->front : h->stream));
    h->cur_images = dev;
    BODCHK(run_forward(h, dev, seed, first_image_id, black_box ? FLAVOUR_RAW : infer_flavour(h), false, ov));
    if (black_box) BODCHK(run_blackbox_samples(h));
    else BODCHK(run_posterior(h, seed, first_image_id));      // waits for the side stream's previous readers
    HIPCHK(h, hipEventRecord(h->ev_posterior, h->stream));
    h->slot = sidx;
    // Round 5: soft-NMS + cluster-and-fuse (and the copies of the records) run on the MAIN stream, behind the posterior, not on the side
    // stream beside the next call's stem.  With them on the side stream a call's detections were not reproducible: one detection in ~60
    // frames with its fused mean moved by up to 0.4 px (same counts and scores: one cluster member more or less) -- in 3-14 of 12 runs of
    // tests/tools/overlap_race.py on overlap handles (64 frames, two calls in flight), and in 5 of 12 fresh processes whose FIRST work is a
    // pipelined pair on a serial handle (tests/tools/pipelined_vs_sync.py, 128 x 128 x 128 frames); with them on the main stream: 0 of 12
    // and 0 of 12.  The mechanism is not found (every buffer the two streams share is ordered by events; tests/tools/side_race.py: the
    // posterior re-run on unchanged inputs differs while ANOTHER handle keeps the GPU busy, never alone; no LDS overrun:
    // tests/tools/lds_canary.py) -- so the contract ("pipelined == synchronous, bit for bit") is kept by not overlapping them.  Cost:
    // the side work no longer hides under the next stem, where it collided for 2.4 ms per 512-frame step anyway (History A.1):
    // measured below.  BOD_SIDE_STREAM=1: the side stream again (A/B).
    static const bool side_on = [] { const char* e = getenv("BOD_SIDE_STREAM"); return e && atoi(e) != 0; }();
    hipStream_t sd = side_on ? h->side : h->stream;
    if (side_on) HIPCHK(h, hipStreamWaitEvent(h->side, h->ev_posterior, 0));
    if (black_box) {
        BODCHK(run_blackbox_merge(h, sd));
    } else {
        BODCHK(run_nms(h, sd));
        BODCHK(run_cluster(h, sd));
    }
    // The records follow the kernels on the side stream into pinned host memory, so bod_collect only waits for
    // this slot's event: it must never queue work behind the NEXT batch's side-stream kernels (that would
    // stall the host until the next batch has finished and drain the pipeline).
    void* const dev_arrays[RecordLayout::SEGS] = {r.nms_nsel, r.scores, r.means, r.covs, r.counts, r.parts, r.cparts};
    BODCHK(copy_staged(h, r, dev_arrays, true, sd));
    if (r.parts) r.parts_staged = true;
    if (r.cparts) r.cparts_staged = true;
    HIPCHK(h, hipEventRecord(r.done, sd));
    r.done_stream = sd;
    r.pending = true;
    *slot_out = sidx;
    return BOD_OK;
}

bod_status bod_collect(bod_handle h, int32_t sidx, int32_t* num, float* scores, float* means, float* covs, float* counts) {
    MarkerRange mr_api("bod:collect");
    if (!h) return BOD_ERR_INVALID_ARG;
    if (sidx < 0 || sidx > 1 || !h->rec[sidx].pending) return h->fail(BOD_ERR_NOT_READY, "slot %d has no pending batch", sidx);
    RecordSlot& r = h->rec[sidx];
    HIPCHK(h, hipEventSynchronize(r.done));
    void* const out[RecordLayout::SEGS] = {num, scores, means, covs, counts, nullptr, nullptr};
    BODCHK(copy_staged(h, r, out, false, nullptr));
    r.pending = false;
    return BOD_OK;
}

bod_status bod_collect_parts(bod_handle h, int32_t sidx, float* parts) {
    BODCHK(parts_handle(h, "bod_collect_parts"));
    if (sidx < 0 || sidx > 1 || !h->rec[sidx].parts_staged) return h->fail(BOD_ERR_NOT_READY, "bod_collect_parts: slot %d holds no batch of bod_infer_async", sidx);
    HIPCHK(h, hipEventSynchronize(h->rec[sidx].done));
    void* const out[RecordLayout::SEGS] = {nullptr, nullptr, nullptr, nullptr, nullptr, parts, nullptr};
    return copy_staged(h, h->rec[sidx], out, false, nullptr);
}

bod_status bod_collect_class_parts(bod_handle h, int32_t sidx, float* rows) {
    BODCHK(class_parts_handle(h, "bod_collect_class_parts"));
    if (sidx < 0 || sidx > 1 || !h->rec[sidx].cparts_staged) return h->fail(BOD_ERR_NOT_READY, "bod_collect_class_parts: slot %d holds no batch of bod_infer_async", sidx);
    const RecordSlot& r = h->rec[sidx];
    HIPCHK(h, hipEventSynchronize(r.done));
    void* const out[RecordLayout::SEGS] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, rows};
    BODCHK(copy_staged(h, r, out, false, nullptr));
    // rows beyond an image's count: zero (the counts lead the staging buffer)
    zero_rows_past_count(rows, reinterpret_cast<const int32_t*>(r.host_stage), (size_t)h->cfg.batch, (size_t)h->cfg.nms_max_output_size, REC_CPARTS);
    return BOD_OK;
}

bod_status bod_stage_conv(int32_t device, const float* x, int32_t B, int32_t H, int32_t W, int32_t Cin,
                          const float* w, const float* bias, int32_t KH, int32_t KW, int32_t Cout,
                          int32_t stride, int32_t same_padding, int32_t relu, const float* residual,
                          float dropout_rate, uint64_t seed, int32_t layer_id, uint32_t image_id,
                          int32_t round_output_bf16, int32_t precision, float* out) {
    StageScope sc;                        // scratch context: owns the temporary device buffers
    bod_context* h = sc.h;
    const int mxfmt = precision == BOD_PRECISION_F16MX ? 1 : precision == BOD_PRECISION_F16MX4 ? 2 : 0;
    const bool mxp = mxfmt != 0;                 // f16mx tower kernel; round_output_bf16 = data path under test (bayesod.h)
    const int mx_mode = mxp ? round_output_bf16 : 0;
    const bool f32 = precision == BOD_PRECISION_FP32, x3 = precision == BOD_PRECISION_BF16X3 || mxp;
    if (mxp) round_output_bf16 = 1;
    h->es = (f32 || x3) ? 4 : 2;
    h->split = x3; h->mx = mxfmt;
    if (!x || !w || !out || B < 1 || H < 1 || W < 1 || KH < 1 || KW < 1 || stride < 1 || stride > 2)
        return sc.done(h->fail(BOD_ERR_INVALID_ARG, "bod_stage_conv: bad argument"));
    if (precision != BOD_PRECISION_BF16 && !f32 && !x3) return sc.done(h->fail(BOD_ERR_INVALID_ARG, "bod_stage_conv: bad precision"));
    if (mxp && (KH != 3 || KW != 3 || stride != 1 || !same_padding || Cin != 256 || Cout != 256 || residual || mx_mode < 0 || mx_mode > 2))
        return sc.done(h->fail(BOD_ERR_INVALID_ARG, "bod_stage_conv: BOD_PRECISION_F16MX / F16MX4 run a head-tower layer (3x3, stride 1, SAME, 256 -> 256, no residual), round_output_bf16 in 0..2"));
    if (f32 && round_output_bf16) return sc.done(h->fail(BOD_ERR_INVALID_ARG, "bod_stage_conv: round_output_bf16 is meaningless in fp32 precision"));
    if (Cin % 64 != 0 || ((round_output_bf16 || (dropout_rate > 0.f && !f32)) && Cout % 4 != 0))
        return sc.done(h->fail(BOD_ERR_INVALID_ARG, "bod_stage_conv: Cin must be a multiple of 64 (and Cout of 4 for bf16 output); got %d, %d", Cin, Cout));
    if (KH > 3 || KW > 3) return sc.done(h->fail(BOD_ERR_INVALID_ARG, "bod_stage_conv: kernel larger than 3x3 needs a wider zero border"));
    if (const bod_status st = sc.open(device)) return sc.done(st);
    h->cfg.batch = B;
    int OH, OW, oy, ox;
    conv_out_geometry(H, W, KH, KW, stride, same_padding != 0, &OH, &OW, &oy, &ox);
    if (OH < 1 || OW < 1) return sc.done(h->fail(BOD_ERR_INVALID_ARG, "bod_stage_conv: empty output"));
    auto run = [&]() -> bod_status {
        Plane in, res;
        BODCHK(new_plane(h, &in, B, H, W, Cin));
        // bf16x3: a pixel holds 2 * C slots, channel c -> hi at (c / 32) * 64 + c % 32, lo 32 slots further on
        auto put_split = [](std::vector<uint16_t>& dst, size_t pix_slot0, int c, float v) {
            const uint16_t hi = f2bf(v);
            const size_t slot = pix_slot0 + (size_t)(c >> 5) * 64 + (c & 31);
            dst[slot] = hi; dst[slot + 32] = f2bf(v - bf2f(hi));
        };
        std::vector<uint16_t> hx(f32 ? 0 : (size_t)B * in.bstride * Cin * (x3 ? 2 : 1), 0);
        std::vector<float> hx32(f32 ? (size_t)B * in.bstride * Cin : 0, 0.f);
        const bool hx_in = mxp && mx_mode != 2;
        for (int b = 0; b < B && hx_in; ++b)
            for (int y = 0; y < H; ++y)
                for (int xx = 0; xx < W; ++xx) {
                    const size_t pix = (size_t)b * in.bstride + (size_t)(y + 1) * in.pitch + (xx + 1);
                    (mxfmt == 2 ? pack_h4_row : pack_hx_row)(x + (((size_t)b * H + y) * W + xx) * Cin, Cin, reinterpret_cast<uint8_t*>(hx.data()) + pix * Cin * 4, false);
                }
        for (int b = 0; b < B && !hx_in; ++b)
            for (int y = 0; y < H; ++y)
                for (int xx = 0; xx < W; ++xx)
                    for (int c = 0; c < Cin; ++c) {
                        const size_t pix = (size_t)b * in.bstride + (size_t)(y + 1) * in.pitch + (xx + 1);
                        const size_t di = pix * Cin + c;
                        const float v = x[(((size_t)b * H + y) * W + xx) * Cin + c];
                        if (f32) hx32[di] = v; else if (x3) put_split(hx, pix * 2 * Cin, c, v); else hx[di] = f2bf(v);
                    }
        HIPCHK(h, hipMemcpyAsync(in.d, f32 ? (const void*)hx32.data() : (const void*)hx.data(),
                                 (size_t)B * in.bstride * Cin * h->es, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (residual) {
            BODCHK(new_plane(h, &res, B, OH, OW, Cout));
            std::vector<uint16_t> hr(f32 ? 0 : (size_t)B * res.bstride * Cout * (x3 ? 2 : 1), 0);
            std::vector<float> hr32(f32 ? (size_t)B * res.bstride * Cout : 0, 0.f);
            for (int b = 0; b < B; ++b)
                for (int y = 0; y < OH; ++y)
                    for (int xx = 0; xx < OW; ++xx)
                        for (int c = 0; c < Cout; ++c) {
                            const size_t pix = (size_t)b * res.bstride + (size_t)(y + 1) * res.pitch + (xx + 1);
                            const size_t di = pix * Cout + c;
                            const float v = residual[(((size_t)b * OH + y) * OW + xx) * Cout + c];
                            if (f32) hr32[di] = v; else if (x3) put_split(hr, pix * 2 * Cout, c, v); else hr[di] = f2bf(v);
                        }
            HIPCHK(h, hipMemcpyAsync(res.d, f32 ? (const void*)hr32.data() : (const void*)hr.data(),
                                     (size_t)B * res.bstride * Cout * h->es, hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
        }
        HostTensor k; k.shape = {KH, KW, Cin, Cout}; k.data.assign(w, w + (size_t)KH * KW * Cin * Cout);
        h->host_w["stage/0"] = std::move(k);
        if (bias) { HostTensor bt; bt.shape = {Cout}; bt.data.assign(bias, bias + Cout); h->host_w["stage/1"] = std::move(bt); }
        PackedConv pc;
        BODCHK(pack_conv(h, "stage", "", 64, &pc, hx_in ? mxfmt : 0));
        // dense fp32 / bf16 output [B,OH,OW,Cout]
        const bool drop = dropout_rate > 0.f;
        const size_t n_out = (size_t)B * OH * OW * Cout;
        float* d_out32 = nullptr; uint16_t* d_out16 = nullptr;
        const bool f32_out = f32 || (!round_output_bf16 && !drop);
        if (f32_out) BODCHK(h->dalloc(&d_out32, n_out)); else BODCHK(h->dalloc(&d_out16, n_out * (x3 ? 2 : 1)));
        std::vector<RowEnt> rows = forward_row_table(B, OH, OW, stride, oy, ox, in.pitch, in.bstride);
        for (size_t r = 0; r < rows.size(); ++r) {          // dense output, the residual's plane, the dropout stream of (image, pixel)
            const int b = (int)(r / ((size_t)OH * OW)), p = (int)(r % ((size_t)OH * OW));
            rows[r].out_off = (int32_t)r;
            if (residual) rows[r].res_off = (int32_t)(b * res.bstride + (int64_t)(p / OW + 1) * res.pitch + (p % OW + 1));
            rows[r].rng_p = p;
            rows[r].rng_zs = b;
        }
        RowEnt* d_rows = nullptr;
        BODCHK(h->dalloc(&d_rows, rows.size(), false));
        HIPCHK(h, hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(RowEnt), hipMemcpyHostToDevice, h->stream));
        ConvArgs a = base_args(pc, d_rows, B * OH * OW, Cin, Cout);
        a.g[0] = ConvGroup{in.d, pc.w, pc.bias, f32_out ? (void*)d_out32 : (void*)d_out16, residual ? res.d : nullptr, nullptr, 0, layer_id, nullptr, nullptr, nullptr, 0, 0};
        if (mxp) {                  // the tower kernel lives on the row-reuse loop: 256-slot tiles of x-adjacent runs + extended rows (plan_tables.h)
            std::vector<RowEnt> tiled;
            std::vector<ExtRow> ext;
            if (!xr_tile_rows(rows, tiled, ext)) return h->fail(BOD_ERR_INVALID_ARG, "bod_stage_conv: row-reuse tiling failed");
            RowEnt* d_tiled = nullptr; int2* d_ext = nullptr;
            BODCHK(h->dalloc(&d_tiled, tiled.size(), false));
            BODCHK(h->dalloc(&d_ext, ext.size(), false));
            HIPCHK(h, hipMemcpyAsync(d_tiled, tiled.data(), tiled.size() * sizeof(RowEnt), hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(d_ext, ext.data(), ext.size() * sizeof(int2), hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            a.rows = d_tiled; a.M = (int)tiled.size(); a.ext = d_ext; a.xreuse = 2;
            a.mx = mx_mode == 2 ? 2 : (mxfmt == 2 ? 3 : 1);
            a.g[0].out_hx = mx_mode != 0 ? mxfmt : 0;
        }
        a.flags = (relu ? CONV_RELU : 0) | (drop ? CONV_DROPOUT : 0) | ((f32_out && !f32) ? CONV_OUT_F32 : 0);
        if (stride == 1 && same_padding && KH == 3 && KW == 3) { a.plane_h = OH; a.plane_w = OW; }      // (the sliding-window kernels walk planes)
        a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.image_base = image_id;
        a.drop_threshold = (uint32_t)std::floor((double)dropout_rate * 65536.0);
        a.drop_scale = (float)(1.0 / (1.0 - (double)dropout_rate));
        if (const char* ks = getenv("BOD_STAGE_KSPLIT")) {        // test hook: run this stage through the split-K path
            const int S = atoi(ks);
            if (S > 1 && !f32_out && !drop && (Cin / 64) % S == 0 && Cin % 64 == 0) {
                a.ksplit = S;
                BODCHK(h->dalloc(&a.partial, (size_t)S * a.M * a.cout_pad));
            }
        }
        if (x3) to_split_args(&a);
        HIPCHK(h, f32 ? launch_conv_igemm_f32(a, h->stream) : launch_conv_igemm(a, h->stream));
        if (f32_out) {
            HIPCHK(h, hipMemcpyAsync(out, d_out32, n_out * 4, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
        } else {
            std::vector<uint16_t> ho(n_out * (x3 ? 2 : 1));
            HIPCHK(h, hipMemcpyAsync(ho.data(), d_out16, ho.size() * 2, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            if (mxp && mx_mode != 0) {
                for (size_t px = 0; px < n_out / Cout; ++px) (mxfmt == 2 ? unpack_h4_row : unpack_hx_row)(reinterpret_cast<const uint8_t*>(ho.data()) + px * Cout * 4, Cout, out + px * Cout);
            } else if (x3) {
                for (size_t px = 0; px < n_out / Cout; ++px)
                    for (int c = 0; c < Cout; ++c) {
                        const size_t slot = px * 2 * Cout + (size_t)(c >> 5) * 64 + (c & 31);
                        out[px * Cout + c] = bf2f(ho[slot]) + bf2f(ho[slot + 32]);
                    }
            } else {
                for (size_t i = 0; i < n_out; ++i) out[i] = bf2f(ho[i]);
            }
        }
        return BOD_OK;
    };
    return sc.done(run());
}

bod_status bod_stage_conv_wgrad(int32_t device, const float* x, int32_t B, int32_t H, int32_t W, int32_t Cin,
                                const float* dy, int32_t KH, int32_t KW, int32_t Cout, int32_t stride, int32_t same_padding,
                                int32_t ksplit, float* dw, float* db) {
    StageScope sc;
    bod_context* h = sc.h;
    h->es = 2;
    if (!x || !dy || !dw || B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || KH < 1 || KW < 1 || KH > 3 || KW > 3 || stride < 1 || stride > 2)
        return sc.done(h->fail(BOD_ERR_INVALID_ARG, "bod_stage_conv_wgrad: bad argument"));
    if (const bod_status st = sc.open(device)) return sc.done(st);
    h->cfg.batch = B;
    int OH, OW, oy, ox;
    conv_out_geometry(H, W, KH, KW, stride, same_padding != 0, &OH, &OW, &oy, &ox);
    if (OH < 1 || OW < 1) return sc.done(h->fail(BOD_ERR_INVALID_ARG, "bod_stage_conv_wgrad: empty output"));
    auto run = [&]() -> bod_status {
        const int M = B * OH * OW, taps = KH * KW;
        // ---- forward-layout inputs: padded bf16 plane of x, dense bf16 dY, the forward row table
        Plane in;
        BODCHK(new_plane(h, &in, B, H, W, Cin));
        std::vector<uint16_t> hx((size_t)B * in.bstride * Cin, 0);
        for (int b = 0; b < B; ++b)
            for (int y = 0; y < H; ++y)
                for (int xx = 0; xx < W; ++xx)
                    for (int c = 0; c < Cin; ++c)
                        hx[((size_t)b * in.bstride + (size_t)(y + 1) * in.pitch + (xx + 1)) * Cin + c] = f2bf(x[(((size_t)b * H + y) * W + xx) * Cin + c]);
        HIPCHK(h, hipMemcpyAsync(in.d, hx.data(), hx.size() * 2, hipMemcpyHostToDevice, h->stream));
        std::vector<uint16_t> hdy((size_t)M * Cout);
        for (size_t i = 0; i < hdy.size(); ++i) hdy[i] = f2bf(dy[i]);
        uint16_t* d_dy = nullptr;
        BODCHK(h->dalloc(&d_dy, hdy.size(), false));
        HIPCHK(h, hipMemcpyAsync(d_dy, hdy.data(), hdy.size() * 2, hipMemcpyHostToDevice, h->stream));
        const std::vector<RowEnt> rows = forward_row_table(B, OH, OW, stride, oy, ox, in.pitch, in.bstride);
        RowEnt* d_rows = nullptr;
        BODCHK(h->dalloc(&d_rows, rows.size(), false));
        HIPCHK(h, hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(RowEnt), hipMemcpyHostToDevice, h->stream));
        // ---- K-contiguous operands: dY^T [cout_pad][Kpad] and Xcol^T [taps*Cin + 1][Kpad] (last row = ones -> db)
        const int cout_pad = (Cout + 63) / 64 * 64;
        const int N = taps * Cin + 1;
        int S = ksplit;
        if (S < 1) {                                  // enough splits for ~512 workgroups, >= 4 K-tiles each
            const long tiles = (long)((N + 127) / 128) * (cout_pad % 128 == 0 ? cout_pad / 128 : cout_pad / 64);
            S = 1;
            while (tiles * S < 512 && S < 64 && (long)M / (64L * S * 2) >= 4) S *= 2;
        }
        const int Kpad = (M + 64 * S - 1) / (64 * S) * (64 * S);
        uint16_t* d_dyt = nullptr; uint16_t* d_xct = nullptr;
        BODCHK(h->dalloc(&d_dyt, (size_t)cout_pad * Kpad));                 // zero-filled: rows >= Cout stay 0
        BODCHK(h->dalloc(&d_xct, (size_t)N * Kpad, false));
        HIPCHK(h, launch_gather_transpose(d_dy, nullptr, d_dyt, M, Kpad, Cout, Cout, 1, 1, false, h->stream));
        HIPCHK(h, launch_gather_transpose(in.d, d_rows, d_xct, M, Kpad, Cin, Cin, taps, KW, true, h->stream));
        // ---- the forward kernel as a plain GEMM: "pixels" = rows of Xcol^T, "weights" = dY^T, reduction = pixels
        std::vector<RowEnt> grow((size_t)N);
        for (int n = 0; n < N; ++n) { RowEnt e{}; e.in_off = n; e.out_off = n; grow[n] = e; }
        RowEnt* d_grow = nullptr;
        BODCHK(h->dalloc(&d_grow, grow.size(), false));
        HIPCHK(h, hipMemcpyAsync(d_grow, grow.data(), grow.size() * sizeof(RowEnt), hipMemcpyHostToDevice, h->stream));
        float* d_zero = nullptr; float* d_out = nullptr; float* d_part = nullptr;
        BODCHK(h->dalloc(&d_zero, (size_t)cout_pad));
        BODCHK(h->dalloc(&d_out, (size_t)N * Cout));
        ConvArgs a{};
        a.rows = d_grow; a.M = N; a.taps = 1; a.KW = 1; a.cin = Kpad; a.in_cstride = Kpad;
        a.cout_pad = cout_pad; a.cout_valid = Cout; a.out_cstride = Cout; a.res_cstride = Cout; a.groups = 1;
        a.fan_count = 1; a.flags = CONV_OUT_F32;
        a.g[0] = ConvGroup{d_xct, d_dyt, d_zero, d_out, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, 0, 0};
        if (S > 1) {
            a.ksplit = S;
            BODCHK(h->dalloc(&d_part, (size_t)S * N * cout_pad, false));
            a.partial = d_part;
        }
        HIPCHK(h, launch_conv_igemm(a, h->stream));
        std::vector<float> ho((size_t)N * Cout);
        HIPCHK(h, hipMemcpyAsync(ho.data(), d_out, ho.size() * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        std::memcpy(dw, ho.data(), (size_t)taps * Cin * Cout * 4);           // [(tap, ci)][co] == HWIO
        if (db) std::memcpy(db, ho.data() + (size_t)taps * Cin * Cout, (size_t)Cout * 4);
        return BOD_OK;
    };
    return sc.done(run());
}

// the handle's buffers of reg_kind 5 (kernels.h: launch_loss_compact), allocated on first use -- never inside a capture: the
// training step runs every configuration eagerly once before it records it
static bod_status energy_buffers(bod_context* h) {
    const size_t n = (size_t)h->cfg.batch * h->A;
    if (!h->energy_list) BODCHK(h->dalloc(&h->energy_list, n + 1));
    if (!h->energy_term) BODCHK(h->dalloc(&h->energy_term, n));
    return BOD_OK;
}

// what bod_loss_options may hold: NULL = the defaults
static bool loss_options_ok(const bod_loss_options* o) {
    return !o || (o->energy_samples >= BOD_ENERGY_MIN_SAMPLES && o->energy_samples <= BOD_ENERGY_MAX_SAMPLES);
}

static bod_status loss_impl(int32_t device, int32_t B, int32_t A, int32_t C, const float* cls, const float* cls_t,
                            const float* box, const float* box_t, const float* cov, const float* anchors,
                            const uint8_t* pos, const uint8_t* neg, int32_t do_cls, int32_t reg_kind,
                            float label_smoothing, double* out4, float w_cls, float w_reg, float* dcls, float* dbox, float* dcov,
                            const bod_loss_options* opt) {
    StageScope sc;
    bod_context* h = sc.h;
    if (B < 1 || A < 1 || (C != 4 && C != 8) || !pos || !neg || !out4 || reg_kind < 0 || reg_kind > 5)
        return sc.done(h->fail(BOD_ERR_INVALID_ARG, "bod_loss_forward: bad argument (C must be 4 or 8)"));
    if (!loss_options_ok(opt))
        return sc.done(h->fail(BOD_ERR_INVALID_ARG, "bod_loss_forward: energy_samples %d outside [%d, %d]", opt->energy_samples,
                            BOD_ENERGY_MIN_SAMPLES, BOD_ENERGY_MAX_SAMPLES));
    if (reg_kind == 5 && (long long)B * A >= 0x7fffffffLL)
        return sc.done(h->fail(BOD_ERR_INVALID_ARG, "bod_loss_forward: reg_kind 5 takes fewer than 2^31 - 1 anchors in a call"));
    if ((do_cls && (!cls || !cls_t)) || (reg_kind && (!box || !box_t)) || (reg_kind >= 2 && (!cov || !anchors)))
        return sc.done(h->fail(BOD_ERR_INVALID_ARG, "bod_loss_forward: a tensor required by the selected losses is NULL"));
    if (const bod_status st = sc.open(device)) return sc.done(st);
    auto run = [&]() -> bod_status {
        const size_t n = (size_t)B * A;
        LossArgs a{};
        a.B = B; a.A = A; a.C = C; a.do_cls = do_cls; a.reg_kind = reg_kind; a.label_smoothing = label_smoothing;
        auto up = [&](const void* src, size_t bytes, const void** dst) -> bod_status {
            if (!src) { *dst = nullptr; return BOD_OK; }
            char* d = nullptr;
            BODCHK(h->dalloc(&d, bytes, false));
            HIPCHK(h, hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, h->stream));
            *dst = d;
            return BOD_OK;
        };
        BODCHK(up(cls, n * C * 4, (const void**)&a.cls)); BODCHK(up(cls_t, n * C * 4, (const void**)&a.cls_t));
        BODCHK(up(box, n * 16, (const void**)&a.box)); BODCHK(up(box_t, n * 16, (const void**)&a.box_t));
        BODCHK(up(cov, n * 40, (const void**)&a.cov)); BODCHK(up(anchors, (size_t)A * 16, (const void**)&a.anchors));
        BODCHK(up(pos, n, (const void**)&a.pos)); BODCHK(up(neg, n, (const void**)&a.neg));
        const int nblocks = (int)((n + 255) / 256);
        float* partial = nullptr;
        BODCHK(h->dalloc(&partial, (size_t)nblocks * 4));
        EnergyArgs ea{};
        if (reg_kind == 5) {                                              // the positives' energy terms first: launch_loss sums them
            int32_t* list = nullptr; float* term = nullptr;
            BODCHK(h->dalloc(&list, n + 1)); BODCHK(h->dalloc(&term, n));
            ea.B = B; ea.A = A; ea.M = opt ? opt->energy_samples : BOD_ENERGY_DEFAULT_SAMPLES;
            ea.box = a.box; ea.box_t = a.box_t; ea.cov = a.cov; ea.anchors = a.anchors;
            ea.seed_lo = opt ? (uint32_t)opt->seed : 0u; ea.seed_hi = opt ? (uint32_t)(opt->seed >> 32) : 0u;
            ea.first_image_id = opt ? opt->first_image_id : 0u;
            ea.id_stride = (opt && (opt->reserved[0] & BOD_LOSS_ONE_IMAGE_ID)) ? 0 : 1;
            ea.list = list; ea.row_term = term; a.row_term = term;
            HIPCHK(h, launch_loss_compact(a.pos, (long long)n, list, h->stream));
            HIPCHK(h, launch_energy_forward(ea, h->stream));
        }
        HIPCHK(h, launch_loss(a, partial, nblocks, h->stream));
        std::vector<float> hp((size_t)nblocks * 4);
        HIPCHK(h, hipMemcpyAsync(hp.data(), partial, hp.size() * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        for (int q = 0; q < 4; ++q) out4[q] = 0.0;
        for (int b = 0; b < nblocks; ++b)
            for (int q = 0; q < 4; ++q) out4[q] += (double)hp[(size_t)b * 4 + q];
        if (dcls || dbox || dcov) {
            float* sums = nullptr; float* g_cls = nullptr; float* g_box = nullptr; float* g_cov = nullptr;
            BODCHK(h->dalloc(&sums, 4));
            if (dcls) BODCHK(h->dalloc(&g_cls, n * C));
            if (dbox) BODCHK(h->dalloc(&g_box, n * 4));
            if (dcov) BODCHK(h->dalloc(&g_cov, n * 10));
            HIPCHK(h, launch_loss_reduce(partial, nblocks, sums, h->stream));
            HIPCHK(h, launch_loss_backward(a, sums, w_cls, w_reg, g_cls, g_box, g_cov, h->stream));
            if (reg_kind == 5 && (g_box || g_cov)) HIPCHK(h, launch_energy_backward(ea, sums, w_reg, g_box, g_cov, h->stream));
            if (dcls) HIPCHK(h, hipMemcpyAsync(dcls, g_cls, n * C * 4, hipMemcpyDeviceToHost, h->stream));
            if (dbox) HIPCHK(h, hipMemcpyAsync(dbox, g_box, n * 16, hipMemcpyDeviceToHost, h->stream));
            if (dcov) HIPCHK(h, hipMemcpyAsync(dcov, g_cov, n * 40, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
        }
        return BOD_OK;
    };
    return sc.done(run());
}

bod_status bod_loss_forward_ex(int32_t device, int32_t B, int32_t A, int32_t C, const float* cls, const float* cls_t,
                               const float* box, const float* box_t, const float* cov, const float* anchors,
                               const uint8_t* pos, const uint8_t* neg, int32_t do_cls, int32_t reg_kind,
                               float label_smoothing, double* out4, const bod_loss_options* options) {
    return loss_impl(device, B, A, C, cls, cls_t, box, box_t, cov, anchors, pos, neg, do_cls, reg_kind, label_smoothing, out4,
                     0.f, 0.f, nullptr, nullptr, nullptr, options);
}

bod_status bod_loss_forward(int32_t device, int32_t B, int32_t A, int32_t C, const float* cls, const float* cls_t,
                            const float* box, const float* box_t, const float* cov, const float* anchors,
                            const uint8_t* pos, const uint8_t* neg, int32_t do_cls, int32_t reg_kind,
                            float label_smoothing, double* out4) {
    return bod_loss_forward_ex(device, B, A, C, cls, cls_t, box, box_t, cov, anchors, pos, neg, do_cls, reg_kind, label_smoothing, out4,
                               nullptr);
}

bod_status bod_loss_backward_ex(int32_t device, int32_t B, int32_t A, int32_t C, const float* cls, const float* cls_t,
                                const float* box, const float* box_t, const float* cov, const float* anchors,
                                const uint8_t* pos, const uint8_t* neg, int32_t do_cls, int32_t reg_kind,
                                float label_smoothing, float w_cls, float w_reg, double* out4, float* dcls, float* dbox, float* dcov,
                                const bod_loss_options* options) {
    if (!dcls && !dbox && !dcov) return BOD_ERR_INVALID_ARG;
    return loss_impl(device, B, A, C, cls, cls_t, box, box_t, cov, anchors, pos, neg, do_cls, reg_kind, label_smoothing, out4,
                     w_cls, w_reg, dcls, dbox, dcov, options);
}

bod_status bod_loss_backward(int32_t device, int32_t B, int32_t A, int32_t C, const float* cls, const float* cls_t,
                             const float* box, const float* box_t, const float* cov, const float* anchors,
                             const uint8_t* pos, const uint8_t* neg, int32_t do_cls, int32_t reg_kind,
                             float label_smoothing, float w_cls, float w_reg, double* out4, float* dcls, float* dbox, float* dcov) {
    return bod_loss_backward_ex(device, B, A, C, cls, cls_t, box, box_t, cov, anchors, pos, neg, do_cls, reg_kind, label_smoothing, w_cls,
                                w_reg, out4, dcls, dbox, dcov, nullptr);
}

bod_status bod_set_loss_options(bod_handle h, const bod_loss_options* options) {
    if (!h) return BOD_ERR_INVALID_ARG;
    if (!loss_options_ok(options))
        return h->fail(BOD_ERR_INVALID_ARG, "bod_set_loss_options: energy_samples %d outside [%d, %d]", options->energy_samples,
                       BOD_ENERGY_MIN_SAMPLES, BOD_ENERGY_MAX_SAMPLES);
    h->energy_samples = options ? options->energy_samples : BOD_ENERGY_DEFAULT_SAMPLES;
    h->loss_seed = options ? options->seed : 0;
    h->loss_first_image_id = options ? options->first_image_id : 0;
    h->loss_id_stride = (options && (options->reserved[0] & BOD_LOSS_ONE_IMAGE_ID)) ? 0 : 1;
    return BOD_OK;
}

// Packs a minibatch's ground truth for launch_anchor_targets: [B+1] row offsets, then the [sum G,4] corners, then the [sum G,C]
// class rows, each part starting on a 16-byte boundary (the kernel reads rows as float4)
struct PackedGt { std::vector<char> bytes; size_t box_off = 0, cls_off = 0; long long sum_g = 0; };
static void pack_gt(int32_t B, const int32_t* num_gt, const float* gt_boxes, const float* gt_classes, int32_t C, PackedGt* p) {
    p->sum_g = 0;
    for (int b = 0; b < B; ++b) p->sum_g += num_gt[b];
    p->box_off = ((size_t)(B + 1) * 4 + 15) & ~(size_t)15;
    p->cls_off = p->box_off + (size_t)p->sum_g * 16;
    p->bytes.resize(p->cls_off + (size_t)p->sum_g * C * 4);
    int32_t* off = reinterpret_cast<int32_t*>(p->bytes.data());
    off[0] = 0;
    for (int b = 0; b < B; ++b) off[b + 1] = off[b] + num_gt[b];
    std::memcpy(p->bytes.data() + p->box_off, gt_boxes, (size_t)p->sum_g * 16);
    std::memcpy(p->bytes.data() + p->cls_off, gt_classes, (size_t)p->sum_g * C * 4);
}

bod_status bod_anchor_targets(int32_t device, int32_t A, const float* anchors_vuhw, int32_t B, const int32_t* num_gt,
                              const float* gt_boxes_vuvu, const float* gt_classes, int32_t C, float min_positive_iou,
                              float max_negative_iou, float* cls_targets, float* box_targets, uint8_t* positive_mask,
                              uint8_t* negative_mask, int32_t* best_gt, float* best_iou) {
    StageScope sc;
    bod_context* h = sc.h;
    if (A < 1 || B < 1 || B > 65535 || C < 2)
        return sc.done(h->fail(BOD_ERR_INVALID_ARG, "bod_anchor_targets: bad argument (A = %d, B = %d in 1..65535, C = %d >= 2)", A, B, C));
    if (!anchors_vuhw || !num_gt || !gt_boxes_vuvu || !gt_classes || !cls_targets || !box_targets || !positive_mask || !negative_mask)
        return sc.done(h->fail(BOD_ERR_INVALID_ARG, "bod_anchor_targets: a required array is NULL"));
    for (int b = 0; b < B; ++b)
        if (num_gt[b] < 1)
            return sc.done(h->fail(BOD_ERR_INVALID_ARG, "bod_anchor_targets: frame %d has %d ground-truth rows (at least the placeholder row is "
                                "required)", b, num_gt[b]));
    if (const bod_status st = sc.open(device)) return sc.done(st);
    auto run = [&]() -> bod_status {
        const size_t n = (size_t)B * A;
        PackedGt p;
        pack_gt(B, num_gt, gt_boxes_vuvu, gt_classes, C, &p);
        char* d_gt = nullptr; float* d_anchors = nullptr;
        BODCHK(h->dalloc(&d_gt, p.bytes.size(), false)); BODCHK(h->dalloc(&d_anchors, (size_t)A * 4, false));
        HIPCHK(h, hipMemcpyAsync(d_gt, p.bytes.data(), p.bytes.size(), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_anchors, anchors_vuhw, (size_t)A * 16, hipMemcpyHostToDevice, h->stream));
        TargetArgs a{};
        a.A = A; a.B = B; a.C = C; a.min_positive_iou = min_positive_iou; a.max_negative_iou = max_negative_iou;
        a.anchors = d_anchors; a.gt_off = reinterpret_cast<const int32_t*>(d_gt);
        a.gt_boxes = reinterpret_cast<const float*>(d_gt + p.box_off); a.gt_classes = reinterpret_cast<const float*>(d_gt + p.cls_off);
        BODCHK(h->dalloc(&a.cls_t, n * C, false)); BODCHK(h->dalloc(&a.box_t, n * 4, false));
        BODCHK(h->dalloc(&a.pos, n, false)); BODCHK(h->dalloc(&a.neg, n, false));
        if (best_gt) BODCHK(h->dalloc(&a.best_gt, n, false));
        if (best_iou) BODCHK(h->dalloc(&a.best_iou, n, false));
        HIPCHK(h, launch_anchor_targets(a, h->stream));
        HIPCHK(h, hipMemcpyAsync(cls_targets, a.cls_t, n * C * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(box_targets, a.box_t, n * 16, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(positive_mask, a.pos, n, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(negative_mask, a.neg, n, hipMemcpyDeviceToHost, h->stream));
        if (best_gt) HIPCHK(h, hipMemcpyAsync(best_gt, a.best_gt, n * 4, hipMemcpyDeviceToHost, h->stream));
        if (best_iou) HIPCHK(h, hipMemcpyAsync(best_iou, a.best_iou, n * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return BOD_OK;
    };
    return sc.done(run());
}

// PDQ evaluation (pdq_kernels.hip): stateless, one stream for the call
static bod_status pdq_call(int32_t device, const std::function<int(hipStream_t, char*, size_t)>& run) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        char buf[128];
        snprintf(buf, sizeof buf, "no HIP device %d: libbayesod_hip has no CPU fallback", device);
        g_create_error = buf;
        return BOD_ERR_NO_DEVICE;
    }
    hipStream_t s = nullptr;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
        g_create_error = "cannot set up the device for the PDQ evaluation";
        return BOD_ERR_HIP;
    }
    char err[1024] = {0};
    const int st = run(s, err, sizeof err);
    hipStreamSynchronize(s);
    hipStreamDestroy(s);
    if (st != BOD_OK) g_create_error = err;
    return (bod_status)st;
}

bod_status bod_pdq_corner_heatmaps(int32_t device, int32_t img_h, int32_t img_w, int32_t n, const double* means_yx,
                                   const double* covs_yx, int32_t* rois, float* heatmaps) {
    return pdq_call(device, [&](hipStream_t s, char* err, size_t cap) {
        return pdq_corner_heatmaps_run(img_h, img_w, n, means_yx, covs_yx, rois, heatmaps, s, err, cap);
    });
}

bod_status bod_pdq_frames(int32_t device, int32_t img_h, int32_t img_w, int32_t num_frames, const int32_t* num_gt,
                          const int32_t* gt_boxes, const int32_t* num_det, const int32_t* det_boxes,
                          const double* det_corner_covs, double* fg_loss, double* bg_loss, double* det_bg_loss,
                          float* heatmaps) {
    return pdq_call(device, [&](hipStream_t s, char* err, size_t cap) {
        return pdq_frames_run(img_h, img_w, num_frames, num_gt, gt_boxes, num_det, det_boxes, det_corner_covs, fg_loss, bg_loss,
                              det_bg_loss, heatmaps, s, err, cap);
    });
}

bod_status bod_score_pairs(int32_t device, int64_t n, const double* means, const double* covs, const double* targets,
                           int32_t num_samples, uint64_t seed, uint64_t first_row_id, double* out, int32_t* status) {
    return pdq_call(device, [&](hipStream_t s, char* err, size_t cap) {
        return score_pairs_run(n, means, covs, targets, num_samples, seed, first_row_id, out, status, s, err, cap);
    });
}

// The corruption stage alone (bayesod.h): packed frames in, packed frames out.  Stateless; its buffers live for the call.
bod_status bod_corrupt_frames_u8(int32_t device, int32_t n, const uint8_t* rgb_packed_in, const int32_t* src_hw, const bod_corrupt_op* ops,
                                 int32_t ops_per_frame, const uint32_t* frame_ids, const uint16_t* taps, int32_t n_taps, const uint8_t* luts,
                                 int32_t n_luts, const uint16_t* qtables, int32_t n_qtables, uint64_t seed, uint8_t* rgb_packed_out) {
    static const char* who = "bod_corrupt_frames_u8";
    if (n < 1 || !rgb_packed_in || !src_hw || !ops || !rgb_packed_out) { g_create_error = std::string(who) + ": NULL argument or no frame"; return BOD_ERR_INVALID_ARG; }
    CorruptSpec spec;
    {
        char err[512] = {0};
        const int st = corrupt_spec_make(who, n, ops, ops_per_frame, frame_ids, taps, n_taps, luts, n_luts, qtables, n_qtables, seed, &spec, err, sizeof err);
        if (st != BOD_OK) { g_create_error = err; return (bod_status)st; }
    }
    return pdq_call(device, [&](hipStream_t s, char* err, size_t cap) -> int {
        CorruptSlot slot;
        uint8_t* d_rgb = nullptr;
        uint8_t* d_out = nullptr;
        int st = corrupt_prepare(slot, who, spec, src_hw, s, err, cap);
        if (st == BOD_OK && hipMalloc(reinterpret_cast<void**>(&d_rgb), slot.frame_bytes) != hipSuccess) {
            d_rgb = nullptr; snprintf(err, cap, "%s: out of device memory for the frames", who); st = BOD_ERR_OOM;
        }
        if (st == BOD_OK && hipMemcpyAsync(d_rgb, rgb_packed_in, slot.frame_bytes, hipMemcpyHostToDevice, s) != hipSuccess) {
            snprintf(err, cap, "%s: copying the frames in failed", who); st = BOD_ERR_HIP;
        }
        if (st == BOD_OK) st = corrupt_enqueue(slot, who, spec, d_rgb, s, &d_out, err, cap);
        if (st == BOD_OK && (hipMemcpyAsync(rgb_packed_out, d_out, slot.frame_bytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
                             hipStreamSynchronize(s) != hipSuccess)) {
            snprintf(err, cap, "%s: copying the frames back failed: %s", who, hipGetErrorString(hipGetLastError())); st = BOD_ERR_HIP;
        }
        hipStreamSynchronize(s);
        if (d_rgb) hipFree(d_rgb);
        slot.release();
        return st;
    });
}

bod_status bod_set_upload_corruption(bod_handle h, const bod_corrupt_op* ops, int32_t ops_per_frame, const uint32_t* frame_ids,
                                     const uint16_t* taps, int32_t n_taps, const uint8_t* luts, int32_t n_luts, const uint16_t* qtables,
                                     int32_t n_qtables, uint64_t seed) {
    if (!h) return BOD_ERR_INVALID_ARG;
    if (!ops) { h->corrupt_pending = CorruptSpec{}; return BOD_OK; }
    CorruptSpec spec;
    char err[512] = {0};
    const int st = corrupt_spec_make("bod_set_upload_corruption", h->cfg.batch, ops, ops_per_frame, frame_ids, taps, n_taps, luts, n_luts, qtables,
                                     n_qtables, seed, &spec, err, sizeof err);
    if (st != BOD_OK) return h->fail((bod_status)st, "%s", err);
    h->corrupt_pending = std::move(spec);
    return BOD_OK;
}

// The rendering stage (bayesod.h; render_kernels.hip).  Stateless; arguments are checked before a device is looked for.
bod_status bod_render_frames_u8(int32_t device, int32_t n, const uint8_t* rgb_packed_in, const int32_t* src_hw, const int32_t* num_det,
                                const int32_t* det_boxes, const float* det_corner_covs, const uint8_t* det_colors, const uint8_t* det_text,
                                const int32_t* num_gt, const int32_t* gt_boxes, const bod_render_options* opt, uint8_t* rgb_packed_out,
                                int32_t* skipped_ellipses) {
    {
        char err[512] = {0};
        const int st = render_validate(n, rgb_packed_in, src_hw, num_det, det_boxes, det_corner_covs, det_colors, det_text, num_gt, gt_boxes, opt,
                                       rgb_packed_out, err, sizeof err);
        g_create_error = err;
        if (st != BOD_OK || n == 0) return (bod_status)st;
    }
    return pdq_call(device, [&](hipStream_t s, char* err, size_t cap) -> int {
        return render_frames_run(n, rgb_packed_in, src_hw, num_det, det_boxes, det_corner_covs, det_colors, det_text, num_gt, gt_boxes, opt,
                                 rgb_packed_out, skipped_ellipses, s, err, cap);
    });
}

bod_status bod_render_font(uint8_t* glyph_rows, int32_t* count) {
    if (!count) { g_create_error = "bod_render_font: count is NULL"; return BOD_ERR_INVALID_ARG; }
    *count = RENDER_FONT_COUNT;
    if (glyph_rows) memcpy(glyph_rows, RENDER_FONT, sizeof RENDER_FONT);
    return BOD_OK;
}

bod_status bod_bench_head_conv(bod_handle h, int32_t layer, int32_t variant, int32_t iters, double* mean_ms, double* flops) {
    if (!h || !mean_ms || iters < 1 || layer < 0 || layer > 7) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    if (!h->weights_ready) return h->fail(BOD_ERR_NOT_READY, "weights not finalized");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int seen = 0; Op* op = nullptr;
    for (Op& o : h->ops) if (o.is_head3x3 && o.flavour != FLAVOUR_RAW && seen++ == layer) { op = &o; break; }    // (layers 2, 3: the flavour bod_infer runs)
    if (!op) return h->fail(BOD_ERR_INVALID_ARG, "no head launch %d", layer);
    ConvArgs a = op->conv;
    a.variant = variant;
    hipEvent_t e0, e1;
    HIPCHK(h, hipEventCreate(&e0)); HIPCHK(h, hipEventCreate(&e1));
    HIPCHK(h, launch_conv_igemm(a, h->stream));            // warm-up
    HIPCHK(h, hipEventRecord(e0, h->stream));
    for (int i = 0; i < iters; ++i) HIPCHK(h, launch_conv_igemm(a, h->stream));
    HIPCHK(h, hipEventRecord(e1, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    float ms = 0; HIPCHK(h, hipEventElapsedTime(&ms, e0, e1));
    hipEventDestroy(e0); hipEventDestroy(e1);
    if ((variant == 90 || variant == 91) && a.mx == 1) {
        unsigned long long c[16];
        conv_igemm_phase_cycles(c, true);
        const double tiles = (double)c[15];
        fprintf(stderr, "# f16mx phase clock, wave 0, cycles per tile (%.0f tiles): whole tile %.0f = set-up %.0f + loop %.0f (of which: waiting for the next K-tile's pieces + barrier %.0f, "
                        "K-tile bodies %.0f; 72 K-tiles) + epilogue %.0f; of the wait: vmcnt / lgkmcnt %.0f, s_barrier %.0f\n", tiles, (double)c[9] / tiles, ((double)c[8] - (double)c[6] - (double)c[7]) / tiles,
                ((double)c[6] + (double)c[7]) / tiles, (double)c[6] / tiles, (double)c[7] / tiles, ((double)c[9] - (double)c[8]) / tiles,
                (double)c[13] / tiles, ((double)c[6] - (double)c[13]) / tiles);
        // round 6: the loop by K-tile flavour (36 H K-tiles of four f16 k-steps, 36 X K-tiles of two block-scaled products: half the MFMA issue on
        // the same staged bytes), for wave 0 (early: issues the weight pieces) and wave 4 (late: its partner on the SIMD)
        fprintf(stderr, "# f16mx phase clock by K-tile flavour, cycles per K-tile: wave 0: H %.0f  X %.0f | wave 4: H %.0f  X %.0f, wait + barrier per K-tile %.0f (wave 0: %.0f)"
                        " | MFMA issue of a SIMD's two waves: H 2048, X 1024\n",
                (double)c[0] / tiles / 36.0, (double)c[1] / tiles / 36.0, (double)c[2] / tiles / 36.0, (double)c[3] / tiles / 36.0, (double)c[4] / tiles / 72.0, (double)c[6] / tiles / 72.0);
    } else if (variant == 90) {
        unsigned long long c[16];
        conv_igemm_phase_cycles(c, true);
        const double tiles = (double)c[15];
        static const char* names[6] = {"set-up", "main loop", "barrier+bias/relu/pack", "philox+lds writes", "barrier", "store loop"};
        fprintf(stderr, "# phase clock, wave 0, cycles per tile (%.0f tiles):", tiles);
        for (int k = 0; k < 6; ++k) fprintf(stderr, "  %s %.0f", names[k], (double)c[k] / tiles);
        // (aggregating tiles leave through the fused 1x1 + MC reduction instead of the store loop: slots 10..12)
        if (c[10] + c[11] + c[12] > 0)
            fprintf(stderr, "  fused 1x1 MFMAs %.0f  barriers+fp32 tile %.0f  MC reduction+stores %.0f", (double)c[10] / tiles, (double)c[11] / tiles, (double)c[12] / tiles);
        double cyc = 0; for (int k = 0; k < 6; ++k) cyc += (double)c[k];
        cyc += (double)c[10] + (double)c[11] + (double)c[12];
        fprintf(stderr, "  | shader clock during the tiles %.3f GHz (cycles / 100 MHz real-time ticks); tiles account for %.3f ms of the %.3f ms launch per CU\n",
                cyc / (double)c[14] * 0.1, (double)c[14] / tiles * 1e-5 * (tiles / (iters + 1)) / 256.0, ms / iters);
    }
    *mean_ms = ms / iters;
    if (flops) *flops = op->flops;
    return BOD_OK;
}

bod_status bod_profile_begin(bod_handle h) {
    if (!h) return BOD_ERR_INVALID_ARG;
    for (auto& e : h->ev_head) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
    for (auto& e : h->ev_post) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
    h->ev_head.clear(); h->ev_post.clear(); h->prof_flops = 0; h->profiling = true;
    return BOD_OK;
}

// ---- the path's one multi-GPU exchange through the C ABI ----
extern "C++" {
namespace {
// RCCL is opened at run time: the library neither links librccl nor needs it on a single GPU.  (ncclGather is RCCL's own entry point;
// datatype 7 = ncclFloat32, result 0 = ncclSuccess -- rccl.h.)
struct Rccl {
    typedef int (*gather_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
    typedef const char* (*errstr_fn)(int);
    gather_fn gather = nullptr; errstr_fn errstr = nullptr; bool tried = false;
    bool load() {
        if (tried) return gather != nullptr;
        tried = true;
        void* lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) return false;
        gather = reinterpret_cast<gather_fn>(dlsym(lib, "ncclGather"));
        errstr = reinterpret_cast<errstr_fn>(dlsym(lib, "ncclGetErrorString"));
        return gather != nullptr;
    }
};
Rccl& rccl() { static Rccl r; return r; }
}  // namespace
}  // extern "C++"

int32_t bod_record_width(bod_handle h) { return h ? record_layout(h).fields.width : 0; }

bod_status bod_gather_detections(bod_handle h, int32_t slot, void* nccl_comm, int32_t world, int32_t rank, int32_t root,
                                 float* gathered_host, float** gathered_device) {
    MarkerRange mr_api("bod:gather_detections");
    if (!h) return BOD_ERR_INVALID_ARG;
    if (world < 1 || rank < 0 || rank >= world || root < 0 || root >= world)
        return h->fail(BOD_ERR_INVALID_ARG, "bod_gather_detections: world %d, rank %d, root %d", world, rank, root);
    if (!nccl_comm && world != 1) return h->fail(BOD_ERR_INVALID_ARG, "bod_gather_detections: %d ranks need an ncclComm_t", world);
    if (rank != root && (gathered_host || gathered_device)) return h->fail(BOD_ERR_INVALID_ARG, "bod_gather_detections: only the root receives");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int B = h->cfg.batch, K = h->cfg.nms_max_output_size, C = h->cfg.num_classes, W = bod_record_width(h);
    const size_t block = (size_t)B * K * W;
    // where the records are and which stream finished them
    int sidx = slot;
    // Round 6: a ticket's pack kernel and gather no longer run on the side stream beside the next call's forward -- a kernel
    // of this library beside its convolution kernels can miscompute a 16-lane row, and the pack kernel is one.  They follow the slot's
    // records on the stream that finished them (the main stream; the back stream of a pipeline_overlap handle): if the next
    // bod_infer_async is already enqueued they run behind its kernels -- one step of latency, nothing beside anything.
    // BOD_SIDE_STREAM=1 (the repro switch of bod_infer_async): the side stream again.
    static const bool side_on = [] { const char* e = getenv("BOD_SIDE_STREAM"); return e && atoi(e) != 0; }();
    hipStream_t st = (slot >= 0 && slot <= 1 && !side_on && h->rec[slot].done_stream) ? h->rec[slot].done_stream : h->side;
    if (slot < 0) {
        // synchronous bod_infer / bod_cluster_fuse: the records are the current buffers, finished on the MAIN stream -- pack and gather
        // go out on that stream too, so the next bod_infer (which rewrites nms_nsel / out_* of this slot on the main stream) and
        // bod_synchronize are ordered behind them by stream order.  (On the side stream nothing would hold the main stream back.)
        if (!h->stage.cluster) return h->fail(BOD_ERR_NOT_READY, "bod_gather_detections: bod_cluster_fuse has not run");
        BODCHK(join_overlap(h));
        sidx = h->slot;
        st = h->stream;
    } else if (slot > 1 || !h->rec[slot].pending) {
        return h->fail(BOD_ERR_NOT_READY, "bod_gather_detections: slot %d has no pending batch", slot);
    }
    const RecordSlot& r = h->rec[sidx];
    for (int img = 0; h->parts && img < B; ++img)
        if (!r.parts_ok[img]) return h->fail(BOD_ERR_NOT_READY, "bod_gather_detections: image %d was fused without its posterior's parts (bod_set_posterior_parts)", img);
    for (int img = 0; h->cparts && img < B; ++img)
        if (!r.cparts_ok[img]) return h->fail(BOD_ERR_NOT_READY, "bod_gather_detections: image %d was fused without its posterior's class parts (bod_set_posterior_class_parts)", img);
    if (!h->rec_send && hipMalloc(reinterpret_cast<void**>(&h->rec_send), block * 4) != hipSuccess)
        return h->fail(BOD_ERR_OOM, "bod_gather_detections: %zu bytes", block * 4);
    // rec_send / rec_recv are shared by the ticket gathers (side stream) and the synchronous form (main stream): a gather that goes to
    // the other stream than the previous one waits for it -- nothing else orders the two streams against each other (round-4 advisor finding)
    if (h->ev_gather && h->gather_stream && h->gather_stream != st) HIPCHK(h, hipStreamWaitEvent(st, h->ev_gather, 0));
    // (on the side stream: behind the slot's event; on the records' own stream the wait is a no-op)
    if (slot >= 0) HIPCHK(h, hipStreamWaitEvent(st, r.done, 0));
    HIPCHK(h, launch_pack_records(r.nms_nsel, r.scores, r.means, r.covs, r.counts, r.parts, r.cparts, h->rec_send, B, K, C, st));
    float* recv = nullptr;
    if (rank == root) {
        if (world == 1 && !nccl_comm) recv = h->rec_send;
        else {
            if (h->rec_recv_elems < block * world) {
                if (h->rec_recv && h->rec_recv != h->rec_send) hipFree(h->rec_recv);
                h->rec_recv = nullptr; h->rec_recv_elems = 0;
                if (hipMalloc(reinterpret_cast<void**>(&h->rec_recv), block * world * 4) != hipSuccess)
                    return h->fail(BOD_ERR_OOM, "bod_gather_detections: %zu bytes", block * world * 4);
                h->rec_recv_elems = block * world;
            }
            recv = h->rec_recv;
        }
    }
    if (nccl_comm) {
        if (!rccl().load()) return h->fail(BOD_ERR_NOT_READY, "bod_gather_detections: librccl.so (ncclGather) could not be opened");
        const int rc = rccl().gather(h->rec_send, recv, block, /*ncclFloat32*/ 7, root, nccl_comm, st);
        if (rc != 0) return h->fail(BOD_ERR_HIP, "ncclGather: %s", rccl().errstr ? rccl().errstr(rc) : "error");
    }
    if (!h->ev_gather) HIPCHK(h, hipEventCreateWithFlags(&h->ev_gather, hipEventDisableTiming));
    if (rank == root && gathered_host) {
        HIPCHK(h, hipMemcpyAsync(gathered_host, recv, block * world * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipEventRecord(h->ev_gather, st)); h->gather_stream = st;
        HIPCHK(h, hipEventSynchronize(h->ev_gather));          // (the copy, not whatever was enqueued on the stream behind it)
    } else {
        HIPCHK(h, hipEventRecord(h->ev_gather, st)); h->gather_stream = st;
    }
    if (!(rank == root && gathered_host) && slot >= 0) {
        // keep bod_collect / the next bod_infer_async of this slot behind the send: re-record the slot's event
        HIPCHK(h, hipEventRecord(h->rec[slot].done, st));
    }
    if (gathered_device) *gathered_device = recv;
    return BOD_OK;
}

bod_status bod_plan_info(bod_handle h, int32_t* info8) {
    if (!h || !info8) return BOD_ERR_INVALID_ARG;
    if (!h->weights_ready) return h->fail(BOD_ERR_NOT_READY, "bod_plan_info: the plan is built by bod_finalize_weights");
    for (int i = 0; i < 8; ++i) info8[i] = 0;
    info8[0] = h->agg_plan; info8[1] = h->plan_fused_out; info8[2] = h->plan_xreuse; info8[3] = h->plan_xreuse0;
    info8[4] = (int32_t)h->ops.size();
    for (const Op& o : h->ops) if (o.kind == Op::CONV && !o.is_head3x3 && o.conv.xreuse) ++info8[5];
    info8[6] = h->plan_mx;
    info8[7] = h->plan_sparse;
    return BOD_OK;
}

bod_status bod_plan_info_n(bod_handle h, int32_t* info, int32_t n) {
    if (!h || !info || n < 0) return BOD_ERR_INVALID_ARG;
    int32_t all[11];
    BODCHK(bod_plan_info(h, all));
    all[8] = h->plan_halo;
    all[9] = h->plan_tail_rows;
    all[10] = h->plan_stage_end;
    for (int i = 0; i < n && i < 11; ++i) info[i] = all[i];
    return BOD_OK;
}

// ---- mergeable MC statistics (include/bayesod.h): handles created with mc_statistics = 1
static bod_status stat_handle(bod_handle h, const char* who) {
    if (!h->cfg.mc_statistics) return h->fail(BOD_ERR_INVALID_ARG, "%s: the handle was not created with mc_statistics = 1", who);
    BODCHK(join_overlap(h));
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return ensure_stat(h);
}

// Mirrored views need mirror-symmetric anchors (include/bayesod.h): checked on the host once per bod_set_anchors
static bod_status stat_view_ready(bod_handle h, const char* who, int32_t view) {
    if (view != BOD_VIEW_IDENTITY && view != BOD_VIEW_HFLIP)
        return h->fail(BOD_ERR_INVALID_ARG, "%s: view must be BOD_VIEW_IDENTITY (0) or BOD_VIEW_HFLIP (1), got %d", who, view);
    if (view == BOD_VIEW_IDENTITY) return BOD_OK;
    if (!h->anchors_ready) return h->fail(BOD_ERR_NOT_READY, "%s: bod_set_anchors has not been called (a mirrored view maps every anchor to its partner)", who);
    const bod_config& c = h->cfg;
    const int K = c.anchors_per_location;
    if (h->mirror_sym < 0) {
        std::vector<float> an((size_t)h->A * 4);
        HIPCHK(h, hipMemcpyAsync(an.data(), h->d_anchors, an.size() * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        const float fw = (float)c.image_w;
        int bad = -1;
        for (int l = 0; l < h->nlev && bad < 0; ++l) {
            const size_t off = (size_t)h->lvl_p0[l] * K;
            const int W = h->lw[l];
            for (int y = 0; y < h->lh[l] && bad < 0; ++y)
                for (int x = 0; x < W && bad < 0; ++x)
                    for (int k = 0; k < K; ++k) {
                        const float* s = &an[(off + ((size_t)y * W + x) * K + k) * 4];
                        const float* p = &an[(off + ((size_t)y * W + (W - 1 - x)) * K + k) * 4];
                        const float want[4] = {s[0], fw - s[1], s[2], s[3]};
                        if (memcmp(p, want, 16) != 0) { bad = l; break; }
                    }
        }
        h->mirror_sym = bad < 0; h->mirror_bad_level = bad < 0 ? 0 : c.min_level + bad;
    }
    if (!h->mirror_sym)
        return h->fail(BOD_ERR_INVALID_ARG, "%s: the anchors of pyramid level %d are not mirror-symmetric about image_w / 2 for a %dx%d image "
                       "(BOD_VIEW_HFLIP needs image_w to be a multiple of 2^max_level = %d)", who, h->mirror_bad_level, c.image_h, c.image_w,
                       1 << c.max_level);
    return BOD_OK;
}

// accumulator (+)= {cls_sum, box_moments, cov_sum} of kb samples, on the handle's stream; view = BOD_VIEW_HFLIP (checked by
// stat_view_ready): the record is that of the mirrored frames and is read through the mirror map
static bod_status stat_fold(bod_handle h, const char* who, const float* cls, const float* box, const float* cov, int kb, int32_t view = BOD_VIEW_IDENTITY) {
    if (kb < 1) return h->fail(BOD_ERR_INVALID_ARG, "%s: a record of %d samples", who, kb);
    if (h->stat_k > (1 << 24) - kb) return h->fail(BOD_ERR_INVALID_ARG, "%s: more than 2^24 samples in one accumulator", who);
    if (h->class_parts && h->stat_ent_k != h->stat_k)
        return h->fail(BOD_ERR_NOT_READY, "%s: ent_sum holds %d of the record's %d samples (bod_stat_merge_entropy / bod_stat_set_entropy has not followed)", who, h->stat_ent_k, h->stat_k);
    StatMergeArgs m{};
    m.BA = (int64_t)h->cfg.batch * h->A; m.C = h->cfg.num_classes; m.ka = h->stat_k; m.kb = kb;
    m.acc_cls = h->stat_acc[0]; m.acc_box = h->stat_acc[1]; m.acc_cov = h->stat_acc[2];
    m.src_cls = cls; m.src_box = box; m.src_cov = h->cfg.has_covar_head ? cov : nullptr;
    if (!cls || !box || (h->cfg.has_covar_head && !cov)) return h->fail(BOD_ERR_INVALID_ARG, "%s: NULL statistics array", who);
    if (cls == m.acc_cls || box == m.acc_box) return h->fail(BOD_ERR_INVALID_ARG, "%s: the source is the accumulator itself", who);
    if (((uintptr_t)cls | (uintptr_t)box | (uintptr_t)m.src_cov) & 15u) return h->fail(BOD_ERR_INVALID_ARG, "%s: statistics arrays must be 16-byte aligned", who);
    if (view == BOD_VIEW_HFLIP) {
        StatMirrorArgs mm{};
        mm.m = m; mm.A = h->A; mm.K = h->cfg.anchors_per_location; mm.nlev = h->nlev;
        for (int l = 0; l < h->nlev; ++l) { mm.lvl_off[l] = (int32_t)h->lvl_p0[l] * mm.K; mm.lvl_w[l] = h->lw[l]; }
        mm.lvl_off[h->nlev] = h->A;
        mm.u_flip = (float)(h->cfg.image_w - 1);
        HIPCHK(h, launch_stat_merge_mirror(mm, h->stream));
    } else {
        HIPCHK(h, launch_stat_merge(m, h->stream));
    }
    h->stat_k += kb;
    return BOD_OK;
}

// The record's fourth array on BOD_PARTS_CLASS handles: stat_ent (+)= ent_sum (acc + src whatever the sample counts; a copy into an
// accumulator that holds none), read through the mirror map for BOD_VIEW_HFLIP.  It follows the stat_fold of the same record and
// brings stat_ent_k level with stat_k.
static bod_status stat_fold_entropy(bod_handle h, const char* who, const float* ent, int32_t view = BOD_VIEW_IDENTITY) {
    if (!ent) return h->fail(BOD_ERR_INVALID_ARG, "%s: ent_sum is NULL", who);
    if (ent == h->stat_ent) return h->fail(BOD_ERR_INVALID_ARG, "%s: the source is the accumulator itself", who);
    if ((uintptr_t)ent & 15u) return h->fail(BOD_ERR_INVALID_ARG, "%s: ent_sum must be 16-byte aligned", who);
    if (h->stat_ent_k >= h->stat_k) return h->fail(BOD_ERR_NOT_READY, "%s: ent_sum already holds the record's %d samples (fold the three arrays first)", who, h->stat_k);
    const int64_t BA = (int64_t)h->cfg.batch * h->A;
    if (view == BOD_VIEW_HFLIP) {
        StatMirrorArgs mm{};
        mm.A = h->A; mm.K = h->cfg.anchors_per_location; mm.nlev = h->nlev;
        for (int l = 0; l < h->nlev; ++l) { mm.lvl_off[l] = (int32_t)h->lvl_p0[l] * mm.K; mm.lvl_w[l] = h->lw[l]; }
        mm.lvl_off[h->nlev] = h->A;
        HIPCHK(h, launch_stat_merge_entropy(h->stat_ent, ent, BA, h->stat_ent_k == 0, &mm, h->stream));
    } else {
        HIPCHK(h, launch_stat_merge_entropy(h->stat_ent, ent, BA, h->stat_ent_k == 0, nullptr, h->stream));
    }
    h->stat_ent_k = h->stat_k;
    return BOD_OK;
}

bod_status bod_stat_reset(bod_handle h) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(stat_handle(h, "bod_stat_reset"));
    h->stat_k = 0; h->stat_ent_k = 0;
    return BOD_OK;
}

static bod_status stat_forward_view(bod_handle h, const char* who, const float* images, int32_t on_device, uint64_t seed, uint32_t first_image_id,
                                    int32_t sample_base, int32_t view) {
    MarkerRange mr_api("bod:stat_forward");
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(stat_handle(h, who));
    if (!h->weights_ready) return h->fail(BOD_ERR_NOT_READY, "weights not finalized");
    if (!h->anchors_ready) return h->fail(BOD_ERR_NOT_READY, "bod_set_anchors has not been called (the box statistics are those of the decoded boxes)");
    const bod_config& c = h->cfg;
    const int n = c.mc_samples;
    if (sample_base < 0 || sample_base + n > 65535 || (c.mc_ensemble_size > 0 && sample_base + n > c.mc_ensemble_size))
        return h->fail(BOD_ERR_INVALID_ARG, "%s: sample_base=%d / mc_samples=%d / mc_ensemble_size=%d inconsistent", who, sample_base, n,
                       c.mc_ensemble_size);
    if (h->stat_k > (1 << 24) - n) return h->fail(BOD_ERR_INVALID_ARG, "%s: more than 2^24 samples in one accumulator", who);
    BODCHK(stat_view_ready(h, who, view));
    if (view == BOD_VIEW_HFLIP && !h->d_mirror) BODCHK(h->dalloc(&h->d_mirror, (size_t)c.batch * c.image_h * c.image_w * 3, false));
    const float* dev = nullptr;
    BODCHK(stage_images(h, images, on_device, &dev));
    if (view == BOD_VIEW_HFLIP) {                          // the source buffer stays as it is; a ragged upload's factors (kscale_now) stay in force
        HIPCHK(h, launch_mirror_images(dev, h->d_mirror, c.batch, c.image_h, c.image_w, h->stream));
        dev = h->d_mirror;
    }
    h->cur_images = dev;
    const int flavour = h->agg_plan ? FLAVOUR_AGG : FLAVOUR_RAW;
    const int32_t base = c.mc_sample_base;
    h->cfg.mc_sample_base = sample_base;                  // (the forward reads it per launch: ConvArgs.sample_base)
    const bod_status st = run_forward(h, dev, seed, first_image_id, flavour);
    h->cfg.mc_sample_base = base;
    BODCHK(st);
    if (flavour == FLAVOUR_RAW) {                          // no aggregating plan (n = 1, small geometries, fp32): the same reduction from raw[]
        StatRawArgs r{};
        r.B = c.batch; r.N = n; r.A = h->A; r.C = c.num_classes;
        r.cls = h->raw[0]; r.box = h->raw[1]; r.cov = c.has_covar_head ? h->raw[2] : nullptr; r.anchors = h->d_anchors;
        r.cls_sum = h->agg[0]; r.box_moments = h->agg[1]; r.cov_sum = c.has_covar_head ? h->agg[2] : nullptr;
        r.ent_sum = h->ent;                               // nullptr without BOD_PARTS_CLASS
        HIPCHK(h, launch_stat_from_raw(r, h->stream));
    }
    BODCHK(stat_fold(h, who, h->agg[0], h->agg[1], h->agg[2], n, view));
    if (h->class_parts) BODCHK(stat_fold_entropy(h, who, h->ent, view));
    return BOD_OK;
}

bod_status bod_stat_forward(bod_handle h, const float* images, int32_t on_device, uint64_t seed, uint32_t first_image_id, int32_t sample_base) {
    return stat_forward_view(h, "bod_stat_forward", images, on_device, seed, first_image_id, sample_base, BOD_VIEW_IDENTITY);
}

bod_status bod_stat_forward_view(bod_handle h, const float* images, int32_t on_device, uint64_t seed, uint32_t first_image_id, int32_t sample_base,
                                 int32_t view) {
    return stat_forward_view(h, "bod_stat_forward_view", images, on_device, seed, first_image_id, sample_base, view);
}

bod_status bod_stat_merge_from(bod_handle dst, bod_handle src) {
    if (!dst) return BOD_ERR_INVALID_ARG;
    if (!src) return dst->fail(BOD_ERR_INVALID_ARG, "bod_stat_merge_from: src is NULL");
    if (src == dst) return dst->fail(BOD_ERR_INVALID_ARG, "bod_stat_merge_from: src and dst are the same handle");
    if (!src->cfg.mc_statistics) return dst->fail(BOD_ERR_INVALID_ARG, "bod_stat_merge_from: src was not created with mc_statistics = 1");
    const bod_config& a = dst->cfg; const bod_config& b = src->cfg;
    const char* field = a.device != b.device ? "device" : a.batch != b.batch ? "batch" : dst->A != src->A ? "num_anchors" :
                        a.num_classes != b.num_classes ? "num_classes" : a.has_covar_head != b.has_covar_head ? "has_covar_head" : nullptr;
    if (field) return dst->fail(BOD_ERR_INVALID_ARG, "bod_stat_merge_from: the handles differ in %s", field);
    if (dst->class_parts && !src->class_parts)
        return dst->fail(BOD_ERR_INVALID_ARG, "bod_stat_merge_from: src carries no ent_sum (it was created without BOD_PARTS_CLASS in covariance_parts, dst with it)");
    BODCHK(stat_handle(dst, "bod_stat_merge_from"));
    if (src->stat_k == 0) return BOD_OK;
    if (stat_handle(src, "bod_stat_merge_from") != BOD_OK) return dst->fail(BOD_ERR_HIP, "bod_stat_merge_from: src: %s", src->err.c_str());
    if (dst->class_parts && (src->stat_ent_k != src->stat_k || dst->stat_ent_k != dst->stat_k))
        return dst->fail(BOD_ERR_NOT_READY, "bod_stat_merge_from: ent_sum is behind its record (src %d of %d samples, dst %d of %d)", src->stat_ent_k, src->stat_k,
                         dst->stat_ent_k, dst->stat_k);
    HIPCHK(dst, hipEventRecord(src->ev_stat, src->stream));              // src's accumulator is complete ...
    HIPCHK(dst, hipStreamWaitEvent(dst->stream, src->ev_stat, 0));
    BODCHK(stat_fold(dst, "bod_stat_merge_from", src->stat_acc[0], src->stat_acc[1], src->stat_acc[2], src->stat_k));
    if (dst->class_parts) BODCHK(stat_fold_entropy(dst, "bod_stat_merge_from", src->stat_ent));
    HIPCHK(dst, hipEventRecord(dst->ev_stat, dst->stream));              // ... and is not rewritten before the merge has read it
    HIPCHK(dst, hipStreamWaitEvent(src->stream, dst->ev_stat, 0));
    return BOD_OK;
}

bod_status bod_stat_merge(bod_handle h, const void* const* ptrs3, int32_t samples) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(stat_handle(h, "bod_stat_merge"));
    if (!ptrs3) return h->fail(BOD_ERR_INVALID_ARG, "bod_stat_merge: ptrs3 is NULL");
    return stat_fold(h, "bod_stat_merge", static_cast<const float*>(ptrs3[0]), static_cast<const float*>(ptrs3[1]),
                     static_cast<const float*>(ptrs3[2]), samples);
}

bod_status bod_stat_merge_view(bod_handle h, const void* const* ptrs3, int32_t samples, int32_t view) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(stat_handle(h, "bod_stat_merge_view"));
    if (!ptrs3) return h->fail(BOD_ERR_INVALID_ARG, "bod_stat_merge_view: ptrs3 is NULL");
    BODCHK(stat_view_ready(h, "bod_stat_merge_view", view));
    return stat_fold(h, "bod_stat_merge_view", static_cast<const float*>(ptrs3[0]), static_cast<const float*>(ptrs3[1]),
                     static_cast<const float*>(ptrs3[2]), samples, view);
}

bod_status bod_stat_device(bod_handle h, void** ptrs3, int32_t* samples) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(stat_handle(h, "bod_stat_device"));
    if (ptrs3) { ptrs3[0] = h->stat_acc[0]; ptrs3[1] = h->stat_acc[1]; ptrs3[2] = h->cfg.has_covar_head ? h->stat_acc[2] : nullptr; }
    if (samples) *samples = h->stat_k;
    return BOD_OK;
}

bod_status bod_stat_get(bod_handle h, float* cls_sum, float* box_moments, float* cov_sum, int32_t* samples) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(stat_handle(h, "bod_stat_get"));
    if (cov_sum && !h->cfg.has_covar_head) return h->fail(BOD_ERR_INVALID_ARG, "model has no covariance head");
    const size_t BA = (size_t)h->cfg.batch * h->A;
    BODCHK(d2h(h, cls_sum, h->stat_acc[0], BA * h->cfg.num_classes));
    BODCHK(d2h(h, box_moments, h->stat_acc[1], BA * 16));
    BODCHK(d2h(h, cov_sum, h->stat_acc[2], BA * 10));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (samples) *samples = h->stat_k;
    return BOD_OK;
}

bod_status bod_stat_set(bod_handle h, const float* cls_sum, const float* box_moments, const float* cov_sum, int32_t samples) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(stat_handle(h, "bod_stat_set"));
    if (samples < 0 || samples > (1 << 24)) return h->fail(BOD_ERR_INVALID_ARG, "bod_stat_set: samples = %d", samples);
    if (cov_sum && !h->cfg.has_covar_head) return h->fail(BOD_ERR_INVALID_ARG, "model has no covariance head");
    const size_t BA = (size_t)h->cfg.batch * h->A;
    if (cls_sum) HIPCHK(h, hipMemcpyAsync(h->stat_acc[0], cls_sum, BA * h->cfg.num_classes * 4, hipMemcpyHostToDevice, h->stream));
    if (box_moments) HIPCHK(h, hipMemcpyAsync(h->stat_acc[1], box_moments, BA * 64, hipMemcpyHostToDevice, h->stream));
    if (cov_sum) HIPCHK(h, hipMemcpyAsync(h->stat_acc[2], cov_sum, BA * 40, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->stat_k = samples;
    h->stat_ent_k = 0;                                    // BOD_PARTS_CLASS handles: bod_stat_set_entropy follows
    return BOD_OK;
}

bod_status bod_stat_merge_entropy(bod_handle h, const void* ent_sum, int32_t view) {
    BODCHK(class_parts_handle(h, "bod_stat_merge_entropy"));
    BODCHK(stat_handle(h, "bod_stat_merge_entropy"));
    BODCHK(stat_view_ready(h, "bod_stat_merge_entropy", view));
    return stat_fold_entropy(h, "bod_stat_merge_entropy", static_cast<const float*>(ent_sum), view);
}

bod_status bod_stat_device_entropy(bod_handle h, void** ptr) {
    BODCHK(class_parts_handle(h, "bod_stat_device_entropy"));
    BODCHK(stat_handle(h, "bod_stat_device_entropy"));
    if (!ptr) return h->fail(BOD_ERR_INVALID_ARG, "bod_stat_device_entropy: ptr is NULL");
    *ptr = h->stat_ent;
    return BOD_OK;
}

bod_status bod_stat_get_entropy(bod_handle h, float* ent_sum) {
    BODCHK(class_parts_handle(h, "bod_stat_get_entropy"));
    BODCHK(stat_handle(h, "bod_stat_get_entropy"));
    if (h->stat_ent_k != h->stat_k)
        return h->fail(BOD_ERR_NOT_READY, "bod_stat_get_entropy: ent_sum holds %d of the record's %d samples", h->stat_ent_k, h->stat_k);
    BODCHK(d2h(h, ent_sum, h->stat_ent, (size_t)h->cfg.batch * h->A));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BOD_OK;
}

bod_status bod_stat_set_entropy(bod_handle h, const float* ent_sum) {
    BODCHK(class_parts_handle(h, "bod_stat_set_entropy"));
    BODCHK(stat_handle(h, "bod_stat_set_entropy"));
    if (!ent_sum) return h->fail(BOD_ERR_INVALID_ARG, "bod_stat_set_entropy: ent_sum is NULL");
    HIPCHK(h, hipMemcpyAsync(h->stat_ent, ent_sum, (size_t)h->cfg.batch * h->A * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->stat_ent_k = h->stat_k;
    return BOD_OK;
}

bod_status bod_stat_posterior(bod_handle h, uint64_t seed, uint32_t first_image_id) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(stat_handle(h, "bod_stat_posterior"));
    if (h->stat_k < 2) return h->fail(BOD_ERR_NOT_READY, "bod_stat_posterior: the accumulator holds %d samples; bayes_od needs >= 2 (sample covariance divides by N-1)", h->stat_k);
    if (h->class_parts && h->stat_ent_k != h->stat_k)
        return h->fail(BOD_ERR_NOT_READY, "bod_stat_posterior: ent_sum holds %d of the record's %d samples (bod_stat_merge_entropy / bod_stat_set_entropy has not followed)", h->stat_ent_k, h->stat_k);
    if (!h->anchors_ready) return h->fail(BOD_ERR_NOT_READY, "bod_set_anchors has not been called");
    BODCHK(wait_pending_slots(h, h->stream));
    MarkerRange mr("bod:posterior");
    PostCfg pc = post_cfg(h, seed, first_image_id);
    pc.N = h->stat_k;                                    // the merged sample count
    pc.aggregated = 1;
    PostBuffers pb = h->pb;
    pb.cls = nullptr; pb.box = nullptr; pb.cov = nullptr; pb.anchors = h->d_anchors;
    pb.agg_cls = h->stat_acc[0]; pb.agg_box = h->stat_acc[1]; pb.agg_cov = h->stat_acc[2];
    h->keep_ready = false;                               // the keep flags are rewritten
    HIPCHK(h, launch_posterior(pc, pb, h->stream));
    if (h->parts) { HIPCHK(h, launch_posterior_parts(pc, pb, h->parts, h->stream)); std::fill(h->parts_ok.begin(), h->parts_ok.end(), 1); }
    if (h->cparts) { HIPCHK(h, launch_posterior_class_parts(pc, pb, h->stat_ent, h->cparts, h->stream)); std::fill(h->cparts_ok.begin(), h->cparts_ok.end(), 1); }
    if (h->cfg.ranking_method == BOD_RANK_JOINT_ENTROPY && h->cfg.gaussian_isotropic && h->cfg.dirichlet_non_informative)
        HIPCHK(h, launch_joint_entropy_rank(pc, pb, h->stream));
    h->stage.posterior_ran();
    return BOD_OK;
}

// Acquisition scores of the accumulator (include/bayesod.h; acq_kernels.hip): reads the record, writes buffers of its own
bod_status bod_stat_acquisition(bod_handle h, const bod_acquisition_options* opt, double* frame_scores, double* per_class) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(stat_handle(h, "bod_stat_acquisition"));
    const bod_acquisition_options o = opt ? *opt : bod_acquisition_options{0.05f, 16, {0, 0}};
    if (!(o.min_foreground >= 0.f && o.min_foreground <= 1.f))
        return h->fail(BOD_ERR_INVALID_ARG, "bod_stat_acquisition: min_foreground must lie in [0, 1], got %g", (double)o.min_foreground);
    if (o.top_k < 1 || o.top_k > 1024) return h->fail(BOD_ERR_INVALID_ARG, "bod_stat_acquisition: top_k must lie in 1..1024, got %d", o.top_k);
    if (o.reserved[0] != 0 || o.reserved[1] != 0) return h->fail(BOD_ERR_INVALID_ARG, "bod_stat_acquisition: reserved fields must be 0");
    if (!frame_scores) return h->fail(BOD_ERR_INVALID_ARG, "bod_stat_acquisition: frame_scores is NULL");
    const bod_config& c = h->cfg;
    if (c.num_classes != 4 && c.num_classes != 8) return h->fail(BOD_ERR_INVALID_ARG, "bod_stat_acquisition: num_classes must be 4 or 8, got %d", c.num_classes);
    if (h->stat_k < 2) return h->fail(BOD_ERR_NOT_READY, "bod_stat_acquisition: the accumulator holds %d samples; the box spread divides by K-1", h->stat_k);
    if (h->class_parts && h->stat_ent_k != h->stat_k)
        return h->fail(BOD_ERR_NOT_READY, "bod_stat_acquisition: ent_sum holds %d of the record's %d samples (bod_stat_merge_entropy / bod_stat_set_entropy has not followed)", h->stat_ent_k, h->stat_k);
    const size_t B = (size_t)c.batch, npc = (size_t)(c.num_classes - 1) * 3;
    const int G = acq_groups(h->A);
    if (!h->acq_partials) BODCHK(h->dalloc(&h->acq_partials, B * G * ACQ_ROW_MAX));      // (each on its own: a failed call allocates nothing twice)
    if (!h->acq_out) BODCHK(h->dalloc(&h->acq_out, B * (12 + npc)));
    if (!h->acq_mi) BODCHK(h->dalloc(&h->acq_mi, B * h->A));
    MarkerRange mr("bod:acquisition");
    AcqArgs a{};
    a.B = c.batch; a.A = h->A; a.C = c.num_classes; a.K = h->stat_k; a.G = G; a.top_k = o.top_k;
    a.thr = (float)((1.0 - (double)o.min_foreground) * (double)h->stat_k);
    a.cls_sum = h->stat_acc[0]; a.box_moments = h->stat_acc[1]; a.cov_sum = c.has_covar_head ? h->stat_acc[2] : nullptr;
    a.ent_sum = h->class_parts ? h->stat_ent : nullptr;
    a.mi = h->acq_mi; a.partials = h->acq_partials; a.scores = h->acq_out; a.per_class = h->acq_out + B * 12;
    HIPCHK(h, launch_acquisition(a, h->stream));
    h->acq_ran = true;
    BODCHK(d2h(h, frame_scores, h->acq_out, B * 12));
    BODCHK(d2h(h, per_class, h->acq_out + B * 12, B * npc));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BOD_OK;
}

bod_status bod_stat_acquisition_map(bod_handle h, float* mi) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(stat_handle(h, "bod_stat_acquisition_map"));
    if (!mi) return h->fail(BOD_ERR_INVALID_ARG, "bod_stat_acquisition_map: mi is NULL");
    if (!h->acq_ran) return h->fail(BOD_ERR_NOT_READY, "bod_stat_acquisition_map: bod_stat_acquisition has not been called");
    BODCHK(d2h(h, mi, h->acq_mi, (size_t)h->cfg.batch * h->A));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BOD_OK;
}

bod_status bod_profile_select(bod_handle h, int32_t which) {
    if (!h) return BOD_ERR_INVALID_ARG;
    if (which < 0 || which > 2) return h->fail(BOD_ERR_INVALID_ARG, "bod_profile_select: %d", which);
    h->prof_which = which;
    return BOD_OK;
}

bod_status bod_profile_end(bod_handle h, double* head_ms, int64_t* head_launches, double* head_flops, double* post_ms, int64_t* post_launches) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    double hm = 0, pm = 0;
    for (auto& e : h->ev_head) { float ms = 0; HIPCHK(h, hipEventElapsedTime(&ms, e.first, e.second)); hm += ms; }
    for (auto& e : h->ev_post) { float ms = 0; HIPCHK(h, hipEventElapsedTime(&ms, e.first, e.second)); pm += ms; }
    if (head_ms) *head_ms = hm;
    if (head_launches) *head_launches = (int64_t)h->ev_head.size();
    if (head_flops) *head_flops = h->prof_flops;
    if (post_ms) *post_ms = pm;
    if (post_launches) *post_launches = (int64_t)h->ev_post.size();
    h->profiling = false;
    return BOD_OK;
}

}  // extern "C"

#include "validate_impl.inc"
#include "train_impl.inc"
#include "upload_impl.inc"

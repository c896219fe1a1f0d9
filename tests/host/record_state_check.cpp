// CPU check of bayes-od-rc_amd/csrc/record_state.h, compiled with -fsanitize=address,undefined by tests/test_host_record_state.py.
//   1. RecordLayout / record_fields against the literal formulas the engine used to spell out at every use: C in {2, 4, 8}, B in
//      {1, 3}, K in {1, 5}, both optional tails on and off;
//   2. StageState against a four-bool restatement of the transition table, over every event sequence up to length 5 from the
//      initial state -- including a save / forward / restore (what materialise_raw does) as one event;
//   3. zero_rows_past_count for counts -1, 0, 1, K, K + 3 on heap buffers of exactly B * K * width elements (the sanitizer sees a
//      write outside them);
//   4. conv_out_geometry for planes 1..9 x 1..9, kernels 1..3 x 1..3, strides 1 and 2, SAME and VALID, empty outputs included.
#include "record_state.h"
#include <cstdio>
#include <vector>

static int failures = 0;
static long cases = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } } } while (0)

// ---- 1
static void check_layout(size_t B, size_t K, int C, bool parts, bool cparts) {
    ++cases;
    const RecordLayout L(B, K, C, parts, cparts);
    const size_t BK = B * K;
    const size_t want[RecordLayout::SEGS] = {B * 4, BK * C * 4, BK * 16, BK * 64, BK * C * 4, parts ? BK * 192 : 0, cparts ? BK * 16 : 0};
    size_t at = 0;
    for (int s = 0; s < RecordLayout::SEGS; ++s) {
        CHECK(L.off[s] == at, "B=%zu K=%zu C=%d %d%d: segment %d starts at %zu, expected %zu", B, K, C, parts, cparts, s, L.off[s], at);
        CHECK(L.bytes((RecordLayout::Seg)s) == want[s], "segment %d has %zu bytes, expected %zu", s, L.bytes((RecordLayout::Seg)s), want[s]);
        CHECK(L.off[s + 1] >= L.off[s], "segment %d ends in front of its start", s);
        at += want[s];
    }
    CHECK(L.total() == (B + BK * (2 * (size_t)C + 20 + (parts ? 48 : 0) + (cparts ? 4 : 0))) * 4, "total %zu", L.total());
    // the offsets bod_collect_parts / bod_collect_class_parts used to compute on their own
    CHECK(L.off[RecordLayout::PARTS] == (B + BK * (2 * (size_t)C + 20)) * 4, "parts at %zu", L.off[RecordLayout::PARTS]);
    CHECK(L.off[RecordLayout::CPARTS] == (B + BK * (2 * (size_t)C + 20 + (parts ? 48 : 0))) * 4, "class parts at %zu", L.off[RecordLayout::CPARTS]);
    const RecordFields& f = L.fields;
    CHECK(f.width == 21 + 2 * C + (parts ? 48 : 0) + (cparts ? 4 : 0), "record width %d", f.width);
    CHECK(f.mean == 1 && f.cov == 5 && f.score == 21 && f.count == 21 + C && f.parts == 21 + 2 * C && f.cparts == 21 + 2 * C + (parts ? 48 : 0),
          "field offsets %d %d %d %d %d %d", f.mean, f.cov, f.score, f.count, f.parts, f.cparts);
}

// ---- 2
enum Event { FORWARD, POSTERIOR, NMS, CLUSTER, PARTS_SET, AFFINITY_SET, MATERIALISE, EVENTS };
struct Ref { bool forward_done = false, posterior_done = false, nms_done = false, cluster_done = false; int affinity_img = -1; };

static void apply(Ref& r, Event e) {
    switch (e) {
        case FORWARD: r.forward_done = true; r.posterior_done = r.nms_done = r.cluster_done = false; r.affinity_img = -1; break;
        case POSTERIOR: r.posterior_done = true; r.nms_done = r.cluster_done = false; r.affinity_img = -1; break;
        case NMS: r.nms_done = true; r.cluster_done = false; r.affinity_img = -1; break;
        case CLUSTER: r.affinity_img = -1; r.cluster_done = true; break;
        case PARTS_SET: r.cluster_done = false; break;
        case AFFINITY_SET: r.affinity_img = 1; break;
        case MATERIALISE: {
            const bool fd = r.forward_done, pd = r.posterior_done, nd = r.nms_done, cd = r.cluster_done;
            const int aff = r.affinity_img;
            apply(r, FORWARD);
            r.forward_done = fd; r.posterior_done = pd; r.nms_done = nd; r.cluster_done = cd; r.affinity_img = aff;
            break;
        }
        default: break;
    }
}
static void apply(StageState& s, Event e) {
    switch (e) {
        case FORWARD: s.forward_ran(); break;
        case POSTERIOR: s.posterior_ran(); break;
        case NMS: s.nms_ran(); break;
        case CLUSTER: s.cluster_ran(); break;
        case PARTS_SET: s.parts_set(); break;
        case AFFINITY_SET: s.affinity_set(1); break;
        case MATERIALISE: { const StageState saved = s; s.forward_ran(); s = saved; break; }
        default: break;
    }
}
static void walk(const StageState& s, const Ref& r, int depth) {
    if (depth == 0) return;
    for (int e = 0; e < EVENTS; ++e) {
        ++cases;
        StageState s2 = s;
        Ref r2 = r;
        apply(s2, (Event)e);
        apply(r2, (Event)e);
        CHECK(s2.forward == r2.forward_done && s2.posterior == r2.posterior_done && s2.nms == r2.nms_done && s2.cluster == r2.cluster_done &&
              s2.affinity_img == r2.affinity_img, "event %d at depth %d: %d%d%d%d %d against %d%d%d%d %d", e, depth, s2.forward, s2.posterior,
              s2.nms, s2.cluster, s2.affinity_img, r2.forward_done, r2.posterior_done, r2.nms_done, r2.cluster_done, r2.affinity_img);
        walk(s2, r2, depth - 1);
    }
}

// ---- 3
template <typename T>
static void check_zero_rows(size_t B, size_t K, size_t width, int rot) {
    ++cases;
    const int32_t counts[5] = {-1, 0, 1, (int32_t)K, (int32_t)K + 3};
    std::vector<int32_t> num(B);
    for (size_t b = 0; b < B; ++b) num[b] = counts[(b + rot) % 5];
    std::vector<T> rows(B * K * width);
    for (size_t i = 0; i < rows.size(); ++i) rows[i] = (T)(i + 1);
    zero_rows_past_count(rows.data(), num.data(), B, K, width);
    for (size_t b = 0; b < B; ++b) {
        const size_t k0 = num[b] < 0 ? 0 : (size_t)num[b] > K ? K : (size_t)num[b];
        for (size_t k = 0; k < K; ++k)
            for (size_t q = 0; q < width; ++q) {
                const size_t i = (b * K + k) * width + q;
                CHECK(rows[i] == (k < k0 ? (T)(i + 1) : (T)0), "count %d K %zu: row %zu of image %zu, element %zu", num[b], K, k, b, q);
            }
    }
    zero_rows_past_count((T*)nullptr, num.data(), B, K, width);            // a caller's NULL array: nothing to do
}

// ---- 4
static void check_geometry(int H, int W, int KH, int KW, int stride, bool same) {
    ++cases;
    int OH, OW, oy = 1, ox = 1;                                            // bod_stage_conv's block, as it stood
    if (same) {
        OH = (H + stride - 1) / stride; OW = (W + stride - 1) / stride;
        const int out_h = (H + stride - 1) / stride, out_w = (W + stride - 1) / stride;
        const int th = (out_h - 1) * stride + KH - H, tw = (out_w - 1) * stride + KW - W;
        oy = 1 - (th > 0 ? th : 0) / 2; ox = 1 - (tw > 0 ? tw : 0) / 2;
    } else {
        OH = (H - KH) / stride + 1; OW = (W - KW) / stride + 1;
    }
    int gh = -99, gw = -99, gy = -99, gx = -99;
    conv_out_geometry(H, W, KH, KW, stride, same, &gh, &gw, &gy, &gx);
    CHECK(gh == OH && gw == OW && gy == oy && gx == ox, "%dx%d k %dx%d s %d same %d: %d %d %d %d, expected %d %d %d %d", H, W, KH, KW, stride,
          same, gh, gw, gy, gx, OH, OW, oy, ox);
    if (same) CHECK(same_pad_before(H, KH, stride) == 1 - oy && same_pad_before(W, KW, stride) == 1 - ox, "same_pad_before");
}

int main() {
    long empty = 0;
    for (int C : {2, 4, 8})
        for (size_t B : {1, 3})
            for (size_t K : {1, 5})
                for (int tails = 0; tails < 4; ++tails) check_layout(B, K, C, tails & 1, tails & 2);
    static_assert(record_fields(8, true, true).width == 89 && record_fields(4, false, false).width == 29, "constexpr for the pack kernel");
    walk(StageState(), Ref(), 5);
    {   // bod_set_posterior on a handle that never ran a forward: the posterior is there, the forward is not
        StageState s;
        s.posterior_ran();
        ++cases;
        CHECK(!s.forward && s.posterior && !s.nms && !s.cluster && s.affinity_img == -1, "set-posterior without a forward");
    }
    for (size_t K : {1, 4})
        for (int rot = 0; rot < 5; ++rot) {
            check_zero_rows<float>(3, K, 4, rot);
            check_zero_rows<float>(5, K, 16, rot);
            check_zero_rows<int32_t>(3, K, 1, rot);
        }
    for (int H = 1; H <= 9; ++H)
        for (int W = 1; W <= 9; ++W)
            for (int KH = 1; KH <= 3; ++KH)
                for (int KW = 1; KW <= 3; ++KW)
                    for (int stride = 1; stride <= 2; ++stride)
                        for (int same = 0; same < 2; ++same) {
                            check_geometry(H, W, KH, KW, stride, same != 0);
                            int OH, OW, oy, ox;
                            conv_out_geometry(H, W, KH, KW, stride, same != 0, &OH, &OW, &oy, &ox);
                            if (OH < 1 || OW < 1) ++empty;
                        }
    CHECK(empty > 0, "no shape with an empty output was checked");
    std::printf("record_state_check: %ld cases (%ld with an empty output), %d failures\n", cases, empty, failures);
    return failures ? 1 : 0;
}

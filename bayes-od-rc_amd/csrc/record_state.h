// Host bookkeeping of the post-processing stages that needs no GPU to be checked (tests/host/record_state_check.cpp builds it with
// plain g++ under the sanitizers): where a detection record's fields lie, which stage of a handle has run, the zero rows behind an
// image's detection count, and the output geometry of a convolution on a zero-bordered plane.  No HIP include.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

// ---- detection records ---------------------------------------------------------------------------------------------------------
// A detection is [valid, mean (v,u,h,w), covariance row-major, score[C], counts[C]], then the three covariance parts (handles with
// BOD_PARTS_COVARIANCE) and the four class-entropy parts (BOD_PARTS_CLASS).  These widths and this order are stated here only.
constexpr int REC_MEAN = 4, REC_COV = 16, REC_PARTS = 48, REC_CPARTS = 4;

// Float offsets of the fields in a packed row (bod_gather_detections, distributed.pack_records); constexpr, so that the pack kernel
// takes them from here too.
struct RecordFields { int mean, cov, score, count, parts, cparts, width; };
constexpr RecordFields record_fields(int C, bool has_cov_parts, bool has_class_parts) {
    RecordFields f{};
    f.mean = 1;
    f.cov = f.mean + REC_MEAN;
    f.score = f.cov + REC_COV;
    f.count = f.score + C;
    f.parts = f.count + C;
    f.cparts = f.parts + (has_cov_parts ? REC_PARTS : 0);
    f.width = f.cparts + (has_class_parts ? REC_CPARTS : 0);
    return f;
}

// The pinned staging buffer of a record slot: num [B] | scores | means | covs | counts | parts? | cparts? ([B,K,.] each), in bytes.
struct RecordLayout {
    enum Seg { NUM = 0, SCORES, MEANS, COVS, COUNTS, PARTS, CPARTS, SEGS };
    size_t off[SEGS + 1];              // off[SEGS] = total; an absent tail has no bytes
    RecordFields fields;
    RecordLayout(size_t B, size_t K, int C, bool has_cov_parts, bool has_class_parts) : fields(record_fields(C, has_cov_parts, has_class_parts)) {
        const size_t BK = B * K;
        const size_t floats[SEGS] = {B, BK * (size_t)C, BK * REC_MEAN, BK * REC_COV, BK * (size_t)C, has_cov_parts ? BK * REC_PARTS : 0,
                                     has_class_parts ? BK * REC_CPARTS : 0};
        off[0] = 0;
        for (int s = 0; s < SEGS; ++s) off[s + 1] = off[s] + floats[s] * 4;
    }
    size_t bytes(Seg s) const { return off[s + 1] - off[s]; }
    size_t total() const { return off[SEGS]; }
};

// Rows behind an image's detection count are whatever an earlier batch left: zero them on the way out.  rows [B][K][width];
// a count below 0 counts as 0, one above K as K.
template <typename T>
void zero_rows_past_count(T* rows, const int32_t* num, size_t B, size_t K, size_t width) {
    for (size_t b = 0; rows && b < B; ++b) {
        const size_t k0 = (size_t)std::min<int64_t>(std::max<int64_t>(num[b], 0), (int64_t)K);
        std::fill(rows + (b * K + k0) * width, rows + (b + 1) * K * width, T(0));
    }
}

// ---- which stage has run ------------------------------------------------------------------------------------------------------
// posterior -> nms -> cluster is a chain: an event takes away everything behind it.  The forward is not part of it: bod_set_posterior
// on a handle that never ran one leaves `forward` false.  affinity_img: the image bod_set_affinity left columns for (-1: none).
struct StageState {
    bool forward = false, posterior = false, nms = false, cluster = false;
    int affinity_img = -1;
    void forward_ran() { forward = true; posterior = nms = cluster = false; affinity_img = -1; }      // + bod_set_raw, bod_device_raw(mark_ready)
    void posterior_ran() { posterior = true; nms = cluster = false; affinity_img = -1; }              // + bod_set_posterior, validation / statistics posteriors
    void nms_ran() { nms = true; cluster = false; affinity_img = -1; }        // + bod_set_nms.  New centres: a pending bod_set_affinity was sized for the old ones
    void cluster_ran() { cluster = true; affinity_img = -1; }                 // (the affinity is consumed)
    void parts_set() { cluster = false; }                                     // bod_set_posterior_parts / _class_parts
    void affinity_set(int img) { affinity_img = img; }
};

// ---- convolution geometry on a plane with a 1-pixel zero border ------------------------------------------------------------------
inline int same_pad_before(int in, int k, int s) {
    const int out = (in + s - 1) / s;
    const int total = std::max((out - 1) * s + k - in, 0);
    return total / 2;
}
// Output size, and the padded coordinate (oy, ox) of the window origin of output (0, 0).  An empty output has OH < 1 or OW < 1.
inline void conv_out_geometry(int H, int W, int KH, int KW, int stride, bool same, int* OH, int* OW, int* oy, int* ox) {
    *oy = 1; *ox = 1;
    if (same) {
        *OH = (H + stride - 1) / stride; *OW = (W + stride - 1) / stride;
        *oy = 1 - same_pad_before(H, KH, stride); *ox = 1 - same_pad_before(W, KW, stride);
    } else {
        *OH = (H - KH) / stride + 1; *OW = (W - KW) / stride + 1;
    }
}

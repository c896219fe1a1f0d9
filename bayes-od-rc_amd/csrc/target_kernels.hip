// Anchor-target assignment on the device: box_utils.bbox_iou_vuvu +
// FpnAnchorGenerator.positive_negative_batching + generate_anchor_targets for every (frame, anchor) of a minibatch in one
// launch.  The host code loops over pyramid levels only to concatenate; every anchor is independent, so the launch covers the
// stacked p3 -> p7 anchor array.  All arithmetic is fp32 in the host code's own order (quirks kept); the file is
// built with -ffp-contract=off and uses the correctly rounded division and the library logf, because its results are compared
// with NumPy for equality.
#include "kernels.h"
#include <math.h>

#define TGT_BLOCK 256
#define TGT_CHUNK 256          // ground-truth rows staged in LDS at a time (5 KB)

// One thread per (frame, anchor); blockIdx.y = frame.  The frame's GT rows and their area terms are staged in LDS chunk by
// chunk (any G >= 1); every lane reads the same LDS address (a broadcast).  C = 0: any class count, scalar class-row copies.
template <int C>
__global__ __launch_bounds__(TGT_BLOCK) void anchor_targets_kernel(TargetArgs a) {
    __shared__ float4 s_box[TGT_CHUNK];
    __shared__ float s_area[TGT_CHUNK];
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int an = blockIdx.x * TGT_BLOCK + tid;
    const bool valid = an < a.A;
    const int g_base = a.gt_off[b], G = a.gt_off[b + 1] - g_base;
    const float4* gt = reinterpret_cast<const float4*>(a.gt_boxes) + g_base;
    float v = 0.f, u = 0.f, h = 1.f, w = 1.f;
    if (valid) { const float4 r = reinterpret_cast<const float4*>(a.anchors)[an]; v = r.x; u = r.y; h = r.z; w = r.w; }
    const float y11 = v - h / 2.0f, x11 = u - w / 2.0f, y12 = v + h / 2.0f, x12 = u + w / 2.0f;
    const float a1 = (x11 - x12 + 1.0f) * (y11 - y12 + 1.0f);          // the reference's area expression (sign quirk kept)
    bool positive = false, negative = true;
    float best = 0.f;
    int best_j = -1;
    for (int g0 = 0; g0 < G; g0 += TGT_CHUNK) {
        const int n = min(TGT_CHUNK, G - g0);
        __syncthreads();                                               // the previous chunk has been read by every thread
        for (int i = tid; i < n; i += TGT_BLOCK) {
            const float4 r = gt[g0 + i];                               // (y21, x21, y22, x22)
            s_box[i] = r;
            s_area[i] = (r.y - r.w + 1.0f) * (r.x - r.z + 1.0f);
        }
        __syncthreads();
        if (valid) {
            for (int j = 0; j < n; ++j) {
                const float4 r = s_box[j];
                const float iw = fmaxf(fminf(x12, r.w) - fmaxf(x11, r.y) + 1.0f, 0.0f);
                const float ih = fmaxf(fminf(y12, r.z) - fmaxf(y11, r.x) + 1.0f, 0.0f);
                const float inter = iw * ih;
                const float iou = inter / ((a1 + s_area[j]) - inter + 0.00001f);
                positive = positive || (iou >= a.min_positive_iou);
                negative = negative && (iou <= a.max_negative_iou);
                if (best_j < 0 || iou > best) { best = iou; best_j = g0 + j; }      // np.argmax: the first of the largest
            }
        }
    }
    if (!valid || best_j < 0) return;
    const size_t idx = (size_t)b * a.A + an;
    const float4 r = gt[best_j];
    const float gt_v = (r.z + r.x) / 2.0f, gt_u = (r.w + r.y) / 2.0f, gt_h = r.z - r.x, gt_w = r.w - r.y;
    float4 t;
    t.x = (gt_v - v) / h * 10.0f;
    t.y = (gt_u - u) / w * 10.0f;
    t.z = logf(gt_h / h) * 5.0f;
    t.w = logf(gt_w / w) * 5.0f;
    reinterpret_cast<float4*>(a.box_t)[idx] = t;                       // written for every anchor, positive or not
    if (C > 0) {
        const float4* src = reinterpret_cast<const float4*>(a.gt_classes + (size_t)(g_base + best_j) * C);
        float4* dst = reinterpret_cast<float4*>(a.cls_t + idx * C);
#pragma unroll
        for (int q = 0; q < C / 4; ++q) {
            float4 c = make_float4(0.f, 0.f, 0.f, q == C / 4 - 1 ? 1.0f : 0.f);      // the background row (0, ..., 0, 1)
            if (positive) c = src[q];
            dst[q] = c;
        }
    } else {
        const float* src = a.gt_classes + (size_t)(g_base + best_j) * a.C;
        float* dst = a.cls_t + idx * a.C;
        for (int q = 0; q < a.C; ++q) dst[q] = positive ? src[q] : (q == a.C - 1 ? 1.0f : 0.f);
    }
    a.pos[idx] = positive ? 1 : 0;
    a.neg[idx] = negative ? 1 : 0;
    if (a.best_gt) a.best_gt[idx] = best_j;
    if (a.best_iou) a.best_iou[idx] = best;
}

hipError_t launch_anchor_targets(const TargetArgs& a, hipStream_t s) {
    if (a.A < 1 || a.B < 1 || a.B > 65535 || a.C < 2) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.A + TGT_BLOCK - 1) / TGT_BLOCK), (unsigned)a.B);
    if (a.C == 8) hipLaunchKernelGGL(anchor_targets_kernel<8>, grid, dim3(TGT_BLOCK), 0, s, a);
    else if (a.C == 4) hipLaunchKernelGGL(anchor_targets_kernel<4>, grid, dim3(TGT_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(anchor_targets_kernel<0>, grid, dim3(TGT_BLOCK), 0, s, a);
    return hipGetLastError();
}

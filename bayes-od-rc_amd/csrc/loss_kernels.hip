// Training-loss FORWARD on the device (BASELINE config 5):
// RetinaNetModel.get_loss for 'classification' (softmax focal loss, src/core/losses.py:30-61),
// 'regression' (Huber), 'regression_var' / 'regression_covar'
// (src/retina_net/models/retinanet_model.py:183-323).  One thread per (image, anchor); block partial
// sums are written out and added on the host in double, so the result is run-to-run deterministic.
// 'regression_nll' (reg_kind 4) is one more branch of that thread; 'regression_energy' (reg_kind 5) has kernels of its own at the
// end of this file (one wave per positive row) and hands its per-row term to the same block sums.
#include "kernels.h"
#include "philox.h"
#include <math.h>

#define LOSS_BLOCK 256

__device__ __forceinline__ float huber1(float e) {
    const float a = fabsf(e);
    return a <= 1.0f ? 0.5f * e * e : a - 0.5f;
}

// The four terms of one (frame, anchor): idx = frame * A + an.  The ONE implementation of the per-anchor loss arithmetic: the
// whole-batch launch (loss_kernel) and the per-frame launch of the validation route (loss_frames_kernel) both call it.
// PROPER = the instantiation that also knows reg_kind 4 / 5 (launched for those two alone): kinds 0-3 run the code they ran before.
template <int C, bool PROPER>
__device__ __forceinline__ void loss_anchor_terms(const LossArgs& a, long long idx, int an, float& s_cls, float& s_cmp, float& s_reg,
                                                  float& s_pos) {
    const float pos = a.pos[idx] ? 1.f : 0.f, neg = a.neg[idx] ? 1.f : 0.f;
    s_pos = pos;
    if (a.do_cls && (pos + neg) > 0.f) {
        const float* x = a.cls + idx * C;
        const float* y = a.cls_t + idx * C;
        float v[C], mx = x[0];
#pragma unroll
        for (int j = 0; j < C; ++j) { v[j] = x[j]; mx = fmaxf(mx, v[j]); }
        float se = 0.f;
#pragma unroll
        for (int j = 0; j < C; ++j) se += expf(v[j] - mx);
        const float lse = logf(se);
        float pt = 0.f, ce = 0.f;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const float ls = v[j] - mx - lse;
            pt += expf(ls) * y[j];
            ce -= (y[j] * (1.0f - a.label_smoothing) + a.label_smoothing / (float)C) * ls;
        }
        const float ngm = y[C - 1];
        const float alpha = 0.5f * (1.0f - ngm) + 0.5f * ngm;
        const float f = 1.0f - pt;
        s_cls = alpha * f * f * ce * (pos + neg);
    }
    if (PROPER && a.reg_kind == 5) {                             // energy score: the row's term comes from energy_forward_kernel
        if (pos > 0.f) s_cmp = a.row_term[idx];
    } else if (a.reg_kind && pos > 0.f) {
        const float4 p = reinterpret_cast<const float4*>(a.box)[idx];
        const float4 t = reinterpret_cast<const float4*>(a.box_t)[idx];
        if (a.reg_kind == 1) {                                   // plain Huber, mean over the 4 coordinates
            s_cmp = 0.25f * (huber1(p.x - t.x) + huber1(p.y - t.y) + huber1(p.z - t.z) + huber1(p.w - t.w));
        } else {
            const float4 anc = reinterpret_cast<const float4*>(a.anchors)[an];
            float pb[4], tb[4];
            pb[0] = anc.z * p.x / 10.0f + anc.x; tb[0] = anc.z * t.x / 10.0f + anc.x;
            pb[1] = anc.w * p.y / 10.0f + anc.y; tb[1] = anc.w * t.y / 10.0f + anc.y;
            pb[2] = anc.z * fminf(fmaxf(expf(p.z / 5.0f), 1e-4f), 1e4f); tb[2] = anc.z * fminf(fmaxf(expf(t.z / 5.0f), 1e-4f), 1e4f);
            pb[3] = anc.w * fminf(fmaxf(expf(p.w / 5.0f), 1e-4f), 1e4f); tb[3] = anc.w * fminf(fmaxf(expf(t.w / 5.0f), 1e-4f), 1e4f);
            const float* c = a.cov + idx * 10;                   // fill_triangular params: diag = (x4,x9,x5,x0)
            const float ld[4] = {c[4], c[9], c[5], c[0]};
            float cmp = 0.f, reg = 0.f;
            if (PROPER && a.reg_kind == 4) {                     // exact Gaussian NLL: Sigma^-1 = A1^T D^-1 A1, r = A1 e
                const float e0 = pb[0] - tb[0], e1 = pb[1] - tb[1], e2 = pb[2] - tb[2], e3 = pb[3] - tb[3];
                const float r[4] = {e0, e1 + c[8] * e0, e2 + c[7] * e0 + c[6] * e1, e3 + c[3] * e0 + c[2] * e1 + c[1] * e2};
#pragma unroll
                for (int k = 0; k < 4; ++k) { cmp += expf(-ld[k]) * r[k] * r[k]; reg += ld[k]; }
                cmp *= 0.5f;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) { cmp += expf(-ld[k]) * huber1(pb[k] - tb[k]); reg += ld[k]; }
                if (a.reg_kind == 3) {                           // x ||L_inv||_F, unit diagonal
                    const float fro = sqrtf(4.0f + c[8] * c[8] + c[7] * c[7] + c[6] * c[6] + c[3] * c[3] + c[2] * c[2] + c[1] * c[1]);
                    cmp *= fro;
                }
            }
            s_cmp = cmp; s_reg = 0.5f * reg;
        }
    }
}

// Block sum of the four terms in a fixed tree order; thread q < 4 then writes term q to out4[q].
__device__ __forceinline__ void loss_block_sums(float (*red)[LOSS_BLOCK], int tid, float s_cls, float s_cmp, float s_reg, float s_pos,
                                                float* __restrict__ out4) {
    red[0][tid] = s_cls; red[1][tid] = s_cmp; red[2][tid] = s_reg; red[3][tid] = s_pos;
    __syncthreads();
    for (int s = LOSS_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int q = 0; q < 4; ++q) red[q][tid] += red[q][tid + s];
        }
        __syncthreads();
    }
    if (tid < 4) out4[tid] = red[tid][0];
}

template <int C, bool PROPER>
__global__ __launch_bounds__(LOSS_BLOCK) void loss_kernel(LossArgs a, float* __restrict__ partial) {
    __shared__ float red[4][LOSS_BLOCK];
    const int tid = threadIdx.x;
    const long long idx = (long long)blockIdx.x * LOSS_BLOCK + tid;
    float s_cls = 0.f, s_cmp = 0.f, s_reg = 0.f, s_pos = 0.f;
    if (idx < (long long)a.B * a.A) loss_anchor_terms<C, PROPER>(a, idx, (int)(idx % a.A), s_cls, s_cmp, s_reg, s_pos);
    loss_block_sums(red, tid, s_cls, s_cmp, s_reg, s_pos, partial + (size_t)blockIdx.x * 4);
}

// Per-frame form (validation from boxes): blockIdx.y = frame, blockIdx.x = a block of 256 of that frame's anchors, so a frame's
// block partials -- partial[(frame * gridDim.x + block) * 4 + q] -- depend on nothing but the frame's own tensors: neither on the
// batch it sits in nor on its position there.
template <int C, bool PROPER>
__global__ __launch_bounds__(LOSS_BLOCK) void loss_frames_kernel(LossArgs a, float* __restrict__ partial) {
    __shared__ float red[4][LOSS_BLOCK];
    const int tid = threadIdx.x;
    const int an = blockIdx.x * LOSS_BLOCK + tid;
    float s_cls = 0.f, s_cmp = 0.f, s_reg = 0.f, s_pos = 0.f;
    if (an < a.A) loss_anchor_terms<C, PROPER>(a, (long long)blockIdx.y * a.A + an, an, s_cls, s_cmp, s_reg, s_pos);
    loss_block_sums(red, tid, s_cls, s_cmp, s_reg, s_pos, partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4);
}

hipError_t launch_loss(const LossArgs& a, float* partial, int nblocks, hipStream_t s) {
    const bool proper = a.reg_kind >= 4;
    if (a.C == 8 && proper) hipLaunchKernelGGL((loss_kernel<8, true>), dim3(nblocks), dim3(LOSS_BLOCK), 0, s, a, partial);
    else if (a.C == 4 && proper) hipLaunchKernelGGL((loss_kernel<4, true>), dim3(nblocks), dim3(LOSS_BLOCK), 0, s, a, partial);
    else if (a.C == 8) hipLaunchKernelGGL((loss_kernel<8, false>), dim3(nblocks), dim3(LOSS_BLOCK), 0, s, a, partial);
    else if (a.C == 4) hipLaunchKernelGGL((loss_kernel<4, false>), dim3(nblocks), dim3(LOSS_BLOCK), 0, s, a, partial);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_loss_frames(const LossArgs& a, float* partial, hipStream_t s) {
    if (a.A < 1 || a.B < 1 || a.B > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.A + LOSS_BLOCK - 1) / LOSS_BLOCK), (unsigned)a.B);
    const bool proper = a.reg_kind >= 4;
    if (a.C == 8 && proper) hipLaunchKernelGGL((loss_frames_kernel<8, true>), grid, dim3(LOSS_BLOCK), 0, s, a, partial);
    else if (a.C == 4 && proper) hipLaunchKernelGGL((loss_frames_kernel<4, true>), grid, dim3(LOSS_BLOCK), 0, s, a, partial);
    else if (a.C == 8) hipLaunchKernelGGL((loss_frames_kernel<8, false>), grid, dim3(LOSS_BLOCK), 0, s, a, partial);
    else if (a.C == 4) hipLaunchKernelGGL((loss_frames_kernel<4, false>), grid, dim3(LOSS_BLOCK), 0, s, a, partial);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}


// ------------------------------------------------------------------------------------------------
// Loss BACKWARD: gradients of
//     total = w_cls * S_cls / max(n_pos, 1) + w_reg * (S_cmp + S_reg) / max(n_pos, 1)
// with respect to the raw head outputs (class logits, box regression targets, the 10 covariance parameters),
// exactly the terms loss_kernel sums; the focal modulating factor is differentiated too (the reference
// applies no stop_gradient, src/core/losses.py:44-61).  sums[3] = n_pos comes from the forward pass on the device.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float huber1_grad(float e) { return fminf(fmaxf(e, -1.0f), 1.0f); }

template <int C, bool PROPER>
__global__ __launch_bounds__(LOSS_BLOCK) void loss_backward_kernel(LossArgs a, const float* __restrict__ sums, float w_cls, float w_reg,
                                                                   float* __restrict__ dcls, float* __restrict__ dbox, float* __restrict__ dcov) {
    const long long idx = (long long)blockIdx.x * LOSS_BLOCK + threadIdx.x;
    if (idx >= (long long)a.B * a.A) return;
    const int an = (int)(idx % a.A);
    const float inv_n = 1.0f / fmaxf(sums[3], 1.0f);
    const float pos = a.pos[idx] ? 1.f : 0.f, neg = a.neg[idx] ? 1.f : 0.f;
    if (dcls) {
        float g[C];
#pragma unroll
        for (int j = 0; j < C; ++j) g[j] = 0.f;
        if (a.do_cls && (pos + neg) > 0.f) {
            const float* x = a.cls + idx * C;
            const float* y = a.cls_t + idx * C;
            float v[C], mx = x[0];
#pragma unroll
            for (int j = 0; j < C; ++j) { v[j] = x[j]; mx = fmaxf(mx, v[j]); }
            float se = 0.f;
#pragma unroll
            for (int j = 0; j < C; ++j) se += expf(v[j] - mx);
            const float lse = logf(se);
            float p[C], q[C], pt = 0.f, ce = 0.f, Q = 0.f;
#pragma unroll
            for (int j = 0; j < C; ++j) {
                const float ls = v[j] - mx - lse;
                p[j] = expf(ls);
                q[j] = y[j] * (1.0f - a.label_smoothing) + a.label_smoothing / (float)C;
                pt += p[j] * y[j]; ce -= q[j] * ls; Q += q[j];
            }
            const float ngm = y[C - 1];
            const float alpha = 0.5f * (1.0f - ngm) + 0.5f * ngm;
            const float f = 1.0f - pt;
            const float k = alpha * (pos + neg) * w_cls * inv_n;
#pragma unroll
            for (int j = 0; j < C; ++j)
                g[j] = k * (-2.0f * f * ce * p[j] * (y[j] - pt) + f * f * (p[j] * Q - q[j]));
        }
#pragma unroll
        for (int j = 0; j < C; ++j) dcls[idx * C + j] = g[j];
    }
    float gb[4] = {0.f, 0.f, 0.f, 0.f};
    float gc[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (a.reg_kind && !(PROPER && a.reg_kind == 5) && pos > 0.f) {   // (kind 5: zeros here, energy_backward_kernel writes the positive rows)
        const float4 p = reinterpret_cast<const float4*>(a.box)[idx];
        const float4 t = reinterpret_cast<const float4*>(a.box_t)[idx];
        const float k = w_reg * inv_n;
        if (a.reg_kind == 1) {
            gb[0] = 0.25f * k * huber1_grad(p.x - t.x); gb[1] = 0.25f * k * huber1_grad(p.y - t.y);
            gb[2] = 0.25f * k * huber1_grad(p.z - t.z); gb[3] = 0.25f * k * huber1_grad(p.w - t.w);
        } else {
            const float4 anc = reinterpret_cast<const float4*>(a.anchors)[an];
            const float ez = expf(p.z / 5.0f), ew = expf(p.w / 5.0f);
            float pb[4], tb[4], dpb[4];
            pb[0] = anc.z * p.x / 10.0f + anc.x; tb[0] = anc.z * t.x / 10.0f + anc.x; dpb[0] = anc.z / 10.0f;
            pb[1] = anc.w * p.y / 10.0f + anc.y; tb[1] = anc.w * t.y / 10.0f + anc.y; dpb[1] = anc.w / 10.0f;
            pb[2] = anc.z * fminf(fmaxf(ez, 1e-4f), 1e4f); tb[2] = anc.z * fminf(fmaxf(expf(t.z / 5.0f), 1e-4f), 1e4f);
            pb[3] = anc.w * fminf(fmaxf(ew, 1e-4f), 1e4f); tb[3] = anc.w * fminf(fmaxf(expf(t.w / 5.0f), 1e-4f), 1e4f);
            dpb[2] = (ez >= 1e-4f && ez <= 1e4f) ? anc.z * ez / 5.0f : 0.f;           // clip_by_value passes no gradient outside
            dpb[3] = (ew >= 1e-4f && ew <= 1e4f) ? anc.w * ew / 5.0f : 0.f;
            const float* c = a.cov + idx * 10;
            const int di[4] = {4, 9, 5, 0};                                           // fill_triangular diagonal = (x4, x9, x5, x0)
            if (PROPER && a.reg_kind == 4) {                                          // u = D^-1 A1 e; d/de = A1^T u, d/dA1[k][j] = u_k e_j
                const float e[4] = {pb[0] - tb[0], pb[1] - tb[1], pb[2] - tb[2], pb[3] - tb[3]};
                const float r[4] = {e[0], e[1] + c[8] * e[0], e[2] + c[7] * e[0] + c[6] * e[1], e[3] + c[3] * e[0] + c[2] * e[1] + c[1] * e[2]};
                float u[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    u[q] = expf(-c[di[q]]) * r[q];
                    gc[di[q]] = k * (-0.5f * u[q] * r[q] + 0.5f);
                }
                gb[0] = k * (u[0] + c[8] * u[1] + c[7] * u[2] + c[3] * u[3]) * dpb[0];
                gb[1] = k * (u[1] + c[6] * u[2] + c[2] * u[3]) * dpb[1];
                gb[2] = k * (u[2] + c[1] * u[3]) * dpb[2];
                gb[3] = k * u[3] * dpb[3];
                gc[8] = k * u[1] * e[0];
                gc[7] = k * u[2] * e[0]; gc[6] = k * u[2] * e[1];
                gc[3] = k * u[3] * e[0]; gc[2] = k * u[3] * e[1]; gc[1] = k * u[3] * e[2];
            } else {
                float eld[4], hub[4], cmp = 0.f;
#pragma unroll
                for (int q = 0; q < 4; ++q) { eld[q] = expf(-c[di[q]]); hub[q] = huber1(pb[q] - tb[q]); cmp += eld[q] * hub[q]; }
                float fro = 1.0f;
                if (a.reg_kind == 3) fro = sqrtf(4.0f + c[8] * c[8] + c[7] * c[7] + c[6] * c[6] + c[3] * c[3] + c[2] * c[2] + c[1] * c[1]);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    gb[q] = k * fro * eld[q] * huber1_grad(pb[q] - tb[q]) * dpb[q];
                    gc[di[q]] = k * (-fro * eld[q] * hub[q] + 0.5f);
                }
                if (a.reg_kind == 3) {
                    const int od[6] = {8, 7, 6, 3, 2, 1};
#pragma unroll
                    for (int q = 0; q < 6; ++q) gc[od[q]] = k * cmp * c[od[q]] / fro;
                }
            }
        }
    }
    if (dbox) reinterpret_cast<float4*>(dbox)[idx] = make_float4(gb[0], gb[1], gb[2], gb[3]);
    if (dcov) {
#pragma unroll
        for (int q = 0; q < 10; ++q) dcov[idx * 10 + q] = gc[q];
    }
}

// sums[0..3] = (S_cls, S_cmp, S_reg, n_pos) from the block partials, on the device: one block per group of `nblocks` partials
// (blockIdx.x = group: the whole batch for the training step, one frame for launch_loss_frames), added in double in a fixed order
template <typename T>
__global__ __launch_bounds__(LOSS_BLOCK) void loss_reduce_kernel(const float* __restrict__ partial, int nblocks, T* __restrict__ sums) {
    __shared__ double red[4][LOSS_BLOCK];
    partial += (size_t)blockIdx.x * nblocks * 4;
    sums += (size_t)blockIdx.x * 4;
    double acc[4] = {0, 0, 0, 0};
    for (int i = threadIdx.x; i < nblocks; i += LOSS_BLOCK)
        for (int q = 0; q < 4; ++q) acc[q] += (double)partial[(size_t)i * 4 + q];
    for (int q = 0; q < 4; ++q) red[q][threadIdx.x] = acc[q];
    __syncthreads();
    for (int s = LOSS_BLOCK / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s)
            for (int q = 0; q < 4; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < 4) sums[threadIdx.x] = (T)red[threadIdx.x][0];
}

hipError_t launch_loss_reduce(const float* partial, int nblocks, float* sums, hipStream_t s) {
    hipLaunchKernelGGL(loss_reduce_kernel<float>, dim3(1), dim3(LOSS_BLOCK), 0, s, partial, nblocks, sums);
    return hipGetLastError();
}

hipError_t launch_loss_frames_reduce(const float* partial, int frames, int nblocks, double* sums, hipStream_t s) {
    if (frames < 1 || nblocks < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(loss_reduce_kernel<double>, dim3(frames), dim3(LOSS_BLOCK), 0, s, partial, nblocks, sums);
    return hipGetLastError();
}

hipError_t launch_loss_backward(const LossArgs& a, const float* sums, float w_cls, float w_reg, float* dcls, float* dbox, float* dcov,
                                hipStream_t s) {
    const int nblocks = (int)(((long long)a.B * a.A + LOSS_BLOCK - 1) / LOSS_BLOCK);
    const bool proper = a.reg_kind >= 4;
    if (a.C == 8 && proper) hipLaunchKernelGGL((loss_backward_kernel<8, true>), dim3(nblocks), dim3(LOSS_BLOCK), 0, s, a, sums, w_cls, w_reg, dcls, dbox, dcov);
    else if (a.C == 4 && proper) hipLaunchKernelGGL((loss_backward_kernel<4, true>), dim3(nblocks), dim3(LOSS_BLOCK), 0, s, a, sums, w_cls, w_reg, dcls, dbox, dcov);
    else if (a.C == 8) hipLaunchKernelGGL((loss_backward_kernel<8, false>), dim3(nblocks), dim3(LOSS_BLOCK), 0, s, a, sums, w_cls, w_reg, dcls, dbox, dcov);
    else if (a.C == 4) hipLaunchKernelGGL((loss_backward_kernel<4, false>), dim3(nblocks), dim3(LOSS_BLOCK), 0, s, a, sums, w_cls, w_reg, dcls, dbox, dcov);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}


// ------------------------------------------------------------------------------------------------
// reg_kind 5, 'regression_energy' (DESIGN.md 9.10): the sample-based energy score of the per-anchor box Gaussian
//     Sigma = A1^-1 diag(exp ld) A1^-T,   A1 unit lower with rows (1), (c8, 1), (c7, c6, 1), (c3, c2, c1, 1),   ld = (c4, c9, c5, c0)
// in corner space (T: vuhw -> x1, y1, x2, y2):  y_i solves A1 y_i = exp(ld / 2) o n_i,  z_i = T (pb + y_i),  g = T tb,
//     term = (1/M) sum_{i<M} |z_i - g| - 1/(2(M-1)) sum_{i<M-1} |z_i - z_{i+1}|.
// T is linear, so z_i - g = T (e + y_i) with e = pb - tb and z_i - z_j = T (y_i - y_j): the kernels carry y, never z, and a
// difference of two samples does not lose the bits a pixel coordinate of ~1e3 would cost it in fp32.
//
// Normals: sample i of (image id, anchor a) is ONE call philox4x32_10(i, a, BOD_LOSS_TAG, image id, seed_lo, seed_hi)
// -> (x, y, z, w), u(t) = (t + 0.5) 2^-32, n0, n1 = sqrt(-2 ln u(x)) (cos, sin)(2 pi u(y)), n2, n3 likewise from (z, w).
//
// Shape: the positives are a few hundred of ~50 k anchors a frame, so loss_compact_kernel lists them (ascending; one block,
// 8 bytes a lane, wave scans, no atomics) and the energy kernels run a FIXED grid -- the step is a captured graph -- of one wave64 per
// row, four rows a workgroup, striding over the list.  Lane l takes samples l, l + 64, ...; sample i - 1 (backward: i + 1 too) is
// a cross-lane read, the lane at the wave's edge taking the sample its neighbour held one trip earlier (generates one trip
// ahead).  Per-lane sums are folded by __shfl_down 32 ... 1: a row's bits depend on (seed, image id, anchor, M) and the row's
// own tensors alone.  Row constants are read at a wave-uniform index.
// ------------------------------------------------------------------------------------------------
#define ENERGY_BLOCK 256
#define ENERGY_ROWS_PER_BLOCK (ENERGY_BLOCK / 64)
#define ENERGY_MAX_GRID 256
#define COMPACT_BLOCK 1024
#define COMPACT_WAVES (COMPACT_BLOCK / 64)

// list[0] = number of set bytes of pos[0..n), list[1 + r] = index of the r-th one.  Wave w owns the contiguous slice
// [w * per, (w + 1) * per), per a multiple of 512, and walks it 512 bytes a trip -- one 8-byte load a lane (pos is 8-byte aligned;
// the slice's last, partial group is read byte by byte) -- twice: count, then (after the 16 counts are known) write.  A lane's
// place in the trip is an exclusive wave scan of the lanes' counts (__shfl_up 1 ... 32).
__device__ __forceinline__ unsigned long long compact_load8(const uint8_t* __restrict__ pos, long long j, long long hi) {
    if (j + 8 <= hi) return *reinterpret_cast<const unsigned long long*>(pos + j);
    unsigned long long v = 0;
    for (int b = 0; b < 8; ++b)
        if (j + b < hi && pos[j + b]) v |= 0xffull << (8 * b);
    return v;
}
__device__ __forceinline__ int compact_count8(unsigned long long v) {
    int c = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) c += ((v >> (8 * b)) & 0xffull) ? 1 : 0;
    return c;
}

__global__ __launch_bounds__(COMPACT_BLOCK) void loss_compact_kernel(const uint8_t* __restrict__ pos, long long n, int32_t* __restrict__ list) {
    __shared__ int wcount[COMPACT_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long per = (n + COMPACT_WAVES * 512 - 1) / (COMPACT_WAVES * 512) * 512;
    const long long lo = (long long)w * per, hi = lo + per < n ? lo + per : n;
    int cnt = 0;
    for (long long i = lo; i < hi; i += 512) cnt += compact_count8(compact_load8(pos, i + 8 * lane, hi));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
    if (lane == 0) wcount[w] = cnt;
    __syncthreads();
    int off = 0, total = 0;
#pragma unroll
    for (int k = 0; k < COMPACT_WAVES; ++k) { const int c = wcount[k]; if (k < w) off += c; total += c; }
    for (long long i = lo; i < hi; i += 512) {                   // wave-uniform bounds: all 64 lanes take part in the scan
        const long long j = i + 8 * lane;
        const unsigned long long v = compact_load8(pos, j, hi);
        const int c = compact_count8(v);
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        int at = 1 + off + incl - c;
#pragma unroll
        for (int b = 0; b < 8; ++b)
            if ((v >> (8 * b)) & 0xffull) list[at++] = (int32_t)(j + b);
        off += __shfl(incl, 63);
    }
    if (threadIdx.x == 0) list[0] = total;
}

__device__ __forceinline__ float energy_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;                                                    // lane 0 holds the total
}

__device__ __forceinline__ float energy_uniform(uint32_t t) { return ((float)t + 0.5f) * 2.3283064365386963e-10f; }      // 2^-32

// What a positive row contributes besides its samples: e = pb - tb, the decode's derivative, exp(ld / 2), A1's off-diagonals
struct EnergyRow {
    float e[4], dpb[4], sd[4];
    float a10, a20, a21, a30, a31, a32;
    uint32_t an, image_id, seed_lo, seed_hi;
};

__device__ __forceinline__ EnergyRow energy_row(const EnergyArgs& a, int idx) {
    EnergyRow R;
    const int b = idx / a.A, an = idx - b * a.A;
    const float4 p = reinterpret_cast<const float4*>(a.box)[idx];
    const float4 t = reinterpret_cast<const float4*>(a.box_t)[idx];
    const float4 anc = reinterpret_cast<const float4*>(a.anchors)[an];
    const float ez = expf(p.z / 5.0f), ew = expf(p.w / 5.0f);        // the decode of reg_kind 2 / 3, clips included
    R.e[0] = (anc.z * p.x / 10.0f + anc.x) - (anc.z * t.x / 10.0f + anc.x); R.dpb[0] = anc.z / 10.0f;
    R.e[1] = (anc.w * p.y / 10.0f + anc.y) - (anc.w * t.y / 10.0f + anc.y); R.dpb[1] = anc.w / 10.0f;
    R.e[2] = anc.z * fminf(fmaxf(ez, 1e-4f), 1e4f) - anc.z * fminf(fmaxf(expf(t.z / 5.0f), 1e-4f), 1e4f);
    R.e[3] = anc.w * fminf(fmaxf(ew, 1e-4f), 1e4f) - anc.w * fminf(fmaxf(expf(t.w / 5.0f), 1e-4f), 1e4f);
    R.dpb[2] = (ez >= 1e-4f && ez <= 1e4f) ? anc.z * ez / 5.0f : 0.f;
    R.dpb[3] = (ew >= 1e-4f && ew <= 1e4f) ? anc.w * ew / 5.0f : 0.f;
    const float* c = a.cov + (size_t)idx * 10;
    R.sd[0] = expf(0.5f * c[4]); R.sd[1] = expf(0.5f * c[9]); R.sd[2] = expf(0.5f * c[5]); R.sd[3] = expf(0.5f * c[0]);
    R.a10 = c[8]; R.a20 = c[7]; R.a21 = c[6]; R.a30 = c[3]; R.a31 = c[2]; R.a32 = c[1];
    R.an = (uint32_t)an;
    if (a.dyn) { R.seed_lo = a.dyn[0]; R.seed_hi = a.dyn[1]; R.image_id = a.dyn[2] + (uint32_t)(b * a.id_stride); }
    else { R.seed_lo = a.seed_lo; R.seed_hi = a.seed_hi; R.image_id = a.first_image_id + (uint32_t)(b * a.id_stride); }
    return R;
}

// sample i of the row: s = exp(ld / 2) o n_i and y with A1 y = s (forward substitution)
__device__ __forceinline__ void energy_sample(const EnergyRow& R, uint32_t i, float s[4], float y[4]) {
    const Philox4 w = philox4x32_10(i, R.an, BOD_LOSS_TAG, R.image_id, R.seed_lo, R.seed_hi);
    const float r0 = sqrtf(-2.0f * logf(energy_uniform(w.x))), r1 = sqrtf(-2.0f * logf(energy_uniform(w.z)));
    float s0, c0, s1, c1;
    sincospif(2.0f * energy_uniform(w.y), &s0, &c0);             // (cos, sin)(2 pi u) with the reduction exact
    sincospif(2.0f * energy_uniform(w.w), &s1, &c1);
    s[0] = R.sd[0] * (r0 * c0); s[1] = R.sd[1] * (r0 * s0); s[2] = R.sd[2] * (r1 * c1); s[3] = R.sd[3] * (r1 * s1);
    y[0] = s[0];
    y[1] = s[1] - R.a10 * y[0];
    y[2] = s[2] - R.a20 * y[0] - R.a21 * y[1];
    y[3] = s[3] - R.a30 * y[0] - R.a31 * y[1] - R.a32 * y[2];
}

// |T d|^2 for a vuhw difference d.  T's columns are orthogonal, T^T T = diag(2, 2, 1/2, 1/2) (corners = (u - w/2, v - h/2,
// u + w/2, v + h/2)), so the corner-space norm and its gradient T^T T d / |T d| need no corner: forming x1 = u - w/2 and
// x2 = u + w/2 first and adding them back in T^T would cancel u against a large w (a row beyond the exp clip: w ~ 1e6 px).
__device__ __forceinline__ float energy_norm2(const float d[4]) {
    return 2.0f * d[0] * d[0] + 2.0f * d[1] * d[1] + 0.5f * d[2] * d[2] + 0.5f * d[3] * d[3];
}

__global__ __launch_bounds__(ENERGY_BLOCK) void energy_forward_kernel(EnergyArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * ENERGY_ROWS_PER_BLOCK + (threadIdx.x >> 6)));
    const int nwaves = (int)gridDim.x * ENERGY_ROWS_PER_BLOCK;
    const int count = a.list[0];
    const int from = (lane + 63) & 63;
    for (int r = wave; r < count; r += nwaves) {                 // (whole waves: nothing below waits for another wave)
        const int idx = __builtin_amdgcn_readfirstlane(a.list[1 + r]);
        const EnergyRow R = energy_row(a, idx);
        float sum_a = 0.f, sum_b = 0.f;
        float yl[4] = {0.f, 0.f, 0.f, 0.f};                      // this lane's sample of the trip before
        for (int base = 0; base < a.M; base += 64) {             // uniform trip count: every lane takes part in the cross-lane reads
            const int i = base + lane;
            float s[4], y[4], d[4], dp[4];
            energy_sample(R, (uint32_t)i, s, y);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // sample i - 1: lane l - 1 of this trip, or (lane 0) lane 63 of the trip before
                const float yp = __shfl(lane == 63 ? yl[k] : y[k], from);
                d[k] = R.e[k] + y[k];
                dp[k] = y[k] - yp;
                yl[k] = y[k];
            }
            const float da = sqrtf(energy_norm2(d)), db = sqrtf(energy_norm2(dp));
            if (i < a.M) {
                sum_a += da;
                if (i >= 1) sum_b += db;
            }
        }
        sum_a = energy_wave_sum(sum_a);
        sum_b = energy_wave_sum(sum_b);
        if (lane == 0) a.row_term[idx] = sum_a / (float)a.M - sum_b / (2.0f * (float)(a.M - 1));
    }
}

// v += scale * T^T u(T d),  u(x) = x / |x| and 0 at x = 0:  T^T T d / |T d|
__device__ __forceinline__ void energy_add_unit(const float d[4], float scale, float v[4]) {
    const float n2 = energy_norm2(d);
    const float f = n2 > 0.f ? scale / sqrtf(n2) : 0.f;
    v[0] += f * 2.0f * d[0]; v[1] += f * 2.0f * d[1]; v[2] += f * 0.5f * d[2]; v[3] += f * 0.5f * d[3];
}

// Gradient of  w_reg * term / max(n_pos, 1)  with respect to the row's box and covariance outputs:
//   w_i = (1/M) u(z_i - g) - 1/(2(M-1)) [u(z_i - z_{i+1}) + u(z_i - z_{i-1})],  u(x) = x / |x|, neighbours where they exist;
//   d/dpb = T^T sum w_i = (1/M) T^T sum u(z_i - g)  (the neighbour terms cancel in pairs);  q_i = A1^-T T^T w_i;  d/dld_k = 0.5 sum q_ik s_ik;  d/dA1[k][j] = -sum q_ik y_ij.
__global__ __launch_bounds__(ENERGY_BLOCK) void energy_backward_kernel(EnergyArgs a, const float* __restrict__ sums, float w_reg,
                                                                       float* __restrict__ dbox, float* __restrict__ dcov) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * ENERGY_ROWS_PER_BLOCK + (threadIdx.x >> 6)));
    const int nwaves = (int)gridDim.x * ENERGY_ROWS_PER_BLOCK;
    const int count = a.list[0];
    const float kk = w_reg / fmaxf(sums[3], 1.0f);
    const float ca = 1.0f / (float)a.M, cb = -1.0f / (2.0f * (float)(a.M - 1));
    const int from = (lane + 63) & 63, to = (lane + 1) & 63;
    for (int r = wave; r < count; r += nwaves) {
        const int idx = __builtin_amdgcn_readfirstlane(a.list[1 + r]);
        const EnergyRow R = energy_row(a, idx);
        float gp[4] = {0.f, 0.f, 0.f, 0.f}, gl[4] = {0.f, 0.f, 0.f, 0.f};
        float g10 = 0.f, g20 = 0.f, g21 = 0.f, g30 = 0.f, g31 = 0.f, g32 = 0.f;
        float yl[4] = {0.f, 0.f, 0.f, 0.f};                      // this lane's sample one trip back, this trip, one trip ahead
        float s[4], y[4], sn[4] = {0.f, 0.f, 0.f, 0.f}, yn[4] = {0.f, 0.f, 0.f, 0.f};
        energy_sample(R, (uint32_t)lane, s, y);
        for (int base = 0; base < a.M; base += 64) {
            const int i = base + lane;
            if (base + 64 < a.M) energy_sample(R, (uint32_t)(i + 64), sn, yn);       // (uniform)
            float d[4], dp[4], dn[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float yp = __shfl(lane == 63 ? yl[k] : y[k], from);            // sample i - 1
                const float yq = __shfl(lane == 0 ? yn[k] : y[k], to);               // sample i + 1
                d[k] = R.e[k] + y[k];
                dp[k] = y[k] - yp;
                dn[k] = y[k] - yq;
            }
            // T^T w_i; its target part alone is what d/dpb sums: the neighbour parts of sample i and of its neighbour are each
            // other's negatives, and summing those O(1) pairs in fp32 would bury a sum that can be 1e-5 of them
            float vg[4] = {0.f, 0.f, 0.f, 0.f};
            energy_add_unit(d, ca, vg);
            float v[4] = {vg[0], vg[1], vg[2], vg[3]};
            if (i >= 1) energy_add_unit(dp, cb, v);
            if (i + 1 < a.M) energy_add_unit(dn, cb, v);
            if (i < a.M) {
                // A1^T q = v by back substitution
                float q[4];
                q[3] = v[3];
                q[2] = v[2] - R.a32 * q[3];
                q[1] = v[1] - R.a21 * q[2] - R.a31 * q[3];
                q[0] = v[0] - R.a10 * q[1] - R.a20 * q[2] - R.a30 * q[3];
#pragma unroll
                for (int k = 0; k < 4; ++k) { gp[k] += vg[k]; gl[k] += q[k] * s[k]; }
                g10 -= q[1] * y[0];
                g20 -= q[2] * y[0]; g21 -= q[2] * y[1];
                g30 -= q[3] * y[0]; g31 -= q[3] * y[1]; g32 -= q[3] * y[2];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) { yl[k] = y[k]; y[k] = yn[k]; s[k] = sn[k]; }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) { gp[k] = energy_wave_sum(gp[k]); gl[k] = energy_wave_sum(gl[k]); }
        g10 = energy_wave_sum(g10); g20 = energy_wave_sum(g20); g21 = energy_wave_sum(g21);
        g30 = energy_wave_sum(g30); g31 = energy_wave_sum(g31); g32 = energy_wave_sum(g32);
        if (lane == 0) {
            if (dbox) reinterpret_cast<float4*>(dbox)[idx] = make_float4(kk * gp[0] * R.dpb[0], kk * gp[1] * R.dpb[1], kk * gp[2] * R.dpb[2],
                                                                         kk * gp[3] * R.dpb[3]);
            if (dcov) {
                float* o = dcov + (size_t)idx * 10;              // fill_triangular order: diagonal = (x4, x9, x5, x0)
                o[4] = kk * 0.5f * gl[0]; o[9] = kk * 0.5f * gl[1]; o[5] = kk * 0.5f * gl[2]; o[0] = kk * 0.5f * gl[3];
                o[8] = kk * g10; o[7] = kk * g20; o[6] = kk * g21; o[3] = kk * g30; o[2] = kk * g31; o[1] = kk * g32;
            }
        }
    }
}

static bool energy_args_ok(const EnergyArgs& a) {
    return a.B >= 1 && a.A >= 1 && (long long)a.B * a.A < 0x7fffffffLL && a.M >= BOD_ENERGY_MIN_SAMPLES && a.M <= BOD_ENERGY_MAX_SAMPLES;
}
static unsigned energy_grid(const EnergyArgs& a) {                // fixed by the shape alone, never by the number of positives
    const long long blocks = ((long long)a.B * a.A + ENERGY_ROWS_PER_BLOCK - 1) / ENERGY_ROWS_PER_BLOCK;
    return (unsigned)(blocks < ENERGY_MAX_GRID ? blocks : ENERGY_MAX_GRID);
}

hipError_t launch_loss_compact(const uint8_t* pos, long long n, int32_t* list, hipStream_t s) {
    if (n < 1 || n >= 0x7fffffffLL || !pos || !list || (reinterpret_cast<uintptr_t>(pos) & 7)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(loss_compact_kernel, dim3(1), dim3(COMPACT_BLOCK), 0, s, pos, n, list);
    return hipGetLastError();
}

hipError_t launch_energy_forward(const EnergyArgs& a, hipStream_t s) {
    if (!energy_args_ok(a) || !a.list || !a.row_term) return hipErrorInvalidValue;
    hipLaunchKernelGGL(energy_forward_kernel, dim3(energy_grid(a)), dim3(ENERGY_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_energy_backward(const EnergyArgs& a, const float* sums, float w_reg, float* dbox, float* dcov, hipStream_t s) {
    if (!energy_args_ok(a) || !a.list || !sums) return hipErrorInvalidValue;
    hipLaunchKernelGGL(energy_backward_kernel, dim3(energy_grid(a)), dim3(ENERGY_BLOCK), 0, s, a, sums, w_reg, dbox, dcov);
    return hipGetLastError();
}

// Bias gradient of a head's output convolution straight from the loss gradient: out[c] = sum over rows of g[row][c], g = dbox or
// dcov read as [B * positions][anchors per location * width].  One block per channel, double sums in a fixed order (no atomics).
// The bf16 training handle uses it for reg_kind 4 / 5 (train_impl.inc), whose weight-gradient GEMM would read dZ from bf16 storage.
__global__ __launch_bounds__(LOSS_BLOCK) void head_bias_grad_kernel(const float* __restrict__ g, long long rows, int nch, float* __restrict__ out) {
    __shared__ double red[LOSS_BLOCK];
    const int c = blockIdx.x;
    double acc = 0.0;
    for (long long r = threadIdx.x; r < rows; r += LOSS_BLOCK) acc += (double)g[r * nch + c];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = LOSS_BLOCK / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[c] = (float)red[0];
}

hipError_t launch_head_bias_grad(const float* g, long long rows, int nch, float* out, hipStream_t s) {
    if (!g || !out || rows < 1 || nch < 1 || nch > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(head_bias_grad_kernel, dim3((unsigned)nch), dim3(LOSS_BLOCK), 0, s, g, rows, nch, out);
    return hipGetLastError();
}

"""Plain restatements (NumPy / torch, no project code) of the backward kernels that only the bf16 training handle launches:
activation backward, the input gradient of a convolution, the stem's max-pool backward and the batch-norm fold with its three
weight packings.  tests/test_gpu_train_backward_kernels.py compares the device with them;
tests/test_train_backward_reference_host.py compares them with float64 autograd, so a restatement cannot be wrong on its own.

Where a device result is a fixed sequence of float32 operations the restatement runs the same sequence in float32 and the
comparison is bit for bit; sums whose order the device does not fix are given in float64 together with the sum of magnitudes
that the error bound scales with."""
import numpy as np

BN_EPS = np.float32(1e-3)


# ------------------------------------------------------------------------------------------------ bf16
def bf16_bits(x):
    """float32 -> bf16 bit patterns (uint16), round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = u + 0x7FFF + ((u >> 16) & 1)
    return ((u >> 16) & 0xFFFF).astype(np.uint16)


def bf16_widen(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x):
    return bf16_widen(bf16_bits(x)).reshape(np.shape(x))


def bits32(x):
    """float32 array -> its bit patterns: equality of these is equality bit for bit (+0 and -0 differ, NaNs compare)."""
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ activation backward
def act_backward_form(cout, cout_pad, out_cstride, kpad, want_dzt, has_dres, f32):
    """Which kernel launch_act_backward_gather picks (its rule, restated): 'tile' writes dZ^T itself."""
    if f32:
        return "element"
    if want_dzt and cout % 8 == 0 and cout_pad % 64 == 0 and out_cstride % 8 == 0 and kpad % 64 == 0:
        return "tile"
    if not has_dres and cout % 8 == 0 and cout_pad % 8 == 0 and out_cstride % 8 == 0:
        return "vector"
    return "element"


def act_backward_reference(dout, out_off, cout, cout_pad, out_cstride, kpad, out_act=None, dout_relu=None, scale=1.0,
                           res_off=None, res_cstride=0, dres=None, dzp=None, f32=False):
    """dout / out_act / dout_relu / dzp: flat arrays in the output buffer's layout (dzp: the prefill); dres: flat prefill.
    Returns dict: dz [M, cout_pad], dzt [cout_pad, kpad], dzp (prefill with the written elements replaced) -- float32, bf16 values
    widened -- and dres (float64 sums) with dres_abs (float64 sums of magnitudes, the scale of its error bound)."""
    store = (lambda v: np.asarray(v, np.float32)) if f32 else bf16_round
    dout = np.array(dout, dtype=np.float32).reshape(-1)
    out_off = np.asarray(out_off, dtype=np.int64)
    m = out_off.size
    stored = None if out_act is None else store(np.asarray(out_act, np.float32).reshape(-1))
    if dout_relu is not None:                                   # second consumer through the ReLU'd copy: one float32 add
        add = np.asarray(dout_relu, np.float32).reshape(-1)
        on = stored > 0
        dout[on] = dout[on] + add[on]
    idx = out_off[:, None] * out_cstride + np.arange(cout)[None, :]                  # [M, cout]
    g = dout[idx]
    if stored is not None:
        g = np.where(stored[idx] == 0, np.float32(0), g * np.float32(scale)).astype(np.float32)      # (+0 and -0 both compare equal to 0)
    dz = np.zeros((m, cout_pad), np.float32)
    dz[:, :cout] = store(g)
    dzt = np.zeros((cout_pad, kpad), np.float32)
    dzt[:, :m] = dz.T
    out = {"dz": dz, "dzt": dzt, "dzp": None, "dres": None, "dres_abs": None}
    if dzp is not None:
        p = store(np.asarray(dzp, np.float32).reshape(-1)).copy()
        p[idx] = dz[:, :cout]
        out["dzp"] = p
    if dres is not None:
        acc = np.asarray(dres, np.float64).reshape(-1).copy()
        mag = np.abs(acc)
        ridx = (np.asarray(res_off, np.int64)[:, None] * res_cstride + np.arange(cout)[None, :]).reshape(-1)
        np.add.at(acc, ridx, g.astype(np.float64).reshape(-1))
        np.add.at(mag, ridx, np.abs(g.astype(np.float64)).reshape(-1))
        out["dres"], out["dres_abs"] = acc, mag
    return out


# ------------------------------------------------------------------------------------------------ input gradient
def same_pads(n, k, stride):
    """Keras SAME: (before, after) with before = total // 2."""
    out = -(-n // stride)
    tot = max((out - 1) * stride + k - n, 0)
    return tot // 2, tot - tot // 2


def dgrad_reference(dz, w, in_hw, stride=1, padding="same"):
    """dL/dx [B,H,W,Cin] in float64 of a Keras Conv2D with kernel w (HWIO) for the output gradient dz [B,OH,OW,Cout]: autograd's
    own input-gradient function (torch.nn.grad.conv2d_input) on the explicitly padded input, cropped."""
    import torch
    h, wd = in_hw
    kh, kw, cin, _ = w.shape
    (pt, pb), (pl, pr) = (same_pads(h, kh, stride), same_pads(wd, kw, stride)) if padding == "same" else ((0, 0), (0, 0))
    g = torch.tensor(np.asarray(dz), dtype=torch.float64).permute(0, 3, 1, 2).contiguous()
    wt = torch.tensor(np.asarray(w), dtype=torch.float64).permute(3, 2, 0, 1).contiguous()
    dxp = torch.nn.grad.conv2d_input((g.shape[0], cin, h + pt + pb, wd + pl + pr), wt, g, stride=stride)
    return dxp[:, :, pt:pt + h, pl:pl + wd].permute(0, 2, 3, 1).contiguous().numpy()


def untouched_input_pixels(in_hw, kernel_hw, stride, padding="same"):
    """[H, W] bool: input pixels that no window of the convolution reaches (their gradient is exactly zero)."""
    h, wd = in_hw
    kh, kw = kernel_hw
    (pt, _), (pl, _) = (same_pads(h, kh, stride), same_pads(wd, kw, stride)) if padding == "same" else ((0, 0), (0, 0))
    oh = -(-h // stride) if padding == "same" else (h - kh) // stride + 1
    ow = -(-wd // stride) if padding == "same" else (wd - kw) // stride + 1
    hit = np.zeros((h, wd), bool)
    for y in range(oh):
        for x in range(ow):
            y0, x0 = y * stride - pt, x * stride - pl
            hit[max(y0, 0):max(y0 + kh, 0), max(x0, 0):max(x0 + kw, 0)] = True
    return ~hit


# ------------------------------------------------------------------------------------------------ stem pool backward
def stem_pool_geometry(ih, iw):
    """ZeroPadding2D((1, 2)) + MaxPool 3x3 stride 2 VALID on an [ih, iw] stem output: pooled size."""
    return (ih + 2 - 3) // 2 + 1, (iw + 4 - 3) // 2 + 1


def stem_pool_backward_reference(stem_out, dpool, f32=False):
    """stem_out [B,ih,iw,C] (post-ReLU), dpool [B,oh+2,ow+2,C]: the pooled gradient on its plane with a one-pixel border.
    Window (oy, ox) covers stem rows 2oy-1..2oy+1 and columns 2ox-2..2ox; its first maximum in row-major order takes the
    window's gradient, and only where it is > 0 (the padding's zeros never win against it).  Sums over the windows in (oy, ox)
    order in float32, then rounded like a stored activation.  Returns [B,ih,iw,C] float32."""
    store = (lambda v: np.asarray(v, np.float32)) if f32 else bf16_round
    v = store(np.asarray(stem_out, np.float32))
    dpool = np.asarray(dpool, np.float32)
    b, ih, iw, c = v.shape
    oh, ow = stem_pool_geometry(ih, iw)
    assert dpool.shape == (b, oh + 2, ow + 2, c)
    g = np.zeros((b, ih, iw, c), np.float32)
    bi, ci = np.meshgrid(np.arange(b), np.arange(c), indexing="ij")
    for oy in range(oh):
        for ox in range(ow):
            pos = [(y, x) for y in range(2 * oy - 1, 2 * oy + 2) for x in range(2 * ox - 2, 2 * ox + 1) if 0 <= y < ih and 0 <= x < iw]
            vals = np.stack([v[:, y, x, :] for y, x in pos], axis=0)             # [n, B, C], row-major window order
            first = np.argmax(vals, axis=0)                                      # (argmax returns the first maximum)
            best = np.take_along_axis(vals, first[None], axis=0)[0]
            ys = np.array([p[0] for p in pos])[first]
            xs = np.array([p[1] for p in pos])[first]
            d = np.where(best > 0, dpool[:, oy + 1, ox + 1, :], np.float32(0)).astype(np.float32)
            g[bi, ys, xs, ci] = g[bi, ys, xs, ci] + d                            # (one target per (b, c): no duplicate indices)
    return store(g)


# ------------------------------------------------------------------------------------------------ fold + pack
def fold_pack_reference(kernel, cout_pad, bias=None, gamma=None, beta=None, mean=None, var=None):
    """kernel [taps, cin, cout] float32.  s = gamma / sqrt(var + eps) and v = kernel * s in float32, rounded to bf16, in the three
    layouts of FoldArgs: w_fwd [cout_pad, taps, cin], w_bwd [taps * cin, cout_pad], w_flip [cin, taps (flipped), cout_pad] (uint16
    bit patterns, zero at co >= cout); v64: the same product from float64 scale (for judging single-ulp flips); b64 [cout_pad]:
    the folded bias in float64 with b_scale = |bias - mean| * |s| + |beta| (the scale of its error bound)."""
    k = np.asarray(kernel, np.float32)
    taps, cin, cout = k.shape
    f = lambda a: None if a is None else np.asarray(a, np.float32)
    bias, gamma, beta, mean, var = f(bias), f(gamma), f(beta), f(mean), f(var)
    if gamma is not None:
        s = (gamma / np.sqrt(var + BN_EPS)).astype(np.float32)
        s64 = gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + np.float64(BN_EPS))
    else:
        s, s64 = np.ones(cout, np.float32), np.ones(cout, np.float64)
    v = (k * s[None, None, :]).astype(np.float32)
    hv = bf16_bits(v).reshape(taps, cin, cout)
    full = np.zeros((taps, cin, cout_pad), np.uint16)
    full[:, :, :cout] = hv
    b0 = np.zeros(cout, np.float64) if bias is None else bias.astype(np.float64)
    if gamma is not None:
        b64 = (b0 - mean.astype(np.float64)) * s64 + beta.astype(np.float64)
        b_scale = np.abs(b0 - mean.astype(np.float64)) * np.abs(s64) + np.abs(beta.astype(np.float64))
    else:
        b64, b_scale = b0, np.abs(b0)
    pad = lambda a: np.concatenate([a, np.zeros(cout_pad - cout, a.dtype)])
    return {"w_fwd": np.ascontiguousarray(full.transpose(2, 0, 1)), "w_bwd": full.reshape(taps * cin, cout_pad).copy(),
            "w_flip": np.ascontiguousarray(full[::-1].transpose(1, 0, 2)), "w_fwd32": v.reshape(taps * cin, cout),
            "v64": k.astype(np.float64) * s64[None, None, :], "b64": pad(b64), "b_scale": pad(b_scale)}

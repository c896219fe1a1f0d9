"""Float64 restatement of the stem (7x7 s2 VALID conv + bias + ReLU) and of ZeroPadding2D((1,2)) + MaxPool 3x3 s2, with the operand
splits of the stem kernels and the error bounds tests/test_gpu_stem_kernels.py holds them to.  NumPy only, no
project code: tests/test_stem_reference_host.py checks it against torch in float64 and checks the exactness claims."""
import numpy as np

SENTINEL = -65536.0                       # exactly representable in bf16
MEANS = np.array([123.68, 116.78, 103.94], np.float32)
U = 2.0 ** -23                            # one fp32 ulp of a value in [1, 2): the relative error of an adder that may truncate

# impulse values.  With a lo part (bf16 kernels): value x bf16 weight has at most 11 + 8 significant bits, exact in fp32.
VALUES_LO = np.array([1.0 + 2.0 ** -10, -(3.0 + 2.0 ** -9), 96.0 + 2.0 ** -3, 1.0, -1.0, 2.0, 0.5], np.float32)
# powers of two (fp32 stem, fused split kernel): a scaling of the 24-bit weight, or of w_hi + w_lo, is exact
VALUES_POW2 = np.array([1.0, -1.0, 2.0, 0.5, -4.0, 0.25, 64.0], np.float32)


def geometry(h, w):
    """(oh, ow, ph, pw): stem plane and pooled plane (without its border) of an H x W frame."""
    oh, ow = (h - 7) // 2 + 1, (w - 7) // 2 + 1
    return oh, ow, (oh - 1) // 2 + 1, (ow + 1) // 2 + 1


def bf16_round(x):
    """float32 -> nearest-even bfloat16 -> float32 (finite inputs)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def split_hi_lo(x):
    """x -> (hi, lo): hi = bf16(x), lo = bf16(x - hi), the subtraction in fp32 (exact: Sterbenz-like, hi is x's leading bits)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = bf16_round(x)
    return hi, bf16_round(x - hi)


def patches(x):
    """[B,H,W,3] -> [B,oh,ow,147] float64, the 7x7 s2 VALID windows in (ky, kx, ci) order."""
    x = np.asarray(x, np.float64)
    b, h, w, _ = x.shape
    oh, ow = (h - 7) // 2 + 1, (w - 7) // 2 + 1
    out = np.empty((b, oh, ow, 7, 7, 3), np.float64)
    for ky in range(7):
        for kx in range(7):
            out[:, :, :, ky, kx, :] = x[:, ky:ky + 2 * (oh - 1) + 1:2, kx:kx + 2 * (ow - 1) + 1:2, :]
    return out.reshape(b, oh, ow, 147)


def conv(x, w):
    """Pre-bias sums of the stem convolution in float64: x [B,H,W,3], w [7,7,3,64] -> [B,oh,ow,64]."""
    return patches(x) @ np.asarray(w, np.float64).reshape(147, 64)


def relu(x):
    return np.maximum(x, 0.0)


def pool(x):
    """ZeroPadding2D((1,2)) + MaxPool 3x3 s2 VALID on [B,ih,iw,C]; keeps the dtype (a maximum is exact)."""
    x = np.pad(x, ((0, 0), (1, 1), (2, 2), (0, 0)))
    _, h, w, _ = x.shape
    oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    out = None
    for ky in range(3):
        for kx in range(3):
            p = x[:, ky:ky + 2 * (oh - 1) + 1:2, kx:kx + 2 * (ow - 1) + 1:2, :]
            out = p if out is None else np.maximum(out, p)
    return out


def pairs_split(plane):
    """[..., 128] pair slots in storage order -> (hi, lo) [..., 64]: 32 hi then 32 lo per 64-slot group."""
    p = np.asarray(plane).reshape(plane.shape[:-1] + (2, 2, 32))
    return p[..., 0, :].reshape(plane.shape[:-1] + (64,)), p[..., 1, :].reshape(plane.shape[:-1] + (64,))


def pairs_of(v):
    """fp32 [..., 64] -> the 128 slots a pair pixel stores: hi = bf16(v), lo = bf16(v - hi)."""
    hi, lo = split_hi_lo(v)
    g = np.stack([hi.reshape(v.shape[:-1] + (2, 32)), lo.reshape(v.shape[:-1] + (2, 32))], axis=-2)
    return g.reshape(v.shape[:-1] + (128,))


def unreached(h, w):
    """(last row unread, last column unread): an odd H - 7 / W - 7 leaves one input row / column outside every window."""
    return (h - 7) % 2 == 1, (w - 7) % 2 == 1


def poison_unreached(img, rng):
    """+-1e30 (finite after the hi / lo split) into the input row and column no window reaches."""
    _, h, w, _ = img.shape
    row, col = unreached(h, w)
    if row:
        img[:, h - 1] = np.where(rng.uniform(size=img[:, h - 1].shape) < 0.5, 1e30, -1e30)
    if col:
        img[:, :, w - 1] = np.where(rng.uniform(size=img[:, :, w - 1].shape) < 0.5, 1e30, -1e30)
    return img


def impulse_image(b, h, w, values, rng):
    """Zero except on a grid of spacing 7 with a random phase: every 7x7 window holds exactly one impulse, in a random channel,
    with a value drawn from `values`."""
    img = np.zeros((b, h, w, 3), np.float32)
    py, px = int(rng.integers(0, 7)), int(rng.integers(0, 7))
    ys, xs = np.arange(py, h, 7), np.arange(px, w, 7)
    for i in range(b):
        for y in ys:
            ch = rng.integers(0, 3, xs.size)
            img[i, y, xs, ch] = values[rng.integers(0, values.size, xs.size)]
    return poison_unreached(img, rng)


def random_image(b, h, w, rng):
    """Integers 0..255 minus the channel means, every row its own content."""
    img = rng.integers(0, 256, (b, h, w, 3)).astype(np.float32) - MEANS
    return poison_unreached(img, rng)


def random_weights(rng):
    w = (rng.normal(0, 1, (7, 7, 3, 64)) * np.sqrt(2.0 / 147)).astype(np.float32)
    return w, rng.normal(0, 0.5, 64).astype(np.float32)


def clean(img):
    """The image with the unreached row / column zeroed (what the operand-wise references may safely square or take |.| of)."""
    _, h, w, _ = img.shape
    row, col = unreached(h, w)
    img = np.array(img, np.float32)
    if row:
        img[:, h - 1] = 0
    if col:
        img[:, :, w - 1] = 0
    return img


# ---------------------------------------------------------------------------------------------- operands per kernel family
def operands(kind, img, w):
    """The float64 operands of the reference, per family: 'bf16' (the three bf16 kernels and the bf16 fused kernels): x_hi + x_lo
    times the bf16-rounded weights; 'fp32' and 'split': the fp32 operands as they are."""
    img = clean(img)
    if kind == "bf16":
        hi, lo = split_hi_lo(img)
        return hi.astype(np.float64) + lo.astype(np.float64), bf16_round(w).astype(np.float64)
    return img.astype(np.float64), np.asarray(w, np.float32).astype(np.float64)


def split_weights_sum(w):
    """w_hi + w_lo of the fused split kernel, float64 (exactly representable in fp32: both lie inside w's 24-bit window)."""
    hi, lo = split_hi_lo(w)
    return hi.astype(np.float64) + lo.astype(np.float64)


def bound(kind, img, w, bias):
    """(ref, e) of the pre-ReLU stem output: ref = sum + bias in float64 on the family's operands, e the derived error bound.
    mag = sum |x_k w_k| + |b|.  bf16: 294 non-zero products + 1 -> 295 * 2^-23 * mag; fp32: 147 + 1 -> 148 * 2^-23 * mag (a chain of
    fp32 adders that may truncate loses at most one ulp of the running magnitude per addition); split: x and w are each replaced
    by hi + lo (a relative error of at most 2^-18 each: the lo half rounds the residue below 2^-9 to eight bits) and the lo x lo
    product (at most 2^-9 * 2^-9 = 2^-18) is dropped -- three terms, together below 2^-16 * mag --, then 441 products + 1."""
    xo, wo = operands(kind, img, w)
    b = np.asarray(bias, np.float64)
    ref = conv(xo, wo) + b
    mag = conv(np.abs(xo), np.abs(wo)) + np.abs(b)
    n = {"bf16": 295, "fp32": 148, "split": 442}[kind]
    e = n * U * mag
    if kind == "split":
        e = e + 2.0 ** -16 * mag
    return ref, e


def impulse_expected(kind, img, w, bias):
    """The stem plane of an impulse image, exactly: relu(float32(sum) + b) in fp32 (one rounding), rounded to bf16 where the kernel
    stores bf16.  Returns (plane float32, the float64 sums): the host test asserts float32(sum) == sum."""
    xo, wo = operands(kind, img, w)
    if kind == "split":
        wo = split_weights_sum(w)
    s = conv(xo, wo)
    v = np.maximum(s.astype(np.float32) + np.asarray(bias, np.float32), np.float32(0))
    return (bf16_round(v) if kind == "bf16" else v), s

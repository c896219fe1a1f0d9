"""NumPy restatement of the corruption ops of include/bayesod.h: integers, or float32 with the stated operation
order, so the device result is ``array_equal``.  GAUSSIAN_NOISE is restated in float64 from the same exact uniforms; its test
allows what float32 libm may differ by.  Counters go through oracle/philox.py."""
import numpy as np

from oracle import philox

NONE, LUT, CONTRAST, IMPULSE_NOISE, GAUSSIAN_NOISE, CONV2D, PIXELATE, JPEG, FOG = range(9)
CORRUPT_TAG = 0x00C02200


def _key(seed):
    return int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF


def _pixel_words(h, w, slot, frame_id, seed):
    y, x = np.mgrid[0:h, 0:w].astype(np.uint64)
    return philox.philox4x32_10(x, y, np.uint64(CORRUPT_TAG | slot), np.uint64(int(frame_id) & 0xFFFFFFFF), *_key(seed))


def lut(frame, table):
    out = np.empty_like(frame)
    for c in range(3):
        out[..., c] = table[c][frame[..., c]]
    return out


def contrast(frame, k):
    h, w = frame.shape[:2]
    out = np.empty_like(frame)
    k = np.float32(k)
    for c in range(3):
        s = int(frame[..., c].astype(np.uint64).sum())
        m = np.float32(np.float64(s) / np.float64(h * w))
        v = frame[..., c].astype(np.float32)
        t = ((v - m).astype(np.float32) * k).astype(np.float32)
        t = (t + m).astype(np.float32)
        out[..., c] = np.rint(np.minimum(np.maximum(t, np.float32(0)), np.float32(255))).astype(np.uint8)
    return out


def impulse_noise(frame, T, slot, frame_id, seed):
    h, w = frame.shape[:2]
    words = _pixel_words(h, w, slot, frame_id, seed)
    out = frame.copy()
    for c in range(3):
        wd = words[c]
        hit = wd.astype(np.uint64) < np.uint64(T)
        out[..., c] = np.where(hit, np.where(wd & np.uint32(1), 255, 0).astype(np.uint8), frame[..., c])
    return out


def _unit(t):
    return ((t >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gaussian_noise_f64(frame, sigma, slot, frame_id, seed):
    """The pre-rounding float64 values [h,w,3]: v + sigma * n, clamped to [0, 255]; sigma as the float32 the record holds."""
    h, w = frame.shape[:2]
    x, y, z, ww = _pixel_words(h, w, slot, frame_id, seed)
    r0, t0 = np.sqrt(-2.0 * np.log(_unit(x))), 2.0 * np.pi * _unit(y)
    r1, t1 = np.sqrt(-2.0 * np.log(_unit(z))), 2.0 * np.pi * _unit(ww)
    n = np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1)], axis=-1)
    return np.clip(frame.astype(np.float64) + float(np.float32(sigma)) * n, 0.0, 255.0)


def gaussian_noise(frame, sigma, slot, frame_id, seed):
    return np.rint(gaussian_noise_f64(frame, sigma, slot, frame_id, seed)).astype(np.uint8)


def conv2d(frame, taps):
    taps = np.asarray(taps, np.uint32)
    K = taps.shape[0]
    r = K // 2
    h, w = frame.shape[:2]
    acc = np.zeros((h, w, 3), np.uint32)
    ys, xs = np.arange(h), np.arange(w)
    src = frame.astype(np.uint32)
    for ky in range(K):
        yy = np.clip(ys + ky - r, 0, h - 1)
        for kx in range(K):
            if taps[ky, kx]:
                xx = np.clip(xs + kx - r, 0, w - 1)
                acc += taps[ky, kx] * src[yy][:, xx]
    return ((acc + np.uint32(1 << 14)) >> np.uint32(15)).astype(np.uint8)


def pixelate(frame, f):
    h, w = frame.shape[:2]
    out = np.empty_like(frame)
    for y0 in range(0, h, f):
        for x0 in range(0, w, f):
            blk = frame[y0:y0 + f, x0:x0 + f].astype(np.int64)
            n = blk.shape[0] * blk.shape[1]
            out[y0:y0 + f, x0:x0 + f] = ((blk.sum(axis=(0, 1)) + n // 2) // n).astype(np.uint8)
    return out


def _descale(x, s):
    return (x + (1 << (s - 1))) >> s


def _fdct_1d(d, pass2):
    """jfdctint.c along the last axis of an int64 array [..., 8]."""
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    sh = 15 if pass2 else 11
    o = [None] * 8
    o[0] = _descale(t10 + t11, 2) if pass2 else (t10 + t11) << 2
    o[4] = _descale(t10 - t11, 2) if pass2 else (t10 - t11) << 2
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, sh)
    o[6] = _descale(z1 - t12 * 15137, sh)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    a4, a5, a6, a7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = _descale(a4 + z1 + z3, sh), _descale(a5 + z2 + z4, sh), _descale(a6 + z2 + z3, sh), _descale(a7 + z1 + z4, sh)
    return np.stack(o, axis=-1)


def _idct_1d(x):
    """jidctint.c along the last axis of an int64 array [..., 8], without the descale."""
    x = [x[..., i] for i in range(8)]
    z1 = (x[2] + x[6]) * 4433
    t2, t3 = z1 - x[6] * 15137, z1 + x[2] * 6270
    t0, t1 = (x[0] + x[4]) << 13, (x[0] - x[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a, b, c, d = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = a + d, b + c, a + c, b + d
    z5 = (z3 + z4) * 9633
    a, b, c, d = a * 2446, b * 16819, c * 25172, d * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    a, b, c, d = a + z1 + z3, b + z2 + z4, c + z2 + z3, d + z1 + z4
    return np.stack([t10 + d, t11 + c, t12 + b, t13 + a, t13 - a, t12 - b, t11 - c, t10 - d], axis=-1)


def _fix(x):
    return int(x * 65536 + 0.5)


def jpeg_forward(frame, qtables):
    """Quantised coefficients int64 [3, bh, bw, 8, 8] (natural order) of the 4:4:4 forward path."""
    h, w = frame.shape[:2]
    bh, bw = (h + 7) // 8, (w + 7) // 8
    pad = frame[np.minimum(np.arange(bh * 8), h - 1)][:, np.minimum(np.arange(bw * 8), w - 1)].astype(np.int64)
    R, G, B = pad[..., 0], pad[..., 1], pad[..., 2]
    Y = (_fix(.299) * R + _fix(.587) * G + _fix(.114) * B + 32768) >> 16
    Cb = (-_fix(.16874) * R - _fix(.33126) * G + _fix(.5) * B + (128 << 16) + 32767) >> 16
    Cr = (_fix(.5) * R - _fix(.41869) * G - _fix(.08131) * B + (128 << 16) + 32767) >> 16
    q = np.asarray(qtables, np.int64).reshape(2, 8, 8)
    out = []
    for ci, pl in enumerate((Y, Cb, Cr)):
        blk = (pl - 128).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)                  # [bh, bw, row, col]
        blk = _fdct_1d(blk, False)                                                   # rows: along col
        blk = _fdct_1d(blk.transpose(0, 1, 3, 2), True).transpose(0, 1, 3, 2)         # columns: along row
        q8 = 8 * q[1 if ci else 0]
        out.append(np.sign(blk) * ((np.abs(blk) + (q8 >> 1)) // q8))
    return np.stack(out)


def jpeg_inverse(coefs, qtables, h, w):
    """The decoder's half: dequantise, jidctint (columns, then rows), clamp, YCbCr -> RGB."""
    q = np.asarray(qtables, np.int64).reshape(2, 8, 8)
    planes = []
    for ci in range(3):
        blk = coefs[ci] * q[1 if ci else 0]
        blk = _descale(_idct_1d(blk.transpose(0, 1, 3, 2)), 11).transpose(0, 1, 3, 2)  # pass 1: columns
        blk = np.clip(_descale(_idct_1d(blk), 18) + 128, 0, 255)                      # pass 2: rows
        bh, bw = blk.shape[:2]
        planes.append(blk.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)[:h, :w])
    Y, cb, cr = planes[0], planes[1] - 128, planes[2] - 128
    R = np.clip(Y + ((91881 * cr + 32768) >> 16), 0, 255)
    B = np.clip(Y + ((116130 * cb + 32768) >> 16), 0, 255)
    G = np.clip(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16), 0, 255)
    return np.stack([R, G, B], axis=-1).astype(np.uint8)


def jpeg(frame, qtables):
    h, w = frame.shape[:2]
    return jpeg_inverse(jpeg_forward(frame, qtables), qtables, h, w)


def fog(frame, a, slot, frame_id, seed):
    h, w = frame.shape[:2]
    y, x = np.mgrid[0:h, 0:w].astype(np.uint64)
    F = np.zeros((h, w), np.uint64)
    k0, k1 = _key(seed)
    fid = np.uint64(int(frame_id) & 0xFFFFFFFF)
    for s in range(7, 1, -1):
        S = np.uint64(1 << s)
        c2 = np.uint64(CORRUPT_TAG | slot | (s << 4))
        ny, nx = ((h - 1) >> s) + 2, ((w - 1) >> s) + 2
        ly, lx = np.mgrid[0:ny, 0:nx].astype(np.uint64)
        lat = (philox.philox4x32_10(lx, ly, c2, fid, k0, k1)[0] >> np.uint32(16)).astype(np.uint64)
        ix, iy = (x >> np.uint64(s)).astype(np.int64), (y >> np.uint64(s)).astype(np.int64)
        fx, fy = x & (S - np.uint64(1)), y & (S - np.uint64(1))
        v00, v01, v10, v11 = lat[iy, ix], lat[iy, ix + 1], lat[iy + 1, ix], lat[iy + 1, ix + 1]
        b = (v00 * (S - fx) + v01 * fx) * (S - fy) + (v10 * (S - fx) + v11 * fx) * fy
        assert int(b.max()) <= 1 << 30
        F += (b >> np.uint64(2 * s)) >> np.uint64(7 - s)
    assert int(F.max()) < 1 << 17
    t = (np.uint64(int(a)) * F) >> np.uint64(17)
    v = frame.astype(np.uint64)
    return ((v * (np.uint64(256) - t)[..., None] + np.uint64(255) * t[..., None] + np.uint64(128)) >> np.uint64(8)).astype(np.uint8)


def apply_op(frame, op, slot, taps, luts, qtables, frame_id, seed):
    """One packed op record (``corruptions.OP_DTYPE``) on one frame."""
    kind = int(op["kind"])
    if kind == NONE:
        return frame.copy()
    if kind == LUT:
        return lut(frame, np.asarray(luts).reshape(-1, 3, 256)[int(op["table"])])
    if kind == CONTRAST:
        return contrast(frame, op["f0"])
    if kind == IMPULSE_NOISE:
        return impulse_noise(frame, int(op["u0"]), slot, frame_id, seed)
    if kind == GAUSSIAN_NOISE:
        return gaussian_noise(frame, op["f0"], slot, frame_id, seed)
    if kind == CONV2D:
        K, off = int(op["ksize"]), int(op["tap_offset"])
        return conv2d(frame, np.asarray(taps).reshape(-1)[off:off + K * K].reshape(K, K))
    if kind == PIXELATE:
        return pixelate(frame, int(op["u0"]))
    if kind == JPEG:
        return jpeg(frame, np.asarray(qtables).reshape(-1, 2, 64)[int(op["table"])])
    if kind == FOG:
        return fog(frame, int(op["u0"]), slot, frame_id, seed)
    raise ValueError("unknown kind %d" % kind)


def apply_packed(frames, ops, taps, luts, qtables, frame_ids=None, seed=0):
    """What bod_corrupt_frames_u8 computes for ``corruptions.pack``'s arrays."""
    out = []
    for i, f in enumerate(frames):
        fid = i if frame_ids is None else frame_ids[i]
        for j in range(ops.shape[1]):
            f = apply_op(f, ops[i, j], j, taps, luts, qtables, fid, seed)
        out.append(f)
    return out

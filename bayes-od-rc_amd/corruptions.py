"""Dataset-shift corruptions of the uint8 RGB source frames: the op chains ``bod_corrupt_frames_u8`` and
``bod_set_upload_corruption`` (include/bayesod.h) run on the device, built here on the host.  ``make(name, severity)`` returns a
``Chain`` -- 1 to 4 ops plus the tables they index; ``pack`` turns one chain per frame into the arrays of the C entry points.
The severity tables are this project's own choice, not ImageNet-C's."""
import math

import numpy as np

NONE, LUT, CONTRAST, IMPULSE_NOISE, GAUSSIAN_NOISE, CONV2D, PIXELATE, JPEG, FOG = range(9)
KIND_NAMES = ("NONE", "LUT", "CONTRAST", "IMPULSE_NOISE", "GAUSSIAN_NOISE", "CONV2D", "PIXELATE", "JPEG", "FOG")
MAX_OPS = 4
TAP_SUM = 1 << 15
MAX_KSIZE = 25

# bod_corrupt_op as a NumPy record
OP_DTYPE = np.dtype([("kind", "<i4"), ("f0", "<f4"), ("u0", "<u4"), ("tap_offset", "<i4"), ("ksize", "<i4"), ("table", "<i4"),
                     ("reserved", "<i4", (2,))])
assert OP_DTYPE.itemsize == 32


class Chain:
    """1..4 ops (dicts with the fields of ``OP_DTYPE``, missing ones 0) and the tables their ``tap_offset`` / ``table`` index:
    ``taps`` uint16 [T], ``luts`` uint8 [L,3,256], ``qtables`` uint16 [Q,2,64]."""

    def __init__(self, ops, taps=None, luts=None, qtables=None):
        self.ops = [dict(o) for o in ops]
        self.taps = np.zeros(0, np.uint16) if taps is None else np.ascontiguousarray(taps, np.uint16).reshape(-1)
        self.luts = np.zeros((0, 3, 256), np.uint8) if luts is None else np.ascontiguousarray(luts, np.uint8).reshape(-1, 3, 256)
        self.qtables = np.zeros((0, 2, 64), np.uint16) if qtables is None else np.ascontiguousarray(qtables, np.uint16).reshape(-1, 2, 64)

    def __len__(self):
        return len(self.ops)


# ---- ops ----------------------------------------------------------------------------------------------------------------------
def impulse_threshold(p):
    """T = floor(p * 2^32) in double, capped at 2^32 - 1 (p = 1 replaces every word but 0xFFFFFFFF)."""
    if not (0.0 <= p <= 1.0):
        raise ValueError("impulse probability %r outside [0, 1]" % (p,))
    return min(int(math.floor(float(p) * 4294967296.0)), 0xFFFFFFFF)


def op_none():
    return Chain([{"kind": NONE}])


def op_lut(lut):
    lut = np.ascontiguousarray(lut, np.uint8)
    if lut.shape == (256,):
        lut = np.stack([lut] * 3)
    return Chain([{"kind": LUT, "table": 0}], luts=lut.reshape(1, 3, 256))


def op_contrast(k):
    return Chain([{"kind": CONTRAST, "f0": float(k)}])


def op_impulse_noise(p):
    return Chain([{"kind": IMPULSE_NOISE, "u0": impulse_threshold(p)}])


def op_gaussian_noise(sigma):
    return Chain([{"kind": GAUSSIAN_NOISE, "f0": float(sigma)}])


def op_conv2d(taps):
    taps = np.ascontiguousarray(taps, np.uint16)
    if taps.ndim != 2 or taps.shape[0] != taps.shape[1]:
        raise ValueError("CONV2D taps must be a square array, got %s" % (taps.shape,))
    return Chain([{"kind": CONV2D, "tap_offset": 0, "ksize": int(taps.shape[0])}], taps=taps)


def op_pixelate(f):
    return Chain([{"kind": PIXELATE, "u0": int(f)}])


def op_jpeg(quality=None, qtables=None):
    q = jpeg_qtables(quality) if qtables is None else np.ascontiguousarray(qtables, np.uint16)
    return Chain([{"kind": JPEG, "table": 0}], qtables=q.reshape(1, 2, 64))


def op_fog(a):
    return Chain([{"kind": FOG, "u0": int(a)}])


def concat(*chains):
    """The chains one after the other as one chain (table indices and tap offsets shifted)."""
    ops, taps, luts, qts = [], [], [], []
    nt = nl = nq = 0
    for ch in chains:
        for o in ch.ops:
            o = dict(o)
            if o.get("kind") == CONV2D:
                o["tap_offset"] = int(o.get("tap_offset", 0)) + nt
            elif o.get("kind") == LUT:
                o["table"] = int(o.get("table", 0)) + nl
            elif o.get("kind") == JPEG:
                o["table"] = int(o.get("table", 0)) + nq
            ops.append(o)
        taps.append(ch.taps); luts.append(ch.luts); qts.append(ch.qtables)
        nt += ch.taps.size; nl += ch.luts.shape[0]; nq += ch.qtables.shape[0]
    if len(ops) > MAX_OPS:
        raise ValueError("a chain holds at most %d ops, got %d" % (MAX_OPS, len(ops)))
    return Chain(ops, np.concatenate(taps), np.concatenate(luts), np.concatenate(qts))


# ---- tables -------------------------------------------------------------------------------------------------------------------
def _round_levels(v):
    return np.clip(np.floor(np.asarray(v, np.float64) + 0.5), 0, 255).astype(np.uint8)


def lut_brightness(delta):
    return _round_levels(np.arange(256, dtype=np.float64) + float(delta))


def lut_gamma(gamma):
    return _round_levels(255.0 * (np.arange(256, dtype=np.float64) / 255.0) ** float(gamma))


def lut_contrast(k, pivot=128.0):
    return _round_levels((np.arange(256, dtype=np.float64) - pivot) * float(k) + pivot)


def quantise_taps(kernel):
    """A non-negative double kernel as uint16 taps that sum to exactly 2^15.  Largest remainder by symmetry orbit: the taps are
    floored, then every group of taps with one and the same value -- the mirror images of a tap have its value -- gains one unit,
    groups in the order of their remainders, while the whole group still fits; what is left goes to the centre tap, which is its
    own mirror image.  A kernel symmetric under a flip or a transposition stays so."""
    k = np.asarray(kernel, np.float64)
    if k.ndim != 2 or k.shape[0] != k.shape[1] or k.shape[0] % 2 != 1 or k.shape[0] > MAX_KSIZE:
        raise ValueError("kernel must be K x K with K odd and at most %d, got %s" % (MAX_KSIZE, k.shape))
    if not np.all(np.isfinite(k)) or np.any(k < 0) or k.sum() <= 0:
        raise ValueError("kernel must be finite, non-negative and not all zero")
    w = k / k.sum() * TAP_SUM
    q = np.floor(w).astype(np.int64)
    rem = w - q
    left = TAP_SUM - int(q.sum())
    values = np.unique(k[rem > 0])
    groups = sorted(((float(rem[k == v][0]), float(v)) for v in values), reverse=True)
    for _, v in groups:
        m = k == v
        size = int(m.sum())
        if size <= left:
            q[m] += 1
            left -= size
    c = k.shape[0] // 2
    q[c, c] += left
    assert q.sum() == TAP_SUM and q.max() <= 65535
    return q.astype(np.uint16)


def disk_kernel(radius):
    r = float(radius)
    c = int(math.floor(r))
    y, x = np.mgrid[-c:c + 1, -c:c + 1]
    return quantise_taps((x * x + y * y <= r * r + 1e-9).astype(np.float64))


def line_kernel(length, angle_deg=0.0):
    """A line of ``length`` (odd) unit samples through the centre, at ``angle_deg`` from the x axis (y grows downwards)."""
    n = int(length)
    if n < 1 or n % 2 != 1 or n > MAX_KSIZE:
        raise ValueError("line length must be odd and in 1..%d" % MAX_KSIZE)
    c = n // 2
    k = np.zeros((n, n), np.float64)
    dx, dy = math.cos(math.radians(angle_deg)), math.sin(math.radians(angle_deg))
    for t in range(-c, c + 1):
        k[c + int(math.floor(t * dy + 0.5)), c + int(math.floor(t * dx + 0.5))] += 1.0
    return quantise_taps(k)


def gaussian_kernel(sigma):
    s = float(sigma)
    c = min(int(math.ceil(3.0 * s)), MAX_KSIZE // 2)
    y, x = np.mgrid[-c:c + 1, -c:c + 1]
    return quantise_taps(np.exp(-((x * x + y * y).astype(np.float64)) / (2.0 * s * s)))


# ITU-T T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance), natural (row-major) order
JPEG_BASE_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
    np.int64)
JPEG_BASE_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99],
    np.int64)


def jpeg_qtables(quality):
    """uint16 [2,64] (luma, chroma; natural order) by libjpeg's quality scaling of the Annex K tables, baseline (entries 1..255)."""
    q = int(quality)
    if q < 1 or q > 100:
        raise ValueError("JPEG quality %r outside 1..100" % (quality,))
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((b * s + 50) // 100, 1, 255) for b in (JPEG_BASE_LUMA, JPEG_BASE_CHROMA)]).astype(np.uint16)


# ---- named corruptions --------------------------------------------------------------------------------------------------------
# severity 1..5 -> parameter (DESIGN.md 9.13 holds the same table)
SEVERITIES = {
    "gaussian_noise": (4.0, 8.0, 16.0, 24.0, 40.0),              # sigma, grey levels
    "impulse_noise": (0.01, 0.02, 0.05, 0.10, 0.20),             # probability per sample
    "defocus_blur": (1.5, 2.5, 4.0, 6.0, 9.0),                   # disk radius, pixels
    "motion_blur": (5, 9, 13, 19, 25),                           # horizontal line length, pixels
    "gaussian_blur": (0.8, 1.5, 2.5, 3.5, 4.0),                  # sigma, pixels
    "pixelate": (2, 3, 4, 6, 8),                                 # block size
    "jpeg_compression": (40, 25, 15, 10, 5),                     # quality
    "contrast": (0.75, 0.6, 0.45, 0.3, 0.15),                    # factor about the frame's channel means
    "brightness": (20.0, 40.0, 60.0, 80.0, 100.0),               # added grey levels
    "low_light": ((1.5, 2.0), (2.0, 3.0), (2.5, 4.0), (3.0, 6.0), (4.0, 8.0)),   # (gamma, sigma of the noise after it)
    "fog": (64, 112, 160, 208, 256),                             # strength a
}
NAMES = tuple(SEVERITIES)


def make(name, severity):
    """The chain of corruption ``name`` at ``severity`` 1..5."""
    if name not in SEVERITIES:
        raise ValueError("unknown corruption %r (one of: %s)" % (name, ", ".join(NAMES)))
    if isinstance(severity, bool) or not isinstance(severity, (int, np.integer)) or not 1 <= int(severity) <= 5:
        raise ValueError("severity must be an integer 1..5, got %r" % (severity,))
    p = SEVERITIES[name][int(severity) - 1]
    if name == "gaussian_noise":
        return op_gaussian_noise(p)
    if name == "impulse_noise":
        return op_impulse_noise(p)
    if name == "defocus_blur":
        return op_conv2d(disk_kernel(p))
    if name == "motion_blur":
        return op_conv2d(line_kernel(p))
    if name == "gaussian_blur":
        return op_conv2d(gaussian_kernel(p))
    if name == "pixelate":
        return op_pixelate(p)
    if name == "jpeg_compression":
        return op_jpeg(p)
    if name == "contrast":
        return op_contrast(p)
    if name == "brightness":
        return op_lut(lut_brightness(p))
    if name == "low_light":
        return concat(op_lut(lut_gamma(p[0])), op_gaussian_noise(p[1]))
    return op_fog(p)


def parse(text):
    """``NAME:SEVERITY`` (the drivers' ``--corrupt``) -> (name, severity); ``ValueError`` says what is wrong."""
    if not isinstance(text, str) or text.count(":") != 1:
        raise ValueError("expected NAME:SEVERITY, got %r" % (text,))
    name, sev = text.split(":")
    name = name.strip()
    if name not in SEVERITIES:
        raise ValueError("unknown corruption %r (one of: %s)" % (name, ", ".join(NAMES)))
    try:
        sev = int(sev.strip())
    except ValueError:
        raise ValueError("severity of %r must be an integer 1..5" % (text,))
    if not 1 <= sev <= 5:
        raise ValueError("severity of %r must be 1..5" % (text,))
    return name, sev


# ---- packing / validation -----------------------------------------------------------------------------------------------------
def pack(chains, n=None):
    """One chain per frame (or one ``Chain`` for all ``n`` frames) -> (ops ``OP_DTYPE`` [n, P], taps uint16, luts uint8 [L,3,256],
    qtables uint16 [Q,2,64]).  Shorter chains are padded with NONE; a chain object used for several frames is stored once."""
    if isinstance(chains, Chain):
        if n is None:
            raise ValueError("one chain for all frames needs the frame count")
        chains = [chains] * int(n)
    chains = list(chains)
    if n is not None and len(chains) != int(n):
        raise ValueError("expected %d chains, got %d" % (int(n), len(chains)))
    if not chains:
        raise ValueError("no chains to pack")
    P = max(len(c) for c in chains)
    if P < 1 or P > MAX_OPS:
        raise ValueError("a chain holds 1..%d ops, got %d" % (MAX_OPS, P))
    ops = np.zeros((len(chains), P), OP_DTYPE)
    base, taps, luts, qts = {}, [], [], []
    nt = nl = nq = 0
    for i, ch in enumerate(chains):
        if id(ch) not in base:
            base[id(ch)] = (nt, nl, nq)
            taps.append(ch.taps); luts.append(ch.luts); qts.append(ch.qtables)
            nt += ch.taps.size; nl += ch.luts.shape[0]; nq += ch.qtables.shape[0]
        bt, bl, bq = base[id(ch)]
        for j, o in enumerate(ch.ops):
            r = ops[i, j]
            for key in ("kind", "f0", "u0", "tap_offset", "ksize", "table"):
                r[key] = o.get(key, 0)
            if r["kind"] == CONV2D:
                r["tap_offset"] += bt
            elif r["kind"] == LUT:
                r["table"] += bl
            elif r["kind"] == JPEG:
                r["table"] += bq
    return (ops, np.ascontiguousarray(np.concatenate(taps), np.uint16), np.ascontiguousarray(np.concatenate(luts), np.uint8),
            np.ascontiguousarray(np.concatenate(qts), np.uint16))


def validate(ops, taps, luts, qtables):
    """The C side's validation rules (corrupt_spec_make) restated: ``ValueError`` naming the frame and the op."""
    ops = np.asarray(ops)
    if ops.ndim != 2 or not 1 <= ops.shape[1] <= MAX_OPS:
        raise ValueError("ops_per_frame outside 1..%d" % MAX_OPS)
    taps = np.asarray(taps).reshape(-1)
    n_luts, n_q = np.asarray(luts).reshape(-1, 3, 256).shape[0], np.asarray(qtables).reshape(-1, 2, 64).shape[0]
    for i in range(ops.shape[0]):
        for j in range(ops.shape[1]):
            o, at = ops[i, j], "frame %d op %d: " % (i, j)
            kind, f0, u0 = int(o["kind"]), float(o["f0"]), int(o["u0"])
            if kind in (NONE, IMPULSE_NOISE):
                continue
            if kind == LUT:
                if not 0 <= int(o["table"]) < n_luts:
                    raise ValueError(at + "LUT table outside the tables given")
            elif kind == CONTRAST:
                if not math.isfinite(f0):
                    raise ValueError(at + "contrast factor is not finite")
            elif kind == GAUSSIAN_NOISE:
                if not math.isfinite(f0) or f0 < 0 or f0 > 128:
                    raise ValueError(at + "sigma is not in [0, 128]")
            elif kind == CONV2D:
                K, off = int(o["ksize"]), int(o["tap_offset"])
                if K < 1 or K > MAX_KSIZE or K % 2 == 0:
                    raise ValueError(at + "kernel size %d is not odd and in 1..25" % K)
                if off < 0 or off + K * K > taps.size:
                    raise ValueError(at + "taps lie past the table")
                if int(taps[off:off + K * K].astype(np.int64).sum()) != TAP_SUM:
                    raise ValueError(at + "the taps do not sum to 2^15")
            elif kind == PIXELATE:
                if not 2 <= u0 <= 64:
                    raise ValueError(at + "block size %d outside 2..64" % u0)
            elif kind == JPEG:
                if not 0 <= int(o["table"]) < n_q:
                    raise ValueError(at + "quantisation table outside the tables given")
                if np.any(np.asarray(qtables).reshape(-1, 2, 64)[int(o["table"])] == 0):
                    raise ValueError(at + "a quantisation entry is zero")
            elif kind == FOG:
                if u0 > 256:
                    raise ValueError(at + "fog strength %d above 256" % u0)
            else:
                raise ValueError(at + "unknown kind %d" % kind)

"""The PNG decoder tests' corpus, built in memory from seeded arrays: PNG is lossless, so the expected RGB of a case
is the array it was written from and no golden file is needed.  ``write_png`` is a test-side writer that forces a filter type per row
(the five of the PNG specification's section 9, cycled from a pattern), a deflate mode and the sizes of the IDAT chunks; PIL-written
files of the same arrays (adaptive filters) join it where PIL imports."""
import io
import struct
import zlib

import numpy as np

SIZES = [(1, 1), (1, 7), (5, 1), (9, 13), (64, 3), (65, 33), (130, 17), (1030, 5)]     # (height, width); 1030 rows: taller than a band
COLOR_TYPES = [0, 2, 4, 6]
CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}
PIL_MODES = {0: "L", 2: "RGB", 4: "LA", 6: "RGBA"}
PATTERNS = [[0], [1], [2], [3], [4], [4, 3, 2, 1, 0], [3, 4]]
DEFLATE = ["stored", "level6", "level9", "fixed"]
IDAT_SPLITS = [1, 7, 4096]
_cache = {}


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def filter_rows(rows, bpp, pattern):
    """rows uint8 [h, w * bpp] -> the filtered scanlines uint8 [h, 1 + w * bpp], row r by filter type pattern[r % len(pattern)]."""
    h, n = rows.shape
    x = rows.astype(np.int32)
    out = np.zeros((h, 1 + n), np.uint8)
    for r in range(h):
        ft = pattern[r % len(pattern)]
        a = np.concatenate([np.zeros(bpp, np.int32), x[r, :n - bpp]]) if n > bpp else np.zeros(n, np.int32)
        b = x[r - 1] if r else np.zeros(n, np.int32)
        c = (np.concatenate([np.zeros(bpp, np.int32), b[:n - bpp]]) if n > bpp else np.zeros(n, np.int32)) if r else np.zeros(n, np.int32)
        if ft == 0:
            pred = 0
        elif ft == 1:
            pred = a
        elif ft == 2:
            pred = b
        elif ft == 3:
            pred = (a + b) >> 1
        else:                        # 4: Paeth; any other value (the corruption tests' 5) is written with Paeth's bytes
            p = a + b - c
            pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        out[r, 0] = ft
        out[r, 1:] = (x[r] - pred) & 255
    return out


def deflate(raw, mode):
    if mode == "stored":
        return zlib.compress(raw, 0)
    if mode == "fixed":
        co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
        return co.compress(raw) + co.flush()
    return zlib.compress(raw, {"level6": 6, "level9": 9}[mode])


def assemble(width, height, color_type, zdata, idat_split=None, before_idat=(), bit_depth=8, interlace=0):
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, bit_depth, color_type, 0, 0, interlace))
    for kind, data in before_idat:
        out += chunk(kind, data)
    step = len(zdata) if not idat_split else idat_split
    for first in range(0, len(zdata), max(step, 1)):
        out += chunk(b"IDAT", zdata[first:first + step])
    return out + chunk(b"IEND", b"")


def write_png(arr, color_type, pattern, mode="level6", idat_split=None, before_idat=()):
    """arr uint8 [h, w, channels of the colour type] -> the file's bytes."""
    h, w, ch = arr.shape
    assert ch == CHANNELS[color_type]
    raw = filter_rows(arr.reshape(h, w * ch), ch, pattern).tobytes()
    return assemble(w, h, color_type, deflate(raw, mode), idat_split, before_idat)


def expected_rgb(arr, color_type):
    """What PIL's convert('RGB') gives: RGB as it is, RGBA without alpha, gray (with or without alpha) three times."""
    if color_type in (2, 6):
        return np.ascontiguousarray(arr[:, :, :3])
    return np.ascontiguousarray(np.repeat(arr[:, :, :1], 3, axis=2))


def make_array(h, w, color_type, seed):
    """Noise on a gradient: every filter type gets neighbours that differ, Paeth all three of its branches."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ch = CHANNELS[color_type]
    base = np.stack([(3 * xx + 5 * yy * (k + 1) + 40 * k) % 256 for k in range(ch)], axis=2)
    noise = rng.integers(-24, 25, (h, w, ch))
    wild = rng.integers(0, 256, (h, w, ch))
    return np.where(rng.random((h, w, 1)) < 0.1, wild, (base + noise) % 256).astype(np.uint8)


def idat_stream(data):
    """The concatenated IDAT data of a file (no CRC check)."""
    pos, z = 8, b""
    while pos + 8 <= len(data):
        n, kind = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        if kind == b"IDAT":
            z += data[pos + 8:pos + 8 + n]
        pos += 12 + n
    return z


class Case:
    def __init__(self, index, data, rgb, arr, color_type, pattern, mode, split):
        self.index, self.data, self.rgb, self.arr = index, data, rgb, arr
        self.height, self.width = rgb.shape[:2]
        self.color_type, self.pattern, self.mode, self.split = color_type, pattern, mode, split

    def __repr__(self):
        return "case %d: %dx%d colour type %d filters %s %s idat %s" % (self.index, self.height, self.width, self.color_type, self.pattern,
                                                                      self.mode, self.split)


def load():
    """-> the list of cases.  Every size x colour type x filter pattern, the deflate modes and IDAT chunk sizes rotating through them
    (each meets every size, colour type and pattern); every deflate mode x IDAT chunk size x colour type at 9x13 with all five filters;
    PIL's own files of every size x colour type."""
    if "v" in _cache:
        return _cache["v"]
    cases = []

    def add(arr, ct, data, pattern, mode, split):
        rgb = expected_rgb(arr, ct)
        rgb.setflags(write=False)
        cases.append(Case(len(cases), data, rgb, arr, ct, pattern, mode, split))
    k = 0
    for si, (h, w) in enumerate(SIZES):
        for ct in COLOR_TYPES:
            arr = make_array(h, w, ct, 100 * si + ct)
            for pi, pattern in enumerate(PATTERNS):
                mode, split = DEFLATE[(k + pi + si) % 4], IDAT_SPLITS[(k + ct // 2 + si) % 3]
                add(arr, ct, write_png(arr, ct, pattern, mode, split), pattern, mode, split)
                k += 1
    for ct in COLOR_TYPES:
        arr = make_array(9, 13, ct, 900 + ct)
        for mode in DEFLATE:
            for split in IDAT_SPLITS + [None]:
                add(arr, ct, write_png(arr, ct, [4, 3, 2, 1, 0], mode, split), [4, 3, 2, 1, 0], mode, split)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        for si, (h, w) in enumerate(SIZES):
            for ct in COLOR_TYPES:
                arr = make_array(h, w, ct, 100 * si + ct)
                buf = io.BytesIO()
                im = Image.fromarray(arr[:, :, 0] if ct == 0 else arr)
                assert im.mode == PIL_MODES[ct]
                im.save(buf, "PNG")
                add(arr, ct, buf.getvalue(), "pil", "pil", "pil")
    _cache["v"] = cases
    return cases


def single_code_stream(raw):
    """A zlib stream no zlib writes but zlib's inflate accepts: ``raw`` in stored blocks, then a final dynamic block whose
    literal/length set is the end-of-block code alone (one code of length 1) and whose distance set is one code of length 1."""
    bits = []

    def put(value, n):
        bits.extend((value >> k) & 1 for k in range(n))
    put(1, 1), put(2, 2), put(0, 5), put(0, 5), put(14, 4)              # final, dynamic, 257 literal/length codes, 1 distance code, 18 lengths
    for sym in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1):
        put(1 if sym in (18, 1) else 0, 3)                               # code-length code: symbol 1 -> '0', symbol 18 -> '1'
    put(1, 1), put(138 - 11, 7), put(1, 1), put(118 - 11, 7)            # 256 zero lengths
    put(0, 1), put(0, 1)                                                # length 1 for symbol 256, length 1 for distance code 0
    put(0, 1)                                                           # end of block
    bits.extend([0] * (-len(bits) % 8))
    tail = bytes(sum(b << k for k, b in enumerate(bits[i:i + 8])) for i in range(0, len(bits), 8))
    out = b"\x78\x01"
    for first in range(0, len(raw), 65535):
        part = raw[first:first + 65535]
        out += b"\x00" + struct.pack("<HH", len(part), len(part) ^ 0xFFFF) + part
    return out + tail + struct.pack(">I", zlib.adler32(raw) & 0xFFFFFFFF)


def unsupported_files():
    """name -> (bytes, a word of the reason): well-formed files outside the supported subset."""
    rgb = make_array(4, 6, 2, 7)
    raw = filter_rows(rgb.reshape(4, 18), 3, [0]).tobytes()
    z = zlib.compress(raw)
    out = {}
    pal_rows = np.zeros((4, 7), np.uint8)
    pal_rows[:, 1:] = np.arange(24).reshape(4, 6) % 4
    out["palette"] = (assemble(6, 4, 3, zlib.compress(pal_rows.tobytes()), before_idat=[(b"PLTE", bytes(range(12)))]), "palette")
    raw16 = np.zeros((4, 1 + 12), np.uint8)
    raw16[:, 1:] = make_array(4, 6, 4, 8).reshape(4, 12)
    out["16-bit"] = (assemble(6, 4, 0, zlib.compress(raw16.tobytes()), bit_depth=16), "bit depth 16")
    raw4 = np.zeros((4, 1 + 3), np.uint8)
    raw4[:, 1:] = make_array(4, 3, 0, 9).reshape(4, 3)
    out["bit depth 4"] = (assemble(6, 4, 0, zlib.compress(raw4.tobytes()), bit_depth=4), "bit depth 4")
    one = zlib.compress(bytes([0, 10, 20, 30]))                     # a 1x1 frame: Adam7's first pass is the whole image
    out["interlaced"] = (assemble(1, 1, 2, one, interlace=1), "interlaced")
    out["tRNS"] = (assemble(6, 4, 2, z, before_idat=[(b"tRNS", bytes(6))]), "tRNS")
    out["acTL"] = (assemble(6, 4, 2, z, before_idat=[(b"acTL", struct.pack(">II", 1, 0))]), "acTL")
    return out


def corrupt_files():
    """name -> (bytes, a word of the message): files every entry point that inflates must refuse."""
    arr = make_array(6, 5, 2, 11)
    h, w = 6, 5
    good = write_png(arr, 2, [4, 1])
    raw = filter_rows(arr.reshape(h, w * 3), 3, [4, 1])
    z = zlib.compress(raw.tobytes())
    out = {}
    at = good.index(b"IDAT")
    n = struct.unpack(">I", good[at - 4:at])[0]
    flipped = bytearray(good)
    flipped[at + 4 + n] ^= 0x40                                      # first byte of the IDAT chunk's CRC
    out["flipped CRC"] = (bytes(flipped), "CRC")
    out["flipped Adler-32"] = (assemble(w, h, 2, z[:-1] + bytes([z[-1] ^ 1])), "Adler")
    out["truncated file"] = (good[:at + 4 + n // 2], "truncated")
    out["truncated IDAT"] = (assemble(w, h, 2, z[:len(z) // 2]), "truncated")
    bad_filter = raw.copy()
    bad_filter[3, 0] = 5
    out["filter byte 5"] = (assemble(w, h, 2, zlib.compress(bad_filter.tobytes())), "filter type")
    out["one row short"] = (assemble(w, h, 2, zlib.compress(raw[:-1].tobytes())), "fewer bytes")
    out["one byte long"] = (assemble(w, h, 2, zlib.compress(raw.tobytes() + b"\x00")), "more bytes")
    return out, good

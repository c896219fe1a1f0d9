"""NumPy restatement, in int64, of the baseline JPEG decoder of DESIGN.md 9.11: marker parsing and Huffman decoding (the library's
host half, csrc/jpeg_entropy.h) and dequantisation, libjpeg's "islow" inverse DCT, "fancy" chroma upsampling and YCbCr -> RGB (its
device half, csrc/jpeg_kernels.hip).  Written from the specification (ITU-T T.81 and the arithmetic listed in DESIGN.md 9.11), for
the tests only: the product never imports it.  It covers valid streams of the supported subset and asserts on anything else."""
import numpy as np

ZIGZAG_TO_NATURAL = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def _huff_table(counts, vals):
    """16-bit window -> (length, symbol) for the canonical code of T.81 C.2 (length 0: no code)."""
    length = np.zeros(65536, np.int64)
    symbol = np.zeros(65536, np.int64)
    code, k = 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            first = code << (16 - l)
            length[first:first + (1 << (16 - l))] = l
            symbol[first:first + (1 << (16 - l))] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return length, symbol


def parse(data):
    """SOI .. SOS of a supported stream."""
    d = bytes(data)
    assert d[:2] == b"\xff\xd8", "no SOI"
    pos = 2
    info = {"restart_interval": 0}
    qt, huff = {}, {}
    while True:
        assert d[pos] == 0xFF
        m = d[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        pos += 2
        seg = (d[pos] << 8) | d[pos + 1]
        p = d[pos + 2:pos + seg]
        if m == 0xC0:
            assert p[0] == 8
            info["height"], info["width"], nc = (p[1] << 8) | p[2], (p[3] << 8) | p[4], p[5]
            info["comps"] = [{"id": p[6 + 3 * c], "h": p[7 + 3 * c] >> 4, "v": p[7 + 3 * c] & 15, "tq": p[8 + 3 * c]} for c in range(nc)]
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise AssertionError("SOF%d is not baseline" % (m - 0xC0))
        elif m == 0xDB:
            q = 0
            while q < len(p):
                assert p[q] >> 4 == 0
                t = np.zeros(64, np.int64)
                t[ZIGZAG_TO_NATURAL] = np.frombuffer(p[q + 1:q + 65], np.uint8)
                qt[p[q] & 15] = t
                q += 65
        elif m == 0xC4:
            q = 0
            while q < len(p):
                counts = list(p[q + 1:q + 17])
                n = sum(counts)
                huff[(p[q] >> 4, p[q] & 15)] = _huff_table(counts, list(p[q + 17:q + 17 + n]))
                q += 17 + n
        elif m == 0xDD:
            info["restart_interval"] = (p[0] << 8) | p[1]
        elif m == 0xDA:
            ns = p[0]
            assert ns == len(info["comps"]), "not one interleaved scan"
            for c in range(ns):
                assert p[1 + 2 * c] == info["comps"][c]["id"]
                info["comps"][c]["td"], info["comps"][c]["ta"] = p[2 + 2 * c] >> 4, p[2 + 2 * c] & 15
            info["scan_off"] = pos + seg
            break
        pos += seg
    comps = info["comps"]
    if len(comps) == 1:
        comps[0]["h"] = comps[0]["v"] = 1             # a one-component scan is not interleaved
    else:
        assert len(comps) == 3 and all(c["h"] == 1 and c["v"] == 1 for c in comps[1:])
        assert (comps[0]["h"], comps[0]["v"]) in ((1, 1), (2, 1), (2, 2))
    hs, vs = comps[0]["h"], comps[0]["v"]
    info["h_samp"], info["v_samp"], info["components"] = hs, vs, len(comps)
    info["mcus_x"] = -(-info["width"] // (8 * hs))
    info["mcus_y"] = -(-info["height"] // (8 * vs))
    for c in comps:
        c["bw"], c["bh"] = info["mcus_x"] * c["h"], info["mcus_y"] * c["v"]
    info["coef_count"] = 64 * sum(c["bw"] * c["bh"] for c in comps)
    info["qt"], info["huff"] = qt, huff
    return info


def _segments(d, pos):
    """The entropy-coded data split at the restart markers, byte stuffing removed."""
    segs, cur = [], bytearray()
    while True:
        b = d[pos]
        if b != 0xFF:
            cur.append(b)
            pos += 1
        elif d[pos + 1] == 0:
            cur.append(0xFF)
            pos += 2
        elif d[pos + 1] == 0xFF:
            pos += 1
        elif 0xD0 <= d[pos + 1] <= 0xD7:
            assert d[pos + 1] == 0xD0 + (len(segs) & 7)
            segs.append(bytes(cur))
            cur = bytearray()
            pos += 2
        else:
            assert d[pos + 1] == 0xD9, "EOI expected after the scan"
            segs.append(bytes(cur))
            return segs


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def entropy_decode(data):
    """-> (coefs int16 [coef_count]: per component the blocks of its MCU-padded plane in raster block order, 64 per block in natural
    order; quant uint16 [3, 64] in natural order; info)."""
    d = bytes(data)
    info = parse(d)
    comps = info["comps"]
    planes = [np.zeros((c["bh"], c["bw"], 64), np.int64) for c in comps]
    segs = _segments(d, info["scan_off"])
    mcus = info["mcus_x"] * info["mcus_y"]
    ri = info["restart_interval"] or mcus
    assert len(segs) == -(-mcus // ri)
    m = 0
    for seg in segs:
        bits = np.concatenate([np.unpackbits(np.frombuffer(seg, np.uint8)), np.zeros(32, np.uint8)]).astype(np.int64)
        n = len(bits) - 16
        win = np.zeros(n, np.int64)
        for k in range(16):
            win |= bits[k:k + n] << (15 - k)
        win = win.tolist()
        avail = 8 * len(seg)
        pos = 0
        pred = [0] * len(comps)
        for _ in range(min(ri, mcus - m)):
            my, mx = divmod(m, info["mcus_x"])
            for ci, c in enumerate(comps):
                dl, ds = info["huff"][(0, c["td"])]
                al, asym = info["huff"][(1, c["ta"])]
                for by in range(c["v"]):
                    for bx in range(c["h"]):
                        blk = planes[ci][my * c["v"] + by, mx * c["h"] + bx]
                        w = win[pos]
                        l, s = int(dl[w]), int(ds[w])
                        assert l > 0
                        pos += l
                        diff = _extend(win[pos] >> (16 - s), s) if s else 0
                        pos += s
                        pred[ci] += diff
                        blk[0] = pred[ci]
                        k = 1
                        while k < 64:
                            w = win[pos]
                            l, rs = int(al[w]), int(asym[w])
                            assert l > 0
                            pos += l
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            assert k <= 63
                            blk[ZIGZAG_TO_NATURAL[k]] = _extend(win[pos] >> (16 - s), s)
                            pos += s
                            k += 1
                        assert pos <= avail, "the scan ends early"
            m += 1
    coefs = np.concatenate([p.reshape(-1) for p in planes])
    assert coefs.min() >= -32768 and coefs.max() <= 32767
    quant = np.zeros((3, 64), np.uint16)
    for ci, c in enumerate(comps):
        quant[ci] = info["qt"][c["tq"]]
    return coefs.astype(np.int16), quant, info


def _idct_1d(x):
    x0, x1, x2, x3, x4, x5, x6, x7 = x
    z1 = (x2 + x6) * 4433
    t2 = z1 - x6 * 15137
    t3 = z1 + x2 * 6270
    t0 = (x0 + x4) << 13
    t1 = (x0 - x4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a, b, c, d = x7, x5, x3, x1
    z1, z2, z3, z4 = a + d, b + c, a + c, b + d
    z5 = (z3 + z4) * 9633
    a, b, c, d = a * 2446, b * 16819, c * 25172, d * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3 = z3 * -16069 + z5
    z4 = z4 * -3196 + z5
    a, b, c, d = a + z1 + z3, b + z2 + z4, c + z2 + z3, d + z1 + z4
    return [t10 + d, t11 + c, t12 + b, t13 + a, t13 - a, t12 - b, t11 - c, t10 - d]


def _descale(x, s):
    return (x + (1 << (s - 1))) >> s


def idct_planes(coefs, quant, info):
    """Dequantise + inverse DCT: the components' MCU-padded uint8 planes."""
    planes, off = [], 0
    for ci, c in enumerate(info["comps"]):
        nb = c["bw"] * c["bh"]
        v = coefs[off:off + 64 * nb].astype(np.int64).reshape(nb, 8, 8) * quant[ci].astype(np.int64).reshape(1, 8, 8)
        off += 64 * nb
        ws = np.stack([_descale(o, 11) for o in _idct_1d([v[:, r, :] for r in range(8)])], axis=1)      # pass 1: columns
        out = np.stack([_descale(o, 18) for o in _idct_1d([ws[:, :, j] for j in range(8)])], axis=2)    # pass 2: rows
        px = np.clip(out + 128, 0, 255).astype(np.uint8).reshape(c["bh"], c["bw"], 8, 8)
        planes.append(px.transpose(0, 2, 1, 3).reshape(c["bh"] * 8, c["bw"] * 8))
    return planes


def _upsample(pl, W, H, hs, vs):
    """One chroma plane at full size (libjpeg's fancy upsampling; replication when the chroma plane is <= 2 wide)."""
    cw, ch = -(-W // hs), -(-H // vs)
    src = pl[:ch, :cw].astype(np.int64)
    if hs == 1:
        return src[:H, :W]
    if cw <= 2:
        return np.repeat(np.repeat(src, vs, axis=0), 2, axis=1)[:H, :W]
    if vs == 1:
        rows, r_e, r_o, shift = src, 1, 2, 2
        scale = 1
    else:
        idx = np.arange(ch)
        up = 3 * src + src[np.clip(idx - 1, 0, ch - 1)]          # output rows 2r
        dn = 3 * src + src[np.clip(idx + 1, 0, ch - 1)]          # output rows 2r + 1
        rows = np.stack([up, dn], axis=1).reshape(2 * ch, cw)
        r_e, r_o, shift, scale = 8, 7, 4, 4
    out = np.zeros((rows.shape[0], 2 * cw), np.int64)
    left = np.concatenate([rows[:, :1], rows[:, :-1]], axis=1)
    right = np.concatenate([rows[:, 1:], rows[:, -1:]], axis=1)
    out[:, 0::2] = (3 * rows + left + r_e) >> shift
    out[:, 1::2] = (3 * rows + right + r_o) >> shift
    if vs == 1:
        out[:, 0] = rows[:, 0]
        out[:, -1] = rows[:, -1]
    else:
        out[:, 0] = (scale * rows[:, 0] + 8) >> 4
        out[:, -1] = (scale * rows[:, -1] + 7) >> 4
    return out[:H, :W]


def _fix(x):
    return int(x * 65536 + 0.5)


def planes_to_rgb(planes, info):
    W, H = info["width"], info["height"]
    y = planes[0][:H, :W].astype(np.int64)
    if info["components"] == 1:
        return np.stack([y, y, y], axis=2).astype(np.uint8)
    cb = _upsample(planes[1], W, H, info["h_samp"], info["v_samp"]) - 128
    cr = _upsample(planes[2], W, H, info["h_samp"], info["v_samp"]) - 128
    r = y + ((_fix(1.402) * cr + 32768) >> 16)
    b = y + ((_fix(1.772) * cb + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def decode_rgb(data):
    coefs, quant, info = entropy_decode(data)
    return planes_to_rgb(idct_planes(coefs, quant, info), info)

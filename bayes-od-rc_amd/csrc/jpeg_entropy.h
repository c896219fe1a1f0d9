// Host half of the JPEG decoder: marker parsing and Huffman decoding of baseline streams, plain C++ (no HIP), shared
// by engine.hip and by the sanitizer build of tests/host/jpeg_entropy_check.cpp (g++ -fsanitize=address,undefined;
// tests/test_host_jpeg_sanitizers.py), which feeds it truncated and byte-substituted files.
//   jpeg_parse    SOI .. SOS: frame geometry, quantisation and Huffman tables, where the entropy-coded segment starts.  A well-formed
//                 stream outside the supported subset is reported through `supported = 0` + a reason, not as an error.
//   jpeg_decode   the one interleaved scan -> per component the coefficient blocks of the MCU-padded plane in raster block order,
//                 64 int16 per block in natural (row-major) order: what jpeg_idct_kernel reads, 16 contiguous bytes per block row
// Every read of the input is bounds-checked and every table index validated: a hostile stream gives JPEG_INVALID with a message.
// Offsets and counts are 64-bit.  (ITU-T T.81: B.2 markers, F.2.2 Huffman decoding, K.1/K.3 zig-zag order.)
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

enum { JPEG_OK = 0, JPEG_INVALID = 1 };           // (BOD_OK / BOD_ERR_INVALID_ARG of include/bayesod.h)

constexpr int JPEG_FAST_BITS = 9;                 // lookup-table width of the Huffman decoder

struct JpegHuff {
    uint16_t fast[1 << JPEG_FAST_BITS];           // (length << 8) | symbol for codes of <= JPEG_FAST_BITS bits, 0: longer or no code
    int32_t maxcode[18];                          // largest code of each length, -1: none
    int32_t valptr[17], mincode[17];
    uint8_t vals[256];
    int32_t nvals;
    int32_t present;
};

struct JpegHeader {
    int32_t width, height, components;
    int32_t h_samp, v_samp;                       // luma sampling; chroma is 1x1
    int32_t restart_interval;
    int32_t supported;
    int32_t mcus_x, mcus_y;
    int32_t bw[3], bh[3];                         // blocks per row / column of each component's MCU-padded plane
    int32_t tq[3], td[3], ta[3];                  // quantisation, DC and AC table selectors per component (all validated)
    int64_t coef_off[3];                          // first int16 of each component in the coefficient output
    int64_t coef_count;
    int64_t scan_off;                             // first byte of the entropy-coded segment
    uint16_t quant[4][64];                        // natural order
    int32_t quant_present[4];
    JpegHuff dc[4], ac[4];
    char msg[192];
};

static const uint8_t kJpegNatural[64] = {         // zig-zag index -> natural index
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

inline int jpeg_fail(char* msg, size_t cap, const char* text) {
    snprintf(msg, cap, "%s", text);
    return JPEG_INVALID;
}

// One DHT table: the canonical code of T.81 C.2 + the lookup table.  0 on success.
inline int jpeg_build_huff(const uint8_t* counts, const uint8_t* vals, int nvals, JpegHuff* t) {
    memset(t, 0, sizeof *t);
    int32_t code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        t->valptr[l] = k; t->mincode[l] = code;
        const int n = counts[l - 1];
        if (code + n > (1 << l)) return 1;                    // more codes of this length than the prefix tree has room for
        for (int i = 0; i < n; ++i, ++k, ++code)
            if (l <= JPEG_FAST_BITS) {
                const int first = code << (JPEG_FAST_BITS - l), span = 1 << (JPEG_FAST_BITS - l);
                for (int j = 0; j < span; ++j) t->fast[first + j] = (uint16_t)((l << 8) | vals[k]);
            }
        t->maxcode[l] = n ? code - 1 : -1;
        code <<= 1;
    }
    t->maxcode[17] = -1;
    if (k != nvals) return 1;
    memcpy(t->vals, vals, (size_t)nvals);
    t->nvals = nvals;
    t->present = 1;
    return 0;
}

inline int jpeg_parse(const uint8_t* d, int64_t len, JpegHeader* h) {
    memset(h, 0, sizeof *h);
    auto bad = [&](const char* m) { return jpeg_fail(h->msg, sizeof h->msg, m); };
    auto unsupported = [&](const char* m) { snprintf(h->msg, sizeof h->msg, "%s", m); h->supported = 0; return JPEG_OK; };
    if (!d || len < 0) return bad("no data");
    if (len < 2 || d[0] != 0xFF || d[1] != 0xD8) return unsupported("not a JPEG file (no SOI marker)");
    int64_t pos = 2;
    bool have_sof = false, jfif = false, adobe = false;
    int adobe_transform = -1;
    int comp_id[3] = {0, 0, 0}, comp_h[3] = {0, 0, 0}, comp_v[3] = {0, 0, 0};
    for (;;) {
        if (pos + 2 > len) return bad("the stream ends before the scan");
        if (d[pos] != 0xFF) return bad("marker expected");
        const int m = d[pos + 1];
        if (m == 0xFF) { ++pos; continue; }                   // fill byte
        pos += 2;
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) return bad("unexpected marker in the header");
        if (m == 0xD9) return bad("EOI before the scan");
        if (pos + 2 > len) return bad("the stream ends inside a marker segment");
        const int64_t seg = ((int64_t)d[pos] << 8) | d[pos + 1];
        if (seg < 2 || pos + seg > len) return bad("marker segment runs past the end of the stream");
        const uint8_t* p = d + pos + 2;
        const int64_t n = seg - 2;
        if (m == 0xC0 || m == 0xC1 || m == 0xC2 || m == 0xC3 || (m >= 0xC5 && m <= 0xCF && m != 0xC8 && m != 0xCC)) {
            if (have_sof) return bad("second frame header");
            if (n < 6) return bad("short frame header");
            h->height = (p[1] << 8) | p[2]; h->width = (p[3] << 8) | p[4]; h->components = p[5];
            if (m != 0xC0) {
                char why[96];
                snprintf(why, sizeof why, "SOF%d stream (%s); only baseline SOF0 is decoded", m - 0xC0,
                         m == 0xC2 ? "progressive" : m == 0xC1 ? "extended sequential" : m >= 0xC9 ? "arithmetic coding" : "lossless or hierarchical");
                return unsupported(why);
            }
            if (p[0] != 8) return unsupported("sample precision is not 8 bits");
            if (h->components == 4) return unsupported("4 components (CMYK / YCCK)");
            if (h->components != 1 && h->components != 3) return unsupported("component count is neither 1 nor 3");
            if (n != 6 + 3 * (int64_t)h->components) return bad("frame header length does not match its component count");
            if (h->height == 0 || h->width == 0) return bad("width or height 0");
            for (int c = 0; c < h->components; ++c) {
                comp_id[c] = p[6 + 3 * c]; comp_h[c] = p[7 + 3 * c] >> 4; comp_v[c] = p[7 + 3 * c] & 15;
                h->tq[c] = p[8 + 3 * c];
                if (comp_h[c] < 1 || comp_h[c] > 4 || comp_v[c] < 1 || comp_v[c] > 4) return bad("sampling factor outside 1..4");
                if (h->tq[c] > 3) return bad("quantisation table selector outside 0..3");
                for (int e = 0; e < c; ++e) if (comp_id[e] == comp_id[c]) return bad("duplicate component id");
            }
            have_sof = true;
        } else if (m == 0xDB) {
            int64_t q = 0;
            while (q < n) {
                const int pq = p[q] >> 4, tq = p[q] & 15;
                if (tq > 3) return bad("quantisation table id outside 0..3");
                if (pq == 1) return unsupported("16-bit quantisation table");
                if (pq != 0) return bad("quantisation table precision");
                if (q + 65 > n) return bad("short quantisation table");
                for (int k = 0; k < 64; ++k) h->quant[tq][kJpegNatural[k]] = p[q + 1 + k];
                h->quant_present[tq] = 1;
                q += 65;
            }
        } else if (m == 0xC4) {
            int64_t q = 0;
            while (q < n) {
                if (q + 17 > n) return bad("short Huffman table");
                const int tc = p[q] >> 4, th = p[q] & 15;
                if (tc > 1 || th > 3) return bad("Huffman table class or id out of range");
                int total = 0;
                for (int l = 0; l < 16; ++l) total += p[q + 1 + l];
                if (total > 256 || q + 17 + total > n) return bad("Huffman table longer than its segment");
                if (jpeg_build_huff(p + q + 1, p + q + 17, total, tc ? &h->ac[th] : &h->dc[th])) return bad("Huffman table is not a prefix code");
                q += 17 + total;
            }
        } else if (m == 0xDD) {
            if (n != 2) return bad("restart interval segment length");
            h->restart_interval = (p[0] << 8) | p[1];
        } else if (m == 0xDC) {
            return unsupported("DNL marker");
        } else if (m == 0xCC) {
            return unsupported("arithmetic conditioning (DAC)");
        } else if (m == 0xE0) {
            if (n >= 5 && !memcmp(p, "JFIF", 5)) jfif = true;
        } else if (m == 0xEE) {
            if (n >= 12 && !memcmp(p, "Adobe", 5)) { adobe = true; adobe_transform = p[11]; }
        } else if (m == 0xDA) {
            if (!have_sof) return bad("scan before the frame header");
            if (n < 1) return bad("short scan header");
            const int ns = p[0];
            if (ns < 1 || ns > 4 || n != 4 + 2 * (int64_t)ns) return bad("scan header length does not match its component count");
            if (ns != h->components) return unsupported("more than one scan (the components are not interleaved)");
            for (int c = 0; c < ns; ++c) {
                if (p[1 + 2 * c] != comp_id[c]) return unsupported("scan lists the components in another order than the frame");
                h->td[c] = p[2 + 2 * c] >> 4; h->ta[c] = p[2 + 2 * c] & 15;
                if (h->td[c] > 3 || h->ta[c] > 3) return bad("Huffman table selector outside 0..3");
                if (!h->dc[h->td[c]].present || !h->ac[h->ta[c]].present) return bad("scan selects a Huffman table that was not defined");
                if (!h->quant_present[h->tq[c]]) return bad("component selects a quantisation table that was not defined");
            }
            if (p[1 + 2 * ns] != 0 || p[2 + 2 * ns] != 63 || p[3 + 2 * ns] != 0) return bad("spectral selection of a baseline scan must be 0..63");
            h->scan_off = pos + seg;
            break;
        }
        // (APPn, COM and anything else with a length: skipped)
        pos += seg;
    }
    if (h->components == 3) {
        if (comp_h[1] != 1 || comp_v[1] != 1 || comp_h[2] != 1 || comp_v[2] != 1) return unsupported("chroma sampling is not 1x1");
        const int hs = comp_h[0], vs = comp_v[0];
        if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2)))
            return unsupported("luma sampling is none of 1x1 (4:4:4), 2x1 (4:2:2), 2x2 (4:2:0)");
        h->h_samp = hs; h->v_samp = vs;
        if (adobe && adobe_transform == 0) return unsupported("Adobe APP14 transform 0: the components are RGB, not YCbCr");
        if (!adobe && !jfif && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B')
            return unsupported("component ids R, G, B: the components are RGB, not YCbCr");
    } else {
        h->h_samp = 1; h->v_samp = 1;                         // a one-component scan is not interleaved: its MCU is one block
    }
    h->mcus_x = (h->width + 8 * h->h_samp - 1) / (8 * h->h_samp);
    h->mcus_y = (h->height + 8 * h->v_samp - 1) / (8 * h->v_samp);
    int64_t off = 0;
    for (int c = 0; c < h->components; ++c) {
        h->bw[c] = h->mcus_x * (c == 0 ? h->h_samp : 1);
        h->bh[c] = h->mcus_y * (c == 0 ? h->v_samp : 1);
        h->coef_off[c] = off;
        off += (int64_t)h->bw[c] * h->bh[c] * 64;
    }
    h->coef_count = off;
    // a coded block takes at least two bits (a DC and an EOB symbol): a header that promises more blocks than the scan has room for
    // is refused here, before anybody sizes a buffer by it
    if (off / 64 > 4 * (len - h->scan_off)) return bad("the scan is too short for the frame size");
    h->supported = 1;
    return JPEG_OK;
}

struct JpegBits {
    const uint8_t* d; int64_t pos, end;
    uint64_t acc; int cnt;                 // the low `cnt` bits of acc are unread
    bool stop;                             // a marker or the end of the data is next: no more bits

    void fill() {
        while (cnt <= 56 && !stop) {
            if (pos >= end) { stop = true; break; }
            const uint8_t b = d[pos];
            if (b == 0xFF) {
                if (pos + 1 >= end) { stop = true; break; }
                const uint8_t b2 = d[pos + 1];
                if (b2 != 0) { stop = true; break; }          // a marker (or fill bytes in front of one)
                pos += 2;
            } else {
                ++pos;
            }
            acc = (acc << 8) | b; cnt += 8;
        }
    }
    // the next n bits (1..16), zero-padded past the end of the data: the caller checks cnt before it consumes them
    uint32_t peek(int n) {
        if (cnt < n) fill();
        const uint64_t v = cnt >= n ? acc >> (cnt - n) : acc << (n - cnt);
        return (uint32_t)(v & ((1u << n) - 1));
    }
};

// One Huffman symbol; -1: no such code, or the data ends inside it.
inline int jpeg_symbol(JpegBits& b, const JpegHuff& t) {
    const uint32_t e = t.fast[b.peek(JPEG_FAST_BITS)];
    if (e) {
        const int l = (int)(e >> 8);
        if (l > b.cnt) return -1;
        b.cnt -= l;
        return (int)(e & 255);
    }
    const int32_t code16 = (int32_t)b.peek(16);
    for (int l = JPEG_FAST_BITS + 1; l <= 16; ++l) {
        const int32_t c = code16 >> (16 - l);
        if (t.maxcode[l] >= 0 && c <= t.maxcode[l] && c >= t.mincode[l]) {
            const int32_t i = t.valptr[l] + c - t.mincode[l];
            if (i < 0 || i >= t.nvals || l > b.cnt) return -1;
            b.cnt -= l;
            return t.vals[i];
        }
    }
    return -1;
}

// s further bits as the signed value of T.81 F.2.2.1 (EXTEND); false: the data ends first.
inline bool jpeg_receive_extend(JpegBits& b, int s, int32_t* v) {
    if (s == 0) { *v = 0; return true; }
    const int32_t r = (int32_t)b.peek(s);
    if (s > b.cnt) return false;
    b.cnt -= s;
    *v = r < (1 << (s - 1)) ? r - (1 << s) + 1 : r;
    return true;
}

// The scan of a parsed, supported stream.  coefs: h.coef_count int16, written whole (zeros included); quant3x64: the tables of
// components 0..2 in natural order (those of absent components zero).  msg receives the reason on failure.
inline int jpeg_decode(const uint8_t* d, int64_t len, const JpegHeader& h, int16_t* coefs, uint16_t* quant3x64, char* msg, size_t msg_cap) {
    auto bad = [&](const char* m) { return jpeg_fail(msg, msg_cap, m); };
    if (!h.supported) return bad("unsupported stream");
    if (h.scan_off < 0 || h.scan_off > len) return bad("scan offset outside the stream");
    memset(coefs, 0, (size_t)h.coef_count * sizeof(int16_t));
    if (quant3x64) {
        memset(quant3x64, 0, 3 * 64 * sizeof(uint16_t));
        for (int c = 0; c < h.components; ++c) memcpy(quant3x64 + 64 * c, h.quant[h.tq[c]], 64 * sizeof(uint16_t));
    }
    JpegBits b{d, h.scan_off, len, 0, 0, false};
    int32_t pred[3] = {0, 0, 0};
    const int64_t mcus = (int64_t)h.mcus_x * h.mcus_y;
    int64_t until_restart = h.restart_interval ? h.restart_interval : -1;
    int next_rst = 0;
    for (int64_t m = 0; m < mcus; ++m) {
        if (until_restart == 0) {
            // the bits left of the interval's last byte are padding; the marker is next, possibly behind fill bytes
            b.acc = 0; b.cnt = 0; b.stop = false;
            while (b.pos + 1 < b.end && b.d[b.pos] == 0xFF && b.d[b.pos + 1] == 0xFF) ++b.pos;
            if (b.pos + 2 > b.end || b.d[b.pos] != 0xFF || b.d[b.pos + 1] != 0xD0 + next_rst) return bad("missing restart marker");
            b.pos += 2;
            next_rst = (next_rst + 1) & 7;
            pred[0] = pred[1] = pred[2] = 0;
            until_restart = h.restart_interval;
        }
        const int64_t my = m / h.mcus_x, mx = m % h.mcus_x;
        for (int c = 0; c < h.components; ++c) {
            const int ch = c == 0 ? h.h_samp : 1, cv = c == 0 ? h.v_samp : 1;
            const JpegHuff& dc = h.dc[h.td[c]];
            const JpegHuff& ac = h.ac[h.ta[c]];
            for (int by = 0; by < cv; ++by)
                for (int bx = 0; bx < ch; ++bx) {
                    const int64_t brow = my * cv + by, bcol = mx * ch + bx;
                    int16_t* blk = coefs + h.coef_off[c] + (brow * h.bw[c] + bcol) * 64;
                    const int s = jpeg_symbol(b, dc);
                    if (s < 0) return bad("bad Huffman code or the stream ends inside the scan (DC)");
                    if (s > 15) return bad("DC size category above 15");
                    int32_t diff;
                    if (!jpeg_receive_extend(b, s, &diff)) return bad("the stream ends inside the scan (DC bits)");
                    pred[c] = (int16_t)(uint16_t)(uint32_t)(pred[c] + diff);          // kept in int16 range: hostile sums wrap, defined
                    blk[0] = (int16_t)pred[c];
                    for (int k = 1; k < 64;) {
                        const int rs = jpeg_symbol(b, ac);
                        if (rs < 0) return bad("bad Huffman code or the stream ends inside the scan (AC)");
                        const int r = rs >> 4, sz = rs & 15;
                        if (sz == 0) {
                            if (r != 15) break;                                       // EOB
                            k += 16;
                            if (k > 64) return bad("coefficient index past 63");
                            continue;
                        }
                        k += r;
                        if (k > 63) return bad("coefficient index past 63");
                        int32_t v;
                        if (!jpeg_receive_extend(b, sz, &v)) return bad("the stream ends inside the scan (AC bits)");
                        blk[kJpegNatural[k]] = (int16_t)v;
                        ++k;
                    }
                }
        }
        if (until_restart > 0) --until_restart;
    }
    // what follows the last MCU: padding bits, then EOI.  Another scan or table means a stream this decoder does not cover.
    int64_t p = b.pos;
    while (p + 1 < len && d[p] == 0xFF && d[p + 1] == 0xFF) ++p;
    if (p + 2 > len || d[p] != 0xFF) return bad("the stream ends without EOI");
    if (d[p + 1] == 0xDA || d[p + 1] == 0xC4 || d[p + 1] == 0xDB) return bad("more than one scan");
    if (d[p + 1] == 0xDC) return bad("DNL marker");
    if (d[p + 1] != 0xD9) return bad("EOI expected after the scan");
    return JPEG_OK;
}

// Host half of the PNG decoder: chunk parsing and zlib inflate, plain C++17 (no HIP, no zlib), shared by engine.hip
// and by the sanitizer build of tests/host/png_inflate_check.cpp (g++ -fsanitize=address,undefined;
// tests/test_host_png_sanitizers.py), which feeds it truncated and byte-substituted files.
//   png_parse     signature, IHDR and the chunk walk up to IEND: geometry, which subset the file is in, how many IDAT bytes there
//                 are.  A well-formed file outside the supported subset is reported through `supported = 0` + a reason, not as an
//                 error.  Only IHDR's CRC is checked here (the walk is serial in a batch; the other CRCs belong to png_decode).
//   png_decode    CRC-32 of every critical chunk, the concatenated IDAT stream's zlib header, inflate into a caller buffer of exactly
//                 height * (1 + width * channels) bytes, the Adler-32 trailer, and every row's filter-type byte (0..4): the filtered
//                 scanlines png_unfilter_kernel reads.
// Every read of the input is bounds-checked, every write lands inside the caller buffer, every loop is bounded by input or output
// length: a hostile file gives PNG_INVALID with a message.  Offsets and counts are 64-bit.
// (PNG specification, 2nd edition: 5 datastream, 9 filtering, 10 compression; RFC 1950, RFC 1951.)
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <new>
#include <vector>

static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "the bit reader loads 8 input bytes as one little-endian word");

enum { PNG_OK = 0, PNG_INVALID = 1 };             // (BOD_OK / BOD_ERR_INVALID_ARG of include/bayesod.h)

constexpr int PNG_FAST_BITS = 10;                 // width of the Huffman decoder's lookup table
constexpr int32_t PNG_MAX_DIM = 65535;            // per side: the ceiling the JPEG route's frames have (a 16-bit field there)

struct PngHeader {
    int32_t width, height, bit_depth, color_type, channels, interlace;
    int32_t supported;
    int64_t raw_bytes;                            // height * (1 + width * channels): the filtered scanlines
    int64_t idat_bytes;                           // all IDAT chunks together
    char msg[192];
};

inline int png_fail(char* msg, size_t cap, const char* text) {
    snprintf(msg, cap, "%s", text);
    return PNG_INVALID;
}

// ---- CRC-32 (PNG annex D's polynomial), eight tables: 8 bytes per step -------------------------------------------------------------
struct PngCrcTables {
    uint32_t t[8][256];
    PngCrcTables() {
        for (uint32_t n = 0; n < 256; ++n) {
            uint32_t c = n;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            t[0][n] = c;
        }
        for (uint32_t n = 0; n < 256; ++n)
            for (int k = 1; k < 8; ++k) t[k][n] = t[0][t[k - 1][n] & 255] ^ (t[k - 1][n] >> 8);
    }
};

inline const PngCrcTables& png_crc_tables() {
    static const PngCrcTables tables;             // (thread-safe initialisation: C++11 6.7)
    return tables;
}

inline uint32_t png_crc32(uint32_t crc, const uint8_t* p, int64_t n) {
    const PngCrcTables& T = png_crc_tables();
    crc = ~crc;
    for (; n >= 8; n -= 8, p += 8) {
        uint32_t lo, hi;
        memcpy(&lo, p, 4); memcpy(&hi, p + 4, 4);
        lo ^= crc;
        crc = T.t[7][lo & 255] ^ T.t[6][(lo >> 8) & 255] ^ T.t[5][(lo >> 16) & 255] ^ T.t[4][lo >> 24] ^
              T.t[3][hi & 255] ^ T.t[2][(hi >> 8) & 255] ^ T.t[1][(hi >> 16) & 255] ^ T.t[0][hi >> 24];
    }
    for (; n > 0; --n, ++p) crc = T.t[0][(crc ^ *p) & 255] ^ (crc >> 8);
    return ~crc;
}

inline uint32_t png_adler32(const uint8_t* p, int64_t n) {
    uint32_t a = 1, b = 0;
    while (n > 0) {
        int64_t k = n < 5552 ? n : 5552;          // the largest run for which b cannot overflow 32 bits
        n -= k;
        for (; k >= 8; k -= 8, p += 8) {
            a += p[0]; b += a; a += p[1]; b += a; a += p[2]; b += a; a += p[3]; b += a;
            a += p[4]; b += a; a += p[5]; b += a; a += p[6]; b += a; a += p[7]; b += a;
        }
        for (; k > 0; --k, ++p) { a += *p; b += a; }
        a %= 65521u; b %= 65521u;
    }
    return (b << 16) | a;
}

inline uint32_t png_be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

constexpr uint32_t png_tag(char a, char b, char c, char d) {
    return ((uint32_t)(uint8_t)a << 24) | ((uint32_t)(uint8_t)b << 16) | ((uint32_t)(uint8_t)c << 8) | (uint32_t)(uint8_t)d;
}

// One step of the chunk walk: the chunk at `pos` -> its type, its data's position and length.  0 when the chunk (with its CRC field)
// lies inside the file.
inline int png_chunk_at(const uint8_t* d, int64_t len, int64_t pos, uint32_t* type, int64_t* data, int64_t* n) {
    if (len - pos < 12) return 1;
    const int64_t cl = png_be32(d + pos);
    if (cl > 0x7FFFFFFF || cl > len - pos - 12) return 1;
    *type = png_be32(d + pos + 4); *data = pos + 8; *n = cl;
    return 0;
}

inline int png_parse(const uint8_t* d, int64_t len, PngHeader* h) {
    memset(h, 0, sizeof *h);
    auto bad = [&](const char* text) { return png_fail(h->msg, sizeof h->msg, text); };
    auto unsupported = [&](const char* text) { if (h->supported) { h->supported = 0; snprintf(h->msg, sizeof h->msg, "%s", text); } };
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    if (len < 8 || memcmp(d, sig, 8) != 0) {      // not this format at all (a JPEG): unsupported, as bod_jpeg_info reports a PNG
        snprintf(h->msg, sizeof h->msg, "not a PNG (no signature)");
        return PNG_OK;
    }
    uint32_t type = 0; int64_t at = 0, n = 0, pos = 8;
    if (png_chunk_at(d, len, pos, &type, &at, &n)) return bad("truncated before the end of IHDR");
    if (type != png_tag('I', 'H', 'D', 'R') || n != 13) return bad("the first chunk is not a 13-byte IHDR");
    if (png_crc32(0, d + at - 4, n + 4) != png_be32(d + at + n)) return bad("CRC mismatch in IHDR");
    const uint32_t w = png_be32(d + at), hh = png_be32(d + at + 4);
    h->bit_depth = d[at + 8]; h->color_type = d[at + 9]; h->interlace = d[at + 12];
    if (w == 0 || hh == 0) return bad("width or height 0");
    if (w > 0x7FFFFFFFu || hh > 0x7FFFFFFFu) return bad("width or height beyond 2^31 - 1");
    const int bd = h->bit_depth, ct = h->color_type;
    const bool combo = (ct == 0 && (bd == 1 || bd == 2 || bd == 4 || bd == 8 || bd == 16)) || (ct == 3 && (bd == 1 || bd == 2 || bd == 4 || bd == 8)) ||
                       ((ct == 2 || ct == 4 || ct == 6) && (bd == 8 || bd == 16));
    if (!combo) return bad("colour type and bit depth do not go together");
    if (d[at + 10] != 0 || d[at + 11] != 0) return bad("unknown compression or filter method");
    if (h->interlace > 1) return bad("unknown interlace method");
    if (w > (uint32_t)PNG_MAX_DIM || hh > (uint32_t)PNG_MAX_DIM) return bad("width or height beyond 65535: more than the frame staging takes");
    h->width = (int32_t)w; h->height = (int32_t)hh;
    h->channels = ct == 0 ? 1 : ct == 2 ? 3 : ct == 3 ? 1 : ct == 4 ? 2 : 4;
    h->supported = 1;
    if (ct == 3) unsupported("palette image (colour type 3)");
    else if (bd != 8) { char t[64]; snprintf(t, sizeof t, "bit depth %d (only 8 is decoded)", bd); unsupported(t); }
    if (h->interlace == 1) unsupported("Adam7 interlaced");
    h->raw_bytes = (int64_t)h->height * (1 + (int64_t)h->width * h->channels);
    pos = at + n + 4;
    bool seen_idat = false, idat_closed = false, seen_plte = false;
    for (;;) {
        if (png_chunk_at(d, len, pos, &type, &at, &n)) return bad("truncated: a chunk runs past the end of the file (no IEND)");
        if (type == png_tag('I', 'E', 'N', 'D')) break;
        if (type == png_tag('I', 'D', 'A', 'T')) {
            if (idat_closed) return bad("IDAT chunks are not consecutive");
            seen_idat = true;
            h->idat_bytes += n;
        } else {
            if (seen_idat) idat_closed = true;
            if (type == png_tag('I', 'H', 'D', 'R')) return bad("a second IHDR");
            else if (type == png_tag('P', 'L', 'T', 'E')) {
                if (seen_plte || seen_idat || n % 3 != 0 || n == 0 || n > 768) return bad("misplaced or malformed PLTE");
                seen_plte = true;
            } else if (type == png_tag('t', 'R', 'N', 'S')) unsupported("tRNS chunk (transparency is not applied)");
            else if (type == png_tag('a', 'c', 'T', 'L')) unsupported("acTL chunk (animated PNG)");
            else if (!(type & 0x20000000u)) return bad("unknown critical chunk");        // (bit 5 of the first letter clear)
        }
        pos = at + n + 4;
    }
    if (n != 0) return bad("IEND with data");
    if (!seen_idat) return bad("no IDAT chunk");
    if (ct == 3 && !seen_plte) return bad("palette image without PLTE");
    return PNG_OK;
}

// ---- inflate (RFC 1951) -----------------------------------------------------------------------------------------------------------
// LSB-first bit reader.  `cnt` is the number of valid low bits of `buf`; bits above them are either 0 or copies of the stream's
// next bits (the 8-byte refill ORs bytes it does not consume yet), so a later refill ORs the same values again.
struct PngBits {
    const uint8_t* p; const uint8_t* end;
    uint64_t buf; int cnt;
    void refill() {
        if (end - p >= 8) {
            uint64_t v;
            memcpy(&v, p, 8);
            buf |= v << cnt;
            p += (63 - cnt) >> 3;
            cnt |= 56;
        } else {
            while (cnt <= 56 && p < end) { buf |= (uint64_t)*p++ << cnt; cnt += 8; }
        }
    }
    void drop(int n) { buf >>= n; cnt -= n; }
};

// A canonical prefix code over up to 288 symbols.  fast[]: for every PNG_FAST_BITS-bit window that starts with a code of at most that
// length, (symbol << 4) | length; 0 otherwise (a longer code or none: the canonical walk of count[] / sym[] decides).
struct PngHuff {
    uint16_t fast[1 << PNG_FAST_BITS];
    uint16_t count[16];
    uint16_t sym[288];
};

// lens[n] -> the decoder.  0: a complete code.  1: over-subscribed.  2: incomplete (2 with *single = 1: one code of length 1,
// 2 with *empty = 1: no code at all), which the caller may accept.
inline int png_build_huff(const uint8_t* lens, int n, PngHuff* t, int* single, int* empty) {
    memset(t, 0, sizeof *t);
    for (int i = 0; i < n; ++i) ++t->count[lens[i]];
    *empty = t->count[0] == n;
    t->count[0] = 0;
    int left = 1, total = 0;
    for (int l = 1; l <= 15; ++l) {
        left = (left << 1) - t->count[l];
        if (left < 0) return 1;
        total += t->count[l];
    }
    *single = total == 1 && t->count[1] == 1;
    uint16_t offs[16], next[16];
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + t->count[l]);
    for (int i = 0; i < n; ++i) if (lens[i]) t->sym[offs[lens[i]]++] = (uint16_t)i;
    uint32_t code = 0;
    for (int l = 1; l <= 15; ++l) { code = (code + t->count[l - 1]) << 1; next[l] = (uint16_t)code; }     // (RFC 1951 3.2.2; count[0] is 0)
    for (int i = 0; i < n; ++i) {
        const int l = lens[i];
        if (l == 0 || l > PNG_FAST_BITS) continue;
        uint32_t c = next[l]++, r = 0;
        for (int k = 0; k < l; ++k) r |= ((c >> k) & 1u) << (l - 1 - k);        // the stream carries a code's first bit lowest
        for (uint32_t j = r; j < (1u << PNG_FAST_BITS); j += 1u << l) t->fast[j] = (uint16_t)((i << 4) | l);
    }
    return left > 0 ? 2 : 0;
}

// One symbol; -1: the input ended inside the code, or the bits are no code of an incomplete set.  At least 15 bits are in the buffer
// unless the input is at its end (refill() before).
inline int png_decode_sym(PngBits& b, const PngHuff& t) {
    const uint16_t e = t.fast[b.buf & ((1u << PNG_FAST_BITS) - 1)];
    if (e) {
        const int l = e & 15;
        if (l > b.cnt) return -1;
        b.drop(l);
        return e >> 4;
    }
    int code = 0, first = 0, index = 0;
    const int avail = b.cnt < 15 ? b.cnt : 15;
    for (int l = 1; l <= avail; ++l) {
        code |= (int)((b.buf >> (l - 1)) & 1);
        const int count = t.count[l];
        if (code - count < first) { b.drop(l); return t.sym[index + (code - first)]; }
        index += count; first += count;
        first <<= 1; code <<= 1;
    }
    return -1;
}

// The deflate stream at b -> exactly out_cap bytes at out.  Leaves b behind the final block.
inline int png_inflate_blocks(PngBits& b, uint8_t* out, int64_t out_cap, PngHuff* lit, PngHuff* dist, char* msg, size_t msg_cap) {
    static const uint16_t len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const uint8_t len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    static const uint16_t dist_base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
                                           8193, 12289, 16385, 24577};
    static const uint8_t dist_extra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    auto bad = [&](const char* text) { return png_fail(msg, msg_cap, text); };
    int64_t o = 0;
    for (;;) {                                                        // (every block consumes at least its 3 header bits)
        b.refill();
        if (b.cnt < 3) return bad("truncated: the deflate stream ends before its final block");
        const int final_block = (int)(b.buf & 1), type = (int)((b.buf >> 1) & 3);
        b.drop(3);
        if (type == 3) return bad("deflate block of reserved type 3");
        if (type == 0) {
            // back to the byte boundary: whole bytes still in the buffer are un-read, then LEN / NLEN and the bytes themselves
            b.drop(b.cnt & 7);
            const uint8_t* p = b.p - (b.cnt >> 3);
            b.buf = 0; b.cnt = 0;
            if (b.end - p < 4) return bad("truncated: stored block without its length");
            const uint32_t n = p[0] | ((uint32_t)p[1] << 8), nn = p[2] | ((uint32_t)p[3] << 8);
            if ((n ^ nn) != 0xFFFFu) return bad("stored block whose length check fails");
            p += 4;
            if ((int64_t)n > b.end - p) return bad("truncated: stored block runs past the input");
            if ((int64_t)n > out_cap - o) return bad("the stream holds more bytes than the header's size gives");
            if (n) memcpy(out + o, p, n);
            o += n;
            b.p = p + n;
        } else {
            uint8_t lens[288 + 32];
            int nlit, ndist;
            if (type == 1) {
                nlit = 288; ndist = 32;
                for (int i = 0; i < 144; ++i) lens[i] = 8;
                for (int i = 144; i < 256; ++i) lens[i] = 9;
                for (int i = 256; i < 280; ++i) lens[i] = 7;
                for (int i = 280; i < 288; ++i) lens[i] = 8;
                for (int i = 0; i < 32; ++i) lens[288 + i] = 5;
            } else {
                if (b.cnt < 14) return bad("truncated: dynamic block header");
                nlit = (int)(b.buf & 31) + 257; ndist = (int)((b.buf >> 5) & 31) + 1;
                const int ncode = (int)((b.buf >> 10) & 15) + 4;
                b.drop(14);
                if (nlit > 286 || ndist > 30) return bad("dynamic block with too many length or distance codes");
                uint8_t cl[19] = {0};
                b.refill();                                            // 19 * 3 = 57 bits at most: in two halves
                for (int i = 0; i < ncode; ++i) {
                    if (i == 12) b.refill();
                    if (b.cnt < 3) return bad("truncated: code-length code lengths");
                    cl[order[i]] = (uint8_t)(b.buf & 7);
                    b.drop(3);
                }
                int single = 0, empty = 0;
                if (png_build_huff(cl, 19, lit, &single, &empty) != 0) return bad("invalid code-length code (over-subscribed or incomplete)");
                int i = 0;
                while (i < nlit + ndist) {                             // (every pass sets at least one length)
                    b.refill();
                    const int s = png_decode_sym(b, *lit);
                    if (s < 0) return bad("truncated or invalid code-length symbol");
                    if (s < 16) { lens[i++] = (uint8_t)s; continue; }
                    int rep, val = 0;
                    if (s == 16) {
                        if (i == 0) return bad("code-length repeat with nothing to repeat");
                        if (b.cnt < 2) return bad("truncated: code-length repeat");
                        val = lens[i - 1]; rep = 3 + (int)(b.buf & 3); b.drop(2);
                    } else if (s == 17) {
                        if (b.cnt < 3) return bad("truncated: code-length repeat");
                        rep = 3 + (int)(b.buf & 7); b.drop(3);
                    } else {
                        if (b.cnt < 7) return bad("truncated: code-length repeat");
                        rep = 11 + (int)(b.buf & 127); b.drop(7);
                    }
                    if (rep > nlit + ndist - i) return bad("code-length repeat runs past the code count");
                    memset(lens + i, val, (size_t)rep);
                    i += rep;
                }
                if (lens[256] == 0) return bad("dynamic block without an end-of-block code");
                memmove(lens + 288, lens + nlit, (size_t)ndist);                        // (the two sets at fixed places)
            }
            int single = 0, empty = 0;
            // (an incomplete set is what zlib permits and no more: one code of length 1 -- for literals/lengths that is the end-of-block
            // code alone, a block without data --, and for distances also none at all, where a block is all literals)
            const int lr = png_build_huff(lens, nlit, lit, &single, &empty);
            if (lr == 1 || (lr == 2 && !single)) return bad("invalid literal/length code (over-subscribed or incomplete)");
            const int dr = png_build_huff(lens + 288, ndist, dist, &single, &empty);
            if (dr == 1 || (dr == 2 && !single && !empty)) return bad("invalid distance code (over-subscribed or incomplete)");
            for (;;) {                                                 // (every pass consumes at least one bit or fails)
                b.refill();                                            // 56 bits or the input's last: a length + distance pair takes 48
                int s = png_decode_sym(b, *lit);
                if (s < 0) return bad("truncated or invalid literal/length symbol");
                if (s < 256) {
                    if (o >= out_cap) return bad("the stream holds more bytes than the header's size gives");
                    out[o++] = (uint8_t)s;
                    // a second and third literal from the same refill (15 bits each, the pair below keeps its 48 only after a refill)
                    if (b.cnt >= 30) {
                        const uint16_t e = lit->fast[b.buf & ((1u << PNG_FAST_BITS) - 1)];
                        if (e && (e >> 4) < 256 && o < out_cap) {
                            b.drop(e & 15); out[o++] = (uint8_t)(e >> 4);
                            const uint16_t e2 = lit->fast[b.buf & ((1u << PNG_FAST_BITS) - 1)];
                            if (e2 && (e2 >> 4) < 256 && o < out_cap) { b.drop(e2 & 15); out[o++] = (uint8_t)(e2 >> 4); }
                        }
                    }
                    continue;
                }
                if (s == 256) break;
                s -= 257;
                if (s >= 29) return bad("invalid length symbol");
                int eb = len_extra[s];
                if (b.cnt < eb) return bad("truncated: length extra bits");
                const int64_t mlen = len_base[s] + (int64_t)(b.buf & ((1u << eb) - 1));
                b.drop(eb);
                const int ds = png_decode_sym(b, *dist);
                if (ds < 0) return bad("truncated or invalid distance symbol");
                if (ds >= 30) return bad("invalid distance symbol");
                eb = dist_extra[ds];
                if (b.cnt < eb) return bad("truncated: distance extra bits");
                const int64_t mdist = dist_base[ds] + (int64_t)(b.buf & ((1u << eb) - 1));
                b.drop(eb);
                if (mdist > o) return bad("distance reaches before the first byte written");
                if (mlen > out_cap - o) return bad("the stream holds more bytes than the header's size gives");
                uint8_t* dst = out + o;
                const uint8_t* src = dst - mdist;
                if (mdist >= mlen) memcpy(dst, src, (size_t)mlen);
                else for (int64_t k = 0; k < mlen; ++k) dst[k] = src[k];
                o += mlen;
            }
        }
        if (final_block) break;
    }
    if (o != out_cap) return bad("the stream holds fewer bytes than the header's size gives");
    return PNG_OK;
}

// The file's filtered scanlines -> raw[h.raw_bytes].  h: png_parse's result for the same bytes, supported.
inline int png_decode(const uint8_t* d, int64_t len, const PngHeader& h, uint8_t* raw, char* msg, size_t msg_cap) try {
    auto bad = [&](const char* text) { return png_fail(msg, msg_cap, text); };
    if (!h.supported || len < 8) return bad("not a supported PNG");
    // the walk png_parse made, now with the CRCs; the IDAT data gathered into one stream (in place when there is one chunk)
    std::vector<uint8_t> joined;
    const uint8_t* z = nullptr;
    int64_t zn = 0, idat_chunks = 0, pos = 8;
    for (;;) {
        uint32_t type = 0; int64_t at = 0, n = 0;
        if (png_chunk_at(d, len, pos, &type, &at, &n)) return bad("truncated: a chunk runs past the end of the file (no IEND)");
        const bool idat = type == png_tag('I', 'D', 'A', 'T');
        const bool critical = idat || type == png_tag('I', 'H', 'D', 'R') || type == png_tag('P', 'L', 'T', 'E') || type == png_tag('I', 'E', 'N', 'D');
        if (critical && png_crc32(0, d + at - 4, n + 4) != png_be32(d + at + n)) {
            char t[64];
            snprintf(t, sizeof t, "CRC mismatch in %c%c%c%c", (char)(type >> 24), (char)(type >> 16), (char)(type >> 8), (char)type);
            return bad(t);
        }
        if (idat) {
            if (n > h.idat_bytes - zn) return bad("the file changed between parsing and decoding");
            if (idat_chunks == 0) { z = d + at; }
            else {
                if (idat_chunks == 1) { joined.reserve((size_t)h.idat_bytes); joined.assign(z, z + zn); }
                joined.insert(joined.end(), d + at, d + at + n);
            }
            zn += n; ++idat_chunks;
        }
        if (type == png_tag('I', 'E', 'N', 'D')) break;
        pos = at + n + 4;
    }
    if (idat_chunks > 1) z = joined.data();
    if (zn < 2) return bad("truncated: no zlib header");
    const int cmf = z[0], flg = z[1];
    if ((cmf & 15) != 8) return bad("zlib compression method is not 8 (deflate)");
    if ((cmf >> 4) > 7) return bad("zlib window beyond 32 KiB");
    if (((cmf << 8) | flg) % 31 != 0) return bad("zlib header check fails");
    if (flg & 0x20) return bad("zlib stream with a preset dictionary");
    PngBits b{z + 2, z + zn, 0, 0};
    PngHuff lit, dist;
    const int st = png_inflate_blocks(b, raw, h.raw_bytes, &lit, &dist, msg, msg_cap);
    if (st != PNG_OK) return st;
    b.drop(b.cnt & 7);
    const uint8_t* p = b.p - (b.cnt >> 3);
    if (b.end - p < 4) return bad("truncated: no Adler-32 trailer");
    if (png_be32(p) != png_adler32(raw, h.raw_bytes)) return bad("Adler-32 mismatch");
    const int64_t stride = 1 + (int64_t)h.width * h.channels;
    for (int64_t r = 0; r < h.height; ++r)
        if (raw[r * stride] > 4) return bad("filter type beyond 4");
    return PNG_OK;
} catch (const std::bad_alloc&) {
    return png_fail(msg, msg_cap, "out of host memory for the IDAT stream");
}

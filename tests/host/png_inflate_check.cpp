// Sanitizer build of the PNG decoder's host half (bayes-od-rc_amd/csrc/png_inflate.h, the code bod_upload_frames_png runs on its
// worker threads): g++ -fsanitize=address,undefined (tests/test_host_png_sanitizers.py).
//   usage: png_inflate_check FILE CHECKSUM [FILE CHECKSUM ...]
// Per file: the intact file must decode and the FNV-1a 64 of its filtered scanlines must equal CHECKSUM (hex); then every truncation
// prefix, and every single-byte substitution by 0x00 and 0xFF at every offset, must come back as PNG_OK or PNG_INVALID with the
// sanitizers silent.  A chunk's CRC-32 stops nearly every such input in front of the inflate, so each substitution inside a chunk is
// fed a second time with that chunk's CRC recomputed, and every prefix of the zlib stream once more as a well-formed file around it.
// Every input lives in a heap block of exactly its length and the scanlines in one of exactly raw_bytes, so a read past the input's
// end or a write past the output's is an ASan report.
#include "png_inflate.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

static uint64_t fnv1a(const void* p, size_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

struct Counts { long tried = 0, decoded = 0, refused = 0, unsupported = 0, failures = 0; };

// One input through parser and decoder.  Returns the decoder's status; `sum` receives the scanlines' checksum when it decoded.
static int run(const uint8_t* d, int64_t len, int64_t max_raw, Counts* c, uint64_t* sum) {
    ++c->tried;
    PngHeader h;
    int st = png_parse(d, len, &h);
    if (st == PNG_OK && !h.supported) { ++c->unsupported; return PNG_OK; }
    if (st == PNG_OK && h.raw_bytes > max_raw) { ++c->refused; return PNG_INVALID; }   // (a substituted size byte: the caller's capacity check)
    if (st == PNG_OK) {
        std::unique_ptr<uint8_t[]> raw(new uint8_t[(size_t)h.raw_bytes]);
        char msg[192];
        st = png_decode(d, len, h, raw.get(), msg, sizeof msg);
        if (st == PNG_OK && sum) *sum = fnv1a(raw.get(), (size_t)h.raw_bytes);
    }
    if (st == PNG_OK) ++c->decoded;
    else if (st == PNG_INVALID) ++c->refused;
    else ++c->failures;
    return st;
}

int main(int argc, char** argv) {
    if (argc < 3 || (argc - 1) % 2) { fprintf(stderr, "usage: %s FILE CHECKSUM [FILE CHECKSUM ...]\n", argv[0]); return 2; }
    Counts intact, hostile;
    const int64_t max_raw = 1 << 24;
    for (int a = 1; a + 1 < argc; a += 2) {
        FILE* fp = fopen(argv[a], "rb");
        if (!fp) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        std::vector<uint8_t> file;
        for (int ch; (ch = fgetc(fp)) != EOF;) file.push_back((uint8_t)ch);
        fclose(fp);
        const uint64_t want = strtoull(argv[a + 1], nullptr, 16);
        const int64_t n = (int64_t)file.size();
        {
            std::unique_ptr<uint8_t[]> in(new uint8_t[(size_t)n]);
            memcpy(in.get(), file.data(), (size_t)n);
            uint64_t sum = 0;
            const long before = intact.decoded;
            run(in.get(), n, max_raw, &intact, &sum);
            if (intact.decoded != before + 1 || sum != want) {
                printf("%s: intact file: decoded %ld, checksum %016" PRIx64 ", expected %016" PRIx64 "\n", argv[a], intact.decoded - before, sum, want);
                ++intact.failures;
            }
        }
        for (int64_t cut = 0; cut < n; ++cut) {                  // every truncation prefix
            std::unique_ptr<uint8_t[]> in(new uint8_t[(size_t)cut]);
            memcpy(in.get(), file.data(), (size_t)cut);
            run(in.get(), cut, max_raw, &hostile, nullptr);
        }
        // the chunks of the intact file: [type .. data) ranges and where their CRC fields are
        std::vector<int64_t> crc_of((size_t)n, -1), first_of((size_t)n, 0);
        std::vector<uint8_t> zstream, head, tail;                // the IDAT data, and the file in front of / behind the IDAT chunks
        for (int64_t pos = 8;;) {
            uint32_t type = 0; int64_t at = 0, cl = 0;
            if (png_chunk_at(file.data(), n, pos, &type, &at, &cl)) break;
            for (int64_t i = at - 4; i < at + cl; ++i) { crc_of[(size_t)i] = at + cl; first_of[(size_t)i] = at - 4; }
            if (type == png_tag('I', 'D', 'A', 'T')) zstream.insert(zstream.end(), file.begin() + at, file.begin() + at + cl);
            else (zstream.empty() ? head : tail).insert((zstream.empty() ? head : tail).end(), file.begin() + pos, file.begin() + at + cl + 4);
            pos = at + cl + 4;
        }
        head.insert(head.begin(), file.begin(), file.begin() + 8);
        static const uint8_t subst[2] = {0x00, 0xFF};
        std::unique_ptr<uint8_t[]> in(new uint8_t[(size_t)n]);
        for (int64_t at = 0; at < n; ++at)
            for (uint8_t v : subst) {
                if (file[(size_t)at] == v) continue;
                memcpy(in.get(), file.data(), (size_t)n);
                in[(size_t)at] = v;
                run(in.get(), n, max_raw, &hostile, nullptr);
                const int64_t c = crc_of[(size_t)at];
                if (c < 0) continue;
                const uint32_t crc = png_crc32(0, in.get() + first_of[(size_t)at], c - first_of[(size_t)at]);
                in[(size_t)c] = (uint8_t)(crc >> 24); in[(size_t)c + 1] = (uint8_t)(crc >> 16); in[(size_t)c + 2] = (uint8_t)(crc >> 8); in[(size_t)c + 3] = (uint8_t)crc;
                run(in.get(), n, max_raw, &hostile, nullptr);
            }
        for (size_t cut = 0; cut < zstream.size(); ++cut) {      // every prefix of the zlib stream in one IDAT chunk with a good CRC
            std::vector<uint8_t> idat = {(uint8_t)(cut >> 24), (uint8_t)(cut >> 16), (uint8_t)(cut >> 8), (uint8_t)cut, 'I', 'D', 'A', 'T'};
            idat.insert(idat.end(), zstream.begin(), zstream.begin() + (int64_t)cut);
            const uint32_t crc = png_crc32(0, idat.data() + 4, (int64_t)idat.size() - 4);
            for (int k = 3; k >= 0; --k) idat.push_back((uint8_t)(crc >> (8 * k)));
            const size_t total = head.size() + idat.size() + tail.size();
            std::unique_ptr<uint8_t[]> f(new uint8_t[total]);
            memcpy(f.get(), head.data(), head.size());
            memcpy(f.get() + head.size(), idat.data(), idat.size());
            if (!tail.empty()) memcpy(f.get() + head.size() + idat.size(), tail.data(), tail.size());
            run(f.get(), (int64_t)total, max_raw, &hostile, nullptr);
        }
    }
    printf("png_inflate_check: %d files, %ld hostile inputs (%ld decoded, %ld refused, %ld unsupported), %ld failures\n", (argc - 1) / 2,
           hostile.tried, hostile.decoded, hostile.refused, hostile.unsupported, intact.failures + hostile.failures);
    return intact.failures + hostile.failures ? 1 : 0;
}

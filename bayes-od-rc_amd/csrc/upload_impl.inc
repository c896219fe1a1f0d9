// Frame uploads (bayesod.h: bod_upload_frames_*; DESIGN.md 9.4, 9.6, 9.11, 9.13, 9.15); included at the end of engine.hip.  uint8 RGB
// frames -- uniform, or packed with a size per frame, as host bytes or as JPEG / PNG files the library decodes -- go to a uint8
// staging buffer on the device, optionally through a pending corruption, and from there through one preprocess kernel into an image
// buffer: synchronously on the main stream into d_images, or pipelined on the copy stream into image buffer 0 / 1 (UploadDest).
// The stateless decoder entry points and bod_augment_boxes, which share the formats and the geometry, close the file.  (The header
// and host-stage entry points, bod_{jpeg,png}_info and their like, are host code alone and stay in engine.hip.)

// Resize / crop / pad geometry of ONE frame for a network input of H x W (every upload route, and bod_augment_boxes).  0 = ok;
// 1 = the resize degenerates (g->rh, g->rw say how); 2 = no resize asked for and the frame is not at the network size.
// scale / off_y / off_x are the augmented route's (bayesod.h, bod_augment): the resize target grows by `scale`, and the crop or the
// pad of an axis takes the share `off` of the size difference.  Their defaults are every other route's: the target is the network
// size and floor(0.5 * d) is the centred d / 2 of tf.image.resize_with_crop_or_pad.
static int frame_geometry(int32_t H, int32_t W, int32_t src_h, int32_t src_w, int32_t aspect_resize, PreprocFrame* g,
                          float scale = 1.f, float off_y = 0.5f, float off_x = 0.5f) {
    PreprocFrame a{};
    a.sh = src_h; a.sw = src_w;
    a.rh = src_h; a.rw = src_w;
    const double kMaxSide = 1048576.0;                                      // (a resized side beyond 2^20 pixels is no resize any more)
    auto scaled = [&](int32_t n, int32_t* out) {
        const double t = std::max(1.0, std::floor((double)scale * (double)n + 0.5));
        *out = t <= kMaxSide ? (int32_t)t : -1;
        return t <= kMaxSide;
    };
    if (aspect_resize) {
        // tf.image.resize(..., preserve_aspect_ratio=True): scale = min(H/sh, W/sw) in float32, size = round(s * in)
        int32_t th = 0, tw = 0;
        if (!scaled(H, &th) || !scaled(W, &tw)) { a.rh = th; a.rw = tw; *g = a; return 1; }
        const float fh = (float)th / (float)src_h, fw = (float)tw / (float)src_w;
        const float sc = fh < fw ? fh : fw;
        const float nh = std::nearbyint(sc * (float)src_h), nw = std::nearbyint(sc * (float)src_w);
        a.rh = nh <= (float)kMaxSide ? (int32_t)nh : -1;
        a.rw = nw <= (float)kMaxSide ? (int32_t)nw : -1;
        if (a.rh < 1 || a.rw < 1) { *g = a; return 1; }
    } else if (src_h != H || src_w != W) {
        return 2;
    } else if (!scaled(src_h, &a.rh) || !scaled(src_w, &a.rw)) {
        *g = a;
        return 1;
    }
    a.scale_y = (float)src_h / (float)a.rh; a.scale_x = (float)src_w / (float)a.rw;
    // resize_with_crop_or_pad, the offsets at the share `off` of the difference (0.5: its centred floor division)
    auto place = [](int d, float off, int32_t* crop, int32_t* pad) {
        *crop = d > 0 ? (int32_t)std::floor((double)off * (double)d) : 0;
        *pad = d < 0 ? (int32_t)std::floor((double)off * (double)-d) : 0;
    };
    place(a.rh - H, off_y, &a.crop_y, &a.pad_y);
    place(a.rw - W, off_x, &a.crop_x, &a.pad_x);
    a.vis_h = std::min(a.rh, H); a.vis_w = std::min(a.rw, W);
    *g = a;
    return 0;
}

static bod_status preproc_geometry(bod_handle h, int32_t src_h, int32_t src_w, const float* rgb_means, int32_t aspect_resize, PreprocArgs* out) {
    const bod_config& c = h->cfg;
    PreprocFrame g{};
    const int bad = frame_geometry(c.image_h, c.image_w, src_h, src_w, aspect_resize, &g);
    if (bad == 1) return h->fail(BOD_ERR_INVALID_ARG, "bod_upload_frames_u8: degenerate resize %dx%d", g.rh, g.rw);
    if (bad == 2)
        return h->fail(BOD_ERR_INVALID_ARG, "bod_upload_frames_u8: frames are %dx%d but the handle expects %dx%d (pass aspect_resize=1 for "
                       "the KITTI-style resize + crop/pad)", src_h, src_w, c.image_h, c.image_w);
    PreprocArgs a{};
    a.B = c.batch; a.sh = g.sh; a.sw = g.sw; a.H = c.image_h; a.W = c.image_w; a.resize = aspect_resize ? 1 : 0;
    a.rh = g.rh; a.rw = g.rw; a.scale_y = g.scale_y; a.scale_x = g.scale_x;
    a.crop_y = g.crop_y; a.crop_x = g.crop_x; a.pad_y = g.pad_y; a.pad_x = g.pad_x; a.vis_h = g.vis_h; a.vis_w = g.vis_w;
    for (int k = 0; k < 3; ++k) a.mean[k] = rgb_means[k];
    *out = a;
    return BOD_OK;
}

// A ragged batch's table on the host (PreprocFrame records, then the [batch][2] factors) and its packed byte count.  Nothing of the
// handle's upload state has changed when this fails.
static bod_status ragged_table(bod_handle h, const char* who, const int32_t* src_hw, int32_t aspect_resize, bod_context::RaggedTable* t,
                               size_t* bytes, bool* with_factors) {
    const bod_config& c = h->cfg;
    const size_t B = (size_t)c.batch;
    t->host.resize(B * (sizeof(PreprocFrame) + 2 * sizeof(float)));
    PreprocFrame* fr = reinterpret_cast<PreprocFrame*>(t->host.data());
    float* fac = reinterpret_cast<float*>(t->host.data() + B * sizeof(PreprocFrame));
    int64_t off = 0;
    for (int b = 0; b < c.batch; ++b) {
        const int32_t sh = src_hw[2 * b], sw = src_hw[2 * b + 1];
        if (sh < 1 || sw < 1) return h->fail(BOD_ERR_INVALID_ARG, "%s: frame %d has size %dx%d", who, b, sh, sw);
        PreprocFrame g{};
        const int bad = frame_geometry(c.image_h, c.image_w, sh, sw, aspect_resize, &g);
        if (bad == 1) return h->fail(BOD_ERR_INVALID_ARG, "%s: frame %d (%dx%d): degenerate resize %dx%d", who, b, sh, sw, g.rh, g.rw);
        if (bad == 2)
            return h->fail(BOD_ERR_INVALID_ARG, "%s: frame %d is %dx%d but the handle expects %dx%d (pass aspect_resize=1 for the "
                           "KITTI-style resize + crop/pad)", who, b, sh, sw, c.image_h, c.image_w);
        g.offset = off;
        off += (int64_t)3 * sh * sw;
        fr[b] = g;
        // S = orig / net per sample (inference_utils.py:147-167), rounded as make_config rounds the handle's pair
        fac[2 * b] = (float)((double)sh / (double)c.image_h);
        fac[2 * b + 1] = (float)((double)sw / (double)c.image_w);
    }
    *bytes = (size_t)off;
    *with_factors = aspect_resize && c.kitti_scale_h > 0.f;
    return BOD_OK;
}

// What is wrong with an augmentation record (nullptr: nothing).
static const char* augment_bad(const bod_augment& a) {
    if (a.flip != 0 && a.flip != 1) return "flip must be 0 or 1";
    if (!std::isfinite(a.scale) || !(a.scale > 0.f)) return "scale must be finite and positive";
    if (!(a.off_y >= 0.f && a.off_y <= 1.f) || !(a.off_x >= 0.f && a.off_x <= 1.f)) return "off_y and off_x must lie in [0, 1]";
    if (!std::isfinite(a.gain) || !std::isfinite(a.bias)) return "gain and bias must be finite";
    return nullptr;
}

// The augmented route's table: [batch] PreprocAugFrame records, no factors (a KITTI handle's own two scalars apply).  As
// ragged_table, nothing of the handle's upload state has changed when this fails.
static bod_status augment_table(bod_handle h, const char* who, const int32_t* src_hw, int32_t aspect_resize, const bod_augment* aug,
                                bod_context::RaggedTable* t, size_t* bytes) {
    const bod_config& c = h->cfg;
    t->host.resize((size_t)c.batch * sizeof(PreprocAugFrame));
    PreprocAugFrame* fr = reinterpret_cast<PreprocAugFrame*>(t->host.data());
    int64_t off = 0;
    for (int b = 0; b < c.batch; ++b) {
        const int32_t sh = src_hw[2 * b], sw = src_hw[2 * b + 1];
        if (sh < 1 || sw < 1) return h->fail(BOD_ERR_INVALID_ARG, "%s: frame %d has size %dx%d", who, b, sh, sw);
        if (const char* why = augment_bad(aug[b])) return h->fail(BOD_ERR_INVALID_ARG, "%s: frame %d: %s", who, b, why);
        PreprocAugFrame r{};
        const int bad = frame_geometry(c.image_h, c.image_w, sh, sw, aspect_resize, &r.g, aug[b].scale, aug[b].off_y, aug[b].off_x);
        if (bad == 1) return h->fail(BOD_ERR_INVALID_ARG, "%s: frame %d (%dx%d): degenerate resize %dx%d", who, b, sh, sw, r.g.rh, r.g.rw);
        if (bad == 2)
            return h->fail(BOD_ERR_INVALID_ARG, "%s: frame %d is %dx%d but the handle expects %dx%d (pass aspect_resize=1 for the "
                           "KITTI-style resize + crop/pad)", who, b, sh, sw, c.image_h, c.image_w);
        r.g.offset = off;
        off += (int64_t)3 * sh * sw;
        r.flip = aug[b].flip;
        r.resize = (aspect_resize || r.g.rh != sh || r.g.rw != sw) ? 1 : 0;
        r.gain = aug[b].gain; r.bias = aug[b].bias;
        fr[b] = r;
    }
    *bytes = (size_t)off;
    return BOD_OK;
}

// Device side of a route's table and the two snapshots, on first use.
static bod_status ragged_alloc(bod_handle h, const char* who, bod_context::RaggedTable* t) {
    const size_t n = t->host.size(), fb = (size_t)h->cfg.batch * 2 * sizeof(float);
    if (!t->dev && hipMalloc(reinterpret_cast<void**>(&t->dev), n) != hipSuccess) { t->dev = nullptr; return h->fail(BOD_ERR_OOM, "%s: %zu bytes of frame table", who, n); }
    for (int k = 0; k < 2; ++k)
        if (!h->kscale_cur[k] && hipMalloc(reinterpret_cast<void**>(&h->kscale_cur[k]), fb) != hipSuccess) {
            h->kscale_cur[k] = nullptr;
            return h->fail(BOD_ERR_OOM, "%s: %zu bytes of frame factors", who, fb);
        }
    return BOD_OK;
}

static PreprocRaggedArgs ragged_args(bod_handle h, const bod_context::RaggedTable& t, const float* rgb_means, int32_t aspect_resize) {
    PreprocRaggedArgs a{};
    a.frames = reinterpret_cast<const PreprocFrame*>(t.dev);
    a.B = h->cfg.batch; a.H = h->cfg.image_h; a.W = h->cfg.image_w; a.resize = aspect_resize ? 1 : 0;
    for (int k = 0; k < 3; ++k) a.mean[k] = rgb_means[k];
    return a;
}
static PreprocAugArgs augment_args(bod_handle h, const bod_context::RaggedTable& t, const float* rgb_means) {
    PreprocAugArgs a{};
    a.frames = reinterpret_cast<const PreprocAugFrame*>(t.dev);
    a.B = h->cfg.batch; a.H = h->cfg.image_h; a.W = h->cfg.image_w;
    for (int k = 0; k < 3; ++k) a.mean[k] = rgb_means[k];
    return a;
}
static const float* ragged_factors(bod_handle h, const bod_context::RaggedTable& t) {
    return reinterpret_cast<const float*>(t.dev + (size_t)h->cfg.batch * sizeof(PreprocFrame));
}

// (a pending corruption is described per frame of a PACKED batch: the uniform uploads refuse it and leave it pending)
static const char* const CORRUPT_UNIFORM_MSG =
    "an upload corruption is pending (bod_set_upload_corruption): it applies to the ragged, augmented and JPEG uploads only";

// ------------------------------------------------------------------------------------------------
// Encoded frames: JPEG (DESIGN.md 9.11; Huffman decoding on host threads, jpeg_entropy.h; the rest on the device, jpeg_kernels.hip)
// and PNG (DESIGN.md 9.15; chunk parsing and inflate on host threads, png_inflate.h; the scanline filters on the device,
// png_kernels.hip).  A format is a struct of what differs: its header and record types, how frame i is laid out in the batch, the
// decode of one frame into the pinned payload, what it leaves in the slot, and its launches.
// ------------------------------------------------------------------------------------------------
#define DECODE_FAIL(st, ...) do { char _b[512]; snprintf(_b, sizeof _b, __VA_ARGS__); *err = _b; return (st); } while (0)

struct JpegFormat {
    typedef JpegHeader Header;
    typedef JpegFrame Frame;
    static constexpr const char* NAME = "JPEG";
    static constexpr const char* PAYLOAD = "coefficient";
    static constexpr const char* PAYLOADS = "coefficients";
    struct Layout { int64_t coefs = 0, planes = 0, rgb = 0, max_blocks = 0, max_groups = 0, idct_wgs = 0, color_wgs = 0; };
    static int parse(const uint8_t* d, int64_t len, Header* h) { return jpeg_parse(d, len, h); }
    static void place(const Header& h, Frame* f, Layout* l) {
        for (int c = 0; c < h.components; ++c) {
            f->coef_off[c] = l->coefs + h.coef_off[c];
            f->plane_off[c] = l->planes;
            f->bw[c] = h.bw[c]; f->bh[c] = h.bh[c];
            l->planes += (int64_t)h.bw[c] * h.bh[c] * 64;          // (multiples of 64: every offset stays 16-byte aligned)
        }
        f->rgb_off = l->rgb;
        f->components = h.components; f->h_samp = h.h_samp; f->v_samp = h.v_samp; f->width = h.width; f->height = h.height;
        l->coefs += h.coef_count;
        l->max_blocks = std::max(l->max_blocks, h.coef_count / 64);
        l->max_groups = std::max(l->max_groups, (int64_t)h.height * ((h.width + 3) / 4));
        l->rgb += (int64_t)3 * h.height * h.width;
    }
    // every frame gets the workgroups of the largest (kernels.h, JpegArgs): both grids must fit a launch
    static bod_status launch_limit(const char* who, int32_t n, Layout* l, std::string* err) {
        l->idct_wgs = (l->max_blocks + 31) / 32; l->color_wgs = (l->max_groups + 255) / 256;
        if (n * l->idct_wgs > 0x7FFFFFFF || n * l->color_wgs > 0x7FFFFFFF)
            DECODE_FAIL(BOD_ERR_INVALID_ARG, "%s: %d frames of up to %lld blocks are more than one launch covers", who, n, (long long)l->max_blocks);
        return BOD_OK;
    }
    static size_t payload_bytes(const Layout& l) { return (size_t)l.coefs * sizeof(int16_t); }
    static int decode(const uint8_t* d, int64_t len, const Header& h, Frame* f, char* payload, char* msg, size_t cap) {
        return jpeg_decode(d, len, h, reinterpret_cast<int16_t*>(payload) + (f->coef_off[0] - h.coef_off[0]), &f->quant[0][0], msg, cap);
    }
    static void finish(const Layout& l, DecodeSlot* s) {
        s->scratch_bytes = (size_t)l.planes; s->idct_wgs_per_frame = (int32_t)l.idct_wgs; s->color_wgs_per_frame = (int32_t)l.color_wgs;
    }
    static hipError_t launch(const DecodeSlot& s, uint8_t* rgb_dst, hipStream_t stream) {
        JpegArgs a{};
        a.frames = reinterpret_cast<const JpegFrame*>(s.dev);
        a.coefs = reinterpret_cast<const int16_t*>(s.dev + s.payload_base);
        a.planes = s.scratch; a.rgb = rgb_dst; a.n = s.n; a.idct_wgs_per_frame = s.idct_wgs_per_frame; a.color_wgs_per_frame = s.color_wgs_per_frame;
        const hipError_t e = launch_jpeg_idct(a, stream);
        return e != hipSuccess ? e : launch_jpeg_color(a, stream);
    }
};

struct PngFormat {
    typedef PngHeader Header;
    typedef PngFrame Frame;
    static constexpr const char* NAME = "PNG";
    static constexpr const char* PAYLOAD = "scanline";
    static constexpr const char* PAYLOADS = "scanlines";
    struct Layout { int64_t raw = 0, rgb = 0; int32_t max_h = 0; };
    static int parse(const uint8_t* d, int64_t len, Header* h) { return png_parse(d, len, h); }
    static void place(const Header& h, Frame* f, Layout* l) {
        f->raw_off = l->raw; f->rgb_off = l->rgb;
        f->height = h.height; f->width = h.width; f->channels = h.channels;
        l->raw += h.raw_bytes;                                     // (each at most 65535 * (1 + 4 * 65535): n of them stay far inside int64)
        l->rgb += (int64_t)3 * h.height * h.width;
        l->max_h = std::max(l->max_h, h.height);
    }
    static bod_status launch_limit(const char*, int32_t, Layout*, std::string*) { return BOD_OK; }      // (bands: any height fits)
    static size_t payload_bytes(const Layout& l) { return (size_t)l.raw; }
    static int decode(const uint8_t* d, int64_t len, const Header& h, Frame* f, char* payload, char* msg, size_t cap) {
        return png_decode(d, len, h, reinterpret_cast<uint8_t*>(payload) + f->raw_off, msg, cap);
    }
    static void finish(const Layout& l, DecodeSlot* s) {
        s->rows_per_band = std::min(PNG_MAX_BAND_ROWS, (l.max_h + 63) / 64 * 64);     // one thread per row; taller frames go band by band
    }
    static hipError_t launch(const DecodeSlot& s, uint8_t* rgb_dst, hipStream_t stream) {
        PngArgs a{};
        a.frames = reinterpret_cast<const PngFrame*>(s.dev);
        a.raw = reinterpret_cast<const uint8_t*>(s.dev + s.payload_base);
        a.rgb = rgb_dst; a.n = s.n; a.rows_per_band = s.rows_per_band;
        return launch_png_unfilter(a, stream);
    }
};

// Host half of a batch: parse every header, lay the batch out, wait until the previous copy has left the slot's pinned staging, then
// decode the files into it on `threads` threads (at most 16, at most one per frame; the calling thread alone when that is 1).
// Nothing is enqueued and nothing of a handle changes here; `data` is no longer needed afterwards.  src_hw: [n][2].
template <class F>
static bod_status host_decode(DecodeSlot& s, const char* who, int32_t n, const uint8_t* const* data, const int64_t* len, int32_t threads,
                              int32_t* src_hw, std::string* err) try {
    std::vector<typename F::Header> hd((size_t)n);
    std::vector<typename F::Frame> fr((size_t)n);
    typename F::Layout lay;
    for (int i = 0; i < n; ++i) {
        if (!data[i] || len[i] < 0) DECODE_FAIL(BOD_ERR_INVALID_ARG, "%s: frame %d has no data", who, i);
        typename F::Header& h = hd[(size_t)i];
        if (F::parse(data[i], len[i], &h) != 0) DECODE_FAIL(BOD_ERR_INVALID_ARG, "%s: frame %d is corrupt: %s", who, i, h.msg);
        if (!h.supported) DECODE_FAIL(BOD_ERR_INVALID_ARG, "%s: frame %d is not a supported %s: %s", who, i, F::NAME, h.msg);
        F::place(h, &fr[(size_t)i], &lay);
        src_hw[2 * i] = h.height; src_hw[2 * i + 1] = h.width;
    }
    BODCHK(F::launch_limit(who, n, &lay, err));
    const size_t payload_base = ((size_t)n * sizeof(typename F::Frame) + 127) & ~(size_t)127;
    const size_t stage_bytes = payload_base + F::payload_bytes(lay);
    if (s.copied && hipEventSynchronize(s.copied) != hipSuccess) DECODE_FAIL(BOD_ERR_HIP, "%s: waiting for the previous %s copy failed", who, F::PAYLOAD);
    if (stage_bytes > s.pinned_cap) {
        if (s.pinned) hipHostFree(s.pinned);
        s.pinned = nullptr; s.pinned_cap = 0;
        if (hipHostMalloc(reinterpret_cast<void**>(&s.pinned), stage_bytes, hipHostMallocDefault) != hipSuccess) {
            s.pinned = nullptr;
            DECODE_FAIL(BOD_ERR_OOM, "%s: %zu bytes of pinned %s staging", who, stage_bytes, F::PAYLOAD);
        }
        s.pinned_cap = stage_bytes;
    }
    char* payload = s.pinned + payload_base;
    std::vector<int> status((size_t)n, 0);
    std::vector<std::array<char, 192>> msgs((size_t)n);
    std::atomic<int> next{0};
    auto work = [&]() {
        for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) {
            msgs[(size_t)i][0] = 0;
            status[(size_t)i] = F::decode(data[i], len[i], hd[(size_t)i], &fr[(size_t)i], payload, msgs[(size_t)i].data(), msgs[(size_t)i].size());
        }
    };
    const int workers = std::max(1, std::min(std::min(threads, 16), n));
    {
        // the calling thread is one of the workers: whatever could not be started is decoded here
        std::vector<std::thread> pool;
        pool.reserve((size_t)workers);
        try { for (int k = 1; k < workers; ++k) pool.emplace_back(work); } catch (const std::system_error&) {}
        work();
        for (std::thread& t : pool) t.join();
    }
    for (int i = 0; i < n; ++i)
        if (status[(size_t)i] != 0) DECODE_FAIL(BOD_ERR_INVALID_ARG, "%s: frame %d is corrupt: %s", who, i, msgs[(size_t)i].data());
    std::memcpy(s.pinned, fr.data(), (size_t)n * sizeof(typename F::Frame));
    s.n = n; s.stage_bytes = stage_bytes; s.payload_base = payload_base; s.rgb_bytes = lay.rgb;
    F::finish(lay, &s);
    return BOD_OK;
} catch (const std::bad_alloc&) {
    DECODE_FAIL(BOD_ERR_OOM, "%s: out of host memory for %d frame headers", who, n);
}

// Device half: one copy of the records + payload, then the format's kernels, which leave the packed RGB frames at rgb_dst (room for
// s.rgb_bytes).  The slot's device buffers grow here; `stream` is the only stream that ever touches them.
template <class F>
static bod_status decode_enqueue(DecodeSlot& s, const char* who, uint8_t* rgb_dst, hipStream_t stream, std::string* err) {
    if (s.stage_bytes > s.dev_cap || s.scratch_bytes > s.scratch_cap) {
        if (hipStreamSynchronize(stream) != hipSuccess) DECODE_FAIL(BOD_ERR_HIP, "%s: hipStreamSynchronize failed", who);
        if (s.stage_bytes > s.dev_cap) {
            if (s.dev) hipFree(s.dev);
            s.dev = nullptr; s.dev_cap = 0;
            if (hipMalloc(reinterpret_cast<void**>(&s.dev), s.stage_bytes) != hipSuccess) { s.dev = nullptr; DECODE_FAIL(BOD_ERR_OOM, "%s: %zu bytes of %s", who, s.stage_bytes, F::PAYLOADS); }
            s.dev_cap = s.stage_bytes;
        }
        if (s.scratch_bytes > s.scratch_cap) {
            if (s.scratch) hipFree(s.scratch);
            s.scratch = nullptr; s.scratch_cap = 0;
            if (hipMalloc(reinterpret_cast<void**>(&s.scratch), s.scratch_bytes) != hipSuccess) { s.scratch = nullptr; DECODE_FAIL(BOD_ERR_OOM, "%s: %zu bytes of component planes", who, s.scratch_bytes); }
            s.scratch_cap = s.scratch_bytes;
        }
    }
    if (!s.copied && hipEventCreateWithFlags(&s.copied, hipEventDisableTiming) != hipSuccess) { s.copied = nullptr; DECODE_FAIL(BOD_ERR_HIP, "%s: hipEventCreate failed", who); }
    hipError_t e = hipMemcpyAsync(s.dev, s.pinned, s.stage_bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipEventRecord(s.copied, stream);
    if (e == hipSuccess) e = F::launch(s, rgb_dst, stream);
    if (e != hipSuccess) DECODE_FAIL(BOD_ERR_HIP, "%s: %s device stage failed: %s", who, F::NAME, hipGetErrorString(e));
    return BOD_OK;
}

// The two halves of each DecodeKind, for the callers that take the kind as a value.
struct Decoder {
    bod_status (*host)(DecodeSlot&, const char*, int32_t, const uint8_t* const*, const int64_t*, int32_t, int32_t*, std::string*);
    bod_status (*enqueue)(DecodeSlot&, const char*, uint8_t*, hipStream_t, std::string*);
};
static const Decoder DECODERS[DECODE_KINDS] = {{host_decode<JpegFormat>, decode_enqueue<JpegFormat>},
                                               {host_decode<PngFormat>, decode_enqueue<PngFormat>}};

// Frame corruptions (DESIGN.md 9.13): the pending one-shot description of bod_set_upload_corruption in a packed upload.  The host half
// runs before anything of the upload is enqueued; the device half runs between the frames' arrival and the preprocess kernel and
// consumes the description.
static bod_status corrupt_prepare_pending(bod_handle h, const char* who, const int32_t* src_hw, CorruptSlot* slot, hipStream_t stream) {
    char err[512] = {0};
    const int st = corrupt_prepare(*slot, who, h->corrupt_pending, src_hw, stream, err, sizeof err);
    return st == BOD_OK ? BOD_OK : h->fail((bod_status)st, "%s", err);
}
static bod_status corrupt_run_pending(bod_handle h, const char* who, CorruptSlot* slot, uint8_t* buf, hipStream_t stream, const uint8_t** result) {
    char err[512] = {0};
    uint8_t* out = buf;
    const int st = corrupt_enqueue(*slot, who, h->corrupt_pending, buf, stream, &out, err, sizeof err);
    if (st != BOD_OK) return h->fail((bod_status)st, "%s", err);
    *result = out;
    h->corrupt_pending = CorruptSpec{};
    return BOD_OK;
}

// ------------------------------------------------------------------------------------------------
// Where an upload lands.  The synchronous route (buffer -1) works on the main stream: uint8 staging d_frames_u8, image buffer
// d_images, every buffer its own, and it ends with a stream synchronize, so nothing of it is in flight between calls.  The pipelined
// route works on the copy stream into image buffer 0 / 1 (0 is d_images again), with that buffer's staging, tables, decode and
// corruption slots.  Its events: ev_img_free[k] (recorded by the forward behind the stem that read buffer k) is waited for ON the
// copy stream before buffer k and its staging are rewritten; ev_img_ready[k] is recorded behind the preprocess kernel for the
// forward to wait on; ev_tab[k], DecodeSlot::copied and CorruptSlot::copied each say that a copy has left a HOST buffer, and the
// host waits for them before it rewrites that buffer.  The copy stream alone touches the pipelined staging and slots.
// ------------------------------------------------------------------------------------------------
struct UploadDest {
    hipStream_t stream;                           // (pipelined: null until open_pipelined has made the copy stream)
    uint8_t*& u8; size_t& u8_cap;                 // the uint8 staging, grown on demand
    float* images;                                // (pipelined: null until open_pipelined has allocated the buffer)
    bod_context::RaggedTable& rag; bod_context::RaggedTable& aug;
    CorruptSlot* corrupt;
    int32_t buffer;                               // 0 / 1, or -1: synchronous
};
static UploadDest upload_dest(bod_handle h, int32_t buffer) {
    if (buffer < 0) return UploadDest{h->stream, h->d_frames_u8, h->frames_u8_cap, h->d_images, h->rag_sync, h->aug_sync, &h->corrupt_slot[2], -1};
    return UploadDest{h->copy, h->d_u8_b[buffer], h->u8_cap_b[buffer], h->d_images_b[buffer], h->rag_b[buffer], h->aug_b[buffer],
                      &h->corrupt_slot[buffer], buffer};
}

// The pipelined route's stream, events and image buffer, on first use.
static bod_status open_pipelined(bod_handle h, UploadDest* d) {
    const bod_config& c = h->cfg;
    if (!h->copy) {
        HIPCHK(h, hipStreamCreateWithFlags(&h->copy, hipStreamNonBlocking));
        for (int k = 0; k < 2; ++k) {
            HIPCHK(h, hipEventCreateWithFlags(&h->ev_img_ready[k], hipEventDisableTiming));
            HIPCHK(h, hipEventCreateWithFlags(&h->ev_img_free[k], hipEventDisableTiming));
        }
    }
    // (no zero fill: dalloc's memset would run on the main stream, behind the forward in flight, and land on the frames)
    if (!h->d_images_b[d->buffer]) BODCHK(h->dalloc(&h->d_images_b[d->buffer], (size_t)c.batch * c.image_h * c.image_w * 3, false));
    d->stream = h->copy; d->images = h->d_images_b[d->buffer];
    return BOD_OK;
}

// Room for `bytes` in the staging.  The old buffer is freed once its stream has drained: the last upload's kernels read it.
static bod_status grow_staging(bod_handle h, const char* who, const UploadDest& d, size_t bytes) {
    if (bytes <= d.u8_cap) return BOD_OK;
    if (d.u8) { HIPCHK(h, hipStreamSynchronize(d.stream)); hipFree(d.u8); d.u8 = nullptr; d.u8_cap = 0; }
    if (hipMalloc(reinterpret_cast<void**>(&d.u8), bytes) != hipSuccess) { d.u8 = nullptr; return h->fail(BOD_ERR_OOM, "%s: %zu bytes of staging", who, bytes); }
    d.u8_cap = bytes;
    return BOD_OK;
}

// Do not overwrite frames a forward pass still has to read (its stem records ev_img_free), nor frames of an upload nobody consumed
// yet (same stream: ordered).  The frames AND the table of a buffer stay until the forward that reads them has passed its stem (it
// snapshots the factors in front of ev_img_free: stage_images).
static bod_status wait_writable(bod_handle h, const UploadDest& d) {
    if (h->img_free_pending[d.buffer]) { HIPCHK(h, hipStreamWaitEvent(d.stream, h->ev_img_free[d.buffer], 0)); h->img_free_pending[d.buffer] = false; }
    else if (d.buffer == 0) {                                                 // buffer 0 doubles as the synchronous d_images
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (h->front) HIPCHK(h, hipStreamSynchronize(h->front));
    }
    return BOD_OK;
}

// The frames of a packed batch: bytes on the host, or a batch the host half of a decoder has left in a slot.
struct PackedSource {
    const uint8_t* host = nullptr;
    DecodeSlot* slot = nullptr; DecodeKind kind = DECODE_JPEG;
};

// The upload of a packed batch, ragged (aug == nullptr) or augmented -- they differ in their table and their kernel only --,
// synchronous (buffer -1) or pipelined into image buffer 0 / 1.
static bod_status upload_packed(bod_handle h, const char* who, const PackedSource& src, const int32_t* src_hw, const float* rgb_means,
                                int32_t aspect_resize, const bod_augment* aug, int32_t buffer) {
    MarkerRange mr_api("bod:upload");
    const bool pipelined = buffer >= 0;
    // prologue: validate, then make room.  Nothing but the wait for ev_img_free is enqueued here, and the frames the handle holds
    // stay as they are when it fails.
    if (!pipelined) BODCHK(join_overlap(h));
    HIPCHK(h, hipSetDevice(h->cfg.device));
    UploadDest d = upload_dest(h, buffer);
    bod_context::RaggedTable& t = aug ? d.aug : d.rag;
    // the host side of the table is rewritten below.  Pipelined: the copy of this buffer's previous one (two uploads back) must have
    // left it (one event per buffer for both kinds of table: they are copied on the one copy stream, so the latest copy is the last
    // to end).  Synchronous: the previous upload of this kind synchronized the stream.
    if (pipelined && h->ev_tab[buffer]) HIPCHK(h, hipEventSynchronize(h->ev_tab[buffer]));
    size_t bytes = 0; bool with_factors = false;
    if (aug) BODCHK(augment_table(h, who, src_hw, aspect_resize, aug, &t, &bytes));
    else BODCHK(ragged_table(h, who, src_hw, aspect_resize, &t, &bytes, &with_factors));
    BODCHK(ragged_alloc(h, who, &t));
    if (pipelined) BODCHK(open_pipelined(h, &d));
    const bool corrupt = h->corrupt_pending.n != 0;
    if (corrupt) BODCHK(corrupt_prepare_pending(h, who, src_hw, d.corrupt, d.stream));
    BODCHK(grow_staging(h, who, d, bytes));
    if (pipelined) BODCHK(wait_writable(h, d));

    // the upload on d.stream: table, frames, corruption, preprocess
    HIPCHK(h, hipMemcpyAsync(t.dev, t.host.data(), t.host.size(), hipMemcpyHostToDevice, d.stream));
    if (pipelined) {
        if (!h->ev_tab[buffer]) HIPCHK(h, hipEventCreateWithFlags(&h->ev_tab[buffer], hipEventDisableTiming));
        HIPCHK(h, hipEventRecord(h->ev_tab[buffer], d.stream));
    }
    if (src.slot) {
        std::string err;
        const bod_status st = DECODERS[src.kind].enqueue(*src.slot, who, d.u8, d.stream, &err);
        if (st != BOD_OK) return h->fail(st, "%s", err.c_str());
    } else {
        HIPCHK(h, hipMemcpyAsync(d.u8, src.host, bytes, hipMemcpyHostToDevice, d.stream));
    }
    // (the corruption's scratch, like the staging, is touched on the upload's stream alone: the preprocess kernel behind it is its last reader)
    const uint8_t* frames_u8 = d.u8;
    if (corrupt) BODCHK(corrupt_run_pending(h, who, d.corrupt, d.u8, d.stream, &frames_u8));
    if (aug) {
        PreprocAugArgs a = augment_args(h, t, rgb_means);
        a.src = frames_u8; a.dst = d.images;
        HIPCHK(h, launch_preprocess_augment(a, d.stream));
    } else {
        PreprocRaggedArgs a = ragged_args(h, t, rgb_means, aspect_resize);
        a.src = frames_u8; a.dst = d.images;
        HIPCHK(h, launch_preprocess_ragged(a, d.stream));
    }

    // epilogue: hand the buffer over
    if (pipelined) {
        HIPCHK(h, hipEventRecord(h->ev_img_ready[buffer], d.stream));
        h->img_ready_pending[buffer] = true;
    } else {
        HIPCHK(h, hipStreamSynchronize(d.stream));       // the caller may reuse its frames on return
    }
    h->kscale_src[pipelined ? buffer : 0] = with_factors ? ragged_factors(h, t) : nullptr;
    return BOD_OK;
}

// The JPEG and PNG upload routes: the host decode first (nothing of the handle has changed when it fails, and `data` is free once it
// is done), then the ragged or augmented upload with the decoded batch in the place of the packed host frames.
static bod_status upload_encoded(bod_handle h, DecodeKind kind, const char* who, const uint8_t* const* data, const int64_t* len,
                                 const float* rgb_means, int32_t aspect_resize, const bod_augment* aug, int32_t threads, int32_t* src_hw_out,
                                 int32_t buffer) {
    if (!h || !data || !len || !rgb_means) return BOD_ERR_INVALID_ARG;
    if (buffer < -1 || buffer > 1) return h->fail(BOD_ERR_INVALID_ARG, "%s: buffer must be 0 or 1", who);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    PackedSource src;
    src.slot = &h->decode_slot[kind][buffer < 0 ? 2 : buffer]; src.kind = kind;
    std::vector<int32_t> hw((size_t)h->cfg.batch * 2);
    std::string err;
    const bod_status st = DECODERS[kind].host(*src.slot, who, h->cfg.batch, data, len, threads, hw.data(), &err);
    if (st != BOD_OK) return h->fail(st, "%s", err.c_str());
    if (src_hw_out) std::memcpy(src_hw_out, hw.data(), hw.size() * sizeof(int32_t));
    return upload_packed(h, who, src, hw.data(), rgb_means, aspect_resize, aug, buffer);
}

// The decoder alone (bod_jpeg_decode_rgb, bod_png_decode_rgb): n files -> packed RGB on the host.  Stateless; its buffers live for
// the call.
static bod_status decode_rgb(DecodeKind kind, const char* who, int32_t device, int32_t n, const uint8_t* const* data, const int64_t* len,
                             int32_t threads, uint8_t* rgb_packed, int64_t rgb_capacity, int32_t* src_hw) {
    if (n < 1 || !data || !len || !rgb_packed || !src_hw) { g_create_error = std::string(who) + ": NULL argument or no frame"; return BOD_ERR_INVALID_ARG; }
    return pdq_call(device, [&](hipStream_t s, char* err, size_t cap) -> int {
        DecodeSlot slot;
        std::string e;
        uint8_t* d_rgb = nullptr;
        bod_status st = DECODERS[kind].host(slot, who, n, data, len, threads, src_hw, &e);
        if (st == BOD_OK && slot.rgb_bytes > rgb_capacity) {
            e = std::string(who) + ": the frames take " + std::to_string(slot.rgb_bytes) + " bytes, the buffer holds " + std::to_string(rgb_capacity);
            st = BOD_ERR_INVALID_ARG;
        }
        if (st == BOD_OK && hipMalloc(reinterpret_cast<void**>(&d_rgb), (size_t)slot.rgb_bytes) != hipSuccess) {
            d_rgb = nullptr; e = std::string(who) + ": out of device memory for the frames"; st = BOD_ERR_OOM;
        }
        if (st == BOD_OK) st = DECODERS[kind].enqueue(slot, who, d_rgb, s, &e);
        if (st == BOD_OK && (hipMemcpyAsync(rgb_packed, d_rgb, (size_t)slot.rgb_bytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
                             hipStreamSynchronize(s) != hipSuccess)) {
            e = std::string(who) + ": copying the frames back failed: " + hipGetErrorString(hipGetLastError()); st = BOD_ERR_HIP;
        }
        hipStreamSynchronize(s);
        if (d_rgb) hipFree(d_rgb);
        slot.release();
        if (st != BOD_OK) snprintf(err, cap, "%s", e.c_str());
        return st;
    });
}

extern "C" {

bod_status bod_upload_frames_u8(bod_handle h, const uint8_t* rgb, int32_t src_h, int32_t src_w, const float* rgb_means,
                                int32_t aspect_resize) {
    static const char* who = "bod_upload_frames_u8";
    MarkerRange mr_api("bod:upload");
    if (!h || !rgb || !rgb_means || src_h < 1 || src_w < 1) return BOD_ERR_INVALID_ARG;
    if (h->corrupt_pending.n) return h->fail(BOD_ERR_INVALID_ARG, "%s: %s", who, CORRUPT_UNIFORM_MSG);
    BODCHK(join_overlap(h));
    const bod_config& c = h->cfg;
    HIPCHK(h, hipSetDevice(c.device));
    PreprocArgs a{};
    BODCHK(preproc_geometry(h, src_h, src_w, rgb_means, aspect_resize, &a));
    const UploadDest d = upload_dest(h, -1);
    const size_t bytes = (size_t)c.batch * src_h * src_w * 3;
    BODCHK(grow_staging(h, who, d, bytes));
    a.src = d.u8; a.dst = d.images;
    HIPCHK(h, hipMemcpyAsync(d.u8, rgb, bytes, hipMemcpyHostToDevice, d.stream));
    HIPCHK(h, launch_preprocess(a, d.stream));
    HIPCHK(h, hipStreamSynchronize(d.stream));        // the caller may reuse `rgb` on return
    h->kscale_src[0] = nullptr;
    return BOD_OK;
}

bod_status bod_upload_frames_u8_async(bod_handle h, const uint8_t* rgb, int32_t src_h, int32_t src_w, const float* rgb_means,
                                      int32_t aspect_resize, int32_t buffer) {
    static const char* who = "bod_upload_frames_u8_async";
    MarkerRange mr_api("bod:upload");
    if (!h || !rgb || !rgb_means || src_h < 1 || src_w < 1) return BOD_ERR_INVALID_ARG;
    if (buffer < 0 || buffer > 1) return h->fail(BOD_ERR_INVALID_ARG, "%s: buffer must be 0 or 1", who);
    const bod_config& c = h->cfg;
    HIPCHK(h, hipSetDevice(c.device));
    if (h->corrupt_pending.n) return h->fail(BOD_ERR_INVALID_ARG, "%s: %s", who, CORRUPT_UNIFORM_MSG);
    PreprocArgs a{};
    BODCHK(preproc_geometry(h, src_h, src_w, rgb_means, aspect_resize, &a));
    UploadDest d = upload_dest(h, buffer);
    BODCHK(open_pipelined(h, &d));
    const size_t bytes = (size_t)c.batch * src_h * src_w * 3;
    BODCHK(grow_staging(h, who, d, bytes));
    BODCHK(wait_writable(h, d));
    a.src = d.u8; a.dst = d.images;
    HIPCHK(h, hipMemcpyAsync(d.u8, rgb, bytes, hipMemcpyHostToDevice, d.stream));
    HIPCHK(h, launch_preprocess(a, d.stream));
    HIPCHK(h, hipEventRecord(h->ev_img_ready[buffer], d.stream));
    h->img_ready_pending[buffer] = true;
    h->kscale_src[buffer] = nullptr;
    return BOD_OK;
}

bod_status bod_upload_frames_u8_ragged(bod_handle h, const uint8_t* rgb_packed, const int32_t* src_hw, const float* rgb_means,
                                       int32_t aspect_resize) {
    if (!h || !rgb_packed || !src_hw || !rgb_means) return BOD_ERR_INVALID_ARG;
    return upload_packed(h, "bod_upload_frames_u8_ragged", PackedSource{rgb_packed}, src_hw, rgb_means, aspect_resize, nullptr, -1);
}

bod_status bod_upload_frames_u8_augmented(bod_handle h, const uint8_t* rgb_packed, const int32_t* src_hw, const float* rgb_means,
                                          int32_t aspect_resize, const bod_augment* aug) {
    if (!h || !rgb_packed || !src_hw || !rgb_means || !aug) return BOD_ERR_INVALID_ARG;
    return upload_packed(h, "bod_upload_frames_u8_augmented", PackedSource{rgb_packed}, src_hw, rgb_means, aspect_resize, aug, -1);
}

bod_status bod_upload_frames_u8_ragged_async(bod_handle h, const uint8_t* rgb_packed, const int32_t* src_hw, const float* rgb_means,
                                             int32_t aspect_resize, int32_t buffer) {
    static const char* who = "bod_upload_frames_u8_ragged_async";
    if (!h || !rgb_packed || !src_hw || !rgb_means) return BOD_ERR_INVALID_ARG;
    if (buffer < 0 || buffer > 1) return h->fail(BOD_ERR_INVALID_ARG, "%s: buffer must be 0 or 1", who);
    return upload_packed(h, who, PackedSource{rgb_packed}, src_hw, rgb_means, aspect_resize, nullptr, buffer);
}

bod_status bod_upload_frames_u8_augmented_async(bod_handle h, const uint8_t* rgb_packed, const int32_t* src_hw, const float* rgb_means,
                                                int32_t aspect_resize, const bod_augment* aug, int32_t buffer) {
    static const char* who = "bod_upload_frames_u8_augmented_async";
    if (!h || !rgb_packed || !src_hw || !rgb_means || !aug) return BOD_ERR_INVALID_ARG;
    if (buffer < 0 || buffer > 1) return h->fail(BOD_ERR_INVALID_ARG, "%s: buffer must be 0 or 1", who);
    return upload_packed(h, who, PackedSource{rgb_packed}, src_hw, rgb_means, aspect_resize, aug, buffer);
}

bod_status bod_upload_frames_jpeg(bod_handle h, const uint8_t* const* data, const int64_t* len, const float* rgb_means,
                                  int32_t aspect_resize, const bod_augment* aug, int32_t threads, int32_t* src_hw_out) {
    return upload_encoded(h, DECODE_JPEG, "bod_upload_frames_jpeg", data, len, rgb_means, aspect_resize, aug, threads, src_hw_out, -1);
}

bod_status bod_upload_frames_jpeg_async(bod_handle h, const uint8_t* const* data, const int64_t* len, const float* rgb_means,
                                        int32_t aspect_resize, const bod_augment* aug, int32_t threads, int32_t* src_hw_out, int32_t buffer) {
    if (h && (buffer < 0 || buffer > 1)) return h->fail(BOD_ERR_INVALID_ARG, "bod_upload_frames_jpeg_async: buffer must be 0 or 1");
    return upload_encoded(h, DECODE_JPEG, "bod_upload_frames_jpeg_async", data, len, rgb_means, aspect_resize, aug, threads, src_hw_out, buffer);
}

bod_status bod_upload_frames_png(bod_handle h, const uint8_t* const* data, const int64_t* len, const float* rgb_means,
                                 int32_t aspect_resize, const bod_augment* aug, int32_t threads, int32_t* src_hw_out) {
    return upload_encoded(h, DECODE_PNG, "bod_upload_frames_png", data, len, rgb_means, aspect_resize, aug, threads, src_hw_out, -1);
}

bod_status bod_upload_frames_png_async(bod_handle h, const uint8_t* const* data, const int64_t* len, const float* rgb_means,
                                       int32_t aspect_resize, const bod_augment* aug, int32_t threads, int32_t* src_hw_out, int32_t buffer) {
    if (h && (buffer < 0 || buffer > 1)) return h->fail(BOD_ERR_INVALID_ARG, "bod_upload_frames_png_async: buffer must be 0 or 1");
    return upload_encoded(h, DECODE_PNG, "bod_upload_frames_png_async", data, len, rgb_means, aspect_resize, aug, threads, src_hw_out, buffer);
}

// Ground truth through an augmented frame's geometry (bayesod.h): host arithmetic only, in fp32, no device call.
bod_status bod_augment_boxes(int32_t B, const int32_t* src_hw, int32_t net_h, int32_t net_w, int32_t aspect_resize, const bod_augment* aug,
                             const int32_t* num_gt, const float* gt_boxes_vuvu_src, const float* gt_classes, int32_t C, float min_visible,
                             int32_t* num_out, float* boxes_out, float* classes_out) {
#pragma clang fp contract(off)                          // multiply, then add: the float32 restatement of the tests rounds twice
    auto fail = [](const char* fmt, auto... args) {
        char buf[512];
        snprintf(buf, sizeof(buf), fmt, args...);
        g_create_error = buf;
        return BOD_ERR_INVALID_ARG;
    };
    static const char* who = "bod_augment_boxes";
    if (B < 1 || net_h < 1 || net_w < 1 || C < 2 || !std::isfinite(min_visible))
        return fail("%s: bad argument (B = %d, network %dx%d, C = %d >= 2, min_visible finite)", who, B, net_h, net_w, C);
    if (!src_hw || !aug || !num_gt || !gt_boxes_vuvu_src || !gt_classes || !num_out || !boxes_out || !classes_out)
        return fail("%s: a required array is NULL", who);
    // everything is checked before the first output is written
    std::vector<PreprocFrame> geo((size_t)B);
    for (int b = 0; b < B; ++b) {
        const int32_t sh = src_hw[2 * b], sw = src_hw[2 * b + 1];
        if (sh < 1 || sw < 1) return fail("%s: frame %d has size %dx%d", who, b, sh, sw);
        if (num_gt[b] < 0) return fail("%s: frame %d has %d ground-truth rows", who, b, num_gt[b]);
        if (const char* why = augment_bad(aug[b])) return fail("%s: frame %d: %s", who, b, why);
        const int bad = frame_geometry(net_h, net_w, sh, sw, aspect_resize, &geo[b], aug[b].scale, aug[b].off_y, aug[b].off_x);
        if (bad == 1) return fail("%s: frame %d (%dx%d): degenerate resize %dx%d", who, b, sh, sw, geo[b].rh, geo[b].rw);
        if (bad == 2) return fail("%s: frame %d is %dx%d but the network size is %dx%d (pass aspect_resize=1 for the KITTI-style "
                                  "resize + crop/pad)", who, b, sh, sw, net_h, net_w);
    }
    size_t in = 0, out = 0;
    for (int b = 0; b < B; ++b) {
        const PreprocFrame& g = geo[b];
        const float ky = (float)((double)g.rh / (double)g.sh), kx = (float)((double)g.rw / (double)g.sw);
        const float dy = (float)(g.pad_y - g.crop_y), dx = (float)(g.pad_x - g.crop_x);
        const float ymax = (float)(net_h - 1), xmax = (float)(net_w - 1), wm1 = (float)(g.sw - 1);
        int32_t kept = 0;
        for (int i = 0; i < num_gt[b]; ++i, ++in) {
            const float* q = gt_boxes_vuvu_src + 4 * in;
            float x1 = q[1], x2 = q[3];
            if (aug[b].flip) { const float t = wm1 - x2; x2 = wm1 - x1; x1 = t; }
            const float ty1 = q[0] * ky + dy, tx1 = x1 * kx + dx, ty2 = q[2] * ky + dy, tx2 = x2 * kx + dx;
            const float cy1 = std::min(std::max(ty1, 0.f), ymax), cx1 = std::min(std::max(tx1, 0.f), xmax);
            const float cy2 = std::min(std::max(ty2, 0.f), ymax), cx2 = std::min(std::max(tx2, 0.f), xmax);
            const float ch = cy2 - cy1, cw = cx2 - cx1;
            const float full = (ty2 - ty1) * (tx2 - tx1);
            if (!(ch >= 1.f) || !(cw >= 1.f) || ch * cw < min_visible * full) continue;
            float* o = boxes_out + 4 * out;
            o[0] = cy1; o[1] = cx1; o[2] = cy2; o[3] = cx2;
            std::copy(gt_classes + (size_t)C * in, gt_classes + (size_t)C * (in + 1), classes_out + (size_t)C * out);
            ++out; ++kept;
        }
        if (!kept) {                                    // the dataset handlers' row for a frame without ground truth
            float* o = boxes_out + 4 * out;
            o[0] = 0.f; o[1] = 0.f; o[2] = 1.f; o[3] = 1.f;
            std::fill(classes_out + (size_t)C * out, classes_out + (size_t)C * (out + 1), 0.f);
            classes_out[(size_t)C * out + C - 1] = 1.f;
            ++out; kept = 1;
        }
        num_out[b] = kept;
    }
    return BOD_OK;
}

bod_status bod_jpeg_decode_rgb(int32_t device, int32_t n, const uint8_t* const* data, const int64_t* len, int32_t threads,
                               uint8_t* rgb_packed, int64_t rgb_capacity, int32_t* src_hw) {
    return decode_rgb(DECODE_JPEG, "bod_jpeg_decode_rgb", device, n, data, len, threads, rgb_packed, rgb_capacity, src_hw);
}

bod_status bod_png_decode_rgb(int32_t device, int32_t n, const uint8_t* const* data, const int64_t* len, int32_t threads,
                              uint8_t* rgb_packed, int64_t rgb_capacity, int32_t* src_hw) {
    return decode_rgb(DECODE_PNG, "bod_png_decode_rgb", device, n, data, len, threads, rgb_packed, rgb_capacity, src_hw);
}

// The PNG decoder's two halves timed apart (bayesod.h; tests/tools/bench_png.py): the host half as the uploads run it, on the
// library's own worker threads, by the host clock; png_unfilter_kernel alone by events around each launch.
bod_status bod_bench_png_decode(int32_t device, int32_t n, const uint8_t* const* data, const int64_t* len, int32_t threads, int32_t iters,
                                double* host_ms, double* kernel_ms) {
    static const char* who = "bod_bench_png_decode";
    if (n < 1 || iters < 1 || !data || !len || !host_ms || !kernel_ms) { g_create_error = std::string(who) + ": NULL argument, no frame or no iteration"; return BOD_ERR_INVALID_ARG; }
    return pdq_call(device, [&](hipStream_t s, char* err, size_t cap) -> int {
        DecodeSlot ps;
        std::string e;
        uint8_t* d_rgb = nullptr;
        hipEvent_t ev[2] = {nullptr, nullptr};
        std::vector<int32_t> hw((size_t)n * 2);
        bod_status st = BOD_OK;
        for (int i = 0; i < iters && st == BOD_OK; ++i) {
            const auto t0 = std::chrono::steady_clock::now();
            st = host_decode<PngFormat>(ps, who, n, data, len, threads, hw.data(), &e);
            host_ms[i] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        if (st == BOD_OK && hipMalloc(reinterpret_cast<void**>(&d_rgb), (size_t)ps.rgb_bytes) != hipSuccess) {
            d_rgb = nullptr; e = std::string(who) + ": out of device memory for the frames"; st = BOD_ERR_OOM;
        }
        if (st == BOD_OK) st = decode_enqueue<PngFormat>(ps, who, d_rgb, s, &e);   // the copy, and one launch that is not timed
        if (st == BOD_OK && (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess)) { e = std::string(who) + ": hipEventCreate failed"; st = BOD_ERR_HIP; }
        for (int i = 0; i < iters && st == BOD_OK; ++i) {
            float ms = 0.f;
            hipError_t he = hipEventRecord(ev[0], s);
            if (he == hipSuccess) he = PngFormat::launch(ps, d_rgb, s);
            if (he == hipSuccess) he = hipEventRecord(ev[1], s);
            if (he == hipSuccess) he = hipEventSynchronize(ev[1]);
            if (he == hipSuccess) he = hipEventElapsedTime(&ms, ev[0], ev[1]);
            if (he != hipSuccess) { e = std::string(who) + ": timing the kernel failed: " + hipGetErrorString(he); st = BOD_ERR_HIP; }
            kernel_ms[i] = ms;
        }
        hipStreamSynchronize(s);
        for (hipEvent_t v : ev) if (v) hipEventDestroy(v);
        if (d_rgb) hipFree(d_rgb);
        ps.release();
        if (st != BOD_OK) snprintf(err, cap, "%s", e.c_str());
        return st;
    });
}

}  // extern "C"

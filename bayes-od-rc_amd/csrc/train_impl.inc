// Training step (SURVEY.md section 8 f1; run_training.train_single_step, run_training.py:208-247): included at the
// end of engine.hip.  Forward = the inference plan with every activation kept and dropout on; backward = a generic
// executor over the same op list -- per convolution: output-gradient gather through the row table (activation
// mask, residual scatter), weight gradient and input gradient as two GEMMs on the forward MFMA kernel
// (im2col^T / transposed dY for the former, folded weights in [(tap, ci)][cout] order + col2im for the latter);
// fp32 master parameters, gradients and Adam moments live in four parallel arenas.
//
// Two precisions share this executor.  bf16 (the product): bf16 activations / folded weights / dZ, fp32 accumulation, the MFMA
// bf16 kernel.  fp32 (precision = BOD_PRECISION_FP32 with training = 1, the gradient-verification mode): every tensor fp32, the
// GEMMs on conv_igemm_f32 (exact fp32 MFMA, no split-K), the element-type-templated scalar forms of the gather / transpose /
// pool kernels -- same op walk, same gradient routing, same unfold / loss / optimizer kernels.  Its gradients meet float64
// autograd element-wise (tests/test_gpu_train_step.py), which bf16 storage cannot (two bf16-storage evaluations that differ only
// in summation order already decorrelate at the level of the bf16 rounding noise after ~10 layers).
struct ParamRef { size_t off = 0; size_t n = 0; bool present = false; };

struct TrainConv {               // one convolution (= one group of one op)
    std::string name, bn;
    int taps = 0, kw = 0, cin = 0, cout = 0, cout_pad = 0;
    ParamRef kernel, bias, gamma, beta;
    float* mean = nullptr; float* var = nullptr;          // BatchNorm moving statistics (not trained: training=False everywhere, SURVEY A.3)
    uint16_t* w_fwd = nullptr; float* b_fwd = nullptr;    // the plan's packed weights (rewritten every step)
    uint16_t* w_bwd = nullptr;                            // [(tap, ci)][cout_pad] for the input gradient
    uint16_t* w_flip = nullptr;                           // [cin][flipped taps][cout_pad]: input gradient as a convolution (same_geom layers)
    float l2 = 0.f;
};

// Second host thread for the weight-gradient stream: the step is about a thousand small launches, and one thread
// enqueueing both streams is the bottleneck at small minibatches.  Jobs are run in order; job ids let the main
// thread wait (on the host) until a job's closing hipEventRecord has been ISSUED before it enqueues a wait on it.
struct SideWorker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::function<hipError_t()>> q;
    bool stop = false;
    std::atomic<long> issued{0}, finished{0};
    std::atomic<int> err{0};
    int device = 0;
    void start(int dev) {
        device = dev;
        th = std::thread([this] {
            (void)hipSetDevice(device);
            for (;;) {
                std::function<hipError_t()> job;
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [this] { return stop || !q.empty(); });
                    if (q.empty()) return;
                    job = std::move(q.front()); q.pop_front();
                }
                const hipError_t e = job();
                if (e != hipSuccess) { int zero = 0; err.compare_exchange_strong(zero, (int)e); }
                finished.fetch_add(1, std::memory_order_release);
            }
        });
    }
    long push(std::function<hipError_t()> job) {
        const long id = issued.fetch_add(1) + 1;
        { std::lock_guard<std::mutex> lk(mu); q.push_back(std::move(job)); }
        cv.notify_one();
        return id;
    }
    void wait_for(long id) const { while (finished.load(std::memory_order_acquire) < id) std::this_thread::yield(); }
    void shutdown() {
        if (!th.joinable()) return;
        { std::lock_guard<std::mutex> lk(mu); stop = true; }
        cv.notify_one();
        th.join();
    }
};

struct TrainState {
    static constexpr int WS = 2;                          // dZ^T slots (and weight-gradient streams)
    SideWorker worker; bool use_worker = false; long slot_job[WS] = {0, 0};
    std::vector<TrainConv> convs;
    std::map<std::string, int> index;                     // conv name -> convs[]
    size_t arena_n = 0;
    float *master = nullptr, *grad = nullptr, *adam_m = nullptr, *adam_v = nullptr;
    std::map<const void*, float*> grad_of;                // activation buffer -> fp32 gradient buffer (same element count)
    std::map<const void*, size_t> grad_elems;
    float* act_grad_arena = nullptr; size_t act_grad_n = 0;   // all activation-gradient planes, zeroed by one memset per step
    // scratch (sized for the largest layer)
    uint16_t *dz = nullptr, *dyt2[WS] = {nullptr, nullptr};
    std::map<std::tuple<const RowEnt*, long, int>, uint16_t*> dzp_of;   // (row table, plane bytes, group) -> dZ plane
    // weight gradients run on a second stream (they feed nothing downstream): dZ^T is double-buffered between the streams
    // (3 / 4 slots and streams measured: 10.8 / 10.9 / 10.9 ms at three ResNet-101 frames -- the main stream
    // does not wait for slots; what the weight-gradient work costs the step (1.9 ms) is its share of the chip)
    // slot k of the dZ^T double buffer owns scratch set k and, for small minibatches, its own stream: consecutive layers'
    // weight gradients then overlap (8.3 -> 7.8 ms at 3 frames, 14.6 -> 13.8 at 8, 23.8 -> 22.9 at 16); at 32 frames of
    // 512x512 the kernels fill the chip by themselves and the extra concurrency costs 3 % (42.8 -> 44.3 ms): one stream
    hipStream_t wstreams[WS] = {nullptr, nullptr}; bool two_wgrad_streams = true;
    uint16_t* xct2[WS] = {nullptr, nullptr}; float *partial2[WS] = {nullptr, nullptr}, *dwp2[WS] = {nullptr, nullptr}, *dot2[WS] = {nullptr, nullptr};
    hipEvent_t ev_ready[WS] = {nullptr, nullptr}, ev_done[WS] = {nullptr, nullptr}; bool pending[WS] = {false, false}; int flip = 0;
    float *dxcol = nullptr, *zero_bias = nullptr;
    float* dgrad_partial = nullptr; size_t dgrad_partial_n = 0;   // split-K partials of the input-gradient launches (main stream)
    bool f32 = false; const float* cur_images = nullptr;   // fp32 handle: element size 4 everywhere; this step's device frames (stem weight gradient)
    RowEnt* iota = nullptr; size_t iota_n = 0;
    std::map<const RowEnt*, RowEnt*> dgrad_rows;         // forward table of a 1x1 layer -> its input-gradient table
    // stem
    float* stem_w32 = nullptr;                            // the plan's stem weights (fp32 [147][64]) are rewritten too
    uint16_t* img_bf16 = nullptr; RowEnt* stem_rows = nullptr; uint16_t* stem_dz = nullptr;
    // loss
    float *cls_t = nullptr, *box_t = nullptr; uint8_t *pos = nullptr, *neg = nullptr;
    // ground truth of bod_train_step_boxes: packed host copy, its device buffer (grown on demand) and the event of the last upload
    PackedGt gt_host; char* gt_dev = nullptr; size_t gt_cap = 0; hipEvent_t gt_ev = nullptr; bool gt_pending = false;
    float *loss_partial = nullptr, *loss_sums = nullptr, *scalars = nullptr, *sumsq_partial = nullptr;   // scalars: [0] l2 loss, [1] sum of squared gradients
    int loss_blocks = 0;
    long step = 0;
    float l2_rate = 0.f;                                  // this step's rate (read by the weight-gradient pass)
    FoldArgs* fold_desc = nullptr; long fold_max = 0;      // device array of the per-layer fold/pack descriptors
    // per-step scalars on the device: {seed_lo, seed_hi, image_base, lr_t (float bits)} -- the recorded step reads them
    uint32_t* dyn = nullptr;
    // the whole step as one hipGraph (about 1 000 launches: at the yaml's minibatch the eager step is host-launch-bound)
    hipGraphExec_t graph = nullptr; std::string graph_key; int eager_runs = 0; bool graph_off = false;
};

namespace {

// splits of the pixel reduction of a weight-gradient GEMM: enough for ~512 workgroups, >= 4 K-tiles each
int wgrad_splits(size_t M, size_t N, size_t cout_pad, bool f32 = false) {
    if (f32) return 1;                            // conv_igemm_f32 has no split-K path
    const long tiles = (long)((N + 127) / 128) * (long)(cout_pad % 128 == 0 ? cout_pad / 128 : cout_pad / 64);
    int S = 1;
    while (tiles * S < 512 && S < 64 && (long)M / (64L * S * 2) >= 4) S *= 2;
    return S;
}

// splits of the channel reduction of an input-gradient launch (the forward pass's rule, engine.hip add_conv): layers with too few
// output tiles to fill the chip and a long reduction -- most of stages 4 / 5 at the yaml's minibatch of three
int dgrad_splits(long M, int k_channels, int taps, int cout_pad, int groups) {
    const long tiles = ((M + 127) / 128) * (cout_pad % 128 == 0 ? cout_pad / 128 : cout_pad / 64) * groups;
    const int chunks = k_channels / 64;
    int S = 1;
    while (tiles * S < 256 && S * 2 <= 16 && chunks % (S * 2) == 0 && (long)taps * (chunks / (S * 2)) >= 4) S *= 2;
    return S;
}

float* grad_buffer(bod_context* h, const void* act, size_t elems) {
    TrainState* t = h->train;
    auto it = t->grad_of.find(act);
    if (it != t->grad_of.end()) return it->second;
    float* g = nullptr;
    if (h->dalloc(&g, elems) != BOD_OK) return nullptr;
    t->grad_of[act] = g; t->grad_elems[act] = elems;
    return g;
}

size_t act_elems_of(bod_context* h, const void* act, size_t elem_bytes) {
    auto it = h->alloc_bytes.find(act);
    return it == h->alloc_bytes.end() ? 0 : it->second / elem_bytes;
}

bod_status add_train_conv(bod_context* h, const std::string& name, const std::string& bn, size_t* cursor) {
    TrainState* t = h->train;
    if (t->index.count(name)) return BOD_OK;
    const HostTensor* k = find_w(h, name, 0);
    if (!k) return h->fail(BOD_ERR_NOT_READY, "training: missing kernel '%s'", name.c_str());
    TrainConv c;
    c.name = name; c.bn = bn;
    c.taps = (int)(k->shape[0] * k->shape[1]); c.kw = (int)k->shape[1]; c.cin = (int)k->shape[2]; c.cout = (int)k->shape[3];
    auto claim = [&](ParamRef& r, size_t n) { r.off = *cursor; r.n = n; r.present = true; *cursor += (n + 63) & ~(size_t)63; };
    claim(c.kernel, k->data.size());
    if (find_w(h, name, 1)) claim(c.bias, (size_t)c.cout);
    if (!bn.empty()) { claim(c.gamma, (size_t)c.cout); claim(c.beta, (size_t)c.cout); }
    // Keras l2(1e-6) on the header tower convs and on cov_out only (multitask_headers.py:85-94,196-205,304-314; SURVEY A.10)
    const bool tower = name.find("pyramid_") == 0 && name.size() > 2 && name[name.size() - 2] == '_';
    c.l2 = (tower || name == "pyramid_cov") ? 1.0f : 0.f;      // multiplied by the step's l2_rate
    t->index[name] = (int)t->convs.size();
    t->convs.push_back(c);
    return BOD_OK;
}

}  // namespace

namespace {

bod_status train_init(bod_context* h) {
    h->train = new TrainState();
    TrainState* t = h->train;
    const bod_config& c = h->cfg;
    t->f32 = h->es == 4;
    if (t->f32) t->graph_off = true;              // the fp32 conv kernel reads the dropout seed from its arguments, not from t->dyn
    const size_t em = h->es / 2;                  // element-count multiplier of the uint16_t-typed scratch allocations
    // ---- parameter arenas, in op order (stem first)
    size_t cursor = 0;
    BODCHK(add_train_conv(h, "conv1", "bn_conv1", &cursor));
    for (const Op& o : h->ops)
        if (o.kind == Op::CONV)
            for (int g = 0; g < o.conv.groups; ++g) BODCHK(add_train_conv(h, o.wname[g], o.bnname[g], &cursor));
    t->arena_n = cursor;
    BODCHK(h->dalloc(&t->master, cursor)); BODCHK(h->dalloc(&t->grad, cursor));
    BODCHK(h->dalloc(&t->adam_m, cursor)); BODCHK(h->dalloc(&t->adam_v, cursor));
    std::vector<float> host(cursor, 0.f);
    size_t max_nk_cout = 0, max_cout_pad = 64, max_n = 0;
    for (TrainConv& tc : t->convs) {
        const HostTensor* k = find_w(h, tc.name, 0);
        std::memcpy(host.data() + tc.kernel.off, k->data.data(), k->data.size() * 4);
        if (tc.bias.present) std::memcpy(host.data() + tc.bias.off, find_w(h, tc.name, 1)->data.data(), (size_t)tc.cout * 4);
        if (!tc.bn.empty()) {
            const HostTensor *g = find_w(h, tc.bn, 2), *be = find_w(h, tc.bn, 3), *mu = find_w(h, tc.bn, 4), *var = find_w(h, tc.bn, 5);
            if (!g || !be || !mu || !var) return h->fail(BOD_ERR_NOT_READY, "training: missing batch-norm '%s'", tc.bn.c_str());
            std::memcpy(host.data() + tc.gamma.off, g->data.data(), (size_t)tc.cout * 4);
            std::memcpy(host.data() + tc.beta.off, be->data.data(), (size_t)tc.cout * 4);
            BODCHK(h->dalloc(&tc.mean, (size_t)tc.cout, false)); BODCHK(h->dalloc(&tc.var, (size_t)tc.cout, false));
            HIPCHK(h, hipMemcpyAsync(tc.mean, mu->data.data(), (size_t)tc.cout * 4, hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(tc.var, var->data.data(), (size_t)tc.cout * 4, hipMemcpyHostToDevice, h->stream));
        }
        if (tc.name == "conv1") {
            tc.cout_pad = 64;
        } else {
            auto it = h->packed.find(tc.name);
            if (it == h->packed.end()) return h->fail(BOD_ERR_NOT_READY, "training: conv '%s' is not part of the plan", tc.name.c_str());
            tc.cout_pad = it->second.cout_pad;
            tc.w_fwd = reinterpret_cast<uint16_t*>(it->second.w); tc.b_fwd = it->second.bias;
            BODCHK(h->dalloc(&tc.w_bwd, (size_t)tc.taps * tc.cin * tc.cout_pad * em));
        }
        max_nk_cout = std::max(max_nk_cout, ((size_t)tc.taps * tc.cin + 1) * tc.cout);
        max_cout_pad = std::max<size_t>(max_cout_pad, (size_t)tc.cout_pad);
        max_n = std::max(max_n, (size_t)tc.taps * tc.cin + 1);
    }
    HIPCHK(h, hipMemcpyAsync(t->master, host.data(), cursor * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    t->stem_w32 = h->stem_w;
    // ---- scratch sized for the largest layer
    size_t max_m = (size_t)c.batch * h->sh * h->sw, dz_e = max_m * 64, dyt_e = 0, xct_e = 0, part_e = 0, dxcol_e = 0;
    auto plan_layer = [&](size_t M, size_t taps, size_t cin, size_t cout, size_t cout_pad, bool dgrad) {
        const size_t N = taps * cin + 1;
        const int S = wgrad_splits(M, N, cout_pad, t->f32);
        const size_t Kpad = (M + 64 * S - 1) / (64 * S) * (64 * S);
        dz_e = std::max(dz_e, M * cout_pad); dyt_e = std::max(dyt_e, cout_pad * Kpad); xct_e = std::max(xct_e, N * Kpad);
        part_e = std::max(part_e, (size_t)S * N * cout_pad);
        if (dgrad) dxcol_e = std::max(dxcol_e, M * taps * cin);
        max_m = std::max(max_m, M);
    };
    plan_layer((size_t)c.batch * h->sh * h->sw, 49, 3, 64, 64, false);
    for (const Op& o : h->ops)
        if (o.kind == Op::CONV) plan_layer((size_t)o.conv.M, (size_t)o.conv.taps, (size_t)o.conv.cin, (size_t)o.conv.cout_valid, (size_t)o.conv.cout_pad, true);
    if (!t->f32)
        for (const Op& o : h->ops)
            if (o.kind == Op::CONV) {
                // the three forms of train_backward's input gradient: convolution over the dZ plane (cout_pad = cin), 1x1 GEMM into
                // the plane (cout_pad = cin), GEMM into dXcol (cout_pad = taps * cin); K = the layer's cout_pad in all three
                const ConvArgs& a = o.conv;
                const bool conv_form = o.same_geom && a.out_cstride == a.cout_pad && !(a.flags & CONV_OUT_F32);
                const int cp = conv_form ? a.cin : a.taps * a.cin;
                if (cp % 64) continue;
                const int S = dgrad_splits(a.M, a.cout_pad, conv_form ? 9 : 1, cp, conv_form ? a.groups : 1);
                if (S > 1) t->dgrad_partial_n = std::max(t->dgrad_partial_n, (size_t)S * (conv_form ? a.groups : 1) * a.M * cp);
            }
    if (t->dgrad_partial_n) BODCHK(h->dalloc(&t->dgrad_partial, t->dgrad_partial_n, false));
    for (const Op& o : h->ops)
        if (o.kind == Op::CONV && o.same_geom)
            for (int g = 0; g < o.conv.groups; ++g) {
                TrainConv& tc = t->convs[t->index.at(o.wname[g])];
                if (!tc.w_flip) BODCHK(h->dalloc(&tc.w_flip, (size_t)tc.cin * tc.taps * tc.cout_pad * em));
                // dZ in the output plane's own layout, one buffer per plane geometry: zeroed once here, after which only
                // interior pixels are ever written (every one of them, by each layer's activation backward), so the
                // zero borders the input-gradient convolution reads never need clearing again
                auto it = h->alloc_bytes.find(o.conv.g[g].out);
                if (it == h->alloc_bytes.end()) continue;
                uint16_t*& plane = t->dzp_of[std::make_tuple(o.conv.rows, (long)it->second, g)];
                if (!plane) BODCHK(h->dalloc(reinterpret_cast<char**>(&plane), it->second));
            }
    BODCHK(h->dalloc(&t->dz, dz_e * em));
    for (int k = 0; k < TrainState::WS; ++k) BODCHK(h->dalloc(&t->dyt2[k], dyt_e * em));
    t->two_wgrad_streams = (size_t)c.batch * c.image_h * c.image_w <= (size_t)20 * 512 * 512;
    if (const char* e = getenv("BOD_TRAIN_WGRAD_STREAMS")) t->two_wgrad_streams = atoi(e) >= 2;
    for (int k = 0; k < TrainState::WS; ++k) {
        BODCHK(h->dalloc(&t->xct2[k], xct_e * em));
        HIPCHK(h, hipStreamCreateWithFlags(&t->wstreams[k], hipStreamNonBlocking));
    }
    for (int k = 0; k < TrainState::WS; ++k) {
        HIPCHK(h, hipEventCreateWithFlags(&t->ev_ready[k], hipEventDisableTiming));
        HIPCHK(h, hipEventCreateWithFlags(&t->ev_done[k], hipEventDisableTiming));
    }
    for (int k = 0; k < TrainState::WS; ++k) { BODCHK(h->dalloc(&t->partial2[k], part_e)); BODCHK(h->dalloc(&t->dwp2[k], max_nk_cout)); BODCHK(h->dalloc(&t->dot2[k], 4096)); }
    BODCHK(h->dalloc(&t->dxcol, std::max<size_t>(dxcol_e, 1)));
    BODCHK(h->dalloc(&t->zero_bias, std::max(max_cout_pad, max_n + 64)));
    t->iota_n = std::max(max_m, max_n);
    {
        std::vector<RowEnt> io(t->iota_n);
        for (size_t i = 0; i < io.size(); ++i) { RowEnt e{}; e.in_off = (int32_t)i; e.out_off = (int32_t)i; io[i] = e; }
        BODCHK(h->dalloc(&t->iota, io.size(), false));
        HIPCHK(h, hipMemcpyAsync(t->iota, io.data(), io.size() * sizeof(RowEnt), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    // ---- stem: bf16 image copy + the row table of its 7x7 s2 VALID windows
    {
        const size_t npx = (size_t)c.batch * c.image_h * c.image_w;
        if (!t->f32) BODCHK(h->dalloc(&t->img_bf16, npx * 3));
        std::vector<RowEnt> rows((size_t)c.batch * h->sh * h->sw);
        size_t r = 0;
        for (int b = 0; b < c.batch; ++b)
            for (int y = 0; y < h->sh; ++y)
                for (int x = 0; x < h->sw; ++x) {
                    RowEnt e{};
                    e.in_off = (int32_t)(((int64_t)b * c.image_h + 2 * y) * c.image_w + 2 * x);
                    e.in_pitch = c.image_w;
                    rows[r++] = e;
                }
        BODCHK(h->dalloc(&t->stem_rows, rows.size(), false));
        HIPCHK(h, hipMemcpyAsync(t->stem_rows, rows.data(), rows.size() * sizeof(RowEnt), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        BODCHK(h->dalloc(&t->stem_dz, (size_t)c.batch * h->sh * h->sw * 64 * em));
    }
    // ---- one arena for every activation-gradient plane (a single memset per step instead of ~120)
    {
        std::vector<std::pair<const void*, size_t>> want;
        auto add = [&](const void* p, size_t elem_bytes) {
            if (!p) return;
            for (auto& w : want) if (w.first == p) return;
            const size_t n = act_elems_of(h, p, elem_bytes);
            if (n) want.emplace_back(p, n);
        };
        for (const Op& o : h->ops) {
            if (o.kind == Op::POOL) add(o.conv.g[0].out, h->es);
            if (o.kind != Op::CONV) continue;
            const bool f32out = o.conv.flags & CONV_OUT_F32;
            for (int g = 0; g < o.conv.groups; ++g) {
                add(o.conv.g[g].out, f32out ? 4 : h->es); add(o.conv.g[g].in, h->es); add(o.conv.g[g].res, h->es); add(o.conv.g[g].out_relu, h->es);
            }
        }
        size_t total = 0;
        for (auto& w : want) total += (w.second + 63) & ~(size_t)63;
        BODCHK(h->dalloc(&t->act_grad_arena, total));
        t->act_grad_n = total;
        size_t off = 0;
        for (auto& w : want) { t->grad_of[w.first] = t->act_grad_arena + off; t->grad_elems[w.first] = w.second; off += (w.second + 63) & ~(size_t)63; }
    }
    // ---- loss inputs
    const size_t BA = (size_t)c.batch * h->A;
    BODCHK(h->dalloc(&t->cls_t, BA * c.num_classes)); BODCHK(h->dalloc(&t->box_t, BA * 4));
    BODCHK(h->dalloc(&t->pos, BA)); BODCHK(h->dalloc(&t->neg, BA));
    t->loss_blocks = (int)((BA + 255) / 256);
    BODCHK(h->dalloc(&t->loss_partial, (size_t)t->loss_blocks * 4)); BODCHK(h->dalloc(&t->loss_sums, 4)); BODCHK(h->dalloc(&t->scalars, 4)); BODCHK(h->dalloc(&t->sumsq_partial, 1024)); BODCHK(h->dalloc(&t->dyn, 4));
    return BOD_OK;
}

const uint32_t* train_dyn_rng(bod_context* h) { return h->train ? h->train->dyn : nullptr; }

void train_destroy(bod_context* h) {
    if (TrainState* t = h->train) {
        t->worker.shutdown();
        if (t->graph) hipGraphExecDestroy(t->graph);
        if (t->gt_ev) hipEventDestroy(t->gt_ev);
        if (t->gt_dev) hipFree(t->gt_dev);
        for (int k = 0; k < TrainState::WS; ++k) if (t->wstreams[k]) { hipStreamSynchronize(t->wstreams[k]); hipStreamDestroy(t->wstreams[k]); }
        for (int k = 0; k < TrainState::WS; ++k) { if (t->ev_ready[k]) hipEventDestroy(t->ev_ready[k]); if (t->ev_done[k]) hipEventDestroy(t->ev_done[k]); }
    }
    delete h->train; h->train = nullptr;
}

}  // namespace

namespace {

bod_status train_fold_all(bod_context* h) {
    TrainState* t = h->train;
    if (t->fold_desc) { HIPCHK(h, launch_fold_pack_all(t->fold_desc, (int)t->convs.size(), t->fold_max, h->stream)); return BOD_OK; }
    std::vector<FoldArgs> all;
    for (TrainConv& tc : t->convs) {
        FoldArgs f{};
        f.kernel = t->master + tc.kernel.off; f.bias = tc.bias.present ? t->master + tc.bias.off : nullptr;
        if (!tc.bn.empty()) { f.gamma = t->master + tc.gamma.off; f.beta = t->master + tc.beta.off; f.mean = tc.mean; f.var = tc.var; }
        f.eps = BN_EPS; f.taps = tc.taps; f.cin = tc.cin; f.cout = tc.cout; f.cout_pad = tc.cout_pad; f.f32 = t->f32 ? 1 : 0;
        if (tc.name == "conv1") { f.w_fwd32 = t->stem_w32; f.b_fwd = h->stem_b; }
        else { f.w_fwd = tc.w_fwd; f.w_bwd = tc.w_bwd; f.w_flip = tc.w_flip; f.b_fwd = tc.b_fwd; }
        all.push_back(f);
        t->fold_max = std::max(t->fold_max, (long)f.cout_pad * f.taps * f.cin);
    }
    BODCHK(h->dalloc(&t->fold_desc, all.size(), false));          // first call (eager): every pointer in the descriptors is fixed for the handle's life
    HIPCHK(h, hipMemcpyAsync(t->fold_desc, all.data(), all.size() * sizeof(FoldArgs), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, launch_fold_pack_all(t->fold_desc, (int)t->convs.size(), t->fold_max, h->stream));
    return BOD_OK;
}

// Weight gradient of one convolution.  Main stream: dZ (dense [M][cout_pad] at dz_src) -> dZ^T into the free half of the
// double buffer.  Second stream: im2col^T of the layer input, the pixel-reduction GEMM, split-K reduce, BatchNorm unfold into
// the gradient arena -- concurrently with the main stream's input-gradient chain of this and the following layers.
// Claims the free half of the dZ^T double buffer for one layer (waits for the GEMM that last read it).
struct WgradSlot { int k, S, Kpad; uint16_t* dzt; };
bod_status train_wgrad_slot(bod_context* h, const TrainConv& tc, int M, WgradSlot* slot) {
    TrainState* t = h->train;
    slot->k = t->flip; t->flip = (t->flip + 1) % TrainState::WS;
    slot->S = wgrad_splits((size_t)M, (size_t)(tc.taps * tc.cin + 1), (size_t)tc.cout_pad, t->f32);
    slot->Kpad = (M + 64 * slot->S - 1) / (64 * slot->S) * (64 * slot->S);
    slot->dzt = t->dyt2[slot->k];
    if (t->pending[slot->k]) {
        if (t->slot_job[slot->k]) t->worker.wait_for(t->slot_job[slot->k]);     // its hipEventRecord has been issued
        HIPCHK(h, hipStreamWaitEvent(h->stream, t->ev_done[slot->k], 0));
    }
    return BOD_OK;
}

// dz_src != nullptr: dZ^T still has to be made from the dense dZ; nullptr: the activation-backward launch already wrote it.
bod_status train_wgrad(bod_context* h, TrainConv& tc, const WgradSlot& slot, const uint16_t* dz_src, const void* in, const RowEnt* rows,
                       int in_cstride, int M) {
    TrainState* t = h->train;
    const int k = slot.k, S = slot.S, Kpad = slot.Kpad;
    const int N = tc.taps * tc.cin + 1;
    const bool f32 = t->f32;
    if (dz_src) HIPCHK(h, launch_gather_transpose(dz_src, nullptr, t->dyt2[k], M, Kpad, tc.cout_pad, tc.cout_pad, 1, 1, false, h->stream, f32));
    HIPCHK(h, hipEventRecord(t->ev_ready[k], h->stream));
    hipStream_t ws = t->wstreams[t->two_wgrad_streams ? k : 0];
    ConvArgs a{};
    a.rows = t->iota; a.M = N; a.taps = 1; a.KW = 1; a.cin = Kpad; a.in_cstride = Kpad;
    a.cout_pad = tc.cout_pad; a.cout_valid = tc.cout; a.out_cstride = tc.cout; a.res_cstride = tc.cout; a.groups = 1;
    a.fan_count = 1; a.flags = CONV_OUT_F32;
    a.g[0] = ConvGroup{t->xct2[k], t->dyt2[k], t->zero_bias, t->dwp2[k], nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, 0, 0};
    if (S > 1) { a.ksplit = S; a.partial = t->partial2[k]; }
    UnfoldArgs u{};
    u.dwp = t->dwp2[k]; u.kernel = t->master + tc.kernel.off; u.bias = tc.bias.present ? t->master + tc.bias.off : nullptr;
    if (!tc.bn.empty()) { u.gamma = t->master + tc.gamma.off; u.mean = tc.mean; u.var = tc.var; u.d_gamma = t->grad + tc.gamma.off; u.d_beta = t->grad + tc.beta.off; }
    u.eps = BN_EPS; u.taps = tc.taps; u.cin = tc.cin; u.cout = tc.cout;
    u.d_kernel = t->grad + tc.kernel.off; u.d_bias = tc.bias.present ? t->grad + tc.bias.off : nullptr;
    u.dot = t->dot2[k];
    u.l2 = t->l2_rate * tc.l2; u.l2_loss = t->scalars;          // Keras l2 on the head kernels rides on the unfold pass
    hipEvent_t ready = t->ev_ready[k], done = t->ev_done[k];
    uint16_t* xct = t->xct2[k];
    const int cin = tc.cin, taps = tc.taps, kw = tc.kw;
    auto side = [=]() -> hipError_t {                       // everything the second stream does for this layer
        hipError_t e;
        if ((e = hipStreamWaitEvent(ws, ready, 0)) != hipSuccess) return e;
        if ((e = launch_gather_transpose(in, rows, xct, M, Kpad, cin, in_cstride, taps, kw, true, ws, f32)) != hipSuccess) return e;
        if ((e = f32 ? launch_conv_igemm_f32(a, ws) : launch_conv_igemm(a, ws)) != hipSuccess) return e;
        if ((e = launch_unfold_grad(u, ws)) != hipSuccess) return e;
        return hipEventRecord(done, ws);
    };
    if (t->use_worker) {
        t->slot_job[k] = t->worker.push(side);
    } else {
        t->slot_job[k] = 0;
        HIPCHK(h, side());
    }
    t->pending[k] = true;
    return BOD_OK;
}

// The three input-gradient launches of a convolution whose forward launch is `a` (train_backward; bod_stage_conv_dgrad runs the
// same three on a layer of its own, so what the tests pin is what the step launches).
// 1. stride-1 SAME 3x3 with identical plane layouts: dX = conv(dZ plane, flipped / swapped weights) through the FORWARD row table
//    (window origin and centre pixel coincide in both planes); accumulates in place
ConvArgs dgrad_flip_args(const ConvArgs& a, const void* dzp, const void* w_flip, const float* zero_bias, float* din) {
    ConvArgs d{};
    d.rows = a.rows; d.M = a.M; d.taps = 9; d.KW = 3; d.cin = a.cout_pad; d.in_cstride = a.out_cstride;
    d.cout_pad = a.cin; d.cout_valid = a.cin; d.out_cstride = a.in_cstride; d.res_cstride = a.in_cstride; d.groups = 1; d.fan_count = 1;
    d.flags = CONV_OUT_F32 | CONV_ACCUM;
    d.g[0] = ConvGroup{dzp, w_flip, zero_bias, din, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, 0, 0};
    return d;
}
// 2. 1x1 (any stride): every output pixel owns one input pixel, so the GEMM accumulates straight into the input's gradient plane
//    through the row table of launch_make_dgrad_rows -- no dXcol, no atomics
ConvArgs dgrad_rows_args(const ConvArgs& a, const RowEnt* dgrad_rows, const void* dz, const void* w_bwd, const float* zero_bias, float* din) {
    const int NK = a.taps * a.cin;
    ConvArgs d{};
    d.rows = dgrad_rows; d.M = a.M; d.taps = 1; d.KW = 1; d.cin = a.cout_pad; d.in_cstride = a.cout_pad;
    d.cout_pad = NK; d.cout_valid = NK; d.out_cstride = a.in_cstride; d.res_cstride = a.in_cstride; d.groups = 1; d.fan_count = 1;
    d.flags = CONV_OUT_F32 | CONV_ACCUM;
    d.g[0] = ConvGroup{dz, w_bwd, zero_bias, din, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, 0, 0};
    return d;
}
// 3. everything else: dXcol[m][(tap, ci)] = dZ[m][:] . Wfolded[(tap, ci)][:] (launch_col2im scatters it into the plane)
ConvArgs dgrad_xcol_args(const ConvArgs& a, const RowEnt* iota, const void* dz, const void* w_bwd, const float* zero_bias, float* dxcol) {
    const int NK = a.taps * a.cin;
    ConvArgs d{};
    d.rows = iota; d.M = a.M; d.taps = 1; d.KW = 1; d.cin = a.cout_pad; d.in_cstride = a.cout_pad;
    d.cout_pad = NK; d.cout_valid = NK; d.out_cstride = NK; d.res_cstride = NK; d.groups = 1; d.fan_count = 1;
    d.flags = CONV_OUT_F32;
    d.g[0] = ConvGroup{dz, w_bwd, zero_bias, dxcol, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, 0, 0};
    return d;
}

bod_status train_backward(bod_context* h) {
    TrainState* t = h->train;
    const bod_config& c = h->cfg;
    const bool f32 = t->f32;
    const size_t es = h->es;
    auto gemm = [&](ConvArgs d) {
        if (f32) return launch_conv_igemm_f32(d, h->stream);
        if (t->dgrad_partial && d.cout_pad % 64 == 0 && d.cin % 64 == 0) {
            const int S = dgrad_splits(d.M, d.cin, d.taps, d.cout_pad, d.groups);
            if (S > 1 && (size_t)S * d.groups * d.M * d.cout_pad <= t->dgrad_partial_n) { d.ksplit = S; d.partial = t->dgrad_partial; }
        }
        return launch_conv_igemm(d, h->stream);
    };
    for (int oi = (int)h->ops.size() - 1; oi >= 0; --oi) {
        Op& op = h->ops[oi];
        if (op.kind == Op::CONV) {
            const ConvArgs& a = op.conv;
            const bool f32out = a.flags & CONV_OUT_F32;
            // The input gradients of a grouped launch whose groups read DIFFERENT inputs (tower layers 1..3: one group per
            // head) are issued as ONE grouped convolution after the loop: three times the tiles per launch.  Groups that
            // share their input (layer 0: the pyramid) accumulate into the same plane and stay sequential.
            bool grouped_dgrad = a.groups > 1 && op.same_geom && !f32out && a.out_cstride == a.cout_pad;
            for (int g = 0; g < a.groups && grouped_dgrad; ++g) {
                if (!t->convs[t->index.at(op.wname[g])].w_flip) grouped_dgrad = false;
                for (int q = 0; q < g; ++q) if (a.g[q].in == a.g[g].in) grouped_dgrad = false;
            }
            ConvArgs dgroup{};
            int ndeferred = 0;
            for (int g = 0; g < a.groups; ++g) {
                const ConvGroup& G = a.g[g];
                TrainConv& tc = t->convs[t->index.at(op.wname[g])];
                float* dout = grad_buffer(h, G.out, act_elems_of(h, G.out, f32out ? 4 : es));
                if (!dout) return h->fail(BOD_ERR_OOM, "training: gradient buffer");
                if (G.out_relu) {
                    const size_t n = act_elems_of(h, G.out_relu, es);
                    float* drelu = grad_buffer(h, G.out_relu, n);
                    HIPCHK(h, launch_relu_merge(drelu, G.out, dout, (long)std::min(n, act_elems_of(h, G.out, es)), h->stream, f32));
                }
                ActBwdArgs ab{};
                ab.dout = dout; ab.out_bf16 = (!f32out && (a.flags & (CONV_RELU | CONV_DROPOUT))) ? reinterpret_cast<const uint16_t*>(G.out) : nullptr;
                ab.rows = a.rows; ab.dz = t->dz; ab.M = a.M; ab.cout = a.cout_valid; ab.cout_pad = a.cout_pad;
                ab.out_cstride = a.out_cstride; ab.res_cstride = a.res_cstride;
                ab.scale = (a.flags & CONV_DROPOUT) ? a.drop_scale : 1.0f;
                ab.f32 = f32 ? 1 : 0;
                ab.dres = G.res ? grad_buffer(h, G.res, act_elems_of(h, G.res, es)) : nullptr;
                const bool conv_dgrad = op.same_geom && tc.w_flip && !f32out && a.out_cstride == a.cout_pad;
                if (conv_dgrad) {
                    ab.dzp = t->dzp_of.at(std::make_tuple(a.rows, (long)h->alloc_bytes.at(G.out), grouped_dgrad ? g : 0));
                }
                WgradSlot slot;
                BODCHK(train_wgrad_slot(h, tc, a.M, &slot));
                ab.dzt = slot.dzt; ab.Kpad = slot.Kpad;
                bool transposed = false;
                HIPCHK(h, launch_act_backward_gather(ab, h->stream, &transposed));
                BODCHK(train_wgrad(h, tc, slot, transposed ? nullptr : t->dz, G.in, a.rows, a.in_cstride, a.M));
                // input gradient: dXcol[m][(tap, ci)] = dZ[m][:] . Wfolded[(tap, ci)][:], then col2im into the input's gradient plane
                float* din = grad_buffer(h, G.in, act_elems_of(h, G.in, es));
                if (!din) return h->fail(BOD_ERR_OOM, "training: gradient buffer");
                if (conv_dgrad) {
                    // stride-1 SAME 3x3 with identical plane layouts: dX = conv(dZ plane, flipped / swapped weights) through the
                    // FORWARD row table (window origin and centre pixel coincide in both planes); accumulates in place
                    ConvArgs d = dgrad_flip_args(a, ab.dzp, tc.w_flip, t->zero_bias, din);
                    if (grouped_dgrad) {
                        if (ndeferred == 0) dgroup = d;
                        dgroup.g[ndeferred++] = d.g[0];
                        continue;
                    }
                    HIPCHK(h, gemm(d));
                    continue;
                }
                if (a.taps == 1) {
                    // 1x1 (any stride): every output pixel owns one input pixel, so the GEMM accumulates straight into the
                    // input's gradient plane through a row table -- no dXcol, no atomics
                    RowEnt*& dr = t->dgrad_rows[a.rows];
                    if (!dr) {
                        BODCHK(h->dalloc(&dr, (size_t)a.M, false));
                        HIPCHK(h, launch_make_dgrad_rows(a.rows, dr, a.M, h->stream));
                    }
                    ConvArgs d = dgrad_rows_args(a, dr, t->dz, tc.w_bwd, t->zero_bias, din);
                    HIPCHK(h, gemm(d));
                    continue;
                }
                ConvArgs d = dgrad_xcol_args(a, t->iota, t->dz, tc.w_bwd, t->zero_bias, t->dxcol);
                HIPCHK(h, gemm(d));
                HIPCHK(h, launch_col2im(t->dxcol, a.rows, din, a.M, a.taps, a.KW, a.cin, a.in_cstride, h->stream));
            }
            if (ndeferred > 0) {
                dgroup.groups = ndeferred;
                HIPCHK(h, gemm(dgroup));
            }
        } else if (op.kind == Op::POOL) {
            const void* pool_out = op.conv.g[0].out;
            float* dpool = grad_buffer(h, pool_out, act_elems_of(h, pool_out, es));
            HIPCHK(h, launch_stem_pool_backward(h->stem_out, dpool, t->stem_dz, c.batch, h->sh, h->sw, h->ph, h->pw, h->pw + 2,
                                                (h->ph + 2) * (h->pw + 2), h->stream, f32));
        } else {                                     // STEM: weight gradient only (nothing upstream of the image)
            TrainConv& tc = t->convs[t->index.at("conv1")];
            const int M = c.batch * h->sh * h->sw;
            WgradSlot slot;
            BODCHK(train_wgrad_slot(h, tc, M, &slot));
            BODCHK(train_wgrad(h, tc, slot, t->stem_dz, f32 ? (const void*)t->cur_images : (const void*)t->img_bf16, t->stem_rows, 3, M));
        }
    }
    // join: every weight gradient is in the arena before the optimizer reads it
    for (int k = 0; k < TrainState::WS; ++k)
        if (t->pending[k]) {
            if (t->slot_job[k]) t->worker.wait_for(t->slot_job[k]);
            HIPCHK(h, hipStreamWaitEvent(h->stream, t->ev_done[k], 0));
            t->pending[k] = false; t->slot_job[k] = 0;
        }
    if (const int we = t->worker.err.exchange(0)) return h->fail(BOD_ERR_HIP, "training: weight-gradient stream: %s", hipGetErrorString((hipError_t)we));
    return BOD_OK;
}

}  // namespace

namespace {
// tf.clip_by_global_norm(5.0) + keras Adam(epsilon = 1e-2) over the whole arena; scalars[1] holds the squared gradient norm
// host side of an update: advance the step counter and put this step's bias-corrected rate where the kernel reads it
bod_status train_set_rate(bod_context* h, float learning_rate) {
    TrainState* t = h->train;
    t->step += 1;
    const double b1 = 0.9, b2 = 0.999;
    const float lr_t = (float)(learning_rate * std::sqrt(1.0 - std::pow(b2, (double)t->step)) / (1.0 - std::pow(b1, (double)t->step)));
    HIPCHK(h, hipMemcpyAsync(t->dyn + 3, &lr_t, 4, hipMemcpyHostToDevice, h->stream));
    return BOD_OK;
}
bod_status train_apply(bod_context* h) {
    TrainState* t = h->train;
    HIPCHK(h, launch_adam(t->master, t->grad, t->adam_m, t->adam_v, (long)t->arena_n, t->scalars + 1, 5.0f, reinterpret_cast<const float*>(t->dyn + 3),
                          0.9f, 0.999f, 1e-2f, h->stream));
    return BOD_OK;
}
}  // namespace

namespace {
// Everything of a step that runs on the device, in stream order (capturable: no allocation, no host synchronisation; the
// dropout seed / image id and the learning rate are read from t->dyn).
bod_status train_enqueue(bod_context* h, const float* dev, uint64_t seed, uint32_t first_image_id, int32_t reg_kind, float label_smoothing,
                         float w_cls, float w_reg, float l2_rate, int32_t apply_update) {
    TrainState* t = h->train;
    const bod_config& c = h->cfg;
    t->l2_rate = l2_rate;
    // ---- forward with the current master weights
    BODCHK(train_fold_all(h));
    BODCHK(run_forward(h, dev, seed, first_image_id));
    // ---- loss and its gradient with respect to the raw head outputs
    LossArgs la{};
    la.B = c.batch; la.A = h->A; la.C = c.num_classes; la.do_cls = 1; la.reg_kind = reg_kind; la.label_smoothing = label_smoothing;
    la.cls = h->raw[0]; la.cls_t = t->cls_t; la.box = h->raw[1]; la.box_t = t->box_t; la.cov = h->raw[2]; la.anchors = h->d_anchors;
    la.pos = t->pos; la.neg = t->neg;
    EnergyArgs ea{};
    if (reg_kind == 5) {
        // the energy score's normals are keyed like the dropout masks: a recorded step reads this step's seed and image base
        // from t->dyn, the fp32 verification handle (never recorded) takes them by argument like its convolutions
        ea.B = c.batch; ea.A = h->A; ea.M = h->energy_samples;
        ea.box = la.box; ea.box_t = la.box_t; ea.cov = la.cov; ea.anchors = la.anchors;
        ea.dyn = t->f32 ? nullptr : t->dyn;
        ea.seed_lo = (uint32_t)seed; ea.seed_hi = (uint32_t)(seed >> 32); ea.first_image_id = first_image_id;
        ea.id_stride = 1;                                           // (a step's frames are consecutive images, as for dropout)
        ea.list = h->energy_list; ea.row_term = h->energy_term; la.row_term = h->energy_term;
        HIPCHK(h, launch_loss_compact(t->pos, (long long)c.batch * h->A, h->energy_list, h->stream));
        HIPCHK(h, launch_energy_forward(ea, h->stream));
    }
    HIPCHK(h, launch_loss(la, t->loss_partial, t->loss_blocks, h->stream));
    HIPCHK(h, launch_loss_reduce(t->loss_partial, t->loss_blocks, t->loss_sums, h->stream));
    HIPCHK(h, hipMemsetAsync(t->act_grad_arena, 0, t->act_grad_n * 4, h->stream));
    for (auto& kv : t->grad_of)                                  // (buffers created outside the arena, if any)
        if (kv.second < t->act_grad_arena || kv.second >= t->act_grad_arena + t->act_grad_n)
            HIPCHK(h, hipMemsetAsync(kv.second, 0, t->grad_elems[kv.first] * 4, h->stream));
    HIPCHK(h, hipMemsetAsync(t->grad, 0, t->arena_n * 4, h->stream));
    HIPCHK(h, hipMemsetAsync(t->scalars, 0, 16, h->stream));
    float* dcls = grad_buffer(h, h->raw[0], act_elems_of(h, h->raw[0], 4));
    float* dbox = grad_buffer(h, h->raw[1], act_elems_of(h, h->raw[1], 4));
    float* dcov = c.has_covar_head ? grad_buffer(h, h->raw[2], act_elems_of(h, h->raw[2], 4)) : nullptr;
    if (!dcls || !dbox) return h->fail(BOD_ERR_OOM, "training: gradient buffer");
    HIPCHK(h, launch_loss_backward(la, t->loss_sums, w_cls, w_reg, dcls, dbox, reg_kind >= 2 ? dcov : nullptr, h->stream));
    if (reg_kind == 5) HIPCHK(h, launch_energy_backward(ea, t->loss_sums, w_reg, dbox, dcov, h->stream));
    // ---- backward through the plan
    t->cur_images = dev;
    if (!t->f32) {
        const size_t npx = (size_t)c.batch * c.image_h * c.image_w * 3;
        HIPCHK(h, launch_f32_to_bf16(dev, t->img_bf16, (long)npx, h->stream));
    }
    BODCHK(train_backward(h));
    if (reg_kind >= 4 && !t->f32) {
        // The proper scoring rules' gradients reach the heads' output biases in fp32: the weight-gradient GEMM above read dZ from bf16
        // storage (2^-9 per element), so for these two kinds the bias rows it wrote are replaced by the column sums of dbox / dcov
        // (train_backward has joined the weight-gradient streams).  Kinds 1-3 keep the gradients they had.
        const long long rows = (long long)c.batch * h->A / c.anchors_per_location;
        const struct { const char* layer; const float* g; int width; } heads[2] = {{"pyramid_regression", dbox, 4}, {"pyramid_cov", dcov, 10}};
        for (const auto& hd : heads) {
            auto it = t->index.find(hd.layer);
            if (it == t->index.end() || !hd.g) return h->fail(BOD_ERR_INVALID_ARG, "training: reg_kind %d needs the output convolution '%s'", reg_kind, hd.layer);
            const TrainConv& tc = t->convs[it->second];
            if (!tc.bias.present || tc.cout != c.anchors_per_location * hd.width)
                return h->fail(BOD_ERR_INVALID_ARG, "training: '%s' has no bias of %d channels", hd.layer, c.anchors_per_location * hd.width);
            HIPCHK(h, launch_head_bias_grad(hd.g, rows, tc.cout, t->grad + tc.bias.off, h->stream));
        }
    }
    // ---- global-norm clip, Adam (the L2 terms were added by the weight-gradient pass)
    HIPCHK(h, launch_sumsq(t->grad, (long)t->arena_n, t->scalars + 1, t->sumsq_partial, h->stream));
    if (apply_update) BODCHK(train_apply(h));
    return BOD_OK;
}

// RetinaNetModel.call(x, 'training') (retinanet_model.py:113-147): the training-mode forward alone -- dropout on at one
// sample, batch-norm frozen, current master weights -- through bod_forward on a training handle
bod_status train_forward_only(bod_context* h, const float* dev, uint64_t seed, uint32_t first_image_id) {
    TrainState* t = h->train;
    const uint32_t rng3[3] = {(uint32_t)seed, (uint32_t)(seed >> 32), first_image_id};
    HIPCHK(h, hipMemcpyAsync(t->dyn, rng3, 12, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));          // rng3 lives on this stack frame
    BODCHK(train_fold_all(h));
    BODCHK(run_forward(h, dev, seed, first_image_id));
    return mark_images_consumed(h);
}
}  // namespace

bod_status bod_train_gradients(bod_handle h, void** device_ptr, int64_t* count) {
    if (!h || !device_ptr || !count) return BOD_ERR_INVALID_ARG;
    if (!h->train) return h->fail(BOD_ERR_NOT_READY, "not a training handle");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));          // the caller's collective runs on its own stream
    *device_ptr = h->train->grad; *count = (int64_t)h->train->arena_n;
    return BOD_OK;
}

bod_status bod_train_apply(bod_handle h, float learning_rate, double* grad_norm) {
    if (!h) return BOD_ERR_INVALID_ARG;
    if (!h->train) return h->fail(BOD_ERR_NOT_READY, "not a training handle");
    TrainState* t = h->train;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemsetAsync(t->scalars + 1, 0, 4, h->stream));
    HIPCHK(h, launch_sumsq(t->grad, (long)t->arena_n, t->scalars + 1, t->sumsq_partial, h->stream));
    BODCHK(train_set_rate(h, learning_rate));
    BODCHK(train_apply(h));
    if (grad_norm) {
        float v = 0.f;
        HIPCHK(h, hipMemcpyAsync(&v, t->scalars + 1, 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        *grad_norm = std::sqrt((double)v);
    }
    return BOD_OK;
}

namespace {
// A step from "stage the frames" onward, with the targets already in t->cls_t / box_t / pos / neg (copied there by
// bod_train_step, assigned there by bod_train_step_boxes): eager, two-thread or hipGraph form, then the out6 read-back.
bod_status train_run_step(bod_context* h, const float* images, int32_t on_device, uint64_t seed, uint32_t first_image_id, int32_t reg_kind,
                          float label_smoothing, float w_cls, float w_reg, float l2_rate, float learning_rate, int32_t apply_update,
                          double* out6) {
    TrainState* t = h->train;
    const bod_config& c = h->cfg;
    const float* dev = nullptr;
    BODCHK(stage_images(h, images, on_device, &dev));
    {
        const uint32_t rng3[3] = {(uint32_t)seed, (uint32_t)(seed >> 32), first_image_id};
        HIPCHK(h, hipMemcpyAsync(t->dyn, rng3, 12, hipMemcpyHostToDevice, h->stream));
    }
    if (apply_update) BODCHK(train_set_rate(h, learning_rate));
    // ---- the device work of the step: replayed from a hipGraph once the same configuration has run eagerly
    if (reg_kind == 5) BODCHK(energy_buffers(h));                 // (before any capture: allocates on the first kind-5 step)
    char key[176];
    snprintf(key, sizeof key, "%p|%d|%a|%a|%a|%a|%d|%d", (const void*)dev, reg_kind, label_smoothing, w_cls, w_reg, l2_rate, apply_update,
             reg_kind == 5 ? h->energy_samples : 0);                // the sample count is baked into a recorded step
    // opt-in (BOD_TRAIN_GRAPH=1): measured on MI355X the replay frees the host (11 ms of enqueue per step at a minibatch of
    // three) but is not faster than the eager two-stream step -- the step is bound by its ~1 000 dependent small kernels
    const char* genv = getenv("BOD_TRAIN_GRAPH");
    const bool graphs_enabled = genv && atoi(genv) != 0;
    if (t->graph && t->graph_key == key) {
        HIPCHK(h, hipGraphLaunch(t->graph, h->stream));
    } else if (graphs_enabled && !t->graph_off && t->graph_key == key && t->eager_runs >= 1) {
        if (t->graph) { hipGraphExecDestroy(t->graph); t->graph = nullptr; }
        hipGraph_t g = nullptr;
        HIPCHK(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
        t->use_worker = false;                                  // the capture is thread-local
        const bod_status es = train_enqueue(h, dev, seed, first_image_id, reg_kind, label_smoothing, w_cls, w_reg, l2_rate, apply_update);
        const hipError_t ce = hipStreamEndCapture(h->stream, &g);
        if (es != BOD_OK || ce != hipSuccess || !g || hipGraphInstantiate(&t->graph, g, nullptr, nullptr, 0) != hipSuccess) {
            if (g) hipGraphDestroy(g);
            t->graph = nullptr; t->graph_off = true;              // this runtime cannot record the step: stay eager
            (void)hipGetLastError();
            BODCHK(train_enqueue(h, dev, seed, first_image_id, reg_kind, label_smoothing, w_cls, w_reg, l2_rate, apply_update));
        } else {
            hipGraphDestroy(g);
            HIPCHK(h, hipGraphLaunch(t->graph, h->stream));
        }
    } else {
        if (t->graph_key != key) { t->graph_key = key; t->eager_runs = 0; if (t->graph) { hipGraphExecDestroy(t->graph); t->graph = nullptr; } }
        // the first step of a configuration runs on one thread (it sets per-kernel attributes and allocates lazily);
        // afterwards BOD_TRAIN_THREADS=2 gives the weight-gradient stream its own enqueue thread.  Opt-in: measured on
        // MI355X it changes nothing (10.4 / 17.1 ms with either setting) -- the step is bound by the main stream's
        // kernels (15.5 ms busy of a 17.1 ms step at a minibatch of 8), not by the host
        const char* tenv = getenv("BOD_TRAIN_THREADS");
        const bool two_threads = tenv && atoi(tenv) == 2;
        t->use_worker = two_threads && t->eager_runs >= 1;
        if (t->use_worker && !t->worker.th.joinable()) t->worker.start(c.device);
        BODCHK(train_enqueue(h, dev, seed, first_image_id, reg_kind, label_smoothing, w_cls, w_reg, l2_rate, apply_update));
        t->eager_runs += 1;
    }
    // The frames are read by the stem forward, by the bf16 copy for the stem's weight gradient and by that weight-gradient pass
    // (whose stream the main stream has joined by now): only here may the copy stream refill the buffer (bod_upload_frames_u8_async
    // waits on this event).  Recorded outside the capture / replay, so it covers the eager and the graph form alike.
    BODCHK(mark_images_consumed(h));
    if (out6) {
        float sums[4], sc[4];
        HIPCHK(h, hipMemcpyAsync(sums, t->loss_sums, 16, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(sc, t->scalars, 16, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        const double np = std::max((double)sums[3], 1.0);
        out6[1] = w_cls * sums[0] / np;                                   // classification loss (weighted, like loss_dict['cls_loss'])
        out6[2] = sums[1] / np;                                           // regression (compute) term
        out6[3] = sums[2] / np;                                           // covariance regulariser
        out6[4] = sc[0];                                                  // L2 regularisation loss
        out6[0] = out6[1] + w_reg * (out6[2] + out6[3]) + out6[4];        // total_loss (run_training.py:226-236)
        out6[5] = std::sqrt((double)sc[1]);                               // global gradient norm before clipping
    }
    return BOD_OK;
}

bod_status train_step_check(bod_context* h, const char* who, int32_t reg_kind) {
    if (!h->train || !h->weights_ready) return h->fail(BOD_ERR_NOT_READY, "%s needs a handle created with training = 1 and finalized weights", who);
    if (!h->anchors_ready) return h->fail(BOD_ERR_NOT_READY, "bod_set_anchors has not been called");
    if (reg_kind < 1 || reg_kind > 5 || (reg_kind >= 2 && !h->cfg.has_covar_head)) return h->fail(BOD_ERR_INVALID_ARG, "%s: reg_kind %d", who, reg_kind);
    return BOD_OK;
}
}  // namespace

bod_status bod_train_step(bod_handle h, const float* images, int32_t on_device, const float* cls_targets, const float* box_targets,
                          const uint8_t* positive_mask, const uint8_t* negative_mask, uint64_t seed, uint32_t first_image_id,
                          int32_t reg_kind, float label_smoothing, float w_cls, float w_reg, float l2_rate, float learning_rate,
                          int32_t apply_update, double* out6) {
    if (!h || !cls_targets || !box_targets || !positive_mask || !negative_mask) return BOD_ERR_INVALID_ARG;
    BODCHK(train_step_check(h, "bod_train_step", reg_kind));
    TrainState* t = h->train;
    const bod_config& c = h->cfg;
    HIPCHK(h, hipSetDevice(c.device));
    const size_t BA = (size_t)c.batch * h->A;
    HIPCHK(h, hipMemcpyAsync(t->cls_t, cls_targets, BA * c.num_classes * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(t->box_t, box_targets, BA * 16, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(t->pos, positive_mask, BA, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(t->neg, negative_mask, BA, hipMemcpyHostToDevice, h->stream));
    return train_run_step(h, images, on_device, seed, first_image_id, reg_kind, label_smoothing, w_cls, w_reg, l2_rate, learning_rate, apply_update,
                          out6);
}

bod_status bod_train_step_boxes(bod_handle h, const float* images, int32_t on_device, const int32_t* num_gt, const float* gt_boxes_vuvu,
                                const float* gt_classes, float min_positive_iou, float max_negative_iou, uint64_t seed,
                                uint32_t first_image_id, int32_t reg_kind, float label_smoothing, float w_cls, float w_reg, float l2_rate,
                                float learning_rate, int32_t apply_update, double* out6) {
    if (!h || !num_gt || !gt_boxes_vuvu || !gt_classes) return BOD_ERR_INVALID_ARG;
    BODCHK(train_step_check(h, "bod_train_step_boxes", reg_kind));
    TrainState* t = h->train;
    const bod_config& c = h->cfg;
    for (int b = 0; b < c.batch; ++b)
        if (num_gt[b] < 1)
            return h->fail(BOD_ERR_INVALID_ARG, "bod_train_step_boxes: frame %d has %d ground-truth rows (at least the placeholder row is required)",
                           b, num_gt[b]);
    HIPCHK(h, hipSetDevice(c.device));
    // ---- the few GT rows go up in one copy; the kernel then writes the buffers bod_train_step fills by four copies
    if (!t->gt_ev) HIPCHK(h, hipEventCreateWithFlags(&t->gt_ev, hipEventDisableTiming));
    if (t->gt_pending) { HIPCHK(h, hipEventSynchronize(t->gt_ev)); t->gt_pending = false; }      // the last upload has left gt_host
    pack_gt(c.batch, num_gt, gt_boxes_vuvu, gt_classes, c.num_classes, &t->gt_host);
    const size_t bytes = t->gt_host.bytes.size();
    if (bytes > t->gt_cap) {
        if (t->gt_dev) { HIPCHK(h, hipStreamSynchronize(h->stream)); hipFree(t->gt_dev); t->gt_dev = nullptr; t->gt_cap = 0; }
        const size_t cap = std::max<size_t>(2 * bytes, 4096);
        if (hipMalloc(reinterpret_cast<void**>(&t->gt_dev), cap) != hipSuccess)
            return h->fail(BOD_ERR_OOM, "bod_train_step_boxes: %zu bytes for the ground truth", cap);
        t->gt_cap = cap;
    }
    HIPCHK(h, hipMemcpyAsync(t->gt_dev, t->gt_host.bytes.data(), bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(t->gt_ev, h->stream));
    t->gt_pending = true;
    TargetArgs ta{};
    ta.A = h->A; ta.B = c.batch; ta.C = c.num_classes; ta.min_positive_iou = min_positive_iou; ta.max_negative_iou = max_negative_iou;
    ta.anchors = h->d_anchors; ta.gt_off = reinterpret_cast<const int32_t*>(t->gt_dev);
    ta.gt_boxes = reinterpret_cast<const float*>(t->gt_dev + t->gt_host.box_off);
    ta.gt_classes = reinterpret_cast<const float*>(t->gt_dev + t->gt_host.cls_off);
    ta.cls_t = t->cls_t; ta.box_t = t->box_t; ta.pos = t->pos; ta.neg = t->neg;
    HIPCHK(h, launch_anchor_targets(ta, h->stream));
    return train_run_step(h, images, on_device, seed, first_image_id, reg_kind, label_smoothing, w_cls, w_reg, l2_rate, learning_rate, apply_update,
                          out6);
}

bod_status bod_train_get_targets(bod_handle h, float* cls_targets, float* box_targets, uint8_t* positive_mask, uint8_t* negative_mask) {
    if (!h || !cls_targets || !box_targets || !positive_mask || !negative_mask) return BOD_ERR_INVALID_ARG;
    if (!h->train) return h->fail(BOD_ERR_NOT_READY, "not a training handle");
    TrainState* t = h->train;
    const size_t BA = (size_t)h->cfg.batch * h->A;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemcpyAsync(cls_targets, t->cls_t, BA * h->cfg.num_classes * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(box_targets, t->box_t, BA * 16, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(positive_mask, t->pos, BA, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(negative_mask, t->neg, BA, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BOD_OK;
}

bod_status bod_train_get(bod_handle h, const char* layer, int32_t kind, int32_t what, float* out, int64_t n) {
    if (!h || !layer || !out) return BOD_ERR_INVALID_ARG;
    if (!h->train) return h->fail(BOD_ERR_NOT_READY, "not a training handle");
    TrainState* t = h->train;
    auto it = t->index.find(layer);
    if (it == t->index.end()) {
        // batch-norm layers are addressed by their own name (kind 2 = gamma, 3 = beta)
        for (size_t i = 0; i < t->convs.size(); ++i) if (t->convs[i].bn == layer) { it = t->index.find(t->convs[i].name); break; }
        if (it == t->index.end()) return h->fail(BOD_ERR_INVALID_ARG, "bod_train_get: unknown layer '%s'", layer);
    }
    const TrainConv& tc = t->convs[it->second];
    const ParamRef* r = kind == 0 ? &tc.kernel : kind == 1 ? &tc.bias : kind == 2 ? &tc.gamma : kind == 3 ? &tc.beta : nullptr;
    if (!r || !r->present || (int64_t)r->n != n) return h->fail(BOD_ERR_INVALID_ARG, "bod_train_get('%s', kind %d): no such parameter of %lld elements", layer, kind, (long long)n);
    const float* src = (what == 0 ? t->master : what == 1 ? t->grad : what == 2 ? t->adam_m : t->adam_v) + r->off;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemcpyAsync(out, src, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BOD_OK;
}

bod_status bod_train_set(bod_handle h, const char* layer, int32_t kind, int32_t what, const float* data, int64_t n) {
    if (!h || !layer || !data) return BOD_ERR_INVALID_ARG;
    if (!h->train) return h->fail(BOD_ERR_NOT_READY, "not a training handle");
    if (what != 2 && what != 3) return h->fail(BOD_ERR_INVALID_ARG, "bod_train_set restores the Adam moments (what = 2 / 3); values are loaded with bod_load_weight");
    TrainState* t = h->train;
    auto it = t->index.find(layer);
    if (it == t->index.end()) {
        for (size_t i = 0; i < t->convs.size(); ++i) if (t->convs[i].bn == layer) { it = t->index.find(t->convs[i].name); break; }
        if (it == t->index.end()) return h->fail(BOD_ERR_INVALID_ARG, "bod_train_set: unknown layer '%s'", layer);
    }
    const TrainConv& tc = t->convs[it->second];
    const ParamRef* r = kind == 0 ? &tc.kernel : kind == 1 ? &tc.bias : kind == 2 ? &tc.gamma : kind == 3 ? &tc.beta : nullptr;
    if (!r || !r->present || (int64_t)r->n != n) return h->fail(BOD_ERR_INVALID_ARG, "bod_train_set('%s', kind %d): no such parameter of %lld elements", layer, kind, (long long)n);
    float* dst = (what == 2 ? t->adam_m : t->adam_v) + r->off;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemcpyAsync(dst, data, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BOD_OK;
}

bod_status bod_train_step_count(bod_handle h, int64_t* get, int64_t set) {
    if (!h) return BOD_ERR_INVALID_ARG;
    if (!h->train) return h->fail(BOD_ERR_NOT_READY, "not a training handle");
    if (set >= 0) h->train->step = set;
    if (get) *get = (int64_t)h->train->step;
    return BOD_OK;
}

// ------------------------------------------------------------------------------------------------
// Stage entry points of the backward kernels that only the bf16 training handle launches (include/bayesod.h): a throw-away
// context (StageScope, engine.hip), host arrays in and out, the launchers called as train_backward / train_fold_all call them.  Every argument a kernel
// turns into an address is checked on the host first; nothing is launched on a bad one.
// ------------------------------------------------------------------------------------------------
namespace {
// host fp32 -> device buffer of the handle's element type (bf16: rounded like a stored activation); synchronises
bod_status stage_upload(bod_context* h, const float* src, size_t n, bool f32, void** dst) {
    char* d = nullptr;
    BODCHK(h->dalloc(&d, n * (f32 ? 4 : 2), false));
    std::vector<uint16_t> hb(f32 ? 0 : n);
    for (size_t i = 0; i < hb.size(); ++i) hb[i] = f2bf(src[i]);
    HIPCHK(h, hipMemcpyAsync(d, f32 ? (const void*)src : (const void*)hb.data(), n * (f32 ? 4 : 2), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *dst = d;
    return BOD_OK;
}
bod_status stage_download(bod_context* h, const void* src, size_t n, bool f32, float* dst) {
    std::vector<uint16_t> hb(f32 ? 0 : n);
    HIPCHK(h, hipMemcpyAsync(f32 ? (void*)dst : (void*)hb.data(), src, n * (f32 ? 4 : 2), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < hb.size(); ++i) dst[i] = bf2f(hb[i]);
    return BOD_OK;
}
}  // namespace

bod_status bod_stage_act_backward(int32_t device, int32_t precision, const float* dout, const float* out_act, const float* dout_relu,
                                  int64_t out_elems, const int32_t* out_off, const int32_t* res_off, int32_t M, int32_t cout,
                                  int32_t cout_pad, int32_t out_cstride, int32_t res_cstride, float scale, int32_t Kpad, float* dres,
                                  int64_t dres_elems, float* dz, float* dzp, float* dzt, int32_t* wrote_transpose) {
    StageScope sc;
    bod_context* h = sc.h;
    const bool f32 = precision == BOD_PRECISION_FP32;
    h->es = f32 ? 4 : 2;
    auto bad = [&](const char* what) { return sc.done(h->fail(BOD_ERR_INVALID_ARG, "bod_stage_act_backward: %s", what)); };
    if (precision != BOD_PRECISION_BF16 && !f32) return bad("precision must be BOD_PRECISION_BF16 or BOD_PRECISION_FP32");
    if (!dout || !out_off || !dz || !wrote_transpose) return bad("dout, out_off, dz and wrote_transpose must not be NULL");
    if (M < 1 || M > (1 << 22) || cout < 1 || cout > cout_pad || cout_pad > 4096) return bad("need 1 <= M <= 2^22 and 1 <= cout <= cout_pad <= 4096");
    if (out_cstride < cout || out_elems < 1 || out_elems > ((int64_t)1 << 28)) return bad("need out_cstride >= cout and 1 <= out_elems <= 2^28");
    if (Kpad < M || Kpad > (1 << 23)) return bad("Kpad must be at least M");
    if (dout_relu && !out_act) return bad("dout_relu needs the stored output");
    if (dres && (!res_off || res_cstride < cout || dres_elems < 1 || dres_elems > ((int64_t)1 << 28))) return bad("dres needs res_off, res_cstride >= cout and 1 <= dres_elems <= 2^28");
    for (int m = 0; m < M; ++m) {
        if (out_off[m] < 0 || (int64_t)out_off[m] * out_cstride + cout > out_elems) return bad("out_off outside the output buffer");
        if (dres && (res_off[m] < 0 || (int64_t)res_off[m] * res_cstride + cout > dres_elems)) return bad("res_off outside the residual gradient buffer");
    }
    if (const bod_status s = sc.open(device)) return sc.done(s);
    auto run = [&]() -> bod_status {
        const size_t es = h->es, n_out = (size_t)out_elems, n_dz = (size_t)M * cout_pad, n_dzt = (size_t)cout_pad * Kpad;
        float *d_dout = nullptr, *d_drelu = nullptr, *d_dres = nullptr;
        void *d_out = nullptr, *d_dzp = nullptr, *d_dzt = nullptr;
        char* d_dz = nullptr;
        BODCHK(stage_upload(h, dout, n_out, true, reinterpret_cast<void**>(&d_dout)));
        if (out_act) BODCHK(stage_upload(h, out_act, n_out, f32, &d_out));
        if (dout_relu) BODCHK(stage_upload(h, dout_relu, n_out, true, reinterpret_cast<void**>(&d_drelu)));
        if (dres) BODCHK(stage_upload(h, dres, (size_t)dres_elems, true, reinterpret_cast<void**>(&d_dres)));
        if (dzp) BODCHK(stage_upload(h, dzp, n_out, f32, &d_dzp));
        if (dzt) BODCHK(stage_upload(h, dzt, n_dzt, f32, &d_dzt));
        BODCHK(h->dalloc(&d_dz, n_dz * es, false));
        HIPCHK(h, hipMemsetAsync(d_dz, 0xFF, n_dz * es, h->stream));             // NaN in either type: an element the launch leaves out shows
        std::vector<RowEnt> rows((size_t)M);
        for (int m = 0; m < M; ++m) { RowEnt e{}; e.out_off = out_off[m]; e.res_off = dres ? res_off[m] : 0; rows[m] = e; }
        RowEnt* d_rows = nullptr;
        BODCHK(h->dalloc(&d_rows, rows.size(), false));
        HIPCHK(h, hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(RowEnt), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (dout_relu) HIPCHK(h, launch_relu_merge(d_drelu, d_out, d_dout, (long)n_out, h->stream, f32));
        ActBwdArgs ab{};
        ab.dout = d_dout; ab.out_bf16 = reinterpret_cast<const uint16_t*>(d_out);
        ab.rows = d_rows; ab.dz = reinterpret_cast<uint16_t*>(d_dz); ab.M = M; ab.cout = cout; ab.cout_pad = cout_pad;
        ab.out_cstride = out_cstride; ab.res_cstride = res_cstride;
        ab.scale = scale;
        ab.f32 = f32 ? 1 : 0;
        ab.dres = d_dres;
        ab.dzp = reinterpret_cast<uint16_t*>(d_dzp);
        ab.dzt = reinterpret_cast<uint16_t*>(d_dzt); ab.Kpad = Kpad;
        bool transposed = false;
        HIPCHK(h, launch_act_backward_gather(ab, h->stream, &transposed));
        if (dzt && !transposed) HIPCHK(h, launch_gather_transpose(d_dz, nullptr, d_dzt, M, Kpad, cout_pad, cout_pad, 1, 1, false, h->stream, f32));
        BODCHK(stage_download(h, d_dz, n_dz, f32, dz));
        if (dzp) BODCHK(stage_download(h, d_dzp, n_out, f32, dzp));
        if (dzt) BODCHK(stage_download(h, d_dzt, n_dzt, f32, dzt));
        if (dres) BODCHK(stage_download(h, d_dres, (size_t)dres_elems, true, dres));
        *wrote_transpose = transposed ? 1 : 0;
        return BOD_OK;
    };
    return sc.done(run());
}

bod_status bod_stage_conv_dgrad(int32_t device, int32_t route, const float* dz, const float* w, int32_t B, int32_t H, int32_t W,
                                int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t same_padding,
                                int32_t ksplit, int32_t groups, float* din, int32_t* info2) {
    StageScope sc;
    bod_context* h = sc.h;
    h->es = 2;
    auto bad = [&](const char* what) { return sc.done(h->fail(BOD_ERR_INVALID_ARG, "bod_stage_conv_dgrad: %s", what)); };
    if (!dz || !w || !din) return bad("dz, w and din must not be NULL");
    if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || KH < 1 || KW < 1 || KH > 3 || KW > 3 || stride < 1 || stride > 2) return bad("bad geometry");
    if (Cin % 64 != 0 || Cin > 4096 || Cout > 4096) return bad("Cin must be a multiple of 64 (the input-gradient launches' output tile); at most 4096 channels");
    if ((int64_t)B * (H + 2) * (W + 2) > (1 << 20)) return bad("at most 2^20 plane pixels");
    if (route < BOD_DGRAD_FLIP || route > BOD_DGRAD_COL2IM) return bad("route must be BOD_DGRAD_FLIP, BOD_DGRAD_ROWS or BOD_DGRAD_COL2IM");
    if (route == BOD_DGRAD_FLIP && !(KH == 3 && KW == 3 && stride == 1 && same_padding)) return bad("BOD_DGRAD_FLIP is the route of 3x3, stride 1, SAME layers");
    if (route == BOD_DGRAD_ROWS && !(KH == 1 && KW == 1)) return bad("BOD_DGRAD_ROWS is the route of 1x1 layers");
    if (groups < 1 || groups > 3 || (groups > 1 && route != BOD_DGRAD_FLIP)) return bad("groups: 1..3, more than one on BOD_DGRAD_FLIP only");
    const int cout_pad = (Cout + 63) / 64 * 64, taps = KH * KW;
    if (ksplit < 0 || ksplit > 64 || (ksplit > 1 && (cout_pad / 64) % ksplit != 0)) return bad("ksplit must divide the reduction's 64-channel chunks (cout_pad / 64)");
    int OH, OW, oy, ox;
    conv_out_geometry(H, W, KH, KW, stride, same_padding != 0, &OH, &OW, &oy, &ox);
    if (OH < 1 || OW < 1) return bad("empty output");
    // forward row table on the zero-bordered input plane (bod_stage_conv_wgrad's); BOD_DGRAD_FLIP: the output plane has the same geometry
    const int pitch = W + 2;
    const int64_t bstride = (int64_t)(H + 2) * (W + 2), npix = (int64_t)B * bstride;
    const int M = B * OH * OW;
    std::vector<RowEnt> rows = forward_row_table(B, OH, OW, stride, oy, ox, pitch, bstride);
    for (size_t r = 0; r < rows.size(); ++r) {
        const int b = (int)(r / ((size_t)OH * OW)), y = (int)(r % ((size_t)OH * OW)) / OW, xx = (int)(r % (size_t)OW);
        rows[r].out_off = route == BOD_DGRAD_FLIP ? (int32_t)(b * bstride + (int64_t)(y + 1) * pitch + (xx + 1)) : (int32_t)r;
        // every pixel a window touches lies on the plane of its own image
        const int y0 = y * stride + oy, x0 = xx * stride + ox;
        if (y0 < 0 || x0 < 0 || y0 + KH - 1 > H + 1 || x0 + KW - 1 > W + 1) return bad("a window leaves the bordered plane");
    }
    if (const bod_status s = sc.open(device)) return sc.done(s);
    auto run = [&]() -> bod_status {
        const size_t n_w = (size_t)taps * Cin * Cout, n_wp = (size_t)taps * Cin * cout_pad, n_dz = (size_t)M * Cout, n_din = (size_t)npix * Cin;
        RowEnt* d_rows = nullptr;
        BODCHK(h->dalloc(&d_rows, rows.size(), false));
        HIPCHK(h, hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(RowEnt), hipMemcpyHostToDevice, h->stream));
        float *d_zero = nullptr, *d_bscratch = nullptr;
        BODCHK(h->dalloc(&d_zero, (size_t)std::max(cout_pad, taps * Cin)));
        BODCHK(h->dalloc(&d_bscratch, (size_t)cout_pad));
        // the forward launch of the layer, as far as the input-gradient launches read it
        ConvArgs a{};
        a.rows = d_rows; a.M = M; a.taps = taps; a.KW = KW; a.cin = Cin; a.in_cstride = Cin;
        a.cout_pad = cout_pad; a.cout_valid = Cout; a.out_cstride = cout_pad; a.res_cstride = cout_pad; a.groups = groups;
        uint16_t* d_wp[3] = {nullptr, nullptr, nullptr};
        uint16_t* d_dz[3] = {nullptr, nullptr, nullptr};
        float* d_din[3] = {nullptr, nullptr, nullptr};
        for (int g = 0; g < groups; ++g) {
            void* d_w = nullptr;
            BODCHK(stage_upload(h, w + (size_t)g * n_w, n_w, true, &d_w));
            BODCHK(h->dalloc(&d_wp[g], n_wp));
            FoldArgs f{};
            f.kernel = reinterpret_cast<const float*>(d_w); f.eps = BN_EPS; f.taps = taps; f.cin = Cin; f.cout = Cout; f.cout_pad = cout_pad;
            if (route == BOD_DGRAD_FLIP) f.w_flip = d_wp[g]; else f.w_bwd = d_wp[g];
            f.b_fwd = d_bscratch;
            HIPCHK(h, launch_fold_pack(f, h->stream));
            // dZ: on the zero-bordered output plane (BOD_DGRAD_FLIP), else dense [M][cout_pad]
            const size_t n_dzb = (route == BOD_DGRAD_FLIP ? (size_t)npix : (size_t)M) * cout_pad;
            std::vector<uint16_t> hz(n_dzb, 0);
            for (int m = 0; m < M; ++m) {
                const size_t pix = route == BOD_DGRAD_FLIP ? (size_t)rows[m].out_off : (size_t)m;
                for (int c = 0; c < Cout; ++c) hz[pix * cout_pad + c] = f2bf(dz[(size_t)g * n_dz + (size_t)m * Cout + c]);
            }
            BODCHK(h->dalloc(&d_dz[g], n_dzb, false));
            HIPCHK(h, hipMemcpyAsync(d_dz[g], hz.data(), n_dzb * 2, hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            void* p = nullptr;
            BODCHK(stage_upload(h, din + (size_t)g * n_din, n_din, true, &p));
            d_din[g] = reinterpret_cast<float*>(p);
        }
        ConvArgs d{};
        float* d_dxcol = nullptr;
        if (route == BOD_DGRAD_FLIP) {
            d = dgrad_flip_args(a, d_dz[0], d_wp[0], d_zero, d_din[0]);
            for (int g = 1; g < groups; ++g) d.g[g] = dgrad_flip_args(a, d_dz[g], d_wp[g], d_zero, d_din[g]).g[0];
            d.groups = groups;                       // (train_backward: one grouped launch for groups that read different inputs)
        } else if (route == BOD_DGRAD_ROWS) {
            RowEnt* dr = nullptr;
            BODCHK(h->dalloc(&dr, (size_t)M, false));
            HIPCHK(h, launch_make_dgrad_rows(d_rows, dr, M, h->stream));
            d = dgrad_rows_args(a, dr, d_dz[0], d_wp[0], d_zero, d_din[0]);
        } else {
            std::vector<RowEnt> io((size_t)M);
            for (int m = 0; m < M; ++m) { RowEnt e{}; e.in_off = m; e.out_off = m; io[m] = e; }
            RowEnt* d_iota = nullptr;
            BODCHK(h->dalloc(&d_iota, io.size(), false));
            HIPCHK(h, hipMemcpyAsync(d_iota, io.data(), io.size() * sizeof(RowEnt), hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            BODCHK(h->dalloc(&d_dxcol, (size_t)M * taps * Cin));
            d = dgrad_xcol_args(a, d_iota, d_dz[0], d_wp[0], d_zero, d_dxcol);
        }
        // split-K as train_backward's `gemm` decides it, or as the caller forces it
        const int S = ksplit > 0 ? ksplit : dgrad_splits(d.M, d.cin, d.taps, d.cout_pad, d.groups);
        if (S > 1) {
            if ((d.cin / 64) % S != 0) return h->fail(BOD_ERR_INVALID_ARG, "bod_stage_conv_dgrad: ksplit %d does not divide %d chunks", S, d.cin / 64);
            d.ksplit = S;
            BODCHK(h->dalloc(&d.partial, (size_t)S * d.groups * d.M * d.cout_pad, false));
        }
        if (info2) { info2[0] = S; info2[1] = (S <= 1 && conv_igemm_uses_big_tile(d)) ? 1 : 0; }
        HIPCHK(h, launch_conv_igemm(d, h->stream));
        if (route == BOD_DGRAD_COL2IM) HIPCHK(h, launch_col2im(d_dxcol, a.rows, d_din[0], a.M, a.taps, a.KW, a.cin, a.in_cstride, h->stream));
        for (int g = 0; g < groups; ++g) BODCHK(stage_download(h, d_din[g], n_din, true, din + (size_t)g * n_din));
        return BOD_OK;
    };
    return sc.done(run());
}

bod_status bod_stage_stem_pool_backward(int32_t device, int32_t precision, const float* stem_out, const float* dpool, int64_t dpool_elems,
                                        int32_t B, int32_t ih, int32_t iw, float* dz) {
    StageScope sc;
    bod_context* h = sc.h;
    const bool f32 = precision == BOD_PRECISION_FP32;
    h->es = f32 ? 4 : 2;
    auto bad = [&](const char* what) { return sc.done(h->fail(BOD_ERR_INVALID_ARG, "bod_stage_stem_pool_backward: %s", what)); };
    if (precision != BOD_PRECISION_BF16 && !f32) return bad("precision must be BOD_PRECISION_BF16 or BOD_PRECISION_FP32");
    if (!stem_out || !dpool || !dz) return bad("stem_out, dpool and dz must not be NULL");
    if (B < 1 || ih < 1 || iw < 1 || (int64_t)B * ih * iw > (1 << 22)) return bad("need B, ih, iw >= 1 and at most 2^22 stem pixels");
    // the pooled plane as bod_create lays it out: ZeroPadding2D((1, 2)) + MaxPool 3x3 s2 VALID, one pixel of border
    const int oh = (ih + 2 - 3) / 2 + 1, ow = (iw + 4 - 3) / 2 + 1;
    const int pool_pitch = ow + 2, pool_plane = (oh + 2) * (ow + 2);
    if (dpool_elems != (int64_t)B * pool_plane * 64) return bad("dpool must hold B * (oh + 2) * (ow + 2) * 64 floats (oh = (ih - 1) / 2 + 1, ow = (iw + 1) / 2 + 1)");
    if (const bod_status s = sc.open(device)) return sc.done(s);
    auto run = [&]() -> bod_status {
        const size_t n = (size_t)B * ih * iw * 64;
        void *d_stem = nullptr, *d_dpool = nullptr;
        char* d_dz = nullptr;
        BODCHK(stage_upload(h, stem_out, n, f32, &d_stem));
        BODCHK(stage_upload(h, dpool, (size_t)dpool_elems, true, &d_dpool));
        BODCHK(h->dalloc(&d_dz, n * h->es, false));
        HIPCHK(h, hipMemsetAsync(d_dz, 0xFF, n * h->es, h->stream));
        HIPCHK(h, launch_stem_pool_backward(d_stem, reinterpret_cast<const float*>(d_dpool), d_dz, B, ih, iw, oh, ow, pool_pitch, pool_plane, h->stream, f32));
        return stage_download(h, d_dz, n, f32, dz);
    };
    return sc.done(run());
}

// ------------------------------------------------------------------------------------------------
// Stage entry points of the stem and stem-pool kernels (include/bayesod.h, DESIGN.md 9.14).  Output planes live between two
// guard regions, everything filled with the caller's sentinel: an element a kernel leaves out, and a store past either end, show.
// ------------------------------------------------------------------------------------------------
namespace {
constexpr size_t STAGE_GUARD = 4096;                    // guard elements on either side of a plane
struct GuardedPlane {
    char* base = nullptr;
    size_t n = 0, es = 0;
    char* plane() const { return base + STAGE_GUARD * es; }
};
bool stage_sentinel_ok(float v) { return std::isfinite(v) && bf2f(f2bf(v)) == v; }
bod_status guarded_alloc(bod_context* h, size_t n, bool f32, float sentinel, GuardedPlane* g) {
    g->n = n; g->es = f32 ? 4 : 2;
    const size_t total = n + 2 * STAGE_GUARD;
    BODCHK(h->dalloc(&g->base, total * g->es, false));
    std::vector<float> hf(f32 ? total : 0, sentinel);
    std::vector<uint16_t> hb(f32 ? 0 : total, f2bf(sentinel));
    HIPCHK(h, hipMemcpyAsync(g->base, f32 ? (const void*)hf.data() : (const void*)hb.data(), total * g->es, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BOD_OK;
}
// plane -> dst (may be NULL) as fp32; BOD_ERR_HIP when a guard element no longer holds the sentinel
bod_status guarded_download(bod_context* h, const GuardedPlane& g, float sentinel, const char* what, float* dst) {
    const size_t total = g.n + 2 * STAGE_GUARD;
    std::vector<char> hb(total * g.es);
    HIPCHK(h, hipMemcpyAsync(hb.data(), g.base, hb.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    auto at = [&](size_t i) {
        if (g.es == 4) { float f; std::memcpy(&f, &hb[i * 4], 4); return f; }
        uint16_t u; std::memcpy(&u, &hb[i * 2], 2); return bf2f(u);
    };
    for (size_t i = 0; i < STAGE_GUARD; ++i)
        if (at(i) != sentinel || at(STAGE_GUARD + g.n + i) != sentinel)
            return h->fail(BOD_ERR_HIP, "%s: a kernel wrote outside its plane (guard element %zu %s it)", what, i, at(i) != sentinel ? "before" : "after");
    if (dst) for (size_t i = 0; i < g.n; ++i) dst[i] = at(STAGE_GUARD + i);
    return BOD_OK;
}
}  // namespace

bod_status bod_stage_stem(int32_t device, int32_t form, int32_t precision, const float* images, int32_t B, int32_t H, int32_t W,
                          const float* w, const float* bias, int32_t misalign, int32_t n_cu, float sentinel, float* stem_out,
                          float* pooled, int32_t* form_ran) {
    StageScope sc;
    bod_context* h = sc.h;
    const bool f32 = precision == BOD_PRECISION_FP32, x3 = precision == BOD_PRECISION_BF16X3;
    h->es = f32 ? 4 : 2;
    auto bad = [&](const char* what) { return sc.done(h->fail(BOD_ERR_INVALID_ARG, "bod_stage_stem: %s", what)); };
    if (precision != BOD_PRECISION_BF16 && !f32 && !x3) return bad("precision must be BOD_PRECISION_BF16, BOD_PRECISION_FP32 or BOD_PRECISION_BF16X3");
    if (!images || !w || !bias || !form_ran) return bad("images, w, bias and form_ran must not be NULL");
    if (form < BOD_STEM_AUTO || form > BOD_STEM_FUSED_SPLIT) return bad("unknown form");
    if (B < 1 || H < 7 || W < 7 || (int64_t)B * H * W > (1 << 22)) return bad("need B >= 1, H, W >= 7 and at most 2^22 input pixels");
    if (!stage_sentinel_ok(sentinel)) return bad("the sentinel must be finite and exact in bf16");
    static const int form_precision[8] = {-1, BOD_PRECISION_FP32, BOD_PRECISION_BF16X3, BOD_PRECISION_BF16, BOD_PRECISION_BF16,
                                          BOD_PRECISION_BF16, BOD_PRECISION_BF16, BOD_PRECISION_BF16X3};
    if (form != BOD_STEM_AUTO && form_precision[form] != precision) return bad("this form does not run in this precision");
    // the stem / pool geometry of bod_create
    const int oh = (H - 7) / 2 + 1, ow = (W - 7) / 2 + 1;
    const int ph = (oh + 2 - 3) / 2 + 1, pw = (ow + 4 - 3) / 2 + 1;
    const int pool_pitch = pw + 2, pool_plane = (ph + 2) * (pw + 2);
    auto is_fused = [](int f) { return f == BOD_STEM_FUSED_8 || f == BOD_STEM_FUSED_4 || f == BOD_STEM_FUSED_SPLIT; };
    if ((form == BOD_STEM_ROW_POOL || is_fused(form)) && ((W & 3) != 0 || misalign))
        return bad("the row and fused kernels need W % 4 == 0 and a 16-byte aligned image");
    if (is_fused(form) && ow > 256) return bad("the fused kernels take stem rows of at most 256 pixels");
    if (const bod_status s = sc.open(device)) return sc.done(s);
    auto run = [&]() -> bod_status {
        const size_t n_img = (size_t)B * H * W * 3;
        float *d_imgbuf = nullptr, *d_w = nullptr, *d_b = nullptr;
        BODCHK(h->dalloc(&d_imgbuf, n_img + 4));
        const float* d_img = d_imgbuf + (misalign ? 1 : 0);
        if ((reinterpret_cast<uintptr_t>(d_img) & 15) != (misalign ? 4u : 0u)) return h->fail(BOD_ERR_HIP, "bod_stage_stem: device allocation is not 16-byte aligned");
        BODCHK(h->dalloc(&d_w, (size_t)147 * 64, false));
        BODCHK(h->dalloc(&d_b, (size_t)64, false));
        HIPCHK(h, hipMemcpyAsync(const_cast<float*>(d_img), images, n_img * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_w, w, (size_t)147 * 64 * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_b, bias, 64 * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        int f = form;
        if (f == BOD_STEM_AUTO) {                      // the forward pass's rule (Op::STEM) for an inference handle that is not traced
            const bool fused = !f32 && (x3 ? stem_split_fused_enabled() : true) && stem_pool_fused_applies(d_img, B, W, ow, n_cu);
            if (f32) f = BOD_STEM_F32_POOL_F32;
            else if (fused) f = x3 ? BOD_STEM_FUSED_SPLIT : (stem_pool_fused_form(0) == STEM_FUSED_8 ? BOD_STEM_FUSED_8 : BOD_STEM_FUSED_4);
            else if (x3) f = BOD_STEM_F32_POOL_SPLIT;
            else f = stem_conv_form(d_img, 0, W) == STEM_CONV_ROW ? BOD_STEM_ROW_POOL : BOD_STEM_SEG64_POOL;
        }
        // whatever chose the form: nothing is launched on a shape the kernel is not built for
        if ((f == BOD_STEM_ROW_POOL && !stem_conv_row_fits(d_img, W)) || (is_fused(f) && !stem_pool_fused_fits(d_img, W, ow)))
            return h->fail(BOD_ERR_INVALID_ARG, "bod_stage_stem: form %d does not fit this image (W %d, ow %d, misalign %d)", f, W, ow, misalign);
        const bool pairs = f == BOD_STEM_F32_POOL_SPLIT || f == BOD_STEM_FUSED_SPLIT;
        const bool stem_f32 = f == BOD_STEM_F32_POOL_F32 || f == BOD_STEM_F32_POOL_SPLIT;
        GuardedPlane gs, gp;
        BODCHK(guarded_alloc(h, (size_t)B * pool_plane * (pairs ? 128 : 64), f == BOD_STEM_F32_POOL_F32, sentinel, &gp));
        if (is_fused(f)) {
            const StemFusedForm ff = f == BOD_STEM_FUSED_SPLIT ? STEM_FUSED_SPLIT : f == BOD_STEM_FUSED_8 ? STEM_FUSED_8 : STEM_FUSED_4;
            HIPCHK(h, launch_stem_pool_fused_form(ff, d_img, d_w, d_b, gp.plane(), B, H, W, oh, ow, ph, pw, pool_pitch, pool_plane, h->stream));
        } else {
            BODCHK(guarded_alloc(h, (size_t)B * oh * ow * 64, stem_f32, sentinel, &gs));
            const StemConvForm cf = stem_f32 ? STEM_CONV_F32 : f == BOD_STEM_ROW_POOL ? STEM_CONV_ROW : STEM_CONV_SEG64;
            HIPCHK(h, launch_stem_conv_form(cf, d_img, d_w, d_b, gs.plane(), B, H, W, oh, ow, h->stream));
            HIPCHK(h, launch_stem_pool(gs.plane(), gp.plane(), f == BOD_STEM_F32_POOL_SPLIT ? 2 : (stem_f32 ? 1 : 0), B, oh, ow, ph, pw, pool_pitch,
                                       pool_plane, h->stream));
            BODCHK(guarded_download(h, gs, sentinel, "bod_stage_stem (stem plane)", stem_out));
        }
        BODCHK(guarded_download(h, gp, sentinel, "bod_stage_stem (pooled plane)", pooled));
        *form_ran = f;
        return BOD_OK;
    };
    return sc.done(run());
}

bod_status bod_stage_stem_pool(int32_t device, int32_t mode, const float* stem, int32_t B, int32_t ih, int32_t iw, float sentinel,
                               float* pooled) {
    StageScope sc;
    bod_context* h = sc.h;
    const bool in_f32 = mode != 0;
    h->es = in_f32 ? 4 : 2;
    auto bad = [&](const char* what) { return sc.done(h->fail(BOD_ERR_INVALID_ARG, "bod_stage_stem_pool: %s", what)); };
    if (mode < 0 || mode > 2) return bad("mode must be 0 (bf16 -> bf16), 1 (fp32 -> fp32) or 2 (fp32 -> pairs)");
    if (!stem || !pooled) return bad("stem and pooled must not be NULL");
    if (B < 1 || ih < 1 || iw < 1 || (int64_t)B * ih * iw > (1 << 22)) return bad("need B, ih, iw >= 1 and at most 2^22 stem pixels");
    if (!stage_sentinel_ok(sentinel)) return bad("the sentinel must be finite and exact in bf16");
    const int oh = (ih + 2 - 3) / 2 + 1, ow = (iw + 4 - 3) / 2 + 1;
    const int pool_pitch = ow + 2, pool_plane = (oh + 2) * (ow + 2);
    if (const bod_status s = sc.open(device)) return sc.done(s);
    auto run = [&]() -> bod_status {
        void* d_stem = nullptr;
        BODCHK(stage_upload(h, stem, (size_t)B * ih * iw * 64, in_f32, &d_stem));
        GuardedPlane gp;
        BODCHK(guarded_alloc(h, (size_t)B * pool_plane * (mode == 2 ? 128 : 64), mode == 1, sentinel, &gp));
        HIPCHK(h, launch_stem_pool(d_stem, gp.plane(), mode, B, ih, iw, oh, ow, pool_pitch, pool_plane, h->stream));
        return guarded_download(h, gp, sentinel, "bod_stage_stem_pool", pooled);
    };
    return sc.done(run());
}

bod_status bod_stage_fold_pack(int32_t device, int32_t count, const bod_fold_layer* layers) {
    StageScope sc;
    bod_context* h = sc.h;
    h->es = 2;
    auto bad = [&](const char* what) { return sc.done(h->fail(BOD_ERR_INVALID_ARG, "bod_stage_fold_pack: %s", what)); };
    if (!layers || count < 1 || count > 64) return bad("1..64 layers");
    for (int i = 0; i < count; ++i) {
        const bod_fold_layer& L = layers[i];
        if (!L.kernel || !L.b_fwd) return bad("kernel and b_fwd must not be NULL");
        if (L.taps < 1 || L.taps > 49 || L.cin < 1 || L.cin > 4096 || L.cout < 1 || L.cout > L.cout_pad || L.cout_pad > 4096) return bad("need 1 <= taps <= 49, 1 <= cin <= 4096, 1 <= cout <= cout_pad <= 4096");
        const int nbn = (L.gamma != nullptr) + (L.beta != nullptr) + (L.mean != nullptr) + (L.var != nullptr);
        if (nbn != 0 && nbn != 4) return bad("gamma, beta, mean and var come together or not at all");
    }
    if (const bod_status s = sc.open(device)) return sc.done(s);
    auto run = [&]() -> bod_status {
        std::vector<FoldArgs> all((size_t)count);
        long fold_max = 0;
        auto up = [&](const float* src, size_t n, const float** dst) -> bod_status {
            void* p = nullptr;
            if (src) BODCHK(stage_upload(h, src, n, true, &p));
            *dst = reinterpret_cast<const float*>(p);
            return BOD_OK;
        };
        for (int i = 0; i < count; ++i) {
            const bod_fold_layer& L = layers[i];
            FoldArgs& f = all[i];
            const size_t n_pack = (size_t)L.cout_pad * L.taps * L.cin;
            BODCHK(up(L.kernel, (size_t)L.taps * L.cin * L.cout, &f.kernel));
            BODCHK(up(L.bias, (size_t)L.cout, &f.bias));
            BODCHK(up(L.gamma, (size_t)L.cout, &f.gamma)); BODCHK(up(L.beta, (size_t)L.cout, &f.beta));
            BODCHK(up(L.mean, (size_t)L.cout, &f.mean)); BODCHK(up(L.var, (size_t)L.cout, &f.var));
            f.eps = BN_EPS; f.taps = L.taps; f.cin = L.cin; f.cout = L.cout; f.cout_pad = L.cout_pad; f.f32 = 0;
            // 0xFF fill (bf16 / fp32 NaN): an element the launch leaves out shows
            auto out16 = [&](uint16_t** p) -> bod_status { BODCHK(h->dalloc(p, n_pack, false)); HIPCHK(h, hipMemsetAsync(*p, 0xFF, n_pack * 2, h->stream)); return BOD_OK; };
            if (L.w_fwd) BODCHK(out16(&f.w_fwd));
            if (L.w_bwd) BODCHK(out16(&f.w_bwd));
            if (L.w_flip) BODCHK(out16(&f.w_flip));
            if (L.w_fwd32) { BODCHK(h->dalloc(&f.w_fwd32, (size_t)L.taps * L.cin * L.cout, false)); HIPCHK(h, hipMemsetAsync(f.w_fwd32, 0xFF, (size_t)L.taps * L.cin * L.cout * 4, h->stream)); }
            BODCHK(h->dalloc(&f.b_fwd, (size_t)L.cout_pad, false));
            HIPCHK(h, hipMemsetAsync(f.b_fwd, 0xFF, (size_t)L.cout_pad * 4, h->stream));
            fold_max = std::max(fold_max, (long)n_pack);
        }
        FoldArgs* d_desc = nullptr;
        BODCHK(h->dalloc(&d_desc, all.size(), false));
        HIPCHK(h, hipMemcpyAsync(d_desc, all.data(), all.size() * sizeof(FoldArgs), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, launch_fold_pack_all(d_desc, count, fold_max, h->stream));
        for (int i = 0; i < count; ++i) {
            const bod_fold_layer& L = layers[i];
            const FoldArgs& f = all[i];
            const size_t n_pack = (size_t)L.cout_pad * L.taps * L.cin;
            if (L.w_fwd) HIPCHK(h, hipMemcpyAsync(L.w_fwd, f.w_fwd, n_pack * 2, hipMemcpyDeviceToHost, h->stream));
            if (L.w_bwd) HIPCHK(h, hipMemcpyAsync(L.w_bwd, f.w_bwd, n_pack * 2, hipMemcpyDeviceToHost, h->stream));
            if (L.w_flip) HIPCHK(h, hipMemcpyAsync(L.w_flip, f.w_flip, n_pack * 2, hipMemcpyDeviceToHost, h->stream));
            if (L.w_fwd32) HIPCHK(h, hipMemcpyAsync(L.w_fwd32, f.w_fwd32, (size_t)L.taps * L.cin * L.cout * 4, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipMemcpyAsync(L.b_fwd, f.b_fwd, (size_t)L.cout_pad * 4, hipMemcpyDeviceToHost, h->stream));
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return BOD_OK;
    };
    return sc.done(run());
}

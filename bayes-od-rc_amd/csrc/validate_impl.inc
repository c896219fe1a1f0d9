// Validation from ground-truth boxes (run_validation.val_single_step, src/retina_net/experiments/run_validation.py:230-260, followed
// by validation_utils.post_process_predictions, :10-77) for `batch` frames; included at the end of engine.hip.  The forward's raw
// head outputs stay on the device: the anchor targets are assigned there (launch_anchor_targets, the kernel of bod_anchor_targets
// and bod_train_step_boxes), the loss terms are summed per frame (launch_loss_frames: the per-anchor arithmetic of bod_loss_forward,
// blockIdx.y = frame), and the selected candidates' class rows and corners are gathered into padded records, so the host takes a
// batch with one copy per array and one synchronise.
struct ValState {
    // dense targets of the batch: written by launch_anchor_targets, read by launch_loss_frames
    float* cls_t = nullptr; float* box_t = nullptr;       // [B,A,C], [B,A,4]
    uint8_t* pos = nullptr; uint8_t* neg = nullptr;       // [B,A]
    float* partial = nullptr;                             // [B][ceil(A / 256)][4] block partials
    double* sums = nullptr;                               // [B][4]
    // records: [B,K,C] class rows, [B,K,4] corners (y1, x1, y2, x2), [B] counts; K = nms_max_output_size
    float* det_scores = nullptr; float* det_corners = nullptr; int32_t* det_num = nullptr;
    // the batch's ground truth: packed host copy and its device buffer (grown on demand)
    PackedGt gt_host; char* gt_dev = nullptr; size_t gt_cap = 0;
    std::vector<void*> owned;
};

namespace {

void val_destroy(bod_context* h) {
    if (!h->val) return;
    for (void* p : h->val->owned) hipFree(p);
    if (h->val->gt_dev) hipFree(h->val->gt_dev);
    delete h->val;
    h->val = nullptr;
}

// The first validation call allocates the state: a handle that never validates holds none of it.
bod_status val_init(bod_context* h) {
    if (h->val) return BOD_OK;
    const bod_config& c = h->cfg;
    const size_t BA = (size_t)c.batch * h->A, BK = (size_t)c.batch * c.nms_max_output_size;
    const size_t nblocks = ((size_t)h->A + 255) / 256;
    std::unique_ptr<ValState> v(new ValState);
    bool ok = true;
    auto get = [&](auto** p, size_t n) {
        void* q = nullptr;
        const size_t bytes = std::max<size_t>(n * sizeof(**p), 256);
        if (!ok || hipMalloc(&q, bytes) != hipSuccess) { ok = false; return; }
        v->owned.push_back(q);
        h->device_bytes += (int64_t)bytes;
        *p = reinterpret_cast<std::remove_reference_t<decltype(*p)>>(q);
    };
    get(&v->cls_t, BA * c.num_classes); get(&v->box_t, BA * 4); get(&v->pos, BA); get(&v->neg, BA);
    get(&v->partial, (size_t)c.batch * nblocks * 4); get(&v->sums, (size_t)c.batch * 4);
    get(&v->det_scores, BK * c.num_classes); get(&v->det_corners, BK * 4); get(&v->det_num, (size_t)c.batch);
    if (!ok) {
        for (void* p : v->owned) hipFree(p);
        return h->fail(BOD_ERR_OOM, "validation buffers for %d frames of %d anchors", c.batch, h->A);
    }
    h->val = v.release();
    return BOD_OK;
}

// What the three entry points refuse (BOD_ERR_INVALID_ARG), then what they wait for (BOD_ERR_NOT_READY)
bod_status val_check(bod_context* h, const char* who, const int32_t* num_gt, int32_t reg_kind, bool need_forward) {
    const bod_config& c = h->cfg;
    if (c.training) return h->fail(BOD_ERR_INVALID_ARG, "%s: a training handle runs its forward with dropout on; validate on an inference handle", who);
    if (c.mc_samples != 1) return h->fail(BOD_ERR_INVALID_ARG, "%s: validation is one deterministic sample, this handle has mc_samples = %d", who, c.mc_samples);
    if (reg_kind < 0 || reg_kind > 5) return h->fail(BOD_ERR_INVALID_ARG, "%s: reg_kind %d", who, reg_kind);
    if (reg_kind >= 2 && !c.has_covar_head) return h->fail(BOD_ERR_INVALID_ARG, "%s: reg_kind %d needs the covariance head, this handle has none", who, reg_kind);
    if (c.num_classes != 4 && c.num_classes != 8)
        return h->fail(BOD_ERR_INVALID_ARG, "%s: the loss kernels support 4 or 8 classes (background included), this handle has %d", who, c.num_classes);
    for (int b = 0; b < c.batch; ++b)
        if (num_gt[b] < 1)
            return h->fail(BOD_ERR_INVALID_ARG, "%s: frame %d has %d ground-truth rows (at least the placeholder row is required)", who, b, num_gt[b]);
    if (!h->anchors_ready) return h->fail(BOD_ERR_NOT_READY, "bod_set_anchors has not been called");
    if (need_forward && !h->stage.forward) return h->fail(BOD_ERR_NOT_READY, "bod_forward / bod_set_raw has not run");
    return BOD_OK;
}

// Ground truth up in one copy, targets, per-frame sums -> ValState.sums; everything on the handle's stream, nothing waited for
bod_status val_losses_enqueue(bod_context* h, const int32_t* num_gt, const float* gt_boxes, const float* gt_classes, float min_positive_iou,
                              float max_negative_iou, int32_t do_cls, int32_t reg_kind, float label_smoothing) {
    BODCHK(materialise_raw(h));
    BODCHK(val_init(h));
    ValState* v = h->val;
    const bod_config& c = h->cfg;
    pack_gt(c.batch, num_gt, gt_boxes, gt_classes, c.num_classes, &v->gt_host);      // (every entry point ends with a synchronise: the last upload has left gt_host)
    const size_t bytes = v->gt_host.bytes.size();
    if (bytes > v->gt_cap) {
        if (v->gt_dev) { HIPCHK(h, hipStreamSynchronize(h->stream)); hipFree(v->gt_dev); v->gt_dev = nullptr; v->gt_cap = 0; }
        const size_t cap = std::max<size_t>(2 * bytes, 4096);
        if (hipMalloc(reinterpret_cast<void**>(&v->gt_dev), cap) != hipSuccess) return h->fail(BOD_ERR_OOM, "%zu bytes for the ground truth", cap);
        v->gt_cap = cap;
    }
    HIPCHK(h, hipMemcpyAsync(v->gt_dev, v->gt_host.bytes.data(), bytes, hipMemcpyHostToDevice, h->stream));
    TargetArgs ta{};
    ta.A = h->A; ta.B = c.batch; ta.C = c.num_classes; ta.min_positive_iou = min_positive_iou; ta.max_negative_iou = max_negative_iou;
    ta.anchors = h->d_anchors; ta.gt_off = reinterpret_cast<const int32_t*>(v->gt_dev);
    ta.gt_boxes = reinterpret_cast<const float*>(v->gt_dev + v->gt_host.box_off);
    ta.gt_classes = reinterpret_cast<const float*>(v->gt_dev + v->gt_host.cls_off);
    ta.cls_t = v->cls_t; ta.box_t = v->box_t; ta.pos = v->pos; ta.neg = v->neg;
    HIPCHK(h, launch_anchor_targets(ta, h->stream));
    LossArgs la{};
    la.B = c.batch; la.A = h->A; la.C = c.num_classes; la.do_cls = do_cls ? 1 : 0; la.reg_kind = reg_kind; la.label_smoothing = label_smoothing;
    la.cls = h->raw[0]; la.box = h->raw[1]; la.cov = h->raw[2];                      // [B,1,A,.]: MC sample 0 is the only one
    la.cls_t = v->cls_t; la.box_t = v->box_t; la.anchors = h->d_anchors; la.pos = v->pos; la.neg = v->neg;
    if (reg_kind == 5) {                                                             // per-row energy terms first (bod_set_loss_options keys them)
        BODCHK(energy_buffers(h));
        EnergyArgs ea{};
        ea.B = c.batch; ea.A = h->A; ea.M = h->energy_samples;
        ea.box = la.box; ea.box_t = la.box_t; ea.cov = la.cov; ea.anchors = la.anchors;
        ea.seed_lo = (uint32_t)h->loss_seed; ea.seed_hi = (uint32_t)(h->loss_seed >> 32); ea.first_image_id = h->loss_first_image_id;
        ea.id_stride = h->loss_id_stride;
        ea.list = h->energy_list; ea.row_term = h->energy_term; la.row_term = h->energy_term;
        HIPCHK(h, launch_loss_compact(v->pos, (long long)c.batch * h->A, h->energy_list, h->stream));
        HIPCHK(h, launch_energy_forward(ea, h->stream));
    }
    HIPCHK(h, launch_loss_frames(la, v->partial, h->stream));
    HIPCHK(h, launch_loss_frames_reduce(v->partial, c.batch, (h->A + 255) / 256, v->sums, h->stream));
    return BOD_OK;
}

bod_status val_gather_enqueue(bod_context* h) {
    BODCHK(val_init(h));
    ValState* v = h->val;
    const bod_config& c = h->cfg;
    ValGatherArgs ga{};
    ga.B = c.batch; ga.A = h->A; ga.C = c.num_classes; ga.max_out = c.nms_max_output_size;
    ga.num_kept = h->pb.num_kept; ga.selected = h->cur().nms_sel; ga.num_selected = h->cur().nms_nsel; ga.score = h->pb.score; ga.corners = h->pb.corners;
    ga.out_scores = v->det_scores; ga.out_corners = v->det_corners; ga.out_num = v->det_num;
    HIPCHK(h, launch_validation_gather(ga, h->stream));
    return BOD_OK;
}

bod_status val_copy_detections(bod_context* h, int32_t* num, float* scores, float* corners) {
    const size_t BK = (size_t)h->cfg.batch * h->cfg.nms_max_output_size;
    BODCHK(d2h(h, num, h->val->det_num, (size_t)h->cfg.batch));
    BODCHK(d2h(h, scores, h->val->det_scores, BK * h->cfg.num_classes));
    BODCHK(d2h(h, corners, h->val->det_corners, BK * 4));
    return BOD_OK;
}

}  // namespace

extern "C" {

bod_status bod_validation_losses_boxes(bod_handle h, const int32_t* num_gt, const float* gt_boxes_vuvu, const float* gt_classes,
                                       float min_positive_iou, float max_negative_iou, int32_t do_classification, int32_t reg_kind,
                                       float label_smoothing, double* sums4) {
    if (!h) return BOD_ERR_INVALID_ARG;
    if (!num_gt || !gt_boxes_vuvu || !gt_classes || !sums4) return h->fail(BOD_ERR_INVALID_ARG, "bod_validation_losses_boxes: a required array is NULL");
    BODCHK(join_overlap(h));
    BODCHK(val_check(h, "bod_validation_losses_boxes", num_gt, reg_kind, true));
    HIPCHK(h, hipSetDevice(h->cfg.device));
    BODCHK(val_losses_enqueue(h, num_gt, gt_boxes_vuvu, gt_classes, min_positive_iou, max_negative_iou, do_classification, reg_kind, label_smoothing));
    BODCHK(d2h(h, sums4, h->val->sums, (size_t)h->cfg.batch * 4));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BOD_OK;
}

bod_status bod_get_validation_detections_batch(bod_handle h, int32_t* num_detections, float* scores, float* corners) {
    if (!h) return BOD_ERR_INVALID_ARG;
    BODCHK(join_overlap(h));
    if (!h->stage.nms) return h->fail(BOD_ERR_NOT_READY, "bod_nms has not run");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    BODCHK(val_gather_enqueue(h));
    BODCHK(val_copy_detections(h, num_detections, scores, corners));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BOD_OK;
}

bod_status bod_validate_boxes(bod_handle h, const float* images, int32_t images_on_device, const int32_t* num_gt, const float* gt_boxes_vuvu,
                              const float* gt_classes, float min_positive_iou, float max_negative_iou, int32_t do_classification,
                              int32_t reg_kind, float label_smoothing, double* sums4, int32_t* num_detections, float* scores, float* corners) {
    if (!h) return BOD_ERR_INVALID_ARG;
    if (!num_gt || !gt_boxes_vuvu || !gt_classes || !sums4) return h->fail(BOD_ERR_INVALID_ARG, "bod_validate_boxes: a required array is NULL");
    BODCHK(join_overlap(h));
    BODCHK(val_check(h, "bod_validate_boxes", num_gt, reg_kind, false));
    if (!h->weights_ready) return h->fail(BOD_ERR_NOT_READY, "weights not finalized");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const float* dev = nullptr;
    BODCHK(stage_images(h, images, images_on_device, &dev));
    h->cur_images = dev;
    BODCHK(run_forward(h, dev, 0, 0));                                 // one deterministic sample: no dropout stream to key
    BODCHK(val_losses_enqueue(h, num_gt, gt_boxes_vuvu, gt_classes, min_positive_iou, max_negative_iou, do_classification, reg_kind, label_smoothing));
    BODCHK(run_validation_post(h));
    BODCHK(run_nms(h, h->stream));
    BODCHK(val_gather_enqueue(h));
    BODCHK(d2h(h, sums4, h->val->sums, (size_t)h->cfg.batch * 4));
    BODCHK(val_copy_detections(h, num_detections, scores, corners));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BOD_OK;
}

}  // extern "C"

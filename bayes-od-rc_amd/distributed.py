"""Image-sharded multi-GPU execution: one process per GPU, images are independent units
(the reference's loop is batch(1) with no cross-image state: run_inference.py:68,137), so the
only exchange is ONE gather of the final fixed-size detection records per step
(SURVEY.md section 8e).  ``torch.distributed`` is plumbing: backend "nccl" is RCCL over xGMI on
ROCm, "gloo" is used by the CPU tests.
"""
import numpy as np
import torch
import torch.distributed as dist


def shard_range(num_images, world_size, rank):
    """Contiguous split of [0, num_images) over ranks; the first (num_images % world) ranks get one more."""
    base, extra = divmod(num_images, world_size)
    start = rank * base + min(rank, extra)
    return start, start + base + (1 if rank < extra else 0)


RECORD_EXTRA = 1      # per-detection record = [valid, means 4, covs 16, scores C, counts C]
RECORD_PARTS = 48     # ... + the three covariance parts (epistemic, aleatoric, prior: 3 x 16) on covariance_parts handles
RECORD_CLASS_PARTS = 4    # ... + total, aleatoric, epistemic_mc, epistemic_spatial class entropy on class_parts handles (last)


def record_width(num_classes, cov_parts=False, class_parts=False):
    return RECORD_EXTRA + 4 + 16 + 2 * num_classes + (RECORD_PARTS if cov_parts else 0) + (RECORD_CLASS_PARTS if class_parts else 0)


def pack_records(num, scores, means, covs, counts, cov_parts=None, class_parts=None):
    """Padded per-image arrays -> one float32 tensor [B, K, 1+4+16+2C]; slot 0 flags valid rows.
    ``cov_parts`` [B,K,3,4,4] (or [B,K,48]): the wide row of a covariance_parts handle, the parts behind the counts.
    ``class_parts`` [B,K,4]: the row of a class_parts handle, the four entropies last.
    Works on torch tensors of any device (device-side pack before the RCCL gather)."""
    b, k, _ = scores.shape
    valid = (torch.arange(k, device=scores.device)[None, :] < num.to(scores.device)[:, None]).to(scores.dtype)
    cols = [valid[:, :, None], means.reshape(b, k, 4), covs.reshape(b, k, 16), scores, counts]
    if cov_parts is not None:
        cols.append(cov_parts.reshape(b, k, RECORD_PARTS))
    if class_parts is not None:
        cols.append(class_parts.reshape(b, k, RECORD_CLASS_PARTS))
    rec = torch.cat(cols, dim=2)
    return rec * valid[:, :, None]


def unpack_records(rec, num_classes):
    """[B,K,W] tensor/array -> list of (scores [k,C], means [k,4], covs [k,4,4], counts [k,C]) per image; rows of the wide
    form (W = 1+4+16+2C+48) give a further element, cov_parts [k,3,4,4]; rows of a class_parts handle (4 floats wider still) one
    more, class_parts [k,4] = total, aleatoric, epistemic_mc, epistemic_spatial."""
    rec = rec.detach().cpu().numpy() if isinstance(rec, torch.Tensor) else np.asarray(rec)
    out = []
    c = num_classes
    widths = {record_width(c, p, q): (p, q) for p in (False, True) for q in (False, True)}
    if rec.shape[-1] not in widths:
        raise ValueError("record rows of %d floats: expected one of %s for %d classes" % (rec.shape[-1], sorted(widths), c))
    wide, cls_parts = widths[rec.shape[-1]]
    w0 = 21 + 2 * c
    w1 = w0 + (RECORD_PARTS if wide else 0)
    for r in rec:
        k = int(r[:, 0].sum())
        r = r[:k]
        row = (r[:, 21:21 + c], r[:, 1:5], r[:, 5:21].reshape(k, 4, 4), r[:, 21 + c:21 + 2 * c])
        if wide:
            row += (r[:, w0:w1].reshape(k, 3, 4, 4),)
        if cls_parts:
            row += (r[:, w1:w1 + RECORD_CLASS_PARTS],)
        out.append(row)
    return out


def gather_records(rec, dst=0, group=None, always=False):
    """One collective per step: every rank contributes its [B,K,W] block; rank ``dst`` receives
    [world, B, K, W] (others None).  Latency-bound (~14 KB per image), never a ring all-reduce.
    ``always``: issue the collective even in a one-rank group (exercises the backend on a one-GPU box)."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    if world == 1 and not (always and dist.is_initialized()):
        return rec[None]
    rank = dist.get_rank(group)
    if rank == dst:
        bufs = [torch.empty_like(rec) for _ in range(world)]
        dist.gather(rec, gather_list=bufs, dst=dst, group=group)
        return torch.stack(bufs)
    dist.gather(rec, gather_list=None, dst=dst, group=group)
    return None


class DeviceArray(object):
    """Zero-copy view of a device buffer owned by the HIP library, for torch.as_tensor()."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr,
                                         "data": (int(ptr), False), "version": 2}


def torch_views(engine, slot=0):
    """torch tensors aliasing the engine's detection buffers (record slot 0/1) on its GPU."""
    p = engine.device_detection_pointers(slot)
    dev = torch.device("cuda", engine.cfg.device)
    views = {}
    for name, (ptr, shape) in p.items():
        views[name] = torch.as_tensor(DeviceArray(ptr, shape, "<i4" if name == "num" else "<f4"), device=dev)
    return views


# ---------------------------------------------------------------------------------------------------
# Second mode: MC-sample sharding for single-frame latency.  Every rank runs the
# backbone/FPN of the SAME frame(s) and n = N/world of the N dropout samples (its handle has
# mc_sample_base = rank*n, so the Philox streams are those of samples rank*n .. rank*n+n-1 of the N-sample
# ensemble); ONE all-gather of the raw head outputs rebuilds the [B,N,A,.] tensors RetinaNetModel.call
# returns on every rank, bit-identical to a single-GPU run, and the (cheap) Bayesian stages run replicated.
# The exchange carries 22 floats per anchor and sample ((C + 4 + 10) * 4 B * A * n per rank; 2.6 MB per
# sample at 512x512) over xGMI -- direct all-gather, no reduction, nothing to re-associate.
# ---------------------------------------------------------------------------------------------------
def sample_shard(total_samples, world_size, rank):
    """(first sample, count) of this rank; the ensemble must split evenly (fixed-size all-gather)."""
    if total_samples % world_size != 0:
        raise ValueError("mc_dropout_samples=%d is not divisible by the %d ranks of the sample-sharded mode"
                         % (total_samples, world_size))
    n = total_samples // world_size
    return rank * n, n


def raw_views(engine, mark_ready=False):
    """torch tensors aliasing the engine's raw head-output buffers: cls [B,N,A,C], box [B,N,A,4], cov [B,N,A,10]."""
    ptrs = engine.device_raw_pointers(mark_ready)
    dev = torch.device("cuda", engine.cfg.device)
    b, n, a = engine.B, engine.N, engine.A
    shapes = {"cls": (b, n, a, engine.Ccls), "box": (b, n, a, 4), "cov": (b, n, a, 10)}
    return {k: torch.as_tensor(DeviceArray(p, shapes[k], "<f4"), device=dev)
            for k, p in zip(("cls", "box", "cov"), ptrs) if p}


def all_gather_samples(local, full, group=None):
    """local [B,n,A,c] of every rank -> full [B,world*n,A,c] on every rank, rank r's samples at r*n.. .
    B == 1 gathers straight into ``full`` (zero copy); B > 1 goes through one staging tensor."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    b, n = local.shape[0], local.shape[1]
    if tuple(full.shape) != (b, world * n) + tuple(local.shape[2:]):
        raise ValueError("full %s does not hold %d x local %s" % (tuple(full.shape), world, tuple(local.shape)))
    if world == 1:
        full.copy_(local)
        return full
    local = local.contiguous()
    if local.is_cuda and dist.get_backend(group) == "gloo":
        # gloo moves device tensors through the host anyway; used by the one-GPU test of this mode (RCCL in production)
        host = torch.empty(tuple(full.shape), dtype=full.dtype)
        all_gather_samples(local.cpu(), host, group)
        full.copy_(host)
        return full
    if b == 1:
        dist.all_gather_into_tensor(full.view((world * n,) + tuple(local.shape[2:])),
                                    local.view((n,) + tuple(local.shape[2:])), group=group)
    else:
        tmp = torch.empty((world * b,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
        dist.all_gather_into_tensor(tmp, local, group=group)           # concatenation along dim 0: [world*B, n, A, c]
        full.view((b, world, n) + tuple(local.shape[2:])).copy_(tmp.view((world,) + tuple(local.shape)).transpose(0, 1))
    return full


class SampleShardedEngine(object):
    """Pair of handles for the sample-sharded mode on this rank's GPU: ``fwd`` computes this rank's n samples,
    ``post`` (no weights: raw buffers only) receives the gathered ensemble and runs posterior / soft-NMS /
    cluster-fuse.  ``make_config_kwargs`` are those of engine.make_config for the FULL ensemble.  ``merge_method``: how ``post``
    merges a cluster ('bayes', 'centre', 'mixture': ``Engine.set_merge_method``)."""

    def __init__(self, image_hw, weights, anchors, mc_samples, device=0, batch=1, group=None, merge_method='bayes', **make_config_kwargs):
        from .engine import Engine, make_config
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        base, n = sample_shard(mc_samples, self.world, self.rank)
        self.fwd = Engine(make_config(image_hw, batch=batch, mc_samples=n, device=device, mc_sample_base=base,
                                      mc_ensemble_size=mc_samples, **make_config_kwargs))
        self.fwd.load_weights(weights)
        self.post = Engine(make_config(image_hw, batch=batch, mc_samples=mc_samples, device=device, **make_config_kwargs))
        self.post.set_anchors(anchors)
        self.post.set_merge_method(merge_method)
        self._local = raw_views(self.fwd)
        self._full = raw_views(self.post, mark_ready=False)

    def infer(self, images, seed=0, first_image_id=0):
        """images: [B,H,W,3] float32 (the same on every rank).  Returns this rank's copy of the detections
        (list over images of (scores, means, covs, counts)); identical on all ranks."""
        self.fwd.forward(images, seed=seed, first_image_id=first_image_id)
        self.fwd.synchronize()                    # the collective runs on torch's stream, not the engine's
        for k, loc in self._local.items():
            all_gather_samples(loc, self._full[k], self.group)
        torch.cuda.synchronize(self._full["cls"].device)
        self.post.device_raw_pointers(mark_ready=True)
        self.post.posterior(seed=seed, first_image_id=first_image_id)
        self.post.nms()
        self.post.cluster_fuse()
        return [self.post.get_detections(i) for i in range(self.post.B)]


# ---------------------------------------------------------------------------------------------------
# Sample sharding on statistics (include/bayesod.h, mc_statistics): every rank reduces its n samples to the per-anchor
# statistics record -- 34 floats per anchor and image whatever n is, against 22 per anchor AND sample of the raw exchange --
# ONE all-gather moves the records, and every rank folds the W records in rank order with the merge kernel, so all ranks
# hold the same bits.  The fold re-associates the Welford sums (Chan's update): results agree with the single-handle run to
# fp32 round-off, not bit for bit -- SampleShardedEngine stays the bit-identical mode.
# ---------------------------------------------------------------------------------------------------
def stat_views(engine):
    """torch tensors aliasing a statistics handle's accumulator: cls [B,A,C], box [B,A,16], cov [B,A,10] (with the head), ent [B,A]
    (class_parts handles)."""
    ptrs = list(engine.stat_device_pointers())
    dev = torch.device("cuda", engine.cfg.device)
    b, a = engine.B, engine.A
    shapes = {"cls": (b, a, engine.Ccls), "box": (b, a, 16), "cov": (b, a, 10), "ent": (b, a)}
    ptrs.append(engine.stat_device_entropy_pointer() if engine.has_class_parts else None)
    return {k: torch.as_tensor(DeviceArray(p, shapes[k], "<f4"), device=dev)
            for k, p in zip(("cls", "box", "cov", "ent"), ptrs) if p}


def _stat_order(stats):
    return [k for k in ("cls", "box", "cov", "ent") if k in stats]


def all_gather_statistics(local, group=None):
    """local {'cls': [B,A,C], 'box': [B,A,16], 'cov': [B,A,10]} of every rank (torch, host or device) -> a list over the ranks of
    such dicts, on every rank, with ONE all-gather of the records laid end to end (cls, box, cov: every part starts on a
    16-byte boundary of its rank's own buffer, as ``bod_stat_merge`` wants)."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    names = _stat_order(local)
    pieces, off, offs = [], 0, {}
    for k in names:                               # ent starts on a 16-byte boundary: a pad in front of it where cov ends off one
        v = local[k].reshape(-1)
        if k == "ent" and off % 4:
            pieces.append(v.new_zeros(4 - off % 4))
            off += 4 - off % 4
        offs[k] = off
        pieces.append(v)
        off += v.numel()
    flat = torch.cat(pieces)
    if world == 1:
        bufs = [flat]
    elif flat.is_cuda and dist.get_backend(group) == "gloo":
        # gloo moves device tensors through the host anyway; used by the one-GPU test of this mode (RCCL in production)
        host = [torch.empty(flat.shape, dtype=flat.dtype) for _ in range(world)]
        dist.all_gather(host, flat.cpu(), group=group)
        bufs = [h.to(flat.device) for h in host]
    else:
        bufs = [torch.empty_like(flat) for _ in range(world)]
        dist.all_gather(bufs, flat, group=group)
    out = []
    for buf in bufs:
        d = {}
        for k in names:
            d[k] = buf[offs[k]:offs[k] + local[k].numel()].view(local[k].shape)
        out.append(d)
    return out


def merge_statistics_np(a, b, ka, kb, dtype=np.float64):
    """The merge of two statistics records on the host, as include/bayesod.h states it: a, b = (cls_sum [...,C], box_moments
    [...,16], cov_sum [...,10] or None) of ka and kb samples; returns the record of ka + kb samples in ``dtype`` (float64: the
    statement the tests compare the kernel with; float32: the kernel's own operation order).  Used by nothing in the product path.
    Records of four arrays (class_parts handles: ent_sum [...] last) give four: ent_sum = a + b whatever ka and kb are."""
    t = np.dtype(dtype).type
    if len(a) == 4 or len(b) == 4:
        if len(a) != len(b):
            raise ValueError("one record carries ent_sum, the other does not")
        ent = np.array(b[3], dtype=t) if int(ka) == 0 else np.asarray(a[3], dtype=t) + np.asarray(b[3], dtype=t)
        return merge_statistics_np(a[:3], b[:3], ka, kb, dtype) + (ent,)
    cls_a, box_a, cov_a = a
    cls_b, box_b, cov_b = b
    if int(ka) == 0:
        box = np.array(box_b, dtype=t)
        box[..., 14:] = 0
        return np.array(cls_b, dtype=t), box, (None if cov_b is None else np.array(cov_b, dtype=t))
    box_a, box_b = np.asarray(box_a, dtype=t), np.asarray(box_b, dtype=t)
    w = t(kb) / (t(ka) + t(kb))
    kw = t(ka) * w
    d = box_b[..., :4] - box_a[..., :4]
    box = np.zeros(box_a.shape, dtype=t)
    box[..., :4] = box_a[..., :4] + d * w
    k = 4
    for i in range(4):
        for j in range(i + 1):
            box[..., k] = (box_a[..., k] + box_b[..., k]) + (d[..., i] * d[..., j]) * kw
            k += 1
    cls = np.asarray(cls_a, dtype=t) + np.asarray(cls_b, dtype=t)
    cov = None if cov_a is None or cov_b is None else np.asarray(cov_a, dtype=t) + np.asarray(cov_b, dtype=t)
    return cls, box, cov


def mirror_anchor_index(level_hw, K):
    """partner[a] of every anchor a = off_l + (y * W_l + x) * K + k (the order of ``FpnAnchorGenerator.generate_all``): the anchor
    at column W_l - 1 - x of the same pyramid row.  ``level_hw``: [(H_l, W_l), ...] (``Engine.levels``).  An involution."""
    parts, off = [], 0
    for h, w in level_hw:
        h, w = int(h), int(w)
        idx = off + np.arange(h * w * K, dtype=np.int64).reshape(h, w, K)
        parts.append(idx[:, ::-1, :].reshape(-1))
        off += h * w * K
    return np.concatenate(parts)


_M2_FLIP = (5, 8, 11)           # box_moments[4 + k] for the stored M2 positions k = 1, 4, 7: (1,0), (2,1), (3,1)
_COV_FLIP = (8, 6, 2)           # the parameters model.fill_triangular_4 places at (1,0), (2,1), (3,1)


def mirror_statistics_np(cls_sum, box_moments, cov_sum, level_hw, K, image_w, ent_sum=None):
    """The mirror map of a statistics record on the host, as include/bayesod.h states it: the record [..., A, .] of a forward of
    the frames mirrored left-right -> the record of the frames as given.  Anchors move to their partner (``mirror_anchor_index``),
    the ``u`` mean becomes ``(image_w - 1) - u`` (one subtraction in the arrays' dtype), the co-moments with exactly one index
    equal to 1 and the covariance parameters 8, 6, 2 change sign; everything else is copied.  ``cov_sum`` may be None.
    ``ent_sum`` [..., A] (class_parts records): moved to the partner anchor, values unchanged; the result then has four arrays."""
    perm = mirror_anchor_index(level_hw, K)
    if np.shape(box_moments)[-2] != perm.shape[0] or np.shape(cls_sum)[-2] != perm.shape[0]:
        raise ValueError("the level table holds %d anchors, the record %d" % (perm.shape[0], np.shape(box_moments)[-2]))
    cls = np.array(np.asarray(cls_sum)[..., perm, :])
    box = np.array(np.asarray(box_moments)[..., perm, :])
    box[..., 1] = box.dtype.type(image_w - 1) - box[..., 1]
    for k in _M2_FLIP:
        box[..., k] = -box[..., k]
    cov = None
    if cov_sum is not None:
        cov = np.array(np.asarray(cov_sum)[..., perm, :])
        for k in _COV_FLIP:
            cov[..., k] = -cov[..., k]
    if ent_sum is not None:
        return cls, box, cov, np.array(np.asarray(ent_sum)[..., perm])
    return cls, box, cov


def anchors_mirror_symmetric(anchors, level_hw, K, image_w, min_level=3):
    """(ok, first_bad_level): is ``anchors[partner[a]]`` equal to ``(v, float(image_w) - u, h, w)`` of ``anchors[a]`` bit for bit,
    for every anchor?  This is what a mirrored view needs (``bod_stat_forward_view``); for the FPN grid it holds when image_w is a
    multiple of 2^max_level.  first_bad_level: the pyramid level (``min_level`` + index) of the first level that fails, else None."""
    a = np.ascontiguousarray(anchors, dtype=np.float32).reshape(-1, 4)
    perm = mirror_anchor_index(level_hw, K)
    if a.shape[0] != perm.shape[0]:
        raise ValueError("the level table holds %d anchors, got %d" % (perm.shape[0], a.shape[0]))
    want = a.copy()
    want[:, 1] = np.float32(image_w) - a[:, 1]
    same = np.all(a[perm].view(np.uint32) == want.view(np.uint32), axis=1)
    off = 0
    for l, (h, w) in enumerate(level_hw):
        n = int(h) * int(w) * K
        if not same[off:off + n].all():
            return False, min_level + l
        off += n
    return True, None


class StatShardedEngine(object):
    """The sample-sharded mode on statistics: ONE statistics handle per rank computes its n = N / world samples
    (``stat_forward`` with sample base rank * n), one all-gather exchanges the 34-float records, every rank resets and folds
    the W records in rank order (identical bits on all ranks), and posterior / soft-NMS / cluster-fuse run replicated.
    ``make_config_kwargs`` are those of engine.make_config for the FULL ensemble.  ``merge_method``: how the handle merges a
    cluster ('bayes', 'centre', 'mixture': ``Engine.set_merge_method``)."""

    def __init__(self, image_hw, weights, anchors, mc_samples, device=0, batch=1, group=None, merge_method='bayes', **make_config_kwargs):
        from .engine import Engine, make_config
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.base, self.n = sample_shard(mc_samples, self.world, self.rank)
        self.engine = Engine(make_config(image_hw, batch=batch, mc_samples=self.n, device=device, mc_ensemble_size=mc_samples,
                                         mc_statistics=True, **make_config_kwargs))
        self.engine.load_weights(weights)
        self.engine.set_anchors(anchors)
        self.engine.set_merge_method(merge_method)
        self._local = stat_views(self.engine)
        self._gathered = None                     # kept alive until the folds that read it have run

    def infer(self, images, seed=0, first_image_id=0):
        """images: [B,H,W,3] float32 (the same on every rank).  Returns this rank's copy of the detections (list over images of
        (scores, means, covs, counts)); identical on all ranks."""
        eng = self.engine
        eng.stat_reset()
        eng.stat_forward(images, seed=seed, first_image_id=first_image_id, sample_base=self.base)
        eng.synchronize()                         # the collective runs on torch's stream, not the engine's
        self._gathered = all_gather_statistics(self._local, self.group)
        torch.cuda.synchronize(self._local["cls"].device)
        eng.stat_reset()
        for rec in self._gathered:                # rank order on every rank
            eng.stat_merge([rec[k].data_ptr() if k in rec else None for k in ("cls", "box", "cov", "ent")], self.n)
        eng.stat_posterior(seed=seed, first_image_id=first_image_id)
        eng.nms()
        eng.cluster_fuse()
        out = [eng.get_detections(i) for i in range(eng.B)]
        if eng.has_class_parts:                   # a fifth element [K,4]: total, aleatoric, epistemic_mc, epistemic_spatial
            out = [d + (eng.get_detection_class_parts(i),) for i, d in enumerate(out)]
        return out


# ---------------------------------------------------------------------------------------------------
# Data-parallel training: every rank runs bod_train_step(apply_update=False) on its own minibatch; the gradients of
# all ~260 tensors sit in ONE contiguous fp32 arena, so the step needs a single all-reduce (39 M floats = 156 MB; a
# ring over 7 xGMI links) instead of per-tensor buckets; the update then runs on the mean gradient (the usual
# data-parallel convention: each rank normalises its loss by its own number of positive anchors).
# ---------------------------------------------------------------------------------------------------
def all_reduce_mean_(grads, group=None):
    """In-place mean of a gradient tensor over the ranks."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    if world == 1:
        return grads
    if grads.is_cuda and dist.get_backend(group) == "gloo":
        host = grads.cpu()
        dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
        grads.copy_(host)
    else:
        dist.all_reduce(grads, op=dist.ReduceOp.SUM, group=group)
    grads.mul_(1.0 / world)
    return grads


def data_parallel_train_step(engine, images, cls_targets, box_targets, positive_mask, negative_mask, learning_rate, group=None,
                             **step_kwargs):
    """One synchronous data-parallel step; returns this rank's loss dict with the norm of the MEAN gradient."""
    out = engine.train_step(images, cls_targets, box_targets, positive_mask, negative_mask, apply_update=False, **step_kwargs)
    g = engine.train_gradients_view()
    all_reduce_mean_(g, group)
    if g.is_cuda:
        torch.cuda.synchronize(g.device)
    out["grad_norm"] = engine.train_apply(learning_rate)
    return out

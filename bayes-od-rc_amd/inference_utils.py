"""``bayes_od_inference`` / ``bayes_od_clustering`` / ``map_dataset_classes`` with the reference's
names, argument meaning, return shapes and error behaviour
(src/retina_net/experiments/inference_utils.py:13-217, :285-364, :372-404), executed by the HIP
pipeline through the C ABI.  Nothing here computes on the host except array reshaping and the
(trivial, index-only) class-name mapping.
"""
import numpy as np

from . import _lib, box_utils, constants


def _bayes_testing_kwargs(bayes_od_config, nms_config, use_full_covar, dataset_name, sample_dict,
                          nms_variant):
    kw = dict(bayes_od_config=bayes_od_config, nms_config=nms_config, use_full_covar=use_full_covar,
              dataset_name=dataset_name, nms_variant=nms_variant)
    if dataset_name == 'kitti':
        orig = np.asarray(sample_dict[constants.ORIGINAL_IM_SIZE_KEY]).reshape(-1, 3)[0]
        kw['orig_size'] = (int(orig[0]), int(orig[1]))
    return kw


def bayes_od_inference(model, sample_dict, bayes_od_config, nms_config, use_full_covar=False,
                       dataset_name='bdd', seed=None, image_id=None, nms_variant='A',
                       return_iou=True, return_engine=False, covariance_parts=False, class_parts=False):
    """Same 5 return values as the reference (:217) for a batch-of-1 ``sample_dict``:

        dirichlet_posterior_count [M,C], gaussian_posterior_means [M,4,1],
        gaussian_posterior_covs [M,4,4], nms_indices [K], predicted_boxes_iou_mat [M,M]

    ``seed`` / ``image_id`` key the Philox streams that replace TF's unseeded RNG.
    ``return_iou=False`` skips materialising the M x M matrix (the device clustering does not
    need it); an empty [0,0] array is returned in its place.
    ``return_engine=True`` appends the handle that produced the results as a sixth value: passing it to
    ``bayes_od_clustering(..., engine=)`` re-uses its device buffers.  Without it the two calls are as independent as
    the reference's (run_inference.py:138-149): nothing is remembered between them.
    ``covariance_parts=True`` appends (in front of the engine) gaussian_posterior_cov_parts [M,3,4,4]: the epistemic, aleatoric
    and prior terms every posterior covariance is the sum of.  ``class_parts=True`` appends (behind it, in front of the engine)
    class_entropy_parts [M,3+C]: total, aleatoric and epistemic entropy of every row's MC class distribution, then that
    distribution itself (mean_probs) -- the array ``bayes_od_clustering(..., class_parts=)`` takes.
    """
    image = np.asarray(sample_dict[constants.IMAGE_NORMALIZED_KEY], dtype=np.float32)
    if image.ndim == 3:
        image = image[None]
    if image.shape[0] != 1:
        raise ValueError("bayes_od_inference mirrors the reference's batch(1) loop; use "
                         "BayesOdPipeline for batched throughput")
    anchors = np.asarray(sample_dict[constants.ANCHORS_KEY], dtype=np.float32)
    anchors = anchors.reshape(-1, 4)
    if model.mc_dropout_samples < 2:
        raise ValueError("bayes_od needs mc_dropout_samples >= 2: the sample covariance divides by N-1 "
                         "(inference_utils.py:241-242)")
    kw = _bayes_testing_kwargs(bayes_od_config, nms_config, use_full_covar, dataset_name, sample_dict,
                               nms_variant)
    if covariance_parts:
        kw['covariance_parts'] = True
    if class_parts:
        kw['class_parts'] = True
    eng = model.engine_for(image.shape[1:3], batch=1, mc_samples=model.mc_dropout_samples, **kw)
    eng.set_anchors(anchors)
    seed = model.seed if seed is None else seed
    if image_id is None:
        image_id = model.image_counter
        model.image_counter += 1
    eng.forward(image, seed=seed, first_image_id=image_id)
    eng.posterior(seed=seed, first_image_id=image_id)
    eng.nms()
    post = eng.get_posterior(0)
    nms_indices = eng.get_nms(0)
    iou = eng.get_iou_matrix(0) if return_iou else np.zeros((0, 0), np.float32)
    out = (post["counts"], post["means"][:, :, None], post["covs"], nms_indices, iou)
    if covariance_parts:
        out += (eng.get_posterior_parts(0),)
    if class_parts:
        out += (np.concatenate([eng.get_posterior_class_parts(0), eng.get_posterior_mean_probs(0)], axis=1),)
    return out + (eng,) if return_engine else out


def bayes_od_clustering(predicted_boxes_class_counts, predicted_boxes_means, predicted_boxes_covs,
                        cluster_centers, affinity_matrix=None, affinity_threshold=0.7, engine=None, class_parts=None,
                        merge_method='bayes', return_merge_terms=False):
    """Bayesian cluster-and-fuse on the device (reference :285-364).

    Returns (final_scores [K,C], final_means [K,4,1], final_covs [K,4,4] (x70), final_counts [K,C]).
    ``affinity_matrix`` [M,M] is used exactly as the reference uses it (:316, members of centre k =
    ``affinity_matrix[:, k] > affinity_threshold``): its K centre columns are uploaded (K*M floats, not M*M).
    ``affinity_matrix=None`` selects the reference pipeline's own affinity, ``bbox_iou_vuvu`` of the
    posterior means (:204-215, run_inference.py:145-149), evaluated on the fly against each centre
    on the device without ever building the M x M matrix.
    ``engine``: optional handle to run on (``bayes_od_inference(..., return_engine=True)``); by default the call runs on a
    small post-processing handle of its own, sized for M boxes -- it depends on nothing but its arguments, like the reference's.
    ``class_parts``: the rows' class_entropy_parts [M,3+C] as ``bayes_od_inference(..., class_parts=True)`` returns them (total,
    aleatoric, epistemic, mean_probs[C]); a fifth value follows, final_class_parts [K,4] = total, aleatoric, epistemic_mc,
    epistemic_spatial entropy of every detection's MC class distribution.  An ``engine`` must then have been made with the option.
    ``merge_method``: 'bayes' (the reference's fusion), 'centre' (the NMS pick: each centre's own row, no factor 70) or 'mixture'
    (the equal-weight Gaussian mixture of the members, no factor 70) -- ``Engine.set_merge_method``; set on every call, the
    default included, because the stand-alone handle is shared between calls.  ``return_merge_terms=True`` (not with 'bayes')
    appends merge_within [K,4,4], merge_between [K,4,4] and merge_members [K]: final_covs = within + between.  Neither goes
    with ``class_parts``.
    """
    from .engine import Engine, make_config, merge_method_id
    merge_method_id(merge_method)
    if merge_method != 'bayes' and class_parts is not None:
        raise ValueError("merge_method=%r does not go with class_parts: the class-entropy parts are defined for the Bayesian fuse only" % merge_method)
    if return_merge_terms and merge_method == 'bayes':
        raise ValueError("return_merge_terms needs merge_method 'centre' or 'mixture': the Bayesian fuse has no merge terms")
    counts = np.ascontiguousarray(predicted_boxes_class_counts, dtype=np.float32)
    means = np.ascontiguousarray(predicted_boxes_means, dtype=np.float32).reshape(-1, 4)
    covs = np.ascontiguousarray(predicted_boxes_covs, dtype=np.float32).reshape(-1, 4, 4)
    centres = np.ascontiguousarray(cluster_centers, dtype=np.int32).reshape(-1)
    m, c = counts.shape
    k = centres.shape[0]
    if class_parts is not None:
        class_parts = np.ascontiguousarray(class_parts, dtype=np.float32)
        if class_parts.shape != (m, 3 + c):
            raise ValueError("class_parts must be [M,3+C] = [%d,%d], got %s" % (m, 3 + c, class_parts.shape))
        if engine is not None and not engine.has_class_parts:
            raise ValueError("class_parts needs an engine made with class_parts=True")
    if k == 0 or m == 0:
        out = (np.zeros((0, c), np.float32), np.zeros((0, 4, 1), np.float32),
               np.zeros((0, 4, 4), np.float32), np.zeros((0, c), np.float32))
        if return_merge_terms:
            out += (np.zeros((0, 4, 4), np.float32), np.zeros((0, 4, 4), np.float32), np.zeros(0, np.int32))
        return out + (np.zeros((0, 4), np.float32),) if class_parts is not None else out
    eng = engine if engine is not None else _standalone_engine(m, c, k, class_parts is not None)
    cfg = eng.cfg
    cfg.nms_iou_threshold = float(affinity_threshold)
    eng.update_config(cfg)
    eng.set_merge_method(merge_method)
    eng.set_posterior(0, counts, means, covs, np.zeros(m, np.float32))
    if class_parts is not None:
        eng.set_posterior_class_parts(0, class_parts[:, 3:], class_parts[:, :3])
    eng._set_centres(0, centres)
    if affinity_matrix is not None:
        aff = np.asarray(affinity_matrix)
        if aff.shape != (m, m):
            raise ValueError("affinity_matrix must be [M,M] = [%d,%d], got %s" % (m, m, aff.shape))
        if centres.min() < 0 or centres.max() >= m:
            raise ValueError("cluster centre out of range [0,%d)" % m)
        eng.set_affinity(0, np.ascontiguousarray(aff[:, centres].T, dtype=np.float32))
    eng.cluster_fuse()
    scores, fmeans, fcovs, fcounts = eng.get_detections(0)
    out = (scores, fmeans[:, :, None], fcovs, fcounts)
    if return_merge_terms:
        out += eng.get_detection_merge_terms(0)
    return out + (eng.get_detection_class_parts(0),) if class_parts is not None else out


_standalone = {}


def _standalone_engine(m, c, k, class_parts=False):
    """Small handle used when bayes_od_clustering is called without a model (pure post-processing):
    geometry only sizes the buffers (A >= M)."""
    from .engine import Engine, make_config
    side = 64
    while True:
        a = sum((-(-side // s)) ** 2 for s in (8, 16, 32, 64, 128)) * 9          # anchors of a side x side input
        if a >= m:
            break
        side *= 2
    key = (side, c, max(k, 100), bool(class_parts))
    if key not in _standalone:
        nms = {'max_output_size': min(max(k, 100), 512), 'iou_threshold': 0.5, 'soft_nms_sigma': 0.5}
        _standalone[key] = Engine(make_config((side, side), batch=1, mc_samples=2, num_classes=c, nms_config=nms,
                                                  class_parts=bool(class_parts)))
    return _standalone[key]


def map_dataset_classes(input_dataset, target_dataset, output_classes):
    """Class-score remapping between label sets (reference :372-404), host-side index shuffling.
    The result has ``len(target_dict) + 1`` columns, as in the reference."""
    mapping = constants.SET_TO_SET_MAPPING_DICTS[input_dataset + '_' + target_dataset]
    if not mapping:
        return output_classes
    in_d = constants.CATEGORY_IDX_MAPPING_DICTS[input_dataset]
    tg_d = constants.CATEGORY_IDX_MAPPING_DICTS[target_dataset]
    mapped = np.zeros([output_classes.shape[0], len(tg_d) + 1])
    if len(output_classes.shape) == 1:
        output_classes = np.expand_dims(output_classes, axis=1)
    names = list(in_d.keys())
    for row, scores in zip(mapped, output_classes):
        j = int(np.argmax(scores))
        row[tg_d[mapping[names[j]]]] = scores[j]
    return mapped


def _detections(engine):
    """Per image the four detection arrays, the covariance parts behind them on a covariance_parts handle, and the class-entropy
    parts [K,4] last on a class_parts handle."""
    dets = [engine.get_detections(b) for b in range(engine.B)]
    if engine.has_cov_parts:
        dets = [d + (engine.get_detection_parts(b),) for b, d in enumerate(dets)]
    if engine.has_class_parts:
        dets = [d + (engine.get_detection_class_parts(b),) for b, d in enumerate(dets)]
    return dets


def _checked_merge_method(merge_method, covariance_parts=False, class_parts=False):
    from .engine import merge_method_id
    merge_method_id(merge_method)
    if merge_method != 'bayes' and (covariance_parts or class_parts):
        raise ValueError("merge_method=%r does not go with covariance_parts / class_parts: the parts are defined for the Bayesian "
                         "fuse only" % merge_method)
    return merge_method


BLACKBOX_OPTIONS = ('min_score', 'min_members', 'affinity_threshold')


def _checked_uncertainty_method(uncertainty_method, blackbox_options, merge_method='bayes', covariance_parts=False, class_parts=False):
    """('bayes_od' | 'black_box', options dict); ValueError for what the library refuses (``bod_set_uncertainty_method``)."""
    from . import _lib
    if uncertainty_method not in _lib.UNCERTAINTY_METHODS:
        raise ValueError("uncertainty_method must be one of %s, got %r" % (sorted(_lib.UNCERTAINTY_METHODS), uncertainty_method))
    opts = dict(blackbox_options or {})
    unknown = sorted(set(opts) - set(BLACKBOX_OPTIONS))
    if unknown:
        raise ValueError("blackbox_options: unknown key(s) %s (known: %s)" % (unknown, list(BLACKBOX_OPTIONS)))
    if uncertainty_method == 'black_box':
        if covariance_parts or class_parts:
            raise ValueError("uncertainty_method='black_box' does not go with covariance_parts / class_parts: the parts are defined "
                             "for 'bayes_od' only")
        if merge_method != 'bayes':
            raise ValueError("uncertainty_method='black_box' does not go with merge_method=%r: black-box MC dropout merges the pooled "
                             "sample detections by its own rule" % merge_method)
    elif opts:
        raise ValueError("blackbox_options belong to uncertainty_method='black_box'")
    return uncertainty_method, opts


class BayesOdPipeline(object):
    """Batched, fully device-resident form of the reference's per-image loop body
    (src/retina_net/experiments/run_inference.py:137-161): forward -> posterior -> soft-NMS ->
    cluster-and-fuse for ``batch`` images per call, no host round trip in between.  ``uncertainty_method='black_box'`` (with
    ``blackbox_options``: min_score, min_members, affinity_threshold) runs the baseline in its place: every MC sample through the
    validation post-process and the soft-NMS on its own, then the pooled detections merged."""

    def __init__(self, model, image_hw, batch, bayes_od_config, nms_config, use_full_covar=True,
                 dataset_name='bdd', orig_size=None, nms_variant='A', anchors=None, covariance_parts=False, class_parts=False,
                 merge_method='bayes', uncertainty_method='bayes_od', blackbox_options=None):
        self._merge = _checked_merge_method(merge_method, covariance_parts, class_parts)
        self._method, self._bb = _checked_uncertainty_method(uncertainty_method, blackbox_options, merge_method, covariance_parts,
                                                             class_parts)
        self._kw = dict(bayes_od_config=bayes_od_config, nms_config=nms_config, use_full_covar=use_full_covar,
                        dataset_name=dataset_name, nms_variant=nms_variant, orig_size=orig_size)
        if covariance_parts:
            self._kw['covariance_parts'] = True
        if class_parts:
            self._kw['class_parts'] = True
        self.model, self._hw, self._batch = model, tuple(image_hw), batch
        self.engine = self.bind()
        if anchors is not None:
            self.engine.set_anchors(anchors)

    def bind(self, orig_size=None):
        """(Re-)apply this pipeline's testing configuration to its engine.  Engines are cached by the model per
        (network size, batch, N), so two pipelines that differ only in ``orig_size`` -- KITTI frames of 370x1224 and
        375x1242 both resize to the same network input -- share one handle: the S mu / S Sigma S^T factors
        (inference_utils.py:147-167 takes them per sample from ORIGINAL_IM_SIZE) must be set before every batch."""
        if orig_size is not None:
            self._kw['orig_size'] = tuple(orig_size)
        self.engine = self.model.engine_for(self._hw, batch=self._batch, mc_samples=self.model.mc_dropout_samples, **self._kw)
        if self._method == 'bayes_od':                     # (the handle is shared: both set on every bind, the defaults included)
            self.engine.set_uncertainty_method('bayes_od')
        self.engine.set_merge_method(self._merge)
        if self._method != 'bayes_od':
            self.engine.set_uncertainty_method(self._method, **self._bb)
        return self.engine

    def merge_terms(self):
        """Per image (within [K,4,4], between [K,4,4], members [K]) of the last call's detections ('centre' / 'mixture' merges and
        uncertainty_method 'black_box')."""
        return [self.engine.get_detection_merge_terms(b) for b in range(self.engine.B)]

    def upload_mixed(self, frames, means, aspect_resize=True, corruption=None):
        """``batch`` uint8 frames of mixed source sizes into the engine, for ``__call__(None, ...)``: every frame is rescaled by
        its own S = orig / net (inference_utils.py:147-167 takes it per sample), so no ``bind(orig_size=...)`` per size.
        ``corruption``: (chain, frame ids, seed) -- the frames are corrupted on the device on their way in."""
        self.bind()
        from . import datasets
        if corruption is not None:
            self.engine.set_upload_corruption(corruption[0], frame_ids=corruption[1], seed=corruption[2])
        datasets.upload_frames(self.engine, frames, means, aspect_resize=aspect_resize)     # (--device_jpeg: frames may be JPEG files)

    def __call__(self, images=None, seed=0, first_image_id=0):
        """images [B,H,W,3] (or None to reuse the uploaded device batch).  Returns, per image,
        (output_classes [K,C], output_boxes_vuhw [K,4], output_covs [K,4,4], output_counts [K,C]); a pipeline made with
        ``covariance_parts=True`` adds output_cov_parts [K,3,4,4] (epistemic, aleatoric, prior), one made with ``class_parts=True``
        output_class_parts [K,4] (total, aleatoric, epistemic_mc, epistemic_spatial) last."""
        self.bind()
        self.engine.infer(images, seed=seed, first_image_id=first_image_id)
        return _detections(self.engine)


class EnsemblePipeline(object):
    """``BayesOdPipeline`` for an ensemble: ONE posterior per image from the MC samples of several weight sets and / or several
    passes of one handle (deep / checkpoint ensembles; more samples than one forward holds).  ``models``: RetinaNetModel
    instances with loaded weights and the same heads; every member runs ``passes`` forwards of ``samples_per_member`` samples on
    a statistics handle of its own (``make_config(mc_statistics=True)``) -- member m, pass p draws the dropout samples
    ``(m * passes + p) * n ..`` -- and the per-anchor statistics (34 floats per anchor, whatever the sample count) are folded
    into member 0's accumulator in member order; posterior, soft-NMS and cluster-and-fuse run there with N = the total.  A list
    of one model with ``passes = k`` is "N = k * n on one handle".  Same call and return shape as ``BayesOdPipeline``.
    ``views``: the test-time views every pass runs, ``'identity'`` and / or ``'hflip'`` (the frames mirrored left-right on the
    device, the record mapped back to the anchors of the frames as given while it is folded: ``Engine.stat_forward(view=)``);
    with V views member m, pass p, view index v draws the samples ``((m * passes + p) * V + v) * n ..``.
    ``acquisition``: ``dict(min_foreground=, top_k=)`` (either may be left out) -- after the folds into member 0 and before its
    posterior, the merged record is reduced to acquisition scores (``Engine.stat_acquisition``), kept as
    ``.acquisition`` = (scores [B,12], per_class [B,C-1,3]); ``acquisition_only=True`` stops there: no posterior, NMS, clustering
    or records, and ``__call__`` returns the acquisition alone."""

    def __init__(self, models, image_hw, batch, bayes_od_config, nms_config, samples_per_member, passes=1, use_full_covar=True,
                 dataset_name='bdd', orig_size=None, nms_variant='A', anchors=None, views=('identity',), covariance_parts=False,
                 class_parts=False, merge_method='bayes', acquisition=None, acquisition_only=False):
        from .engine import Engine, make_config
        self._merge = _checked_merge_method(merge_method, covariance_parts, class_parts)
        if acquisition is not None and set(acquisition) - {'min_foreground', 'top_k'}:
            raise ValueError("acquisition takes min_foreground and top_k, got %s" % sorted(acquisition))
        if acquisition_only and acquisition is None:
            raise ValueError("acquisition_only needs acquisition=dict(...)")
        self._acq = None if acquisition is None else dict(acquisition)
        self._acq_only = bool(acquisition_only)
        self.acquisition = None
        models = list(models)
        if not models:
            raise ValueError("EnsemblePipeline needs at least one model")
        n, passes = int(samples_per_member), int(passes)
        if n < 1 or passes < 1:
            raise ValueError("samples_per_member and passes must be >= 1")
        self.views = [Engine._view(v) for v in ([views] if isinstance(views, (str, int)) else views)]
        if not self.views:
            raise ValueError("EnsemblePipeline needs at least one view")
        self.total = len(models) * passes * len(self.views) * n
        if self.total < 2:
            raise ValueError("bayes_od needs at least 2 samples in all: the sample covariance divides by N-1 "
                             "(inference_utils.py:241-242)")
        first = models[0]
        for m in models:
            if m._weights is None:
                raise ValueError("no weights loaded: call model.load_weights(...) on every ensemble member")
            if (m.num_classes, m.anchors_per_location, m.compute_covar) != (first.num_classes, first.anchors_per_location,
                                                                            first.compute_covar):
                raise ValueError("ensemble members must share num_classes, anchors_per_location and the covariance head")
        self.models, self.n, self.passes = models, n, passes
        self._hw, self._batch = tuple(image_hw), int(batch)
        self._kw = dict(bayes_od_config=bayes_od_config, nms_config=nms_config, use_full_covar=use_full_covar,
                        dataset_name=dataset_name, nms_variant=nms_variant, orig_size=orig_size)
        self._parts = bool(covariance_parts)          # on member 0's handle, where the merged posterior and the fusion run
        self._class_parts = bool(class_parts)         # on every member's handle: each record carries ent_sum into the merge
        self.engines = []
        for m in models:
            eng = Engine(self._config(m, first=not self.engines))
            eng.load_weights(m._weights)
            self.engines.append(eng)
        self.engine = self.engines[0]             # uploads, the merged accumulator and the Bayesian stages live here
        self.engine.set_merge_method(self._merge)
        if anchors is not None:
            self.set_anchors(anchors)

    def _config(self, m, first=False):
        from .engine import make_config
        return make_config(self._hw, batch=self._batch, mc_samples=self.n, num_classes=m.num_classes + 1,
                           anchors_per_location=m.anchors_per_location, device=m.device, dropout_rate=m.dropout_rate,
                           has_covar_head=m.compute_covar, precision=m.precision, backbone_depth=m.backbone_depth,
                           mc_ensemble_size=self.total, mc_statistics=True, covariance_parts=self._parts and first,
                           class_parts=self._class_parts, **self._kw)

    def set_anchors(self, anchors):
        for eng in self.engines:
            eng.set_anchors(anchors)

    def bind(self, orig_size=None):
        """Re-apply the testing configuration (a new ``orig_size``: KITTI's per-size rescale) to every member's handle."""
        if orig_size is not None:
            self._kw['orig_size'] = tuple(orig_size)
            for i, (m, eng) in enumerate(zip(self.models, self.engines)):
                eng.update_config(self._config(m, first=i == 0))
        return self.engine

    def upload_mixed(self, frames, means, aspect_resize=True, corruption=None):
        from . import datasets
        if corruption is not None:
            self.engine.set_upload_corruption(corruption[0], frame_ids=corruption[1], seed=corruption[2])
        datasets.upload_frames(self.engine, frames, means, aspect_resize=aspect_resize)

    def __call__(self, images=None, seed=0, first_image_id=0):
        """images [B,H,W,3], or None to run every member on the batch uploaded into member 0's handle."""
        shared = None
        if images is None:
            shared = self.engine._device_images(None)
            self.engine.synchronize()             # the upload is complete before another handle's stream reads it
        for m, eng in enumerate(self.engines):
            eng.stat_reset()
            for p in range(self.passes):
                for v, view in enumerate(self.views):
                    base = ((m * self.passes + p) * len(self.views) + v) * self.n
                    if images is None and m > 0:
                        eng.stat_forward(None, seed=seed, first_image_id=first_image_id, sample_base=base, device_images=shared, view=view)
                    else:
                        eng.stat_forward(images, seed=seed, first_image_id=first_image_id, sample_base=base, view=view)
        for eng in self.engines[1:]:
            self.engine.stat_merge_from(eng)
        if self._acq is not None:
            self.acquisition = self.engine.stat_acquisition(**self._acq)
            if self._acq_only:
                return self.acquisition
        self.engine.stat_posterior(seed=seed, first_image_id=first_image_id)
        self.engine.nms()
        self.engine.cluster_fuse()
        return _detections(self.engine)

    def merge_terms(self):
        """Per image (within [K,4,4], between [K,4,4], members [K]) of the last call's detections ('centre' / 'mixture' only)."""
        return [self.engine.get_detection_merge_terms(b) for b in range(self.engine.B)]


def post_process_predictions(sample_dict, prediction_dict, dataset_name='bdd', engine=None, nms_config=None):
    """Validation post-processing with the reference's signature and return value
    (src/retina_net/experiments/validation_utils.py:10-77): ``(predicted_boxes_classes [K,C],
    predicted_boxes_corners [K,4])`` of the first image of the batch -- softmax, background filter, soft-NMS on the
    top score -- computed on the device (``bod_validation_post`` + ``bod_nms``).  ``engine``: the handle that produced
    ``prediction_dict`` (default: a post-only handle of the right geometry is created)."""
    from .engine import Engine, make_config
    anchors = _lib.as_f32(np.asarray(sample_dict[constants.ANCHORS_KEY]))
    if anchors.ndim == 3:
        anchors = anchors[0]
    cls = _lib.as_f32(np.asarray(prediction_dict[constants.ANCHORS_CLASS_PREDICTIONS_KEY]))[0:1]
    box = _lib.as_f32(np.asarray(prediction_dict[constants.ANCHORS_BOX_PREDICTIONS_KEY]))[0:1]
    image = np.asarray(sample_dict[constants.IMAGE_NORMALIZED_KEY])
    hw = image.shape[1:3] if image.ndim == 4 else image.shape[0:2]
    if engine is None:
        engine = Engine(make_config(hw, batch=1, mc_samples=1, num_classes=cls.shape[-1], nms_config=nms_config,
                                    has_covar_head=False))
        engine.set_anchors(anchors)
    if (engine.B, engine.N) != (1, 1):
        raise ValueError("post_process_predictions works on a batch-1, single-sample handle")
    engine.set_raw(cls.reshape(1, 1, -1, cls.shape[-1]), box.reshape(1, 1, -1, 4), None)
    engine.validation_post()
    engine.nms()
    post = engine.get_posterior(0)
    idx = engine.get_nms(0)
    corners = box_utils.vuhw_to_vuvu_np(post["means"]) if post["means"].size else np.zeros((0, 4), np.float32)
    if dataset_name == 'kitti':
        orig = np.asarray(sample_dict[constants.ORIGINAL_IM_SIZE_KEY]).reshape(-1)[-3:]
        n = np.asarray([hw[0], hw[1]] * 2, np.float32)
        s = np.asarray([orig[0], orig[1]] * 2, np.float32)
        corners = (corners / n) * s
    return post["score"][idx], corners[idx]

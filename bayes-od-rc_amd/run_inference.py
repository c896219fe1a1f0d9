"""Inference driver with the reference's CLI (src/retina_net/experiments/run_inference.py:254-299):

    python -m bayes_od_rc_amd.run_inference --gpu_device 0 --yaml_path <cfg.yaml> --data_split test \
        [--weights weights.npz] [--dataset | --frames frames.npy | --synthetic N] [--image_size H W]

``--dataset`` reads the yaml's BDD / KITTI tree through ``datasets.build_dataset`` (the reference's default,
run_inference.py:60-72): frames are decoded on the host, uploaded as uint8 and normalised / resized on the GPU
(``bod_upload_frames_u8``); frames of one batch must share a size, so a batch ends where the size changes.  With
``--mixed_sizes`` batches are formed in dataset order whatever the sizes (``bod_upload_frames_u8_ragged``: every frame
is resized and its boxes rescaled by its own size).  Otherwise frames come from an .npy of
normalised BGR images or are synthetic.  Weights: an .npz with Keras layer names (the TF-checkpoint converter is
SURVEY.md section 8 f3).
"""
import argparse
import os
import sys
import time

import numpy as np

from . import box_utils, config_utils, inference_utils, synthetic, writers
from .anchor_generator import FpnAnchorGenerator
from .model import RetinaNetModel


def test_model(config, args):
    test_config = config['testing_config']
    want_class = _want_class_parts(config, args)          # decided once: the writer and every pipeline get the same answer
    merge = check_merge_options(config, args)             # likewise; refuses what does not go together before anything is built
    method, bb_options = check_uncertainty_options(config, args)
    acq = check_acquisition_options(config, args)         # None, or the options of --acquisition
    dataset_config = config['dataset_config']
    training_dataset = dataset_config['dataset']
    test_dataset = test_config['test_dataset']
    nms_config = test_config['nms_config']
    model = RetinaNetModel(config['model_config'], device=int(args.gpu_device), seed=args.seed)
    if getattr(args, 'ensemble', None):
        model = _ensemble_members(config, args)
    elif args.weights:
        if not os.path.exists(args.weights):
            raise ValueError('%s must exist (no checkpoint entry)' % args.weights)
        model.load_weights(args.weights)
    else:
        model.load_weights(synthetic.make_weights(config['model_config']['header']['num_classes'] + 1,
                                                  config['model_config']['header']['anchors_per_location']))
    if args.dataset:
        return _test_model_on_dataset(config, args, model)
    if args.frames:
        frames = np.load(args.frames).astype(np.float32)
    else:
        frames = synthetic.make_frames(args.synthetic, args.image_size[0], args.image_size[1])
    hw = frames.shape[1:3]
    gen = FpnAnchorGenerator(dataset_config['anchor_generator'])
    anchors = gen.generate_all((hw[0], hw[1], 3))
    batch = max(1, min(args.batch, len(frames)))
    orig = tuple(args.orig_size) if args.orig_size else (hw[0], hw[1])
    pipes = {}

    def pipe_for(b):                      # the tail (len(frames) % batch frames) runs through a smaller-batch handle
        if b not in pipes:
            pipes[b] = _make_pipeline(model, args, hw, b, test_config['bayes_od_config'], nms_config,
                                      use_full_covar=test_config['use_full_covar'],
                                      dataset_name=test_dataset, orig_size=orig, anchors=anchors, class_parts=want_class,
                                      merge_method=merge, uncertainty_method=method, blackbox_options=bb_options,
                                      acquisition=acq)
        return pipes[b]
    predictions_dir = os.path.join(config_utils.data_dir(), 'outputs', config['checkpoint_name'], 'predictions')
    fusion = writer_fusion_name(test_config['bayes_od_config']['fusion_method'], merge)
    log = _AcquisitionLog(acq, writers.tree_root(predictions_dir, test_dataset, test_config['ckpt_idx'], method, fusion),
                          only=getattr(args, 'acq_only', False))
    if log.only:                                         # --acq_only: the scores alone, no prediction tree
        for lo in range(0, len(frames), batch):
            chunk = frames[lo:lo + batch]
            pipe = pipe_for(len(chunk))
            pipe(chunk, seed=args.seed, first_image_id=lo)
            log.add(['%06d' % (lo + b) for b in range(len(chunk))], pipe)
        return log.write()
    writer = writers.PredictionWriter(predictions_dir, test_dataset, test_config['ckpt_idx'],
                                      method, fusion,
                                      cov_parts=_want_parts(args), class_parts=want_class)
    categories = dataset_config[training_dataset]['training_data_config']['categories']
    start = time.time()
    n_done = 0
    for lo in range(0, len(frames), batch):              # every frame, like the reference's loop (run_inference.py:137)
        chunk = frames[lo:lo + batch]
        dets = pipe_for(len(chunk))(chunk, seed=args.seed, first_image_id=lo)
        log.add(['%06d' % (lo + b) for b in range(len(chunk))], pipe_for(len(chunk)))
        if _want_merge_terms(args):
            _write_merge_terms(writer.root, ['%06d' % (lo + b) for b in range(len(chunk))], pipe_for(len(chunk)).merge_terms())
        for b, (classes, boxes_vuhw, covs, counts, *parts) in enumerate(dets):
            parts = _part_kwargs(_want_parts(args), want_class, parts)
            boxes = box_utils.vuhw_to_vuvu_np(boxes_vuhw) if boxes_vuhw.size else boxes_vuhw
            mapped = classes
            if training_dataset != test_dataset and boxes.size > 0:
                mapped = inference_utils.map_dataset_classes(training_dataset, test_dataset, classes)
            writer.write('%06d' % (lo + b), boxes, mapped, boxes_vuhw, covs, classes, counts, categories, **parts)
            n_done += 1
        if getattr(args, 'render', None):     # (normalised BGR frames back to the uint8 RGB they were made from)
            from . import constants
            rgb = np.clip(np.rint(chunk[:, :, :, ::-1] + np.asarray(constants.MEANS_DICT['ImageNet'], np.float32)), 0, 255).astype(np.uint8)
            _render_batch(args, writer.root, ['%06d' % (lo + b) for b in range(len(chunk))], list(rgb), categories)
        sys.stdout.write('\r{}'.format(n_done) + ' /' + str(len(frames)))
    writer.close()
    log.write()
    elapsed = time.time() - start
    print("\nMean frame rate: " + str(n_done / max(elapsed, 1e-9)))
    return writer.root


def _ensemble_members(config, args):
    """--ensemble w0.npz w1.npz ...: one model per weight file (a deep / checkpoint ensemble)."""
    members = []
    for path in args.ensemble:
        if not os.path.exists(path):
            raise ValueError('%s must exist (no checkpoint entry)' % path)
        m = RetinaNetModel(config['model_config'], device=int(args.gpu_device), seed=args.seed)
        m.load_weights(path)
        members.append(m)
    return members


MERGE_TERM_DIRS = ('merge_within', 'merge_between', 'merge_members')


def resolve_merge_method(config, flag=None):
    """How a cluster becomes a detection: --merge_method if given, else the yaml's testing_config.bayes_od_config.merge_method,
    else 'bayes'.  ValueError for a name that is none of 'bayes', 'centre', 'mixture'."""
    from .engine import MERGE_METHODS
    name = flag
    if name is None:
        name = ((config.get('testing_config') or {}).get('bayes_od_config') or {}).get('merge_method')
    if name is None:
        name = 'bayes'
    if name not in MERGE_METHODS:
        raise ValueError("merge_method must be one of %s, got %r" % (sorted(MERGE_METHODS), name))
    return name


def writer_fusion_name(fusion_method, merge_method):
    """The ``fusion_method`` PredictionWriter names the tree after: the yaml's for the default method (today's path), and
    '<fusion_method>-<merge_method>' for another, so the trees of one checkpoint sit side by side."""
    return fusion_method if merge_method == 'bayes' else '%s-%s' % (fusion_method, merge_method)


def check_merge_options(config, args):
    """The resolved merge method; ValueError for a combination the library refuses: a non-default method with the covariance or
    class-entropy parts (they are defined for the Bayesian fuse only), --merge_terms with the default method (it has none)."""
    merge = resolve_merge_method(config, getattr(args, 'merge_method', None))
    if merge != 'bayes' and _want_parts(args):
        raise ValueError("--merge_method %s does not go with --covariance_parts: the covariance parts are defined for the Bayesian "
                         "fuse only" % merge)
    if merge != 'bayes' and _want_class_parts(config, args):
        raise ValueError("--merge_method %s does not go with --class_uncertainty: the class-entropy parts are defined for the "
                         "Bayesian fuse only" % merge)
    if merge == 'bayes' and _want_merge_terms(args) and resolve_uncertainty_method(config, getattr(args, 'uncertainty_method', None)) != 'black_box':
        raise ValueError("--merge_terms needs --merge_method centre or mixture: the Bayesian fuse has no merge terms")
    return merge


UNCERTAINTY_METHODS = ('bayes_od', 'black_box')


def resolve_uncertainty_method(config, flag=None):
    """--uncertainty_method if given, else the yaml's testing_config.uncertainty_method, else 'bayes_od'.  ValueError for any other
    name (the reference's other methods are not implemented)."""
    name = flag
    if name is None:
        name = (config.get('testing_config') or {}).get('uncertainty_method')
    if name is None:
        name = 'bayes_od'
    if name not in UNCERTAINTY_METHODS:
        raise ValueError("uncertainty_method must be one of %s, got %r" % (list(UNCERTAINTY_METHODS), name))
    return name


def check_uncertainty_options(config, args):
    """(method, black-box options); ValueError, with the reason, for what black-box MC dropout does not go with: the covariance and
    class-entropy parts and a non-default merge method (defined for 'bayes_od' only), --ensemble and --tta_flip (they merge
    per-anchor statistics, and the method needs every sample's own head outputs), and its options without it."""
    method = resolve_uncertainty_method(config, getattr(args, 'uncertainty_method', None))
    opts = {}
    if getattr(args, 'bb_min_score', None) is not None:
        opts['min_score'] = float(args.bb_min_score)
    if getattr(args, 'bb_min_members', None) is not None:
        opts['min_members'] = int(args.bb_min_members)
    if method != 'black_box':
        if opts:
            raise ValueError("--bb_min_score / --bb_min_members belong to --uncertainty_method black_box")
        return method, None
    if _want_parts(args):
        raise ValueError("--uncertainty_method black_box does not go with --covariance_parts: the covariance parts are defined for "
                         "bayes_od only")
    if _want_class_parts(config, args):
        raise ValueError("--uncertainty_method black_box does not go with --class_uncertainty: the class-entropy parts are defined "
                         "for bayes_od only")
    if getattr(args, 'ensemble', None) or getattr(args, 'tta_flip', False):
        raise ValueError("--uncertainty_method black_box does not go with --ensemble / --tta_flip: they merge per-anchor statistics, "
                         "and black-box MC dropout post-processes every sample's own head outputs")
    if resolve_merge_method(config, getattr(args, 'merge_method', None)) != 'bayes':
        raise ValueError("--uncertainty_method black_box does not go with --merge_method %s: it merges the pooled sample detections "
                         "by its own rule" % resolve_merge_method(config, getattr(args, 'merge_method', None)))
    if opts.get('min_members', 1) < 1 or not (0.0 <= opts.get('min_score', 0.0) < float('inf')):
        raise ValueError("--bb_min_members must be >= 1 and --bb_min_score finite and >= 0")
    return method, opts


def _want_acquisition(args):
    return bool(getattr(args, 'acquisition', False) or getattr(args, 'acq_only', False))


def check_acquisition_options(config, args):
    """None, or ``dict(min_foreground=, top_k=)`` for --acquisition / --acq_only; ValueError, with the reason, for what does not go
    with them: black-box MC dropout (it has no statistics handle to score), a non-default merge method (the handles carry the
    class-entropy parts, defined for the Bayesian fuse only), the options without the flag, and with --acq_only everything that
    needs the detections it skips."""
    from . import acquisition
    opts = {}
    if getattr(args, 'acq_min_foreground', None) is not None:
        opts['min_foreground'] = float(args.acq_min_foreground)
    if getattr(args, 'acq_top_k', None) is not None:
        opts['top_k'] = int(args.acq_top_k)
    if not _want_acquisition(args):
        if opts:
            raise ValueError("--acq_min_foreground / --acq_top_k belong to --acquisition")
        return None
    if resolve_uncertainty_method(config, getattr(args, 'uncertainty_method', None)) == 'black_box':
        raise ValueError("--acquisition does not go with --uncertainty_method black_box: the scores are read from a statistics handle, "
                         "and black-box MC dropout has none")
    if getattr(args, 'acq_only', False):
        for flag, on in (('--render', getattr(args, 'render', None)), ('--covariance_parts', _want_parts(args)),
                         ('--class_uncertainty', _want_class_parts(config, args)),
                         ('--merge_method', getattr(args, 'merge_method', None) is not None), ('--merge_terms', _want_merge_terms(args))):
            if on:
                raise ValueError("--acq_only does not go with %s: it skips the posterior, NMS and clustering, so there are no "
                                 "detections" % flag)
    elif resolve_merge_method(config, getattr(args, 'merge_method', None)) != 'bayes':
        raise ValueError("--acquisition does not go with a non-default merge method: its handles carry the class-entropy parts, which "
                         "are defined for the Bayesian fuse only")
    opts = dict(acquisition.DEFAULTS, **opts)
    if not 0.0 <= opts['min_foreground'] <= 1.0 or not 1 <= opts['top_k'] <= 1024:
        raise ValueError("--acq_min_foreground must lie in [0, 1] and --acq_top_k in 1..1024")
    return opts


class _AcquisitionLog(object):
    """--acquisition: every batch's scores (``EnsemblePipeline.acquisition``) under its frames' names, written as
    <tree>/acquisition.npz (``frames``, ``columns``, ``scores``, ``per_class``) at the end.  Inert without the flag."""

    def __init__(self, options, root, only=False):
        self.on, self.root = options is not None, root
        self.only = self.on and bool(only)            # --acq_only: the pipelines return no detections and no tree is written
        self.names, self.scores, self.per_class = [], [], []

    def add(self, names, pipe):
        if self.on:
            scores, per_class = pipe.acquisition
            self.names.extend(names)
            self.scores.append(np.array(scores[:len(names)]))
            self.per_class.append(np.array(per_class[:len(names)]))

    def write(self):
        if self.on and self.names:
            from . import acquisition
            os.makedirs(self.root, exist_ok=True)
            acquisition.save(os.path.join(self.root, 'acquisition.npz'), self.names, np.concatenate(self.scores),
                             np.concatenate(self.per_class))
        return self.root


def _want_merge_terms(args):
    return bool(getattr(args, 'merge_terms', False))


def _write_merge_terms(root, names, terms):
    """--merge_terms: merge_within/<frame>.npy [K,4,4], merge_between/<frame>.npy [K,4,4], merge_members/<frame>.npy [K] beside cov/."""
    for d in MERGE_TERM_DIRS:
        os.makedirs(os.path.join(root, d), exist_ok=True)
    for name, arrays in zip(names, terms):
        for d, a in zip(MERGE_TERM_DIRS, arrays):
            np.save(os.path.join(root, d, name + '.npy'), a)


def _want_parts(args):
    return bool(getattr(args, 'covariance_parts', False))


def _want_class_parts(config, args):
    """--class_uncertainty, or the yaml's testing_config.class_uncertainty."""
    return bool(getattr(args, 'class_uncertainty', False) or config.get('testing_config', {}).get('class_uncertainty', False))


def _part_kwargs(want_cov, want_class, parts):
    """The arrays a pipeline appends to a detection tuple (covariance parts, then class parts) as PredictionWriter.write keywords."""
    names = (['output_cov_parts'] if want_cov else []) + (['output_class_parts'] if want_class else [])
    return dict(zip(names, parts))


def _make_pipeline(model, args, hw, batch, bayes_od_config, nms_config, **kw):
    """``class_parts=``: the caller's ``_want_class_parts(config, args)`` -- the same value its writer was made with.
    BayesOdPipeline of the one model, or -- ``model`` a list (--ensemble) -- EnsemblePipeline with the yaml's
    mc_dropout_samples per member and --mc_passes passes each.  --tta_flip: every pass runs the frames as given and mirrored
    left-right; without --ensemble that is a one-member EnsemblePipeline of the one model, and so is --acquisition."""
    tta = bool(getattr(args, 'tta_flip', False))
    acq = kw.pop('acquisition', None)     # --acquisition: check_acquisition_options' answer, decided once by the caller
    if _want_parts(args):                 # --covariance_parts: every detection's epistemic / aleatoric / prior covariance
        kw = dict(kw, covariance_parts=True)
    if kw.pop('class_parts', False):      # --class_uncertainty / testing_config.class_uncertainty, decided once by the caller
        kw = dict(kw, class_parts=True)
    if acq is not None:                   # statistics handles that carry ent_sum, so that the mutual information exists
        kw = dict(kw, class_parts=True, acquisition=dict(acq), acquisition_only=bool(getattr(args, 'acq_only', False)))
        if kw['acquisition_only']:        # (no cluster is merged: a yaml's merge method has nothing to act on)
            kw['merge_method'] = 'bayes'
    if isinstance(model, list) or tta or acq is not None:
        members = model if isinstance(model, list) else [model]
        # statistics handles: bayes_od only (check_uncertainty_options has refused black_box with --ensemble / --tta_flip)
        kw = dict(kw)
        if kw.pop('uncertainty_method', 'bayes_od') != 'bayes_od':
            raise ValueError("uncertainty_method 'black_box' does not go with --ensemble / --tta_flip")
        kw.pop('blackbox_options', None)
        return inference_utils.EnsemblePipeline(members, hw, batch, bayes_od_config, nms_config, members[0].mc_dropout_samples,
                                                passes=int(getattr(args, 'mc_passes', 1) or 1),
                                                views=('identity', 'hflip') if tta else ('identity',), **kw)
    return inference_utils.BayesOdPipeline(model, hw, batch, bayes_od_config, nms_config, **kw)


def _test_model_on_dataset(config, args, model):
    """The reference's loop over the dataset handler (run_inference.py:60-72,137-171): batch(1) there, batches
    of equally sized frames here; preprocessing on the device."""
    from . import constants, datasets
    test_config = config['testing_config']
    want_class = _want_class_parts(config, args)
    merge = check_merge_options(config, args)
    method, bb_options = check_uncertainty_options(config, args)
    acq = check_acquisition_options(config, args)
    dataset_config = config['dataset_config']
    training_dataset, test_dataset = dataset_config['dataset'], test_config['test_dataset']
    handler = datasets.build_dataset(dict(dataset_config, dataset=test_dataset), 'test')
    kitti = test_dataset == 'kitti'
    predictions_dir = os.path.join(config_utils.data_dir(), 'outputs', config['checkpoint_name'], 'predictions')
    fusion = writer_fusion_name(test_config['bayes_od_config']['fusion_method'], merge)
    log = _AcquisitionLog(acq, writers.tree_root(predictions_dir, test_dataset, test_config['ckpt_idx'], method, fusion),
                          only=getattr(args, 'acq_only', False))
    writer = None if log.only else writers.PredictionWriter(predictions_dir, test_dataset, test_config['ckpt_idx'], method, fusion,
                                                            cov_parts=_want_parts(args), class_parts=want_class)
    categories = dataset_config[training_dataset]['training_data_config']['categories']
    gen = FpnAnchorGenerator(dataset_config['anchor_generator'])
    pipes = {}
    pending = []
    device_jpeg = bool(getattr(args, 'device_jpeg', False))
    device_png = bool(getattr(args, 'device_png', False))
    corrupt = _corruption(args)              # --corrupt NAME:SEVERITY: frames are corrupted on the device at upload
    # --device_jpeg, --device_png and --corrupt form their batches as --mixed_sizes does
    mixed = bool(getattr(args, 'mixed_sizes', False)) or device_jpeg or device_png or corrupt is not None
    handler.defer_decode = device_jpeg       # JPEG files travel as bytes and are decoded on the device at upload
    handler.defer_png = device_png           # PNG files likewise

    def emit(dets, pipe):
        log.add([p[0] for p in pending], pipe)
        if log.only:                         # (dets is the acquisition itself)
            del pending[:]
            return
        if _want_merge_terms(args):
            _write_merge_terms(writer.root, [p[0] for p in pending], pipe.merge_terms())
        for (name, _, _), (classes, boxes_vuhw, covs, counts, *parts) in zip(pending, dets):
            parts = _part_kwargs(_want_parts(args), want_class, parts)
            boxes = box_utils.vuhw_to_vuvu_np(boxes_vuhw) if boxes_vuhw.size else boxes_vuhw
            mapped = classes
            if training_dataset != test_dataset and boxes.size > 0:
                mapped = inference_utils.map_dataset_classes(training_dataset, test_dataset, classes)
            writer.write(name, boxes, mapped, boxes_vuhw, covs, classes, counts, categories, **parts)
        _render_batch(args, writer.root, [p[0] for p in pending], [p[1] for p in pending], categories)
        del pending[:]

    def flush_mixed():
        """--mixed_sizes: one handle per batch count (the full batch, the tail); the frames' own sizes travel with the upload."""
        if not pending:
            return
        hw = tuple(handler.resize_shape) if kitti else pending[0][1].shape[:2]
        key = ('mixed', len(pending))
        if key not in pipes:
            # orig_size only switches the KITTI rescale on: the ragged upload gives every frame its own factors
            pipes[key] = _make_pipeline(
                model, args, hw, len(pending), test_config['bayes_od_config'], test_config['nms_config'],
                use_full_covar=test_config['use_full_covar'], dataset_name=test_dataset, orig_size=hw,
                anchors=gen.generate_all((hw[0], hw[1], 3)), class_parts=want_class, merge_method=merge,
                uncertainty_method=method, blackbox_options=bb_options, acquisition=acq)
        pipe = pipes[key]
        # (a frame's corruption is keyed on its dataset index: the same whatever batch or run it falls into)
        corruption = None if corrupt is None else (corrupt[0], [p[2] for p in pending], corrupt[1])
        pipe.upload_mixed([p[1] for p in pending], constants.MEANS_DICT[handler.im_normalization], aspect_resize=kitti,
                          corruption=corruption)
        emit(pipe(None, seed=args.seed, first_image_id=pending[0][2]), pipe)

    def flush():
        if mixed:
            return flush_mixed()
        if not pending:
            return
        frames = np.stack([p[1] for p in pending])
        src_hw = frames.shape[1:3]
        hw = tuple(handler.resize_shape) if kitti else src_hw
        key = (src_hw, len(pending))
        if key not in pipes:
            pipes[key] = _make_pipeline(
                model, args, hw, len(pending), test_config['bayes_od_config'], test_config['nms_config'],
                use_full_covar=test_config['use_full_covar'], dataset_name=test_dataset, orig_size=src_hw,
                anchors=gen.generate_all((hw[0], hw[1], 3)), class_parts=want_class, merge_method=merge,
                uncertainty_method=method, blackbox_options=bb_options, acquisition=acq)
        pipe = pipes[key]
        pipe.bind(orig_size=src_hw)      # the handle may be shared with a pipe of another source size: re-apply the KITTI scale
        pipe.engine.upload_frames_u8(frames, constants.MEANS_DICT[handler.im_normalization], aspect_resize=kitti)
        emit(pipe(None, seed=args.seed, first_image_id=pending[0][2]), pipe)

    start, n_done = time.time(), 0
    for idx, sample in enumerate(handler.create_dataset()):
        rgb = datasets.sample_frame(sample)
        name = os.path.splitext(os.path.basename(handler.im_paths[idx]))[0]
        if pending and ((not mixed and pending[0][1].shape != rgb.shape) or len(pending) == args.batch):
            flush()
        pending.append((name, rgb, idx))
        n_done += 1
    flush()
    if writer is not None:
        writer.close()
    log.write()
    print("\nMean frame rate: " + str(n_done / max(time.time() - start, 1e-9)))
    return log.root


def _render_batch(args, tree, names, frames, categories):
    """--render DIR: the batch whose records were just written, drawn on the GPU (one bod_render_frames_u8 call per
    view for the whole batch, mixed sizes included) and written as DIR/<frame>_<view>.png.  The source frames are the host's: a frame
    that travelled as a file for --device_jpeg / --device_png is decoded here by PIL, and --corrupt is not shown."""
    out = getattr(args, 'render', None)
    if not out or not names:
        return
    from . import show_predictions
    view = getattr(args, 'render_view', 'overlay')
    frames = [f.decode() if hasattr(f, 'decode') else np.ascontiguousarray(f, np.uint8) for f in frames]
    show_predictions.render_tree_frames(tree, list(names), frames, ('overlay', 'heat') if view == 'both' else (view,), out,
                                        device=int(args.gpu_device), min_score=float(getattr(args, 'render_min_score', 0.5)),
                                        categories=list(categories))


def _corruption(args):
    """--corrupt NAME:SEVERITY [--corrupt_seed S] -> (chain, seed), or None."""
    spec = getattr(args, 'corrupt', None)
    if not spec:
        return None
    from . import corruptions
    return corruptions.make(*corruptions.parse(spec)), int(getattr(args, 'corrupt_seed', 0) or 0)


def main(argv=None):
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpu_device', type=str, default='0')
    ap.add_argument('--yaml_path', type=str, default=os.path.join(here, 'configs', 'retinanet_bdd_covar.yaml'))
    ap.add_argument('--data_split', type=str, default='test')
    ap.add_argument('--weights', type=str, default=None)
    ap.add_argument('--dataset', action='store_true', help='read the yaml\'s test dataset from disk')
    ap.add_argument('--frames', type=str, default=None)
    ap.add_argument('--synthetic', type=int, default=8)
    ap.add_argument('--image_size', type=int, nargs=2, default=[512, 512])
    ap.add_argument('--orig_size', type=int, nargs=2, default=None)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--mixed_sizes', action='store_true', help='with --dataset: batches in dataset order whatever the frame sizes '
                    '(default: a batch ends where the source size changes)')
    ap.add_argument('--device_jpeg', action='store_true', help='with --dataset: baseline JPEG files are decoded inside the library '
                    '(Huffman decoding on host threads, the rest on the GPU) instead of by PIL; batches as under --mixed_sizes; a batch '
                    'with any other file in it takes the PIL route; the outputs are identical either way')
    ap.add_argument('--device_png', action='store_true', help='with --dataset: 8-bit gray / RGB / RGBA PNG files (KITTI) are decoded '
                    'inside the library (inflate on host threads, the scanline filters on the GPU) instead of by PIL; batches as under '
                    '--mixed_sizes; composes with --device_jpeg; a batch that is not all PNG (or all JPEG) takes the PIL route; the '
                    'outputs are identical either way')
    ap.add_argument('--ensemble', type=str, nargs='+', default=None, help='weight files of an ensemble: every member runs the '
                    'yaml\'s mc_dropout_samples samples and ONE posterior is formed from all of them (overrides --weights)')
    ap.add_argument('--mc_passes', type=int, default=1, help='with --ensemble or --tta_flip: forwards per member (k passes of n '
                    'samples = k * n samples per member; one weight file with --mc_passes k is N = k * n on one handle)')
    ap.add_argument('--tta_flip', action='store_true', help='test-time augmentation: every pass also runs the frames mirrored '
                    'left-right and its samples enter the same posterior (the network width must be a multiple of 2^max_level)')
    ap.add_argument('--covariance_parts', action='store_true', help='also write every detection\'s epistemic, aleatoric and prior '
                    'covariance (cov_epistemic/, cov_aleatoric/, cov_prior/ beside cov/: they sum to it); works with --ensemble, '
                    '--mc_passes and --tta_flip')
    ap.add_argument('--class_uncertainty', action='store_true', help='also write every detection\'s class entropy and its parts '
                    '(class_entropy/<frame>.npy [K,4]: total, aleatoric, epistemic_mc, epistemic_spatial; the last three sum to the '
                    'first) beside cov/; works with --ensemble, --mc_passes, --tta_flip and --covariance_parts; yaml key: '
                    'testing_config.class_uncertainty')
    ap.add_argument('--merge_method', choices=('bayes', 'centre', 'mixture'), default=None, help='how a cluster of kept anchors becomes a '
                    'detection: bayes (default) multiplies the members\' Gaussians; centre reports the centre\'s own posterior, what plain '
                    'NMS would; mixture is the equal-weight Gaussian mixture of the members.  The tree of a non-default method is '
                    'bayes_od_<fusion_method>-<merge_method>; yaml key: testing_config.bayes_od_config.merge_method (the flag wins); not '
                    'with --covariance_parts / --class_uncertainty')
    ap.add_argument('--merge_terms', action='store_true', help='with --merge_method centre / mixture or --uncertainty_method black_box: '
                    'also write merge_within/, merge_between/ ([K,4,4] each; cov = within + between) and merge_members/ ([K]) beside cov/')
    ap.add_argument('--uncertainty_method', choices=UNCERTAINTY_METHODS, default=None, help='bayes_od (default), or black_box: every '
                    'MC sample goes through the ordinary post-processing and NMS on its own, the detection sets are grouped by overlap and '
                    'each group becomes one detection with the sample mean and covariance of its members.  The tree is '
                    'black_box_<fusion_method>, beside the default one; yaml key: testing_config.uncertainty_method (the flag wins); not '
                    'with --covariance_parts, --class_uncertainty, --ensemble, --tta_flip or a non-default --merge_method')
    ap.add_argument('--bb_min_score', type=float, default=None, help='with black_box: sample detections whose top score is below this '
                    'are discarded before pooling (default 0)')
    ap.add_argument('--bb_min_members', type=int, default=None, help='with black_box: a group with fewer members is not reported '
                    '(default 1)')
    ap.add_argument('--corrupt', type=str, default=None, metavar='NAME:SEVERITY', help='with --dataset: corrupt every frame on the '
                    'GPU before preprocessing, to score uncertainty under dataset shift (gaussian_noise, impulse_noise, defocus_blur, '
                    'motion_blur, gaussian_blur, pixelate, jpeg_compression, contrast, brightness, low_light, fog; severity 1..5); '
                    'batches as under --mixed_sizes; works with --device_jpeg, --ensemble, --tta_flip and the parts flags')
    ap.add_argument('--corrupt_seed', type=int, default=0, help='seed of the random corruptions; a frame\'s noise depends on it and '
                    'on the frame\'s dataset index alone')
    ap.add_argument('--render', type=str, default=None, metavar='DIR', help='also draw every batch\'s detections onto its source '
                    'frames on the GPU right after its records are written (boxes, labels and a 2-sigma ellipse on each corner) and '
                    'write DIR/<frame>_<view>.png; the stand-alone tool is python -m bayes_od_rc_amd.show_predictions')
    ap.add_argument('--render_view', choices=('overlay', 'heat', 'both'), default='overlay', help='with --render: the overlay, the '
                    'jet-coloured spatial-probability map, or both')
    ap.add_argument('--render_min_score', type=float, default=0.5, help='with --render: detections below this score are not drawn')
    ap.add_argument('--acquisition', action='store_true', help='active learning: also score every frame by the model\'s uncertainty '
                    'about it, from the per-anchor MC statistics on the GPU, and write acquisition.npz (frames, columns, scores [F,12], '
                    'per_class [F,C-1,3]) into the prediction tree; choose frames from it with python -m bayes_od_rc_amd.select_frames.  '
                    'Runs on statistics handles like --tta_flip; works with --ensemble, --mc_passes, --tta_flip, --corrupt, '
                    '--mixed_sizes, --device_jpeg and --device_png; not with --uncertainty_method black_box or a non-default --merge_method')
    ap.add_argument('--acq_only', action='store_true', help='--acquisition without the posterior, NMS and clustering: acquisition.npz '
                    'is the only output; not with --render, --covariance_parts, --class_uncertainty, --merge_method or --merge_terms')
    ap.add_argument('--acq_min_foreground', type=float, default=None, help='with --acquisition: an anchor counts as foreground when '
                    'its mean background probability is at most 1 - this (default 0.05)')
    ap.add_argument('--acq_top_k', type=int, default=None, help='with --acquisition: mi_topk is the mean of this many largest '
                    'per-anchor mutual informations of a frame (default 16, at most 1024)')
    args = ap.parse_args(argv)
    if args.corrupt:
        if not args.dataset:
            ap.error('--corrupt requires --dataset')
        from . import corruptions
        try:
            corruptions.parse(args.corrupt)
        except ValueError as e:
            ap.error('--corrupt: %s' % e)
    config = config_utils.load_yaml(args.yaml_path)
    config = config_utils.setup(config, args)
    if args.device_jpeg and not args.dataset:
        ap.error('--device_jpeg requires --dataset')
    try:
        check_merge_options(config, args)
        check_uncertainty_options(config, args)
        check_acquisition_options(config, args)
    except ValueError as e:
        ap.error(str(e))
    if args.device_png and not args.dataset:
        ap.error('--device_png requires --dataset')
    try:
        return test_model(config, args)
    except ValueError as e:
        if args.tta_flip and 'mirror-symmetric' in str(e):
            sys.exit(str(e))                  # the library's message for a geometry whose anchors have no mirror partners
        raise


if __name__ == '__main__':
    main()

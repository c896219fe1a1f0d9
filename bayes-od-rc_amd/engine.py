"""Object wrapper over one ``bod_handle`` (include/bayesod.h).  NumPy in / NumPy out.

One Engine = one GPU, one HIP stream, one (image size, batch, MC sample count) geometry.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import BodConfig, BodSizes, as_f32, fptr, iptr

_KINDS = {"kernel": 0, "bias": 1, "gamma": 2, "beta": 3, "mean": 4, "var": 5}
# bod_config.precision (include/bayesod.h): bf16 = throughput path; fp32 = exact-fp32 MFMA; bf16x3 = (hi, lo) bf16 pairs with
# three MFMA products, the 1e-3 end-to-end parity mode on the bf16 matrix pipe
PRECISIONS = {"bf16": 0, "fp32": 1, "bf16x3": 2, "f16mx": 3, "f16mx4": 4}
VIEWS = {"identity": _lib.BOD_VIEW_IDENTITY, "hflip": _lib.BOD_VIEW_HFLIP}      # test-time views of a statistics handle
MERGE_METHODS = _lib.MERGE_METHODS                # how a cluster becomes a detection (bod_set_merge_method)


def merge_method_id(method):
    """'bayes' / 'centre' / 'mixture' -> BOD_MERGE_*; ValueError names the choices for anything else."""
    if not isinstance(method, str) or method not in MERGE_METHODS:
        raise ValueError("merge_method must be one of %s, got %r" % (sorted(MERGE_METHODS), method))
    return MERGE_METHODS[method]


def make_config(image_hw, batch=1, mc_samples=10, num_classes=8, anchors_per_location=9, device=0,
                dropout_rate=0.3, use_full_covar=True, bayes_od_config=None, nms_config=None,
                has_covar_head=True, dataset_name='bdd', orig_size=None, nms_variant='A',
                num_categorical_draws=30, layers=(3, 4, 5, 6, 7), precision='bf16', mc_sample_base=0,
                mc_ensemble_size=0, training=False, backbone_depth=50, pipeline_overlap=False, mc_statistics=False,
                covariance_parts=False, class_parts=False):
    """Translates the reference's yaml dictionaries (configs/retinanet_bdd_covar.yaml:61-143)
    into a ``bod_config``."""
    bo = bayes_od_config or {'ranking_method': 'score', 'dirichlet_prior': {'type': 'non_informative'},
                             'gaussian_prior': {'type': 'isotropic', 'isotropic_variance': 100000.0}}
    nms = nms_config or {'max_output_size': 100, 'iou_threshold': 0.5, 'soft_nms_sigma': 0.5}
    cfg = BodConfig()
    cfg.device = int(device)
    cfg.image_h, cfg.image_w = int(image_hw[0]), int(image_hw[1])
    cfg.batch, cfg.mc_samples = int(batch), int(mc_samples)
    cfg.num_classes = int(num_classes)
    cfg.anchors_per_location = int(anchors_per_location)
    cfg.min_level, cfg.max_level = int(min(layers)), int(max(layers))
    cfg.dropout_rate = float(dropout_rate)
    cfg.use_full_covar = int(bool(use_full_covar))
    cfg.dirichlet_non_informative = int(bo['dirichlet_prior']['type'] == 'non_informative')
    cfg.gaussian_isotropic = int(bo['gaussian_prior']['type'] == 'isotropic')
    cfg.isotropic_variance = float(bo['gaussian_prior'].get('isotropic_variance', 100000.0))
    if bo['ranking_method'] not in ('score', 'joint_entropy'):
        raise ValueError("ranking_method must be 'score' or 'joint_entropy'")
    cfg.ranking_method = int(bo['ranking_method'] == 'joint_entropy')
    cfg.nms_max_output_size = int(nms['max_output_size'])
    cfg.nms_iou_threshold = float(nms['iou_threshold'])
    cfg.nms_soft_sigma = float(nms['soft_nms_sigma'])
    cfg.nms_variant = {'A': 0, 'B': 1}[nms_variant]
    cfg.num_categorical_draws = int(num_categorical_draws)
    cfg.has_covar_head = int(bool(has_covar_head))
    if precision not in PRECISIONS:
        raise ValueError("precision must be one of %s" % (sorted(PRECISIONS),))
    cfg.precision = PRECISIONS[precision]
    cfg.mc_sample_base, cfg.mc_ensemble_size = int(mc_sample_base), int(mc_ensemble_size)
    cfg.training = int(bool(training))
    if int(backbone_depth) not in (50, 101):
        raise ValueError("backbone_depth must be 50 or 101")
    cfg.backbone_depth = int(backbone_depth)
    # infer_async overlaps the front (stem / backbone / FPN) of batch i+1 with the towers of batch i on CU-partitioned streams
    cfg.pipeline_overlap = int(bool(pipeline_overlap))
    # a statistics handle (include/bayesod.h): mergeable MC statistics beside the forward's own -- ensembles, passes, sample shards
    cfg.mc_statistics = int(bool(mc_statistics))
    if cfg.mc_statistics and (cfg.training or cfg.pipeline_overlap):
        raise ValueError("mc_statistics handles are inference handles on one stream: training / pipeline_overlap cannot be combined with it")
    # every posterior row and detection also reports the epistemic / aleatoric / prior terms of its covariance (include/bayesod.h)
    # ... (bit BOD_PARTS_COVARIANCE) and / or the aleatoric / epistemic / spatial parts of its class entropy (bit BOD_PARTS_CLASS)
    cfg.covariance_parts = (_lib.BOD_PARTS_COVARIANCE if covariance_parts else 0) | (_lib.BOD_PARTS_CLASS if class_parts else 0)
    if cfg.covariance_parts and cfg.training:
        raise ValueError("covariance_parts / class_parts belong to inference and statistics handles: training cannot be combined with them")
    if dataset_name == 'kitti':
        if orig_size is None:
            raise ValueError("dataset_name='kitti' needs orig_size (sample_dict['im_size'])")
        cfg.kitti_scale_h = float(orig_size[0]) / float(image_hw[0])
        cfg.kitti_scale_w = float(orig_size[1]) / float(image_hw[1])
    return cfg


class Engine(object):
    def __init__(self, cfg):
        self.lib = _lib.load()
        self.cfg = cfg
        self.h = C.c_void_p()
        st = self.lib.bod_create(C.byref(cfg), C.byref(self.h))
        _lib.check(self.lib, None, st)
        s = BodSizes()
        self._chk(self.lib.bod_query_sizes(self.h, C.byref(s)))
        self.P, self.A = s.num_pixels, s.num_anchors
        self.levels = [(s.level_h[i], s.level_w[i]) for i in range(s.num_levels)]
        self.B, self.N, self.Ccls = cfg.batch, cfg.mc_samples, cfg.num_classes
        self.K = cfg.nms_max_output_size
        self._anchors_set = False

    # ------------------------------------------------------------------ plumbing
    def _chk(self, st):
        _lib.check(self.lib, self.h, st)

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.lib.bod_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def device_bytes(self):
        s = BodSizes()
        self._chk(self.lib.bod_query_sizes(self.h, C.byref(s)))
        return int(s.device_bytes)

    def update_config(self, cfg):
        self._chk(self.lib.bod_update_config(self.h, C.byref(cfg)))
        self.cfg = cfg

    # ------------------------------------------------------------------ weights / anchors
    def load_weights(self, weights):
        """weights: {keras_layer_name: {"kernel"/"bias"/"gamma"/"beta"/"mean"/"var": ndarray}}"""
        for name, entry in weights.items():
            for field, arr in entry.items():
                if arr is None:
                    continue
                a = as_f32(arr)
                shape = (C.c_int64 * a.ndim)(*a.shape)
                self._chk(self.lib.bod_load_weight(self.h, name.encode(), _KINDS[field], shape, a.ndim, fptr(a)))
        self._chk(self.lib.bod_finalize_weights(self.h))

    def set_anchors(self, anchors):
        a = as_f32(anchors)
        self._chk(self.lib.bod_set_anchors(self.h, fptr(a), a.shape[0]))
        self._anchors_set = True

    # ------------------------------------------------------------------ stages
    def _img(self, images):
        a = as_f32(images)
        expect = (self.B, self.cfg.image_h, self.cfg.image_w, 3)
        if a.shape != expect:
            raise ValueError("images must have shape %s, got %s" % (expect, a.shape))
        return a

    def upload_images(self, images):
        a = self._img(images)
        self._chk(self.lib.bod_upload_images(self.h, fptr(a)))

    def upload_frames_u8(self, frames_rgb_u8, means=None, aspect_resize=False):
        """Decoded uint8 RGB frames [B,h,w,3] -> the device image buffer, preprocessed on the device like the
        reference's dataset handlers (mean subtraction, BGR flip; aspect_resize=True adds KITTI's bilinear
        aspect-preserving resize + centred crop/pad).  Then call forward()/infer() with images=None."""
        from . import constants
        a = np.ascontiguousarray(frames_rgb_u8, dtype=np.uint8)
        if a.ndim != 4 or a.shape[0] != self.B or a.shape[3] != 3:
            raise ValueError("expected uint8 frames of shape (%d, h, w, 3), got %s" % (self.B, a.shape))
        m = np.ascontiguousarray(constants.MEANS_DICT['ImageNet'] if means is None else means, dtype=np.float32)
        self._chk(self.lib.bod_upload_frames_u8(self.h, a.ctypes.data_as(C.POINTER(C.c_uint8)), a.shape[1], a.shape[2],
                                                fptr(m), int(bool(aspect_resize))))

    def upload_frames_u8_async(self, frames_rgb_u8, buffer, means=None, aspect_resize=False):
        """Pipelined upload (``bod_upload_frames_u8_async``): copy + preprocessing run on the handle's copy stream into
        image buffer 0/1 and return at once; pass ``image_buffer=buffer`` to forward()/infer()/infer_async().  The array must
        be C-contiguous uint8 (pinned host memory for a truly asynchronous copy) and stay alive until that batch is
        collected."""
        from . import constants
        a = frames_rgb_u8
        if a.dtype != np.uint8 or not a.flags['C_CONTIGUOUS'] or a.ndim != 4 or a.shape[0] != self.B or a.shape[3] != 3:
            raise ValueError("expected C-contiguous uint8 frames of shape (%d, h, w, 3), got %s %s" % (self.B, a.dtype, a.shape))
        m = np.ascontiguousarray(constants.MEANS_DICT['ImageNet'] if means is None else means, dtype=np.float32)
        self._chk(self.lib.bod_upload_frames_u8_async(self.h, a.ctypes.data_as(C.POINTER(C.c_uint8)), a.shape[1], a.shape[2],
                                                      fptr(m), int(bool(aspect_resize)), int(buffer)))

    def upload_frames_u8_ragged(self, frames, means=None, aspect_resize=True):
        """``upload_frames_u8`` for ``batch`` frames of mixed source sizes (``bod_upload_frames_u8_ragged``): ``frames`` is a
        list of uint8 [h,w,3] arrays.  Every frame is resized / padded by its own geometry; on a handle made with
        ``dataset_name='kitti'`` and ``aspect_resize=True`` the next forward on these frames rescales every frame's boxes by that
        frame's own ``orig / net`` factors instead of the handle's ``orig_size``."""
        from . import constants
        buf, sizes = pack_ragged(frames, self.B)
        m = np.ascontiguousarray(constants.MEANS_DICT['ImageNet'] if means is None else means, dtype=np.float32)
        self._chk(self.lib.bod_upload_frames_u8_ragged(self.h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), iptr(sizes), fptr(m),
                                                       int(bool(aspect_resize))))

    def upload_frames_u8_ragged_async(self, frames, buffer, means=None, aspect_resize=True):
        """Pipelined form (``bod_upload_frames_u8_ragged_async``), used like ``upload_frames_u8_async``.  The packed copy of the
        frames is kept alive by the engine until the next upload into the same buffer."""
        from . import constants
        buf, sizes = pack_ragged(frames, self.B)
        m = np.ascontiguousarray(constants.MEANS_DICT['ImageNet'] if means is None else means, dtype=np.float32)
        self._chk(self.lib.bod_upload_frames_u8_ragged_async(self.h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), iptr(sizes), fptr(m),
                                                             int(bool(aspect_resize)), int(buffer)))
        if not hasattr(self, "_ragged_keep"):
            self._ragged_keep = {}
        self._ragged_keep[int(buffer)] = buf

    def upload_frames_u8_augmented(self, frames, aug, means=None, aspect_resize=True):
        """``upload_frames_u8_ragged`` with every frame shown in a form of its own (``bod_upload_frames_u8_augmented``, training
        only): ``aug`` holds one record per frame -- an ``AUGMENT_DTYPE`` array or a list of dicts with its field names, missing
        ones meaning "none" -- as ``draw_augmentation`` returns them.  ``augment_boxes`` maps the ground truth the same way."""
        from . import constants
        buf, sizes = pack_ragged(frames, self.B)
        rec = augment_records(aug, self.B)
        m = np.ascontiguousarray(constants.MEANS_DICT['ImageNet'] if means is None else means, dtype=np.float32)
        self._chk(self.lib.bod_upload_frames_u8_augmented(self.h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), iptr(sizes), fptr(m),
                                                          int(bool(aspect_resize)), rec.ctypes.data_as(C.POINTER(_lib.BodAugment))))

    def upload_frames_u8_augmented_async(self, frames, aug, buffer, means=None, aspect_resize=True):
        """Pipelined form (``bod_upload_frames_u8_augmented_async``), used like ``upload_frames_u8_ragged_async``."""
        from . import constants
        buf, sizes = pack_ragged(frames, self.B)
        rec = augment_records(aug, self.B)
        m = np.ascontiguousarray(constants.MEANS_DICT['ImageNet'] if means is None else means, dtype=np.float32)
        self._chk(self.lib.bod_upload_frames_u8_augmented_async(self.h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), iptr(sizes), fptr(m),
                                                                int(bool(aspect_resize)), rec.ctypes.data_as(C.POINTER(_lib.BodAugment)),
                                                                int(buffer)))
        if not hasattr(self, "_ragged_keep"):
            self._ragged_keep = {}
        self._ragged_keep[int(buffer)] = buf

    def _encoded_upload(self, kind, files, means, aspect_resize, aug, threads, buffer):
        """The JPEG / PNG uploads (``kind``: "jpeg" or "png"), synchronous (``buffer=None``) or pipelined."""
        from . import constants
        ptrs, lens = _encoded_files(files, self.B, kind.upper())
        m = np.ascontiguousarray(constants.MEANS_DICT['ImageNet'] if means is None else means, dtype=np.float32)
        rec = None if aug is None else augment_records(aug, self.B)
        recp = None if rec is None else rec.ctypes.data_as(C.POINTER(_lib.BodAugment))
        src_hw = np.zeros((self.B, 2), np.int32)
        threads = min(16, self.B) if threads is None else int(threads)
        args = (self.h, ptrs, lens, fptr(m), int(bool(aspect_resize)), recp, threads, iptr(src_hw))
        if buffer is None:
            st = getattr(self.lib, "bod_upload_frames_%s" % kind)(*args)
        else:
            st = getattr(self.lib, "bod_upload_frames_%s_async" % kind)(*args, int(buffer))
        self._chk(st)
        return src_hw

    def upload_frames_jpeg(self, files, means=None, aspect_resize=True, aug=None, threads=None):
        """``upload_frames_u8_ragged`` (``aug=None``) or ``upload_frames_u8_augmented`` of JPEG files decoded inside the library
        (``bod_upload_frames_jpeg``): ``files`` is a list of ``batch`` ``bytes`` objects, each a baseline JPEG file.
        The Huffman decoding runs on ``threads`` host threads outside the GIL (default ``min(16, batch)``), the rest on the device;
        the image buffer ends up bit for bit as after the upload of PIL's ``convert('RGB')`` decode of the files.  Returns the
        frames' sizes, int32 [batch, 2] (h, w).  ``ValueError`` naming the frame for a corrupt or unsupported file
        (``jpeg_info`` tells in advance); the handle and the frames it held stay as they were."""
        return self._encoded_upload("jpeg", files, means, aspect_resize, aug, threads, None)

    def upload_frames_jpeg_async(self, files, buffer, means=None, aspect_resize=True, aug=None, threads=None):
        """Pipelined form (``bod_upload_frames_jpeg_async``), used like ``upload_frames_u8_ragged_async``.  The host decode is
        done when this returns: ``files`` need not be kept."""
        return self._encoded_upload("jpeg", files, means, aspect_resize, aug, threads, int(buffer))

    def set_upload_corruption(self, chains, frame_ids=None, seed=0, ops_arrays=None):
        """Corrupt the frames of the NEXT packed upload on the device (``bod_set_upload_corruption``): ``chains``
        is one ``corruptions.Chain`` for the whole batch or a list of one per frame, ``frame_ids`` [batch] the ids the random ops
        key their numbers on (default 0, 1, ..).  One-shot: the next ``upload_frames_u8_ragged[_async]``,
        ``upload_frames_u8_augmented[_async]`` or ``upload_frames_jpeg[_async]`` consumes it; the image buffer ends up bit for bit
        as after the upload of ``corrupt_frames(...)``'s output.  ``None`` clears a pending one; ``ops_arrays`` gives
        already packed (ops, taps, luts, qtables) arrays instead of chains.  A uniform ``upload_frames_u8``
        with one pending raises ``ValueError`` and leaves it pending."""
        if chains is None and ops_arrays is None:
            self._chk(self.lib.bod_set_upload_corruption(self.h, None, 0, None, None, 0, None, 0, None, 0, 0))
            return
        args, _keep = _corruption_args(chains, self.B, frame_ids, ops_arrays)
        self._chk(self.lib.bod_set_upload_corruption(self.h, *args, int(seed) & 0xFFFFFFFFFFFFFFFF))

    def upload_frames_png(self, files, means=None, aspect_resize=True, aug=None, threads=None):
        """``upload_frames_u8_ragged`` (``aug=None``) or ``upload_frames_u8_augmented`` of PNG files decoded inside the library
        (``bod_upload_frames_png``): ``files`` is a list of ``batch`` ``bytes`` objects, each an 8-bit gray, RGB,
        gray + alpha or RGBA PNG file without interlacing.  The inflate runs on ``threads`` host threads outside the GIL (default
        ``min(16, batch)``), the scanline filters on the device; the image buffer ends up bit for bit as after the upload of PIL's
        ``convert('RGB')`` decode of the files.  Returns the frames' sizes, int32 [batch, 2] (h, w).  ``ValueError`` naming the
        frame for a corrupt or unsupported file (``png_info`` tells in advance); the handle and the frames it held stay as they
        were."""
        return self._encoded_upload("png", files, means, aspect_resize, aug, threads, None)

    def upload_frames_png_async(self, files, buffer, means=None, aspect_resize=True, aug=None, threads=None):
        """Pipelined form (``bod_upload_frames_png_async``), used like ``upload_frames_u8_ragged_async``.  The host inflate is
        done when this returns: ``files`` need not be kept."""
        return self._encoded_upload("png", files, means, aspect_resize, aug, threads, int(buffer))

    def _device_images(self, image_buffer):
        ptr = self.lib.bod_device_images(self.h) if image_buffer is None else self.lib.bod_device_images_buffer(self.h, int(image_buffer))
        if not ptr:
            raise ValueError("image buffer %r has not been filled" % (image_buffer,))
        return ptr

    def get_images(self, image_buffer=None):
        """The device image buffer [B,H,W,3] float32 (normalised BGR) copied to the host; ``image_buffer`` 0 / 1: that buffer of
        the pipelined uploads, once its upload has completed (``synchronize()``)."""
        import torch
        from .distributed import DeviceArray
        ptr = self._device_images(image_buffer)
        t = torch.as_tensor(DeviceArray(ptr, (self.B, self.cfg.image_h, self.cfg.image_w, 3), "<f4"),
                            device=torch.device("cuda", self.cfg.device))
        return t.cpu().numpy()

    def forward(self, images=None, seed=0, first_image_id=0, image_buffer=None):
        """images=None => use the device-resident buffer filled by upload_images() (or buffer `image_buffer` of
        upload_frames_u8_async)."""
        if images is None:
            ptr = self._device_images(image_buffer)
            self._chk(self.lib.bod_forward(self.h, ptr, 1, seed, first_image_id))
        else:
            a = self._img(images)
            self._chk(self.lib.bod_forward(self.h, a.ctypes.data, 0, seed, first_image_id))

    def infer(self, images=None, seed=0, first_image_id=0, image_buffer=None):
        if images is None:
            ptr = self._device_images(image_buffer)
            self._chk(self.lib.bod_infer(self.h, ptr, 1, seed, first_image_id))
        else:
            a = self._img(images)
            self._chk(self.lib.bod_infer(self.h, a.ctypes.data, 0, seed, first_image_id))

    def infer_async(self, images=None, seed=0, first_image_id=0, image_buffer=None):
        """Enqueue a whole pass; returns the slot ticket for collect()."""
        slot = C.c_int32(-1)
        if images is None:
            ptr = self._device_images(image_buffer)
            self._chk(self.lib.bod_infer_async(self.h, ptr, 1, seed, first_image_id, C.byref(slot)))
        else:
            a = self._img(images)
            self._chk(self.lib.bod_infer_async(self.h, a.ctypes.data, 0, seed, first_image_id, C.byref(slot)))
        return slot.value

    def collect(self, slot, out=None):
        b, k, c = self.B, self.K, self.Ccls
        if out is None:
            out = {"num": np.empty(b, np.int32), "scores": np.empty((b, k, c), np.float32),
                   "means": np.empty((b, k, 4), np.float32), "covs": np.empty((b, k, 4, 4), np.float32),
                   "counts": np.empty((b, k, c), np.float32)}
        if self.cfg.covariance_parts & _lib.BOD_PARTS_CLASS:
            if "class_parts" not in out:
                out["class_parts"] = np.empty((b, k, 4), np.float32)
            self._chk(self.lib.bod_collect_class_parts(self.h, slot, fptr(out["class_parts"])))
        if self.cfg.covariance_parts & _lib.BOD_PARTS_COVARIANCE:      # (before bod_collect: the parts wait for the batch, the records release the slot)
            if "cov_parts" not in out:
                out["cov_parts"] = np.empty((b, k, 3, 4, 4), np.float32)
            self._chk(self.lib.bod_collect_parts(self.h, slot, fptr(out["cov_parts"])))
        self._chk(self.lib.bod_collect(self.h, slot, iptr(out["num"]), fptr(out["scores"]), fptr(out["means"]),
                                       fptr(out["covs"]), fptr(out["counts"])))
        return out

    def synchronize(self):
        self._chk(self.lib.bod_synchronize(self.h))

    def get_raw(self):
        n = (self.B, self.N, self.A)
        cls = np.empty(n + (self.Ccls,), np.float32)
        box = np.empty(n + (4,), np.float32)
        cov = np.empty(n + (10,), np.float32) if self.cfg.has_covar_head else None
        self._chk(self.lib.bod_get_raw(self.h, fptr(cls), fptr(box), fptr(cov)))
        return cls, box, cov

    def set_raw(self, cls, box, cov=None):
        cls, box = as_f32(cls), as_f32(box)
        cov = as_f32(cov) if cov is not None else None
        n = (self.B, self.N, self.A)
        if cls.shape != n + (self.Ccls,) or box.shape != n + (4,) or (cov is not None and cov.shape != n + (10,)):
            raise ValueError("raw head outputs have the wrong shape")
        self._chk(self.lib.bod_set_raw(self.h, fptr(cls), fptr(box), fptr(cov)))

    def get_pyramid(self, level_index):
        h, w = self.levels[level_index]
        out = np.empty((self.B, h, w, 256), np.float32)
        self._chk(self.lib.bod_get_pyramid(self.h, level_index, fptr(out)))
        return out

    def posterior(self, seed=0, first_image_id=0):
        self._chk(self.lib.bod_posterior(self.h, seed, first_image_id))

    # -- options of the proper-scoring-rule losses -------------------------------
    def set_loss_options(self, energy_samples=None, seed=None, first_image_id=None, one_image_id=None):
        """``bod_set_loss_options``: M of 'regression_energy' (reg_kind 5) for every entry of this handle; ``seed``,
        ``first_image_id`` and ``one_image_id`` (every frame of a call is image ``first_image_id`` itself, so a frame's loss
        is the one it has alone) key its normals in validation_losses_boxes / validate_boxes (a training step takes its own).
        An argument left at None keeps the handle's value (initially 64, 0, 0, False).  A sample count outside [2, 1024] is a
        ValueError and changes nothing."""
        cur = dict(getattr(self, "_loss_options", {"energy_samples": 64, "seed": 0, "first_image_id": 0, "one_image_id": False}))
        for k, v in (("energy_samples", energy_samples), ("seed", seed), ("first_image_id", first_image_id), ("one_image_id", one_image_id)):
            if v is not None:
                cur[k] = v
        self._chk(self.lib.bod_set_loss_options(self.h, C.byref(_lib.loss_options(**cur))))
        self._loss_options = cur

    # -- training ------------------------------------------------------
    def train_step(self, images, cls_targets, box_targets, positive_mask, negative_mask, seed=0, first_image_id=0,
                   reg_kind=3, label_smoothing=0.001, w_cls=5.0, w_reg=1.0, l2_rate=1e-6, learning_rate=1e-3,
                   apply_update=True, energy_samples=None):
        """run_training.train_single_step on a handle made with make_config(training=True): returns a dict with
        total_loss, cls_loss, reg_loss, covariance_loss, regularization_loss and the global gradient norm.
        ``energy_samples``: set_loss_options(energy_samples) first (reg_kind 5; None keeps the handle's)."""
        if energy_samples is not None:
            self.set_loss_options(energy_samples)
        b, a = self.B, self.A
        ct = as_f32(cls_targets).reshape(b, a, self.Ccls)
        bt = as_f32(box_targets).reshape(b, a, 4)
        pm = np.ascontiguousarray(np.asarray(positive_mask).reshape(b, a), dtype=np.uint8)
        nm = np.ascontiguousarray(np.asarray(negative_mask).reshape(b, a), dtype=np.uint8)
        out = (C.c_double * 6)()
        u8 = C.POINTER(C.c_uint8)
        if images is None:
            ptr, on_dev = self.lib.bod_device_images(self.h), 1
        else:
            img = self._img(images)
            ptr, on_dev = img.ctypes.data, 0
        self._chk(self.lib.bod_train_step(self.h, ptr, on_dev, fptr(ct), fptr(bt), pm.ctypes.data_as(u8), nm.ctypes.data_as(u8),
                                          seed, first_image_id, int(reg_kind), float(label_smoothing), float(w_cls), float(w_reg),
                                          float(l2_rate), float(learning_rate), int(bool(apply_update)), out))
        keys = ("total_loss", "cls_loss", "reg_loss", "covariance_loss", "regularization_loss", "grad_norm")
        return dict(zip(keys, [out[i] for i in range(6)]))

    def train_step_boxes(self, images, gt_boxes, gt_classes, min_positive_iou=0.5, max_negative_iou=0.4, seed=0, first_image_id=0,
                         reg_kind=3, label_smoothing=0.001, w_cls=5.0, w_reg=1.0, l2_rate=1e-6, learning_rate=1e-3,
                         apply_update=True, energy_samples=None):
        """train_step from ground-truth boxes (``bod_train_step_boxes``): per-frame lists of [G_b,4] corners (y1,x1,y2,x2)
        and [G_b,C] class rows; the dense targets are assigned on the device against the handle's anchors."""
        if energy_samples is not None:
            self.set_loss_options(energy_samples)
        ng, boxes, classes = _pack_gt(gt_boxes, gt_classes, self.B, self.Ccls)
        out = (C.c_double * 6)()
        if images is None:
            ptr, on_dev = self.lib.bod_device_images(self.h), 1
        else:
            img = self._img(images)
            ptr, on_dev = img.ctypes.data, 0
        self._chk(self.lib.bod_train_step_boxes(self.h, ptr, on_dev, iptr(ng), fptr(boxes), fptr(classes), float(min_positive_iou),
                                                float(max_negative_iou), seed, first_image_id, int(reg_kind), float(label_smoothing),
                                                float(w_cls), float(w_reg), float(l2_rate), float(learning_rate),
                                                int(bool(apply_update)), out))
        keys = ("total_loss", "cls_loss", "reg_loss", "covariance_loss", "regularization_loss", "grad_norm")
        return dict(zip(keys, [out[i] for i in range(6)]))

    def train_targets(self):
        """The dense targets the last training step used (``bod_train_get_targets``): cls [B,A,C], box [B,A,4], positive and
        negative masks [B,A] (bool)."""
        b, a = self.B, self.A
        ct, bt = np.empty((b, a, self.Ccls), np.float32), np.empty((b, a, 4), np.float32)
        pm, nm = np.empty((b, a), np.uint8), np.empty((b, a), np.uint8)
        u8 = C.POINTER(C.c_uint8)
        self._chk(self.lib.bod_train_get_targets(self.h, fptr(ct), fptr(bt), pm.ctypes.data_as(u8), nm.ctypes.data_as(u8)))
        return ct, bt, pm.astype(bool), nm.astype(bool)

    def train_gradients_view(self):
        """torch tensor aliasing the contiguous fp32 gradient arena (for the data-parallel all-reduce)."""
        import torch
        from .distributed import DeviceArray
        ptr, n = C.c_void_p(), C.c_int64()
        self._chk(self.lib.bod_train_gradients(self.h, C.byref(ptr), C.byref(n)))
        return torch.as_tensor(DeviceArray(ptr.value, (n.value,), "<f4"), device=torch.device("cuda", self.cfg.device))

    def train_apply(self, learning_rate):
        """Clip + Adam on the gradient arena's current contents; returns the global gradient norm."""
        g = C.c_double()
        self._chk(self.lib.bod_train_apply(self.h, float(learning_rate), C.byref(g)))
        return g.value

    def train_get(self, layer, kind, shape, what="value"):
        """A trainable tensor (kind: 'kernel' | 'bias' | 'gamma' | 'beta') or its gradient / Adam moments."""
        kinds = {"kernel": 0, "bias": 1, "gamma": 2, "beta": 3}
        whats = {"value": 0, "grad": 1, "adam_m": 2, "adam_v": 3}
        out = np.empty(shape, np.float32)
        self._chk(self.lib.bod_train_get(self.h, layer.encode(), kinds[kind], whats[what], fptr(out), out.size))
        return out

    def train_set_moment(self, layer, kind, what, value):
        """Restore an Adam moment (what: 'adam_m' | 'adam_v') of a trainable tensor (checkpoint resume)."""
        kinds = {"kernel": 0, "bias": 1, "gamma": 2, "beta": 3}
        whats = {"adam_m": 2, "adam_v": 3}
        a = as_f32(value)
        self._chk(self.lib.bod_train_set(self.h, layer.encode(), kinds[kind], whats[what], fptr(a), a.size))

    def train_step_count(self, set_to=None):
        """Number of optimizer updates applied (enters Adam's bias correction); ``set_to`` restores it."""
        got = C.c_int64(0)
        self._chk(self.lib.bod_train_step_count(self.h, C.byref(got), -1 if set_to is None else int(set_to)))
        return int(got.value)

    def validation_post(self):
        """validation_utils.post_process_predictions up to the NMS input (softmax, background filter, ranking)."""
        self._chk(self.lib.bod_validation_post(self.h))

    # -- validation from ground-truth boxes (run_validation.py:230-260 + validation_utils.py:10-77) -------------
    def _chk_val(self, st):
        """Status of a validation entry point: a stage-order violation (no anchors, no forward, no NMS yet) is a RuntimeError,
        a refused argument or handle a ValueError."""
        if st == _lib.BOD_ERR_NOT_READY:
            msg = self.lib.bod_last_error(self.h)
            raise RuntimeError(msg.decode() if msg else "not ready")
        self._chk(st)

    def validation_losses_boxes(self, gt_boxes, gt_classes, min_positive_iou=0.5, max_negative_iou=0.4, do_classification=True,
                                reg_kind=3, label_smoothing=0.001, loss_options=None):
        """Per-frame loss sums of the handle's current raw outputs (``bod_validation_losses_boxes``): [B,4] float64 rows
        (sum of masked focal terms, sum of positive regression terms, sum of positive 0.5 sum(log D) terms, positives).
        Ground truth as in train_step_boxes; the dense targets are assigned on the device.  ``loss_options``: keyword
        arguments of set_loss_options, applied first (reg_kind 5)."""
        if loss_options is not None:
            self.set_loss_options(**loss_options)
        ng, boxes, classes = _pack_gt(gt_boxes, gt_classes, self.B, self.Ccls)
        sums = np.empty((self.B, 4), np.float64)
        self._chk_val(self.lib.bod_validation_losses_boxes(self.h, iptr(ng), fptr(boxes), fptr(classes), float(min_positive_iou),
                                                           float(max_negative_iou), int(bool(do_classification)), int(reg_kind),
                                                           float(label_smoothing), _lib.dptr(sums)))
        return sums

    def _val_records(self, num, scores, corners):
        return [(scores[b, :num[b]].copy(), corners[b, :num[b]].copy()) for b in range(self.B)]

    def validation_detections_batch(self):
        """After validation_post() + nms(): per image (class rows [K,C], corners [K,4] as y1, x1, y2, x2 in network pixels) of
        the selected candidates in soft-NMS order, gathered on the device (``bod_get_validation_detections_batch``)."""
        num = np.empty(self.B, np.int32)
        scores, corners = np.empty((self.B, self.K, self.Ccls), np.float32), np.empty((self.B, self.K, 4), np.float32)
        self._chk_val(self.lib.bod_get_validation_detections_batch(self.h, iptr(num), fptr(scores), fptr(corners)))
        return self._val_records(num, scores, corners)

    def validate_boxes(self, images, gt_boxes, gt_classes, min_positive_iou=0.5, max_negative_iou=0.4, do_classification=True,
                       reg_kind=3, label_smoothing=0.001, loss_options=None):
        """The validation loop body for a batch (``bod_validate_boxes``): forward, per-frame loss sums, validation post,
        soft-NMS, record gather.  images=None uses the frames uploaded with upload_frames_u8 / upload_images.  Returns
        (sums [B,4] float64, [(class rows [K,C], corners [K,4])] per image).  ``loss_options`` as in validation_losses_boxes."""
        if loss_options is not None:
            self.set_loss_options(**loss_options)
        ng, boxes, classes = _pack_gt(gt_boxes, gt_classes, self.B, self.Ccls)
        if images is None:
            ptr, on_dev = self.lib.bod_device_images(self.h), 1
        else:
            img = self._img(images)
            ptr, on_dev = img.ctypes.data, 0
        sums, num = np.empty((self.B, 4), np.float64), np.empty(self.B, np.int32)
        scores, corners = np.empty((self.B, self.K, self.Ccls), np.float32), np.empty((self.B, self.K, 4), np.float32)
        self._chk_val(self.lib.bod_validate_boxes(self.h, ptr, on_dev, iptr(ng), fptr(boxes), fptr(classes), float(min_positive_iou),
                                                  float(max_negative_iou), int(bool(do_classification)), int(reg_kind),
                                                  float(label_smoothing), _lib.dptr(sums), iptr(num), fptr(scores), fptr(corners)))
        return sums, self._val_records(num, scores, corners)

    def num_kept(self):
        out = np.zeros(self.B, np.int32)
        self._chk(self.lib.bod_get_num_kept(self.h, iptr(out)))
        return out

    def get_posterior(self, image_index=0):
        m = int(self.num_kept()[image_index])
        counts = np.empty((m, self.Ccls), np.float32)
        score = np.empty((m, self.Ccls), np.float32)
        means = np.empty((m, 4), np.float32)
        covs = np.empty((m, 4, 4), np.float32)
        ranking = np.empty((m,), np.float32)
        aidx = np.empty((m,), np.int32)
        self._chk(self.lib.bod_get_posterior(self.h, image_index, fptr(counts), fptr(score), fptr(means),
                                             fptr(covs), fptr(ranking), iptr(aidx)))
        return {"counts": counts, "score": score, "means": means, "covs": covs, "ranking": ranking,
                "anchor_index": aidx}

    def set_posterior(self, image_index, counts, means, covs, ranking):
        counts, means, covs, ranking = as_f32(counts), as_f32(means).reshape(-1, 4), as_f32(covs), as_f32(ranking)
        m = means.shape[0]
        self._chk(self.lib.bod_set_posterior(self.h, image_index, m, fptr(counts), fptr(means), fptr(covs),
                                             fptr(ranking)))

    # -- covariance parts (handles made with make_config(covariance_parts=True)): [rows, 3, 4, 4] = epistemic, aleatoric, prior
    def get_posterior_parts(self, image_index=0):
        """The three terms every row of ``get_posterior(image_index)["covs"]`` is the sum of (``bod_get_posterior_parts``)."""
        m = int(self.num_kept()[image_index])
        parts = np.empty((m, 3, 4, 4), np.float32)
        self._chk(self.lib.bod_get_posterior_parts(self.h, image_index, fptr(parts)))
        return parts

    def set_posterior_parts(self, image_index, parts):
        """The injection that goes with ``set_posterior``: ``parts`` [M,3,4,4] (``bod_set_posterior_parts``)."""
        parts = as_f32(parts).reshape(-1, 3, 4, 4)
        self._chk(self.lib.bod_set_posterior_parts(self.h, image_index, parts.shape[0], fptr(parts)))

    def get_detection_parts(self, image_index=0):
        """[K,3,4,4]: the three terms of every covariance of ``get_detections(image_index)`` (``bod_get_detection_parts``)."""
        parts = np.empty((self.K, 3, 4, 4), np.float32)
        n = C.c_int32(0)
        self._chk(self.lib.bod_get_detection_parts(self.h, image_index, fptr(parts)))
        self._chk(self.lib.bod_get_detections(self.h, image_index, C.byref(n), None, None, None, None))
        return parts[:n.value].copy()

    def get_detection_parts_batch(self):
        """[B,K,3,4,4], padded like ``get_detections_batch`` (``bod_get_detection_parts_batch``)."""
        parts = np.empty((self.B, self.K, 3, 4, 4), np.float32)
        self._chk(self.lib.bod_get_detection_parts_batch(self.h, fptr(parts)))
        return parts

    def device_detection_parts_pointer(self, slot=0):
        p = C.c_void_p(0)
        self._chk(self.lib.bod_device_detection_parts(self.h, slot, C.byref(p)))
        return int(p.value or 0), (self.B, self.K, 3, 16)

    # -- class-entropy parts (handles made with make_config(class_parts=True); include/bayesod.h)
    @property
    def has_cov_parts(self):
        return bool(self.cfg.covariance_parts & _lib.BOD_PARTS_COVARIANCE)

    @property
    def has_class_parts(self):
        return bool(self.cfg.covariance_parts & _lib.BOD_PARTS_CLASS)

    def get_posterior_class_parts(self, image_index=0):
        """[M,3] = total, aleatoric, epistemic entropy of the MC class distribution of every row of ``get_posterior(image_index)``
        (``bod_get_posterior_class_parts``)."""
        m = int(self.num_kept()[image_index])
        rows = np.empty((m, 3), np.float32)
        self._chk(self.lib.bod_get_posterior_class_parts(self.h, image_index, fptr(rows)))
        return rows

    def get_posterior_mean_probs(self, image_index=0):
        """[M,C]: the mean over the MC samples of softmax(class logits) of every row of ``get_posterior(image_index)`` -- the
        distribution the class parts decompose (``bod_get_posterior_mean_probs``)."""
        m = int(self.num_kept()[image_index])
        p = np.empty((m, self.Ccls), np.float32)
        self._chk(self.lib.bod_get_posterior_mean_probs(self.h, image_index, fptr(p)))
        return p

    def set_posterior_class_parts(self, image_index, mean_probs, rows):
        """The injection that goes with ``set_posterior``: ``mean_probs`` [M,C] and ``rows`` [M,3] (``bod_set_posterior_class_parts``)."""
        mean_probs = as_f32(mean_probs).reshape(-1, self.Ccls)
        rows = as_f32(rows).reshape(-1, 3)
        if rows.shape[0] != mean_probs.shape[0]:
            raise ValueError("mean_probs has %d rows, rows has %d" % (mean_probs.shape[0], rows.shape[0]))
        self._chk(self.lib.bod_set_posterior_class_parts(self.h, image_index, rows.shape[0], fptr(mean_probs), fptr(rows)))

    def get_detection_class_parts(self, image_index=0):
        """[K,4] = total, aleatoric, epistemic_mc, epistemic_spatial of every detection of ``get_detections(image_index)``
        (``bod_get_detection_class_parts``); the last three sum to the first."""
        rows = np.empty((self.K, 4), np.float32)
        n = C.c_int32(0)
        self._chk(self.lib.bod_get_detection_class_parts(self.h, image_index, fptr(rows)))
        self._chk(self.lib.bod_get_detections(self.h, image_index, C.byref(n), None, None, None, None))
        return rows[:n.value].copy()

    def get_detection_class_parts_batch(self):
        """[B,K,4], padded with zero rows like ``get_detections_batch`` (``bod_get_detection_class_parts_batch``)."""
        rows = np.empty((self.B, self.K, 4), np.float32)
        self._chk(self.lib.bod_get_detection_class_parts_batch(self.h, fptr(rows)))
        return rows

    def device_detection_class_parts_pointer(self, slot=0):
        p = C.c_void_p(0)
        self._chk(self.lib.bod_device_detection_class_parts(self.h, slot, C.byref(p)))
        return int(p.value or 0), (self.B, self.K, 4)

    def nms(self):
        self._chk(self.lib.bod_nms(self.h))

    def get_nms(self, image_index=0):
        idx = np.zeros(self.K, np.int32)
        n = C.c_int32(0)
        self._chk(self.lib.bod_get_nms(self.h, image_index, iptr(idx), C.byref(n)))
        return idx[:n.value].copy()

    def _set_centres(self, image_index, centres):
        c = np.ascontiguousarray(centres, dtype=np.int32)
        self._chk(self.lib.bod_set_nms(self.h, image_index, iptr(c), c.shape[0]))

    def set_affinity(self, image_index, centre_columns):
        """centre_columns [K,M]: affinity_matrix[:, centre_k] for every cluster centre (one-shot, next cluster_fuse)."""
        c = as_f32(centre_columns)
        self._chk(self.lib.bod_set_affinity(self.h, image_index, fptr(c), c.shape[0], c.shape[1]))

    def get_iou_matrix(self, image_index=0):
        m = int(self.num_kept()[image_index])
        out = np.empty((m, m), np.float32)
        if m:
            self._chk(self.lib.bod_get_iou_matrix(self.h, image_index, fptr(out)))
        return out

    def cluster_fuse(self):
        self._chk(self.lib.bod_cluster_fuse(self.h))

    # -- how a cluster becomes a detection (include/bayesod.h, bod_set_merge_method) ----------
    def set_merge_method(self, method):
        """'bayes' (the default: the Bayesian fuse), 'centre' (the NMS pick: the centre's own posterior) or 'mixture' (the
        equal-weight Gaussian mixture of the members), for the next cluster_fuse / infer / infer_async (``bod_set_merge_method``)."""
        self._chk(self.lib.bod_set_merge_method(self.h, merge_method_id(method)))

    @property
    def merge_method(self):
        m = C.c_int32(0)
        self._chk(self.lib.bod_get_merge_method(self.h, C.byref(m)))
        return {v: k for k, v in _lib.MERGE_METHODS.items()}[int(m.value)]

    def get_detection_merge_terms(self, image_index=0):
        """(within [K,4,4], between [K,4,4], members [K]) of every detection of ``get_detections(image_index)`` after a 'centre' or
        'mixture' cluster stage; covs = within + between (``bod_get_detection_merge_terms``)."""
        within = np.empty((self.K, 4, 4), np.float32)
        between = np.empty((self.K, 4, 4), np.float32)
        members = np.empty(self.K, np.int32)
        n = C.c_int32(0)
        self._chk(self.lib.bod_get_detection_merge_terms(self.h, image_index, fptr(within), fptr(between), iptr(members)))
        self._chk(self.lib.bod_get_detections(self.h, image_index, C.byref(n), None, None, None, None))
        n = n.value
        return within[:n].copy(), between[:n].copy(), members[:n].copy()

    def get_detection_merge_terms_batch(self, slot=-1):
        """{'within' [B,K,4,4], 'between' [B,K,4,4], 'members' [B,K]}, padded with zero rows like ``get_detections_batch``;
        ``slot``: a ticket of ``infer_async`` (waits for that batch), -1 after a synchronous call
        (``bod_get_detection_merge_terms_batch``)."""
        out = {"within": np.empty((self.B, self.K, 4, 4), np.float32), "between": np.empty((self.B, self.K, 4, 4), np.float32),
               "members": np.empty((self.B, self.K), np.int32)}
        self._chk(self.lib.bod_get_detection_merge_terms_batch(self.h, int(slot), fptr(out["within"]), fptr(out["between"]),
                                                               iptr(out["members"])))
        return out

    def device_detection_merge_terms_pointers(self, slot=0):
        ptrs = (C.c_void_p * 3)()
        self._chk(self.lib.bod_device_detection_merge_terms(self.h, slot, ptrs))
        shapes = [(self.B, self.K, 16), (self.B, self.K, 16), (self.B, self.K)]
        return {n: (int(p or 0), s) for n, p, s in zip(("within", "between", "members"), ptrs, shapes)}

    # -- black-box MC dropout: per-sample NMS, then the detections merged (include/bayesod.h) ----------
    def set_uncertainty_method(self, method, min_score=0.0, min_members=1, affinity_threshold=0.0):
        """'bayes_od' (the default) or 'black_box': every MC sample through the validation post-process and the soft-NMS on its own,
        the image's detection sets pooled, grouped by overlap and merged to their sample mean and covariance, for the next
        infer / infer_async (``bod_set_uncertainty_method``).  The three options belong to 'black_box'."""
        if method not in _lib.UNCERTAINTY_METHODS:
            raise ValueError("uncertainty_method must be one of %s, got %r" % (sorted(_lib.UNCERTAINTY_METHODS), method))
        opt = _lib.BodBlackBoxOptions(float(min_score), int(min_members), float(affinity_threshold), 0)
        self._chk(self.lib.bod_set_uncertainty_method(self.h, _lib.UNCERTAINTY_METHODS[method], C.byref(opt)))

    @property
    def uncertainty_method(self):
        m = C.c_int32(0)
        self._chk(self.lib.bod_get_uncertainty_method(self.h, C.byref(m)))
        return {v: k for k, v in _lib.UNCERTAINTY_METHODS.items()}[int(m.value)]

    def blackbox_samples(self):
        """Stage 1 on the last forward's (or ``set_raw``'s) head outputs (``bod_blackbox_samples``)."""
        self._chk(self.lib.bod_blackbox_samples(self.h))

    def blackbox_merge(self):
        """Stage 2: the pooled sample detections merged into detections; ``get_detections`` / ``get_detection_merge_terms`` follow
        (``bod_blackbox_merge``)."""
        self._chk(self.lib.bod_blackbox_merge(self.h))

    def get_sample_detections(self, image_index=0, sample_index=0):
        """{'anchor_index' [k], 'scores' [k,C], 'means' [k,4], 'covs' [k,4,4]} of one (image, MC sample)
        (``bod_get_sample_detections``)."""
        k = self.K
        idx = np.empty(k, np.int32)
        scores = np.empty((k, self.Ccls), np.float32)
        means = np.empty((k, 4), np.float32)
        covs = np.empty((k, 4, 4), np.float32)
        n = C.c_int32(0)
        self._chk(self.lib.bod_get_sample_detections(self.h, image_index, sample_index, C.byref(n), iptr(idx), fptr(scores),
                                                     fptr(means), fptr(covs)))
        n = n.value
        return {"anchor_index": idx[:n].copy(), "scores": scores[:n].copy(), "means": means[:n].copy(), "covs": covs[:n].copy()}

    def set_sample_detections(self, image_index, sample_index, scores, means, covs, anchor_index=None):
        """Replace the sample detections of one (image, MC sample); the others stay (``bod_set_sample_detections``)."""
        scores = as_f32(scores).reshape(-1, self.Ccls)
        means = as_f32(means).reshape(-1, 4)
        covs = as_f32(covs).reshape(-1, 16)
        k = scores.shape[0]
        if means.shape[0] != k or covs.shape[0] != k:
            raise ValueError("scores, means and covs must have the same number of rows")
        idx = None if anchor_index is None else np.ascontiguousarray(anchor_index, dtype=np.int32)
        if idx is not None and idx.shape != (k,):
            raise ValueError("anchor_index must have one entry per row")
        self._chk(self.lib.bod_set_sample_detections(self.h, image_index, sample_index, k, iptr(idx), fptr(scores), fptr(means),
                                                     fptr(covs)))

    def get_detections(self, image_index=0):
        k = self.K
        scores = np.empty((k, self.Ccls), np.float32)
        means = np.empty((k, 4), np.float32)
        covs = np.empty((k, 4, 4), np.float32)
        counts = np.empty((k, self.Ccls), np.float32)
        n = C.c_int32(0)
        self._chk(self.lib.bod_get_detections(self.h, image_index, C.byref(n), fptr(scores), fptr(means),
                                              fptr(covs), fptr(counts)))
        n = n.value
        return scores[:n].copy(), means[:n].copy(), covs[:n].copy(), counts[:n].copy()

    def get_detections_batch(self, out=None):
        """One D2H per array for the whole batch. Returns dict of padded arrays + 'num' [B]."""
        b, k, c = self.B, self.K, self.Ccls
        if out is None:
            out = {"num": np.empty(b, np.int32), "scores": np.empty((b, k, c), np.float32),
                   "means": np.empty((b, k, 4), np.float32), "covs": np.empty((b, k, 4, 4), np.float32),
                   "counts": np.empty((b, k, c), np.float32)}
        self._chk(self.lib.bod_get_detections_batch(self.h, iptr(out["num"]), fptr(out["scores"]),
                                                    fptr(out["means"]), fptr(out["covs"]), fptr(out["counts"])))
        return out

    def wait_slot(self, slot):
        """Block until the batch in ``slot`` is complete without copying anything."""
        self._chk(self.lib.bod_collect(self.h, slot, None, None, None, None, None))

    def device_raw_pointers(self, mark_ready=False):
        """Device addresses (cls, box, cov-or-None) of the raw head outputs [B,N,A,.] fp32."""
        ptrs = (C.c_void_p * 3)()
        self._chk(self.lib.bod_device_raw(self.h, ptrs, int(mark_ready)))
        return [ptrs[i] for i in range(3)]

    def device_detection_pointers(self, slot=0):
        ptrs = (C.c_void_p * 5)()
        self._chk(self.lib.bod_device_detections(self.h, slot, ptrs))
        b, k, c = self.B, self.K, self.Ccls
        shapes = [(b,), (b, k, c), (b, k, 4), (b, k, 16), (b, k, c)]
        names = ["num", "scores", "means", "covs", "counts"]
        return {n: (int(p), s) for n, p, s in zip(names, ptrs, shapes)}

    # -- mergeable MC statistics (handles made with make_config(mc_statistics=True); include/bayesod.h) ----------
    def stat_reset(self):
        """Empty the accumulator (K = 0)."""
        self._chk(self.lib.bod_stat_reset(self.h))

    @staticmethod
    def _view(view):
        """'identity' / 'hflip' or 0 / 1 -> BOD_VIEW_*; any other int goes to the library, which refuses it."""
        if isinstance(view, str):
            if view not in VIEWS:
                raise ValueError("view must be one of %s or 0 / 1, got %r" % (sorted(VIEWS), view))
            return VIEWS[view]
        return int(view)

    def stat_forward(self, images=None, seed=0, first_image_id=0, sample_base=0, image_buffer=None, device_images=None, view=0):
        """Forward of this handle's n samples as samples ``sample_base .. sample_base + n - 1`` of the dropout streams, reduced to
        the statistics record and folded into the accumulator (``bod_stat_forward``).  images as in forward();
        ``device_images``: the address of a [B,H,W,3] float32 batch already on this device (another handle's image buffer,
        complete before the call) in place of this handle's own.  ``view='hflip'`` (or 1): the forward sees the frames mirrored
        left-right and its record is mapped back to the anchors of the frames as given (``bod_stat_forward_view``)."""
        v = self._view(view)
        if images is None:
            ptr, on_device = (self._device_images(image_buffer) if device_images is None else int(device_images)), 1
        else:
            a = self._img(images)
            ptr, on_device = a.ctypes.data, 0
        if v == _lib.BOD_VIEW_IDENTITY:
            self._chk(self.lib.bod_stat_forward(self.h, ptr, on_device, seed, first_image_id, int(sample_base)))
        else:
            self._chk(self.lib.bod_stat_forward_view(self.h, ptr, on_device, seed, first_image_id, int(sample_base), v))

    def stat_merge_from(self, other):
        """Fold ``other``'s accumulator into this one's (``bod_stat_merge_from``); ``other`` is unchanged."""
        self._chk(self.lib.bod_stat_merge_from(self.h, other.h))

    def stat_merge(self, ptrs, samples, view=0):
        """Fold a record of ``samples`` samples given as device addresses (cls_sum, box_moments, cov_sum or None); ``view='hflip'``:
        the record is that of a mirrored forward and is mapped back while it is folded (``bod_stat_merge_view``)."""
        ptrs = list(ptrs)
        p = (C.c_void_p * 3)(*[int(x) if x else None for x in (ptrs + [None])[:3]])
        v = self._view(view)
        if v == _lib.BOD_VIEW_IDENTITY:
            self._chk(self.lib.bod_stat_merge(self.h, p, int(samples)))
        else:
            self._chk(self.lib.bod_stat_merge_view(self.h, p, int(samples), v))
        if len(ptrs) > 3 and ptrs[3]:                     # a class_parts record: ent_sum follows (bod_stat_merge_entropy)
            self.stat_merge_entropy(ptrs[3], view=v)

    def stat_merge_entropy(self, ptr, view=0):
        """Fold the ``ent_sum`` [B,A] (device address) of the record the last ``stat_merge`` folded (``bod_stat_merge_entropy``)."""
        self._chk(self.lib.bod_stat_merge_entropy(self.h, C.c_void_p(int(ptr)), self._view(view)))

    def stat_device_entropy_pointer(self):
        """Device address of the accumulator's ``ent_sum`` [B,A] (``bod_stat_device_entropy``)."""
        p = C.c_void_p(0)
        self._chk(self.lib.bod_stat_device_entropy(self.h, C.byref(p)))
        return int(p.value or 0)

    def get_entropy(self):
        """``ent_sum`` [B,A] of the accumulator: the sum over its samples of the entropy of softmax(class logits)."""
        ent = np.empty((self.B, self.A), np.float32)
        self._chk(self.lib.bod_stat_get_entropy(self.h, fptr(ent)))
        return ent

    def set_entropy(self, ent_sum):
        """Replace the accumulator's ``ent_sum`` (``bod_stat_set_entropy``); follows ``set_statistics`` on a class_parts handle."""
        ent = as_f32(ent_sum)
        if ent.shape != (self.B, self.A):
            raise ValueError("ent_sum of shape %s, expected %s" % (ent.shape, (self.B, self.A)))
        self._chk(self.lib.bod_stat_set_entropy(self.h, fptr(ent)))

    def stat_device_pointers(self):
        """Device addresses [cls_sum [B,A,C], box_moments [B,A,16], cov_sum [B,A,10] or None] of the accumulator."""
        ptrs = (C.c_void_p * 3)()
        self._chk(self.lib.bod_stat_device(self.h, ptrs, None))
        return [ptrs[i] for i in range(3)]

    @property
    def stat_samples(self):
        """K: the number of MC samples the accumulator holds."""
        k = C.c_int32(0)
        self._chk(self.lib.bod_stat_device(self.h, None, C.byref(k)))
        return int(k.value)

    def get_statistics(self):
        """(cls_sum [B,A,C], box_moments [B,A,16], cov_sum [B,A,10] or None, samples) of the accumulator, on the host."""
        n = (self.B, self.A)
        cls = np.empty(n + (self.Ccls,), np.float32)
        box = np.empty(n + (16,), np.float32)
        cov = np.empty(n + (10,), np.float32) if self.cfg.has_covar_head else None
        k = C.c_int32(0)
        self._chk(self.lib.bod_stat_get(self.h, fptr(cls), fptr(box), fptr(cov), C.byref(k)))
        return cls, box, cov, int(k.value)

    def set_statistics(self, cls_sum, box_moments, cov_sum=None, samples=0):
        """Replace the accumulator (``bod_stat_set``): arrays as get_statistics returns them (None: left as it is), K = samples."""
        n = (self.B, self.A)
        arrs = []
        for a, w in ((cls_sum, self.Ccls), (box_moments, 16), (cov_sum, 10)):
            a = as_f32(a) if a is not None else None
            if a is not None and a.shape != n + (w,):
                raise ValueError("statistics array of shape %s, expected %s" % (a.shape, n + (w,)))
            arrs.append(a)
        self._chk(self.lib.bod_stat_set(self.h, fptr(arrs[0]), fptr(arrs[1]), fptr(arrs[2]), int(samples)))

    def stat_posterior(self, seed=0, first_image_id=0):
        """posterior() on the accumulator with N = stat_samples (``bod_stat_posterior``); nms() / cluster_fuse() follow."""
        self._chk(self.lib.bod_stat_posterior(self.h, seed, first_image_id))

    def stat_acquisition(self, min_foreground=0.05, top_k=16):
        """Acquisition scores of the accumulator (``bod_stat_acquisition``): ``(scores [B,12], per_class [B,C-1,3])``
        float64; the columns are ``acquisition.COLUMNS`` / ``acquisition.PER_CLASS_COLUMNS``.  Reads the record only."""
        opt = _lib.BodAcquisitionOptions(float(min_foreground), int(top_k), (C.c_int32 * 2)(0, 0))
        scores = np.empty((self.B, 12), np.float64)
        per_class = np.empty((self.B, self.Ccls - 1, 3), np.float64)
        self._chk(self.lib.bod_stat_acquisition(self.h, C.byref(opt), _lib.dptr(scores), _lib.dptr(per_class)))
        return scores, per_class

    def stat_acquisition_map(self):
        """[B,A] float32: every anchor's mutual information of the last ``stat_acquisition``, NaN outside the foreground set
        (``bod_stat_acquisition_map``, a test hook)."""
        mi = np.empty((self.B, self.A), np.float32)
        self._chk(self.lib.bod_stat_acquisition_map(self.h, fptr(mi)))
        return mi

    def bench_head_conv(self, layer=1, variant=0, iters=10):
        ms, fl = C.c_double(0), C.c_double(0)
        self._chk(self.lib.bod_bench_head_conv(self.h, layer, variant, iters, C.byref(ms), C.byref(fl)))
        return ms.value, fl.value

    # ------------------------------------------------------------------ measurement
    def gather_detections(self, slot=-1, comm=None, world=1, rank=0, root=0, want_host=True):
        """The path's one multi-GPU exchange through the C ABI (``bod_gather_detections``): packs this batch's detection
        records on the device and gathers every rank's block on ``root`` with ONE RCCL gather.  ``comm``: an ``ncclComm_t``
        as an integer / ``c_void_p`` (None: single process).  ``slot``: ticket of ``infer_async`` (-1 after ``infer``).
        Returns [world, B, K, 1+4+16+2C] float32 on the root (None elsewhere; covariance_parts handles: 48 floats wider, class_parts handles: 4); unpack
        with distributed.unpack_records.
        ``want_host=False`` (root only): nothing is copied or waited for; returns ``(device pointer, shape)`` of the gathered
        block, complete after ``collect(slot)`` (a ticket) or ``synchronize()`` (slot -1) -- see include/bayesod.h."""
        w = int(self.lib.bod_record_width(self.h))
        out = None
        dev = C.c_void_p(0)
        if rank == root and want_host:
            out = np.empty((world, self.B, self.K, w), np.float32)
        self._chk(self.lib.bod_gather_detections(self.h, int(slot), C.c_void_p(int(comm) if comm else 0), int(world), int(rank), int(root),
                                                 out.ctypes.data if out is not None else None,
                                                 C.byref(dev) if rank == root else None))
        if rank == root and not want_host:
            return int(dev.value or 0), (world, self.B, self.K, w)
        return out

    def plan_info(self):
        """{'aggregating', 'fused_head_outputs', 'row_reuse', 'fan_out_row_reuse', 'ops', 'plane_row_reuse_layers', 'tower_mx',
        'sparse_tail', 'sparse_halo', 'sparse_tail_rows', 'stage_end_pixels'} of the forward plan (bod_plan_info_n)."""
        info = (C.c_int32 * 11)()
        self._chk(self.lib.bod_plan_info_n(self.h, info, 11))
        return {"aggregating": bool(info[0]), "fused_head_outputs": bool(info[1]), "row_reuse": bool(info[2]),
                "fan_out_row_reuse": bool(info[3]), "ops": int(info[4]), "plane_row_reuse_layers": int(info[5]), "tower_mx": bool(info[6]), "tower_mx_format": int(info[6]),
                "sparse_tail": bool(info[7]), "sparse_halo": bool(info[8]), "sparse_tail_rows": int(info[9]),
                "stage_end_pixels": int(info[10])}

    @property
    def aggregating(self):
        return self.plan_info()["aggregating"]

    def profile_begin(self, which=None):
        """which: None keeps the current selection; 0 = every head 3x3 launch, 1 = the row-reuse tower kernel's launches
        only (one kernel symbol), 2 = the others (the fan-out launch of the first tower layer)."""
        if which is not None:
            self._chk(self.lib.bod_profile_select(self.h, int(which)))
        self._chk(self.lib.bod_profile_begin(self.h))

    def profile_end(self):
        hm, pm, fl = C.c_double(0), C.c_double(0), C.c_double(0)
        hl, pl = C.c_int64(0), C.c_int64(0)
        self._chk(self.lib.bod_profile_end(self.h, C.byref(hm), C.byref(hl), C.byref(fl), C.byref(pm), C.byref(pl)))
        return {"head_conv_ms": hm.value, "head_conv_launches": hl.value, "head_conv_flops": fl.value,
                "posterior_ms": pm.value, "posterior_launches": pl.value}


def pack_ragged(frames, batch=None):
    """Frames of mixed sizes as the ragged uploads take them: (packed uint8 buffer -- the frames back to back, frame b at byte
    3 * sum of h_i * w_i over i < b -- and sizes [n,2] int32 (h, w)).  ``frames``: a sequence of uint8 [h,w,3] arrays, ``batch``
    of them when given."""
    frames = list(frames)
    if batch is not None and len(frames) != int(batch):
        raise ValueError("expected %d frames, got %d" % (int(batch), len(frames)))
    if not frames:
        raise ValueError("no frames to pack")
    for i, f in enumerate(frames):
        if not isinstance(f, np.ndarray) or f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3 or f.shape[0] < 1 or f.shape[1] < 1:
            raise ValueError("frame %d: expected a uint8 array of shape (h, w, 3), got %s %s" %
                             (i, getattr(f, "dtype", type(f).__name__), getattr(f, "shape", "")))
    sizes = np.asarray([f.shape[:2] for f in frames], np.int32)
    buf = np.empty(3 * int(np.sum(sizes[:, 0].astype(np.int64) * sizes[:, 1])), np.uint8)
    off = 0
    for f in frames:
        buf[off:off + f.size] = f.reshape(-1)
        off += f.size
    return buf, sizes


# bod_augment as a NumPy record: what the augmented uploads and augment_boxes take
AUGMENT_DTYPE = np.dtype([("flip", "<i4"), ("scale", "<f4"), ("off_y", "<f4"), ("off_x", "<f4"), ("gain", "<f4"), ("bias", "<f4")])
AUGMENT_IDENTITY = {"flip": 0, "scale": 1.0, "off_y": 0.5, "off_x": 0.5, "gain": 1.0, "bias": 0.0}
# training_config['augmentation'] of the yaml: keys and (mild) defaults
AUGMENT_DEFAULTS = {"flip_probability": 0.5, "scale_range": [0.8, 1.25], "random_placement": True, "gain_range": [0.8, 1.2],
                    "bias_range": [-20.0, 20.0], "min_visible": 0.25}


def augment_records(aug, batch=None):
    """``aug`` -- an ``AUGMENT_DTYPE`` array or a sequence of dicts (missing fields: no augmentation) -- as one C-contiguous
    ``AUGMENT_DTYPE`` array of ``batch`` records."""
    if isinstance(aug, np.ndarray):
        if aug.dtype != AUGMENT_DTYPE:
            raise ValueError("augmentation records must have dtype AUGMENT_DTYPE, got %s" % (aug.dtype,))
        rec = np.ascontiguousarray(aug).reshape(-1)
    else:
        rec = np.empty(len(aug), AUGMENT_DTYPE)
        for i, d in enumerate(aug):
            unknown = set(d) - set(AUGMENT_IDENTITY)
            if unknown:
                raise ValueError("frame %d: unknown augmentation field(s) %s" % (i, sorted(unknown)))
            rec[i] = tuple(d.get(k, v) for k, v in AUGMENT_IDENTITY.items())
    if batch is not None and rec.shape[0] != int(batch):
        raise ValueError("expected %d augmentation records, got %d" % (int(batch), rec.shape[0]))
    return rec


def augment_config(cfg=None):
    """``AUGMENT_DEFAULTS`` overridden by ``cfg`` (``training_config['augmentation']``); an unknown key is an error."""
    out = dict(AUGMENT_DEFAULTS)
    unknown = set(cfg or {}) - set(out)
    if unknown:
        raise ValueError("unknown augmentation setting(s) %s (known: %s)" % (sorted(unknown), sorted(out)))
    out.update(cfg or {})
    return out


def _f32_in(x, lo, hi):
    """x in [lo, hi] as a float32 that is still in [lo, hi] (rounding to float32 may step over a bound by one ulp)."""
    v = np.float32(x)
    if float(v) > hi:
        v = np.nextafter(v, np.float32(-np.inf))
    elif float(v) < lo:
        v = np.nextafter(v, np.float32(np.inf))
    return v


def draw_augmentation(cfg, seed, image_ids):
    """One record per frame (``AUGMENT_DTYPE``), drawn from ``numpy.random.Generator(numpy.random.Philox(key=[seed, image_id]))``:
    a frame's record depends on (seed, image id) alone -- not on the batch it sits in, the step a run was resumed at or the rank
    that draws it.  Six doubles are drawn per frame, always and in this order, whatever ``cfg`` switches off:

      1. ``random()`` -> flip = 1 when below ``flip_probability``;
      2. ``random()`` -> scale = exp(log lo + u (log hi - log lo)) over ``scale_range`` (log-uniform);
      3. ``random()`` -> off_y, 4. ``random()`` -> off_x: the draw itself with ``random_placement``, else 0.5;
      5. ``random()`` -> gain = lo + u (hi - lo) over ``gain_range``;
      6. ``random()`` -> bias = lo + u (hi - lo) over ``bias_range``.

    ``cfg``: ``AUGMENT_DEFAULTS`` keys (None: the defaults); ``min_visible`` is ``augment_boxes``' business, not a record field."""
    cfg = augment_config(cfg)
    ids = [int(i) for i in np.asarray(image_ids).reshape(-1)]
    rec = np.empty(len(ids), AUGMENT_DTYPE)
    (s_lo, s_hi), (g_lo, g_hi), (b_lo, b_hi) = cfg["scale_range"], cfg["gain_range"], cfg["bias_range"]
    if not (0.0 < s_lo <= s_hi) or g_lo > g_hi or b_lo > b_hi or not (0.0 <= cfg["flip_probability"] <= 1.0):
        raise ValueError("bad augmentation ranges: %r" % (cfg,))
    for k, image_id in enumerate(ids):
        u = np.random.Generator(np.random.Philox(key=[int(seed), image_id])).random(6)
        placed = bool(cfg["random_placement"])
        rec[k] = (int(u[0] < cfg["flip_probability"]),
                  _f32_in(np.exp(np.log(s_lo) + u[1] * (np.log(s_hi) - np.log(s_lo))), s_lo, s_hi),
                  np.float32(u[2]) if placed else 0.5, np.float32(u[3]) if placed else 0.5,
                  _f32_in(g_lo + u[4] * (g_hi - g_lo), g_lo, g_hi), _f32_in(b_lo + u[5] * (b_hi - b_lo), b_lo, b_hi))
    return rec


def augment_boxes(src_hw, net_hw, aug, gt_boxes, gt_classes, aspect_resize=True, min_visible=0.25):
    """Ground truth of augmented frames (``bod_augment_boxes``; host arithmetic, no device): ``src_hw`` [B,2] source sizes, ``gt_boxes``
    / ``gt_classes`` per-frame lists of [G_b,4] corners (y1,x1,y2,x2) in SOURCE pixels and [G_b,C] class rows.  Returns the two
    lists in network pixels of the augmented frames: boxes flipped, scaled, shifted by pad - crop and clipped; a box of which less
    than ``min_visible`` stays visible is dropped; a frame left without a box gets the row [0,0,1,1] of the background class."""
    lib = _lib.load()
    sizes = np.ascontiguousarray(src_hw, dtype=np.int32).reshape(-1, 2)
    b = sizes.shape[0]
    rec = augment_records(aug, b)
    if len(gt_boxes) != b or len(gt_classes) != b:
        raise ValueError("expected ground truth for %d frames, got %d box and %d class arrays" % (b, len(gt_boxes), len(gt_classes)))
    boxes = [as_f32(x).reshape(-1, 4) for x in gt_boxes]
    classes = [as_f32(c) for c in gt_classes]
    width = max([c.shape[-1] for c in classes if c.ndim == 2] + [c.size // x.shape[0] for x, c in zip(boxes, classes) if x.shape[0]])
    for i, (x, c) in enumerate(zip(boxes, classes)):
        if c.size != x.shape[0] * width:
            raise ValueError("frame %d: class rows of shape %s do not match %d boxes x %d classes" % (i, c.shape, x.shape[0], width))
    ng = np.asarray([x.shape[0] for x in boxes], np.int32)
    # (one spare row: a pointer to an empty array may be NULL)
    allb = as_f32(np.concatenate(boxes + [np.zeros((1, 4), np.float32)], axis=0))
    allc = as_f32(np.concatenate([c.reshape(-1, width) for c in classes] + [np.zeros((1, width), np.float32)], axis=0))
    rows = int(np.maximum(ng, 1).sum())
    num_out, bo, co = np.empty(b, np.int32), np.empty((rows, 4), np.float32), np.empty((rows, width), np.float32)
    st = lib.bod_augment_boxes(b, iptr(sizes), int(net_hw[0]), int(net_hw[1]), int(bool(aspect_resize)),
                               rec.ctypes.data_as(C.POINTER(_lib.BodAugment)), iptr(ng), fptr(allb), fptr(allc), width,
                               float(min_visible), iptr(num_out), fptr(bo), fptr(co))
    _lib.check(lib, None, st)
    ends = np.cumsum(num_out)
    return ([bo[e - n:e].copy() for n, e in zip(num_out, ends)], [co[e - n:e].copy() for n, e in zip(num_out, ends)])


def _pack_gt(gt_boxes, gt_classes, batch, num_classes=None):
    """Per-frame lists -> (num_gt [B] int32, boxes [sum G,4], class rows [sum G,C]) as the C ABI takes them."""
    if len(gt_boxes) != batch or len(gt_classes) != batch:
        raise ValueError("expected ground truth for %d frames, got %d box and %d class arrays" % (batch, len(gt_boxes), len(gt_classes)))
    boxes = [as_f32(b).reshape(-1, 4) for b in gt_boxes]
    classes = [as_f32(c) for c in gt_classes]
    classes = [c.reshape(b.shape[0], -1) if c.ndim != 2 else c for b, c in zip(boxes, classes)]
    width = classes[0].shape[1] if num_classes is None else num_classes
    for b, c in zip(boxes, classes):
        if c.shape != (b.shape[0], width):
            raise ValueError("class rows of shape %s do not match %d boxes x %d classes" % (c.shape, b.shape[0], width))
    ng = np.asarray([b.shape[0] for b in boxes], np.int32)
    return ng, as_f32(np.concatenate(boxes, axis=0)), as_f32(np.concatenate(classes, axis=0))


def anchor_targets(anchors, gt_boxes, gt_classes, min_positive_iou=0.5, max_negative_iou=0.4, device=0, return_best=False):
    """Dense anchor targets on the device (``bod_anchor_targets``): anchors [A,4] (v,u,h,w); gt_boxes / gt_classes are
    per-frame lists of [G_b,4] corners (y1,x1,y2,x2) and [G_b,C] class rows.  Returns cls_targets [B,A,C], box_targets
    [B,A,4], positive and negative masks [B,A] (bool), plus best_gt [B,A] int32 and best_iou [B,A] with return_best."""
    lib = _lib.load()
    anchors = as_f32(anchors).reshape(-1, 4)
    b, a = len(gt_boxes), anchors.shape[0]
    ng, boxes, classes = _pack_gt(gt_boxes, gt_classes, b)
    c = classes.shape[1]
    ct, bt = np.empty((b, a, c), np.float32), np.empty((b, a, 4), np.float32)
    pm, nm = np.empty((b, a), np.uint8), np.empty((b, a), np.uint8)
    bg = np.empty((b, a), np.int32) if return_best else None
    bi = np.empty((b, a), np.float32) if return_best else None
    u8 = C.POINTER(C.c_uint8)
    st = lib.bod_anchor_targets(device, a, fptr(anchors), b, iptr(ng), fptr(boxes), fptr(classes), c, float(min_positive_iou),
                                float(max_negative_iou), fptr(ct), fptr(bt), pm.ctypes.data_as(u8), nm.ctypes.data_as(u8),
                                iptr(bg), fptr(bi))
    _lib.check(lib, None, st)
    out = (ct, bt, pm.astype(bool), nm.astype(bool))
    return out + (bg, bi) if return_best else out


def stage_conv(x, w, bias=None, stride=1, padding="same", relu=False, residual=None, dropout_rate=0.0,
               seed=0, layer_id=0, image_id=0, round_output_bf16=False, device=0, precision='bf16'):
    """One convolution through the pipeline's MFMA kernel (``bod_stage_conv``), for parity tests.
    x [B,H,W,Cin], w HWIO; returns [B,OH,OW,Cout] float32.  precision='f16mx' (a head-tower layer: 3x3, SAME, 256 -> 256):
    round_output_bf16 = 0 / 1 / 2 selects hx -> pairs / hx -> hx / pairs -> hx (include/bayesod.h)."""
    lib = _lib.load()
    x, w = as_f32(x), as_f32(w)
    b, h, wd, cin = x.shape
    kh, kw, cin2, cout = w.shape
    if cin2 != cin:
        raise ValueError("kernel Cin %d != input Cin %d" % (cin2, cin))
    if padding == "same":
        oh, ow = -(-h // stride), -(-wd // stride)
    else:
        oh, ow = (h - kh) // stride + 1, (wd - kw) // stride + 1
    out = np.empty((b, oh, ow, cout), np.float32)
    bias = as_f32(bias) if bias is not None else None
    residual = as_f32(residual) if residual is not None else None
    st = lib.bod_stage_conv(device, fptr(x), b, h, wd, cin, fptr(w), fptr(bias), kh, kw, cout, stride,
                            int(padding == "same"), int(relu), fptr(residual), float(dropout_rate), seed,
                            layer_id, image_id, int(round_output_bf16), PRECISIONS[precision], fptr(out))
    _lib.check(lib, None, st)
    return out


def stage_conv_wgrad(x, dy, kernel_hw, stride=1, padding="same", ksplit=0, device=0):
    """Weight / bias gradient of one Conv2D through the MFMA kernel (``bod_stage_conv_wgrad``): returns
    (dw [KH,KW,Cin,Cout], db [Cout]) for layer input x [B,H,W,Cin] and output gradient dy [B,OH,OW,Cout]."""
    lib = _lib.load()
    x, dy = as_f32(x), as_f32(dy)
    b, h, wd, cin = x.shape
    kh, kw = int(kernel_hw[0]), int(kernel_hw[1])
    cout = dy.shape[-1]
    dw = np.empty((kh, kw, cin, cout), np.float32)
    db = np.empty((cout,), np.float32)
    st = lib.bod_stage_conv_wgrad(device, fptr(x), b, h, wd, cin, fptr(dy), kh, kw, cout, stride,
                                  int(padding == "same"), int(ksplit), fptr(dw), fptr(db))
    _lib.check(lib, None, st)
    return dw, db


def stage_conv_dgrad(dy, w, padding="same", device=0):
    """Input gradient of a stride-1 Conv2D: the forward kernel on dy with the spatially flipped, cin/cout-swapped
    weights (SAME: symmetric padding for odd kernels; VALID forward = full correlation, not covered here)."""
    w = as_f32(w)
    if padding != "same" or w.shape[0] % 2 == 0 or w.shape[1] % 2 == 0:
        raise ValueError("stage_conv_dgrad covers stride-1 SAME convolutions with odd kernels")
    wt = np.ascontiguousarray(np.transpose(w[::-1, ::-1], (0, 1, 3, 2)))
    return stage_conv(dy, wt, None, stride=1, padding="same", device=device)


def stage_act_backward(dout, out_off, cout, cout_pad, out_cstride, kpad, out_act=None, dout_relu=None, scale=1.0, res_off=None,
                       res_cstride=0, dres=None, dzp=None, dzt=None, precision="bf16", device=0):
    """Activation backward of one layer as the training step launches it (``bod_stage_act_backward``).  dout / out_act /
    dout_relu: flat arrays in the output buffer's layout; out_off / res_off [M] int32 pixel indices; dres, dzp (like dout) and dzt
    [cout_pad, kpad] are prefills (None: not wanted).  Returns dict(dz [M, cout_pad], dzp, dzt, dres, wrote_transpose); bf16 values
    come back widened to float32."""
    lib = _lib.load()
    dout = as_f32(dout).reshape(-1)
    out_off = np.ascontiguousarray(out_off, dtype=np.int32).reshape(-1)
    m = int(out_off.size)
    flat = lambda a: None if a is None else as_f32(a).reshape(-1).copy()
    out_act, dout_relu, dres, dzp, dzt = flat(out_act), flat(dout_relu), flat(dres), flat(dzp), flat(dzt)
    for name, a in (("out_act", out_act), ("dout_relu", dout_relu), ("dzp", dzp)):
        if a is not None and a.size != dout.size:
            raise ValueError("%s must have dout's %d elements" % (name, dout.size))
    if dzt is not None and dzt.size != int(cout_pad) * int(kpad):
        raise ValueError("dzt must have cout_pad * kpad elements")
    if res_off is not None:
        res_off = np.ascontiguousarray(res_off, dtype=np.int32).reshape(-1)
        if res_off.size != m:
            raise ValueError("res_off must have one entry per row")
    dz = np.empty((m, int(cout_pad)), np.float32)
    wrote = C.c_int32(-1)
    st = lib.bod_stage_act_backward(device, PRECISIONS[precision], fptr(dout), fptr(out_act), fptr(dout_relu), dout.size, iptr(out_off),
                                    iptr(res_off), m, int(cout), int(cout_pad), int(out_cstride), int(res_cstride), float(scale),
                                    int(kpad), fptr(dres), 0 if dres is None else dres.size, fptr(dz), fptr(dzp), fptr(dzt),
                                    C.byref(wrote))
    _lib.check(lib, None, st)
    return {"dz": dz, "dzp": dzp, "dzt": None if dzt is None else dzt.reshape(int(cout_pad), int(kpad)), "dres": dres,
            "wrote_transpose": bool(wrote.value)}


DGRAD_ROUTES = {"flip": _lib.BOD_DGRAD_FLIP, "rows": _lib.BOD_DGRAD_ROWS, "col2im": _lib.BOD_DGRAD_COL2IM}


def stage_conv_dgrad_route(dz, w, in_hw, din, route, stride=1, padding="same", ksplit=0, device=0):
    """Input gradient of one bf16 Conv2D through one of the training step's three launches (``bod_stage_conv_dgrad``): dz
    [G,B,OH,OW,Cout] or [B,OH,OW,Cout], w [G,KH,KW,Cin,Cout] or HWIO, din [G,B,H+2,W+2,Cin] or [B,H+2,W+2,Cin]: the prefilled fp32
    gradient plane of the input with its border.  Returns (din after the launch, same shape; split-K factor used; whether the
    launch took the 256x256 tile)."""
    lib = _lib.load()
    dz, w, din = as_f32(dz), as_f32(w), as_f32(din).copy()
    grouped = w.ndim == 5
    g = w.shape[0] if grouped else 1
    kh, kw, cin, cout = w.shape[-4:]
    h, wd = int(in_hw[0]), int(in_hw[1])
    b = dz.shape[-4]
    if padding == "same":
        oh, ow = -(-h // stride), -(-wd // stride)
    else:
        oh, ow = (h - kh) // stride + 1, (wd - kw) // stride + 1
    lead = (g,) if grouped else ()
    if dz.shape != lead + (b, oh, ow, cout) or din.shape != lead + (b, h + 2, wd + 2, cin):
        raise ValueError("dz %s / din %s do not fit %d group(s) of a %dx%d input" % (dz.shape, din.shape, g, h, wd))
    info = np.zeros(2, np.int32)
    st = lib.bod_stage_conv_dgrad(device, DGRAD_ROUTES[route], fptr(dz), fptr(w), b, h, wd, cin, cout, kh, kw, int(stride),
                                  int(padding == "same"), int(ksplit), g, fptr(din), iptr(info))
    _lib.check(lib, None, st)
    return din, int(info[0]), bool(info[1])


def stage_stem_pool_backward(stem_out, dpool, precision="bf16", device=0):
    """Backward of the stem's zero-pad + 3x3 s2 max-pool under its ReLU (``bod_stage_stem_pool_backward``): stem_out [B,ih,iw,64],
    dpool [B,oh+2,ow+2,64] (the pooled gradient on its bordered plane); returns dz [B,ih,iw,64] float32."""
    lib = _lib.load()
    stem_out, dpool = as_f32(stem_out), as_f32(dpool)
    b, ih, iw, c = stem_out.shape
    if c != 64:
        raise ValueError("the stem has 64 channels")
    dz = np.empty_like(stem_out)
    st = lib.bod_stage_stem_pool_backward(device, PRECISIONS[precision], fptr(stem_out), fptr(dpool), dpool.size, b, ih, iw, fptr(dz))
    _lib.check(lib, None, st)
    return dz


STEM_FORMS = {"auto": _lib.BOD_STEM_AUTO, "f32+pool_f32": _lib.BOD_STEM_F32_POOL_F32, "f32+pool_split": _lib.BOD_STEM_F32_POOL_SPLIT,
              "seg64+pool": _lib.BOD_STEM_SEG64_POOL, "row+pool": _lib.BOD_STEM_ROW_POOL, "fused8": _lib.BOD_STEM_FUSED_8,
              "fused4": _lib.BOD_STEM_FUSED_4, "fused_split": _lib.BOD_STEM_FUSED_SPLIT}
STEM_FORM_PRECISION = {"f32+pool_f32": "fp32", "f32+pool_split": "bf16x3", "seg64+pool": "bf16", "row+pool": "bf16", "fused8": "bf16",
                       "fused4": "bf16", "fused_split": "bf16x3"}
STEM_SENTINEL = -65536.0


def stem_geometry(h, w):
    """(oh, ow, ph, pw) of the stem and its pooled plane for an H x W frame, as handle creation derives them."""
    oh, ow = (h - 7) // 2 + 1, (w - 7) // 2 + 1
    return oh, ow, (oh - 1) // 2 + 1, (ow + 1) // 2 + 1


def stage_stem(images, w, bias, form="auto", precision=None, misalign=False, n_cu=0, sentinel=STEM_SENTINEL, device=0):
    """One form of the stem through the library's launchers (``bod_stage_stem``): images [B,H,W,3], w [7,7,3,64] (folded), bias [64].
    form: a key of STEM_FORMS; precision is implied by an explicit form and required ('fp32', 'bf16', 'bf16x3') with 'auto'.
    Returns dict(form: the key of the form that ran, stem: [B,oh,ow,64] float32 or None for a fused form, pooled:
    [B,ph+2,pw+2,64 or 128] float32 with its border); both device planes were prefilled with ``sentinel``."""
    lib = _lib.load()
    images, w, bias = as_f32(images), as_f32(w), as_f32(bias)
    if images.ndim != 4 or images.shape[3] != 3 or w.shape != (7, 7, 3, 64) or bias.shape != (64,):
        raise ValueError("stage_stem: images [B,H,W,3], w [7,7,3,64], bias [64]")
    if precision is None:
        precision = STEM_FORM_PRECISION[form]           # KeyError for 'auto': the rule needs a precision
    b, h, wd, _ = images.shape
    oh, ow, ph, pw = stem_geometry(h, wd)
    if min(oh, ow) < 1:
        raise ValueError("stage_stem: H and W must be at least 7")
    stem = np.full((b, oh, ow, 64), np.nan, np.float32)
    pooled = np.full((b, ph + 2, pw + 2, 128 if precision == "bf16x3" else 64), np.nan, np.float32)
    ran = C.c_int32(-1)
    st = lib.bod_stage_stem(device, STEM_FORMS[form], PRECISIONS[precision], fptr(images), b, h, wd, fptr(w), fptr(bias), int(bool(misalign)),
                            int(n_cu), float(sentinel), fptr(stem), fptr(pooled), C.byref(ran))
    _lib.check(lib, None, st)
    name = {v: k for k, v in STEM_FORMS.items()}[ran.value]
    return {"form": name, "stem": None if name.startswith("fused") else stem, "pooled": pooled}


def stage_stem_pool(stem, mode, sentinel=STEM_SENTINEL, device=0):
    """The stem's zero-pad + 3x3 s2 max-pool alone (``bod_stage_stem_pool``) on stem [B,ih,iw,64]; mode 0 bf16 -> bf16, 1 fp32 ->
    fp32, 2 fp32 -> (hi, lo) pairs.  Returns the pooled plane with its border, [B,oh+2,ow+2,64 (mode 2: 128)] float32."""
    lib = _lib.load()
    stem = as_f32(stem)
    if stem.ndim != 4 or stem.shape[3] != 64:
        raise ValueError("stage_stem_pool: stem [B,ih,iw,64]")
    b, ih, iw, _ = stem.shape
    oh, ow = (ih - 1) // 2 + 1, (iw + 1) // 2 + 1
    pooled = np.full((b, oh + 2, ow + 2, 128 if int(mode) == 2 else 64), np.nan, np.float32)
    st = lib.bod_stage_stem_pool(device, int(mode), fptr(stem), b, ih, iw, float(sentinel), fptr(pooled))
    _lib.check(lib, None, st)
    return pooled


def stage_fold_pack(layers, device=0):
    """Batch-norm folding and the three bf16 weight packings of every layer in ONE launch (``bod_stage_fold_pack``).  layers:
    dicts with kernel [taps,cin,cout] (or HWIO), cout_pad, optional bias and gamma / beta / mean / var.  Returns one dict per
    layer: w_fwd [cout_pad,taps,cin], w_bwd [taps*cin,cout_pad], w_flip [cin,taps,cout_pad] (uint16: raw bf16 bits), b_fwd
    [cout_pad] (float32) and, for a layer with ``fwd32`` set, w_fwd32 [taps*cin,cout] (float32; else None).  As in the training
    step, a layer that asks for the fp32 packing (the stem) is packed element by element, the others in 64x64 tiles when their
    cin and cout_pad allow."""
    lib = _lib.load()
    n = len(layers)
    arr = (_lib.BodFoldLayer * max(n, 1))()
    u16 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint16))
    keep, outs = [], []
    for i, layer in enumerate(layers):
        k = as_f32(layer["kernel"])
        cin, cout = k.shape[-2:]
        taps = int(k.size // (cin * cout))
        cp = int(layer["cout_pad"])
        ins = {name: (as_f32(layer[name]).reshape(-1) if layer.get(name) is not None else None)
               for name in ("bias", "gamma", "beta", "mean", "var")}
        for name, a in ins.items():
            if a is not None and a.size != cout:
                raise ValueError("layer %d: %s must have %d elements" % (i, name, cout))
        o = {"w_fwd": np.zeros((max(cp, 0), taps, cin), np.uint16), "w_bwd": np.zeros((taps * cin, max(cp, 0)), np.uint16),
             "w_flip": np.zeros((cin, taps, max(cp, 0)), np.uint16),
             "w_fwd32": np.zeros((taps * cin, cout), np.float32) if layer.get("fwd32") else None,
             "b_fwd": np.zeros((max(cp, 0),), np.float32)}
        keep.append((k, ins))
        outs.append(o)
        arr[i] = _lib.BodFoldLayer(fptr(k), fptr(ins["bias"]), fptr(ins["gamma"]), fptr(ins["beta"]), fptr(ins["mean"]), fptr(ins["var"]),
                                   taps, cin, cout, cp, u16(o["w_fwd"]), u16(o["w_bwd"]), u16(o["w_flip"]), fptr(o["w_fwd32"]),
                                   fptr(o["b_fwd"]))
    st = lib.bod_stage_fold_pack(device, n, arr)
    _lib.check(lib, None, st)
    return outs


def pdq_corner_heatmaps(img_hw, means_yx, covs_yx, device=0, heatmaps=True):
    """Gaussian corners on the device (``bod_pdq_corner_heatmaps``), for parity tests of prob_detection_quality.corner_roi /
    corner_heatmap: means_yx [n,2], covs_yx [n,2,2] in (y, x) order; returns (rois [n,4] x0 y0 x1 y1, heatmaps [n,H,W] float32
    or None)."""
    lib = _lib.load()
    h, w = int(img_hw[0]), int(img_hw[1])
    means = np.ascontiguousarray(means_yx, dtype=np.float64).reshape(-1, 2)
    covs = np.ascontiguousarray(covs_yx, dtype=np.float64).reshape(-1, 2, 2)
    n = means.shape[0]
    rois = np.zeros((n, 4), np.int32)
    heat = np.empty((n, h, w), np.float32) if heatmaps else None
    st = lib.bod_pdq_corner_heatmaps(device, h, w, n, _lib.dptr(means), _lib.dptr(covs), iptr(rois), fptr(heat))
    _lib.check(lib, None, st)
    return rois, heat


def pdq_frames(img_hw, num_gt, gt_boxes, num_det, det_boxes, det_corner_covs, device=0, heatmaps=False):
    """Per-frame PDQ losses on the device (``bod_pdq_frames``) for frames of one image size: gt_boxes [sum G,4] and
    det_boxes [sum D,4] as int32 x1 y1 x2 y2, det_corner_covs [sum D,2,2,2] (PBoxDetInst.covs).  Returns per frame lists
    (fg_loss [G,D], bg_loss [G,D], det_bg_loss [D]) as float64 arrays, and the heatmaps [sum D,H,W] (or None)."""
    lib = _lib.load()
    h, w = int(img_hw[0]), int(img_hw[1])
    ng = np.ascontiguousarray(num_gt, dtype=np.int32).reshape(-1)
    nd = np.ascontiguousarray(num_det, dtype=np.int32).reshape(-1)
    if ng.shape != nd.shape:
        raise ValueError("num_gt and num_det must have one entry per frame")
    gtb = np.ascontiguousarray(gt_boxes, dtype=np.int32).reshape(-1, 4)
    detb = np.ascontiguousarray(det_boxes, dtype=np.int32).reshape(-1, 4)
    covs = np.ascontiguousarray(det_corner_covs, dtype=np.float64).reshape(-1, 2, 2, 2)
    if gtb.shape[0] != int(ng.sum()) or detb.shape[0] != int(nd.sum()) or covs.shape[0] != detb.shape[0]:
        raise ValueError("box / covariance rows do not match the per-frame counts")
    pairs = int(np.sum(ng.astype(np.int64) * nd))
    fg = np.zeros(pairs, np.float64)
    bg = np.zeros(pairs, np.float64)
    dbg = np.zeros(detb.shape[0], np.float64)
    heat = np.empty((detb.shape[0], h, w), np.float32) if heatmaps else None
    st = lib.bod_pdq_frames(device, h, w, ng.size, iptr(ng), iptr(gtb), iptr(nd), iptr(detb), _lib.dptr(covs), _lib.dptr(fg),
                            _lib.dptr(bg), _lib.dptr(dbg), fptr(heat))
    _lib.check(lib, None, st)
    fgs, bgs, dbgs = [], [], []
    p = d = 0
    for g_n, d_n in zip(ng.tolist(), nd.tolist()):
        fgs.append(fg[p:p + g_n * d_n].reshape(g_n, d_n))
        bgs.append(bg[p:p + g_n * d_n].reshape(g_n, d_n))
        dbgs.append(dbg[d:d + d_n])
        p += g_n * d_n
        d += d_n
    return fgs, bgs, dbgs, heat


def _encoded_files(files, batch=None, kind="JPEG"):
    """A list of bytes objects as the (const uint8_t* const*, const int64_t*) pair of the JPEG (and PNG) entry points."""
    files = list(files)
    if batch is not None and len(files) != batch:
        raise ValueError("expected %d %s files, got %d" % (batch, kind, len(files)))
    for i, f in enumerate(files):
        if not isinstance(f, bytes):
            raise ValueError("%s file %d must be a bytes object, got %s" % (kind, i, type(f).__name__))
    ptrs = (C.c_char_p * len(files))(*files)
    lens = (C.c_int64 * len(files))(*[len(f) for f in files])
    return ptrs, lens


def jpeg_info(data):
    """What a JPEG file's header says (``bod_jpeg_info``; host only): a dict of width, height, components, h_samp, v_samp (luma
    sampling), restart_interval, coef_count, supported, and ``reason`` -- why not, for a well-formed file outside the subset the
    library decodes (progressive, CMYK, ...; a file without SOI marker, such as a PNG, is reported the same way).  ``ValueError``
    for a corrupt header."""
    lib = _lib.load()
    if not isinstance(data, bytes):
        raise ValueError("a JPEG file must be a bytes object, got %s" % type(data).__name__)
    info = _lib.BodJpegInfo()
    _lib.check(lib, None, lib.bod_jpeg_info(data, len(data), C.byref(info)))
    out = {name: int(getattr(info, name)) for name, _ in _lib.BodJpegInfo._fields_}
    out["supported"] = bool(info.supported)
    reason = lib.bod_last_error(None)
    out["reason"] = "" if info.supported else (reason.decode() if reason else "")
    return out


def jpeg_entropy_decode(data):
    """The host half of the decoder alone (``bod_jpeg_entropy_decode``): (coefs int16 [coef_count] -- per component the blocks of
    its MCU-padded plane in raster block order, 64 per block in natural order --, quant uint16 [3, 64] in natural order)."""
    lib = _lib.load()
    info = jpeg_info(data)
    if not info["supported"]:
        raise ValueError(info["reason"])
    coefs = np.empty(info["coef_count"], np.int16)
    quant = np.zeros((3, 64), np.uint16)
    st = lib.bod_jpeg_entropy_decode(data, len(data), coefs.ctypes.data_as(C.POINTER(C.c_int16)), coefs.size,
                                     quant.ctypes.data_as(C.POINTER(C.c_uint16)))
    _lib.check(lib, None, st)
    return coefs, quant


def _decode_rgb(kind, files, device, threads):
    """``decode_jpeg_rgb`` / ``decode_png_rgb`` (``kind``: "jpeg" or "png")."""
    lib = _lib.load()
    ptrs, lens = _encoded_files(files, kind=kind.upper())
    n = len(lens)
    if n == 0:
        return []
    total = 0
    for i in range(n):
        info = (jpeg_info if kind == "jpeg" else png_info)(files[i])
        if not info["supported"]:
            raise ValueError("bod_%s_decode_rgb: frame %d is not a supported %s: %s" % (kind, i, kind.upper(), info["reason"]))
        total += 3 * info["width"] * info["height"]
    rgb = np.empty(total, np.uint8)
    src_hw = np.zeros((n, 2), np.int32)
    st = getattr(lib, "bod_%s_decode_rgb" % kind)(int(device), n, ptrs, lens, min(16, n) if threads is None else int(threads),
                                                  rgb.ctypes.data_as(C.POINTER(C.c_uint8)), rgb.size, iptr(src_hw))
    _lib.check(lib, None, st)
    out, off = [], 0
    for h, w in src_hw:
        out.append(rgb[off:off + 3 * h * w].reshape(h, w, 3))
        off += 3 * h * w
    return out


def decode_jpeg_rgb(files, device=0, threads=None):
    """JPEG files -> a list of uint8 [h, w, 3] RGB frames, decoded by the library (``bod_jpeg_decode_rgb``: Huffman decoding on
    ``threads`` host threads, default ``min(16, len(files))``, everything else on the device).  Equal to PIL's ``convert('RGB')``."""
    return _decode_rgb("jpeg", files, device, threads)


def _corruption_args(chains, n, frame_ids, ops_arrays=None):
    """(ops, ops_per_frame, frame_ids, taps, n_taps, luts, n_luts, qtables, n_qtables) as the corruption entry points take them,
    and the arrays that must outlive the call.  ``ops_arrays``: already packed (ops [n,P], taps, luts, qtables) instead of chains."""
    from . import corruptions
    ops, taps, luts, qts = corruptions.pack(chains, n) if ops_arrays is None else ops_arrays
    ops = np.ascontiguousarray(ops, corruptions.OP_DTYPE)
    taps = np.ascontiguousarray(taps, np.uint16).reshape(-1)
    luts = np.ascontiguousarray(luts, np.uint8).reshape(-1, 3, 256)
    qts = np.ascontiguousarray(qts, np.uint16).reshape(-1, 2, 64)
    if ops.ndim != 2 or ops.shape[0] != n:
        raise ValueError("expected ops of shape (%d, ops_per_frame), got %s" % (n, ops.shape))
    ids = None
    if frame_ids is not None:
        ids = np.ascontiguousarray(np.asarray(frame_ids, np.int64) & 0xFFFFFFFF, np.uint32).reshape(-1)
        if ids.size != n:
            raise ValueError("expected %d frame ids, got %d" % (n, ids.size))
    args = (ops.ctypes.data_as(C.POINTER(_lib.BodCorruptOp)), int(ops.shape[1]),
            None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_uint32)),
            taps.ctypes.data_as(C.POINTER(C.c_uint16)) if taps.size else None, int(taps.size),
            luts.ctypes.data_as(C.POINTER(C.c_uint8)) if luts.size else None, int(luts.shape[0]),
            qts.ctypes.data_as(C.POINTER(C.c_uint16)) if qts.size else None, int(qts.shape[0]))
    return args, (ops, ids, taps, luts, qts)


def corrupt_frames(frames, chains, frame_ids=None, seed=0, device=0, ops_arrays=None):
    """The corruption stage alone (``bod_corrupt_frames_u8``): ``frames`` is a list of uint8 [h,w,3] arrays of
    any sizes, ``chains`` one ``corruptions.Chain`` for all of them or a list of one per frame, ``frame_ids`` the ids the random
    ops key their numbers on (default 0, 1, ..).  Returns the corrupted frames as a list of uint8 [h,w,3] arrays.  A frame's result
    depends on its bytes, its chain, its id and the seed alone."""
    lib = _lib.load()
    buf, sizes = pack_ragged(frames)
    n = sizes.shape[0]
    args, _keep = _corruption_args(chains, n, frame_ids, ops_arrays)
    out = np.empty_like(buf)
    st = lib.bod_corrupt_frames_u8(int(device), n, buf.ctypes.data_as(C.POINTER(C.c_uint8)), iptr(sizes), *args,
                                   int(seed) & 0xFFFFFFFFFFFFFFFF, out.ctypes.data_as(C.POINTER(C.c_uint8)))
    _lib.check(lib, None, st)
    res, off = [], 0
    for h, w in sizes:
        res.append(out[off:off + 3 * h * w].reshape(h, w, 3))
        off += 3 * h * w
    return res


def png_info(data):
    """What a PNG file's header says (``bod_png_info``; host only): a dict of width, height, bit_depth, color_type, channels (bytes
    per pixel of the filtered scanlines), interlace, raw_bytes, supported, and ``reason`` -- why not, for a well-formed file outside
    the subset the library decodes (palette, 16-bit, interlaced, tRNS, ...; a file without the PNG signature, such as a JPEG, is
    reported the same way).  ``ValueError`` for a corrupt header or chunk layout."""
    lib = _lib.load()
    if not isinstance(data, bytes):
        raise ValueError("a PNG file must be a bytes object, got %s" % type(data).__name__)
    info = _lib.BodPngInfo()
    _lib.check(lib, None, lib.bod_png_info(data, len(data), C.byref(info)))
    out = {name: int(getattr(info, name)) for name, _ in _lib.BodPngInfo._fields_}
    out["supported"] = bool(info.supported)
    reason = lib.bod_last_error(None)
    out["reason"] = "" if info.supported else (reason.decode() if reason else "")
    return out


def png_inflate(data):
    """The host half of the decoder alone (``bod_png_inflate``): the filtered scanlines, uint8 [height, 1 + width * channels] --
    per row the filter-type byte, then the filtered bytes.  Equal to ``zlib.decompress`` of the file's concatenated IDAT chunks."""
    lib = _lib.load()
    info = png_info(data)
    if not info["supported"]:
        raise ValueError(info["reason"])
    raw = np.empty(info["raw_bytes"], np.uint8)
    _lib.check(lib, None, lib.bod_png_inflate(data, len(data), raw.ctypes.data_as(C.POINTER(C.c_uint8)), raw.size))
    return raw.reshape(info["height"], 1 + info["width"] * info["channels"])


def decode_png_rgb(files, device=0, threads=None):
    """PNG files -> a list of uint8 [h, w, 3] RGB frames, decoded by the library (``bod_png_decode_rgb``: inflate on ``threads``
    host threads, default ``min(16, len(files))``, the scanline filters on the device).  Equal to PIL's ``convert('RGB')``."""
    return _decode_rgb("png", files, device, threads)


def bench_png_decode(files, threads=16, iters=5, device=0):
    """The PNG decoder's two halves timed apart (``bod_bench_png_decode``; tests/tools/bench_png.py): (host_ms [iters] -- the host
    half of an upload of ``files`` on ``threads`` of the library's worker threads, by the host clock --, kernel_ms [iters] --
    ``png_unfilter_kernel`` alone on the batch, by events)."""
    lib = _lib.load()
    ptrs, lens = _encoded_files(files, kind="PNG")
    host, kernel = np.zeros(int(iters), np.float64), np.zeros(int(iters), np.float64)
    st = lib.bod_bench_png_decode(int(device), len(lens), ptrs, lens, int(threads), int(iters),
                                  host.ctypes.data_as(C.POINTER(C.c_double)), kernel.ctypes.data_as(C.POINTER(C.c_double)))
    _lib.check(lib, None, st)
    return host, kernel


def score_pairs(means, covs, targets, num_samples=1000, seed=0, first_row_id=0, device=0):
    """Scoring rules of n paired box Gaussians on the device (``bod_score_pairs``, score_kernels.hip): means [n,4], covs
    [n,4,4] (lower triangle read), targets [n,4].  Returns (out [n,8] float64 = nll, squared Mahalanobis distance, energy
    score, four PITs, ln det; status [n] int32: 0 ok, 1 not positive definite, 2 non-finite input -- such rows are NaN).
    Row i draws its normals from the id ``first_row_id + i`` alone (scoring_rules.score_pairs_np is the host twin)."""
    lib = _lib.load()
    means = np.ascontiguousarray(means, dtype=np.float64).reshape(-1, 4)
    covs = np.ascontiguousarray(covs, dtype=np.float64).reshape(-1, 4, 4)
    targets = np.ascontiguousarray(targets, dtype=np.float64).reshape(-1, 4)
    n = means.shape[0]
    if covs.shape[0] != n or targets.shape[0] != n:
        raise ValueError("means, covs and targets must have one row per pair")
    out = np.empty((n, 8), np.float64)
    status = np.zeros(n, np.int32)
    st = lib.bod_score_pairs(device, n, _lib.dptr(means), _lib.dptr(covs), _lib.dptr(targets), int(num_samples),
                             int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_row_id) & 0xFFFFFFFFFFFFFFFF, _lib.dptr(out), iptr(status))
    _lib.check(lib, None, st)
    return out, status

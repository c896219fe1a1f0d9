"""GPU: every upload route on ONE handle, so that they share its staging buffers, pinned buffers, decode slots and copy stream
(the tests of each route run it on a handle of its own).  A fixed sequence of uploads -- uniform, ragged, augmented, JPEG and PNG;
synchronous and into both pipelined buffers; two of them consuming an upload corruption -- runs three times: on small frames, on
larger ones, on small ones again.  Every buffer a route owns is thereby allocated, regrown and reused, each time while an upload
into the other image buffer may still be running.  The image buffer after every synchronous upload, and both image buffers after
each round's synchronize(), equal what a second handle holds after the ragged / augmented upload of the same decoded frames."""
import io

import numpy as np
import pytest

from conftest import ANCHOR_CFG, BAYES_CFG, NMS_CFG
import png_corpus

pytestmark = pytest.mark.gpu

HW = (128, 128)
B = 3
SMALL = [(40, 60), (37, 52), (44, 31)]
LARGE = [(94, 150), (128, 128), (61, 77)]
AUG = [dict(flip=1, scale=1.25, off_y=0.25, off_x=0.75, gain=1.1, bias=-6.0), dict(scale=0.8, off_y=1.0, off_x=0.0),
       dict(flip=1, gain=0.9, bias=4.0)]
FRAME_IDS, SEED = [7, 8, 9], 3


def _engine():
    from bayes_od_rc_amd import synthetic
    from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
    from bayes_od_rc_amd.engine import Engine, make_config
    eng = Engine(make_config(HW, batch=B, mc_samples=3, bayes_od_config=BAYES_CFG, nms_config=NMS_CFG, use_full_covar=True,
                             dataset_name="kitti", orig_size=HW))
    eng.load_weights(synthetic.make_weights(cls_fg_bias=-1.0))
    eng.set_anchors(FpnAnchorGenerator(ANCHOR_CFG).generate_all((HW[0], HW[1], 3)))
    return eng


def _chain():
    from bayes_od_rc_amd import corruptions as c
    return c.concat(c.op_jpeg(50), c.op_gaussian_noise(12.0))


def _scene(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.clip(np.stack([2 * xx, 2 * yy, 255 - xx - yy], axis=2) + rng.integers(-60, 60, (h, w, 3)), 0, 255).astype(np.uint8)


def _round_data(sizes, seed):
    """The frames of one round, per kind of upload: what is sent and the decoded RGB frames it stands for."""
    from PIL import Image
    d = {}
    h, w = sizes[0]
    uniform = np.stack([_scene(h, w, seed + k) for k in range(B)])
    d["u8"] = (uniform, list(uniform))
    ragged = [_scene(h, w, seed + 10 + k) for k, (h, w) in enumerate(sizes)]
    d["ragged"] = (ragged, ragged)
    d["augmented"] = (ragged[::-1], ragged[::-1])
    files, rgbs = [], []
    for k, ((h, w), kw) in enumerate(zip(sizes, (dict(subsampling="4:2:0"), dict(subsampling="4:2:2", restart_marker_blocks=1), dict()))):
        a = _scene(h, w, seed + 20 + k)
        buf = io.BytesIO()
        (Image.fromarray(a) if k < 2 else Image.fromarray(a[:, :, 0], "L")).save(buf, "JPEG", quality=90, **kw)
        files.append(buf.getvalue())
        rgbs.append(np.asarray(Image.open(io.BytesIO(files[-1])).convert("RGB")))
    d["jpeg"] = (files, rgbs)
    files, rgbs = [], []
    for k, ((h, w), ct, pattern) in enumerate(zip(sizes, (2, 6, 0), ([4, 3, 2, 1, 0], [3, 4], [4]))):
        arr = png_corpus.make_array(h, w, ct, seed + 30 + k)
        files.append(png_corpus.write_png(arr, ct, pattern, ("level6", "fixed", "stored")[k], (None, 7, 4096)[k]))
        rgbs.append(png_corpus.expected_rgb(arr, ct))
    d["png"] = (files, rgbs)
    return d


# (kind, buffer -- None: synchronous --, augmented, corrupted).  The synchronous route writes image buffer 0, so its uploads come
# while only buffer 1 has uploads in flight; a synchronous upload has completed when it returns, and is compared there and then.
SEQUENCE = [
    ("ragged", 1, False, False),
    ("u8", None, False, False),
    ("jpeg", 1, True, False),
    ("png", None, False, False),
    ("png", 1, False, False),
    ("jpeg", None, False, True),
    ("augmented", 1, True, False),
    ("augmented", None, True, False),
    ("u8", 1, False, False),
    ("ragged", None, False, False),
    ("png", 0, False, True),
    ("png", 1, True, False),
    ("jpeg", 0, True, False),
    ("ragged", 0, False, False),
    ("jpeg", 1, False, False),
    ("u8", 0, False, False),
]
TAIL = 10                                # from here on image buffer 0 has pipelined uploads in flight: no synchronous upload


def _upload(eng, kind, sent, buffer, aug, corrupt, means):
    if corrupt:
        eng.set_upload_corruption(_chain(), FRAME_IDS, seed=SEED)
    if kind == "u8":
        if buffer is None:
            eng.upload_frames_u8(sent, means, aspect_resize=True)
        else:
            eng.upload_frames_u8_async(sent, buffer, means, aspect_resize=True)
    elif kind == "ragged":
        if buffer is None:
            eng.upload_frames_u8_ragged(sent, means, aspect_resize=True)
        else:
            eng.upload_frames_u8_ragged_async(sent, buffer, means, aspect_resize=True)
    elif kind == "augmented":
        if buffer is None:
            eng.upload_frames_u8_augmented(sent, AUG, means, aspect_resize=True)
        else:
            eng.upload_frames_u8_augmented_async(sent, AUG, buffer, means, aspect_resize=True)
    else:
        name = "upload_frames_%s%s" % (kind, "" if buffer is None else "_async")
        args = (sent,) if buffer is None else (sent, buffer)
        hw = getattr(eng, name)(*args, means, aspect_resize=True, aug=AUG if aug else None)
        return hw


def test_all_routes_share_one_handle_through_growing_and_shrinking_frames():
    from bayes_od_rc_amd import constants
    means = constants.MEANS_DICT["Kitti"]
    eng, ref = _engine(), _engine()
    expected = {}

    def want(r, data, kind, aug, corrupt):
        key = (r, kind, aug, corrupt)
        if key not in expected:
            if corrupt:
                ref.set_upload_corruption(_chain(), FRAME_IDS, seed=SEED)
            if aug:
                ref.upload_frames_u8_augmented(data[kind][1], AUG, means, aspect_resize=True)
            else:
                ref.upload_frames_u8_ragged(data[kind][1], means, aspect_resize=True)
            expected[key] = ref.get_images().copy()
        return expected[key]

    keep = []                                                           # the pipelined uniform upload reads its array until it is collected
    for r, (sizes, seed) in enumerate(((SMALL, 100), (LARGE, 200), (SMALL, 300))):
        data = _round_data(sizes, seed)
        keep.append(data)
        # the pipelined tail starts two steps later in every round, so that each round leaves other uploads in the two buffers
        order = SEQUENCE[:TAIL] + SEQUENCE[TAIL + 2 * r:] + SEQUENCE[TAIL:TAIL + 2 * r]
        last = {}
        for step, (kind, buffer, aug, corrupt) in enumerate(order):
            hw = _upload(eng, kind, data[kind][0], buffer, aug, corrupt, means)
            if hw is not None:
                assert hw.tolist() == [list(f.shape[:2]) for f in data[kind][1]], (r, step)
            if buffer is None:
                assert np.array_equal(eng.get_images(), want(r, data, kind, aug, corrupt)), (r, step, kind)
            else:
                last[buffer] = (step, kind, aug, corrupt)
        eng.synchronize()
        for buffer, (step, kind, aug, corrupt) in sorted(last.items()):
            assert np.array_equal(eng.get_images(buffer), want(r, data, kind, aug, corrupt)), (r, step, kind, buffer)
    # the rounds differ, and so do the plain, augmented and corrupted forms of one round's frames
    assert not np.array_equal(want(0, keep[0], "png", False, False), want(2, keep[2], "png", False, False))
    assert not np.array_equal(want(1, keep[1], "png", False, False), want(1, keep[1], "png", False, True))
    assert not np.array_equal(want(1, keep[1], "jpeg", False, False), want(1, keep[1], "jpeg", True, False))
    eng.close()
    ref.close()

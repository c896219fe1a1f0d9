"""GPU: training-time augmentation on the device -- bod_upload_frames_u8_augmented[_async] (preprocess_augment_kernel: flip,
scale, off-centre crop / pad, gain and bias) bit-exact against the NumPy float32 restatement of tests/augment_reference.py
(built on oracle/preprocess.py), its refusals, the pipelined form, and a training step on an augmented upload.

Network input 128x416 (tests/test_gpu_mixed_sizes.py's).  Source sizes: (94,311) odd width, (92,306) even width, (200,150)
narrower and (100,500) wider than the network; (2,500) resizes to one row at scale 0.5."""
import numpy as np
import pytest

from augment_reference import augmented_boxes, augmented_frame, geometry, record
from conftest import ANCHOR_CFG

pytestmark = pytest.mark.gpu

HW = (128, 416)
FOUR = [(94, 311), (92, 306), (200, 150), (100, 500)]


def _u8(sizes, seed):
    """Random frames with a few pixels forced to 0 and 255 (the corners among them: the first / last row and column)."""
    rng = np.random.default_rng(seed)
    out = []
    for hw in sizes:
        f = rng.integers(0, 256, size=tuple(hw) + (3,), dtype=np.uint8)
        f[0, 0], f[-1, -1], f[0, -1], f[-1, 0] = 0, 255, 255, 0
        f[hw[0] // 2, hw[1] // 3], f[hw[0] // 3, hw[1] // 2] = 0, 255
        out.append(f)
    return out


def _means():
    from bayes_od_rc_amd import constants
    return constants.MEANS_DICT['Kitti']


@pytest.fixture(scope="module")
def eng():
    from bayes_od_rc_amd.engine import Engine, make_config
    e = Engine(make_config(HW, batch=4, mc_samples=2))
    yield e
    e.close()


def _expect(eng, frames, recs, aspect):
    """Uploads augmented and compares every frame with the restatement, bit for bit; returns the images."""
    eng.upload_frames_u8_augmented(frames, recs, _means(), aspect_resize=aspect)
    got = eng.get_images()
    for b, (f, r) in enumerate(zip(frames, recs)):
        ref = augmented_frame(f, HW, _means(), aspect, r)
        assert got[b].shape == ref.shape
        assert got[b].tobytes() == ref.tobytes(), (b, r, float(np.abs(got[b] - ref).max()), int((got[b] != ref).sum()))
    return got


def test_identity_records_equal_the_ragged_upload(eng):
    frames = _u8(FOUR, 1)
    eng.upload_frames_u8_ragged(frames, _means(), aspect_resize=True)
    ragged = eng.get_images()
    got = _expect(eng, frames, [record()] * 4, True)
    assert got.tobytes() == ragged.tobytes()
    flat = _u8([HW] * 4, 2)
    eng.upload_frames_u8_ragged(flat, _means(), aspect_resize=False)
    ragged = eng.get_images()
    got = _expect(eng, flat, [record()] * 4, False)
    assert got.tobytes() == ragged.tobytes()


def test_flip_is_the_upload_of_the_mirrored_sources(eng):
    frames = _u8(FOUR, 3)                                                      # odd and even widths, mixed sizes in one batch
    mirrored = [np.ascontiguousarray(f[:, ::-1]) for f in frames]
    eng.upload_frames_u8_ragged(mirrored, _means(), aspect_resize=True)
    want = eng.get_images()
    eng.upload_frames_u8_augmented(frames, [record(flip=1)] * 4, _means(), aspect_resize=True)
    got = eng.get_images()
    assert got.tobytes() == want.tobytes()
    assert got.tobytes() != _expect(eng, frames, [record()] * 4, True).tobytes()
    # with everything else switched on, and only some frames of the batch flipped
    recs = [record(flip=1, scale=1.3, off_y=0.2, off_x=0.9, gain=1.1, bias=4.0), record(scale=0.8, off_y=1.0, gain=0.9),
            record(flip=1, scale=0.9, off_x=0.0, bias=-9.0), record(flip=1, scale=1.2, off_y=0.6, off_x=0.4)]
    eng.upload_frames_u8_augmented(mirrored, [dict(r, flip=0) for r in recs[:1]] + [recs[1]] + [dict(r, flip=0) for r in recs[2:]],
                                   _means(), aspect_resize=True)
    want = eng.get_images()
    want[1] = augmented_frame(frames[1], HW, _means(), True, recs[1])          # (frame 1 is not flipped: its mirrored upload is another image)
    got = _expect(eng, frames, recs, True)
    assert got.tobytes() == want.tobytes()
    # no resize at all (frames at the network size): the mirror alone
    flat = _u8([HW] * 4, 4)
    eng.upload_frames_u8_ragged([np.ascontiguousarray(f[:, ::-1]) for f in flat], _means(), aspect_resize=False)
    want = eng.get_images()
    got = _expect(eng, flat, [record(flip=1)] * 4, False)
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("scale", [0.7, 1.4])
def test_scale_and_placement(eng, scale):
    """0.7 pads every frame on both axes; 1.4 crops (94,311) and (92,306) on both, crops (200,150) in y while it pads it in x,
    and pads (100,500) in y while it crops it in x.  Offsets 0 and 1 put the first / last source row and column on the frame's
    edge."""
    frames = _u8(FOUR, 5)
    for b, hw in enumerate(FOUR):
        rh, rw = geometry(hw, HW, True, scale)[:2]
        if scale < 1:
            assert rh < HW[0] and rw < HW[1]
        elif b == 2:
            assert rh > HW[0] and rw < HW[1]
        elif b == 3:
            assert rh < HW[0] and rw > HW[1]
        else:
            assert rh > HW[0] and rw > HW[1]
    for oy, ox in ((0.0, 0.0), (1.0, 1.0), (0.37, 0.37), (0.0, 1.0)):
        _expect(eng, frames, [record(scale=scale, off_y=oy, off_x=ox)] * 4, True)
    if scale > 1:                                                               # the crop at offset 1 ends on the last resized row / column
        rh, rw, cy, cx, _, _ = geometry(FOUR[0], HW, True, scale, 1.0, 1.0)
        assert cy + HW[0] == rh and cx + HW[1] == rw


def test_one_pixel_axis_and_the_route_without_aspect_resize(eng):
    frames = _u8([(2, 500), (94, 311), (2, 500), (200, 150)], 6)
    assert geometry((2, 500), HW, True, 0.5)[:2] == (1, 208)
    _expect(eng, frames, [record(scale=0.5, off_y=1.0), record(scale=0.5), record(flip=1, scale=0.5, off_y=0.0, off_x=1.0), record(scale=0.5)], True)
    # frames at the network size scaled about themselves: shrunk and padded, grown and cropped, untouched (no resize at all)
    flat = _u8([HW] * 4, 7)
    assert geometry(HW, HW, False, 0.75)[:2] == (96, 312) and geometry(HW, HW, False, 1.3)[:2] == (166, 541)
    _expect(eng, flat, [record(scale=0.75, off_y=0.0, off_x=1.0), record(flip=1, scale=1.3, off_y=1.0, off_x=0.0),
                        record(gain=1.2, bias=-3.0), record(flip=1, scale=0.75, off_y=0.37, off_x=0.37, gain=0.8, bias=11.0)], False)


def test_gain_and_bias_clamp_and_leave_the_padding_alone(eng):
    frames = _u8(FOUR, 8)
    recs = [record(gain=1.9, bias=-60.0), record(gain=-3.0, bias=300.0), record(scale=0.7, off_y=0.3, off_x=0.8, gain=3.0, bias=-300.0),
            record(flip=1, gain=0.5, bias=200.5)]
    got = _expect(eng, frames, recs, True)
    bgr_means = np.asarray(_means(), np.float32)[::-1]
    for b, (f, r) in enumerate(zip(frames, recs)):
        rh, rw, cy, cx, py, px = geometry(f.shape[:2], HW, True, r["scale"], r["off_y"], r["off_x"])
        vis = np.zeros(HW, bool)
        vis[py:py + min(rh, HW[0]), px:px + min(rw, HW[1])] = True
        assert (~vis).any()                                                     # every frame has padding ...
        assert (got[b][~vis] == -bgr_means).all()                               # ... which is exactly -mean
        v = got[b][vis] + bgr_means
        assert v.min() >= -1e-4 and v.max() <= 255 + 1e-4
        if b < 3:                                                               # clamped at both ends
            assert (got[b][vis] == -bgr_means).all(axis=-1).any() and (got[b][vis] == np.float32(255) - bgr_means).all(axis=-1).any()


def test_refusals_name_the_frame_and_keep_the_previous_upload(eng):
    frames = _u8(FOUR, 9)
    eng.upload_frames_u8_augmented(frames, [record(flip=1, scale=0.9)] * 4, _means())
    before = eng.get_images()
    lib, BOD_ERR_INVALID_ARG = eng.lib, 1
    for bad in (dict(flip=2), dict(flip=-1), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan")), dict(scale=float("inf")),
                dict(off_y=-0.01), dict(off_y=1.01), dict(off_x=float("nan")), dict(off_x=2.0), dict(gain=float("inf")),
                dict(gain=float("nan")), dict(bias=float("-inf")), dict(bias=float("nan")), dict(scale=1e9)):
        recs = [record(), record(), record(**bad), record()]
        with pytest.raises(ValueError, match="bod_upload_frames_u8_augmented: frame 2"):
            eng.upload_frames_u8_augmented(frames, recs, _means())
        with pytest.raises(ValueError, match="bod_upload_frames_u8_augmented_async: frame 2"):
            eng.upload_frames_u8_augmented_async(frames, recs, 1, _means())
    # the status itself, and the message through bod_last_error
    import ctypes as C
    from bayes_od_rc_amd import _lib
    from bayes_od_rc_amd.engine import augment_records, pack_ragged
    buf, sizes = pack_ragged(frames, 4)
    rec = augment_records([record(), record(), record(flip=3), record()], 4)
    m = np.asarray(_means(), np.float32)
    st = lib.bod_upload_frames_u8_augmented(eng.h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), _lib.iptr(sizes), _lib.fptr(m), 1,
                                            rec.ctypes.data_as(C.POINTER(_lib.BodAugment)))
    assert st == BOD_ERR_INVALID_ARG == _lib.BOD_ERR_INVALID_ARG and b"frame 2" in lib.bod_last_error(eng.h)
    # a degenerate resize, and the ragged uploads' errors
    with pytest.raises(ValueError, match="frame 1.*degenerate"):
        eng.upload_frames_u8_augmented([frames[0], np.zeros((1, 2000, 3), np.uint8)] + frames[2:], [record()] * 4, _means())
    with pytest.raises(ValueError, match="frame 0 is 94x311"):
        eng.upload_frames_u8_augmented(frames, [record()] * 4, _means(), aspect_resize=False)
    with pytest.raises(ValueError, match="expected 4 frames"):
        eng.upload_frames_u8_augmented(frames[:3], [record()] * 3, _means())
    with pytest.raises(ValueError, match="expected 4 augmentation records"):
        eng.upload_frames_u8_augmented(frames, [record()] * 3, _means())
    with pytest.raises(ValueError, match="buffer must be 0 or 1"):
        eng.upload_frames_u8_augmented_async(frames, [record()] * 4, 2, _means())
    assert eng.get_images().tobytes() == before.tobytes()


def test_pipelined_form_equals_the_synchronous_one():
    from bayes_od_rc_amd import synthetic
    from bayes_od_rc_amd.engine import Engine, make_config
    frames = _u8(FOUR[:3], 10)
    recs = [record(flip=1, scale=1.3, off_y=0.1, off_x=0.7, gain=1.1, bias=-5.0), record(scale=0.8, off_y=0.9, off_x=0.2),
            record(flip=1, gain=0.85, bias=12.0)]
    e = Engine(make_config(HW, batch=3, mc_samples=2))
    e.load_weights(synthetic.make_weights())
    e.upload_frames_u8_augmented(frames, recs, _means())
    want = e.get_images()
    e.forward(None, seed=2, first_image_id=6)
    want_raw = [a.copy() for a in e.get_raw() if a is not None]
    e.upload_frames_u8_ragged(frames, _means())                                 # (buffer 0 holds something else now)
    e.upload_frames_u8_augmented_async(frames, recs, 1, _means())
    e.forward(None, seed=2, first_image_id=6, image_buffer=1)
    e.synchronize()
    got = e.get_images(image_buffer=1)
    assert got.tobytes() == want.tobytes()
    for b, (f, r) in enumerate(zip(frames, recs)):
        assert got[b].tobytes() == augmented_frame(f, HW, _means(), True, r).tobytes(), b
    for a, b in zip(want_raw, [a for a in e.get_raw() if a is not None]):
        assert np.isfinite(a).all() and a.tobytes() == b.tobytes()
    e.close()


def test_training_step_on_an_augmented_upload():
    """train_step_boxes on the frames the augmented upload left on the device, with the boxes of augment_boxes, against the same
    step fed the HOST copy of those frames and the same boxes; same weights (no update is applied), same seed.  The three
    losses that depend on the frames are compared bitwise; the regularisation term is summed with float atomics and is held
    to the 1e-5 tests/test_gpu_mixed_sizes.py holds it to, and the total to the sum of its parts."""
    from bayes_od_rc_amd import synthetic
    from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
    from bayes_od_rc_amd.engine import Engine, augment_boxes, make_config
    hw = (64, 64)                                                               # tests/test_gpu_train_from_boxes.py's smallest
    sizes = [(50, 81), (90, 60)]
    frames = _u8(sizes, 11)
    recs = [record(flip=1, scale=1.25, off_y=0.3, off_x=0.8, gain=1.1, bias=-6.0), record(scale=0.9, off_y=1.0, off_x=0.0, gain=0.9, bias=8.0)]
    src_boxes = [np.asarray([[5, 10, 40, 60], [20, 50, 45, 80]], np.float32), np.asarray([[10, 5, 70, 50], [85, 1, 89, 4]], np.float32)]
    src_classes = [np.eye(8, dtype=np.float32)[[0, 2]], np.eye(8, dtype=np.float32)[[1, 3]]]
    boxes, classes = augment_boxes(sizes, hw, recs, src_boxes, src_classes, aspect_resize=True, min_visible=0.25)
    for i in range(2):
        wb, wc = augmented_boxes(sizes[i], hw, True, recs[i], src_boxes[i], src_classes[i], 0.25)
        assert boxes[i].tobytes() == wb.tobytes() and np.array_equal(classes[i], wc)
    print("boxes", [b.tolist() for b in boxes])
    eng = Engine(make_config(hw, batch=2, mc_samples=1, training=True))
    eng.load_weights(synthetic.make_weights(cls_fg_bias=-2.0))
    eng.set_anchors(FpnAnchorGenerator(ANCHOR_CFG).generate_all(hw + (3,)))
    eng.upload_frames_u8_augmented(frames, recs, _means())
    got = eng.train_step_boxes(None, boxes, classes, 0.5, 0.4, seed=3, first_image_id=8, apply_update=False)
    host = eng.get_images()
    for b in range(2):
        assert host[b].tobytes() == augmented_frame(frames[b], hw, _means(), True, recs[b]).tobytes(), b
    ref = eng.train_step_boxes(host, boxes, classes, 0.5, 0.4, seed=3, first_image_id=8, apply_update=False)
    print("losses", got, ref)
    assert np.isfinite(got["total_loss"]) and got["reg_loss"] > 0
    for key in ("cls_loss", "reg_loss", "covariance_loss"):
        assert got[key] == ref[key], (key, got[key], ref[key])
    assert abs(got["regularization_loss"] - ref["regularization_loss"]) <= 1e-5 * ref["regularization_loss"]
    for out in (got, ref):
        assert out["total_loss"] == out["cls_loss"] + 1.0 * (out["reg_loss"] + out["covariance_loss"]) + out["regularization_loss"]
    eng.close()

"""GPU: PNG frames decoded inside the library -- inflate on host threads, png_unfilter_kernel on the device -- against
the arrays the corpus files were written from (tests/png_corpus.py; PNG is lossless), byte for byte.  Then the upload routes: the
image buffer, the pipelined form and one infer after bod_upload_frames_png equal those after the ragged / augmented upload of the
same frames, with and without an upload corruption; a bad frame is refused by name and changes nothing; datasets.upload_frames sends
all-PNG, all-JPEG and mixed batches down their routes with identical image buffers."""
import io
import zlib

import numpy as np
import pytest

from conftest import ANCHOR_CFG, BAYES_CFG, NMS_CFG
import png_corpus
import png_reference

pytestmark = pytest.mark.gpu

HW = (128, 128)


@pytest.fixture(scope="module")
def corpus():
    return png_corpus.load()


def _explain(c, got):
    """Where a decode leaves the expected RGB, and whether the NumPy restatement of the filters agrees with the expectation."""
    ch = png_corpus.CHANNELS[c.color_type]
    raw = np.frombuffer(zlib.decompress(png_corpus.idat_stream(c.data)), np.uint8).reshape(c.height, 1 + c.width * ch)
    ref = png_reference.decode(raw, c.width, ch)
    bad = np.argwhere((got != c.rgb).any(axis=2)) if got.shape == c.rgb.shape else []
    return "%r: shape %s, %d pixels differ, first at %s (filter type %s); restatement equals the expectation: %s" % (
        c, got.shape, len(bad), None if not len(bad) else bad[0].tolist(), None if not len(bad) else int(raw[bad[0][0], 0]),
        np.array_equal(ref, c.rgb))


def test_every_corpus_file_decodes_to_its_expected_rgb(corpus):
    from bayes_od_rc_amd.engine import decode_png_rgb
    for c in corpus:
        (got,) = decode_png_rgb([c.data])
        assert got.shape == c.rgb.shape and np.array_equal(got, c.rgb), _explain(c, got)


@pytest.mark.parametrize("batch", [1, 3, 64])
def test_batches_of_mixed_sizes_types_and_filters(corpus, batch):
    from bayes_od_rc_amd.engine import decode_png_rgb
    order = np.random.default_rng(batch).permutation(len(corpus))           # neighbours differ in size, colour type and filter pattern
    picked = [corpus[i] for i in order[:max(batch, 6)]]
    assert len({(c.height, c.width) for c in picked}) >= 4 and len({c.color_type for c in picked}) == 4
    for first in range(0, len(picked) - batch + 1, batch):
        group = picked[first:first + batch]
        one = decode_png_rgb([c.data for c in group], threads=1)
        four = decode_png_rgb([c.data for c in group], threads=4)
        assert len(one) == len(four) == batch
        for c, a, b in zip(group, one, four):
            assert a.shape == c.rgb.shape and np.array_equal(a, c.rgb), _explain(c, a)
            assert np.array_equal(a, b), c


def _engine(batch, kitti):
    from bayes_od_rc_amd import synthetic
    from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
    from bayes_od_rc_amd.engine import Engine, make_config
    kw = dict(dataset_name="kitti", orig_size=HW) if kitti else {}
    eng = Engine(make_config(HW, batch=batch, mc_samples=3, bayes_od_config=BAYES_CFG, nms_config=NMS_CFG, use_full_covar=True, **kw))
    eng.load_weights(synthetic.make_weights(cls_fg_bias=-1.0))             # the detecting synthetic weights of the mixed-size tests
    eng.set_anchors(FpnAnchorGenerator(ANCHOR_CFG).generate_all((HW[0], HW[1], 3)))
    return eng


def _frames(sizes):
    """One PNG file per (height, width, colour type, filter pattern) with the RGB it decodes to."""
    files, rgbs = [], []
    for k, (h, w, ct, pattern) in enumerate(sizes):
        arr = png_corpus.make_array(h, w, ct, 40 + k)
        # a scene rather than noise, so that the synthetic weights detect something: a bright box on the array's gradient
        arr[h // 4:h // 2, w // 4:w // 2, :png_corpus.CHANNELS[ct] if ct in (2, 6) else 1] = 240
        files.append(png_corpus.write_png(arr, ct, pattern, ("level6", "fixed", "stored")[k % 3], (None, 7, 4096)[k % 3]))
        rgbs.append(png_corpus.expected_rgb(arr, ct))
    return files, rgbs


def _detections(eng, image_buffer=None):
    eng.infer(None, seed=5, first_image_id=40, image_buffer=image_buffer)
    return {k: v.copy() for k, v in eng.get_detections_batch().items()}


def _same(a, b):
    if not np.array_equal(a["num"], b["num"]):
        return False
    return all(np.array_equal(a[key][img, :k], b[key][img, :k]) for img, k in enumerate(a["num"]) for key in ("scores", "means", "covs", "counts"))


AUG = [dict(flip=1, scale=1.25, off_y=0.25, off_x=0.75, gain=1.1, bias=-6.0), dict(scale=0.8, off_y=1.0, off_x=0.0),
       dict(flip=1, gain=0.9, bias=4.0)]


def _chain():
    from bayes_od_rc_amd import corruptions as c
    return c.concat(c.op_jpeg(50), c.op_gaussian_noise(12.0))


def _check_routes(eng, files, rgbs, means, aspect_resize):
    # synchronous: image buffer, src_hw and one infer's detections
    eng.upload_frames_u8_ragged(rgbs, means, aspect_resize=aspect_resize)
    ref_images = eng.get_images().copy()
    ref_dets = _detections(eng)
    src_hw = eng.upload_frames_png(files, means, aspect_resize=aspect_resize)
    assert src_hw.tolist() == [list(r.shape[:2]) for r in rgbs]
    assert np.array_equal(eng.get_images(), ref_images)
    dets = _detections(eng)
    print("detections per frame", ref_dets["num"].tolist(), dets["num"].tolist())
    assert _same(dets, ref_dets)
    # threads: one worker or several, the same bytes
    eng.upload_frames_png(files, means, aspect_resize=aspect_resize, threads=1)
    assert np.array_equal(eng.get_images(), ref_images)
    # augmented
    eng.upload_frames_u8_augmented(rgbs, AUG, means, aspect_resize=aspect_resize)
    ref_aug = eng.get_images().copy()
    ref_aug_dets = _detections(eng)
    assert not np.array_equal(ref_aug, ref_images)
    eng.upload_frames_png(files, means, aspect_resize=aspect_resize, aug=AUG)
    assert np.array_equal(eng.get_images(), ref_aug)
    assert _same(_detections(eng), ref_aug_dets)
    # an upload corruption set: consumed by the PNG upload as by the ragged one
    eng.set_upload_corruption(_chain(), [7, 8, 9], seed=3)
    eng.upload_frames_u8_ragged(rgbs, means, aspect_resize=aspect_resize)
    ref_cor = eng.get_images().copy()
    ref_cor_dets = _detections(eng)
    assert not np.array_equal(ref_cor, ref_images)
    eng.set_upload_corruption(_chain(), [7, 8, 9], seed=3)
    eng.upload_frames_png(files, means, aspect_resize=aspect_resize)
    assert np.array_equal(eng.get_images(), ref_cor)
    assert _same(_detections(eng), ref_cor_dets)
    eng.upload_frames_png(files, means, aspect_resize=aspect_resize)               # consumed: the plain frames again
    assert np.array_equal(eng.get_images(), ref_images)
    # pipelined, into both buffers (twice into buffer 1: the second inflate waits for the first copy out of its staging)
    for buffer, threads in ((0, None), (1, 2), (1, 1)):
        hw = eng.upload_frames_png_async(files, buffer, means, aspect_resize=aspect_resize, threads=threads)
        assert np.array_equal(hw, src_hw)
        eng.synchronize()
        assert np.array_equal(eng.get_images(buffer), ref_images), buffer
        assert _same(_detections(eng, image_buffer=buffer), ref_dets), buffer
    eng.upload_frames_png_async(files, 1, means, aspect_resize=aspect_resize, aug=AUG)
    eng.synchronize()
    assert np.array_equal(eng.get_images(1), ref_aug)
    eng.set_upload_corruption(_chain(), [7, 8, 9], seed=3)
    eng.upload_frames_png_async(files, 0, means, aspect_resize=aspect_resize)
    eng.synchronize()
    assert np.array_equal(eng.get_images(0), ref_cor)
    with pytest.raises(ValueError, match="buffer must be 0 or 1"):
        eng.upload_frames_png_async(files, 2, means, aspect_resize=aspect_resize)


def test_kitti_style_upload_equals_the_ragged_upload_of_the_same_frames():
    """Frames of three sizes and colour types, each resized and padded by its own geometry and rescaled by its own factors."""
    from bayes_od_rc_amd import constants
    files, rgbs = _frames([(94, 150, 2, [4, 3, 2, 1, 0]), (128, 128, 6, [3, 4]), (61, 77, 0, [4])])
    eng = _engine(3, kitti=True)
    _check_routes(eng, files, rgbs, constants.MEANS_DICT["Kitti"], True)
    eng.close()


def test_upload_at_the_network_size_without_rescale():
    files, rgbs = _frames([(128, 128, 2, [4]), (128, 128, 4, [1, 2]), (128, 128, 6, [4, 3, 2, 1, 0])])
    eng = _engine(3, kitti=False)
    _check_routes(eng, files, rgbs, None, False)
    # a frame that is not at the network size is the ragged upload's geometry error, naming the frame
    small, _ = _frames([(64, 128, 2, [4])])
    before = eng.get_images().copy()
    with pytest.raises(ValueError, match="frame 1 is 64x128 but the handle expects 128x128"):
        eng.upload_frames_png([files[0], small[0], files[2]], aspect_resize=False)
    assert np.array_equal(eng.get_images(), before)
    eng.close()


def test_a_bad_frame_is_refused_by_index_and_changes_nothing():
    from bayes_od_rc_amd import constants
    files, _ = _frames([(33, 47, 2, [4]), (31, 5, 6, [3]), (64, 48, 0, [1])])
    corrupt, _ = png_corpus.corrupt_files()
    unsupported = png_corpus.unsupported_files()
    eng = _engine(3, kitti=True)
    means = constants.MEANS_DICT["Kitti"]
    eng.upload_frames_png(files, means)
    before = eng.get_images().copy()
    # one corrupt and one unsupported file in a batch: the first bad index is named, whichever kind it is
    for batch, why in (([files[0], corrupt["flipped Adler-32"][0], unsupported["palette"][0]], "frame 2 .*not a supported PNG.*palette"),
                       ([corrupt["filter byte 5"][0], files[1], files[2]], "frame 0 is corrupt.*filter type"),
                       ([files[0], unsupported["interlaced"][0], corrupt["truncated IDAT"][0]], "frame 1 .*interlaced"),
                       ([files[0], files[1], corrupt["one byte long"][0]], "frame 2 is corrupt.*more bytes"),
                       ([files[0], corrupt["flipped CRC"][0], files[2]], "frame 1 is corrupt.*CRC")):
        with pytest.raises(ValueError, match=why):
            eng.upload_frames_png(batch, means)
        assert np.array_equal(eng.get_images(), before), why
        with pytest.raises(ValueError, match=why):
            eng.upload_frames_png_async(batch, 0, means)
        eng.synchronize()
        assert np.array_equal(eng.get_images(), before), why
    with pytest.raises(ValueError, match="expected 3 PNG files"):
        eng.upload_frames_png([files[0]], means)
    eng.close()


def test_datasets_upload_frames_routes_png_jpeg_and_mixed_batches(monkeypatch):
    from PIL import Image
    from bayes_od_rc_amd import constants, datasets
    from bayes_od_rc_amd.engine import Engine
    pngs, rgbs = _frames([(94, 150, 2, [4, 3]), (128, 128, 6, [2]), (61, 77, 0, [4])])
    jpegs, jpeg_rgbs = [], []
    for r in rgbs:
        buf = io.BytesIO()
        Image.fromarray(r).save(buf, "JPEG", quality=90)
        jpegs.append(buf.getvalue())
        jpeg_rgbs.append(np.asarray(Image.open(io.BytesIO(jpegs[-1])).convert("RGB")))
    calls = []
    for name in ("upload_frames_png", "upload_frames_jpeg", "upload_frames_u8_ragged", "upload_frames_u8_augmented"):
        real = getattr(Engine, name)
        monkeypatch.setattr(Engine, name, (lambda real, name: lambda self, *a, **k: (calls.append(name), real(self, *a, **k))[1])(real, name))
    eng = _engine(3, kitti=True)
    means = constants.MEANS_DICT["Kitti"]
    as_png = [datasets.DeferredPng(f, r.shape) for f, r in zip(pngs, rgbs)]
    as_jpeg = [datasets.DeferredJpeg(f, r.shape) for f, r in zip(jpegs, jpeg_rgbs)]

    def images(frames, aug=None):
        del calls[:]
        datasets.upload_frames(eng, frames, means, aspect_resize=True, aug=aug)
        return eng.get_images().copy(), list(calls)
    ref_png, route = images(rgbs)
    assert route == ["upload_frames_u8_ragged"]
    ref_jpeg, _ = images(jpeg_rgbs)
    got, route = images(as_png)
    assert route == ["upload_frames_png"] and np.array_equal(got, ref_png)
    got, route = images(as_jpeg)
    assert route == ["upload_frames_jpeg"] and np.array_equal(got, ref_jpeg)
    # mixtures take the PIL route: PNG + decoded array, PNG + JPEG
    got, route = images([as_png[0], rgbs[1], as_png[2]])
    assert route == ["upload_frames_u8_ragged"] and np.array_equal(got, ref_png)
    ref_mixed, _ = images([rgbs[0], jpeg_rgbs[1], rgbs[2]])
    got, route = images([as_png[0], as_jpeg[1], as_png[2]])
    assert route == ["upload_frames_u8_ragged"] and np.array_equal(got, ref_mixed)
    # with augmentation records
    ref_aug, route = images(rgbs, AUG)
    assert route == ["upload_frames_u8_augmented"]
    got, route = images(as_png, AUG)
    assert route == ["upload_frames_png"] and np.array_equal(got, ref_aug)
    got, route = images([as_png[0], as_png[1], rgbs[2]], AUG)
    assert route == ["upload_frames_u8_augmented"] and np.array_equal(got, ref_aug)
    eng.close()

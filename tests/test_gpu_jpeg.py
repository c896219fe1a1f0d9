"""GPU: baseline JPEG frames decoded inside the library -- Huffman decoding on host threads, jpeg_idct_kernel and
jpeg_color_kernel on the device -- against PIL's decode: the golden RGB of tests/golden/jpeg_cases.npz (written by PIL here, so the
tests do not depend on this machine's PIL build), byte for byte.  Then the upload routes: the image buffer, the pipelined form and
one infer after bod_upload_frames_jpeg equal those after the ragged / augmented upload of the golden frames; a bad frame is refused
by name and changes nothing; run_inference --device_jpeg writes the files the default route writes."""
import io
import os

import numpy as np
import pytest

from conftest import ANCHOR_CFG, BAYES_CFG, NMS_CFG
import jpeg_corpus

pytestmark = pytest.mark.gpu

HW = (128, 128)


@pytest.fixture(scope="module")
def corpus():
    return jpeg_corpus.load()


def _pick(cases, w, h, sampling, k=0):
    return [c for c in cases if (c.width, c.height, c.sampling) == (w, h, sampling)][k]


def test_every_case_decodes_to_the_golden_rgb(corpus):
    from bayes_od_rc_amd.engine import decode_jpeg_rgb
    cases, _ = corpus
    for c in cases:
        (got,) = decode_jpeg_rgb([c.data])
        assert got.shape == c.rgb.shape and np.array_equal(got, c.rgb), (c, int(np.abs(got.astype(int) - c.rgb).max()))


@pytest.mark.parametrize("batch", [1, 3, 64])
def test_batches_of_mixed_sizes_and_samplings(corpus, batch):
    from bayes_od_rc_amd.engine import decode_jpeg_rgb
    cases, _ = corpus
    order = np.random.default_rng(batch).permutation(len(cases))            # neighbours differ in size, sampling and variant
    picked = [cases[i] for i in order[:max(batch, 6)]]
    for first in range(0, len(picked) - batch + 1, batch):
        group = picked[first:first + batch]
        one = decode_jpeg_rgb([c.data for c in group], threads=1)
        four = decode_jpeg_rgb([c.data for c in group], threads=4)
        assert len(one) == len(four) == batch
        for c, a, b in zip(group, one, four):
            assert a.shape == c.rgb.shape and np.array_equal(a, c.rgb), c
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


def _network_size_frames():
    """Three JPEG files at the network size (noise on a gradient; 4:2:0, 4:2:2 with restart markers, grayscale) with PIL's decode of
    each -- the role the golden RGB plays for the small cases."""
    from PIL import Image
    rng = np.random.default_rng(8)
    yy, xx = np.mgrid[0:HW[0], 0:HW[1]]
    files, rgbs = [], []
    for k, kw in enumerate((dict(subsampling="4:2:0"), dict(subsampling="4:2:2", restart_marker_blocks=1), dict())):
        a = np.clip(np.stack([2 * xx, 2 * yy, 255 - xx - yy], axis=2) + rng.integers(-60, 60, HW + (3,)), 0, 255).astype(np.uint8)
        im = Image.fromarray(a) if k < 2 else Image.fromarray(a[:, :, 0], "L")
        buf = io.BytesIO()
        im.save(buf, "JPEG", quality=90, **kw)
        files.append(buf.getvalue())
        rgbs.append(np.asarray(Image.open(io.BytesIO(files[-1])).convert("RGB")))
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


def _check_routes(eng, files, rgbs, means, aspect_resize, want_detections):
    # synchronous: image buffer and src_hw
    eng.upload_frames_u8_ragged(rgbs, means, aspect_resize=aspect_resize)
    ref_images = eng.get_images().copy()
    ref_dets = _detections(eng)
    src_hw = eng.upload_frames_jpeg(files, means, aspect_resize=aspect_resize)
    assert src_hw.tolist() == [list(r.shape[:2]) for r in rgbs]
    assert np.array_equal(eng.get_images(), ref_images)
    dets = _detections(eng)
    print("detections per frame", ref_dets["num"].tolist(), dets["num"].tolist())
    assert _same(dets, ref_dets)
    if want_detections:
        assert ref_dets["num"].min() > 0
    # threads: one worker or several, the same bytes
    eng.upload_frames_jpeg(files, means, aspect_resize=aspect_resize, threads=1)
    assert np.array_equal(eng.get_images(), ref_images)
    # augmented
    eng.upload_frames_u8_augmented(rgbs, AUG, means, aspect_resize=aspect_resize)
    ref_aug = eng.get_images().copy()
    assert not np.array_equal(ref_aug, ref_images)
    eng.upload_frames_jpeg(files, means, aspect_resize=aspect_resize, aug=AUG)
    assert np.array_equal(eng.get_images(), ref_aug)
    # pipelined, into both buffers (twice into buffer 1: the second decode waits for the first copy out of its staging)
    for buffer, threads in ((0, None), (1, 2), (1, 1)):
        hw = eng.upload_frames_jpeg_async(files, buffer, means, aspect_resize=aspect_resize, threads=threads)
        assert np.array_equal(hw, src_hw)
        eng.synchronize()
        assert np.array_equal(eng.get_images(buffer), ref_images), buffer
        assert _same(_detections(eng, image_buffer=buffer), ref_dets), buffer
    eng.upload_frames_jpeg_async(files, 1, means, aspect_resize=aspect_resize, aug=AUG)
    eng.synchronize()
    assert np.array_equal(eng.get_images(1), ref_aug)
    with pytest.raises(ValueError, match="buffer must be 0 or 1"):
        eng.upload_frames_jpeg_async(files, 2, means, aspect_resize=aspect_resize)


def test_kitti_style_upload_equals_the_ragged_upload_of_the_golden_frames(corpus):
    """Frames of three sizes and samplings, each resized and padded by its own geometry and rescaled by its own factors."""
    from bayes_od_rc_amd import constants
    cases, _ = corpus
    picked = [_pick(cases, 33, 47, "4:2:0"), _pick(cases, 64, 48, "4:2:2", 1), _pick(cases, 16, 16, "gray", 2)]
    eng = _engine(3, kitti=True)
    _check_routes(eng, [c.data for c in picked], [c.rgb for c in picked], constants.MEANS_DICT["Kitti"], True, False)
    eng.close()


def test_bdd_style_upload_at_the_network_size():
    files, rgbs = _network_size_frames()
    eng = _engine(3, kitti=False)
    _check_routes(eng, files, rgbs, None, False, True)
    # a frame that is not at the network size is the ragged upload's geometry error, naming the frame
    small = io.BytesIO()
    from PIL import Image
    Image.fromarray(rgbs[1][:64]).save(small, "JPEG")
    before = eng.get_images().copy()
    with pytest.raises(ValueError, match="frame 1 is 64x128 but the handle expects 128x128"):
        eng.upload_frames_jpeg([files[0], small.getvalue(), files[2]], aspect_resize=False)
    assert np.array_equal(eng.get_images(), before)
    eng.close()


def test_a_bad_frame_is_refused_by_name_and_changes_nothing(corpus):
    from bayes_od_rc_amd import constants
    cases, extras = corpus
    good = [_pick(cases, 33, 47, "4:4:4"), _pick(cases, 31, 5, "4:2:0"), _pick(cases, 64, 48, "gray")]
    eng = _engine(3, kitti=True)
    means = constants.MEANS_DICT["Kitti"]
    eng.upload_frames_jpeg([c.data for c in good], means)
    before = eng.get_images().copy()
    truncated = good[1].data[:len(good[1].data) * 2 // 3]
    for bad, why in ((truncated, "corrupt"), (extras["progressive"], "progressive"), (extras["png"], "not a JPEG"), (extras["cmyk"], "4 components")):
        files = [good[0].data, bad, good[2].data]
        with pytest.raises(ValueError, match="frame 1 .*" + why):
            eng.upload_frames_jpeg(files, means)
        assert np.array_equal(eng.get_images(), before), why
        with pytest.raises(ValueError, match="frame 1 .*" + why):
            eng.upload_frames_jpeg_async(files, 0, means)
        eng.synchronize()
        assert np.array_equal(eng.get_images(), before), why
    with pytest.raises(ValueError, match="expected 3 JPEG files"):
        eng.upload_frames_jpeg([good[0].data], means)
    eng.close()


def test_run_inference_device_jpeg_writes_the_same_files(tmp_path, monkeypatch):
    """A BDD-layout tree of three small JPEGs and one PNG at --batch 2: the first batch is decoded on the device, the second holds the
    PNG and takes the PIL route; every output file equals the default route's byte for byte."""
    import json
    import yaml
    from PIL import Image
    from bayes_od_rc_amd import config_utils, run_inference, synthetic
    from bayes_od_rc_amd.model import RetinaNetModel
    root = tmp_path / "bdd100k"
    (root / "images" / "100k" / "val").mkdir(parents=True)
    (root / "labels").mkdir()
    (root / "labels" / "val.json").write_text(json.dumps([]))
    files, rgbs = _network_size_frames()
    for name, data in zip(("a.jpg", "b.jpg", "c.jpg"), files):
        (root / "images" / "100k" / "val" / name).write_bytes(data)
    Image.fromarray(rgbs[0][::-1].copy()).save(str(root / "images" / "100k" / "val" / "d.png"))
    weights = str(tmp_path / "weights.npz")
    RetinaNetModel.save_weights_npz(synthetic.make_weights(8, 9, cls_fg_bias=-1.0), weights)
    here = os.path.dirname(os.path.abspath(run_inference.__file__))
    cfg = config_utils.load_yaml(os.path.join(here, "configs", "retinanet_bdd_covar.yaml"))
    cfg["dataset_config"]["bdd"]["paths_config"]["dataset_dir"] = str(root)
    ypath = tmp_path / "retinanet_bdd_covar.yaml"          # the file name must equal checkpoint_name
    ypath.write_text(yaml.safe_dump(cfg))
    args = ["--gpu_device", "0", "--yaml_path", str(ypath), "--data_split", "test", "--dataset", "--batch", "2", "--weights", weights]
    uploads = []
    from bayes_od_rc_amd.engine import Engine
    real = Engine.upload_frames_jpeg
    monkeypatch.setattr(Engine, "upload_frames_jpeg", lambda self, *a, **k: (uploads.append(len(a[0])), real(self, *a, **k))[1])
    monkeypatch.setenv("BAYESOD_DATA_DIR", str(tmp_path / "default"))
    ref = run_inference.main(args)
    assert uploads == []
    monkeypatch.setenv("BAYESOD_DATA_DIR", str(tmp_path / "jpeg"))
    out = run_inference.main(args + ["--device_jpeg"])
    assert uploads == [2]                                    # (a, b) on the device; (c, d.png) by PIL
    assert ref != out
    listing = sorted(os.path.relpath(os.path.join(d, f), ref) for d, _, fs in os.walk(ref) for f in fs)
    assert listing == sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
    assert len(listing) >= 4 * 4
    for rel in listing:
        with open(os.path.join(ref, rel), "rb") as fa, open(os.path.join(out, rel), "rb") as fb:
            assert fa.read() == fb.read(), rel
    total = sum(np.load(os.path.join(out, "mean", n + ".npy")).shape[0] for n in "abcd")
    print("detections over the four frames:", total)
    assert total >= 4
    with pytest.raises(SystemExit):
        run_inference.main(["--gpu_device", "0", "--data_split", "test", "--synthetic", "2", "--device_jpeg"])

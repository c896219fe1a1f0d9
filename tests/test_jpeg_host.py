"""CPU: the host half of the JPEG decoder through the C ABI -- bod_jpeg_info and bod_jpeg_entropy_decode, no device
-- against the NumPy restatement (tests/jpeg_reference.py), the restatement's full decode against PIL (the golden RGB of
tests/golden/jpeg_cases.npz, and live PIL where it imports), and the dataset handlers' opt-in ``defer_decode``."""
import ctypes as C
import io
import json
import os

import numpy as np
import pytest

from conftest import ROOT
import jpeg_corpus
import jpeg_reference


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "bayes-od-rc_amd", "lib", "libbayesod_hip.so")):
        g.build()
    from bayes_od_rc_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def corpus():
    return jpeg_corpus.load()


@pytest.fixture(scope="module")
def reference(corpus):
    """The restatement's (coefs, quant, info) of every case, computed once."""
    return [jpeg_reference.entropy_decode(c.data) for c in corpus[0]]


def test_corpus_covers_every_size_and_sampling(corpus):
    cases, extras = corpus
    assert 200 <= len(cases) <= 300
    sizes = [(1, 1), (2, 1), (1, 3), (3, 3), (5, 4), (8, 8), (17, 2), (2, 17), (16, 16), (33, 47), (31, 5), (64, 48)]
    assert {(c.width, c.height, c.sampling) for c in cases} == {(w, h, s) for w, h in sizes for s in jpeg_corpus.SAMPLINGS}
    assert {c.quality for c in cases} == {1, 30, 90, 100} and {c.variant for c in cases} == set(jpeg_corpus.VARIANTS)
    assert {c.content for c in cases} == {"noise", "smooth"}
    assert set(extras) >= {"progressive", "cmyk", "png"}


def test_jpeg_info_fields(lib, corpus, reference):
    from bayes_od_rc_amd import engine
    for c, (_, _, info) in zip(corpus[0], reference):
        got = engine.jpeg_info(c.data)
        assert got["supported"] and got["reason"] == "", c
        assert (got["width"], got["height"]) == (c.width, c.height), c
        assert got["components"] == (1 if c.sampling == "gray" else 3), c
        assert (got["h_samp"], got["v_samp"]) == jpeg_corpus.LUMA[c.sampling], c
        assert got["restart_interval"] == info["restart_interval"], c
        assert (got["restart_interval"] > 0) == (c.variant == "restart"), c
        assert got["coef_count"] == info["coef_count"], c


def test_entropy_decode_equals_the_restatement(lib, corpus, reference):
    from bayes_od_rc_amd import engine
    for c, (coefs, quant, _) in zip(corpus[0], reference):
        got_coefs, got_quant = engine.jpeg_entropy_decode(c.data)
        assert got_coefs.dtype == np.int16 and np.array_equal(got_coefs, coefs), c
        assert np.array_equal(got_quant, quant), c


def test_restatement_equals_pil(corpus, reference):
    try:
        from PIL import Image
    except ImportError:
        Image = None
    for c, (coefs, quant, info) in zip(corpus[0], reference):
        rgb = jpeg_reference.planes_to_rgb(jpeg_reference.idct_planes(coefs, quant, info), info)
        assert rgb.shape == c.rgb.shape and np.array_equal(rgb, c.rgb), c
        if Image is not None:
            live = np.asarray(Image.open(io.BytesIO(c.data)).convert("RGB"))
            assert np.array_equal(rgb, live), c


def test_unsupported_files_are_reported_with_a_reason(lib, corpus):
    from bayes_od_rc_amd import engine
    _, extras = corpus
    for key, word in (("progressive", "progressive"), ("cmyk", "4 components"), ("png", "not a JPEG")):
        got = engine.jpeg_info(extras[key])
        assert not got["supported"] and word in got["reason"], (key, got)
        with pytest.raises(ValueError, match=word):
            engine.jpeg_entropy_decode(extras[key])


def test_capacity_and_corruption_are_invalid_arg(lib, corpus):
    from bayes_od_rc_amd import _lib, engine
    c = next(c for c in corpus[0] if (c.width, c.height, c.sampling) == (33, 47, "4:2:0"))
    n = engine.jpeg_info(c.data)["coef_count"]
    coefs = np.zeros(n, np.int16)
    quant = np.zeros((3, 64), np.uint16)
    cp, qp = coefs.ctypes.data_as(C.POINTER(C.c_int16)), quant.ctypes.data_as(C.POINTER(C.c_uint16))
    assert lib.bod_jpeg_entropy_decode(c.data, len(c.data), cp, n, qp) == _lib.BOD_OK
    assert lib.bod_jpeg_entropy_decode(c.data, len(c.data), cp, n - 1, qp) == _lib.BOD_ERR_INVALID_ARG
    assert b"coefficients" in lib.bod_last_error(None)
    cut = c.data[:len(c.data) // 2]
    assert lib.bod_jpeg_entropy_decode(cut, len(cut), cp, n, qp) == _lib.BOD_ERR_INVALID_ARG
    assert lib.bod_last_error(None)
    with pytest.raises(ValueError):
        engine.jpeg_info(c.data[:40])                     # the header itself is cut
    zero_w = bytearray(c.data)
    sof = c.data.index(b"\xff\xc0")
    zero_w[sof + 7:sof + 9] = b"\x00\x00"
    with pytest.raises(ValueError, match="width or height 0"):
        engine.jpeg_info(bytes(zero_w))


ANCHOR_GEN = {"layers": [3, 4, 5, 6, 7], "aspect_ratios": [[1.0, 1.0], [1.0, 2.0], [2.0, 1.0]], "scales": [1.0, 1.26, 1.59],
              "min_positive_iou": 0.5, "max_negative_iou": 0.4}


def _bdd_tree(tmp_path):
    from PIL import Image
    root = tmp_path / "bdd100k"
    (root / "images" / "100k" / "val").mkdir(parents=True)
    (root / "labels").mkdir()
    rng = np.random.default_rng(3)
    frame = rng.integers(0, 256, size=(128, 192, 3), dtype=np.uint8)
    Image.fromarray(frame).save(str(root / "images" / "100k" / "val" / "a.jpg"), quality=90)
    Image.fromarray(frame).save(str(root / "images" / "100k" / "val" / "b.png"))
    Image.fromarray(frame).save(str(root / "images" / "100k" / "val" / "c.jpg"), quality=90, progressive=True)
    (root / "labels" / "val.json").write_text(json.dumps([{"name": "a.jpg", "category": "car", "bbox": [10.0, 20.0, 90.0, 100.0]}]))
    return {"dataset": "bdd", "data_split": "val", "im_normalization": "ImageNet", "anchor_generator": ANCHOR_GEN,
            "bdd": {"paths_config": {"dataset_dir": str(root), "100k_or_10k": "100k"},
                    "training_data_config": {"categories": ["car", "truck", "bus", "person", "rider", "bike", "motor"],
                                             "frac_training_data": 1.0}}}, root


def test_defer_decode_yields_jpeg_bytes_and_falls_back(lib, tmp_path):
    from bayes_od_rc_amd import constants, datasets
    cfg, root = _bdd_tree(tmp_path)
    default = datasets.build_dataset(cfg, "val")
    assert default.defer_decode is False
    plain = list(default.create_dataset())
    deferred = datasets.build_dataset(cfg, "val")
    deferred.defer_decode = True
    got = list(deferred.create_dataset())
    assert default.sample_ids == ["a.jpg", "b.png", "c.jpg"]
    # the default handler's keys are what they were: no new key, the decoded frame and the host-normalised image present
    for s in plain:
        assert datasets.IMAGE_JPEG_KEY not in s and s[datasets.IMAGE_UINT8_KEY].shape == (128, 192, 3)
        assert s[constants.IMAGE_NORMALIZED_KEY].shape == (128, 192, 3)
    # the baseline JPEG travels as bytes, its size from the header, its normalisation left to the device
    a = got[0]
    assert a[datasets.IMAGE_JPEG_KEY] == (root / "images" / "100k" / "val" / "a.jpg").read_bytes()
    assert datasets.IMAGE_UINT8_KEY not in a and a[constants.IMAGE_NORMALIZED_KEY] is None
    assert list(a[constants.ORIGINAL_IM_SIZE_KEY]) == [128, 192, 3]
    for key in (constants.ANCHORS_KEY, constants.ANCHORS_CLASS_TARGETS_KEY, constants.ANCHORS_BOX_TARGETS_KEY, constants.POSITIVE_ANCHORS_MASK_KEY):
        assert np.array_equal(a[key], plain[0][key]), key
    frame = datasets.sample_frame(a)
    assert isinstance(frame, datasets.DeferredJpeg) and frame.shape == (128, 192, 3)
    assert np.array_equal(frame.decode(), plain[0][datasets.IMAGE_UINT8_KEY])
    # the PNG and the progressive JPEG take the PIL path, with the default handler's keys and values
    for s, p in zip(got[1:], plain[1:]):
        assert set(s) == set(p) and datasets.IMAGE_JPEG_KEY not in s
        assert np.array_equal(s[datasets.IMAGE_UINT8_KEY], p[datasets.IMAGE_UINT8_KEY])
        assert np.array_equal(s[constants.IMAGE_NORMALIZED_KEY], p[constants.IMAGE_NORMALIZED_KEY])
        assert datasets.sample_frame(s) is s[datasets.IMAGE_UINT8_KEY]

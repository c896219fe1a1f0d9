"""CPU: the host half of the PNG decoder through the C ABI -- bod_png_info and bod_png_inflate, no device -- against
zlib and PIL on the corpus of tests/png_corpus.py, the NumPy restatement of the five filters (tests/png_reference.py) against PIL, the
unsupported and corrupt kinds, and the dataset handlers' opt-in ``defer_png``."""
import ctypes as C
import io
import os
import zlib

import numpy as np
import pytest

from conftest import ROOT
import png_corpus
import png_reference


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "bayes-od-rc_amd", "lib", "libbayesod_hip.so")):
        g.build()
    from bayes_od_rc_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def corpus():
    return png_corpus.load()


def test_corpus_covers_every_size_type_filter_and_deflate_mode(corpus):
    hand = [c for c in corpus if c.mode != "pil"]
    assert {(c.height, c.width, c.color_type, tuple(c.pattern)) for c in hand} >= {
        (h, w, ct, tuple(p)) for h, w in png_corpus.SIZES for ct in png_corpus.COLOR_TYPES for p in png_corpus.PATTERNS}
    for h, w in png_corpus.SIZES:
        assert {c.mode for c in hand if (c.height, c.width) == (h, w)} == set(png_corpus.DEFLATE)
        assert {c.split for c in hand if (c.height, c.width) == (h, w)} >= set(png_corpus.IDAT_SPLITS)
    for p in png_corpus.PATTERNS:
        assert {c.mode for c in hand if c.pattern == p} == set(png_corpus.DEFLATE)
    assert {(c.mode, c.split, c.color_type) for c in hand} >= {(m, s, ct) for m in png_corpus.DEFLATE for s in png_corpus.IDAT_SPLITS
                                                              for ct in png_corpus.COLOR_TYPES}
    # the deflate modes are what their names say: stored blocks, fixed codes, dynamic codes (the block type of the first block)
    kinds = {}
    for c in hand:
        kinds.setdefault(c.mode, set()).add((png_corpus.idat_stream(c.data)[2] >> 1) & 3)
    # (zlib's Z_FIXED never emits dynamic codes, but stores a block that fixed codes would lengthen)
    assert kinds["stored"] == {0} and 1 in kinds["fixed"] and kinds["fixed"] <= {0, 1} and 2 in kinds["level6"] and 2 in kinds["level9"]
    assert len(corpus) <= 400


def test_every_corpus_file_decodes_through_pil_to_its_expected_rgb(corpus):
    """Pins the corpus writer: its filters, chunks and checksums are what an independent decoder accepts."""
    from PIL import Image
    for c in corpus:
        with Image.open(io.BytesIO(c.data)) as im:
            got = np.asarray(im.convert("RGB"))
        assert got.shape == c.rgb.shape and np.array_equal(got, c.rgb), c


def test_png_info_fields(lib, corpus):
    from bayes_od_rc_amd import engine
    for c in corpus:
        got = engine.png_info(c.data)
        assert got["supported"] and got["reason"] == "", c
        assert (got["height"], got["width"]) == (c.height, c.width), c
        assert (got["bit_depth"], got["color_type"], got["interlace"]) == (8, c.color_type, 0), c
        assert got["channels"] == png_corpus.CHANNELS[c.color_type], c
        assert got["raw_bytes"] == c.height * (1 + c.width * got["channels"]), c


def test_inflate_equals_zlib(lib, corpus):
    from bayes_od_rc_amd import engine
    for c in corpus:
        want = zlib.decompress(png_corpus.idat_stream(c.data))
        got = engine.png_inflate(c.data)
        assert got.dtype == np.uint8 and got.tobytes() == want, c
        if c.mode != "pil":
            assert [int(v) for v in got[:, 0]] == [c.pattern[r % len(c.pattern)] for r in range(c.height)], c


def test_the_incomplete_code_sets_zlib_accepts_are_accepted(lib):
    """A literal/length set of the end-of-block code alone and a one-code distance set: zlib's inflate takes both, so a file with them
    must not be reported as supported and then refused as corrupt."""
    from bayes_od_rc_amd import engine
    arr = png_corpus.make_array(9, 13, 2, 5)
    raw = png_corpus.filter_rows(arr.reshape(9, 39), 3, [4, 1]).tobytes()
    z = png_corpus.single_code_stream(raw)
    assert (z[2 + 5 + len(raw)] >> 1) & 3 == 2 and zlib.decompress(z) == raw          # a dynamic block behind the stored one
    data = png_corpus.assemble(13, 9, 2, z)
    assert engine.png_info(data)["supported"]
    assert engine.png_inflate(data).tobytes() == raw
    # the same set with a second bit pattern in use is no code of it
    at = 2 + 5 + len(raw)
    tail = bytearray(z[at:-4])
    nbits = 17 + 54 + 16 + 2                                   # the end-of-block code is the bit behind the header and the lengths
    tail[nbits // 8] |= 1 << (nbits % 8)
    with pytest.raises(ValueError, match="literal/length symbol"):
        engine.png_inflate(png_corpus.assemble(13, 9, 2, z[:at] + bytes(tail) + z[-4:]))


def test_restatement_equals_pil(lib, corpus):
    from PIL import Image
    for c in corpus:
        ch = png_corpus.CHANNELS[c.color_type]
        raw = np.frombuffer(zlib.decompress(png_corpus.idat_stream(c.data)), np.uint8).reshape(c.height, 1 + c.width * ch)
        rgb = png_reference.decode(raw, c.width, ch)
        with Image.open(io.BytesIO(c.data)) as im:
            live = np.asarray(im.convert("RGB"))
        assert np.array_equal(rgb, live) and np.array_equal(rgb, c.rgb), c


def test_unsupported_files_are_reported_with_a_reason(lib):
    from bayes_od_rc_amd import engine
    files = png_corpus.unsupported_files()
    assert set(files) == {"palette", "16-bit", "bit depth 4", "interlaced", "tRNS", "acTL"}
    for name, (data, word) in files.items():
        got = engine.png_info(data)
        assert not got["supported"] and word in got["reason"], (name, got)
        with pytest.raises(ValueError, match=word):
            engine.png_inflate(data)
    # PIL's own palette and 16-bit files, and a file of another format
    from PIL import Image
    rgb = png_corpus.make_array(4, 6, 2, 1)
    for im, word in ((Image.fromarray(rgb).quantize(8), "palette"), (Image.fromarray(np.arange(24, dtype=np.uint16).reshape(4, 6)), "bit depth 16")):
        buf = io.BytesIO()
        im.save(buf, "PNG")
        got = engine.png_info(buf.getvalue())
        assert not got["supported"] and word in got["reason"], (im.mode, got)
    buf = io.BytesIO()
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(buf, "JPEG")
    got = engine.png_info(buf.getvalue())
    assert not got["supported"] and "not a PNG" in got["reason"]


def test_corruption_is_invalid_arg(lib):
    from bayes_od_rc_amd import _lib, engine
    files, good = png_corpus.corrupt_files()
    assert set(files) == {"flipped CRC", "flipped Adler-32", "truncated file", "truncated IDAT", "filter byte 5", "one row short", "one byte long"}
    n = engine.png_info(good)["raw_bytes"]
    raw = np.zeros(n + 8, np.uint8)
    rp = raw.ctypes.data_as(C.POINTER(C.c_uint8))
    assert lib.bod_png_inflate(good, len(good), rp, n) == _lib.BOD_OK
    assert raw[:n].tobytes() == zlib.decompress(png_corpus.idat_stream(good)) and not raw[n:].any()
    assert lib.bod_png_inflate(good, len(good), rp, n - 1) == _lib.BOD_ERR_INVALID_ARG
    assert b"the buffer holds" in lib.bod_last_error(None)
    for name, (data, word) in files.items():
        raw[:] = 0
        assert lib.bod_png_inflate(data, len(data), rp, n) == _lib.BOD_ERR_INVALID_ARG, name
        assert word.encode() in lib.bod_last_error(None), (name, lib.bod_last_error(None))
        assert not raw[n:].any(), name                                  # nothing lands behind the scanlines' size
    # the header's own faults are bod_png_info's
    ihdr = good.index(b"IHDR")
    for field, word in ((4, "width or height 0"), (8, "width or height 0")):
        bad = bytearray(good)
        bad[ihdr + field:ihdr + field + 4] = bytes(4)
        bad[ihdr + 17:ihdr + 21] = (zlib.crc32(bytes(bad[ihdr:ihdr + 17])) & 0xFFFFFFFF).to_bytes(4, "big")
        with pytest.raises(ValueError, match=word):
            engine.png_info(bytes(bad))
    big = bytearray(good)
    big[ihdr + 4:ihdr + 8] = (70000).to_bytes(4, "big")
    big[ihdr + 17:ihdr + 21] = (zlib.crc32(bytes(big[ihdr:ihdr + 17])) & 0xFFFFFFFF).to_bytes(4, "big")
    with pytest.raises(ValueError, match="beyond 65535"):
        engine.png_info(bytes(big))
    bad = bytearray(good)
    bad[ihdr + 17] ^= 1
    with pytest.raises(ValueError, match="CRC mismatch in IHDR"):
        engine.png_info(bytes(bad))
    with pytest.raises(ValueError, match="truncated"):
        engine.png_info(good[:40])


ANCHOR_GEN = {"layers": [3, 4, 5, 6, 7], "aspect_ratios": [[1.0, 1.0], [1.0, 2.0], [2.0, 1.0]], "scales": [1.0, 1.26, 1.59],
              "min_positive_iou": 0.5, "max_negative_iou": 0.4}


def _kitti_tree(tmp_path):
    from PIL import Image
    root = tmp_path / "object"
    (root / "training" / "image_2").mkdir(parents=True)
    (root / "training" / "label_2").mkdir()
    ids = ["000000", "000001", "000002"]
    (root / "val.txt").write_text("\n".join(ids) + "\n")
    rng = np.random.default_rng(3)
    frame = rng.integers(0, 256, size=(94, 310, 3), dtype=np.uint8)
    Image.fromarray(frame).save(str(root / "training" / "image_2" / "000000.png"))
    Image.fromarray(frame).quantize(16).save(str(root / "training" / "image_2" / "000001.png"))          # a palette file
    Image.fromarray(frame[:, :, 0]).save(str(root / "training" / "image_2" / "000002.png"))
    for sid in ids:
        (root / "training" / "label_2" / (sid + ".txt")).write_text(
            "Car 0.00 0 -1.57 100.00 20.00 200.00 80.00 1.5 1.6 3.9 1.0 1.5 10.0 -1.5\n")
    return {"dataset": "kitti", "data_split": "val", "im_normalization": "Kitti", "anchor_generator": ANCHOR_GEN,
            "kitti": {"resize_shape": [128, 416], "paths_config": {"dataset_dir": str(root), "data_split_dir": "training"},
                      "training_data_config": {"categories": ["car", "pedestrian", "cyclist"], "difficulty": "all"}}}, root


def test_defer_png_yields_png_bytes_and_falls_back(lib, tmp_path, monkeypatch):
    from bayes_od_rc_amd import constants, datasets
    cfg, root = _kitti_tree(tmp_path)
    default = datasets.build_dataset(cfg, "val")
    assert default.defer_png is False and default.defer_decode is False
    plain = list(default.create_dataset())
    jpeg_only = datasets.build_dataset(cfg, "val")
    jpeg_only.defer_decode = True                          # --device_jpeg alone: PNG files keep the PIL path, exactly as before
    for s, p in zip(jpeg_only.create_dataset(), plain):
        assert set(s) == set(p) and datasets.IMAGE_PNG_KEY not in s
        assert np.array_equal(s[datasets.IMAGE_UINT8_KEY], p[datasets.IMAGE_UINT8_KEY])
    reads = []
    real_open = open

    def counting_open(path, *a, **k):
        if str(path).endswith(".png"):
            reads.append(os.path.basename(str(path)))
        return real_open(path, *a, **k)
    both = datasets.build_dataset(cfg, "val")
    both.defer_decode = both.defer_png = True
    monkeypatch.setattr("builtins.open", counting_open)
    got = list(both.create_dataset())
    monkeypatch.undo()
    assert reads.count("000000.png") == 1 and reads.count("000002.png") == 1          # read once with both flags on
    for k in (0, 2):                                       # RGB and gray travel as bytes, their size from the header
        s = got[k]
        assert s[datasets.IMAGE_PNG_KEY] == (root / "training" / "image_2" / ("00000%d.png" % k)).read_bytes()
        assert datasets.IMAGE_UINT8_KEY not in s and datasets.IMAGE_JPEG_KEY not in s and s[constants.IMAGE_NORMALIZED_KEY] is None
        assert list(s[constants.ORIGINAL_IM_SIZE_KEY]) == [94, 310, 3]
        assert np.array_equal(s[constants.BOXES_2D_GT_KEY], plain[k][constants.BOXES_2D_GT_KEY])
        frame = datasets.sample_frame(s)
        assert isinstance(frame, datasets.DeferredPng) and frame.shape == (94, 310, 3) and datasets.sample_is_deferred(s)
        assert np.array_equal(frame.decode(), plain[k][datasets.IMAGE_UINT8_KEY])
    # the palette file takes the PIL path, with the default handler's keys and values
    s, p = got[1], plain[1]
    assert set(s) == set(p) and not datasets.sample_is_deferred(s)
    assert np.array_equal(s[datasets.IMAGE_UINT8_KEY], p[datasets.IMAGE_UINT8_KEY])
    assert datasets.sample_frame(s) is s[datasets.IMAGE_UINT8_KEY]

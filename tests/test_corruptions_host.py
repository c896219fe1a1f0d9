"""CPU checks of the corruption stage's host side: the NumPy reference's JPEG op against PIL's own save-then-load
bytes, the quality scaling against the tables PIL writes, the generated tap sets, the NAME:SEVERITY parser, and every named chain
against the C side's validation rules restated in Python."""
import io

import numpy as np
import pytest
from PIL import Image as PIL_Image

import conftest  # noqa: F401  (puts the repository root on sys.path)
import corruption_reference as ref
import jpeg_reference
from bayes_od_rc_amd import corruptions

JPEG_SIZES = [(1, 1), (8, 8), (13, 21), (33, 47), (64, 48), (7, 130)]
JPEG_QUALITIES = [5, 50, 90, 100]


def make_frame(h, w, kind, seed=0):
    rng = np.random.RandomState(seed + 1000 * h + w)
    if kind == "noise":
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    ramp = np.stack([(3 * x + y) % 256, (255 * y) // max(h - 1, 1), (255 * x) // max(w - 1, 1)], axis=-1)
    if kind == "smooth":
        return ramp.astype(np.uint8)
    return np.where(rng.rand(h, w, 1) < 0.5, ramp, rng.randint(0, 256, (h, w, 3))).astype(np.uint8)


def pil_round_trip(frame, quality):
    buf = io.BytesIO()
    PIL_Image.fromarray(frame).save(buf, format="JPEG", quality=quality, subsampling=0)
    return buf.getvalue(), np.asarray(PIL_Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))


@pytest.mark.parametrize("quality", JPEG_QUALITIES)
@pytest.mark.parametrize("hw", JPEG_SIZES)
def test_reference_jpeg_equals_pil_round_trip(hw, quality):
    for kind in ("noise", "smooth", "mixed"):
        frame = make_frame(hw[0], hw[1], kind)
        _, want = pil_round_trip(frame, quality)
        got = ref.jpeg(frame, corruptions.jpeg_qtables(quality))
        assert np.array_equal(got, want), (hw, quality, kind, int(np.abs(got.astype(int) - want.astype(int)).max()))


@pytest.mark.parametrize("quality", [1, 5, 24, 25, 49, 50, 51, 75, 90, 95, 100])
def test_quality_scaling_reproduces_pil_tables(quality):
    data, _ = pil_round_trip(make_frame(8, 8, "noise"), quality)
    info = jpeg_reference.parse(data)
    q = corruptions.jpeg_qtables(quality)
    assert np.array_equal(q[0], info["qt"][info["comps"][0]["tq"]])
    assert np.array_equal(q[1], info["qt"][info["comps"][1]["tq"]])
    assert q.min() >= 1 and q.max() <= 255


def test_reference_forward_path_equals_pil_coefficients():
    """The quantised coefficients themselves, read back from PIL's stream: the forward half alone."""
    for hw, quality in (((13, 21), 50), ((33, 47), 90), ((7, 130), 5)):
        frame = make_frame(hw[0], hw[1], "mixed")
        data, _ = pil_round_trip(frame, quality)
        info = jpeg_reference.parse(data)
        coefs, _ = jpeg_reference.entropy_decode(data)[:2]
        got = ref.jpeg_forward(frame, corruptions.jpeg_qtables(quality))
        assert info["h_samp"] == 1 and info["v_samp"] == 1
        assert np.array_equal(got.reshape(-1), np.asarray(coefs, np.int64).reshape(-1))


def _tap_sets():
    sets = []
    for name in ("defocus_blur", "motion_blur", "gaussian_blur"):
        for sev in range(1, 6):
            ch = corruptions.make(name, sev)
            K = ch.ops[0]["ksize"]
            sets.append((name, sev, ch.taps.reshape(K, K)))
    return sets


def test_tap_sets_sum_to_2_15_and_are_symmetric():
    for name, sev, t in _tap_sets():
        K = t.shape[0]
        assert K % 2 == 1 and 1 <= K <= 25, (name, sev, K)
        assert int(t.astype(np.int64).sum()) == 1 << 15, (name, sev)
        assert np.array_equal(t, t[::-1]) and np.array_equal(t, t[:, ::-1]), (name, sev)
        if name != "motion_blur":
            assert np.array_equal(t, t.T), (name, sev)
        else:
            assert np.count_nonzero(t) == K and np.count_nonzero(t[K // 2]) == K
    for angle in (0, 45, 90, 135):
        t = corruptions.line_kernel(9, angle)
        assert int(t.astype(np.int64).sum()) == 1 << 15 and np.array_equal(t, t[::-1, ::-1])
    diag = corruptions.line_kernel(5, 45) > 0                  # 5 unit steps along the diagonal reach +-1.41 pixels per axis
    assert not np.any(diag & ~np.eye(5, dtype=bool)) and np.count_nonzero(diag) == 3
    assert corruptions.quantise_taps(np.ones((1, 1)))[0, 0] == 1 << 15


def test_quantise_taps_on_awkward_kernels():
    rng = np.random.RandomState(3)
    for K in (1, 3, 7, 25):
        k = rng.rand(K, K)
        t = corruptions.quantise_taps(k)
        assert int(t.astype(np.int64).sum()) == 1 << 15
        assert np.abs(t.astype(np.float64) - k / k.sum() * (1 << 15)).max() <= K * K     # the centre takes what is left
    for bad in (np.ones((2, 2)), np.ones((27, 27)), -np.ones((3, 3)), np.zeros((3, 3)), np.ones((3, 5))):
        with pytest.raises(ValueError):
            corruptions.quantise_taps(bad)


def test_parser_and_its_errors():
    assert corruptions.parse("gaussian_noise:3") == ("gaussian_noise", 3)
    assert corruptions.parse(" fog : 5 ") == ("fog", 5)
    for name in corruptions.NAMES:
        assert corruptions.parse("%s:1" % name) == (name, 1)
    for bad, msg in (("gaussian_noise", "NAME:SEVERITY"), ("a:b:c", "NAME:SEVERITY"), ("zoom:3", "unknown corruption"),
                     ("fog:0", "1..5"), ("fog:6", "1..5"), ("fog:x", "integer"), ("fog:2.5", "integer"), (None, "NAME:SEVERITY")):
        with pytest.raises(ValueError, match=msg):
            corruptions.parse(bad)
    with pytest.raises(ValueError):
        corruptions.make("fog", 0)
    with pytest.raises(ValueError):
        corruptions.make("nothing", 1)
    assert set(corruptions.NAMES) == {"gaussian_noise", "impulse_noise", "defocus_blur", "motion_blur", "gaussian_blur", "pixelate",
                                      "jpeg_compression", "contrast", "brightness", "low_light", "fog"}


def test_every_named_chain_passes_validation():
    for name in corruptions.NAMES:
        for sev in range(1, 6):
            ch = corruptions.make(name, sev)
            assert 1 <= len(ch) <= corruptions.MAX_OPS
            corruptions.validate(*corruptions.pack(ch, 3))
    ch = corruptions.make("low_light", 2)
    assert [o["kind"] for o in ch.ops] == [corruptions.LUT, corruptions.GAUSSIAN_NOISE]
    # mixed chains per frame: tables are concatenated and the indices shifted
    chains = [corruptions.make("defocus_blur", 1), corruptions.make("low_light", 1), corruptions.make("jpeg_compression", 2),
              corruptions.make("motion_blur", 2), corruptions.make("brightness", 1)]
    ops, taps, luts, qts = corruptions.pack(chains)
    corruptions.validate(ops, taps, luts, qts)
    assert ops.shape == (5, 2) and luts.shape[0] == 2 and qts.shape[0] == 1
    assert ops[3, 0]["tap_offset"] == chains[0].taps.size and ops[4, 0]["table"] == 1
    assert ops[0, 1]["kind"] == corruptions.NONE


def test_validation_rules_reject_what_the_library_rejects():
    good = corruptions.pack(corruptions.make("defocus_blur", 2), 1)

    def bad(field, value, chain=None, **tables):
        ops, taps, luts, qts = corruptions.pack(chain, 1) if chain is not None else [a.copy() for a in good]
        if field:
            ops[0, 0][field] = value
        t = {"taps": taps, "luts": luts, "qtables": qts}
        t.update(tables)
        with pytest.raises(ValueError, match="frame 0 op 0"):
            corruptions.validate(ops, t["taps"], t["luts"], t["qtables"])

    bad("kind", 9)
    bad("kind", -1)
    bad("ksize", 4)
    bad("ksize", 27)
    bad("tap_offset", 1)
    bad(None, None, taps=good[1] + np.uint16(1))
    bad("u0", 1, corruptions.op_pixelate(2))
    bad("u0", 65, corruptions.op_pixelate(2))
    bad("f0", np.nan, corruptions.op_gaussian_noise(1.0))
    bad("f0", 129.0, corruptions.op_gaussian_noise(1.0))
    bad("f0", -1.0, corruptions.op_gaussian_noise(1.0))
    bad("f0", np.inf, corruptions.op_contrast(1.0))
    bad("u0", 257, corruptions.op_fog(10))
    bad("table", 1, corruptions.op_jpeg(50))
    q = corruptions.jpeg_qtables(50).copy()
    q[1, 63] = 0
    bad(None, None, corruptions.op_jpeg(qtables=q))
    with pytest.raises(ValueError, match="ops_per_frame"):
        corruptions.validate(np.zeros((1, 5), corruptions.OP_DTYPE), good[1], good[2], good[3])


def test_gaussian_seed_keeps_the_excused_fraction_small():
    """tests/test_gpu_corruptions.py excuses samples whose float64 value lies within 2^-9 of a rounding boundary, at most 1 % of
    them: the reference alone must stay under that for the seed, sizes and sigmas the GPU test uses."""
    import test_gpu_corruptions as g
    for sigma in g.GAUSS_SIGMAS:
        near = total = 0
        for i, f in enumerate(g.base_frames()):
            v = ref.gaussian_noise_f64(f, sigma, 0, g.FRAME_IDS[i], g.SEED)
            near += int(g.near_boundary(v).sum())
            total += v.size
        assert near <= 0.01 * total, (sigma, near, total)


def test_reference_ops_small_cases_by_hand():
    f = np.array([[[10, 20, 30], [50, 60, 70]], [[90, 100, 110], [130, 140, 150]]], np.uint8)
    assert np.array_equal(ref.pixelate(f, 2)[0, 0], [70, 80, 90])
    one_hot = np.zeros((3, 3), np.uint16)
    one_hot[0, 2] = 1 << 15                                    # reads (y - 1, x + 1), clamped
    out = ref.conv2d(f, one_hot)
    assert np.array_equal(out[1, 0], f[0, 1]) and np.array_equal(out[0, 1], f[0, 1]) and np.array_equal(out[1, 1], f[0, 1])
    assert np.array_equal(ref.contrast(f, 0.0)[..., 0], np.full((2, 2), 70))
    assert np.array_equal(ref.impulse_noise(f, 0, 0, 5, 7), f)
    assert set(np.unique(ref.impulse_noise(f, 0xFFFFFFFF, 0, 5, 7))) <= {0, 255}
    assert np.array_equal(ref.gaussian_noise(f, 0.0, 0, 5, 7), f)
    assert np.array_equal(ref.fog(f, 0, 0, 5, 7), f)
    fogged = ref.fog(np.zeros((40, 50, 3), np.uint8), 256, 0, 5, 7)
    assert fogged.max() > fogged.min() and np.array_equal(fogged[..., 0], fogged[..., 2])


def test_offline_eval_shift_prints_every_tree_and_its_difference(tmp_path, capsys):
    import json
    import shutil
    import scores_reference
    from bayes_od_rc_amd import offline_eval, scoring_rules
    gt, root = scores_reference.write_tree(str(tmp_path / "clean"))
    other = str(tmp_path / "shifted")
    shutil.copytree(root, other)
    name = scores_reference.TREE_FRAMES[0]
    cov = np.load(other + "/cov/%s.npy" % name)
    np.save(other + "/cov/%s.npy" % name, cov * 4.0)                 # wider boxes' distributions on one frame
    args = ["shift", "--labels", root + "/labels.json", "--predictions", "clean=" + root, "wide=" + other, "--samples", "64", "--seed", "5"]
    out = offline_eval.main(args + ["--json"])
    text = capsys.readouterr().out
    assert out["names"] == ["clean", "wide"]
    want = scoring_rules.scores_report(gt, root, scores_reference.TREE_FRAMES, num_samples=64, seed=5)
    assert out["reports"]["clean"] == want
    assert all(v in (0.0, None) for v in out["delta"]["clean"].values())
    assert out["delta"]["wide"]["n_tp"] == 0.0
    moved = [k for k, v in out["delta"]["wide"].items() if v not in (0.0, None)]
    assert moved, out["delta"]["wide"]
    for k in moved:
        assert out["delta"]["wide"][k] == out["metrics"]["wide"][k] - out["metrics"]["clean"][k]
    lines = text.splitlines()
    assert lines[0].split() == ["metric", "clean", "wide"]
    assert any(l.startswith("n_tp") for l in lines) and "(" in text
    assert json.loads(text[text.index("{"):])["names"] == ["clean", "wide"]
    for bad in (["clean"], ["a=" + root, "a=" + other], ["=x"]):
        with pytest.raises(SystemExit):
            offline_eval.main(["shift", "--labels", root + "/labels.json", "--predictions"] + bad)
    with pytest.raises(SystemExit):
        offline_eval.main(["scores", "--labels", root + "/labels.json", "--predictions", root, other])

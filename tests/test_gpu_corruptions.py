"""GPU: the corruption stage (csrc/corrupt_kernels.hip) against tests/corruption_reference.py.  Everything goes
through bod_corrupt_frames_u8 unless it says otherwise.  The exact ops are array_equal to the reference (JPEG also to PIL's own
save-then-load bytes); GAUSSIAN_NOISE is equal outside a derived band around the rounding boundaries; a frame's bytes do not depend
on where it sits; the one-shot upload setting gives the image buffer of the upload of the corrupted frames; bad descriptions are
refused by frame and op; run_inference --corrupt, run_validation --corrupt and offline_eval shift work end to end on small trees.

Kernel tiles this file's sizes are chosen against: CONV2D works on 32 x 32 output tiles, PIXELATE on tiles of (64 / f) * f pixels
per side (64 for f = 2 and 64, 60 for f = 5), JPEG on 8 x 8 blocks, the pointwise ops on groups of 4 pixels.  The 70 x 75 frame
exceeds every one of them by a ragged remainder in both directions; 7 x 9 is smaller than an 8 x 8 block and than the K = 25 halo."""
import io
import os

import numpy as np
import pytest

import conftest  # noqa: F401
import corruption_reference as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EED0000C0FFEE
SIZES = [(1, 1), (7, 9), (8, 8), (13, 21), (33, 47), (64, 48), (70, 75)]
FRAME_IDS = [11, 3, 2 ** 31 + 5, 7, 0, 100, 42, 9]          # one per frame of base_frames()
GAUSS_SIGMAS = (4.0, 64.0)
GAUSS_BAND = 2.0 ** -9


def base_frames():
    """Random uint8 frames of SIZES plus one smooth ramp."""
    rng = np.random.RandomState(7)
    frames = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SIZES]
    y, x = np.mgrid[0:21, 0:40]
    frames.append(np.stack([(6 * x + y) % 256, 12 * y, 255 - 6 * x], axis=-1).astype(np.uint8))
    return frames


def near_boundary(v):
    """Samples whose float64 pre-rounding value lies within GAUSS_BAND of a rounding boundary k + 0.5."""
    return np.abs(v - np.floor(v) - 0.5) <= GAUSS_BAND


def _mod():
    from bayes_od_rc_amd import corruptions
    return corruptions


def _run(frames, chains, frame_ids=None, seed=SEED, ops_arrays=None):
    from bayes_od_rc_amd.engine import corrupt_frames
    return corrupt_frames(frames, chains, frame_ids=frame_ids, seed=seed, ops_arrays=ops_arrays)


def _want(frames, chains, frame_ids=None, seed=SEED):
    c = _mod()
    ops, taps, luts, qts = c.pack(chains, len(frames))
    return ref.apply_packed(frames, ops, taps, luts, qts, frame_ids, seed)


def _assert_equal(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == np.uint8, (what, i)
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            raise AssertionError("%s: frame %d %s differs at %d samples, first (y, x, c) = %s: got %d, want %d" %
                                 (what, i, a.shape, len(bad), tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])]))


def _one_hot(K, ky, kx):
    t = np.zeros((K, K), np.uint16)
    t[ky, kx] = 1 << 15
    return t


def _exact_cases():
    c = _mod()
    rng = np.random.RandomState(11)
    diag = c.quantise_taps(np.eye(25))
    cases = [
        ("none", c.op_none()),
        ("lut_random_per_channel", c.op_lut(rng.randint(0, 256, (3, 256)).astype(np.uint8))),
        ("lut_gamma", c.op_lut(c.lut_gamma(2.2))),
        ("contrast_0.5", c.op_contrast(0.5)),
        ("contrast_1.7", c.op_contrast(1.7)),
        ("contrast_0", c.op_contrast(0.0)),
        ("impulse_0", c.op_impulse_noise(0.0)),
        ("impulse_0.1", c.op_impulse_noise(0.1)),
        ("impulse_1", c.op_impulse_noise(1.0)),
        ("conv_k1", c.op_conv2d(_one_hot(1, 0, 0))),
        ("conv_k3_disk", c.op_conv2d(c.disk_kernel(1.5))),
        ("conv_k3_one_hot", c.op_conv2d(_one_hot(3, 0, 2))),
        ("conv_k25_disk", c.op_conv2d(c.disk_kernel(12.0))),
        ("conv_k25_diagonal", c.op_conv2d(diag)),
        ("conv_k25_one_hot", c.op_conv2d(_one_hot(25, 3, 20))),
        ("pixelate_2", c.op_pixelate(2)),
        ("pixelate_5", c.op_pixelate(5)),
        ("pixelate_64", c.op_pixelate(64)),
        ("jpeg_5", c.op_jpeg(5)),
        ("jpeg_50", c.op_jpeg(50)),
        ("jpeg_100", c.op_jpeg(100)),
        ("fog_0", c.op_fog(0)),
        ("fog_137", c.op_fog(137)),
        ("fog_256", c.op_fog(256)),
    ]
    assert diag.shape == (25, 25) and c.disk_kernel(12.0).shape == (25, 25) and c.disk_kernel(1.5).shape == (3, 3)
    return cases


def test_every_exact_op_alone_on_every_size():
    """One op at a time over the whole mixed-size batch (plus a constant frame: CONTRAST's mean equals every sample)."""
    frames = base_frames() + [np.full((9, 5, 3), 77, np.uint8)]
    ids = FRAME_IDS + [77]
    for name, chain in _exact_cases():
        got = _run(frames, chain, ids)
        _assert_equal(got, _want(frames, chain, ids), name)
        if name == "conv_k1" or name in ("none", "impulse_0", "fog_0"):
            _assert_equal(got, frames, name + " is the identity")
        if name == "contrast_0":
            assert np.array_equal(got[-1], frames[-1])
        if name == "impulse_1":
            assert all(set(np.unique(g)) <= {0, 255} for g in got)
        if name.startswith("jpeg_"):
            from PIL import Image
            q = int(name.split("_")[1])
            for i, f in enumerate(frames):
                buf = io.BytesIO()
                Image.fromarray(f).save(buf, format="JPEG", quality=q, subsampling=0)
                pil = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
                assert np.array_equal(got[i], pil), (name, i, f.shape)


def test_mixed_batch_with_a_different_chain_per_frame():
    c = _mod()
    frames = base_frames()
    cases = dict(_exact_cases())
    chains = [
        c.concat(cases["fog_137"], cases["jpeg_50"], cases["impulse_0.1"], cases["conv_k3_one_hot"]),
        cases["conv_k25_disk"],
        cases["none"],
        c.concat(cases["pixelate_5"], cases["contrast_0.5"]),
        c.concat(cases["jpeg_5"], cases["lut_random_per_channel"], cases["fog_256"]),
        c.concat(cases["contrast_1.7"], cases["pixelate_64"], cases["conv_k25_diagonal"], cases["jpeg_100"]),
        c.concat(cases["conv_k25_one_hot"], cases["pixelate_2"], cases["impulse_0.1"], cases["fog_137"]),
        c.concat(cases["lut_gamma"], cases["contrast_0"]),
    ]
    got = _run(frames, chains, FRAME_IDS)
    _assert_equal(got, _want(frames, chains, FRAME_IDS), "mixed batch")
    _assert_equal([got[2]], [frames[2]], "the NONE chain")
    # the same impulse op in slot 2 and in slot 0 draws different numbers (the slot is part of the counter)
    a = _run([frames[4]], c.concat(cases["none"], cases["none"], cases["impulse_0.1"]), [5])[0]
    b = _run([frames[4]], cases["impulse_0.1"], [5])[0]
    assert not np.array_equal(a, b)


@pytest.mark.parametrize("sigma", GAUSS_SIGMAS)
def test_gaussian_noise_equals_the_reference_outside_the_rounding_band(sigma):
    """u is exact in fp32, so the device normals differ from float64 only by libm's few-ulp errors and the fp32 rounding of
    2 pi u: about 5e-6 in n, about 4e-4 levels at sigma 64.  The band, 2^-9, is five times that.  Outside it the result equals
    the reference; inside it is within one level; at most 1 % of the samples lie inside (checked for the reference alone on the
    CPU: tests/test_corruptions_host.py)."""
    c = _mod()
    frames = base_frames()
    got = _run(frames, c.op_gaussian_noise(sigma), FRAME_IDS)
    excused = total = worst = 0
    for i, f in enumerate(frames):
        v = ref.gaussian_noise_f64(f, sigma, 0, FRAME_IDS[i], SEED)
        want = np.rint(v).astype(np.uint8)
        near = near_boundary(v)
        diff = np.abs(got[i].astype(np.int32) - want.astype(np.int32))
        assert np.array_equal(got[i][~near], want[~near]), (sigma, i, int((diff[~near] > 0).sum()))
        assert diff.max() <= 1, (sigma, i)
        excused += int(near.sum())
        total += v.size
        worst += int((diff > 0).sum())
    print("sigma %g: %d of %d samples inside the band, %d of them differ" % (sigma, excused, total, worst))
    assert excused <= 0.01 * total
    assert any(not np.array_equal(g, f) for g, f in zip(got, frames))
    # the noise has the asked-for spread (frames away from the clamps: a mid-grey frame)
    grey = np.full((64, 64, 3), 128, np.uint8)
    (noisy,) = _run([grey], c.op_gaussian_noise(sigma if sigma < 32 else 24.0), [1])
    s = float(np.std(noisy.astype(np.float64) - 128.0))
    assert abs(s / (sigma if sigma < 32 else 24.0) - 1.0) < 0.05, s


def test_gaussian_sigma_zero_is_the_identity():
    frames = base_frames()
    _assert_equal(_run(frames, _mod().op_gaussian_noise(0.0), FRAME_IDS), frames, "sigma 0")


def test_a_frames_bytes_do_not_depend_on_its_position_or_the_calls():
    c = _mod()
    frames = base_frames()
    cases = dict(_exact_cases())
    chain = c.concat(cases["impulse_0.1"], c.op_gaussian_noise(9.0), cases["fog_137"], cases["contrast_0.5"])
    k = 4                                                           # the 33 x 47 frame
    full = _run(frames, chain, FRAME_IDS)
    alone = _run([frames[k]], chain, [FRAME_IDS[k]])
    _assert_equal(alone, [full[k]], "alone")
    order = [6, 1, k, 0]
    moved = _run([frames[i] for i in order], chain, [FRAME_IDS[i] for i in order])
    _assert_equal([moved[2]], [full[k]], "another batch index")
    _assert_equal([moved[0]], [full[6]], "another batch index (the 70 x 75 frame)")
    # the chain as two calls: slots 0, 1 then slots 2, 3, the other call's slots holding NONE
    first = c.Chain(chain.ops[:2] + [{"kind": c.NONE}] * 2, chain.taps, chain.luts, chain.qtables)
    second = c.Chain([{"kind": c.NONE}] * 2 + chain.ops[2:], chain.taps, chain.luts, chain.qtables)
    half = _run([frames[k]], first, [FRAME_IDS[k]])
    both = _run(half, second, [FRAME_IDS[k]])
    _assert_equal(both, [full[k]], "two calls")
    # ... and it does depend on the id and on the seed
    assert not np.array_equal(_run([frames[k]], chain, [FRAME_IDS[k] + 1])[0], full[k])
    assert not np.array_equal(_run([frames[k]], chain, [FRAME_IDS[k]], seed=SEED + 1)[0], full[k])


# ---- upload integration -------------------------------------------------------------------------------------------------------
HW = (128, 128)


@pytest.fixture(scope="module")
def eng():
    from bayes_od_rc_amd.engine import Engine, make_config
    e = Engine(make_config(HW, batch=3, mc_samples=2))
    yield e
    e.close()


def _upload_case():
    c = _mod()
    rng = np.random.RandomState(21)
    frames = [rng.randint(0, 256, hw + (3,)).astype(np.uint8) for hw in ((96, 150), (128, 128), (61, 77))]
    cases = dict(_exact_cases())
    chains = [c.concat(cases["conv_k3_disk"], c.op_gaussian_noise(12.0), cases["jpeg_50"]), cases["fog_137"],
              c.concat(cases["pixelate_5"], cases["impulse_0.1"])]
    return frames, chains, [40, 41, 2 ** 32 - 1]


def test_upload_corruption_equals_the_upload_of_the_corrupted_frames(eng):
    from bayes_od_rc_amd.engine import AUGMENT_IDENTITY
    frames, chains, ids = _upload_case()
    corrupted = _run(frames, chains, ids, seed=9)
    assert not any(np.array_equal(a, b) for a, b in zip(corrupted, frames))
    eng.upload_frames_u8_ragged(frames)
    plain = eng.get_images().copy()
    eng.upload_frames_u8_ragged(corrupted)
    want = eng.get_images().copy()
    assert not np.array_equal(plain, want)
    # the synchronous ragged upload
    eng.set_upload_corruption(chains, ids, seed=9)
    eng.upload_frames_u8_ragged(frames)
    assert np.array_equal(eng.get_images(), want)
    # consumed: the next upload is the plain one
    eng.upload_frames_u8_ragged(frames)
    assert np.array_equal(eng.get_images(), plain)
    # the pipelined form on buffer 1 (and buffer 0, whose scratch is another one)
    for buffer in (1, 0):
        eng.set_upload_corruption(chains, ids, seed=9)
        eng.upload_frames_u8_ragged_async(frames, buffer)
        eng.synchronize()
        assert np.array_equal(eng.get_images(buffer), want), buffer
        eng.upload_frames_u8_ragged_async(frames, buffer)
        eng.synchronize()
        assert np.array_equal(eng.get_images(buffer), plain), buffer
    # the augmented upload
    aug = [dict(AUGMENT_IDENTITY, flip=1, gain=0.9, bias=3.0), dict(AUGMENT_IDENTITY, scale=0.8, off_x=0.2), dict(AUGMENT_IDENTITY)]
    eng.upload_frames_u8_augmented(corrupted, aug)
    want_aug = eng.get_images().copy()
    eng.set_upload_corruption(chains, ids, seed=9)
    eng.upload_frames_u8_augmented(frames, aug)
    assert np.array_equal(eng.get_images(), want_aug)
    eng.set_upload_corruption(chains, ids, seed=9)
    eng.upload_frames_u8_augmented_async(frames, aug, 1)
    eng.synchronize()
    assert np.array_equal(eng.get_images(1), want_aug)
    # a pending one is cleared by None
    eng.set_upload_corruption(chains, ids, seed=9)
    eng.set_upload_corruption(None)
    eng.upload_frames_u8_ragged(frames)
    assert np.array_equal(eng.get_images(), plain)


def test_upload_corruption_on_jpeg_files(eng):
    from PIL import Image
    from bayes_od_rc_amd.engine import decode_jpeg_rgb
    frames, chains, ids = _upload_case()
    files = []
    for f, sub in zip(frames, (0, 2, 1)):
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, format="JPEG", quality=85, subsampling=sub)
        files.append(buf.getvalue())
    decoded = decode_jpeg_rgb(files)
    eng.upload_frames_u8_ragged(_run(decoded, chains, ids, seed=3))
    want = eng.get_images().copy()
    eng.set_upload_corruption(chains, ids, seed=3)
    eng.upload_frames_jpeg(files)
    assert np.array_equal(eng.get_images(), want)
    eng.set_upload_corruption(chains, ids, seed=3)
    eng.upload_frames_jpeg_async(files, 1)
    eng.synchronize()
    assert np.array_equal(eng.get_images(1), want)
    eng.upload_frames_jpeg(files)                                   # consumed
    eng.upload_frames_u8_ragged(decoded)
    plain = eng.get_images().copy()
    eng.upload_frames_jpeg(files)
    assert np.array_equal(eng.get_images(), plain) and not np.array_equal(plain, want)


def test_a_uniform_upload_refuses_a_pending_corruption_and_keeps_it(eng):
    frames, chains, ids = _upload_case()
    same = [frames[1]] * 3
    corrupted = _run(same, chains, ids, seed=4)
    eng.upload_frames_u8_ragged(corrupted)
    want = eng.get_images().copy()
    eng.upload_frames_u8_ragged(same)
    before = eng.get_images().copy()
    eng.set_upload_corruption(chains, ids, seed=4)
    with pytest.raises(ValueError, match="pending"):
        eng.upload_frames_u8(np.stack(same))
    with pytest.raises(ValueError, match="pending"):
        eng.upload_frames_u8_async(np.stack(same), 1)
    assert np.array_equal(eng.get_images(), before)
    eng.upload_frames_u8_ragged(same)                               # the pending one survived both
    assert np.array_equal(eng.get_images(), want)
    eng.upload_frames_u8(np.stack(same))                            # and is gone now
    assert np.array_equal(eng.get_images(), before)


def _bad_descriptions():
    """(what the message must name, ops, taps, luts, qtables): one per clause of the header's validation list."""
    c = _mod()
    out = []

    def add(match, chain, n=3, frame=1, slot=0, taps=None, qtables=None, **fields):
        ops, t, l, q = c.pack(chain, n)
        ops = ops.copy()
        for k, v in fields.items():
            ops[frame, slot][k] = v
        out.append((match, ops, t if taps is None else taps, l, q if qtables is None else qtables))

    disk = c.op_conv2d(c.disk_kernel(2.5))
    add("frame 1 op 0.*unknown kind", c.op_none(), kind=9)
    add("frame 1 op 0.*unknown kind", c.op_none(), kind=-1)
    add("frame 2 op 1.*unknown kind", c.concat(c.op_none(), c.op_none()), frame=2, slot=1, kind=77)
    add("frame 1 op 0.*kernel size", disk, ksize=4)
    add("frame 1 op 0.*kernel size", disk, ksize=27)
    add("frame 1 op 0.*kernel size", disk, ksize=0)
    add("frame 1 op 0.*past the table", disk, tap_offset=1)
    add("frame 1 op 0.*past the table", disk, tap_offset=-1)
    add("frame 0 op 0.*2\\^15", disk, taps=disk.taps + np.uint16(1))
    add("frame 1 op 0.*block size", c.op_pixelate(2), u0=1)
    add("frame 1 op 0.*block size", c.op_pixelate(2), u0=65)
    q = c.jpeg_qtables(50).copy()
    q[1, 63] = 0
    add("frame 0 op 0.*zero", c.op_jpeg(50), qtables=q.reshape(1, 2, 64))
    add("frame 1 op 0.*table", c.op_jpeg(50), table=1)
    add("frame 1 op 0.*table", c.op_lut(c.lut_gamma(2.0)), table=-1)
    add("frame 1 op 0.*sigma", c.op_gaussian_noise(1.0), f0=np.nan)
    add("frame 1 op 0.*sigma", c.op_gaussian_noise(1.0), f0=np.inf)
    add("frame 1 op 0.*sigma", c.op_gaussian_noise(1.0), f0=-0.5)
    add("frame 1 op 0.*sigma", c.op_gaussian_noise(1.0), f0=128.5)
    add("frame 1 op 0.*contrast", c.op_contrast(1.0), f0=np.nan)
    add("frame 1 op 0.*fog", c.op_fog(1), u0=257)
    return out


def test_bad_descriptions_are_refused_by_frame_and_op(eng):
    c = _mod()
    frames, chains, ids = _upload_case()
    eng.upload_frames_u8_ragged(frames)
    before = eng.get_images().copy()
    bad = _bad_descriptions()
    for match, ops, taps, luts, qts in bad:
        with pytest.raises(ValueError, match=match):
            _run(frames, None, ops_arrays=(ops, taps, luts, qts))
        with pytest.raises(ValueError, match=match):
            eng.set_upload_corruption(None, ops_arrays=(ops, taps, luts, qts))
        with pytest.raises(ValueError):                              # the Python restatement agrees
            c.validate(ops, taps, luts, qts)
    five = np.zeros((3, 5), c.OP_DTYPE)
    for run in (lambda: _run(frames, None, ops_arrays=(five, [], [], [])),
                lambda: eng.set_upload_corruption(None, ops_arrays=(five, [], [], []))):
        with pytest.raises(ValueError, match="ops_per_frame 5 outside 1..4"):
            run()
    # nothing was left pending and nothing changed on the handle
    assert np.array_equal(eng.get_images(), before)
    eng.upload_frames_u8(np.stack([frames[1]] * 3))
    eng.upload_frames_u8_ragged(frames)
    assert np.array_equal(eng.get_images(), before)
    # a good description that follows a refused one is the one that stays pending
    eng.set_upload_corruption(chains, ids, seed=9)
    with pytest.raises(ValueError):
        eng.set_upload_corruption(None, ops_arrays=bad[0][1:])
    eng.upload_frames_u8_ragged(frames)
    assert not np.array_equal(eng.get_images(), before)


# ---- drivers ------------------------------------------------------------------------------------------------------------------
def _bdd_tree(tmp_path):
    """Four JPEG frames at the network size in a BDD-layout tree, with one label box per frame."""
    import json
    from PIL import Image
    root = tmp_path / "bdd100k"
    (root / "images" / "100k" / "val").mkdir(parents=True)
    (root / "labels").mkdir()
    rng = np.random.RandomState(2)
    y, x = np.mgrid[0:128, 0:128]
    names, labels = [], []
    for i in range(4):
        f = np.clip(np.stack([x + 20 * i, 2 * y, 255 - x], axis=-1) + rng.randint(-30, 31, (128, 128, 3)), 0, 255).astype(np.uint8)
        name = "f%d.jpg" % i
        Image.fromarray(f).save(str(root / "images" / "100k" / "val" / name), format="JPEG", quality=92, subsampling=2 if i % 2 else 0)
        names.append(name[:-4])
        labels.append({"name": name, "category": "car", "bbox": [20.0, 30.0, 90.0, 100.0]})
    (root / "labels" / "val.json").write_text(json.dumps([]))
    return root, names, labels


def _trees_equal(a, b, names):
    for n in names:
        for kind in ("mean", "cov", "cat_param", "cat_count"):
            x, y = np.load(os.path.join(a, kind, n + ".npy")), np.load(os.path.join(b, kind, n + ".npy"))
            if x.shape != y.shape or not np.array_equal(x, y):
                return False
    return True


def test_run_inference_corrupt_and_offline_eval_shift(tmp_path, monkeypatch, capsys):
    import json
    import yaml
    from bayes_od_rc_amd import config_utils, offline_eval, run_inference, synthetic
    from bayes_od_rc_amd.engine import Engine
    from bayes_od_rc_amd.model import RetinaNetModel
    root, names, labels = _bdd_tree(tmp_path)
    weights = str(tmp_path / "weights.npz")
    RetinaNetModel.save_weights_npz(synthetic.make_weights(8, 9, cls_fg_bias=-1.0), weights)
    here = os.path.dirname(os.path.abspath(run_inference.__file__))
    cfg = config_utils.load_yaml(os.path.join(here, "configs", "retinanet_bdd_covar.yaml"))
    cfg["dataset_config"]["bdd"]["paths_config"]["dataset_dir"] = str(root)
    ypath = tmp_path / "retinanet_bdd_covar.yaml"          # the file name must equal checkpoint_name
    ypath.write_text(yaml.safe_dump(cfg))
    base = ["--gpu_device", "0", "--yaml_path", str(ypath), "--data_split", "test", "--dataset", "--weights", weights]
    seen = []
    real = Engine.set_upload_corruption
    monkeypatch.setattr(Engine, "set_upload_corruption", lambda self, *a, **k: (seen.append(list(k.get("frame_ids"))), real(self, *a, **k))[1])

    def run(tag, extra):
        monkeypatch.setenv("BAYESOD_DATA_DIR", str(tmp_path / tag))
        del seen[:]
        return run_inference.main(base + extra), [list(s) for s in seen]

    clean, ids = run("clean", ["--batch", "4"])
    assert ids == []
    noisy, ids = run("noisy", ["--batch", "4", "--corrupt", "gaussian_noise:3", "--corrupt_seed", "5"])
    assert ids == [[0, 1, 2, 3]]                            # the dataset indices
    assert not _trees_equal(clean, noisy, names)
    jpeg, ids = run("jpeg", ["--batch", "4", "--corrupt", "gaussian_noise:3", "--corrupt_seed", "5", "--device_jpeg"])
    assert ids == [[0, 1, 2, 3]] and _trees_equal(noisy, jpeg, names)
    split, ids = run("split", ["--batch", "2", "--corrupt", "gaussian_noise:3", "--corrupt_seed", "5"])
    assert ids == [[0, 1], [2, 3]] and _trees_equal(noisy, split, names)
    other, _ = run("other", ["--batch", "4", "--corrupt", "gaussian_noise:3", "--corrupt_seed", "6"])
    assert not _trees_equal(noisy, other, names)
    with pytest.raises(SystemExit):
        run_inference.main(["--gpu_device", "0", "--data_split", "test", "--synthetic", "2", "--corrupt", "fog:1"])
    with pytest.raises(SystemExit):
        run_inference.main(base + ["--corrupt", "fog:7"])
    total = sum(np.load(os.path.join(noisy, "mean", n + ".npy")).shape[0] for n in names)
    print("detections over the four corrupted frames:", total)
    lab = tmp_path / "labels.json"
    lab.write_text(json.dumps([dict(l, name=l["name"][:-4]) for l in labels]))
    capsys.readouterr()
    out = offline_eval.main(["shift", "--labels", str(lab), "--predictions", "clean=" + clean, "noise3=" + noisy, "--gpu-device", "0",
                             "--samples", "64", "--score-threshold", "0.05"])
    text = capsys.readouterr().out
    assert out["names"] == ["clean", "noise3"] and set(out["reports"]) == {"clean", "noise3"}
    assert text.splitlines()[0].split() == ["metric", "clean", "noise3"]
    assert any(l.startswith("n_fp") for l in text.splitlines())


def test_run_validation_corrupt(tmp_path, monkeypatch):
    """--corrupt on the validation driver (the KITTI tree of the mixed-size tests): the losses move, and a frame's loss does not
    depend on the batch it falls into (frame ids are dataset indices)."""
    from bayes_od_rc_amd import run_validation
    from test_gpu_mixed_sizes import _kitti_tree, _yaml
    from test_gpu_validation_boxes import _checkpoint
    root, ids = _kitti_tree(tmp_path, "val")

    def edit(cfg):
        cfg["dataset_config"]["dataset"] = "kitti"
    ypath = _yaml(tmp_path, root, edit)
    real_batch = run_validation.validate_batch
    results = {}
    for tag, flags in (("clean", ["--batch", "4", "--mixed_sizes"]), ("noisy4", ["--batch", "4", "--corrupt", "gaussian_noise:4"]),
                       ("noisy2", ["--batch", "2", "--corrupt", "gaussian_noise:4"])):
        (tmp_path / tag).mkdir()
        monkeypatch.setenv("BAYESOD_DATA_DIR", str(tmp_path / tag / "data"))
        _checkpoint(tmp_path / tag, 4)
        totals, seen_ids = [], []

        def watched_batch(model, config, batch, **kw):
            out = real_batch(model, config, batch, **kw)
            totals.extend(float(t) for t, _, _, _ in out)
            seen_ids.append(None if kw.get("corruption") is None else list(kw["corruption"][1]))
            return out
        monkeypatch.setattr(run_validation, "validate_batch", watched_batch)
        res = run_validation.main(["--gpu_device", "0", "--yaml_path", ypath, "--data_split", "val", "--dataset"] + flags)
        monkeypatch.setattr(run_validation, "validate_batch", real_batch)
        assert len(res) == 1 and res[0]["num_frames"] == 5
        results[tag] = (totals, seen_ids, res[0]["mean_total_loss"])
    assert results["clean"][1] == [None, None]
    assert results["noisy4"][1] == [[0, 1, 2, 3], [4]] and results["noisy2"][1] == [[0, 1], [2, 3], [4]]
    assert results["noisy4"][0] == results["noisy2"][0]
    assert all(a != b for a, b in zip(results["clean"][0], results["noisy4"][0]))
    print("validation loss clean / gaussian_noise:4:", results["clean"][2], results["noisy4"][2])
    with pytest.raises(SystemExit):
        run_validation.main(["--gpu_device", "0", "--synthetic", "2", "--corrupt", "fog:1"])

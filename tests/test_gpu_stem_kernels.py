"""GPU: every stem and stem-pool kernel of aux_kernels.hip alone, through bod_stage_stem / bod_stage_stem_pool
(the library's own launchers on sentinel-filled, guarded planes) against tests/stem_reference.py:

(a) impulse images -- one impulse per 7x7 window, so one product per operand split and ONE rounding (the bias add): stem and
    pooled planes bit for bit, in every form;
(b) random images against float64 on the kernel's own operands, every element inside a derived interval (stem_reference.bound;
    rounding, ReLU and max are monotone, so a bf16 output lies in [bf16(relu(ref - e)), bf16(relu(ref + e))] and a pooled one
    between the pools of those planes);
(c) the forms the code claims bit-identical, plane against plane;
(d) the pooled border keeps the sentinel, nothing is written outside a plane (the entry's guards), and the input row / column
    no window reaches holds +-1e30 in EVERY image of (a) and (b) without changing an output;
(e) the three pooling kernels alone on planted planes, bit for bit.

Shapes are the smallest that reach each edge: one pixel, a second segment of one pixel, three segments, closing rows of
either parity, a ring that wraps more than twice, and one case per persistent kernel with more tasks than its grid cap."""
import os

import numpy as np
import pytest

import stem_reference as R

pytestmark = pytest.mark.gpu

KIND = {"f32+pool_f32": "fp32", "f32+pool_split": "fp32", "seg64+pool": "bf16", "row+pool": "bf16", "fused8": "bf16", "fused4": "bf16",
        "fused_split": "split"}
PAIRS = ("f32+pool_split", "fused_split")
# family -> (forms under test, widths, heights); (c) also runs the 64-pixel and row forms on the row and fused families' shapes
FAMILIES = {
    "seg64": (("f32+pool_f32", "f32+pool_split", "seg64+pool"), (7, 9, 133, 135, 263), (7, 8, 9, 12)),
    "row": (("row+pool",), (8, 12, 516, 520, 1032), (7, 8, 9, 12)),
    "fused": (("fused8", "fused4", "fused_split"), (8, 12, 132, 260, 512, 516), (7, 8, 9, 10, 11, 23, 24, 41)),
}
BATCHES = (1, 3)
FAMILY_W = [(f, w) for f, v in FAMILIES.items() for w in v[1]]
# more tasks than the grid cap of each persistent kernel: the prefetch / commit double buffer alternates
PERSISTENT = [("f32+pool_f32", 5, 421, 9, 1024), ("seg64+pool", 4, 393, 9, 768), ("row+pool", 2, 267, 8, 256), ("row+pool", 1, 267, 520, 256)]

_cache = {}


def _inputs(image, kind, b, h, w):
    """Image, weights and bias of a case, shared by every form of one operand family.  Impulse values depend on the family (a lo
    part for the bf16 kernels, powers of two for the fp32 stem and the split kernel); random images are the same for all."""
    vals = "lo" if kind == "bf16" else "pow2"
    key = ("in", image, vals if image == "impulse" else "", b, h, w)
    if key not in _cache:
        rng = np.random.default_rng([b, h, w, 1 if image == "impulse" else 2, 1 if vals == "lo" else 2])
        wt, bias = R.random_weights(rng)
        if image == "impulse":
            img = R.impulse_image(b, h, w, R.VALUES_LO if vals == "lo" else R.VALUES_POW2, rng)
        else:
            img = R.random_image(b, h, w, rng)
            bias[5], bias[17] = -4000.0, 4000.0             # one channel all zero after the ReLU, one that never clips
        _cache[key] = (img, wt, bias)
    return _cache[key]


def _run(form, image, b, h, w):
    from bayes_od_rc_amd.engine import stage_stem
    key = ("run", form, image, b, h, w)
    if key not in _cache:
        img, wt, bias = _inputs(image, KIND[form], b, h, w)
        out = stage_stem(img, wt, bias, form)
        assert out["form"] == form
        _cache[key] = out
    return _cache[key]


def _reference(what, kind, image, b, h, w):
    key = (what, kind, image, b, h, w)
    if key not in _cache:
        img, wt, bias = _inputs(image, kind, b, h, w)
        _cache[key] = R.impulse_expected(kind, img, wt, bias)[0] if what == "impulse" else R.bound(kind, img, wt, bias)
    return _cache[key]


def _diff(a, b):
    """Number of elements that differ (NaN differs from everything: a host buffer the entry did not fill shows)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int((~(a == b)).sum())


def _split_border(pooled):
    """(interior, border elements) of a pooled plane [B,ph+2,pw+2,C]."""
    mask = np.ones(pooled.shape[1:3], bool)
    mask[1:-1, 1:-1] = False
    return pooled[:, 1:-1, 1:-1, :], pooled[:, mask, :]


def _check_planes_are_whole(out, b, h, w):
    """(d): geometry, border = sentinel, every interior / stem element written (none is the sentinel, none NaN)."""
    oh, ow, ph, pw = R.geometry(h, w)
    slots = 128 if out["form"] in PAIRS else 64
    assert out["pooled"].shape == (b, ph + 2, pw + 2, slots)
    inner, border = _split_border(out["pooled"])
    assert _diff(border, np.full_like(border, R.SENTINEL)) == 0, "the pooled border was written"
    assert np.isfinite(inner).all() and not (inner == R.SENTINEL).any()
    if out["stem"] is not None:
        assert out["stem"].shape == (b, oh, ow, 64)
        assert np.isfinite(out["stem"]).all() and (out["stem"] >= 0).all()
    return inner


def _shapes(family):
    heights = FAMILIES[family][2]
    return [(b, h) for h in heights for b in BATCHES]


# ------------------------------------------------------------------------------------------------ (a) impulse images, bit for bit
@pytest.mark.parametrize("family,w", FAMILY_W)
def test_impulse_images_bit_for_bit(family, w):
    forms = FAMILIES[family][0]
    wrong = {}
    for b, h in _shapes(family):
        for form in forms:
            out = _run(form, "impulse", b, h, w)
            inner = _check_planes_are_whole(out, b, h, w)
            exp = _reference("impulse", KIND[form], "impulse", b, h, w)
            assert (exp > 0).any() and (exp == 0).any()
            n = 0 if out["stem"] is None else _diff(out["stem"], exp)
            pooled = R.pool(exp)                                    # the exact maximum
            n += _diff(inner, R.pairs_of(pooled) if form in PAIRS else pooled)
            if n:
                wrong[(form, b, h, w)] = n
    print("impulse %s W=%d: %d cases, differing elements %s" % (family, w, len(forms) * len(_shapes(family)), wrong or 0))
    assert not wrong, wrong


# ------------------------------------------------------------------------------------------------ (b) random images, derived interval
def _check_random(form, b, h, w):
    """Every element of a random-image run inside its interval; returns the worst err / e of an fp32 or pair form (else 0)."""
    out = _run(form, "random", b, h, w)
    inner = _check_planes_are_whole(out, b, h, w)
    kind = KIND[form]
    ref, e = _reference("bound", kind, "random", b, h, w)
    assert (ref[..., 5] + e[..., 5] < 0).all() and (ref[..., 17] - e[..., 17] > 0).all()       # both sides of the ReLU occur
    lo64, hi64 = R.relu(ref - e), R.relu(ref + e)
    worst = 0.0
    if kind == "bf16":
        lo, hi = R.bf16_round(lo64), R.bf16_round(hi64)
        if out["stem"] is not None:
            bad = (out["stem"] < lo) | (out["stem"] > hi)
            assert not bad.any(), (form, b, h, w, int(bad.sum()), np.argwhere(bad)[:4].tolist())
            assert (out["stem"][..., 5] == 0).all() and (out["stem"][..., 17] > 0).all()
        plo, phi = R.pool(lo), R.pool(hi)
        bad = (inner < plo) | (inner > phi)
        assert not bad.any(), (form, b, h, w, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        assert (inner[..., 5] == 0).all() and (inner[..., 17] > 0).all()
        return worst
    if out["stem"] is not None:                                    # the fp32 stem: |got - ref| <= e under the monotone ReLU
        got = out["stem"].astype(np.float64)
        bad = (got < lo64) | (got > hi64)
        assert not bad.any(), (form, b, h, w, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        worst = float((np.abs(got - R.relu(ref)) / e).max())
        exact = R.pool(out["stem"])                                # and the pooling launch on that very plane is exact
        assert _diff(inner, R.pairs_of(exact) if form in PAIRS else exact) == 0
    if form in PAIRS:                                              # hi + lo within e + 2^-17 |ref| of the pooled reference
        hi, lo = R.pairs_split(inner)
        assert (hi >= 0).all() and (np.abs(lo) <= 2.0 ** -8 * hi).all(), "not 32 hi then 32 lo per 64-slot group"
        assert _diff(hi, R.bf16_round(hi)) == 0 and _diff(lo, R.bf16_round(lo)) == 0
        s = hi.astype(np.float64) + lo.astype(np.float64)
        plo, phi, pref = R.pool(lo64), R.pool(hi64), R.pool(R.relu(ref))
        bad = (s < plo - 2.0 ** -17 * plo) | (s > phi + 2.0 ** -17 * phi)
        assert not bad.any(), (form, b, h, w, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        assert (s[..., 5] == 0).all() and (s[..., 17] > 0).all()
        room = np.maximum(phi - pref, pref - plo) + 2.0 ** -17 * pref
        ok = room > 0
        worst = max(worst, float((np.abs(s - pref)[ok] / room[ok]).max()))
    return worst


@pytest.mark.parametrize("family,w", FAMILY_W)
def test_random_images_inside_the_derived_interval(family, w):
    worst = {}
    for b, h in _shapes(family):
        for form in FAMILIES[family][0]:
            worst[form] = max(worst.get(form, 0.0), _check_random(form, b, h, w))
    print("random %s W=%d: worst err/e %s" % (family, w, {k: "%.4f" % v for k, v in worst.items() if KIND[k] != "bf16"}))


@pytest.mark.parametrize("form,b,h,w,cap", PERSISTENT)
def test_more_tasks_than_the_grid_cap(form, b, h, w, cap):
    oh, ow, _, _ = R.geometry(h, w)
    seg = 256 if form == "row+pool" else 64
    assert b * oh * ((ow + seg - 1) // seg) > cap
    worst = _check_random(form, b, h, w)
    if form == "row+pool":                                         # (c) on the same case
        other = _run("seg64+pool", "random", b, h, w)
        assert _diff(_run(form, "random", b, h, w)["stem"], other["stem"]) == 0
    print("persistent %s B=%d H=%d W=%d: worst err/e %.4f" % (form, b, h, w, worst))


# ------------------------------------------------------------------------------------------------ (c) forms that claim identity
@pytest.mark.parametrize("family,w", [fw for fw in FAMILY_W if fw[0] != "seg64"])
def test_forms_are_bit_identical_plane_against_plane(family, w):
    n = 0
    for b, h in _shapes(family):
        for image in ("impulse", "random"):
            row, seg = _run("row+pool", image, b, h, w), _run("seg64+pool", image, b, h, w)
            assert _diff(row["stem"], seg["stem"]) == 0, (image, b, h, w)
            assert _diff(row["pooled"], seg["pooled"]) == 0, (image, b, h, w)
            if family == "fused":
                for form in ("fused8", "fused4"):
                    assert _diff(_run(form, image, b, h, w)["pooled"], row["pooled"]) == 0, (form, image, b, h, w)
            n += 1
    print("identity %s W=%d: %d plane pairs, 0 differing bits" % (family, w, n))


# ------------------------------------------------------------------------------------------------ the library's own rule, refusals
def _env(name):
    v = os.environ.get(name)
    return None if v is None else int(v)


def test_the_librarys_rule_picks_the_form_and_a_misaligned_image_falls_back():
    from bayes_od_rc_amd.engine import stage_stem
    seg_forced = _env("BOD_STEM_SEG64") == 1
    fused_on = _env("BOD_STEM_POOL_FUSED") != 0 and _env("BOD_STEM_POOL_FUSED_MIN_B") is None
    fused = "fused4" if _env("BOD_STEM_WAVES") == 4 else "fused8"
    split_fused = fused_on and _env("BOD_STEM_SPLIT_FUSED") != 0
    row = "seg64+pool" if seg_forced else "row+pool"
    b, h = 3, 9
    cases = [("bf16", 12, False, 0, row),                           # three images on a 256-CU rule: the two launches
             ("bf16", 12, False, 1, fused if fused_on else row),    # a one-CU share: the fused kernel
             ("bf16", 12, True, 1, "seg64+pool"),                   # 4 bytes off: neither 16-byte-load kernel
             ("bf16", 9, False, 1, "seg64+pool"),                   # W % 4 != 0
             ("bf16", 520, False, 1, row),                          # 257 stem pixels: not the fused kernel
             ("bf16", 520, True, 1, "seg64+pool"),
             ("fp32", 12, False, 1, "f32+pool_f32"), ("fp32", 12, True, 1, "f32+pool_f32"),
             ("bf16x3", 12, False, 1, "fused_split" if split_fused else "f32+pool_split"),
             ("bf16x3", 12, False, 0, "f32+pool_split"), ("bf16x3", 12, True, 1, "f32+pool_split"),
             ("bf16x3", 520, False, 1, "f32+pool_split")]
    for precision, w, misalign, n_cu, expect in cases:
        kind = {"fp32": "fp32", "bf16": "bf16", "bf16x3": "fp32"}[precision]
        img, wt, bias = _inputs("random", kind, b, h, w)
        out = stage_stem(img, wt, bias, "auto", precision=precision, misalign=misalign, n_cu=n_cu)
        assert out["form"] == expect, (precision, w, misalign, n_cu, out["form"], expect)
        _check_planes_are_whole(out, b, h, w)
        same = _run(out["form"], "random", b, h, w)                 # the same kernel on an aligned copy: the same bits
        assert _diff(out["pooled"], same["pooled"]) == 0
        if out["stem"] is not None:
            assert _diff(out["stem"], same["stem"]) == 0
    # an explicit 64-pixel or fp32 form takes a misaligned image as well
    for form in ("seg64+pool", "f32+pool_f32", "f32+pool_split"):
        img, wt, bias = _inputs("random", KIND[form], b, h, 12)
        out = stage_stem(img, wt, bias, form, misalign=True)
        assert _diff(out["pooled"], _run(form, "random", b, h, 12)["pooled"]) == 0


def test_shapes_a_kernel_is_not_built_for_are_refused_before_any_launch():
    from bayes_od_rc_amd.engine import stage_stem
    img, wt, bias = _inputs("random", "bf16", 1, 8, 520)
    for form in ("fused8", "fused4", "fused_split"):                # W = 520: 257 stem pixels
        with pytest.raises(ValueError, match="at most 256"):
            stage_stem(img, wt, bias, form)
    assert stage_stem(img, wt, bias, "row+pool")["form"] == "row+pool"
    img9 = _inputs("random", "bf16", 1, 8, 9)[0]
    for form in ("row+pool", "fused8", "fused4", "fused_split"):
        with pytest.raises(ValueError, match="W % 4 == 0"):
            stage_stem(img9, wt, bias, form)
        with pytest.raises(ValueError, match="16-byte aligned"):
            stage_stem(_inputs("random", "bf16", 1, 8, 12)[0], wt, bias, form, misalign=True)


# ------------------------------------------------------------------------------------------------ (e) the pooling kernels alone
def _planted_planes():
    """Non-negative stem planes (the kernels' zero padding stands for ZeroPadding2D under a ReLU), [name, plane]."""
    rng = np.random.default_rng(77)
    special = np.array([0.0, 2.0 ** -133, 2.0 ** -127, 1e-39, 2.0 ** -126, 1.0, 3.0e38, 65280.0, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -20,
                        257.0 / 3.0], np.float32)
    planes = []
    for ih in (1, 2, 3):
        for iw in (1, 2, 3):
            v = np.abs(rng.normal(0, 3, (3, ih, iw, 64))).astype(np.float32)
            pick = rng.uniform(size=v.shape) < 0.4
            v[pick] = special[rng.integers(0, special.size, int(pick.sum()))]
            planes.append(("small %dx%d" % (ih, iw), v))
    for ih, iw in ((7, 9), (6, 8)):
        oh, ow = (ih - 1) // 2 + 1, (iw + 1) // 2 + 1
        for ky in range(3):
            for kx in range(3):                                    # the maximum of every window at position (ky, kx), where inside
                v = rng.uniform(0, 1, (1, ih, iw, 64)).astype(np.float32)
                ys, xs = 2 * np.arange(oh) + ky - 1, 2 * np.arange(ow) + kx - 2
                ys, xs = ys[(ys >= 0) & (ys < ih)], xs[(xs >= 0) & (xs < iw)]
                v[:, ys[:, None], xs[None, :], :] += rng.uniform(2, 100, (1, ys.size, xs.size, 64)).astype(np.float32)
                planes.append(("max at (%d,%d) of %dx%d" % (ky, kx, ih, iw), v))
        planes.append(("equal maxima %dx%d" % (ih, iw), np.full((1, ih, iw, 64), 5.0, np.float32)))
        planes.append(("all zero %dx%d" % (ih, iw), np.zeros((3, ih, iw, 64), np.float32)))
        v = rng.uniform(0, 1, (3, ih, iw, 64)).astype(np.float32)
        for sl in ((slice(None), 0), (slice(None), ih - 1), (slice(None), slice(None), 0), (slice(None), slice(None), iw - 1)):
            v[sl] += rng.uniform(10, 1000, v[sl].shape).astype(np.float32)
        planes.append(("border maxima %dx%d" % (ih, iw), v))
        v = np.abs(rng.normal(0, 3, (3, ih, iw, 64))).astype(np.float32)
        pick = rng.uniform(size=v.shape) < 0.5
        v[pick] = special[rng.integers(0, special.size, int(pick.sum()))]
        planes.append(("subnormal and large %dx%d" % (ih, iw), v))
    return planes


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_pooling_kernels_alone_bit_for_bit(mode):
    from bayes_od_rc_amd.engine import stage_stem_pool
    wrong = {}
    planes = _planted_planes()
    for name, v in planes:
        if mode == 0:
            v = R.bf16_round(v)                                    # what the bf16 plane holds
        got = stage_stem_pool(v, mode)
        b, ih, iw, _ = v.shape
        oh, ow = (ih - 1) // 2 + 1, (iw + 1) // 2 + 1
        assert got.shape == (b, oh + 2, ow + 2, 128 if mode == 2 else 64)
        inner, border = _split_border(got)
        assert _diff(border, np.full_like(border, R.SENTINEL)) == 0, name
        exp = R.pool(v)
        assert exp.dtype == np.float32 and exp.shape == (b, oh, ow, 64)
        if mode == 2:
            hi, lo = R.pairs_split(inner)
            assert _diff(hi, R.bf16_round(exp)) == 0 and _diff(lo, R.bf16_round(exp - R.bf16_round(exp))) == 0, name
            exp = R.pairs_of(exp)
        n = _diff(inner, exp) + int((np.signbit(inner) != np.signbit(exp)).sum())
        if n:
            wrong[name] = n
    print("pooling mode %d: %d planes, differing elements %s" % (mode, len(planes), wrong or 0))
    assert not wrong, wrong

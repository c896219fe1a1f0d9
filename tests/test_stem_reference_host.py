"""CPU: tests/stem_reference.py against torch in float64, the exactness claims tests/test_gpu_stem_kernels.py rests on, the
bound's slack and bite on an fp32 emulation, and the host-side refusals of bod_stage_stem / bod_stage_stem_pool (nothing is
launched on a bad argument, so they are refused without a GPU too)."""
import ctypes as C
import os

import numpy as np
import pytest

import stem_reference as R
from conftest import ROOT

SHAPES = [(1, 7, 7), (3, 8, 9), (2, 12, 135), (1, 9, 133), (2, 11, 132), (1, 41, 516), (1, 12, 263)]


def _torch_stem(img, w, bias):
    import torch
    import torch.nn.functional as F
    x = torch.from_numpy(np.asarray(img, np.float64)).permute(0, 3, 1, 2)
    k = torch.from_numpy(np.asarray(w, np.float64)).permute(3, 2, 0, 1)
    y = F.conv2d(x, k, torch.from_numpy(np.asarray(bias, np.float64)), stride=2)
    p = F.max_pool2d(F.pad(F.relu(y), (2, 2, 1, 1)), 3, 2)
    return y.permute(0, 2, 3, 1).numpy(), p.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("b,h,w", SHAPES)
def test_reference_matches_torch_in_float64(b, h, w):
    rng = np.random.default_rng(h * 1000 + w)
    img = R.clean(R.random_image(b, h, w, rng))
    wt, bias = R.random_weights(rng)
    ref = R.conv(img, wt) + bias.astype(np.float64)
    y, p = _torch_stem(img, wt, bias)
    oh, ow, ph, pw = R.geometry(h, w)
    assert ref.shape == (b, oh, ow, 64) and y.shape == ref.shape
    scale = np.abs(y).max()
    assert np.abs(ref - y).max() <= 1e-12 * scale
    pooled = R.pool(R.relu(ref))
    assert pooled.shape == (b, ph, pw, 64) == p.shape
    assert np.abs(pooled - p).max() <= 1e-12 * scale
    assert np.array_equal(R.pool(R.relu(y)), p)                   # the pooling alone: exact


def test_unreached_rows_and_columns_are_what_the_convolution_never_reads():
    rng = np.random.default_rng(1)
    for h, w in [(8, 9), (7, 8), (10, 12), (9, 135)]:
        img = R.random_image(2, h, w, rng)
        row, col = R.unreached(h, w)
        assert row == (h % 2 == 0) and col == (w % 2 == 0)
        assert (np.abs(img) >= 1e29).any() == (row or col)
        wt, _ = R.random_weights(rng)
        assert np.array_equal(R.conv(img, wt), R.conv(R.clean(img), wt))        # float64 holds 1e30 * w: it is simply never read
        hi, lo = R.split_hi_lo(img)
        assert np.isfinite(hi).all() and np.isfinite(lo).all()


def test_pair_layout_round_trip():
    rng = np.random.default_rng(2)
    v = np.abs(rng.normal(0, 30, (2, 3, 4, 64))).astype(np.float32)
    slots = R.pairs_of(v)
    assert slots.shape == (2, 3, 4, 128)
    hi, lo = R.pairs_split(slots)
    assert np.array_equal(hi, R.bf16_round(v)) and np.array_equal(lo, R.bf16_round(v - hi))
    for c in (0, 31, 32, 63):                                     # channel c: hi at (c >> 5) * 64 + (c & 31), lo 32 slots on
        s = (c >> 5) * 64 + (c & 31)
        assert np.array_equal(slots[..., s], hi[..., c]) and np.array_equal(slots[..., s + 32], lo[..., c])
    assert np.abs(hi.astype(np.float64) + lo - v).max() <= 2.0 ** -17 * np.abs(v).max()


# ------------------------------------------------------------------------------------------------ exactness of the impulse planes
@pytest.mark.parametrize("kind,values", [("bf16", R.VALUES_LO), ("fp32", R.VALUES_POW2), ("split", R.VALUES_POW2)])
def test_impulse_sums_are_exact_in_fp32(kind, values):
    """The GPU test's 'one rounding' claim: with these values every pre-bias sum of an impulse image (one product per operand
    split) and every partial sum of it is an fp32 number, so the accumulation order cannot matter."""
    rng = np.random.default_rng(3)
    wt, bias = R.random_weights(rng)
    wo = {"bf16": R.bf16_round(wt).astype(np.float64), "fp32": wt.astype(np.float64), "split": R.split_weights_sum(wt)}[kind]
    # every value times every weight, and for the bf16 family each half of the value on its own
    halves = [values.astype(np.float64)]
    if kind == "bf16":
        hi, lo = R.split_hi_lo(values)
        assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64), values.astype(np.float64))      # x = hi + lo exactly
        assert (lo != 0).sum() >= 3                                # the lo path carries something
        halves += [hi.astype(np.float64), lo.astype(np.float64)]
    if kind == "split":
        whi, wlo = R.split_hi_lo(wt)
        assert np.array_equal(R.split_weights_sum(wt).astype(np.float32).astype(np.float64), R.split_weights_sum(wt))
        for part in (whi, wlo):
            p = values.astype(np.float64)[:, None] * part.astype(np.float64).reshape(1, -1)
            assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    for v in halves:
        p = v[:, None] * wo.reshape(1, -1)
        assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    # and the planes the GPU test expects, on a few of its shapes
    for b, h, w in [(1, 7, 7), (3, 8, 9), (2, 12, 135), (1, 23, 132)]:
        img = R.impulse_image(b, h, w, values, rng)
        exp, s = R.impulse_expected(kind, img, wt, bias)
        assert np.array_equal(s.astype(np.float32).astype(np.float64), s)
        # exactly one impulse per window: the sum is one product
        nz = (R.patches(R.clean(img)) != 0).sum(axis=-1)
        assert np.array_equal(nz, np.ones_like(nz))
        assert (exp > 0).any() and (exp == 0).any()


def test_a_24_bit_weight_times_a_value_with_a_lo_part_is_not_exact():
    """Why the fp32 stem and the split kernel get powers of two only."""
    rng = np.random.default_rng(4)
    wt, _ = R.random_weights(rng)
    p = R.VALUES_LO.astype(np.float64)[:3, None] * wt.astype(np.float64).reshape(1, -1)
    assert not np.array_equal(p.astype(np.float32).astype(np.float64), p)


# ------------------------------------------------------------------------------------------------ the bound: slack and bite
def _fp32_chain(xparts, wo):
    """Sequential fp32 accumulation of the products of every operand part, the way a plain fp32 adder chain would."""
    acc = None
    w32 = wo.reshape(147, 64).astype(np.float32)
    for xp in xparts:
        p32 = R.patches(xp).astype(np.float32)
        if acc is None:
            acc = np.zeros(p32.shape[:3] + (64,), np.float32)
        for k in range(147):
            acc = acc + p32[..., k:k + 1] * w32[k]
    return acc


def test_bf16_bound_holds_an_fp32_chain_and_catches_a_wrong_tap():
    rng = np.random.default_rng(5)
    img = R.random_image(2, 12, 135, rng)
    wt, bias = R.random_weights(rng)
    bias[5], bias[17] = -4000.0, 4000.0
    ref, e = R.bound("bf16", img, wt, bias)
    lo, hi = R.bf16_round(R.relu(ref - e)), R.bf16_round(R.relu(ref + e))
    two = float((lo != hi).mean())
    assert 0.02 < two < 0.25                                      # most outputs have one allowed value
    xhi, xlo = R.split_hi_lo(R.clean(img))
    wb = R.bf16_round(wt)
    acc = _fp32_chain([xhi, xlo], wb)
    worst = float((np.abs(acc.astype(np.float64) + bias.astype(np.float64) - ref) / e).max())
    assert worst < 0.1, worst
    got = R.bf16_round(np.maximum(acc + bias, np.float32(0)))
    assert ((got >= lo) & (got <= hi)).all()
    pl, phh = R.pool(lo), R.pool(hi)
    gp = R.pool(got)
    assert ((gp >= pl) & (gp <= phh)).all()
    assert (ref[..., 5] + e[..., 5] < 0).all() and (ref[..., 17] - e[..., 17] > 0).all()
    # one tap's weights taken from its neighbour
    wrong = wb.copy()
    wrong[3, 4] = wb[3, 5]
    bad = R.bf16_round(np.maximum(_fp32_chain([xhi, xlo], wrong) + bias, np.float32(0)))
    outside = float(((bad < lo) | (bad > hi)).mean())
    assert outside > 0.3, outside


def test_split_bound_holds_the_three_product_form():
    rng = np.random.default_rng(6)
    img = R.random_image(2, 12, 135, rng)
    wt, bias = R.random_weights(rng)
    ref, e = R.bound("split", img, wt, bias)
    xhi, xlo = R.split_hi_lo(R.clean(img))
    whi, wlo = R.split_hi_lo(wt)
    three = (R.conv(xhi, whi) + R.conv(xlo, whi) + R.conv(xhi, wlo)) + bias.astype(np.float64)
    mag = e / (442 * R.U + 2.0 ** -16)
    worst = float((np.abs(three - ref) / mag).max())
    assert worst < 2.0 ** -16, worst                              # (measured 2.2e-6 against 1.5e-5)


# ------------------------------------------------------------------------------------------------ host-side argument checks
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "bayes-od-rc_amd", "lib", "libbayesod_hip.so")):
        g.build()
    from bayes_od_rc_amd import _lib
    return _lib.load()


def _runs_or_fails_loudly(fn):
    import torch
    if torch.cuda.is_available():
        fn()
    else:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()


def test_stage_stem_refuses_what_a_kernel_is_not_built_for(lib):
    from bayes_od_rc_amd.engine import stage_stem, stem_geometry
    assert stem_geometry(12, 135) == R.geometry(12, 135) == (3, 65, 2, 34)
    z = lambda *s: np.zeros(s, np.float32)
    w, b = z(7, 7, 3, 64), z(64)
    _runs_or_fails_loudly(lambda: stage_stem(z(1, 8, 12, 3), w, b, "fused8"))
    bad = [dict(images=z(1, 8, 9, 3), form="row+pool"),                       # W % 4 != 0
           dict(images=z(1, 8, 9, 3), form="fused8"), dict(images=z(1, 8, 9, 3), form="fused4"),
           dict(images=z(1, 8, 9, 3), form="fused_split"),
           dict(images=z(1, 8, 12, 3), form="row+pool", misalign=True),       # 4 bytes off a 16-byte boundary
           dict(images=z(1, 8, 12, 3), form="fused8", misalign=True),
           dict(images=z(1, 8, 12, 3), form="fused_split", misalign=True),
           dict(images=z(1, 8, 520, 3), form="fused8"),                       # ow = 257
           dict(images=z(1, 8, 520, 3), form="fused4"), dict(images=z(1, 8, 520, 3), form="fused_split"),
           dict(images=z(1, 8, 12, 3), form="fused8", precision="fp32"),      # a form runs in its own precision
           dict(images=z(1, 8, 12, 3), form="f32+pool_f32", precision="bf16"),
           dict(images=z(1, 8, 12, 3), form="auto", precision="f16mx"),
           dict(images=z(1, 8, 12, 3), form="seg64+pool", sentinel=0.1),      # not a bf16 number
           dict(images=z(1, 8, 12, 3), form="seg64+pool", sentinel=float("inf")),
           dict(images=z(5, 1024, 1024, 3), form="seg64+pool")]               # more than 2^22 pixels
    for change in bad:
        kw = dict(dict(images=None, w=w, bias=b), **change)
        with pytest.raises(ValueError, match="bod_stage_stem"):
            stage_stem(**kw)
    for hw in [(6, 12), (12, 6)]:                                             # no window fits
        with pytest.raises(ValueError):
            stage_stem(z(1, hw[0], hw[1], 3), w, b, "seg64+pool")
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))                     # the C entry itself, past the wrapper's own check
    st = lib.bod_stage_stem(0, 3, 0, fp(z(1, 6, 12, 3)), 1, 6, 12, fp(w), fp(b), 0, 0, -65536.0, None, None, C.byref(C.c_int32(0)))
    assert st == 1 and b"H, W >= 7" in lib.bod_last_error(None)


def test_stage_stem_pool_refuses_bad_arguments(lib):
    from bayes_od_rc_amd.engine import stage_stem_pool
    z = lambda *s: np.zeros(s, np.float32)
    _runs_or_fails_loudly(lambda: stage_stem_pool(z(1, 3, 2, 64), 0))
    for stem, mode, kw in [(z(1, 3, 2, 64), 3, {}), (z(1, 3, 2, 64), -1, {}), (z(1, 3, 2, 64), 1, {"sentinel": 1.0 + 2.0 ** -12}),
                           (z(0, 3, 2, 64), 0, {})]:
        with pytest.raises(ValueError, match="bod_stage_stem_pool"):
            stage_stem_pool(stem, mode, **kw)
    with pytest.raises(ValueError):
        stage_stem_pool(z(1, 3, 2, 32), 0)

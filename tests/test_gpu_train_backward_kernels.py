"""GPU: the backward kernels that only the bf16 training handle launches, one layer at a time.

tests/test_gpu_train_step.py can hold the bf16 step as a whole only to direction and size (cosine, norm ratio); one layer deep,
sharp bounds exist.  Through the stage entry points bod_stage_act_backward / _conv_dgrad / _stem_pool_backward / _fold_pack
(the library's own launchers, called as train_backward / train_fold_all call them) against tests/train_backward_reference.py:

* activation backward (tile, vector and element forms, relu_merge ahead of it): dZ, its plane copy and its transposed copy bit
  for bit -- one fp32 multiply, one rounding --, padding channels and dZ^T columns [M, Kpad) zero, plane borders untouched; the
  residual gradient within 2^-22 of the sum of its terms' magnitudes (at most five terms, four fp32 roundings, any atomic order);
* the three input-gradient routes (CONV_OUT_F32 | CONV_ACCUM convolution on flipped weights, 1x1 through the dgrad row table,
  dXcol + col2im), with and without split-K, grouped, and on the 256x256 tile: 1e-3 of the gradient's rms against float64 autograd
  on the bf16-rounded operands plus the prefill (the bound of tests/test_gpu_train_blocks.py); pixels no window reaches keep
  their prefill exactly; forced split-K agrees with ksplit = 1 to 1e-5 of the rms (fp32 summation order);
* stem max-pool backward: bit for bit, ties to the first maximum in row-major order, in bf16 and fp32 mode;
* batch-norm fold and the three weight packings of five layers in one launch: bit for bit, folded bias within 4 * 2^-24.

Measured on an MI355X (this file's prints): see DESIGN.md 9.12."""
import numpy as np
import pytest

import train_backward_reference as R
from conftest import rel_err

pytestmark = pytest.mark.gpu

SENTINEL = -65536.0                      # exactly representable in bf16


def _rms(a):
    return float(np.sqrt((np.asarray(a, np.float64) ** 2).mean()))


# ------------------------------------------------------------------------------------------------ activation backward
_GRID = {1: (1, 1), 28: (4, 7), 29: (1, 29), 57: (3, 19), 63: (7, 9), 64: (8, 8), 65: (5, 13), 200: (10, 20)}


def _stored_output(rng, n):
    """What a layer may have stored: ReLU'd / dropped values with +0, -0, negative values (a layer with dropout and no ReLU),
    a value whose bf16 rounding is zero (1e-42) and a bf16 subnormal that is not (1e-39)."""
    v = (rng.normal(0, 1, n) * (rng.uniform(size=n) < 0.6)).astype(np.float32)
    special = np.array([0.0, -0.0, -1.5, 1e-42, -1e-42, 1e-39, -1e-39, 2.0 ** -127], np.float32)
    pick = rng.uniform(size=n) < 0.25
    v[pick] = special[rng.integers(0, special.size, int(pick.sum()))]
    return v


def _run_act(m, cout, cout_pad, kpad, stored, scale, res_mode, relu, want_dzp, want_dzt, precision, seed, plane=True):
    """One bod_stage_act_backward call against the restatement; returns the form that ran."""
    from bayes_od_rc_amd.engine import stage_act_backward
    rng = np.random.default_rng(seed)
    f32 = precision == "fp32"
    hh, ww = _GRID[m]
    ys, xs = np.divmod(np.arange(m), ww)
    if plane:                                            # a zero-bordered output plane, pixel stride cout_pad
        npix, cs = (hh + 2) * (ww + 2), cout_pad
        out_off = ((ys + 1) * (ww + 2) + xs + 1).astype(np.int32)
    else:                                                # dense rows (the fp32 head outputs), pixel stride cout
        npix, cs = m, cout
        out_off = np.arange(m, dtype=np.int32)
    n = npix * cs
    dout = rng.normal(0, 1, n).astype(np.float32)
    out_act = _stored_output(rng, n) if stored else None
    dout_relu = rng.normal(0, 1, n).astype(np.float32) if relu else None
    res_off = dres = None
    res_cs = 0
    if res_mode == "identity":
        res_off, res_cs = out_off.copy(), cout_pad
        dres = rng.normal(0, 1, npix * res_cs).astype(np.float32)
    elif res_mode == "up2":                              # nearest-upsampled residual (FPN): up to four output pixels share a pixel
        rw = (ww + 1) // 2
        res_off, res_cs = ((ys // 2 + 1) * (rw + 2) + xs // 2 + 1).astype(np.int32), cout_pad
        dres = rng.normal(0, 1, ((hh + 1) // 2 + 2) * (rw + 2) * res_cs).astype(np.float32)
    dzp = np.full(n, SENTINEL, np.float32) if want_dzp else None
    dzt = np.full((cout_pad, kpad), SENTINEL, np.float32) if want_dzt else None
    got = stage_act_backward(dout, out_off, cout, cout_pad, cs, kpad, out_act=out_act, dout_relu=dout_relu, scale=scale,
                             res_off=res_off, res_cstride=res_cs, dres=dres, dzp=dzp, dzt=dzt, precision=precision)
    ref = R.act_backward_reference(dout, out_off, cout, cout_pad, cs, kpad, out_act=out_act, dout_relu=dout_relu, scale=scale,
                                   res_off=res_off, res_cstride=res_cs, dres=dres, dzp=dzp, f32=f32)
    form = R.act_backward_form(cout, cout_pad, cs, kpad, want_dzt, dres is not None, f32)
    what = (form, m, cout, cout_pad, kpad, stored, scale, res_mode, relu)
    assert got["wrote_transpose"] == (form == "tile"), what
    assert np.array_equal(R.bits32(got["dz"]), R.bits32(ref["dz"])), what
    assert not got["dz"][:, cout:].any(), what
    if stored and m * cout >= 64:
        assert (ref["dz"] == 0).any() and (ref["dz"] != 0).any(), what              # (the case exercises both sides of the mask)
    if want_dzp:
        assert np.array_equal(R.bits32(got["dzp"]), R.bits32(ref["dzp"])), what     # interior = dZ, everything else the sentinel
        border = np.ones(npix, bool)
        border[out_off] = False
        assert np.all(got["dzp"].reshape(npix, cs)[border] == SENTINEL), what
    if want_dzt:
        assert np.array_equal(R.bits32(got["dzt"]), R.bits32(ref["dzt"])), what
        assert not got["dzt"][:, m:].any(), what                                    # the weight-gradient GEMM reads these columns
    if dres is not None:
        err = np.abs(got["dres"].astype(np.float64) - ref["dres"])
        assert np.all(err <= 2.0 ** -22 * ref["dres_abs"]), (what, float((err / np.maximum(ref["dres_abs"], 1e-300)).max()))
        quiet = ref["dres_abs"] == np.abs(dres.astype(np.float64))                  # nothing (or only zeros) arrives: exactly the prefill
        assert np.array_equal(got["dres"][quiet], dres[quiet]), what
        _run_act.worst = max(getattr(_run_act, "worst", 0.0), float((err / np.maximum(ref["dres_abs"], 1e-300)).max()))
    return form


def _variants():
    """(stored output, keep scale, residual, dout_relu)"""
    out = [(False, 1.0, res, False) for res in (None, "identity", "up2")]
    for scale in (1.0, 1.0 / 0.7):
        for res in (None, "identity", "up2"):
            for relu in (False, True):
                out.append((True, scale, res, relu))
    return out


@pytest.mark.parametrize("cout,cout_pad", [(64, 64), (72, 128), (8, 64), (256, 256)])
@pytest.mark.parametrize("m,kpad", [(1, 64), (63, 64), (64, 64), (65, 128), (200, 256), (200, 512)])
def test_act_backward_tile_form(m, kpad, cout, cout_pad):
    """act_backward_tile_kernel (+ relu_merge_kernel<uint16_t>): dZ, dZp and dZ^T of one launch."""
    _run_act.worst = 0.0
    for i, (stored, scale, res, relu) in enumerate(_variants()):
        assert _run_act(m, cout, cout_pad, kpad, stored, scale, res, relu, True, True, "bf16", 1000 * m + cout + i) == "tile"
    print("act backward tile M=%d Kpad=%d cout=%d/%d: wrote_transpose=1, dZ / dZp / dZ^T bit-identical, worst dres error %.2e of "
          "sum|terms| (bound 2^-22 = %.2e)" % (m, kpad, cout, cout_pad, _run_act.worst, 2.0 ** -22))


@pytest.mark.parametrize("cout,cout_pad", [(72, 72), (64, 64)])
@pytest.mark.parametrize("m", [1, 28, 29, 57])
def test_act_backward_vector_form(m, cout, cout_pad):
    """act_backward_gather_vec_kernel: no dZ^T requested, no residual (28 / 29 rows of nine 8-channel groups bracket a 256-thread block)."""
    for i, (stored, scale, res, relu) in enumerate(_variants()):
        if res is None:
            assert _run_act(m, cout, cout_pad, 64, stored, scale, None, relu, True, False, "bf16", 77 * m + cout + i) == "vector"
    print("act backward vector M=%d cout=%d/%d: wrote_transpose=0, dZ / dZp bit-identical" % (m, cout, cout_pad))


@pytest.mark.parametrize("m", [1, 65, 200])
def test_act_backward_element_form(m):
    """act_backward_gather_kernel<uint16_t>: channel counts off the 8-grid (the heads' fp32 outputs have no stored output), and
    layers with a residual whose cout_pad is no multiple of 64 (the launcher keeps them on this form)."""
    _run_act.worst = 0.0
    kpad = -(-m // 64) * 64
    for cout, cout_pad in ((36, 36), (90, 96)):
        for stored in (False, True):
            for res in (None, "up2"):
                form = _run_act(m, cout, cout_pad, kpad, stored, 1.0 / 0.7 if stored else 1.0, res, stored, stored, True, "bf16",
                                31 * m + cout, plane=stored)
                assert form == "element"
    # cout_pad % 8 == 0 with a residual, dZ^T not requested: the vector form would fit, the launcher's rule keeps the element form
    for res in ("identity", "up2"):
        assert _run_act(m, 72, 72, kpad, True, 1.0 / 0.7, res, False, True, False, "bf16", 5 * m) == "element"
    print("act backward element M=%d: wrote_transpose=0 (dZ^T by launch_gather_transpose), bit-identical, worst dres error %.2e of "
          "sum|terms| (bound %.2e)" % (m, _run_act.worst, 2.0 ** -22))


@pytest.mark.parametrize("m,cout,cout_pad", [(65, 64, 64), (29, 90, 96)])
def test_act_backward_fp32_mode(m, cout, cout_pad):
    """The fp32 handle's form (act_backward_gather_kernel<float>, gather_transpose_kernel<float>) through the same entry."""
    _run_act.worst = 0.0
    for res, relu in ((None, False), ("up2", True)):
        assert _run_act(m, cout, cout_pad, 128, True, 1.0 / 0.7, res, relu, True, True, "fp32", m + cout) == "element"
    print("act backward fp32 M=%d cout=%d/%d: bit-identical, worst dres error %.2e of sum|terms|" % (m, cout, cout_pad, _run_act.worst))


# ------------------------------------------------------------------------------------------------ input gradient
_dgrad_cache = {}


def _dgrad_problem(route, g, b, h, w, cin, cout, k, stride):
    """Operands, float64 reference and prefill of one case: computed once, shared by the ksplit variants, never modified."""
    key = (route, g, b, h, w, cin, cout, k, stride)
    if key not in _dgrad_cache:
        rng = np.random.default_rng(sum(key[1:]) + len(route))
        oh, ow = -(-h // stride), -(-w // stride)
        dz = rng.normal(0, 1, (g, b, oh, ow, cout)).astype(np.float32)
        wt = (rng.normal(0, 1, (g, k, k, cin, cout)) * np.sqrt(2.0 / (k * k * cin))).astype(np.float32)
        ref = np.stack([R.dgrad_reference(R.bf16_round(dz[i]), R.bf16_round(wt[i]), (h, w), stride, "same") for i in range(g)])
        prefill = rng.normal(0, _rms(ref), (g, b, h + 2, w + 2, cin)).astype(np.float32)
        for a in (dz, wt, ref, prefill):
            a.setflags(write=False)
        _dgrad_cache[key] = (dz, wt, ref, prefill)
    return _dgrad_cache[key]


def _run_dgrad(route, g, b, h, w, cin, cout, k, stride, ksplit):
    from bayes_od_rc_amd.engine import stage_conv_dgrad_route
    dz, wt, ref, prefill = _dgrad_problem(route, g, b, h, w, cin, cout, k, stride)
    sq = (lambda a: a[0]) if g == 1 else (lambda a: a)
    got, used, big = stage_conv_dgrad_route(sq(dz), sq(wt), (h, w), sq(prefill), route, stride=stride, ksplit=ksplit)
    got = got.reshape(prefill.shape)
    inner = (slice(None), slice(None), slice(1, -1), slice(1, -1))
    delta = got[inner].astype(np.float64) - prefill[inner].astype(np.float64)
    err = rel_err(delta, ref, floor=_rms(ref))
    print("dgrad %s %s groups=%d ksplit=%d (used %d, %s tile): worst error %.2e of the rms (bound 1e-3)"
          % (route, (b, h, w, cin, cout, k, stride), g, ksplit, used, "256x256" if big else "128-row", err))
    assert err < 1e-3
    dead = R.untouched_input_pixels((h, w), (k, k), stride)
    assert np.array_equal(got[inner][:, :, dead], prefill[inner][:, :, dead])           # no window reaches them: the prefill, exactly
    if route != "col2im":                                                               # (col2im adds the out-of-image taps to the border, as the step does)
        edge = np.ones((h + 2, w + 2), bool)
        edge[1:-1, 1:-1] = False
        assert np.array_equal(got[:, :, edge], prefill[:, :, edge])
    if ksplit > 0:
        assert used == ksplit
    return got, used, big, _rms(ref)


def _splits_agree(route, case, splits):
    """Forced split-K against ksplit = 1: the same products, another fp32 summation order."""
    base, _, _, rms = _run_dgrad(route, *case, 1)
    for s in splits:
        got, _, _, _ = _run_dgrad(route, *case, s)
        gap = float(np.abs(got.astype(np.float64) - base.astype(np.float64)).max()) / rms
        print("dgrad %s %s: ksplit=%d against ksplit=1: %.2e of the rms (bound 1e-5)" % (route, case, s, gap))
        assert gap < 1e-5


@pytest.mark.parametrize("g,b,h,w,cin,cout", [(1, 1, 1, 1, 256, 256), (1, 2, 2, 2, 256, 256), (1, 1, 9, 13, 64, 64),
                                               (1, 1, 9, 13, 128, 256), (3, 1, 9, 13, 256, 256)])
def test_dgrad_flip_route(g, b, h, w, cin, cout):
    """3x3, stride 1, SAME: convolution of the dZ plane with w_flip, accumulated into the gradient plane (ksplit 0: the step's rule)."""
    _run_dgrad("flip", g, b, h, w, cin, cout, 3, 1, 0)


def test_dgrad_flip_route_split_k():
    """(2, 16, 16, 256 -> 256): the step's own rule splits four ways (8 tiles, 4 chunks of 9 taps); forced 1, 2, 4."""
    case = (1, 2, 16, 16, 256, 256, 3, 1)
    _, used, big, _ = _run_dgrad("flip", *case, 0)
    assert used == 4 and not big
    _splits_agree("flip", case, (2, 4))


def test_dgrad_flip_route_three_groups_on_the_big_tile():
    """(2, 64, 64, 256 -> 256) x 3 groups, ksplit 1: 96 tiles of 256 rows, the first shape conv_big_tile_pays sends to the 256x256 tile."""
    _, used, big, _ = _run_dgrad("flip", 3, 2, 64, 64, 256, 256, 3, 1, 1)
    assert used == 1 and big


@pytest.mark.parametrize("b,h,w,cin,cout,stride", [(2, 12, 12, 64, 256, 1), (1, 15, 17, 256, 128, 2)])
def test_dgrad_rows_route(b, h, w, cin, cout, stride):
    """1x1: GEMM through the table of make_dgrad_rows_kernel straight into the plane; under stride 2 the odd pixels are never written."""
    _run_dgrad("rows", 1, b, h, w, cin, cout, 1, stride, 0)


def test_dgrad_rows_route_long_reduction():
    """Stage 5, (1, 4, 4, 2048 -> 512): ksplit 0 (the rule: 2) and 8."""
    case = (1, 1, 4, 4, 2048, 512, 1, 1)
    _, used, _, _ = _run_dgrad("rows", *case, 0)
    assert used == 2
    _splits_agree("rows", case, (8,))


@pytest.mark.parametrize("b,h,w", [(1, 16, 16), (1, 7, 5)])
def test_dgrad_col2im_route(b, h, w):
    """3x3, stride 2, SAME (pad 0/1 and 1/1), 128 -> 256: dXcol GEMM, then col2im_kernel's atomics into the plane."""
    case = (1, b, h, w, 128, 256, 3, 2)
    _run_dgrad("col2im", *case, 0)
    _splits_agree("col2im", case, (2, 4))


# ------------------------------------------------------------------------------------------------ stem pool backward
def _stem_with_ties(rng, b, ih, iw):
    """Post-ReLU stem values on a coarse bf16 grid (equal maxima inside a window and across windows are the rule, not the
    exception), plus channels with a maximum on each border, an all-zero channel and a constant one."""
    v = (rng.integers(0, 5, (b, ih, iw, 64)) * 0.5).astype(np.float32)
    v[:, 0, :, 0] = 3.0
    v[:, -1, :, 1] = 3.0
    v[:, :, 0, 2] = 3.0
    v[:, :, -1, 3] = 3.0
    v[..., 4] = 0.0
    v[..., 5] = 1.25
    v[..., 6] = (rng.uniform(size=(b, ih, iw)) < 0.2) * 2.0              # mostly all-zero windows
    v[..., 8:16] = rng.normal(0, 1, (b, ih, iw, 8)).clip(min=0)         # generic values
    return v


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("ih,iw", [(1, 1), (2, 3), (5, 4), (8, 8), (7, 9)])
def test_stem_pool_backward(ih, iw, precision):
    from bayes_od_rc_amd.engine import stage_stem_pool_backward
    rng = np.random.default_rng(100 * ih + iw)
    b = 2
    oh, ow = R.stem_pool_geometry(ih, iw)
    stem = _stem_with_ties(rng, b, ih, iw)
    dpool = rng.normal(0, 1, (b, oh + 2, ow + 2, 64)).astype(np.float32)        # (the border holds values too: it is never read)
    got = stage_stem_pool_backward(stem, dpool, precision=precision)
    ref = R.stem_pool_backward_reference(stem, dpool, f32=precision == "fp32")
    assert (ref != 0).any() and not ref[..., 4].any()
    assert np.array_equal(R.bits32(got), R.bits32(ref)), int((R.bits32(got) != R.bits32(ref)).sum())


# ------------------------------------------------------------------------------------------------ fold + pack
def _fold_layers():
    rng = np.random.default_rng(5)
    spec = [(9, 256, 256, 256, True, True), (1, 64, 256, 256, True, False), (1, 256, 72, 128, False, True), (9, 64, 64, 64, True, True),
            (49, 3, 64, 64, True, True)]                 # taps, cin, cout, cout_pad, batch-norm, bias
    layers = []
    for taps, cin, cout, cp, bn, bias in spec:
        layer = {"kernel": (rng.normal(0, 1, (taps, cin, cout)) * np.sqrt(2.0 / (taps * cin))).astype(np.float32), "cout_pad": cp,
                 "fwd32": cin == 3}               # (the fp32 packing is the stem's; asking for it selects the element-wise branch)
        if bias:
            layer["bias"] = rng.normal(0, 0.5, cout).astype(np.float32)
        if bn:
            layer["gamma"] = (rng.uniform(0.5, 1.5, cout) * rng.choice([-1.0, 1.0], cout, p=[0.1, 0.9])).astype(np.float32)
            layer["beta"] = rng.normal(0, 0.5, cout).astype(np.float32)
            layer["mean"] = rng.normal(0, 0.5, cout).astype(np.float32)
            layer["var"] = rng.uniform(0.05, 2.0, cout).astype(np.float32)
        layers.append(layer)
    return layers


def test_fold_pack_all_layers_in_one_launch():
    """fold_pack_all_kernel: blockIdx.y over five layers, the grid-stride over the 144 tiles of the largest one (128 blocks), the
    64x64-tile branch (first four layers) and the element-wise branch (the 7x7, 3 -> 64 stem)."""
    from bayes_od_rc_amd.engine import stage_fold_pack
    layers = _fold_layers()
    got = stage_fold_pack(layers)
    flips = 0
    for i, (layer, g) in enumerate(zip(layers, got)):
        ref = R.fold_pack_reference(layer["kernel"], layer["cout_pad"], **{k: layer.get(k) for k in ("bias", "gamma", "beta", "mean", "var")})
        taps, cin, cout = layer["kernel"].shape
        full64 = np.zeros((taps, cin, layer["cout_pad"]))
        full64[:, :, :cout] = ref["v64"]
        exact = {"w_fwd": full64.transpose(2, 0, 1), "w_bwd": full64.reshape(taps * cin, -1), "w_flip": full64[::-1].transpose(1, 0, 2)}
        for name in ("w_fwd", "w_bwd", "w_flip"):
            assert g[name].shape == ref[name].shape
            bad = g[name] != ref[name]
            if bad.any():
                # single bf16-ulp flips are tolerated only where the exact product sits on a rounding tie (2^-20 relative)
                a, b, v = g[name][bad].astype(np.int64), ref[name][bad].astype(np.int64), exact[name][bad]
                assert np.all(np.abs(a - b) == 1), (i, name, int(bad.sum()))
                mid = (R.bf16_widen(g[name][bad]).astype(np.float64) + R.bf16_widen(ref[name][bad]).astype(np.float64)) / 2
                assert np.all(np.abs(v - mid) <= 2.0 ** -20 * np.abs(v)), (i, name, int(bad.sum()))
                flips += int(bad.sum())
            assert not g[name].reshape(ref[name].shape)[..., cout:].any() if name != "w_fwd" else not g[name][cout:].any(), (i, name)
        assert (g["w_fwd32"] is not None) == (cin == 3)
        if g["w_fwd32"] is not None:
            assert np.array_equal(R.bits32(g["w_fwd32"]), R.bits32(ref["w_fwd32"])), i
        err = np.abs(g["b_fwd"].astype(np.float64) - ref["b64"])
        assert np.all(err <= 4 * 2.0 ** -24 * ref["b_scale"]), (i, float(err.max()))
        assert not g["b_fwd"][cout:].any(), i
        print("fold pack layer %d (%d taps, %d -> %d/%d): worst folded-bias error %.2e of its scale (bound %.2e)"
              % (i, taps, cin, cout, layer["cout_pad"], float((err / np.maximum(ref["b_scale"], 1e-300)).max()), 4 * 2.0 ** -24))
    print("fold pack: %d single-ulp flips on rounding ties (0 = the three packings are bit-identical)" % flips)

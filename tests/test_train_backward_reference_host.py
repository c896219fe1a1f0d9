"""CPU: the restatements of tests/train_backward_reference.py against float64 autograd on tie-free inputs (so that a restatement
cannot be wrong on its own), and the host-side argument checks of the four stage entry points they are compared with on the GPU
(bod_stage_act_backward, bod_stage_conv_dgrad, bod_stage_stem_pool_backward, bod_stage_fold_pack): a bad offset is refused before
anything is launched, with or without a device."""
import os

import numpy as np
import pytest

import train_backward_reference as R
from conftest import ROOT


def test_bf16_rounding_is_round_to_nearest_even():
    import torch
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.normal(0, 1, 4096), rng.normal(0, 1e-39, 64), [0.0, -0.0, 1e-42, -1e-42, 1e-39, 3.0e38],
                        # exact ties: odd and even bf16 neighbours
                        np.array([0x3F808000, 0x3F818000, 0xBF808000, 0x00008000, 0x00018000], np.uint32).view(np.float32)]).astype(np.float32)
    want = torch.tensor(x).to(torch.bfloat16).to(torch.float32).numpy()
    got = R.bf16_round(x)
    assert np.array_equal(R.bits32(got), R.bits32(want))
    assert np.array_equal(R.bf16_widen(R.bf16_bits(got)), got)
    assert R.bf16_bits(np.float32(1e-42)) == 0 and R.bf16_bits(np.float32(1e-39)) != 0


def test_act_backward_restatement_matches_autograd():
    import torch
    rng = np.random.default_rng(1)
    m, cout, cout_pad, scale = 40, 24, 32, 1 / 0.7
    z = torch.tensor(rng.normal(0, 1, (m, cout)), dtype=torch.float64, requires_grad=True)
    res = torch.tensor(rng.normal(0, 1, (m // 4, cout)), dtype=torch.float64, requires_grad=True)
    res_off = np.arange(m) // 4                                   # four output pixels share a residual pixel
    keep = torch.tensor(rng.uniform(size=(m, cout)) > 0.3, dtype=torch.float64)
    out = torch.relu(z + res[torch.tensor(res_off)]) * keep * scale
    dout = rng.normal(0, 1, (m, cout)).astype(np.float32)
    (out * torch.tensor(dout, dtype=torch.float64)).sum().backward()
    # rows of the output buffer in reverse order on a wider pixel stride
    out_off = np.arange(m)[::-1].copy() + 3
    cs = cout_pad + 8
    buf = lambda a: _scatter(a, out_off, cs, m + 5)
    dres0 = rng.normal(0, 1, (m // 4) * cout)
    ref = R.act_backward_reference(buf(dout), out_off, cout, cout_pad, cs, 64, out_act=buf(out.detach().numpy()), scale=scale,
                                   res_off=res_off, res_cstride=cout, dres=dres0, dzp=np.full((m + 5) * cs, -65536.0), f32=True)
    assert np.allclose(ref["dz"][:, :cout], z.grad.numpy(), rtol=1e-6, atol=1e-7)
    assert not ref["dz"][:, cout:].any() and not ref["dzt"][:, m:].any() and np.array_equal(ref["dzt"][:, :m], ref["dz"].T)
    assert np.allclose(ref["dres"] - dres0, res.grad.numpy().reshape(-1), rtol=1e-6, atol=1e-6)
    assert np.all(ref["dres_abs"] >= np.abs(ref["dres"]) - 1e-12)
    dzp = ref["dzp"].reshape(m + 5, cs)
    assert np.array_equal(dzp[out_off, :cout], ref["dz"][:, :cout])
    untouched = np.ones((m + 5, cs), bool)
    untouched[out_off, :cout] = False
    assert np.all(dzp[untouched] == -65536.0)
    # the bf16 form is the fp32 one rounded once
    ref16 = R.act_backward_reference(buf(dout), out_off, cout, cout_pad, cs, 64, out_act=buf(out.detach().numpy()), scale=scale)
    assert np.array_equal(R.bits32(ref16["dz"]), R.bits32(R.bf16_round(ref["dz"])))


def _scatter(rows, out_off, cstride, npix):
    a = np.zeros((npix, cstride), np.float32)
    a[out_off, :rows.shape[1]] = rows
    return a.reshape(-1)


def test_relu_merge_restatement_matches_autograd():
    import torch
    rng = np.random.default_rng(2)
    m, c = 17, 8
    y = torch.tensor(rng.normal(0, 1, (m, c)), dtype=torch.float64, requires_grad=True)       # no activation of its own (P6)
    d1, d2 = rng.normal(0, 1, (m, c)).astype(np.float32), rng.normal(0, 1, (m, c)).astype(np.float32)
    ((y * torch.tensor(d1, dtype=torch.float64)).sum() + (torch.relu(y) * torch.tensor(d2, dtype=torch.float64)).sum()).backward()
    ref = R.act_backward_reference(d1.reshape(-1), np.arange(m), c, c, c, 64, out_act=y.detach().numpy().reshape(-1),
                                   dout_relu=d2.reshape(-1), f32=True)
    assert np.allclose(ref["dz"], y.grad.numpy(), rtol=1e-6, atol=1e-7)


def test_act_backward_form_rule():
    f = R.act_backward_form
    assert f(64, 64, 64, 64, True, True, False) == "tile" and f(72, 128, 128, 128, True, False, False) == "tile"
    assert f(64, 64, 64, 64, False, False, False) == "vector" and f(72, 72, 72, 64, True, False, False) == "vector"
    assert f(72, 72, 72, 64, True, True, False) == "element" and f(36, 36, 36, 64, True, False, False) == "element"
    assert f(90, 96, 96, 64, True, False, False) == "element" and f(64, 64, 64, 64, True, False, True) == "element"


@pytest.mark.parametrize("b,h,w,cin,cout,k,stride", [(2, 5, 6, 8, 16, 3, 1), (1, 7, 5, 8, 4, 3, 2), (1, 16, 16, 4, 8, 3, 2),
                                                      (1, 15, 17, 8, 4, 1, 2), (2, 4, 4, 16, 8, 1, 1)])
def test_dgrad_restatement_matches_autograd(b, h, w, cin, cout, k, stride):
    from test_gpu_train_blocks import _torch_grads
    rng = np.random.default_rng(h * w + k)
    wt = rng.normal(0, 1, (k, k, cin, cout))
    oh, ow = -(-h // stride), -(-w // stride)
    dz = rng.normal(0, 1, (b, oh, ow, cout))
    want, _, _ = _torch_grads(np.zeros((b, h, w, cin)), wt, dz, stride, "same")
    got = R.dgrad_reference(dz, wt, (h, w), stride, "same")
    assert got.shape == want.shape and np.allclose(got, want, rtol=1e-12, atol=1e-12)
    dead = R.untouched_input_pixels((h, w), (k, k), stride)
    assert not got[:, dead].any() and np.all(np.abs(got[:, ~dead]).sum(axis=(0, 2)) > 0)
    assert dead.any() == (k == 1 and stride == 2)


@pytest.mark.parametrize("ih,iw", [(1, 1), (2, 3), (5, 4), (8, 8), (7, 9)])
def test_stem_pool_restatement_matches_autograd(ih, iw):
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(ih * 16 + iw)
    b, c = 2, 64
    assert R.stem_pool_geometry(ih, iw) == ((ih - 1) // 2 + 1, (iw + 1) // 2 + 1)
    oh, ow = R.stem_pool_geometry(ih, iw)
    stem = rng.permutation(b * ih * iw * c).reshape(b, ih, iw, c).astype(np.float32) + 1.0        # positive, tie-free
    x = torch.tensor(stem, dtype=torch.float64).permute(0, 3, 1, 2).requires_grad_(True)
    y = F.max_pool2d(F.pad(x, (2, 2, 1, 1)), 3, stride=2)                                         # ZeroPadding2D((1, 2)), VALID
    assert tuple(y.shape) == (b, c, oh, ow)
    dp = rng.normal(0, 1, (b, oh, ow, c)).astype(np.float32)
    y.backward(torch.tensor(dp, dtype=torch.float64).permute(0, 3, 1, 2))
    plane = np.full((b, oh + 2, ow + 2, c), 1e6, np.float32)           # the border is never read
    plane[:, 1:-1, 1:-1] = dp
    got = R.stem_pool_backward_reference(stem, plane, f32=True)
    assert np.allclose(got, x.grad.permute(0, 2, 3, 1).numpy(), rtol=1e-6, atol=1e-6)
    # ReLU mask: a window whose maximum is zero passes nothing
    assert not R.stem_pool_backward_reference(np.zeros_like(stem), plane, f32=True).any()


def test_stem_pool_restatement_gives_ties_to_the_first_maximum():
    stem = np.zeros((1, 3, 3, 1), np.float32)
    stem[0, 0, 1, 0] = stem[0, 1, 0, 0] = stem[0, 1, 1, 0] = 2.0          # window (0, 1) covers rows -1..1, columns 0..2
    plane = np.zeros((1, 4, 5, 1), np.float32)                           # oh, ow = 2, 3
    plane[0, 1, 2, 0] = 5.0
    got = R.stem_pool_backward_reference(stem, plane, f32=True)
    assert got[0, 0, 1, 0] == 5.0 and got.sum() == 5.0


def test_fold_pack_restatement():
    rng = np.random.default_rng(3)
    taps, cin, cout, cp = 9, 5, 6, 8
    k = rng.normal(0, 1, (taps, cin, cout)).astype(np.float32)
    bn = {n: rng.uniform(0.5, 1.5, cout).astype(np.float32) for n in ("gamma", "beta", "mean", "var")}
    bias = rng.normal(0, 1, cout).astype(np.float32)
    ref = R.fold_pack_reference(k, cp, bias=bias, **bn)
    s = bn["gamma"].astype(np.float64) / np.sqrt(bn["var"].astype(np.float64) + 1e-3)
    for t in range(taps):
        for ci in range(cin):
            for co in range(cp):
                v = ref["w_fwd"][co, t, ci]
                assert v == ref["w_bwd"][t * cin + ci, co] == ref["w_flip"][ci, taps - 1 - t, co]
                if co >= cout:
                    assert v == 0
                else:
                    exact = float(k[t, ci, co]) * s[co]
                    assert abs(float(R.bf16_widen(v)) - exact) <= abs(exact) * 2.0 ** -8          # (half a bf16 ulp is at most 2^-9 relative)
                    assert abs(ref["v64"][t, ci, co] - exact) <= abs(exact) * 1e-7
    assert np.allclose(ref["b64"][:cout], (bias - bn["mean"].astype(np.float64)) * s + bn["beta"], rtol=1e-6) and not ref["b64"][cout:].any()
    plain = R.fold_pack_reference(k, cp)
    assert np.array_equal(plain["w_bwd"][:, :cout].reshape(taps, cin, cout), R.bf16_bits(k).reshape(taps, cin, cout)) and not plain["b64"].any()


# ------------------------------------------------------------------------------------------------ host-side argument checks
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "bayes-od-rc_amd", "lib", "libbayesod_hip.so")):
        g.build()
    from bayes_od_rc_amd import _lib
    return _lib.load()


def _runs_or_fails_loudly(fn):
    """A valid call: runs on a GPU, and without one fails with the library's no-fallback message (tests/test_abi.py)."""
    import torch
    if torch.cuda.is_available():
        fn()
    else:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()


def test_act_backward_entry_refuses_bad_arguments(lib):
    from bayes_od_rc_amd.engine import stage_act_backward
    m, c = 4, 8
    dout = np.zeros(m * c, np.float32)
    off = np.arange(m, dtype=np.int32)
    ok = dict(dout=dout, out_off=off, cout=c, cout_pad=c, out_cstride=c, kpad=64)
    _runs_or_fails_loudly(lambda: stage_act_backward(**ok))
    bad = [dict(cout=16),                                                   # cout > cout_pad
           dict(kpad=m - 1),                                                # Kpad < M
           dict(out_off=np.array([0, 1, 2, m], np.int32)),                  # an offset past the buffer
           dict(out_off=np.array([0, -1, 2, 3], np.int32)),
           dict(out_cstride=c - 1),
           dict(dout_relu=dout),                                            # needs the stored output
           dict(dres=np.zeros(m * c, np.float32), res_cstride=c),           # dres without res_off
           dict(dres=np.zeros(m * c, np.float32), res_cstride=c, res_off=np.array([0, 1, 2, m], np.int32)),
           dict(dres=np.zeros(m * c, np.float32), res_cstride=c - 1, res_off=off),
           dict(precision="bf16x3")]
    for change in bad:
        with pytest.raises(ValueError, match="bod_stage_act_backward"):
            stage_act_backward(**dict(ok, **change))
    with pytest.raises(ValueError):
        stage_act_backward(**dict(ok, dzt=np.zeros(5, np.float32)))


def test_conv_dgrad_entry_refuses_bad_arguments(lib):
    from bayes_od_rc_amd.engine import stage_conv_dgrad_route
    z = lambda *s: np.zeros(s, np.float32)
    _runs_or_fails_loudly(lambda: stage_conv_dgrad_route(z(1, 4, 4, 64), z(3, 3, 64, 64), (4, 4), z(1, 6, 6, 64), "flip"))
    bad = [(z(1, 4, 4, 64), z(1, 1, 64, 64), (4, 4), z(1, 6, 6, 64), "flip", {}),                 # the flip route is 3x3
           (z(1, 2, 2, 64), z(3, 3, 64, 64), (4, 4), z(1, 6, 6, 64), "flip", {"stride": 2}),      # ... and stride 1
           (z(1, 4, 4, 64), z(3, 3, 64, 64), (4, 4), z(1, 6, 6, 64), "rows", {}),                 # the row-table route is 1x1
           (z(1, 4, 4, 64), z(3, 3, 32, 64), (4, 4), z(1, 6, 6, 32), "col2im", {}),               # Cin not a multiple of 64
           (z(1, 4, 4, 128), z(3, 3, 64, 128), (4, 4), z(1, 6, 6, 64), "flip", {"ksplit": 4}),    # 2 chunks do not split in 4
           (z(1, 4, 4, 64), z(3, 3, 64, 64), (4, 4), z(1, 6, 6, 64), "flip", {"ksplit": -1}),
           (z(2, 1, 4, 4, 64), z(2, 1, 1, 64, 64), (4, 4), z(2, 1, 6, 6, 64), "rows", {}),        # groups on the flip route only
           (z(4, 1, 4, 4, 64), z(4, 3, 3, 64, 64), (4, 4), z(4, 1, 6, 6, 64), "flip", {})]        # at most three groups
    for dz, w, hw, din, route, kw in bad:
        with pytest.raises(ValueError, match="bod_stage_conv_dgrad"):
            stage_conv_dgrad_route(dz, w, hw, din, route, **kw)
    with pytest.raises(ValueError):                                          # a plane without its border
        stage_conv_dgrad_route(z(1, 4, 4, 64), z(3, 3, 64, 64), (4, 4), z(1, 4, 4, 64), "flip")


def test_stem_pool_backward_entry_refuses_bad_arguments(lib):
    from bayes_od_rc_amd.engine import stage_stem_pool_backward
    z = lambda *s: np.zeros(s, np.float32)
    _runs_or_fails_loudly(lambda: stage_stem_pool_backward(z(1, 5, 4, 64), z(1, 5, 5, 64)))           # oh, ow = 3, 3
    for stem, dpool, kw in [(z(1, 5, 4, 64), z(1, 5, 4, 64), {}), (z(1, 5, 4, 64), z(1, 3, 3, 64), {}),
                            (z(1, 5, 4, 64), z(1, 5, 5, 64), {"precision": "f16mx"})]:
        with pytest.raises(ValueError, match="bod_stage_stem_pool_backward"):
            stage_stem_pool_backward(stem, dpool, **kw)
    with pytest.raises(ValueError):
        stage_stem_pool_backward(z(1, 5, 4, 32), z(1, 5, 5, 32))


def test_fold_pack_entry_refuses_bad_arguments(lib):
    from bayes_od_rc_amd.engine import stage_fold_pack
    k = np.zeros((1, 64, 64), np.float32)
    v = np.ones(64, np.float32)
    _runs_or_fails_loudly(lambda: stage_fold_pack([dict(kernel=k, cout_pad=64)]))
    for layers in ([], [dict(kernel=k, cout_pad=32)], [dict(kernel=k, cout_pad=64, gamma=v)],
                   [dict(kernel=k, cout_pad=64, gamma=v, beta=v, mean=v)], [dict(kernel=k, cout_pad=8192)]):
        with pytest.raises(ValueError, match="bod_stage_fold_pack"):
            stage_fold_pack(layers)

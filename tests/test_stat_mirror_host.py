"""Horizontal-flip views of the MC statistics, host side: the ABI of bod_stat_forward_view / bod_stat_merge_view, the mirror map
of a record (distributed.mirror_statistics_np) against statistics computed from mirrored samples in float64, the sign changes of
the covariance parameters against the oracle's aleatoric construction, and the symmetry condition on FPN anchors."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ANCHOR_CFG, ROOT

K = 9


def _levels(hw):
    return [(-(-hw[0] // s), -(-hw[1] // s)) for s in (8, 16, 32, 64, 128)]


def test_view_symbols_in_header_binding_cdef_and_library():
    from bayes_od_rc_amd import _lib, build
    raw = open(os.path.join(ROOT, "include", "bayesod.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(bod_[a-z0-9_]+)\s*\(", header))
    cdef_text = build.cdef_text()
    cdef = set(re.findall(r"\b(bod_[a-z0-9_]+)\s*\(", cdef_text))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("bod_stat_forward_view", "bod_stat_merge_view"):
        assert name in declared and name in cdef and name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
    enum = r"enum\s*\{\s*BOD_VIEW_IDENTITY\s*=\s*0\s*,\s*BOD_VIEW_HFLIP\s*=\s*1\s*\}\s*;"
    assert re.search(enum, header) and re.search(enum, cdef_text)
    assert (_lib.BOD_VIEW_IDENTITY, _lib.BOD_VIEW_HFLIP) == (0, 1)
    assert open(os.path.join(ROOT, "include", "bayesod_cdef.h")).read() == cdef_text
    # one argument more than the plain entry points: the view, an int32 at the end
    for name in ("bod_stat_forward", "bod_stat_merge"):
        plain, view = _lib.SIGNATURES[name], _lib.SIGNATURES[name + "_view"]
        assert view[0] is plain[0] and view[1][:-1] == plain[1] and view[1][-1] is ctypes.c_int32
    from bayes_od_rc_amd.engine import Engine
    assert [Engine._view(v) for v in ("identity", "hflip", 0, 1, 2)] == [0, 1, 0, 1, 2]
    with pytest.raises(ValueError):
        Engine._view("vflip")


def _stats64(x):
    """float64 statistics record [A,16] of samples x [n,A,4]."""
    mean = x.mean(axis=0)
    d = x - mean
    m2 = np.einsum("nai,naj->aij", d, d)
    rec = np.zeros((x.shape[1], 16))
    rec[:, :4] = mean
    k = 4
    for i in range(4):
        for j in range(i + 1):
            rec[:, k] = m2[:, i, j]
            k += 1
    return rec


@pytest.mark.parametrize("hw", [(128, 128), (64, 384)])
def test_mirror_statistics_np_equals_the_statistics_of_mirrored_samples(hw):
    from bayes_od_rc_amd.distributed import mirror_anchor_index, mirror_statistics_np
    levels, image_w = _levels(hw), hw[1]
    perm = mirror_anchor_index(levels, K)
    a_n = sum(h * w for h, w in levels) * K
    assert perm.shape == (a_n,) and np.array_equal(perm[perm], np.arange(a_n))          # the permutation is an involution
    # the partner of a = off + (y * W + x) * K + k, written out for the first level and the last
    h0, w0 = levels[0]
    y, x, k = h0 - 1, 2, 4
    assert perm[(y * w0 + x) * K + k] == (y * w0 + (w0 - 1 - x)) * K + k
    off = a_n - levels[-1][0] * levels[-1][1] * K
    assert perm[off + 3] == off + (levels[-1][1] - 1) * K + 3
    rng = np.random.default_rng(11)
    n = 6
    x = np.concatenate([rng.uniform(0, hw[0], (1, a_n, 1)), rng.uniform(0, hw[1], (1, a_n, 1)), rng.uniform(8, 90, (1, a_n, 2))], axis=2) \
        + rng.normal(0, 1.5, (n, a_n, 4))
    cls = rng.random((n, a_n, 8)).sum(axis=0)
    cov = rng.normal(size=(n, a_n, 10)).sum(axis=0)
    xm = np.empty_like(x)                            # what the mirrored forward's samples mean in the frame as given
    xm[:, perm] = x
    xm[..., 1] = (image_w - 1) - xm[..., 1]
    want = _stats64(xm)
    got = mirror_statistics_np(cls, _stats64(x), cov, levels, K, image_w)
    assert got[1].dtype == np.float64
    assert np.max(np.abs(got[1] - want) / (np.abs(want) + 1.0)) < 1e-12
    assert np.all(got[1][:, 14:] == 0)
    assert np.array_equal(got[0][perm], cls) and np.array_equal(got[2][perm][:, [0, 1, 3, 4, 5, 7, 9]], cov[:, [0, 1, 3, 4, 5, 7, 9]])
    assert np.array_equal(got[2][perm][:, [8, 6, 2]], -cov[:, [8, 6, 2]])
    # twice: the anchors and the signs return bit for bit (the u mean takes two roundings, hence 1e-12 and not equality)
    rec32 = (cls.astype(np.float32), _stats64(x).astype(np.float32), cov.astype(np.float32))
    once = mirror_statistics_np(*rec32, levels, K, image_w)
    twice = mirror_statistics_np(*once, levels, K, image_w)
    assert all(t.dtype == np.float32 for t in twice)
    assert np.array_equal(twice[0], rec32[0]) and np.array_equal(twice[2], rec32[2])
    keep = [c for c in range(16) if c != 1]
    assert np.array_equal(twice[1][:, keep], rec32[1][:, keep])
    assert np.array_equal(once[1][:, 1], np.float32(image_w - 1) - rec32[1][perm][:, 1])          # one fp32 subtraction
    assert np.array_equal(once[1][:, [5, 8, 11]], -rec32[1][perm][:, [5, 8, 11]])
    # without the covariance head the third array stays absent; a batch axis in front is carried along
    b = mirror_statistics_np(np.stack([cls, cls]), np.stack([_stats64(x)] * 2), None, levels, K, image_w)
    assert b[2] is None and np.array_equal(b[1][1], got[1])
    with pytest.raises(ValueError):
        mirror_statistics_np(cls[:-1], _stats64(x)[:-1], None, levels, K, image_w)


@pytest.mark.parametrize("use_full_covar", [True, False])
def test_mirrored_covariance_parameters_give_s_sigma_st(use_full_covar):
    """The oracle's aleatoric construction (fill_triangular, unit diagonal, inverse, L D L^T) on the parameters with the signs of
    indices 8, 6, 2 changed equals S Sigma S^T with S = diag(1,-1,1,1): only u changes sign under a mirror."""
    from bayes_od_rc_amd.distributed import mirror_anchor_index, mirror_statistics_np
    from oracle import bayes_od, network
    rng = np.random.default_rng(12)
    levels = [(3, 5), (2, 3), (1, 1)]
    a_n = sum(h * w for h, w in levels) * 2
    p = rng.normal(0, 0.7, (a_n, 10))
    pm = mirror_statistics_np(np.zeros((a_n, 4)), np.zeros((a_n, 16)), p, levels, 2, 40)[2]
    perm = mirror_anchor_index(levels, 2)
    sigma = bayes_od.aleatoric_covariance(network.fill_triangular_4(p), use_full_covar)
    sigma_m = bayes_od.aleatoric_covariance(network.fill_triangular_4(pm), use_full_covar)
    s = np.diag([1.0, -1.0, 1.0, 1.0])
    want = (s @ sigma @ s.T)[perm]
    assert np.max(np.abs(sigma_m - want) / (np.abs(want) + 1.0)) < 1e-12
    if use_full_covar:
        assert np.abs(sigma - s @ sigma @ s.T).max() > 1e-3          # the signs matter
        for wrong in ((8, 6, 3), (7, 6, 2), (8, 1, 2)):               # any other triple of parameters does not give it
            q = p.copy()
            q[:, list(wrong)] *= -1
            other = bayes_od.aleatoric_covariance(network.fill_triangular_4(q), True)
            assert np.abs(other - s @ sigma @ s.T).max() > 1e-3


def test_anchors_mirror_symmetric_on_fpn_anchors():
    from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
    from bayes_od_rc_amd.distributed import anchors_mirror_symmetric
    gen = FpnAnchorGenerator(ANCHOR_CFG)
    assert gen.anchors_per_location == K
    for hw in ((128, 128), (64, 384), (512, 512), (720, 1280)):
        anchors = gen.generate_all((hw[0], hw[1], 3))
        assert anchors_mirror_symmetric(anchors, _levels(hw), K, hw[1]) == (True, None), hw
    for hw in ((384, 1248), (128, 160)):
        anchors = gen.generate_all((hw[0], hw[1], 3))
        assert anchors_mirror_symmetric(anchors, _levels(hw), K, hw[1]) == (False, 6), hw          # levels 3 .. 5 still fit the frame
    anchors = gen.generate_all((128, 128, 3)).copy()
    anchors[5, 2] = np.nextafter(anchors[5, 2], np.float32(1e9))                                    # one bit in one height
    assert anchors_mirror_symmetric(anchors, _levels((128, 128)), K, 128) == (False, 3)
    with pytest.raises(ValueError):
        anchors_mirror_symmetric(anchors[:-1], _levels((128, 128)), K, 128)


def test_ensemble_pipeline_and_cli_know_the_views():
    import inspect
    from bayes_od_rc_amd import run_inference
    from bayes_od_rc_amd.inference_utils import EnsemblePipeline
    assert inspect.signature(EnsemblePipeline.__init__).parameters["views"].default == ("identity",)
    assert "--tta_flip" in inspect.getsource(run_inference.main)

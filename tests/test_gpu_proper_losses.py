"""GPU: 'regression_nll' (reg_kind 4) and 'regression_energy' (reg_kind 5) through bod_loss_forward_ex / bod_loss_backward_ex
against their float64 twin (bayes_od_rc_amd/proper_losses.py, pinned to torch.autograd by test_proper_losses_host.py), at the
block / frame / mask edges and on planted rows, plus the bit-level properties: dcls untouched, kinds 1-3 untouched, a row's
bits its own, repeatable, keyed by the image id.

Tolerance.  The device is fp32, the twin float64; the deviation comes from fp32 log / sincospi / exp and from sums of at most
M terms and is not derivable, so it is MEASURED on an MI355X over every case of this file, per output, as
|got - want| / (|want| + scale): scale = the sum of the absolute terms the sum is made of (proper_loss_abs_terms_np) for the
forward sums; for the gradients max |g| of the ROW -- a row beyond an exp clip has terms and gradients ten orders of magnitude
above an ordinary row's, so one scale per tensor would hide every other row behind it.  For the same reason every case runs on
a problem without planted rows (the sums then see ordinary rows) as well as with them, and every planted row and several ordinary
ones are also the ONLY positive of a call, where the forward sum is that row's term.  The constants below are 4 x the measured
worst."""
import ctypes as C
import functools

import numpy as np
import pytest

from bayes_od_rc_amd import _lib, proper_losses as pl

import proper_loss_reference as ref

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE1234567
FIRST = 10
W_CLS, W_REG, EPS = 5.0, 1.5, 0.001
# 4 x the worst deviation measured on an MI355X over the cases of this file, per output (s_cmp, s_reg, dbox, dcov).  Measured:
#   kind 4: 4.42e-07 (one positive, ordinary row 3), 3.34e-08 (one positive, row 0), 6.12e-06 (2, 300, 8, no plants),
#           7.86e-06 (3, 171, 8, no plants)
#   kind 5: 2.23e-07 (one positive, row 3), 0 (the sum is an exact 0), 7.16e-06 (3, 171, 8, all of frame 1, no plants),
#           6.60e-06 (2, 300, 8, no plants)
# (the gradients' worst rows are ordinary ones: e = pb - tb is a difference of two decoded boxes of some 1e2 px)
TOL = {4: (4 * 4.42e-07, 4 * 3.34e-08, 4 * 6.12e-06, 4 * 7.86e-06),
       5: (4 * 2.23e-07, 0.0, 4 * 7.16e-06, 4 * 6.60e-06)}
BUG = 1e-4                                          # fp32 over <= 1024 terms cannot deviate by this much: not a tolerance

SHAPES = [(1, 1), (1, 257), (3, 171), (2, 300)]
MASKS = ["edges", "none", "none_in_frame_1", "one", "all_of_frame_1"]


@functools.lru_cache(maxsize=None)
def problem(b, a, c, mask="edges", plant="all"):
    """float32 inputs of one call: random positives (one in five) plus the flat indices 0, 255, 256 and b*a - 1.  plant "all":
    the planted rows of proper_loss_reference.raw_rows() are written onto the first positives; "none": ordinary rows only; an
    integer (mask "one"): the single positive is row ``plant`` of raw_rows().  Cached, never modified."""
    rng = np.random.default_rng(100000 * b + 100 * a + c)
    n = b * a
    raw = ref.raw_rows()
    take = rng.integers(0, ref.N_RANDOM, n)
    box, box_t, cov = (np.array(r[take], np.float32) for r in (raw[0], raw[1], raw[3]))
    anchors = np.concatenate([rng.uniform(20.0, 600.0, (a, 2)), rng.uniform(16.0, 256.0, (a, 2))], axis=1).astype(np.float32)
    pos = rng.random(n) < 0.2
    for i in (0, 255, 256, n - 1):
        if i < n:
            pos[i] = True
    if mask == "none":
        pos[:] = False
    elif mask == "none_in_frame_1":
        pos[a:2 * a] = False
    elif mask == "one":
        pos[:] = False
        pos[a + 3] = True
    elif mask == "all_of_frame_1":
        pos[a:2 * a] = True
    where = np.nonzero(pos)[0]
    if plant == "all":
        for k, i in enumerate(where[:len(ref.EDGE_NAMES)]):     # the planted rows
            box[i], box_t[i], cov[i] = raw[0][ref.N_RANDOM + k], raw[1][ref.N_RANDOM + k], raw[3][ref.N_RANDOM + k]
    elif plant != "none":
        assert mask == "one"
        box[where[0]], box_t[where[0]], cov[where[0]] = raw[0][plant], raw[1][plant], raw[3][plant]
    neg = ~pos & (rng.random(n) < 0.5)
    cls = rng.normal(0.0, 2.0, (n, c)).astype(np.float32)
    cls_t = np.eye(c, dtype=np.float32)[np.where(pos, rng.integers(0, c - 1, n), c - 1)]
    p = {"b": b, "a": a, "c": c, "cls": cls, "cls_t": cls_t, "box": box, "box_t": box_t, "cov": cov, "anchors": anchors,
         "pos": pos.astype(np.uint8), "neg": neg.astype(np.uint8)}
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return p


def _call(p, kind, opts=None, backward=True, ex=True, do_cls=1, w_cls=W_CLS, w_reg=W_REG):
    """(status, out4, dcls, dbox, dcov) of bod_loss_backward[_ex] (forward: the gradients are None)."""
    lib = _lib.load()
    u8 = C.POINTER(C.c_uint8)
    n, c = p["b"] * p["a"], p["c"]
    out = (C.c_double * 4)()
    head = (0, p["b"], p["a"], c, _lib.fptr(p["cls"]), _lib.fptr(p["cls_t"]), _lib.fptr(p["box"]), _lib.fptr(p["box_t"]),
            _lib.fptr(p["cov"]), _lib.fptr(p["anchors"]), p["pos"].ctypes.data_as(u8), p["neg"].ctypes.data_as(u8), do_cls, kind, EPS)
    tail = (C.byref(opts) if opts is not None else None,) if ex else ()
    if not backward:
        st = (lib.bod_loss_forward_ex if ex else lib.bod_loss_forward)(*head, out, *tail)
        return st, np.array(out[:]), None, None, None
    dcls, dbox, dcov = np.full((n, c), np.nan, np.float32), np.full((n, 4), np.nan, np.float32), np.full((n, 10), np.nan, np.float32)
    st = (lib.bod_loss_backward_ex if ex else lib.bod_loss_backward)(*head, w_cls, w_reg, out, _lib.fptr(dcls), _lib.fptr(dbox),
                                                                      _lib.fptr(dcov), *tail)
    return st, np.array(out[:]), dcls, dbox, dcov


@functools.lru_cache(maxsize=None)
def device(key, kind, m=64, first=FIRST, seed=SEED):
    st, out, dcls, dbox, dcov = _call(problem(*key), kind, _lib.loss_options(m, seed, first))
    assert st == _lib.BOD_OK, _lib.load().bod_last_error(None)
    for v in (out, dcls, dbox, dcov):
        v.setflags(write=False)
    return out, dcls, dbox, dcov


@functools.lru_cache(maxsize=None)
def twin(key, kind, m=64, first=FIRST, seed=SEED):
    """What the call must return, float64: (sums (S_cmp, S_reg, n_pos), their scales, dbox [n,4], dcov [n,10])."""
    p = problem(*key)
    idx = np.nonzero(p["pos"])[0]
    frame, an = idx // p["a"], idx % p["a"]
    pb, dpb = pl.decode_rows_np(p["box"][idx], p["anchors"][an])
    tb, _ = pl.decode_rows_np(p["box_t"][idx], p["anchors"][an])
    args = (pb, tb, p["cov"][idx], first + frame, an, kind, m, seed)
    s_cmp, s_reg, d_pb, d_c = pl.proper_loss_rows_np(*args)
    a_cmp, a_reg = pl.proper_loss_abs_terms_np(*args)
    k = W_REG / max(len(idx), 1)
    dbox, dcov = np.zeros((p["b"] * p["a"], 4)), np.zeros((p["b"] * p["a"], 10))
    dbox[idx], dcov[idx] = k * d_pb * dpb, k * d_c
    return (s_cmp.sum(), s_reg.sum(), float(len(idx))), (a_cmp.sum(), a_reg.sum()), dbox, dcov


def deviations(key, kind, m):
    """Per output (s_cmp, s_reg, dbox, dcov) the largest |got - want| / (|want| + scale), the gradients row by row with the
    row's max |g| as scale; everything finite, zeros exact."""
    out, dcls, dbox, dcov = device(key, kind, m)
    (w_cmp, w_reg, n_pos), (a_cmp, a_reg), w_box, w_cov = twin(key, kind, m)
    assert out[3] == n_pos
    assert np.isfinite(out).all() and np.isfinite(dcls).all() and np.isfinite(dbox).all() and np.isfinite(dcov).all()
    rest = problem(*key)["pos"] == 0
    assert not dbox[rest].any() and not dcov[rest].any()                       # rows that are not positive: exact zeros
    devs = []
    for got, want, scale in ((out[1], w_cmp, a_cmp), (out[2], w_reg, a_reg)):
        devs.append(abs(got - want) / (abs(want) + scale) if (abs(want) + scale) > 0 else (0.0 if got == 0.0 else np.inf))
    for got, want in ((dbox, w_box), (dcov, w_cov)):
        scale = np.abs(want).max(axis=1, keepdims=True)
        live = scale[:, 0] > 0
        assert not got[~live].any()                                            # a row whose gradient is an exact 0
        devs.append(float(np.max(np.abs(got[live] - want[live]) / (np.abs(want[live]) + scale[live]))) if live.any() else 0.0)
    return devs


def _check(key, kind, m):
    devs = deviations(key, kind, m)
    print("DEV kind=%d key=%s M=%d  s_cmp %.3e  s_reg %.3e  dbox %.3e  dcov %.3e" % ((kind, key, m) + tuple(devs)))
    for name, d, tol in zip(("s_cmp", "s_reg", "dbox", "dcov"), devs, TOL[kind]):
        assert d < BUG, (name, d)
        assert d <= tol, (name, d, tol)


@pytest.mark.parametrize("kind", [4, 5])
@pytest.mark.parametrize("c", [4, 8])
@pytest.mark.parametrize("b,a", SHAPES)
@pytest.mark.parametrize("plant", ["none", "all"])
def test_sums_and_gradients_match_the_twin_at_the_edges(b, a, c, kind, plant):
    p = problem(b, a, c, "edges", plant)
    assert p["pos"][0] and p["pos"][b * a - 1] and (b * a <= 256 or (p["pos"][255] and p["pos"][256]))
    _check((b, a, c, "edges", plant), kind, 64)


@pytest.mark.parametrize("kind", [4, 5])
@pytest.mark.parametrize("row", [0, 1, 2, 3, 4, 5] + [ref.N_RANDOM + k for k in range(len(ref.EDGE_NAMES))])
def test_a_single_positive_row_matches_the_twin(row, kind):
    """One positive in the call: S_cmp / S_reg ARE that row's terms, so the forward is checked row by row -- six ordinary rows
    and every planted one."""
    key = (3, 171, 8, "one", row)
    _check(key, kind, 64)
    out = device(key, kind, 64)[0]
    assert out[3] == 1.0 and (out[1] != 0.0 or (kind == 4 and row == ref.N_RANDOM))       # (pb == tb: the NLL's s_cmp is 0)


@pytest.mark.parametrize("kind", [4, 5])
@pytest.mark.parametrize("mask", MASKS[1:])
@pytest.mark.parametrize("plant", ["none", "all"])
def test_sums_and_gradients_match_the_twin_for_every_mask(mask, kind, plant):
    _check((3, 171, 8, mask, plant), kind, 64)
    if mask == "none":
        out, _, dbox, dcov = device((3, 171, 8, mask, plant), kind, 64)
        assert out[1] == 0.0 and out[2] == 0.0 and out[3] == 0.0 and not dbox.any() and not dcov.any()


@pytest.mark.parametrize("m", [2, 63, 65, 200])
@pytest.mark.parametrize("b,a,c", [(1, 257, 8), (2, 300, 4)])
@pytest.mark.parametrize("plant", ["none", "all"])
def test_energy_score_at_every_sample_count(b, a, c, m, plant):
    _check((b, a, c, "edges", plant), 5, m)


def test_planted_rows():
    """pb == tb, no off-diagonals, ld = +8 / -8, p beyond both exp clips (no gradient through that coordinate), t beyond it."""
    key = (2, 300, 4, "edges")
    p = problem(*key)
    where = np.nonzero(p["pos"])[0][:len(ref.EDGE_NAMES)]
    names = dict(zip(ref.EDGE_NAMES, where))
    assert (p["box"][names["pb_equals_tb"]] == p["box_t"][names["pb_equals_tb"]]).all()
    for kind in (4, 5):
        _, _, dbox, dcov = device(key, kind, 64)
        for name in ("p_beyond_upper_clip", "p_beyond_lower_clip"):
            i = names[name]
            assert (dbox[i, 2:] == 0.0).all() and (dbox[i, :2] != 0.0).all(), (kind, name)
        assert (dbox[names["t_beyond_clip"]] != 0.0).all()
        assert np.isfinite(dbox[where]).all() and np.isfinite(dcov[where]).all()
    _, _, dbox, dcov = device(key, 4, 64)
    i = names["pb_equals_tb"]                                    # NLL at e = 0: only the 0.5 of the log-determinant's slope is left
    k = np.float32(W_REG) / np.float32(p["pos"].sum())
    assert not dbox[i].any() and not dcov[i, [1, 2, 3, 6, 7, 8]].any() and (dcov[i, [4, 9, 5, 0]] == k * np.float32(0.5)).all()


def test_dcls_is_the_classification_kernels_own():
    for key in [(3, 171, 8, "edges"), (2, 300, 4, "edges")]:
        _, _, dcls3, _, _ = _call(problem(*key), 3, ex=False)
        for kind in (4, 5):
            assert device(key, kind, 64)[1].tobytes() == dcls3.tobytes(), (key, kind)


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_old_kinds_through_the_new_entries_are_bit_equal(kind):
    p = problem(3, 171, 8)
    opts = _lib.loss_options(200, SEED, 77)
    old, new = _call(p, kind, ex=False), _call(p, kind, opts)
    assert old[0] == new[0] == _lib.BOD_OK
    for x, y in zip(old[1:], new[1:]):
        assert x.tobytes() == y.tobytes()
    assert _call(p, kind, backward=False, ex=False)[1].tobytes() == _call(p, kind, opts, backward=False)[1].tobytes() == old[1].tobytes()


def _frames(parts):
    """A problem of the frames ``parts``: (problem, frame index) pairs of equal anchor count, sharing the first one's anchors."""
    keys = ("cls", "cls_t", "box", "box_t", "cov", "pos", "neg")
    a = parts[0][0]["a"]
    q = {k: np.ascontiguousarray(np.concatenate([p[k].reshape((p["b"], a) + p[k].shape[1:])[f].reshape((a,) + p[k].shape[1:])
                                                 for p, f in parts])) for k in keys}
    q.update(b=len(parts), a=a, c=parts[0][0]["c"], anchors=parts[0][0]["anchors"])
    return q


@pytest.mark.parametrize("kind", [4, 5])
def test_a_rows_bits_are_its_own(kind):
    """Frame F (image id 11) as frame 1 of a batch of two and as frame 0 of a batch of three.  One positive in the call: the
    forward sum IS that row's term.  Many positives, the same number in both calls: F's gradient rows."""
    one, empty, many = problem(3, 171, 8, "one", 2), problem(3, 171, 8, "none"), problem(3, 171, 8, "edges")
    a1 = _call(_frames([(empty, 0), (one, 1)]), kind, _lib.loss_options(65, SEED, 10))
    a2 = _call(_frames([(one, 1), (empty, 0), (empty, 2)]), kind, _lib.loss_options(65, SEED, 11))
    assert a1[0] == a2[0] == _lib.BOD_OK and a1[1][3] == a2[1][3] == 1.0
    assert a1[1][1:].tobytes() == a2[1][1:].tobytes() and a1[1][1:3].any()       # (the focal sum is the whole batch's)
    assert a1[3][171:342].tobytes() == a2[3][:171].tobytes() and a1[4][171:342].tobytes() == a2[4][:171].tobytes()
    other = dict(many)
    other["box"] = np.ascontiguousarray(many["box"][::-1])       # another frame 0 with the same mask
    b1 = _call(_frames([(many, 0), (many, 1)]), kind, _lib.loss_options(65, SEED, 10))
    b2 = _call(_frames([(many, 1), (other, 0), (empty, 2)]), kind, _lib.loss_options(65, SEED, 11))
    assert b1[0] == b2[0] == _lib.BOD_OK and b1[1][3] == b2[1][3] > 20
    assert b1[3][171:342].any() and b1[4][171:342].any()
    assert b1[3][171:342].tobytes() == b2[3][:171].tobytes() and b1[4][171:342].tobytes() == b2[4][:171].tobytes()


def test_repeatable_and_keyed_by_the_image_id():
    key = (2, 300, 4, "edges")
    p = problem(*key)
    for kind in (4, 5):
        first = device(key, kind, 64)
        again = _call(p, kind, _lib.loss_options(64, SEED, FIRST))
        for x, y in zip(first, again[1:]):
            assert x.tobytes() == y.tobytes(), kind
        moved = _call(p, kind, _lib.loss_options(64, SEED, FIRST + 1))
        same = all(x.tobytes() == y.tobytes() for x, y in zip(first, moved[1:]))
        assert same == (kind == 4)
        if kind == 5:
            assert moved[1][1] != first[0][1] and moved[3].tobytes() != first[2].tobytes()
            reseeded = _call(p, kind, _lib.loss_options(64, SEED + 1, FIRST))
            assert reseeded[1][1] != first[0][1]
    # the plain entries are the defaults: M = 64, seed 0, first image id 0
    plain, dflt = _call(p, 5, ex=False), _call(p, 5, _lib.loss_options(64, 0, 0))
    null = _call(p, 5, None)
    for x, y, z in zip(plain[1:], dflt[1:], null[1:]):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    assert _call(p, 5, backward=False, ex=False)[1].tobytes() == plain[1].tobytes()


@pytest.mark.parametrize("m", [1, 1025, 0, -3])
def test_sample_counts_outside_the_range_are_refused(m):
    p = problem(1, 257, 8)
    for kind in (5, 3):
        assert _call(p, kind, _lib.loss_options(m, 0, 0))[0] == _lib.BOD_ERR_INVALID_ARG
        assert _call(p, kind, _lib.loss_options(m, 0, 0), backward=False)[0] == _lib.BOD_ERR_INVALID_ARG
    assert b"energy_samples" in _lib.load().bod_last_error(None)


def test_the_covariance_head_is_required():
    p = dict(problem(1, 257, 8))
    p["cov"] = None
    for kind in (4, 5):
        assert _call(p, kind, _lib.loss_options(64, 0, 0), backward=False)[0] == _lib.BOD_ERR_INVALID_ARG

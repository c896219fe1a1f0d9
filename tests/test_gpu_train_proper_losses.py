"""GPU: 'regression_nll' (reg_kind 4) and 'regression_energy' (reg_kind 5) inside the training step and the validation entries
(DESIGN.md 9.10): the step's loss terms and the gradients its backward receives are those of bod_loss_forward_ex /
bod_loss_backward_ex (pinned to the float64 twin by test_gpu_proper_losses.py) on the step's own raw outputs and targets; a
replayed graph draws new normals every step and re-records when the sample count changes; the step descends; the command line
trains from the example yaml; a frame's validation sums do not depend on its batch.

Geometry of tests/test_gpu_train_step.py::_problem (64 x 64, two frames), on the bf16 handle with the step recorded into a
hipGraph and replayed, and on the fp32 verification handle, which never records."""
import os

import numpy as np
import pytest

from bayes_od_rc_amd import _lib

from test_gpu_proper_losses import _call
from test_gpu_train_step import _problem

pytestmark = pytest.mark.gpu

HW, BATCH, SEED = (64, 64), 2, 3
W_CLS, W_REG = 5.0, 1.0                         # Engine.train_step's defaults


@pytest.fixture(scope="module")
def prob():
    return _problem(HW, BATCH)


@pytest.fixture(scope="module")
def graph_env():
    """BOD_TRAIN_GRAPH=1 for the module: a configuration's second step is recorded, later ones are replays."""
    old = os.environ.get("BOD_TRAIN_GRAPH")
    os.environ["BOD_TRAIN_GRAPH"] = "1"
    yield
    if old is None:
        os.environ.pop("BOD_TRAIN_GRAPH", None)
    else:
        os.environ["BOD_TRAIN_GRAPH"] = old


def _engine(prob, **kw):
    from bayes_od_rc_amd.engine import Engine, make_config
    eng = Engine(make_config(HW, batch=BATCH, mc_samples=1, training=True, **kw))
    eng.load_weights(prob[0])
    eng.set_anchors(prob[1])
    return eng


@pytest.fixture(scope="module")
def engines(prob, graph_env):
    made = {"bf16": _engine(prob), "fp32": _engine(prob, precision="fp32")}
    yield made
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def still(prob, graph_env):
    """bf16 handle without dropout: the forward does not depend on the image id, only the energy score's normals do."""
    eng = _engine(prob, dropout_rate=0.0)
    yield eng
    eng.close()


def _step(eng, prob, kind, first, m=None, lr=None):
    _, _, frames, cls_t, box_t, pos, neg = prob
    return eng.train_step(frames, cls_t, box_t, pos, neg, seed=SEED, first_image_id=first, reg_kind=kind, energy_samples=m,
                          apply_update=lr is not None, learning_rate=lr or 0.0)


def _stateless(eng, anchors, kind, first, m, backward=False):
    """bod_loss_forward_ex / bod_loss_backward_ex on the raw outputs and the targets of the handle's last step."""
    cls, box, cov = eng.get_raw()
    cls_t, box_t, pos, neg = eng.train_targets()
    b, a = pos.shape
    p = {"b": b, "a": a, "c": cls.shape[-1], "cls": np.ascontiguousarray(cls.reshape(b * a, -1)), "cls_t": np.ascontiguousarray(cls_t),
         "box": np.ascontiguousarray(box.reshape(b * a, 4)), "box_t": np.ascontiguousarray(box_t),
         "cov": np.ascontiguousarray(cov.reshape(b * a, 10)), "anchors": anchors, "pos": pos.astype(np.uint8), "neg": neg.astype(np.uint8)}
    got = _call(p, kind, _lib.loss_options(m, SEED, first), backward=backward, w_cls=W_CLS, w_reg=W_REG)
    assert got[0] == _lib.BOD_OK
    return got


CASES = [(4, 64), (5, 64), (5, 130)]


@pytest.fixture(scope="module")
def stepped(engines, prob):
    """(out6 dict, bod_loss_backward_ex on the step's raw outputs and targets) of the THIRD step of a configuration -- on the
    bf16 handle a replay of the recorded graph -- computed once per (handle, kind, M)."""
    cache = {}

    def get(handle, kind, m):
        if (handle, kind, m) not in cache:
            eng = engines[handle]
            for first in (20, 22, 24):
                out = _step(eng, prob, kind, first, m)
            _, sums, _, dbox, dcov = _stateless(eng, prob[1], kind, 24, m, backward=True)
            bias = {layer: eng.train_get(layer, "bias", (9 * width,), what="grad").astype(np.float64)
                    for layer, width in (("pyramid_regression", 4), ("pyramid_cov", 10))}
            cache[(handle, kind, m)] = (out, sums, dbox, dcov, bias)
        return cache[(handle, kind, m)]
    return get


@pytest.mark.parametrize("kind,m", CASES)
@pytest.mark.parametrize("handle", ["bf16", "fp32"])
def test_step_loss_terms_are_the_loss_entries(stepped, handle, kind, m):
    """out6's reg_loss / covariance_loss against bod_loss_forward_ex with the step's seed, image ids and M: loss terms to 1e-5,
    the tolerance of the existing step tests."""
    out, sums, _, _, _ = stepped(handle, kind, m)
    n_pos = max(sums[3], 1.0)
    assert sums[3] > 20
    for name, ref in (("reg_loss", sums[1] / n_pos), ("covariance_loss", sums[2] / n_pos)):
        print("%s kind %d M=%d %s: step %.9g entries %.9g" % (handle, kind, m, name, out[name], ref))
        assert abs(out[name] - ref) <= 1e-5 * abs(ref) + 1e-7, (name, out[name], ref)
    assert (out["covariance_loss"] == 0.0) == (kind == 5)


@pytest.mark.parametrize("kind,m", CASES)
@pytest.mark.parametrize("handle", ["bf16", "fp32"])
def test_head_bias_gradients_are_the_loss_entries_column_sums(stepped, handle, kind, m):
    """The gradient of the box and covariance heads' output biases against the sums over frames and positions of
    bod_loss_backward_ex's dbox / dcov columns: 1e-4 max|g| per tensor, the bound of the fp32 step test.

    Measured on an MI355X, worst |d| / max|g| (pyramid_regression / pyramid_cov) for kind 4, kind 5 at M = 64, kind 5 at M = 130:
    fp32 handle 3.8e-8 / 1.7e-8, 6.3e-8 / 4.0e-8, 2.2e-8 / 4.8e-8; bf16 handle 2.5e-8 / 3.0e-8, 3.0e-8 / 2.6e-8, 2.0e-8 / 3.5e-8.
    On the bf16 handle the step writes these two bias gradients as fp32 column sums of dbox / dcov for kinds 4 / 5
    (head_bias_grad_kernel): its weight-gradient GEMM reads dZ from bf16 storage (2^-9 per element) and gave 1.5e-3 to 3.5e-3
    here -- what the existing reg_kind 3, whose gradients are left as they were, still gives in this comparison (3.5e-3 / 2.6e-4)."""
    _, _, dbox, dcov, bias = stepped(handle, kind, m)
    errs = {}
    for layer, g, width in (("pyramid_regression", dbox, 4), ("pyramid_cov", dcov, 10)):
        want = g.astype(np.float64).reshape(BATCH, -1, 9, width).sum(axis=(0, 1)).ravel()
        assert np.abs(want).max() > 0
        errs[layer] = float(np.abs(bias[layer] - want).max() / np.abs(want).max())
        print("%s kind %d M=%d d %s/bias: worst |d| / max|g| = %.2e" % (handle, kind, m, layer, errs[layer]))
    assert max(errs.values()) <= 1e-4, errs


def test_replays_draw_new_normals(still, prob):
    for kind in (4, 5):
        for _ in range(3):
            _step(still, prob, kind, 6)                              # eager, recorded, replayed
        vals = [_step(still, prob, kind, first)["reg_loss"] for first in (0, 2, 4, 0)]
        print("kind %d reg_loss over image ids 0, 2, 4, 0: %s" % (kind, vals))
        assert np.isfinite(vals).all() and vals[3] == vals[0]
        if kind == 4:
            assert vals[0] == vals[1] == vals[2]
        else:
            assert len(set(vals[:3])) == 3


def test_changing_the_sample_count_re_records(still, prob):
    seen = {}
    for m in (64, 65, 64, 1024):
        for _ in range(3):
            out = _step(still, prob, 5, 8, m)
        _, sums, _, _, _ = _stateless(still, prob[1], 5, 8, m)
        ref = sums[1] / max(sums[3], 1.0)
        assert abs(out["reg_loss"] - ref) <= 1e-5 * abs(ref) + 1e-7, (m, out["reg_loss"], ref)
        if m in seen:
            assert out["reg_loss"] == seen[m]
        seen[m] = out["reg_loss"]
    assert len(set(seen.values())) == 3, seen
    for m in (1, 1025):
        with pytest.raises(ValueError):
            still.set_loss_options(m)
    assert _step(still, prob, 5, 8)["reg_loss"] == seen[1024]         # a refused count leaves the handle's as it was


def test_energy_score_descends(prob, graph_env):
    eng = _engine(prob)
    try:
        losses = [_step(eng, prob, 5, 10, 64, lr=1e-3)["reg_loss"] for _ in range(9)]       # the ninth is evaluated after eight updates
    finally:
        eng.close()
    print("reg_loss:", losses)
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses


def test_run_training_cli_with_the_energy_yaml(tmp_path, monkeypatch):
    monkeypatch.setenv("BAYESOD_DATA_DIR", str(tmp_path))
    from bayes_od_rc_amd import run_training
    here = os.path.dirname(os.path.abspath(run_training.__file__))
    yaml_path = os.path.join(here, "configs", "retinanet_bdd_covar_energy.yaml")
    history, ckpt_dir = run_training.main(["--gpu_device", "0", "--yaml_path", yaml_path, "--synthetic", "3", "--image_size", "128", "128",
                                           "--steps", "2"])
    assert len(history) == 2 and np.isfinite(history).all()
    assert os.path.exists(os.path.join(ckpt_dir, "ckpt-2.npz")) and "retinanet_bdd_covar_energy" in ckpt_dir


def test_validation_sums_of_a_frame_do_not_depend_on_its_batch(prob):
    """bod_validate_boxes with reg_kind 5: frame F as frame 1 of two (first image id 5) and as frame 0 of three (first image
    id 6) -- the same image id 6 -- gives the same four sums, bit for bit; another image id gives another energy score."""
    from bayes_od_rc_amd import synthetic
    from bayes_od_rc_amd.engine import Engine, make_config
    from test_gpu_train_from_boxes import _gt_from_anchors
    weights, anchors = prob[0], prob[1]
    frames = synthetic.make_frames(3, HW[0], HW[1], seed=5)
    gt = [_gt_from_anchors(anchors, s) for s in range(3)]
    sums, alone = {}, {}
    for order, first in (((0, 1), 5), ((1, 2, 0), 6), ((2, 0, 1), 6)):
        eng = Engine(make_config(HW, batch=len(order), mc_samples=1))
        try:
            eng.load_weights(weights)
            eng.set_anchors(anchors)
            s, _ = eng.validate_boxes(frames[list(order)], [gt[f][0] for f in order], [gt[f][1] for f in order], 0.5, 0.4, reg_kind=5,
                                      loss_options={"energy_samples": 65, "seed": SEED, "first_image_id": first})
            again = eng.validation_losses_boxes([gt[f][0] for f in order], [gt[f][1] for f in order], 0.5, 0.4, reg_kind=5)
            assert s.tobytes() == again.tobytes()
            # one_image_id (run_validation's setting): every frame is image `first_image_id` itself
            alone[order] = eng.validation_losses_boxes([gt[f][0] for f in order], [gt[f][1] for f in order], 0.5, 0.4, reg_kind=5,
                                                       loss_options={"first_image_id": 6, "one_image_id": True})
        finally:
            eng.close()
        sums[order] = s
    a, b, c = sums[(0, 1)], sums[(1, 2, 0)], sums[(2, 0, 1)]
    assert np.isfinite(a).all() and a[1, 3] > 0 and a[1, 1] > 0 and a[1, 2] == 0.0
    assert a[1].tobytes() == b[0].tobytes()                           # frame 1 with image id 6, in two batches
    assert b[1].tobytes() != c[0].tobytes() and (b[1][[0, 3]] == c[0][[0, 3]]).all()      # frame 2 with image ids 7 and 6
    assert b[1][1] != c[0][1]
    # with one image id for every frame, a frame's sums are its own wherever it sits: frames 0, 1, 2 across the three batches
    x, y, z = alone[(0, 1)], alone[(1, 2, 0)], alone[(2, 0, 1)]
    assert x[0].tobytes() == y[2].tobytes() == z[1].tobytes() and x[1].tobytes() == y[0].tobytes() == z[2].tobytes()
    assert y[1].tobytes() == z[0].tobytes() == c[0].tobytes() and y[0].tobytes() == b[0].tobytes()

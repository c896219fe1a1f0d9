"""GPU: a plain `bench.py` run times only the headline, and --dump-outputs writes what its last timed step computed -- the same
detections a synchronous bod_infer of that step's frames and image ids returns."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.mark.gpu
def test_plain_bench_dumps_the_last_timed_step(tmp_path):
    import bench
    from bayes_od_rc_amd import synthetic
    from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
    hw, batch, steps, warmup = (512, 512), 4, 2, 1
    d = str(tmp_path / "dump")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                          "--batch", str(batch), "--dump-outputs", d], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1, out.stdout[-2000:]
    rec = json.loads(line[0])
    assert rec["steps"] == steps and rec["ms_per_step"] > 0 and rec["value"] > 0 and rec["dtype"] == "bf16"
    assert rec["unit"] == "images/sec" and rec["higher_is_better"] is True
    for k in ("roofline", "cpu_baseline", "parity_mode", "secondary", "value_with_h2d", "telemetry"):
        assert k not in rec, k
    got = {k: np.load(os.path.join(d, k + ".npy")) for k in ("num_detections", "scores", "means", "covs", "counts", "frame_index")}
    assert all(v.dtype == np.float32 for k, v in got.items() if k != "frame_index")
    assert np.array_equal(got["frame_index"], np.arange(batch))

    # the last timed step: frames of seed 0 (rank 0's shard), image ids from (warmup + steps - 1) * batch, Philox seed 0
    weights = synthetic.make_weights(cls_fg_bias=bench.CALIBRATED_FG_BIAS)
    anchors = FpnAnchorGenerator(bench.ANCHOR_CFG).generate_all((hw[0], hw[1], 3))
    eng = bench.make_engine(hw, batch, 10, 0, weights=weights, anchors=anchors)
    try:
        eng.upload_images(synthetic.make_frames(batch, hw[0], hw[1], seed=0))
        eng.infer(None, seed=0, first_image_id=(warmup + steps - 1) * batch)
        want = bench.detections_to_arrays(eng.get_detections_batch())
    finally:
        eng.close()
    assert got["num_detections"].min() > 0
    for k, v in want.items():
        assert np.array_equal(got[k], v), k

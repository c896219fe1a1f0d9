#!/usr/bin/env python3
"""Worker of tests/test_gpu_stat_merge.py::test_stat_sharded_two_ranks_on_one_gpu: every rank (all on GPU 0, gloo) runs its
share of the MC ensemble through distributed.StatShardedEngine and writes its detections and posterior to <dir>/rank<r>.npz
(the test compares the ranks' files for equality); rank 0 also gathers the ranks' raw head outputs and checks the posterior
against the oracle on the union of the samples."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import torch.distributed as dist
from conftest import ANCHOR_CFG, BAYES_CFG, NMS_CFG, compare_posterior
from bayes_od_rc_amd import synthetic, distributed as bd
from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator

out_dir = sys.argv[1]
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
torch.cuda.set_device(0)
hw, batch, n_total, seed, first = (128, 128), 2, 10, 20261018, 3
weights = synthetic.make_weights(cls_fg_bias=-1.0)
anchors = FpnAnchorGenerator(ANCHOR_CFG).generate_all((hw[0], hw[1], 3))
frames = synthetic.make_frames(batch, hw[0], hw[1], seed=31)
sse = bd.StatShardedEngine(hw, weights, anchors, n_total, batch=batch, use_full_covar=True, bayes_od_config=BAYES_CFG, nms_config=NMS_CFG)
dets = sse.infer(frames, seed=seed, first_image_id=first)
eng = sse.engine
assert eng.stat_samples == n_total
out = {}
for b in range(batch):
    for k, v in zip(("scores", "means", "covs", "counts"), dets[b]):
        out["det%d_%s" % (b, k)] = v
    for k, v in eng.get_posterior(b).items():
        out["post%d_%s" % (b, k)] = v
np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
# the union of the samples: every rank's raw head outputs [B,n,A,.] of its own pass, gathered on the host
full = []
for local in eng.get_raw():
    local = torch.from_numpy(local)
    buf = torch.empty((batch, n_total) + tuple(local.shape[2:]), dtype=local.dtype)
    full.append(bd.all_gather_samples(local, buf).numpy())
ok = True
if rank == 0:
    from oracle import bayes_od, network, philox
    for img in range(batch):
        u = philox.categorical_uniforms(seed, first + img, eng.A)
        pred = {"anchors_class_predictions": full[0][img], "anchors_box_predictions": full[1][img],
                "anchors_box_covar_predictions": network.fill_triangular_4(full[2][img])}
        ref = bayes_od.bayes_od_posterior(pred, anchors, u, BAYES_CFG, use_full_covar=True, dtype=np.float64, return_debug=True)
        checked, _ = compare_posterior(eng.get_posterior(img), ref, u, tol=1e-3, min_checked=20)
        print("image %d: %d anchors compared with the oracle" % (img, checked), flush=True)
    print("STAT_SHARD_OK", flush=True)
dist.barrier()
dist.destroy_process_group()
sys.exit(0 if ok else 1)

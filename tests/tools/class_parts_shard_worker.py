#!/usr/bin/env python3
"""Worker of tests/test_gpu_class_parts.py::test_two_ranks_on_one_gpu_gather_wide_rows: every rank (all on GPU 0, gloo) runs its
share of the MC ensemble through distributed.StatShardedEngine on a class_parts handle -- the all-gathered records carry ent_sum
-- and writes its detections with their class parts to <dir>/rank<r>.npz (the test compares the ranks' files for equality).  Every
rank then packs its wide record rows and rank 0 gathers them: each block must arrive as it was sent, and rank 0 checks the class
parts against float64 on the union of the ranks' raw samples."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import torch.distributed as dist
import class_parts_reference as clr
from conftest import ANCHOR_CFG, BAYES_CFG, NMS_CFG
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
sse = bd.StatShardedEngine(hw, weights, anchors, n_total, batch=batch, use_full_covar=True, bayes_od_config=BAYES_CFG, nms_config=NMS_CFG,
                           class_parts=True)
dets = sse.infer(frames, seed=seed, first_image_id=first)
eng = sse.engine
assert eng.stat_samples == n_total and "ent" in sse._local
out = {"ent_sum": eng.get_entropy()}
for b in range(batch):
    assert len(dets[b]) == 5
    for k, v in zip(("scores", "means", "covs", "counts", "class_parts"), dets[b]):
        out["det%d_%s" % (b, k)] = v
    out["post%d_class_parts" % b] = eng.get_posterior_class_parts(b)
np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
# the wide rows: packed on every rank, gathered on rank 0
k, c = eng.K, eng.Ccls
det = eng.get_detections_batch()
rows = eng.get_detection_class_parts_batch()
rec = bd.pack_records(*[torch.from_numpy(det[x]) for x in ("num", "scores", "means", "covs", "counts")], class_parts=torch.from_numpy(rows))
assert rec.shape == (batch, k, bd.record_width(c, class_parts=True))
mine = rec * float(rank + 1)                              # every rank's block is recognisably its own
got = bd.gather_records(mine, dst=0)
# the union of the samples: every rank's raw class logits [B,n,A,C] of its own pass, gathered on the host
local = torch.from_numpy(eng.get_raw()[0])
full = bd.all_gather_samples(local, torch.empty((batch, n_total) + tuple(local.shape[2:]), dtype=local.dtype)).numpy()
if rank == 0:
    assert got.shape == (world, batch, k, rec.shape[2])
    for r in range(world):
        assert torch.equal(got[r], rec * float(r + 1))    # (the ranks' detections are identical: asserted by the test on the files)
    for img, row in enumerate(bd.unpack_records(got[0], c)):
        assert len(row) == 5 and np.array_equal(row[4], dets[img][4]) and np.array_equal(row[2], dets[img][2])
    for img in range(batch):
        idx = eng.get_posterior(img)["anchor_index"]
        want, _ = clr.posterior_rows(*clr.statistics(full[img][:, idx], sample_axis=0), n_total)
        err = np.abs(eng.get_posterior_class_parts(img).astype(np.float64) - want).max()
        print("image %d: %d rows against float64 on the union of the samples: %.2e" % (img, len(idx), err), flush=True)
        assert len(idx) > 20 and err <= 1e-5
    print("CLASS_PARTS_SHARD_OK", flush=True)
else:
    assert got is None
dist.barrier()
dist.destroy_process_group()

"""Float64 restatement of the acquisition scores of a statistics record (include/bayesod.h, bod_stat_acquisition),
with plain loops over the anchors.  It shares no code with the product: the inputs are the record's fp32 arrays, the gate ``thr``
(a float32, compared with the stored float32 background sum, so the foreground set is the library's exactly) and ``top_k``."""
import math

import numpy as np

NAN = float("nan")


def threshold(min_foreground, samples):
    """The gate the library computes on the host: (float)((1.0 - (double)min_foreground) * K)."""
    return np.float32((1.0 - float(np.float32(min_foreground))) * samples)


def _finite(row):
    return all(math.isfinite(float(x)) for x in row)


def _mean(values):
    return sum(values) / len(values) if values else NAN


def _max(values):
    return max(values) if values else NAN


def acquisition(cls_sum, box_moments, cov_sum, ent_sum, samples, thr, top_k):
    """(scores [B,12], per_class [B,C-1,3], mi_map [B,A]) float64; ``cov_sum`` / ``ent_sum`` may be None."""
    cls_sum = np.asarray(cls_sum, np.float32)
    box_moments = np.asarray(box_moments, np.float32)
    nb, na, nc = cls_sum.shape
    k = float(samples)
    thr = np.float32(thr)
    scores = np.full((nb, 12), NAN)
    per_class = np.full((nb, nc - 1, 3), NAN)
    mi_map = np.full((nb, na), NAN)
    for b in range(nb):
        n_bad = 0
        ent_w, ale_w, mi_w, ebox_w, lda_w = [], [], [], [], []
        soft_num, soft_den, n_good = 0.0, 0.0, 0
        by_class = [[] for _ in range(nc - 1)]
        for a in range(na):
            rows = [cls_sum[b, a], box_moments[b, a]]
            if cov_sum is not None:
                rows.append(cov_sum[b, a])
            if ent_sum is not None:
                rows.append([ent_sum[b, a]])
            if not all(_finite(r) for r in rows):
                n_bad += 1
                continue
            n_good += 1
            c = [float(x) for x in cls_sum[b, a]]
            bg = c[nc - 1]
            h = 0.0
            for j in range(nc):
                p = c[j] / k
                if p > 0.0:
                    h -= p * math.log(p)
            ha = mi = NAN
            fg = 1.0 - bg / k
            if ent_sum is not None:
                ha = float(ent_sum[b, a]) / k
                mi = max(h - ha, 0.0)
                soft_num += fg * mi
                soft_den += fg
            if not cls_sum[b, a, nc - 1] <= thr:           # two stored float32
                continue
            m = [float(x) for x in box_moments[b, a]]
            den = m[2] * m[2] + m[3] * m[3]
            num = (m[4] + m[6] + m[9] + m[13]) / (k - 1.0)
            ebox = num / den if den != 0.0 else (NAN if num == 0.0 else math.copysign(math.inf, num))
            best = 0
            for j in range(1, nc - 1):
                if cls_sum[b, a, j] > cls_sum[b, a, best]:
                    best = j
            ent_w.append(h)
            ebox_w.append(ebox)
            if ent_sum is not None:
                ale_w.append(ha)
                mi_w.append(mi)
                mi_map[b, a] = mi
            if cov_sum is not None:
                x = [float(v) for v in cov_sum[b, a]]
                lda_w.append((x[0] + x[4] + x[5] + x[9]) / k)
            by_class[best].append((mi, ebox))
        top = sorted(mi_w, reverse=True)[:min(int(top_k), len(mi_w))]
        scores[b] = [len(ent_w), n_bad, _mean(ent_w), _mean(ale_w), _mean(mi_w), _max(mi_w),
                     soft_num / soft_den if (ent_sum is not None and soft_den != 0.0) else NAN, _mean(top),
                     _mean(ebox_w), _max(ebox_w), _mean(lda_w), _max(lda_w)]
        for j in range(nc - 1):
            members = by_class[j]
            per_class[b, j, 0] = len(members)
            per_class[b, j, 1] = _max([m[0] for m in members]) if ent_sum is not None else NAN
            per_class[b, j, 2] = _max([m[1] for m in members])
    return scores, per_class, mi_map

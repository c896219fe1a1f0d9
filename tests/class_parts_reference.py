"""TEST INFRASTRUCTURE shared by tests/test_class_parts_host.py and tests/test_gpu_class_parts.py: the float64 statement of the
class-entropy parts (include/bayesod.h).  Nothing here calls the code under test.

The MC predictive class distribution of an anchor is the mean pbar of its K samples' softmax rows p_n.  Its entropy H(pbar) splits
into the mean of the samples' entropies (aleatoric) and the rest, the mutual information between class and weights (epistemic).
A detection's M members count as M * K samples of one object: the entropy of the members' mean distribution splits into the
members' mean aleatoric part, their mean mutual information and the disagreement between the members' means (spatial)."""
import numpy as np


def entropy(p):
    """H(p) = -sum_j p_j log p_j over the last axis (natural log, 0 log 0 = 0), float64."""
    p = np.asarray(p, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(p > 0, p * np.log(p), 0.0)
    return -t.sum(axis=-1)


def softmax(logits):
    z = np.asarray(logits, np.float64)
    z = z - z.max(axis=-1, keepdims=True)
    e = np.exp(z)
    return e / e.sum(axis=-1, keepdims=True)


def sample_entropy(logits):
    """H(softmax(logits)) in the form the kernels use: log(sden) - (sum_j v_j (l_j - mx)) / sden, float64."""
    z = np.asarray(logits, np.float64)
    z = z - z.max(axis=-1, keepdims=True)
    v = np.exp(z)
    sden = v.sum(axis=-1)
    return np.log(sden) - (v * z).sum(axis=-1) / sden


def statistics(cls, sample_axis=1):
    """(cls_sum [...,A,C], ent_sum [...,A]) of raw logits [..., n, A, C] summed over ``sample_axis``."""
    return softmax(cls).sum(axis=sample_axis), sample_entropy(cls).sum(axis=sample_axis)


def posterior_rows(cls_sum, ent_sum, k):
    """rows [...,3] = total, aleatoric, epistemic and mean_probs [...,C] of a record of k samples."""
    pbar = np.asarray(cls_sum, np.float64) / float(k)
    total = entropy(pbar)
    ale = np.asarray(ent_sum, np.float64) / float(k)
    return np.stack([total, ale, np.maximum(total - ale, 0.0)], axis=-1), pbar


def posterior_rows_from_debug(debug, cls):
    """The kept rows of ``oracle.bayes_od.bayes_od_posterior(..., return_debug=True)`` for one image: ``cls`` [n,A,C] are the raw
    logits the oracle saw; its own ``mean_probs`` [A,C] is pbar.  Returns (rows [M,3], mean_probs [M,C])."""
    keep = np.asarray(debug["keep"], bool)
    pbar = np.asarray(debug["mean_probs"], np.float64)[keep]
    total = entropy(pbar)
    ale = sample_entropy(np.asarray(cls)[:, keep]).mean(axis=0)
    return np.stack([total, ale, np.maximum(total - ale, 0.0)], axis=-1), pbar


def cluster_rows(mean_probs, rows, members):
    """One detection: ``members`` (bool [M] or an index list) of the posterior rows -> total, aleatoric, epistemic_mc,
    epistemic_spatial."""
    p = np.asarray(mean_probs, np.float64)[members]
    r = np.asarray(rows, np.float64)[members]
    total = entropy(p.mean(axis=0))
    ale, emc = r[:, 1].mean(), r[:, 2].mean()
    return np.array([total, ale, emc, max(total - (ale + emc), 0.0)])


def cluster_class_parts(mean_probs, rows, centres, affinity, affinity_threshold=0.7):
    """[K,4] for ``oracle.clustering.bayes_od_clustering``'s clusters: members of centre k are
    ``affinity[:, centre] > affinity_threshold`` (the oracle's rule, inference_utils.py:316)."""
    out = [cluster_rows(mean_probs, rows, np.asarray(affinity)[:, c] > affinity_threshold) for c in centres]
    return np.asarray(out, np.float64).reshape(-1, 4)

"""Choosing frames to label from the acquisition scores of a statistics handle (``Engine.stat_acquisition``):
the column names, a ranking and a budgeted, optionally class-balanced selection.  NumPy only; the scores come from the GPU."""
import numpy as np

COLUMNS = ('n_fg', 'n_bad', 'entropy_mean', 'aleatoric_entropy_mean', 'mi_mean', 'mi_max', 'mi_soft', 'mi_topk',
           'box_epistemic_mean', 'box_epistemic_max', 'box_aleatoric_mean', 'box_aleatoric_max')
PER_CLASS_COLUMNS = ('count', 'mi_max', 'box_epistemic_max')
DEFAULTS = {'min_foreground': 0.05, 'top_k': 16}


def column(by):
    """Index of the score column ``by`` (a name of COLUMNS, or its index)."""
    if isinstance(by, str):
        if by not in COLUMNS:
            raise ValueError("by must be one of %s, got %r" % (list(COLUMNS), by))
        return COLUMNS.index(by)
    by = int(by)
    if not 0 <= by < len(COLUMNS):
        raise ValueError("score column %d outside 0..%d" % (by, len(COLUMNS) - 1))
    return by


def _descending(values):
    """Indices by value, largest first; NaN last; ties (and the NaNs among themselves) by the lower index."""
    values = np.asarray(values, np.float64)
    nan = np.isnan(values)
    key = np.where(nan, -np.inf, values)
    return np.lexsort((np.arange(len(values)), -key, nan))


def rank_frames(scores, by):
    """Frame indices in descending order of the column ``by`` of ``scores`` [F,12]: NaN last, ties broken by the lower index."""
    scores = np.asarray(scores, np.float64)
    if scores.ndim != 2 or scores.shape[1] != len(COLUMNS):
        raise ValueError("scores must be [F,%d], got %s" % (len(COLUMNS), scores.shape))
    return _descending(scores[:, column(by)])


def select_frames(scores, per_class, by, budget, class_balanced=False):
    """The ``budget`` frames to label next (fewer when the pool is smaller), as indices in the order they were chosen.
    Without ``class_balanced`` they are the head of ``rank_frames(scores, by)``.  With it the choice is greedy: take the class
    the fewest already-selected frames contain (a frame contains class j when ``per_class[f, j, 0] > 0``; ties go to the lower
    class), pick the unselected frame containing it whose MI maximum for that class is largest (``per_class[f, j, 1]``; the box
    spread ``per_class[f, j, 2]`` when the scores carry no MI), and when no frame is left for that class take the next of the
    plain ranking."""
    order = rank_frames(scores, by)
    budget = int(budget)
    if budget < 0:
        raise ValueError("budget must be >= 0, got %d" % budget)
    n = min(budget, len(order))
    if not class_balanced:
        return order[:n]
    per_class = np.asarray(per_class, np.float64)
    if per_class.ndim != 3 or per_class.shape[0] != len(order) or per_class.shape[2] != len(PER_CLASS_COLUMNS):
        raise ValueError("per_class must be [%d,C-1,3], got %s" % (len(order), per_class.shape))
    has = per_class[:, :, 0] > 0
    value = per_class[:, :, 2] if np.all(np.isnan(per_class[:, :, 1])) else per_class[:, :, 1]
    chosen, taken = [], np.zeros(len(order), bool)
    held = np.zeros(per_class.shape[1], np.int64)        # selected frames that contain class j
    while len(chosen) < n:
        j = int(np.argmin(held))                          # (the first minimum: the lower class index)
        left = has[:, j] & ~taken
        if left.any():
            pick = int(_descending(np.where(left, np.nan_to_num(value[:, j], nan=-np.inf), np.nan))[0])
        else:
            pick = int(next(f for f in order if not taken[f]))
        chosen.append(pick)
        taken[pick] = True
        held[has[pick]] += 1
    return np.asarray(chosen, np.int64)


def save(path, frames, scores, per_class):
    """acquisition.npz: ``frames`` (names), ``columns``, ``scores`` [F,12], ``per_class`` [F,C-1,3]."""
    np.savez(path, frames=np.asarray([str(f) for f in frames]), columns=np.asarray(COLUMNS), scores=np.asarray(scores, np.float64),
             per_class=np.asarray(per_class, np.float64))
    return path


def load(path):
    """(frames, scores, per_class) of a file written by ``save``; the columns must be this module's."""
    with np.load(path, allow_pickle=False) as z:
        columns = tuple(str(c) for c in z['columns'])
        if columns != COLUMNS:
            raise ValueError("%s: columns %s are not %s" % (path, list(columns), list(COLUMNS)))
        return [str(f) for f in z['frames']], z['scores'].astype(np.float64), z['per_class'].astype(np.float64)

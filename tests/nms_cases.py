"""Inputs and the NumPy restatement shared by the NMS tests (s2v_nms, face.nms_device).

A candidate row is ``row_stride`` float32 values: [0] the position index (int bits), [1..4] x1 y1 x2 y2,
[5] the score, the rest payload.  ``contract`` restates s2v_nms's contract (include/s2v.h) in NumPy, sweep
included, without calling face.py_cpu_nms: the host tests prove the two equal on distinct scores."""
import numpy as np

OK, OVER_CAPACITY, NAN_SCORE = 0, 1, 2


def position_index(rows):
    return np.ascontiguousarray(rows[:, 0]).view(np.uint32)


def position_sorted(rows):
    """The rows as the host path sees them: ordered by position index."""
    return rows[np.argsort(position_index(rows), kind="stable")]


def contract(rows, iou_thresh, min_score=-np.inf, top_k=0, keep_max=None, capacity=None):
    """rows float32 [K, rs] in any order -> (kept rows [min(kept, keep_max), rs] in keep order, kept, status)."""
    rows = np.asarray(rows, np.float32)
    none = rows[:0]
    if np.isnan(rows[:, 5]).any():
        return none, 0, NAN_SCORE
    rows = rows[rows[:, 5] > np.float32(min_score)]                       # 1. the pre-filter
    left = min(len(rows), top_k) if top_k > 0 else len(rows)             # the rows steps 1 and 3 leave
    if capacity is not None and left > capacity:
        return none, 0, OVER_CAPACITY
    # 2. score descending, the larger position index first among equal scores (-0 == +0)
    order = np.lexsort((-position_index(rows).astype(np.int64), -rows[:, 5].astype(np.float64)))
    if top_k > 0:
        order = order[:top_k]                                             # 3.
    r = rows[order]
    x1, y1, x2, y2 = (r[:, k] for k in (1, 2, 3, 4))
    one, zero, thr = np.float32(1), np.float32(0), np.float32(iou_thresh)
    area = (x2 - x1 + one) * (y2 - y1 + one)
    dead = np.zeros(len(r), bool)
    keep = []
    with np.errstate(all="ignore"):
        for i in range(len(r)):                                           # 4. the greedy sweep, fp32
            if dead[i]:
                continue
            keep.append(i)
            w = np.maximum(zero, np.minimum(x2[i], x2[i + 1:]) - np.maximum(x1[i], x1[i + 1:]) + one)
            h = np.maximum(zero, np.minimum(y2[i], y2[i + 1:]) - np.maximum(y1[i], y1[i + 1:]) + one)
            inter = w * h
            ovr = inter / (area[i] + area[i + 1:] - inter)
            dead[i + 1:] |= ~(ovr <= thr)                                  # a NaN overlap suppresses
    kept = r[keep]
    return (kept if keep_max is None else kept[:keep_max]), len(keep), OK


def by_py_cpu_nms(rows, iou_thresh):
    """The host path on position-ordered rows: face.py_cpu_nms over [x1, y1, x2, y2, score]."""
    from s2v_amd import face
    r = position_sorted(np.asarray(rows, np.float32))
    return r[face.py_cpu_nms(r[:, 1:6], iou_thresh)] if len(r) else r


def distinct_scores(rows):
    s = rows[:, 5]
    return len(np.unique(s)) == len(s)


def clustered(seed, k, row_stride=8, spread=6.0, extent=400.0):
    """k rows in clusters of overlapping boxes, pairwise distinct scores in (0.05, 1), increasing distinct
    position indices, a payload in the remaining columns; then shuffled into "slot" order."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((k, row_stride), np.float32)
    if k == 0:
        return rows
    nclus = max(1, k // 12)
    centres = rng.uniform(20.0, extent, (nclus, 2))
    sizes = rng.uniform(15.0, 90.0, nclus)
    c = rng.integers(0, nclus, k)
    cx = centres[c, 0] + rng.normal(0.0, spread, k)
    cy = centres[c, 1] + rng.normal(0.0, spread, k)
    bw = sizes[c] * rng.uniform(0.7, 1.4, k)
    bh = sizes[c] * rng.uniform(0.7, 1.4, k)
    rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4] = cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2
    rows[:, 5] = (0.05 + 0.95 * (rng.permutation(k) + 1.0) / (k + 1.0)).astype(np.float32)
    assert distinct_scores(rows), "clustered: the scores must be pairwise distinct"
    idx = np.sort(rng.choice(8 * k + 8, k, replace=False)).astype(np.int32)
    rows[:, 0] = idx.view(np.float32)
    if row_stride > 6:
        rows[:, 6:] = rng.uniform(-50.0, 50.0, (k, row_stride - 6))
    return rows[rng.permutation(k)]


def with_ties(seed, k, row_stride=8, levels=7):
    """clustered rows whose scores take only ``levels`` values: many equal scores."""
    rows = clustered(seed, k, row_stride)
    rows[:, 5] = (np.floor(rows[:, 5] * levels) / levels + 0.01).astype(np.float32)
    assert not distinct_scores(rows)
    return rows


def disjoint(scores, row_stride=8, first_index=3):
    """One 10 x 10 box per score, far apart (nothing is suppressed): position index first_index + 2 r."""
    scores = np.asarray(scores, np.float32)
    rows = np.zeros((len(scores), row_stride), np.float32)
    rows[:, 1] = 100.0 * np.arange(len(scores))
    rows[:, 2] = 7.0
    rows[:, 3] = rows[:, 1] + 9.0
    rows[:, 4] = 16.0
    rows[:, 5] = scores
    rows[:, 0] = (first_index + 2 * np.arange(len(scores))).astype(np.int32).view(np.float32)
    return rows


def boxes(box_list, scores, row_stride=8):
    """Rows of the given [x1, y1, x2, y2] boxes and scores, position index = list position."""
    rows = np.zeros((len(box_list), row_stride), np.float32)
    rows[:, 1:5] = np.asarray(box_list, np.float32)
    rows[:, 5] = np.asarray(scores, np.float32)
    rows[:, 0] = np.arange(len(box_list), dtype=np.int32).view(np.float32)
    return rows

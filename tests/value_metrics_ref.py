"""numpy / Python-int restatement of the value-type metrics of recbole/evaluator/metrics.py (AUC, LogLoss, MAE, RMSE) and of
GAUC with the Collector's `rec.meanrank`, the reference of tests/test_value_metrics*.py and tests/test_eval_labeled_hip.py.
tests/test_value_metrics.py pins this file to sklearn.

score, label: the concatenation over all evaluation batches.  A row is positive iff label == 1.
"""
import math

import numpy as np


def auc_exact(score, label):
    """(2U, P, Nn) as Python integers: sort by score ascending, C[j] = negatives among the first j rows, and every positive
    row adds C[s] + C[e] for the run [s, e) of rows with its score.  AUC = 2U / (2 * P * Nn): the trapezoid over distinct
    thresholds (tied scores share one)."""
    score = np.asarray(score, dtype=np.float32)
    pos = np.asarray(label, dtype=np.float32) == 1
    order = np.argsort(score, kind="stable")
    s, p = score[order], pos[order]
    n = len(s)
    C = np.concatenate([[0], np.cumsum(~p)]).astype(np.int64)
    head = np.ones(n, dtype=bool)
    head[1:] = s[1:] != s[:-1]
    starts = np.flatnonzero(head)
    ends = np.append(starts[1:], n)
    two_u = 0
    for a, b in zip(starts.tolist(), ends.tolist()):
        n_pos = (b - a) - int(C[b] - C[a])
        two_u += n_pos * (int(C[a]) + int(C[b]))
    P = int(p.sum())
    return two_u, P, n - P


def auc(score, label):
    two_u, P, Nn = auc_exact(score, label)
    return float("nan") if P == 0 or Nn == 0 else two_u / (2 * P * Nn)


def sums(score, label):
    """(sum |e|, sum e^2, LogLoss sum) with math.fsum over float64 terms."""
    s = np.asarray(score, dtype=np.float32).astype(np.float64)
    y = np.asarray(label, dtype=np.float32).astype(np.float64)
    e = s - y
    p = np.clip(s, 1e-15, 1 - 1e-15)
    ll = -y * np.log(p) - (1 - y) * np.log(1 - p)
    return math.fsum(np.abs(e).tolist()), math.fsum((e * e).tolist()), math.fsum(ll.tolist())


def mae(score, label):
    return sums(score, label)[0] / len(score)


def rmse(score, label):
    return math.sqrt(sums(score, label)[1] / len(score))


def logloss(score, label):
    return sums(score, label)[2] / len(score)


def value_metrics(score, label, names):
    fn = {"auc": auc, "logloss": logloss, "mae": mae, "rmse": rmse}
    return {m: fn[m](score, label) for m in names}


def meanrank(dense_row, pos_mask):
    """[2 * pos_rank_sum, user_len, pos_len] (Python ints) of one user's row of the dense score matrix (missing = -inf):
    1-based rank in descending order, tied entries share the mean of their ranks = #greater + (#equal + 1) / 2."""
    row = np.asarray(dense_row, dtype=np.float32)
    pos_mask = np.asarray(pos_mask, dtype=bool)
    two = 0
    for v in row[pos_mask].tolist():
        two += 2 * int((row > v).sum()) + int((row == v).sum()) + 1
    return [two, int((row > -np.inf).sum()), int(pos_mask.sum())]


def dense_rows(seg_start, items, scores, pos_rows, n_items):
    """The dense restatement of a candidate batch: rows [seg_start[u], seg_start[u+1]) scattered into a [-inf] row per user (a
    repeated item is one cell), and the 0/1 matrix of the positives (`pos_rows`: row numbers of the batch)."""
    U = len(seg_start) - 1
    dense = np.full((U, n_items), -np.inf, dtype=np.float32)
    mask = np.zeros((U, n_items), dtype=bool)
    is_pos = np.zeros(len(items), dtype=bool)
    is_pos[np.asarray(pos_rows, dtype=np.int64)] = True
    for u in range(U):
        for j in range(int(seg_start[u]), int(seg_start[u + 1])):
            dense[u, items[j]] = scores[j]
            if is_pos[j]:
                mask[u, items[j]] = True
    return dense, mask


def gauc(triples):
    """GAUC from the [U, 3] triples [2 * pos_rank_sum, user_len, pos_len]; users without a positive or without a negative
    are dropped.  nan when none is left."""
    num, den = [], 0
    for two_rank, user_len, pos_len in np.asarray(triples).tolist():
        if pos_len == 0 or user_len == pos_len:
            continue
        pair = (user_len + 1) * pos_len - pos_len * (pos_len + 1) / 2 - two_rank / 2
        num.append(pair / ((user_len - pos_len) * pos_len) * pos_len)
        den += pos_len
    return math.fsum(num) / den if den else float("nan")

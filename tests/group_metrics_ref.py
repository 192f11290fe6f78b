"""TEST INFRASTRUCTURE ONLY (never imported by the product path).

References and inputs for the grouped metric kernels of csrc/metrics.hip (fr_topk_metrics_grouped, fr_gauc_grouped) and for the
`utility_by_group` results of the Evaluator.  Group g's top-k reference is metrics_ref.topk_metrics_ref on the group's rows in
member order -- the exact-rational reference of the ungrouped kernel, nothing new; GAUC's sums are exact rationals
(fractions.Fraction) rounded once.  tests/test_group_metrics_ref.py pins both to oracle/metrics.py and to evaluator.gauc's formula
on the CPU; tests/test_group_metrics_hip.py compares the kernels with them.

Tolerances (u = 2^-53, gamma_n = n u / (1 - n u)):
  * top-k: metrics_ref.topk_tolerance(ref_g, n_g, K) per group -- its count (K additions, a division, a 2-ulp log2 per rank, six
    butterfly additions, ceil(n / 64) chunk additions, one multiplication, the reference's rounding) holds for a group of n_g
    members as it stands, because the grouped kernel adds a group's chunks in the order the ungrouped one adds its blocks.
  * GAUC sums: non-negative terms; per user one division and one multiplication, then six butterfly additions, ceil(n_g / 64)
    chunk additions and the reference's rounding: gamma_(9 + ceil(n_g / 64)) |ref|.
  * counts, NaN positions and everything whose bound is 0: exact.
"""
from fractions import Fraction

import numpy as np

import metrics_ref as R

NAN = float("nan")


def segments(gidx, G):
    """(perm, group_start) of a group index: a stable argsort and the cumulative bincount (what the Evaluator hands over)"""
    gidx = np.asarray(gidx, dtype=np.int64)
    perm = np.argsort(gidx, kind="stable").astype(np.int64)
    start = np.concatenate(([0], np.cumsum(np.bincount(gidx, minlength=G)))).astype(np.int64)
    return perm, start


def members(perm, start, g):
    rows = np.arange(int(start[g]), int(start[g + 1]))
    return rows if perm is None else np.asarray(perm)[rows]


def group_topk_ref(rec, perm, start):
    """float64 [G, 6, K]: topk_metrics_ref of every group's rows in member order (an empty group: NaN), and the sizes"""
    rec = np.asarray(rec)
    G, K = len(start) - 1, rec.shape[1] - 1
    out = np.full((G, 6, K), NAN)
    for g in range(G):
        rows = members(perm, start, g)
        if len(rows):
            out[g] = R.topk_metrics_ref(rec[rows])
    return out, np.diff(np.asarray(start))


def group_topk_tolerance(ref, sizes, K):
    return np.stack([R.topk_tolerance(ref[g], max(int(n), 1), K) for g, n in enumerate(sizes)])


def gauc_user(two_rank, user_len, pos_len):
    """auc_u of one kept user as an exact rational: pair / ((user_len - pos_len) * pos_len)"""
    pair = Fraction((user_len + 1) * pos_len) - Fraction(pos_len * (pos_len + 1), 2) - Fraction(two_rank, 2)
    return pair / ((user_len - pos_len) * pos_len)


def group_gauc_ref(meanrank, perm, start):
    """(sums float64 [G, 2] = { sum auc_u * pos_len, sum pos_len }, kept int64 [G, 3] = { kept, no positive, no negative })"""
    t = [[int(x) for x in row] for row in np.asarray(meanrank)]
    G = len(start) - 1
    sums, kept = np.zeros((G, 2)), np.zeros((G, 3), dtype=np.int64)
    for g in range(G):
        a, w = Fraction(0), 0
        for u in members(perm, start, g):
            two_rank, user_len, pos_len = t[u]
            if pos_len == 0:
                kept[g, 1] += 1
            elif user_len == pos_len:
                kept[g, 2] += 1
            else:
                kept[g, 0] += 1
                a += gauc_user(two_rank, user_len, pos_len) * pos_len
                w += pos_len
        sums[g] = float(a), float(w)
    return sums, kept


def gauc_tolerance(ref, sizes):
    return np.array([[R.gamma(9 + (int(n) + 63) // 64)] for n in sizes]) * np.abs(ref)


def gauc_float64(meanrank):
    """evaluator.gauc's formula restated in numpy float64 (the quotient of the two sums; NaN if no user is kept)"""
    t = np.asarray(meanrank, dtype=np.float64).reshape(-1, 3)
    two_rank, user_len, pos_len = t[:, 0], t[:, 1], t[:, 2]
    keep = (pos_len != 0) & (user_len != pos_len)
    two_rank, user_len, pos_len = two_rank[keep], user_len[keep], pos_len[keep]
    if not pos_len.size:
        return NAN
    pair = (user_len + 1) * pos_len - pos_len * (pos_len + 1) / 2 - two_rank / 2
    return float((pair / ((user_len - pos_len) * pos_len) * pos_len).sum() / pos_len.sum())


# ---- the inputs of the tests ---------------------------------------------------------------------------------------------------------

CHUNK_SIZES = [1, 63, 64, 65, 129]
CHUNK_K = [1, 20, 62]
GROUP_COUNTS = [(1, 65), (2, 129), (3, 200), (9, 200), (70, 70), (5, 200)]          # (G, U)
GROUP_K = 20
IDENTITY_SHAPES = [(1, 1), (64, 1), (65, 20), (129, 2), (200, 20)]


def assignment(n_users, G):
    """group of every user: a seeded shuffle of u mod G, so the groups interleave, every group is present and none walks in
    step with the 8-row cycle of metrics_ref.topk_case"""
    return np.random.default_rng([n_users, G, 29]).permutation(np.arange(n_users) % G).astype(np.int64)


def chunk_case(K, shuffled):
    """(rec, perm or None, group_start): five groups of CHUNK_SIZES members over topk_case rows.  perm None: the groups are
    contiguous in row order; shuffled: the rows of the groups interleave and perm is a real sort of the group index."""
    n = sum(CHUNK_SIZES)
    rec = R.topk_case(n, K)
    if not shuffled:
        return rec, None, np.concatenate(([0], np.cumsum(CHUNK_SIZES))).astype(np.int64)
    gidx = np.random.default_rng([K, 31]).permutation(np.repeat(np.arange(len(CHUNK_SIZES)), CHUNK_SIZES))
    perm, start = segments(gidx, len(CHUNK_SIZES))
    return rec, perm, start


def meanrank_case(n_users, seed=0):
    """int64 [U, 3] triples of users with 1 .. 12 positives among 20 .. 60 cells and a consistent doubled rank sum"""
    rng = np.random.default_rng([n_users, seed, 37])
    out = np.zeros((n_users, 3), dtype=np.int64)
    for u in range(n_users):
        user_len = int(rng.integers(20, 61))
        pos_len = int(rng.integers(1, 13))
        ranks = rng.choice(np.arange(1, user_len + 1), pos_len, replace=False)
        out[u] = 2 * int(ranks.sum()) - int(rng.integers(0, 2)), user_len, pos_len       # (an odd value: a tied rank)
    return out


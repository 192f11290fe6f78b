"""TEST INFRASTRUCTURE ONLY (never imported by the product path).

Plain references for the four metric kernels of csrc/metrics.hip that every reported number comes out of: exact rationals
(fractions.Fraction) where the quantity is rational, float64 and math.fsum elsewhere, Python loops over tiny shapes.  None of
them calls oracle/metrics.py; tests/test_metrics_ref.py pins them to it on the CPU, tests/test_metrics_kernels_hip.py
compares the kernels with them.

  topk_metrics_ref        fr_topk_metrics            [6, K] = Hit, MRR, NDCG, Recall, Precision, MAP @ 1..K
  eval_hits_ref           fr_eval_hits               the `rec.topk` matrix from the dense 0/1 matrix of the positives
  group_sums_ref          fr_group_sums              [K, G, 3] by fsum, with the sums of magnitudes a tolerance needs
  fair_from_stats_ref     fr_fair_metrics_from_stats five numbers and their error bounds

Tolerances: u = 2^-53 (double), v = 2^-24 (float32), gamma(n, w) = n w / (1 - n w).
"""
import math
from fractions import Fraction

import numpy as np

U64 = 2.0 ** -53
V32 = 2.0 ** -24
NAN = float("nan")


def gamma(n, w=U64):
    return n * w / (1.0 - n * w)


# ---- fr_topk_metrics -----------------------------------------------------------------------------------------------------------

def _mean(terms):
    """mean of one column of per-user terms: exact for Fractions (rounded once), fsum for floats; NaN if any term is NaN"""
    if any(isinstance(t, float) and math.isnan(t) for t in terms):
        return NAN
    if all(isinstance(t, Fraction) for t in terms):
        return float(sum(terms, Fraction(0)) / len(terms))
    return math.fsum(float(t) for t in terms) / len(terms)


def topk_metrics_ref(rec_topk):
    """rec_topk integer [U, K + 1] = hit flags (any non-zero value is a hit) | number of positives  ->  float64 [6, K].
    Per user and rank k (1-based): hit = [a hit among the first k], mrr = 1 / rank of the first hit if it is <= k,
    recall = hits / positives, precision = hits / k, map = (sum over the hits j <= k of precision@j) / min(k, min(positives, K))
    -- all rationals; ndcg = dcg / idcg in float64 with idcg over the first min(k, min(positives, K)) ranks.
    A row with zero positives: recall 0 / 0 = NaN; idcg over ALL K ranks (the reference's index min(k, 0) - 1 wraps to the last
    rank), so ndcg = 0; map = sum / K = 0."""
    rows = [[int(x) for x in r] for r in np.asarray(rec_topk)]
    n_users, K = len(rows), len(rows[0]) - 1
    disc = [1.0 / math.log2(k + 2.0) for k in range(K)]
    cols = [[[None] * n_users for _ in range(K)] for _ in range(6)]
    for u, row in enumerate(rows):
        pos_len = row[K]
        ilen = min(pos_len, K)
        csum, first, sum_pre, hit_disc = 0, None, Fraction(0), []
        for k in range(K):
            if row[k] != 0:
                csum += 1
                first = k if first is None else first
                sum_pre += Fraction(csum, k + 1)
                hit_disc.append(disc[k])
            idcg = math.fsum(disc[:min(k + 1, ilen)]) if ilen > 0 else math.fsum(disc)
            cols[0][k][u] = Fraction(1 if csum else 0)
            cols[1][k][u] = Fraction(1, first + 1) if first is not None else Fraction(0)
            cols[2][k][u] = math.fsum(hit_disc) / idcg
            cols[3][k][u] = Fraction(csum, pos_len) if pos_len != 0 else (NAN if csum == 0 else math.inf)
            cols[4][k][u] = Fraction(csum, k + 1)
            cols[5][k][u] = sum_pre / (min(k + 1, ilen) if ilen > 0 else K)
    return np.array([[_mean(cols[m][k]) for k in range(K)] for m in range(6)], dtype=np.float64)


def topk_tolerance(ref, n_users, K):
    """|kernel - ref| <= gamma_n |ref|, n = 3 K + 9 + ceil(U / 64), never looser than 1e-13 |ref| (derivation: the docstring
    of tests/test_metrics_kernels_hip.py)"""
    return min(gamma(3 * K + 9 + (n_users + 63) // 64), 1e-13) * np.abs(ref)


# ---- fr_eval_hits --------------------------------------------------------------------------------------------------------------

DENSE_CELLS = 1 << 22


def eval_hits_ref(topk_idx, n_items, pos_u, pos_i):
    """topk_idx int [U, K], positives as (row, item) pairs  ->  int64 [U, K + 1]: rec[u, k] = dense[u, topk_idx[u, k]],
    rec[u, K] = dense[u].sum(), dense = the [U, n_items] 0/1 matrix of the reference's collector.  A list entry outside
    [0, n_items) addresses no cell and gives 0.  Above DENSE_CELLS cells the rows of the matrix are kept as sets of
    column indices (the same matrix, stored sparsely; test_metrics_ref.py compares the two forms)."""
    idx = [[int(x) for x in r] for r in np.asarray(topk_idx)]
    n_users, K = len(idx), len(idx[0])
    pairs = [(int(a), int(b)) for a, b in zip(pos_u, pos_i)]
    assert all(0 <= a < n_users and 0 <= b < n_items for a, b in pairs)
    rec = np.zeros((n_users, K + 1), dtype=np.int64)
    if n_users * n_items <= DENSE_CELLS:
        dense = np.zeros((n_users, n_items), dtype=np.int64)
        for a, b in pairs:
            dense[a, b] = 1
        cell = lambda u, i: int(dense[u, i])
        count = lambda u: int(dense[u].sum())
    else:
        sets = [set() for _ in range(n_users)]
        for a, b in pairs:
            sets[a].add(b)
        cell = lambda u, i: 1 if i in sets[u] else 0
        count = lambda u: len(sets[u])
    for u in range(n_users):
        for k in range(K):
            rec[u, k] = cell(u, idx[u][k]) if 0 <= idx[u][k] < n_items else 0
        rec[u, K] = count(u)
    return rec


def pos_keys(n_items, pos_u, pos_i):
    """the sorted int64 keys row * n_items + item that fr_eval_hits takes (Python integers: no overflow on the way)"""
    keys = sorted(int(a) * int(n_items) + int(b) for a, b in zip(pos_u, pos_i))
    assert all(k < 2 ** 63 for k in keys)
    return np.array(keys, dtype=np.int64)


# ---- fr_group_sums -------------------------------------------------------------------------------------------------------------

def group_sums_ref(perm, seg_start, group, value, wtrue, G):
    """stats float64 [K, G, 3] = fsum of value, count, fsum of wtrue over the members perm[seg_start[k] .. seg_start[k + 1])
    whose group index is g (perm None: identity; wtrue None: 0); a group index outside [0, G) is counted nowhere.
    Also abs_value, abs_wtrue [K, G] = the sums of |value|, |wtrue| per cell, which the tolerance needs."""
    seg = [int(x) for x in seg_start]
    K = len(seg) - 1
    stats, absv, abst = np.zeros((K, G, 3)), np.zeros((K, G)), np.zeros((K, G))
    for k in range(K):
        rows = [int(perm[j]) if perm is not None else j for j in range(seg[k], seg[k + 1])]
        for g in range(G):
            mine = [b for b in rows if int(group[b]) == g]
            vals = [float(value[b]) for b in mine]
            wts = [float(wtrue[b]) for b in mine] if wtrue is not None else []
            stats[k, g] = (math.fsum(vals), len(mine), math.fsum(wts))
            absv[k, g], abst[k, g] = math.fsum(map(abs, vals)), math.fsum(map(abs, wts))
    return stats, absv, abst


def group_sums_tolerance(abs_sum, counts):
    """gamma_(ceil(L / 16) + 5) * sum |x| per cell of L members: the cell's members spread over 16 lanes, four butterfly
    additions follow, one more for the reference's own rounding.  (A lane takes every 16th member of the SEGMENT, so it can
    meet more than ceil(L / 16) members of one cell, at most min(L, ceil(segment / 16)); the bound is kept at the tighter
    form, and worst-case rounding bounds leave room for that.)"""
    return np.array([[gamma((int(L) + 15) // 16 + 5) for L in row] for row in np.asarray(counts)]) * abs_sum


# ---- fr_fair_metrics_from_stats ------------------------------------------------------------------------------------------------

def df_table(stats):
    """the float32 table of DifferentialFairness: float32((score_sum + 1 / K) / (count + 1)), K = number of items"""
    stats = np.asarray(stats, dtype=np.float64)
    return ((stats[:, :, 0] + 1.0 / stats.shape[0]) / (stats[:, :, 1] + 1.0)).astype(np.float32)


def logf_ulp_of_numpy(table):
    """worst error of numpy's float32 logarithm on the table's entries, in units of 2 v |log a| (the reference side only:
    the kernel is not involved)"""
    a = np.asarray(table, dtype=np.float32).ravel()
    a = a[(a > 0) & (a != 1)]
    exact = np.array([math.log(float(x)) for x in a])
    return float(np.max(np.abs(np.log(a).astype(np.float64) - exact) / (2 * V32 * np.abs(exact)))) if a.size else 0.0


def fair_from_stats_ref(stats, G, logf_ulp=1.0):
    """stats float64 [K, G, 3] (sum score, count, sum true) -> (out[5], bound[5]).
    out[0..3] (G == 2, else 0): with n_g = count_g + 1e-5, p_g = score_g / n_g, r_g = true_g / n_g, the means over the items of
      value |(p0 - r0) - (p1 - r1)|, absolute ||p0 - r0| - |p1 - r1||, under |max(r0 - p0, 0) - max(r1 - p1, 0)|,
      over |max(p0 - r0, 0) - max(p1 - r1, 0)|                                         (float64 throughout, fsum mean).
    out[4]: the mean over the items of max over the pairs of |log a - log b|, a, b entries of df_table, float64 logarithms.  A pair
      with a non-positive entry (no real logarithm) does not enter the maximum -- what the kernel does; the oracle returns NaN.
    bound[0..3] = gamma_(12 + 2 + ceil(K / 256)) * max(|p|, |r|) over the call's items.
    bound[4]: the kernel rounds two logf (each within logf_ulp * 2 v |log x|) and one float32 subtraction (v |log a - log b|) per
      pair, so it sees d_ij + err_ij, |err_ij| <= b_ij = logf_ulp 2 v (|log a| + |log b|) + v d_ij, and its maximum lies in
      [d_max - b_argmax, max_ij (d_ij + b_ij)]: the item's bound is the larger distance of the two ends from d_max (a pair far
      below the maximum adds nothing).  The mean adds only double roundings: gamma_(8 + ceil(K / 256)) of the mean."""
    stats = np.asarray(stats, dtype=np.float64)
    K = stats.shape[0]
    assert stats.shape == (K, G, 3)
    out, bound = np.zeros(5), np.zeros(5)
    if G == 2:
        n = stats[:, :, 1] + 1e-5
        p, r = stats[:, :, 0] / n, stats[:, :, 2] / n
        d = p - r
        terms = (np.abs(d[:, 0] - d[:, 1]), np.abs(np.abs(d[:, 0]) - np.abs(d[:, 1])),
                 np.abs(np.where(-d[:, 0] > 0, -d[:, 0], 0.0) - np.where(-d[:, 1] > 0, -d[:, 1], 0.0)),
                 np.abs(np.where(d[:, 0] > 0, d[:, 0], 0.0) - np.where(d[:, 1] > 0, d[:, 1], 0.0)))
        for q, t in enumerate(terms):
            out[q] = math.fsum(t.tolist()) / K
        bound[:4] = gamma(12 + 2 + (K + 255) // 256) * max(float(np.abs(p).max()), float(np.abs(r).max()))
    table = df_table(stats)
    eps, item_bound = [], []
    for k in range(K):
        logs = [math.log(float(a)) if a > 0 else None for a in table[k]]
        dmax, bmax, upper = 0.0, 0.0, 0.0
        for i in range(G):
            for j in range(i + 1, G):
                if logs[i] is None or logs[j] is None:
                    continue
                dij = abs(logs[i] - logs[j])
                bij = (logf_ulp * 2 * V32 * (abs(logs[i]) + abs(logs[j])) + V32 * dij) * (1 + 4 * V32)
                if dij > dmax:
                    dmax, bmax = dij, bij
                upper = max(upper, dij + bij)
        eps.append(dmax)
        item_bound.append(max(bmax, upper - dmax))
    out[4] = math.fsum(eps) / K
    bound[4] = math.fsum(item_bound) / K + gamma(8 + (K + 255) // 256) * out[4]
    return out, bound


def fairness_ref(pos_score, pos_i, sst, neg_score=None, neg_i=None, mode="full", logf_ulp=1.0):
    """fairrec.evaluator.fairness_metrics composed from the references above, with its result keys -> (values, bounds).
    Group index = rank of the attribute value among the values present; items = the distinct item ids in ascending order;
    NonParity from one segment over all pairs; value-type metrics on the first attribute, the j-th negative attributed to the
    group of the j-th positive's user, min(len(neg), len(pos)) of them."""
    pos_score = np.asarray(pos_score, dtype=np.float32)
    pos_i = np.asarray(pos_i)
    P = len(pos_score)
    res, bnd = {}, {}

    def tables(items, group, value, wtrue, G):
        order = np.argsort(items, kind="stable")
        _, counts = np.unique(items, return_counts=True)
        seg = np.concatenate(([0], np.cumsum(counts)))
        st, absv, abst = group_sums_ref(order, seg, group, value, wtrue, G)
        # what the kernel's table errors can move a per-item term by: four quotients of a sum and a count above 1e-5
        slack = 4 * float(np.max((group_sums_tolerance(absv, st[:, :, 1]) + group_sums_tolerance(abst, st[:, :, 1])) /
                                 (st[:, :, 1] + 1e-5)))
        return st, slack

    for n, (name, col) in enumerate(sst.items()):
        vals, gidx = np.unique(np.asarray(col), return_inverse=True)
        G = len(vals)
        st, absv, _ = group_sums_ref(None, [0, P], gidx, pos_score, None, G)
        means = st[0, :, 0] / st[0, :, 1]
        key = f"NonParity Unfairness of sensitive attribute {name}"
        res[key] = float(abs(means[0] - means[1])) if G == 2 else float(np.std(means))
        bnd[key] = 4 * float(np.max(group_sums_tolerance(absv, st[:, :, 1])[0] / st[0, :, 1])) + gamma(4 * G + 8) * float(np.abs(means).max())
        st, slack = tables(pos_i, gidx, pos_score, None, G)
        out, b = fair_from_stats_ref(st, G, logf_ulp)
        key = f"Differential Fairness of sensitive attribute {name}"
        res[key], bnd[key] = float(out[4]), float(b[4]) + slack
        if n == 0:
            if mode != "full" and neg_i is not None:
                m = min(len(neg_i), P)
                items = np.concatenate((pos_i, np.asarray(neg_i)[:m]))
                value = np.concatenate((pos_score, np.asarray(neg_score, dtype=np.float32)[:m]))
                group = np.concatenate((gidx, gidx[:m]))
                wtrue = np.concatenate((np.ones(P, np.float32), np.zeros(m, np.float32)))
            else:
                items, value, group, wtrue = pos_i, pos_score, gidx, np.ones(P, np.float32)
            st, slack = tables(items, group, value, wtrue, 2)
            out, b = fair_from_stats_ref(st, 2, logf_ulp)
            for q, label in enumerate(("Value", "Absolute", "Underestimation", "Overestimation")):
                key = f"{label} Unfairness of sensitive attribute {name}"
                res[key], bnd[key] = float(out[q]), float(b[q]) + slack
    return res, bnd


# ---- the inputs of the tests (shared by test_metrics_ref.py on the CPU and test_metrics_kernels_hip.py on the GPU) -----------------

TOPK_USERS = [1, 63, 64, 65, 129, 200]
TOPK_K = [1, 2, 20, 62, 100]
TOPK_SHAPES = sorted({(65, K) for K in TOPK_K} | {(U, 20) for U in TOPK_USERS} | {(1, 1), (64, 1), (129, 2)})
ROW_KINDS = 8


def topk_case(n_users, K, zero_positive_row=None):
    """int32 [U, K + 1].  Row 0: every rank a hit with ONE positive (the row the tail lanes of the last wave read: a leak of
    it moves every column).  Rows 1.. cycle through: no hit; a hit only at rank K; every rank a hit with K positives; random
    hits with more than K positives; random hits with 10^6 positives; hit flags that are non-zero values other than 1; random
    hits with as many positives as hits; one positive hit at a random rank."""
    rng = np.random.default_rng([n_users, K, 17])
    rec = np.zeros((n_users, K + 1), dtype=np.int64)
    rec[0, :K], rec[0, K] = 1, 1
    for u in range(1, n_users):
        kind = (u - 1) % ROW_KINDS
        hits = (rng.random(K) < 0.3).astype(np.int64)
        if kind == 0:
            rec[u, K] = 3
        elif kind == 1:
            rec[u, K - 1], rec[u, K] = 1, 1
        elif kind == 2:
            rec[u, :K], rec[u, K] = 1, K
        elif kind == 3:
            rec[u, :K], rec[u, K] = hits, K + 5
        elif kind == 4:
            rec[u, :K], rec[u, K] = hits, 10 ** 6
        elif kind == 5:
            rec[u, :K] = hits * rng.choice([2, 7, -3, -1, 2 ** 31 - 1, -2 ** 31], K)
            rec[u, K] = max(int(hits.sum()), 1)
        elif kind == 6:
            rec[u, :K], rec[u, K] = hits, max(int(hits.sum()), 1)
        else:
            rec[u, rng.integers(0, K)], rec[u, K] = 1, 1
    if zero_positive_row is not None:
        rec[zero_positive_row] = 0
    return rec.astype(np.int32)


HITS_SHAPES = [(1, 1), (51, 4), (64, 3), (1, 256), (125, 7)]       # U * (K + 1) = 2, 255, 256, 257, 1000
HITS_ITEMS = [1, 2, 1000]
HITS_NPOS = ["none", "one", "two", "many"]


def eval_hits_case(n_users, K, n_items, kind):
    """(topk_idx int64 [U, K], pos_u, pos_i).  kind: none | one (a listed item of the middle row: every listed item of the rows
    before it has a key below the first positive key, of the rows after it a key above the last) | two (item n_items - 1 of a
    row and item 0 of the next: adjacent keys, each row also lists the OTHER's item) | many (a few hundred at most: the first,
    a middle and the last row without positives; a row whose every listed item is positive; positives at items 0 and
    n_items - 1 of neighbouring rows; random ones)."""
    rng = np.random.default_rng([n_users, K, n_items % 1000003, HITS_NPOS.index(kind)])
    idx = rng.integers(0, n_items, (n_users, K), dtype=np.int64)
    pairs = set()
    mid = n_users // 2
    if kind == "one":
        pairs.add((mid, int(idx[mid, 0])))
    elif kind in ("two", "many"):
        a, b = (mid, mid + 1) if mid + 1 < n_users else (max(mid - 1, 0), mid)
        idx[a, 0], idx[b, 0], idx[a, K - 1], idx[b, K - 1] = n_items - 1, 0, 0, n_items - 1
        if K == 1:
            idx[a, 0], idx[b, 0] = n_items - 1, 0
        pairs |= {(a, n_items - 1), (b, 0)}
        if kind == "many":
            empty = {0, n_users - 1, min(mid + 2, n_users - 1)} if n_users >= 6 else set()
            full = 1 if n_users >= 6 else None
            for u in range(n_users):
                if u in empty or u in (a, b):
                    continue
                if u == full:
                    pairs |= {(u, int(i)) for i in idx[u]}
                    continue
                for k in range(K):
                    if rng.random() < 0.3 and len(pairs) < 400:
                        pairs.add((u, int(idx[u, k])))
                if rng.random() < 0.5 and len(pairs) < 400:
                    pairs.add((u, int(rng.integers(0, n_items))))       # a positive the list may not hold
    pairs = sorted(pairs)
    return idx, [p[0] for p in pairs], [p[1] for p in pairs]


def eval_hits_alias_case():
    """n_items = 5, three rows: list entries -1 and 5 whose keys u * 5 + entry are positives of the NEIGHBOURING rows -- (0, 4),
    (1, 0), (1, 4), (2, 0) -- next to in-range entries that are hits and misses.  An entry out of range is never a hit."""
    idx = np.array([[5, 4, -1, 0], [-1, 5, 0, 3], [-1, 0, 5, 4]], dtype=np.int64)
    pairs = [(0, 4), (1, 0), (1, 4), (2, 0)]
    want = np.array([[0, 1, 0, 0, 1], [0, 0, 1, 0, 2], [0, 1, 0, 0, 1]], dtype=np.int64)
    return idx, 5, [p[0] for p in pairs], [p[1] for p in pairs], want


SEG_LENGTHS = [0, 1, 15, 16, 17, 33]          # cycled after one segment of 1000 members
SEG_COUNTS = [1, 15, 16, 17, 40]
GROUPS = [1, 2, 3, 8]
VALUE_KINDS = ["uniform", "mixed", "cancel", "big"]
WTRUE_KINDS = ["null", "ones", "floats"]


def group_sums_case(n_segments, G, value_kind, with_perm, wtrue_kind):
    """(perm or None, seg_start, group int32, value float32, wtrue float32 or None).  Segment 0 has 1000 members, the others cycle
    through SEG_LENGTHS.  About one member in twelve has a group index outside [0, G): -1, G or one of 8 .. 100.
    value kinds (by POSITION in the segment, whatever perm does to the rows): uniform in [0, 1); mixed signs; `cancel` = +-1e8
    alternating in sign at every 7th position among values near 1e-3; `big` = 16777216 at the head of the segment, then ones
    (float32 accumulation is visibly wrong on both; double is not)."""
    rng = np.random.default_rng([n_segments, G, VALUE_KINDS.index(value_kind), int(with_perm), WTRUE_KINDS.index(wtrue_kind)])
    lens = [1000] + [SEG_LENGTHS[(s - 1) % len(SEG_LENGTHS)] for s in range(1, n_segments)]
    seg = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    n = int(seg[-1])
    by_pos = np.empty(n, dtype=np.float32)
    for s, L in enumerate(lens):
        j = np.arange(L)
        if value_kind == "uniform":
            v = rng.random(L)
        elif value_kind == "mixed":
            v = rng.standard_normal(L) * 10.0 ** rng.integers(-3, 4, L)
        elif value_kind == "cancel":
            v = np.where(j % 7 == 0, 1e8 * np.where((j // 7) % 2 == 0, 1.0, -1.0), 1e-3 * (1 + rng.random(L)))
        else:
            v = np.where(j == 0, 16777216.0, 1.0)
        by_pos[seg[s]:seg[s + 1]] = v.astype(np.float32)
    group_pos = rng.integers(0, G, n).astype(np.int32)
    bad = rng.random(n) < 1 / 12
    group_pos[bad] = rng.choice(np.array([-1, G] + list(range(8, 101)), dtype=np.int32), int(bad.sum()))
    wt_pos = None if wtrue_kind == "null" else (np.ones(n, np.float32) if wtrue_kind == "ones"
                                                 else (rng.standard_normal(n) * 3).astype(np.float32))
    if not with_perm:
        return None, seg, group_pos, by_pos, wt_pos
    perm = rng.permutation(n).astype(np.int64)
    value, group = np.empty_like(by_pos), np.empty_like(group_pos)
    value[perm], group[perm] = by_pos, group_pos
    wtrue = None
    if wt_pos is not None:
        wtrue = np.empty_like(wt_pos)
        wtrue[perm] = wt_pos
    return perm, seg, group, value, wtrue


STATS_ITEMS = [1, 2, 255, 256, 257, 600]
ITEM_KINDS = 8


def stats_case(n_items, G):
    """float64 [K, G, 3] = (score sum, count, true sum) per (item, group), every DifferentialFairness table entry positive.
    Items cycle through: group 0 empty (count 0, sums 0: the `+ 1e-5` quotient 0 / 1e-5); group G - 1 empty; every group one
    member; p == r in every group; and the four sign patterns of (p0 - r0, p1 - r1), which take each of the four clamps through
    each branch.  Score sums span 1e-4 .. 1e4 against counts of 1 .. 50: table entries over several orders of magnitude."""
    rng = np.random.default_rng([n_items, G, 5])
    st = np.zeros((n_items, G, 3))
    for k in range(n_items):
        kind = k % ITEM_KINDS
        c = rng.integers(1, 51, G).astype(np.float64)
        t = np.floor(rng.random(G) * (c + 1))
        s = 10.0 ** rng.uniform(-4, 4, G)
        if kind == 2:
            c[:] = 1.0
            t = np.minimum(t, 1.0)
        if kind == 3:
            s = t.copy()
        if kind >= 4:
            over = [(kind - 4) & 1, (kind - 4) >> 1]
            for g in range(min(G, 2)):
                t[g] = max(t[g], 1.0)
                s[g] = t[g] * (1.0 + rng.random()) if over[g] else t[g] * rng.random()
        st[k, :, 0], st[k, :, 1], st[k, :, 2] = s, c, t
        if kind == 0:
            st[k, 0] = 0.0
        if kind == 1:
            st[k, G - 1] = 0.0
    assert bool((df_table(st) > 0).all())
    return st


def stats_case_nonpositive():
    """three items, three groups; item 1 has a NEGATIVE score sum in group 1, so that table entry is negative and its logarithm
    NaN: the pairs (0, 1) and (1, 2) of that item do not enter its maximum, the pair (0, 2) does"""
    st = np.array([[[2.0, 3, 1], [1.0, 2, 1], [0.5, 4, 2]],
                   [[3.0, 2, 1], [-5.0, 3, 1], [0.25, 1, 0]],
                   [[1.5, 1, 1], [4.0, 5, 2], [2.5, 2, 1]]], dtype=np.float64)
    assert int((df_table(st) <= 0).sum()) == 1
    return st


def chain_case(neg_len):
    """40 items, 300 positive pairs, a binary and a three-valued attribute, neg_len negatives"""
    rng = np.random.default_rng([40, neg_len])
    P = 300
    pos_i = np.concatenate((np.arange(1, 41), rng.integers(1, 41, P - 40))).astype(np.int64)
    return {"pos_score": rng.random(P).astype(np.float32), "pos_i": pos_i,
            "neg_score": rng.random(neg_len).astype(np.float32), "neg_i": rng.integers(1, 41, neg_len).astype(np.int64),
            "gender": rng.integers(0, 2, P).astype(np.float32), "age": rng.choice([18, 35, 50], P).astype(np.int64)}

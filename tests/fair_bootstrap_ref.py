"""TEST INFRASTRUCTURE ONLY (never imported by the product path).

The float64 restatement of the bootstrap of the fairness metrics: fr_bootstrap_fair_metrics (csrc/bootstrap_fair.hip), its Python
wrapper fairrec.evaluator.bootstrap_fairness and the `fairness_bootstrap` keys of the Evaluator.  tests/test_fair_bootstrap_ref.py
pins what is here on the CPU against brute force (the multiset built with np.repeat, metrics_ref.fairness_ref on it);
tests/test_fair_bootstrap_hip.py and tests/test_fair_bootstrap_eval_hip.py compare the device with it.

The statistic (include/fairrec_hip.h): in replicate b member j occurs w(unit[j], b) times, w = bootstrap_ref.weights.  Per item k and
group g the cell is S = sum w value, C = sum w, T = sum w wtrue; an item is present when sum_g C > 0, K_b = the present items.
The value-type metrics and DifferentialFairness are metrics_ref.fair_from_stats_ref of the present items' tables -- so alpha is
1 / K_b --, NonParity is metrics_ref.fairness_ref's formula on the group totals over all members.

  replicates_ref    per replicate: K_b, the five metric values and their bounds, the group totals
  nonparity_ref     NonParity per replicate from the group totals, and its bound
  evaluation_ref    the members `fairness_metrics` forms from collected arrays -> {result key: (statistic [B], bound [B])}
  interval_ref      a statistic's percentile interval and what it may move by

Every cell sum is EXACT before its one rounding: w value is exact in float64 (w <= 12, value a float32), math.fsum adds exactly.

Tolerances (u = 2^-53, v = 2^-24, gamma_n = n u / (1 - n u)); L = the members of a cell, n_g = the members of a group:
  * K_b and the group weights: exact integers.
  * group sums: the kernel adds the exact products one by one and folds per-chunk partials; no summand passes through more than
    n_g roundings whatever the order, the reference rounds once: gamma_(n_g + 1) sum w |value|.
  * value-type metrics: fair_from_stats_ref's own bound (a fixed chain in double per item) + what the kernel's cell errors move an
    item's term by, 4 quotients of a sum within gamma_(L + 1) sum w |x| over a count above 1e-5 -- the `slack` of
    metrics_ref.fairness_ref.tables, with this kernel's sequential cell sums in place of fr_group_sums' -- + the kernel's order of
    adding the K_b non-negative terms (item after item in a chunk, then the chunks) and the host's division:
    gamma_(K_b + 2) of the value.
  * DifferentialFairness: fair_from_stats_ref's bound (two device logf and a float32 subtraction per pair) + the cell errors: a
    table entry (S + alpha) / (C + 1) moves by delta = gamma_(L + 1) sum w |value| / |S + alpha| relative, which can carry it
    across one float32 rounding boundary (2 v relative); a pair's log difference moves by 2 (delta + 2 v) at the most; nothing is
    added where every cell of the item has one member (its sum is exact).  + gamma_(K_b + 2) of the value for the order.
  * NonParity: metrics_ref.fairness_ref's bound with the group-sum bound above: 4 max_g (bound_g / weight_g) +
    gamma_(4 G + 8) max |mean|.
  * a percentile: the largest bound among the usable replicates + 2 u |q| (bootstrap_ref).
"""
import math

import numpy as np

import bootstrap_ref as BR
import metrics_ref as R

NAN = float("nan")
U64, V32 = R.U64, R.V32

# the kernel's shape constants (csrc/bootstrap_fair.hip)
MAX_CHUNKS = 1024            # BF_MAX_CHUNKS
REP_TILE = 256               # one wave: 64 lanes x 4 replicates
TILE = 64                    # members, and item ends, staged at a time
MAX_GROUPS, MAX_REP = 8, 65536
WANT_VALUE, WANT_DF = 1, 2
NAMES = ("value", "absolute", "under", "over", "differential")


def chunks(n_members, n_items, n_rep):
    """min(1024, n_items, max(1, 2^20 / n_rep), ceil(n_members / 64))"""
    return max(1, min(MAX_CHUNKS, n_items, (1 << 20) // n_rep, (n_members + 63) // 64))


def workspace_bytes(n_members, n_items, n_groups, n_rep):
    """the formula include/fairrec_hip.h states"""
    return chunks(n_members, n_items, n_rep) * n_rep * (2 * n_groups + 6) * 8


def _wsum(w, x):
    """sum w x rounded once: every product exact"""
    return math.fsum((w * x).tolist())


def replicates_ref(perm, item_start, group, value, wtrue, unit, G, n_rep, seed, logf_ulp=1.0):
    """-> dict: items int64 [B]; values, bounds float64 [5, B] (NaN where K_b = 0; rows 0..3 are 0 unless G == 2);
    group_sum, group_abs float64 [G, B]; group_weight int64 [G, B]; group_size int64 [G]"""
    start = [int(x) for x in item_start]
    K, M = len(start) - 1, len(group)
    order = np.arange(M) if perm is None else np.asarray(perm, dtype=np.int64)
    group = np.asarray(group, dtype=np.int64)
    value = np.asarray(value, dtype=np.float32).astype(np.float64)
    wtrue = np.zeros(M) if wtrue is None else np.asarray(wtrue, dtype=np.float32).astype(np.float64)
    unit = np.asarray(unit, dtype=np.int64)
    users, user_of = np.unique(unit, return_inverse=True)
    W = BR.weights(users, n_rep, seed)[user_of]                                     # [M, B]
    cells = []                                                                     # (item, group, member rows in walk order)
    for k in range(K):
        rows = order[start[k]:start[k + 1]]
        for g in range(G):
            mine = rows[group[rows] == g]
            if len(mine):
                cells.append((k, g, mine))
    in_range = (group >= 0) & (group < G)
    out = {"items": np.zeros(n_rep, dtype=np.int64), "values": np.zeros((5, n_rep)), "bounds": np.zeros((5, n_rep)),
           "group_sum": np.zeros((G, n_rep)), "group_abs": np.zeros((G, n_rep)),
           "group_weight": np.zeros((G, n_rep), dtype=np.int64),
           "group_size": np.array([int((group == g).sum()) for g in range(G)], dtype=np.int64)}
    for b in range(n_rep):
        w = W[:, b].astype(np.float64)
        for g in range(G):
            rows = np.flatnonzero(in_range & (group == g))
            out["group_sum"][g, b] = _wsum(w[rows], value[rows])
            out["group_abs"][g, b] = _wsum(w[rows], np.abs(value[rows]))
            out["group_weight"][g, b] = int(W[rows, b].sum())
        stats, tol, exact = np.zeros((K, G, 3)), np.zeros((K, G, 2)), np.ones(K, dtype=bool)
        for k, g, mine in cells:
            wm = w[mine]
            stats[k, g] = (_wsum(wm, value[mine]), float(wm.sum()), _wsum(wm, wtrue[mine]))
            gam = R.gamma(len(mine) + 1)
            tol[k, g] = (gam * _wsum(wm, np.abs(value[mine])), gam * _wsum(wm, np.abs(wtrue[mine])))
            exact[k] &= len(mine) == 1
        present = stats[:, :, 1].sum(axis=1) > 0
        Kb = int(present.sum())
        out["items"][b] = Kb
        if Kb == 0:
            out["values"][:, b] = out["bounds"][:, b] = NAN
            continue
        st, tl, ex = stats[present], tol[present], exact[present]
        val, bnd = R.fair_from_stats_ref(st, G, logf_ulp)
        order_slack = R.gamma(Kb + 2) * val
        cell_slack = 4 * float(np.max((tl[:, :, 0] + tl[:, :, 1]) / (st[:, :, 1] + 1e-5)))
        with np.errstate(divide="ignore", invalid="ignore"):
            delta = np.where(ex[:, None], 0.0, tl[:, :, 0] / np.abs(st[:, :, 0] + 1.0 / Kb))
        df_slack = 0.0 if ex.all() else 2 * (float(np.max(delta)) + 2 * V32)
        out["values"][:, b] = val
        out["bounds"][:4, b] = (bnd[:4] + cell_slack + order_slack[:4]) if G == 2 else 0.0
        out["bounds"][4, b] = bnd[4] + df_slack + order_slack[4]
    return out


def nonparity_ref(ref):
    """(value [B], bound [B]) from replicates_ref's group totals: |M0 - M1| for two groups, else the population std of the group
    means sum / weight; NaN (value and bound) where a group has weight 0"""
    gs, ga, gw, size = ref["group_sum"], ref["group_abs"], ref["group_weight"], ref["group_size"]
    G, B = gs.shape
    val, bnd = np.full(B, NAN), np.full(B, NAN)
    gam = np.array([R.gamma(int(n) + 1) for n in size])
    for b in range(B):
        if (gw[:, b] == 0).any():
            continue
        means = gs[:, b] / gw[:, b]
        val[b] = abs(means[0] - means[1]) if G == 2 else float(np.std(means))
        bnd[b] = 4 * float(np.max(gam * ga[:, b] / gw[:, b])) + R.gamma(4 * G + 8) * float(np.abs(means).max())
    return val, bnd


def group_index(columns):
    """the point estimate's group index of an attribute (one column) or an intersection (several): the rank of the value, or of
    the value tuple, among those present -> (index int64 [rows], G)"""
    cols = np.stack([np.asarray(c, dtype=np.float64) for c in columns], axis=1)
    tuples, inv = np.unique(cols, axis=0, return_inverse=True)
    return inv.reshape(-1).astype(np.int64), len(tuples)


def _sorted_items(items):
    items = np.asarray(items)
    order = np.argsort(items, kind="stable")
    _, counts = np.unique(items, return_counts=True)
    return order, np.concatenate(([0], np.cumsum(counts))).astype(np.int64)


def evaluation_ref(pos_score, pos_i, pos_user, sst, n_rep, seed, neg_score=None, neg_i=None, mode="full", intersections=(),
                   value_type=True, logf_ulp=1.0):
    """{result key of the point estimate: (statistic [B], bound [B])} for every attribute of `sst` (a dict of per-positive
    columns) and every entry of `intersections`, attributes of more than eight groups left out; the value-type metrics on the
    first attribute, over the positives and (outside `full`) the first min(len(neg), P) negatives, negative j with the group and
    the unit of positive j"""
    pos_score = np.asarray(pos_score, dtype=np.float32)
    pos_i, unit = np.asarray(pos_i), np.asarray(pos_user, dtype=np.int64)
    P = len(pos_score)
    res = {}
    order, start = _sorted_items(pos_i)
    groups = [(name, [sst[name]]) for name in sst] + [("&".join(e), [sst[n] for n in e]) for e in intersections]
    for n, (name, cols) in enumerate(groups):
        gidx, G = group_index(cols)
        if G > MAX_GROUPS:
            continue
        ref = replicates_ref(order, start, gidx, pos_score, None, unit, G, n_rep, seed, logf_ulp)
        res[f"NonParity Unfairness of sensitive attribute {name}"] = nonparity_ref(ref)
        res[f"Differential Fairness of sensitive attribute {name}"] = (ref["values"][4], ref["bounds"][4])
        if n == 0 and value_type:
            if mode != "full" and neg_i is not None:
                m = min(len(neg_i), P)
                items = np.concatenate((pos_i, np.asarray(neg_i)[:m]))
                value = np.concatenate((pos_score, np.asarray(neg_score, dtype=np.float32)[:m]))
                group, units = np.concatenate((gidx, gidx[:m])), np.concatenate((unit, unit[:m]))
                wtrue = np.concatenate((np.ones(P, np.float32), np.zeros(m, np.float32)))
            else:
                items, value, group, units, wtrue = pos_i, pos_score, gidx, unit, np.ones(P, np.float32)
            o2, s2 = _sorted_items(items)
            ref = replicates_ref(o2, s2, group, value, wtrue, units, 2, n_rep, seed, logf_ulp)
            for q, label in enumerate(("Value", "Absolute", "Underestimation", "Overestimation")):
                res[f"{label} Unfairness of sensitive attribute {name}"] = (ref["values"][q], ref["bounds"][q])
    return res


def interval_ref(stat, bound, level):
    """(low, high, tolerance) of one statistic's percentile interval: bootstrap_ref.intervals_ref on the [1, B] row, and the
    largest bound among its usable replicates + 2 u |q|"""
    stat, bound = np.asarray(stat, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    low, high, _, _, usable, _ = BR.intervals_ref(stat[None, :], level)
    ok = np.isfinite(stat)
    worst = float(bound[ok].max()) if ok.any() else 0.0
    return float(low[0]), float(high[0]), worst + 2 * U64 * max(abs(float(low[0])), abs(float(high[0]))) if usable[0] else 0.0


def ci_keys(key):
    head, name = key.split(" of sensitive attribute ", 1)
    return f"{head} ci_low of sensitive attribute {name}", f"{head} ci_high of sensitive attribute {name}"


# ---- the inputs of the tests -----------------------------------------------------------------------------------------------------

N_REPS = [1, 3, 4, 5, 63, 64, 65, 257]           # the Philox quad, the wave of 256 replicates
N_ITEMS = [1, 2, 17, 257]                        # one chunk; two; 17 items in fewer chunks than items; more than 64 item ends
GROUPS = [2, 3, 8]
ITEM_LENGTHS = [1, 15, 16, 17, 33]               # cycled after item 0, which has 1000 members (16 member tiles, one chunk's chain)
UNIT_KINDS = ["spread", "own", "one"]


def case(n_items, G, with_perm, wtrue_kind, unit_kind="spread", bad_groups=False):
    """(perm or None, item_start, group int32, value float32, wtrue float32 or None, unit int64), member arrays indexed by member.
    Item 0 has 1000 members, the rest cycle through ITEM_LENGTHS.  Values uniform in (0, 1): every table entry is positive.
    wtrue: 'null', or 'ones' = ones on the first half of every item's members and zeros on the rest.
    unit: 'spread' = 129 users dealt round-robin over the positions (at least 40 per group with G <= 3: a replicate with an empty
    group has probability below e^-20); 'own' = the same, but every single-member item belongs to a user of its own (items vanish
    in some replicates, K_b varies); 'one' = one user owns every member (weight 0: K_b = 0, NaN everywhere).
    bad_groups: about one member in twelve has a group index outside [0, G): -1, G or one of 8 .. 100."""
    rng = np.random.default_rng([n_items, G, int(with_perm), ["null", "ones"].index(wtrue_kind), UNIT_KINDS.index(unit_kind),
                                 int(bad_groups), 71])
    lens = [1000] + [ITEM_LENGTHS[(k - 1) % len(ITEM_LENGTHS)] for k in range(1, n_items)]
    start = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    M = int(start[-1])
    value_pos = (rng.random(M) * 0.998 + 0.001).astype(np.float32)
    group_pos = ((np.arange(M) // 129 + np.arange(M)) % G).astype(np.int32)      # every user meets every group
    unit_pos = (np.arange(M) % 129).astype(np.int64)
    if unit_kind == "own":
        for k, L in enumerate(lens):
            if L == 1:
                unit_pos[start[k]] = 1000 + k
    elif unit_kind == "one":
        unit_pos[:] = 5
    if bad_groups:
        bad = rng.random(M) < 1 / 12
        group_pos[bad] = rng.choice(np.array([-1, G] + list(range(8, 101)), dtype=np.int32), int(bad.sum()))
    wt_pos = None
    if wtrue_kind == "ones":
        wt_pos = np.concatenate([(np.arange(L) < (L + 1) // 2).astype(np.float32) for L in lens])
    if not with_perm:
        return None, start, group_pos, value_pos, wt_pos, unit_pos
    perm = rng.permutation(M).astype(np.int64)
    group, value, unit = np.empty_like(group_pos), np.empty_like(value_pos), np.empty_like(unit_pos)
    group[perm], value[perm], unit[perm] = group_pos, value_pos, unit_pos
    wtrue = None
    if wt_pos is not None:
        wtrue = np.empty_like(wt_pos)
        wtrue[perm] = wt_pos
    return perm, start, group, value, wtrue, unit


def collected_case(mode, n_users=60, n_items=25, seed=3):
    """a synthetic collected dict (numpy) in `full` or `uni100` form: every user two to five positives, user rows ascending as the
    loaders emit them; a binary attribute `gender`, a three-valued `age` and a nine-valued `zip` per positive pair (a user's value
    on each of its pairs); in uni100 form as many negatives as positives minus three"""
    rng = np.random.default_rng([n_users, n_items, seed, ["full", "uni100"].index(mode)])
    per_user = rng.integers(2, 6, n_users)
    pos_user = np.repeat(np.arange(n_users), per_user).astype(np.int64)
    P = len(pos_user)
    pos_i = np.concatenate([rng.choice(np.arange(1, n_items), n, replace=False) for n in per_user]).astype(np.int64)
    attrs = {"gender": rng.integers(0, 2, n_users).astype(np.float32), "age": rng.choice([18, 35, 50], n_users).astype(np.int64),
             "zip": (np.arange(n_users) % 9).astype(np.int64)}
    out = {"rec.positive_score": (rng.random(P) * 0.9 + 0.05).astype(np.float32), "data.positive_i": pos_i,
           "data.positive_user": pos_user, "rec.topk": np.concatenate(
               (rng.integers(0, 2, (n_users, 5)), per_user[:, None]), axis=1).astype(np.int32)}
    out.update({"data." + k: v[pos_user] for k, v in attrs.items()})
    if mode != "full":
        out["rec.negative_score"] = (rng.random(P - 3) * 0.9 + 0.05).astype(np.float32)
        out["data.negative_i"] = rng.integers(1, n_items, P - 3).astype(np.int64)
    return out

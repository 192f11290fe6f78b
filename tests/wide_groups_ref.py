"""TEST INFRASTRUCTURE ONLY (never imported by the product path).

Plain numpy / float64 reference (math.fsum for the sums) of fr_df_cells (include/fairrec_hip.h, csrc/metrics.hip
df_cells_kernel): DifferentialFairness for any number of groups from the members in (item, group) order, and of the group
means behind NonParity.  tests/test_wide_groups_ref.py pins it to oracle/metrics.py on the CPU, tests/test_wide_groups_hip.py
compares the kernel with it.

The error bound, u = 2^-53, v = 2^-24, gamma_n = n u / (1 - n u) (metrics_ref.gamma), built the way the docstring of
tests/test_metrics_kernels_hip.py builds the one of the dense path:
  * a cell of L members: the kernel adds its members by a segmented scan over 16 lanes (at most four additions inside a trip)
    plus one carry addition per further trip the run reaches into; a run may start anywhere in a trip, so it reaches into at
    most floor((L + 14) / 16) further trips: every member passes through at most n = 4 + floor((L + 14) / 16) additions
    (`n_additions`), one more for the reference's own rounding: |sum - fsum| <= delta = gamma_(n + 1) * sum |x|.
  * the table entry: (s + 1 / K) / (c + 1) in double (4 u relative, generously) rounded to float32.  Rounding is monotone, so the
    kernel's entry lies in [a_lo, a_hi] = float32 of the two ends of s -+ delta.
  * its logarithm: the device's logf within e * 2 v |log a| of the true one -- no accuracy statement for it is at hand, so e is
    MEASURED: twice the worst error of numpy's float32 logarithm, in that unit, on this file's own tables (`logf_ulp`), on the
    reference side.  So the kernel's l_i lies in [lo_i, hi_i] = [log a_lo - e 2 v |log a_lo|, log a_hi + e 2 v |log a_hi|].
  * the item: d = lmax - lmin with one float32 subtraction, so the kernel's epsilon lies in
    [max(0, max lo_i - min hi_i) (1 - v), (max hi_i - min lo_i) (1 + v)]; the item's bound is the larger distance of the two
    ends from the float64 epsilon.  An item with ONE entry has lmax == lmin bit for bit: bound 0.
  * the mean: 15 additions inside a block of 16 items, ceil(K / 16) block additions, one multiplication, the reference's own
    rounding: gamma_(18 + ceil(K / 16)) of the mean on top of the mean of the items' bounds.
"""
import functools
import math

import numpy as np

import metrics_ref as R

V32, gamma = R.V32, R.gamma
VALUE_KINDS = R.VALUE_KINDS


def n_additions(L):
    """additions a member of a run of L members passes through in df_cells_kernel, at most"""
    return 4 + (int(L) + 14) // 16


def n_additions_dense(L, segment):
    """... in group_sums_kernel: a lane takes every 16th member of the segment, then four butterfly additions (and the
    reference's rounding, which the caller of this adds)"""
    return min(int(L), (int(segment) + 15) // 16) + 4


# ---- the cells --------------------------------------------------------------------------------------------------------------------

def cells_ref(perm, item_start, group, value, G):
    """per item the list of its cells (g, fsum of value, members, fsum of |value|), one per run of equal group index in the
    item's range, runs whose group index is outside [0, G) left out"""
    start = [int(x) for x in item_start]
    items = []
    for k in range(len(start) - 1):
        rows = [int(perm[j]) if perm is not None else j for j in range(start[k], start[k + 1])]
        cells, at = [], 0
        while at < len(rows):
            g, end = int(group[rows[at]]), at + 1
            while end < len(rows) and int(group[rows[end]]) == g:
                end += 1
            vals = [float(value[b]) for b in rows[at:end]]
            if 0 <= g < G:
                cells.append((g, math.fsum(vals), end - at, math.fsum(map(abs, vals))))
            at = end
        items.append(cells)
    return items


def table_entries(cells, K, G):
    """the float32 table entries of one item: float32((s + 1 / K) / (c + 1)) per cell, and float32(1 / K) once when fewer than G
    groups have a cell"""
    a = [np.float32((s + 1.0 / K) / (c + 1.0)) for _, s, c, _ in cells]
    if len(cells) < G:
        a.append(np.float32(1.0 / K))
    return a


def df_cells_ref(perm, item_start, group, value, G, logf_ulp=1.0, n_add=n_additions):
    """-> dict: cells (cells_ref), table (per item the float32 entries), eps float64 [K] (max - min of the float64 logarithms of
    the positive entries; 0 without one), mean, item_bound [K], bound (see the docstring of this file).  `n_add(L)` = the
    additions a member of a cell of L members passes through in the code under test."""
    return df_from_cells(cells_ref(perm, item_start, group, value, G), G, logf_ulp, n_add)


def df_from_cells(cells, G, logf_ulp=1.0, n_add=n_additions):
    """df_cells_ref from the cells of cells_ref (which hold every sum the rest needs)"""
    K = len(cells)
    alpha = 1.0 / K
    eps, item_bound, table = [], [], []
    for item in cells:
        ref_l, lo, hi = [], [], []
        entries = table_entries(item, K, G)
        table.append(entries)
        for n, a in enumerate(entries):
            if n < len(item):
                _, s, c, absx = item[n]
                delta = gamma(n_add(c) + 1) * absx
                x_lo, x_hi = (s - delta + alpha) / (c + 1.0), (s + delta + alpha) / (c + 1.0)
                a_lo = np.float32(x_lo - 4 * R.U64 * abs(x_lo))
                a_hi = np.float32(x_hi + 4 * R.U64 * abs(x_hi))
            else:
                a_lo = a_hi = a
            assert a_lo > 0 or a_hi < 0, "a table entry the rounding errors can carry across zero: not a case for this reference"
            if a_hi < 0:
                continue                      # a NaN logarithm is left out
            ref_l.append(math.log(float(a)))
            l_lo, l_hi = math.log(float(a_lo)), math.log(float(a_hi))
            lo.append(l_lo - logf_ulp * 2 * V32 * abs(l_lo))
            hi.append(l_hi + logf_ulp * 2 * V32 * abs(l_hi))
        if len(ref_l) < 2:
            eps.append(0.0)
            item_bound.append(0.0)
            continue
        e = max(ref_l) - min(ref_l)
        upper = (max(hi) - min(lo)) * (1 + V32)
        lower = max(0.0, max(lo) - min(hi)) * (1 - V32)
        eps.append(e)
        item_bound.append(max(upper - e, e - lower))
    mean = math.fsum(eps) / K
    bound = math.fsum(item_bound) / K + gamma(18 + (K + 15) // 16) * mean
    return {"cells": cells, "table": table, "eps": np.array(eps), "mean": mean, "item_bound": np.array(item_bound),
            "bound": bound}


def eps_pairwise_f32(entries):
    """the reference's form on one item's float32 entries with numpy's own float32 logarithm: the largest |log a - log b| over the
    pairs, a NaN difference left out"""
    with np.errstate(invalid="ignore", divide="ignore"):
        l = np.log(np.asarray(entries, dtype=np.float32))
        d = np.abs(l[:, None] - l[None, :])          # float32, every pair
    assert d.dtype == np.float32
    d = d[~np.isnan(d)]
    return np.float32(max(d.max(), np.float32(0))) if d.size else np.float32(0)


def eps_maxmin_f32(entries):
    """the kernel's form on the same entries and logarithm: lmax - lmin over the logarithms that are no NaN, 0 unless positive"""
    with np.errstate(invalid="ignore", divide="ignore"):
        l = np.log(np.asarray(entries, dtype=np.float32))
        l = l[~np.isnan(l)]
        if not l.size:
            return np.float32(0)
        d = np.float32(l.max() - l.min())
    return d if d > 0 else np.float32(0)


def group_means_ref(group, value, G):
    """(means float64 [G] by fsum, bound [G] for means that come out of fr_group_sums with the groups as its segments: a lane
    takes every 16th member, four butterfly additions, the reference's rounding, one division)"""
    means, bound = np.zeros(G), np.zeros(G)
    for g in range(G):
        vals = [float(x) for x in np.asarray(value)[np.asarray(group) == g]]
        L = len(vals)
        means[g] = math.fsum(vals) / L
        bound[g] = gamma((L + 15) // 16 + 5) * math.fsum(map(abs, vals)) / L + 2 * R.U64 * abs(means[g])
    return means, bound


def attribute_ref(pos_score, pos_i, gidx, G, logf_ulp, n_add=n_additions):
    """what fairrec.evaluator.fairness_metrics reports for an attribute with group index gidx in [0, G), every group present:
    -> (NonParity, its bound, DifferentialFairness, its bound).  The members are walked in the order of a stable sort of the key
    item * G + group; the items are the distinct item ids."""
    pos_score = np.asarray(pos_score, dtype=np.float32)
    gidx = np.asarray(gidx, dtype=np.int64)
    means, mb = group_means_ref(gidx, pos_score, G)
    nonparity = float(abs(means[0] - means[1])) if G == 2 else float(np.std(means))
    np_bound = 4 * float(mb.max()) + gamma(4 * G + 8) * float(np.abs(means).max())
    key = np.asarray(pos_i, dtype=np.int64) * G + gidx
    order = np.argsort(key, kind="stable")
    _, counts = np.unique(key[order] // G, return_counts=True)
    start = np.concatenate(([0], np.cumsum(counts)))
    df = df_cells_ref(order, start, gidx, pos_score, G, logf_ulp, n_add)
    return nonparity, np_bound, df["mean"], df["bound"]


# ---- the inputs (shared by test_wide_groups_ref.py on the CPU and test_wide_groups_hip.py on the GPU) ---------------------------

ITEM_COUNTS = [1, 2, 15, 16, 17, 40, 257]          # the 16 items of a block -+ 1, more than one block, 256 + 1
GROUPS = [1, 2, 9, 21, 64, 65, 300]
RUN_LENGTHS = [1, 15, 16, 17, 33]                  # cycled after one run of 1000 members
MAX_SOME = 11                                      # runs of an item that has "some" groups


def _run_values(rng, kind, L):
    """float32 [L] by position in the run.  uniform in [0, 1); `mixed` signs over seven orders of magnitude, the run negated if
    its sum is not positive; `cancel` = +-1e8 alternating at every 7th position (from the 4th) among values near 1e-3: the runs
    of 15, 16 and 17 members hold one pair that cancels, the runs of 33 and 1000 an odd number; `big` = 16777216, then ones
    (float32 accumulation is visibly wrong on the last two; double is not)."""
    j = np.arange(L)
    if kind == "uniform":
        v = rng.random(L)
    elif kind == "mixed":
        v = (rng.standard_normal(L) * 10.0 ** rng.integers(-3, 4, L)).astype(np.float32)
        if math.fsum(float(x) for x in v) <= 0:
            v = -v
    elif kind == "cancel":
        v = np.where(j % 7 == 3, 1e8 * np.where((j // 7) % 2 == 0, 1.0, -1.0), 1e-3 * (1 + rng.random(L)))
    else:
        v = np.where(j == 0, 16777216.0, 1.0)
    return v.astype(np.float32)


def cells_case(n_items, G, with_perm, salt=0, empty_item=True, bad_groups=False, negative_cell=False):
    """(perm or None, item_start int64 [n_items + 1], group int32, value float32).
    Item 0 has every group (its first run 1000 members long); the others cycle through: some groups (1 .. MAX_SOME of them,
    ascending), exactly one group, a few groups in SHUFFLED order (runs only have to be contiguous), every group (G <= 21
    only).  The middle item's range is empty (n_items >= 3, `empty_item`).  Run lengths cycle through RUN_LENGTHS, value kinds
    through VALUE_KINDS, run by run.
    bad_groups: every third item also has a run with group index -1 at its head and one with G at its tail, of large values.
    negative_cell: the second run of item 0 (or its only one) sums to about -5 L."""
    rng = np.random.default_rng([n_items, G, int(with_perm), salt, int(bad_groups), int(negative_cell)])
    start, groups, values = [0], [], []
    n_run = 0

    def add_run(g, L, kind, negate=False):
        v = _run_values(rng, kind, L)
        if negate:
            v = -(5 + rng.random(L)).astype(np.float32)
        groups.append(np.full(L, g, dtype=np.int32))
        values.append(v)

    for k in range(n_items):
        if empty_item and n_items >= 3 and k == n_items // 2:
            start.append(start[-1])
            continue
        shape = (k - 1) % 4
        if k == 0 or (shape == 3 and G <= 21):
            present = list(range(G))
        elif shape == 0:
            present = sorted(rng.choice(G, size=min(G, int(rng.integers(1, MAX_SOME + 1))), replace=False).tolist())
        elif shape == 1:
            present = [int(rng.integers(0, G))]
        else:
            present = rng.permutation(rng.choice(G, size=min(G, 3), replace=False)).tolist()
        bad = bad_groups and k % 3 == 0
        if bad:
            add_run(-1, 17, "big")
        for r, g in enumerate(present):
            L = 1000 if (k == 0 and r == 0) else RUN_LENGTHS[n_run % len(RUN_LENGTHS)]
            add_run(g, L, VALUE_KINDS[(n_run + salt) % len(VALUE_KINDS)],
                    negate=negative_cell and k == 0 and r == min(1, len(present) - 1))
            n_run += 1
        if bad:
            add_run(G, 16, "big")
        start.append(sum(len(x) for x in groups))
    start = np.array(start, dtype=np.int64)
    g_pos = np.concatenate(groups) if groups else np.zeros(0, np.int32)
    v_pos = np.concatenate(values) if values else np.zeros(0, np.float32)
    if not with_perm:
        return None, start, g_pos, v_pos
    perm = rng.permutation(len(g_pos)).astype(np.int64)
    group, value = np.empty_like(g_pos), np.empty_like(v_pos)
    group[perm], value[perm] = g_pos, v_pos
    return perm, start, group, value


def grid_case(n_items, G):
    """the case of the (items, groups) grid: the value kind a run starts the cycle with and perm NULL / a real permutation vary
    over the grid"""
    ii, gi = ITEM_COUNTS.index(n_items), GROUPS.index(G)
    return cells_case(n_items, G, with_perm=(ii + gi) % 2 == 1, salt=ii + gi)


@functools.lru_cache(maxsize=None)
def grid_cells(n_items, G):
    return cells_ref(*grid_case(n_items, G), G)


def grid_ref(n_items, G):
    return df_from_cells(grid_cells(n_items, G), G, logf_ulp())


def dense_restatement(perm, item_start, group, value):
    """(score float64, item ids, attribute values) per member, for oracle/metrics.py: the attribute value of group g is 10 + 3 g,
    the id of item k is 7 + 2 k"""
    start = [int(x) for x in item_start]
    rows = np.array([int(perm[j]) if perm is not None else j for j in range(start[-1])], dtype=np.int64)
    item = np.repeat(np.arange(len(start) - 1), np.diff(start))
    return (np.asarray(value, dtype=np.float64)[rows], 7 + 2 * item, 10 + 3 * np.asarray(group, dtype=np.int64)[rows])


@functools.lru_cache(maxsize=None)
def logf_ulp():
    """e of the bound: twice the worst error of numpy's float32 logarithm on the tables of this file's grid, in units of
    2 v |log x| (reference side only: the kernel is not involved)"""
    worst = 0.0
    for n_items in ITEM_COUNTS:
        for G in GROUPS:
            ref = df_from_cells(grid_cells(n_items, G), G)
            worst = max(worst, R.logf_ulp_of_numpy(np.array([a for row in ref["table"] for a in row], dtype=np.float32)))
    return 2 * worst


def chain_case():
    """40 items, 300 positive pairs; a binary `gender`, a 7-valued `age`, a 21-valued `occupation`, every value present"""
    rng = np.random.default_rng([40, 21])
    P = 300
    pos_i = np.concatenate((np.arange(1, 41), rng.integers(1, 41, P - 40))).astype(np.int64)
    col = lambda vals: np.concatenate((vals, rng.choice(vals, P - len(vals))))[rng.permutation(P)]
    return {"pos_score": rng.random(P).astype(np.float32), "pos_i": pos_i,
            "gender": col(np.array([0.0, 1.0], dtype=np.float32)),
            "age": col(np.array([1, 18, 25, 35, 45, 50, 56], dtype=np.int64)),
            "occupation": col(np.arange(21, dtype=np.int64))}

"""GPU: bootstrap intervals for the per-group metrics -- fr_bootstrap_group_sums (csrc/bootstrap.hip), fr_topk_user_terms and
fr_gauc_user_terms (csrc/metrics.hip) through the C ABI against the references of tests/bootstrap_ref.py (pinned on the CPU by
tests/test_bootstrap_ref.py, where the refusals of bad arguments are tested too: they need no GPU), then the `group_bootstrap`
key through Collector, Evaluator and Trainer.evaluate on the 40-user x 71-item FOCF model of tests/test_group_metrics_hip.py.
Shapes are the smallest that reach each edge: groups of 1, 63, 64, 65 and 129 members (the 64-position chunk and LDS row tile of
small inputs), 127 / 128 / 129 / 257 members among 131 073 rows (the first n_rows whose chunks are 128 positions, two row tiles),
1 .. 1025 replicates (the Philox quad, the wave, the 1024 replicates of a workgroup), 1 .. 64 columns (the 8-column tile), 1 .. 70
groups, empty groups, perm NULL and a real sort.  Every output and every workspace sits between canary frames, every return code
is asserted, as in tests/test_group_metrics_hip.py.

Tolerances are derived in tests/bootstrap_ref.py: the weight sums exact; gamma_(n_g + 1) sum w |x| for the sums; NaN positions and
zero-bound entries exact; the user terms byte for byte what fr_topk_metrics / fr_gauc_grouped give on one row; a replicate statistic
gamma_(n_g + 2) relative (GAUC: gamma_(2 n_g + 6)), a quantile the largest such bound among its usable replicates plus 2 u |q|, a
gap two of them, and the half step of the rounding to 12 places.  Every test prints its largest error / bound, none may exceed 1.

Worst error / bound measured on an MI355X, per test group (the weight sums exact everywhere):
  fr_bootstrap_group_sums at the chunk edges 0.046 (perm NULL; 0.031 with the sorted perm); 131 073 rows 0.022 (every group
  reversed; 0.0074 in row order); 1 .. 1025 replicates 0.14 (B = 257 and 1025; 0.055 .. 0.075 below); 1 .. 64 columns 0.16
  (C = 64; 0.06 .. 0.10 below, ld = n_cols + 3 the same 0.091 as ld = n_cols); 1 / 2 / 9 / 70 groups 0.15 (G = 9; 0 with 70 groups
  of one row: one rounding each side); empty groups 0.030; one NaN value 0.082; a 64-bit seed 0.042; 6 refined groups added up
  against their 2 groups 0.015
  fr_topk_user_terms against the exact per-row terms 0.061 (byte for byte fr_topk_metrics of the row at K = 1, 20, 255);
  fr_gauc_user_terms against the exact rationals 0.66 (of 3 u: a division and a multiplication against one rounding)
  evaluator.bootstrap_group_sums over 70 columns 0.12; intervals with 134 of 200 usable replicates 0.049; two one-row groups 0
  through the Evaluator 0.987 in full mode, 0.99 in uni5: the rounding to 12 decimal places, which the bound allows for with its
  full half step, is what these two measure (the kernels' share is the figures above)
"""
import functools
import logging
import math

import numpy as np
import pytest
import torch

import bootstrap_ref as BR
import group_metrics_ref as GR
import metrics_ref as R
import test_group_metrics_hip as GMH
from test_group_metrics_hip import _evaluate, _host_groups, _run
from test_metrics_kernels_hip import _bytes, _dev, _Frames, _lib, _ptr, _st, _topk, _within

pytestmark = pytest.mark.gpu
U64 = BR.U64
SEED = 2020


# ---- fr_bootstrap_group_sums ---------------------------------------------------------------------------------------------------------

def _boot(values, perm, start, n_rep, seed=SEED, n_cols=None):
    """values [U, ld]; the first n_cols columns (default: all) are summed -> (sums [G, B, C], weight [G, B])"""
    U, ld = values.shape
    C = ld if n_cols is None else n_cols
    G = len(start) - 1
    lib, f = _lib(), _Frames()
    sums, weight = f.new(torch.float64, G, n_rep, C), f.new(torch.int64, G, n_rep)
    need = lib.fr_bootstrap_group_sums_workspace_bytes(U, C, G, n_rep)
    assert need == BR.workspace_bytes(U, C, G, n_rep)
    ws = f.ws(need)
    d = [_dev(x) for x in (values, perm, start)]
    rc = lib.fr_bootstrap_group_sums(d[0].data_ptr(), U, C, ld, _ptr(d[1]), d[2].data_ptr(), G, n_rep, seed, sums.data_ptr(),
                                     weight.data_ptr(), ws.data_ptr(), need, _st())
    assert rc == 0, lib.fr_last_error()
    assert f.intact()
    return sums.cpu().numpy(), weight.cpu().numpy()


def _check_sums(tag, got, ref):
    """the weight sums exact, NaN exactly where the reference has it, everything else within gamma_(n_g + 1) sum w |x|"""
    (sums, weight), (rsums, rweight, absw, sizes) = got, ref
    assert np.array_equal(weight, rweight), f"{tag}: weight sums differ"
    assert np.array_equal(np.isnan(sums), np.isnan(rsums)), f"{tag}: NaN positions differ"
    fin = ~np.isnan(rsums)
    bound = BR.sums_tolerance(np.where(fin, absw, 0.0), sizes)
    return _within(tag, sums[fin], rsums[fin], bound[fin])


@functools.lru_cache(maxsize=None)
def _chunk_ref(shuffled):
    _, perm, start = GR.chunk_case(3, shuffled)
    values = BR.values_case(sum(GR.CHUNK_SIZES), 3)
    return values, perm, start, BR.group_sums_ref(values, perm, start, 5, SEED)


@pytest.mark.parametrize("shuffled", [False, True])
def test_sums_at_the_chunk_edges(shuffled):
    values, perm, start, ref = _chunk_ref(shuffled)
    assert ref[3].tolist() == GR.CHUNK_SIZES and (perm is None) == (not shuffled)
    _check_sums(f"bootstrap sizes 1/63/64/65/129 perm={'sort' if shuffled else 'NULL'}", _boot(values, perm, start, 5), ref)


def test_chunks_of_two_row_tiles():
    """131 073 rows: chunks of 128 positions, each two LDS row tiles; groups of CH - 1, CH, CH + 1, 2 CH + 1 rows and the rest"""
    U = BR.LONG_ROWS
    assert BR.chunk_len(U) == 2 * BR.ROW_TILE == 128 and BR.chunk_len(U - 1) == 64
    sizes = BR.LONG_SIZES + [U - sum(BR.LONG_SIZES)]
    start = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    values = BR.values_case(U, 1)
    ref = BR.group_sums_ref(values, None, start, 2, SEED)
    _check_sums("bootstrap 131073 rows, sizes 127/128/129/257/rest", _boot(values, None, start, 2), ref)
    # the same rows through a permutation that reverses every group
    perm = np.concatenate([np.arange(start[g], start[g + 1])[::-1] for g in range(len(sizes))]).astype(np.int64)
    got = _boot(values, perm, start, 2)
    assert np.array_equal(got[1], ref[1])
    _check_sums("bootstrap 131073 rows, every group reversed", got, ref)


@pytest.mark.parametrize("n_rep", BR.N_REPS)
def test_replicate_counts(n_rep):
    values = BR.values_case(70, 2)
    perm, start = GR.segments(GR.assignment(70, 2), 2)
    got = _boot(values, perm, start, n_rep)
    _check_sums(f"bootstrap B={n_rep}", got, BR.group_sums_ref(values, perm, start, n_rep, SEED))
    # sum_g out_weight[g][b] = the column sums of the reference's weights over all rows
    assert got[1].sum(axis=0).tolist() == BR.weights(np.arange(70), n_rep, SEED).sum(axis=0).tolist()


@pytest.mark.parametrize("n_cols", BR.N_COLS)
def test_column_counts(n_cols):
    values = BR.values_case(70, n_cols)
    perm, start = GR.segments(GR.assignment(70, 2), 2)
    ref = BR.group_sums_ref(values, perm, start, 5, SEED)
    _check_sums(f"bootstrap C={n_cols}", _boot(values, perm, start, 5), ref)
    if n_cols == 9:
        wide = np.concatenate((values, np.full((70, 3), np.nan)), axis=1)          # ld = n_cols + 3: the padding is never read
        _check_sums("bootstrap C=9, ld=12", _boot(wide, perm, start, 5, n_cols=9), ref)


@pytest.mark.parametrize("G,U", BR.GROUP_COUNTS)
def test_group_counts(G, U):
    values = BR.values_case(U, 3)
    perm, start = GR.segments(GR.assignment(U, G), G)
    got = _boot(values, perm, start, 7)
    _check_sums(f"bootstrap G={G} U={U}", got, BR.group_sums_ref(values, perm, start, 7, SEED))
    if G == 70:
        assert (np.diff(start) == 1).all() and (got[0][got[1] == 0] == 0).all() and (got[1] == 0).any()


def test_empty_groups_give_zeros():
    values = BR.values_case(65, 2)
    start = np.array([0, 0, 64, 64, 65, 65], dtype=np.int64)
    got = _boot(values, None, start, 5)
    assert (got[0][[0, 2, 4]] == 0).all() and (got[1][[0, 2, 4]] == 0).all()
    _check_sums("bootstrap with empty groups first, middle and last", got, BR.group_sums_ref(values, None, start, 5, SEED))


def test_a_nan_value_makes_its_group_and_column_nan_in_every_replicate():
    values = BR.values_case(90, 3)
    values[40, 1] = np.nan
    gidx = np.arange(90) // 30
    for perm, start in ((None, np.array([0, 30, 60, 90], dtype=np.int64)), GR.segments(gidx, 3)):
        ref = BR.group_sums_ref(values, perm, start, 9, SEED)
        assert np.isnan(ref[0][1, :, 1]).all() and np.isnan(ref[0]).sum() == 9
        assert (BR.weights([40], 9, SEED) == 0).any()                  # w = 0 enters the sum as well: 0 * NaN
        _check_sums("bootstrap with one NaN value", _boot(values, perm, start, 9), ref)


def test_malformed_tables_stay_inside_the_inputs():
    """group_start beyond n_rows / descending and perm entries outside [0, n_rows): unspecified values, frames intact"""
    values = BR.values_case(70, 4)
    perm = np.arange(70, dtype=np.int64)
    perm[[3, 40]] = (-5, 10 ** 12)
    for start in ([0, 500, 20, 70], [-9, 10, 10 ** 15, 70], [60, 0, 0, 0]):
        _boot(values, perm, np.array(start, dtype=np.int64), 5)


def test_seeds_and_reproducibility():
    values, perm, start, _ = _chunk_ref(True)
    a, b = _boot(values, perm, start, 5), _boot(values, perm, start, 5)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    other = (7 << 32) | 5                                               # both key words in use
    c = _boot(values, perm, start, 5, seed=other)
    assert not np.array_equal(a[1], c[1])
    _check_sums("bootstrap with a 64-bit seed", c, BR.group_sums_ref(values, perm, start, 5, other))


def test_refined_groups_add_up():
    """the weights belong to the rows: 6 groups that refine 2 give weight sums that add up exactly and sums within both bounds"""
    U = 200
    values = BR.values_case(U, 3)
    fine = GR.assignment(U, 6)
    coarse = fine // 3
    got2 = _boot(values, *GR.segments(coarse, 2), 9)
    got6 = _boot(values, *GR.segments(fine, 6), 9)
    ref2 = BR.group_sums_ref(values, *GR.segments(coarse, 2), 9, SEED)
    ref6 = BR.group_sums_ref(values, *GR.segments(fine, 6), 9, SEED)
    assert np.array_equal(got6[1].reshape(2, 3, 9).sum(axis=1), got2[1])
    assert got2[1].sum(axis=0).tolist() == BR.weights(np.arange(U), 9, SEED).sum(axis=0).tolist()
    both = BR.sums_tolerance(ref2[2], ref2[3]) + BR.sums_tolerance(ref6[2], ref6[3]).reshape(2, 3, 9, 3).sum(axis=1)
    # (the test's own two additions per cell: gamma_2 of the sum of magnitudes)
    _within("6 refined groups added up against their 2 groups", got6[0].reshape(2, 3, 9, 3).sum(axis=1), got2[0],
            both + R.gamma(2) * ref2[2])


# ---- fr_topk_user_terms, fr_gauc_user_terms ------------------------------------------------------------------------------------------

def _user_terms(rec, columns):
    import ctypes
    U, K, C = rec.shape[0], rec.shape[1] - 1, len(columns)
    lib, f = _lib(), _Frames()
    out = f.new(torch.float64, U, C)
    rec_ = _dev(rec)
    rc = lib.fr_topk_user_terms(rec_.data_ptr(), U, K, (ctypes.c_int32 * C)(*[BR.TOPK_NAMES.index(m) for m, _ in columns]),
                                (ctypes.c_int32 * C)(*[k for _, k in columns]), C, out.data_ptr(), _st())
    assert rc == 0, lib.fr_last_error()
    assert f.intact()
    return out.cpu()


def _rows_through_topk_metrics(rec, columns):
    """[U, C]: fr_topk_metrics applied to every row on its own (a mean over one row is exact)"""
    out = torch.empty((rec.shape[0], len(columns)), dtype=torch.float64)
    for u in range(rec.shape[0]):
        one = _topk(rec[u:u + 1])
        out[u] = torch.stack([one[BR.TOPK_NAMES.index(m), k - 1] for m, k in columns])
    return out


def test_topk_user_terms_are_fr_topk_metrics_of_one_row_byte_for_byte():
    rec = R.topk_case(200, 20, zero_positive_row=40)
    columns = [(m, k) for k in (1, 5, 20) for m in BR.TOPK_NAMES]
    got = _user_terms(rec, columns)
    assert _bytes(got) == _bytes(_rows_through_topk_metrics(rec, columns))
    row = got[40].numpy().reshape(3, 6)
    assert np.isnan(row[:, 3]).all() and (row[:, [2, 5]] == 0).all() and np.isfinite(row[:, [0, 1, 2, 4, 5]]).all()
    ref = BR.topk_user_terms_ref(rec, columns)
    fin = ~np.isnan(ref)
    assert np.array_equal(np.isnan(got.numpy()), ~fin)
    _within("topk_user_terms against the exact per-row terms", got.numpy()[fin], ref[fin], R.topk_tolerance(ref, 1, 20)[fin])
    # the Python wrapper: the same launch, the same bits
    from fairrec.evaluator import topk_user_terms
    assert _bytes(topk_user_terms(_dev(rec), columns)) == _bytes(got)


@pytest.mark.parametrize("K", [1, 255])
def test_topk_user_terms_smallest_and_largest_k(K):
    rec = R.topk_case(10, K)
    columns = [(m, k) for k in sorted({1, K}) for m in BR.TOPK_NAMES]
    assert _bytes(_user_terms(rec, columns)) == _bytes(_rows_through_topk_metrics(rec, columns))


def test_gauc_user_terms_are_fr_gauc_grouped_with_singleton_groups_byte_for_byte():
    U = 130
    t = GR.meanrank_case(U)
    t[10] = (0, 33, 0)                       # no positive
    t[70] = (42, 6, 6)                       # no negative
    lib, f = _lib(), _Frames()
    out = f.new(torch.float64, U, 2)
    t_ = _dev(t)
    rc = lib.fr_gauc_user_terms(t_.data_ptr(), U, out.data_ptr(), _st())
    assert rc == 0 and f.intact()
    single, kept = GMH._gauc(t, None, np.arange(U + 1, dtype=np.int64))
    assert _bytes(out) == single.tobytes() and (out[10] == 0).all() and (out[70] == 0).all() and kept[:, 0].sum() == U - 2
    ref = BR.gauc_user_terms_ref(t)
    _within("gauc_user_terms against the exact rationals", out.cpu().numpy(), ref, 3 * U64 * ref)
    from fairrec.evaluator import gauc_user_terms
    assert _bytes(gauc_user_terms(t_)) == _bytes(out)


# ---- the Python wrappers and the intervals ---------------------------------------------------------------------------------------------

def _stat_bound(stat, sizes, per_row):
    """[G, B]: gamma_(per_row(n_g)) |stat| per replicate, 0 where the statistic is unusable"""
    rel = np.array([R.gamma(per_row(int(n))) for n in sizes])[:, None]
    return np.where(np.isfinite(stat), rel * np.abs(np.where(np.isfinite(stat), stat, 0.0)), 0.0)


def _interval_bounds(want, bound):
    """(bound of every group's two quantiles [G], of the gap's): the largest replicate bound of the group plus 2 u |q|; the gap's
    the two largest groups' together"""
    per_group = bound.max(axis=1)
    q = np.nan_to_num(np.maximum(np.abs(want[0]), np.abs(want[1])))
    two = np.sort(per_group)[-2:].sum() if len(per_group) > 1 else per_group.sum()
    gq = max(abs(np.nan_to_num(want[2])), abs(np.nan_to_num(want[3])))
    return per_group + 2 * U64 * q, two + 2 * U64 * gq


def test_wrappers_and_intervals_with_dropped_replicates(caplog):
    """sizes 1 / 63 / 64 / 65 / 129 with seed 2020 and B = 200: the one-row group is unusable in 66 replicates (weight 0), above
    the B / 2 threshold -- 134 usable, and the gap with it; two groups of one row share 78 usable replicates, below it: the gap's
    interval is NaN with a warning, the groups' own (134 and 119 usable) are not"""
    from fairrec.evaluator import bootstrap_group_sums, bootstrap_intervals
    B = 200
    n = sum(GR.CHUNK_SIZES)
    values = np.abs(BR.values_case(n, 70))                             # 70 columns: two library calls
    gidx = np.repeat(np.arange(5), GR.CHUNK_SIZES)
    perm, start = GR.segments(gidx, 5)
    sums, weight = bootstrap_group_sums(_dev(values), _dev(gidx), 5, B, SEED)
    assert sums.shape == (5, B, 70) and weight.shape == (5, B)
    for c in (0, 63, 64, 69):
        ref = BR.group_sums_ref(values[:, c:c + 1], perm, start, B, SEED)
        _check_sums(f"evaluator.bootstrap_group_sums, column {c} of 70", (sums[:, :, c:c + 1].cpu().numpy(), weight.cpu().numpy()), ref)
    rstat = BR.replicate_stats(ref[0][:, :, 0], ref[1])
    want = BR.intervals_ref(rstat, 0.95)
    assert want[4].tolist() == [134, 200, 200, 200, 200] and want[5] == 134
    from fairrec.evaluator.metrics import _ratio
    stat = _ratio(sums[:, :, 69].cpu().numpy(), weight.cpu().numpy())
    assert np.array_equal(np.isfinite(stat), np.isfinite(rstat))
    with caplog.at_level(logging.WARNING):
        got = bootstrap_intervals(stat, 0.95, "a column of sensitive attribute sizes")
    assert not caplog.records and got[4].tolist() == want[4].tolist() and got[5] == want[5]
    gb, gapb = _interval_bounds(want, _stat_bound(rstat, ref[3], lambda n_g: n_g + 2))
    _within("intervals with 134 of 200 usable replicates", np.concatenate((got[0], got[1], [got[2], got[3]])),
            np.concatenate((want[0], want[1], [want[2], want[3]])), np.concatenate((gb, gb, [gapb, gapb])))
    # two groups of one row each
    two = np.array([0, 1], dtype=np.int64)
    sums, weight = bootstrap_group_sums(_dev(values[:2, :1]), _dev(two), 2, B, SEED)
    ref = BR.group_sums_ref(values[:2, :1], *GR.segments(two, 2), B, SEED)
    _check_sums("two groups of one row", (sums.cpu().numpy(), weight.cpu().numpy()), ref)
    want = BR.intervals_ref(BR.replicate_stats(ref[0][:, :, 0], ref[1]), 0.95)
    assert want[4].tolist() == [134, 119] and want[5] == 78
    with caplog.at_level(logging.WARNING):
        got = bootstrap_intervals(_ratio(sums[:, :, 0].cpu().numpy(), weight.cpu().numpy()), 0.95, "x of sensitive attribute pair")
    assert got[4].tolist() == [134, 119] and got[5] == 78 and math.isnan(got[2]) and math.isnan(got[3])
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    warned = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warned) == 1 and "x of sensitive attribute pair" in warned[0] and "the gap (78)" in warned[0]


# ---- through the Evaluator: the 40-user x 71-item FOCF model ----------------------------------------------------------------------------

B_EVAL = 200
ON = dict(utility_by_group=True, group_bootstrap=B_EVAL)
# usable gap replicates of the reference with seed 2020 and B = 200 on the 39 collected rows, top-k columns: the users' weights alone
# decide them (the six intersection groups keep 200 / 196 / 200 / 198 / 200 / 196 replicates each)
GAP_USABLE = {"gender": 200, "age": 200, "gender&age": 191}


def _check_ci(res, collected, topk, names, with_gauc, tag):
    """every ci_ key against tests/bootstrap_ref.py on the collected arrays; the usable sets against the device's own sums"""
    from fairrec.evaluator import bootstrap_group_sums, gauc_user_terms, topk_user_terms
    from fairrec.evaluator.metrics import _ratio
    rec = collected["rec.topk"].cpu().numpy()
    columns = [(m, k) for m in BR.TOPK_NAMES if m in names for k in topk]
    terms = BR.topk_user_terms_ref(rec, columns)
    assert np.isfinite(terms).all() and (terms >= 0).all()
    stats = {f"{m}@{k}": (j, None) for j, (m, k) in enumerate(columns)}
    dev_values = topk_user_terms(collected["rec.topk"], columns)
    if with_gauc:
        g = BR.gauc_user_terms_ref(collected["rec.meanrank"].cpu().numpy())
        stats["gauc"] = (terms.shape[1], terms.shape[1] + 1)
        terms = np.concatenate((terms, g), axis=1)
        dev_values = torch.cat((dev_values, gauc_user_terms(collected["rec.meanrank"])), dim=1)
    got, want, bound, expected, gap_usable = [], [], [], set(), {}
    for attr, (gidx, labels) in _host_groups(collected).items():
        G = len(labels)
        perm, start = GR.segments(gidx, G)
        rsums, rweight, _, sizes = BR.group_sums_ref(terms, perm, start, B_EVAL, SEED, with_abs=False)
        dsums, dweight = (t.cpu().numpy() for t in bootstrap_group_sums(dev_values, _dev(gidx), G, B_EVAL, SEED))
        assert np.array_equal(dweight, rweight), attr
        for m, (num, den) in stats.items():
            rstat = BR.replicate_stats(rsums[:, :, num], rweight if den is None else rsums[:, :, den])
            dstat = _ratio(dsums[:, :, num], dweight if den is None else dsums[:, :, den])
            assert np.array_equal(np.isfinite(dstat), np.isfinite(rstat)), (attr, m)          # the usable sets, exactly
            ref = BR.intervals_ref(rstat, 0.95)
            print(f"{tag}: {m} of {attr}: usable per group {ref[4].tolist()}, gap {ref[5]}")
            if den is None:
                assert (ref[4] >= ref[5]).all() and gap_usable.setdefault(attr, ref[5]) == ref[5], (attr, m, ref[4], ref[5])
            assert 2 * ref[5] >= B_EVAL and np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all(), (attr, m)
            gb, gapb = _interval_bounds(ref, _stat_bound(rstat, sizes, (lambda n: n + 2) if den is None else (lambda n: 2 * n + 6)))
            for g, lab in enumerate(labels):
                got += [res[f"{m} ci_low of {attr}={lab}"], res[f"{m} ci_high of {attr}={lab}"]]
                want += [ref[0][g], ref[1][g]]
                bound += [gb[g] + GMH.ROUND] * 2
                expected |= {f"{m} ci_low of {attr}={lab}", f"{m} ci_high of {attr}={lab}"}
            got += [res[f"{m} gap ci_low of sensitive attribute {attr}"], res[f"{m} gap ci_high of sensitive attribute {attr}"]]
            want += [ref[2], ref[3]]
            bound += [gapb + GMH.ROUND] * 2
            expected |= {f"{m} gap ci_low of sensitive attribute {attr}", f"{m} gap ci_high of sensitive attribute {attr}"}
            # (a percentile interval need not hold the point estimate; it is ordered)
            assert all(res[f"{m} ci_low of {attr}={lab}"] <= res[f"{m} ci_high of {attr}={lab}"] for lab in labels)
    assert {k for k in res if "ci_" in k} == expected
    _within(tag, got, want, bound)
    assert gap_usable == GAP_USABLE, gap_usable


def _without_ci(res):
    return {k: repr(v) for k, v in res.items() if "ci_" not in k}


def test_full_evaluation_with_intervals_matrix_and_fused(tmp_path_factory, monkeypatch):
    trainer, loader = _run("full", tmp_path_factory, **GMH.FULL)
    assert trainer.config["seed"] == SEED and trainer.config["group_bootstrap"] is None
    monkeypatch.setattr(trainer, "full_sort_eval", "matrix")
    matrix, collected = _evaluate(trainer, loader, monkeypatch, **ON)
    monkeypatch.setattr(trainer, "full_sort_eval", "fused")
    fused, collected_f = _evaluate(trainer, loader, monkeypatch, **ON)
    assert torch.equal(collected["rec.topk"], collected_f["rec.topk"])
    ci = {k: repr(v) for k, v in matrix.items() if "ci_" in k}
    assert ci and ci == {k: repr(v) for k, v in fused.items() if "ci_" in k}
    assert collected["rec.topk"].shape[0] > 30
    names = [n.lower() for n in GMH.TOPK_NAMES]
    _check_ci(fused, collected_f, [5, 10], names, True, "Evaluator intervals, full mode")
    assert "ndcg@10 ci_low of gender=1" in fused and "gauc ci_high of gender&age=0&18" in fused
    assert "ndcg@10 gap ci_high of sensitive attribute age" in fused
    # the key unset (and 0): the result of the same call without the interval keys, key for key and bit for bit, and no other
    # collected array
    for value in (None, 0):
        off, collected_off = _evaluate(trainer, loader, monkeypatch, utility_by_group=True, group_bootstrap=value)
        assert {k: repr(v) for k, v in off.items()} == _without_ci(fused) and not any("ci_" in k for k in off)
        assert set(collected_off) == set(collected_f)
    # another level: other intervals from the same replicates; the 0.5 interval lies inside the 0.95 one
    half, _ = _evaluate(trainer, loader, monkeypatch, group_bootstrap_level=0.5, **ON)
    assert _without_ci(half) == _without_ci(fused)
    assert fused["ndcg@10 ci_low of age=35"] <= half["ndcg@10 ci_low of age=35"] <= half["ndcg@10 ci_high of age=35"] \
        <= fused["ndcg@10 ci_high of age=35"]
    # a list selects its names
    only, _ = _evaluate(trainer, loader, monkeypatch, utility_by_group=["age"], group_bootstrap=B_EVAL)
    assert "ndcg@10 ci_low of age=35" in only and not any("of gender=" in k or "gender&age" in k for k in only if "ci_" in k)
    assert all(repr(only[k]) == repr(fused[k]) for k in only)


def test_uni_evaluation_with_intervals(tmp_path_factory, monkeypatch):
    trainer, loader = _run("uni5", tmp_path_factory, metrics=["NDCG", "Recall", "GAUC"], topk=[10], valid_metric="ndcg@10")
    res, collected = _evaluate(trainer, loader, monkeypatch, topk=[5, 10], **ON)
    assert collected["rec.topk"].shape[0] > 30 and collected["rec.topk"].shape[1] == 11
    _check_ci(res, collected, [5, 10], ["ndcg", "recall"], True, "Evaluator intervals, uni5")
    # (every uni5 evaluation draws its own negatives, so two calls are not compared; the full-mode test compares the key set and
    # unset on the same lists)
    per_group = [k for k in res if "=" in k and "ci_" not in k]
    assert len(per_group) == 5 * (2 + 3 + 6) and all(k.replace(" of ", " ci_low of ", 1) in res for k in per_group)

"""CPU: the references of tests/metrics_ref.py against oracle/metrics.py -- on every metrics golden and on the edge inputs that
tests/test_metrics_kernels_hip.py feeds the kernels, wherever the oracle is defined -- before anything runs on a GPU.  The two
places where a reference (and the kernel) differs from the oracle on purpose are asserted as such: the Recall / NDCG of a row
with zero positives, and DifferentialFairness with a non-positive table entry.

The oracle takes the same float64 steps in another order (np.cumsum, np.mean), so the rational and float64 metrics agree to
1e-13 relative; its DifferentialFairness takes float32 logarithms, which is what bound[4] of fair_from_stats_ref describes
with numpy's own measured logf error put in for the device's.
"""
import glob
import json
import math
import os

import numpy as np
import pytest

import metrics_ref as R
from oracle import metrics as OM

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CASES = sorted(glob.glob(os.path.join(GOLDEN, "metrics_*.npz")))
NAMES = ("hit", "mrr", "ndcg", "recall", "precision", "map")
REL = 1e-13


def _oracle_topk(rec):
    K = rec.shape[1] - 1
    with np.errstate(invalid="ignore", divide="ignore"):
        d = OM.topk_metrics(rec, range(1, K + 1))
    return np.array([[d[f"{n}@{k}"] for k in range(1, K + 1)] for n in NAMES])


def _close(got, ref, rel=REL):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return bool((np.abs(got - ref) <= rel * np.abs(ref)).all())


def _f32_mean_slack(K, mean):
    """the oracle averages its float32 epsilons in float32 (pairwise): log2(K) + 2 roundings of v"""
    return R.gamma(math.ceil(math.log2(max(K, 2))) + 2, R.V32) * mean


def test_there_are_goldens():
    assert len(CASES) >= 5


@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p)[8:-4] for p in CASES])
def test_references_match_the_oracle_on_the_goldens(path):
    z = np.load(path)
    assert _close(R.topk_metrics_ref(z["rec_topk"]), _oracle_topk(z["rec_topk"]))
    sst = ["gender"] + (["age"] if "age" in z.files else [])
    mode = str(z["mode"])
    neg = (None, None) if mode == "full" else (z["neg_score"], z["neg_i"])
    ulp = R.logf_ulp_of_numpy(np.concatenate([R.df_table(_tables(z, s)).ravel() for s in sst]))
    got, bnd = R.fairness_ref(z["pos_score"], z["pos_i"], {s: z[s] for s in sst}, neg[0], neg[1], mode, logf_ulp=ulp)
    want = OM.all_metrics(z, [1], mode, sst)
    golden = json.loads(str(z["result_json"]))
    for key, v in got.items():
        if "Unfairness" in key and "NonParity" not in key and len(sst) > 1:
            continue        # the reference's classes, the oracle and the goldens have them for a single attribute only
        slack = _f32_mean_slack(len(np.unique(z["pos_i"])), v) if "Differential" in key else 0.0
        if "NonParity" in key:      # the oracle's group means are float32 (np.mean of the float32 scores)
            slack = R.gamma(24, R.V32) * 1.0
        assert abs(v - want[key]) <= bnd[key] + slack + REL * abs(v), (key, v, want[key], bnd[key])
        # the golden was written by the reference's own classes, rounded to ten decimal places
        assert abs(v - golden[key]) <= bnd[key] + slack + REL * abs(v) + 1e-10, (key, v, golden[key])


def _tables(z, s):
    vals, gidx = np.unique(z[s], return_inverse=True)
    order = np.argsort(z["pos_i"], kind="stable")
    seg = np.concatenate(([0], np.cumsum(np.unique(z["pos_i"], return_counts=True)[1])))
    return R.group_sums_ref(order, seg, gidx, z["pos_score"], None, len(vals))[0]


# ---- fr_topk_metrics' edge inputs ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("U,K", R.TOPK_SHAPES)
def test_topk_reference_matches_the_oracle_on_the_edge_rows(U, K):
    rec = R.topk_case(U, K)
    ref = R.topk_metrics_ref(rec)
    assert np.isfinite(ref).all() and _close(ref, _oracle_topk(rec))


def test_topk_case_holds_every_row_kind():
    rec = R.topk_case(65, 20)
    assert rec[0, :20].all() and rec[0, 20] == 1
    body, pos = rec[1:, :20], rec[1:, 20]
    assert (~body.any(axis=1)).any()                                           # no hit
    assert ((body[:, 19] != 0) & (body[:, :19] == 0).all(axis=1)).any()        # a hit only at rank K
    assert (body.all(axis=1) & (pos == 20)).any()                              # every rank a hit, pos_len == K
    assert (pos == 1).any() and (pos == 25).any() and (pos == 10 ** 6).any()
    assert ((body != 0) & (body != 1)).any()                                   # hit flags other than 1
    assert (pos >= 1).all()


def test_zero_positive_row_difference_from_the_oracle_is_recall_only():
    """One row of three has zero positives.  Oracle and reference agree: NDCG of that row is 0 (the wrapped idcg index), MAP 0,
    Recall NaN.  Before the kernel's fix its NDCG was 0 / 0 = NaN; that is the difference this case is here for."""
    rec = R.topk_case(3, 20, zero_positive_row=1)
    assert not rec[1].any()
    ref, ora = R.topk_metrics_ref(rec), _oracle_topk(rec)
    assert np.isnan(ref[3]).all() and np.isnan(ora[3]).all()
    rows = [0, 1, 2, 4, 5]
    assert np.isfinite(ref[rows]).all() and _close(ref[rows], ora[rows])
    # the row contributes 0 to NDCG and MAP: the means are 2/3 of the means without it
    two = R.topk_metrics_ref(rec[[0, 2]])
    assert _close(ref[[2, 5]], two[[2, 5]] * 2 / 3, 1e-15 * 4)
    one = R.topk_metrics_ref(rec[[1]])
    assert (one[[0, 1, 2, 4, 5]] == 0).all() and np.isnan(one[3]).all()


# ---- fr_eval_hits ------------------------------------------------------------------------------------------------------------------

def _collector_rec_topk(idx, n_items, pos_u, pos_i):
    """collector.py:146-154 in numpy: gather the dense 0/1 matrix at the list, append the row sums"""
    dense = np.zeros((idx.shape[0], n_items), dtype=np.int64)
    dense[pos_u, pos_i] = 1
    return np.concatenate((np.take_along_axis(dense, idx, axis=1), dense.sum(axis=1, keepdims=True)), axis=1)


@pytest.mark.parametrize("U,K", R.HITS_SHAPES)
def test_eval_hits_reference_is_the_dense_gather(U, K):
    for n_items in R.HITS_ITEMS:
        for kind in R.HITS_NPOS:
            idx, pu, pi = R.eval_hits_case(U, K, n_items, kind)
            ref = R.eval_hits_ref(idx, n_items, pu, pi)
            assert np.array_equal(ref, _collector_rec_topk(idx, n_items, np.array(pu, dtype=np.int64), np.array(pi, dtype=np.int64)))
            assert len(set(zip(pu, pi))) == len(pu) == {"none": 0, "one": 1}.get(kind, len(pu))
            keys = R.pos_keys(n_items, pu, pi)
            assert (np.diff(keys) > 0).all()
            if kind == "many" and U >= 6:
                assert ref[0, K] == 0 and ref[U - 1, K] == 0 and (ref[1, :K] == 1).all()
            if kind in ("two", "many") and U >= 2 and n_items >= 2:
                assert (keys[1:] - keys[:-1] == 1).any()         # positives at n_items - 1 and 0 of neighbouring rows


def test_eval_hits_reference_sparse_form_is_the_dense_one(monkeypatch):
    idx, pu, pi = R.eval_hits_case(51, 4, 1000, "many")
    dense = R.eval_hits_ref(idx, 1000, pu, pi)
    monkeypatch.setattr(R, "DENSE_CELLS", 0)
    assert np.array_equal(R.eval_hits_ref(idx, 1000, pu, pi), dense) and dense[:, :4].any()
    big = 2 ** 40
    idx, pu, pi = R.eval_hits_case(4, 5, big, "many")
    ref = R.eval_hits_ref(idx, big, pu, pi)
    assert ref[:, :5].any() and int(R.pos_keys(big, pu, pi).max()) > 2 ** 41


def test_eval_hits_out_of_range_entries_are_no_hits():
    idx, n_items, pu, pi, want = R.eval_hits_alias_case()
    assert np.array_equal(R.eval_hits_ref(idx, n_items, pu, pi), want)
    keys = set(R.pos_keys(n_items, pu, pi).tolist())
    aliased = [(u, k) for u in range(3) for k in range(4)
               if not 0 <= idx[u, k] < n_items and u * n_items + int(idx[u, k]) in keys]
    assert len(aliased) >= 4 and all(want[u, k] == 0 for u, k in aliased)


# ---- fr_group_sums -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_segments", R.SEG_COUNTS)
def test_group_sums_reference_matches_add_at(n_segments):
    """np.add.at is what the oracle builds its tables with; float64 sums in member order, so within gamma_L of the fsum"""
    for gi, G in enumerate(R.GROUPS):
        for vi, kind in enumerate(R.VALUE_KINDS):
            perm, seg, group, value, wtrue = R.group_sums_case(n_segments, G, kind, vi % 2 == 1, R.WTRUE_KINDS[(vi + gi) % 3])
            st, absv, abst = R.group_sums_ref(perm, seg, group, value, wtrue, G)
            rows = perm if perm is not None else np.arange(seg[-1])
            k_of = np.repeat(np.arange(n_segments), np.diff(seg))
            g_of = group[rows]
            ok = (g_of >= 0) & (g_of < G)
            want = np.zeros((n_segments, G, 3))
            np.add.at(want[:, :, 0], (k_of[ok], g_of[ok]), value[rows][ok].astype(np.float64))
            np.add.at(want[:, :, 1], (k_of[ok], g_of[ok]), 1.0)
            if wtrue is not None:
                np.add.at(want[:, :, 2], (k_of[ok], g_of[ok]), wtrue[rows][ok].astype(np.float64))
            assert np.array_equal(st[:, :, 1], want[:, :, 1])
            lim = np.vectorize(lambda L: R.gamma(L + 1))(st[:, :, 1])
            assert (np.abs(st[:, :, 0] - want[:, :, 0]) <= lim * absv).all()
            assert (np.abs(st[:, :, 2] - want[:, :, 2]) <= lim * abst).all()
            assert (~ok).any() and (st[1:, :, 1].sum(axis=1) <= np.diff(seg)[1:]).all()
            if n_segments > 1:
                assert (st[1] == 0).all()                     # the empty segment
            if G > 1 and n_segments > 2:
                assert (st[2, :, 1] == 0).sum() >= G - 1      # one member: the other groups are (0, 0, 0)


def test_adversarial_values_defeat_float32_accumulation():
    """what makes the `cancel` and `big` sets worth having: a float32 accumulator misses the derived bound on them by orders
    of magnitude (so a kernel that accumulated in float32 fails the GPU test), float64 in member order does not"""
    for kind in ("cancel", "big"):
        perm, seg, group, value, wtrue = R.group_sums_case(1, 1, kind, False, "null")
        st, absv, _ = R.group_sums_ref(perm, seg, group, value, wtrue, 1)
        mine = value[group == 0]
        acc32 = np.float32(0)
        for x in mine:
            acc32 = np.float32(acc32 + x)
        tol = float(R.group_sums_tolerance(absv, st[:, :, 1])[0, 0])
        assert abs(float(acc32) - st[0, 0, 0]) > 1e3 * tol
        assert abs(float(np.sum(mine.astype(np.float64))) - st[0, 0, 0]) <= R.gamma(len(mine)) * absv[0, 0]


# ---- fr_fair_metrics_from_stats ----------------------------------------------------------------------------------------------------

def _oracle_from_stats(st):
    """the oracle's formulas (value_type_unfairness, differential_fairness) on ready tables"""
    K, G = st.shape[:2]
    out = np.zeros(5)
    if G == 2:
        num = st[:, :, 1] + 1e-5
        pred, true = st[:, :, 0] / num, st[:, :, 2] / num
        for q, d in enumerate((pred - true, np.abs(pred - true), np.where(true - pred > 0, true - pred, 0),
                               np.where(pred - true > 0, pred - true, 0))):
            out[q] = float(np.mean(np.abs(d[:, 0] - d[:, 1])))
    table = ((st[:, :, 0] + 1.0 / K) / (st[:, :, 1] + 1.0)).astype(np.float32)
    eps = np.zeros(K, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        for i in range(G):
            for j in range(i + 1, G):
                eps = np.maximum(eps, np.abs(np.log(table[:, i]) - np.log(table[:, j])))
    out[4] = float(eps.mean())
    return out


@pytest.mark.parametrize("K", R.STATS_ITEMS)
def test_fair_reference_matches_the_oracle_formulas(K):
    for G in R.GROUPS:
        st = R.stats_case(K, G)
        table = R.df_table(st)
        ulp = R.logf_ulp_of_numpy(table)
        out, bound = R.fair_from_stats_ref(st, G, logf_ulp=ulp)
        ora = _oracle_from_stats(st)
        assert np.isfinite(out).all()
        if G == 2:
            assert (out[:4] > 0).all() or K < 8
            assert (np.abs(out[:4] - ora[:4]) <= bound[:4]).all()
        else:
            assert (out[:4] == 0).all() and (bound[:4] == 0).all()
        if G == 1:
            assert out[4] == 0.0 and bound[4] == 0.0 and ora[4] == 0.0
        else:
            assert abs(out[4] - ora[4]) <= bound[4] + _f32_mean_slack(K, out[4]), (out[4], ora[4], bound[4])
            assert bound[4] <= 1e-5 * out[4]
        if K >= 255:
            assert table.max() / table.min() > 1e6


def test_stats_case_takes_every_clamp_through_both_branches():
    st = R.stats_case(256, 2)
    n = st[:, :, 1] + 1e-5
    d = st[:, :, 0] / n - st[:, :, 2] / n
    for g in (0, 1):
        assert (d[:, g] > 0).any() and (d[:, g] < 0).any() and (d[:, g] == 0).any()
    assert {(a, b) for a, b in zip(d[:, 0] > 0, d[:, 1] > 0)} == {(False, False), (False, True), (True, False), (True, True)}
    assert (st[:, :, 1] == 0).any(axis=0).all() and (st[:, :, 1] == 1).all(axis=1).any()
    assert ((st[:, :, 0] == st[:, :, 2]) & (st[:, :, 1] > 0)).all(axis=1).any()


def test_nonpositive_table_entry_difference_from_the_oracle():
    """A negative score sum: the oracle's np.maximum carries the NaN logarithm into the mean; the reference, like the kernel,
    leaves the pairs with that entry out and stays finite."""
    st = R.stats_case_nonpositive()
    out, _ = R.fair_from_stats_ref(st, 3)
    assert math.isnan(_oracle_from_stats(st)[4]) and math.isfinite(out[4])
    table = R.df_table(st).astype(np.float64)
    item1 = abs(math.log(table[1, 0]) - math.log(table[1, 2]))
    others = [max(abs(math.log(table[k, i]) - math.log(table[k, j])) for i in range(3) for j in range(i + 1, 3)) for k in (0, 2)]
    assert out[4] == math.fsum([others[0], item1, others[1]]) / 3
    # ... and the same through oracle.metrics.differential_fairness on raw columns
    score = np.array([1.0, 1.0, -5.0, 2.0, 0.5], dtype=np.float32)
    with np.errstate(invalid="ignore"):
        assert math.isnan(OM.differential_fairness(score, np.array([1, 2, 2, 2, 1]), np.array([0, 0, 1, 2, 1])))


# ---- the chain ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("neg_len", [120, 300, 500])
def test_chain_reference_matches_the_oracle(neg_len):
    """negatives shorter than, as many as and longer than the positives: both sides of min(len(neg), P)"""
    z = R.chain_case(neg_len)
    assert len(np.unique(z["pos_i"])) == 40 and len(np.unique(z["age"])) == 3 and len(z["pos_score"]) == 300
    got, bnd = R.fairness_ref(z["pos_score"], z["pos_i"], {"gender": z["gender"], "age": z["age"]}, z["neg_score"], z["neg_i"],
                              "uni100", logf_ulp=4.0)
    want = {}
    for s in ("gender", "age"):
        want[f"NonParity Unfairness of sensitive attribute {s}"] = OM.nonparity(z["pos_score"], z[s])
        want[f"Differential Fairness of sensitive attribute {s}"] = OM.differential_fairness(z["pos_score"], z["pos_i"], z[s])
    for kind, label in (("value", "Value"), ("absolute", "Absolute"), ("under", "Underestimation"), ("over", "Overestimation")):
        want[f"{label} Unfairness of sensitive attribute gender"] = OM.value_type_unfairness(
            kind, z["pos_score"], z["pos_i"], z["neg_score"], z["neg_i"], z["gender"])
    assert set(got) == set(want)
    for key, v in want.items():
        slack = _f32_mean_slack(40, abs(v)) if "Differential" in key else R.gamma(24, R.V32) if "NonParity" in key else 0.0
        assert abs(got[key] - v) <= bnd[key] + slack + REL * abs(v), (key, got[key], v)

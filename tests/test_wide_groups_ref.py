"""CPU: the reference of tests/wide_groups_ref.py (DifferentialFairness from the sorted (item, group) cells, the group means
behind NonParity) against oracle/metrics.py on dense restatements of the cases tests/test_wide_groups_hip.py feeds the kernel,
before anything runs on a GPU; the max - min form of the epsilon against the pairwise form, bit for bit, where numpy computes
both; and the `sst_intersections` key of the Evaluator.

The oracle adds a cell's members one after the other in float64 (np.add.at: L additions for L members), takes numpy's float32
logarithms and averages its float32 epsilons in float32; the reference's bound with exactly those put in -- n_add(L) = L, e =
twice numpy's measured logf error, (log2(K) + 2) v of the mean -- is the tolerance.
"""
import math

import numpy as np
import pytest
import torch

import metrics_ref as R
import wide_groups_ref as W
from oracle import metrics as OM

ORACLE_GRID = [(n, G) for n in (1, 2, 17, 40) for G in (2, 9, 21, 65)] + [(16, 300)]


def _oracle_case(n_items, G):
    return W.cells_case(n_items, G, with_perm=(n_items + G) % 2 == 1, salt=n_items + G, empty_item=False)


@pytest.mark.parametrize("n_items,G", ORACLE_GRID)
def test_reference_is_the_oracle_differential_fairness(n_items, G):
    case = _oracle_case(n_items, G)
    ref = W.df_cells_ref(*case, G, W.logf_ulp(), n_add=lambda L: L)
    assert all(a > 0 for row in ref["table"] for a in row)
    assert all(len(item) >= 1 for item in ref["cells"]) and len(ref["cells"][0]) == G
    score, iids, sst = W.dense_restatement(*case)
    got = OM.differential_fairness(score, iids, sst)
    tol = ref["bound"] + (math.log2(n_items) + 2) * R.V32 * ref["mean"]
    print(f"K={n_items} G={G}: oracle {got!r}, reference {ref['mean']!r}, |difference| / tolerance "
          f"{abs(got - ref['mean']) / tol:.3g}")
    assert ref["mean"] > 0 and abs(got - ref["mean"]) <= tol


@pytest.mark.parametrize("n_items,G", ORACLE_GRID)
def test_max_minus_min_is_the_pairwise_maximum_bit_for_bit(n_items, G):
    ref = W.df_cells_ref(*_oracle_case(n_items, G), G)
    for row in ref["table"]:
        assert W.eps_maxmin_f32(row).tobytes() == W.eps_pairwise_f32(row).tobytes()


def test_max_minus_min_is_the_pairwise_maximum_with_non_positive_entries():
    """random float32 tables, negative entries and zeros among them: NaN logarithms are left out of both forms, -inf enters both"""
    rng = np.random.default_rng(5)
    for t in range(200):
        G = int(rng.integers(1, 12))
        row = (rng.standard_normal(G) * 10.0 ** rng.integers(-6, 7, G)).astype(np.float32)
        if t % 5 == 0:
            row = np.abs(row)
        if t % 7 == 0:
            row[rng.integers(0, G)] = 0.0
        a, b = W.eps_maxmin_f32(row), W.eps_pairwise_f32(row)
        assert a.tobytes() == b.tobytes() or (np.isnan(a) and np.isnan(b)), (row, a, b)


def test_reference_group_means_are_the_oracle_nonparity():
    for G in (9, 21, 300):
        perm, start, group, value = W.cells_case(17, G, with_perm=True, empty_item=False)
        score, _, sst = W.dense_restatement(perm, start, group, value)
        rows = perm[:int(start[-1])]
        means, _ = W.group_means_ref(group[rows], value[rows], G)
        ref = float(np.std(means))
        got = OM.nonparity(score, sst)
        assert ref > 0 and abs(got - ref) <= 1e-12 * float(np.abs(means).max()), (G, got, ref)


def test_negative_cell_the_oracle_is_nan_the_reference_finite():
    """the documented split (oracle/metrics.py differential_fairness): a negative score sum makes a table entry negative; numpy's
    maximum carries the NaN, the reference (and the kernel) leave that entry out"""
    case = W.cells_case(17, 9, with_perm=False, empty_item=False, negative_cell=True)
    ref = W.df_cells_ref(*case, 9, W.logf_ulp())
    assert sum(a < 0 for row in ref["table"] for a in row) == 1
    assert math.isfinite(ref["mean"]) and ref["mean"] > 0 and math.isfinite(ref["bound"])
    with np.errstate(invalid="ignore"):
        assert math.isnan(OM.differential_fairness(*W.dense_restatement(*case)))


def test_out_of_range_groups_form_no_cell():
    case = W.cells_case(17, 9, with_perm=True, bad_groups=True)
    perm, start, group, value = case
    assert (group == -1).any() and (group == 9).any()
    keep = (group >= 0) & (group < 9)
    cells = W.cells_ref(*case, 9)
    assert sum(c for item in cells for _, _, c, _ in item) == int(keep.sum())
    assert all(0 <= g < 9 for item in cells for g, _, _, _ in item)


def test_attribute_ref_is_the_oracle_on_the_chain_case():
    z = W.chain_case()
    for name, G in (("gender", 2), ("age", 7), ("occupation", 21)):
        vals, gidx = np.unique(z[name], return_inverse=True)
        assert len(vals) == G
        nonparity, _, df, bound = W.attribute_ref(z["pos_score"], z["pos_i"], gidx, G, W.logf_ulp(), n_add=lambda L: L)
        assert abs(OM.nonparity(z["pos_score"].astype(np.float64), z[name]) - nonparity) <= 1e-12
        got = OM.differential_fairness(z["pos_score"], z["pos_i"], z[name])
        assert abs(got - df) <= bound + (math.log2(40) + 2) * R.V32 * df, (name, got, df, bound)


# ---- the Evaluator's `sst_intersections` ------------------------------------------------------------------------------------------

def _evaluator(**extra):
    from fairrec.config import Config
    from fairrec.evaluator import Evaluator
    d = {"device": "cpu", "metrics": ["NDCG", "NonParityUnfairness", "DifferentialFairness"], "topk": [5],
         "sst_attr_list": ["gender", "age", "occupation"], "eval_args": {"mode": "full"}}
    d.update(extra)
    return Evaluator(Config(config_dict=d))


def test_evaluator_accepts_valid_intersections():
    assert _evaluator().intersections == []
    ev = _evaluator(sst_intersections=[["gender", "occupation"], ["gender", "age", "occupation"]])
    assert ev.intersections == [["gender", "occupation"], ["gender", "age", "occupation"]]


@pytest.mark.parametrize("bad", [[["gender", "zip"]], [["gender"]], [["gender", "gender"]], "gender&age", [["gender", "age"], "age"],
                                 [[]], [["gender", 3]]],
                         ids=["unknown-name", "one-name", "repeated-name", "not-a-list", "entry-not-a-list", "empty-entry",
                              "not-a-name"])
def test_evaluator_refuses_bad_intersections(bad):
    with pytest.raises(ValueError, match="sst_intersections"):
        _evaluator(sst_intersections=bad)


def _stub_fairness(monkeypatch):
    """fairness_metrics without a device: the keys it would report, and what it was called with"""
    from fairrec.evaluator import metrics as M
    calls = []

    def stub(pos_score, pos_i, sst, neg_score=None, neg_i=None, mode="full", value_type=True, **kw):
        calls.append(kw)
        names = list(sst) + ["&".join(e) for e in kw.get("intersections") or ()]
        return {f"{m} of sensitive attribute {n}": 0.5 for n in names for m in ("NonParity Unfairness", "Differential Fairness")}

    monkeypatch.setattr(M, "fairness_metrics", stub)
    return calls


def _collected():
    z = torch.zeros(4)
    return {"rec.positive_score": z, "data.positive_i": z.long(), "data.gender": z, "data.age": z, "data.occupation": z}


def test_without_the_key_an_evaluation_reports_todays_keys(monkeypatch):
    calls = _stub_fairness(monkeypatch)
    res = _evaluator(metrics=["NonParityUnfairness", "DifferentialFairness"]).evaluate(_collected())
    assert calls == [{}]                                   # fairness_metrics is called exactly as before
    assert sorted(res) == sorted(f"{m} of sensitive attribute {n}" for n in ("gender", "age", "occupation")
                                 for m in ("NonParity Unfairness", "Differential Fairness"))


def test_intersections_add_their_keys_for_the_requested_metrics_only(monkeypatch):
    calls = _stub_fairness(monkeypatch)
    both = [["gender", "occupation"]]
    res = _evaluator(metrics=["DifferentialFairness"], sst_intersections=both).evaluate(_collected())
    assert calls[-1] == {"intersections": both}
    assert sorted(res) == sorted(f"Differential Fairness of sensitive attribute {n}"
                                 for n in ("gender", "age", "occupation", "gender&occupation"))
    # neither of the two metrics requested: the key is ignored
    _evaluator(metrics=["ValueUnfairness"], sst_intersections=both).evaluate(_collected())
    assert calls[-1] == {}

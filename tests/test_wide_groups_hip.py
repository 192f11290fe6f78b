"""GPU: fr_df_cells (csrc/metrics.hip df_cells_kernel) -- DifferentialFairness for any number of groups from the sorted
(item, group) cells -- through the C ABI against the float64 reference of tests/wide_groups_ref.py (pinned to oracle/metrics.py
on the CPU by tests/test_wide_groups_ref.py), at the smallest shapes that reach each edge: the 16 items of a block, one item
past 256, runs that end inside a 16-member trip, on its boundary and many trips later, items with every group, some, one and
no member at all; then the chain through fairrec.evaluator.fairness_metrics for an attribute with 21 values, the
`sst_intersections` key of the Evaluator, and a tiny PFCN_PMF evaluated on a 12-valued attribute.  Outputs and workspaces sit
between canary frames (NaN / 0xFF start values), every return code is asserted, as in tests/test_metrics_kernels_hip.py.

The tolerance is the bound of wide_groups_ref.py (its docstring derives it from the kernel's order of additions, the measured
logf error e and the float32 subtraction); every test prints its largest error / bound, none may exceed 1.

Worst error / bound measured on an MI355X, per test group:
  fr_df_cells on the (items, groups) grid 0.23 (1 item; 0.19 at 2 items, 0.03 .. 0.06 from 15 items on); with a negative cell
  0.05; with out-of-range groups 0.012
  against the dense path at G = 2, 3, 8: 0.008 of the sum of both bounds (each path within 0.05 of its own)
  the fairness_metrics chain 0.12; through the Evaluator with the intersection gender&occupation (42 groups) 0.40
  (e = 2.84: numpy's float32 logarithm is within 1.42 x 2 v |log x| on the reference's tables)
"""
import math

import numpy as np
import pytest
import torch

import wide_groups_ref as W
from test_metrics_kernels_hip import _bytes, _dev, _Frames, _lib, _ptr, _refused, _st, _untouched, _within

pytestmark = pytest.mark.gpu


def _df(perm, start, group, value, G):
    K = len(start) - 1
    lib, f = _lib(), _Frames()
    out = f.new(torch.float64, 1)
    need = lib.fr_df_cells_workspace_bytes(K)
    assert need == (K + 15) // 16 * 8
    ws = f.ws(need)
    t = [_dev(x) for x in (perm, start, group, value)]
    if t[2].numel() == 0:                       # no member at all: the columns still need an address
        t[2], t[3] = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.float32, device="cuda")
    rc = lib.fr_df_cells(_ptr(t[0]), t[1].data_ptr(), K, t[2].data_ptr(), t[3].data_ptr(), G, out.data_ptr(), ws.data_ptr(),
                         need, _st())
    assert rc == 0, lib.fr_last_error()
    assert f.intact()
    return out.cpu().numpy()


# ---- against the float64 reference ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_items", W.ITEM_COUNTS)
def test_df_cells_against_float64(n_items):
    worst = 0.0
    for G in W.GROUPS:
        case = W.grid_case(n_items, G)
        ref = W.grid_ref(n_items, G)
        assert all(a > 0 for row in ref["table"] for a in row)            # every table entry positive
        got = _df(*case, G)
        tag = f"df_cells K={n_items} G={G} perm={'yes' if case[0] is not None else 'NULL'}"
        if G == 1:
            assert _bytes(torch.from_numpy(got)) == _bytes(torch.zeros(1, dtype=torch.float64)), tag      # exactly +0.0
        else:
            assert ref["mean"] > 0
            worst = max(worst, _within(tag, got, [ref["mean"]], [ref["bound"]]))
    print(f"df_cells K={n_items}: worst error / bound {worst:.3g}")


def test_df_cells_every_item_range_empty():
    """no member at all: every item has the absent entry only"""
    start = np.zeros(18, dtype=np.int64)
    got = _df(None, start, np.zeros(0, np.int32), np.zeros(0, np.float32), 21)
    assert _bytes(torch.from_numpy(got)) == _bytes(torch.zeros(1, dtype=torch.float64))


def test_df_cells_leaves_a_negative_cell_out():
    """a negative score sum makes a table entry negative and its logarithm NaN: it does not enter the item's maximum or minimum,
    the result is finite (the oracle returns NaN there, tests/test_wide_groups_ref.py)"""
    for G, with_perm in ((9, False), (21, True)):
        case = W.cells_case(17, G, with_perm, negative_cell=True)
        ref = W.df_cells_ref(*case, G, W.logf_ulp())
        assert sum(a < 0 for row in ref["table"] for a in row) == 1
        _within(f"df_cells with a negative cell, G={G}", _df(*case, G), [ref["mean"]], [ref["bound"]])


def test_df_cells_counts_out_of_range_groups_nowhere():
    """runs with group index -1 and n_groups (large values) at the head and the tail of every third item's range form no cell"""
    for G, with_perm in ((9, True), (65, False)):
        case = W.cells_case(40, G, with_perm, bad_groups=True)
        assert (case[2] == -1).any() and (case[2] == G).any()
        ref = W.df_cells_ref(*case, G, W.logf_ulp())
        # counted as cells they would move the result far beyond the bound
        moved = W.df_cells_ref(case[0], case[1], np.where(case[2] == -1, 0, case[2]), case[3], G + 1)
        assert abs(moved["mean"] - ref["mean"]) > 1e3 * ref["bound"]
        _within(f"df_cells with out-of-range groups, G={G}", _df(*case, G), [ref["mean"]], [ref["bound"]])


# ---- against the dense path where both exist -------------------------------------------------------------------------------------

def _dense_df(perm, start, group, value, G):
    K = len(start) - 1
    lib, f = _lib(), _Frames()
    stats = f.new(torch.float64, K, G, 3)
    t = [_dev(x) for x in (perm, start, group, value)]
    assert lib.fr_group_sums(_ptr(t[0]), t[1].data_ptr(), K, t[2].data_ptr(), t[3].data_ptr(), 0, G, stats.data_ptr(), _st()) == 0
    out = f.new(torch.float64, 5)
    need = lib.fr_fair_metrics_workspace_bytes(K)
    ws = f.ws(need)
    assert lib.fr_fair_metrics_from_stats(stats.data_ptr(), K, G, out.data_ptr(), ws.data_ptr(), need, _st()) == 0
    assert f.intact()
    return float(out.cpu()[4])


@pytest.mark.parametrize("G", [2, 3, 8])
def test_df_cells_agrees_with_the_dense_path(G):
    """fr_group_sums + fr_fair_metrics_from_stats on the same members: the two paths add in different orders, so they agree
    within the sum of their bounds (the dense path's: the same bound with ITS chain of additions -- a lane takes every 16th
    member of the item's range, the longest range put in for all, then four butterfly additions; the term for the mean
    covers its fold of a block of 256 items by butterflies as well)"""
    for with_perm in (False, True):
        case = W.cells_case(40, G, with_perm, salt=G)
        cells = W.cells_ref(*case, G)
        new = W.df_from_cells(cells, G, W.logf_ulp())
        longest = int(np.diff(case[1]).max())
        dense_bound = W.df_from_cells(cells, G, W.logf_ulp(), n_add=lambda L: W.n_additions_dense(L, longest))["bound"]
        a, b = float(_df(*case, G)[0]), _dense_df(*case, G)
        _within(f"df_cells G={G}", [a], [new["mean"]], [new["bound"]])
        _within(f"df_cells against the dense path G={G} perm={'yes' if with_perm else 'NULL'}", [a], [b],
                [new["bound"] + dense_bound])


# ---- the same bits on every call ----------------------------------------------------------------------------------------------------

def test_df_cells_is_bit_reproducible():
    for n_items, G in ((257, 21), (40, 300)):
        case = W.grid_case(n_items, G)
        assert _df(*case, G).tobytes() == _df(*case, G).tobytes()


# ---- bad arguments: the error code, fr_last_error, nothing written -------------------------------------------------------------------

def test_df_cells_refuses_bad_arguments():
    lib, f = _lib(), _Frames()
    K, G = 17, 9
    perm, start, group, value = (_dev(x) for x in W.cells_case(K, G, True))
    out = f.new(torch.float64, 1)
    need = lib.fr_df_cells_workspace_bytes(K)
    ws = f.ws(need)
    good = [perm.data_ptr(), start.data_ptr(), K, group.data_ptr(), value.data_ptr(), G, out.data_ptr(), ws.data_ptr(), need]
    for pos, bad in ((1, 0), (3, 0), (4, 0), (6, 0), (7, 0), (2, 0), (2, -1), (5, 0), (5, -1), (8, need - 1), (8, 0)):
        args = list(good)
        args[pos] = bad
        ok, why = _refused(lib.fr_df_cells(*args, _st()), "fr_df_cells")
        assert ok and f.intact() and _untouched(out) and _untouched(ws), (pos, bad, why)
    assert lib.fr_df_cells_workspace_bytes(0) == 0 and lib.fr_df_cells_workspace_bytes(-1) == 0
    assert lib.fr_df_cells(*good, _st()) == 0 and f.intact() and not _untouched(out)
    assert lib.fr_df_cells(*([0] + good[1:]), _st()) == 0 and f.intact()          # perm may be NULL


# ---- the chain: fairrec.evaluator.fairness_metrics ----------------------------------------------------------------------------------

NP = "NonParity Unfairness of sensitive attribute "
DF = "Differential Fairness of sensitive attribute "


def _chain_ref(z, name, gidx=None, G=None):
    if gidx is None:
        vals, gidx = np.unique(z[name], return_inverse=True)
        G = len(vals)
    return W.attribute_ref(z["pos_score"], z["pos_i"], gidx, G, W.logf_ulp())


def test_fairness_metrics_chain_with_a_wide_attribute():
    """40 items, 300 positives, mode full: a binary gender, a 7-valued age (the dense path), a 21-valued occupation (the new one)"""
    from fairrec.evaluator import fairness_metrics
    z = W.chain_case()
    d = lambda k: torch.from_numpy(z[k]).cuda()
    names = ["gender", "age", "occupation"]
    got = fairness_metrics(d("pos_score"), d("pos_i"), {n: d(n) for n in names}, None, None, "full")
    value_type = [f"{m} Unfairness of sensitive attribute gender" for m in ("Value", "Absolute", "Underestimation", "Overestimation")]
    assert sorted(got) == sorted([NP + n for n in names] + [DF + n for n in names] + value_type)
    nonparity, np_bound, df, df_bound = _chain_ref(z, "occupation")
    assert nonparity > 0 and df > 0
    _within("fairness_metrics, occupation (21 values)", [got[NP + "occupation"], got[DF + "occupation"]], [nonparity, df],
            [np_bound, df_bound])
    # the narrow attributes: the bytes of a call that never sees the wide one
    narrow = fairness_metrics(d("pos_score"), d("pos_i"), {n: d(n) for n in names[:2]}, None, None, "full")
    assert len(narrow) == 8
    for k, v in narrow.items():
        assert np.float64(got[k]).tobytes() == np.float64(v).tobytes(), k


def test_evaluator_reports_an_intersection():
    from fairrec.config import Config
    from fairrec.evaluator import Evaluator
    z = W.chain_case()
    d = lambda k: torch.from_numpy(z[k]).cuda()
    cfg = {"metrics": ["NonParityUnfairness", "DifferentialFairness"], "topk": [5], "metric_decimal_place": 12,
           "sst_attr_list": ["gender", "age", "occupation"], "eval_args": {"mode": "full"}, "device": "cuda"}
    collected = {"rec.positive_score": d("pos_score"), "data.positive_i": d("pos_i"), "data.gender": d("gender"),
                 "data.age": d("age"), "data.occupation": d("occupation")}
    plain = Evaluator(Config(config_dict=cfg)).evaluate(collected)
    got = Evaluator(Config(config_dict=dict(cfg, sst_intersections=[["gender", "occupation"]]))).evaluate(collected)
    name = "gender&occupation"
    assert sorted(got) == sorted(list(plain) + [NP + name, DF + name]) and all(got[k] == plain[k] for k in plain)
    # the composite code: the distinct (gender, occupation) pairs present, in any order of their own
    pairs, code = np.unique(np.stack((z["gender"].astype(np.int64), z["occupation"])), axis=1, return_inverse=True)
    G = pairs.shape[1]
    assert 21 < G <= 42
    nonparity, np_bound, df, df_bound = _chain_ref(z, name, code.reshape(-1), G)
    rounding = 0.5e-12                                          # metric_decimal_place
    _within("Evaluator, gender&occupation", [got[NP + name], got[DF + name]], [nonparity, df],
            [np_bound + rounding, df_bound + rounding])


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

def test_pfcn_pmf_evaluates_a_12_valued_attribute(tmp_path):
    """a tiny PFCN_PMF on a synthetic dataset whose sensitive column has 12 values: Trainer.evaluate reports both fairness metrics"""
    from fairrec.config import Config
    from fairrec.data.dataset import synthetic_dataset
    from fairrec.quick_start import run_recbole
    cfg = {"epochs": 1, "train_batch_size": 512, "device": "cuda", "checkpoint_dir": str(tmp_path), "embedding_size": 16,
           "topk": [5], "valid_metric": "ndcg@5", "valid_metric_bigger": True, "filter_mode": "none",
           "metrics": ["NDCG", "NonParityUnfairness", "DifferentialFairness"], "sst_attr_list": ["occupation"],
           "eval_args": {"mode": "full"}, "eval_batch_size": 4096, "metric_decimal_place": 6}
    ds = synthetic_dataset(Config(model="PFCN_PMF", dataset="synthetic", config_dict=cfg), 200, 100, 3000, seed=7,
                           sst_field="occupation")
    occupation = (torch.arange(200) % 12).to(torch.float32)
    ds.user_feat["occupation"] = occupation
    res = run_recbole(model="PFCN_PMF", dataset=ds, config_dict=cfg, saved=False)["test_result"]
    flat = {}
    for k, v in res.items():
        flat.update(v if isinstance(v, dict) else {k: v})
    assert NP + "occupation" in flat and DF + "occupation" in flat and "ndcg@5" in flat
    assert math.isfinite(flat[NP + "occupation"]) and math.isfinite(flat[DF + "occupation"]) and flat[DF + "occupation"] > 0

"""CPU: the reference of the fairness bootstrap (tests/fair_bootstrap_ref.py) against brute force -- the replicate's multiset built
with np.repeat and handed to metrics_ref.fairness_ref --, the `fairness_bootstrap` keys of the Evaluator, and the way its replicate
statistics become 'ci_low' / 'ci_high' keys (the device call replaced by a hand-made statistic: no GPU here).  The kernel itself is
compared with the reference in tests/test_fair_bootstrap_hip.py."""
import logging

import numpy as np
import pytest
import torch

import bootstrap_ref as BR
import fair_bootstrap_ref as FR
import metrics_ref as R

SEED = 2020
FAIR = ["NonParityUnfairness", "ValueUnfairness", "AbsoluteUnfairness", "UnderUnfairness", "OverUnfairness", "DifferentialFairness"]


# ---- the reference against brute force ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_users,neg_len,mode", [(5, 300, "uni100"), (40, 300, "uni100"), (129, 120, "uni100"), (40, 0, "full")])
def test_reference_against_the_repeated_multiset(n_users, neg_len, mode):
    """replicate b IS the metric of the rows repeated w(user, b) times: the point estimate's reference on that multiset, with the
    point estimate's group indices as the attribute columns"""
    z = R.chain_case(max(neg_len, 1))
    P = len(z["pos_score"])
    rng = np.random.default_rng([n_users, neg_len])
    user = np.sort(rng.integers(0, n_users, P)).astype(np.int64) + 7                 # global rows need not start at 0
    gender, _ = FR.group_index([z["gender"]])
    age, _ = FR.group_index([z["age"]])
    n_rep = 13
    neg = dict(neg_score=z["neg_score"][:neg_len], neg_i=z["neg_i"][:neg_len]) if mode != "full" else {}
    ref = FR.evaluation_ref(z["pos_score"], z["pos_i"], user, {"gender": gender, "age": age}, n_rep, SEED, mode=mode, **neg)
    assert len(ref) == 8
    W = BR.weights(user, n_rep, SEED)
    m = min(neg_len, P)
    compared, worst = 0, 0.0
    for b in range(n_rep):
        idx = np.repeat(np.arange(P), W[:, b])
        whole = all(len(np.unique(col[idx])) == len(np.unique(col)) for col in (gender, age))
        if not len(idx) or not whole:
            # a group without weight: NonParity of that attribute is NaN here; the brute force would renumber the groups
            gone = [n for n, col in (("gender", gender), ("age", age)) if len(np.unique(col[idx])) < len(np.unique(col))]
            assert all(np.isnan(ref[f"NonParity Unfairness of sensitive attribute {n}"][0][b]) for n in gone)
            continue
        kw = dict(neg_score=z["neg_score"][idx[idx < m]], neg_i=z["neg_i"][idx[idx < m]]) if mode != "full" else {}
        brute, bound = R.fairness_ref(z["pos_score"][idx], z["pos_i"][idx], {"gender": gender[idx], "age": age[idx]}, mode=mode, **kw)
        assert set(brute) == set(ref)
        for key in brute:
            got, mine = ref[key][0][b], ref[key][1][b]
            assert np.isfinite(got) and abs(got - brute[key]) <= mine + bound[key], (key, b, got, brute[key])
            worst = max(worst, abs(got - brute[key]) / (mine + bound[key]))
        compared += 1
    print(f"{n_users} users, {mode}: {compared} of {n_rep} replicates compared, worst error / bound {worst:.3g}")
    assert compared >= (n_rep // 2 if n_users > 5 else 1)


def test_items_vanish_and_alpha_follows():
    """single-member items of users of their own: K_b varies over the replicates, and the DifferentialFairness entry uses 1 / K_b"""
    perm, start, group, value, wtrue, unit = FR.case(17, 2, True, "ones", "own")
    ref = FR.replicates_ref(perm, start, group, value, wtrue, unit, 2, 9, SEED)
    assert len(set(ref["items"].tolist())) > 1 and ref["items"].max() <= 17 and ref["items"].min() >= 13
    assert np.isfinite(ref["values"]).all() and (ref["bounds"] > 0).all()
    one = FR.replicates_ref(*FR.case(2, 3, False, "null", "one"), 3, 9, SEED)
    dead = BR.weights([5], 9, SEED)[0] == 0
    assert dead.any() and (one["items"][dead] == 0).all() and np.isnan(one["values"][:, dead]).all()
    assert (one["items"][~dead] == 2).all() and np.isfinite(one["values"][:, ~dead]).all()
    assert np.isnan(FR.nonparity_ref(one)[0][dead]).all()


def test_workspace_formula():
    assert FR.chunks(1000, 1, 5) == 1 and FR.chunks(1016, 2, 5) == 2 and FR.chunks(5000, 257, 5) == 79
    assert FR.chunks(10 ** 6, 10 ** 5, 200) == 1024 and FR.chunks(10 ** 6, 10 ** 5, 65536) == 16
    assert FR.workspace_bytes(1000, 1, 2, 5) == 5 * 10 * 8


# ---- the Evaluator's keys ----------------------------------------------------------------------------------------------------------

def _config(**kw):
    from fairrec.config import Config
    base = {"metrics": FAIR, "topk": [5], "sst_attr_list": ["gender", "age"], "eval_args": {"mode": "full"}, "device": "cpu"}
    return Config(model="FOCF", config_dict=dict(base, **kw))


def test_fairness_bootstrap_key_values():
    from fairrec.evaluator import Collector, Evaluator
    assert _config()["fairness_bootstrap"] is None and _config()["fairness_bootstrap_level"] == 0.95
    for value in (None, 0):
        assert Evaluator(_config(fairness_bootstrap=value)).fair_bootstrap == 0
        assert Collector(_config(fairness_bootstrap=value)).positive_user is False
    ev = Evaluator(_config(fairness_bootstrap=200))
    assert ev.fair_bootstrap == 200 and ev.fair_bootstrap_level == 0.95 and ev.seed == 2020
    assert Collector(_config(fairness_bootstrap=200)).positive_user is True
    ev = Evaluator(_config(fairness_bootstrap=65536, fairness_bootstrap_level=0.5, seed=7, eval_args={"mode": "pop20"}))
    assert ev.fair_bootstrap == 65536 and ev.fair_bootstrap_level == 0.5 and ev.seed == 7
    with pytest.raises(ValueError, match="fairness_bootstrap needs a fairness metric"):
        Evaluator(_config(fairness_bootstrap=200, metrics=["NDCG", "GAUC"]))
    with pytest.raises(ValueError, match="fairness_bootstrap needs eval_args.mode full / uniN / popN, not 'labeled'"):
        Evaluator(_config(fairness_bootstrap=200, metrics=["AUC"], eval_args={"mode": "labeled"}))
    for value in (1, -3, 65537, 2.5, "200", True, [200]):
        with pytest.raises(ValueError, match="fairness_bootstrap must be"):
            Evaluator(_config(fairness_bootstrap=value))
    for level in (0, 1, 0.0, 1.0, -0.5, 1.5, "0.9", True):
        with pytest.raises(ValueError, match="fairness_bootstrap_level"):
            Evaluator(_config(fairness_bootstrap=200, fairness_bootstrap_level=level))
    # the neighbouring key keeps its own wording
    with pytest.raises(ValueError, match="group_bootstrap must be"):
        Evaluator(_config(group_bootstrap=1, utility_by_group=True))


def _stand_ins(monkeypatch, B, calls):
    """fairness_metrics and bootstrap_fairness replaced by host stand-ins with recognisable values"""
    from fairrec.evaluator import metrics as M

    def point(pos_score, pos_i, sst, *a, value_type=True, intersections=None, **kw):
        res = {}
        for n, name in enumerate(list(sst) + ["&".join(e) for e in intersections or []]):
            res[f"NonParity Unfairness of sensitive attribute {name}"] = 0.25
            res[f"Differential Fairness of sensitive attribute {name}"] = 0.5
            if n == 0 and value_type:
                res.update({f"{q} Unfairness of sensitive attribute {name}": 0.125
                            for q in ("Value", "Absolute", "Underestimation", "Overestimation")})
        return res

    def replicates(items, group, value, wtrue, unit, n_groups, n_rep, seed, value_type=False, differential=True, sort=None):
        calls.append((int(n_groups), int(items.numel()), bool(value_type), bool(differential), wtrue is not None, sort is not None))
        assert n_rep == B and seed == 2020 and unit.dtype == torch.int64
        base = np.arange(B, dtype=np.float64) + 100.0 * n_groups
        out = {"items": np.full(B, 3), "nonparity": base + 0.1}
        if value_type:
            out.update({k: base + j for j, k in enumerate(("value", "absolute", "under", "over"), 1)})
        if differential:
            out["differential"] = np.where(np.arange(B) % 5 == 0, np.nan, base + 0.7)
        return out

    monkeypatch.setattr(M, "fairness_metrics", point)
    monkeypatch.setattr(M, "bootstrap_fairness", replicates)


def _collected(mode):
    z = FR.collected_case(mode)
    return {k: torch.from_numpy(v) for k, v in z.items()}


@pytest.mark.parametrize("mode", ["full", "uni100"])
def test_interval_keys_and_their_order(monkeypatch, mode):
    from fairrec.evaluator import Evaluator
    B, calls = 40, []
    _stand_ins(monkeypatch, B, calls)
    collected = _collected(mode)
    P = collected["data.positive_i"].numel()
    cfg = dict(fairness_bootstrap=B, fairness_bootstrap_level=0.9, sst_intersections=[["gender", "age"]], eval_args={"mode": mode},
               metric_decimal_place=12)
    res = Evaluator(_config(**cfg)).evaluate(collected)
    rows = P if mode == "full" else 2 * P - 3
    assert calls == [(2, P, False, True, False, True), (2, rows, True, False, True, False), (3, P, False, True, False, True),
                     (6, P, False, True, False, True)]
    keys = list(res)
    points = [k for k in keys if " ci_" not in k]
    assert len(points) == 10 and keys[:10] == points
    assert keys[10:] == [c for k in points for c in FR.ci_keys(k)]                    # the order of the point-estimate keys
    for key, G, shift in (("Value Unfairness of sensitive attribute gender", 2, 1.0),
                          ("Overestimation Unfairness of sensitive attribute gender", 2, 4.0),
                          ("NonParity Unfairness of sensitive attribute gender&age", 6, 0.1),
                          ("Differential Fairness of sensitive attribute age", 3, 0.7)):
        stat = np.arange(B, dtype=np.float64) + 100.0 * G + shift
        if shift == 0.7:
            stat[::5] = np.nan                                                       # unusable replicates are left out
        low, high, _, _, usable, _ = BR.intervals_ref(stat[None, :], 0.9)
        lo_key, hi_key = FR.ci_keys(key)
        assert usable[0] == (B if shift != 0.7 else B - B // 5)
        assert res[lo_key] == pytest.approx(low[0], abs=1e-9) and res[hi_key] == pytest.approx(high[0], abs=1e-9)
    # only the metrics asked for
    calls.clear()
    res = Evaluator(_config(metrics=["NonParityUnfairness"], **cfg)).evaluate(collected)
    assert [c[3] for c in calls] == [False, False, False] and not any(c[2] for c in calls)
    assert sorted(k for k in res if "ci_" in k) == sorted(
        c for n in ("gender", "age", "gender&age") for c in FR.ci_keys(f"NonParity Unfairness of sensitive attribute {n}"))
    calls.clear()
    res = Evaluator(_config(metrics=["AbsoluteUnfairness"], **cfg)).evaluate(collected)
    assert calls == [(2, rows, True, False, True, False)]
    assert [k for k in res if "ci_" in k] == list(FR.ci_keys("Absolute Unfairness of sensitive attribute gender"))


def test_starved_intervals_are_nan_with_one_warning(monkeypatch, caplog):
    from fairrec.evaluator import Evaluator
    from fairrec.evaluator import metrics as M
    B = 10
    _stand_ins(monkeypatch, B, [])
    real = M.bootstrap_fairness

    def mostly_nan(*a, **kw):
        out = real(*a, **kw)
        out["nonparity"] = np.where(np.arange(B) < 6, np.nan, out["nonparity"])
        return out

    monkeypatch.setattr(M, "bootstrap_fairness", mostly_nan)
    with caplog.at_level(logging.WARNING):
        res = Evaluator(_config(metrics=["NonParityUnfairness"], sst_attr_list=["gender"], fairness_bootstrap=B)).evaluate(
            _collected("full"))
    lo, hi = FR.ci_keys("NonParity Unfairness of sensitive attribute gender")
    assert np.isnan(res[lo]) and np.isnan(res[hi])
    assert len([r for r in caplog.records if "fewer than half" in r.getMessage()]) == 1


def test_more_than_eight_groups_get_no_interval(monkeypatch, caplog):
    from fairrec.evaluator import Evaluator
    calls = []
    _stand_ins(monkeypatch, 8, calls)
    with caplog.at_level(logging.WARNING):
        res = Evaluator(_config(metrics=["NonParityUnfairness", "DifferentialFairness"], sst_attr_list=["gender", "zip"],
                                fairness_bootstrap=8)).evaluate(_collected("full"))
    assert [c[0] for c in calls] == [2]
    assert "NonParity Unfairness of sensitive attribute zip" in res and not any("ci_" in k and "zip" in k for k in res)
    assert len([k for k in res if "ci_" in k]) == 4
    assert len([r for r in caplog.records if "zip has 9 groups" in r.getMessage()]) == 1


def test_nothing_changes_without_the_key(monkeypatch):
    from fairrec.evaluator import Evaluator
    from fairrec.evaluator import metrics as M
    _stand_ins(monkeypatch, 8, [])

    def forbidden(*a, **kw):
        raise AssertionError("the bootstrap path ran with fairness_bootstrap unset")

    monkeypatch.setattr(M, "bootstrap_fairness", forbidden)
    monkeypatch.setattr(M, "bootstrap_intervals", forbidden)
    collected = _collected("full")
    del collected["data.positive_user"]
    for extra in ({}, {"fairness_bootstrap": None}, {"fairness_bootstrap": 0}):
        res = Evaluator(_config(**extra)).evaluate(collected)
        assert len(res) == 8 and not any("ci_" in k for k in res)


def test_value_type_rows_match_the_reference_members():
    from fairrec.evaluator import value_type_rows
    z = FR.collected_case("uni100")
    t = {k: torch.from_numpy(v) for k, v in z.items()}
    gidx = torch.from_numpy(FR.group_index([z["data.gender"]])[0]).to(torch.int32)
    P = len(z["data.positive_i"])
    items, group, value, wtrue, unit = value_type_rows(t["rec.positive_score"], t["data.positive_i"], gidx, t["data.positive_user"],
                                                       t["rec.negative_score"], t["data.negative_i"], "uni100")
    m = P - 3
    assert items.tolist() == z["data.positive_i"].tolist() + z["data.negative_i"][:m].tolist()
    assert unit.tolist() == z["data.positive_user"].tolist() + z["data.positive_user"][:m].tolist()
    assert group.tolist() == gidx.tolist() + gidx[:m].tolist() and wtrue.tolist() == [1.0] * P + [0.0] * m
    assert value.dtype == torch.float32 and value.numel() == P + m
    full = value_type_rows(t["rec.positive_score"], t["data.positive_i"], gidx, t["data.positive_user"], None, None, "full")
    assert full[0].numel() == P and full[3].tolist() == [1.0] * P and full[4] is t["data.positive_user"]

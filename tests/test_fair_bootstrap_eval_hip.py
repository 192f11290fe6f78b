"""GPU: the `fairness_bootstrap` key end to end.  Evaluator.evaluate on synthetic collected arrays in `full` and `uni100` form
against the intervals of the reference (tests/fair_bootstrap_ref.py: the replicate statistics restated in float64,
bootstrap_ref.intervals_ref on them), then Collector + Evaluator through Trainer.evaluate of a FOCF model on a synthetic data set
of 200 users and 60 items in `full` (the matrix path and `full_sort_eval: fused`) and `uni50`, eight users per batch, so that
`data.positive_user` has to carry the rows of the batches before.

Tolerances: an interval end may move by the largest bound among its usable replicates + 2 u |q| (fair_bootstrap_ref.interval_ref)
and by the half step of the rounding to 12 places.  Every comparison prints its largest error / bound, none may exceed 1.

Worst error / bound measured on an MI355X:
  Evaluator on collected arrays 0.85 (full), 0.89 (uni100); Trainer.evaluate 0.92 (full, matrix), 0.83 (full, fused), 0.86 (uni50):
  the rounding to 12 decimal places, which the bound allows for with its full half step, is what these measure (the kernel's
  share is the figures of tests/test_fair_bootstrap_hip.py)
"""
import logging

import numpy as np
import pytest
import torch

import fair_bootstrap_ref as FR
from test_group_metrics_hip import _evaluate
from test_metrics_kernels_hip import _logf_ulp, _within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DP = 12
ROUND = 0.5 * 10.0 ** -DP
FAIR = ["NonParityUnfairness", "ValueUnfairness", "AbsoluteUnfairness", "UnderUnfairness", "OverUnfairness", "DifferentialFairness"]
B, LEVEL = 40, 0.9


def _check_intervals(tag, res, ref, level=LEVEL):
    """every key of `ref` has its two ci keys in `res`, within the reference interval's tolerance; no other ci key"""
    got, want, bound = [], [], []
    for key, (stat, bnd) in ref.items():
        low, high, tol = FR.interval_ref(stat, bnd, level)
        assert np.isfinite([low, high]).all(), key
        lo_key, hi_key = FR.ci_keys(key)
        got += [res[lo_key], res[hi_key]]
        want += [low, high]
        bound += [tol + ROUND, tol + ROUND]
        med = float(np.median(stat[np.isfinite(stat)]))
        assert res[lo_key] <= med <= res[hi_key], (key, res[lo_key], med, res[hi_key])
    assert {k for k in res if " ci_" in k} == {c for key in ref for c in FR.ci_keys(key)}
    return _within(tag, got, want, bound)


# ---- Evaluator.evaluate on collected arrays ----------------------------------------------------------------------------------------

def _config(**kw):
    from fairrec.config import Config
    base = {"metrics": FAIR, "topk": [5], "sst_attr_list": ["gender", "age"], "sst_intersections": [["gender", "age"]],
            "metric_decimal_place": DP, "device": DEV, "fairness_bootstrap": B, "fairness_bootstrap_level": LEVEL}
    return Config(model="FOCF", config_dict=dict(base, **kw))


@pytest.mark.parametrize("mode", ["full", "uni100"])
def test_evaluator_intervals_against_the_reference(mode):
    from fairrec.evaluator import Evaluator
    z = FR.collected_case(mode)
    collected = {k: torch.from_numpy(v).to(DEV) for k, v in z.items()}
    cfg = _config(eval_args={"mode": mode})
    res = Evaluator(cfg).evaluate(collected)
    sst = {a: z["data." + a] for a in ("gender", "age")}
    ref = FR.evaluation_ref(z["rec.positive_score"], z["data.positive_i"], z["data.positive_user"], sst, B, cfg["seed"],
                            z.get("rec.negative_score"), z.get("data.negative_i"), mode, [["gender", "age"]], True, _logf_ulp())
    assert len(ref) == 10
    _check_intervals(f"Evaluator fairness_bootstrap, {mode}", res, ref)
    # the point estimates are what they are without the key, in the same order, the ci keys after them
    off = Evaluator(_config(eval_args={"mode": mode}, fairness_bootstrap=None)).evaluate(
        {k: v for k, v in collected.items() if k != "data.positive_user"})
    assert list(off) == [k for k in res if " ci_" not in k] == list(res)[:10] and all(repr(off[k]) == repr(res[k]) for k in off)
    assert list(res)[10:] == [c for k in off for c in FR.ci_keys(k)]
    # the seed moves the replicates; the same seed gives the same bytes
    again = Evaluator(cfg).evaluate(collected)
    assert {k: repr(v) for k, v in again.items()} == {k: repr(v) for k, v in res.items()}
    other = Evaluator(_config(eval_args={"mode": mode}, seed=7)).evaluate(collected)
    assert all(repr(other[k]) == repr(res[k]) for k in off) and any(other[k] != res[k] for k in res if " ci_" in k)
    # only the metrics asked for
    few = Evaluator(_config(eval_args={"mode": mode}, metrics=["UnderUnfairness", "DifferentialFairness"])).evaluate(collected)
    keep = [k for k in ref if k.startswith(("Underestimation", "Differential"))]
    assert len(keep) == 4 and {k for k in few if " ci_" in k} == {c for k in keep for c in FR.ci_keys(k)}
    assert all(repr(few[k]) == repr(res[k]) for k in few)


def test_nine_groups_get_no_interval_and_one_warning(caplog):
    from fairrec.evaluator import Evaluator
    z = FR.collected_case("full")
    collected = {k: torch.from_numpy(v).to(DEV) for k, v in z.items()}
    keys = dict(eval_args={"mode": "full"}, sst_attr_list=["gender", "zip"], sst_intersections=None,
                metrics=["NonParityUnfairness", "DifferentialFairness"])
    with caplog.at_level(logging.WARNING):
        res = Evaluator(_config(**keys)).evaluate(collected)
    off = Evaluator(_config(fairness_bootstrap=None, **keys)).evaluate(collected)
    assert len(off) == 4 and all(repr(off[k]) == repr(res[k]) for k in off)
    assert {k for k in res if " ci_" in k} == {c for k in off if k.endswith("gender") for c in FR.ci_keys(k)}
    assert len([r for r in caplog.records if "zip has 9 groups" in r.getMessage()]) == 1


def test_refusals():
    from fairrec.evaluator import Evaluator
    with pytest.raises(ValueError, match="fairness_bootstrap needs a fairness metric"):
        Evaluator(_config(metrics=["NDCG"], eval_args={"mode": "full"}))
    with pytest.raises(ValueError, match="fairness_bootstrap needs eval_args.mode full / uniN / popN, not 'labeled'"):
        Evaluator(_config(metrics=["AUC"], eval_args={"mode": "labeled"}))
    with pytest.raises(ValueError, match="fairness_bootstrap must be"):
        Evaluator(_config(fairness_bootstrap=1, eval_args={"mode": "full"}))
    with pytest.raises(ValueError, match="fairness_bootstrap_level"):
        Evaluator(_config(fairness_bootstrap_level=1.0, eval_args={"mode": "full"}))


# ---- through Trainer.evaluate ------------------------------------------------------------------------------------------------------

N_USERS, N_ITEMS = 201, 61           # row 0 of either table is [PAD]
COMMON = {"epochs": 1, "train_batch_size": 512, "device": DEV, "embedding_size": 8, "fair_objective": "value",
          "valid_metric_bigger": True, "sst_attr_list": ["gender", "age"], "sst_intersections": [["gender", "age"]],
          "eval_batch_size": 8 * N_ITEMS, "metric_decimal_place": DP, "metrics": ["NDCG"] + FAIR, "topk": [10],
          "valid_metric": "ndcg@10"}
_runs = {}


def _run(mode, tmp_path_factory):
    """(trainer, test loader) of a FOCF model trained for one epoch under `eval_args.mode: mode`, once per mode"""
    if mode not in _runs:
        from fairrec.config import Config
        from fairrec.data import dataloader as DL
        from fairrec.data.dataset import synthetic_dataset
        from fairrec.quick_start import run_recbole
        cfg = dict(COMMON, eval_args={"mode": mode}, checkpoint_dir=str(tmp_path_factory.mktemp("fairboot_" + mode)))
        ds = synthetic_dataset(Config(model="FOCF", dataset="synthetic", config_dict=cfg), N_USERS, N_ITEMS, 4000, seed=11)
        ds.user_feat["age"] = torch.tensor([18, 35, 50])[torch.arange(N_USERS) * 7 % 3]
        seen, loaders, inits = {}, [], {}
        classes = (DL.FullSortEvalDataLoader, DL.NegSampleEvalDataLoader)

        def recording(cls):
            init = inits[cls] = cls.__init__

            def wrapped(self, *a, **kw):
                init(self, *a, **kw)
                loaders.append(self)
            cls.__init__ = wrapped

        for cls in classes:
            recording(cls)
        try:
            run_recbole(model="FOCF", dataset=ds, config_dict=cfg, saved=False, before_fit=lambda m, tr: seen.update(trainer=tr))
        finally:
            for cls in classes:
                cls.__init__ = inits[cls]
        _runs[mode] = (seen["trainer"], loaders[-1])               # the test loader is built last
    return _runs[mode]


def _reference(collected, mode, seed, value_type=True):
    h = {k: v.cpu().numpy() for k, v in collected.items() if torch.is_tensor(v)}
    sst = {a: h["data." + a] for a in ("gender", "age")}
    return FR.evaluation_ref(h["rec.positive_score"], h["data.positive_i"], h["data.positive_user"], sst, B, seed,
                             h.get("rec.negative_score"), h.get("data.negative_i"), mode, [["gender", "age"]], value_type,
                             _logf_ulp())


def _check_units(collected):
    """`data.positive_user` is the row of the pair's user in `rec.topk`: ascending over the batches, every row's number of
    positives (the last column of `rec.topk`) is the number of pairs that carry it"""
    unit = collected["data.positive_user"].cpu().numpy()
    rec = collected["rec.topk"].cpu().numpy()
    assert unit.dtype == np.int64 and len(unit) == len(collected["data.positive_i"]) and (np.diff(unit) >= 0).all()
    assert np.array_equal(np.bincount(unit, minlength=rec.shape[0]), rec[:, -1]) and rec.shape[0] > 100


def test_trainer_full_matrix_and_fused(tmp_path_factory, monkeypatch):
    trainer, loader = _run("full", tmp_path_factory)
    on = dict(fairness_bootstrap=B, fairness_bootstrap_level=LEVEL)
    monkeypatch.setattr(trainer, "full_sort_eval", "matrix")
    matrix, collected = _evaluate(trainer, loader, monkeypatch, **on)
    _check_units(collected)
    _check_intervals("Trainer.evaluate fairness_bootstrap, full (matrix)", matrix, _reference(collected, "full", trainer.config["seed"]))
    monkeypatch.setattr(trainer, "full_sort_eval", "fused")
    fused, collected_f = _evaluate(trainer, loader, monkeypatch, **on)
    assert torch.equal(collected["data.positive_user"], collected_f["data.positive_user"])
    _check_intervals("Trainer.evaluate fairness_bootstrap, full (fused)", fused, _reference(collected_f, "full", trainer.config["seed"]))
    # the same seed: the same result; another seed: other intervals, the same point estimates
    again, _ = _evaluate(trainer, loader, monkeypatch, **on)
    assert {k: repr(v) for k, v in again.items()} == {k: repr(v) for k, v in fused.items()}
    other, _ = _evaluate(trainer, loader, monkeypatch, seed=7, **on)
    assert set(other) == set(fused) and any(other[k] != fused[k] for k in fused if " ci_" in k)
    assert all(repr(other[k]) == repr(fused[k]) for k in fused if " ci_" not in k)
    # only the requested metrics get keys
    few, _ = _evaluate(trainer, loader, monkeypatch, metrics=["NDCG", "NonParityUnfairness"], **on)
    assert {k for k in few if " ci_" in k} == {c for a in ("gender", "age", "gender&age")
                                               for c in FR.ci_keys(f"NonParity Unfairness of sensitive attribute {a}")}
    assert all(repr(few[k]) == repr(fused[k]) for k in few)
    # the key unset: the result and the collected keys of a run that never mentions it
    for value in (None, 0):
        off, collected_off = _evaluate(trainer, loader, monkeypatch, fairness_bootstrap=value)
        assert list(off) == [k for k in fused if " ci_" not in k] and all(repr(off[k]) == repr(fused[k]) for k in off)
        assert set(collected) - set(collected_off) == {"data.positive_user"}
    del trainer.config.final_config_dict["fairness_bootstrap"], trainer.config.final_config_dict["fairness_bootstrap_level"]
    never, collected_never = _evaluate(trainer, loader, monkeypatch)
    assert {k: repr(v) for k, v in never.items()} == {k: repr(v) for k, v in off.items()} and list(never) == list(off)
    assert set(collected_never) == set(collected_off)


def test_trainer_uni50(tmp_path_factory, monkeypatch):
    trainer, loader = _run("uni50", tmp_path_factory)
    res, collected = _evaluate(trainer, loader, monkeypatch, fairness_bootstrap=B, fairness_bootstrap_level=LEVEL)
    _check_units(collected)
    assert "rec.negative_score" in collected
    _check_intervals("Trainer.evaluate fairness_bootstrap, uni50", res, _reference(collected, "uni50", trainer.config["seed"]))
    # (the loader draws fresh negatives for every evaluation: the keys are compared, not the values)
    off, collected_off = _evaluate(trainer, loader, monkeypatch, fairness_bootstrap=None)
    assert list(off) == [k for k in res if " ci_" not in k]
    assert set(collected) - set(collected_off) == {"data.positive_user"}

"""GPU: evaluation by value end to end -- `eval_args.mode: labeled` through Trainer.evaluate / PFCNTrainer.evaluate and
run_recbole (AUC / LogLoss / MAE / RMSE of `predict` against LABEL_FIELD), and GAUC next to the ranking metrics in the
full / uniN / popN modes -- against tests/value_metrics_ref.py fed with predictions the test recomputes itself."""
import numpy as np
import pytest
import torch

import value_metrics_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
VALUE = ["AUC", "LogLoss", "MAE", "RMSE"]
SMALL = {"NFCF": dict(mlp_hidden_size=[16, 8], load_pretrain_path=None),
         "PFCN_BiasedMF": dict(filter_mode="none"),
         "FOCF": dict(fair_objective="value")}


def _close(got, want, what=""):
    """after the Evaluator's rounding at metric_decimal_place 10: relative 1e-9 (plus the rounding step)"""
    assert abs(got - want) <= 1e-9 * abs(want) + 0.5e-10, (what, got, want)


def _reference(model, loader, names, sst_list=None, dp=10):
    """predict batch by batch over the loader, the concatenation through the numpy restatement, rounded like the Evaluator."""
    extra = () if sst_list is None else (sst_list,)
    scores, labels = [], []
    model.eval()
    with torch.no_grad():
        for inter in loader:
            inter = inter.to(DEV)
            scores.append(model.predict(inter, *extra).view(-1).float().cpu().numpy())
            labels.append(inter["label"].float().cpu().numpy())
    s, y = np.concatenate(scores), np.concatenate(labels)
    return {m: round(v, dp) for m, v in R.value_metrics(s, y, [n.lower() for n in names]).items()}, s, y


@pytest.mark.parametrize("name", ["NFCF", "PFCN_BiasedMF"])
def test_trainer_evaluate_over_a_labeled_loader(name, tmp_path):
    from fairrec.config import Config
    from fairrec.data.dataloader import LabeledEvalDataLoader
    from fairrec.data.dataset import synthetic_dataset
    from fairrec.sampler import global_random_state
    from fairrec.utils import get_model, get_trainer, init_seed
    cfg = Config(model=name, config_dict=dict(SMALL[name], device=DEV, checkpoint_dir=str(tmp_path), embedding_size=16,
                                              eval_args={"mode": "labeled"}, metrics=VALUE, metric_decimal_place=10,
                                              eval_batch_size=300, valid_metric="auc"))
    init_seed(5, True)
    ds = synthetic_dataset(cfg, 90, 70, 2030)
    ds.inter_feat["label"] = (ds.inter_feat["rating"] >= 3).float()
    model = get_model(name)(cfg, ds).to(DEV)
    trainer = get_trainer(None, name)(cfg, model)
    loader = LabeledEvalDataLoader(cfg, ds.to(DEV))
    assert len(loader) == 7 and all(b["user_id"].is_cuda and "gender" in b for b in loader)
    rs = global_random_state(torch.device(DEV))
    before = (np.random.get_state()[1].copy(), torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone(), rs.get_state())
    raw = trainer.evaluate(loader)
    after = (np.random.get_state()[1], torch.get_rng_state(), torch.cuda.get_rng_state(), rs.get_state())
    assert (before[0] == after[0]).all() and torch.equal(before[1], after[1]) and torch.equal(before[2], after[2])
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(before[3], after[3]))
    got = raw
    if name == "PFCN_BiasedMF":
        assert list(raw) == ["none"]
        got = raw["none"]
    want, s, y = _reference(model, loader, VALUE)
    assert list(got) == ["auc", "logloss", "mae", "rmse"]
    assert len(np.unique(s)) > 100 and 0 < y.sum() < len(y)
    for m in want:
        print(name, m, got[m], want[m])
        _close(got[m], want[m], m)
    assert trainer.evaluate(loader) == raw                    # a second pass over the loader: the same result


def _run(model, extra, tmp_path):
    from fairrec.quick_start import run_recbole
    seen = {"valid": [], "loaders": []}

    def before_fit(m, trainer):
        seen["model"], seen["trainer"] = m, trainer
        valid_epoch, evaluate = trainer._valid_epoch, trainer.evaluate

        def rec_valid(valid_data, show_progress=False):
            out = valid_epoch(valid_data, show_progress=show_progress)
            seen["valid"].append(out)
            return out

        def rec_eval(eval_data, *a, **k):
            seen["loaders"].append(eval_data)
            return evaluate(eval_data, *a, **k)

        trainer._valid_epoch, trainer.evaluate = rec_valid, rec_eval

    cfg = dict(SMALL.get(model, {}), epochs=3, train_batch_size=512, synthetic_users=120, synthetic_items=80,
               synthetic_interactions=3000, device=DEV, checkpoint_dir=str(tmp_path), embedding_size=16, eval_batch_size=256,
               metric_decimal_place=10)
    cfg.update(extra)
    return run_recbole(model=model, config_dict=cfg, before_fit=before_fit), seen


@pytest.mark.parametrize("model,metrics,valid_metric", [("NFCF", ["AUC", "LogLoss"], "auc"),
                                                        ("FOCF", ["RMSE", "MAE", "AUC"], "rmse")])
def test_run_recbole_labeled(model, metrics, valid_metric, tmp_path):
    from fairrec.data.dataloader import LabeledEvalDataLoader
    out, seen = _run(model, dict(eval_args={"mode": "labeled"}, metrics=metrics, valid_metric=valid_metric,
                                 threshold={"rating": 3}), tmp_path)
    keys = [m.lower() for m in metrics]
    assert list(out["test_result"]) == keys and list(out["best_valid_result"]) == keys
    bigger = valid_metric == "auc"
    assert out["valid_score_bigger"] is bigger
    # the best epoch is the first strict best of the per-epoch validation scores
    assert len(seen["valid"]) == 3 and all(sc == res[valid_metric] for sc, res in seen["valid"])
    scores = [sc for sc, _ in seen["valid"]]
    best = (max if bigger else min)(scores)
    assert out["best_valid_score"] == best and out["best_valid_result"] == seen["valid"][scores.index(best)][1]
    # both evaluation loaders are labeled ones over splits that kept the rating column; training batches are what they were
    test_loader = seen["loaders"][-1]
    assert all(isinstance(d, LabeledEvalDataLoader) for d in seen["loaders"])
    feat = test_loader.dataset.inter_feat
    assert torch.equal(feat["label"], (feat["rating"] >= 3).float())
    # the test result is an evaluation of the saved checkpoint, redone here
    trainer, m = seen["trainer"], seen["model"]
    ck = torch.load(trainer.saved_model_file, weights_only=False)
    m.load_state_dict(ck["state_dict"])
    m.load_other_parameter(ck.get("other_parameter"))
    want, s, y = _reference(m, test_loader, metrics)
    for k in keys:
        print(model, k, out["test_result"][k], want[k])
        _close(out["test_result"][k], want[k], k)


def _record_collects(monkeypatch):
    from fairrec.evaluator import Collector
    log = []
    cand, full = Collector.eval_batch_collect_candidates, Collector.eval_batch_collect
    c = lambda t: t.detach().cpu().numpy().copy()

    def rec_cand(self, origin_scores, row_idx, interaction, positive_u, positive_i, n_items):
        log.append((self, "cand", c(origin_scores).reshape(-1), c(row_idx), c(interaction["item_id"]), c(positive_u), c(positive_i),
                    n_items))
        return cand(self, origin_scores, row_idx, interaction, positive_u, positive_i, n_items)

    def rec_full(self, scores, interaction, positive_u, positive_i):
        log.append((self, "full", c(scores), None, None, c(positive_u), c(positive_i), scores.shape[1]))
        return full(self, scores, interaction, positive_u, positive_i)

    monkeypatch.setattr(Collector, "eval_batch_collect_candidates", rec_cand)
    monkeypatch.setattr(Collector, "eval_batch_collect", rec_full)
    return log


def _triples(entry):
    _, kind, scores, row_idx, items, pu, pi, n_items = entry
    U = int(pu[-1]) + 1 if kind == "cand" else scores.shape[0]
    if kind == "cand":
        dense = np.full((U, n_items), -np.inf, dtype=np.float32)
        dense[row_idx, items] = scores
    else:
        dense = scores.astype(np.float32)
    mask = np.zeros((U, n_items), dtype=bool)
    mask[pu, pi] = True
    return [R.meanrank(dense[u], mask[u]) for u in range(U)]


@pytest.mark.parametrize("mode", ["uni20", "pop20", "full"])
def test_gauc_next_to_ndcg(mode, tmp_path, monkeypatch):
    common = dict(eval_args={"mode": mode}, topk=[5, 10], valid_metric="ndcg@10", epochs=1, synthetic_items=300,
                  sst_attr_list=["gender"], eval_batch_size=2048)
    plain, _ = _run("FOCF", dict(common, metrics=["NDCG", "Recall", "DifferentialFairness"]), tmp_path / "a")
    log = _record_collects(monkeypatch)
    with_gauc, _ = _run("FOCF", dict(common, metrics=["NDCG", "GAUC", "Recall", "DifferentialFairness"]), tmp_path / "b")
    monkeypatch.undo()
    res = with_gauc["test_result"]
    assert "gauc" in res and "gauc" in with_gauc["best_valid_result"]
    # every other value is what the run without GAUC gave
    assert {k: v for k, v in res.items() if k != "gauc"} == plain["test_result"]
    assert {k: v for k, v in with_gauc["best_valid_result"].items() if k != "gauc"} == plain["best_valid_result"]
    # gauc from the scores the test's Collector was handed
    last = log[-1][0]
    triples = [t for e in log if e[0] is last for t in _triples(e)]
    assert len(triples) > 50 and any(t[2] > 1 for t in triples)
    want = R.gauc(triples)
    print(mode, "gauc", res["gauc"], want)
    _close(res["gauc"], round(want, 10), "gauc")
    assert 0.0 <= res["gauc"] <= 1.0


def test_pfcn_filtered_labeled_results_per_subset_and_fairgo_refusal(tmp_path):
    out, seen = _run("PFCN_BiasedMF", dict(filter_mode="sm", dis_hidden_size_list=[16, 8], train_epoch_interval=1, epochs=2,
                                           eval_args={"mode": "labeled"}, metrics=["AUC", "LogLoss"], valid_metric="auc",
                                           threshold={"rating": 3}, sst_attr_list=["gender"]), tmp_path / "pfcn")
    key = "sm-['gender']"
    assert list(out["test_result"]) == [key] and list(out["test_result"][key]) == ["auc", "logloss"]
    assert list(out["best_valid_result"]) == ["auc", "logloss"]           # validation pools the subsets into one result
    trainer, m = seen["trainer"], seen["model"]
    ck = torch.load(trainer.saved_model_file, weights_only=False)
    m.load_state_dict(ck["state_dict"])
    m.load_other_parameter(ck.get("other_parameter"))
    want, s, y = _reference(m, seen["loaders"][-1], ["AUC", "LogLoss"], sst_list=["gender"])
    for k in ("auc", "logloss"):
        print("PFCN_BiasedMF sm", k, out["test_result"][key][k], want[k])
        _close(out["test_result"][key][k], want[k], k)
    with pytest.raises(NotImplementedError, match="labeled"):
        _run("FairGo_PMF", dict(epochs=1, pretrain_epochs=1, train_epoch_interval=1, n_layers=2, dis_hidden_size_list=[16, 8, 4],
                                filter_hidden_size_list=[32, 16], neg_sampling=None, eval_args={"mode": "labeled"},
                                metrics=["AUC"], valid_metric="auc", threshold={"rating": 3}, sst_attr_list=["gender"]),
             tmp_path / "fairgo")

"""GPU: fairrec.evaluator.leakage.probe_leakage end to end -- the fused probe (csrc/probe.hip) on the three data sets of
probe_ref.leak_data, under the bounds tests/test_probe_ref.py holds the float64 reference to on the CPU -- and the trainers'
`leakage_probe` key: the new result keys in every subset's dict, every earlier key unchanged, and probe_file on the file
save_sst_embed wrote giving the trainer's numbers.

U = 10 000, D = 16, H = 16, test_ratio 0.2, lr 0.01, batch 1024, 20 epochs:
  planted      x[:, 0] += 2 (2y - 1) on unit-normal noise: the Bayes AUC is Phi(2.83) ~ 0.998; AUC >= 0.9
  independent  labels independent of X: |AUC - 0.5| <= 0.06 (2 000 balanced test rows: the null AUC's standard deviation is about
               0.013, so more than four of them; a probe that peeks at its test rows fails it)
  seven        seven classes independent of X: |accuracy - majority| <= 0.05
"""
import numpy as np
import pytest
import torch

import probe_ref as R

pytestmark = pytest.mark.gpu

L = R.LEAK
CONFIG = {"leakage_probe_hidden": L["hidden"], "leakage_probe_epochs": L["epochs"], "leakage_probe_batch": L["batch"],
          "leakage_probe_lr": L["lr"], "leakage_probe_test_ratio": L["test_ratio"], "seed": L["seed"], "metric_decimal_place": 6}
_refs = {}


def _both(kind):
    """(the package's keys, the float64 reference's metrics) on one data set; each computed once"""
    if kind not in _refs:
        from fairrec.evaluator.leakage import probe_leakage
        X, y = R.leak_data(kind)
        got = probe_leakage(torch.from_numpy(X).cuda(), {"a": torch.from_numpy(y.astype(np.float32))}, CONFIG)
        ref = R.probe_f64(X, {"a": y}, L["hidden"], L["epochs"], L["batch"], L["lr"], L["test_ratio"], L["seed"])["a"]
        print(kind, got, ref)
        _refs[kind] = ({k.split()[1]: v for k, v in got.items()}, ref)
        assert set(got) == {f"leakage {m} of sensitive attribute a" for m in ("auc", "accuracy", "majority", "logloss")}
    return _refs[kind]


def test_planted_signal_is_found():
    got, _ = _both("planted")
    assert got["auc"] >= 0.9


def test_independent_attribute_leaks_nothing():
    got, _ = _both("independent")
    assert abs(got["auc"] - 0.5) <= 0.06


def test_seven_independent_classes_sit_at_the_majority_rate():
    got, _ = _both("seven")
    assert abs(got["accuracy"] - got["majority"]) <= 0.05


@pytest.mark.parametrize("kind", ["planted", "independent", "seven"])
def test_same_split_and_init_as_the_reference(kind):
    """the majority share is a function of the split alone: exact; the trained numbers follow the float64 procedure closely
    (160 float32 Adam steps from the same init on the same batches: far inside 0.02)"""
    got, ref = _both(kind)
    assert abs(got["majority"] - ref["majority"]) <= 1e-6
    assert abs(got["auc"] - ref["auc"]) <= 0.02 and abs(got["accuracy"] - ref["accuracy"]) <= 0.02
    assert abs(got["logloss"] - ref["logloss"]) <= 0.02


def test_linear_probe_and_several_attributes_in_one_run():
    from fairrec.evaluator.leakage import probe_leakage
    X, y = R.leak_data("planted")
    _, y7 = R.leak_data("seven")
    cfg = dict(CONFIG, leakage_probe_hidden=0, leakage_probe_epochs=5)
    got = probe_leakage(torch.from_numpy(X).cuda(), {"g": torch.from_numpy(y), "s": torch.from_numpy(y7 * 3 + 1)}, cfg)
    ref = R.probe_f64(X, {"g": y, "s": y7}, 0, 5, L["batch"], L["lr"], L["test_ratio"], L["seed"])
    assert len(got) == 8
    for name in ("g", "s"):
        for m in ("auc", "accuracy", "logloss"):
            assert abs(got[f"leakage {m} of sensitive attribute {name}"] - ref[name][m]) <= 0.02, (name, m)
    assert got["leakage auc of sensitive attribute g"] >= 0.9


def test_refusals_name_the_key_or_the_attribute():
    from fairrec.evaluator.leakage import probe_leakage
    X = torch.randn(50, 4)
    y = {"a": torch.arange(50) % 2}
    for key, bad in (("leakage_probe_hidden", 257), ("leakage_probe_hidden", 1.5), ("leakage_probe_epochs", 0),
                     ("leakage_probe_batch", 0), ("leakage_probe_batch", 65537), ("leakage_probe_lr", 0.0),
                     ("leakage_probe_test_ratio", 1.0), ("leakage_probe", "yes")):
        with pytest.raises(ValueError, match=key):
            probe_leakage(X, y, dict(CONFIG, **{key: bad}))
    one_class_in_test = torch.zeros(50, dtype=torch.int64)
    g = torch.Generator().manual_seed(CONFIG["seed"])
    perm = torch.randperm(50, generator=g)
    one_class_in_test[perm[10:]] = torch.arange(40) % 2          # the 10 test rows all hold class 0
    with pytest.raises(ValueError, match="attribute b.*test"):
        probe_leakage(X, {"b": one_class_in_test}, CONFIG)
    with pytest.raises(ValueError, match="only one value for c"):
        probe_leakage(X, {"c": torch.zeros(50)}, CONFIG)


# ---- the trainers ----------------------------------------------------------------------------------------------------------------

COMMON = {"epochs": 3, "train_batch_size": 512, "synthetic_users": 400, "synthetic_items": 80, "synthetic_interactions": 6000,
          "device": "cuda", "embedding_size": 16, "eval_args": {"mode": "full"}, "topk": [5], "valid_metric": "ndcg@5",
          "valid_metric_bigger": True, "metrics": ["NDCG", "Recall", "DifferentialFairness"], "sst_attr_list": ["gender"],
          "eval_batch_size": 4096, "metric_decimal_place": 6, "leakage_probe_hidden": 8, "leakage_probe_epochs": 3,
          "leakage_probe_batch": 128, "leakage_probe_lr": 0.01}
LEAK_KEYS = {f"leakage {m} of sensitive attribute gender" for m in ("auc", "accuracy", "majority", "logloss")}


def _trained(tmp, **extra):
    """one small PFCN_PMF flow through run_recbole -> (trainer, the test loader and keywords its final evaluate was called with)"""
    from fairrec.quick_start import run_recbole
    seen = {}

    def before_fit(model, trainer):
        inner = trainer.evaluate

        def evaluate(eval_data, **kw):
            seen.update(trainer=trainer, data=eval_data, kw=kw, evaluate=inner)
            return inner(eval_data, **kw)
        trainer.evaluate = evaluate

    run_recbole(model="PFCN_PMF", config_dict=dict(COMMON, checkpoint_dir=str(tmp), **extra), before_fit=before_fit)
    return seen


def _evaluate(seen, probe):
    """the trainer's final evaluation again, with or without the probe, from the same generator states (the filters of a
    filtered model run in training mode during evaluation)"""
    seen["trainer"].config["leakage_probe"] = True if probe else None
    torch.manual_seed(5)
    np.random.seed(5)
    return seen["evaluate"](seen["data"], **seen["kw"])


@pytest.mark.parametrize("mode", ["none", "sm"])
def test_trainer_adds_the_keys_and_changes_no_other(tmp_path, mode):
    extra = dict(filter_mode=mode) if mode == "none" else dict(filter_mode=mode, dis_hidden_size_list=[16, 8], train_epoch_interval=1)
    seen = _trained(tmp_path, save_sst_embed=(mode == "none"), **extra)
    plain, probed, plain_again = _evaluate(seen, False), _evaluate(seen, True), _evaluate(seen, False)
    assert list(plain) == list(probed) == (["none"] if mode == "none" else ["sm-['gender']"])
    for sub, res in plain.items():
        assert not LEAK_KEYS & set(res) and "ndcg@5" in res
        assert set(probed[sub]) == set(res) | LEAK_KEYS
        for k, v in res.items():
            assert probed[sub][k] == v or (np.isnan(v) and np.isnan(probed[sub][k])), (sub, k)
            assert plain_again[sub][k] == v or (np.isnan(v) and np.isnan(plain_again[sub][k])), (sub, k)      # nothing left behind
        assert all(np.isfinite(probed[sub][k]) for k in LEAK_KEYS)
        assert 0.0 <= probed[sub]["leakage auc of sensitive attribute gender"] <= 1.0
    if mode == "none":
        from fairrec.utils.leakage import probe_file
        path = tmp_path / "PFCN_PMF_embed-none.pth"
        assert path.exists()
        again = probe_file(str(path), seen["trainer"].config)
        assert again == {k: probed["none"][k] for k in LEAK_KEYS}


def test_a_model_without_get_sst_embed_points_to_probe_leakage(tmp_path):
    from fairrec.quick_start import run_recbole
    with pytest.raises(ValueError, match="probe_leakage"):
        run_recbole(model="FOCF", config_dict=dict(COMMON, checkpoint_dir=str(tmp_path), fair_objective="value", epochs=1,
                                                   leakage_probe=True))

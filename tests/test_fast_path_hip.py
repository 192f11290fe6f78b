"""GPU: which path serves a call -- not what it computes.  Untrained models on the dataset of tests/test_case_study_hip.py (150
users x 300 items, 4000 interactions); `functional.recommend_topk`, `pair_mlp_scores`, `dyn_neg_dot_select`,
`dyn_neg_mlp_select` and the model's `predict` / `full_sort_predict` are wrapped with call counters (Python wrappers only), and every row asserts
which of them ran for `full_sort_topk`, for `Trainer.evaluate` under `full_sort_eval: fused` and `matrix`, and for one
loader batch of dynamic negatives.  A decline rule that turns true by mistake moves no value beyond rounding -- the dense path
serves the call -- so the value tests cannot see it; these counters do."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

COMMON = {"device": DEV, "embedding_size": 16, "train_batch_size": 200, "eval_args": {"mode": "full"}, "topk": [5, 10],
          "metrics": ["NDCG", "Recall", "Hit", "MRR"], "sst_attr_list": ["gender"], "eval_batch_size": 4096, "seed": 5}
PFCN_SM = dict(filter_mode="sm", dis_hidden_size_list=[16, 8])
MLP = dict(filter_mode="none", mlp_hidden_size_list=[16, 8])
NFCF = dict(mlp_hidden_size=[16, 8], load_pretrain_path=None, LABEL_FIELD="label")
FULL_SORT = {                       # case: (model, config, attribute subset, path)
    "PFCN_PMF-none": ("PFCN_PMF", dict(filter_mode="none"), None, "fused"),
    "PFCN_BiasedMF-sm": ("PFCN_BiasedMF", PFCN_SM, ["gender"], "fused"),
    "PFCN_DMF-towers": ("PFCN_DMF", dict(PFCN_SM, num_layers=2, mlp_dropout=0.0, full_sort_scorer="towers"), ["gender"], "fused"),
    "FOCF": ("FOCF", dict(fair_objective="value"), None, "fused"),
    "FairGo_PMF": ("FairGo_PMF", dict(n_layers=2, dis_hidden_size_list=[16, 8, 4], filter_hidden_size_list=[32, 16],
                                      neg_sampling=None), None, "fused"),
    "NFCF-split": ("NFCF", dict(NFCF, full_sort_scorer="split"), None, "split"),
    "PFCN_MLP-split": ("PFCN_MLP", dict(MLP, full_sort_scorer="split"), None, "split"),
    "NFCF": ("NFCF", NFCF, None, "dense"),
    "PFCN_MLP": ("PFCN_MLP", MLP, None, "dense"),
    "PFCN_DMF-pairs": ("PFCN_DMF", dict(PFCN_SM, num_layers=2, mlp_dropout=0.0), ["gender"], "dense"),
}
DYNAMIC = {                         # case: (model, config, in training mode, the one function that rates the candidates)
    "PFCN_PMF": ("PFCN_PMF", dict(filter_mode="none"), False, "dyn_neg_dot_select"),
    "NFCF-split": ("NFCF", dict(NFCF, dynamic_neg_scorer="split"), False, "dyn_neg_mlp_select"),
    "PFCN_MLP-split": ("PFCN_MLP", dict(MLP, dynamic_neg_scorer="split"), False, "dyn_neg_mlp_select"),
    "NFCF-pairs": ("NFCF", dict(NFCF, dynamic_neg_scorer="pairs"), False, "predict"),
    "NFCF-split-dropout": ("NFCF", dict(NFCF, dynamic_neg_scorer="split", dropout=0.2), True, "predict"),
}
COUNTED = ("recommend_topk", "pair_mlp_scores", "dyn_neg_dot_select", "dyn_neg_mlp_select")


def _setup(model_name, extra, tmp_path, dynamic=False):
    """(model, trainer, full-sort test loader, training loader) without a training run."""
    from fairrec.config import Config
    from fairrec.data.dataloader import FullSortEvalDataLoader, TrainDataLoader
    from fairrec.data.dataset import synthetic_dataset
    from fairrec.quick_start import split_dataset
    from fairrec.sampler import Sampler
    from fairrec.utils import get_model, get_trainer, init_seed
    more = {"neg_sampling": {"uniform": 1, "dynamic": 4}} if dynamic else {}
    cfg = Config(model=model_name, config_dict=dict(COMMON, checkpoint_dir=str(tmp_path), **more, **extra))
    init_seed(cfg["seed"], cfg["reproducibility"])
    parts = split_dataset(synthetic_dataset(cfg, 150, 300, 4000, seed=5))
    phases = Sampler(["train", "valid", "test"], list(parts), "uniform", device=DEV)
    test_data = FullSortEvalDataLoader(cfg, parts[2], phases.set_phase("test"))
    train_data = None
    if dynamic:
        sampler = Sampler(["train", "valid", "test"], list(parts), "uniform", device=DEV).set_phase("train")
        train_data = TrainDataLoader(cfg, parts[0].to(DEV), sampler=sampler, shuffle=False)
    model = get_model(model_name)(cfg, parts[0]).to(DEV)
    return model, get_trainer(None, model_name)(cfg, model), test_data, train_data


def _count(monkeypatch, model):
    from fairrec import functional as F
    from fairrec.model.abstract_recommender import AbstractRecommender
    calls = dict.fromkeys(COUNTED + ("predict",), 0)

    def counting(name, real):
        def wrapper(*a, **kw):
            calls[name] += 1
            return real(*a, **kw)
        return wrapper

    for name in COUNTED:
        monkeypatch.setattr(F, name, counting(name, getattr(F, name)))
    monkeypatch.setattr(model, "predict", counting("predict", model.predict))
    if type(model).full_sort_predict is not AbstractRecommender.full_sort_predict:      # (FOCF, FairGo_PMF: their dense path)
        monkeypatch.setattr(model, "full_sort_predict", counting("predict", model.full_sort_predict))
    return calls


def _took(calls, path):
    """The counters of one call under `path`; resets them."""
    seen = {k: v > 0 for k, v in calls.items()}
    for k in calls:
        calls[k] = 0
    want = {"fused": {"recommend_topk"}, "split": {"pair_mlp_scores"}, "dense": {"predict"}, "matrix": {"predict"}}[path]
    return {k for k, v in seen.items() if v} == want


@pytest.mark.parametrize("case", list(FULL_SORT))
def test_full_sort_calls_take_their_path(case, tmp_path, monkeypatch):
    from fairrec.utils.case_study import full_sort_scores, full_sort_topk
    model_name, extra, sst_list, path = FULL_SORT[case]
    model, trainer, test_data, _ = _setup(model_name, extra, tmp_path)
    calls = _count(monkeypatch, model)
    uids = test_data.uid_list[:13]
    full_sort_topk(uids, model, test_data, 10, sst_list=sst_list)
    assert _took(calls, path), (case, "full_sort_topk")
    full_sort_scores(uids, model, test_data, sst_list=sst_list)
    assert _took(calls, path), (case, "full_sort_scores")
    assert trainer.full_sort_eval == "matrix"
    trainer.evaluate(test_data)
    assert _took(calls, "matrix" if path == "fused" else path), (case, "evaluate under matrix")
    monkeypatch.setattr(trainer, "full_sort_eval", "fused")
    trainer.evaluate(test_data)
    assert _took(calls, path), (case, "evaluate under fused")


@pytest.mark.parametrize("case", list(DYNAMIC))
def test_a_dynamic_negatives_batch_takes_its_path(case, tmp_path, monkeypatch):
    model_name, extra, training, path = DYNAMIC[case]
    model, _, _, dl = _setup(model_name, extra, tmp_path, dynamic=True)
    dl.get_model(model)
    calls = _count(monkeypatch, model)
    if training:        # the loader rates candidates in eval mode; a model that stays in training mode drops out while it does
        monkeypatch.setattr(model, "eval", lambda: model)
        model.train()
    neg = dl._dynamic_negatives(dl.dataset[0:dl.step])
    assert neg.shape == (dl.step,) and neg.dtype == torch.int64
    assert {k for k, v in calls.items() if v} == {path} and calls[path] == 1, (case, calls)

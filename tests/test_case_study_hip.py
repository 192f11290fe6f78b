"""GPU: recbole.utils.case_study on trained models -- FOCF, PFCN_BiasedMF (filter_mode none and sm) and FairGo_PMF through the
fused kernel, NFCF through the dense scores and fr_topk_rows -- against the dense scores the Trainer's full-sort evaluation
ranks (utils/case_study.dense_full_sort_scores, masked as the Trainer masks them).

NFCF: the lists equal the restatement of the total order on those scores, in bits and ids.  Fused models: their dense path
sums in another order (FairGo: torch.matmul), so the rules of tests/test_recommend_hip.py check 3 hold against the dense
scores with tau = gamma_D * sum_d |x w| (+ 4 ulp for the epilogue) of the factors the model hands to the kernel; and the
lists equal the restatement on the model's own full_sort_scores exactly."""
import numpy as np
import pytest
import torch

import recommend_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = 10

COMMON = {"epochs": 1, "train_batch_size": 512, "synthetic_users": 150, "synthetic_items": 300, "synthetic_interactions": 4000,
          "device": DEV, "embedding_size": 16, "eval_args": {"mode": "full"}, "topk": [5, 10], "valid_metric": "ndcg@10",
          "valid_metric_bigger": True, "metrics": ["NDCG", "Recall", "Hit", "MRR"], "sst_attr_list": ["gender"],
          "eval_batch_size": 4096, "metric_decimal_place": 4}
CASES = {
    "FOCF": ("FOCF", dict(fair_objective="value"), None),
    # (embedding_size 4: the model's tables start as N(0, 1); at D = 16 a user's best scores are sigmoids of 8 .. 12, a few 1e-6
    #  apart, while tau is taken on the dot product, 4e-5: 16 of the 300 items then sit inside the 2 tau band of check 3 -- the
    #  float64 restatement on N(0, 1) data of this shape gives 16 at D = 16, 3 at D = 8, 1 at D = 4 -- and the check's
    #  condition, at most 8, is one on the data)
    "PFCN_BiasedMF-none": ("PFCN_BiasedMF", dict(filter_mode="none", embedding_size=4), None),
    "PFCN_BiasedMF-sm": ("PFCN_BiasedMF", dict(filter_mode="sm", dis_hidden_size_list=[16, 8], train_epoch_interval=1,
                                               learning_rate=0.01), ["gender"]),
    "FairGo_PMF": ("FairGo_PMF", dict(pretrain_epochs=1, train_epoch_interval=1, n_layers=2, dis_hidden_size_list=[16, 8, 4],
                                      filter_hidden_size_list=[32, 16], neg_sampling=None), None),
    "NFCF": ("NFCF", dict(mlp_hidden_size=[16, 8], load_pretrain_path=None, LABEL_FIELD="label"), None),
}


def _train(case, tmp_path, monkeypatch):
    from fairrec.data.dataloader import FullSortEvalDataLoader
    from fairrec.quick_start import run_recbole
    model_name, extra, sst_list = CASES[case]
    seen, loaders = {}, []
    init = FullSortEvalDataLoader.__init__

    def recording_init(self, *a, **kw):
        init(self, *a, **kw)
        loaders.append(self)

    monkeypatch.setattr(FullSortEvalDataLoader, "__init__", recording_init)

    def before_fit(m, trainer):
        seen["model"], seen["trainer"] = m, trainer

    run_recbole(model=model_name, config_dict=dict(COMMON, checkpoint_dir=str(tmp_path), **extra), before_fit=before_fit)
    monkeypatch.undo()
    return seen["model"], seen["trainer"], loaders[-1], sst_list          # the test loader is built last


def _dense(model, test_data, uids, sst_list):
    """The helper's scores of `uids`, masked as Trainer._ranking_evaluate masks them."""
    from fairrec.data.interaction import Interaction
    from fairrec.utils.case_study import dense_full_sort_scores, users_per_batch
    ds = test_data.dataset
    inter = ds.join(Interaction({ds.uid_field: uids})).to(DEV)
    model.eval()
    with torch.no_grad():
        s = dense_full_sort_scores(model, inter, ds.item_num, users_per_batch(test_data.config, ds.item_num), ds.iid_field,
                                   torch.device(DEV), sst_list).float().clone()
    s[:, 0] = -float("inf")
    hu, hi = test_data._rows(test_data.hist_indptr, test_data.hist_items, uids)
    s[hu, hi] = -float("inf")
    return s.cpu().numpy()


@pytest.mark.parametrize("case", list(CASES))
def test_full_sort_topk_and_scores(case, tmp_path, monkeypatch):
    import recbole.utils.case_study as aliased
    from fairrec import _C
    from fairrec.utils import case_study
    from fairrec.utils.case_study import full_sort_scores, full_sort_topk, users_per_batch
    assert aliased is case_study and aliased.full_sort_topk is full_sort_topk
    model, trainer, test_data, sst_list = _train(case, tmp_path, monkeypatch)
    before = trainer.evaluate(test_data)
    every = test_data.uid_list
    rng = np.random.default_rng(2)
    n_items = test_data.dataset.item_num
    # with repeats, and as long as a whole number of the evaluation's predict batches: a last batch of ONE user has zero variance
    # in the filters' BatchNorm statistics, where the dense path's scores of that user are its own rounding noise over sqrt(eps)
    per = users_per_batch(test_data.config, n_items)
    extra = 7 + (-(len(every) + 7)) % per
    shuffled = torch.from_numpy(rng.permutation(np.concatenate([every.cpu().numpy(), every.cpu().numpy()[:extra]]))).to(DEV)
    assert len(shuffled) % per == 0 and len(shuffled) >= len(every) + 7
    for uids, given in ((every, every.cpu().numpy()), (shuffled, shuffled.cpu().tolist())):      # an array and a plain list
        val, idx = full_sort_topk(given, model, test_data, K, sst_list=sst_list)
        scores = full_sort_scores(given, model, test_data, sst_list=sst_list)
        assert val.shape == idx.shape == (len(uids), K) and scores.shape == (len(uids), n_items)
        assert idx.dtype == torch.int64 and val.dtype == torch.float32 and val.is_cuda
        val, idx, scores = val.cpu().numpy(), idx.cpu().numpy(), scores.cpu().numpy()
        dense = _dense(model, test_data, uids, sst_list)
        # -inf exactly at the pad item and the history cells
        assert np.array_equal(np.isneginf(scores), np.isneginf(dense)) and np.isneginf(dense[:, 0]).all()
        assert np.isfinite(scores[~np.isneginf(scores)]).all()
        # the lists are the total order's on the model's own scores, bit for bit
        rv, ri = R.topk(scores, K)
        np.testing.assert_array_equal(idx, ri)
        assert R.same_bits(val, rv)
        if case == "NFCF":
            assert model.full_sort_factors(None) is None
            assert R.same_bits(scores, dense)
        else:
            ds = test_data.dataset
            from fairrec.data.interaction import Interaction
            with torch.no_grad():
                f = model.full_sort_factors(ds.join(Interaction({ds.uid_field: uids})).to(DEV), sst_list,
                                            users_per_batch=users_per_batch(test_data.config, n_items))
            assert f is not None
            X, W = f["X"].double().cpu().numpy(), f["W"].double().cpu().numpy()
            tau = R.gamma(X.shape[1]) * (np.abs(X) @ np.abs(W).T)
            if f.get("epilogue", 0):
                fin = np.where(np.isfinite(dense), dense, 0).astype(np.float32)
                tau = tau + 4.0 * np.spacing(np.abs(fin)).astype(np.float64)
            fin = np.isfinite(dense)
            diff = np.abs(scores.astype(np.float64)[fin] - dense[fin])
            spread = np.where(fin, dense, np.nan)
            print(f"{case}: max |fused - dense| = {diff.max():.3g}, max |fused - dense| / tau = {(diff / tau[fin]).max():.3g}, "
                  f"median spread of a user's scores = {np.median(np.nanmax(spread, 1) - np.nanmin(spread, 1)):.3g}")
            assert np.all(diff <= tau[fin])
            worst = R.check_band(val, idx, dense.astype(np.float64), tau, K)
            print(f"{case}: at most {worst} items of a user within 2 tau of its k-th best")
    with pytest.raises(ValueError, match="256"):
        full_sort_topk(every, model, test_data, 257, sst_list=sst_list)
    with pytest.raises(_C.FairrecError):
        full_sort_topk(every, model, test_data, K, device="cpu", sst_list=sst_list)
    assert trainer.evaluate(test_data) == before         # the calls left the engine's state as they found it

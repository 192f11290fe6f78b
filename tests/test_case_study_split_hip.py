"""GPU: `full_sort_scorer: split` end to end -- NFCF and PFCN_MLP (filter_mode none and sm) trained through run_recbole at
the sizes of tests/test_case_study_hip.py, then recbole.utils.case_study and the Trainer's full-sort evaluation on the split
scorer (fr_pair_mlp_scores) against the dense path (`predict` on every pair) and the float64 restatement with its running
bound (tests/pair_mlp_ref.py).

The scorer's parameters are overwritten after training by a seeded draw (`_set_scorer`: seed 7, scale 1, weights
N(0, 1 / n_in), biases N(0, 1/4)): check_band's condition, at most 8 items of a user within 2 tau of its k-th best, is one
on the data, and an MLP that ends in a ReLU can score most items sigmoid(0) = 0.5 exactly.  Checked on the CPU with the
float64 reference alone, N(0, 1) and N(0, 0.09) user rows against N(0, 1) item rows of this shape (150 x 300, D = 16,
[32, 16, 8, 1]), three table seeds each: seeds 3, 6 and 7 at scale 1 give a largest band of 2 (5 % of the cells at 0.5 for
seed 7); seeds 0, 4, 5 give 299 (two thirds or more of the cells at 0.5), and scale 2 up to 299 for every seed tried."""
import numpy as np
import pytest
import torch

import pair_mlp_ref as P
import recommend_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = 10
D = 16

COMMON = {"epochs": 1, "train_batch_size": 512, "synthetic_users": 150, "synthetic_items": 300, "synthetic_interactions": 4000,
          "device": DEV, "embedding_size": D, "eval_args": {"mode": "full"}, "topk": [5, 10], "valid_metric": "ndcg@10",
          "valid_metric_bigger": True, "metrics": ["NDCG", "Recall", "Hit", "MRR"], "sst_attr_list": ["gender"],
          "eval_batch_size": 4096, "metric_decimal_place": 4}
CASES = {
    "NFCF": ("NFCF", dict(mlp_hidden_size=[16, 8], load_pretrain_path=None, LABEL_FIELD="label"), None),
    "PFCN_MLP-none": ("PFCN_MLP", dict(filter_mode="none", mlp_hidden_size_list=[16, 8]), None),
    "PFCN_MLP-sm": ("PFCN_MLP", dict(filter_mode="sm", mlp_hidden_size_list=[16, 8], dis_hidden_size_list=[16, 8],
                                     train_epoch_interval=1, learning_rate=0.01), ["gender"]),
}


def _train(case, tmp_path, monkeypatch, **more):
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

    run_recbole(model=model_name, config_dict=dict(COMMON, checkpoint_dir=str(tmp_path), **extra, **more), before_fit=before_fit)
    monkeypatch.undo()
    return seen["model"], seen["trainer"], loaders[-1], sst_list          # the test loader is built last


def _scorer(model):
    return model.mlp_layers if hasattr(model, "mlp_layers") else model.mlp_layer


def _set_scorer(model, seed=7, scale=1.0):
    """The scorer's parameters, in place, from a seeded draw (the module's docstring says which were checked)."""
    lins = _scorer(model).linears()
    widths = [lin.out_features for lin in lins]
    rng = np.random.default_rng(seed)
    W1 = (scale * rng.standard_normal((widths[0], 2 * D)) / np.sqrt(2 * D)).astype(np.float32)
    b1 = (0.5 * rng.standard_normal(widths[0])).astype(np.float32)
    with torch.no_grad():
        for lin, (W, b) in zip(lins, [(W1, b1)] + P.random_layers(rng, widths, scale)):
            lin.weight.copy_(torch.from_numpy(W))
            lin.bias.copy_(torch.from_numpy(b))


def _dense(model, test_data, uids, sst_list):
    """The dense path's scores of `uids`, masked as Trainer._ranking_evaluate masks them."""
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


def _user_rows(model, uids, sst_list, per, n_items, repeated):
    """The user rows a path feeds its scorer: looked up (NFCF), or filtered `per` users at a time (PFCN_MLP) -- on the rows
    themselves (the split path) or, `repeated`, on every row n_items times over as `predict` sees them (the dense path:
    under batch statistics the filters' BatchNorm sums over the repeats)."""
    model.eval()
    with torch.no_grad():
        if hasattr(model, "mlp_layers"):
            return model.hip_engine().lookup("user_embedding.weight", uids).cpu().numpy()
        out = []
        for lo in range(0, len(uids), per):
            u = uids[lo:lo + per]
            if repeated and model.filter_mode != "none":
                out.append(model.forward(u.repeat_interleave(n_items), None, sst_list)[0][::n_items])
            else:
                out.append(model.forward(u, None, sst_list)[0])
        return torch.cat(out).cpu().numpy()


def _item_rows(model, n_items):
    model.hip_engine().flush()
    table = model.item_embedding if hasattr(model, "mlp_layers") else getattr(model, model.item_table_attr)
    return table.weight.detach()[:n_items].cpu().numpy()


@pytest.mark.parametrize("case", list(CASES))
def test_split_scorer_end_to_end(case, tmp_path, monkeypatch):
    from fairrec.data.interaction import Interaction
    from fairrec.utils.case_study import full_sort_scores, full_sort_topk, users_per_batch
    model, trainer, test_data, sst_list = _train(case, tmp_path, monkeypatch, full_sort_scorer="split")
    _set_scorer(model)
    ds = test_data.dataset
    n_items = ds.item_num
    per = users_per_batch(test_data.config, n_items)
    sst_lists = (sst_list,)
    before = trainer.evaluate(test_data)
    assert trainer.evaluate(test_data) == before
    every = test_data.uid_list
    rng = np.random.default_rng(2)
    extra = 7 + (-(len(every) + 7)) % per          # whole predict batches (tests/test_case_study_hip.py says why)
    shuffled = torch.from_numpy(rng.permutation(np.concatenate([every.cpu().numpy(), every.cpu().numpy()[:extra]]))).to(DEV)
    W1, b1, layers = P.pieces_of_module(_scorer(model))
    w = _item_rows(model, n_items)
    for uids in (every, shuffled):
        inter = ds.join(Interaction({ds.uid_field: uids})).to(DEV)
        model.eval()
        with torch.no_grad():
            assert model.full_sort_pair_mlp(inter, sst_list, users_per_batch=per) is not None
        val, idx = full_sort_topk(uids, model, test_data, K, sst_list=sst_list)
        scores = full_sort_scores(uids, model, test_data, sst_list=sst_list)
        assert val.shape == idx.shape == (len(uids), K) and scores.shape == (len(uids), n_items)
        assert idx.dtype == torch.int64 and val.dtype == torch.float32 and val.is_cuda
        val, idx, scores = val.cpu().numpy(), idx.cpu().numpy(), scores.cpu().numpy()
        dense = _dense(model, test_data, uids, sst_list)
        masked = np.isneginf(dense)
        assert np.array_equal(np.isneginf(scores), masked) and masked[:, 0].all()
        assert np.isfinite(scores[~masked]).all()
        # the lists are the total order's on exactly the scores full_sort_scores returns
        rv, ri = R.topk(scores, K)
        np.testing.assert_array_equal(idx, ri)
        assert R.same_bits(val, rv)
        # both paths against float64 on the rows each feeds its scorer, and against each other
        xs = _user_rows(model, uids, sst_list, per, n_items, repeated=False)
        xd = _user_rows(model, uids, sst_list, per, n_items, repeated=True)
        s_split, b_split = P.bound_rows(xs, w, W1, b1, layers, split=True)
        s_dense, b_dense = P.bound_rows(xd, w, W1, b1, layers, split=False)
        live = ~masked
        e_split = np.abs(scores.astype(np.float64) - s_split)[live]
        e_dense = np.abs(dense.astype(np.float64) - s_dense)[live]
        gap = np.abs(scores.astype(np.float64) - dense.astype(np.float64))[live]
        moved = np.abs(s_split - s_dense)[live]          # 0 unless the filters' batch statistics saw the repeats
        print(f"{case}: max |split - f64| / bound = {(e_split / b_split[live]).max():.3g}, max |dense - f64| / bound = "
              f"{(e_dense / b_dense[live]).max():.3g}, max |split - dense| = {gap.max():.3g} against "
              f"{(b_split + b_dense)[live].max():.3g}, rows moved the f64 scores by {moved.max():.3g}, "
              f"cells at 0.5: {np.mean(scores[live] == 0.5):.3g}")
        assert np.all(e_split <= b_split[live])
        assert np.all(gap <= (b_split + b_dense)[live] + moved)
        s64 = np.where(masked, -np.inf, s_split)
        worst = R.check_band(val, idx, s64, b_split, K)
        print(f"{case}: at most {worst} items of a user within 2 tau of its k-th best")
    # the Trainer's evaluation ranks the same bits
    model.eval()
    seen = 0
    for user_df, (hist_u, hist_i), positive_u, positive_i in test_data:
        user_df = user_df.to(DEV)
        with torch.no_grad():
            got = trainer._full_sort_scores(user_df, n_items, sst_list)
        uids = user_df[ds.uid_field]
        want = full_sort_scores(uids, model, test_data, sst_list=sst_list)
        keep = ~torch.isneginf(want)
        assert got.shape == want.shape and torch.equal(got[keep].view(torch.int32), want[keep].view(torch.int32))
        seen += len(uids)
    assert seen >= len(every)
    assert trainer.evaluate(test_data) == before         # the calls left the engine's state as they found it


@pytest.mark.parametrize("case", ["NFCF", "PFCN_MLP-sm"])
def test_default_key_is_the_dense_path(case, tmp_path, monkeypatch):
    from fairrec.data.interaction import Interaction
    from fairrec.utils.case_study import full_sort_scores, users_per_batch
    model, trainer, test_data, sst_list = _train(case, tmp_path, monkeypatch)
    assert model.full_sort_scorer == "pairs"
    ds = test_data.dataset
    every = test_data.uid_list
    per = users_per_batch(test_data.config, ds.item_num)
    uids = every[:len(every) // per * per]
    inter = ds.join(Interaction({ds.uid_field: uids})).to(DEV)
    model.eval()
    with torch.no_grad():
        assert model.full_sort_pair_mlp(inter, sst_list, users_per_batch=per) is None
    scores = full_sort_scores(uids, model, test_data, sst_list=sst_list).cpu().numpy()
    assert R.same_bits(scores, _dense(model, test_data, uids, sst_list))

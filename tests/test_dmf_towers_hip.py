"""GPU: PFCN_DMF with `full_sort_scorer: towers` -- the tower outputs normalised once per user and once per item
(fr_rows_l2_normalize) and ranked as a dot-product model by the fused kernels -- against `pairs`, the dense path.

Synthetic models as tests/test_case_study_hip.py trains them: 40 users x 71 items (three 32-item steps of the ranking kernel
with a ragged last one, two user tiles with a ragged second), embedding_size 8 and one case at 65 (two fragments), two tower
layers, one epoch of two steps (the tables stay lazily stale), filter_mode none, sm, and sm on the running
statistics.  Training runs without dropout (mlp_dropout, dis_dropout 0): a module's dropout stream is seeded with the number
of MLP modules the process built before it, so the trained tables, and every figure below, would depend on which tests ran
earlier.  eval_batch_size 568 = 8 users per predict batch, so the filters see five groups.  After training the towers'
and filters' Linear layers are overwritten by a seeded draw, weights N(0, 1 / n_in) and biases N(0, 1 / 16): the trained ones
(N(0, 1e-4) at initialisation, two steps later) leave most ReLU towers dead, and every score would be sigmoid(0).

Measured on an MI355X (maxima over the unmasked cells; ref64 = predict restated in float64 from the fp32 parameters):
    case          e_pairs = max |pairs - ref64|    max |towers - ref64|    allowance 2 e_pairs
    none          8.78e-8                          7.86e-8                 1.76e-7
    sm            1.43e-7                          1.49e-7                 2.86e-7
    sm-running    9.48e-8                          8.55e-8                 1.90e-7
    sm-65         8.77e-8                          8.39e-8                 1.75e-7
and in every case the item `towers` ranks r-th has exactly the dense path's r-th score (HISTORY.md, "PFCN_DMF from tower
outputs").
"""
import copy

import numpy as np
import pytest
import torch

import recommend_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_ITEMS = 71
PER = 8
U = 2.0 ** -24

COMMON = {"epochs": 1, "train_batch_size": 1024, "synthetic_users": 41, "synthetic_items": N_ITEMS, "synthetic_interactions": 2000,
          "device": DEV, "embedding_size": 8, "eval_args": {"mode": "full"}, "topk": [5, 10], "valid_metric": "ndcg@10",
          "valid_metric_bigger": True, "sst_attr_list": ["gender"], "eval_batch_size": PER * N_ITEMS, "metric_decimal_place": 4,
          "popularity_ratio": 0.1, "tail_ratio": 0.1, "num_layers": 2, "dis_hidden_size_list": [16, 8], "train_epoch_interval": 1,
          "learning_rate": 0.01, "mlp_dropout": 0.0, "dis_dropout": 0.0,
          "metrics": ["Hit", "MRR", "NDCG", "Recall", "Precision", "GiniIndex", "ItemCoverage", "NonParityUnfairness",
                      "DifferentialFairness", "GAUC"]}
CASES = {
    "none": (dict(filter_mode="none"), None),
    "sm": (dict(filter_mode="sm"), ["gender"]),
    "sm-running": (dict(filter_mode="sm", filter_eval_statistics="running"), ["gender"]),
    "sm-65": (dict(filter_mode="sm", embedding_size=65), ["gender"]),
}
_trained = {}


def _set_linears(model, seed=11):
    rng = np.random.default_rng(seed)
    mlps = [model.user_mlp, model.item_mlp] + [model.filter_layer[k] for k in sorted(getattr(model, "filter_layer", {}))]
    with torch.no_grad():
        for mlp in mlps:
            for lin in mlp.linears():
                w = rng.standard_normal(tuple(lin.weight.shape)) / np.sqrt(lin.in_features)
                lin.weight.copy_(torch.from_numpy(w.astype(np.float32)))
                lin.bias.copy_(torch.from_numpy((0.25 * rng.standard_normal(lin.out_features)).astype(np.float32)))


def _train(case, tmp_path_factory):
    """(model, trainer, test loader, attribute subset, users) of a case, trained once for the tests below; the users are whole
    predict batches (a last batch of ONE user has zero variance in the filters' BatchNorm statistics)."""
    if case not in _trained:
        from fairrec.data.dataloader import FullSortEvalDataLoader
        from fairrec.quick_start import run_recbole
        extra, sst_list = CASES[case]
        seen, loaders = {}, []
        init = FullSortEvalDataLoader.__init__

        def recording_init(self, *a, **kw):
            init(self, *a, **kw)
            loaders.append(self)

        FullSortEvalDataLoader.__init__ = recording_init
        try:
            run_recbole(model="PFCN_DMF", config_dict=dict(COMMON, checkpoint_dir=str(tmp_path_factory.mktemp(case)), **extra),
                        before_fit=lambda m, trainer: seen.update(model=m, trainer=trainer))
        finally:
            FullSortEvalDataLoader.__init__ = init
        model, test_data = seen["model"], loaders[-1]          # the test loader is built last
        assert model.full_sort_scorer == "pairs" and test_data.dataset.item_num == N_ITEMS
        _set_linears(model)
        every = test_data.uid_list
        uids = every[:len(every) // PER * PER]
        assert len(uids) >= 3 * PER
        _trained[case] = (model, seen["trainer"], test_data, sst_list, uids)
    return _trained[case]


class _Scorer:
    """The model with its key set for the length of a `with` block."""

    def __init__(self, model, name):
        self.model, self.name = model, name

    def __enter__(self):
        self.was, self.model.full_sort_scorer = self.model.full_sort_scorer, self.name

    def __exit__(self, *exc):
        self.model.full_sort_scorer = self.was


def _inter(test_data, uids):
    from fairrec.data.interaction import Interaction
    ds = test_data.dataset
    return ds.join(Interaction({ds.uid_field: uids})).to(DEV)


def _factors(model, test_data, uids, sst_list):
    model.eval()
    with torch.no_grad():
        return model.full_sort_factors(_inter(test_data, uids), sst_list, users_per_batch=PER)


def _dense(model, test_data, uids, sst_list):
    """The dense path's scores of `uids`, masked as Trainer._ranking_evaluate masks them: the parent behaviour."""
    from fairrec.utils.case_study import dense_full_sort_scores
    ds = test_data.dataset
    model.eval()
    with torch.no_grad():
        s = dense_full_sort_scores(model, _inter(test_data, uids), ds.item_num, PER, ds.iid_field, torch.device(DEV),
                                   sst_list).float().clone()
    s[:, 0] = -float("inf")
    hu, hi = test_data._rows(test_data.hist_indptr, test_data.hist_items, uids)
    s[hu, hi] = -float("inf")
    return s.cpu().numpy()


def _mlp64(mlp, training):
    """The module's own layers as torch's standard modules in float64 on the CPU, with its fp32 parameters and buffers."""
    return copy.deepcopy(mlp.mlp_layers).cpu().double().train(training)


def _ref64(model, uids, sst_list):
    """predict() on every item restated in float64 from the fp32 parameters: towers (eval mode), the filter on the users of
    one predict batch at a time (batch statistics, whose values over a batch's repeated rows are those of its rows; or the
    running ones), cosine with eps 1e-8, sigmoid."""
    model.hip_engine().flush()
    with torch.no_grad():
        rows = getattr(model, model.user_table_attr).weight.detach()[uids].cpu().double()
        items = getattr(model, model.item_table_attr).weight.detach().cpu().double()
        a = _mlp64(model.user_mlp, False)(rows)
        if model.filter_mode != "none":
            key = sum(model.sst_dict[s] for s in sst_list)
            f = _mlp64(model.filter_layer[key], model.filter_eval_statistics == "batch")
            a = torch.cat([f(a[lo:lo + PER]) for lo in range(0, a.shape[0], PER)])
        b = _mlp64(model.item_mlp, False)(items)
        na, nb = a.norm(dim=1).clamp_min(1e-8), b.norm(dim=1).clamp_min(1e-8)
        return torch.sigmoid((a @ b.T) / (na[:, None] * nb[None, :])).numpy()


# ---- 1. the hook answers -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_the_hook_answers_under_towers_and_declines_under_pairs(case, tmp_path_factory):
    from fairrec.utils.case_study import full_sort_scores
    model, _, test_data, sst_list, uids = _train(case, tmp_path_factory)
    with _Scorer(model, "towers"):
        f = _factors(model, test_data, uids, sst_list)
        assert f is not None, "full_sort_scorer: towers is declined"
        assert set(f) == {"X", "W", "epilogue"} and f["epilogue"] == 2
        D = model.embedding_size
        assert f["X"].shape == (len(uids), D) and f["W"].shape == (N_ITEMS, D)
        for M in (f["X"], f["W"]):
            n = M.double().norm(dim=1)
            assert bool((((n - 1.0).abs() <= 8 * U) | ((n == 0) & (M == 0).all(dim=1))).all())
        empty = _factors(model, test_data, uids[:0], sst_list)
        assert empty["X"].shape == (0, D) and empty["W"].shape == (N_ITEMS, D)
        assert full_sort_scores(uids[:0], model, test_data, sst_list=sst_list).shape == (0, N_ITEMS)
    assert model.full_sort_scorer == "pairs" and _factors(model, test_data, uids, sst_list) is None
    scores = full_sort_scores(uids, model, test_data, sst_list=sst_list).cpu().numpy()
    assert R.same_bits(scores, _dense(model, test_data, uids, sst_list))


# ---- 2, 3. scores and lists ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_scores_and_lists_under_towers(case, tmp_path_factory):
    from fairrec.utils.case_study import full_sort_scores, full_sort_topk
    model, _, test_data, sst_list, uids = _train(case, tmp_path_factory)
    masked = np.isneginf(_dense(model, test_data, uids, sst_list))
    with _Scorer(model, "towers"):
        f = _factors(model, test_data, uids, sst_list)
        scores = full_sort_scores(uids, model, test_data, sst_list=sst_list).cpu().numpy()
        assert scores.shape == (len(uids), N_ITEMS) and scores.dtype == np.float32
        assert np.array_equal(np.isneginf(scores), masked) and masked[:, 0].all() and np.isfinite(scores[~masked]).all()
        s64, tau = R.scores64(f["X"].cpu().numpy(), f["W"].cpu().numpy(), epilogue=2)
        err = np.abs(scores.astype(np.float64) - s64)[~masked]
        print(f"{case}: max |towers - f64 of the factors| / tau = {(err / tau[~masked]).max():.3g}")
        assert np.all(err <= tau[~masked])
        for k in (1, 10, N_ITEMS):
            val, idx = full_sort_topk(uids, model, test_data, k, sst_list=sst_list)
            assert val.shape == idx.shape == (len(uids), k) and idx.dtype == torch.int64 and val.dtype == torch.float32
            rv, ri = R.topk(scores, k)
            np.testing.assert_array_equal(idx.cpu().numpy(), ri)
            assert R.same_bits(val.cpu().numpy(), rv)


# ---- 4. against the dense path -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_towers_against_the_dense_path(case, tmp_path_factory):
    from fairrec.utils.case_study import full_sort_scores, full_sort_topk
    model, _, test_data, sst_list, uids = _train(case, tmp_path_factory)
    pairs = _dense(model, test_data, uids, sst_list)
    live = ~np.isneginf(pairs)
    ref64 = _ref64(model, uids, sst_list)
    with _Scorer(model, "towers"):
        towers = full_sort_scores(uids, model, test_data, sst_list=sst_list).cpu().numpy()
        _, idx = full_sort_topk(uids, model, test_data, N_ITEMS, sst_list=sst_list)
    idx = idx.cpu().numpy()
    e_pairs = np.abs(pairs.astype(np.float64) - ref64)[live].max()
    e_towers = np.abs(towers.astype(np.float64) - ref64)[live].max()
    print(f"{case}: e_pairs = max |pairs - ref64| = {e_pairs:.4g}, max |towers - ref64| = {e_towers:.4g}, "
          f"max |towers - pairs| = {np.abs(towers.astype(np.float64) - pairs)[live].max():.4g}")
    assert e_pairs > 0 and e_towers <= 2 * e_pairs
    # the lists agree up to near-ties: the dense score of the item `towers` puts at rank r is the dense path's r-th value
    worst = 0.0
    for u in range(len(uids)):
        n = int(live[u].sum())
        by_dense = np.sort(pairs[u][live[u]].astype(np.float64))[::-1]
        assert live[u][idx[u, :n]].all() and len(set(idx[u, :n].tolist())) == n
        worst = max(worst, np.abs(pairs[u, idx[u, :n]].astype(np.float64) - by_dense).max())
    print(f"{case}: largest |dense score of towers' rank-r item - dense r-th value| = {worst:.4g} against {2 * e_pairs:.4g}")
    assert worst <= 2 * e_pairs


# ---- 5. request independence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["none", "sm-running"])
def test_a_users_scores_do_not_depend_on_the_request(case, tmp_path_factory):
    from fairrec.utils.case_study import full_sort_scores
    model, _, test_data, sst_list, uids = _train(case, tmp_path_factory)
    every = test_data.uid_list
    assert len(every) >= 33                  # the last user sits in the second user tile
    who = every[-1:]
    with _Scorer(model, "towers"):
        alone = full_sort_scores(who, model, test_data, sst_list=sst_list)
        first = full_sort_scores(torch.cat([who, every[:4]]), model, test_data, sst_list=sst_list)[:1]
        last = full_sort_scores(every, model, test_data, sst_list=sst_list)[-1:]
    assert alone.shape == (1, N_ITEMS)
    assert R.same_bits(alone.cpu().numpy(), first.cpu().numpy()) and R.same_bits(alone.cpu().numpy(), last.cpu().numpy())


# ---- 6. evaluation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["none", "sm"])
def test_trainer_evaluates_on_the_factors_under_fused(case, tmp_path_factory, monkeypatch):
    from fairrec.evaluator import Collector
    from fairrec.functional import recommend_topk
    from fairrec.utils.case_study import users_per_batch
    model, trainer, test_data, _, _ = _train(case, tmp_path_factory)
    assert trainer.full_sort_eval == "matrix" and users_per_batch(trainer.config, N_ITEMS) == PER
    n_fused, n_matrix = [0], [0]
    collect = Collector.eval_batch_collect_fused

    def counting(self, *a, **kw):
        n_fused[0] += 1
        return collect(self, *a, **kw)

    def unmasked(interaction, n_items, sst_list=None):
        """The fused kernel's own matrix of the batch's factors, before the masks the Trainer writes."""
        n_matrix[0] += 1
        f = model.full_sort_factors(interaction, sst_list, users_per_batch=PER)
        return recommend_topk(f["X"], f["W"], 1, want_scores=True, epilogue=f["epilogue"])[2]

    def flat(d):
        return {k: (flat(v) if isinstance(v, dict) else repr(v)) for k, v in d.items()}

    monkeypatch.setattr(Collector, "eval_batch_collect_fused", counting)
    before = trainer.evaluate(test_data, load_best_model=False)               # pairs, matrix: today's path
    monkeypatch.setattr(trainer, "full_sort_eval", "fused")
    assert flat(trainer.evaluate(test_data, load_best_model=False)) == flat(before) and n_fused[0] == 0      # pairs declines
    with _Scorer(model, "towers"):
        fused = trainer.evaluate(test_data, load_best_model=False)
        assert n_fused[0] > 0 and n_matrix[0] == 0
        monkeypatch.setattr(trainer, "full_sort_eval", "matrix")
        monkeypatch.setattr(trainer, "_full_sort_scores", unmasked)
        n_fused[0] = 0
        matrix = trainer.evaluate(test_data, load_best_model=False)
        assert n_fused[0] == 0 and n_matrix[0] > 0
    assert flat(fused) == flat(matrix)
    results = [r for r in fused.values() if isinstance(r, dict)] or [fused]
    assert all("gauc" in r and "ndcg@10" in r and "giniindex@10" in r for r in results)
    assert any(k.startswith("Differential") for k in results[0])


# ---- 7. a dead tower -----------------------------------------------------------------------------------------------------
def test_a_dead_item_tower_scores_every_item_one_half(tmp_path_factory):
    from fairrec.utils.case_study import full_sort_scores, full_sort_topk
    model, _, test_data, sst_list, uids = _train("none", tmp_path_factory)
    last = model.item_mlp.linears()[-1]
    keep = last.weight.detach().clone(), last.bias.detach().clone()
    try:
        with torch.no_grad():
            last.weight.zero_()
            last.bias.zero_()
        with _Scorer(model, "towers"):
            f = _factors(model, test_data, uids, sst_list)
            assert bool((f["W"] == 0).all())
            scores = full_sort_scores(uids, model, test_data, sst_list=sst_list).cpu().numpy()
            val, idx = full_sort_topk(uids, model, test_data, 10, sst_list=sst_list)
        masked = np.isneginf(scores)
        assert masked[:, 0].all() and np.all(scores[~masked] == 0.5)
        assert bool((val == 0.5).all())
        for u in range(len(uids)):
            np.testing.assert_array_equal(idx[u].cpu().numpy(), np.nonzero(~masked[u])[0][:10])
    finally:
        with torch.no_grad():
            last.weight.copy_(keep[0])
            last.bias.copy_(keep[1])

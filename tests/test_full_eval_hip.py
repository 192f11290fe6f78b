"""GPU: full-sort evaluation without the score matrix (`full_sort_eval: fused`).  Every comparison is exact.

1. Kernels.  fr_recommend_cells on every cell of the matrix equals fr_recommend_topk's scores_out bit for bit, and
   fr_recommend_meanrank equals both tests/full_eval_ref.py's restatement on scores_out and fr_eval_meanrank_segments on it --
   over users x items x D at the tile edges, every epilogue, with and without biases and histories, the items cut into 1
   and 3 slices; on integer factors under the clamp (runs of equal cells), a saturated sigmoid, a user without positives,
   one with 300 (three passes of 128 thresholds), a key listed twice, a key beyond the matrix, positives on masked cells.
2. Collector.  eval_batch_collect_fused gathers what eval_batch_collect gathers from the fused kernel's own matrix, key by
   key, with and without gauc, for a FOCF and a filtered PFCN_BiasedMF model and on integer factors where every user's list
   hangs on a tie (the host-order fallback).
3. Trainer.  evaluate under `fused` returns the dict of the same trainer under `matrix` fed the fused kernel's matrix.
4. Memory.  One fused batch of 2 048 users x 100 001 items stays below 1/8 of the matrix it does not build."""

import numpy as np
import pytest
import torch

import full_eval_ref as E
from fairrec import _C
from fairrec.functional import recommend_cells, recommend_meanrank, recommend_topk

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _segments(dense, keys):
    """fr_eval_meanrank_segments on the dense rows, as Collector.eval_batch_collect calls it."""
    U, N = dense.shape
    seg = torch.arange(U + 1, device=DEV, dtype=torch.int64) * N
    out = torch.empty((U, 3), dtype=torch.int64, device=DEV)
    _C.check(_C.lib().fr_eval_meanrank_segments(seg.data_ptr(), U, None, dense.data_ptr(), _C.ptr(keys), keys.numel(), N, U * N,
                                                out.data_ptr(), None, 0, _C.current_stream()), "fr_eval_meanrank_segments")
    return out


def _check_kernels(monkeypatch, X, W, keys, **kw):
    """Checks 1 for one set of arguments (torch tensors); returns (dense, triple)."""
    U, N = X.shape[0], W.shape[0]
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    dense = recommend_topk(X, W, 1, want_scores=True, slices=1, **kw)[2]
    assert _same_bits(dense, recommend_topk(X, W, 1, want_scores=True, slices=3, **kw)[2])
    cu = torch.arange(U, device=DEV).repeat_interleave(N)
    ci = torch.arange(N, device=DEV).repeat(U)
    cells = recommend_cells(X, W, cu, ci, err, **kw)
    assert _same_bits(cells.view(U, N), dense), "fr_recommend_cells differs from scores_out"
    want = E.meanrank(dense.cpu().numpy(), keys.cpu().numpy())
    assert np.array_equal(_segments(dense, keys).cpu().numpy(), want), "the restatement and fr_eval_meanrank_segments disagree"
    for slices in ("1", "3"):
        monkeypatch.setenv("FAIRREC_REC_SLICES", slices)
        got = recommend_meanrank(X, W, keys, err, **kw)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), f"fr_recommend_meanrank, {slices} slices"
    monkeypatch.delenv("FAIRREC_REC_SLICES")
    assert int(err.item()) == 0
    return dense, want


# ---- 1. kernels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 129, 257, 1000])
@pytest.mark.parametrize("U", [1, 31, 33, 70])
def test_kernels_equal_the_matrix(U, N, monkeypatch):
    rng = np.random.default_rng(1000 * U + N)
    for D in (1, 7, 64, 65, 256):
        X = _t((0.5 * rng.standard_normal((U, D))).astype(np.float32))
        W = _t((0.5 * rng.standard_normal((N, D))).astype(np.float32))
        ub, ib = (0.3 * rng.standard_normal(U)).astype(np.float32), (0.3 * rng.standard_normal(N)).astype(np.float32)
        indptr, items = E.histories(rng, U, N)
        for epilogue in (0, 1, 2):
            for biased in (False, True):
                for hist in (False, True):
                    kw = dict(epilogue=epilogue, scale=0.7, mask_pad=bool(hist or D % 2 == 0))
                    if biased:
                        kw.update(user_bias=_t(ub), item_bias=_t(ib), bias0=0.05)
                    if hist:
                        kw.update(hist_indptr=_t(indptr), hist_items=_t(items))
                    # a user without positives and one with 300 (all items of a smaller catalogue); with one user, either
                    long_user = (0 if N == 1000 else None) if U == 1 else 1
                    keys = E.positives(rng, U, N, indptr if hist else None, items, long_user=long_user,
                                       empty_user=None if long_user == 0 else 0)
                    _, triple = _check_kernels(monkeypatch, X, W, _t(keys), **kw)
                    if long_user is not None:
                        assert min(300, N) <= triple[long_user, 2] <= min(300, N) + 2      # (+ the pad item, + a history cell)
                    if long_user != 0:
                        assert triple[0, 0] == 0 and triple[0, 2] == 0


def test_integer_factors_under_the_clamp(monkeypatch):
    """Entries in -2..2, D = 7, clamp at 5: whole runs of cells are equal (0, k / 5, 1), so the equal counts carry the result."""
    rng = np.random.default_rng(5)
    U, N, D = 33, 257, 7
    X, W = _t(rng.integers(-2, 3, (U, D)).astype(np.float32)), _t(rng.integers(-2, 3, (N, D)).astype(np.float32))
    indptr, items = E.histories(rng, U, N)
    keys = _t(E.positives(rng, U, N, indptr, items, long_user=2, empty_user=0))
    kw = dict(epilogue=1, scale=5.0, mask_pad=True, hist_indptr=_t(indptr), hist_items=_t(items))
    dense, triple = _check_kernels(monkeypatch, X, W, keys, **kw)
    assert len(np.unique(dense.cpu().numpy())) <= 7 and triple[2, 2] == 257
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    again = recommend_meanrank(X, W, keys, err, **kw)
    assert np.array_equal(again.cpu().numpy(), triple) and torch.equal(again, recommend_meanrank(X, W, keys, err, **kw))


def test_saturated_sigmoid(monkeypatch):
    """Entries in -4..4, D = 64: most dots are beyond +-17, where the sigmoid is exactly 1 (or a value next to 0)."""
    rng = np.random.default_rng(6)
    U, N, D = 33, 257, 64
    X, W = _t(rng.integers(-4, 5, (U, D)).astype(np.float32)), _t(rng.integers(-4, 5, (N, D)).astype(np.float32))
    keys = _t(E.positives(rng, U, N, long_user=1, empty_user=0))
    dense, _ = _check_kernels(monkeypatch, X, W, keys, epilogue=2, mask_pad=True)
    assert (dense == 1.0).float().mean() > 0.2
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    cu, ci = torch.arange(U, device=DEV), torch.arange(U, device=DEV) + 3
    a, b = (recommend_cells(X, W, cu, ci, err, epilogue=2, mask_pad=True) for _ in range(2))
    assert _same_bits(a, b) and _same_bits(a, dense[cu, ci])


def test_cells_flag_an_id_outside_its_table():
    rng = np.random.default_rng(7)
    X, W = _t(rng.standard_normal((5, 8)).astype(np.float32)), _t(rng.standard_normal((40, 8)).astype(np.float32))
    dense = recommend_topk(X, W, 1, want_scores=True)[2]
    for cu, ci in (([0, 5], [1, 1]), ([0, 1], [40, 1]), ([-1, 1], [2, 2]), ([2, 1], [2, -3])):
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        out = recommend_cells(X, W, torch.tensor(cu), torch.tensor(ci), err)
        assert int(err.item()) == _C.DEV_ERR_INDEX_RANGE
        ok = [j for j in range(2) if 0 <= cu[j] < 5 and 0 <= ci[j] < 40]
        assert len(ok) == 1 and _same_bits(out[ok], dense[cu[ok[0]], ci[ok[0]]].view(1)) and bool(torch.isnan(out[1 - ok[0]]))
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert recommend_cells(X, W, torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), err).numel() == 0
    none = recommend_meanrank(X, W, torch.zeros(0, dtype=torch.int64), err, mask_pad=True)       # no positives: user_len alone
    assert np.array_equal(none.cpu().numpy(), [[0, 39, 0]] * 5) and int(err.item()) == 0


# ---- 2. collector --------------------------------------------------------------------------------------------------------
class _Cfg(dict):
    __getitem__ = dict.get


def _collected(cfg, fused, factors, matrix, inter, ip, hi, pos_u, pos_i):
    from fairrec.evaluator import Collector
    c = Collector(cfg)
    if fused:
        c.eval_batch_collect_fused(factors, inter, ip, hi, pos_u, pos_i)
        c.check_device_errors()
    else:
        c.eval_batch_collect(matrix.clone(), inter, pos_u, pos_i)
    return c.get_data_struct()


def _assert_same_collection(factors, matrix, inter, ip, hi, pos_u, pos_i, topk):
    for metrics in (["NDCG", "GAUC"], ["NDCG"]):
        cfg = _Cfg(topk=topk, sst_attr_list=["gender"], eval_args={"mode": "full"}, metrics=metrics, device=DEV)
        a = _collected(cfg, True, factors, None, inter, ip, hi, pos_u, pos_i)
        b = _collected(cfg, False, None, matrix, inter, ip, hi, pos_u, pos_i)
        assert set(a) == set(b) == {"rec.topk", "rec.items", "rec.positive_score", "data.positive_i", "data.gender"} | (
            {"rec.meanrank"} if "GAUC" in metrics else set())
        for key in b:
            assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, key
            same = _same_bits(a[key], b[key]) if a[key].dtype == torch.float32 else torch.equal(a[key], b[key])
            assert same, key


def test_collector_on_integer_factors_ranks_ties_in_host_order():
    """33 users x 257 items, D = 7, entries in -2..2, clamp at 5: every user has a tie inside its best 11, so every list comes
    from the host-order fallback on the user's dense row."""
    from fairrec.data.interaction import Interaction
    rng = np.random.default_rng(8)
    U, N, D = 33, 257, 7
    X, W = _t(rng.integers(-2, 3, (U, D)).astype(np.float32)), _t(rng.integers(-2, 3, (N, D)).astype(np.float32))
    indptr, items = E.histories(rng, U, N)
    ip, hi = _t(indptr), _t(items)
    keys = np.unique(E.positives(rng, U, N, long_user=4, empty_user=None))
    keys = keys[(keys < U * N) & (keys % N != 0)]
    pos_u, pos_i = _t(keys // N), _t(keys % N)
    inter = Interaction({"gender": torch.from_numpy(rng.integers(0, 2, U)).to(DEV)})
    for factors in (dict(X=X, W=W, epilogue=1, scale=5.0),
                    dict(X=X / 4, W=W, epilogue=2, user_bias=_t(rng.integers(-1, 2, U).astype(np.float32)),
                         item_bias=_t(rng.integers(-1, 2, N).astype(np.float32)), bias0=0.5)):
        kw = {k: v for k, v in factors.items() if k not in ("X", "W")}
        vals, _, matrix = recommend_topk(factors["X"], W, 11, mask_pad=True, hist_indptr=ip, hist_items=hi, want_scores=True, **kw)
        tied = (vals[:, 1:] == vals[:, :-1]).any(dim=1)
        assert int(tied.sum()) > 0
        if factors["epilogue"] == 1:
            assert bool(tied.all())
        _assert_same_collection(factors, matrix, inter, ip, hi, pos_u, pos_i, [5, 10])


COMMON = {"epochs": 1, "train_batch_size": 512, "synthetic_users": 150, "synthetic_items": 300, "synthetic_interactions": 4000,
          "device": DEV, "embedding_size": 16, "eval_args": {"mode": "full"}, "topk": [5, 10], "valid_metric": "ndcg@10",
          "valid_metric_bigger": True, "sst_attr_list": ["gender"], "eval_batch_size": 4096, "metric_decimal_place": 4,
          "popularity_ratio": 0.1, "tail_ratio": 0.1,
          "metrics": ["Hit", "MRR", "NDCG", "Recall", "Precision", "MAP", "GiniIndex", "PopularityPercentage", "ItemCoverage",
                      "AveragePopularity", "ShannonEntropy", "TailPercentage", "NonParityUnfairness", "ValueUnfairness",
                      "AbsoluteUnfairness", "UnderUnfairness", "OverUnfairness", "DifferentialFairness", "GAUC"]}
CASES = {
    "FOCF": ("FOCF", dict(fair_objective="value"), None),
    "PFCN_BiasedMF-sm": ("PFCN_BiasedMF", dict(filter_mode="sm", dis_hidden_size_list=[16, 8], train_epoch_interval=1,
                                               learning_rate=0.01), ["gender"]),
    "FairGo_PMF": ("FairGo_PMF", dict(pretrain_epochs=1, train_epoch_interval=1, n_layers=2, dis_hidden_size_list=[16, 8, 4],
                                      filter_hidden_size_list=[32, 16], neg_sampling=None), None),
}
_trained = {}


def _train(case, tmp_path_factory):
    """(model, trainer, test loader, attribute subset) of a case, trained once for the tests below."""
    if case not in _trained:
        from fairrec.data.dataloader import FullSortEvalDataLoader
        from fairrec.quick_start import run_recbole
        model_name, extra, sst_list = CASES[case]
        seen, loaders = {}, []
        init = FullSortEvalDataLoader.__init__

        def recording_init(self, *a, **kw):
            init(self, *a, **kw)
            loaders.append(self)

        FullSortEvalDataLoader.__init__ = recording_init
        try:
            run_recbole(model=model_name, config_dict=dict(COMMON, checkpoint_dir=str(tmp_path_factory.mktemp(case)), **extra),
                        before_fit=lambda m, trainer: seen.update(model=m, trainer=trainer))
        finally:
            FullSortEvalDataLoader.__init__ = init
        _trained[case] = (seen["model"], seen["trainer"], loaders[-1], sst_list)       # the test loader is built last
    return _trained[case]


@pytest.mark.parametrize("case", ["FOCF", "PFCN_BiasedMF-sm"])
def test_collector_on_a_model(case, tmp_path_factory):
    from fairrec.data.interaction import Interaction
    from fairrec.utils.case_study import full_sort_scores, history_csr, users_per_batch
    model, trainer, test_data, sst_list = _train(case, tmp_path_factory)
    ds, n_items = test_data.dataset, test_data.dataset.item_num
    uids = test_data.uid_list
    inter = ds.join(Interaction({ds.uid_field: uids})).to(DEV)
    model.eval()
    with torch.no_grad():
        factors = model.full_sort_factors(inter, sst_list, users_per_batch=users_per_batch(test_data.config, n_items))
        matrix = full_sort_scores(uids, model, test_data, sst_list=sst_list)
    assert factors is not None
    ip, hi = history_csr(test_data.hist_indptr, test_data.hist_items, uids, n_items)
    pos_u, pos_i = test_data._rows(test_data.pos_indptr, test_data.pos_items, uids)
    _assert_same_collection(factors, matrix, inter, ip, hi, pos_u, pos_i, [5, 10])


# ---- 3. trainer ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_trainer_evaluates_the_same_under_fused(case, tmp_path_factory, monkeypatch):
    from fairrec.utils.case_study import users_per_batch
    model, trainer, test_data, _ = _train(case, tmp_path_factory)
    assert trainer.full_sort_eval == "matrix"
    n_fused, n_matrix = [0], [0]

    def unmasked(interaction, n_items, sst_list=None):
        """The fused kernel's own matrix of the batch, before the masks the Trainer writes."""
        n_matrix[0] += 1
        f = model.full_sort_factors(interaction, sst_list, users_per_batch=users_per_batch(trainer.config, n_items))
        kw = {k: v for k, v in f.items() if k not in ("X", "W")}
        return recommend_topk(f["X"], f["W"], 1, want_scores=True, **kw)[2]

    from fairrec.evaluator import Collector
    collect = Collector.eval_batch_collect_fused

    def counting(self, *a, **kw):
        n_fused[0] += 1
        return collect(self, *a, **kw)

    monkeypatch.setattr(Collector, "eval_batch_collect_fused", counting)
    monkeypatch.setattr(trainer, "full_sort_eval", "fused")
    fused = trainer.evaluate(test_data, load_best_model=False)
    assert n_fused[0] > 0 and n_matrix[0] == 0
    monkeypatch.setattr(trainer, "full_sort_eval", "matrix")
    monkeypatch.setattr(trainer, "_full_sort_scores", unmasked)
    n_fused[0] = 0
    matrix = trainer.evaluate(test_data, load_best_model=False)
    assert n_fused[0] == 0 and n_matrix[0] > 0

    def flat(d):
        return {k: (flat(v) if isinstance(v, dict) else repr(v)) for k, v in d.items()}
    assert flat(fused) == flat(matrix)
    results = [r for r in fused.values() if isinstance(r, dict)] or [fused]
    assert all("gauc" in r and "ndcg@10" in r and "giniindex@10" in r for r in results)
    assert any(k.startswith("Differential") for k in results[0])


# ---- 4. memory -----------------------------------------------------------------------------------------------------------
def test_a_fused_batch_does_not_hold_the_matrix():
    from fairrec.data.interaction import Interaction
    from fairrec.evaluator import Collector
    U, N, D, K = 2048, 100001, 16, 10
    g = torch.Generator(device="cpu").manual_seed(9)
    X = (0.1 * torch.randn(U, D, generator=g)).to(DEV)
    W = (0.1 * torch.randn(N, D, generator=g)).to(DEV)
    pos_u = torch.arange(U).repeat_interleave(10).to(DEV)
    pos_i = torch.randint(1, N, (U * 10,), generator=g).to(DEV)
    order = torch.argsort(pos_u * N + pos_i)
    pos_u, pos_i = pos_u[order], pos_i[order]
    hist_items = torch.sort(torch.randint(1, N, (U, 20), generator=g), dim=1).values.reshape(-1).to(DEV)
    hist_indptr = (torch.arange(U + 1) * 20).to(DEV)
    inter = Interaction({"gender": torch.randint(0, 2, (U,), generator=g).to(DEV)})
    c = Collector(_Cfg(topk=[K], sst_attr_list=["gender"], eval_args={"mode": "full"}, metrics=["NDCG", "GAUC"], device=DEV))
    factors = dict(X=X, W=W, epilogue=1, scale=5.0)
    limit = U * N * 4 // 8
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    c.eval_batch_collect_fused(factors, inter, hist_indptr, hist_items, pos_u, pos_i)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak memory rose by {rise / 2 ** 20:.1f} MiB; the matrix would take {U * N * 4 / 2 ** 20:.0f} MiB")
    assert rise < limit
    c.check_device_errors()
    out = c.get_data_struct()
    assert out["rec.meanrank"].shape == (U, 3) and out["rec.topk"].shape == (U, K + 1) and out["rec.items"].shape == (U, K)
    # a sample of the users against their dense rows
    sel = torch.arange(0, U, 409, device=DEV)
    ip = torch.arange(sel.numel() + 1, device=DEV) * 20
    hi = hist_items.view(U, 20)[sel].reshape(-1)
    vals, idx, dense = recommend_topk(X[sel], W, K + 1, epilogue=1, scale=5.0, mask_pad=True, hist_indptr=ip, hist_items=hi,
                                      want_scores=True)
    assert not bool((vals[:, 1:] == vals[:, :-1]).any())          # (no list of the sample hangs on a tie)
    assert torch.equal(out["rec.items"][sel], idx[:, :K])
    keys = torch.cat([j * N + pos_i[pos_u == u] for j, u in enumerate(sel.tolist())])
    assert np.array_equal(out["rec.meanrank"][sel].cpu().numpy(), E.meanrank(dense.cpu().numpy(), keys.cpu().numpy()))
    assert (dense == 0).float().mean() > 0.4                      # half of the cells tie at 0: the equal counts are exercised
    sample = pos_u % 409 == 0
    assert _same_bits(out["rec.positive_score"][sample], dense[pos_u[sample] // 409, pos_i[sample]])

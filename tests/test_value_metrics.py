"""CPU: the numpy restatement of the value-type metrics and of GAUC (tests/value_metrics_ref.py) against sklearn, the
Evaluator's config rules for the value / ranking families, LabeledEvalDataLoader's batch geometry, and the argument checks of
the new C entries (no device needed: they return before any launch)."""
import ctypes
import logging
import math

import numpy as np
import pytest
import torch

import value_metrics_ref as R


def _case(rng, n, levels, p_pos=0.3):
    score = rng.random(n).astype(np.float32)
    if levels:
        score = (np.floor(score * levels) / levels).astype(np.float32)
    label = (rng.random(n) < p_pos * 0.5 + 0.5 * score * p_pos * 2).astype(np.float32)
    return score, label


@pytest.mark.parametrize("n", [1000, 30000, 200000])
@pytest.mark.parametrize("levels", [0, 2, 64, 1024])
def test_restatement_against_sklearn(n, levels):
    sk = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(n + levels)
    score, label = _case(rng, n, levels)
    two_u, P, Nn = R.auc_exact(score, label)
    assert P + Nn == n and P == int((label == 1).sum())
    assert abs(two_u / (2 * P * Nn) - sk.roc_auc_score(label, score)) <= n * 2.0 ** -52
    s64 = score.astype(np.float64)
    assert abs(R.logloss(score, label) - sk.log_loss(label, np.clip(s64, 1e-15, 1 - 1e-15))) <= 1e-12
    rating = rng.integers(1, 6, n).astype(np.float32)          # MAE / RMSE on rating-valued labels too
    for y in (label, rating):
        assert abs(R.mae(score, y) - sk.mean_absolute_error(y, s64)) <= 1e-12
        assert abs(R.rmse(score, y) - math.sqrt(sk.mean_squared_error(y, s64))) <= 1e-12


def test_auc_exact_edges():
    assert R.auc_exact([0.5], [1.0]) == (0, 1, 0) and math.isnan(R.auc([0.5], [1.0]))
    assert R.auc_exact([0.5, 0.5], [1.0, 0.0]) == (1, 1, 1) and R.auc([0.5, 0.5], [1.0, 0.0]) == 0.5
    assert R.auc([0.1, 0.9], [0.0, 1.0]) == 1.0 and R.auc([0.9, 0.1], [0.0, 1.0]) == 0.0
    # a label other than 0 / 1 counts as a negative
    assert R.auc_exact([0.1, 0.2, 0.3], [2.0, 1.0, 0.5]) == (2, 1, 2)
    assert math.isnan(R.auc([0.1, 0.2], [0.0, 0.0]))


def test_meanrank_and_gauc_against_sklearn_per_user():
    sk = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(5)
    n_items, triples, aucs, weights = 150, [], [], []
    for u in range(300):
        n_cand = int(rng.integers(5, 121))
        items = rng.choice(np.arange(1, n_items), n_cand, replace=False)
        row = np.full(n_items, -np.inf, dtype=np.float32)
        row[items] = (np.floor(rng.random(n_cand) * 16) / 16).astype(np.float32)
        mask = np.zeros(n_items, dtype=bool)
        mask[items[:int(rng.integers(1, max(n_cand // 3, 2)))]] = True
        t = R.meanrank(row, mask)
        triples.append(t)
        two_rank, user_len, pos_len = t
        assert user_len == n_cand
        pair = (user_len + 1) * pos_len - pos_len * (pos_len + 1) / 2 - two_rank / 2
        auc_u = pair / ((user_len - pos_len) * pos_len)
        want = sk.roc_auc_score(mask[items], row[items])
        assert abs(auc_u - want) < 1e-12
        aucs.append(want * pos_len)
        weights.append(pos_len)
    triples += [[0, 7, 0], [12, 3, 3]]                      # a user without positives, one without negatives: dropped
    assert abs(R.gauc(triples) - sum(aucs) / sum(weights)) < 1e-12
    assert math.isnan(R.gauc([[0, 7, 0]]))


def test_dense_rows_count_a_repeated_item_once():
    seg = [0, 4, 5]
    items = np.array([3, 5, 5, 2, 7])
    scores = np.array([0.5, 0.25, 0.25, 0.5, 1.0], dtype=np.float32)
    dense, mask = R.dense_rows(seg, items, scores, [0, 4], 9)
    assert R.meanrank(dense[0], mask[0]) == [2 * 0 + 2 + 1, 3, 1]         # tied with item 2: rank 1.5
    assert R.meanrank(dense[1], mask[1]) == [2, 1, 1]


# ---- Evaluator config rules --------------------------------------------------------------------------------------------
def _evaluator(metrics, mode):
    from fairrec.config import Config
    from fairrec.evaluator import Evaluator
    d = {"device": "cpu", "metrics": metrics, "topk": [5]}
    if mode is not None:
        d["eval_args"] = {"mode": mode}
    return Evaluator(Config(config_dict=d))


def test_evaluator_config_rules():
    assert _evaluator(["NDCG", "GAUC"], "uni20").metrics == ["ndcg", "gauc"]
    assert _evaluator(["AUC", "RMSE"], "labeled").metrics == ["auc", "rmse"]
    assert _evaluator(["LogLoss", "MAE"], "labeled").metrics == ["logloss", "mae"]
    with pytest.raises(RuntimeError, match="Ranking metrics and value metrics can not be used at the same time."):
        _evaluator(["AUC", "NDCG"], "labeled")
    with pytest.raises(RuntimeError):
        _evaluator(["GAUC", "LogLoss"], "full")
    with pytest.raises(ValueError, match="labeled.*uni20"):
        _evaluator(["AUC"], "uni20")
    with pytest.raises(ValueError, match="labeled"):
        _evaluator(["RMSE"], None)                          # no eval_args: the mode is full
    with pytest.raises(ValueError, match="gauc.*labeled"):
        _evaluator(["GAUC"], "labeled")
    with pytest.raises(ValueError, match="ndcg.*labeled"):
        _evaluator(["NDCG"], "labeled")
    with pytest.raises(NotImplementedError, match="bogus"):
        _evaluator(["Bogus"], "labeled")
    with pytest.raises(NotImplementedError):
        _evaluator(["AUC", "Bogus"], "full")


def test_gauc_from_triples_matches_the_restatement(caplog):
    from fairrec.evaluator.metrics import gauc
    rng = np.random.default_rng(2)
    triples = []
    for _ in range(200):
        user_len = int(rng.integers(2, 60))
        pos_len = int(rng.integers(0, user_len + 1))
        row = (np.floor(rng.random(user_len) * 8) / 8).astype(np.float32)
        mask = np.zeros(user_len, dtype=bool)
        mask[:pos_len] = True
        triples.append(R.meanrank(row, mask))
    with caplog.at_level(logging.WARNING):
        got = gauc(torch.tensor(triples, dtype=torch.int64))
    assert abs(got - R.gauc(triples)) <= 1e-12 * abs(R.gauc(triples))
    assert "No positive samples" in caplog.text and "No negative samples" in caplog.text
    assert math.isnan(gauc(torch.tensor([[0, 4, 0]], dtype=torch.int64)))


# ---- LabeledEvalDataLoader ---------------------------------------------------------------------------------------------
def _dataset(n, with_label=True):
    from fairrec.config import Config
    from fairrec.data.dataset import InteractionDataset
    from fairrec.data.interaction import Interaction
    cfg = Config(config_dict={"device": "cpu", "eval_batch_size": 64, "eval_args": {"mode": "labeled"}})
    rng = np.random.default_rng(0)
    cols = {"user_id": torch.from_numpy(rng.integers(1, 20, n)), "item_id": torch.from_numpy(rng.integers(1, 30, n)),
            "rating": torch.from_numpy(rng.integers(1, 6, n).astype(np.float32))}
    if with_label:
        cols["label"] = torch.from_numpy((rng.random(n) < 0.4).astype(np.float32))
    users = Interaction({"user_id": torch.arange(20), "gender": torch.from_numpy(rng.integers(0, 2, 20).astype(np.float32))})
    return cfg, InteractionDataset(cfg, Interaction(cols), users, 20, 30)


def test_labeled_loader_batches_and_missing_label():
    from fairrec.data.dataloader import LabeledEvalDataLoader
    cfg, ds = _dataset(150)
    np_state, torch_state = np.random.get_state()[1].copy(), torch.get_rng_state().clone()
    dl = LabeledEvalDataLoader(cfg, ds)
    assert len(dl) == 3
    for _ in range(2):                                       # a second pass yields the same batches
        batches = list(dl)
        assert [len(b) for b in batches] == [64, 64, 22]
        for col in ("user_id", "item_id", "rating", "label"):
            assert torch.equal(torch.cat([b[col] for b in batches]), ds.inter_feat[col])
        for b in batches:
            assert torch.equal(b["gender"], ds.user_feat["gender"][b["user_id"]])
    assert "gender" not in ds.inter_feat                      # the join is the batch's, not the dataset's
    assert (np.random.get_state()[1] == np_state).all() and torch.equal(torch.get_rng_state(), torch_state)
    cfg2, ds2 = _dataset(10, with_label=False)
    with pytest.raises(ValueError, match=r"\[label\]"):
        LabeledEvalDataLoader(cfg2, ds2)


def test_set_label_by_threshold_keeps_the_source_column():
    from fairrec.quick_start import set_label_by_threshold
    cfg, ds = _dataset(50, with_label=False)
    set_label_by_threshold(cfg, ds)                          # no threshold configured: nothing happens
    assert "label" not in ds.inter_feat
    cfg["threshold"] = {"rating": 3}
    set_label_by_threshold(cfg, ds)
    assert torch.equal(ds.inter_feat["label"], (ds.inter_feat["rating"] >= 3).float()) and "rating" in ds.inter_feat
    kept = ds.inter_feat["label"].clone()
    cfg["threshold"] = {"rating": 5}
    set_label_by_threshold(cfg, ds)                          # a label column that is there is left alone
    assert torch.equal(ds.inter_feat["label"], kept)
    cfg3, ds3 = _dataset(5, with_label=False)
    cfg3["threshold"] = {"stars": 3}
    with pytest.raises(ValueError, match="stars"):
        set_label_by_threshold(cfg3, ds3)


def test_eval_neg_sample_args_still_refuses_labeled():
    from fairrec.data.dataloader import eval_neg_sample_args
    with pytest.raises(NotImplementedError):
        eval_neg_sample_args("labeled")


# ---- argument checks of the new entries: FR_EINVAL before any launch, the outputs untouched ------------------------------
def test_argument_validation_without_gpu():
    from fairrec import _C
    lib = _C.lib()
    f32 = (ctypes.c_float * 4)(0.1, 0.2, 0.3, 0.4)
    f64 = (ctypes.c_double * 3)(-7.0, -7.0, -7.0)
    i64 = (ctypes.c_int64 * 3)(-7, -7, -7)
    ws = (ctypes.c_uint8 * 4096)()
    a = ctypes.addressof
    assert lib.fr_value_metrics_workspace_bytes(0) == 0 and lib.fr_value_metrics_workspace_bytes(2 ** 31) == 0
    assert lib.fr_value_metrics_workspace_bytes(-3) == 0 and lib.fr_auc_sorted_workspace_bytes(2 ** 31) == 0
    assert lib.fr_value_metrics_workspace_bytes(4) > 0 and lib.fr_auc_sorted_workspace_bytes(4) >= 5 * 4 + 8
    assert lib.fr_value_metrics_workspace_bytes(2 ** 31 - 1) == lib.fr_value_metrics_workspace_bytes(10 ** 8)
    assert lib.fr_eval_meanrank_workspace_bytes(100) >= 100 and lib.fr_eval_meanrank_workspace_bytes(0) == 0
    bad_value = [(None, a(f32), 4, a(f64), a(i64), a(ws), 4096), (a(f32), None, 4, a(f64), a(i64), a(ws), 4096),
                 (a(f32), a(f32), 4, None, a(i64), a(ws), 4096), (a(f32), a(f32), 4, a(f64), None, a(ws), 4096),
                 (a(f32), a(f32), 4, a(f64), a(i64), None, 4096), (a(f32), a(f32), 0, a(f64), a(i64), a(ws), 4096),
                 (a(f32), a(f32), -1, a(f64), a(i64), a(ws), 4096), (a(f32), a(f32), 2 ** 31, a(f64), a(i64), a(ws), 4096),
                 (a(f32), a(f32), 4, a(f64), a(i64), a(ws), lib.fr_value_metrics_workspace_bytes(4) - 1)]
    for args in bad_value:
        assert lib.fr_value_metrics(*args, None) == -1 and lib.fr_last_error()
    bad_auc = [(None, a(f32), 4, a(i64), a(ws), 4096), (a(f32), None, 4, a(i64), a(ws), 4096),
               (a(f32), a(f32), 4, None, a(ws), 4096), (a(f32), a(f32), 4, a(i64), None, 4096),
               (a(f32), a(f32), 0, a(i64), a(ws), 4096), (a(f32), a(f32), 2 ** 31, a(i64), a(ws), 4096),
               (a(f32), a(f32), 4, a(i64), a(ws), lib.fr_auc_sorted_workspace_bytes(4) - 1)]
    for args in bad_auc:
        assert lib.fr_auc_sorted(*args, None) == -1 and lib.fr_last_error()
    assert b"2^31" in lib.fr_last_error() or b"workspace" in lib.fr_last_error()
    seg = (ctypes.c_int64 * 2)(0, 4)
    it = (ctypes.c_int64 * 4)(1, 2, 3, 4)
    keys = (ctypes.c_int64 * 2)(1, 3)
    bad_rank = [(None, 1, a(it), a(f32), a(keys), 2, 9, 4, a(i64), a(ws), 4096),
                (a(seg), 1, a(it), None, a(keys), 2, 9, 4, a(i64), a(ws), 4096),
                (a(seg), 1, a(it), a(f32), None, 2, 9, 4, a(i64), a(ws), 4096),
                (a(seg), 1, a(it), a(f32), a(keys), 2, 9, 4, None, a(ws), 4096),
                (a(seg), 0, a(it), a(f32), a(keys), 2, 9, 4, a(i64), a(ws), 4096),
                (a(seg), 1, a(it), a(f32), a(keys), -1, 9, 4, a(i64), a(ws), 4096),
                (a(seg), 1, a(it), a(f32), a(keys), 2, 0, 4, a(i64), a(ws), 4096),
                (a(seg), 1, a(it), a(f32), a(keys), 2, 9, 0, a(i64), a(ws), 4096),
                (a(seg), 1, a(it), a(f32), a(keys), 2, 9, 4, a(i64), None, 0),          # items given: the workspace is needed
                (a(seg), 1, a(it), a(f32), a(keys), 2, 9, 4, a(i64), a(ws), 3)]
    for args in bad_rank:
        assert lib.fr_eval_meanrank_segments(*args, None) == -1 and lib.fr_last_error()
    assert list(f64) == [-7.0] * 3 and list(i64) == [-7] * 3

"""GPU: ranking and value metrics per sensitive group -- fr_topk_metrics_grouped and fr_gauc_grouped (csrc/metrics.hip) through
the C ABI against the references of tests/group_metrics_ref.py (pinned to oracle/metrics.py and to evaluator.gauc's formula on
the CPU by tests/test_group_metrics_ref.py, where the refusals of bad arguments are tested too: they need no GPU), then the
`utility_by_group` key through Collector, Evaluator and Trainer.evaluate on a 40-user x 71-item FOCF model with two attributes
and their intersection.  Shapes are the smallest that reach each edge: groups of 1, 63, 64, 65 and 129 members (the 64-position
chunk), 1 .. 70 groups, groups contiguous in row order (perm NULL) and interleaved (perm a real sort).  Every output and every
workspace sits between canary frames (NaN / sentinel / 0xFF start values), every return code is asserted, as in
tests/test_metrics_kernels_hip.py.

Tolerances are derived in tests/group_metrics_ref.py: metrics_ref.topk_tolerance(ref_g, n_g, K) per group, gamma_(9 + ceil(n_g /
64)) |ref| for GAUC's sums; counts, NaN positions and zero-bound entries exact; one group with the identity permutation equals
fr_topk_metrics byte for byte.  Every test prints its largest error / bound, none may exceed 1.

Worst error / bound measured on an MI355X, per test group:
  fr_topk_metrics_grouped at the chunk edges 0.15 (K = 1, perm NULL; 0.02 .. 0.08 in the other five cases)
  group counts 1 / 2 / 3 / 9 / 70 / 5: 0.054 (G = 70; 0.03 .. 0.05 elsewhere); the size-weighted mean against fr_topk_metrics
  0.031; with a zero-positive row 0.040; with empty groups 0.056
  fr_gauc_grouped 0.13 (perm NULL; 0 with the sorted perm); evaluator.group_gauc 0.16
  through the Evaluator 0.998 in full mode, 0.97 / 0.96 in uni5 at K = 10 / 63: the rounding to 12 decimal places, which the
  bound allows for with its full half step, is what these three measure (the kernels' share is the figures above)
"""
import functools
import math

import numpy as np
import pytest
import torch

import group_metrics_ref as GR
import metrics_ref as R
import value_metrics_ref as V
from test_metrics_kernels_hip import _bytes, _dev, _Frames, _lib, _ptr, _st, _topk, _within

pytestmark = pytest.mark.gpu
DEV = "cuda"
U64 = 2.0 ** -53


# ---- fr_topk_metrics_grouped ---------------------------------------------------------------------------------------------------------

def _grouped(rec, perm, start):
    U, K, G = rec.shape[0], rec.shape[1] - 1, len(start) - 1
    lib, f = _lib(), _Frames()
    out = f.new(torch.float64, G, 6, K)
    need = lib.fr_topk_metrics_grouped_workspace_bytes(U, K, G)
    assert need == (((U + 63) // 64 + G) * 6 * K + G + 1) * 8
    ws = f.ws(need)
    t = [_dev(x) for x in (rec, perm, start)]
    rc = lib.fr_topk_metrics_grouped(t[0].data_ptr(), _ptr(t[1]), t[2].data_ptr(), U, K, G, out.data_ptr(), ws.data_ptr(), need,
                                     _st())
    assert rc == 0, lib.fr_last_error()
    assert f.intact()
    return out.cpu().numpy()


def _check_groups(tag, got, ref, sizes, K):
    """NaN exactly where the reference has it, everything else within the group's bound"""
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{tag}: NaN positions differ"
    fin = ~np.isnan(ref)
    bound = GR.group_topk_tolerance(np.where(fin, ref, 0.0), sizes, K)
    return _within(tag, got[fin], ref[fin], bound[fin])


@functools.lru_cache(maxsize=None)
def _chunk_ref(K, shuffled):
    rec, perm, start = GR.chunk_case(K, shuffled)
    return rec, perm, start, GR.group_topk_ref(rec, perm, start)


@pytest.mark.parametrize("K", GR.CHUNK_K)
def test_groups_at_the_chunk_edges(K):
    for shuffled in (False, True):
        rec, perm, start, (ref, sizes) = _chunk_ref(K, shuffled)
        assert sizes.tolist() == GR.CHUNK_SIZES and (perm is None) == (not shuffled)
        assert all((ref[g][:, K - 1] > 0).all() for g in range(1, 5))
        _check_groups(f"topk_grouped sizes 1/63/64/65/129 K={K} perm={'sort' if shuffled else 'NULL'}", _grouped(rec, perm, start),
                      ref, sizes, K)


@functools.lru_cache(maxsize=None)
def _count_ref(G, U):
    rec = R.topk_case(U, GR.GROUP_K)
    perm, start = GR.segments(GR.assignment(U, G), G)
    return rec, perm, start, GR.group_topk_ref(rec, perm, start), R.topk_metrics_ref(rec)


@pytest.mark.parametrize("G,U", GR.GROUP_COUNTS)
def test_group_counts_and_the_overall_mean(G, U):
    K = GR.GROUP_K
    rec, perm, start, (ref, sizes), whole = _count_ref(G, U)
    assert all((ref[g][:, K - 1] > 0).all() for g in range(G) if sizes[g] >= R.ROW_KINDS)
    got = _grouped(rec, perm, start)
    _check_groups(f"topk_grouped G={G} U={U}", got, ref, sizes, K)
    if G == 70:
        assert (sizes == 1).all() and (got[ref == 0] == 0).all() and (ref == 0).any()
    # sum_g n_g out[g] / n against fr_topk_metrics, within the sum of both tolerances
    mean = (got * sizes[:, None, None]).sum(0) / U
    both = (GR.group_topk_tolerance(ref, sizes, K) * sizes[:, None, None]).sum(0) / U + R.topk_tolerance(whole, U, K)
    # (the host's own G multiplications, G - 1 additions and one division: gamma_(G + 2) of the mean)
    _within(f"size-weighted mean of {G} groups against fr_topk_metrics", mean, _topk(rec).numpy(), both + R.gamma(G + 2) * whole)


@pytest.mark.parametrize("U,K", GR.IDENTITY_SHAPES)
def test_one_group_is_fr_topk_metrics_byte_for_byte(U, K):
    rec = R.topk_case(U, K)
    plain = _bytes(_topk(rec))
    start = np.array([0, U], dtype=np.int64)
    assert _bytes(torch.from_numpy(_grouped(rec, None, start))) == plain
    assert _bytes(torch.from_numpy(_grouped(rec, np.arange(U, dtype=np.int64), start))) == plain


def test_zero_positive_row_makes_its_group_nan_in_recall_only():
    K = 20
    rec = R.topk_case(90, K, zero_positive_row=40)
    gidx = np.arange(90) // 30
    for perm, start in ((None, np.array([0, 30, 60, 90], dtype=np.int64)), GR.segments(gidx, 3)):
        ref, sizes = GR.group_topk_ref(rec, perm, start)
        assert np.isnan(ref[1, 3]).all() and np.isfinite(ref[[0, 2]]).all() and np.isfinite(ref[1][[0, 1, 2, 4, 5]]).all()
        _check_groups("topk_grouped with a zero-positive row in group 1", _grouped(rec, perm, start), ref, sizes, K)


def test_empty_groups_are_nan():
    rec = R.topk_case(65, 3)
    start = np.array([0, 0, 64, 64, 65, 65], dtype=np.int64)
    ref, sizes = GR.group_topk_ref(rec, None, start)
    got = _grouped(rec, None, start)
    assert np.isnan(got[[0, 2, 4]]).all()
    _check_groups("topk_grouped with empty groups", got, ref, sizes, 3)


def test_malformed_tables_stay_inside_the_inputs():
    """group_start beyond n_users / descending and perm entries outside [0, n_users): unspecified values, frames intact"""
    rec = R.topk_case(70, 4)
    perm = np.arange(70, dtype=np.int64)
    perm[[3, 40]] = (-5, 10 ** 12)
    for start in ([0, 500, 20, 70], [-9, 10, 10 ** 15, 70], [60, 0, 0, 0]):
        _grouped(rec, perm, np.array(start, dtype=np.int64))


def test_python_wrappers():
    from fairrec.evaluator import group_gauc, group_topk_metrics
    G, U = 9, 200
    rec, perm, start, (ref, sizes), _ = _count_ref(G, U)
    gidx = torch.from_numpy(GR.assignment(U, G)).cuda()
    got = group_topk_metrics(_dev(rec), gidx, G, [1, 20])
    assert sorted(got) == sorted(f"{n}@{k}" for n in ("hit", "mrr", "ndcg", "recall", "precision", "map") for k in (1, 20))
    raw = _grouped(rec, perm, start)
    for m, n in enumerate(("hit", "mrr", "ndcg", "recall", "precision", "map")):
        assert got[f"{n}@20"] == raw[:, m, 19].tolist()                # the same launch, the same bits
    t = GR.meanrank_case(U)
    sums, _ = GR.group_gauc_ref(t, perm, start)
    want = sums[:, 0] / sums[:, 1]
    _within("evaluator.group_gauc", group_gauc(_dev(t), gidx, G), want,
            (GR.gauc_tolerance(sums, sizes)[:, 0] / sums[:, 0] + 2 * U64) * want)


# ---- fr_gauc_grouped -----------------------------------------------------------------------------------------------------------------

def _gauc(t, perm, start):
    U, G = t.shape[0], len(start) - 1
    lib, f = _lib(), _Frames()
    out, kept = f.new(torch.float64, G, 2), f.new(torch.int64, G, 3)
    need = lib.fr_gauc_grouped_workspace_bytes(U, G)
    assert need == (((U + 63) // 64 + G) * 5 + G + 1) * 8
    ws = f.ws(need)
    d = [_dev(x) for x in (t, perm, start)]
    rc = lib.fr_gauc_grouped(d[0].data_ptr(), _ptr(d[1]), d[2].data_ptr(), U, G, out.data_ptr(), kept.data_ptr(), ws.data_ptr(),
                             need, _st())
    assert rc == 0, lib.fr_last_error()
    assert f.intact()
    return out.cpu().numpy(), kept.cpu().numpy()


def test_gauc_grouped_sizes_and_dropped_users():
    """groups of 1, 64 and 65 users and one of 3 whose users are all dropped; a no-positive and a no-negative user in different
    groups; contiguous (perm NULL) and interleaved"""
    sizes = [1, 64, 65, 3]
    U = sum(sizes)
    t = GR.meanrank_case(U)
    g_of = np.repeat(np.arange(4), sizes)
    t[10] = (0, 33, 0)                       # group 1: no positive
    t[70] = (42, 6, 6)                       # group 2: no negative
    t[130:133] = ((0, 20, 0), (30, 5, 5), (0, 9, 0))
    shuffle = np.random.default_rng(41).permutation(U)
    for perm, start, rows in ((None, np.concatenate(([0], np.cumsum(sizes))).astype(np.int64), t),
                              (*GR.segments(g_of[shuffle], 4), t[shuffle])):
        ref, kept_ref = GR.group_gauc_ref(rows, perm, start)
        assert kept_ref.tolist() == [[1, 0, 0], [63, 1, 0], [64, 0, 1], [0, 2, 1]]
        got, kept = _gauc(rows, perm, start)
        assert np.array_equal(kept, kept_ref)
        _within(f"gauc_grouped sizes 1/64/65/3 perm={'NULL' if perm is None else 'sort'}", got, ref, GR.gauc_tolerance(ref, sizes))
        assert (got[3] == 0).all()           # every user dropped: the host quotient 0 / 0 is NaN
        again, kept2 = _gauc(rows, perm, start)
        assert got.tobytes() == again.tobytes() and kept.tobytes() == kept2.tobytes()


def test_results_are_bit_reproducible():
    rec, perm, start, _ = _chunk_ref(20, True)
    assert _grouped(rec, perm, start).tobytes() == _grouped(rec, perm, start).tobytes()
    rec, perm, start, _, _ = _count_ref(9, 200)
    assert _grouped(rec, perm, start).tobytes() == _grouped(rec, perm, start).tobytes()


# ---- through the Evaluator: a 40-user x 71-item FOCF model ------------------------------------------------------------------------------

N_USERS, N_ITEMS = 41, 71            # row 0 of either table is [PAD]
TOPK_NAMES = ["Hit", "MRR", "NDCG", "Recall", "Precision", "MAP"]
DP = 12
ROUND = 0.5 * 10.0 ** -DP
COMMON = {"epochs": 1, "train_batch_size": 512, "device": DEV, "embedding_size": 8, "fair_objective": "value",
          "valid_metric_bigger": True, "sst_attr_list": ["gender", "age"], "sst_intersections": [["gender", "age"]],
          "eval_batch_size": 8 * N_ITEMS, "metric_decimal_place": DP}
_runs = {}


def _run(mode, tmp_path_factory, **extra):
    """(trainer, test loader) of a FOCF model trained for one epoch under `eval_args.mode: mode`, once per mode"""
    if mode not in _runs:
        from fairrec.config import Config
        from fairrec.data import dataloader as DL
        from fairrec.data.dataset import synthetic_dataset
        from fairrec.quick_start import run_recbole
        cfg = dict(COMMON, eval_args={"mode": mode}, checkpoint_dir=str(tmp_path_factory.mktemp("group_" + mode)), **extra)
        ds = synthetic_dataset(Config(model="FOCF", dataset="synthetic", config_dict=cfg), N_USERS, N_ITEMS, 1500, seed=11)
        ds.user_feat["age"] = torch.tensor([18, 35, 50])[torch.arange(N_USERS) * 7 % 3]
        seen, loaders, inits = {}, [], {}
        classes = (DL.FullSortEvalDataLoader, DL.NegSampleEvalDataLoader, DL.LabeledEvalDataLoader)

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


def _evaluate(trainer, loader, monkeypatch, **keys):
    """Trainer.evaluate with config keys set for the call -> (result dict, what the Collector handed to the Evaluator)"""
    from fairrec.evaluator import Collector
    get = Collector.get_data_struct
    seen = []

    def recording(self):
        out = get(self)
        seen.append(out)
        return out

    old = {k: trainer.config[k] for k in keys}
    monkeypatch.setattr(Collector, "get_data_struct", recording)
    for k, v in keys.items():
        trainer.config[k] = v
    try:
        res = trainer.evaluate(loader, load_best_model=False)
    finally:
        for k, v in old.items():
            trainer.config[k] = v
        monkeypatch.setattr(Collector, "get_data_struct", get)
    assert len(seen) == 1
    return dict(res), seen[0]


def _name(v):
    return str(int(v)) if float(v).is_integer() else repr(float(v))


def _host_groups(collected, prefix="data.user."):
    """{attribute or intersection: (group index per row, labels)} from the collected attribute columns, on the host"""
    cols = {a: collected[prefix + a].cpu().numpy() for a in ("gender", "age")}
    out = {}
    for a, col in cols.items():
        vals, inv = np.unique(col, return_inverse=True)
        out[a] = (inv.reshape(-1), [_name(v) for v in vals])
    pairs, inv = np.unique(np.stack([cols["gender"].astype(np.float64), cols["age"].astype(np.float64)]), axis=1, return_inverse=True)
    out["gender&age"] = (inv.reshape(-1), [f"{_name(a)}&{_name(b)}" for a, b in pairs.T])
    return out


def _check_utility(res, collected, topk, with_gauc, tag):
    """every per-group key against the host reference on the collected arrays; the summaries against numpy on the group values"""
    rec = collected["rec.topk"].cpu().numpy()
    K = rec.shape[1] - 1
    got, want, bound, expected = [], [], [], set()
    for attr, (gidx, labels) in _host_groups(collected).items():
        G = len(labels)
        assert G >= 2 and gidx.shape[0] == rec.shape[0]
        perm, start = GR.segments(gidx, G)
        ref, sizes = GR.group_topk_ref(rec, perm, start)
        tol = GR.group_topk_tolerance(ref, sizes, K)
        per_metric = {f"{n.lower()}@{k}": (ref[:, m, k - 1], tol[:, m, k - 1]) for m, n in enumerate(TOPK_NAMES) for k in topk}
        if with_gauc:
            sums, _ = GR.group_gauc_ref(collected["rec.meanrank"].cpu().numpy(), perm, start)
            q = sums[:, 0] / sums[:, 1]
            per_metric["gauc"] = (q, (GR.gauc_tolerance(sums, sizes)[:, 0] / sums[:, 0] + 2 * U64) * q)
        for m, (r, t) in per_metric.items():
            assert np.isfinite(r).all(), (attr, m)
            values = np.array([res[f"{m} of {attr}={lab}"] for lab in labels])
            got += values.tolist()
            want += r.tolist()
            bound += (t + ROUND).tolist()
            expected |= {f"{m} of {attr}={lab}" for lab in labels}
            for what, fn in (("gap", lambda v: v.max() - v.min()), ("std", np.std), ("min", np.min)):
                key = f"{m} {what} of sensitive attribute {attr}"
                expected.add(key)
                assert abs(res[key] - fn(values)) <= 4 * ROUND, (key, res[key], fn(values))
    assert {k for k in res if " of " in k and "Unfairness" not in k and "Fairness" not in k} == expected
    _within(tag, got, want, bound)


FULL = dict(metrics=TOPK_NAMES + ["GAUC", "NonParityUnfairness"], topk=[5, 10], valid_metric="ndcg@10")


def test_full_evaluation_by_group_matrix_and_fused(tmp_path_factory, monkeypatch):
    from fairrec.functional import recommend_topk
    from fairrec.utils.case_study import users_per_batch
    trainer, loader = _run("full", tmp_path_factory, **FULL)
    model = trainer.model

    def unmasked(interaction, n_items, sst_list=None):
        """the fused kernel's own matrix of the batch (as tests/test_full_eval_hip.py compares the two paths)"""
        f = model.full_sort_factors(interaction, sst_list, users_per_batch=users_per_batch(trainer.config, n_items))
        return recommend_topk(f["X"], f["W"], 1, want_scores=True, **{k: v for k, v in f.items() if k not in ("X", "W")})[2]

    monkeypatch.setattr(trainer, "_full_sort_scores", unmasked)
    monkeypatch.setattr(trainer, "full_sort_eval", "matrix")
    matrix, collected = _evaluate(trainer, loader, monkeypatch, utility_by_group=True)
    monkeypatch.setattr(trainer, "full_sort_eval", "fused")
    fused, collected_f = _evaluate(trainer, loader, monkeypatch, utility_by_group=True)
    assert {k: repr(v) for k, v in matrix.items()} == {k: repr(v) for k, v in fused.items()}
    assert torch.equal(collected["rec.topk"], collected_f["rec.topk"])
    for a in ("gender", "age"):
        assert torch.equal(collected["data.user." + a], collected_f["data.user." + a])
        assert collected["data.user." + a].shape[0] == collected["rec.topk"].shape[0] > 30
    _check_utility(matrix, collected, [5, 10], True, "Evaluator by group, full mode")
    assert "ndcg@10 of gender=1" in matrix and "gauc of gender&age=0&18" in matrix and "ndcg@10 min of sensitive attribute age" in matrix

    # a list selects its names; the intersection needs all of its attributes
    only, _ = _evaluate(trainer, loader, monkeypatch, utility_by_group=["age"])
    assert "ndcg@10 of age=35" in only and not any("of gender=" in k or "gender&age=" in k for k in only)
    assert all(only[k] == fused[k] for k in only)

    # the key unset: the result keys and the collected keys of before, and the same values
    off, collected_off = _evaluate(trainer, loader, monkeypatch, utility_by_group=None)
    base = {f"{n.lower()}@{k}" for n in TOPK_NAMES for k in (5, 10)} | {"gauc"} | {
        "NonParity Unfairness of sensitive attribute " + a for a in ("gender", "age", "gender&age")}
    assert set(off) == base and all(repr(off[k]) == repr(fused[k]) for k in off)
    assert set(collected_off) - {"data.num_items", "data.count_items"} == {
        "rec.topk", "rec.items", "rec.positive_score", "data.positive_i", "data.gender", "data.age", "rec.meanrank"}
    assert set(collected) - set(collected_off) == {"data.user.gender", "data.user.age"}
    assert not any(k.startswith("data.user.") for k in collected_off)


@pytest.mark.parametrize("K", [10, 63])
def test_uni_evaluation_by_group(K, tmp_path_factory, monkeypatch):
    """negative-sampled candidates: the segment form (K <= 62) and the general form (K = 63) of the candidates branch"""
    trainer, loader = _run("uni5", tmp_path_factory, metrics=["NDCG", "Recall", "GAUC"], topk=[10], valid_metric="ndcg@10")
    res, collected = _evaluate(trainer, loader, monkeypatch, utility_by_group=True, topk=[K])
    assert collected["rec.topk"].shape[1] == K + 1
    # the scattered attribute column is the user's value: the users of the loader in id order
    uids = loader.uid_list.cpu()
    for a in ("gender", "age"):
        assert torch.equal(collected["data.user." + a].cpu(), loader.dataset.user_feat[a].cpu()[uids])
    rec = collected["rec.topk"].cpu().numpy()
    K_ = rec.shape[1] - 1
    got, want, bound = [], [], []
    for attr, (gidx, labels) in _host_groups(collected).items():
        perm, start = GR.segments(gidx, len(labels))
        ref, sizes = GR.group_topk_ref(rec, perm, start)
        tol = GR.group_topk_tolerance(ref, sizes, K_)
        sums, _ = GR.group_gauc_ref(collected["rec.meanrank"].cpu().numpy(), perm, start)
        q = sums[:, 0] / sums[:, 1]
        for g, lab in enumerate(labels):
            got += [res[f"ndcg@{K} of {attr}={lab}"], res[f"recall@{K} of {attr}={lab}"], res[f"gauc of {attr}={lab}"]]
            want += [ref[g, 2, K - 1], ref[g, 3, K - 1], q[g]]
            bound += [tol[g, 2, K - 1] + ROUND, tol[g, 3, K - 1] + ROUND,
                      (GR.gauc_tolerance(sums, sizes)[g, 0] / sums[g, 0] + 2 * U64) * q[g] + ROUND]
        v = np.array([res[f"ndcg@{K} of {attr}={lab}"] for lab in labels])
        assert abs(res[f"ndcg@{K} gap of sensitive attribute {attr}"] - (v.max() - v.min())) <= 4 * ROUND
        assert abs(res[f"ndcg@{K} std of sensitive attribute {attr}"] - v.std()) <= 4 * ROUND
        assert abs(res[f"ndcg@{K} min of sensitive attribute {attr}"] - v.min()) <= 4 * ROUND
    assert np.isfinite(want).all()
    _within(f"Evaluator by group, uni5, K={K}", got, want, bound)


def test_labeled_evaluation_by_group():
    """AUC / LogLoss / MAE / RMSE per group against the float64 restatements of tests/value_metrics_ref.py on every group's rows;
    age 50 has positives only: its AUC is NaN, and so are the three summaries of AUC over age"""
    from fairrec.config import Config
    from fairrec.evaluator import Evaluator
    rng = np.random.default_rng(43)
    n = 300
    score = rng.random(n).astype(np.float32)
    score[::7] = score[1::7][:len(score[::7])]                       # tied scores across the classes
    label = (rng.random(n) < 0.4).astype(np.float32)
    gender = rng.integers(0, 2, n).astype(np.float32)
    age = rng.choice([18, 35, 50], n).astype(np.int64)
    label[age == 50] = 1.0
    names = ["auc", "logloss", "mae", "rmse"]
    keys = {"metrics": ["AUC", "LogLoss", "MAE", "RMSE"], "metric_decimal_place": DP, "sst_attr_list": ["gender", "age"],
            "sst_intersections": [["gender", "age"]], "eval_args": {"mode": "labeled"}, "device": DEV}
    collected = {"rec.score": _dev(score), "data.label": _dev(label), "data.gender": _dev(gender), "data.age": _dev(age)}
    res = Evaluator(Config(model="FOCF", config_dict=dict(keys, utility_by_group=True))).evaluate(collected)
    plain = Evaluator(Config(model="FOCF", config_dict=keys)).evaluate(collected)
    assert sorted(plain) == names and all(repr(res[k]) == repr(plain[k]) for k in plain)
    n_keys = 0
    for attr, (gidx, labels) in _host_groups(collected, prefix="data.").items():
        for m in names:
            values = []
            for g, lab in enumerate(labels):
                rows = gidx == g
                want = V.value_metrics(score[rows], label[rows], [m])[m]
                got = res[f"{m} of {attr}={lab}"]
                values.append(got)
                n_keys += 1
                if math.isnan(want):
                    assert m == "auc" and lab.endswith("50") and math.isnan(got), (attr, m, lab)
                else:
                    assert abs(got - want) <= 1e-9 * abs(want) + ROUND, (attr, m, lab, got, want)
            v = np.array(values)
            for what, fn in (("gap", lambda v: v.max() - v.min()), ("std", np.std), ("min", np.min)):
                key = f"{m} {what} of sensitive attribute {attr}"
                n_keys += 1
                assert np.isnan(res[key]) if np.isnan(v).any() else abs(res[key] - fn(v)) <= 4 * ROUND, key
    assert math.isnan(res["auc of age=50"]) and math.isnan(res["auc gap of sensitive attribute age"])
    assert not math.isnan(res["auc of age=18"]) and not math.isnan(res["auc min of sensitive attribute gender"])
    assert len(res) == 4 + n_keys


def test_labeled_run_reports_by_group(tmp_path_factory, monkeypatch):
    """`eval_args.mode: labeled` end to end: the labeled loader joins the attributes, the Collector keeps them per row"""
    trainer, loader = _run("labeled", tmp_path_factory, metrics=["RMSE", "MAE"], valid_metric="rmse", valid_metric_bigger=False,
                           threshold={"rating": 3})
    res, collected = _evaluate(trainer, loader, monkeypatch, utility_by_group=["gender"])
    assert collected["data.gender"].shape == collected["rec.score"].shape and "data.age" not in collected
    s, y, g = (collected[k].cpu().numpy() for k in ("rec.score", "data.label", "data.gender"))
    for value in (0, 1):
        rows = g == value
        assert rows.sum() > 5
        for m in ("rmse", "mae"):
            want = V.value_metrics(s[rows], y[rows], [m])[m]
            assert abs(res[f"{m} of gender={value}"] - want) <= 1e-9 * abs(want) + ROUND
    assert set(res) == {"rmse", "mae"} | {f"{m} {w}" for m in ("rmse", "mae") for w in (
        "of gender=0", "of gender=1", "gap of sensitive attribute gender", "std of sensitive attribute gender",
        "min of sensitive attribute gender")}


def test_one_value_only_is_refused():
    from fairrec.config import Config
    from fairrec.evaluator import Evaluator
    keys = {"metrics": ["NDCG"], "topk": [3], "sst_attr_list": ["gender"], "eval_args": {"mode": "full"}, "device": DEV}
    collected = {"rec.topk": _dev(R.topk_case(10, 3)), "data.user.gender": torch.ones(10, device=DEV)}
    with pytest.raises(ValueError, match="there is only one value for gender"):
        Evaluator(Config(model="FOCF", config_dict=dict(keys, utility_by_group=True))).evaluate(collected)
    with pytest.raises(ValueError, match="nope"):
        Evaluator(Config(model="FOCF", config_dict=dict(keys, utility_by_group=["nope"])))

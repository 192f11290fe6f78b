"""GPU: exposure metrics per sensitive group -- fr_exposure_grouped (csrc/exposure.hip) through the C ABI against the reference of
tests/exposure_ref.py (pinned to the six existing exposure functions on the CPU by tests/test_exposure_ref.py, where the refusals
of bad arguments are tested too: they need no GPU), then the `exposure_by_group` key through Collector, Evaluator and
Trainer.evaluate on a 40-user x 71-item FOCF model with two attributes and their intersection.  Shapes are the smallest that reach
each edge: groups of 1 / 63 / 64 / 65 / 129 / 257 users with an item every user of the group holds (counts at and across the fold
kernel's 256-count chunk), 1 .. 70 groups, groups contiguous in row order and interleaved, cell heads at the entry positions 0, 63,
64, 65 and at the last entry, cells over a wave boundary, padded lists whose item-0 cell counts more than the group has users.
Every output and the workspace sit between canary frames (sentinel / NaN / 0xFF start values), every return code is asserted, as
in tests/test_metrics_kernels_hip.py.

Exactness: out_i equals the reference integers in every case; m / N and S / (n_g k) / N equal item_coverage / gini_index of the
group's rows bit for bit (gini_index on CPU tensors, where it divides twice as written; on device tensors torch multiplies by the
reciprocals, and the two agree within gamma_4); the three per-entry means equal float(Fraction(sum, n_g k)) and sit within exposure_ref.mean_tolerance
of popularity_percentage / tail_percentage / average_popularity on the group's rows.  The entropy: exposure_ref.entropy_bound.
Every test prints its largest error / bound, none may exceed 1.

Worst error / bound measured on an MI355X, per test group (entropy against exposure_ref.entropy_bound | the three means against
the existing functions within mean_tolerance; the integers, coverage and Gini are exact everywhere):
  counts at the chunk edges 0.16 | 0.064 (K = 62; 0.155 | 0.047 at K = 20; K = 1 is exact: every q is 1)
  1 / 2 / 3 / 9 / 70 groups 0.22 (G = 70) | 0.096 (G = 9); one group over the same rows 0.061 | 0.041
  cell heads at the wave edges 0.35 (two groups, four cells each) | 0.005
  counts above the group size 0.15 | 0.082; ks beyond K 0.081 | 0.042; an empty group 0.085 | 0.11
  evaluator.group_exposure_metrics against the existing functions 0.11
  through the Evaluator: 132 (full), 36 (a list of names) and 132 (uni5) per-group values equal the existing functions on the group's
  rows after rounding to 8 places
"""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import exposure_ref as X
from test_metrics_kernels_hip import _dev, _Frames, _lib, _ptr, _st, _within

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _tables(N):
    """(popular, tail, counts): the masks as popularity_percentage / tail_percentage build them from the counts"""
    from fairrec.evaluator.metrics import _popular_mask, _tail_mask
    counts = X.item_tables(N)[2]
    t = torch.from_numpy(counts)
    return _popular_mask(t).numpy().astype(np.uint8), _tail_mask(t).numpy().astype(np.uint8), counts


def _call(keys, start, n_entries, N, K, G, ks, popular, tail, counts):
    lib, f = _lib(), _Frames()
    n_k = len(ks)
    out_i, out_e = f.new(torch.int64, G, n_k, 5), f.new(torch.float64, G, n_k)
    U = n_entries // K
    need = lib.fr_exposure_grouped_workspace_bytes(U, K, G, n_k)
    assert need == 8 * (G * n_k * 3 + G * n_k * K + (n_k * (U + G) + 1) // 2 + (G * n_k + 1) // 2)
    ws = f.ws(need)
    d = [_dev(x) for x in (keys, start, popular, tail, counts)]
    from fairrec import _C
    rc = lib.fr_exposure_grouped(d[0].data_ptr(), n_entries, N, K, d[1].data_ptr(), G, (_C.c_int32 * n_k)(*ks), n_k, _ptr(d[2]),
                                 _ptr(d[3]), _ptr(d[4]), out_i.data_ptr(), out_e.data_ptr(), ws.data_ptr(), need, _st())
    assert rc == 0, lib.fr_last_error()
    assert f.intact()
    return out_i.cpu().numpy(), out_e.cpu().numpy()


def _run_case(items, gidx, G, N, ks, popular, tail, counts):
    U, K = items.shape
    return _call(X.sorted_keys(items, gidx, N), X.segments(gidx, G), U * K, N, K, G, ks, popular, tail, counts)


def _check_case(tag, items, gidx, G, N, ks, existing=True):
    """the kernel on one case against the reference (integers exact, entropy within its bound) and -- `existing` -- against the
    six existing functions on every group's rows; returns (out_i, entropy)"""
    from fairrec.evaluator import metrics as M
    popular, tail, counts = _tables(N)
    got_i, got_e = _run_case(items, gidx, G, N, ks, popular, tail, counts)
    ref_i, ref_e, info = X.group_ref(items, gidx, G, N, ks, popular, tail, counts)
    assert got_i.tolist() == ref_i, f"{tag}: integer sums differ"
    empty = np.isnan(ref_e.astype(np.float64))
    assert np.array_equal(np.isnan(got_e), empty), f"{tag}: NaN positions differ"
    _within(f"{tag}: entropy", got_e[~empty], ref_e.astype(np.float64)[~empty], X.entropy_bound(info)[~empty])
    # the double nearest the long-double reference is itself up to u / 2 off: entropy_bound's C0 counts it
    sizes = np.bincount(gidx, minlength=G)
    means = X.exact_means(ref_i, sizes, ks)
    K = items.shape[1]
    got_m, want_m, tol_m = [], [], []
    for g in range(G):
        n_g = int(sizes[g])
        if not n_g:
            continue
        rows = _dev(items[gidx == g])
        c = _dev(counts)
        for j, k in enumerate(ks):
            m, S, pop, tl, cnt = (int(v) for v in got_i[g, j])
            for q, v in enumerate((pop, tl, cnt)):
                assert v / (n_g * k) == float(Fraction(v, n_g * k)) == means[g][j][q]
            if not existing:
                continue
            assert m / N == M.item_coverage(rows, N, [k])[f"itemcoverage@{k}"], (tag, g, k)
            gini = float(S) / float(n_g * k) / N
            assert gini == M.gini_index(rows.cpu(), N, [k])[f"giniindex@{k}"], (tag, g, k)
            # (on device tensors torch divides by a Python scalar by multiplying with its reciprocal: two roundings per division)
            assert abs(gini - M.gini_index(rows, N, [k])[f"giniindex@{k}"]) <= X.gamma(4) * abs(gini), (tag, g, k)
            if k <= K:                                   # (`_mean_at_k` reads column k - 1)
                got_m += [pop / (n_g * k), tl / (n_g * k), cnt / (n_g * k)]
                want_m += [M.popularity_percentage(rows, c, [k])[f"popularitypercentage@{k}"],
                           M.tail_percentage(rows, c, [k])[f"tailpercentage@{k}"],
                           M.average_popularity(rows, c, [k])[f"averagepopularity@{k}"]]
                tol_m += [X.mean_tolerance(n_g) * abs(x) for x in got_m[-3:]]
    if want_m:
        _within(f"{tag}: means against _mean_at_k", got_m, want_m, tol_m)
    return got_i, got_e


# ---- the kernel chain ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,ks", X.CHUNK_SHAPES)
def test_counts_at_the_chunk_edges(K, ks):
    for inter in (False, True):
        items, gidx, G, N = X.chunk_case(K, inter)
        got_i, _ = _check_case(f"sizes 1/63/64/65/129/257 K={K} {'interleaved' if inter else 'contiguous'}", items, gidx, G, N, ks)
        assert [int(got_i[g, 0, 0]) >= 1 for g in range(G)] == [True] * G


@pytest.mark.parametrize("G,U", X.GROUP_COUNTS)
def test_group_counts_and_the_whole_population(G, U):
    items, gidx, G, N = X.count_case(G, U)
    ks = X.GROUP_KS
    got_i, _ = _check_case(f"G={G} U={U}", items, gidx, G, N, ks)
    # one group = the whole population (against the six existing functions on all rows, by the same rules) ...
    whole_i, _ = _check_case(f"one group over the U={U} rows", items, np.zeros(U, dtype=np.int64), 1, N, ks)
    # ... and the per-entry integer sums add up over the groups exactly
    assert got_i[:, :, 2:].sum(axis=0).tolist() == whole_i[0, :, 2:].tolist()
    if G == 70:
        assert (np.bincount(gidx) == 1).all()


def test_cell_heads_at_the_wave_edges():
    """heads at the entry positions 0, 63, 64, 65 and the last entry; cells over the wave boundaries at 128 and 192; a group
    boundary on a wave boundary"""
    _check_case("heads at 0 / 50 / 63 / 64 / 65 / 200 / 259", *X.heads_case(), [1])
    _check_case("heads at 0 / 63 / 64 / 65 / 129, two groups", *X.heads_case_two_groups(), [1])


def test_counts_above_the_group_size():
    """padded lists: cell (g, 0) counts more than n_g; a one-user group whose whole list is item 0; two such cells in one (g, j).
    An implementation that clamps a count to n_g fails the integer comparison"""
    items, gidx, G, N = X.padded_case()
    got_i, got_e = _check_case("padded lists", items, gidx, G, N, [1, 5, 10])
    rows = items[gidx == 0]
    assert (np.bincount(rows[:, :10].reshape(-1)) > 30).sum() == 2 and got_i[1, 2, 0] == 1 and got_e[1, 2] == 0.0


def test_cutoff_beyond_the_list_length():
    """ks = [5, 99] with K = 10: the counts are those of the 10 columns, the denominator uses 99"""
    items, gidx, G, N = X.count_case(3, 120)
    got_i, got_e = _check_case("ks = [5, 99], K = 10", items, gidx, G, N, [5, 99])
    at10, e10 = _run_case(items, gidx, G, N, [10], *_tables(N))
    assert got_i[:, 1].tolist() == at10[:, 0].tolist()            # the integers do not see the denominator
    assert (got_e[:, 1] != e10[:, 0]).all()                        # the entropy does


def test_empty_group_in_the_middle():
    items, gidx, G, N = X.empty_group_case()
    got_i, got_e = _check_case("empty group", items, gidx, G, N, X.GROUP_KS)
    assert (got_i[2] == 0).all() and np.isnan(got_e[2]).all() and np.isfinite(got_e[[0, 1, 3]]).all()


def test_optional_arrays_may_be_null():
    items, gidx, G, N = X.count_case(3, 120)
    popular, tail, counts = _tables(N)
    full_i, full_e = _run_case(items, gidx, G, N, X.GROUP_KS, popular, tail, counts)
    assert (full_i[:, :, 2:] > 0).all()
    for drop in range(3):
        arrays = [popular, tail, counts]
        arrays[drop] = None
        got_i, got_e = _run_case(items, gidx, G, N, X.GROUP_KS, *arrays)
        want = full_i.copy()
        want[:, :, 2 + drop] = 0
        assert np.array_equal(got_i, want) and got_e.tobytes() == full_e.tobytes(), drop
    got_i, _ = _run_case(items, gidx, G, N, X.GROUP_KS, None, None, None)
    assert (got_i[:, :, 2:] == 0).all() and np.array_equal(got_i[:, :, :2], full_i[:, :, :2])


def test_results_are_bit_reproducible():
    items, gidx, G, N = X.chunk_case(20, True)
    a = _run_case(items, gidx, G, N, [5, 10, 20], *_tables(N))
    b = _run_case(items, gidx, G, N, [5, 10, 20], *_tables(N))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    items, gidx, G, N = X.padded_case()
    a = _run_case(items, gidx, G, N, [1, 5, 10], *_tables(N))
    b = _run_case(items, gidx, G, N, [1, 5, 10], *_tables(N))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_malformed_input_stays_inside_the_arrays():
    """unsorted keys, keys whose group part is >= n_groups, negative keys, a group_start beyond n_users / descending: unspecified
    values, every frame intact"""
    items, gidx, G, N = X.count_case(3, 120)
    U, K = items.shape
    popular, tail, counts = _tables(N)
    keys = X.sorted_keys(items, gidx, N)
    start = X.segments(gidx, G)
    shuffled = np.random.default_rng(1).permutation(keys)
    beyond = keys.copy()
    beyond[-200:] += 5 * N * K
    beyond[:3] = (-9, -1, -2 ** 62)
    beyond[-1] = 2 ** 63 - 1
    for k_, s_ in ((shuffled, start), (beyond, start), (keys, np.array([0, 500, 20, U], dtype=np.int64)),
                   (keys, np.array([-9, 10, 10 ** 15, U], dtype=np.int64)), (shuffled, np.array([60, 0, 0, 0], dtype=np.int64))):
        _call(k_, s_, U * K, N, K, G, X.GROUP_KS, popular, tail, counts)


def test_python_wrapper():
    from fairrec.evaluator import group_exposure_metrics
    from fairrec.evaluator import metrics as M
    items, gidx, G, N = X.empty_group_case()
    counts = _dev(X.item_tables(N)[2])
    names = list(M.EXPOSURE_NAMES)
    got = group_exposure_metrics(_dev(items), _dev(gidx), G, N, counts, [5, 10], names)
    assert sorted(got) == sorted(f"{n}@{k}" for n in names for k in (5, 10))
    fns = {"giniindex": lambda r, k: M.gini_index(r, N, [k]), "itemcoverage": lambda r, k: M.item_coverage(r, N, [k]),
           "shannonentropy": lambda r, k: M.shannon_entropy(r, [k]), "popularitypercentage": lambda r, k: M.popularity_percentage(r, counts, [k]),
           "tailpercentage": lambda r, k: M.tail_percentage(r, counts, [k]), "averagepopularity": lambda r, k: M.average_popularity(r, counts, [k])}
    vals, want, tol = [], [], []
    sizes = np.bincount(gidx, minlength=G)
    for key, per_group in got.items():
        name, k = key.split("@")
        assert len(per_group) == G and math.isnan(per_group[2])
        for g in (0, 1, 3):
            w = fns[name](_dev(items[gidx == g]), int(k))[key]
            if name == "itemcoverage":
                assert per_group[g] == w, (key, g)
            if name == "giniindex":                       # bit for bit where gini_index divides (CPU tensors; see _check_case)
                assert per_group[g] == M.gini_index(torch.from_numpy(items[gidx == g]), N, [int(k)])[key], (key, g)
            vals.append(per_group[g])
            want.append(w)
            # the entropy: both sides sum at most N terms of a few roundings and a logarithm each (exposure_ref, test_exposure_ref)
            tol.append({"giniindex": X.gamma(4), "itemcoverage": 0.0, "shannonentropy": 2 * X.gamma(N + X.C0 + X.E_LOG + 1)}.get(
                name, X.mean_tolerance(int(sizes[g]))) * abs(w))
    _within("evaluator.group_exposure_metrics against the existing functions", vals, want, tol)
    with pytest.raises(ValueError, match="do not fit"):
        group_exposure_metrics(_dev(items), _dev(gidx), 2 ** 40, 2 ** 20, counts, [5], ["giniindex"])
    with pytest.raises(ValueError, match="group indices"):
        group_exposure_metrics(_dev(items), _dev(gidx[:5]), G, N, counts, [5], ["giniindex"])
    # more cut-offs than one call takes
    many = group_exposure_metrics(_dev(items), _dev(gidx), G, N, counts, list(range(1, 11)), ["itemcoverage"])
    for key in ("itemcoverage@5", "itemcoverage@10"):
        assert np.array_equal(many[key], got[key], equal_nan=True), key


# ---- through the Evaluator: a 40-user x 71-item FOCF model ------------------------------------------------------------------------------

N_USERS, N_ITEMS = 41, 71            # row 0 of either table is [PAD]
EXPOSURE = ["GiniIndex", "ItemCoverage", "ShannonEntropy", "PopularityPercentage", "TailPercentage", "AveragePopularity"]
DP = 8
ROUND = 0.5 * 10.0 ** -DP
COMMON = {"epochs": 1, "train_batch_size": 512, "device": DEV, "embedding_size": 8, "fair_objective": "value",
          "valid_metric_bigger": True, "sst_attr_list": ["gender", "age"], "sst_intersections": [["gender", "age"]],
          "eval_batch_size": 8 * N_ITEMS, "metric_decimal_place": DP, "metrics": ["NDCG"] + EXPOSURE, "valid_metric": "ndcg@10"}
_runs = {}


def _run(mode, tmp_path_factory, **extra):
    """(trainer, test loader) of a FOCF model trained for one epoch under `eval_args.mode: mode`, once per mode"""
    if mode not in _runs:
        from fairrec.config import Config
        from fairrec.data import dataloader as DL
        from fairrec.data.dataset import synthetic_dataset
        from fairrec.quick_start import run_recbole
        cfg = dict(COMMON, eval_args={"mode": mode}, checkpoint_dir=str(tmp_path_factory.mktemp("exposure_" + mode)), **extra)
        ds = synthetic_dataset(Config(model="FOCF", dataset="synthetic", config_dict=cfg), N_USERS, N_ITEMS, 1500, seed=11)
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


MISSING = object()


def _evaluate(trainer, loader, monkeypatch, **keys):
    """Trainer.evaluate with config keys set for the call (MISSING: the key taken out of the config) -> (result dict, what the
    Collector handed to the Evaluator)"""
    from fairrec.evaluator import Collector
    get = Collector.get_data_struct
    seen = []

    def recording(self):
        out = get(self)
        seen.append(out)
        return out

    conf = trainer.config.final_config_dict
    old = {k: conf.get(k, MISSING) for k in keys}
    monkeypatch.setattr(Collector, "get_data_struct", recording)
    for k, v in keys.items():
        if v is MISSING:
            conf.pop(k, None)
        else:
            conf[k] = v
    try:
        res = trainer.evaluate(loader, load_best_model=False)
    finally:
        for k, v in old.items():
            if v is MISSING:
                conf.pop(k, None)
            else:
                conf[k] = v
        monkeypatch.setattr(Collector, "get_data_struct", get)
    assert len(seen) == 1
    return dict(res), seen[0]


def _name(v):
    return str(int(v)) if float(v).is_integer() else repr(float(v))


def _host_groups(collected, attrs=("gender", "age"), pair=True):
    """{attribute or intersection: (group index per row, labels)} from the collected attribute columns, on the host"""
    cols = {a: collected["data.user." + a].cpu().numpy() for a in attrs}
    out = {}
    for a, col in cols.items():
        vals, inv = np.unique(col, return_inverse=True)
        out[a] = (inv.reshape(-1), [_name(v) for v in vals])
    if pair:
        pairs, inv = np.unique(np.stack([cols["gender"].astype(np.float64), cols["age"].astype(np.float64)]), axis=1,
                               return_inverse=True)
        out["gender&age"] = (inv.reshape(-1), [f"{_name(a)}&{_name(b)}" for a, b in pairs.T])
    return out


def _check_exposure(res, collected, topk, groups, tag):
    """every per-group key = the existing function on that group's rows of the collected `rec.items`, rounded to DP places; the
    four summaries against numpy on the group values; no other per-group key"""
    from fairrec.evaluator import metrics as M
    items, N, counts = collected["rec.items"], collected["data.num_items"], collected["data.count_items"]
    expected = set()
    n = 0
    for attr, (gidx, labels) in groups.items():
        assert len(labels) >= 2 and gidx.shape[0] == items.shape[0]
        per_metric = {}
        for g, lab in enumerate(labels):
            rows = items[torch.from_numpy(gidx == g).to(items.device)]
            assert rows.shape[0] >= 1
            want = {}
            for d in (M.gini_index(rows, N, topk), M.item_coverage(rows, N, topk), M.shannon_entropy(rows, topk),
                      M.popularity_percentage(rows, counts, topk), M.tail_percentage(rows, counts, topk),
                      M.average_popularity(rows, counts, topk)):
                want.update(d)
            for m, w in want.items():
                key = f"{m} of {attr}={lab}"
                expected.add(key)
                assert res[key] == round(w, DP), (key, res[key], w)
                per_metric.setdefault(m, []).append(res[key])
                n += 1
        for m, values in per_metric.items():
            v = np.array(values)
            for what, fn in (("gap", lambda v: v.max() - v.min()), ("std", np.std), ("min", np.min), ("max", np.max)):
                key = f"{m} {what} of sensitive attribute {attr}"
                expected.add(key)
                assert abs(res[key] - fn(v)) <= 4 * ROUND, (key, res[key], fn(v))
    assert {k for k in res if " of " in k and "Unfairness" not in k and "Fairness" not in k} == expected
    print(f"{tag}: {n} per-group values equal the existing functions on the group's rows after rounding to {DP} places")


def test_full_evaluation_by_group(tmp_path_factory, monkeypatch):
    trainer, loader = _run("full", tmp_path_factory, topk=[5, 10])
    res, collected = _evaluate(trainer, loader, monkeypatch, exposure_by_group=True)
    assert collected["rec.items"].shape[0] == collected["data.user.gender"].shape[0] > 30
    _check_exposure(res, collected, [5, 10], _host_groups(collected), "Evaluator by group, full mode")
    assert "giniindex@10 of gender=1" in res and "shannonentropy@5 of gender&age=0&18" in res
    assert "averagepopularity@10 max of sensitive attribute age" in res

    # a list selects its names; the intersection needs all of its attributes
    only, collected_o = _evaluate(trainer, loader, monkeypatch, exposure_by_group=["age"])
    assert "giniindex@10 of age=35" in only and not any("of gender=" in k or "gender&age=" in k for k in only)
    assert all(only[k] == res[k] for k in only) and "data.user.gender" not in collected_o
    _check_exposure(only, collected_o, [5, 10], _host_groups(collected_o, ("age",), pair=False), "exposure_by_group: ['age']")

    # `utility_by_group` alone keeps producing no per-group exposure key; both keys together give both halves
    util, _ = _evaluate(trainer, loader, monkeypatch, utility_by_group=True)
    assert "ndcg@10 of gender=1" in util and not any(k.split("@")[0] in [e.lower() for e in EXPOSURE] and " of " in k for k in util)
    both, _ = _evaluate(trainer, loader, monkeypatch, utility_by_group=True, exposure_by_group=True)
    assert both == {**util, **res}

    # the key unset: the result dict and the collected keys of a config that never mentions the key
    unset, collected_u = _evaluate(trainer, loader, monkeypatch, exposure_by_group=None)
    never, collected_n = _evaluate(trainer, loader, monkeypatch, exposure_by_group=MISSING)
    assert {k: repr(v) for k, v in unset.items()} == {k: repr(v) for k, v in never.items()}
    assert set(collected_u) == set(collected_n) and not any(k.startswith("data.user.") for k in collected_u)
    assert not any(" of " in k and "sensitive attribute" not in k for k in unset)
    assert all(repr(unset[k]) == repr(res[k]) for k in unset)

    with pytest.raises(ValueError, match="nope"):
        _evaluate(trainer, loader, monkeypatch, exposure_by_group=["nope"])


def test_uni_evaluation_by_group(tmp_path_factory, monkeypatch):
    """negative-sampled candidates: users with fewer than K candidates get their list filled up (the candidates branch)"""
    trainer, loader = _run("uni5", tmp_path_factory, topk=[10])
    res, collected = _evaluate(trainer, loader, monkeypatch, exposure_by_group=True, topk=[5, 10])
    items = collected["rec.items"]
    assert items.shape[1] == 10
    _check_exposure(res, collected, [5, 10], _host_groups(collected), "Evaluator by group, uni5")


def test_labeled_mode_and_strangers_are_refused():
    from fairrec.config import Config
    from fairrec.evaluator import Evaluator
    keys = {"metrics": ["GiniIndex"], "topk": [3], "sst_attr_list": ["gender"], "eval_args": {"mode": "full"}, "device": DEV}
    with pytest.raises(ValueError, match="nope"):
        Evaluator(Config(model="FOCF", config_dict=dict(keys, exposure_by_group=["nope"])))
    labeled = dict(keys, metrics=["AUC"], eval_args={"mode": "labeled"})
    with pytest.raises(ValueError, match="exposure_by_group"):
        Evaluator(Config(model="FOCF", config_dict=dict(labeled, exposure_by_group=True)))
    collected = {"rec.items": torch.ones((10, 3), dtype=torch.int64, device=DEV), "data.num_items": 5,
                 "data.count_items": torch.ones(5, dtype=torch.int64, device=DEV), "data.user.gender": torch.ones(10, device=DEV)}
    with pytest.raises(ValueError, match="there is only one value for gender"):
        Evaluator(Config(model="FOCF", config_dict=dict(keys, exposure_by_group=True))).evaluate(collected)

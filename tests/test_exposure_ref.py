"""CPU: the reference of tests/exposure_ref.py before anything runs on a GPU, and what of `exposure_by_group` needs none.

* the reference against the six existing exposure functions of fairrec.evaluator.metrics on CPU tensors, applied to each group's
  rows, on 200 random cases with repeated items and padded lists: GiniIndex and ItemCoverage bit for bit (the histogram form and
  the two divisions of gini_index give the same doubles while the sums stay below 2^53), the three means within
  exposure_ref.mean_tolerance, ShannonEntropy within gamma_(m + 6) of its value (m terms of four roundings and a logarithm each,
  their sum, one division);
* the case builders reach what they promise (group sizes, head positions, counts above n_g, the empty group);
* fr_exposure_grouped refuses bad arguments before anything is launched or written (host buffers: a refused call never follows
  a pointer), and fr_exposure_grouped_workspace_bytes returns 0 out of range;
* the `exposure_by_group` key: its values, the ValueError for a stranger, for a value of another type and in labeled mode, the
  attributes the Collector keeps for the union of both keys, and nothing kept with the keys unset.
"""
import ctypes

import numpy as np
import pytest
import torch

import exposure_ref as X

EINVAL = -1


def _existing(rows, N, counts, ks):
    """the six existing functions on one group's rows (CPU tensors) -> {name: [value per k]}"""
    from fairrec.evaluator import metrics as M
    t, c = torch.from_numpy(rows), torch.from_numpy(counts)
    out = {}
    for d in (M.gini_index(t, N, ks), M.item_coverage(t, N, ks), M.shannon_entropy(t, ks), M.popularity_percentage(t, c, ks),
              M.tail_percentage(t, c, ks), M.average_popularity(t, c, ks)):
        for key, v in d.items():
            out.setdefault(key.split("@")[0], []).append(v)
    return out


def test_reference_matches_the_existing_functions_on_each_groups_rows():
    from fairrec.evaluator.metrics import _popular_mask, _tail_mask
    rng = np.random.default_rng(2024)
    worst = {"shannonentropy": 0.0, "means": 0.0}
    for case in range(200):
        U, K, N, G = int(rng.integers(3, 40)), int(rng.integers(1, 9)), int(rng.integers(5, 30)), int(rng.integers(1, 4))
        items = rng.integers(1, N, (U, K)).astype(np.int64)
        if case % 2:                                      # padded lists: item 0 from a random rank on
            cut = rng.integers(0, K + 1, U)
            items[np.arange(K)[None, :] >= cut[:, None]] = 0
        gidx = np.concatenate((np.arange(G), rng.integers(0, G, U - G))).astype(np.int64)
        counts = rng.integers(0, 50, N).astype(np.int64)
        counts[1] = 7                                     # (at least one item occurs in training)
        ks = sorted(set(rng.integers(1, K + 1, 2).tolist()))
        popular = _popular_mask(torch.from_numpy(counts)).numpy().astype(np.uint8)
        tail = _tail_mask(torch.from_numpy(counts)).numpy().astype(np.uint8)
        out_i, ent, _ = X.group_ref(items, gidx, G, N, ks, popular, tail, counts)
        sizes = np.bincount(gidx, minlength=G)
        means = X.exact_means(out_i, sizes, ks)
        for g in range(G):
            want = _existing(items[gidx == g], N, counts, ks)
            n_g = int(sizes[g])
            for j, k in enumerate(ks):
                m, S = out_i[g][j][:2]
                assert S < 2 ** 53 and float(S) / float(n_g * k) / N == want["giniindex"][j], (case, g, k)
                assert m / N == want["itemcoverage"][j], (case, g, k)
                h = float(ent[g][j]) / m
                err = abs(h - want["shannonentropy"][j])
                assert err <= X.gamma(m + 6) * abs(h), (case, g, k, h, want["shannonentropy"][j])
                if h:
                    worst["shannonentropy"] = max(worst["shannonentropy"], err / (X.gamma(m + 6) * abs(h)))
                for q, name in enumerate(("popularitypercentage", "tailpercentage", "averagepopularity")):
                    err, tol = abs(means[g][j][q] - want[name][j]), X.mean_tolerance(n_g) * abs(means[g][j][q])
                    assert err <= tol, (case, g, k, name, means[g][j][q], want[name][j])
                    if tol:
                        worst["means"] = max(worst["means"], err / tol)
    print("largest error / bound against the existing functions:", worst)


def test_case_builders_reach_their_edges():
    for K, ks in X.CHUNK_SHAPES:
        for inter in (False, True):
            items, gidx, G, N = X.chunk_case(K, inter)
            assert np.bincount(gidx).tolist() == X.CHUNK_SIZES and items.shape == (sum(X.CHUNK_SIZES), K) and max(ks) <= K
            assert (items[:, 0] == 3).all()                              # count n_g: the last slot of every segment
            assert ((np.diff(gidx) != 0).sum() > 100) == inter
    for G, U in X.GROUP_COUNTS:
        items, gidx, G_, N = X.count_case(G, U)
        assert sorted(set(gidx.tolist())) == list(range(G)) and items.shape == (U, X.GROUP_K)
    assert (np.bincount(X.count_case(70, 70)[1]) == 1).all()
    # heads: the sorted keys of the K = 1 case are the sorted items
    items, gidx, G, N = X.heads_case()
    keys = X.sorted_keys(items, gidx, N)
    heads = np.nonzero(np.concatenate(([True], keys[1:] != keys[:-1])))[0]
    assert heads.tolist() == [0, 50, 63, 64, 65, 200, 259] and keys.shape[0] == 260
    items, gidx, G, N = X.heads_case_two_groups()
    keys = X.sorted_keys(items, gidx, N)
    heads = np.nonzero(np.concatenate(([True], keys[1:] != keys[:-1])))[0]
    assert heads.tolist() == [0, 63, 64, 65, 129] and keys.shape[0] == 130 and keys[64] // N == 1 and keys[63] // N == 0
    # padded: counts above n_g, two of them in (group 0, k = 5 and 10), the one-user group all item 0
    items, gidx, G, N = X.padded_case()
    for g, n_g, over in ((0, 30, {1: 0, 5: 2, 10: 2}), (1, 1, {1: 0, 5: 1, 10: 1}), (2, 12, {1: 0, 5: 0, 10: 1})):
        rows = items[gidx == g]
        assert rows.shape[0] == n_g
        for k, n_over in over.items():
            assert (np.bincount(rows[:, :k].reshape(-1)) > n_g).sum() == n_over, (g, k)
    assert (items[gidx == 1] == 0).all()
    items, gidx, G, N = X.empty_group_case()
    assert np.bincount(gidx, minlength=G).tolist() == [40, 17, 0, 33]
    assert len(X.kernel_cases()) == 16


def test_reference_of_one_group_is_the_sum_of_its_parts():
    """the integer per-entry sums add up over the groups; an empty group is five zeros and NaN"""
    items, gidx, G, N = X.count_case(9, 200)
    popular, tail, counts = X.item_tables(N)
    parts, _, _ = X.group_ref(items, gidx, G, N, X.GROUP_KS, popular, tail, counts)
    whole, _, _ = X.group_ref(items, np.zeros_like(gidx), 1, N, X.GROUP_KS, popular, tail, counts)
    for j in range(len(X.GROUP_KS)):
        for q in (2, 3, 4):
            assert sum(parts[g][j][q] for g in range(G)) == whole[0][j][q] > 0
    items, gidx, G, N = X.empty_group_case()
    out_i, ent, info = X.group_ref(items, gidx, G, N, X.GROUP_KS, popular, tail, counts)
    assert out_i[2] == [[0] * 5] * 2 and np.isnan(ent[2]).all() and np.isfinite(ent[[0, 1, 3]]).all()


# ---- refusals: the error code, fr_last_error, nothing written (no GPU: a refused call follows no pointer) -----------------------------

def _host(dtype, n, fill):
    a = np.full(n, fill, dtype=dtype)
    return a, a.ctypes.data


def _ks(*values):
    return (ctypes.c_int32 * len(values))(*values)


def test_exposure_grouped_refuses_bad_arguments_without_gpu():
    from fairrec import _C
    lib = _C.lib()
    U, K, N, G, n_k = 65, 10, 50, 4, 2
    need = lib.fr_exposure_grouped_workspace_bytes(U, K, G, n_k)
    assert need == 8 * (G * n_k * 3 + G * n_k * K + (n_k * (U + G) + 1) // 2 + (G * n_k + 1) // 2)
    keys, keys_p = _host(np.int64, U * K, 0)
    start, start_p = _host(np.int64, G + 1, 0)
    flag, flag_p = _host(np.uint8, N, 0)
    cnt, cnt_p = _host(np.int64, N, 0)
    out_i, out_i_p = _host(np.int64, G * n_k * 5, -77)
    out_e, out_e_p = _host(np.float64, G * n_k, 1234.5)
    ws, ws_p = _host(np.uint8, need, 0xA5)
    good = [keys_p, U * K, N, K, start_p, G, _ks(5, 10), n_k, flag_p, flag_p, cnt_p, out_i_p, out_e_p, ws_p, need]
    bad_args = [(0, 0), (4, 0), (6, None), (11, 0), (12, 0), (13, 0),                      # null pointers
                (1, 0), (1, -10), (2, 0), (2, -1), (3, 0), (3, -1), (5, 0), (5, -1),        # sizes below 1
                (1, U * K + 1),                                                             # no multiple of k_cols
                (7, 0), (7, -1), (7, 9),                                                    # n_k outside 1..8
                (6, _ks(10, 5)), (6, _ks(5, 5)), (6, _ks(0, 5)), (6, _ks(-3, 5)),           # ks not strictly ascending / below 1
                (5, 2 ** 63 // (N * K) + 1),                                                # G N K >= 2^63
                (2, 2 ** 62 // (U * K) + 1),                                                # N U K >= 2^62
                (14, need - 1), (14, 0)]                                                    # workspace too small
    for pos, bad in bad_args:
        args = list(good)
        args[pos] = bad
        rc = lib.fr_exposure_grouped(*args, None)
        assert rc == EINVAL and b"fr_exposure_grouped" in lib.fr_last_error(), (pos, bad, rc)
        assert (out_i == -77).all() and (out_e == 1234.5).all() and (ws == 0xA5).all()
    for args in ((0, K, G, n_k), (-1, K, G, n_k), (U, 0, G, n_k), (U, -1, G, n_k), (U, K, 0, n_k), (U, K, -1, n_k), (U, K, G, 0),
                 (U, K, G, 9), (U, K, G, -1), (U, K, 2 ** 31, n_k), (2 ** 41, K, G, n_k)):
        assert lib.fr_exposure_grouped_workspace_bytes(*args) == 0, args
    assert lib.fr_exposure_grouped_workspace_bytes(1, 1, 1, 1) == 8 * (3 + 1 + 1 + 1)
    assert ctypes.sizeof(ctypes.c_size_t) == 8


# ---- the config key ------------------------------------------------------------------------------------------------------------------

def _config(**kw):
    from fairrec.config import Config
    base = {"metrics": ["NDCG", "GiniIndex"], "topk": [5], "sst_attr_list": ["gender", "age"], "eval_args": {"mode": "full"},
            "device": "cpu"}
    return Config(model="FOCF", config_dict=dict(base, **kw))


def test_exposure_by_group_key_values():
    from fairrec.evaluator import Collector, Evaluator
    assert _config()["exposure_by_group"] is None                                       # the default of overall.yaml: off
    for value, want in ((None, []), (False, []), (True, ["gender", "age"]), (["age"], ["age"]), (["age", "gender"], ["age", "gender"]),
                        ([], [])):
        cfg = _config(exposure_by_group=value)
        assert Evaluator(cfg).exposure == want and Collector(cfg).exposure == want, value
        assert Evaluator(cfg).utility == [] and Collector(cfg).user_attrs == want
    with pytest.raises(ValueError, match="exposure_by_group.*nope"):
        Evaluator(_config(exposure_by_group=["nope"]))
    with pytest.raises(ValueError, match="exposure_by_group.*nope"):
        Collector(_config(exposure_by_group=["gender", "nope"]))
    for value in ("gender", 3, 1.5, {"gender": True}, [1, 2]):
        with pytest.raises(ValueError, match="exposure_by_group must be"):
            Evaluator(_config(exposure_by_group=value))
    with pytest.raises(ValueError, match="utility_by_group.*nope"):                      # the other key keeps its own name
        Evaluator(_config(utility_by_group=["nope"]))


def test_labeled_mode_refuses_the_key():
    from fairrec.evaluator import Evaluator
    labeled = dict(metrics=["AUC"], eval_args={"mode": "labeled"}, LABEL_FIELD="label")
    Evaluator(_config(**labeled))
    Evaluator(_config(utility_by_group=True, **labeled))
    with pytest.raises(ValueError, match="exposure_by_group"):
        Evaluator(_config(exposure_by_group=True, **labeled))
    with pytest.raises(ValueError, match="exposure_by_group"):
        Evaluator(_config(exposure_by_group=["age"], **labeled))


def test_collector_keeps_the_union_of_both_keys():
    from fairrec.evaluator import Collector
    both = Collector(_config(utility_by_group=["age"], exposure_by_group=["gender", "age"]))
    assert both.utility == ["age"] and both.exposure == ["gender", "age"] and both.user_attrs == ["age", "gender"]
    off = Collector(_config())
    assert off.user_attrs == [] and off.utility == [] and off.exposure == []


def test_mask_helpers_are_what_the_two_functions_use():
    """popularity_percentage / tail_percentage through their shared mask helpers, against the masks spelt out"""
    from fairrec.evaluator import metrics as M
    rng = np.random.default_rng(8)
    counts = torch.from_numpy(rng.integers(0, 30, 40).astype(np.int64))
    rec = torch.from_numpy(rng.integers(0, 40, (25, 6)).astype(np.int64))
    present = [i for i in range(40) if counts[i] > 0]
    for ratio in (None, 0.3, 5):
        r = 0.1 if ratio is None else ratio
        by_desc = sorted(present, key=lambda i: (-int(counts[i]), -i))
        by_asc = sorted(present, key=lambda i: (int(counts[i]), i))
        popular = {i for i in range(40) if counts[i] >= r} if r > 1 else set(by_desc[:max(int(len(present) * r), 1)])
        tail = {i for i in present if counts[i] <= r} if r > 1 else set(by_asc[:max(int(len(present) * r), 1)])
        assert set(torch.nonzero(M._popular_mask(counts, ratio)).view(-1).tolist()) == popular
        assert set(torch.nonzero(M._tail_mask(counts, ratio)).view(-1).tolist()) == tail
        for k in (1, 6):
            want_p = np.mean([sum(int(i) in popular for i in row[:k]) / k for row in rec.tolist()])
            want_t = np.mean([sum(int(i) in tail for i in row[:k]) / k for row in rec.tolist()])
            assert abs(M.popularity_percentage(rec, counts, [k], ratio)[f"popularitypercentage@{k}"] - want_p) < 1e-12
            assert abs(M.tail_percentage(rec, counts, [k], ratio)[f"tailpercentage@{k}"] - want_t) < 1e-12

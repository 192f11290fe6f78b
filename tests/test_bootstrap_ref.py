"""CPU: the references of tests/bootstrap_ref.py before anything runs on a GPU, and what of `group_bootstrap` needs none.

* Philox4x32-10 against the three Random123 known answers; the twelve thresholds recomputed from `decimal` at 50 digits; the
  weight at both sides of every threshold;
* the definition, statistically: the standard deviation of the replicate means of 2000 values over std / sqrt(n) lies in
  [0.85, 1.15] for B = 400 and three seeds (measured 0.972, 1.035, 1.058; four standard errors of the ratio are 0.14);
* the exact weighted sum against Fractions; the user terms against the grouped references they restate;
* fairrec.evaluator.bootstrap_intervals against a hand-written case and against intervals_ref: a NaN replicate, a group unusable in
  more than half of the replicates (NaN interval, the warning captured), G = 2 and G = 6;
* fr_bootstrap_group_sums / fr_topk_user_terms / fr_gauc_user_terms refuse bad arguments before anything is launched or written
  (host buffers: a refused call never follows a pointer), and the workspace function returns 0 out of range;
* the `group_bootstrap` / `group_bootstrap_level` keys: their values, the ValueErrors, and no `ci_` key with the key unset.
"""
import logging
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import bootstrap_ref as BR
import group_metrics_ref as GR
import metrics_ref as R

EINVAL = -1


# ---- the weights -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, want):
    assert tuple(int(x) for x in BR.philox4x32_10(counter, key)) == want


def test_thresholds_and_the_weight_at_their_edges():
    assert BR.thresholds_from_decimal() == BR.T and len(BR.T) == 12 and list(BR.T) == sorted(set(BR.T))
    for j, t in enumerate(BR.T):
        assert int(BR.weight_of(t - 1)) == j and int(BR.weight_of(t)) == j + 1
    assert int(BR.weight_of(0)) == 0 and int(BR.weight_of(0xffffffff)) == 12


def test_weights_follow_the_counter_layout():
    """w(r, b) reads word b & 3 of the call with counter (r, 0, b >> 2, 0); a row's weights do not depend on the other rows"""
    seed = (0x1234 << 32) | 0xabcdef01
    w = BR.weights([0, 5, 70000, 2 ** 31 - 1], 9, seed)
    assert w.shape == (4, 9) and w.dtype == np.int64
    for i, r in enumerate((0, 5, 70000, 2 ** 31 - 1)):
        for b in range(9):
            words = BR.philox4x32_10((r, 0, b >> 2, 0), (0xabcdef01, 0x1234))
            assert w[i, b] == int(BR.weight_of(words[b & 3]))
    assert np.array_equal(BR.weights([70000], 9, seed)[0], w[2])
    assert not np.array_equal(BR.weights([0, 5], 64, 1), BR.weights([0, 5], 64, 2))
    many = BR.weights(np.arange(20000), 64, 2020)
    assert abs(many.mean() - 1.0) < 0.01 and abs(many.var() - 1.0) < 0.02 and many.max() <= 12


@pytest.mark.parametrize("seed", [2020, 7, 1])
def test_replicate_means_spread_like_the_standard_error(seed):
    x = np.random.default_rng(5).random(2000)
    w = BR.weights(np.arange(2000), 400, seed)
    means = (w * x[:, None]).sum(axis=0) / w.sum(axis=0)
    ratio = means.std() / (x.std() / math.sqrt(2000))
    print(f"seed {seed}: std of the replicate means / (std / sqrt(n)) = {ratio:.3f}")
    assert 0.85 <= ratio <= 1.15


# ---- the reference sums and terms ------------------------------------------------------------------------------------------------

def test_exact_weighted_sum_against_fractions():
    v = BR.values_case(70, 3)
    perm, start = GR.segments(GR.assignment(70, 2), 2)
    sums, weight, absw, sizes = BR.group_sums_ref(v, perm, start, 5, 11)
    assert sizes.tolist() == [35, 35]
    for g in range(2):
        rows = perm[start[g]:start[g + 1]]
        w = BR.weights(rows, 5, 11)
        assert weight[g].tolist() == w.sum(axis=0).tolist()
        for b in range(5):
            for c in range(3):
                exact = sum((int(w[i, b]) * Fraction(float(v[r, c])) for i, r in enumerate(rows)), Fraction(0))
                assert sums[g, b, c] == float(exact)
                assert absw[g, b, c] == float(sum((int(w[i, b]) * abs(Fraction(float(v[r, c]))) for i, r in enumerate(rows)), Fraction(0)))
    # an empty group: zeros; a NaN value: its (group, column) NaN in every replicate, nothing else
    v[perm[3], 1] = np.nan
    s2, w2, _, _ = BR.group_sums_ref(v, perm, np.array([0, 0, 35, 70]), 5, 11)
    assert (s2[0] == 0).all() and (w2[0] == 0).all() and np.isnan(s2[1, :, 1]).all()
    assert np.array_equal(s2[1][:, [0, 2]], sums[0][:, [0, 2]]) and np.array_equal(s2[2], sums[1])


def test_user_terms_restate_the_grouped_references():
    rec = R.topk_case(40, 10, zero_positive_row=7)
    columns = [(m, k) for m in BR.TOPK_NAMES for k in (1, 5, 10)]
    terms = BR.topk_user_terms_ref(rec, columns)
    whole = R.topk_metrics_ref(rec)
    for j, (m, k) in enumerate(columns):
        want = whole[BR.TOPK_NAMES.index(m), k - 1]
        if m == "recall":
            assert math.isnan(terms[7, j]) and math.isnan(want)
        else:
            assert abs(terms[:, j].mean() - want) <= 1e-13 * want
    assert terms[7, columns.index(("ndcg", 10))] == 0 and terms[7, columns.index(("map", 10))] == 0
    t = GR.meanrank_case(50)
    t[3], t[4] = (0, 30, 0), (20, 4, 4)
    g = BR.gauc_user_terms_ref(t)
    assert (g[3] == 0).all() and (g[4] == 0).all() and (g[:3] > 0).all()
    want = GR.gauc_float64(t)
    assert abs(g[:, 0].sum() / g[:, 1].sum() - want) <= 1e-13 * want


# ---- bootstrap_intervals ---------------------------------------------------------------------------------------------------------

def test_intervals_hand_written_case(caplog):
    from fairrec.evaluator import bootstrap_intervals
    nan = float("nan")
    # B = 5, level 0.5: the quantiles at 0.25 and 0.75
    stat = np.array([[1.0, 2.0, 3.0, 4.0, 5.0],           # 0.25 -> position 1.0 -> 2, 0.75 -> 4
                     [10.0, nan, 30.0, 20.0, 40.0],       # four usable 10 20 30 40: positions 0.75, 2.25 -> 17.5, 32.5
                     [7.0, nan, nan, nan, 9.0]])          # two usable of five: fewer than B / 2 -> NaN
    with caplog.at_level(logging.WARNING):
        low, high, gl, gh, usable, gu = bootstrap_intervals(stat, 0.5, "ndcg@10 of sensitive attribute age")
    assert low[:2].tolist() == [2.0, 17.5] and high[:2].tolist() == [4.0, 32.5] and math.isnan(low[2]) and math.isnan(high[2])
    assert usable.tolist() == [5, 4, 2] and gu == 2 and math.isnan(gl) and math.isnan(gh)
    warned = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warned) == 1 and "ndcg@10 of sensitive attribute age" in warned[0] and "group 2" in warned[0] and "gap" in warned[0]
    # without the starved group: gaps of the usable replicates 0, 2, 3, 4 are 9, 27, 16, 35 -> sorted 9 16 27 35
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        low, high, gl, gh, usable, gu = bootstrap_intervals(stat[:2], 0.5)
    assert gu == 4 and gl == 9 + 0.75 * 7 and gh == 27 + 0.25 * 8 and not caplog.records


@pytest.mark.parametrize("G", [2, 6])
def test_intervals_against_the_written_out_quantile(G, caplog):
    from fairrec.evaluator import bootstrap_intervals
    rng = np.random.default_rng([G, 3])
    stat = rng.random((G, 200)) + np.arange(G)[:, None] * 0.1
    stat[0, 17] = np.nan
    stat[G - 1, rng.choice(200, 120, replace=False)] = np.nan          # 80 usable of 200: below B / 2
    with caplog.at_level(logging.WARNING):
        got = bootstrap_intervals(stat, 0.95, f"case {G}")
    want = BR.intervals_ref(stat, 0.95)
    assert got[4].tolist() == want[4].tolist() == [199] + [200] * (G - 2) + [80] and got[5] == want[5] < 100
    assert math.isnan(got[0][G - 1]) and math.isnan(got[1][G - 1]) and math.isnan(got[2]) and math.isnan(got[3])
    for a, b in ((got[0], want[0]), (got[1], want[1])):
        assert np.array_equal(np.isnan(a), np.isnan(b))
        assert (np.abs(a - b)[:G - 1] <= 4 * BR.U64 * np.abs(b)[:G - 1]).all()
    assert len([r for r in caplog.records if r.levelno == logging.WARNING]) == 1
    # the gap, once the starved group is left out
    got, want = bootstrap_intervals(stat[:G - 1], 0.9), BR.intervals_ref(stat[:G - 1], 0.9)
    assert got[5] == want[5] == 199
    if G > 2:
        assert abs(got[2] - want[2]) <= 4 * BR.U64 * want[2] and abs(got[3] - want[3]) <= 4 * BR.U64 * want[3]


# ---- refusals: the error code, fr_last_error, nothing written (no GPU: a refused call follows no pointer) -------------------------

def _host(dtype, n, fill):
    a = np.full(n, fill, dtype=dtype)
    return a, a.ctypes.data


def test_workspace_formula_and_its_bound():
    from fairrec import _C
    lib = _C.lib()
    for args in ((1, 1, 1, 1), (65, 3, 4, 7), (322, 8, 5, 257), (BR.LONG_ROWS - 1, 9, 2, 1025), (BR.LONG_ROWS, 64, 70, 65536),
                 (10 ** 6, 8, 64, 1000), (2 ** 31 - 1, 1, 1, 1)):
        assert lib.fr_bootstrap_group_sums_workspace_bytes(*args) == BR.workspace_bytes(*args), args
    assert BR.chunk_len(BR.LONG_ROWS - 1) == 64 and BR.chunk_len(BR.LONG_ROWS) == 128
    # bounded by the chunks, never by n_rows * n_rep: 10^6 rows x 1000 replicates x 8 columns stay below 2049 + G chunks
    assert BR.workspace_bytes(10 ** 6, 8, 2, 1000) <= ((BR.MAX_CHUNKS + 1 + 2) * 1000 * 9 + 3) * 8 < 10 ** 6 * 1000 * 8 // 40
    for args in ((0, 1, 1, 1), (-1, 1, 1, 1), (2 ** 31, 1, 1, 1), (5, 0, 1, 1), (5, 65, 1, 1), (5, 1, 0, 1), (5, 1, -1, 1),
                 (5, 1, 1, 0), (5, 1, 1, 65537), (5, 64, 2 ** 40, 65536)):
        assert lib.fr_bootstrap_group_sums_workspace_bytes(*args) == 0, args


def test_bootstrap_group_sums_refuses_bad_arguments_without_gpu():
    from fairrec import _C
    lib = _C.lib()
    U, C, ld, G, B = 65, 3, 5, 4, 7
    need = lib.fr_bootstrap_group_sums_workspace_bytes(U, C, G, B)
    assert need == BR.workspace_bytes(U, C, G, B) == ((2 + G) * B * (C + 1) + G + 1) * 8
    values, values_p = _host(np.float64, U * ld, 0.0)
    perm, perm_p = _host(np.int64, U, 0)
    start, start_p = _host(np.int64, G + 1, 0)
    sums, sums_p = _host(np.float64, G * B * C, 1234.5)
    weight, weight_p = _host(np.int64, G * B, -77)
    ws, ws_p = _host(np.uint8, need, 0xA5)
    good = [values_p, U, C, ld, perm_p, start_p, G, B, 2020, sums_p, weight_p, ws_p, need]
    for pos, bad in ((0, 0), (5, 0), (9, 0), (10, 0), (11, 0), (1, 0), (1, -1), (1, 2 ** 31), (2, 0), (2, -1), (2, 65), (3, C - 1),
                     (3, 0), (6, 0), (6, -1), (7, 0), (7, -1), (7, 65537), (12, need - 1), (12, 0)):
        args = list(good)
        args[pos] = bad
        rc = lib.fr_bootstrap_group_sums(*args, None)
        assert rc == EINVAL and b"fr_bootstrap_group_sums" in lib.fr_last_error(), (pos, bad, rc)
        assert (sums == 1234.5).all() and (weight == -77).all() and (ws == 0xA5).all()


def test_user_terms_refuse_bad_arguments_without_gpu():
    import ctypes
    from fairrec import _C
    lib = _C.lib()
    U, K, C = 10, 5, 3
    rec, rec_p = _host(np.int32, U * (K + 1), 0)
    out, out_p = _host(np.float64, U * C, 1234.5)

    def arr(*v):
        return (ctypes.c_int32 * len(v))(*v)

    good = [rec_p, U, K, arr(0, 2, 5), arr(1, 5, 3), C, out_p]
    for pos, bad in ((0, 0), (3, None), (4, None), (6, 0), (1, 0), (1, -1), (1, 2 ** 31), (2, 0), (2, -1), (5, 0), (5, -1), (5, 65),
                     (3, arr(0, 6, 5)), (3, arr(-1, 2, 5)), (4, arr(1, 6, 3)), (4, arr(0, 5, 3))):
        args = list(good)
        args[pos] = bad
        rc = lib.fr_topk_user_terms(*args, None)
        assert rc == EINVAL and b"fr_topk_user_terms" in lib.fr_last_error(), (pos, rc)
        assert (out == 1234.5).all()
    mr, mr_p = _host(np.int64, U * 3, 0)
    out2, out2_p = _host(np.float64, U * 2, 1234.5)
    for args in ((0, U, out2_p), (mr_p, U, 0), (mr_p, 0, out2_p), (mr_p, -1, out2_p), (mr_p, 2 ** 31, out2_p)):
        rc = lib.fr_gauc_user_terms(*args, None)
        assert rc == EINVAL and b"fr_gauc_user_terms" in lib.fr_last_error(), args
        assert (out2 == 1234.5).all()


# ---- the config keys ---------------------------------------------------------------------------------------------------------------

def _config(**kw):
    from fairrec.config import Config
    base = {"metrics": ["NDCG", "GAUC"], "topk": [5], "sst_attr_list": ["gender", "age"], "eval_args": {"mode": "full"},
            "device": "cpu"}
    return Config(model="FOCF", config_dict=dict(base, **kw))


def test_group_bootstrap_key_values():
    from fairrec.evaluator import Evaluator
    assert _config()["group_bootstrap"] is None and _config()["group_bootstrap_level"] == 0.95 and _config()["seed"] == 2020
    for value in (None, 0):
        ev = Evaluator(_config(group_bootstrap=value))
        assert ev.bootstrap == 0
        assert Evaluator(_config(group_bootstrap=value, utility_by_group=True)).bootstrap == 0
    ev = Evaluator(_config(group_bootstrap=200, utility_by_group=True))
    assert ev.bootstrap == 200 and ev.bootstrap_level == 0.95 and ev.seed == 2020
    ev = Evaluator(_config(group_bootstrap=65536, group_bootstrap_level=0.5, utility_by_group=["age"], seed=7))
    assert ev.bootstrap == 65536 and ev.bootstrap_level == 0.5 and ev.seed == 7
    with pytest.raises(ValueError, match="group_bootstrap needs utility_by_group"):
        Evaluator(_config(group_bootstrap=200))
    with pytest.raises(ValueError, match="group_bootstrap needs eval_args.mode full / uniN / popN, not 'labeled'"):
        Evaluator(_config(group_bootstrap=200, utility_by_group=True, metrics=["AUC"], eval_args={"mode": "labeled"}))
    for value in (1, -3, 65537, 2.5, "200", True, [200]):
        with pytest.raises(ValueError, match="group_bootstrap must be"):
            Evaluator(_config(group_bootstrap=value, utility_by_group=True))
    for level in (0, 1, 0.0, 1.0, -0.5, 1.5, "0.9", True):
        with pytest.raises(ValueError, match="group_bootstrap_level"):
            Evaluator(_config(group_bootstrap=200, group_bootstrap_level=level, utility_by_group=True))


def test_no_interval_key_without_the_key(monkeypatch):
    """the key unset: `_utility_by_group` asks for no user term and no bootstrap, and reports no ci_ key (the grouped kernels are
    replaced by host stand-ins: this runs without a GPU)"""
    from fairrec.evaluator import Evaluator
    from fairrec.evaluator import metrics as M

    def forbidden(*a, **kw):
        raise AssertionError("the bootstrap path ran with group_bootstrap unset")

    for name in ("topk_user_terms", "gauc_user_terms", "bootstrap_group_sums", "bootstrap_intervals"):
        monkeypatch.setattr(M, name, forbidden)
    monkeypatch.setattr(M, "topk_metrics", lambda rec, topk: {f"{n}@{k}": 0.5 for n in M.TOPK_NAMES for k in topk})
    monkeypatch.setattr(M, "gauc", lambda mr: 0.5)
    monkeypatch.setattr(M, "group_topk_metrics", lambda rec, gidx, G, topk: {f"{n}@{k}": [0.25] * G for n in M.TOPK_NAMES for k in topk})
    monkeypatch.setattr(M, "group_gauc", lambda mr, gidx, G: [0.75] * G)
    collected = {"rec.topk": torch.zeros((6, 6), dtype=torch.int32), "rec.meanrank": torch.zeros((6, 3), dtype=torch.int64),
                 "data.user.gender": torch.tensor([0.0, 1, 0, 1, 0, 1]), "data.user.age": torch.tensor([18, 18, 35, 35, 50, 50])}
    for extra in ({}, {"group_bootstrap": None}, {"group_bootstrap": 0}):
        res = Evaluator(_config(utility_by_group=True, **extra)).evaluate(collected)
        assert "ndcg@5 of gender=1" in res and "gauc gap of sensitive attribute age" in res
        assert not any("ci_" in k for k in res)

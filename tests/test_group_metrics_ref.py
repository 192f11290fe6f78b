"""CPU: the references of tests/group_metrics_ref.py before anything runs on a GPU, and what of `utility_by_group` needs none.

* the per-group top-k reference (metrics_ref.topk_metrics_ref on a group's rows) against oracle/metrics.py on the group's rows,
  to 1e-13 relative as tests/test_metrics_ref.py pins the ungrouped one;
* the exact-rational GAUC sums per group against a float64 restatement of evaluator.gauc's formula, and that restatement
  against fairrec.evaluator.metrics.gauc itself;
* the input condition of the mixed GPU cases: every group with at least ROW_KINDS members has a positive reference in all six
  rows at rank K;
* fr_topk_metrics_grouped / fr_gauc_grouped refuse bad arguments before anything is launched or written (host buffers: a
  refused call never follows a pointer), and the workspace functions return 0 out of range;
* the `utility_by_group` key: its values, the ValueError for a stranger and for a value of another type, the labeled branch of
  the Collector, and the collected keys with the key unset.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import group_metrics_ref as GR
import metrics_ref as R
from oracle import metrics as OM

NAMES = ("hit", "mrr", "ndcg", "recall", "precision", "map")
REL = 1e-13


def _oracle_topk(rec):
    K = rec.shape[1] - 1
    with np.errstate(invalid="ignore", divide="ignore"):
        d = OM.topk_metrics(rec, range(1, K + 1))
    return np.array([[d[f"{n}@{k}"] for k in range(1, K + 1)] for n in NAMES])


def test_group_reference_matches_the_oracle_on_the_groups_rows():
    U, K, G = 200, 20, 5
    rec = R.topk_case(U, K)
    perm, start = GR.segments(GR.assignment(U, G), G)
    ref, sizes = GR.group_topk_ref(rec, perm, start)
    assert sizes.tolist() == [40] * 5 and np.isfinite(ref).all()
    for g in range(G):
        want = _oracle_topk(rec[perm[start[g]:start[g + 1]]])
        assert (np.abs(ref[g] - want) <= REL * np.abs(want)).all(), g
    # the size-weighted mean of the groups is the ungrouped reference
    whole = R.topk_metrics_ref(rec)
    assert (np.abs((ref * sizes[:, None, None]).sum(0) / U - whole) <= REL * whole).all()
    # an empty group is NaN everywhere
    ref, sizes = GR.group_topk_ref(rec, None, np.array([0, 0, U]))
    assert np.isnan(ref[0]).all() and np.isfinite(ref[1]).all() and sizes.tolist() == [0, U]


@pytest.mark.parametrize("G,U", GR.GROUP_COUNTS)
def test_mixed_cases_have_positive_references(G, U):
    rec = R.topk_case(U, GR.GROUP_K)
    gidx = GR.assignment(U, G)
    assert sorted(set(gidx.tolist())) == list(range(G))
    if G > 1 and U // G >= R.ROW_KINDS:
        # not in step with the 8-row cycle: no group is made of one or two row kinds
        assert all(len(set(((np.nonzero(gidx == g)[0] - 1) % R.ROW_KINDS).tolist())) > 2 for g in range(G))
    ref, sizes = GR.group_topk_ref(rec, *GR.segments(gidx, G))
    for g in range(G):
        if sizes[g] >= R.ROW_KINDS:
            assert (ref[g][:, GR.GROUP_K - 1] > 0).all(), (g, ref[g][:, GR.GROUP_K - 1])


def test_chunk_cases_cover_every_size():
    for K in GR.CHUNK_K:
        for shuffled in (False, True):
            rec, perm, start = GR.chunk_case(K, shuffled)
            assert np.diff(start).tolist() == GR.CHUNK_SIZES and rec.shape == (322, K + 1)
            if shuffled:
                assert sorted(perm.tolist()) == list(range(322))
                g_of = np.repeat(np.arange(5), GR.CHUNK_SIZES)
                inv = np.empty(322, dtype=np.int64)
                inv[perm] = g_of
                assert (np.diff(inv) != 0).sum() > 100            # the groups interleave in row order


def test_gauc_restatement_per_group():
    from fairrec.evaluator.metrics import gauc
    U, G = 200, 5
    t = GR.meanrank_case(U)
    t[3] = (0, 30, 0)             # no positive
    t[4] = (20, 4, 4)             # no negative
    perm, start = GR.segments(GR.assignment(U, G), G)
    sums, kept = GR.group_gauc_ref(t, perm, start)
    assert kept.sum() == U and kept[:, 1].sum() == 1 and kept[:, 2].sum() == 1
    for g in range(G):
        rows = perm[start[g]:start[g + 1]]
        want = GR.gauc_float64(t[rows])
        assert abs(sums[g, 0] / sums[g, 1] - want) <= 1e-13 * want
        assert abs(gauc(torch.from_numpy(t[rows])) - want) <= 1e-13 * want
    assert math.isnan(GR.gauc_float64(t[3:5])) and math.isnan(gauc(torch.from_numpy(t[3:5])))


# ---- refusals: the error code, fr_last_error, nothing written (no GPU: a refused call follows no pointer) -----------------------------

EINVAL = -1


def _host(dtype, n, fill):
    a = np.full(n, fill, dtype=dtype)
    return a, a.ctypes.data


def test_topk_metrics_grouped_refuses_bad_arguments_without_gpu():
    from fairrec import _C
    lib = _C.lib()
    U, K, G = 65, 3, 4
    need = lib.fr_topk_metrics_grouped_workspace_bytes(U, K, G)
    assert need == (((U + 63) // 64 + G) * 6 * K + G + 1) * 8
    rec, rec_p = _host(np.int32, U * (K + 1), 0)
    perm, perm_p = _host(np.int64, U, 0)
    start, start_p = _host(np.int64, G + 1, 0)
    out, out_p = _host(np.float64, G * 6 * K, 1234.5)
    ws, ws_p = _host(np.uint8, need, 0xA5)
    good = [rec_p, perm_p, start_p, U, K, G, out_p, ws_p, need]
    for pos, bad in ((0, 0), (2, 0), (6, 0), (7, 0), (3, 0), (3, -1), (4, 0), (4, -1), (5, 0), (5, -1), (8, need - 1), (8, 0)):
        args = list(good)
        args[pos] = bad
        rc = lib.fr_topk_metrics_grouped(*args, None)
        assert rc == EINVAL and b"fr_topk_metrics_grouped" in lib.fr_last_error(), (pos, bad, rc)
        assert (out == 1234.5).all() and (ws == 0xA5).all()
    for args in ((0, K, G), (-1, K, G), (U, 0, G), (U, -1, G), (U, K, 0), (U, K, -1), (U, K, 2 ** 31), (2 ** 40, K, G)):
        assert lib.fr_topk_metrics_grouped_workspace_bytes(*args) == 0, args
    assert lib.fr_topk_metrics_grouped_workspace_bytes(1, 1, 1) == (2 * 6 + 2) * 8


def test_gauc_grouped_refuses_bad_arguments_without_gpu():
    from fairrec import _C
    lib = _C.lib()
    U, G = 65, 4
    need = lib.fr_gauc_grouped_workspace_bytes(U, G)
    assert need == (((U + 63) // 64 + G) * 5 + G + 1) * 8
    mr, mr_p = _host(np.int64, U * 3, 0)
    perm, perm_p = _host(np.int64, U, 0)
    start, start_p = _host(np.int64, G + 1, 0)
    out, out_p = _host(np.float64, G * 2, 1234.5)
    kept, kept_p = _host(np.int64, G * 3, -77)
    ws, ws_p = _host(np.uint8, need, 0xA5)
    good = [mr_p, perm_p, start_p, U, G, out_p, kept_p, ws_p, need]
    for pos, bad in ((0, 0), (2, 0), (5, 0), (6, 0), (7, 0), (3, 0), (3, -1), (4, 0), (4, -1), (8, need - 1), (8, 0)):
        args = list(good)
        args[pos] = bad
        rc = lib.fr_gauc_grouped(*args, None)
        assert rc == EINVAL and b"fr_gauc_grouped" in lib.fr_last_error(), (pos, bad, rc)
        assert (out == 1234.5).all() and (kept == -77).all() and (ws == 0xA5).all()
    for args in ((0, G), (-1, G), (U, 0), (U, -1), (U, 2 ** 31), (2 ** 40, G)):
        assert lib.fr_gauc_grouped_workspace_bytes(*args) == 0, args
    assert ctypes.sizeof(ctypes.c_size_t) == 8


# ---- the config key ------------------------------------------------------------------------------------------------------------------

def _config(**kw):
    from fairrec.config import Config
    base = {"metrics": ["NDCG", "GAUC"], "topk": [5], "sst_attr_list": ["gender", "age"], "eval_args": {"mode": "full"},
            "device": "cpu"}
    return Config(model="FOCF", config_dict=dict(base, **kw))


def test_utility_by_group_key_values():
    from fairrec.evaluator import Collector, Evaluator
    assert _config()["utility_by_group"] is None                                       # the default of overall.yaml: off
    for value, want in ((None, []), (False, []), (True, ["gender", "age"]), (["age"], ["age"]), (["age", "gender"], ["age", "gender"]),
                        ([], [])):
        cfg = _config(utility_by_group=value)
        assert Evaluator(cfg).utility == want and Collector(cfg).utility == want, value
    with pytest.raises(ValueError, match="nope"):
        Evaluator(_config(utility_by_group=["nope"]))
    with pytest.raises(ValueError, match="nope"):
        Evaluator(_config(utility_by_group=["gender", "nope"]))
    for value in ("gender", 3, 1.5, {"gender": True}, [1, 2]):
        with pytest.raises(ValueError, match="utility_by_group"):
            Evaluator(_config(utility_by_group=value))


def test_labeled_collector_keeps_the_attributes_only_with_the_key():
    from fairrec.data.interaction import Interaction
    from fairrec.evaluator import Collector
    inter = Interaction({"label": torch.tensor([1.0, 0.0, 1.0]), "gender": torch.tensor([0.0, 1.0, 1.0]),
                         "age": torch.tensor([18, 35, 18])})
    scores = torch.tensor([0.2, 0.7, 0.9])
    labeled = dict(metrics=["AUC"], eval_args={"mode": "labeled"}, LABEL_FIELD="label")
    off = Collector(_config(**labeled))
    off.eval_batch_collect_labeled(scores, inter)
    assert sorted(off.get_data_struct()) == ["data.label", "rec.score"]
    on = Collector(_config(utility_by_group=True, **labeled))
    on.eval_batch_collect_labeled(scores, inter)
    on.eval_batch_collect_labeled(scores, inter)
    got = on.get_data_struct()
    assert sorted(got) == ["data.age", "data.gender", "data.label", "rec.score"]
    assert got["data.age"].tolist() == [18, 35, 18] * 2 and got["data.gender"].tolist() == [0.0, 1.0, 1.0] * 2
    missing = Collector(_config(utility_by_group=["age"], **labeled))
    with pytest.raises(ValueError, match="age"):
        missing.eval_batch_collect_labeled(scores, Interaction({"label": torch.tensor([1.0, 0.0, 1.0])}))


# ---- where the groups are built (fairrec/evaluator/groups.py): torch index plumbing, no GPU ------------------------------------------

def test_attribute_groups_are_numpys_unique_inverse():
    from fairrec.evaluator.groups import attribute_groups
    rng = np.random.default_rng(11)
    cols = {"gender": rng.integers(0, 2, 300).astype(np.float32),                       # float column, integer values
            "age": rng.choice(np.array([18, 25, 35, 45, 56]), 300),                     # int64 column, gaps between the values
            "score": rng.choice(np.array([0.5, 1.25, -2.0], dtype=np.float32), 300)}    # float column, fractional values
    both = ["age", "score"]
    groups = attribute_groups({n: torch.from_numpy(c) for n, c in cols.items()}, [both])
    assert [g.name for g in groups] == ["gender", "age", "score", "age&score"] and all(g.labels is None for g in groups)
    inverse = {}
    for g in groups[:3]:
        vals, inverse[g.name] = np.unique(cols[g.name], return_inverse=True)
        assert g.index.dtype == torch.int64 and g.index.numpy().tolist() == inverse[g.name].tolist(), g.name
        assert g.n_groups == len(vals)
    tuples, inv = np.unique(np.stack([inverse[n] for n in both], axis=1), axis=0, return_inverse=True)
    assert len(tuples) == 15 and groups[3].n_groups == 15 and groups[3].index.numpy().tolist() == inv.reshape(-1).tolist()
    # the labels, only when asked for: value names, '&'-joined along a tuple, in sorted-tuple order
    named = attribute_groups({n: torch.from_numpy(c) for n, c in cols.items()}, [both], labels=True)
    assert [g.index.tolist() for g in named] == [g.index.tolist() for g in groups]
    assert named[0].labels == ["0", "1"] and named[1].labels == ["18", "25", "35", "45", "56"]
    assert named[2].labels == ["-2", "0.5", "1.25"]
    assert named[3].labels == [f"{a}&{s}" for a in named[1].labels for s in named[2].labels]
    # a 2-D column [rows, 1] groups as its flattened values
    assert attribute_groups({"age": torch.from_numpy(cols["age"])[:, None]})[0].index.tolist() == inverse["age"].tolist()


def test_attribute_groups_refuse_a_single_value():
    from fairrec.evaluator.groups import attribute_groups
    two, one = torch.tensor([0.0, 1.0, 1.0, 0.0]), torch.full((4,), 7.0)
    with pytest.raises(ValueError, match="there is only one value for age sensitive attribute"):
        attribute_groups({"gender": two, "age": one})
    with pytest.raises(ValueError, match="there is only one value for age sensitive attribute"):
        attribute_groups({"gender": two, "age": one}, [["gender", "age"]], labels=True)


def test_group_segments_with_an_empty_group_in_the_middle():
    from fairrec.evaluator.groups import group_segments, item_segments
    gidx = torch.tensor([3, 0, 1, 3, 0, 3, 1, 0, 3], dtype=torch.int32)              # group 2 is empty, 4 groups
    perm, start = group_segments(gidx, 4)
    assert start.dtype == torch.int64 and start.tolist() == [0, 3, 5, 5, 9]            # G + 1 entries, the empty group repeats 5
    assert perm.dtype == torch.int64 and perm.tolist() == [1, 4, 7, 2, 6, 0, 3, 5, 8]  # each group's rows in ascending row order
    want_perm, want_start = GR.segments(gidx.numpy(), 4)
    assert perm.tolist() == want_perm.tolist() and start.tolist() == want_start.tolist()
    none, only_start = group_segments(gidx, 4, perm=False)
    assert none is None and only_start.tolist() == start.tolist()
    K, runs = item_segments(torch.tensor([2, 2, 5, 9, 9, 9]))
    assert K == 3 and runs.dtype == torch.int64 and runs.tolist() == [0, 2, 3, 6]

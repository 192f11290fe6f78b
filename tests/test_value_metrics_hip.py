"""GPU: the value-metric kernels through the C ABI against tests/value_metrics_ref.py -- fr_auc_sorted's integer counts EQUAL to
the Python-int restatement, fr_value_metrics within relative 1e-9 of the fsum reference (the tolerance tests/test_metrics_hip.py
holds the float64 metric reductions to) and bit-reproducible, fr_eval_meanrank_segments' int64 triples EQUAL to the dense
restatement, and the FR_EINVAL cases with the output buffers untouched."""
import logging
import math

import numpy as np
import pytest
import torch

import value_metrics_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [1, 2, 255, 256, 257, 65_537, 1_000_003]


def _auc_device(score, label):
    from fairrec import _C
    lib = _C.lib()
    s = torch.from_numpy(np.asarray(score, dtype=np.float32)).to(DEV)
    y = torch.from_numpy(np.asarray(label, dtype=np.float32)).to(DEV)
    srt, order = torch.sort(s)
    ys = y[order].contiguous()
    n = s.numel()
    out = torch.full((3,), -7, dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.fr_auc_sorted_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    _C.check(lib.fr_auc_sorted(srt.data_ptr(), ys.data_ptr(), n, out.data_ptr(), ws.data_ptr(), ws.numel(), _C.current_stream()),
             "fr_auc_sorted")
    return tuple(out.cpu().tolist())


def _scores(rng, n, kind):
    s = rng.random(n).astype(np.float32)
    if kind == "q2":
        s = (np.floor(s * 2) / 2).astype(np.float32)
    elif kind == "q64":
        s = (np.floor(s * 64) / 64).astype(np.float32)
    elif kind == "one":
        s = np.full(n, 0.25, dtype=np.float32)
    return s


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["continuous", "q2", "q64", "one"])
def test_auc_sorted_counts_equal_the_restatement(n, kind):
    rng = np.random.default_rng(n * 7 + len(kind))
    score = _scores(rng, n, kind)
    label = (rng.random(n) < 0.2 + 0.5 * score).astype(np.float32)
    got, want = _auc_device(score, label), R.auc_exact(score, label)
    print(f"n={n} {kind}: device {got} reference {want}")
    assert got == want


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("labels", ["no_positive", "no_negative", "other_values"])
def test_auc_sorted_degenerate_labels(n, labels):
    rng = np.random.default_rng(n)
    score = _scores(rng, n, "q64" if n % 2 else "continuous")
    if labels == "no_positive":
        label = np.zeros(n, dtype=np.float32)
    elif labels == "no_negative":
        label = np.ones(n, dtype=np.float32)
    else:                                   # ratings 0 .. 5 and a half: only == 1 is a positive
        label = rng.choice(np.array([0, 0.5, 1, 2, 5], dtype=np.float32), n)
    got, want = _auc_device(score, label), R.auc_exact(score, label)
    print(f"n={n} {labels}: device {got} reference {want}")
    assert got == want
    if labels == "no_positive":
        assert got == (0, 0, n)
    if labels == "no_negative":
        assert got == (0, n, 0)


def _value_device(score, label):
    from fairrec import _C
    lib = _C.lib()
    s = torch.from_numpy(np.asarray(score, dtype=np.float32)).to(DEV)
    y = torch.from_numpy(np.asarray(label, dtype=np.float32)).to(DEV)
    n = s.numel()
    out = torch.empty(3, dtype=torch.float64, device=DEV)
    counts = torch.empty(2, dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.fr_value_metrics_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    _C.check(lib.fr_value_metrics(s.data_ptr(), y.data_ptr(), n, out.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
                                  _C.current_stream()), "fr_value_metrics")
    return out.cpu(), counts.cpu().tolist()


@pytest.mark.parametrize("n", SIZES + [3_000_000])
@pytest.mark.parametrize("labels", ["binary", "rating"])
def test_value_metrics_against_fsum(n, labels):
    rng = np.random.default_rng(n + len(labels))
    score = rng.random(n).astype(np.float32)
    score[rng.random(n) < 0.05] = 0.0                        # the clip, both ends
    score[rng.random(n) < 0.05] = 1.0
    if n >= 2:
        score[0], score[1] = 0.0, 1.0
    label = (rng.random(n) < 0.4).astype(np.float32) if labels == "binary" else rng.integers(0, 6, n).astype(np.float32)
    got, counts = _value_device(score, label)
    again, counts2 = _value_device(score, label)
    assert got.numpy().tobytes() == again.numpy().tobytes() and counts == counts2         # the same bits on every call
    want = R.sums(score, label)
    print(f"n={n} {labels}: device {got.tolist()} reference {want}")
    assert counts == [n, int((label == 1).sum())]
    for g, w in zip(got.tolist(), want):
        assert abs(g - w) <= 1e-9 * abs(w), (g, w)


def test_value_metrics_python_entry(caplog):
    from fairrec.evaluator.metrics import value_metrics
    rng = np.random.default_rng(11)
    n = 50_001
    score = (np.floor(rng.random(n) * 512) / 512).astype(np.float32)
    label = (rng.random(n) < score).astype(np.float32)
    names = ["rmse", "auc", "logloss", "mae"]
    got = value_metrics(torch.from_numpy(score).to(DEV), torch.from_numpy(label).to(DEV), names)
    want = R.value_metrics(score, label, names)
    assert list(got) == names
    for m in names:
        print(m, got[m], want[m])
        assert abs(got[m] - want[m]) <= 1e-9 * abs(want[m]), m
    two_u, P, Nn = R.auc_exact(score, label)
    assert got["auc"] == two_u / (2 * P * Nn)                 # exact integers, one float64 division
    with caplog.at_level(logging.WARNING):
        res = value_metrics(torch.from_numpy(score).to(DEV), torch.zeros(n, device=DEV), ["auc", "mae"])
    assert math.isnan(res["auc"]) and "positive" in caplog.text and np.isfinite(res["mae"])


# ---- fr_eval_meanrank_segments -----------------------------------------------------------------------------------------
def _meanrank_device(seg, items, scores, pos_rows, n_items):
    """pos_rows: the row numbers of the positives; the entry takes them as the sorted keys user row * n_items + item."""
    from fairrec import _C
    lib = _C.lib()
    seg = np.asarray(seg, dtype=np.int64)
    pos_rows = np.asarray(pos_rows, dtype=np.int64)
    owner = np.searchsorted(seg, pos_rows, side="right") - 1
    pos_item = pos_rows - seg[owner] if items is None else np.asarray(items)[pos_rows]
    seg_t = torch.from_numpy(seg).to(DEV)
    sc = torch.as_tensor(np.asarray(scores, dtype=np.float32)).to(DEV)
    it = None if items is None else torch.as_tensor(np.asarray(items, dtype=np.int64)).to(DEV)
    keys = torch.from_numpy(np.sort(owner * n_items + pos_item)).to(DEV)
    U, n_rows = len(seg) - 1, sc.numel()
    out = torch.full((U, 3), -7, dtype=torch.int64, device=DEV)
    ws = None if it is None else torch.empty(lib.fr_eval_meanrank_workspace_bytes(n_rows), dtype=torch.uint8, device=DEV)
    _C.check(lib.fr_eval_meanrank_segments(seg_t.data_ptr(), U, _C.ptr(it), sc.data_ptr(), keys.data_ptr(), keys.numel(), n_items,
                                           n_rows, out.data_ptr(), _C.ptr(ws), 0 if ws is None else ws.numel(),
                                           _C.current_stream()), "fr_eval_meanrank_segments")
    return out.cpu().numpy()


def _candidate_batch(seed, U=200, n_items=400):
    """Users with 1 .. 5 positives (some listed twice) followed by 20 negatives per positive drawn with replacement; a third of the
    users score on 6 levels (exact ties between positives and negatives); user 3 has one candidate, user 4 only positives, user 5
    none at all, user 6 a long segment (several chunks of 64 with repeats across them)."""
    rng = np.random.default_rng(seed)
    seg, items, scores, pos_rows = [0], [], [], []
    for u in range(U):
        n_pos = int(rng.integers(1, 6))
        pos = rng.choice(np.arange(1, n_items), n_pos, replace=False)
        if u % 5 == 0:
            pos = np.append(pos, pos[0])                       # the same (user, item) twice in the evaluation set
        n_neg = 20 * len(pos)
        if u == 3:
            pos, n_neg = pos[:1], 0
        if u == 4:
            n_neg = 0
        if u == 5:
            pos, n_neg = pos[:0], 0
        if u == 6:
            n_neg = 700
        rest = np.setdiff1d(np.arange(1, n_items), pos)
        neg = rng.choice(rest, n_neg, replace=True) if n_neg else np.zeros(0, dtype=np.int64)
        its = np.concatenate([pos, neg]).astype(np.int64)
        table = rng.random(n_items).astype(np.float32)         # one score per item: copies agree
        if u % 3 == 0:
            table = (np.floor(table * 6) / 6).astype(np.float32)
        base = seg[-1]
        pos_rows += list(range(base, base + len(pos)))
        items += its.tolist()
        scores += table[its].tolist()
        seg.append(base + len(its))
    return seg, np.array(items, dtype=np.int64), np.array(scores, dtype=np.float32), pos_rows, n_items


@pytest.mark.parametrize("seed", [0, 1])
def test_meanrank_segments_equal_the_dense_restatement(seed):
    seg, items, scores, pos_rows, n_items = _candidate_batch(seed)
    got = _meanrank_device(seg, items, scores, pos_rows, n_items)
    dense, mask = R.dense_rows(seg, items, scores, pos_rows, n_items)
    want = np.array([R.meanrank(dense[u], mask[u]) for u in range(len(seg) - 1)], dtype=np.int64)
    np.testing.assert_array_equal(got, want)
    assert got[3].tolist() == [2, 1, 1] and got[4][1] == got[4][2] and got[5].tolist() == [0, 0, 0]
    assert any(len(set(items[seg[u]:seg[u + 1]].tolist())) < seg[u + 1] - seg[u] for u in range(len(seg) - 1))
    from fairrec.evaluator.metrics import gauc
    g, w = gauc(torch.from_numpy(got)), R.gauc(want)
    print("gauc", g, w)
    assert abs(g - w) <= 1e-9 * abs(w)


def test_meanrank_dense_rows_with_masked_history():
    """`full` mode: items == NULL, a row per user of the masked score matrix (column 0 and the history -inf)."""
    rng = np.random.default_rng(4)
    U, n_items = 37, 333
    dense = rng.random((U, n_items)).astype(np.float32)
    dense[::2] = np.floor(dense[::2] * 10) / 10                 # ties
    dense[:, 0] = -np.inf
    mask = np.zeros((U, n_items), dtype=bool)
    for u in range(U):
        free = np.arange(1, n_items)
        hist = rng.choice(free, int(rng.integers(0, 100)), replace=False)
        dense[u, hist] = -np.inf
        cand = np.setdiff1d(free, hist)
        mask[u, rng.choice(cand, int(rng.integers(0, 9)), replace=False)] = True
    seg = np.arange(U + 1) * n_items
    got = _meanrank_device(seg, None, dense.reshape(-1), np.flatnonzero(mask.reshape(-1)), n_items)
    want = np.array([R.meanrank(dense[u], mask[u]) for u in range(U)], dtype=np.int64)
    np.testing.assert_array_equal(got, want)


def test_collector_general_form_matches_the_kernel():
    """The general (ungrouped or K > 62) fallback of eval_batch_collect_candidates computes the triple with index arithmetic:
    the same integers as the kernel path on the same batch."""
    from fairrec.config import Config
    from fairrec.data.interaction import Interaction
    from fairrec.evaluator import Collector
    seg, items, scores, pos_rows, n_items = _candidate_batch(7, U=60)
    keep = [u for u in range(60) if u != 5]                    # (the collector's batches have no user without positives)
    rows = np.concatenate([np.arange(seg[u], seg[u + 1]) for u in keep])
    row_idx = np.concatenate([np.full(seg[u + 1] - seg[u], r) for r, u in enumerate(keep)])
    is_pos = np.zeros(len(items), dtype=bool)
    is_pos[pos_rows] = True
    d = lambda a: torch.as_tensor(a).to(DEV)
    outs = []
    for K in (10, 70):
        cfg = Config(config_dict={"metrics": ["GAUC", "NDCG"], "topk": [K], "eval_args": {"mode": "uni20"}, "device": DEV})
        col = Collector(cfg)
        inter = Interaction({"item_id": d(items[rows])})
        col.eval_batch_collect_candidates(d(scores[rows]), d(row_idx), inter, d(row_idx[is_pos[rows]]),
                                          d(items[rows][is_pos[rows]]), n_items)
        outs.append(col.get_data_struct()["rec.meanrank"].cpu().numpy())
    dense, mask = R.dense_rows(seg, items, scores, pos_rows, n_items)
    want = np.array([R.meanrank(dense[u], mask[u]) for u in keep], dtype=np.int64)
    np.testing.assert_array_equal(outs[0], want)
    np.testing.assert_array_equal(outs[1], want)


# ---- FR_EINVAL: nothing launched, nothing written ----------------------------------------------------------------------
def test_bad_arguments_leave_the_outputs_untouched():
    from fairrec import _C
    lib = _C.lib()
    n = 1000
    s = torch.rand(n, device=DEV)
    y = (torch.rand(n, device=DEV) < 0.5).float()
    out_d = torch.full((3,), -7.0, dtype=torch.float64, device=DEV)
    out_i = torch.full((3,), -7, dtype=torch.int64, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    st = _C.current_stream()
    p = lambda t: t.data_ptr()
    need_v, need_a = lib.fr_value_metrics_workspace_bytes(n), lib.fr_auc_sorted_workspace_bytes(n)
    for args in [(0, p(y), n, p(out_d), p(out_i), p(ws), ws.numel()), (p(s), 0, n, p(out_d), p(out_i), p(ws), ws.numel()),
                 (p(s), p(y), n, 0, p(out_i), p(ws), ws.numel()), (p(s), p(y), n, p(out_d), 0, p(ws), ws.numel()),
                 (p(s), p(y), n, p(out_d), p(out_i), 0, ws.numel()), (p(s), p(y), -5, p(out_d), p(out_i), p(ws), ws.numel()),
                 (p(s), p(y), 0, p(out_d), p(out_i), p(ws), ws.numel()), (p(s), p(y), 2 ** 31, p(out_d), p(out_i), p(ws), ws.numel()),
                 (p(s), p(y), n, p(out_d), p(out_i), p(ws), need_v - 1)]:
        assert lib.fr_value_metrics(*args, st) == -1
    for args in [(0, p(y), n, p(out_i), p(ws), ws.numel()), (p(s), 0, n, p(out_i), p(ws), ws.numel()),
                 (p(s), p(y), n, 0, p(ws), ws.numel()), (p(s), p(y), n, p(out_i), 0, ws.numel()),
                 (p(s), p(y), 0, p(out_i), p(ws), ws.numel()), (p(s), p(y), 2 ** 31, p(out_i), p(ws), ws.numel()),
                 (p(s), p(y), n, p(out_i), p(ws), need_a - 1)]:
        assert lib.fr_auc_sorted(*args, st) == -1
    seg = torch.tensor([0, 600, n], dtype=torch.int64, device=DEV)
    items = torch.randint(1, 50, (n,), device=DEV)
    keys = torch.tensor([int(items[0]), 50 + int(items[600])], dtype=torch.int64, device=DEV)
    for args in [(0, 2, p(items), p(s), p(keys), 2, 50, n, p(out_i), p(ws), ws.numel()),
                 (p(seg), 2, p(items), 0, p(keys), 2, 50, n, p(out_i), p(ws), ws.numel()),
                 (p(seg), 2, p(items), p(s), 0, 2, 50, n, p(out_i), p(ws), ws.numel()),
                 (p(seg), 2, p(items), p(s), p(keys), 2, 50, n, 0, p(ws), ws.numel()),
                 (p(seg), 0, p(items), p(s), p(keys), 2, 50, n, p(out_i), p(ws), ws.numel()),
                 (p(seg), 2, p(items), p(s), p(keys), -1, 50, n, p(out_i), p(ws), ws.numel()),
                 (p(seg), 2, p(items), p(s), p(keys), 2, 0, n, p(out_i), p(ws), ws.numel()),
                 (p(seg), 2, p(items), p(s), p(keys), 2, 50, 0, p(out_i), p(ws), ws.numel()),
                 (p(seg), 2, p(items), p(s), p(keys), 2, 50, n, p(out_i), 0, 0),
                 (p(seg), 2, p(items), p(s), p(keys), 2, 50, n, p(out_i), p(ws), n - 1)]:
        assert lib.fr_eval_meanrank_segments(*args, st) == -1
    torch.cuda.synchronize()
    assert out_d.cpu().tolist() == [-7.0] * 3 and out_i.cpu().tolist() == [-7] * 3 and int(ws.sum()) == 0

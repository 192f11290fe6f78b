"""CPU: the recommendation kernels' contract without a GPU -- the numpy restatement of their total order against torch.topk
and hand-written rows, the argument checks of both entries (before any launch, outputs untouched), and the history CSR
that utils/case_study.py hands to the fused kernel."""
import ctypes

import numpy as np
import pytest
import torch

import recommend_ref as R
from fairrec import _C
from fairrec.utils.case_study import history_csr


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(1, 1), (64, 10), (1000, 50), (5001, 256)])
def test_restatement_equals_torch_topk_on_tie_free_rows(n, k):
    g = torch.Generator().manual_seed(n)
    s = torch.stack([(torch.randperm(n, generator=g).float() - n // 2) / 8 for _ in range(7)])     # distinct by construction
    assert all(len(torch.unique(r)) == n for r in s)
    tv, ti = torch.topk(s, k, dim=1)
    rv, ri = R.topk(s.numpy(), k)
    np.testing.assert_array_equal(ri, ti.numpy())
    assert R.same_bits(rv, tv.numpy())


def test_restatement_on_tied_nan_and_inf_rows():
    inf, nan = np.inf, np.nan
    rows = np.array([
        [1.0, 3.0, 3.0, 2.0, 3.0, 0.0],                     # ties: the lower id first
        [nan, 5.0, inf, nan, -inf, inf],                    # NaN above +inf, NaNs tie, +inf ties
        [-inf, -inf, -inf, 1.0, -inf, -inf],                # fewer finite cells than k: -inf in ascending id
        [0.0, -0.0, 0.0, -1.0, -0.0, 1.0],                  # the two zeros tie
        [2.0, 2.0, 2.0, 2.0, 2.0, 2.0],                     # constant
    ], dtype=np.float32)
    want = [[1, 2, 4, 3], [0, 3, 2, 5], [3, 0, 1, 2], [5, 0, 1, 2], [0, 1, 2, 3]]
    rv, ri = R.topk(rows, 4)
    np.testing.assert_array_equal(ri, np.array(want))
    assert R.same_bits(rv, np.take_along_axis(rows, np.array(want), 1))
    assert list(R.order(rows[1])) == [0, 3, 2, 5, 1, 4]


def test_tau_bounds_a_float32_dot_in_any_order():
    rng = np.random.default_rng(0)
    X = rng.standard_normal((8, 256)).astype(np.float32)
    W = rng.standard_normal((100, 256)).astype(np.float32)
    s64, tau = R.scores64(X, W)
    fwd = np.zeros((8, 100), np.float32)
    for d in range(256):
        fwd = fwd + X[:, d:d + 1] * W[:, d][None, :]        # one rounding per product and per sum: within the bound as well
    assert np.all(np.abs((X @ W.T).astype(np.float64) - s64) <= tau)
    assert np.all(np.abs(fwd.astype(np.float64) - s64) <= 2 * tau)


# ---- argument checks ---------------------------------------------------------------------------------------------------
def _args(**over):
    X = np.zeros((4, 8), np.float32)
    W = np.zeros((100, 8), np.float32)
    indptr = np.zeros(5, np.int64)
    items = np.zeros(1, np.int64)
    keep = (X, W, indptr, items)
    f = dict(X=X.ctypes.data, W=W.ctypes.data, user_bias=None, item_bias=None, hist_indptr=indptr.ctypes.data,
             hist_items=items.ctypes.data, scores_out=None, n_users=4, n_items=100, hist_len=0, dim=8, k=10, epilogue=0,
             mask_pad=1, hist_sorted=1, slices=0, bias0=0.0, scale=1.0)
    f.update(over)
    return _C.FrRecArgs(**f), keep


SENTINEL = 12345


def _outputs(n):
    return np.full(n, SENTINEL, np.float32), np.full(n, SENTINEL, np.int64)


@pytest.mark.parametrize("over,word", [
    (dict(k=0), b"k 0"), (dict(k=257), b"k 257"), (dict(k=101), b"k 101"), (dict(dim=257), b"dim 257"), (dict(dim=0), b"dim 0"),
    (dict(X=None), b"null X or W"), (dict(W=None), b"null X or W"), (dict(hist_sorted=0), b"ascending"),
    (dict(epilogue=3), b"epilogue"), (dict(epilogue=1, scale=0.0), b"scale"), (dict(slices=65), b"slice"),
])
def test_recommend_topk_refuses_before_any_launch(over, word):
    lib = _C.lib()
    a, keep = _args(**over)
    val, idx = _outputs(4 * 10)
    ws = np.full(4 * 64 * 10, SENTINEL, np.int64)
    rc = lib.fr_recommend_topk(ctypes.byref(a), val.ctypes.data, idx.ctypes.data, ws.ctypes.data, ws.nbytes, None)
    assert rc == -1 and word in lib.fr_last_error(), lib.fr_last_error()
    assert (val == SENTINEL).all() and (idx == SENTINEL).all() and (ws == SENTINEL).all()
    if "slices" not in over:
        assert lib.fr_recommend_topk_workspace_bytes(ctypes.byref(a)) == 0


def test_recommend_topk_refuses_a_short_workspace_and_null_outputs():
    lib = _C.lib()
    a, keep = _args(n_items=1000, slices=2)
    need = lib.fr_recommend_topk_workspace_bytes(ctypes.byref(a))
    assert need == 4 * 2 * 10 * 8
    val, idx = _outputs(4 * 10)
    ws = np.full(need // 8, SENTINEL, np.int64)
    assert lib.fr_recommend_topk(ctypes.byref(a), val.ctypes.data, idx.ctypes.data, ws.ctypes.data, need - 8, None) == -1
    assert b"workspace" in lib.fr_last_error()
    assert lib.fr_recommend_topk(ctypes.byref(a), val.ctypes.data, idx.ctypes.data, None, 0, None) == -1
    assert lib.fr_recommend_topk(ctypes.byref(a), None, idx.ctypes.data, ws.ctypes.data, need, None) == -1
    assert lib.fr_recommend_topk(None, val.ctypes.data, idx.ctypes.data, ws.ctypes.data, need, None) == -1
    assert (val == SENTINEL).all() and (idx == SENTINEL).all() and (ws == SENTINEL).all()


def test_topk_rows_refuses_before_any_launch():
    lib = _C.lib()
    s = np.zeros((3, 50), np.float32)
    val, idx = _outputs(3 * 10)
    need = lib.fr_topk_rows_workspace_bytes(3, 50, 10, 0)
    assert need == 3 * 1 * 10 * 8                           # 50 columns: one slice
    ws = np.full(need // 8, SENTINEL, np.int64)
    good = dict(scores=s.ctypes.data, n_rows=3, n_cols=50, ld=50, k=10, slices=0, val=val.ctypes.data, idx=idx.ctypes.data,
                ws=ws.ctypes.data, ws_bytes=need)
    for over in (dict(k=0), dict(k=51), dict(n_cols=1000, ld=1000, k=257), dict(scores=None), dict(val=None), dict(idx=None),
                 dict(ld=49), dict(ws_bytes=need - 1), dict(ws=None), dict(slices=-1), dict(slices=65), dict(n_cols=0)):
        c = dict(good, **over)
        rc = lib.fr_topk_rows(c["scores"], c["n_rows"], c["n_cols"], c["ld"], c["k"], c["slices"], c["val"], c["idx"], c["ws"],
                              c["ws_bytes"], None)
        assert rc == -1 and lib.fr_last_error(), over
        assert (val == SENTINEL).all() and (idx == SENTINEL).all() and (ws == SENTINEL).all(), over
    assert lib.fr_topk_rows_workspace_bytes(3, 50, 0, 0) == 0 and lib.fr_topk_rows_workspace_bytes(3, 50, 257, 0) == 0
    assert _C.FR_TOPK_MAX == 256


def test_workspace_does_not_grow_with_users_times_items():
    lib = _C.lib()
    a, keep = _args(n_users=4096, n_items=200001, dim=64, k=10, hist_indptr=None, hist_items=None)
    ws = lib.fr_recommend_topk_workspace_bytes(ctypes.byref(a))
    assert 0 < ws + 4096 * 10 * 12 < 4096 * 200001 * 4 // 16


# ---- the CSR case_study builds -----------------------------------------------------------------------------------------
def test_history_csr_of_a_user_list_with_repeats():
    rng = np.random.default_rng(1)
    n_users, n_items = 30, 200
    rows = [rng.permutation(np.arange(1, n_items))[:rng.integers(0, 40)] for _ in range(n_users)]      # unsorted within a user
    rows[3] = np.zeros(0, np.int64)
    indptr = np.zeros(n_users + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    items = np.concatenate(rows).astype(np.int64)
    for uids in ([5, 3, 5, 29, 0, 5], [], list(range(n_users)), [3, 3]):
        ip, it = history_csr(torch.from_numpy(indptr), torch.from_numpy(items), torch.tensor(uids, dtype=torch.int64), n_items)
        rip, rit = R.history_csr(indptr, items, uids)
        np.testing.assert_array_equal(ip.numpy(), rip)
        np.testing.assert_array_equal(it.numpy(), rit)
        for j in range(len(uids)):
            assert np.all(np.diff(it.numpy()[rip[j]:rip[j + 1]]) > 0)

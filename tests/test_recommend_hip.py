"""GPU: the recommendation kernels (csrc/recommend.hip) against the numpy restatement in tests/recommend_ref.py.

1. fr_topk_rows equals the restatement in values (bits) and indices on continuous, few-level, constant, NaN-bearing and
   mostly -inf data, at the column counts around the wave / step edges and with ld > n_cols.
2. fr_recommend_topk on integer data, where every dot product is exact in fp32 in any order, equals the restatement exactly:
   every epilogue, biases, the pad mask, histories (one user keeps fewer than k items), an asymmetric W.
3. fr_recommend_topk on real data: the float64 band rules, exact selection against its own scores_out, and the same lists
   for two forced slice counts.
4. The memory the fused call touches does not grow with users * items."""
import numpy as np
import pytest
import torch

import recommend_ref as R
from fairrec import _C
from fairrec.functional import recommend_topk, topk_rows

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- 1. fr_topk_rows ---------------------------------------------------------------------------------------------------
def _rows_data(kind, rows, n, rng):
    if kind == "continuous":
        return rng.standard_normal((rows, n)).astype(np.float32)
    if kind == "levels2":
        return rng.integers(0, 2, (rows, n)).astype(np.float32)
    if kind == "levels64":
        return (rng.integers(0, 64, (rows, n)) / 8.0 - 3.0).astype(np.float32)
    if kind == "constant":
        return np.full((rows, n), 0.25, np.float32)
    if kind == "nan":
        s = rng.standard_normal((rows, n)).astype(np.float32)
        s[rng.random((rows, n)) < 0.02] = np.nan
        s[0, :] = np.nan
        s[rng.random((rows, n)) < 0.01] = np.inf
        s[rng.random((rows, n)) < 0.01] = -0.0
        s[rng.random((rows, n)) < 0.01] = 0.0
        return s
    if kind == "mostly_neg_inf":
        s = np.full((rows, n), -np.inf, np.float32)
        keep = rng.random((rows, n)) < 0.003
        s[keep] = rng.standard_normal(int(keep.sum())).astype(np.float32)
        s[-1, :] = -np.inf
        return s
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["continuous", "levels2", "levels64", "constant", "nan", "mostly_neg_inf"])
@pytest.mark.parametrize("n_cols", [1, 63, 64, 65, 5001, 100001])
def test_topk_rows_equals_the_restatement(kind, n_cols):
    rng = np.random.default_rng(n_cols)
    rows = 5 if n_cols > 5001 else 37
    s = _rows_data(kind, rows, n_cols, rng)
    wide = torch.full((rows, n_cols + 3), 7e9, dtype=torch.float32, device=DEV)        # ld > n_cols: the padding must not be read
    wide[:, :n_cols] = torch.from_numpy(s).to(DEV)
    for k in (1, 10, 50, 256):
        if k > n_cols:
            continue
        val, idx = topk_rows(wide[:, :n_cols], k)
        rv, ri = R.topk(s, k)
        np.testing.assert_array_equal(idx.cpu().numpy(), ri, err_msg=f"k={k}")
        assert R.same_bits(val.cpu().numpy(), rv), f"k={k}"


def test_topk_rows_does_not_depend_on_the_slices():
    rng = np.random.default_rng(3)
    s = _rows_data("levels64", 3, 100001, rng)
    d = torch.from_numpy(s).to(DEV)
    rv, ri = R.topk(s, 50)
    for slices in (1, 3, 16):
        val, idx = topk_rows(d, 50, slices=slices)
        np.testing.assert_array_equal(idx.cpu().numpy(), ri)
        assert R.same_bits(val.cpu().numpy(), rv)


# ---- 2. fused, exact arithmetic ----------------------------------------------------------------------------------------
U2, N2, D2 = 64, 5001, 64


def _int_data(seed=11):
    rng = np.random.default_rng(seed)
    X = rng.integers(-4, 5, (U2, D2)).astype(np.float32)
    W = rng.integers(-4, 5, (N2, D2)).astype(np.float32)
    return rng, X, W


def _histories(rng, U, N, leave3_user=None):
    rows = []
    for u in range(U):
        n = int(rng.integers(0, 200))
        rows.append(np.sort(rng.choice(np.arange(1, N), n, replace=False)))
    if leave3_user is not None:
        keep = rng.choice(np.arange(1, N), 3, replace=False)
        rows[leave3_user] = np.setdiff1d(np.arange(1, N), keep)            # the pad is masked too: 3 items left
    indptr = np.zeros(U + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, np.concatenate(rows).astype(np.int64)


def _fused(X, W, k, **kw):
    t = {}
    for name in ("user_bias", "item_bias", "hist_indptr", "hist_items"):
        if kw.get(name) is not None:
            t[name] = torch.from_numpy(np.asarray(kw.pop(name))).to(DEV)
    out = recommend_topk(torch.from_numpy(X).to(DEV), torch.from_numpy(W).to(DEV), k, **t, **kw)
    return [o.cpu().numpy() for o in out]


def _exact_scores(X, W, ub=None, ib=None, b0=0.0, epilogue=0, scale=1.0):
    """fp32 scores of exactly representable data: the float64 sums are exact, so is their cast."""
    s = X.astype(np.float64) @ W.astype(np.float64).T
    if ub is not None:
        s = s + ub[:, None]
    if ib is not None:
        s = s + ib[None, :]
    s = (s + b0).astype(np.float32)
    if epilogue == 1:
        s = (np.clip(s, np.float32(0), np.float32(scale)) / np.float32(scale)).astype(np.float32)
    return s


@pytest.mark.parametrize("case", ["plain", "clamp5", "biases", "pad", "history", "asymmetric"])
@pytest.mark.parametrize("k", [10, 50])
def test_fused_exact_on_integer_data(case, k):
    rng, X, W = _int_data()
    kw, ref_kw, mask_kw = {}, {}, dict(mask_pad=False)
    if case == "clamp5":
        kw = dict(epilogue=1, scale=5.0)
        ref_kw = dict(epilogue=1, scale=5.0)
    if case == "biases":
        ub = rng.integers(-3, 4, U2).astype(np.float32)
        ib = rng.integers(-3, 4, N2).astype(np.float32)
        kw = dict(user_bias=ub, item_bias=ib, bias0=2.0)
        ref_kw = dict(ub=ub, ib=ib, b0=2.0)
    if case == "pad":
        W[0] = 4.0 * np.sign(X[0])                       # the pad item would be user 0's best
        kw = dict(mask_pad=True)
        mask_kw = dict(mask_pad=True)
    if case == "history":
        indptr, items = _histories(rng, U2, N2, leave3_user=5)
        kw = dict(mask_pad=True, hist_indptr=indptr, hist_items=items)
        mask_kw = dict(mask_pad=True, indptr=indptr, items=items)
    if case == "asymmetric":
        W = (np.arange(N2)[:, None] % 7 - 3 + 2 * (np.arange(D2)[None, :] % 3)).astype(np.float32)     # W[i, d] != W[d, i]
        X = np.eye(U2, D2, dtype=np.float32) * 2 + np.float32(1) * (np.arange(D2)[None, :] == 63)
    s = R.mask(_exact_scores(X, W, **ref_kw), **mask_kw)
    if case == "plain":
        assert np.abs(s).max() <= 1024 and min(len(np.unique(r)) for r in s) < N2 // 4       # exact, and full of ties
    val, idx, dense = _fused(X, W, k, want_scores=True, **kw)
    assert R.same_bits(dense, s)
    rv, ri = R.topk(s, k)
    np.testing.assert_array_equal(idx, ri)
    assert R.same_bits(val, rv)
    val2, idx2 = _fused(X, W, k, **kw)                   # and without the dense output
    np.testing.assert_array_equal(idx2, ri)
    assert R.same_bits(val2, rv)
    if case == "history":
        assert np.isinf(rv[5, 3:]).all() and np.all(np.diff(ri[5, 3:]) > 0)       # -inf entries in ascending id


def test_fused_sigmoid_ranks_like_the_raw_scores():
    rng, X, W = _int_data()
    Xs = (X / 64.0).astype(np.float32)                   # exact scaling: the dots stay exact
    v0, i0 = _fused(Xs, W, 50)
    # the sigmoid of distinct fp32 scores may round to equal values: compare through the restatement on the kernel's own scores
    v2, i2, dense = _fused(Xs, W, 50, epilogue=2, want_scores=True)
    s64, tau = R.scores64(Xs, W, epilogue=2)
    assert np.all(np.abs(dense.astype(np.float64) - s64) <= tau)
    assert np.all(np.abs(v2.astype(np.float64) - np.take_along_axis(s64, i2, 1)) <= np.take_along_axis(tau, i2, 1))
    rv, ri = R.topk(dense, 50)
    np.testing.assert_array_equal(i2, ri)
    assert R.same_bits(v2, rv)
    raw = _exact_scores(Xs, W)
    tied = np.take_along_axis(raw, i0, 1) != np.take_along_axis(raw, i2, 1)
    assert not tied.any(), "epilogue 2 ranks other raw scores than epilogue 0"
    np.testing.assert_array_equal(i0, i2)


# ---- 3. fused, real data -----------------------------------------------------------------------------------------------
U3, N3 = 256, 20001


@pytest.mark.parametrize("D", [1, 48, 64, 128, 256])
def test_fused_real_data(D):
    rng = np.random.default_rng(7)
    X = (0.1 * rng.standard_normal((U3, D))).astype(np.float32)
    W = (0.1 * rng.standard_normal((N3, D))).astype(np.float32)
    indptr, items = _histories(rng, U3, N3)
    s64, tau = R.scores64(X, W)
    s64 = R.mask(s64, True, indptr, items)
    for k in (10, 50, 256):
        val, idx, dense = _fused(X, W, k, mask_pad=True, hist_indptr=indptr, hist_items=items, want_scores=True)
        assert np.array_equal(np.isneginf(dense), np.isneginf(s64))
        worst = R.check_band(val, idx, s64, tau, k)
        print(f"D={D} k={k}: at most {worst} items of a user within 2 tau of its k-th best")
        rv, ri = R.topk(dense, k)
        np.testing.assert_array_equal(idx, ri)
        assert R.same_bits(val, rv)
        for slices in (1, 7):
            v, i = _fused(X, W, k, mask_pad=True, hist_indptr=indptr, hist_items=items, slices=slices)
            np.testing.assert_array_equal(i, ri, err_msg=f"slices={slices}")
            assert R.same_bits(v, rv)


@pytest.mark.parametrize("epilogue", [1, 2])
def test_fused_real_data_epilogues(epilogue):
    rng = np.random.default_rng(7)
    D, k = 48, 50
    X = (0.1 * rng.standard_normal((U3, D))).astype(np.float32)
    W = (0.1 * rng.standard_normal((N3, D))).astype(np.float32)
    ub = (0.1 * rng.standard_normal(U3)).astype(np.float32)
    ib = (0.1 * rng.standard_normal(N3)).astype(np.float32)
    kw = dict(epilogue=epilogue, scale=0.05, user_bias=ub, item_bias=ib, bias0=0.01)
    val, idx, dense = _fused(X, W, k, want_scores=True, **kw)
    rv, ri = R.topk(dense, k)
    np.testing.assert_array_equal(idx, ri)
    assert R.same_bits(val, rv)
    v, i = _fused(X, W, k, slices=5, **kw)
    np.testing.assert_array_equal(i, ri)
    assert R.same_bits(v, rv)


# ---- 4. memory ---------------------------------------------------------------------------------------------------------
def test_fused_memory_does_not_grow_with_users_times_items():
    U, N, D, k = 4096, 200001, 64, 10
    g = torch.Generator(device="cpu").manual_seed(5)
    X = (0.1 * torch.randn(U, D, generator=g)).to(DEV)
    W = (0.1 * torch.randn(N, D, generator=g)).to(DEV)
    limit = U * N * 4 // 16
    a = _C.FrRecArgs(X.data_ptr(), W.data_ptr(), 0, 0, 0, 0, 0, U, N, 0, D, k, 0, 1, 0, 0, 0.0, 1.0)
    import ctypes
    ws = _C.lib().fr_recommend_topk_workspace_bytes(ctypes.byref(a))
    assert 0 < ws + U * k * (4 + 8) < limit
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    val, idx = recommend_topk(X, W, k, mask_pad=True)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before < limit
    # the lists are right for a sample of the users
    sel = np.arange(0, U, 257)
    s = (X[sel].double() @ W.double().T).cpu().numpy()
    s[:, 0] = -np.inf
    top = np.sort(s, 1)[:, ::-1][:, :k]
    got = np.take_along_axis(s, idx[sel].cpu().numpy(), 1)
    np.testing.assert_allclose(got, top, atol=1e-5)

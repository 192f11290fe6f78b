"""numpy restatement of the recommendation kernels' contract (csrc/recommend.hip), for the tests.

- The total order: higher score first, NaN above +inf, the lower id first among equal scores (all NaNs equal, -0 == +0):
  a stable argsort on (NaN first, then -score, then id).
- float64 scores of the fused entry and the rounding bound of its fp32 dot product in ANY summation order,
  tau(u, i) = gamma_D * sum_d |x_ud * w_id| with gamma_D = D u / (1 - D u), u = 2^-24, plus 4 ulp of the result for the
  epilogues 1 and 2 (the division, expf)."""
import numpy as np


def order(row):
    """Indices of a 1-d score row from best to worst."""
    row = np.asarray(row)
    nan = np.isnan(row)
    neg = np.where(nan, 0.0, -row.astype(np.float64))
    return np.lexsort((np.arange(row.size), neg, ~nan))       # last key first: NaN, then -score, then id


def topk(scores, k):
    """(values, indices) [rows, k] of a 2-d fp32 matrix in the total order; the values are the cells' own bits."""
    scores = np.asarray(scores, dtype=np.float32)
    idx = np.stack([order(r)[:k] for r in scores]).astype(np.int64)
    return np.take_along_axis(scores, idx, 1), idx


def same_bits(a, b):
    """Equal fp32 arrays bit for bit, except that any NaN equals any NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def gamma(D):
    u = 2.0 ** -24
    return D * u / (1.0 - D * u)


def epilogue64(x, epilogue, scale=1.0):
    if epilogue == 1:
        return np.clip(x, 0.0, scale) / scale
    if epilogue == 2:
        return 1.0 / (1.0 + np.exp(-x))
    return x


def scores64(X, W, user_bias=None, item_bias=None, bias0=0.0, epilogue=0, scale=1.0):
    """(float64 scores [U, n_items], tau [U, n_items]) of fp32 inputs."""
    X64, W64 = np.asarray(X, np.float64), np.asarray(W, np.float64)
    s = X64 @ W64.T
    if user_bias is not None:
        s = s + np.asarray(user_bias, np.float64)[:, None]
    if item_bias is not None:
        s = s + np.asarray(item_bias, np.float64)[None, :]
    s = epilogue64(s + float(bias0), epilogue, scale)
    tau = gamma(X64.shape[1]) * (np.abs(X64) @ np.abs(W64).T)
    if epilogue:
        tau = tau + 4.0 * np.spacing(np.abs(s).astype(np.float32)).astype(np.float64)
    return s, tau


def mask(scores, mask_pad, indptr=None, items=None):
    """The pad item and the CSR's cells set to -inf (a copy)."""
    s = np.array(scores, copy=True)
    if mask_pad:
        s[:, 0] = -np.inf
    if indptr is not None:
        for u in range(s.shape[0]):
            s[u, np.asarray(items[indptr[u]:indptr[u + 1]], np.int64)] = -np.inf
    return s


def check_band(val, idx, s64, tau, k, max_band=8):
    """Check 3 of the fused entry against float64 scores `s64` (masked cells -inf) and their bound `tau`.  Returns the
    largest number of items of one user inside the band where either side is right."""
    U, N = s64.shape
    worst = 0
    for u in range(U):
        ids, v = idx[u], val[u].astype(np.float64)
        assert len(set(ids.tolist())) == k, f"user {u}: repeated items"
        assert np.all(np.isfinite(s64[u, ids])), f"user {u}: a masked item was returned"
        assert np.all(v[:-1] >= v[1:]), f"user {u}: values increase"
        assert np.all(np.abs(v - s64[u, ids]) <= tau[u, ids]), f"user {u}: a value is off its float64 score by more than tau"
        kth = np.sort(s64[u])[::-1][k - 1]
        assert np.all(s64[u, ids] >= kth - 2 * tau[u, ids]), f"user {u}: a returned item is below the k-th best by more than 2 tau"
        out = np.ones(N, bool)
        out[ids] = False
        assert np.all(s64[u, out] <= kth + 2 * tau[u, out]), f"user {u}: an item left out is above the k-th best by more than 2 tau"
        band = int(np.sum(np.isfinite(s64[u]) & (np.abs(s64[u] - kth) <= 2 * tau[u])))           # the k-th best itself included
        assert band <= max_band, f"user {u}: {band} items within 2 tau of the k-th best"
        worst = max(worst, band)
    return worst


def history_csr(indptr, items, uids):
    """The CSR of the rows `uids` (repeats allowed, order kept) of a per-user CSR, items ascending within each row."""
    indptr, items = np.asarray(indptr, np.int64), np.asarray(items, np.int64)
    rows = [np.sort(items[indptr[u]:indptr[u + 1]]) for u in np.asarray(uids, np.int64)]
    out = np.zeros(len(rows) + 1, np.int64)
    out[1:] = np.cumsum([len(r) for r in rows])
    return out, (np.concatenate(rows) if rows else np.zeros(0, np.int64))

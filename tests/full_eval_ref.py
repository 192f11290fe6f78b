"""numpy restatement of what the matrix-free full-sort evaluation must return (csrc/recommend.hip: fr_recommend_cells,
fr_recommend_meanrank), for the tests.  Everything here is exact: integers, or fp32 values compared by their bits.

`meanrank(scores, pos_keys)` is `rec.meanrank` of a dense masked [users, n_items] fp32 matrix, as fr_eval_meanrank_segments
(items = NULL) defines it: per user { 2 * pos_rank_sum, user_len, pos_len } with
    user_len = cells scoring above -inf,
    pos_len  = distinct keys user * n_items + item of the user (a key outside the matrix is none),
    2 * rank of a positive p = 2 #{live cells > p} + #{live cells == p} + 1     (a tied rank is a half: hence the doubling),
where a positive that is a masked cell scores -inf: every live cell ranks above it and none ties with it."""
import numpy as np


def meanrank(scores, pos_keys):
    scores = np.asarray(scores, np.float32)
    U, N = scores.shape
    keys = np.unique(np.asarray(pos_keys, np.int64).reshape(-1))
    keys = keys[(keys >= 0) & (keys < U * N)]
    out = np.zeros((U, 3), np.int64)
    for u in range(U):
        row = scores[u]
        live = row[row > -np.inf]                       # (a NaN is no live cell)
        out[u, 1] = live.size
        for item in keys[(keys >= u * N) & (keys < (u + 1) * N)] - u * N:
            sp = row[item]
            out[u, 0] += 2 * int(np.sum(live > sp)) + int(np.sum(live == sp)) + 1
            out[u, 2] += 1
    return out


def positives(rng, U, N, indptr=None, items=None, long_user=None, empty_user=None, long_len=300):
    """Sorted keys of a batch: 0..8 positives per user, none for `empty_user`, min(long_len, N) for `long_user`, the pad item of
    one user, one cell of a history when there is one, one key listed twice and one key beyond the matrix."""
    keys = []
    for u in range(U):
        n = int(rng.integers(0, min(8, N) + 1))
        if u == long_user:
            n = min(long_len, N)
        if u == empty_user:
            continue
        keys.extend(u * N + rng.choice(N, n, replace=False))
    last = U - 1 if U - 1 != empty_user else (0 if empty_user != 0 else None)
    if last is not None:
        keys.append(last * N)                           # the pad item: a masked positive
        if indptr is not None:
            for u in range(U):
                if u != empty_user and indptr[u + 1] > indptr[u]:
                    keys.append(u * N + int(items[indptr[u]]))      # a positive inside the history
                    break
    if keys:
        keys.append(keys[len(keys) // 2])               # a key listed twice
    keys.append(U * N + 1)                              # beyond the matrix: no positive of anyone
    return np.sort(np.asarray(keys, np.int64))


def histories(rng, U, N, most=40):
    """A per-user CSR of ascending items in 1..N-1 (some users without any)."""
    rows = []
    for u in range(U):
        n = int(rng.integers(0, min(most, N - 1) + 1)) if N > 1 else 0
        rows.append(np.sort(rng.choice(np.arange(1, N), n, replace=False)) if n else np.zeros(0, np.int64))
    indptr = np.zeros(U + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, np.concatenate(rows).astype(np.int64)

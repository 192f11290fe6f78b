"""Plain numpy reference of the FairGo graph kernels (csrc/graph.hip, csrc/frontier.hip): no torch, no GPU.

* `spmm_sel_ref`: the frontier-restricted product of fr_spmm_csr_sel in float64, with what its error bound needs: per output
  element sum |val * x| over the kept terms, and per output row the number of kept terms.
* `gamma`: the bound of a chain of n float32 roundings, gamma_n = n u / (1 - n u) with u = 2^-24 (Higham, Accuracy and
  Stability of Numerical Algorithms, Lemma 3.1).  A row of n kept terms is n fmaf steps in a fixed order, so
  |got - exact| <= gamma_n * sum |val x|; the tests allow gamma_(n+1), one step more for the float64 reference's own
  rounding (n * 2^-53 * sum |val x|, far below u) and nothing else.
* `act_bwd_ref`, `act_grid`: the derivative through the activation's output in float64 (leaky relu's slope is the float32
  constant 0.01f), and outputs on a dyadic grid where that derivative is exact in float32 however `1 - y * y` is evaluated
  (y = k / 8: y * y = k^2 / 64 and 1 - y * y = (64 - k^2) / 64 have at most 7 significant bits; fused or not, no rounding).
* `scatter_f32`: fr_row_scatter_sum's contract "duplicates summed in ascending position" restated IN FLOAT32: every row starts
  at 0.0f and takes its members one by one in position order.  `scatter_ref`: the same sum in float64 with sum |g| and the
  member count, for the order-independent bound gamma_n * sum |g|.
* `bits_of`, `ids_of`, `frontier_*_ref`: the bitmap row sets of fr_frontier_mark / _expand / _count / _scatter as numpy sets.
* `mse_ref`: nn.MSELoss and its gradient in float64.
* `graph_a`, `graph_b`, `maps_for`: the CSR matrices and column maps the kernel tests run on, built here so that the CPU
  suite can assert the structures they are chosen for (tests/test_graph_ref.py).

A CSR matrix is a SimpleNamespace(indptr int64 [n_rows + 1], col int32 sorted within a row, val float32, n_rows, n_cols).
"""
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
LEAKY = float(np.float32(0.01))
ACT_RELU, ACT_LEAKY, ACT_SIGMOID, ACT_TANH = 1, 2, 3, 4


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def normals(rng, shape):
    """float32 values of magnitude 0.1 .. 1 with a random sign: finite normals, no subnormal enters a product's operands"""
    return (rng.uniform(0.1, 1.0, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def make_csr(lengths, n_cols, rng):
    lengths = np.asarray(lengths, dtype=np.int64)
    assert lengths.min() >= 0 and lengths.max() <= n_cols
    indptr = np.zeros(len(lengths) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(lengths)
    col = np.concatenate([np.sort(rng.choice(n_cols, int(n), replace=False)) for n in lengths] + [np.zeros(0, dtype=np.int64)])
    return SimpleNamespace(indptr=indptr, col=col.astype(np.int32), val=normals(rng, len(col)), n_rows=len(lengths), n_cols=n_cols)


def head_rows(g, n):
    """the first n rows of g as a matrix of its own (same arrays: fr_spmm_csr_sel reads indptr[0 .. n] only)"""
    return SimpleNamespace(indptr=g.indptr[:n + 1], col=g.col, val=g.val, n_rows=n, n_cols=g.n_cols)


A_ROWS, A_COLS = 300, 333
A_PLACED = {0: 0, 1: 1, 2: 63, 3: 64, 4: 65, 5: 129, 6: 333, 7: 0, 299: 0}
A_SUBSET = 37


def graph_a():
    """300 x 333 (333 is no multiple of 32: the bitmap's tail word is partial).  Rows 0 and 299 are empty, rows 1 .. 6 hold 1,
    63, 64, 65, 129 and 333 nonzeros (one 64-nonzero chunk less one, exactly one, one more, two and one more, every column),
    the others 0 .. 20."""
    rng = np.random.default_rng(300333)
    lengths = rng.integers(0, 21, A_ROWS)
    for r, n in A_PLACED.items():
        lengths[r] = n
    return make_csr(lengths, A_COLS, rng)


def rows_a():
    """37 ascending output rows of graph A: every hand-placed row and 28 of the others"""
    rng = np.random.default_rng(37)
    rest = rng.choice(np.setdiff1d(np.arange(A_ROWS), list(A_PLACED)), A_SUBSET - len(A_PLACED), replace=False)
    return np.sort(np.concatenate([np.array(list(A_PLACED)), rest])).astype(np.int32)


B_ROWS, B_COLS = 1037, 700
B_PLACED = [0] * 8 + [256, 257, 600, 0, 0, 1, 0, 700] + [0, 1, 0, 255, 0, 1, 0, 0] + [32] * 8


def graph_b():
    """1037 x 700 for the runs kernel (a wave owns 8 / 16 / 32 consecutive rows and walks their nonzeros 256 at a time):
    1037 = 32 * 32 + 13 leaves a tail run of 5 (of 13 at 32 rows per wave) and idle waves in the last workgroup.  Rows 0 .. 31
    are placed by hand (B_PLACED), the last row is not empty, of the others about a third is empty and the rest holds 1 .. 40."""
    rng = np.random.default_rng(1037700)
    lengths = np.where(rng.random(B_ROWS) < 1.0 / 3.0, 0, rng.integers(1, 41, B_ROWS))
    lengths[:len(B_PLACED)] = B_PLACED
    lengths[B_ROWS - 1] = 17
    return make_csr(lengths, B_COLS, rng)


def column_map(n_cols, kept, rng):
    """map[c] = row of column c in a compact block (a random bijection of the kept columns onto 0 .. n_x - 1), -1 elsewhere"""
    kept = np.asarray(kept, dtype=np.int64)
    m = np.full(n_cols, -1, dtype=np.int32)
    m[kept] = rng.permutation(len(kept)).astype(np.int32)
    return m


def maps_for(n_cols, share):
    """the column maps of a test graph: `share` of the columns at random, every column, none, exactly one"""
    rng = np.random.default_rng(n_cols)
    some = np.nonzero(rng.random(n_cols) < share)[0]
    assert 0 < len(some) < n_cols
    return {"some": column_map(n_cols, some, rng), "all": column_map(n_cols, np.arange(n_cols), rng),
            "none": column_map(n_cols, [], rng), "one": column_map(n_cols, [n_cols // 2 + 1], rng)}


def bits_of(ids, n):
    """uint32 [(n + 31) // 32] with bit i set for every i in ids"""
    w = np.zeros((n + 31) // 32, dtype=np.uint32)
    ids = np.unique(np.asarray(ids, dtype=np.int64))
    np.bitwise_or.at(w, ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
    return w


def ids_of(bits, n):
    """the ascending ids whose bit is set among the first n"""
    b = (np.asarray(bits, dtype=np.uint32)[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & np.uint32(1)
    return np.nonzero(b.reshape(-1)[:n])[0]


def map_bits(m):
    return bits_of(np.nonzero(np.asarray(m) >= 0)[0], len(m))


def whole_table(X, m, n_cols):
    """the whole-table operand a compact block stands for: row c = X[map[c]], exact zeros where the map has no row"""
    X = np.asarray(X)
    if m is None:
        return X
    W = np.zeros((n_cols, X.shape[1]), dtype=X.dtype)
    W[m >= 0] = X[m[m >= 0]]
    return W


def spmm_sel_ref(g, X, rows=None, m=None):
    """(Y, absY, kept): Y[i] = sum over the nonzeros j of row rows[i] (row i) of val[j] * X[xrow(col[j])] in float64, absY the
    same sum of |val[j] * X[.]|, kept[i] the number of terms (nonzeros whose map entry is a row)."""
    X = np.asarray(X, dtype=np.float64)
    out_rows = np.arange(g.n_rows) if rows is None else np.asarray(rows, dtype=np.int64)
    Y = np.zeros((len(out_rows), X.shape[1]))
    absY = np.zeros_like(Y)
    kept = np.zeros(len(out_rows), dtype=np.int64)
    for i, r in enumerate(out_rows):
        j0, j1 = int(g.indptr[r]), int(g.indptr[r + 1])
        c = g.col[j0:j1].astype(np.int64)
        v = g.val[j0:j1].astype(np.float64)
        if m is not None:
            c = np.asarray(m)[c].astype(np.int64)
            v, c = v[c >= 0], c[c >= 0]
        if len(c):
            t = v[:, None] * X[c]
            Y[i], absY[i], kept[i] = t.sum(0), np.abs(t).sum(0), len(c)
    return Y, absY, kept


def act_bwd_ref(y, act):
    """act'(x) written through the output y = act(x), float64"""
    y = np.asarray(y, dtype=np.float64)
    if act == ACT_RELU:
        return (y > 0).astype(np.float64)
    if act == ACT_LEAKY:
        return np.where(y > 0, 1.0, LEAKY)
    if act == ACT_SIGMOID:
        return y * (1.0 - y)
    if act == ACT_TANH:
        return 1.0 - y * y
    raise ValueError(act)


def act_grid(rng, shape, act):
    """activation outputs whose derivative float32 evaluates exactly: multiples of 1/8 in [-7/8, 7/8] for tanh and in
    [1/8, 7/8] for the sigmoid; for the two relus signed values of magnitude 0.1 .. 1 with exact zeros among them"""
    if act == ACT_TANH:
        return (rng.integers(-7, 8, shape) / 8.0).astype(np.float32)
    if act == ACT_SIGMOID:
        return (rng.integers(1, 8, shape) / 8.0).astype(np.float32)
    y = normals(rng, shape)
    y[rng.random(shape) < 0.1] = 0.0
    return y


def act_random(rng, shape, act):
    """activation outputs off the grid: tanh in (-1, 1), sigmoid in (0, 1), anything for the relus"""
    if act == ACT_TANH:
        return np.tanh(rng.normal(0.0, 1.0, shape)).astype(np.float32)
    if act == ACT_SIGMOID:
        return np.clip(1.0 / (1.0 + np.exp(-rng.normal(0.0, 2.0, shape))), 2.0 ** -20, 1.0 - 2.0 ** -20).astype(np.float32)
    return rng.normal(0.0, 1.0, shape).astype(np.float32)


def scatter_f32(g, idx, n_rows, prior=None):
    """(sums, touched): float32 [n_rows, D] whose row r is ((0.0f + g[p0]) + g[p1]) + ... over the positions p0 < p1 < ... with
    idx[p] == r, one float32 addition per member; with `prior`, float32(prior[r] + that sum) at the rows that have a member
    and prior[r] itself elsewhere.  Ids outside [0, n_rows) contribute nothing."""
    g = np.asarray(g, dtype=np.float32)
    idx = np.asarray(idx, dtype=np.int64)
    acc = np.zeros((n_rows, g.shape[1]), dtype=np.float32)
    touched = np.zeros(n_rows, dtype=bool)
    for p in range(len(idx)):
        r = idx[p]
        if 0 <= r < n_rows:
            acc[r] = acc[r] + g[p]
            touched[r] = True
    if prior is None:
        return acc, touched
    out = np.array(prior, dtype=np.float32, copy=True)
    out[touched] = out[touched] + acc[touched]
    return out, touched


def scatter_ref(g, idx, n_rows):
    """(S, absS, members): the same sums in float64, the sums of |g| and the member count per row"""
    g = np.asarray(g, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    ok = (idx >= 0) & (idx < n_rows)
    S = np.zeros((n_rows, g.shape[1]))
    absS = np.zeros_like(S)
    np.add.at(S, idx[ok], g[ok])
    np.add.at(absS, idx[ok], np.abs(g[ok]))
    return S, absS, np.bincount(idx[ok], minlength=n_rows)


def frontier_mark_ref(ids, n_rows, bits):
    """bits |= {ids}; an id outside [0, n_rows) sets no bit (the kernel raises FR_DEV_ERR_INDEX_RANGE for it)"""
    ids = np.asarray(ids, dtype=np.int64)
    have = set(ids_of(bits, n_rows).tolist()) | set(int(i) for i in ids if 0 <= i < n_rows)
    return bits_of(sorted(have), n_rows)


def frontier_expand_ref(g, rows, bits):
    """bits |= the columns of the listed rows of g"""
    have = set(ids_of(bits, g.n_cols).tolist())
    for r in np.asarray(rows, dtype=np.int64):
        have |= set(g.col[g.indptr[r]:g.indptr[r + 1]].tolist())
    return bits_of(sorted(have), g.n_cols)


def frontier_count_ref(bits):
    return np.array([bin(int(w)).count("1") for w in np.asarray(bits, dtype=np.uint32)], dtype=np.int32)


def frontier_scatter_ref(bits, n_rows):
    """(rows_out, pos): the set's ids ascending, and pos[row] = rank of the row in the set, -1 outside it"""
    rows_out = ids_of(bits, n_rows).astype(np.int32)
    pos = np.full(n_rows, -1, dtype=np.int32)
    pos[rows_out] = np.arange(len(rows_out), dtype=np.int32)
    return rows_out, pos


def mse_ref(pred, target):
    """(loss, dpred) of nn.MSELoss in float64: mean (pred - target)^2 and 2 (pred - target) / B"""
    e = np.asarray(pred, dtype=np.float64) - np.asarray(target, dtype=np.float64)
    return float((e * e).sum() / len(e)), 2.0 * e / len(e)

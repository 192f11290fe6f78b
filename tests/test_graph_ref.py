"""CPU: tests/graph_ref.py -- the numpy reference the graph kernel tests compare with -- against dense numpy at tiny sizes and
hand-worked cases, and the structures the two test graphs are built for."""
import numpy as np
import pytest

import graph_ref as R


def _dense(g):
    L = np.zeros((g.n_rows, g.n_cols))
    for r in range(g.n_rows):
        for j in range(g.indptr[r], g.indptr[r + 1]):
            L[r, g.col[j]] += float(g.val[j])
    return L


def _tiny(seed=5, n_rows=9, n_cols=11):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, n_cols + 1, n_rows)
    lengths[[0, 4]] = 0
    lengths[3] = n_cols
    return R.make_csr(lengths, n_cols, rng), rng


def test_gamma_is_the_bound_of_a_rounding_chain():
    assert R.gamma(1) == pytest.approx(2.0 ** -24, rel=1e-6)
    assert R.gamma(0) == 0.0
    # a chain of n float32 additions of equal-signed terms stays inside gamma_(n-1) * sum
    x = R.normals(np.random.default_rng(0), 2000)
    x = np.abs(x)
    acc = np.float32(0.0)
    for v in x:
        acc = np.float32(acc + v)
    exact = float(x.astype(np.float64).sum())
    assert abs(float(acc) - exact) <= R.gamma(len(x) - 1) * exact
    assert abs(float(acc) - exact) > 0.0


def test_normals_are_finite_normals_of_magnitude_a_tenth_to_one():
    x = R.normals(np.random.default_rng(1), (50, 7))
    assert x.dtype == np.float32 and (np.abs(x) >= np.float32(0.1) - 1e-8).all() and (np.abs(x) <= 1.0).all()
    assert (x < 0).any() and (x > 0).any()


@pytest.mark.parametrize("with_rows", [False, True])
@pytest.mark.parametrize("which", [None, "some", "all", "none", "one"])
def test_spmm_sel_ref_equals_the_dense_product(with_rows, which):
    g, rng = _tiny()
    L = _dense(g)
    m = None if which is None else R.maps_for(g.n_cols, 0.4)[which]
    n_x = g.n_cols if m is None else int((m >= 0).sum())
    X = R.normals(rng, (max(n_x, 1), 3))
    rows = np.array([0, 3, 3, 8], dtype=np.int32) if with_rows else None
    Y, absY, kept = R.spmm_sel_ref(g, X, rows, m)
    W = R.whole_table(X, m, g.n_cols).astype(np.float64)
    sel = np.arange(g.n_rows) if rows is None else rows
    np.testing.assert_allclose(Y, (L @ W)[sel], rtol=0, atol=1e-14)
    np.testing.assert_allclose(absY, (np.abs(L) @ np.abs(W))[sel], rtol=0, atol=1e-14)
    live = np.ones(g.n_cols, dtype=bool) if m is None else m >= 0
    np.testing.assert_array_equal(kept, ((L != 0) & live[None, :]).sum(1)[sel])
    if which == "none":
        assert not Y.any() and not kept.any()
    if which == "one":
        assert kept.max() == 1


def test_column_maps_are_bijections_and_their_bitmaps_match():
    for name, m in R.maps_for(333, 0.3).items():
        kept = m[m >= 0]
        np.testing.assert_array_equal(np.sort(kept), np.arange(len(kept)))
        np.testing.assert_array_equal(R.ids_of(R.map_bits(m), 333), np.nonzero(m >= 0)[0])
        assert len(R.map_bits(m)) == 11
        assert {"all": 333, "none": 0, "one": 1}.get(name, len(kept)) == len(kept)
    some = R.maps_for(333, 0.3)["some"]
    assert 0.2 * 333 < (some >= 0).sum() < 0.4 * 333
    assert not np.array_equal(some[some >= 0], np.arange((some >= 0).sum()))      # the rank is not the position's


def test_bits_round_trip_and_tail_word():
    ids = [0, 31, 32, 33, 63, 64, 332]
    w = R.bits_of(ids + [31, 0], 333)
    assert w.dtype == np.uint32 and len(w) == 11
    assert w[0] == (1 | 1 << 31) and w[1] == (1 | 2 | 1 << 31) and w[2] == 1 and w[10] == 1 << (332 - 320)
    np.testing.assert_array_equal(R.ids_of(w, 333), ids)
    np.testing.assert_array_equal(R.ids_of(w, 332), ids[:-1])
    assert len(R.bits_of([], 1)) == 1 and not R.bits_of([], 1).any()


def test_act_bwd_ref_and_the_grid_on_which_float32_is_exact():
    y = np.array([-0.5, 0.0, 0.25, 0.875])
    np.testing.assert_array_equal(R.act_bwd_ref(y, R.ACT_RELU), [0, 0, 1, 1])
    np.testing.assert_array_equal(R.act_bwd_ref(y, R.ACT_LEAKY), [R.LEAKY, R.LEAKY, 1, 1])
    np.testing.assert_array_equal(R.act_bwd_ref(y, R.ACT_SIGMOID), y * (1 - y))
    np.testing.assert_array_equal(R.act_bwd_ref(y, R.ACT_TANH), 1 - y * y)
    assert R.LEAKY != 0.01 and np.float32(R.LEAKY) == np.float32(0.01)
    rng = np.random.default_rng(2)
    for act, lo, hi in ((R.ACT_TANH, -7, 7), (R.ACT_SIGMOID, 1, 7)):
        y = R.act_grid(rng, 4000, act)
        assert y.dtype == np.float32 and set(np.unique(y * 8).tolist()) == set(range(lo, hi + 1))
        d = R.act_bwd_ref(y, act)
        np.testing.assert_array_equal(d.astype(np.float32).astype(np.float64), d)       # representable ...
        one = np.float32(1.0)
        rounded = (one - y * y) if act == R.ACT_TANH else y * (one - y)                    # ... and every float32 step exact
        np.testing.assert_array_equal(rounded.astype(np.float64), d)
        assert (d > 0).all()
    for act in (R.ACT_RELU, R.ACT_LEAKY):
        y = R.act_grid(rng, 4000, act)
        assert (y == 0).any() and (y > 0).any() and (y < 0).any()
    for act in (R.ACT_SIGMOID, R.ACT_TANH):
        y = R.act_random(rng, 4000, act)
        assert y.dtype == np.float32 and (np.abs(y) < 1).all() and (act == R.ACT_TANH or (y > 0).all())


def test_scatter_f32_adds_in_ascending_position():
    # 2^24 + 1 + 1: one by one from the left both ones are lost, any other order keeps them
    g = np.array([[2.0 ** 24], [1.0], [7.0], [1.0]], dtype=np.float32)
    idx = [2, 2, 0, 2]
    s, touched = R.scatter_f32(g, idx, 4)
    np.testing.assert_array_equal(s[:, 0], [7.0, 0.0, 2.0 ** 24, 0.0])
    np.testing.assert_array_equal(touched, [True, False, True, False])
    s, _ = R.scatter_f32(g[::-1], idx[::-1], 4)
    assert s[2, 0] == 2.0 ** 24 + 2
    # the sum is formed first and added to the prior value in one step; rows without a member keep theirs, NaN included
    prior = np.array([[1.0], [np.nan], [-(2.0 ** 24)], [5.0]], dtype=np.float32)
    a, _ = R.scatter_f32(g, idx, 4, prior)
    assert a[0, 0] == 8.0 and np.isnan(a[1, 0]) and a[2, 0] == 0.0 and a[3, 0] == 5.0
    # ids outside the table (the sort's padding hole -1 among them) contribute nothing
    s, touched = R.scatter_f32(g, [-1, 4, 0, -5], 4)
    np.testing.assert_array_equal(s[:, 0], [7.0, 0, 0, 0])
    assert touched.sum() == 1


def test_scatter_ref_equals_a_dense_one_hot_product():
    rng = np.random.default_rng(4)
    g = R.normals(rng, (40, 3))
    idx = rng.integers(0, 6, 40)
    idx[[3, 9]] = [-1, 6]
    S, absS, members = R.scatter_ref(g, idx, 6)
    P = (idx[None, :] == np.arange(6)[:, None]).astype(np.float64)
    np.testing.assert_allclose(S, P @ g.astype(np.float64), rtol=0, atol=1e-14)
    np.testing.assert_allclose(absS, P @ np.abs(g.astype(np.float64)), rtol=0, atol=1e-14)
    np.testing.assert_array_equal(members, P.sum(1))
    s32, _ = R.scatter_f32(g, idx, 6)
    assert (np.abs(s32 - S) <= R.gamma(members)[:, None] * absS).all()


def test_frontier_refs_against_python_sets():
    g, _ = _tiny()
    bits = R.frontier_mark_ref([3, 3, 8, -1, 9], g.n_rows, R.bits_of([1], g.n_rows))
    np.testing.assert_array_equal(R.ids_of(bits, g.n_rows), [1, 3, 8])
    cols = R.frontier_expand_ref(g, [0, 8, 8, 4], R.bits_of([10], g.n_cols))
    want = {10} | set(g.col[g.indptr[8]:g.indptr[9]].tolist())
    np.testing.assert_array_equal(R.ids_of(cols, g.n_cols), sorted(want))
    np.testing.assert_array_equal(R.ids_of(R.frontier_expand_ref(g, [3], R.bits_of([], g.n_cols)), g.n_cols), np.arange(g.n_cols))
    np.testing.assert_array_equal(R.frontier_count_ref(np.array([0, 1, 0xFFFFFFFF, 0x80000001], dtype=np.uint32)), [0, 1, 32, 2])
    rows_out, pos = R.frontier_scatter_ref(R.bits_of([0, 31, 32, 40], 41), 41)
    np.testing.assert_array_equal(rows_out, [0, 31, 32, 40])
    assert pos[0] == 0 and pos[31] == 1 and pos[32] == 2 and pos[40] == 3 and (pos >= 0).sum() == 4 and pos.min() == -1


def test_mse_ref():
    loss, d = R.mse_ref([1.0, 2.0, 4.0], [1.0, 4.0, 1.0])
    assert loss == 13.0 / 3.0
    np.testing.assert_array_equal(d, np.array([0.0, -4.0, 6.0]) / 3.0)


def test_graph_a_has_the_rows_the_row_wise_kernel_can_get_wrong():
    g = R.graph_a()
    n = np.diff(g.indptr)
    assert (g.n_rows, g.n_cols) == (300, 333) and g.n_cols % 32 != 0
    assert n[0] == 0 and n[-1] == 0
    assert [int(n[r]) for r in range(1, 7)] == [1, 63, 64, 65, 129, 333]
    assert n[8:-1].max() <= 20 and n[8:-1].min() == 0
    for r in range(g.n_rows):
        c = g.col[g.indptr[r]:g.indptr[r + 1]]
        assert (np.diff(c) > 0).all() and (len(c) == 0 or (c[0] >= 0 and c[-1] < g.n_cols))
    assert g.val.dtype == np.float32 and (np.abs(g.val) >= np.float32(0.1) - 1e-8).all() and (np.abs(g.val) <= 1).all()
    rows = R.rows_a()
    assert len(rows) == 37 and (np.diff(rows) > 0).all() and set(R.A_PLACED) <= set(rows.tolist())
    m = R.maps_for(g.n_cols, 0.3)["some"]
    _, _, kept = R.spmm_sel_ref(g, np.zeros((int((m >= 0).sum()), 1)), None, m)
    assert (kept[n > 0] == 0).any() and (kept > 0).any()        # non-empty rows no kept term reaches, and reached ones
    assert (m[320:] >= 0).any()                                  # a kept column in the bitmap's partial tail word


def test_graph_b_has_the_runs_the_runs_kernel_can_get_wrong():
    g = R.graph_b()
    n = np.diff(g.indptr)
    assert (g.n_rows, g.n_cols) == (1037, 700) and g.n_rows == 32 * 32 + 13 and g.n_cols % 32 != 0
    assert not n[0:8].any()
    assert n[8:16].tolist() == [256, 257, 600, 0, 0, 1, 0, 700]
    assert n[16:24].tolist() == [0, 1, 0, 255, 0, 1, 0, 0]
    assert g.indptr[20] - g.indptr[16] == 256                   # the run's first trip ends exactly where row 19 does
    assert n[24:32].tolist() == [32] * 8 and g.indptr[32] - g.indptr[24] == 256
    assert n[-1] > 0 and g.indptr[-1] == len(g.col)
    rest = n[32:-1]
    assert rest.max() <= 40 and 0.25 < (rest == 0).mean() < 0.42
    m = R.maps_for(g.n_cols, 0.02)["some"]
    assert 5 <= (m >= 0).sum() <= 25
    h = R.head_rows(g, 1024)
    assert h.n_rows == 1024 and len(h.indptr) == 1025

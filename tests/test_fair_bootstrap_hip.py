"""GPU: fr_bootstrap_fair_metrics (csrc/bootstrap_fair.hip) through the C ABI against the float64 restatement of
tests/fair_bootstrap_ref.py (pinned on the CPU by tests/test_fair_bootstrap_ref.py).  Shapes are the smallest that reach each edge:
1 .. 257 replicates (the Philox quad, the wave of 256 replicates), 1 / 2 / 17 / 257 items (one chunk, two, fewer chunks than
items, more than the 64 item ends staged at a time) with item 0 of 1000 members (16 member tiles inside one item) and the rest of
1 / 15 / 16 / 17 / 33, 2 / 3 / 8 groups (both kernel widths), perm NULL and a real permutation, wtrue NULL and ones-then-zeros.
Every output and every workspace sits between canary frames, every return code is asserted, as in
tests/test_metrics_kernels_hip.py.

Tolerances are derived in tests/fair_bootstrap_ref.py: K_b and the group weights exact; gamma_(n_g + 1) sum w |value| for the
group sums; the reference's own bound plus the slack of this kernel's cell sums and summation order for the five metrics; NaN
exactly in the reference's replicates.  Every test prints its largest error / bound, none may exceed 1.

Worst error / bound measured on an MI355X, per test group (K_b and the group weights exact everywhere):
  the group sums 0 everywhere: float32 values in (0.001, 1) times weights up to 12, a few thousand of them, add up exactly in
  double in any order (the cell sums S are exact for the same reason; what the figures below measure is the per-item chain)
  1 .. 257 replicates 0.079 (B = 257; 0.0019 at B = 1, 0.027 .. 0.050 between)
  items x groups x perm 0.13 (K = 1, G = 3, a real perm; 0.02 .. 0.12 elsewhere; K = 257: 0.04 .. 0.11)
  want = value-type only 0.0005, DifferentialFairness only 0.027 (the value-type bound scales with max |p|, |r|; the
  DifferentialFairness figures are the device logf against e = 3.3)
  items of their own users (K_b varies) 0.074 (K = 17) and 0.087 (K = 257, G = 3); one user 0.029, NaN in the reference's replicates
  group indices outside [0, G) 0.028 (G = 2), 0.046 (G = 8)
  the Python wrapper 0.046 (DifferentialFairness; value-type 0.00025, NonParity 0)
"""
import functools

import numpy as np
import pytest
import torch

import bootstrap_ref as BR
import fair_bootstrap_ref as FR
from test_metrics_kernels_hip import EINVAL, _bytes, _dev, _Frames, _lib, _logf_ulp, _ptr, _refused, _st, _untouched, _within

pytestmark = pytest.mark.gpu
SEED = 2020


def _run(case, G, n_rep, want, seed=SEED):
    """-> (terms [5, B], items [B], group_sum [G, B], group_weight [G, B]) as numpy"""
    perm, start, group, value, wtrue, unit = case
    K, M = len(start) - 1, len(group)
    lib, f = _lib(), _Frames()
    terms, items = f.new(torch.float64, 5, n_rep), f.new(torch.int64, n_rep)
    gsum, gw = f.new(torch.float64, G, n_rep), f.new(torch.int64, G, n_rep)
    need = lib.fr_bootstrap_fair_metrics_workspace_bytes(M, K, G, n_rep)
    assert need == FR.workspace_bytes(M, K, G, n_rep)
    ws = f.ws(need)
    d = [_dev(x) for x in (perm, start, group, value, wtrue, unit)]
    rc = lib.fr_bootstrap_fair_metrics(_ptr(d[0]), d[1].data_ptr(), K, M, d[2].data_ptr(), d[3].data_ptr(), _ptr(d[4]),
                                       d[5].data_ptr(), G, n_rep, seed, want, terms.data_ptr(), items.data_ptr(), gsum.data_ptr(),
                                       gw.data_ptr(), ws.data_ptr(), need, _st())
    assert rc == 0, lib.fr_last_error()
    assert f.intact()
    return terms.cpu().numpy(), items.cpu().numpy(), gsum.cpu().numpy(), gw.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case_ref(n_items, G, with_perm, wtrue_kind, unit_kind, bad_groups, n_rep):
    case = FR.case(n_items, G, with_perm, wtrue_kind, unit_kind, bad_groups)
    return case, FR.replicates_ref(*case, G, n_rep, SEED, _logf_ulp())


def _check(tag, got, ref, G, want):
    """K_b and the group weights exact, the group sums within gamma_(n_g + 1) sum w |value|, the wanted metrics (term sum / K_b)
    within the reference's bounds and NaN exactly where it is, the others exactly +0.0"""
    terms, items, gsum, gw = got
    assert np.array_equal(items, ref["items"]), f"{tag}: K_b differs"
    assert np.array_equal(gw, ref["group_weight"]), f"{tag}: group weights differ"
    gam = np.array([FR.R.gamma(int(n) + 1) for n in ref["group_size"]])[:, None]
    worst = _within(tag + " group sums", gsum, ref["group_sum"], gam * ref["group_abs"])
    rows = [q for q in range(5) if (q < 4 and want & FR.WANT_VALUE) or (q == 4 and want & FR.WANT_DF)]
    for q in range(5):
        if q not in rows:
            assert _bytes(torch.from_numpy(terms[q])) == _bytes(torch.zeros(len(items), dtype=torch.float64)), f"{tag}: row {q}"
    if rows:
        with np.errstate(invalid="ignore", divide="ignore"):
            values = terms[rows] / items[None, :]
        dead = items == 0
        assert np.isnan(values[:, dead]).all() and np.isnan(ref["values"][rows][:, dead]).all(), f"{tag}: NaN replicates differ"
        live = ~dead
        if live.any():
            worst = max(worst, _within(tag + " metrics", values[:, live], ref["values"][rows][:, live], ref["bounds"][rows][:, live]))
    return worst


@pytest.mark.parametrize("n_rep", FR.N_REPS)
def test_replicate_counts(n_rep):
    case, ref = _case_ref(17, 2, True, "ones", "spread", False, n_rep)
    want = FR.WANT_VALUE | FR.WANT_DF
    _check(f"fair bootstrap B={n_rep}", _run(case, 2, n_rep, want), ref, 2, want)


@pytest.mark.parametrize("with_perm", [False, True])
@pytest.mark.parametrize("G", FR.GROUPS)
@pytest.mark.parametrize("n_items", FR.N_ITEMS)
def test_items_groups_and_perm(n_items, G, with_perm):
    wtrue_kind = "ones" if (n_items + G) % 2 else "null"
    case, ref = _case_ref(n_items, G, with_perm, wtrue_kind, "spread", False, 5)
    assert ref["items"].min() >= 1 and (ref["group_weight"] > 0).all()           # (a one-member item may vanish with its user)
    want = (FR.WANT_VALUE if G == 2 else 0) | FR.WANT_DF
    _check(f"fair bootstrap K={n_items} G={G} perm={'yes' if with_perm else 'NULL'} wtrue={wtrue_kind}", _run(case, G, 5, want), ref, G, want)


@pytest.mark.parametrize("want", [0, FR.WANT_VALUE, FR.WANT_DF])
def test_want_selects_the_rows(want):
    case, ref = _case_ref(17, 2, True, "ones", "spread", False, 5)
    _check(f"fair bootstrap want={want}", _run(case, 2, 5, want), ref, 2, want)


@pytest.mark.parametrize("n_items,G", [(17, 2), (257, 3)])
def test_items_vanish_with_their_users(n_items, G):
    """every single-member item belongs to a user of its own: K_b varies and equals the reference exactly; alpha = 1 / K_b"""
    case, ref = _case_ref(n_items, G, True, "ones", "own", False, 65)
    assert len(set(ref["items"].tolist())) > 1 and ref["items"].max() <= n_items
    want = (FR.WANT_VALUE if G == 2 else 0) | FR.WANT_DF
    _check(f"fair bootstrap K={n_items} G={G}, items of their own users", _run(case, G, 65, want), ref, G, want)


def test_one_user_owns_every_member():
    """the replicates in which that user has weight 0 have K_b = 0 and are NaN, exactly the reference's"""
    case, ref = _case_ref(17, 2, False, "ones", "one", False, 65)
    dead = BR.weights([5], 65, SEED)[0] == 0
    assert dead.any() and (~dead).any() and np.array_equal(ref["items"] == 0, dead)
    want = FR.WANT_VALUE | FR.WANT_DF
    got = _run(case, 2, 65, want)
    _check("fair bootstrap, one user", got, ref, 2, want)
    assert (got[3][:, dead] == 0).all() and (got[2][:, dead] == 0).all()


@pytest.mark.parametrize("G", [2, 8])
def test_group_indices_out_of_range_are_counted_nowhere(G):
    case, ref = _case_ref(17, G, True, "ones", "spread", True, 5)
    group = case[2]
    assert ((group < 0) | (group >= G)).sum() > 50
    want = (FR.WANT_VALUE if G == 2 else 0) | FR.WANT_DF
    _check(f"fair bootstrap G={G}, group indices outside [0, G)", _run(case, G, 5, want), ref, G, want)


def test_group_weights_equal_the_row_bootstrap():
    """one member per user, unit = the row index: the integer group weights are fr_bootstrap_group_sums' out_weight"""
    from test_bootstrap_hip import _boot
    import group_metrics_ref as GR
    U, G, n_rep = 200, 3, 65
    rng = np.random.default_rng(5)
    gidx = GR.assignment(U, G)
    perm, gstart = GR.segments(gidx, G)
    values = rng.random((U, 1))
    sums, weight = _boot(values, perm, gstart, n_rep)
    items = rng.integers(0, 30, U)
    order = np.argsort(items, kind="stable").astype(np.int64)
    start = np.concatenate(([0], np.cumsum(np.unique(items, return_counts=True)[1]))).astype(np.int64)
    case = (order, start, np.asarray(gidx, dtype=np.int32), values[:, 0].astype(np.float32), None, np.arange(U, dtype=np.int64))
    got = _run(case, G, n_rep, 0)
    assert np.array_equal(got[3], weight)


def test_two_calls_give_the_same_bytes():
    case, _ = _case_ref(257, 3, True, "ones", "own", False, 65)
    a, b = _run(case, 3, 65, FR.WANT_DF), _run(case, 3, 65, FR.WANT_DF)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    case, _ = _case_ref(17, 2, True, "ones", "spread", False, 257)
    a, b = _run(case, 2, 257, 3), _run(case, 2, 257, 3)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_bad_arguments_are_refused_before_any_write():
    perm, start, group, value, wtrue, unit = FR.case(17, 2, True, "ones")
    K, M, G, B = len(start) - 1, len(group), 2, 5
    lib, f = _lib(), _Frames()
    outs = [f.new(torch.float64, 5, B), f.new(torch.int64, B), f.new(torch.float64, G, B), f.new(torch.int64, G, B)]
    need = lib.fr_bootstrap_fair_metrics_workspace_bytes(M, K, G, B)
    ws = f.ws(need)
    d = [_dev(x) for x in (perm, start, group, value, wtrue, unit)]
    good = dict(perm=d[0].data_ptr(), item_start=d[1].data_ptr(), K=K, M=M, group=d[2].data_ptr(), value=d[3].data_ptr(),
                wtrue=d[4].data_ptr(), unit=d[5].data_ptr(), G=G, B=B, seed=SEED, want=3, terms=outs[0].data_ptr(),
                items=outs[1].data_ptr(), gsum=outs[2].data_ptr(), gw=outs[3].data_ptr(), ws=ws.data_ptr(), ws_bytes=need)
    bad = [dict(item_start=None), dict(group=None), dict(value=None), dict(unit=None), dict(terms=None), dict(items=None),
           dict(gsum=None), dict(gw=None), dict(ws=None), dict(K=0), dict(M=0), dict(K=2 ** 31), dict(M=2 ** 28 + 1), dict(G=0),
           dict(G=9), dict(B=0), dict(B=65537), dict(want=4), dict(want=-1), dict(G=3, want=1), dict(ws_bytes=need - 1)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.fr_bootstrap_fair_metrics(*a.values(), _st())
        ok, info = _refused(rc, "fr_bootstrap_fair_metrics")
        assert ok, (change, info)
        assert all(_untouched(o) for o in outs) and f.intact(), change
    for args in ((0, K, G, B), (M, 0, G, B), (M, K, 0, B), (M, K, 9, B), (M, K, G, 0), (M, K, G, 65537), (2 ** 28 + 1, K, G, B)):
        assert lib.fr_bootstrap_fair_metrics_workspace_bytes(*args) == 0, args
    assert EINVAL == -1
    rc = lib.fr_bootstrap_fair_metrics(*good.values(), _st())
    assert rc == 0 and f.intact() and not any(_untouched(o) for o in outs)


def test_python_wrapper():
    from fairrec.evaluator import bootstrap_fairness
    case, ref = _case_ref(17, 2, False, "ones", "own", False, 65)
    _, start, group, value, wtrue, unit = case
    items = np.repeat(np.arange(17) * 3 + 1, np.diff(start))                       # item ids ascending with the positions
    shuffle = np.random.default_rng(3).permutation(len(items))                     # the wrapper sorts by item, stably
    inv = np.argsort(shuffle, kind="stable")
    order = np.argsort(items[shuffle], kind="stable")
    assert not np.array_equal(shuffle[order], np.arange(len(items)))
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a[shuffle])).cuda()
    got = bootstrap_fairness(d(items), d(group), d(value), d(wtrue), d(unit), 2, 65, SEED, value_type=True, differential=True)
    ref2 = FR.replicates_ref(order, start, group[shuffle], value[shuffle], wtrue[shuffle], unit[shuffle], 2, 65, SEED, _logf_ulp())
    assert np.array_equal(got["items"], ref2["items"]) and np.array_equal(ref2["items"], ref["items"]) and inv.size
    for q, name in enumerate(FR.NAMES):
        _within(f"bootstrap_fairness {name}", got[name], ref2["values"][q], ref2["bounds"][q])
    val, bnd = FR.nonparity_ref(ref2)
    _within("bootstrap_fairness nonparity", got["nonparity"], val, bnd)

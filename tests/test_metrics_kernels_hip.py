"""GPU: the four kernels of csrc/metrics.hip that every reported number comes out of -- fr_topk_metrics, fr_eval_hits,
fr_group_sums, fr_fair_metrics_from_stats -- one by one through the C ABI against the plain references of tests/metrics_ref.py
(pinned to oracle/metrics.py on the CPU by tests/test_metrics_ref.py), at the smallest shapes that reach each edge: the
64-user wave of the top-k kernel, the 16-lane sub-group and the 16 segments per block of the group sums, the 256-item block
of the fairness kernel, the U * (K + 1) grid tail of the hit matrix.  Every output buffer and every workspace sits between
canary frames; outputs start as NaN (a sentinel for integers), workspaces as 0xFF bytes; every return code is asserted and
every frame checked after the call.

Tolerances (u = 2^-53, v = 2^-24, gamma_n = n w / (1 - n w) with w = u unless said):
  * integers, counts, hit flags: exact.
  * fr_topk_metrics: every output is a mean of non-negative per-user terms, so relative errors do not grow in the sums.  Per
    user: K additions (dcg and idcg, or the precision sum), one division, one double log2 per rank -- no accuracy statement
    for the device's log2 is at hand, so 2 ulp a call; then six butterfly additions, ceil(U / 64) block additions, one
    multiplication by 1 / U and the reference's own rounding: gamma_n |ref| with n = 3 K + 9 + ceil(U / 64), and never
    looser than 1e-13 |ref| (n <= 313 here: 3.5e-14).
  * fr_group_sums sums: gamma_(ceil(L / 16) + 5) * sum |x| per (segment, group) cell of L members against the exact fsum.
  * value-type terms: a fixed chain in double, gamma_(12 + 2 + ceil(K / 256)) * max(|p|, |r|) over the call's items.
  * DifferentialFairness: per item and pair two device logf, each within e * 2 v |log x|, and one float32 subtraction,
    v |log a - log b|; the maximum over the pairs lies between (largest true difference - its pair's bound) and the largest
    (difference + bound), see metrics_ref.fair_from_stats_ref; the mean adds double roundings only.  e: no accuracy statement
    for the device's logf is at hand, so e = 2 x the worst error of numpy's float32 logarithm on these very tables in the same
    unit, measured on the reference side (_logf_ulp: 1.65 with numpy's AVX-512 logarithm, so e = 3.3).

Worst error / bound measured on an MI355X, per case group (every test prints its own; none may exceed 1):
  fr_topk_metrics 0.12 (U = 129, K = 2); its zero-positive-row case 0.04; the Python wrapper 0.04
  fr_group_sums 0.45 (15 segments; 0.08 .. 0.30 at the other segment counts)
  value-type terms 0.0021 (the bound scales with max |p|, |r| ~ 1e4 of the spread-out tables)
  DifferentialFairness 0.16 (K = 2; 0.03 .. 0.05 from 255 items on); with a negative table entry 0.13
  the fairness_metrics chain 0.08
"""
import functools

import numpy as np
import pytest
import torch

import metrics_ref as R

pytestmark = pytest.mark.gpu

PAD = 64                    # elements of the frame on either side
EINVAL = -1
CANARY = {torch.float64: 1234.5, torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A, torch.uint8: 0xA5}
START = {torch.float64: float("nan"), torch.int32: -77777, torch.int64: -7777777777, torch.uint8: 0xFF}


def _lib():
    from fairrec import _C
    return _C.lib()


def _st():
    from fairrec import _C
    return _C.current_stream()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return 0 if t is None else t.data_ptr()


class _Frames:
    """the buffers a call may write: each between PAD canary elements, outputs prefilled with NaN / a sentinel, workspaces with
    0xFF bytes; `intact()` after the call: every frame as it was"""

    def __init__(self):
        self.held = []

    def new(self, dtype, *shape):
        n = int(np.prod(shape))
        pad = PAD * 8 if dtype == torch.uint8 else PAD           # a workspace keeps its 512-byte alignment
        whole = torch.full((pad + n + pad,), CANARY[dtype], dtype=dtype, device="cuda")
        view = whole[pad:pad + n]
        view.fill_(START[dtype])
        self.held.append((whole, pad, n, CANARY[dtype]))
        return view.view(*shape) if shape else view

    def ws(self, nbytes):
        return self.new(torch.uint8, int(nbytes))

    def intact(self):
        torch.cuda.synchronize()
        return all(bool((w[:pad] == c).all()) and bool((w[pad + n:] == c).all()) for w, pad, n, c in self.held)


def _bytes(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()


def _untouched(t):
    """an output buffer still holds what _Frames.new put there"""
    return _bytes(t) == _bytes(torch.full_like(t, START[t.dtype]))


def _within(what, got, ref, bound):
    """|got - ref| <= bound element by element, everything finite; prints and returns the largest error / bound"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape)
    assert np.isfinite(got).all(), f"{what}: not finite at {np.argwhere(~np.isfinite(got))[:4].tolist()}"
    err = np.abs(got - ref)
    assert (err[bound == 0] == 0).all(), f"{what}: an entry with a zero bound is not exact"
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"{what}: largest error / bound {ratio:.3g}")
    bad = ~(err <= bound)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} out of bound, first at {i}: got {got[i]!r}, reference "
                             f"{ref[i]!r}, bound {bound[i]:.3g}; largest error / bound {ratio:.3g}")
    return ratio


def _refused(rc, entry):
    err = _lib().fr_last_error()
    return rc == EINVAL and entry.encode() in err, (rc, err)


# ---- fr_topk_metrics -----------------------------------------------------------------------------------------------------------------

def _topk(rec):
    U, K = rec.shape[0], rec.shape[1] - 1
    lib, f = _lib(), _Frames()
    out = f.new(torch.float64, 6, K)
    need = lib.fr_topk_metrics_workspace_bytes(U, K)
    assert need == (U + 63) // 64 * 6 * K * 8
    ws = f.ws(need)
    rec_ = _dev(rec)
    rc = lib.fr_topk_metrics(rec_.data_ptr(), U, K, out.data_ptr(), ws.data_ptr(), need, _st())
    assert rc == 0 and f.intact()
    return out.cpu()


@functools.lru_cache(maxsize=None)
def _topk_ref(U, K):
    rec = R.topk_case(U, K)
    return rec, R.topk_metrics_ref(rec)


@pytest.mark.parametrize("U,K", R.TOPK_SHAPES)
def test_topk_metrics_against_exact_rationals(U, K):
    rec, ref = _topk_ref(U, K)
    assert np.isfinite(ref).all() and (ref > 0).all()
    _within(f"topk_metrics U={U} K={K}", _topk(rec).numpy(), ref, R.topk_tolerance(ref, U, K))


def test_topk_metrics_python_wrapper():
    from fairrec.evaluator import topk_metrics
    U, K = 65, 20
    rec, ref = _topk_ref(U, K)
    got = topk_metrics(_dev(rec), range(1, K + 1))
    assert len(got) == 6 * K
    vals = np.array([[got[f"{n}@{k}"] for k in range(1, K + 1)] for n in ("hit", "mrr", "ndcg", "recall", "precision", "map")])
    _within("evaluator.topk_metrics", vals, ref, R.topk_tolerance(ref, U, K))
    assert _bytes(torch.from_numpy(vals)) == _bytes(_topk(rec))          # the same launch, the same bits
    got64 = topk_metrics(torch.from_numpy(rec.astype(np.int64)).cuda(), [1, K])      # the collector's int64 matrix
    assert got64 == {k: got[k] for k in got64}


def test_topk_metrics_row_with_zero_positives():
    """hit, mrr, precision, map as the reference; ndcg its finite value (the row counts 0); recall NaN, as the reference's"""
    rec = R.topk_case(3, 20, zero_positive_row=1)
    ref = R.topk_metrics_ref(rec)
    got = _topk(rec).numpy()
    rows = [0, 1, 2, 4, 5]
    assert np.isnan(ref[3]).all() and np.isnan(got[3]).all()
    _within("topk_metrics with a zero-positive row", got[rows], ref[rows], R.topk_tolerance(ref[rows], 3, 20))
    only = _topk(rec[1:2]).numpy()
    assert (only[rows] == 0).all() and np.isnan(only[3]).all()


# ---- fr_eval_hits --------------------------------------------------------------------------------------------------------------------

def _hits(idx, n_items, keys):
    U, K = idx.shape
    f = _Frames()
    rec = f.new(torch.int32, U, K + 1)
    idx_, keys_ = _dev(idx), (_dev(keys) if len(keys) else None)
    rc = _lib().fr_eval_hits(idx_.data_ptr(), U, K, n_items, _ptr(keys_), len(keys), rec.data_ptr(), _st())
    assert rc == 0 and f.intact()
    return rec.cpu().numpy()


@pytest.mark.parametrize("U,K", R.HITS_SHAPES)
def test_eval_hits_against_the_dense_matrix(U, K):
    for n_items in R.HITS_ITEMS:
        for kind in R.HITS_NPOS:
            idx, pu, pi = R.eval_hits_case(U, K, n_items, kind)
            got = _hits(idx, n_items, R.pos_keys(n_items, pu, pi))
            assert np.array_equal(got, R.eval_hits_ref(idx, n_items, pu, pi)), (U, K, n_items, kind)


def test_eval_hits_keys_above_2_to_41():
    n_items = 2 ** 40
    idx, pu, pi = R.eval_hits_case(4, 5, n_items, "many")
    keys = R.pos_keys(n_items, pu, pi)
    ref = R.eval_hits_ref(idx, n_items, pu, pi)
    assert int(keys.max()) > 2 ** 41 and ref[:, :5].any() and not ref[:, :5].all()
    assert np.array_equal(_hits(idx, n_items, keys), ref)


def test_eval_hits_entries_out_of_range_are_no_hits():
    idx, n_items, pu, pi, want = R.eval_hits_alias_case()
    assert np.array_equal(_hits(idx, n_items, R.pos_keys(n_items, pu, pi)), want)


# ---- fr_group_sums -------------------------------------------------------------------------------------------------------------------

def _gsums(perm, seg, group, value, wtrue, G):
    K = len(seg) - 1
    f = _Frames()
    stats = f.new(torch.float64, K, G, 3)
    t = [_dev(x) for x in (perm, seg, group, value, wtrue)]
    rc = _lib().fr_group_sums(_ptr(t[0]), t[1].data_ptr(), K, t[2].data_ptr(), t[3].data_ptr(), _ptr(t[4]), G,
                              stats.data_ptr(), _st())
    assert rc == 0 and f.intact()
    return stats.cpu().numpy()


@pytest.mark.parametrize("n_segments", R.SEG_COUNTS)
def test_group_sums_against_fsum(n_segments):
    worst = 0.0
    for gi, G in enumerate(R.GROUPS):
        for vi, kind in enumerate(R.VALUE_KINDS):
            case = R.group_sums_case(n_segments, G, kind, vi % 2 == 1, R.WTRUE_KINDS[(vi + gi) % 3])
            ref, absv, abst = R.group_sums_ref(*case, G)
            got = _gsums(*case, G)
            tag = f"group_sums K={n_segments} G={G} {kind}"
            assert np.array_equal(got[:, :, 1], ref[:, :, 1]), tag              # counts, out-of-range groups nowhere
            worst = max(worst, _within(tag + " value", got[:, :, 0], ref[:, :, 0], R.group_sums_tolerance(absv, ref[:, :, 1])),
                        _within(tag + " wtrue", got[:, :, 2], ref[:, :, 2], R.group_sums_tolerance(abst, ref[:, :, 1])))
            empty = ref[:, :, 1] == 0
            assert (empty.any() or n_segments == 1) and (got[empty] == 0).all(), tag      # a group no member has: (0, 0, 0)
    print(f"group_sums K={n_segments}: worst error / bound {worst:.3g}")


# ---- fr_fair_metrics_from_stats ------------------------------------------------------------------------------------------------------

def _fair(stats, G):
    K = stats.shape[0]
    lib, f = _lib(), _Frames()
    out = f.new(torch.float64, 5)
    need = lib.fr_fair_metrics_workspace_bytes(K)
    assert need == (K + 255) // 256 * 5 * 8
    ws = f.ws(need)
    st_ = _dev(stats)
    rc = lib.fr_fair_metrics_from_stats(st_.data_ptr(), K, G, out.data_ptr(), ws.data_ptr(), need, _st())
    assert rc == 0 and f.intact()
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _logf_ulp():
    """e of the DifferentialFairness bound: twice the worst error of numpy's float32 logarithm on the tables of this file, in
    units of 2 v |log x| (reference side only)"""
    worst = max(R.logf_ulp_of_numpy(R.df_table(R.stats_case(K, G))) for K in R.STATS_ITEMS for G in R.GROUPS)
    print(f"numpy's float32 log on the tables: worst error {worst:.3g} x 2 v |log x|; e = {2 * worst:.3g}")
    return 2 * worst


@pytest.mark.parametrize("K", R.STATS_ITEMS)
def test_fair_metrics_from_stats_against_float64(K):
    worst_v, worst_d = 0.0, 0.0
    for G in R.GROUPS:
        st = R.stats_case(K, G)
        assert (R.df_table(st) > 0).all()
        ref, bound = R.fair_from_stats_ref(st, G, _logf_ulp())
        got = _fair(st, G)
        tag = f"fair_from_stats K={K} G={G}"
        if G == 2:
            assert K < 8 or (ref[:4] > 0).all()
            worst_v = max(worst_v, _within(tag + " value-type", got[:4], ref[:4], bound[:4]))
        else:
            assert _bytes(torch.from_numpy(got[:4])) == _bytes(torch.zeros(4, dtype=torch.float64)), tag      # exactly +0.0
        if G == 1:
            assert _bytes(torch.from_numpy(got[4:])) == _bytes(torch.zeros(1, dtype=torch.float64)), tag
        else:
            worst_d = max(worst_d, _within(tag + " DifferentialFairness", got[4:], ref[4:], bound[4:]))
    print(f"fair_from_stats K={K}: worst error / bound: value-type {worst_v:.3g}, DifferentialFairness {worst_d:.3g}")


def test_differential_fairness_leaves_a_nan_logarithm_out_of_the_maximum():
    """a negative score sum makes a table entry negative: the pairs with it do not enter the item's maximum, the result is
    finite (the oracle returns NaN there, tests/test_metrics_ref.py)"""
    st = R.stats_case_nonpositive()
    ref, bound = R.fair_from_stats_ref(st, 3, _logf_ulp())
    got = _fair(st, 3)
    assert (got[:4] == 0).all()
    _within("DifferentialFairness with a negative table entry", got[4:], ref[4:], bound[4:])


# ---- the chain: fairrec.evaluator.fairness_metrics ----------------------------------------------------------------------------------

@pytest.mark.parametrize("neg_len", [120, 500])
def test_fairness_metrics_chain(neg_len):
    """40 items, a binary attribute (the value-type metrics) and a three-valued one (the population-std branch of NonParity),
    negatives shorter and longer than the 300 positives: both sides of min(len(neg), P)"""
    from fairrec.evaluator import fairness_metrics
    z = R.chain_case(neg_len)
    d = lambda k: torch.from_numpy(z[k]).cuda()
    got = fairness_metrics(d("pos_score"), d("pos_i"), {"gender": d("gender"), "age": d("age")}, d("neg_score"), d("neg_i"),
                           "uni100")
    ref, bound = R.fairness_ref(z["pos_score"], z["pos_i"], {"gender": z["gender"], "age": z["age"]}, z["neg_score"],
                                z["neg_i"], "uni100", logf_ulp=_logf_ulp())
    assert set(got) == set(ref) and len(ref) == 8
    keys = sorted(ref)
    assert all(ref[k] > 0 for k in keys)
    _within(f"fairness_metrics, {neg_len} negatives", [got[k] for k in keys], [ref[k] for k in keys], [bound[k] for k in keys])


# ---- the same bits on every call ----------------------------------------------------------------------------------------------------

def test_results_are_bit_reproducible():
    rec, _ = _topk_ref(129, 20)
    assert _bytes(_topk(rec)) == _bytes(_topk(rec))
    idx, pu, pi = R.eval_hits_case(125, 7, 1000, "many")
    keys = R.pos_keys(1000, pu, pi)
    assert _hits(idx, 1000, keys).tobytes() == _hits(idx, 1000, keys).tobytes()
    case = R.group_sums_case(40, 3, "cancel", True, "floats")
    assert _gsums(*case, 3).tobytes() == _gsums(*case, 3).tobytes()
    for G in (2, 8):
        st = R.stats_case(600, G)
        assert _fair(st, G).tobytes() == _fair(st, G).tobytes()


# ---- bad arguments: the error code, fr_last_error, nothing written -------------------------------------------------------------------

def test_topk_metrics_refuses_bad_arguments():
    lib, f = _lib(), _Frames()
    U, K = 65, 3
    rec = _dev(R.topk_case(U, K))
    out = f.new(torch.float64, 6, K)
    need = lib.fr_topk_metrics_workspace_bytes(U, K)
    ws = f.ws(need)
    good = [rec.data_ptr(), U, K, out.data_ptr(), ws.data_ptr(), need]
    for pos, bad in ((0, 0), (3, 0), (4, 0), (1, 0), (1, -1), (2, 0), (2, -1), (5, need - 1), (5, 0)):
        args = list(good)
        args[pos] = bad
        ok, why = _refused(lib.fr_topk_metrics(*args, _st()), "fr_topk_metrics")
        assert ok and f.intact() and _untouched(out) and _untouched(ws), (pos, bad, why)
    assert lib.fr_topk_metrics_workspace_bytes(0, K) == 0 and lib.fr_topk_metrics_workspace_bytes(U, 0) == 0
    assert lib.fr_topk_metrics(*good, _st()) == 0 and f.intact() and not _untouched(out)


def test_eval_hits_refuses_bad_arguments():
    lib, f = _lib(), _Frames()
    idx, pu, pi = R.eval_hits_case(51, 4, 1000, "many")
    keys = _dev(R.pos_keys(1000, pu, pi))
    idx_ = _dev(idx)
    rec = f.new(torch.int32, 51, 5)
    good = [idx_.data_ptr(), 51, 4, 1000, keys.data_ptr(), keys.numel(), rec.data_ptr()]
    for pos, bad in ((0, 0), (6, 0), (4, 0), (1, 0), (2, 0), (3, 0), (5, -1), (1, -1)):
        args = list(good)
        args[pos] = bad
        ok, why = _refused(lib.fr_eval_hits(*args, _st()), "fr_eval_hits")
        assert ok and f.intact() and _untouched(rec), (pos, bad, why)
    assert lib.fr_eval_hits(*good, _st()) == 0 and f.intact() and not _untouched(rec)


def test_group_sums_refuses_bad_arguments():
    lib, f = _lib(), _Frames()
    perm, seg, group, value, wtrue = (_dev(x) for x in R.group_sums_case(17, 8, "mixed", True, "floats"))
    stats = f.new(torch.float64, 17, 8, 3)
    good = [perm.data_ptr(), seg.data_ptr(), 17, group.data_ptr(), value.data_ptr(), wtrue.data_ptr(), 8, stats.data_ptr()]
    for pos, bad in ((1, 0), (3, 0), (4, 0), (7, 0), (2, 0), (2, -1), (6, 0), (6, 9), (6, -1)):
        args = list(good)
        args[pos] = bad
        ok, why = _refused(lib.fr_group_sums(*args, _st()), "fr_group_sums")
        assert ok and f.intact() and _untouched(stats), (pos, bad, why)
    assert lib.fr_group_sums(*good, _st()) == 0 and f.intact() and not _untouched(stats)


def test_fair_metrics_from_stats_refuses_bad_arguments():
    lib, f = _lib(), _Frames()
    K = 257
    st = _dev(R.stats_case(K, 2))
    out = f.new(torch.float64, 5)
    need = lib.fr_fair_metrics_workspace_bytes(K)
    ws = f.ws(need)
    good = [st.data_ptr(), K, 2, out.data_ptr(), ws.data_ptr(), need]
    for pos, bad in ((0, 0), (3, 0), (4, 0), (1, 0), (1, -1), (2, 0), (2, 9), (5, need - 1), (5, 0)):
        args = list(good)
        args[pos] = bad
        ok, why = _refused(lib.fr_fair_metrics_from_stats(*args, _st()), "fr_fair_metrics_from_stats")
        assert ok and f.intact() and _untouched(out) and _untouched(ws), (pos, bad, why)
    assert lib.fr_fair_metrics_workspace_bytes(0) == 0
    assert lib.fr_fair_metrics_from_stats(*good, _st()) == 0 and f.intact() and not _untouched(out)

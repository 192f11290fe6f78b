"""CPU: tests/focf_ref.py -- the float64 reference the FOCF step forms are compared with -- against oracle.focf.loss run on
float64 tensors under torch autograd (which fixes the kink semantics by torch, not by anybody's reading), the conditions its
builders promise, and the measurement behind the tolerance constants: the reference's own float32 arithmetic (oracle.focf in
float32, torch autograd, torch.optim.Adam) against float64 on the builders' inputs, printed and asserted against
focf_ref.MEASURED."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import focf_ref as R
from oracle import focf as O

U = R.U
FW = R.FAIR_WEIGHT
CASES = [(name, D) for name, widths in R.BUILDER_WIDTHS.items() for D in widths]


def _t(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype)


def _oracle(objective, b, cols, dtype):
    """oracle.focf.loss + autograd in `dtype` -> (loss, mse, fair, pred, gradU, gradI)"""
    user, item, rating, sst = cols
    Ut, It = _t(b.U, dtype).requires_grad_(), _t(b.I, dtype).requires_grad_()
    u, i, r, s = _t(user, torch.int64), _t(item, torch.int64), _t(rating, dtype), _t(sst, dtype)
    loss, pred = O.loss(objective, FW, Ut, It, u, i, r, s)
    loss.backward()
    with torch.no_grad():
        mse = F.mse_loss(pred, r)
        fair = O.fairness_term(objective, pred, r, s, i) if objective != "none" else torch.zeros((), dtype=dtype)
    return float(loss.detach()), float(mse), float(fair), pred.detach().numpy(), Ut.grad.numpy(), It.grad.numpy()


def _rel(a, b, bound, rtol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert (np.abs(a - b) <= rtol * (np.abs(b) + bound)).all(), float(np.abs(a - b).max())


@pytest.mark.parametrize("objective", R.OBJECTIVES)
@pytest.mark.parametrize("name,D", CASES, ids=[f"{n}-{D}" for n, D in CASES])
def test_focf_loss_is_the_oracle_in_double_under_autograd(name, D, objective):
    for b in R.batches(name, D):
        for contiguous in (False, True):
            cols = b.cols(contiguous)
            r = R.reference(b, objective, contiguous)
            if objective == "nonparity" and not R.two_groups(b):
                with pytest.raises(IndexError):                  # the reference itself raises; the kernels report fair = 0
                    _oracle(objective, b, cols, torch.float64)
                assert r.fair == 0.0 and r.loss == r.mse
                continue
            loss, mse, fair, pred, gU, gI = _oracle(objective, b, cols, torch.float64)
            _rel(r.mse, mse, 0.0)
            # (nonparity: the two group means may cancel; sl1'(z) (|a| + |b|) is what their rounding carries into the term)
            z = r.gmean if objective == "nonparity" else np.zeros(2)
            _rel(r.fair, fair, min(abs(z[0] - z[1]), 1.0) * np.abs(z).sum())
            _rel(r.loss, loss, FW * min(abs(z[0] - z[1]), 1.0) * np.abs(z).sum())
            ue, ie = np.abs(b.U.astype(np.float64)[cols[0]]), np.abs(b.I.astype(np.float64)[cols[1]])
            ppos = (ue * ie).sum(-1)
            _rel(r.pred, pred, ppos)
            # relative to the entry's bound A, and to what the rounding of pred itself (relative to sum |u i|) carries into
            # dLoss/dpred where pred - rating cancels: its slope in pred is at most 2 / B + fair_weight / K
            slope = (2.0 / b.B + FW / (len(r.rows_i) if objective in R.PER_ITEM else 1.0)) * ppos
            EU, EI = np.zeros_like(r.AU), np.zeros_like(r.AI)
            np.add.at(EU, cols[0], slope[:, None] * ie)
            np.add.at(EI, cols[1], slope[:, None] * ue)
            _rel(r.gradU, gU, r.AU + EU)
            _rel(r.gradI, gI, r.AI + EI)
            _rel(r.norm, np.sqrt((gU ** 2).sum() + (gI ** 2).sum()), 0.0)
            assert (r.AU >= np.abs(r.gradU) * (1 - 1e-14)).all() and (r.AI >= np.abs(r.gradI) * (1 - 1e-14)).all()
            outside = np.setdiff1d(np.arange(b.U.shape[0]), r.rows_u)
            assert not r.gradU[outside].any() and not gU[outside].any()


def test_the_kink_the_kernels_must_take_as_torch_does():
    """one item, a group-0 member whose pred equals its rating (3), a group-1 member with pred 3 and
    rating 5; under `under` the first member's user row gets a gradient from torch's clamp (mask x >= min), none from x > 0"""
    Ut = np.zeros((2, 4), np.float32)
    It = np.zeros((1, 4), np.float32)
    Ut[:, 1], It[0, 1] = 1.5, 2.0
    cols = (np.array([0, 1]), np.array([0, 0]), np.array([3.0, 5.0], np.float32), np.array([0.0, 1.0], np.float32))
    r = R.focf_loss("under", FW, Ut, It, *cols)
    b = R.Batch("issue", Ut, It, *cols)
    g = _oracle("under", b, cols, torch.float64)[4]
    # |delta| = 2 / 1.00001 > 1: d fair / d P_0 = (-1) (-1), through 1 / (1 + 1e-5) and the item row's 2.0
    assert r.P[0, 0] == r.T[0, 0] and g[0, 1] == pytest.approx(FW * 2.0 / (1 + 1e-5), rel=1e-12)
    assert r.gradU[0, 1] == pytest.approx(g[0, 1], rel=1e-12)
    assert R.focf_loss("absolute", FW, Ut, It, *cols).gradU[0, 1] == 0.0
    assert _oracle("absolute", b, cols, torch.float64)[4][0, 1] == 0.0


@pytest.mark.parametrize("name,D", CASES, ids=[f"{n}-{D}" for n, D in CASES])
def test_builders_keep_their_promises(name, D):
    bs = R.batches(name, D)
    for b in bs:
        assert b.U.dtype == np.float32 and b.U.shape[1] == D == b.I.shape[1] and b.U.shape[0] <= 800 and b.I.shape[0] <= 800
        u, i, _, _ = b.cols(True)
        assert len(np.unique(i)) == 1 + int((np.diff(i) != 0).sum())            # item-contiguous
        us, is_, rs, ss = b.cols(False)
        assert sorted(zip(us.tolist(), is_.tolist(), rs.tolist(), ss.tolist())) == sorted(zip(*[c.tolist() for c in b.cols(True)]))
    b = bs[0]
    if name == "segments":
        lengths = b.seg_lengths().tolist()
        assert all(n in lengths for n in R.SEGMENT_LENGTHS) and len(lengths) > 64
        assert set(R.USER_SEGMENTS) <= set(np.unique(b.user, return_counts=True)[1].tolist())
        pc = np.unique(np.stack([b.user, b.item]), axis=1, return_counts=True)[1]
        assert (pc == 2).sum() == 1 and pc.max() == 2
        for it, n in zip(*np.unique(b.item, return_counts=True)):
            if n in R.SEGMENT_LENGTHS and n >= 2:
                assert len(np.unique(b.sst[b.item == it])) == 2
    elif name == "one_sided":
        r = R.reference(b, "value", True)
        for g in (0, 1):
            alone = (r.n[:, 1 - g] == 0)
            assert sorted(set(r.n[alone, g].tolist())) == [1, 2, 5, 17, 70]
            assert (r.P[alone, 1 - g] == 0).all() and (r.T[alone, 1 - g] == 0).all()
        assert ((r.n > 0).all(1)).sum() >= 10
    elif name == "encodings":
        assert [np.unique(x.sst).tolist() for x in bs] == [[0, 1], [1, 2], [-1, 0.5], [0], [1], [0, 1]]
        assert (bs[5].sst == 0).sum() == 1
        r = R.reference(bs[5], "nonparity", True)
        assert r.fair > 0
        # the coding does not matter, only which value is the smaller one
        a, c = R.reference(bs[0], "under", True), R.reference(bs[1], "under", True)
        assert a.loss == c.loss and np.array_equal(a.gradU, c.gradU)
    elif name == "regimes":
        for obj in R.PER_ITEM:
            r = R.reference(b, obj, True)
            assert not R._regime_bad(r).any()
            assert (np.abs(r.P - r.T) >= R.MARGIN).all() and (np.abs(r.delta) >= R.MARGIN).all()
            assert (np.abs(np.abs(r.delta) - 1) >= R.MARGIN).all()
            cells = R._regime_cells(r)
            assert len(cells) == 8 and min(cells.values()) >= R.REGIME_CELL, (obj, cells)
    elif name == "exact_kinks":
        assert len(b.on_kink) and len(b.zero_fair)
        for obj in R.PER_ITEM:
            r = R.reference(b, obj, True)
            rn = R.reference(b, "none", True)
            assert np.array_equal(r.dpred[b.zero_fair], rn.dpred[b.zero_fair])       # (b): the fairness gradient is exactly 0
            kinds = [b.kind[int(it)] for it in r.items]
            for j, kd in enumerate(kinds):
                if kd.startswith("a_"):
                    g = int(kd[-1])
                    assert r.P[j, g] == r.T[j, g]
        # (a): under `under` / `over` the members on the kink get a fairness gradient in the items made for that objective
        for obj in ("under", "over"):
            r, rn = R.reference(b, obj, True), R.reference(b, "none", True)
            item = b.cols(True)[1]
            mine = np.array([b.kind[int(item[p])].split("_")[1] == obj for p in b.on_kink])
            assert mine.sum() >= 4 and (r.dpred[b.on_kink][mine] != rn.dpred[b.on_kink][mine]).all()
            assert (r.dpred[b.on_kink][~mine] == rn.dpred[b.on_kink][~mine]).all()
        r, rn = R.reference(b, "absolute", True), R.reference(b, "none", True)
        assert (r.dpred[b.on_kink] == rn.dpred[b.on_kink]).all()                        # abs'(0) = 0
    elif name == "counts":
        assert [(x.B, len(np.unique(x.item))) for x in bs] == list(R.COUNTS)
        assert {x.B for x in bs} == {1, 2, 3, 5, 1025} and {1, 63, 64, 65, 129} <= {len(np.unique(x.item)) for x in bs}
        assert (1025 + 3) // 4 == 257


def test_adam_first_step_and_predict():
    g = np.array([0.5, -2.0, 0.0])
    m, v = R.adam_first_step(g)
    p = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=1e-3, weight_decay=0.0)
    p.grad = torch.tensor(g)
    opt.step()
    np.testing.assert_allclose(m, opt.state[p]["exp_avg"].numpy(), rtol=1e-15)
    np.testing.assert_allclose(v, opt.state[p]["exp_avg_sq"].numpy(), rtol=1e-15)
    np.testing.assert_allclose(m / (1 - R.B1), g, rtol=1e-15)
    for D in R.FRAGMENT_WIDTHS:
        b = R.batches("segments", D)[0]
        u, i, _, _ = b.cols(False)
        for scale in (1.0, -1.0, 3.0):                  # interior, below 0, above the maximum
            Us = b.U * np.float32(scale)
            ref = O.predict(_t(Us, torch.float64), _t(b.I, torch.float64), _t(u, torch.int64), _t(i, torch.int64), 5.0).numpy()
            got = R.predict(Us, b.I, u, i, 5.0)
            np.testing.assert_allclose(got, ref, rtol=1e-13, atol=1e-15)
            assert got.min() >= 0 and got.max() <= 1 and (scale != -1.0 or (got == 0).any()) and (scale != 3.0 or (got == 1).any())


def _units(got, ref, unit):
    got, ref, unit = (np.asarray(x, dtype=np.float64) for x in (got, ref, unit))
    err = np.abs(got - ref)
    ok = unit > 0
    assert (err[~ok] == 0).all(), "an error where the unit is zero"
    return float((err[ok] / unit[ok]).max()) if ok.any() else 0.0


def test_measure_the_float32_reference_against_float64(capsys):
    """the constants of focf_ref.MEASURED: the reference's float32 arithmetic, never a kernel"""
    worst = dict.fromkeys(R.MEASURED, 0.0)
    for name, D in CASES:
        for b in R.batches(name, D):
            for objective in R.OBJECTIVES:
                if objective == "nonparity" and not R.two_groups(b):
                    continue
                cols = b.cols(False)
                r = R.reference(b, objective, False)
                l32, mse32, fair32, _, _, _ = _oracle(objective, b, cols, torch.float32)
                out = O.train(objective, b.U, b.I, *[c[None] for c in cols], lr=1e-3, wd=0.0, fair_weight=FW, snaps=(1,),
                              clip_max_norm=1e30)
                w = lambda q: f"{q}_{name}"
                worst[w("loss")] = max(worst[w("loss")], _units(l32, r.loss, U * (abs(r.loss) + r.mse + FW * r.fair)))
                worst[w("mse")] = max(worst[w("mse")], _units(mse32, r.mse, U * 2 * r.mse))
                worst[w("fair")] = max(worst[w("fair")], _units(fair32, r.fair, U * 2 * r.fair))
                worst[w("norm")] = max(worst[w("norm")], _units(out["grad_norm"][0], r.norm, U * r.norm))
                for tag, g, A in (("U", r.gradU, r.AU), ("I", r.gradI, r.AI)):
                    worst[w("grad")] = max(worst[w("grad")], _units(out[f"grad{tag}_step1"], g, U * A))
                    m, v = R.adam_first_step(g)
                    worst[w("m")] = max(worst[w("m")], _units(out[f"m{tag}_after1"] / (1 - R.B1), g, U * A))
                    # v is not measured: its bound follows from the gradient's, and holds for the float32 reference
                    tol_v = R.v_tolerance(g, R.tol_const(w("m")) * U * A)
                    assert (np.abs(out[f"v{tag}_after1"] - v) <= tol_v).all(), (name, D, objective, tag)
    with capsys.disabled():
        for key, w in worst.items():
            print(f"\nfocf_ref measurement {key}: the float32 reference's worst error {w:.4g} units (recorded {R.MEASURED[key]})")
    for key, w in worst.items():
        assert w <= R.MEASURED[key], f"{key}: the float32 reference errs by {w:.4g} units, recorded {R.MEASURED[key]}"
        assert w >= 0.5 * R.MEASURED[key] or R.MEASURED[key] == R.FLOOR, f"{key}: recorded {R.MEASURED[key]} is no measurement ({w:.4g})"

"""CPU: tests/loss_ref.py -- the float64 references the loss kernel tests compare with -- against torch float64 autograd of the
literal expressions, the conditions its input builders promise at every size the GPU file uses, and the measurement behind the
tolerance constants: the float32 restatement of the kernels' formulas against float64 on those inputs (printed, and asserted
against loss_ref.MEASURED)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_ref as R
from oracle import nfcf as ON
from oracle import pfcn as OP

U = R.U
# the sizes tests/test_loss_kernels_hip.py runs the builders at
REGIME_SQUARE = [17, 64, 255, 257, 300]
REGIME_RECT = [(257, 31), (100, 300)]
DF_B = [1, 17, 256, 257, 1000]
CE_M, CE_C, CE_SHIFT = [1, 255, 256, 257], [1, 2, 3, 64], [0.0, 100.0, -100.0, 1e4, -1e4]


def _close(a, b, rtol=1e-12, atol=0.0):
    np.testing.assert_allclose(torch.as_tensor(a).detach().numpy(), torch.as_tensor(b).detach().numpy(), rtol=rtol, atol=atol)


# ---- references against autograd ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R_", [1, 2, 3])
def test_rowdot_references_are_autograd_of_mul_sum(R_):
    g = torch.Generator().manual_seed(R_)
    A, D = 5, 65
    a = torch.randn(A, D, generator=g)
    b = torch.randn(R_ * A, D, generator=g)
    go = torch.randn(R_ * A, generator=g)
    a64, b64 = a.double().requires_grad_(), b.double().requires_grad_()
    out = (a64.repeat(R_, 1) * b64).sum(-1)
    out.backward(go.double())
    ref, ab = R.rowdot_rep(a, b, R_)
    _close(ref, out)
    _close(ab, (a.double().repeat(R_, 1) * b.double()).abs().sum(-1))
    da, db, absda = R.rowdot_rep_bwd(go, a, b, R_)
    _close(da, a64.grad)
    _close(db, b64.grad)
    sep, db2 = R.rowdot_rep_bwd_sep(go, a, b, R_)
    _close(sep.view(R_, A, D).sum(0), a64.grad)
    _close(db2, b64.grad)
    assert bool((absda >= da.abs() * (1 - 1e-15)).all())
    if R_ == 1:
        p, pab = R.rowdot(a, b)
        assert torch.equal(p, ref) and torch.equal(pab, ab)
        pda, pdb = R.rowdot_bwd(go, a, b)
        assert torch.equal(pda, da) and torch.equal(pdb, db)


def test_bpr_reference_is_autograd_of_the_literal_expression():
    pos = torch.tensor([0.3, -1.0, 20.0, -20.0, 50.0, -50.0, 100.0, -100.0, 150.0, -150.0, -200.0])
    neg = torch.zeros_like(pos)
    p64, n64 = pos.double().requires_grad_(), neg.double().requires_grad_()
    (-torch.log(1e-10 + torch.sigmoid(p64 - n64))).mean().backward()
    loss, dpos, dneg = R.bpr(pos, neg)
    _close(loss, (-torch.log(1e-10 + torch.sigmoid(pos.double()))).mean())
    # autograd forms 1 - sigmoid(x), which is 0 from x = 37 on; the reference's sigmoid(-x) is e^-x there: below 1e-16 / B
    _close(dpos, p64.grad, rtol=1e-9, atol=1e-17)
    _close(dneg, n64.grad, rtol=1e-9, atol=1e-17)
    assert bool(torch.isfinite(dpos).all()) and float(dpos[-1]) < 0 and float(dpos[-1]) > -1e-70     # x = -200: about -1e-78


@pytest.mark.parametrize("Na,Nc", [(1, 1), (5, 3), (33, 17)])
def test_bpr_outer_reference_is_autograd_and_the_oracle(Na, Nc):
    g = torch.Generator().manual_seed(Na)
    a, c = torch.randn(Na, generator=g) * 3, torch.randn(Nc, generator=g) * 3
    inv = 1.0 / (Na * Nc)
    a64, c64 = a.double().requires_grad_(), c.double().requires_grad_()
    l = (-torch.log(1e-10 + torch.sigmoid(a64[None, :] + c64[:, None]))).mean()
    l.backward()
    loss, da, dc = R.bpr_outer_rect(a, c, inv)
    _close(loss, l)
    _close(da, a64.grad, rtol=1e-10)
    _close(dc, c64.grad, rtol=1e-10)
    if Na == Nc:
        ol, oda, odc = OP.bpr_outer(a, c)
        _close(loss, ol)
        _close(da, oda, rtol=1e-10)
        _close(dc, odc, rtol=1e-10)


@pytest.mark.parametrize("shift", [0.0, -1e4])
def test_softmax_ce_reference_is_autograd_of_cross_entropy(shift):
    z, y = R.softmax_logits(7, 5, shift)
    z64 = z.double().requires_grad_()
    l = F.cross_entropy(z64, y)
    l.backward()
    loss, dz = R.softmax_ce(z, y)
    assert bool(torch.isinf(z).any())
    _close(loss, l)
    _close(dz, z64.grad, atol=1e-18)


def test_nfcf_reference_is_autograd_of_bce_and_the_oracle_df():
    b = R.df_batch(257, 400)
    y, label, sst, item = (torch.from_numpy(x) for x in (b.y, b.label, b.sst, b.item))
    fw = 0.37
    y64 = y.double().requires_grad_()
    o = torch.sigmoid(y64)
    bce = F.binary_cross_entropy(o, label.double())
    df = ON.differential_fairness(o, label.double(), sst.double(), item)
    (bce + fw * df).backward()
    r = R.nfcf_loss(y, label, sst, item, fw)
    _close(r.out, o)
    _close(r.loss, torch.stack([bce + fw * df, bce, df]), rtol=1e-11)
    # rows whose float64 sigmoid is 1 to the last bit: autograd's BCE gradient is torch's clamped one, the reference's rule too
    _close(r.dy, y64.grad, rtol=1e-9, atol=1e-18)
    assert r.K == len(torch.unique(item[label == 1]))
    bce_only = R.nfcf_loss(y, label)
    _close(bce_only.loss, torch.stack([bce, bce, torch.zeros(())]).detach())
    assert torch.equal(bce_only.dy, r.dy_bce)


def test_nfcf_reference_without_two_groups_or_without_positives_has_no_df():
    b = R.df_batch(64, 100)
    one = R.nfcf_loss(b.y, b.label, np.ones_like(b.sst), b.item, 0.5)
    none = R.nfcf_loss(b.y, np.zeros_like(b.label), b.sst, b.item, 0.5)
    for r in (one, none):
        assert float(r.loss[2]) == 0.0 and not bool(r.dy_df.any()) and float(r.loss[0]) == float(r.loss[1])
    assert none.K == 0 and one.K > 0


# ---- builders ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Na,Nc", [(B, B) for B in REGIME_SQUARE] + REGIME_RECT)
def test_bpr_regimes_hold_and_the_reference_is_finite_there(Na, Nc):
    a, c = R.bpr_regimes(Na, Nc)                   # asserts its regimes itself
    assert a.dtype == np.float32 and c.dtype == np.float32 and a.shape == (Na,) and c.shape == (Nc,)
    loss, da, dc = R.bpr_outer_rect(a, c, 1.0 / (Na * Nc))
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(da).all()) and bool(torch.isfinite(dc).all())
    # the largest gradient belongs to a benign column / row, so the absolute term of the tolerance is the benign part's
    assert abs(a[int(da.abs().argmax())]) < 8 and abs(c[int(dc.abs().argmax())]) < 8
    with pytest.raises(AssertionError):
        R.bpr_regimes(13, 40)


def test_the_unclamped_slow_path_is_not_a_number_below_minus_88_7():
    """the defect the kernel had: exp(-x) = inf gives r = 0 and r r e = 0 * inf; held at FLT_MAX it is a plain -0"""
    a, c = R.bpr_regimes(64)
    _, da, dc = R.f32_bpr_outer_rect(a, c, 1.0 / 64 ** 2, clamp=False)
    assert bool(torch.isnan(da).any()) and bool(torch.isnan(dc).any())
    loss, da, dc = R.f32_bpr_outer_rect(a, c, 1.0 / 64 ** 2)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(da).all()) and bool(torch.isfinite(dc).all())


@pytest.mark.parametrize("B", DF_B)
def test_df_batch_holds_its_structures(B):
    n_items = B + 50
    b = R.df_batch(B, n_items)
    assert all(x.shape == (B,) for x in (b.y, b.label, b.sst, b.item))
    assert set(np.unique(b.label)) <= {0.0, 1.0} and set(np.unique(b.sst)) <= {1.0, 2.0}
    assert b.item.min() >= 0 and b.item.max() < n_items and (b.y >= 0).all()
    r = R.nfcf_loss(b.y, b.label, b.sst, b.item, 0.5)
    assert bool(torch.isfinite(r.loss).all()) and bool(torch.isfinite(r.dy).all())
    for it in r.items:                                     # the reference alone keeps every log ratio away from rounding
        assert (it.d == 0.0 and it.item == b.zero_item) or abs(it.d) >= R.DF_MIN_LOG_RATIO
    ids, counts = np.unique(b.item, return_counts=True)
    if B >= R.DF_FULL_B:
        assert b.has == {"zero", "single", "no_positive", "one_group", "every_length_mod_16", "hot"}
        assert set(counts % 16) == set(range(16)) and counts.max() > 16 * 6 and (counts == 1).sum() >= 3
        assert (b.y == 0).any() and (b.y >= 20).any()
        counted = {it.item: it for it in r.items}
        assert any(min(it.n) == 0 for it in r.items), "no item whose positives are all of one group"
        assert any(not (b.label[b.item == k] == 1).any() for k in ids), "no item without a positive row"
        z = counted[b.zero_item]
        assert z.n == [1, 1] and z.d == 0.0
        assert not bool(r.dy_df[torch.from_numpy(b.item == b.zero_item)].any())
        assert 0 in ids and n_items - 1 in ids
    if B >= 2:
        assert "zero" in b.has


def test_softmax_logits_hold_their_cases():
    for C in CE_C:
        z, y = R.softmax_logits(257, C, 1e4)
        assert z.dtype == torch.float32 and set(y.tolist()) == set(range(C))
        assert int(torch.isinf(z).sum()) == (1 if C >= 2 else 0)
        assert not bool(torch.isinf(z[torch.arange(257), y]).any())
        loss, dz = R.softmax_ce(z, y)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(dz).all())


# ---- the measurement behind the tolerance constants --------------------------------------------------------------------------

def _units(got, ref, unit):
    return float(((got.double() - ref).abs() / unit).max())


def _record(worst):
    """print every figure, then hold each to the recorded constant: not above it, and the record within twice of it"""
    for key, w in worst.items():
        print(f"\nloss_ref measurement {key}: float32 restatement's worst error {w:.4g} units (recorded {R.MEASURED[key]})")
    for key, w in worst.items():
        assert w <= R.MEASURED[key], f"{key}: the float32 restatement errs by {w:.4g} units, recorded {R.MEASURED[key]}"
        assert w >= 0.5 * R.MEASURED[key], f"{key}: recorded {R.MEASURED[key]} is no measurement ({w:.4g})"


def test_measure_bpr_in_the_saturated_regimes():
    worst = {"bpr_loss": 0.0, "bpr_da": 0.0, "bpr_dc": 0.0}
    for Na, Nc in [(B, B) for B in REGIME_SQUARE] + REGIME_RECT:
        a, c = R.bpr_regimes(Na, Nc)
        inv = 1.0 / (Na * Nc)
        loss, da, dc = R.bpr_outer_rect(a, c, inv)
        l32, da32, dc32 = R.f32_bpr_outer_rect(a, c, inv)
        worst["bpr_loss"] = max(worst["bpr_loss"], _units(l32, loss, R.LOSS_REL * loss.abs()))
        worst["bpr_da"] = max(worst["bpr_da"], _units(da32, da, R.GRAD_REL * da.abs() + R.GRAD_ABS * da.abs().max()))
        worst["bpr_dc"] = max(worst["bpr_dc"], _units(dc32, dc, R.GRAD_REL * dc.abs() + R.GRAD_ABS * dc.abs().max()))
    _record(worst)


BPR_B = [255, 256, 257, 1000]       # the sizes of the GPU file that hold the extremes (B = 1 runs them one by one)


def test_measure_the_plain_bpr_with_its_extremes():
    worst = {"bprp_loss": 0.0, "bprp_d": 0.0}
    cases = [R.bpr_columns(B) for B in BPR_B]
    for pos, neg in cases:
        assert set(R.BPR_EXTREMES) <= set((pos.astype(np.float64) - neg).tolist())
        loss, dpos, dneg = R.bpr(pos, neg)
        l32, d32, n32 = R.f32_bpr(pos, neg)
        assert bool(torch.isfinite(dpos).all()) and torch.equal(n32, -d32)
        worst["bprp_loss"] = max(worst["bprp_loss"], _units(l32, loss, R.LOSS_REL * loss.abs()))
        worst["bprp_d"] = max(worst["bprp_d"], _units(d32, dpos, R.GRAD_REL * dpos.abs() + R.GRAD_ABS * dpos.abs().max()))
    _record(worst)


def test_measure_softmax_ce():
    worst = {"ce_loss": 0.0, "ce_dlogits": 0.0}
    before = 0.0
    for M in CE_M:
        for C in CE_C:
            for shift in CE_SHIFT:
                z, y = R.softmax_logits(M, C, shift)
                loss, dz = R.softmax_ce(z, y)
                l32, dz32 = R.f32_softmax_ce(z, y)
                worst["ce_loss"] = max(worst["ce_loss"], _units(l32, loss, U * loss.abs() + U))
                worst["ce_dlogits"] = max(worst["ce_dlogits"], _units(dz32, dz, U * (dz.abs() + dz.abs().max())))
                if abs(shift) == 1e4 and C >= 2:
                    old, _ = R.f32_softmax_ce(z, y, fixed=False)
                    before = max(before, _units(old, loss, U * loss.abs() + U))
    _record(worst)
    # the kernel that added the maximum back before subtracting z[y] is off by ulp(1e4) / 2 = 5e-4: thousands of units
    print(f"lse = mx + log(se) at a shift of 1e4: {before:.4g} units")
    assert before > 100 * R.tol_const("ce_loss")


def test_measure_the_df_term():
    worst = {"df_loss": 0.0, "df_dy": 0.0}
    fw = 0.5
    for B in DF_B:
        b = R.df_batch(B, B + 50)
        r = R.nfcf_loss(b.y, b.label, b.sst, b.item, fw)
        o32, l32, dy32, part32 = R.f32_nfcf_loss(b.y, b.label, b.sst, b.item, fw)
        if not r.items:
            assert float(l32[2]) == 0.0
            continue
        worst["df_loss"] = max(worst["df_loss"], _units(l32[2], r.loss[2], U * r.loss[2].abs() + r.seg_loss))
        over = ((part32.double() - r.dy_df).abs() - r.seg_dy).clamp(min=0.0)
        worst["df_dy"] = max(worst["df_dy"], float((over / (U * (r.dy_df.abs() + r.dy_df.abs().max()))).max()))
        assert bool(torch.isfinite(dy32).all())
    _record(worst)

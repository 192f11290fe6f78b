"""GPU: the loss kernels of csrc/pfcn.hip (row dots, BPR, the [B] + [B, 1] broadcast BPR, softmax cross-entropy) and
fr_nfcf_loss of csrc/nfcf.hip, one by one through the C ABI against the float64 references of tests/loss_ref.py, at the
smallest shapes that reach each edge: one row, the row / wave / block tails, widths that are no multiple of 64, saturated
arguments.  Every output buffer sits between canaries and starts as NaN, every workspace starts as 0xFF bytes (a NaN in every
float), every return code is asserted.

Tolerances (u = 2^-24, gamma_n = n u / (1 - n u)):
  * derived: a row dot is one fmaf chain of ceil(D / 64) steps per lane, six butterfly additions and the reference's own
    rounding: gamma_(ceil(D/64) + 7) * sum |a b|; the summed gradient of the `rep` form gamma_(R+1) * sum_r |g b|; single
    products, negated copies and the identities between entry points are bit for bit;
  * the project's, on benign inputs (test_mlp_hip.py::test_bpr_outer_at_the_baseline_batch): BPR loss 1e-5 relative,
    gradients 1e-4 |ref| + 1e-6 max |ref|; the BCE head: test_scorer_hip._head_ref's per-row tolerances;
    the loss term of a head row with y < 0: 4 u (|y| + 2), derived in NEG_LOSS_TOL (_head_ref's is void for a small o);
  * measured on the reference side, times 8 (loss_ref.MEASURED, asserted by tests/test_loss_ref.py): the worst error of the
    float32 restatement of the kernel's formulas against float64 on the same inputs, in units of the form:
      plain BPR with its extremes   loss 0.004 x 1e-5 |ref|         -> 3.2e-7 |ref|
                                    gradients 0.02 x (1e-4 |ref| + 1e-6 max |ref|) -> 1.6e-5 |ref| + 1.6e-7 max |ref|
      broadcast BPR on bpr_regimes  loss 0.014 x 1e-5 |ref|         -> 1.12e-6 |ref|
                                    da 0.0021, dc 0.002 x (1e-4 |ref| + 1e-6 max |ref|) -> 1.68e-6 |ref| + 1.68e-8 max |ref|
      softmax cross-entropy         loss 2.0 x u (|ref| + 1)        -> 16 u (|ref| + 1)
                                    dlogits 48 x u (|ref| + max |ref|) -> 384 u (|ref| + max |ref|)   (M = 1, C = 3: p - 1 of
                                    a probability near 1 is all there is to compare with)
      differential fairness         loss[2] 0.18 x (u |ref| + segment-sum bound) -> 1.44 x
                                    dy's DF part 2.6 x u (|ref| + max |ref|) -> 20.8 u (|ref| + max |ref|), next to the head's
                                    tolerance, the segment-sum bound and u |dy| for the addition of the two parts
"""
import functools

import numpy as np
import pytest
import torch

import loss_ref as R
from test_scorer_hip import _head_ref

pytestmark = pytest.mark.gpu

U = R.U
CANARY = 1234.5
PAD = 64
EINVAL = -1


def _lib():
    from fairrec import _C
    return _C.lib()


def _st():
    from fairrec import _C
    return _C.current_stream()


def _dev(a):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).cuda()


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _framed(n):
    """(whole, view): `view` = n floats prefilled with NaN, PAD canary floats on either side"""
    whole = torch.full((PAD + n + PAD,), CANARY, dtype=torch.float32, device="cuda")
    view = whole[PAD:PAD + n]
    view.fill_(float("nan"))
    return whole, view


class _Outs:
    """output buffers of one call: each framed, NaN-filled; `ok()` after the call: every frame intact"""

    def __init__(self):
        self.frames = []

    def new(self, *shape):
        n = int(np.prod(shape))
        whole, view = _framed(n)
        self.frames.append((whole, n))
        return view.view(*shape)

    def ok(self):
        torch.cuda.synchronize()
        return all(bool((w[:PAD] == CANARY).all()) and bool((w[PAD + n:] == CANARY).all()) for w, n in self.frames)


def _ws(nbytes):
    return torch.full((max(int(nbytes), 256),), 0xFF, dtype=torch.uint8, device="cuda")


def _errflag():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _bits(a, b):
    """bit-for-bit equality of two float tensors (NaN payloads and the sign of zero included)"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _within(what, got, ref, bound):
    """|got - ref| <= bound element by element, everything finite; prints the largest error / bound"""
    got, ref, bound = (torch.as_tensor(x, dtype=torch.float64).cpu() for x in (got, ref, bound))
    bound = bound.expand_as(ref)
    assert bool(torch.isfinite(got).all()), f"{what}: not finite: {got[~torch.isfinite(got)][:4].tolist()}"
    err = (got - ref).abs()
    bad = ~(err <= bound)
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: largest error / bound {ratio:.3g}")
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} out of bound, first at flat index {i}: got "
                             f"{float(got.reshape(-1)[i])!r}, reference {float(ref.reshape(-1)[i])!r}, bound "
                             f"{float(bound.reshape(-1)[i]):.3g}; largest error / bound {ratio:.3g}")


def _grad_tol(ref, rel, ab):
    ref = torch.as_tensor(ref, dtype=torch.float64)
    return rel * ref.abs() + ab * ref.abs().max()


# ---- A. row dots -------------------------------------------------------------------------------------------------------------

ROWS = [1, 3, 4, 5, 257]
WIDTHS = [1, 63, 64, 65, 128, 200]


def _normals(rng, *shape):
    """magnitudes 0.1 .. 1 with a random sign: no product of two of them is subnormal"""
    return torch.from_numpy((rng.uniform(0.1, 1.0, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32))


def _rowdot_fwd(a, b, reps=None):
    o = _Outs()
    n = b.shape[0]
    out = o.new(n)
    if reps is None:
        rc = _lib().fr_rowdot_fwd(a.data_ptr(), b.data_ptr(), n, a.shape[1], out.data_ptr(), _st())
    else:
        rc = _lib().fr_rowdot_rep_fwd(a.data_ptr(), b.data_ptr(), a.shape[0], reps, a.shape[1], out.data_ptr(), _st())
    assert rc == 0 and o.ok()
    return out.cpu()


def _rowdot_bwd(fn, g, a, b, reps=None, want_da=True, want_db=True, da_rows=None):
    o = _Outs()
    da = o.new(da_rows if da_rows is not None else a.shape[0], a.shape[1]) if want_da else None
    db = o.new(*b.shape) if want_db else None
    head = (g.data_ptr(), a.data_ptr(), b.data_ptr(), a.shape[0]) + (() if reps is None else (reps,)) + (a.shape[1],)
    rc = getattr(_lib(), fn)(*head, _ptr(da), _ptr(db), _st())
    assert rc == 0 and o.ok()
    return (None if da is None else da.cpu()), (None if db is None else db.cpu())


@pytest.mark.parametrize("B", ROWS)
def test_rowdot_forward_and_backward(B):
    for D in WIDTHS:
        rng = np.random.default_rng([B, D])
        a, b, g = _normals(rng, B, D), _normals(rng, B, D), _normals(rng, B)
        da_, db_, g_ = a.cuda(), b.cuda(), g.cuda()
        ref, ab = R.rowdot(a, b)
        _within(f"rowdot_fwd B={B} D={D}", _rowdot_fwd(da_, db_), ref, R.gamma((D + 63) // 64 + 7) * ab)
        da, db = _rowdot_bwd("fr_rowdot_bwd", g_, da_, db_)
        assert _bits(da, g[:, None] * b) and _bits(db, g[:, None] * a), (B, D)      # single float32 products
        only_a, none = _rowdot_bwd("fr_rowdot_bwd", g_, da_, db_, want_db=False)
        none2, only_b = _rowdot_bwd("fr_rowdot_bwd", g_, da_, db_, want_da=False)
        assert none is None and none2 is None and _bits(only_a, da) and _bits(only_b, db), (B, D)


@pytest.mark.parametrize("A", ROWS)
def test_rowdot_rep_forward_and_backward(A):
    for D in WIDTHS:
        for reps in (1, 2, 3):
            rng = np.random.default_rng([A, D, reps])
            a, b, g = _normals(rng, A, D), _normals(rng, reps * A, D), _normals(rng, reps * A)
            a_, b_, g_ = a.cuda(), b.cuda(), g.cuda()
            tag = f"A={A} D={D} R={reps}"
            ref, ab = R.rowdot_rep(a, b, reps)
            out = _rowdot_fwd(a_, b_, reps)
            _within("rowdot_rep_fwd " + tag, out, ref, R.gamma((D + 63) // 64 + 7) * ab)
            rda, rdb, absda = R.rowdot_rep_bwd(g, a, b, reps)
            da, db = _rowdot_bwd("fr_rowdot_rep_bwd", g_, a_, b_, reps)
            _within("rowdot_rep_bwd da " + tag, da, rda, R.gamma(reps + 1) * absda)
            assert _bits(db, g[:, None] * a.repeat(reps, 1)), tag
            sep, sdb = _rowdot_bwd("fr_rowdot_rep_bwd_sep", g_, a_, b_, reps, da_rows=reps * A)
            assert _bits(sep, g[:, None] * b) and _bits(sdb, db), tag
            for fn, full_a, rows in (("fr_rowdot_rep_bwd", da, None), ("fr_rowdot_rep_bwd_sep", sep, reps * A)):
                only_a, _ = _rowdot_bwd(fn, g_, a_, b_, reps, want_db=False, da_rows=rows)
                _, only_b = _rowdot_bwd(fn, g_, a_, b_, reps, want_da=False, da_rows=rows)
                assert _bits(only_a, full_a) and _bits(only_b, db), (fn, tag)
            if reps == 1:       # one row block: the plain form, bit for bit
                pda, pdb = _rowdot_bwd("fr_rowdot_bwd", g_, a_, b_)
                assert _bits(out, _rowdot_fwd(a_, b_)) and _bits(da, pda) and _bits(db, pdb), tag


# ---- B. fr_bpr ---------------------------------------------------------------------------------------------------------------

def _bpr(pos, neg):
    B = len(pos)
    o = _Outs()
    loss, dpos, dneg = o.new(1), o.new(B), o.new(B)
    ws = _ws(_lib().fr_bpr_workspace_bytes(B, 0))
    p_, n_ = _dev(pos), _dev(neg)
    rc = _lib().fr_bpr(p_.data_ptr(), n_.data_ptr(), B, loss.data_ptr(), dpos.data_ptr(), dneg.data_ptr(),
                       ws.data_ptr(), ws.numel(), _st())
    assert rc == 0 and o.ok()
    return loss.cpu(), dpos.cpu(), dneg.cpu()


def _check_bpr(tag, pos, neg, saturated):
    loss, dpos, dneg = _bpr(pos, neg)
    rl, rp, rn = R.bpr(pos, neg)
    cl = R.tol_const("bprp_loss") if saturated else 1.0
    cg = R.tol_const("bprp_d") if saturated else 1.0
    _within(tag + " loss", loss[0], rl, cl * R.LOSS_REL * rl.abs())
    _within(tag + " dpos", dpos, rp, cg * _grad_tol(rp, R.GRAD_REL, R.GRAD_ABS))
    _within(tag + " dneg", dneg, rn, cg * _grad_tol(rn, R.GRAD_REL, R.GRAD_ABS))
    assert _bits(dneg, -dpos), tag


@pytest.mark.parametrize("B", [1, 255, 256, 257, 1000])
def test_bpr_against_float64(B):
    rng = np.random.default_rng(B)
    _check_bpr(f"bpr benign B={B}", rng.standard_normal(B).astype(np.float32), rng.standard_normal(B).astype(np.float32), False)
    if B >= 32:
        pos, neg = R.bpr_columns(B)
        _check_bpr(f"bpr extremes B={B}", pos, neg, True)


def test_bpr_of_one_saturated_row_is_finite():
    """B = 1 with each extreme on its own: nothing benign to scale a tolerance by, so what float32 must give is asserted:
    the loss within the plain relative bound where it is not tiny, a finite gradient no larger than the true one's scale"""
    for x in R.BPR_EXTREMES:
        pos, neg = np.array([0.5 + x], dtype=np.float32), np.array([0.5], dtype=np.float32)
        loss, dpos, dneg = _bpr(pos, neg)
        rl, rp, _ = R.bpr(pos, neg)
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dpos).all()) and _bits(dneg, -dpos), x
        if x < 0:
            _within(f"bpr one row x={x} loss", loss[0], rl, R.tol_const("bprp_loss") * R.LOSS_REL * rl.abs())
            _within(f"bpr one row x={x} dpos", dpos, rp, R.tol_const("bprp_d") * R.GRAD_REL * rp.abs() + 1e-10)
        else:               # loss and gradient of the order of e^-x: below 1e-8, absolutely
            assert abs(float(loss[0]) - float(rl)) <= 1e-7 and abs(float(dpos[0]) - float(rp[0])) <= 1e-7, x


# ---- C. fr_bpr_outer, fr_bpr_outer2, fr_bpr_outer_rect -----------------------------------------------------------------------

SQUARE = [1, 15, 16, 17, 64, 255, 257, 300]
RECT = [(1, 33), (65, 1), (257, 31), (100, 300)]


def _outer(a, c):
    B = len(a)
    o = _Outs()
    loss, da, dc = o.new(1), o.new(B), o.new(B)
    ws = _ws(_lib().fr_bpr_workspace_bytes(B, 1))
    a_, c_ = _dev(a), _dev(c)
    rc = _lib().fr_bpr_outer(a_.data_ptr(), c_.data_ptr(), B, loss.data_ptr(), da.data_ptr(), dc.data_ptr(),
                             ws.data_ptr(), ws.numel(), _st())
    assert rc == 0 and o.ok()
    return loss.cpu(), da.cpu(), dc.cpu()


def _outer2(pos, neg, pb, nb):
    B = len(pos)
    o = _Outs()
    loss, d = o.new(1), [o.new(B) for _ in range(4)]
    ws = _ws(_lib().fr_bpr_workspace_bytes(B, 1))
    cols = [_dev(x) for x in (pos, neg, pb, nb)]
    rc = _lib().fr_bpr_outer2(*(x.data_ptr() for x in cols), B, loss.data_ptr(), *(x.data_ptr() for x in d),
                              ws.data_ptr(), ws.numel(), _st())
    assert rc == 0 and o.ok()
    return (loss.cpu(),) + tuple(x.cpu() for x in d)


def _rect(a, c, inv, want_da=True, want_dc=True):
    Na, Nc = len(a), len(c)
    o = _Outs()
    loss = o.new(1)
    da = o.new(Na) if want_da else None
    dc = o.new(Nc) if want_dc else None
    ws = _ws(_lib().fr_bpr_outer_rect_workspace_bytes(Na, Nc))
    a_, c_ = _dev(a), _dev(c)
    rc = _lib().fr_bpr_outer_rect(a_.data_ptr(), Na, c_.data_ptr(), Nc, inv, loss.data_ptr(), _ptr(da), _ptr(dc),
                                  ws.data_ptr(), ws.numel(), _st())
    assert rc == 0 and o.ok()
    return loss.cpu(), (None if da is None else da.cpu()), (None if dc is None else dc.cpu())


def _check_outer(tag, got, a, c, inv, saturated):
    loss, da, dc = got
    rl, rda, rdc = R.bpr_outer_rect(a, c, inv)
    k = (R.tol_const("bpr_loss"), R.tol_const("bpr_da"), R.tol_const("bpr_dc")) if saturated else (1.0, 1.0, 1.0)
    _within(tag + " loss", loss[0], rl, k[0] * R.LOSS_REL * rl.abs())
    _within(tag + " da", da, rda, k[1] * _grad_tol(rda, R.GRAD_REL, R.GRAD_ABS))
    _within(tag + " dc", dc, rdc, k[2] * _grad_tol(rdc, R.GRAD_REL, R.GRAD_ABS))


def _outer_inputs(Na, Nc):
    cases = [("benign", R.bpr_benign(Na, Nc), False)]
    if Na >= 14 and Nc >= R.OUTER_ROWS + 1:
        cases.append(("regimes", R.bpr_regimes(Na, Nc), True))
    return cases


@pytest.mark.parametrize("B", SQUARE)
def test_bpr_outer_square_against_float64(B):
    inv = float(np.float32(1.0) / (np.float32(B) * np.float32(B)))       # the scale as the entry point forms it
    for name, (a, c), sat in _outer_inputs(B, B):
        tag = f"bpr_outer {name} B={B}"
        got = _outer(a, c)
        _check_outer(tag, got, a, c, inv, sat)
        # the four-column form on (pos, neg, pos_bias, neg_bias): the one-column form on the float32 differences
        # (benign: random second columns, the differences rounded; saturated: zeros, so that the differences ARE the
        # builder's columns and the saturated constants apply to them)
        rng = np.random.default_rng([B, 2])
        neg, nb = (np.zeros(B, dtype=np.float32),) * 2 if sat else \
            (rng.standard_normal(B).astype(np.float32), rng.standard_normal(B).astype(np.float32))
        pos, pb = (a + neg).astype(np.float32), (c + nb).astype(np.float32)
        assert not sat or (np.array_equal(pos - neg, a) and np.array_equal(pb - nb, c))
        loss2, dp, dn, dpb, dnb = _outer2(pos, neg, pb, nb)
        _check_outer(tag + " (outer2)", (loss2, dp, dpb), pos - neg, pb - nb, inv, sat)
        l1, da1, dc1 = _outer(pos - neg, pb - nb)
        assert _bits(loss2, l1) and _bits(dp, da1) and _bits(dpb, dc1), tag
        assert _bits(dn, -dp) and _bits(dnb, -dpb), tag
        # ... and the rectangular entry point with Na = Nc = B and the same scale
        lr, dar, dcr = _rect(a, c, inv)
        assert _bits(lr, got[0]) and _bits(dar, got[1]) and _bits(dcr, got[2]), tag


@pytest.mark.parametrize("Na,Nc", RECT)
def test_bpr_outer_rect_against_float64(Na, Nc):
    inv = 1.0 / 4096.0
    for name, (a, c), sat in _outer_inputs(Na, Nc):
        tag = f"bpr_outer_rect {name} Na={Na} Nc={Nc}"
        loss, da, dc = _rect(a, c, inv)
        _check_outer(tag, (loss, da, dc), a, c, inv, sat)
        la, only_a, none = _rect(a, c, inv, want_dc=False)
        lc, none2, only_c = _rect(a, c, inv, want_da=False)
        assert none is None and none2 is None
        assert _bits(only_a, da) and _bits(only_c, dc) and _bits(la, loss) and _bits(lc, loss), tag


def test_bpr_outer_column_does_not_depend_on_another_columns_path():
    """one benign row block, two calls that differ in ONE column: below 40 (every column on the product-of-exponentials path)
    and at 50 (that column takes the exponential of the sum).  Every other column's gradient is the same bits: which path a
    column takes is decided by the column and the row block alone.  The row gradients sum over the changed column too, so
    they are compared with float64."""
    Na, Nc = 300, 16
    a, c = R.bpr_benign(Na, Nc)
    inv = 1.0 / (Na * Nc)
    k = 7
    a1, a2 = a.copy(), a.copy()
    a1[k], a2[k] = 3.0, 50.0
    assert R.outer_paths(a1, c).all() and not R.outer_paths(a2, c)[:, k].any() and R.outer_paths(a2, c)[:, :k].all()
    l1, da1, dc1 = _rect(a1, c, inv)
    l2, da2, dc2 = _rect(a2, c, inv)
    others = torch.arange(Na) != k
    assert _bits(da1[others], da2[others])
    _check_outer("bpr_outer paths (all fast)", (l1, da1, dc1), a1, c, inv, False)
    _check_outer("bpr_outer paths (one slow column)", (l2, da2, dc2), a2, c, inv, False)


@pytest.mark.parametrize("B", [1, 15, 16])
def test_bpr_outer_single_block_below_minus_88_7_is_finite(B):
    """shapes too small for bpr_regimes: one row block whose last row is c = -100, so every pair of the block takes the
    exponential of the sum and the last row's sums lie below -88.7.  Everything finite; the loss within the project's 1e-5 (the
    saturated row's terms are -log(1e-10) to the rounding of that constant); the saturated row's gradient 0 within the absolute
    term; and at B >= 15, where the benign rows carry a gradient to scale by, da and dc within the project's form."""
    a, c = R.bpr_benign(B)
    c[B - 1] = -100.0
    assert not R.outer_paths(a, c).any() and ((a.astype(np.float64) + c[B - 1]) < -88.7).all()
    inv = float(np.float32(1.0) / (np.float32(B) * np.float32(B)))
    loss, da, dc = _outer(a, c)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(da).all()) and bool(torch.isfinite(dc).all())
    rl, rda, rdc = R.bpr_outer_rect(a, c, inv)
    _within(f"bpr_outer one block B={B} loss", loss[0], rl, R.LOSS_REL * rl.abs())
    assert abs(float(dc[B - 1])) <= 1e-30
    if B >= 15:
        _within(f"bpr_outer one block B={B} da", da, rda, _grad_tol(rda, R.GRAD_REL, R.GRAD_ABS))
        _within(f"bpr_outer one block B={B} dc", dc, rdc, _grad_tol(rdc, R.GRAD_REL, R.GRAD_ABS))


@pytest.mark.parametrize("where", ["a", "c"])
def test_bpr_outer_keeps_a_nan_score_in_the_loss_and_its_gradients(where):
    """a NaN column or row goes down the slow path (no NaN is below 40), where only the OVERFLOW of the exponential is held:
    the loss, the NaN column's da and every dc (each row sums over that column) are NaN; for a NaN row the loss, that row's dc
    and every da.  Divergence is detected by the NaN of the summed loss, so it may not be turned into a finite term."""
    Na, Nc = 40, 33
    a, c = R.bpr_benign(Na, Nc)
    k = 5
    (a if where == "a" else c)[k] = float("nan")
    loss, da, dc = _rect(a, c, 1.0 / (Na * Nc))
    assert bool(torch.isnan(loss).all())
    if where == "a":
        assert bool(torch.isnan(da[k])) and bool(torch.isnan(dc).all())
        assert bool(torch.isfinite(da[torch.arange(Na) != k]).all())
    else:
        assert bool(torch.isnan(dc[k])) and bool(torch.isnan(da).all())
        assert bool(torch.isfinite(dc[torch.arange(Nc) != k]).all())
    loss2, _, _ = _outer(a[:Nc].copy(), c)              # the square entry point: row 5 or column 5 of its 33 x 33 is NaN too
    assert bool(torch.isnan(loss2).all())


# ---- D. fr_softmax_ce --------------------------------------------------------------------------------------------------------

def _softmax_ce(z, y, expect=0):
    M, C = z.shape
    o = _Outs()
    loss, dz = o.new(1), o.new(M, C)
    ws = _ws(((M + 255) // 256) * 4)
    err = _errflag()
    z_, y_ = _dev(z), _dev(y)
    rc = _lib().fr_softmax_ce(z_.data_ptr(), y_.data_ptr(), M, C, loss.data_ptr(), dz.data_ptr(), ws.data_ptr(),
                              ws.numel(), err.data_ptr(), _st())
    assert rc == expect and o.ok()
    return loss.cpu(), dz.cpu(), int(err.item()), ws


def _check_ce(tag, z, y, loss, dz):
    M, C = z.shape
    rl, rdz = R.softmax_ce(z, y)
    _within(tag + " loss", loss[0], rl, R.tol_const("ce_loss") * U * (rl.abs() + 1.0))
    _within(tag + " dlogits", dz, rdz, R.tol_const("ce_dlogits") * U * (rdz.abs() + rdz.abs().max()))
    _within(tag + " row sums", dz.double().sum(1), torch.zeros(M, dtype=torch.float64), torch.tensor(C * U / M))


@pytest.mark.parametrize("shift", [0.0, 100.0, -100.0, 1e4, -1e4])
@pytest.mark.parametrize("M", [1, 255, 256, 257])
def test_softmax_ce_against_float64(M, shift):
    for C in (1, 2, 3, 64):
        z, y = R.softmax_logits(M, C, shift)
        loss, dz, err, _ = _softmax_ce(z, y)
        assert err == 0
        _check_ce(f"softmax_ce M={M} C={C} shift={shift:g}", z, y, loss, dz)


@pytest.mark.parametrize("bad", [-1, "C"])
def test_softmax_ce_flags_a_label_out_of_range_and_scores_class_0(bad):
    from fairrec import _C
    M, C = 257, 3
    z, y = R.softmax_logits(M, C, 0.0)
    y_bad = y.clone()
    y_bad[256] = C if bad == "C" else bad
    loss, dz, err, _ = _softmax_ce(z, y_bad)
    assert err == _C.DEV_ERR_INDEX_RANGE
    y0 = y.clone()
    y0[256] = 0
    _check_ce(f"softmax_ce label {bad}", z, y0, loss, dz)


def test_softmax_ce_refuses_65_classes_before_any_launch():
    z = torch.randn(5, 65)
    y = torch.zeros(5, dtype=torch.int64)
    loss, dz, err, ws = _softmax_ce(z, y, expect=EINVAL)
    assert err == 0 and bool(torch.isnan(loss).all()) and bool(torch.isnan(dz).all()) and bool((ws == 0xFF).all())


# ---- E. fr_nfcf_loss, BCE only -----------------------------------------------------------------------------------------------

def _nfcf(y, label, sst=None, fw=0.0, table=None):
    """fr_nfcf_loss -> out, dy, loss[3], the error word and K as the kernels report it (DF only).  `table`: the item table whose
    training workspace holds the sorted segments of the batch's item ids."""
    lib = _lib()
    B = y.numel()
    o = _Outs()
    out, dy, loss = o.new(B), o.new(B), o.new(3)
    ws = _ws(lib.fr_nfcf_loss_workspace_bytes(B))
    err = _errflag()
    y_, l_ = _dev(y), _dev(label)
    s_ = None if sst is None else _dev(sst)
    iws = None if table is None else table._ws
    rc = lib.fr_nfcf_loss(y_.data_ptr(), l_.data_ptr(), _ptr(s_), B, fw, _ptr(iws), 0 if iws is None else iws.numel(),
                          1 if table is None else table.dim, out.data_ptr(), dy.data_ptr(), loss.data_ptr(), ws.data_ptr(),
                          ws.numel(), err.data_ptr(), _st())
    assert rc == 0 and o.ok()
    K = None
    if table is not None:       # the workspace's layout (csrc/nfcf.hip): bce_part | df_part | kpart | stats | minmax | kout | ..
        up = lambda n: (n + 255) // 256 * 256
        nb, ndf = (B + 255) // 256, (B * 16 + 255) // 256
        off = up(nb * 4) + 2 * up(ndf * 4) + up(B * 16) + 256
        K = float(ws[off:off + 4].view(torch.float32).item())
    return out.cpu(), dy.cpu(), loss.cpu(), int(err.item()), K


def _head_scores(B, kind_):
    """y for the head.  "relu": what the scorer's ReLU lets through: 0, (0, 8), >= 20.  "negative": negatives down to -100 next
    to them; "band": the 15.5 .. 17.5 band where the float32 sigmoid turns to 1.  _head_ref's tolerance of a band row's loss
    is 100 by its own rule, so the mean loss is pinned by the "relu" and "negative" batches (the rows with y < 0 under
    NEG_LOSS_TOL) and the per-row out and dy by all three."""
    band, negative = kind_ == "band", kind_ == "negative"
    g = torch.Generator().manual_seed(B + len(kind_))
    y = torch.rand(B, generator=g) * 8
    kind = torch.rand(B, generator=g)
    y = torch.where(kind < 0.15, torch.zeros(B), y)
    y = torch.where((kind >= 0.15) & (kind < 0.25), 20 + torch.rand(B, generator=g) * 30, y)
    if negative:
        y = torch.where((kind >= 0.25) & (kind < 0.40), -torch.rand(B, generator=g) * 100, y)
    if band:
        y = torch.where((kind >= 0.40) & (kind < 0.50), 15.5 + torch.rand(B, generator=g) * 2, y)
    if B >= 255:
        y[3], y[B - 1], y[64] = (-100.0 if negative else 0.5), 0.0, 25.0
    label = (torch.rand(B, generator=g) < 0.5).float()
    return y, label


def NEG_LOSS_TOL(y):
    """per-row loss bound for y < 0, in place of _head_ref's (which divides the absolute error of an o near 1 by min(o, 1 - o)
    and is void for a small o).  The float64 term is -max(y - log1p(e^y), -100) for label 1 and log1p(e^y) for label 0.  For
    y < 0 the error of o is relative, (|y| + 3) u (the fast exponential's |y| u + 2 u, the addition, the division), and goes
    into the logarithm one to one.  The logarithm is the hardware log2, 1 ulp (2 u relative) of a value of at most
    1.4427 (|y| + 1), times ln 2: 2 u (|y| + 1), and the product's rounding, u (|y| + 1).  Together (4 |y| + 6) u, below
    4 u (|y| + 2), the factor _head_ref uses for the relative error of o.  Label 0: log(1 - o) with 1 - o >= 1/2, below 8 u."""
    return 4 * U * (y.double().abs() + 2)


def _check_head(tag, y, label, out, dy, loss):
    B = y.numel()
    special, o_ref, l_ref, dy_ref, tol_o, tol_l, tol_dy = _head_ref(y, label)
    tol_l = torch.where(y < 0, NEG_LOSS_TOL(y), tol_l)
    _within(tag + " out", out, o_ref, tol_o)
    _within(tag + " dy", dy, dy_ref, tol_dy)
    # the mean: every row's term goes through at most 20 float32 additions and one division on its way to loss[1]
    _within(tag + " bce", loss[1], l_ref.sum() / B, (tol_l.sum() + R.gamma(20) * l_ref.abs().sum()) / B)
    return dy_ref, tol_dy


@pytest.mark.parametrize("kind", ["relu", "negative", "band"])
@pytest.mark.parametrize("B", [1, 255, 256, 257, 1000])
def test_nfcf_loss_bce_only_against_the_head_reference(B, kind):
    y, label = _head_scores(B, kind)
    if B >= 255:
        assert bool((y == 0).any()) and bool(((y > 0) & (y < 8)).any()) and bool((y >= 20).any())
        assert bool((y <= -88).any()) == (kind == "negative") and bool((y < 0).any()) == (kind == "negative")
        assert bool(((y > 15.5) & (y < 17.5)).any()) == (kind == "band")
    out, dy, loss, err, _ = _nfcf(y, label)
    assert err == 0
    _check_head(f"nfcf_loss bce B={B}", y, label, out, dy, loss)
    assert float(loss[1]) == float(loss[0]) and float(loss[2]) == 0.0


def test_nfcf_loss_bce_of_one_row_in_every_regime():
    # (B = 1: loss[1] IS the row's term.  -28 .. -100: the rows of the exact-exponential branch; -88.5, -95: exp(-y) at and past
    # its overflow, where the term is |y| and not the clamp's 100; -100: the clamp itself)
    for yv in (0.0, 3.0, 16.5, 25.0, -5.0, -26.9, -27.1, -28.0, -30.0, -50.0, -88.5, -95.0, -100.0):
        for t in (0.0, 1.0):
            y, label = torch.tensor([yv]), torch.tensor([t])
            out, dy, loss, err, _ = _nfcf(y, label)
            _check_head(f"nfcf_loss bce one row y={yv} t={t}", y, label, out, dy, loss)
            assert err == 0 and float(loss[1]) == float(loss[0]) and float(loss[2]) == 0.0


# ---- F. fr_nfcf_loss with the differential-fairness term ---------------------------------------------------------------------

FW = 0.5


def _segments(item, n_items):
    """an item table looked up with the batch's ids, as the model does: its workspace then holds their sorted segments"""
    from fairrec.optim import AdamHyper, LazyTable
    table = LazyTable(torch.zeros(n_items, 64, device="cuda"))
    table.ensure_state()
    hyper = AdamHyper(1e-3, 0.0, device="cuda")
    err = _errflag()
    table.gather_train(hyper, _dev(item), err)
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    return table, hyper


@functools.lru_cache(maxsize=None)
def _df_case(B):
    b = R.df_batch(B, B + 50)
    return b, R.nfcf_loss(b.y, b.label, b.sst, b.item, FW)


@pytest.mark.parametrize("B", [1, 17, 256, 257, 1000])
def test_nfcf_loss_with_the_df_term_against_float64(B):
    b, r = _df_case(B)
    y, label = torch.from_numpy(b.y), torch.from_numpy(b.label)
    table, hyper = _segments(b.item, B + 50)
    out, dy, loss, err, K = _nfcf(y, label, b.sst, FW, table)
    assert err == 0 and K == float(r.K)
    tag = f"nfcf_loss df B={B}"
    special, o_ref, l_ref, dy_head, tol_o, tol_l, tol_dy = _head_ref(y, label)
    _within(tag + " out", out, o_ref, tol_o)
    bce_tol = (tol_l.sum() + R.gamma(20) * l_ref.abs().sum()) / B
    _within(tag + " bce", loss[1], l_ref.sum() / B, bce_tol)
    t_loss, t_dy = R.df_tolerances(r, tol_dy)
    _within(tag + " df", loss[2], r.loss[2], t_loss)
    _within(tag + " loss", loss[0], l_ref.sum() / B + FW * r.loss[2], bce_tol + FW * t_loss + 2 * U * float(r.loss[0].abs()))
    _within(tag + " dy", dy, dy_head + r.dy_df, t_dy)
    # the item with one positive row per group and equal scores: d == 0, nothing added to the BCE gradient of its rows
    o0, dy0, loss0, err0, _ = _nfcf(y, label)
    if "zero" in b.has and r.items:
        rows = torch.from_numpy(b.item == b.zero_item)
        assert int(rows.sum()) == 2 and _bits(dy[rows], dy0[rows])
    assert _bits(out, o0) and _bits(loss[1:2], loss0[1:2])
    if r.items:
        assert not _bits(dy, dy0)


@pytest.mark.parametrize("case", ["one_group", "no_positive"])
def test_nfcf_loss_df_is_exactly_zero_without_two_groups(case):
    b, _ = _df_case(257)
    y, label, sst = torch.from_numpy(b.y), torch.from_numpy(b.label).clone(), b.sst.copy()
    if case == "one_group":
        sst[b.label == 1] = 2.0                  # the negatives keep both values: only the positive rows count
        assert len(np.unique(sst)) == 2
    else:
        label.zero_()
    table, hyper = _segments(b.item, 307)
    out, dy, loss, err, K = _nfcf(y, label, sst, FW, table)
    o0, dy0, loss0, err0, _ = _nfcf(y, label)
    assert err == 0 and err0 == 0
    assert float(loss[2]) == 0.0 and _bits(loss[:2], loss0[:2]) and _bits(dy, dy0) and _bits(out, o0)
    assert K == (float(len(np.unique(b.item[b.label == 1]))) if case == "one_group" else 0.0)


def test_nfcf_loss_df_flags_a_third_group_among_the_positives():
    from fairrec import _C
    b, _ = _df_case(257)
    y, label, sst = torch.from_numpy(b.y), torch.from_numpy(b.label), b.sst.copy()
    table, hyper = _segments(b.item, 307)
    sst_neg = sst.copy()
    sst_neg[np.nonzero(b.label == 0)[0][0]] = 1.5            # a third value on a NEGATIVE row: not counted, no error
    *_, err, _ = _nfcf(y, label, sst_neg, FW, table)
    assert err == 0
    sst[np.nonzero(b.label == 1)[0][5]] = 1.5
    *_, err, _ = _nfcf(y, label, sst, FW, table)
    assert err == _C.DEV_ERR_SST_GROUPS

"""GPU: the FOCF loss and its gradient in every step form against the float64 reference of tests/focf_ref.py (pinned to
oracle.focf.loss under float64 autograd by tests/test_focf_ref.py).

One engine per case: FocfEngine + FusedLazyAdam(lr=1e-3, weight_decay=0, sweep_period=3), zero optimizer state, ONE batch.
After backward_adam(); finish(); flush(); check_device_errors() the loss triple is compared with the reference, m / (1 - b1)
of both tables with gradU / gradI in units of u A, v with the bound that follows, and the rows outside the batch must be
bit-unchanged with m == v == 0.  The form is chosen through the engine's own switches and asserted in every case.
Tolerances: focf_ref.tol_const(key) on the units focf_ref states -- constants measured on the reference's float32 arithmetic,
never on a kernel."""
import numpy as np
import pytest
import torch

import focf_ref as R

pytestmark = pytest.mark.gpu

U = R.U
FW = R.FAIR_WEIGHT
MAX_RATING = 5.0
FORMS = ("CHAIN", "SORTED", "STAGED", "RUNS", "RUNS_PIPE")
RUN_FORMS = ("RUNS", "RUNS_PIPE")
# the only combinations left out: what the engine documents as unsupported -- nonparity (needs the groups' means between loss
# and update) and clip_grad_norm (needs every gradient row before any update) in a one-launch form
UNSUPPORTED = [(form, what) for form in FORMS[1:] for what in ("nonparity", "clip")]
COMBOS = [(form, obj) for form in FORMS for obj in R.OBJECTIVES if (form, obj) not in UNSUPPORTED]
CLIP_FORMS = [form for form in FORMS if (form, "clip") not in UNSUPPORTED]
STEP_CASES = [(name, D) for name in ("segments", "one_sided", "encodings", "regimes", "counts") for D in R.BUILDER_WIDTHS[name]]


def _engine(b, objective, form):
    from fairrec.model.fair_recommender.focf import FocfEngine
    from fairrec.optim import FusedLazyAdam
    eng = FocfEngine(torch.tensor(b.U, device="cuda"), torch.tensor(b.I, device="cuda"), objective, FW, MAX_RATING)
    FusedLazyAdam(eng, lr=1e-3, weight_decay=0.0, sweep_period=3)
    eng.defer_loss = form != "CHAIN"
    eng.staged = form == "STAGED"
    eng.item_runs = form in RUN_FORMS
    eng.PIPE = form == "RUNS_PIPE"
    return eng


def _cols(b, form):
    return [torch.tensor(c, device="cuda") for c in b.cols(form in RUN_FORMS)]


def _assert_ran_as(eng, form):
    """after backward_adam(): the record the form leaves on the engine (the table of the engine's module docstring)"""
    if form == "CHAIN":
        assert eng._prev is None and eng._pipe is None
    elif form == "RUNS_PIPE":
        assert eng._pipe is not None
    else:
        assert eng._pipe is None and eng._prev is not None and eng._prev.staged == (form == "STAGED")


def _step(b, objective, form, max_norm=None):
    """one step of batch b from zero optimizer state -> (engine, loss triple, norm_out of clip_grad_norm or None)"""
    from fairrec.model.fair_recommender.focf import Form
    eng = _engine(b, objective, form)
    cols = _cols(b, form)
    loss, _ = eng.forward(*cols)
    assert eng._form_of(eng._stash) is Form[form], (eng._form_of(eng._stash), form)
    clip = eng.clip_grad_norm(max_norm).clone() if max_norm is not None else None
    eng.backward_adam()
    _assert_ran_as(eng, form)
    eng.finish()
    eng.flush()
    if objective == "nonparity" and not R.two_groups(b):
        # one sst value: the kernels report fair = 0, leave the MSE gradient alone and flag what the reference raises eagerly
        with pytest.raises(IndexError, match="sensitive groups"):
            eng.check_device_errors()
    eng.check_device_errors()
    assert eng.U.step == 1 and eng._prev is None and eng._pipe is None
    return eng, loss[:3].cpu().double().numpy(), (clip.cpu().double().numpy() if clip is not None else None)


def _tol(b, key):
    return R.tol_const(f"{key}_{b.builder}")


def _check_loss(b, r, loss, what):
    for j, (key, ref, bound) in enumerate((("loss", r.loss, r.mse + FW * r.fair), ("mse", r.mse, r.mse), ("fair", r.fair, r.fair))):
        tol = _tol(b, key) * U * (abs(ref) + bound)
        assert abs(loss[j] - ref) <= tol, f"{what}: {key} {loss[j]!r} against {ref!r}, {abs(loss[j] - ref) / max(tol, 1e-300) * _tol(b, key):.3g} units"


def _check_tables(b, r, eng, what, coef=1.0, coef_rel=0.0):
    """m / (1 - b1) against coef * grad within tol_const(m) u A (+ coef_rel |coef grad|: a clip coefficient's own bound), v
    against the bound that follows, rows outside the batch untouched"""
    for tag, tab, T0, g, A, rows in (("U", eng.U, b.U, r.gradU, r.AU, r.rows_u), ("I", eng.I, b.I, r.gradI, r.AI, r.rows_i)):
        g, A = coef * g, coef * A
        m, v = tab.m.cpu().double().numpy(), tab.v.cpu().double().numpy()
        tol_g = _tol(b, "m") * U * A + coef_rel * np.abs(g)
        err = np.abs(m / (1.0 - R.B1) - g)
        bad = err > tol_g
        assert not bad.any(), (f"{what}: grad{tag} {int(bad.sum())} of {bad.size} entries outside, worst "
                               f"{float((err[A > 0] / (U * A[A > 0])).max()):.4g} units of u A (allowed {_tol(b, 'm'):.4g})")
        bad = np.abs(v - R.adam_first_step(g)[1]) > R.v_tolerance(g, tol_g)
        assert not bad.any(), f"{what}: v{tag} {int(bad.sum())} of {bad.size} entries outside"
        out = np.ones(T0.shape[0], dtype=bool)
        out[rows] = False
        assert not m[out].any() and not v[out].any(), f"{what}: moments of {tag} rows outside the batch"
        assert np.array_equal(tab.weight.cpu().numpy()[out].view(np.int32), T0[out].view(np.int32)), f"{what}: {tag} rows outside the batch"
        assert (tab.weight.cpu().numpy()[rows] != T0[rows]).any()


@pytest.mark.parametrize("name,D", STEP_CASES, ids=[f"{n}-{D}" for n, D in STEP_CASES])
@pytest.mark.parametrize("form,objective", COMBOS, ids=[f"{f}-{o}" for f, o in COMBOS])
def test_one_step_matches_the_float64_reference(form, objective, name, D):
    for b in R.batches(name, D):
        r = R.reference(b, objective, form in RUN_FORMS)
        eng, loss, _ = _step(b, objective, form)
        what = f"{b.name} D={D} {form} {objective}"
        _check_loss(b, r, loss, what)
        _check_tables(b, r, eng, what)


@pytest.mark.parametrize("D", R.BUILDER_WIDTHS["exact_kinks"])
@pytest.mark.parametrize("objective", R.PER_ITEM)
@pytest.mark.parametrize("form", FORMS)
def test_exact_kinks_take_torchs_side(form, objective, D):
    """(a) a group with P == T exactly: the members on the kink get the reference's gradient (under / over pass it at equality,
    abs'(0) = 0); (b) delta == 0 exactly with d != 0: the fairness gradient is exactly 0 -- the rows' moments are the bits of the
    same step without a fairness term."""
    b = R.batches("exact_kinks", D)[0]
    r = R.reference(b, objective, True)         # (the batch is item-contiguous as built; a shuffle changes no gradient)
    eng, loss, _ = _step(b, objective, form)
    what = f"exact_kinks D={D} {form} {objective}"
    _check_loss(b, r, loss, what)
    _check_tables(b, r, eng, what)
    users = b.user[b.on_kink]                   # every user of this batch has one interaction: its row's gradient is the member's
    m = eng.U.m.cpu().double().numpy()[users] / (1.0 - R.B1)
    err = np.abs(m - r.gradU[users])
    assert (err <= _tol(b, "m") * U * r.AU[users]).all(), f"{what}: members on the kink"
    if objective in ("under", "over"):
        mine = np.array([b.kind[int(it)].split("_")[1] == objective for it in b.item[b.on_kink]])
        assert mine.sum() >= 4 and (np.abs(r.gradU[users][mine]).max(1) > 0).all() and (np.abs(m[mine]).max(1) > 0).all(), what
    plain, _, _ = _step(b, "none", form)
    for tab, tab0, rows in ((eng.U, plain.U, b.user[b.zero_fair]), (eng.I, plain.I, np.unique(b.item[b.zero_fair]))):
        rows = torch.tensor(rows, device="cuda")
        assert torch.equal(tab.m[rows], tab0.m[rows]) and torch.equal(tab.v[rows], tab0.v[rows]), f"{what}: (b) rows"
        assert torch.equal(tab.weight[rows], tab0.weight[rows])


@pytest.mark.parametrize("factor", [2.0, 0.5], ids=["above", "below"])
@pytest.mark.parametrize("objective", ["value", "nonparity"])
@pytest.mark.parametrize("name,D", [(n, D) for n in ("regimes", "segments") for D in R.FRAGMENT_WIDTHS])
@pytest.mark.parametrize("form", CLIP_FORMS)
def test_clip_grad_norm_matches_the_float64_reference(form, name, D, objective, factor):
    """max_norm above the gradient norm (the coefficient is held at 1) and below it: norm_out = (norm, coef) against float64,
    m afterwards = coef (1 - b1) g"""
    b = R.batches(name, D)[0]
    r = R.reference(b, objective, False)
    max_norm = factor * r.norm
    eng, loss, out = _step(b, objective, form, max_norm=max_norm)
    coef = min(1.0, max_norm / (r.norm + 1e-6))
    rel = _tol(b, "norm") * U
    what = f"{name} D={D} clip {factor} {objective}"
    assert abs(out[0] - r.norm) <= rel * r.norm, f"{what}: norm {out[0]!r} against {r.norm!r}"
    assert abs(out[1] - coef) <= (rel + 2 * U) * coef and (factor < 1 or out[1] == 1.0), f"{what}: coef {out[1]!r} against {coef!r}"
    _check_loss(b, r, loss, what)
    _check_tables(b, r, eng, what, coef=coef, coef_rel=rel + 2 * U)


@pytest.mark.parametrize("D", [40, 64, 256])
def test_predict_at_the_clamp_edges(D):
    """fr_focf_predict: pred exactly 0, exactly max_rating, below 0, above max_rating (rows of one nonzero each: the products are
    exact) and interior rows"""
    from fairrec.model.fair_recommender.focf import FocfEngine
    from fairrec.optim import FusedLazyAdam
    b = R.batches("segments", D)[0]
    Ut, It = b.U.copy(), b.I.copy()
    It[0] = 0
    It[0, D - 1] = 2.0
    Ut[:5] = 0
    Ut[0, 0], Ut[1, D - 1], Ut[2, D - 1], Ut[3, D - 1], Ut[4, D - 1] = 1.0, 2.5, -1.5, 4.0, 1.25
    user = np.concatenate([np.arange(5), b.user])
    item = np.concatenate([np.zeros(5, np.int64), np.where(b.item == 0, 1, b.item)])
    eng = FocfEngine(torch.tensor(Ut, device="cuda"), torch.tensor(It, device="cuda"), "value", FW, MAX_RATING)
    FusedLazyAdam(eng, lr=1e-3, weight_decay=0.0, sweep_period=3)
    got = eng.predict(torch.tensor(user, device="cuda"), torch.tensor(item, device="cuda")).cpu().double().numpy()
    eng.check_device_errors()
    ref = R.predict(Ut, It, user, item, MAX_RATING)
    assert ref[:5].tolist() == [0.0, 1.0, 0.0, 1.0, 0.5]
    assert got[0] == 0.0 and got[2] == 0.0                                   # exactly 0, and below 0
    assert abs(got[1] - 1.0) <= 2 * U and abs(got[3] - 1.0) <= 2 * U         # exactly max_rating, and above (a division or a
    assert abs(got[4] - 0.5) <= 2 * U                                        #   multiplication by the rounded reciprocal)
    ppos = (np.abs(Ut.astype(np.float64)[user]) * np.abs(It.astype(np.float64)[item])).sum(-1)
    g = (D + 2) * U / (1 - (D + 2) * U)
    assert (np.abs(got - ref) <= g * ppos / MAX_RATING + 2 * U * ref).all()
    assert ((ref > 0) & (ref < 1)).sum() > 100 and got.min() >= 0.0 and got.max() <= 1.0


@pytest.mark.parametrize("runs", [False, True], ids=["steps_many", "runs_many"])
def test_library_loops_report_the_same_loss_and_moments(runs):
    """fr_focf_steps_many / fr_focf_runs_many on one batch against float64 (their bit-identity with the per-batch forms is
    tested in test_focf_hip.py)"""
    D, objective = 64, "value"
    b = R.batches("segments", D)[0]
    form = "RUNS_PIPE" if runs else "STAGED"
    r = R.reference(b, objective, runs)
    eng = _engine(b, objective, form)
    assert eng.can_step_many()
    assert eng.steps_many(*_cols(b, form), b.B) == 1
    _assert_ran_as(eng, form)
    loss = eng.loss_ring[1]
    eng.finish()
    eng.flush()
    eng.check_device_errors()
    what = f"segments {form} through the library loop"
    _check_loss(b, r, loss[:3].cpu().double().numpy(), what)
    _check_tables(b, r, eng, what)
    np.testing.assert_array_equal(eng.loss_acc[:3].cpu().numpy(), loss[:3].cpu().numpy())

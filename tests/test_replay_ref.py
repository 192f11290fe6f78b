"""CPU: tests/replay_ref.py -- the float64 reference the replay kernel tests compare with -- against torch.optim in float64, the
conditions its input builders promise at every shape the GPU file uses, the sensitivity of those inputs to a replay that
miscounts by one step, and the measurement behind the tolerance constants: the float32 restatement of the device formulas
against float64 on those inputs (printed, and asserted against replay_ref.MEASURED)."""
import numpy as np
import pytest
import torch

import replay_ref as R

U = R.U


@pytest.fixture(scope="module")
def decay_hyper():
    return R.make_hyper("adagrad", 1e-2, lr_decay=R.LR_DECAY)          # (a large host table: built once)


# ---- the reference against torch ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,wd", [(n, wd) for n in R.LEARNERS for wd in R.WDS] + [("adagrad_decay", 1e-2)])
def test_reference_is_torch_optim_in_float64(name, wd, decay_hyper):
    """stock torch.optim.<Learner> on float64 tensors, state poked in at step `frm`, zero gradients and one real one"""
    decay = name == "adagrad_decay"
    name = "adagrad" if decay else name
    h = decay_hyper if decay else R.make_hyper(name, wd)
    hp = R.hp_of(h)
    p0, m0, v0 = R.table_values(3, 5, seed=9)
    m0, v0 = R.state_of(name, m0, v0)
    frm, to, real = 4, 11, 8
    g = np.random.default_rng(1).standard_normal((3, 5)) * 0.01
    P = torch.nn.Parameter(torch.from_numpy(p0).double())
    if name == "adam":
        opt = torch.optim.Adam([P], lr=hp.lr, betas=(hp.b1, hp.b2), eps=hp.eps, weight_decay=wd, foreach=False)
        opt.state[P] = {"step": torch.tensor(float(frm)), "exp_avg": torch.from_numpy(m0).double(),
                        "exp_avg_sq": torch.from_numpy(v0).double()}
    elif name == "sgd":
        opt = torch.optim.SGD([P], lr=hp.lr, weight_decay=wd, foreach=False)
    elif name == "adagrad":
        opt = torch.optim.Adagrad([P], lr=hp.lr, lr_decay=hp.lr_decay, weight_decay=wd, eps=hp.eps, foreach=False)
        opt.state[P]["step"] = torch.tensor(float(frm))
        opt.state[P]["sum"] = torch.from_numpy(m0).double()
    else:
        opt = torch.optim.RMSprop([P], lr=hp.lr, alpha=hp.alpha, eps=hp.eps, weight_decay=wd, foreach=False)
        opt.state[P] = {"step": torch.tensor(float(frm)), "square_avg": torch.from_numpy(m0).double()}
    for j in range(frm + 1, to + 1):
        P.grad = torch.from_numpy(g).double() if j == real else torch.zeros_like(P)
        opt.step()
    p, m, v = R.ref_replay(hp, p0, m0, v0, [frm] * 3, to, {real: g})
    np.testing.assert_allclose(p, P.detach().numpy(), rtol=1e-13)
    key = {"adam": "exp_avg", "adagrad": "sum", "rmsprop": "square_avg"}.get(name)
    if key:
        np.testing.assert_allclose(m, opt.state[P][key].numpy(), rtol=1e-12, atol=1e-300)
    if name == "adam":
        np.testing.assert_allclose(v, opt.state[P]["exp_avg_sq"].numpy(), rtol=1e-12)


def test_scalar_tables_saturate_where_the_cases_expect():
    from fairrec.optim import AdamHyper
    assert R.make_hyper("adam", 1e-2).cap == R.CAP_SMALL == 256
    assert R.make_hyper("adam", 0.0, betas=(0.9, 0.999)).cap == R.CAP_DEFAULT == 16384
    h = AdamHyper(R.LR["adam"], 0.0, betas=(0.5, 0.75), cap=8, device="cpu")
    assert h.saturated and h.cap == 64
    # entry `cap` is what the entries before it have already become: the cases around `cap` see the count, not the entry
    tab = R.make_hyper("adam", 1e-2).host_scalars.reshape(-1, 4)
    assert (tab[R.CAP_SMALL - 3:] == tab[R.CAP_SMALL]).all() and not (tab[20] == tab[R.CAP_SMALL]).all()


def test_end_steps_put_from_below_on_and_above_cap():
    frm = {to - s for to in R.wide_end_steps() for s in R.WIDE if s <= to}
    assert 0 in frm and {R.CAP_SMALL - 1, R.CAP_SMALL, R.CAP_SMALL + 1} <= frm and max(frm) > R.CAP_SMALL + 60
    frm = {to - s for to in R.narrow_end_steps() for s in R.NARROW + (R.LONGEST,) if s <= to}
    assert 0 in frm and {R.CAP_SMALL - 1, R.CAP_SMALL, R.CAP_SMALL + 1} <= frm and min(f for f in frm if f) < R.CAP_SMALL - 64


# ---- the float32 restatement's fixed points ----------------------------------------------------------------------------------

@pytest.mark.parametrize("wd", R.WDS)
@pytest.mark.parametrize("name", R.LEARNERS)
def test_current_rows_and_identity_steps_keep_their_bits(name, wd):
    h = R.make_hyper(name, wd)
    c = R.flush_case(name, 3, 14)
    p, m, v = R.f32_run(h, c.p, c.m, c.v, [("replay", np.arange(c.n_rows), c.frm, c.to)])
    cur = c.s == 0
    assert cur.any() and (p[cur] == c.p[cur]).all()
    if c.m is not None:
        assert (m[cur] == c.m[cur]).all()
    if wd == 0.0 and name != "adam":          # a missed step leaves p as it is (RMSprop: square_avg decays all the same)
        assert (p == c.p).all()
        assert name != "rmsprop" or (m[~cur] < c.m[~cur]).all()
        assert name != "adagrad" or (m == c.m).all()
    elif wd == 1e-2 or name == "adam":        # (at 1e-6 the other learners' step is below an ulp of p)
        assert (p[~cur] != c.p[~cur]).all()


# ---- builders ----------------------------------------------------------------------------------------------------------------

def test_narrow_ages_hold_their_kinds():
    for n in R.NARROW_ROWS:
        for to in R.narrow_end_steps():
            s = R.narrow_ages(n, to)
            assert s.shape == (n,) and (s <= to).all() and set(s.tolist()) <= set(R.NARROW + (R.LONGEST,))
            if n >= 64:
                wave = s[:64]
                assert len(set(wave.tolist())) >= 8, "ages are not mixed inside a wave"
        assert not R.narrow_ages(n, 300, "current").any()
        assert (R.narrow_ages(n, 300, "single") > 0).sum() == 1
    assert R.LONGEST in R.narrow_ages(130, 326) and R.LONGEST not in R.narrow_ages(130, 261)


@pytest.mark.parametrize("n_rows,S", R.SWEEP_SHAPES)
def test_sweep_scenario_holds_its_structures(n_rows, S):
    sc = R.sweep_scenario(n_rows, S, 2)
    assert len(sc.batches) == S + 2 and sc.step0 >= sc.ages.max()
    slices = [R.sweep_range(n_rows, t, S) for t in range(S)]
    assert sorted(set(r for lo, hi in slices for r in range(lo, hi))) == list(range(n_rows))
    if (n_rows, S) == (5, 4):
        assert R.sweep_range(5, 3, 4) == (5, 5)                      # the empty last slice
    if (n_rows, S) == (10, 4):
        assert R.sweep_range(10, 3, 4) == (9, 10)                    # the short one
    for pairs in (False, True):
        sch = R.schedule(sc, pairs)
        # after S consecutive steps every row has been in a slice or a batch: nobody is older than S steps
        assert (sch.last[-1] >= sch.T - S).all() and (sch.last[-1] <= sch.T).all()
        for i, ids in enumerate(sc.batches):
            t = sc.step0 + 1 + i
            assert (sch.last[i][ids] == t).all() and (sch.stamp[i][ids] == t).all()
    if (n_rows, S) == (130, 3):
        kinds = R.schedule(sc, True).kinds
        assert {("equal", 0), ("partner in batch", 0)} <= kinds
        assert {("stagger", d) for d in (1, 3, 4, 9)} <= kinds
        a, b = sc.ages[0::2], sc.ages[1::2]
        assert ((a < b).any() and (b < a).any()), "both orders of a staggered pair"


# ---- sensitivity: a replay that miscounts by one step does not pass -----------------------------------------------------------

def _p_tol(name, kind, ref_p):
    return R.tol_const(f"{name}_{kind}_p") * U * np.abs(ref_p)


@pytest.mark.parametrize("name", R.LEARNERS)
def test_one_step_short_or_long_is_far_outside_the_tolerance(name, decay_hyper):
    cases = [(R.kind_of(name, "short", wd), R.make_hyper(name, wd), R.flush_case(name, D, to)) for wd in R.WDS
             for D in (2, 64, 129) for to in R.wide_end_steps()]
    cases += [(R.kind_of(name, "long", wd), R.make_hyper(name, wd), R.narrow_case(name, 130, to)) for wd in R.WDS
              for to in R.narrow_end_steps()]
    if name == "adagrad":
        cases += [("short", decay_hyper, R.flush_case(name, D, 14)) for D in (1, 64)]
    for kind, h, c in cases:
        hp = R.hp_of(h)
        ref = R.ref_replay(hp, c.p, c.m, c.v, c.frm, c.to)
        behind = c.s >= 1
        for wrong in R.miscount(hp, c):
            assert (wrong[0][~behind] == ref[0][~behind]).all()
            if hp.wd == 1e-2:         # every learner moves p: some element of every row that is behind shows it
                off = np.abs(wrong[0] - ref[0]) / _p_tol(name, kind, ref[0])
                caught = off.max(axis=1) >= 10.0
                # (a D == 1 row has one element: one or two steps behind, Adam's m is still mostly m0 ~ N(0, 0.01), which
                # may lie next to zero -- more than half of those rows, and every older row)
                sure = behind if c.D > 1 or name != "adam" else c.s > 2
                assert caught[sure].all() and caught[behind].mean() > 0.5, (name, kind, c.D, c.to, off.max(axis=1))
            elif name in ("adam", "rmsprop") and kind.startswith("short"):     # the decaying state carries the count, in every element
                k = 2 if name == "adam" else 1
                e = np.abs(wrong[k] - ref[k]) / (U * (np.abs(ref[k]) + np.abs(ref[k]).max()))
                assert (e[behind] >= 10.0 * R.tol_const(f"{name}_{kind}_{'v' if name == 'adam' else 'm'}")).all()


# ---- the measurement behind the tolerance constants --------------------------------------------------------------------------

def _worst(worst, name, kind, got, ref):
    for key, e in R.units(name, got, ref).items():
        k = f"{name}_{kind}_{key}"
        worst[k] = max(worst.get(k, 0.0), float(e.max()))


def _record(worst):
    """print every figure, then hold each to the recorded constant: not above it, and the record within twice of it"""
    for key, w in worst.items():
        print(f"\nreplay_ref measurement {key}: float32 restatement's worst error {w:.4g} units (recorded {R.MEASURED.get(key)})")
    for key, w in worst.items():
        assert w <= R.MEASURED[key], f"{key}: the float32 restatement errs by {w:.4g} units, recorded {R.MEASURED[key]}"
        assert w >= 0.5 * R.MEASURED[key], f"{key}: recorded {R.MEASURED[key]} is no measurement ({w:.4g})"


def _measure_case(worst, name, kind, h, c, track):
    ref = R.ref_replay(R.hp_of(h), c.p, c.m, c.v, c.frm, c.to, track=track)
    got = R.f32_run(h, c.p, c.m, c.v, [("replay", np.arange(c.n_rows), c.frm, c.to)])
    _worst(worst, name, kind, got, ref)


@pytest.mark.parametrize("name", R.LEARNERS)
def test_measure_short_stretches(name, decay_hyper):
    """the tables of the flush and gather tests: every width, weight decay and end step, the wide list"""
    worst, track = {}, []
    for wd in R.WDS:
        h = R.make_hyper(name, wd)
        for D in R.WIDTHS:
            for to in R.wide_end_steps():
                _measure_case(worst, name, R.kind_of(name, "short", wd), h, R.flush_case(name, D, to), track)
        if name == "adam":        # the default betas, inside their table
            hd = R.make_hyper(name, wd, betas=(0.9, 0.999))
            for to in (13, 14, 200):
                _measure_case(worst, name, "short", hd, R.flush_case(name, 64, to), track)
    if name == "adagrad":
        for D in (1, 64):
            _measure_case(worst, name, "short", decay_hyper, R.flush_case(name, D, 14), track)
    R.assert_conditioned(track)
    _record(worst)


@pytest.mark.parametrize("name", R.LEARNERS)
def test_measure_long_stretches(name):
    """the D == 1 tables: the narrow list and one row LONGEST steps behind"""
    worst, track = {}, []
    for wd in R.WDS:
        h = R.make_hyper(name, wd)
        for n in R.NARROW_ROWS:
            for to in R.narrow_end_steps():
                _measure_case(worst, name, R.kind_of(name, "long", wd), h, R.narrow_case(name, n, to), track)
        for kind in ("current", "single"):
            _measure_case(worst, name, R.kind_of(name, "long", wd), h, R.narrow_case(name, 64, R.CAP_SMALL + 5, kind), track)
    # the longest stretch there is, on every row: min |p| after LONGEST steps at the strongest weight decay
    c = R.flush_case(name, 64, R.LONGEST, ages=(R.LONGEST,), reps=32)
    R.ref_replay(R.hp_of(R.make_hyper(name, 1e-2)), c.p, c.m, c.v, c.frm, c.to, track=track)
    print(f"\nreplay_ref conditioning {name}: min |p| over all stretches {min(t[0] for t in track):.4g}")
    R.assert_conditioned(track)
    _record(worst)


@pytest.mark.parametrize("name", ["adam", "rmsprop"])
def test_measure_trajectories_with_real_steps(name):
    """the sweep scenario (gather_train + apply_grad with the sweeper slice, then a flush) and Adam's real step at stale rows"""
    worst, track = {}, []
    h = R.make_hyper(name, 1e-2)
    hp = R.hp_of(h)
    for n_rows, S in R.SWEEP_SHAPES:
        for D in R.SWEEP_WIDTHS:
            sc = R.sweep_scenario(n_rows, S, D)
            state = R.state_of(name, sc.m, sc.v)
            sch = R.schedule(sc, pairs=name == "adam" and 1 < D <= 64)
            got = R.f32_run(h, sc.p, state[0], state[1], sch.ops)
            _worst(worst, name, "real", got, R.scenario_ref(hp, sc, state))
    if name == "adam":
        for wd in (0.0, 1e-2):
            hw = R.make_hyper(name, wd)
            for D in (1, 64, 129):
                for to in (14, R.CAP_SMALL + 1):
                    sb = R.stale_batch(D, to)
                    c, rows = sb.case, np.unique(sb.ids)
                    G = R.batch_grad32(c.n_rows, sb.ids, sb.g)
                    got = R.f32_run(hw, c.p, c.m, c.v, [("replay", rows, c.frm[rows], to - 1), ("real", rows, to, G[rows])])
                    G64 = np.zeros((c.n_rows, D))
                    np.add.at(G64, sb.ids, sb.g.astype(np.float64))
                    frm = np.where(np.isin(np.arange(c.n_rows), rows), c.frm, to)        # rows outside the batch stay
                    ref = R.ref_replay(R.hp_of(hw), c.p, c.m, c.v, frm, to, {to: G64}, track=track)
                    _worst(worst, name, "real", [x[rows] for x in got], [x[rows] for x in ref])
    R.assert_conditioned(track)
    _record(worst)

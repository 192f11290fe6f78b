"""Float64 reference of the lazy tables' replay (csrc/common.hpp: adam_zero, adam_zero_scaled, replay_loop, replay_scaled,
replay_plain; csrc/table.hpp: row_at_step, sweep_row, sweep_row_pair, sweep_rows_narrow) and the inputs its tests run on:
plain numpy on the CPU, no GPU, and of fairrec only fairrec.optim for the host scalar tables.  tests/test_replay_ref.py checks
what the builders promise and measures the tolerance constants; tests/test_replay_hip.py compares the kernels with it.

* `ref_replay`: one row element over a stretch (from, to] of optimizer steps, torch's step restated in float64 for each learner
  (Adam: torch/optim/adam.py::_single_tensor_adam with bc1, bc2 per step in double; SGD, Adagrad, RMSprop: the formulas of
  test_learners_hip._ref_step, Adagrad with clr_j = lr / (1 + (j - 1) lr_decay)).  A step without an entry in `grads` has a zero
  data gradient (a replayed step), one with an entry is a real step.  It knows nothing of `cap`, of scaled moments or of
  unrolling.
* `f32_run`: the device formulas restated in numpy float32 operation by operation, fma where the code has fma (the product
  of two float32 is exact in float64, so float32(a * b + c) in float64 is the fma up to a double rounding), the scalars from
  the project's own host table (`hyper.host_scalars`, entry min(j, cap)), the scaled moments where weight decay is on, one
  scale / unscale per replay call as on the device.  numpy's correctly rounded sqrt and reciprocal stand for the 1-ulp
  v_sqrt_f32 / v_rcp_f32.  Its error against float64 is what the tolerance constants are measured from.
* `table_values`, `flush_case`, `narrow_case`, `sweep_scenario`, `stale_batch`: the inputs, each builder asserting what it is
  built for.  `schedule` restates the bookkeeping of fr_table_gather_train / fr_table_apply_grad (kernels.hpp: sweep_range;
  stamps; the pairs of sweep_row_pair) on the integers.

Conditioning.  With a zero data gradient Adam moves p by about lr per step whatever p is, so at lr = 1e-2 it walks a weight
of 0.1 through zero within some 40 steps and oscillates there; the float32 restatement is then 1e7 u away from float64, which
says something about the reference and nothing about a kernel.  The builders use lr = 1e-4 for Adam (|p| in [0.05, 0.2],
m0 ~ N(0, 0.01), v0 in [1e-4, 1.1e-3]) and assert that no reference p changes sign and min |p| >= 0.02 over the longest
stretch; the other learners' lr is chosen by the same rule (LR below) and asserted the same way.

Tolerances: the project's form, tol_const(key) = SAFETY * MEASURED[key] with SAFETY = 8 = 4 (1-ulp sqrt and rcp where numpy
rounds correctly) * 2 (another seed).  MEASURED is the worst error of `f32_run` against `ref_replay` on the builders' inputs:
p in units of u |ref| per element; m and v in units of u (|ref| + max |ref| over the tensor) -- m cancels against wd p, and
with weight decay off and beta1 = 0.5 it decays below the float32 normal range over 300 steps, so the states need the
per-tensor term.  Keys: `<learner>_<short|long|real>_<p|m|v>`; short = stretches of the wide list (up to 13 steps), long = the
narrow list (up to 297), real = trajectories that hold real steps (the sweep scenario, a batch of stale rows).
At weight decay 1e-6 the step of SGD, Adagrad and RMSprop is below half an ulp of p, which float32 then does not move at
all while float64 does: an error that grows with the stretch and is the number format's own.  Those cases have keys of their
own (`<learner>_<short|long>_tiny_<p|m>`), so that they do not loosen the others.
tests/test_replay_ref.py asserts every constant (the restatement may not exceed it, and reaches at least half of it): they
are a measurement of the REFERENCE side, never of the kernels.

What these cases cannot see.  `cap` is only valid once the table's entries have stopped changing in float32, so near `cap`
the entries already equal entry `cap`: the cases around `cap` catch a wrong step count or a read past the table, not entry
`cap` being used a step early.

Sensitivity (`miscount`).  A replay one step short or one step long must not pass.  Where the weight decay is 1e-2 every
learner's step moves p: in every row that is behind, some element of the miscounted reference is off by at least 10 times
its tolerance.  Not every element: Adam's step is lr |m_hat| / sqrt(v_hat), and m passes through zero on its way from m0 to
wd p (in a D == 1 table, whose rows have one element, that leaves some of the rows one or two steps behind uncaught).  At weight decay 0 and 1e-6 the step of SGD, Adagrad and RMSprop is below an ulp of p (or the identity), and Adam's m
halves every step (beta1 = 0.5), so late steps no longer move p; over the short stretches the states carry the count there:
Adam's v and RMSprop's square_avg shrink by beta2 / alpha per step, percents of themselves in every element.  Blind to the
count are SGD and Adagrad at these two weight decays (the step is the identity, or below the rounding of p and sum), and at
these weight decays the rows of the narrow tables that are 63 and more steps behind: their moments have decayed to nothing
next to the other rows', and one step more or less changes nothing that could be measured.
"""
from types import SimpleNamespace

import numpy as np

from fairrec.optim import AdagradHyper, AdamHyper, RMSpropHyper, SGDHyper

U = 2.0 ** -24
SAFETY = 8.0
F = np.float32

LEARNERS = ("adam", "sgd", "adagrad", "rmsprop")
WDS = (0.0, 1e-6, 1e-2)
# lr per learner: the largest round value at which the conditioning assertion of `assert_conditioned` holds over 297 steps
LR = {"adam": 1e-4, "sgd": 1e-2, "adagrad": 1e-3, "rmsprop": 1e-3}
LR_ADAGRAD_DECAY, LR_DECAY = 1e-2, 0.25           # the lr_decay case runs 14 steps only
BETAS_SMALL, CAP_SMALL = (0.5, 0.9), 256          # AdamHyper(betas=BETAS_SMALL, cap=8) saturates at 256
CAP_DEFAULT = 16384                               # ... and the default betas at 16384
WIDE = tuple(range(14))
NARROW = (0, 1, 2, 63, 64, 65, 127, 128, 129, 130)
LONGEST = 297                                     # one more age of the narrow tables: the longest stretch
WIDTHS = (1, 2, 63, 64, 65, 128, 129, 192, 256)
MIN_ABS_P = 0.02

# worst error of the float32 restatement against float64 on the builders' inputs (test_replay_ref.py prints and asserts them)
MEASURED = {"adam_short_p": 6.9, "adam_short_m": 1.9, "adam_short_v": 4.6, "sgd_short_p": 3.5,
            "sgd_short_tiny_p": 2.3, "adagrad_short_p": 8.8, "adagrad_short_m": 4, "adagrad_short_tiny_p": 14,
            "adagrad_short_tiny_m": 0.0071, "rmsprop_short_p": 5.1, "rmsprop_short_m": 5.3,
            "rmsprop_short_tiny_p": 13, "rmsprop_short_tiny_m": 2.8, "adam_long_p": 22, "adam_long_m": 4.3,
            "adam_long_v": 18, "sgd_long_p": 7.8, "sgd_long_tiny_p": 51, "adagrad_long_p": 20, "adagrad_long_m": 8.7,
            "adagrad_long_tiny_p": 270, "adagrad_long_tiny_m": 0.13, "rmsprop_long_p": 19, "rmsprop_long_m": 7.3,
            "rmsprop_long_tiny_p": 89, "rmsprop_long_tiny_m": 7.3, "adam_real_p": 7.5, "adam_real_m": 1.9,
            "adam_real_v": 3.9, "rmsprop_real_p": 6.9, "rmsprop_real_m": 5.7}


def tol_const(key):
    return SAFETY * MEASURED[key]


def kind_of(name, kind, wd):
    """the key's middle part for a case of weight decay wd: SGD, Adagrad and RMSprop at 1e-6 have keys of their own (above)"""
    return kind + "_tiny" if name != "adam" and wd == 1e-6 else kind


def wide_end_steps(cap=CAP_SMALL):
    """`to` of the wide list: 13 makes from = 0 occur (a row never touched: bc1 = 1 - beta1 at its first step), the others put
    `from` below, on and above `cap`"""
    return (13, 14, cap - 1, cap, cap + 1, cap + 5, cap + 70)


def narrow_end_steps(cap=CAP_SMALL):
    return (130, cap - 1, cap, cap + 1, cap + 5, cap + 70)


# ---- hyper-parameters ----------------------------------------------------------------------------------------------------------

def make_hyper(name, wd, device="cpu", betas=BETAS_SMALL, lr_decay=0.0):
    """The project's hyper object (host scalar table included) for a learner, asserting the table it is built for."""
    if name == "adam":
        h = AdamHyper(LR["adam"], wd, betas=betas, cap=8, device=device)
        assert h.saturated and h.cap == (CAP_SMALL if tuple(betas) == BETAS_SMALL else CAP_DEFAULT), (h.saturated, h.cap)
    elif name == "sgd":
        h = SGDHyper(LR["sgd"], wd, device=device)
        assert h.saturated and h.cap == 1
    elif name == "adagrad":
        h = AdagradHyper(LR_ADAGRAD_DECAY if lr_decay else LR["adagrad"], lr_decay=lr_decay, weight_decay=wd, device=device)
        # (with lr_decay the table grows until clr stops changing in float32, or to 2^22 entries: far beyond every step here)
        assert (h.cap >= 1 << 20) if lr_decay else (h.saturated and h.cap == 1), (h.saturated, h.cap)
    else:
        h = RMSpropHyper(LR["rmsprop"], weight_decay=wd, device=device)
        assert h.saturated and h.cap == 1
    h.name = name
    return h


def hp_of(h):
    """what the float64 reference may know: torch's constructor arguments"""
    if h.name == "adam":
        return SimpleNamespace(name="adam", lr=h.lr, wd=h.weight_decay, b1=h.betas[0], b2=h.betas[1], eps=h.eps)
    if h.name == "adagrad":
        return SimpleNamespace(name="adagrad", lr=h.lr, wd=h.weight_decay, lr_decay=h.lr_decay, eps=h.eps)
    if h.name == "rmsprop":
        return SimpleNamespace(name="rmsprop", lr=h.lr, wd=h.weight_decay, alpha=h.alpha, eps=h.eps)
    return SimpleNamespace(name="sgd", lr=h.lr, wd=h.weight_decay)


def has_m(name):
    return name != "sgd"


def has_v(name):
    return name == "adam"


# ---- float64 reference ---------------------------------------------------------------------------------------------------------

def _ref_one(hp, p, m, v, j, gd):
    """step j on float64 arrays with data gradient gd"""
    g = gd + hp.wd * p
    if hp.name == "adam":
        m = m + (1.0 - hp.b1) * (g - m)                       # exp_avg.lerp_(grad, 1 - beta1)
        v = hp.b2 * v + (1.0 - hp.b2) * g * g
        bc1, bc2 = 1.0 - hp.b1 ** j, 1.0 - hp.b2 ** j
        return p - (hp.lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + hp.eps), m, v
    if hp.name == "sgd":
        return p - hp.lr * g, m, v
    if hp.name == "adagrad":
        clr = hp.lr / (1.0 + (j - 1) * hp.lr_decay)
        m = m + g * g
        return p - clr * g / (np.sqrt(m) + hp.eps), m, v
    m = hp.alpha * m + (1.0 - hp.alpha) * g * g
    return p - hp.lr * g / (np.sqrt(m) + hp.eps), m, v


def ref_replay(hp, p, m, v, frm, to, grads=None, track=None):
    """Rows [n, D] in float64 through the steps (frm[r], to]; grads = {step: [n, D] data gradient} (absent: zero).
    -> (p, m, v); `track` (a list) receives min |p| and whether a sign changed."""
    p = np.array(p, dtype=np.float64)
    m = np.array(m, dtype=np.float64) if m is not None else np.zeros_like(p)
    v = np.array(v, dtype=np.float64) if v is not None else np.zeros_like(p)
    frm = np.asarray(frm, dtype=np.int64).reshape(-1, 1)
    sign0, lo = np.sign(p), np.abs(p).min()
    flipped = False
    for j in range(int(frm.min()) + 1, int(to) + 1):
        on = j > frm
        gd = np.asarray(grads[j], dtype=np.float64) if grads and j in grads else 0.0
        pn, mn, vn = _ref_one(hp, p, m, v, j, gd)
        p, m, v = np.where(on, pn, p), np.where(on, mn, m), np.where(on, vn, v)
        lo = min(lo, np.abs(p).min())
        flipped = flipped or bool((np.sign(p) != sign0).any())
    if track is not None:
        track.append((lo, flipped))
    return p, m, v


def assert_conditioned(track):
    for lo, flipped in track:
        assert not flipped and lo >= MIN_ABS_P, f"the reference is not well conditioned here: min |p| = {lo}, sign change {flipped}"


# ---- float32 restatement of the device code ------------------------------------------------------------------------------------

def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def _rcp(x):
    return (F(1.0) / x).astype(F)


def consts(h):
    """AdamC as make_adamc builds it from fr_adam"""
    a = h.c()
    wd, b1, b2, eps = a.weight_decay, a.beta1, a.beta2, a.eps
    k1, k2 = (1.0 - b1) * wd, (1.0 - b2) * wd * wd
    return SimpleNamespace(name=h.name, tab=h.host_scalars.reshape(-1, 4), cap=h.cap, wd=F(wd), b1=F(b1), omb1=F(1.0 - b1),
                           b2=F(b2), omb2=F(1.0 - b2), eps=F(eps), k1=F(k1), k2=F(k2),
                           inv_k1=F(1.0 / k1) if wd != 0.0 else F(0), inv_k2=F(1.0 / k2) if wd != 0.0 else F(0))


def _entry(c, j):
    return c.tab[min(j, c.cap)]


def _zero32(c, p, m, v, j, scaled):
    s = _entry(c, j)
    if c.name == "adam":
        if scaled:
            m = _fma(c.b1, m, p)
            v = _fma(c.b2, v, p * p)
            den = _fma(np.sqrt(v), s[2], s[3])
            return _fma(-m, _rcp(den), p), m, v
        m = _fma(c.k1, p, c.b1 * m)
        v = _fma(c.k2 * p, p, c.b2 * v)
        den = _fma(np.sqrt(v), s[1], c.eps)
        return _fma(-s[0] * m, _rcp(den), p), m, v
    if c.name == "sgd":
        return _fma(s[1], p, p), m, v
    if c.name == "rmsprop" and c.wd == 0:
        return p, m * c.b2, v
    g = c.wd * p
    m = _fma(g, g, m) if c.name == "adagrad" else _fma(c.omb2 * g, g, m * c.b2)
    return _fma(-s[0] * g, _rcp(np.sqrt(m) + c.eps), p), m, v


def _elem32(c, p, m, v, j, gd):
    s = _entry(c, j)
    g = _fma(c.wd, p, gd)
    if c.name == "adam":
        m = _fma(c.omb1, g - m, m)
        v = _fma(c.omb2 * g, g, v * c.b2)
        den = _fma(np.sqrt(v), s[1], c.eps)
        return _fma(-s[0] * m, _rcp(den), p), m, v
    if c.name == "sgd":
        return _fma(-s[0], g, p), m, v
    m = _fma(g, g, m) if c.name == "adagrad" else _fma(c.omb2 * g, g, m * c.b2)
    return _fma(-s[0] * g, _rcp(np.sqrt(m) + c.eps), p), m, v


def _identity(c):
    return c.name in ("sgd", "adagrad") and c.wd == 0


def f32_replay(c, p, m, v, frm, to):
    """one replay call per row: rows [n, D] float32 through the zero-gradient steps (frm[r], to]; a row with frm >= to comes
    back as it went in (no scaling round trip)"""
    frm = np.asarray(frm, dtype=np.int64).reshape(-1, 1)
    act = frm < to
    if _identity(c) or not act.any():
        return p, m, v
    scaled = c.name == "adam" and c.k1 != 0
    p0, m0, v0 = p, m, v
    if scaled:
        m, v = m * c.inv_k1, v * c.inv_k2
    for j in range(int(frm.min()) + 1, int(to) + 1):
        on = j > frm
        pn, mn, vn = _zero32(c, p, m, v, j, scaled)
        p, m, v = np.where(on, pn, p), np.where(on, mn, m), np.where(on, vn, v)
    if scaled:
        m, v = m * c.k1, v * c.k2
    return np.where(act, p, p0), np.where(act, m, m0), np.where(act, v, v0)


def f32_run(h, p, m, v, ops):
    """The device's sequence of calls on a table [n, D] in float32.  ops: ("replay", rows, frm, to) -- one replay call per row
    of `rows`, from its own frm -- or ("real", rows, step, G) -- step `step` with the data gradients G [len(rows), D]."""
    c = consts(h)
    p = np.array(p, dtype=F)
    m = np.array(m, dtype=F) if m is not None else np.zeros_like(p)
    v = np.array(v, dtype=F) if v is not None else np.zeros_like(p)
    for op in ops:
        rows = np.asarray(op[1], dtype=np.int64)
        if rows.size == 0:
            continue
        if op[0] == "replay":
            p[rows], m[rows], v[rows] = f32_replay(c, p[rows], m[rows], v[rows], op[2], op[3])
        else:
            p[rows], m[rows], v[rows] = _elem32(c, p[rows], m[rows], v[rows], op[2], np.asarray(op[3], dtype=F))
    return p, m, v


# ---- errors in the units of the tolerances -------------------------------------------------------------------------------------

def units(name, got, ref):
    """{'p': ..., 'm': ..., 'v': ...}: per-element error of got = (p, m, v) against ref in units of u |ref| (p) and of
    u (|ref| + max |ref| over the tensor) (the states the learner keeps)"""
    out = {}
    for k, key in enumerate("pmv"[:len(got)]):          # (got = (p,): the parameters alone)
        if key == "m" and not has_m(name) or key == "v" and not has_v(name):
            continue
        r = np.asarray(ref[k], dtype=np.float64)
        e = np.abs(np.asarray(got[k], dtype=np.float64) - r)
        out[key] = e / (U * np.abs(r)) if key == "p" else e / (U * (np.abs(r) + np.abs(r).max()))
    return out


def assert_close(name, kind, got, ref, what=""):
    """got against the float64 reference at tol_const(<name>_<kind>_<p|m|v>)"""
    for key, e in units(name, got, ref).items():
        tol = tol_const(f"{name}_{kind}_{key}")
        assert np.isfinite(e).all() and (e <= tol).all(), \
            f"{what} {name} {key}: worst {np.nanmax(e):.4g} units at {np.unravel_index(np.nanargmax(e), e.shape)}, allowed {tol:.4g}"


# ---- builders ------------------------------------------------------------------------------------------------------------------

def table_values(n_rows, D, seed=0):
    """(p, m, v) float32 [n_rows, D]: |p| in [0.05, 0.2] with random sign, m ~ N(0, 0.01), v in [1e-4, 1.1e-3].  A learner that
    keeps one state array (Adagrad's sum, RMSprop's square_avg) takes v for it: they are sums of squares."""
    rng = np.random.default_rng([seed, n_rows, D])
    p = (rng.uniform(0.05, 0.2, (n_rows, D)) * rng.choice([-1.0, 1.0], (n_rows, D))).astype(F)
    m = (rng.standard_normal((n_rows, D)) * 0.01).astype(F)
    v = rng.uniform(1e-4, 1.1e-3, (n_rows, D)).astype(F)
    assert (np.abs(p) >= 0.05).all() and (np.abs(p) <= F(0.2)).all() and (v >= F(1e-4)).all()
    return p, m, v


def state_of(name, m, v):
    """the (m, v) arrays of a table of this learner"""
    return (m, v) if name == "adam" else ((v, None) if has_m(name) else (None, None))


def flush_case(name, D, to, ages=WIDE, reps=1, seed=0):
    """A stale table: row r is ages[r % len(ages)] steps behind `to`.  -> SimpleNamespace(p, m, v, s, frm, to)"""
    s = np.array([a for a in ages if a <= to] * reps, dtype=np.int64)
    assert s.size and (to - s >= 0).all()
    p, m, v = table_values(s.size, D, seed)
    m, v = state_of(name, m, v)
    return SimpleNamespace(p=p, m=m, v=v, s=s, frm=to - s, to=int(to), n_rows=s.size, D=D)


NARROW_ROWS = (1, 63, 64, 65, 130)


def narrow_ages(n_rows, to, kind="mixed"):
    """ages of a D == 1 table: `mixed` = the narrow list and LONGEST shuffled over the rows (every age that fits below `to`
    occurs once n_rows allows), `current` = nobody behind (the wave returns early), `single` = one stale lane"""
    if kind == "current":
        return np.zeros(n_rows, dtype=np.int64)
    if kind == "single":
        s = np.zeros(n_rows, dtype=np.int64)
        s[min(37, n_rows - 1)] = 65
        return s
    pool = [a for a in NARROW + (LONGEST,) if a <= to]
    rng = np.random.default_rng([n_rows, to])
    s = np.array([pool[(k * 7 + 3) % len(pool)] for k in range(n_rows)], dtype=np.int64)
    if n_rows >= len(pool):
        assert set(s.tolist()) == set(pool)
    return rng.permutation(s)


def narrow_case(name, n_rows, to, kind="mixed", seed=1):
    s = narrow_ages(n_rows, to, kind)
    p, m, v = table_values(n_rows, 1, seed)
    m, v = state_of(name, m, v)
    return SimpleNamespace(p=p, m=m, v=v, s=s, frm=to - s, to=int(to), n_rows=n_rows, D=1)


def miscount(hp, case):
    """the reference one step short and one step long: -> [(p, m, v) at to - 1, (p, m, v) at to + 1]; a row that is current
    stays as it is in both"""
    frm = case.frm
    out = []
    for to in (case.to - 1, case.to + 1):
        f = np.where(case.s >= 1, frm, to)          # current rows: no step at all
        out.append(ref_replay(hp, case.p, case.m, case.v, f, to))
    return out


# ---- the sweeper slice: bookkeeping on the integers ----------------------------------------------------------------------------

def sweep_range(n_rows, step, S):
    """kernels.hpp: the slice of rows the sweeper takes at `step` with period S"""
    if S <= 0:
        return 0, 0
    chunk = (n_rows + S - 1) // S
    lo = (step % S) * chunk
    return min(lo, n_rows), min(lo + chunk, n_rows)


SWEEP_SHAPES = ((5, 4), (10, 4), (129, 2), (130, 3))     # (5, 4): an empty last slice; (10, 4): a short one; (129, 2): tails
SWEEP_WIDTHS = (1, 2, 64, 65)
SWEEP_STEP0 = 21
# ages of the rows (2k, 2k + 1), cycling: equal; ta < tb and tb < ta with differences 1, 3, 4, 9; one row current; both current.
# (By the step that sweeps it a row that started current is one step behind: outside a batch the sweeper meets no current row,
# and a pair of which only one row is replayed is a pair with the other row in the batch.)
PAIR_AGES = ((3, 3), (2, 1), (1, 2), (4, 1), (1, 4), (6, 2), (2, 6), (10, 1), (1, 10), (0, 5), (5, 0), (0, 0), (13, 13), (7, 8))


def sweep_scenario(n_rows, S, D, seed=2):
    """Table values, initial ages and S + 2 batches for consecutive steps SWEEP_STEP0 + 1 ...: 3 to 8 ids with a duplicate
    inside the batch and, where that step's slice is not empty, one id inside it."""
    rng = np.random.default_rng([seed, n_rows, S])
    ages = np.array([PAIR_AGES[(r // 2) % len(PAIR_AGES)][r % 2] for r in range(n_rows)], dtype=np.int64)
    p, m, v = table_values(n_rows, D, seed)
    batches, grads = [], []
    for t in range(SWEEP_STEP0 + 1, SWEEP_STEP0 + S + 3):
        lo, hi = sweep_range(n_rows, t, S)
        k = int(rng.integers(3, 9))
        ids = rng.integers(0, n_rows, k)
        if hi > lo:
            ids[0] = rng.integers(lo, hi)
        ids[-1] = ids[int(rng.integers(0, k - 1))]                       # a duplicate inside the batch
        ids = rng.permutation(ids)
        assert 3 <= ids.size <= 8 and len(set(ids.tolist())) < ids.size and (hi == lo or ((ids >= lo) & (ids < hi)).any())
        batches.append(ids.astype(np.int64))
        grads.append((rng.standard_normal((k, D)) * 0.01).astype(F))
    return SimpleNamespace(p=p, m=m, v=v, ages=ages, step0=SWEEP_STEP0, batches=batches, grads=grads, n_rows=n_rows, S=S, D=D)


def batch_grad32(n_rows, ids, g):
    """the duplicate-summed gradient rows as segment_grad_sum adds them: float32, ascending batch position, from zero"""
    G = np.zeros((n_rows, g.shape[1]), dtype=F)
    for j, r in enumerate(ids):
        G[r] = G[r] + g[j]
    return G


def schedule(sc, pairs, sweeps=True):
    """fr_table_gather_train + fr_table_apply_grad(sweep = S) over the scenario's steps, on the integers.
    -> SimpleNamespace(ops for f32_run (a final flush included), last[t], stamp[t] after every step, pair_kinds seen)"""
    n = sc.n_rows
    last = sc.step0 - sc.ages
    stamp = np.zeros(n, dtype=np.int64)
    ops, lasts, stamps, kinds = [], [], [], set()
    for i, ids in enumerate(sc.batches):
        t = sc.step0 + 1 + i
        rows = np.unique(ids)
        stamp[rows] = t                                                  # gather_train_row
        ops.append(("replay", rows, last[rows].copy(), t - 1))
        lo, hi = sweep_range(n, t, sc.S) if sweeps else (0, 0)
        todo = lambda r: stamp[r] < t and last[r] < t                    # noqa: E731  (the sweeper's test for one row)
        if pairs:
            for a in range(lo, hi, 2):
                b = a + 1 if a + 1 < hi else -1
                if b >= 0 and todo(a) and todo(b):
                    ta, tb = int(last[a]), int(last[b])
                    kinds.add(("stagger", abs(ta - tb)) if ta != tb else ("equal", 0))
                    if ta != tb:                                        # the older row alone first, then both together
                        old = a if ta < tb else b
                        ops.append(("replay", [old], [min(ta, tb)], max(ta, tb)))
                    ops.append(("replay", [a, b], [max(ta, tb)] * 2, t))
                else:
                    for r in (a, b):
                        if r >= 0 and todo(r):
                            ops.append(("replay", [r], [int(last[r])], t))
                            if (b if r == a else a) >= 0:
                                kinds.add(("partner in batch", 0))
        else:
            sw = np.array([r for r in range(lo, hi) if todo(r)], dtype=np.int64)
            ops.append(("replay", sw, last[sw].copy(), t))
        for r in range(lo, hi):
            if todo(r):
                last[r] = t
        ops.append(("real", rows, t, batch_grad32(n, ids, sc.grads[i])[rows]))       # segment_update
        last[rows] = t
        lasts.append(last.copy())
        stamps.append(stamp.copy())
    T = sc.step0 + len(sc.batches)
    ops.append(("replay", np.arange(n), last.copy(), T))                             # the flush
    return SimpleNamespace(ops=ops, last=lasts, stamp=stamps, kinds=kinds, T=T)


def scenario_ref(hp, sc, state):
    """every row on its own in float64: a real step with the duplicate-summed gradient where it is in the batch, a
    zero-gradient step where it is not"""
    grads = {}
    for i, ids in enumerate(sc.batches):
        G = np.zeros((sc.n_rows, sc.D), dtype=np.float64)
        np.add.at(G, ids, sc.grads[i].astype(np.float64))
        grads[sc.step0 + 1 + i] = G
    return ref_replay(hp, sc.p, state[0], state[1], sc.step0 - sc.ages, sc.step0 + len(sc.batches), grads)


def stale_batch(D, to, seed=3):
    """Adam's real step `to` at stale rows: a table carrying the wide list three times over, a batch that holds every row of
    the first two thirds once and two of them twice.  -> SimpleNamespace(case, ids, g)"""
    case = flush_case("adam", D, to - 1, WIDE, reps=3, seed=seed)          # ages relative to to - 1: from = to - 1 - s
    rng = np.random.default_rng([seed, D, to])
    n_b = 2 * case.n_rows // 3
    ids = np.concatenate([rng.permutation(n_b), [1, n_b - 1]]).astype(np.int64)
    g = (rng.standard_normal((ids.size, D)) * 0.01).astype(F)
    return SimpleNamespace(case=case, ids=ids, g=g, to=int(to))

"""Float64 reference of the FOCF loss and its gradient (csrc/focf_ws.hpp: focf_objective / focf_fair_eval, csrc/focf_step.hip:
focf_fair_single, and the five step forms that go through them) and the inputs their tests run on: plain numpy on the CPU, no
GPU, no fairrec.  tests/test_focf_ref.py pins the reference to oracle.focf.loss on float64 tensors under torch autograd and
checks what the builders promise; tests/test_focf_loss_hip.py compares every step form with it.

* `focf_loss` takes the kernels' float32 inputs and computes in float64, in closed form per item and per group (no autograd):
  pred, MSE, the per-item group means with the `count + 1e-5` denominator, d_g of the objective, delta = d_0 - d_1, the
  smooth-L1 term, dLoss/dpred per interaction, the dense gradients summed over duplicates and their 2-norm.  Group 0 is the
  smaller sst value present; a batch with one value present has only column 0 (the other column's P = T = 0); `nonparity`
  with one value present reports fair = 0 and the MSE gradient alone (what the kernels write there, next to the device error
  word that the engine raises as the reference's IndexError; the reference itself raises).  The kinks
  are torch's: abs'(0) = 0, clamp(x, min=0)' = 1 at x == 0, smooth-L1' at 0 is 0.
* Bounds carried with the result: A[row, d] = sum_b |coef_b| |other_row_b[d]| over the row's members, the bound a gradient
  entry is compared in; the loss values are sums of non-negative terms (sum_b e_b / B, sum_k term_k / K), so they are their
  own bounds.
* `adam_first_step`: Adam from zero state with weight_decay = 0, m = (1 - b1) g, v = (1 - b2) g^2: the tests read a gradient
  out of an engine as m / (1 - b1).
* `predict`: clamp(pred, 0, max) / max.
* Builders (`segments`, `one_sided`, `encodings`, `regimes`, `exact_kinks`, `counts`): each asserts in float64 what it is
  built for.  Tables have at most about 700 rows; widths WIDTHS hold one width per row-fragment count (64 columns a fragment)
  with full and partial fragments.

Tolerances take the form the project uses elsewhere, a constant MEASURED[key] * 8 on a unit that follows from the bounds:
  u A            for gradient entries ("grad") and for m / (1 - b1) ("m"),
  u (|ref| + bound)  for the three loss values ("loss", "mse", "fair"),
  u |ref|        for the gradient norm ("norm"),
and for v the bound that follows from the gradient's: (1 - b2) (2 |g| tol_g + tol_g^2) + u |v|.
MEASURED["<quantity>_<builder>"] is the worst error against float64 of the reference's own float32 arithmetic -- oracle.focf.loss with autograd
in float32, oracle.focf.train(..., snaps=(1,)) for m and v -- on that builder's inputs, in those units (most of it is the
conditioning of the inputs, which the units do not see: pred - rating and the group means P - T, d_0 - d_1 are differences of
numbers of size 3; `ill_conditioned` keeps the builders' rows away from the worst of it); times 4 for another
order of summation and fused multiply-adds, times 2 so that another seed does not flip a test.  tests/test_focf_ref.py prints
the measurement and asserts it against MEASURED (not above, and at least half), so the constants measure the REFERENCE side,
never a kernel.
"""
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
B1, B2 = 0.9, 0.999
SAFETY = 8.0
WIDTHS = (40, 64, 100, 128, 256)
PER_ITEM = ("value", "absolute", "under", "over")
OBJECTIVES = ("none",) + PER_ITEM + ("nonparity",)
MARGIN = 1e-3
FAIR_WEIGHT = 0.7

QUANTITIES = ("loss", "mse", "fair", "grad", "m", "norm")
BUILDERS = ("segments", "regimes", "one_sided", "encodings", "counts", "exact_kinks")
# "<quantity>_<builder>": worst error of the float32 reference on that builder's inputs, in the units above
FLOOR = 1.0       # a measurement below one unit is recorded as one: the rounding of the result itself, in any order of evaluation
MEASURED = {
    "loss_segments": 1.2, "mse_segments": 1, "fair_segments": 51, "grad_segments": 240, "m_segments": 240, "norm_segments": 26,
    "loss_regimes": 1.2, "mse_regimes": 1, "fair_regimes": 21, "grad_regimes": 180, "m_regimes": 180, "norm_regimes": 15,
    "loss_one_sided": 1.9, "mse_one_sided": 1.2, "fair_one_sided": 7.9, "grad_one_sided": 78, "m_one_sided": 79, "norm_one_sided": 5,
    "loss_encodings": 1.1, "mse_encodings": 1, "fair_encodings": 40, "grad_encodings": 190, "m_encodings": 190, "norm_encodings": 12,
    "loss_counts": 7, "mse_counts": 3.4, "fair_counts": 180, "grad_counts": 830, "m_counts": 830, "norm_counts": 160,
    "loss_exact_kinks": 1, "mse_exact_kinks": 1, "fair_exact_kinks": 3, "grad_exact_kinks": 2.6, "m_exact_kinks": 2.6, "norm_exact_kinks": 1.6,
}


def tol_const(key):
    return SAFETY * MEASURED[key]


# ---- the reference -----------------------------------------------------------------------------------------------------------

def _objective(objective, P, T):
    """d_g = f(P_g - T_g) and q_g = d d_g / d P_g, [K, 2] each, kinks as torch takes them"""
    a = P - T
    if objective == "value":
        return a, np.ones_like(a)
    if objective == "absolute":
        return np.abs(a), np.sign(a)                                # abs'(0) = 0
    if objective == "under":
        return np.maximum(-a, 0.0), np.where(-a >= 0.0, -1.0, 0.0)  # clamp(T - P, min=0): the mask is x >= min
    if objective == "over":
        return np.maximum(a, 0.0), np.where(a >= 0.0, 1.0, 0.0)
    raise ValueError(objective)


def _sl1(x):
    """smooth-L1 (beta = 1) of x and its derivative"""
    ax = np.abs(x)
    return np.where(ax < 1.0, 0.5 * ax * ax, ax - 0.5), np.where(ax < 1.0, x, np.sign(x))


def focf_loss(objective, fair_weight, U_, I_, user, item, rating, sst, grads=True):
    """-> SimpleNamespace(loss, mse, fair, pred [B], dpred [B] = dLoss/dpred, gradU, gradI (dense, summed over duplicates),
    AU, AI (their bounds), norm, rows_u, rows_i (the rows of the batch), and per item (in ascending item id): items, n, P, T
    [K, 2], d [K, 2], delta, term [K]; for nonparity gmean [2] instead)"""
    objective = objective.strip().lower()
    U64, I64 = np.asarray(U_, dtype=np.float64), np.asarray(I_, dtype=np.float64)
    user, item = np.asarray(user, dtype=np.int64), np.asarray(item, dtype=np.int64)
    rating = np.asarray(rating, dtype=np.float64)
    B = user.shape[0]
    ue, ie = U64[user], I64[item]
    pred = (ue * ie).sum(-1)
    err = pred - rating
    r = SimpleNamespace(pred=pred, mse=float((err * err).sum() / B), fair=0.0)
    fpart = np.zeros(B)
    if objective != "none":
        s = np.asarray(sst, dtype=np.float64)
        vals, g = np.unique(s, return_inverse=True)
        assert len(vals) <= 2, "the reference forms one difference: two groups"
        if objective == "nonparity":
            r.gmean = np.array([pred[g == c].mean() if (g == c).any() else 0.0 for c in range(2)])
            if len(vals) == 2:
                t, dt = _sl1(r.gmean[0] - r.gmean[1])
                r.fair = float(t)
                cnt = np.bincount(g, minlength=2).astype(np.float64)
                fpart = np.where(g == 0, dt / cnt[0], -dt / cnt[1])
        else:
            items, k = np.unique(item, return_inverse=True)
            K = len(items)
            sp, st, n = np.zeros((K, 2)), np.zeros((K, 2)), np.zeros((K, 2))
            np.add.at(sp, (k, g), pred)
            np.add.at(st, (k, g), rating)
            np.add.at(n, (k, g), 1.0)
            c = n + 1e-5
            P, T = sp / c, st / c
            d, q = _objective(objective, P, T)
            delta = d[:, 0] - d[:, 1]
            term, dterm = _sl1(np.abs(delta))
            ddelta = dterm * np.sign(delta) / K                     # d mean_k sl1(|delta_k|) / d delta_k; abs'(0) = 0
            gg = np.stack([ddelta, -ddelta], 1) * q / c             # ... / d pred of a member of group 0 / 1
            fpart = gg[k, g]
            r.fair = float(term.sum() / K)
            r.items, r.n, r.P, r.T, r.d, r.delta, r.term, r.K = items, n, P, T, d, delta, term, K
    r.loss = r.mse + fair_weight * r.fair
    r.dpred = 2.0 * err / B + fair_weight * fpart
    if not grads:                       # (the builders ask per interaction only)
        return r
    r.gradU, r.gradI = np.zeros_like(U64), np.zeros_like(I64)
    r.AU, r.AI = np.zeros_like(U64), np.zeros_like(I64)
    np.add.at(r.gradU, user, r.dpred[:, None] * ie)
    np.add.at(r.gradI, item, r.dpred[:, None] * ue)
    np.add.at(r.AU, user, np.abs(r.dpred)[:, None] * np.abs(ie))
    np.add.at(r.AI, item, np.abs(r.dpred)[:, None] * np.abs(ue))
    r.norm = float(np.sqrt((r.gradU ** 2).sum() + (r.gradI ** 2).sum()))
    r.rows_u, r.rows_i = np.unique(user), np.unique(item)
    return r


def adam_first_step(g):
    """Adam from zero state, weight_decay = 0 -> (m, v)"""
    g = np.asarray(g, dtype=np.float64)
    return (1.0 - B1) * g, (1.0 - B2) * g * g


def v_tolerance(g, tol_g):
    """the bound on v that follows from the bound tol_g on the gradient"""
    g = np.abs(np.asarray(g, dtype=np.float64))
    return (1.0 - B2) * (2.0 * g * tol_g + tol_g * tol_g) + U * (1.0 - B2) * g * g


def predict(U_, I_, user, item, max_rating):
    p = (np.asarray(U_, np.float64)[np.asarray(user)] * np.asarray(I_, np.float64)[np.asarray(item)]).sum(-1)
    return np.clip(p, 0.0, max_rating) / max_rating


# ---- batches -----------------------------------------------------------------------------------------------------------------

class Batch:
    """Tables U [n_users, D], I [n_items, D] (float32) and the columns of one batch, kept item-contiguous; `cols(False)`
    gives them in a fixed shuffled order, `cols(True)` item-contiguous (what the run forms need)."""

    def __init__(self, name, U_, I_, user, item, rating, sst, seed=0):
        self.name, self.U, self.I = name, np.ascontiguousarray(U_, np.float32), np.ascontiguousarray(I_, np.float32)
        self.user, self.item = np.asarray(user, np.int64), np.asarray(item, np.int64)
        self.rating, self.sst = np.asarray(rating, np.float32), np.asarray(sst, np.float32)
        self.B, self.D = len(self.user), self.U.shape[1]
        assert len(self.item) == len(self.rating) == len(self.sst) == self.B
        assert self.user.min() >= 0 and self.user.max() < self.U.shape[0] and self.item.min() >= 0 and self.item.max() < self.I.shape[0]
        change = np.flatnonzero(np.diff(self.item) != 0)
        assert len(np.unique(self.item)) == len(change) + 1, "not item-contiguous"
        self.perm = np.random.default_rng([seed, self.B, 11]).permutation(self.B)

    def cols(self, contiguous):
        o = np.arange(self.B) if contiguous else self.perm
        return self.user[o], self.item[o], self.rating[o], self.sst[o]

    def seg_lengths(self):
        return np.unique(self.item, return_counts=True)[1]


def _tables(rng, n_users, n_items, D):
    """Rows whose dot products are sums of positive terms (a column has one sign in both tables, half of the columns are
    negative), so a float32 prediction is as good as its D terms allow: about 3 times a factor per user row and a factor per
    item row, each in (0.6, 1.4) -- predictions on both sides of ratings 1 .. 5."""
    sign = np.where(rng.permutation(D) % 2 == 0, 1.0, -1.0)
    a = np.sqrt(12.0 / D)
    U_ = rng.uniform(0.0, a, (n_users, D)) * sign * rng.uniform(0.6, 1.4, (n_users, 1))
    U_[1::2] *= 1.12                  # odd ids are group 1: the groups' mean predictions differ (nonparity does not cancel)
    I_ = rng.uniform(0.0, a, (n_items, D)) * sign * rng.uniform(0.6, 1.4, (n_items, 1))
    return U_.astype(np.float32), I_.astype(np.float32)


def _fill(rng, groups_per_item, n_users, n_items, fixed_users=None):
    """groups_per_item: one list of group ids (0 / 1) per item -> user, item, gender-consistent sst columns, item-contiguous.
    Users are distinct, even ids for group 0 and odd ids for group 1 (sst is a user's attribute), items are random distinct
    ids; both tables keep rows no interaction touches, the first and the last row of each are used."""
    K = len(groups_per_item)
    assert K <= n_items - 2
    ids = rng.permutation(np.arange(1, n_items - 1))[:K - 2].tolist() if K > 2 else []
    ids = ([0, n_items - 1] + ids)[:K]
    pools = [list(rng.permutation(np.arange(0, n_users, 2))), list(rng.permutation(np.arange(1, n_users, 2)))]
    for g, first in ((0, 0), (1, n_users - 1 if (n_users - 1) % 2 else n_users - 2)):      # table edges first
        pools[g].remove(first)
        pools[g].append(first)
    user, item, sst = [], [], []
    for k, groups in enumerate(groups_per_item):
        for g in groups:
            user.append(int(pools[g].pop()))
            item.append(ids[k])
            sst.append(float(g))
    return np.array(user), np.array(item), np.array(sst)


def _mixed(rng, n):
    """n group ids, both groups present from n = 2 on"""
    g = rng.permutation(np.arange(n) % 2) if n >= 2 else rng.integers(0, 2, n)
    if n >= 2:
        g[0], g[1] = 0, 1
    return g.tolist()


ERR_MIN, PART_MIN, GAP_MIN, DELTA_MIN, PARITY_MIN = 0.25, 0.1, 0.02, 0.2, 0.1


class _Redraw(Exception):
    pass


def ill_conditioned(U_, I_, user, item, rating, sst, kink_margin=GAP_MIN, split=False):
    """[B] bool: interactions at which float32 cannot be compared in units of u A under some objective, because
    dLoss/dpred = 2 (pred - rating) / B + fair_weight g cancels -- |pred - rating| < ERR_MIN, or the sum below PART_MIN of its
    parts' sizes -- or because the interaction's item has a present group with |P - T| < kink_margin, or a delta within
    DELTA_MIN of 0 that is not 0 by both clamps (delta is a difference of means of size 3), or within MARGIN of 1.  Raises
    _Redraw where the two group means of nonparity are closer than PARITY_MIN (no rating changes that)."""
    bad, bad_item = np.zeros(len(user), dtype=bool), np.zeros(len(user), dtype=bool)
    two = len(np.unique(sst)) == 2
    for obj in OBJECTIVES:
        r = focf_loss(obj, FAIR_WEIGHT, U_, I_, user, item, rating, sst, grads=False)
        err = r.pred - np.asarray(rating, dtype=np.float64)
        cm = 2.0 * err / len(user)
        bad |= np.abs(err) < ERR_MIN
        bad |= np.abs(r.dpred) < PART_MIN * (np.abs(cm) + np.abs(r.dpred - cm))
        if obj in PER_ITEM:
            k = np.searchsorted(r.items, item)
            clamped = (r.d == 0).all(1) & (obj in ("under", "over"))
            badk = ((np.abs(r.P - r.T) < kink_margin) & (r.n > 0)).any(1)
            badk |= (np.abs(r.delta) < DELTA_MIN) & ~clamped
            badk |= np.abs(np.abs(r.delta) - 1.0) < MARGIN
            bad_item |= badk[k]
        elif obj == "nonparity" and two and abs(r.gmean[0] - r.gmean[1]) < PARITY_MIN:
            raise _Redraw("nonparity: the group means cancel")
    return (bad, bad_item) if split else bad | bad_item          # split: (by the interaction's own values, by its item's)


def _ratings(rng, U_, I_, user, item, sst):
    """Ratings 1 .. 5 that lean on the prediction: pred plus an offset of 0.5 .. 1.5 of either sign per (item, group) -- so a
    group mean P - T does not shrink with the group's size -- plus noise, rounded.  Where `ill_conditioned` names an
    interaction by its own values it gets any of the five ratings, where by its item's that item new offsets."""
    pred = (U_.astype(np.float64)[user] * I_.astype(np.float64)[item]).sum(-1)
    cell = np.unique(np.stack([item, (sst > sst.min()).astype(np.int64)]), axis=1, return_inverse=True)[1].reshape(-1)
    draw_offsets = lambda n: rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)
    offset = draw_offsets(cell.max() + 1)
    draw = lambda sel: np.clip(np.rint(pred[sel] + offset[cell[sel]] + rng.uniform(-1.0, 1.0, int(sel.sum()))), 1, 5).astype(np.float32)
    rating = draw(np.ones(len(user), dtype=bool))
    for attempt in range(400):
        bad, bad_item = ill_conditioned(U_, I_, user, item, rating, sst, split=True)
        if not (bad.any() or bad_item.any()):
            return rating
        rating[bad] = rng.integers(1, 6, int(bad.sum())).astype(np.float32)
        if bad_item.any():
            cells = np.unique(cell[bad_item])
            offset[cells] = draw_offsets(len(cells))
            again = np.isin(cell, cells)
            rating[again] = draw(again)
    raise _Redraw("ratings did not settle")


def _retry(build):
    """a builder draws again, from another stream, where its rows cannot be conditioned by the ratings alone"""
    def wrapped(*args, seed=0):
        for attempt in range(32):
            try:
                return build(*args, seed=seed, attempt=attempt)
            except _Redraw:
                continue
        raise AssertionError("no draw was well conditioned")
    wrapped.__doc__, wrapped.__name__ = build.__doc__, build.__name__
    return wrapped


def _check_conditioned(b, kink_margin=GAP_MIN):
    assert not ill_conditioned(b.U, b.I, *b.cols(True), kink_margin=kink_margin).any(), b.name
    return b


SEGMENT_LENGTHS = (1, 2, 15, 16, 17, 63, 64, 65, 129, 257)
USER_SEGMENTS = (1, 2, 65)


@_retry
def segments(D, seed=0, attempt=0):
    """Item segments of SEGMENT_LENGTHS members (around the 16 lanes the fairness kernel gives a segment, the wave, and item-run
    workgroups of several waves), each of two or more with both groups, plus 56 short items so that one user can sit in 65
    distinct items and the batch holds more than 64 distinct items (two fairness workgroups); user segments of 1, 2 and 65;
    one repeated (user, item) pair."""
    rng = np.random.default_rng([seed, D, 1, attempt])
    n_users, n_items = 800, 80
    groups = [_mixed(rng, n) for n in SEGMENT_LENGTHS] + [_mixed(rng, 1 + j % 2) for j in range(56)]
    groups[0] = [1]
    for k in range(10, 66):
        groups[k][0] = 0
    user, item, sst = _fill(rng, groups, n_users, n_items)
    start = np.concatenate(([0], np.cumsum([len(g) for g in groups])))
    hot = user[start[1]]                                    # group 0: the first member of 65 distinct items
    at = [start[k] for k in range(1, 66)]
    assert (sst[at] == 0).all()
    user[at] = hot
    two = user[start[2] + 1]                                # group 1: the second member of two items
    assert sst[start[3] + 1] == 1 == sst[start[2] + 1]
    user[start[3] + 1] = two
    a, c = start[9] + 5, start[9] + 9                       # the repeated pair, inside the longest item
    sst[c] = sst[a]
    user[c] = user[a]
    U_, I_ = _tables(rng, n_users, n_items, D)
    b = Batch("segments", U_, I_, user, item, _ratings(rng, U_, I_, user, item, sst), sst, seed)
    # what it is built for
    lengths = b.seg_lengths()
    assert set(SEGMENT_LENGTHS) <= set(lengths.tolist()) and len(lengths) > 64
    for k, n in enumerate(SEGMENT_LENGTHS):
        sel = b.sst[start[k]:start[k + 1]]
        assert len(sel) == n and (n < 2 or (sel.min() == 0 and sel.max() == 1))
    ucount = np.unique(b.user, return_counts=True)[1]
    assert set(USER_SEGMENTS) <= set(ucount.tolist()) and ucount.max() == 65
    pairs, pc = np.unique(np.stack([b.user, b.item]), axis=1, return_counts=True)
    assert (pc == 2).sum() == 1 and pc.max() == 2
    assert len(np.unique(b.item[b.user == hot])) == 65
    for u in np.unique(b.user):
        assert len(np.unique(b.sst[b.user == u])) == 1      # sst is a user's attribute
    su, si = set(b.user.tolist()), set(b.item.tolist())
    assert len(su) < n_users and len(si) < n_items          # rows outside the batch exist
    assert not np.array_equal(np.sort(b.cols(False)[1]), b.cols(False)[1])
    return _check_conditioned(b)


@_retry
def one_sided(D, seed=0, attempt=0):
    """Items whose members are all of group 0 and items whose members are all of group 1 (the absent group has P = T = 0),
    with 1 (the single-member path, in group 0 and in group 1), 2, 5, 17 and 70 members, between items that hold both groups."""
    rng = np.random.default_rng([seed, D, 2, attempt])
    groups, kind = [], []
    for n in (1, 2, 5, 17, 70):
        for g in (0, 1):
            groups.append(_mixed(rng, int(rng.integers(2, 20))))
            kind.append(-1)
            groups.append([g] * n)
            kind.append(g)
    groups.append(_mixed(rng, 3))
    kind.append(-1)
    user, item, sst = _fill(rng, groups, 500, 40)
    U_, I_ = _tables(rng, 500, 40, D)
    b = Batch("one_sided", U_, I_, user, item, _ratings(rng, U_, I_, user, item, sst), sst, seed)
    r = focf_loss("value", 1.0, b.U, b.I, *b.cols(True))
    first = {it: k for k, it in zip(kind, item[np.concatenate(([0], np.cumsum([len(g) for g in groups])[:-1]))])}
    for j, it in enumerate(r.items):
        g = first[it]
        if g >= 0:
            assert r.n[j, 1 - g] == 0 and r.n[j, g] > 0 and r.P[j, 1 - g] == 0.0 and r.T[j, 1 - g] == 0.0
        else:
            assert (r.n[j] > 0).all()
    for g in (0, 1):
        assert ((r.n.sum(1) == 1) & (r.n[:, g] == 1)).any()
    return _check_conditioned(b)


ENCODINGS = ("01", "12", "neg", "only0", "only1", "lone0")


@_retry
def encodings(D, which, seed=0, attempt=0):
    """The same rows under another coding of the sensitive attribute: {0, 1}, {1, 2}, {-1, 0.5}; one value only, as 0.0 and as
    1.0; and one interaction of group 0 beside B - 1 of group 1 (nonparity with n0 = 1)."""
    rng = np.random.default_rng([seed, D, 3, attempt])
    groups = [_mixed(rng, int(n)) for n in rng.integers(1, 9, 36)]
    if which == "lone0":
        groups = [[1] * len(g) for g in groups]
        groups[3][0] = 0
    user, item, sst = _fill(rng, groups, 400, 60)
    sst = {"01": sst, "12": sst + 1.0, "neg": np.where(sst == 0, -1.0, 0.5), "only0": sst * 0.0, "only1": sst * 0.0 + 1.0,
           "lone0": sst}[which]
    U_, I_ = _tables(rng, 400, 60, D)
    b = Batch("encodings_" + which, U_, I_, user, item, _ratings(rng, U_, I_, user, item, sst), sst, seed)
    vals, cnt = np.unique(b.sst, return_counts=True)
    want = {"01": [0, 1], "12": [1, 2], "neg": [-1, 0.5], "only0": [0], "only1": [1], "lone0": [0, 1]}[which]
    assert vals.tolist() == want
    if which == "lone0":
        assert cnt.tolist() == [1, b.B - 1]
    return _check_conditioned(b)


REGIME_ITEMS, REGIME_CELL = 96, 8


def _regime_cells(r):
    """the cells of one objective's record -> {name: number of items}"""
    a = r.P - r.T
    c = {}
    for g in (0, 1):
        c[f"P{g}>T{g}"] = int((a[:, g] > 0).sum())
        c[f"P{g}<T{g}"] = int((a[:, g] < 0).sum())
    c["|delta|<1"], c["|delta|>1"] = int((np.abs(r.delta) < 1).sum()), int((np.abs(r.delta) > 1).sum())
    c["delta>0"], c["delta<0"] = int((r.delta > 0).sum()), int((r.delta < 0).sum())
    return c


def _regime_bad(r):
    """items of one objective's record closer than MARGIN to a kink"""
    return ((np.abs(r.P - r.T) < MARGIN).any(1) | (np.abs(np.abs(r.delta) - 1.0) < MARGIN) | (np.abs(r.delta) < MARGIN))


@_retry
def regimes(D, seed=0, attempt=0):
    """REGIME_ITEMS items of 2 .. 6 members, both groups in each, ratings set so that the group means P - T of the two groups
    have opposite signs (under and over then have one active group each: no delta is 0 by a clamp on both sides) and sizes
    drawn from (0.3, 0.65) and (1.2, 3), every member within 15 % of its group's: every per-item objective sees, for each group, P > T and P < T, |delta| < 1 and
    |delta| > 1 and delta of both signs, in at least REGIME_CELL items each, and every item keeps MARGIN from every kink
    (|P - T|, ||delta| - 1|, |delta|) under every objective -- with that margin float32 and float64 take the same branches.
    Items that miss a margin, or hold an interaction that `ill_conditioned` names, get new ratings until none does."""
    rng = np.random.default_rng([seed, D, 4, attempt])
    n_users, n_items = 600, 120
    groups = [_mixed(rng, int(n)) for n in rng.integers(2, 7, REGIME_ITEMS)]
    user, item, sst = _fill(rng, groups, n_users, n_items)
    U_, I_ = _tables(rng, n_users, n_items, D)
    pred = (U_.astype(np.float64)[user] * I_.astype(np.float64)[item]).sum(-1)
    items = np.unique(item)
    rating = np.zeros(len(user), dtype=np.float32)
    todo = items
    for _ in range(500):
        for it in todo:
            j = int(np.searchsorted(items, it))
            sign = 1.0 if j % 2 else -1.0
            for g in (0, 1):
                big = (j // 2 + g * (j // 4)) % 2
                a = sign * (1 - 2 * g) * (rng.uniform(1.2, 3.0) if big else rng.uniform(0.3, 0.65))       # the target P_g - T_g
                sel = (item == it) & (sst == g)
                rating[sel] = (pred[sel] - a * rng.uniform(0.85, 1.15, int(sel.sum()))).astype(np.float32)
        bad = np.zeros(len(items), dtype=bool)
        bad[np.searchsorted(items, item[ill_conditioned(U_, I_, user, item, rating, sst)])] = True
        for obj in PER_ITEM:
            r = focf_loss(obj, 1.0, U_, I_, user, item, rating, sst, grads=False)
            bad |= _regime_bad(r)
            bad |= np.sign(r.P[:, 0] - r.T[:, 0]) == np.sign(r.P[:, 1] - r.T[:, 1])
        todo = items[bad]
        if not bad.any():
            break
    else:
        raise _Redraw("ratings did not settle")
    b = Batch("regimes", U_, I_, user, item, rating, sst, seed)
    b.cells = {}
    for obj in PER_ITEM:
        r = focf_loss(obj, 1.0, b.U, b.I, *b.cols(True))
        assert not _regime_bad(r).any(), (obj, "an item within the margin of a kink")
        b.cells[obj] = _regime_cells(r)
        assert min(b.cells[obj].values()) >= REGIME_CELL, (obj, b.cells[obj])
    return _check_conditioned(b)


def exact_kinks(D):
    """Rows a e_j and c e_j of small dyadic numbers (pred = a c exactly, in float32 and in float64), one coordinate per item.
    Item kinds -- (a) one group with P == T exactly while the other has d != 0 and 0 < |delta| < 1: `a_under*` (the other
    member's rating above its pred), `a_over*` (below); the kink in group 0 and in group 1, in a one-member group and in a
    group of two members whose sums agree (preds 2, 4 against ratings 4, 2).  (b) `b*`: both groups with identical sums and
    counts, delta == 0 exactly with d != 0: the fairness gradient is exactly 0.  `single*`: one member with pred == rating.
    -> Batch with .kind (item id -> name), .on_kink (positions, item-contiguous, of members of a group with P == T in a kind
    (a) item), .zero_fair (positions of the members of kind (b) items)."""
    rows = []       # (kind, [(group, pred, rating)])
    for kg in (0, 1):
        o = 1 - kg
        rows.append((f"a_under_g{kg}", [(kg, 3.0, 3.0), (o, 3.0, 3.5)]))
        rows.append((f"a_over_g{kg}", [(kg, 3.0, 3.0), (o, 3.0, 2.5)]))
        rows.append((f"a_under_pair_g{kg}", [(kg, 2.0, 4.0), (kg, 4.0, 2.0), (o, 3.0, 3.75)]))
        rows.append((f"a_over_pair_g{kg}", [(kg, 2.0, 4.0), (kg, 4.0, 2.0), (o, 3.0, 2.25), (o, 2.0, 1.5)]))
        rows.append((f"single_g{kg}", [(kg, 3.0, 3.0)]))
    rows.append(("b_under", [(0, 3.0, 4.0), (1, 3.0, 4.0)]))
    rows.append(("b_over", [(0, 4.0, 3.0), (1, 4.0, 3.0)]))
    rows.append(("b_pairs", [(0, 2.0, 4.0), (0, 3.0, 2.0), (1, 3.0, 2.0), (1, 2.0, 4.0)]))
    B = sum(len(m) for _, m in rows)
    n_users, n_items = 2 * B + 3, len(rows) + 5
    U_, I_ = np.zeros((n_users, D), np.float32), np.zeros((n_items, D), np.float32)
    user, item, rating, sst, kind, on_kink, zero_fair = [], [], [], [], {}, [], []
    for k, (name, members) in enumerate(rows):
        it = k + 2
        kind[it] = name
        I_[it, (7 * k) % D] = 2.0
        for g, p, rt in members:
            u = 2 * len(user) + 2 + g                               # even ids group 0, odd ids group 1
            U_[u, (7 * k) % D] = p / 2.0
            if name.startswith("a_") and g == int(name[-1]):
                on_kink.append(len(user))
            if name.startswith("b"):
                zero_fair.append(len(user))
            user.append(u); item.append(it); rating.append(rt); sst.append(float(g))
    b = Batch("exact_kinks", U_, I_, user, item, rating, sst)
    b.kind, b.on_kink, b.zero_fair = kind, np.array(on_kink), np.array(zero_fair)
    # the equalities, bitwise in float32: every pred is exact, a kink group's sums agree, kind (b) has equal sums per group
    p32 = (b.U[b.user] * b.I[b.item]).sum(-1, dtype=np.float32)
    want = np.array([p for _, m in rows for _, p, _ in m], dtype=np.float32)
    assert p32.dtype == np.float32 and (p32.view(np.int32) == want.view(np.int32)).all()
    for it, name in kind.items():
        sel = b.item == it
        s = lambda g, col: col[sel & (b.sst == g)].sum(dtype=np.float32)
        if name.startswith("a_"):
            g = int(name[-1])
            assert s(g, p32).view(np.int32) == s(g, b.rating).view(np.int32)
        if name.startswith("b"):
            assert s(0, p32).view(np.int32) == s(1, p32).view(np.int32) and s(0, b.rating).view(np.int32) == s(1, b.rating).view(np.int32)
            assert (sel & (b.sst == 0)).sum() == (sel & (b.sst == 1)).sum() and s(0, p32) != s(0, b.rating)
    # ... and in float64 what they are for
    for obj in PER_ITEM:
        r = focf_loss(obj, 1.0, b.U, b.I, *b.cols(True))
        for j, it in enumerate(r.items):
            name = kind[int(it)]
            if name.startswith("a_"):
                g = int(name[-1])
                assert r.P[j, g] == r.T[j, g]
                active = obj in ("value", "absolute") or obj == name.split("_")[1]
                if active:
                    assert r.d[j, 1 - g] != 0 and 0 < abs(r.delta[j]) < 1 - MARGIN and abs(r.delta[j]) > MARGIN
            if name.startswith("b"):
                assert r.delta[j] == 0.0 and (obj not in ("value", "absolute") or r.d[j, 0] != 0)
    return b


COUNTS = ((1, 1), (2, 1), (2, 2), (3, 3), (5, 1), (5, 5), (1025, 1), (1025, 63), (1025, 64), (1025, 65), (1025, 129))


@_retry
def counts(D, B, K, seed=0, attempt=0):
    """B interactions over K distinct items, segments as even as they come; from B = 2 on both groups are present.  With
    B = 1025 the loss reduction has nb = 257 partial sums, beyond one stride of 256; K in {63, 64, 65, 129} sits around the 64
    item segments of a fairness workgroup.  700 users: with B = 1025 some recur."""
    assert (B, K) in COUNTS
    rng = np.random.default_rng([seed, D, B, K, attempt])
    n_users, n_items = 700, 140
    sizes = np.full(K, B // K)
    sizes[:B % K] += 1
    item = np.repeat(rng.permutation(n_items)[:K], sizes)
    user = np.concatenate([rng.permutation(n_users), rng.permutation(n_users)])[:B]
    sst = (user % 2).astype(np.float32)
    if B >= 2 and len(np.unique(sst)) < 2:
        user[0] = user[0] ^ 1
        sst = (user % 2).astype(np.float32)
    o = np.argsort(item, kind="stable")
    U_, I_ = _tables(rng, n_users, n_items, D)
    user, item, sst = user[o], item[o], sst[o]
    b = Batch(f"counts_{B}_{K}", U_, I_, user, item, _ratings(rng, U_, I_, user, item, sst), sst, seed)
    assert b.B == B and len(np.unique(b.item)) == K and (B < 2 or len(np.unique(b.sst)) == 2)
    return _check_conditioned(b)


# ---- the cases both test files run ---------------------------------------------------------------------------------------------

FRAGMENT_WIDTHS = (64, 100, 256)       # one width per row-fragment count: 1 full, 2 with a partial one, 4 full
BUILDER_WIDTHS = {"segments": WIDTHS, "regimes": WIDTHS, "one_sided": FRAGMENT_WIDTHS, "encodings": FRAGMENT_WIDTHS,
                  "counts": FRAGMENT_WIDTHS, "exact_kinks": FRAGMENT_WIDTHS}
_cache = {}


def batches(name, D):
    """the batches of builder `name` at width D (built once)"""
    if (name, D) not in _cache:
        _cache[name, D] = {"segments": lambda: [segments(D)], "regimes": lambda: [regimes(D)], "one_sided": lambda: [one_sided(D)],
                           "encodings": lambda: [encodings(D, w) for w in ENCODINGS],
                           "counts": lambda: [counts(D, B, K) for B, K in COUNTS],
                           "exact_kinks": lambda: [exact_kinks(D)]}[name]()
        for b in _cache[name, D]:
            b.builder = name
    return _cache[name, D]


def reference(b, objective, contiguous):
    """focf_loss of batch b in the given order (computed once)"""
    key = (id(b), objective, bool(contiguous))
    if key not in _cache:
        _cache[key] = focf_loss(objective, FAIR_WEIGHT, b.U, b.I, *b.cols(contiguous))
    return _cache[key]


def two_groups(b):
    return len(np.unique(b.sst)) == 2

"""Float64 references of the loss kernels (csrc/pfcn.hip, csrc/nfcf.hip: fr_nfcf_loss) and the inputs their tests run on:
plain numpy / torch on the CPU, no GPU, no fairrec.  tests/test_loss_ref.py pins every reference to torch.autograd of the
literal expression and checks what the builders promise; tests/test_loss_kernels_hip.py compares the kernels with them.

Every reference takes the kernel's float32 inputs and computes in float64.

* `rowdot*`: torch.mul(a, b).sum(-1) and its gradients, in the plain form and with the rows of `a` reused by R row blocks
  of `b` (b [R * A, D], out[r * A + i] = a[i] . b[r * A + i]); with sum |a b| (and sum_r |g b|) for the bounds.
* `bpr`, `bpr_outer_rect`: BPRLoss -log(1e-10 + sigmoid(x)) on x = pos - neg, and on the [Nc, Na] broadcast x_ij = a_j + c_i
  scaled by `inv`.  sigmoid(-x) stands for 1 - sigmoid(x), so the derivative is exact down to x = -200 and up to +200.
* `softmax_ce`: nn.CrossEntropyLoss (mean) and its gradient.
* `nfcf_loss`: sigmoid + BCELoss by the rules of scorer_ref.loss_head (torch's clamp of both logs at -100 and its backward's
  max(o (1 - o), 1e-12)), plus fair_weight times the differential fairness of oracle.nfcf.differential_fairness restated
  per item, its gradient by float64 autograd through the sigmoid.
* `f32_*`: the kernels' formulas restated in torch float32 on the CPU, operation by operation (exp and log from libm).
  Their error against float64 is what the constants of the tolerances that cannot be derived are measured from.
* `bpr_regimes`, `df_batch`, `softmax_logits`: the inputs, each builder asserting what it is built for.

Tolerances that are not derived (the hardware exp, log and rcp have no bound the project states) take the form the project
uses elsewhere, with a constant MEASURED[...] * 8: the worst error of the float32 restatement against float64 on the builders'
inputs, in units of the form, times 4 for transcendentals of a couple of ulp where libm gives half an ulp, times 2 so that
another seed does not flip a test.  MEASURED is asserted by tests/test_loss_ref.py (the restatement may not exceed it, and
reaches at least half of it), so the constants are a measurement of the REFERENCE side, never of the kernels.
"""
from types import SimpleNamespace

import numpy as np
import torch

import scorer_ref

U = 2.0 ** -24
FLT_MAX = float(np.finfo(np.float32).max)
OUTER_ROWS = 16           # rows of c per workgroup of bpr_outer_kernel
PATH_LIMIT = 40.0         # |a_j|, |c_i| below it: the product-of-exponentials path
GRAD_REL, GRAD_ABS = 1e-4, 1e-6     # the project's BPR gradient form: GRAD_REL |ref| + GRAD_ABS max |ref|
LOSS_REL = 1e-5                      # ... and its relative bound on the BPR loss (benign inputs)
SAFETY = 8.0

# worst error of the float32 restatement against float64 on the builders' inputs (test_loss_ref.py prints and asserts them):
#   bprp_*: the plain BPR (fr_bpr) on bpr_columns with its extremes, units as bpr_*
#   bpr_*: BPR on bpr_regimes, loss in units of LOSS_REL |ref|, gradients in units of GRAD_REL |ref| + GRAD_ABS max |ref|
#   ce_*:  softmax cross-entropy, loss in units of u |ref| (+ u: a loss of exactly 0), dlogits in units of u (|ref| + max |ref|)
#   df_*:  the DF term, loss[2] in units of u |ref| + the carried segment-sum bound, dy's DF part in units of
#          u (|ref| + max |ref|) beyond the carried segment-sum bound (the kernel test adds the BCE head's own tolerance
#          and u |dy| for the one float32 addition of the two parts)
MEASURED = {"bprp_loss": 0.004, "bprp_d": 0.02, "bpr_loss": 0.014, "bpr_da": 0.0021, "bpr_dc": 0.002, "ce_loss": 2.0, "ce_dlogits": 48.0, "df_loss": 0.18, "df_dy": 2.6}


def tol_const(key):
    return SAFETY * MEASURED[key]


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def _t(x, dtype=torch.float32):
    return x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).to(dtype)


# ---- row dots ----------------------------------------------------------------------------------------------------------------

def rowdot(a, b):
    """out[r] = a[r] . b[r]; -> (out, sum_d |a b|)"""
    p = _t(a).double() * _t(b).double()
    return p.sum(-1), p.abs().sum(-1)


def rowdot_bwd(g, a, b):
    """-> (da = g[:, None] b, db = g[:, None] a)"""
    g = _t(g).double()[:, None]
    return g * _t(b).double(), g * _t(a).double()


def rowdot_rep(a, b, R):
    """a [A, D], b [R * A, D] -> (out [R * A], sum_d |a b| [R * A])"""
    a, b = _t(a).double(), _t(b).double()
    p = a.repeat(R, 1) * b
    return p.sum(-1), p.abs().sum(-1)


def rowdot_rep_bwd_sep(g, a, b, R):
    """-> (da_sep [R * A, D] = g b unsummed, db [R * A, D] = g a)"""
    g = _t(g).double()[:, None]
    return g * _t(b).double(), g * _t(a).double().repeat(R, 1)


def rowdot_rep_bwd(g, a, b, R):
    """-> (da [A, D] = sum_r g b, db [R * A, D], sum_r |g b| [A, D])"""
    sep, db = rowdot_rep_bwd_sep(g, a, b, R)
    A = _t(a).shape[0]
    sep = sep.view(R, A, -1)
    return sep.sum(0), db, sep.abs().sum(0)


# ---- BPR ---------------------------------------------------------------------------------------------------------------------

def bpr_term(x):
    """-log(1e-10 + sigmoid(x)) and its derivative -sigmoid(x) sigmoid(-x) / (1e-10 + sigmoid(x)), x float64"""
    s = torch.sigmoid(x)
    return -torch.log(1e-10 + s), -s * torch.sigmoid(-x) / (1e-10 + s)


def bpr(pos, neg):
    """-> (loss, dpos, dneg) of mean_b term(pos_b - neg_b)"""
    x = _t(pos).double() - _t(neg).double()
    t, d = bpr_term(x)
    return t.mean(), d / x.numel(), -d / x.numel()


BPR_EXTREMES = (20.0, -20.0, 50.0, -50.0, 100.0, -100.0, 150.0, -150.0)


def bpr_columns(B, seed=0):
    """pos, neg [B] for the plain BPR: randn scores, and from B = 32 on the differences BPR_EXTREMES at spread positions (both
    columns nonzero there, the difference exact); at least three quarters of the rows stay benign"""
    rng = np.random.default_rng([seed, B, 3])
    pos, neg = rng.standard_normal(B).astype(np.float32), rng.standard_normal(B).astype(np.float32)
    if B >= 32:
        at = np.unique(np.linspace(0, B - 1, len(BPR_EXTREMES)).astype(int))
        assert len(at) == len(BPR_EXTREMES)
        neg[at] = np.float32(0.5)
        pos[at] = np.float32(0.5) + np.asarray(BPR_EXTREMES, dtype=np.float32)
        assert (pos[at].astype(np.float64) - neg[at] == np.asarray(BPR_EXTREMES)).all()
    return pos, neg


def f32_bpr(pos, neg):
    """bpr_kernel's arithmetic in float32: s = 1 / (1 + exp(-x)), term = -log(1e-10 + s), dterm = -s (1 - s) / (1e-10 + s)"""
    pos, neg = _t(pos), _t(neg)
    B = pos.numel()
    s = 1.0 / (1.0 + torch.exp(-(pos - neg)))
    d = -s * (1.0 - s) / (1e-10 + s)
    return (-torch.log(1e-10 + s)).sum() / B, d / B, -d / B


def bpr_outer_rect(a, c, inv):
    """-> (loss, da [Na], dc [Nc]) of inv * sum_{i < Nc, j < Na} term(a_j + c_i)"""
    x = _t(a).double()[None, :] + _t(c).double()[:, None]
    t, d = bpr_term(x)
    return inv * t.sum(), inv * d.sum(0), inv * d.sum(1)


def outer_paths(a, c):
    """[Nc, Na] bool: True where bpr_outer_kernel evaluates the pair on the product-of-exponentials path (its whole row block
    and its column below PATH_LIMIT), False where it takes the exponential of the sum"""
    a, c = _t(a), _t(c)
    nb = (c.numel() + OUTER_ROWS - 1) // OUTER_ROWS
    small = torch.nn.functional.pad(c.abs() < PATH_LIMIT, (0, nb * OUTER_ROWS - c.numel()), value=True)
    rows_ok = small.view(nb, OUTER_ROWS).all(1).repeat_interleave(OUTER_ROWS)[:c.numel()]
    return rows_ok[:, None] & (a.abs() < PATH_LIMIT)[None, :]


def f32_bpr_outer_rect(a, c, inv, clamp=True):
    """bpr_outer_kernel's arithmetic in float32: e = exp(-a_j) exp(-c_i) on the fast path, exp(-(a_j + c_i)) held at the
    largest finite float on the other (clamp = False: the kernel before it was held there), r = 1 / (1 + e),
    term = -log(1e-10 + r), dterm = -(r r e) / (1e-10 + r); sums in float32"""
    a, c = _t(a), _t(c)
    e_fast = torch.exp(-a)[None, :] * torch.exp(-c)[:, None]
    e_slow = torch.exp(-(a[None, :] + c[:, None]))
    if clamp:
        e_slow = e_slow.clamp(max=FLT_MAX)
    e = torch.where(outer_paths(a, c), e_fast, e_slow)
    r = 1.0 / (1.0 + e)
    den = 1e-10 + r
    d = -(r * r * e) / den
    t = -torch.log(den)
    inv = torch.tensor(inv, dtype=torch.float32)
    return t.sum() * inv, d.sum(0) * inv, d.sum(1) * inv


def bpr_regimes(Na, Nc=None, seed=0):
    """Columns a [Na] and rows c [Nc] (Nc = Na by default) that reach every branch of bpr_outer_kernel.  The first row block is
    benign (|c| < 40: the fast path for every column below 40), the last one holds c = -100 (the exponential of the sum for
    every column).  The sums x = a_j + c_i fall below -88.7, where exp(-x) overflows in float32, around -95 and around -150, by
    a column and by a row; into (-88, -44), where r r underflows, on both paths; above +40; and within 1 of -23.03, where
    sigmoid(x) = 1e-10.  At least half of a and half of c are benign (|.| < 8), so at least half of every row and of every
    column of the matrix is, and the largest gradient is a benign one."""
    Nc = Na if Nc is None else Nc
    assert Na >= 14 and Nc >= OUTER_ROWS + 1, "too small to hold every regime next to a benign half"
    rng = np.random.default_rng([seed, Na, Nc])
    a = rng.uniform(-6.0, 6.0, Na).astype(np.float32)
    c = rng.uniform(-4.0, 4.0, Nc).astype(np.float32)
    special = np.array([-95.0, 60.0, -23.03, -35.0, -150.0, 35.0, -53.0], dtype=np.float32)     # -53 + 30: -23 on the slow path
    at = np.unique(np.linspace(0, Na - 1, len(special)).astype(int))
    assert len(at) == len(special)
    a[at] = special
    c[0], c[1], c[2] = -30.0, 30.0, 0.25
    c[Nc - 1] = -100.0
    if Nc >= OUTER_ROWS + 3:
        c[Nc - 2] = 45.0
    x = a.astype(np.float64)[None, :] + c.astype(np.float64)[:, None]
    fast = outer_paths(a, c).numpy()
    assert fast[:OUTER_ROWS].any() and not fast[OUTER_ROWS * ((Nc - 1) // OUTER_ROWS):].any()
    assert (np.abs(a) < 8).sum() * 2 >= Na and (np.abs(c) < 8).sum() * 2 >= Nc
    slow = ~fast
    for lo, hi, where in ((-88.0, -44.0, fast), (-88.0, -44.0, slow), (-110.0, -88.7, slow), (-200.0, -140.0, slow),
                          (40.0, 200.0, fast), (40.0, 200.0, slow), (-24.03, -22.03, fast), (-24.03, -22.03, slow)):
        assert ((x > lo) & (x < hi) & where).any(), (lo, hi)
    col_slow = slow & (np.abs(c) < PATH_LIMIT)[:, None]          # the slow path taken because of the column ...
    row_slow = slow & (np.abs(a) < PATH_LIMIT)[None, :]          # ... and because of a row of the block
    assert ((x < -88.7) & col_slow).any() and ((x < -88.7) & row_slow).any()
    return a, c


def bpr_benign(Na, Nc=None, seed=0):
    rng = np.random.default_rng([seed, Na, Na if Nc is None else Nc, 7])
    return (rng.standard_normal(Na).astype(np.float32), rng.standard_normal(Na if Nc is None else Nc).astype(np.float32))


# ---- softmax cross-entropy ---------------------------------------------------------------------------------------------------

def softmax_ce(logits, label):
    """-> (loss, dlogits [M, C]); a logit of -inf has probability 0"""
    z = _t(logits).double()
    y = _t(label, torch.int64)
    M = z.shape[0]
    d = z - z.max(1, keepdim=True).values
    ls = d - torch.log(torch.exp(d).sum(1, keepdim=True))
    onehot = torch.zeros_like(z)
    onehot[torch.arange(M), y] = 1.0
    return -ls[torch.arange(M), y].mean(), (torch.exp(ls) - onehot) / M


def f32_softmax_ce(logits, label, fixed=True):
    """softmax_ce_kernel's arithmetic in float32: se summed in class order; fixed = False: the kernel that added the maximum
    back first (lse = mx + log(se), loss = lse - z[y], p = exp(z - lse))"""
    z = _t(logits)
    y = _t(label, torch.int64)
    M, C = z.shape
    rows = torch.arange(M)
    mx = z.max(1).values
    se = torch.zeros(M, dtype=torch.float32)
    for c in range(C):
        se = se + torch.exp(z[:, c] - mx)
    if fixed:
        l = torch.log(se) - (z[rows, y] - mx)
        p = torch.exp(z - mx[:, None]) / se[:, None]
    else:
        lse = mx + torch.log(se)
        l = lse - z[rows, y]
        p = torch.exp(z - lse[:, None])
    onehot = torch.zeros_like(z)
    onehot[rows, y] = 1.0
    return l.sum() / M, (p - onehot) / M


def softmax_logits(M, C, shift, seed=0):
    """randn * 3 + shift as float32, labels over every class; with C >= 2, row M // 2 has one -inf logit that is not its label"""
    g = torch.Generator().manual_seed(1000 * M + 10 * C + seed)
    z = (torch.randn(M, C, generator=g, dtype=torch.float64) * 3 + shift).float()
    y = torch.randint(0, C, (M,), generator=g)
    y[:min(M, C)] = torch.arange(min(M, C))
    if C >= 2:
        m = M // 2
        z[m, (int(y[m]) + 1) % C] = float("-inf")
    return z, y


# ---- NFCF: sigmoid + BCE + differential fairness -----------------------------------------------------------------------------

def _df(o, label, sst, item, n_rows_of):
    """differential fairness of the scores o on the label == 1 rows (oracle.nfcf.differential_fairness: M[k, g] =
    (sum + 1 / K) / (count + 1) per item k and group g, eps_k = |log M[k, 0] - log M[k, 1]|, mean over the K items with a
    positive row) -> (df, K, per-item records); 0 when fewer than two groups have a positive row"""
    pos = label == 1
    groups = torch.unique(sst[pos])
    items = torch.unique(item[pos])
    K = len(items)
    assert len(groups) <= 2, "the reference forms one ratio: two groups"
    if K == 0 or len(groups) < 2:
        return o.sum() * 0.0, K, []
    total, recs = o.sum() * 0.0, []
    for k in items.tolist():
        sel = [pos & (item == k) & (sst == g) for g in groups]
        S = [o[s].sum() for s in sel]
        n = [int(s.sum()) for s in sel]
        M = [(S[g] + 1.0 / K) / (n[g] + 1.0) for g in range(2)]
        d = torch.log(M[0]) - torch.log(M[1])
        total = total + d.abs()
        recs.append(SimpleNamespace(item=k, sel=sel, S=[float(s.detach()) for s in S], n=n, d=float(d.detach()), rows=int(n_rows_of[k])))
    return total / K, K, recs


def nfcf_loss(y, label, sst=None, item=None, fair_weight=0.0):
    """fr_nfcf_loss in float64 -> out [B], loss[3] = (total, BCE, DF), dy [B], and for the bounds: dy_bce, dy_df, K, the
    per-item records, seg_loss (the bound the float32 segment sums carry into loss[2]: gamma_(n+5) sum |out| through 1 / M and
    the logarithm, n the rows of the item's segment) and seg_dy [B] (the same through dy's 1 / M factor).  sst = None: BCE only."""
    y, label = _t(y).double(), _t(label).double()
    B = y.numel()
    out, l, dy_bce = scorer_ref.loss_head(y, label)
    r = SimpleNamespace(out=out, dy_bce=dy_bce, dy_df=torch.zeros(B, dtype=torch.float64), K=0, items=[],
                        seg_loss=0.0, seg_dy=torch.zeros(B, dtype=torch.float64))
    bce = l.mean()
    df = torch.zeros((), dtype=torch.float64)
    if sst is not None:
        sst, item = _t(sst).double(), _t(item, torch.int64)
        yy = y.clone().requires_grad_()
        n_rows_of = dict(zip(*[v.tolist() for v in torch.unique(item, return_counts=True)]))
        dfv, r.K, r.items = _df(torch.sigmoid(yy), label, sst, item, n_rows_of)
        if r.items:
            (fair_weight * dfv).backward()
            r.dy_df = yy.grad.detach()
            df = dfv.detach()
            alpha = 1.0 / r.K
            for it in r.items:
                rel = [float(gamma(it.rows + 5)) * it.S[g] / (it.S[g] + alpha) for g in range(2)]
                r.seg_loss += (rel[0] + rel[1]) / r.K
                for g in range(2):
                    r.seg_dy[it.sel[g]] = (rel[0] + rel[1]) * r.dy_df[it.sel[g]].abs()
    r.loss = torch.stack([bce + fair_weight * df, bce, df])
    r.dy = dy_bce + r.dy_df
    return r


def df_tolerances(r, tol_dy_head):
    """(bound on loss[2], bound on dy [B]) for a float32 result against the record r of nfcf_loss: the measured constants on
    their forms, the carried segment-sum bounds, the BCE head's own per-row tolerance (test_scorer_hip._head_ref) and u |dy| for
    the one float32 addition of the two parts of dy"""
    t_loss = tol_const("df_loss") * (U * float(r.loss[2].abs()) + r.seg_loss)
    t_dy = tol_dy_head + r.seg_dy + tol_const("df_dy") * U * (r.dy_df.abs() + r.dy_df.abs().max()) + U * r.dy.abs()
    return t_loss, t_dy


def f32_nfcf_loss(y, label, sst, item, fair_weight):
    """fr_nfcf_loss's arithmetic in float32 (BCE head as nfcf_bce_kernel writes it, segment sums in batch order, M, d, g0 / g1
    and the o (1 - o) factor as nfcf_df_coef_kernel forms them) -> (out, loss[3], dy, the DF part of dy before it is added)"""
    f = torch.float32
    y, label, sst, item = _t(y), _t(label), _t(sst), _t(item, torch.int64)
    B = y.numel()
    o = 1.0 / (1.0 + torch.exp(-y))
    l = -(label * torch.log(o).clamp(min=-100.0) + (1.0 - label) * torch.log(1.0 - o).clamp(min=-100.0))
    s = o * (1.0 - o)
    dy = (o - label) / s.clamp(min=torch.tensor(1e-12, dtype=f)) / B * s
    bce = l.sum() / B
    pos = label == 1
    groups = torch.unique(sst[pos])
    items = torch.unique(item[pos])
    K = len(items)
    eps_sum = torch.zeros((), dtype=f)
    part = torch.zeros(B, dtype=f)
    if K > 0 and len(groups) == 2:
        Kf, fw = torch.tensor(float(K), dtype=f), torch.tensor(fair_weight, dtype=f)
        alpha = 1.0 / Kf
        for k in items.tolist():
            sel = [pos & (item == k) & (sst == g) for g in groups]
            S = [o[q].sum() for q in sel]
            n = [torch.tensor(float(q.sum()), dtype=f) for q in sel]
            M0, M1 = (S[0] + alpha) / (n[0] + 1.0), (S[1] + alpha) / (n[1] + 1.0)
            d = torch.log(M0) - torch.log(M1)
            eps_sum = eps_sum + d.abs()
            sgn = torch.sign(d)
            g0 = fw * sgn / Kf / M0 / (n[0] + 1.0)
            g1 = -fw * sgn / Kf / M1 / (n[1] + 1.0)
            part[sel[0]] = g0 * o[sel[0]] * (1.0 - o[sel[0]])
            part[sel[1]] = g1 * o[sel[1]] * (1.0 - o[sel[1]])
        df = eps_sum / Kf
    else:
        df = torch.zeros((), dtype=f)
    return o, torch.stack([bce + torch.tensor(fair_weight, dtype=f) * df, bce, df]), dy + part, part


DF_HOT = 100               # rows of the hot item: more than 16 x 6, the 16-lane walk of a segment loops
DF_MIN_LOG_RATIO = 1e-3
DF_FULL_B = 256            # from this batch size on every structure below fits


def head_scores(n, rng):
    """scorer outputs after the ReLU: most in (0, 6), some exactly 0, some in (8, 12) where 1 - sigmoid cancels, some >= 20
    where the float32 sigmoid is 1"""
    y = rng.uniform(0.05, 6.0, n)
    kind = rng.random(n)
    y = np.where(kind < 0.15, 0.0, y)
    y = np.where((kind >= 0.15) & (kind < 0.25), rng.uniform(8.0, 12.0, n), y)
    y = np.where((kind >= 0.25) & (kind < 0.30), rng.uniform(20.0, 25.0, n), y)
    return y.astype(np.float32)


def df_batch(B, n_items, seed=0):
    """-> SimpleNamespace(y, label, sst, item, has, zero_item): a batch for the DF term, rows in shuffled order.  As far as B
    rows hold them, in this order: one item with exactly one positive row per group and equal y (d == 0 exactly); items with
    one row (a positive of each group, a negative: an item with no positive row); an item whose positives are all of one
    group; items of 2 .. 16 rows (with the one-row items every segment length modulo 16); one hot item of DF_HOT rows; the
    rest random items.  `has` names the structures that fit (all of them from B = DF_FULL_B on).  y >= 0 with exact zeros.
    Asserted: the float64 |log M0 - log M1| of every item that counts is exactly 0 (the constructed item only) or at least
    DF_MIN_LOG_RATIO, so no gradient's sign turns on float32 rounding; a draw that misses it is drawn again."""
    assert n_items >= B + 8
    for attempt in range(64):
        rng = np.random.default_rng([seed, B, attempt])
        ids = rng.permutation(n_items)
        ids = np.concatenate([[0, n_items - 1], ids[(ids != 0) & (ids != n_items - 1)]])     # the table's first and last row are used
        nxt = iter(ids.tolist())
        item, label, sst, has, fixed_y = [], [], [], set(), {}
        zero_item = None

        def put(n, lab=None, grp=None):
            k = next(nxt)
            for q in range(n):
                item.append(k)
                label.append(float(rng.random() < 0.6) if lab is None else float(lab[q]))
                sst.append(float(rng.integers(1, 3)) if grp is None else float(grp[q]))
            return k

        left = lambda: B - len(item)
        if left() >= 2:
            zero_item = put(2, [1, 1], [1, 2])
            fixed_y[len(item) - 2] = fixed_y[len(item) - 1] = 1.25
            has.add("zero")
        if left() >= 3:
            put(1, [1], [1]); put(1, [1], [2]); put(1, [0], [1])
            has.update(("single", "no_positive"))
        if left() >= 3:
            put(3, [1, 1, 0], [2, 2, 1])
            has.add("one_group")
        sizes_done = 0
        for n in range(2, 17):
            if left() >= n:
                put(n)
                sizes_done += 1
        if sizes_done == 15:
            has.add("every_length_mod_16")
        if left() >= DF_HOT:
            put(DF_HOT)
            has.add("hot")
        while left() > 0:
            put(min(left(), int(rng.integers(1, 6))))
        y = head_scores(B, rng)
        for q, v in fixed_y.items():
            y[q] = v
        perm = rng.permutation(B)
        b = SimpleNamespace(y=y[perm], label=np.asarray(label, np.float32)[perm], sst=np.asarray(sst, np.float32)[perm],
                            item=np.asarray(item, np.int64)[perm], has=has, zero_item=zero_item)
        r = nfcf_loss(b.y, b.label, b.sst, b.item, 1.0)
        if all((it.d == 0.0 and it.item == zero_item) or abs(it.d) >= DF_MIN_LOG_RATIO for it in r.items):
            assert (b.y >= 0).all() and (B < 32 or (b.y == 0).any())
            return b
    raise AssertionError("no draw kept every item's log ratio away from 0")

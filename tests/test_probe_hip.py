"""GPU: the leakage probe's kernels (csrc/probe.hip) through the C ABI against the float64 references of tests/probe_ref.py, at
the smallest shapes that reach each edge (probe_ref.cases(): the row tails of a tile, more than one workgroup with more than
one tile each under the grid rule, widths around 32 / 64 / 128 / 256, the head lists, a class absent from the batch, a saturated
logit, relu's edge).  Every output buffer sits between canaries and starts as NaN, the workspace starts as 0xFF bytes, every
return code is asserted (the harness of tests/test_loss_kernels_hip.py).

Tolerances: probe_ref.MEASURED times 8, in units of u (|ref| + max |ref|), u = 2^-24 -- the worst error of the float32
restatement of the kernel's formulas against float64 over these very cases (measured and asserted on the reference side by
tests/test_probe_ref.py: loss 1.5, gradient 4.3, updated parameters 0.5 units), times 8 by the project's rule for kernels whose
error is not derived in closed form.  Identities (two calls, rows given or contiguous, fr_adam_dense on grad_out) are bit for
bit; counts are exact integers."""
import ctypes

import numpy as np
import pytest
import torch

import probe_ref as R
from test_loss_kernels_hip import CANARY, PAD, _Outs, _bits, _dev, _errflag, _lib, _st, _within, _ws

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -3
CASES = R.cases()


def _carr(classes):
    return (ctypes.c_int32 * len(classes))(*classes)


def _adam(lr):
    from fairrec.optim import AdamHyper
    return AdamHyper(lr=lr, device="cuda")


class _Run:
    """one fr_probe_step call on a case: X / labels as given (contiguous rows) or scattered into a wider table read through
    `rows`; params / m / v / loss / grad_out framed"""

    def __init__(self, c, D, H, classes, scatter=False, labels=None, rows=None, U=None):
        from fairrec import _C
        B = c["X"].shape[0]
        lab = c["labels"] if labels is None else labels
        self.o = _Outs()
        if scatter:
            rng = np.random.default_rng(B + D)
            self.U, ldx = B + 17, D + 3
            pick = rng.permutation(self.U)[:B]
            X = np.full((self.U, ldx), 7.5, dtype=np.float32)
            X[pick, :D] = c["X"]
            table = np.full((len(classes), self.U), -5, dtype=np.int64)      # rows outside the batch: labels nobody may read
            table[:, pick] = lab
            self.rows = _dev(pick.astype(np.int64)) if rows is None else _dev(rows)
        else:
            self.U, ldx, X, table = (B if U is None else U), D, c["X"], lab
            self.rows = None if rows is None else _dev(rows)
        self.X, self.table = _dev(X), _dev(np.ascontiguousarray(table))
        P = len(c["params"])
        self.P = P
        self.params, self.m, self.v = self.o.new(P), self.o.new(P), self.o.new(P)
        for t, k in ((self.params, "params"), (self.m, "m"), (self.v, "v")):
            t.copy_(torch.from_numpy(c[k]))
        self.loss, self.grad = self.o.new(1 + len(classes)), self.o.new(P)
        self.err = _errflag()
        self.hyper = _adam(c["lr"])
        self.step = c["step"]
        self.args = _C.FrProbeArgs(self.X.data_ptr(), 0 if self.rows is None else self.rows.data_ptr(), self.table.data_ptr(),
                                   self.U, ldx, self.table.shape[1], B, D, H, len(classes))
        for i, C in enumerate(classes):
            self.args.classes[i] = C
        self.need = _lib().fr_probe_step_workspace_bytes(D, H, len(classes), _carr(classes), B)
        self.ws = _ws(self.need)

    def call(self, **over):
        a = dict(params=self.params.data_ptr(), m=self.m.data_ptr(), v=self.v.data_ptr(), adam=ctypes.byref(self.hyper.c()),
                 step=self.step, loss=self.loss.data_ptr(), grad=self.grad.data_ptr(), ws=self.ws.data_ptr(),
                 ws_bytes=self.ws.numel(), err=self.err.data_ptr())
        a.update(over)
        return _lib().fr_probe_step(ctypes.byref(self.args), a["params"], a["m"], a["v"], a["adam"], a["step"], a["loss"],
                                    a["grad"], a["ws"], a["ws_bytes"], a["err"], _st())

    def outputs(self):
        return [t.cpu() for t in (self.loss, self.grad, self.params, self.m, self.v)]


def _tol(ref, key):
    ref = torch.as_tensor(ref, dtype=torch.float64)
    return R.tol_const(key) * R.U * (ref.abs() + ref.abs().max())


def _check(tag, run, ref):
    loss, grad, params, m, v = run.outputs()
    _within(f"{tag} loss", loss, ref["loss"], _tol(ref["loss"], "loss"))
    _within(f"{tag} grad", grad, ref["grad"], _tol(ref["grad"], "grad"))
    _within(f"{tag} params", params, ref["params"], _tol(ref["params"], "param"))


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[f"B{B}-D{D}-H{H}-C{'x'.join(map(str, cl))}-{tag}" for B, D, H, cl, tag in CASES])
def test_step_against_float64(idx):
    B, D, H, classes, tag = CASES[idx]
    c = R.make_case(B, D, H, classes, tag)
    ref = R.step_f64(c["params"], c["m"], c["v"], c["X"], c["labels"], D, H, classes, c["lr"], c["step"])
    assert _lib().fr_probe_supported(D, H, len(classes), _carr(classes)) == 0
    assert _lib().fr_probe_param_count(D, H, len(classes), _carr(classes)) == len(c["params"])
    assert _lib().fr_probe_grid(B) == R.grid(B)[2]
    a = _Run(c, D, H, classes)
    assert a.call() == 0 and a.o.ok() and int(a.err.item()) == 0
    _check("contiguous", a, ref)
    # two calls on equal inputs give equal bits; so do rows given as a permutation slice of a wider table (ldx > D)
    b = _Run(c, D, H, classes)
    assert b.call() == 0 and b.o.ok()
    s = _Run(c, D, H, classes, scatter=True)
    assert s.call() == 0 and s.o.ok() and int(s.err.item()) == 0
    for x, y, z in zip(a.outputs(), b.outputs(), s.outputs()):
        assert _bits(x, y) and _bits(x, z)
    # the update is fr_adam_dense on grad_out, bit for bit
    p, m, v = (_dev(c[k].copy()) for k in ("params", "m", "v"))
    assert _lib().fr_adam_dense(p.data_ptr(), a.grad.data_ptr(), m.data_ptr(), v.data_ptr(), a.P, ctypes.byref(a.hyper.c()),
                                c["step"], _st()) == 0
    torch.cuda.synchronize()
    assert _bits(p, a.params) and _bits(m, a.m) and _bits(v, a.v)
    # grad_out is optional: the same step without it
    n = _Run(c, D, H, classes)
    assert n.call(grad=0) == 0 and n.o.ok()
    assert _bits(n.params, a.params) and _bits(n.loss, a.loss) and bool(torch.isnan(n.grad).all())


def test_forward_only_gives_the_logits():
    for B, D, H, classes in ((65, 6, 5, (2, 7, 21)), (33, 65, 0, (3,)), (R.BIG_B, 3, 2, (2, 3))):
        c = R.make_case(B, D, H, classes, "plain")
        r = _Run(c, D, H, classes, scatter=True)
        o = _Outs()
        z = o.new(B, sum(classes))
        rc = _lib().fr_probe_forward(ctypes.byref(r.args), r.params.data_ptr(), z.data_ptr(), r.err.data_ptr(), _st())
        assert rc == 0 and o.ok() and r.o.ok() and int(r.err.item()) == 0
        ref = torch.from_numpy(R.forward_f64(c["params"], c["X"], D, H, classes))
        # a logit is one or two ascending fma chains and a bias: gamma_(n_in + 2) on sum |terms|, bounded by its own inputs
        absr = torch.from_numpy(R.forward_f64(np.abs(c["params"]), np.abs(c["X"]), D, H, classes))
        _within(f"logits B={B} D={D} H={H}", z.cpu(), ref, float(R.U * (D + H + 4) / (1 - R.U * (D + H + 4))) * absr)
        assert _bits(r.params, torch.from_numpy(c["params"]))


def test_bad_label_and_bad_row_set_the_flag_and_drop_the_row():
    B, D, H, classes = 65, 6, 5, (3, 2)
    c = R.make_case(B, D, H, classes, "plain")
    # a label outside 0..C-1 of head 0: the row contributes nothing to head 0, everything to head 1
    lab = c["labels"].copy()
    lab[0, 7], lab[0, 64] = 3, -1
    drop0 = np.zeros(B, dtype=bool)
    drop0[[7, 64]] = True
    ref = R.step_f64(c["params"], c["m"], c["v"], c["X"], c["labels"], D, H, classes, c["lr"], c["step"], drop_head=[drop0, None])
    r = _Run(c, D, H, classes, labels=lab)
    assert r.call() == 0 and r.o.ok() and int(r.err.item()) & 1
    _check("bad label", r, ref)
    # a row index outside 0..U-1: the row contributes nothing to any head; the divisor stays B
    rows = np.arange(B, dtype=np.int64)
    rows[3], rows[40] = B, -1
    drop = np.zeros(B, dtype=bool)
    drop[[3, 40]] = True
    ref = R.step_f64(c["params"], c["m"], c["v"], c["X"], c["labels"], D, H, classes, c["lr"], c["step"], drop=drop)
    r = _Run(c, D, H, classes, rows=rows)
    assert r.call() == 0 and r.o.ok() and int(r.err.item()) & 1
    _check("bad row", r, ref)
    # ... and the step equals the step on the batch without those rows, scaled by the divisor (checked on the reference side too)
    keep = ~drop
    c2 = dict(c, X=c["X"][keep], labels=c["labels"][:, keep])
    r2 = _Run(c2, D, H, classes)
    assert r2.call() == 0 and int(r2.err.item()) == 0
    g, g2 = r.grad.cpu().double() * B, r2.grad.cpu().double() * (B - 2)
    _within("bad row against the shorter batch", g, g2, 2 * _tol(g2, "grad"))


def test_refusals_write_nothing():
    B, D, H, classes = 33, 5, 7, (3, 2)
    c = R.make_case(B, D, H, classes, "plain")

    def fresh():
        return _Run(c, D, H, classes)

    def untouched(r):
        torch.cuda.synchronize()
        return (r.o.ok() and _bits(r.params, torch.from_numpy(c["params"])) and _bits(r.m, torch.from_numpy(c["m"]))
                and _bits(r.v, torch.from_numpy(c["v"])) and bool(torch.isnan(r.loss).all()) and bool(torch.isnan(r.grad).all())
                and bool((r.ws == 0xFF).all()) and int(r.err.item()) == 0)

    def shape(**kw):
        def f(r):
            for k, val in kw.items():
                if k == "C0":
                    r.args.classes[0] = val
                else:
                    setattr(r.args, k, val)
            return r.call()
        return f

    wd = _adam(1e-3)
    wd.c().weight_decay = 0.1
    refusals = [
        ("D", EUNSUPPORTED, shape(D=0)), ("D", EUNSUPPORTED, shape(D=257)), ("H", EUNSUPPORTED, shape(H=-1)),
        ("H", EUNSUPPORTED, shape(H=257)), ("classes[0]", EUNSUPPORTED, shape(C0=1)), ("classes[0]", EUNSUPPORTED, shape(C0=65)),
        ("n_heads", EUNSUPPORTED, shape(n_heads=0)), ("n_heads", EUNSUPPORTED, shape(n_heads=9)),
        ("B", EUNSUPPORTED, shape(B=0)), ("B", EUNSUPPORTED, shape(B=65537)),
        ("X", EINVAL, shape(X=0)), ("ldx", EINVAL, shape(ldx=D - 1)), ("ldl", EINVAL, shape(ldl=B - 1)),
        ("U", EINVAL, shape(U=0)), ("rows", EINVAL, shape(U=B - 1)), ("labels", EINVAL, shape(labels=0)),
        ("step", EINVAL, lambda r: r.call(step=0)), ("ws", EINVAL, lambda r: r.call(ws_bytes=r.need - 1)),
        ("ws", EINVAL, lambda r: r.call(ws=0)), ("params", EINVAL, lambda r: r.call(params=0)),
        ("params", EINVAL, lambda r: r.call(m=0)), ("params", EINVAL, lambda r: r.call(v=0)),
        ("loss", EINVAL, lambda r: r.call(loss=0)), ("err_flag", EINVAL, lambda r: r.call(err=0)),
        ("adam", EINVAL, lambda r: r.call(adam=None)), ("weight_decay", EINVAL, lambda r: r.call(adam=ctypes.byref(wd.c()))),
    ]
    for word, code, f in refusals:
        r = fresh()
        rc = f(r)
        msg = _lib().fr_last_error().decode()
        assert rc == code and word in msg and "fr_probe_step" in msg, (word, rc, msg)
        assert untouched(r), word
    carr = _carr(classes)
    assert _lib().fr_probe_supported(D, H, 2, carr) == 0 and _lib().fr_probe_supported(300, H, 2, carr) == EUNSUPPORTED
    assert _lib().fr_probe_step_workspace_bytes(300, H, 2, carr, B) == 0 and _lib().fr_probe_grid(0) == 0
    # fr_probe_forward and fr_probe_eval refuse in the same way
    r = fresh()
    o = _Outs()
    z = o.new(B, sum(classes))
    r.args.D = 300
    assert _lib().fr_probe_forward(ctypes.byref(r.args), r.params.data_ptr(), z.data_ptr(), r.err.data_ptr(), _st()) == EUNSUPPORTED
    r.args.D = D
    assert _lib().fr_probe_forward(ctypes.byref(r.args), r.params.data_ptr(), 0, r.err.data_ptr(), _st()) == EINVAL
    assert "logits" in _lib().fr_last_error().decode()
    assert o.ok() and bool(torch.isnan(z).all()) and untouched(r)


# ---- fr_probe_eval -----------------------------------------------------------------------------------------------------------

def _eval(z, table, classes, rows=None, U=None):
    n, heads, sumC = z.shape[0], len(classes), sum(classes)
    o = _Outs()
    probs = o.new(n, sumC)
    correct = torch.full((heads,), -7, dtype=torch.int64, device="cuda")
    count = torch.full((sumC,), -7, dtype=torch.int64, device="cuda")
    ll = torch.full((heads,), float("nan"), dtype=torch.float64, device="cuda")
    err = _errflag()
    carr = _carr(classes)
    ws = _ws(_lib().fr_probe_eval_workspace_bytes(n, heads, carr))
    zd, td = _dev(z), _dev(table)
    rd = None if rows is None else _dev(rows)
    rc = _lib().fr_probe_eval(zd.data_ptr(), td.data_ptr(), table.shape[1], 0 if rd is None else rd.data_ptr(),
                              table.shape[1] if U is None else U, n, heads, carr, correct.data_ptr(), ll.data_ptr(),
                              count.data_ptr(), probs.data_ptr(), ws.data_ptr(), ws.numel(), err.data_ptr(), _st())
    assert rc == 0 and o.ok()
    return correct.cpu().numpy(), ll.cpu().numpy(), count.cpu().numpy(), probs.cpu().numpy(), int(err.item())


def test_eval_counts_are_exact_and_the_logloss_is_float64():
    classes = (2, 3)
    rng = np.random.default_rng(5)
    n = 700                                                     # three blocks of 256 rows
    z = np.round(rng.standard_normal((n, 5)), 1).astype(np.float32)      # rounded: ties in the argmax, tied probabilities
    z[:40, 0] = z[:40, 1]                                       # the two classes of head 0 tied: p = 0.5 each, class 0 wins
    z[40:60, 2:] = 0.25                                         # a three-way tie: class 0 wins
    y = np.stack([rng.integers(0, 2, n), rng.integers(0, 3, n)]).astype(np.int64)
    correct, ll, count, probs, err = _eval(z, y, classes)
    assert err == 0
    off = 0
    for a, C in enumerate(classes):
        za = z[:, off:off + C].astype(np.float64)
        assert correct[a] == int((za.argmax(axis=1) == y[a]).sum())              # numpy's argmax: the first maximum
        assert (count[off:off + C] == np.bincount(y[a], minlength=C)).all()
        ref = R.metrics(za, y[a], y[a], C)
        # a float64 sum of n terms, each within an ulp or two of float64: far inside the rule's MEASURED * 8 float32 units
        assert abs(ll[a] - ref["logloss"] * n) <= R.tol_const("loss") * R.U * 2 * abs(ref["logloss"] * n)
        e = np.exp(za - za.max(axis=1, keepdims=True))
        p = e / e.sum(axis=1, keepdims=True)
        assert (np.abs(probs[:, off:off + C] - p) <= 2 * R.U * p).all()
        off += C
    assert (probs[:40, 0] == 0.5).all() and (probs[:40, 1] == 0.5).all()
    # the AUC inputs: fr_auc_sorted on a sorted probability column gives the integers of a direct count on the same column
    s = torch.from_numpy(probs[:, 1].copy()).cuda()
    srt, order = torch.sort(s)
    lab = torch.from_numpy((y[0] == 1).astype(np.float32)).cuda()[order].contiguous()
    out = torch.zeros(3, dtype=torch.int64, device="cuda")
    ws = _ws(_lib().fr_auc_sorted_workspace_bytes(n))
    assert _lib().fr_auc_sorted(srt.data_ptr(), lab.data_ptr(), n, out.data_ptr(), ws.data_ptr(), ws.numel(), _st()) == 0
    two_u, P, N = out.cpu().tolist()
    s1, s0 = probs[:, 1][y[0] == 1], probs[:, 1][y[0] == 0]
    assert (P, N) == (len(s1), len(s0))
    assert two_u == 2 * int((s1[:, None] > s0[None, :]).sum()) + int((s1[:, None] == s0[None, :]).sum())
    assert abs(two_u / (2.0 * P * N) - R.binary_auc(probs[:, 1], y[0] == 1)) <= 1e-12


def test_eval_reads_labels_through_rows_and_skips_bad_ones():
    classes = (3,)
    rng = np.random.default_rng(6)
    n, U = 300, 400
    z = rng.standard_normal((n, 3)).astype(np.float32)
    rows = rng.permutation(U)[:n].astype(np.int64)
    table = np.full((1, U), -9, dtype=np.int64)
    y = rng.integers(0, 3, n)
    table[0, rows] = y
    correct, ll, count, probs, err = _eval(z, table, classes, rows=rows)
    assert err == 0 and correct[0] == int((z.argmax(axis=1) == y).sum()) and (count == np.bincount(y, minlength=3)).all()
    table[0, rows[5]] = 3                                       # a bad label and a bad row: flagged, counted nowhere
    rows2 = rows.copy()
    rows2[9] = U
    keep = np.ones(n, dtype=bool)
    keep[[5, 9]] = False
    correct, ll, count, probs, err = _eval(z, table, classes, rows=rows2)
    assert err & 1 and correct[0] == int((z.argmax(axis=1) == y)[keep].sum()) and (count == np.bincount(y[keep], minlength=3)).all()
    ref = R.metrics(z[keep].astype(np.float64), y[keep], y[keep], 3)
    assert abs(ll[0] - ref["logloss"] * keep.sum()) <= 1e-9 * abs(ll[0])
    assert np.isfinite(probs).all()

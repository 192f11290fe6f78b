"""GPU: csrc/scorer.hip (fr_scorer_fwd / fr_scorer_bwd, then fr_linear_bwd_weight_multi and fr_parts_sum) through the C ABI
against the float64 reference of tests/scorer_ref.py, over the whole shape space fr_scorer_supported accepts.

Each stage is judged on the kernel's own stored inputs to it (h1 from x0d | x1d, h2 from h1, y from h2, dz2 from dz3, ...,
dW from the kernel's dz and dropped activations), ReLU decisions are read off the kernel's stored activations, and every
product is held to one per-element bound, scorer_ref.product_bound with C below: a lost chunk, a wrong tile or stride gives
errors the size of the value itself.  Dropout patterns are drawn independently with fr_dropout_apply at the documented
offsets.  The loss head's saturated rows and its y == 0 rows are compared with torch's fp32 op sequence (that is what parity
with the reference means there; float64 would not saturate), every other row with float64."""
import ctypes
import math
import threading

import pytest
import torch
import torch.nn.functional as F

import scorer_ref as R

pytestmark = pytest.mark.gpu

C = 4                   # the constant of every product bound: c (K + 2) 2^-24 (|A| |B|^T + |bias|)
U = R.U
RATIO = {}              # largest error / bound seen per stage (printed at the end of the module)
SHAPES = [(k0, n1, n2) for k0 in range(32, 257, 32) for n1 in (32, 64, 96, 128) for n2 in (32, 64)]
VARIANTS = [(True, True), (False, True), (True, False), (False, False)]      # (dx0 wanted, dx1 wanted): frozen tables


def _c():
    from fairrec import _C
    return _C


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if RATIO:
        print("\nscorer: largest error / bound per stage: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(RATIO.items())))


def _ratio(stage, r):
    RATIO[stage] = max(RATIO.get(stage, 0.0), math.inf if math.isnan(r) else r)


def _near(stage, got, ref, bound):
    """|got - ref| <= bound element by element; a NaN on either side (an element the kernel never wrote: the outputs start
    as NaN where that can be seen) is out of bound."""
    err = (got.double() - ref).abs()
    _ratio(stage, float((err / bound.clamp_min(1e-300)).nan_to_num(math.inf).max()) if err.numel() else 0.0)
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int(bad.view(-1).nonzero()[0])
        raise AssertionError(f"{stage}: {int(bad.sum())} of {err.numel()} elements out of bound; first at flat index {i}: "
                             f"got {float(got.reshape(-1)[i])!r}, ref {float(ref.reshape(-1)[i])!r}, bound {float(bound.reshape(-1)[i])!r}")


def _data(k0, n1, n2, B, seed):
    """Inputs with asymmetric scale (x1 ~ 0.5 x0 + 0.1, row ramps on the weights) and a control channel that fixes each
    row's loss-head regime: x0[:, 0] passes straight to z3 (W1[0] = e0, W2[0] = e0, W3[0, 0] = 1, b3 = -1.5), so rows
    with control 0 end at a negative z3 (y == 0), rows with control 22..30 at z3 >= 20 (fp32 sigmoid == 1), the rest
    in between."""
    g = torch.Generator().manual_seed(seed)
    K = 2 * k0
    x0 = torch.randn(B, k0, generator=g)
    x1 = torch.randn(B, k0, generator=g) * 0.5 + 0.1
    kind = torch.arange(B) % 3
    x0[:, 0] = torch.where(kind == 0, 0.0, torch.where(kind == 1, 1.5 + 2.5 * torch.rand(B, generator=g),
                                                       22.0 + 8.0 * torch.rand(B, generator=g)))
    W1 = torch.randn(n1, K, generator=g) / K ** 0.5 * (0.5 + torch.arange(n1)[:, None] / n1)
    W1[0] = 0.0
    W1[0, 0] = 1.0
    b1 = torch.randn(n1, generator=g) * 0.1
    b1[0] = 0.0
    W2 = torch.randn(n2, n1, generator=g) / n1 ** 0.5 * (0.5 + torch.arange(n1)[None, :] / n1)
    W2[0] = 0.0
    W2[0, 0] = 1.0
    b2 = torch.randn(n2, generator=g) * 0.1
    b2[0] = 0.0
    W3 = torch.randn(1, n2, generator=g) * 0.3 / n2 ** 0.5
    W3[0, 0] = 1.0
    b3 = torch.tensor([-1.5])
    label = (torch.rand(B, generator=g) < 0.5).float()
    if B >= 64:
        label[32:64] = 0.0                      # one workgroup without a positive row
    sst = torch.randint(0, 5, (B,), generator=g).float()
    return x0, x1, [W1, b1, W2, b2, W3, b3], label, sst


def _drop_pattern(lib, _C, n, p, seed, off, used, x=None):
    """fr_dropout_apply's output at element offset `off` of the call `used` recorded (x = ones: the kept scale / 0)."""
    src = x if x is not None else torch.ones(n, device="cuda")
    out = torch.empty_like(src)
    _C.check(lib.fr_dropout_apply(src.data_ptr(), n, p, seed, off, used.data_ptr(), None, None, out.data_ptr(),
                                  _C.current_stream()), "fr_dropout_apply")
    return out


def _launch(k0, n1, n2, B, p, *, dx=(True, True), gscale=None, label_zero=False, close_loss=False, seed=None):
    """One forward + backward + weight-gradient chain on the device; everything it stored, on the host."""
    from fairrec.model.fair_recommender.nfcf import _NfcfFused
    _C = _c()
    lib, st = _C.lib(), _C.current_stream()
    seed = seed if seed is not None else k0 * 1009 + n1 * 31 + n2 * 7 + B
    x0, x1, params, label, sst = _data(k0, n1, n2, B, seed)
    if label_zero:
        label.zero_()
    dev = dict(device="cuda")
    P = [t.cuda().contiguous() for t in params]
    x0g, x1g, lab, sstg = x0.cuda(), x1.cuda(), label.cuda(), sst.cuda()
    dseed = 0x5EED0000 + seed
    d = _NfcfFused._desc(k0, k0, P, p, dseed, B)
    nblk = lib.fr_scorer_blocks(B)
    f32 = dict(dtype=torch.float32, **dev)
    state = torch.tensor([5 + seed % 7, 0], dtype=torch.int64, **dev)       # {call counter, ticket}
    used = torch.full((1,), -1, dtype=torch.int64, **dev)
    x0d = torch.empty((B, k0), **f32) if p > 0 else None
    x1d = torch.empty((B, k0), **f32) if p > 0 else None
    h1, h2 = torch.empty((B, n1), **f32), torch.empty((B, n2), **f32)
    y, out, dy = torch.empty(B, **f32), torch.empty(B, **f32), torch.empty(B, **f32)
    bce_part, mm_part = torch.empty(nblk, **f32), torch.empty(2 * nblk, **f32)
    loss = torch.full((3,), float("nan"), **f32) if close_loss else None
    ticket = torch.zeros(1, dtype=torch.int32, **dev) if close_loss else None
    _C.check(lib.fr_scorer_fwd(ctypes.byref(d), x0g.data_ptr(), x1g.data_ptr(), B, state.data_ptr() if p > 0 else None,
                               _C.ptr(used) if p > 0 else None, state.data_ptr() if p > 0 else None, _C.ptr(x0d), _C.ptr(x1d),
                               h1.data_ptr(), h2.data_ptr(), y.data_ptr(), lab.data_ptr(), sstg.data_ptr(), out.data_ptr(),
                               dy.data_ptr(), bce_part.data_ptr(), mm_part.data_ptr(), _C.ptr(loss), _C.ptr(ticket), st),
             "fr_scorer_fwd")
    gs = torch.tensor([gscale], **f32) if gscale is not None else None
    dz1, dz2, dz3 = torch.empty((B, n1), **f32), torch.empty((B, n2), **f32), torch.empty((B, 1), **f32)
    dx0 = torch.full((B, k0), float("nan"), **f32) if dx[0] else None
    dx1 = torch.full((B, k0), float("nan"), **f32) if dx[1] else None
    w3part = torch.empty((nblk, n2 + 1), **f32)
    _C.check(lib.fr_scorer_bwd(ctypes.byref(d), dy.data_ptr(), _C.ptr(gs), y.data_ptr(), h1.data_ptr(), h2.data_ptr(), B,
                               _C.ptr(used) if p > 0 else None, dz1.data_ptr(), dz2.data_ptr(), dz3.data_ptr(), _C.ptr(dx0),
                               _C.ptr(dx1), w3part.data_ptr(), st), "fr_scorer_bwd")
    xa, xb = (x0d, x1d) if p > 0 else (x0g, x1g)
    dW1, db1, dW2, db2 = (torch.empty_like(t) for t in P[:4])
    w3 = torch.empty(n2 + 1, **f32)
    jobs = (_C.FrWgradJob * 3)(
        _C.FrWgradJob(dz1.data_ptr(), xa.data_ptr(), k0, xb.data_ptr(), k0, n1, dW1.data_ptr(), db1.data_ptr(), None, 0),
        _C.FrWgradJob(dz2.data_ptr(), h1.data_ptr(), n1, None, 0, n2, dW2.data_ptr(), db2.data_ptr(), None, 0),
        _C.FrWgradJob(None, None, n2 + 1, None, 0, 1, w3.data_ptr(), None, w3part.data_ptr(), nblk))
    ws = torch.empty(lib.fr_linear_bwd_weight_multi_workspace_bytes(jobs, 3, B), dtype=torch.uint8, **dev)
    _C.check(lib.fr_linear_bwd_weight_multi(jobs, 3, B, ws.data_ptr(), ws.numel(), st), "fr_linear_bwd_weight_multi")
    w3s = torch.empty(n2 + 1, **f32)
    _C.check(lib.fr_parts_sum(w3part.data_ptr(), nblk, n2 + 1, w3s.data_ptr(), st), "fr_parts_sum")
    r = dict(k0=k0, n1=n1, n2=n2, B=B, p=p, nblk=nblk, x0=x0, x1=x1, params=params, label=label, sst=sst, gscale=gscale)
    if p > 0:
        r["pat"] = {"x0": _drop_pattern(lib, _C, B * k0, p, dseed, d.off_x0, used, x0g),
                    "x1": _drop_pattern(lib, _C, B * k0, p, dseed, d.off_x1, used, x1g),
                    "k0": _drop_pattern(lib, _C, B * k0, p, dseed, d.off_x0, used),
                    "k1": _drop_pattern(lib, _C, B * k0, p, dseed, d.off_x1, used),
                    "h1": _drop_pattern(lib, _C, B * n1, p, dseed, d.off_h1, used),
                    "h2": _drop_pattern(lib, _C, B * n2, p, dseed, d.off_h2, used)}
        r["used"], r["state"] = used, state
    for k, v in dict(x0d=x0d, x1d=x1d, h1=h1, h2=h2, y=y, out=out, dy=dy, bce_part=bce_part, mm_part=mm_part, loss=loss,
                     ticket=ticket, dz1=dz1, dz2=dz2, dz3=dz3, dx0=dx0, dx1=dx1, w3part=w3part, dW1=dW1, db1=db1, dW2=dW2,
                     db2=db2, w3=w3, w3s=w3s).items():
        r[k] = v.cpu() if v is not None else None
    if p > 0:
        r["pat"] = {k: v.cpu() for k, v in r["pat"].items()}
        r["used"], r["state"] = int(used.cpu()), r["state"].cpu()
    return r


def _head_ref(y, label):
    """Expected out / per-row BCE / dy from the kernel's own y, with per-element tolerances.  Rows with y == 0 or an fp32
    sigmoid of exactly 1: torch's fp32 op sequence (exact there); every other row: float64, within what __expf and the fp32
    sigmoid / log can be off by (o's error 4u (o (1 - o)(|y| + 2) + 1), carried through log and the division)."""
    B = y.numel()
    yy = y.clone().requires_grad_()
    o32 = torch.sigmoid(yy)
    F.binary_cross_entropy(o32, label).backward()
    l32 = F.binary_cross_entropy(o32.detach(), label, reduction="none")
    special = (y == 0) | (o32.detach() == 1.0)
    o64, l64, dy64 = R.loss_head(y.double(), label.double())
    tol_o = 4 * U * (o64 * (1 - o64) * (y.double().abs() + 2) + 1)
    tol_l = tol_o / torch.minimum(o64, 1 - o64).clamp_min(1e-300) + 4 * U * l64
    tol_dy = (tol_o + 4 * U * (o64 - label.double()).abs()) / B
    o_ref = torch.where(special, o32.detach().double(), o64)
    l_ref = torch.where(special, l32.double(), l64)
    dy_ref = torch.where(special, yy.grad.double(), dy64)
    tol_o = torch.where(special, torch.zeros_like(tol_o), tol_o)
    tol_l = torch.where(special, 4 * U * l_ref, tol_l)
    tol_dy = torch.where(special, 4 * U * dy_ref.abs(), tol_dy)
    # 15.5 < y < 17.5: whether fp32 sigmoid rounds to 1 (and the BCE of a negative row to the clamp) turns on one ulp of exp
    band = (y > 15.5) & (y < 17.5)
    tol_o = torch.where(band, torch.full_like(tol_o, 4 * U), tol_o)
    tol_l = torch.where(band, torch.full_like(tol_l, 100.0), tol_l)
    tol_dy = torch.where(band, dy_ref.abs() + 4 * U / B, tol_dy)
    return special, o_ref, l_ref, dy_ref, tol_o, tol_l, tol_dy


def _check(r, regimes=False):
    k0, n1, n2, B, p = r["k0"], r["n1"], r["n2"], r["B"], r["p"]
    W1, b1, W2, b2, W3, b3 = r["params"]
    s = 1.0 / (1.0 - p) if p > 0 else 1.0
    # ---- dropout: the dropped inputs bit-equal to fr_dropout_apply's, the hidden activations zero where it drops -----------
    if p > 0:
        assert r["used"] == int(r["state"][0]) - 1 and int(r["state"][1]) == 0      # the counter protocol: used, advanced
        assert torch.equal(r["x0d"].view(-1), r["pat"]["x0"].view(-1)) and torch.equal(r["x1d"].view(-1), r["pat"]["x1"].view(-1))
        keep0 = torch.cat([r["pat"]["k0"].view(B, k0), r["pat"]["k1"].view(B, k0)], 1) != 0
        keep1, keep2 = r["pat"]["h1"].view(B, n1) != 0, r["pat"]["h2"].view(B, n2) != 0
        assert bool((r["h1"][~keep1] == 0).all()) and bool((r["h2"][~keep2] == 0).all())
        X = torch.cat([r["x0d"], r["x1d"]], 1)
    else:
        keep0 = torch.ones(B, 2 * k0, dtype=torch.bool)
        keep1, keep2 = torch.ones(B, n1, dtype=torch.bool), torch.ones(B, n2, dtype=torch.bool)
        X = torch.cat([r["x0"], r["x1"]], 1)

    def layer(stage, a, W, b, got, keep, K, s=s):
        z = a.double() @ W.double().t() + b.double()
        bnd = R.product_bound(a, W, b, K, C)
        on = got > 0
        assert bool((got[~on] == 0).all()), stage + ": a stored activation is negative or not a number (ReLU not applied)"
        assert bool(keep[on].all()), stage + ": an activation survives where the pattern drops"
        _near(stage, got[on], z[on] * s, bnd[on] * s)                    # active: the product, scaled
        off = ~on & keep
        assert bool((z[off] <= bnd[off]).all()), stage + ": the kernel cut a pre-activation that is positive beyond rounding"
    layer("h1", X, W1, b1, r["h1"], keep1, 2 * k0)
    layer("h2", r["h1"], W2, b2, r["h2"], keep2, n1)
    layer("y", r["h2"], W3, b3, r["y"].view(B, 1), torch.ones(B, 1, dtype=torch.bool), n2, s=1.0)
    # ---- loss head -------------------------------------------------------------------------------------------------------
    y, label = r["y"], r["label"]
    special, o_ref, l_ref, dy_ref, tol_o, tol_l, tol_dy = _head_ref(y, label)
    if regimes:       # the batch reaches all three regimes of the head
        assert int((y == 0).sum()) >= 1 and int((y >= 20).sum()) >= 1 and int(((y > 0) & (y < 8)).sum()) >= 1
    _near("out", r["out"], o_ref, tol_o)
    _near("dy", r["dy"], dy_ref, tol_dy)
    nb = r["nblk"]
    pad = nb * 32 - B
    lp = F.pad(l_ref, (0, pad)).view(nb, 32)
    _near("bce_part", r["bce_part"], lp.sum(1), F.pad(tol_l, (0, pad)).view(nb, 32).sum(1) + 34 * U * lp.abs().sum(1))
    pos = F.pad(label, (0, pad)).view(nb, 32) == 1
    sv = F.pad(r["sst"], (0, pad)).view(nb, 32)
    lo = torch.where(pos, sv, torch.full_like(sv, float("inf"))).min(1).values
    hi = torch.where(pos, sv, torch.full_like(sv, -float("inf"))).max(1).values
    assert torch.equal(r["mm_part"].view(nb, 2)[:, 0], lo) and torch.equal(r["mm_part"].view(nb, 2)[:, 1], hi)
    if r["loss"] is not None:
        ref = l_ref.sum() / B
        bnd = (tol_l.sum() + (nb + 40) * U * l_ref.abs().sum()) / B
        _near("loss", r["loss"][:2], ref.expand(2), bnd.expand(2))
        assert float(r["loss"][2]) == 0.0 and int(r["ticket"][0]) == 0
    # ---- backward ---------------------------------------------------------------------------------------------------------
    gs = r["gscale"] if r["gscale"] is not None else 1.0
    dz3 = r["dz3"].view(-1)
    ref3 = torch.where(y > 0, r["dy"].double() * gs, torch.zeros(B, dtype=torch.float64))
    _near("dz3", dz3, ref3, 3 * C * U * ref3.abs())
    ref2 = torch.where(r["h2"] > 0, dz3.double()[:, None] * W3.double() * s, torch.zeros(B, n2, dtype=torch.float64))
    _near("dz2", r["dz2"], ref2, 3 * C * U * ref2.abs())
    m1 = (r["h1"] > 0).double() * s
    _near("dz1", r["dz1"], (r["dz2"].double() @ W2.double()) * m1, R.product_bound(r["dz2"], W2.t(), None, n2, C) * m1)
    dxr = r["dz1"].double() @ W1.double()
    dxb = R.product_bound(r["dz1"], W1.t(), None, n1, C)
    m0 = keep0.double() * s
    for j, name in enumerate(("dx0", "dx1")):
        if r[name] is not None:
            sl = slice(j * k0, (j + 1) * k0)
            _near(name, r[name], dxr[:, sl] * m0[:, sl], dxb[:, sl] * m0[:, sl])
    ones = torch.ones(B, 1)
    h2e = torch.cat([r["h2"], ones], 1)          # (dW3 | db3): fr_linear_bwd_weight_multi's parts job and fr_parts_sum
    for stage, dz, a, got in (("dW1|db1", r["dz1"], torch.cat([X, ones], 1), torch.cat([r["dW1"], r["db1"][:, None]], 1)),
                              ("dW2|db2", r["dz2"], torch.cat([r["h1"], ones], 1), torch.cat([r["dW2"], r["db2"][:, None]], 1)),
                              ("dW3|db3", r["dz3"], h2e, r["w3"].view(1, -1)), ("dW3|db3 parts_sum", r["dz3"], h2e, r["w3s"].view(1, -1))):
        _near(stage, got, dz.double().t() @ a.double(), R.product_bound(dz.t(), a.t(), None, B, C))


# ---- the shape matrix -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("k0,n1,n2", SHAPES, ids=[f"k{a}_n{b}_{c}" for a, b, c in SHAPES])
def test_every_supported_width_matches_float64(k0, n1, n2, p):
    i = SHAPES.index((k0, n1, n2))
    dx = VARIANTS[(i + (p > 0)) % 4]
    gscale = 0.7 if (i // 4 + (p > 0)) % 2 else None
    r = _launch(k0, n1, n2, 97, p, dx=dx, gscale=gscale)
    _check(r, regimes=True)


BATCHES = [1, 31, 32, 33, 4097, 8192, 8193]


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("k0,n1,n2", [(256, 128, 64), (32, 32, 32)], ids=["k256_n128_64", "k32_n32_32"])
def test_batch_tails_match_float64(k0, n1, n2, B):
    r = _launch(k0, n1, n2, B, 0.2, dx=(False, True) if B % 2 else (True, True), close_loss=True)
    _check(r, regimes=B >= 97)


@pytest.mark.parametrize("p", [0.5, 0.9])
@pytest.mark.parametrize("k0,n1,n2", [(96, 32, 64), (224, 128, 32)], ids=["k96_n32_64", "k224_n128_32"])
def test_heavy_dropout_matches_float64(k0, n1, n2, p):
    _check(_launch(k0, n1, n2, 1000, p, gscale=1.3))


def test_batch_without_a_positive_row():
    """Every workgroup's (min, max) partial is the identity (+inf, -inf); fr_nfcf_loss_tail still closes a finite loss, the
    oracle's (no positive row: no fairness term)."""
    from oracle import nfcf as O
    _C = _c()
    lib = _C.lib()
    r = _launch(64, 128, 64, 300, 0.0, label_zero=True, close_loss=True)
    _check(r)
    assert bool((r["mm_part"][0::2] == float("inf")).all()) and bool((r["mm_part"][1::2] == -float("inf")).all())
    B = r["B"]
    loss = torch.full((3,), float("nan"), device="cuda")
    ws = torch.empty(lib.fr_nfcf_loss_workspace_bytes(B), dtype=torch.uint8, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    lab, sst, out, dy, bce_part, mm_part = (r[k].cuda() for k in ("label", "sst", "out", "dy", "bce_part", "mm_part"))
    _C.check(lib.fr_nfcf_loss_tail(lab.data_ptr(), sst.data_ptr(), B, 0.5, None, 0, 64, out.data_ptr(), dy.data_ptr(),
                                   loss.data_ptr(), bce_part.data_ptr(), mm_part.data_ptr(), r["nblk"], ws.data_ptr(), ws.numel(),
                                   err.data_ptr(), _C.current_stream()), "fr_nfcf_loss_tail")
    got = loss.cpu()
    assert bool(torch.isfinite(got).all()) and int(err.cpu()) == 0
    # (the oracle in its own fp32 arithmetic: this batch's saturated negative rows cost the clamp, 100, there and here)
    ref, _ = O.loss("pretrain", 0.5, r["x0"], r["x1"], r["params"][0::2], r["params"][1::2], torch.arange(B), torch.arange(B),
                    r["label"], r["sst"])
    assert abs(float(got[0]) - float(ref)) <= 1e-5 * float(ref), (got.tolist(), float(ref))
    assert float(got[1]) == float(got[0]) and float(got[2]) == 0.0
    assert abs(float(got[0]) - float(r["loss"][0])) <= 1e-6 * float(got[0])      # the launch's own closure: the same mean


def test_loss_closure_across_block_counts():
    """Consecutive launches that close their own loss on ONE arrival word, 1 -> 300 -> 2 -> 257 workgroups: each loss is its
    batch's float64 mean BCE, and the word is back at 0 after each."""
    _C = _c()
    lib = _C.lib()
    ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
    for B in (17, 9590, 33, 8193):
        assert lib.fr_scorer_blocks(B) in (1, 300, 2, 257)
        r = _prep_closing(32, 32, 32, B, seed=B)
        _launch_closing(r, ticket)
        _check_loss(r)
        assert int(ticket.cpu()) == 0


def _prep_closing(k0, n1, n2, B, seed):
    """Inputs and output buffers of a forward that closes its own loss (no dropout), on the device."""
    from fairrec.model.fair_recommender.nfcf import _NfcfFused
    _C = _c()
    lib = _C.lib()
    x0, x1, params, label, sst = _data(k0, n1, n2, B, seed)
    P = [t.cuda() for t in params]
    d = _NfcfFused._desc(k0, k0, P, 0.0, 0, B)
    nblk = lib.fr_scorer_blocks(B)
    f32 = dict(dtype=torch.float32, device="cuda")
    r = dict(B=B, label=label, P=P, x0=x0.cuda(), x1=x1.cuda(), lab=label.cuda(), h1=torch.empty((B, n1), **f32),
             h2=torch.empty((B, n2), **f32), y=torch.empty(B, **f32), out=torch.empty(B, **f32), dy=torch.empty(B, **f32),
             part=torch.empty(nblk, **f32), loss=torch.full((3,), float("nan"), **f32), nblk=nblk, d=d)
    return r


def _launch_closing(r, ticket, stream=None):
    _C = _c()
    lib, B, d = _C.lib(), r["B"], r["d"]
    st = stream if stream is not None else _C.current_stream()
    _C.check(lib.fr_scorer_fwd(ctypes.byref(d), r["x0"].data_ptr(), r["x1"].data_ptr(), B, None, None, None, None, None,
                               r["h1"].data_ptr(), r["h2"].data_ptr(), r["y"].data_ptr(), r["lab"].data_ptr(), None,
                               r["out"].data_ptr(), r["dy"].data_ptr(), r["part"].data_ptr(), None, r["loss"].data_ptr(),
                               ticket.data_ptr(), st), "fr_scorer_fwd")


def _check_loss(r):
    y, loss = r["y"].cpu(), r["loss"].cpu()
    _, _, l_ref, _, _, tol_l, _ = _head_ref(y, r["label"])
    B = r["B"]
    bnd = float((tol_l.sum() + (r["nblk"] + 40) * U * l_ref.abs().sum()) / B)
    ref = float(l_ref.sum() / B)
    _ratio("loss", abs(float(loss[0]) - ref) / bnd)
    assert abs(float(loss[0]) - ref) <= bnd and float(loss[1]) == float(loss[0]) and float(loss[2]) == 0.0, \
        (B, loss.tolist(), ref, bnd)


def test_loss_closure_from_two_host_threads():
    """Two host threads, each with its own stream, buffers and arrival word, each closing ~50 losses at different batch
    sizes: every loss is its own batch's mean BCE (a counter shared between concurrent launches would mix them)."""
    _C = _c()
    results, errs = [[], []], []
    sizes = [[257 + 997 * j % 7000 for j in range(50)], [9000 - 613 * j % 8000 for j in range(50)]]
    tickets = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2)]
    prepared = [[_prep_closing(32, 32, 32, B, seed=1000 * t + j) for j, B in enumerate(sizes[t])] for t in range(2)]
    torch.cuda.synchronize()
    # both streams wait behind a spin on a third one while the threads queue their launches: when it ends, the two queues
    # drain side by side and the launches' workgroups interleave on the device
    hold = torch.cuda.Stream()
    with torch.cuda.stream(hold):
        torch.cuda._sleep(200_000_000)
    gate = threading.Barrier(2)

    def run(t):
        try:
            s = torch.cuda.Stream()
            s.wait_stream(hold)
            with torch.cuda.stream(s):
                gate.wait()
                for r in prepared[t]:          # back to back: the two threads' launches overlap on the device
                    _launch_closing(r, tickets[t], stream=_C.current_stream())
                    results[t].append(r)
            s.synchronize()
        except Exception as e:       # noqa: BLE001 -- re-raised in the main thread
            errs.append(e)

    th = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    torch.cuda.synchronize()
    for rs in results:
        assert len(rs) == 50
        for r in rs:
            _check_loss(r)
    assert int(tickets[0].cpu()) == 0 and int(tickets[1].cpu()) == 0


def test_two_identical_launches_are_bit_equal():
    a = _launch(160, 96, 64, 1000, 0.2, gscale=0.9, close_loss=True)
    b = _launch(160, 96, 64, 1000, 0.2, gscale=0.9, close_loss=True)
    for k in ("x0d", "x1d", "h1", "h2", "y", "out", "dy", "bce_part", "mm_part", "loss", "dz1", "dz2", "dz3", "dx0", "dx1",
              "w3part", "dW1", "db1", "dW2", "db2", "w3", "w3s"):
        assert torch.equal(a[k], b[k]), k


# ---- the dispatch boundary ------------------------------------------------------------------------------------------------
def _fwd_rc(k0, k1, n1, n2, p, B=64, shift=None):
    """fr_scorer_supported and fr_scorer_fwd's return code for a descriptor; every buffer is real and large enough, `shift`
    moves one operand 4 bytes off 16-byte alignment (inside its allocation)."""
    _C = _c()
    lib = _C.lib()
    K = k0 + k1
    t = lambda *s: torch.zeros(*s, device="cuda")      # noqa: E731
    bufs = dict(W1=t(n1 * K + 4), b1=t(n1), W2=t(n2 * n1 + 4), b2=t(n2), W3=t(n2 + 4), b3=t(1), x0=t(B * k0 + 4),
                x1=t(B * k1 + 4), h1=t(B * n1), h2=t(B * n2), y=t(B), out=t(B), dy=t(B), part=t(3 * B))
    ptr = {k: v.data_ptr() + (4 if k == shift else 0) for k, v in bufs.items()}
    d = _C.FrScorer(k0, k1, n1, n2, ptr["W1"], ptr["b1"], ptr["W2"], ptr["b2"], ptr["W3"], ptr["b3"], p, 1, 0, 0, 0, 0)
    sup = lib.fr_scorer_supported(ctypes.byref(d))
    rc = lib.fr_scorer_fwd(ctypes.byref(d), ptr["x0"], ptr["x1"], B, None, None, None, None, None, ptr["h1"], ptr["h2"],
                           ptr["y"], ptr["y"], None, ptr["out"], ptr["dy"], ptr["part"], None, None, None, _C.current_stream())
    torch.cuda.synchronize()
    return sup, rc


REFUSED = [(16, 16, 128, 64, 0.0), (64, 32, 128, 64, 0.0), (288, 288, 128, 64, 0.0), (64, 64, 48, 64, 0.0),
           (64, 64, 160, 64, 0.0), (64, 64, 128, 16, 0.0), (64, 64, 128, 96, 0.0), (64, 64, 128, 64, 1.0),
           (64, 64, 128, 64, -0.1)]


@pytest.mark.parametrize("k0,k1,n1,n2,p", REFUSED, ids=["k16", "k0_ne_k1", "k288", "n1_48", "n1_160", "n2_16", "n2_96", "p1",
                                                        "p_negative"])
def test_refused_shapes(k0, k1, n1, n2, p):
    assert _fwd_rc(k0, k1, n1, n2, p) == (0, -1)        # FR_EINVAL


@pytest.mark.parametrize("operand", ["W1", "x0"])
def test_misaligned_operand_is_refused_before_launch(operand):
    assert _fwd_rc(64, 64, 128, 64, 0.0) == (1, 0)
    assert _fwd_rc(64, 64, 128, 64, 0.0, shift=operand) == (1, -1)


def _model(D, hidden, finetune, n_users=400, n_items=300, seed=0):
    from fairrec.config import Config
    from fairrec.model.fair_recommender.nfcf import NFCF
    from tests_helpers import NfcfDataset
    g = torch.Generator().manual_seed(seed)
    gender = (torch.rand(n_users, generator=g) < 0.5).float().numpy()
    torch.manual_seed(seed)
    cfg = Config(model="NFCF", config_dict={"embedding_size": D, "mlp_hidden_size": list(hidden), "dropout": 0.0,
                                            "fair_weight": 0.3, "device": "cuda", "load_pretrain_path": None})
    m = NFCF(cfg, NfcfDataset(n_users, n_items, gender))
    with torch.no_grad():
        m.user_embedding.weight.mul_(0.5)
        m.item_embedding.weight.mul_(0.5)
        for lin in m.mlp_layers.linears():
            lin.bias.add_(0.05)
    if finetune:
        m.load_pretrain_path = "a-checkpoint"
        m.user_embedding.weight.requires_grad = False
    return m.to("cuda").train(), gender


def _against_oracle(m, gender, u, i, label, stage):
    from fairrec.data.interaction import Interaction
    from oracle import nfcf as O
    lins = m.mlp_layers.linears()
    tables = [("user_embedding.weight", stage == "pretrain"), ("item_embedding.weight", True)]      # (name, trains)
    U64 = m.user_embedding.weight.detach().cpu().double().requires_grad_(stage == "pretrain")
    I64 = m.item_embedding.weight.detach().cpu().double().requires_grad_()
    Ws = [lin.weight.detach().cpu().double().requires_grad_() for lin in lins]
    bs = [lin.bias.detach().cpu().double().requires_grad_() for lin in lins]
    sst = torch.from_numpy(gender)[u].double()
    ref, _ = O.loss(stage, 0.3, U64, I64, Ws, bs, u, i, label.double(), sst)
    ref.backward()
    ref = ref.detach()
    from fairrec.optim import FusedLazyAdam
    inter = Interaction({"user_id": u, "item_id": i, "label": label, "gender": torch.from_numpy(gender)[u]}).to("cuda")
    opt = FusedLazyAdam(m.hip_engine(), lr=1e-3)
    opt.zero_grad()
    loss = m.calculate_loss(inter)
    loss.backward()
    m.hip_engine().check_device_errors()
    assert abs(float(loss.detach()) - float(ref)) <= 2e-5 * abs(float(ref)), (float(loss.detach()), float(ref))
    pairs = [(lin.weight.grad, W.grad) for lin, W in zip(lins, Ws)] + [(lin.bias.grad, b.grad) for lin, b in zip(lins, bs)]
    eng = m.hip_engine()
    for (name, trains), ref_t in zip(tables, (U64, I64)):
        t = eng._tables[name]
        if not trains:
            assert t._grad_rows is None, name          # the frozen table receives no gradient
            continue
        # the table's gradient as the engine holds it after backward(): one row per batch position, summed per id here
        dense = torch.zeros(t.n_rows, t.dim, dtype=torch.float64)
        dense.index_add_(0, t._keep.cpu(), t._grad_rows.cpu().double())
        pairs.append((dense, ref_t.grad))
    for got, want in pairs:
        err = (got.cpu().double() - want).abs()
        assert bool(torch.isfinite(got).all()) and float(err.max()) <= 1e-4 * float(want.abs().max()) + 1e-9, \
            (tuple(want.shape), float(err.max()), float(want.abs().max()))


def test_fallback_shape_matches_the_oracle():
    """Just outside the fused boundary (D = 48, [160, 64]): the layer-by-layer path, held to the same float64 oracle."""
    m, gender = _model(48, (160, 64), finetune=False)
    assert not m._fused_scorer()
    g = torch.Generator().manual_seed(5)
    B = 777
    u, i = torch.randint(1, 400, (B,), generator=g), torch.randint(1, 300, (B,), generator=g)
    _against_oracle(m, gender, u, i, (torch.rand(B, generator=g) < 0.5).float(), "pretrain")


def test_fused_finetune_with_the_fairness_tail_matches_the_oracle():
    """D = 96, [32, 32], B = 1000 in the finetune stage (user table frozen, differential fairness behind the scorer): items
    whose positives all fall in one group, 32-row workgroups without a positive row."""
    m, gender = _model(96, (32, 32), finetune=True)
    assert m._fused_scorer()
    g = torch.Generator().manual_seed(6)
    B = 1000
    u, i = torch.randint(1, 400, (B,), generator=g), torch.randint(1, 300, (B,), generator=g)
    label = (torch.rand(B, generator=g) < 0.5).float()
    label[64:160] = 0.0                                  # workgroups 2..4: no positive row
    g0 = torch.from_numpy(gender)[u] == 0
    one_group = (i % 7 == 0)                             # these items' positives: group 0 only
    label[one_group & ~g0] = 0.0
    assert int((label[one_group] == 1).sum()) > 0
    _against_oracle(m, gender, u, i, label, "finetune")

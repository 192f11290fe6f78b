"""References of the sensitive-attribute leakage probe (csrc/probe.hip, fairrec/evaluator/leakage.py): plain numpy / torch on the
CPU, no GPU, no fairrec.  tests/test_probe_ref.py pins them to torch autograd and sklearn; tests/test_probe_hip.py and
tests/test_leakage_hip.py compare the kernels and the package with them.

* `layout`: the flat parameter layout [head][W1 | b1 | W2 | b2] (H == 0: [W | b]).
* `step_f64`: one optimiser step of all heads on one batch in float64 from the kernel's float32 inputs: per-head mean softmax
  cross-entropy, flat gradient, Adam (torch's formulas, no weight decay).  relu' = (z1 > 0).  `drop` rows contribute nothing
  (the divisor stays B); `drop_head` = per head rows that contribute nothing to that head alone.
* `step_f32`: the kernel's formulas restated in float32 in the kernel's order: every product an ascending fma chain from 0
  (one fma per inner index: what a chain of v_mfma_f32_32x32x2_f32 computes), gradients per 32-row tile, tiles added per
  workgroup, workgroups added in order under the grid rule `grid`; softmax as fr_softmax_ce writes it; Adam as adam_elem
  (exp, log, sqrt and the reciprocal from numpy, correctly rounded or within half an ulp or so).
* `probe_f64`: the whole procedure of the probe (split, init, epochs, metrics) in float64, host randomness as the package draws it.
* `macro_auc`, `metrics`: the result keys from test probabilities.
* `cases`: the shapes tests/test_probe_hip.py runs, `make_case` their inputs; MEASURED the worst error of step_f32 against
  step_f64 over them, in units of u (|ref| + max |ref|), u = 2^-24 (asserted by tests/test_probe_ref.py: the restatement
  does not exceed it and reaches half of it).  The kernel tests allow MEASURED * 8 (loss_ref.py states the rule).
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
SAFETY = 8.0
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
TILE, MAX_WG = 32, 256

# worst error of step_f32 against step_f64 over cases(), units of u (|ref| + max |ref|): test_probe_ref.py prints and asserts
MEASURED = {"loss": 1.5, "grad": 4.3, "param": 0.5}


def tol_const(key):
    return SAFETY * MEASURED[key]


def grid(B):
    """(tiles, tiles per workgroup, workgroups) of fr_probe_step: a function of B alone"""
    tiles = (B + TILE - 1) // TILE
    tpw = (tiles + MAX_WG - 1) // MAX_WG
    return tiles, tpw, (tiles + tpw - 1) // tpw


def head_params(D, H, C):
    return H * D + H + C * H + C if H else C * D + C


def layout(D, H, classes):
    """per head: dict of (offset, shape) for W1, b1, W2, b2 (H == 0: W2 = W [C, D], b2 = b); and the total"""
    out, off = [], 0
    for C in classes:
        d = {}
        if H:
            d["W1"] = (off, (H, D)); off += H * D
            d["b1"] = (off, (H,)); off += H
        n_in = H if H else D
        d["W2"] = (off, (C, n_in)); off += C * n_in
        d["b2"] = (off, (C,)); off += C
        out.append(d)
    return out, off


def _get(flat, entry):
    off, shape = entry
    return flat[off:off + int(np.prod(shape))].reshape(shape)


def init_params(g, D, H, classes):
    """float32 flat parameters: per head, in order, W1, b1, W2, b2 uniform in +-1/sqrt(fan_in) from the torch generator g"""
    lay, P = layout(D, H, classes)
    flat = torch.empty(P, dtype=torch.float32)
    for d in lay:
        for name in ("W1", "b1", "W2", "b2"):
            if name not in d:
                continue
            off, shape = d[name]
            fan_in = D if name in ("W1", "b1") or not H else H
            bound = 1.0 / math.sqrt(fan_in)
            n = int(np.prod(shape))
            flat[off:off + n] = (torch.rand(n, generator=g, dtype=torch.float32) * 2.0 - 1.0) * bound
    return flat


def adam_f64(p, g, m, v, lr, step):
    m = BETA1 * m + (1.0 - BETA1) * g
    v = BETA2 * v + (1.0 - BETA2) * g * g
    bc1, bc2 = 1.0 - BETA1 ** step, 1.0 - BETA2 ** step
    p = p - (lr / bc1) * m / (np.sqrt(v) / math.sqrt(bc2) + EPS)
    return p, m, v


def forward_f64(params, X, D, H, classes):
    """logits [n, sum C] in float64"""
    lay, _ = layout(D, H, classes)
    params, X = np.asarray(params, dtype=np.float64), np.asarray(X, dtype=np.float64)
    out = []
    for d in lay:
        hid = np.maximum(X @ _get(params, d["W1"]).T + _get(params, d["b1"]), 0.0) if H else X
        out.append(hid @ _get(params, d["W2"]).T + _get(params, d["b2"]))
    return np.concatenate(out, axis=1)


def step_f64(params, m, v, X, labels, D, H, classes, lr, step, drop=None, drop_head=None):
    """X [B, D] (the batch's rows, gathered), labels [n_heads, B] -> dict(loss [1 + heads], grad, params, m, v)"""
    lay, P = layout(D, H, classes)
    params, m, v, X = (np.asarray(a, dtype=np.float64) for a in (params, m, v, X))
    B = X.shape[0]
    grad, loss = np.zeros(P), np.zeros(1 + len(classes))
    for a, (d, C) in enumerate(zip(lay, classes)):
        keep = np.ones(B, dtype=bool)
        if drop is not None:
            keep &= ~np.asarray(drop, dtype=bool)
        if drop_head is not None and drop_head[a] is not None:
            keep &= ~np.asarray(drop_head[a], dtype=bool)
        y = np.where(keep, labels[a], 0)
        if H:
            W1, b1 = _get(params, d["W1"]), _get(params, d["b1"])
            z1 = X @ W1.T + b1
            hid = np.maximum(z1, 0.0)
        else:
            hid = X
        W2, b2 = _get(params, d["W2"]), _get(params, d["b2"])
        z2 = hid @ W2.T + b2
        mx = z2.max(axis=1, keepdims=True)
        e = np.exp(z2 - mx)
        se = e.sum(axis=1, keepdims=True)
        term = np.log(se[:, 0]) - (z2[np.arange(B), y] - mx[:, 0])
        loss[1 + a] = (term * keep).sum() / B
        dz2 = e / se
        dz2[np.arange(B), y] -= 1.0
        dz2 = dz2 * keep[:, None] / B
        _get(grad, d["W2"])[...] = dz2.T @ hid
        _get(grad, d["b2"])[...] = dz2.sum(axis=0)
        if H:
            dz1 = (dz2 @ W2) * (z1 > 0)
            _get(grad, d["W1"])[...] = dz1.T @ X
            _get(grad, d["b1"])[...] = dz1.sum(axis=0)
    loss[0] = loss[1:].sum()
    p2, m2, v2 = adam_f64(params, grad, m, v, lr, step)
    return dict(loss=loss, grad=grad, params=p2, m=m2, v=v2)


# ---- the float32 restatement ---------------------------------------------------------------------------------------------------

F = np.float32


def _fma(a, b, c):
    """float32 fma: the product of two float32 is exact in float64; one rounding of the sum to float64, one to float32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def _chain(A, Bm):
    """[n, K] x [K, m] -> [n, m]: per cell an fma chain ascending over k from 0"""
    acc = np.zeros((A.shape[0], Bm.shape[1]), dtype=F)
    for k in range(A.shape[1]):
        acc = _fma(A[:, k:k + 1], Bm[k:k + 1, :], acc)
    return acc


def _colsum(T):
    a = np.zeros(T.shape[1], dtype=F)
    for r in range(T.shape[0]):
        a = (a + T[r]).astype(F)
    return a


def step_f32(params, m, v, X, labels, D, H, classes, lr, step):
    lay, P = layout(D, H, classes)
    params, m, v, X = (np.asarray(a, dtype=F) for a in (params, m, v, X))
    B = X.shape[0]
    tiles, tpw, wgs = grid(B)
    total = np.zeros(P, dtype=F)
    loss_heads = np.zeros(len(classes), dtype=F)
    for w in range(wgs):
        slot = None
        lacc = np.zeros((len(classes), TILE), dtype=F)
        for t in range(w * tpw, min((w + 1) * tpw, tiles)):
            xs = np.zeros((TILE, D), dtype=F)
            n = min(TILE, B - t * TILE)
            xs[:n] = X[t * TILE:t * TILE + n]
            g = np.zeros(P, dtype=F)
            for a, (d, C) in enumerate(zip(lay, classes)):
                y = np.full(TILE, -1)
                y[:n] = labels[a][t * TILE:t * TILE + n]
                if H:
                    W1, b1 = _get(params, d["W1"]), _get(params, d["b1"])
                    z1 = (_chain(xs, W1.T.copy()) + b1).astype(F)
                    hid = np.where(z1 < 0, F(0), z1).astype(F)
                else:
                    hid = xs
                W2, b2 = _get(params, d["W2"]), _get(params, d["b2"])
                z2 = (_chain(hid, W2.T.copy()) + b2).astype(F)
                dz2 = np.zeros((TILE, C), dtype=F)
                for r in range(n):
                    z = z2[r]
                    mx = z.max()
                    e = np.exp((z - mx).astype(F)).astype(F)
                    se = F(0)
                    for c in range(C):
                        se = F(se + e[c])
                    lacc[a, r] = F(lacc[a, r] + F(F(np.log(se)) - F(z[y[r]] - mx)))
                    one = np.zeros(C, dtype=F)
                    one[y[r]] = 1
                    dz2[r] = ((e / se).astype(F) - one).astype(F) / F(B)
                _get(g, d["W2"])[...] = _chain(dz2.T.copy(), hid)
                _get(g, d["b2"])[...] = _colsum(dz2)
                if H:
                    dz1 = np.where(hid > 0, _chain(dz2, W2), F(0)).astype(F)
                    _get(g, d["W1"])[...] = _chain(dz1.T.copy(), xs)
                    _get(g, d["b1"])[...] = _colsum(dz1)
            slot = g if slot is None else (slot + g).astype(F)
        total = slot if w == 0 else (total + slot).astype(F)
        part = np.zeros(len(classes), dtype=F)
        for r in range(TILE):
            part = (part + lacc[:, r]).astype(F)
        loss_heads = (loss_heads + part).astype(F)
    loss_heads = (loss_heads * F(F(1) / F(B))).astype(F)
    loss = np.zeros(1 + len(classes), dtype=F)
    loss[1:] = loss_heads
    for a in range(len(classes)):
        loss[0] = F(loss[0] + loss_heads[a])
    # adam_elem (csrc/common.hpp), weight decay 0
    ss, ib = F(lr / (1.0 - BETA1 ** step)), F(1.0 / math.sqrt(1.0 - BETA2 ** step))
    omb1, omb2, b2c, eps = F(1.0 - BETA1), F(1.0 - BETA2), F(BETA2), F(EPS)
    g = total
    m2 = _fma(np.full(P, omb1), (g - m).astype(F), m)
    v2 = _fma((omb2 * g).astype(F), g, (v * b2c).astype(F))
    den = _fma(np.sqrt(v2).astype(F), np.full(P, ib), np.full(P, eps))
    p2 = _fma((-ss * m2).astype(F), (F(1) / den).astype(F), params)
    return dict(loss=loss, grad=total, params=p2, m=m2, v=v2)


# ---- metrics -------------------------------------------------------------------------------------------------------------------

def binary_auc(score, pos):
    """P(score of a positive > score of a negative) + half the ties, by ranks (ties share the mean rank)"""
    score, pos = np.asarray(score), np.asarray(pos, dtype=bool)
    order = np.argsort(score, kind="stable")
    s = score[order]
    ranks = np.empty(len(s))
    i = 0
    while i < len(s):
        j = i
        while j + 1 < len(s) and s[j + 1] == s[i]:
            j += 1
        ranks[order[i:j + 1]] = 0.5 * (i + j) + 1.0
        i = j + 1
    n1, n0 = int(pos.sum()), int((~pos).sum())
    return (ranks[pos].sum() - n1 * (n1 + 1) / 2.0) / (n1 * n0)


def macro_auc(probs, y):
    """C == 2: the AUC of p(class 1); else the mean one-vs-rest AUC over the classes with a positive and a negative row"""
    probs, y = np.asarray(probs), np.asarray(y)
    C = probs.shape[1]
    if C == 2:
        return binary_auc(probs[:, 1], y == 1)
    vals = [binary_auc(probs[:, c], y == c) for c in range(C) if 0 < int((y == c).sum()) < len(y)]
    return float(np.mean(vals))


def metrics(logits, y_test, y_train, C):
    """-> dict(auc, accuracy, majority, logloss) of one head from its test logits [n, C] (float64)"""
    z = np.asarray(logits, dtype=np.float64)
    mx = z.max(axis=1, keepdims=True)
    e = np.exp(z - mx)
    se = e.sum(axis=1, keepdims=True)
    n = len(y_test)
    return dict(auc=macro_auc(e / se, y_test), accuracy=float((z.argmax(axis=1) == y_test).mean()),
                majority=float((y_test == np.bincount(y_train, minlength=C).argmax()).mean()),
                logloss=float((np.log(se[:, 0]) - (z[np.arange(n), y_test] - mx[:, 0])).sum() / n))


def split(U_rows, test_ratio, g):
    perm = torch.randperm(U_rows, generator=g)
    n_test = int(math.floor(test_ratio * U_rows))
    return perm[:n_test].numpy(), perm[n_test:].numpy()


def probe_f64(X, labels, hidden, epochs, batch, lr, test_ratio, seed):
    """The whole probe in float64.  X [U, D] float32, labels: dict name -> int array [U] of class indices 0..C-1 (every class
    present).  -> dict name -> metrics dict.  Host randomness: one generator; the split, the heads' init, one permutation per
    epoch."""
    X = np.asarray(X, dtype=np.float32)
    names = list(labels)
    lab = np.stack([np.asarray(labels[k]) for k in names])
    classes = [int(l.max()) + 1 for l in lab]
    n_rows, D = X.shape
    g = torch.Generator().manual_seed(seed)
    test, train = split(n_rows, test_ratio, g)
    params = init_params(g, D, hidden, classes).numpy().astype(np.float64)
    m, v = np.zeros_like(params), np.zeros_like(params)
    step = 0
    for _ in range(epochs):
        order = train[torch.randperm(len(train), generator=g).numpy()]
        for s in range(0, len(order), batch):
            rows = order[s:s + batch]
            step += 1
            r = step_f64(params, m, v, X[rows], lab[:, rows], D, hidden, classes, lr, step)
            params, m, v = r["params"], r["m"], r["v"]
    z = forward_f64(params, X[test], D, hidden, classes)
    out, off = {}, 0
    for a, k in enumerate(names):
        out[k] = metrics(z[:, off:off + classes[a]], lab[a][test], lab[a][train], classes[a])
        off += classes[a]
    return out


# the three data sets of tests/test_leakage_hip.py and tests/test_probe_ref.py
LEAK = dict(U=10000, D=16, hidden=16, test_ratio=0.2, lr=0.01, batch=1024, epochs=20, seed=2020)


def leak_data(kind):
    rng = np.random.default_rng([7, {"planted": 0, "independent": 1, "seven": 2}[kind]])
    X = rng.standard_normal((LEAK["U"], LEAK["D"])).astype(np.float32)
    if kind == "seven":
        y = rng.integers(0, 7, LEAK["U"])
    else:
        y = rng.integers(0, 2, LEAK["U"])
        if kind == "planted":
            X[:, 0] += (2.0 * (2 * y - 1)).astype(np.float32)
    return X, y.astype(np.int64)


# ---- the kernel cases ------------------------------------------------------------------------------------------------------------

BIG_B = 257 * 32 + 5        # 258 tiles: two tiles per workgroup, 129 workgroups


def cases():
    """(B, D, H, classes, tag): every B at a mid shape, every D and H at B = 33, the head lists, and the special inputs"""
    out = []
    for B in (1, 31, 32, 33, 65):
        out.append((B, 5, 7, (3,), "plain"))
        out.append((B, 5, 0, (2, 3), "plain"))
    out.append((BIG_B, 3, 2, (2, 3), "plain"))
    out.append((BIG_B, 3, 0, (2,), "plain"))
    for D in (1, 2, 3, 63, 64, 65, 256):
        out.append((33, D, 33, (3,), "plain"))
        out.append((33, D, 0, (3,), "plain"))
    for H in (1, 31, 32, 33, 128, 129, 256):
        out.append((33, 9, H, (2, 7), "plain"))
    for cl in ((2,), (3,), (2, 7, 21), (64,), (2,) * 8):
        out.append((65, 6, 5, cl, "plain"))
        out.append((65, 6, 0, cl, "plain"))
    out.append((33, 256, 256, (64,), "plain"))
    out.append((65, 6, 5, (3, 4), "absent"))        # class 1 of head 0 absent from the batch
    out.append((65, 6, 5, (3,), "saturated"))       # |z2| ~ 80 in class 0
    out.append((65, 6, 5, (3,), "relu_edge"))       # z1 exactly 0 in unit 0 of row 0
    out.append((65, 6, 0, (3,), "saturated"))
    return out


def make_case(B, D, H, classes, tag, seed=0):
    """-> dict(X [B, D] float32, labels [heads, B] int64, params, m, v float32, lr, step): a step in mid-training (nonzero
    m, a v well above eps^2, so that the update is a smooth function of the gradient)"""
    rng = np.random.default_rng([seed, B, D, H, len(classes), sum(classes)])
    lay, P = layout(D, H, classes)
    X = rng.standard_normal((B, D)).astype(np.float32)
    labels = np.stack([rng.integers(0, C, B) for C in classes]).astype(np.int64)
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    params = init_params(g, D, H, classes).numpy()
    if tag == "absent":
        labels[0][labels[0] == 1] = 2
        assert not (labels[0] == 1).any()
    if tag == "saturated":
        _get(params, lay[0]["b2"])[0] = np.float32(80.0)
    if tag == "relu_edge":
        _get(params, lay[0]["W1"])[0, :] = 0.0
        _get(params, lay[0]["b1"])[0] = 0.0
        X[0, :] = np.float32(0.5)
    m = (rng.standard_normal(P) * 0.05).astype(np.float32)
    v = rng.uniform(0.01, 0.1, P).astype(np.float32)
    return dict(X=X, labels=labels, params=params, m=m, v=v, lr=1e-3, step=5)

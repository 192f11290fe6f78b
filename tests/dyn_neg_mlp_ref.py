"""numpy float64 restatement of fr_dyn_neg_mlp_select / fr_dyn_neg_mlp_scores (include/fairrec_hip.h,
csrc/dyn_neg_mlp.hip), for the tests, and the seeded cases the CPU and the GPU tests share.

The entry takes fp32 inputs: the candidates' rows as of the table's step (`rows` [M*num*n, D], in cand's order: what
LazyTable.gather returns for cand), P [n, n1] (the user half of the first layer, b1 added), the item half W1i [n1, D] of the
first weight, the remaining `layers` (W [n_out, n_in], bias [n_out]; the last has one output).  Candidate k = (r*num + j)*n +
i belongs to output column c = j*n + i, round r, and to row i of P:

    z1 = P[i] + rows[k] W1i^T,   score = sigmoid(relu(... relu(W[0] relu(z1) + bias[0]) ...))

The rounding bound is tests/pair_mlp_ref.py's (`upper_bound`), entered with the first layer's own error: the kernel forms
q = rows[k] W1i^T as a chain of D fmas and adds P[i] once -- gamma_(D + 1) over sum_k |W1i[j, k]| |rows[k]|, and one rounding
u |z1| of the add (u = 2^-24, gamma_n = n u / (1 - n u)), plus (D + 4) 2^-126 for underflow.

The pick of a column follows torch.max(dim=0): the lowest r among equal maxima, a NaN beats every number, the first NaN
wins.  A pick is DECIDED when the float64 gap between the best score and the runner-up exceeds the sum of their two bounds
(then every fp32 evaluation inside the bounds picks the same candidate); a column with one candidate, or with a NaN, is
decided."""
import ctypes

import numpy as np

from mlp_infer_ref import TINY, U, gamma
from pair_mlp_ref import random_layers, upper64, upper_bound

UNDECIDED_CAP = 0.05


def z1_of(rows, P, W1i, n):
    """First-layer pre-activations [K, n1] in float64 and the magnitude sum_k |W1i[j, k]| |rows[k]| of the in-kernel product."""
    rows, P, W1i = (np.asarray(t, np.float64) for t in (rows, P, W1i))
    i = np.arange(rows.shape[0]) % n
    return P[i] + rows @ W1i.T, np.abs(rows) @ np.abs(W1i).T


def scores64(rows, P, W1i, layers, n):
    """The [M*num*n] scores in float64, in cand's order."""
    return upper64(z1_of(rows, P, W1i, n)[0], layers)


def bound(rows, P, W1i, layers, n):
    """(float64 scores [K], rounding bound [K]) of the entry."""
    D = np.asarray(rows).shape[1]
    z1, mag = z1_of(rows, P, W1i, n)
    return upper_bound(z1, U * np.abs(z1) + gamma(D + 1) * mag + (D + 4) * TINY, layers)


def concat64(x, rows, W1, b1, layers, n):
    """The plain MLP on cat(x[i], rows[k]) in float64, no split: x [n, D_user], W1 [n1, D_user + D]."""
    x, rows = np.asarray(x, np.float64), np.asarray(rows, np.float64)
    cat = np.concatenate([x[np.arange(rows.shape[0]) % n], rows], axis=1)
    return upper64(cat @ np.asarray(W1, np.float64).T + np.asarray(b1, np.float64), layers)


def pick(scores):
    """Index r of the pick of every column of [M, cols] scores: torch.max(dim=0)'s."""
    scores = np.asarray(scores)
    nan = np.isnan(scores)
    best = np.where(nan, -np.inf, scores).argmax(axis=0)          # the first maximum
    return np.where(nan.any(axis=0), nan.argmax(axis=0), best)    # the first NaN


def decided(scores, bounds):
    """Which columns of [M, cols] float64 scores have a decided pick under the [M, cols] bounds."""
    scores, bounds = np.asarray(scores, np.float64), np.asarray(bounds, np.float64)
    M, cols = scores.shape
    nan = np.isnan(scores).any(axis=0)
    if M == 1:
        return np.ones(cols, bool)
    order = np.argsort(-np.where(np.isnan(scores), -np.inf, scores), axis=0, kind="stable")[:2]
    c = np.arange(cols)
    with np.errstate(invalid="ignore"):
        gap = scores[order[0], c] - scores[order[1], c]
        return nan | (gap > bounds[order[0], c] + bounds[order[1], c])


def select(scores, cand):
    """(ids [cols], r [cols]) the entry returns for [M, cols] scores and candidates."""
    r = pick(scores)
    return np.asarray(cand)[r, np.arange(np.asarray(scores).shape[1])], r


# ---- the seeded cases ------------------------------------------------------------------------------------------------------
N_ITEMS = 300
TABLES = ("adam", "sgd", "adagrad", "rmsprop", "fresh")      # aged under the learner with weight decay | nothing behind

CASES = {}
for _n in (1, 33):
    for _num in (1, 2):
        for _M in (1, 3):
            CASES[f"n{_n}-num{_num}-M{_M}"] = dict(n=_n, num=_num, M=_M, D=16, widths=[24, 16, 1])
for _D in (1, 31, 33, 65, 256):
    CASES[f"D{_D}"] = dict(n=33, num=2, M=3, D=_D, widths=[16, 16, 1])
for _n1 in (1, 33, 128, 129):
    CASES[f"n1-{_n1}-direct"] = dict(n=33, num=2, M=3, D=16, widths=[_n1, 1])
    CASES[f"n1-{_n1}-hidden"] = dict(n=33, num=2, M=3, D=33, widths=[_n1, 16, 1])
CASES["net-33-17-9-1"] = dict(n=33, num=2, M=3, D=31, widths=[33, 17, 9, 1])
CASES["net-256-256-256-1"] = dict(n=33, num=1, M=1, D=33, widths=[256, 256, 256, 1])       # streamed upper weights
CASES["nfcf-yaml"] = dict(n=70, num=1, M=4, D=64, widths=[128, 64, 1])
for _k, _name in enumerate(CASES):
    CASES[_name].update(seed=1000 + _k, table=TABLES[_k % len(TABLES)])


def make_case(name):
    """The fp32 inputs of case `name` but for the table's state: the initial item table `table0` [N_ITEMS, D], the user rows
    `x` [n, D], the first layer (W1 [n1, 2 D], b1), the upper layers and the candidate ids `cand` [M*num*n]."""
    c = dict(CASES[name])
    rng = np.random.default_rng(c["seed"])
    n, num, M, D, widths = c["n"], c["num"], c["M"], c["D"], c["widths"]
    c["table0"] = rng.standard_normal((N_ITEMS, D)).astype(np.float32)
    c["x"] = rng.standard_normal((n, D)).astype(np.float32)
    c["W1"] = (rng.standard_normal((widths[0], 2 * D)) / np.sqrt(2 * D)).astype(np.float32)
    c["b1"] = (0.5 * rng.standard_normal(widths[0])).astype(np.float32)
    narrow = widths[0] < 8  # (a narrow first layer with its units dead gives every candidate of a column the same score)
    if narrow:
        c["b1"] = (np.float32(4) + np.abs(c["b1"])).astype(np.float32)
    layers = random_layers(rng, widths)
    # (the last layer's weights halved and its bias in [1, 1.5 + ...): the last ReLU then passes the candidates on -- a negative
    # pre-activation scores 0.5 exactly whatever the layers below computed, and a user whose candidates all end there leaves
    # the column undecided -- and the scores stay where the sigmoid's slope is near the 1/4 the bound grants it)
    layers[-1] = ((np.float32(0.5) * layers[-1][0]).astype(np.float32),
                  (np.float32(1) + np.float32(0.5) * np.abs(layers[-1][1])).astype(np.float32))
    if narrow:
        layers = [((np.float32(0.25) * np.abs(W)).astype(np.float32), b) for W, b in layers]      # (live, not saturated)
    c["layers"] = layers
    # M distinct ids per column (the same item twice in a column scores the same twice: undecided by construction)
    c["cand"] = np.stack([rng.choice(N_ITEMS, M, replace=False) for _ in range(num * n)], axis=1).reshape(-1).astype(np.int64)
    return c


def user_half(x, W1, b1):
    """P = x W1[:, :D_user]^T + b1 in float64 (the GPU tests take the product the library forms, in fp32)."""
    x, W1 = np.asarray(x, np.float64), np.asarray(W1, np.float64)
    return x @ W1[:, :x.shape[1]].T + np.asarray(b1, np.float64)


# ---- argument checks of the two entries (no device needed) ----------------------------------------------------------------
def _valid_args(keep, n_linears=3, width=4, dim=4, learner=0):
    from fairrec import _C
    f = (ctypes.c_float * 1024)(*([0.5] * 1024))
    i32 = (ctypes.c_int32 * 16)(*([0] * 16))
    cand = (ctypes.c_int64 * 8)(*range(8))
    out = (ctypes.c_int64 * 4)(*([-7] * 4))
    scores = (ctypes.c_float * 8)(*([-7.0] * 8))
    err = (ctypes.c_uint32 * 1)(0)
    p, q = ctypes.addressof(f), ctypes.addressof(i32)
    table = _C.FrTable(p, p, p, q, q, 16, dim, 0, None)
    optim = _C.FrAdam(p, 1, learner, 1e-3, 0.9, 0.999, 1e-8)
    a = _C.FrDynNegMlpArgs()
    a.item_t, a.item_optim = ctypes.pointer(table), ctypes.pointer(optim)
    a.P, a.W1_item, a.cand = p, p, ctypes.addressof(cand)
    for l in range(n_linears - 1):
        a.W[l], a.bias[l], a.n_out[l] = p, p, (width if l < n_linears - 2 else 1)
    a.ldp, a.ldw1, a.n, a.n1, a.n_linears, a.act, a.num, a.M = width, 2 * dim, 2, width, n_linears, 1, 2, 2
    keep.extend([f, i32, cand, out, scores, err, table, optim])
    return a, table, optim, out, scores, err


def check_refusals():
    """Both entries refuse, with FR_EINVAL and the argument's name in fr_last_error, before any device work: nothing is written."""
    from fairrec import _C
    lib = _C.lib()
    keep = []

    def call(a, out, scores, err, null_out=False, null_err=False):
        e = None if null_err else ctypes.addressof(err)
        rc = (lib.fr_dyn_neg_mlp_select(ctypes.byref(a), None if null_out else ctypes.addressof(out), e, None),
              lib.fr_dyn_neg_mlp_scores(ctypes.byref(a), None if null_out else ctypes.addressof(scores), e, None))
        assert list(out) == [-7] * 4 and list(scores) == [-7.0] * 8 and err[0] == 0
        return rc

    def refused(word, table_fields=None, optim_fields=None, null_out=False, null_err=False, **fields):
        a, table, optim, out, scores, err = _valid_args(keep)
        for name, value in fields.items():
            if "[" in name:
                getattr(a, name[:-3])[int(name[-2])] = value
            else:
                setattr(a, name, value)
        for name, value in (table_fields or {}).items():
            setattr(table, name, value)
        for name, value in (optim_fields or {}).items():
            setattr(optim, name, value)
        for rc in call(a, out, scores, err, null_out, null_err):
            assert rc == -1, (word, fields, rc)
            assert word.encode() in lib.fr_last_error(), (word, lib.fr_last_error())

    a, _, _, out, scores, err = _valid_args(keep)
    a.n = 0                                                     # zero size: success, nothing launched
    assert call(a, out, scores, err) == (0, 0)
    for n_linears in (2, 6):                                    # the limits themselves are served
        a, _, _, out, scores, err = _valid_args(keep, n_linears=n_linears, width=256, dim=256)
        a.n = 0
        assert call(a, out, scores, err) == (0, 0)
    for learner in (1, 2, 3):
        a, _, _, out, scores, err = _valid_args(keep, learner=learner)
        a.n = 0
        assert call(a, out, scores, err) == (0, 0)
    assert lib.fr_dyn_neg_mlp_select(None, ctypes.addressof(out), ctypes.addressof(err), None) == -1
    assert b"null" in lib.fr_last_error()
    refused("n1", n1=0)
    refused("n1", n1=257)                                       # unsupported width
    refused("n_out[0]", **{"n_out[0]": 257})
    refused("n_out[1]", **{"n_out[1]": 2})                      # the last layer has one output
    refused("n_linears", n_linears=1)
    refused("n_linears", n_linears=7)
    for act in (0, 2, 3, 4, 5, -1):
        refused("act", act=act)
    refused("D", table_fields={"dim": 257})
    refused("D", table_fields={"dim": 0})
    refused("null", table_fields={"p": None})
    refused("null", table_fields={"last": None})
    refused("learner", optim_fields={"learner": 4})
    refused("learner", optim_fields={"learner": -1})
    refused("item_t", item_t=None)
    refused("item_optim", item_optim=None)
    refused("P is null", P=None)
    refused("W1_item", W1_item=None)
    refused("W[1]", **{"W[1]": None})
    refused("bias[0]", **{"bias[0]": None})
    refused("cand", cand=None)
    refused("null", null_out=True)
    refused("err_flag", null_err=True)
    refused("ldp", ldp=3)
    refused("ldw1", ldw1=3)
    refused("n ", n=-1)
    refused("num", num=0)
    refused("M ", M=0)

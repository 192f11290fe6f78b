"""numpy float64 restatement of fr_pair_mlp_scores' contract (include/fairrec_hip.h, csrc/pair_mlp.hip), for the tests.

The scorer is MLPLayers([2 D, n1, ..., 1]) with ReLU after every layer, the last included, and a sigmoid on top.  Its first
Linear is split: z1(u, i) = P[u] + Q[i], P = x W1[:, :D]^T + b1, Q = w W1[:, D:]^T.  `layers` is the list of the remaining
(W [n_out, n_in], bias [n_out]); the last has one output.

`upper_bound` carries a rounding bound for the fp32 kernel through the layers, in the manner of tests/mlp_infer_ref.py
(u = 2^-24, gamma_n = n u / (1 - n u), e_in the bound on a layer's input against the float64 one):

  first layer, from P and Q as the entry takes them (fp32 numbers, exact): one add, e_1 = u |P + Q|
  first layer, from the rows and W1 (the host path): P is D products, D adds and the bias add, Q is D products and D adds,
      P + Q one more add: gamma_(D + 2) over |x| |W1u|^T + |w| |W1i|^T + |b1|, whatever the order of the two sums.  The dense
      path sums all 2 D products in one chain of its own order: gamma_(2 D + 2) over the same sum.
  ReLU is 1-Lipschitz and exact.
  each further layer, n_in products, n_in adds and the bias add in any order:
      e_z = |W| e_in + gamma_(n_in + 2) (|W| (|h| + e_in) + |bias|)
  sigmoid: slope <= 1/4, and 4 ulp of the result for expf, the add and the division (what tests/test_case_study_hip.py and
      tests/recommend_ref.py grant epilogue 2): e_s = e_z / 4 + 4 ulp(s), the ulp taken at |s| + e so that the kernel's own
      value is covered.
  every operation may also lose up to 2^-126 to underflow: (n_in + 4) 2^-126 per layer, carried for rigour."""
import numpy as np

from mlp_infer_ref import TINY, U, gamma, ulp32


def relu64(z):
    return np.where(z < 0, 0.0, z)          # keeps a NaN, as the kernel's relu does


def halves64(x, w, W1, b1):
    """(P, Q) in float64 of fp32 rows and parameters."""
    x, w, W1, b1 = (np.asarray(t, np.float64) for t in (x, w, W1, b1))
    D = x.shape[1]
    return x @ W1[:, :D].T + b1, w @ W1[:, D:].T


def upper64(z1, layers):
    """Scores [U, N] from the first layer's pre-activations z1 [U, N, n1]."""
    h = relu64(z1)
    for W, b in layers:
        h = relu64(h @ np.asarray(W, np.float64).T + np.asarray(b, np.float64))
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-h[..., 0]))


def scores64(P, Q, layers):
    """The entry in float64: P [U, n1], Q [N, n1] -> [U, N]."""
    return upper64(np.asarray(P, np.float64)[:, None, :] + np.asarray(Q, np.float64)[None, :, :], layers)


def concat64(x, w, W1, b1, layers):
    """The plain MLP on cat(x[u], w[i]) in float64, no split."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    cat = np.concatenate([np.repeat(x[:, None, :], w.shape[0], 1), np.repeat(w[None, :, :], x.shape[0], 0)], axis=2)
    return upper64(cat @ np.asarray(W1, np.float64).T + np.asarray(b1, np.float64), layers)


def upper_bound(z1, e1, layers):
    """(float64 scores [U, N], rounding bound [U, N]) from z1 [U, N, n1] and the bound e1 on the kernel's z1."""
    h, e = relu64(z1), e1
    for W, b in layers:
        W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
        n_in, aW = W.shape[1], np.abs(W).T
        z = h @ W.T + b
        e = e @ aW + gamma(n_in + 2) * ((np.abs(h) + e) @ aW + np.abs(b)) + (n_in + 4) * TINY
        h = relu64(z)
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-h[..., 0]))
    e = 0.25 * e[..., 0]
    return s, e + 4.0 * ulp32(np.abs(s) + e)


def bound_pq(P, Q, layers):
    """(scores, bound) of the entry on fp32 P and Q."""
    z1 = np.asarray(P, np.float64)[:, None, :] + np.asarray(Q, np.float64)[None, :, :]
    return upper_bound(z1, U * np.abs(z1) + TINY, layers)


def bound_rows(x, w, W1, b1, layers, split=True):
    """(scores, bound) of a whole fp32 path from the rows: the split path (`split`), or a path that sums the first layer's
    2 D products in one chain (the dense path)."""
    x, w, W1, b1 = (np.asarray(t, np.float64) for t in (x, w, W1, b1))
    D = x.shape[1]
    P, Q = halves64(x, w, W1, b1)
    mag = (np.abs(x) @ np.abs(W1[:, :D]).T + np.abs(b1))[:, None, :] + (np.abs(w) @ np.abs(W1[:, D:]).T)[None, :, :]
    n = D + 2 if split else W1.shape[1] + 2
    return upper_bound(P[:, None, :] + Q[None, :, :], gamma(n) * mag + (n + 4) * TINY, layers)


def _fma32(a, b, c):
    """fl32(a * b + c) of fp32 arrays through float64 (the product is exact there; the sum rounds once more, which the
    bound's slack covers)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate32(P, Q, layers):
    """The contract's order in fp32 numpy: one add, ascending fmaf chains from 0, the bias last, relu, the sigmoid as
    1 / (1 + exp(-x))."""
    P, Q = np.asarray(P, np.float32), np.asarray(Q, np.float32)
    z = P[:, None, :] + Q[None, :, :]
    h = np.where(z < 0, np.float32(0), z)
    for W, b in layers:
        W, b = np.asarray(W, np.float32), np.asarray(b, np.float32)
        acc = np.zeros(h.shape[:2] + (W.shape[0],), np.float32)
        for k in range(W.shape[1]):
            acc = _fma32(h[:, :, k:k + 1], W[None, None, :, k], acc)
        z = acc + b
        h = np.where(z < 0, np.float32(0), z)
    with np.errstate(over="ignore"):
        return (np.float32(1) / (np.float32(1) + np.exp(-h[..., 0], dtype=np.float32))).astype(np.float32)


def random_layers(rng, widths, scale=1.0):
    """Upper layers for `widths` = [n1, n2, ..., 1]: weights ~ N(0, scale^2 / n_in), biases ~ N(0, 1/4), fp32."""
    return [((scale * rng.standard_normal((n_out, n_in)) / np.sqrt(n_in)).astype(np.float32),
             (0.5 * rng.standard_normal(n_out)).astype(np.float32)) for n_in, n_out in zip(widths[:-1], widths[1:])]


def pieces_of_module(mlp):
    """(W1, b1, upper layers) of a fairrec `MLPLayers` scorer, as numpy."""
    np_ = lambda t: t.detach().cpu().numpy()
    lins = mlp.linears()
    return np_(lins[0].weight), np_(lins[0].bias), [(np_(lin.weight), np_(lin.bias)) for lin in lins[1:]]

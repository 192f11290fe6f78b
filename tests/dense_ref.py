"""numpy float64 references of the dense-layer and BatchNorm entry points (csrc/mlp.hip, csrc/mlp_glds.hip,
csrc/mlp_stream.hip; include/fairrec_hip.h "dense layers"), the rounding bounds of their fp32 kernels and the input builders
of tests/test_dense_ref.py (CPU) and tests/test_dense_kernels_hip.py (GPU).  No fairrec import: CPU only.

Every reference takes the kernel's float32 inputs and computes in float64.  A derivative of an activation is taken through
the OUTPUT Y that the entry point is handed (csrc/mlp_act.hpp), and the reference is handed the same fp32 Y: no element is
excluded near a kink.

Two input regimes, both asymmetric (a second block with other statistics, so that a transposed or swapped fragment map
cannot pass):
  exact  every operand a small integer held in fp32 (entries -3 .. 3, second block -1 .. 3, keep scale 2, activation none or
         ReLU): every product and every partial sum, in any order, is an integer below 2^24, so a correct kernel EQUALS the
         float64 reference whatever its summation order -- the check that sees one lost, doubled or misplaced term in a
         reduction of any length.  `exact_case` asserts max sum |a| |b| < 2^24 for the three reductions.
  real   the data of tests/test_mlp_hip.py: randn, a second block randn * 0.5 + 0.1, W * 0.3, keep with p = 0.3.

Bounds of the real regime, all derived (u = 2^-24, gamma_n = n u / (1 - n u), both from tests/mlp_infer_ref.py; no constant
here is measured, so there is no MEASURED table):
  product   a sum of R products in any order, plus a bias:  gamma_(R + 2 + pre) (|A| |B| + |b|), R = K, N or M; `pre` counts
            the roundings that form an operand first: PRE[act] for dY act'(Y) (none, relu 0: a factor 0 or 1; leakyrelu 2: the
            constant 0.01f and the product; sigmoid 3: 1 - y, y (1 - y), the product; tanh 2: the fused 1 - y y, the product),
            one for x * scale under a mask.  The split reductions of the weight gradient (slabs summed afterwards) are one more
            summation order of the same M terms.
  activation  Lipschitz constant and own error as mlp_infer_ref.net_bound; the TRAINING sigmoid is 1 / (1 + __expf(-x)):
            the project's form for it, 4 u (o (1 - o)(|z| + 2) + 1) (tests/test_scorer_hip.py::_head_ref).
  fused epilogue  the product is rounded, then multiplied: product bound |act'| + gamma_3 |ref|.
  BatchNorm forward, as the kernels compute it (rc-row chunks, bn_chunk_rows; per chunk a mean and the sum of squared
            deviations from it; a fold over the chunks), carried operation by operation in `bn_fwd`:
              chunk mean          e_c    = gamma_(n_c + 1) mean_chunk |z|      (n_c rows; one row: exact)
              mean (the fold)     e_mean = sum_c n_c e_c / M + gamma_(chunks + 3) mean |z|      (M = 1: exact)
              sum of squares      the fold's identity  sum_c [S_c + n_c (a_c - b)^2] = M var + M (b - mean)^2 + 2 sum_c n_c
                                  (a_c - b) eps_c  holds for the ROUNDED chunk means a_c = m_c + eps_c and folded mean b:
                                  d1 = M e_mean^2 + 2 M e_c (sigma + e_mean), then gamma_(rc + chunks + 8) on the sum of its
                                  non-negative terms
              1 / sqrtf(var + eps)  IEEE division, addition, square root, division (no fast-math flag in the build)
              xhat = (z - mean) invstd, fmaf(gamma, xhat, beta), activation
            so the bound on Y scales with (|z| + |mean|) / sigma and a column whose mean is far from zero stays covered.
            `e_in`: a bound on the kernel's INPUT against the reference's (the product in front of fr_linear_fwd_bnstats),
            carried through: mean by its column mean, sigma by its column maximum (the standard deviation is 1-Lipschitz in
            the sup norm).
  BatchNorm backward  sums of M terms gamma_(M + pre + 3), then dZ = isg (dA - a1 - xhat a2) term by term (`bn_bwd`).
A bound cannot prove that every row is counted: `planted` builds Z with ONE entry 2^20 per column, the row walking over the
edges of the chunks, for which running_mean = 2^20 / M, invstd and dbeta are known to a few ulp / exactly."""
from types import SimpleNamespace

import numpy as np

from mlp_infer_ref import ACT_LIP, ACT_ULPS, TINY, U, act64, gamma, ulp32

PRE = {0: 0, 1: 0, 2: 2, 3: 3, 4: 2}
EXACT_LIMIT = 2.0 ** 24
PLANT = 2.0 ** 20


def f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def dact64(Y, act):
    """act'(z) through the output Y = act(z)"""
    Y = f64(Y)
    if act == 1:
        return (Y > 0).astype(np.float64)
    if act == 2:
        return np.where(Y > 0, 1.0, 0.01)
    if act == 3:
        return Y * (1.0 - Y)
    if act == 4:
        return 1.0 - Y * Y
    return np.ones_like(Y)


def cat(x0, x1=None):
    return f64(x0) if x1 is None else np.concatenate([f64(x0), f64(x1)], axis=1)


def dropped(X, keep, scale):
    """X o keep * scale (keep: bytes, 0 = dropped; scale as the float32 the entry point receives)"""
    return X if keep is None else X * ((np.asarray(keep) != 0) * float(np.float32(scale)))


def product(A, B, bias=None, pre=0):
    """(A B^T + bias, bound): A [M, R], B [N, R]"""
    A, B = f64(A), f64(B)
    R = A.shape[1]
    z, ab = A @ B.T, np.abs(A) @ np.abs(B).T
    if bias is not None:
        z, ab = z + f64(bias), ab + np.abs(f64(bias))
    return z, gamma(R + 2 + pre) * ab + (R + 4) * TINY


def act_out(z, ez, act):
    """(act(z), bound) of the kernel's activation of a value within ez of z"""
    out = act64(z, act)
    if act == 3:
        return out, ACT_LIP[3] * ez + 4 * U * (out * (1 - out) * (np.abs(z) + 2) + 1)
    e = ACT_LIP[act] * ez
    return out, e + ACT_ULPS[act] * ulp32(np.abs(out) + e)


def linear_fwd(x0, x1, keep, scale, W, bias, act):
    """Y = act(([x0 | x1] o keep * scale) W^T + bias) and its bound"""
    z, ez = product(dropped(cat(x0, x1), keep, scale), W, bias, pre=0 if keep is None else 1)
    return act_out(z, ez, act)


def grad_at_z(dY, Y, act):
    return f64(dY) * dact64(Y, act)


def linear_bwd_input(dY, Y, act, W, keep, scale):
    """dX = ((dY o act'(Y)) W) o keep * scale: the literal transpose of linear_fwd"""
    dX, e = product(grad_at_z(dY, Y, act), f64(W).T, pre=PRE[act] + (0 if keep is None else 1))
    return dropped(dX, keep, scale), dropped(e, keep, scale)


def linear_bwd_weight(dY, Y, act, x0, x1, keep, scale):
    """dW = g^T (X o keep * scale), db = column sums of g, g = dY o act'(Y); (dW, e_dW, db, e_db)"""
    g = grad_at_z(dY, Y, act)
    M = g.shape[0]
    dW, e = product(g.T, dropped(cat(x0, x1), keep, scale).T, pre=PRE[act] + (0 if keep is None else 1))
    return dW, e, g.sum(0), gamma(M + PRE[act] + 1) * np.abs(g).sum(0) + (M + 4) * TINY


def bwd_input_act(dY, W, Yin, act):
    """(dY W) o act'(Yin): fr_linear_bwd_input_act -- the product is rounded, then multiplied"""
    P, e = product(dY, f64(W).T)
    s = dact64(Yin, act)
    return P * s, e * np.abs(s) + gamma(3) * np.abs(P * s)


def bwd_input_relu(dY, W, Xd, scale):
    """(dY W) o scale o [Xd > 0]: fr_linear_bwd_input_relu"""
    P, e = product(dY, f64(W).T)
    s = (f64(Xd) > 0) * float(np.float32(scale))
    return P * s, e * s + gamma(3) * np.abs(P * s)


def n1_bwd(dY, Y, act, X, W, relu_scale=0.0):
    """fr_linear_n1_bwd (N == 1): dW [K], db, dX [M, K] (on through a dropped ReLU when relu_scale > 0), each with its bound"""
    dz = grad_at_z(dY, Y, act).reshape(-1)
    X, W = f64(X), f64(W).reshape(-1)
    M = X.shape[0]
    r = SimpleNamespace()
    r.dW, r.e_dW = dz @ X, gamma(M + 2 + PRE[act]) * (np.abs(dz) @ np.abs(X)) + (M + 4) * TINY
    r.db, r.e_db = dz.sum(), gamma(M + 1 + PRE[act]) * np.abs(dz).sum() + (M + 4) * TINY
    r.dX = dz[:, None] * W[None, :]
    if relu_scale > 0:
        r.dX = r.dX * ((X > 0) * float(np.float32(relu_scale)))
    r.e_dX = gamma(PRE[act] + 3) * np.abs(r.dX) + 4 * TINY
    return r


def parts_sum(part):
    """fr_parts_sum and the slab sum: out[i] = sum_p part[p, i] in a fixed order; (sum, bound)"""
    part = f64(part)
    return part.sum(0), gamma(part.shape[0]) * np.abs(part).sum(0)


# ---- BatchNorm ---------------------------------------------------------------------------------------------------------------

def bn_chunk_rows(M):
    """rows of a statistics chunk (csrc/mlp.hip: at least 32, at most 1024 chunks)"""
    rc = 32
    while (M + rc - 1) // rc > 1024:
        rc *= 2
    return rc


def bn_running(old, momentum, value):
    """(1 - momentum) old + momentum value with the float32 momentum (mlp_bn_math.hpp::bn_running)"""
    m = float(np.float32(momentum))
    return (1.0 - m) * f64(old) + m * value


def bn_fwd(Z, gam, beta, eps, momentum, rmean, rvar, act, e_in=None):
    """Training-mode BatchNorm1d of Z [M, N]: two-pass mean and variance, xhat, invstd, Y = act(gamma xhat + beta), the running
    statistics (unbiased variance; M == 1: the biased one) -- and the bound of each (module docstring)."""
    Z, gam, beta = f64(Z), f64(gam), f64(beta)
    M, N = Z.shape
    eps, mom = float(np.float32(eps)), float(np.float32(momentum))
    r = SimpleNamespace()
    r.mean = Z.mean(0)
    d = Z - r.mean
    r.m2 = (d * d).sum(0)
    r.var = r.m2 / M
    sd = np.sqrt(r.var + eps)
    r.invstd = 1.0 / sd
    r.xhat = d * r.invstd
    pre = gam * r.xhat + beta
    unb = r.m2 / (M - 1) if M > 1 else r.var
    r.rmean, r.rvar = bn_running(rmean, momentum, r.mean), bn_running(rvar, momentum, unb)

    ein = np.zeros_like(Z) if e_in is None else f64(e_in) * np.ones_like(Z)
    rc = bn_chunk_rows(M)
    starts = np.arange(0, M, rc)
    chunks = len(starts)
    counts = np.minimum(M, starts + rc) - starts
    absz = np.abs(Z) + ein
    # (a chunk of ONE row -- M == 1, or a last chunk of one row -- has an exact mean: a sum of one term, a division by 1)
    e_cs = gamma(np.where(counts > 1, counts + 1, 0))[:, None] * (np.add.reduceat(absz, starts, axis=0) / counts[:, None])
    e_c = e_cs.max(0)
    # the kernel's arithmetic on its own input: the chunk means' errors, then the fold (M == 1: 1 * z + 0, / 1 -- exact)
    e_mean_k = (counts[:, None] * e_cs).sum(0) / M + (gamma(chunks + 3) * absz.mean(0) if M > 1 else 0.0)
    e_mean = e_mean_k + ein.mean(0)
    e_sig_in = ein.max(0)
    sig_k = np.sqrt(r.var) + e_sig_in
    d1 = M * e_mean_k ** 2 + 2 * M * e_c * (sig_k + e_mean_k)
    e_m2 = gamma(rc + chunks + 8) * (M * sig_k ** 2 + d1) + d1 + (M + 8) * TINY
    e_v = e_m2 / M + gamma(2) * (sig_k ** 2 + eps)
    ve_lo = np.maximum(sd - e_sig_in, 0.0) ** 2 - e_v
    assert (ve_lo > 0).all(), "bn_fwd: the variance is lost in its own bound"
    e_sd = e_sig_in + e_v / (2 * np.sqrt(ve_lo)) + U * sd
    r.e_invstd = e_sd / (sd * (sd - e_sd)) + U * r.invstd
    dd = np.abs(d) + e_mean + ein
    r.e_xhat = r.invstd * (e_mean + ein + gamma(2) * dd) + dd * r.e_invstd + 4 * TINY
    e_pre = np.abs(gam) * r.e_xhat
    e_pre = e_pre + ulp32(np.abs(pre) + e_pre)
    r.Y, r.e_Y = act_out(pre, e_pre, act)
    den = M - 1 if M > 1 else M
    r.e_rmean = mom * e_mean + gamma(3) * (np.abs(mom * r.mean) + np.abs((1 - mom) * f64(rmean)))
    r.e_rvar = mom * (e_m2 + M * e_sig_in * (2 * np.sqrt(r.var) + e_sig_in)) / den \
        + gamma(4) * (np.abs(mom * unb) + np.abs((1 - mom) * f64(rvar)))
    return r


def bn_bwd(dY, Y, act, xhat, invstd, gam, e_in=None):
    """dZ = invstd gamma (dA - mean(dA) - xhat mean(dA xhat)), dgamma = sum dA xhat, dbeta = sum dA, dA = dY o act'(Y) through the
    given Y, xhat and invstd; `e_in`: a bound on the kernel's dY against the reference's."""
    dY, xhat = f64(dY), f64(xhat)
    M = dY.shape[0]
    s = dact64(Y, act)
    dA = dY * s
    eA = 0.0 * dA if e_in is None else f64(e_in) * np.abs(s)
    aA = np.abs(dA) + eA
    r = SimpleNamespace()
    r.dbeta, r.dgamma = dA.sum(0), (dA * xhat).sum(0)
    r.e_dbeta = gamma(M + PRE[act] + 2) * aA.sum(0) + eA.sum(0) + (M + 4) * TINY
    r.e_dgamma = gamma(M + PRE[act] + 3) * (aA * np.abs(xhat)).sum(0) + (eA * np.abs(xhat)).sum(0) + (M + 4) * TINY
    a1, a2 = r.dbeta / M, r.dgamma / M
    e_a1, e_a2 = r.e_dbeta / M + U * np.abs(a1), r.e_dgamma / M + U * np.abs(a2)
    isg = f64(invstd) * f64(gam)
    r.dZ = isg * (dA - a1 - xhat * a2)
    r.e_dZ = np.abs(isg) * (eA + e_a1 + np.abs(xhat) * e_a2) \
        + gamma(PRE[act] + 5) * np.abs(isg) * (aA + np.abs(a1) + e_a1 + np.abs(xhat) * (np.abs(a2) + e_a2)) + 8 * TINY
    return r


# ---- builders ----------------------------------------------------------------------------------------------------------------

def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def exact_case(M, k0, k1, N, mask=False, seed=0):
    """integers held in fp32; asserts that no reduction of the case can leave the integers fp32 holds exactly"""
    rng = _rng(1, M, k0, k1, N, int(mask), seed)
    c = SimpleNamespace(M=M, k0=k0, k1=k1, N=N, K=k0 + k1, regime="exact")
    ints = lambda lo, hi, *shape: rng.integers(lo, hi + 1, shape).astype(np.float32)
    c.x0 = ints(-3, 3, M, k0)
    c.x1 = ints(-1, 3, M, k1) if k1 else None
    c.W, c.b, c.dY = ints(-3, 3, N, c.K), ints(-3, 3, N), ints(-3, 2, M, N)
    c.keep = (rng.random((M, c.K)) >= 0.5).astype(np.uint8) if mask else None
    c.scale = 2.0 if mask else 1.0
    assert_exact(3 * c.scale, 3, max(c.K, N, M), 3)
    return c


def assert_exact(amax, bmax, R, bias=0.0):
    """max sum |a| |b| (+ |bias|) of a reduction of length R is below 2^24"""
    worst = float(amax) * float(bmax) * R + float(bias)
    assert worst < EXACT_LIMIT, f"exact regime: a sum may reach {worst} >= 2^24"


def real_case(M, k0, k1, N, mask=False, seed=0):
    rng = _rng(2, M, k0, k1, N, int(mask), seed)
    c = SimpleNamespace(M=M, k0=k0, k1=k1, N=N, K=k0 + k1, regime="real")
    nrm = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    c.x0 = nrm(M, k0)
    c.x1 = (nrm(M, k1) * np.float32(0.5) + np.float32(0.1)) if k1 else None
    c.W, c.b, c.dY = nrm(N, c.K) * np.float32(0.3), nrm(N), nrm(M, N)
    c.keep = (rng.random((M, c.K)) >= 0.3).astype(np.uint8) if mask else None
    c.scale = 1.0 / 0.7 if mask else 1.0
    return c


def case(regime, *a, **k):
    return exact_case(*a, **k) if regime == "exact" else real_case(*a, **k)


def bn_case(M, N, seed=0):
    """test_batchnorm_forward_and_backward_match_torch's data: column scales 0.1 .. 3.1, column means N(0, 50^2)"""
    rng = _rng(3, M, N, seed)
    c = SimpleNamespace(M=M, N=N)
    f = np.float32
    c.Z = (rng.standard_normal((M, N)) * (rng.random(N) * 3 + 0.1) + rng.standard_normal(N) * 50).astype(f)
    c.gamma = ((rng.random(N) + 0.5) * np.where(rng.random(N) < 0.3, -1.0, 1.0)).astype(f)
    c.beta, c.dY = rng.standard_normal(N).astype(f), rng.standard_normal((M, N)).astype(f)
    c.rmean, c.rvar = rng.standard_normal(N).astype(f), (rng.random(N) + 0.5).astype(f)
    c.eps, c.momentum = 1e-5, 0.1
    return c


def planted_rows(M, seed=0):
    """the rows a planted entry walks over: 0-3, 30-33, M - 2, M - 1 and a seeded sample"""
    rows = [m for m in (0, 1, 2, 3, 30, 31, 32, 33, M - 2, M - 1) if 0 <= m < M]
    rows += [int(m) for m in _rng(4, M, seed).integers(0, M, 6)]
    return list(dict.fromkeys(rows))


def planted(M, N, seed=0):
    """Z [M, N] zero except Z[row(n), n] = 2^20; returns (Z, row of each column)"""
    rows = planted_rows(M, seed)
    at = np.array([rows[n % len(rows)] for n in range(N)])
    Z = np.zeros((M, N), np.float32)
    Z[at, np.arange(N)] = PLANT
    return Z, at

"""CPU: the float64 references and bounds of tests/dense_ref.py, checked without a kernel.

  * each reference equals float64 torch.autograd of the literal expression (BatchNorm: torch.nn.functional.batch_norm in
    double), the derivative through the output included;
  * a float32 restatement of each formula on the CPU -- torch's fp32 products, the kernels' chunked BatchNorm written out in
    numpy float32 -- stays inside its bound at the shapes the GPU module uses (its error over the bound is printed and is at
    most 1): a bound that a correct fp32 evaluation breaks is wrong, whatever a kernel does;
  * the exact-regime builders are bit-exact for fp32 torch at the longest reductions used (M = 65537, K = 1024);
  * every constant of a bound is derived (dense_ref's docstring): there is no measured table to assert."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dense_ref as D

ACTS = {0: lambda x: x, 1: torch.relu, 2: lambda x: F.leaky_relu(x, 0.01), 3: torch.sigmoid, 4: torch.tanh}
t64 = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.float64))
t32 = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.float32))


def _tanh_d(y):
    """fmaf(-y, y, 1) as csrc/mlp_act.hpp writes it: ONE rounding of 1 - y y"""
    if isinstance(y, torch.Tensor):
        return (1.0 - y.double() * y.double()).float()
    return (1.0 - y.astype(np.float64) ** 2).astype(np.float32)


def _ratio(what, got, ref, bound):
    got, ref, bound = (np.asarray(x, np.float64) for x in (got, ref, bound))
    assert np.isfinite(got).all(), what
    r = float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max()) if got.size else 0.0
    print(f"{what}: fp32 restatement error / bound {r:.3g}")
    assert r <= 1.0, (what, r)
    return r


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, what
    assert np.abs(a - b).max() <= 1e-11 * max(1.0, np.abs(b).max()), (what, np.abs(a - b).max())


# ---- the references are the literal expressions --------------------------------------------------------------------------------

@pytest.mark.parametrize("act", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("mask", [False, True])
def test_linear_references_equal_float64_autograd(act, mask):
    c = D.real_case(37, 12, 7, 9, mask=mask, seed=act)
    X = torch.cat([t64(c.x0), t64(c.x1)], 1).requires_grad_()
    W, b = t64(c.W).requires_grad_(), t64(c.b).requires_grad_()
    Xe = X * (t64(c.keep != 0) * float(np.float32(c.scale))) if mask else X
    Y = ACTS[act](F.linear(Xe, W, b))
    Y.backward(t64(c.dY))
    Y64 = Y.detach().numpy()
    ref, _ = D.linear_fwd(c.x0, c.x1, c.keep, c.scale, c.W, c.b, act)
    _close(ref, Y64, "forward")
    _close(D.linear_fwd(c.x0, c.x1, c.keep, c.scale, c.W, None, act)[0],
           ACTS[act](F.linear(Xe, W)).detach().numpy(), "forward without bias")
    _close(D.linear_bwd_input(c.dY, Y64, act, c.W, c.keep, c.scale)[0], X.grad.numpy(), "input gradient")
    dW, _, db, _ = D.linear_bwd_weight(c.dY, Y64, act, c.x0, c.x1, c.keep, c.scale)
    _close(dW, W.grad.numpy(), "weight gradient")
    _close(db, b.grad.numpy(), "bias gradient")


@pytest.mark.parametrize("act", [1, 2, 3, 4])
def test_fused_input_gradients_equal_float64_autograd(act):
    rng = np.random.default_rng(act)
    z = torch.from_numpy(rng.standard_normal((21, 10))).requires_grad_()
    W, dY = rng.standard_normal((6, 10)), rng.standard_normal((21, 6))
    Yin = ACTS[act](z)
    (Yin @ t64(W).t()).backward(t64(dY))
    _close(D.bwd_input_act(dY, W, Yin.detach().numpy(), act)[0], z.grad.numpy(), "through the activation below")
    if act == 1:
        z.grad = None
        keep = (rng.random((21, 10)) >= 0.5) * 2.0
        Xd = torch.relu(z) * t64(keep)
        (Xd @ t64(W).t()).backward(t64(dY))
        _close(D.bwd_input_relu(dY, W, Xd.detach().numpy(), 2.0)[0], z.grad.numpy(), "through a dropped relu")


@pytest.mark.parametrize("act", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("relu_scale", [0.0, 2.0])
def test_one_output_pair_equals_float64_autograd(act, relu_scale):
    rng = np.random.default_rng(act + 10)
    z = torch.from_numpy(rng.standard_normal((19, 8))).requires_grad_()
    keep = (rng.random((19, 8)) >= 0.5) * relu_scale
    X = torch.relu(z) * t64(keep) if relu_scale else z
    W, b = t64(rng.standard_normal((1, 8))).requires_grad_(), t64(rng.standard_normal(1)).requires_grad_()
    dY = rng.standard_normal((19, 1))
    Y = ACTS[act](F.linear(X, W, b))
    Y.backward(t64(dY))
    r = D.n1_bwd(dY, Y.detach().numpy(), act, X.detach().numpy(), W.detach().numpy(), relu_scale)
    _close(r.dW, W.grad.numpy().reshape(-1), "dW")
    _close(r.db, b.grad.numpy().reshape(()), "db")
    _close(r.dX, z.grad.numpy(), "dX")


@pytest.mark.parametrize("act", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("M,N", [(2, 5), (33, 4), (257, 7)])
def test_batchnorm_reference_equals_torch_in_double(M, N, act):
    c = D.bn_case(M, N, seed=act)
    Z = t64(c.Z).requires_grad_()
    g, b = t64(c.gamma).requires_grad_(), t64(c.beta).requires_grad_()
    rm, rv = t64(c.rmean).clone(), t64(c.rvar).clone()
    eps, mom = float(np.float32(c.eps)), float(np.float32(c.momentum))
    Y = ACTS[act](F.batch_norm(Z, rm, rv, g, b, True, mom, eps))
    Y.backward(t64(c.dY))
    r = D.bn_fwd(c.Z, c.gamma, c.beta, c.eps, c.momentum, c.rmean, c.rvar, act)
    _close(r.Y, Y.detach().numpy(), "Y")
    _close(r.rmean, rm.numpy(), "running_mean")
    _close(r.rvar, rv.numpy(), "running_var")
    _close(r.invstd, 1.0 / np.sqrt(np.asarray(c.Z, np.float64).var(0) + eps), "invstd")
    q = D.bn_bwd(c.dY, r.Y, act, r.xhat, r.invstd, c.gamma)
    _close(q.dZ, Z.grad.numpy(), "dZ")
    _close(q.dgamma, g.grad.numpy(), "dgamma")
    _close(q.dbeta, b.grad.numpy(), "dbeta")


def test_batchnorm_reference_of_one_row_takes_the_biased_variance():
    c = D.bn_case(1, 5)
    r = D.bn_fwd(c.Z, c.gamma, c.beta, c.eps, c.momentum, c.rmean, c.rvar, 0)
    assert (r.xhat == 0).all() and (r.var == 0).all()
    _close(r.rvar, 0.9 * np.asarray(c.rvar, np.float64) * (1 - float(np.float32(0.1))) / 0.9, "running_var")
    _close(r.Y, np.asarray(c.beta, np.float64)[None, :], "Y")


def test_parts_sum_and_planted_rows():
    part = np.random.default_rng(0).standard_normal((5, 65)).astype(np.float32)
    s, e = D.parts_sum(part)
    _close(s, part.astype(np.float64).sum(0), "parts_sum")
    _ratio("parts_sum", part.sum(0, dtype=np.float32), s, e)
    for M in (1, 2, 31, 33, 257, 8193):
        Z, at = D.planted(M, 100)
        assert (np.count_nonzero(Z, axis=0) == 1).all() and (Z[at, np.arange(100)] == D.PLANT).all()
        want = [m for m in (0, 1, 2, 3, 30, 31, 32, 33, M - 2, M - 1) if 0 <= m < M]
        assert set(want) <= set(at.tolist())
        r = D.bn_fwd(Z, np.ones(100), np.zeros(100), 1e-5, 1.0, np.zeros(100), np.ones(100), 0)
        _close(r.rmean, np.full(100, D.PLANT / M), "planted running_mean")


# ---- an fp32 restatement stays inside each bound ----------------------------------------------------------------------------

FWD_SHAPES = [(1, 32, 0, 8), (33, 96, 32, 65), (65, 36, 0, 7), (97, 256, 0, 96), (64, 37, 11, 33), (17, 512, 0, 1),
              (4097, 64, 32, 40), (8129, 64, 0, 200), (32769, 128, 0, 128)]


@pytest.mark.parametrize("M,k0,k1,N", FWD_SHAPES)
def test_fp32_products_stay_inside_their_bounds(M, k0, k1, N):
    for mask in (False, True):
        c = D.real_case(M, k0, k1, N, mask=mask)
        X32 = torch.cat([t32(c.x0), t32(c.x1)], 1) if k1 else t32(c.x0)
        if mask:
            X32 = X32 * (t32(c.keep != 0) * float(np.float32(c.scale)))
        for act in (0, 1, 2, 3, 4):
            Y32 = ACTS[act](F.linear(X32, t32(c.W), t32(c.b))).numpy()
            ref, e = D.linear_fwd(c.x0, c.x1, c.keep, c.scale, c.W, c.b, act)
            _ratio(f"forward act={act} mask={mask}", Y32, ref, e)
            s32 = {0: torch.ones_like, 1: lambda y: (y > 0).float(), 2: lambda y: torch.where(y > 0, 1.0, 0.01).float(),
                   3: lambda y: y * (1 - y), 4: _tanh_d}[act](torch.from_numpy(Y32))
            g32 = t32(c.dY) * s32
            dX32 = g32 @ t32(c.W)
            if mask:
                dX32 = dX32 * (t32(c.keep != 0) * float(np.float32(c.scale)))
            ref, e = D.linear_bwd_input(c.dY, Y32, act, c.W, c.keep, c.scale)
            _ratio(f"input gradient act={act} mask={mask}", dX32.numpy(), ref, e)
            dW, e_dW, db, e_db = D.linear_bwd_weight(c.dY, Y32, act, c.x0, c.x1, c.keep, c.scale)
            _ratio(f"weight gradient act={act} mask={mask}", (g32.t() @ X32).numpy(), dW, e_dW)
            _ratio(f"bias gradient act={act} mask={mask}", g32.sum(0).numpy(), db, e_db)
            if act and not mask and k1 == 0:
                Yin = ACTS[act](t32(c.x0)).numpy()
                P32 = t32(c.dY) @ t32(c.W)
                d32 = {1: lambda y: (y > 0).float(), 2: lambda y: torch.where(y > 0, 1.0, 0.01).float(),
                       3: lambda y: y * (1 - y), 4: _tanh_d}[act](torch.from_numpy(Yin))
                ref, e = D.bwd_input_act(c.dY, c.W, Yin, act)
                _ratio(f"fused input gradient act={act}", (P32 * d32).numpy(), ref, e)
                if act == 1:
                    Xd = Yin * (np.asarray(D.real_case(M, k0, 0, N, mask=True).keep != 0, np.float32) * np.float32(1 / 0.6))
                    ref, e = D.bwd_input_relu(c.dY, c.W, Xd, 1 / 0.6)
                    _ratio("fused dropped-relu input gradient", (P32 * (t32(Xd) > 0) * float(np.float32(1 / 0.6))).numpy(), ref, e)


@pytest.mark.parametrize("M,K", [(1, 64), (129, 512), (4097, 64)])
def test_fp32_one_output_pair_stays_inside_its_bounds(M, K):
    for act in (0, 1, 2, 3, 4):
        for rs in (0.0, 2.0):
            c = D.real_case(M, K, 0, 1, seed=act)
            X = np.maximum(c.x0, 0) * ((c.x0 * 7 % 1 > 0.5) * np.float32(rs)) if rs else c.x0
            Y32 = ACTS[act](F.linear(t32(X), t32(c.W), t32(c.b))).numpy()
            r = D.n1_bwd(c.dY, Y32, act, X, c.W, rs)
            s32 = np.asarray(D.dact64(Y32, act), np.float32) if act < 3 else (Y32 * (1 - Y32) if act == 3 else _tanh_d(Y32))
            dz = (c.dY * s32).reshape(-1)
            _ratio(f"n1 dW act={act}", t32(dz) @ t32(X), r.dW, r.e_dW)
            _ratio(f"n1 db act={act}", dz.sum(dtype=np.float32), r.db, r.e_db)
            dX = dz[:, None] * c.W.reshape(1, -1)
            if rs:
                dX = np.where(X > 0, dX * np.float32(rs), np.float32(0))
            _ratio(f"n1 dX act={act}", dX, r.dX, r.e_dX)


def _bn_fwd_f32(Z, gam, beta, eps, mom, rmean, rvar, act):
    """the kernels' forward pass in numpy float32: chunk means and sums of squared deviations, the two-pass fold, the apply"""
    f = np.float32
    M, N = Z.shape
    rc = D.bn_chunk_rows(M)
    starts = np.arange(0, M, rc)
    cnt = (np.minimum(M, starts + rc) - starts).astype(f)[:, None]
    mean_c = np.add.reduceat(Z, starts, axis=0, dtype=f) / cnt
    dev = Z - np.repeat(mean_c, cnt.reshape(-1).astype(int), axis=0)
    m2_c = np.add.reduceat(dev * dev, starts, axis=0, dtype=f)
    mean = (cnt * mean_c).sum(0, dtype=f) / f(M)
    dm = mean_c - mean
    m2 = (cnt * dm * dm + m2_c).sum(0, dtype=f)
    var = m2 / f(M)
    invstd = f(1) / np.sqrt(var + f(eps))
    xhat = (Z - mean) * invstd
    Y = ACTS[act](torch.from_numpy(gam * xhat + beta)).numpy()
    unb = m2 / f(M - 1) if M > 1 else var
    return Y, xhat, invstd, f(mom) * mean + (f(1) - f(mom)) * rmean, f(mom) * unb + (f(1) - f(mom)) * rvar


@pytest.mark.parametrize("M", [1, 2, 31, 33, 257, 8193, 32769])
def test_fp32_batchnorm_stays_inside_its_bounds(M):
    for N in (1, 4, 65):
        for act in (0, 1, 2, 3, 4):
            c = D.bn_case(M, N, seed=act)
            r = D.bn_fwd(c.Z, c.gamma, c.beta, c.eps, c.momentum, c.rmean, c.rvar, act)
            Y, xhat, invstd, rm, rv = _bn_fwd_f32(c.Z, c.gamma, c.beta, c.eps, c.momentum, c.rmean, c.rvar, act)
            tag = f"bn M={M} N={N} act={act}"
            _ratio(tag + " invstd", invstd, r.invstd, r.e_invstd)
            _ratio(tag + " xhat", xhat, r.xhat, r.e_xhat)
            _ratio(tag + " Y", Y, r.Y, r.e_Y)
            _ratio(tag + " running_mean", rm, r.rmean, r.e_rmean)
            _ratio(tag + " running_var", rv, r.rvar, r.e_rvar)
            q = D.bn_bwd(c.dY, Y, act, xhat, invstd, c.gamma)
            f = np.float32
            s = np.asarray(D.dact64(Y, act), f) if act < 3 else (Y * (1 - Y) if act == 3 else _tanh_d(Y))
            dA = c.dY * s
            s1, s2 = dA.sum(0, dtype=f), (dA * xhat).sum(0, dtype=f)
            dZ = (invstd * c.gamma) * (dA - s1 / f(M) - xhat * (s2 / f(M)))
            _ratio(tag + " dbeta", s1, q.dbeta, q.e_dbeta)
            _ratio(tag + " dgamma", s2, q.dgamma, q.e_dgamma)
            _ratio(tag + " dZ", dZ, q.dZ, q.e_dZ)


def test_batchnorm_bound_carries_an_input_error_through():
    """e_in: the statistics of Z + delta (|delta| <= e_in) stay inside the bound taken at Z"""
    rng = np.random.default_rng(5)
    c = D.bn_case(257, 9)
    e_in = np.abs(rng.standard_normal((257, 9))) * 1e-4
    Zp = (c.Z.astype(np.float64) + e_in * rng.choice([-1.0, 1.0], (257, 9))).astype(np.float32)
    r = D.bn_fwd(c.Z, c.gamma, c.beta, c.eps, c.momentum, c.rmean, c.rvar, 2, e_in=e_in + np.spacing(np.abs(c.Z)))
    Y, xhat, invstd, rm, rv = _bn_fwd_f32(Zp, c.gamma, c.beta, c.eps, c.momentum, c.rmean, c.rvar, 2)
    for what, got, ref, e in (("Y", Y, r.Y, r.e_Y), ("xhat", xhat, r.xhat, r.e_xhat), ("invstd", invstd, r.invstd, r.e_invstd),
                              ("running_mean", rm, r.rmean, r.e_rmean), ("running_var", rv, r.rvar, r.e_rvar)):
        assert _ratio("perturbed " + what, got, ref, e) > 1e-3 or what.startswith("running")


# ---- the exact regime is exact ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,k0,k1,N,mask", [(65537, 64, 0, 64, False), (65537, 128, 0, 128, True), (33, 992, 32, 65, True),
                                            (129, 1024, 0, 8, False)])
def test_exact_regime_is_bit_exact_in_fp32(M, k0, k1, N, mask):
    c = D.exact_case(M, k0, k1, N, mask=mask)
    X32 = torch.cat([t32(c.x0), t32(c.x1)], 1) if k1 else t32(c.x0)
    if mask:
        X32 = X32 * (t32(c.keep != 0) * 2.0)
    for act in (0, 1):
        Y32 = ACTS[act](F.linear(X32, t32(c.W), t32(c.b))).numpy()
        ref, _ = D.linear_fwd(c.x0, c.x1, c.keep, c.scale, c.W, c.b, act)
        assert (Y32.astype(np.float64) == ref).all()
        g32 = t32(c.dY) * torch.from_numpy(np.asarray(D.dact64(Y32, act), np.float32))
        dX = g32 @ t32(c.W) * (t32(c.keep != 0) * 2.0 if mask else 1.0)
        assert (dX.numpy().astype(np.float64) == D.linear_bwd_input(c.dY, Y32, act, c.W, c.keep, c.scale)[0]).all()
        dW, _, db, _ = D.linear_bwd_weight(c.dY, Y32, act, c.x0, c.x1, c.keep, c.scale)
        assert ((g32.t() @ X32).numpy().astype(np.float64) == dW).all() and (g32.sum(0).numpy().astype(np.float64) == db).all()
        assert np.abs(dW).max() < D.EXACT_LIMIT and np.abs(ref).max() < D.EXACT_LIMIT


def test_exact_builder_refuses_a_reduction_that_could_round():
    with pytest.raises(AssertionError):
        D.assert_exact(6, 3, 1 << 20)
    D.assert_exact(6, 3, 65537, 3)

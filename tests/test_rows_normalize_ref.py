"""CPU: the float64 restatement of fr_rows_l2_normalize (tests/rows_normalize_ref.py) is torch's `normalize`, the dot product of
two normalised rows is torch's cosine similarity, and the entry refuses bad arguments before it touches a device."""
import numpy as np
import torch

import rows_normalize_ref as N


def _rows(rng, M, D):
    x = rng.standard_normal((M, D)).astype(np.float32)
    x[1 % M] *= 1e-12          # norm below eps: the quotient is by eps
    x[2 % M] *= 1e12
    if M > 3:
        x[3] = 0.0
    return x


def test_restatement_is_torch_normalize():
    rng = np.random.default_rng(0)
    for D in (1, 2, 63, 64, 65, 256):
        x = _rows(rng, 9, D)
        y, n = N.normalize64(x, eps=1e-8)
        want = torch.nn.functional.normalize(torch.from_numpy(x).double(), dim=1, eps=1e-8).numpy()
        np.testing.assert_allclose(y, want, rtol=1e-14, atol=0.0)
        np.testing.assert_allclose(n, np.linalg.norm(x.astype(np.float64), axis=1), rtol=1e-14, atol=0.0)
        assert np.all(y[3] == 0.0)


def test_dot_of_unit_rows_is_the_cosine():
    rng = np.random.default_rng(1)
    for D in (1, 8, 65, 256):
        a, b = _rows(rng, 9, D), _rows(rng, 9, D)[::-1].copy()
        ya, _ = N.normalize64(a, eps=1e-8)
        yb, _ = N.normalize64(b, eps=1e-8)
        want = torch.nn.functional.cosine_similarity(torch.from_numpy(a).double(), torch.from_numpy(b).double(), dim=1, eps=1e-8)
        assert np.max(np.abs((ya * yb).sum(1) - want.numpy())) <= 1e-12


def test_special_rows():
    x = np.array([[1.0, np.nan, 2.0], [3.0, np.inf, -4.0], [1e20, 1e20, -1e20], [0.0, 0.0, 0.0]], dtype=np.float32)
    y, n = N.normalize64(x, eps=1e-8)
    assert np.isnan(n[0]) and np.isnan(y[0, 1]) and y[0, 0] == 1.0 / 1e-8 and y[0, 2] == 2.0 / 1e-8     # fmax(NaN, eps) = eps
    assert np.isinf(n[1]) and y[1, 0] == 0.0 and np.isnan(y[1, 1]) and y[1, 2] == 0.0
    assert np.isinf(n[2]) and np.all(y[2] == 0.0)                # the squares overflow fp32: an infinite norm
    assert n[3] == 0.0 and np.all(y[3] == 0.0)


def test_bounds_follow_the_contract():
    assert [N.frags(D) for D in (1, 64, 65, 128, 129, 256)] == [1, 1, 2, 2, 3, 4]
    assert ((N.frags(256) + 6) / 2 + 2) * N.U <= 7 * N.U < 8 * N.U
    assert N.y_bound(np.array([0.0, 1.0])).tolist() == [2.0 ** -149, 8 * 2.0 ** -24 + 2.0 ** -149]
    assert N.norm_bound(np.array([2.0]), 65)[0] == 4.5 * 2.0 ** -24 * 2.0


def test_argument_errors_need_no_device():
    from fairrec import _C
    lib = _C.lib()
    x = np.ones((2, 8), dtype=np.float32)
    px = x.ctypes.data
    for args in ((px, 2, 0, 8, px, 8), (px, 2, 257, 300, px, 300), (px, 2, 8, 7, px, 8), (px, 2, 8, 8, px, 7),
                 (px, 2, 8, 8, None, 8), (None, 2, 8, 8, px, 8), (px, -1, 8, 8, px, 8)):
        X, M, D, ldx, Y, ldy = args
        assert lib.fr_rows_l2_normalize(X, M, D, ldx, 1e-8, Y, ldy, None, None) == -1
        assert b"fr_rows_l2_normalize" in lib.fr_last_error()
    assert lib.fr_rows_l2_normalize(px, 2, 8, 8, -1.0, px, 8, None, None) == -1
    assert lib.fr_rows_l2_normalize(None, 0, 8, 8, 1e-8, None, 8, None, None) == 0         # M == 0: nothing to do
    assert np.all(x == 1.0)

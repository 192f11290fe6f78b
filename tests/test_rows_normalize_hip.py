"""GPU: fr_rows_l2_normalize against its float64 restatement (tests/rows_normalize_ref.py) within the bound its contract gives,
8 * 2^-24 |y| + 2^-149 for the rows and (E + 7) / 2 * 2^-24 for the norms, over every fragment count and both sides of each
fragment edge, partial and several workgroups, strided and in-place calls, rows below eps, large, zero, with a NaN, with an
infinity and with squares that overflow; a row's bits do not depend on where it sits or what sits next to it -- also where
a wave takes two rows per trip (more than 8192 rows) and a second trip (more than 16384)."""
import numpy as np
import pytest
import torch

import rows_normalize_ref as N
from fairrec import _C
from fairrec.functional import rows_l2_normalize

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = float(np.float32(1e-8))          # the value the fp32 entry receives
DIMS = [1, 2, 63, 64, 65, 128, 129, 255, 256]
NAN_ROW, INF_ROW, BIG_ROW, PROBE = 5, 6, 7, 200


def _matrix(D, M=257):
    """Rows 0 / 4 standard normal, 1 scaled to 1e-12, 2 to 1e12, 3 all zero, 5 with one NaN, 6 with one +inf, 7 scaled to 1e20
    (its squares overflow), the rest standard normal."""
    rng = np.random.default_rng(D)
    x = rng.standard_normal((M, D)).astype(np.float32)
    x[1] *= np.float32(1e-12)
    x[2] *= np.float32(1e12)
    x[3] = 0.0
    x[NAN_ROW, D // 2] = np.nan
    x[INF_ROW, (D - 1) // 3] = np.inf
    x[BIG_ROW] = np.float32(1e20) * (np.where(x[BIG_ROW] < 0, -1, 1) + x[BIG_ROW]).astype(np.float32)     # every |entry| >= 1e20
    return x


_cache = {}


def _case(D):
    """(x, y64, n64) of dimension D, computed once."""
    if D not in _cache:
        x = _matrix(D)
        _cache[D] = (x,) + N.normalize64(x, EPS)
    return _cache[D]


def _check(y, n, y64, n64, D):
    fin = np.isfinite(y64)
    assert np.array_equal(np.isnan(y), np.isnan(y64)) and np.array_equal(np.isinf(y), np.isinf(y64))
    err = np.abs(y.astype(np.float64)[fin] - y64[fin])
    assert np.all(err <= N.y_bound(y64[fin])), f"D = {D}: a row is off by {np.max(err / N.y_bound(y64[fin])):.3g} bounds"
    if n is not None:
        nf = np.isfinite(n64)
        assert np.array_equal(np.isnan(n), np.isnan(n64)) and np.array_equal(np.isinf(n), np.isinf(n64))
        assert np.all(np.abs(n.astype(np.float64)[nf] - n64[nf]) <= N.norm_bound(n64[nf], D))


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("D", DIMS)
def test_rows_against_float64(D):
    x, y64, n64 = _case(D)
    for M in (1, 3, 4, 5, 257):
        y, n = rows_l2_normalize(torch.from_numpy(x[:M]).to(DEV), eps=1e-8, want_norm=True)
        assert y.shape == (M, D) and n.shape == (M,) and y.dtype == n.dtype == torch.float32
        _check(y.cpu().numpy(), n.cpu().numpy(), y64[:M], n64[:M], D)
    y = y.cpu().numpy()
    assert np.all(y[3] == 0.0) and np.all(y[BIG_ROW] == 0.0)                    # a zero row; an infinite norm
    assert np.isnan(y[NAN_ROW]).sum() == 1 and np.isnan(y[INF_ROW]).sum() == 1
    if D > 1:
        assert np.max(np.abs(np.linalg.norm(y[[0, 2, 4, PROBE]].astype(np.float64), axis=1) - 1.0)) <= 8 * N.U
        assert np.all(y[1].astype(np.float64) == (x[1].astype(np.float64) / EPS).astype(np.float32))     # below eps: x / eps


@pytest.mark.parametrize("D", [1, 65, 256])
def test_strided_and_in_place(D):
    x, y64, n64 = _case(D)
    M = 257
    xs = torch.full((M, D + 3), 3.0, device=DEV)
    xs[:, :D] = torch.from_numpy(x).to(DEV)
    ys = torch.full((M, D + 5), 7.0, device=DEV)
    dense, norms = rows_l2_normalize(xs[:, :D].contiguous(), eps=1e-8, want_norm=True)
    out, n = rows_l2_normalize(xs[:, :D], eps=1e-8, out=ys[:, :D], want_norm=True)
    assert out.data_ptr() == ys.data_ptr() and bool((ys[:, D:] == 7.0).all()) and bool((xs[:, D:] == 3.0).all())
    _check(ys[:, :D].cpu().numpy(), n.cpu().numpy(), y64, n64, D)
    assert torch.equal(_bits(ys[:, :D]), _bits(dense)) and torch.equal(_bits(n), _bits(norms))          # the strides do not matter
    rows_l2_normalize(xs[:, :D], eps=1e-8, out=xs[:, :D])                                               # in place, strided
    assert torch.equal(_bits(xs[:, :D]), _bits(dense)) and bool((xs[:, D:] == 3.0).all())
    z = torch.from_numpy(x).to(DEV)
    assert rows_l2_normalize(z, eps=1e-8, out=z) is z and torch.equal(_bits(z), _bits(dense))          # in place, dense


@pytest.mark.parametrize("D", DIMS)
def test_a_row_does_not_depend_on_its_place(D):
    x, _, _ = _case(D)
    probe = x[PROBE:PROBE + 1]
    alone, n_alone = rows_l2_normalize(torch.from_numpy(probe).to(DEV), eps=1e-8, want_norm=True)
    five = x[:5].copy()
    five[2] = probe
    near_nan = x.copy()
    near_nan[PROBE - 1, 0] = np.nan
    near_nan[PROBE + 1] = np.nan
    for m, r in ((five, 2), (x, PROBE), (near_nan, PROBE)):
        y, n = rows_l2_normalize(torch.from_numpy(m).to(DEV), eps=1e-8, want_norm=True)
        assert torch.equal(_bits(y[r:r + 1]), _bits(alone)) and torch.equal(_bits(n[r:r + 1]), _bits(n_alone))


@pytest.mark.parametrize("D,M", [(65, 8195), (129, 16389)])
def test_two_rows_per_wave_and_a_second_trip(D, M):
    """Above 8192 rows a wave takes two rows per trip (row r with row r + 8192), above 16384 it makes a second trip."""
    x, y64, n64 = _case(D)
    big = np.tile(x, (M // 257 + 1, 1))[:M].copy()
    mate, probe_at = M - 8192 - 1, M - 1        # at 8195 rows the last row shares its wave's trip with `mate`; at 16389 it is alone
    big[mate] = np.nan
    big[probe_at] = x[PROBE]
    y, n = rows_l2_normalize(torch.from_numpy(big).to(DEV), eps=1e-8, want_norm=True)
    alone, n_alone = rows_l2_normalize(torch.from_numpy(x[PROBE:PROBE + 1]).to(DEV), eps=1e-8, want_norm=True)
    assert torch.equal(_bits(y[probe_at:]), _bits(alone)) and torch.equal(_bits(n[probe_at:]), _bits(n_alone))
    assert bool(torch.isnan(y[mate]).all())
    ref = rows_l2_normalize(torch.from_numpy(x).to(DEV), eps=1e-8)
    keep = np.ones(M, bool)
    keep[[mate, probe_at]] = False
    idx = torch.from_numpy(np.nonzero(keep)[0]).to(DEV)
    assert torch.equal(_bits(y[idx]), _bits(ref[idx % 257]))      # every other row: the bits it has in the 257-row call
    _check(ref.cpu().numpy(), None, y64, n64, D)


def test_argument_errors_and_the_empty_call():
    lib = _C.lib()
    x = torch.ones((4, 8), device=DEV)
    y = torch.full((4, 8), 7.0, device=DEV)
    s = _C.current_stream()
    for X, M, D, ldx, Y in ((x, 4, 0, 8, y), (x, 4, 257, 300, y), (x, 4, 8, 7, y), (x, 4, 8, 8, None), (x, -1, 8, 8, y)):
        assert lib.fr_rows_l2_normalize(_C.ptr(X), M, D, ldx, 1e-8, _C.ptr(Y), max(ldx, 8), None, s) == -1
        assert b"fr_rows_l2_normalize" in lib.fr_last_error()
    assert lib.fr_rows_l2_normalize(_C.ptr(x), 0, 8, 8, 1e-8, _C.ptr(y), 8, None, s) == 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())                       # nothing was launched or written
    empty = rows_l2_normalize(torch.empty((0, 8), device=DEV), want_norm=True)
    assert empty[0].shape == (0, 8) and empty[1].shape == (0,)
    with pytest.raises(ValueError, match="256"):
        rows_l2_normalize(torch.ones((2, 257), device=DEV))
    with pytest.raises(_C.FairrecError):
        rows_l2_normalize(torch.ones((2, 8)))

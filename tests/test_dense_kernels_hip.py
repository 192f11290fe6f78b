"""GPU: the dense-layer and BatchNorm kernels of csrc/mlp.hip, csrc/mlp_glds.hip and csrc/mlp_stream.hip, form by form
through the C ABI against the float64 references of tests/dense_ref.py, at the smallest shapes that reach each form and each
tile edge.  A form is selected by shape, alignment or a variable the library reads per call (FAIRREC_LINEAR_NO_SHARED,
FAIRREC_BN_FOLD_SEPARATE); the variables it reads once per process are not used.

Every output buffer sits between canaries and starts as NaN, every workspace starts as 0xFF bytes, every return code is
asserted (the framing helpers are tests/test_loss_kernels_hip.py's).  Two regimes per case (dense_ref's docstring):
  exact  small integers: the kernel must EQUAL the float64 reference (as values: the sign of a zero is not part of the
         contract) -- one lost, doubled or misplaced term of a reduction of any length shows;
  real   the data of tests/test_mlp_hip.py, every activation: |got - ref| <= the derived bound, element by element; each case
         prints its largest error over bound.
BatchNorm statistics: next to the bound, planted rows (one entry 2^20 per column, the row walking over the chunk edges) with
momentum 1: running_mean = 2^20 / M and invstd within 4 ulp, dbeta exact -- a row the kernel skips yields 0.

Which case reaches which kernel:
  linear_n1_fwd_kernel            test_forward_row_dot
  linear_fwd_fast_kernel<64>      test_forward_row_dot_neighbours, test_forward_fast64, the short cases of test_forward_fast128
  linear_fwd_fast_kernel<128>     test_forward_fast128 (full)
  linear_fwd_kernel               test_forward_slow
  linear_glds64_kernel<FWD, KS 1 / 2 / 4>   test_forward_lds_dma[macro-*]    linear_glds_kernel<FWD>   [private-*]
  linear_stream_kernel<fwd>       test_forward_streaming
  linear_glds64_kernel<BWD_IN> / linear_glds_kernel<BWD_IN>   test_input_gradient_lds_dma, test_fused_input_gradients
  linear_stream_kernel<bwd>       test_input_gradient_streaming, test_fused_input_gradients_at_the_streaming_threshold
  linear_bwd_input_kernel         test_input_gradient_general
  linear_bwd_weight_kernel, slab_reduce_kernel   test_weight_gradient[general-*], test_weight_gradient_rows_per_split_switch
  linear_glds64_kernel<BWD_W> / linear_glds_kernel<BWD_W>   test_weight_gradient[macro-* / private-*], ..._empty_trailing_splits
  wgrad_stream_kernel             test_weight_gradient_streaming
  linear_glds64_wmulti_kernel, slab_reduce_multi_kernel (wide and plain)   test_weight_gradient_multi*
  parts_sum_kernel                test_parts_sum
  linear_n1_bwd_kernel            test_one_output_backward
  bn_fwd_stats_kernel, bn_fwd_apply_fold_kernel<false>, bn_bwd_stats_kernel, bn_bwd_apply_fold_kernel   test_batchnorm[inline-*]
  bn_fwd_fold_kernel, bn_fwd_apply_kernel, bn_bwd_fold_kernel, bn_bwd_apply_kernel   test_batchnorm[separate-*]
                                  (both rows also: test_batchnorm_planted_rows; one against the other, bit for bit:
                                  test_batchnorm_fold_forms_agree)
  bn_fwd_apply_fold_kernel<true> / bn_fwd_apply_drop_kernel   test_batchnorm_forward_with_dropout[inline / separate]
  the statistics epilogues of linear_glds64_kernel<FWD> and <BWD_IN_BN>   test_forward_statistics_epilogue,
                                                                          test_backward_statistics_epilogue
"""
import numpy as np
import pytest
import torch

import dense_ref as D
from test_loss_kernels_hip import _Outs, _bits, _lib, _ptr, _st, _within, _ws

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -3
ACTS_OF = {"exact": (0, 1), "real": (0, 1, 2, 3, 4)}
ROWS32 = [1, 31, 32, 33, 63, 64, 65, 97]


def _d(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _Dev:
    """the device copies of a case's operands"""

    def __init__(self, c):
        self.x0, self.x1, self.W, self.b, self.dY, self.keep = (_d(a) for a in (c.x0, c.x1, c.W, c.b, c.dY, c.keep))


def _exact(what, got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = ~(got == ref)
    print(f"{what}: exact regime, {got.size} values, {int(bad.sum())} differ")
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} values differ from the float64 reference, first at {i}: "
                             f"got {got[i]!r}, reference {ref[i]!r}")


def _check(what, regime, got, ref, bound):
    if regime == "exact":
        _exact(what, got, ref)
    else:
        _within(what, np.asarray(got, np.float64), ref, bound)


# ---- forward ----------------------------------------------------------------------------------------------------------------

def _fwd(c, d, act, bias=True, x0=None, keep=None):
    o = _Outs()
    Y = o.new(c.M, c.N)
    rc = _lib().fr_linear_fwd((d.x0 if x0 is None else x0).data_ptr(), c.k0, _ptr(d.x1), c.k1,
                              _ptr(d.keep if keep is None else keep), c.scale, d.W.data_ptr(), _ptr(d.b if bias else None), c.M, c.N,
                              act, Y.data_ptr(), _st())
    assert rc == 0 and o.ok(), (rc, c.M, c.k0, c.k1, c.N, act)
    return Y.cpu().numpy()


def _check_fwd(tag, M, k0, k1, N, mask=False, **kw):
    """both regimes, every activation of the regime with a bias, no activation without one"""
    for regime in ("exact", "real"):
        c = D.case(regime, M, k0, k1, N, mask=mask)
        d = _Dev(c)
        X = D.dropped(D.cat(c.x0, c.x1), c.keep, c.scale)
        for bias in (True, False):
            z, ez = D.product(X, c.W, c.b if bias else None, pre=int(mask))
            for act in (ACTS_OF[regime] if bias else (0,)):
                ref, e = D.act_out(z, ez, act)
                _check(f"fr_linear_fwd {tag} {regime} M={M} k={k0}+{k1} N={N} act={act} bias={bias}", regime,
                       _fwd(c, d, act, bias, **kw), ref, e)


@pytest.mark.parametrize("K", [64, 512])
def test_forward_row_dot(K):
    for M in (1, 15, 16, 17):
        _check_fwd("row-dot", M, K, 0, 1)


@pytest.mark.parametrize("k0,k1", [(576, 0), (96, 0), (32, 32)], ids=["K576", "K96", "two_blocks"])
def test_forward_row_dot_neighbours(k0, k1):
    """N == 1 just outside the row-dot form (K > 512, K % 64 != 0, a second block): another kernel, the same result"""
    for M in (1, 16, 17):
        _check_fwd("row-dot neighbour", M, k0, k1, 1)


GLDS_K = [(32, 0), (96, 0), (160, 0), (128, 0), (192, 0), (256, 0), (32, 96), (96, 32)]


@pytest.mark.parametrize("k0,k1", GLDS_K, ids=[f"k{a}+{b}" for a, b in GLDS_K])
@pytest.mark.parametrize("form", ["macro", "private"])
def test_forward_lds_dma(form, k0, k1, monkeypatch):
    """the LDS-DMA forward (no mask, K and k0 multiples of 32, N >= 8), macro-tile and wave-private, each against float64:
    reduction parts 1 (K = 32, 96, 160), 2 (128, 192) and 4 (256), ragged rows and columns, two-block inputs"""
    if form == "private":
        monkeypatch.setenv("FAIRREC_LINEAR_NO_SHARED", "1")
    for N in (8, 31, 32, 33, 64, 65, 96):
        for M in ROWS32:
            _check_fwd(form, M, k0, k1, N)


@pytest.mark.parametrize("M,K,N", [(32768, 32, 64), (32769, 128, 128), (32769, 96, 64)])
def test_forward_streaming(M, K, N):
    _check_fwd("streaming", M, K, 0, N)


@pytest.mark.parametrize("k0,k1,N,mask", [(36, 0, 7, False), (36, 0, 65, False), (4, 8, 64, False), (32, 0, 1, False), (32, 0, 7, False),
                                          (64, 0, 40, True)], ids=["K36_N7", "K36_N65", "k4+8", "K32_N1", "K32_N7", "K64_mask"])
def test_forward_fast64(k0, k1, N, mask):
    for M in (1, 63, 64, 65, 129):
        _check_fwd("fast<64>", M, k0, k1, N, mask=mask)


@pytest.mark.parametrize("M,N,K,mask", [(16321, 65, 36, False), (8129, 129, 36, False), (8129, 200, 64, True)])
@pytest.mark.parametrize("short", ["full", "one_row_short", "one_column_short"])
def test_forward_fast128(M, N, K, mask, short):
    """linear_fwd_fast_kernel<128> needs N > 64 and ceil(M / 64) ceil(N / 128) >= 256; one row or one column less takes
    linear_fwd_fast_kernel<64> -- both must be right"""
    if short == "one_row_short":
        M = (M - 1) // 64 * 64
    if short == "one_column_short":
        N = {65: 64, 129: 128, 200: 128}[N]
    full = N > 64 and ((M + 63) // 64) * ((N + 127) // 128) >= 256
    assert full == (short == "full"), (M, N)
    _check_fwd("fast<128>" if full else "fast<64> below fast<128>", M, K, 0, N, mask=mask)


@pytest.mark.parametrize("k0,k1,mask", [(37, 0, False), (37, 11, True)], ids=["K37", "k37+11_mask"])
def test_forward_slow(k0, k1, mask):
    for N in (3, 65):
        for M in (1, 63, 64, 65):
            _check_fwd("slow", M, k0, k1, N, mask=mask)


def test_forward_slow_by_alignment():
    """operands of a fast shape that are not aligned take the general kernel: x0 a view one float into its buffer, a mask
    pointer off by one byte"""
    for regime in ("exact", "real"):
        for M in (33, 65):
            c = D.case(regime, M, 64, 0, 40, mask=True)
            d = _Dev(c)
            z, ez = D.product(D.dropped(D.cat(c.x0), c.keep, c.scale), c.W, c.b, pre=1)
            buf = torch.zeros(M * 64 + 1, device="cuda")
            buf[1:] = d.x0.reshape(-1)
            x0 = buf[1:].view(M, 64)
            kbuf = torch.zeros(M * 64 + 1, dtype=torch.uint8, device="cuda")
            kbuf[1:] = d.keep.reshape(-1)
            keep = kbuf[1:].view(M, 64)
            assert x0.data_ptr() % 16 == 4 and keep.data_ptr() % 4 == 1
            for act in ACTS_OF[regime]:
                ref, e = D.act_out(z, ez, act)
                _check(f"fr_linear_fwd x0 + 4 bytes {regime} M={M} act={act}", regime, _fwd(c, d, act, x0=x0), ref, e)
                _check(f"fr_linear_fwd mask + 1 byte {regime} M={M} act={act}", regime, _fwd(c, d, act, keep=keep), ref, e)
            c2 = D.case(regime, M, 64, 0, 32)           # without a mask: the LDS-DMA shape, but for the pointer
            d2 = _Dev(c2)
            buf[1:] = d2.x0.reshape(-1)
            ref, e = D.linear_fwd(c2.x0, None, None, 1.0, c2.W, c2.b, 0)
            _check(f"fr_linear_fwd x0 + 4 bytes, no mask {regime} M={M}", regime, _fwd(c2, d2, 0, x0=x0), ref, e)


# ---- input gradient ---------------------------------------------------------------------------------------------------------

def _bwd_input(c, d, Y, act):
    o = _Outs()
    dx0 = o.new(c.M, c.k0)
    dx1 = o.new(c.M, c.k1) if c.k1 else None
    rc = _lib().fr_linear_bwd_input(d.dY.data_ptr(), Y.data_ptr(), act, d.W.data_ptr(), _ptr(d.keep), c.scale, c.M, c.N,
                                    dx0.data_ptr(), c.k0, _ptr(dx1), c.k1, _st())
    assert rc == 0 and o.ok(), (rc, c.M, c.N, c.k0, c.k1, act)
    return np.concatenate([dx0.cpu().numpy()] + ([dx1.cpu().numpy()] if c.k1 else []), axis=1)


def _outputs_of(c, act):
    """the fp32 Y = act(z) a backward entry point is handed (any fp32 tensor of the activation's range serves the contract)"""
    z, _ = D.product(D.dropped(D.cat(c.x0, c.x1), c.keep, c.scale), c.W, c.b)
    return D.act_out(z, 0 * z, act)[0].astype(np.float32)


def _check_bwd_input(tag, M, N, k0, k1, mask=False, acts=None):
    for regime in ("exact", "real"):
        c = D.case(regime, M, k0, k1, N, mask=mask)
        d = _Dev(c)
        for act in (acts if acts is not None else ACTS_OF[regime]):
            if regime == "exact" and act > 1:
                continue
            Y = _outputs_of(c, act)
            ref, e = D.linear_bwd_input(c.dY, Y, act, c.W, c.keep, c.scale)
            _check(f"fr_linear_bwd_input {tag} {regime} M={M} N={N} k={k0}+{k1} act={act}", regime, _bwd_input(c, d, _d(Y), act), ref, e)


@pytest.mark.parametrize("N", [32, 96, 160, 128, 192, 256])
@pytest.mark.parametrize("form", ["macro", "private"])
def test_input_gradient_lds_dma(form, N, monkeypatch):
    """dX = dY W in the LDS-DMA form (act none, no mask, widths multiples of 32): the reduction runs over N (parts 1, 2, 4),
    one- and two-block outputs"""
    if form == "private":
        monkeypatch.setenv("FAIRREC_LINEAR_NO_SHARED", "1")
    for k0, k1 in ((32, 0), (64, 0), (96, 0), (32, 96), (96, 32)):
        for M in ROWS32:
            _check_bwd_input(form, M, N, k0, k1, acts=(0,))


@pytest.mark.parametrize("M,N,K", [(32768, 64, 64), (32769, 128, 128), (32769, 96, 64)])
def test_input_gradient_streaming(M, N, K):
    _check_bwd_input("streaming", M, N, K, 0, acts=(0,))


@pytest.mark.parametrize("M,N,k0,k1,mask", [(65, 33, 37, 0, True), (1, 7, 5, 0, False), (64, 70, 37, 11, True), (33, 64, 32, 32, True),
                                            (63, 32, 32, 0, False)])
def test_input_gradient_general(M, N, k0, k1, mask):
    """linear_bwd_input_kernel: an activation, a mask, or ragged widths (the last case: a fast shape kept out by its activation)"""
    _check_bwd_input("general", M, N, k0, k1, mask=mask, acts=(1, 2, 3, 4) if (M, N) == (63, 32) else None)


def _fused_case(regime, M, N, K, act):
    c = D.case(regime, M, K, 0, N, seed=act)
    if regime == "exact":
        src = c.x0 if act else np.maximum(c.x0, 0) * 2 * (np.random.default_rng(M).random((M, K)) >= 0.5)
    else:
        src = D.act_out(c.x0.astype(np.float64), 0.0, act or 1)[0]
        if not act:
            src = src * (np.random.default_rng(M).random((M, K)) >= 0.4) * np.float32(1 / 0.6)
    return c, np.ascontiguousarray(src, dtype=np.float32)


def _check_fused(tag, M, N, K):
    """fr_linear_bwd_input_relu (act 0 here) and fr_linear_bwd_input_act (acts 1-4) against float64"""
    lib = _lib()
    for regime in ("exact", "real"):
        for act in ((0, 1) if regime == "exact" else (0, 1, 2, 3, 4)):
            c, src = _fused_case(regime, M, N, K, act)
            d, s = _Dev(c), _d(src)
            o = _Outs()
            dA = o.new(M, K)
            if act == 0:
                scale = 2.0 if regime == "exact" else 1 / 0.6
                rc = lib.fr_linear_bwd_input_relu(d.dY.data_ptr(), d.W.data_ptr(), M, N, K, s.data_ptr(), scale, dA.data_ptr(), _st())
                ref, e = D.bwd_input_relu(c.dY, c.W, src, scale)
            else:
                rc = lib.fr_linear_bwd_input_act(d.dY.data_ptr(), d.W.data_ptr(), M, N, K, s.data_ptr(), act, dA.data_ptr(), _st())
                ref, e = D.bwd_input_act(c.dY, c.W, src, act)
            assert rc == 0 and o.ok(), (rc, M, N, K, act)
            _check(f"{'fr_linear_bwd_input_act' if act else 'fr_linear_bwd_input_relu'} {tag} {regime} M={M} N={N} K={K} act={act}",
                   regime, dA.cpu().numpy(), ref, e)


@pytest.mark.parametrize("N,K", [(32, 32), (64, 96), (128, 256)])
def test_fused_input_gradients(N, K):
    for M in (1, 33, 64, 65):
        _check_fused("macro", M, N, K)
    dY, W, src, dA = (torch.zeros(64 * 256, device="cuda") for _ in range(4))
    lib = _lib()
    assert lib.fr_linear_bwd_input_relu(dY.data_ptr(), W.data_ptr(), 64, 24, K, src.data_ptr(), 2.0, dA.data_ptr(), _st()) == EUNSUPPORTED
    assert lib.fr_linear_bwd_input_act(dY.data_ptr(), W.data_ptr(), 64, 24, K, src.data_ptr(), 1, dA.data_ptr(), _st()) == EUNSUPPORTED


@pytest.mark.parametrize("M", [32768, 32769])
@pytest.mark.parametrize("N,K", [(64, 64), (128, 128)])
def test_fused_input_gradients_at_the_streaming_threshold(M, N, K):
    _check_fused("streaming threshold", M, N, K)


# ---- weight gradient --------------------------------------------------------------------------------------------------------

def _bwd_weight(c, d, Y, act, want_db=True):
    lib = _lib()
    o = _Outs()
    dW = o.new(c.N, c.K)
    db = o.new(c.N) if want_db else None
    ws = _ws(lib.fr_linear_bwd_weight_workspace_bytes(c.M, c.N, c.K))
    rc = lib.fr_linear_bwd_weight(d.dY.data_ptr(), Y.data_ptr(), act, d.x0.data_ptr(), c.k0, _ptr(d.x1), c.k1, _ptr(d.keep), c.scale,
                                  c.M, c.N, dW.data_ptr(), _ptr(db), ws.data_ptr(), ws.numel(), _st())
    assert rc == 0 and o.ok(), (rc, c.M, c.N, c.k0, c.k1, act)
    return dW.cpu().numpy(), None if db is None else db.cpu().numpy()


def _check_bwd_weight(tag, M, N, k0, k1, mask=False, regimes=("exact",), acts=None, no_db=True):
    for regime in regimes:
        c = D.case(regime, M, k0, k1, N, mask=mask)
        d = _Dev(c)
        for act in (acts if acts is not None else ACTS_OF[regime]):
            if regime == "exact" and act > 1:
                continue
            Y = _outputs_of(c, act)
            rW, eW, rb, eb = D.linear_bwd_weight(c.dY, Y, act, c.x0, c.x1, c.keep, c.scale)
            dW, db = _bwd_weight(c, d, _d(Y), act)
            what = f"fr_linear_bwd_weight {tag} {regime} M={M} N={N} k={k0}+{k1} act={act}"
            _check(what + " dW", regime, dW, rW, eW)
            _check(what + " db", regime, db, rb, eb)
            if no_db and act == 0:
                only, none = _bwd_weight(c, d, _d(Y), act, want_db=False)
                assert none is None and _bits(torch.from_numpy(only), torch.from_numpy(dW)), what + ": db == NULL changes dW"


WG_ROWS = [1, 31, 32, 33, 128, 129, 161, 4095, 4096, 4097]


@pytest.mark.parametrize("N,k0,k1", [(32, 32, 0), (64, 64, 32), (96, 32, 0)], ids=["32x32", "64x64+32", "96x32"])
@pytest.mark.parametrize("form", ["macro", "private"])
def test_weight_gradient_lds_dma(form, N, k0, k1, monkeypatch):
    """widths multiples of 32, act none, no mask: one split (M <= 128) and more, a last split of one row (M = 129 with 96-row
    splits ends on 33 rows; M = 4097 = 32 x 128 + 1), the reduction tail inside a 32-row chunk; exact regime"""
    if form == "private":
        monkeypatch.setenv("FAIRREC_LINEAR_NO_SHARED", "1")
    for M in WG_ROWS:
        _check_bwd_weight(form, M, N, k0, k1, acts=(0,))


@pytest.mark.parametrize("N,k0,k1,mask", [(33, 37, 0, False), (70, 37, 11, True), (3, 5, 0, True), (32, 32, 0, True)],
                         ids=["33x37", "70x37+11_mask", "3x5_mask", "32x32_mask"])
def test_weight_gradient_general(N, k0, k1, mask):
    """linear_bwd_weight_kernel: ragged widths, masks, every activation (real regime: bound; exact regime: none and relu)"""
    for M in WG_ROWS:
        _check_bwd_weight("general", M, N, k0, k1, mask=mask, regimes=("exact", "real") if M in (1, 33, 129, 4097) else ("exact",))


@pytest.mark.parametrize("N,K", [(512, 256), (256, 256), (510, 250), (250, 250)])
def test_weight_gradient_rows_per_split_switch(N, K):
    """128 -> 256 rows per split needs M >= 4096 and ceil(N / 64) ceil(K / 64) ceil(M / 256) >= 512: either side of both
    conditions, both kernels (widths multiples of 32 and not)"""
    for M in (4095, 4096, 4097):
        rows = 256 if M >= 4096 and ((N + 63) // 64) * ((K + 63) // 64) * ((M + 255) // 256) >= 512 else 128
        assert rows == (256 if M >= 4096 and N >= 510 else 128)
        _check_bwd_weight(f"{rows} rows per split", M, N, K, 0, acts=(0,), no_db=False)


def test_weight_gradient_empty_trailing_splits():
    """M = 1921, N = K = 1024: the 64 MiB slab cap leaves 15 splits of 160 rows, so split 12 holds one row and splits 13 and 14
    none -- they must come out as zeros (the workspace starts as NaN bytes), or the slab sum adds what was there"""
    assert _lib().fr_linear_bwd_weight_workspace_bytes(1921, 1024, 1024) == 15 * 1024 * 1025 * 4
    _check_bwd_weight("empty splits", 1921, 1024, 1024, 0, acts=(0,), no_db=False)


@pytest.mark.parametrize("M", [65536, 65537])
@pytest.mark.parametrize("N,K", [(64, 64), (128, 64), (128, 128)])
def test_weight_gradient_streaming(M, N, K):
    _check_bwd_weight("streaming", M, N, K, 0, acts=(0,))


def _jobs_call(M, specs, seed=0):
    """one fr_linear_bwd_weight_multi call; spec = (N, k0, k1, want_db) or ('parts', n_parts, n); exact regime"""
    from fairrec import _C
    lib = _lib()
    o = _Outs()
    hold, jobs, want = [], [], []
    for j, s in enumerate(specs):
        if s[0] == "parts":
            _, P, n = s
            part = np.random.default_rng([seed, j]).integers(-3, 4, (P, n)).astype(np.float32)
            pd, dW = _d(part), o.new(n)
            hold += [pd]
            jobs.append(_C.FrWgradJob(None, None, n, None, 0, 1, dW.data_ptr(), None, pd.data_ptr(), P))
            want.append((dW, None, D.parts_sum(part)[0], None))
            continue
        N, k0, k1, want_db = s
        c = D.exact_case(M, k0, k1, N, seed=seed + j)
        d = _Dev(c)
        dW, db = o.new(N, c.K), (o.new(N) if want_db else None)
        hold += [d]
        jobs.append(_C.FrWgradJob(d.dY.data_ptr(), d.x0.data_ptr(), k0, _ptr(d.x1) or None, k1, N, dW.data_ptr(), _ptr(db) or None, None, 0))
        rW, _, rb, _ = D.linear_bwd_weight(c.dY, c.dY, 0, c.x0, c.x1, None, 1.0)
        want.append((dW, db, rW, rb))
    arr = (_C.FrWgradJob * len(jobs))(*jobs)
    ws = _ws(lib.fr_linear_bwd_weight_multi_workspace_bytes(arr, len(jobs), M))
    rc = lib.fr_linear_bwd_weight_multi(arr, len(jobs), M, ws.data_ptr(), ws.numel(), _st())
    assert rc == 0 and o.ok(), rc
    for j, (dW, db, rW, rb) in enumerate(want):
        _exact(f"fr_linear_bwd_weight_multi M={M} job {j} {specs[j]} dW", dW.cpu().numpy().reshape(rW.shape), rW)
        if db is not None:
            _exact(f"fr_linear_bwd_weight_multi M={M} job {j} {specs[j]} db", db.cpu().numpy(), rb)
    return arr, hold, ws


SIX_JOBS = [(32, 32, 0, True), (64, 64, 0, True), (128, 96, 0, True), (64, 32, 32, True), (32, 64, 0, False), ("parts", 3, 64)]


def test_weight_gradient_multi_six_jobs_of_different_shapes():
    """M = 8321: the (32, 32) job has 66 splits and 1056 outputs -- the `wide` slab sum --, the others the plain one; a two-block
    job, a job without db, a sums-only job of 3 parts"""
    assert _lib().fr_linear_bwd_weight_workspace_bytes(8321, 32, 32) == 66 * 32 * 33 * 4
    _jobs_call(8321, SIX_JOBS)


def test_weight_gradient_multi_small_batch_and_eight_jobs():
    _jobs_call(33, SIX_JOBS, seed=1)
    _jobs_call(257, SIX_JOBS + [(96, 32, 64, True), ("parts", 5, 33)], seed=2)


def test_weight_gradient_multi_refuses_a_ninth_job_and_a_job_outside_the_fast_form():
    from fairrec import _C
    lib = _lib()
    c = D.exact_case(33, 32, 0, 32)
    d = _Dev(c)
    o = _Outs()
    dW = o.new(32, 32)
    job = lambda N, k0, dY=d.dY: _C.FrWgradJob(dY.data_ptr(), d.x0.data_ptr(), k0, None, 0, N, dW.data_ptr(), None, None, 0)
    ws = _ws(9 * lib.fr_linear_bwd_weight_workspace_bytes(33, 32, 32) + 4096)
    nine = (_C.FrWgradJob * 9)(*[job(32, 32) for _ in range(9)])
    assert lib.fr_linear_bwd_weight_multi(nine, 9, 33, ws.data_ptr(), ws.numel(), _st()) == EINVAL
    for N, k0 in ((24, 32), (32, 24)):
        one = (_C.FrWgradJob * 1)(job(N, k0))
        assert lib.fr_linear_bwd_weight_multi(one, 1, 33, ws.data_ptr(), ws.numel(), _st()) == EUNSUPPORTED
    shifted = torch.zeros(33 * 32 + 1, device="cuda")[1:]
    one = (_C.FrWgradJob * 1)(job(32, 32, dY=shifted))
    assert lib.fr_linear_bwd_weight_multi(one, 1, 33, ws.data_ptr(), ws.numel(), _st()) == EUNSUPPORTED
    assert o.ok() and bool(torch.isnan(dW).all())             # nothing was written


def test_backward_fast_form_edges(monkeypatch):
    """The one rule of the backward fast form (csrc/mlp.hip::bwd_fast_form) at its edges, through the entries that exist in
    that form only -- the three epilogue entries and a one-job fr_linear_bwd_weight_multi -- at M = 33: (N, K) = (32, 32) is
    served; N = 31, K = 33, K = 48 and a dY 4 bytes off a 16-byte boundary are FR_EUNSUPPORTED; layers._fast_form, the host's
    copy of the rule, answers each case alike.  fr_linear_bwd_input_bnstats also refuses when the BatchNorm apply launch
    would not fold the partials it leaves (FAIRREC_BN_FOLD_SEPARATE)."""
    from fairrec import _C
    from fairrec.model.layers import _fast_form
    lib, M = _lib(), 33
    z = lambda *shape: torch.zeros(*shape, device="cuda")

    def calls(N, K, shift):
        dY = z(M * N + 1)[1:].view(M, N) if shift else z(M, N)
        W, src, X = z(N, K), z(M, K), z(M, K)
        o = _Outs()
        dA, dX, dW = o.new(M, K), o.new(M, K), o.new(N, K)
        ws = _ws(lib.fr_bn_workspace_bytes(M, K))
        job = (_C.FrWgradJob * 1)(_C.FrWgradJob(dY.data_ptr(), X.data_ptr(), K, None, 0, N, dW.data_ptr(), None, None, 0))
        wsm = _ws(lib.fr_linear_bwd_weight_multi_workspace_bytes(job, 1, M))
        rcs = dict(
            relu=lib.fr_linear_bwd_input_relu(dY.data_ptr(), W.data_ptr(), M, N, K, src.data_ptr(), 2.0, dA.data_ptr(), _st()),
            act=lib.fr_linear_bwd_input_act(dY.data_ptr(), W.data_ptr(), M, N, K, src.data_ptr(), 1, dA.data_ptr(), _st()),
            bnstats=lib.fr_linear_bwd_input_bnstats(dY.data_ptr(), W.data_ptr(), M, N, K, dX.data_ptr(), src.data_ptr(), src.data_ptr(), 0,
                                                    ws.data_ptr(), ws.numel(), 0.0, 0, 0, None, _st()),
            multi=lib.fr_linear_bwd_weight_multi(job, 1, M, wsm.data_ptr(), wsm.numel(), _st()))
        assert o.ok(), (N, K, shift)
        return rcs, _fast_form(N, K, K, dY, W) and _fast_form(N, K, K, dY, X), (dA, dX, dW)

    rcs, host, outs = calls(32, 32, False)
    assert host and all(rc == 0 for rc in rcs.values()), rcs
    assert all(bool((t == 0).all()) for t in outs)                  # zeros in: every output written, as zeros
    for N, K, shift in ((31, 32, False), (32, 33, False), (64, 48, False), (32, 32, True)):
        rcs, host, outs = calls(N, K, shift)
        assert not host and all(rc == EUNSUPPORTED for rc in rcs.values()), (N, K, shift, rcs)
        assert all(bool(torch.isnan(t).all()) for t in outs), (N, K, shift)      # nothing was written
    monkeypatch.setenv("FAIRREC_BN_FOLD_SEPARATE", "1")
    rcs, host, outs = calls(32, 32, False)
    assert host and rcs == dict(relu=0, act=0, bnstats=EUNSUPPORTED, multi=0), rcs
    assert bool(torch.isnan(outs[1]).all())


@pytest.mark.parametrize("parts", [1, 3, 5])
def test_parts_sum(parts):
    for n in (1, 63, 64, 65, 4097):
        for regime in ("exact", "real"):
            rng = np.random.default_rng([parts, n])
            part = (rng.integers(-3, 4, (parts, n)) if regime == "exact" else rng.standard_normal((parts, n))).astype(np.float32)
            o = _Outs()
            out = o.new(n)
            pd = _d(part)
            rc = _lib().fr_parts_sum(pd.data_ptr(), parts, n, out.data_ptr(), _st())
            assert rc == 0 and o.ok()
            ref, e = D.parts_sum(part)
            _check(f"fr_parts_sum {regime} parts={parts} n={n}", regime, out.cpu().numpy(), ref, e)


# ---- the one-output pair ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [64, 512])
@pytest.mark.parametrize("relu_scale", [0.0, 2.0])
def test_one_output_backward(K, relu_scale):
    lib = _lib()
    for M in (1, 127, 128, 129, 4097):
        for regime in ("exact", "real"):
            for act in ACTS_OF[regime]:
                c = D.case(regime, M, K, 0, 1, seed=act)
                X = c.x0
                if relu_scale:
                    X = np.maximum(X, 0) * ((np.random.default_rng(M).random((M, K)) >= 0.5) * np.float32(relu_scale))
                    D.assert_exact(6, 3, max(M, K), 3)
                X = np.ascontiguousarray(X, dtype=np.float32)
                z, _ = D.product(X, c.W, c.b)
                Y = D.act_out(z, 0 * z, act)[0].astype(np.float32)
                r = D.n1_bwd(c.dY, Y, act, X, c.W, relu_scale)
                Xd, Wd, dYd, Yd = _d(X), _d(c.W), _d(c.dY), _d(Y)
                full = None
                for want_dx, want_db in ((True, True), (False, True), (True, False), (False, False)):
                    o = _Outs()
                    dW = o.new(K)
                    dX = o.new(M, K) if want_dx else None
                    db = o.new(1) if want_db else None
                    ws = _ws(lib.fr_linear_bwd_weight_workspace_bytes(M, 1, K))
                    rc = lib.fr_linear_n1_bwd(dYd.data_ptr(), Yd.data_ptr(), act, Xd.data_ptr(), K, Wd.data_ptr(), M, relu_scale,
                                              _ptr(dX), dW.data_ptr(), _ptr(db), ws.data_ptr(), ws.numel(), _st())
                    assert rc == 0 and o.ok(), (rc, M, K, act)
                    if full is None:
                        what = f"fr_linear_n1_bwd {regime} M={M} K={K} act={act} relu_scale={relu_scale}"
                        _check(what + " dW", regime, dW.cpu().numpy(), r.dW, r.e_dW)
                        _check(what + " db", regime, db.cpu().numpy()[0], r.db, r.e_db)
                        _check(what + " dX", regime, dX.cpu().numpy(), r.dX, r.e_dX)
                        full = (dW.cpu(), dX.cpu(), db.cpu())
                    else:       # an output left out changes none of the others
                        assert _bits(dW, full[0]) and (dX is None or _bits(dX, full[1])) and (db is None or _bits(db, full[2]))


# ---- BatchNorm ----------------------------------------------------------------------------------------------------------------

BN_ROWS = [1, 2, 31, 32, 33, 257, 8192, 8193, 32768, 32769]
BN_COLS = [1, 4, 63, 64, 65, 100]


def _bn_fwd(Z, gam, beta, eps, mom, rm, rv, act, M, N):
    """fr_bn_fwd on device operands; returns (Y, xhat, invstd, running_mean, running_var) as device tensors"""
    lib = _lib()
    o = _Outs()
    Y, xh, inv, rmo, rvo = o.new(M, N), o.new(M, N), o.new(N), o.new(N), o.new(N)
    rmo.copy_(rm)
    rvo.copy_(rv)
    ws = _ws(lib.fr_bn_workspace_bytes(M, N))
    rc = lib.fr_bn_fwd(Z.data_ptr(), gam.data_ptr(), beta.data_ptr(), eps, mom, rmo.data_ptr(), rvo.data_ptr(), M, N, act, Y.data_ptr(),
                       xh.data_ptr(), inv.data_ptr(), ws.data_ptr(), ws.numel(), _st())
    assert rc == 0 and o.ok(), (rc, M, N, act)
    return Y, xh, inv, rmo, rvo


def _bn_bwd(dY, Y, act, xh, inv, gam, M, N, have_stats=0, ws=None):
    lib = _lib()
    o = _Outs()
    dZ, dg, db = o.new(M, N), o.new(N), o.new(N)
    ws = _ws(lib.fr_bn_workspace_bytes(M, N)) if ws is None else ws
    rc = lib.fr_bn_bwd_ex(dY.data_ptr(), Y.data_ptr(), act, xh.data_ptr(), inv.data_ptr(), gam.data_ptr(), M, N, dZ.data_ptr(),
                          dg.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), have_stats, _st())
    assert rc == 0 and o.ok(), (rc, M, N, act)
    return dZ.cpu().numpy(), dg.cpu().numpy(), db.cpu().numpy()


def _ulps(got, ref):
    """|got - ref| in units of the fp32 spacing at ref"""
    ref = np.asarray(ref, np.float64)
    return float((np.abs(np.asarray(got, np.float64) - ref) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)).max())


def _check_bn_fwd_outputs(tag, got, r):
    Y, xh, inv, rm, rv = (t.cpu().numpy() for t in got)
    _within(tag + " Y", Y, r.Y, r.e_Y)
    _within(tag + " xhat", xh, r.xhat, r.e_xhat)
    _within(tag + " invstd", inv, r.invstd, r.e_invstd)
    _within(tag + " running_mean", rm, r.rmean, r.e_rmean)
    _within(tag + " running_var", rv, r.rvar, r.e_rvar)


@pytest.mark.parametrize("M", BN_ROWS)
@pytest.mark.parametrize("fold", ["inline", "separate"])
def test_batchnorm(fold, M, monkeypatch):
    """fr_bn_fwd and fr_bn_bwd, the fold inside the apply launch and as a launch of its own: every activation against the
    carried bound (column means far from zero included)"""
    if fold == "separate":
        monkeypatch.setenv("FAIRREC_BN_FOLD_SEPARATE", "1")
    for N in BN_COLS:
        for act in (0, 1, 2, 3, 4):
            c = D.bn_case(M, N, seed=act)
            Zd, gd, bd, dYd = _d(c.Z), _d(c.gamma), _d(c.beta), _d(c.dY)
            got = _bn_fwd(Zd, gd, bd, c.eps, c.momentum, _d(c.rmean), _d(c.rvar), act, M, N)
            tag = f"fr_bn_fwd {fold} M={M} N={N} act={act}"
            _check_bn_fwd_outputs(tag, got, D.bn_fwd(c.Z, c.gamma, c.beta, c.eps, c.momentum, c.rmean, c.rvar, act))
            Y, xh, inv = got[:3]
            if M == 1:
                assert bool((xh == 0).all())
            q = D.bn_bwd(c.dY, Y.cpu().numpy(), act, xh.cpu().numpy(), inv.cpu().numpy(), c.gamma)
            dZ, dg, db = _bn_bwd(dYd, Y, act, xh, inv, gd, M, N)
            tag = f"fr_bn_bwd {fold} M={M} N={N} act={act}"
            _within(tag + " dZ", dZ, q.dZ, q.e_dZ)
            _within(tag + " dgamma", dg, q.dgamma, q.e_dgamma)
            _within(tag + " dbeta", db, q.dbeta, q.e_dbeta)


@pytest.mark.parametrize("M", BN_ROWS)
@pytest.mark.parametrize("fold", ["inline", "separate"])
def test_batchnorm_planted_rows(fold, M, monkeypatch):
    """Every row is counted: Z (backward: dY) is zero but for one entry 2^20 per column, whose row walks over rows 0-3, 30-33,
    M - 2, M - 1 and a seeded sample; momentum 1.  dbeta must be 2^20 exactly, running_mean 2^20 / M and invstd the float64
    value within 4 ulp -- a skipped row yields 0.

    M = 32768 is the regression case of the fold's compensated chains (mlp_bn_math.hpp::bn_sum_comp).  With a plain chain per
    wave invstd was 44.8 ulp off there, with no row lost: the chunk with the planted entry comes first and leaves the chain at
    ~2^40, where the spacing of fp32 is 2^16, and each of the 255 terms 32 (2^20 / M)^2 = 2^15 behind it is half a spacing
    and was rounded away -- 2^23 of 2^40 missing, 2^-17 of the variance.  (At M = 8192 the terms are 2^19 and survive; at
    M = 32769 the chunks have 64 rows and the terms are 2^16.)"""
    if fold == "separate":
        monkeypatch.setenv("FAIRREC_BN_FOLD_SEPARATE", "1")
    N = 100
    Z, at = D.planted(M, N)
    ones, zeros = torch.ones(N, device="cuda"), torch.zeros(N, device="cuda")
    Zd = _d(Z)
    Y, xh, inv, rm, rv = _bn_fwd(Zd, ones, zeros, 1e-5, 1.0, zeros, ones, 0, M, N)
    r = D.bn_fwd(Z, np.ones(N), np.zeros(N), 1e-5, 1.0, np.zeros(N), np.ones(N), 0)
    dZ, dg, db = _bn_bwd(Zd, Y, 0, xh, inv, ones, M, N)       # dY = the planted matrix: dbeta = 2^20 in every column
    _exact(f"fr_bn_bwd {fold} planted M={M} dbeta", db, np.full(N, D.PLANT))
    u_mean, u_inv = _ulps(rm.cpu().numpy(), np.full(N, D.PLANT / M)), _ulps(inv.cpu().numpy(), r.invstd)
    print(f"fr_bn_fwd {fold} planted M={M}: running_mean off by {u_mean:.3g} ulp, invstd by {u_inv:.3g} ulp")
    assert u_mean <= 4, u_mean
    assert u_inv <= 4, u_inv


def _pattern(M, N, p, seed, offset, counter_value):
    """the keep-scales fr_dropout_apply gives on ones"""
    ctr = torch.tensor([counter_value, 0], dtype=torch.int64, device="cuda")
    ones = torch.ones(M * N, device="cuda")
    out = torch.empty_like(ones)
    rc = _lib().fr_dropout_apply(ones.data_ptr(), M * N, p, seed, offset, ctr.data_ptr(), None, None, out.data_ptr(), _st())
    assert rc == 0
    return out.view(M, N)


@pytest.mark.parametrize("fold", ["inline", "separate"])
def test_batchnorm_forward_with_dropout(fold, monkeypatch):
    """fr_bn_fwd_drop and fr_bn_fwd_ex(Yd): Y, xhat and the statistics as without dropout (bit for bit), Yd = Y times the
    pattern fr_dropout_apply draws with the same seed, offset and counter (bit for bit), the used / tick protocol of
    tests/test_dropout_hip.py, num_batches_tracked moved by `passes`; a misaligned tensor and N = 6 refused"""
    if fold == "separate":
        monkeypatch.setenv("FAIRREC_BN_FOLD_SEPARATE", "1")
    lib = _lib()
    p, seed, offset = 0.5, 77, 64
    for M in (1, 33, 257):
        for N in (4, 36, 100):
            for entry in ("fr_bn_fwd_drop", "fr_bn_fwd_ex"):
                c = D.bn_case(M, N, seed=N)
                Zd, gd, bd = _d(c.Z), _d(c.gamma), _d(c.beta)
                plain = _bn_fwd(Zd, gd, bd, c.eps, c.momentum, _d(c.rmean), _d(c.rvar), 2, M, N)
                o = _Outs()
                Y, xh, Yd, inv, rm, rv = o.new(M, N), o.new(M, N), o.new(M, N), o.new(N), o.new(N), o.new(N)
                rm.copy_(_d(c.rmean))
                rv.copy_(_d(c.rvar))
                state = torch.tensor([41, 0], dtype=torch.int64, device="cuda")
                used = torch.zeros(1, dtype=torch.int64, device="cuda")
                nbt = torch.full((1,), 5, dtype=torch.int64, device="cuda")
                ws = _ws(lib.fr_bn_workspace_bytes(M, N))
                head = (Zd.data_ptr(), gd.data_ptr(), bd.data_ptr(), c.eps, c.momentum, rm.data_ptr(), rv.data_ptr(), M, N, 2, Y.data_ptr(),
                        xh.data_ptr(), inv.data_ptr(), ws.data_ptr(), ws.numel())
                drop = (Yd.data_ptr(), p, seed, offset, state.data_ptr(), used.data_ptr(), state.data_ptr())
                if entry == "fr_bn_fwd_drop":
                    rc = lib.fr_bn_fwd_drop(*head, *drop, _st())
                else:
                    rc = lib.fr_bn_fwd_ex(*head, 0, *drop, nbt.data_ptr(), 3, _st())
                assert rc == 0 and o.ok(), (rc, entry, M, N)
                assert int(used.item()) == 41 and state.cpu().tolist() == [42, 0], (entry, M, N)
                assert entry == "fr_bn_fwd_drop" or int(nbt.item()) == 8
                for a, b in zip((Y, xh, inv, rm, rv), plain):
                    assert _bits(a, b), (entry, M, N)
                assert _bits(Yd, Y * _pattern(M, N, p, seed, offset, 41)), (entry, M, N)
    # refusals: N % 4 != 0, a tensor that is not 16-byte aligned
    M, N = 8, 8
    z = torch.zeros(M * N + 4, device="cuda")
    t = lambda: torch.zeros(M * N, device="cuda")
    Y, xh, Yd, inv, g, b = t(), t(), t(), t(), t(), t()
    state = torch.zeros(2, dtype=torch.int64, device="cuda")
    ws = _ws(lib.fr_bn_workspace_bytes(M, N))
    for Zp, n in ((z[1:], 8), (z, 6)):
        rc = lib.fr_bn_fwd_drop(Zp.data_ptr(), g.data_ptr(), b.data_ptr(), 1e-5, 0.1, None, None, M, n, 0, Y.data_ptr(), xh.data_ptr(),
                                inv.data_ptr(), ws.data_ptr(), ws.numel(), Yd.data_ptr(), p, seed, 0, state.data_ptr(), None, None, _st())
        assert rc == EINVAL
        rc = lib.fr_bn_fwd_ex(Zp.data_ptr(), g.data_ptr(), b.data_ptr(), 1e-5, 0.1, None, None, M, n, 0, Y.data_ptr(), xh.data_ptr(),
                              inv.data_ptr(), ws.data_ptr(), ws.numel(), 0, Yd.data_ptr(), p, seed, 0, state.data_ptr(), None, None, None,
                              0, _st())
        assert rc == EINVAL


def _bn_both_ways(c, act, M, N):
    """fr_bn_fwd and fr_bn_bwd on the case's data: every output, on the host"""
    Zd, gd, bd, dYd = _d(c.Z), _d(c.gamma), _d(c.beta), _d(c.dY)
    Y, xh, inv, rm, rv = _bn_fwd(Zd, gd, bd, c.eps, c.momentum, _d(c.rmean), _d(c.rvar), act, M, N)
    dZ, dg, db = _bn_bwd(dYd, Y, act, xh, inv, gd, M, N)
    return dict(Y=Y.cpu(), xhat=xh.cpu(), invstd=inv.cpu(), running_mean=rm.cpu(), running_var=rv.cpu(),
                dZ=torch.from_numpy(dZ), dgamma=torch.from_numpy(dg), dbeta=torch.from_numpy(db))


def _bn_drop_outputs(c, M, N):
    """fr_bn_fwd_ex with the next layer's dropout (p = 0.5, counter 41): every output, on the host"""
    lib = _lib()
    Zd, gd, bd = _d(c.Z), _d(c.gamma), _d(c.beta)
    o = _Outs()
    Y, xh, Yd, inv, rm, rv = o.new(M, N), o.new(M, N), o.new(M, N), o.new(N), o.new(N), o.new(N)
    rm.copy_(_d(c.rmean))
    rv.copy_(_d(c.rvar))
    state = torch.tensor([41, 0], dtype=torch.int64, device="cuda")
    ws = _ws(lib.fr_bn_workspace_bytes(M, N))
    rc = lib.fr_bn_fwd_ex(Zd.data_ptr(), gd.data_ptr(), bd.data_ptr(), c.eps, c.momentum, rm.data_ptr(), rv.data_ptr(), M, N, 2,
                          Y.data_ptr(), xh.data_ptr(), inv.data_ptr(), ws.data_ptr(), ws.numel(), 0, Yd.data_ptr(), 0.5, 77, 64,
                          state.data_ptr(), None, None, None, 0, _st())
    assert rc == 0 and o.ok(), (rc, M, N)
    return dict(Y=Y.cpu(), xhat=xh.cpu(), Yd=Yd.cpu(), invstd=inv.cpu(), running_mean=rm.cpu(), running_var=rv.cpu())


@pytest.mark.parametrize("M", [1, 33, 8192, 8193, 32769])
def test_batchnorm_fold_forms_agree(M, monkeypatch):
    """The fold inside the apply launch and the fold launch of its own run the same device functions (bn_fold_stats_inline,
    bn_fold_sums_inline), so every output of fr_bn_fwd and fr_bn_bwd -- Y, xhat, invstd, both running statistics, dZ, dgamma,
    dbeta -- and Yd of fr_bn_fwd_ex with dropout must be EQUAL between the two forms, bit for bit.  M = 8192 is the last batch
    whose quarter of the chunks (64 of 256) is held in registers, 8193 the first that walks them in a loop, 32769 has 64-row
    chunks; N = 1, 65, 100: a lone column, a second column block of one column, a ragged one."""
    cases = [(N, act) for N in (1, 65, 100) for act in (0, 2)]
    got = {}
    for fold in ("inline", "separate"):
        if fold == "separate":
            monkeypatch.setenv("FAIRREC_BN_FOLD_SEPARATE", "1")
        got[fold] = [_bn_both_ways(D.bn_case(M, N, seed=act), act, M, N) for N, act in cases]
        if M == 33:
            got[fold].append(_bn_drop_outputs(D.bn_case(33, 36, seed=36), 33, 36))
    for i, (a, b) in enumerate(zip(got["inline"], got["separate"])):
        for name in a:
            assert _bits(a[name], b[name]), (M, cases[i] if i < len(cases) else "dropout [33, 36]", name)


# ---- statistics from a product's epilogue -----------------------------------------------------------------------------------

@pytest.mark.parametrize("N,k0,k1", [(8, 32, 0), (40, 64, 32), (65, 32, 0)])
@pytest.mark.parametrize("M", [1, 33, 4097, 32768])
def test_forward_statistics_epilogue(M, N, k0, k1):
    """fr_linear_fwd_bnstats + fr_bn_fwd_ex(have_stats = 1): Z against the float64 product of the INPUTS, and Y, xhat, invstd and
    the running statistics against the float64 BatchNorm of that product, the product's bound carried through"""
    lib = _lib()
    c = D.real_case(M, k0, k1, N)
    d = _Dev(c)
    b = D.bn_case(M, N)
    z, ez = D.product(D.cat(c.x0, c.x1), c.W, c.b)
    o = _Outs()
    Z, Y, xh, inv, rm, rv = o.new(M, N), o.new(M, N), o.new(M, N), o.new(N), o.new(N), o.new(N)
    rm.copy_(_d(b.rmean))
    rv.copy_(_d(b.rvar))
    ws = _ws(lib.fr_bn_workspace_bytes(M, N))
    rc = lib.fr_linear_fwd_bnstats(d.x0.data_ptr(), k0, _ptr(d.x1), k1, d.W.data_ptr(), d.b.data_ptr(), M, N, Z.data_ptr(), ws.data_ptr(),
                                   ws.numel(), _st())
    assert rc == 0 and o.ok(), rc
    tag = f"fr_linear_fwd_bnstats M={M} N={N} k={k0}+{k1}"
    _within(tag + " Z", Z.cpu().numpy(), z, ez)
    nbt = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    gd, bd = _d(b.gamma), _d(b.beta)
    rc = lib.fr_bn_fwd_ex(Z.data_ptr(), gd.data_ptr(), bd.data_ptr(), b.eps, b.momentum, rm.data_ptr(), rv.data_ptr(), M, N, 2, Y.data_ptr(),
                          xh.data_ptr(), inv.data_ptr(), ws.data_ptr(), ws.numel(), 1, None, 0.0, 0, 0, None, None, None, nbt.data_ptr(), 2,
                          _st())
    assert rc == 0 and o.ok() and int(nbt.item()) == 7, rc
    _check_bn_fwd_outputs("fr_bn_fwd_ex(have_stats) after " + tag, (Y, xh, inv, rm, rv),
                          D.bn_fwd(z, b.gamma, b.beta, b.eps, b.momentum, b.rmean, b.rvar, 2, e_in=ez))


def test_forward_statistics_epilogue_refuses_64_row_chunks():
    lib = _lib()
    M, N, K = 32769, 8, 32
    x, W, Z = torch.zeros(M, K, device="cuda"), torch.zeros(N, K, device="cuda"), torch.zeros(M, N, device="cuda")
    ws = _ws(lib.fr_bn_workspace_bytes(M, N))
    assert lib.fr_linear_fwd_bnstats(x.data_ptr(), K, None, 0, W.data_ptr(), None, M, N, Z.data_ptr(), ws.data_ptr(), ws.numel(),
                                     _st()) == EUNSUPPORTED
    assert lib.fr_linear_bwd_input_bnstats(Z.data_ptr(), W.data_ptr(), M, 32, 32, x.data_ptr(), x.data_ptr(), x.data_ptr(), 0, ws.data_ptr(),
                                           _lib().fr_bn_workspace_bytes(M, 32), 0.0, 0, 0, None, _st()) in (EUNSUPPORTED, EINVAL)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("N,K", [(32, 32), (64, 96)])
@pytest.mark.parametrize("M", [1, 33, 32768])
def test_backward_statistics_epilogue(M, N, K, p):
    """fr_linear_bwd_input_bnstats + fr_bn_bwd_ex(have_stats = 1): dX = (dY W) o keep against float64 (the pattern regenerated
    from seed, offset and the recorded counter), and dZ, dgamma, dbeta of the BatchNorm layer below against float64 of the
    inputs, the product's bound carried through.  Exact regime for dX and dbeta (act none below), real regime for all."""
    lib = _lib()
    seed, offset, counter = 91, 128, 17
    keep = _pattern(M, K, p, seed, offset, counter).cpu().numpy() if p else None
    used = torch.tensor([counter], dtype=torch.int64, device="cuda")
    for regime in ("exact", "real"):
        for act_b in ((0,) if regime == "exact" else (2, 4)):
            c = D.case(regime, M, K, 0, N, seed=act_b)
            d = _Dev(c)
            b = D.bn_case(M, K, seed=act_b)
            if regime == "exact":
                # the column sums run over the PRODUCT's entries: dY and xhat in -1 .. 1 keep sum_m |dX| |xhat| below 2^24
                c.dY = np.clip(c.dY, -1, 1)
                d = _Dev(c)
                xhat = np.random.default_rng(M).integers(-1, 2, (M, K)).astype(np.float32)
                Yb, invstd, gam = xhat, np.ones(K, np.float32), np.ones(K, np.float32)
                D.assert_exact(3 * N * (2 if p else 1), 1, M)
            else:
                r = D.bn_fwd(b.Z, b.gamma, b.beta, b.eps, b.momentum, b.rmean, b.rvar, act_b)
                xhat, Yb, invstd, gam = r.xhat.astype(np.float32), r.Y.astype(np.float32), r.invstd.astype(np.float32), b.gamma
            P, eP = D.product(c.dY, np.asarray(c.W, np.float64).T)
            dXr, eX = (P * keep, eP * keep + D.gamma(1) * np.abs(P * keep)) if p else (P, eP)
            o = _Outs()
            dX = o.new(M, K)
            Ybd, xhd, invd, gd = _d(Yb), _d(xhat), _d(invstd), _d(gam)
            ws = _ws(lib.fr_bn_workspace_bytes(M, K))
            rc = lib.fr_linear_bwd_input_bnstats(d.dY.data_ptr(), d.W.data_ptr(), M, N, K, dX.data_ptr(), Ybd.data_ptr(), xhd.data_ptr(), act_b,
                                                 ws.data_ptr(), ws.numel(), p, seed, offset, used.data_ptr() if p else None, _st())
            assert rc == 0 and o.ok(), rc
            tag = f"fr_linear_bwd_input_bnstats {regime} M={M} N={N} K={K} p={p} act_b={act_b}"
            _check(tag + " dX", regime, dX.cpu().numpy(), dXr, eX)
            dZ, dg, db = _bn_bwd(dX, Ybd, act_b, xhd, invd, gd, M, K, have_stats=1, ws=ws)
            q = D.bn_bwd(dXr, Yb, act_b, xhat, invstd, gam, e_in=None if regime == "exact" else eX)
            tag = "fr_bn_bwd_ex(have_stats) after " + tag
            if regime == "exact":
                _exact(tag + " dbeta", db, q.dbeta)
                _exact(tag + " dgamma", dg, q.dgamma)
            else:
                _within(tag + " dbeta", db, q.dbeta, q.e_dbeta)
                _within(tag + " dgamma", dg, q.dgamma, q.e_dgamma)
            _within(tag + " dZ", dZ, q.dZ, q.e_dZ)

"""GPU: the FairGo graph kernels (csrc/graph.hip, csrc/frontier.hip) one by one through the C ABI against tests/graph_ref.py.

Every tolerance here is derived, none is measured (u = 2^-24, gamma_n = n u / (1 - n u)):
  * a row of fr_spmm_csr_sel is a chain of n fmaf steps in CSR order: |got - float64| <= gamma_(n+1) * sum |val x|, n the
    number of kept terms, the one extra step for the float64 reference's own rounding; a row without a term is exactly 0;
  * through an activation (fr_spmm_csr_sel_act) one multiplication more: gamma_(n+2) * sum |val x| * |act'|, the derivative
    exact in float32 because the activation's outputs sit on a dyadic grid (graph_ref.act_grid);
  * fr_row_scatter_sum adds a row's members one by one in ascending position: EQUAL to the float32 emulation of that order,
    and within gamma_n * sum |g| of float64 as the independent check;
  * everything else is an identity the header states: bit for bit.
Output buffers sit between 64 canary floats and are prefilled with NaN, so a row that is not written and a write outside
the buffer both show.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import graph_ref as R

pytestmark = pytest.mark.gpu

CANARY = 1234.5
PAD = 64
ACTS = [R.ACT_RELU, R.ACT_LEAKY, R.ACT_SIGMOID, R.ACT_TANH]
ENV_ROWWISE, ENV_RUN_ROWS = "FAIRREC_SPMM_SEL_ROWWISE", "FAIRREC_SEL_RUNS_ROWS"


def _lib():
    from fairrec import _C
    return _C.lib()


def _st():
    from fairrec import _C
    return _C.current_stream()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _framed(n, fill=float("nan"), dtype=torch.float32, off=0, canary=CANARY):
    """(whole, view): `view` = n elements prefilled with `fill`, PAD + off canary elements in front of it and PAD behind"""
    whole = torch.full((PAD + off + n + PAD,), canary, dtype=dtype, device="cuda")
    view = whole[PAD + off:PAD + off + n]
    view.fill_(fill)
    return whole, view


def _frame_intact(whole, n, off=0, canary=CANARY):
    return bool((whole[:PAD + off] == canary).all()) and bool((whole[PAD + off + n:] == canary).all())


def _same(a, b):
    """value equality that also holds NaN against NaN (torch.equal where neither side has one)"""
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and \
        torch.equal(torch.nan_to_num(a, nan=CANARY), torch.nan_to_num(b, nan=CANARY))


def _errflag():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


# ---- the shared graphs, maps and operands (host and device), built once -----------------------------------------------------

def _dev_graph(g):
    return SimpleNamespace(indptr=_dev(g.indptr), col=_dev(g.col), val=_dev(g.val), n_rows=g.n_rows, n_cols=g.n_cols)


@functools.lru_cache(maxsize=None)
def _graph(name):
    g = R.graph_a() if name == "a" else R.graph_b()
    return g, _dev_graph(g), R.maps_for(g.n_cols, 0.3 if name == "a" else 0.02)


@functools.lru_cache(maxsize=None)
def _case(name, n_out, mname, D):
    """graph `name` cut to its first n_out rows, the column map `mname` (None: no map) and a compact operand X for it"""
    g, dg, maps = _graph(name)
    if n_out != g.n_rows:
        g = R.head_rows(g, n_out)
        dg = SimpleNamespace(indptr=dg.indptr[:n_out + 1], col=dg.col, val=dg.val, n_rows=n_out, n_cols=g.n_cols)
    m = None if mname is None else maps[mname]
    n_x = g.n_cols if m is None else int((m >= 0).sum())
    rng = np.random.default_rng([D, n_x, len(name)])
    X = R.normals(rng, (max(n_x, 1), D))
    c = SimpleNamespace(g=g, dg=dg, m=m, X=X, D=D, dX=_dev(X), dm=None, dbits=None)
    if m is not None:
        c.dm, c.dbits = _dev(m), _dev(R.map_bits(m).view(np.int32))
    c.dW = _dev(R.whole_table(X, m, g.n_cols))
    return c


@functools.lru_cache(maxsize=None)
def _ref(name, n_out, mname, D, with_rows):
    c = _case(name, n_out, mname, D)
    return R.spmm_sel_ref(c.g, c.X, R.rows_a() if with_rows else None, c.m)


def _sel(c, rows=None, bits=True, act=None, expect_ok=True, n_out=None, fill=float("nan")):
    """fr_spmm_csr_sel (act = (act_src tensor, code, skip words or None): fr_spmm_csr_sel_act) -> Y [n_out, D], canaries checked"""
    n = (c.dg.n_rows if rows is None else rows.numel()) if n_out is None else n_out
    whole, flat = _framed(max(n, 1) * c.D, fill)
    head = (c.dg.indptr.data_ptr(), c.dg.col.data_ptr(), c.dg.val.data_ptr(), c.dX.data_ptr(), _ptr(rows), n, _ptr(c.dm),
            _ptr(c.dbits) if bits else 0, c.D, flat.data_ptr())
    if act is None:
        rc = _lib().fr_spmm_csr_sel(*head, _st())
    else:
        rc = _lib().fr_spmm_csr_sel_act(*head, act[0].data_ptr(), act[1], _ptr(act[2]), _st())
    torch.cuda.synchronize()
    assert _frame_intact(whole, max(n, 1) * c.D), "written outside Y"
    if expect_ok:
        assert rc == 0, rc
        return flat[:n * c.D].view(n, c.D)
    return rc, flat


def _spmm(dg, dW, D):
    whole, flat = _framed(dg.n_rows * D)
    rc = _lib().fr_spmm_csr(dg.indptr.data_ptr(), dg.col.data_ptr(), dg.val.data_ptr(), dW.data_ptr(), dg.n_rows, D, flat.data_ptr(), _st())
    torch.cuda.synchronize()
    assert rc == 0 and _frame_intact(whole, dg.n_rows * D)
    return flat.view(dg.n_rows, D)


def _act_bwd(dY, Y, act):
    """fr_act_bwd on tensors of any size (the entry point takes multiples of 4 floats: zero padded here)"""
    n = dY.numel()
    n4 = (n + 3) // 4 * 4
    a, b, o = (torch.zeros(n4, dtype=torch.float32, device="cuda") for _ in range(3))
    a[:n], b[:n] = dY.reshape(-1), Y.reshape(-1)
    rc = _lib().fr_act_bwd(a.data_ptr(), b.data_ptr(), act, n4, o.data_ptr(), _st())
    torch.cuda.synchronize()
    assert rc == 0
    return o[:n].view(dY.shape)


def _assert_bound(got, ref, absref, n, steps, scale=None, rows=None, what=""):
    """|got - ref * scale| <= gamma_(n + steps) * absref * |scale| elementwise (n per row), on `rows` (all)"""
    got = got.double().cpu().numpy()
    bound = R.gamma(n + steps)[:, None] * absref
    if scale is not None:
        ref, bound = ref * scale, bound * np.abs(scale)
    err = np.abs(got - ref)
    bad = ~(err <= bound)          # (a NaN is bad)
    if rows is not None:
        bad = bad[rows]
    assert not bad.any(), "%s: %d elements outside the bound, worst excess %.3g" % (what, bad.sum(), np.nanmax((err - bound)))


# ---- A. fr_spmm_csr_sel, one wave per row -----------------------------------------------------------------------------------

@pytest.mark.parametrize("mname", [None, "some", "all", "none", "one"])
@pytest.mark.parametrize("with_rows", [False, True], ids=["all_rows", "rows37"])
@pytest.mark.parametrize("D", [1, 16, 64, 100, 128, 256])
def test_sel_rowwise_against_float64_and_the_whole_table_product(D, with_rows, mname):
    c = _case("a", R.A_ROWS, mname, D)
    rows = R.rows_a() if with_rows else None
    drows = _dev(rows) if with_rows else None
    ref, absref, kept = _ref("a", R.A_ROWS, mname, D, with_rows)
    Y = _sel(c, drows, bits=False)
    _assert_bound(Y, ref, absref, kept, 1, what="fr_spmm_csr_sel")
    assert bool((Y[_dev(kept == 0)] == 0).all())
    whole = _spmm(c.dg, c.dW, D)
    assert torch.equal(Y, whole[drows.long()] if with_rows else whole)
    if mname is not None:
        assert torch.equal(Y, _sel(c, drows, bits=True))


@pytest.mark.parametrize("with_rows", [False, True])
def test_sel_of_no_rows_writes_nothing(with_rows):
    c = _case("a", R.A_ROWS, "some", 64)
    rc, flat = _sel(c, _dev(R.rows_a()) if with_rows else None, expect_ok=False, n_out=0, fill=7.0)
    assert rc == 0 and bool((flat == 7.0).all())


def test_sel_refuses_a_bitmap_without_its_map():
    c = _case("a", R.A_ROWS, "some", 64)
    bare = SimpleNamespace(dg=c.dg, dX=c.dW, dm=None, dbits=c.dbits, D=64)
    rc, flat = _sel(bare, None, bits=True, expect_ok=False, fill=7.0)
    assert rc != 0 and bool((flat == 7.0).all())


# ---- B. fr_spmm_csr_sel, one wave per run of rows ---------------------------------------------------------------------------

def _assert_runs_structure(g):
    """the row structures a runs kernel can get wrong are in the graph (from indptr)"""
    ip = g.indptr
    n = np.diff(ip)
    assert ip[8] == ip[0]                                              # a run of 8 empty rows: j0 == j1
    assert n[8:16].tolist() == [256, 257, 600, 0, 0, 1, 0, 700]        # one trip exactly, one over, three trips, full width
    assert n[16:24].tolist() == [0, 1, 0, 255, 0, 1, 0, 0] and ip[20] - ip[16] == 256      # trip ends on a row boundary
    assert n[24:32].tolist() == [32] * 8                               # a run that is one trip
    assert g.n_rows < R.B_ROWS or (n[-1] > 0 and ip[-1] == len(g.col))      # the last row ends the arrays


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("mname", ["all", "none", "some", "one"])
@pytest.mark.parametrize("n_out", [1037, 1024, 1023])
def test_sel_runs_against_float64_the_row_wise_kernel_and_the_whole_table_product(monkeypatch, n_out, mname, D):
    """n_out = 1037: four workgroups of 8-row runs plus a tail run of 5 (13 at 32 rows per wave); 1024 is the smallest
    n_out that takes the runs kernel, 1023 the largest the row-wise kernel takes."""
    monkeypatch.delenv(ENV_ROWWISE, raising=False)
    monkeypatch.delenv(ENV_RUN_ROWS, raising=False)
    c = _case("b", n_out, mname, D)
    _assert_runs_structure(c.g)
    ref, absref, kept = _ref("b", n_out, mname, D, False)
    Y = _sel(c, bits=True)
    assert not bool(torch.isnan(Y).any()), "a row of Y was not written"
    _assert_bound(Y, ref, absref, kept, 1, what="runs kernel")
    assert bool((Y[_dev(kept == 0)] == 0).all())
    assert torch.equal(Y, _sel(c, bits=False))
    assert torch.equal(Y, _spmm(c.dg, c.dW, D))
    for r in ("16", "32"):
        monkeypatch.setenv(ENV_RUN_ROWS, r)
        assert torch.equal(Y, _sel(c, bits=True)), "rows per wave " + r
        assert torch.equal(Y, _sel(c, bits=False)), "rows per wave %s, no bitmap" % r
    monkeypatch.delenv(ENV_RUN_ROWS)
    monkeypatch.setenv(ENV_ROWWISE, "1")
    assert torch.equal(Y, _sel(c, bits=True))


# ---- C. fr_spmm_csr_sel_act -------------------------------------------------------------------------------------------------

def _skip_cases(kept, n, rng, hand=()):
    """{name: bool [n] or None}: no bitmap, an empty one, 20 % at random, one reached and one unreached row (and `hand`)"""
    some = np.zeros(n, dtype=bool)
    some[[int(r[0]) for r in (np.nonzero(kept > 0)[0][::-1], np.nonzero(kept == 0)[0]) if len(r)] + list(hand)] = True
    return {"null": None, "empty": np.zeros(n, dtype=bool), "random": rng.random(n) < 0.2, "hand": some}


def _check_sel_act(c, drows, ref, absref, kept, act, hand=(), variants=()):
    """assertions C1-C3 for one (graph, map, rows, D, activation) over the skip cases"""
    n = len(kept)
    rng = np.random.default_rng([act, c.D, n])
    plain = _sel(c, drows)
    for kind in ("grid", "random"):
        src = (R.act_grid if kind == "grid" else R.act_random)(rng, (n, c.D), act)
        dsrc = _dev(src)
        through = _act_bwd(plain, dsrc, act)           # what the whole-table pass of fr_act_bwd makes of the plain product
        dact = R.act_bwd_ref(src, act)
        for name, skip in _skip_cases(kept, n, rng, hand).items():
            if kind == "random" and name != "random":
                continue
            what = "act %d, %s act_src, skip %s" % (act, kind, name)
            dskip = None if skip is None else _dev(R.bits_of(np.nonzero(skip)[0], n).view(np.int32))
            skipped = _dev(np.zeros(n, dtype=bool) if skip is None else skip)
            Y = _sel(c, drows, act=(dsrc, act, dskip))
            assert torch.equal(Y[skipped], plain[skipped]), what + ": a skipped row differs from the plain product"
            assert torch.equal(Y, torch.where(skipped[:, None], plain, through)), what + ": not the three-pass result"
            if kind == "grid":
                live = np.zeros(n, dtype=bool) if skip is None else skip
                _assert_bound(Y, ref, absref, kept, 2, scale=dact, rows=~live, what=what)
            if c.dm is not None:
                assert torch.equal(Y, _sel(c, drows, bits=False, act=(dsrc, act, dskip))), what + ": differs without map_bits"
            for setenv in variants:
                with pytest.MonkeyPatch.context() as mp:
                    mp.setenv(*setenv)
                    assert torch.equal(Y, _sel(c, drows, act=(dsrc, act, dskip))), what + ", %s=%s" % setenv


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("with_rows,mname", [(False, None), (True, None), (False, "some"), (True, "some"), (False, "all"),
                                             (False, "none"), (True, "one")],
                         ids=["plain", "rows37", "map", "rows37_map", "map_all", "map_none", "rows37_map_one"])
@pytest.mark.parametrize("D", [1, 16, 64, 100, 128, 256])
def test_sel_act_rowwise(D, with_rows, mname, act):
    c = _case("a", R.A_ROWS, mname, D)
    ref, absref, kept = _ref("a", R.A_ROWS, mname, D, with_rows)
    _check_sel_act(c, _dev(R.rows_a()) if with_rows else None, ref, absref, kept, act)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("mname", ["all", "none", "some", "one"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_sel_act_runs(monkeypatch, D, mname, act):
    """... skip bits also on the rows that span several trips (10, 15) and on the last row of the tail run"""
    monkeypatch.delenv(ENV_ROWWISE, raising=False)
    monkeypatch.delenv(ENV_RUN_ROWS, raising=False)
    c = _case("b", R.B_ROWS, mname, D)
    ref, absref, kept = _ref("b", R.B_ROWS, mname, D, False)
    _check_sel_act(c, None, ref, absref, kept, act, hand=(10, 15, R.B_ROWS - 1),
                   variants=((ENV_RUN_ROWS, "16"), (ENV_RUN_ROWS, "32"), (ENV_ROWWISE, "1")))


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("name,D", [("a", 64), ("a", 100), ("b", 64)], ids=["rowwise_d64", "rowwise_d100", "runs_d64"])
def test_sel_act_stores_zeros_at_unreached_rows_without_reading_act_src(monkeypatch, name, D, act):
    """The header: "a row no term reaches is stored as zeros without reading act_src".  NaN at the act_src of every such row
    (0 * act'(NaN) would be NaN through the sigmoid and tanh): Y holds exact zeros there, the other rows are unchanged."""
    monkeypatch.delenv(ENV_ROWWISE, raising=False)
    monkeypatch.delenv(ENV_RUN_ROWS, raising=False)
    n = R.A_ROWS if name == "a" else R.B_ROWS
    c = _case(name, n, "some", D)
    _, _, kept = _ref(name, n, "some", D, False)
    rng = np.random.default_rng([act, D])
    src = R.act_grid(rng, (n, D), act)
    clean = _sel(c, act=(_dev(src), act, None))
    src[kept == 0] = np.nan
    assert (kept == 0).sum() > 10 and (kept > 0).sum() > 10
    for dskip in (None, torch.zeros((n + 31) // 32, dtype=torch.int32, device="cuda")):
        Y = _sel(c, act=(_dev(src), act, dskip))
        assert bool((Y[_dev(kept == 0)] == 0).all()), "an unreached row is not zeros: %d NaN" % int(torch.isnan(Y).sum())
        assert torch.equal(Y, clean)


def test_sel_act_refuses_a_misaligned_act_src_and_an_unknown_activation():
    c = _case("a", R.A_ROWS, "some", 64)
    src = torch.zeros(R.A_ROWS * 64 + 4, dtype=torch.float32, device="cuda")
    assert src.data_ptr() % 16 == 0
    for off, act in ((1, R.ACT_TANH), (2, R.ACT_RELU), (0, 0), (0, 5), (0, -1)):
        rc, flat = _sel(c, act=(src[off:], act, None), expect_ok=False, fill=7.0)
        assert rc != 0 and bool((flat == 7.0).all()), (off, act)
    assert _sel(c, act=(src[4:], R.ACT_TANH, None)).shape == (R.A_ROWS, 64)      # 16 bytes on: accepted


# ---- D. fr_row_gather, fr_row_scatter_sum / _add / _add_act -----------------------------------------------------------------

@pytest.mark.parametrize("n_rows", [1, 977])
@pytest.mark.parametrize("M", [1, 5, 1025])
@pytest.mark.parametrize("D", [1, 63, 64, 65, 256, 300])
def test_row_gather_is_exact(D, M, n_rows):
    rng = np.random.default_rng([D, M, n_rows])
    X = _dev(R.normals(rng, (n_rows, D)))
    idx = _dev(rng.integers(0, n_rows, M))
    idx[-1] = n_rows - 1
    whole, out = _framed(M * D)
    err = _errflag()
    rc = _lib().fr_row_gather(X.data_ptr(), idx.data_ptr(), M, n_rows, D, out.data_ptr(), err.data_ptr(), _st())
    torch.cuda.synchronize()
    assert rc == 0 and int(err) == 0 and _frame_intact(whole, M * D)
    assert torch.equal(out.view(M, D), X[idx])


def test_row_gather_flags_ids_outside_the_table():
    rng = np.random.default_rng(11)
    n_rows, M, D = 50, 40, 65
    X = _dev(R.normals(rng, (n_rows, D)))
    idx = rng.integers(0, n_rows, M)
    idx[[3, 17]] = [n_rows, -5]
    ok = _dev((idx >= 0) & (idx < n_rows))
    didx = _dev(idx)
    whole, out = _framed(M * D)
    err = _errflag()
    rc = _lib().fr_row_gather(X.data_ptr(), didx.data_ptr(), M, n_rows, D, out.data_ptr(), err.data_ptr(), _st())
    torch.cuda.synchronize()
    from fairrec import _C
    assert rc == 0 and int(err) & _C.DEV_ERR_INDEX_RANGE and _frame_intact(whole, M * D)
    assert torch.equal(out.view(M, D)[ok], X[didx[ok]])


def _scatter(kind, g, idx, n_rows, D, dX, act_src=None, act=0, err=None, M=None):
    """fr_row_scatter_<kind> into the flat float view dX; returns the return code"""
    M = idx.numel() if M is None else M
    nb = _lib().fr_row_scatter_workspace_bytes(M)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda")
    head = (g.data_ptr(), idx.data_ptr(), M, n_rows, D, dX.data_ptr(), ws.data_ptr(), nb)
    if kind == "add_act":
        rc = _lib().fr_row_scatter_add_act(*head, act_src.data_ptr(), act, _ptr(err), _st())
    else:
        rc = getattr(_lib(), "fr_row_scatter_" + kind)(*head, _ptr(err), _st())
    torch.cuda.synchronize()
    return rc


SCATTER_SHAPES = [(1, 1, 1), (64, 7, 3), (65, 5000, 64), (2049, 300, 100), (16384, 7, 256), (16384, 10 ** 5, 64)]


@functools.lru_cache(maxsize=None)
def _scatter_case(M, n_rows, D):
    """gradient rows, ids drawn from four fifths of the rows of a table of ten or more (the others have no member) and both
    references"""
    rng = np.random.default_rng([M, n_rows, D])
    g = R.normals(rng, (M, D))
    live = np.sort(rng.choice(n_rows, n_rows * 4 // 5 if n_rows >= 10 else n_rows, replace=False))
    idx = live[rng.integers(0, len(live), M)]
    s32, touched = R.scatter_f32(g, idx, n_rows)
    return SimpleNamespace(g=g, idx=idx, s32=s32, touched=touched, ref=R.scatter_ref(g, idx, n_rows), rng=rng)


@pytest.mark.parametrize("M,n_rows,D", SCATTER_SHAPES)
def test_row_scatter_sum_and_add_in_ascending_position(M, n_rows, D):
    """(16384, 7, 256): segments of about 2300 members, where any other order of the additions gives other bits."""
    c = _scatter_case(M, n_rows, D)
    g, idx, err = _dev(c.g), _dev(c.idx), _errflag()
    whole, dX = _framed(n_rows * D)
    assert _scatter("sum", g, idx, n_rows, D, dX, err=err) == 0 and int(err) == 0 and _frame_intact(whole, n_rows * D)
    got = dX.view(n_rows, D)
    assert torch.equal(got, _dev(c.s32))
    S, absS, members = c.ref
    _assert_bound(got, S, absS, members, 0, what="fr_row_scatter_sum")
    assert bool((got[_dev(~c.touched)] == 0).all())
    prior = R.normals(np.random.default_rng(M + D), (n_rows, D))
    want, _ = R.scatter_f32(c.g, c.idx, n_rows, prior)
    whole, dX = _framed(n_rows * D)
    dX.copy_(_dev(prior).view(-1))
    assert _scatter("add", g, idx, n_rows, D, dX, err=err) == 0 and int(err) == 0 and _frame_intact(whole, n_rows * D)
    assert torch.equal(dX.view(n_rows, D), _dev(want))
    # n - 1 additions in the segment and one to the prior value: n roundings, one step to spare
    _assert_bound(dX.view(n_rows, D), prior.astype(np.float64) + S, np.abs(prior.astype(np.float64)) + absS, members, 1, what="_add")


@pytest.mark.parametrize("n_rows,D", [(1, 1), (2, 1), (3, 1), (5, 1), (6, 4), (7, 3), (11, 2), (23, 1), (300, 7), (13, 77), (150, 7),
                                      (301, 7)])
@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_row_scatter_sum_clears_unaligned_heads_and_tails(off, n_rows, D):
    """zero_fill_kernel stores float4 over the 16-byte aligned middle of dX and single floats before and behind it: dX starts
    0 .. 3 floats past a 16-byte boundary and holds 1, 2, 3 and 5 floats, 4 k + 0 .. 3 floats inside one workgroup (24, 21, 22,
    23) and over several (2100, 1001, 1050, 2107)."""
    n = n_rows * D
    rng = np.random.default_rng([n_rows, D])
    idx = np.array([n_rows - 1, 0, n_rows - 1])[:min(3, n_rows)]
    g = R.normals(rng, (len(idx), D))
    whole, dX = _framed(n, off=off)
    assert (dX.data_ptr() - 4 * off) % 16 == 0
    err = _errflag()
    assert _scatter("sum", _dev(g), _dev(idx), n_rows, D, dX, err=err) == 0 and int(err) == 0
    assert _frame_intact(whole, n, off=off), "written outside dX"
    assert bool(torch.isfinite(dX).all()), "%d elements of dX were not cleared" % int((~torch.isfinite(dX)).sum())
    want, touched = R.scatter_f32(g, idx, n_rows)
    assert torch.equal(dX.view(n_rows, D), _dev(want)) and not want[~touched].any()


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("M,n_rows,D", [(64, 7, 3), (65, 5000, 64), (2049, 300, 100), (16384, 7, 256)])
def test_row_scatter_add_act_scales_the_rows_it_adds_to_and_no_other(M, n_rows, D, act):
    c = _scatter_case(M, n_rows, D)
    rng = np.random.default_rng([M, D, act])
    prior = R.normals(rng, (n_rows, D))
    prior[~c.touched] = np.where(rng.random((int((~c.touched).sum()), 1)) < 0.5, np.nan, prior[~c.touched])
    src = R.act_grid(rng, (n_rows, D), act)
    added, touched = R.scatter_f32(c.g, c.idx, n_rows, prior)
    want = added.copy()
    want[touched] = added[touched] * R.act_bwd_ref(src, act).astype(np.float32)[touched]       # exact derivative, one rounding
    g, idx, dsrc, err = _dev(c.g), _dev(c.idx), _dev(src), _errflag()
    whole, dX = _framed(n_rows * D)
    dX.copy_(_dev(prior).view(-1))
    assert _scatter("add_act", g, idx, n_rows, D, dX, dsrc, act, err) == 0 and int(err) == 0 and _frame_intact(whole, n_rows * D)
    got = dX.view(n_rows, D)
    assert _same(got, _dev(want))
    assert _same(got[_dev(~touched)], _dev(prior)[_dev(~touched)])
    # ... and what fr_row_scatter_add followed by fr_act_bwd gives on the touched rows
    two = _dev(prior).clone()
    assert _scatter("add", g, idx, n_rows, D, two.view(-1), err=err) == 0
    assert _same(got, torch.where(_dev(touched)[:, None], _act_bwd(two, dsrc, act), two))


@pytest.mark.parametrize("act", ACTS)
def test_sel_act_then_scatter_add_act_equal_the_three_whole_table_passes(monkeypatch, act):
    """(L^T dY + scatter(g)) o act'(act_src): fr_frontier_mark -> fr_spmm_csr_sel_act -> fr_row_scatter_add_act against
    fr_spmm_csr_sel -> fr_row_scatter_add -> fr_act_bwd over the whole table, bit for bit, and against float64.  A row with n
    product terms and m scattered members takes at most n + m + 1 roundings (n fmaf, m - 1 additions of the segment, one
    addition of the two, one multiplication by the exact derivative): gamma_(n+m+2) with the reference's step."""
    monkeypatch.delenv(ENV_ROWWISE, raising=False)
    monkeypatch.delenv(ENV_RUN_ROWS, raising=False)
    n, D, M = R.B_ROWS, 64, 160
    c = _case("b", n, "some", D)
    ref, absref, kept = _ref("b", n, "some", D, False)
    rng = np.random.default_rng([act, 160])
    ids = rng.choice(n, M - 8, replace=False)
    ids = np.concatenate([ids, ids[:8]])[rng.permutation(M)]
    assert len(np.unique(ids)) == M - 8 and (kept[ids] == 0).any() and (kept[ids] > 0).any()
    g, src = R.normals(rng, (M, D)), R.act_grid(rng, (n, D), act)
    dg, dids, dsrc, err = _dev(g), _dev(ids), _dev(src), _errflag()
    skip = torch.zeros((n + 31) // 32, dtype=torch.int32, device="cuda")
    assert _lib().fr_frontier_mark(dids.data_ptr(), M, n, skip.data_ptr(), err.data_ptr(), _st()) == 0
    fused = _sel(c, act=(dsrc, act, skip)).clone()
    assert _scatter("add_act", dg, dids, n, D, fused.view(-1), dsrc, act, err) == 0
    three = _sel(c).clone()
    assert _scatter("add", dg, dids, n, D, three.view(-1), err=err) == 0
    three = _act_bwd(three, dsrc, act)
    assert int(err) == 0 and torch.equal(fused, three)
    S, absS, members = R.scatter_ref(g, ids, n)
    _assert_bound(fused, ref + S, absref + absS, kept + members, 2, scale=R.act_bwd_ref(src, act), what="composition")


def test_row_scatter_ignores_the_padding_id():
    rng = np.random.default_rng(6)
    M, n_rows, D = 70, 9, 65
    g = R.normals(rng, (M, D))
    idx = rng.integers(0, n_rows, M)
    idx[[0, 13, 69]] = -1
    err = _errflag()
    whole, dX = _framed(n_rows * D)
    assert _scatter("sum", _dev(g), _dev(idx), n_rows, D, dX, err=err) == 0 and int(err) == 0 and _frame_intact(whole, n_rows * D)
    assert torch.equal(dX.view(n_rows, D), _dev(R.scatter_f32(g, idx, n_rows)[0]))


def test_row_scatter_flags_ids_outside_the_table_and_stays_inside_dX():
    from fairrec import _C
    rng = np.random.default_rng(7)
    M, n_rows, D = 70, 9, 65
    g = R.normals(rng, (M, D))
    idx = rng.integers(1, n_rows, M)
    idx[[5, 40]] = [n_rows, -5]
    for kind in ("sum", "add"):
        err = _errflag()
        whole, dX = _framed(n_rows * D, fill=0.0)
        assert _scatter(kind, _dev(g), _dev(idx), n_rows, D, dX, err=err) == 0
        assert int(err) & _C.DEV_ERR_INDEX_RANGE and _frame_intact(whole, n_rows * D)
        # the rows of the valid ids are their sums; the sort files a bad id under row 0 (csrc/sort_body.hpp: "r = 0" beside the
        # flag -- inside dX whatever the id was), so row 0, which no valid id of this list names, holds the bad members' rows
        # summed in position order.  The header promises the flag and nothing about row 0: a caller that sees the flag raises.
        assert torch.equal(dX.view(n_rows, D), _dev(R.scatter_f32(g, np.where((idx < 0) | (idx >= n_rows), 0, idx), n_rows)[0]))


def test_row_scatter_refuses_more_ids_than_the_sort_takes():
    from fairrec import _C
    M = _C.FR_SORT_MAX + 1
    g = torch.zeros(M, 1, device="cuda")
    idx = torch.zeros(M, dtype=torch.int64, device="cuda")
    src = torch.zeros(4, device="cuda")
    for kind in ("sum", "add", "add_act"):
        whole, dX = _framed(4, fill=7.0)
        assert _scatter(kind, g, idx, 4, 1, dX, src, R.ACT_RELU) != 0
        assert bool((dX == 7.0).all()) and _frame_intact(whole, 4)
    whole, dX = _framed(4, fill=7.0)
    assert _scatter("sum", g, idx, 4, 1, dX, M=_C.FR_SORT_MAX) == 0 and bool((dX == 0.0).all())


# ---- E. the frontier bitmaps ------------------------------------------------------------------------------------------------

IPAD = 0x5A5A5A5A


def _words(bits):
    return _framed(len(bits), 0, torch.int32, canary=IPAD)


def _np_bits(view):
    return view.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("n_rows", [1, 31, 32, 33, 8193])
def test_frontier_mark(n_rows):
    from fairrec import _C
    rng = np.random.default_rng(n_rows)
    before = R.bits_of(rng.integers(0, n_rows, max(1, n_rows // 7)), n_rows)
    ids = rng.integers(0, n_rows, 3 + n_rows // 3)
    ids = np.concatenate([ids, ids[:3], [n_rows - 1, 0]])
    whole, bits = _words(before)
    bits.copy_(_dev(before.view(np.int32)))
    err, dids = _errflag(), _dev(ids)
    assert _lib().fr_frontier_mark(dids.data_ptr(), 0, n_rows, bits.data_ptr(), err.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np_bits(bits), before)
    assert _lib().fr_frontier_mark(dids.data_ptr(), len(ids), n_rows, bits.data_ptr(), err.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    want = R.frontier_mark_ref(ids, n_rows, before)
    np.testing.assert_array_equal(_np_bits(bits), want)
    assert int(err) == 0 and _frame_intact(whole, len(before), canary=IPAD)
    for bad in (n_rows, -1, n_rows + 31, -(2 ** 40), 2 ** 40):
        dbad = _dev(np.array([bad], dtype=np.int64))
        err.zero_()
        assert _lib().fr_frontier_mark(dbad.data_ptr(), 1, n_rows, bits.data_ptr(), err.data_ptr(), _st()) == 0
        torch.cuda.synchronize()
        assert int(err) & _C.DEV_ERR_INDEX_RANGE, bad
        np.testing.assert_array_equal(_np_bits(bits), want)
        assert _frame_intact(whole, len(before), canary=IPAD)


def test_frontier_expand():
    """the listed rows of graph A: the 333-nonzero row (more than one nonzero per lane), empty rows, a row listed twice"""
    g, dg, _ = _graph("a")
    for rows, seed in (([6], []), ([0, 299], [5, 332]), ([12, 3, 12, 0, 40, 5, 299, 41, 42], [320]), (list(range(8, 299)), [])):
        before = R.bits_of(seed, g.n_cols)
        whole, bits = _words(before)
        bits.copy_(_dev(before.view(np.int32)))
        drows = _dev(np.array(rows, dtype=np.int32))
        args = (dg.indptr.data_ptr(), dg.col.data_ptr(), drows.data_ptr())
        assert _lib().fr_frontier_expand(*args, 0, bits.data_ptr(), _st()) == 0
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_np_bits(bits), before)
        assert _lib().fr_frontier_expand(*args, len(rows), bits.data_ptr(), _st()) == 0
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_np_bits(bits), R.frontier_expand_ref(g, rows, before))
        assert _frame_intact(whole, len(before), canary=IPAD)
    assert len(R.ids_of(R.frontier_expand_ref(g, [6], R.bits_of([], g.n_cols)), g.n_cols)) == g.n_cols


@pytest.mark.parametrize("fill", ["empty", "full", "random"])
@pytest.mark.parametrize("n_rows", [1, 31, 32, 33, 8193])
def test_frontier_count_and_scatter(n_rows, fill):
    rng = np.random.default_rng(n_rows)
    members = {"empty": np.zeros(0, dtype=np.int64), "full": np.arange(n_rows),
               "random": np.unique(np.concatenate([rng.integers(0, n_rows, 1 + n_rows // 3), [n_rows - 1]]))}[fill]
    host = R.bits_of(members, n_rows)
    nw = len(host)
    bits = _dev(host.view(np.int32))
    whole_c, count = _framed(nw, -3, torch.int32, canary=IPAD)
    assert _lib().fr_frontier_count(bits.data_ptr(), n_rows, count.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(count.cpu().numpy(), R.frontier_count_ref(host))
    assert _frame_intact(whole_c, nw, canary=IPAD)
    incl = torch.cumsum(count, 0, dtype=torch.int32)
    assert int(incl[-1]) == len(members)
    want_rows, want_pos = R.frontier_scatter_ref(host, n_rows)
    for prefill in (7, -7):       # (7 is a rank a row can have; -7 is nothing the kernel writes)
        whole_r, rows_out = _framed(len(members), -3, torch.int32, canary=IPAD)
        whole_p, pos = _framed(n_rows, prefill, torch.int32, canary=IPAD)
        out_ptr = whole_r.data_ptr() + PAD * 4       # (an empty view has no address of its own: the empty set's list starts here too)
        assert _lib().fr_frontier_scatter(bits.data_ptr(), incl.data_ptr(), n_rows, out_ptr, pos.data_ptr(), _st()) == 0
        torch.cuda.synchronize()
        got_rows, got_pos = rows_out.cpu().numpy(), pos.cpu().numpy()
        np.testing.assert_array_equal(got_rows, want_rows)
        np.testing.assert_array_equal(got_pos, want_pos)
        assert (np.diff(got_rows) > 0).all() and (got_pos[got_rows] == np.arange(len(members))).all()
        assert _frame_intact(whole_r, len(members), canary=IPAD) and _frame_intact(whole_p, n_rows, canary=IPAD)


# ---- F. fr_mse --------------------------------------------------------------------------------------------------------------

def _mse(pred, target):
    B = len(pred)
    nb = (B + 255) // 256
    ws = torch.empty(nb, dtype=torch.float32, device="cuda")
    loss = torch.full((1,), float("nan"), device="cuda")
    whole, dpred = _framed(B)
    dp, dt = _dev(pred), _dev(target)
    rc = _lib().fr_mse(dp.data_ptr(), dt.data_ptr(), B, loss.data_ptr(), dpred.data_ptr(), ws.data_ptr(), nb * 4, _st())
    torch.cuda.synchronize()
    assert rc == 0 and _frame_intact(whole, B)
    return loss.cpu().numpy()[0], dpred.cpu().numpy()


@pytest.mark.parametrize("B", [1, 255, 256, 257, 70001])
def test_mse_on_a_grid_where_every_sum_is_exact(B):
    """target in {1 .. 5}, pred a multiple of 0.5 in [0, 6]: the errors are multiples of 0.5 up to 5, their squares multiples
    of 0.25 up to 25 and every partial sum an integer number of quarters below 2^24 -- exact in float32 in ANY order.  So
    loss = float32(S) / float32(B) and dpred = float32(2 e) / float32(B), each to the one ulp of a division that need not be
    correctly rounded."""
    rng = np.random.default_rng(B)
    target = rng.integers(1, 6, B).astype(np.float32)
    pred = (rng.integers(0, 13, B) / 2.0).astype(np.float32)
    e = pred.astype(np.float64) - target
    S = float((e * e).sum())
    assert S * 4 < 2 ** 24 and S * 4 == int(S * 4)
    loss, dpred = _mse(pred, target)
    want = np.float32(S) / np.float32(B)
    assert abs(float(loss) - float(want)) <= float(np.spacing(want)), (loss, want)
    want_d = (2.0 * e).astype(np.float32) / np.float32(B)
    assert (np.abs(dpred.astype(np.float64) - want_d.astype(np.float64)) <= np.spacing(np.abs(want_d)).astype(np.float64)).all()
    assert (dpred[e == 0] == 0).all()


def test_mse_on_random_inputs_within_the_any_order_bound():
    """A sum of B non-negative terms, each a rounded square of a rounded difference, in any order, then one division: at most
    B + 2 roundings on any term's way into the result, |loss - ref| <= (B + 2) u ref."""
    B = 257
    rng = np.random.default_rng(257)
    pred, target = R.normals(rng, B) * 5, rng.integers(1, 6, B).astype(np.float32)
    loss, dpred = _mse(pred, target)
    ref, dref = R.mse_ref(pred, target)
    assert abs(float(loss) - ref) <= (B + 2) * R.U * ref
    # a rounded difference (u), a doubling (exact), a division to one ulp (2 u): 3 u + 2 u^2 < 4 u
    assert (np.abs(dpred - dref) <= 4 * R.U * np.abs(dref)).all()

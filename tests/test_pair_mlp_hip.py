"""GPU: fr_pair_mlp_scores (csrc/pair_mlp.hip) against its float64 restatement and running rounding bound
(tests/pair_mlp_ref.py): every finite cell within the bound -- no fixed tolerance --, -inf exactly at the pad item and the
history cells, a cell's bits a function of its user, its item and the parameters alone, NaN rows, saturated scores through
fr_topk_rows, a leading dimension above n_items, and the zero sizes.

The cuts the kernel makes, each with a case on both sides: 32 users per workgroup (1, 32, 33 users), 32 items per step (31,
32, 33 items), several steps per item slice (16 500 items for two user tiles: 512 slices of two steps), 128 output columns
per group (128 / 129), weights resident in LDS or streamed through it ([256, 256, 1] above 33 / 256 columns does not fit),
and, streamed, 32 input columns per chunk (n1 = 32 / 33).

test_nan_pattern_of_the_layered_path: the layered path (MLPLayers under no_grad, what `predict` runs) keeps a NaN through
every relu of fr_linear_fwd -- `x <= 0 ? 0 : x` in the general and one-output kernels (csrc/mlp_act.hpp: act_fwd),
`v > 0 ? v : v * 0` in the fast forms -- and so does this kernel: the two matrices have the same NaN cells."""
import numpy as np
import pytest
import torch

import pair_mlp_ref as R
import recommend_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _inputs(rng, U, N, widths, scale=1.0):
    P = rng.standard_normal((U, widths[0])).astype(np.float32)
    Q = rng.standard_normal((N, widths[0])).astype(np.float32)
    layers = R.random_layers(rng, widths, scale)
    # (a last bias of 1 or more: the last ReLU then passes most cells on, where a negative pre-activation scores 0.5 exactly
    # whatever the layers below computed)
    layers[-1] = (layers[-1][0], (np.float32(1) + np.abs(layers[-1][1])).astype(np.float32))
    return P, Q, layers


def _history(rng, U, N):
    """A CSR with an empty user, the pad item listed, and the last item listed."""
    rows = [np.sort(rng.choice(N, size=min(N, int(rng.integers(0, 4))), replace=False)) for _ in range(U)]
    rows[0] = np.array(sorted({0, N - 1}), np.int64)
    if U > 1:
        rows[1] = np.zeros(0, np.int64)
    indptr = np.zeros(U + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, np.concatenate(rows).astype(np.int64)


def _run(P, Q, layers, mask_pad=False, indptr=None, items=None, out=None):
    from fairrec.functional import pair_mlp_scores
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    pieces = {"P": t(P), "Q": t(Q), "layers": [(t(W), t(b)) for W, b in layers]}
    s = pair_mlp_scores(pieces, mask_pad=mask_pad, hist_indptr=None if indptr is None else t(indptr),
                        hist_items=None if items is None else t(items), out=out)
    torch.cuda.synchronize()
    return s.cpu().numpy()


def _check(P, Q, layers, seed=0):
    U, N = P.shape[0], Q.shape[0]
    indptr, items = _history(np.random.default_rng(seed), U, N)
    got = _run(P, Q, layers, True, indptr, items)
    s, bound = R.bound_pq(P, Q, layers)
    want = RR.mask(s, True, indptr, items)
    assert got.shape == (U, N) and got.dtype == np.float32
    assert np.array_equal(np.isneginf(got), np.isneginf(want)) and np.isneginf(got[:, 0]).all()
    live = ~np.isneginf(want)
    assert np.isfinite(got[live]).all()
    err = np.abs(got.astype(np.float64) - s)[live]
    if err.size:
        print(f"users {U} items {N} widths {[P.shape[1]] + [W.shape[0] for W, _ in layers]}: max err {err.max():.3g}, "
              f"max err / bound {(err / bound[live]).max():.3g}, cells at 0.5: {np.mean(got[live] == 0.5):.3g}")
    assert np.all(err <= bound[live])
    # without masks: the same bits outside the masked cells
    plain = _run(P, Q, layers)
    assert np.isfinite(plain).all() and np.array_equal(plain.view(np.uint32)[live], got.view(np.uint32)[live])


GRID = [(U, N, [n1] + tail) for U in (1, 33) for N in (1, 2, 31, 33, 130) for n1 in (1, 8, 33, 128)
        for tail in ([1], [1, 1], [16, 1], [64, 1])]


@pytest.mark.parametrize("U,N,widths", GRID, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else str(v))
def test_shape_grid(U, N, widths):
    rng = np.random.default_rng(1000 * U + 10 * N + sum(widths))
    _check(*_inputs(rng, U, N, widths), seed=N)


CUTS = [(33, 33, [33, 17, 9, 1]), (33, 33, [256, 256, 256, 1]), (32, 32, [8, 16, 1]), (33, 32, [8, 128, 1]),
        (5, 40, [8, 129, 1]), (5, 40, [16, 128, 129, 1]), (3, 40, [32, 256, 256, 1]), (3, 40, [33, 256, 256, 1]),
        (3, 40, [33, 256, 129, 1]), (2, 35, [256, 1]), (2, 35, [40, 24, 16, 8, 4, 1]), (33, 16500, [8, 1])]


@pytest.mark.parametrize("U,N,widths", CUTS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else str(v))
def test_cuts(U, N, widths):
    rng = np.random.default_rng(7 + U + N + sum(widths))
    _check(*_inputs(rng, U, N, widths), seed=U)


@pytest.mark.parametrize("widths", [[33, 17, 9, 1], [128, 64, 1], [33, 256, 256, 1]], ids=lambda w: "-".join(map(str, w)))
def test_a_cell_depends_on_its_user_its_item_and_the_parameters(widths):
    rng = np.random.default_rng(5)
    U, N = 40, 70
    P, Q, layers = _inputs(rng, U, N, widths)
    base = _run(P, Q, layers).view(np.uint32)
    perm = rng.permutation(U)
    assert np.array_equal(_run(P[perm], Q, layers).view(np.uint32), base[perm])                  # permuted
    rep = np.concatenate([np.arange(U), rng.integers(0, U, 27)])
    assert np.array_equal(_run(P[rep], Q, layers).view(np.uint32), base[rep])                    # repeated
    for u in (0, 31, 32, 39):
        assert np.array_equal(_run(P[u:u + 1], Q, layers).view(np.uint32), base[u:u + 1])        # alone
    for n in (1, 31, 33, 69):
        assert np.array_equal(_run(P, Q[:n], layers).view(np.uint32), base[:, :n])               # n_items truncated
    iperm = rng.permutation(N)
    assert np.array_equal(_run(P, Q[iperm], layers).view(np.uint32), base[:, iperm])             # the items' places


@pytest.mark.parametrize("widths", [[33, 17, 9, 1], [128, 64, 1], [33, 256, 256, 1]], ids=lambda w: "-".join(map(str, w)))
def test_nan_rows(widths):
    rng = np.random.default_rng(6)
    U, N = 35, 40
    P, Q, layers = _inputs(rng, U, N, widths)
    indptr, items = _history(rng, U, N)
    base = _run(P, Q, layers, True, indptr, items)
    masked = np.isneginf(base)
    for u in (0, 2, 34):
        P2 = P.copy()
        P2[u, rng.integers(0, widths[0])] = np.nan
        got = _run(P2, Q, layers, True, indptr, items)
        assert np.array_equal(np.isneginf(got), masked)
        assert np.isnan(got[u][~masked[u]]).all() and RR.same_bits(np.delete(got, u, 0), np.delete(base, u, 0))
    for i in (1, 33, 39):
        Q2 = Q.copy()
        Q2[i, rng.integers(0, widths[0])] = np.nan
        got = _run(P, Q2, layers, True, indptr, items)
        assert np.array_equal(np.isneginf(got), masked)
        assert np.isnan(got[:, i][~masked[:, i]]).all() and RR.same_bits(np.delete(got, i, 1), np.delete(base, i, 1))


def test_nan_pattern_of_the_layered_path():
    """The matrix's NaN pattern against MLPLayers under no_grad on the same rows (one NaN in one user's row: that user's row of the matrix, and nothing else, is NaN on both paths)."""
    from fairrec.functional import pair_mlp_pieces, pair_mlp_scores
    from fairrec.model.layers import MLPLayers
    torch.manual_seed(3)
    D, U, N = 16, 3, 40
    mlp = MLPLayers([2 * D, 32, 16, 1]).to(DEV).eval()
    x, w = torch.randn(U, D, device=DEV), torch.randn(N, D, device=DEV)
    x[1, 5] = float("nan")
    with torch.no_grad():
        split = pair_mlp_scores(pair_mlp_pieces(mlp, x, w))
        layered = torch.sigmoid(mlp(x.repeat_interleave(N, 0), w.repeat(U, 1)).view(U, N))
    a, b = torch.isnan(split).cpu().numpy(), torch.isnan(layered).cpu().numpy()
    print(f"NaN cells: split {int(a.sum())} of {a.size}, layered {int(b.sum())}; layered scores of the NaN user: "
          f"{layered[1].min().item()} .. {layered[1].max().item()}")
    assert a[1].all() and int(a.sum()) == N
    assert np.array_equal(a, b)


def test_saturated_scores_rank_in_ascending_id():
    from fairrec.functional import topk_rows
    U, N, k = 5, 300, 10
    P = np.full((U, 8), 50.0, np.float32)
    Q = np.full((N, 8), 50.0, np.float32)
    layers = [(np.ones((4, 8), np.float32), np.zeros(4, np.float32)), (np.ones((1, 4), np.float32), np.zeros(1, np.float32))]
    rng = np.random.default_rng(8)
    indptr, items = _history(rng, U, N)
    got = _run(P, Q, layers, True, indptr, items)
    want = RR.mask(np.ones((U, N), np.float32), True, indptr, items)
    assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32))
    val, idx = topk_rows(torch.from_numpy(got).to(DEV), k)
    for u in range(U):
        assert idx[u].cpu().tolist() == np.flatnonzero(want[u] == 1.0)[:k].tolist()
    assert np.array_equal(val.cpu().numpy(), np.ones((U, k), np.float32))


def test_leading_dimension_and_zero_sizes():
    rng = np.random.default_rng(9)
    P, Q, layers = _inputs(rng, 33, 45, [8, 16, 1])
    indptr, items = _history(rng, 33, 45)
    base = _run(P, Q, layers, True, indptr, items)
    buf = torch.full((33, 50), -7.0, device=DEV)
    got = _run(P, Q, layers, True, indptr, items, out=buf)
    assert np.array_equal(got[:, :45].view(np.uint32), base.view(np.uint32)) and np.all(got[:, 45:] == -7.0)
    one = torch.full((1, 50), -7.0, device=DEV)
    got = _run(P[:1], Q, layers, True, indptr[:2], items[:indptr[1]], out=one)
    assert np.array_equal(got[:, :45].view(np.uint32), base[:1].view(np.uint32)) and np.all(got[:, 45:] == -7.0)
    assert _run(P[:0], Q, layers, True, indptr[:1], items[:0]).shape == (0, 45)
    assert _run(P, Q[:0], layers, False).shape == (33, 0)
    assert _run(P[:0], Q[:0], layers, False).shape == (0, 0)

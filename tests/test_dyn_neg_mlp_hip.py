"""GPU: fr_dyn_neg_mlp_select / fr_dyn_neg_mlp_scores (csrc/dyn_neg_mlp.hip) against their float64 restatement and running
rounding bound (tests/dyn_neg_mlp_ref.py): every score within its bound -- no fixed tolerance --, every decided column's pick
the reference's, the ids those of fr_dyn_neg_select on the scores, a score's bits a function of its candidate's row, its P
row and the parameters alone, ties, NaNs, an id outside the table, the refusals, and a table left as it was.

The rows the reference consumes are LazyTable.gather's for the same ids, from item tables of 300 rows aged five steps under
each of the four learners with weight decay (most candidate rows are behind the step) and from one with nothing behind.

The cuts the kernel makes, each with a case on both sides (tests/dyn_neg_mlp_ref.py: CASES): 32 columns per workgroup (1, 33,
66 columns), the rounds (M = 1, 3), 32 input columns per chunk of the streamed item half of W1 (D = 1, 31, 33, 65, 256), 128
output columns per group (n1 = 1, 33, 128, 129), upper weights resident in LDS or streamed ([256, 256, 256, 1])."""
import numpy as np
import pytest
import torch

import dyn_neg_mlp_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS = 5


def _hyper(kind):
    from fairrec.optim import AdagradHyper, AdamHyper, RMSpropHyper, SGDHyper
    if kind == "sgd":
        return SGDHyper(1e-2, 1e-3, device=DEV)
    if kind == "adagrad":
        return AdagradHyper(1e-2, weight_decay=1e-3, device=DEV)
    if kind == "rmsprop":
        return RMSpropHyper(1e-2, weight_decay=1e-3, device=DEV)
    return AdamHyper(lr=1e-2, weight_decay=1e-3, device=DEV)


def _table(table0, kind, seed=0):
    """A LazyTable over `table0` stepped STEPS times under learner `kind` on batches of 40 rows and left unflushed: the rows
    of no batch, and those of the early batches, are behind the step.  `fresh`: flushed, nothing behind."""
    from fairrec.optim import LEARNER_ADAGRAD, LEARNER_RMSPROP, LEARNER_SGD, LazyTable
    t = LazyTable(torch.from_numpy(table0).to(DEV).contiguous())
    learner = {"sgd": LEARNER_SGD, "adagrad": LEARNER_ADAGRAD, "rmsprop": LEARNER_RMSPROP}.get(kind)
    if learner is not None:
        t.set_learner(learner)
    h = _hyper(kind)
    g = torch.Generator(device="cpu").manual_seed(seed)
    for _ in range(STEPS):
        idx = torch.randint(0, t.n_rows, (40,), generator=g).to(DEV)
        rows = t.gather_train(h, idx)
        t.apply_grad(h, (torch.randn(rows.shape, generator=g) * 0.05).to(DEV), 0)
    if kind == "fresh":
        t.flush(h)
    torch.cuda.synchronize()
    assert t.step == STEPS
    behind = float((t.last < t.step).float().mean())
    assert behind == 0.0 if kind == "fresh" else behind > 0.5, behind
    return t, h


def _state(t):
    return [x.clone() for x in (t.weight, t.m, t.v, t.last, t.stamp) if x is not None]


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                                        b.view(np.uint32) if b.dtype == np.float32 else b)


def _pieces(P, W1, layers):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return {"P": t(P), "W1": t(W1), "layers": [(t(W), t(b)) for W, b in layers]}


def _run(tab, hyper, P, W1, layers, cand, num, M, err=None):
    """(ids, scores, flag) of the two entries, as numpy."""
    from fairrec.functional import dyn_neg_mlp_select
    err = torch.zeros(1, dtype=torch.int32, device=DEV) if err is None else err
    ids, scores = dyn_neg_mlp_select(_pieces(P, W1, layers), tab, hyper, torch.from_numpy(cand).to(DEV), num, M, err,
                                     want_scores=True)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), scores.cpu().numpy(), int(err.item())


def _setup(name):
    c = R.make_case(name)
    tab, hyper = _table(c["table0"], c["table"], seed=c["seed"])
    c["P"] = R.user_half(c["x"], c["W1"], c["b1"]).astype(np.float32)
    return c, tab, hyper


@pytest.mark.parametrize("name", list(R.CASES))
def test_scores_within_the_bound_and_decided_picks(name):
    from fairrec.functional import dyn_neg_select
    c, tab, hyper = _setup(name)
    n, num, M, D = c["n"], c["num"], c["M"], c["D"]
    before = _state(tab)
    ids, scores, flag = _run(tab, hyper, c["P"], c["W1"], c["layers"], c["cand"], num, M)
    assert flag == 0 and ids.shape == (num * n,) and ids.dtype == np.int64
    assert scores.shape == (M * num * n,) and scores.dtype == np.float32 and np.isfinite(scores).all()
    for a, b in zip(before, _state(tab)):                    # purity: p / m / v / last / stamp bit-identical
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    cand_dev = torch.from_numpy(c["cand"]).to(DEV)
    rows = tab.gather(hyper, cand_dev, err).cpu().numpy()
    if c["table"] != "fresh":
        assert float((tab.last[cand_dev] < tab.step).float().mean()) > 0.5          # most candidate rows are behind
    s, bound = R.bound(rows, c["P"], c["W1"][:, D:], c["layers"], n)
    e = np.abs(scores.astype(np.float64) - s)
    ratio = float((e / bound).max())
    print(f"{name}: max err {e.max():.3g}, max err / bound {ratio:.3g}, scores at 0.5: {np.mean(scores == 0.5):.3g}")
    assert np.all(e <= bound), f"largest error / bound {ratio:.3g}"
    dec = R.decided(s.reshape(M, -1), bound.reshape(M, -1))
    assert np.mean(~dec) <= R.UNDECIDED_CAP, np.mean(~dec)
    want, _ = R.select(s.reshape(M, -1), c["cand"].reshape(M, -1))
    assert np.array_equal(ids[dec], want[dec])
    # select against scores: fr_dyn_neg_select on the twin's output, every column
    again = dyn_neg_select(torch.from_numpy(scores).to(DEV).view(M, -1), cand_dev.view(M, -1)).cpu().numpy()
    assert np.array_equal(ids, again)


@pytest.mark.parametrize("kind", R.TABLES)
def test_every_learner_at_the_yaml_shape(kind):
    """The nfcf-yaml case's parameters over a table aged under each learner, against LazyTable.gather's rows."""
    c = R.make_case("nfcf-yaml")
    tab, hyper = _table(c["table0"], kind, seed=3)
    n, num, M, D = c["n"], c["num"], c["M"], c["D"]
    P = R.user_half(c["x"], c["W1"], c["b1"]).astype(np.float32)
    before = _state(tab)
    ids, scores, flag = _run(tab, hyper, P, c["W1"], c["layers"], c["cand"], num, M)
    assert flag == 0
    for a, b in zip(before, _state(tab)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    rows = tab.gather(hyper, torch.from_numpy(c["cand"]).to(DEV)).cpu().numpy()
    s, bound = R.bound(rows, P, c["W1"][:, D:], c["layers"], n)
    e = np.abs(scores.astype(np.float64) - s)
    assert np.all(e <= bound), f"largest error / bound {(e / bound).max():.3g}"
    dec = R.decided(s.reshape(M, -1), bound.reshape(M, -1))
    assert np.mean(~dec) <= R.UNDECIDED_CAP
    assert np.array_equal(ids[dec], R.select(s.reshape(M, -1), c["cand"].reshape(M, -1))[0][dec])


@pytest.mark.parametrize("name", ["n33-num2-M3", "net-33-17-9-1", "nfcf-yaml", "D256"])
def test_a_score_depends_on_its_row_its_p_row_and_the_parameters(name):
    c, tab, hyper = _setup(name)
    n, num, M = c["n"], c["num"], c["M"]
    rng = np.random.default_rng(5)
    run = lambda P, cand, n_, num_, M_: _run(tab, hyper, P, c["W1"], c["layers"], np.ascontiguousarray(cand).reshape(-1),
                                             num_, M_)
    cand = c["cand"].reshape(M, num, n)
    ids, scores, _ = run(c["P"], cand, n, num, M)
    ids, scores = ids.reshape(num, n), scores.reshape(M, num, n)
    perm = rng.permutation(n)                                                      # the batch rows permuted
    ids2, scores2, _ = run(c["P"][perm], cand[:, :, perm], n, num, M)
    assert _same_bits(scores2.reshape(M, num, n), scores[:, :, perm]) and np.array_equal(ids2.reshape(num, n), ids[:, perm])
    rep = cand.copy()                                                              # a candidate repeated within its column
    rep[M - 1] = rep[0]
    _, scores3, _ = run(c["P"], rep, n, num, M)
    scores3 = scores3.reshape(M, num, n)
    assert _same_bits(scores3[M - 1], scores[0]) and _same_bits(scores3[:M - 1], scores[:M - 1])
    for j, i in ((0, 0), (num - 1, n - 1), (0, min(31, n - 1)), (num - 1, min(32, n - 1))):     # one column alone
        ids1, scores1, _ = run(c["P"][i:i + 1], cand[:, j, i], 1, 1, M)
        assert _same_bits(scores1, scores[:, j, i]) and ids1[0] == ids[j, i]
    ids4, scores4, _ = run(c["P"], cand[:1], n, num, 1)                            # M truncated
    assert _same_bits(scores4.reshape(num, n), scores[0]) and np.array_equal(ids4, cand[0].reshape(-1))


def test_equal_scores_pick_the_first_candidate():
    c, tab, hyper = _setup("n33-num2-M3")
    layers = [(np.zeros_like(W), b) for W, b in c["layers"]]
    ids, scores, _ = _run(tab, hyper, c["P"], c["W1"], layers, c["cand"], c["num"], c["M"])
    assert len(set(scores.view(np.uint32).tolist())) == 1 and scores[0] > 0.5
    assert np.array_equal(ids, c["cand"][:c["num"] * c["n"]])


def test_nan_in_an_item_row_or_a_p_row():
    c, tab, hyper = _setup("n33-num2-M3")
    n, num, M = c["n"], c["num"], c["M"]
    cand = c["cand"].reshape(M, num * n)
    base_ids, base, _ = _run(tab, hyper, c["P"], c["W1"], c["layers"], c["cand"], num, M)
    base = base.reshape(M, num * n)
    item = int(cand[1, 40])                                   # an item row with a NaN: its candidates, and only they
    keep = tab.weight[item, 3].clone()
    tab.weight[item, 3] = float("nan")
    ids, scores, flag = _run(tab, hyper, c["P"], c["W1"], c["layers"], c["cand"], num, M)
    tab.weight[item, 3] = keep
    scores = scores.reshape(M, num * n)
    hit = cand == item
    assert flag == 0 and hit.sum() >= 1 and np.isnan(scores[hit]).all()
    assert np.array_equal(scores.view(np.uint32)[~hit], base.view(np.uint32)[~hit])
    cols = hit.any(axis=0)
    assert (ids[cols] == item).all() and np.array_equal(ids[~cols], base_ids[~cols])
    P = c["P"].copy()                                         # a P row with a NaN: that row's columns, every round
    P[7, 2] = np.nan
    ids, scores, flag = _run(tab, hyper, P, c["W1"], c["layers"], c["cand"], num, M)
    scores = scores.reshape(M, num, n)
    assert flag == 0 and np.isnan(scores[:, :, 7]).all()
    assert np.array_equal(np.delete(scores, 7, 2).view(np.uint32), np.delete(base.reshape(M, num, n), 7, 2).view(np.uint32))
    ids, base_ids = ids.reshape(num, n), base_ids.reshape(num, n)
    assert np.array_equal(ids[:, 7], cand[0].reshape(num, n)[:, 7])            # the first NaN wins
    assert np.array_equal(np.delete(ids, 7, 1), np.delete(base_ids, 7, 1))


def test_an_id_outside_the_table_sets_the_flag():
    from fairrec import _C
    c, tab, hyper = _setup("n33-num2-M3")
    n, num, M = c["n"], c["num"], c["M"]
    base_ids, base, _ = _run(tab, hyper, c["P"], c["W1"], c["layers"], c["cand"], num, M)
    for bad in (R.N_ITEMS, -1):
        cand = c["cand"].copy()
        k = 1 * num * n + 37                                  # round 1 of column 37
        cand[k] = bad
        ids, scores, flag = _run(tab, hyper, c["P"], c["W1"], c["layers"], cand, num, M)
        assert flag & _C.DEV_ERR_INDEX_RANGE
        assert np.array_equal(np.delete(scores, k).view(np.uint32), np.delete(base, k).view(np.uint32))
        assert np.array_equal(np.delete(ids, 37), np.delete(base_ids, 37))


def test_refusals_write_nothing():
    R.check_refusals()


def test_wrapper_raises_on_shapes():
    from fairrec.functional import dyn_neg_mlp_select
    c, tab, hyper = _setup("n33-num2-M3")
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    cand = torch.from_numpy(c["cand"]).to(DEV)
    good = _pieces(c["P"], c["W1"], c["layers"])
    with pytest.raises(ValueError):
        dyn_neg_mlp_select(good, tab, hyper, cand[:-1], c["num"], c["M"], err)
    with pytest.raises(ValueError):
        dyn_neg_mlp_select(dict(good, W1=good["W1"][:, :c["D"]].contiguous()), tab, hyper, cand, c["num"], c["M"], err)
    with pytest.raises(ValueError):
        dyn_neg_mlp_select(dict(good, P=good["P"][:, :-1].contiguous()), tab, hyper, cand, c["num"], c["M"], err)
    with pytest.raises(ValueError):
        dyn_neg_mlp_select(dict(good, layers=good["layers"][:-1] + [(good["layers"][-1][0][:, :-1].contiguous(),
                                                                     good["layers"][-1][1])]), tab, hyper, cand, c["num"], c["M"], err)

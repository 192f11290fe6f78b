"""GPU: SGD / Adagrad / RMSprop on the lazy tables and the dense step, against torch.

- LazyTable.gather_train + apply_grad (with the sweeper slice) for T steps over batches with repeated rows and duplicates
  inside a batch, then a flush: against a float64 restatement of torch's step (every row stepped every step) and against
  a stock torch.optim.<Learner> on the device run dense on the same gradients; the lazy table against a table flushed
  after every step; rows in no batch bit-identical to their initial values where a zero-gradient step is the identity.
- fr_adam_dense / fr_adam_dense_multi with each learner against torch.optim.<Learner>.
- one case per learner at the 10 000 001 x 256 table of BASELINE configs[4] (rows checked: the batches' and a sample).
- fr_dyn_neg_dot_select on a table aged under SGD with weight decay against the composed path.
- a captured step (GraphedStep) against the eager step, bit for bit.
- the trainer's learner dispatch."""
import ctypes

import numpy as np
import pytest
import torch

from fairrec import _C
from fairrec.optim import (LEARNER_ADAGRAD, LEARNER_RMSPROP, LEARNER_SGD, AdagradHyper, LazyTable, RMSpropHyper,
                           SGDHyper)

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR = 1e-2
LEARNERS = ("sgd", "adagrad", "rmsprop")
ID = {"sgd": LEARNER_SGD, "adagrad": LEARNER_ADAGRAD, "rmsprop": LEARNER_RMSPROP}


def _hyper(name, wd):
    if name == "sgd":
        return SGDHyper(LR, wd, device=DEV)
    if name == "adagrad":
        return AdagradHyper(LR, weight_decay=wd, device=DEV)
    return RMSpropHyper(LR, weight_decay=wd, device=DEV)


def _torch_opt(name, params, wd):
    cls = {"sgd": torch.optim.SGD, "adagrad": torch.optim.Adagrad, "rmsprop": torch.optim.RMSprop}[name]
    return cls(params, lr=LR, weight_decay=wd)


def _ref_step(name, p, s, g, wd):
    """torch's step in float64 (p, s, g: float64 arrays; s = sum / square_avg or None)."""
    g = g + wd * p
    if name == "sgd":
        return p - LR * g, s
    if name == "adagrad":
        s = s + g * g
        return p - LR * g / (np.sqrt(s) + 1e-10), s
    s = 0.99 * s + 0.01 * g * g
    return p - LR * g / (np.sqrt(s) + 1e-8), s


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    bad = ~(np.abs(a - b) <= 1e-4 * np.abs(b) + 1e-6)
    assert not bad.any(), f"{what}: {bad.sum()} elements off, worst {np.abs(a - b).max()}"


def _batches(n_rows, M, T, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    hot = torch.randint(1, n_rows, (8,), generator=g)
    out = []
    for t in range(T):
        idx = torch.randint(1, n_rows, (M,), generator=g)
        idx[: M // 4] = hot[torch.randint(0, 8, (M // 4,), generator=g)]     # rows repeated across and inside batches
        idx[M // 2] = idx[M // 2 + 1]
        out.append(idx[torch.randperm(M, generator=g)])
    return out


def _run_lazy(name, wd, W0, batches, grads, sweep, flush_every):
    w = W0.clone()
    t = LazyTable(w)
    t.set_learner(ID[name])
    h = _hyper(name, wd)
    for idx, gr in zip(batches, grads):
        rows = t.gather_train(h, idx.to(DEV))
        assert rows.shape == gr.shape
        t.apply_grad(h, gr, sweep)
        if flush_every:
            t.flush(h)
    t.flush(h)
    torch.cuda.synchronize()
    return t, w


@pytest.mark.parametrize("D", [1, 48, 64, 128, 256])
@pytest.mark.parametrize("wd", [0.0, 1e-3])
@pytest.mark.parametrize("name", LEARNERS)
def test_lazy_table_against_torch(name, wd, D):
    n_rows, M, T = 600, 96, 6
    gen = torch.Generator(device="cpu").manual_seed(D * 7 + int(wd > 0))
    W0 = (torch.randn(n_rows, D, generator=gen) * 0.1).to(DEV)
    batches = _batches(n_rows, M, T, seed=D)
    grads = [(torch.randn(M, D, generator=gen) * 0.05).to(DEV) for _ in range(T)]
    lazy, w = _run_lazy(name, wd, W0, batches, grads, sweep=4, flush_every=False)
    eager, w2 = _run_lazy(name, wd, W0, batches, grads, sweep=0, flush_every=True)
    assert lazy.step == T
    if name == "sgd":
        assert lazy.m is None and lazy.v is None           # built without state: nothing can read or write it
    else:
        assert lazy.v is None
    # float64 restatement, every row stepped every step (dense gradient = duplicate sum)
    p = W0.double().cpu().numpy()
    s = np.zeros_like(p)
    for idx, gr in zip(batches, grads):
        G = np.zeros_like(p)
        np.add.at(G, idx.numpy(), gr.double().cpu().numpy())
        p, s = _ref_step(name, p, s, G, wd)
    _close(w.cpu().numpy(), p, "weights vs float64")
    if name != "sgd":
        _close(lazy.m.cpu().numpy(), s, "state vs float64")
    # stock torch optimizer on the device, dense
    P = torch.nn.Parameter(W0.clone())
    opt = _torch_opt(name, [P], wd)
    for idx, gr in zip(batches, grads):
        opt.zero_grad()
        P.grad = torch.zeros_like(P).index_add_(0, idx.to(DEV), gr)
        opt.step()
    _close(w.cpu().numpy(), P.detach().cpu().numpy(), "weights vs torch.optim")
    if name != "sgd":
        key = "sum" if name == "adagrad" else "square_avg"
        _close(lazy.m.cpu().numpy(), opt.state[P][key].cpu().numpy(), "state vs torch.optim")
    # lazy against flushed every step: the same replayed steps one at a time
    torch.testing.assert_close(w, w2, rtol=5e-7, atol=1e-9)
    if name != "sgd":
        torch.testing.assert_close(lazy.m, eager.m, rtol=5e-7, atol=1e-12)
    # rows in no batch
    seen = torch.zeros(n_rows, dtype=torch.bool)
    for idx in batches:
        seen[idx] = True
    cold = (~seen).nonzero().view(-1).to(DEV)
    assert cold.numel() > 0
    if wd == 0.0:       # a zero-gradient step leaves p as it is (RMSprop: square_avg of a cold row stays 0 as well)
        assert torch.equal(w[cold], W0[cold])
        if name != "sgd":
            assert torch.equal(lazy.m[cold], torch.zeros_like(lazy.m[cold]))
    else:
        assert not torch.equal(w[cold], W0[cold])


@pytest.mark.parametrize("name", LEARNERS)
def test_dense_step_against_torch(name):
    lib = _C.lib()
    wd, T = 1e-3, 5
    gen = torch.Generator(device="cpu").manual_seed(1)
    shapes = [(3001,), (17, 33), (64,)]
    ps = [(torch.randn(*s, generator=gen) * 0.1).to(DEV) for s in shapes]
    gs = [[(torch.randn(*s, generator=gen) * 0.05).to(DEV) for s in shapes] for _ in range(T)]
    h = _hyper(name, wd)
    has_m = name != "sgd"
    a = [p.clone() for p in ps]                      # fr_adam_dense
    am = [torch.zeros_like(p) for p in ps] if has_m else [None] * len(ps)
    b = [p.clone() for p in ps]                      # fr_adam_dense_multi
    bm = [torch.zeros_like(p) for p in ps] if has_m else [None] * len(ps)
    st = _C.current_stream()
    for t in range(T):
        for k in range(len(ps)):
            _C.check(lib.fr_adam_dense(a[k].data_ptr(), gs[t][k].data_ptr(), _C.ptr(am[k]), 0, a[k].numel(),
                                       ctypes.byref(h.c()), t + 1, st), "fr_adam_dense")
        descs = (_C.FrDenseDesc * len(ps))(*[_C.FrDenseDesc(b[k].data_ptr(), gs[t][k].data_ptr(), _C.ptr(bm[k]), 0,
                                                            b[k].numel(), t + 1, None) for k in range(len(ps))])
        _C.check(lib.fr_adam_dense_multi(descs, len(ps), ctypes.byref(h.c()), st), "fr_adam_dense_multi")
    P = [torch.nn.Parameter(p.clone()) for p in ps]
    opt = _torch_opt(name, P, wd)
    for t in range(T):
        for k in range(len(ps)):
            P[k].grad = gs[t][k]
        opt.step()
    torch.cuda.synchronize()
    for k in range(len(ps)):
        _close(a[k].cpu().numpy(), P[k].detach().cpu().numpy(), f"fr_adam_dense[{k}]")
        assert torch.equal(a[k], b[k]) and (not has_m or torch.equal(am[k], bm[k]))
        if has_m:
            key = "sum" if name == "adagrad" else "square_avg"
            _close(am[k].cpu().numpy(), opt.state[P[k]][key].cpu().numpy(), f"state[{k}]")


@pytest.mark.parametrize("name", LEARNERS)
def test_baseline_config4_table_size(name):
    """10 000 001 x 256 (BASELINE configs[4]'s item table), B = 8192, weight decay on, default sweep: the rows of the
    batches and a sample of the others against the float64 restatement (each row evolves on its own)."""
    n_rows, D, M, T, wd = 10_000_001, 256, 8192, 3, 1e-3
    gen = torch.Generator(device=DEV).manual_seed(5)
    w = torch.randn(n_rows, D, device=DEV, generator=gen) * 0.1
    batches = _batches(n_rows, M, T, seed=9)
    grads = [torch.randn(M, D, device=DEV, generator=gen) * 0.05 for _ in range(T)]
    sample = torch.unique(torch.cat(batches[:1] + [torch.randint(0, n_rows, (2000,))]))
    W0 = w[sample.to(DEV)].double().cpu().numpy()
    t = LazyTable(w)
    t.set_learner(ID[name])
    h = _hyper(name, wd)
    for idx, gr in zip(batches, grads):
        t.gather_train(h, idx.to(DEV))
        t.apply_grad(h, gr, t.default_sweep(M))
    t.flush(h)
    got = w[sample.to(DEV)].cpu().numpy()
    pos = {int(r): k for k, r in enumerate(sample)}
    p, s = W0, np.zeros_like(W0)
    for idx, gr in zip(batches, grads):
        G = np.zeros_like(p)
        g64 = gr.double().cpu().numpy()
        for j, r in enumerate(idx.tolist()):
            if r in pos:
                G[pos[r]] += g64[j]
        p, s = _ref_step(name, p, s, G, wd)
    _close(got, p, f"{name} at 10M x 256")
    if name != "sgd":
        _close(t.m[sample.to(DEV)].cpu().numpy(), s, f"{name} state at 10M x 256")
    del t, w
    torch.cuda.empty_cache()


def test_dyn_neg_dot_select_on_a_table_aged_under_sgd():
    from fairrec.functional import dyn_neg_dot_select
    n_rows, D, M, T, wd = 5000, 64, 128, 7, 1e-3
    gen = torch.Generator(device="cpu").manual_seed(4)
    w = (torch.randn(n_rows, D, generator=gen) * 0.1).to(DEV)
    t = LazyTable(w)
    t.set_learner(LEARNER_SGD)
    h = _hyper("sgd", wd)
    p64 = w.double().cpu().numpy()              # float64 restatement of the aged table (every row stepped every step)
    for idx in _batches(n_rows, M, T, seed=2):
        gr = torch.randn(M, D, generator=gen) * 0.05
        t.gather_train(h, idx.to(DEV))
        t.apply_grad(h, gr.to(DEV), 0)                      # no sweep: most rows stay behind
        G = np.zeros_like(p64)
        np.add.at(G, idx.numpy(), gr.double().numpy())
        p64, _ = _ref_step("sgd", p64, None, G, wd)
    n, num, Mc = 300, 2, 6
    user = (torch.randn(n, D, generator=gen) * 0.1).to(DEV)
    cand = torch.randint(0, n_rows, (Mc * num * n,), generator=gen).to(DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = dyn_neg_dot_select(t, h, user, cand, num, Mc, err)
    scores = dyn_neg_dot_select(t, h, user, cand, num, Mc, err, scores_only=True)
    # composed: rows as of the step (fr_table_gather), then the dot, sigmoid and torch.max
    rows = t.gather(h, cand, err)
    _close(rows.cpu().numpy(), p64[cand.cpu().numpy()], "aged rows vs float64")      # the replay, independently
    users = user[torch.arange(Mc * num * n, device=DEV) % n]
    s64 = 1.0 / (1.0 + np.exp(-(p64[cand.cpu().numpy()] * users.double().cpu().numpy()).sum(1)))
    np.testing.assert_allclose(scores.double().cpu().numpy(), s64, rtol=1e-5, atol=1e-6)
    s_ref = torch.sigmoid((rows * users).sum(1))
    torch.testing.assert_close(scores, s_ref, rtol=1e-5, atol=1e-6)
    sc = scores.view(Mc, num * n)
    want = cand.view(Mc, num * n)[torch.max(sc, dim=0)[1], torch.arange(num * n, device=DEV)]
    assert torch.equal(got.view(-1), want)
    # and the rows read equal the flushed table's
    t.flush(h)
    assert torch.equal(rows, w[cand])
    assert int(err.item()) == 0


def test_graphed_step_equals_eager_step():
    from fairrec.data.interaction import Interaction
    from fairrec.engine import GenericEngine
    from fairrec.graph import GraphedStep
    from fairrec.optim import FusedLazyRMSprop
    n_rows, D, M, T = 3000, 64, 256, 6
    gen = torch.Generator(device="cpu").manual_seed(8)
    W0 = torch.randn(n_rows, D, generator=gen) * 0.1
    B0 = torch.randn(D, generator=gen) * 0.1
    feeds = [Interaction({"id": b, "y": torch.randn(M, generator=gen)}) for b in _batches(n_rows, M, T, seed=3)]
    outs = []
    for graphed in (False, True):
        emb = torch.nn.Parameter(W0.clone().to(DEV))
        bias = torch.nn.Parameter(B0.clone().to(DEV))
        eng = GenericEngine(DEV)
        eng.add_table("emb", emb)
        eng.add_dense("bias", bias)
        opt = FusedLazyRMSprop(eng, lr=LR, weight_decay=1e-3, sweep_period=8)

        def loss_fn(inter):
            r = eng.lookup("emb", inter["id"])
            return (((r + bias).sum(1) - inter["y"]) ** 2).mean()

        step = GraphedStep(eng, opt, loss_fn) if graphed else None
        losses = []
        for b in feeds:
            if graphed:
                losses.append(step(b).clone())
            else:
                opt.zero_grad()
                loss = loss_fn(b.to(DEV))
                loss.backward()
                opt.step()
                losses.append(loss.detach())
        if graphed:
            assert step.graph is not None
        eng.sync_steps()
        eng.flush()
        torch.cuda.synchronize()
        outs.append((torch.stack(losses), emb.detach().clone(), bias.detach().clone(),
                     eng._tables["emb"].m.clone(), eng._dense["bias"].m.clone(), eng._tables["emb"].step))
    (l0, e0, b0, m0, d0, s0), (l1, e1, b1, m1, d1, s1) = outs
    assert s0 == s1 == T
    assert torch.equal(l0, l1) and torch.equal(e0, e1) and torch.equal(b0, b1)
    assert torch.equal(m0, m1) and torch.equal(d0, d1)


# ---- trainer -----------------------------------------------------------------------------------------------------------
def _trainer(tmp_path, model, learner, extra=None, wd=1e-3):
    from fairrec.config import Config
    from fairrec.data.dataloader import TrainDataLoader
    from fairrec.data.dataset import synthetic_dataset
    from fairrec.utils import get_model, get_trainer, init_seed
    d = {"train_batch_size": 256, "embedding_size": 16, "epochs": 2, "device": "cuda", "checkpoint_dir": str(tmp_path),
         "learning_rate": LR, "weight_decay": wd, "learner": learner}
    d.update(extra or {})
    cfg = Config(model=model, config_dict=d)
    init_seed(3)
    ds = synthetic_dataset(cfg, 300, 120, 2000, seed=11)
    if model in ("NFCF", "PFCN_BiasedMF"):       # pairwise / labelled models: negatives from the device sampler
        from fairrec.quick_start import split_dataset
        from fairrec.sampler import Sampler
        tr, va, te = split_dataset(ds)
        sampler = Sampler(["train", "valid", "test"], [tr, va, te], "uniform", device=DEV).set_phase("train")
        train = TrainDataLoader(cfg, tr.to(DEV), sampler=sampler, shuffle=False)
        ds = train.dataset
    else:
        train = TrainDataLoader(cfg, ds, shuffle=False)
    m = get_model(model)(cfg, ds).to(cfg["device"])
    return cfg, train, m, get_trainer(None, model)(cfg, m)


def test_trainer_dispatch(tmp_path, caplog):
    import logging
    from fairrec.optim import FusedLazyAdam, FusedLazyAdagrad, FusedLazyRMSprop, FusedLazySGD
    for learner, cls in (("SGD", FusedLazySGD), ("adagrad", FusedLazyAdagrad), ("RMSprop", FusedLazyRMSprop),
                         ("adam", FusedLazyAdam)):
        _, _, _, tr = _trainer(tmp_path, "NFCF", learner)
        assert type(tr.optimizer) is cls
    with pytest.raises(ValueError, match="SparseAdam"):
        _trainer(tmp_path, "NFCF", "sparse_adam")
    with caplog.at_level(logging.WARNING):
        _, _, _, tr = _trainer(tmp_path, "NFCF", "lbfgs")
    assert type(tr.optimizer) is FusedLazyAdam and tr.optimizer.hyper.weight_decay == 0.0
    assert "unrecognized optimizer" in caplog.text
    for learner in ("sgd", "adagrad", "rmsprop"):
        with pytest.raises(NotImplementedError):
            _trainer(tmp_path, "FOCF", learner)
    from fairrec.replicated_engine import ReplicatedGenericEngine
    from fairrec.sharded_engine import ShardedGenericEngine
    for cls in (ReplicatedGenericEngine, ShardedGenericEngine):
        eng = cls.__new__(cls)
        eng.device = torch.device(DEV)
        with pytest.raises(NotImplementedError):
            FusedLazySGD(eng, lr=LR)


@pytest.mark.parametrize("model,extra", [("NFCF", {}), ("PFCN_BiasedMF", {"filter_mode": "none"}),
                                         ("PFCN_BiasedMF", {"filter_mode": "sm"}), ("FairGo_PMF", {"pretrain_epochs": 1})])
@pytest.mark.parametrize("learner", LEARNERS)
def test_trainer_fit_runs(tmp_path, model, extra, learner):
    cfg, train, m, tr = _trainer(tmp_path, model, learner, extra)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    tr.fit(train, valid_data=None, verbose=False, saved=False)
    losses = [tr.train_loss_dict[e] for e in range(2)]
    assert all(np.isfinite(losses)), losses
    after = m.state_dict()
    assert any(not torch.equal(before[k], after[k]) for k in before if k in after)


@pytest.mark.parametrize("learner", LEARNERS)
def test_checkpoint_round_trip_with_stock_torch(tmp_path, learner):
    """state_dict(param_names=...) loads into torch.optim.<Learner>; one more step of both from there agrees, and the
    stock optimizer's state dict resumes the fused one."""
    cfg, train, m, tr = _trainer(tmp_path, "NFCF", learner)
    tr._train_epoch(train, 0)
    names = [n for n, _ in m.named_parameters()]
    sd = tr.optimizer.state_dict(param_names=names)
    params = [p for _, p in m.named_parameters()]
    stock = _torch_opt(learner, params, 1e-3)
    stock.load_state_dict(sd)               # accepted as it is
    if learner == "sgd":
        assert sd["state"] == {}
    elif learner == "adagrad":
        assert sorted(sd["state"]) == list(range(len(names)))
    for k, st in sd["state"].items():
        assert st["step"].dtype == torch.float32
    # the stock state dict resumes through load_state_dict(param_names=...)
    tr.optimizer.load_state_dict(stock.state_dict(), param_names=names)
    sd2 = tr.optimizer.state_dict(param_names=names)
    assert sorted(sd2["state"]) == sorted(sd["state"])
    for k in sd["state"]:
        for key, v in sd["state"][k].items():
            assert torch.equal(torch.as_tensor(v).cpu(), torch.as_tensor(sd2["state"][k][key]).cpu()), (k, key)

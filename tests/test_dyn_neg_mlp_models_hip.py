"""GPU: `dynamic_neg_scorer: split` end to end -- NFCF and PFCN_MLP (filter_mode none), 150 users x 300 items, D = 16,
`neg_sampling: {uniform: 1, dynamic: 4}`.

With `split` the models' `dyn_neg_select` hook returns the ids of fr_dyn_neg_mlp_select: a loader batch's negatives against
the float64 restatement's pick on the same draws wherever that pick is decided (tests/dyn_neg_mlp_ref.py), the sampler's
generator left where the `pairs` run leaves it, no lazy table with a pending batch, and a two-epoch run with finite losses.
With the key absent or `pairs` the hook answers None and the loader's batches are those of `predict` + fr_dyn_neg_select, bit
for bit.  A bad key value, a filtered PFCN_MLP and a scorer with BatchNorm keep their refusals and fallbacks.

The scorer's parameters are overwritten by a seeded draw whose last bias is 1 or more (`_set_scorer`, as make_case's): an MLP that ends in a
ReLU scores sigmoid(0) = 0.5 exactly wherever its last pre-activation is negative, and equal scores leave a pick undecided."""
import numpy as np
import pytest
import torch

import dyn_neg_mlp_ref as R
import pair_mlp_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 16
M, NUM = 4, 1
MODELS = {"NFCF": dict(mlp_hidden_size=[32, 16], load_pretrain_path=None, LABEL_FIELD="label"),
          "PFCN_MLP": dict(filter_mode="none", mlp_hidden_size_list=[32, 16])}


def _setup(model_name, ck_dir, seed=5, **more):
    from fairrec.config import Config
    from fairrec.data.dataloader import TrainDataLoader
    from fairrec.data.dataset import synthetic_dataset
    from fairrec.quick_start import split_dataset
    from fairrec.sampler import Sampler
    from fairrec.utils import get_model, get_trainer, init_seed
    cfg = Config(model=model_name, config_dict=dict({"device": DEV, "train_batch_size": 200, "embedding_size": D,
                                                     "neg_sampling": {"uniform": NUM, "dynamic": M},
                                                     "checkpoint_dir": str(ck_dir), "seed": seed}, **MODELS[model_name], **more))
    init_seed(cfg["seed"], cfg["reproducibility"])
    ds = synthetic_dataset(cfg, 150, 300, 4000, seed=seed)
    tr, va, te = split_dataset(ds)
    sampler = Sampler(["train", "valid", "test"], [tr, va, te], "uniform", device=DEV).set_phase("train")
    dl = TrainDataLoader(cfg, tr.to(DEV), sampler=sampler, shuffle=False)
    model = get_model(model_name)(cfg, dl.dataset).to(DEV)
    trainer = get_trainer(None, model_name)(cfg, model)
    dl.get_model(model)
    return dl, model, trainer


def _scorer(model):
    return model.mlp_layers if hasattr(model, "mlp_layers") else model.mlp_layer


def _tables(model):
    return ("user_embedding.weight", "item_embedding.weight") if hasattr(model, "mlp_layers") else (model._utab, model._itab)


def _set_scorer(model, seed=7):
    lins = _scorer(model).linears()
    widths = [lin.out_features for lin in lins]
    rng = np.random.default_rng(seed)
    W1 = (rng.standard_normal((widths[0], 2 * D)) / np.sqrt(2 * D)).astype(np.float32)
    b1 = (0.5 * rng.standard_normal(widths[0])).astype(np.float32)
    layers = P.random_layers(rng, widths)
    layers[-1] = ((np.float32(0.5) * layers[-1][0]).astype(np.float32),                   # (as tests/dyn_neg_mlp_ref.py: make_case)
                  (np.float32(1) + np.float32(0.5) * np.abs(layers[-1][1])).astype(np.float32))
    with torch.no_grad():
        for lin, (W, b) in zip(lins, [(W1, b1)] + layers):
            lin.weight.copy_(torch.from_numpy(W))
            lin.bias.copy_(torch.from_numpy(b))


def _restated(loader, inter_feat):
    """abstract_dataloader.py `_neg_sampling`, dynamic branch, through `predict` + fr_dyn_neg_select: the parent's path."""
    from fairrec.data.interaction import Interaction
    from fairrec.functional import dyn_neg_select
    m, num, model = loader.candidate_num, loader.neg_sample_num, loader.model
    cand = loader.sampler.sample_by_user_ids(inter_feat[loader.uid_field], inter_feat[loader.iid_field], num * m).to(DEV)
    model.eval()
    inter = inter_feat.repeat(num * m)
    inter.update(Interaction({loader.iid_field: cand}))
    with torch.no_grad():
        neg = dyn_neg_select(model.predict(inter).reshape(m, -1), cand.view(m, -1))
    model.train()
    return neg


def _batches_with(dl, fn=None):
    from fairrec.data import dataloader as DL
    orig = DL.TrainDataLoader._dynamic_negatives
    if fn is not None:
        DL.TrainDataLoader._dynamic_negatives = fn
    try:
        return [b.interaction for b in dl]
    finally:
        DL.TrainDataLoader._dynamic_negatives = orig


@pytest.mark.parametrize("model_name", list(MODELS))
def test_split_picks_the_reference_s_candidates(model_name, tmp_path):
    from fairrec.functional import dyn_neg_mlp_pieces
    dl, model, _ = _setup(model_name, tmp_path, dynamic_neg_scorer="split")
    assert model.dynamic_neg_scorer == "split"
    _set_scorer(model)
    eng = model.hip_engine()
    utab, itab = _tables(model)
    rs = dl.sampler.rs
    W1, b1, layers = P.pieces_of_module(_scorer(model))
    model.train()
    undecided, columns = 0, 0
    for lo in range(0, len(dl.dataset), dl.step):
        cur = dl.dataset[lo:lo + dl.step]
        uid, iid = cur[dl.uid_field], cur[dl.iid_field]
        n = len(cur)
        st0 = rs.get_state()
        cand = dl.sampler.sample_by_user_ids(uid, iid, NUM * M).to(DEV)
        st_draw = rs.get_state()
        rs.set_state(st0)
        model.eval()
        hook = model.dyn_neg_select(cur, cand, NUM, M)
        model.train()
        assert hook is not None and hook.shape == (NUM * n,) and hook.dtype == torch.int64
        neg = dl._dynamic_negatives(cur)                        # the loader: the same draws, the hook's ids
        st_split = rs.get_state()
        assert model.training and torch.equal(neg, hook)
        assert all(t._pending is None for t in eng._tables.values())
        assert int(eng.err_flag.item()) == 0
        with torch.no_grad():
            x = eng.lookup(utab, uid)
            rows = eng._tables[itab].gather(eng._hyper(itab), cand).cpu().numpy()
            P32 = dyn_neg_mlp_pieces(_scorer(model), x)["P"].cpu().numpy()
        s, bound = R.bound(rows, P32, W1[:, D:], layers, n)
        dec = R.decided(s.reshape(M, -1), bound.reshape(M, -1))
        want, _ = R.select(s.reshape(M, -1), cand.cpu().numpy().reshape(M, -1))
        assert np.array_equal(neg.cpu().numpy()[dec], want[dec]), lo
        undecided, columns = undecided + int((~dec).sum()), columns + dec.size
        # the `pairs` run from the same generator state: the same draws, so the same state afterwards
        rs.set_state(st0)
        model.dynamic_neg_scorer = "pairs"
        try:
            model.eval()
            assert model.dyn_neg_select(cur, cand, NUM, M) is None
            model.train()
            dl._dynamic_negatives(cur)
        finally:
            model.dynamic_neg_scorer = "split"
        for a, b in ((st_split, rs.get_state()), (st_split, st_draw)):
            np.testing.assert_array_equal(a[1], b[1])
            assert a[2] == b[2]
    print(f"{model_name}: {undecided} of {columns} columns undecided")
    assert columns > 0 and undecided <= R.UNDECIDED_CAP * columns


@pytest.mark.parametrize("model_name", list(MODELS))
def test_split_trains_two_epochs(model_name, tmp_path, monkeypatch):
    from fairrec import functional as F
    from fairrec.quick_start import run_recbole
    calls, seen = [], {}
    real = F.dyn_neg_mlp_select

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(F, "dyn_neg_mlp_select", counting)
    cfg = dict({"device": DEV, "epochs": 2, "eval_step": 0, "train_batch_size": 256, "embedding_size": D,
                "neg_sampling": {"uniform": 1, "dynamic": 4}, "checkpoint_dir": str(tmp_path), "synthetic_users": 150,
                "synthetic_items": 300, "synthetic_interactions": 4000, "seed": 9, "dynamic_neg_scorer": "split"},
               **MODELS[model_name])
    run_recbole(model=model_name, config_dict=cfg, saved=False,
                before_fit=lambda model, trainer: seen.update(model=model, trainer=trainer))
    losses = dict(seen["trainer"].train_loss_dict)
    flat = [float(x) for v in losses.values() for x in (v if isinstance(v, (tuple, list)) else [v])]
    assert len(losses) == 2 and np.isfinite(flat).all(), losses
    assert len(calls) >= 2                                       # every batch's negatives came from the kernel
    eng = seen["model"].hip_engine()
    eng.check_device_errors()
    assert all(t._pending is None for t in eng._tables.values())
    for p in seen["model"].parameters():
        assert torch.isfinite(p).all()


@pytest.mark.parametrize("key", [None, "pairs"])
@pytest.mark.parametrize("model_name", list(MODELS))
def test_pairs_is_the_parent_s_path_bit_for_bit(model_name, key, tmp_path):
    dl, model, _ = _setup(model_name, tmp_path, **({} if key is None else {"dynamic_neg_scorer": key}))
    assert model.dynamic_neg_scorer == "pairs"
    _set_scorer(model)
    cur = dl.dataset[0:dl.step]
    rs = dl.sampler.rs
    st0 = rs.get_state()
    cand = dl.sampler.sample_by_user_ids(cur[dl.uid_field], cur[dl.iid_field], NUM * M).to(DEV)
    assert model.dyn_neg_select(cur, cand, NUM, M) is None
    rs.set_state(st0)
    model.train()
    got = _batches_with(dl)
    st_got = rs.get_state()
    rs.set_state(st0)
    want = _batches_with(dl, _restated)
    st_want = rs.get_state()
    assert len(got) == len(want) > 1
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.keys() == b.keys()
        for col in a:
            assert torch.equal(a[col], b[col]), (k, col)
    np.testing.assert_array_equal(st_got[1], st_want[1])
    assert st_got[2] == st_want[2]


def test_a_bad_key_value_raises(tmp_path):
    for model_name in MODELS:
        with pytest.raises(ValueError, match="dynamic_neg_scorer"):
            _setup(model_name, tmp_path, dynamic_neg_scorer="fused")


def test_filtered_pfcn_mlp_still_raises(tmp_path):
    from fairrec.config import Config
    from fairrec.data.dataset import synthetic_dataset
    from fairrec.utils import get_model
    cfg = Config(model="PFCN_MLP", config_dict={"device": DEV, "embedding_size": D, "filter_mode": "sm",
                                                "mlp_hidden_size_list": [32, 16], "dis_hidden_size_list": [16, 8],
                                                "dynamic_neg_scorer": "split", "checkpoint_dir": str(tmp_path)})
    ds = synthetic_dataset(cfg, 150, 300, 4000, seed=5)
    model = get_model("PFCN_MLP")(cfg, ds).to(DEV)
    cand = torch.randint(1, 300, (8,), device=DEV)
    with pytest.raises(NotImplementedError, match="filter_mode"):
        model.dyn_neg_select(ds[0:2], cand, 1, 4)


@pytest.mark.parametrize("model_name", list(MODELS))
def test_a_batchnorm_scorer_falls_back_to_predict(model_name, tmp_path):
    from fairrec.model.layers import MLPLayers
    dl, model, trainer = _setup(model_name, tmp_path, dynamic_neg_scorer="split")
    name = "mlp_layers" if hasattr(model, "mlp_layers") else "mlp_layer"
    old = getattr(model, name)
    torch.manual_seed(3)
    setattr(model, name, MLPLayers(list(old.layers), dropout=old.dropout, bn=True).to(DEV))
    model._engine = None                                         # (built over the scorer's parameters)
    trainer = type(trainer)(trainer.config, model)
    cur = dl.dataset[0:dl.step]
    rs = dl.sampler.rs
    st0 = rs.get_state()
    cand = dl.sampler.sample_by_user_ids(cur[dl.uid_field], cur[dl.iid_field], NUM * M).to(DEV)
    model.eval()
    with torch.no_grad():
        assert model.dyn_neg_select(cur, cand, NUM, M) is None
    model.train()
    rs.set_state(st0)
    neg = dl._dynamic_negatives(cur)
    rs.set_state(st0)
    assert torch.equal(neg, _restated(dl, cur))

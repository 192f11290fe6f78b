"""GPU: dynamic negative sampling on the device.

- fr_dyn_neg_select against torch.max(dim=0) + the advanced index of the reference's dynamic branch;
- fr_dyn_neg_dot_select against the composed device path (fr_table_gather + RowDot + biases + torch.sigmoid + torch.max),
  and its scores against torch.sigmoid's bits;
- the loader against a plain-torch restatement of abstract_dataloader.py `_neg_sampling` (dynamic branch), per model;
- two-epoch training runs against the same runs with the restatement in the loader."""
import numpy as np
import pytest
import torch

from fairrec import _C
from fairrec.functional import RowDot, dyn_neg_dot_select, dyn_neg_select
from fairrec.optim import AdamHyper, LazyTable

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _torch_pick(scores, cand):
    idx = torch.max(scores, dim=0)[1]
    return cand[idx, torch.arange(cand.shape[1], device=cand.device)]


# ---- fr_dyn_neg_select -----------------------------------------------------------------------------------------------
def _select_cases():
    g = torch.Generator(device="cpu").manual_seed(7)
    cases = {}
    for M, num, n in ((4, 1, 1000), (4, 3, 333), (1, 1, 130), (1, 3, 65), (16, 2, 77), (8, 1, 4097)):
        cases[f"random-M{M}-num{num}-n{n}"] = torch.randn(M, num * n, generator=g)
    s = torch.randn(5, 200, generator=g)
    s[:, :50] = 0.25                                   # whole columns equal
    s[2, 50:100] = 9.0
    s[4, 50:100] = 9.0                                 # tie between rows 2 and 4
    s[1, 100:120] = float("nan")                       # NaN before the maximum
    s[3, 120:140] = 50.0
    s[4, 120:140] = float("nan")                       # NaN after the maximum
    s[1, 140:160] = float("nan")
    s[3, 140:160] = float("nan")                       # two NaNs
    s[0, 160:170] = float("inf")
    s[3, 160:170] = float("inf")                       # +inf tie
    s[:, 170:180] = -float("inf")                      # all -inf
    s[2, 180:190] = -float("inf")
    cases["ties-nan-inf"] = s
    cases["large"] = torch.randn(2, (1 << 20) + 3, generator=g)
    return cases


@pytest.mark.parametrize("name", list(_select_cases()))
def test_select_equals_torch_max(name):
    s = _select_cases()[name].to(DEV)
    M, cols = s.shape
    cand = torch.randint(1, 1 << 40, (M, cols), device=DEV)
    got = dyn_neg_select(s, cand)
    np.testing.assert_array_equal(got.cpu().numpy(), _torch_pick(s, cand).cpu().numpy())


# ---- fr_dyn_neg_dot_select -------------------------------------------------------------------------------------------
def _aged_table(n_rows, D, steps, hyper, g, scale=0.1):
    w = (torch.randn(n_rows, D, generator=g) * scale).to(DEV)
    t = LazyTable(w)
    t.ensure_state()
    t.m.copy_(torch.randn(n_rows, D, generator=g).to(DEV) * 1e-2)
    t.v.copy_(torch.rand(n_rows, D, generator=g).to(DEV) * 1e-3)
    t.last.copy_(torch.randint(0, steps + 1, (n_rows,), generator=g, dtype=torch.int32).to(DEV))  # rows left behind
    t.step = steps
    return t


def _composed(tab, hyper, ue, cand, num, M, ib=None, ub=None, gb=None):
    """predict() of PFCNBase on the repeated interaction, then the reference's torch.max pick."""
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    rows = tab.gather(hyper, cand, err)
    score = RowDot.apply(ue.repeat(num * M, 1), rows).unsqueeze(-1)
    if ub is not None:
        score = score + ub.view(-1, 1).repeat(num * M, 1) + ib[0].gather(ib[1], cand, err) + gb
    score = torch.sigmoid(score)
    return score.view(-1), _torch_pick(score.reshape(M, -1), cand.view(M, -1))


@pytest.mark.parametrize("D", [64, 128, 32, 200])
@pytest.mark.parametrize("biased", [False, True])
@pytest.mark.parametrize("M,num", [(1, 1), (4, 1), (4, 2), (5, 3)])
@pytest.mark.parametrize("scale", [0.1, 3.0])       # 3.0: logits far beyond +-20, sigmoid saturates and ties decide
def test_dot_select_equals_the_composed_path(D, biased, M, num, scale):
    g = torch.Generator(device="cpu").manual_seed(D * 131 + M * 7 + num + int(biased) * 1000)
    hyper = AdamHyper(lr=1e-2, weight_decay=1e-3 if biased else 0.0, device=DEV)
    n_items, n = 3000, 517
    tab = _aged_table(n_items, D, 9, hyper, g, scale=0.1 if scale < 1 else 1.0)
    ue = (torch.randn(n, D, generator=g) * scale).to(DEV)
    cand = torch.randint(0, n_items, (M * num * n,), generator=g).to(DEV)
    ib = ub = gb = None
    if biased:
        ib = (_aged_table(n_items, 1, 9, hyper, g, scale=scale), hyper)
        ub = (torch.randn(n, generator=g) * scale).to(DEV)
        gb = torch.tensor(0.1, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    want_scores, want = _composed(tab, hyper, ue, cand, num, M, ib, ub, gb)
    got = dyn_neg_dot_select(tab, hyper, ue, cand, num, M, err, item_bias=ib, user_bias=ub, global_bias=gb)
    scores = dyn_neg_dot_select(tab, hyper, ue, cand, num, M, err, item_bias=ib, user_bias=ub, global_bias=gb,
                                scores_only=True)
    assert int(err.item()) == 0
    np.testing.assert_array_equal(scores.cpu().view(torch.int32).numpy(), want_scores.cpu().view(torch.int32).numpy())
    np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())
    if scale > 1:
        assert (want_scores == 1.0).any()                 # saturated: the pick among equal scores was exercised


def test_dot_select_flags_an_id_out_of_range():
    g = torch.Generator(device="cpu").manual_seed(3)
    hyper = AdamHyper(device=DEV)
    tab = _aged_table(100, 64, 2, hyper, g)
    ue = torch.randn(10, 64, generator=g).to(DEV)
    cand = torch.randint(0, 100, (20,), generator=g).to(DEV)
    cand[13] = 100
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    dyn_neg_dot_select(tab, hyper, ue, cand, 1, 2, err)
    assert int(err.item()) & _C.DEV_ERR_INDEX_RANGE


def test_dot_select_at_size():
    """n = 8192, D = 128, M = 8 over 1 M items: the fused pick equals the composed one."""
    g = torch.Generator(device="cpu").manual_seed(11)
    hyper = AdamHyper(lr=1e-3, device=DEV)
    n_items, n, D, M = 1 << 20, 8192, 128, 8
    tab = _aged_table(n_items, D, 5, hyper, g)
    ib = (_aged_table(n_items, 1, 5, hyper, g), hyper)
    ue = (torch.randn(n, D, generator=g) * 0.3).to(DEV)
    ub = torch.randn(n, generator=g).to(DEV)
    gb = torch.tensor(0.1, device=DEV)
    cand = torch.randint(1, n_items, (M * n,), generator=g).to(DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    _, want = _composed(tab, hyper, ue, cand, 1, M, ib, ub, gb)
    got = dyn_neg_dot_select(tab, hyper, ue, cand, 1, M, err, item_bias=ib, user_bias=ub, global_bias=gb)
    assert int(err.item()) == 0
    np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())


# ---- the loader against the restatement --------------------------------------------------------------------------------
def restated_dynamic_negatives(loader, inter_feat):
    """abstract_dataloader.py `_neg_sampling`, dynamic branch, in plain torch on the device with the same sampler/model."""
    from fairrec.data.interaction import Interaction
    candidate_num = loader.candidate_num
    num = loader.neg_sample_num
    model = loader.model
    user_ids, item_ids = inter_feat[loader.uid_field], inter_feat[loader.iid_field]
    neg_candidate_ids = loader.sampler.sample_by_user_ids(user_ids, item_ids, num * candidate_num)
    model.eval()
    interaction = inter_feat.repeat(num * candidate_num)
    interaction.update(Interaction({loader.iid_field: neg_candidate_ids.to(user_ids.device)}))
    with torch.no_grad():
        scores = model.predict(interaction).reshape(candidate_num, -1)
    indices = torch.max(scores, dim=0)[1].detach()
    neg_candidate_ids = neg_candidate_ids.reshape(candidate_num, -1)
    neg_item_ids = neg_candidate_ids[indices, [i for i in range(neg_candidate_ids.shape[1])]].view(-1)
    model.train()
    return neg_item_ids


MODELS = ["PFCN_PMF", "PFCN_BiasedMF", "PFCN_MLP", "PFCN_DMF", "NFCF", "FairGo_PMF"]


def _setup(model_name, M, num, ck_dir, seed=5):
    from fairrec.config import Config
    from fairrec.data.dataloader import TrainDataLoader
    from fairrec.data.dataset import synthetic_dataset
    from fairrec.quick_start import split_dataset
    from fairrec.sampler import Sampler
    from fairrec.utils import get_model, get_trainer, init_seed
    cfg = Config(model=model_name, config_dict={"device": DEV, "train_batch_size": 200, "embedding_size": 64,
                                                "filter_mode": "none", "neg_sampling": {"uniform": num, "dynamic": M},
                                                "checkpoint_dir": str(ck_dir), "seed": seed})
    init_seed(cfg["seed"], cfg["reproducibility"])
    ds = synthetic_dataset(cfg, 300, 250, 4000, seed=seed)
    tr, va, te = split_dataset(ds)
    sampler = Sampler(["train", "valid", "test"], [tr, va, te], "uniform", device=DEV).set_phase("train")
    dl = TrainDataLoader(cfg, tr.to(DEV), sampler=sampler, shuffle=False)
    model = get_model(model_name)(cfg, dl.dataset).to(DEV)
    trainer = get_trainer(None, model_name)(cfg, model)
    dl.get_model(model)
    return dl, model, trainer


def _bn_stats(model):
    return [b.clone() for n, b in model.named_buffers()]


@pytest.mark.parametrize("model_name", MODELS)
@pytest.mark.parametrize("M,num", [(1, 1), (4, 1), (1, 2), (4, 2)])
def test_loader_equals_the_restatement(model_name, M, num, tmp_path):
    from fairrec.data import dataloader as D
    dl, model, _ = _setup(model_name, M, num, tmp_path)
    rs = dl.sampler.rs
    st0 = rs.get_state()
    stats0 = _bn_stats(model)
    model.train()
    got = [b.interaction for b in dl]
    st_got = rs.get_state()
    assert model.training
    for a, b in zip(stats0, _bn_stats(model)):
        assert torch.equal(a, b)
    eng = model.hip_engine()
    assert all(t._pending is None for t in eng._tables.values())
    rs.set_state(st0)
    orig = D.TrainDataLoader._dynamic_negatives
    D.TrainDataLoader._dynamic_negatives = restated_dynamic_negatives
    try:
        want = [b.interaction for b in dl]
    finally:
        D.TrainDataLoader._dynamic_negatives = orig
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.keys() == b.keys()
        for col in a:
            assert torch.equal(a[col], b[col]), (k, col)
    st_want = rs.get_state()
    np.testing.assert_array_equal(st_got[1], st_want[1])
    assert st_got[2] == st_want[2]


# ---- trainer level --------------------------------------------------------------------------------------------------
def _run(model_name, restated, tmp_path):
    from fairrec.data import dataloader as D
    from fairrec.quick_start import run_recbole
    seen = {}

    def before_fit(model, trainer):
        seen["model"], seen["trainer"] = model, trainer

    cfg = {"device": DEV, "epochs": 2, "eval_step": 0, "train_batch_size": 256, "embedding_size": 64,
           "filter_mode": "none", "neg_sampling": {"uniform": 1, "dynamic": 4}, "checkpoint_dir": str(tmp_path),
           "synthetic_users": 300, "synthetic_items": 250, "synthetic_interactions": 5000, "seed": 9}
    from fairrec.model.layers import MLPLayers
    orig, n_mlps = D.TrainDataLoader._dynamic_negatives, MLPLayers._instances
    if restated:
        D.TrainDataLoader._dynamic_negatives = restated_dynamic_negatives
    MLPLayers._instances = 0          # dropout seeds count the MLPs built in the process: both runs start from the same count
    try:
        run_recbole(model=model_name, config_dict=cfg, saved=False, before_fit=before_fit)
    finally:
        D.TrainDataLoader._dynamic_negatives, MLPLayers._instances = orig, n_mlps
    sd = {k: v.detach().clone() for k, v in seen["model"].state_dict().items()}
    return dict(seen["trainer"].train_loss_dict), sd


@pytest.mark.parametrize("model_name", ["PFCN_BiasedMF", "NFCF"])
def test_training_equals_the_restated_loader(model_name, tmp_path):
    loss_a, sd_a = _run(model_name, False, tmp_path)
    loss_b, sd_b = _run(model_name, True, tmp_path)
    assert loss_a == loss_b
    assert sd_a.keys() == sd_b.keys()
    for k in sd_a:
        assert torch.equal(sd_a[k], sd_b[k]), k

"""GPU: Trainer.fit with learner sgd / adagrad / rmsprop (weight decay on) against a plain-torch restatement.

The restatement drives the oracle's model math (oracle/nfcf.py, oracle/pfcn.py) on the batches the trainer ran -- recorded
step by step, with the attribute subset and the filter / discriminator phase of each step -- through stock
torch.optim.<Learner> optimizers over the same parameter groups the trainer builds.  Dropout is 0, batches are fixed
(no shuffle, negatives in the dataset).  Checked: every step's loss and the per-epoch losses at rtol 1e-4, the final
parameters within the Adam trainer tests' bound |a - b| <= 1e-4 |b| + 1e-6 (tests/test_trainer_hip.py).  (The e2e tests' tighter
band, 2e-6 of a tensor's largest value, is exceeded by Adam itself on the BatchNorm-fed discriminator / filter weights of
this small run: fp32 reduction order, up to ~1e-6 absolute on weights of ~0.04.)

Checkpoints: half-way, the restatement's optimizer is REPLACED by a fresh stock optimizer loaded from the fused optimizer's
`state_dict(param_names=...)` and the run continues from there -- a wrong index mapping or a wrong sum / square_avg / step
makes the second epoch diverge.  And a stock optimizer's state dict (with the restated weights) resumes a fresh trainer
through `resume_checkpoint`: its next epoch equals the restatement's."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, WD = 1e-3, 1e-3          # (the reference configs' learning rate)
LEARNERS = ("sgd", "adagrad", "rmsprop")
STOCK = {"sgd": torch.optim.SGD, "adagrad": torch.optim.Adagrad, "rmsprop": torch.optim.RMSprop}


def _data(model_name, cfg):
    from fairrec.data.dataset import InteractionDataset
    from fairrec.data.interaction import Interaction
    g = torch.Generator().manual_seed(21)
    n_users, n_items, n = 80, 60, 960
    cols = {"user_id": torch.randint(1, n_users, (n,), generator=g), "item_id": torch.randint(1, n_items, (n,), generator=g)}
    if model_name == "NFCF":
        cols["label"] = (torch.rand(n, generator=g) < 0.5).float()
    else:
        cols["neg_item_id"] = torch.randint(1, n_items, (n,), generator=g)
    users = {"user_id": torch.arange(n_users), "gender": (torch.rand(n_users, generator=g) < 0.5).float(),
             "age": torch.randint(0, 3, (n_users,), generator=g)}
    users["gender"][1:3] = torch.tensor([0.0, 1.0])
    users["age"][1:4] = torch.tensor([0, 1, 2])
    return InteractionDataset(cfg, Interaction(cols), Interaction(users), n_users, n_items)


def _setup(tmp_path, model_name, learner, mode=None, epochs=2):
    from fairrec.config import Config
    from fairrec.data.dataloader import TrainDataLoader
    from fairrec.utils import get_model, get_trainer, init_seed
    d = {"embedding_size": 16, "train_batch_size": 160, "epochs": epochs, "device": DEV, "checkpoint_dir": str(tmp_path),
         "learning_rate": LR, "weight_decay": WD, "learner": learner, "neg_sampling": None, "graph_train_step": False,
         "eval_step": 0}
    if model_name == "NFCF":
        d.update(mlp_hidden_size=[32, 16], dropout=0.0, fair_weight=0.1, load_pretrain_path=None, sst_attr_list=["gender"])
    else:
        d.update(sst_attr_list=["gender", "age"], filter_mode=mode, dis_hidden_size_list=[16, 8], dis_dropout=0.0,
                 train_epoch_interval=1)
    cfg = Config(model=model_name, config_dict=d)
    init_seed(7)
    ds = _data(model_name, cfg)
    loader = TrainDataLoader(cfg, ds, shuffle=False)
    model = get_model(model_name)(cfg, ds).to(DEV)
    trainer = get_trainer(None, model_name)(cfg, model)
    return cfg, ds, loader, model, trainer


class _Listen:
    """Every optimizer step the trainer runs: (epoch, kind L / D, attribute subset, batch columns, loss)."""

    def __init__(self, model, trainer):
        self.steps, self.epoch = [], 0
        for kind, name in (("L", "calculate_loss"), ("D", "calculate_dis_loss")):
            fn = getattr(model, name, None)
            if fn is not None:
                setattr(model, name, self._wrap(kind, fn))
        orig = trainer._train_epoch

        def epoch(train_data, epoch_idx, *a, **kw):
            self.epoch = epoch_idx
            return orig(train_data, epoch_idx, *a, **kw)
        trainer._train_epoch = epoch

    def _wrap(self, kind, fn):
        def wrapped(interaction, *args, **kw):
            out = fn(interaction, *args, **kw)
            sst = args[0] if args else kw.get("sst_list")
            self.steps.append((self.epoch, kind, list(sst) if sst else None,
                               {k: v.detach().cpu().clone() for k, v in interaction.interaction.items()},
                               float(out.detach().reshape(-1)[0])))
            return out
        return wrapped


# ---- restatements ------------------------------------------------------------------------------------------------------
class _NfcfRef:
    def __init__(self, model, ds):
        from oracle import nfcf as O
        self.O = O
        sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        self.stage = "pretrain" if model.user_embedding.weight.requires_grad else "finetune"
        self.fw = float(model.fair_weight) if hasattr(model, "fair_weight") else 0.1
        self.U = sd["user_embedding.weight"].requires_grad_(self.stage == "pretrain")
        self.I = sd["item_embedding.weight"].requires_grad_()
        n_l = len([k for k in sd if k.startswith("mlp_layers.mlp_layers.") and k.endswith(".weight")])
        self.Ws = [sd[f"mlp_layers.mlp_layers.{3 * l + 1}.weight"].requires_grad_() for l in range(n_l)]
        self.bs = [sd[f"mlp_layers.mlp_layers.{3 * l + 1}.bias"].requires_grad_() for l in range(n_l)]
        self.gender = ds.user_feat["gender"].float()
        self.named = {"user_embedding.weight": self.U, "item_embedding.weight": self.I}
        for l in range(n_l):
            self.named[f"mlp_layers.mlp_layers.{3 * l + 1}.weight"] = self.Ws[l]
            self.named[f"mlp_layers.mlp_layers.{3 * l + 1}.bias"] = self.bs[l]

    def groups(self):
        return {None: [p for p in self.named.values() if p.requires_grad]}

    def step_loss(self, kind, sst, cols):
        u, i, lab = cols["user_id"], cols["item_id"], cols["label"].float()
        s = None if self.stage == "pretrain" else (cols["gender"].float() if "gender" in cols else self.gender[u])
        l, _ = self.O.loss(self.stage, self.fw, self.U, self.I, self.Ws, self.bs, u, i, lab, s)
        return None, l

    def params(self):
        return {k: v.detach().numpy() for k, v in self.named.items()}


class _PfcnRef:
    def __init__(self, model, cfg, ds):
        from oracle import pfcn as O
        self.mode = cfg["filter_mode"]
        attrs = list(cfg["sst_attr_list"])
        z = {"model": np.array("PFCN_BiasedMF"), "mode": np.array(self.mode), "attrs": np.array(attrs),
             "hyper": np.array([LR, WD, float(cfg["dis_weight"]), 0.0])}
        for k, v in model.state_dict().items():
            z["init.model." + k] = v.detach().cpu().numpy().copy()
        for i, mlp in (getattr(model, "filter_layer", None) or {}).items():
            for k, v in mlp.state_dict().items():
                z[f"init.filter.{i}.{k}"] = v.detach().cpu().numpy().copy()
        for a, mlp in (getattr(model, "dis_layer_dict", None) or {}).items():
            for k, v in mlp.state_dict().items():
                z[f"init.dis.{a}.{k}"] = v.detach().cpu().numpy().copy()
        self.m = O.Model(z)
        self.users = {a: ds.user_feat[a] for a in ("gender", "age")}

    def groups(self):
        if self.mode == "none":
            return {None: self.m.all_params()}
        return {"filter": self.m.filter_params(), "dis": self.m.dis_params()}

    def step_loss(self, kind, sst, cols):
        u, pos, neg = cols["user_id"], cols["item_id"], cols["neg_item_id"]
        labels = {a: v[u] for a, v in self.users.items()}
        if kind == "L":
            return ("filter" if self.mode != "none" else None), self.m.loss(u, pos, neg, sst, labels, None)
        return "dis", self.m.dis_loss(u, sst, labels, None)

    def params(self):
        m = self.m
        out = {"user_embedding_layer.weight": m.U, "item_embedding_layer.weight": m.I, "user_bias.weight": m.bu,
               "item_bias.weight": m.bi, "global_bias": m.gb}
        out = {k: v.detach().numpy() for k, v in out.items()}
        for tag, d in (("filter_layer", m.filters), ("dis_layer_dict", m.dis)):
            for key, mlp in d.items():
                ex = {}
                mlp.export("x", ex)
                out.update({f"{tag}.{key}.{k[2:]}": v for k, v in ex.items()})
        return out


def _fused_params(model):
    out = {k: v.detach().float().cpu().numpy() for k, v in model.state_dict().items()}
    for attr in ("filter_layer", "dis_layer_dict"):
        d = getattr(model, attr, None)
        if isinstance(d, dict):
            for key, mlp in d.items():
                for k, v in mlp.state_dict().items():
                    out[f"{attr}.{key}.{k}"] = v.detach().float().cpu().numpy()
    return out


def _restate(ref, steps, learner, swap_at_epoch=None, fused_sd=None, names=None):
    """Run the recorded steps on the restatement with stock optimizers; at the first step of `swap_at_epoch` the optimizer
    of group None is rebuilt from `fused_sd` (torch's integer layout over `names`)."""
    opts = {g: STOCK[learner](ps, lr=LR, weight_decay=WD) for g, ps in ref.groups().items()}
    losses = []
    swapped = False
    for ep, kind, sst, cols, _ in steps:
        if swap_at_epoch is not None and ep == swap_at_epoch and not swapped:
            params = [ref.named[n] for n in names]
            opt = STOCK[learner](params, lr=LR, weight_decay=WD)
            opt.load_state_dict({"state": {k: {n: (v.cpu() if torch.is_tensor(v) else v) for n, v in st.items()}
                                           for k, st in fused_sd["state"].items()},
                                 "param_groups": fused_sd["param_groups"]})
            opts[None] = opt
            swapped = True
        g, l = ref.step_loss(kind, sst, cols)
        opt = opts[g]
        opt.zero_grad(set_to_none=True)
        losses.append(float(l.item()))
        l.backward()
        opt.step()
    return losses, opts


def _compare(fused, want, what):
    worst = (0.0, "")
    for name, ref in want.items():
        if name not in fused:
            continue
        # (a Linear bias that feeds BatchNorm has a true gradient of exactly 0: rounding noise of either side is turned into
        # steps by the adaptive learners and never reaches an output -- as in tests/test_e2e_hip.py; so is running_mean)
        if name.startswith(("filter_layer.", "dis_layer_dict.")) and (name.endswith("running_mean") or (
                name.endswith(".bias") and np.ndim(want.get(name.replace(".bias", ".weight"))) == 2)):
            continue
        if name.endswith(("running_var", "num_batches_tracked")):
            continue
        ref = np.asarray(ref, np.float64)
        ratio = float((np.abs(fused[name] - ref) / (1e-4 * np.abs(ref) + 1e-6)).max())
        if ratio > worst[0]:
            worst = (ratio, name)
    assert worst[0] <= 1.0, (what, worst)


def _check_losses(lis, ref_losses, trainer, epochs):
    got = [l for *_, l in lis.steps]
    assert len(got) == len(ref_losses)
    np.testing.assert_allclose(got, ref_losses, rtol=1e-4, atol=1e-7)
    for e in epochs:
        idx = [k for k, s in enumerate(lis.steps) if s[0] == e]
        np.testing.assert_allclose(trainer.train_loss_dict[e], sum(ref_losses[k] for k in idx), rtol=1e-4)


@pytest.mark.parametrize("model_name,mode", [("NFCF", None), ("PFCN_BiasedMF", "none"), ("PFCN_BiasedMF", "sm")])
@pytest.mark.parametrize("learner", LEARNERS)
def test_two_epoch_fit_matches_plain_torch(tmp_path, learner, model_name, mode):
    cfg, ds, loader, model, trainer = _setup(tmp_path, model_name, learner, mode)
    ref = _NfcfRef(model, ds) if model_name == "NFCF" else _PfcnRef(model, cfg, ds)
    lis = _Listen(model, trainer)
    trainer.fit(loader, None, verbose=False, saved=False)
    assert {s[0] for s in lis.steps} == {0, 1}
    if mode == "sm":
        assert {s[1] for s in lis.steps} == {"L", "D"}
    ref_losses, _ = _restate(ref, lis.steps, learner)
    _check_losses(lis, ref_losses, trainer, (0, 1))
    _compare(_fused_params(model), ref.params(), f"{learner} {model_name} {mode}")


@pytest.mark.parametrize("learner", LEARNERS)
def test_checkpoint_continues_in_stock_torch_and_resumes_from_it(tmp_path, learner):
    # (1) the fused state after epoch 0 drives a stock optimizer through epoch 1: same weights as the fused run
    cfg, ds, loader, model, trainer = _setup(tmp_path, "NFCF", learner, epochs=1)
    ref = _NfcfRef(model, ds)
    lis = _Listen(model, trainer)
    names = [n for n, _ in model.named_parameters()]
    trainer.fit(loader, None, verbose=False, saved=False)
    # (a state dict holds the live state tensors, as torch's does: copy it before training on)
    sd = trainer.optimizer.state_dict(param_names=names)
    sd = {"state": {k: {n: (v.detach().clone() if torch.is_tensor(v) else v) for n, v in st.items()}
                    for k, st in sd["state"].items()}, "param_groups": sd["param_groups"]}
    if learner == "sgd":
        assert sd["state"] == {}
    else:
        key = "sum" if learner == "adagrad" else "square_avg"
        assert all(st[key].shape == dict(model.named_parameters())[names[k]].shape for k, st in sd["state"].items())
    if learner == "adagrad":
        assert sorted(sd["state"]) == list(range(len(names)))
    trainer.epochs = 2
    trainer.start_epoch = 1
    trainer.fit(loader, None, verbose=False, saved=False)
    # the restatement runs epoch 0 with its own stock optimizer, then epoch 1 with one LOADED from the fused state dict
    for n in names:
        assert n in ref.named, n
    ref_losses, opts = _restate(ref, lis.steps, learner, swap_at_epoch=1, fused_sd=sd, names=names)
    _check_losses(lis, ref_losses, trainer, (0, 1))
    _compare(_fused_params(model), ref.params(), f"{learner}: stock optimizer continued from the fused state")

    # (2) resume_checkpoint with the stock optimizer's state dict and the restated weights: a fresh trainer's next epoch
    # equals the restatement continued with its own optimizer
    stock_sd = opts[None].state_dict()
    model_sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for k, p in ref.named.items():
        model_sd[k] = p.detach().clone()
    ck = os.path.join(str(tmp_path), "stock.pth")
    torch.save({"epoch": 1, "cur_step": 0, "best_valid_score": 0.0, "state_dict": model_sd, "other_parameter": None,
                "optimizer": stock_sd}, ck)
    cfg2, ds2, loader2, model2, trainer2 = _setup(tmp_path / "r", "NFCF", learner, epochs=3)
    trainer2.resume_checkpoint(ck)
    assert trainer2.start_epoch == 2
    lis2 = _Listen(model2, trainer2)
    trainer2.fit(loader2, None, verbose=False, saved=False)
    assert {s[0] for s in lis2.steps} == {2}
    ref_losses2, _ = _restate_continue(ref, lis2.steps, opts[None])
    _check_losses(lis2, ref_losses2, trainer2, (2,))
    _compare(_fused_params(model2), ref.params(), f"{learner}: resumed from a stock optimizer's checkpoint")


def _restate_continue(ref, steps, opt):
    losses = []
    for ep, kind, sst, cols, _ in steps:
        _, l = ref.step_loss(kind, sst, cols)
        opt.zero_grad(set_to_none=True)
        losses.append(float(l.item()))
        l.backward()
        opt.step()
    return losses, opt

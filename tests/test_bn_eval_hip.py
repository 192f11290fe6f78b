"""GPU: BatchNorm on running statistics at inference -- `MLPLayers` in eval mode (one fr_mlp_infer launch, no buffer touched)
and the PFCN family's opt-in `filter_eval_statistics: running`: a user's filtered embedding is a function of that user
alone, scoring mutates nothing, the default stays the reference's behaviour, and the key does not change what is learnt."""
import copy

import numpy as np
import pytest
import torch

import mlp_infer_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = 10

# the small synthetic configuration of tests/test_case_study_hip.py
COMMON = {"epochs": 1, "train_batch_size": 512, "synthetic_users": 150, "synthetic_items": 300, "synthetic_interactions": 4000,
          "device": DEV, "embedding_size": 16, "eval_args": {"mode": "full"}, "topk": [5, 10], "valid_metric": "ndcg@10",
          "valid_metric_bigger": True, "metrics": ["NDCG", "Recall", "Hit", "MRR"], "sst_attr_list": ["gender"],
          "eval_batch_size": 4096, "metric_decimal_place": 4, "dis_hidden_size_list": [16, 8], "train_epoch_interval": 1,
          "learning_rate": 0.01}
MODELS = {"PFCN_BiasedMF-sm": ("PFCN_BiasedMF", "sm"), "PFCN_PMF-cm": ("PFCN_PMF", "cm"), "PFCN_MLP-sm": ("PFCN_MLP", "sm")}


def _bits(t):
    return t.detach().clone().contiguous().view(torch.int32 if t.dtype == torch.float32 else t.dtype)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _run(model_name, tmp_path, **extra):
    """(model, trainer, test loader) of a finished run_recbole."""
    from fairrec.data.dataloader import FullSortEvalDataLoader
    from fairrec.model.layers import MLPLayers
    from fairrec.quick_start import run_recbole
    MLPLayers._instances = 0      # the dropout streams are seeded by construction rank: every run starts as a fresh program would
    seen, loaders = {}, []
    init = FullSortEvalDataLoader.__init__

    def recording_init(self, *a, **kw):
        init(self, *a, **kw)
        loaders.append(self)

    def before_fit(m, trainer):
        seen["model"], seen["trainer"] = m, trainer

    FullSortEvalDataLoader.__init__ = recording_init
    try:
        run_recbole(model=model_name, config_dict=dict(COMMON, checkpoint_dir=str(tmp_path), **extra), saved=False,
                    before_fit=before_fit)
    finally:
        FullSortEvalDataLoader.__init__ = init
    return seen["model"], seen["trainer"], loaders[-1]          # the test loader is built last


_trained = {}


@pytest.fixture
def trained(request, tmp_path_factory):
    """A model trained once per module with filter_eval_statistics: running."""
    case = request.param
    if case not in _trained:
        name, mode = MODELS[case]
        _trained[case] = _run(name, tmp_path_factory.mktemp(case), filter_mode=mode, filter_eval_statistics="running")
    return _trained[case]


def _filter_buffers(model):
    return [_bits(b) for i in sorted(model.filter_layer) for b in model.filter_layer[i].buffers()]


# ---- MLPLayers in eval mode -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers, dropout", [([16, 32, 16], 0.0), ([16, 16, 8, 1], 0.3)])
def test_mlplayers_eval_mode(layers, dropout):
    from fairrec.model.layers import MLPLayers
    torch.manual_seed(11)
    mlp = MLPLayers(layers, dropout=dropout, activation="leakyrelu", bn=True, init_method="norm").to(DEV)
    with torch.no_grad():
        for lin in mlp.linears():                       # (init 'norm' is N(0, 0.01): spread the weights so that every layer matters)
            lin.weight.mul_(25.0)
            lin.bias.normal_(0.0, 0.3)
        for bn in mlp.batchnorms():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0.0, 0.3)
    for i in range(3):                                  # the running statistics leave 0 and 1
        mlp(torch.randn(200 + 17 * i, layers[0], device=DEV) * (1.0 + i) + 0.5 * i)
    for bn in mlp.batchnorms():
        assert int(bn.num_batches_tracked) == 3 and float(bn.running_mean.abs().max()) > 0
    never_eval = copy.deepcopy(mlp)
    x = torch.randn(77, layers[0], device=DEV)
    mlp.eval()
    before = [_bits(b) for b in mlp.buffers()]
    with torch.no_grad():
        y1 = mlp(x)
        y2 = mlp(x)
    y, bound = R.forward_bound([R.net_of_module(mlp)], x.cpu().numpy())
    err = np.abs(y1.cpu().numpy().astype(np.float64) - y)
    print(f"MLPLayers{layers} eval: max error / bound = {(err / bound).max():.3g}")
    assert y1.shape == (77, layers[-1]) and np.all(err <= bound)
    assert _same(y1, y2)                                # dropout is inactive
    assert all(torch.equal(a, _bits(b)) for a, b in zip(before, mlp.buffers()))
    with pytest.raises(NotImplementedError, match="no_grad"):
        mlp(x)
    assert all(torch.equal(a, _bits(b)) for a, b in zip(before, mlp.buffers()))
    mlp.train()
    xb = torch.randn(90, layers[0], device=DEV)
    assert _same(mlp(xb), never_eval(xb))               # back in training mode: the module that never left it
    for a, b in zip(mlp.buffers(), never_eval.buffers()):
        assert _same(a, b)


# ---- one user equals that user in a crowd ---------------------------------------------------------------------------------
@pytest.mark.parametrize("trained", list(MODELS), indirect=True)
def test_one_user_equals_that_user_in_a_crowd(trained):
    from fairrec.data.interaction import Interaction
    from fairrec.utils.case_study import full_sort_scores, full_sort_topk
    model, trainer, test_data = trained
    sst = ["gender"]
    every = test_data.uid_list
    ids = every.cpu().numpy()
    rng = np.random.default_rng(4)
    shuffled = rng.permutation(np.concatenate([ids, ids[:23]]))
    all_val, all_idx = full_sort_topk(every, model, test_data, K, sst_list=sst)
    all_scores = full_sort_scores(every, model, test_data, sst_list=sst)
    sh_val, sh_idx = full_sort_topk(shuffled, model, test_data, K, sst_list=sst)
    sh_scores = full_sort_scores(shuffled, model, test_data, sst_list=sst)
    for pos in (0, 7, 64, 101, len(ids) - 1):           # the last user of the list among them
        u = int(ids[pos])
        val, idx = full_sort_topk([u], model, test_data, K, sst_list=sst)
        scores = full_sort_scores([u], model, test_data, sst_list=sst)
        assert _same(val[0], all_val[pos]) and torch.equal(idx[0], all_idx[pos]) and _same(scores[0], all_scores[pos])
        at = int(np.flatnonzero(shuffled == u)[0])
        assert _same(val[0], sh_val[at]) and torch.equal(idx[0], sh_idx[at]) and _same(scores[0], sh_scores[at])
        open_cells = scores[0][~torch.isinf(scores[0])]
        assert bool(torch.isfinite(open_cells).all()) and float(open_cells.max()) > float(open_cells.min())
    ds = test_data.dataset
    inter = ds.join(Interaction({ds.uid_field: every})).to(DEV)
    model.eval()
    factors = [model.full_sort_factors(inter, sst, users_per_batch=per) for per in (1, 13, len(ids))]
    if type(model).__name__ == "PFCN_MLP":
        assert factors == [None, None, None]            # the dense path: a scorer of its own
    else:
        assert _same(factors[0]["X"], factors[1]["X"]) and _same(factors[0]["X"], factors[2]["X"])
    model.train()


@pytest.mark.parametrize("trained", list(MODELS), indirect=True)
def test_scoring_mutates_nothing(trained):
    from fairrec.utils.case_study import full_sort_topk
    model, trainer, test_data = trained
    before = _filter_buffers(model)
    assert before and any(int(b.abs().max()) for b in before)
    first = trainer.evaluate(test_data)
    second = trainer.evaluate(test_data)
    full_sort_topk(test_data.uid_list, model, test_data, K, sst_list=["gender"])
    assert first == second
    assert all(torch.equal(a, b) for a, b in zip(before, _filter_buffers(model)))
    model.eval()
    assert not any(m.training for m in model.filter_layer.values())
    assert all(m.training for m in model.dis_layer_dict.values())       # the discriminators keep the reference's behaviour
    model.train()
    assert all(m.training for m in model.filter_layer.values())


def test_the_default_is_untouched(tmp_path):
    model, trainer, test_data = _run("PFCN_BiasedMF", tmp_path, filter_mode="sm")
    assert model.filter_eval_statistics == "batch"
    model.eval()
    assert all(m.training for m in model.filter_layer.values())
    counts = [int(bn.num_batches_tracked) for m in model.filter_layer.values() for bn in m.batchnorms()]
    trainer.evaluate(test_data)
    after = [int(bn.num_batches_tracked) for m in model.filter_layer.values() for bn in m.batchnorms()]
    assert all(b > a for a, b in zip(counts, after))


def _equal_nested(a, b, path="optimizer"):
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and _same(a, b), path
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), path
        for k in a:
            _equal_nested(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _equal_nested(x, y, f"{path}[{i}]")
    else:
        assert a == b, path


def test_the_key_does_not_affect_training(tmp_path):
    runs = {}
    for stats in ("batch", "running"):
        d = tmp_path / stats
        d.mkdir()
        runs[stats] = _run("PFCN_BiasedMF", d, filter_mode="sm", filter_eval_statistics=stats, epochs=2, eval_step=1)
    (ma, ta, _), (mb, tb, _) = runs["batch"], runs["running"]
    sa, sb = ma.state_dict(), mb.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert _same(sa[k], sb[k]), k
    for group in ("filter_layer", "dis_layer_dict"):
        for key, mod in getattr(ma, group).items():
            other = getattr(mb, group)[key]
            for (n, p), (_, q) in zip(mod.named_parameters(), other.named_parameters()):
                assert _same(p, q), (group, key, n)
    for key, mod in ma.dis_layer_dict.items():          # nothing evaluates the discriminators: their buffers agree too
        for a, b in zip(mod.buffers(), mb.dis_layer_dict[key].buffers()):
            assert _same(a, b)
    _equal_nested(ta.optimizer_filter.state_dict(), tb.optimizer_filter.state_dict(), "optimizer_filter")
    _equal_nested(ta.optimizer_dis.state_dict(), tb.optimizer_dis.state_dict(), "optimizer_dis")
    # only the filters' BatchNorm buffers differ: `batch` advanced them in every evaluation
    na = [int(bn.num_batches_tracked) for m in ma.filter_layer.values() for bn in m.batchnorms()]
    nb = [int(bn.num_batches_tracked) for m in mb.filter_layer.values() for bn in m.batchnorms()]
    assert all(a > b for a, b in zip(na, nb))


@pytest.mark.parametrize("trained", ["PFCN_PMF-cm"], indirect=True)
def test_cm_with_several_filters_is_one_launch(trained):
    from fairrec.functional import mlp_infer
    from fairrec.model.layers import MLPLayers
    model, trainer, test_data = trained
    D = model.embedding_size
    filters, sst_dict = dict(model.filter_layer), dict(model.sst_dict)
    try:
        torch.manual_seed(5)
        for i, name in ((2, "second"), (3, "third")):   # the dicts are plain: a second and a third filter by hand
            mlp = MLPLayers([D, 2 * D, D], activation=model._filter_activation(), bn=True, init_method="norm").to(DEV)
            with torch.no_grad():
                for lin in mlp.linears():
                    lin.weight.mul_(25.0)
                for _ in range(3):
                    mlp(torch.randn(100, D, device=DEV) + 0.3 * i)
            model.filter_layer[i] = mlp
            model.sst_dict[name] = i
        model.eval()
        x = torch.randn(45, D, device=DEV)
        with torch.no_grad():
            got = model._filter(x, ["gender", "third"])
        pair = [model.filter_layer[1], model.filter_layer[3]]
        y, bound = R.forward_bound([R.net_of_module(m) for m in pair], x.cpu().numpy(), 3.0)
        assert np.all(np.abs(got.cpu().numpy().astype(np.float64) - y) <= bound)
        assert _same(got, mlp_infer(pair, x, out_div=3.0))
    finally:
        model.filter_layer.clear()
        model.filter_layer.update(filters)
        model.sst_dict.clear()
        model.sst_dict.update(sst_dict)
        model.train()


def test_a_bad_value_for_the_key_raises(tmp_path):
    with pytest.raises(ValueError, match="filter_eval_statistics"):
        _run("PFCN_BiasedMF", tmp_path, filter_mode="sm", filter_eval_statistics="population")

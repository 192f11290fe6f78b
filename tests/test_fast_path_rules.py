"""CPU: the rules of fairrec/model/fast_path.py as the models' hooks apply them -- the two-valued config keys, which methods of
a subclass make `full_sort_factors` / `full_sort_pair_mlp` / `dyn_neg_select` decline, row-sharded models, and the filter loop.

The sets of method names are literals taken from the hooks as they stood before the rules were gathered (each was a chain of
`cls._x is not Base._x or ...`), asymmetries included: `_score` counts for PFCNBase.full_sort_factors and not for its
dyn_neg_select, `forward` for the MLP-scored models' dyn_neg_select only, and the full_sort_pair_mlp hooks and
PFCN_DMF.full_sort_factors look at no method at all.  A hook that does not decline goes on to its engine, which a CPU model
cannot build: `hip_engine` is replaced by a stand-in that raises `_Reached`, so "declines" is None and "does not" is the raise.
Models of 20 users x 30 items, embedding_size 4, as tests/test_dmf_towers.py builds them."""
import types

import pytest
import torch


class _Reached(Exception):
    pass


def _build(name, **more):
    from fairrec.config import Config
    from fairrec.data.dataset import synthetic_dataset
    from fairrec.utils import get_model
    config = Config(model=name, config_dict=dict(device="cpu", embedding_size=4, **more))
    return get_model(name)(config, synthetic_dataset(config, 20, 30, 200, seed=1))


SPLIT = dict(full_sort_scorer="split", dynamic_neg_scorer="split")
MODELS = {
    "PFCN_PMF": dict(filter_mode="none"),
    "PFCN_MLP": dict(filter_mode="none", **SPLIT),
    "PFCN_DMF": dict(filter_mode="none", num_layers=2, full_sort_scorer="towers"),
    "NFCF": dict(load_pretrain_path=None, **SPLIT),
    "FairGo_PMF": {},
}
USERS = type("I", (), {"__getitem__": lambda self, field: torch.zeros(2, dtype=torch.int64)})()      # any column: two users
CALLS = {"full_sort_factors": lambda m: m.full_sort_factors(USERS), "full_sort_pair_mlp": lambda m: m.full_sort_pair_mlp(USERS),
         "dyn_neg_select": lambda m: m.dyn_neg_select(USERS, None, 1, 4)}
# (model, hook): (the methods whose override makes the hook decline, some methods whose override does not)
DECLINES = {
    ("PFCN_PMF", "dyn_neg_select"): (("_predict_score", "_item_tower", "_user_tower", "predict"), ("_score", "forward")),
    ("PFCN_PMF", "full_sort_factors"): (("_predict_score", "_score", "_item_tower", "_user_tower", "predict"), ("forward",)),
    ("PFCN_MLP", "dyn_neg_select"): (("_predict_score", "_item_tower", "_user_tower", "predict", "forward"), ("_score",)),
    ("PFCN_MLP", "full_sort_pair_mlp"): ((), ("_predict_score", "_item_tower", "_user_tower", "predict", "forward", "_score")),
    ("NFCF", "dyn_neg_select"): (("predict", "forward", "_score_logits"), ("calculate_loss",)),
    ("NFCF", "full_sort_pair_mlp"): ((), ("predict", "forward", "_score_logits")),
    ("PFCN_DMF", "full_sort_factors"): ((), ("_predict_score", "_score", "_item_tower", "_user_tower", "predict", "forward")),
    ("FairGo_PMF", "full_sort_factors"): (("full_sort_predict",), ("predict", "forward")),
}


def _cfg(key, value):
    return type("C", (), {"__getitem__": lambda self, k: value if k == key else None})()


def test_the_four_keys_parse_alike():
    from fairrec.model.layers import dynamic_neg_scorer_of, full_sort_scorer_of
    from fairrec.model.fair_recommender.pfcn_dmf import dmf_full_sort_scorer_of

    def filter_stats(config):
        return _build("PFCN_PMF", filter_mode="none", filter_eval_statistics=config["filter_eval_statistics"]).filter_eval_statistics

    for key, parse, default, other, sibling, message in (
            ("full_sort_scorer", full_sort_scorer_of, "pairs", "split", "towers",
             r"full_sort_scorer must be pairs or split, not \[towers\]"),
            ("dynamic_neg_scorer", dynamic_neg_scorer_of, "pairs", "split", "towers",
             r"dynamic_neg_scorer must be pairs or split, not \[towers\]"),
            ("full_sort_scorer", dmf_full_sort_scorer_of, "pairs", "towers", "split",
             r"full_sort_scorer of PFCN_DMF must be pairs or towers, not \[split\]"),
            ("filter_eval_statistics", filter_stats, "batch", "running", "pairs",
             r"filter_eval_statistics must be batch or running, not \[pairs\]")):
        assert parse(_cfg(key, None)) == default
        assert parse(_cfg(key, default.upper())) == default and parse(_cfg(key, other.capitalize())) == other
        with pytest.raises(ValueError, match=message):
            parse(_cfg(key, sibling))


def test_full_sort_eval_keeps_its_case():
    from fairrec.trainer.trainer import full_sort_eval_of
    assert full_sort_eval_of(_cfg("full_sort_eval", None)) == "matrix" and full_sort_eval_of(_cfg("full_sort_eval", "fused")) == "fused"
    with pytest.raises(ValueError, match=r"full_sort_eval must be matrix or fused, not \[Fused\]"):
        full_sort_eval_of(_cfg("full_sort_eval", "Fused"))


def _stand_in(model):
    def reached():
        raise _Reached
    model.hip_engine = reached
    return model.eval()


@pytest.mark.parametrize("name,hook", list(DECLINES))
def test_each_hook_declines_for_its_own_methods_only(name, hook):
    declining, indifferent = DECLINES[name, hook]
    model = _stand_in(_build(name, **MODELS[name]))
    parent = type(model)
    with pytest.raises(_Reached):
        CALLS[hook](model)
    for method in declining + indifferent:      # the one model as an instance of a subclass with this method of its own
        inherited = getattr(parent, method)
        model.__class__ = type(parent.__name__ + "Sub", (parent,), {method: lambda self, *a, **kw: inherited(self, *a, **kw)})
        if method in declining:
            assert CALLS[hook](model) is None, method
        else:
            with pytest.raises(_Reached):
                CALLS[hook](model)


@pytest.mark.parametrize("name", ["PFCN_PMF", "PFCN_MLP", "PFCN_DMF", "NFCF"])
def test_a_row_sharded_model_declines_without_an_engine(name):
    model = _stand_in(_build(name, **MODELS[name]))
    model.shard = (0, 2)
    for hook, call in CALLS.items():
        if hasattr(model, hook):
            assert call(model) is None, hook
    assert model._engine is None


def test_dyn_neg_select_declines_under_pairs_and_under_dropout():
    for name in ("NFCF", "PFCN_MLP"):
        model = _stand_in(_build(name, **dict(MODELS[name], full_sort_scorer="pairs", dynamic_neg_scorer="pairs")))
        assert CALLS['dyn_neg_select'](model) is None
        model = _stand_in(_build(name, **dict(MODELS[name], dropout=0.5))).train()
        assert CALLS['dyn_neg_select'](model) is None          # a scorer that drops out now
        with pytest.raises(_Reached):
            CALLS['dyn_neg_select'](model.eval())


@pytest.mark.parametrize("U,per,sizes", [(0, 5, []), (0, None, []), (1, 1, [1]), (13, 5, [5, 5, 3]), (13, None, [13]), (13, 64, [13])])
def test_the_filter_loop(U, per, sizes):
    from fairrec.model.fast_path import filtered_users
    seen = []

    def record(rows, sst_list):
        assert sst_list == ["gender"]
        seen.append(rows.shape[0])
        return rows + 1.0

    rows = torch.arange(U * 4, dtype=torch.float32).view(U, 4)
    out = filtered_users(types.SimpleNamespace(filter_mode="sm", _filter=record), rows, ["gender"], per)
    assert seen == sizes
    assert out is rows if U == 0 else torch.equal(out, rows + 1.0)
    assert filtered_users(types.SimpleNamespace(filter_mode="none", _filter=record), rows, None, per) is rows and seen == sizes

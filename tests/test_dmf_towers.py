"""CPU: PFCN_DMF's config key `full_sort_scorer` -- pairs (the default) or towers, read when the model is built."""
import pytest


def _cfg(value):
    return type("C", (), {"__getitem__": lambda self, k: value if k == "full_sort_scorer" else None})()


def _build(**more):
    from fairrec.config import Config
    from fairrec.data.dataset import synthetic_dataset
    from fairrec.utils import get_model
    config = Config(model="PFCN_DMF", config_dict=dict(device="cpu", embedding_size=4, filter_mode="none", num_layers=2, **more))
    return get_model("PFCN_DMF")(config, synthetic_dataset(config, 20, 30, 200, seed=1))


def test_key_parses():
    from fairrec.model.fair_recommender.pfcn_dmf import dmf_full_sort_scorer_of
    assert dmf_full_sort_scorer_of(_cfg(None)) == "pairs" and dmf_full_sort_scorer_of(_cfg("pairs")) == "pairs"
    assert dmf_full_sort_scorer_of(_cfg("towers")) == "towers" and dmf_full_sort_scorer_of(_cfg("ToWeRs")) == "towers"
    assert dmf_full_sort_scorer_of(_cfg("PAIRS")) == "pairs"
    for bad in ("bogus", "split", ""):
        with pytest.raises(ValueError, match="full_sort_scorer.*pairs or towers"):
            dmf_full_sort_scorer_of(_cfg(bad))


def test_bogus_raises_when_the_model_is_built():
    with pytest.raises(ValueError, match="full_sort_scorer"):
        _build(full_sort_scorer="bogus")


def test_default_is_pairs_and_declines():
    from fairrec.config import Config
    assert Config(model="PFCN_DMF", config_dict=dict(device="cpu"))["full_sort_scorer"] == "pairs"
    model = _build()
    assert model.full_sort_scorer == "pairs"
    assert model.full_sort_factors(None) is None              # the dense path serves the call; no device is touched
    assert _build(full_sort_scorer="Towers").full_sort_scorer == "towers"


def test_the_other_models_keep_their_key():
    from fairrec.model.layers import full_sort_scorer_of
    with pytest.raises(ValueError, match="pairs or split"):
        full_sort_scorer_of(_cfg("towers"))

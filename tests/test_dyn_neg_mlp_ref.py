"""CPU: the float64 restatement of fr_dyn_neg_mlp_select (tests/dyn_neg_mlp_ref.py) against a torch-double MLP on
cat(x_u, w_c), its pick against torch.max(dim=0) with NaNs and ties, the condition on the inputs of every seeded case the GPU
tests name (the reference alone leaves at most 5 % of the columns undecided), the argument checks of the two entries (no
device needed: they refuse before any device work and write nothing), and the config key `dynamic_neg_scorer`."""
import numpy as np
import pytest
import torch

import dyn_neg_mlp_ref as R


def _torch_mlp(x, rows, W1, b1, layers, n):
    """MLPLayers([2 D, n1, ..., 1]) in eval mode, in double: Linear then ReLU for every layer, the last included; sigmoid."""
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    h = torch.cat([t(x)[torch.arange(rows.shape[0]) % n], t(rows)], dim=1)
    for W, b in [(W1, b1)] + list(layers):
        h = torch.relu(torch.nn.functional.linear(h, t(W), t(b)))
    return torch.sigmoid(h[:, 0]).numpy()


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_equals_the_concat_mlp_and_the_case_is_decided(name):
    c = R.make_case(name)
    n, num, M, D = c["n"], c["num"], c["M"], c["D"]
    # (the GPU tests take the rows LazyTable.gather returns from the aged table -- a few optimizer steps away from these -- and
    # assert the same cap on them)
    rows = c["table0"][c["cand"]]
    P = R.user_half(c["x"], c["W1"], c["b1"]).astype(np.float32)
    W1i = c["W1"][:, D:]
    got = R.scores64(rows, P, W1i, c["layers"], n)
    assert got.shape == (M * num * n,)
    P64 = R.user_half(c["x"], c["W1"], c["b1"])
    exact = R.scores64(rows, P64, W1i, c["layers"], n)
    want = _torch_mlp(c["x"], rows, c["W1"], c["b1"], c["layers"], n)
    assert np.abs(exact - want).max() <= 1e-12
    assert np.abs(exact - R.concat64(c["x"], rows, c["W1"], c["b1"], c["layers"], n)).max() <= 1e-12
    s, b = R.bound(rows, P, W1i, c["layers"], n)
    # (the worst case grows by |W| per layer: 1e-2 at most on these shapes, against scores in [0.5, 1])
    assert np.array_equal(s, got) and np.all(b > 0) and np.all(b < 1e-2)
    dec = R.decided(s.reshape(M, -1), b.reshape(M, -1))
    assert dec.shape == (num * n,) and np.mean(~dec) <= R.UNDECIDED_CAP, np.mean(~dec)
    if M == 1:
        assert dec.all()
    # the pick is torch.max's on the float64 scores
    idx = torch.max(torch.from_numpy(s.reshape(M, -1)), dim=0)[1].numpy()
    ids, r = R.select(s.reshape(M, -1), c["cand"].reshape(M, -1))
    assert np.array_equal(r, idx) and np.array_equal(ids, c["cand"].reshape(M, -1)[idx, np.arange(num * n)])


def test_pick_follows_torch_max_with_nans_and_ties():
    g = torch.Generator().manual_seed(7)
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
    for t in (s, s.double(), torch.randn(1, 9, generator=g), torch.randn(16, 77, generator=g)):
        assert np.array_equal(R.pick(t.numpy()), torch.max(t, dim=0)[1].numpy())
    b = np.full(s.shape, 1e-6)
    dec = R.decided(s.numpy(), b)
    assert not dec[:100].any()                         # equal best scores: undecided
    assert dec[100:160].all()                          # a NaN decides
    assert not dec[160:180].any()
    close = np.array([[1.0, 1.0, 1.0], [1.0 - 1e-6, 1.0 - 3e-6, 0.0], [0.0, 0.0, 1.0 - 1e-6]])
    assert R.decided(close, np.full(close.shape, 1e-6)).tolist() == [False, True, False]


def test_argument_validation_without_gpu():
    R.check_refusals()


def test_wrapper_checks_shapes():
    from fairrec import _C
    from fairrec.functional import dyn_neg_mlp_select
    pieces = {"P": torch.zeros(2, 4), "W1": torch.zeros(4, 8), "layers": [(torch.zeros(1, 4), torch.zeros(1))]}
    with pytest.raises(_C.FairrecError):
        dyn_neg_mlp_select(pieces, None, None, torch.zeros(4, dtype=torch.int64), 1, 2, None)


@pytest.mark.parametrize("model", ["NFCF", "PFCN_MLP"])
def test_dynamic_neg_scorer_key(model):
    from fairrec.model.layers import dynamic_neg_scorer_of
    cfg = lambda v: type("C", (), {"__getitem__": lambda self, k: v if k == "dynamic_neg_scorer" else None})()
    assert dynamic_neg_scorer_of(cfg(None)) == "pairs" and dynamic_neg_scorer_of(cfg("pairs")) == "pairs"
    assert dynamic_neg_scorer_of(cfg("split")) == "split" and dynamic_neg_scorer_of(cfg("Split")) == "split"
    with pytest.raises(ValueError, match="bogus"):
        dynamic_neg_scorer_of(cfg("bogus"))
    # ... and when the model is built (the constructors read the key before they touch a device)
    from fairrec.config import Config
    from fairrec.data.dataset import synthetic_dataset
    from fairrec.utils import get_model
    extra = {"NFCF": dict(mlp_hidden_size=[8, 4], load_pretrain_path=None, LABEL_FIELD="label"),
             "PFCN_MLP": dict(filter_mode="none", mlp_hidden_size_list=[8, 4])}[model]
    config = Config(model=model, config_dict=dict(device="cpu", embedding_size=4, dynamic_neg_scorer="bogus", **extra))
    dataset = synthetic_dataset(config, 20, 30, 200, seed=1)
    with pytest.raises(ValueError, match="dynamic_neg_scorer"):
        get_model(model)(config, dataset)
    config = Config(model=model, config_dict=dict(device="cpu", embedding_size=4, **extra))
    assert config["dynamic_neg_scorer"] == "pairs"
    assert get_model(model)(config, dataset).dynamic_neg_scorer == "pairs"

"""CPU: the float64 restatement of fr_pair_mlp_scores (tests/pair_mlp_ref.py) against a plain float64 MLP on the
concatenation, its rounding bound against an fp32 emulation of the contract's order, the argument checks of the entry (no
device needed: it refuses before any launch and writes nothing), and the config key `full_sort_scorer`."""
import ctypes

import numpy as np
import pytest

import pair_mlp_ref as R

SHAPES = [(5, [7, 1]), (16, [33, 17, 9, 1]), (64, [128, 64, 1]), (3, [1, 1, 1]), (8, [40, 24, 16, 8, 4, 1])]


def _case(rng, D, widths, U=6, N=9):
    x = rng.standard_normal((U, D)).astype(np.float32)
    w = rng.standard_normal((N, D)).astype(np.float32)
    W1 = (rng.standard_normal((widths[0], 2 * D)) / np.sqrt(2 * D)).astype(np.float32)
    b1 = (0.5 * rng.standard_normal(widths[0])).astype(np.float32)
    return x, w, W1, b1, R.random_layers(rng, widths)


@pytest.mark.parametrize("D,widths", SHAPES)
def test_split_restatement_equals_the_concat_mlp(D, widths):
    x, w, W1, b1, layers = _case(np.random.default_rng(D), D, widths)
    P, Q = R.halves64(x, w, W1, b1)
    got, want = R.scores64(P, Q, layers), R.concat64(x, w, W1, b1, layers)
    assert got.shape == want.shape == (6, 9)
    assert np.abs(got - want).max() <= 1e-12
    s, bound = R.bound_rows(x, w, W1, b1, layers)
    assert np.array_equal(s, got) and np.all(bound > 0) and np.all(bound < 1e-3)
    _, dense = R.bound_rows(x, w, W1, b1, layers, split=False)
    assert np.all(dense >= bound)           # the longer first chain has the wider bound


@pytest.mark.parametrize("D,widths", SHAPES)
def test_fp32_emulation_of_the_contract_stays_inside_the_bound(D, widths):
    rng = np.random.default_rng(100 + D)
    x, w, W1, b1, layers = _case(rng, D, widths, U=7, N=35)
    P64, Q64 = R.halves64(x, w, W1, b1)
    P, Q = P64.astype(np.float32), Q64.astype(np.float32)
    got = R.emulate32(P, Q, layers)
    s, bound = R.bound_pq(P, Q, layers)
    assert got.dtype == np.float32 and np.all(np.abs(got.astype(np.float64) - s) <= bound)
    # (1e-3 at most on these shapes -- the worst case grows by |W| per layer -- against scores in [0.5, 1])
    assert np.all(bound > 0) and np.all(bound < 1e-3)
    # a NaN row of P reaches every score of that user and no other
    P[2] = np.nan
    nan = np.isnan(R.emulate32(P, Q, layers))
    assert nan[2].all() and not np.delete(nan, 2, 0).any()
    assert np.array_equal(np.isnan(R.scores64(P, Q, layers)), nan)


# ---- argument checks: FR_EINVAL before any launch, scores_out untouched --------------------------------------------------
def _valid(keep, n_linears=3, width=4):
    from fairrec import _C
    a = _C.FrPairMlpArgs()
    f = (ctypes.c_float * 1024)(*([0.5] * 1024))
    ip = (ctypes.c_int64 * 3)(0, 1, 2)
    items = (ctypes.c_int64 * 2)(1, 2)
    out = (ctypes.c_float * 8)(*([-7.0] * 8))
    keep.extend([f, ip, items, out])
    p = ctypes.addressof(f)
    a.P, a.Q, a.scores_out = p, p, ctypes.addressof(out)
    for l in range(n_linears - 1):
        a.W[l], a.bias[l], a.n_out[l] = p, p, (width if l < n_linears - 2 else 1)
    a.hist_indptr, a.hist_items, a.hist_len, a.hist_sorted = ctypes.addressof(ip), ctypes.addressof(items), 2, 1
    a.n_users, a.n_items, a.ld, a.n1, a.n_linears, a.act, a.mask_pad = 2, 4, 4, width, n_linears, 1, 1
    return a, out


def test_argument_validation_without_gpu():
    from fairrec import _C
    lib = _C.lib()
    keep = []

    def refused(word, **fields):
        a, out = _valid(keep)
        for name, value in fields.items():
            if "[" in name:
                field, l = name[:-3], int(name[-2])
                getattr(a, field)[l] = value
            else:
                setattr(a, name, value)
        assert lib.fr_pair_mlp_scores(ctypes.byref(a), None) == -1, (word, fields)
        assert word.encode() in lib.fr_last_error(), (word, lib.fr_last_error())
        assert list(out) == [-7.0] * 8

    a, out = _valid(keep)
    for zero in ("n_users", "n_items"):                       # zero sizes: success, nothing launched
        a, out = _valid(keep)
        setattr(a, zero, 0)
        assert lib.fr_pair_mlp_scores(ctypes.byref(a), None) == 0 and list(out) == [-7.0] * 8
    for n_linears in (2, 6):                                  # the limits themselves are served
        a, out = _valid(keep, n_linears=n_linears, width=256)
        a.n_users = 0
        assert lib.fr_pair_mlp_scores(ctypes.byref(a), None) == 0
        n_out = (ctypes.c_int32 * (n_linears - 1))(*([256] * (n_linears - 2) + [1]))
        assert lib.fr_pair_mlp_supported(256, n_linears, n_out, 1) == 1
    assert lib.fr_pair_mlp_scores(None, None) == -1 and b"null" in lib.fr_last_error()
    refused("n1", n1=0)
    refused("n1", n1=257)
    refused("n_out[0]", **{"n_out[0]": 0})
    refused("n_out[0]", **{"n_out[0]": 257})
    refused("n_out[1]", **{"n_out[1]": 2})                    # the last layer has one output
    refused("n_linears", n_linears=1)
    refused("n_linears", n_linears=7)
    refused("P is null", P=None)
    refused("Q is null", Q=None)
    refused("scores_out", scores_out=None)
    refused("W[1]", **{"W[1]": None})
    refused("bias[0]", **{"bias[0]": None})
    refused("hist_sorted", hist_sorted=0)
    refused("hist_items", hist_items=None)
    refused("n_users", n_users=-1)
    refused("n_items", n_items=-1)
    refused("ld", ld=3)
    for act in (0, 2, 3, 4, 5, -1):
        refused("act", act=act)
    n_out = (ctypes.c_int32 * 2)(4, 1)
    assert lib.fr_pair_mlp_supported(4, 3, n_out, 1) == 1
    assert lib.fr_pair_mlp_supported(4, 3, n_out, 2) == 0 and lib.fr_pair_mlp_supported(257, 3, n_out, 1) == 0
    assert lib.fr_pair_mlp_supported(4, 7, n_out, 1) == 0 and lib.fr_pair_mlp_supported(4, 1, n_out, 1) == 0


def test_wrapper_refuses_cpu_tensors():
    import torch

    from fairrec import _C
    from fairrec.functional import pair_mlp_scores
    with pytest.raises(_C.FairrecError):
        pair_mlp_scores({"P": torch.zeros(2, 4), "Q": torch.zeros(3, 4), "layers": [(torch.zeros(1, 4), torch.zeros(1))]})


@pytest.mark.parametrize("who", ["pair_mlp_scores", "dyn_neg_mlp_select"])
def test_upper_layer_checks_keep_each_caller_s_wording(who):
    """The (W, bias) checks both wrappers share: the caller's name leads, the texts are the ones each wrapper raised itself."""
    import torch

    from fairrec import _C
    from fairrec.functional import _check_upper_layers
    cpu, ok = torch.device("cpu"), [(torch.zeros(3, 4), torch.zeros(3)), (torch.zeros(1, 3), torch.zeros(1))]
    _check_upper_layers(who, ok, 4, cpu)
    one = (torch.zeros(1, 1), torch.zeros(1))
    _check_upper_layers(who, [one] * (_C.PAIR_MLP_MAX_LINEARS - 1), 1, cpu)
    for layers in ([], [one] * _C.PAIR_MLP_MAX_LINEARS):
        with pytest.raises(ValueError, match=f"^{who}: {len(layers) + 1} linears, not in 2..{_C.PAIR_MLP_MAX_LINEARS}$"):
            _check_upper_layers(who, layers, 1, cpu)
    bad = [[(torch.zeros(3, 5), torch.zeros(3))],                               # the width of the layer below
           [ok[0], (torch.zeros(1, 4), torch.zeros(1))],                        # ... of the layer before
           [(torch.zeros(3, 4), torch.zeros(2))],                               # bias length
           [(torch.zeros(3, 4, dtype=torch.float64), torch.zeros(3))],
           [(torch.zeros(3, 4), torch.zeros(3, dtype=torch.float64))],
           [(torch.zeros(4, 3).t(), torch.zeros(3))],                           # not contiguous
           [(torch.zeros(3, 4), torch.zeros(6)[::2])],
           [(torch.zeros(3, 4, device="meta"), torch.zeros(3))]]                # another device
    for layers in bad:
        with pytest.raises(ValueError, match=f"^{who}: each layer is \\(W \\[n_out, n_in\\], bias \\[n_out\\]\\), contiguous fp32"):
            _check_upper_layers(who, layers, 4, cpu)


@pytest.mark.parametrize("model", ["NFCF", "PFCN_MLP"])
def test_full_sort_scorer_key(model):
    from fairrec.model.layers import full_sort_scorer_of
    cfg = lambda v: type("C", (), {"__getitem__": lambda self, k: v if k == "full_sort_scorer" else None})()
    assert full_sort_scorer_of(cfg(None)) == "pairs" and full_sort_scorer_of(cfg("pairs")) == "pairs"
    assert full_sort_scorer_of(cfg("split")) == "split" and full_sort_scorer_of(cfg("Split")) == "split"
    with pytest.raises(ValueError, match="bogus"):
        full_sort_scorer_of(cfg("bogus"))
    # ... and when the model is built (the constructors read the key before they touch a device)
    from fairrec.config import Config
    from fairrec.data.dataset import synthetic_dataset
    extra = {"NFCF": dict(mlp_hidden_size=[8, 4], load_pretrain_path=None, LABEL_FIELD="label"),
             "PFCN_MLP": dict(filter_mode="none", mlp_hidden_size_list=[8, 4])}[model]
    config = Config(model=model, config_dict=dict(device="cpu", embedding_size=4, full_sort_scorer="bogus", **extra))
    dataset = synthetic_dataset(config, 20, 30, 200, seed=1)
    from fairrec.utils import get_model
    with pytest.raises(ValueError, match="full_sort_scorer"):
        get_model(model)(config, dataset)

"""CPU: the float64 restatement of fr_mlp_infer (tests/mlp_infer_ref.py) against torch.nn.Sequential(Linear, BatchNorm1d,
act).double().eval(), and the argument checks of the entry (no device needed: it refuses before any launch and writes
nothing)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import mlp_infer_ref as R

TORCH_ACT = {0: None, 1: nn.ReLU, 2: nn.LeakyReLU, 3: nn.Sigmoid, 4: nn.Tanh}


def _sequential(net):
    mods = []
    for lay in net:
        n_out, n_in = lay["W"].shape
        lin = nn.Linear(n_in, n_out)
        lin.weight.data, lin.bias.data = torch.from_numpy(lay["W"]).clone(), torch.from_numpy(lay["bias"]).clone()
        mods.append(lin)
        if lay["bn"] is not None:
            w, b, mean, var, eps = lay["bn"]
            bn = nn.BatchNorm1d(n_out, eps=float(np.float32(eps)))
            bn.weight.data, bn.bias.data = torch.from_numpy(w).clone(), torch.from_numpy(b).clone()
            bn.running_mean.data, bn.running_var.data = torch.from_numpy(mean).clone(), torch.from_numpy(var).clone()
            mods.append(bn)
        if TORCH_ACT[lay["act"]] is not None:
            mods.append(TORCH_ACT[lay["act"]]())
    return nn.Sequential(*mods).double().eval()


@pytest.mark.parametrize("act", [0, 1, 2, 3, 4])
def test_restatement_against_torch_double(act):
    rng = np.random.default_rng(10 + act)
    # two nets, a layer without BatchNorm in each, out_div = 3
    nets = [R.random_net(rng, [12, 24, 9, 5], act, bn=[True, False, True]), R.random_net(rng, [12, 7, 5], act, bn=[False, True])]
    X = rng.standard_normal((37, 12)).astype(np.float32)
    got = R.forward64(nets, X, out_div=3)
    with torch.no_grad():
        x = torch.from_numpy(X).double()
        want = ((_sequential(nets[0])(x) + _sequential(nets[1])(x)) / 3).numpy()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    y, bound = R.forward_bound(nets, X, out_div=3)
    assert np.array_equal(y, got) and np.all(bound > 0) and np.all(bound < 1e-3)
    # (the bound is a few thousand ulp at most on these shapes: a check against it means something)
    assert np.all(bound <= 4096 * R.ulp32(np.abs(y) + 1.0))


def test_bound_grows_with_the_net_and_covers_fp32_numpy():
    """The bound holds for a plain fp32 evaluation in numpy (another summation order, the host's expf / tanhf)."""
    rng = np.random.default_rng(3)
    for act in range(5):
        net = R.random_net(rng, [100, 200, 100], act)
        X = rng.standard_normal((40, 100)).astype(np.float32)
        x = X
        for lay in net:
            z = (x @ lay["W"].T + lay["bias"]).astype(np.float32)
            w, b, mean, var, eps = lay["bn"]
            sc = (w * (np.float32(1) / np.sqrt(var + np.float32(eps)))).astype(np.float32)
            x = R.act64(((z - mean) * sc + b).astype(np.float32), act).astype(np.float32)
        y, bound = R.forward_bound([net], X)
        assert np.all(np.abs(x.astype(np.float64) - y) <= bound)


# ---- argument checks: FR_EINVAL before any launch, Y untouched ----------------------------------------------------------
def _valid(n_nets=1, n_layers=2):
    from fairrec import _C
    f = (ctypes.c_float * 64)(*([0.5] * 64))
    a = ctypes.addressof(f)
    nets = (_C.FrMlpNet * max(n_nets, 1))()
    for n in range(n_nets):
        nets[n].n_layers, nets[n].k_in = n_layers, 4
        for l in range(n_layers):
            nets[n].layer[l] = _C.FrMlpLayer(a, a, a, a, a, a, 1e-5, 4, 2)
    return nets, f


def test_argument_validation_without_gpu():
    from fairrec import _C
    lib = _C.lib()
    Y = (ctypes.c_float * 8)(*([-7.0] * 8))
    X = (ctypes.c_float * 8)(*([1.0] * 8))
    ax, ay = ctypes.addressof(X), ctypes.addressof(Y)

    def call(nets, n_nets=1, out_div=1.0, x=ax, M=2, y=ay):
        return lib.fr_mlp_infer(nets, n_nets, out_div, x, M, y, None)

    def refused(word, *args, **kw):
        assert call(*args, **kw) == -1, word
        assert word.encode() in lib.fr_last_error(), (word, lib.fr_last_error())

    nets, keep = _valid()
    assert call(nets, M=0) == 0                              # M == 0: success, nothing launched
    refused("nets", None)
    refused("n_nets", nets, n_nets=0)
    refused("n_nets", nets, n_nets=9)
    refused("X", nets, x=None)
    refused("Y", nets, y=None)
    refused("M", nets, M=-1)
    refused("out_div", nets, out_div=0.0)
    for field, bad in (("n_layers", 0), ("n_layers", 9), ("k_in", 0), ("k_in", 513)):
        nets, keep = _valid()
        setattr(nets[0], field, bad)
        refused(field, nets)
    for field, bad in (("n_out", 0), ("n_out", 513), ("act", -1), ("act", 5), ("W", None), ("bias", None)):
        nets, keep = _valid()
        setattr(nets[0].layer[1], field, bad)
        refused("layer[1]", nets)
        assert (field if field in ("n_out", "act") else "null").encode() in lib.fr_last_error()
    for field in ("bn_weight", "bn_bias", "bn_mean", "bn_var"):       # a partly-null BatchNorm quadruple
        nets, keep = _valid()
        setattr(nets[0].layer[0], field, None)
        refused("bn_", nets)
    nets, keep = _valid()
    for field in ("bn_weight", "bn_bias", "bn_mean", "bn_var"):       # all four null: a layer without BatchNorm, accepted
        setattr(nets[0].layer[0], field, None)
    assert call(nets, M=0) == 0
    nets, keep = _valid(n_nets=2)
    nets[1].k_in = 5
    refused("k_in", nets, n_nets=2)
    nets, keep = _valid(n_nets=2)
    nets[1].layer[1].n_out = 3
    refused("nets[1]", nets, n_nets=2)
    nets, keep = _valid(n_nets=8, n_layers=8)
    assert call(nets, n_nets=8, M=0) == 0                    # the limits themselves are served
    assert list(Y) == [-7.0] * 8


def test_wrapper_refuses_cpu_tensors():
    from fairrec import _C
    from fairrec.functional import mlp_infer
    from fairrec.model.layers import MLPLayers
    with pytest.raises(_C.FairrecError):
        mlp_infer(MLPLayers([4, 8, 4], bn=True), torch.zeros(3, 4))

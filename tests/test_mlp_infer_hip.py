"""GPU: fr_mlp_infer through the C ABI against the float64 restatement and its running rounding bound
(tests/mlp_infer_ref.py), and the properties the entry exists for: a row's bits depend on that row and the parameters alone
(not on M, its position, its tile or the other rows), nothing but Y is written, two calls agree.

Every parameter tensor, X and Y start one float past an allocation's start: the entry asks for float alignment only."""
import ctypes

import numpy as np
import pytest
import torch

import mlp_infer_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
MS = (1, 31, 32, 33, 65, 1000)
M_MAX = 1000
CANARY = 64
WIDTHS = ([4, 8, 4], [16, 32, 16], [100, 200, 100], [128, 256, 128], [256, 512, 256], [64, 32, 16, 1], [16, 16, 8, 7], [33, 1])


def _case(name):
    """(nets, out_div, X) of a named case, from a seed that is the name's own."""
    rng = np.random.default_rng(sum(name.encode()) * 7919 + len(name))
    kind, _, arg = name.partition(":")
    out_div = 1.0
    if kind == "widths":                       # the issue's shapes, BatchNorm in every layer, the activation rotating
        i = int(arg)
        nets = [R.random_net(rng, WIDTHS[i], act=(i + 2) % 5)]
    elif kind == "act":                        # every activation, on a shape with odd tails and more than one column group
        nets = [R.random_net(rng, [100, 200, 100], act=int(arg))]
    elif kind == "deep":                       # eight layers, BatchNorm in some, every activation
        nets = [R.random_net(rng, [24, 40, 33, 64, 17, 130, 32, 9, 5], act=0, bn=[True, False, True, True, False, True, False, True],
                             acts=[2, 1, 4, 3, 0, 2, 4, 1])]
    elif kind == "mixed":                      # layers with and without BatchNorm in one net
        nets = [R.random_net(rng, [16, 32, 16], act=2, bn=[False, True]), R.random_net(rng, [16, 8, 16, 16], act=3, bn=[True, False, True])]
        out_div = 3.0
    elif kind == "nets":                       # 1, 2, 3 and 8 filters [D, 2D, D], out_div 1 and 3
        n, div = arg.split("/")
        nets = [R.random_net(rng, [16, 32, 16], act=2) for _ in range(int(n))]
        out_div = float(div)
    elif kind == "nets3l":                     # eight nets of three layers: the input tile is reloaded between nets
        nets = [R.random_net(rng, [20, 40, 24, 12], act=(j % 5)) for j in range(8)]
        out_div = 3.0
    else:
        raise KeyError(name)
    X = rng.standard_normal((M_MAX, nets[0][0]["W"].shape[1])).astype(np.float32)
    return nets, out_div, X


CASES = [f"widths:{i}" for i in range(len(WIDTHS))] + [f"act:{a}" for a in range(5)] + \
    ["deep", "mixed", "nets:1/3", "nets:2/3", "nets:3/1", "nets:8/3", "nets3l"]


def _odd(a):
    """A device copy of a numpy array that starts one float past its allocation."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
    view = buf[1:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view


class DevNets:
    def __init__(self, nets):
        from fairrec import _C
        self.tensors = []
        self.arr = (_C.FrMlpNet * len(nets))()
        for n, net in enumerate(nets):
            self.arr[n].n_layers, self.arr[n].k_in = len(net), net[0]["W"].shape[1]
            for l, lay in enumerate(net):
                ts = [_odd(lay["W"]), _odd(lay["bias"])] + ([_odd(t) for t in lay["bn"][:4]] if lay["bn"] is not None else [])
                self.tensors += ts
                self.arr[n].layer[l] = _C.FrMlpLayer(*[t.data_ptr() for t in ts], *([None] * (6 - len(ts))),
                                                     float(lay["bn"][4]) if lay["bn"] is not None else 0.0, lay["W"].shape[0],
                                                     lay["act"])
        self.n = len(nets)
        self.n_out = nets[0][-1]["W"].shape[0]

    def __call__(self, X, out_div=1.0):
        """(Y [M, n_out], the canary floats behind it) of device rows X."""
        from fairrec import _C
        M = X.shape[0]
        buf = torch.full((1 + M * self.n_out + CANARY,), -7.0, dtype=torch.float32, device=DEV)
        Y = buf[1:1 + M * self.n_out].view(M, self.n_out)
        _C.check(_C.lib().fr_mlp_infer(self.arr, self.n, float(out_div), X.data_ptr(), M, Y.data_ptr(), _C.current_stream()),
                 "fr_mlp_infer")
        return Y, buf[1 + M * self.n_out:]

    def bits(self):
        return [t.clone().view(torch.int32) for t in self.tensors]


_cache = {}


def _setup(name):
    """(device nets, out_div, X numpy, X device, float64 reference, bound): built once per case, never changed."""
    if name not in _cache:
        nets, out_div, X = _case(name)
        y, bound = R.forward_bound(nets, X, out_div)
        _cache[name] = (DevNets(nets), out_div, X, _odd(X), y, bound)
    return _cache[name]


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("name", CASES)
def test_values_within_the_running_bound(name):
    dev, out_div, X, Xd, y, bound = _setup(name)
    worst = 0.0
    for M in MS:
        got, canary = dev(Xd[:M], out_div)
        got = got.cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all()
        ratio = np.abs(got - y[:M]) / bound[:M]
        worst = max(worst, float(ratio.max()))
        print(f"{name}: M = {M}: max |Y - float64| / bound = {ratio.max():.3g} (max error {np.abs(got - y[:M]).max():.3g})")
        assert np.all(ratio <= 1.0)
        assert bool((canary == -7.0).all())
    print(f"{name}: largest error / bound over every M = {worst:.3g}")


@pytest.mark.parametrize("name", ["widths:2", "widths:4", "widths:5", "widths:7", "act:3", "deep", "mixed", "nets:3/1", "nets:8/3", "nets3l"])
def test_a_row_depends_on_that_row_alone(name):
    dev, out_div, X, Xd, _, _ = _setup(name)
    full, _ = dev(Xd, out_div)
    for r in (0, 31, 32, 63, 64, 998, 999):                                  # a row alone (M = 1) = that row of the full call
        one, _ = dev(Xd[r:r + 1].clone(), out_div)
        assert _same(one[0], full[r]), r
    head, _ = dev(Xd[:33], out_div)
    assert _same(head, full[:33])
    perm = torch.from_numpy(np.random.default_rng(1).permutation(M_MAX)).to(DEV)
    moved, _ = dev(Xd[perm].contiguous(), out_div)
    assert _same(moved, full[perm])
    again, _ = dev(Xd, out_div)                                              # two calls: the same bits
    assert _same(again, full)


@pytest.mark.parametrize("name", ["widths:2", "widths:3", "act:4", "nets:2/3", "nets3l"])
def test_a_nan_or_inf_row_stays_in_its_row(name):
    dev, out_div, X, Xd, _, _ = _setup(name)
    full, _ = dev(Xd, out_div)
    bad = Xd.clone()
    rows = {5: float("nan"), 40: float("inf"), 63: float("-inf"), 999: float("nan")}
    for r, v in rows.items():
        bad[r] = v
    got, _ = dev(bad, out_div)
    keep = torch.ones(M_MAX, dtype=torch.bool, device=DEV)
    keep[list(rows)] = False
    assert _same(got[keep], full[keep])
    assert bool(torch.isfinite(got[keep]).all())
    one = Xd.clone()
    one[40, 0] = float("nan")                                                # one poisoned cell of one row
    got, _ = dev(one, out_div)
    keep[:] = True
    keep[40] = False
    assert _same(got[keep], full[keep])


@pytest.mark.parametrize("name", ["widths:1", "widths:6", "mixed", "nets:8/3"])
def test_nothing_but_y_is_written(name):
    dev, out_div, X, Xd, _, _ = _setup(name)
    before, x_before = dev.bits(), Xd.clone().view(torch.int32)
    for M in (1, 33):
        y, canary = dev(Xd[:M], out_div)
        assert bool((canary == -7.0).all()) and bool(torch.isfinite(y).all())
    after = dev.bits()
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert torch.equal(Xd.view(torch.int32), x_before)


def test_the_wrapper_builds_the_same_call():
    """functional.mlp_infer on MLPLayers modules = the C entry on their parameters and running statistics."""
    from fairrec.functional import mlp_infer
    from fairrec.model.layers import MLPLayers
    torch.manual_seed(3)
    mods = [MLPLayers([16, 32, 16], activation="leakyrelu", bn=True, init_method="norm").to(DEV) for _ in range(2)]
    for m in mods:
        for bn in m.batchnorms():
            bn.running_mean.normal_()
            bn.running_var.uniform_(0.25, 4.0)
    x = torch.randn(70, 16, device=DEV)
    got = mlp_infer(mods, x, out_div=3.0)
    nets = [R.net_of_module(m) for m in mods]
    y, bound = R.forward_bound(nets, x.cpu().numpy(), 3.0)
    assert np.all(np.abs(got.cpu().numpy().astype(np.float64) - y) <= bound)
    direct, _ = DevNets(nets)(x, 3.0)
    assert _same(got, direct)
    assert mlp_infer(mods, x[:0]).shape == (0, 16)

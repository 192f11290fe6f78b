"""CPU: the references of tests/probe_ref.py.  The float64 step is pinned to torch autograd (nn.Linear, CrossEntropyLoss,
torch.optim.Adam in float64), the metrics to sklearn (or a direct O(n^2) count), the whole float64 procedure to the bounds
tests/test_leakage_hip.py asserts of the package on the same three data sets; and the constants behind the kernel tolerances
are measured here, on the reference side (against probe_ref.MEASURED)."""
import numpy as np
import pytest
import torch

import probe_ref as R


# ---- the float64 step against autograd -----------------------------------------------------------------------------------------

def _torch_steps(c, D, H, classes, n_steps):
    lay, P = R.layout(D, H, classes)
    p0 = torch.from_numpy(c["params"]).double()
    nets, tensors = [], []
    for d, C in zip(lay, classes):
        mods = []
        if H:
            l1 = torch.nn.Linear(D, H).double()
            l1.weight.data = R._get(p0, d["W1"]).clone()
            l1.bias.data = R._get(p0, d["b1"]).clone()
            mods += [l1, torch.nn.ReLU()]
            tensors += [l1.weight, l1.bias]
        l2 = torch.nn.Linear(H if H else D, C).double()
        l2.weight.data = R._get(p0, d["W2"]).clone()
        l2.bias.data = R._get(p0, d["b2"]).clone()
        tensors += [l2.weight, l2.bias]
        nets.append(torch.nn.Sequential(*mods, l2))
    opt = torch.optim.Adam(tensors, lr=c["lr"])
    X, y = torch.from_numpy(c["X"]).double(), torch.from_numpy(c["labels"])
    out = []
    for _ in range(n_steps):
        opt.zero_grad()
        losses = [torch.nn.CrossEntropyLoss()(net(X), y[a]) for a, net in enumerate(nets)]
        sum(losses).backward()
        grad = torch.cat([t.grad.reshape(-1) for t in tensors]).clone()
        opt.step()
        out.append((torch.stack(losses).detach().numpy(), grad.numpy(),
                    torch.cat([t.detach().reshape(-1) for t in tensors]).numpy().copy()))
    return out


def _close(what, got, ref, rel=1e-12):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bound = rel * (np.abs(ref) + np.abs(ref).max())
    assert (np.abs(got - ref) <= bound).all(), f"{what}: {np.abs(got - ref).max():.3g} against {bound.min():.3g}"


@pytest.mark.parametrize("case", [(33, 5, 7, (3,)), (65, 6, 5, (2, 7, 21)), (65, 6, 0, (2, 3)), (1, 3, 4, (2,)),
                                  (200, 17, 33, (64,))])
def test_float64_step_is_autograd_and_torch_adam(case):
    B, D, H, classes = case
    c = R.make_case(B, D, H, classes, "plain")
    ref = _torch_steps(c, D, H, classes, 3)
    p, m, v = c["params"].astype(np.float64), np.zeros(len(c["params"])), np.zeros(len(c["params"]))
    for step, (loss, grad, after) in enumerate(ref, start=1):
        r = R.step_f64(p, m, v, c["X"], c["labels"], D, H, classes, c["lr"], step)
        _close("loss", r["loss"][1:], loss)
        _close("loss total", r["loss"][0], loss.sum())
        _close("grad", r["grad"], grad)
        _close("params", r["params"], after)
        p, m, v = r["params"], r["m"], r["v"]


def test_relu_edge_takes_the_zero_branch():
    c = R.make_case(65, 6, 5, (3,), "relu_edge")
    lay, _ = R.layout(6, 5, (3,))
    r = R.step_f64(c["params"], c["m"], c["v"], c["X"], c["labels"], 6, 5, (3,), c["lr"], c["step"])
    assert not R._get(r["grad"], lay[0]["W1"])[0].any() and R._get(r["grad"], lay[0]["b1"])[0] == 0.0
    assert R._get(r["grad"], lay[0]["W1"])[1].any()


def test_dropped_rows_contribute_nothing_and_keep_the_divisor():
    c = R.make_case(33, 5, 7, (3, 2), "plain")
    drop = np.zeros(33, dtype=bool)
    drop[[4, 32]] = True
    a = R.step_f64(c["params"], c["m"], c["v"], c["X"], c["labels"], 5, 7, (3, 2), c["lr"], c["step"], drop=drop)
    keep = ~drop
    b = R.step_f64(c["params"], c["m"], c["v"], c["X"][keep], c["labels"][:, keep], 5, 7, (3, 2), c["lr"], c["step"])
    _close("grad", a["grad"] * 33, b["grad"] * 31)
    _close("loss", a["loss"] * 33, b["loss"] * 31)


# ---- metrics ---------------------------------------------------------------------------------------------------------------------

def _auc_count(score, pos):
    s1, s0 = score[pos], score[~pos]
    return ((s1[:, None] > s0[None, :]).sum() + 0.5 * (s1[:, None] == s0[None, :]).sum()) / (len(s1) * len(s0))


@pytest.mark.parametrize("C", [2, 3, 7])
def test_metrics_equal_sklearn_or_a_direct_count(C):
    rng = np.random.default_rng(C)
    n = 400
    z = np.round(rng.standard_normal((n, C)), 1)          # rounded: ties in the argmax and among the probabilities
    y = rng.integers(0, C if C < 7 else C - 1, n)          # C = 7: class 6 has no test row
    y_train = rng.integers(0, C, 1000)
    got = R.metrics(z, y, y_train, C)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    present = [c for c in range(C) if 0 < (y == c).sum() < n]
    try:
        from sklearn.metrics import accuracy_score, roc_auc_score
        auc = roc_auc_score(y == 1, p[:, 1]) if C == 2 else float(np.mean([roc_auc_score(y == c, p[:, c]) for c in present]))
        acc = accuracy_score(y, z.argmax(axis=1))
    except ImportError:
        auc = _auc_count(p[:, 1], y == 1) if C == 2 else float(np.mean([_auc_count(p[:, c], y == c) for c in present]))
        acc = float((z.argmax(axis=1) == y).mean())
    assert abs(got["auc"] - auc) <= 1e-12 and abs(got["accuracy"] - acc) <= 1e-12
    assert abs(got["auc"] - (_auc_count(p[:, 1], y == 1) if C == 2 else
                             float(np.mean([_auc_count(p[:, c], y == c) for c in present])))) <= 1e-12
    assert got["majority"] == float((y == np.bincount(y_train, minlength=C).argmax()).mean())
    assert abs(got["logloss"] - float(-np.log(p[np.arange(n), y]).mean())) <= 1e-12


# ---- the whole procedure on the three data sets of tests/test_leakage_hip.py ------------------------------------------------------

def _run(kind):
    X, y = R.leak_data(kind)
    L = R.LEAK
    return R.probe_f64(X, {"a": y}, L["hidden"], L["epochs"], L["batch"], L["lr"], L["test_ratio"], L["seed"])["a"]


def test_reference_finds_a_planted_signal():
    r = _run("planted")
    print("planted:", r)
    assert r["auc"] >= 0.9


def test_reference_finds_nothing_in_an_independent_attribute():
    r = _run("independent")
    print("independent:", r)
    assert abs(r["auc"] - 0.5) <= 0.06


def test_reference_accuracy_of_an_independent_seven_class_attribute_is_the_majority_rate():
    r = _run("seven")
    print("seven:", r)
    assert abs(r["accuracy"] - r["majority"]) <= 0.05


# ---- the measurement behind the tolerance constants ------------------------------------------------------------------------------

def _units(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float((np.abs(np.asarray(got, dtype=np.float64) - ref) / (R.U * (np.abs(ref) + np.abs(ref).max()))).max())


def test_grid_rule_reaches_two_tiles_per_workgroup():
    assert R.grid(1) == (1, 1, 1) and R.grid(8192) == (256, 1, 256) and R.grid(65536) == (2048, 8, 256)
    tiles, tpw, wgs = R.grid(R.BIG_B)
    assert tpw == 2 and wgs == 129 and tiles == 258


def test_measure_the_float32_restatement():
    worst = {"loss": 0.0, "grad": 0.0, "param": 0.0}
    for B, D, H, classes, tag in R.cases():
        c = R.make_case(B, D, H, classes, tag)
        args = (c["params"], c["m"], c["v"], c["X"], c["labels"], D, H, classes, c["lr"], c["step"])
        ref, f32 = R.step_f64(*args), R.step_f32(*args)
        worst["loss"] = max(worst["loss"], _units(f32["loss"], ref["loss"]))
        worst["grad"] = max(worst["grad"], _units(f32["grad"], ref["grad"]))
        worst["param"] = max(worst["param"], _units(f32["params"], ref["params"]))
    for key, w in worst.items():
        print(f"\nprobe_ref measurement {key}: float32 restatement's worst error {w:.4g} units (recorded {R.MEASURED[key]})")
    for key, w in worst.items():
        assert w <= R.MEASURED[key], f"{key}: the float32 restatement errs by {w:.4g} units, recorded {R.MEASURED[key]}"
        assert w >= 0.5 * R.MEASURED[key], f"{key}: recorded {R.MEASURED[key]} is no measurement ({w:.4g})"

"""numpy float64 restatement of fr_mlp_infer's contract (include/fairrec_hip.h, csrc/mlp_infer.hip), for the tests.

A layer is a dict {W [n_out, n_in], bias [n_out], bn: None | (weight, bias, mean, var, eps), act: 0..4}; a net is a list of
layers; the entry computes (net_0(X) + net_1(X) + ...) / out_div with BatchNorm on the RUNNING statistics.

`forward_bound` carries a rounding bound for the fp32 kernel through the layers.  With u = 2^-24, gamma_n = n u / (1 - n u)
(as tests/recommend_ref.py and tests/graph_ref.py take theirs), x the float64 input of a layer and e_in the bound on the
kernel's input against it:

  product + bias, in any summation order (n_in products, n_in adds, one bias add):
      e_z = |W| e_in + gamma_(n_in + 2) (|W| (|x| + e_in) + |bias|)
  BatchNorm, y = fmaf(z - mean, sc, beta), sc = weight * (1 / sqrtf(var + eps)): the subtraction rounds once, sc four times
  (add, sqrt, quotient, product), the fma once -- gamma_6 on the product |z - mean| |sc|, one ulp of the result for the fma:
      e_y = |sc| e_z + gamma_6 |sc| (|z - mean| + e_z) + ulp(y)
  activation, Lipschitz constant L (1/4 for the sigmoid, 1 otherwise) and the error of its own evaluation:
      e_out = L e_y + c_act ulp(out)
      c_act = 0 for none and relu; 2 for leakyrelu (0.01f against 0.01: 2.2e-8 relative, and the product's rounding);
      6 for sigmoid and tanh: the device library (OCML) implements expf and tanhf to the accuracy the OpenCL specification asks
      of a full-profile device, exp <= 3 ulp and tanh <= 5 ulp.  Through 1 / (1 + e) an error of 3 ulp in e = expf(-y) moves
      the quotient by 3 u f (1 - f) <= 3 u f, the add and the IEEE division by u f each: 5 u f <= 5 ulp(f); tanhf: 5 ulp.
      One more ulp covers the rounding of y the reference does not have.
  every operation may also lose up to 2^-126 to underflow: (n_in + 4) 2^-126 per layer, negligible and carried for rigour.

  the sum over n nets and the division:  e_Y = (sum e_n + gamma_n (sum |out_n| + e_n)) / |out_div| + ulp(Y)

ulp(v) is the spacing of fp32 at |v| (>= u |v|), taken at |v| + bound so that the kernel's own value is covered."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
ACT_NAMES = {0: None, 1: "relu", 2: "leakyrelu", 3: "sigmoid", 4: "tanh"}
ACT_ULPS = {0: 0.0, 1: 0.0, 2: 2.0, 3: 6.0, 4: 6.0}
ACT_LIP = {0: 1.0, 1: 1.0, 2: 1.0, 3: 0.25, 4: 1.0}


def gamma(n):
    return n * U / (1.0 - n * U)


def ulp32(v):
    """Spacing of fp32 at |v| (float64 in, float64 out)."""
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def act64(y, act):
    if act == 1:
        return np.where(y < 0, 0.0, y)
    if act == 2:
        return np.where(y < 0, 0.01 * y, y)
    if act == 3:
        return 1.0 / (1.0 + np.exp(-y))
    if act == 4:
        return np.tanh(y)
    return y


def bn_scale(bn):
    w, b, mean, var, eps = bn
    return np.asarray(w, np.float64) / np.sqrt(np.asarray(var, np.float64) + float(np.float32(eps)))


def layer64(x, lay):
    W, b = np.asarray(lay["W"], np.float64), np.asarray(lay["bias"], np.float64)
    z = x @ W.T + b
    if lay["bn"] is not None:
        z = (z - np.asarray(lay["bn"][2], np.float64)) * bn_scale(lay["bn"]) + np.asarray(lay["bn"][1], np.float64)
    return act64(z, lay["act"])


def net64(net, X):
    x = np.asarray(X, np.float64)
    for lay in net:
        x = layer64(x, lay)
    return x


def forward64(nets, X, out_div=1.0):
    """Y in float64 of fp32 parameters and inputs."""
    total = None
    for net in nets:
        y = net64(net, X)
        total = y if total is None else total + y
    return total / float(out_div)


def net_bound(net, X):
    """(float64 output [M, n_out], rounding bound [M, n_out]) of one net."""
    x = np.asarray(X, np.float64)
    e = np.zeros_like(x)
    for lay in net:
        W, b = np.asarray(lay["W"], np.float64), np.asarray(lay["bias"], np.float64)
        n_in = W.shape[1]
        aW = np.abs(W).T
        z = x @ W.T + b
        ez = e @ aW + gamma(n_in + 2) * ((np.abs(x) + e) @ aW + np.abs(b)) + (n_in + 4) * TINY
        if lay["bn"] is not None:
            sc = np.abs(bn_scale(lay["bn"]))
            d = np.abs(z - np.asarray(lay["bn"][2], np.float64))
            y = (z - np.asarray(lay["bn"][2], np.float64)) * bn_scale(lay["bn"]) + np.asarray(lay["bn"][1], np.float64)
            ey = sc * ez + gamma(6) * sc * (d + ez)
            ey = ey + ulp32(np.abs(y) + ey)
        else:
            y, ey = z, ez
        out = act64(y, lay["act"])
        e = ACT_LIP[lay["act"]] * ey
        e = e + ACT_ULPS[lay["act"]] * ulp32(np.abs(out) + e)
        x = out
    return x, e


def forward_bound(nets, X, out_div=1.0):
    """(Y float64, bound) of the whole entry."""
    outs = [net_bound(net, X) for net in nets]
    total = sum(o for o, _ in outs)
    e = sum(b for _, b in outs) + gamma(len(nets)) * sum(np.abs(o) + b for o, b in outs)
    Y = total / float(out_div)
    e = e / abs(float(out_div))
    return Y, e + ulp32(np.abs(Y) + e)


def random_net(rng, widths, act, bn=True, acts=None):
    """A net of `widths` ([k_in, n_1, ..., n_L]) with fp32 parameters: weights ~ N(0, 1 / n_in) (activations stay O(1)),
    bn_var in [0.25, 4], bn_mean away from 0 (|mean| in [0.5, 1.5]), bn_weight of both signs (|weight| in [0.5, 1.5]).  `bn`: one
    flag or one per layer; `acts`: one code per layer instead of `act`."""
    L = len(widths) - 1
    flags = [bn] * L if isinstance(bn, bool) else list(bn)
    net = []
    for l in range(L):
        n_in, n_out = widths[l], widths[l + 1]
        lay = {"W": (rng.standard_normal((n_out, n_in)) / np.sqrt(n_in)).astype(np.float32),
               "bias": (0.5 * rng.standard_normal(n_out)).astype(np.float32), "bn": None,
               "act": int(acts[l]) if acts is not None else int(act)}
        if flags[l]:
            sign = lambda: np.where(rng.random(n_out) < 0.5, -1.0, 1.0)
            lay["bn"] = ((sign() * rng.uniform(0.5, 1.5, n_out)).astype(np.float32), (0.5 * rng.standard_normal(n_out)).astype(np.float32),
                         (sign() * rng.uniform(0.5, 1.5, n_out)).astype(np.float32), rng.uniform(0.25, 4.0, n_out).astype(np.float32),
                         1e-5)
        net.append(lay)
    return net


def net_of_module(module):
    """The layers of a fairrec `MLPLayers` module (its own parameters and running statistics, as numpy)."""
    from fairrec.model.layers import ACT_CODES
    name = module.activation.lower() if isinstance(module.activation, str) else module.activation
    np_ = lambda t: t.detach().cpu().numpy()
    bns = module.batchnorms()
    return [{"W": np_(lin.weight), "bias": np_(lin.bias), "act": ACT_CODES[name],
             "bn": (np_(bns[l].weight), np_(bns[l].bias), np_(bns[l].running_mean), np_(bns[l].running_var), bns[l].eps)
             if module.use_bn else None} for l, lin in enumerate(module.linears())]

"""Float64 reference of the NFCF scorer, MLPLayers([k0 + k1, n1, n2, 1], dropout p) + sigmoid + BCELoss (test helper).

Forward (layers.py:56-85, nfcf.py:73, :105): per layer Dropout -> Linear -> ReLU, the last layer included, then sigmoid
and BCELoss with torch's clamp of both logs at -100.  Backward: the analytic gradients at the three pre-activations, the
two input blocks and the six parameters, with BCELoss's gradient epsilon (torch divides by max(o (1 - o), 1e-12)).
`masks` are 0/1 keep masks of the three dropped tensors ([B, k0 + k1], [B, n1], [B, n2]); kept elements are scaled by
1 / (1 - p), as nn.Dropout does.  tests/test_scorer_ref.py pins all of it to torch.autograd.
"""
import torch

U = 2.0 ** -24          # unit roundoff of fp32
BCE_EPS = float(torch.tensor(1e-12, dtype=torch.float32))   # torch's BCE backward: (o - t) / max(o (1 - o), EPS), EPS an fp32 1e-12


def product_bound(a, w, bias, K, c):
    """Per-element bound on an fp32 product's error: c (K + 2) u (|a| |w|^T + |bias|), the absolute product in float64.
    (K + 2: the K-term reduction, the bias add and one rounding of the epilogue.)"""
    base = a.double().abs() @ w.double().abs().t()
    if bias is not None:
        base = base + bias.double().abs()
    return c * (K + 2) * U * base


def bce(o, t):
    """BCELoss per row as torch forms it: log(o) and log1p(-o), both clamped at -100."""
    return -(t * torch.clamp(torch.log(o), min=-100.0) + (1 - t) * torch.clamp(torch.log1p(-o), min=-100.0))


def bce_grad_out(o, t, B):
    """d mean(BCE) / d out: torch's binary_cross_entropy backward."""
    return (o - t) / torch.clamp(o * (1 - o), min=BCE_EPS) / B


def loss_head(y, label):
    """out = sigmoid(y), per-row BCE and d mean(BCE) / dy, in the dtype of `y`."""
    o = torch.sigmoid(y)
    return o, bce(o, label), bce_grad_out(o, label, y.shape[0]) * o * (1 - o)


def forward(x0, x1, params, p=0.0, masks=None):
    """The stored tensors of the scorer's forward: dropped input x, the pre-activations z1 / z2 / z3, the dropped hidden
    activations h1 / h2 and the output y (after its ReLU)."""
    W1, b1, W2, b2, W3, b3 = params
    s = 1.0 / (1.0 - p) if masks is not None else 1.0
    x = torch.cat([x0, x1], 1)
    if masks is not None:
        x = x * masks[0] * s
    z1 = x @ W1.t() + b1
    h1 = torch.relu(z1) * (masks[1] * s if masks is not None else 1.0)
    z2 = h1 @ W2.t() + b2
    h2 = torch.relu(z2) * (masks[2] * s if masks is not None else 1.0)
    z3 = h2 @ W3.t() + b3
    y = torch.relu(z3).view(-1)
    return dict(x=x, z1=z1, h1=h1, z2=z2, h2=h2, z3=z3.view(-1), y=y)


def backward(f, params, dy, k0, p=0.0, masks=None, gscale=1.0):
    """Gradients of gscale * loss from dy = d loss / dy and the forward's tensors `f`."""
    W1, b1, W2, b2, W3, b3 = params
    s = 1.0 / (1.0 - p) if masks is not None else 1.0
    dz3 = dy * gscale * (f["z3"] > 0)
    dz2 = dz3[:, None] * W3 * (f["z2"] > 0) * (masks[2] * s if masks is not None else 1.0)
    dz1 = (dz2 @ W2) * (f["z1"] > 0) * (masks[1] * s if masks is not None else 1.0)
    dx = dz1 @ W1
    if masks is not None:
        dx = dx * masks[0] * s
    return dict(dz3=dz3, dz2=dz2, dz1=dz1, dx0=dx[:, :k0], dx1=dx[:, k0:],
                dW1=dz1.t() @ f["x"], db1=dz1.sum(0), dW2=dz2.t() @ f["h1"], db2=dz2.sum(0),
                dW3=dz3[None, :] @ f["h2"], db3=dz3.sum().view(1))

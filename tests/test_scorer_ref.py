"""CPU: the float64 scorer reference of tests/scorer_ref.py (what tests/test_scorer_hip.py holds csrc/scorer.hip to) against
torch.autograd and torch's own binary_cross_entropy."""
import pytest
import torch
import torch.nn.functional as F

import scorer_ref as R


def _params(k, n1, n2, g):
    return [torch.randn(n1, k, generator=g, dtype=torch.float64) / k ** 0.5, torch.randn(n1, generator=g, dtype=torch.float64) * 0.1,
            torch.randn(n2, n1, generator=g, dtype=torch.float64) / n1 ** 0.5, torch.randn(n2, generator=g, dtype=torch.float64) * 0.1,
            torch.randn(1, n2, generator=g, dtype=torch.float64) / n2 ** 0.5, torch.full((1,), 0.2, dtype=torch.float64)]


@pytest.mark.parametrize("B,k0,n1,n2,p,gscale", [(37, 8, 16, 8, 0.0, 1.0), (64, 32, 32, 32, 0.3, 0.7), (5, 4, 12, 6, 0.5, 2.0),
                                                 (200, 16, 24, 16, 0.9, 1.0)])
def test_reference_gradients_match_autograd(B, k0, n1, n2, p, gscale):
    g = torch.Generator().manual_seed(B * 7 + k0)
    x0 = torch.randn(B, k0, generator=g, dtype=torch.float64)
    x1 = torch.randn(B, k0, generator=g, dtype=torch.float64) * 0.5 + 0.1
    params = _params(2 * k0, n1, n2, g)
    masks = [(torch.rand(B, w, generator=g) >= p).double() for w in (2 * k0, n1, n2)] if p > 0 else None
    label = (torch.rand(B, generator=g) < 0.5).double()
    # autograd through the oracle's op sequence (oracle/nfcf.py: Dropout -> Linear -> ReLU per layer, sigmoid, BCELoss)
    xa, xb = x0.clone().requires_grad_(), x1.clone().requires_grad_()
    pa = [t.clone().requires_grad_() for t in params]
    x = torch.cat([xa, xb], 1)
    for l in range(3):
        if masks is not None:
            x = x * (masks[l] / (1.0 - p))
        x = torch.relu(F.linear(x, pa[2 * l], pa[2 * l + 1]))
    yt = x.view(-1)
    yt.retain_grad()
    loss = F.binary_cross_entropy(torch.sigmoid(yt), label) * gscale
    loss.backward()
    f = R.forward(x0, x1, params, p, masks)
    torch.testing.assert_close(f["y"], yt.detach(), rtol=1e-13, atol=1e-14)
    o, l, dy = R.loss_head(f["y"], label)
    torch.testing.assert_close(l.mean() * gscale, loss.detach(), rtol=1e-13, atol=0)
    torch.testing.assert_close(dy * gscale, yt.grad, rtol=1e-12, atol=1e-15)
    d = R.backward(f, params, dy, k0, p, masks, gscale)
    got = dict(dx0=xa.grad, dx1=xb.grad, dW1=pa[0].grad, db1=pa[1].grad, dW2=pa[2].grad, db2=pa[3].grad, dW3=pa[4].grad,
               db3=pa[5].grad)
    for k, v in got.items():
        torch.testing.assert_close(d[k], v, rtol=1e-12, atol=1e-15, msg=k)
    assert bool((d["dz3"] != 0).any()) and bool((d["dz1"] != 0).any())       # the case exercises the gradient at all


def test_bce_clamp_and_epsilon_match_torch():
    """Outputs at 0 and 1 exactly (the -100 log clamp) and within 1e-12 of them (BCELoss's gradient epsilon), in float64
    and in fp32 (where sigmoid saturates at y >= ~16.7)."""
    for dt in (torch.float64, torch.float32):
        o = torch.tensor([0.0, 1.0, 1e-300 if dt == torch.float64 else 1e-40, 1 - 1e-13, 0.5, 0.25, 1e-13, 1.0, 0.0], dtype=dt)
        t = torch.tensor([1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0], dtype=dt)
        oo = o.clone().requires_grad_()
        F.binary_cross_entropy(oo, t).backward()
        rt = 0 if dt == torch.float64 else 2 * R.U       # (fp32: one rounding of the log apart)
        torch.testing.assert_close(R.bce(o, t), F.binary_cross_entropy(o, t, reduction="none"), rtol=rt, atol=0)
        torch.testing.assert_close(R.bce_grad_out(o, t, o.numel()), oo.grad, rtol=1e-6 if dt == torch.float32 else 1e-15, atol=0)
        y = torch.tensor([0.0, 20.0, 40.0, -30.0, 3.0, 16.0, 17.0], dtype=dt)
        lab = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0, 0.0, 1.0], dtype=dt)
        yy = y.clone().requires_grad_()
        lt = F.binary_cross_entropy(torch.sigmoid(yy), lab)
        lt.backward()
        o2, l2, dy2 = R.loss_head(y, lab)
        torch.testing.assert_close(l2.mean(), lt.detach(), rtol=1e-6 if dt == torch.float32 else 1e-15, atol=0)
        torch.testing.assert_close(dy2, yy.grad, rtol=1e-6 if dt == torch.float32 else 1e-14, atol=0)
    # fp32 saturation: out == 1 exactly, the loss of a negative row is the clamp (100), its gradient exactly 0
    o, l, dy = R.loss_head(torch.tensor([20.0, 20.0]), torch.tensor([0.0, 1.0]))
    assert o.tolist() == [1.0, 1.0] and l.tolist() == [100.0, 0.0] and dy.tolist() == [0.0, 0.0]


def test_product_bound_is_tight_enough_to_see_a_dropped_term():
    """The bound is far below one term of the product: a reduction that loses a 32-wide chunk cannot hide under it."""
    g = torch.Generator().manual_seed(3)
    a, w = torch.randn(64, 512, generator=g), torch.randn(32, 512, generator=g)
    full = a.double() @ w.double().t()
    part = a[:, :480].double() @ w[:, :480].double().t()
    bnd = R.product_bound(a, w, None, 512, 4)
    assert bool(((full - part).abs() > bnd).float().mean() > 0.99)
    assert bool(((a @ w.t()).double() - full).abs().le(bnd).all())

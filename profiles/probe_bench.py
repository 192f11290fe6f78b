"""The fused leakage probe (csrc/probe.hip: fr_probe_step) against a stock-torch probe on the same device and the same batches:
U = 1 000 000 users, D = 64, H = 64, heads of 2 / 7 / 21 classes (the gender / age / occupation shape), batch 8192, 20 % of
the rows held out -- one epoch is 98 optimiser steps of every head.

The baseline is what a user writes today: one nn.Sequential(Linear, ReLU, Linear) per head, F.cross_entropy, one
torch.optim.Adam over all heads, the batch's rows gathered ONCE per step (X[rows], kinder to the baseline than one gather per
head) and the labels gathered per head.  Both sides walk the same permutation.

Whole epochs are timed with device events after PROBE_BENCH_WARM warm epochs of each side, PROBE_BENCH_REPS times, the two sides
alternating; median and spread (min, max) are printed.  A second pass with the library's event profiler on (fr_prof_*) counts the
launches per step and gives the step kernel's own time, from which its share of the fp32 MFMA peak (157.3 TFLOP/s) follows: the
FLOP the algorithm needs (6 B per weight: forward, input gradient, weight gradient, at 2 FLOP per multiply-add) over kernel time.
One JSON object on the last line."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "recbole-fairrec_amd")]
from fairrec import _C  # noqa: E402
from fairrec.evaluator.leakage import Probe, init_params  # noqa: E402

U = int(os.environ.get("PROBE_BENCH_USERS", 1_000_000))
D, H, CLASSES, BATCH = 64, 64, [2, 7, 21], 8192
REPS, WARM = int(os.environ.get("PROBE_BENCH_REPS", 7)), int(os.environ.get("PROBE_BENCH_WARM", 2))
LR = 1e-3
PEAK = 157.3e12

assert torch.cuda.is_available(), "probe_bench needs a GPU"
g = torch.Generator().manual_seed(11)
X = torch.randn(U, D, generator=g).cuda()
table = torch.stack([torch.randint(0, C, (U,), generator=g) for C in CLASSES]).cuda().contiguous()
train = torch.randperm(U, generator=g)[U // 5:].cuda()
n_steps = (train.numel() + BATCH - 1) // BATCH
flat = init_params(g, D, H, CLASSES)

probe = Probe(X, table, CLASSES, H, LR, flat)

# the baseline's heads start from the same parameters
nets, off = [], 0
for C in CLASSES:
    l1, l2 = torch.nn.Linear(D, H), torch.nn.Linear(H, C)
    for t in (l1.weight, l1.bias, l2.weight, l2.bias):
        t.data.copy_(flat[off:off + t.numel()].view_as(t))
        off += t.numel()
    nets.append(torch.nn.Sequential(l1, torch.nn.ReLU(), l2).cuda())
assert off == flat.numel()
opt = torch.optim.Adam([p for n in nets for p in n.parameters()], lr=LR)


def epoch_fused(order):
    for lo in range(0, order.numel(), BATCH):
        probe.train_step(order[lo:lo + BATCH])


def epoch_torch(order):
    for lo in range(0, order.numel(), BATCH):
        rows = order[lo:lo + BATCH]
        xb = X[rows]
        opt.zero_grad(set_to_none=True)
        loss = sum(F.cross_entropy(net(xb), table[a][rows]) for a, net in enumerate(nets))
        loss.backward()
        opt.step()


def timed(fn, order):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn(order)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


orders = [train[torch.randperm(train.numel(), generator=g).cuda()] for _ in range(2)]
for _ in range(WARM):
    epoch_fused(orders[0])
    epoch_torch(orders[0])
torch.cuda.synchronize()
ms = {"fused": [], "torch": []}
for r in range(REPS):
    o = orders[r % 2]
    ms["fused"].append(timed(epoch_fused, o))
    ms["torch"].append(timed(epoch_torch, o))
probe.check_device_errors()

# the two sides took the same steps from the same init on the same batches: their parameters stay close
ref = torch.cat([p.detach().reshape(-1) for n in nets for p in n.parameters()])
drift = float((probe.params - ref).abs().max())

_C.prof_enable(True)
_C.prof_reset()
epoch_fused(orders[0])
torch.cuda.synchronize()
prof, work = _C.prof_read(), _C.prof_read_work()
_C.prof_enable(False)
step_ms, step_n = prof["probe_step_kernel"]
apply_ms, apply_n = prof["probe_apply_kernel"]


def summary(v):
    v = np.array(v)
    return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max()), "reps": len(v)}


res = {"U": U, "D": D, "H": H, "classes": CLASSES, "batch": BATCH, "steps_per_epoch": n_steps,
       "fused_epoch": summary(ms["fused"]), "torch_epoch": summary(ms["torch"]),
       "torch_over_fused": float(np.median(ms["torch"]) / np.median(ms["fused"])),
       "launches_per_step": (step_n + apply_n) / n_steps, "other_kernels_in_the_epoch": sorted(set(prof) - {"probe_step_kernel", "probe_apply_kernel"}),
       "step_kernel_us": 1e3 * step_ms / step_n, "apply_kernel_us": 1e3 * apply_ms / apply_n,
       "step_kernel_flop": work["probe_step_kernel"] / step_n,
       "step_kernel_share_of_fp32_mfma_peak": work["probe_step_kernel"] / (step_ms * 1e-3) / PEAK,
       "max_abs_parameter_difference_after_the_timed_epochs": drift}
print(json.dumps(res))

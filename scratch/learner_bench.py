"""The lazy tables' training pair per learner: fr_table_gather_train + fr_table_apply_grad (default sweeper period) on the
configs[4] item table (10 M x 256) and configs[2]'s user table (10 M x 128), B = 8192 uniform ids, weight decay 0 and
1e-3, on device events over warm steps.  Also each learner's HBM footprint of the table (weights + state).  Prints one
JSON line per case."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "recbole-fairrec_amd")]
import torch

from fairrec.optim import (LEARNER_ADAGRAD, LEARNER_ADAM, LEARNER_RMSPROP, LEARNER_SGD, AdagradHyper, AdamHyper,
                           LazyTable, RMSpropHyper, SGDHyper)

DEV = "cuda"
N, B, WARM, STEPS = 10_000_000, 8192, 20, 50


def hyper(name, wd):
    return {"adam": lambda: AdamHyper(1e-3, wd, device=DEV), "sgd": lambda: SGDHyper(1e-3, wd, device=DEV),
            "adagrad": lambda: AdagradHyper(1e-3, weight_decay=wd, device=DEV),
            "rmsprop": lambda: RMSpropHyper(1e-3, weight_decay=wd, device=DEV)}[name]()


ID = {"adam": LEARNER_ADAM, "sgd": LEARNER_SGD, "adagrad": LEARNER_ADAGRAD, "rmsprop": LEARNER_RMSPROP}


def case(name, D, wd):
    g = torch.Generator(device=DEV).manual_seed(0)
    t = LazyTable(torch.randn(N, D, device=DEV, generator=g) * 0.1)
    t.set_learner(ID[name])
    t.ensure_state()
    h = hyper(name, wd)
    ids = [torch.randint(0, N, (B,), device=DEV, generator=g) for _ in range(8)]
    grad = torch.randn(B, D, device=DEV, generator=g) * 1e-2
    sweep = t.default_sweep(B)
    def step(k):
        t.gather_train(h, ids[k % 8])
        t.apply_grad(h, grad, sweep)
    for k in range(WARM):
        step(k)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(STEPS):
        step(k)
    b.record()
    torch.cuda.synchronize()
    state = sum(x.numel() * 4 for x in (t.m, t.v) if x is not None)
    out = dict(learner=name, rows=N, dim=D, B=B, wd=wd, sweep_period=sweep, us_per_step=round(a.elapsed_time(b) / STEPS * 1e3, 1),
               weights_GB=round(N * D * 4 / 1e9, 2), state_GB=round(state / 1e9, 2))
    del t
    torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    for D in (256, 128):
        for wd in (0.0, 1e-3):
            for name in ("adam", "sgd", "adagrad", "rmsprop"):
                print(json.dumps(case(name, D, wd)), flush=True)

"""Times fairrec.evaluator.bootstrap_group_sums (fr_bootstrap_group_sums: the weights made in registers) against a torch baseline
on the same GPU that computes the same quantity from MATERIALISED weights: torch.poisson for blocks of 65 536 rows, one fp64
matmul per (block, group slice).  The baseline matches in distribution, not in bits (another generator).

    python profiles/bootstrap_probe.py --out profiles/bootstrap_probe_mi355x.json

Device events around work that ends in a synchronise; every shape warmed up; the two contenders alternate `--repeats` times in
one process; min / median / max of each are written, with the library's workspace bytes and the baseline's peak memory.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recbole-fairrec_amd"))

from fairrec import _C  # noqa: E402
from fairrec.evaluator import bootstrap_group_sums  # noqa: E402
from fairrec.evaluator.groups import group_segments  # noqa: E402

BLOCK = 65536


def baseline(values, gidx, G, B):
    """(sums [G, B, C], weight [G, B]) from materialised Poisson(1) weights, block by block"""
    perm, start = group_segments(gidx, G)
    sorted_values = values[perm]
    bounds = start.cpu().tolist()
    U, C = values.shape
    sums = torch.zeros((G, B, C), dtype=torch.float64, device=values.device)
    weight = torch.zeros((G, B), dtype=torch.float64, device=values.device)
    ones = torch.ones((min(BLOCK, U), B), dtype=torch.float64, device=values.device)
    for lo in range(0, U, BLOCK):
        hi = min(lo + BLOCK, U)
        w = torch.poisson(ones[:hi - lo])
        for g in range(G):
            a, b = max(bounds[g], lo), min(bounds[g + 1], hi)
            if a < b:
                wg = w[a - lo:b - lo]
                sums[g] += wg.t() @ sorted_values[a:b]
                weight[g] += wg.sum(dim=0)
    return sums, weight


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop), out


def spread(ms):
    return {"min_ms": round(min(ms), 3), "median_ms": round(statistics.median(ms), 3), "max_ms": round(max(ms), 3), "runs": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--cols", type=int, default=8)
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--groups", type=int, nargs="+", default=[2, 64])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this probe measures on the GPU"
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(5)
    values = torch.rand((a.rows, a.cols), dtype=torch.float64, device=dev, generator=gen)
    result = {"device": torch.cuda.get_device_name(0), "rows": a.rows, "cols": a.cols, "replicates": a.reps, "cases": []}
    for G in a.groups:
        gidx = torch.randint(0, G, (a.rows,), device=dev, generator=gen)
        kernel = lambda: bootstrap_group_sums(values, gidx, G, a.reps, 2020)       # noqa: E731
        torch_way = lambda: baseline(values, gidx, G, a.reps)                       # noqa: E731
        (_, (s, w)), (_, (bs, bw)) = timed(kernel), timed(torch_way)               # warm-up of both, and a sanity check:
        mean, bmean = (s[:, :, 0] / w).mean().item(), (bs[:, :, 0] / bw).mean().item()
        assert abs(mean - 0.5) < 0.01 and abs(bmean - 0.5) < 0.01, (mean, bmean)   # replicate means of uniform values
        del s, w, bs, bw
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        timed(torch_way)
        peak = torch.cuda.max_memory_allocated() - before
        t_kernel, t_base = [], []
        for _ in range(a.repeats):
            t_kernel.append(timed(kernel)[0])
            t_base.append(timed(torch_way)[0])
        case = {"groups": G, "bootstrap_group_sums": spread(t_kernel), "torch_materialised": spread(t_base),
                "workspace_bytes": int(_C.lib().fr_bootstrap_group_sums_workspace_bytes(a.rows, a.cols, G, a.reps)),
                "torch_peak_bytes": int(peak),
                "weight_matrix_bytes_if_stored_whole": a.rows * a.reps * 8}
        print(json.dumps(case), flush=True)
        result["cases"].append(case)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

"""Times fairrec.evaluator.bootstrap_fairness (fr_bootstrap_fair_metrics: every replicate in one walk of the item-sorted members,
the weights made in registers) against what a user could do before it on the same tree: resample the users explicitly and run
fairrec.evaluator.fairness_metrics on the repeated rows, once per replicate.  The baseline is timed for `--baseline-reps`
replicates and scaled to B; it matches in distribution, not in bits (torch.poisson, another generator).

    python profiles/fair_bootstrap_probe.py --out profiles/fair_bootstrap_probe_mi355x.json

Members over items by a Zipf popularity (weight 1 / rank), so the longest item -- which one wave walks alone -- shows; its share
of the members is written out.  Device events around work that ends in a synchronise; every shape warmed up; the two contenders
alternate `--repeats` times in one process; min / median / max of each are written.
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
from fairrec.evaluator import bootstrap_fairness, fairness_metrics  # noqa: E402


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
    ap.add_argument("--members", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--users", type=int, default=50_000)
    ap.add_argument("--reps", type=int, nargs="+", default=[200, 1000])
    ap.add_argument("--baseline-reps", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this probe measures on the GPU"
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(5)
    M, K, U = a.members, a.items, a.users
    popularity = 1.0 / torch.arange(1, K + 1, dtype=torch.float64, device=dev)
    items = torch.multinomial(popularity, M, replacement=True, generator=gen) + 1
    user = torch.sort(torch.randint(0, U, (M,), device=dev, generator=gen)).values
    gender = torch.randint(0, 2, (U,), device=dev, generator=gen).to(torch.float32)
    attr = gender[user]
    group = attr.to(torch.int32)
    score = torch.rand(M, device=dev, generator=gen)
    ones = torch.ones(M, device=dev)
    longest = int(torch.bincount(items).max())
    result = {"device": torch.cuda.get_device_name(0), "members": M, "items": K, "users": U, "groups": 2,
              "longest_item_members": longest, "longest_item_share": round(longest / M, 4), "cases": []}

    def baseline():
        out = []
        for _ in range(a.baseline_reps):
            w = torch.poisson(torch.ones(U, device=dev)).to(torch.int64)
            idx = torch.repeat_interleave(torch.arange(M, device=dev), w[user])
            out.append(fairness_metrics(score[idx], items[idx], {"gender": attr[idx]}, mode="full"))
        return out

    for B in a.reps:
        fused = lambda: bootstrap_fairness(items, group, score, ones, user, 2, B, 2020, value_type=True)        # noqa: E731
        (_, rep), (_, base) = timed(fused), timed(baseline)                         # warm-up of both, and a sanity check:
        key = "Value Unfairness of sensitive attribute gender"
        mean, bmean = float(rep["value"].mean()), sum(r[key] for r in base) / len(base)
        assert abs(mean - bmean) < 0.2 * bmean, (mean, bmean)                      # the replicates scatter around one value
        t_fused, t_base = [], []
        for _ in range(a.repeats):
            t_fused.append(timed(fused)[0])
            t_base.append(timed(baseline)[0] * B / a.baseline_reps)
        case = {"replicates": B, "bootstrap_fairness": spread(t_fused), "fairness_metrics_per_replicate_scaled": spread(t_base),
                "ratio_of_medians": round(statistics.median(t_base) / statistics.median(t_fused), 2),
                "workspace_bytes": int(_C.lib().fr_bootstrap_fair_metrics_workspace_bytes(M, K, 2, B))}
        print(json.dumps(case), flush=True)
        result["cases"].append(case)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

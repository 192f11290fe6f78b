"""fr_exposure_grouped at U = 1 000 001 users, N = 100 001 items, K = 50, topk [10, 20, 50], Zipf-popular lists, G = 2 / 21 / 294:
"index" (key build + torch.sort + group_start) and "kernel" (the library call: memset, exposure_heads_kernel, exposure_fold_kernel)
apart, against what a user has to do without it: a host loop over the groups that calls the six existing exposure functions on
each group's rows.  Device events, 5 warm calls, median of 20 (the host loop: median of 5 after 2 warm calls once one pass takes
more than half a second; the JSON says which)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "recbole-fairrec_amd")]
from fairrec import _C  # noqa: E402
from fairrec.evaluator import metrics as M  # noqa: E402

lib = _C.lib()
U, N, K, TOPK = 1_000_001, 100_001, 50, [10, 20, 50]
GROUPS = [int(x) for x in os.environ.get("EXPOSURE_TIMING_GROUPS", "2,21,294").split(",")]
g = torch.Generator(device="cpu").manual_seed(3)
w = 1.0 / torch.arange(1, N, dtype=torch.float64) ** 1.05
cdf = torch.cumsum(w / w.sum(), 0).cuda()
items = (torch.searchsorted(cdf, torch.rand(U, K, generator=g, dtype=torch.float64).cuda()).clamp_(max=N - 2) + 1).contiguous()
counts = torch.bincount(items.reshape(-1)[::7], minlength=N)            # a training popularity in step with the lists
st = _C.current_stream()


def timed(fn, reps=20, warm=5):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    if time.perf_counter() - t0 > 0.5:
        reps, warm = 5, 2
    for _ in range(warm - 1):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts = np.array(ts)
    return {"median_us": float(np.median(ts)), "min_us": float(ts.min()), "p90_us": float(np.percentile(ts, 90)), "reps": reps}


def host_loop(gidx, G):
    """today's way: the six existing functions on each group's rows"""
    out = []
    for q in range(G):
        rows = items[gidx == q]
        out.append((M.gini_index(rows, N, TOPK), M.item_coverage(rows, N, TOPK), M.shannon_entropy(rows, TOPK),
                    M.popularity_percentage(rows, counts, TOPK), M.tail_percentage(rows, counts, TOPK),
                    M.average_popularity(rows, counts, TOPK)))
    return out


res = {"U": U, "N": N, "K": K, "topk": TOPK}
popular = M._popular_mask(counts).to(torch.uint8).contiguous()
tail = M._tail_mask(counts).to(torch.uint8).contiguous()
ks = (_C.c_int32 * len(TOPK))(*TOPK)
for G in GROUPS:
    gidx = torch.randint(0, G, (U,), generator=g).cuda()
    state = {}

    def index():
        keys = torch.sort((((gidx[:, None] * N + items) * K) + torch.arange(K, device="cuda", dtype=torch.int64)).reshape(-1)).values
        start = torch.zeros(G + 1, dtype=torch.int64, device="cuda")
        torch.cumsum(torch.bincount(gidx, minlength=G)[:G], 0, out=start[1:])
        state["keys"], state["start"] = keys, start

    res[f"G={G} index"] = timed(index)
    out_i = torch.empty((G, len(TOPK), 5), dtype=torch.int64, device="cuda")
    out_e = torch.empty((G, len(TOPK)), dtype=torch.float64, device="cuda")
    ws = torch.empty(lib.fr_exposure_grouped_workspace_bytes(U, K, G, len(TOPK)), dtype=torch.uint8, device="cuda")
    res[f"G={G} workspace_MiB"] = ws.numel() / 2 ** 20
    res[f"G={G} kernel"] = timed(lambda: _C.check(lib.fr_exposure_grouped(
        state["keys"].data_ptr(), U * K, N, K, state["start"].data_ptr(), G, ks, len(TOPK), popular.data_ptr(), tail.data_ptr(),
        counts.data_ptr(), out_i.data_ptr(), out_e.data_ptr(), ws.data_ptr(), ws.numel(), st), "fr_exposure_grouped"))
    res[f"G={G} group_exposure_metrics"] = timed(lambda: M.group_exposure_metrics(items, gidx, G, N, counts, TOPK, M.EXPOSURE_NAMES))
    res[f"G={G} host loop over the six functions"] = timed(lambda: host_loop(gidx, G))
    chain = res[f"G={G} index"]["median_us"] + res[f"G={G} kernel"]["median_us"]
    res[f"G={G} host loop / (index + kernel)"] = res[f"G={G} host loop over the six functions"]["median_us"] / chain
    # the two ways agree: coverage and Gini bit for bit up to torch's reciprocal division, the rest to 1e-12
    mine = M.group_exposure_metrics(items, gidx, G, N, counts, TOPK, M.EXPOSURE_NAMES)
    theirs = host_loop(gidx, min(G, 3))
    worst = 0.0
    for q, dicts in enumerate(theirs):
        for d in dicts:
            for key, v in d.items():
                worst = max(worst, abs(mine[key][q] - v) / max(abs(v), 1e-300))
    res[f"G={G} max rel diff to the six functions (first groups)"] = worst
    assert worst < 1e-12, worst
    print(json.dumps({k: v for k, v in res.items() if k.startswith(f"G={G}")}, indent=1), flush=True)
print(json.dumps(res, indent=1))

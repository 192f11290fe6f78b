"""fr_topk_metrics_grouped against fr_topk_metrics at U = 1 000 001, K = 50, G = 2 and 1 000: device events, medians."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "recbole-fairrec_amd")]
from fairrec import _C  # noqa: E402

lib = _C.lib()
U, K = 1_000_001, 50
g = torch.Generator(device="cpu").manual_seed(3)
rec = (torch.rand(U, K + 1, generator=g) < 0.2).to(torch.int32)
rec[:, K] = torch.randint(1, 30, (U,), generator=g, dtype=torch.int32)
rec = rec.cuda()
st = _C.current_stream()


def timed(fn, reps=30, warm=5):
    for _ in range(warm):
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
    return {"median_us": float(np.median(ts)), "min_us": float(ts.min()), "p90_us": float(np.percentile(ts, 90))}


out0 = torch.empty(6 * K, dtype=torch.float64, device="cuda")
ws0 = torch.empty(lib.fr_topk_metrics_workspace_bytes(U, K), dtype=torch.uint8, device="cuda")
res = {"U": U, "K": K}
res["fr_topk_metrics"] = timed(lambda: _C.check(lib.fr_topk_metrics(rec.data_ptr(), U, K, out0.data_ptr(), ws0.data_ptr(),
                                                                     ws0.numel(), st), "plain"))
for G in (1, 2, 1000):
    gidx = torch.randint(0, G, (U,), generator=g).cuda()
    perm = torch.sort(gidx, stable=True).indices.contiguous()
    start = torch.zeros(G + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(torch.bincount(gidx, minlength=G), 0, out=start[1:])
    out = torch.empty(G * 6 * K, dtype=torch.float64, device="cuda")
    ws = torch.empty(lib.fr_topk_metrics_grouped_workspace_bytes(U, K, G), dtype=torch.uint8, device="cuda")
    for tag, p in (("sorted perm", perm.data_ptr()),) + ((("perm NULL", 0),) if G == 1 else ()):
        res[f"grouped G={G} {tag}"] = timed(lambda: _C.check(lib.fr_topk_metrics_grouped(
            rec.data_ptr(), p, start.data_ptr(), U, K, G, out.data_ptr(), ws.data_ptr(), ws.numel(), st), "grouped"))
    if G == 1:
        assert torch.equal(out.view(torch.int64), out0.view(torch.int64)), "G = 1 differs from fr_topk_metrics"
    else:
        # size-weighted mean of the groups against the plain call
        n = (start[1:] - start[:-1]).to(torch.float64)
        mean = (out.view(G, 6 * K) * n[:, None]).sum(0) / U
        res[f"grouped G={G} max rel diff of the weighted mean"] = float(((mean - out0).abs() / out0.abs()).max())
for k, v in res.items():
    if isinstance(v, dict) and k != "fr_topk_metrics":
        v["ratio_to_plain"] = v["median_us"] / res["fr_topk_metrics"]["median_us"]
print(json.dumps(res, indent=1))

"""Times every entry of the negative sampler (csrc/sampler.hip) and fr_randperm through the C ABI, one entry at a time.

    python profiles/sampler_probe.py --out run.json
    FAIRREC_HIP_LIB=scratch/lib/libfairrec_hip_parent.so python profiles/sampler_probe.py      # another build of the library

profiles/sampler_probe_mi355x.json holds three such runs of each of two builds (the commit before the sampler's consolidation and
the commit itself, alternating in one job), entry by entry, with the bound the later build was held to.

Device events around each call, every entry warmed up once, min / median / max of `--repeats` calls.  The stream is re-seeded
before every call, so each repeat of an entry does the same work.  Shapes:

* fr_sample_negatives, fr_sample_negatives_pop: bench.py's sampler line -- 8192 x 16 users x 100 negatives, bench.py's item_num,
  the used-sets of the training phase of its 2 M-interaction dataset;
* fr_sample_negatives_calls, fr_sample_negatives_pop_calls: the evaluation loader's -- 4096 single-user calls of 101, 202 or 303
  values; the uniform entry with a workspace that holds the speculative form and with one for the call-by-call form only;
* fr_randperm: 8.4 M elements (a 1024-step epoch of 8192-row batches).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "recbole-fairrec_amd"))

import bench  # noqa: E402   (sizes only)
from fairrec import _C  # noqa: E402
from fairrec.config import Config  # noqa: E402
from fairrec.data.dataset import synthetic_dataset  # noqa: E402
from fairrec.quick_start import split_dataset  # noqa: E402
from fairrec.sampler import Sampler  # noqa: E402
from fairrec.sampler.sampler import DeviceRandomState  # noqa: E402


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop)


def spread(ms):
    return {"min_ms": round(min(ms), 4), "median_ms": round(statistics.median(ms), 4), "max_ms": round(max(ms), 4), "runs": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=4096)
    ap.add_argument("--randperm", type=int, default=8192 * 1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this probe measures on the GPU"
    dev = torch.device("cuda")
    lib, stream = _C.lib(), _C.current_stream()
    cfg = Config(model="FOCF", config_dict={"device": str(dev), "eval_args": {"split": {"RS": [8, 1, 1]}, "group_by": "user",
                                                                             "order": "RO", "mode": "uni100"}})
    ds = synthetic_dataset(cfg, bench.N_USERS, bench.N_ITEMS, 2_000_000, seed=bench.SEED + 3)
    parts = split_dataset(ds)
    rs = DeviceRandomState(dev)
    smp = Sampler(["train", "valid", "test"], list(parts), "popularity", device=dev, random_state=rs)
    table = smp._pop_table
    indptr, items, _ = smp.set_phase("train").used_ids
    n_users, low, high = indptr.numel() - 1, 1, bench.N_ITEMS
    g = torch.Generator(device="cpu").manual_seed(bench.SEED + 4)
    uids = torch.randint(1, bench.N_USERS, (bench.BATCH * 16,), generator=g).to(dev)
    num, total = 100, bench.BATCH * 16 * 100
    call_keys = torch.randint(1, bench.N_USERS, (a.calls,), generator=g).to(dev)
    counts = 101 * torch.randint(1, 4, (a.calls,), generator=g)
    offsets = torch.zeros(a.calls + 1, dtype=torch.int64)
    torch.cumsum(counts, 0, out=offsets[1:])
    calls_total, max_call = int(offsets[-1]), int(counts.max())
    offsets = offsets.to(dev)

    def buf(nbytes):
        return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)
    ws_one = buf(lib.fr_sample_negatives_workspace_bytes(total))
    ws_lists = buf(lib.fr_sample_negatives_workspace_bytes(max_call))
    ws_spec = buf(max(lib.fr_sample_negatives_calls_workspace_bytes(calls_total, max_call), ws_lists.numel()))
    ws_perm = buf(lib.fr_randperm_workspace_bytes(a.randperm))
    out_one = torch.empty(total, dtype=torch.int64, device=dev)
    out_calls = torch.empty(calls_total, dtype=torch.int64, device=dev)
    out_perm = torch.empty(a.randperm, dtype=torch.int64, device=dev)
    st, err = rs.state.data_ptr(), rs.err_flag.data_ptr()
    used = (indptr.data_ptr(), items.data_ptr(), n_users)

    def uniform_calls(ws):
        return lambda: lib.fr_sample_negatives_calls(st, low, high, call_keys.data_ptr(), offsets.data_ptr(), a.calls, max_call,
                                                     *used, out_calls.data_ptr(), ws.data_ptr(), ws.numel(), err, stream)
    entries = {
        "fr_sample_negatives": lambda: lib.fr_sample_negatives(st, low, high, uids.data_ptr(), uids.numel(), num, *used,
                                                               out_one.data_ptr(), None, ws_one.data_ptr(), ws_one.numel(), err, stream),
        "fr_sample_negatives_calls[speculative workspace]": uniform_calls(ws_spec),
        "fr_sample_negatives_calls[call-by-call workspace]": uniform_calls(ws_lists),
        "fr_sample_negatives_pop": lambda: lib.fr_sample_negatives_pop(st, table, uids.data_ptr(), uids.numel(), num, *used,
                                                                       out_one.data_ptr(), None, ws_one.data_ptr(), ws_one.numel(), err,
                                                                       stream),
        "fr_sample_negatives_pop_calls": lambda: lib.fr_sample_negatives_pop_calls(st, table, call_keys.data_ptr(), offsets.data_ptr(),
                                                                                   a.calls, max_call, *used, out_calls.data_ptr(),
                                                                                   ws_lists.data_ptr(), ws_lists.numel(), err, stream),
        "fr_randperm": lambda: lib.fr_randperm(st, a.randperm, out_perm.data_ptr(), ws_perm.data_ptr(), ws_perm.numel(), stream),
    }
    result = {"device": torch.cuda.get_device_name(0), "library": os.path.basename(_C.LIB_PATH), "item_num": bench.N_ITEMS,
              "positions_per_call": total, "calls": a.calls, "call_values": calls_total, "randperm_n": a.randperm, "entries": {}}
    for name, call in entries.items():
        ms = []
        for rep in range(a.repeats + 1):      # the first one warms up
            rs.seed(bench.SEED)
            torch.cuda.synchronize()
            rc = []
            t = timed(lambda: rc.append(call()))
            _C.check(rc[0], name)
            if rep:
                ms.append(t)
        assert int(rs.err_flag.item()) == 0, name
        result["entries"][name] = spread(ms)
        print(json.dumps({name: result["entries"][name]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

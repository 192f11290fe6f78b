"""Full-sort evaluation: one `Trainer.evaluate` over the same FullSortEvalDataLoader under `full_sort_eval: matrix` (the dense
[users, n_items] scores, the two masking writes, torch.topk, fr_eval_meanrank_segments) and under `fused` (fr_recommend_topk,
fr_recommend_cells, fr_recommend_meanrank: no matrix).  Device events around the whole call, 5 warm runs, then the median and
min-max of 20; the kernels' own times come from the library's event profiler in a pass of its own.  One JSON line per row.

    python scratch/full_eval_bench.py [focf] [pfcn] [--mode matrix|fused|both]

`--mode matrix` sets nothing a commit before the key would not understand, so the same script times the parent commit."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "recbole-fairrec_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch

DEV = "cuda"
KERNELS = ("recommend_kernel", "topk_rows_kernel", "recommend_cells_kernel", "recommend_meanrank_kernel")


def timed(fn, warm=5, reps=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def kernel_times(fn):
    """{kernel: ms per evaluate} of one profiled call."""
    from fairrec import _C
    torch.cuda.synchronize()
    _C.prof_enable(True)
    _C.prof_reset()
    fn()
    torch.cuda.synchronize()
    got = _C.prof_read()
    _C.prof_enable(False)
    return {k: {"ms": round(got[k][0], 3), "launches": got[k][1]} for k in KERNELS if k in got}


def build(model_name, n_users, n_items, dim, extra, eval_users, users_per_batch):
    from fairrec.config import Config
    from fairrec.data.dataloader import FullSortEvalDataLoader
    from fairrec.data.dataset import synthetic_dataset
    from fairrec.data.interaction import Interaction
    from fairrec.quick_start import split_dataset
    from fairrec.sampler import Sampler
    from fairrec.utils import get_model, get_trainer, init_seed
    cfg = Config(model=model_name, config_dict=dict({
        "embedding_size": dim, "train_batch_size": 8192, "device": DEV, "epochs": 1, "checkpoint_dir": tempfile.mkdtemp(),
        "sst_attr_list": ["gender"], "eval_args": {"mode": "full"}, "metrics": ["NDCG"], "valid_metric": "NDCG@10", "topk": [10],
        "eval_batch_size": users_per_batch * n_items}, **extra))
    init_seed(2020)
    ds = synthetic_dataset(cfg, n_users, n_items, 2_000_000, seed=2023)
    train_set, valid_set, test_set = split_dataset(ds)
    phases = Sampler(["train", "valid", "test"], [train_set, valid_set, test_set], "uniform", device=DEV)
    test = FullSortEvalDataLoader(cfg, test_set, phases.set_phase("test"))
    test.uid_list = test.uid_list[:eval_users]                   # the evaluation set: its first users
    test.user_df = Interaction({k: v[:eval_users] for k, v in test.user_df.interaction.items()})
    model = get_model(model_name)(cfg, train_set).to(DEV)
    trainer = get_trainer(None, model_name)(cfg, model)          # binds the optimizer the lazy tables read their step from
    return cfg, model, test, trainer


def rows(name, cfg, trainer, test, modes, ks, gaucs, note=None):
    for k in ks:
        for gauc in gaucs:
            cfg["topk"], cfg["metrics"] = [k], ["NDCG"] + (["GAUC"] if gauc else [])
            for mode in modes:
                if mode == "fused" or hasattr(trainer, "full_sort_eval"):
                    trainer.full_sort_eval = mode
                run = lambda: trainer.evaluate(test, load_best_model=False)
                res = {"case": name, "mode": mode, "users": int(test.uid_list.numel()), "batches": len(test), "k": k, "gauc": gauc}
                if note:
                    res["note"] = note
                res.update(timed(run))
                res["kernels"] = kernel_times(run)
                print(json.dumps(res), flush=True)


if __name__ == "__main__":
    argv = sys.argv[1:]
    mode = argv[argv.index("--mode") + 1] if "--mode" in argv else "both"
    modes = ("matrix", "fused") if mode == "both" else (mode,)
    what = [a for a in argv if a in ("focf", "pfcn")] or ["focf", "pfcn"]
    if "focf" in what:
        cfg, model, test, trainer = build("FOCF", 1_000_001, 100_001, 64, {"fair_objective": "value"}, 14_480, 1_448)
        rows("FOCF 1000001 x 100001, D = 64", cfg, trainer, test, modes, (10, 50), (False, True))
        del cfg, model, test, trainer
        torch.cuda.empty_cache()
    if "pfcn" in what:
        # the matrix path scores every (user, item) pair through predict: 16 users of it (two per predict batch) are what fits
        # next to the tables; `fused` runs on the same 16 and, alone, on 1 448
        extra = {"filter_mode": "none"}
        cfg, model, test, trainer = build("PFCN_BiasedMF", 100_001, 1_000_001, 128, extra, 16, 2)
        rows("PFCN_BiasedMF 100001 x 1000001, D = 128", cfg, trainer, test, modes, (10,), (False, True))
        del cfg, model, test, trainer
        torch.cuda.empty_cache()
        if "fused" in modes:
            cfg, model, test, trainer = build("PFCN_BiasedMF", 100_001, 1_000_001, 128, extra, 1_448, 1_448)
            rows("PFCN_BiasedMF 100001 x 1000001, D = 128", cfg, trainer, test, ("fused",), (10,), (False, True), note="fused alone")

"""Inference through a PFCN filter: the fused launch (fr_mlp_infer, BatchNorm on running statistics) against the same module's
training-mode forward under no_grad, which is what an evaluation runs when `model.eval()` does not reach the filters
(fr_linear_fwd_bnstats + fr_bn_fwd_ex per layer).  The filter is [128, 256, 128] with BatchNorm and leakyrelu; M = 1 448 (the
users of one uni100 batch), 282 000 (the repeated rows of one evaluation batch through predict) and 1 000 000 (get_sst_embed
on a million users).  Both variants run in one process, alternating; device events, 5 warm calls, then the median and
min-max of 20.  Launch counts and the fused kernel's own time come from the library's event profiler in a pass of its own;
the kernel's bounds are the HBM time of its traffic (M x (128 + 128) floats; weights stay in L2) and the fp32-MFMA time of
its 2 M (128 x 256 + 256 x 128) FLOP.  `end2end`: full_sort_topk for 1 448 users of a trained PFCN_BiasedMF sm model
(100 001 synthetic items, k = 10) under filter_eval_statistics batch and running.
Prints one JSON line per case.  `python scratch/mlp_infer_bench.py [filter] [end2end]`"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "recbole-fairrec_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch

DEV = "cuda"
PEAK_TF = 157.3          # fp32 MFMA, TFLOP/s
PEAK_HBM = 8.0e12        # bytes/s
SIZES = (1448, 282_000, 1_000_000)


def alternating(variants, warm=5, reps=20):
    """{name: {median_us, min_us, max_us}} of callables timed turn by turn."""
    for _ in range(warm):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ts = {n: [] for n in variants}
    for _ in range(reps):
        for n, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts[n].append(a.elapsed_time(b) * 1e3)
    return {n: {"median_us": round(float(np.median(t)), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}
            for n, t in ts.items()}


def profile(fn, reps=5):
    """{kernel: (mean us per call of fn, launches per call)} from the library's event pairs."""
    from fairrec import _C
    fn()
    torch.cuda.synchronize()
    _C.prof_enable(True)
    _C.prof_reset()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    out = {k: (round(ms * 1e3 / reps, 1), n / reps) for k, (ms, n) in _C.prof_read().items()}
    _C.prof_enable(False)
    return out


def filter_case():
    from fairrec.model.layers import MLPLayers
    torch.manual_seed(0)
    D = 128
    mlp = MLPLayers([D, 2 * D, D], activation="leakyrelu", bn=True, init_method="norm").to(DEV)
    with torch.no_grad():
        for _ in range(3):
            mlp(torch.randn(4096, D, device=DEV))
    twin = MLPLayers([D, 2 * D, D], activation="leakyrelu", bn=True, init_method="norm").to(DEV)
    twin.load_state_dict(mlp.state_dict())
    mlp.eval()
    for M in SIZES:
        x = torch.randn(M, D, device=DEV)

        def fused():
            with torch.no_grad():
                return mlp(x)

        def layered():
            with torch.no_grad():
                return twin(x)

        res = {"case": "filter [128, 256, 128] bn leakyrelu", "M": M}
        res.update(alternating({"fused_eval": fused, "layered_train_mode": layered}))
        pf, pl = profile(fused), profile(layered)
        res["fused_launches"] = sum(n for _, n in pf.values())
        res["layered_launches"] = sum(n for _, n in pl.values())
        res["layered_kernels_us"] = {k: v[0] for k, v in pl.items()}
        kt = pf.get("mlp_infer_kernel", (None, 0))[0]
        if kt:
            flop, byts = 2.0 * M * (D * 2 * D + 2 * D * D), 4.0 * M * 2 * D
            t_mfma, t_hbm = flop / (PEAK_TF * 1e12) * 1e6, byts / PEAK_HBM * 1e6
            res["mlp_infer_kernel"] = {"mean_us": kt, "tflops": round(flop / (kt * 1e-6) / 1e12, 2), "gb_per_s": round(byts / (kt * 1e-6) / 1e9, 1),
                                       "hbm_bound_us": round(t_hbm, 1), "mfma_bound_us": round(t_mfma, 1),
                                       "share_of_hbm_bound": round(t_hbm / kt, 3), "share_of_mfma_bound": round(t_mfma / kt, 3)}
        print(json.dumps(res), flush=True)
        del x
        torch.cuda.empty_cache()


def end_to_end_case():
    from fairrec.config import Config
    from fairrec.data.dataloader import FullSortEvalDataLoader
    from fairrec.data.dataset import synthetic_dataset
    from fairrec.quick_start import run_recbole, split_dataset
    from fairrec.sampler import Sampler
    from fairrec.utils.case_study import full_sort_topk
    res = {"case": "full_sort_topk, PFCN_BiasedMF sm, 100 001 items, k = 10, 1 448 users"}
    for stats in ("batch", "running"):
        # one epoch with a cheap evaluation (uni100), then the recommendation request through a full-sort loader of the test set
        cfg_dict = {"epochs": 1, "train_batch_size": 8192, "device": DEV, "embedding_size": 64, "learning_rate": 0.001, "eval_args": {"mode": "uni100"},
                    "topk": [10], "valid_metric": "ndcg@10", "metrics": ["NDCG"], "sst_attr_list": ["gender"], "filter_mode": "sm",
                    "train_epoch_interval": 1, "filter_eval_statistics": stats, "checkpoint_dir": tempfile.mkdtemp()}
        cfg = Config(model="PFCN_BiasedMF", config_dict=cfg_dict)
        splits = split_dataset(synthetic_dataset(cfg, 20_001, 100_001, 400_000, seed=2023))
        seen = {}
        try:
            run_recbole(model="PFCN_BiasedMF", saved=False, splits=splits, config_dict=cfg_dict,
                        before_fit=lambda m, t: seen.update(model=m, trainer=t))
            trained = True
        except ValueError as e:      # a diverged epoch ('Training loss is nan'): time the model as it stands, and say so
            trained = f"no ({e}); filters' statistics moved by three training-mode forwards"
            with torch.no_grad():
                seen["model"].train()
                for _ in range(3):
                    seen["model"]._filter(torch.randn(4096, cfg_dict["embedding_size"], device=DEV), ["gender"])
        model = seen["model"]
        full_cfg = Config(model="PFCN_BiasedMF", config_dict=dict(cfg_dict, eval_args={"mode": "full"}))
        phases = Sampler(["train", "valid", "test"], list(splits), "uniform", device=DEV)
        test = FullSortEvalDataLoader(full_cfg, splits[2], phases.set_phase("test"))
        uids = test.uid_list[:1448]
        res[stats] = dict(users=int(uids.numel()), trained=trained,
                          **alternating({"f": lambda: full_sort_topk(uids, model, test, 10, sst_list=["gender"])})["f"])
        del model, seen, test
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    what = sys.argv[1:] or ["filter", "end2end"]
    if "filter" in what:
        filter_case()
    if "end2end" in what:
        end_to_end_case()

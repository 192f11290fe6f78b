"""PFCN_DMF recommendation: utils/case_study.full_sort_topk under `full_sort_scorer: pairs` (predict on every pair, the two
masking writes, fr_topk_rows) against `towers` (each tower once per row, fr_rows_l2_normalize, fr_recommend_topk).
filter_mode sm, 20 001 items, D = 64, 64 users, k = 10, 8 users per predict batch.  Both variants run in one process,
alternating; device events, 5 warm calls, then the median and min-max of 20.  The item side of `towers` (flush, item tower
over the catalogue, normalisation) is the hook on an empty request; the normalisation kernel's own time comes from the
library's event profiler in a pass of its own.  Prints one JSON line.
Run it under a time limit of its own:  timeout -k 10 600 python scratch/dmf_towers_bench.py"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "recbole-fairrec_amd")]
import numpy as np
import torch

DEV = "cuda"
N_ITEMS, DIM, USERS, K, PER = 20001, 64, 64, 10, 8


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


def kernel_times(fn, names, reps=5):
    """{kernel name: mean device us per launch} over `reps` calls of fn (the library's event pairs around each kernel)."""
    from fairrec import _C
    fn()
    torch.cuda.synchronize()
    _C.prof_enable(True)
    _C.prof_reset()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    got = _C.prof_read()
    _C.prof_enable(False)
    return {n: (round(got[n][0] * 1e3 / got[n][1], 2), got[n][1] // reps) for n in names if n in got}


def build():
    from fairrec.config import Config
    from fairrec.data.dataloader import FullSortEvalDataLoader
    from fairrec.data.dataset import synthetic_dataset
    from fairrec.quick_start import split_dataset
    from fairrec.sampler import Sampler
    from fairrec.utils import get_model, get_trainer, init_seed
    cfg = Config(model="PFCN_DMF", config_dict={
        "embedding_size": DIM, "train_batch_size": 8192, "device": DEV, "epochs": 1, "checkpoint_dir": tempfile.mkdtemp(),
        "sst_attr_list": ["gender"], "eval_args": {"mode": "full"}, "metrics": ["NDCG"], "valid_metric": "NDCG@5", "topk": [5],
        "eval_batch_size": PER * N_ITEMS, "filter_mode": "sm", "dis_hidden_size_list": [64, 32]})
    init_seed(2020)
    ds = synthetic_dataset(cfg, 2000, N_ITEMS, 200_000, seed=2023)
    train_set, valid_set, test_set = split_dataset(ds)
    phases = Sampler(["train", "valid", "test"], [train_set, valid_set, test_set], "uniform", device=DEV)
    test = FullSortEvalDataLoader(cfg, test_set, phases.set_phase("test"))
    model = get_model("PFCN_DMF")(cfg, train_set).to(DEV)
    get_trainer(None, "PFCN_DMF")(cfg, model)      # binds the optimizer the lazy tables read their step from
    # the towers' Linear layers start as N(0, 1e-4): nearly every ReLU output is dead; a seeded N(0, 1 / n_in) draw instead
    rng = np.random.default_rng(11)
    with torch.no_grad():
        for mlp in (model.user_mlp, model.item_mlp):
            for lin in mlp.linears():
                lin.weight.copy_(torch.from_numpy((rng.standard_normal(tuple(lin.weight.shape)) / np.sqrt(lin.in_features)).astype(np.float32)))
                lin.bias.copy_(torch.from_numpy((0.25 * rng.standard_normal(lin.out_features)).astype(np.float32)))
    model.eval()
    return model, test


def main():
    if not torch.cuda.is_available():
        raise SystemExit("dmf_towers_bench: needs a ROCm device; there is no CPU path")
    from fairrec.data.interaction import Interaction
    from fairrec.functional import rows_l2_normalize
    from fairrec.utils.case_study import full_sort_topk
    model, test = build()
    uids = test.uid_list[:USERS]
    assert len(uids) == USERS
    sst = ["gender"]
    ds = test.dataset
    none = ds.join(Interaction({ds.uid_field: uids[:0]})).to(DEV)

    def run(name):
        model.full_sort_scorer = name
        return full_sort_topk(uids, model, test, K, sst_list=sst)

    def item_side():
        model.full_sort_scorer = "towers"
        with torch.no_grad():
            return model.full_sort_factors(none, sst, users_per_batch=PER)

    vp, ip = run("pairs")
    vt, it = run("towers")
    same = float((ip == it).float().mean())
    gap = float((vp - vt).abs().max())
    t = alternating({"pairs": lambda: run("pairs"), "towers": lambda: run("towers"), "towers_item_side": item_side})
    x = torch.randn(N_ITEMS, DIM, device=DEV)
    kt = kernel_times(lambda: run("towers"), ["rows_l2_normalize_kernel", "recommend_kernel"])
    kn = kernel_times(lambda: rows_l2_normalize(x), ["rows_l2_normalize_kernel"], reps=20)
    print(json.dumps({"case": "pfcn_dmf_sm", "n_items": N_ITEMS, "dim": DIM, "users": USERS, "k": K, "users_per_batch": PER,
                      "times": t, "speedup": round(t["pairs"]["median_us"] / t["towers"]["median_us"], 2),
                      "item_side_share": round(t["towers_item_side"]["median_us"] / t["towers"]["median_us"], 3),
                      "kernels_in_a_towers_call_us_and_launches": kt, "normalize_20001x64_us": kn["rows_l2_normalize_kernel"][0],
                      "normalize_bytes_per_s": round(2 * N_ITEMS * DIM * 4 / (kn["rows_l2_normalize_kernel"][0] * 1e-6)),
                      "lists_equal_share": round(same, 4), "max_value_gap": gap}))


if __name__ == "__main__":
    main()

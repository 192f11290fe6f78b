"""Recommendation: utils/case_study.full_sort_topk on the fused kernel (fr_recommend_topk) against the composition that gives
the same answer from stock pieces -- the dense scores the Trainer's full-sort evaluation ranks (full_sort_predict, or predict
over every pair), the two masking writes, torch.topk -- and fr_topk_rows against torch.topk on a dense matrix.  Both variants
of a case run in one process, alternating; device events, 5 warm calls, then the median and min-max of 20.  The fused
kernel's own time comes from the library's event profiler in a pass of its own (FLOP/s = 2 U n_items D / kernel time).
Prints one JSON line per case.  `python scratch/recommend_bench.py [focf] [pfcn] [rows]`"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "recbole-fairrec_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch

DEV = "cuda"
USERS = 1448
PEAK_TF = 157.3


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


def kernel_time(fn, reps=5):
    """Mean device time of recommend_kernel over `reps` calls of fn, in us (the library's event pairs around the kernel)."""
    from fairrec import _C
    fn()
    torch.cuda.synchronize()
    _C.prof_enable(True)
    _C.prof_reset()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    ms, n = _C.prof_read().get("recommend_kernel", (0.0, 0))
    _C.prof_enable(False)
    return ms * 1e3 / n if n else None


def build(model_name, n_users, n_items, dim, extra):
    from fairrec.config import Config
    from fairrec.data.dataloader import FullSortEvalDataLoader
    from fairrec.data.dataset import synthetic_dataset
    from fairrec.quick_start import split_dataset
    from fairrec.sampler import Sampler
    from fairrec.utils import get_model, get_trainer, init_seed
    cfg = Config(model=model_name, config_dict=dict({
        "embedding_size": dim, "train_batch_size": 8192, "device": DEV, "epochs": 1, "checkpoint_dir": tempfile.mkdtemp(),
        "sst_attr_list": ["gender"], "eval_args": {"mode": "full"}, "metrics": ["NDCG"], "valid_metric": "NDCG@5", "topk": [5],
        "eval_batch_size": 2 * n_items}, **extra))
    init_seed(2020)
    ds = synthetic_dataset(cfg, n_users, n_items, 2_000_000, seed=2023)
    train_set, valid_set, test_set = split_dataset(ds)
    phases = Sampler(["train", "valid", "test"], [train_set, valid_set, test_set], "uniform", device=DEV)
    test = FullSortEvalDataLoader(cfg, test_set, phases.set_phase("test"))
    model = get_model(model_name)(cfg, train_set).to(DEV)
    trainer = get_trainer(None, model_name)(cfg, model)      # binds the optimizer the lazy tables read their step from
    model.eval()
    return model, test, trainer


def composition(model, test, uids, k, sst_list=None):
    """What gives the answer without the new kernels: the Trainer's dense scores, its two masking writes, torch.topk."""
    from fairrec.data.interaction import Interaction
    from fairrec.utils.case_study import dense_full_sort_scores, users_per_batch
    ds = test.dataset
    with torch.no_grad():
        inter = ds.join(Interaction({ds.uid_field: uids})).to(DEV)
        scores = dense_full_sort_scores(model, inter, ds.item_num, users_per_batch(test.config, ds.item_num), ds.iid_field,
                                        torch.device(DEV), sst_list)
        scores[:, 0] = -float("inf")
        hu, hi = test._rows(test.hist_indptr, test.hist_items, uids)
        scores[hu, hi] = -float("inf")
        return torch.topk(scores, k)


def agreement(a, b):
    """Share of users whose two value lists agree to 1e-5 (the lists may order tied or near-tied items differently)."""
    return round(float(((a[0] - b[0]).abs().max(dim=1).values <= 1e-5).float().mean()), 4)


def model_case(name, model_name, n_users, n_items, dim, extra, ks, comp_users):
    from fairrec.utils.case_study import full_sort_topk
    model, test, trainer = build(model_name, n_users, n_items, dim, extra)
    uids = test.uid_list[:USERS]
    sub = uids[:comp_users]
    for k in ks:
        fused = lambda: full_sort_topk(sub, model, test, k)
        comp = lambda: composition(model, test, sub, k)
        res = {"case": name, "n_items": n_items, "dim": dim, "k": k, "users": int(sub.numel()),
               "agreement": agreement(fused(), comp())}
        res.update(alternating({"full_sort_topk_fused": fused, "composition": comp}))
        full = lambda: full_sort_topk(uids, model, test, k)
        if sub.numel() != uids.numel():
            res["full_sort_topk_fused_all_users"] = dict(users=int(uids.numel()), **alternating({"f": full})["f"])
        kt = kernel_time(full)
        if kt:
            tf = 2.0 * uids.numel() * n_items * dim / (kt * 1e-6) / 1e12
            res["recommend_kernel"] = {"users": int(uids.numel()), "mean_us": round(kt, 1), "tflops": round(tf, 2),
                                       "share_of_fp32_mfma_peak": round(tf / PEAK_TF, 3)}
        print(json.dumps(res), flush=True)
    del model, test, trainer
    torch.cuda.empty_cache()


def rows_case():
    from fairrec.functional import topk_rows
    g = torch.Generator(device=DEV).manual_seed(1)
    s = torch.randn(USERS, 100_001, device=DEV, generator=g)
    for k in (10, 50):
        a, b = topk_rows(s, k), torch.topk(s, k)
        assert torch.equal(a[0], b[0])                      # equal values; torch.topk leaves the order of equal scores open
        res = {"case": "fr_topk_rows vs torch.topk", "shape": list(s.shape), "k": k,
               "rows_with_equal_indices": round(float((a[1] == b[1]).all(dim=1).float().mean()), 4)}
        res.update(alternating({"fr_topk_rows": lambda: topk_rows(s, k), "torch_topk": lambda: torch.topk(s, k)}))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    what = sys.argv[1:] or ["focf", "pfcn", "rows"]
    if "rows" in what:
        rows_case()
    if "focf" in what:
        model_case("FOCF", "FOCF", 1_000_001, 100_001, 64, {"fair_objective": "value"}, (10, 50), USERS)
    if "pfcn" in what:
        # the composition scores every (user, item) pair through predict: 16 users of it (two per predict batch) stand for the
        # 1 448 whose 5.8 GB matrix and gathered rows do not fit next to the tables; the fused path is also timed on all 1 448
        model_case("PFCN_BiasedMF", "PFCN_BiasedMF", 100_001, 1_000_001, 128, {"filter_mode": "none"}, (10,), 16)

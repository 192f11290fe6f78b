"""Recommendation from an MLP scorer: utils/case_study.full_sort_topk with `full_sort_scorer: split` (fr_pair_mlp_scores +
fr_topk_rows) against what the `pairs` path runs for the same answer -- dense_full_sort_scores (predict on every pair), the
two masking writes, fr_topk_rows.  NFCF, 1 000 001 users x 100 001 items, D = 256, [128, 64], k = 10.  Both variants run in
one process, alternating; device events, 5 warm calls, then the median and min-max of 20.  The composition scores every
pair through predict and is timed on COMP_USERS users (two per predict batch); the split path is also timed alone on 1 448.
The scoring kernel's own time comes from the library's event profiler in a pass of its own; its FLOP count is
users * items * (n1 + sum 2 n_in n_out) over the layers above the first.  Prints one JSON line."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "recbole-fairrec_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch

from recommend_bench import DEV, PEAK_TF, USERS, alternating

COMP_USERS = 16


def kernel_time(fn, name, reps=5):
    from fairrec import _C
    fn()
    torch.cuda.synchronize()
    _C.prof_enable(True)
    _C.prof_reset()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    ms, n = _C.prof_read().get(name, (0.0, 0))
    _C.prof_enable(False)
    return ms * 1e3 / n if n else None


def build(n_users, n_items, dim, hidden):
    from fairrec.config import Config
    from fairrec.data.dataloader import FullSortEvalDataLoader
    from fairrec.data.dataset import synthetic_dataset
    from fairrec.quick_start import split_dataset
    from fairrec.sampler import Sampler
    from fairrec.utils import get_model, get_trainer, init_seed
    cfg = Config(model="NFCF", config_dict={
        "embedding_size": dim, "mlp_hidden_size": hidden, "train_batch_size": 8192, "device": DEV, "epochs": 1,
        "checkpoint_dir": tempfile.mkdtemp(), "sst_attr_list": ["gender"], "eval_args": {"mode": "full"}, "metrics": ["NDCG"],
        "valid_metric": "NDCG@5", "topk": [5], "eval_batch_size": 2 * n_items, "load_pretrain_path": None, "LABEL_FIELD": "label",
        "full_sort_scorer": "split"})
    init_seed(2020)
    ds = synthetic_dataset(cfg, n_users, n_items, 2_000_000, seed=2023)
    train_set, valid_set, test_set = split_dataset(ds)
    phases = Sampler(["train", "valid", "test"], [train_set, valid_set, test_set], "uniform", device=DEV)
    test = FullSortEvalDataLoader(cfg, test_set, phases.set_phase("test"))
    model = get_model("NFCF")(cfg, train_set).to(DEV)
    trainer = get_trainer(None, "NFCF")(cfg, model)      # binds the optimizer the lazy tables read their step from
    model.eval()
    return model, test, trainer


def composition(model, test, uids, k):
    from fairrec.data.interaction import Interaction
    from fairrec.functional import topk_rows
    from fairrec.utils.case_study import dense_full_sort_scores, users_per_batch
    ds = test.dataset
    with torch.no_grad():
        inter = ds.join(Interaction({ds.uid_field: uids})).to(DEV)
        scores = dense_full_sort_scores(model, inter, ds.item_num, users_per_batch(test.config, ds.item_num), ds.iid_field,
                                        torch.device(DEV), None)
        scores[:, 0] = -float("inf")
        hu, hi = test._rows(test.hist_indptr, test.hist_items, uids)
        scores[hu, hi] = -float("inf")
        return topk_rows(scores, k)


if __name__ == "__main__":
    from fairrec.utils.case_study import full_sort_topk
    n_users, n_items, dim, hidden, k = 1_000_001, 100_001, 256, [128, 64], 10
    model, test, trainer = build(n_users, n_items, dim, hidden)
    uids = test.uid_list[:USERS]
    sub = uids[:COMP_USERS]
    split = lambda: full_sort_topk(sub, model, test, k)
    comp = lambda: composition(model, test, sub, k)
    a, b = split(), comp()
    res = {"case": "NFCF full_sort_topk, split against pairs", "n_users": n_users, "n_items": n_items, "dim": dim, "hidden": hidden,
           "k": k, "users": int(sub.numel()),
           "users_whose_values_agree_to_1e-5": round(float(((a[0] - b[0]).abs().max(dim=1).values <= 1e-5).float().mean()), 4)}
    res.update(alternating({"full_sort_topk_split": split, "composition_pairs": comp}))
    full = lambda: full_sort_topk(uids, model, test, k)
    res["full_sort_topk_split_all_users"] = dict(users=int(uids.numel()), **alternating({"f": full})["f"])
    kt = kernel_time(full, "pair_mlp_kernel")
    if kt:
        widths = [hidden[0]] + hidden[1:] + [1]
        flop = float(uids.numel()) * n_items * (widths[0] + sum(2 * i * o for i, o in zip(widths[:-1], widths[1:])))
        tf = flop / (kt * 1e-6) / 1e12
        res["pair_mlp_kernel"] = {"users": int(uids.numel()), "mean_us": round(kt, 1), "tflops": round(tf, 2),
                                  "share_of_fp32_mfma_time_of_its_flops": round(tf / PEAK_TF, 3)}
    print(json.dumps(res), flush=True)

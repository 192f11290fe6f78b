"""Popularity-biased negatives on the device (fr_sample_negatives_pop) against the uniform sampler at the same shape and the
numpy host path they replace (the former Sampler._pop_sample_by_user_ids: state hand-over, used-key rebuild, numpy draws,
searchsorted membership), timed in the same run; then `popN` evaluation against `uni100` at bench.py's next_rows shapes.
Device events over warm repeated calls (median, min, max); the host path on the host clock around a device synchronise.
Prints one JSON line per case.  `python scratch/pop_neg_bench.py [train] [eval]`"""
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "recbole-fairrec_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch

DEV = "cuda"


class _DS:
    uid_field, iid_field = "user_id", "item_id"

    def __init__(self, user_num, item_num, u, i):
        self.user_num, self.item_num = user_num, item_num
        self.inter_feat = {"user_id": torch.from_numpy(u), "item_id": torch.from_numpy(i)}


def dev_timed(fn, reps=30):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return {"median_us": round(float(np.median(ts)), 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1)}


def host_timed(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return {"median_us": round(float(np.median(ts)), 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1)}


def host_path(smp, user_ids, num):
    """The numpy path the device kernel replaces, as it stood (sampler.py before this change)."""
    keys_t = smp._pop_host
    indptr, items, _ = smp.used_ids
    ip, it = indptr.cpu().numpy(), items.cpu().numpy().astype(np.int64)
    keys = np.tile(user_ids.cpu().numpy().astype(np.int64), num)
    used_key = keys * smp.item_num
    allk = np.repeat(np.arange(smp.user_num, dtype=np.int64), np.diff(ip)) * smp.item_num + it
    value = np.zeros(len(keys), dtype=np.int64)
    check = np.arange(len(keys))
    np.random.set_state(smp.rs.get_state())
    while len(check) > 0:
        k_, p_, a_ = keys_t
        idx = np.random.randint(0, len(k_), len(check))
        coin = np.random.random(len(check))
        value[check] = np.where(p_[idx] > coin, k_[idx], a_[idx])
        k = used_key[check] + value[check]
        pos = np.searchsorted(allk, k)
        hit = (pos < len(allk)) & (allk[np.minimum(pos, len(allk) - 1)] == k)
        check = check[hit]
    smp.rs.set_state(np.random.get_state())
    return torch.from_numpy(value).to(DEV)


def training_cases():
    from fairrec.sampler import DeviceRandomState, Sampler
    for name, user_num, item_num, n_inter in (("ml-1m-sized", 6041, 3707, 1_000_209), ("configs[1] 1M x 100k", 1_000_001, 100_001, 10_000_000)):
        rng = np.random.default_rng(0)
        u = rng.integers(1, user_num, n_inter)
        w = 1.0 / np.arange(1, item_num) ** 0.8                        # a long-tailed popularity
        i = rng.choice(np.arange(1, item_num), n_inter, p=w / w.sum())
        rs = DeviceRandomState(DEV, 2020)
        t0 = time.perf_counter()
        pop = Sampler("train", _DS(user_num, item_num, u, i), "popularity", device=DEV, random_state=rs).set_phase("train")
        setup = time.perf_counter() - t0
        uni = Sampler("train", _DS(user_num, item_num, u, i), "uniform", device=DEV, random_state=rs).set_phase("train")
        pop._pop_host = tuple(t.cpu().numpy() for t in pop._pop)
        for B in (2048, 8192):
            keys = torch.from_numpy(rng.integers(1, user_num, B)).to(DEV)
            st = rs.get_state()
            a = pop.sample_by_user_ids(keys, None, 1)
            rs.set_state(st)
            b = host_path(pop, keys, 1)
            assert torch.equal(a, b)
            res = {"case": "training negatives", "shape": name, "pairs": int(pop.used_ids[0][-1].item()), "B": B, "num": 1,
                   "device_popularity": dev_timed(lambda: pop.sample_by_user_ids(keys, None, 1)),
                   "device_uniform": dev_timed(lambda: uni.sample_by_user_ids(keys, None, 1)),
                   "host_numpy_popularity": host_timed(lambda: host_path(pop, keys, 1)),
                   "alias_table_and_used_sets_build_s": round(setup, 2)}
            assert int(rs.err_flag.item()) == 0
            print(json.dumps(res), flush=True)


def eval_cases():
    import bench
    from fairrec.config import Config
    from fairrec.data.dataloader import NegSampleEvalDataLoader
    from fairrec.data.dataset import synthetic_dataset
    from fairrec.quick_start import split_dataset
    from fairrec.sampler import Sampler
    from fairrec.utils import get_model, get_trainer, init_seed
    import tempfile
    for mode in ("uni100", "pop100"):
        cfg = Config(model="FOCF", config_dict={
            "embedding_size": bench.DIM, "train_batch_size": bench.BATCH, "device": DEV, "epochs": 1, "fair_objective": "value",
            "fair_weight": 1.0, "weight_decay": 1e-3, "learning_rate": 1e-3, "checkpoint_dir": tempfile.mkdtemp(),
            "sst_attr_list": ["gender"], "eval_args": {"split": {"RS": [8, 1, 1]}, "group_by": "user", "order": "RO", "mode": mode},
            "metrics": ["NDCG", "Recall", "Hit", "MRR", "DifferentialFairness", "GiniIndex", "PopularityPercentage",
                        "ValueUnfairness", "AbsoluteUnfairness", "UnderUnfairness", "OverUnfairness", "NonParityUnfairness"],
            "valid_metric": "NDCG@5", "topk": [5], "popularity_ratio": 0.1, "eval_batch_size": 4096 * 101, "eval_step": 1})
        init_seed(bench.SEED)
        ds = synthetic_dataset(cfg, bench.N_USERS, bench.N_ITEMS, 2_000_000, seed=bench.SEED + 3)
        train_set, valid_set, test_set = split_dataset(ds)
        dist = "uniform" if mode == "uni100" else "popularity"
        phases = Sampler(["train", "valid", "test"], [train_set, valid_set, test_set], dist, device=DEV)
        valid = NegSampleEvalDataLoader(cfg, valid_set, phases.set_phase("valid"))
        model = get_model("FOCF")(cfg, train_set).to(DEV)
        trainer = get_trainer(None, "FOCF")(cfg, model)
        trainer._train_data_for_eval = types.SimpleNamespace(dataset=train_set)
        trainer.evaluate(valid)
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            trainer.evaluate(valid)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / len(valid) * 1e3)
        # the sampler's call sequence of the first batch alone
        uids, P = valid.uid_list[:valid.step], valid.counts[:valid.step]
        smp = valid.sampler
        calls = dev_timed(lambda: smp.sample_calls(uids, P * valid.neg_sample_num), reps=5)
        print(json.dumps({"case": "evaluation", "mode": mode, "batches": len(valid), "users_per_batch": valid.step,
                          "ms_per_batch": {"median": round(float(np.median(ts)), 3), "min": round(min(ts), 3),
                                           "max": round(max(ts), 3)},
                          "sampler_calls_first_batch_us": calls, "calls_per_batch": int(uids.numel())}), flush=True)
        del trainer, model, valid, phases
        torch.cuda.empty_cache()


if __name__ == "__main__":
    what = sys.argv[1:] or ["train", "eval"]
    if "train" in what:
        training_cases()
    if "eval" in what:
        eval_cases()

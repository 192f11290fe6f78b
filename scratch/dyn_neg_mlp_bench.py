"""Dynamic negative sampling for an MLP scorer: one batch's candidate scoring + pick, NFCF at 1 000 001 users x 100 001
items, D = 256, the yaml's `mlp_hidden_size` [128, 64], n = 8192 rows, num = 1, M candidates per slot, the item rows behind the
table's step as in scratch/dyn_neg_bench.py.  Three things per M:
  generic   repeat + predict + fr_dyn_neg_select: what `dynamic_neg_scorer: pairs` (the default) runs
  split     the model's dyn_neg_select hook: user lookup + P + fr_dyn_neg_mlp_select
  kernel    fr_dyn_neg_mlp_select alone on prepared pieces; its own time also from the library's event profiler, with its FLOP
            rate against the fp32 MFMA peak and the bytes it reads against HBM
Device events, 5 warm calls, then the median and min-max of 20, the variants alternating in one process.  `steps` as an
argument: also the NFCF training step (loader + step, wall clock per batch over whole epochs) without dynamic sampling and
with `dynamic: 4` under both key values.  Prints one JSON line per measurement."""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "recbole-fairrec_amd"), os.path.join(ROOT, "scratch")]
import torch

from recommend_bench import DEV, PEAK_TF, alternating

HBM_TBPS = 8.0
N_USERS, N_ITEMS, DIM, HIDDEN, N, STEPS = 1_000_001, 100_001, 256, [128, 64], 8192, 7


def build(neg_sampling, scorer, n_inter=400_000):
    from fairrec.config import Config
    from fairrec.data.dataloader import TrainDataLoader
    from fairrec.data.dataset import synthetic_dataset
    from fairrec.quick_start import split_dataset
    from fairrec.sampler import Sampler
    from fairrec.utils import get_model, get_trainer, init_seed
    cfg = Config(model="NFCF", config_dict={
        "embedding_size": DIM, "mlp_hidden_size": HIDDEN, "train_batch_size": N, "device": DEV, "epochs": 1,
        "checkpoint_dir": tempfile.mkdtemp(), "sst_attr_list": ["gender"], "load_pretrain_path": None, "LABEL_FIELD": "label",
        "neg_sampling": neg_sampling, "dynamic_neg_scorer": scorer})
    init_seed(2020)
    ds = synthetic_dataset(cfg, N_USERS, N_ITEMS, n_inter, seed=2023)
    tr, va, te = split_dataset(ds)
    sampler = Sampler(["train", "valid", "test"], [tr, va, te], "uniform", device=DEV).set_phase("train")
    dl = TrainDataLoader(cfg, tr.to(DEV), sampler=sampler, shuffle=True)
    model = get_model("NFCF")(cfg, dl.dataset).to(DEV)
    trainer = get_trainer(None, "NFCF")(cfg, model)
    dl.get_model(model)
    return dl, model, trainer


def age(table, g):
    """Rows left behind the step, as scratch/dyn_neg_bench.py leaves them."""
    table.ensure_state()
    table.m.normal_(0, 1e-2)
    table.v.uniform_(0, 1e-3)
    table.last.copy_(torch.randint(0, STEPS + 1, (table.n_rows,), generator=g, dtype=torch.int32).to(DEV))
    table.step = STEPS
    table._dirty = True
    return float((table.last < table.step).float().mean())


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
    work = _C.prof_read_work().get(name, 0.0)
    _C.prof_enable(False)
    return (ms * 1e3 / n, work / n) if n else (None, None)


def scoring(Ms):
    from fairrec.data.interaction import Interaction
    from fairrec.functional import dyn_neg_mlp_pieces, dyn_neg_mlp_select, dyn_neg_select
    dl, model, _ = build({"uniform": 1, "dynamic": 4}, "split")
    g = torch.Generator(device="cpu").manual_seed(0)
    eng = model.hip_engine()
    itab = eng._tables["item_embedding.weight"]
    behind = age(itab, g)
    hyper = eng._hyper("item_embedding.weight")
    uid = torch.randint(1, N_USERS, (N,), generator=g).to(DEV)
    inter = Interaction({dl.uid_field: uid, dl.iid_field: torch.randint(1, N_ITEMS, (N,), generator=g).to(DEV)})
    model.eval()
    for M in Ms:
        cand = torch.randint(1, N_ITEMS, (M * N,), generator=g).to(DEV)

        def generic():
            with torch.no_grad():
                rep = inter.repeat(M)
                rep.update(Interaction({dl.iid_field: cand}))
                return dyn_neg_select(model.predict(rep).reshape(M, -1), cand.view(M, -1))

        def split():
            with torch.no_grad():
                return model.dyn_neg_select(inter, cand, 1, M)

        with torch.no_grad():
            pieces = dyn_neg_mlp_pieces(model.mlp_layers, eng.lookup("user_embedding.weight", uid))

        def kernel():
            return dyn_neg_mlp_select(pieces, itab, hyper, cand, 1, M, eng.err_flag)

        a, b = generic(), split()
        res = {"case": "NFCF dynamic negatives, one batch", "n": N, "M": M, "D": DIM, "hidden": HIDDEN, "items": N_ITEMS,
               "rows_behind": round(behind, 3), "picks_equal_to_generic": round(float((a == b).float().mean()), 4)}
        res.update(alternating({"generic": generic, "split": split, "kernel": kernel}))
        kt, flop = kernel_time(kernel, "dyn_neg_mlp_kernel")
        if kt:
            n1 = HIDDEN[0]
            # per candidate: id 8, last 4, p D*4 (+ m, v for a row behind the step), its P row n1*4; the weights once per 32
            byts = M * N * (12 + DIM * 4 * (1 + 2 * behind) + n1 * 4 + (n1 * DIM * 4) / 32) + N * 8
            tf = flop / (kt * 1e-6) / 1e12
            res["dyn_neg_mlp_kernel"] = {"mean_us": round(kt, 1), "tflops": round(tf, 2), "share_of_fp32_mfma_peak": round(tf / PEAK_TF, 3),
                                         "bytes": int(byts), "TBps": round(byts / (kt * 1e-6) / 1e12, 3),
                                         "share_of_hbm": round(byts / (kt * 1e-6) / 1e12 / HBM_TBPS, 3)}
        print(json.dumps(res), flush=True)
    eng.check_device_errors()


def steps():
    for label, neg, scorer in (("plain", {"uniform": 1}, "pairs"), ("dynamic4_pairs", {"uniform": 1, "dynamic": 4}, "pairs"),
                               ("dynamic4_split", {"uniform": 1, "dynamic": 4}, "split")):
        dl, model, trainer = build(neg, scorer)
        trainer._train_epoch(dl, 0)                   # warm
        torch.cuda.synchronize()
        ts = []
        for e in range(3):
            t0 = time.perf_counter()
            trainer._train_epoch(dl, e + 1)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / len(dl) * 1e3)
        print(json.dumps({"case": "NFCF training step incl. loader, wall clock per batch", "variant": label, "batches": len(dl),
                          "train_batch_size": N, "ms_per_step_median": round(sorted(ts)[1], 4), "ms_min": round(min(ts), 4),
                          "ms_max": round(max(ts), 4)}), flush=True)
        del dl, model, trainer
        torch.cuda.empty_cache()


if __name__ == "__main__":
    args = sys.argv[1:]
    if "steps" in args:
        steps()
    else:
        scoring([int(x) for x in (args or ["2", "4", "8", "16"])])

"""bench.py's one-line JSON contract (task statement + ④): run a short bench on the GPU and check the fields the driver and
the judge read, in a plain run (the headline only) and with --full (every block).  Also the item-complete distribution (the
shape FOCFDataLoader produces) and the eager-only mode."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "12", "--warmup", "2", "--age", "8", *args],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]          # ONE JSON line
    return json.loads(lines[0])


def _bench(*args):
    return _line("--no-cpu-baseline", *args)


HEADLINE_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                 "vs_baseline", "dtype", "data", "config", "roofline")
FULL_ONLY_BLOCKS = ("other_batch_shapes", "trainer_fit", "next_rows", "other_workloads", "cpu_baseline", "nfcf100m")


def test_bench_plain_line():
    """Without --full (`bench.py --gpus 1 --steps K --warmup W`) the run ends at the headline: the same headline fields, and
    nothing that takes runs of its own -- no other launch modes, no per-kernel roofline, no other shapes or workloads, no
    CPU baseline."""
    d = _line("--gpus", "1")
    assert set(HEADLINE_KEYS) <= set(d) and not set(FULL_ONLY_BLOCKS) & set(d), sorted(d)
    assert d["metric"].startswith("training interactions/sec") and "FOCF emb=64" in d["metric"]
    assert d["n_gpus"] == 1 and d["steps"] == 12 and d["warmup"] == 2 and d["higher_is_better"] is True
    assert d["unit"] == "interactions/s" and d["dtype"] == "f32" and d["data"] == "synthetic" and d["vs_baseline"] is None
    assert d["ms_per_step"] > 0 and abs(d["value"] - 12 * 8192 / (d["ms_per_step"] * 12e-3)) <= 1e-3 * d["value"]
    assert d["roofline"] is None and d["config"]["launch_modes_timed"] is None
    assert d["config"]["launch"] == "hipGraph" and d["config"]["aged_steps"] == 8
    assert d["config"]["final_loss"] == d["config"]["final_loss"]      # not NaN


SMALL = ("--users", "200001", "--items", "50001", "--nfcf-users", "200001", "--nfcf-items", "50001")   # the other_workloads tables


@pytest.mark.parametrize("args", [SMALL, ("--item-dist", "grouped"), ("--no-graph", "--no-workloads"), ("--launch", "graph", "--no-workloads"),
                                  ("--launch", "library", "--no-workloads"), ("--launch", "library", "--item-dist", "grouped")],
                         ids=["default", "grouped", "eager", "graph", "library", "library_grouped"])
def test_bench_json_contract(args):
    d = _bench("--full", *args)
    for k in HEADLINE_KEYS:
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 12 and d["warmup"] == 2 and d["higher_is_better"] is True
    assert d["unit"] == "interactions/s" and d["dtype"] == "f32" and d["data"] == "synthetic" and d["vs_baseline"] is None
    assert "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - 12 * 8192 / (d["ms_per_step"] * 12e-3)) <= 1e-3 * d["value"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and 0.0 < r["frac"] < 1.0
    assert d["config"]["final_loss"] == d["config"]["final_loss"]      # not NaN
    if "--item-dist" not in args:
        # the item-complete shape FOCF's real loader produces is reported next to the figure of record,
        # under the unique-row bytes definition it names
        shapes = {x["item_distribution"]: x for x in d["other_batch_shapes"]}
        assert set(shapes) == {"grouped", "zipf"}
        g = shapes["grouped"]
        assert "unique rows" in g["bytes_definition"] and g["us_per_step"] > 0 and "fr_focf_step_runs" in g["step"]
        assert 60 < g["distinct_item_rows_per_batch"] < 100 and g["bytes_per_interaction"] < 3096
        assert abs(g["frac_of_hbm_peak"] - g["achieved_GBps"] / 8000.0) < 1e-3 and g["hipGraph_us_per_step"] > 0
    else:
        assert "other_batch_shapes" not in d
    # --launch auto (the default): 12 timed steps are one hipGraph replay (the library's step loop from 64 steps on), and the
    # line says so
    if "--no-graph" in args:
        mode = "eager"
    elif "--launch" in args:
        mode = {"graph": "hipGraph", "library": "library step loop"}[args[args.index("--launch") + 1]]
    else:
        mode = "hipGraph"
        assert "auto" in d["config"]["launch_note"]
    assert d["config"]["launch"].startswith(mode), d["config"]["launch"]
    if args is SMALL:
        # BASELINE.json configs[2..4] ride in the --full line (here on small tables): ms per step, rate, roofline of each
        modes = d["config"]["launch_modes_timed"]
        assert {"library_loop_ms_per_step", "hipGraph_ms_per_step", "eager_ms_per_step"} <= set(modes)
        assert abs(modes["hipGraph_ms_per_step"] - d["ms_per_step"]) < 1e-4
        w = d["other_workloads"]
        assert set(w) == {"pfcn10m", "nfcf100m", "fairgo10m"}
        for name, x in w.items():
            assert "skipped_reason" not in x, (name, x)
            assert x["steps"] >= 5 and x["ms_per_step"] > 0 and x["interactions_per_s"] > 0, (name, x)
            assert x["roofline"]["bound"] in ("hbm", "mfma", "valu (exact replay)") and 0.0 < x["roofline"]["frac"] < 1.0, (name, x)
            assert abs(x["interactions_per_s"] - 8192 / (x["ms_per_step"] * 1e-3)) <= 2e-3 * x["interactions_per_s"], (name, x)
    else:
        assert "other_workloads" not in d


def _eager_reference(item_dist, age=8, W=2, K=12):
    """bench.py's batches (same seeds, same counts) stepped by a fresh engine on the three-launch chain (fr_focf_forward +
    fr_focf_backward_adam, no deferred loss, no look-ahead): an independent path to what `--dump-outputs` reports.  Returns the
    (loss, mse, fair) of every step, the flushed tables and the user ids of the last timed batch."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    import torch
    from fairrec.model.fair_recommender.focf import FocfEngine
    from fairrec.optim import FusedLazyAdam
    dev = torch.device("cuda")
    pipe = FocfEngine.LOW_WATER + FocfEngine.GROUP + 4          # one GPU: bench.py draws K + W + PIPE batches
    aged = bench.synth_batches(age, bench.BATCH, bench.N_USERS, bench.N_ITEMS, bench.SEED + 104729, item_dist)
    timed = bench.synth_batches(K + W + pipe, bench.BATCH, bench.N_USERS, bench.N_ITEMS, bench.SEED, item_dist)
    U, I = bench.xavier_tables(bench.N_USERS, bench.N_ITEMS, bench.DIM, bench.SEED, dev)
    eng = FocfEngine(U, I, bench.OBJECTIVE, bench.FAIR_WEIGHT, 5.0)
    FusedLazyAdam(eng, lr=bench.LR, weight_decay=bench.WD)
    losses = []
    for cols, n in ((aged, age), (timed, W + K)):
        u, i, r, s = (t.to(dev) for t in cols)
        for k in range(n):
            loss, _ = eng.forward(u[k], i[k], r[k], s[k])
            losses.append(loss[:3].clone())
            eng.backward_adam()
    eng.flush()
    eng.check_device_errors()
    return (torch.stack(losses).double().cpu().numpy(), eng.U.weight.cpu().numpy(), eng.I.weight.cpu().numpy(),
            timed[0][W + K - 1].numpy())


DUMP_FILES = ["item_embedding.npy", "loss_last_step.npy", "loss_running_total.npy", "user_embedding_row_ids.npy",
              "user_embedding_rows.npy"]


def _load_dump(path):
    import numpy as np
    files = sorted(os.listdir(path))
    assert files == DUMP_FILES, files
    assert sum(os.path.getsize(os.path.join(path, f)) for f in files) <= 64 << 20
    z = {f[:-4]: np.load(os.path.join(path, f)) for f in files}
    for name, a in z.items():
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), name
    return z


@pytest.mark.parametrize("args", [("--launch", "graph"), ("--launch", "library"), ("--launch", "library", "--item-dist", "grouped")],
                         ids=["graph", "library", "library_grouped"])
def test_bench_dump_outputs(tmp_path, args):
    """`--dump-outputs DIR`: what the timed steps computed up to and including the last one, as float32 / float64 .npy files
    under 64 MB in all, checked against an eager re-run of the same batches on another launch path: the last step's loss
    terms, the running total over all 8 + 2 + 12 steps, the whole item table and the dumped user rows (the last batch's
    among them).  Two runs with the same arguments feed the same inputs, so their dumps agree."""
    import numpy as np
    import bench
    d = _bench("--no-shapes", "--graph-only", "--dump-outputs", str(tmp_path / "a"), *args)
    assert d["steps"] == 12 and d["ms_per_step"] > 0
    z = _load_dump(tmp_path / "a")
    ref_loss, ref_U, ref_I, last_users = _eager_reference("grouped" if "grouped" in args else "uniform")
    assert ref_loss.shape == (22, 3)
    tot = z["loss_running_total"]
    assert tot[3] == 22 and tot[4] == 0, tot                         # every step counted, none NaN
    last = z["loss_last_step"]
    assert last.shape == (3,) and last[0] > 1.0 and last[1] > 1.0, last
    np.testing.assert_allclose(last, ref_loss[-1], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(tot[:3], ref_loss.sum(0), rtol=1e-4, atol=1e-5)
    assert abs(float(last[0]) - d["config"]["final_loss"]) <= 1e-6    # (the line rounds it to 6 places)
    ids = z["user_embedding_row_ids"]
    assert (np.diff(ids) > 0).all() and ids.size >= 65536 and z["user_embedding_rows"].shape == (ids.size, 64)
    assert np.isin(last_users, ids).all()
    # (rows no batch touches wobble around zero by Adam steps of ~1e-7: another launch path moves them by a fraction of one)
    tol = 2e-3 * bench.LR
    assert z["item_embedding"].shape == ref_I.shape
    assert float(np.abs(z["item_embedding"] - ref_I).max()) <= tol
    assert float(np.abs(z["user_embedding_rows"] - ref_U[ids.astype(np.int64)]).max()) <= tol
    if args[1] == "graph":
        _bench("--no-shapes", "--graph-only", "--dump-outputs", str(tmp_path / "b"), *args)
        b = _load_dump(tmp_path / "b")
        for name in z:
            np.testing.assert_allclose(z[name], b[name], rtol=1e-4, atol=1e-6 * float(np.abs(b[name]).max()) + 1e-12,
                                       err_msg=name)


def test_bench_nfcf_workload_contract():
    """`--workload nfcf100m` (BASELINE.json configs[4]) at a reduced table size: same JSON contract, NFCF finetune step."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "nfcf100m", "--nfcf-users", "200001",
                          "--nfcf-items", "50001", "--steps", "6", "--warmup", "2"], capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["steps"] == 6 and d["unit"] == "interactions/s" and d["value"] > 0
    assert "NFCF finetune" in d["config"]["workload"] and d["roofline"]["algorithmic_bytes_per_launch"] == 7192 * 8192
    assert d["config"]["final_loss"] == d["config"]["final_loss"]

"""Dynamic negative sampling at configs[2]-like sizes (n = 8192 rows, D = 128, 1 M items): one batch's candidate scoring +
pick, composed path (fr_table_gather + RowDot + biases + torch.sigmoid + fr_dyn_neg_select, what predict() on the repeated
interaction costs for PFCN_BiasedMF with the user side on n*M rows) against fr_dyn_neg_dot_select, on device events over
warm repeated calls.  Prints one JSON line per M."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "recbole-fairrec_amd")]
import torch

from fairrec.functional import RowDot, dyn_neg_dot_select, dyn_neg_select
from fairrec.optim import AdamHyper, LazyTable

DEV = "cuda"
n, D, N_ITEMS, STEPS = 8192, 128, 1 << 20, 7


def table(dim, g):
    t = LazyTable((torch.randn(N_ITEMS, dim, generator=g) * 0.1).to(DEV))
    t.ensure_state()
    t.m.normal_(0, 1e-2)
    t.v.uniform_(0, 1e-3)
    t.last.copy_(torch.randint(0, STEPS + 1, (N_ITEMS,), generator=g, dtype=torch.int32).to(DEV))
    t.step = STEPS
    return t


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    g = torch.Generator(device="cpu").manual_seed(0)
    hyper = AdamHyper(lr=1e-3, device=DEV)
    it, bt = table(D, g), table(1, g)
    uids = torch.randint(1, N_ITEMS, (n,), generator=g).to(DEV)
    ut, ubt = table(D, g), table(1, g)
    gb = torch.tensor(0.1, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    behind = float((it.last < it.step).float().mean())
    for M in [int(x) for x in (sys.argv[1:] or ["2", "4", "8", "16"])]:
        cand = torch.randint(1, N_ITEMS, (M * n,), generator=g).to(DEV)

        def composed():
            u_rep = uids.repeat(M)
            ue = ut.gather(hyper, u_rep, err)
            rows = it.gather(hyper, cand, err)
            s = RowDot.apply(ue, rows).unsqueeze(-1)
            s = s + ubt.gather(hyper, u_rep, err) + bt.gather(hyper, cand, err) + gb
            return dyn_neg_select(torch.sigmoid(s).reshape(M, -1), cand.view(M, -1))

        def fused():
            ue = ut.gather(hyper, uids, err)
            return dyn_neg_dot_select(it, hyper, ue, cand, 1, M, err, item_bias=(bt, hyper),
                                      user_bias=ubt.gather(hyper, uids, err), global_bias=gb)

        def kernel_only(ue=ut.gather(hyper, uids, err), ub=ubt.gather(hyper, uids, err)):
            return dyn_neg_dot_select(it, hyper, ue, cand, 1, M, err, item_bias=(bt, hyper), user_bias=ub, global_bias=gb)

        assert torch.equal(composed(), fused())
        tc, tf, tk = timed(composed), timed(fused), timed(kernel_only)
        # bytes the fused kernel reads per candidate: id 8 + last 4 (+ bias last 4) + p D*4 + bias p 4, and m, v (D*4 each,
        # bias 4 each) for a row that is behind the table's step
        per = 8 + 4 + 4 + D * 4 + 4 + behind * (2 * D * 4 + 8)
        byts = M * n * per + n * (D * 4 + 4) + n * 8
        print(json.dumps({"M": M, "n": n, "D": D, "items": N_ITEMS, "rows_behind": round(behind, 3),
                          "composed_ms": round(tc, 4), "fused_ms": round(tf, 4), "fused_kernel_ms": round(tk, 4),
                          "speedup": round(tc / tf, 2), "kernel_bytes": int(byts),
                          "kernel_TBps": round(byts / tk / 1e9, 3)}), flush=True)
    assert int(err.item()) == 0


if __name__ == "__main__":
    main()

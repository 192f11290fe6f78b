"""Autograd bridges over the HIP scoring / loss kernels (csrc/pfcn.hip, csrc/nfcf.hip): each Function's forward and
backward are single kernel launches through the C ABI; torch only chains them."""
from __future__ import annotations

import ctypes

import torch

from . import _C


def _ws(nbytes, dev):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)


class SplitRows(torch.autograd.Function):
    """(x[:n], x[n:]) of rows that ONE lookup gathered for two id lists.  Autograd's own slices give each half a backward of
    its own -- a zero-filled [2B, D] buffer, a copy into it, and an add of the two buffers: five launches where the gradient
    is simply the two halves side by side (one `cat`; the same values, x + 0 = x)."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.n, ctx.shape = int(n), x.shape
        return x[:n], x[n:]

    @staticmethod
    def backward(ctx, ga, gb):
        if ga is None and gb is None:
            return None, None
        ref = ga if ga is not None else gb
        if ga is None:
            ga = ref.new_zeros((ctx.n,) + tuple(ctx.shape[1:]))
        if gb is None:
            gb = ref.new_zeros((ctx.shape[0] - ctx.n,) + tuple(ctx.shape[1:]))
        return torch.cat([ga, gb]), None


class RowDot(torch.autograd.Function):
    """torch.mul(a, b).sum(-1) (pfcn_pmf.py:182-183)."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = a.contiguous(), b.contiguous()
        out = torch.empty(a.shape[0], dtype=torch.float32, device=a.device)
        _C.check(_C.lib().fr_rowdot_fwd(a.data_ptr(), b.data_ptr(), a.shape[0], a.shape[1], out.data_ptr(),
                                        _C.current_stream()), "fr_rowdot_fwd")
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous()
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        if da is not None or db is not None:
            _C.check(_C.lib().fr_rowdot_bwd(g.data_ptr(), a.data_ptr(), b.data_ptr(), a.shape[0], a.shape[1], _C.ptr(da),
                                            _C.ptr(db), _C.current_stream()), "fr_rowdot_bwd")
        return da, db


class RowDotRep(torch.autograd.Function):
    """RowDot with the rows of `a` [A, D] reused by the R = b.shape[0] / A row blocks of `b`: out[r*A + i] = a[i] . b[r*A + i]
    (a user row against its positive and its negative item row, which one lookup gathered as [2B, D])."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = a.contiguous(), b.contiguous()
        A, D = a.shape
        reps = b.shape[0] // A
        assert b.shape[0] == reps * A and b.shape[1] == D
        out = torch.empty(b.shape[0], dtype=torch.float32, device=a.device)
        _C.check(_C.lib().fr_rowdot_rep_fwd(a.data_ptr(), b.data_ptr(), A, reps, D, out.data_ptr(), _C.current_stream()),
                 "fr_rowdot_rep_fwd")
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous()
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        if da is not None or db is not None:
            _C.check(_C.lib().fr_rowdot_rep_bwd(g.data_ptr(), a.data_ptr(), b.data_ptr(), a.shape[0], b.shape[0] // a.shape[0],
                                                a.shape[1], _C.ptr(da), _C.ptr(db), _C.current_stream()), "fr_rowdot_rep_bwd")
        return da, db


class RowDotPair(torch.autograd.Function):
    """cat(RowDot(a, b[:A]), RowDot(a, b[A:])) for the rows `b` [2A, D] that one lookup gathered for a positive and a negative
    id list: ONE forward launch (fr_rowdot_rep_fwd) instead of two and a `cat`, ONE backward launch (fr_rowdot_rep_bwd_sep: the
    products RowDot's two backward launches form, the gradient of `b` whole instead of two halves glued by autograd).  `a` is
    passed TWICE -- `RowDotPair.apply(a, a, b)` -- so that its two gradients reach autograd unsummed and are added to
    whatever else `a` feeds in the order the two RowDot nodes gave them (the negative's first: the later node runs first);
    summing them here would round once differently (the d128 golden)."""

    @staticmethod
    def forward(ctx, a_neg, a_pos, b):
        a, b = a_pos.contiguous(), b.contiguous()
        A, D = a.shape
        assert a_neg.data_ptr() == a_pos.data_ptr() and b.shape[0] == 2 * A and b.shape[1] == D
        out = torch.empty(2 * A, dtype=torch.float32, device=a.device)
        _C.check(_C.lib().fr_rowdot_rep_fwd(a.data_ptr(), b.data_ptr(), A, 2, D, out.data_ptr(), _C.current_stream()),
                 "fr_rowdot_rep_fwd")
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous()
        A, D = a.shape
        want_a = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        da = torch.empty_like(b) if want_a else None        # [pos part; neg part], unsummed
        db = torch.empty_like(b) if ctx.needs_input_grad[2] else None
        if da is not None or db is not None:
            _C.check(_C.lib().fr_rowdot_rep_bwd_sep(g.data_ptr(), a.data_ptr(), b.data_ptr(), A, 2, D, _C.ptr(da), _C.ptr(db),
                                                    _C.current_stream()), "fr_rowdot_rep_bwd_sep")
        da_neg = da[A:] if ctx.needs_input_grad[0] else None
        da_pos = da[:A] if ctx.needs_input_grad[1] else None
        return da_neg, da_pos, db


class SubScaled(torch.autograd.Function):
    """a - alpha * b of two scalar losses: torch.sub's backward negates and scales in two launches; here one."""

    @staticmethod
    def forward(ctx, a, b, alpha):
        ctx.alpha = float(alpha)
        return torch.sub(a, b, alpha=alpha)

    @staticmethod
    def backward(ctx, g):
        return (g if ctx.needs_input_grad[0] else None), (g * (-ctx.alpha) if ctx.needs_input_grad[1] else None), None


class Bpr(torch.autograd.Function):
    """BPRLoss(pos, neg), loss.py:45-47."""

    @staticmethod
    def forward(ctx, pos, neg):
        pos, neg = pos.contiguous(), neg.contiguous()
        B, dev = pos.numel(), pos.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        dpos, dneg = torch.empty_like(pos), torch.empty_like(neg)
        ws = _ws(_C.lib().fr_bpr_workspace_bytes(B, 0), dev)
        _C.check(_C.lib().fr_bpr(pos.data_ptr(), neg.data_ptr(), B, loss.data_ptr(), dpos.data_ptr(), dneg.data_ptr(),
                                 ws.data_ptr(), ws.numel(), _C.current_stream()), "fr_bpr")
        ctx.save_for_backward(dpos, dneg)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        dpos, dneg = ctx.saved_tensors
        if _C.is_one(g):            # GraphedStep's backward seed: nothing to scale by
            return dpos, dneg
        return dpos * g, dneg * g


class BprBroadcast(torch.autograd.Function):
    """PFCN_BiasedMF's training loss (pfcn_biasedmf.py:192-195): pos/neg scores are `[B] + [B,1]` sums, i.e. a [B,B]
    matrix x_ij = (dp_j - dn_j) + (bpi_i - bni_i); user_bias and global_bias cancel but stay in the graph with an
    exactly-zero gradient, as in the reference (so their optimizer state still steps)."""

    @staticmethod
    def forward(ctx, dp, dn, user_bias, pos_bias, neg_bias, global_bias):
        a = (dp - dn).contiguous()
        c = (pos_bias - neg_bias).reshape(-1).contiguous()
        B, dev = a.numel(), a.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        da, dc = torch.empty_like(a), torch.empty_like(c)
        ws = _ws(_C.lib().fr_bpr_workspace_bytes(B, 1), dev)
        _C.check(_C.lib().fr_bpr_outer(a.data_ptr(), c.data_ptr(), B, loss.data_ptr(), da.data_ptr(), dc.data_ptr(),
                                       ws.data_ptr(), ws.numel(), _C.current_stream()), "fr_bpr_outer")
        ctx.save_for_backward(da, dc)
        ctx.shapes = (user_bias.shape, pos_bias.shape, global_bias.shape)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        da, dc = ctx.saved_tensors
        ub, pb, gb = ctx.shapes
        dev = da.device
        return (da * g, -da * g, torch.zeros(ub, device=dev), (dc * g).reshape(pb), (-dc * g).reshape(pb),
                torch.zeros(gb, device=dev))


class BprBroadcastPacked(torch.autograd.Function):
    """BprBroadcast on packed columns: `scores` = [pos | neg] ([2B], RowDotRep's output), `item_bias` = the [2B, 1] lookup of
    [pos items | neg items].  The differences are formed in the kernel and the four gradient columns come out of it, so the
    loss costs no elementwise launches (the unpacked form: 2 subtractions before, 6 products / negations and 2 slice
    gradients after)."""

    @staticmethod
    def forward(ctx, scores, user_bias, item_bias, global_bias):
        scores = scores.contiguous()
        ib = item_bias.contiguous()
        B, dev = scores.numel() // 2, scores.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        ds = torch.empty_like(scores)
        dib = torch.empty(2 * B, dtype=torch.float32, device=dev)
        ws = _ws(_C.lib().fr_bpr_workspace_bytes(B, 1), dev)
        sp, bp = scores.data_ptr(), ib.data_ptr()
        _C.check(_C.lib().fr_bpr_outer2(sp, sp + 4 * B, bp, bp + 4 * B, B, loss.data_ptr(), ds.data_ptr(), ds.data_ptr() + 4 * B,
                                        dib.data_ptr(), dib.data_ptr() + 4 * B, ws.data_ptr(), ws.numel(),
                                        _C.current_stream()), "fr_bpr_outer2")
        ctx.save_for_backward(ds, dib)
        ctx.shapes = (user_bias.shape, item_bias.shape, global_bias.shape)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        ds, dib = ctx.saved_tensors
        ub, ibs, gb = ctx.shapes
        dev = ds.device
        if not _C.is_one(g):
            ds, dib = ds * g, dib * g
        return ds, _C.zeros_cached(ub, dev), dib.reshape(ibs), _C.zeros_cached(gb, dev)


class BprBroadcastGlobal(torch.autograd.Function):
    """BprBroadcastPacked on row-sharded tables: the [B] + [B, 1] broadcast runs over the GLOBAL batch (every rank's rows and
    columns: ShardedGenericEngine.global_bpr_broadcast), so a G-rank step is the single-device step on the concatenated
    batch."""

    @staticmethod
    def forward(ctx, scores, user_bias, item_bias, global_bias, engine):
        B = scores.numel() // 2
        ib = item_bias.reshape(-1)
        a = (scores[:B] - scores[B:]).contiguous()
        c = (ib[:B] - ib[B:]).contiguous()
        loss, da, dc = engine.global_bpr_broadcast(a, c)
        ctx.save_for_backward(da, dc)
        ctx.shapes = (user_bias.shape, item_bias.shape, global_bias.shape)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        da, dc = ctx.saved_tensors
        ub, ibs, gb = ctx.shapes
        dev = da.device
        if not _C.is_one(g):
            da, dc = da * g, dc * g
        return (torch.cat([da, -da]), torch.zeros(ub, device=dev), torch.cat([dc, -dc]).reshape(ibs), torch.zeros(gb, device=dev),
                None)


class SigmoidBce(torch.autograd.Function):
    """nn.BCELoss()(sigmoid(y), label) (pfcn_biasedmf.py:212-213) -- the BCE leg of fr_nfcf_loss."""

    @staticmethod
    def forward(ctx, y, label):
        lib = _C.lib()
        shape = y.shape
        y = y.contiguous().view(-1)
        label = label.contiguous().view(-1).to(torch.float32)
        B, dev = y.numel(), y.device
        out = torch.empty(B, dtype=torch.float32, device=dev)
        dy = torch.empty(B, dtype=torch.float32, device=dev)
        loss = torch.empty(3, dtype=torch.float32, device=dev)
        ws = _ws(lib.fr_nfcf_loss_workspace_bytes(B), dev)
        _C.check(lib.fr_nfcf_loss(y.data_ptr(), label.data_ptr(), None, B, 0.0, None, 0, 1, out.data_ptr(), dy.data_ptr(),
                                  loss.data_ptr(), ws.data_ptr(), ws.numel(), None, _C.current_stream()), "fr_nfcf_loss")
        ctx.save_for_backward(dy)
        ctx.shape = shape
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dy,) = ctx.saved_tensors
        return (dy if _C.is_one(g) else dy * g).view(ctx.shape), None


class SoftmaxCe(torch.autograd.Function):
    """nn.CrossEntropyLoss()(logits, label) (pfcn_biasedmf.py:216)."""

    @staticmethod
    def forward(ctx, logits, label, err_flag):
        logits = logits.contiguous()
        label = label.contiguous().to(torch.int64)
        M, C = logits.shape
        dev = logits.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        dl = torch.empty_like(logits)
        ws = _ws(((M + 255) // 256) * 4, dev)
        _C.check(_C.lib().fr_softmax_ce(logits.data_ptr(), label.data_ptr(), M, C, loss.data_ptr(), dl.data_ptr(),
                                        ws.data_ptr(), ws.numel(), _C.ptr(err_flag), _C.current_stream()), "fr_softmax_ce")
        ctx.save_for_backward(dl)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return (dl if _C.is_one(g) else dl * g), None, None


class Mse(torch.autograd.Function):
    """nn.MSELoss()(pred, target) (fairgo_pmf.py:182)."""

    @staticmethod
    def forward(ctx, pred, target):
        pred, target = pred.contiguous(), target.contiguous().to(torch.float32)
        B, dev = pred.numel(), pred.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        dp = torch.empty_like(pred)
        ws = _ws(((B + 255) // 256) * 4, dev)
        _C.check(_C.lib().fr_mse(pred.data_ptr(), target.data_ptr(), B, loss.data_ptr(), dp.data_ptr(), ws.data_ptr(),
                                 ws.numel(), _C.current_stream()), "fr_mse")
        ctx.save_for_backward(dp)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dp,) = ctx.saved_tensors
        return (dp if _C.is_one(g) else dp * g), None


class CsrMatrix:
    """A sparse matrix and its transpose as device CSR arrays (indptr int64, col int32, val fp32)."""

    def __init__(self, scipy_csr, device):
        import numpy as np
        self.shape = scipy_csr.shape
        self.fwd = self._pack(scipy_csr, device)
        self.bwd = self._pack(scipy_csr.transpose().tocsr(), device)

    @staticmethod
    def _pack(m, device):
        import numpy as np
        m.sort_indices()
        return (torch.from_numpy(m.indptr.astype(np.int64)).to(device), torch.from_numpy(m.indices.astype(np.int32)).to(device),
                torch.from_numpy(m.data.astype(np.float32)).to(device))


class SpMM(torch.autograd.Function):
    """Y = L X (torch.sparse.mm, fairgo_pmf.py:198); backward dX = L^T dY with the pre-built transpose."""

    @staticmethod
    def forward(ctx, X, L: CsrMatrix):
        X = X.contiguous()
        Y = torch.empty((L.shape[0], X.shape[1]), dtype=torch.float32, device=X.device)
        ip, col, val = L.fwd
        _C.check(_C.lib().fr_spmm_csr(ip.data_ptr(), col.data_ptr(), val.data_ptr(), X.data_ptr(), L.shape[0], X.shape[1],
                                      Y.data_ptr(), _C.current_stream()), "fr_spmm_csr")
        ctx.L = L
        return Y

    @staticmethod
    def backward(ctx, dY):
        L = ctx.L
        dY = dY.contiguous()
        dX = torch.empty((L.shape[1], dY.shape[1]), dtype=torch.float32, device=dY.device)
        ip, col, val = L.bwd
        _C.check(_C.lib().fr_spmm_csr(ip.data_ptr(), col.data_ptr(), val.data_ptr(), dY.data_ptr(), L.shape[1], dY.shape[1],
                                      dX.data_ptr(), _C.current_stream()), "fr_spmm_csr")
        return dX, None


class SpMMSel(torch.autograd.Function):
    """Rows of Y = L X where the batch can see them (fr_spmm_csr_sel): Y[i] = sum_j L[rows[i], j] * X[xmap[j]] with the
    nonzeros in CSR order and nonzeros whose `xmap` entry is -1 skipped.  `rows` / `rpos` (int32 [R] / its inverse map over
    the rows of L, -1 elsewhere) select the output rows; `xrows` / `xmap` (int32 [n_x] / inverse over the columns) say which
    columns the rows of a COMPACT X stand for; either pair may be None (all rows / X is the whole table).  The backward is the
    same kernel on the CSR of L^T with the two pairs swapped.  Kept terms are added in SpMM's order and skipped terms are the
    ones SpMM adds as exact zeros, so values and gradients are those of the whole-table product restricted to the rows."""

    @staticmethod
    def forward(ctx, X, L: CsrMatrix, rows, rpos, xrows, xmap, rbits=None, xbits=None):
        """`rbits` / `xbits`: the bitmaps of `rpos` / `xmap` (bit c set where the map is >= 0; fr_spmm_csr_sel)."""
        X = X.contiguous()
        n_out = L.shape[0] if rows is None else rows.numel()
        Y = torch.empty((n_out, X.shape[1]), dtype=torch.float32, device=X.device)
        ip, col, val = L.fwd
        _C.check(_C.lib().fr_spmm_csr_sel(ip.data_ptr(), col.data_ptr(), val.data_ptr(), X.data_ptr(), _C.ptr(rows), n_out,
                                          _C.ptr(xmap), _C.ptr(xbits), X.shape[1], Y.data_ptr(), _C.current_stream()),
                 "fr_spmm_csr_sel")
        ctx.L, ctx.sel, ctx.n_x = L, (rows, rpos, xrows, xmap, rbits), X.shape[0]
        return Y

    @staticmethod
    def backward(ctx, dY):
        L = ctx.L
        rows, rpos, xrows, xmap, rbits = ctx.sel
        dY = dY.contiguous()
        dX = torch.empty((ctx.n_x, dY.shape[1]), dtype=torch.float32, device=dY.device)
        ip, col, val = L.bwd
        _C.check(_C.lib().fr_spmm_csr_sel(ip.data_ptr(), col.data_ptr(), val.data_ptr(), dY.data_ptr(), _C.ptr(xrows), ctx.n_x,
                                          _C.ptr(rpos), _C.ptr(rbits), dY.shape[1], dX.data_ptr(), _C.current_stream()),
                 "fr_spmm_csr_sel")
        return dX, None, None, None, None, None, None, None


class GatherAndSpMMSel(torch.autograd.Function):
    """(X[idx], SpMMSel(X, L, rows, rpos)) of ONE whole-table operand as one autograd node: the two uses of X meet in the
    backward as ONE dense [N, D] gradient -- fr_spmm_csr_sel writes it (every row: zeros where the batch sees nothing), then
    fr_row_scatter_add adds the gathered rows' gradients, duplicates summed in ascending position -- where two nodes cost a
    zero fill, a second dense tensor and autograd's addition of the two (three more whole-table passes).  The same two
    addends per element: the same bits."""

    @staticmethod
    def forward(ctx, X, idx, err_flag, L: CsrMatrix, rows, rpos, rbits=None, act=0):
        """`act` != 0: X is the output of that activation (an MLP built with `grad_at_z=True`) and the backward returns the
        gradient at the activation's INPUT -- (L^T dY + scatter(g_rows)) o act'(X) -- from the same two launches
        (fr_spmm_csr_sel_act / fr_row_scatter_add_act) instead of a third whole-table pass in the MLP's backward."""
        X = X.contiguous()
        idx = idx.contiguous().to(torch.int64)
        M, (N, D) = idx.numel(), X.shape
        out = torch.empty((M, D), dtype=torch.float32, device=X.device)
        _C.check(_C.lib().fr_row_gather(X.data_ptr(), idx.data_ptr(), M, N, D, out.data_ptr(), _C.ptr(err_flag),
                                        _C.current_stream()), "fr_row_gather")
        Y = torch.empty((rows.numel(), D), dtype=torch.float32, device=X.device)
        ip, col, val = L.fwd
        _C.check(_C.lib().fr_spmm_csr_sel(ip.data_ptr(), col.data_ptr(), val.data_ptr(), X.data_ptr(), rows.data_ptr(),
                                          rows.numel(), None, None, D, Y.data_ptr(), _C.current_stream()), "fr_spmm_csr_sel")
        if act:
            ctx.save_for_backward(idx, X)
        else:
            ctx.save_for_backward(idx)
        ctx.meta = (N, D, err_flag, L, rpos, rbits, int(act))
        return out, Y

    @staticmethod
    def backward(ctx, g_rows, dY):
        idx = ctx.saved_tensors[0]
        N, D, err, L, rpos, rbits, act = ctx.meta
        lib, st = _C.lib(), _C.current_stream()
        dX = torch.empty((N, D), dtype=torch.float32, device=idx.device)
        ip, col, val = L.bwd
        if act and (dY is None or g_rows is None):      # (not FairGo's step: both uses carry a gradient there)
            raise _C.FairrecError("GatherAndSpMMSel(act=...): both outputs must receive a gradient")
        if act:
            X = ctx.saved_tensors[1]
            M = idx.numel()
            # the rows the scatter adds to are scaled by IT, after the addition: a bitmap of them for the product to leave alone
            skip = torch.zeros((N + 31) // 32, dtype=torch.int32, device=idx.device)
            _C.check(lib.fr_frontier_mark(idx.data_ptr(), M, N, skip.data_ptr(), _C.ptr(err), st), "fr_frontier_mark")
            dY = dY.contiguous()
            _C.check(lib.fr_spmm_csr_sel_act(ip.data_ptr(), col.data_ptr(), val.data_ptr(), dY.data_ptr(), None, N, rpos.data_ptr(),
                                             _C.ptr(rbits), D, dX.data_ptr(), X.data_ptr(), act, skip.data_ptr(), st),
                     "fr_spmm_csr_sel_act")
            g_rows = g_rows.contiguous()
            ws = _ws(lib.fr_row_scatter_workspace_bytes(M), dX.device)
            _C.check(lib.fr_row_scatter_add_act(g_rows.data_ptr(), idx.data_ptr(), M, N, D, dX.data_ptr(), ws.data_ptr(), ws.numel(),
                                                X.data_ptr(), act, _C.ptr(err), st), "fr_row_scatter_add_act")
            return dX, None, None, None, None, None, None, None
        if dY is None:
            dX.zero_()
        else:
            dY = dY.contiguous()
            _C.check(lib.fr_spmm_csr_sel(ip.data_ptr(), col.data_ptr(), val.data_ptr(), dY.data_ptr(), None, N,
                                         rpos.data_ptr(), _C.ptr(rbits), D, dX.data_ptr(), st), "fr_spmm_csr_sel")
        if g_rows is not None:
            g_rows = g_rows.contiguous()
            M = idx.numel()
            ws = _ws(lib.fr_row_scatter_workspace_bytes(M), dX.device)
            _C.check(lib.fr_row_scatter_add(g_rows.data_ptr(), idx.data_ptr(), M, N, D, dX.data_ptr(), ws.data_ptr(),
                                            ws.numel(), _C.ptr(err), st), "fr_row_scatter_add")
        return dX, None, None, None, None, None, None, None


class RowGather(torch.autograd.Function):
    """X[idx] on a whole-table activation (fairgo_pmf.py:178-179); backward = dense gradient with duplicates summed in
    ascending batch position (fixed order, no atomics)."""

    @staticmethod
    def forward(ctx, X, idx, err_flag):
        X = X.contiguous()
        idx = idx.contiguous().to(torch.int64)
        M, (N, D) = idx.numel(), X.shape
        out = torch.empty((M, D), dtype=torch.float32, device=X.device)
        _C.check(_C.lib().fr_row_gather(X.data_ptr(), idx.data_ptr(), M, N, D, out.data_ptr(), _C.ptr(err_flag),
                                        _C.current_stream()), "fr_row_gather")
        ctx.save_for_backward(idx)
        ctx.shape, ctx.err = (N, D), err_flag
        return out

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        N, D = ctx.shape
        g = g.contiguous()
        M = idx.numel()
        dX = torch.empty((N, D), dtype=torch.float32, device=g.device)
        ws = _ws(_C.lib().fr_row_scatter_workspace_bytes(M), g.device)
        _C.check(_C.lib().fr_row_scatter_sum(g.data_ptr(), idx.data_ptr(), M, N, D, dX.data_ptr(), ws.data_ptr(), ws.numel(),
                                             _C.ptr(ctx.err), _C.current_stream()), "fr_row_scatter_sum")
        return dX, None, None


def dyn_neg_select(scores: torch.Tensor, cand: torch.Tensor) -> torch.Tensor:
    """`cand[argmax(scores, 0), range(cols)]` of [M, cols] scores and candidate ids -- the pick of dynamic negative sampling
    (abstract_dataloader.py `_neg_sampling`: `torch.max(scores, dim=0)[1]` then the advanced index), in one launch
    (fr_dyn_neg_select): the first maximum wins ties, a NaN wins, the first NaN among several."""
    scores = scores.to(torch.float32).contiguous()
    cand = cand.to(torch.int64).contiguous()
    if scores.dim() != 2 or cand.shape != scores.shape:
        raise ValueError(f'dyn_neg_select: scores {tuple(scores.shape)} and candidates {tuple(cand.shape)} must be the same [M, cols]')
    M, cols = scores.shape
    out = torch.empty(cols, dtype=torch.int64, device=scores.device)
    _C.check(_C.lib().fr_dyn_neg_select(scores.data_ptr(), cand.data_ptr(), cols, M, out.data_ptr(), _C.current_stream()),
             "fr_dyn_neg_select")
    return out


def dyn_neg_dot_select(item_table, item_hyper, user_rows, cand, num, M, err_flag, item_bias=None, user_bias=None,
                       global_bias=None, scores_only=False):
    """fr_dyn_neg_dot_select: of the M candidates cand[(r*num + j)*n + i] of column j*n + i keep the one with the highest
    sigmoid(((user_rows[i] . item row + user_bias[i]) + item bias) + global_bias) -- PFCNBase.predict's values, the item rows
    read as of the lazy table's step, never materialised.  `item_bias` = (LazyTable, AdamHyper) or None.  `scores_only`: the
    [M*num*n] scores in cand's order instead (fr_dyn_neg_dot_scores)."""
    user_rows = user_rows.to(torch.float32).contiguous()
    cand = cand.to(torch.int64).contiguous()
    n = user_rows.shape[0]
    if user_rows.dim() != 2 or user_rows.shape[1] != item_table.dim or cand.numel() != n * int(num) * int(M):
        raise ValueError('dyn_neg_dot_select: user rows [n, D] against [M*num*n] candidates of a D-wide table')
    ub = user_bias.to(torch.float32).contiguous().view(-1) if user_bias is not None else None
    gb = global_bias.detach().to(torch.float32).contiguous() if global_bias is not None else None
    bt, bh = (item_bias[0].c(), item_bias[1].c()) if item_bias is not None else (None, None)
    it = item_table.c()
    dev = user_rows.device
    if scores_only:
        out, fn, name = torch.empty(cand.numel(), dtype=torch.float32, device=dev), _C.lib().fr_dyn_neg_dot_scores, "fr_dyn_neg_dot_scores"
    else:
        out, fn, name = torch.empty(n * int(num), dtype=torch.int64, device=dev), _C.lib().fr_dyn_neg_dot_select, "fr_dyn_neg_dot_select"
    _C.check(fn(ctypes.byref(it), ctypes.byref(item_hyper.c()), ctypes.byref(bt) if bt is not None else None,
                ctypes.byref(bh) if bh is not None else None, user_rows.data_ptr(), _C.ptr(ub), _C.ptr(gb), cand.data_ptr(),
                n, int(num), int(M), out.data_ptr(), _C.ptr(err_flag), _C.current_stream()), name)
    return out


# ---- recommendation: top-k without the dense score matrix (csrc/recommend.hip) ------------------------------------------
def _check_k(k, n_cols):
    k = int(k)
    if k > _C.FR_TOPK_MAX:
        raise ValueError(f'k = {k} is above FR_TOPK_MAX = {_C.FR_TOPK_MAX}, the most the top-k kernels select')
    if k < 1 or k > n_cols:
        raise ValueError(f'k = {k} not in 1..{n_cols}')
    return k


def topk_rows(scores, k, slices=0):
    """fr_topk_rows: (values, indices) of the k best cells of every row of a dense fp32 matrix (rows may be strided), in the
    library's total order: higher score first, NaN above +inf, the lower column first among equal scores."""
    if scores.dim() != 2 or scores.dtype != torch.float32 or not scores.is_cuda or scores.stride(1) != 1:
        raise _C.FairrecError('topk_rows: a [rows, cols] fp32 matrix with unit column stride on a ROCm device')
    R, N = scores.shape
    k = _check_k(k, N)
    ld = scores.stride(0) if R > 1 else max(scores.stride(0), N)
    lib = _C.lib()
    ws = torch.empty(lib.fr_topk_rows_workspace_bytes(R, N, k, int(slices)) // 8, dtype=torch.int64, device=scores.device)
    val = torch.empty((R, k), dtype=torch.float32, device=scores.device)
    idx = torch.empty((R, k), dtype=torch.int64, device=scores.device)
    _C.check(lib.fr_topk_rows(scores.data_ptr(), R, N, ld, k, int(slices), val.data_ptr(), idx.data_ptr(), _C.ptr(ws),
                              ws.numel() * 8, _C.current_stream()), "fr_topk_rows")
    return val, idx


def _rec_args(who, X, W, user_bias, item_bias, bias0, epilogue, scale, mask_pad, hist_indptr, hist_items):
    """The fr_rec_args of a call (k, slices and scores_out left 0 for the caller) and the tensors its pointers belong to."""
    if not X.is_cuda:
        raise _C.FairrecError(f'{who}: ROCm device tensors only')
    X = X.detach().to(torch.float32).contiguous()
    W = W.detach().to(torch.float32).contiguous()
    U, D = X.shape
    N = W.shape[0]
    if W.dim() != 2 or W.shape[1] != D:
        raise ValueError(f'{who}: X [U, D] against W [n_items, D]')
    dev = X.device
    ub = user_bias.detach().to(torch.float32).contiguous().view(-1) if user_bias is not None else None
    ib = item_bias.detach().to(torch.float32).contiguous().view(-1) if item_bias is not None else None
    if (ub is not None and ub.numel() != U) or (ib is not None and ib.numel() != N):
        raise ValueError(f'{who}: user_bias [U], item_bias [n_items]')
    ip = hi = None
    if hist_indptr is not None:
        ip = hist_indptr.to(dev, torch.int64).contiguous()
        hi = hist_items.to(dev, torch.int64).contiguous()
        if ip.numel() != U + 1:
            raise ValueError(f'{who}: hist_indptr [U + 1]')
    a = _C.FrRecArgs(X.data_ptr(), W.data_ptr(), _C.ptr(ub), _C.ptr(ib), _C.ptr(ip), _C.ptr(hi), 0, U, N,
                     hi.numel() if hi is not None else 0, D, 0, int(epilogue), int(bool(mask_pad)), 1, 0,
                     float(bias0), float(scale))
    return a, (X, W, ub, ib, ip, hi)


def recommend_kwargs(factors, rows=None):
    """What a model's `full_sort_factors` dict says to recommend_topk / recommend_cells / recommend_meanrank, as their keyword
    arguments: X and W, and the optional pieces with the defaults of a plain dot product.  `rows`: only these users, in this
    order (X[rows], user_bias[rows])."""
    X, ub = factors['X'], factors.get('user_bias')
    if rows is not None:
        X, ub = X[rows], None if ub is None else ub.view(-1)[rows]
    return dict(X=X, W=factors['W'], user_bias=ub, item_bias=factors.get('item_bias'), bias0=factors.get('bias0', 0.0),
                epilogue=factors.get('epilogue', 0), scale=factors.get('scale', 1.0))


def recommend_topk(X, W, k, user_bias=None, item_bias=None, bias0=0.0, epilogue=0, scale=1.0, mask_pad=False,
                   hist_indptr=None, hist_items=None, want_scores=False, slices=0):
    """fr_recommend_topk: (values, indices[, scores]) of the k best items of every row of X against the item table W, score
    = epilogue(((X[u] . W[i] + user_bias[u]) + item_bias[i]) + bias0), the pad item and the history CSR (ascending within a
    user) scored -inf.  Nothing of size [users, items] is stored unless `want_scores` asks for the dense masked matrix."""
    a, keep = _rec_args('recommend_topk', X, W, user_bias, item_bias, bias0, epilogue, scale, mask_pad, hist_indptr, hist_items)
    U, N, dev = a.n_users, a.n_items, keep[0].device
    k = _check_k(k, N)
    scores = torch.empty((U, N), dtype=torch.float32, device=dev) if want_scores else None
    a.k, a.slices, a.scores_out = k, int(slices), _C.ptr(scores) or None
    lib = _C.lib()
    ws = torch.empty(lib.fr_recommend_topk_workspace_bytes(ctypes.byref(a)) // 8, dtype=torch.int64, device=dev)
    val = torch.empty((U, k), dtype=torch.float32, device=dev)
    idx = torch.empty((U, k), dtype=torch.int64, device=dev)
    _C.check(lib.fr_recommend_topk(ctypes.byref(a), val.data_ptr(), idx.data_ptr(), _C.ptr(ws), ws.numel() * 8,
                                   _C.current_stream()), "fr_recommend_topk")
    return (val, idx, scores) if want_scores else (val, idx)


def recommend_cells(X, W, cell_user, cell_item, err_flag, user_bias=None, item_bias=None, bias0=0.0, epilogue=0, scale=1.0,
                    mask_pad=False, hist_indptr=None, hist_items=None):
    """fr_recommend_cells: float32 [n] = the cells (cell_user[c], cell_item[c]) of the masked matrix `recommend_topk(...,
    want_scores=True)` would return for the same arguments, bit for bit, without the matrix.  An id outside its table sets
    DEV_ERR_INDEX_RANGE in `err_flag` (a device int32 / uint32 scalar the caller reads when it can afford the sync)."""
    a, keep = _rec_args('recommend_cells', X, W, user_bias, item_bias, bias0, epilogue, scale, mask_pad, hist_indptr, hist_items)
    dev = keep[0].device
    cu = cell_user.to(dev, torch.int64).contiguous().view(-1)
    ci = cell_item.to(dev, torch.int64).contiguous().view(-1)
    if cu.numel() != ci.numel():
        raise ValueError('recommend_cells: cell_user and cell_item of one length')
    out = torch.empty(cu.numel(), dtype=torch.float32, device=dev)
    _C.check(_C.lib().fr_recommend_cells(ctypes.byref(a), _C.ptr(cu), _C.ptr(ci), cu.numel(), _C.ptr(out), _C.ptr(err_flag),
                                         _C.current_stream()), "fr_recommend_cells")
    return out


def recommend_meanrank(X, W, pos_keys, err_flag, user_bias=None, item_bias=None, bias0=0.0, epilogue=0, scale=1.0,
                       mask_pad=False, hist_indptr=None, hist_items=None):
    """fr_recommend_meanrank: int64 [U, 3] = [2 * pos_rank_sum, user_len, pos_len] per user, what fr_eval_meanrank_segments
    returns on the dense masked matrix of the same arguments; pos_keys = the SORTED keys user * n_items + item."""
    a, keep = _rec_args('recommend_meanrank', X, W, user_bias, item_bias, bias0, epilogue, scale, mask_pad, hist_indptr, hist_items)
    dev = keep[0].device
    keys = pos_keys.to(dev, torch.int64).contiguous().view(-1)
    lib = _C.lib()
    out = torch.empty((a.n_users, 3), dtype=torch.int64, device=dev)
    ws = torch.empty(lib.fr_recommend_meanrank_workspace_bytes(ctypes.byref(a), keys.numel()) // 4, dtype=torch.int32, device=dev)
    _C.check(lib.fr_recommend_meanrank(ctypes.byref(a), _C.ptr(keys), keys.numel(), _C.ptr(out), _C.ptr(ws), ws.numel() * 4,
                                       _C.ptr(err_flag), _C.current_stream()), "fr_recommend_meanrank")
    return out


# ---- unit rows: the cosine of two rows as the dot product of their normalised forms (csrc/rows_normalize.hip) ------------
def rows_l2_normalize(X, eps=1e-8, out=None, want_norm=False):
    """fr_rows_l2_normalize: Y[r] = X[r] / max(|X[r]|, eps) for every row of a [rows, D] fp32 matrix, D in 1..256 (rows may be
    strided, columns not), with the arithmetic of include/fairrec_hip.h: a row's bits depend on that row, D and eps alone.
    `out`: where to write -- X itself for an in-place call -- else a new tensor.  `want_norm`: also the rows' unclamped norms,
    (Y, norms [rows]).  Inference only: no autograd graph."""
    if not X.is_cuda:
        raise _C.FairrecError('rows_l2_normalize: ROCm device tensors only; there is no CPU fallback')
    if X.dim() != 2 or X.dtype != torch.float32:
        raise _C.FairrecError('rows_l2_normalize: X is a [rows, D] fp32 matrix')
    X = X.detach()
    M, D = X.shape
    if not 1 <= D <= 256:
        raise ValueError(f'rows_l2_normalize: D = {D} not in 1..256')
    if D > 1 and X.stride(1) != 1:
        X = X.contiguous()
    Y = torch.empty((M, D), dtype=torch.float32, device=X.device) if out is None else out.detach()
    if Y.shape != X.shape or Y.dtype != torch.float32 or Y.device != X.device or (D > 1 and Y.stride(1) != 1):
        raise _C.FairrecError('rows_l2_normalize: out is an fp32 matrix of the shape and device of X with unit column stride')
    norms = torch.empty(M, dtype=torch.float32, device=X.device) if want_norm else None
    if M:
        ldx = X.stride(0) if M > 1 else max(X.stride(0), D)
        ldy = Y.stride(0) if M > 1 else max(Y.stride(0), D)
        _C.check(_C.lib().fr_rows_l2_normalize(X.data_ptr(), M, D, ldx, float(eps), Y.data_ptr(), ldy, _C.ptr(norms),
                                               _C.current_stream()), "fr_rows_l2_normalize")
    Y = Y if out is None else out
    return (Y, norms) if want_norm else Y


# ---- inference through whole MLPs in one launch (csrc/mlp_infer.hip) ----------------------------------------------------
def mlp_net(module) -> "_C.FrMlpNet":
    """The fr_mlp_net of an `MLPLayers` module: its Linear layers, its BatchNorm layers' RUNNING statistics, its activation.
    The struct holds raw pointers: the module's tensors must outlive the launch it is handed to."""
    from .model.layers import ACT_CODES
    lins, bns = module.linears(), module.batchnorms()
    if not 1 <= len(lins) <= _C.MLP_INFER_MAX_LAYERS:
        raise ValueError(f'mlp_infer: {len(lins)} layers, not in 1..{_C.MLP_INFER_MAX_LAYERS}')
    name = module.activation.lower() if isinstance(module.activation, str) else module.activation
    net = _C.FrMlpNet()
    net.n_layers, net.k_in = len(lins), lins[0].in_features
    for l, lin in enumerate(lins):
        bn = bns[l] if module.use_bn else None
        tensors = [lin.weight, lin.bias] + ([bn.weight, bn.bias, bn.running_mean, bn.running_var] if bn is not None else [])
        for t in tensors:
            if t is None or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
                raise _C.FairrecError('mlp_infer: every weight, bias and running statistic is a contiguous fp32 tensor on a ROCm '
                                      'device (a Linear without bias or a BatchNorm without affine / running statistics is not served)')
        net.layer[l] = _C.FrMlpLayer(*[t.data_ptr() for t in tensors], *([None] * (6 - len(tensors))),
                                     float(bn.eps) if bn is not None else 0.0, lin.out_features, ACT_CODES[name])
    return net


def mlp_infer(nets, X, out_div=1.0):
    """fr_mlp_infer: (nets[0](X) + nets[1](X) + ...) / out_div for `MLPLayers` modules (or prepared `mlp_net` structs) in ONE
    launch -- Linear, BatchNorm1d on the running statistics, activation -- with every output row a function of its input row
    alone.  Inference only: no autograd graph, no buffer of the modules is touched, dropout is not applied."""
    nets = list(nets) if isinstance(nets, (list, tuple)) else [nets]
    if not 1 <= len(nets) <= _C.MLP_INFER_MAX_NETS:
        raise ValueError(f'mlp_infer: {len(nets)} nets, not in 1..{_C.MLP_INFER_MAX_NETS}')
    if not X.is_cuda:
        raise _C.FairrecError('mlp_infer: ROCm device tensors only; there is no CPU fallback')
    if X.dim() != 2 or X.dtype != torch.float32:
        raise _C.FairrecError('mlp_infer: X is a [rows, k_in] fp32 matrix')
    X = X.detach().contiguous()
    structs = [n if isinstance(n, _C.FrMlpNet) else mlp_net(n) for n in nets]
    if X.shape[1] != structs[0].k_in:
        raise ValueError(f'mlp_infer: X has {X.shape[1]} columns, the nets take {structs[0].k_in}')
    arr = (_C.FrMlpNet * len(structs))(*structs)
    last = structs[0].layer[structs[0].n_layers - 1].n_out
    Y = torch.empty((X.shape[0], last), dtype=torch.float32, device=X.device)
    if X.shape[0] == 0:
        return Y
    _C.check(_C.lib().fr_mlp_infer(arr, len(structs), float(out_div), X.data_ptr(), X.shape[0], Y.data_ptr(),
                                   _C.current_stream()), "fr_mlp_infer")
    return Y


def _check_upper_layers(who, layers, n_in, dev):
    """The (W, bias) of the linears above a split first one of n_in outputs, as the fused scorers take them on device `dev`."""
    if not 1 <= len(layers) <= _C.PAIR_MLP_MAX_LINEARS - 1:
        raise ValueError(f'{who}: {len(layers) + 1} linears, not in 2..{_C.PAIR_MLP_MAX_LINEARS}')
    for W, b in layers:
        if tuple(W.shape[1:]) != (n_in,) or tuple(b.shape) != (W.shape[0],) or W.dtype != torch.float32 or b.dtype != torch.float32 \
                or W.device != dev or b.device != dev or not W.is_contiguous() or not b.is_contiguous():
            raise ValueError(f'{who}: each layer is (W [n_out, n_in], bias [n_out]), contiguous fp32 on the device of P')
        n_in = W.shape[0]


def _set_upper_layers(a, layers):
    for l, (W, b) in enumerate(layers):
        a.W[l], a.bias[l], a.n_out[l] = W.data_ptr(), b.data_ptr(), W.shape[0]


# ---- all-item scores of an MLP scorer over cat(user, item), first layer split (csrc/pair_mlp.hip) ------------------------
def pair_mlp_supported(mlp, n_first=None) -> bool:
    """Does fr_pair_mlp_scores serve this `MLPLayers` scorer?  ReLU, no BatchNorm, no recorded dropout masks, 2..6 linears with
    biases, one output, the first layer's and every hidden width in 1..256."""
    from .model.layers import ACT_CODES
    name = mlp.activation.lower() if isinstance(mlp.activation, str) else mlp.activation
    lins = mlp.linears()
    if mlp.use_bn or mlp.forced_masks is not None or any(lin.bias is None for lin in lins):
        return False
    if not 2 <= len(lins) <= _C.PAIR_MLP_MAX_LINEARS:
        return False
    n_out = (ctypes.c_int32 * (len(lins) - 1))(*[lin.out_features for lin in lins[1:]])
    return bool(_C.lib().fr_pair_mlp_supported(lins[0].out_features if n_first is None else n_first, len(lins), n_out,
                                               ACT_CODES[name]))


def pair_mlp_pieces(mlp, user_rows, item_rows):
    """The pieces fr_pair_mlp_scores takes, of an `MLPLayers` scorer over cat(user_rows[u], item_rows[i]): P = user_rows
    W1[:, :D]^T + b1 and Q = item_rows W1[:, D:]^T (two fr_linear_fwd products), and the remaining layers' parameters.  Nothing
    is kept between calls: the parameters may move."""
    lins = mlp.linears()
    x = user_rows.detach().to(torch.float32).contiguous()
    w = item_rows.detach().to(torch.float32).contiguous()
    D, Di = x.shape[1], w.shape[1]
    W1 = lins[0].weight.detach()
    if W1.shape[1] != D + Di:
        raise ValueError(f'pair_mlp_pieces: the first layer takes {W1.shape[1]} columns, the rows have {D} + {Di}')
    n1 = W1.shape[0]
    lib, st = _C.lib(), _C.current_stream()

    def product(rows, Wpart, bias):
        out = torch.empty((rows.shape[0], n1), dtype=torch.float32, device=rows.device)
        if rows.shape[0]:
            _C.check(lib.fr_linear_fwd(rows.data_ptr(), rows.shape[1], None, 0, None, 1.0, Wpart.data_ptr(), _C.ptr(bias),
                                       rows.shape[0], n1, 0, out.data_ptr(), st), "fr_linear_fwd")
        return out

    P = product(x, W1[:, :D].contiguous(), lins[0].bias.detach().contiguous())
    Q = product(w, W1[:, D:].contiguous(), None)
    return {'P': P, 'Q': Q, 'layers': [(lin.weight.detach().contiguous(), lin.bias.detach().contiguous()) for lin in lins[1:]]}


def pair_mlp_scores(pieces, mask_pad=False, hist_indptr=None, hist_items=None, out=None, act=1):
    """fr_pair_mlp_scores: the dense [users, items] matrix sigmoid(act(upper layers(act(P[u] + Q[i])))) of `pair_mlp_pieces`,
    the pad item and the history CSR (ascending within a user) scored -inf.  `out`: a [users, >= items] fp32 buffer with unit
    column stride to write into (its columns beyond the items are left alone)."""
    P, Q, layers = pieces['P'], pieces['Q'], pieces['layers']
    if not P.is_cuda:
        raise _C.FairrecError('pair_mlp_scores: ROCm device tensors only; there is no CPU fallback')
    P, Q = P.contiguous(), Q.contiguous()
    U, N, dev = P.shape[0], Q.shape[0], P.device
    if P.dim() != 2 or Q.dim() != 2 or Q.shape[1] != P.shape[1] or P.dtype != torch.float32 or Q.dtype != torch.float32 \
            or Q.device != dev:
        raise ValueError('pair_mlp_scores: P [users, n1] and Q [items, n1], fp32, on one device')
    _check_upper_layers('pair_mlp_scores', layers, P.shape[1], dev)
    if out is None:
        out = torch.empty((U, N), dtype=torch.float32, device=dev)
    if out.dim() != 2 or out.dtype != torch.float32 or out.shape[0] != U or out.shape[1] < N or (N and out.stride(1) != 1):
        raise _C.FairrecError('pair_mlp_scores: out is a [users, >= items] fp32 matrix with unit column stride')
    if U == 0 or N == 0:
        return out
    ld = out.stride(0) if U > 1 else max(out.stride(0), out.shape[1])
    ip = hi = None
    if hist_indptr is not None:
        ip = hist_indptr.to(dev, torch.int64).contiguous()
        hi = hist_items.to(dev, torch.int64).contiguous()
        if ip.numel() != U + 1:
            raise ValueError('pair_mlp_scores: hist_indptr [users + 1]')
    a = _C.FrPairMlpArgs()
    a.P, a.Q = P.data_ptr(), Q.data_ptr()
    _set_upper_layers(a, layers)
    a.hist_indptr, a.hist_items, a.scores_out = _C.ptr(ip), _C.ptr(hi), out.data_ptr()
    a.n_users, a.n_items, a.ld, a.hist_len = U, N, ld, hi.numel() if hi is not None else 0
    a.n1, a.n_linears, a.act, a.mask_pad, a.hist_sorted = P.shape[1], len(layers) + 1, int(act), int(bool(mask_pad)), 1
    _C.check(_C.lib().fr_pair_mlp_scores(ctypes.byref(a), _C.current_stream()), "fr_pair_mlp_scores")
    return out


# ---- dynamic negatives of an MLP scorer over cat(user, item), first layer split (csrc/dyn_neg_mlp.hip) --------------------
def dyn_neg_mlp_pieces(mlp, user_rows):
    """The pieces fr_dyn_neg_mlp_select takes, of an `MLPLayers` scorer over cat(user_rows[i], item row): P = user_rows
    W1[:, :D]^T + b1 (one fr_linear_fwd product over the batch rows), the first weight itself -- its item half is read in place
    -- and the remaining layers' parameters.  Nothing is kept between calls: the parameters may move."""
    lins = mlp.linears()
    x = user_rows.detach().to(torch.float32).contiguous()
    D = x.shape[1]
    W1 = lins[0].weight.detach().contiguous()
    if W1.shape[1] <= D:
        raise ValueError(f'dyn_neg_mlp_pieces: the first layer takes {W1.shape[1]} columns, the user rows alone have {D}')
    n1 = W1.shape[0]
    P = torch.empty((x.shape[0], n1), dtype=torch.float32, device=x.device)
    if x.shape[0]:
        _C.check(_C.lib().fr_linear_fwd(x.data_ptr(), D, None, 0, None, 1.0, W1[:, :D].contiguous().data_ptr(),
                                        lins[0].bias.detach().contiguous().data_ptr(), x.shape[0], n1, 0, P.data_ptr(),
                                        _C.current_stream()), "fr_linear_fwd")
    return {'P': P, 'W1': W1, 'layers': [(lin.weight.detach().contiguous(), lin.bias.detach().contiguous()) for lin in lins[1:]]}


def dyn_neg_mlp_select(pieces, item_table, item_hyper, cand, num, M, err_flag, want_scores=False):
    """fr_dyn_neg_mlp_select: of the M candidates cand[(r*num + j)*n + i] of column j*n + i keep the one the scorer rates
    highest, sigmoid(relu(upper layers(relu(P[i] + W1[:, D_user:] w_c)))) with w_c the candidate's row of the lazy item table as
    of its step, never materialised.  `pieces`: {'P': [n, n1] (the user half of the first layer, bias added), 'W1': the first
    layer's whole [n1, D_user + D] weight (its item half is read in place), 'layers': the remaining (W, bias)}.
    `want_scores`: (ids, the [M*num*n] scores in cand's order they were picked from) -- fr_dyn_neg_mlp_scores, a second launch."""
    P, W1, layers = pieces['P'], pieces['W1'], pieces['layers']
    if not P.is_cuda:
        raise _C.FairrecError('dyn_neg_mlp_select: ROCm device tensors only; there is no CPU fallback')
    dev, D = P.device, item_table.dim
    num, M = int(num), int(M)
    if P.dim() != 2 or P.dtype != torch.float32 or P.stride(1) != 1 or (P.shape[0] > 1 and P.stride(0) < P.shape[1]):
        raise ValueError('dyn_neg_mlp_select: P is an fp32 [n, n1] matrix with unit column stride')
    n, n1 = P.shape
    if W1.dim() != 2 or W1.dtype != torch.float32 or W1.device != dev or not W1.is_contiguous() or W1.shape[0] != n1 \
            or W1.shape[1] <= D:
        raise ValueError(f'dyn_neg_mlp_select: W1 is the contiguous fp32 [n1 = {n1}, D_user + {D}] first weight on the device of P')
    _check_upper_layers('dyn_neg_mlp_select', layers, n1, dev)
    if num < 1 or M < 1 or cand.numel() != n * num * M:
        raise ValueError(f'dyn_neg_mlp_select: {cand.numel()} candidates, not M * num * n = {M} * {num} * {n}')
    cand = cand.to(dev, torch.int64).contiguous()
    it, hy = item_table.c(), item_hyper.c()
    a = _C.FrDynNegMlpArgs()
    a.item_t, a.item_optim = ctypes.pointer(it), ctypes.pointer(hy)
    a.P, a.W1_item = P.data_ptr(), W1.data_ptr() + 4 * (W1.shape[1] - D)
    _set_upper_layers(a, layers)
    a.cand, a.ldp, a.ldw1, a.n = cand.data_ptr(), (P.stride(0) if n > 1 else n1), W1.shape[1], n
    a.n1, a.n_linears, a.act, a.num, a.M = n1, len(layers) + 1, 1, num, M
    lib, st = _C.lib(), _C.current_stream()
    out = torch.empty(n * num, dtype=torch.int64, device=dev)
    _C.check(lib.fr_dyn_neg_mlp_select(ctypes.byref(a), out.data_ptr(), _C.ptr(err_flag), st), "fr_dyn_neg_mlp_select")
    if not want_scores:
        return out
    scores = torch.empty(n * num * M, dtype=torch.float32, device=dev)
    _C.check(lib.fr_dyn_neg_mlp_scores(ctypes.byref(a), scores.data_ptr(), _C.ptr(err_flag), st), "fr_dyn_neg_mlp_scores")
    return out, scores

"""recbole.utils.case_study: what a trained model recommends.

`full_sort_scores` / `full_sort_topk` (reference case_study.py:20-91) for a list of users, on the device, plus the optional
attribute subset the filtered models take.  Which of three paths serves a call is decided in one place,
model/fast_path.full_sort_plan, which the Trainer's full-sort evaluation asks as well.  A dot-product model answers
`full_sort_factors` and is ranked by
fr_recommend_topk, which never stores the [users, n_items] matrix; a model whose MLP scorer over cat(user, item) answers
`full_sort_pair_mlp` (NFCF, PFCN_MLP with `full_sort_scorer: split`) is scored by fr_pair_mlp_scores -- the first layer
split into a user half and an item half, the rest per pair in one kernel -- and ranked by fr_topk_rows; every other model
is scored densely (the scores the Trainer's full-sort evaluation ranks: `dense_full_sort_scores`) and ranked by
fr_topk_rows.  All rank by the library's
total order -- higher score first, NaN first of all, the lower item id among equal scores -- where torch.topk leaves the
order of equal scores open.  The pad item and each user's history (the items of earlier phases, as the reference's
`uid2history_item`) score -inf.  Single device; there is no CPU path.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _C
from ..data.interaction import Interaction
from ..model.fast_path import full_sort_plan, with_subset


def dense_full_sort_scores(model, interaction, n_items, users_per_batch, iid_field, device, sst_list=None):
    """[users, n_items] scores of a batch of users: `model.full_sort_predict`, or -- as the reference does when a model has
    none (trainer.py:425-433) -- `predict` on every (user, item) pair, `users_per_batch` users at a time."""
    from ..model.abstract_recommender import AbstractRecommender
    if type(model).full_sort_predict is not AbstractRecommender.full_sort_predict:
        try:
            return with_subset(model.full_sort_predict, interaction, sst_list).view(-1, n_items)
        except NotImplementedError:
            pass
    U = len(interaction)
    items = torch.arange(n_items, device=device)
    out = torch.empty((U, n_items), dtype=torch.float32, device=device)
    per = max(int(users_per_batch), 1)
    for lo in range(0, U, per):
        part = interaction[lo:lo + per].repeat_interleave(n_items)
        part.update(type(part)({iid_field: items.repeat(min(per, U - lo))}))
        out[lo:lo + per] = with_subset(model.predict, part, sst_list).view(-1, n_items)
    return out


def users_per_batch(config, n_items):
    """Users of one `predict` batch of the full-sort evaluation (general_dataloader.py:186)."""
    return max(int(config['eval_batch_size'] or 4096) // int(n_items), 1)


def history_csr(hist_indptr, hist_items, uids, n_items):
    """(indptr [len(uids) + 1], items) of the rows `uids` of a per-user CSR, in the order given (repeats allowed), the items
    of each row ascending: the form fr_recommend_topk searches."""
    uids = uids.to(hist_indptr.device, torch.int64).view(-1)
    lo, n = hist_indptr[uids], hist_indptr[uids + 1] - hist_indptr[uids]
    indptr = torch.zeros(uids.numel() + 1, dtype=torch.int64, device=uids.device)
    torch.cumsum(n, 0, out=indptr[1:])
    row = torch.repeat_interleave(torch.arange(uids.numel(), device=uids.device), n)
    pos = torch.arange(row.numel(), device=uids.device) + torch.repeat_interleave(lo - indptr[:-1], n)
    keys = torch.sort(row * int(n_items) + hist_items[pos].to(torch.int64)).values
    return indptr, keys % int(n_items)


class _Request:
    """The users of one call: their feature rows, their history CSR, and the model in eval mode for the call's length."""

    def __init__(self, uid_series, model, test_data, device):
        from ..data.dataloader import FullSortEvalDataLoader
        if not isinstance(test_data, FullSortEvalDataLoader):
            raise TypeError('case_study: test_data must be a FullSortEvalDataLoader (eval_args.mode: full)')
        self.device = torch.device(device) if device is not None else test_data.device
        if self.device.type != 'cuda' or not torch.cuda.is_available():
            raise _C.FairrecError(f'case_study runs on a ROCm device; [{self.device}] has no path (there is no CPU fallback)')
        dataset = test_data.dataset
        self.n_items = int(dataset.item_num)
        if torch.is_tensor(uid_series):
            uids = uid_series.to(self.device, torch.int64).view(-1)
        else:
            uids = torch.as_tensor(np.asarray(uid_series, dtype=np.int64).reshape(-1), device=self.device)
        if uids.numel() and (int(uids.min()) < 0 or int(uids.max()) >= int(dataset.user_num)):
            raise ValueError(f'case_study: user ids must be in 0..{int(dataset.user_num) - 1}')
        self.uids = uids
        self.interaction = dataset.join(Interaction({dataset.uid_field: uids})).to(self.device)
        self.indptr, self.items = history_csr(test_data.hist_indptr, test_data.hist_items, uids, self.n_items)
        self.per = users_per_batch(test_data.config, self.n_items)
        self.iid_field = dataset.iid_field
        self.model = model

    def split(self, pieces, lo, hi, out=None):
        """Rows lo..hi of the split scorer's masked matrix (fr_pair_mlp_scores)."""
        from ..functional import pair_mlp_scores
        a, b = int(self.indptr[lo]), int(self.indptr[hi])
        return pair_mlp_scores(dict(pieces, P=pieces['P'][lo:hi]), mask_pad=True, hist_indptr=self.indptr[lo:hi + 1] - a,
                               hist_items=self.items[a:b], out=out)

    def dense(self, lo, hi, sst_list):
        """Rows lo..hi of the dense scores, masked as the Trainer masks them."""
        scores = dense_full_sort_scores(self.model, self.interaction[lo:hi], self.n_items, self.per, self.iid_field,
                                        self.device, sst_list)
        if not scores.is_contiguous() or scores.dtype != torch.float32:
            scores = scores.to(torch.float32).contiguous()
        scores[:, 0] = -float('inf')
        a, b = int(self.indptr[lo]), int(self.indptr[hi])
        n = self.indptr[lo + 1:hi + 1] - self.indptr[lo:hi]
        scores[torch.repeat_interleave(torch.arange(hi - lo, device=self.device), n), self.items[a:b]] = -float('inf')
        return scores

    def fused(self, f, k, want_scores):
        from ..functional import recommend_kwargs, recommend_topk
        return recommend_topk(k=k, mask_pad=True, hist_indptr=self.indptr, hist_items=self.items, want_scores=want_scores,
                              **recommend_kwargs(f))


class _EvalMode:
    def __init__(self, model):
        self.model = model

    def __enter__(self):
        self.was = self.model.training
        self.model.eval()

    def __exit__(self, *exc):
        self.model.train(self.was)


DENSE_ROWS_BYTES = 1 << 30      # dense path of full_sort_topk: users are ranked in groups whose score matrix stays below this


@torch.no_grad()
def full_sort_scores(uid_series, model, test_data, device=None, sst_list=None):
    """[len(uid_series), n_items] scores of every item for the given (internal) user ids, in the order given; the pad item
    and each user's history are -inf.  For a model with `full_sort_factors` these are exactly the scores `full_sort_topk`
    ranks (one kernel writes them and selects from them); so they are with `full_sort_pair_mlp` (a cell's bits depend on its
    user, its item and the parameters alone)."""
    req = _Request(uid_series, model, test_data, device)
    with _EvalMode(model):
        kind, answer = full_sort_plan(model, req.interaction, sst_list, req.per)
        if kind == 'factors':
            if req.uids.numel() == 0:
                return torch.empty((0, req.n_items), dtype=torch.float32, device=req.device)
            return req.fused(answer, 1, True)[2]
        if kind == 'pair_mlp':
            return req.split(answer, 0, req.uids.numel())
        return req.dense(0, req.uids.numel(), sst_list)


@torch.no_grad()
def full_sort_topk(uid_series, model, test_data, k, device=None, sst_list=None):
    """(values, indices) [len(uid_series), k] of the k best items the users have not interacted with, as torch.topk
    returns them.  k is at most FR_TOPK_MAX (256)."""
    k = int(k)
    if k > _C.FR_TOPK_MAX:
        raise ValueError(f'full_sort_topk: k = {k} is above FR_TOPK_MAX = {_C.FR_TOPK_MAX}, the most the top-k kernels select')
    req = _Request(uid_series, model, test_data, device)
    if k < 1 or k > req.n_items:
        raise ValueError(f'full_sort_topk: k = {k} not in 1..{req.n_items}')
    from ..functional import topk_rows
    with _EvalMode(model):
        kind, pieces = full_sort_plan(model, req.interaction, sst_list, req.per)
        if kind == 'factors':
            return req.fused(pieces, k, False)
        U = req.uids.numel()
        if kind == 'pair_mlp':      # (the users' halves are formed already: any grouping gives the same bits)
            group = max(DENSE_ROWS_BYTES // (4 * req.n_items), 1)
            buf = torch.empty((min(group, U), req.n_items), dtype=torch.float32, device=req.device)
        else:
            group = max(DENSE_ROWS_BYTES // (4 * req.n_items) // req.per, 1) * req.per      # whole predict batches
        vals, idxs = [], []
        for lo in range(0, U, group):
            hi = min(lo + group, U)
            v, i = topk_rows(req.split(pieces, lo, hi, buf[:hi - lo]) if kind == 'pair_mlp' else req.dense(lo, hi, sst_list), k)
            vals.append(v)
            idxs.append(i)
        if not vals:
            return (torch.empty((0, k), dtype=torch.float32, device=req.device),
                    torch.empty((0, k), dtype=torch.int64, device=req.device))
        return torch.cat(vals), torch.cat(idxs)

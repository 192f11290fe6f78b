"""Collector for full-sort ranking evaluation on the device: the `full` branch of recbole/evaluator/collector.py:131-205.

Per user batch it receives the masked score matrix [users, n_items] (column 0 and the users' history already -inf,
trainer.py:435-437), the batch's positives and the batch Interaction, and keeps -- as device tensors -- what the metrics
need: `rec.topk` (hit flags of the top-max(topk) items | number of positives), `rec.positive_score`, `data.positive_i`
and `data.<sst>`.  The reference builds a dense [users, items] 0/1 matrix per batch to mark the positives; here the hit
flags come from binary searches in the sorted positive keys (fr_eval_hits).

With 'gauc' among the metrics the three ranking branches also gather `rec.meanrank`, int64 [users, 3] =
[2 * pos_rank_sum, user_len, pos_len] per user (fr_eval_meanrank_segments; exact integers, the first column doubled because a
tied rank is a half); without it they collect and launch what they did before.  `eval_args.mode: labeled` keeps `rec.score`
and `data.label` per batch (eval_batch_collect_labeled).

With `utility_by_group` or `exposure_by_group` set, every ranking branch also keeps `data.user.<attr>` -- the attributes either
key selects, one value per row of `rec.topk` -- and (`utility_by_group`) the labeled branch `data.<attr>` per row; without the
keys the collected keys are what they were.

With `fairness_bootstrap` set, every ranking branch also keeps `data.positive_user`: per positive pair the row of its user in
`rec.topk` over the whole evaluation (the batch's row plus the rows of the batches before), the unit the bootstrap resamples;
without the key the collected keys are what they were.

`full_sort_eval: fused` feeds `eval_batch_collect_fused` the model's factors instead of the matrix (same keys, same values).

The three ranking branches differ in how they rank; each ends in `_finish_ranking` (the hit flags and the keys every branch adds).
"""
from __future__ import annotations

from typing import Dict, List

import torch

from .. import _C


def utility_attrs(value, attrs, key='utility_by_group') -> List[str]:
    """`utility_by_group` / `exposure_by_group` (`key`: the name the error messages use): None / False = off ([]), True = every
    attribute of `sst_attr_list`, a list of names = those, each out of `sst_attr_list`."""
    if value is None or value is False:
        return []
    if value is True:
        return list(attrs)
    if not isinstance(value, (list, tuple)) or not all(isinstance(n, str) for n in value):
        raise ValueError(f'{key} must be True or a list of attribute names out of sst_attr_list, not {value!r}')
    strangers = [n for n in value if n not in attrs]
    if strangers:
        raise ValueError(f'{key}: {strangers} not in sst_attr_list {list(attrs)}')
    return list(dict.fromkeys(value))


class Collector:
    def __init__(self, config):
        self.config = config
        topk = config['topk'] or [10]
        self.topk = [topk] if isinstance(topk, int) else list(topk)
        self.sst = list(config['sst_attr_list'] or [])
        self.utility = utility_attrs(config['utility_by_group'], self.sst)
        self.exposure = utility_attrs(config['exposure_by_group'], self.sst, 'exposure_by_group')
        # attributes kept per USER (`data.user.<attr>`): what either key selects
        self.user_attrs = list(dict.fromkeys(self.utility + self.exposure))
        self.full = 'full' in (config['eval_args'] or {}).get('mode', 'full')
        self.meanrank = 'gauc' in [m.lower() for m in (config['metrics'] or [])]
        self.positive_user = bool(config['fairness_bootstrap'])
        self._rows = 0        # rows of `rec.topk` the batches before this one added (get_data_struct resets it)
        self._parts: Dict[str, List[torch.Tensor]] = {}
        self._data: Dict[str, object] = {}
        self._err = None      # device error word of the fused path's kernels (eval_batch_collect_fused)

    def data_collect(self, train_data):
        """collector.py:80-97: what the exposure metrics need from the training data -- the catalogue size and how often
        every item occurs in training (a dense count vector here, a Counter in the reference)."""
        ds = train_data.dataset
        items = ds.inter_feat[ds.iid_field].to(torch.int64)
        self._data['data.num_items'] = int(ds.item_num)
        self._data['data.count_items'] = torch.bincount(items.reshape(-1), minlength=int(ds.item_num)).to(
            torch.device(self.config['device']))

    def _add(self, key, t):
        self._parts.setdefault(key, []).append(t)

    @staticmethod
    def _host_topk(dense: torch.Tensor, K: int) -> torch.Tensor:
        """`torch.topk(dense, K, dim=-1).indices` as the CPU backend orders EQUAL values (fr_topk_like_torch_cpu): the reference
        ranks on the host (collector.py:149), and where a list hangs on an exact tie -- an untrained scorer that clamps, a
        saturated sigmoid -- which candidates enter it and in which order is that kernel's doing (csrc/topk_host.hip).  `dense`:
        the tied users' rows of the reference's [users, n_items] matrix (float32, any device)."""
        rows = dense.to("cpu", torch.float32).contiguous()
        out = torch.empty((rows.shape[0], K), dtype=torch.int64)
        _C.check(_C.lib().fr_topk_like_torch_cpu(rows.data_ptr(), rows.shape[0], rows.shape[1], K, out.data_ptr(), None),
                 "fr_topk_like_torch_cpu")
        return out

    def _attr(self, interaction, name):
        if name not in interaction:
            raise ValueError(f"utility_by_group / exposure_by_group: the evaluation batches carry no column '{name}'")
        return interaction[name]

    def _add_user_attrs(self, interaction, dev, row_idx=None, n_users=None):
        """`utility_by_group` / `exposure_by_group`: `data.user.<attr>`, one value per row of the batch's `rec.topk`.  `interaction`
        has one row per user, or (row_idx given) one per candidate: every row of a user carries the user's value, scattered to
        its row."""
        for s in self.user_attrs:
            col = self._attr(interaction, s).to(dev).reshape(-1)
            if row_idx is not None:
                col = torch.zeros(n_users, dtype=col.dtype, device=dev).index_put_((row_idx,), col)
            self._add('data.user.' + s, col)

    def eval_batch_collect_labeled(self, scores: torch.Tensor, interaction):
        """collector.py:176-181 (`rec.score`, `data.label`): the batch's predictions as they are and its LABEL_FIELD column
        (`utility_by_group`: and `data.<attr>` per row, which the labeled loader joins)."""
        scores = scores.reshape(-1)
        self._add('rec.score', scores.to(torch.float32))
        self._add('data.label', interaction[self.config['LABEL_FIELD']].to(scores.device, torch.float32).reshape(-1))
        for s in self.utility:
            self._add('data.' + s, self._attr(interaction, s).to(scores.device).reshape(-1))

    def _meanrank(self, seg, items, scores, pos_keys, n_items):
        """`rec.meanrank` of a batch: one launch, a wave per user (items None: dense rows); pos_keys = the sorted keys
        row * n_items + item of the batch's positives, as fr_eval_hits takes them."""
        U, n_rows = seg.numel() - 1, scores.numel()
        out = torch.empty((U, 3), dtype=torch.int64, device=scores.device)
        ws = None if items is None else torch.empty(_C.lib().fr_eval_meanrank_workspace_bytes(n_rows), dtype=torch.uint8,
                                                    device=scores.device)
        _C.call('eval_meanrank_segments', seg.data_ptr(), U, _C.ptr(items), scores.data_ptr(), pos_keys.data_ptr(), pos_keys.numel(),
                n_items, n_rows, out.data_ptr(), _C.ptr(ws), 0 if ws is None else ws.numel())
        self._add('rec.meanrank', out)

    def eval_batch_collect(self, scores: torch.Tensor, interaction, positive_u: torch.Tensor, positive_i: torch.Tensor):
        U, n_items = scores.shape
        K = min(max(self.topk), n_items)
        positive_u, positive_i = positive_u.to(scores.device, torch.int64), positive_i.to(scores.device, torch.int64)
        vals, topk_idx = torch.topk(scores, min(K + 1, n_items), dim=-1)
        topk_idx = topk_idx[:, :K].contiguous()
        # rows whose list is decided by an exact tie (inside the list, or at its end): ranked as the reference's host kernel does
        tied = (vals[:, 1:] == vals[:, :-1]).any(dim=1).nonzero().view(-1)
        if tied.numel():
            topk_idx[tied] = self._host_topk(scores[tied], K).to(scores.device)
        keys = torch.sort(positive_u * n_items + positive_i).values
        if self.meanrank:
            # the dense masked rows as they are: row u * n_items + i is the cell of item i
            seg = torch.arange(U + 1, device=scores.device, dtype=torch.int64) * n_items
            self._meanrank(seg, None, scores.to(torch.float32).contiguous().view(-1), keys, n_items)
        self._finish_ranking(topk_idx, keys, scores[positive_u, positive_i], positive_i, interaction, positive_u, K, n_items, U,
                             scores.device, positive_u)
        self._add_user_attrs(interaction, scores.device)

    def eval_batch_collect_fused(self, factors, interaction, hist_indptr: torch.Tensor, hist_items: torch.Tensor,
                                 positive_u: torch.Tensor, positive_i: torch.Tensor):
        """`eval_batch_collect` without its [users, n_items] matrix (`full_sort_eval: fused`): `factors` is what the model's
        `full_sort_factors` hook answered for the batch's users, (hist_indptr, hist_items) their history CSR, ascending within a
        user (case_study.history_csr).  The same keys, shapes and dtypes, and the same values as `eval_batch_collect` gathers
        from the matrix fr_recommend_topk would write for these arguments: the list is selected in the kernel that scores
        (k = K + 1, to see a tie at its end), a user whose list hangs on an exact tie gets its dense row after all and is
        ranked on the host as there, the positives' scores are single cells (fr_recommend_cells), and `rec.meanrank` counts
        the cells against them tile by tile (fr_recommend_meanrank)."""
        from ..functional import recommend_cells, recommend_kwargs, recommend_meanrank, recommend_topk
        from ..utils.case_study import DENSE_ROWS_BYTES, history_csr
        kw = dict(recommend_kwargs(factors), mask_pad=True, hist_indptr=hist_indptr, hist_items=hist_items)
        U, n_items, dev = kw['X'].shape[0], kw['W'].shape[0], kw['X'].device
        K = min(max(self.topk), n_items)
        positive_u, positive_i = positive_u.to(dev, torch.int64), positive_i.to(dev, torch.int64)
        if self._err is None:
            self._err = torch.zeros(1, dtype=torch.int32, device=dev)
        vals, topk_idx = recommend_topk(k=min(K + 1, n_items), **kw)
        topk_idx = topk_idx[:, :K].contiguous()
        # the rows `eval_batch_collect` finds: the K + 1 best values of a row are the same whoever selects them
        tied = (vals[:, 1:] == vals[:, :-1]).any(dim=1).nonzero().view(-1)
        group = max(DENSE_ROWS_BYTES // (4 * n_items), 1)
        for lo in range(0, tied.numel(), group):
            rows = tied[lo:lo + group]
            ip, hi = history_csr(hist_indptr, hist_items, rows, n_items)
            dense = recommend_topk(k=1, mask_pad=True, hist_indptr=ip, hist_items=hi, want_scores=True,
                                   **recommend_kwargs(factors, rows))[2]
            topk_idx[rows] = self._host_topk(dense, K).to(dev)
        keys = torch.sort(positive_u * n_items + positive_i).values
        if self.meanrank:
            self._add('rec.meanrank', recommend_meanrank(pos_keys=keys, err_flag=self._err, **kw))
        cells = recommend_cells(cell_user=positive_u, cell_item=positive_i, err_flag=self._err, **kw)
        self._finish_ranking(topk_idx, keys, cells, positive_i, interaction, positive_u, K, n_items, U, dev, positive_u)
        self._add_user_attrs(interaction, dev)

    def check_device_errors(self):
        """Raises if a kernel of the fused path met an id outside its table (one host sync; the matrix path indexes with
        torch and raises there)."""
        if self._err is not None and int(self._err.item()):
            raise _C.FairrecError('full_sort_eval fused: a positive (user row, item) lies outside the batch or the item table')

    def eval_batch_collect_candidates(self, origin_scores: torch.Tensor, row_idx: torch.Tensor, interaction,
                                      positive_u: torch.Tensor, positive_i: torch.Tensor, n_items: int):
        """The negative-sampling (`uni100`) branch (collector.py:131-205 with full == False, fed by
        trainer.py:440-456): `origin_scores[r]` is the prediction of row r of `interaction` (user row `row_idx[r]` of the
        batch, item `interaction[item][r]`); a user's candidates are its positives and sampled negatives.  The reference
        scatters them into a dense [users, n_items] -inf matrix; here a (row, item) -> score map is a sorted key array,
        the ranking is a sort over the distinct candidates, and every lookup the reference makes in the dense matrix
        -- including the ones that land on -inf -- is a binary search (missing = -inf).  `rec.negative_score` /
        `data.negative_i` / `data.<sst>` follow the reference's row arithmetic literally: rows [P, 2P) of the batch and
        the first P rows, P = number of positives in the batch."""
        dev = origin_scores.device
        iid = self.config['ITEM_ID_FIELD']
        items = interaction[iid].to(dev, torch.int64)
        row_idx = row_idx.to(dev, torch.int64)
        positive_u, positive_i = positive_u.to(dev, torch.int64), positive_i.to(dev, torch.int64)
        U = int(positive_u[-1].item()) + 1                                    # batch_user_num, trainer.py:453
        K = max(self.topk)
        P = positive_u.numel()
        pos_keys = torch.sort(positive_u * n_items + positive_i).values
        self._add_user_attrs(interaction, dev, row_idx, U)
        if K <= 62 and (row_idx.numel() < 2 or bool((row_idx[1:] >= row_idx[:-1]).all())):
            # The evaluation loaders emit a batch user by user: a user's candidates are a contiguous segment, and the whole
            # ranking is ONE launch, a wave per user (fr_eval_topk_segments); every lookup the reference makes in its dense
            # -inf matrix is a scan of the user's segment (fr_eval_lookup_segments).  No sort of the batch's candidates.
            items = items.contiguous()
            sc = origin_scores.reshape(-1).to(torch.float32).contiguous()
            seg = torch.searchsorted(row_idx, torch.arange(U + 1, device=dev, dtype=torch.int64)).contiguous()
            topk_idx = torch.empty((U, K), dtype=torch.int64, device=dev)
            flags = torch.empty(U, dtype=torch.int32, device=dev)
            _C.call('eval_topk_segments', seg.data_ptr(), U, items.data_ptr(), sc.data_ptr(), K, topk_idx.data_ptr(), flags.data_ptr())
            # users whose list hangs on an exact tie (or who have fewer than K + 1 distinct candidates): their rows of the reference's
            # dense -inf matrix are ranked on the host, in torch.topk's CPU order (csrc/topk_host.hip)
            self._rank_tied_on_host(topk_idx, flags.nonzero().view(-1), row_idx, items, sc, n_items, K)

            def lookup(rows, its):
                rows, its = rows.contiguous(), its.contiguous()
                out = torch.empty(rows.numel(), dtype=torch.float32, device=dev)
                _C.call('eval_lookup_segments', seg.data_ptr(), U, items.data_ptr(), sc.data_ptr(), rows.data_ptr(), its.data_ptr(),
                        rows.numel(), out.data_ptr())
                return out.to(origin_scores.dtype)
            if self.meanrank:
                self._meanrank(seg, items, sc, pos_keys, n_items)
        else:
            topk_idx, lookup = self._rank_candidates_general(origin_scores, row_idx, items, pos_keys, n_items, U, K)
        self._finish_ranking(topk_idx, pos_keys, lookup(positive_u, positive_i), positive_i, interaction, slice(P), K, n_items, U, dev,
                             positive_u)
        neg_items = items[P:2 * P]
        self._add('rec.negative_score', lookup(positive_u[:neg_items.numel()], neg_items))
        self._add('data.negative_i', neg_items)

    def _rank_candidates_general(self, origin_scores, row_idx, items, pos_keys, n_items, U, K):
        """The general form of `eval_batch_collect_candidates`, for a batch whose rows are not grouped by user, or K > 62: the
        lists [U, K] and the lookup in the (row, item) -> score map; adds `rec.meanrank` when it is collected."""
        dev = origin_scores.device
        keys, order = torch.sort(row_idx * n_items + items, stable=True)
        first = torch.ones_like(keys, dtype=torch.bool)
        first[1:] = keys[1:] != keys[:-1]
        ckeys, cscore = keys[first], origin_scores.view(-1)[order][first]     # distinct candidates (equal pairs, equal score)

        def lookup(rows, its):
            q = rows * n_items + its
            p = torch.searchsorted(ckeys, q).clamp_(max=ckeys.numel() - 1)
            return torch.where(ckeys[p] == q, cscore[p], torch.full_like(cscore[p], -float('inf')))

        # ranking among a user's candidates: stable sort by score (descending) inside each row
        o1 = torch.sort(cscore, descending=True, stable=True).indices
        o2 = torch.sort((ckeys // n_items)[o1], stable=True).indices
        ranked = o1[o2]                                                        # candidates by (row asc, score desc)
        rrow = (ckeys // n_items)[ranked]
        start = torch.searchsorted(rrow, torch.arange(U, device=dev))
        rank = torch.arange(ranked.numel(), device=dev) - start[rrow]
        topk_idx = torch.zeros((U, K), dtype=torch.int64, device=dev)          # short lists are padded with [PAD] item 0
        keep = rank < K
        topk_idx[rrow[keep], rank[keep]] = (ckeys % n_items)[ranked][keep]
        # users whose list is decided by an exact tie between candidates (ranks j - 1 and j equal, j <= K), or who have fewer
        # than K candidates (the rest of the list is then the host kernel's pick among the -inf entries): their rows of the
        # reference's dense -inf matrix are ranked on the host, in torch.topk's CPU order
        sr = cscore[ranked]
        pair = (rrow[1:] == rrow[:-1]) & (sr[1:] == sr[:-1]) & (rank[1:] <= K)
        cnt = torch.bincount(rrow, minlength=U)
        tied = torch.unique(torch.cat([rrow[1:][pair], (cnt < min(K + 1, n_items)).nonzero().view(-1)]))
        self._rank_tied_on_host(topk_idx, tied, ckeys // n_items, ckeys % n_items, cscore, n_items, K)
        if self.meanrank:
            self._add('rec.meanrank', self._meanrank_general(ckeys, cscore, pos_keys, n_items, U))
        return topk_idx, lookup

    def _rank_tied_on_host(self, topk_idx, tied, rows, items, scores, n_items, K):
        """the lists of the `tied` users, in place: their candidates (user row rows[r], item items[r], score scores[r]) scattered
        into their rows of the reference's dense -inf matrix, ranked in torch.topk's CPU order (_host_topk)"""
        if not tied.numel():
            return
        dev = topk_idx.device
        slot = torch.full((topk_idx.shape[0],), -1, dtype=torch.int64, device=dev)
        slot[tied] = torch.arange(tied.numel(), device=dev)
        sel = slot[rows] >= 0
        dense = torch.full((tied.numel(), n_items), -float('inf'), dtype=torch.float32, device=dev)
        dense[slot[rows[sel]], items[sel]] = scores[sel].to(torch.float32)
        topk_idx[tied] = self._host_topk(dense, K).to(dev)

    @staticmethod
    def _meanrank_general(ckeys, cscore, pos_keys, n_items, U):
        """`rec.meanrank` of the general form above from its distinct cells (ckeys sorted, cscore): index arithmetic over the
        cells ordered by (row, score); a run of equal scores in a row shares the mean rank."""
        dev = ckeys.device
        live = cscore > -float('inf')
        ck, cs = ckeys[live], cscore[live].to(torch.float32)
        o1 = torch.sort(cs, stable=True).indices
        order = o1[torch.sort((ck // n_items)[o1], stable=True).indices]                  # cells by (row asc, score asc)
        r, sc, n = (ck // n_items)[order], cs[order], ck.numel()
        head = torch.ones(n, dtype=torch.bool, device=dev)
        head[1:] = (r[1:] != r[:-1]) | (sc[1:] != sc[:-1])
        run_id = torch.cumsum(head, 0) - 1
        run_start = head.nonzero().view(-1)
        run_end = torch.cat([run_start[1:], torch.tensor([n], device=dev)])
        row_end = torch.searchsorted(r, torch.arange(U, device=dev), right=True)
        pos = torch.isin(ck[order], pos_keys)
        greater, equal = row_end[r] - run_end[run_id], run_end[run_id] - run_start[run_id]
        out = torch.zeros((U, 3), dtype=torch.int64, device=dev)
        out[:, 0].index_add_(0, r[pos], (2 * greater + equal + 1)[pos])
        out[:, 1] = torch.bincount(r, minlength=U)
        out[:, 2] = torch.bincount(r[pos], minlength=U)
        return out

    def _finish_ranking(self, topk_idx, pos_keys, positive_score, positive_i, interaction, sst_rows, K, n_items, U, dev, positive_u):
        """Where a ranking batch is finished, whichever branch ranked it: the hit flags of the lists against the SORTED positive keys
        row * n_items + item (fr_eval_hits), then `rec.topk`, `rec.items`, `rec.positive_score`, `data.positive_i` and `data.<sst>`
        (rows `sst_rows` of the batch's columns: the positives' user rows, or the reference's [:P] in the candidates branch).
        `fairness_bootstrap`: and `data.positive_user` = positive_u (the positives' rows in the batch) plus the rows before it."""
        rec = torch.empty((U, K + 1), dtype=torch.int32, device=dev)
        _C.call('eval_hits', topk_idx.data_ptr(), U, K, n_items, pos_keys.data_ptr(), pos_keys.numel(), rec.data_ptr())
        self._add('rec.topk', rec)
        self._add('rec.items', topk_idx)
        self._add('rec.positive_score', positive_score)
        self._add('data.positive_i', positive_i)
        for s in self.sst:
            if s in interaction:
                self._add('data.' + s, interaction[s].to(dev)[sst_rows])
        if self.positive_user:
            self._add('data.positive_user', positive_u + self._rows)
            self._rows += U

    def get_data_struct(self) -> Dict[str, torch.Tensor]:
        out = {k: torch.cat(v, dim=0) for k, v in self._parts.items()}
        out.update(self._data)
        self._parts = {}
        self._rows = 0
        return out

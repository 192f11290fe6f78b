"""Evaluation metrics on the device with the result keys of recbole/evaluator/metrics.py:
'hit@k', 'mrr@k', 'ndcg@k', 'recall@k', 'precision@k' and '<Name> Unfairness of sensitive attribute <sst>' /
'Differential Fairness of sensitive attribute <sst>', rounded to `metric_decimal_place`.

Inputs are the arrays the reference's Collector gathers (collector.py:131-205), as device tensors:
  rec_topk       [users, max(topk) + 1]  hit flags of the ranked list | number of positives
  pos_score, pos_i                        score and item id of every positive (user, item) pair
  neg_score, neg_i                        (uni100-style modes) the first len(pos) negatives of the batch order
  sst[<name>]                             the user's attribute value per positive pair
The torch ops here are index plumbing (sort / unique of the id columns; the groups of an attribute or intersection and their
segments are built in groups.py, nowhere else); every reduction is a HIP kernel
(csrc/metrics.hip: fr_topk_metrics, fr_group_sums, fr_fair_metrics_from_stats; fr_df_cells for an attribute, or an
intersection of attributes (`sst_intersections`), with more than eight values).

`utility_by_group` (off by default) adds the ranking and value metrics per group of a sensitive attribute or intersection,
'<m> of <A>=<value>', and their '<m> gap | std | min of sensitive attribute <A>': group_topk_metrics (fr_topk_metrics_grouped),
group_gauc (fr_gauc_grouped), group_value_metrics (the value kernels on each group's slice of the rows sorted by group).

`exposure_by_group` (off by default) adds the six exposure metrics per group in the same key form, with '<m> max of sensitive
attribute <A>' as well: group_exposure_metrics (csrc/exposure.hip: fr_exposure_grouped, every group and every k in one chain after
ONE torch.sort of the keys (group, item, rank); no [groups, items] table).

`group_bootstrap: B` (off by default; with `utility_by_group`) adds percentile intervals from B replicates of a Poisson bootstrap over
users, '<m> ci_low | ci_high of <A>=<value>' and '<m> gap ci_low | ci_high of sensitive attribute <A>', for the top-k metrics and
gauc: topk_user_terms / gauc_user_terms once per evaluation, bootstrap_group_sums per attribute (csrc/bootstrap.hip:
fr_bootstrap_group_sums, the U x B weights made in registers and never stored), bootstrap_intervals on the host.

`fairness_bootstrap: B` (off by default) adds percentile intervals of the fairness metrics from B replicates of the same Poisson
bootstrap over users, '<metric> ci_low | ci_high of sensitive attribute <A>': bootstrap_fairness (csrc/bootstrap_fair.hip:
fr_bootstrap_fair_metrics walks the item-sorted members once for all replicates; no weight and no per-replicate table is stored),
bootstrap_intervals on the host.  Attributes and intersections with at most NARROW_GROUPS groups.

`eval_args.mode: labeled` is evaluation by value: 'auc', 'logloss', 'mae', 'rmse' of `rec.score` (what `predict` returned)
against `data.label` (LABEL_FIELD), every row of the evaluation set (fr_value_metrics, fr_auc_sorted).  'gauc' is a ranking
metric: it reads `rec.meanrank` (fr_eval_meanrank_segments) in the full / uniN / popN modes.
"""
from __future__ import annotations

from logging import getLogger
from typing import Dict, Iterable, Optional

import numpy as np
import torch

from .. import _C
from .groups import attribute_groups, group_segments, item_segments

TOPK_NAMES = ("hit", "mrr", "ndcg", "recall", "precision", "map")
EXPOSURE_NAMES = ("giniindex", "itemcoverage", "shannonentropy", "popularitypercentage", "tailpercentage", "averagepopularity")
EXPOSURE_MAX_K = 8     # cut-offs per fr_exposure_grouped call
NARROW_GROUPS = 8      # fr_group_sums / fr_fair_metrics_from_stats keep a segment's per-group sums in registers: n_groups <= 8


def topk_metrics(rec_topk: torch.Tensor, topk: Iterable[int]) -> Dict[str, float]:
    rec = rec_topk.to(torch.int32).contiguous()
    U, K = rec.shape[0], rec.shape[1] - 1
    out = torch.empty(6 * K, dtype=torch.float64, device=rec.device)
    _C.call('topk_metrics', rec.data_ptr(), U, K, out.data_ptr(), ws=(U, K), device=rec.device)
    vals = out.view(6, K).cpu()
    return {f"{name}@{k}": float(vals[m, k - 1]) for m, name in enumerate(TOPK_NAMES) for k in topk}


def _group_sums(perm: Optional[torch.Tensor], seg_start, K, group, value, wtrue, G):
    """stats [K, G, 3] of fr_group_sums over the K segments of `perm` (None: the rows as they are)"""
    value = value.contiguous()
    stats = torch.empty((K, G, 3), dtype=torch.float64, device=value.device)
    _C.call('group_sums', _C.ptr(perm), seg_start.data_ptr(), K, group.data_ptr(), value.data_ptr(), _C.ptr(wtrue), G, stats.data_ptr())
    return stats


def _item_sort(items: torch.Tensor):
    """the members sorted by item, stably: (perm, seg_start int64 [K + 1], K); item k's members are perm[seg_start[k] .. seg_start[k + 1])"""
    keys, perm = torch.sort(items, stable=True)
    K, seg_start = item_segments(keys)
    return perm, seg_start, K


def _item_sums(items: Optional[torch.Tensor], group, value, wtrue, G):
    """stats [K, G, 3] over the distinct items (items = None: one segment), and K"""
    if items is None:
        return _group_sums(None, torch.tensor([0, value.numel()], dtype=torch.int64, device=value.device), 1, group, value, wtrue, G), 1
    perm, seg_start, K = _item_sort(items)
    return _group_sums(perm, seg_start, K, group, value, wtrue, G), K


def _from_stats(stats, K, G):
    out = torch.empty(5, dtype=torch.float64, device=stats.device)
    _C.call('fair_metrics_from_stats', stats.data_ptr(), K, G, out.data_ptr(), ws=(K,), ws_of='fair_metrics',
            device=stats.device)
    return out.cpu()


def _group_means_wide(gidx, value, G):
    """the G group means for G > NARROW_GROUPS, from fr_group_sums with the roles swapped: the GROUPS are its segments, every
    member sits in its one group 0."""
    perm, seg_start = group_segments(gidx, G)
    zero = torch.zeros(value.numel(), dtype=torch.int32, device=value.device)
    stats = _group_sums(perm, seg_start, G, zero, value, None, 1)
    return (stats[:, 0, 0] / stats[:, 0, 1]).cpu()


def _df_wide(items, gidx, value, G):
    """DifferentialFairness for G > NARROW_GROUPS: ONE stable sort of the key item * G + group, the item boundaries from the
    sorted keys, then fr_df_cells walks the (item, group) cells -- no [items, G] table.  The members are handed over in sorted
    order (perm = NULL), so the walk reads its two columns front to back."""
    skey, perm = torch.sort(items.to(torch.int64) * G + gidx.to(torch.int64), stable=True)
    item_of = torch.div(skey, G, rounding_mode='floor')
    K, item_start = item_segments(item_of)
    group = (skey - item_of * G).to(torch.int32)
    val = value[perm].contiguous()
    out = torch.empty(1, dtype=torch.float64, device=value.device)
    _C.call('df_cells', 0, item_start.data_ptr(), K, group.data_ptr(), val.data_ptr(), G, out.data_ptr(), ws=(K,), device=value.device)
    return float(out.cpu()[0])


def _nonparity_and_df(res, name, G, gidx, pos_score, pos_i):
    """the two metrics every attribute (and every intersection of attributes) gets; the path is chosen by G"""
    if G <= NARROW_GROUPS:
        # NonParity (metrics.py:864-882): |difference| of the two group means, population std for more groups
        st, _ = _item_sums(None, gidx, pos_score, None, G)
        means = (st[0, :, 0] / st[0, :, 1]).cpu()
        res[f'NonParity Unfairness of sensitive attribute {name}'] = float(
            (means[0] - means[1]).abs() if G == 2 else means.std(unbiased=False))
        st, K = _item_sums(pos_i, gidx, pos_score, None, G)
        res[f'Differential Fairness of sensitive attribute {name}'] = float(_from_stats(st, K, G)[4])
    else:
        means = _group_means_wide(gidx, pos_score, G)
        res[f'NonParity Unfairness of sensitive attribute {name}'] = float(means.std(unbiased=False))
        res[f'Differential Fairness of sensitive attribute {name}'] = _df_wide(pos_i, gidx, pos_score, G)


def fairness_metrics(pos_score, pos_i, sst: Dict[str, torch.Tensor], neg_score=None, neg_i=None, mode="full",
                     value_type=True, intersections=None) -> Dict[str, float]:
    """NonParity + DifferentialFairness per attribute, any number of values; Value / Absolute / Under / Over unfairness on the
    FIRST attribute (as the reference's classes read `sst_attr_list[0]`, metrics.py:905), which has to be binary.
    `intersections`: lists of attribute names out of `sst`; each adds NonParity + DifferentialFairness 'of sensitive attribute
    a&b', whose groups are the distinct value tuples present among the rows (groups.attribute_groups)."""
    res = {}
    pos_score = pos_score.to(torch.float32).contiguous()
    for n, (name, index, G, _) in enumerate(attribute_groups(sst, intersections)):
        gidx = index.to(torch.int32).contiguous()
        _nonparity_and_df(res, name, G, gidx, pos_score, pos_i)
        if n == 0 and value_type:
            if G != 2:
                raise ValueError('sensitive attribute must be binary')
            items, group, value, wtrue, _ = value_type_rows(pos_score, pos_i, gidx, None, neg_score, neg_i, mode)
            st, K = _item_sums(items, group.contiguous(), value.contiguous(), wtrue.contiguous(), 2)
            v = _from_stats(st, K, 2)
            for q, label in enumerate(("Value", "Absolute", "Underestimation", "Overestimation")):
                res[f'{label} Unfairness of sensitive attribute {name}'] = float(v[q])
    return res


def gini_index(rec_items: torch.Tensor, num_items: int, topk) -> Dict[str, float]:
    """GiniIndex@k (metrics.py:638-662) of the item exposure in the top-k lists: counts by bincount, no host loop."""
    res = {}
    for k in topk:
        cnt = torch.bincount(rec_items[:, :k].reshape(-1), minlength=num_items)
        cnt = torch.sort(cnt[cnt > 0]).values.to(torch.float64)
        idx = torch.arange(num_items - cnt.numel() + 1, num_items + 1, device=cnt.device, dtype=torch.float64)
        res[f'giniindex@{k}'] = float(((2 * idx - num_items - 1) * cnt).sum() / (rec_items.shape[0] * k) / num_items)
    return res


def _popular_mask(count_items: torch.Tensor, popularity_ratio=None) -> torch.Tensor:
    """bool [items]: the popular items of PopularityPercentage (see popularity_percentage)"""
    ratio = 0.1 if popularity_ratio is None or popularity_ratio <= 0 else popularity_ratio
    present = torch.nonzero(count_items > 0).view(-1)
    if ratio > 1:
        return count_items >= ratio
    cnt = count_items[present]
    order = torch.sort(cnt * (count_items.numel() + 1) + present, descending=True).indices   # (count, id) descending
    popular = torch.zeros_like(count_items, dtype=torch.bool)
    popular[present[order[:max(int(present.numel() * ratio), 1)]]] = True
    return popular


def _tail_mask(count_items: torch.Tensor, tail_ratio=None) -> torch.Tensor:
    """bool [items]: the long-tail items of TailPercentage (see tail_percentage)"""
    ratio = 0.1 if tail_ratio is None or tail_ratio <= 0 else tail_ratio
    present = torch.nonzero(count_items > 0).view(-1)
    tail = torch.zeros_like(count_items, dtype=torch.bool)
    if ratio > 1:
        tail[present[count_items[present] <= ratio]] = True
    else:
        order = torch.sort(count_items[present] * (count_items.numel() + 1) + present).indices       # (count, id) ascending
        tail[present[order[:max(int(present.numel() * ratio), 1)]]] = True
    return tail


def popularity_percentage(rec_items: torch.Tensor, count_items: torch.Tensor, topk, popularity_ratio=None) -> Dict[str, float]:
    """PopularityPercentage@k (metrics.py:749-821): popular = top `ratio` fraction of the items that occur in training,
    ordered by (count, id) descending, or the items with count >= ratio when ratio > 1."""
    hit = _popular_mask(count_items, popularity_ratio)[rec_items].to(torch.float64)
    avg = (hit.cumsum(dim=1) / torch.arange(1, hit.shape[1] + 1, device=hit.device, dtype=torch.float64)).mean(dim=0).cpu()
    return {f'popularitypercentage@{k}': float(avg[k - 1]) for k in topk}


def _mean_at_k(values: torch.Tensor, name: str, topk) -> Dict[str, float]:
    """mean over users of cumsum(values)[:k] / k (the `metric_info` / `topk_result` pair of the exposure metrics)."""
    v = values.to(torch.float64)
    avg = (v.cumsum(dim=1) / torch.arange(1, v.shape[1] + 1, device=v.device, dtype=torch.float64)).mean(dim=0).cpu()
    return {f'{name}@{k}': float(avg[k - 1]) for k in topk}


def item_coverage(rec_items, num_items, topk) -> Dict[str, float]:
    """ItemCoverage@k (metrics.py:438-482): distinct recommended items / catalogue size."""
    return {f'itemcoverage@{k}': float(torch.unique(rec_items[:, :k]).numel() / num_items) for k in topk}


def average_popularity(rec_items, count_items, topk) -> Dict[str, float]:
    """AveragePopularity@k (metrics.py:484-551): mean training popularity of the recommended items."""
    return _mean_at_k(count_items[rec_items], 'averagepopularity', topk)


def shannon_entropy(rec_items, topk) -> Dict[str, float]:
    """ShannonEntropy@k (metrics.py:553-606): -sum p log p over the recommended items, divided by their number (as the
    reference does)."""
    res = {}
    for k in topk:
        cnt = torch.unique(rec_items[:, :k], return_counts=True)[1].to(torch.float64)
        p = cnt / (rec_items.shape[0] * k)
        res[f'shannonentropy@{k}'] = float((-p * torch.log(p)).sum() / cnt.numel())
    return res


def tail_percentage(rec_items, count_items, topk, tail_ratio=None) -> Dict[str, float]:
    """TailPercentage@k (metrics.py:664-747): share of long-tail items; tail = the bottom `ratio` fraction of the items
    that occur in training ordered by (count, id) ascending, or the items with count <= ratio when ratio > 1."""
    return _mean_at_k(_tail_mask(count_items, tail_ratio)[rec_items], 'tailpercentage', topk)


def value_metrics(score: torch.Tensor, label: torch.Tensor, names: Iterable[str]) -> Dict[str, float]:
    """metrics.py AUC / LogLoss / MAE / RMSE over the concatenated (score, label) columns.  The sums and the AUC's integer
    counts come from the device (one pass each; the AUC after ONE torch.sort of the score column), the last division and
    square root are float64 on the host.  AUC without a positive or without a negative row: nan and a warning."""
    names = [n.lower() for n in names]
    score = score.reshape(-1).to(torch.float32).contiguous()
    label = label.reshape(-1).to(torch.float32).contiguous()
    n, dev = score.numel(), score.device
    if label.numel() != n or n < 1:
        raise ValueError(f'value metrics need as many labels as scores and at least one row (got {n} scores, {label.numel()} labels)')
    if n >= 2 ** 31:
        raise ValueError(f'value metrics: {n} rows; the device path takes fewer than 2^31')
    res = {}
    if {'logloss', 'mae', 'rmse'} & set(names):
        out = torch.empty(3, dtype=torch.float64, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        _C.call('value_metrics', score.data_ptr(), label.data_ptr(), n, out.data_ptr(), counts.data_ptr(), ws=(n,), device=dev)
        sums = out.cpu().tolist()
        res['mae'] = sums[0] / n
        res['rmse'] = (sums[1] / n) ** 0.5
        res['logloss'] = sums[2] / n
    if 'auc' in names:
        srt, order = torch.sort(score)
        out = torch.empty(3, dtype=torch.int64, device=dev)
        by_score = label[order].contiguous()     # (named: it has to outlive the call's workspace allocation)
        _C.call('auc_sorted', srt.data_ptr(), by_score.data_ptr(), n, out.data_ptr(), ws=(n,), device=dev)
        two_u, P, Nn = out.cpu().tolist()
        if P == 0 or Nn == 0:
            getLogger().warning('AUC: the evaluation set has no %s row (label %s 1); the result is nan',
                                'positive' if P == 0 else 'negative', '==' if P == 0 else '!=')
            res['auc'] = float('nan')
        else:
            res['auc'] = two_u / (2 * P * Nn)          # Python integers: the one division is exact-to-rounding float64
    return {m: res[m] for m in names}


def gauc(meanrank: torch.Tensor) -> float:
    """metrics.py GAUC from `rec.meanrank` int64 [users, 3] = [2 * pos_rank_sum, user_len, pos_len]: users without a positive
    or without a negative are dropped (a warning each kind), the rest averaged weighted by pos_len, in float64."""
    t = meanrank.cpu()
    two_rank, user_len, pos_len = t[:, 0].to(torch.float64), t[:, 1].to(torch.float64), t[:, 2].to(torch.float64)
    no_pos, no_neg = pos_len == 0, (user_len == pos_len) & (pos_len != 0)
    if bool(no_pos.any()):
        getLogger().warning('No positive samples in some users, true positive value should be meaningless, '
                            'these users have been removed from GAUC calculation')
    if bool(no_neg.any()):
        getLogger().warning('No negative samples in some users, false positive value should be meaningless, '
                            'these users have been removed from GAUC calculation')
    keep = ~(no_pos | no_neg)
    two_rank, user_len, pos_len = two_rank[keep], user_len[keep], pos_len[keep]
    if not pos_len.numel():
        return float('nan')
    pair = (user_len + 1) * pos_len - pos_len * (pos_len + 1) / 2 - two_rank / 2
    auc_u = pair / ((user_len - pos_len) * pos_len)
    return float((auc_u * pos_len).sum() / pos_len.sum())


def group_topk_metrics(rec_topk: torch.Tensor, group_index: torch.Tensor, n_groups: int, topk: Iterable[int]):
    """`topk_metrics` per group of users: {'<name>@<k>': [n_groups values]}.  group_index[u] in [0, n_groups) is the group of row
    u of `rec_topk`; one launch chain for all groups (fr_topk_metrics_grouped), no host read of the group sizes."""
    rec = rec_topk.to(torch.int32).contiguous()
    U, K = rec.shape[0], rec.shape[1] - 1
    if group_index.numel() != U:
        raise ValueError(f'group_topk_metrics: {group_index.numel()} group indices for {U} rows')
    perm, start = group_segments(group_index, n_groups)
    out = torch.empty(n_groups * 6 * K, dtype=torch.float64, device=rec.device)
    _C.call('topk_metrics_grouped', rec.data_ptr(), perm.data_ptr(), start.data_ptr(), U, K, n_groups, out.data_ptr(),
            ws=(U, K, n_groups), device=rec.device)
    vals = out.view(n_groups, 6, K).cpu()
    return {f"{name}@{k}": [float(vals[g, m, k - 1]) for g in range(n_groups)] for m, name in enumerate(TOPK_NAMES) for k in topk}


def group_gauc(meanrank: torch.Tensor, group_index: torch.Tensor, n_groups: int):
    """`gauc` per group of users from `rec.meanrank`: [n_groups values], NaN for a group whose users are all dropped
    (fr_gauc_grouped: the two sums per group on the device, the one quotient in float64 on the host)."""
    mr = meanrank.to(torch.int64).contiguous()
    U = mr.shape[0]
    if group_index.numel() != U:
        raise ValueError(f'group_gauc: {group_index.numel()} group indices for {U} rows')
    perm, start = group_segments(group_index, n_groups)
    out = torch.empty((n_groups, 2), dtype=torch.float64, device=mr.device)
    kept = torch.empty((n_groups, 3), dtype=torch.int64, device=mr.device)
    _C.call('gauc_grouped', mr.data_ptr(), perm.data_ptr(), start.data_ptr(), U, n_groups, out.data_ptr(), kept.data_ptr(),
            ws=(U, n_groups), device=mr.device)
    return [s / w if w > 0 else float('nan') for s, w in out.cpu().tolist()]


def group_value_metrics(score: torch.Tensor, label: torch.Tensor, group_index: torch.Tensor, n_groups: int, names: Iterable[str]):
    """`value_metrics` per group of rows: {'<name>': [n_groups values]}.  The rows are sorted by group once; every group's
    contiguous slice goes through the kernels of `value_metrics`.  A group with one label class: AUC NaN; an empty group: NaN."""
    names = [n.lower() for n in names]
    score, label = score.reshape(-1), label.reshape(-1)
    perm, start = group_segments(group_index, n_groups)
    score, label = score[perm], label[perm]
    bounds = start.cpu().tolist()
    res = {n: [] for n in names}
    for g in range(n_groups):
        lo, hi = bounds[g], bounds[g + 1]
        one = value_metrics(score[lo:hi], label[lo:hi], names) if hi > lo else {n: float('nan') for n in names}
        for n in names:
            res[n].append(one[n])
    return res


def group_exposure_metrics(rec_items: torch.Tensor, group_index: torch.Tensor, n_groups: int, num_items: int, count_items,
                           topk: Iterable[int], names: Iterable[str], popularity_ratio=None, tail_ratio=None):
    """The exposure metrics of `names` per group of users: {'<name>@<k>': [n_groups values]}, what gini_index, item_coverage,
    shannon_entropy, popularity_percentage, tail_percentage and average_popularity give on each group's rows of `rec_items`.
    group_index[u] in [0, n_groups) is the group of row u.  ONE sort of the keys (group * num_items + item) * K + rank, then one
    library call for every group, metric and k (fr_exposure_grouped; up to EXPOSURE_MAX_K cut-offs a call): exact integer sums
    and the entropy sum per (group, k), finished in float64 on the host with the operations of the ungrouped functions.  No host
    read of the group sizes for the launch; memory is O(list entries).  An empty group: NaN everywhere."""
    names = [n.lower() for n in names]
    stranger = [n for n in names if n not in EXPOSURE_NAMES]
    if stranger:
        raise ValueError(f'group_exposure_metrics: {stranger} are no exposure metrics {EXPOSURE_NAMES}')
    items = rec_items.to(torch.int64)
    U, K = items.shape
    G, N = int(n_groups), int(num_items)
    if group_index.numel() != U:
        raise ValueError(f'group_exposure_metrics: {group_index.numel()} group indices for {U} rows')
    if G * N * K >= 2 ** 63:
        raise ValueError(f'group_exposure_metrics: {G} groups x {N} items x {K} ranks do not fit the int64 sort key')
    dev = items.device
    gidx = group_index.reshape(-1).to(torch.int64)
    keys = torch.sort((((gidx[:, None] * N + items) * K) + torch.arange(K, device=dev, dtype=torch.int64)).reshape(-1)).values
    _, start = group_segments(gidx, G, perm=False)
    popular = _popular_mask(count_items, popularity_ratio).to(torch.uint8).contiguous() if 'popularitypercentage' in names else None
    tail = _tail_mask(count_items, tail_ratio).to(torch.uint8).contiguous() if 'tailpercentage' in names else None
    counts = count_items.to(torch.int64).contiguous() if 'averagepopularity' in names else None
    ks = sorted(set(int(k) for k in topk))
    sums, entropy = {}, {}
    for lo in range(0, len(ks), EXPOSURE_MAX_K):
        part = ks[lo:lo + EXPOSURE_MAX_K]
        n_k = len(part)
        out_i = torch.empty((G, n_k, 5), dtype=torch.int64, device=dev)
        out_e = torch.empty((G, n_k), dtype=torch.float64, device=dev)
        _C.call('exposure_grouped', keys.data_ptr(), U * K, N, K, start.data_ptr(), G, (_C.c_int32 * n_k)(*part), n_k,
                _C.ptr(popular), _C.ptr(tail), _C.ptr(counts), out_i.data_ptr(), out_e.data_ptr(), ws=(U, K, G, n_k), device=dev)
        out_i, out_e = out_i.cpu().tolist(), out_e.cpu().tolist()
        for j, k in enumerate(part):
            sums[k] = [out_i[g][j] for g in range(G)]
            entropy[k] = [out_e[g][j] for g in range(G)]
    bounds = start.cpu().tolist()
    nan = float('nan')
    res = {}
    for name in names:
        for k in topk:
            vals = []
            for g in range(G):
                n_g = bounds[g + 1] - bounds[g]
                m, S, pop, tl, cnt = sums[int(k)][g]
                if n_g == 0:
                    vals.append(nan)
                elif name == 'giniindex':
                    vals.append(float(S) / float(n_g * k) / N)
                elif name == 'itemcoverage':
                    vals.append(m / N)
                elif name == 'shannonentropy':
                    vals.append(entropy[int(k)][g] / m if m else nan)
                else:       # Python integers: the one division is correctly rounded
                    vals.append({'popularitypercentage': pop, 'tailpercentage': tl, 'averagepopularity': cnt}[name] / (n_g * k))
            res[f'{name}@{k}'] = vals
    return res


def topk_user_terms(rec_topk: torch.Tensor, columns) -> torch.Tensor:
    """double [U, C] on the device: column j = every row's own term of top-k metric columns[j][0] (a name out of TOPK_NAMES) at
    cut-off columns[j][1] -- what `topk_metrics` averages over the rows, the same bits (fr_topk_user_terms)."""
    rec = rec_topk.to(torch.int32).contiguous()
    U, K = rec.shape[0], rec.shape[1] - 1
    columns = [(str(m).lower(), int(k)) for m, k in columns]
    bad = [c for c in columns if c[0] not in TOPK_NAMES or not 1 <= c[1] <= K]
    if bad or not columns:
        raise ValueError(f'topk_user_terms: columns {bad} are not (name out of {TOPK_NAMES}, cut-off in 1..{K}) pairs')
    parts = []
    for lo in range(0, len(columns), _C.BOOTSTRAP_MAX_COLS):
        part = columns[lo:lo + _C.BOOTSTRAP_MAX_COLS]
        n = len(part)
        out = torch.empty((U, n), dtype=torch.float64, device=rec.device)
        _C.call('topk_user_terms', rec.data_ptr(), U, K, (_C.c_int32 * n)(*[TOPK_NAMES.index(m) for m, _ in part]),
                (_C.c_int32 * n)(*[k for _, k in part]), n, out.data_ptr())
        parts.append(out)
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)


def gauc_user_terms(meanrank: torch.Tensor) -> torch.Tensor:
    """double [U, 2] on the device: (auc_u * pos_len, pos_len) of every user `gauc` keeps, (0, 0) of a dropped one
    (fr_gauc_user_terms); GAUC of a set of users = the quotient of the two column sums."""
    mr = meanrank.to(torch.int64).contiguous()
    out = torch.empty((mr.shape[0], 2), dtype=torch.float64, device=mr.device)
    _C.call('gauc_user_terms', mr.data_ptr(), mr.shape[0], out.data_ptr())
    return out


def bootstrap_group_sums(values: torch.Tensor, group_index: torch.Tensor, n_groups: int, n_rep: int, seed: int):
    """Poisson bootstrap over the rows of `values` (double [U, C] on the device): (sums double [G, B, C], weight int64 [G, B]),
    sums[g, b, c] = sum over group g's rows r of w(r, b) * values[r, c], weight[g, b] = their sum of w(r, b); w(r, b) ~ Poisson(1)
    from Philox by the contract of fairrec_hip.h, a function of (row index, replicate, seed) alone: the same replicates under
    every grouping.  fr_bootstrap_group_sums makes the weights in registers, never in memory; more than 64 columns go through
    several calls."""
    if values.dim() != 2 or values.dtype != torch.float64:
        raise ValueError(f'bootstrap_group_sums: values must be a float64 [rows, columns] tensor, not {values.dtype} {tuple(values.shape)}')
    values = values.contiguous()
    U, C = values.shape
    G, B = int(n_groups), int(n_rep)
    if group_index.numel() != U:
        raise ValueError(f'bootstrap_group_sums: {group_index.numel()} group indices for {U} rows')
    if not 1 <= B <= _C.BOOTSTRAP_MAX_REP or C < 1:
        raise ValueError(f'bootstrap_group_sums: {B} replicates of {C} columns; 1..{_C.BOOTSTRAP_MAX_REP} replicates, at least one column')
    perm, start = group_segments(group_index, G)
    dev = values.device
    weight = torch.empty((G, B), dtype=torch.int64, device=dev)
    parts = []
    for lo in range(0, C, _C.BOOTSTRAP_MAX_COLS):
        n = min(C - lo, _C.BOOTSTRAP_MAX_COLS)
        sums = torch.empty((G, B, n), dtype=torch.float64, device=dev)
        _C.call('bootstrap_group_sums', values.data_ptr() + lo * 8, U, n, C, perm.data_ptr(), start.data_ptr(), G, B,
                int(seed) & (2 ** 64 - 1), sums.data_ptr(), weight.data_ptr(), ws=(U, n, G, B), device=dev)
        parts.append(sums)
    return (parts[0] if len(parts) == 1 else torch.cat(parts, dim=2)), weight


FAIR_STATS = ("value", "absolute", "under", "over", "differential")     # the rows of fr_bootstrap_fair_metrics' out_terms


def value_type_rows(pos_score, pos_i, gidx, unit, neg_score=None, neg_i=None, mode="full"):
    """the rows the value-type metrics of `fairness_metrics` are taken over: (items, group, value, wtrue, unit).  Outside the
    `full` mode the first min(len(neg), P) negatives follow the P positives with wtrue 0; negative j carries the group and the
    resampling unit of positive j (metrics.py:957-960).  unit = None (the point estimate): None."""
    P = pos_score.numel()
    ones = torch.ones(P, dtype=torch.float32, device=pos_score.device)
    if mode == 'full' or neg_i is None:
        return pos_i, gidx, pos_score, ones, unit
    m = min(neg_i.numel(), P)
    return (torch.cat([pos_i, neg_i[:m]]), torch.cat([gidx, gidx[:m]]), torch.cat([pos_score, neg_score[:m].to(torch.float32)]),
            torch.cat([ones, torch.zeros(m, dtype=torch.float32, device=ones.device)]),
            None if unit is None else torch.cat([unit, unit[:m]]))


def bootstrap_fairness(items, group, value, wtrue, unit, n_groups: int, n_rep: int, seed: int, value_type=False,
                       differential=True, sort=None):
    """The fairness metrics of the rows (items, group, value, wtrue) -- what `fairness_metrics` forms -- in every one of n_rep
    replicates of a Poisson bootstrap over users: member j occurs w(unit[j], b) times in replicate b, w the weights of
    `bootstrap_group_sums` (fairrec_hip.h), unit[j] = the global row of the member's user in the evaluation.  -> {name: float64
    [n_rep] on the host}: 'nonparity' (|difference| of the two weighted group means, the population std for more groups; NaN when
    a group has weight 0), with value_type (two groups) 'value', 'absolute', 'under', 'over', with differential 'differential'
    (means over the K_b items present in the replicate, alpha = 1 / K_b; NaN when K_b = 0), and 'items' = K_b (int64).
    One library call (fr_bootstrap_fair_metrics): no weight and no per-replicate table is stored.  `sort`: what `_item_sort(items)`
    returned, when the caller has it.  1 <= n_groups <= NARROW_GROUPS."""
    G, B = int(n_groups), int(n_rep)
    M = items.numel()
    if not 1 <= G <= NARROW_GROUPS:
        raise ValueError(f'bootstrap_fairness: {G} groups; the device path takes 1..{NARROW_GROUPS}')
    if not 1 <= B <= _C.BOOTSTRAP_MAX_REP:
        raise ValueError(f'bootstrap_fairness: {B} replicates; 1..{_C.BOOTSTRAP_MAX_REP}')
    if value_type and G != 2:
        raise ValueError('sensitive attribute must be binary')
    if M < 1 or any(t.numel() != M for t in (group, value, unit)) or (wtrue is not None and wtrue.numel() != M):
        raise ValueError(f'bootstrap_fairness: {M} items need as many groups, values, units (and wtrue), and at least one')
    dev = value.device
    perm, seg_start, K = sort if sort is not None else _item_sort(items)
    group = group.to(torch.int32).contiguous()
    value = value.to(torch.float32).contiguous()
    wtrue = None if wtrue is None else wtrue.to(torch.float32).contiguous()
    unit = unit.to(torch.int64).contiguous()
    terms = torch.empty((5, B), dtype=torch.float64, device=dev)
    n_items = torch.empty(B, dtype=torch.int64, device=dev)
    gsum = torch.empty((G, B), dtype=torch.float64, device=dev)
    gweight = torch.empty((G, B), dtype=torch.int64, device=dev)
    want = (_C.FAIR_WANT_VALUE if value_type else 0) | (_C.FAIR_WANT_DF if differential else 0)
    _C.call('bootstrap_fair_metrics', perm.data_ptr(), seg_start.data_ptr(), K, M, group.data_ptr(), value.data_ptr(), _C.ptr(wtrue),
            unit.data_ptr(), G, B, int(seed) & (2 ** 64 - 1), want, terms.data_ptr(), n_items.data_ptr(), gsum.data_ptr(),
            gweight.data_ptr(), ws=(M, K, G, B), device=dev)
    terms, n_items = terms.cpu().numpy(), n_items.cpu().numpy()
    means = _ratio(gsum.cpu().numpy(), gweight.cpu().numpy())                       # [G, B], NaN where a group has weight 0
    res = {'items': n_items, 'nonparity': np.abs(means[0] - means[1]) if G == 2 else means.std(axis=0)}
    for q, name in enumerate(FAIR_STATS):
        if (value_type and q < 4) or (differential and q == 4):
            res[name] = _ratio(terms[q], n_items)
    return res


def bootstrap_intervals(stat, level: float, what: str = ''):
    """Percentile intervals of bootstrap replicates.  stat: float64 [G, B] on the host, the statistic of group g in replicate b,
    NaN (or infinite) = unusable.  -> (low [G], high [G], gap_low, gap_high, usable [G], gap_usable): per group
    np.quantile(its usable values, [(1 - level) / 2, (1 + level) / 2]); the gap of a replicate is max_g - min_g, usable when every
    group's value is; `usable` counts them.  Fewer usable replicates than B / 2: a NaN interval and one warning (`what` names
    the attribute and the metric in it)."""
    stat = np.asarray(stat, dtype=np.float64)
    G, B = stat.shape
    q = [(1.0 - level) / 2.0, (1.0 + level) / 2.0]
    ok = np.isfinite(stat)
    usable = ok.sum(axis=1)
    low, high = np.full(G, np.nan), np.full(G, np.nan)
    for g in range(G):
        if 2 * usable[g] >= B:
            low[g], high[g] = np.quantile(stat[g][ok[g]], q)
    every = ok.all(axis=0)
    gap_usable = int(every.sum())
    gap_low = gap_high = float('nan')
    if 2 * gap_usable >= B:
        cols = stat[:, every]
        gap_low, gap_high = (float(x) for x in np.quantile(cols.max(axis=0) - cols.min(axis=0), q))
    starved = [f'group {g} ({int(usable[g])})' for g in range(G) if 2 * usable[g] < B]
    if 2 * gap_usable < B:
        starved.append(f'the gap ({gap_usable})')
    if starved:
        getLogger().warning('bootstrap intervals of %s: fewer than half of the %d replicates are usable for %s; these intervals '
                            'are nan', what or 'a statistic', B, ', '.join(starved))
    return low, high, gap_low, gap_high, usable, gap_usable


def _ratio(num, den):
    """num / den on the host, NaN where the denominator is zero"""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(den != 0, num / np.where(den != 0, den, 1.0), np.nan)


class Evaluator:
    """recbole/evaluator/evaluator.py: metric names from `config['metrics']` -> one result dict."""

    TOPK = frozenset(TOPK_NAMES)
    EXPOSURE = frozenset(EXPOSURE_NAMES)
    # the ungrouped exposure metrics in the order of their result keys: name -> function of (collected, topk, config)
    UNGROUPED_EXPOSURE = {
        "giniindex": lambda c, topk, cfg: gini_index(c['rec.items'], c['data.num_items'], topk),
        "popularitypercentage": lambda c, topk, cfg: popularity_percentage(c['rec.items'], c['data.count_items'], topk,
                                                                          cfg['popularity_ratio']),
        "itemcoverage": lambda c, topk, cfg: item_coverage(c['rec.items'], c['data.num_items'], topk),
        "averagepopularity": lambda c, topk, cfg: average_popularity(c['rec.items'], c['data.count_items'], topk),
        "shannonentropy": lambda c, topk, cfg: shannon_entropy(c['rec.items'], topk),
        "tailpercentage": lambda c, topk, cfg: tail_percentage(c['rec.items'], c['data.count_items'], topk, cfg['tail_ratio']),
    }
    # metric name -> the prefix of its keys among what fairness_metrics reports
    FAIR_PREFIX = {"nonparityunfairness": "NonParity", "valueunfairness": "Value Unfairness", "absoluteunfairness": "Absolute",
                   "underunfairness": "Underestimation", "overunfairness": "Overestimation", "differentialfairness": "Differential"}
    FAIR = frozenset(FAIR_PREFIX)
    RANKING = {"gauc"}                                   # reads `rec.meanrank`; a ranking-type metric in the reference too
    VALUE = {"auc", "logloss", "mae", "rmse"}            # evaluation by value: `eval_args.mode: labeled` only

    def __init__(self, config):
        self.config = config
        self.metrics = [m.lower() for m in (config['metrics'] or [])]
        self.topk = config['topk'] or [10]
        if isinstance(self.topk, int):
            self.topk = [self.topk]
        self.decimal_place = config['metric_decimal_place'] if config['metric_decimal_place'] is not None else 4
        self.mode = (config['eval_args'] or {}).get('mode', 'full')
        unknown = [m for m in self.metrics if m not in self.TOPK | self.FAIR | self.EXPOSURE | self.RANKING | self.VALUE]
        if unknown:
            raise NotImplementedError(f'metrics {unknown} are not on the device path')
        value = [m for m in self.metrics if m in self.VALUE]
        ranking = [m for m in self.metrics if m not in self.VALUE]
        if value and ranking:
            raise RuntimeError('Ranking metrics and value metrics can not be used at the same time.')
        if value and self.mode != 'labeled':
            raise ValueError(f"value metrics {value} need eval_args.mode 'labeled', not '{self.mode}'")
        if ranking and self.mode == 'labeled':
            raise ValueError(f"ranking metrics {ranking} need eval_args.mode full / uniN / popN, not 'labeled'")
        self.intersections = self._intersections(config['sst_intersections'], list(config['sst_attr_list'] or []))
        from .collector import utility_attrs
        self.utility = utility_attrs(config['utility_by_group'], list(config['sst_attr_list'] or []))
        self.exposure = utility_attrs(config['exposure_by_group'], list(config['sst_attr_list'] or []), 'exposure_by_group')
        if self.exposure and self.mode == 'labeled':
            raise ValueError("exposure_by_group needs eval_args.mode full / uniN / popN, not 'labeled': the exposure metrics "
                             "read the ranked lists")
        self.bootstrap, self.bootstrap_level = self._bootstrap_keys(config['group_bootstrap'], config['group_bootstrap_level'])
        if self.bootstrap and not self.utility:
            raise ValueError('group_bootstrap needs utility_by_group: the intervals belong to its per-group metrics')
        if self.bootstrap and self.mode == 'labeled':
            raise ValueError("group_bootstrap needs eval_args.mode full / uniN / popN, not 'labeled': the bootstrap resamples "
                             "users, and the rows of the labeled mode are interactions")
        self.fair_bootstrap, self.fair_bootstrap_level = self._bootstrap_keys(
            config['fairness_bootstrap'], config['fairness_bootstrap_level'], 'fairness_bootstrap')
        if self.fair_bootstrap and self.mode == 'labeled':
            raise ValueError("fairness_bootstrap needs eval_args.mode full / uniN / popN, not 'labeled': the bootstrap resamples "
                             "users, and the rows of the labeled mode are interactions")
        if self.fair_bootstrap and not self.FAIR & set(self.metrics):
            raise ValueError('fairness_bootstrap needs a fairness metric among `metrics`: the intervals belong to '
                             f'{sorted(self.FAIR)}')
        self.seed = int(config['seed']) if config['seed'] is not None else 0

    @staticmethod
    def _bootstrap_keys(n_rep, level, key='group_bootstrap'):
        """`group_bootstrap` / `fairness_bootstrap` (`key`: the name the error messages use; None / 0: off, else an integer B in
        2..65536) and its `<key>_level` (strictly inside 0..1)"""
        if n_rep is None or (not isinstance(n_rep, bool) and n_rep == 0):
            return 0, None
        if isinstance(n_rep, bool) or not isinstance(n_rep, int) or not 2 <= n_rep <= _C.BOOTSTRAP_MAX_REP:
            raise ValueError(f'{key} must be None, 0 or an integer in 2..{_C.BOOTSTRAP_MAX_REP}, not {n_rep!r}')
        level = 0.95 if level is None else level
        if isinstance(level, bool) or not isinstance(level, (int, float)) or not 0.0 < level < 1.0:
            raise ValueError(f'{key}_level must lie strictly between 0 and 1, not {level!r}')
        return int(n_rep), float(level)

    @staticmethod
    def _intersections(entries, attrs):
        """`sst_intersections`: a list of lists, each two or more distinct names out of `sst_attr_list`"""
        if entries is None:
            return []
        if not isinstance(entries, (list, tuple)):
            raise ValueError(f'sst_intersections must be a list of lists of attribute names, not {entries!r}')
        for e in entries:
            if not isinstance(e, (list, tuple)) or len(e) < 2 or not all(isinstance(n, str) for n in e):
                raise ValueError(f'sst_intersections: {e!r} is not a list of two or more attribute names')
            if len(set(e)) != len(e):
                raise ValueError(f'sst_intersections: {e!r} names an attribute twice')
            missing = [n for n in e if n not in attrs]
            if missing:
                raise ValueError(f'sst_intersections: {missing} not in sst_attr_list {attrs}')
        return [list(e) for e in entries]

    def evaluate(self, collected: Dict[str, torch.Tensor]) -> Dict[str, float]:
        res = {}
        if self.VALUE & set(self.metrics):
            res.update(value_metrics(collected['rec.score'], collected['data.label'],
                                     [m for m in self.metrics if m in self.VALUE]))
        if "gauc" in self.metrics:
            res['gauc'] = gauc(collected['rec.meanrank'])
        if self.TOPK & set(self.metrics):
            allk = topk_metrics(collected['rec.topk'], self.topk)
            res.update({k: v for k, v in allk.items() if k.split('@')[0] in self.metrics})
        for name, fn in self.UNGROUPED_EXPOSURE.items():
            if name in self.metrics:
                res.update(fn(collected, self.topk, self.config))
        if self.FAIR & set(self.metrics):
            sst = {s: collected['data.' + s] for s in self.config['sst_attr_list']}
            extra = {}
            if self.intersections and {"nonparityunfairness", "differentialfairness"} & set(self.metrics):
                extra['intersections'] = self.intersections
            fair = fairness_metrics(collected['rec.positive_score'], collected['data.positive_i'], sst,
                                    collected.get('rec.negative_score'), collected.get('data.negative_i'), self.mode,
                                    value_type=bool({"valueunfairness", "absoluteunfairness", "underunfairness",
                                                     "overunfairness"} & set(self.metrics)), **extra)
            reported = [k for k in fair if any(k.startswith(p) for m, p in self.FAIR_PREFIX.items() if m in self.metrics)]
            res.update({k: fair[k] for k in reported})
            if self.fair_bootstrap:
                res.update(self._fairness_intervals(collected, sst, extra.get('intersections'), reported))
        if self.utility:
            res.update(self._utility_by_group(collected))
        if self.exposure:
            res.update(self._exposure_by_group(collected))
        return {k: round(v, self.decimal_place) for k, v in res.items()}

    # metric name -> (the head of its result keys, its statistic among what bootstrap_fairness returns)
    FAIR_STAT = {"nonparityunfairness": ("NonParity Unfairness", "nonparity"), "valueunfairness": ("Value Unfairness", "value"),
                 "absoluteunfairness": ("Absolute Unfairness", "absolute"), "underunfairness": ("Underestimation Unfairness", "under"),
                 "overunfairness": ("Overestimation Unfairness", "over"), "differentialfairness": ("Differential Fairness", "differential")}

    def _fairness_intervals(self, collected, sst, intersections, reported) -> Dict[str, float]:
        """`fairness_bootstrap`: '<metric> ci_low | ci_high of sensitive attribute <A>' for every key of `reported` (the point
        estimates, whose order the new keys follow): the percentile interval of the metric over the replicates of the bootstrap
        over users.  One bootstrap_fairness call per attribute or intersection for NonParity and DifferentialFairness, one more
        on the first attribute for the value-type rows; the positives are sorted by item once.  More than NARROW_GROUPS groups:
        no interval keys and one warning."""
        B, seed = self.fair_bootstrap, self.seed
        pos_score = collected['rec.positive_score'].to(torch.float32).contiguous()
        pos_i, unit = collected['data.positive_i'], collected['data.positive_user']
        per_attr = [m for m in ("nonparityunfairness", "differentialfairness") if m in self.metrics]
        value_type = [m for m in ("valueunfairness", "absoluteunfairness", "underunfairness", "overunfairness") if m in self.metrics]
        sort = _item_sort(pos_i) if per_attr else None
        stats = {}
        for n, (name, index, G, _) in enumerate(attribute_groups(sst, intersections)):
            if G > NARROW_GROUPS:
                getLogger().warning('fairness_bootstrap: sensitive attribute %s has %d groups, more than the %d the bootstrap '
                                    'takes; it gets no ci_low / ci_high keys', name, G, NARROW_GROUPS)
                continue
            gidx = index.to(torch.int32).contiguous()
            found = {}
            if per_attr:
                found.update(bootstrap_fairness(pos_i, gidx, pos_score, None, unit, G, B, seed,
                                                differential="differentialfairness" in self.metrics, sort=sort))
            if n == 0 and value_type:
                rows = value_type_rows(pos_score, pos_i, gidx, unit, collected.get('rec.negative_score'),
                                       collected.get('data.negative_i'), self.mode)
                found.update({k: v for k, v in bootstrap_fairness(*rows, 2, B, seed, value_type=True, differential=False).items()
                              if k in ("value", "absolute", "under", "over")})
            for m in per_attr + (value_type if n == 0 else []):
                head, stat = self.FAIR_STAT[m]
                stats[f'{head} of sensitive attribute {name}'] = found[stat]
        res = {}
        for key in reported:
            if key in stats:
                low, high, _, _, _, _ = bootstrap_intervals(stats[key][None, :], self.fair_bootstrap_level, key)
                head, name = key.split(' of sensitive attribute ', 1)
                res[f'{head} ci_low of sensitive attribute {name}'] = float(low[0])
                res[f'{head} ci_high of sensitive attribute {name}'] = float(high[0])
        return res

    def _utility_by_group(self, collected) -> Dict[str, float]:
        """`utility_by_group`: every requested top-k / gauc / value metric per group of each selected attribute, and of each
        `sst_intersections` entry whose attributes are all selected: '<m> of <A>=<value>' per group, '<m> gap | std | min of
        sensitive attribute <A>' (max - min, population std, worst group; float64 on the host, NaN if a group is NaN)."""
        labeled = self.mode == 'labeled'
        res = {}
        boot = self._bootstrap_columns(collected) if self.bootstrap else None
        for name, gidx, G, labels in self._groups(collected, self.utility, 'data.' if labeled else 'data.user.'):
            by_group = {}
            if labeled:
                by_group.update(group_value_metrics(collected['rec.score'], collected['data.label'], gidx, G,
                                                    [m for m in self.metrics if m in self.VALUE]))
            if "gauc" in self.metrics:
                by_group['gauc'] = group_gauc(collected['rec.meanrank'], gidx, G)
            if self.TOPK & set(self.metrics):
                allk = group_topk_metrics(collected['rec.topk'], gidx, G, self.topk)
                by_group.update({k: v for k, v in allk.items() if k.split('@')[0] in self.metrics})
            self._report_groups(res, name, labels, by_group, ('gap', 'std', 'min'))
            if boot is not None:
                self._report_intervals(res, name, labels, gidx, G, *boot)
        return res

    def _bootstrap_columns(self, collected):
        """`group_bootstrap`: the per-user terms every attribute's bootstrap sums up, made once per evaluation -> (values double
        [U, C] on the device, {result metric: (its column, None) for a top-k metric -- the statistic is sum / weight --, or
        (numerator column, denominator column) for gauc})"""
        parts, stats, C = [], {}, 0
        columns = [(m, int(k)) for m in TOPK_NAMES if m in self.metrics for k in self.topk]
        if "gauc" in self.metrics:
            parts.append(gauc_user_terms(collected['rec.meanrank']))
            stats['gauc'] = (0, 1)
            C = 2
        if columns:
            parts.append(topk_user_terms(collected['rec.topk'], columns))
            stats.update({f'{m}@{k}': (C + j, None) for j, (m, k) in enumerate(columns)})
        if not parts:
            return None
        return (parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)).contiguous(), stats

    def _report_intervals(self, res, name, labels, gidx, G, values, stats):
        """'<m> ci_low | ci_high of <A>=<value>' and '<m> gap ci_low | ci_high of sensitive attribute <A>': the percentile
        intervals of `group_bootstrap` replicates of every group's metric and of max - min over the groups"""
        sums, weight = bootstrap_group_sums(values, gidx, G, self.bootstrap, self.seed)
        sums, weight = sums.cpu().numpy(), weight.cpu().numpy()
        for m, (num, den) in stats.items():
            stat = _ratio(sums[:, :, num], weight if den is None else sums[:, :, den])
            low, high, gap_low, gap_high, _, _ = bootstrap_intervals(stat, self.bootstrap_level, f'{m} of sensitive attribute {name}')
            for g, label in enumerate(labels):
                res[f'{m} ci_low of {name}={label}'] = float(low[g])
                res[f'{m} ci_high of {name}={label}'] = float(high[g])
            res[f'{m} gap ci_low of sensitive attribute {name}'] = gap_low
            res[f'{m} gap ci_high of sensitive attribute {name}'] = gap_high

    def _exposure_by_group(self, collected) -> Dict[str, float]:
        """`exposure_by_group`: every requested exposure metric and k per group of each selected attribute, and of each
        `sst_intersections` entry whose attributes are all selected, in the key form of `_utility_by_group`, and '<m>@<k> max of
        sensitive attribute <A>' as well (for most of these metrics the larger value is the worse one)."""
        names = [m for m in EXPOSURE_NAMES if m in self.metrics]
        res = {}
        for name, gidx, G, labels in self._groups(collected, self.exposure, 'data.user.'):
            by_group = group_exposure_metrics(collected['rec.items'], gidx, G, collected['data.num_items'],
                                              collected.get('data.count_items'), self.topk, names, self.config['popularity_ratio'],
                                              self.config['tail_ratio']) if names else {}
            self._report_groups(res, name, labels, by_group, ('gap', 'std', 'min', 'max'))
        return res

    def _groups(self, collected, selected, prefix):
        """the Groups (with value labels) of the `selected` attributes (columns `prefix + name`) and of every `sst_intersections`
        entry whose attributes are all selected"""
        return attribute_groups({name: collected[prefix + name] for name in selected},
                                [e for e in self.intersections if all(n in selected for n in e)], labels=True)

    @staticmethod
    def _report_groups(res, name, labels, by_group, summaries):
        """'<m> of <A>=<value>' per group and '<m> <summary> of sensitive attribute <A>': max - min, population std, the
        smallest, the largest group value; float64 on the host, NaN if a group is NaN"""
        for m, per_group in by_group.items():
            v = np.asarray(per_group, dtype=np.float64)
            for label, x in zip(labels, per_group):
                res[f'{m} of {name}={label}'] = float(x)
            for what in summaries:
                res[f'{m} {what} of sensitive attribute {name}'] = float(
                    {'gap': v.max() - v.min(), 'std': v.std(), 'min': v.min(), 'max': v.max()}[what])
        return res

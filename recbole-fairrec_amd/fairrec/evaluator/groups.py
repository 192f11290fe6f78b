"""Where the evaluator builds its groups: attribute columns -> group indices (attribute_groups), a group index -> segments of a
permutation (group_segments), sorted keys -> runs (item_segments).  Index plumbing in torch on the columns' device; nothing here
reads a value back to the host unless labels are asked for."""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional

import torch


class Group(NamedTuple):
    name: str                           # the attribute, or 'a&b' for an intersection
    index: torch.Tensor                 # int64 [rows]: the row's group, in [0, n_groups)
    n_groups: int
    labels: Optional[List[str]] = None  # the groups' value names ('a-value&b-value'), when asked for


def _value_name(v: float) -> str:
    return str(int(v)) if float(v).is_integer() else repr(float(v))


def attribute_groups(columns: Dict[str, torch.Tensor], intersections=(), labels=False) -> List[Group]:
    """One Group per attribute column, then one per entry of `intersections` (lists of names out of `columns`).  An attribute's
    group index is np.unique(column, return_inverse=True): the rank of the value among the values present.  An intersection's
    groups are the distinct tuples present among the rows, in sorted-tuple order; equal tuples of group indices <=> equal tuples of
    values.  `labels` costs one device-to-host copy per group set.  An attribute with one value is refused."""
    def rank(t, **kw):
        vals, inv = torch.unique(t, sorted=True, return_inverse=True, **kw)
        return vals, inv.reshape(-1)

    by_name, groups = {}, []
    for name, col in columns.items():
        vals, inv = rank(col.reshape(-1))
        names = [_value_name(v) for v in vals.cpu().tolist()] if labels else None
        by_name[name] = Group(name, inv, int(vals.numel()), names)
        groups.append(by_name[name])
    for names in intersections or ():
        tuples, inv = rank(torch.stack([by_name[n].index for n in names], dim=1), dim=0)
        joined = ['&'.join(by_name[n].labels[j] for n, j in zip(names, row)) for row in tuples.cpu().tolist()] if labels else None
        groups.append(Group('&'.join(names), inv, int(tuples.shape[0]), joined))
    for g in groups:
        if g.n_groups < 2:
            raise ValueError(f'there is only one value for {g.name} sensitive attribute')
    return groups


def group_segments(group_index: torch.Tensor, n_groups: int, perm=True):
    """Groups as segments: perm = a stable sort of the group index (every group's rows in ascending row order; None with
    perm=False), start = int64 [n_groups + 1], the zero-led cumulative bincount.  Both stay on the device."""
    gidx = group_index.reshape(-1).to(torch.int64)
    order = torch.sort(gidx, stable=True).indices.contiguous() if perm else None
    start = torch.zeros(n_groups + 1, dtype=torch.int64, device=gidx.device)
    torch.cumsum(torch.bincount(gidx, minlength=n_groups)[:n_groups], 0, out=start[1:])
    return order, start


def item_segments(sorted_keys: torch.Tensor):
    """The runs of equal values in `sorted_keys`: (K, start int64 [K + 1]), run k = positions start[k] .. start[k + 1])."""
    _, counts = torch.unique_consecutive(sorted_keys, return_counts=True)
    K = counts.numel()
    start = torch.zeros(K + 1, dtype=torch.int64, device=sorted_keys.device)
    torch.cumsum(counts, 0, out=start[1:])
    return K, start

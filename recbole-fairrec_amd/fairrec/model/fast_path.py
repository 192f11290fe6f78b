"""The small rules of "score every item for these users" and "rate these candidate negatives", each stated once; the models'
hooks (`full_sort_factors`, `full_sort_pair_mlp`, `dyn_neg_select`), utils/case_study.py and the Trainer ask here.  A rule
that answers wrongly sends a call down the dense path and moves no value beyond rounding, so none is restated elsewhere."""
import torch

from ..engine import GenericEngine


def config_choice(config, key, allowed, default, of='', lower=True):
    """The value of a config key that takes one of the names `allowed`: None reads as `default`, the case is folded unless
    `lower` is off, anything else raises.  `of`: ' of MODEL' where two models read one key differently."""
    value = config[key]
    name = default if value is None else (str(value).lower() if lower else value)
    if name not in allowed:
        raise ValueError(f'{key}{of} must be {" or ".join(allowed)}, not [{value}]')
    return name


def single_device_engine(model):
    """The model's engine when its tables lie whole on one device, else None: the fused kernels read a table in place, so the
    row-sharded and replicated engines take the generic path.  A row-sharded model answers before an engine is built."""
    if model.shard is not None:
        return None
    eng = model.hip_engine()
    return None if type(eng) is not GenericEngine else eng


def overrides_any(cls, base, names):
    """Does `cls` replace any of `base`'s methods `names`?  A fused path restates what those methods compute, so a subclass
    with one of its own is served by the dense path.  Each hook keeps its tuple of names beside it."""
    return any(getattr(cls, n) is not getattr(base, n) for n in names)


def drops_out(mlp):
    """Does a forward pass of this MLP draw a dropout pattern now?"""
    return mlp.training and float(mlp.dropout) > 0.0


def filtered_users(model, rows, sst_list, users_per_batch):
    """The user rows through the model's filters, `users_per_batch` rows at a time (None or 0: all at once) -- the filters'
    BatchNorm layers normalise by the statistics of the batch they are given, and these are the users of one predict() batch
    of the full-sort evaluation.  A model without filters (NFCF has no `filter_mode`) and an empty request: the rows as they are."""
    if getattr(model, 'filter_mode', 'none') == 'none' or not rows.shape[0]:
        return rows
    per = int(users_per_batch) if users_per_batch else rows.shape[0]
    return torch.cat([model._filter(rows[lo:lo + per], sst_list) for lo in range(0, rows.shape[0], per)])


def flushed(table, hyper):
    """The weight of a lazy table with every row brought up to the optimizer step: what a kernel that reads whole tables sees."""
    table.flush(hyper)
    return table.weight


def with_subset(predict, interaction, sst_list=None):
    """`model.predict` / `model.full_sort_predict` on a batch, with the attribute subset only where the caller has one."""
    return predict(interaction) if sst_list is None else predict(interaction, sst_list)


def full_sort_plan(model, interaction, sst_list=None, users_per_batch=None, ask=('factors', 'pair_mlp')):
    """Which path scores every item for the users of `interaction`, and with what: ('factors', the dict of
    `model.full_sort_factors`) for the fused score-and-select kernels, ('pair_mlp', the pieces of `model.full_sort_pair_mlp`)
    for the split scorer, or ('dense', None) for full_sort_predict / predict.  The hooks named in `ask` are asked in this
    order; a model without a hook, and a hook that answers None, pass the call on."""
    for kind in ask:
        hook = getattr(model, {'factors': 'full_sort_factors', 'pair_mlp': 'full_sort_pair_mlp'}[kind], None)
        answer = hook(interaction, sst_list, users_per_batch=users_per_batch) if hook is not None else None
        if answer is not None:
            return kind, answer
    return 'dense', None

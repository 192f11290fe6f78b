"""The leakage probe on a file `save_sst_embed` wrote: a dict with 'embedding' ([users, dim]) and one column per sensitive
attribute -- the attacker "trained afterwards" the file is saved for, run by the project's own fused probe."""
from __future__ import annotations

from typing import Dict

import torch


def probe_file(path, config) -> Dict[str, float]:
    """`probe_leakage` (fairrec/evaluator/leakage.py) of the embeddings in `path` against every attribute column stored next to
    them, in the file's order; the settings are the `leakage_probe_*` keys and `seed` of `config`."""
    from ..evaluator.leakage import probe_leakage
    stored = torch.load(path, weights_only=False)
    if not isinstance(stored, dict) or 'embedding' not in stored:
        raise ValueError(f"{path}: not a file save_sst_embed wrote (a dict with 'embedding' and one column per attribute)")
    labels = {k: v for k, v in stored.items() if k != 'embedding'}
    if not labels:
        raise ValueError(f'{path}: no sensitive attribute column next to the embedding')
    return probe_leakage(stored['embedding'], labels, config)

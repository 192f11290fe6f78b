"""Sensitive-attribute leakage of user embeddings: how well a freshly trained attacker recovers each attribute from the
embeddings of held-out users -- the number the adversarial models (PFCN_*, FairGo_*) are built to push down.

`probe_leakage(embedding, labels, config)` trains one attacker per attribute (a linear probe, or an MLP with one hidden layer:
`leakage_probe_hidden`) with Adam on mean softmax cross-entropy, all attackers in ONE fused step per batch (csrc/probe.hip:
fr_probe_step, two launches whatever the number of attributes, a tile of the embedding matrix read once for all of them), then
reads the held-out rows with the same kernel's forward (fr_probe_forward) and reduces them on the device (fr_probe_eval, then one
torch.sort per class and fr_auc_sorted).  torch does index plumbing only.

The procedure, all host randomness from ONE `torch.Generator().manual_seed(seed)` in this order:
  1. perm = torch.randperm(U): the first floor(test_ratio * U) rows are the test rows, the rest the train rows;
  2. per attribute, in the order of `labels`: W1, b1, W2, b2 uniform in +-1/sqrt(fan_in) (hidden 0: W, b);
  3. per epoch one torch.randperm(n_train); batches are consecutive slices of `leakage_probe_batch` rows, the short last one kept.
No standardisation of the embedding, no class weights, no early stopping.

Result keys per attribute <A> (rounded to `metric_decimal_place`):
  'leakage auc of sensitive attribute <A>'       two classes: AUC of p(class 1); more: the mean one-vs-rest AUC over the classes
                                                 that have a positive and a negative test row
  'leakage accuracy of sensitive attribute <A>'  (= micro-F1 for single-label classes)
  'leakage majority of sensitive attribute <A>'  the share of test rows in the largest train class: what accuracy has to beat
  'leakage logloss of sensitive attribute <A>'   mean log-loss on the test rows
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict

import torch

from .. import _C
from .groups import attribute_groups

KEYS = ('leakage_probe', 'leakage_probe_hidden', 'leakage_probe_epochs', 'leakage_probe_batch', 'leakage_probe_lr',
        'leakage_probe_test_ratio')
DEFAULTS = {'leakage_probe_hidden': 64, 'leakage_probe_epochs': 20, 'leakage_probe_batch': 4096, 'leakage_probe_lr': 0.001,
            'leakage_probe_test_ratio': 0.2}


def _get(config, key):
    try:
        value = config[key]
    except KeyError:
        value = None
    return DEFAULTS.get(key) if value is None else value


def _integer(config, key, lo, hi):
    value = _get(config, key)
    if isinstance(value, bool) or not isinstance(value, int) or not lo <= value <= hi:
        raise ValueError(f'{key} must be an integer in {lo}..{hi}, not {value!r}')
    return value


def probe_enabled(config) -> bool:
    """`leakage_probe`: None / False = off, True = on; anything else is refused"""
    value = _get(config, 'leakage_probe')
    if value is None or value is False:
        return False
    if value is not True:
        raise ValueError(f'leakage_probe must be None, False or True, not {value!r}')
    return True


def probe_settings(config) -> dict:
    """The validated leakage_probe_* keys (a ValueError names the key) and the seed"""
    probe_enabled(config)
    out = {'hidden': _integer(config, 'leakage_probe_hidden', 0, 256),
           'epochs': _integer(config, 'leakage_probe_epochs', 1, 1 << 20),
           'batch': _integer(config, 'leakage_probe_batch', 1, _C.PROBE_MAX_BATCH)}
    lr = _get(config, 'leakage_probe_lr')
    if isinstance(lr, bool) or not isinstance(lr, (int, float)) or not (lr > 0 and math.isfinite(lr)):
        raise ValueError(f'leakage_probe_lr must be a positive number, not {lr!r}')
    ratio = _get(config, 'leakage_probe_test_ratio')
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not 0.0 < ratio < 1.0:
        raise ValueError(f'leakage_probe_test_ratio must lie strictly between 0 and 1, not {ratio!r}')
    seed = _get(config, 'seed')
    places = _get(config, 'metric_decimal_place')
    out.update(lr=float(lr), test_ratio=float(ratio), seed=int(seed) if seed is not None else 0,
               places=int(places) if places is not None else 4)
    return out


def init_params(g: torch.Generator, D: int, H: int, classes) -> torch.Tensor:
    """The flat parameter vector [head][W1 | b1 | W2 | b2] (H == 0: [W | b]) on the host: every tensor uniform in
    +-1/sqrt(fan_in), drawn in layout order"""
    parts = []
    for C in classes:
        shapes = ([(H * D, D), (H, D), (C * H, H), (C, H)] if H else [(C * D, D), (C, D)])
        for n, fan_in in shapes:
            parts.append((torch.rand(n, generator=g, dtype=torch.float32) * 2.0 - 1.0) * (1.0 / math.sqrt(fan_in)))
    return torch.cat(parts)


class Probe:
    """The attackers of one probe on the device: parameters, Adam state, the argument block of the kernels"""

    def __init__(self, X: torch.Tensor, label_table: torch.Tensor, classes, hidden: int, lr: float, params: torch.Tensor):
        from ..optim import AdamHyper
        self.X, self.labels, self.classes, self.H = X, label_table, [int(c) for c in classes], int(hidden)
        self.U, self.D = X.shape
        self.dev = X.device
        self.carr = (ctypes.c_int32 * len(self.classes))(*self.classes)
        rc = _C.lib().fr_probe_supported(self.D, self.H, len(self.classes), self.carr)
        _C.check(rc, 'fr_probe_supported')
        self.P = int(_C.lib().fr_probe_param_count(self.D, self.H, len(self.classes), self.carr))
        if params.numel() != self.P:
            raise ValueError(f'the probe has {self.P} parameters, not {params.numel()}')
        self.params = params.to(self.dev, torch.float32).contiguous()
        self.m, self.v = torch.zeros_like(self.params), torch.zeros_like(self.params)
        self.hyper = AdamHyper(lr=lr, device=self.dev)
        self.step = 0
        self.loss = torch.zeros(1 + len(self.classes), dtype=torch.float32, device=self.dev)
        self.err = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.ws = None

    def _args(self, rows: torch.Tensor):
        a = _C.FrProbeArgs(self.X.data_ptr(), rows.data_ptr(), self.labels.data_ptr(), self.U, self.X.stride(0),
                           self.labels.stride(0), rows.numel(), self.D, self.H, len(self.classes))
        for i, c in enumerate(self.classes):
            a.classes[i] = c
        return a

    def train_step(self, rows: torch.Tensor):
        """one optimiser step of every head on the rows `rows` (int64, on the device)"""
        need = _C.lib().fr_probe_step_workspace_bytes(self.D, self.H, len(self.classes), self.carr, rows.numel())
        if self.ws is None or self.ws.numel() < need:
            self.ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
        self.step += 1
        self.hyper.check_step(self.step)
        a = self._args(rows)
        _C.check(_C.lib().fr_probe_step(ctypes.byref(a), self.params.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                                        ctypes.byref(self.hyper.c()), self.step, self.loss.data_ptr(), None, self.ws.data_ptr(),
                                        self.ws.numel(), self.err.data_ptr(), _C.current_stream()), 'fr_probe_step')

    def logits(self, rows: torch.Tensor) -> torch.Tensor:
        """[len(rows), sum C] logits of the rows, in slices the kernel takes"""
        out = torch.empty(rows.numel(), sum(self.classes), dtype=torch.float32, device=self.dev)
        for lo in range(0, rows.numel(), _C.PROBE_MAX_BATCH):
            part = rows[lo:lo + _C.PROBE_MAX_BATCH]
            a = self._args(part)
            _C.check(_C.lib().fr_probe_forward(ctypes.byref(a), self.params.data_ptr(), out[lo:].data_ptr(), self.err.data_ptr(),
                                               _C.current_stream()), 'fr_probe_forward')
        return out

    def evaluate(self, rows: torch.Tensor):
        """-> (correct int64 [heads], logloss double [heads], class_count int64 [sum C], probs float [n, sum C]) of the rows"""
        z = self.logits(rows)
        n, heads, sumC = rows.numel(), len(self.classes), sum(self.classes)
        correct = torch.empty(heads, dtype=torch.int64, device=self.dev)
        logloss = torch.empty(heads, dtype=torch.float64, device=self.dev)
        count = torch.empty(sumC, dtype=torch.int64, device=self.dev)
        probs = torch.empty(n, sumC, dtype=torch.float32, device=self.dev)
        carr = self.carr
        ws = torch.empty(_C.lib().fr_probe_eval_workspace_bytes(n, heads, carr), dtype=torch.uint8, device=self.dev)
        _C.check(_C.lib().fr_probe_eval(z.data_ptr(), self.labels.data_ptr(), self.labels.stride(0), rows.data_ptr(), self.U, n,
                                        heads, carr, correct.data_ptr(), logloss.data_ptr(), count.data_ptr(), probs.data_ptr(),
                                        ws.data_ptr(), ws.numel(), self.err.data_ptr(), _C.current_stream()), 'fr_probe_eval')
        return correct, logloss, count, probs

    def check_device_errors(self):
        if int(self.err.item()) != 0:
            raise _C.FairrecError('leakage probe: a row index or a label was out of range on the device')


def _auc(score: torch.Tensor, positive: torch.Tensor):
    """(2U, P, N) of fr_auc_sorted for one score column and a 0 / 1 float label column"""
    srt, order = torch.sort(score)
    out = torch.empty(3, dtype=torch.int64, device=score.device)
    by_score = positive[order].contiguous()
    _C.call('auc_sorted', srt.data_ptr(), by_score.data_ptr(), score.numel(), out.data_ptr(), ws=(score.numel(),),
            device=score.device)
    return out.cpu().tolist()


def probe_leakage(embedding: torch.Tensor, labels: Dict[str, torch.Tensor], config) -> Dict[str, float]:
    """Train the attackers on `embedding` [U, D] (any model's user matrix; moved to the GPU if it is not there) against
    `labels` (attribute name -> column [U] of attribute values) and report the leakage keys of the module docstring."""
    s = probe_settings(config)
    if not labels:
        raise ValueError('probe_leakage needs at least one attribute column')
    if len(labels) > _C.PROBE_MAX_HEADS:
        raise ValueError(f'probe_leakage takes at most {_C.PROBE_MAX_HEADS} attributes at once, not {len(labels)}')
    X = embedding.detach()
    if X.dim() != 2 or X.shape[0] < 2:
        raise ValueError(f'probe_leakage needs an embedding matrix [users, dim] with at least two users, not {tuple(X.shape)}')
    if not X.is_cuda:
        X = X.cuda()
    X = X.to(torch.float32)
    if X.stride(1) != 1:
        X = X.contiguous()
    dev, n_rows = X.device, X.shape[0]
    for name, col in labels.items():
        if col.numel() != n_rows:
            raise ValueError(f'sensitive attribute {name}: {col.numel()} labels for {n_rows} embedding rows')
    groups = attribute_groups({k: v.to(dev) for k, v in labels.items()})      # (refuses an attribute with one value)
    classes = [g.n_groups for g in groups]
    table = torch.stack([g.index.to(torch.int64) for g in groups]).contiguous()

    g = torch.Generator().manual_seed(s['seed'])
    perm = torch.randperm(n_rows, generator=g)
    n_test = int(math.floor(s['test_ratio'] * n_rows))
    test, train = perm[:n_test].to(dev), perm[n_test:].to(dev)
    probe = Probe(X, table, classes, s['hidden'], s['lr'], init_params(g, X.shape[1], s['hidden'], classes))
    counts = {}
    for part, rows in (('train', train), ('test', test)):      # rows per class, by the metric kernel (the parameters do not matter)
        counts[part] = probe.evaluate(rows)[2].cpu().tolist() if rows.numel() else [0] * sum(classes)
    off = 0
    for a, grp in enumerate(groups):
        for part in ('train', 'test'):
            present = sum(1 for c in counts[part][off:off + classes[a]] if c > 0)
            if present < 2:
                raise ValueError(f'sensitive attribute {grp.name}: fewer than two classes among the {part} rows of the leakage '
                                 f'probe ({present} of {classes[a]})')
        off += classes[a]
    for _ in range(s['epochs']):
        order = train[torch.randperm(train.numel(), generator=g).to(dev)]
        for lo in range(0, order.numel(), s['batch']):
            probe.train_step(order[lo:lo + s['batch']])
    correct, logloss, _, probs = probe.evaluate(test)
    probe.check_device_errors()
    correct, logloss = correct.cpu().tolist(), logloss.cpu().tolist()
    res, off = {}, 0
    for a, grp in enumerate(groups):
        C = classes[a]
        y_test = table[a][test]
        train_count = counts['train'][off:off + C]
        majority = train_count.index(max(train_count))          # (the lowest class among equal counts)
        aucs = []
        for c in ([1] if C == 2 else range(C)):
            two_u, P, N = _auc(probs[:, off + c].contiguous(), (y_test == c).to(torch.float32))
            if P > 0 and N > 0:
                aucs.append(two_u / (2.0 * P * N))
        tail = f'of sensitive attribute {grp.name}'
        res[f'leakage auc {tail}'] = round(sum(aucs) / len(aucs), s['places'])
        res[f'leakage accuracy {tail}'] = round(correct[a] / n_test, s['places'])
        res[f'leakage majority {tail}'] = round(counts['test'][off + majority] / n_test, s['places'])
        res[f'leakage logloss {tail}'] = round(logloss[a] / n_test, s['places'])
        off += C
    return res

"""Negative sampling on the device with the interface of recbole/sampler/sampler.py (`Sampler(phases, datasets,
distribution)`, `set_phase`, `sample_by_user_ids`) and the SAME numbers: the sampled ids are bit-identical to what
the reference's numpy-based sampler draws from the same generator state (fr_sample_negatives).

The numpy global generator the reference draws from (`np.random.randint`, sampler.py:240-241) is mirrored by a
`DeviceRandomState` that keeps numpy's legacy MT19937 state in device memory.  `get_state()` / `set_state()` use
numpy's own tuple format, so host code that must draw from the same stream between batches (FOCFDataLoader's
`np.random.choice`, the trainers' per-epoch attribute masks, trainer.py:879-882) can take the stream over and hand it
back:   np.random.set_state(rs.get_state()); ...host draws...; rs.set_state(np.random.get_state())
"""
from __future__ import annotations

import copy
from typing import Dict, Optional

import numpy as np
import torch

from .. import _C

STATE_WORDS = 625     # key[624] + pos


class DeviceRandomState:
    """numpy's legacy RandomState (MT19937), resident on the GPU."""

    def __init__(self, device, seed: Optional[int] = None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _C.FairrecError("DeviceRandomState needs a GPU (no CPU fallback by design)")
        _C.lib()
        self.state = torch.zeros(STATE_WORDS, dtype=torch.int32, device=self.device)
        self._ws: Optional[torch.Tensor] = None
        self.err_flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.seed(0 if seed is None else seed)

    def seed(self, seed: int):
        """np.random.seed(seed) for an int seed."""
        seed = int(seed)
        if not 0 <= seed <= 0xFFFFFFFF:
            raise ValueError("Seed must be between 0 and 2**32 - 1")
        _C.check(_C.lib().fr_mt19937_seed(self.state.data_ptr(), seed, _C.current_stream()), "fr_mt19937_seed")

    def get_state(self):
        """np.random.get_state() tuple of the device stream (host sync)."""
        w = self.state.cpu().numpy().view(np.uint32)
        return ("MT19937", w[:624].copy(), int(w[624]), 0, 0.0)

    def set_state(self, state):
        key = np.asarray(state[1], dtype=np.uint32)
        w = np.concatenate([key, np.array([int(state[2])], dtype=np.uint32)]).view(np.int32)
        self.state.copy_(torch.from_numpy(w.copy()))

    def _workspace(self, nbytes: int) -> torch.Tensor:
        """The scratch buffer, grown to at least `nbytes` (the only place it grows)."""
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws

    def _lists_workspace(self, positions: int) -> torch.Tensor:
        """Room for the two collision lists of a call of `positions` values."""
        return self._workspace(_C.lib().fr_sample_negatives_workspace_bytes(positions))

    def _call_sequence(self, call_keys: torch.Tensor, call_counts: torch.Tensor):
        """(keys, offsets, total, max_call, out) of a sequence of single-key calls: call c fills
        out[offsets[c]:offsets[c + 1]] for key keys[c] (one host sync for the two sizes)."""
        keys = call_keys.to(self.device, torch.int64).contiguous()
        counts = call_counts.to(self.device, torch.int64)
        offsets = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=self.device)
        torch.cumsum(counts, 0, out=offsets[1:])
        total, max_call = int(offsets[-1].item()), int(counts.max().item()) if counts.numel() else 0
        return keys, offsets, total, max_call, torch.empty(total, dtype=torch.int64, device=self.device)

    def randint(self, low: int, high: int, n: int) -> torch.Tensor:
        """np.random.randint(low, high, n) as an int64 device tensor (range below 2**32 - 1)."""
        out = torch.empty(n, dtype=torch.int64, device=self.device)
        if n:
            _C.check(_C.lib().fr_sample_negatives(self.state.data_ptr(), low, high, None, n, 1, None, None, 0,
                                                  out.data_ptr(), None, None, 0, self.err_flag.data_ptr(),
                                                  _C.current_stream()), "fr_sample_negatives")
        return out

    def sample_excluding(self, low: int, high: int, key_ids: torch.Tensor, num: int, used_indptr: torch.Tensor,
                         used_items: torch.Tensor, rounds_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        key_ids = key_ids.to(self.device, torch.int64).contiguous()
        n = key_ids.numel()
        out = torch.empty(n * num, dtype=torch.int64, device=self.device)
        if n:
            ws = self._lists_workspace(n * num)
            _C.check(_C.lib().fr_sample_negatives(self.state.data_ptr(), low, high, key_ids.data_ptr(), n, num,
                                                  used_indptr.data_ptr(), used_items.data_ptr(), used_indptr.numel() - 1,
                                                  out.data_ptr(), _C.ptr(rounds_out), ws.data_ptr(), ws.numel(),
                                                  self.err_flag.data_ptr(), _C.current_stream()), "fr_sample_negatives")
        return out

    def sample_calls(self, low: int, high: int, call_keys: torch.Tensor, call_counts: torch.Tensor,
                     used_indptr: torch.Tensor, used_items: torch.Tensor) -> torch.Tensor:
        """Consecutive single-key calls on this stream in one launch: call c draws call_counts[c] values for key
        call_keys[c] (each call finishes its re-draw rounds before the next one draws).  Returns the concatenation."""
        call_keys, offsets, total, max_call, out = self._call_sequence(call_keys, call_counts)
        if total:
            # (room for the speculative form of a long call sequence: csrc/sampler.hip, sample_calls_fast_kernel)
            ws = self._workspace(max(_C.lib().fr_sample_negatives_calls_workspace_bytes(total, max_call),
                                     _C.lib().fr_sample_negatives_workspace_bytes(max_call)))
            _C.check(_C.lib().fr_sample_negatives_calls(self.state.data_ptr(), low, high, call_keys.data_ptr(),
                                                        offsets.data_ptr(), call_keys.numel(), max_call,
                                                        used_indptr.data_ptr(), used_items.data_ptr(),
                                                        used_indptr.numel() - 1, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                        self.err_flag.data_ptr(), _C.current_stream()),
                     "fr_sample_negatives_calls")
        return out

    def sample_pop(self, table, key_ids: torch.Tensor, num: int, used_indptr: Optional[torch.Tensor],
                   used_items: Optional[torch.Tensor], rounds_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Popularity-biased negatives (fr_sample_negatives_pop): entry j for key key_ids[j % n], drawn through the alias
        table `table` (an _C.FrAliasTable of device arrays); used_indptr None = plain draws, no rejection."""
        key_ids = key_ids.to(self.device, torch.int64).contiguous()
        n = key_ids.numel()
        out = torch.empty(n * num, dtype=torch.int64, device=self.device)
        if n:
            ws = self._lists_workspace(n * num) if used_indptr is not None else None
            _C.check(_C.lib().fr_sample_negatives_pop(self.state.data_ptr(), table, key_ids.data_ptr(), n, num,
                                                      _C.ptr(used_indptr), _C.ptr(used_items),
                                                      used_indptr.numel() - 1 if used_indptr is not None else 0,
                                                      out.data_ptr(), _C.ptr(rounds_out), _C.ptr(ws),
                                                      ws.numel() if ws is not None else 0, self.err_flag.data_ptr(),
                                                      _C.current_stream()), "fr_sample_negatives_pop")
        return out

    def sample_calls_pop(self, table, call_keys: torch.Tensor, call_counts: torch.Tensor, used_indptr: torch.Tensor,
                         used_items: torch.Tensor) -> torch.Tensor:
        """`sample_calls` with popularity-biased draws (fr_sample_negatives_pop_calls): the calls one after the other in
        one launch, each finishing its re-draw rounds before the next one draws."""
        call_keys, offsets, total, max_call, out = self._call_sequence(call_keys, call_counts)
        if total:
            ws = self._lists_workspace(max_call)
            _C.check(_C.lib().fr_sample_negatives_pop_calls(self.state.data_ptr(), table, call_keys.data_ptr(),
                                                            offsets.data_ptr(), call_keys.numel(), max_call,
                                                            used_indptr.data_ptr(), used_items.data_ptr(),
                                                            used_indptr.numel() - 1, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                            self.err_flag.data_ptr(), _C.current_stream()),
                     "fr_sample_negatives_pop_calls")
        return out


_GLOBAL: Dict[str, DeviceRandomState] = {}


def global_random_state(device) -> DeviceRandomState:
    """The device mirror of numpy's global generator (one per device); `fairrec.utils.init_seed` seeds it together
    with numpy, as the reference seeds numpy (utils.py:172-189)."""
    key = str(torch.device(device))
    if key not in _GLOBAL:
        _GLOBAL[key] = DeviceRandomState(device)
        _GLOBAL[key].set_state(np.random.get_state())
    return _GLOBAL[key]


class host_numpy_stream:
    """`with host_numpy_stream():` -- host code inside draws from np.random exactly where the reference would: the
    device mirror(s) of numpy's global generator hand the stream to numpy on entry and take it back on exit (a 2.5 KB
    copy each way; meant for the rare host draws between batches -- per-epoch attribute masks, FOCF's item picks).
    Without a device mirror in use it does nothing."""

    def __enter__(self):
        self._rs = next(iter(_GLOBAL.values()), None)
        if self._rs is not None:
            np.random.set_state(self._rs.get_state())
        return self

    def __exit__(self, *exc):
        if self._rs is not None:
            st = np.random.get_state()
            for rs in _GLOBAL.values():
                rs.set_state(st)
        return False


def seed_all(seed: int):
    for rs in _GLOBAL.values():
        rs.seed(seed)


class Sampler:
    """recbole.sampler.Sampler (sampler.py:200-303): negative items per user, never one of the user's positive items
    of the current or an earlier phase.  Both distributions are drawn on the device from the shared numpy-compatible
    stream: 'uniform' (the reference default, overall.yaml) and 'popularity' (the alias method; the table is built on
    the host in the reference's float64 arithmetic and uploaded once)."""

    def __init__(self, phases, datasets, distribution='uniform', device=None, random_state: Optional[DeviceRandomState] = None):
        if not isinstance(phases, list):
            phases = [phases]
        if not isinstance(datasets, list):
            datasets = [datasets]
        if len(phases) != len(datasets):
            raise ValueError(f'Phases {phases} and datasets {datasets} should have the same length.')
        self._check_distribution(distribution)
        self.phases, self.datasets, self.distribution = phases, datasets, distribution
        self.uid_field, self.iid_field = datasets[0].uid_field, datasets[0].iid_field
        self.user_num, self.item_num = datasets[0].user_num, datasets[0].item_num
        self.device = torch.device(device if device is not None else "cuda")
        self.rs = random_state if random_state is not None else global_random_state(self.device)
        self._pop = None
        self.used_ids = self.get_used_ids()
        self.phase = None
        if distribution == 'popularity':
            self._build_alias_table()

    @staticmethod
    def _check_distribution(distribution):
        if distribution not in ('uniform', 'popularity'):
            raise NotImplementedError(f'The sampling distribution [{distribution}] is not implemented.')

    def get_used_ids(self):
        """Per phase a CSR (indptr int64 [user_num+1], items int32 sorted per user) of the items used up to and
        including that phase (sampler.py:243-265: each phase's sets start from the previous phase's)."""
        out, u_all, i_all = {}, [], []
        for phase, ds in zip(self.phases, self.datasets):
            u_all.append(ds.inter_feat[self.uid_field].cpu().numpy().astype(np.int64))
            i_all.append(ds.inter_feat[self.iid_field].cpu().numpy().astype(np.int64))
            pairs = np.unique(np.concatenate(u_all) * self.item_num + np.concatenate(i_all))   # sorted by (user, item)
            users, items = pairs // self.item_num, pairs % self.item_num
            counts = np.bincount(users, minlength=self.user_num)
            indptr = np.zeros(self.user_num + 1, dtype=np.int64)
            np.cumsum(counts, out=indptr[1:])
            out[phase] = (torch.from_numpy(indptr).to(self.device), torch.from_numpy(items.astype(np.int32)).to(self.device),
                          int(counts.max()) if len(counts) else 0)
            self._used_last = (users, items)       # the largest sets (every phase's), for the popularity support guard
        if out and out[self.phases[-1]][2] + 1 >= self.item_num:      # [pad] is an item (sampler.py:258-264)
            raise ValueError('Some users have interacted with all items, which we can not sample negative items for '
                             'them. Please set `user_inter_num_interval` to filter those users.')
        return out

    # --- popularity-biased sampling (sampler.py:72-118): the alias method over the items of all phases' interactions.
    # The table is built here, on the host, in the reference's float64 arithmetic and dict insertion order (the ids
    # depend on every bit of it), uploaded once per Sampler (the set_phase copies share it), and drawn from on the device
    # by fr_sample_negatives_pop* at the reference's position of the ONE stream shared with numpy.
    def _build_alias_table(self):
        from collections import Counter
        cand = []
        for ds in self.datasets:                                   # _get_candidates_list, sampler.py:229-233
            cand.extend(ds.inter_feat[self.iid_field].cpu().numpy())
        prob = dict(Counter(cand))                                 # insertion order = first occurrence, as in the reference
        alias = prob.copy()
        large_q, small_q = [], []
        for i in prob:
            alias[i] = -1
            prob[i] = prob[i] / len(cand) * len(prob)
            if prob[i] > 1:
                large_q.append(i)
            elif prob[i] < 1:
                small_q.append(i)
        while len(large_q) != 0 and len(small_q) != 0:
            l, s = large_q.pop(0), small_q.pop(0)
            alias[s] = l
            prob[l] = prob[l] - (1 - prob[s])
            if prob[l] < 1:
                small_q.append(l)
            elif prob[l] > 1:
                large_q.append(l)
        keys = np.array(list(prob.keys()), dtype=np.int64)
        # support guard: a user whose used-set holds every key of the table has nothing left to draw (the reference's
        # rejection loop never ends for that user); refused here, before any launch.  (An empty table is refused by
        # fr_sample_negatives_pop at the first draw, where the reference's randint(0, 0) raises.)
        users, items = self._used_last
        cover = np.bincount(users[np.isin(items, keys)], minlength=self.user_num)
        if len(keys) and len(cover) and int(cover.max()) >= len(keys):
            raise ValueError(f'Some users have interacted with every item of the popularity table ({len(keys)} items), '
                             'which we can not sample popularity-biased negative items for them. Please set '
                             '`user_inter_num_interval` to filter those users.')
        host = (keys, np.array([prob[k] for k in keys], dtype=np.float64), np.array([alias[k] for k in keys], dtype=np.int64))
        self._pop = tuple(torch.from_numpy(a).to(self.device) for a in host)
        self._pop_table = _C.FrAliasTable(self._pop[0].data_ptr(), self._pop[1].data_ptr(), self._pop[2].data_ptr(),
                                          len(keys))

    def set_distribution(self, distribution):
        """sampler.py `set_distribution`: switch between 'uniform' and 'popularity' (the alias table is built on the
        first switch to 'popularity')."""
        self._check_distribution(distribution)
        self.distribution = distribution
        if distribution == 'popularity' and self._pop is None:
            self._build_alias_table()

    def set_phase(self, phase):
        if phase not in self.phases:
            raise ValueError(f'Phase [{phase}] not exist.')
        new = copy.copy(self)
        new.phase = phase
        new.used_ids = self.used_ids[phase]
        return new

    def sample_by_user_ids(self, user_ids, item_ids, num):
        """[len(user_ids) * num] negative item ids on the device: entry j belongs to user_ids[j % len(user_ids)]
        (sampler.py:283-303); `item_ids` is unused, as in the reference."""
        if self.phase is None:
            raise ValueError('call set_phase() first')
        if not torch.is_tensor(user_ids):
            user_ids = torch.as_tensor(np.asarray(user_ids), dtype=torch.int64)
        indptr, items, _ = self.used_ids
        if self.distribution == 'popularity':
            return self.rs.sample_pop(self._pop_table, user_ids, int(num), indptr, items)
        return self.rs.sample_excluding(1, self.item_num, user_ids, int(num), indptr, items)

    def sample_calls(self, call_keys, counts):
        """Consecutive single-user sample_by_user_ids calls in one launch (the evaluation loader's user-by-user draws):
        call c draws counts[c] negatives for user call_keys[c] and finishes its re-draw rounds before call c + 1 draws.
        Returns the concatenation."""
        if self.phase is None:
            raise ValueError('call set_phase() first')
        indptr, items, _ = self.used_ids
        if self.distribution == 'popularity':
            return self.rs.sample_calls_pop(self._pop_table, call_keys, counts, indptr, items)
        return self.rs.sample_calls(1, self.item_num, call_keys, counts, indptr, items)

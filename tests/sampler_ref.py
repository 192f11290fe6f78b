"""Plain numpy reference of the negative sampler's call sequences, and a host model of their speculative form.

* `calls_ref`: consecutive single-key `sample_by_key_ids` calls (reference sampler.py:145-197) on a real
  np.random.RandomState -- what fr_sample_negatives_calls must reproduce, ids and generator state alike.
* `by_key_ids_ref`: one mixed-key call (np.tile order) -- fr_sample_negatives.
* `spec_model`: the control flow of sample_calls_fast_kernel (csrc/sampler.hip) restated from what each call consumed, so
  that a test can say which path a case takes (no collision, a shift D < 32 at the end, a restart from the incoming state,
  a colliding call found behind a 65 536-position window boundary) and cannot drift into the easy path unnoticed.
* `calls_workspace_bytes`, `lo_t_for` and `accepted_available`: the host's workspace layout, the capacity it reads back
  from a workspace size, and the accepted values the twist and temper kernels make available.

Used-sets are CSR pairs (indptr int64 [n_users + 1], items sorted ascending per user), the layout of the C ABI.  A key
outside [0, n_users) has no used-set here: the kernels raise FR_DEV_ERR_INDEX_RANGE for it and never reject its values.
"""
from types import SimpleNamespace

import numpy as np

MT_N = 624
CALLS_WINDOW = 1 << 16      # positions the resolver searches at once for the next colliding call
CALLS_SHIFTS = 32           # shifts the per-position hit bits cover
CALLS_MIN = 16              # sequences shorter than this run call by call


class _Used:
    """Membership in the used-sets through one sorted array of user * stride + item keys."""

    def __init__(self, used, high):
        indptr, items = (np.asarray(a, dtype=np.int64) for a in used)
        self.n_users = len(indptr) - 1
        self.stride = max(int(high), int(items.max()) + 1 if len(items) else 1)
        self.keys = np.sort(np.repeat(np.arange(self.n_users, dtype=np.int64), np.diff(indptr)) * self.stride + items)

    def contains(self, keys, values):
        keys = np.asarray(keys, dtype=np.int64)
        ok = (keys >= 0) & (keys < self.n_users)
        q = np.where(ok, keys, 0) * self.stride + np.asarray(values, dtype=np.int64)
        at = np.searchsorted(self.keys, q)
        found = self.keys[np.minimum(at, len(self.keys) - 1)] == q if len(self.keys) else np.zeros(len(q), dtype=bool)
        return ok & (at < len(self.keys)) & found


def calls_ref(rs, low, high, keys, counts, used):
    """Call c draws counts[c] values for keys[c] with rs.randint(low, high, .), then re-draws its colliding positions in
    ascending order until none is left.  Returns (ids, consumed, first_hit): consumed[c] = accepted values call c took
    (counts[c] + its re-draws), first_hit[c] = offset in the call of its first colliding position in the first round
    (-1: none)."""
    mem = _Used(used, high)
    counts = np.asarray(counts, dtype=np.int64)
    ids = np.empty(int(counts.sum()), dtype=np.int64)
    consumed = np.zeros(len(counts), dtype=np.int64)
    first_hit = np.full(len(counts), -1, dtype=np.int64)
    o = 0
    for c, (k, n) in enumerate(zip(np.asarray(keys, dtype=np.int64), counts)):
        n = int(n)
        if n == 0:
            continue
        v = rs.randint(low, high, n)
        took = n
        check = np.nonzero(mem.contains(np.full(n, k), v))[0]
        if len(check):
            first_hit[c] = check[0]
        while len(check):
            v[check] = rs.randint(low, high, len(check))
            took += len(check)
            check = check[mem.contains(np.full(len(check), k), v[check])]
        ids[o:o + n] = v
        consumed[c] = took
        o += n
    return ids, consumed, first_hit


def by_key_ids_ref(rs, low, high, key_ids, num, used):
    """One sample_by_key_ids call over np.tile(key_ids, num): draw all, re-draw the colliding positions in ascending
    order until none is left."""
    mem = _Used(used, high)
    keys = np.tile(np.asarray(key_ids, dtype=np.int64), int(num))
    v = rs.randint(low, high, len(keys))
    check = np.nonzero(mem.contains(keys, v))[0]
    while len(check):
        v[check] = rs.randint(low, high, len(check))
        check = check[mem.contains(keys[check], v[check])]
    return v


# ---- the host side of fr_sample_negatives_calls (csrc/sampler.hip: calls_fast_layout, the lo_t bisection) ----------------
def _align(x):
    return (x + 255) // 256 * 256


def _layout(total, max_call):
    cap = total + max(1024, total // 32)
    nblk = 2 * cap // MT_N + 4
    size = 2 * _align(cap * 4) + _align(nblk * MT_N * 4) + 2 * _align(max_call * 4) + _align(32) + 2 * _align(total * 4) \
        + _align(nblk * 4)
    return cap, nblk, size


def calls_workspace_bytes(total, max_call):
    """fr_sample_negatives_calls_workspace_bytes."""
    return 0 if total < 1 or max_call < 1 else _layout(total, max_call)[2]


def lo_t_for(ws_bytes, max_call):
    """The largest total whose layout fits ws_bytes: the capacity the host lays the workspace out for."""
    lo, hi = 0, 1 << 30
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if calls_workspace_bytes(mid, max_call) <= ws_bytes:
            lo = mid
        else:
            hi = mid - 1
    return lo


def _mask(span):
    m = span
    for s in (1, 2, 4, 8, 16):
        m |= m >> s
    return m


def accepted_available(state, low, high, total, lo_t):
    """n_acc: the accepted values the twist kernel's block estimate and the temper passes make available to the resolver,
    for a sequence of `total` values starting from numpy state tuple `state` with a layout for lo_t."""
    span = int(high) - 1 - int(low)
    mask = _mask(span)
    cap, nblk_max, _ = _layout(lo_t, 1)
    want = min(total + max(total // 32, 1024), cap)
    pos0 = int(state[2])
    rate = (span + 1.0) / (mask + 1.0)
    need = want - int((MT_N - pos0) * rate * 0.9)
    nblk = int(need / (MT_N * rate * 0.94)) + 2 if need > 0 else 0
    nblk = min(nblk, nblk_max - 1)
    rs = np.random.RandomState()
    rs.set_state(state)
    words = rs.randint(0, 2 ** 32, MT_N - pos0 + nblk * MT_N, dtype=np.uint32)      # (the raw words, one per draw)
    return min(int(np.count_nonzero((words & np.uint32(mask)) <= span)), want)


def spec_model(counts, extra, first_hit=None, *, span=1, lo_t=None, n_acc=None):
    """The resolver's control flow from each call's extra consumption (consumed - count).

    first_hit[c]: offset of call c's first colliding position (default: its first position).  lo_t: the capacity of the
    workspace layout (default: the total).  n_acc: accepted values available (default: unlimited).

    Returns a namespace: speculative (the sequence takes the speculative form at all), path ("call_by_call", "restart" or
    "speculative"), D (the shift after each call, -1 behind a restart), restart_at (the call after which the resolver gives
    up and restarts from the incoming state; -1 before the first, None: no restart), restart_reason ("shift", "slack",
    "capacity"), collided (the calls resolved round by round), straddles ([(call, window start)]: colliding calls found in
    a window that starts inside them)."""
    counts = np.asarray(counts, dtype=np.int64)
    extra = np.asarray(extra, dtype=np.int64)
    n_calls = len(counts)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    total = int(offsets[-1])
    lo_t = total if lo_t is None else lo_t
    n_acc = float("inf") if n_acc is None else n_acc
    out = SimpleNamespace(speculative=n_calls >= CALLS_MIN and span > 0 and lo_t >= n_calls, path="call_by_call",
                          D=np.cumsum(extra), restart_at=None, restart_reason=None, collided=[], straddles=[])
    if not out.speculative:
        return out

    def give_up(call, reason):
        out.path, out.restart_at, out.restart_reason = "restart", call, reason
        out.D[call + 1:] = -1
        return out

    if total > lo_t:
        return give_up(-1, "capacity")
    if total > n_acc:
        return give_up(-1, "slack")
    hit_at = offsets[:-1] + (0 if first_hit is None else np.asarray(first_hit, dtype=np.int64))
    colliding = [c for c in range(n_calls) if extra[c] > 0]
    D, p0, k = 0, 0, 0
    while p0 < total:
        pe = min(p0 + CALLS_WINDOW, total)
        cf = colliding[k] if k < len(colliding) and hit_at[colliding[k]] < pe else None
        pf = int(offsets[cf]) if cf is not None else pe
        if pf + D > n_acc:
            return give_up(int(np.searchsorted(offsets, pf, side="right")) - 2, "slack")
        if cf is None:
            p0 = pe
            continue
        if pf < p0:
            out.straddles.append((cf, p0))
        if pf + D + counts[cf] + extra[cf] > n_acc:
            return give_up(cf - 1, "slack")
        D += int(extra[cf])
        out.collided.append(cf)
        k += 1
        p0 = int(offsets[cf + 1])
        if D >= CALLS_SHIFTS:
            return give_up(cf, "shift")
    out.path = "speculative"
    return out

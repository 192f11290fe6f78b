"""GPU: fr_sample_negatives_calls through the C ABI against tests/sampler_ref.py -- consecutive sample_by_key_ids calls on a
real np.random.RandomState -- id for id, and the generator state (key[624], pos) afterwards.

The test chooses the workspace, and with it the path: the speculative form of csrc/sampler.hip (twist, temper, per-position
hit bits, the single-workgroup resolver) or the call-by-call kernel.  Every case states the path it is built for, and
sampler_ref.spec_model -- the resolver's control flow restated from what each call consumed in numpy -- must agree, so a
case can not drift into an easier path unnoticed.  Collisions are placed on purpose: the accepted values of the stream are
known in advance (numpy draws them), so a call's used-set can be made to contain exactly the values it should collide with.
"""
import numpy as np
import pytest
import torch

import sampler_ref as R

pytestmark = pytest.mark.gpu


def _lib():
    from fairrec import _C
    return _C


def _state(pos, seed=1234):
    """numpy state at stream position `pos`: 624 = fresh seed, else that many words drawn; 0 = a state tuple with pos 0."""
    rs = np.random.RandomState(seed)
    if pos == 0:
        st = rs.get_state()
        return (st[0], st[1], 0, 0, 0.0)
    if pos != 624:
        rs.randint(0, 2 ** 32, pos, dtype=np.uint32)
    return rs.get_state()


def _csr(sets):
    indptr = np.zeros(len(sets) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(s) for s in sets])
    items = np.concatenate([np.sort(np.fromiter(s, dtype=np.int64, count=len(s))) for s in sets] + [np.zeros(0, np.int64)])
    return indptr, items.astype(np.int32)


def _design(state, low, high, counts, coll=(), empty=(), seed=0):
    """One user per call (user c + 1; user 0 has no used-set).  coll = {call: (hit offsets, chain)}: the call's first round
    collides at exactly those offsets, then `chain` more single collisions follow (extra consumption = hits + chain).  Every
    other call's user gets a few used items that none of its values hits; calls in `empty` get an empty used-set."""
    coll = dict(coll)
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    A = np.random.RandomState()
    A.set_state(state)
    A = A.randint(low, high, int(offsets[-1]) + sum(len(h) + ch for h, ch in coll.values()) + 8)
    sets, D = [set()], 0
    for c, n in enumerate(counts):
        s, n = int(offsets[c]) + D, int(n)
        if c in coll:
            hits, chain = coll[c]
            for shift in range(64):
                H = [j + shift for j in hits]
                assert H[-1] < n, "design: no room for the hits"
                r2 = A[s + n:s + n + len(H)]
                tail = A[s + n + len(H):s + n + len(H) + chain]
                U = set(A[s + j] for j in H) | (set([r2[0]]) | set(tail[:-1]) if chain else set())
                final = list(np.delete(A[s:s + n], H)) + list(r2[1:]) + [tail[-1] if chain else r2[0]]
                if not U & set(final):
                    break
            else:
                raise AssertionError("design: no collision-free placement")
            sets.append(U)
            D += len(H) + chain
        elif c in empty:
            sets.append(set())
        else:
            cand = rng.integers(low, high, 4)
            sets.append(set(cand[~np.isin(cand, A[s:s + n])].tolist()))
    keys = np.arange(1, len(counts) + 1, dtype=np.int64)
    return keys, counts, _csr(sets)


def _ws_bytes(kind, total, max_call, n_calls):
    C = _lib()
    if kind == "exact":
        return C.lib().fr_sample_negatives_calls_workspace_bytes(total, max_call)
    if kind == "x4":                 # the in-tree case: Sampler._ws is reused for smaller batches
        return C.lib().fr_sample_negatives_calls_workspace_bytes(4 * total, max_call)
    if kind == "calls":              # room for the call-by-call form only
        return C.lib().fr_sample_negatives_workspace_bytes(max_call)
    if kind == "short":              # laid out for n_calls <= lo_t < total
        return C.lib().fr_sample_negatives_calls_workspace_bytes(max(n_calls, total // 2), max_call)
    raise ValueError(kind)


def _launch(dev_state, low, high, keys, counts, used, ws_bytes):
    """One fr_sample_negatives_calls launch on a device state (int32[625], numpy's layout); returns (ids, err_flag)."""
    C = _lib()
    counts = np.asarray(counts, dtype=np.int64)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)])).cuda()
    keys_d = torch.from_numpy(np.asarray(keys, dtype=np.int64)).cuda()
    indptr, items = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in used)
    if items.numel() == 0:           # (no used item at all: the ABI still wants a non-null list)
        items = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.full((int(counts.sum()),), -7, dtype=torch.int64, device="cuda")
    ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device="cuda")       # (the kernels must not rely on zeroed room)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    C.check(C.lib().fr_sample_negatives_calls(dev_state.data_ptr(), low, high, keys_d.data_ptr(), offsets.data_ptr(),
                                              len(counts), max(1, int(counts.max())), indptr.data_ptr(), items.data_ptr(),
                                              len(indptr) - 1, out.data_ptr(), ws.data_ptr(), ws_bytes, err.data_ptr(),
                                              C.current_stream()), "fr_sample_negatives_calls")
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(err.item())


def _dev_state(state):
    w = np.concatenate([np.asarray(state[1], dtype=np.uint32), np.array([state[2]], dtype=np.uint32)])
    return torch.from_numpy(w.view(np.int32).copy()).cuda()


def _read_state(dev_state):
    w = dev_state.cpu().numpy().view(np.uint32)
    return w[:624], int(w[624])


def _model(state, low, high, counts, consumed, first_hit, ws_bytes):
    counts = np.asarray(counts, dtype=np.int64)
    max_call, total = max(1, int(counts.max())), int(counts.sum())
    lo_t = R.lo_t_for(ws_bytes, max_call)
    n_acc = R.accepted_available(state, low, high, total, lo_t) if lo_t >= len(counts) else None
    return R.spec_model(counts, consumed - counts, first_hit, span=high - 1 - low, lo_t=lo_t, n_acc=n_acc)


def _run(state, low, high, keys, counts, used, ws="exact"):
    """Kernel vs numpy from `state`: every id, the state afterwards, a clean error flag.  Returns the spec model."""
    rs = np.random.RandomState()
    rs.set_state(state)
    want, consumed, first_hit = R.calls_ref(rs, low, high, keys, counts, used)
    counts = np.asarray(counts, dtype=np.int64)
    ws_bytes = _ws_bytes(ws, int(counts.sum()), max(1, int(counts.max())), len(counts))
    m = _model(state, low, high, counts, consumed, first_hit, ws_bytes)
    dev = _dev_state(state)
    got, err = _launch(dev, low, high, keys, counts, used, ws_bytes)
    np.testing.assert_array_equal(got, want)
    key, pos = _read_state(dev)
    st = rs.get_state()
    np.testing.assert_array_equal(key, st[1])
    assert pos == st[2]
    assert err == 0
    m.final = st
    return m


def _counts(n, rng, lo=50, hi=301, empty_at=()):
    c = rng.integers(lo, hi, n)
    c[list(empty_at)] = 0
    return c


BIG = 1_000_001           # span 999 999: designed collisions, nothing else collides


# ---- path ------------------------------------------------------------------------------------------------------------------
PATH_CASES = {
    # id: (n_calls, {call: (hit offsets, chain)}, expected path, expected D at the end / restart call)
    "spec_no_collision": (40, {}, "speculative", 0),
    "spec_D31_at_end": (40, {5: ([0], 9), 17: ([3, 40], 18), 39: ([7], 0)}, "speculative", 31),
    "restart_D32_mid": (40, {5: ([0], 11), 17: ([2], 19), 30: ([1], 2)}, "restart", 17),
    "restart_D32_last_call": (40, {5: ([0], 11), 39: ([2], 19)}, "restart", 39),
    "restart_one_call_40_extra": (40, {12: ([1, 9], 38)}, "restart", 12),
    "cbc_15_calls": (15, {3: ([0], 4)}, "call_by_call", None),
    "spec_16_calls": (16, {3: ([0], 4)}, "speculative", 5),
}


@pytest.mark.parametrize("ws", ["exact", "x4", "calls"])
@pytest.mark.parametrize("case", list(PATH_CASES))
def test_path(case, ws):
    n, coll, path, at = PATH_CASES[case]
    state = _state(311)
    rng = np.random.default_rng(len(case))
    keys, counts, used = _design(state, 1, BIG, _counts(n, rng), coll)
    m = _run(state, 1, BIG, keys, counts, used, ws)
    if ws == "calls":
        assert m.path == "call_by_call"
        return
    assert m.path == path, (m.path, m.restart_at, m.D)
    assert m.collided == sorted(coll)[:len(m.collided)]
    if path == "speculative":
        assert m.D[-1] == at
    elif path == "restart":
        assert m.restart_at == at and m.restart_reason == "shift" and m.D[at] >= 32


# ---- acceptance rate -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("low,high", [(1, 3), (1, 257), (1, 258), (1, 300), (1, 100_001), (1, BIG), (1000, 1300), (0, 1)],
                         ids=["span1", "span255_all_words", "span256_worst_rate", "span298", "span99999", "span999999",
                              "low1000_span299", "span0"])
def test_acceptance_rate(low, high):
    """Natural used-sets (a few random items per user, some users without any): the path is whatever the stream makes of
    it, stated by the model; both the no-collision and the colliding sequence are compared."""
    span = high - 1 - low
    rng = np.random.default_rng(high)
    state = _state(311)
    counts = _counts(48, rng, 1, 60, empty_at=(0, 20, 47))
    keys = rng.integers(1, 48, 48)
    none = _csr([set()] * 48)
    m = _run(state, low, high, keys, counts, none)
    assert m.path == ("speculative" if span > 0 else "call_by_call") and m.collided == []
    if span == 0:
        return
    # users 1..7 have one random item of the range (at span 1: every second draw collides), the others none
    sets = [set()] + [{int(low + rng.integers(0, span + 1))} if u < 8 else set() for u in range(1, 48)]
    m = _run(state, low, high, keys, counts, _csr(sets))
    assert m.speculative


# ---- incoming stream position ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos", [624, 311, 623, 0])
@pytest.mark.parametrize("kind", ["spec_collide", "restart"])
def test_incoming_position(pos, kind):
    state = _state(pos, seed=99)
    rng = np.random.default_rng(pos)
    coll = {4: ([1], 3), 20: ([0, 5], 1)} if kind == "spec_collide" else {4: ([1], 3), 20: ([0], 40)}
    keys, counts, used = _design(state, 1, BIG, _counts(32, rng), coll)
    m = _run(state, 1, BIG, keys, counts, used)
    assert m.path == ("speculative" if kind == "spec_collide" else "restart")


@pytest.mark.parametrize("pos", [311, 623])
def test_sequence_ending_in_the_incoming_block(pos):
    """16 calls of 8 values from pos 311: every consumed word is one of the incoming block's, so the state handed back is
    block 0 and the position a raw index inside it (from pos 623 the block has one word: the rest come from block 1)."""
    state = _state(pos, seed=5)
    rng = np.random.default_rng(1)
    keys, counts, used = _design(state, 1, 100_001, np.full(16, 8), {6: ([2], 1)})
    m = _run(state, 1, 100_001, keys, counts, used)
    assert m.path == "speculative" and m.D[-1] == 2
    assert np.array_equal(m.final[1], state[1]) == (pos == 311)          # (from 311: no twist, still block 0)


# ---- windows ---------------------------------------------------------------------------------------------------------------
def test_windows_and_long_calls():
    """230 k positions in 65 536-position resolver windows: a colliding call that starts before the first window boundary
    and collides behind it, another that straddles the boundary of the window searched after it, a call longer than
    CALLS_WINDOW colliding 66 000 positions in, and a 3 000-value call (longer than the 1 024-thread workgroup) with
    first-round hits on both sides of position 1 024."""
    state = _state(624, seed=8)
    counts = np.full(800, 200, dtype=np.int64)
    counts[327] = 900                        # [65 400, 66 300): hit at 65 400 + 500
    counts[720] = 70_000
    counts[780] = 3_000
    offsets = np.concatenate([[0], np.cumsum(counts)])
    assert offsets[327] < 65536 < offsets[328]
    e1 = int(offsets[328])                   # the resolver's next window is [e1, e1 + 65 536)
    c2 = int(np.searchsorted(offsets, e1 + 65536, side="right")) - 1
    hit2 = e1 + 65536 - int(offsets[c2]) + 3
    assert hit2 < counts[c2]
    assert c2 < 720
    coll = {327: ([500], 0), c2: ([hit2], 1), 720: ([66_000], 2), 780: ([10, 1500, 2900], 1)}
    keys, counts, used = _design(state, 1, BIG, counts, coll)
    m = _run(state, 1, BIG, keys, counts, used)
    assert int(np.sum(counts)) > 200_000
    assert m.path == "speculative" and m.collided == sorted(coll)
    assert [c for c, _ in m.straddles] == [327, c2, 720], m.straddles
    assert m.straddles[0][1] == 65536


# ---- call shapes -----------------------------------------------------------------------------------------------------------
def test_empty_calls_everywhere():
    """Empty calls first, in the middle (alone and in runs) and last: the hit kernel's call search must skip them; the calls
    behind each run collide at their first position."""
    state = _state(311, seed=3)
    rng = np.random.default_rng(4)
    empty = (0, 1, 2, 9, 15, 16, 17, 18, 30, 37, 38, 39)
    counts = _counts(40, rng, empty_at=empty)
    coll = {3: ([0], 0), 10: ([0], 1), 19: ([0], 0), 31: ([0], 2)}
    keys, counts, used = _design(state, 1, BIG, counts, coll, empty=empty)
    m = _run(state, 1, BIG, keys, counts, used)
    assert m.path == "speculative" and m.collided == sorted(coll)
    # ... and the same with call-by-call room
    _run(state, 1, BIG, keys, counts, used, "calls")


def test_single_value_calls_colliding_at_call_starts():
    """Calls of one value each, most of them colliding: every colliding position is its call's first."""
    state = _state(623, seed=12)
    counts = np.ones(64, dtype=np.int64)
    coll = {c: ([0], 0) for c in (1, 2, 3, 10, 20, 40, 63)}
    keys, counts, used = _design(state, 1, BIG, counts, coll)
    m = _run(state, 1, BIG, keys, counts, used)
    assert m.path == "speculative" and m.collided == sorted(coll) and m.D[-1] == 7


def test_one_item_left_long_rejection_chains():
    """Users whose used-set leaves one item of 299, with calls of 1-3 values, among users with empty used-sets."""
    state = _state(311, seed=21)
    rng = np.random.default_rng(21)
    item_num, n = 300, 24
    sets = [set()]
    for u in range(1, n + 1):
        if u % 5 == 0:
            sets.append(set(range(1, item_num)) - {int(rng.integers(1, item_num))})
        else:
            sets.append(set())
    keys = np.arange(1, n + 1)
    counts = np.where(keys % 5 == 0, rng.integers(1, 4, n), rng.integers(0, 40, n))
    m = _run(state, 1, item_num, keys, counts, _csr(sets))
    assert m.path == "restart" and m.restart_reason == "shift"
    _run(state, 1, item_num, keys, counts, _csr(sets), "calls")


# ---- workspace -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ws", ["exact", "x4", "short", "calls"])
def test_workspace_sizes(ws):
    """`short`: a workspace laid out for n_calls <= lo_t < total -- the kernels must mark no hit beyond the layout's
    positions and run the calls one after the other."""
    state = _state(624, seed=30)
    rng = np.random.default_rng(30)
    keys, counts, used = _design(state, 1, BIG, _counts(300, rng), {40: ([3], 2), 250: ([0], 0)})
    m = _run(state, 1, BIG, keys, counts, used, ws)
    want = {"exact": "speculative", "x4": "speculative", "short": "restart", "calls": "call_by_call"}[ws]
    assert m.path == want
    if ws == "short":
        assert m.restart_reason == "capacity"


# ---- continuation ----------------------------------------------------------------------------------------------------------
def test_two_launches_then_randint_and_sample_excluding_on_one_stream():
    from fairrec.sampler import DeviceRandomState
    state = _state(311, seed=44)
    rng = np.random.default_rng(44)
    keys, counts, used = _design(state, 1, BIG, _counts(40, rng), {7: ([0], 3)})
    rs = np.random.RandomState()
    rs.set_state(state)
    drs = DeviceRandomState("cuda", 0)
    drs.set_state(state)
    ws_bytes = _ws_bytes("exact", int(counts.sum()), int(counts.max()), len(counts))
    indptr_d, items_d = (torch.from_numpy(a).cuda() for a in used)
    for rep in range(2):
        want, consumed, _ = R.calls_ref(rs, 1, BIG, keys, counts, used)
        got, err = _launch(drs.state, 1, BIG, keys, counts, used, ws_bytes)
        np.testing.assert_array_equal(got, want)
        assert err == 0
    np.testing.assert_array_equal(drs.randint(1, 5000, 777).cpu().numpy(), rs.randint(1, 5000, 777))
    users = np.random.default_rng(0).integers(0, len(keys) + 1, 300)
    got = drs.sample_excluding(1, BIG, torch.from_numpy(users).cuda(), 2, indptr_d, items_d).cpu().numpy()
    np.testing.assert_array_equal(got, R.by_key_ids_ref(rs, 1, BIG, users, 2, used))
    st, (key, pos) = rs.get_state(), _read_state(drs.state)
    np.testing.assert_array_equal(key, st[1])
    assert pos == st[2]


# ---- error flag ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ws", ["exact", "calls"])
@pytest.mark.parametrize("bad", ["n_users", "minus1"])
def test_out_of_range_key_sets_the_error_flag(bad, ws):
    state = _state(311, seed=50)
    rng = np.random.default_rng(50)
    keys, counts, used = _design(state, 1, BIG, _counts(30, rng), {3: ([0], 1)})
    n_users = len(used[0]) - 1
    keys = keys.copy()
    keys[12] = n_users if bad == "n_users" else -1
    rs = np.random.RandomState()
    rs.set_state(state)
    want, consumed, first_hit = R.calls_ref(rs, 1, BIG, keys, counts, used)
    ws_bytes = _ws_bytes(ws, int(counts.sum()), int(counts.max()), len(counts))
    m = _model(state, 1, BIG, counts, consumed, first_hit, ws_bytes)
    assert m.path == ("speculative" if ws == "exact" else "call_by_call")
    got, err = _launch(_dev_state(state), 1, BIG, keys, counts, used, ws_bytes)
    assert err == _lib().DEV_ERR_INDEX_RANGE
    offsets = np.concatenate([[0], np.cumsum(counts)])
    other = np.ones(len(want), dtype=bool)
    other[offsets[12]:offsets[13]] = False
    np.testing.assert_array_equal(got[other], want[other])

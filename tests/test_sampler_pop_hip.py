"""GPU: popularity-biased negatives drawn on the device (fr_sample_negatives_pop, fr_sample_negatives_pop_calls and
Sampler('popularity')) are numpy's, id for id and word for word.  The restatement below is numpy itself: a RandomState,
the reference's dict-based alias construction (sampler.py `_build_alias_table`) and its `_pop_sampling` inside the
`sample_by_key_ids` rejection loop.  Every case also checks the generator state handed back (key, pos) and that numpy
continuing from it draws the same next 1000 words."""
from collections import Counter

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- the numpy restatement -------------------------------------------------------------------------------------------
def alias_table(cand):
    """sampler.py `_build_alias_table` over the candidate list: float64, dict insertion order (first occurrence)."""
    prob = dict(Counter(int(c) for c in cand))
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
    keys = np.array(list(prob), dtype=np.int64)
    return keys, np.array([prob[k] for k in keys], dtype=np.float64), np.array([alias[k] for k in keys], dtype=np.int64)


def pop_sampling(rs, tab, m):
    """sampler.py `_pop_sampling`: slots, then coins, then the alias choice."""
    keys, prob, alias = tab
    idx = rs.randint(0, len(keys), m)
    coin = rs.random_sample(m)
    return np.where(prob[idx] > coin, keys[idx], alias[idx])


def sample_by_key_ids(rs, tab, key_ids, num, used):
    """sampler.py `sample_by_key_ids`: draw all positions, re-draw the ones whose value is in the key's used-set, in
    ascending order, until none is left.  used=None: one plain draw."""
    keys = np.tile(np.asarray(key_ids, dtype=np.int64), num)
    value = np.zeros(len(keys), dtype=np.int64)
    check = np.arange(len(keys))
    while len(check) > 0:
        value[check] = pop_sampling(rs, tab, len(check))
        if used is None:
            break
        check = np.array([i for i in check if value[i] in used[keys[i]]], dtype=np.int64)
    return value


# ---- helpers ---------------------------------------------------------------------------------------------------------
def _device_table(keys, prob, alias):
    from fairrec import _C
    t = (torch.as_tensor(np.asarray(keys, dtype=np.int64), device=DEV),
         torch.as_tensor(np.asarray(prob, dtype=np.float64), device=DEV),
         torch.as_tensor(np.asarray(alias, dtype=np.int64), device=DEV))
    return _C.FrAliasTable(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), len(keys)), t


def _csr(used, n_users):
    indptr = np.zeros(n_users + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(used[u]) for u in range(n_users)])
    items = np.concatenate([np.array(sorted(used[u]), dtype=np.int32) for u in range(n_users)] + [np.zeros(0, np.int32)])
    return torch.from_numpy(indptr).to(DEV), torch.from_numpy(items).to(DEV)


def _states(seed, pos):
    """A numpy generator and its device mirror, both at stream position `pos` of the same key."""
    from fairrec.sampler import DeviceRandomState
    ref = np.random.RandomState(seed)
    ref.random_sample(3)
    st = ref.get_state()
    st = (st[0], st[1], pos, 0, 0.0)
    ref.set_state(st)
    dev = DeviceRandomState(DEV)
    dev.set_state(st)
    return ref, dev


def _check_state(dev, ref):
    got, want = dev.get_state(), ref.get_state()
    np.testing.assert_array_equal(got[1], want[1])
    assert got[2] == want[2]
    cont = np.random.RandomState()
    cont.set_state(got)
    np.testing.assert_array_equal(cont.randint(0, 2 ** 32, 1000, dtype=np.uint32), ref.randint(0, 2 ** 32, 1000, dtype=np.uint32))
    assert int(dev.err_flag.item()) == 0


def _world(rng, n_users, n_items, n_inter, skew=1.2, heavy=()):
    """Candidate list with a power-law popularity; used-sets = each user's interactions; the users in `heavy` also hold
    the most popular items up to >= 90 % of the popularity mass."""
    w = 1.0 / np.arange(1, n_items) ** skew
    items = rng.choice(np.arange(1, n_items), n_inter, p=w / w.sum())
    users = rng.integers(0, n_users, n_inter)
    used = [set() for _ in range(n_users)]
    for u, i in zip(users.tolist(), items.tolist()):
        used[u].add(i)
    tab = alias_table(items)
    cnt = Counter(items.tolist())
    for u in heavy:
        mass = 0
        for k, c in cnt.most_common():
            used[u].add(k)
            mass += c
            if mass >= 0.9 * n_inter:
                break
    return tab, used


# ---- ABI-level cases -------------------------------------------------------------------------------------------------
POSITIONS = [0, 1, 2, 311, 312, 313, 622, 623, 624]
TOTALS = [1, 63, 65, 1025, 3000, 32768]


@pytest.mark.parametrize("mix", ["mixed", "equal"])
@pytest.mark.parametrize("num", [1, 3])
@pytest.mark.parametrize("total", TOTALS)
def test_key_mixes_and_draw_counts(mix, num, total):
    rng = np.random.default_rng(total * 7 + num)
    n_users = 40
    tab, used = _world(rng, n_users, 500, 6000, heavy=(3, 17))
    n_keys = max(1, total // num)
    keys = rng.integers(0, n_users, n_keys) if mix == "mixed" else np.full(n_keys, 3)
    if mix == "mixed":
        keys[: min(n_keys, 8)] = 17                                     # a heavy user in every mixed case
    pos = POSITIONS[(total + num) % len(POSITIONS)]
    ref, dev = _states(total + num, pos)
    indptr, items = _csr(used, n_users)
    table, _keep = _device_table(*tab)
    rounds = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = dev.sample_pop(table, torch.from_numpy(keys), num, indptr, items, rounds_out=rounds).cpu().numpy()
    want = sample_by_key_ids(ref, tab, keys, num, used)
    np.testing.assert_array_equal(got, want)
    _check_state(dev, ref)
    assert int(rounds.item()) >= 1


@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("n_pop", [1, 2, 64, 65])
def test_stream_positions_and_table_sizes(pos, n_pop):
    """Incoming positions around both twists and at the block's end: the coin phase starts at either parity and its pairs
    straddle a twist.  n_pop == 1: the slot draw takes no words, the coins still take 2m."""
    rng = np.random.default_rng(pos * 100 + n_pop)
    n_users, n_items = 12, n_pop + 50
    cand = rng.choice(np.arange(1, n_pop + 1), 4 * n_pop + 7)
    cand[:n_pop] = np.arange(1, n_pop + 1)                               # every key present
    tab = alias_table(cand)
    used = [set(rng.choice(np.arange(1, n_items), 5).tolist()) for _ in range(n_users)]
    for s in used:
        if set(tab[0].tolist()) <= s:                                     # (every key used: the reference never ends)
            s.discard(int(tab[0][0]))
    used[5] = set(tab[0][: max(0, n_pop - 1)].tolist())                  # every key but one
    indptr, items = _csr(used, n_users)
    table, _keep = _device_table(*tab)
    ref, dev = _states(pos + 11, pos)
    for k, (n, num) in enumerate([(1, 1), (311, 1), (157, 3), (700, 1)]):      # one continuing stream
        keys = rng.integers(0, n_users, n)
        keys[0] = 5
        got = dev.sample_pop(table, torch.from_numpy(keys), num, indptr, items).cpu().numpy()
        np.testing.assert_array_equal(got, sample_by_key_ids(ref, tab, keys, num, used), err_msg=f"call {k}")
    _check_state(dev, ref)


def test_alias_minus_one_is_copied():
    """A hand-built table whose entries with prob < 1 have alias -1: the coins above prob pick -1, copied verbatim (and
    never re-drawn: -1 is in no used-set)."""
    keys, prob, alias = np.array([4, 9, 13]), np.array([0.25, 1.0, 0.5]), np.array([-1, -1, 9])
    used = [{9}, {4, 13}, set()]
    indptr, items = _csr(used, 3)
    table, _keep = _device_table(keys, prob, alias)
    ref, dev = _states(1, 300)
    uk = np.arange(3).repeat(400)
    got = dev.sample_pop(table, torch.from_numpy(uk), 1, indptr, items).cpu().numpy()
    want = sample_by_key_ids(ref, (keys, prob, alias), uk, 1, used)
    np.testing.assert_array_equal(got, want)
    assert (got == -1).sum() > 0
    _check_state(dev, ref)


def test_prob_equal_to_a_coin_takes_the_alias():
    """prob[idx] == coin exactly: `prob > coin` is false and the alias is taken (the coin is fp64, rounded nowhere)."""
    keys, prob, alias = np.array([5, 6, 7, 8]), np.array([0.5, 0.5, 0.5, 0.5]), np.array([8, 8, 8, 8])
    ref, dev = _states(3, 620)
    peek = np.random.RandomState()
    peek.set_state(ref.get_state())
    idx0 = peek.randint(0, 4, 50)[0]
    coin0 = peek.random_sample(50)[0]
    prob = prob.copy()
    prob[idx0] = coin0
    table, _keep = _device_table(keys, prob, alias)
    got = dev.sample_pop(table, torch.zeros(50, dtype=torch.int64), 1, None, None).cpu().numpy()
    want = sample_by_key_ids(ref, (keys, prob, alias), np.zeros(50, np.int64), 1, None)
    np.testing.assert_array_equal(got, want)
    assert got[0] == alias[idx0]
    _check_state(dev, ref)


@pytest.mark.parametrize("n", [1, 1000, 5000])
def test_without_used_sets_is_plain_pop_sampling(n):
    rng = np.random.default_rng(n)
    w = np.linspace(1, 5, 299)
    tab = alias_table(rng.choice(np.arange(1, 300), 2000, p=w / w.sum()))
    table, _keep = _device_table(*tab)
    ref, dev = _states(n, 623)
    got = dev.sample_pop(table, torch.zeros(n, dtype=torch.int64), 1, None, None).cpu().numpy()
    np.testing.assert_array_equal(got, pop_sampling(ref, tab, n))
    _check_state(dev, ref)


@pytest.mark.parametrize("n_calls,lo,hi", [(1, 5, 40), (15, 5, 40), (16, 5, 40), (17, 1, 700), (2821, 101, 303)])
def test_call_sequences(n_calls, lo, hi):
    """fr_sample_negatives_pop_calls: consecutive single-key calls, each finishing its rounds before the next draws."""
    rng = np.random.default_rng(n_calls)
    n_users = 3000
    tab, used = _world(rng, n_users, 2000, 60000, skew=1.0, heavy=(1, 2))
    call_keys = rng.integers(0, n_users, n_calls)
    call_keys[: min(n_calls, 2)] = [1, 2][: min(n_calls, 2)]
    counts = rng.integers(lo, hi + 1, n_calls)
    indptr, items = _csr(used, n_users)
    table, _keep = _device_table(*tab)
    ref, dev = _states(n_calls, 622)
    got = dev.sample_calls_pop(table, torch.from_numpy(call_keys), torch.from_numpy(counts), indptr, items).cpu().numpy()
    want = np.concatenate([sample_by_key_ids(ref, tab, [u], int(c), used) for u, c in zip(call_keys, counts)])
    np.testing.assert_array_equal(got, want)
    _check_state(dev, ref)


def test_out_of_range_user_sets_the_index_flag():
    from fairrec import _C
    rng = np.random.default_rng(1)
    tab, used = _world(rng, 10, 100, 500)
    indptr, items = _csr(used, 10)
    table, _keep = _device_table(*tab)
    _, dev = _states(4, 100)
    dev.sample_pop(table, torch.tensor([1, 2, 10, 3]), 2, indptr, items)
    assert int(dev.err_flag.item()) & _C.DEV_ERR_INDEX_RANGE
    _, dev = _states(4, 100)
    dev.sample_calls_pop(table, torch.tensor([1, -1]), torch.tensor([3, 3]), indptr, items)
    assert int(dev.err_flag.item()) & _C.DEV_ERR_INDEX_RANGE


# ---- the Sampler ------------------------------------------------------------------------------------------------------
class _DS:
    uid_field, iid_field = "user_id", "item_id"

    def __init__(self, user_num, item_num, u, i):
        self.user_num, self.item_num = user_num, item_num
        self.inter_feat = {"user_id": torch.from_numpy(np.asarray(u, np.int64)),
                           "item_id": torch.from_numpy(np.asarray(i, np.int64))}


def _phases(rng, n_users=60, n_items=200):
    mk = lambda n: _DS(n_users, n_items, rng.integers(1, n_users, n), np.minimum(rng.zipf(1.3, n), n_items - 1))
    return [mk(3000), mk(400), mk(400)]


def _used(dss, n_users=60):
    used = [set() for _ in range(n_users)]
    for d in dss:
        for u, i in zip(d.inter_feat["user_id"].tolist(), d.inter_feat["item_id"].tolist()):
            used[u].add(i)
    return used


def test_sampler_draws_on_the_device_without_numpy_state(monkeypatch):
    """Sampler('popularity').sample_by_user_ids hands no state to numpy (the host path did, every call): numpy's
    get_state / set_state raising changes nothing, and the ids are the restatement's."""
    from fairrec.sampler import DeviceRandomState, Sampler
    rng = np.random.default_rng(5)
    dss = _phases(rng)
    rs = DeviceRandomState(DEV, 2024)
    sampler = Sampler(["train", "valid", "test"], dss, "popularity", device=DEV, random_state=rs).set_phase("valid")
    tab = alias_table(np.concatenate([d.inter_feat["item_id"].numpy() for d in dss]))
    used = _used(dss[:2])
    ref = np.random.RandomState(2024)

    def boom(*a, **k):
        raise AssertionError("numpy's global generator state was handed over")

    users = rng.integers(1, 60, 512)
    monkeypatch.setattr(np.random, "get_state", boom)
    monkeypatch.setattr(np.random, "set_state", boom)
    got = [sampler.sample_by_user_ids(torch.from_numpy(users).to(DEV), None, num) for num in (1, 2, 1)]
    monkeypatch.undo()
    for g, num in zip(got, (1, 2, 1)):
        np.testing.assert_array_equal(g.cpu().numpy(), sample_by_key_ids(ref, tab, users, num, used))
    _check_state(rs, ref)


def test_sampler_sample_calls_and_set_distribution():
    from fairrec.sampler import DeviceRandomState, Sampler
    rng = np.random.default_rng(9)
    dss = _phases(rng)
    rs = DeviceRandomState(DEV, 99)
    sampler = Sampler(["train", "valid", "test"], dss, device=DEV, random_state=rs)
    assert sampler.distribution == "uniform"
    sampler.set_distribution("popularity")
    test = sampler.set_phase("test")
    tab = alias_table(np.concatenate([d.inter_feat["item_id"].numpy() for d in dss]))
    used = _used(dss)
    keys, counts = np.arange(1, 60), rng.integers(1, 50, 59)
    got = test.sample_calls(torch.from_numpy(keys), torch.from_numpy(counts)).cpu().numpy()
    ref = np.random.RandomState(99)
    want = np.concatenate([sample_by_key_ids(ref, tab, [u], int(c), used) for u, c in zip(keys, counts)])
    np.testing.assert_array_equal(got, want)
    _check_state(rs, ref)
    with pytest.raises(NotImplementedError):
        sampler.set_distribution("zipf")


def test_support_guard_refuses_before_any_launch():
    """A user whose used-set holds every key of the table: the reference's loop never ends; refused on the host."""
    from fairrec.sampler import DeviceRandomState, Sampler
    rs = DeviceRandomState(DEV, 3)
    st0 = rs.get_state()
    u = np.array([1] * 10 + [2, 3, 4])
    i = np.array(list(range(1, 11)) + [1, 1, 2])
    ds = _DS(6, 50, u, i)                              # 50 items in the catalogue, 10 of them ever interacted with
    with pytest.raises(ValueError, match="popularity"):
        Sampler("train", ds, "popularity", device=DEV, random_state=rs)
    s = Sampler("train", ds, "uniform", device=DEV, random_state=rs)
    with pytest.raises(ValueError, match="popularity"):
        s.set_distribution("popularity")
    torch.cuda.synchronize()
    st = rs.get_state()
    np.testing.assert_array_equal(st[1], st0[1])
    assert st[2] == st0[2]

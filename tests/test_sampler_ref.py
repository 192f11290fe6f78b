"""CPU: tests/sampler_ref.py -- the numpy reference of the sampler's call sequences -- against the oracle (its own MT19937)
and the reference's golden vectors, and its model of the speculative resolver against hand-worked sequences."""
import glob
import os

import numpy as np
import pytest

import sampler_ref as R
from oracle import sampler as OS

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
UNIFORM = [p for p in sorted(glob.glob(os.path.join(GOLDEN, "sampler_*.npz")))
           if "distribution" not in np.load(p).files or str(np.load(p)["distribution"]) == "uniform"]


def _csr(sets, n_users):
    indptr = np.zeros(n_users + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(sets.get(u, ())) for u in range(n_users)])
    items = np.array([i for u in range(n_users) for i in sorted(sets.get(u, ()))], dtype=np.int32)
    return indptr, items


def _case(seed=3, n_users=30, item_num=40):
    rng = np.random.default_rng(seed)
    sets = {u: set(rng.choice(np.arange(1, item_num), size=int(rng.integers(0, item_num - 3)), replace=False).tolist())
            for u in range(1, n_users)}
    sets[5] = set(range(1, item_num - 1))          # one item left: long rejection chains
    sets[0] = sets[6] = set()
    return sets, _csr(sets, n_users)


def _same_state(a, b):
    return np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_calls_ref_equals_consecutive_oracle_calls():
    sets, used = _case()
    keys = np.array([1, 5, 6, 5, 9, 0, 29, 5], dtype=np.int64)
    counts = np.array([7, 3, 0, 1, 650, 2, 1, 700], dtype=np.int64)
    rs, ors = np.random.RandomState(17), OS.MT19937(17)
    ids, consumed, first_hit = R.calls_ref(rs, 1, 40, keys, counts, used)
    want = np.concatenate([OS.sample_by_key_ids(ors, [k], int(c), sets, 40) for k, c in zip(keys, counts) if c])
    np.testing.assert_array_equal(ids, want)
    assert _same_state(rs.get_state(), ors.get_state())
    assert (consumed >= counts).all() and consumed[2] == 0 and first_hit[2] == -1
    assert consumed[1] > counts[1] and first_hit[7] >= 0          # user 5 collides
    # what the calls consumed is what the stream advanced by: the same number of accepted values drawn in one go
    rs2 = np.random.RandomState(17)
    rs2.randint(1, 40, int(consumed.sum()))
    assert _same_state(rs.get_state(), rs2.get_state())


@pytest.mark.parametrize("num", [1, 3])
def test_by_key_ids_ref_equals_oracle(num):
    sets, used = _case(seed=4)
    keys = np.random.default_rng(0).integers(1, 30, 257)
    rs, ors = np.random.RandomState(5), OS.MT19937(5)
    for _ in range(2):
        np.testing.assert_array_equal(R.by_key_ids_ref(rs, 1, 40, keys, num, used), OS.sample_by_key_ids(ors, keys, num, sets, 40))
    assert _same_state(rs.get_state(), ors.get_state())


def test_out_of_range_keys_have_no_used_set():
    _, used = _case()
    rs, rs2 = np.random.RandomState(1), np.random.RandomState(1)
    ids, consumed, _ = R.calls_ref(rs, 1, 40, [-1, 30], [5, 6], used)
    np.testing.assert_array_equal(ids, rs2.randint(1, 40, 11))
    np.testing.assert_array_equal(consumed, [5, 6])


@pytest.mark.parametrize("path", UNIFORM, ids=[os.path.basename(p)[8:-4] for p in UNIFORM])
def test_by_key_ids_ref_reproduces_reference_golden(path):
    z = np.load(path)
    item_num, user_num = int(z["item_num"]), int(z["user_num"])
    pairs = np.unique(z["train_user"].astype(np.int64) * item_num + z["train_item"])
    indptr = np.zeros(user_num + 1, dtype=np.int64)
    np.cumsum(np.bincount(pairs // item_num, minlength=user_num), out=indptr[1:])
    used = (indptr, (pairs % item_num).astype(np.int32))
    rs = np.random.RandomState(int(z["seed"]))
    for c in range(int(z["n_calls"])):
        np.testing.assert_array_equal(R.by_key_ids_ref(rs, 1, item_num, z[f"users{c}"], int(z[f"num{c}"]), used), z[f"neg{c}"])
    st = rs.get_state()
    np.testing.assert_array_equal(st[1], z["final_key"])
    assert st[2] == int(z["final_pos"])


@pytest.mark.parametrize("total,max_call", [(1, 1), (100, 7), (1500, 303), (280_300, 300), (8_000_000, 1 << 20)])
def test_workspace_layout_restates_the_library(total, max_call):
    from fairrec import _C
    lib = _C.lib()
    assert R.calls_workspace_bytes(total, max_call) == lib.fr_sample_negatives_calls_workspace_bytes(total, max_call)
    ws = lib.fr_sample_negatives_calls_workspace_bytes(total, max_call)
    assert R.lo_t_for(ws, max_call) >= total
    assert R.lo_t_for(ws - 1, max_call) < total


def test_accepted_available_counts_the_stream():
    rs = np.random.RandomState(2)
    st = rs.get_state()
    n = R.accepted_available(st, 1, 258, 3000, 3000)          # span 256: the worst acceptance rate
    assert n == 3000 + 1024                                   # the estimate leaves enough blocks here
    # the resolver's slack = the accepted values in the blocks the twist kernel keeps; never above what was wanted
    assert R.accepted_available(st, 1, 3, 10, 10) == 10 + 1024


# ---- spec_model on hand-worked sequences ----------------------------------------------------------------------------------
def test_model_no_collision():
    m = R.spec_model(np.full(20, 10), np.zeros(20, dtype=np.int64))
    assert m.speculative and m.path == "speculative" and m.collided == [] and (m.D == 0).all() and m.restart_at is None


def test_model_shift_31_at_the_last_call():
    extra = np.zeros(20, dtype=np.int64)
    extra[[3, 10, 19]] = [10, 20, 1]
    m = R.spec_model(np.full(20, 10), extra)
    assert m.path == "speculative" and m.collided == [3, 10, 19]
    np.testing.assert_array_equal(m.D, [0] * 3 + [10] * 7 + [30] * 9 + [31])


@pytest.mark.parametrize("at", [10, 19])
def test_model_shift_32_exactly_restarts(at):
    extra = np.zeros(20, dtype=np.int64)
    extra[[3, at]] = [12, 20]
    m = R.spec_model(np.full(20, 10), extra)
    assert m.path == "restart" and m.restart_reason == "shift" and m.restart_at == at
    assert m.D[at] == 32 and (m.D[at + 1:] == -1).all()


def test_model_one_call_consuming_40_extra_restarts():
    extra = np.zeros(20, dtype=np.int64)
    extra[5] = 40
    m = R.spec_model(np.full(20, 100), extra)
    assert m.path == "restart" and m.restart_at == 5 and m.collided == [5]


def test_model_thresholds():
    assert R.spec_model(np.full(15, 10), np.zeros(15)).path == "call_by_call"
    assert R.spec_model(np.full(16, 10), np.zeros(16)).path == "speculative"
    assert R.spec_model(np.full(16, 10), np.zeros(16), span=0).path == "call_by_call"
    assert R.spec_model(np.full(16, 10), np.zeros(16), lo_t=15).path == "call_by_call"
    m = R.spec_model(np.full(16, 10), np.zeros(16), lo_t=16)                # room for the calls, not for the total
    assert m.path == "restart" and m.restart_reason == "capacity" and m.restart_at == -1
    m = R.spec_model(np.full(16, 10), np.zeros(16), n_acc=159)
    assert m.path == "restart" and m.restart_reason == "slack"


def test_model_window_straddle():
    counts, extra, first_hit = np.full(20, 4000), np.zeros(20, dtype=np.int64), np.full(20, -1)
    extra[16], first_hit[16] = 2, 2000                      # call 16 = [64 000, 68 000), first hit at 66 000
    m = R.spec_model(counts, extra, first_hit)
    assert m.path == "speculative" and m.straddles == [(16, 65536)]
    first_hit[16] = 0                                       # ... at 64 000: found in the first window
    assert R.spec_model(counts, extra, first_hit).straddles == []

"""CPU: the optimizer state of the four learners as a checkpoint sees it -- what `FusedLazyOptimizer.state_dict` writes,
that the stock torch optimizer accepts it, and what `load_state_dict` does with an entry that is there and with one that
is not (per learner, for a lazy table and for a dense tensor).

No device: a stub engine with CPU tensors, one 5x3 table and one 4-element dense tensor; a "stepped" optimizer is one
whose step counts and state arrays were set by hand (state_dict / load_state_dict launch nothing on a table that is not
dirty).  Everything here is equality."""
import pytest
import torch

from fairrec.engine import GenericEngine
from fairrec.optim import FusedLazyAdagrad, FusedLazyAdam, FusedLazyRMSprop, FusedLazySGD

TABLE, DENSE = "emb.weight", "mlp.bias"
NAMES = [TABLE, DENSE]

# learner -> (fused class, stock class, its kwargs, torch's names of the state arrays kept in m and v)
LEARNERS = {
    "adam": (FusedLazyAdam, torch.optim.Adam, dict(lr=1e-3, weight_decay=1e-4), ("exp_avg", "exp_avg_sq")),
    "sgd": (FusedLazySGD, torch.optim.SGD, dict(lr=1e-2, weight_decay=1e-4), (None, None)),
    "adagrad": (FusedLazyAdagrad, torch.optim.Adagrad, dict(lr=1e-2, weight_decay=1e-4), ("sum", None)),
    "rmsprop": (FusedLazyRMSprop, torch.optim.RMSprop, dict(lr=1e-2, weight_decay=1e-4), ("square_avg", None)),
}
ADAM_GROUP_KEYS = {"lr", "weight_decay", "betas", "eps", "amsgrad", "maximize", "foreach", "capturable", "differentiable",
                   "fused", "params"}


class StubEngine(GenericEngine):
    """GenericEngine's bookkeeping without a device or the library."""

    def __init__(self):
        self.device = torch.device("cpu")
        self._tables, self._weights, self._dense, self._group, self._hyper_of = {}, {}, {}, {}, {}
        self.hyper = self.optimizer = self.sweep_period = None
        self._group_version = {}
        self._counters = None
        self._counter_slot, self._advance_idx, self._seg_src = {}, {}, {}


def make(learner, groups=(None,)):
    """An engine with one table and one dense tensor per group and the optimizer of `learner` bound to the first group."""
    eng = StubEngine()
    g = torch.Generator().manual_seed(0)
    for grp in groups:
        pre = "" if grp is None else grp + "."
        eng.add_table(pre + TABLE, torch.nn.Parameter(torch.randn(5, 3, generator=g)), group=grp)
        eng.add_dense(pre + DENSE, torch.nn.Parameter(torch.randn(4, generator=g)), group=grp)
    cls, _, kw, _ = LEARNERS[learner]
    extra = {} if groups[0] is None else {"group": groups[0]}
    return eng, cls(eng, **kw, **extra)


def entries(eng, pre=""):
    return eng._tables[pre + TABLE], eng._dense[pre + DENSE]


def step_by_hand(eng, pre="", t_step=3, d_step=2):
    """The table at step `t_step`, the dense tensor at `d_step`, every state array they keep filled with known values."""
    t, d = entries(eng, pre)
    t.ensure_state()
    t.step, d.step = t_step, d_step
    for k, x in enumerate((t.m, t.v, d.m, d.v)):
        if x is not None:
            x.copy_(torch.arange(x.numel(), dtype=torch.float32).reshape(x.shape) + 10.0 * (k + 1))
    t.last.fill_(t_step)


def snapshot(t, d):
    c = lambda x: None if x is None else x.clone()
    return dict(t_step=t.step, t_m=c(t.m), t_v=c(t.v), last=t.last.clone(), stamp=t.stamp.clone(), gen=t.stamp_gen,
                dirty=t._dirty, t_dev=c(t.step_dev), d_step=d.step, d_m=c(d.m), d_v=c(d.v), d_dev=c(d.step_dev))


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def attach_counters(t, d, stale=99):
    """Device-resident step counters (CPU tensors here) that hold a stale value: a load that refills them shows."""
    t.ensure_state()
    t.attach_step_counter(torch.zeros(1, dtype=torch.int32))
    d.step_dev = torch.zeros(1, dtype=torch.int32)
    t.step_dev.fill_(stale)
    d.step_dev.fill_(stale)


def assert_current(t, gen_before):
    """`last` = step everywhere, no stamps, look-ahead stamping void, device counter refilled, nothing left to flush."""
    assert (t.last == t.step).all() and (t.stamp == 0).all()
    assert t.stamp_gen == gen_before + 1 and t._dirty is False
    if t.step_dev is not None:
        assert int(t.step_dev) == t.step


def stock(learner):
    _, cls, kw, _ = LEARNERS[learner]
    return cls([torch.nn.Parameter(torch.zeros(5, 3)), torch.nn.Parameter(torch.zeros(4))], **kw)


@pytest.mark.parametrize("learner", list(LEARNERS))
def test_fresh_state_dict(learner):
    eng, opt = make(learner)
    m_name, v_name = LEARNERS[learner][3]
    sd = opt.state_dict(param_names=NAMES)
    want = {"adam": [0, 1], "adagrad": [0, 1], "rmsprop": [], "sgd": []}[learner]
    assert sorted(sd["state"]) == want
    for k, shape in zip(want, ((5, 3), (4,))):
        st = sd["state"][k]
        assert set(st) == {"step"} | {n for n in (m_name, v_name) if n}
        assert float(st["step"]) == 0.0
        for n in (m_name, v_name):
            if n:
                assert st[n].shape == shape and (st[n] == 0).all()
    (group,) = sd["param_groups"]
    assert group["params"] == [0, 1]
    if learner == "adam":
        assert set(group) == ADAM_GROUP_KEYS
    else:
        assert set(group) == set(stock(learner).param_groups[0])
    # the name-keyed layout: the optimizer's own arguments and the names that have state
    by_name = opt.state_dict()
    assert list(by_name["state"]) == [NAMES[k] for k in want]
    assert by_name["param_groups"][0]["params"] == [NAMES[k] for k in want]
    assert set(by_name["param_groups"][0]) == set(opt.defaults) | {"params"}
    stock(learner).load_state_dict(sd)


@pytest.mark.parametrize("learner", list(LEARNERS))
def test_stepped_state_dict_round_trip_through_torch(learner):
    eng, opt = make(learner)
    m_name, v_name = LEARNERS[learner][3]
    step_by_hand(eng)
    t, d = entries(eng)
    sd = opt.state_dict(param_names=NAMES)
    assert sorted(sd["state"]) == ([] if learner == "sgd" else [0, 1])
    for k, x in ((0, t), (1, d)):
        if learner == "sgd":
            break
        st = sd["state"][k]
        assert set(st) == {"step"} | {n for n in (m_name, v_name) if n}
        assert float(st["step"]) == x.step
        assert torch.equal(st[m_name], x.m)
        if v_name:
            assert torch.equal(st[v_name], x.v)
    ref = stock(learner)
    ref.load_state_dict(sd)
    back = ref.state_dict()

    eng2, opt2 = make(learner)
    t2, d2 = entries(eng2)
    attach_counters(t2, d2)
    t2._dirty = True
    gen = t2.stamp_gen
    opt2.load_state_dict(back, param_names=NAMES)
    if learner == "sgd":        # torch keeps no state: nothing to restore, the table is current as it stands
        assert t2.step == 0 and d2.step == 0 and int(d2.step_dev) == 0
    else:
        assert t2.step == 3 and d2.step == 2 and int(d2.step_dev) == 2
        assert torch.equal(t2.m, t.m) and torch.equal(d2.m, d.m)
        if v_name:
            assert torch.equal(t2.v, t.v) and torch.equal(d2.v, d.v)
    assert_current(t2, gen)
    # ... and its own name-keyed layout loads the same
    eng3, opt3 = make(learner)
    opt3.load_state_dict(opt.state_dict())
    t3, d3 = entries(eng3)
    if learner != "sgd":
        assert t3.step == 3 and d3.step == 2 and torch.equal(t3.m, t.m) and torch.equal(d3.m, d.m)
    assert_current(t3, 0)


@pytest.mark.parametrize("learner", list(LEARNERS))
def test_entry_absent_from_the_loaded_state(learner):
    eng, opt = make(learner)
    step_by_hand(eng)
    t, d = entries(eng)
    attach_counters(t, d)
    t._dirty = True
    t.stamp.fill_(7)
    before = snapshot(t, d)
    opt.load_state_dict({"state": {}, "param_groups": [{"params": []}]})
    after = snapshot(t, d)
    if learner == "adam":       # untouched, not even marked current
        same(before, after)
        return
    # tables: SGD and Adagrad keep step (and Adagrad its sum), RMSprop starts over; all are marked current
    if learner == "rmsprop":
        assert t.step == 0 and (t.m == 0).all()
    else:
        assert t.step == 3
        if learner == "adagrad":
            assert torch.equal(t.m, before["t_m"])
    assert_current(t, before["gen"])
    # dense tensors: step 0, the state they keep zeroed, device counter refilled
    assert d.step == 0 and int(d.step_dev) == 0
    if learner != "sgd":
        assert (d.m == 0).all()
    assert d.v is None and (d.m is None) == (learner == "sgd")


@pytest.mark.parametrize("learner", list(LEARNERS))
def test_group_optimizer_touches_only_what_it_owns(learner):
    eng, opt = make(learner, groups=("filter", "dis"))
    step_by_hand(eng, "filter.")
    step_by_hand(eng, "dis.", t_step=5, d_step=4)
    sd = opt.state_dict()
    assert list(sd["state"]) == ([] if learner == "sgd" else ["filter." + TABLE, "filter." + DENSE])

    eng2, opt2 = make(learner, groups=("filter", "dis"))
    step_by_hand(eng2, "dis.", t_step=5, d_step=4)
    other = entries(eng2, "dis.")
    attach_counters(*other)
    other[0]._dirty = True
    before = snapshot(*other)
    opt2.load_state_dict(sd)
    t, d = entries(eng, "filter.")
    t2, d2 = entries(eng2, "filter.")
    if learner != "sgd":
        assert t2.step == 3 and d2.step == 2 and torch.equal(t2.m, t.m) and torch.equal(d2.m, d.m)
    assert_current(t2, 0)
    same(before, snapshot(*other))
    # an empty state resets (RMSprop) or keeps (the others) the owned entries and leaves the other group alone
    opt2.load_state_dict({"state": {}, "param_groups": [{"params": []}]})
    same(before, snapshot(*other))
    if learner == "rmsprop":
        assert t2.step == 0 and d2.step == 0 and (t2.m == 0).all()

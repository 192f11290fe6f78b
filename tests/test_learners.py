"""CPU: the host side of the SGD / Adagrad / RMSprop learners of the lazy tables.

- the per-learner step-scalar tables against Python double arithmetic (torch/optim/{sgd,adagrad,rmsprop}.py);
- the fr_adam binding carries `learner`, and the library refuses what it does not run before touching a device: a FOCF
  entry point with a learner other than Adam, and any entry point with an unknown learner value;
- the trainer's learner dispatch errors that need no device."""
import ctypes
import logging

import numpy as np
import pytest

from fairrec import _C
from fairrec.optim import (LEARNER_ADAGRAD, LEARNER_ADAM, LEARNER_RMSPROP, LEARNER_SGD, AdagradHyper, RMSpropHyper,
                           SGDHyper, adagrad_step_scalars, rmsprop_step_scalars, sgd_step_scalars)


def test_learner_ids_match_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "fairrec_hip.h")).read()
    ids = {k: int(v) for k, v in re.findall(r"#define FR_LEARNER_(\w+) (\d+)", text)}
    assert ids == {"ADAM": LEARNER_ADAM, "SGD": LEARNER_SGD, "ADAGRAD": LEARNER_ADAGRAD, "RMSPROP": LEARNER_RMSPROP}


def test_fr_adam_binding_has_learner_and_keeps_its_size():
    names = [f[0] for f in _C.FrAdam._fields_]
    assert names == ["scalars", "cap", "learner", "weight_decay", "beta1", "beta2", "eps"]
    assert ctypes.sizeof(_C.FrAdam) == 48


@pytest.mark.parametrize("lr,wd", [(1e-3, 0.0), (1e-3, 1e-3), (0.05, 0.3), (7e-4, 1e-5)])
def test_sgd_scalars(lr, wd):
    cap = 5
    tab = sgd_step_scalars(lr, wd, cap)
    assert tab.dtype == np.float32 and tab.shape == (4 * (cap + 1),)
    assert (tab[:4] == 0).all()
    for j in range(1, cap + 1):
        assert tab[4 * j] == np.float32(lr)
        assert tab[4 * j + 1] == np.float32(-(lr * wd))
        assert tab[4 * j + 2] == 0 and tab[4 * j + 3] == 0


@pytest.mark.parametrize("lr,decay", [(1e-2, 0.0), (1e-3, 0.1), (0.5, 1e-4)])
def test_adagrad_scalars(lr, decay):
    cap = 9
    tab = adagrad_step_scalars(lr, decay, cap)
    for j in range(1, cap + 1):
        assert tab[4 * j] == np.float32(lr / (1 + (j - 1) * decay))
        assert (tab[4 * j + 1:4 * j + 4] == 0).all()


def test_rmsprop_scalars():
    tab = rmsprop_step_scalars(3e-3, 4)
    assert (tab[4::4] == np.float32(3e-3)).all() and (tab[:4] == 0).all()
    assert (tab.reshape(-1, 4)[:, 1:] == 0).all()


def test_hyper_structs_without_device():
    s = SGDHyper(0.01, 1e-3, device="cpu")
    assert s.c().learner == LEARNER_SGD and s.c().cap == 1 and s.saturated
    assert s.c().weight_decay == 1e-3
    a = AdagradHyper(0.01, weight_decay=0.5, device="cpu")
    assert a.c().learner == LEARNER_ADAGRAD and a.c().eps == 1e-10 and a.cap == 1
    a2 = AdagradHyper(0.01, lr_decay=0.25, device="cpu")
    assert a2.cap > 1 and a2.host_scalars[4 * 3] == np.float32(0.01 / (1 + 2 * 0.25))
    r = RMSpropHyper(0.02, weight_decay=1e-4, device="cpu")
    assert r.c().learner == LEARNER_RMSPROP and r.c().beta2 == 0.99 and r.c().eps == 1e-8
    s.check_step(10 ** 6)           # constant scalars: any step


def _fake_table(m=True, v=True):
    buf = ctypes.c_void_p(4096)      # never dereferenced: every call below must fail its argument check first
    return _C.FrTable(buf.value, buf.value if m else None, buf.value if v else None, buf.value, buf.value, 10, 8, 1, None)


def test_focf_refuses_other_learners_before_device_work():
    lib = _C.lib()
    U, I = _fake_table(), _fake_table()
    for learner in (LEARNER_SGD, LEARNER_ADAGRAD, LEARNER_RMSPROP):
        adam = _C.FrAdam(4096, 1, learner, 0.0, 0.9, 0.999, 1e-8)
        rc = lib.fr_focf_step(ctypes.byref(U), ctypes.byref(I), ctypes.byref(adam), None, None, None, None, 8, 0, 1.0, 0,
                              1, None, 0, None, None, 0, None, None, None, None)
        assert rc == -1, rc
        assert b"adam only" in lib.fr_last_error()


def test_unknown_learner_is_refused():
    lib = _C.lib()
    t = _fake_table()
    for learner in (-1, 4, 99):
        adam = _C.FrAdam(4096, 1, learner, 0.0, 0.9, 0.999, 1e-8)
        assert lib.fr_table_flush(ctypes.byref(t), ctypes.byref(adam), None) == -1
        assert b"unknown learner" in lib.fr_last_error()
        U = _fake_table()
        rc = lib.fr_focf_step(ctypes.byref(U), ctypes.byref(t), ctypes.byref(adam), None, None, None, None, 8, 0, 1.0, 0,
                              1, None, 0, None, None, 0, None, None, None, None)
        assert rc == -1 and b"unknown learner" in lib.fr_last_error()


def test_state_arrays_each_learner_needs():
    lib = _C.lib()
    for learner, need_m, need_v in ((LEARNER_ADAM, True, True), (LEARNER_SGD, False, False),
                                    (LEARNER_ADAGRAD, True, False), (LEARNER_RMSPROP, True, False)):
        adam = _C.FrAdam(4096, 1, learner, 0.0, 0.9, 0.999, 1e-8)
        # without m: refused exactly when the learner keeps m (the call with M = 0 then returns before any launch)
        t = _fake_table(m=False, v=True)
        rc = lib.fr_table_gather(ctypes.byref(t), ctypes.byref(adam), 4096, 0, 4096, None, None)
        assert (rc == -1) == need_m, (learner, rc)
        t = _fake_table(m=True, v=False)
        rc = lib.fr_table_gather(ctypes.byref(t), ctypes.byref(adam), 4096, 0, 4096, None, None)
        assert (rc == -1) == need_v, (learner, rc)


def test_trainer_learner_names(caplog):
    from fairrec.trainer.trainer import Trainer
    from fairrec.optim import FusedLazyAdagrad, FusedLazyRMSprop, FusedLazySGD
    tr = Trainer.__new__(Trainer)
    tr.logger = logging.getLogger("test_learners")
    assert tr._learner_class("SGD") is FusedLazySGD
    assert tr._learner_class("Adagrad") is FusedLazyAdagrad
    assert tr._learner_class("rmsprop") is FusedLazyRMSprop
    with pytest.raises(ValueError, match="SparseAdam"):
        tr._learner_class("sparse_adam")
    with caplog.at_level(logging.WARNING, logger="test_learners"):
        assert tr._learner_class("lbfgs") is None
    assert "unrecognized optimizer" in caplog.text

"""CPU: the host side of `full_sort_eval: fused` (fr_recommend_cells / fr_recommend_meanrank, csrc/recommend.hip).

- both entries refuse what they do not run before any device work (fake pointers that are never dereferenced);
- the config key is validated when the trainer is built, `fused` with a list longer than FR_TOPK_MAX - 1 included;
- tests/full_eval_ref.py's restatement of the `rec.meanrank` triple agrees with a hand-worked example."""
import ctypes

import numpy as np
import pytest

import full_eval_ref as E
from fairrec import _C

P = 4096        # a pointer that is never dereferenced: every refused call fails its argument check first


def _args(**kw):
    f = dict(X=P, W=P, user_bias=None, item_bias=None, hist_indptr=None, hist_items=None, scores_out=None, n_users=8, n_items=10,
             hist_len=0, dim=4, k=0, epilogue=0, mask_pad=1, hist_sorted=1, slices=0, bias0=0.0, scale=1.0)
    f.update(kw)
    return _C.FrRecArgs(*[f[name] for name, _ in _C.FrRecArgs._fields_])


BAD_ARGS = [dict(X=None), dict(W=None), dict(dim=0), dict(dim=257), dict(n_users=-1), dict(n_items=0), dict(epilogue=3),
            dict(epilogue=1, scale=0.0), dict(hist_indptr=P, hist_items=P, hist_len=3, hist_sorted=0),
            dict(hist_indptr=P, hist_items=None, hist_len=3), dict(hist_indptr=P, hist_items=P, hist_len=-1)]


def test_cells_refuses_before_device_work():
    lib = _C.lib()
    for bad in BAD_ARGS:
        assert lib.fr_recommend_cells(ctypes.byref(_args(**bad)), P, P, 5, P, P, None) == -1, bad
        assert lib.fr_last_error()
    a = _args()
    assert lib.fr_recommend_cells(None, P, P, 5, P, P, None) == -1
    assert lib.fr_recommend_cells(ctypes.byref(a), None, P, 5, P, P, None) == -1
    assert lib.fr_recommend_cells(ctypes.byref(a), P, None, 5, P, P, None) == -1
    assert lib.fr_recommend_cells(ctypes.byref(a), P, P, 5, None, P, None) == -1
    assert lib.fr_recommend_cells(ctypes.byref(a), P, P, 5, P, None, None) == -1 and b"null" in lib.fr_last_error()
    assert lib.fr_recommend_cells(ctypes.byref(a), P, P, -1, P, P, None) == -1
    assert lib.fr_recommend_cells(ctypes.byref(_args(n_users=0)), P, P, 5, P, P, None) == -1
    assert lib.fr_recommend_cells(ctypes.byref(a), None, None, 0, None, P, None) == 0        # no cells: nothing to do
    assert lib.fr_recommend_cells(ctypes.byref(_args(k=999, slices=-7, scores_out=P)), None, None, 0, None, P, None) == 0


def test_meanrank_refuses_before_device_work():
    lib = _C.lib()
    for bad in BAD_ARGS:
        assert lib.fr_recommend_meanrank(ctypes.byref(_args(**bad)), P, 5, P, P, 64, P, None) == -1, bad
        assert lib.fr_recommend_meanrank_workspace_bytes(ctypes.byref(_args(**bad)), 5) == 0
    a = _args()
    need = lib.fr_recommend_meanrank_workspace_bytes(ctypes.byref(a), 5)
    assert need == 20 and lib.fr_recommend_meanrank_workspace_bytes(ctypes.byref(a), 0) == 0
    assert lib.fr_recommend_meanrank_workspace_bytes(ctypes.byref(a), -1) == 0
    assert need == lib.fr_recommend_meanrank_workspace_bytes(ctypes.byref(_args(n_users=10 ** 6, n_items=10 ** 6)), 5)   # not users x items
    assert lib.fr_recommend_meanrank(None, P, 5, P, P, 64, P, None) == -1
    assert lib.fr_recommend_meanrank(ctypes.byref(a), None, 5, P, P, 64, P, None) == -1
    assert lib.fr_recommend_meanrank(ctypes.byref(a), P, 5, None, P, 64, P, None) == -1
    assert lib.fr_recommend_meanrank(ctypes.byref(a), P, 5, P, P, 64, None, None) == -1
    assert lib.fr_recommend_meanrank(ctypes.byref(a), P, 5, P, None, 64, P, None) == -1
    assert lib.fr_recommend_meanrank(ctypes.byref(a), P, 5, P, P, need - 1, P, None) == -1 and b"workspace" in lib.fr_last_error()
    assert lib.fr_recommend_meanrank(ctypes.byref(a), P, 5, P, P + 2, 64, P, None) == -1        # misaligned
    assert lib.fr_recommend_meanrank(ctypes.byref(a), P, -1, P, P, 64, P, None) == -1
    assert lib.fr_recommend_meanrank(ctypes.byref(_args(n_users=0)), None, 0, P, None, 0, P, None) == 0      # no users: nothing to do


class _NoOptimizer:
    def _build_optimizer(self, **kwargs):
        return None


def _trainer(tmp_path, **extra):
    from fairrec.config import Config
    from fairrec.trainer.trainer import Trainer

    class T(_NoOptimizer, Trainer):
        pass

    cfg = Config(config_dict=dict({"device": "cpu", "checkpoint_dir": str(tmp_path), "model": "FOCF", "topk": [5, 10]}, **extra))
    return T(cfg, object()), cfg


def test_config_key_is_validated_when_the_trainer_is_built(tmp_path):
    from fairrec.trainer.trainer import full_sort_eval_of
    tr, cfg = _trainer(tmp_path)
    assert cfg["full_sort_eval"] == "matrix" and tr.full_sort_eval == "matrix"          # the default of overall.yaml
    assert _trainer(tmp_path, full_sort_eval="fused")[0].full_sort_eval == "fused"
    assert _trainer(tmp_path, full_sort_eval="matrix", topk=[300])[0].full_sort_eval == "matrix"     # matrix: any list length
    for bad in ("dense", "Fused", "", 1, True):
        with pytest.raises(ValueError, match="full_sort_eval"):
            _trainer(tmp_path, full_sort_eval=bad)
    bare = type("Bare", (dict,), {"__getitem__": dict.get})       # a hand-built config that does not carry the key
    assert full_sort_eval_of(bare()) == "matrix" and full_sort_eval_of(bare(full_sort_eval="fused", topk=10)) == "fused"


@pytest.mark.parametrize("topk", [256, [10, 256], [1000]])
def test_fused_refuses_a_list_longer_than_the_kernel_selects(tmp_path, topk):
    assert _C.FR_TOPK_MAX == 256
    with pytest.raises(ValueError, match="255"):
        _trainer(tmp_path, full_sort_eval="fused", topk=topk)
    assert _trainer(tmp_path, full_sort_eval="fused", topk=[10, 255])[0].full_sort_eval == "fused"


def test_filtered_trainers_validate_the_key_too(tmp_path):
    from fairrec.config import Config
    from fairrec.trainer.trainer import PFCNTrainer

    class T(_NoOptimizer, PFCNTrainer):
        pass

    cfg = dict(device="cpu", checkpoint_dir=str(tmp_path), model="PFCN_BiasedMF", filter_mode="none", topk=[10])
    assert T(Config(config_dict=dict(cfg, full_sort_eval="fused")), object()).full_sort_eval == "fused"
    with pytest.raises(ValueError, match="full_sort_eval"):
        T(Config(config_dict=dict(cfg, full_sort_eval="topk")), object())


def test_restatement_on_a_hand_worked_example():
    inf = np.inf
    s = np.array([[-inf, 0.5, 0.5, 0.2, -inf, 0.9],       # positives 1 (ties with 2) and 5
                  [-inf, 0.1, -inf, 0.3, 0.2, 0.4],       # positives 2 (a masked cell) and 4
                  [-inf, 0.7, 0.6, 0.5, 0.4, 0.3]],       # no positive
                 np.float32)
    keys = np.array([0 * 6 + 1, 0 * 6 + 5, 0 * 6 + 5, 1 * 6 + 2, 1 * 6 + 4, 3 * 6 + 1], np.int64)     # one twice, one beyond
    # user 0: item 1 has 1 cell above and 2 equal (itself included): 2 * rank = 2 + 2 + 1 = 5 (rank 2.5); item 5 is first: 0 + 1 + 1
    # user 1: item 2 is masked: the 4 live cells rank above it, 8 + 0 + 1; item 4 has 2 above: 4 + 1 + 1
    want = np.array([[5 + 2, 4, 2], [9 + 6, 4, 2], [0, 5, 0]], np.int64)
    got = E.meanrank(s, keys)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(E.meanrank(s, keys[::-1]), want)          # the restatement sorts for itself
    assert np.array_equal(E.meanrank(s, np.zeros(0, np.int64)), [[0, 4, 0], [0, 4, 0], [0, 5, 0]])

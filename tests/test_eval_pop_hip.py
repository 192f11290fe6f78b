"""GPU: `eval_args.mode: popN` -- the negative-sampled ranking evaluation with popularity-biased negatives drawn on the device
-- and training with `neg_sampling: {popularity: N}` (plain and dynamic) draw the numpy restatement's ids
(tests/test_sampler_pop_hip.py: RandomState + the reference's alias table and rejection loop), batch by batch."""
import numpy as np
import pytest
import torch

import test_sampler_pop_hip as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _used_sets(csr, n_users):
    indptr, items, _ = csr
    ip, it = indptr.cpu().numpy(), items.cpu().numpy()
    return [set(it[ip[u]:ip[u + 1]].tolist()) for u in range(n_users)]


def test_pop_eval_loader_against_the_restated_loader():
    """popN loader: users in id order, per user [positives | N popularity-biased negatives per positive], the negatives from
    consecutive single-user sample_by_user_ids calls on ONE numpy stream.  A steep popularity skew makes a user's candidates
    repeat often."""
    from fairrec.config import Config
    from fairrec.data.dataloader import NegSampleEvalDataLoader
    from fairrec.data.dataset import InteractionDataset
    from fairrec.data.interaction import Interaction
    from fairrec.sampler import DeviceRandomState, Sampler
    rng = np.random.default_rng(3)
    n_users, n_items, N = 40, 120, 20
    cfg = Config(config_dict={"eval_batch_size": 2000, "device": DEV, "eval_args": {"mode": f"pop{N}"}})
    users = Interaction({"user_id": torch.arange(n_users), "gender": torch.from_numpy(rng.integers(0, 2, n_users).astype(np.float32))})
    w = 1.0 / np.arange(1, n_items) ** 1.5
    mk = lambda n: InteractionDataset(cfg, Interaction({"user_id": torch.from_numpy(rng.integers(1, n_users, n)),
                                                        "item_id": torch.from_numpy(rng.choice(np.arange(1, n_items), n,
                                                                                               p=w / w.sum()))}),
                                      users, n_users, n_items)
    train, test = mk(600), mk(150)
    tu, ti = test.inter_feat["user_id"].numpy().copy(), test.inter_feat["item_id"].numpy().copy()
    tab = R.alias_table(np.concatenate([train.inter_feat["item_id"].numpy(), ti]))
    used = [set() for _ in range(n_users)]
    for a, b in list(zip(train.inter_feat["user_id"].tolist(), train.inter_feat["item_id"].tolist())) + list(zip(tu.tolist(), ti.tolist())):
        used[a].add(int(b))
    rs = DeviceRandomState(DEV, 77)
    sampler = Sampler(["train", "test"], [train, test], "popularity", device=DEV, random_state=rs).set_phase("test")
    dl = NegSampleEvalDataLoader(cfg, test, sampler)
    order = np.argsort(tu, kind="stable")
    su, si = tu[order], ti[order]
    uid_list = np.unique(su)
    sizes = sorted((np.bincount(su, minlength=n_users)[uid_list] * (1 + N)).tolist(), reverse=True)
    step, tot = 1, sizes[0]
    for k in range(1, len(sizes)):
        if tot + sizes[k] > 2000:
            break
        step, tot = k + 1, tot + sizes[k]
    assert dl.step == step
    ref = np.random.RandomState(77)
    seen, dup = 0, 0
    for b, (inter, row_idx, pu, pi) in enumerate(dl):
        uids = uid_list[b * step:(b + 1) * step]
        exp_u, exp_i, exp_row, exp_pu, exp_pi = [], [], [], [], []
        for r, u in enumerate(uids):
            pos = si[su == u]
            neg = R.sample_by_key_ids(ref, tab, np.full(len(pos), u), N, used)
            dup += len(neg) - len(set(neg.tolist()))
            exp_u += [u] * (len(pos) * (1 + N))
            exp_i += list(pos) + list(neg)
            exp_row += [r] * (len(pos) * (1 + N))
            exp_pu += [r] * len(pos)
            exp_pi += list(pos)
        np.testing.assert_array_equal(inter["user_id"].cpu().numpy(), exp_u)
        np.testing.assert_array_equal(inter["item_id"].cpu().numpy(), exp_i)
        np.testing.assert_array_equal(row_idx.cpu().numpy(), exp_row)
        np.testing.assert_array_equal(pu.cpu().numpy(), exp_pu)
        np.testing.assert_array_equal(pi.cpu().numpy(), exp_pi)
        np.testing.assert_array_equal(inter["gender"].cpu().numpy(), users["gender"].numpy()[np.array(exp_u)])
        seen += len(uids)
    assert seen == len(uid_list)
    assert dup > len(uid_list)                   # duplicate candidates are common
    R._check_state(rs, ref)


# ---- run_recbole ------------------------------------------------------------------------------------------------------
def _record(monkeypatch):
    """Every Sampler.sample_calls / sample_by_user_ids call (the phase copy, the generator state before it, its arguments
    and ids), every NegSampleEvalDataLoader built, and the candidate list each alias table was built from."""
    from fairrec.data import dataloader as D
    from fairrec.sampler import sampler as S
    log = {"calls": [], "by_user": [], "loaders": []}
    calls, by_user, build, init = (S.Sampler.sample_calls, S.Sampler.sample_by_user_ids, S.Sampler._build_alias_table,
                                   D.NegSampleEvalDataLoader.__init__)

    def rec_calls(self, call_keys, counts):
        st = self.rs.get_state()
        out = calls(self, call_keys, counts)
        log["calls"].append((self, st, call_keys.cpu().numpy().copy(), counts.cpu().numpy().copy(), out.cpu().numpy()))
        return out

    def rec_by_user(self, user_ids, item_ids, num):
        st = self.rs.get_state()
        out = by_user(self, user_ids, item_ids, num)
        log["by_user"].append((self, st, torch.as_tensor(user_ids).cpu().numpy().copy(), int(num), out.cpu().numpy()))
        return out

    def rec_build(self):
        self._cand_for_test = np.concatenate([ds.inter_feat[self.iid_field].cpu().numpy() for ds in self.datasets])
        return build(self)

    def rec_init(self, *a, **k):
        init(self, *a, **k)
        log["loaders"].append(self)

    monkeypatch.setattr(S.Sampler, "sample_calls", rec_calls)
    monkeypatch.setattr(S.Sampler, "sample_by_user_ids", rec_by_user)
    monkeypatch.setattr(S.Sampler, "_build_alias_table", rec_build)
    monkeypatch.setattr(D.NegSampleEvalDataLoader, "__init__", rec_init)
    return log


def _restated_calls(entry):
    smp, st, keys, counts, _ = entry
    ref = np.random.RandomState()
    ref.set_state(st)
    used = _used_sets(smp.used_ids, smp.user_num)
    tab = R.alias_table(smp._cand_for_test)
    return np.concatenate([R.sample_by_key_ids(ref, tab, [u], int(c), used) for u, c in zip(keys, counts)])


class _Replay:
    """Stands in for a loader's sampler: sample_calls hands out the restatement's ids, call by call."""

    def __init__(self, sampler, ids):
        self.used_ids, self.distribution, self._ids = sampler.used_ids, sampler.distribution, list(ids)

    def sample_calls(self, call_keys, counts):
        return torch.from_numpy(self._ids.pop(0)).to(DEV)


MODELS = {"PFCN_PMF": dict(filter_mode="none"), "FOCF": dict(fair_objective="value")}


@pytest.mark.parametrize("model", sorted(MODELS))
def test_run_recbole_pop_evaluation(model, tmp_path, monkeypatch):
    from fairrec.quick_start import run_recbole
    seen = {}
    common = {"epochs": 1, "train_batch_size": 512, "synthetic_users": 120, "synthetic_items": 300, "synthetic_interactions": 3000,
              "device": DEV, "checkpoint_dir": str(tmp_path), "embedding_size": 16, "topk": [5, 10], "valid_metric": "ndcg@10",
              "valid_metric_bigger": True, "metrics": ["NDCG", "Recall", "Hit", "MRR", "DifferentialFairness", "NonParityUnfairness"],
              "sst_attr_list": ["gender"], "eval_batch_size": 2048, "metric_decimal_place": 4, **MODELS[model]}
    uni = run_recbole(model=model, config_dict=dict(common, eval_args={"mode": "uni20"}))["test_result"]
    log = _record(monkeypatch)

    def before_fit(m, trainer):
        seen["trainer"] = trainer

    out = run_recbole(model=model, config_dict=dict(common, eval_args={"mode": "pop20"}), before_fit=before_fit)
    monkeypatch.undo()
    pop = out["test_result"]
    assert pop is not None
    flat = lambda res: sorted(k for v in res.values() for k in v) if model == "PFCN_PMF" else sorted(res)
    assert flat(pop) == flat(uni)
    # every call of the valid and test loaders drew the restatement's ids
    assert log["calls"] and {e[0].phase for e in log["calls"]} == {"valid", "test"}
    assert all(e[0].distribution == "popularity" for e in log["calls"])
    restated = [_restated_calls(e) for e in log["calls"]]
    for e, want in zip(log["calls"], restated):
        np.testing.assert_array_equal(e[4], want)
    # the test result is Trainer.evaluate's on the test loader with the restatement's ids in place of the draws
    test_dl = [d for d in log["loaders"] if d.sampler.phase == "test"][-1]
    test_dl.sampler = _Replay(test_dl.sampler, [w for e, w in zip(log["calls"], restated) if e[0].phase == "test"])
    assert seen["trainer"].evaluate(test_dl) == pop


@pytest.mark.parametrize("neg", [{"popularity": 1}, {"popularity": 1, "dynamic": 2}], ids=["plain", "dynamic"])
def test_training_draws_the_restated_ids(neg, tmp_path, monkeypatch):
    """One epoch of PFCN_PMF with popularity-biased training negatives: every batch's draw is the restatement's."""
    from fairrec.quick_start import run_recbole
    log = _record(monkeypatch)
    run_recbole(model="PFCN_PMF", config_dict={
        "epochs": 1, "eval_step": 0, "train_batch_size": 256, "synthetic_users": 150, "synthetic_items": 200,
        "synthetic_interactions": 3000, "device": DEV, "checkpoint_dir": str(tmp_path), "embedding_size": 16,
        "filter_mode": "none", "neg_sampling": neg, "eval_args": {"mode": "full"}, "topk": [5], "valid_metric": "ndcg@5",
        "metrics": ["NDCG"]}, saved=False)
    monkeypatch.undo()
    draws = [e for e in log["by_user"] if e[0].phase == "train"]
    assert len(draws) >= 3
    M = neg.get("dynamic", 1)
    for k, (smp, st, users, num, got) in enumerate(draws):
        assert smp.distribution == "popularity" and num == M
        ref = np.random.RandomState()
        ref.set_state(st)
        want = R.sample_by_key_ids(ref, R.alias_table(smp._cand_for_test), users, num, _used_sets(smp.used_ids, smp.user_num))
        np.testing.assert_array_equal(got, want, err_msg=f"batch {k}")

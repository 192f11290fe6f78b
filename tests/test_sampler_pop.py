"""CPU: the popularity sampler's entry points refuse bad arguments with FR_EINVAL before any device work, and the evaluation
mode `popN` parses the way `uniN` does (RecBole 1.0's configurator: int() of what follows the three letters)."""
import pytest

from fairrec import _C
from fairrec.data.dataloader import eval_neg_sample_args

FAKE = 0x1000      # never dereferenced: every call below stops at an argument check


def _tab(n=10, keys=FAKE, prob=FAKE, alias=FAKE):
    return _C.FrAliasTable(keys, prob, alias, n)


def _pop(table, state=FAKE, key_ids=FAKE, n_keys=4, num=2, used_indptr=FAKE, used_items=FAKE, n_users=5, out=FAKE,
         ws=FAKE, ws_bytes=1 << 20):
    return _C.lib().fr_sample_negatives_pop(state, table, key_ids, n_keys, num, used_indptr, used_items, n_users, out, None,
                                            ws, ws_bytes, FAKE, None)


def _calls(table, state=FAKE, call_keys=FAKE, call_offsets=FAKE, n_calls=3, max_call=8, used_indptr=FAKE, used_items=FAKE,
           n_users=5, out=FAKE, ws=FAKE, ws_bytes=1 << 20):
    return _C.lib().fr_sample_negatives_pop_calls(state, table, call_keys, call_offsets, n_calls, max_call, used_indptr,
                                                  used_items, n_users, out, ws, ws_bytes, FAKE, None)


BAD_TABLES = {"null table": None, "null keys": _tab(keys=None), "null prob": _tab(prob=None), "null alias": _tab(alias=None),
              "n = 0": _tab(n=0), "n < 0": _tab(n=-3), "n - 1 = 2^32 - 1": _tab(n=1 << 32), "n - 1 > 2^32": _tab(n=(1 << 32) + 5)}


@pytest.mark.parametrize("case", sorted(BAD_TABLES))
def test_bad_tables_are_refused(case):
    lib = _C.lib()
    assert _pop(BAD_TABLES[case]) == -1
    assert b"fr_sample_negatives_pop" in lib.fr_last_error()
    assert _calls(BAD_TABLES[case]) == -1
    assert b"fr_sample_negatives_pop_calls" in lib.fr_last_error()


@pytest.mark.parametrize("kw", [dict(state=None), dict(out=None), dict(n_keys=0), dict(num=0), dict(n_keys=-1),
                                dict(n_keys=1 << 20, num=1 << 11), dict(used_items=None), dict(key_ids=None),
                                dict(n_users=0), dict(ws=None), dict(ws_bytes=0)])
def test_bad_sizes_and_used_sets_are_refused(kw):
    assert _pop(_tab(), **kw) == -1
    assert b"fr_sample_negatives_pop" in _C.lib().fr_last_error()


def test_workspace_one_byte_short_is_refused():
    lib = _C.lib()
    need = lib.fr_sample_negatives_workspace_bytes(4 * 2)
    assert _pop(_tab(), ws_bytes=need - 1) == -1
    assert b"workspace" in lib.fr_last_error()
    need = lib.fr_sample_negatives_workspace_bytes(8)
    assert _calls(_tab(), ws_bytes=need - 1) == -1
    assert b"workspace" in lib.fr_last_error()


@pytest.mark.parametrize("kw", [dict(state=None), dict(out=None), dict(call_keys=None), dict(call_offsets=None),
                                dict(n_calls=0), dict(max_call=0), dict(max_call=(1 << 30) + 1), dict(used_indptr=None),
                                dict(used_items=None), dict(n_users=0), dict(ws=None)])
def test_bad_call_sequences_are_refused(kw):
    assert _calls(_tab(), **kw) == -1
    assert b"fr_sample_negatives_pop_calls" in _C.lib().fr_last_error()


@pytest.mark.parametrize("mode,want", [("uni100", ("uniform", 100)), ("uni1", ("uniform", 1)), ("pop20", ("popularity", 20)),
                                       ("pop1", ("popularity", 1)), ("pop100", ("popularity", 100))])
def test_negative_sampled_modes_parse(mode, want):
    assert eval_neg_sample_args(mode) == want


@pytest.mark.parametrize("tail", ["", "x", "2.5", "-"])
def test_malformed_pop_fails_like_malformed_uni(tail):
    with pytest.raises(ValueError) as uni:
        eval_neg_sample_args("uni" + tail)
    with pytest.raises(ValueError) as pop:
        eval_neg_sample_args("pop" + tail)
    assert type(uni.value) is type(pop.value)


@pytest.mark.parametrize("mode", ["full", "labeled", "zipf20", ""])
def test_other_modes_are_not_negative_sampled(mode):
    with pytest.raises(NotImplementedError):
        eval_neg_sample_args(mode)

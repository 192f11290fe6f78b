"""CPU: dynamic negative sampling (`neg_sampling: {uniform: 1, dynamic: M}`) -- the training loader takes the key, refuses to
draw without a model, keeps its batch geometry, and the trainer fetches no batch of such a loader ahead of the step."""
import pytest
import torch

from fairrec.config import Config
from fairrec.data.dataloader import TrainDataLoader
from fairrec.data.dataset import synthetic_dataset
from fairrec.trainer.trainer import Trainer


class _NoSampler:
    """Stands in for fairrec.sampler.Sampler where nothing may be drawn."""

    def sample_by_user_ids(self, *a):
        raise AssertionError('drew candidates before the model was known')


def _loader(model, neg_sampling, batch=64):
    cfg = Config(model=model, config_dict={'device': 'cpu', 'train_batch_size': batch, 'neg_sampling': neg_sampling})
    ds = synthetic_dataset(cfg, 50, 40, 500, seed=1)
    return TrainDataLoader(cfg, ds, sampler=_NoSampler(), shuffle=False)


@pytest.mark.parametrize('model', ['PFCN_PMF', 'FairGo_PMF'])      # pairwise, pointwise
@pytest.mark.parametrize('dist', ['uniform', 'popularity'])
@pytest.mark.parametrize('num', [1, 3])
def test_dynamic_loader_constructs_with_the_plain_geometry(model, dist, num):
    plain = _loader(model, {dist: num})
    dyn = _loader(model, {dist: num, 'dynamic': 4})
    assert dyn.dynamic and not plain.dynamic
    assert dyn.candidate_num == 4 and plain.candidate_num is None
    assert (dyn.step, dyn.times, len(dyn)) == (plain.step, plain.times, len(plain))


@pytest.mark.parametrize('bad', [0, -2, 1.5, True])
def test_dynamic_must_be_a_positive_integer(bad):
    with pytest.raises(ValueError, match='dynamic'):
        _loader('PFCN_PMF', {'uniform': 1, 'dynamic': bad})


def test_iterating_without_a_model_is_a_clear_error():
    dl = _loader('PFCN_PMF', {'uniform': 1, 'dynamic': 2})
    with pytest.raises(RuntimeError, match='get_model'):
        next(iter(dl))


class _Recorder:
    """A loader whose every fetch and every optimizer step lands in one log."""

    def __init__(self, log, n, dynamic):
        self.log, self.n, self.dynamic, self.model = log, n, dynamic, None

    def get_model(self, model):
        self.model = model

    def __iter__(self):
        self.k = 0
        return self

    def __next__(self):
        if self.k == self.n:
            raise StopIteration()
        self.log.append(('fetch', self.k))
        self.k += 1
        return _Batch(self.k - 1)


class _Batch:
    def __init__(self, k):
        self.k = k

    def to(self, dev):
        return self


def _fake_trainer(log, dynamic):
    tr = Trainer.__new__(Trainer)
    tr.device = 'cpu'
    tr.config = {'train_neg_sample_args': {'strategy': 'by', 'by': 1, 'dynamic': 4 if dynamic else 'none'},
                 'graph_train_step': None, 'train_steps_per_call': None}

    class _Opt:
        def zero_grad(self):
            pass

        def step(self):
            log.append(('step', None))

    class _Model:
        PREFETCH = 2

        def train(self):
            pass

        def hip_engine(self):
            return None

        def calculate_loss(self, b):
            log.append(('loss', b.k))
            return torch.zeros((), requires_grad=True)

        def hint_next_batch(self, *queue):
            pass

    tr.model, tr.optimizer = _Model(), _Opt()
    tr._accumulate = lambda total, part: total
    tr._epoch_loss = lambda total, n_tuple: 0.0
    return tr


def test_trainer_fetches_a_dynamic_loaders_batch_only_after_the_step():
    log = []
    tr = _fake_trainer(log, dynamic=True)
    dl = _Recorder(log, 3, dynamic=True)
    tr._give_model(dl)
    assert dl.model is tr.model
    tr._train_epoch(dl, 0)
    assert log == [('fetch', 0), ('loss', 0), ('step', None), ('fetch', 1), ('loss', 1), ('step', None),
                   ('fetch', 2), ('loss', 2), ('step', None)]


def test_trainer_still_looks_ahead_on_a_plain_loader():
    log = []
    tr = _fake_trainer(log, dynamic=False)
    dl = _Recorder(log, 3, dynamic=False)
    tr._give_model(dl)
    assert dl.model is None
    tr._train_epoch(dl, 0)
    assert log[:4] == [('fetch', 0), ('fetch', 1), ('fetch', 2), ('loss', 0)]

"""The built-in Trainer's Lightning options without a GPU: argument validation, and the stepping bookkeeping of
``accumulate_grad_batches`` on a stub module whose optimizer, scheduler and loss count their calls."""
import math

import pytest

from climsr_amd.core.trainer import Trainer


class Loss:
    """Stands in for the loss tensor: remembers what it was divided by and reports its backward to the log."""

    def __init__(self, log, idx, div=1):
        self.log, self.idx, self.div = log, idx, div

    def __truediv__(self, k):
        return Loss(self.log, self.idx, self.div * k)

    def backward(self):
        self.log.append(("backward", self.idx, self.div))


class Opt:
    def __init__(self, owner, name="opt"):
        self.owner, self.log, self.name = owner, owner.calls, name

    def zero_grad(self, set_to_none=True):
        self.log.append(("zero_grad", self.name, self.owner.cur))

    def step(self):
        self.log.append(("step", self.name, self.owner.cur))


class Sched:
    def __init__(self, owner):
        self.owner, self.log = owner, owner.calls

    def step(self):
        self.log.append(("sched", self.owner.cur))


class Net:
    def parameters(self):
        return []


class Stub:
    def __init__(self, nopt=1):
        self.calls = []
        self.generator, self.discriminator = Net(), (Net() if nopt == 2 else None)
        self.nopt = nopt
        self.batch_idx = None
        self.cur = None  # the batch in flight, set by driven()

    def configure_optimizers(self):
        opts = [Opt(self, f"opt{i}") for i in range(self.nopt)]
        return opts, [{"scheduler": Sched(self), "interval": "step"} for _ in opts]

    def training_step(self, batch, batch_idx, optimizer_idx=None):
        self.batch_idx = batch_idx
        return Loss(self.calls, batch_idx)


@pytest.mark.parametrize("kw, exc", [
    (dict(gradient_clip_val=-0.5), ValueError),
    (dict(gradient_clip_val=1.0, gradient_clip_algorithm="value"), NotImplementedError),
    (dict(gradient_clip_algorithm="median"), ValueError),
    (dict(track_grad_norm=3), ValueError),
    (dict(track_grad_norm="three"), ValueError),
    (dict(accumulate_grad_batches=0), ValueError),
    (dict(accumulate_grad_batches=-2), ValueError),
    (dict(accumulate_grad_batches=2.0), ValueError),
    (dict(accumulate_grad_batches={4: 2}), NotImplementedError),
    (dict(accumulate_grad_batches=[1, 2]), NotImplementedError),
])
def test_bad_options_are_refused(kw, exc):
    with pytest.raises(exc):
        Trainer(Stub(), num_training_steps=10, **kw)


def driven(t, m):
    """Have the stub know which batch the trainer is on (zero_grad comes before training_step tells it)."""
    orig = t.training_batch

    def training_batch(batch, idx, last=False):
        m.cur = idx
        return orig(batch, idx, last=last)

    t.training_batch = training_batch
    return t


def test_lightning_defaults_and_accepted_values():
    t = Trainer(Stub(), num_training_steps=10)
    assert (t.gradient_clip_val, t.gradient_clip_algorithm, t.track_grad_norm, t.terminate_on_nan) == (0.0, "norm", -1, False)
    assert t.accumulate_grad_batches == 1
    for v in (2, 2.0, "2", "inf", float("inf"), -1):
        Trainer(Stub(), num_training_steps=10, track_grad_norm=v)
    Trainer(Stub(), num_training_steps=10, gradient_clip_val=None)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("nopt", [1, 2])
def test_accumulation_bookkeeping_through_fit(k, nopt):
    n = 7
    m = Stub(nopt)
    t = Trainer(m, num_training_steps=n, accumulate_grad_batches=k)
    m.calls.clear()
    driven(t, m)
    outs = t.fit(iter([{} for _ in range(n)]))  # a plain iterator: no len() to lean on
    assert len(outs) == n
    steps = [c for c in m.calls if c[0] == "step"]
    assert len(steps) == nopt * math.ceil(n / k)
    assert len([c for c in m.calls if c[0] == "sched"]) == nopt * math.ceil(n / k)  # each scheduler: once per stepping batch
    # every backward is on loss / k (k == 1: the loss itself, untouched), in batch order, once per optimizer
    assert [c for c in m.calls if c[0] == "backward"] == [("backward", i, k) for i in range(n) for _ in range(nopt)]
    # zero_grad exactly at i % k == 0; optimizer and scheduler steps exactly at (i + 1) % k == 0 or the last batch
    assert [c[-1] for c in m.calls if c[0] == "zero_grad"] == [b for b in range(n) if b % k == 0 for _ in range(nopt)]
    assert [c[-1] for c in m.calls if c[0] == "step"] == [b for b in _stepping(n, k) for _ in range(nopt)]
    assert [c[-1] for c in m.calls if c[0] == "sched"] == [b for b in _stepping(n, k) for _ in range(nopt)]


def _stepping(n, k):
    return [b for b in range(n) if (b + 1) % k == 0 or b == n - 1]


def test_order_within_a_stepping_batch():
    m = Stub(1)
    t = Trainer(m, num_training_steps=4, accumulate_grad_batches=2)
    m.calls.clear()
    driven(t, m).fit([{}, {}])
    assert m.calls == [("zero_grad", "opt0", 0), ("backward", 0, 2), ("backward", 1, 2), ("step", "opt0", 1), ("sched", 1)]


def test_training_batch_by_hand_and_last_flag():
    m = Stub(1)
    t = Trainer(m, num_training_steps=10, accumulate_grad_batches=3)
    m.calls.clear()
    t.training_batch({}, 0)
    t.training_batch({}, 1)
    assert not [c for c in m.calls if c[0] in ("step", "sched")]
    t.training_batch({}, 2)
    assert [c[0] for c in m.calls].count("step") == 1
    t.training_batch({}, 3, last=True)  # an open window closed by hand
    assert [c[0] for c in m.calls].count("step") == 2 and [c[0] for c in m.calls].count("sched") == 2
    assert [c[0] for c in m.calls].count("zero_grad") == 2


def test_default_fit_does_not_look_ahead():
    """With the defaults the trainer consumes a batch only when it trains on it (as before the options existed)."""
    m = Stub(1)
    t = Trainer(m, num_training_steps=3)
    drawn = []

    def gen():
        for i in range(3):
            drawn.append((i, m.batch_idx))
            yield {}

    t.fit(gen())
    assert drawn == [(0, None), (1, 0), (2, 1)]

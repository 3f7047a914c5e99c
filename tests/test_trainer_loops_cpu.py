"""The built-in Trainer's epoch, validation, test, checkpoint, early-stopping and resume loops without a GPU: call order
and bookkeeping on a stub module that records its calls, and resume on a tiny real task (nn.Linear, torch AdamW,
OneCycleLR)."""
import os

import pytest
import torch

from climsr_amd.core.checkpoint import save_checkpoint
from climsr_amd.core.trainer import EarlyStopping, ListDataModule, ModelCheckpoint, Trainer


class Loss:
    def __init__(self, log):
        self.log = log

    def __truediv__(self, k):
        return self

    def backward(self):
        self.log.append("backward")


class Opt:
    def __init__(self, log):
        self.log = log

    def zero_grad(self, set_to_none=True):
        pass

    def step(self):
        self.log.append("step")


class Sched:
    def step(self):
        pass


class Net:
    def parameters(self):
        return []


class Stub:
    """Records ("train", epoch, idx) / ("val", epoch, idx) / ("val_end", epoch) / ("test", idx) and the mode switches."""

    def __init__(self, val_rmse=None):
        self.calls, self.modes, self.logged = [], [], {}
        self.generator, self.discriminator, self.training = Net(), None, True
        self.val_rmse = val_rmse  # per validation epoch, the val/rmse every batch reports
        self.nval = 0
        self.saved = []

    def configure_optimizers(self):
        return [Opt(self.calls)], [{"scheduler": Sched(), "interval": "step"}]

    def train(self, mode=True):
        self.training = mode
        self.modes.append("train" if mode else "eval")
        return self

    def eval(self):
        return self.train(False)

    def log(self, k, v):
        self.logged[k] = v

    def training_step(self, batch, idx):
        assert self.training and torch.is_grad_enabled()
        self.calls.append(("train", self.current_epoch, idx))
        return Loss(self.calls)

    def validation_step(self, batch, idx):
        assert not self.training and not torch.is_grad_enabled()
        self.calls.append(("val", self.current_epoch, idx))
        rmse = batch["rmse"] if self.val_rmse is None else torch.tensor(self.val_rmse[self.nval], dtype=torch.float64)
        out = {"val/rmse": rmse, "val/mae": batch["mae"], "note": "not a tensor", "map": torch.zeros(2, 2)}
        self.log("val/mae", out["val/mae"])
        return out

    def validation_epoch_end(self, outputs):
        assert not self.training
        self.calls.append(("val_end", self.current_epoch))
        self.nval += 1
        self.log("hp_metric", torch.stack([o["val/rmse"] for o in outputs]).mean())

    def test_step(self, batch, idx):
        assert not self.training and not torch.is_grad_enabled()
        self.calls.append(("test", idx))
        return {"test/mae": batch["mae"], "sr": torch.zeros(1, 1, 4, 4)}

    def save_checkpoint(self, path, epoch=0, global_step=0, optimizers=(), schedulers=()):
        self.saved.append((os.path.basename(path), epoch, global_step, len(optimizers), len(schedulers)))
        open(path, "w").close()


def vb(n, mae, rmse):
    return {"lr": torch.zeros(n, 1), "mae": torch.tensor(mae, dtype=torch.float64), "rmse": torch.tensor(rmse, dtype=torch.float64)}


A, B = 0.3, 0.9
VAL = [vb(3, A, 1.0), vb(1, B, 2.0)]
TRAIN = [{}, {}, {}]


def marks(m, *kinds):
    return [c for c in m.calls if isinstance(c, tuple) and c[0] in kinds]


def test_epoch_order_with_validation_every_second_epoch():
    m = Stub()
    t = Trainer(m, max_epochs=3, check_val_every_n_epoch=2, datamodule=ListDataModule(TRAIN, VAL))
    outs = t.fit()
    assert len(outs) == 9
    want = [("train", 0, i) for i in range(3)] + [("train", 1, i) for i in range(3)] + \
           [("val", 1, 0), ("val", 1, 1), ("val_end", 1)] + [("train", 2, i) for i in range(3)]
    assert marks(m, "train", "val", "val_end") == want
    assert (t.current_epoch, t.global_step, m.current_epoch, m.global_step) == (2, 9, 2, 9)


def test_eval_no_grad_then_back_to_train():
    m = Stub()
    t = Trainer(m, max_epochs=1)
    t.fit(datamodule=ListDataModule(TRAIN, VAL))  # the steps themselves assert the mode and the grad switch
    assert m.modes == ["eval", "train"] and m.training and torch.is_grad_enabled()
    m.train(False)
    t.validate(VAL)
    assert not m.training  # a module that was in eval() stays there
    m.train(True)
    t.test([vb(2, 0.5, 0.0)])
    assert m.training


def test_epoch_value_is_the_sample_weighted_mean_and_hp_metric_the_plain_one():
    m = Stub()
    t = Trainer(m, max_epochs=1)
    res = t.validate(VAL)
    got = t.callback_metrics["val/mae"]
    assert got.dtype == torch.float64 and got.item() == pytest.approx((3 * A + B) / 4, abs=1e-15)
    assert abs(got.item() - (A + B) / 2) > 0.1
    assert t.callback_metrics["hp_metric"].item() == pytest.approx(1.5, abs=1e-15)  # unweighted mean of val/rmse 1, 2
    assert t.callback_metrics["val/rmse"].item() == pytest.approx(1.25, abs=1e-15)
    assert set(t.callback_metrics) == {"val/mae", "val/rmse", "hp_metric"}  # strings and maps are no epoch values
    assert m.logged["val/mae"] is got and m.logged["hp_metric"] is t.callback_metrics["hp_metric"]
    assert isinstance(res, list) and len(res) == 1 and res[0]["val/mae"] == got.item() and isinstance(res[0]["hp_metric"], float)


def test_limits_sanity_steps_and_unsupported_interval():
    m = Stub()
    t = Trainer(m, max_epochs=1, limit_val_batches=1)
    t.validate(VAL)
    assert marks(m, "val") == [("val", 0, 0)] and t.callback_metrics["val/mae"].item() == A
    m = Stub()
    Trainer(m, max_epochs=1, limit_val_batches=0.5).validate(VAL)
    assert len(marks(m, "val")) == 1
    with pytest.raises(TypeError):
        Trainer(Stub(), max_epochs=1, limit_val_batches=0.5).validate(iter(VAL))  # a fraction needs len()
    m = Stub()
    t = Trainer(m, max_epochs=1, limit_test_batches=2)
    res = t.test([vb(1, 1.0, 0), vb(1, 2.0, 0), vb(1, 30.0, 0)])
    assert marks(m, "test") == [("test", 0), ("test", 1)] and res == [{"test/mae": 1.5}]
    m = Stub()
    t = Trainer(m, max_epochs=1, num_sanity_val_steps=1, datamodule=ListDataModule(TRAIN, VAL))
    m.logged["kept"] = 1
    t.fit()
    assert marks(m, "val", "val_end", "train")[:2] == [("val", 0, 0), ("train", 0, 0)]  # one sanity batch, no epoch end
    assert marks(m, "val_end") == [("val_end", 0)] and m.logged["kept"] == 1
    with pytest.raises(NotImplementedError):
        Trainer(Stub(), max_epochs=1, val_check_interval=0.5)


def test_max_steps_stops_inside_an_epoch_and_global_step_counts_optimizer_steps():
    m = Stub()
    t = Trainer(m, max_epochs=5, max_steps=4, datamodule=ListDataModule(TRAIN, VAL))
    t.fit()
    assert marks(m, "train") == [("train", 0, 0), ("train", 0, 1), ("train", 0, 2), ("train", 1, 0)]
    assert t.global_step == 4 and m.calls.count("step") == 4
    assert marks(m, "val_end") == [("val_end", 0)]  # the cut epoch is not validated
    m = Stub()
    t = Trainer(m, max_epochs=2, accumulate_grad_batches=2, datamodule=ListDataModule(TRAIN))
    t.fit()
    # per epoch of 3 batches: one full window and the open one the epoch's last batch closes
    assert m.calls.count("backward") == 6 and m.calls.count("step") == 4 and t.global_step == 4


def test_checkpoint_file_name_follows_lightning():
    cb = ModelCheckpoint(filename="{epoch:03d}_{step:05d}_{hp_metric:0.5f}")
    assert cb.format_checkpoint_name({"epoch": 29, "step": 165419, "hp_metric": 0.167083}) == \
        "epoch=029_step=165419_hp_metric=0.16708.ckpt"
    assert ModelCheckpoint().format_checkpoint_name({"epoch": 3, "step": 10}) == "epoch=3-step=10.ckpt"
    cb = ModelCheckpoint(filename="{epoch}_{val/mae:.2f}", auto_insert_metric_name=False)
    assert cb.format_checkpoint_name({"epoch": 1, "val/mae": 0.256}) == "1_0.26.ckpt"


@pytest.mark.parametrize("mode, kept", [("min", ["epoch=1", "epoch=3"]), ("max", ["epoch=0", "epoch=2"])])
def test_top_k_pruning_and_save_last(tmp_path, mode, kept):
    m = Stub(val_rmse=[3.0, 1.0, 4.0, 2.0])
    cb = ModelCheckpoint(monitor="hp_metric", mode=mode, save_top_k=2, save_last=True, dirpath=str(tmp_path), filename="{epoch}")
    t = Trainer(m, max_epochs=4, callbacks=[cb], datamodule=ListDataModule(TRAIN, VAL))
    t.fit()
    assert sorted(os.listdir(tmp_path)) == sorted(k + ".ckpt" for k in kept) + ["last.ckpt"]
    best = {"min": ("epoch=1.ckpt", 1.0), "max": ("epoch=2.ckpt", 4.0)}[mode]
    assert (os.path.basename(cb.best_model_path), cb.best_model_score) == best
    assert sorted(cb.best_k_models.values()) == {"min": [1.0, 2.0], "max": [3.0, 4.0]}[mode]
    # saved through the task with the live optimizer and scheduler, at the epoch's end
    assert ("epoch=1.ckpt", 1, 6, 1, 1) in m.saved and m.saved[-1] == ("last.ckpt", 3, 12, 1, 1)


def test_early_stopping_patience_and_min_delta():
    # best 3.0; 2.95 is no improvement by more than 0.1 (wait 1), 2.8 is (wait 0), then two misses stop after epoch 4
    m = Stub(val_rmse=[3.0, 2.95, 2.8, 2.75, 2.9, 1.0, 1.0])
    es = EarlyStopping(monitor="hp_metric", mode="min", patience=2, min_delta=0.1)
    t = Trainer(m, max_epochs=7, callbacks=[es], datamodule=ListDataModule(TRAIN, VAL))
    t.fit()
    assert marks(m, "val_end") == [("val_end", e) for e in range(5)]
    assert (es.stopped_epoch, es.best_score, es.wait_count, t.should_stop) == (4, 2.8, 2, True)
    m = Stub(val_rmse=[1.0, 1.05, 2.0, 2.0])
    es = EarlyStopping(monitor="hp_metric", mode="max", patience=1)
    Trainer(m, max_epochs=4, callbacks=[es], datamodule=ListDataModule(TRAIN, VAL)).fit()
    assert es.stopped_epoch == 3 and es.best_score == 2.0
    m = Stub(val_rmse=[float("nan")])
    es = EarlyStopping(patience=5)
    Trainer(m, max_epochs=3, callbacks=[es], datamodule=ListDataModule(TRAIN, VAL)).fit()
    assert es.stopped_epoch == 0  # a NaN monitor stops at once


def test_fit_batches_is_still_one_pass():
    m = Stub()
    t = Trainer(m, max_epochs=3, datamodule=ListDataModule(TRAIN, VAL))
    outs = t.fit(TRAIN)
    assert len(outs) == 3 and marks(m, "train", "val") == [("train", 0, i) for i in range(3)] and m.modes == []


# -- resume on a tiny real task ---------------------------------------------------------------------------------------
class LinearTask(torch.nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(5)
        self.generator, self.discriminator = torch.nn.Linear(4, 2), None
        self.logged = {}

    def log(self, k, v):
        self.logged[k] = v

    def configure_optimizers(self):
        self.opt = torch.optim.AdamW(self.generator.parameters(), lr=1e-2, weight_decay=1e-2)
        self.sch = torch.optim.lr_scheduler.OneCycleLR(self.opt, max_lr=1e-2, total_steps=6, pct_start=0.3)
        return [self.opt], [{"scheduler": self.sch, "interval": "step"}]

    def training_step(self, batch, idx):
        return ((self.generator(batch["lr"]) - batch["hr"]) ** 2).mean()

    def validation_step(self, batch, idx):
        return {"val/rmse": ((self.generator(batch["lr"]) - batch["hr"]) ** 2).mean().sqrt().double()}

    def validation_epoch_end(self, outputs):
        self.log("hp_metric", torch.stack([o["val/rmse"] for o in outputs]).mean())

    def save_checkpoint(self, path, epoch=0, global_step=0, optimizers=(), schedulers=()):
        return save_checkpoint(self, path, epoch, global_step, optimizers, schedulers, {})


def linear_data():
    g = torch.Generator().manual_seed(6)
    mk = lambda: {"lr": torch.randn(5, 4, generator=g), "hr": torch.randn(5, 2, generator=g)}  # noqa: E731
    return ListDataModule([mk() for _ in range(3)], [mk()])


def test_resume_is_bit_identical_to_the_uninterrupted_run(tmp_path):
    dm = linear_data()
    straight = LinearTask()
    Trainer(straight, max_epochs=2, datamodule=dm).fit()

    first = LinearTask()
    cb = ModelCheckpoint(dirpath=str(tmp_path), save_top_k=0, save_last=True)
    Trainer(first, max_epochs=1, callbacks=[cb], datamodule=dm).fit()
    ckpt = torch.load(cb.last_model_path, weights_only=True)
    assert (ckpt["epoch"], ckpt["global_step"]) == (0, 3)

    resumed = LinearTask()
    with torch.no_grad():
        resumed.generator.weight.add_(1.0)  # whatever it held is replaced by the file
    t = Trainer(resumed, max_epochs=2, resume_from_checkpoint=cb.last_model_path, datamodule=dm)
    assert (t.current_epoch, t.global_step) == (1, 3) and resumed.sch.last_epoch == 3
    outs = t.fit()
    assert len(outs) == 3 and (t.current_epoch, t.global_step) == (1, 6)
    for a, b in zip(straight.generator.parameters(), resumed.generator.parameters()):
        assert torch.equal(a, b)
    sa, sb = straight.opt.state_dict()["state"], resumed.opt.state_dict()["state"]
    assert sa.keys() == sb.keys()
    for k in sa:
        for name in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(torch.as_tensor(sa[k][name]), torch.as_tensor(sb[k][name])), (k, name)
    assert straight.sch.last_epoch == resumed.sch.last_epoch == 6
    assert straight.opt.param_groups[0]["lr"] == resumed.opt.param_groups[0]["lr"]
    assert torch.equal(straight.logged["hp_metric"], resumed.logged["hp_metric"])

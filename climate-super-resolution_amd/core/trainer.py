"""Built-in trainer loop with Lightning-1.x automatic-optimisation semantics (used when
pytorch_lightning is absent, and by bench.py).  Per batch and per optimizer i:
toggle (only optimizer i's params require grad), zero_grad, training_step(batch, idx[, i]),
backward, optimizer i step; then every scheduler steps (interval "step", task.py:58-59).

It carries the ``pytorch_lightning.Trainer`` attributes the task's ``num_training_steps`` reads
(task.py:61-83: limit_train_batches, datamodule, max_epochs, max_steps, accumulate_grad_batches,
num_gpus / num_processes) and calls the zero-argument ``configure_optimizers()`` hook.  The one extension is
``num_training_steps=N``: a run of exactly N batches (limit_train_batches=N, max_epochs=1).

Lightning trainer options of conf/trainer/default.yaml (climsr/core/config.py:105-143), all off by default -- the
default trainer launches exactly what is described above:

- ``accumulate_grad_batches=k``: batch i zeroes the gradients only when i % k == 0, backpropagates loss / k (the native
  backward accumulates while ``.grad`` still views the flat buffer), and the optimizers and the "step" schedulers step
  only when (i + 1) % k == 0 or i is the last batch ``fit`` will see (it looks one batch ahead).
- ``gradient_clip_val`` (algorithm "norm"): the L2 norm over the stepped network comes from one segmented reduction of
  its flat gradient buffer (core/optim.GradNorm); the clip coefficient stays on the device and the fused AdamW applies
  it while reading the gradient (``AdamW.step(grad_scale=...)``), so ``.grad`` keeps the unclipped gradient.  Any other
  optimizer gets the flat gradient scaled in place first (``clip_grad_norm_`` semantics).  Logs ``grad_clip_coef/{net}``.
- ``track_grad_norm`` (2 or "inf"): logs ``grad_{p}_norm/{net}.{param}`` and ``grad_{p}_norm_total`` of the network
  about to step, before clipping, as device tensors (no rounding to 4 decimals, no stale norms of the other network).
- ``terminate_on_nan``: reads the loss and the norm's finite flag before each optimizer step (the only host sync these
  options introduce) and raises ``ValueError`` instead of stepping.

Epochs, validation, test and resume (all off by default; ``fit(batches)`` stays the single pass described above, with
``max_epochs`` ignored):

- ``fit(datamodule=dm)`` (or ``Trainer(datamodule=dm)`` and ``fit()``): ``dm.train_dataloader()`` / ``dm.val_dataloader()``
  are called once and iterated once per epoch, for ``max_epochs`` epochs or until ``max_steps`` optimizer steps (the
  epoch is cut there and not validated).  ``limit_train_batches`` (int count / float fraction) bounds each epoch.
  ``current_epoch`` and ``global_step`` (optimizer steps of optimizer 0) live on the trainer and the module.
- ``validate``: after epoch e when (e + 1) % ``check_val_every_n_epoch`` == 0, or on its own.  eval() + no_grad, then
  back to train(); ``validation_step`` per batch, ``validation_epoch_end(outputs)`` at the end.  Every scalar tensor of
  the step's dict becomes an epoch value: the mean over batches weighted by ``batch["lr"].shape[0]`` (Lightning 1.x's
  ``on_epoch=True`` reduction), accumulated on the device in fp64 with no host read.  They land, with ``hp_metric``, in
  ``trainer.callback_metrics`` and ``module.logged``.  ``limit_val_batches``; ``num_sanity_val_steps`` (default 0 here).
- ``test(per_image=, baselines=)``: the same loop over ``test_step``; returns Lightning's ``[{name: float}]``.  With
  ``per_image`` the ``SRMetrics.per_image`` rows of every batch's ``sr`` are concatenated in loader order as
  ``trainer.test_table`` ([N, 17] float64 on the device); ``baselines`` adds ``test_table_nearest`` / ``test_table_cubic``.
- ``callbacks=[ModelCheckpoint(...), EarlyStopping(...)]`` run after each validation inside ``fit`` (one host read of the
  monitored value each).  ``resume_from_checkpoint=path`` restores weights, optimizer and scheduler states, ``epoch`` and
  ``global_step`` and continues with the next epoch, bit-identical to the uninterrupted run.

``graph_steps=True`` (off by default; ``graph_warmup=2``): every optimizer / scheduler pair becomes its device-stepped
form (core/optim.DeviceStepped) at construction, after a resume.  The first ``graph_warmup`` batches run that step
eagerly on a side stream; then the batch's whole step -- every optimizer's zero_grad, training_step, backward and device
step, with the toggling -- is captured once, on one stream, into a private graph pool, and every later batch with the same
tensor shapes and dtypes is copied into static inputs and replayed.  Before each replay the host checks the capture's
key: the batch signature, and per network the flat buffer's pointer, the engine object and the re-pack rule's version
key.  Another signature (an epoch's short last batch) runs one eager device-stepped step and leaves the capture alone; a
moved pointer, engine or version (``load_state_dict``, ``p.mul_()``, ``.to()``) drops it, one eager step re-packs, and
the step is captured again.  ``training_batch`` returns copies of the losses; ``module.logged`` holds the capture's own
output tensors.  The step counts and ``last_epoch`` live on the device and are flushed to the optimizers and schedulers
before ``save_checkpoint``, the callbacks after a validation and the end of ``fit``.  ``accumulate_grad_batches > 1``,
``track_grad_norm``, ``terminate_on_nan``, a DDP-wrapped network, a grad-ready hook and a pair the device cannot step
are refused at construction.  ``graph_stats`` counts captures, replayed and eager steps.
"""
from __future__ import annotations

import itertools
import math
import os
import re
from typing import Any, Dict, Iterable, List, Optional

NET_NAMES = ("generator", "discriminator")
_END = object()


class ListDataModule:
    """A datamodule over lists (or any re-iterable) of ready batches."""

    def __init__(self, train, val=None, test=None):
        self.train_dataloader, self.val_dataloader, self.test_dataloader = (lambda: train), (lambda: val), (lambda: test)


def _limited(batches, limit, what: str):
    """``batches`` cut to Lightning's ``limit_*_batches``: an int is a batch count, a float a fraction of ``len()``."""
    if isinstance(limit, bool) or not isinstance(limit, (int, float)) or limit < 0:
        raise ValueError(f"{what} must be an int count or a float fraction >= 0, got {limit!r}")
    if isinstance(limit, float):
        if limit == 1.0:
            return batches
        if limit > 1.0:
            raise ValueError(f"{what}={limit!r}: a float is a fraction in [0, 1]; pass an int for a batch count")
        limit = int(len(batches) * limit)
    return itertools.islice(batches, limit)


def _batch_size(batch) -> int:
    try:
        return int(batch["lr"].shape[0])
    except (KeyError, TypeError, AttributeError, IndexError):
        return 1


def _better(mode: str):
    if mode not in ("min", "max"):
        raise ValueError(f'mode must be "min" or "max", got {mode!r}')
    return (lambda a, b: a < b) if mode == "min" else (lambda a, b: a > b)


def _monitored(trainer, monitor: str, who: str) -> float:
    if monitor not in trainer.callback_metrics:
        raise RuntimeError(f"{who}(monitor={monitor!r}): no such metric after validation; have "
                           f"{sorted(trainer.callback_metrics)}")
    return float(trainer.callback_metrics[monitor])  # the callback's one host read per validation


class ModelCheckpoint:
    """Lightning's ``ModelCheckpoint`` for the built-in trainer (conf/callbacks/model_checkpoint.yaml monitors
    ``hp_metric``): after each validation inside ``fit`` it saves through the task's ``save_checkpoint`` with the live
    optimizers and schedulers, keeps the best ``save_top_k`` files (-1: all, 0: none) and deletes the rest;
    ``save_last`` also writes ``last.ckpt``."""

    def __init__(self, monitor: str = "hp_metric", mode: str = "min", save_top_k: int = 1, save_last: Optional[bool] = None,
                 dirpath: str = "checkpoints", filename: Optional[str] = None, auto_insert_metric_name: bool = True):
        self._is_better = _better(mode)
        self.monitor, self.mode, self.save_top_k, self.save_last = monitor, mode, int(save_top_k), bool(save_last)
        self.dirpath, self.filename, self.auto_insert_metric_name = dirpath, filename, auto_insert_metric_name
        self.best_k_models: Dict[str, float] = {}
        self.best_model_path, self.best_model_score, self.last_model_path = "", None, ""

    def format_checkpoint_name(self, metrics: Dict[str, Any]) -> str:
        """Lightning's file-name rule: ``{name...}`` becomes ``name={name...}`` (auto_insert_metric_name), a metric
        that is missing counts as 0, and the default is ``{epoch}-{step}``."""
        name = self.filename or "{epoch}-{step}"
        metrics = dict(metrics)
        for group in dict.fromkeys(re.findall(r"(\{.*?)[:\}]", name)):
            key = group[1:]
            name = name.replace(group, (key + "=" if self.auto_insert_metric_name else "") + "{0[" + key + "]")
            metrics.setdefault(key, 0)
        return name.format(metrics) + ".ckpt"

    def on_validation_end(self, trainer) -> None:
        score = _monitored(trainer, self.monitor, "ModelCheckpoint")
        if math.isnan(score):  # Lightning: NaN is the worst score
            score = math.inf if self.mode == "min" else -math.inf
        os.makedirs(self.dirpath, exist_ok=True)
        k = self.save_top_k
        worst = (max if self.mode == "min" else min)(self.best_k_models, key=self.best_k_models.get, default=None)
        if k != 0 and (k < 0 or len(self.best_k_models) < k or self._is_better(score, self.best_k_models[worst])):
            fields = {"epoch": trainer.current_epoch, "step": trainer.global_step, self.monitor: score}
            for key in re.findall(r"\{(.*?)[:\}]", self.filename or ""):  # other metrics named by the file name
                if key not in fields and key in trainer.callback_metrics:
                    fields[key] = float(trainer.callback_metrics[key])
            path = os.path.join(self.dirpath, self.format_checkpoint_name(fields))
            trainer.save_checkpoint(path)
            self.best_k_models[path] = score
            if k > 0 and len(self.best_k_models) > k:
                del self.best_k_models[worst]
                if worst != path and os.path.exists(worst):
                    os.remove(worst)
            best = min if self.mode == "min" else max
            self.best_model_path = best(self.best_k_models, key=self.best_k_models.get)
            self.best_model_score = self.best_k_models[self.best_model_path]
        if self.save_last:
            self.last_model_path = os.path.join(self.dirpath, "last.ckpt")
            trainer.save_checkpoint(self.last_model_path)


class EarlyStopping:
    """Lightning's ``EarlyStopping`` (conf/callbacks/early_stopping.yaml): the monitored value improves when it beats the
    best so far by more than ``min_delta``; after ``patience`` validations in a row without that, or on a NaN / infinite
    value (``check_finite``), ``fit`` stops after the current epoch."""

    def __init__(self, monitor: str = "hp_metric", mode: str = "min", patience: int = 3, min_delta: float = 0.0,
                 check_finite: bool = True):
        self._is_better = _better(mode)
        self.monitor, self.mode, self.patience, self.check_finite = monitor, mode, int(patience), check_finite
        self.min_delta = abs(float(min_delta)) * (1.0 if mode == "max" else -1.0)
        self.best_score = math.inf if mode == "min" else -math.inf
        self.wait_count, self.stopped_epoch = 0, None

    def on_validation_end(self, trainer) -> None:
        cur = _monitored(trainer, self.monitor, "EarlyStopping")
        stop = False
        if self.check_finite and not math.isfinite(cur):
            stop = True
        elif self._is_better(cur - self.min_delta, self.best_score):
            self.best_score, self.wait_count = cur, 0
        else:
            self.wait_count += 1
            stop = self.wait_count >= self.patience
        if stop:
            trainer.should_stop, self.stopped_epoch = True, trainer.current_epoch


def _reachable_tensors(roots) -> List[Any]:
    """Every tensor reachable from ``roots`` through containers, nn.Modules and this package's own objects."""
    import torch

    seen, found, todo = set(), [], list(roots)
    while todo:
        x = todo.pop()
        if id(x) in seen:
            continue
        seen.add(id(x))
        if isinstance(x, torch.Tensor):
            found.append(x)
        elif isinstance(x, dict):
            todo.extend(x.values())
        elif isinstance(x, (list, tuple, set)):
            todo.extend(x)
        elif isinstance(x, torch.nn.Module) or type(x).__module__.split(".")[0] == __name__.split(".")[0]:
            todo.extend(getattr(x, "__dict__", {}).values())
    return found


def _norm_label(track_grad_norm) -> Optional[str]:
    """Lightning's ``track_grad_norm`` value as the ``{p}`` of its log keys ("2.0" / "inf"), None for off (-1)."""
    t = track_grad_norm
    if isinstance(t, str):
        if t.lower() == "inf":
            return "inf"
        try:
            t = float(t)
        except ValueError:
            raise ValueError(f"track_grad_norm={track_grad_norm!r}: expected -1, 2 or 'inf'") from None
    if isinstance(t, bool) or not isinstance(t, (int, float)):
        raise ValueError(f"track_grad_norm={track_grad_norm!r}: expected -1, 2 or 'inf'")
    if t == -1:
        return None
    if t == 2:
        return "2.0"
    if t == float("inf"):
        return "inf"
    raise ValueError(f"track_grad_norm={track_grad_norm!r}: only the 2-norm and the inf-norm are implemented")


class Trainer:
    def __init__(self, module, num_training_steps: Optional[int] = None, max_epochs: int = 1, max_steps: Optional[int] = None,
                 limit_train_batches=1.0, accumulate_grad_batches: int = 1, datamodule=None, num_gpus: int = 0,
                 num_processes: int = 1, gradient_clip_val: float = 0.0, gradient_clip_algorithm: str = "norm",
                 track_grad_norm=-1, terminate_on_nan: bool = False, check_val_every_n_epoch: int = 1, limit_val_batches=1.0,
                 limit_test_batches=1.0, num_sanity_val_steps: int = 0, val_check_interval=1.0, callbacks=None,
                 resume_from_checkpoint: Optional[str] = None, graph_steps: bool = False, graph_warmup: int = 2):
        if isinstance(accumulate_grad_batches, (dict, list, tuple)):
            raise NotImplementedError("accumulate_grad_batches: Lightning's per-epoch schedules (dict / list) are not "
                                      "implemented; pass one int >= 1")
        if isinstance(accumulate_grad_batches, bool) or not isinstance(accumulate_grad_batches, int) or accumulate_grad_batches < 1:
            raise ValueError(f"accumulate_grad_batches must be an int >= 1, got {accumulate_grad_batches!r}")
        gradient_clip_val = 0.0 if gradient_clip_val is None else float(gradient_clip_val)
        if not gradient_clip_val >= 0.0:
            raise ValueError(f"gradient_clip_val must be >= 0, got {gradient_clip_val!r}")
        if gradient_clip_algorithm == "value":
            raise NotImplementedError('gradient_clip_algorithm="value" is not implemented; only "norm"')
        if gradient_clip_algorithm != "norm":
            raise ValueError(f'gradient_clip_algorithm must be "norm" or "value", got {gradient_clip_algorithm!r}')
        if val_check_interval != 1.0:
            raise NotImplementedError("val_check_interval: validation inside an epoch is not implemented; only 1.0 "
                                      "(validate after the epochs check_val_every_n_epoch selects)")
        if isinstance(check_val_every_n_epoch, bool) or not isinstance(check_val_every_n_epoch, int) or check_val_every_n_epoch < 1:
            raise ValueError(f"check_val_every_n_epoch must be an int >= 1, got {check_val_every_n_epoch!r}")
        self._norm_label = _norm_label(track_grad_norm)
        self.gradient_clip_val, self.gradient_clip_algorithm = gradient_clip_val, gradient_clip_algorithm
        self.track_grad_norm, self.terminate_on_nan = track_grad_norm, bool(terminate_on_nan)
        if num_training_steps is not None:
            limit_train_batches, max_epochs = int(num_training_steps), 1
        self.module = module
        self.max_epochs, self.max_steps = max_epochs, max_steps
        self.limit_train_batches, self.accumulate_grad_batches = limit_train_batches, accumulate_grad_batches
        self.datamodule, self.num_gpus, self.num_processes, self.tpu_cores = datamodule, num_gpus, num_processes, None
        module.trainer = self
        self.optimizers, self.schedulers = module.configure_optimizers()
        self.nets = [module.generator] + ([module.discriminator] if module.discriminator is not None else [])
        self._param_names: Dict[int, List[str]] = {}
        self.check_val_every_n_epoch, self.num_sanity_val_steps = check_val_every_n_epoch, int(num_sanity_val_steps)
        self.limit_val_batches, self.limit_test_batches = limit_val_batches, limit_test_batches
        self.callbacks = list(callbacks or [])
        self.callback_metrics: Dict[str, Any] = {}
        self.should_stop = False
        self.test_table = self.test_table_nearest = self.test_table_cubic = None
        self._set_progress(0, 0)
        if resume_from_checkpoint is not None:
            self._resume(resume_from_checkpoint)
        self.graph_steps, self.graph_warmup = bool(graph_steps), graph_warmup
        self.graph_stats = {"captures": 0, "replayed": 0, "eager": 0}
        self._device_opts: List[Any] = []
        self._capture = None  # (key, graph, static batch tensors, static outputs, entries of module.logged)
        self._graph_streams = None
        self._graph_seen, self._graph_sig = 0, None  # eager steps taken towards the capture, and the batch signature it is for
        if self.graph_steps:
            self._init_graph_steps()

    # -- graph mode: device-stepped optimizers, one captured step per batch signature
    def _init_graph_steps(self) -> None:
        """The refusals of ``graph_steps=True`` (nothing it cannot capture is silently run eagerly), then every
        optimizer / scheduler pair into its device-stepped form (core/optim.DeviceStepped)."""
        if isinstance(self.graph_warmup, bool) or not isinstance(self.graph_warmup, int) or self.graph_warmup < 1:
            raise ValueError(f"graph_warmup must be an int >= 1 (the eager steps before the capture make the engines' "
                             f"lazy allocations), got {self.graph_warmup!r}")
        if self.accumulate_grad_batches > 1:
            raise NotImplementedError(f"graph_steps=True does not support accumulate_grad_batches={self.accumulate_grad_batches} "
                                      "(an accumulation window inside a capture is not implemented); use 1")
        if self._norm_label is not None:
            raise NotImplementedError(f"graph_steps=True does not support track_grad_norm={self.track_grad_norm!r} "
                                      "(per-parameter norm logging is not captured); use -1")
        if self.terminate_on_nan:
            raise NotImplementedError("graph_steps=True does not support terminate_on_nan=True (it reads the loss on the "
                                      "host before every update)")
        for name, net in zip(NET_NAMES, self.nets):
            if any(c.__name__ == "DistributedDataParallel" for c in type(net).__mro__):
                raise NotImplementedError(f"graph_steps=True does not support a {name} wrapped in torch "
                                          "DistributedDataParallel (multi-rank capture is bench.py's)")
            if getattr(net, "_grad_ready_hook", None) is not None:
                raise NotImplementedError(f"graph_steps=True does not support a grad-ready hook on the {name} "
                                          "(set_grad_ready_hook: multi-rank capture is bench.py's)")
        if len(self.optimizers) != len(self.nets):
            raise NotImplementedError(f"graph_steps=True needs one optimizer per network, got {len(self.optimizers)} for "
                                      f"{len(self.nets)}")
        from .optim import DeviceStepped

        scheds = [s["scheduler"] if isinstance(s, dict) else s for s in self.schedulers]
        used = set()
        for i, opt in enumerate(self.optimizers):
            mine = [s for s in scheds if getattr(s, "optimizer", None) is opt]
            if len(mine) > 1:
                raise NotImplementedError(f"graph_steps=True: optimizer {i} has {len(mine)} schedulers; one at most")
            used.update(id(s) for s in mine)
            try:
                dev = DeviceStepped(opt, mine[0] if mine else None, max_grad_norm=self.gradient_clip_val or None)
            except NotImplementedError as e:
                raise NotImplementedError(f"graph_steps=True: optimizer {i}: {e}") from None
            if dev.module is not self.nets[i]:
                raise NotImplementedError(f"graph_steps=True: optimizer {i} does not own the {NET_NAMES[i]}'s parameters")
            self._device_opts.append(dev)
        if len(used) != len(scheds):
            raise NotImplementedError("graph_steps=True: a scheduler drives an optimizer that is not one of the trainer's")

    def flush_graph_state(self) -> None:
        """Graph mode keeps the step counts and ``last_epoch`` on the device; this writes them back to the optimizers
        and schedulers (one host read each).  Called before anything reads those: ``save_checkpoint``, the callbacks
        after a validation, the end of ``fit``."""
        for dev in self._device_opts:
            dev.flush()

    def _graph_key(self, batch):
        sig = tuple((k, tuple(v.shape), v.dtype) for k, v in batch.items() if hasattr(v, "data_ptr"))
        nets = tuple((net._flat.data_ptr(), id(net.engine())) + tuple(net.engine()._params_version()) for net in self.nets)
        return sig, nets

    def _graph_body(self, batch, batch_idx: int) -> List[Any]:
        """The Trainer's step with the device-stepped optimizers: the launches of a warm-up step, of an eager step of
        another batch signature, and of the capture."""
        outs = []
        nopt = len(self._device_opts)
        for i, dev in enumerate(self._device_opts):
            self._graph_opt = i
            if nopt > 1:
                self._toggle(i)
            dev.zero_grad(set_to_none=True)
            out = self.module.training_step(batch, batch_idx, i) if nopt > 1 else self.module.training_step(batch, batch_idx)
            loss = out["loss"] if isinstance(out, dict) else out
            loss.backward()
            coef = dev.step()
            if coef is not None:
                self.module.log(f"grad_clip_coef/{NET_NAMES[i]}", coef.clone())
            outs.append(out)
        if nopt > 1:
            for net in self.nets:
                for p in net.parameters():
                    p.requires_grad_(True)
        return outs

    @staticmethod
    def _copies(x, clone: bool = True):
        """``x`` with every tensor in it detached and, with ``clone``, copied (it stays valid after the next replay)."""
        if hasattr(x, "data_ptr"):
            return x.detach().clone() if clone else x.detach()
        if isinstance(x, dict):
            return {k: Trainer._copies(v, clone) for k, v in x.items()}
        if isinstance(x, (list, tuple)):
            return type(x)(Trainer._copies(v, clone) for v in x)
        return x

    def _graph_eager(self, batch, batch_idx: int, side: bool) -> List[Any]:
        import torch

        self.graph_stats["eager"] += 1
        if not side:
            return self._copies(self._graph_body(batch, batch_idx))
        if self._graph_streams is None:
            self._graph_streams = (torch.cuda.Stream(), torch.cuda.Stream())
        s = self._graph_streams[0]
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            outs = self._copies(self._graph_body(batch, batch_idx))
        torch.cuda.current_stream().wait_stream(s)
        return outs

    def _graph_capture(self, batch, batch_idx: int, key) -> None:
        """Capture this batch's step into ``self._capture`` (nothing runs: the replay that follows is the step)."""
        import torch

        static = {k: (torch.empty_like(v) if hasattr(v, "data_ptr") else v) for k, v in batch.items()}
        for k, v in batch.items():
            if hasattr(v, "data_ptr"):
                static[k].copy_(v)
        pool = torch.cuda.graph_pool_handle()  # private, and new for every capture: a dropped capture takes its pool along
        cap = self._graph_streams[1]
        logged = getattr(self.module, "logged", None)
        before = dict(logged) if logged is not None else {}
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        cap.wait_stream(torch.cuda.current_stream())
        self._graph_opt = 0
        with torch.cuda.stream(cap):
            # "relaxed": the backward's launches come from the autograd thread
            graph.capture_begin(pool=pool, capture_error_mode="relaxed")
            try:
                outs = self._graph_body(static, batch_idx)
            except BaseException as e:
                try:
                    graph.capture_end()  # never leave the stream capturing
                except Exception:
                    pass
                for net in self.nets:  # the aborted step may have left one network frozen
                    for p in net.parameters():
                        p.requires_grad_(True)
                raise RuntimeError(f"graph_steps=True: the step of optimizer {self._graph_opt} ({NET_NAMES[self._graph_opt]}) "
                                   f"could not be captured: {type(e).__name__}: {e}") from e
            graph.capture_end()
        torch.cuda.current_stream().wait_stream(cap)
        slogged = {k: v for k, v in logged.items() if before.get(k) is not v} if logged is not None else {}
        outs = self._copies(outs, clone=False)  # the capture's own output tensors, without the autograd graph
        # the capture reads and writes the engines' scratch tensors by address: hold every tensor reachable from the task
        # now, so a step of another batch shape that re-allocates a scratch buffer cannot free one the replay still uses
        self._capture = (key, graph, static, outs, slogged, _reachable_tensors([self.module, self._device_opts]))
        self.graph_stats["captures"] += 1

    def _graph_batch(self, batch: Dict[str, Any], batch_idx: int) -> List[Any]:
        key = self._graph_key(batch)
        cap = self._capture
        if cap is not None and cap[0][1] != key[1]:  # a pointer, an engine or a version key moved: the capture is stale
            cap = self._capture = None
            # one eager step (it re-packs and re-allocates), then a new capture
            self._graph_seen, self._graph_sig = self.graph_warmup - 1, None
        if cap is None:
            if self._graph_sig is None:
                self._graph_sig = key[0]  # the signature the capture will be made for
            if key[0] != self._graph_sig or self._graph_seen < self.graph_warmup:
                if key[0] == self._graph_sig:
                    self._graph_seen += 1
                return self._graph_eager(batch, batch_idx, side=True)
            self._graph_capture(batch, batch_idx, key)
            cap = self._capture
        elif cap[0][0] != key[0]:  # another signature (an epoch's short last batch): one eager step, the capture stays
            return self._graph_eager(batch, batch_idx, side=False)
        _key, graph, static, outs, slogged, _held = cap
        for k, v in batch.items():
            if hasattr(v, "data_ptr"):
                static[k].copy_(v)
        graph.replay()
        self.graph_stats["replayed"] += 1
        if slogged:
            self.module.logged.update(slogged)
        return self._copies(outs)

    def _toggle(self, i: int) -> None:
        for j, net in enumerate(self.nets):
            for p in net.parameters():
                p.requires_grad_(j == i)

    # -- the optimizer step with the norm options
    def _names(self, i: int) -> List[str]:
        if i not in self._param_names:
            net = self.nets[i]
            named = list(net.named_parameters())
            if len(named) != len(net._flat_index) or any(p is not q for (_k, p), (q, _o, _n) in zip(named, net._flat_index)):
                raise RuntimeError("the network's named_parameters() do not match its flat parameter index")
            self._param_names[i] = [k for k, _p in named]
        return self._param_names[i]

    def _log_norms(self, i: int, per, total) -> None:
        label, net = self._norm_label, NET_NAMES[i]
        for k, v in zip(self._names(i), per.clone().unbind(0)):
            self.module.log(f"grad_{label}_norm/{net}.{k}", v)
        self.module.log(f"grad_{label}_norm_total", total.clone())

    def _optimizer_step(self, i: int, opt, loss, batch_idx: int) -> None:
        clip, label = self.gradient_clip_val, self._norm_label
        if not (clip > 0 or label is not None or self.terminate_on_nan):
            opt.step()
            return
        from .optim import AdamW, GradNorm, scale_grad_

        net = self.nets[i]
        gn = GradNorm.of(net)
        coef = finite = None
        if label == "inf":
            per, total, _c, finite = gn("inf")
            self._log_norms(i, per, total)
        if label == "2.0" or clip > 0 or finite is None:  # one L2 launch serves tracking, clipping and the finite flag
            per, total, c, finite = gn(2, clip)
            if label == "2.0":
                self._log_norms(i, per, total)
            if clip > 0:
                coef = c
                self.module.log(f"grad_clip_coef/{NET_NAMES[i]}", c.clone())
        if self.terminate_on_nan:
            import torch

            if not (bool(torch.isfinite(loss.detach()).all()) and bool(finite)):  # the one host sync, before the update
                raise ValueError(f"terminate_on_nan: the loss or a gradient of the {NET_NAMES[i]} is NaN or infinite at "
                                 f"batch {batch_idx}; the optimizer did not step")
        if coef is None:
            opt.step()
        elif isinstance(opt, AdamW):
            opt.step(grad_scale=coef)  # applied while the update reads the gradient; .grad stays unclipped
        else:
            scale_grad_(net, coef)  # clip_grad_norm_ semantics: .grad is clipped, then any optimizer steps
            opt.step()

    def training_batch(self, batch: Dict[str, Any], batch_idx: int, last: bool = False) -> List[Any]:
        """One batch through every optimizer.  ``last``: no batch follows, so an open accumulation window steps now."""
        if self.graph_steps:
            outs = self._graph_batch(batch, batch_idx)
            self._set_progress(self.current_epoch, self.global_step + 1)
            return outs
        outs = []
        nopt = len(self.optimizers)
        k = self.accumulate_grad_batches
        first = batch_idx % k == 0
        stepping = (batch_idx + 1) % k == 0 or last
        for i, opt in enumerate(self.optimizers):
            if nopt > 1:
                self._toggle(i)
            if first:
                opt.zero_grad(set_to_none=True)
            out = self.module.training_step(batch, batch_idx, i) if nopt > 1 else self.module.training_step(batch, batch_idx)
            loss = out["loss"] if isinstance(out, dict) else out
            (loss if k == 1 else loss / k).backward()
            if stepping:
                self._optimizer_step(i, opt, loss, batch_idx)
            outs.append(out)
        if nopt > 1:
            for net in self.nets:
                for p in net.parameters():
                    p.requires_grad_(True)
        if stepping:
            for s in self.schedulers:
                s["scheduler"].step()
            self._set_progress(self.current_epoch, self.global_step + 1)  # optimizer 0's steps, as Lightning counts
        return outs

    def fit(self, batches: Optional[Iterable[Dict[str, Any]]] = None, datamodule=None):
        """``fit(batches)``: one pass over the iterable.  ``fit(datamodule=dm)`` / ``fit()``: the epoch loop."""
        if batches is None:
            return self._fit_epochs(datamodule if datamodule is not None else self.datamodule)
        if datamodule is not None:
            raise ValueError("fit: pass either batches (one pass) or datamodule= (the epoch loop), not both")
        outs = []
        if self.accumulate_grad_batches == 1:
            for idx, b in enumerate(batches):
                outs.append(self.training_batch(b, idx))
            self.flush_graph_state()
            return outs
        it = iter(batches)  # one batch ahead: the last batch closes an open accumulation window
        try:
            cur = next(it)
        except StopIteration:
            return outs
        idx = 0
        while True:
            try:
                nxt, last = next(it), False
            except StopIteration:
                nxt, last = None, True
            outs.append(self.training_batch(cur, idx, last=last))
            if last:
                return outs
            cur, idx = nxt, idx + 1

    # -- epochs, validation, test, checkpoints
    def _set_progress(self, epoch: int, global_step: Optional[int] = None) -> None:
        self.current_epoch = epoch
        if global_step is not None:
            self.global_step = global_step
        for k, v in (("current_epoch", self.current_epoch), ("global_step", self.global_step)):
            try:
                setattr(self.module, k, v)
            except AttributeError:  # a read-only property of the module
                pass

    def _steps_done(self) -> bool:
        return bool(self.max_steps) and self.max_steps > 0 and self.global_step >= self.max_steps

    def _train_epoch(self, batches, outs: List[Any]) -> bool:
        """One pass over the epoch's batches (batch_idx restarts at 0); True when ``max_steps`` cut it short."""
        it = iter(_limited(batches, self.limit_train_batches, "limit_train_batches"))
        ahead = self.accumulate_grad_batches > 1  # the epoch's last batch closes an open accumulation window
        cur, idx = next(it, _END), 0
        while cur is not _END:
            nxt = next(it, _END) if ahead else None
            outs.append(self.training_batch(cur, idx, last=nxt is _END))
            if self._steps_done():
                return True
            cur, idx = (nxt if ahead else next(it, _END)), idx + 1
        return False

    def _fit_epochs(self, dm):
        try:
            return self._fit_epochs_loop(dm)
        finally:
            self.flush_graph_state()

    def _fit_epochs_loop(self, dm):
        if dm is None:
            raise ValueError("fit() without batches needs a datamodule: fit(datamodule=dm) or Trainer(datamodule=dm)")
        train = dm.train_dataloader()
        val = dm.val_dataloader() if hasattr(dm, "val_dataloader") and self.limit_val_batches else None  # 0 switches it off
        if val is not None and self.num_sanity_val_steps:
            self._eval_loop("val", itertools.islice(val, self.num_sanity_val_steps) if self.num_sanity_val_steps > 0 else val,
                            discard=True)
        outs: List[Any] = []
        self.should_stop = False
        for epoch in range(self.current_epoch, self.max_epochs):
            if self._steps_done():
                break
            self._set_progress(epoch)
            if self._train_epoch(train, outs):
                break
            if val is not None and (epoch + 1) % self.check_val_every_n_epoch == 0:
                self._eval_loop("val", _limited(val, self.limit_val_batches, "limit_val_batches"))
                self.flush_graph_state()
                for cb in self.callbacks:
                    cb.on_validation_end(self)
            if self.should_stop:
                break
        return outs

    def _eval_loop(self, stage: str, batches, discard: bool = False, per_image: bool = False, baselines: bool = False):
        """``validation_step`` / ``test_step`` over ``batches`` in eval() under no_grad; the epoch values (device
        tensors, no host read) go to ``callback_metrics`` and ``module.logged`` unless ``discard`` (the sanity check)."""
        import torch

        m = self.module
        step = m.validation_step if stage == "val" else m.test_step
        was_training = getattr(m, "training", True)
        logged = getattr(m, "logged", None)
        keep = dict(logged) if discard and logged is not None else None
        sums: Dict[str, Any] = {}
        weight: Dict[str, int] = {}
        outputs, tables = [], {"sr": [], "nearest": [], "cubic": []}
        m.eval()
        try:
            with torch.no_grad():
                for idx, batch in enumerate(batches):
                    out = step(batch, idx)
                    bs = _batch_size(batch)
                    if per_image:
                        maps = [("sr", out["sr"])] + ([("nearest", batch["nearest"]), ("cubic", batch["cubic"])] if baselines else [])
                        for name, x in maps:
                            tables[name].append(m.metrics.per_image(x, batch["hr"], batch["original_data"], batch["mask"],
                                                                    batch.get("min"), batch.get("max")))
                    scalars = {k: v for k, v in out.items() if isinstance(v, torch.Tensor) and v.numel() == 1}
                    for k, v in scalars.items():
                        v = v.detach().reshape(()).to(torch.float64) * bs
                        sums[k] = v if k not in sums else sums[k] + v
                        weight[k] = weight.get(k, 0) + bs
                    if stage == "val":
                        outputs.append(scalars)
                if stage == "val" and outputs and not discard:
                    m.validation_epoch_end(outputs)
        finally:
            m.train(was_training)
        if discard:
            if keep is not None:
                logged.clear()
                logged.update(keep)
            return {}
        metrics = {k: s / weight[k] for k, s in sums.items()}
        if stage == "val" and logged is not None and "hp_metric" in logged:
            metrics["hp_metric"] = logged["hp_metric"]
        if logged is not None:
            logged.update(metrics)
        self.callback_metrics.update(metrics)
        if per_image:
            cat = lambda rows: torch.cat(rows, 0) if rows else None  # noqa: E731
            self.test_table, self.test_table_nearest, self.test_table_cubic = (cat(tables[k]) for k in ("sr", "nearest", "cubic"))
        return metrics

    def _loader(self, stage: str, batches, datamodule):
        if batches is not None:
            return batches
        dm = datamodule if datamodule is not None else self.datamodule
        if dm is None:
            raise ValueError(f"{stage}: pass batches, datamodule= or Trainer(datamodule=...)")
        loader = getattr(dm, "val_dataloader" if stage == "validate" else "test_dataloader")()
        if loader is None:
            raise ValueError(f"{stage}: the datamodule has no {stage} batches")
        return loader

    @staticmethod
    def _floats(metrics: Dict[str, Any]) -> List[Dict[str, float]]:
        import torch

        if not metrics:
            return [{}]
        vals = torch.stack([torch.as_tensor(v, dtype=torch.float64).reshape(()) for v in metrics.values()]).tolist()
        return [dict(zip(metrics, vals))]  # one host read

    def validate(self, batches=None, datamodule=None) -> List[Dict[str, float]]:
        """One validation epoch on its own (no callbacks); Lightning's return shape, one host read at the end."""
        loader = _limited(self._loader("validate", batches, datamodule), self.limit_val_batches, "limit_val_batches")
        return self._floats(self._eval_loop("val", loader))

    def test(self, batches=None, datamodule=None, per_image: bool = False, baselines: bool = False) -> List[Dict[str, float]]:
        if baselines and not per_image:
            raise ValueError("test(baselines=True) fills the nearest / cubic per-image tables: it needs per_image=True")
        loader = _limited(self._loader("test", batches, datamodule), self.limit_test_batches, "limit_test_batches")
        return self._floats(self._eval_loop("test", loader, per_image=per_image, baselines=baselines))

    def save_checkpoint(self, path: str):
        self.flush_graph_state()
        return self.module.save_checkpoint(path, epoch=self.current_epoch, global_step=self.global_step,
                                           optimizers=self.optimizers, schedulers=self.schedulers)

    def _resume(self, path: str) -> None:
        from .checkpoint import restore_training_state

        epoch, global_step = restore_training_state(self.module, path, self.optimizers, self.schedulers)
        self._set_progress(epoch + 1, global_step)  # the file was written after its epoch: go on with the next

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
"""
from __future__ import annotations

from typing import Any, Dict, Iterable, List, Optional

NET_NAMES = ("generator", "discriminator")


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
                 track_grad_norm=-1, terminate_on_nan: bool = False):
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
        return outs

    def fit(self, batches: Iterable[Dict[str, Any]]):
        outs = []
        if self.accumulate_grad_batches == 1:
            for idx, b in enumerate(batches):
                outs.append(self.training_batch(b, idx))
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

"""Lightning-format checkpoint interop.

The reference saves its task modules through Lightning's ``ModelCheckpoint`` and restores them with
``TaskSuperResolutionModule.load_from_checkpoint`` (cli/train.py:91-93, 112-121; inference.py:143):
a ``torch.save`` dict whose ``state_dict`` carries ``generator.`` / ``discriminator.`` prefixed keys, plus
``epoch``, ``global_step``, ``optimizer_states``, ``lr_schedulers`` and ``hyper_parameters``
(``on_save_checkpoint`` also pickles the Hydra instantiator, task.py:228-233).

Here:
* ``save_checkpoint`` writes the same layout (state_dict with the reference's key names, optimiser / scheduler
  states, hyper-parameters as plain values; no pickled objects), so the reference's
  ``load_from_checkpoint`` and this build read each other's weights;
* ``load_checkpoint`` reads with ``torch.load(weights_only=True)`` only: checkpoints that carry pickled
  Python objects (the reference's ``instantiator`` entry, OmegaConf hyper-parameters) are refused unless the
  caller vouches for the file with ``trusted=True`` (never use that on files you did not write);
* ``load_from_checkpoint`` rebuilds a task module from a checkpoint (hyper-parameters + overrides) and loads
  its weights; ``load_generator_weights`` moves just the ``generator.`` entries into a generator module
  (the GAN fine-tuning path of cli/train.py:115-119).
"""
from __future__ import annotations

from typing import Any, Dict, Iterable, Optional

import torch
from torch import nn

LIGHTNING_VERSION = "1.5.10"  # the Lightning 1.x layout the reference writes


def _plain(v: Any) -> Any:
    """Hyper-parameters as JSON-like values (dict / list / str / number / bool / None)."""
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, (str, int, float, bool)) or v is None:
        return v
    return repr(v)


def save_checkpoint(module: nn.Module, path: str, epoch: int = 0, global_step: int = 0,
                    optimizers: Iterable[torch.optim.Optimizer] = (), schedulers: Iterable[Any] = (),
                    hyper_parameters: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
    hp = hyper_parameters
    if hp is None:
        hp = dict(vars(module.hparams)) if hasattr(module, "hparams") and hasattr(module.hparams, "__dict__") else {}
    ckpt = {
        "epoch": int(epoch),
        "global_step": int(global_step),
        "pytorch-lightning_version": LIGHTNING_VERSION,
        "state_dict": {k: v.detach().cpu() for k, v in module.state_dict().items()},
        "optimizer_states": [o.state_dict() for o in optimizers],
        "lr_schedulers": [(s["scheduler"] if isinstance(s, dict) else s).state_dict() for s in schedulers],
        "hparams_name": "kwargs",
        "hyper_parameters": _plain(hp),
    }
    torch.save(ckpt, path)
    return ckpt


def load_checkpoint(path: str, map_location="cpu", trusted: bool = False) -> Dict[str, Any]:
    try:
        return torch.load(path, map_location=map_location, weights_only=True)
    except Exception as e:  # pickled objects inside
        if not trusted:
            raise RuntimeError(f"{path}: checkpoint holds pickled Python objects ({type(e).__name__}); it is loaded with "
                               "weights_only=True only. Re-save it with climsr_amd.core.checkpoint.save_checkpoint, or pass "
                               "trusted=True for a file you wrote yourself.") from e
        return torch.load(path, map_location=map_location, weights_only=False)


def restore_training_state(module: nn.Module, path: str, optimizers: Iterable[torch.optim.Optimizer] = (),
                           schedulers: Iterable[Any] = (), trusted: bool = False):
    """Lightning's ``resume_from_checkpoint`` (cli/train.py:91-93): weights, every optimizer's and scheduler's state.
    Returns the file's ``(epoch, global_step)``.  Optimizer states are read on the CPU and moved by each optimizer's
    ``load_state_dict`` (the fused AdamW checks its moment buffers against the flat parameter buffer there)."""
    ckpt = load_checkpoint(path, map_location="cpu", trusted=trusted)
    optimizers, schedulers = list(optimizers), [s["scheduler"] if isinstance(s, dict) else s for s in schedulers]
    ostates, sstates = ckpt.get("optimizer_states") or [], ckpt.get("lr_schedulers") or []
    if len(ostates) != len(optimizers) or len(sstates) != len(schedulers):
        raise ValueError(f"{path}: holds {len(ostates)} optimizer and {len(sstates)} scheduler states, the trainer has "
                         f"{len(optimizers)} and {len(schedulers)}")
    module.load_state_dict(ckpt["state_dict"], strict=True)
    for opt, st in zip(optimizers, ostates):
        opt.load_state_dict(st)
    for sch, st in zip(schedulers, sstates):
        sch.load_state_dict(st)
    return int(ckpt["epoch"]), int(ckpt["global_step"])


def strip_prefix(state_dict: Dict[str, torch.Tensor], prefix: str) -> Dict[str, torch.Tensor]:
    return {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}


def load_generator_weights(generator: nn.Module, path: str, strict: bool = True, trusted: bool = False) -> nn.Module:
    ckpt = load_checkpoint(path, trusted=trusted)
    sd = strip_prefix(ckpt["state_dict"], "generator.")
    if not sd:
        raise KeyError(f"{path}: no 'generator.' entries in state_dict")
    generator.load_state_dict(sd, strict=strict)
    return generator


def load_from_checkpoint(cls, path: str, strict: bool = False, trusted: bool = False, map_location="cpu", **overrides):
    """``cls.load_from_checkpoint`` (Lightning semantics): hyper-parameters from the file, overridden by kwargs."""
    ckpt = load_checkpoint(path, map_location=map_location, trusted=trusted)
    hp = dict(ckpt.get("hyper_parameters") or {})
    hp.update(overrides)
    module = cls(**hp)
    missing, unexpected = module.load_state_dict(ckpt["state_dict"], strict=strict)
    module._loaded_checkpoint_keys = (list(missing), list(unexpected))
    return module

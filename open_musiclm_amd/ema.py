"""Exponential moving average (EMA) of the weights, kept by the fused optimizer step itself (no reference counterpart).

The rule is stated once, in include/omlm.h (omlm_adamw_clip_step_ema): after an APPLIED optimizer step with clock t has produced p',

    n = t - update_after_step;   d(t) = 0 if n <= 0, min(decay, (1 + n) / (10 + n)) under warm-up, else decay;   e' = p' + d (e - p').

:func:`ema_decay_at` is d(t) on the host, :func:`check_ema_settings` the refusals, and :func:`EmaTwin` a read-only
TokenConditionedTransformer whose parameters are views of the optimizer's flat EMA buffer (``FusedAdam.ema_flat``): what
``generate`` / validation run on, and what an inference script loads (``twin.state_dict()``).
"""
from __future__ import annotations

import copy
import math
import weakref

import numpy as np


def check_ema_settings(decay, update_after_step=0, warmup=True):
    """(decay, update_after_step, warmup) as the C ABI takes them, or a ValueError that names the setting."""
    try:
        d = float(decay)
    except (TypeError, ValueError):
        raise ValueError(f"ema_decay must be a number in [0, 1), got {decay!r}") from None
    if math.isnan(d) or not (0.0 <= d < 1.0):
        raise ValueError(f"ema_decay must be a number in [0, 1), got {decay!r}")
    if float(np.float32(d)) >= 1.0:                  # the kernel receives a float: 1 - 1e-9 would arrive as 1
        raise ValueError(f"ema_decay must be a number in [0, 1) as fp32, got {decay!r}")
    if isinstance(update_after_step, bool) or int(update_after_step) != update_after_step or update_after_step < 0:
        raise ValueError(f"ema_update_after_step must be an integer >= 0, got {update_after_step!r}")
    return d, int(update_after_step), bool(warmup)


def ema_decay_at(t: int, decay: float, update_after_step: int = 0, warmup: bool = True) -> float:
    """d(t) of the rule for the clock t (counted from 1), as the kernel forms it: `decay` as the fp32 the C ABI receives, the
    quotient in double, one rounding to fp32."""
    d, after, warmup = check_ema_settings(decay, update_after_step, warmup)
    n = int(t) - after
    if n <= 0:
        return 0.0
    d = float(np.float32(d))
    if warmup:
        d = min(d, (1.0 + n) / (10.0 + n))
    return float(np.float32(d))


def bind_twin(twin, model, optim):
    """Point the twin's parameters at the optimizer's EMA buffer (again after a re-flatten): matched to the optimizer's offsets by the
    identity of the MODEL's parameters, which the twin's follow in order."""
    f = optim._flat
    E = f['E']
    slot = {id(p): k for k, p in enumerate(optim._all_params())}
    for mp, tp in zip(model.parameters(), twin.parameters()):
        k = slot.get(id(mp))
        if k is None:
            raise RuntimeError("EmaTwin: a parameter of the model is not held by this optimizer")
        o, n = f['offs'][k], f['sizes'][k]
        tp.data = E[o:o + n].view(mp.shape)
        tp.grad = None
        tp.__dict__.pop("_omlm_bf16", None)         # no 16-bit shadow of E is kept: engine.h16_operand casts afresh
    for b in twin.buffers():
        if b.device != E.device:
            b.data = b.data.to(E.device)
    twin.__dict__.pop("_omlm_prepared", None)


def EmaTwin(model, optim):
    """A TokenConditionedTransformer with `model`'s structure whose parameters are views of `optim.ema_flat`: read-only
    (requires_grad False, eval mode), no 16-bit shadow.  The optimizer bumps its parameters' version counters after every step, so
    engine.prepared_weights rebuilds its operand images, and re-binds the views when it re-flattens.  Its state_dict() has the model's
    keys and the EMA's values.  Keep it OUT of any nn.Module's registered submodules (SingleStageTrainer holds it in its __dict__):
    parameters(), .to() and state_dict() of the holder must not reach it."""
    if not optim.ema_enabled:
        raise ValueError("EmaTwin: the optimizer keeps no EMA (FusedAdam(..., ema_decay=...))")
    optim._ensure_flat()
    twin = copy.deepcopy(model)                      # TokenConditionedTransformer.__setstate__ registers the copy's parameters
    for k in ("_omlm_wbuf", "_omlm_ls_state"):       # training-step images / loss-scale block of the original: the twin never trains
        twin.__dict__.pop(k, None)
    twin.requires_grad_(False)
    twin.eval()
    bind_twin(twin, model, optim)
    optim._ema_twins.append((weakref.ref(twin), weakref.ref(model)))      # (on the optimizer, not the twin: the twin stays picklable)
    return twin

"""The weight-EMA rule of include/omlm.h (omlm_adamw_clip_step_ema) restated in numpy / torch, for the EMA tests.

After an APPLIED optimizer step with clock t (counted from 1) has produced the new parameter p':

    n    = t - update_after_step
    d(t) = 0                                  if n <= 0
         = min(decay, (1 + n) / (10 + n))     if warmup
         = decay                              otherwise
    e'   = p' + d * (e - p')

`decay` is the fp32 value the C ABI receives, d is formed in double and rounded to fp32 once; the blend here runs in fp64."""
import numpy as np
import torch

U32 = 2.0 ** -24                                     # unit roundoff of fp32


def f32(x):
    """x as the fp32 a `float` argument of the C ABI receives."""
    return float(np.float32(x))


def decay_at(t, decay, update_after_step=0, warmup=True):
    """d(t) as an fp32 value (python float)."""
    n = t - update_after_step
    if n <= 0:
        return 0.0
    d = f32(decay)
    if warmup:
        d = min(d, (1.0 + n) / (10.0 + n))
    return f32(d)


def blend(e, p_new, d):
    """e' in fp64 from e (any float dtype) and the fp32 p' the kernel produced."""
    e, p_new = e.double().cpu(), p_new.double().cpu()
    return p_new + d * (e - p_new)


def bound(steps, p, e):
    """|E - ref| <= steps * 3 * 2^-24 * max(|p|, |e|): per step one rounding each for the subtract, the multiply (or the fused
    multiply-add) and the add.  With u = 2^-24: the subtract leaves u |e - p'| <= 2 u max, scaled by d < 1; the result lies between e
    and p', so its own rounding is at most u max; what the earlier steps left is scaled by d < 1 again."""
    return steps * 3 * U32 * torch.maximum(p.double().cpu().abs(), e.double().cpu().abs())


def bits(t):
    """Integer view for bit-for-bit comparisons (-0.0 != +0.0, NaN == NaN)."""
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])

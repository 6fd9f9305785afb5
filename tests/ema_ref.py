"""Float64 restatement of the EMA forms of the fused optimizer step (ldm_adam_step_ema / ldm_model_adam_step_ema, include/ldm3d.h), built
on gan_ops_ref.adam_ref and taking the hyper-parameters as the fp32 values the kernels receive.  Host only: shared by tests/test_ema_cpu.py
(known answers) and the GPU parity tests."""
import math

import torch

import gan_ops_ref as R


def ema_decay_at(applied, decay, warmup):
    """The decay of update number ``applied`` (>= 1): a = applied - 1 updates came before it; warm-up (1 + a) / (10 + a) capped at decay."""
    a = int(applied) - 1
    assert a >= 0
    return min(float(decay), (1.0 + a) / (10.0 + a)) if warmup else float(decay)


def adam_ema_ref(p, g, m, v, ema, lr, b1, b2, eps, wd, step, skipped, decay, warmup, sq_norm=None, max_norm=0.0):
    """One call of the EMA optimizer step in float64 -> (p, m, v, ema, skipped).  ``step``: the caller's call count (1, 2, ...);
    ``skipped``: the device counter as the call finds it.  A non-finite ``sq_norm`` skips: nothing changes but the counter.  Otherwise
    Adam / AdamW at the bias corrections of step - skipped, then ema += (1 - d) (p_new - ema) with d of that same applied-update number."""
    if sq_norm is not None and not math.isfinite(float(sq_norm)):
        return p, m, v, ema, skipped + 1
    applied = max(int(step) - int(skipped), 1)
    p, m, v = R.adam_ref(p, g, m, v, lr, b1, b2, eps, wd, applied, sq_norm, max_norm)
    d = ema_decay_at(applied, decay, warmup)
    ema = ema.double() + (1.0 - d) * (p - ema.double())
    return p, m, v, ema, skipped

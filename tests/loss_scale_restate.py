"""The scaled optimiser step of include/epnet_ops.h (epnet_adam_onecycle_step_scaled) restated on the CPU in numpy, from the
header's text: the unscaling, the decision, the skip and the scale's rule, wrapped around optim_restate.run, which does the
applied steps. tests/test_loss_scale.py holds the scale's rule to stock torch._amp_update_scale_, tests/test_loss_scale_gpu.py
holds the kernels to this file bit for bit.
"""
import math

import numpy as np

import optim_restate as orr

F = np.float32


def inverse(scale):
    """inv = (float)(1.0 / (double)scale)"""
    return F(1.0 / float(F(scale)))


def unscale(grads, scale):
    """gu = g * inv, rounded to float32 (an overflow gives an infinity, which is the point)"""
    inv = inverse(scale)
    with np.errstate(over="ignore", invalid="ignore"):
        return [None if g is None else np.asarray(g, F) * inv for g in grads]


def sum_of_squares(grads):
    """float64 sum over (double)gu * (double)gu; finite exactly when every gu is (squares of floats cannot overflow a double)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return sum(float(np.sum(np.asarray(g, np.float64) ** 2)) for g in grads if g is not None)


def update_scale(scale, tracker, non_finite, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, min_scale=1.0):
    """(scale, tracker) after a step: products in double, rounded once to float32; growth_interval 0 never writes the scale"""
    scale, new = F(scale), F(scale)
    with np.errstate(over="ignore"):
        if non_finite:
            new = max(F(float(scale) * backoff_factor), F(min_scale))
            tracker = 0
        else:
            tracker += 1
            if tracker == growth_interval:
                grown = F(float(scale) * growth_factor)
                if np.isfinite(grown):
                    new = grown
                tracker = 0
    return (new if growth_interval > 0 else scale), tracker


def run(params, grads_per_step, total_steps, scale, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, min_scale=1.0,
        tracker=0, skipped=0, first_step=0, coefs=None, **settings):
    """len(grads_per_step) calls from applied-step index first_step; `settings` go to optim_restate.run (wd, b2, eps, clip and the
    schedule's), coefs[k] is the clip coefficient to use in call k if it is applied. Yields (params, exp_avg, exp_avg_sq, info)
    after every call; info: skip, scale_used, scale, tracker, skipped, applied (the counter), and for an applied step
    optim_restate's own entries."""
    params = [np.asarray(p, F) for p in params]
    m = [np.zeros_like(p) for p in params]
    v = [np.zeros_like(p) for p in params]
    applied = first_step
    scale = F(scale)
    for k, grads in enumerate(grads_per_step):
        gu = unscale(grads, scale)
        ssq = sum_of_squares(gu)
        skip = not math.isfinite(ssq)
        used = scale
        info = {}
        if skip:
            skipped += 1
        else:
            params, m, v, info = next(orr.run(params, [gu], total_steps, first_step=applied, exp_avg=m, exp_avg_sq=v,
                                              coefs=None if coefs is None else [coefs[k]], **settings))
            applied += 1
        scale, tracker = update_scale(scale, tracker, skip, growth_factor, backoff_factor, growth_interval, min_scale)
        yield params, m, v, dict(info, skip=skip, scale_used=used, scale=scale, tracker=tracker, skipped=skipped, applied=applied)

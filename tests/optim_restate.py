"""The optimiser step of include/epnet_ops.h (epnet_adam_onecycle_step) restated on the CPU in numpy: the one-cycle schedule and
its row, the clip, and the float32 update in source order. Written from the header's formulas, independently of
epnet_amd/optim.py; tests/test_optim.py holds it to the reference's own run (tests/golden/optim.npz), tests/test_optim_gpu.py
holds the kernels to it bit for bit.

A step takes lists of float32 arrays (one per tensor; a gradient may be None: the tensor only decays) and returns new lists.
"""
import math

import numpy as np

F = np.float32


def one_cycle(t, total_steps, lr_max=0.002, moms=(0.95, 0.85), div_factor=10.0, pct_start=0.4):
    """(lr, mom) of step t in Python doubles: cosine from `start` to `end`, end + (start - end) / 2 * (cos(pi pct) + 1), first
    phase [0, a1), second [a1, total) with a1 = int(total * pct_start)"""
    a1 = int(total_steps * pct_start)
    low = lr_max / div_factor

    def anneal(start, end, pct):
        return end + (start - end) / 2 * (np.cos(np.pi * pct) + 1)
    if t >= a1:
        pct = (t - a1) / (total_steps - a1)
        return float(anneal(lr_max, low / 1e4, pct)), float(anneal(moms[1], moms[0], pct))
    pct = t / a1
    return float(anneal(low, lr_max, pct)), float(anneal(moms[0], moms[1], pct))


def row(t, lr, mom, wd, b2):
    """the step's scalars, computed in double and rounded once to float32"""
    return {"decay": F(1 - wd * lr), "b1": F(mom), "omb1": F(1 - mom), "step_size": F(lr / (1 - mom ** (t + 1))),
            "bc2_sqrt": F(math.sqrt(1 - b2 ** (t + 1))), "lr": F(lr), "mom": F(mom)}


def total_norm(grads):
    """L2 norm over every gradient present, in float64"""
    return math.sqrt(sum(float(np.sum(np.asarray(g, np.float64) ** 2)) for g in grads if g is not None))


def clip_coef(norm, clip):
    return F(min(1.0, clip / (norm + 1e-6)))


def step(params, grads, exp_avg, exp_avg_sq, r, coef, b2, eps):
    """one update with the row r and the clip coefficient coef (float32): new (params, exp_avg, exp_avg_sq)"""
    b2f, omb2, epsf, coef = F(b2), F(1.0 - b2), F(eps), F(coef)
    out_p, out_m, out_v = [], [], []
    for p, g, m, v in zip(params, grads, exp_avg, exp_avg_sq):
        p, m, v = np.asarray(p, F), np.asarray(m, F), np.asarray(v, F)
        p = p * r["decay"]
        if g is not None:
            gc = np.asarray(g, F) * coef
            m = m * r["b1"] + r["omb1"] * gc
            v = v * b2f + omb2 * gc * gc
            p = p - r["step_size"] * (m / (np.sqrt(v) / r["bc2_sqrt"] + epsf))
        assert p.dtype == F and m.dtype == F and v.dtype == F
        out_p.append(p); out_m.append(m); out_v.append(v)
    return out_p, out_m, out_v


def run(params, grads_per_step, total_steps, wd=0.001, b2=0.99, eps=1e-8, clip=1.0, first_step=0, exp_avg=None, exp_avg_sq=None,
        coefs=None, **schedule):
    """len(grads_per_step) steps from step index first_step; coefs: per-step clip coefficients to use instead of this module's
    own (the GPU tests pass the device's). Yields (params, exp_avg, exp_avg_sq, info) after every step."""
    m = [np.zeros_like(np.asarray(p, F)) for p in params] if exp_avg is None else exp_avg
    v = [np.zeros_like(np.asarray(p, F)) for p in params] if exp_avg_sq is None else exp_avg_sq
    for k, grads in enumerate(grads_per_step):
        t = first_step + k
        used = min(t, total_steps - 1)
        lr, mom = one_cycle(used, total_steps, **schedule)
        r = row(used, lr, mom, wd, b2)
        norm = total_norm(grads)
        coef = clip_coef(norm, clip) if coefs is None else F(coefs[k])
        params, m, v = step(params, grads, m, v, r, coef, b2, eps)
        yield params, m, v, {"lr": lr, "mom": mom, "total_norm": norm, "coef": coef, "step": used, "past_end": t >= total_steps}

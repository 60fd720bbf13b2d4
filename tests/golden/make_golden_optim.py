"""Regenerates tests/golden/optim.npz. Runs ONLY in the build container (needs /root/reference), on the CPU; the fixture is plain data.

What runs is the REFERENCE'S OWN Python, imported unmodified from /root/reference/tools/train_utils: ``fastai_optim.OptimWrapper``
created as tools/train_rcnn.py:101-114 creates it (flattened leaf modules, Adam with betas (0.9, 0.99), wd, true_wd, bn_wd),
``learning_schedules_fastai.OneCycle`` with the yaml's values, and torch's ``clip_grad_norm_``, over the installed torch, in the
order of train_utils.py:126-136 with the scheduler stepped per iteration before it (:186-187). ``collections.Iterable`` is
aliased first (fastai_optim.py:3 predates its removal); no bytecode is written.

The model is tests/optim_cases.build_model(). STEPS steps of a TOTAL_STEPS cycle with stored gradients: every third step's
gradients have a norm of about 450 (the clip engages), the others about 0.45 (coef is 1). One parameter is frozen after the
optimiser exists, one never gets a gradient. The same run is made in float64 (the yardstick) and in float32.

Stored: p0 (initial parameters, flat in optim_cases.NAMES order), grads (STEPS, flat over GRAD_NAMES), lr / mom (float64, what
the scheduler set), total_norm (float64 run), p32 / p64 (STEPS, flat: the parameters after each step), err32 (max |p32 - p64| per
step), upd (max |p64[t] - p64[t-1]|), order (the names of the reference's state-dict indices), groups (parameters per group),
has_state, step, m32 / v32 (exp_avg / exp_avg_sq of the float32 run after the last step, flat in `order`'s order over the
entries that have state), schedule_lr / schedule_mom (all TOTAL_STEPS steps of the scheduler, float64).
"""
import collections
import collections.abc
import os
import sys
from functools import partial

import numpy as np
import torch
from torch import nn, optim
from torch.nn.utils import clip_grad_norm_

sys.dont_write_bytecode = True
collections.Iterable = collections.abc.Iterable

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, "/root/reference/tools")

import optim_cases as oc  # noqa: E402
from train_utils.fastai_optim import OptimWrapper  # noqa: E402
from train_utils import learning_schedules_fastai as lsf  # noqa: E402


def make_inputs():
    rng = np.random.default_rng(20240521)
    p0 = {n: (rng.standard_normal(oc.SHAPES[n]) * 0.5).astype(np.float32) for n in oc.NAMES}
    for n in ("bn1.weight", "bn2.weight"):
        p0[n] = (1 + 0.1 * rng.standard_normal(oc.SHAPES[n])).astype(np.float32)
    count = sum(oc.numel(n) for n in oc.GRAD_NAMES)
    grads = np.empty((oc.STEPS, count), np.float32)
    for t in range(oc.STEPS):
        g = rng.standard_normal(count)
        grads[t] = (g / np.linalg.norm(g) * (450.0 if t % 3 == 2 else 0.45) * rng.uniform(0.9, 1.1)).astype(np.float32)
    return oc.join(p0), grads


def run(p0, grads, dtype):
    model = oc.build_model().to(dtype)
    oc.set_params(model, p0, dtype)
    named = dict(model.named_parameters())

    leaves = [m for m in model.modules() if not any(True for _ in m.children())]       # the model flattened to its leaf modules
    wrapper = OptimWrapper.create(partial(optim.Adam, betas=(0.9, oc.BETA2)), 3e-3, [nn.Sequential(*leaves)], wd=oc.WD,
                                  true_wd=True, bn_wd=True)
    named[oc.FROZEN].requires_grad = False
    sched = lsf.OneCycle(wrapper, oc.TOTAL_STEPS, oc.SETTINGS["lr_max"], list(oc.SETTINGS["moms"]), oc.SETTINGS["div_factor"],
                         oc.SETTINGS["pct_start"])
    out = {"lr": [], "mom": [], "total_norm": [], "p": []}
    for it in range(oc.STEPS):
        sched.step(it)
        wrapper.zero_grad()
        for n, g in oc.split(grads[it], oc.GRAD_NAMES).items():
            named[n].grad = torch.from_numpy(np.array(g)).to(dtype)  # a copy: the clip scales it in place
        norm = clip_grad_norm_(model.parameters(), oc.CLIP)
        wrapper.step()
        out["lr"].append(float(wrapper.lr)); out["mom"].append(float(wrapper.mom)); out["total_norm"].append(float(norm))
        out["p"].append(oc.join({n: named[n].detach().numpy() for n in oc.NAMES}))
    name_of = {id(p): n for n, p in named.items()}
    sd = wrapper.opt.state_dict()
    out["order"] = [name_of[id(p)] for g in wrapper.opt.param_groups for p in g["params"]]
    out["groups"] = [len(g["params"]) for g in sd["param_groups"]]
    out["state"] = sd["state"]
    schedule = ([], [])
    for t in range(oc.TOTAL_STEPS):
        sched.step(t)
        schedule[0].append(float(wrapper.lr)); schedule[1].append(float(wrapper.mom))
    out["schedule"] = schedule
    return out


def main():
    p0, grads = make_inputs()
    r64, r32 = run(p0, grads, torch.float64), run(p0, grads, torch.float32)
    assert r64["lr"] == r32["lr"] and r64["mom"] == r32["mom"] and r64["order"] == r32["order"]
    p64, p32 = np.stack(r64["p"]), np.stack(r32["p"])
    assert p64.dtype == np.float64 and p32.dtype == np.float32
    err32 = np.abs(p32.astype(np.float64) - p64).max(axis=1)
    prev = np.concatenate([p0[None].astype(np.float64), p64[:-1]])
    upd = np.abs(p64 - prev).max(axis=1)
    has_state = [int(k in r32["state"]) for k in range(len(r32["order"]))]
    steps = {float(s["step"]) for s in r32["state"].values()}
    assert steps == {float(oc.STEPS)}
    m32 = np.concatenate([r32["state"][k]["exp_avg"].numpy().reshape(-1) for k in range(len(has_state)) if has_state[k]])
    v32 = np.concatenate([r32["state"][k]["exp_avg_sq"].numpy().reshape(-1) for k in range(len(has_state)) if has_state[k]])
    np.savez_compressed(oc.FIXTURE, p0=p0, grads=grads, lr=np.array(r64["lr"]), mom=np.array(r64["mom"]),
                        total_norm=np.array(r64["total_norm"]), p32=p32, p64=p64, err32=err32, upd=upd, order=np.array(r32["order"]),
                        groups=np.array(r32["groups"]), has_state=np.array(has_state), step=np.array(oc.STEPS), m32=m32, v32=v32,
                        schedule_lr=np.array(r64["schedule"][0]), schedule_mom=np.array(r64["schedule"][1]))
    print("wrote", oc.FIXTURE, os.path.getsize(oc.FIXTURE), "bytes")
    print("order", r32["order"], "groups", r32["groups"], "has_state", has_state)
    for t in range(oc.STEPS):
        print("step %2d lr %.6e mom %.6f norm %9.4f err32 %.2e update %.2e" % (t, r64["lr"][t], r64["mom"][t], r64["total_norm"][t], err32[t], upd[t]))


if __name__ == "__main__":
    main()

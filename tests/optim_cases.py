"""The fixture model of tests/golden/optim.npz and the readers of that file, shared by its generator
(tests/golden/make_golden_optim.py), test_optim.py and test_optim_gpu.py.

The model is the smallest that has what the optimiser distinguishes: BatchNorm and other leaves (the state dict's two groups),
a bias-free layer, one parameter frozen after the optimiser is built (RPN.FIXED), one that never gets a gradient, and one
tensor (fc, 1031 elements) that is no multiple of 4. Flat vectors in the fixture hold the parameters in NAMES order."""
import os
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "optim.npz")

NAMES = ("conv1.weight", "conv1.bias", "bn1.weight", "bn1.bias", "conv2.weight", "bn2.weight", "bn2.bias", "fc.weight", "fc.bias")
SHAPES = {"conv1.weight": (7, 5, 1), "conv1.bias": (7,), "bn1.weight": (7,), "bn1.bias": (7,), "conv2.weight": (3, 7, 1),
          "bn2.weight": (3,), "bn2.bias": (3,), "fc.weight": (1031, 1), "fc.bias": (1031,)}
FROZEN = "bn2.weight"     # requires_grad = False after the optimiser exists
NO_GRAD = "conv1.bias"    # trainable, but its grad stays None
TOTAL_STEPS = 40
STEPS = 12
SETTINGS = dict(lr_max=0.002, moms=(0.95, 0.85), div_factor=10.0, pct_start=0.4)
WD, BETA2, EPS, CLIP = 0.001, 0.99, 1e-8, 1.0


def build_model():
    from torch import nn
    return nn.Sequential(OrderedDict([("conv1", nn.Conv1d(5, 7, 1)), ("bn1", nn.BatchNorm1d(7)), ("conv2", nn.Conv1d(7, 3, 1, bias=False)),
                                      ("bn2", nn.BatchNorm1d(3)), ("fc", nn.Linear(1, 1031))]))


def numel(name):
    return int(np.prod(SHAPES[name]))


def split(flat, names=NAMES):
    """a flat vector in `names` order -> {name: array of the parameter's shape}"""
    out, at = {}, 0
    for n in names:
        out[n] = np.asarray(flat[at:at + numel(n)]).reshape(SHAPES[n])
        at += numel(n)
    assert at == len(flat)
    return out


def join(by_name, names=NAMES):
    return np.concatenate([np.asarray(by_name[n]).reshape(-1) for n in names])


GRAD_NAMES = tuple(n for n in NAMES if n not in (FROZEN, NO_GRAD))


def load():
    return np.load(FIXTURE)


def set_params(model, flat, dtype=None):
    """the fixture's initial parameters into a build_model()"""
    import torch
    params = dict(model.named_parameters())
    with torch.no_grad():
        for n, a in split(flat).items():
            t = torch.from_numpy(np.ascontiguousarray(a))
            params[n].copy_(t if dtype is None else t.to(dtype))

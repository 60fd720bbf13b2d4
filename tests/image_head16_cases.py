"""TEST INFRASTRUCTURE shared by tests/test_image_head16.py and tests/test_image_head16_gpu.py: the yardsticks of the 16-bit image
head at the points (include/epnet_ops.h: epnet_image_head_points_h), all in stock float64 ops on the device
of their inputs.

  R  the rule without its inner rounding: float64 modules carrying the pack's ROUNDED weights (wd16 = round_T(wd), wf16 =
     round_T(wf), bias = shift), on maps.double(); neither d nor out is rounded
  A  the magnitude sum of the same expression: |wd16| on |F|, |wf16|, bias |shift|, no ReLU, then the sampler (linear, with
     non-negative tap weights)
  bound  |got - R| <= (2 u + (K + 8) 2^-24) A elementwise, u the unit roundoff of T, K = max C_l + sum R: rounding d costs at most
     u sum_j |wf16 d| <= u A, the final rounding at most u |out| <= u A, float32 accumulation over at most K terms about K 2^-24 A
  Y  the true head: the float64 head of the float32 modules on maps.double()
  S  what autocast runs today: the stock dense head under torch.autocast of T
"""
import torch
import torch.nn.functional as F

import image_head_cases as cases

CONFIGS = dict(cases.CONFIGS)
# R and q span several 16-column blocks of the MFMA, sum R = 64 is two whole K steps of stage 2
CONFIGS["wide"] = dict(chans=[40, 72], reduce=[24, 40], kernels=[4, 16], q=48, h=32, w=48, b=2, n=300)

UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TYPES = [torch.float16, torch.bfloat16]


def grid_xy(cfg, b=None, n=None, seed=2):
    """cases.make_xy on a grid of 2^-10: the float32 tap weights are exact (the device of test_full_size_scene)"""
    return torch.round(cases.make_xy(cfg, b, n, seed) * 1024.0) / 1024.0


def maps_of(cfg, dtype, b=None, seed=1):
    return [m.to(dtype) for m in cases.make_maps(cfg, b, seed)]


def _sample(fmap, xy):
    from epnet_amd.rpn_backbone import stock_feature_gather
    return stock_feature_gather(fmap, xy.double())


def _rounded_weights(packed, dtype):
    """float64 values of the rounded pack: per level ConvTranspose2d's (C, R, k, k), and the 1x1's (q, sum R, 1, 1)"""
    wd = [v.to(dtype).double().permute(2, 3, 0, 1).contiguous() for v in packed.weights]
    return wd, packed.wf.to(dtype).double()[:, :, None, None]


def _up(wd, maps, kernels, magnitude=False):
    parts = []
    for w, m, k in zip(wd, maps, kernels):
        w, m = (w.abs(), m.double().abs()) if magnitude else (w, m.double())
        parts.append(F.conv_transpose2d(m, w.to(m.device), stride=k))
    return parts


def rule_unrounded(packed, maps, xy, dtype):
    """R"""
    wd, wf = _rounded_weights(packed, dtype)
    up = torch.cat(_up(wd, maps, packed.kernels), dim=1)
    return _sample(F.relu(F.conv2d(up, wf.to(up.device), packed.shift.double().to(up.device))), xy)


def rule_magnitude(packed, maps, xy, dtype):
    """A"""
    wd, wf = _rounded_weights(packed, dtype)
    up = torch.cat(_up(wd, maps, packed.kernels, magnitude=True), dim=1)
    return _sample(F.conv2d(up, wf.abs().to(up.device), packed.shift.double().abs().to(up.device)), xy)


def rule_emulated(packed, maps, xy, dtype):
    """the rule itself in float64 with its two roundings (d and out); the sums are float64 instead of float32"""
    wd, wf = _rounded_weights(packed, dtype)
    up = torch.cat([d.to(dtype).double() for d in _up(wd, maps, packed.kernels)], dim=1)
    return _sample(F.relu(F.conv2d(up, wf.to(up.device), packed.shift.double().to(up.device))), xy).to(dtype)


def bound_factor(cfg, dtype):
    return 2.0 * UNIT[dtype] + (max(cfg["chans"]) + sum(cfg["reduce"]) + 8) * 2.0 ** -24


def worst_of_bound(got, packed, maps, xy, cfg, dtype):
    """max of |got - R| / bound (<= 1 passes) over the elements; an element with A == 0 must be exact"""
    ref, mag = rule_unrounded(packed, maps, xy, dtype), rule_magnitude(packed, maps, xy, dtype)
    err, lim = (got.double() - ref).abs(), bound_factor(cfg, dtype) * mag
    assert torch.isfinite(got.double()).all() and (err[lim == 0] == 0).all()
    return (err[lim > 0] / lim[lim > 0]).max().item() if (lim > 0).any() else 0.0


def true_head(head, maps, xy):
    """Y; `head` float32 modules on the maps' device"""
    with torch.no_grad():
        return cases.dense_head(cases.head_to(head, dtype=torch.float64), [m.double() for m in maps], xy.double())


def autocast_head(head, maps, xy, dtype):
    """S"""
    with torch.no_grad(), torch.autocast(maps[0].device.type, dtype):
        return cases.dense_head(head, maps, xy)

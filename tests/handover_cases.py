"""Inputs, the float64 yardstick, the exclusion rule and the tolerances of the RPN hand-over tests, shared by the CPU test (which
checks the test design: the stock float32 composition must itself pass) and the GPU tests.

Yardstick: ``bbox_transform.decode_bbox_target`` on float64 CPU copies. Tolerances: columns 0-5 rtol = atol = 1e-5 (the
project's parity for float outputs); column 6 the difference wrapped into (-pi, pi], at most 1e-5 (the ``> pi`` wrap is a
legitimate 2 pi flip between precisions). Rows left out, with ``ry_with_bin`` only, where the function is discontinuous -- the
conditions are evaluated in float64: a bin's heading within 1e-4 of its side boundary (pi coarse, 0 fine), a bin's heading within
1e-4 of the wrap points 0 / 2 pi (coarse), side masses closer than 1e-4. Their share is asserted to be at most 1 %.
"""
import functools
import math

import numpy as np
import torch

from epnet_amd.bbox_transform import decode_bbox_target

ANCHOR_SIZE = np.array([1.52563191462, 1.62856739989, 3.88311640418], dtype=np.float32)
TOL = 1e-5
EDGE = 1e-4
ROWS = (1, 63, 64, 65, 1000, 4099)
SCALES = (1.0, 3.0)

_RPN = dict(acols=3, loc_scope=3.0, loc_bin_size=0.5, num_head_bin=12, get_xz_fine=True, get_y_by_bin=False, loc_y_scope=0.5,
            loc_y_bin_size=0.25, get_ry_fine=False, bbox_avg_by_bin=True, ry_with_bin=False)
_RCNN = dict(acols=7, loc_scope=1.5, loc_bin_size=0.5, num_head_bin=9, get_xz_fine=True, get_y_by_bin=False, loc_y_scope=0.5,
             loc_y_bin_size=0.25, get_ry_fine=True, bbox_avg_by_bin=True, ry_with_bin=False)
CONFIGS = {
    "rpn_soft": _RPN,                                                       # the RPN yaml: 76 channels
    "rpn_hard": dict(_RPN, bbox_avg_by_bin=False),
    "rpn_ry_with_bin": dict(_RPN, ry_with_bin=True),
    "rcnn": _RCNN,                                                          # the RCNN yaml: 46 channels
    "rcnn_y_by_bin": dict(_RCNN, get_y_by_bin=True),                        # 53 channels
    "hard_coarse_xz": dict(_RPN, bbox_avg_by_bin=False, get_xz_fine=False),   # 52 channels
    "rcnn_ry_with_bin": dict(_RCNN, ry_with_bin=True),                      # the fine-heading side rule
    # the ends of the staging loop's (row, column) bookkeeping, dr = 256 / c, dc = 256 - dr * c (the names sort behind the
    # entries above, whose seeds depend on their place in the sorted list): the fewest channels the argument rules allow
    # (int(scope / bin) * 2 >= 2 bins per axis, one heading bin), either side of 128, and the two largest (255 = kMaxChannels)
    "staging_c010": dict(_RPN, loc_scope=0.5, num_head_bin=1, get_xz_fine=False, bbox_avg_by_bin=False),
    "staging_c128": dict(_RPN, loc_scope=6.0, num_head_bin=14),
    "staging_c129": dict(_RCNN, loc_scope=6.0, get_y_by_bin=True, loc_y_bin_size=0.5, num_head_bin=13),
    "staging_c254": dict(_RPN, loc_scope=12.5, num_head_bin=25, bbox_avg_by_bin=False),
    "staging_c255": dict(_RCNN, loc_scope=12.5, get_y_by_bin=True, loc_y_bin_size=0.5, num_head_bin=24, bbox_avg_by_bin=False),
}
STAGING = {"staging_c010": 10, "staging_c128": 128, "staging_c129": 129, "staging_c254": 254, "staging_c255": 255}
TOO_WIDE = dict(_RPN, loc_scope=12.5, num_head_bin=26)                      # 256 channels: one more than the LDS tile takes


def channels(cfg):
    nb = int(cfg["loc_scope"] / cfg["loc_bin_size"]) * 2
    nby = int(cfg["loc_y_scope"] / cfg["loc_y_bin_size"]) * 2
    return (4 if cfg["get_xz_fine"] else 2) * nb + (2 * nby if cfg["get_y_by_bin"] else 1) + 2 * cfg["num_head_bin"] + 3


def decode_kwargs(cfg):
    return {k: v for k, v in cfg.items() if k != "acols"}


def regression_values(rows, c, scale, seed):
    """N(0,1) * scale rounded to float16: exact in every wider format, and already full of exact ties between logits"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((rows, c), generator=g) * scale).half().float()


def anchors(rows, acols, seed):
    """points uniform in [-40, 40] x [-1, 3] x [0, 70.4]; 7-wide: car-like sizes and a heading in (-pi, pi)"""
    g = torch.Generator().manual_seed(seed + 104729)
    u = torch.rand((rows, 7), generator=g)
    a = torch.stack([u[:, 0] * 80 - 40, u[:, 1] * 4 - 1, u[:, 2] * 70.4, 1.2 + u[:, 3] * 0.8, 1.4 + u[:, 4] * 0.6, 3.0 + u[:, 5] * 2.0,
                     (u[:, 6] * 2 - 1) * math.pi], dim=1)
    return a[:, :acols].contiguous()


@functools.lru_cache(maxsize=None)
def case(name, rows, scale):
    """(anchors, pred_reg) float32 CPU tensors of a decode case; cached, never modified"""
    cfg = CONFIGS[name]
    seed = 1000 * sorted(CONFIGS).index(name) + rows + int(scale * 7)
    return anchors(rows, cfg["acols"], seed), regression_values(rows, channels(cfg), scale, seed)


def reference64(cfg, anchor, reg, y_to_bottom=False):
    box = decode_bbox_target(anchor.double(), reg.double(), anchor_size=torch.from_numpy(ANCHOR_SIZE).double(), **decode_kwargs(cfg))
    if y_to_bottom:
        box[:, 1] += box[:, 3] / 2
    return box


@functools.lru_cache(maxsize=None)
def case_reference(name, rows, scale):
    anchor, reg = case(name, rows, scale)
    return reference64(CONFIGS[name], anchor, reg), excluded(CONFIGS[name], reg)


def excluded(cfg, reg):
    """bool (rows): the rows at a discontinuity of the ry_with_bin heading, evaluated in float64"""
    rows = reg.shape[0]
    if not cfg["ry_with_bin"]:
        return torch.zeros((rows,), dtype=torch.bool)
    reg = reg.double()
    nb = int(cfg["loc_scope"] / cfg["loc_bin_size"]) * 2
    nby = int(cfg["loc_y_scope"] / cfg["loc_y_bin_size"]) * 2
    cursor = (4 if cfg["get_xz_fine"] else 2) * nb + (2 * nby if cfg["get_y_by_bin"] else 1)
    nh = cfg["num_head_bin"]
    logits, res = reg[:, cursor:cursor + nh], reg[:, cursor + nh:cursor + 2 * nh]
    prob = torch.softmax(logits, dim=1)
    k = torch.arange(nh, dtype=torch.float64)
    if cfg["get_ry_fine"]:
        per_bin = (math.pi / 2) / nh
        each = (k * per_bin + per_bin / 2) + res * (per_bin / 2) - math.pi / 4
        right = each >= 0
        at_edge = (each.abs() < EDGE).any(dim=1)
    else:
        per_bin = (2 * math.pi) / nh
        each = (k * per_bin + res * (per_bin / 2)) % (2 * math.pi)
        right = each <= math.pi
        at_edge = ((each - math.pi).abs() < EDGE).any(dim=1) | (each < EDGE).any(dim=1) | (each > 2 * math.pi - EDGE).any(dim=1)
    zero = torch.zeros_like(prob)
    mass_right, mass_left = torch.where(right, prob, zero).sum(dim=1), torch.where(right, zero, prob).sum(dim=1)
    return at_edge | ((mass_right - mass_left).abs() < EDGE)


def errors(boxes, ref, skip):
    """(largest |error| / (atol + rtol |ref|) over columns 0-5, largest wrapped heading error) on the kept rows, (-1, -1) if none"""
    keep = ~skip
    if not bool(keep.any()):
        return -1.0, -1.0
    got, want = boxes.double()[keep], ref[keep]
    size = ((got[:, :6] - want[:, :6]).abs() / (TOL + TOL * want[:, :6].abs())).max().item()
    d = got[:, 6] - want[:, 6]
    d = d - 2 * math.pi * torch.ceil((d - math.pi) / (2 * math.pi))          # into (-pi, pi]
    return size, d.abs().max().item()


def check(boxes, ref, skip, what):
    """assert the tolerances; returns the two figures. A NaN anywhere fails."""
    assert boxes.shape == ref.shape and boxes.dtype == torch.float32, what
    assert float(skip.float().mean()) <= 0.01, (what, "rows left out", float(skip.float().mean()))
    size, heading = errors(boxes, ref, skip)
    print("%s: columns 0-5 at %.3f of the tolerance, heading error %.3e, %d of %d rows left out" % (what, size, heading, int(skip.sum()), len(skip)))
    assert size == size and heading == heading, (what, "NaN")
    assert size <= 1.0, (what, size)
    assert heading <= TOL, (what, heading)
    return size, heading


def score_kinds(b, n, seed):
    """name -> scores (b, n) float32: distinct values; all equal; two values only; mixed +-0.0; +-inf; a few NaN"""
    g = torch.Generator().manual_seed(seed)
    distinct = torch.stack([torch.randperm(n, generator=g) for _ in range(b)]).float() / 8 - n / 16
    two = torch.where(torch.rand((b, n), generator=g) < 0.5, torch.tensor(-1.5), torch.tensor(2.25))
    zeros = torch.where(torch.rand((b, n), generator=g) < 0.5, torch.tensor(-0.0), torch.tensor(0.0))
    zeros = torch.where(torch.rand((b, n), generator=g) < 0.2, torch.randn((b, n), generator=g).half().float(), zeros)
    infs = torch.randn((b, n), generator=g).half().float()
    u = torch.rand((b, n), generator=g)
    infs = torch.where(u < 0.1, torch.tensor(float("inf")), torch.where(u > 0.9, torch.tensor(float("-inf")), infs))
    nans = torch.where(torch.rand((b, n), generator=g) < 0.05, torch.tensor(float("nan")), infs)
    return {"distinct": distinct.contiguous(), "equal": torch.full((b, n), 0.75), "two": two, "zeros": zeros, "infs": infs, "nans": nans}


def stable_order(scores):
    return torch.sort(scores.cpu(), dim=1, descending=True, stable=True)[1]


@functools.lru_cache(maxsize=None)
def scene_inputs(n, seed=11, scale=1.0):
    """(scores (2,n) distinct, rpn_reg (2,n,76), xyz (2,n,3)) float32 CPU tensors for the end-to-end test; scene 1 has no point
    beyond z = 40 (the empty-far-bin branch of the distance-based proposal)"""
    from epnet_amd import synth
    xyz = synth.scenes("kitti", 2, n, seed=seed)
    xyz[1, :, 2] = xyz[1, :, 2] * (39.0 / 70.4)
    g = torch.Generator().manual_seed(seed)
    scores = torch.stack([torch.randperm(n, generator=g) for _ in range(2)]).float() * (12.0 / n) - 6.0   # distinct, either side of any threshold
    reg = regression_values(2 * n, 76, scale, seed).view(2, n, 76)
    return scores.contiguous(), reg.contiguous(), xyz.contiguous()

"""The NMS kernels on suppression patterns that random proposal sets do not contain: a chain of mutually-neighbouring boxes (all 64
rounds of nms_sweep_kernel's fixed-point iteration inside a tile), a suppressed suppressor in an earlier tile, one box that
suppresses 2048 others, 2049 boxes that all stay; the batched path of the proposal layer on such scenes; and rotated NMS at
threshold 0 around the hull pre-filter of nms_mask_rot_kernel.

Every pattern is laid out in a frame of its own (u along the boxes' length): box = (u, v, length, width) with small dyadic
numbers. At angle 0 the frame is the world and all coordinates and IoUs are exact in float32; the exact IoU of a pair is the
axis-aligned formula in the frame at ANY common angle. Pair IoUs are 0, 1/3 or at least 0.6 against thresholds of 0.25, so the
expected keep list -- the plain greedy loop of tests/exact_geometry.py on the frame's IoU matrix, cross-checked against
oracle.nms -- is exact. At the common non-zero angle the world coordinates are rounded to float32; there the threshold is the
midpoint of the two exact IoU levels (tests/exact_geometry.py on the float32 boxes) either side of 0.25, with the gap asserted."""
import functools

import numpy as np
import pytest
import torch

import exact_geometry as eg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F = np.float32
ANGLE = 0.4375          # the common non-zero angle
THRESH = 0.25
ORACLE_HEAD = 321       # the oracle's rotated NMS of 2049 mutually overlapping boxes takes seconds: it cross-checks the first 321
                        # boxes, whose greedy list is the head of the whole one (every pattern but the two of 2049 is shorter)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- patterns: rows (u, v, length, width) in score order ---------------------------------------------------------------------------
def fillers(n, row=0):
    """n unit boxes 3 apart on lines of their own, far from everything at v <= 1"""
    k = np.arange(n)
    return np.stack([3.0 * (k % 40), 8.0 + 3.0 * (k // 40) + 40.0 * row, np.ones(n), np.ones(n)], axis=1)


def chain(n, lead=0):
    """box i overlaps only i +- 1: IoU(i, i+1) = 1/3, IoU(i, i+2) = 0; `lead` disjoint boxes first"""
    k = np.arange(n)
    links = np.stack([0.5 * k, np.zeros(n), np.ones(n), np.ones(n)], axis=1)
    return np.concatenate([fillers(lead), links]), np.concatenate([np.arange(lead), lead + k[::2]])


def star(n=2049):
    """box 0, 64 x 64, and 2048 distinct copies moved by less than (8, 4): every IoU is at least 0.6"""
    j = np.arange(1, n)
    moved = np.stack([32.0 + (j % 64) / 8.0, 32.0 + (j // 64) / 8.0, np.full(n - 1, 64.0), np.full(n - 1, 64.0)], axis=1)
    return np.concatenate([[[32.0, 32.0, 64.0, 64.0]], moved]), np.array([0])


def disjoint(n=2049):
    k = np.arange(n)
    return np.stack([2.0 * (k % 50), 2.0 * (k // 50), np.ones(n), np.ones(n)], axis=1), k


def suppressed_suppressor(n, first, second, third):
    """`first` suppresses `second`; `second` overlaps `third`, which `first` does not touch: `third` stays"""
    boxes = fillers(n)
    for pos, u in ((first, 0.0), (second, 0.5), (third, 1.0)):
        boxes[pos] = (u, 0.0, 1.0, 1.0)
    return boxes, np.array([k for k in range(n) if k != second])


PATTERNS = {"chain64": lambda: chain(64), "chain65": lambda: chain(65), "chain130": lambda: chain(130), "chain200": lambda: chain(200),
            "lead37_chain64": lambda: chain(64, 37), "lead37_chain65": lambda: chain(65, 37), "lead37_chain130": lambda: chain(130, 37),
            "lead37_chain200": lambda: chain(200, 37), "star2049": star, "disjoint2049": disjoint,
            "suppressor_across_tiles": lambda: suppressed_suppressor(141, 1, 70, 140),
            "suppressor_in_one_tile": lambda: suppressed_suppressor(64, 1, 20, 40)}


def frame_iou(p):
    """the exact IoU matrix of a pattern: axis-aligned in its frame"""
    lo, hi = p[:, 0:2] - p[:, 2:4] / 2, p[:, 0:2] + p[:, 2:4] / 2
    side = np.maximum(np.minimum(hi[:, None], hi[None, :]) - np.maximum(lo[:, None], lo[None, :]), 0.0)
    inter = side[..., 0] * side[..., 1]
    area = p[:, 2] * p[:, 3]
    return inter / (area[:, None] + area[None, :] - inter)


def world_bev(p, angle):
    """frame rows -> BEV boxes (n,5) float32 at `angle`: the frame's u axis is the boxes' own length axis, (1, 0) turned"""
    c, s = np.cos(angle), np.sin(angle)
    cx, cy = p[:, 0] * c + p[:, 1] * s, -p[:, 0] * s + p[:, 1] * c
    return np.stack([cx - p[:, 2] / 2, cy - p[:, 3] / 2, cx + p[:, 2] / 2, cy + p[:, 3] / 2, np.full(len(p), angle)], axis=1).astype(F)


@functools.lru_cache(maxsize=None)
def pattern(name):
    p, keep = PATTERNS[name]()
    iou = frame_iou(p)
    assert np.array_equal(eg.greedy_nms(iou, THRESH), keep), name                  # the greedy loop gives the list the pattern states
    upper = iou[np.triu_indices(len(p), 1)]
    assert not ((upper > 0.01) & (upper < 0.33)).any() and abs(upper[(upper > 0.01) & (upper < 0.5)] - 1 / 3).max(initial=0) < 1e-12
    return p, keep, iou


def rotated_threshold(p, iou, boxes):
    """the midpoint of the two exact IoU levels of the float32 boxes either side of THRESH, over every pair up to 20000 per side
    (a seeded sample beyond that; box 0's pairs always)"""
    rng = np.random.RandomState(1)
    i, j = np.triu_indices(len(p), 1)
    levels = []
    for side in (iou[i, j] > THRESH, iou[i, j] <= THRESH):
        idx = np.nonzero(side)[0]
        if idx.size > 20000:
            idx = np.union1d(rng.choice(idx, 20000, replace=False), idx[i[idx] == 0])
        ov = eg.overlap_bev_pairs(boxes[i[idx]], boxes[j[idx]])
        levels.append(ov / (eg.area_bev(boxes[i[idx]]) + eg.area_bev(boxes[j[idx]]) - ov))
    above = levels[0].min() if levels[0].size else 1.0
    below = levels[1].max() if levels[1].size else 0.0
    assert above - below > 0.3, (above, below)
    return (above + below) / 2


def run(fn_name, boxes, thresh):
    from epnet_amd import iou3d_cuda
    keep, num = getattr(iou3d_cuda, fn_name)(dev(boxes), thresh)
    n = int(num.item())
    return keep.cpu().numpy()[:n]


@pytest.mark.parametrize("name", list(PATTERNS))
def test_pattern(hiplib, oracle, name):
    p, keep, iou = pattern(name)
    flat = world_bev(p, 0.0)
    assert np.array_equal(flat[:, 0:2].astype(np.float64), p[:, 0:2] - p[:, 2:4] / 2) and np.array_equal(
        flat[:, 2:4].astype(np.float64), p[:, 0:2] + p[:, 2:4] / 2)                # angle 0: the float32 boxes are the pattern itself
    head = min(len(p), ORACLE_HEAD)
    for rotated in (False, True):
        assert np.array_equal(oracle.nms(flat[:head], THRESH, rotated), keep[keep < head]), (name, rotated)
        got = run("nms_device" if rotated else "nms_normal_device", flat, THRESH)
        assert np.array_equal(got, keep), (name, "rotated kernel, angle 0" if rotated else "normal kernel")
    turned = world_bev(p, ANGLE)
    thresh = rotated_threshold(p, iou, turned)
    assert np.array_equal(oracle.nms(turned[:head], thresh, True), keep[keep < head]), name
    assert np.array_equal(run("nms_device", turned, thresh), keep), (name, "rotated kernel, angle %g" % ANGLE, thresh)


# ---- the batched path ----------------------------------------------------------------------------------------------------------------
def test_proposal_layer_on_a_chain_and_a_star(hiplib, oracle):
    """rpn_proposals_gpu, score based: scene 0 a chain (65 of the first 130 stay: more than post), scene 1 a star (one stays: fewer)"""
    from epnet_amd import iou3d_cuda
    n, pre, post = 150, 130, 32
    frames = [chain(n)[0], star(n)[0]]
    frames[1][:, 0:2] /= 2                                                         # 32 x 32 boxes moved by less than (4, 2)
    frames[1][:, 2:4] /= 2
    for angle in (0.0, ANGLE):
        props = np.zeros((2, n, 7), F)
        for k, p in enumerate(frames):
            c, s = np.cos(angle), np.sin(angle)
            props[k] = np.stack([p[:, 0] * c + p[:, 1] * s, np.full(n, 1.5), -p[:, 0] * s + p[:, 1] * c + 10.0, np.full(n, 1.5), p[:, 3], p[:, 2],
                                 np.full(n, angle)], axis=1)
        scores = np.tile((1.0 - np.arange(n) / n).astype(F), (2, 1))
        order = np.tile(np.arange(n), (2, 1))
        rb, rs = torch.full((2, post, 7), float("nan"), device=DEV), torch.full((2, post), float("nan"), device=DEV)
        rc = torch.full((2,), -1, dtype=torch.int32, device=DEV)
        iou3d_cuda.rpn_proposals_gpu(dev(props), dev(scores), dev(order), False, pre, post, THRESH, True, rb, rs, rc)
        want_b, want_s, want_c = oracle.rpn_proposals(props, scores, order, False, pre, post, THRESH, True)
        assert want_c.tolist() == [post, 1]
        assert np.array_equal(want_b[0, :, 0], props[0, 0:2 * post:2, 0])          # the even positions of the chain
        assert rc.cpu().numpy().tolist() == want_c.tolist()
        assert np.array_equal(rb.cpu().numpy(), want_b) and np.array_equal(rs.cpu().numpy(), want_s)


# ---- the hull pre-filter -------------------------------------------------------------------------------------------------------------
GAPS = (0.0, 5e-4, 2e-3, -0.5)      # between the axis-aligned hulls of a pair: touching, inside the filter's 1e-3, outside, overlapping


def hull_pairs(angle):
    """86 pairs of unit boxes at one angle, pair k at (8 (k % 16), 8 (k // 16)): the second box moved along the world's x by the
    hull's width plus GAPS[k % 4]. Order: the first boxes of 70 pairs, then their partners (a pair is 70 positions apart: across
    a tile boundary), then 16 pairs side by side (inside a tile)"""
    width = abs(np.cos(angle)) + abs(np.sin(angle))                                  # the hull of a unit box
    first, second = [], []
    for k in range(86):
        x, y = 8.0 * (k % 16), 8.0 * (k // 16)
        first.append((x - 0.5, y - 0.5, x + 0.5, y + 0.5, angle))
        x2 = x + width + GAPS[k % 4]
        second.append((x2 - 0.5, y - 0.5, x2 + 0.5, y + 0.5, angle))
    rows = first[:70] + second[:70]
    for k in range(70, 86):
        rows += [first[k], second[k]]
    return np.array(rows, F)


@pytest.mark.parametrize("angle", [0.0, ANGLE])
def test_threshold_zero_around_the_hull_filter(hiplib, oracle, angle):
    boxes = hull_pairs(angle)
    want = oracle.nms(boxes, 0.0, True)
    got = run("nms_device", boxes, 0.0)
    exact = eg.iou_bev(boxes, boxes)
    overlapping = int((exact[np.triu_indices(len(boxes), 1)] > 1e-3).sum())
    assert overlapping == 21                                                       # the GAPS[3] pairs, and only they, share area
    assert len(boxes) - 21 - 22 <= len(want) <= len(boxes) - 21                    # at most the 22 touching pairs go as well
    assert np.array_equal(got, want), (angle, sorted(set(want.tolist()) ^ set(got.tolist())))

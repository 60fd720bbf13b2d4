"""Stand-in of an extension module the reference does not have: its AP evaluator is numba (tools/kitti_object_eval_python/
rotate_iou.py, a numba.cuda kernel, and eval.py's CPU JIT). One function per entry point of csrc/kitti_eval.hip
(include/epnet_ops.h, "The KITTI AP evaluator"), on the tensors' device and current stream; ``kitti_thresholds_cpu`` is the host op.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from . import pointnet2_utils
from ._tensor import dev_ptr, host_ptr, need, on_device_of, writes

_D = torch.float64
_I = torch.int32
_L = torch.int64

MAX_DT, MAX_GT, MAX_DC, MAX_COMBOS, MAX_THRESHOLDS = 1024, 256, 256, 16, 64   # EPNET_KITTI_MAX_*
BOX_WIDTH = (4, 5, 7)


def workspace(like, frames, combos, tstride):
    """epnet_kitti_pr's scratch, from the package's allocation helper (the GPU tests put canaries around it)"""
    nbytes = _lib.lib().epnet_kitti_pr_workspace_bytes(frames, combos, tstride)
    return pointnet2_utils._new(like, (max(nbytes, 16),), torch.uint8)


def _host_array(values, ctype):
    return (ctype * max(len(values), 1))(*values)


@writes("overlaps")
def kitti_overlaps_gpu(metric, criterion, max_rows, max_cols, row_off, col_off, ov_off, row_boxes, col_boxes, overlaps):
    """row_off / col_off (F+1) int32, ov_off (F+1) int64, boxes (n, 4 | 5 | 7) float64 -> overlaps (ov_off[F]) float64"""
    frames = row_off.numel() - 1
    if metric not in (0, 1, 2):
        raise RuntimeError("metric must be 0 (bbox), 1 (bev) or 2 (3d)")
    pr, pc, po = dev_ptr(row_off, "row_off", _I), dev_ptr(col_off, "col_off", _I), dev_ptr(ov_off, "ov_off", _L)
    need(col_off, frames + 1, "col_off"); need(ov_off, frames + 1, "ov_off")
    pa, pb, pv = dev_ptr(row_boxes, "row_boxes", _D), dev_ptr(col_boxes, "col_boxes", _D), dev_ptr(overlaps, "overlaps", _D)
    if row_boxes.numel() % BOX_WIDTH[metric] or col_boxes.numel() % BOX_WIDTH[metric]:
        raise RuntimeError("metric %d takes boxes of %d columns" % (metric, BOX_WIDTH[metric]))
    with on_device_of(overlaps) as s:
        _lib.check(_lib.lib().epnet_kitti_overlaps(int(metric), int(criterion), frames, int(max_rows), int(max_cols), pr, pc, po, pa, pb,
                                                   pv, s), "kitti_overlaps")
    return 1


@writes("matched")
def kitti_match_gpu(max_gt, max_dt, combo_difficulty, combo_min_overlap, gt_off, dt_off, ov_off, overlaps, dt_score, ignored_gt,
                    ignored_dt, matched):
    """ignored_gt (D, total_gt) / ignored_dt (D, total_dt) int32, dt_score (total_dt) float64 -> matched (combos, total_gt) float64"""
    frames, combos = gt_off.numel() - 1, len(combo_difficulty)
    if ignored_gt.dim() != 2 or ignored_dt.dim() != 2 or ignored_gt.shape[0] != ignored_dt.shape[0]:
        raise RuntimeError("ignored_gt and ignored_dt must be (difficulties, rows)")
    nd, total_gt, total_dt = ignored_gt.shape[0], ignored_gt.shape[1], ignored_dt.shape[1]
    if len(combo_min_overlap) != combos:
        raise RuntimeError("one min_overlap per combination")
    pg, pd, po = dev_ptr(gt_off, "gt_off", _I), dev_ptr(dt_off, "dt_off", _I), dev_ptr(ov_off, "ov_off", _L)
    need(dt_off, frames + 1, "dt_off"); need(ov_off, frames + 1, "ov_off")
    pv, ps = dev_ptr(overlaps, "overlaps", _D), dev_ptr(dt_score, "dt_score", _D)
    pig, pid, pm = dev_ptr(ignored_gt, "ignored_gt", _I), dev_ptr(ignored_dt, "ignored_dt", _I), dev_ptr(matched, "matched", _D)
    need(dt_score, total_dt, "dt_score"); need(matched, combos * total_gt, "matched")
    cd, cm = _host_array([int(v) for v in combo_difficulty], ctypes.c_int), _host_array([float(v) for v in combo_min_overlap], ctypes.c_double)
    with on_device_of(matched) as s:
        _lib.check(_lib.lib().epnet_kitti_match(frames, total_gt, total_dt, int(max_gt), int(max_dt), nd, combos,
                                                ctypes.cast(cd, ctypes.c_void_p), ctypes.cast(cm, ctypes.c_void_p), pg, pd, po, pv, ps, pig,
                                                pid, pm, s), "kitti_match")
    return 1


@writes("pr_counts", "pr_similarity")
def kitti_pr_gpu(max_gt, max_dt, max_dc, metric, compute_aos, combo_difficulty, combo_min_overlap, combo_num_thresholds, gt_off, dt_off,
                 dc_off, ov_off, overlaps, dt_score, ignored_gt, ignored_dt, dt_bbox, dc_bbox, gt_alpha, dt_alpha, thresholds,
                 pr_counts, pr_similarity, ws=None):
    """thresholds (combos, tstride) float64 -> pr_counts (combos, tstride, 3) int32 = tp, fp, fn; pr_similarity (combos, tstride)"""
    frames, combos = gt_off.numel() - 1, len(combo_difficulty)
    if thresholds.dim() != 2 or thresholds.shape[0] != combos:
        raise RuntimeError("thresholds must be (combinations, tstride)")
    tstride = thresholds.shape[1]
    if ignored_gt.dim() != 2 or ignored_dt.dim() != 2 or ignored_gt.shape[0] != ignored_dt.shape[0]:
        raise RuntimeError("ignored_gt and ignored_dt must be (difficulties, rows)")
    nd, total_gt, total_dt = ignored_gt.shape[0], ignored_gt.shape[1], ignored_dt.shape[1]
    if len(combo_min_overlap) != combos or len(combo_num_thresholds) != combos:
        raise RuntimeError("one min_overlap and one threshold count per combination")
    pg, pd, pq, po = dev_ptr(gt_off, "gt_off", _I), dev_ptr(dt_off, "dt_off", _I), dev_ptr(dc_off, "dc_off", _I), dev_ptr(ov_off, "ov_off", _L)
    need(dt_off, frames + 1, "dt_off"); need(dc_off, frames + 1, "dc_off"); need(ov_off, frames + 1, "ov_off")
    pv, ps = dev_ptr(overlaps, "overlaps", _D), dev_ptr(dt_score, "dt_score", _D)
    pig, pid = dev_ptr(ignored_gt, "ignored_gt", _I), dev_ptr(ignored_dt, "ignored_dt", _I)
    pbb, pdc = dev_ptr(dt_bbox, "dt_bbox", _D), dev_ptr(dc_bbox, "dc_bbox", _D)
    pga, pda, pt = dev_ptr(gt_alpha, "gt_alpha", _D), dev_ptr(dt_alpha, "dt_alpha", _D), dev_ptr(thresholds, "thresholds", _D)
    pc, pz = dev_ptr(pr_counts, "pr_counts", _I), dev_ptr(pr_similarity, "pr_similarity", _D)
    need(dt_score, total_dt, "dt_score"); need(dt_bbox, total_dt * 4, "dt_bbox"); need(dt_alpha, total_dt, "dt_alpha")
    need(gt_alpha, total_gt, "gt_alpha"); need(pr_counts, combos * tstride * 3, "pr_counts"); need(pr_similarity, combos * tstride, "pr_similarity")
    if ws is None:
        ws = workspace(pr_counts, frames, combos, tstride)
    pw = dev_ptr(ws, "workspace", torch.uint8)
    cd, cm = _host_array([int(v) for v in combo_difficulty], ctypes.c_int), _host_array([float(v) for v in combo_min_overlap], ctypes.c_double)
    cn = _host_array([int(v) for v in combo_num_thresholds], ctypes.c_int)
    with on_device_of(pr_counts) as s:
        _lib.check(_lib.lib().epnet_kitti_pr(frames, total_gt, total_dt, int(max_gt), int(max_dt), int(max_dc), nd, combos, tstride,
                                             int(metric), int(bool(compute_aos)), ctypes.cast(cd, ctypes.c_void_p),
                                             ctypes.cast(cm, ctypes.c_void_p), ctypes.cast(cn, ctypes.c_void_p), pg, pd, pq, po, pv, ps,
                                             pig, pid, pbb, pdc, pga, pda, pt, pw, ws.numel(), pc, pz, s), "kitti_pr")
    return 1


def kitti_thresholds_cpu(matched, num_gt, num_sample_pts=41):
    """get_thresholds (eval.py:8-25) of one combination's matched scores (a CPU float64 tensor, NaN = no match) -> numpy array"""
    p = host_ptr(matched, "matched", _D)
    out = np.zeros(num_sample_pts, np.float64)
    count = ctypes.c_int(0)
    _lib.check(_lib.lib().epnet_kitti_thresholds_host(p, matched.numel(), int(num_gt), int(num_sample_pts),
                                                      out.ctypes.data_as(ctypes.c_void_p), num_sample_pts, ctypes.byref(count)),
               "kitti_thresholds_host")
    return out[:count.value].copy()

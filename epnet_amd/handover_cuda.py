"""Stand-in of an extension module the reference does not have: between its RPN heads and its proposal layer's NMS it runs
stock tensor ops (lib/utils/bbox_transform.py:25-262, lib/rpn/proposal_layer.py:23-35, lib/net/point_rcnn.py:44-52).
``decode_bbox_target_gpu`` is the one call of ``epnet_decode_bbox_target``, ``score_order_gpu`` of ``epnet_score_order`` and
``rpn_handover_gpu`` of ``epnet_rpn_handover`` (include/epnet_ops.h), on the tensors' device and current stream, nothing read
back; the workspace comes from the caching allocator.
"""
import ctypes

import torch

from . import _lib
from ._tensor import dev_ptr, need, on_device_of, opt_ptr, writes

_F = torch.float32


def _bins(scope, bin_size):
    """bins per axis as the reference's Python computes them (bbox_transform.py:42-43)"""
    return int(scope / bin_size) * 2


def _anchor3(anchor_size):
    """three host floats, copied by the library at the call"""
    if isinstance(anchor_size, torch.Tensor) and anchor_size.is_cuda:
        raise RuntimeError("anchor_size must be host numbers (a CPU tensor, an array or a sequence): the call copies them")
    values = [float(v) for v in (anchor_size.reshape(-1).tolist() if hasattr(anchor_size, "reshape") else anchor_size)]
    if len(values) != 3:
        raise RuntimeError("anchor_size must hold 3 numbers")
    return (ctypes.c_float * 3)(*values)


@writes("boxes")
def decode_bbox_target_gpu(anchors, pred_reg, loc_scope, loc_bin_size, num_head_bin, anchor_size, xz_fine, y_by_bin, loc_y_scope,
                           loc_y_bin_size, ry_fine, avg_by_bin, ry_with_bin, y_to_bottom, boxes):
    """anchors (R,3|7), pred_reg (R,C), anchor_size: 3 host numbers -> boxes (R,7) in one launch"""
    if anchors.dim() != 2 or pred_reg.dim() != 2 or anchors.shape[0] != pred_reg.shape[0]:
        raise RuntimeError("anchors must be (R, 3|7) and pred_reg (R, C)")
    rows, acols, c = anchors.shape[0], anchors.shape[1], pred_reg.shape[1]
    pa, pr, pb = dev_ptr(anchors, "anchors", _F), dev_ptr(pred_reg, "pred_reg", _F), dev_ptr(boxes, "boxes", _F)
    need(boxes, rows * 7, "boxes")
    size = _anchor3(anchor_size)
    with on_device_of(pred_reg) as s:
        _lib.check(_lib.lib().epnet_decode_bbox_target(rows, acols, pa, pr, c, _bins(loc_scope, loc_bin_size),
                                                       _bins(loc_y_scope, loc_y_bin_size), float(loc_scope), float(loc_bin_size),
                                                       float(loc_y_scope), float(loc_y_bin_size), int(num_head_bin),
                                                       ctypes.cast(size, ctypes.c_void_p), int(bool(xz_fine)), int(bool(y_by_bin)),
                                                       int(bool(ry_fine)), int(bool(avg_by_bin)), int(bool(ry_with_bin)),
                                                       int(bool(y_to_bottom)), pb, s), "decode_bbox_target")
    return 1


@writes("order")
def score_order_gpu(scores, order):
    """scores (B,N) -> order (B,N) int64: per scene the stable descending order (equal scores in ascending index, a NaN first)"""
    if scores.dim() != 2:
        raise RuntimeError("scores must be (B, N)")
    b, n = scores.shape
    ps, po = dev_ptr(scores, "scores", _F), dev_ptr(order, "order", torch.int64)
    need(order, b * n, "order")
    with on_device_of(scores) as s:
        _lib.check(_lib.lib().epnet_score_order(b, n, ps, po, s), "score_order (1 <= N <= 16384, B <= 65535)")
    return 1


@writes("ret_bbox3d", "ret_scores", "ret_count", "seg_mask", "pts_depth", "proposals", "order")
def rpn_handover_gpu(scores, rpn_reg, xyz, loc_scope, loc_bin_size, num_head_bin, anchor_size, xz_fine, avg_by_bin, ry_with_bin,
                     score_thresh, distance_based, pre_nms_top_n, post_nms_top_n, nms_thresh, rotated, ret_bbox3d, ret_scores,
                     ret_count=None, seg_mask=None, pts_depth=None, proposals=None, order=None, y_by_bin=False, loc_y_scope=0.5,
                     loc_y_bin_size=0.25, ry_fine=False):
    """lib/net/point_rcnn.py:44-52 for the whole batch, no host sync: scores (B,N), rpn_reg (B,N,C), xyz (B,N,3) -> ret_bbox3d
    (B,post,7), ret_scores (B,post) and, where given, ret_count (B) int32, seg_mask (B,N), pts_depth (B,N), proposals (B,N,7),
    order (B,N) int64"""
    if scores.dim() != 2 or rpn_reg.dim() != 3 or tuple(rpn_reg.shape[:2]) != tuple(scores.shape):
        raise RuntimeError("scores must be (B, N) and rpn_reg (B, N, C)")
    if xyz.dim() != 3 or tuple(xyz.shape) != (scores.shape[0], scores.shape[1], 3):
        raise RuntimeError("xyz must be (B, N, 3)")
    b, n, c = rpn_reg.shape
    post = int(post_nms_top_n)
    ps, pr, px = dev_ptr(scores, "scores", _F), dev_ptr(rpn_reg, "rpn_reg", _F), dev_ptr(xyz, "xyz", _F)
    pb, pq = dev_ptr(ret_bbox3d, "ret_bbox3d", _F), dev_ptr(ret_scores, "ret_scores", _F)
    need(ret_bbox3d, b * post * 7, "ret_bbox3d"); need(ret_scores, b * post, "ret_scores")
    outs = [opt_ptr(ret_count, "ret_count", torch.int32, b), opt_ptr(seg_mask, "seg_mask", _F, b * n), opt_ptr(pts_depth, "pts_depth", _F, b * n),
            opt_ptr(proposals, "proposals", _F, b * n * 7), opt_ptr(order, "order", torch.int64, b * n)]
    size = _anchor3(anchor_size)
    l = _lib.lib()
    ws_bytes = l.epnet_rpn_handover_workspace_bytes(b, n, int(bool(distance_based)), int(pre_nms_top_n), post)
    ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=scores.device)
    with on_device_of(scores) as s:
        _lib.check(l.epnet_rpn_handover(b, n, c, ps, pr, px, _bins(loc_scope, loc_bin_size), _bins(loc_y_scope, loc_y_bin_size),
                                        float(loc_scope), float(loc_bin_size), float(loc_y_scope), float(loc_y_bin_size),
                                        int(num_head_bin), ctypes.cast(size, ctypes.c_void_p), int(bool(xz_fine)), int(bool(y_by_bin)),
                                        int(bool(ry_fine)), int(bool(avg_by_bin)), int(bool(ry_with_bin)), float(score_thresh),
                                        int(bool(distance_based)), int(pre_nms_top_n), post, float(nms_thresh), int(bool(rotated)),
                                        ws.data_ptr(), ws.numel(), pb, pq, *outs, s),
                   "rpn_handover (1 <= N <= 16384, B <= 32767)")
    return 1

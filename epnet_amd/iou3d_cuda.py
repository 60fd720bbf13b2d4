"""Stand-in for the reference's ``iou3d_cuda`` extension module (lib/utils/iou3d/src/iou3d.cpp:174-179).

``nms_gpu`` / ``nms_normal_gpu`` keep the reference contract -- boxes (N,5) on the GPU sorted by
descending score, ``keep`` a CPU int64 tensor that receives the kept positions, return value = their
count (iou3d.cpp:73-120) -- but mask AND greedy sweep run on the device; only the kept positions
(N*8 B instead of the reference's N*ceil(N/64)*8 B mask) cross PCIe. ``nms_device`` /
``nms_normal_device`` expose the all-device form for callers that do not need a host list.
"""
import ctypes

import torch

from . import _lib
from ._tensor import dev_ptr, host_ptr, need, on_device_of, opt_ptr, writes

_F = torch.float32


@writes("ans")
def _pairwise(fn_name, boxes_a, boxes_b, ans):
    pa, pb, po = dev_ptr(boxes_a, "boxes_a", _F), dev_ptr(boxes_b, "boxes_b", _F), dev_ptr(ans, "ans", _F)
    na, nb = boxes_a.size(0), boxes_b.size(0)
    need(boxes_a, na * 5, "boxes_a"); need(boxes_b, nb * 5, "boxes_b"); need(ans, na * nb, "ans")
    with on_device_of(boxes_a) as s:
        _lib.check(getattr(_lib.lib(), fn_name)(na, pa, nb, pb, po, s), fn_name)
    return 1


def boxes_overlap_bev_gpu(boxes_a, boxes_b, ans_overlap):
    """iou3d.cpp:31-50"""
    return _pairwise("epnet_boxes_overlap_bev", boxes_a, boxes_b, ans_overlap)


def boxes_iou_bev_gpu(boxes_a, boxes_b, ans_iou):
    """iou3d.cpp:52-71"""
    return _pairwise("epnet_boxes_iou_bev", boxes_a, boxes_b, ans_iou)


@writes("ans_iou3d")
def boxes_iou3d_fused_gpu(boxes_a, boxes_b, ans_iou3d):
    """(N,7) x (M,7) -> (N,M) 3-D IoU in one launch (not in the reference extension; see epnet_ops.h)"""
    pa, pb, po = dev_ptr(boxes_a, "boxes_a", _F), dev_ptr(boxes_b, "boxes_b", _F), dev_ptr(ans_iou3d, "ans", _F)
    na, nb = boxes_a.size(0), boxes_b.size(0)
    need(boxes_a, na * 7, "boxes_a"); need(boxes_b, nb * 7, "boxes_b"); need(ans_iou3d, na * nb, "ans")
    with on_device_of(boxes_a) as s:
        _lib.check(_lib.lib().epnet_boxes_iou3d(na, pa, nb, pb, po, s), "boxes_iou3d")
    return 1


@writes("ans_iou3d")
def boxes_iou3d_pairs_gpu(boxes_a, boxes_b, ans_iou3d):
    """(K,7), (K,7) -> (K,) 3-D IoU of corresponding pairs in one launch"""
    pa, pb, po = dev_ptr(boxes_a, "boxes_a", _F), dev_ptr(boxes_b, "boxes_b", _F), dev_ptr(ans_iou3d, "ans", _F)
    k = boxes_a.size(0)
    need(boxes_a, k * 7, "boxes_a"); need(boxes_b, k * 7, "boxes_b"); need(ans_iou3d, k, "ans")
    with on_device_of(boxes_a) as s:
        _lib.check(_lib.lib().epnet_boxes_iou3d_pairs(k, pa, pb, po, s), "boxes_iou3d_pairs")
    return 1


@writes("roi_boxes3d", "iou_of_rois")
def aug_roi_by_noise_gpu(roi_boxes3d, gt_boxes3d, iou3d_src, keep_draw, noise, pos_thresh, iou_of_rois, tries=None):
    """the ROI augmentation loop of lib/rpn/proposal_target_layer.py:220-247 for all K ROIs in one launch; roi_boxes3d
    (K,7) is updated in place; keep_draw (K,T) uint8, noise (K,T,7), tries (K) int32 per-ROI try limits or None (not in
    the reference extension; see epnet_ops.h)"""
    k = roi_boxes3d.size(0)
    t = keep_draw.size(1) if keep_draw is not None else 0
    pr, pg = dev_ptr(roi_boxes3d, "roi_boxes3d", _F), dev_ptr(gt_boxes3d, "gt_boxes3d", _F)
    ps, po = dev_ptr(iou3d_src, "iou3d_src", _F), dev_ptr(iou_of_rois, "iou_of_rois", _F)
    need(roi_boxes3d, k * 7, "roi_boxes3d"); need(gt_boxes3d, k * 7, "gt_boxes3d"); need(iou3d_src, k, "iou3d_src")
    need(iou_of_rois, k, "iou_of_rois")
    pk = pn = pt = None
    if tries is not None:
        pt = dev_ptr(tries, "tries", torch.int32)
        need(tries, k, "tries")
    if t:
        pk, pn = dev_ptr(keep_draw, "keep_draw", torch.uint8), dev_ptr(noise, "noise", _F)
        need(keep_draw, k * t, "keep_draw"); need(noise, k * t * 7, "noise")
    with on_device_of(roi_boxes3d) as s:
        _lib.check(_lib.lib().epnet_aug_roi_by_noise(k, t, float(pos_thresh), pr, pg, ps, pt, pk, pn, po, s), "aug_roi_by_noise")
    return 1


def _overlap(a, b):
    """do the bytes of two tensors intersect"""
    if a.numel() == 0 or b.numel() == 0 or a.device != b.device:
        return False
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


@writes("batch_rois", "batch_gt_of_rois", "batch_roi_iou", "scene_info", "src_inds", "iou_src", "tries", "max_overlaps", "gt_assignment")
def rcnn_sample_rois_gpu(rois, gt_boxes3d, fg_key, slot_u, keep_draw, noise, fg_per_image, fg_thresh, cls_bg_thresh, cls_bg_thresh_lo,
                         hard_bg_ratio, batch_rois, batch_gt_of_rois, batch_roi_iou, scene_info, src_inds=None, iou_src=None, tries=None,
                         max_overlaps=None, gt_assignment=None):
    """lib/rpn/proposal_target_layer.py:85-218 (sample_rois_for_rcnn) for the whole batch, no host sync: rois (B,M,7),
    gt_boxes3d (B,G,gc) zero-padded, the draw tables fg_key (B,M) and slot_u (B,R), keep_draw (B*R,T) uint8 and noise (B*R,T,7)
    (both None for no noise loop) -> batch_rois (B,R,7), batch_gt_of_rois (B,R,7), batch_roi_iou (B,R), scene_info (B,6) int32
    and, where given, src_inds / tries (B,R) int32, iou_src (B,R), max_overlaps (B,M), gt_assignment (B,M) int32 (not in the
    reference extension; see epnet_ops.h)"""
    if rois.dim() != 3 or rois.shape[2] != 7:
        raise RuntimeError("rois must be (B, M, 7)")
    if gt_boxes3d.dim() != 3 or gt_boxes3d.shape[0] != rois.shape[0]:
        raise RuntimeError("gt_boxes3d must be (B, G, 7..16)")
    if fg_key.dim() != 2 or tuple(fg_key.shape) != (rois.shape[0], rois.shape[1]):
        raise RuntimeError("fg_key must be (B, M)")
    if slot_u.dim() != 2 or slot_u.shape[0] != rois.shape[0]:
        raise RuntimeError("slot_u must be (B, R)")
    b, m, g, gc, r = rois.shape[0], rois.shape[1], gt_boxes3d.shape[1], gt_boxes3d.shape[2], slot_u.shape[1]
    t = keep_draw.size(1) if keep_draw is not None else 0
    I = torch.int32
    pr, pg = dev_ptr(rois, "rois", _F), dev_ptr(gt_boxes3d, "gt_boxes3d", _F)
    pk, pu = dev_ptr(fg_key, "fg_key", _F), dev_ptr(slot_u, "slot_u", _F)
    need(fg_key, b * m, "fg_key"); need(slot_u, b * r, "slot_u")
    outs = [dev_ptr(batch_rois, "batch_rois", _F), dev_ptr(batch_gt_of_rois, "batch_gt_of_rois", _F),
            dev_ptr(batch_roi_iou, "batch_roi_iou", _F), dev_ptr(scene_info, "scene_info", I)]
    need(batch_rois, b * r * 7, "batch_rois"); need(batch_gt_of_rois, b * r * 7, "batch_gt_of_rois")
    need(batch_roi_iou, b * r, "batch_roi_iou"); need(scene_info, b * 6, "scene_info")
    for name, out, dtype, count in (("src_inds", src_inds, I, b * r), ("iou_src", iou_src, _F, b * r), ("tries", tries, I, b * r),
                                    ("max_overlaps", max_overlaps, _F, b * m), ("gt_assignment", gt_assignment, I, b * m)):
        if out is None:
            outs.append(None)
        else:
            outs.append(dev_ptr(out, name, dtype))
            need(out, count, name)
    pd = pn = None
    if t:
        pd, pn = dev_ptr(keep_draw, "keep_draw", torch.uint8), dev_ptr(noise, "noise", _F)
        need(keep_draw, b * r * t, "keep_draw"); need(noise, b * r * t * 7, "noise")
    # no output may alias an input (the selection reads whole scenes of every input while other slots are being written)
    given = (batch_rois, batch_gt_of_rois, batch_roi_iou, scene_info, src_inds, iou_src, tries, max_overlaps, gt_assignment)
    for out in given:
        for name, inp in (("rois", rois), ("gt_boxes3d", gt_boxes3d), ("fg_key", fg_key), ("slot_u", slot_u), ("keep_draw", keep_draw),
                          ("noise", noise)):
            if out is not None and inp is not None and _overlap(out, inp):
                raise RuntimeError("an output must not alias %s" % name)
    l = _lib.lib()
    ws_bytes = l.epnet_rcnn_sample_rois_workspace_bytes(b, m, g, r)
    ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=rois.device)
    with on_device_of(rois) as s:
        _lib.check(l.epnet_rcnn_sample_rois(b, m, g, gc, r, int(fg_per_image), float(fg_thresh), float(cls_bg_thresh),
                                            float(cls_bg_thresh_lo), float(hard_bg_ratio), t, pr, pg, pk, pu, pd, pn, ws.data_ptr(),
                                            ws.numel(), *outs, s), "rcnn_sample_rois")
    return 1


@writes("ret_bbox3d", "ret_scores", "ret_count")
def rpn_proposals_gpu(proposals, scores, order, distance_based, pre_nms_top_n, post_nms_top_n, nms_thresh, rotated,
                      ret_bbox3d, ret_scores, ret_count=None):
    """lib/rpn/proposal_layer.py:34-55 for the whole batch, no host sync: proposals (B,N,7), scores (B,N), order (B,N)
    int64 (descending scores) -> ret_bbox3d (B,post,7), ret_scores (B,post) (not in the reference extension; see
    epnet_ops.h)"""
    b, n = scores.size(0), scores.size(1)
    pp, ps, po = dev_ptr(proposals, "proposals", _F), dev_ptr(scores, "scores", _F), dev_ptr(order, "order", torch.int64)
    pb, pr = dev_ptr(ret_bbox3d, "ret_bbox3d", _F), dev_ptr(ret_scores, "ret_scores", _F)
    need(proposals, b * n * 7, "proposals"); need(order, b * n, "order")
    need(ret_bbox3d, b * post_nms_top_n * 7, "ret_bbox3d"); need(ret_scores, b * post_nms_top_n, "ret_scores")
    pc = None
    if ret_count is not None:
        pc = dev_ptr(ret_count, "ret_count", torch.int32)
        need(ret_count, b, "ret_count")
    l = _lib.lib()
    ws_bytes = l.epnet_rpn_proposals_workspace_bytes(b, int(bool(distance_based)), pre_nms_top_n, post_nms_top_n)
    ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=scores.device)
    with on_device_of(scores) as s:
        _lib.check(l.epnet_rpn_proposals(b, n, pp, ps, po, int(bool(distance_based)), pre_nms_top_n, post_nms_top_n,
                                         float(nms_thresh), int(bool(rotated)), ws.data_ptr(), ws.numel(), pb, pr, pc, s),
                   "rpn_proposals")
    return 1


@writes("det_boxes3d", "det_scores", "det_count")
def rcnn_detections_gpu(boxes3d, raw_scores, norm_scores, score_thresh, nms_thresh, det_boxes3d, det_scores, det_count):
    """tools/eval_rcnn.py:663-683 for the whole batch, no host sync: boxes3d (B,M,7), raw_scores / norm_scores (B,M) ->
    det_boxes3d (B,M,7), det_scores (B,M) (the kept boxes and their raw scores, zero rows behind), det_count (B) int32
    (not in the reference extension; see epnet_ops.h)"""
    b, m = raw_scores.size(0), raw_scores.size(1)
    pb, pr, pn = dev_ptr(boxes3d, "boxes3d", _F), dev_ptr(raw_scores, "raw_scores", _F), dev_ptr(norm_scores, "norm_scores", _F)
    ob, os_, oc = dev_ptr(det_boxes3d, "det_boxes3d", _F), dev_ptr(det_scores, "det_scores", _F), dev_ptr(det_count, "det_count", torch.int32)
    need(boxes3d, b * m * 7, "boxes3d"); need(norm_scores, b * m, "norm_scores")
    need(det_boxes3d, b * m * 7, "det_boxes3d"); need(det_scores, b * m, "det_scores"); need(det_count, b, "det_count")
    l = _lib.lib()
    ws_bytes = l.epnet_rcnn_detections_workspace_bytes(b, m)
    ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=raw_scores.device)
    with on_device_of(raw_scores) as s:
        _lib.check(l.epnet_rcnn_detections(b, m, pb, pr, pn, float(score_thresh), float(nms_thresh), ws.data_ptr(), ws.numel(),
                                           ob, os_, oc, s), "rcnn_detections")
    return 1


@writes("scene_stats", "seg_counts", "totals", "gt_max_pred", "gt_max_roi", "pred_max_iou")
def eval_recall_gpu(pred_boxes3d, roi_boxes3d, gt_boxes3d, thresholds, seg_result, rpn_cls_label, scene_stats, seg_counts=None,
                    totals=None, gt_max_pred=None, gt_max_roi=None, pred_max_iou=None):
    """tools/eval_rcnn.py:598-632 for the whole batch, no host sync: pred_boxes3d (B,M,7), roi_boxes3d (B,M,7) or None,
    gt_boxes3d (B,G,7..16) zero-padded, thresholds a sequence of at most 8 Python floats, seg_result / rpn_cls_label (B,N) int32
    or both None -> scene_stats (B, 1 + 2 T) int32 = [num_gt, recalled_refined[T], recalled_roi[T]], seg_counts (3) int64 =
    [correct, fg, pos] (None exactly when the segmentation inputs are) and, where given, totals (1 + 2 T) int64 (added to),
    gt_max_pred / gt_max_roi (B,G), pred_max_iou (B,M) (not in the reference extension; see epnet_ops.h)"""
    if pred_boxes3d.dim() != 3 or pred_boxes3d.shape[2] != 7:
        raise RuntimeError("pred_boxes3d must be (B, M, 7)")
    if gt_boxes3d.dim() != 3 or gt_boxes3d.shape[0] != pred_boxes3d.shape[0]:
        raise RuntimeError("gt_boxes3d must be (B, G, 7..16)")
    if (seg_result is None) != (rpn_cls_label is None) or (seg_result is None) != (seg_counts is None):
        raise RuntimeError("seg_result, rpn_cls_label and seg_counts are given together or not at all")
    b, m, g, gc = pred_boxes3d.shape[0], pred_boxes3d.shape[1], gt_boxes3d.shape[1], gt_boxes3d.shape[2]
    thr = [float(t) for t in thresholds]
    nt = len(thr)
    I, L = torch.int32, torch.int64
    pp = dev_ptr(pred_boxes3d, "pred_boxes3d", _F)
    pr = opt_ptr(roi_boxes3d, "roi_boxes3d", _F, b * m * 7)
    pg = dev_ptr(gt_boxes3d, "gt_boxes3d", _F)
    n = 0
    ps = pl = None
    if seg_result is not None:
        if seg_result.dim() != 2 or seg_result.shape[0] != b or seg_result.shape != rpn_cls_label.shape:
            raise RuntimeError("seg_result and rpn_cls_label must both be (B, N)")
        n = seg_result.shape[1]
        ps, pl = dev_ptr(seg_result, "seg_result", I), dev_ptr(rpn_cls_label, "rpn_cls_label", I)
    po = dev_ptr(scene_stats, "scene_stats", I)
    need(scene_stats, b * (1 + 2 * nt), "scene_stats")
    outs = [opt_ptr(seg_counts, "seg_counts", L, 3), opt_ptr(totals, "totals", L, 1 + 2 * nt), opt_ptr(gt_max_pred, "gt_max_pred", _F, b * g),
            opt_ptr(gt_max_roi, "gt_max_roi", _F, b * g), opt_ptr(pred_max_iou, "pred_max_iou", _F, b * m)]
    l = _lib.lib()
    ws_bytes = l.epnet_eval_recall_workspace_bytes(b, m, g)
    ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=pred_boxes3d.device)
    host_thr = (ctypes.c_float * max(nt, 1))(*thr)
    with on_device_of(pred_boxes3d) as s:
        _lib.check(l.epnet_eval_recall(b, m, g, gc, n, nt, ctypes.cast(host_thr, ctypes.c_void_p), pp, pr, pg, ps, pl, ws.data_ptr(),
                                       ws.numel(), po, *outs, s), "eval_recall")
    return 1


@writes("records", "rec_count", "bbox_raw", "valid")
def kitti_records_gpu(boxes3d, scores, count, P2, img_shape, records, rec_count, bbox_raw=None, valid=None):
    """save_kitti_format (tools/eval_rcnn.py:76-101) for the whole batch in one launch: boxes3d (B,M,7), scores (B,M), count (B)
    int32 or None (all M rows), P2 (B,3,4), img_shape (B,2) int32 [h, w] -> records (B,M,13) float64 (the valid rows, compacted,
    zero rows behind), rec_count (B) int32 and, where given, bbox_raw (B,M,4), valid (B,M) int32 (not in the reference
    extension; see epnet_ops.h)"""
    if boxes3d.dim() != 3 or boxes3d.shape[2] != 7:
        raise RuntimeError("boxes3d must be (B, M, 7)")
    b, m = boxes3d.shape[0], boxes3d.shape[1]
    I = torch.int32
    pb, ps = dev_ptr(boxes3d, "boxes3d", _F), dev_ptr(scores, "scores", _F)
    need(scores, b * m, "scores")
    pc = opt_ptr(count, "count", I, b)
    pp, pi = dev_ptr(P2, "P2", _F), dev_ptr(img_shape, "img_shape", I)
    need(P2, b * 12, "P2"); need(img_shape, b * 2, "img_shape")
    pr, pn = dev_ptr(records, "records", torch.float64), dev_ptr(rec_count, "rec_count", I)
    need(records, b * m * 13, "records"); need(rec_count, b, "rec_count")
    px, pv = opt_ptr(bbox_raw, "bbox_raw", _F, b * m * 4), opt_ptr(valid, "valid", I, b * m)
    with on_device_of(boxes3d) as s:
        _lib.check(_lib.lib().epnet_kitti_records(b, m, pb, ps, pc, pp, pi, pr, pn, px, pv, s), "kitti_records")
    return 1


def _nms_device(fn_name, boxes, thresh):
    """returns (keep_dev int64 (N,), num_keep_dev int32 (1,)), both on the boxes' device, no sync"""
    pb = dev_ptr(boxes, "boxes", _F)
    n = boxes.size(0)
    need(boxes, n * 5, "boxes")
    l = _lib.lib()
    ws_bytes = l.epnet_nms_workspace_bytes(n)
    ws = torch.empty((max(ws_bytes, 8),), dtype=torch.uint8, device=boxes.device)
    keep = torch.empty((max(n, 1),), dtype=torch.int64, device=boxes.device)
    num = torch.empty((1,), dtype=torch.int32, device=boxes.device)
    with on_device_of(boxes) as s:
        _lib.check(getattr(l, fn_name)(pb, n, float(thresh), ws.data_ptr(), ws.numel(), keep.data_ptr(),
                                       num.data_ptr(), s), fn_name)
    return keep, num


def nms_device(boxes, thresh):
    return _nms_device("epnet_nms", boxes, thresh)


def nms_normal_device(boxes, thresh):
    return _nms_device("epnet_nms_normal", boxes, thresh)


def _nms_host_contract(fn_name, boxes, keep, thresh):
    host_ptr(keep, "keep", torch.int64)
    need(keep, boxes.size(0), "keep")
    keep_dev, num = _nms_device(fn_name, boxes, thresh)
    n = int(num.item())  # the one unavoidable sync: the output length is data dependent
    keep[:n].copy_(keep_dev[:n])
    return n


def nms_gpu(boxes, keep, nms_overlap_thresh):
    """iou3d.cpp:73-120"""
    return _nms_host_contract("epnet_nms", boxes, keep, nms_overlap_thresh)


def nms_normal_gpu(boxes, keep, nms_overlap_thresh):
    """iou3d.cpp:123-170"""
    return _nms_host_contract("epnet_nms_normal", boxes, keep, nms_overlap_thresh)

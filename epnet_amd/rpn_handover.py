"""From the RPN heads to the ROIs in one call (reference: lib/net/point_rcnn.py:44-52 over lib/rpn/proposal_layer.py:23-55
and lib/utils/bbox_transform.py:25-262).

The reference -- and ``ProposalLayer.forward`` by default -- decodes the boxes with about thirty small tensor kernels, moves y
to the bottom centre, sorts the scores (tie order unspecified) and forms ``seg_mask`` and ``pts_depth`` with three more stock
ops before the proposal kernels start. Here that is ``epnet_rpn_handover`` (csrc/handover.hip): one launch decodes and writes the
mask and the depths, one launch orders the scores of every scene (stable: equal scores in ascending index), and the proposal
layer's bin / NMS / emit kernels follow unchanged. ``decode_boxes`` and ``score_order`` are the two new kernels on their own;
``decode_boxes`` also serves the second stage (``DetectionLayer(fused_decode=True)``). Nothing is read back to the host, so every
call records into a HIP graph. Opt-in: ``ProposalLayer(mode, fused_head=True)`` and ``compat.install_callers(fused_head=True)``.
"""
from collections import namedtuple

import numpy as np
import torch

from . import handover_cuda
from .proposal_layer import _ambient_cfg
from ._tensor import as_f32, f32_region

RpnHandover = namedtuple("RpnHandover", ["rois", "roi_scores_raw", "seg_mask", "pts_depth", "roi_count", "proposals", "order"])

MAX_POINTS = 16384     # epnet_score_order keeps a scene's keys on the chip


def decode_boxes(roi_box3d, pred_reg, loc_scope, loc_bin_size, num_head_bin, anchor_size, get_xz_fine=True, get_y_by_bin=False,
                 loc_y_scope=0.5, loc_y_bin_size=0.25, get_ry_fine=False, bbox_avg_by_bin=True, ry_with_bin=False, y_to_bottom=False):
    """``bbox_transform.decode_bbox_target`` in one launch: roi_box3d (R,3|7), pred_reg (R,C) -> boxes (R,7); anchor_size: three
    HOST numbers (a CPU tensor, an array or a sequence -- a device tensor would have to be read back). y_to_bottom adds h / 2 to
    y (lib/rpn/proposal_layer.py:31)"""
    boxes = torch.empty((pred_reg.shape[0], 7), dtype=torch.float32, device=pred_reg.device)
    handover_cuda.decode_bbox_target_gpu(roi_box3d.float().contiguous(), pred_reg.float().contiguous(), loc_scope, loc_bin_size,
                                         num_head_bin, anchor_size, get_xz_fine, get_y_by_bin, loc_y_scope, loc_y_bin_size,
                                         get_ry_fine, bbox_avg_by_bin, ry_with_bin, y_to_bottom, boxes)
    return boxes


def score_order(scores):
    """scores (B,N) -> (B,N) int64: ``torch.sort(scores, dim=1, descending=True, stable=True)[1]`` in one launch, at most 16384
    scores per scene"""
    order = torch.empty(scores.shape, dtype=torch.int64, device=scores.device)
    handover_cuda.score_order_gpu(scores.float().contiguous(), order)
    return order


def _mode_cfg(cfg, mode):
    return cfg[mode] if isinstance(cfg, dict) else getattr(cfg, mode)


def handover_args(cfg, mode):
    """the keys ProposalLayer reads (lib/rpn/proposal_layer.py:23-30, :35-55), as rpn_handover_gpu's keyword arguments"""
    m = _mode_cfg(cfg, mode)
    distance_based = bool(cfg.TEST.RPN_DISTANCE_BASED_PROPOSE)                            # :45 reads cfg.TEST's switch in both modes
    if distance_based:
        if cfg.RPN.NMS_TYPE not in ('rotate', 'normal'):
            raise NotImplementedError                                                     # :104-109
        rotated = cfg.RPN.NMS_TYPE == 'rotate'
    else:
        rotated = True                                                                    # score_based_proposal: nms_gpu (:137)
    return dict(loc_scope=cfg.RPN.LOC_SCOPE, loc_bin_size=cfg.RPN.LOC_BIN_SIZE, num_head_bin=cfg.RPN.NUM_HEAD_BIN,
                anchor_size=np.asarray(cfg.CLS_MEAN_SIZE[0], dtype=np.float32), xz_fine=cfg.RPN.LOC_XZ_FINE,
                avg_by_bin=cfg.TRAIN.BBOX_AVG_BY_BIN, ry_with_bin=cfg.TEST.RY_WITH_BIN,
                score_thresh=getattr(cfg.RPN, "SCORE_THRESH", 0.3), distance_based=distance_based,
                pre_nms_top_n=m.RPN_PRE_NMS_TOP_N, post_nms_top_n=m.RPN_POST_NMS_TOP_N, nms_thresh=m.RPN_NMS_THRESH, rotated=rotated)


@f32_region
def rpn_handover(rpn_cls, rpn_reg, backbone_xyz, cfg=None, mode='TRAIN'):
    """rpn_cls (B,N,1) or (B,N), rpn_reg (B,N,C), backbone_xyz (B,N,3) -> RpnHandover(rois (B,M,7), roi_scores_raw (B,M), seg_mask
    (B,N), pts_depth (B,N), roi_count (B) int32, proposals (B,N,7), order (B,N) int64), M = the mode's RPN_POST_NMS_TOP_N: what
    point_rcnn.py:44-52 hands to the RCNN stage, plus the decoded boxes and the order they were proposed in"""
    cfg = cfg if cfg is not None else _ambient_cfg()
    rpn_cls, rpn_reg = as_f32(rpn_cls), as_f32(rpn_reg)   # bf16 / fp16 heads: upcast once here
    scores = (rpn_cls[:, :, 0] if rpn_cls.dim() == 3 else rpn_cls).float().contiguous()   # :45
    b, n = scores.shape
    if n > MAX_POINTS:
        from ._lib import EpnetError
        raise EpnetError("rpn_handover: %d points per scene, epnet_score_order takes at most %d" % (n, MAX_POINTS))
    args = handover_args(cfg, mode)
    dev, post = scores.device, args["post_nms_top_n"]
    out = RpnHandover(torch.empty((b, post, 7), dtype=torch.float32, device=dev), torch.empty((b, post), dtype=torch.float32, device=dev),
                      torch.empty((b, n), dtype=torch.float32, device=dev), torch.empty((b, n), dtype=torch.float32, device=dev),
                      torch.empty((b,), dtype=torch.int32, device=dev), torch.empty((b, n, 7), dtype=torch.float32, device=dev),
                      torch.empty((b, n), dtype=torch.int64, device=dev))
    handover_cuda.rpn_handover_gpu(scores, rpn_reg.float().contiguous(), backbone_xyz.float().contiguous(), ret_bbox3d=out.rois,
                                   ret_scores=out.roi_scores_raw, ret_count=out.roi_count, seg_mask=out.seg_mask,
                                   pts_depth=out.pts_depth, proposals=out.proposals, order=out.order, **args)
    return out

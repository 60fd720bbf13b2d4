"""Second-stage inference (reference: the eval branch of RCNNNet.forward, lib/net/rcnn_net.py:138-164, and the end of
eval_one_epoch_joint, tools/eval_rcnn.py:555-583 + :663-683) with its per-scene host work moved onto the device.

The reference pools 100 ROIs per scene into a zero-filled tensor, subtracts the ROI centres in a second pass and rotates
scene by scene in a Python loop (cos, sin, three ``cat``, an indexed read, a batched matmul, an indexed write -- per scene);
behind the network it thresholds the scores and walks the scenes again: ``inds[k].sum() == 0`` (a sync), boolean-mask
indexing (a sync), a sort, an NMS whose mask goes to the host, more indexing, ``.cpu()``. Here ``pool_rois`` is the input
``cat`` + one launch of ``epnet_roipool3d_canonical`` (csrc/roipool3d.hip) and ``DetectionLayer`` is the decoding (stock tensor
ops, or with ``fused_decode=True`` one launch of ``epnet_decode_bbox_target``, csrc/handover.hip), a sigmoid
and ``epnet_rcnn_detections`` (csrc/detections.hip: select, batched rotated NMS with device-side counts, emit). Nothing is read
back to the host, so the whole second stage can sit inside a captured HIP graph; the results are padded to M rows per scene
with a device-side count instead of ragged host arrays.
"""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

from . import iou3d_cuda
from . import roipool3d_utils
from .bbox_transform import decode_bbox_target
from ._tensor import as_f32, f32_region


def default_cfg():
    """the keys these layers read, values of tools/cfgs/LI_Fusion_with_attention_use_ce_loss.yaml (:19, :21, :91-106, :115,
    :140-141, and :180-181, :191-192, which the reference's decode_bbox_target reads from the global config); any object
    with the same attributes works (e.g. the reference's lib.config.cfg)"""
    rcnn = SimpleNamespace(LOC_SCOPE=1.5, LOC_BIN_SIZE=0.5, NUM_HEAD_BIN=9, LOC_Y_BY_BIN=False, LOC_Y_SCOPE=0.5,
                           LOC_Y_BIN_SIZE=0.25, SIZE_RES_ON_ROI=False, SCORE_THRESH=0.2, NMS_THRESH=0.1, POOL_EXTRA_WIDTH=0.2,
                           NUM_POINTS=512, USE_MASK=True, USE_DEPTH=True, USE_INTENSITY=False)
    return SimpleNamespace(CLS_MEAN_SIZE=np.array([[1.52563191462, 1.62856739989, 3.88311640418]], dtype=np.float32),
                           USE_IOU_BRANCH=False, RCNN=rcnn, TRAIN=SimpleNamespace(BBOX_AVG_BY_BIN=True, RY_WITH_BIN=False),
                           TEST=SimpleNamespace(BBOX_AVG_BY_BIN=True, RY_WITH_BIN=False))


def _ambient_cfg():
    """the reference's global config when its module is loaded in this process (drop-in use under lib/net/*), else the
    yaml-valued defaults above"""
    import sys
    ref = sys.modules.get("lib.config")
    return ref.cfg if ref is not None and hasattr(ref, "cfg") else default_cfg()


@f32_region
def pool_rois(rpn_xyz, rpn_features, roi_boxes3d, seg_mask, pts_depth=None, rpn_intensity=None, cfg=None):
    """lib/net/rcnn_net.py:138-164: rpn_xyz (B,N,3), rpn_features (B,N,C), roi_boxes3d (B,M,7), seg_mask (B,N), pts_depth
    (B,N) with RCNN.USE_DEPTH, rpn_intensity (B,N) with RCNN.USE_INTENSITY -> pts_input (B*M, S, 3 + extra + C) in each ROI's
    own frame and pooled_empty_flag (B,M) int32. The extra-input columns come in the reference's order: intensity, mask,
    depth."""
    cfg = cfg if cfg is not None else _ambient_cfg()
    rpn_features = as_f32(rpn_features)   # bf16 / fp16 backbone output: upcast once here
    if cfg.RCNN.USE_INTENSITY:
        extra = [rpn_intensity.unsqueeze(dim=2), seg_mask.unsqueeze(dim=2)]              # :140-142
    else:
        extra = [seg_mask.unsqueeze(dim=2)]                                              # :144
    if cfg.RCNN.USE_DEPTH:
        # :146-148. Divided by a tensor, not by the Python scalar: torch's GPU kernels turn a division by a scalar into a
        # multiplication by its reciprocal (1 ulp off the quotient now and then), a tensor divisor is divided by -- the same
        # values on either device
        extra.append((pts_depth / torch.full_like(pts_depth, 70.0) - 0.5).unsqueeze(dim=2))
    pts_feature = torch.cat(extra + [rpn_features], dim=2)                               # :149-151
    pooled, empty = roipool3d_utils.roipool3d_canonical_gpu(rpn_xyz, pts_feature.float(), roi_boxes3d, cfg.RCNN.POOL_EXTRA_WIDTH,
                                                            sampled_pt_num=cfg.RCNN.NUM_POINTS)  # :152-162
    return pooled.view(-1, pooled.shape[2], pooled.shape[3]), empty                      # :164


class DetectionLayer(nn.Module):
    def __init__(self, cfg=None, fused_decode=False):
        super().__init__()
        self.cfg = cfg if cfg is not None else _ambient_cfg()
        self.fused_decode = bool(fused_decode)
        self.register_buffer("MEAN_SIZE", torch.from_numpy(np.asarray(self.cfg.CLS_MEAN_SIZE[0], dtype=np.float32)), persistent=False)

    @f32_region
    def forward(self, rois, rcnn_cls, rcnn_reg, rcnn_iou_branch=None):
        """rois (B,M,7), rcnn_cls (B*M,1), rcnn_reg (B*M,C), rcnn_iou_branch (B*M,1) with USE_IOU_BRANCH -> pred_boxes3d
        (B,M,7), raw_scores (B,M), norm_scores (B,M), det_boxes3d (B,M,7), det_scores (B,M), det_count (B) int32: the
        detections of scene k are det_boxes3d[k, :det_count[k]], highest raw score first, zero rows behind"""
        rcnn = self.cfg.RCNN
        batch_size = rois.shape[0]
        rcnn_cls, rcnn_reg, rcnn_iou_branch = as_f32(rcnn_cls), as_f32(rcnn_reg), as_f32(rcnn_iou_branch)   # bf16 / fp16 heads
        rcnn_cls = rcnn_cls.view(batch_size, -1, rcnn_cls.shape[1])                      # :555
        rcnn_reg = rcnn_reg.view(batch_size, -1, rcnn_reg.shape[1])                      # :556
        if rcnn_iou_branch is not None:                                                  # :558-561
            iou = rcnn_iou_branch.view(batch_size, -1, rcnn_iou_branch.shape[1])
            rcnn_cls = torch.clamp(iou, min=1e-4) * rcnn_cls
        if rcnn.SIZE_RES_ON_ROI:
            raise NotImplementedError("RCNN.SIZE_RES_ON_ROI (the reference asserts False, tools/eval_rcnn.py:565-566)")
        if rcnn_cls.shape[2] != 1:
            raise NotImplementedError("a class head wider than 1 (tools/eval_rcnn.py:584-587)")
        if self.fused_decode:
            from .rpn_handover import decode_boxes
            decode, anchor_size = decode_boxes, np.asarray(self.cfg.CLS_MEAN_SIZE[0], dtype=np.float32)   # host numbers: no read-back
        else:
            decode, anchor_size = decode_bbox_target, self.MEAN_SIZE
        pred_boxes3d = decode(rois.reshape(-1, 7), rcnn_reg.reshape(-1, rcnn_reg.shape[-1]), anchor_size=anchor_size,
                              loc_scope=rcnn.LOC_SCOPE, loc_bin_size=rcnn.LOC_BIN_SIZE, num_head_bin=rcnn.NUM_HEAD_BIN,
                              get_xz_fine=True, get_y_by_bin=rcnn.LOC_Y_BY_BIN, loc_y_scope=rcnn.LOC_Y_SCOPE,
                              loc_y_bin_size=rcnn.LOC_Y_BIN_SIZE, get_ry_fine=True, bbox_avg_by_bin=self.cfg.TRAIN.BBOX_AVG_BY_BIN,
                              ry_with_bin=self.cfg.TEST.RY_WITH_BIN).view(batch_size, -1, 7)  # :568-575
        raw_scores = rcnn_cls[:, :, 0].float().contiguous()                              # :579
        norm_scores = torch.sigmoid(raw_scores)                                          # :581
        pred_boxes3d = pred_boxes3d.float().contiguous()
        m = raw_scores.shape[1]
        det_boxes3d = torch.empty((batch_size, m, 7), dtype=torch.float32, device=rois.device)
        det_scores = torch.empty((batch_size, m), dtype=torch.float32, device=rois.device)
        det_count = torch.empty((batch_size,), dtype=torch.int32, device=rois.device)
        iou3d_cuda.rcnn_detections_gpu(pred_boxes3d, raw_scores, norm_scores, rcnn.SCORE_THRESH, rcnn.NMS_THRESH, det_boxes3d,
                                       det_scores, det_count)                            # :663-683
        return pred_boxes3d, raw_scores, norm_scores, det_boxes3d, det_scores, det_count

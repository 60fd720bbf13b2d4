"""The RPN training targets on the device, with no host synchronisation (reference: the loader path get_rpn_with_li_fusion,
lib/datasets/kitti_rcnn_dataset.py:378-408, which calls data_augmentation :698-755 and generate_rpn_training_labels :547-576
per scene on a host core, two scipy Delaunay point-in-hull tests per box over all points).

The loader hands over ``pts_rect (B,N,3)``, ``gt_boxes3d (B,G,7)`` zero-padded as ``collate_batch`` pads them and
``gt_alpha (B,G)``; ``draw_augmentation`` draws the per-scene table on the device by the reference's rules, and
``augment_and_label`` is ONE launch of ``epnet_rpn_targets`` (csrc/targets.hip) for the whole batch: augmented points and
boxes, ``rpn_cls_label`` and ``rpn_reg_label`` as ``loss_utils.rpn_loss`` takes them. Nothing is read back, so the step can be
queued behind the previous one or captured into a HIP graph together with the loss.
"""
import math
from types import SimpleNamespace

import torch

from . import pointnet2_utils
from . import rpn_target_cuda


def default_cfg():
    """the keys draw_augmentation reads, values of tools/cfgs/LI_Fusion_with_attention_use_ce_loss.yaml (:7-9); any object
    with the same attributes works (e.g. the reference's lib.config.cfg)"""
    return SimpleNamespace(AUG_METHOD_LIST=["rotation", "scaling", "flip"], AUG_METHOD_PROB=[1.0, 1.0, 0.5], AUG_ROT_RANGE=18)


def _ambient_cfg():
    """the reference's global config when its module is loaded in this process, else the yaml-valued defaults above"""
    import sys
    ref = sys.modules.get("lib.config")
    return ref.cfg if ref is not None and hasattr(ref, "cfg") else default_cfg()


def draw_augmentation(batch, cfg=None, generator=None, device="cuda"):
    """the draws of data_augmentation (:705-734) for `batch` scenes -> (batch,4) fp32 [rotate 0/1, angle, scale, flip 0/1] on
    the device: ``aug_enable = 1 - rand(3)`` against AUG_METHOD_PROB, a method absent from AUG_METHOD_LIST is off, the angle
    uniform in +-pi / AUG_ROT_RANGE, the scale uniform in 0.95 - 1.05 (angle 0 and scale 1 where the method is off). Drawn
    with torch on the device, nothing read back; the draws differ from numpy's stream, the rules do not."""
    cfg = cfg if cfg is not None else _ambient_cfg()
    u = torch.rand((batch, 5), generator=generator, device=device, dtype=torch.float32)
    enable = 1.0 - u[:, 0:3]
    on = [(enable[:, k] < float(cfg.AUG_METHOD_PROB[k])) if name in cfg.AUG_METHOD_LIST else torch.zeros_like(enable[:, k], dtype=torch.bool)
          for k, name in enumerate(("rotation", "scaling", "flip"))]
    bound = math.pi / cfg.AUG_ROT_RANGE
    angle = (u[:, 3] * 2.0 - 1.0) * bound
    scale = (0.95 + 0.1 * u[:, 4]).clamp(0.95, 1.05)
    zero, one = torch.zeros_like(angle), torch.ones_like(angle)
    return torch.stack([on[0].float(), torch.where(on[0], angle, zero), torch.where(on[1], scale, one), on[2].float()], dim=1).contiguous()


def _inputs(pts_rect, gt_boxes3d):
    for name, t in (("pts_rect", pts_rect), ("gt_boxes3d", gt_boxes3d)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError("%s must be a CUDAtensor (epnet_amd has no CPU fallback)" % name)
    if pts_rect.dim() != 3 or pts_rect.shape[2] != 3:
        raise RuntimeError("pts_rect must be (B, N, 3)")
    if gt_boxes3d.dim() != 3 or gt_boxes3d.shape[2] != 7 or gt_boxes3d.shape[0] != pts_rect.shape[0]:
        raise RuntimeError("gt_boxes3d must be (B, G, 7)")
    return pts_rect.float().contiguous(), gt_boxes3d.float().contiguous()


def _labels_like(pts, dtype, cls_label):
    if dtype == torch.int32:
        return cls_label
    if dtype == torch.int64:
        return cls_label.long()
    raise RuntimeError("cls_label is int32 (what rpn_loss takes without a copy) or int64 (the reference's .long())")


def rpn_training_labels(pts_rect, gt_boxes3d, extra_width=0.2, dtype=torch.int32):
    """generate_rpn_training_labels (:547-576) for a batch: pts_rect (B,N,3), gt_boxes3d (B,G,7) zero-padded ->
    cls_label (B,N) in {-1, 0, 1}, reg_label (B,N,7) [centre - point, h, w, l, ry]; the last box decides, as in the
    reference's loop (include/epnet_ops.h)"""
    pts, gt = _inputs(pts_rect, gt_boxes3d)
    b, n = pts.shape[0], pts.shape[1]
    new = pointnet2_utils._new
    cls_label, reg_label = new(pts, (b, n), torch.int32), new(pts, (b, n, 7))
    rpn_target_cuda.rpn_targets_gpu(pts, gt, None, None, extra_width, None, None, cls_label, reg_label)
    return _labels_like(pts, dtype, cls_label), reg_label


def augment_and_label(pts_rect, gt_boxes3d, gt_alpha, aug, extra_width=0.2, dtype=torch.int32):
    """data_augmentation (:698-755, stage 1) with the draws of `aug` (B,4) (draw_augmentation) and then
    generate_rpn_training_labels on the augmented values, in one launch: -> aug_pts (B,N,3), aug_gt_boxes3d (B,G,7),
    cls_label (B,N), reg_label (B,N,7). gt_alpha (B,G) is zero where gt_boxes3d is padding. The LI-Fusion image coordinates
    are not touched by the reference's augmentation and are not touched here."""
    pts, gt = _inputs(pts_rect, gt_boxes3d)
    if not isinstance(gt_alpha, torch.Tensor) or not gt_alpha.is_cuda or not isinstance(aug, torch.Tensor) or not aug.is_cuda:
        raise RuntimeError("gt_alpha and aug must be CUDAtensors (epnet_amd has no CPU fallback)")
    b, n, g = pts.shape[0], pts.shape[1], gt.shape[1]
    if tuple(gt_alpha.shape) != (b, g) or tuple(aug.shape) != (b, 4):
        raise RuntimeError("gt_alpha must be (B, G) and aug (B, 4)")
    new = pointnet2_utils._new
    pts_out, gt_out = new(pts, (b, n, 3)), new(pts, (b, g, 7))
    cls_label, reg_label = new(pts, (b, n), torch.int32), new(pts, (b, n, 7))
    rpn_target_cuda.rpn_targets_gpu(pts, gt, gt_alpha.float().contiguous(), aug.float().contiguous(), extra_width, pts_out, gt_out,
                                    cls_label, reg_label)
    return pts_out, gt_out, _labels_like(pts, dtype, cls_label), reg_label

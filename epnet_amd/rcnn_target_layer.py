"""The RCNN training targets on the device, with no host synchronisation (reference: lib/rpn/proposal_target_layer.py:16-349,
ProposalTargetLayer.forward with sample_rois_for_rcnn :85-218 and data_augmentation :292-349).

``proposal_target_layer.ProposalTargetLayer`` restates the reference's host random streams draw for draw and therefore reads
the overlaps back and samples on the host. This module is the sync-free form of the same layer: every random decision comes
from a table drawn on the device (``draw_sampling_tables``), ``sample_rois`` is ONE call of ``epnet_rcnn_sample_rois``
(csrc/rcnn_targets.hip: the IoU of all scenes, classes, selection, gather and the noise loop) and ``pool_targets`` ONE launch of
``epnet_roipool3d_train`` (csrc/roipool3d.hip: pooling, per-ROI augmentation, canonical transformation, labels). Nothing is read
back, so the whole ``rcnn_online`` step can be queued behind the previous one or captured into one HIP graph.

Random streams: the DISTRIBUTIONS are the reference's, the streams are not. The foreground subset is the ``fg_this`` smallest
of one uniform key per ROI (a uniform subset without replacement in uniform order -- ``np.random.permutation``'s
distribution), a background slot is ``floor(u * len)`` of one uniform draw (``torch.randint``'s distribution up to fp32
rounding of the product), the noise loop and the augmentation use the tables of ``proposal_target_layer``. The two cases the
reference cannot run are defined (include/epnet_ops.h): a scene without ground truth counts as one zero box (every ROI easy
background), a scene with neither foreground nor background ROIs takes uniformly drawn ROIs, which end up with class -1.
"""
import numpy as np
import torch
import torch.nn as nn

from . import iou3d_cuda, pointnet2_utils, roipool3d_cuda
from .proposal_target_layer import _ambient_cfg, default_cfg, draw_aug_tables  # noqa: F401  (default_cfg: part of the surface)
from ._tensor import as_f32, f32_region


def _thresholds(cfg):
    rcnn = cfg.RCNN
    per_image = int(rcnn.ROI_PER_IMAGE)
    return per_image, int(np.round(rcnn.FG_RATIO * per_image)), min(rcnn.REG_FG_THRESH, rcnn.CLS_FG_THRESH)


def draw_sampling_tables(batch, num_roi, cfg=None, device="cuda", generator=None):
    """every random draw of one forward pass, on `device`, nothing read back -> dict:
    fg_key (B,M) and slot_u (B,R) uniform [0,1) for the selection; keep_draw (B*R,T) uint8 and noise (B*R,T,7) for the noise
    loop (``draw_aug_tables``; None with ROI_FG_AUG_TIMES == 0); aug (B,R,3) = [angle, scale, flip] by data_augmentation's
    expressions (:300-337, the reference's ``- 0.5 / 0.5`` included: the angle is (u - 1) * pi / AUG_ROT_RANGE), None with
    AUG_DATA False. REG_AUG_METHOD 'normal' raises NotImplementedError, as in proposal_target_layer."""
    cfg = cfg if cfg is not None else _ambient_cfg()
    per_image = int(cfg.RCNN.ROI_PER_IMAGE)
    aug_times = int(cfg.RCNN.ROI_FG_AUG_TIMES)
    tables = {"fg_key": torch.rand((batch, num_roi), device=device, generator=generator),
              "slot_u": torch.rand((batch, per_image), device=device, generator=generator), "keep_draw": None, "noise": None, "aug": None}
    if cfg.RCNN.REG_AUG_METHOD not in ("single", "multiple"):
        raise NotImplementedError("REG_AUG_METHOD %r" % (cfg.RCNN.REG_AUG_METHOD,))
    if aug_times > 0:
        tables["keep_draw"], tables["noise"] = draw_aug_tables(batch * per_image, aug_times, cfg.RCNN.REG_AUG_METHOD, device, generator)
    if cfg.AUG_DATA:
        rot_u, scale_u, flip_u = (torch.rand((batch, per_image), device=device, generator=generator) for _ in range(3))
        tables["aug"] = aug_table_from_draws(rot_u, scale_u, flip_u, cfg)
    return tables


def aug_table_from_draws(rot_u, scale_u, flip_u, cfg):
    """(B,R) uniform draws -> aug (B,R,3) = [angle, scale, flip] with data_augmentation's expressions (:302, :330, :336)"""
    angles = (rot_u - 0.5 / 0.5) * (np.pi / cfg.AUG_ROT_RANGE)
    scales = 1 + ((scale_u - 0.5) / 0.5) * 0.05
    flip = torch.sign(flip_u - 0.5)
    return torch.stack([angles, scales, flip], dim=2).float().contiguous()


def _cuda_f32(t, name, dims, last=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s must be a CUDAtensor (epnet_amd has no CPU fallback)" % name)
    if t.dim() != dims or (last is not None and t.shape[-1] != last):
        raise RuntimeError("%s has the wrong shape %s" % (name, tuple(t.shape)))
    return t.float().contiguous()


def sample_rois(roi_boxes3d, gt_boxes3d, tables, cfg=None, details=False):
    """sample_rois_for_rcnn (:85-218) for the batch in one call: roi_boxes3d (B,M,7), gt_boxes3d (B,G,7+) zero-padded, tables
    from draw_sampling_tables -> batch_rois (B,R,7), batch_gt_of_rois (B,R,7), batch_roi_iou (B,R), scene_info (B,6) int32 =
    [num_gt, fg_num, hard_num, easy_num, fg_this, case]; details=True adds a dict with src_inds, tries, iou_src, max_overlaps,
    gt_assignment"""
    cfg = cfg if cfg is not None else _ambient_cfg()
    rois = _cuda_f32(roi_boxes3d, "roi_boxes3d", 3, 7)
    gts = _cuda_f32(gt_boxes3d, "gt_boxes3d", 3)
    per_image, fg_per_image, fg_thresh = _thresholds(cfg)
    b, m = rois.shape[0], rois.shape[1]
    new, i32 = pointnet2_utils._new, torch.int32
    batch_rois, batch_gt, batch_iou = new(rois, (b, per_image, 7)), new(rois, (b, per_image, 7)), new(rois, (b, per_image))
    info = new(rois, (b, 6), i32)
    extra = {}
    if details:
        extra = {"src_inds": new(rois, (b, per_image), i32), "iou_src": new(rois, (b, per_image)), "tries": new(rois, (b, per_image), i32),
                 "max_overlaps": new(rois, (b, m)), "gt_assignment": new(rois, (b, m), i32)}
    keep, noise = tables.get("keep_draw"), tables.get("noise")
    if int(cfg.RCNN.ROI_FG_AUG_TIMES) <= 0:
        keep = noise = None
    iou3d_cuda.rcnn_sample_rois_gpu(rois, gts, tables["fg_key"], tables["slot_u"], keep, noise, fg_per_image, fg_thresh,
                                    cfg.RCNN.CLS_BG_THRESH, cfg.RCNN.CLS_BG_THRESH_LO, cfg.RCNN.HARD_BG_RATIO, batch_rois, batch_gt,
                                    batch_iou, info, **extra)
    if details:
        return batch_rois, batch_gt, batch_iou, info, extra
    return batch_rois, batch_gt, batch_iou, info


def pool_targets(rpn_xyz, pts_feature, batch_rois, batch_gt_of_rois, batch_roi_iou, aug, cfg=None):
    """the tail of forward (:36-83) in one launch: rpn_xyz (B,N,3), pts_feature (B,N,C), the sampled rows of sample_rois, aug
    (B,R,3) or None -> dict with sampled_pts (B*R,S,3), pts_feature (B*R,S,C), cls_label / reg_valid_mask (B*R) int32,
    mask_score (B*R), gt_of_rois / roi_boxes3d (B*R,7), pooled_empty_flag (B,R) int32"""
    cfg = cfg if cfg is not None else _ambient_cfg()
    xyz, feat = _cuda_f32(rpn_xyz, "rpn_xyz", 3, 3), _cuda_f32(pts_feature, "pts_feature", 3)
    rois, gts, iou = _cuda_f32(batch_rois, "batch_rois", 3, 7), _cuda_f32(batch_gt_of_rois, "batch_gt_of_rois", 3, 7), _cuda_f32(batch_roi_iou, "batch_roi_iou", 2)
    b, r, s, c = rois.shape[0], rois.shape[1], int(cfg.RCNN.NUM_POINTS), feat.shape[2]
    new, i32 = pointnet2_utils._new, torch.int32
    out = {"sampled_pts": new(xyz, (b * r, s, 3)), "pts_feature": new(xyz, (b * r, s, c)), "cls_label": new(xyz, (b * r,), i32),
           "mask_score": new(xyz, (b * r,)), "reg_valid_mask": new(xyz, (b * r,), i32), "gt_of_rois": new(xyz, (b * r, 7)),
           "roi_boxes3d": new(xyz, (b * r, 7)), "pooled_empty_flag": new(xyz, (b, r), i32)}
    roipool3d_cuda.forward_train(xyz, feat, rois, gts, iou, None if aug is None else aug.float().contiguous(), cfg.RCNN.POOL_EXTRA_WIDTH,
                                 cfg.RCNN.REG_FG_THRESH, cfg.RCNN.CLS_FG_THRESH, cfg.RCNN.CLS_BG_THRESH, out["sampled_pts"],
                                 out["pts_feature"], out["roi_boxes3d"], out["gt_of_rois"], out["cls_label"], out["reg_valid_mask"],
                                 out["mask_score"], out["pooled_empty_flag"])
    return out


class RCNNTargetLayer(nn.Module):
    """ProposalTargetLayer.forward without a host synchronisation: the same eight keys, shapes and meanings, plus scene_info.
    label_dtype: int32 (what rcnn_loss takes without a copy) or int64 (the reference's .long())"""

    def __init__(self, cfg=None, generator=None, label_dtype=torch.int32):
        super().__init__()
        if label_dtype not in (torch.int32, torch.int64):
            raise RuntimeError("label_dtype is int32 (what rcnn_loss takes without a copy) or int64 (the reference's .long())")
        self.cfg = cfg if cfg is not None else _ambient_cfg()
        self.generator = generator  # device generator for the tables (None: the default one)
        self.label_dtype = label_dtype

    @f32_region
    def forward(self, input_dict, tables=None):
        cfg = self.cfg
        roi_boxes3d, gt_boxes3d = as_f32(input_dict['roi_boxes3d']), input_dict['gt_boxes3d']
        if cfg.RCNN.REG_AUG_METHOD not in ("single", "multiple"):
            raise NotImplementedError("REG_AUG_METHOD %r" % (cfg.RCNN.REG_AUG_METHOD,))
        if tables is None:
            tables = draw_sampling_tables(roi_boxes3d.shape[0], roi_boxes3d.shape[1], cfg, roi_boxes3d.device, self.generator)
        batch_rois, batch_gt_of_rois, batch_roi_iou, scene_info = sample_rois(roi_boxes3d, gt_boxes3d, tables, cfg)

        rpn_xyz, rpn_features = input_dict['rpn_xyz'], as_f32(input_dict['rpn_features'])   # bf16 / fp16 backbone output: upcast once here
        if cfg.RCNN.USE_INTENSITY:
            extra = [input_dict['rpn_intensity'].unsqueeze(dim=2), input_dict['seg_mask'].unsqueeze(dim=2)]
        else:
            extra = [input_dict['seg_mask'].unsqueeze(dim=2)]
        if cfg.RCNN.USE_DEPTH:
            extra.append((input_dict['pts_depth'] / 70.0 - 0.5).unsqueeze(dim=2))
        if cfg.RCNN.USE_RGB:
            extra.append(input_dict['pts_rgb'])
        pts_feature = torch.cat(extra + [rpn_features], dim=2)

        out = pool_targets(rpn_xyz, pts_feature, batch_rois, batch_gt_of_rois, batch_roi_iou, tables.get("aug") if cfg.AUG_DATA else None, cfg)
        del out["pooled_empty_flag"]
        if self.label_dtype == torch.int64:
            out["cls_label"], out["reg_valid_mask"] = out["cls_label"].long(), out["reg_valid_mask"].long()
        out["gt_iou"] = batch_roi_iou.view(-1)
        out["scene_info"] = scene_info
        return out

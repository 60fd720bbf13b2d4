"""Stand-in for the reference's ``roipool3d_cuda`` extension module (lib/utils/roipool3d/src/roipool3d.cpp:198-203)."""
import torch

from . import _lib
from ._tensor import dev_ptr, host_ptr, need, on_device_of, writes

_F = torch.float32


@writes("pooled_features", "pooled_empty_flag")
def forward(xyz, boxes3d, pts_feature, pooled_features, pooled_empty_flag):
    """roipool3d_gpu, roipool3d.cpp:48-79 (S is read from pooled_features.size(2), :64)"""
    px, pb, pf = dev_ptr(xyz, "xyz", _F), dev_ptr(boxes3d, "boxes3d", _F), dev_ptr(pts_feature, "pts_feature", _F)
    po, pe = dev_ptr(pooled_features, "pooled_features", _F), dev_ptr(pooled_empty_flag, "pooled_empty_flag", torch.int32)
    b, n = xyz.size(0), xyz.size(1)
    m, c, s_num = boxes3d.size(1), pts_feature.size(2), pooled_features.size(2)
    need(xyz, b * n * 3, "xyz"); need(boxes3d, b * m * 7, "boxes3d"); need(pts_feature, b * n * c, "pts_feature")
    need(pooled_features, b * m * s_num * (3 + c), "pooled_features"); need(pooled_empty_flag, b * m, "pooled_empty_flag")
    with on_device_of(xyz) as s:
        _lib.check(_lib.lib().epnet_roipool3d(b, n, m, c, s_num, px, pb, pf, po, pe, None, 0, s), "roipool3d")
    return 1


@writes("pooled_features", "pooled_empty_flag")
def forward_canonical(xyz, rois, pts_feature, pool_extra_width, pooled_features, pooled_empty_flag):
    """roipool3d_gpu on the ROIs enlarged by pool_extra_width + the canonical transformation of lib/net/rcnn_net.py:151-164
    in one launch; every element of both outputs is written (not in the reference extension; see epnet_ops.h)"""
    px, pb, pf = dev_ptr(xyz, "xyz", _F), dev_ptr(rois, "rois", _F), dev_ptr(pts_feature, "pts_feature", _F)
    po, pe = dev_ptr(pooled_features, "pooled_features", _F), dev_ptr(pooled_empty_flag, "pooled_empty_flag", torch.int32)
    b, n = xyz.size(0), xyz.size(1)
    m, c, s_num = rois.size(1), pts_feature.size(2), pooled_features.size(2)
    need(xyz, b * n * 3, "xyz"); need(rois, b * m * 7, "rois"); need(pts_feature, b * n * c, "pts_feature")
    need(pooled_features, b * m * s_num * (3 + c), "pooled_features"); need(pooled_empty_flag, b * m, "pooled_empty_flag")
    with on_device_of(xyz) as s:
        _lib.check(_lib.lib().epnet_roipool3d_canonical(b, n, m, c, s_num, float(pool_extra_width), px, pb, pf, po, pe, s),
                   "roipool3d_canonical")
    return 1


@writes("sampled_pts", "pts_feature_out", "rois_out", "gt_out", "cls_label", "reg_valid_mask", "mask_score", "pooled_empty_flag")
def forward_train(xyz, pts_feature, rois, gt_of_rois, roi_iou, aug, pool_extra_width, reg_fg_thresh, cls_fg_thresh, cls_bg_thresh,
                  sampled_pts, pts_feature_out, rois_out, gt_out, cls_label, reg_valid_mask, mask_score, pooled_empty_flag):
    """the tail of ProposalTargetLayer.forward (lib/rpn/proposal_target_layer.py:16-83) in one launch: pooling on the enlarged
    ROIs, per-ROI data augmentation (aug (B,R,3) = [angle, scale, flip] or None), canonical transformation and labels; every
    element of every output is written (not in the reference extension; see epnet_ops.h)"""
    I = torch.int32
    px, pf, pb = dev_ptr(xyz, "xyz", _F), dev_ptr(pts_feature, "pts_feature", _F), dev_ptr(rois, "rois", _F)
    pg, pi = dev_ptr(gt_of_rois, "gt_of_rois", _F), dev_ptr(roi_iou, "roi_iou", _F)
    b, n = xyz.size(0), xyz.size(1)
    m, c, s_num = rois.size(1), pts_feature.size(2), sampled_pts.size(1)
    need(xyz, b * n * 3, "xyz"); need(rois, b * m * 7, "rois"); need(pts_feature, b * n * c, "pts_feature")
    need(gt_of_rois, b * m * 7, "gt_of_rois"); need(roi_iou, b * m, "roi_iou")
    pa = None
    if aug is not None:
        pa = dev_ptr(aug, "aug", _F)
        need(aug, b * m * 3, "aug")
    outs = []
    for name, out, dtype, count in (("sampled_pts", sampled_pts, _F, b * m * s_num * 3), ("pts_feature_out", pts_feature_out, _F, b * m * s_num * c),
                                    ("rois_out", rois_out, _F, b * m * 7), ("gt_out", gt_out, _F, b * m * 7), ("cls_label", cls_label, I, b * m),
                                    ("reg_valid_mask", reg_valid_mask, I, b * m), ("mask_score", mask_score, _F, b * m),
                                    ("pooled_empty_flag", pooled_empty_flag, I, b * m)):
        outs.append(dev_ptr(out, name, dtype))
        need(out, count, name)
    if b * m and (outs[2] == pb or outs[3] == pg):
        raise RuntimeError("rois_out / gt_out must not alias rois / gt_of_rois")
    with on_device_of(xyz) as s:
        _lib.check(_lib.lib().epnet_roipool3d_train(b, n, m, c, s_num, float(pool_extra_width), float(reg_fg_thresh), float(cls_fg_thresh),
                                                    float(cls_bg_thresh), px, pf, pb, pg, pi, pa, *outs, s), "roipool3d_train")
    return 1


# forward_slow (roipool3d.cpp:15-44) computes the same result with one thread per box; same entry here
forward_slow = forward


@writes("pts_flag")
def pts_in_boxes3d_cpu(pts_flag, pts, boxes3d):
    """roipool3d.cpp:97-125 -- a HOST op in the reference as well"""
    pf, pp, pb = host_ptr(pts_flag, "pts_flag", torch.int64), host_ptr(pts, "pts", _F), host_ptr(boxes3d, "boxes3d", _F)
    m, n = boxes3d.size(0), pts.size(0)
    need(pts_flag, m * n, "pts_flag"); need(pts, n * 3, "pts"); need(boxes3d, m * 7, "boxes3d")
    _lib.check(_lib.lib().epnet_pts_in_boxes3d_host(pf, pp, pb, m, n), "pts_in_boxes3d_cpu")
    return 1


@writes("pooled_pts", "pooled_features", "pooled_empty_flag")
def roipool3d_cpu(pts, boxes3d, pts_feature, pooled_pts, pooled_features, pooled_empty_flag):
    """roipool3d.cpp:127-195 -- a HOST op in the reference as well"""
    pp, pb, pf = host_ptr(pts, "pts", _F), host_ptr(boxes3d, "boxes3d", _F), host_ptr(pts_feature, "pts_feature", _F)
    op, of = host_ptr(pooled_pts, "pooled_pts", _F), host_ptr(pooled_features, "pooled_features", _F)
    oe = host_ptr(pooled_empty_flag, "pooled_empty_flag", torch.int64)
    m, n, c, s = boxes3d.size(0), pts.size(0), pts_feature.size(1), pooled_pts.size(1)
    need(pts, n * 3, "pts"); need(boxes3d, m * 7, "boxes3d"); need(pts_feature, n * c, "pts_feature")
    need(pooled_pts, m * s * 3, "pooled_pts"); need(pooled_features, m * s * c, "pooled_features"); need(pooled_empty_flag, m, "pooled_empty_flag")
    _lib.check(_lib.lib().epnet_roipool3d_host(pp, pb, pf, op, of, oe, m, n, c, s), "roipool3d_cpu")
    return 1

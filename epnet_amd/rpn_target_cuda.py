"""Stand-in of an extension module the reference does not have: its RPN training targets are made in the loader, per scene, on
the host (lib/datasets/kitti_rcnn_dataset.py: data_augmentation :698-755, generate_rpn_training_labels :547-576).
``rpn_targets_gpu`` is the one call of ``epnet_rpn_targets`` (include/epnet_ops.h): augmentation and per-point labels of a
whole batch in one launch on the tensors' device and current stream, nothing read back.
"""
import torch

from . import _lib
from ._tensor import dev_ptr, need, on_device_of, writes

_F = torch.float32
_I = torch.int32


@writes("pts_out", "gt_out", "cls_label", "reg_label")
def rpn_targets_gpu(pts, gt_boxes3d, gt_alpha, aug, extra_width, pts_out, gt_out, cls_label, reg_label):
    """pts (B,N,3), gt_boxes3d (B,G,7) zero-padded, gt_alpha (B,G) or None, aug (B,4) [rotate, angle, scale, flip] or None ->
    pts_out (B,N,3) and gt_out (B,G,7) (both may be None without aug), cls_label (B,N) int32, reg_label (B,N,7). No output
    may be the input it corresponds to."""
    if pts.dim() != 3 or pts.shape[2] != 3:
        raise RuntimeError("pts must be (B, N, 3)")
    if gt_boxes3d.dim() != 3 or gt_boxes3d.shape[2] != 7 or gt_boxes3d.shape[0] != pts.shape[0]:
        raise RuntimeError("gt_boxes3d must be (B, G, 7)")
    b, n, g = pts.shape[0], pts.shape[1], gt_boxes3d.shape[1]
    pp, pg = dev_ptr(pts, "pts", _F), dev_ptr(gt_boxes3d, "gt_boxes3d", _F)
    pc, pr = dev_ptr(cls_label, "cls_label", _I), dev_ptr(reg_label, "reg_label", _F)
    need(cls_label, b * n, "cls_label"); need(reg_label, b * n * 7, "reg_label")
    pa = pu = po = pgo = None
    if gt_alpha is not None:
        pa = dev_ptr(gt_alpha, "gt_alpha", _F)
        need(gt_alpha, b * g, "gt_alpha")
    if aug is not None:
        pu = dev_ptr(aug, "aug", _F)
        need(aug, b * 4, "aug")
        if gt_alpha is None or pts_out is None or gt_out is None:
            raise RuntimeError("aug needs gt_alpha, pts_out and gt_out")
    if pts_out is not None:
        po = dev_ptr(pts_out, "pts_out", _F)
        need(pts_out, b * n * 3, "pts_out")
        if po == pp and b * n:
            raise RuntimeError("pts_out must not alias pts")
    if gt_out is not None:
        pgo = dev_ptr(gt_out, "gt_out", _F)
        need(gt_out, b * g * 7, "gt_out")
        if pgo == pg and b * g:
            raise RuntimeError("gt_out must not alias gt_boxes3d")
    with on_device_of(pts) as s:
        _lib.check(_lib.lib().epnet_rpn_targets(b, n, g, float(extra_width), pp, pg, pa, pu, po, pgo, pc, pr, s), "rpn_targets")
    return 1

"""Stand-in of an extension module the reference does not have: its losses are Python (lib/utils/loss_utils.py,
lib/net/train_functions.py:92-284). ``box_loss_gpu`` is the one call of ``epnet_box_loss`` (include/epnet_ops.h): a whole RPN or
RCNN loss, forward and backward, on the tensors' device and current stream, nothing read back.
"""
import torch

from . import _lib
from . import pointnet2_utils
from ._tensor import dev_ptr, need, on_device_of, writes

_F = torch.float32
_I = torch.int32

TERMS = 24  # EPNET_BOX_LOSS_TERMS
IOU_LOSS_TYPES = {"raw": 0, "cls_mask_with_bin": 1}
CLS_LOSS_TYPES = {"SigmoidFocalLoss": 0, "BinaryCrossEntropy": 1, "none": 2}


def workspace(like, rows, c):
    """the call's scratch, from the package's allocation helper (the GPU tests put canaries around it)"""
    nbytes = _lib.lib().epnet_box_loss_workspace_bytes(rows, c)
    return pointnet2_utils._new(like, (max(nbytes, 16),), torch.uint8)


@writes("terms", "grad_cls", "grad_reg", "grad_iou_branch")
def box_loss_gpu(cls_logit, pred_reg, reg_label, cls_label, reg_mask, iou_branch_pred, anchor, loc_scope, loc_bin_size, num_head_bin,
                 ry_fine, iou_loss_type, cls_loss_type, focal_alpha, focal_gamma, fg_weight, w_cls, w_reg, w_train, ce_weight,
                 terms, grad_cls, grad_reg, grad_iou_branch=None, ws=None):
    """cls_logit (R), pred_reg (R,C), reg_label (R,7), cls_label (R) int32, reg_mask (R) int32 or None, iou_branch_pred (R) or
    None, anchor (3) -> terms (24), grad_cls (R), grad_reg (R,C), grad_iou_branch (R) or None; iou_loss_type / cls_loss_type by
    the reference's names (IOU_LOSS_TYPES, CLS_LOSS_TYPES)"""
    if pred_reg.dim() != 2:
        raise RuntimeError("pred_reg must be (rows, C)")
    rows, c = pred_reg.shape
    if iou_loss_type not in IOU_LOSS_TYPES:
        raise NotImplementedError("TRAIN.IOU_LOSS_TYPE %r (the reference knows %s)" % (iou_loss_type, sorted(IOU_LOSS_TYPES)))
    if cls_loss_type not in CLS_LOSS_TYPES:
        raise NotImplementedError("classification loss %r" % (cls_loss_type,))
    pc, pr, pl = dev_ptr(cls_logit, "cls_logit", _F), dev_ptr(pred_reg, "pred_reg", _F), dev_ptr(reg_label, "reg_label", _F)
    pk, pa = dev_ptr(cls_label, "cls_label", _I), dev_ptr(anchor, "anchor", _F)
    pt, gc, gr = dev_ptr(terms, "terms", _F), dev_ptr(grad_cls, "grad_cls", _F), dev_ptr(grad_reg, "grad_reg", _F)
    need(cls_logit, rows, "cls_logit"); need(reg_label, rows * 7, "reg_label"); need(cls_label, rows, "cls_label"); need(anchor, 3, "anchor")
    need(terms, TERMS, "terms"); need(grad_cls, rows, "grad_cls"); need(grad_reg, rows * c, "grad_reg")
    pm = pb = gb = None
    if reg_mask is not None:
        pm = dev_ptr(reg_mask, "reg_mask", _I)
        need(reg_mask, rows, "reg_mask")
    if (iou_branch_pred is None) != (grad_iou_branch is None):
        raise RuntimeError("iou_branch_pred and grad_iou_branch come together")
    if iou_branch_pred is not None:
        pb, gb = dev_ptr(iou_branch_pred, "iou_branch_pred", _F), dev_ptr(grad_iou_branch, "grad_iou_branch", _F)
        need(iou_branch_pred, rows, "iou_branch_pred"); need(grad_iou_branch, rows, "grad_iou_branch")
    if ws is None:
        ws = workspace(pred_reg, rows, c)
    pw = dev_ptr(ws, "workspace", torch.uint8)
    with on_device_of(pred_reg) as s:
        _lib.check(_lib.lib().epnet_box_loss(rows, c, float(loc_scope), float(loc_bin_size), int(num_head_bin), int(bool(ry_fine)),
                                             IOU_LOSS_TYPES[iou_loss_type], CLS_LOSS_TYPES[cls_loss_type], float(focal_alpha),
                                             float(focal_gamma), float(fg_weight), float(w_cls), float(w_reg), float(w_train),
                                             float(ce_weight), pc, pr, pl, pk, pm, pb, pa, pt, gc, gr, gb, pw, ws.numel(), s), "box_loss")
    return 1

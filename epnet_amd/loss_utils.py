"""The training losses (reference: get_rpn_loss / get_rcnn_loss of lib/net/train_functions.py:92-284 over get_reg_loss and
SigmoidFocalClassificationLoss of lib/utils/loss_utils.py) with no host synchronisation.

The reference selects the foreground rows by boolean-mask indexing four to six times per loss, branches on ``fg_sum`` on the
host and reads some 25 scalars back with ``.item()`` in the middle of every step; ``get_reg_loss`` itself is well over a
hundred small torch kernels on a few hundred rows, and autograd replays as many. Here a whole loss -- classification term,
every regression term, the consistency-enforcing IoU term, the IoU branch, the callers' weights -- and the gradients with
respect to the three head outputs are ONE call of ``epnet_box_loss`` (csrc/loss.hip); ``backward`` multiplies the stored
gradients by the incoming scalar. Nothing is read back: ``rpn_loss`` / ``rcnn_loss`` return the differentiable total and a
small ``terms`` tensor on the device with every scalar the reference logs (``names`` says which is which, in the reference's
keys), so a trainer that logs does ONE read-back when it chooses to -- ``dict(zip(names, terms.tolist()))`` -- and one that
does not does none. A step can therefore be queued behind the previous one, or captured into a HIP graph.

No foreground row gives regression terms of exactly 0 with zero gradients (sums over no rows divided by max(count, 1)), as
train_functions.py:151-153, 262-263 do with a host branch.
"""
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import loss_cuda
from . import pointnet2_utils
from ._tensor import as_f32, f32_region

# the order of `terms` (EPNET_BOX_LOSS_TERMS, include/epnet_ops.h)
TERM_NAMES = ["total", "loss", "loss_cls", "loss_cls_pos", "loss_cls_neg", "loss_reg", "loss_loc", "loss_angle", "loss_size", "loss_iou",
              "loss_x_bin", "loss_z_bin", "loss_x_res", "loss_z_res", "loss_y_offset", "loss_ry_bin", "loss_ry_res", "iou_branch_loss",
              "fg_sum", "cls_pos", "cls_neg", "cls_valid", "loss_size_unweighted", "loss_iou_unweighted"]
# the same slots under the keys the reference's tb_dict / disp_dict / reg_loss_dict use for them. `total` carries
# TRAIN.RPN_TRAIN_WEIGHT / RCNN_TRAIN_WEIGHT (disp_dict's rpn_loss / rcnn_loss), `loss` does not (tb_dict's)
RPN_TERM_NAMES = ["rpn_loss_weighted", "rpn_loss", "rpn_loss_cls", "rpn_loss_cls_pos", "rpn_loss_cls_neg", "rpn_loss_reg", "rpn_loss_loc",
                  "rpn_loss_angle", "rpn_loss_size", "rpn_loss_iou", "rpn_loss_x_bin", "rpn_loss_z_bin", "rpn_loss_x_res", "rpn_loss_z_res",
                  "rpn_loss_y_offset", "rpn_loss_ry_bin", "rpn_loss_ry_res", "rpn_iou_branch_loss", "rpn_fg_sum", "rpn_cls_fg", "rpn_cls_bg",
                  "rpn_cls_valid", "rpn_loss_size_unweighted", "rpn_loss_iou_unweighted"]
RCNN_TERM_NAMES = ["rcnn_loss_weighted", "rcnn_loss", "rcnn_loss_cls", "rcnn_loss_cls_pos", "rcnn_loss_cls_neg", "rcnn_loss_reg", "rcnn_loss_loc",
                   "rcnn_loss_angle", "rcnn_loss_size", "rcnn_loss_iou", "loss_x_bin", "loss_z_bin", "loss_x_res", "loss_z_res",
                   "loss_y_offset", "loss_ry_bin", "loss_ry_res", "iou_branch_loss", "rcnn_reg_fg", "rcnn_cls_fg", "rcnn_cls_bg",
                   "rcnn_cls_valid", "loss_size", "loss_iou"]
# further keys of the reference that hold one of the values above: reg_loss_dict's loss_loc / loss_angle (get_rcnn_loss copies
# them into tb_dict, :261), disp_dict's reg_fg_sum / rcnn_iou_loss (:72-78), and the RCNN focal branch's pos / neg parts, which
# the reference logs under the RPN's keys (:199-200)
RCNN_KEY_ALIASES = {"loss_loc": "rcnn_loss_loc", "loss_angle": "rcnn_loss_angle", "reg_fg_sum": "rcnn_reg_fg", "rcnn_iou_loss": "rcnn_loss_iou",
                    "rpn_loss_cls_pos": "rcnn_loss_cls_pos", "rpn_loss_cls_neg": "rcnn_loss_cls_neg"}

LossReturn = namedtuple("LossReturn", ["loss", "terms", "names"])


def default_cfg():
    """the keys the two losses read, values of tools/cfgs/LI_Fusion_with_attention_use_ce_loss.yaml (:19, :21, :46-49, :70-75,
    :100-103, :127-129, :176-179); any object with the same attributes works (e.g. the reference's lib.config.cfg)"""
    rpn = SimpleNamespace(LOC_XZ_FINE=True, LOC_SCOPE=3.0, LOC_BIN_SIZE=0.5, NUM_HEAD_BIN=12, LOSS_CLS="SigmoidFocalLoss", FG_WEIGHT=15,
                          FOCAL_ALPHA=[0.25, 0.75], FOCAL_GAMMA=2.0, LOSS_WEIGHT=[1.0, 1.0])
    rcnn = SimpleNamespace(LOC_SCOPE=1.5, LOC_BIN_SIZE=0.5, NUM_HEAD_BIN=9, LOC_Y_BY_BIN=False, LOC_Y_SCOPE=0.5, LOC_Y_BIN_SIZE=0.25,
                           SIZE_RES_ON_ROI=False, LOSS_CLS="BinaryCrossEntropy", FOCAL_ALPHA=[0.25, 0.75], FOCAL_GAMMA=2.0)
    train = SimpleNamespace(RPN_TRAIN_WEIGHT=1.0, RCNN_TRAIN_WEIGHT=1.0, CE_WEIGHT=5.0, IOU_LOSS_TYPE="cls_mask_with_bin")
    return SimpleNamespace(CLS_MEAN_SIZE=np.array([[1.52563191462, 1.62856739989, 3.88311640418]], dtype=np.float32),
                           USE_IOU_BRANCH=False, RPN=rpn, RCNN=rcnn, TRAIN=train)


def _ambient_cfg():
    """the reference's global config when its module is loaded in this process, else the yaml-valued defaults above"""
    import sys
    ref = sys.modules.get("lib.config")
    return ref.cfg if ref is not None and hasattr(ref, "cfg") else default_cfg()


_anchors = {}


def _anchor_on(device, cfg):
    """CLS_MEAN_SIZE[0] as a device tensor, uploaded once per device and value (an upload per call would be a host copy in
    the middle of the step, and cannot be captured into a graph)"""
    values = tuple(float(v) for v in np.asarray(cfg.CLS_MEAN_SIZE[0], dtype=np.float32))
    key = (str(device), values)
    if key not in _anchors:
        _anchors[key] = torch.tensor(values, dtype=torch.float32, device=device)
    return _anchors[key]


class BoxLoss(Function):
    """(cls_logit (R), pred_reg (R,C), iou_branch (R) or None | reg_label (R,7), cls_label (R) int32, reg_mask (R) int32 or None,
    anchor (3), settings) -> total (scalar, differentiable w.r.t. the first three), terms (24)"""

    @staticmethod
    def forward(ctx, cls_logit, pred_reg, iou_branch, reg_label, cls_label, reg_mask, anchor, settings):
        rows, c = pred_reg.shape
        new = pointnet2_utils._new
        terms = new(pred_reg, (loss_cuda.TERMS,))
        grad_cls, grad_reg = new(pred_reg, (rows,)), new(pred_reg, (rows, c))
        grad_branch = new(pred_reg, (rows,)) if iou_branch is not None else None
        if rows == 0:
            terms.zero_()
        else:
            loss_cuda.box_loss_gpu(cls_logit, pred_reg, reg_label, cls_label, reg_mask, iou_branch, anchor, terms=terms, grad_cls=grad_cls,
                                   grad_reg=grad_reg, grad_iou_branch=grad_branch, **settings)
        ctx.grads = (grad_cls, grad_reg, grad_branch)
        ctx.mark_non_differentiable(terms)
        return terms[0].clone(), terms

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_total, _grad_terms):
        grad_cls, grad_reg, grad_branch = ctx.grads
        return (grad_cls * grad_total, grad_reg * grad_total, None if grad_branch is None else grad_branch * grad_total,
                None, None, None, None, None)


def _dice_loss(logit, target):
    """DiceLoss of loss_utils.py:8-23 (the config.py default for the RPN): no synchronisation in the reference either"""
    prob = torch.sigmoid(logit.view(-1))
    target = target.float().view(-1)
    mask = (target != -1).float()
    return 1.0 - (torch.min(prob, target) * mask).sum() / torch.clamp((torch.max(prob, target) * mask).sum(), min=1.0)


def _flat_inputs(cls_logit, pred_reg, reg_label, cls_label, reg_mask, iou_branch):
    for name, t in (("cls", cls_logit), ("reg", pred_reg), ("reg_label", reg_label), ("cls_label", cls_label)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError("%s must be a CUDAtensor (epnet_amd has no CPU fallback)" % name)
    rows = cls_label.numel()
    cls_logit = cls_logit.reshape(-1).float().contiguous()
    if cls_logit.numel() != rows:
        raise NotImplementedError("a class head wider than 1 (CrossEntropy, train_functions.py:208-215, reads cfg.TRAIN.LOSS_CLS, "
                                  "a key that does not exist)")
    pred_reg = pred_reg.reshape(rows, -1).float().contiguous()
    reg_label = reg_label.reshape(rows, 7).float().contiguous()
    cls_label = cls_label.reshape(-1).to(torch.int32).contiguous()
    if reg_mask is not None:
        reg_mask = reg_mask.reshape(-1).to(torch.int32).contiguous()
    if iou_branch is not None:
        iou_branch = iou_branch.reshape(-1).float().contiguous()
    return cls_logit, pred_reg, reg_label, cls_label, reg_mask, iou_branch


def _run(stage_cfg, cfg, names, cls_logit, pred_reg, reg_label, cls_label, reg_mask, iou_branch, ry_fine, w_cls, w_reg, w_train, fg_weight):
    loss_cls = stage_cfg.LOSS_CLS
    if loss_cls not in ("DiceLoss", "SigmoidFocalLoss", "BinaryCrossEntropy"):
        raise NotImplementedError("LOSS_CLS %r (CrossEntropy is a multi-class head read from cfg.TRAIN.LOSS_CLS, a key that does "
                                  "not exist: train_functions.py:208)" % (loss_cls,))
    nb = int(stage_cfg.LOC_SCOPE / stage_cfg.LOC_BIN_SIZE) * 2
    cls_logit, pred_reg, reg_label, cls_label, reg_mask, iou_branch = _flat_inputs(cls_logit, pred_reg, reg_label, cls_label, reg_mask, iou_branch)
    if pred_reg.shape[1] != 4 * nb + 1 + 2 * stage_cfg.NUM_HEAD_BIN + 3:
        raise RuntimeError("%d regression channels, the configuration has %d" % (pred_reg.shape[1], 4 * nb + 1 + 2 * stage_cfg.NUM_HEAD_BIN + 3))
    settings = dict(loc_scope=stage_cfg.LOC_SCOPE, loc_bin_size=stage_cfg.LOC_BIN_SIZE, num_head_bin=stage_cfg.NUM_HEAD_BIN, ry_fine=ry_fine,
                    iou_loss_type=cfg.TRAIN.IOU_LOSS_TYPE, cls_loss_type="none" if loss_cls == "DiceLoss" else loss_cls,
                    focal_alpha=stage_cfg.FOCAL_ALPHA[0], focal_gamma=stage_cfg.FOCAL_GAMMA, fg_weight=fg_weight, w_cls=w_cls, w_reg=w_reg,
                    w_train=w_train, ce_weight=cfg.TRAIN.CE_WEIGHT)
    total, terms = BoxLoss.apply(cls_logit, pred_reg, iou_branch, reg_label, cls_label, reg_mask, _anchor_on(pred_reg.device, cfg), settings)
    if loss_cls == "DiceLoss":
        dice = _dice_loss(cls_logit, cls_label)
        total = total + dice * (w_cls * w_train)
        add = torch.zeros_like(terms)
        d = dice.detach()
        add[0], add[1], add[2] = d * (w_cls * w_train), d * w_cls, d
        terms = terms + add
    return LossReturn(total, terms, names)


@f32_region
def rpn_loss(rpn_cls, rpn_reg, rpn_cls_label, rpn_reg_label, cfg=None):
    """get_rpn_loss, train_functions.py:92-163, times TRAIN.RPN_TRAIN_WEIGHT (:60): rpn_cls (B,N,1), rpn_reg (B,N,C),
    rpn_cls_label (B,N) in {-1, 0, 1}, rpn_reg_label (B,N,7) -> LossReturn(loss, terms, RPN_TERM_NAMES)"""
    cfg = cfg if cfg is not None else _ambient_cfg()
    rpn_cls, rpn_reg = as_f32(rpn_cls), as_f32(rpn_reg)   # bf16 / fp16 heads: one upcast; autograd casts the gradients back
    if not cfg.RPN.LOC_XZ_FINE:
        raise NotImplementedError("RPN.LOC_XZ_FINE = False: the reference's IoU term reads x_res_l, which that configuration "
                                  "never defines (loss_utils.py:235)")
    return _run(cfg.RPN, cfg, RPN_TERM_NAMES, rpn_cls, rpn_reg, rpn_reg_label, rpn_cls_label, None, None, False,
                cfg.RPN.LOSS_WEIGHT[0], cfg.RPN.LOSS_WEIGHT[1], cfg.TRAIN.RPN_TRAIN_WEIGHT, cfg.RPN.FG_WEIGHT)


@f32_region
def rcnn_loss(ret_dict, cfg=None):
    """get_rcnn_loss, train_functions.py:165-284, times TRAIN.RCNN_TRAIN_WEIGHT (:74): reads rcnn_cls (R,1), rcnn_reg (R,C),
    cls_label (R), reg_valid_mask (R), gt_of_rois (R,7) and, with USE_IOU_BRANCH, rcnn_iou_branch (R,1) -- the keys
    ProposalTargetLayer and the RCNN head produce -> LossReturn(loss, terms, RCNN_TERM_NAMES)"""
    cfg = cfg if cfg is not None else _ambient_cfg()
    if cfg.RCNN.LOC_Y_BY_BIN:
        raise NotImplementedError("RCNN.LOC_Y_BY_BIN = True: the reference's IoU term reads y_offset_l, which that configuration "
                                  "never defines (loss_utils.py:236)")
    if cfg.RCNN.SIZE_RES_ON_ROI:
        raise NotImplementedError("RCNN.SIZE_RES_ON_ROI (per-ROI anchors; the anchor is the 3-vector CLS_MEAN_SIZE here)")
    branch = as_f32(ret_dict["rcnn_iou_branch"]) if cfg.USE_IOU_BRANCH else None   # bf16 / fp16 heads, as rpn_loss
    return _run(cfg.RCNN, cfg, RCNN_TERM_NAMES, as_f32(ret_dict["rcnn_cls"]), as_f32(ret_dict["rcnn_reg"]), ret_dict["gt_of_rois"], ret_dict["cls_label"],
                ret_dict["reg_valid_mask"], branch, True, 1.0, 1.0, cfg.TRAIN.RCNN_TRAIN_WEIGHT, 1.0)

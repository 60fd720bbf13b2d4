"""Readers of tests/golden/loss.npz shared by test_loss.py and test_loss_gpu.py: the case table is the generator's, the settings
are loss_restate.settings with the case's variations."""
import ast
import os

import numpy as np

import loss_restate as lr

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "loss.npz")

GENERATOR = os.path.join(HERE, "golden", "make_golden_loss.py")


def case_table():
    """name -> (stage, kind, iou type, classification loss, IoU branch), parsed from the generator's source (importing it would
    import torch stand-ins this process does not want)"""
    tree = ast.parse(open(GENERATOR).read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == "CASES":
            return ast.literal_eval(node.value)
    raise AssertionError("CASES not found")


CASES = case_table()

# the reference's key of a scalar -> the name of the term that holds it (loss_restate.TERM_NAMES)
RPN_KEYS = {"rpn_loss": "total", "rpn_loss_cls": "loss_cls", "rpn_loss_cls_pos": "loss_cls_pos", "rpn_loss_cls_neg": "loss_cls_neg",
            "rpn_loss_reg": "loss_reg", "rpn_loss_loc": "loss_loc", "rpn_loss_angle": "loss_angle", "rpn_loss_size": "loss_size",
            "rpn_loss_iou": "loss_iou", "rpn_fg_sum": "fg_sum"}
RCNN_KEYS = {"rcnn_loss": "total", "rcnn_loss_cls": "loss_cls", "rpn_loss_cls_pos": "loss_cls_pos", "rpn_loss_cls_neg": "loss_cls_neg",
             "rcnn_loss_reg": "loss_reg", "rcnn_loss_loc": "loss_loc", "rcnn_loss_angle": "loss_angle", "rcnn_loss_size": "loss_size",
             "rcnn_loss_iou": "loss_iou", "rcnn_iou_loss": "loss_iou", "rcnn_cls_fg": "cls_pos", "rcnn_cls_bg": "cls_neg",
             "rcnn_reg_fg": "fg_sum", "reg_fg_sum": "fg_sum", "loss_loc": "loss_loc", "loss_angle": "loss_angle",
             "loss_size": "loss_size_unweighted", "loss_iou": "loss_iou_unweighted", "iou_branch_loss": "iou_branch_loss",
             "loss_x_bin": "loss_x_bin", "loss_z_bin": "loss_z_bin", "loss_x_res": "loss_x_res", "loss_z_res": "loss_z_res",
             "loss_y_offset": "loss_y_offset", "loss_ry_bin": "loss_ry_bin", "loss_ry_res": "loss_ry_res"}


def settings(name):
    stage, _, iou_type, cls_type, branch = CASES[name]
    return lr.settings(stage, iou_type=iou_type, cls_type=cls_type, use_iou_branch=branch)


def load():
    return np.load(FIXTURE)


def inputs(fx, name):
    pre = name + "__"
    get = lambda k: fx[pre + k] if (pre + k) in fx.files else None  # noqa: E731
    return {"cls_logit": fx[pre + "cls_logit"], "pred_reg": fx[pre + "pred_reg_f16"].astype(np.float32), "reg_label": fx[pre + "reg_label"],
            "cls_label": fx[pre + "cls_label"], "reg_mask": get("reg_mask"), "iou_branch": get("iou_branch")}


def reference_scalars(fx, name):
    """-> [(reference key, term name, float64 value, bound)]"""
    pre = name + "__"
    keys = RPN_KEYS if CASES[name][0] == "rpn" else RCNN_KEYS
    return [(str(k), keys[str(k)], float(v), float(b))
            for k, v, b in zip(fx[pre + "scalar_names"], fx[pre + "scalars_f64"], fx[pre + "scalars_bound"])]

"""Regenerates tests/golden/loss.npz. Runs ONLY in the build container (needs /root/reference); the fixture is plain data.

What runs is the REFERENCE'S OWN Python, imported unmodified from /root/reference: ``lib/utils/loss_utils.py`` (get_reg_loss,
SigmoidFocalClassificationLoss) and the closures get_rpn_loss / get_rcnn_loss of ``lib/net/train_functions.py``, which are local
to model_joint_fn_decorator and are reached by calling the model_fn it returns with a stand-in model (a callable that returns a
prepared ret_dict and carries rpn.rpn_cls_loss_func / rcnn_net.cls_loss_func) and a data dict of numpy arrays. Stand-ins as in
make_golden_rcnn.py: easydict, torch.cuda.FloatTensor -> the CPU constructor, Tensor.cuda = identity, no bytecode written.

Every case runs twice: in float64 (torch.cuda.FloatTensor = torch.DoubleTensor and Tensor.float = Tensor.double while model_fn
runs, so that the labels model_fn casts with .float() stay float64 too) -- the yardstick -- and in float32. Stored per case: the
inputs, every returned loss and dict entry, the autograd gradients w.r.t. the regression output, the classification logits and
the IoU-branch output, in both precisions, and per compared tensor the bound of the float32 kernel:
4 x max |float32 run - float64 run|, not less than 1e-6 x max |float64 run|.

Inputs are float32 numbers (the regression outputs float16 numbers: half the bytes). Background rows' regression outputs, which
no loss reads, are drawn on a grid of 1/4 so that the file compresses below the 1 MB limit. A foreground row within 1e-4 of a
kink (a smooth-L1 argument at +-1, the two operands of a clamp / min / max within 1e-4 relative) is redrawn; the count is
stored and may not exceed 1 % of a case's rows.
"""
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import loss_restate as lr  # noqa: E402
from make_golden_rcnn import install_easydict  # noqa: E402

REF = "/root/reference"
MARGIN = 1e-4

# name -> (stage, kind, iou type, classification loss, IoU branch)
CASES = {
    "rpn_a_bin": ("rpn", "a", "cls_mask_with_bin", "SigmoidFocalLoss", False),
    "rpn_b_bin": ("rpn", "b", "cls_mask_with_bin", "SigmoidFocalLoss", False),
    "rpn_c_bin": ("rpn", "c", "cls_mask_with_bin", "SigmoidFocalLoss", False),
    "rpn_a_raw": ("rpn", "a", "raw", "BinaryCrossEntropy", False),
    "rpn_b_raw": ("rpn", "b", "raw", "BinaryCrossEntropy", False),
    "rpn_nofg": ("rpn", "nofg", "cls_mask_with_bin", "SigmoidFocalLoss", False),
    "rpn_onefg": ("rpn", "onefg", "cls_mask_with_bin", "SigmoidFocalLoss", False),
    "rcnn_a_bin": ("rcnn", "a", "cls_mask_with_bin", "BinaryCrossEntropy", False),
    "rcnn_b_bin": ("rcnn", "b", "cls_mask_with_bin", "BinaryCrossEntropy", False),
    "rcnn_c_bin": ("rcnn", "c", "cls_mask_with_bin", "BinaryCrossEntropy", False),
    "rcnn_a_raw": ("rcnn", "a", "raw", "SigmoidFocalLoss", True),
    "rcnn_b_raw": ("rcnn", "b", "raw", "SigmoidFocalLoss", True),
    "rcnn_b_bin_branch": ("rcnn", "b", "cls_mask_with_bin", "BinaryCrossEntropy", True),
    "rcnn_nofg": ("rcnn", "nofg", "cls_mask_with_bin", "BinaryCrossEntropy", False),
    "rcnn_onefg": ("rcnn", "onefg", "cls_mask_with_bin", "SigmoidFocalLoss", True),
}
ROWS = {"rpn": 512, "rcnn": 128}


def case_settings(name):
    stage, _, iou_type, cls_type, branch = CASES[name]
    return lr.settings(stage, iou_type=iou_type, cls_type=cls_type, use_iou_branch=branch)


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def f16(a):
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float32)


def draw_labels(rng, s, rows, kind):
    scope, bs = s["loc_scope"], s["loc_bin_size"]
    nb = int(scope / bs) * 2
    anchor = np.asarray(s["anchor"])
    lab = np.zeros((rows, 7))
    lab[:, 0] = rng.uniform(-scope, scope, rows) * 0.95
    lab[:, 2] = rng.uniform(-scope, scope, rows) * 0.95
    lab[:, 1] = rng.normal(0, 0.3, rows)
    lab[:, 3:6] = anchor * (1 + 0.1 * rng.normal(size=(rows, 3)))
    lab[:, 6] = rng.uniform(-np.pi, 2 * np.pi, rows)
    if kind == "c":
        # exactly on bin edges, on +-scope and beyond it; every bin of x and z, every heading class, both sides of every branch of the flip
        edges = np.concatenate([-scope + bs * np.arange(nb + 1), [-scope - 0.75, scope + 1.25, -scope - 1e-3, scope - 1e-3, scope - 5e-4]])
        lab[:, 0] = edges[np.arange(rows) % len(edges)]
        lab[:, 2] = edges[(np.arange(rows) // 3) % len(edges)]
        heads = np.concatenate([(np.arange(24) + 0.5) * (2 * np.pi / 24), [0.0, -0.3, -2.0, -4.5, 7.0, 1.5, 1.65, 4.6, 4.8, 3.1, 0.78, 0.79, 5.49, 5.5]])
        lab[:, 6] = heads[(np.arange(rows) // 2) % len(heads)]
    return f32(lab)


def draw_row_predictions(rng, s, lab, kind, score_logit):
    """regression outputs of foreground rows: 'a' = the labels' own encoding plus noise, otherwise N(0, 1)"""
    rows = lab.shape[0]
    c = lr.channels(s)
    if kind in ("b", "c"):
        return f16(rng.normal(size=(rows, c)))
    scope, bs, nh = s["loc_scope"], s["loc_bin_size"], s["num_head_bin"]
    nb = int(scope / bs) * 2
    probe = lr.box_loss(dict(s, use_iou_branch=False), score_logit, np.zeros((rows, c)), lab, np.ones(rows, np.int64))
    xb, zb, rb = probe["aux"]["x_bin"], probe["aux"]["z_bin"], probe["aux"]["ry_bin"]
    shift = np.clip(lab[:, [0, 2]].astype(np.float64) + scope, 0, 2 * scope - 1e-3)
    resn = (shift - (np.stack([xb, zb], 1) * bs + bs / 2)) / bs
    r_resn = lr.heading_labels(lab[:, 6].astype(np.float64), nh, s["ry_fine"], np.float64)[1]
    pred = 0.1 * rng.normal(size=(rows, c))
    r = np.arange(rows)
    pred[r, xb] += 8
    pred[r, nb + zb] += 8
    pred[r, 2 * nb + xb] = resn[:, 0] + 0.05 * rng.normal(size=rows)
    pred[r, 3 * nb + zb] = resn[:, 1] + 0.05 * rng.normal(size=rows)
    pred[:, 4 * nb] = lab[:, 1] + 0.05 * rng.normal(size=rows)
    pred[r, 4 * nb + 1 + rb] += 6
    pred[r, 4 * nb + 1 + nh + rb] = r_resn + 0.05 * rng.normal(size=rows)
    anchor = np.asarray(s["anchor"])
    pred[:, -3:] = (lab[:, 3:6] - anchor) / anchor + 0.03 * rng.normal(size=(rows, 3))
    return f16(pred)


def make_inputs(name, seed):
    stage, kind, _, cls_type, branch = CASES[name]
    s = case_settings(name)
    rng = np.random.default_rng(seed)
    rows, c = ROWS[stage], lr.channels(s)
    u = rng.uniform(size=rows)
    if stage == "rpn":
        fg = u < 0.09                                             # a KITTI scene: a few per cent of the points lie in a box
        cls_label = np.where(fg, 1, np.where(u > 0.97, -1, 0)).astype(np.int64)
        reg_mask = None
    else:
        fg = u > 0.55                                             # REG_FG_THRESH; CLS_FG_THRESH 0.6, CLS_BG_THRESH 0.45
        if cls_type == "BinaryCrossEntropy":                      # (the reference run cannot take -1 here under torch 2.10)
            cls_label = (u > 0.6).astype(np.int64)
        else:
            cls_label = np.where(u > 0.6, 1, np.where(u < 0.45, 0, -1)).astype(np.int64)
        reg_mask = fg.astype(np.int64)
    if kind in ("nofg", "onefg"):
        fg[:] = False
        if kind == "onefg":
            fg[rows // 3] = True
        if stage == "rpn":
            cls_label = np.where(fg, 1, np.minimum(cls_label, 0))
        else:
            reg_mask = fg.astype(np.int64)
            cls_label = np.where(fg, 1, np.minimum(cls_label, 0) if cls_type != "BinaryCrossEntropy" else 0)
    label_kind = "b" if kind in ("nofg", "onefg") else kind
    lab = draw_labels(rng, s, rows, label_kind)
    if stage == "rpn":
        lab[~fg] = 0                                              # the loader leaves the labels of background points zero
    cls_logit = f32(np.where(fg, 2.0, -2.0) + rng.normal(size=rows) * (0.5 if kind == "a" else 1.5))
    pred = f16(np.round(rng.normal(size=(rows, c)) * 4) / 4)
    idx = np.nonzero(fg)[0]
    pred[idx] = draw_row_predictions(rng, s, lab[idx], label_kind, cls_logit[idx])
    iou_branch = None
    if branch:
        iou_branch = f32(1 / (1 + np.exp(-rng.normal(size=rows) * 2)))
        if kind == "b" and len(idx) > 4:                          # both clamps of the branch's input (the head has no activation)
            iou_branch[idx[0]], iou_branch[idx[1]], iou_branch[idx[2]] = np.float32(5e-5), np.float32(1.25), np.float32(-0.2)
    # ---- kink margins: redraw the foreground rows that sit within MARGIN of one
    redrawn = 0
    for _ in range(20):
        out = lr.box_loss(s, cls_logit, pred, lab, cls_label, reg_mask, iou_branch)
        aux = out["aux"]
        bad = np.nonzero((aux["margin_smooth_l1"] < MARGIN) | (aux["margin_relative"] < MARGIN))[0]
        if not len(bad):
            break
        rows_bad = aux["fg_rows"][bad]
        redrawn += len(rows_bad)
        pred[rows_bad] = draw_row_predictions(rng, s, lab[rows_bad], label_kind, cls_logit[rows_bad])
        if iou_branch is not None:
            iou_branch[rows_bad] = f32(1 / (1 + np.exp(-rng.normal(size=len(rows_bad)) * 2)))
    else:
        raise AssertionError("rows on a kink after 20 redraws: " + name)
    assert redrawn <= 0.01 * rows, (name, redrawn)
    # the bin labels must not depend on the precision (a label that does is not a test of the loss)
    o32 = lr.box_loss(s, cls_logit, pred, lab, cls_label, reg_mask, iou_branch, dtype=np.float32)
    for k in ("x_bin", "z_bin", "ry_bin", "opposite"):
        assert np.array_equal(o32["aux"][k], out["aux"][k]), (name, k)
    return {"cls_logit": cls_logit, "pred_reg": pred, "reg_label": lab, "cls_label": cls_label, "reg_mask": reg_mask,
            "iou_branch": iou_branch, "redrawn": redrawn}


def import_reference():
    torch.cuda.FloatTensor = torch.FloatTensor
    torch.Tensor.cuda = lambda self, *a, **k: self
    install_easydict()
    sys.path.insert(0, REF)
    from lib.config import cfg
    import lib.utils.loss_utils as loss_utils
    import lib.net.train_functions as train_functions
    return cfg, loss_utils, train_functions


class Precision:
    """float64: the reference's explicit float32 spots (torch.cuda.FloatTensor, Tensor.float) become float64 while it runs"""

    def __init__(self, double):
        self.double = double

    def __enter__(self):
        self.saved = (torch.cuda.FloatTensor, torch.Tensor.float)
        if self.double:
            torch.cuda.FloatTensor = torch.DoubleTensor
            torch.Tensor.float = lambda t, *a, **k: t.double()
        return self

    def __exit__(self, *exc):
        torch.cuda.FloatTensor, torch.Tensor.float = self.saved
        return False


def set_cfg(cfg, rpn_s, rcnn_s):
    """the yaml's loss keys, and the two cases' variations"""
    cfg.RPN.ENABLED, cfg.RCNN.ENABLED, cfg.RPN.FIXED, cfg.LI_FUSION.ENABLED = True, True, False, False
    cfg.RPN.USE_RGB = cfg.RCNN.USE_RGB = False
    cfg.CLS_MEAN_SIZE = np.array([[1.52563191462, 1.62856739989, 3.88311640418]], dtype=np.float32)
    cfg.RPN.LOC_XZ_FINE, cfg.RPN.LOC_SCOPE, cfg.RPN.LOC_BIN_SIZE, cfg.RPN.NUM_HEAD_BIN = True, 3.0, 0.5, 12
    cfg.RPN.LOSS_CLS, cfg.RPN.FG_WEIGHT, cfg.RPN.LOSS_WEIGHT = rpn_s["cls_type"], rpn_s["fg_weight"], [1.0, 1.0]
    cfg.RCNN.LOC_SCOPE, cfg.RCNN.LOC_BIN_SIZE, cfg.RCNN.NUM_HEAD_BIN = 1.5, 0.5, 9
    cfg.RCNN.LOC_Y_BY_BIN, cfg.RCNN.LOC_Y_SCOPE, cfg.RCNN.LOC_Y_BIN_SIZE, cfg.RCNN.SIZE_RES_ON_ROI = False, 0.5, 0.25, False
    cfg.RCNN.LOSS_CLS = rcnn_s["cls_type"]
    cfg.TRAIN.RPN_TRAIN_WEIGHT, cfg.TRAIN.RCNN_TRAIN_WEIGHT, cfg.TRAIN.CE_WEIGHT = 1.0, 1.0, 5.0
    assert rpn_s["iou_type"] == rcnn_s["iou_type"]
    cfg.TRAIN.IOU_LOSS_TYPE = rpn_s["iou_type"]
    cfg.USE_IOU_BRANCH = bool(rcnn_s["use_iou_branch"])


def run_reference(cfg, loss_utils, train_functions, rpn_name, rcnn_name, inputs, double):
    rpn_s, rcnn_s = case_settings(rpn_name), case_settings(rcnn_name)
    set_cfg(cfg, rpn_s, rcnn_s)
    dt = torch.float64 if double else torch.float32
    rp, rc = inputs[rpn_name], inputs[rcnn_name]

    def leaf(a, shape):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dt).view(*shape).requires_grad_(True)
    n_rpn, n_rcnn = ROWS["rpn"], ROWS["rcnn"]
    rpn_cls, rpn_reg = leaf(rp["cls_logit"], (2, n_rpn // 2, 1)), leaf(rp["pred_reg"], (2, n_rpn // 2, -1))
    rcnn_cls, rcnn_reg = leaf(rc["cls_logit"], (n_rcnn, 1)), leaf(rc["pred_reg"], (n_rcnn, -1))
    leaves = {"rpn": [rpn_cls, rpn_reg], "rcnn": [rcnn_cls, rcnn_reg]}
    ret = {"rpn_cls": rpn_cls, "rpn_reg": rpn_reg, "rcnn_cls": rcnn_cls, "rcnn_reg": rcnn_reg,
           "cls_label": torch.from_numpy(rc["cls_label"]), "reg_valid_mask": torch.from_numpy(rc["reg_mask"]),
           "roi_boxes3d": torch.zeros((n_rcnn, 7), dtype=dt), "gt_of_rois": torch.from_numpy(rc["reg_label"]).to(dt),
           "pts_input": torch.zeros((n_rcnn, 1, 3), dtype=dt), "mask_score": torch.zeros((n_rcnn,), dtype=dt),
           "gt_iou": torch.zeros((n_rcnn,), dtype=dt)}
    if rcnn_s["use_iou_branch"]:
        branch = leaf(rc["iou_branch"], (n_rcnn, 1))
        ret["rcnn_iou_branch"] = branch
        leaves["rcnn"].append(branch)

    def loss_func(s):
        return loss_utils.SigmoidFocalClassificationLoss(alpha=s["alpha"], gamma=s["gamma"]) if s["cls_type"] == "SigmoidFocalLoss" \
            else torch.nn.functional.binary_cross_entropy
    model = lambda input_data: ret  # noqa: E731
    model.rpn = types.SimpleNamespace(rpn_cls_loss_func=loss_func(rpn_s))
    model.rcnn_net = types.SimpleNamespace(cls_loss_func=loss_func(rcnn_s))
    data = {"pts_rect": np.zeros((2, 4, 3), np.float32), "pts_features": np.zeros((2, 4, 1), np.float32), "pts_input": np.zeros((2, 4, 3), np.float32),
            "gt_boxes3d": np.zeros((2, 1, 7), np.float32), "rpn_cls_label": rp["cls_label"].reshape(2, -1),
            "rpn_reg_label": (rp["reg_label"].astype(np.float64) if double else rp["reg_label"]).reshape(2, -1, 7)}
    with Precision(double):
        model_fn = train_functions.model_joint_fn_decorator()
        result = model_fn(model, data)
        result.loss.backward()
    scalars = {}
    for d in (result.tb_dict, result.disp_dict):
        for k, v in d.items():
            scalars[k] = float(v)
    scalars["loss"] = float(result.loss)
    grads = {st: [np.zeros(t.shape) if t.grad is None else t.grad.numpy().copy() for t in ts] for st, ts in leaves.items()}
    return scalars, grads, sorted(result.tb_dict), sorted(result.disp_dict)


def bound(x64, x32):
    x64, x32 = np.asarray(x64, np.float64), np.asarray(x32, np.float64)
    if x64.size == 0:
        return 0.0
    return max(4 * float(np.abs(x32 - x64).max()), 1e-6 * float(np.abs(x64).max()))


def main():
    assert os.path.isdir(REF), "needs the reference checkout"
    cfg, loss_utils, train_functions = import_reference()
    names = list(CASES)
    inputs = {n: make_inputs(n, 1000 + i) for i, n in enumerate(names)}
    rpn_names = [n for n in names if CASES[n][0] == "rpn"]
    rcnn_names = [n for n in names if CASES[n][0] == "rcnn"]

    def partner(name, pool):
        return next(n for n in pool if CASES[n][2] == CASES[name][2])
    out = {"cases": np.array(names)}
    for name in names:
        stage = CASES[name][0]
        pair = (name, partner(name, rcnn_names)) if stage == "rpn" else (partner(name, rpn_names), name)
        runs = {}
        for double in (True, False):
            scalars, grads, tb_keys, disp_keys = run_reference(cfg, loss_utils, train_functions, pair[0], pair[1], inputs, double)
            runs[double] = (scalars, grads[stage])
        inp = inputs[name]
        pre = name + "__"
        out[pre + "cls_logit"], out[pre + "pred_reg_f16"] = inp["cls_logit"], inp["pred_reg"].astype(np.float16)
        out[pre + "reg_label"], out[pre + "cls_label"] = inp["reg_label"], inp["cls_label"].astype(np.int32)
        if inp["reg_mask"] is not None:
            out[pre + "reg_mask"] = inp["reg_mask"].astype(np.int32)
        if inp["iou_branch"] is not None:
            out[pre + "iou_branch"] = inp["iou_branch"]
        out[pre + "redrawn"] = np.int64(inp["redrawn"])
        # the scalars of this stage: the stage's own keys, the shared reg_loss_dict entries (written by the RCNN stage only) and,
        # for the RCNN stage, the quirk key 'rpn_loss_cls_pos / neg' its focal branch writes (train_functions.py:199-200)
        own = "rpn" if stage == "rpn" else "rcnn"
        keep = [k for k in runs[True][0] if k.startswith(own) or (stage == "rcnn" and not k.startswith("rpn") and k != "loss")]
        if stage == "rcnn" and CASES[name][3] == "SigmoidFocalLoss":
            keep += ["rpn_loss_cls_pos", "rpn_loss_cls_neg"]
        if stage == "rpn" and CASES[name][3] != "SigmoidFocalLoss":
            keep = [k for k in keep if k not in ("rpn_loss_cls_pos", "rpn_loss_cls_neg")]   # (the partner RCNN case's, see above)
        keep = sorted(set(keep))
        out[pre + "scalar_names"] = np.array(keep)
        out[pre + "scalars_f64"] = np.array([runs[True][0][k] for k in keep], np.float64)
        out[pre + "scalars_f32"] = np.array([runs[False][0][k] for k in keep], np.float32)
        out[pre + "scalars_bound"] = np.array([bound(runs[True][0][k], runs[False][0][k]) for k in keep], np.float64)
        out[pre + "tb_keys"], out[pre + "disp_keys"] = np.array(tb_keys), np.array(disp_keys)
        for label, g64, g32 in zip(("grad_cls", "grad_reg", "grad_iou_branch"), runs[True][1], runs[False][1]):
            g64, g32 = g64.reshape(ROWS[stage], -1), g32.reshape(ROWS[stage], -1)
            out[pre + label + "_f64"], out[pre + label + "_f32"] = g64, g32.astype(np.float32)
            out[pre + label + "_bound"] = np.float64(bound(g64, g32))
        print("%-18s fg %3d redrawn %d  loss %.6f  bounds: grad_reg %.2e grad_cls %.2e" % (
            name, int((inp["cls_label"] > 0).sum() if inp["reg_mask"] is None else inp["reg_mask"].sum()), inp["redrawn"],
            runs[True][0][own + "_loss"], out[pre + "grad_reg_bound"], out[pre + "grad_cls_bound"]))
    path = os.path.join(HERE, "loss.npz")
    np.savez_compressed(path, **out)
    print("wrote loss.npz", os.path.getsize(path), "bytes")
    return out


if __name__ == "__main__":
    main()

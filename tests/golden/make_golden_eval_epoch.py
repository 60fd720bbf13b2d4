"""Regenerates tests/golden/eval_epoch.npz. Runs ONLY where the reference checkout exists (see make_golden_rcnn.py, whose import
shims this script reuses); the fixture is plain data: arrays and the written text lines.

What runs is the REFERENCE'S OWN Python, imported unmodified at run time: ``kitti_utils.boxes3d_to_corners3d``,
``Calibration.corners3d_to_img_boxes`` (a Calibration built from a dict) and ``iou3d_utils.boxes_iou3d_gpu`` (on the CPU over the
oracle-backed extension stand-ins, tests/oracle_ext.py), driven the way tools/eval_rcnn.py:76-101 (save_kitti_format) and
:598-632 (the recall and RPN-IoU bookkeeping of eval_one_epoch_joint) drive them, with the summary of :706-734, over 4 scenes of
48 boxes in two batches of two.

The generator redraws until, and ASSERTS that, the fixture is a fair yardstick: no gt-max IoU lies within 3e-4 of a threshold
(B_IOU3D of tests/exact_geometry.py: the oracle's IoU against the kernel's) and no clipped image-box width or height lies
within 1e-2 px of its 0.8 bound (the reference projects in float64, the package in float32).
"""
import os
import sys
import tempfile

import numpy as np
import torch

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_rcnn as base  # noqa: E402  (path set-up, easydict / extension stand-ins, scene_boxes)

THRESH_LIST = [0.1, 0.3, 0.5, 0.7, 0.9]
IOU_CLEARANCE, FILTER_CLEARANCE = 3e-4, 1e-2
P2 = np.array([[721.5, 0.0, 609.6, 44.9], [0.0, 721.5, 172.9, 0.22], [0.0, 0.0, 1.0, 0.0027]], np.float32)
IMG_SHAPE = (375, 1242)
CLASSES = "Car"


def draw(seed):
    """4 scenes x 48 boxes: ground truth (12 rows, zero-padded), refined boxes and ROIs scattered around it, detections"""
    rng = np.random.RandomState(seed)
    b, m, g, n = 4, 48, 12, 512
    gt = np.zeros((b, g, 7), np.float32)
    pred, rois = np.zeros((b, m, 7), np.float32), np.zeros((b, m, 7), np.float32)
    for k in range(b):
        objects = base._np(base.scene_boxes(9, 9, seed + 17 * k)[0])[:9]
        gt[k, :9] = objects
        pick = rng.randint(0, 9, m)
        pred[k] = objects[pick] + rng.normal(0, 1, (m, 7)).astype(np.float32) * np.array([0.3, 0.08, 0.3, 0.08, 0.08, 0.2, 0.12], np.float32)
        rois[k] = pred[k] + rng.normal(0, 1, (m, 7)).astype(np.float32) * np.array([0.4, 0.1, 0.4, 0.1, 0.1, 0.3, 0.2], np.float32)
        far = rng.rand(m) < 0.25
        pred[k, far, 0] += 30.0
    gt[1] = 0                                   # scene 1: no ground truth
    gt[2, 0:3] = 0                              # scene 2: zero rows in front of a gt row
    det = pred.copy()
    det_scores = rng.normal(0, 2, (b, m)).astype(np.float32)
    det[:, 5::8, 2] = -np.abs(det[:, 5::8, 2])                      # behind the camera
    det[:, 6::8, 2] = rng.uniform(1.2, 2.2, det[:, 6::8, 2].shape)  # close and across the view: fails the 0.8 filter
    det[:, 6::8, 0] = rng.uniform(-1.0, 1.0, det[:, 6::8, 0].shape)
    det[:, 6::8, 6] = rng.uniform(-0.2, 0.2, det[:, 6::8, 6].shape)
    det_count = np.array([30, 48, 17, 0], np.int32)
    for k in range(b):
        det[k, det_count[k]:] = 0
        det_scores[k, det_count[k]:] = 0
    seg = (rng.rand(b, n) < 0.4).astype(np.int64)
    label = rng.randint(-1, 2, (b, n)).astype(np.int64)
    p2 = np.stack([P2 * np.float32(1 + 0.01 * k) for k in range(b)]).astype(np.float32)
    shape = np.array([[IMG_SHAPE[0] - 5 * k, IMG_SHAPE[1] - 7 * k] for k in range(b)], np.int32)
    return dict(gt_boxes3d=gt, pred_boxes3d=pred, rois=rois, det_boxes3d=det, det_scores=det_scores, det_count=det_count,
                seg_result=seg, rpn_cls_label=label, P2=p2, img_shape=shape, sample_ids=np.array([11, 12, 25, 26], np.int64))


def run_reference(d, out_dir):
    """the reference's functions in the reference's order; returns the fixture's outputs or None when a clearance fails"""
    import lib.utils.iou3d.iou3d_utils as iou3d_utils
    import lib.utils.kitti_utils as kitti_utils
    from lib.utils.calibration import Calibration
    b, m = d["det_scores"].shape
    g = d["gt_boxes3d"].shape[1]
    out = {"num_gt": np.zeros(b, np.int32), "recalled": np.zeros((b, 5), np.int32), "roi_recalled": np.zeros((b, 5), np.int32),
           "gt_max_iou": np.zeros((b, g), np.float32), "gt_max_iou_in": np.zeros((b, g), np.float32),
           "refined_iou": np.zeros((b, m), np.float32), "img_boxes": np.zeros((b, m, 4), np.float64),
           "valid": np.zeros((b, m), np.int32), "alpha": np.zeros((b, m), np.float64), "seg_counts": np.zeros((2, 3), np.int64)}
    total_recalled, total_roi_recalled, total_gt, total_rpn_iou, cnt, final_total = [0] * 5, [0] * 5, 0, 0.0, 0, 0
    lines = []
    for first in (0, 2):                                      # two batches of two scenes
        cnt += 1
        sl = slice(first, first + 2)
        seg_result = torch.from_numpy(d["seg_result"][sl])
        rpn_cls_label = torch.from_numpy(d["rpn_cls_label"][sl])
        for k in range(first, first + 2):
            cur = d["gt_boxes3d"][k]                          # :598-625
            idx = len(cur) - 1
            while idx >= 0 and cur[idx].sum() == 0:
                idx -= 1
            if idx >= 0:
                cur_t = torch.from_numpy(cur[:idx + 1]).float()
                iou3d = iou3d_utils.boxes_iou3d_gpu(torch.from_numpy(d["pred_boxes3d"][k]), cur_t)
                gt_max_iou, _ = iou3d.max(dim=0)
                refined_iou, _ = iou3d.max(dim=1)
                iou3d_in = iou3d_utils.boxes_iou3d_gpu(torch.from_numpy(d["rois"][k]), cur_t)
                gt_max_iou_in, _ = iou3d_in.max(dim=0)
                for t, thresh in enumerate(THRESH_LIST):
                    out["recalled"][k, t] = (gt_max_iou > thresh).sum().item()
                    out["roi_recalled"][k, t] = (gt_max_iou_in > thresh).sum().item()
                    total_recalled[t] += int(out["recalled"][k, t])
                    total_roi_recalled[t] += int(out["roi_recalled"][k, t])
                    if min(abs(float(v) - thresh) for v in torch.cat([gt_max_iou, gt_max_iou_in])) <= IOU_CLEARANCE:
                        return None
                total_gt += cur_t.shape[0]
                out["num_gt"][k] = cur_t.shape[0]
                out["gt_max_iou"][k, :idx + 1], out["gt_max_iou_in"][k, :idx + 1] = base._np(gt_max_iou), base._np(gt_max_iou_in)
                out["refined_iou"][k] = base._np(refined_iou)
            fg = rpn_cls_label > 0                            # :627-632, on the whole batch tensor, once per scene
            correct = (fg & (seg_result == rpn_cls_label)).sum().float()
            union = fg.sum().float() + (seg_result > 0).sum().float() - correct
            total_rpn_iou += (correct / torch.clamp(union, min=1.0)).item()
            out["seg_counts"][first // 2] = [int(correct), int(fg.sum()), int((seg_result > 0).sum())]
        for k in range(first, first + 2):                     # :668-690 from the detections on
            n = int(d["det_count"][k])
            if n == 0:
                lines.append(np.array([], dtype="U1"))
                continue
            bbox3d, scores, img_shape = d["det_boxes3d"][k, :n], d["det_scores"][k, :n], d["img_shape"][k]
            final_total += n
            calib = Calibration({"P2": d["P2"][k], "R0": np.eye(3, dtype=np.float32), "Tr_velo2cam": np.zeros((3, 4), np.float32)})
            corners3d = kitti_utils.boxes3d_to_corners3d(bbox3d)                                  # :77-87
            img_boxes, _ = calib.corners3d_to_img_boxes(corners3d)
            for col, hi in ((0, img_shape[1] - 1), (1, img_shape[0] - 1), (2, img_shape[1] - 1), (3, img_shape[0] - 1)):
                img_boxes[:, col] = np.clip(img_boxes[:, col], 0, hi)
            img_boxes_w, img_boxes_h = img_boxes[:, 2] - img_boxes[:, 0], img_boxes[:, 3] - img_boxes[:, 1]
            box_valid_mask = (img_boxes_w < img_shape[1] * 0.8) & (img_boxes_h < img_shape[0] * 0.8)
            if min(np.abs(img_boxes_w - img_shape[1] * 0.8).min(), np.abs(img_boxes_h - img_shape[0] * 0.8).min()) <= FILTER_CLEARANCE:
                return None
            path = os.path.join(out_dir, "%06d.txt" % d["sample_ids"][k])
            with open(path, "w") as f:                                                            # :89-101
                for j in range(bbox3d.shape[0]):
                    x, z, ry = bbox3d[j, 0], bbox3d[j, 2], bbox3d[j, 6]
                    beta = np.arctan2(z, x)
                    alpha = -np.sign(beta) * np.pi / 2 + beta + ry
                    out["alpha"][k, j] = alpha
                    if box_valid_mask[j] == 0:
                        continue
                    fields = (alpha,) + tuple(img_boxes[j]) + tuple(bbox3d[j, [3, 4, 5, 0, 1, 2, 6]]) + (scores[j],)
                    f.write("%s -1 -1 " % CLASSES + " ".join("%.4f" % v for v in fields) + "\n")
            out["img_boxes"][k, :n], out["valid"][k, :n] = img_boxes, box_valid_mask
            lines.append(np.array([line.rstrip("\n") for line in open(path)]))
    ret = {"empty_cnt": int((d["det_count"] == 0).sum()), "rpn_iou": total_rpn_iou / max(cnt, 1.0), "rcnn_cls_acc": 0.0,      # :706-734
           "rcnn_cls_acc_refined": 0.0, "rcnn_avg_num": final_total / max(b, 1.0)}
    for t, thresh in enumerate(THRESH_LIST):
        ret["rpn_recall(thresh=%.2f)" % thresh] = total_roi_recalled[t] / max(total_gt, 1.0)
        ret["rcnn_recall(thresh=%.2f)" % thresh] = total_recalled[t] / max(total_gt, 1.0)
    out["ret_keys"] = np.array(sorted(ret))
    out["ret_values"] = np.array([ret[key] for key in sorted(ret)], np.float64)
    for k in range(b):
        out["lines_%d" % k] = lines[k]
    return out


def main():
    assert os.path.isdir(base.REF), "needs the reference checkout"
    base.import_reference()
    for seed in range(700, 760):
        d = draw(seed)
        with tempfile.TemporaryDirectory() as tmp:
            out = run_reference(d, tmp)
        if out is not None and all(0 < out["valid"][k, :d["det_count"][k]].sum() < d["det_count"][k] for k in (0, 1, 2)):
            break
    else:
        raise AssertionError("no seed with both clearances")
    # ---- what makes the fixture a fair yardstick (tests/test_eval_epoch.py asserts the same from the stored arrays)
    assert out["num_gt"].tolist() == [9, 0, 9, 9] and not d["gt_boxes3d"][2, 0:3].any()
    for key in ("gt_max_iou", "gt_max_iou_in"):
        for k in range(4):
            v = out[key][k, :out["num_gt"][k]]
            assert all(np.abs(v - t).min() > IOU_CLEARANCE for t in THRESH_LIST) if v.size else True
    assert 0 < out["recalled"].sum() and (out["recalled"][:, 0] > out["recalled"][:, 4]).any()
    valid, n = out["valid"], d["det_count"]
    assert all(0 < valid[k, :n[k]].sum() < n[k] for k in (0, 1, 2)) and n[3] == 0
    behind = d["det_boxes3d"][..., 2] < 0
    assert behind.any()
    d.update(out)
    d["thresh_list"] = np.array(THRESH_LIST, np.float64)
    path = os.path.join(HERE, "eval_epoch.npz")
    np.savez_compressed(path, **d)
    print("seed", seed, "wrote eval_epoch.npz", os.path.getsize(path), "bytes; num_gt", out["num_gt"].tolist(), "recalled",
          out["recalled"].tolist(), "valid rows", valid.sum(1).tolist(), "of", n.tolist())
    assert os.path.getsize(path) < 200000


if __name__ == "__main__":
    main()

"""TEST INFRASTRUCTURE: numpy restatement of the sync-free RCNN training targets (include/epnet_ops.h: epnet_rcnn_sample_rois,
epnet_roipool3d_train; reference: lib/rpn/proposal_target_layer.py:16-349). Never imported by the product.

``select`` takes ONE scene's IoU matrix and the draw tables and returns everything step 1 defines before the noise loop: the
maxima, the first arg-max, the class lists, the slots, the try limits. It decides on the float32 values it is given, so a test
that feeds it the matrix of ``boxes_iou3d_gpu`` sees the same floats as the kernel and no ROI is "near a threshold".
``sample`` adds the padding rule and the gather for a batch. ``pool_train`` restates step 2: the oracle's pooling on the enlarged
ROIs picks the rows (exact), the augmentation, the canonical transformation and the labels are float32 arithmetic in the
header's order (``precise=True``: the same formulas in float64, the yardstick of the float32 form).
"""
import numpy as np

from oracle import oracle
from detections_restate import enlarge

F = np.float32
PI = F(np.pi)
TWO_PI = F(2 * np.pi)


# ---- step 1 -----------------------------------------------------------------------------------------------------------------------
def ordered_key(v):
    """float32 -> uint32, order preserving: -0.0 and +0.0 share a key, every NaN sits above +inf"""
    v = np.array(v, F, copy=True).reshape(-1)
    v[v == 0] = 0.0
    u = v.view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    key[np.isnan(v)] = np.uint32(0xFFFFFFFF)
    return key


def count_gt(gt):
    """gt (G,gc) float32 -> 1 + the last row whose float32 sum over all columns, ascending, is not 0 (0 without one)"""
    gt = np.asarray(gt, F)
    total = np.zeros(gt.shape[0], F)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(gt.shape[1]):
            total = (total + gt[:, c]).astype(F)
    nz = np.nonzero(total != 0)[0]
    return int(nz[-1]) + 1 if nz.size else 0


def pick_pos(u, length):
    with np.errstate(invalid="ignore", over="ignore"):
        p = F(u) * F(length)
    if not (p >= 0):
        return 0
    return length - 1 if p >= F(length) else int(p)


def row_max_first(row):
    """the maximum and the first column that reaches it; a NaN wins over every number and the first one stays"""
    best, arg = row[0], 0
    for j in range(1, len(row)):
        v = row[j]
        if v > best or (np.isnan(v) and not np.isnan(best)):
            best, arg = v, j
    return best, arg


def select(iou, fg_key, slot_u, per_image, fg_per_image, fg_thresh, bg_thresh, bg_thresh_lo, hard_bg_ratio, aug_times):
    """iou (M, num_gt) float32 (columns = the ground-truth rows that count), fg_key (M), slot_u (R) -> dict"""
    iou, fg_key, slot_u = np.asarray(iou, F), np.asarray(fg_key, F), np.asarray(slot_u, F)
    m = iou.shape[0]
    if iou.shape[1] <= 64 and not np.isnan(iou).any():
        ov, assign = iou.max(axis=1), iou.argmax(axis=1).astype(np.int32)     # numpy's argmax is the first maximum
    else:
        pairs = [row_max_first(r) for r in iou]
        ov, assign = np.array([p[0] for p in pairs], F), np.array([p[1] for p in pairs], np.int32)
    with np.errstate(invalid="ignore"):
        fg = np.nonzero(ov >= F(fg_thresh))[0]
        easy = np.nonzero(ov < F(bg_thresh_lo))[0]
        hard = np.nonzero((ov < F(bg_thresh)) & (ov >= F(bg_thresh_lo)))[0]
    fg_num, bg_num = fg.size, hard.size + easy.size
    src = np.empty(per_image, np.int32)

    def background(first):
        slots = per_image - first
        hard_slots = int(slots * float(hard_bg_ratio))
        for j in range(first, per_image):
            if hard.size and easy.size:
                lst = hard if j - first < hard_slots else easy
            else:
                lst = hard if hard.size else easy
            src[j] = lst[pick_pos(slot_u[j], lst.size)]

    if fg_num and bg_num:
        case, fg_this = 0, min(fg_per_image, fg_num)
        keys = ordered_key(fg_key[fg]).astype(np.uint64) << np.uint64(32) | fg.astype(np.uint64)
        src[:fg_this] = fg[np.argsort(keys, kind="stable")[:fg_this]]
        background(fg_this)
    elif fg_num:
        case, fg_this = 1, per_image
        for j in range(per_image):
            src[j] = fg[pick_pos(slot_u[j], fg_num)]
    elif bg_num:
        case, fg_this = 2, 0
        background(0)
    else:
        case, fg_this = 3, 0
        for j in range(per_image):
            src[j] = pick_pos(slot_u[j], m)
    tries = np.where(np.arange(per_image) < fg_this, aug_times, 1 if aug_times > 0 else 0).astype(np.int32)
    return {"max_overlaps": ov.astype(F), "gt_assignment": assign, "src_inds": src, "tries": tries, "fg_this": fg_this, "case": case,
            "counts": (fg_num, hard.size, easy.size), "iou_src": ov.astype(F)[src]}


def sample(rois, gt, iou_of, fg_key, slot_u, per_image, fg_per_image, fg_thresh, bg_thresh, bg_thresh_lo, hard_bg_ratio, aug_times):
    """a batch: rois (B,M,7), gt (B,G,gc); iou_of(scene, num_gt) -> (M, num_gt) float32 IoU matrix of that scene's ROIs against
    its first num_gt ground-truth rows -> dict of stacked arrays (the state BEFORE the noise loop)"""
    rois, gt = np.asarray(rois, F), np.asarray(gt, F)
    out = {k: [] for k in ("max_overlaps", "gt_assignment", "src_inds", "tries", "iou_src", "scene_info", "batch_rois", "batch_gt_of_rois")}
    for b in range(rois.shape[0]):
        counted = count_gt(gt[b])
        num_gt = max(counted, 1)
        s = select(iou_of(b, num_gt), fg_key[b], slot_u[b], per_image, fg_per_image, fg_thresh, bg_thresh, bg_thresh_lo, hard_bg_ratio, aug_times)
        for k in ("max_overlaps", "gt_assignment", "src_inds", "tries", "iou_src"):
            out[k].append(s[k])
        out["scene_info"].append(np.array([counted, *s["counts"], s["fg_this"], s["case"]], np.int32))
        out["batch_rois"].append(rois[b][s["src_inds"]])
        out["batch_gt_of_rois"].append(gt[b][s["gt_assignment"][s["src_inds"]]][:, 0:7])
    return {k: np.stack(v) for k, v in out.items()}


# ---- step 2 -----------------------------------------------------------------------------------------------------------------------
def _trig(a, T):
    a64 = np.asarray(a, np.float64)
    return np.cos(a64).astype(T), np.sin(a64).astype(T)


def _atan2(y, x, T):
    return np.arctan2(np.asarray(y, np.float64), np.asarray(x, np.float64)).astype(T)


def augment_boxes(boxes, aug, T=F):
    """data_augmentation's box rules (:305-347) on boxes (K,7) with aug (K,3) = [angle, scale, flip], in the header's order"""
    b = np.array(boxes, T, copy=True)
    pi = T(PI)
    ca, sa = _trig(np.asarray(aug, F)[:, 0], T)
    scale, flip = np.asarray(aug, F)[:, 1].astype(T), np.asarray(aug, F)[:, 2].astype(T)
    beta = _atan2(b[:, 2], b[:, 0], T)
    alpha = ((-np.sign(beta) * pi) / T(2) + beta) + b[:, 6]
    x = b[:, 0] * ca + b[:, 2] * (-sa)
    z = b[:, 0] * sa + b[:, 2] * ca
    b[:, 0], b[:, 2] = x, z
    beta2 = _atan2(z, x, T)
    b[:, 6] = ((np.sign(beta2) * pi) / T(2) + alpha) - beta2
    b[:, 0:6] = b[:, 0:6] * scale[:, None]
    b[:, 0] = b[:, 0] * flip
    keep, mirror = (flip == 1).astype(T), (flip == -1).astype(T)
    b[:, 6] = keep * b[:, 6] + mirror * (np.sign(b[:, 6]) * pi - b[:, 6])
    return b


def pool_train(xyz, pts_feature, rois, gt_of_rois, roi_iou, aug, extra, reg_fg, cls_fg, cls_bg, num_points, precise=False):
    """xyz (B,N,3), pts_feature (B,N,C), rois / gt_of_rois (B,R,7), roi_iou (B,R), aug (B,R,3) or None -> dict of the eight
    outputs of epnet_roipool3d_train; the integer outputs and the choice of rows do not depend on `precise`"""
    T = np.float64 if precise else F
    xyz, feat, rois = np.asarray(xyz, F), np.asarray(pts_feature, F), np.asarray(rois, F)
    b, r, s, c = rois.shape[0], rois.shape[1], int(num_points), feat.shape[2]
    pooled, flag = oracle.roipool3d(xyz, enlarge(rois, extra), feat, s)              # (B,R,S,3+C), zero rows where empty
    k = b * r
    p = pooled[..., 0:3].reshape(k, s, 3).astype(T)
    a_roi, a_gt = rois.reshape(k, 7).astype(T), np.asarray(gt_of_rois, F).reshape(k, 7).astype(T)
    if aug is not None:
        aug = np.asarray(aug, F).reshape(k, 3)
        a_roi, a_gt = augment_boxes(a_roi, aug, T), augment_boxes(a_gt, aug, T)
        ca, sa = (v[:, None] for v in _trig(aug[:, 0], T))
        scale, flip = aug[:, 1].astype(T)[:, None], aug[:, 2].astype(T)[:, None]
        x1 = p[..., 0] * ca + p[..., 2] * (-sa)
        z1 = p[..., 0] * sa + p[..., 2] * ca
        p = np.stack([(x1 * scale) * flip, p[..., 1] * scale, z1 * scale], axis=2)
    d = p - a_roi[:, None, 0:3]
    c2, s2 = (v[:, None] for v in _trig(a_roi[:, 6], T))
    pts = np.stack([d[..., 0] * c2 + d[..., 2] * (-s2), d[..., 1], d[..., 0] * s2 + d[..., 2] * c2], axis=2)
    two_pi = T(TWO_PI)
    ry_mod = np.fmod(a_roi[:, 6], two_pi)
    ry_mod = np.where((ry_mod != 0) & (ry_mod < 0), ry_mod + two_pi, ry_mod).astype(T)
    cm, sm = _trig(ry_mod, T)
    e = a_gt[:, 0:3] - a_roi[:, 0:3]
    gt_out = np.concatenate([np.stack([e[:, 0] * cm + e[:, 2] * (-sm), e[:, 1], e[:, 0] * sm + e[:, 2] * cm], axis=1), a_gt[:, 3:6],
                             (a_gt[:, 6] - ry_mod)[:, None]], axis=1)
    iou = np.asarray(roi_iou, F).reshape(k)
    valid = flag.reshape(k) == 0
    with np.errstate(invalid="ignore"):
        cls = (iou > F(cls_fg)).astype(np.int32)
        cls[(iou > F(cls_bg)) & (iou < F(cls_fg))] = -1
        cls[~valid] = -1
        reg_valid = ((iou > F(reg_fg)) & valid).astype(np.int32)
    feats = pooled[..., 3:].reshape(k, s, c)
    mask = (feats[..., 0].astype(np.float64).sum(axis=1) / s) if c else np.zeros(k)
    return {"sampled_pts": pts, "pts_feature": feats, "roi_boxes3d": a_roi, "gt_of_rois": gt_out, "cls_label": cls,
            "reg_valid_mask": reg_valid, "mask_score": mask, "pooled_empty_flag": flag.astype(np.int32)}

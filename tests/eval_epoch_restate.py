"""TEST INFRASTRUCTURE: numpy restatements of epnet_eval_recall and epnet_kitti_records -- elementwise float32 in the order the
contract of include/epnet_ops.h gives (no np.matmul; trigonometry through float64, rounded once) -- plus CPU stand-ins for
`iou3d_cuda.eval_recall_gpu` / `iou3d_cuda.kitti_records_gpu`, so that epnet_amd.eval_epoch runs on CPU tensors, and the seeded
case generators of tests/test_eval_epoch_gpu.py. The recall restatement TAKES the two IoU matrices (as
tests/rcnn_targets_restate.py does): it sees the floats the kernel sees. Never imported by the product.
"""
import numpy as np
import torch

F = np.float32
PI = F(3.14159265358979323846)

# synthetic KITTI calibration and image size
P2_KITTI = np.array([[721.5, 0.0, 609.6, 44.9], [0.0, 721.5, 172.9, 0.22], [0.0, 0.0, 1.0, 0.0027]], F)
IMG_KITTI = (375, 1242)


def r4(v):
    """the float64 that '%.4f' % v parses back to (csrc/r4.h), elementwise on a float32 array"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.rint(np.asarray(v, F).astype(np.float64) * 1e4) / 1e4


def count_gt(gt):
    """gt (g,gc) -> 1 + the last row whose float32 sum over all columns, in ascending column order, is not 0; 0 without one"""
    gt = np.asarray(gt, F)
    last = 0
    for r in range(gt.shape[0]):
        s = F(0)
        with np.errstate(invalid="ignore", over="ignore"):
            for c in range(gt.shape[1]):
                s = F(s + gt[r, c])
        if s != 0:          # a NaN sum is not 0
            last = r + 1
    return last


def nan_max(a, axis):
    """np.max propagates a NaN already; spelled out for the reader"""
    with np.errstate(invalid="ignore"):
        return np.max(a, axis=axis)


def eval_recall(iou_pred, iou_roi, gt_boxes3d, thresholds, seg_result=None, rpn_cls_label=None):
    """iou_pred / iou_roi (b,m,g) float32: IoU of every box with every gt ROW (only the columns below num_gt are read; iou_roi
    may be None) -> scene_stats (b, 1 + 2 nt) int32, seg_counts (3) int64 or None, gt_max_pred, gt_max_roi (b,g), pred_max_iou
    (b,m)"""
    gt = np.asarray(gt_boxes3d, F)
    b, g = gt.shape[0], gt.shape[1]
    m = iou_pred.shape[1]
    thr = [F(t) for t in thresholds]
    nt = len(thr)
    stats = np.zeros((b, 1 + 2 * nt), np.int32)
    gmp, gmr, pmi = np.zeros((b, g), F), np.zeros((b, g), F), np.zeros((b, m), F)
    for k in range(b):
        num_gt = count_gt(gt[k])
        stats[k, 0] = num_gt
        if num_gt == 0:
            continue
        gmp[k, :num_gt] = nan_max(iou_pred[k][:, :num_gt], 0)
        pmi[k] = nan_max(iou_pred[k][:, :num_gt], 1)
        if iou_roi is not None:
            gmr[k, :num_gt] = nan_max(iou_roi[k][:, :num_gt], 0)
        with np.errstate(invalid="ignore"):
            for t in range(nt):
                stats[k, 1 + t] = int((gmp[k, :num_gt] > thr[t]).sum())
                stats[k, 1 + nt + t] = int((gmr[k, :num_gt] > thr[t]).sum()) if iou_roi is not None else 0
    seg = None
    if seg_result is not None:
        s, l = np.asarray(seg_result), np.asarray(rpn_cls_label)
        seg = np.array([((l > 0) & (s == l)).sum(), (l > 0).sum(), (s > 0).sum()], np.int64)
    return stats, seg, gmp, gmr, pmi


def image_boxes(boxes3d, P2, img_shape):
    """boxes3d (n,7), P2 (3,4), img_shape (h, w) -> clipped image boxes (n,4) float32, valid (n) bool, alpha (n) float32"""
    bx = np.asarray(boxes3d, F).reshape(-1, 7)
    P = np.asarray(P2, F)
    x, y, z, h, w, l, ry = (bx[:, q] for q in range(7))
    with np.errstate(all="ignore"):
        c = np.cos(ry.astype(np.float64)).astype(F)
        s = np.sin(ry.astype(np.float64)).astype(F)
        hl, hw = l / F(2), w / F(2)
        xc = np.stack([hl, hl, -hl, -hl, hl, hl, -hl, -hl], 1)
        zc = np.stack([hw, -hw, -hw, hw, hw, -hw, -hw, hw], 1)
        zero = np.zeros_like(h)
        yc = np.stack([zero, zero, zero, zero, -h, -h, -h, -h], 1)
        c_, s_ = c[:, None], s[:, None]
        X = x[:, None] + ((xc * c_).astype(F) + (zc * s_).astype(F)).astype(F)
        Y = y[:, None] + yc
        Z = z[:, None] + ((xc * (-s_)).astype(F) + (zc * c_).astype(F)).astype(F)
        p = [(((X * P[r, 0]).astype(F) + (Y * P[r, 1]).astype(F)).astype(F) + (Z * P[r, 2]).astype(F)).astype(F) + P[r, 3] for r in range(3)]
        u, v = (p[0] / p[2]).astype(F), (p[1] / p[2]).astype(F)
        box = np.stack([np.min(u, 1), np.min(v, 1), np.max(u, 1), np.max(v, 1)], 1).astype(F)     # a NaN propagates
        img_h, img_w = int(img_shape[0]), int(img_shape[1])
        box[:, 0] = np.clip(box[:, 0], F(0), F(img_w - 1))
        box[:, 1] = np.clip(box[:, 1], F(0), F(img_h - 1))
        box[:, 2] = np.clip(box[:, 2], F(0), F(img_w - 1))
        box[:, 3] = np.clip(box[:, 3], F(0), F(img_h - 1))
        valid = ((box[:, 2] - box[:, 0]).astype(F) < F(img_w * 0.8)) & ((box[:, 3] - box[:, 1]).astype(F) < F(img_h * 0.8))
        beta = np.arctan2(z.astype(np.float64), x.astype(np.float64)).astype(F)
        alpha = ((((-np.sign(beta)).astype(F) * PI).astype(F) / F(2)).astype(F) + beta).astype(F) + ry
    return box, valid, alpha.astype(F)


def kitti_records(boxes3d, scores, count, P2, img_shape):
    """-> records (b,m,13) float64, rec_count (b) int32, bbox_raw (b,m,4) float32, valid (b,m) int32"""
    boxes3d, scores = np.asarray(boxes3d, F), np.asarray(scores, F)
    b, m = scores.shape
    rec, cnt = np.zeros((b, m, 13), np.float64), np.zeros((b,), np.int32)
    raw, val = np.zeros((b, m, 4), F), np.zeros((b, m), np.int32)
    for k in range(b):
        n = m if count is None else min(max(int(count[k]), 0), m)
        box, valid, alpha = image_boxes(boxes3d[k, :n], P2[k], img_shape[k])
        raw[k, :n], val[k, :n] = box, valid
        bx, sc = boxes3d[k, :n][valid], scores[k, :n][valid]
        rows = np.concatenate([alpha[valid][:, None], box[valid], bx[:, 3:6], bx[:, 0:3], bx[:, 6:7], sc[:, None]], axis=1)
        cnt[k] = rows.shape[0]
        rec[k, :rows.shape[0]] = r4(rows)
    return rec, cnt, raw, val


# ---- CPU stand-ins for the two extension entry points -------------------------------------------------------------------------
def _np(t):
    return t.detach().cpu().numpy()


def _wr(t, arr):
    if t is not None:
        t.copy_(torch.from_numpy(np.ascontiguousarray(arr)).view_as(t))


def iou_matrices(boxes, gt):
    """(b,m,7), (b,g,gc) -> (b,m,g) from the oracle's boxes_iou3d"""
    from oracle import oracle
    boxes, gt = np.asarray(boxes, F), np.asarray(gt, F)
    if gt.shape[1] == 0:
        return np.zeros((boxes.shape[0], boxes.shape[1], 0), F)
    return np.stack([oracle.boxes_iou3d(boxes[k], np.ascontiguousarray(gt[k][:, :7])) for k in range(boxes.shape[0])])


def eval_recall_gpu(pred_boxes3d, roi_boxes3d, gt_boxes3d, thresholds, seg_result, rpn_cls_label, scene_stats, seg_counts=None,
                    totals=None, gt_max_pred=None, gt_max_roi=None, pred_max_iou=None):
    gt = _np(gt_boxes3d)
    iou_p = iou_matrices(_np(pred_boxes3d), gt)
    iou_r = iou_matrices(_np(roi_boxes3d), gt) if roi_boxes3d is not None else None
    stats, seg, gmp, gmr, pmi = eval_recall(iou_p, iou_r, gt, thresholds, None if seg_result is None else _np(seg_result),
                                            None if rpn_cls_label is None else _np(rpn_cls_label))
    _wr(scene_stats, stats)
    _wr(seg_counts, seg)
    _wr(gt_max_pred, gmp)
    _wr(gt_max_roi, gmr)
    _wr(pred_max_iou, pmi)
    if totals is not None:
        totals += torch.from_numpy(stats.astype(np.int64).sum(0))
    return 1


def kitti_records_gpu(boxes3d, scores, count, P2, img_shape, records, rec_count, bbox_raw=None, valid=None):
    rec, cnt, raw, val = kitti_records(_np(boxes3d), _np(scores), None if count is None else _np(count), _np(P2), _np(img_shape))
    _wr(records, rec)
    _wr(rec_count, cnt)
    _wr(bbox_raw, raw)
    _wr(valid, val)
    return 1


def install(monkeypatch):
    from epnet_amd import iou3d_cuda
    monkeypatch.setattr(iou3d_cuda, "eval_recall_gpu", eval_recall_gpu)
    monkeypatch.setattr(iou3d_cuda, "kitti_records_gpu", kitti_records_gpu)


# ---- the GPU sweep's cases (tests/test_eval_epoch_gpu.py) -----------------------------------------------------------------------
REC_M = (1, 63, 64, 65, 100, 257, 4096)
REC_G = (0, 1, 20, 64, 65)
REC_B = (1, 2, 5)
REC_GC = (7, 8, 16)
REC_NT = (1, 5, 8)
SEG_N = (None, 1, 255, 256, 257, 16384)


def recall_cases():
    """(b, m, g, gc, nt, n, with_roi, seed): every listed value of every set at least once; the large m only with small b * g"""
    cases = []
    for i in range(15):
        m, g = REC_M[i % len(REC_M)], REC_G[(i + i // 7) % len(REC_G)]
        b = REC_B[i % len(REC_B)]
        if m == 4096:
            b, g = min(b, 2), (20, 65, 1)[i % 3]
        cases.append((b, m, g, REC_GC[i % len(REC_GC)], REC_NT[(i // 2) % len(REC_NT)], SEG_N[i % len(SEG_N)], i % 4 != 3, 3000 + i))
    return cases


def scene_boxes(m, g, seed):
    """m boxes scattered around g objects and the g ground-truth rows: overlaps of every size"""
    from epnet_amd import synth
    gt = synth.object_boxes(max(g, 1), seed).float()[:g]
    boxes, _ = synth.proposal_boxes(m, seed=seed + 1, num_objects=max(1, min(g, 12)))
    boxes = boxes.float()
    if g:
        rng = np.random.RandomState(seed)
        pick = torch.from_numpy(rng.randint(0, g, size=(m,)))
        near = gt[pick] + torch.from_numpy(rng.normal(0, 0.25, size=(m, 7)).astype(F)) * torch.tensor([1, 0.3, 1, 0.2, 0.2, 0.4, 0.3])
        use = torch.from_numpy(rng.rand(m) < 0.6).view(m, 1)
        boxes = torch.where(use, near, boxes)
    return boxes.contiguous(), gt.contiguous()


def recall_inputs(b, m, g, gc, n, seed):
    """-> pred (b,m,7), roi (b,m,7), gt (b,g,gc), seg (b,n) int32 or None, label (b,n) int32 or None (torch CPU tensors). Scene
    families by scene index mod 5: plain; no gt; leading zero rows; a gt row whose columns cancel to 0 in float32 (+ extra columns
    where gc > 7); a gt identical to a box, a NaN box, and (m >= 4, g >= 2)
    a box / gt pair whose IoU is NaN"""
    rng = np.random.RandomState(seed)
    pred, roi, gts = [], [], []
    for k in range(b):
        p, gt = scene_boxes(m, g, seed + 10 * k)
        r = p + torch.from_numpy(rng.normal(0, 0.15, size=(m, 7)).astype(F))
        full = torch.zeros((g, gc))
        full[:, :7] = gt
        if gc > 7:
            full[:, 7:] = torch.from_numpy(rng.rand(g, gc - 7).astype(F))
        fam = (k + seed) % 5
        if fam == 1:
            full.zero_()
        elif fam == 2 and g >= 2:
            full[:max(1, g // 3)] = 0
            full[g - 1] = 0                      # and a padding row behind
        elif fam == 3 and g >= 2:
            row = torch.zeros((gc,))
            row[:7] = torch.tensor([8.0, 1.5, -8.0, 1.5, 1.5, -3.0, -1.5])      # sums to exactly 0: not a box row when it is last
            full[g - 1] = row
        elif fam == 4 and g >= 1:
            p[m // 2] = full[0, :7]
            if m >= 2:
                p[0] = float("nan")
                r[m - 1, 3] = float("nan")
            if m >= 4 and g >= 2:
                # a NaN IoU: box 1 and the last gt row both of infinite height with disjoint footprints -- BEV overlap 0 times
                # height overlap inf; every other pair of either stays a number
                p[1] = torch.tensor([500.0, 1.6, 20.0, float("inf"), 1.6, 3.9, 0.3])
                r[1] = p[1]
                full[g - 1, :7] = torch.tensor([-500.0, 1.6, 20.0, float("inf"), 1.6, 3.9, -0.2])
        pred.append(p)
        roi.append(r)
        gts.append(full)
    seg = label = None
    if n is not None:
        seg = torch.from_numpy(rng.randint(0, 2, size=(b, n)).astype(np.int32))
        label = torch.from_numpy(rng.randint(-1, 2, size=(b, n)).astype(np.int32))
    return torch.stack(pred).contiguous(), torch.stack(roi).contiguous(), torch.stack(gts).contiguous(), seg, label


KR_M = (1, 63, 64, 65, 100, 4096)


def records_cases():
    """(b, m, count mode, seed): every m with count 0, 1, m and NULL, and a count drawn per scene"""
    modes = ("zero", "one", "full", "none", "mixed")
    return [((1, 2, 3)[(i + j) % 3] if m < 4096 else 1 + j % 2, m, mode, 4000 + 10 * i + j) for i, m in enumerate(KR_M) for j, mode in enumerate(modes)]


def records_inputs(b, m, mode, seed):
    """-> boxes3d (b,m,7), scores (b,m), count (b) int32 or None, P2 (b,3,4), img_shape (b,2) int32. Row families by row index mod
    8: in front of the camera (valid), behind it, straddling Z = 0, wider than 0.8 of the image, NaN, ry at +-pi / +-pi/2, x = 0 and
    z = 0; each scene with its own P2 and image size"""
    rng = np.random.RandomState(seed)
    boxes = np.zeros((b, m, 7), F)
    boxes[..., 0] = rng.uniform(-15, 15, (b, m))
    boxes[..., 1] = rng.uniform(0.8, 2.2, (b, m))
    boxes[..., 2] = rng.uniform(8, 60, (b, m))
    boxes[..., 3:6] = np.array([1.5, 1.6, 3.9], F) * rng.uniform(0.8, 1.2, (b, m, 3))
    boxes[..., 6] = rng.uniform(-np.pi, np.pi, (b, m))
    i = np.arange(m)
    fam = i % 8
    if m >= 128:                          # valid rows on both sides of the wave boundaries
        fam[[0, 63, 64, 127]] = 0
    boxes[:, fam == 1, 2] = -boxes[:, fam == 1, 2]
    boxes[:, fam == 2, 2] = rng.uniform(-1.0, 1.0, (b, int((fam == 2).sum())))
    boxes[:, fam == 3, 2] = rng.uniform(1.2, 2.2, (b, int((fam == 3).sum())))      # close and across the view
    boxes[:, fam == 3, 0] = rng.uniform(-0.3, 0.3, (b, int((fam == 3).sum())))
    boxes[:, fam == 3, 6] = rng.uniform(-0.2, 0.2, (b, int((fam == 3).sum())))
    boxes[:, fam == 4, rng.randint(0, 7)] = np.nan
    boxes[:, fam == 5, 6] = np.array([np.pi, -np.pi, np.pi / 2, -np.pi / 2], F)[rng.randint(0, 4, int((fam == 5).sum()))]
    boxes[:, fam == 6, 0] = 0.0
    boxes[:, fam == 7, 2] = np.where(rng.rand(b, int((fam == 7).sum())) < 0.5, 0.0, boxes[:, fam == 7, 2])
    scores = rng.normal(0, 2, (b, m)).astype(F)
    P2 = np.stack([P2_KITTI * (1 + F(0.01) * k) for k in range(b)]).astype(F)
    shape = np.array([[IMG_KITTI[0] - 5 * k, IMG_KITTI[1] - 7 * k] for k in range(b)], np.int32)
    count = {"zero": np.zeros(b), "one": np.ones(b), "full": np.full(b, m), "none": None,
             "mixed": rng.randint(0, m + 1, b)}[mode]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))   # noqa: E731
    return T(boxes), T(scores), None if count is None else T(count.astype(np.int32)), T(P2), T(shape)

"""numpy restatement of the reference's KITTI AP evaluator (tools/kitti_object_eval_python/eval.py, rotate_iou.py), written from
their text: the three overlap functions (float32 where the reference has float32), the literal matching loops of
compute_statistics_jit, get_thresholds, eval_class over per-frame blocks and the official result. The kernels of
epnet_amd/csrc/kitti_eval.hip are tested against this file; this file is held to the reference's own run by
tests/golden/kitti_eval.npz (tests/test_kitti_eval.py)."""
import math

import numpy as np

F32 = np.float32
NO_DETECTION = -10000000
OFFICIAL_MIN_OVERLAPS = (0.7, 0.5, 0.25)
POLY_PTS = 8   # rotate_iou.py:236 has room for 8 points; a ninth is dropped (the reference would write past its array)


# ---- overlaps -----------------------------------------------------------------------------------------------------------------
def image_box_overlap(boxes, query_boxes, criterion=-1):
    """eval.py:85-111, float64"""
    n, k = boxes.shape[0], query_boxes.shape[0]
    out = np.zeros((n, k), np.float64)
    for kk in range(k):
        q = query_boxes[kk]
        qbox_area = (q[2] - q[0]) * (q[3] - q[1])
        for nn in range(n):
            b = boxes[nn]
            iw = min(b[2], q[2]) - max(b[0], q[0])
            if iw > 0:
                ih = min(b[3], q[3]) - max(b[1], q[1])
                if ih > 0:
                    if criterion == -1:
                        ua = (b[2] - b[0]) * (b[3] - b[1]) + qbox_area - iw * ih
                    elif criterion == 0:
                        ua = (b[2] - b[0]) * (b[3] - b[1])
                    elif criterion == 1:
                        ua = qbox_area
                    else:
                        ua = 1.0
                    out[nn, kk] = iw * ih / ua
    return out


def _corners(rbbox):
    """rbbox_to_corners, rotate_iou.py:205-229; cos / sin correctly rounded to float32"""
    a_cos, a_sin = F32(math.cos(float(rbbox[4]))), F32(math.sin(float(rbbox[4])))
    cx0, cy0, x_d, y_d = rbbox[0], rbbox[1], rbbox[2], rbbox[3]
    two = F32(2)
    xs = [-x_d / two, -x_d / two, x_d / two, x_d / two]
    ys = [-y_d / two, y_d / two, y_d / two, -y_d / two]
    c = np.zeros(8, F32)
    for i in range(4):
        c[2 * i] = a_cos * xs[i] + a_sin * ys[i] + cx0
        c[2 * i + 1] = -a_sin * xs[i] + a_cos * ys[i] + cy0
    return c


def _point_in_quad(px, py, c):
    ab0, ab1 = c[2] - c[0], c[3] - c[1]
    ad0, ad1 = c[6] - c[0], c[7] - c[1]
    ap0, ap1 = px - c[0], py - c[1]
    abab = ab0 * ab0 + ab1 * ab1
    abap = ab0 * ap0 + ab1 * ap1
    adad = ad0 * ad0 + ad1 * ad1
    adap = ad0 * ap0 + ad1 * ap1
    return abab >= abap and abap >= 0 and adad >= adap and adap >= 0


def _segment_intersection(p1, p2, i, j):
    a0, a1 = p1[2 * i], p1[2 * i + 1]
    b0, b1 = p1[2 * ((i + 1) % 4)], p1[2 * ((i + 1) % 4) + 1]
    c0, c1 = p2[2 * j], p2[2 * j + 1]
    d0, d1 = p2[2 * ((j + 1) % 4)], p2[2 * ((j + 1) % 4) + 1]
    ba0, ba1 = b0 - a0, b1 - a1
    da0, ca0 = d0 - a0, c0 - a0
    da1, ca1 = d1 - a1, c1 - a1
    acd = da1 * ca0 > ca1 * da0
    bcd = (d1 - b1) * (c0 - b0) > (c1 - b1) * (d0 - b0)
    if acd != bcd:
        abc = ca1 * ba0 > ba1 * ca0
        abd = da1 * ba0 > ba1 * da0
        if abc != abd:
            dc0, dc1 = d0 - c0, d1 - c1
            abba = a0 * b1 - b0 * a1
            cddc = c0 * d1 - d0 * c1
            dh = ba1 * dc0 - ba0 * dc1
            dx = abba * dc0 - ba0 * cddc
            dy = abba * dc1 - ba1 * cddc
            return dx / dh, dy / dh
    return None


def rotated_inter(rbbox1, rbbox2):
    """inter, rotate_iou.py:232-246, all float32"""
    with np.errstate(all="ignore"):
        c1, c2 = _corners(rbbox1), _corners(rbbox2)
        pts = []
        for i in range(4):
            if _point_in_quad(c1[2 * i], c1[2 * i + 1], c2):
                pts.append((c1[2 * i], c1[2 * i + 1]))
            if _point_in_quad(c2[2 * i], c2[2 * i + 1], c1):
                pts.append((c2[2 * i], c2[2 * i + 1]))
        for i in range(4):
            for j in range(4):
                hit = _segment_intersection(c1, c2, i, j)
                if hit is not None:
                    pts.append(hit)
        pts = pts[:POLY_PTS]
        n = len(pts)
        if n > 0:
            cx, cy = F32(0), F32(0)
            for p in pts:
                cx = cx + p[0]
                cy = cy + p[1]
            cx, cy = cx / F32(n), cy / F32(n)
            vs = []
            for p in pts:
                v0, v1 = p[0] - cx, p[1] - cy
                d = np.sqrt(v0 * v0 + v1 * v1)
                v0, v1 = v0 / d, v1 / d
                if v1 < 0:
                    v0 = F32(-2) - v0
                vs.append(v0)
            for i in range(1, n):
                if vs[i - 1] > vs[i]:
                    temp, tp = vs[i], pts[i]
                    j = i
                    while j > 0 and vs[j - 1] > temp:
                        vs[j], pts[j] = vs[j - 1], pts[j - 1]
                        j -= 1
                    vs[j], pts[j] = temp, tp
        area = F32(0)
        for i in range(n - 2):
            a, b, c = pts[0], pts[i + 1], pts[i + 2]
            area = area + abs(((a[0] - c[0]) * (b[1] - c[1]) - (a[1] - c[1]) * (b[0] - c[0])) / F32(2))
        return area


def rotate_iou_eval(boxes, query_boxes, criterion=-1):
    """rotate_iou_gpu_eval: out[n, k] = devRotateIoUEval(query_boxes[k], boxes[n]) (rotate_iou.py:293), float32"""
    boxes, query_boxes = boxes.astype(F32), query_boxes.astype(F32)
    out = np.zeros((boxes.shape[0], query_boxes.shape[0]), F32)
    with np.errstate(all="ignore"):
        for n in range(boxes.shape[0]):
            for k in range(query_boxes.shape[0]):
                r1, r2 = query_boxes[k], boxes[n]
                area1, area2 = r1[2] * r1[3], r2[2] * r2[3]
                ai = rotated_inter(r1, r2)
                if criterion == -1:
                    out[n, k] = ai / (area1 + area2 - ai)
                elif criterion == 0:
                    out[n, k] = ai / area1
                elif criterion == 1:
                    out[n, k] = ai / area2
                else:
                    out[n, k] = ai
    return out


def d3_box_overlap(boxes, qboxes):
    """eval.py:120-152, criterion -1; the ratio is stored into the float32 array rotate_iou_gpu_eval returned"""
    rinc = rotate_iou_eval(boxes[:, [0, 2, 3, 5, 6]], qboxes[:, [0, 2, 3, 5, 6]], 2)
    for i in range(boxes.shape[0]):
        for j in range(qboxes.shape[0]):
            if rinc[i, j] > 0:
                iw = min(boxes[i, 1], qboxes[j, 1]) - max(boxes[i, 1] - boxes[i, 4], qboxes[j, 1] - qboxes[j, 4])
                if iw > 0:
                    area1 = boxes[i, 3] * boxes[i, 4] * boxes[i, 5]
                    area2 = qboxes[j, 3] * qboxes[j, 4] * qboxes[j, 5]
                    inc = iw * np.float64(rinc[i, j])
                    rinc[i, j] = inc / (area1 + area2 - inc)
                else:
                    rinc[i, j] = 0.0
    return rinc


def metric_boxes(anno, metric):
    """the columns calculate_iou_partly concatenates (eval.py:354-387), float64"""
    if metric == 0:
        return np.asarray(anno["bbox"], np.float64).reshape(-1, 4)
    loc = np.asarray(anno["location"], np.float64).reshape(-1, 3)
    dims = np.asarray(anno["dimensions"], np.float64).reshape(-1, 3)
    rots = np.asarray(anno["rotation_y"], np.float64).reshape(-1, 1)
    if metric == 1:
        return np.concatenate([loc[:, [0, 2]], dims[:, [0, 2]], rots], axis=1)
    return np.concatenate([loc, dims, rots], axis=1)


def frame_overlaps(gt_annos, dt_annos, metric):
    """per frame the (dt, gt) block eval_class indexes as overlaps[j, i], float64"""
    out = []
    for g, d in zip(gt_annos, dt_annos):
        db, gb = metric_boxes(d, metric), metric_boxes(g, metric)
        if metric == 0:
            out.append(image_box_overlap(db, gb))
        elif metric == 1:
            out.append(rotate_iou_eval(db, gb).astype(np.float64))
        else:
            out.append(d3_box_overlap(db, gb).astype(np.float64))
    return out


def min_margin(blocks, levels=OFFICIAL_MIN_OVERLAPS):
    """the smallest distance between any overlap of the blocks and any min_overlap of the official tables"""
    best = np.inf
    for b in blocks:
        b = np.asarray(b, np.float64).ravel()
        b = b[np.isfinite(b)]
        for lv in levels:
            if b.size:
                best = min(best, float(np.abs(b - lv).min()))
    return best


# ---- matching -----------------------------------------------------------------------------------------------------------------
def clean_data(gt_anno, dt_anno, current_class, difficulty):
    """eval.py:28-81"""
    class_names = ["car", "pedestrian", "cyclist"]
    min_height, max_occlusion, max_truncation = [40, 25, 25], [0, 1, 2], [0.15, 0.3, 0.5]
    cur = class_names[current_class]
    dc_bboxes, ignored_gt, ignored_dt = [], [], []
    num_valid_gt = 0
    for i in range(len(gt_anno["name"])):
        bbox = gt_anno["bbox"][i]
        name = str(gt_anno["name"][i]).lower()
        height = bbox[3] - bbox[1]
        if name == cur:
            valid = 1
        elif cur == "pedestrian" and name == "person_sitting":
            valid = 0
        elif cur == "car" and name == "van":
            valid = 0
        else:
            valid = -1
        ignore = (gt_anno["occluded"][i] > max_occlusion[difficulty] or gt_anno["truncated"][i] > max_truncation[difficulty]
                  or height <= min_height[difficulty])
        if valid == 1 and not ignore:
            ignored_gt.append(0)
            num_valid_gt += 1
        elif valid == 0 or (ignore and valid == 1):
            ignored_gt.append(1)
        else:
            ignored_gt.append(-1)
        if gt_anno["name"][i] == "DontCare":
            dc_bboxes.append(gt_anno["bbox"][i])
    for i in range(len(dt_anno["name"])):
        valid = 1 if str(dt_anno["name"][i]).lower() == cur else -1
        height = abs(dt_anno["bbox"][i, 3] - dt_anno["bbox"][i, 1])
        if height < min_height[difficulty]:
            ignored_dt.append(1)
        elif valid == 1:
            ignored_dt.append(0)
        else:
            ignored_dt.append(-1)
    return num_valid_gt, ignored_gt, ignored_dt, dc_bboxes


def compute_statistics(overlaps, gt_alphas, dt_alphas, dt_bboxes, dt_scores, ignored_gt, ignored_det, dc_bboxes, metric, min_overlap,
                       thresh=0.0, compute_fp=False, compute_aos=False):
    """compute_statistics_jit, eval.py:155-272, loop for loop; also returns per ground-truth row the matched score or NaN
    (what epnet_kitti_match writes) and the number of similarity terms"""
    det_size, gt_size = len(dt_scores), len(ignored_gt)
    assigned = [False] * det_size
    ignored_threshold = [False] * det_size
    if compute_fp:
        for i in range(det_size):
            if dt_scores[i] < thresh:
                ignored_threshold[i] = True
    tp = fp = fn = 0
    similarity = 0
    thresholds, delta = [], []
    matched = np.full(gt_size, np.nan)
    for i in range(gt_size):
        if ignored_gt[i] == -1:
            continue
        det_idx = -1
        valid_detection = NO_DETECTION
        max_overlap = 0
        assigned_ignored_det = False
        for j in range(det_size):
            if ignored_det[j] == -1:
                continue
            if assigned[j]:
                continue
            if ignored_threshold[j]:
                continue
            overlap = overlaps[j, i]
            dt_score = dt_scores[j]
            if not compute_fp and overlap > min_overlap and dt_score > valid_detection:
                det_idx = j
                valid_detection = dt_score
            elif compute_fp and overlap > min_overlap and (overlap > max_overlap or assigned_ignored_det) and ignored_det[j] == 0:
                max_overlap = overlap
                det_idx = j
                valid_detection = 1
                assigned_ignored_det = False
            elif compute_fp and overlap > min_overlap and valid_detection == NO_DETECTION and ignored_det[j] == 1:
                det_idx = j
                valid_detection = 1
                assigned_ignored_det = True
        if valid_detection == NO_DETECTION and ignored_gt[i] == 0:
            fn += 1
        elif valid_detection != NO_DETECTION and (ignored_gt[i] == 1 or ignored_det[det_idx] == 1):
            assigned[det_idx] = True
        elif valid_detection != NO_DETECTION:
            tp += 1
            thresholds.append(dt_scores[det_idx])
            matched[i] = dt_scores[det_idx]
            if compute_aos:
                delta.append(gt_alphas[i] - dt_alphas[det_idx])
            assigned[det_idx] = True
    if compute_fp:
        for i in range(det_size):
            if not (assigned[i] or ignored_det[i] == -1 or ignored_det[i] == 1 or ignored_threshold[i]):
                fp += 1
        nstuff = 0
        if metric == 0:
            dc = np.asarray(dc_bboxes, np.float64).reshape(-1, 4)
            ov_dc = image_box_overlap(np.asarray(dt_bboxes, np.float64).reshape(-1, 4), dc, 0)
            for i in range(dc.shape[0]):
                for j in range(det_size):
                    if assigned[j]:
                        continue
                    if ignored_det[j] == -1 or ignored_det[j] == 1:
                        continue
                    if ignored_threshold[j]:
                        continue
                    if ov_dc[j, i] > min_overlap:
                        assigned[j] = True
                        nstuff += 1
        fp -= nstuff
        if compute_aos:
            tmp = np.zeros((fp + len(delta),))
            for i in range(len(delta)):
                tmp[i + fp] = (1.0 + np.cos(delta[i])) / 2.0
            similarity = np.sum(tmp) if (tp > 0 or fp > 0) else -1
    return tp, fp, fn, similarity, np.array(thresholds, np.float64), matched, len(delta)


def get_thresholds(scores, num_gt, num_sample_pts=41):
    """eval.py:8-25"""
    scores = np.sort(np.asarray(scores, np.float64))[::-1]
    current_recall = 0
    thresholds = []
    for i, score in enumerate(scores):
        l_recall = (i + 1) / num_gt
        r_recall = (i + 2) / num_gt if i < (len(scores) - 1) else l_recall
        if (r_recall - current_recall) < (current_recall - l_recall) and i < (len(scores) - 1):
            continue
        thresholds.append(score)
        current_recall += 1 / (num_sample_pts - 1.0)
    return thresholds


def prepare(gt_annos, dt_annos, current_class, difficulty):
    frames = []
    total_valid = 0
    for g, d in zip(gt_annos, dt_annos):
        nv, ig, idt, dc = clean_data(g, d, current_class, difficulty)
        total_valid += nv
        frames.append(dict(ignored_gt=np.array(ig, np.int64), ignored_dt=np.array(idt, np.int64),
                           dc=np.asarray(dc, np.float64).reshape(-1, 4), gt_alpha=np.asarray(g["alpha"], np.float64),
                           dt_alpha=np.asarray(d["alpha"], np.float64), dt_bbox=np.asarray(d["bbox"], np.float64).reshape(-1, 4),
                           dt_score=np.asarray(d["score"], np.float64)))
    return frames, total_valid


def eval_combo(overlaps, frames, total_valid, metric, min_overlap, compute_aos, thresholds=None):
    """one (class, difficulty, min_overlap) of eval_class (eval.py:483-541): -> dict(thresholds, pr (T,4), terms (T,),
    matched: per-frame arrays of pass 1)"""
    matched = []
    scores = []
    for ov, fr in zip(overlaps, frames):
        r = compute_statistics(ov, fr["gt_alpha"], fr["dt_alpha"], fr["dt_bbox"], fr["dt_score"], fr["ignored_gt"], fr["ignored_dt"],
                               fr["dc"], metric, min_overlap, 0.0, False)
        scores += r[4].tolist()
        matched.append(r[5])
    if thresholds is None:
        thresholds = get_thresholds(np.array(scores), total_valid)
    thresholds = np.array(thresholds, np.float64)
    pr = np.zeros((len(thresholds), 4))
    terms = np.zeros(len(thresholds), np.int64)
    for ov, fr in zip(overlaps, frames):
        for t, thresh in enumerate(thresholds):
            tp, fp, fn, sim, _, _, nt = compute_statistics(ov, fr["gt_alpha"], fr["dt_alpha"], fr["dt_bbox"], fr["dt_score"],
                                                           fr["ignored_gt"], fr["ignored_dt"], fr["dc"], metric, min_overlap, thresh,
                                                           True, compute_aos)
            pr[t, 0] += tp
            pr[t, 1] += fp
            pr[t, 2] += fn
            if sim != -1:
                pr[t, 3] += sim
            terms[t] += nt
    return dict(thresholds=thresholds, pr=pr, terms=terms, matched=matched)


def curves(pr, compute_aos, n_sample_pts=41):
    """eval.py:531-541: -> precision, recall, aos rows of n_sample_pts"""
    precision, recall, aos = np.zeros(n_sample_pts), np.zeros(n_sample_pts), np.zeros(n_sample_pts)
    n = pr.shape[0]
    with np.errstate(all="ignore"):
        for i in range(n):
            recall[i] = pr[i, 0] / (pr[i, 0] + pr[i, 2])
            precision[i] = pr[i, 0] / (pr[i, 0] + pr[i, 1])
            if compute_aos:
                aos[i] = pr[i, 3] / (pr[i, 0] + pr[i, 1])
        for i in range(n):
            precision[i] = np.max(precision[i:], axis=-1)
            recall[i] = np.max(recall[i:], axis=-1)
            if compute_aos:
                aos[i] = np.max(aos[i:], axis=-1)
    return precision, recall, aos


def eval_class(gt_annos, dt_annos, current_classes, difficultys, metric, min_overlaps, compute_aos=False, overlaps=None, detail=None):
    """eval.py:442-547 on per-frame blocks; `detail`, a dict, receives (m, l, k) -> eval_combo's result"""
    if overlaps is None:
        overlaps = frame_overlaps(gt_annos, dt_annos, metric)
    shape = [len(current_classes), len(difficultys), len(min_overlaps), 41]
    precision, recall, aos = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    for m, current_class in enumerate(current_classes):
        for l, difficulty in enumerate(difficultys):
            frames, total_valid = prepare(gt_annos, dt_annos, current_class, difficulty)
            for k, min_overlap in enumerate(min_overlaps[:, metric, m]):
                r = eval_combo(overlaps, frames, total_valid, metric, min_overlap, compute_aos)
                if detail is not None:
                    detail[(m, l, k)] = r
                precision[m, l, k], recall[m, l, k], aos[m, l, k] = curves(r["pr"], compute_aos)
    return {"recall": recall, "precision": precision, "orientation": aos}


def get_mAP(prec):
    """eval.py:556-560, the 40-point form"""
    sums = 0
    for i in range(1, prec.shape[-1], 1):
        sums = sums + prec[..., i]
    return sums / 40 * 100


CLASS_TO_NAME = {0: "Car", 1: "Pedestrian", 2: "Cyclist", 3: "Van", 4: "Person_sitting"}


def official_min_overlaps(current_classes):
    overlap_0_7 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5], [0.7, 0.5, 0.5, 0.7, 0.5], [0.7, 0.5, 0.5, 0.7, 0.5]])
    overlap_0_5 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25], [0.5, 0.25, 0.25, 0.5, 0.25]])
    return np.stack([overlap_0_7, overlap_0_5], axis=0)[:, :, current_classes]


def wants_aos(dt_annos):
    for anno in dt_annos:
        if anno["alpha"].shape[0] != 0:
            return bool(anno["alpha"][0] != -10)
    return False


def format_result(current_classes, min_overlaps, mAPbbox, mAPbev, mAP3d, mAPaos):
    """eval.py:650-682"""
    result = ""
    for j, curcls in enumerate(current_classes):
        for i in range(min_overlaps.shape[0]):
            result += "%s AP@%.2f, %.2f, %.2f:\n" % ((CLASS_TO_NAME[curcls],) + tuple(min_overlaps[i, :, j]))
            result += "bbox AP:%.4f, %.4f, %.4f\n" % tuple(mAPbbox[j, :, i])
            result += "bev  AP:%.4f, %.4f, %.4f\n" % tuple(mAPbev[j, :, i])
            result += "3d   AP:%.4f, %.4f, %.4f\n" % tuple(mAP3d[j, :, i])
            if mAPaos is not None:
                result += "aos  AP:%.2f, %.2f, %.2f\n" % tuple(mAPaos[j, :, i])
    ret = {}
    for key, arr in (("3d", mAP3d), ("bev", mAPbev), ("image", mAPbbox)):
        for d, name in enumerate(("easy", "moderate", "hard")):
            ret["Car_%s_%s" % (key, name)] = arr[0, d, 0]
    return result, ret


def get_official_eval_result(gt_annos, dt_annos, current_classes, overlaps=None, detail=None):
    """eval.py:613-682; `overlaps`: optional {metric: per-frame blocks}; `detail` receives (metric, m, l, k) -> eval_combo's result
    and ("mAP", metric) -> the mAP array"""
    if not isinstance(current_classes, (list, tuple)):
        current_classes = [current_classes]
    name_to_class = {v: n for n, v in CLASS_TO_NAME.items()}
    current_classes = [name_to_class[c] if isinstance(c, str) else c for c in current_classes]
    min_overlaps = official_min_overlaps(current_classes)
    compute_aos = wants_aos(dt_annos)
    maps = []
    aos = None
    for metric in range(3):
        det = {} if detail is not None else None
        ret = eval_class(gt_annos, dt_annos, current_classes, [0, 1, 2], metric, min_overlaps, compute_aos and metric == 0,
                         None if overlaps is None else overlaps[metric], det)
        maps.append(get_mAP(ret["precision"]))
        if metric == 0 and compute_aos:
            aos = get_mAP(ret["orientation"])
        if detail is not None:
            for key, val in det.items():
                detail[(metric,) + key] = val
            detail[("mAP", metric)] = maps[-1]
            detail[("curves", metric)] = ret
    if detail is not None and aos is not None:
        detail[("mAP", "aos")] = aos
    return format_result(current_classes, min_overlaps, maps[0], maps[1], maps[2], aos)

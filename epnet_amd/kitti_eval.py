"""The KITTI AP evaluator under the reference's public names (tools/kitti_object_eval_python: evaluate.py, eval.py and the
annotation helpers of kitti_common.py), so that tools/eval_rcnn.py:739 gets its AP on an MI355X without numba. Written from
the evaluator's behaviour -- same names, arguments and results, pinned by tests/golden/kitti_eval.npz -- not from its text.

Device side (csrc/kitti_eval.hip through kitti_eval_cuda): the per-frame overlap blocks of the three metrics, pass 1 (the
matched scores at threshold 0) and pass 2 (tp / fp / fn / similarity per threshold) for every frame x threshold x
(difficulty, min_overlap) of a class in one launch each. Host side, in numpy: label parsing, the ignore tables (whole data
set at once), the recall thresholds (a host op of the library), precision / recall / running maximum / AP and the text.
``device=`` selects the GPU (default: the current one). ``coco=True`` is not implemented: tools/eval_rcnn.py never sets it.
"""
import contextlib
import os
import re
import time

import numpy as np
import torch

from . import kitti_eval_cuda as kc
from . import pointnet2_utils

N_SAMPLE_PTS = 41
CLASS_NAMES = ("Car", "Pedestrian", "Cyclist", "Van", "Person_sitting")     # class index -> name
# per difficulty (easy, moderate, hard): smallest 2D box height in pixels, highest occlusion level, highest truncation
DIFFICULTY_RULES = ((40, 0, 0.15), (25, 1, 0.3), (25, 2, 0.5))
# a ground truth of the neighbouring class neither counts nor costs: a detection on it is no false positive
NEIGHBOUR_CLASS = {"car": "van", "pedestrian": "person_sitting"}
# min_overlap per class index: the official row, and the relaxed row for the bev / 3d metrics
OVERLAP_STRICT = (0.7, 0.5, 0.5, 0.7, 0.5)
OVERLAP_RELAXED = (0.5, 0.25, 0.25, 0.5, 0.25)
LABEL_FIELDS = ("name", "truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y", "score")


@contextlib.contextmanager
def _timed(profile, name, device):
    """adds the seconds of the body to profile[name], a device synchronisation either side; nothing when profile is None"""
    if profile is None:
        yield
        return
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    try:
        yield
    finally:
        torch.cuda.synchronize(device)
        profile[name] = profile.get(name, 0.0) + time.perf_counter() - t0


# ---- annotations ----------------------------------------------------------------------------------------------------------------
def get_label_anno(label_path):
    """one KITTI label / result file -> dict of arrays (LABEL_FIELDS). A line is `name truncated occluded alpha x1 y1 x2 y2 h w l
    x y z ry [score]`; dimensions come back as (l, h, w). The score column is read when the first line has it, zeros otherwise."""
    with open(label_path, "r") as f:
        rows = [line.split() for line in f if line.strip()]
    numbers = np.array([[float(v) for v in row[1:15]] for row in rows], np.float64).reshape(-1, 14)
    anno = {
        "name": np.array([row[0] for row in rows]),
        "truncated": numbers[:, 0].copy(),
        "occluded": np.array([int(row[2]) for row in rows], np.int64) if rows else np.zeros(0),
        "alpha": numbers[:, 2].copy(),
        "bbox": numbers[:, 3:7].copy(),
        "dimensions": numbers[:, [9, 7, 8]],
        "location": numbers[:, 10:13].copy(),
        "rotation_y": numbers[:, 13].copy(),
    }
    scored = bool(rows) and len(rows[0]) == 16
    anno["score"] = np.array([float(row[15]) for row in rows], np.float64) if scored else np.zeros(len(rows))
    return anno


def get_label_annos(label_folder, image_ids=None):
    """the annos of a folder of `%06d.txt` files: all of them in ascending order (image_ids None), the first image_ids (an int) or
    the listed ones"""
    folder = os.fspath(label_folder)
    if image_ids is None:
        image_ids = sorted(int(name[:6]) for name in os.listdir(folder) if re.fullmatch(r"\d{6}\.txt", name))
    elif not isinstance(image_ids, list):
        image_ids = list(range(image_ids))
    return [get_label_anno(os.path.join(folder, "%06d.txt" % idx)) for idx in image_ids]


def filter_annos_low_score(image_annos, thresh):
    """per frame only the rows with score >= thresh, every field"""
    out = []
    for anno in image_annos:
        keep = np.flatnonzero(np.asarray(anno["score"]) >= thresh)
        out.append({key: value[keep] for key, value in anno.items()})
    return out


def _ignore_codes(gt_name, gt_occluded, gt_truncated, gt_bbox, dt_name, dt_bbox, current_class, difficulty):
    """the evaluator's ignore tables for rows of any number of frames at once.
    ground truth: 0 = counts (the class, within the difficulty's limits), 1 = neutral (the class but harder, or the neighbouring
    class), -1 = another class. detection: 1 = too small for the difficulty (whatever its class), 0 = the class, -1 = another."""
    min_height, max_occlusion, max_truncation = DIFFICULTY_RULES[difficulty]
    wanted = CLASS_NAMES[current_class].lower()
    gt_lower = np.char.lower(np.asarray(gt_name, dtype=str)) if len(gt_name) else np.zeros(0, dtype=str)
    dt_lower = np.char.lower(np.asarray(dt_name, dtype=str)) if len(dt_name) else np.zeros(0, dtype=str)
    same = gt_lower == wanted
    neighbour = gt_lower == NEIGHBOUR_CLASS.get(wanted, "")
    harder = (gt_occluded > max_occlusion) | (gt_truncated > max_truncation) | ((gt_bbox[:, 3] - gt_bbox[:, 1]) <= min_height)
    gt_code = np.full(len(gt_lower), -1, np.int32)
    gt_code[neighbour | (same & harder)] = 1
    gt_code[same & ~harder] = 0
    dt_code = np.where(dt_lower == wanted, 0, -1).astype(np.int32)
    dt_code[np.abs(dt_bbox[:, 3] - dt_bbox[:, 1]) < min_height] = 1
    return gt_code, dt_code


def clean_data(gt_anno, dt_anno, current_class, difficulty):
    """(num_valid_gt, ignored_gt, ignored_dt, dc_bboxes) of one frame, as the reference's function of this name: the ignore codes
    of _ignore_codes as lists, the number of ground truths that count, and the 2D boxes of the rows named exactly DontCare"""
    gt_bbox = np.asarray(gt_anno["bbox"], np.float64).reshape(-1, 4)
    gt_code, dt_code = _ignore_codes(gt_anno["name"], np.asarray(gt_anno["occluded"]), np.asarray(gt_anno["truncated"]), gt_bbox,
                                     dt_anno["name"], np.asarray(dt_anno["bbox"], np.float64).reshape(-1, 4), current_class, difficulty)
    dontcare = [gt_bbox[i] for i, name in enumerate(gt_anno["name"]) if name == "DontCare"]
    return int((gt_code == 0).sum()), gt_code.tolist(), dt_code.tolist(), dontcare


# ---- the device side --------------------------------------------------------------------------------------------------------------
def _metric_boxes(annos, metric):
    """the columns calculate_iou_partly concatenates (eval.py:354-387), all frames, float64"""
    if metric == 0:
        return _cat(annos, "bbox", 4)
    loc, dims, rots = _cat(annos, "location", 3), _cat(annos, "dimensions", 3), _cat(annos, "rotation_y", 1)[:, None]
    if metric == 1:
        return np.concatenate([loc[:, [0, 2]], dims[:, [0, 2]], rots], axis=1)
    return np.concatenate([loc, dims, rots], axis=1)


def _cat(annos, key, width):
    """one float64 array of a field over all frames: (total,) for width 1, (total, width) otherwise"""
    parts = [np.asarray(a[key], np.float64).reshape(-1, width) for a in annos] + [np.zeros((0, width))]
    out = np.concatenate(parts, 0)
    return out.reshape(-1) if width == 1 else out


def _offsets(counts, dtype=np.int32):
    off = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    return off.astype(dtype)


def _device(device):
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("epnet_amd.kitti_eval runs on the GPU (there is no CPU fallback), got device %s" % (device,))
    return torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())


class _Uploaded:
    """the annotations of one evaluation on the device: ragged offsets and the float64 columns the kernels read. Rows are
    (boxes = first argument, query_boxes = second), as calculate_iou_partly names them; eval_class passes (dt, gt)."""

    def __init__(self, row_annos, col_annos, device, profile=None):
        assert len(row_annos) == len(col_annos)
        self.profile = profile
        self.device = _device(device)
        self.row_annos, self.col_annos = row_annos, col_annos
        self.row_num = np.array([len(a["name"]) for a in row_annos], np.int64)
        self.col_num = np.array([len(a["name"]) for a in col_annos], np.int64)
        self.frames = len(row_annos)
        self.max_rows = int(self.row_num.max()) if self.frames else 0
        self.max_cols = int(self.col_num.max()) if self.frames else 0
        self.ov_off_h = _offsets(self.row_num * self.col_num, np.int64)
        self.anchor = torch.empty((1,), device=self.device)
        self.row_off = self._up(_offsets(self.row_num))
        self.col_off = self._up(_offsets(self.col_num))
        self.ov_off = self._up(self.ov_off_h)
        self.overlaps = {}
        self.tables = {}
        self.columns = None     # host columns of the ignore tables, built once
        self.dt_score = None    # the matching kernels' inputs, uploaded by the first eval_class

    def _up(self, array):
        return torch.from_numpy(np.ascontiguousarray(array)).to(self.device)

    def overlap(self, metric):
        """the (row, col) blocks of one metric, one flat float64 device tensor"""
        if metric not in self.overlaps:
            if metric not in (0, 1, 2):
                raise ValueError("unknown metric")
            with _timed(self.profile, "upload", self.device):
                rows, cols = self._up(_metric_boxes(self.row_annos, metric)), self._up(_metric_boxes(self.col_annos, metric))
            with _timed(self.profile, "overlaps_metric%d" % metric, self.device):
                out = pointnet2_utils._new(self.anchor, (max(int(self.ov_off_h[-1]), 1),), torch.float64)
                kc.kitti_overlaps_gpu(metric, -1, self.max_rows, self.max_cols, self.row_off, self.col_off, self.ov_off, rows, cols, out)
            self.overlaps[metric] = out
        return self.overlaps[metric]


def calculate_iou_partly(gt_annos, dt_annos, metric, num_parts=50, device=None):
    """eval.py:334-408: per frame the (gt_annos[i], dt_annos[i]) block of the metric (0: bbox, 1: bev, 2: 3d), float64, as the
    list the reference returns first. Only these blocks are computed, so the second value (the reference's part x part
    matrices) is None; num_parts is accepted and has no effect.

    The per-frame limits follow the ARGUMENT ORDER, not the names: the first argument supplies the rows of a block (at most
    kitti_eval_cuda.MAX_DT = 1024 per frame), the second its columns (at most MAX_GT = 256). eval_class calls this with
    (dt_annos, gt_annos), as the reference does; a caller that passes (gt, dt) gets 1024 ground truths and 256 detections per
    frame, and beyond either the library's "problem size outside the supported range" error."""
    for what, annos, limit in (("first", gt_annos, kc.MAX_DT), ("second", dt_annos, kc.MAX_GT)):
        worst = max([len(a["name"]) for a in annos] + [0])
        if worst > limit:
            raise ValueError("calculate_iou_partly: a frame of the %s argument has %d boxes, the limit for that position is %d"
                             % (what, worst, limit))
    up = _Uploaded(gt_annos, dt_annos, device)
    flat = up.overlap(metric).cpu().numpy()
    overlaps = [flat[up.ov_off_h[f]:up.ov_off_h[f + 1]].reshape(int(up.row_num[f]), int(up.col_num[f])) for f in range(up.frames)]
    return overlaps, None, up.row_num.copy(), up.col_num.copy()


def rotate_iou_gpu_eval(boxes, query_boxes, criterion=-1, device_id=0):
    """rotate_iou.py:297-332 for criterion -1: (N,5) x (K,5) [x, y, x_d, y_d, angle] -> (N,K) float32"""
    if criterion != -1:
        raise NotImplementedError("rotate_iou_gpu_eval: criterion %r (the evaluator's bev metric uses -1; the 3d metric's area is internal)" % (criterion,))
    boxes, query_boxes = np.asarray(boxes), np.asarray(query_boxes)
    n, k = boxes.shape[0], query_boxes.shape[0]
    if n == 0 or k == 0:
        return np.zeros((n, k), np.float32)
    if n > kc.MAX_DT or k > kc.MAX_GT:   # tile the matrix into frames of the supported size
        out = np.zeros((n, k), np.float32)
        for r in range(0, n, kc.MAX_DT):
            for c in range(0, k, kc.MAX_GT):
                out[r:r + kc.MAX_DT, c:c + kc.MAX_GT] = rotate_iou_gpu_eval(boxes[r:r + kc.MAX_DT], query_boxes[c:c + kc.MAX_GT], -1, device_id)
        return out
    dev = torch.device("cuda", device_id)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    rows, cols = up(boxes.astype(np.float32).astype(np.float64)), up(query_boxes.astype(np.float32).astype(np.float64))
    out = pointnet2_utils._new(rows, (n * k,), torch.float64)
    kc.kitti_overlaps_gpu(1, -1, n, k, up(np.array([0, n], np.int32)), up(np.array([0, k], np.int32)), up(np.array([0, n * k], np.int64)),
                          rows, cols, out)
    return out.cpu().numpy().reshape(n, k).astype(np.float32)


def _class_tables(up, gt_annos, dt_annos, current_class, difficultys):
    """ignore tables of the whole data set -> (D, total_gt) int32, (D, total_dt) int32, the ground truths that count per difficulty"""
    if up.columns is None:
        names = lambda annos: np.array([str(n) for a in annos for n in a["name"]], dtype=str)  # noqa: E731
        up.columns = (names(gt_annos), _cat(gt_annos, "occluded", 1), _cat(gt_annos, "truncated", 1), _cat(gt_annos, "bbox", 4),
                      names(dt_annos), _cat(dt_annos, "bbox", 4))
    pairs = [_ignore_codes(*up.columns, current_class, difficulty) for difficulty in difficultys]
    gt_codes = np.stack([g for g, _ in pairs]).reshape(len(difficultys), -1)
    dt_codes = np.stack([d for _, d in pairs]).reshape(len(difficultys), -1)
    return gt_codes, dt_codes, [int((g == 0).sum()) for g, _ in pairs]


def _curve(values, count):
    """a 41-point row: the first `count` values, each replaced by the largest value at or after it"""
    row = np.zeros(N_SAMPLE_PTS)
    row[:count] = values
    return np.maximum.accumulate(row[::-1])[::-1]


def eval_class(gt_annos, dt_annos, current_classes, difficultys, metric, min_overlaps, compute_aos=False, num_parts=50, device=None,
               _uploaded=None, _detail=None, _profile=None):
    """precision / recall / orientation curves of one metric (0: bbox, 1: bev, 2: 3d). min_overlaps: [num_overlap, metric, class].
    Returns {"recall", "precision", "orientation"}, each [num_class, num_difficulty, num_minoverlap, 41]. num_parts is accepted
    and has no effect. `_detail`, a dict, receives per (m, l, k) the thresholds and the pr table."""
    assert len(gt_annos) == len(dt_annos)
    up = _uploaded if _uploaded is not None else _Uploaded(dt_annos, gt_annos, device, _profile)   # rows = detections
    dev, prof = up.device, up.profile
    overlaps = up.overlap(metric)
    if up.dt_score is None:
        with _timed(prof, "upload", dev):
            up.dt_score = up._up(_cat(dt_annos, "score", 1))
            up.dt_alpha = up._up(_cat(dt_annos, "alpha", 1))
            up.gt_alpha = up._up(_cat(gt_annos, "alpha", 1))
            up.dt_bbox = up._up(_cat(dt_annos, "bbox", 4))
            dc = [np.asarray(a["bbox"], np.float64).reshape(-1, 4)[np.array([n == "DontCare" for n in a["name"]], bool)] for a in gt_annos]
            up.dc_num = np.array([len(b) for b in dc], np.int64)
            up.dc_bbox = up._up(np.concatenate(dc + [np.zeros((0, 4))], 0))
            up.dc_off = up._up(_offsets(up.dc_num))
    max_dt, max_gt = up.max_rows, up.max_cols
    max_dc = int(up.dc_num.max()) if up.frames else 0
    shape = [len(current_classes), len(difficultys), len(min_overlaps), N_SAMPLE_PTS]
    curves = {"recall": np.zeros(shape), "precision": np.zeros(shape), "orientation": np.zeros(shape)}
    every = [(l, k) for l in range(len(difficultys)) for k in range(len(min_overlaps))]
    for m, current_class in enumerate(current_classes):
        with _timed(prof, "clean_data", dev):
            key = (current_class, tuple(difficultys))   # the three metrics of do_eval share the tables
            if key not in up.tables:
                up.tables[key] = _class_tables(up, gt_annos, dt_annos, current_class, difficultys)
            ign_gt_h, ign_dt_h, valid = up.tables[key]
        with _timed(prof, "upload", dev):
            ign_gt, ign_dt = up._up(ign_gt_h), up._up(ign_dt_h)
        total_gt = ign_gt_h.shape[1]
        for start in range(0, len(every), kc.MAX_COMBOS):
            combos = every[start:start + kc.MAX_COMBOS]
            c_diff = [l for l, _ in combos]
            c_min = [float(min_overlaps[k, metric, m]) for _, k in combos]
            with _timed(prof, "pass1", dev):
                matched = pointnet2_utils._new(up.anchor, (len(combos), max(total_gt, 1)), torch.float64)
                if total_gt:
                    kc.kitti_match_gpu(max_gt, max_dt, c_diff, c_min, up.col_off, up.row_off, up.ov_off, overlaps, up.dt_score, ign_gt,
                                       ign_dt, matched)
                matched_h = matched.cpu() if total_gt else torch.zeros((len(combos), 0), dtype=torch.float64)
            with _timed(prof, "thresholds_host", dev):
                thr = [kc.kitti_thresholds_cpu(matched_h[c].contiguous(), valid[l], N_SAMPLE_PTS) for c, (l, _) in enumerate(combos)]
                thr_h = np.zeros((len(combos), N_SAMPLE_PTS))
                for c, t in enumerate(thr):
                    thr_h[c, :len(t)] = t
            with _timed(prof, "pass2", dev):
                counts = pointnet2_utils._new(up.anchor, (len(combos), N_SAMPLE_PTS, 3), torch.int32)
                sims = pointnet2_utils._new(up.anchor, (len(combos), N_SAMPLE_PTS), torch.float64)
                kc.kitti_pr_gpu(max_gt, max_dt, max_dc, metric, compute_aos, c_diff, c_min, [len(t) for t in thr], up.col_off, up.row_off,
                                up.dc_off, up.ov_off, overlaps, up.dt_score, ign_gt, ign_dt, up.dt_bbox, up.dc_bbox, up.gt_alpha,
                                up.dt_alpha, up._up(thr_h), counts, sims)
                counts_h, sims_h = counts.cpu().numpy().astype(np.float64), sims.cpu().numpy()
            with _timed(prof, "host_tail", dev):
                for c, (l, k) in enumerate(combos):
                    n = len(thr[c])
                    tp, fp, fn = counts_h[c, :n, 0], counts_h[c, :n, 1], counts_h[c, :n, 2]
                    if _detail is not None:
                        _detail[(m, l, k)] = {"thresholds": thr[c], "pr": np.column_stack([tp, fp, fn, sims_h[c, :n]])}
                    with np.errstate(all="ignore"):
                        curves["recall"][m, l, k] = _curve(tp / (tp + fn), n)
                        curves["precision"][m, l, k] = _curve(tp / (tp + fp), n)
                        if compute_aos:
                            curves["orientation"][m, l, k] = _curve(sims_h[c, :n] / (tp + fp), n)
    return curves


def get_mAP(prec):
    """average over the 40 recall points after the first, in percent: [..., 41] -> [...]"""
    total = np.zeros(prec.shape[:-1])
    for column in np.moveaxis(prec[..., 1:], -1, 0):
        total = total + column
    return total / 40 * 100


def do_eval(gt_annos, dt_annos, current_classes, min_overlaps, compute_aos=False, device=None, _detail=None, _profile=None):
    """(mAP_bbox, mAP_bev, mAP_3d, mAP_aos or None), each [num_class, 3 difficulties, num_minoverlap]; min_overlaps:
    [num_minoverlap, metric, num_class]. One upload serves the three metrics."""
    up = _Uploaded(dt_annos, gt_annos, device, _profile)
    out = []
    aos = None
    for metric in range(3):
        detail = _detail.setdefault(metric, {}) if _detail is not None else None
        curves = eval_class(gt_annos, dt_annos, current_classes, [0, 1, 2], metric, min_overlaps, compute_aos and metric == 0,
                            _uploaded=up, _detail=detail)
        out.append(get_mAP(curves["precision"]))
        if metric == 0 and compute_aos:
            aos = get_mAP(curves["orientation"])
    return out[0], out[1], out[2], aos


def _class_index(c):
    return CLASS_NAMES.index(c) if isinstance(c, str) else int(c)


def get_official_eval_result(gt_annos, dt_annos, current_classes, device=None, _detail=None, _profile=None):
    """the official AP of the classes (indices or names, one or a list) -> (text, dict of the nine Car_* values). Per class two
    blocks, AP at the official min_overlaps and at the relaxed bev / 3d ones, each with a bbox / bev / 3d line of easy, moderate,
    hard and, when the detections carry alpha (the first one is not -10), an aos line."""
    classes = [_class_index(c) for c in (current_classes if isinstance(current_classes, (list, tuple)) else [current_classes])]
    table = np.array([[OVERLAP_STRICT] * 3, [OVERLAP_STRICT, OVERLAP_RELAXED, OVERLAP_RELAXED]])   # [row, metric, class index]
    min_overlaps = table[:, :, classes]
    first = next((a["alpha"] for a in dt_annos if a["alpha"].shape[0] != 0), None)
    compute_aos = first is not None and bool(first[0] != -10)
    ap = dict(zip(("bbox", "bev", "3d", "aos"),
                  do_eval(gt_annos, dt_annos, classes, min_overlaps, compute_aos, device=device, _detail=_detail, _profile=_profile)))
    with _timed(_profile, "host_tail", _device(device)):
        lines = []
        for j, cls in enumerate(classes):
            for row in range(min_overlaps.shape[0]):
                lines.append("%s AP@%s:" % (CLASS_NAMES[cls], ", ".join("%.2f" % v for v in min_overlaps[row, :, j])))
                for label, key, digits in (("bbox", "bbox", 4), ("bev ", "bev", 4), ("3d  ", "3d", 4), ("aos ", "aos", 2)):
                    if ap[key] is not None:
                        lines.append("%s AP:%s" % (label, ", ".join("%.*f" % (digits, v) for v in ap[key][j, :, row])))
        ret_dict = {"Car_%s_%s" % (name, level): ap[key][0, d, 0]
                    for name, key in (("3d", "3d"), ("bev", "bev"), ("image", "bbox")) for d, level in enumerate(("easy", "moderate", "hard"))}
    return "".join(line + "\n" for line in lines), ret_dict


def get_coco_eval_result(gt_annos, dt_annos, current_classes):
    raise NotImplementedError("the COCO-style AP is not implemented: tools/eval_rcnn.py:739 evaluates with coco=False")


def evaluate(label_path, result_path, label_split_file, current_class=0, coco=False, score_thresh=-1, device=None):
    """the call of tools/eval_rcnn.py:739: detections from result_path (all files), ground truth from label_path for the image
    ids listed in label_split_file (one per line), detections below a positive score_thresh dropped -> get_official_eval_result"""
    if coco:
        raise NotImplementedError("coco=True: the COCO-style AP is not implemented; tools/eval_rcnn.py:739 never sets it")
    dt_annos = get_label_annos(result_path)
    if score_thresh > 0:
        dt_annos = filter_annos_low_score(dt_annos, score_thresh)
    with open(label_split_file, "r") as f:
        image_ids = [int(line) for line in f if line.strip()]
    return get_official_eval_result(get_label_annos(label_path, image_ids), dt_annos, current_class, device=device)

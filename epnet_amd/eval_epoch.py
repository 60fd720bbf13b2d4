"""The evaluation loop of eval_one_epoch_joint (reference: tools/eval_rcnn.py:589-690 with save_kitti_format :76-101 and the
summary :693-734) with its per-scene host work moved onto the device.

Between the detector's outputs and the AP evaluator the reference trims the padded ground truth on the host, calls
``boxes_iou3d_gpu`` twice per scene, reads ``(gt_max_iou > thresh).sum().item()`` ten times and the RPN segmentation IoU
once, copies the detections to the host, projects their corners with numpy, and prints a text file per frame that the
evaluator parses again -- about 25 synchronisations per scene. Here ``eval_batch`` is two library calls,
``epnet_eval_recall`` and ``epnet_kitti_records`` (csrc/eval.hip), that leave counters and the records of
the would-be text lines on the device; ``EvalEpoch`` collects them batch by batch without a synchronisation and reads
everything back ONCE at the end of the epoch: the ``ret_dict`` entries the reference logs, and the ``dt_annos`` that
``kitti_eval.get_official_eval_result`` takes in place of the parsed files.
"""
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import iou3d_cuda

THRESH_LIST = (0.1, 0.3, 0.5, 0.7, 0.9)      # tools/eval_rcnn.py:518
RECORD_COLUMNS = ("alpha", "x1", "y1", "x2", "y2", "h", "w", "l", "x", "y", "z", "ry", "score")


def eval_batch(pred_boxes3d, rois, det_boxes3d, det_scores, det_count, gt_boxes3d, P2, img_shape, seg_result=None,
               rpn_cls_label=None, thresh_list=THRESH_LIST, totals=None):
    """One batch of tools/eval_rcnn.py:598-632 and of save_kitti_format on the final detections (:685-690), with no
    synchronisation (graph-capturable). pred_boxes3d / rois (B,M,7), det_boxes3d (B,M,7) / det_scores (B,M) / det_count (B)
    int32 as DetectionLayer returns them, gt_boxes3d (B,G,7..16) zero-padded, P2 (B,3,4), img_shape (B,2) int32 [h, w];
    seg_result / rpn_cls_label (B,N) integer tensors or both None (RPN.FIXED); totals (1 + 2 T) int64 or None: running epoch
    sums the batch's counts are added to. Returns a namespace of device tensors: scene_stats (B, 1 + 2 T) int32 = [num_gt,
    recalled_refined[T], recalled_roi[T]], seg_counts (3) int64 = [correct, fg, pos] or None, gt_max_pred / gt_max_roi (B,G),
    pred_max_iou (B,M), records (B,M,13) float64 in RECORD_COLUMNS order, rec_count (B) int32, bbox_raw (B,M,4), valid (B,M)
    int32, det_count, totals."""
    dev = pred_boxes3d.device
    b, m, g = pred_boxes3d.shape[0], pred_boxes3d.shape[1], gt_boxes3d.shape[1]
    nt = len(thresh_list)
    F, I = torch.float32, torch.int32
    out = SimpleNamespace(det_count=det_count, totals=totals)
    out.scene_stats = torch.empty((b, 1 + 2 * nt), dtype=I, device=dev)
    out.gt_max_pred = torch.empty((b, g), dtype=F, device=dev)
    out.gt_max_roi = torch.empty((b, g), dtype=F, device=dev)
    out.pred_max_iou = torch.empty((b, m), dtype=F, device=dev)
    out.seg_counts = None
    if seg_result is not None:
        seg_result, rpn_cls_label = seg_result.to(I).contiguous(), rpn_cls_label.to(I).contiguous()
        out.seg_counts = torch.empty((3,), dtype=torch.int64, device=dev)
    iou3d_cuda.eval_recall_gpu(pred_boxes3d.float().contiguous(), rois.float().contiguous(), gt_boxes3d.float().contiguous(),
                               thresh_list, seg_result, rpn_cls_label, out.scene_stats, out.seg_counts, totals, out.gt_max_pred,
                               out.gt_max_roi, out.pred_max_iou)
    dm = det_boxes3d.shape[1]
    out.records = torch.empty((b, dm, 13), dtype=torch.float64, device=dev)
    out.rec_count = torch.empty((b,), dtype=I, device=dev)
    out.bbox_raw = torch.empty((b, dm, 4), dtype=F, device=dev)
    out.valid = torch.empty((b, dm), dtype=I, device=dev)
    iou3d_cuda.kitti_records_gpu(det_boxes3d.float().contiguous(), det_scores.float().contiguous(), det_count,
                                 P2.float().contiguous(), img_shape.to(I).contiguous(), out.records, out.rec_count, out.bbox_raw,
                                 out.valid)
    return out


def _fetch(tensors):
    """the tensors as numpy arrays through ONE device-to-host copy (one synchronisation)"""
    flat = torch.cat([t.contiguous().view(-1).view(torch.uint8) for t in tensors]).cpu().numpy()
    out, off = [], 0
    for t in tensors:
        nbytes = t.numel() * t.element_size()
        dtype = {torch.int32: np.int32, torch.int64: np.int64, torch.float32: np.float32, torch.float64: np.float64}[t.dtype]
        out.append(flat[off:off + nbytes].view(dtype).reshape(tuple(t.shape)).copy())
        off += nbytes
    return out


class EvalEpoch:
    """the bookkeeping of eval_one_epoch_joint over the batches of an epoch: ``update`` per batch (no synchronisation),
    then ``result`` / ``dt_annos`` / ``write_kitti_files``, which share one read-back"""

    def __init__(self, classes="Car", thresh_list=THRESH_LIST):
        self.classes = classes              # cfg.CLASSES: the name written into every record
        self.thresh_list = tuple(float(t) for t in thresh_list)
        self.batches = []                   # (sample ids, the device tensors result() reads back)
        self.totals = None
        self._host = None

    def update(self, sample_ids, pred_boxes3d, rois, det_boxes3d, det_scores, det_count, gt_boxes3d, P2, img_shape,
               seg_result=None, rpn_cls_label=None):
        """eval_batch on one batch. Keeps what the read-back needs -- rec_count, records, seg_counts and a COPY of det_count
        (a detector may reuse its output buffers for the next batch) -- and returns the whole namespace. No synchronisation."""
        if self.totals is None:
            self.totals = torch.zeros((1 + 2 * len(self.thresh_list),), dtype=torch.int64, device=pred_boxes3d.device)
        out = eval_batch(pred_boxes3d, rois, det_boxes3d, det_scores, det_count, gt_boxes3d, P2, img_shape, seg_result,
                         rpn_cls_label, self.thresh_list, self.totals)
        kept = SimpleNamespace(det_count=det_count.clone(), rec_count=out.rec_count, records=out.records, seg_counts=out.seg_counts)
        self.batches.append(([int(s) for s in sample_ids], kept))
        self._host = None
        return out

    def _read_back(self):
        if self._host is None:
            tensors = [self.totals] if self.totals is not None else []
            for _, out in self.batches:
                tensors += [out.det_count, out.rec_count, out.records]
                if out.seg_counts is not None:
                    tensors.append(out.seg_counts)
            arrays = iter(_fetch(tensors)) if tensors else iter(())
            host = SimpleNamespace(totals=next(arrays) if self.totals is not None else None, batches=[])
            for ids, out in self.batches:
                det_count, rec_count, records = next(arrays), next(arrays), next(arrays)
                seg = next(arrays) if out.seg_counts is not None else None
                host.batches.append(SimpleNamespace(ids=ids, det_count=det_count, rec_count=rec_count, records=records, seg=seg))
            self._host = host
        return self._host

    def result(self, num_frames, split_ids=None):
        """the ret_dict entries of tools/eval_rcnn.py:706-734 under the reference's keys, after ONE synchronisation.
        num_frames = len(dataset); split_ids: the ids of the split file, to count the frames never seen (:693-704).

        rpn_iou keeps the reference's quirk: :627-632 sits inside the per-scene loop but works on the whole batch tensor, so the
        batch's IoU -- correct / clamp(fg + pos - correct, min=1.0) in fp32 -- is added batch_size times, and :711 divides the
        sum by the number of BATCHES. rcnn_cls_acc and rcnn_cls_acc_refined are 0.0: the reference never updates them."""
        host = self._read_back()
        nt = len(self.thresh_list)
        totals = host.totals if host.totals is not None else np.zeros(1 + 2 * nt, np.int64)
        total_gt = int(totals[0])
        cnt, total_rpn_iou, final_total, empty_cnt, seen = 0, 0.0, 0, 0, set()
        for bt in host.batches:
            cnt += 1
            if bt.seg is not None:
                correct, fg, pos = (np.float32(v) for v in bt.seg)
                union = np.float32(np.float32(fg + pos) - correct)
                rpn_iou = float(np.float32(correct / max(union, np.float32(1.0))))
                for _ in bt.ids:
                    total_rpn_iou += rpn_iou
            final_total += int(bt.det_count.sum())
            empty_cnt += int((bt.det_count == 0).sum())
            seen.update(bt.ids)
        if split_ids is not None:
            empty_cnt += sum(1 for s in split_ids if int(s) not in seen)
        ret = {"empty_cnt": empty_cnt, "rpn_iou": total_rpn_iou / max(cnt, 1.0), "rcnn_cls_acc": 0.0, "rcnn_cls_acc_refined": 0.0,
               "rcnn_avg_num": final_total / max(num_frames, 1.0)}
        for idx, thresh in enumerate(self.thresh_list):
            ret["rpn_recall(thresh=%.2f)" % thresh] = int(totals[1 + nt + idx]) / max(total_gt, 1.0)
        for idx, thresh in enumerate(self.thresh_list):
            ret["rcnn_recall(thresh=%.2f)" % thresh] = int(totals[1 + idx]) / max(total_gt, 1.0)
        return ret

    def _frames(self):
        """(sample id, records (n,13) float64) per frame in update order"""
        for bt in self._read_back().batches:
            for k, sid in enumerate(bt.ids):
                yield sid, bt.records[k, :int(bt.rec_count[k])]

    def dt_annos(self):
        """one dict per frame, in update order, with the keys, dtypes and column orders kitti_eval.get_label_anno returns for
        the frame's text file (dimensions as (l, h, w)); feeds kitti_eval.get_official_eval_result unchanged"""
        annos = []
        for _, rec in self._frames():
            n = rec.shape[0]
            annos.append({
                "name": np.array([self.classes] * n),
                "truncated": np.full((n,), -1.0),
                "occluded": np.full((n,), -1, np.int64) if n else np.zeros(0),
                "alpha": rec[:, 0].copy(),
                "bbox": rec[:, 1:5].copy(),
                "dimensions": rec[:, [7, 5, 6]],
                "location": rec[:, 8:11].copy(),
                "rotation_y": rec[:, 11].copy(),
                "score": rec[:, 12].copy(),
            })
        return annos

    def write_kitti_files(self, directory):
        """the reference's text lines (:98-101), one `%06d.txt` per frame; a frame with no valid record gets an empty file"""
        os.makedirs(directory, exist_ok=True)
        for sid, rec in self._frames():
            with open(os.path.join(directory, "%06d.txt" % sid), "w") as f:
                for row in rec:
                    f.write("%s -1 -1 " % self.classes + " ".join("%.4f" % v for v in row) + "\n")

"""GT-database augmentation of the point-only loader on the device, with no host synchronisation (reference:
apply_gt_aug_to_one_scene, lib/datasets/kitti_rcnn_dataset.py:590-696, called per scene on a host core from get_rpn_sample
:443-455 and :506-509 when GT_AUG_ENABLED is set; the database is the pickle tools/generate_gt_database.py writes, split into
easy and hard objects at :96-104).

``GTDatabase.from_list`` packs the pickle's list once on the host and moves it to the device. ``draw_gt_aug_tables`` draws the
loop's random decisions as device tables, ``place_objects`` is ONE call of ``epnet_gt_aug_place`` (csrc/gtaug.hip, one launch, one
wave per scene) and ``prepare_scans_gt_aug`` adds ``epnet_gt_aug_points`` (one launch) and ``epnet_scan_prepare_aug`` (csrc/scan.hip,
four launches): three library calls and six launches whatever the data, nothing read back. Its result feeds
``rpn_target_layer.augment_and_label`` unchanged. Only the point-only path is served: a pasted object has no pixels, so the
reference switches the augmentation off on the LI-Fusion path (:312), and RGB columns are not carried.
"""
import numpy as np
import torch

from . import gt_aug_cuda
from . import pointnet2_utils
from . import scan_layer
from .scan_layer import NEAR_DEPTH, _dev

TRIES = 100                                                 # kitti_rcnn_dataset.py:603
EASY_ABOVE = 100                                            # :100
GT_AUG_KEYS = ("GT_AUG_ENABLED", "GT_EXTRA_NUM", "GT_AUG_RAND_NUM", "GT_AUG_APPLY_PROB", "GT_AUG_HARD_RATIO")


def default_cfg():
    """scan_layer.default_cfg plus the five GT_AUG_* keys with the values of lib/config.py:19-23, switched on"""
    cfg = scan_layer.default_cfg()
    cfg.GT_AUG_ENABLED, cfg.GT_EXTRA_NUM, cfg.GT_AUG_RAND_NUM, cfg.GT_AUG_APPLY_PROB, cfg.GT_AUG_HARD_RATIO = True, 15, False, 0.75, 0.6
    return cfg


def _ambient_cfg():
    """the reference's global config when its module is loaded in this process, else the defaults above"""
    import sys
    ref = sys.modules.get("lib.config")
    return ref.cfg if ref is not None and hasattr(ref, "cfg") else default_cfg()


class GTDatabase:
    """the database on the device: boxes (D,7) f32, alpha (D) f32, npts (D) i32, offsets (D+1) i32, points (S,4) f32
    [x, y, z, intensity] packed in object order, easy / hard (i32 row lists: more than 100 points, or not); num_easy, num_hard
    and max_npts are host integers"""

    def __init__(self, boxes, alpha, npts, offsets, points, easy, hard):
        self.boxes, self.alpha, self.npts, self.offsets, self.points, self.easy, self.hard = boxes, alpha, npts, offsets, points, easy, hard
        self.num_objects, self.num_easy, self.num_hard = int(boxes.shape[0]), int(easy.shape[0]), int(hard.shape[0])
        self.max_npts = int(npts.max()) if npts.numel() and not npts.is_cuda else None

    @classmethod
    def from_list(cls, objects, device="cuda"):
        """objects: the reference's pickle, a list of dicts with 'gt_box3d' (7), 'points' (n,3), 'intensity' (n) and 'obj' (an
        object with .alpha); 'alpha' may stand in for 'obj'. Runs once, on the host."""
        if len(objects) == 0:
            raise RuntimeError("the GT database is empty")
        boxes = np.stack([np.asarray(o["gt_box3d"], np.float32).reshape(7) for o in objects])
        alpha = np.array([o["obj"].alpha if "obj" in o else o["alpha"] for o in objects], np.float32)
        rows = []
        for o in objects:
            pts = np.asarray(o["points"], np.float32).reshape(-1, 3)
            inten = np.asarray(o["intensity"], np.float32).reshape(-1)
            if len(inten) != len(pts):
                raise RuntimeError("an object's points and intensity differ in length")
            rows.append(np.concatenate([pts, inten[:, None]], axis=1))
        npts = np.array([len(r) for r in rows], np.int64)
        if int(npts.sum()) >= 2 ** 31:
            raise RuntimeError("the GT database holds 2^31 points or more")
        offsets = np.concatenate([[0], np.cumsum(npts)]).astype(np.int32)
        points = np.concatenate(rows + [np.zeros((1, 4), np.float32)], axis=0)    # one spare row: never an empty tensor
        easy = np.nonzero(npts > EASY_ABOVE)[0].astype(np.int32)
        hard = np.nonzero(npts <= EASY_ABOVE)[0].astype(np.int32)
        host = cls(*[torch.from_numpy(np.ascontiguousarray(a)) for a in (boxes, alpha, npts.astype(np.int32), offsets, points, easy, hard)])
        out = cls(*[t.to(device) for t in (host.boxes, host.alpha, host.npts, host.offsets, host.points, host.easy, host.hard)])
        out.max_npts = host.max_npts
        return out


def draw_gt_aug_tables(batch, db, cfg=None, generator=None, device="cuda", tries=TRIES):
    """the draws of :451 and :599-635 for `batch` scenes -> {"apply": int32 (B), "extra_num": int32 (B), "cand": int32 (B,T)} on the
    device: apply = rand < GT_AUG_APPLY_PROB, and 0 for every scene when GT_AUG_ENABLED is false (the reference's :443, so that
    prepare_scans_gt_aug then is prepare_scans on the raw rows); extra_num = randint(10, GT_EXTRA_NUM) with GT_AUG_RAND_NUM, else
    GT_EXTRA_NUM; per try, with GT_AUG_HARD_RATIO > 0 one uniform p picks the easy (p > ratio) or the hard list and floor(u * len) of a second
    uniform the row in it (an empty list gives -1: the try is skipped), otherwise the row is floor(u * D). Drawn with torch on
    the device, nothing read back; the draws differ from numpy's stream, the distributions do not."""
    cfg = cfg if cfg is not None else _ambient_cfg()
    kw = {"generator": generator, "device": device}
    apply = (torch.rand((batch,), **kw) < float(cfg.GT_AUG_APPLY_PROB)).to(torch.int32)
    if not bool(cfg.GT_AUG_ENABLED):                            # the same draws are consumed either way
        apply = torch.zeros_like(apply)
    top = int(cfg.GT_EXTRA_NUM)
    if bool(cfg.GT_AUG_RAND_NUM):
        if top <= 10:
            raise RuntimeError("GT_AUG_RAND_NUM needs GT_EXTRA_NUM above 10 (np.random.randint(10, GT_EXTRA_NUM))")
        extra = torch.randint(10, top, (batch,), dtype=torch.int64, **kw).to(torch.int32)
    else:
        extra = torch.full((batch,), top, dtype=torch.int32, device=device)

    def pick(u, length, rows):
        if length == 0:
            return torch.full(u.shape, -1, dtype=torch.int32, device=device)
        at = (u * length).floor().clamp_(max=length - 1).to(torch.int64)
        return at.to(torch.int32) if rows is None else rows[at]

    ratio = float(cfg.GT_AUG_HARD_RATIO)
    if ratio > 0:
        p, u = torch.rand((batch, tries), **kw), torch.rand((batch, tries), **kw)
        cand = torch.where(p > ratio, pick(u, db.num_easy, db.easy), pick(u, db.num_hard, db.hard))
    else:
        cand = pick(torch.rand((batch, tries), **kw), db.num_objects, None)
    return {"apply": apply.contiguous(), "extra_num": extra.contiguous(), "cand": cand.contiguous()}


def place_objects(db, tables, all_gt_boxes3d, num_all, gt_boxes3d, gt_alpha, num_gt, road_plane, cfg=None, extra_rows=4096,
                  k_max=gt_aug_cuda.MAX_ACCEPT):
    """db: GTDatabase; tables: draw_gt_aug_tables' dict; all_gt_boxes3d (B,A,7) with num_all (B) rows per scene (every object of
    the label file but DontCare, :447-448: the overlap test); gt_boxes3d (B,G,7), gt_alpha (B,G) with num_gt (B) rows (the
    filtered label rows, :506-513); road_plane (B,4) [a, b, c, d]; extra_rows: the point rows a scene can take -> dict of
    acc_db (B,K) int32, acc_box (B,K,7), acc_move (B,K) float64, acc_row0 (B,K) int32, remove_boxes (B,K,7), gt_boxes3d
    (B,G+K,7), gt_alpha (B,G+K), gt_aug_info (B,8) int32 (include/epnet_ops.h, epnet_gt_aug_place)."""
    cfg = cfg if cfg is not None else _ambient_cfg()
    cand = tables["cand"]
    if not isinstance(cand, torch.Tensor) or not cand.is_cuda:
        raise RuntimeError("cand must be a CUDAtensor (epnet_amd has no CPU fallback)")
    if cand.dim() != 2:
        raise RuntimeError("cand must be (B, T)")
    if not isinstance(all_gt_boxes3d, torch.Tensor) or all_gt_boxes3d.dim() != 3 or not isinstance(gt_boxes3d, torch.Tensor) or gt_boxes3d.dim() != 3:
        raise RuntimeError("all_gt_boxes3d must be (B, A, 7) and gt_boxes3d (B, G, 7)")
    b, a, g, k = cand.shape[0], all_gt_boxes3d.shape[1], gt_boxes3d.shape[1], int(k_max)
    cand = _dev(cand, "cand", torch.int32, cand.shape)
    apply, extra = _dev(tables["apply"], "apply", torch.int32, (b,)), _dev(tables["extra_num"], "extra_num", torch.int32, (b,))
    all_boxes, num_all = _dev(all_gt_boxes3d, "all_gt_boxes3d", torch.float32, (b, a, 7)), _dev(num_all, "num_all", torch.int32, (b,))
    gt, alpha = _dev(gt_boxes3d, "gt_boxes3d", torch.float32, (b, g, 7)), _dev(gt_alpha, "gt_alpha", torch.float32, (b, g))
    num_gt = _dev(num_gt, "num_gt", torch.int32, (b,))
    plane = _dev(road_plane, "road_plane", torch.float64, (b, 4))
    new = pointnet2_utils._new
    out = {"acc_db": new(gt, (b, k), torch.int32), "acc_box": new(gt, (b, k, 7)), "acc_move": new(gt, (b, k), torch.float64),
           "acc_row0": new(gt, (b, k), torch.int32), "remove_boxes": new(gt, (b, k, 7)), "gt_boxes3d": new(gt, (b, g + k, 7)),
           "gt_alpha": new(gt, (b, g + k)), "gt_aug_info": new(gt, (b, 8), torch.int32)}
    scope = [float(v) for v in np.asarray(cfg.PC_AREA_SCOPE, dtype=np.float64).reshape(-1)]
    gt_aug_cuda.gt_aug_place_gpu(db.boxes, db.alpha, db.npts, apply, extra, cand, all_boxes, num_all, gt, alpha, num_gt, plane,
                                 int(cfg.GT_EXTRA_NUM), int(extra_rows), bool(cfg.PC_REDUCE_BY_RANGE), scope, out["acc_db"], out["acc_box"],
                                 out["acc_move"], out["acc_row0"], out["remove_boxes"], out["gt_boxes3d"], out["gt_alpha"], out["gt_aug_info"])
    return out


def draw_tables(batch, p, db, extra_rows=4096, npoints=16384, cfg=None, generator=None, device="cuda"):
    """every draw of one prepare_scans_gt_aug call: draw_gt_aug_tables' dict plus scan_layer.draw_scan_tables' over the p raw and
    the extra rows ("keys" (B,P+E), "slot_perm" (B,N))"""
    tables = draw_gt_aug_tables(batch, db, cfg, generator, device)
    tables.update(scan_layer.draw_scan_tables(batch, p + int(extra_rows), npoints, generator, device))
    return tables


def prepare_scans_gt_aug(pts_lidar, num_raw, V2C, R0, P2, img_shape, tables, db, all_gt_boxes3d, num_all, gt_boxes3d, gt_alpha, num_gt,
                         road_plane, npoints=16384, extra_rows=4096, k_max=gt_aug_cuda.MAX_ACCEPT, cfg=None):
    """scan_layer.prepare_scans with GT-database augmentation between the validity filter and the selection: placement, the
    objects' points, and the sampling over the raw rows that no accepted object's removal box holds plus the objects' rows.
    tables = draw_tables' dict (``keys`` is (B,P+E); ``slot_perm`` may be None). Three library calls, six launches, nothing read
    back. -> prepare_scans' dict (choice >= P names extra row choice - P; scene_info (B,8) adds [raw points removed, extra
    rows]) plus gt_boxes3d (B,G+K,7) and gt_alpha (B,G+K) (the label rows, the accepted boxes directly behind them), gt_aug_info
    (B,8) int32 and extra_pts (B,E,4)."""
    cfg = cfg if cfg is not None else _ambient_cfg()
    if not isinstance(pts_lidar, torch.Tensor) or not pts_lidar.is_cuda:
        raise RuntimeError("pts_lidar must be a CUDAtensor (epnet_amd has no CPU fallback)")
    if pts_lidar.dim() != 3 or pts_lidar.shape[2] != 4:
        raise RuntimeError("pts_lidar must be (B, P, 4)")
    b, p, n, e = pts_lidar.shape[0], pts_lidar.shape[1], int(npoints), int(extra_rows)
    pts = pts_lidar.float().contiguous()
    num_raw = _dev(num_raw, "num_raw", torch.int32, (b,))
    V2C, R0, P2 = _dev(V2C, "V2C", torch.float32, (b, 3, 4)), _dev(R0, "R0", torch.float32, (b, 3, 3)), _dev(P2, "P2", torch.float32, (b, 3, 4))
    img_shape = _dev(img_shape, "img_shape", torch.int32, (b, 2))
    keys = _dev(tables["keys"], "keys", torch.int32, (b, p + e))
    perm = tables.get("slot_perm")
    if perm is not None:
        perm = _dev(perm, "slot_perm", torch.int32, (b, n))
    placed = place_objects(db, tables, all_gt_boxes3d, num_all, gt_boxes3d, gt_alpha, num_gt, road_plane, cfg, e, k_max)
    new = pointnet2_utils._new
    extra_pts = new(pts, (b, e, 4))
    gt_aug_cuda.gt_aug_points_gpu(db.points, db.offsets, placed["acc_db"], placed["acc_move"], placed["acc_row0"], placed["gt_aug_info"],
                                  extra_pts)
    use_intensity = bool(cfg.RPN.USE_INTENSITY)
    pts_rect, feat, xy = new(pts, (b, n, 3)), new(pts, (b, n, 1)), new(pts, (b, n, 2))
    pts_input = new(pts, (b, n, 4)) if use_intensity else None
    choice, info = new(pts, (b, n), torch.int32), new(pts, (b, 8), torch.int32)
    scope = [float(v) for v in np.asarray(cfg.PC_AREA_SCOPE, dtype=np.float64).reshape(-1)]
    gt_aug_cuda.scan_prepare_aug_gpu(pts, num_raw, V2C, R0, P2, img_shape, extra_pts, placed["remove_boxes"], placed["gt_aug_info"], keys,
                                     perm, bool(cfg.PC_REDUCE_BY_RANGE), scope, NEAR_DEPTH, pts_rect, feat, xy, pts_input, choice, info)
    return {"pts_rect": pts_rect, "pts_features": feat, "pts_input": pts_input if use_intensity else pts_rect, "pts_origin_xy": xy,
            "choice": choice, "scene_info": info, "gt_boxes3d": placed["gt_boxes3d"], "gt_alpha": placed["gt_alpha"],
            "gt_aug_info": placed["gt_aug_info"], "extra_pts": extra_pts, "placed": placed}

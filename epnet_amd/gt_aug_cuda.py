"""Stand-in of an extension module the reference does not have: its GT-database augmentation is a host loop of the loader
(lib/datasets/kitti_rcnn_dataset.py:590-696). ``gt_aug_place_gpu`` is the one call of ``epnet_gt_aug_place``, ``gt_aug_points_gpu``
of ``epnet_gt_aug_points`` and ``scan_prepare_aug_gpu`` of ``epnet_scan_prepare_aug`` (include/epnet_ops.h), on the tensors' device
and current stream, nothing read back; the workspace comes from the caching allocator.
"""
import ctypes

import torch

from . import _lib
from ._tensor import dev_ptr, need, on_device_of, writes
from .scan_cuda import _doubles

_F = torch.float32
_D = torch.float64
_I = torch.int32

MAX_TRIES, MAX_EXISTING, MAX_ACCEPT = 128, 224, 32    # EPNET_GT_AUG_MAX_* of include/epnet_ops.h


@writes("acc_db", "acc_box", "acc_move", "acc_row0", "remove_boxes", "gt_out", "alpha_out", "info")
def gt_aug_place_gpu(db_boxes, db_alpha, db_npts, apply, extra_num, cand, all_boxes, num_all, gt_boxes, gt_alpha, num_gt, road_plane,
                     extra_max, e, reduce_by_range, scope, acc_db, acc_box, acc_move, acc_row0, remove_boxes, gt_out, alpha_out, info):
    """db_boxes (D,7), db_alpha (D), db_npts (D) int32; apply (B), extra_num (B), cand (B,T) int32; all_boxes (B,A,7), num_all (B)
    int32; gt_boxes (B,G,7), gt_alpha (B,G), num_gt (B) int32; road_plane (B,4) float64; extra_max: the host's bound on extra_num;
    e: the extra point rows per scene -> acc_db (B,K) int32, acc_box (B,K,7), acc_move (B,K) float64, acc_row0 (B,K) int32,
    remove_boxes (B,K,7), gt_out (B,G+K,7), alpha_out (B,G+K), info (B,8) int32; K is acc_db's."""
    if cand.dim() != 2 or all_boxes.dim() != 3 or gt_boxes.dim() != 3 or acc_db.dim() != 2:
        raise RuntimeError("cand must be (B, T), all_boxes (B, A, 7), gt_boxes (B, G, 7), acc_db (B, K)")
    b, t, a, g, k, d = cand.shape[0], cand.shape[1], all_boxes.shape[1], gt_boxes.shape[1], acc_db.shape[1], db_boxes.shape[0]
    p_db, p_al, p_np = dev_ptr(db_boxes, "db_boxes", _F), dev_ptr(db_alpha, "db_alpha", _F), dev_ptr(db_npts, "db_npts", _I)
    need(db_boxes, d * 7, "db_boxes"); need(db_alpha, d, "db_alpha"); need(db_npts, d, "db_npts")
    p_ap, p_ex, p_ca = dev_ptr(apply, "apply", _I), dev_ptr(extra_num, "extra_num", _I), dev_ptr(cand, "cand", _I)
    need(apply, b, "apply"); need(extra_num, b, "extra_num")
    p_ab, p_na = dev_ptr(all_boxes, "all_boxes", _F), dev_ptr(num_all, "num_all", _I)
    need(all_boxes, b * a * 7, "all_boxes"); need(num_all, b, "num_all")
    p_gb, p_ga, p_ng = dev_ptr(gt_boxes, "gt_boxes", _F), dev_ptr(gt_alpha, "gt_alpha", _F), dev_ptr(num_gt, "num_gt", _I)
    need(gt_boxes, b * g * 7, "gt_boxes"); need(gt_alpha, b * g, "gt_alpha"); need(num_gt, b, "num_gt")
    p_rp = dev_ptr(road_plane, "road_plane", _D)
    need(road_plane, b * 4, "road_plane")
    o_db, o_box, o_mv, o_r0 = dev_ptr(acc_db, "acc_db", _I), dev_ptr(acc_box, "acc_box", _F), dev_ptr(acc_move, "acc_move", _D), dev_ptr(acc_row0, "acc_row0", _I)
    o_rm, o_gt, o_al, o_in = dev_ptr(remove_boxes, "remove_boxes", _F), dev_ptr(gt_out, "gt_out", _F), dev_ptr(alpha_out, "alpha_out", _F), dev_ptr(info, "info", _I)
    need(acc_db, b * k, "acc_db"); need(acc_box, b * k * 7, "acc_box"); need(acc_move, b * k, "acc_move"); need(acc_row0, b * k, "acc_row0")
    need(remove_boxes, b * k * 7, "remove_boxes"); need(gt_out, b * (g + k) * 7, "gt_out"); need(alpha_out, b * (g + k), "alpha_out")
    need(info, b * 8, "info")
    sc = _doubles(scope, 6, "scope")
    with on_device_of(cand) as s:
        _lib.check(_lib.lib().epnet_gt_aug_place(b, t, a, g, k, int(e), d, int(extra_max), int(bool(reduce_by_range)),
                                                 ctypes.cast(sc, ctypes.c_void_p), p_db, p_al, p_np, p_ap, p_ex, p_ca, p_ab, p_na, p_gb, p_ga,
                                                 p_ng, p_rp, o_db, o_box, o_mv, o_r0, o_rm, o_gt, o_al, o_in, s), "gt_aug_place")
    return 1


@writes("extra_pts")
def gt_aug_points_gpu(db_points, db_offsets, acc_db, acc_move, acc_row0, info, extra_pts):
    """db_points (S,4), db_offsets (D+1) int32, acc_db / acc_move / acc_row0 (B,K), info (B,8) as gt_aug_place_gpu wrote them ->
    extra_pts (B,E,4)"""
    if extra_pts.dim() != 3 or extra_pts.shape[2] != 4 or acc_db.dim() != 2 or extra_pts.shape[0] != acc_db.shape[0]:
        raise RuntimeError("extra_pts must be (B, E, 4) and acc_db (B, K)")
    b, e, k, d, rows = extra_pts.shape[0], extra_pts.shape[1], acc_db.shape[1], db_offsets.numel() - 1, db_points.shape[0]
    p_pt, p_of = dev_ptr(db_points, "db_points", _F), dev_ptr(db_offsets, "db_offsets", _I)
    p_db, p_mv, p_r0 = dev_ptr(acc_db, "acc_db", _I), dev_ptr(acc_move, "acc_move", _D), dev_ptr(acc_row0, "acc_row0", _I)
    p_in, o_pt = dev_ptr(info, "info", _I), dev_ptr(extra_pts, "extra_pts", _F)
    need(db_points, rows * 4, "db_points"); need(db_offsets, d + 1, "db_offsets"); need(acc_db, b * k, "acc_db")
    need(acc_move, b * k, "acc_move"); need(acc_row0, b * k, "acc_row0"); need(info, b * 8, "info"); need(extra_pts, b * e * 4, "extra_pts")
    if d < 1:
        raise RuntimeError("db_offsets must hold D + 1 entries, D >= 1")
    with on_device_of(extra_pts) as s:
        _lib.check(_lib.lib().epnet_gt_aug_points(b, e, k, d, rows, p_pt, p_of, p_db, p_mv, p_r0, p_in, o_pt, s), "gt_aug_points")
    return 1


@writes("pts_rect", "pts_intensity", "pts_origin_xy", "pts_input", "choice", "scene_info")
def scan_prepare_aug_gpu(pts_lidar, num_raw, V2C, R0, P2, img_shape, extra_pts, remove_boxes, info, keys, slot_perm, reduce_by_range,
                         scope, near_depth, pts_rect, pts_intensity, pts_origin_xy, pts_input, choice, scene_info):
    """scan_cuda.scan_prepare_gpu with extra_pts (B,E,4), remove_boxes (B,K,7) and info (B,8) int32 of gt_aug_place_gpu (columns 4
    and 7 are the counts of removal boxes and extra rows); keys (B,P+E); scene_info (B,8) int32"""
    if pts_lidar.dim() != 3 or pts_lidar.shape[2] != 4:
        raise RuntimeError("pts_lidar must be (B, P, 4)")
    if pts_rect.dim() != 3 or pts_rect.shape[2] != 3 or pts_rect.shape[0] != pts_lidar.shape[0]:
        raise RuntimeError("pts_rect must be (B, N, 3)")
    if extra_pts.dim() != 3 or extra_pts.shape[2] != 4 or remove_boxes.dim() != 3 or remove_boxes.shape[2] != 7:
        raise RuntimeError("extra_pts must be (B, E, 4) and remove_boxes (B, K, 7)")
    b, p, n, e, k = pts_lidar.shape[0], pts_lidar.shape[1], pts_rect.shape[1], extra_pts.shape[1], remove_boxes.shape[1]
    pl, pn = dev_ptr(pts_lidar, "pts_lidar", _F), dev_ptr(num_raw, "num_raw", _I)
    pv, pr, pp = dev_ptr(V2C, "V2C", _F), dev_ptr(R0, "R0", _F), dev_ptr(P2, "P2", _F)
    ps, pk = dev_ptr(img_shape, "img_shape", _I), dev_ptr(keys, "keys", _I)
    px, pb, pi = dev_ptr(extra_pts, "extra_pts", _F), dev_ptr(remove_boxes, "remove_boxes", _F), dev_ptr(info, "info", _I)
    need(num_raw, b, "num_raw"); need(V2C, b * 12, "V2C"); need(R0, b * 9, "R0"); need(P2, b * 12, "P2")
    need(img_shape, b * 2, "img_shape"); need(keys, b * (p + e), "keys")
    need(extra_pts, b * e * 4, "extra_pts"); need(remove_boxes, b * k * 7, "remove_boxes"); need(info, b * 8, "info")
    pm = None
    if slot_perm is not None:
        pm = dev_ptr(slot_perm, "slot_perm", _I)
        need(slot_perm, b * n, "slot_perm")
    o_rect, o_int, o_xy = dev_ptr(pts_rect, "pts_rect", _F), dev_ptr(pts_intensity, "pts_intensity", _F), dev_ptr(pts_origin_xy, "pts_origin_xy", _F)
    o_choice, o_info = dev_ptr(choice, "choice", _I), dev_ptr(scene_info, "scene_info", _I)
    need(pts_intensity, b * n, "pts_intensity"); need(pts_origin_xy, b * n * 2, "pts_origin_xy")
    need(choice, b * n, "choice"); need(scene_info, b * 8, "scene_info")
    o_in = None
    if pts_input is not None:
        o_in = dev_ptr(pts_input, "pts_input", _F)
        need(pts_input, b * n * 4, "pts_input")
    sc = _doubles(scope, 6, "scope")
    l = _lib.lib()
    ws_bytes = l.epnet_scan_prepare_aug_workspace_bytes(b, p, e, n)
    ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=pts_lidar.device)
    with on_device_of(pts_lidar) as s:
        _lib.check(l.epnet_scan_prepare_aug(b, p, e, n, k, int(bool(reduce_by_range)), ctypes.cast(sc, ctypes.c_void_p), float(near_depth),
                                            pl, pn, pv, pr, pp, ps, px if e else None, (pi + 28) if e else None, pb if k else None,
                                            (pi + 16) if k else None, 8, pk, pm, ws.data_ptr(), ws_bytes, o_rect, o_int, o_xy, o_in,
                                            o_choice, o_info, s), "scan_prepare_aug")
    return 1

"""Stand-in of an extension module the reference does not have: its RPN inputs are made in the loader, per scene, on the host
(lib/datasets/kitti_rcnn_dataset.py:281-356; lib/datasets/kitti_dataset.py:37-57). ``scan_prepare_gpu`` is the one call of
``epnet_scan_prepare`` and ``image_normalise_gpu`` of ``epnet_image_normalise`` (include/epnet_ops.h), on the tensors' device
and current stream, nothing read back; the workspace comes from the caching allocator.
"""
import ctypes

import torch

from . import _lib
from ._tensor import dev_ptr, need, on_device_of, writes

_F = torch.float32
_I = torch.int32


def _doubles(values, count, name):
    values = [float(v) for v in values]
    if len(values) != count:
        raise RuntimeError("%s must hold %d numbers" % (name, count))
    return (ctypes.c_double * count)(*values)


@writes("pts_rect", "pts_intensity", "pts_origin_xy", "pts_input", "choice", "scene_info")
def scan_prepare_gpu(pts_lidar, num_raw, V2C, R0, P2, img_shape, keys, slot_perm, reduce_by_range, scope, near_depth,
                     pts_rect, pts_intensity, pts_origin_xy, pts_input, choice, scene_info):
    """pts_lidar (B,P,4), num_raw (B) int32, V2C (B,3,4), R0 (B,3,3), P2 (B,3,4), img_shape (B,2) int32 [h, w], keys (B,P) int32,
    slot_perm (B,N) int32 or None; scope: 6 numbers [x0, x1, y0, y1, z0, z1] -> pts_rect (B,N,3), pts_intensity (B,N),
    pts_origin_xy (B,N,2), pts_input (B,N,4) or None, choice (B,N) int32, scene_info (B,6) int32; N is pts_rect's."""
    if pts_lidar.dim() != 3 or pts_lidar.shape[2] != 4:
        raise RuntimeError("pts_lidar must be (B, P, 4)")
    if pts_rect.dim() != 3 or pts_rect.shape[2] != 3 or pts_rect.shape[0] != pts_lidar.shape[0]:
        raise RuntimeError("pts_rect must be (B, N, 3)")
    b, p, n = pts_lidar.shape[0], pts_lidar.shape[1], pts_rect.shape[1]
    pl, pn = dev_ptr(pts_lidar, "pts_lidar", _F), dev_ptr(num_raw, "num_raw", _I)
    pv, pr, pp = dev_ptr(V2C, "V2C", _F), dev_ptr(R0, "R0", _F), dev_ptr(P2, "P2", _F)
    ps, pk = dev_ptr(img_shape, "img_shape", _I), dev_ptr(keys, "keys", _I)
    need(num_raw, b, "num_raw"); need(V2C, b * 12, "V2C"); need(R0, b * 9, "R0"); need(P2, b * 12, "P2")
    need(img_shape, b * 2, "img_shape"); need(keys, b * p, "keys")
    pm = None
    if slot_perm is not None:
        pm = dev_ptr(slot_perm, "slot_perm", _I)
        need(slot_perm, b * n, "slot_perm")
    o_rect, o_int, o_xy = dev_ptr(pts_rect, "pts_rect", _F), dev_ptr(pts_intensity, "pts_intensity", _F), dev_ptr(pts_origin_xy, "pts_origin_xy", _F)
    o_choice, o_info = dev_ptr(choice, "choice", _I), dev_ptr(scene_info, "scene_info", _I)
    need(pts_intensity, b * n, "pts_intensity"); need(pts_origin_xy, b * n * 2, "pts_origin_xy")
    need(choice, b * n, "choice"); need(scene_info, b * 6, "scene_info")
    o_in = None
    if pts_input is not None:
        o_in = dev_ptr(pts_input, "pts_input", _F)
        need(pts_input, b * n * 4, "pts_input")
    sc = _doubles(scope, 6, "scope")
    l = _lib.lib()
    ws_bytes = l.epnet_scan_prepare_workspace_bytes(b, p, n)
    ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=pts_lidar.device)
    with on_device_of(pts_lidar) as s:
        _lib.check(l.epnet_scan_prepare(b, p, n, int(bool(reduce_by_range)), ctypes.cast(sc, ctypes.c_void_p), float(near_depth), pl, pn,
                                        pv, pr, pp, ps, pk, pm, ws.data_ptr(), ws_bytes, o_rect, o_int, o_xy, o_in, o_choice, o_info, s),
                   "scan_prepare")
    return 1


@writes("out")
def image_normalise_gpu(img, img_shape, mean, std, out):
    """img (B,H,W,3) uint8, img_shape (B,2) int32 [h, w] or None, mean / std: 3 numbers each -> out (B,3,H_out,W_out) fp32"""
    if img.dim() != 4 or img.shape[3] != 3:
        raise RuntimeError("img must be (B, H, W, 3)")
    if out.dim() != 4 or out.shape[1] != 3 or out.shape[0] != img.shape[0]:
        raise RuntimeError("out must be (B, 3, H_out, W_out)")
    b, h_in, w_in, h_out, w_out = img.shape[0], img.shape[1], img.shape[2], out.shape[2], out.shape[3]
    pi, po = dev_ptr(img, "img", torch.uint8), dev_ptr(out, "out", _F)
    ps = None
    if img_shape is not None:
        ps = dev_ptr(img_shape, "img_shape", _I)
        need(img_shape, b * 2, "img_shape")
    m, d = _doubles(mean, 3, "mean"), _doubles(std, 3, "std")
    with on_device_of(img) as s:
        _lib.check(_lib.lib().epnet_image_normalise(b, h_in, w_in, h_out, w_out, pi, ps, ctypes.cast(m, ctypes.c_void_p),
                                                    ctypes.cast(d, ctypes.c_void_p), po, s), "image_normalise")
    return 1

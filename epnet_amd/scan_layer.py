"""The RPN inputs from the raw scans on the device, with no host synchronisation (reference: the first half of
get_rpn_with_li_fusion, lib/datasets/kitti_rcnn_dataset.py:281-356, per scene on a host core: Calibration.lidar_to_rect and
rect_to_img, get_valid_flag, every point at 40 m or farther plus a random subset of the nearer ones up to 16384, a shuffle; and
get_image_rgb_with_normal, lib/datasets/kitti_dataset.py:37-57, a 384 x 1280 x 3 float64 image per scene).

The loader hands over what is on disk: the ``.bin`` scans (``collate_scans`` pads them to one length), the calibration
matrices and the 8-bit image. ``draw_scan_tables`` draws the sampling keys and the shuffle on the device, ``prepare_scans`` is
ONE call of ``epnet_scan_prepare`` (csrc/scan.hip, four launches whatever the data) for the whole batch, and
``normalise_images`` one launch of ``epnet_image_normalise``. Nothing is read back, so the step can be queued behind the
previous one or captured into a HIP graph together with ``rpn_target_layer.augment_and_label`` and the loss.
get_rpn_sample (the loader without LI-Fusion) applies the same rule and does not use ``pts_origin_xy``.
"""
from types import SimpleNamespace

import numpy as np
import torch

from . import pointnet2_utils
from . import scan_cuda

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)   # lib/datasets/kitti_dataset.py:24-25
NEAR_DEPTH = 40.0                                           # kitti_rcnn_dataset.py:329
PAD_TO = 1024


def default_cfg():
    """the keys prepare_scans reads, values of lib/config.py (:25-28, :53); any object with the same attributes works"""
    return SimpleNamespace(PC_REDUCE_BY_RANGE=True, PC_AREA_SCOPE=np.array([[-40, 40], [-1, 3], [0, 70.4]], dtype=np.float64),
                           RPN=SimpleNamespace(USE_INTENSITY=True))


def _ambient_cfg():
    """the reference's global config when its module is loaded in this process, else the defaults above"""
    import sys
    ref = sys.modules.get("lib.config")
    return ref.cfg if ref is not None and hasattr(ref, "cfg") else default_cfg()


def collate_scans(scans):
    """list of (P_i,4) float32 arrays or tensors (a .bin file reshaped) -> pts_lidar (B,P,4) fp32 zero-padded CPU tensor, P the
    longest scan rounded up to a multiple of 1024, and num_raw (B) int32. Host-side padding, as collate_batch pads boxes."""
    scans = [torch.as_tensor(np.asarray(s, dtype=np.float32)) if not isinstance(s, torch.Tensor) else s.float().cpu() for s in scans]
    for s in scans:
        if s.dim() != 2 or s.shape[1] != 4:
            raise RuntimeError("a scan must be (P, 4)")
    longest = max([s.shape[0] for s in scans] + [1])
    p = (longest + PAD_TO - 1) // PAD_TO * PAD_TO
    pts = torch.zeros((len(scans), p, 4), dtype=torch.float32)
    for k, s in enumerate(scans):
        pts[k, :s.shape[0]] = s
    return pts, torch.tensor([s.shape[0] for s in scans], dtype=torch.int32)


def draw_scan_tables(batch, p, npoints=16384, generator=None, device="cuda"):
    """the draws of :332-342 for `batch` scenes of `p` raw points -> {"keys": int32 (B,P), "slot_perm": int32 (B,N)} on the
    device: one key per raw point over the full 32 bits (the r smallest keys of the candidates are a uniform r-subset, as
    np.random.choice(replace=False) draws), and a uniform permutation of the output rows (np.random.shuffle) as the argsort of
    uniform numbers. Drawn with torch on the device, nothing read back; the draws differ from numpy's stream, the rules do not."""
    keys = torch.randint(-2 ** 31, 2 ** 31, (batch, p), generator=generator, device=device, dtype=torch.int64).to(torch.int32)
    perm = torch.rand((batch, npoints), generator=generator, device=device).argsort(1).to(torch.int32)
    return {"keys": keys.contiguous(), "slot_perm": perm.contiguous()}


def _dev(t, name, dtype, shape):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s must be a CUDAtensor (epnet_amd has no CPU fallback)" % name)
    if tuple(t.shape) != tuple(shape):
        raise RuntimeError("%s must be %s, got %s" % (name, tuple(shape), tuple(t.shape)))
    return t.to(dtype).contiguous()


def prepare_scans(pts_lidar, num_raw, V2C, R0, P2, img_shape, tables, npoints=16384, cfg=None):
    """pts_lidar (B,P,4), num_raw (B), V2C (B,3,4), R0 (B,3,3), P2 (B,3,4), img_shape (B,2) [h, w], tables = draw_scan_tables'
    dict (``slot_perm`` may be None: no shuffle) -> dict of pts_rect (B,N,3), pts_features (B,N,1) = intensity - 0.5,
    pts_input (B,N,4) (= pts_rect without RPN.USE_INTENSITY, as :359-362), pts_origin_xy (B,N,2) the raw pixel coordinates,
    choice (B,N) int32 the raw row of each output row, scene_info (B,6) int32 = [num_raw, valid, far, case, r, q]
    (include/epnet_ops.h, epnet_scan_prepare: the cases 3, 4 and 5, where the reference raises, are defined there)."""
    cfg = cfg if cfg is not None else _ambient_cfg()
    if not isinstance(pts_lidar, torch.Tensor) or not pts_lidar.is_cuda:
        raise RuntimeError("pts_lidar must be a CUDAtensor (epnet_amd has no CPU fallback)")
    if pts_lidar.dim() != 3 or pts_lidar.shape[2] != 4:
        raise RuntimeError("pts_lidar must be (B, P, 4)")
    b, p, n = pts_lidar.shape[0], pts_lidar.shape[1], int(npoints)
    pts = pts_lidar.float().contiguous()
    num_raw = _dev(num_raw, "num_raw", torch.int32, (b,))
    V2C, R0, P2 = _dev(V2C, "V2C", torch.float32, (b, 3, 4)), _dev(R0, "R0", torch.float32, (b, 3, 3)), _dev(P2, "P2", torch.float32, (b, 3, 4))
    img_shape = _dev(img_shape, "img_shape", torch.int32, (b, 2))
    keys = _dev(tables["keys"], "keys", torch.int32, (b, p))
    perm = tables.get("slot_perm")
    if perm is not None:
        perm = _dev(perm, "slot_perm", torch.int32, (b, n))
    use_intensity = bool(cfg.RPN.USE_INTENSITY)
    new = pointnet2_utils._new
    pts_rect, feat, xy = new(pts, (b, n, 3)), new(pts, (b, n, 1)), new(pts, (b, n, 2))
    pts_input = new(pts, (b, n, 4)) if use_intensity else None
    choice, info = new(pts, (b, n), torch.int32), new(pts, (b, 6), torch.int32)
    scope = [float(v) for v in np.asarray(cfg.PC_AREA_SCOPE, dtype=np.float64).reshape(-1)]
    scan_cuda.scan_prepare_gpu(pts, num_raw, V2C, R0, P2, img_shape, keys, perm, bool(cfg.PC_REDUCE_BY_RANGE), scope, NEAR_DEPTH,
                               pts_rect, feat, xy, pts_input, choice, info)
    return {"pts_rect": pts_rect, "pts_features": feat, "pts_input": pts_input if use_intensity else pts_rect, "pts_origin_xy": xy,
            "choice": choice, "scene_info": info}


def normalise_images(img_u8, img_shape=None, out_hw=(384, 1280)):
    """img_u8 (B,H,W,3) uint8 RGB, img_shape (B,2) [h, w] of each scene or None (all H x W) -> (B,3,384,1280) fp32: the
    reference's ((img / 255 - mean) / std) in float64 rounded once, zero-padded, in the layout the image backbone takes"""
    if not isinstance(img_u8, torch.Tensor) or not img_u8.is_cuda:
        raise RuntimeError("img_u8 must be a CUDAtensor (epnet_amd has no CPU fallback)")
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 4 or img_u8.shape[3] != 3:
        raise RuntimeError("img_u8 must be uint8 (B, H, W, 3)")
    b = img_u8.shape[0]
    if img_shape is not None:
        img_shape = _dev(img_shape, "img_shape", torch.int32, (b, 2))
    out = torch.empty((b, 3, int(out_hw[0]), int(out_hw[1])), dtype=torch.float32, device=img_u8.device)
    scan_cuda.image_normalise_gpu(img_u8.contiguous(), img_shape, MEAN, STD, out)
    return out

"""ctypes binding of libepnet_hip.so (C ABI: include/epnet_ops.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C epnet_amd/csrc``. Loading is
lazy and LOUD: if the shared object is missing or lacks a symbol the header declares, a
RuntimeError is raised -- there is no fallback path.
"""
import contextlib
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# EPNET_HIP_LIB lets kernel experiments load an alternative build; the default is the in-tree library
LIB_PATH = os.environ.get("EPNET_HIP_LIB") or os.path.join(_HERE, "lib", "libepnet_hip.so")

_vp = ctypes.c_void_p
_i = ctypes.c_int
_f = ctypes.c_float
_d = ctypes.c_double
_sz = ctypes.c_size_t
_i64 = ctypes.c_int64

# name -> (restype, argtypes); mirrors include/epnet_ops.h one to one
SIGNATURES = {
    "epnet_abi_version": (_i, []),
    "epnet_strerror": (ctypes.c_char_p, [_i]),
    "epnet_last_hip_error": (ctypes.c_char_p, []),
    "epnet_set_tuning": (_i, [ctypes.c_char_p, _i]),
    "epnet_get_tuning": (_i, [ctypes.c_char_p, ctypes.POINTER(_i)]),
    "epnet_furthest_point_sampling": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp]),
    "epnet_gather_points": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "epnet_gather_points_grad": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "epnet_ball_query": (_i, [_i, _i, _i, _f, _i, _vp, _vp, _vp, _vp]),
    "epnet_ball_query_workspace_bytes": (_sz, [_i, _i, _i]),
    "epnet_ball_query_ws": (_i, [_i, _i, _i, _f, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "epnet_group_points": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "epnet_group_points_grad": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "epnet_group_concat": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "epnet_group_concat_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "epnet_group_concat_ws": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "epnet_group_concat_grad": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp]),
    "epnet_group_points_grad_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "epnet_group_points_grad_ws": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "epnet_group_concat_grad_ws": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "epnet_three_nn": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "epnet_three_nn_workspace_bytes": (_sz, [_i, _i, _i]),
    "epnet_three_nn_ws": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "epnet_three_interpolate": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "epnet_three_interpolate_grad": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "epnet_three_interpolate_grad_workspace_bytes": (_sz, [_i, _i, _i]),
    "epnet_three_interpolate_grad_ws": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "epnet_group_linear": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "epnet_group_linear_grad_w": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "epnet_feature_gather": (_i, [_i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "epnet_feature_gather_grad": (_i, [_i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "epnet_gather_points_grad_det_workspace_bytes": (_sz, [_i, _i, _i]),
    "epnet_gather_points_grad_det": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "epnet_group_points_grad_det_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "epnet_group_points_grad_det": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "epnet_group_concat_grad_det_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "epnet_group_concat_grad_det": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "epnet_three_interpolate_grad_det_workspace_bytes": (_sz, [_i, _i, _i]),
    "epnet_three_interpolate_grad_det": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "epnet_feature_gather_grad_det_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "epnet_feature_gather_grad_det": (_i, [_i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "epnet_group_linear_grad_w_det_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "epnet_group_linear_grad_w_det": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "epnet_pool_max": (_i, [ctypes.c_longlong, _i, _vp, _vp, _vp, _vp]),
    "epnet_pool_max_grad": (_i, [ctypes.c_longlong, _i, _vp, _vp, _vp, _vp]),
    "epnet_group_linear_h": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "epnet_pool_max_h": (_i, [ctypes.c_longlong, _i, _vp, _vp, _vp, _i, _vp]),
    "epnet_pool_max_grad_h": (_i, [ctypes.c_longlong, _i, _vp, _vp, _vp, _i, _vp]),
    "epnet_three_interpolate_h": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    "epnet_scene_index_bytes": (_sz, [_i, _i]),
    "epnet_scene_index_build": (_i, [_i, _i, _vp, _vp, _sz, _vp]),
    "epnet_scene_index_build_gathered": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "epnet_furthest_point_sampling_indexed": (_i, [_i, _i, _i, _vp, _vp, _sz, _vp, _vp, _vp]),
    "epnet_sample_centres": (_i, [_i, _i, _i, _vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "epnet_sample_centres_chain": (_i, [_i, _i, _i, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "epnet_sample_centres_chain_index": (_i, [_i, _i, _i, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "epnet_group_concat_multi": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "epnet_ball_query_indexed_multi": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "epnet_ball_query_ordered": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp]),
    "epnet_three_nn_indexed": (_i, [_i, _i, _i, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp]),
    "epnet_ball_query_indexed": (_i, [_i, _i, _i, _f, _i, _vp, _vp, _vp, _sz, _vp, _vp]),
    "epnet_boxes_overlap_bev": (_i, [_i, _vp, _i, _vp, _vp, _vp]),
    "epnet_boxes_iou_bev": (_i, [_i, _vp, _i, _vp, _vp, _vp]),
    "epnet_boxes_iou3d": (_i, [_i, _vp, _i, _vp, _vp, _vp]),
    "epnet_boxes_iou3d_pairs": (_i, [_i, _vp, _vp, _vp, _vp]),
    "epnet_aug_roi_by_noise": (_i, [_i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "epnet_rcnn_sample_rois_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "epnet_rcnn_sample_rois": (_i, [_i, _i, _i, _i, _i, _i, _f, _f, _f, _d, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp,
                                    _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "epnet_rpn_proposals_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "epnet_rpn_proposals": (_i, [_i, _i, _vp, _vp, _vp, _i, _i, _i, _f, _i, _vp, _sz, _vp, _vp, _vp, _vp]),
    "epnet_decode_bbox_target": (_i, [ctypes.c_longlong, _i, _vp, _vp, _i, _i, _i, _d, _d, _d, _d, _i, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "epnet_score_order": (_i, [_i, _i, _vp, _vp, _vp]),
    "epnet_rpn_handover_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "epnet_rpn_handover": (_i, [_i, _i, _i, _vp, _vp, _vp, _i, _i, _d, _d, _d, _d, _i, _vp, _i, _i, _i, _i, _i, _f, _i, _i, _i, _f, _i, _vp,
                                _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "epnet_rcnn_detections_workspace_bytes": (_sz, [_i, _i]),
    "epnet_rcnn_detections": (_i, [_i, _i, _vp, _vp, _vp, _f, _f, _vp, _sz, _vp, _vp, _vp, _vp]),
    "epnet_eval_recall_workspace_bytes": (_sz, [_i, _i, _i]),
    "epnet_eval_recall": (_i, [_i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "epnet_kitti_records": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "epnet_nms_workspace_bytes": (_sz, [_i]),
    "epnet_nms": (_i, [_vp, _i, _f, _vp, _sz, _vp, _vp, _vp]),
    "epnet_nms_normal": (_i, [_vp, _i, _f, _vp, _sz, _vp, _vp, _vp]),
    "epnet_roipool3d_workspace_bytes": (_sz, [_i, _i, _i]),
    "epnet_roipool3d": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "epnet_roipool3d_canonical": (_i, [_i, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    "epnet_roipool3d_train": (_i, [_i, _i, _i, _i, _i, _f, _f, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                   _vp, _vp]),
    "epnet_box_loss_workspace_bytes": (_sz, [ctypes.c_longlong, _i]),
    "epnet_box_loss": (_i, [ctypes.c_longlong, _i, _d, _d, _i, _i, _i, _i, _d, _d, _d, _d, _d, _d, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                            _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "epnet_adam_onecycle_workspace_bytes": (_sz, [ctypes.c_longlong]),
    "epnet_adam_onecycle_step": (_i, [_i, ctypes.c_longlong, ctypes.c_longlong, _vp, _vp, _vp, ctypes.c_longlong, _d, _d, _d, _i, _vp, _vp,
                                      _vp, _vp, _vp, _sz, _vp]),
    "epnet_adam_onecycle_step_scaled": (_i, [_i, ctypes.c_longlong, ctypes.c_longlong, _vp, _vp, _vp, ctypes.c_longlong, _d, _d, _d, _i, _vp,
                                             _vp, _vp, _vp, _vp, _vp, _d, _d, ctypes.c_longlong, _d, _vp, _sz, _vp]),
    "epnet_rpn_targets": (_i, [_i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "epnet_scan_prepare_workspace_bytes": (_sz, [_i, _i, _i]),
    "epnet_scan_prepare": (_i, [_i, _i, _i, _i, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "epnet_image_normalise": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "epnet_gt_aug_place": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "epnet_gt_aug_points": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "epnet_scan_prepare_aug_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "epnet_scan_prepare_aug": (_i, [_i, _i, _i, _i, _i, _i, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _sz,
                                    _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "epnet_kitti_overlaps": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "epnet_kitti_match": (_i, [_i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "epnet_kitti_pr_workspace_bytes": (_sz, [_i, _i, _i]),
    "epnet_kitti_pr": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                            _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    "epnet_image_head_points_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _i]),
    "epnet_image_head_points": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "epnet_image_head_points_h_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _i]),
    "epnet_image_head_points_h": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "epnet_sa_tail_f32": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "epnet_kitti_thresholds_host": (_i, [_vp, _i64, _i64, _i, _vp, _i, ctypes.POINTER(_i)]),
    "epnet_pts_in_boxes3d_host": (_i, [_vp, _vp, _vp, _i64, _i64]),
    "epnet_roipool3d_host": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64]),
}

_lib = None


class EpnetError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "epnet_amd: %s not found -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C epnet_amd/csrc` (there is no CPU fallback)" % LIB_PATH)
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(handle, name)
            except AttributeError:
                raise RuntimeError("epnet_amd: %s does not export %s (stale build?)" % (LIB_PATH, name))
            fn.restype = res
            fn.argtypes = args
        if handle.epnet_abi_version() != 1:
            raise RuntimeError("epnet_amd: ABI version mismatch in %s" % LIB_PATH)
        _lib = handle
    return _lib


def check(code, what):
    """turn a non-zero C-ABI return code into a Python exception (the reference exit()s instead)."""
    if code != 0:
        l = lib()
        msg = l.epnet_strerror(code).decode()
        hip = l.epnet_last_hip_error().decode()
        raise EpnetError("%s failed: %s%s" % (what, msg, (" [" + hip + "]") if (code == -2 and hip) else ""))


@contextlib.contextmanager
def tuning(**overrides):
    """kernel-selection overrides for the body, by the names of the EPNET_* variables (-1 = the library's own choice), e.g.
    ``with tuning(EPNET_BQ_PAIR=1): ...``; the previous values come back on exit, also when the body raises. An unknown name
    or a value out of range raises, so that a typo cannot quietly test the default kernel."""
    l = lib()
    saved = []
    try:
        for name, value in overrides.items():
            old = _i()
            check(l.epnet_get_tuning(name.encode(), ctypes.byref(old)), "epnet_get_tuning(%s)" % name)
            check(l.epnet_set_tuning(name.encode(), int(value)), "epnet_set_tuning(%s, %r)" % (name, value))
            saved.append((name, old.value))
        yield
    finally:
        for name, old in reversed(saved):
            l.epnet_set_tuning(name.encode(), old)

"""Every device implementation of a rotated-rectangle intersection against exact float64 geometry (tests/exact_geometry.py):
pairwise_bev_kernel, iou3d_matrix_kernel / iou3d_pairs_kernel, rcnn_iou_kernel (inside epnet_rcnn_sample_rois), the evaluator's
own intersection (kitti_eval.hip) and nms_mask_rot_kernel (through the keep list of epnet_nms).

Bounds. Areas: B_IOU3D and B_EVAL, measured on the CPU (exact_geometry.py). Ratios: the area bound mapped through the
denominator by exact_geometry.ratio_tolerance / iou3d_tolerance, which hold the derivation. Decisions (the best ground truth of
a ROI, an NMS keep list) are compared only where exact geometry is further from the decision than that tolerance; that enough
such rows and thresholds exist is checked on the CPU (tests/test_exact_geometry.py). The degenerate families, where the
reference's arithmetic itself leaves geometry, are held to the oracle / the restatement at the project's 1e-5.
Each test prints the largest distance it saw next to its bound."""
import functools

import numpy as np
import pytest
import torch

import exact_geometry as eg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F = np.float32
PROJECT_TOL = 1e-5


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().cpu().numpy()


def report(path, case, worst, bound):
    print("exact-geometry %-28s %-14s max distance %.3e  bound %.3e" % (path, case, worst, bound))


def pairwise(fn_name, a, b):
    from epnet_amd import iou3d_cuda
    out = torch.full((a.shape[0], b.shape[0]), float("nan"), device=DEV)
    getattr(iou3d_cuda, fn_name)(dev(a), dev(b), out)
    return host(out).astype(np.float64)


@functools.lru_cache(maxsize=None)
def bev_reference(name):
    a, b = eg.matrix_case(name)
    return a, b, eg.overlap_bev(a, b), eg.iou_bev(a, b)


@functools.lru_cache(maxsize=None)
def iou3d_reference(name):
    a, b = eg.matrix_case(name, lifted=True)
    return a, b, eg.iou3d(a, b)


# ---- boxes_overlap_bev_gpu, boxes_iou_bev_gpu --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", eg.NON_DEGENERATE)
def test_bev_overlap_and_iou(hiplib, name):
    a, b, want_ov, want_iou = bev_reference(name)
    got_ov, got_iou = pairwise("boxes_overlap_bev_gpu", a, b), pairwise("boxes_iou_bev_gpu", a, b)
    tol = eg.iou_tolerance(a, b)
    worst_ov, worst_iou = np.abs(got_ov - want_ov).max(), np.abs(got_iou - want_iou).max()
    report("boxes_overlap_bev_gpu", name, worst_ov, eg.B_IOU3D)
    report("boxes_iou_bev_gpu", name, worst_iou, tol)
    assert (want_ov > 0).sum() >= 100 or name in ("aa_touching", "far")          # the matrix is not a table of zeros
    assert worst_ov <= eg.B_IOU3D and worst_iou <= tol


# ---- boxes_iou3d_fused_gpu, boxes_iou3d_pairs_gpu ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", eg.NON_DEGENERATE)
def test_iou3d_matrix_and_pairs(hiplib, name):
    from epnet_amd import iou3d_cuda
    a, b, want = iou3d_reference(name)
    tol = eg.iou3d_tolerance(a, b)
    got = pairwise("boxes_iou3d_fused_gpu", a, b)
    worst = np.abs(got - want).max()
    report("boxes_iou3d_fused_gpu", name, worst, tol)
    pa, pb = eg.pairs_case(name)
    out = torch.full((pa.shape[0],), float("nan"), device=DEV)
    iou3d_cuda.boxes_iou3d_pairs_gpu(dev(pa), dev(pb), out)
    want_pairs, tol_pairs = eg.iou3d(pa, pb, pairs=True), eg.iou3d_tolerance(pa, pb)
    worst_pairs = np.abs(host(out) - want_pairs).max()
    report("boxes_iou3d_pairs_gpu", name, worst_pairs, tol_pairs)
    assert (want_pairs > 0).mean() > 0.5 or name in ("aa_touching", "far")       # heights and rectangles really overlap
    assert worst <= tol and worst_pairs <= tol_pairs


# ---- rcnn_sample_rois_gpu: max_overlaps, gt_assignment ------------------------------------------------------------------------------
def test_rcnn_sampling_overlaps_and_assignment(hiplib):
    from epnet_amd import rcnn_target_layer as rtl
    rois, gts = eg.rcnn_case()
    rng = np.random.RandomState(3)
    cfg = rtl.default_cfg()
    cfg.RCNN.ROI_PER_IMAGE, cfg.RCNN.ROI_FG_AUG_TIMES = 16, 0
    tables = {"fg_key": dev(rng.rand(2, eg.RCNN_M).astype(F)), "slot_u": dev(rng.rand(2, 16).astype(F)), "keep_draw": None, "noise": None}
    info, d = rtl.sample_rois(dev(rois), dev(gts), tables, cfg, details=True)[3:5]
    torch.cuda.synchronize()
    assert host(info)[:, 0].tolist() == list(eg.RCNN_VALID)
    left_out = 0
    for k, valid in enumerate(eg.RCNN_VALID):
        want = eg.iou3d(rois[k], gts[k, :valid])
        tol = eg.iou3d_tolerance(rois[k], gts[k, :valid])
        worst = np.abs(host(d["max_overlaps"])[k] - want.max(axis=1)).max()
        report("rcnn_sample_rois max_overlaps", "scene %d" % k, worst, tol)
        assert worst <= tol
        top = np.sort(want, axis=1)
        decided = top[:, -1] - top[:, -2] > 2 * tol
        left_out += int((~decided).sum())
        assert np.array_equal(host(d["gt_assignment"])[k][decided], want.argmax(axis=1)[decided])
    print("rows without a decided best ground truth: %d of %d" % (left_out, 2 * eg.RCNN_M))
    assert left_out <= 0.02 * 2 * eg.RCNN_M


# ---- kitti_overlaps_gpu ------------------------------------------------------------------------------------------------------------
def offsets(counts, dtype=np.int32):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(dtype)


def kitti_overlaps(metric, rows, cols):
    """per-frame (rows_f, cols_f) blocks of epnet_kitti_overlaps through the offset tables"""
    from epnet_amd import kitti_eval_cuda, pointnet2_utils
    nr, nc = [len(r) for r in rows], [len(c) for c in cols]
    ov_off = offsets([a * b for a, b in zip(nr, nc)], np.int64)
    row_boxes, col_boxes = dev(np.concatenate(rows)), dev(np.concatenate(cols))
    out = pointnet2_utils._new(row_boxes, (int(ov_off[-1]),), torch.float64)
    out.fill_(float("nan"))
    kitti_eval_cuda.kitti_overlaps_gpu(metric, -1, max(nr), max(nc), dev(offsets(nr)), dev(offsets(nc)), dev(ov_off), row_boxes, col_boxes, out)
    flat = host(out)
    return [flat[ov_off[f]:ov_off[f + 1]].reshape(nr[f], nc[f]) for f in range(len(rows))]


@pytest.mark.parametrize("name", eg.NON_DEGENERATE_EVAL)
def test_kitti_overlaps_bev_and_3d(hiplib, name):
    """criterion -1, the only one the entry point serves for the rotated metrics (0 and 1 are held to geometry on the
    restatement, tests/test_exact_geometry.py)"""
    rows, cols = eg.eval_frames(name)
    area = min(np.concatenate(rows)[:, 2:4].prod(axis=1).min(), np.concatenate(cols)[:, 2:4].prod(axis=1).min())
    tol = eg.ratio_tolerance(eg.B_EVAL, area)
    got = kitti_overlaps(1, rows, cols)
    worst = max(np.abs(g - eg.eval_bev(r, c, -1)).max() for g, r, c in zip(got, rows, cols) if g.size)
    report("kitti_overlaps metric 1", name, worst, tol)
    rows7, cols7 = eg.eval_frames(name, lifted=True)
    tol7 = eg.iou3d_tolerance(np.concatenate(rows7), np.concatenate(cols7), bound=eg.B_EVAL, columns=(3, 4, 5), height=4)
    got7 = kitti_overlaps(2, rows7, cols7)
    worst7 = max(np.abs(g - eg.eval_3d(r, c)).max() for g, r, c in zip(got7, rows7, cols7) if g.size)
    report("kitti_overlaps metric 2", name, worst7, tol7)
    assert [g.shape for g in got] == [tuple(s) for s in eg.EVAL_FRAMES]
    assert worst <= tol and worst7 <= tol7


# ---- rotated NMS against greedy NMS on the exact IoU matrix ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,seed", eg.NMS_CASES)
def test_rotated_nms_against_exact_greedy(hiplib, name, n, seed):
    from epnet_amd import iou3d_cuda
    boxes = eg.nms_case(name, n, seed)
    iou = eg.iou_bev(boxes, boxes)
    tol = eg.iou_tolerance(boxes, boxes)
    boxes_dev = dev(boxes)
    for start in eg.NMS_STARTS:
        thresh = eg.clear_threshold(iou, start, tol)
        assert thresh is not None, ("no threshold clear of every exact IoU", name, n, seed, start)
        keep, num = iou3d_cuda.nms_device(boxes_dev, thresh)
        want = eg.greedy_nms(iou, thresh)
        got = host(keep)[:int(num.item())]
        print("nms_device %s n=%d thresh %.4f: kept %d" % (name, n, thresh, len(got)))
        assert np.array_equal(got, want), (name, n, thresh)


# ---- the degenerate families: the reference's arithmetic, not geometry -------------------------------------------------------------------
@pytest.mark.parametrize("name", eg.DEGENERATE)
def test_degenerate_pairs_follow_the_oracle(hiplib, oracle, name):
    from epnet_amd import iou3d_cuda
    a, b = (eg.bev_of_centre(v) for v in eg.family_pairs(name, eg.N_PAIRS, eg.DEGENERATE_SEED_IOU3D[name]))
    chunks = range(0, eg.N_PAIRS, 250)
    on_pairs = np.concatenate([np.diagonal(oracle.boxes_overlap_bev(a[k:k + 250], b[k:k + 250])) for k in chunks])
    beyond = np.nonzero(np.abs(on_pairs - eg.overlap_bev_pairs(a, b)) > eg.B_IOU3D)[0]
    assert beyond.size > 0                                                        # the pairs the oracle itself loses are in the set
    sel = np.union1d(np.arange(0, eg.N_PAIRS, 16), beyond)                        # pair i sits on the diagonal of a[sel] x b[sel]
    got = pairwise("boxes_overlap_bev_gpu", a[sel], b[sel])
    worst = np.abs(got - oracle.boxes_overlap_bev(a[sel], b[sel])).max()
    assert not np.diagonal(got)[np.searchsorted(sel, beyond)].any()               # the device loses the same pairs
    # all 2000 pairs as 7-column boxes of equal height through the pairs kernel
    a7 = np.stack([(a[:, 0] + a[:, 2]) / 2, np.full(len(a), 2, F), (a[:, 1] + a[:, 3]) / 2, np.full(len(a), 1, F), a[:, 3] - a[:, 1],
                   a[:, 2] - a[:, 0], a[:, 4]], axis=1).astype(F)
    b7 = a7.copy()
    b7[:, 6] = b[:, 4]
    out = torch.full((len(a7),), float("nan"), device=DEV)
    iou3d_cuda.boxes_iou3d_pairs_gpu(dev(a7), dev(b7), out)
    want_pairs = np.concatenate([np.diagonal(oracle.boxes_iou3d(a7[k:k + 250], b7[k:k + 250])) for k in chunks])
    worst_pairs = np.abs(host(out) - want_pairs).max()
    report("degenerate vs oracle", name, max(worst, worst_pairs), PROJECT_TOL)
    assert worst <= PROJECT_TOL and worst_pairs <= PROJECT_TOL


@pytest.mark.parametrize("name", eg.DEGENERATE_EVAL)
def test_degenerate_pairs_follow_the_restatement(hiplib, name):
    import kitti_eval_restate as kr
    rows, cols = eg.eval_frames(name, eg.EVAL_FRAMES_SMALL)
    got = kitti_overlaps(1, rows, cols)
    worst = max(np.abs(g - kr.rotate_iou_eval(r, c, -1)).max() for g, r, c in zip(got, rows, cols) if g.size)
    rows7, cols7 = eg.eval_frames(name, eg.EVAL_FRAMES_SMALL, lifted=True)
    got7 = kitti_overlaps(2, rows7, cols7)
    worst7 = max(np.abs(g - kr.d3_box_overlap(r, c)).max() for g, r, c in zip(got7, rows7, cols7) if g.size)
    report("degenerate vs restatement", name, max(worst, worst7), PROJECT_TOL)
    assert worst <= PROJECT_TOL and worst7 <= PROJECT_TOL

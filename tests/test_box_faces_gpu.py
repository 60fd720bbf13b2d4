"""Point-in-box membership ON the box faces, in every kernel that decides it: roipool3d.hip (plain, canonical, training),
targets.hip (the box and the enlarged "ignore" box) and scan.hip (in_remove_box).

The clouds are those of tests/box_faces.py: points built on all six faces of rotated boxes and stepped ulp by ulp across them,
the ones on which a decision hangs kept first -- points whose float32 x_rot, z_rot or |y - cy| EQUALS the bound, and points that
change sides when a product is fused into the sum. tests/test_box_faces.py asserts, without a kernel, that every case holds at
least 100 of the former and 30 of the latter, and that the restatement agrees with the CPU oracle and the host ops on all of them.

Bounds. Every membership comparison is BIT-EXACT and covers ALL points: no band, no exclusions. What the training mode computes
beyond the choice of rows (augmented and canonical coordinates, boxes) is held to tests/rcnn_targets_restate.py within
rtol 1e-5, atol 5e-5, as tests/test_rcnn_targets_gpu.py holds it. A NaN compares equal to a NaN."""
import numpy as np
import pytest
import torch

import box_faces as bf
import gt_aug_restate as gr
import rcnn_targets_restate as rr
import rpn_targets_restate as rs
import scan_restate as sr
from detections_restate import canonical_xyz

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F = np.float32
TOL = dict(rtol=1e-5, atol=5e-5)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().cpu().numpy()


def differing(got, want):
    """the number of elements whose bits differ (a NaN equals a NaN)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind == "f":
        same = (got.view(np.int32) == want.view(np.int32)) | (np.isnan(got) & np.isnan(want))
    else:
        same = got == want
    return int((~same).sum())


def enlarged(rois, extra):
    from epnet_amd import kitti_utils
    if not extra:
        return rois
    return kitti_utils.enlarge_box3d(torch.from_numpy(rois).view(-1, 7), extra).view(rois.shape).numpy()


@pytest.fixture(scope="module")
def oracle_pools(oracle):
    """oracle.roipool3d of every (extra, S), computed once and shared"""
    cache = {}

    def get(extra, S):
        if (extra, S) not in cache:
            case = bf.pool_case(extra)
            pooled, flag = oracle.roipool3d(case["xyz"], enlarged(case["boxes"], extra), case["feat"], S)
            pooled.setflags(write=False)
            flag.setflags(write=False)
            cache[(extra, S)] = (pooled, flag)
        return cache[(extra, S)]
    return get


# ---- roipool3d ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", (16, 512))
def test_plain_pooling_on_the_faces(hiplib, oracle_pools, S):
    """roipool3d_cuda.forward: b = 2, n = 4000 (more than one sweep of 4 waves x 8 chunks x 64 points), 14 boxes, face points at
    seeded rows all over the cloud; the feature is the row number, so the feature column lists the chosen rows. S = 16 truncates
    among face points, S = 512 pads cyclically; the last box holds two points, both on a face"""
    from epnet_amd import roipool3d_cuda
    case = bf.pool_case(0.0)
    b, m = case["boxes"].shape[:2]
    pooled, flag = torch.zeros((b, m, S, 4), device=DEV), torch.zeros((b, m), dtype=torch.int32, device=DEV)
    roipool3d_cuda.forward(dev(case["xyz"]), dev(case["boxes"]), dev(case["feat"]), pooled, flag)
    want, want_flag = oracle_pools(0.0, S)
    assert want_flag[:, -1].tolist() == [0, 0] and want_flag.sum() >= 2 * b          # the two-member box; far and degenerate boxes are empty
    bad = (differing(host(pooled)[..., 3], want[..., 3]), differing(host(flag), want_flag), differing(host(pooled), want))
    assert bad == (0, 0, 0), "roipool3d plain S=%d: %d chosen rows, %d flags, %d elements differ" % ((S,) + bad)


@pytest.mark.parametrize("extra", (0.2, 1.0))
@pytest.mark.parametrize("S", (16, 512))
def test_canonical_pooling_on_the_faces_of_the_enlarged_boxes(hiplib, oracle_pools, extra, S):
    from epnet_amd import roipool3d_cuda
    case = bf.pool_case(extra)
    b, m = case["boxes"].shape[:2]
    pooled, flag = torch.full((b, m, S, 4), 7.0, device=DEV), torch.full((b, m), 7, dtype=torch.int32, device=DEV)
    roipool3d_cuda.forward_canonical(dev(case["xyz"]), dev(case["boxes"]), dev(case["feat"]), extra, pooled, flag)
    want, want_flag = oracle_pools(extra, S)
    assert want_flag[:, -1].tolist() == [0, 0]
    with np.errstate(invalid="ignore", over="ignore"):
        want_xyz = canonical_xyz(want[..., 0:3], case["boxes"])
    got = host(pooled)
    bad = (differing(got[..., 3], want[..., 3]), differing(host(flag), want_flag), differing(got[..., 0:3], want_xyz))
    assert bad == (0, 0, 0), "roipool3d canonical e=%g S=%d: %d chosen rows, %d flags, %d coordinates differ" % ((extra, S) + bad)


@pytest.mark.parametrize("with_aug", (False, True))
@pytest.mark.parametrize("S", (16, 512))
def test_training_pooling_on_the_faces_of_the_enlarged_boxes(hiplib, oracle_pools, S, with_aug):
    """forward_train: membership is decided on the ROI as given, with or without an augmentation table -- the chosen rows are the
    canonical mode's; everything else against rcnn_targets_restate.pool_train"""
    from epnet_amd import roipool3d_cuda
    extra = 0.2
    case = bf.pool_case(extra)
    b, m = case["boxes"].shape[:2]
    rng = np.random.default_rng(5 + S)
    rois = case["boxes"]
    gt = (rois + rng.normal(size=rois.shape) * [0.3, 0.1, 0.3, 0.05, 0.05, 0.1, 0.2]).astype(F)
    iou = rng.uniform(0, 1, (b, m)).astype(F)
    aug = None
    if with_aug:
        aug = np.stack([rng.uniform(-np.pi / 18, np.pi / 18, (b, m)), rng.uniform(0.95, 1.05, (b, m)), np.where(rng.uniform(size=(b, m)) < 0.5, -1.0, 1.0)],
                       axis=2).astype(F)
    i32 = torch.int32
    fill = lambda shape, dtype=torch.float32: torch.full(shape, 7, dtype=dtype, device=DEV)  # noqa: E731
    out = {"sampled_pts": fill((b * m, S, 3)), "pts_feature": fill((b * m, S, 1)), "roi_boxes3d": fill((b * m, 7)), "gt_of_rois": fill((b * m, 7)),
           "cls_label": fill((b * m,), i32), "reg_valid_mask": fill((b * m,), i32), "mask_score": fill((b * m,)), "pooled_empty_flag": fill((b, m), i32)}
    roipool3d_cuda.forward_train(dev(case["xyz"]), dev(case["feat"]), dev(rois), dev(gt), dev(iou), None if aug is None else dev(aug), extra, 0.55, 0.6, 0.45,
                                 *[out[k] for k in ("sampled_pts", "pts_feature", "roi_boxes3d", "gt_of_rois", "cls_label", "reg_valid_mask", "mask_score",
                                                    "pooled_empty_flag")])
    got = {k: host(v) for k, v in out.items()}
    pooled, flag = oracle_pools(extra, S)
    bad = (differing(got["pts_feature"].reshape(b, m, S), pooled[..., 3]), differing(got["pooled_empty_flag"], flag))
    assert bad == (0, 0), "roipool3d train S=%d aug=%d: %d chosen rows, %d flags differ" % ((S, with_aug) + bad)
    with np.errstate(invalid="ignore", over="ignore"):
        want = rr.pool_train(case["xyz"], case["feat"], rois, gt, iou, aug, extra, 0.55, 0.6, 0.45, S, precise=True)
    for key in ("cls_label", "reg_valid_mask"):
        assert np.array_equal(got[key], want[key]), key
    for key in ("sampled_pts", "mask_score"):
        np.testing.assert_allclose(got[key], want[key], err_msg=key, **TOL)
    for key in ("roi_boxes3d", "gt_of_rois"):      # ry is an angle: equal modulo 2 pi (a box with ry = 0 may come out a rounding below 0)
        np.testing.assert_allclose(got[key][:, 0:6], want[key][:, 0:6], err_msg=key, **TOL)
        turn = (got[key][:, 6].astype(np.float64) - want[key][:, 6] + np.pi) % (2 * np.pi) - np.pi
        assert np.abs(turn).max() <= 5e-5, key
    if aug is None:
        assert got["roi_boxes3d"].tobytes() == rois.reshape(-1, 7).tobytes()


# ---- RPN targets ------------------------------------------------------------------------------------------------------------------------
def run_targets(case):
    from epnet_amd import rpn_target_layer as rtl
    if case["aug"] is None:
        cls, reg = rtl.rpn_training_labels(dev(case["pts"]), dev(case["gt"]), bf.RPN_EXTRA)
        return case["pts"], case["gt"], host(cls), host(reg)
    return tuple(host(t) for t in rtl.augment_and_label(dev(case["pts"]), dev(case["gt"]), dev(case["alpha"]), dev(case["aug"]), bf.RPN_EXTRA))


@pytest.mark.parametrize("with_aug", (False, True))
@pytest.mark.parametrize("n", bf.RPN_N)
@pytest.mark.parametrize("g", bf.RPN_G)
def test_rpn_labels_on_the_faces(hiplib, g, n, with_aug):
    """face points on the box and on the enlarged box of boxes on either side of the 64-box chunk, some of them in two overlapping
    boxes; n % 4 != 0 takes the scalar path, n = 3001 spans three tiles; cls and reg BYTEWISE equal to labels32 of the kernel's own
    pts_out / gt_out (the labels are defined on those)"""
    case = bf.rpn_case(g, n, with_aug)
    pts_out, gt_out, cls, reg = run_targets(case)
    assert cls.dtype == np.int32 and cls.shape == (bf.RPN_B, n) and reg.shape == (bf.RPN_B, n, 7)
    bad_cls = bad_reg = 0
    twice = 0
    for s in range(bf.RPN_B):
        with np.errstate(invalid="ignore", over="ignore"):
            want_cls, want_reg = rs.labels32(pts_out[s], gt_out[s], bf.RPN_EXTRA)
            if with_aug:                                                        # the augmentation itself, by the fixture's bounds
                want_pts, want_gt = rs.augment(case["pts"][s], case["gt"][s], case["alpha"][s], case["aug"][s])
                ok = np.isfinite(want_pts).all(axis=1)
                bad = rs.augmentation_failures(s, pts_out[s][ok], gt_out[s], want_pts[ok], want_gt)
                assert not bad and np.array_equal(np.isfinite(pts_out[s]).all(axis=1), ok), bad
        bad_cls += differing(cls[s], want_cls)
        bad_reg += int((reg[s].view(np.int32) != want_reg.view(np.int32)).any(axis=1).sum())
        assert (want_cls == 1).any() and (want_cls == -1).any() and (want_cls == 0).any()
        if g > 1:
            inside = np.stack([bf.membership32(pts_out[s], b, gate=False, cy=b[1] - b[3] / F(2))[0] for b in gt_out[s][:2]])
            twice += int(inside.all(axis=0).sum())
    assert g == 1 or twice > 0                                                  # points in two boxes: the later one decides
    assert (bad_cls, bad_reg) == (0, 0), "rpn targets g=%d n=%d aug=%d: %d classes, %d regression rows differ" % (g, n, with_aug, bad_cls, bad_reg)


# ---- scan removal -----------------------------------------------------------------------------------------------------------------------
def test_scan_removal_on_the_faces(hiplib):
    """scan_prepare_aug_gpu: p = 3000 lidar rows whose rectified values stand on the faces of k = 3 removal boxes; the removed
    count, the choice and every output against gt_aug_restate.prepare_aug"""
    from epnet_amd import gt_aug_cuda
    scenes = bf.scan_case()
    b, p, n, e, k = len(scenes), bf.SCAN_P, bf.SCAN_N, bf.SCAN_E, bf.SCAN_K
    stack = lambda key, dtype: np.stack([np.asarray(s[key], dtype) for s in scenes])  # noqa: E731
    info = np.zeros((b, 8), np.int32)
    info[:, 4], info[:, 7] = k, [s["num_extra"] for s in scenes]
    z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=DEV)  # noqa: E731
    outs = [z((b, n, 3)), z((b, n, 1)), z((b, n, 2)), z((b, n, 4)), z((b, n), torch.int32), z((b, 8), torch.int32)]
    gt_aug_cuda.scan_prepare_aug_gpu(dev(stack("pts", F)), dev(stack("num_raw", np.int32)), dev(stack("V2C", F)), dev(stack("R0", F)), dev(stack("P2", F)),
                                     dev(stack("img_shape", np.int32)), dev(stack("extra_pts", F)), dev(stack("remove_boxes", F)), dev(info),
                                     dev(stack("keys", np.int32)), dev(stack("slot_perm", np.int32)), True, sr.SCOPE.reshape(-1), 40.0, *outs)
    got = dict(zip(("pts_rect", "pts_intensity", "pts_origin_xy", "pts_input", "choice", "scene_info"), (host(o) for o in outs)))
    got["pts_intensity"] = got["pts_intensity"].reshape(b, n)
    bad = {}
    for i, s in enumerate(scenes):
        want = gr.prepare_aug(s["pts"], s["num_raw"], s["V2C"], s["R0"], s["P2"], s["img_shape"], s["extra_pts"], s["num_extra"], s["remove_boxes"], k,
                              s["keys"], s["slot_perm"], n)
        assert want["scene_info"][6] >= 500 and want["scene_info"][1] > n      # hundreds of face points are removed; the rest are sampled
        for key in got:
            count = differing(got[key][i], want[key])
            if count:
                bad[(i, key)] = (count, int(got["scene_info"][i, 6]), int(want["scene_info"][6]))
    assert not bad, "scan removal: elements that differ, removed count got / want: %s" % bad


# ---- one cloud, every family --------------------------------------------------------------------------------------------------------------
def test_the_three_families_hold_the_same_points(hiplib):
    """plain roipool3d, scan removal and the RPN targets on one cloud and one box set (extra = 0, every point within 10 m of the
    centres, so the gate does not tell them apart): the same member set per box, which is membership32's"""
    from epnet_amd import gt_aug_cuda, roipool3d_cuda, rpn_target_layer as rtl
    case = bf.cross_case()
    pts, boxes = case["pts"], case["boxes"]
    n, m = len(pts), len(boxes)
    want = [set(np.nonzero(bf.membership32(pts, box)[0])[0].tolist()) for box in boxes]
    assert all(100 < len(w) < n for w in want)
    # roipool3d: S = n rows per box, the feature is the row number
    pooled, flag = torch.zeros((1, m, n, 4), device=DEV), torch.zeros((1, m), dtype=torch.int32, device=DEV)
    roipool3d_cuda.forward(dev(pts[None]), dev(boxes[None]), dev(np.arange(n, dtype=F)[None, :, None]), pooled, flag)
    pool_sets = [set(host(pooled)[0, k, :, 3].astype(np.int64).tolist()) for k in range(m)]
    assert not host(flag).any()
    # RPN targets: one scene per box
    cls, _ = rtl.rpn_training_labels(dev(np.broadcast_to(pts, (m, n, 3))), dev(boxes[:, None, :]), 0.2)
    rpn_sets = [set(np.nonzero(host(cls)[k] == 1)[0].tolist()) for k in range(m)]
    # scan removal: one scene per box under the identity calibration; n output rows for n points, so every kept row is chosen
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(F)
    P2 = np.array([[1, 0, 1000, 0], [0, 1, 1000, 0], [0, 0, 1, 0]], F)
    rep = lambda a: dev(np.broadcast_to(a, (m,) + a.shape))  # noqa: E731
    info = np.zeros((m, 8), np.int32)
    info[:, 4] = 1
    z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=DEV)  # noqa: E731
    outs = [z((m, n, 3)), z((m, n, 1)), z((m, n, 2)), z((m, n, 4)), z((m, n), torch.int32), z((m, 8), torch.int32)]
    lidar = np.concatenate([pts, np.zeros((n, 1), F)], axis=1)
    gt_aug_cuda.scan_prepare_aug_gpu(rep(lidar), dev(np.full(m, n, np.int32)), rep(eye), rep(np.eye(3, dtype=F)), rep(P2), rep(np.array([2000, 2000], np.int32)),
                                     z((m, 0, 4)), dev(boxes[:, None, :]), dev(info), z((m, n), torch.int32), None, False, sr.SCOPE.reshape(-1), 40.0, *outs)
    choice, scene_info = host(outs[4]), host(outs[5])
    scan_sets = [set(range(n)) - set(choice[k].tolist()) for k in range(m)]
    assert (scene_info[:, 0] == n).all() and all(scene_info[k, 1] + scene_info[k, 6] == n for k in range(m))      # every row is valid or removed
    bad = [(k, len(want[k]), len(pool_sets[k] ^ want[k]), len(rpn_sets[k] ^ want[k]), len(scan_sets[k] ^ want[k])) for k in range(m)
           if not (pool_sets[k] == rpn_sets[k] == scan_sets[k] == want[k])]
    assert not bad, "box, members, points that differ in roipool3d / rpn targets / scan removal: %s" % bad

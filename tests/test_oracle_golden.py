"""The oracle against (i) the reference's own compiled roipool3d CPU ops -- through the committed fixtures captured from that
build everywhere, and live where the build is at hand -- and (iii) against the fixtures captured by running the reference's
Python surface (tests/golden/make_golden.py)."""
import os

import numpy as np

from conftest import golden


def test_roipool3d_fixture_from_reference_build(oracle):
    fx = golden("roipool3d_ref.npz")
    n = fx["pts"].shape[0]
    flags = np.unpackbits(fx["pts_flag"], axis=1)[:, :n].astype(np.int64)
    np.testing.assert_array_equal(oracle.pts_in_boxes3d(fx["pts"], fx["boxes3d"]), flags)
    pp, pf, ef = oracle.roipool3d_cpu(fx["pts"], fx["boxes3d"], fx["pts_feature"], fx["pooled_pts"].shape[1])
    np.testing.assert_array_equal(pp, fx["pooled_pts"])
    np.testing.assert_array_equal(pf, fx["pooled_features"])
    np.testing.assert_array_equal(ef, fx["pooled_empty_flag"])
    # the device-flavoured restatement (roipool3d_kernel.cu) must agree with the CPU one on the same boxes
    pooled, flag = oracle.roipool3d(fx["pts"][None], fx["boxes3d"][None], fx["pts_feature"][None], fx["pooled_pts"].shape[1])
    np.testing.assert_array_equal(flag[0], fx["pooled_empty_flag"].astype(np.int32))
    np.testing.assert_array_equal(pooled[0, :, :, :3], fx["pooled_pts"])
    np.testing.assert_array_equal(pooled[0, :, :, 3:], fx["pooled_features"])


def test_oracle_vs_live_reference_build(oracle):
    """three random scenes through the reference's compiled ops, stored by tests/golden/make_golden_roipool3d_trials.py; where
    that build is at hand (oracle/_ref/), it runs again live on the same inputs"""
    import torch
    from oracle import build_ref
    fx = golden("roipool3d_ref_trials.npz")
    ref = build_ref.load() if (os.path.exists(build_ref.OUT) or build_ref.available()) else None
    for trial in range(3):
        pts, boxes, feat = fx["pts_%d" % trial], fx["boxes3d_%d" % trial], fx["pts_feature_%d" % trial]
        m, n, c, s = boxes.shape[0], pts.shape[0], feat.shape[1], fx["pooled_pts_%d" % trial].shape[1]
        flag = np.unpackbits(fx["pts_flag_%d" % trial], axis=1)[:, :n].astype(np.int64)
        pp, pf, ef = fx["pooled_pts_%d" % trial], fx["pooled_features_%d" % trial], fx["pooled_empty_flag_%d" % trial]
        if ref is not None:
            live = torch.zeros((m, n), dtype=torch.int64)
            ref.pts_in_boxes3d_cpu(live, torch.from_numpy(pts), torch.from_numpy(boxes))
            np.testing.assert_array_equal(live.numpy(), flag)
            lp, lf, le = torch.zeros((m, s, 3)), torch.zeros((m, s, c)), torch.zeros(m, dtype=torch.int64)
            ref.roipool3d_cpu(torch.from_numpy(pts), torch.from_numpy(boxes), torch.from_numpy(feat), lp, lf, le)
            np.testing.assert_array_equal(lp.numpy(), pp)
            np.testing.assert_array_equal(lf.numpy(), pf)
            np.testing.assert_array_equal(le.numpy(), ef)
        np.testing.assert_array_equal(flag, oracle.pts_in_boxes3d(pts, boxes))
        assert flag.sum() > 0
        a, b, e = oracle.roipool3d_cpu(pts, boxes, feat, s)
        np.testing.assert_array_equal(pp, a)
        np.testing.assert_array_equal(pf, b)
        np.testing.assert_array_equal(ef, e)


def test_cfg1_fixture(oracle):
    """BASELINE config 1: 4096-pt cloud, npoint 1024, nsample 32 -- index bit-exactness on the CPU path"""
    fx = golden("pointnet2_cfg1.npz")
    xyz = fx["xyz"]
    idx = oracle.furthest_point_sampling(xyz, 1024)
    np.testing.assert_array_equal(idx, fx["fps_idx"])
    new_xyz = oracle.gather_points(np.ascontiguousarray(xyz.transpose(0, 2, 1)), idx).transpose(0, 2, 1)
    np.testing.assert_array_equal(new_xyz, fx["new_xyz"])
    np.testing.assert_array_equal(oracle.ball_query(0.1, 32, xyz, new_xyz), fx["ball_idx_r01"])
    bq = oracle.ball_query(2.0, 32, xyz, new_xyz)
    np.testing.assert_array_equal(bq, fx["ball_idx_r20"])
    grouped = oracle.group_points(np.ascontiguousarray(xyz.transpose(0, 2, 1)), bq)
    np.testing.assert_array_equal(grouped - new_xyz.transpose(0, 2, 1)[..., None], fx["query_and_group_r20"])
    # every centre is a cloud point -> it is inside its own ball (d2 = 0 < r2)
    assert (fx["ball_idx_r20"] != 0).any() and len(set(fx["fps_idx"][0].tolist())) == 1024


def test_fps_tie_fixture(oracle):
    fx = golden("fps_ties.npz")
    np.testing.assert_array_equal(oracle.furthest_point_sampling(fx["dup_xyz"], 1500), fx["dup_idx"])
    np.testing.assert_array_equal(oracle.furthest_point_sampling(fx["odd_xyz"], 300), fx["odd_idx"])
    # 1200 unique rows, 1500 picks: the tail of the sequence is decided purely by zero-distance ties
    assert len(np.unique(fx["dup_xyz"][0], axis=0)) == 1200


def test_iou3d_fixture(oracle):
    fx = golden("iou3d.npz")
    bev_a = fx["bev_a"]
    order = np.argsort(-fx["scores"], kind="stable")
    for name, thr, rot in (("keep_rot_010", 0.1, True), ("keep_rot_050", 0.5, True), ("keep_normal_085", 0.85, False),
                           ("keep_normal_050", 0.5, False)):
        np.testing.assert_array_equal(order[oracle.nms(bev_a[order], thr, rot)], fx[name])
    assert fx["iou3d"].shape == (300, 24) and fx["iou3d"].max() <= 1.0 + 1e-5 and (fx["iou3d"] > 0.3).sum() > 10

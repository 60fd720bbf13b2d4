"""Point-in-box membership ON the box faces, without a GPU: the float32 restatement (tests/box_faces.py: membership32) against the
CPU oracle, the reference's own compiled host op (where the build made it) and the library's host ops, on the whole point set of
every case tests/test_box_faces_gpu.py runs -- and the input conditions of those cases, asserted from the restatement alone:

  * at least 100 points per case stand exactly ON a face (inside only because the bounds are inclusive),
  * at least 30 change sides when a product of x_rot or z_rot is fused into the sum,
  * between 30 % and 70 % of the face points are inside,
  * every regular box decides both ways within one ulp step on each of its six faces.

All comparisons are exact and cover every point."""
import os

import numpy as np
import pytest
import torch

import box_faces as bf
import rpn_targets_restate as rs
import scan_restate as sr

F = np.float32
RPN_CASES = [(g, n, aug) for g in bf.RPN_G for n in bf.RPN_N for aug in (False, True)]


def rpn_values(case, s):
    """the values the labels are defined on: the restatement's augmented points and boxes of scene s"""
    if case["aug"] is None:
        return case["pts"][s], case["gt"][s]
    with np.errstate(invalid="ignore", over="ignore"):
        return rs.augment(case["pts"][s], case["gt"][s], case["alpha"][s], case["aug"][s])


def clouds():
    """(name, pts (N,3), boxes (M,7), extra) of every GPU case; extra > 0: the canonical enlargement"""
    for e in (0.0, 0.2, 1.0):
        case = bf.pool_case(e)
        for s in range(bf.POOL_B):
            yield "pool e=%g scene %d" % (e, s), case["xyz"][s], case["boxes"][s], e
    for g, n, aug in RPN_CASES:
        case = bf.rpn_case(g, n, aug)
        for s in range(bf.RPN_B):
            yield ("rpn g=%d n=%d aug=%d scene %d" % (g, n, aug, s),) + rpn_values(case, s) + (0.0,)
    for s, scene in enumerate(bf.scan_case()):
        rect = sr.classify(scene["pts"], scene["num_raw"], scene["V2C"], scene["R0"], scene["P2"], scene["img_shape"])[0]
        yield "scan scene %d" % s, rect, scene["remove_boxes"], 0.0
    cross = bf.cross_case()
    yield "cross", cross["pts"], cross["boxes"], 0.0


def restated(pts, boxes, extra):
    return np.stack([bf.membership32(pts, b, extra, gate=True, canonical=extra > 0)[0] for b in boxes]).astype(np.int64)


def enlarged(boxes, extra):
    from epnet_amd import kitti_utils
    return kitti_utils.enlarge_box3d(np.ascontiguousarray(boxes, F), extra) if extra else np.ascontiguousarray(boxes, F)


def test_restatement_equals_the_oracle_the_reference_and_the_host_op(oracle, hiplib):
    from epnet_amd import roipool3d_cuda
    from oracle import build_ref
    ref = build_ref.load() if (os.path.exists(build_ref.OUT) or build_ref.available()) else None
    members = boxes_seen = boxes_compared = 0
    for name, pts, boxes, extra in clouds():
        want = restated(pts, boxes, extra)
        big = enlarged(boxes, extra)
        assert np.array_equal(oracle.pts_in_boxes3d(pts, big), want), name
        flags = torch.full(want.shape, 7, dtype=torch.int64)
        roipool3d_cuda.pts_in_boxes3d_cpu(flags, torch.from_numpy(np.ascontiguousarray(pts)), torch.from_numpy(big))
        assert np.array_equal(flags.numpy(), want), name
        if ref is not None:
            live = torch.full(want.shape, 7, dtype=torch.int64)
            ref.pts_in_boxes3d_cpu(live, torch.from_numpy(np.ascontiguousarray(pts)), torch.from_numpy(big))
            same_trig = libm_trig_is_correctly_rounded(big[:, 6])
            assert np.array_equal(live.numpy()[same_trig], want[same_trig]), name
            boxes_seen += len(big)
            boxes_compared += int(same_trig.sum())
        members += int(want.sum())
    assert members > 10000 and (ref is None or boxes_compared > 0.9 * boxes_seen)


def libm_trig_is_correctly_rounded(angles):
    """The reference's host op calls the C library's float cos and sin, which are good to an ulp but not correctly rounded: for
    about one angle in forty one of the two differs in its last bit from (float)cos((double)x), the parity definition's value
    ("Trigonometry": those bits are not part of the reference's contract). On a face that bit decides, so the compiled
    reference is compared on the boxes whose two values it rounds correctly -> (M) bool"""
    import ctypes
    import ctypes.util
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    for f in (libm.cosf, libm.sinf):
        f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float]
    ok = []
    for a in np.asarray(angles, F):
        ok.append(F(libm.cosf(a)) == F(np.cos(np.float64(a))) and F(libm.sinf(a)) == F(np.sin(np.float64(a))))
    return np.array(ok, bool)


@pytest.mark.parametrize("extra", (0.0, 0.2, 1.0))
def test_host_pooling_picks_the_first_members_in_index_order(hiplib, extra):
    """epnet_roipool3d_host over host.cpp's hoisted pt_in_box: S = 16 truncates among face points, S = 512 pads cyclically"""
    from epnet_amd import roipool3d_cuda
    case = bf.pool_case(extra)
    for s in range(bf.POOL_B):
        pts, boxes = case["xyz"][s], enlarged(case["boxes"][s], extra)
        inside = restated(pts, case["boxes"][s], extra).astype(bool)
        for S in (16, 512):
            out_p, out_f, flag = torch.zeros((len(boxes), S, 3)), torch.zeros((len(boxes), S, 1)), torch.full((len(boxes),), 7, dtype=torch.int64)
            roipool3d_cuda.roipool3d_cpu(torch.from_numpy(pts), torch.from_numpy(boxes), torch.from_numpy(case["feat"][s]), out_p, out_f, flag)
            for k in range(len(boxes)):
                idx = np.nonzero(inside[k])[0][:S]
                assert int(flag[k]) == int(len(idx) == 0), (s, S, k)
                if len(idx):
                    chosen = idx[np.arange(S) % len(idx)]
                    assert np.array_equal(out_f[k, :, 0].numpy(), chosen.astype(F)), (s, S, k)
                    assert out_p[k].numpy().tobytes() == pts[chosen].tobytes(), (s, S, k)
        counts = inside.sum(axis=1)
        assert counts[-1] == 2 and ((counts > 16) & (counts < 512)).sum() >= 8                # the two-member box; both S regimes
        on = bf.classify(pts, case["boxes"][s, -1], extra, True, extra > 0)["on_face"]
        assert np.array_equal(on, inside[-1])                                                # ... and both of its members stand on a face


# ---- the input conditions of the GPU cases ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", (0.0, 0.2, 1.0))
def test_conditions_of_the_pooling_cases(extra):
    c = bf.case_conditions(bf.scenes_of(bf.pool_case(extra)), gate=True)
    print(c)
    bf.check_conditions(c)


@pytest.mark.parametrize("g,n,aug", RPN_CASES)
def test_conditions_of_the_rpn_cases(g, n, aug):
    case = bf.rpn_case(g, n, aug)
    c = bf.case_conditions(bf.scenes_of(case), gate=False)
    print(c)
    bf.check_conditions(c)
    if aug:     # the marks belong to the cloud: taken again on the restatement's augmented values of the rows, for the first faced box
        for s in range(bf.RPN_B):
            pts, gt = rpn_values(case, s)
            first = case["meta"][s]["box"] == 0
            again = bf.classify(pts[case["rows"][s]][first], gt[0], 0.0, gate=False, cy=gt[0, 1] - gt[0, 3] / F(2))
            assert all(np.array_equal(again[key], case["marks"][s][key][first]) for key in again)


def test_conditions_of_the_scan_and_the_cross_case():
    scenes = bf.scan_case()
    c = bf.case_conditions(scenes, gate=True)
    print(c)
    bf.check_conditions(c)
    for scene in scenes:    # the marks belong to the rectified values of the rows in the scene
        rect, _, valid, _ = sr.classify(scene["pts"], scene["num_raw"], scene["V2C"], scene["R0"], scene["P2"], scene["img_shape"])
        meta = scene["meta"]
        first = meta["box"] == 0
        again = bf.classify(rect[scene["rows"]][first], scene["remove_boxes"][0])
        assert all(np.array_equal(again[key], scene["marks"][key][first]) for key in again)
        assert valid[scene["rows"]][meta["face"] >= 0].all()
    cross = bf.cross_case()
    c = bf.case_conditions([cross], gate=True)
    print(c)
    bf.check_conditions(c)
    for box in cross["boxes"]:     # within the gate of every box it belongs to: the families may be compared
        _, v = bf.membership32(cross["pts"][cross["rows"]], box)
        near = np.hypot(v["dx"], v["dz"]) < 6
        assert (np.abs(v["dx"][near]) < 10).all() and np.isfinite(cross["pts"]).all()


def test_the_gate_points_decide_on_the_gate():
    """|x - cx| or |z - cz| of exactly 10 lies inside the gate, the coordinate's next float beyond it outside although inside the box"""
    boxes, kinds = bf.box_set(np.random.default_rng(1), 0)
    seen = 0
    for box, kind in zip(boxes, kinds):
        if kind != "gate":
            continue
        pts, meta = bf.face_points(box, 1, 0, np.random.default_rng(2))
        tail = pts[-8:]
        gated, v = bf.membership32(tail, box)
        free = bf.membership32(tail, box, gate=False)[0]
        d = np.maximum(np.abs(v["dx"]), np.abs(v["dz"]))
        assert np.array_equal(d[0::2], np.full(4, F(10))) and (d[1::2] > F(10)).all() and (d[1::2] < F(10.00001)).all()
        assert np.array_equal(gated, free & (d == F(10))) and gated.sum() == 2 and free.sum() == 4
        seen += 1
    assert seen == 2


def test_degenerate_and_special_boxes():
    boxes, kinds = bf.box_set(np.random.default_rng(3), 2)
    assert kinds.count("random") == 2 and kinds.count("aligned") == 4 and kinds.count("degenerate") == 2 and "far" in kinds and "dyadic" in kinds
    flat, neg = (b for b, k in zip(boxes, kinds) if k == "degenerate")
    assert flat[4] == 0 and neg[5] < 0
    pts, meta = bf.face_points(neg, 16, 3, np.random.default_rng(4))
    assert not bf.membership32(pts, neg)[0].any() and not bf.membership32(pts, neg, gate=False)[0].any()
    pts, meta = bf.face_points(flat, 64, 3, np.random.default_rng(4))
    inside, v = bf.membership32(pts, flat)
    assert inside.any() and (v["z_rot"][inside] == 0).all()                                  # a box without width holds its mid-plane
    cls, reg = rs.labels32(pts, np.stack([flat, neg]))
    assert not cls.any() and not reg.any()                                                   # ... but labels nothing
    dyadic = boxes[kinds.index("dyadic")]
    pts, meta = bf.face_points(dyadic, 8, 0, np.random.default_rng(5))
    assert bf.classify(pts, dyadic)["on_face"][meta["face"] >= 0].all()                      # its faces are float32 values


# ---- the float64 yardstick stays honest ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g,n,aug", RPN_CASES)
def test_float64_labels_agree_away_from_the_faces(g, n, aug):
    case = bf.rpn_case(g, n, aug)
    near = 0
    for s in range(bf.RPN_B):
        pts, gt = rpn_values(case, s)
        cls64, reg64, dist = rs.labels(pts, gt, bf.RPN_EXTRA)
        cls32, reg32 = rs.labels32(pts, gt, bf.RPN_EXTRA)
        with np.errstate(invalid="ignore"):
            keep = dist > rs.BAND
        assert np.array_equal(cls64[keep], cls32[keep]) and reg64[keep].tobytes() == reg32[keep].tobytes(), (g, n, aug, s)
        near += int((~keep).sum())
        assert (cls32 == 1).any() and (cls32 == -1).any() and (cls32 == 0).any()
    assert near > n                                                                          # most of the cloud is within the band

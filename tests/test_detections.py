"""Second-stage inference without a GPU: epnet_roipool3d_canonical / epnet_rcnn_detections (declared, exported, typed, their
arguments validated before any launch), the numpy restatements of tests/detections_restate.py against what the REFERENCE'S OWN
code produced (tests/golden/rcnn_eval_input.npz, detections.npz, written by tests/golden/make_golden_detections.py), and
epnet_amd.detection_layer on CPU tensors over the restatement-backed stand-ins. The GPU half is tests/test_detections_gpu.py.

Bounds. Detections: scores and counts exactly (copies of inputs, index-valued), boxes to 1e-5 (the decoding's tolerance, as
tests/test_proposal_layer.py). Canonical pooling: feature columns and flags exactly; dy exactly; the rotated columns within
1e-6 * (|dx| + |dz|) + 1e-6 -- each side rounds the trigonometry (<= 1 ulp), two products and one sum: <= 2 ulp of
|dx| + |dz| per side, 4 * 2^-23 = 4.8e-7 for both.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden

import detections_restate as R

NEW_SYMBOLS = ("epnet_roipool3d_canonical", "epnet_rcnn_detections", "epnet_rcnn_detections_workspace_bytes")
EINVAL, ELAUNCH, ENOMEM, ELIMIT = -1, -2, -3, -4


def T(a, device="cpu"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ---- header / export / binding table -----------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_typed(hiplib):
    from epnet_amd import _lib
    text = open(os.path.join(ROOT, "include", "epnet_ops.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    vp, i, f, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    assert _lib.SIGNATURES["epnet_roipool3d_canonical"] == (i, [i, i, i, i, i, f, vp, vp, vp, vp, vp, vp])
    assert _lib.SIGNATURES["epnet_rcnn_detections_workspace_bytes"] == (sz, [i, i])
    assert _lib.SIGNATURES["epnet_rcnn_detections"] == (i, [i, i, vp, vp, vp, f, f, vp, sz, vp, vp, vp, vp])
    assert "#define EPNET_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "epnet_ops.h")).read()


# ---- argument validation: everything is refused before a launch --------------------------------------------------------------
P, WS = 256, 1 << 40      # placeholder pointer (never dereferenced), workspace size that is never short


def det_call(l, b, m, ptrs=(P,) * 7, ws_bytes=WS):
    boxes, raw, norm, ws, ob, os_, oc = ptrs
    return l.epnet_rcnn_detections(b, m, boxes, raw, norm, 0.2, 0.1, ws, ws_bytes, ob, os_, oc, None)


def test_detections_arguments_are_checked_before_a_launch(hiplib):
    l = hiplib
    if not torch.cuda.is_available():                           # (with a GPU the placeholder pointers must not reach a launch)
        assert det_call(l, 1, 100) == ELAUNCH                   # a shape inside the limits reaches its first launch
        assert det_call(l, 65535, 4096) == ELAUNCH              # ... also right at the limits
    assert det_call(l, 1, 4097) == ELIMIT and det_call(l, 65536, 100) == ELIMIT and det_call(l, 1, 0) == ELIMIT
    assert det_call(l, -1, 100) == EINVAL and det_call(l, 1, -1) == EINVAL
    for k in range(7):                                          # each pointer on its own
        ptrs = tuple(None if j == k else P for j in range(7))
        assert det_call(l, 2, 100, ptrs) == EINVAL, k
    need = l.epnet_rcnn_detections_workspace_bytes(2, 100)
    assert need > 0 and det_call(l, 2, 100, ws_bytes=need - 1) == ENOMEM and det_call(l, 2, 100, ws_bytes=0) == ENOMEM
    if not torch.cuda.is_available():
        assert det_call(l, 2, 100, ws_bytes=need) == ELAUNCH
    assert det_call(l, 0, 100) == 0 and det_call(l, 0, 100, (None,) * 7, 0) == 0      # no scene: nothing to do


def test_detections_workspace_depends_on_the_shape_alone(hiplib):
    from epnet_amd import _lib
    l = hiplib
    size = l.epnet_rcnn_detections_workspace_bytes
    ms = (1, 2, 63, 64, 65, 100, 128, 129, 512, 1000, 4096)
    for b in (1, 2, 3, 16, 257, 65535):
        sizes = [size(b, m) for m in ms]
        assert all(x > 0 for x in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes), (b, sizes)
    for m in ms:
        sizes = [size(b, m) for b in (1, 2, 3, 16, 257, 65535)]
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes), (m, sizes)
    assert size(0, 100) == 0 and size(1, 0) == 0 and size(1, 4097) == 0 and size(65536, 1) == 0 and size(-1, 5) == 0
    # the layout: counts, kept counts, selection, BEV boxes, one 80-byte record and one keep slot per box, the mask words
    al = lambda x: (x + 15) & ~15   # noqa: E731
    assert size(3, 100) == al(12) * 2 + al(3 * 100 * 4) + al(3 * 100 * 20) + al(3 * 100 * 80) + al(3 * 100 * 8) + al(3 * 100 * 2 * 8)
    before = {(b, m): size(b, m) for b in (1, 16) for m in (100, 4096)}
    knobs = {"EPNET_BQ_PAIR": (0, 1), "EPNET_BQ_STREAM": (0, 1), "EPNET_BQ_ORDERED": (0, 1), "EPNET_FPS_PRUNE": (0, 1),
             "EPNET_FPS_PWAVES": (4, 8), "EPNET_FPS_WAVES": (4, 16), "EPNET_FPS_PRUNE_MIN": (0, 4096), "EPNET_NN_TILE_MIN_BUCKETS": (0, 1000)}
    v = ctypes.c_int()
    for name, values in knobs.items():
        assert l.epnet_get_tuning(name.encode(), ctypes.byref(v)) == 0, name
        for value in values:
            with _lib.tuning(**{name: value}):
                assert {k: size(*k) for k in before} == before, (name, value)


def test_canonical_pooling_arguments_are_checked_before_a_launch(hiplib):
    l = hiplib
    call = lambda b, n, m, c, s, ptrs=(P,) * 5: l.epnet_roipool3d_canonical(b, n, m, c, s, 0.2, *ptrs, None)   # noqa: E731
    s_max = 150 * 1024 // 20                                    # the LDS bound on S: 5 lists of S ints in 150 KB
    if not torch.cuda.is_available():                           # (with a GPU the placeholder pointers must not reach a launch)
        assert call(1, 1000, 100, 5, 512) == ELAUNCH and call(65535, 1000, 1, 5, 512) == ELAUNCH
        assert call(1, 1000, 100, 5, s_max) == ELAUNCH
    assert call(65536, 1000, 100, 5, 512) == ELIMIT and call(1, 1000, 100, 5, s_max + 1) == ELIMIT
    for bad in ((-1, 10, 10, 1, 8), (1, -1, 10, 1, 8), (1, 10, -1, 1, 8), (1, 10, 10, -1, 8), (1, 10, 10, 1, -8)):
        assert call(*bad) == EINVAL, bad
    for k in (0, 1, 2, 3, 4):
        assert call(1, 1000, 100, 5, 32, tuple(None if j == k else P for j in range(5))) == EINVAL, k
    assert call(0, 1000, 100, 5, 32, (None,) * 5) == 0 and call(2, 1000, 0, 5, 32, (None,) * 5) == 0


# ---- the restatement against the reference's own results -------------------------------------------------------------------------
def check_pooled(got, flag, fx):
    """got (B*M, S, 3+C) against the fixture with the module docstring's bounds"""
    want, rois = fx["pts_input"], fx["in_roi_boxes3d"].reshape(-1, 7)
    assert got.shape == want.shape
    np.testing.assert_array_equal(flag, fx["pooled_empty_flag"])
    np.testing.assert_array_equal(got[:, :, 3:], want[:, :, 3:])
    np.testing.assert_array_equal(got[:, :, 1], want[:, :, 1])
    # |dx| + |dz| is at least the length of (dx, dz), which the rotation keeps: the bound used here is no wider than the stated one
    size = np.hypot(want[:, :, 0].astype(np.float64), want[:, :, 2].astype(np.float64))
    bound = 1e-6 * size + 1e-6
    for col in (0, 2):
        err = np.abs(got[:, :, col].astype(np.float64) - want[:, :, col].astype(np.float64))
        print("canonical xyz column %d: largest error / bound = %.3f" % (col, float((err / bound).max())))
        assert (err <= bound).all(), (col, float((err / bound).max()))
    empty = fx["pooled_empty_flag"].reshape(-1) == 1
    assert empty.any() and (got[empty][:, :, 3:] == 0).all() and (np.abs(got[empty][:, :, 0:3]).max(axis=(1, 2)) > 1).all()


def check_detections(got, fx, boxes_exact):
    pred, raw, norm, det_b, det_s, det_c = (np.asarray(a) for a in got)
    np.testing.assert_array_equal(det_c, fx["det_count"])
    np.testing.assert_array_equal(det_s, fx["det_scores"])
    np.testing.assert_array_equal(raw, fx["raw_scores"])
    if boxes_exact:
        np.testing.assert_array_equal(det_b, fx["det_boxes3d"])
    else:
        np.testing.assert_allclose(pred, fx["pred_boxes3d"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(norm, fx["norm_scores"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(det_b, fx["det_boxes3d"], rtol=1e-5, atol=1e-5)
    for k in range(det_c.shape[0]):      # zero rows behind the detections
        assert not det_b[k, det_c[k]:].any() and not det_s[k, det_c[k]:].any()


def test_fixtures_cover_what_they_are_for():
    fx, dx = golden("rcnn_eval_input.npz"), golden("detections.npz")
    flag = fx["pooled_empty_flag"]
    assert flag.sum() > 0 and (flag == 0).sum() > 0
    cand = (dx["norm_scores"] > dx["cfg"][0]).sum(1)
    m = dx["raw_scores"].shape[1]
    assert (cand == 0).any() and (cand == m).any() and ((cand > 0) & (cand < m)).any()
    assert (dx["det_count"][cand > 0] < cand[cand > 0]).all()      # the NMS suppresses something in every scene it runs on
    size = sum(os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in ("rcnn_eval_input.npz", "detections.npz"))
    assert size < 1000000


def test_restated_pooling_equals_the_reference(oracle):
    fx = golden("rcnn_eval_input.npz")
    extra, s = float(fx["cfg"][0]), int(fx["cfg"][1])
    depth = (fx["in_pts_depth"] / np.float32(70.0) - np.float32(0.5)).astype(np.float32)
    feat = np.concatenate([fx["in_seg_mask"][..., None], depth[..., None], fx["in_rpn_features"]], axis=2)
    pooled, flag = R.roipool3d_canonical(fx["in_rpn_xyz"], fx["in_roi_boxes3d"], feat, extra, s)
    check_pooled(pooled.reshape(-1, s, pooled.shape[-1]), flag, fx)


def test_restated_detections_equal_the_reference(oracle):
    fx = golden("detections.npz")
    det = R.rcnn_detections(fx["pred_boxes3d"], fx["raw_scores"], fx["norm_scores"], fx["cfg"][0], fx["cfg"][1])
    check_detections((fx["pred_boxes3d"], fx["raw_scores"], fx["norm_scores"]) + det, fx, boxes_exact=True)


# ---- the layers on CPU tensors over the stand-ins ------------------------------------------------------------------------------
@pytest.fixture()
def cpu_surface(monkeypatch, oracle):
    R.install(monkeypatch)
    return "cpu"


def run_pool_rois(device):
    from epnet_amd import detection_layer as dl
    fx = golden("rcnn_eval_input.npz")
    cfg = dl.default_cfg()
    cfg.RCNN.POOL_EXTRA_WIDTH, cfg.RCNN.NUM_POINTS = float(fx["cfg"][0]), int(fx["cfg"][1])
    pts_input, flag = dl.pool_rois(T(fx["in_rpn_xyz"], device), T(fx["in_rpn_features"], device), T(fx["in_roi_boxes3d"], device),
                                   T(fx["in_seg_mask"], device), pts_depth=T(fx["in_pts_depth"], device), cfg=cfg)
    assert flag.dtype == torch.int32
    check_pooled(pts_input.cpu().numpy(), flag.cpu().numpy(), fx)


def run_detection_layer(device):
    from epnet_amd import detection_layer as dl
    fx = golden("detections.npz")
    cfg = dl.default_cfg()
    assert (cfg.RCNN.SCORE_THRESH, cfg.RCNN.NMS_THRESH) == tuple(fx["cfg"])
    layer = dl.DetectionLayer(cfg).to(device)
    got = layer(T(fx["rois"], device), T(fx["rcnn_cls"], device), T(fx["rcnn_reg_f16"], device).float())
    assert got[5].dtype == torch.int32
    check_detections([g.cpu().numpy() for g in got], fx, boxes_exact=False)


def test_pool_rois_matches_the_reference_cpu(cpu_surface):
    run_pool_rois("cpu")


def test_detection_layer_matches_the_reference_cpu(cpu_surface):
    run_detection_layer("cpu")


def test_default_cfg_holds_the_yaml_values():
    from epnet_amd import detection_layer as dl
    r = dl.default_cfg().RCNN
    assert (r.LOC_SCOPE, r.LOC_BIN_SIZE, r.NUM_HEAD_BIN, r.LOC_Y_BY_BIN, r.LOC_Y_SCOPE, r.LOC_Y_BIN_SIZE) == (1.5, 0.5, 9, False, 0.5, 0.25)
    assert (r.SIZE_RES_ON_ROI, r.SCORE_THRESH, r.NMS_THRESH, r.POOL_EXTRA_WIDTH, r.NUM_POINTS) == (False, 0.2, 0.1, 0.2, 512)
    assert (r.USE_MASK, r.USE_DEPTH, r.USE_INTENSITY, dl.default_cfg().USE_IOU_BRANCH) == (True, True, False, False)
    np.testing.assert_allclose(dl.default_cfg().CLS_MEAN_SIZE, [[1.52563191462, 1.62856739989, 3.88311640418]], rtol=1e-7)


def test_refused_configurations_raise(cpu_surface):
    from epnet_amd import detection_layer as dl
    fx = golden("detections.npz")
    rois, reg = T(fx["rois"]), T(fx["rcnn_reg_f16"]).float()
    with pytest.raises(NotImplementedError):
        dl.DetectionLayer(dl.default_cfg())(rois, torch.zeros((rois.shape[0] * rois.shape[1], 2)), reg)
    cfg = dl.default_cfg()
    cfg.RCNN.SIZE_RES_ON_ROI = True
    with pytest.raises(NotImplementedError):
        dl.DetectionLayer(cfg)(rois, T(fx["rcnn_cls"]), reg)


def test_iou_branch_scales_the_class_score(cpu_surface):
    """tools/eval_rcnn.py:558-561: max(iou, 1e-4) * cls is what is thresholded and sorted"""
    from epnet_amd import detection_layer as dl
    fx = golden("detections.npz")
    rois, cls, reg = T(fx["rois"]), T(fx["rcnn_cls"]), T(fx["rcnn_reg_f16"]).float()
    iou = torch.rand(cls.shape, generator=torch.Generator().manual_seed(5)) - 0.2
    got = dl.DetectionLayer(dl.default_cfg())(rois, cls, reg, rcnn_iou_branch=iou)
    want_raw = (torch.max(iou, torch.full_like(iou, 1e-4)) * cls).view(rois.shape[0], -1)
    assert torch.equal(got[1], want_raw) and torch.equal(got[2], torch.sigmoid(want_raw))
    det = R.rcnn_detections(got[0].numpy(), want_raw.numpy(), got[2].numpy(), 0.2, 0.1)
    np.testing.assert_array_equal(got[4].numpy(), det[1])
    np.testing.assert_array_equal(got[5].numpy(), det[2])


def test_intensity_column_comes_first(cpu_surface):
    """lib/net/rcnn_net.py:140-148: [intensity, mask, depth] then the RPN features"""
    from epnet_amd import detection_layer as dl
    fx = golden("rcnn_eval_input.npz")
    cfg = dl.default_cfg()
    cfg.RCNN.USE_INTENSITY, cfg.RCNN.USE_DEPTH, cfg.RCNN.NUM_POINTS = True, False, 8
    xyz, mask = T(fx["in_rpn_xyz"]), T(fx["in_seg_mask"])
    inten = torch.rand(mask.shape, generator=torch.Generator().manual_seed(6)) + 2.0     # values no other column holds
    pts, flag = dl.pool_rois(xyz, T(fx["in_rpn_features"]), T(fx["in_roi_boxes3d"]), mask, rpn_intensity=inten, cfg=cfg)
    full = pts[flag.view(-1) == 0]
    assert pts.shape[2] == 3 + 2 + fx["in_rpn_features"].shape[2] and full.shape[0] > 0
    assert (full[:, :, 3] >= 2.0).all() and ((full[:, :, 4] == 0) | (full[:, :, 4] == 1)).all()


# ---- known answers written by hand -------------------------------------------------------------------------------------------
def box(x, z, ry=0.0):
    return [x, 1.6, z, 1.5, 2.0, 4.0, ry]      # BEV: 4 m along x, 2 m along z


def test_chain_of_three_the_middle_one_goes(oracle):
    """boxes 0 - 1 and 1 - 2 overlap (shift 2 m of 4: IoU 1/3), 0 - 2 only touch: the best keeps, the middle one goes, the third
    -- suppressed by nobody that was kept -- stays"""
    boxes = np.array([[box(0, 10), box(2, 10), box(4, 10)]], np.float32)
    raw = np.array([[3.0, 2.0, 1.0]], np.float32)
    det_b, det_s, det_c = R.rcnn_detections(boxes, raw, np.full((1, 3), 0.9, np.float32), 0.2, 0.1)
    assert det_c.tolist() == [2] and det_s[0].tolist() == [3.0, 1.0, 0.0]
    np.testing.assert_array_equal(det_b[0], np.array([box(0, 10), box(4, 10), [0] * 7], np.float32))


def test_equal_scores_resolve_by_index_and_the_rule_is_observable(oracle):
    """the same chain with one score for all: index order decides -- box 0 first, so boxes 0 and 2 stay; with the rows
    reversed the chain is walked from the other end and the kept SET differs in the outer pair's order, while a pair
    (0 - 1 overlapping, 2 apart) shows it outright: whichever of the two comes first in the index survives"""
    raw = np.full((1, 3), 0.5, np.float32)
    norm = np.full((1, 3), 0.9, np.float32)
    rows = [box(0, 10), box(2, 10, 0.02), box(30, 10)]
    det_b, det_s, det_c = R.rcnn_detections(np.array([rows], np.float32), raw, norm, 0.2, 0.1)
    assert det_c.tolist() == [2]
    np.testing.assert_array_equal(det_b[0, :2], np.array([rows[0], rows[2]], np.float32))
    rev = rows[::-1]
    det_b, det_s, det_c = R.rcnn_detections(np.array([rev], np.float32), raw, norm, 0.2, 0.1)
    assert det_c.tolist() == [2]
    np.testing.assert_array_equal(det_b[0, :2], np.array([rows[2], rows[1]], np.float32))     # the OTHER box of the pair
    # -0.0 and +0.0 are one score
    det_b, det_s, det_c = R.rcnn_detections(np.array([rows], np.float32), np.array([[-0.0, 0.0, -0.0]], np.float32), norm, 0.2, 0.1)
    np.testing.assert_array_equal(det_b[0, :2], np.array([rows[0], rows[2]], np.float32))


def test_nan_inf_and_threshold_equality(oracle):
    far = np.array([[box(0, 10), box(10, 10), box(20, 10), box(30, 10), box(40, 10)]], np.float32)
    thresh = np.float32(0.2)
    raw = np.array([[1.0, -np.inf, np.inf, np.nan, 0.5]], np.float32)
    # norm == thresh is not a candidate; a NaN norm is never one; the NaN raw score of a candidate ranks first
    norm = np.array([[0.9, 0.9, 0.9, 0.9, thresh]], np.float32)
    det_b, det_s, det_c = R.rcnn_detections(far, raw, norm, 0.2, 0.1)
    assert det_c.tolist() == [4] and np.isnan(det_s[0, 0]) and det_s[0, 1:4].tolist() == [np.inf, 1.0, -np.inf]
    np.testing.assert_array_equal(det_b[0, :4], far[0, [3, 2, 0, 1]])
    norm = np.array([[np.nan, 0.9, np.nan, np.nextafter(thresh, np.float32(1)), thresh]], np.float32)
    det_b, det_s, det_c = R.rcnn_detections(far, raw, norm, 0.2, 0.1)
    assert det_c.tolist() == [2] and np.isnan(det_s[0, 0]) and det_s[0, 1] == -np.inf
    det_b, det_s, det_c = R.rcnn_detections(far, raw, np.full((1, 5), np.nan, np.float32), 0.2, 0.1)
    assert det_c.tolist() == [0] and not det_b.any() and not det_s.any()


def test_an_empty_box_holds_the_rotated_minus_centre(oracle):
    xyz = np.array([[[1.0, 1.0, 10.0], [1.2, 1.1, 10.3]]], np.float32)
    rois = np.array([[[1.0, 1.6, 10.0, 1.5, 2.0, 4.0, 0.0], [50.0, 2.0, -7.0, 1.5, 2.0, 4.0, np.pi / 2], [3.0, -4.0, 0.0, 1.0, 1.0, 1.0, np.pi]]], np.float32)
    feat = np.array([[[7.0], [8.0]]], np.float32)
    pooled, flag = R.roipool3d_canonical(xyz, rois, feat, 0.2, 4)
    assert flag.tolist() == [[0, 1, 1]]
    # ROI 0 (ry = 0): plain differences, the two points cyclically
    np.testing.assert_allclose(pooled[0, 0, :, 0:3], [[0, -0.6, 0], [0.2, -0.5, 0.3]] * 2, atol=1e-6)
    assert pooled[0, 0, :, 3].tolist() == [7, 8, 7, 8]
    # ROI 1 (ry = pi/2): (dx, dz) = (-50, 7) -> (dx c - dz s, dx s + dz c) = (-7, -50); dy = -2; the same in all S rows, features 0
    np.testing.assert_allclose(pooled[0, 1, :, 0:3], [[-7.0, -2.0, -50.0]] * 4, atol=1e-5)
    # ROI 2 (ry = pi): (-3, 0) -> (3, 0); dy = +4
    np.testing.assert_allclose(pooled[0, 2, :, 0:3], [[3.0, 4.0, 0.0]] * 4, atol=1e-6)
    assert not pooled[0, 1:, :, 3].any()


# ---- the sweep of the GPU half covers what it says -------------------------------------------------------------------------------
def test_gpu_sweep_cases_cover_every_listed_value():
    cases = R.detection_cases()
    assert 140 <= len(cases) <= 160 and len(set(cases)) == len(cases)
    assert {c[0] for c in cases} == set(R.DET_B) == {1, 2, 3, 16, 257}
    assert {c[1] for c in cases} == set(R.DET_M) == {1, 2, 63, 64, 65, 100, 127, 128, 129, 512, 1000, 4096}
    assert {c[2] for c in cases} == set(R.DET_SCORES) and {c[3] for c in cases} == set(R.DET_BOXES)
    assert {(c[2], c[3]) for c in cases} == {(s, b) for s in R.DET_SCORES for b in R.DET_BOXES}
    assert any(c[1] > 128 and c[3] == "clustered" and c[2] in ("distinct", "ties", "all_above") for c in cases)    # chains across tiles
    assert cases == R.detection_cases()      # seeded: the same list in every process
    pool = R.pooling_cases()
    assert {c[1] for c in pool} == set(R.POOL_N) == {1, 63, 64, 65, 1000, 16384}
    assert {c[2] for c in pool} == set(R.POOL_M) == {1, 100, 128}
    assert {c[3] for c in pool} == set(R.POOL_S) == {1, 16, 512, 513}
    assert {c[4] for c in pool} == set(R.POOL_C) == {0, 1, 3, 130}
    assert min(c[0] for c in pool) == 1 and max(c[0] for c in pool) == 17


def test_sweep_inputs_are_what_their_families_say():
    for sf in R.DET_SCORES:
        boxes, raw, norm = R.detection_inputs(3, 130, sf, "clustered", 11)
        assert boxes.shape == (3, 130, 7) and raw.shape == (3, 130)
        n = torch.sigmoid(raw) if norm is None else norm
        above = (n > 0.2).sum().item()
        if sf == "none_above":
            assert above == 0
        elif sf in ("all_above", "all_equal"):
            assert above == raw.numel()
        elif sf == "nonfinite":
            assert torch.isnan(raw).any() and torch.isinf(raw).any() and torch.isnan(norm).any() and (torch.isnan(raw) & (norm > 0.2)).any()
        elif sf == "ties":
            assert raw.unique().numel() < raw.numel() // 4
        if sf == "zeros":
            assert ((raw == 0) & torch.signbit(raw)).any() and ((raw == 0) & ~torch.signbit(raw)).any()
    xyz, rois, feat = R.pooling_inputs(2, 1000, 100, 3, 5)
    assert xyz.shape == (2, 1000, 3) and rois.shape == (2, 100, 7) and feat.shape == (2, 1000, 3) and (rois[:, 3::7, 0] > 400).all()

"""The evaluation epoch without a GPU: epnet_eval_recall / epnet_kitti_records (declared, exported, typed, their arguments validated
before any launch), the numpy restatements of tests/eval_epoch_restate.py against what the REFERENCE'S OWN code produced
(tests/golden/eval_epoch.npz, written by tests/golden/make_golden_eval_epoch.py), r4 against printf on the host, and
epnet_amd.eval_epoch on CPU tensors over the restatement-backed stand-ins. The GPU half is tests/test_eval_epoch_gpu.py.

Bounds against the fixture. Counters, num_gt, valid flags and rec_count: exactly. Image boxes and alpha: the reference projects
the float32 corners in float64 (np.ones makes corners3d_hom float64) and builds the corners with a float32 np.matmul; the package
works in float32 throughout. MEASURED on the fixture: the largest distance of a clipped image coordinate is 1.5005e-4 px and of an
alpha 4.7684e-7 rad (one ulp at 4); the bars are four times that, rounded up: 7e-4 px and 2e-6 rad (DESIGN.md "Evaluation
epoch").
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, golden

import eval_epoch_restate as R

NEW_SYMBOLS = ("epnet_eval_recall", "epnet_eval_recall_workspace_bytes", "epnet_kitti_records")
EINVAL, ELAUNCH, ENOMEM, ELIMIT = -1, -2, -3, -4
BBOX_BAR_PX, ALPHA_BAR_RAD = 7e-4, 2e-6
IOU_CLEARANCE, FILTER_CLEARANCE = 3e-4, 1e-2


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
    vp, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    assert _lib.SIGNATURES["epnet_eval_recall_workspace_bytes"] == (sz, [i, i, i])
    assert _lib.SIGNATURES["epnet_eval_recall"] == (i, [i] * 6 + [vp] * 7 + [sz] + [vp] * 7)
    assert _lib.SIGNATURES["epnet_kitti_records"] == (i, [i, i] + [vp] * 10)
    from epnet_amd import eval_epoch, iou3d_cuda
    assert callable(iou3d_cuda.eval_recall_gpu) and callable(iou3d_cuda.kitti_records_gpu) and callable(eval_epoch.eval_batch)


# ---- argument validation: everything is refused before a launch --------------------------------------------------------------
P, WS = 256, 1 << 40      # placeholder pointer (never dereferenced), workspace size that is never short
THR = (ctypes.c_float * 8)(0.1, 0.3, 0.5, 0.7, 0.9, 0.2, 0.4, 0.6)
THR_P = ctypes.cast(THR, ctypes.c_void_p)


def recall_call(l, b=2, m=100, g=20, gc=7, n=512, nt=5, thr=THR_P, pred=P, roi=P, gt=P, seg=P, label=P, ws=P, ws_bytes=WS, stats=P,
                seg_counts=P, totals=None, gmp=None, gmr=None, pmi=None):
    return l.epnet_eval_recall(b, m, g, gc, n, nt, thr, pred, roi, gt, seg, label, ws, ws_bytes, stats, seg_counts, totals, gmp, gmr,
                               pmi, None)


def test_recall_arguments_are_checked_before_a_launch(hiplib):
    l = hiplib
    if not torch.cuda.is_available():                           # (with a GPU the placeholder pointers must not reach a launch)
        assert recall_call(l) == ELAUNCH                        # a shape inside the limits reaches its first launch
        assert recall_call(l, b=65535, m=4096, nt=8) == ELAUNCH and recall_call(l, m=1, g=0) == ELAUNCH     # ... also at the limits
        assert recall_call(l, roi=None) == ELAUNCH and recall_call(l, seg=None, label=None, seg_counts=None, n=0) == ELAUNCH
        assert recall_call(l, totals=P, gmp=P, gmr=P, pmi=P) == ELAUNCH
        assert recall_call(l, ws_bytes=l.epnet_eval_recall_workspace_bytes(2, 100, 20)) == ELAUNCH
    assert recall_call(l, m=4097) == ELIMIT and recall_call(l, m=0) == ELIMIT and recall_call(l, b=65536) == ELIMIT
    assert recall_call(l, nt=9) == ELIMIT and recall_call(l, g=-1) == ELIMIT
    assert recall_call(l, b=-1) == EINVAL and recall_call(l, m=-1) == EINVAL and recall_call(l, n=-1) == EINVAL and recall_call(l, nt=-1) == EINVAL
    assert recall_call(l, gc=6) == EINVAL and recall_call(l, gc=17) == EINVAL
    for name in ("thr", "pred", "gt", "ws", "stats"):           # each required pointer on its own
        assert recall_call(l, **{name: None}) == EINVAL, name
    # the segmentation inputs and their output come together or not at all
    assert recall_call(l, seg=None) == EINVAL and recall_call(l, label=None) == EINVAL and recall_call(l, seg_counts=None) == EINVAL
    assert recall_call(l, seg=None, label=None) == EINVAL and recall_call(l, label=None, seg_counts=None) == EINVAL
    need = l.epnet_eval_recall_workspace_bytes(2, 100, 20)
    assert need > 0 and recall_call(l, ws_bytes=need - 1) == ENOMEM and recall_call(l, ws_bytes=0) == ENOMEM
    assert recall_call(l, b=0) == 0 and recall_call(l, b=0, pred=None, gt=None, ws=None, stats=None, thr=None) == 0     # no scene: nothing to do


def test_recall_workspace_is_pure_arithmetic(hiplib):
    size = hiplib.epnet_eval_recall_workspace_bytes
    al = lambda x: (x + 15) & ~15   # noqa: E731
    # the segmentation partials (256 workgroups x 3 int64), the (b,2,g) column maxima, the (b,g,m) IoU matrix
    for b, m, g in ((1, 1, 0), (2, 100, 20), (5, 257, 65), (3, 4096, 1), (65535, 4096, 7)):
        assert size(b, m, g) == al(256 * 3 * 8) + al(b * 2 * g * 4) + al(b * g * m * 4), (b, m, g)
    assert size(0, 100, 20) == 0 and size(1, 0, 20) == 0 and size(1, 4097, 20) == 0 and size(65536, 1, 1) == 0 and size(1, 1, -1) == 0
    assert size(2, 100, 20) == size(2, 100, 20)


def records_call(l, b=2, m=100, ptrs=(P,) * 9):
    boxes, scores, count, p2, shape, rec, cnt, raw, val = ptrs
    return l.epnet_kitti_records(b, m, boxes, scores, count, p2, shape, rec, cnt, raw, val, None)


def test_records_arguments_are_checked_before_a_launch(hiplib):
    l = hiplib
    if not torch.cuda.is_available():
        assert records_call(l) == ELAUNCH and records_call(l, 65535, 4096) == ELAUNCH
        assert records_call(l, ptrs=(P, P, None, P, P, P, P, None, None)) == ELAUNCH      # count, bbox_raw and valid are optional
    assert records_call(l, m=4097) == ELIMIT and records_call(l, b=65536) == ELIMIT and records_call(l, m=0) == ELIMIT
    assert records_call(l, b=-1) == EINVAL and records_call(l, m=-1) == EINVAL
    for k in (0, 1, 3, 4, 5, 6):
        assert records_call(l, ptrs=tuple(None if j == k else P for j in range(9))) == EINVAL, k
    assert records_call(l, b=0) == 0 and records_call(l, b=0, ptrs=(None,) * 9) == 0


# ---- the fixture is what it says ---------------------------------------------------------------------------------------------
def test_fixture_covers_what_it_is_for():
    fx = golden("eval_epoch.npz")
    assert fx["pred_boxes3d"].shape == (4, 48, 7) and fx["det_boxes3d"].shape == (4, 48, 7)
    gt, num_gt, n = fx["gt_boxes3d"], fx["num_gt"], fx["det_count"]
    assert not gt[1].any() and num_gt[1] == 0                                   # a scene without ground truth
    assert not gt[2, :3].any() and gt[2, 3].any() and num_gt[2] == 9            # zero rows in front of a gt row
    assert (n == 0).any() and (n == 48).any()
    det = np.concatenate([fx["det_boxes3d"][k, :n[k]] for k in range(4)])
    valid = np.concatenate([fx["valid"][k, :n[k]] for k in range(4)])
    assert (det[:, 2] < 0).any() and 0 < valid.sum() < valid.size                # behind the camera; some fail the filter
    # IoU clearance: no gt-max IoU within 3e-4 of a threshold
    for key in ("gt_max_iou", "gt_max_iou_in"):
        for k in range(4):
            v = fx[key][k, :num_gt[k]].astype(np.float64)
            assert all(np.abs(v - t).min() > IOU_CLEARANCE for t in fx["thresh_list"]) if v.size else True
    # filter clearance: no clipped width or height within 1e-2 px of its 0.8 bound
    for k in range(4):
        box, (h, w) = fx["img_boxes"][k, :n[k]], fx["img_shape"][k]
        if n[k]:
            assert np.abs((box[:, 2] - box[:, 0]) - w * 0.8).min() > FILTER_CLEARANCE
            assert np.abs((box[:, 3] - box[:, 1]) - h * 0.8).min() > FILTER_CLEARANCE
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "eval_epoch.npz")) < 200000


# ---- the restatement against the reference's own results -------------------------------------------------------------------------
def test_restated_recall_equals_the_reference(oracle):
    fx = golden("eval_epoch.npz")
    iou_p = R.iou_matrices(fx["pred_boxes3d"], fx["gt_boxes3d"])
    iou_r = R.iou_matrices(fx["rois"], fx["gt_boxes3d"])
    nt = len(fx["thresh_list"])
    for first in (0, 2):
        sl = slice(first, first + 2)
        stats, seg, gmp, gmr, pmi = R.eval_recall(iou_p[sl], iou_r[sl], fx["gt_boxes3d"][sl], fx["thresh_list"], fx["seg_result"][sl],
                                                  fx["rpn_cls_label"][sl])
        np.testing.assert_array_equal(stats[:, 0], fx["num_gt"][sl])
        np.testing.assert_array_equal(stats[:, 1:1 + nt], fx["recalled"][sl])
        np.testing.assert_array_equal(stats[:, 1 + nt:], fx["roi_recalled"][sl])
        np.testing.assert_array_equal(seg, fx["seg_counts"][first // 2])
        # the same oracle on both sides: equal, not merely close
        np.testing.assert_array_equal(gmp, fx["gt_max_iou"][sl])
        np.testing.assert_array_equal(gmr, fx["gt_max_iou_in"][sl])
        np.testing.assert_array_equal(pmi, fx["refined_iou"][sl])
    stats, seg, gmp, gmr, _ = R.eval_recall(iou_p, None, fx["gt_boxes3d"], fx["thresh_list"])
    assert seg is None and not stats[:, 1 + nt:].any() and not gmr.any()


def test_restated_records_equal_the_reference():
    """valid flags and rec_count exactly, no row left out; bbox and alpha within the measured bars of the module docstring"""
    fx = golden("eval_epoch.npz")
    rec, cnt, raw, val = R.kitti_records(fx["det_boxes3d"], fx["det_scores"], fx["det_count"], fx["P2"], fx["img_shape"])
    np.testing.assert_array_equal(val, fx["valid"])
    np.testing.assert_array_equal(cnt, fx["valid"].sum(1))
    worst_px = worst_rad = 0.0
    for k in range(4):
        n = int(fx["det_count"][k])
        assert not raw[k, n:].any() and not val[k, n:].any() and not rec[k, cnt[k]:].any()
        if n == 0:
            continue
        worst_px = max(worst_px, float(np.abs(raw[k, :n].astype(np.float64) - fx["img_boxes"][k, :n]).max()))
        _, _, alpha = R.image_boxes(fx["det_boxes3d"][k, :n], fx["P2"][k], fx["img_shape"][k])
        worst_rad = max(worst_rad, float(np.abs(alpha.astype(np.float64) - fx["alpha"][k, :n]).max()))
        # the records against the reference's text lines: every line present, in order, each number within the bars (+ the
        # half unit of the fourth decimal the two roundings can differ by); the copied columns exactly
        lines = [line.split() for line in fx["lines_%d" % k]]
        assert len(lines) == cnt[k]
        want = np.array([[float(v) for v in line[3:]] for line in lines], np.float64).reshape(-1, 13)
        assert all(line[:3] == ["Car", "-1", "-1"] for line in lines)
        np.testing.assert_array_equal(rec[k, :cnt[k], 5:], want[:, 5:])
        assert np.abs(rec[k, :cnt[k], 1:5] - want[:, 1:5]).max() <= BBOX_BAR_PX + 1e-4
        assert np.abs(rec[k, :cnt[k], 0] - want[:, 0]).max() <= ALPHA_BAR_RAD + 1e-4
    print("largest distance to the reference: image box %.4e px, alpha %.4e rad" % (worst_px, worst_rad))
    assert worst_px <= BBOX_BAR_PX and worst_rad <= ALPHA_BAR_RAD


# ---- r4 on the host ------------------------------------------------------------------------------------------------------------
def test_r4_equals_printf_and_strtod(tmp_path):
    """tests/r4_selftest.cpp, built with the host compiler from the header the kernel includes: more than 4 million float32
    values, every exact half-unit tie up to 65536 among them, zero differences"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "r4_selftest")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "epnet_amd", "csrc"),
                           os.path.join(ROOT, "tests", "r4_selftest.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    m = re.fullmatch(r"(\d+) values \((\d+) ties\), 0 differences\n", out.stdout)
    assert m and int(m.group(1)) >= 1000000 and int(m.group(2)) >= 1000000, out.stdout


def test_numpy_r4_equals_python_formatting():
    """a guard on the TEST SIDE only: the numpy r4 of tests/eval_epoch_restate.py, which the GPU tests compare the kernel with,
    against Python's own '%.4f' (the library's r4 is held to printf by the selftest above)"""
    rng = np.random.RandomState(5)
    v = np.concatenate([rng.normal(0, 50, 20000), (np.arange(1, 4001, 2) / 32.0), [-1e-5, -0.0, 0.0, 1241.0, 1e30]]).astype(np.float32)
    got = R.r4(v)
    want = np.array([float("%.4f" % x) for x in v])
    assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))
    assert np.isnan(R.r4(np.float32("nan"))) and R.r4(np.float32("inf")) == np.inf


# ---- the Python layer on CPU tensors over the stand-ins ------------------------------------------------------------------------
@pytest.fixture()
def cpu_surface(monkeypatch, oracle):
    R.install(monkeypatch)
    return "cpu"


def run_epoch(device, with_seg=True):
    """the fixture's four scenes in two batches through EvalEpoch"""
    from epnet_amd import eval_epoch
    fx = golden("eval_epoch.npz")
    ep = eval_epoch.EvalEpoch("Car", fx["thresh_list"])
    for first in (0, 2):
        sl = slice(first, first + 2)
        seg = (T(fx["seg_result"][sl], device), T(fx["rpn_cls_label"][sl], device)) if with_seg else (None, None)
        ep.update(fx["sample_ids"][sl], T(fx["pred_boxes3d"][sl], device), T(fx["rois"][sl], device), T(fx["det_boxes3d"][sl], device),
                  T(fx["det_scores"][sl], device), T(fx["det_count"][sl], device), T(fx["gt_boxes3d"][sl], device),
                  T(fx["P2"][sl], device), T(fx["img_shape"][sl], device), *seg)
    return ep, fx


def check_result(ep, fx):
    ret = ep.result(num_frames=4)
    want = dict(zip(fx["ret_keys"].tolist(), fx["ret_values"].tolist()))
    assert sorted(ret) == sorted(want)
    for key in want:
        assert ret[key] == want[key], (key, ret[key], want[key])      # the rpn_iou quirk included: bit for bit
    assert isinstance(ret["empty_cnt"], int)
    assert ep.result(4, split_ids=[11, 12, 25, 26, 30, 31])["empty_cnt"] == ret["empty_cnt"] + 2


def check_text_round_trip(ep, fx, tmp_path):
    """write_kitti_files -> kitti_eval.get_label_annos == dt_annos(), every key exactly: the end-to-end proof of r4"""
    from epnet_amd import kitti_eval
    ep.write_kitti_files(str(tmp_path))
    ids = [int(s) for s in fx["sample_ids"]]
    assert sorted(os.listdir(str(tmp_path))) == ["%06d.txt" % s for s in ids]
    parsed = kitti_eval.get_label_annos(str(tmp_path), ids)
    annos = ep.dt_annos()
    assert len(annos) == len(parsed) == 4
    for a, p in zip(annos, parsed):
        assert list(a) == list(p)
        for key in p:
            assert a[key].dtype == p[key].dtype and a[key].shape == p[key].shape, key
            np.testing.assert_array_equal(a[key], p[key])
    assert os.path.getsize(os.path.join(str(tmp_path), "%06d.txt" % ids[3])) == 0       # det_count 0: an empty file
    return annos, parsed


def gt_annos_of(fx):
    """KITTI label dicts of the fixture's ground truth (projected with the restatement), for the AP evaluator"""
    annos = []
    for k in range(4):
        n = int(fx["num_gt"][k])
        gt = fx["gt_boxes3d"][k, :n]
        gt = gt[gt.any(1)]
        box, _, alpha = R.image_boxes(gt, fx["P2"][k], fx["img_shape"][k])
        annos.append({"name": np.array(["Car"] * len(gt)), "truncated": np.zeros(len(gt)), "occluded": np.zeros(len(gt), np.int64),
                      "alpha": alpha.astype(np.float64), "bbox": box.astype(np.float64), "dimensions": gt[:, [5, 3, 4]].astype(np.float64),
                      "location": gt[:, 0:3].astype(np.float64), "rotation_y": gt[:, 6].astype(np.float64), "score": np.zeros(len(gt))})
    return annos


def test_epoch_result_equals_the_reference_cpu(cpu_surface):
    ep, fx = run_epoch("cpu")
    check_result(ep, fx)
    ep2, _ = run_epoch("cpu", with_seg=False)                                  # RPN.FIXED: no segmentation inputs
    ret = ep2.result(4)
    assert ret["rpn_iou"] == 0.0 and ret["rcnn_recall(thresh=0.70)"] == dict(zip(fx["ret_keys"], fx["ret_values"]))["rcnn_recall(thresh=0.70)"]


def test_text_round_trip_cpu(cpu_surface, tmp_path):
    ep, fx = run_epoch("cpu")
    annos, parsed = check_text_round_trip(ep, fx, tmp_path)
    import kitti_eval_restate as KR
    gts = gt_annos_of(fx)
    text_a, ap_a = KR.get_official_eval_result(gts, annos, [0])
    text_p, ap_p = KR.get_official_eval_result(gts, parsed, [0])
    assert text_a == text_p and ap_a == ap_p and "Car" in text_a


def test_eval_batch_returns_every_tensor(cpu_surface):
    from epnet_amd import eval_epoch
    fx = golden("eval_epoch.npz")
    totals = torch.zeros((11,), dtype=torch.int64)
    args = [T(fx[k]) for k in ("pred_boxes3d", "rois", "det_boxes3d", "det_scores", "det_count", "gt_boxes3d", "P2", "img_shape")]
    out = eval_epoch.eval_batch(*args, T(fx["seg_result"]), T(fx["rpn_cls_label"]), totals=totals)
    out = eval_epoch.eval_batch(*args, totals=totals)                            # the running sums take two batches
    assert out.seg_counts is None and out.scene_stats.shape == (4, 11) and out.scene_stats.dtype == torch.int32
    np.testing.assert_array_equal(totals.numpy(), 2 * out.scene_stats.numpy().astype(np.int64).sum(0))
    assert out.records.shape == (4, 48, 13) and out.records.dtype == torch.float64 and out.rec_count.dtype == torch.int32
    assert out.gt_max_pred.shape == (4, 12) and out.pred_max_iou.shape == (4, 48) and out.bbox_raw.shape == (4, 48, 4) and out.valid.shape == (4, 48)
    np.testing.assert_array_equal(out.rec_count.numpy(), fx["valid"].sum(1))

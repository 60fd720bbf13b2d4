"""The KITTI AP evaluator without a GPU: the numpy restatement (tests/kitti_eval_restate.py) against the reference's own run
(tests/golden/kitti_eval.npz, written by tests/golden/make_golden_kitti_eval.py), the host op, the annotation helpers, the
import path and the C ABI's argument checks.

Bounds. Metric-0 overlaps: bit-equal (float64, same operation order). Metric 1 / 2: 1e-5 absolute (the reference's float32
functions ran under the interpreter, which accumulates a little differently). No stored overlap lies within 1e-4 of a
min_overlap of the official tables, so every integer statistic is compared exactly, and with them precision, recall and mAP.
similarity: n * 2^-52 * sum for n summed terms."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import kitti_eval_cases as kc
import kitti_eval_restate as kr
from conftest import ROOT

FX = kc.load()
EINVAL, ENOMEM, ELIMIT = -1, -3, -4


@pytest.fixture(scope="module")
def set_a():
    gts, dts = kc.annos(FX, "a_gt"), kc.annos(FX, "a_dt")
    detail = {}
    overlaps = {m: kr.frame_overlaps(gts, dts, m) for m in range(3)}
    result, ret = kr.get_official_eval_result(gts, dts, [0], overlaps, detail)
    return dict(gts=gts, dts=dts, overlaps=overlaps, detail=detail, result=result, ret=ret)


@pytest.fixture(scope="module")
def set_b():
    gts, dts = kc.annos(FX, "b_gt"), kc.annos(FX, "b_dt")
    detail = {}
    result, ret = kr.get_official_eval_result(gts, dts, [2], None, detail)
    return dict(gts=gts, dts=dts, detail=detail, result=result, ret=ret)


def test_fixture_has_what_it_promises():
    gts, dts = kc.annos(FX, "a_gt"), kc.annos(FX, "a_dt")
    assert len(gts) == 60
    ng, nd = FX["a_gt_num"], FX["a_dt_num"]
    assert ((ng == 0) & (nd > 0)).any() and ((ng > 0) & (nd == 0)).any() and ((ng == 0) & (nd == 0)).any()
    assert set(str(n) for g in gts for n in g["name"]) == set(str(n) for n in FX["names"])
    assert set(int(o) for g in gts for o, n in zip(g["occluded"], g["name"]) if n != "DontCare") >= {0, 1, 2}
    assert any(len(d["score"]) >= 3 and len(set(d["score"].tolist())) <= 2 for d in dts), "a frame of deliberately equal scores"
    for m in range(3):
        flat = FX["a_overlaps_m%d" % m]
        assert (flat == 0).any() and np.isfinite(flat).all()
    assert (FX["a_overlaps_m0"] == 1.0).any() and (np.abs(FX["a_overlaps_m1"] - 1.0) < 1e-5).any(), "identical boxes"
    for key in ("a_overlaps_m0", "a_overlaps_m1", "a_overlaps_m2", "b_overlaps_m0", "b_overlaps_m1", "b_overlaps_m2"):
        margin = kr.min_margin([FX[key]])
        print(key, "smallest distance to 0.7 / 0.5 / 0.25: %.3e" % margin)
        assert margin >= kc.MARGIN


def test_restated_overlaps_match_the_reference(set_a):
    for m in range(3):
        want = kc.blocks(FX, "a_overlaps_m%d" % m, set_a["gts"], set_a["dts"])
        worst = 0.0
        for got, ref in zip(set_a["overlaps"][m], want):
            assert got.shape == ref.shape and got.dtype == np.float64
            if m == 0:
                assert np.array_equal(got, ref)
            elif got.size:
                worst = max(worst, float(np.abs(got - ref).max()))
        print("metric %d: max |restatement - reference| %.3e" % (m, worst))
        assert worst <= kc.ROTATED_TOL


@pytest.mark.parametrize("which,prefix,cls", [("set_a", "a_car", 0), ("set_b", "b_cyc", 2)])
def test_restated_statistics_match_the_reference(request, which, prefix, cls):
    s = request.getfixturevalue(which)
    for metric in range(3):
        for l in range(3):
            for k in range(2):
                key = "%s_m%d_c0_d%d_k%d" % (prefix, metric, l, k)
                got = s["detail"][(metric, 0, l, k)]
                assert np.array_equal(got["thresholds"], FX[key + "_thresholds"]), key
                want = FX[key + "_pr"]
                assert np.array_equal(got["pr"][:, :3], want[:, :3]), key
                bound = kc.similarity_bound(got["terms"], want[:, 3])
                assert (np.abs(got["pr"][:, 3] - want[:, 3]) <= bound).all(), (key, got["pr"][:, 3] - want[:, 3], bound)
        curves = s["detail"][("curves", metric)]
        assert np.array_equal(curves["precision"], FX["%s_m%d_precision" % (prefix, metric)])
        assert np.array_equal(curves["recall"], FX["%s_m%d_recall" % (prefix, metric)])
        np.testing.assert_allclose(curves["orientation"], FX["%s_m%d_orientation" % (prefix, metric)], rtol=0,
                                   atol=int(FX[prefix[0] + "_gt_num"].sum()) * 2.0 ** -52)   # aos <= 1 and at most one term per ground-truth row
    assert s["result"] == str(FX[prefix + "_result"])
    assert np.array_equal(np.array([s["ret"][k] for k in sorted(s["ret"])]), FX[prefix + "_ret"])
    assert [str(k) for k in FX[prefix + "_ret_keys"]] == sorted(s["ret"]) and len(s["ret"]) == 9


def test_no_valid_ground_truth_gives_zero_ap_and_no_thresholds(set_b):
    for metric in range(3):
        for l in range(3):
            for k in range(2):
                assert FX["b_cyc_m%d_c0_d%d_k%d_thresholds" % (metric, l, k)].size == 0
                assert set_b["detail"][(metric, 0, l, k)]["thresholds"].size == 0
    assert not FX["b_cyc_ret"].any() and all(v == 0 for v in set_b["ret"].values())


def test_thresholds_host_op_equals_the_reference(hiplib, set_a, set_b):
    import torch
    from epnet_amd import kitti_eval_cuda
    for s, prefix, cls in ((set_a, "a_car", 0), (set_b, "b_cyc", 2)):
        for metric in range(3):
            for l in range(3):
                _, valid = kr.prepare(s["gts"], s["dts"], cls, l)
                for k in range(2):
                    matched = np.concatenate(s["detail"][(metric, 0, l, k)]["matched"] + [np.zeros(0)])
                    got = kitti_eval_cuda.kitti_thresholds_cpu(torch.from_numpy(matched), valid)
                    want = FX["%s_m%d_c0_d%d_k%d_thresholds" % (prefix, metric, l, k)]
                    assert got.dtype == np.float64 and np.array_equal(got, want), (prefix, metric, l, k)
    # capacity, validation
    out = (ctypes.c_double * 4)()
    n = ctypes.c_int(-1)
    scores = (ctypes.c_double * 6)(0.9, 0.8, float("nan"), 0.7, 0.6, 0.5)
    assert hiplib.epnet_kitti_thresholds_host(scores, 6, 5, 41, out, 4, ctypes.byref(n)) == ENOMEM
    assert hiplib.epnet_kitti_thresholds_host(scores, 6, 5, 41, out, 4, None) == EINVAL
    assert hiplib.epnet_kitti_thresholds_host(None, 6, 5, 41, out, 4, ctypes.byref(n)) == EINVAL
    assert hiplib.epnet_kitti_thresholds_host(scores, 6, 0, 41, out, 4, ctypes.byref(n)) == EINVAL
    assert hiplib.epnet_kitti_thresholds_host(None, 0, 0, 41, None, 0, ctypes.byref(n)) == 0 and n.value == 0
    out5 = (ctypes.c_double * 5)()
    assert hiplib.epnet_kitti_thresholds_host(scores, 6, 5, 41, out5, 5, ctypes.byref(n)) == 0
    assert list(out5[:n.value]) == kr.get_thresholds([0.9, 0.8, 0.7, 0.6, 0.5], 5)


def _label_line(a, i, with_score):
    dims = a["dimensions"][i][[1, 2, 0]]   # lhw -> the file's hwl
    vals = [str(a["name"][i]), repr(float(a["truncated"][i])), str(int(a["occluded"][i])), repr(float(a["alpha"][i]))]
    vals += [repr(float(v)) for v in a["bbox"][i]] + [repr(float(v)) for v in dims] + [repr(float(v)) for v in a["location"][i]]
    vals.append(repr(float(a["rotation_y"][i])))
    if with_score:
        vals.append(repr(float(a["score"][i])))
    return " ".join(vals)


def test_label_files_round_trip(tmp_path):
    from epnet_amd import kitti_eval
    gts, dts = kc.annos(FX, "a_gt"), kc.annos(FX, "a_dt")
    for name, annos, with_score in (("gt", gts, False), ("dt", dts, True)):
        os.mkdir(tmp_path / name)
        for f, a in enumerate(annos):
            (tmp_path / name / ("%06d.txt" % f)).write_text("".join(_label_line(a, i, with_score) + "\n" for i in range(len(a["name"]))))
        (tmp_path / name / "notes.txt").write_text("not a label file\n")
    assert any(len(a["name"]) == 0 for a in dts), "an empty file is part of the test"
    for name, annos, ids in (("gt", gts, list(range(len(gts)))), ("dt", dts, None), ("dt", dts[:7], 7)):
        back = kitti_eval.get_label_annos(str(tmp_path / name), ids)
        assert len(back) == len(annos)
        for got, want in zip(back, annos):
            assert [str(n) for n in got["name"]] == [str(n) for n in want["name"]]
            for key in kc.FIELDS:
                assert got[key].shape == want[key].shape, key
                assert np.array_equal(got[key], want[key] if (name == "dt" or key != "score") else np.zeros(len(want["name"]))), key
    one = kitti_eval.get_label_anno(str(tmp_path / "dt" / "000000.txt"))
    assert set(one) == {"name", "truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y", "score"}


def test_clean_data_matches_the_reference():
    from epnet_amd import kitti_eval
    gts, dts = kc.annos(FX, "a_gt"), kc.annos(FX, "a_dt")
    for mod in (kitti_eval, kr):
        for d in range(3):
            rows = [mod.clean_data(g, t, 0, d) for g, t in zip(gts, dts)]
            assert np.array_equal(np.concatenate([np.array(r[1], np.int8) for r in rows]), FX["a_ignored_gt_d%d" % d])
            assert np.array_equal(np.concatenate([np.array(r[2], np.int8) for r in rows]), FX["a_ignored_dt_d%d" % d])
            assert np.array_equal(np.array([r[0] for r in rows]), FX["a_num_valid_gt_d%d" % d])
            assert np.array_equal(np.array([len(r[3]) for r in rows]), FX["a_dc_num"])
    for d in range(3):
        table = FX["a_ignored_gt_d%d" % d]
        assert set(table.tolist()) == {-1, 0, 1} and set(FX["a_ignored_dt_d%d" % d].tolist()) == {-1, 0, 1}


def test_filter_annos_low_score():
    from epnet_amd import kitti_eval
    dts = kc.annos(FX, "a_dt")
    out = kitti_eval.filter_annos_low_score(dts, 0.5)
    assert len(out) == len(dts)
    for got, want in zip(out, dts):
        keep = want["score"] >= 0.5   # a score equal to the threshold stays
        assert set(got) == set(want)
        for key in want:
            assert np.array_equal(got[key], want[key][keep])
    assert any((d["score"] == 0.5).any() for d in dts)


def test_install_evaluator_resolves_the_import_in_a_fresh_process():
    code = ("import sys; from epnet_amd import compat; compat.install_evaluator()\n"
            "from tools.kitti_object_eval_python.evaluate import evaluate as kitti_evaluate\n"
            "from tools.kitti_object_eval_python.eval import get_official_eval_result, clean_data, calculate_iou_partly, eval_class, do_eval, get_mAP\n"
            "from tools.kitti_object_eval_python.rotate_iou import rotate_iou_gpu_eval\n"
            "import tools.kitti_object_eval_python.kitti_common as kitti\n"
            "from epnet_amd import kitti_eval\n"
            "assert kitti_evaluate is kitti_eval.evaluate and kitti.get_label_annos is kitti_eval.get_label_annos\n"
            "assert 'numba' not in sys.modules; print('resolved')\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "resolved", out.stderr


def test_coco_is_not_implemented(tmp_path):
    from epnet_amd import kitti_eval
    with pytest.raises(NotImplementedError, match="coco"):
        kitti_eval.evaluate(str(tmp_path), str(tmp_path), str(tmp_path / "val.txt"), coco=True)
    with pytest.raises(NotImplementedError):
        kitti_eval.get_coco_eval_result([], [], 0)


def test_argument_validation_and_workspace_without_gpu(hiplib):
    fake = ctypes.c_void_p(4096)   # never dereferenced: the calls return before anything touches the device
    diff, mino, nthr = (ctypes.c_int * 2)(0, 1), (ctypes.c_double * 2)(0.7, 0.5), (ctypes.c_int * 2)(41, 3)
    cd, cm, cn = ctypes.cast(diff, ctypes.c_void_p), ctypes.cast(mino, ctypes.c_void_p), ctypes.cast(nthr, ctypes.c_void_p)
    # workspace: 3 int32 and one float64 per (frame, combination, threshold), each array rounded up to 16 bytes
    assert hiplib.epnet_kitti_pr_workspace_bytes(3769, 6, 41) == 3769 * 6 * 41 * 12 + (-(3769 * 6 * 41 * 12) % 16) + 3769 * 6 * 41 * 8 + (-(3769 * 6 * 41 * 8) % 16)
    assert hiplib.epnet_kitti_pr_workspace_bytes(1, 1, 1) == 16 + 16
    for args in ((0, 6, 41), (5, 0, 41), (5, 6, 0), (-1, 6, 41), (5, 17, 41), (5, 6, 65)):
        assert hiplib.epnet_kitti_pr_workspace_bytes(*args) == 0, args
    ov = lambda *a: hiplib.epnet_kitti_overlaps(*a)  # noqa: E731
    assert ov(3, -1, 1, 1, 1, fake, fake, fake, fake, fake, fake, None) == EINVAL          # metric
    assert ov(1, 0, 1, 1, 1, fake, fake, fake, fake, fake, fake, None) == EINVAL           # rotated metrics: criterion -1 only
    assert ov(0, 2, 1, 1, 1, fake, fake, fake, fake, fake, fake, None) == EINVAL
    assert ov(0, -1, -1, 1, 1, fake, fake, fake, fake, fake, fake, None) == EINVAL
    assert ov(0, -1, 1, 1, 1, None, fake, fake, fake, fake, fake, None) == EINVAL
    assert ov(0, -1, 1, 1, 1, fake, fake, fake, fake, fake, None, None) == EINVAL
    assert ov(0, -1, 0, 1, 1, None, None, None, None, None, None, None) == 0               # empty problems are no-ops
    assert ov(2, -1, 4, 0, 3, None, None, None, None, None, None, None) == 0
    match = lambda frames, tg, td, mg, md, nd, c, d=cd, m=cm, p=fake: hiplib.epnet_kitti_match(frames, tg, td, mg, md, nd, c, d, m, p, p, p, p, p, p, p, p, None)  # noqa: E731
    assert match(-1, 4, 4, 2, 2, 3, 2) == EINVAL
    assert match(2, 4, 4, 2, 2, 0, 2) == EINVAL
    assert match(2, 4, 4, 2, 2, 1, 2) == EINVAL            # difficulty 1 of the second combination with one difficulty table
    assert match(2, 4, 4, 2, 2, 3, 2, p=None) == EINVAL
    assert match(2, 4, 4, 2, 2, 3, 2, d=None) == EINVAL
    neg = (ctypes.c_double * 2)(0.7, -0.1)
    assert match(2, 4, 4, 2, 2, 3, 2, m=ctypes.cast(neg, ctypes.c_void_p)) == EINVAL   # min_overlap >= 0
    assert match(0, 0, 0, 0, 0, 3, 2, p=None) == 0 and match(2, 0, 4, 0, 2, 3, 2, p=None) == 0
    pr = lambda frames, c, ts, metric, wsb, mg=2, md=2, mdc=2, n=cn, p=fake: hiplib.epnet_kitti_pr(  # noqa: E731
        frames, 4, 4, mg, md, mdc, 3, c, ts, metric, 1, cd, cm, n, p, p, p, p, p, p, p, p, p, p, p, p, p, p, wsb, p, p, None)
    assert pr(2, 2, 41, 3, 1 << 20) == EINVAL
    assert pr(2, 2, 41, 0, 16) == ENOMEM
    assert pr(2, 2, 40, 0, 1 << 20) == EINVAL              # 41 thresholds asked of a table 40 wide
    assert pr(2, 2, 41, 0, 1 << 20, p=None) == EINVAL
    assert pr(2, 0, 41, 0, 0, p=None) == 0


def test_sizes_beyond_the_limits_return_elimit(hiplib):
    from epnet_amd import kitti_eval_cuda as cu
    fake = ctypes.c_void_p(4096)
    header = open(os.path.join(ROOT, "include", "epnet_ops.h")).read()
    for name, value in (("MAX_DT", cu.MAX_DT), ("MAX_GT", cu.MAX_GT), ("MAX_DC", cu.MAX_DC), ("MAX_COMBOS", cu.MAX_COMBOS),
                        ("MAX_THRESHOLDS", cu.MAX_THRESHOLDS)):
        assert "#define EPNET_KITTI_%s %d " % (name, value) in header
    assert cu.MAX_DT >= 512 and cu.MAX_GT >= 128 and cu.MAX_DC >= 64
    diff, mino, nthr = (ctypes.c_int * 17)(), (ctypes.c_double * 17)(), (ctypes.c_int * 17)()
    cd, cm, cn = ctypes.cast(diff, ctypes.c_void_p), ctypes.cast(mino, ctypes.c_void_p), ctypes.cast(nthr, ctypes.c_void_p)
    assert hiplib.epnet_kitti_overlaps(1, -1, 1, cu.MAX_DT + 1, 1, fake, fake, fake, fake, fake, fake, None) == ELIMIT
    assert hiplib.epnet_kitti_overlaps(2, -1, 1, 1, cu.MAX_GT + 1, fake, fake, fake, fake, fake, fake, None) == ELIMIT
    m = lambda mg, md, c: hiplib.epnet_kitti_match(1, 1, 1, mg, md, 3, c, cd, cm, fake, fake, fake, fake, fake, fake, fake, fake, None)  # noqa: E731
    assert m(cu.MAX_GT + 1, 1, 1) == ELIMIT and m(1, cu.MAX_DT + 1, 1) == ELIMIT and m(1, 1, cu.MAX_COMBOS + 1) == ELIMIT
    p = lambda mg, md, mdc, c, ts: hiplib.epnet_kitti_pr(1, 1, 1, mg, md, mdc, 3, c, ts, 0, 0, cd, cm, cn, fake, fake, fake, fake, fake,  # noqa: E731
                                                         fake, fake, fake, fake, fake, fake, fake, fake, fake, 1 << 20, fake, fake, None)
    assert p(cu.MAX_GT + 1, 1, 1, 1, 1) == ELIMIT and p(1, cu.MAX_DT + 1, 1, 1, 1) == ELIMIT and p(1, 1, cu.MAX_DC + 1, 1, 1) == ELIMIT
    assert p(1, 1, 1, cu.MAX_COMBOS + 1, 1) == ELIMIT and p(1, 1, 1, 1, cu.MAX_THRESHOLDS + 1) == ELIMIT

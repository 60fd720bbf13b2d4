"""The sync-free RCNN training targets without a GPU: epnet_rcnn_sample_rois / epnet_roipool3d_train are declared, exported and
typed; the workspace size is arithmetic; limits and NULL pointers are refused before a launch; and the numpy restatement
(tests/rcnn_targets_restate.py) is pinned to the project's existing truth -- ``ProposalTargetLayer.sample_rois_for_rcnn`` over the
oracle-backed stand-ins, its three host random calls answered from the draw tables, must pick the same ROIs in the same order.

The draw tables of the pinning tests are multiples of 2^-12: ``u * len`` is then exact in float32 and in float64 for every list
of up to 4096 entries, so the existing layer's float64 ``floor(rand * len)`` and the restatement's float32 product cannot differ
by rounding (the restatement's own float32 rule is what the GPU tests hold the kernel to)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden

import rcnn_targets_restate as rs

NEW_SYMBOLS = ("epnet_rcnn_sample_rois", "epnet_rcnn_sample_rois_workspace_bytes", "epnet_roipool3d_train")
EINVAL, ELAUNCH, ENOMEM, ELIMIT = -1, -2, -3, -4
F = np.float32


def T(a, device="cpu"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ---- header / export / binding table ------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_typed(hiplib):
    from epnet_amd import _lib
    text = open(os.path.join(ROOT, "include", "epnet_ops.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    vp, i, f, d, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_size_t
    assert _lib.SIGNATURES["epnet_rcnn_sample_rois_workspace_bytes"] == (sz, [i, i, i, i])
    assert _lib.SIGNATURES["epnet_rcnn_sample_rois"] == (i, [i] * 6 + [f, f, f, d, i] + [vp] * 7 + [sz] + [vp] * 10)
    assert _lib.SIGNATURES["epnet_roipool3d_train"] == (i, [i] * 5 + [f] * 4 + [vp] * 15)
    # the declarations carry as many parameters as the binding table
    for name in ("epnet_rcnn_sample_rois", "epnet_roipool3d_train"):
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name


# ---- the workspace size is arithmetic ------------------------------------------------------------------------------------------------
def test_workspace_bytes(hiplib):
    size = hiplib.epnet_rcnn_sample_rois_workspace_bytes
    al = lambda x: (x + 15) & ~15   # noqa: E731
    for b, m, g, r in ((1, 1, 1, 1), (2, 512, 20, 64), (3, 257, 65, 100), (16, 4096, 8, 1024), (65535, 64, 1, 16)):
        want = al(b * 4) + al(b * m * g * 4) + 2 * al(b * m * 4) + 2 * al(b * r * 4)
        assert size(b, m, g, r) == want, (b, m, g, r)
    assert size(2, 512, 1 << 20, 64) > 2 * 512 * (1 << 20) * 4          # any number of box rows
    for bad in ((0, 512, 20, 64), (-1, 512, 20, 64), (2, 0, 20, 64), (2, 4097, 20, 64), (2, 512, 0, 64), (2, 512, -3, 64),
                (2, 512, 20, 0), (2, 512, 20, 1025), (65536, 512, 20, 64)):
        assert size(*bad) == 0, bad


# ---- argument validation: everything is refused before a launch ----------------------------------------------------------------------
P, WS = 256, 1 << 40      # placeholder pointer (never dereferenced), workspace size that is never short
REQUIRED = 9              # rois, gt, fg_key, slot_u, workspace, batch_rois, batch_gt_of_rois, batch_roi_iou, scene_info


def smp_call(l, b=2, m=512, g=20, gc=7, r=64, fg=32, t=0, req=(P,) * REQUIRED, tables=(None, None), opt=(None,) * 5, ws_bytes=WS):
    rois, gt, key, slot, ws, o_rois, o_gt, o_iou, info = req
    return l.epnet_rcnn_sample_rois(b, m, g, gc, r, fg, 0.55, 0.45, 0.05, 0.8, t, rois, gt, key, slot, tables[0], tables[1], ws, ws_bytes,
                                    o_rois, o_gt, o_iou, info, *opt, None)


def test_sampling_arguments_are_checked_before_a_launch(hiplib):
    l = hiplib
    if not torch.cuda.is_available():                           # (with a GPU the placeholder pointers must not reach a launch)
        assert smp_call(l) == ELAUNCH                           # a shape inside the limits reaches its first launch
        assert smp_call(l, b=65535, m=4096, r=1024, fg=1024) == ELAUNCH and smp_call(l, m=1, g=1, r=1, fg=1) == ELAUNCH
        assert smp_call(l, gc=16, g=1 << 20) == ELAUNCH and smp_call(l, t=10, tables=(P, P), opt=(P,) * 5) == ELAUNCH
    for bad in (dict(m=0), dict(m=4097), dict(r=0, fg=0), dict(r=1025), dict(g=0), dict(b=65536)):
        assert smp_call(l, **bad) == ELIMIT, bad
    for bad in (dict(b=-1), dict(m=-1), dict(g=-1), dict(r=-1), dict(t=-1), dict(fg=-1), dict(gc=6), dict(gc=17), dict(fg=65)):
        assert smp_call(l, **bad) == EINVAL, bad
    for k in range(REQUIRED):                                   # each required pointer on its own
        assert smp_call(l, req=tuple(None if j == k else P for j in range(REQUIRED))) == EINVAL, k
    assert smp_call(l, t=10) == EINVAL and smp_call(l, t=10, tables=(P, None)) == EINVAL and smp_call(l, t=10, tables=(None, P)) == EINVAL
    need = l.epnet_rcnn_sample_rois_workspace_bytes(2, 512, 20, 64)
    assert need > 0 and smp_call(l, ws_bytes=need - 1) == ENOMEM and smp_call(l, ws_bytes=0) == ENOMEM
    if not torch.cuda.is_available():
        assert smp_call(l, ws_bytes=need) == ELAUNCH
    assert smp_call(l, b=0) == 0 and smp_call(l, b=0, req=(None,) * REQUIRED, ws_bytes=0) == 0      # no scene: nothing to do


def test_train_pooling_arguments_are_checked_before_a_launch(hiplib):
    l = hiplib
    # xyz, pts_feature, rois, gt_of_rois, roi_iou, aug | sampled_pts, pts_feature_out, rois_out, gt_out, cls, reg_valid, mask, flag
    call = lambda b, n, m, c, s, ptrs=(P,) * 14: l.epnet_roipool3d_train(b, n, m, c, s, 0.2, 0.55, 0.6, 0.45, *ptrs, None)   # noqa: E731
    s_max = 150 * 1024 // 20                                    # the LDS bound on S, as epnet_roipool3d
    if not torch.cuda.is_available():
        assert call(1, 1000, 64, 5, 512) == ELAUNCH and call(65535, 1000, 1, 5, 512) == ELAUNCH and call(1, 1000, 64, 5, s_max) == ELAUNCH
        assert call(1, 1000, 64, 5, 512, tuple(None if j == 5 else P for j in range(14))) == ELAUNCH      # aug may be NULL
    assert call(65536, 1000, 64, 5, 512) == ELIMIT and call(1, 1000, 64, 5, s_max + 1) == ELIMIT
    for bad in ((-1, 10, 10, 1, 8), (1, -1, 10, 1, 8), (1, 10, -1, 1, 8), (1, 10, 10, -1, 8), (1, 10, 10, 1, -8)):
        assert call(*bad) == EINVAL, bad
    for k in (0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13):
        assert call(1, 1000, 64, 5, 32, tuple(None if j == k else P for j in range(14))) == EINVAL, k
    assert call(0, 1000, 64, 5, 32, (None,) * 14) == 0 and call(2, 1000, 0, 5, 32, (None,) * 14) == 0


def test_surface_refuses_cpu_tensors_and_the_normal_method(hiplib):
    from epnet_amd import iou3d_cuda, rcnn_target_layer as rtl, roipool3d_cuda
    cfg = rtl.default_cfg()
    tables = rtl.draw_sampling_tables(1, 8, cfg, "cpu", torch.Generator().manual_seed(1))
    with pytest.raises(RuntimeError, match="CUDAtensor"):
        rtl.sample_rois(torch.zeros((1, 8, 7)), torch.zeros((1, 2, 7)), tables, cfg)
    with pytest.raises(RuntimeError, match="CUDAtensor"):
        rtl.pool_targets(torch.zeros((1, 8, 3)), torch.zeros((1, 8, 2)), torch.zeros((1, 4, 7)), torch.zeros((1, 4, 7)), torch.zeros((1, 4)), None, cfg)
    z = torch.zeros((1, 4, 7))
    with pytest.raises(RuntimeError, match="CUDAtensor"):
        iou3d_cuda.rcnn_sample_rois_gpu(z, z, torch.zeros((1, 4)), torch.zeros((1, 4)), None, None, 2, 0.55, 0.45, 0.05, 0.8, z, z,
                                        torch.zeros((1, 4)), torch.zeros((1, 6), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="CUDAtensor"):
        roipool3d_cuda.forward_train(torch.zeros((1, 8, 3)), torch.zeros((1, 8, 2)), z, z, torch.zeros((1, 4)), None, 0.2, 0.55, 0.6, 0.45,
                                     *[torch.zeros((4,))] * 8)
    cfg.RCNN.REG_AUG_METHOD = "normal"
    with pytest.raises(NotImplementedError):
        rtl.draw_sampling_tables(1, 8, cfg, "cpu")
    with pytest.raises(NotImplementedError):
        rtl.RCNNTargetLayer(cfg)({"roi_boxes3d": torch.zeros((1, 8, 7)), "gt_boxes3d": torch.zeros((1, 2, 7))})
    with pytest.raises(RuntimeError, match="int32"):
        rtl.RCNNTargetLayer(rtl.default_cfg(), label_dtype=torch.float32)


# ---- the draw tables -------------------------------------------------------------------------------------------------------------------
def test_draw_sampling_tables_rules():
    from epnet_amd import rcnn_target_layer as rtl
    cfg = rtl.default_cfg()
    t = rtl.draw_sampling_tables(50, 512, cfg, "cpu", torch.Generator().manual_seed(2))
    assert tuple(t["fg_key"].shape) == (50, 512) and tuple(t["slot_u"].shape) == (50, 64)
    assert tuple(t["keep_draw"].shape) == (3200, 10) and t["keep_draw"].dtype == torch.uint8 and tuple(t["noise"].shape) == (3200, 10, 7)
    for u in (t["fg_key"], t["slot_u"]):
        assert u.dtype == torch.float32 and float(u.min()) >= 0 and float(u.max()) < 1 and abs(float(u.mean()) - 0.5) < 0.02
    aug = t["aug"]
    assert tuple(aug.shape) == (50, 64, 3) and aug.dtype == torch.float32
    bound = np.pi / 18
    # the reference's `- 0.5 / 0.5` (:302): the draw minus ONE, an angle in [-pi / 18, 0)
    assert float(aug[..., 0].max()) <= 0 and float(aug[..., 0].min()) >= -bound - 1e-6 and float(aug[..., 0].min()) < -0.9 * bound
    assert float(aug[..., 1].min()) >= 0.95 - 1e-6 and float(aug[..., 1].max()) <= 1.05 + 1e-6 and float(aug[..., 1].max()) > 1.04
    assert set(aug[..., 2].unique().tolist()) <= {-1.0, 0.0, 1.0} and abs(float((aug[..., 2] == 1).float().mean()) - 0.5) < 0.05
    u = [torch.rand((2, 4), generator=torch.Generator().manual_seed(k)) for k in (5, 6, 7)]
    got = rtl.aug_table_from_draws(*u, cfg)
    assert torch.equal(got[..., 0], ((u[0] - 0.5 / 0.5) * (np.pi / 18)).float()) and torch.equal(got[..., 2], torch.sign(u[2] - 0.5))
    cfg.AUG_DATA, cfg.RCNN.ROI_FG_AUG_TIMES = False, 0
    t = rtl.draw_sampling_tables(2, 16, cfg, "cpu")
    assert t["aug"] is None and t["keep_draw"] is None and t["noise"] is None


def test_install_callers_serves_the_sync_free_layer_on_request():
    import sys
    from epnet_amd import compat, proposal_target_layer as ptl, rcnn_target_layer as rtl
    saved = {k: sys.modules.get(k) for k in list(sys.modules) if k == "lib" or k.startswith("lib.") or k.endswith("_cuda")}
    try:
        compat.install_callers()
        assert sys.modules["lib.rpn.proposal_target_layer"].ProposalTargetLayer is ptl.ProposalTargetLayer      # the default stays
        compat.install_callers(sync_free=True)
        mod = sys.modules["lib.rpn.proposal_target_layer"]
        assert mod.ProposalTargetLayer is rtl.RCNNTargetLayer and sys.modules["lib.rpn"].proposal_target_layer is mod
        assert sys.modules["lib.rpn.proposal_layer"].ProposalLayer.__module__ == "epnet_amd.proposal_layer"
    finally:
        for k in [k for k in sys.modules if k == "lib" or k.startswith("lib.") or k in ("pointnet2_cuda", "iou3d_cuda", "roipool3d_cuda")]:
            del sys.modules[k]
        sys.modules.update({k: v for k, v in saved.items() if v is not None})


# ---- the restatement's pieces ----------------------------------------------------------------------------------------------------------
def test_restatement_pieces():
    keys = rs.ordered_key(np.array([-np.inf, -1.0, -0.0, 0.0, 1e-30, 0.5, np.inf, np.nan], F))
    assert keys[2] == keys[3] and list(keys) == sorted(keys) and keys[-1] == 0xFFFFFFFF
    gt = np.zeros((5, 8), F)
    assert rs.count_gt(gt) == 0
    gt[1, 7] = 2.0                                               # a column beyond the seven box columns counts (:105)
    gt[3, 0:2] = (1.0, -1.0)                                     # a row whose sum is 0 is padding when it is the last one
    assert rs.count_gt(gt) == 2
    gt[4, 2] = np.nan
    assert rs.count_gt(gt) == 5
    assert [rs.pick_pos(u, 7) for u in (0.0, 0.999, np.nan, -0.1, 1.0, 3.0)] == [0, 6, 0, 0, 6, 6]
    assert rs.pick_pos(F(1) - F(2.0 ** -24), 3) == 2 and rs.pick_pos(F(1) - F(2.0 ** -24), 4096) == 4095
    assert rs.row_max_first(np.array([0.1, 0.7, 0.7, np.nan, 0.9, np.nan], F))[1] == 3
    # hand-checkable selection: 3 fg (ROIs 1, 4, 5), 2 hard (0, 3), 1 easy (2)
    iou = np.array([[0.3, 0.1], [0.1, 0.9], [0.0, 0.01], [0.2, 0.2], [0.7, 0.7], [0.6, 0.56]], F)
    s = rs.select(iou, np.array([0, 0.5, 0, 0, 0.2, 0.5], F), np.array([0.9, 0.9, 0.0, 0.6, 0.99, 0.3, 0.0, 0.7], F), 8, 2, 0.55, 0.45, 0.05, 0.8, 10)
    assert s["gt_assignment"].tolist() == [0, 1, 1, 0, 0, 0] and s["case"] == 0 and s["fg_this"] == 2 and s["counts"] == (3, 2, 1)
    # slots 0-1: keys 0.2 (ROI 4), then the tie 0.5 by index (ROI 1); 6 background slots, int(6 * 0.8) = 4 hard, 2 easy
    assert s["src_inds"].tolist() == [4, 1, 0, 3, 3, 0, 2, 2] and s["tries"].tolist() == [10, 10, 1, 1, 1, 1, 1, 1]


# ---- the restatement against the existing layer over the oracle-backed stand-ins -----------------------------------------------------------
@pytest.fixture()
def cpu_surface(monkeypatch, oracle):
    import oracle_ext
    from epnet_amd import iou3d_cuda, pointnet2_cuda, roipool3d_cuda
    p2, iou, rp = oracle_ext.make_modules()
    for real, fake in ((pointnet2_cuda, p2), (iou3d_cuda, iou), (roipool3d_cuda, rp)):
        for name, fn in vars(fake).items():
            if callable(fn):
                monkeypatch.setattr(real, name, fn)
    return "cpu"


def coarse_tables(b, m, r, seed):
    """uniform draws on the grid of 2^-12 (see the module docstring), with equal keys among them"""
    rng = np.random.RandomState(seed)
    return (rng.randint(0, 4096, (b, m)) / 4096.0).astype(F), (rng.randint(0, 4096, (b, r)) / 4096.0).astype(F)


def existing_layer_against_restatement(monkeypatch, oracle, rois, gt, per_image, seed, aug_times=10):
    """-> the restatement's dict, after asserting that the existing layer, its host random calls answered from the tables, picked
    the same rows in the same order"""
    from epnet_amd import proposal_target_layer as ptl
    cfg = ptl.default_cfg()
    cfg.RCNN.NUM_POINTS, cfg.RCNN.ROI_PER_IMAGE, cfg.RCNN.ROI_FG_AUG_TIMES = 32, per_image, aug_times
    fg_per_image = int(np.round(cfg.RCNN.FG_RATIO * per_image))
    b, m = rois.shape[0], rois.shape[1]
    fg_key, slot_u = coarse_tables(b, m, per_image, seed)
    matrices = [oracle.boxes_iou3d(rois[k], np.ascontiguousarray(gt[k, :, 0:7])) for k in range(b)]   # what the stand-in hands the layer
    want = rs.sample(rois, gt, lambda k, num_gt: matrices[k][:, :num_gt], fg_key, slot_u, per_image, fg_per_image, 0.55,
                     cfg.RCNN.CLS_BG_THRESH, cfg.RCNN.CLS_BG_THRESH_LO, cfg.RCNN.HARD_BG_RATIO, aug_times)

    state = {"scene": 0, "slot": 0}

    def scene_of_call():
        if state["slot"] >= per_image:
            state["scene"], state["slot"] = state["scene"] + 1, 0
        return state["scene"]

    def permutation(fg_num):                 # :133 -- positions of the foreground list in ascending (key, index) order
        k = scene_of_call()
        assert state["slot"] == 0
        ov = matrices[k][:, :max(rs.count_gt(gt[k]), 1)].max(axis=1)
        fg = np.nonzero(ov >= F(0.55))[0]
        assert fg.size == fg_num
        state["slot"] = min(fg_per_image, fg_num)
        return np.lexsort((fg, rs.ordered_key(fg_key[k][fg])))

    def rand(count):                          # :142 -- the slots' own draws
        k = scene_of_call()
        out = slot_u[k, state["slot"]:state["slot"] + count].astype(np.float64)
        state["slot"] += count
        return out

    def randint(high, size):                  # :197-213 -- floor(u * high) of the next `size` slots
        k = scene_of_call()
        out = np.array([rs.pick_pos(slot_u[k, state["slot"] + i], int(high)) for i in range(int(size))], np.int64)
        state["slot"] += int(size)
        return out

    monkeypatch.setattr(np.random, "permutation", permutation)
    monkeypatch.setattr(np.random, "rand", rand)
    monkeypatch.setattr(ptl.ProposalTargetLayer, "_randint", staticmethod(randint))
    monkeypatch.setattr(ptl, "draw_aug_tables", lambda k, t, method, dev, gen: (torch.ones((k, t), dtype=torch.uint8), torch.zeros((k, t, 7))))
    got_rois, got_gt, got_iou = ptl.ProposalTargetLayer(cfg).sample_rois_for_rcnn(T(rois), T(gt))
    assert state["scene"] == b - 1 and state["slot"] == per_image              # every slot of every scene was answered
    np.testing.assert_array_equal(got_rois.numpy(), want["batch_rois"])        # same ROIs picked, in the same order
    np.testing.assert_array_equal(got_gt.numpy(), want["batch_gt_of_rois"])    # same ground truth assigned
    np.testing.assert_array_equal(got_iou.numpy(), want["iou_src"])            # identity noise: the IoU of the pick
    return want


def test_restatement_picks_what_the_existing_layer_picks_on_the_fixture(cpu_surface, monkeypatch, oracle):
    fx = golden("proposal_target.npz")
    rois, gt = fx["smp__roi_boxes3d"], fx["smp__gt_boxes3d"]
    want = existing_layer_against_restatement(monkeypatch, oracle, rois, gt, 16, seed=3)
    assert want["scene_info"][:, 1:4].tolist() == [[85, 24, 1], [90, 24, 0], [71, 42, 0]]
    assert want["scene_info"][:, 4:6].tolist() == [[8, 0]] * 3
    for thresh in (0.55, 0.45, 0.05):                                          # no ROI within 1e-4 of a threshold
        assert float(np.abs(want["max_overlaps"].astype(np.float64) - thresh).min()) > 1e-4
    # every ROI of a scene is distinct, so equal rows mean equal picks
    assert all(len({r.tobytes() for r in rois[k]}) == rois.shape[1] for k in range(3))


def shifted_rois(shifts):
    """ROIs = the ground-truth box moved along x: IoU falls from 1 (shift 0) to 0 (beyond the box)"""
    gt = np.zeros((1, 4, 7), F)
    gt[0, 0] = (0.0, 1.6, 20.0, 1.5, 1.6, 3.9, 0.3)
    gt[0, 2] = (30.0, 1.5, 40.0, 1.4, 1.5, 3.6, -1.2)                          # a zero row in front of it
    rois = np.repeat(gt[:, 0:1], len(shifts), axis=1).copy()
    rois[0, :, 0] += np.asarray(shifts, F)
    return rois, gt


@pytest.mark.parametrize("name,shifts,case,counts", [
    ("fg only", np.linspace(0.0, 0.6, 23), 1, (23, 0, 0)),
    ("bg only", np.concatenate([np.linspace(1.6, 2.8, 9), np.linspace(6.0, 9.0, 11)]), 2, (0, 9, 11)),
    ("only easy", np.linspace(6.0, 12.0, 19), 2, (0, 0, 19)),
    ("only hard", np.linspace(1.6, 2.8, 21), 2, (0, 21, 0)),
    ("both, fewer fg than slots", np.concatenate([np.linspace(0.0, 0.4, 3), np.linspace(1.6, 2.8, 9), np.linspace(6.0, 9.0, 5)]), 0, (3, 9, 5)),
])
def test_restatement_picks_what_the_existing_layer_picks_on_generated_scenes(cpu_surface, monkeypatch, oracle, name, shifts, case, counts):
    rois, gt = shifted_rois(shifts)
    want = existing_layer_against_restatement(monkeypatch, oracle, rois, gt, 16, seed=len(shifts))
    assert want["scene_info"][0].tolist() == [3, *counts, {0: min(8, counts[0]), 1: 16, 2: 0}[case], case], name

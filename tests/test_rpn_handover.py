"""The RPN hand-over without a GPU: the library's argument checks and limits, the Python surface (CPU tensors refused, the
``cfg`` keys read, every switch off by default) and the DESIGN OF THE GPU TEST: on the very inputs tests/test_rpn_handover_gpu.py
uses, the stock float32 composition on the CPU must itself pass that test's tolerance against float64, and the exclusion rule
must leave out at most 1 % of the rows (tests/handover_cases.py states both)."""
import ctypes
import inspect
import types

import numpy as np
import pytest
import torch

import handover_cases as hc

EINVAL, ENOMEM, ELIMIT = -1, -3, -4
FAKE = ctypes.c_void_p(4096)          # never dereferenced: the calls return before anything touches the device
SIZE = (ctypes.c_float * 3)(*hc.ANCHOR_SIZE.tolist())
SIZE_P = ctypes.cast(SIZE, ctypes.c_void_p)


def decode_args(rows=64, acols=3, channels=76, bins_xz=12, bins_y=4, nh=12, xz_fine=1, y_by_bin=0, ry_fine=0, avg=1, ry_bin=0,
                anchors=FAKE, reg=FAKE, size=SIZE_P, boxes=FAKE):
    return (rows, acols, anchors, reg, channels, bins_xz, bins_y, 3.0, 0.5, 0.5, 0.25, nh, size, xz_fine, y_by_bin, ry_fine, avg, ry_bin,
            0, boxes, None)


def handover_args(b=2, n=16384, channels=76, bins_xz=12, nh=12, xz_fine=1, avg=1, pre=9000, post=512, ws=FAKE, ws_bytes=1 << 40,
                  scores=FAKE, reg=FAKE, xyz=FAKE, bbox=FAKE, ret_scores=FAKE):
    return (b, n, channels, scores, reg, xyz, bins_xz, 4, 3.0, 0.5, 0.5, 0.25, nh, SIZE_P, xz_fine, 0, 0, avg, 0, 0.3, 1, pre, post, 0.85,
            0, ws, ws_bytes, bbox, ret_scores, None, None, None, None, None, None)


def test_decode_argument_checks_without_a_gpu(hiplib):
    f = hiplib.epnet_decode_bbox_target
    # the channel-count rule: (xz_fine ? 4 : 2) * bins_xz + (y_by_bin ? 2 * bins_y : 1) + 2 * num_head_bin + 3
    for kw in (dict(channels=75), dict(channels=77), dict(channels=76, xz_fine=0, avg=0), dict(channels=76, y_by_bin=1),
               dict(channels=46, bins_xz=6, nh=12), dict(channels=0), dict(bins_xz=0, channels=28), dict(nh=0, channels=52)):
        assert f(*decode_args(**kw)) == EINVAL, kw
    for kw in (dict(), dict(channels=52, xz_fine=0, avg=0), dict(channels=83, y_by_bin=1), dict(channels=46, bins_xz=6, nh=9, acols=7),
               dict(channels=53, bins_xz=6, nh=9, acols=7, y_by_bin=1, ry_fine=1)):
        assert f(*decode_args(rows=0, **kw)) == 0, kw                       # a well-formed empty problem
    for acols in (0, 1, 4, 6, 8):
        assert f(*decode_args(acols=acols)) == EINVAL, acols
    assert f(*decode_args(channels=52, xz_fine=0, avg=1)) == EINVAL         # avg_by_bin without xz_fine: the reference asserts
    assert f(*decode_args(rows=-1)) == EINVAL
    assert f(*decode_args(rows=0, anchors=None, reg=None, size=None, boxes=None)) == 0     # rows == 0: nothing is looked at
    for kw in (dict(anchors=None), dict(reg=None), dict(size=None), dict(boxes=None)):
        assert f(*decode_args(**kw)) == EINVAL, kw
    assert f(*decode_args(channels=4 * 60 + 1 + 24 + 3, bins_xz=60)) == ELIMIT                  # 268 channels: beyond the LDS tile


def test_order_limits_without_a_gpu(hiplib):
    f = hiplib.epnet_score_order
    assert f(1, 16385, FAKE, FAKE, None) == ELIMIT and f(1, 0, FAKE, FAKE, None) == ELIMIT and f(65536, 16, FAKE, FAKE, None) == ELIMIT
    assert f(0, 16, None, None, None) == 0 and f(0, 16385, None, None, None) == 0
    assert f(-1, 16, FAKE, FAKE, None) == EINVAL and f(1, -1, FAKE, FAKE, None) == EINVAL
    assert f(1, 16, None, FAKE, None) == EINVAL and f(1, 16, FAKE, None, None) == EINVAL


def test_handover_limits_and_workspace_without_a_gpu(hiplib):
    f, size, inner = hiplib.epnet_rpn_handover, hiplib.epnet_rpn_handover_workspace_bytes, hiplib.epnet_rpn_proposals_workspace_bytes
    assert f(*handover_args(n=16385)) == ELIMIT and f(*handover_args(n=0)) == ELIMIT and f(*handover_args(b=32768)) == ELIMIT
    assert f(*handover_args(b=0, scores=None, reg=None, xyz=None, bbox=None, ret_scores=None, ws=None, ws_bytes=0)) == 0
    assert f(*handover_args(b=-1)) == EINVAL and f(*handover_args(post=0)) == EINVAL
    assert f(*handover_args(channels=75)) == EINVAL and f(*handover_args(channels=52, xz_fine=0, avg=1)) == EINVAL
    for kw in (dict(scores=None), dict(reg=None), dict(xyz=None), dict(bbox=None), dict(ret_scores=None)):
        assert f(*handover_args(**kw)) == EINVAL, kw
    assert f(*handover_args(ws=None)) == ENOMEM and f(*handover_args(ws_bytes=size(2, 16384, 1, 9000, 512) - 1)) == ENOMEM
    for b, n, dist, pre, post in ((1, 1, 1, 9000, 512), (2, 16384, 1, 9000, 512), (3, 2048, 0, 9000, 100), (256, 16384, 1, 9000, 100)):
        rows = b * n
        want = (rows * 28 + 15) // 16 * 16 + (rows * 8 + 15) // 16 * 16 + inner(b, dist, pre, post)      # proposals, order, the proposal kernels' own
        assert size(b, n, dist, pre, post) == want and want >= inner(b, dist, pre, post) > 0, (b, n, dist, pre, post)
    for b, n in ((0, 16384), (1, 0), (1, 16385), (32768, 16), (-1, 16)):
        assert size(b, n, 1, 9000, 512) == 0, (b, n)
    assert size(1, 16, 1, -1, 512) == 0 and size(1, 16, 1, 9000, -1) == 0


def test_cpu_tensors_are_rejected(hiplib):
    from epnet_amd import handover_cuda, rpn_handover
    anchor, reg = hc.case("rpn_soft", 64, 1.0)
    with pytest.raises(RuntimeError, match="CUDAtensor"):
        rpn_handover.decode_boxes(anchor, reg, 3.0, 0.5, 12, hc.ANCHOR_SIZE)
    with pytest.raises(RuntimeError, match="CUDAtensor"):
        rpn_handover.score_order(torch.zeros((1, 8)))
    with pytest.raises(RuntimeError, match="CUDAtensor"):
        rpn_handover.rpn_handover(torch.zeros((1, 64, 1)), reg.view(1, 64, 76), anchor.view(1, 64, 3))
    with pytest.raises(RuntimeError, match="CUDAtensor"):
        handover_cuda.score_order_gpu(torch.zeros((1, 8)), torch.zeros((1, 8), dtype=torch.int64))
    with pytest.raises(RuntimeError, match="3 numbers"):
        handover_cuda._anchor3([1.0, 2.0])


def test_too_many_points_name_the_op_and_the_limit():
    from epnet_amd import _lib, rpn_handover
    with pytest.raises(_lib.EpnetError, match="rpn_handover.*16384"):
        rpn_handover.rpn_handover(torch.zeros((1, 16385, 1)), torch.zeros((1, 16385, 76)), torch.zeros((1, 16385, 3)))


def _cfg(**rpn):
    from epnet_amd import proposal_layer
    cfg = proposal_layer.default_cfg()
    for k, v in rpn.items():
        setattr(cfg.RPN, k, v)
    return cfg


def test_the_cfg_keys_are_read(monkeypatch):
    from epnet_amd import rpn_handover
    a = rpn_handover.handover_args(_cfg(), "TRAIN")
    assert (a["loc_scope"], a["loc_bin_size"], a["num_head_bin"], a["xz_fine"], a["avg_by_bin"], a["ry_with_bin"]) == (3.0, 0.5, 12, True, True, False)
    assert (a["pre_nms_top_n"], a["post_nms_top_n"], a["nms_thresh"], a["distance_based"], a["rotated"]) == (9000, 512, 0.85, True, False)
    assert a["score_thresh"] == 0.3 and np.array_equal(a["anchor_size"], hc.ANCHOR_SIZE)
    t = rpn_handover.handover_args(_cfg(), "TEST")
    assert (t["post_nms_top_n"], t["nms_thresh"]) == (100, 0.8)
    cfg = _cfg(LOC_SCOPE=1.5, LOC_BIN_SIZE=0.25, NUM_HEAD_BIN=9, LOC_XZ_FINE=False, NMS_TYPE="rotate", SCORE_THRESH=0.45)
    cfg.TRAIN.BBOX_AVG_BY_BIN, cfg.TEST.RY_WITH_BIN, cfg.CLS_MEAN_SIZE = False, True, np.array([[1.0, 2.0, 3.0]])
    cfg.TRAIN.RPN_PRE_NMS_TOP_N, cfg.TRAIN.RPN_POST_NMS_TOP_N, cfg.TRAIN.RPN_NMS_THRESH = 700, 64, 0.5
    a = rpn_handover.handover_args(cfg, "TRAIN")
    assert (a["loc_scope"], a["loc_bin_size"], a["num_head_bin"], a["xz_fine"], a["avg_by_bin"], a["ry_with_bin"]) == (1.5, 0.25, 9, False, False, True)
    assert (a["pre_nms_top_n"], a["post_nms_top_n"], a["nms_thresh"], a["rotated"], a["score_thresh"]) == (700, 64, 0.5, True, 0.45)
    assert a["anchor_size"].tolist() == [1.0, 2.0, 3.0]
    cfg.TEST.RPN_DISTANCE_BASED_PROPOSE = False                             # cfg.TEST's switch in both modes; score-based: the rotated NMS
    cfg.RPN.NMS_TYPE = "normal"
    a = rpn_handover.handover_args(cfg, "TRAIN")
    assert a["distance_based"] is False and a["rotated"] is True
    cfg.TEST.RPN_DISTANCE_BASED_PROPOSE, cfg.RPN.NMS_TYPE = True, "soft"
    with pytest.raises(NotImplementedError):
        rpn_handover.handover_args(cfg, "TRAIN")
    # the reference's global config when its module is loaded
    import sys
    mod = types.ModuleType("lib.config")
    mod.cfg = _cfg(NUM_HEAD_BIN=7)
    monkeypatch.setitem(sys.modules, "lib.config", mod)
    assert rpn_handover._ambient_cfg() is mod.cfg


def test_every_switch_defaults_to_off():
    from epnet_amd import compat, detection_layer, proposal_layer
    assert proposal_layer.ProposalLayer().fused_head is False and proposal_layer.ProposalLayer("TEST", fused_head=True).fused_head is True
    assert detection_layer.DetectionLayer().fused_decode is False and detection_layer.DetectionLayer(fused_decode=True).fused_decode is True
    assert inspect.signature(proposal_layer.ProposalLayer.__init__).parameters["fused_head"].default is False
    assert inspect.signature(detection_layer.DetectionLayer.__init__).parameters["fused_decode"].default is False
    sig = inspect.signature(compat.install_callers).parameters
    assert sig["fused_head"].default is False and sig["sync_free"].default is False
    import bench_step
    assert "--proposals" in inspect.getsource(bench_step) and bench_step.PROPOSALS_DEFAULT == "composed"


def test_install_callers_serves_the_fused_layer():
    import sys
    from epnet_amd import compat, proposal_layer
    mine = lambda name: name == "lib" or name.startswith("lib.") or name in compat._EXT  # noqa: E731
    before = {name: mod for name, mod in sys.modules.items() if mine(name)}
    try:
        for name in before:
            if name not in compat._EXT:
                del sys.modules[name]
        compat.install_callers()
        assert sys.modules["lib.rpn.proposal_layer"] is proposal_layer
        compat.install_callers(fused_head=True)
        served = sys.modules["lib.rpn.proposal_layer"].ProposalLayer
        assert issubclass(served, proposal_layer.ProposalLayer) and served(mode="TEST").fused_head is True and served().mode == "TRAIN"
        assert sys.modules["lib.rpn.proposal_layer"].default_cfg is proposal_layer.default_cfg
    finally:                                                                # leave sys.modules as it was found
        for name in [name for name in sys.modules if mine(name)]:
            del sys.modules[name]
        sys.modules.update(before)


# ---- the design of the GPU test ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(hc.CONFIGS))
def test_the_stock_float32_composition_passes_the_gpu_tolerance(name):
    cfg = hc.CONFIGS[name]
    left_out = total = 0
    for rows in hc.ROWS:
        for scale in hc.SCALES:
            anchor, reg = hc.case(name, rows, scale)
            ref, skip = hc.case_reference(name, rows, scale)
            stock = hc.decode_bbox_target(anchor.clone(), reg.clone(), anchor_size=torch.from_numpy(hc.ANCHOR_SIZE), **hc.decode_kwargs(cfg))
            assert reg.shape[1] == hc.channels(cfg)
            if rows >= 1000:
                hc.check(stock, ref, skip, "%s rows %d scale %g" % (name, rows, scale))
            else:                       # too few rows for a share: the tolerances alone
                size, heading = hc.errors(stock, ref, skip)
                assert size <= 1.0 and heading <= hc.TOL, (name, rows, scale, size, heading)
            left_out += int(skip.sum())
            total += rows
            if not cfg["ry_with_bin"]:
                assert not bool(skip.any())
    assert left_out <= 0.01 * total, (name, left_out, total)


def test_the_inputs_hold_exact_ties_and_the_first_maximum_wins():
    """float16-rounded logits tie exactly; float32 and float64 then pick the same (first) bin"""
    anchor, reg = hc.case("rpn_hard", 4099, 1.0)
    seen = 0
    for at in (0, 12, 49):                                                  # x bins, z bins, heading bins
        bins = reg[:, at:at + 12]
        top = bins.max(dim=1, keepdim=True)[0]
        tied = (bins == top).sum(dim=1) > 1
        seen += int(tied.sum())
        first = torch.argmax(bins[tied], dim=1)
        assert torch.equal(first, (bins[tied] == top[tied]).float().argmax(dim=1)) and torch.equal(first, torch.argmax(bins[tied].double(), dim=1))
    assert seen > 0


def test_the_end_to_end_inputs():
    for n in (2048, 16384):
        scores, reg, xyz = hc.scene_inputs(n)
        assert scores.shape == (2, n) and reg.shape == (2, n, 76) and xyz.shape == (2, n, 3)
        assert all(len(torch.unique(s)) == n for s in scores)                                        # distinct
        assert bool((xyz[0, :, 2] > 40).any()) and not bool((xyz[1, :, 2] > 40).any())               # scene 1: the empty far bin
        prob = torch.sigmoid(scores.double())
        near = (prob - 0.3).abs() <= 1e-6
        assert float(near.float().mean()) <= 0.001
        assert bool((prob > 0.31).any()) and bool((prob < 0.29).any())                               # rows well to either side

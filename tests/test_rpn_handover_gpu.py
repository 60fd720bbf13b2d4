"""The RPN hand-over on the GPU (csrc/handover.hip through epnet_amd.rpn_handover): decode parity against the float64
yardstick, the exact stable order, the one-call hand-over end to end, graph capture, and the opt-in switches. Inputs, yardstick,
exclusion rule and tolerances: tests/handover_cases.py (checked on the CPU by tests/test_rpn_handover.py)."""
import math

import pytest
import torch

import handover_cases as hc
from conftest import GuardedAlloc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _guard_the_handover_allocations(monkeypatch):
    """canaries around what handover_cuda (the workspace) and rpn_handover (every output) allocate themselves"""
    from epnet_amd import handover_cuda, rpn_handover
    g = GuardedAlloc()

    class _TorchProxy:
        def __getattr__(self, name):
            return getattr(torch, name)

        @staticmethod
        def empty(*shape, dtype=torch.float32, device=None, **kw):
            if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
                shape = tuple(shape[0])
            if device is not None and torch.device(device).type == "cuda" and not kw:
                return g.alloc(shape, dtype, device)
            return torch.empty(shape, dtype=dtype, device=device, **kw)

    proxy = _TorchProxy()
    monkeypatch.setattr(handover_cuda, "torch", proxy)
    monkeypatch.setattr(rpn_handover, "torch", proxy)
    yield
    torch.cuda.synchronize()
    g.check()


def gpu_decode(cfg, anchor, reg, y_to_bottom=False):
    from epnet_amd import rpn_handover
    box = rpn_handover.decode_boxes(anchor.to(DEV), reg.to(DEV), anchor_size=hc.ANCHOR_SIZE, y_to_bottom=y_to_bottom, **hc.decode_kwargs(cfg))
    return box.cpu()


# ---- 1. decode parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(hc.CONFIGS))
def test_decode_parity(name):
    cfg = hc.CONFIGS[name]
    left_out = total = 0
    for rows in hc.ROWS:
        for scale in hc.SCALES:
            anchor, reg = hc.case(name, rows, scale)
            ref, skip = hc.case_reference(name, rows, scale)
            got = gpu_decode(cfg, anchor, reg)
            what = "%s rows %d scale %g" % (name, rows, scale)
            if rows >= 1000:
                hc.check(got, ref, skip, what)
            else:                       # too few rows for a share: the tolerances alone, the share over the whole configuration below
                size, heading = hc.errors(got, ref, skip)
                print("%s: columns 0-5 at %.3f of the tolerance, heading error %.3e" % (what, size, heading))
                assert got.shape == ref.shape and size == size and size <= 1.0 and heading <= hc.TOL, (what, size, heading)
            left_out += int(skip.sum())
            total += rows
    assert left_out <= 0.01 * total, (name, left_out, total)


def test_decode_explicit_rows():
    cfg = hc.CONFIGS["rpn_hard"]
    per_bin = 2 * math.pi / 12
    reg = torch.zeros((6, 76))
    anchor = torch.tensor([[1.0, 0.5, 20.0]] * 6)
    # row 0: all-equal logits everywhere -> bin 0 on every axis: x = z = 0.25 - 3, heading 0
    # row 1: heading bin 0 with residual -1: -per_bin / 2 modulo 2 pi lands near 2 pi and must wrap back to -per_bin / 2
    reg[1, 61] = -1.0
    # row 2: heading bin 11 (largest logit) with residual +3: 11 per_bin + 1.5 per_bin passes 2 pi and must wrap to per_bin / 2
    reg[2, 49 + 11], reg[2, 61 + 11] = 2.0, 3.0
    # row 3: two equal maxima (bins 4 and 9) on x and on the heading: the first wins
    reg[3, 4], reg[3, 9], reg[3, 48 + 1 + 4], reg[3, 48 + 1 + 9] = 1.5, 1.5, 0.75, 0.75
    # row 4: a residual on the winning x bin, none used from the others
    reg[4, 7], reg[4, 24 + 7], reg[4, 24 + 6] = 1.0, 0.5, 9.0
    # row 5: sizes and the y offset
    reg[5, 48], reg[5, 73], reg[5, 74], reg[5, 75] = -0.25, 0.5, -0.5, 1.0
    for bottom in (False, True):
        got = gpu_decode(cfg, anchor, reg, y_to_bottom=bottom).double()
        ref = hc.reference64(cfg, anchor, reg, y_to_bottom=bottom)
        hc.check(got.float(), ref, torch.zeros(6, dtype=torch.bool), "explicit rows, y_to_bottom %s" % bottom)
        h = float(hc.ANCHOR_SIZE[0])
        lift = h / 2 if bottom else 0.0
        assert got[0, 0] == 1.0 + 0.25 - 3.0 and got[0, 2] == 20.0 + 0.25 - 3.0 and got[0, 6] == 0.0
        assert abs(float(got[0, 1]) - (0.5 + lift)) <= 1e-6
        assert abs(float(got[1, 6]) + per_bin / 2) <= 1e-5 and abs(float(got[2, 6]) - per_bin / 2) <= 1e-5
        assert got[3, 0] == 1.0 + 4 * 0.5 + 0.25 - 3.0 and abs(float(got[3, 6]) - 4 * per_bin) <= 1e-5
        assert got[4, 0] == 1.0 + 7 * 0.5 + 0.25 - 3.0 + 0.25
        assert abs(float(got[5, 3]) - 1.5 * h) <= 1e-6 and abs(float(got[5, 1]) - (0.25 + (1.5 * h / 2 if bottom else 0.0))) <= 1e-6
        assert abs(float(got[5, 4]) - 0.5 * float(hc.ANCHOR_SIZE[1])) <= 1e-6 and abs(float(got[5, 5]) - 2 * float(hc.ANCHOR_SIZE[2])) <= 1e-6


# ---- 2. order --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1023, 1024, 1025, 4097, 16383, 16384])
@pytest.mark.parametrize("b", [1, 3])
def test_score_order_is_the_stable_sort(b, n):
    from epnet_amd import rpn_handover
    for kind, scores in hc.score_kinds(b, n, seed=31 * n + b).items():
        got = rpn_handover.score_order(scores.to(DEV)).cpu()
        assert got.dtype == torch.int64 and torch.equal(got, hc.stable_order(scores)), (kind, b, n)


def test_score_order_refuses_more_than_16384():
    from epnet_amd import _lib, rpn_handover
    with pytest.raises(_lib.EpnetError, match="score_order.*16384"):
        rpn_handover.score_order(torch.zeros((1, 16385), device=DEV))
    with pytest.raises(_lib.EpnetError, match="rpn_handover.*16384"):
        rpn_handover.rpn_handover(torch.zeros((1, 16385, 1), device=DEV), torch.zeros((1, 16385, 76), device=DEV), torch.zeros((1, 16385, 3), device=DEV))


# ---- 3. the hand-over end to end -------------------------------------------------------------------------------------------------
def handover_cfg(distance_based=True, nms_type="normal"):
    from epnet_amd import proposal_layer
    cfg = proposal_layer.default_cfg()
    cfg.TEST.RPN_DISTANCE_BASED_PROPOSE = distance_based
    cfg.RPN.NMS_TYPE = nms_type
    return cfg


_REF = {}


def proposals_reference(n):
    """the float64 decoding of the end-to-end inputs, y at the bottom centre; computed once per n"""
    if n not in _REF:
        _, reg, xyz = hc.scene_inputs(n)
        _REF[n] = hc.reference64(hc.CONFIGS["rpn_soft"], xyz.view(-1, 3), reg.view(-1, 76), y_to_bottom=True).view(2, n, 7)
    return _REF[n]


@pytest.mark.parametrize("variant", ["distance_normal", "distance_rotate", "score_based"])
@pytest.mark.parametrize("mode", ["TRAIN", "TEST"])
@pytest.mark.parametrize("n", [2048, 16384])
def test_handover_end_to_end(n, mode, variant):
    from epnet_amd import iou3d_cuda, rpn_handover
    cfg = handover_cfg(variant != "score_based", "rotate" if variant == "distance_rotate" else "normal")
    scores_h, reg_h, xyz_h = hc.scene_inputs(n)
    scores, reg, xyz = scores_h.to(DEV), reg_h.to(DEV), xyz_h.to(DEV)
    out = rpn_handover.rpn_handover(scores.unsqueeze(2), reg, xyz, cfg=cfg, mode=mode)
    args = rpn_handover.handover_args(cfg, mode)
    post = args["post_nms_top_n"]
    assert out.rois.shape == (2, post, 7) and out.roi_scores_raw.shape == (2, post) and out.roi_count.dtype == torch.int32
    # the order
    assert torch.equal(out.order.cpu(), hc.stable_order(scores_h))
    # the decoded boxes
    hc.check(out.proposals.cpu().view(-1, 7), proposals_reference(n).view(-1, 7), torch.zeros(2 * n, dtype=torch.bool), "proposals n %d" % n)
    # the downstream kernels are unchanged: bit-equal to the existing op fed the call's own proposals and order
    rb, rs = torch.empty_like(out.rois), torch.empty_like(out.roi_scores_raw)
    rc = torch.empty_like(out.roi_count)
    iou3d_cuda.rpn_proposals_gpu(out.proposals, scores, out.order, args["distance_based"], args["pre_nms_top_n"], post, args["nms_thresh"],
                                 args["rotated"], rb, rs, rc)
    assert torch.equal(out.rois, rb) and torch.equal(out.roi_scores_raw, rs) and torch.equal(out.roi_count, rc)
    assert int(out.roi_count.min()) > 0 and int(out.roi_count.max()) <= post
    # mask and depth
    prob = torch.sigmoid(scores_h.double())
    clear = (prob - 0.3).abs() > 1e-6
    assert float((~clear).float().mean()) <= 0.001
    mask = out.seg_mask.cpu()
    assert torch.equal(mask[clear], (prob > 0.3).float()[clear]) and bool(((mask == 0) | (mask == 1)).all())
    assert bool(mask[prob > 0.31].all()) and not bool(mask[prob < 0.29].any())
    depth = xyz_h.double().norm(dim=2)
    assert bool(((out.pts_depth.cpu().double() - depth).abs() <= 1e-5 * depth).all())


def test_handover_mask_of_a_nan_score_is_zero_and_optional_outputs_may_be_absent():
    from epnet_amd import handover_cuda, rpn_handover
    scores_h, reg_h, xyz_h = hc.scene_inputs(2048)
    scores_h = scores_h.clone()
    scores_h[0, 5], scores_h[1, 7] = float("nan"), float("inf")
    scores, reg, xyz = scores_h.to(DEV), reg_h.to(DEV), xyz_h.to(DEV)
    cfg = handover_cfg()
    full = rpn_handover.rpn_handover(scores, reg, xyz, cfg=cfg, mode="TEST")
    assert float(full.seg_mask[0, 5]) == 0.0 and float(full.seg_mask[1, 7]) == 1.0 and int(full.order[0, 0]) == 5 and int(full.order[1, 0]) == 7
    rb, rs = torch.empty_like(full.rois), torch.empty_like(full.roi_scores_raw)
    handover_cuda.rpn_handover_gpu(scores, reg, xyz, ret_bbox3d=rb, ret_scores=rs, **rpn_handover.handover_args(cfg, "TEST"))
    # proposals and order in the workspace: the same bits (a NaN score may be a kept ROI's: compare the bit patterns)
    assert torch.equal(rb, full.rois) and torch.equal(rs.view(torch.int32), full.roi_scores_raw.view(torch.int32))


# ---- 4. capture ------------------------------------------------------------------------------------------------------------------
def test_handover_records_into_a_graph_and_never_synchronises():
    from epnet_amd import rpn_handover
    cfg = handover_cfg()
    scores_h, reg_h, xyz_h = hc.scene_inputs(2048)
    other_s, other_r, other_x = hc.scene_inputs(2048, seed=23, scale=3.0)
    scores, reg, xyz = scores_h.to(DEV), reg_h.to(DEV), xyz_h.to(DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        eager = rpn_handover.rpn_handover(scores, reg, xyz, cfg=cfg, mode="TRAIN")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = rpn_handover.rpn_handover(scores, reg, xyz, cfg=cfg, mode="TRAIN")       # a second run, on a side stream: the same bits
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, again))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = rpn_handover.rpn_handover(scores, reg, xyz, cfg=cfg, mode="TRAIN")
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, captured))
    scores.copy_(other_s.to(DEV)); reg.copy_(other_r.to(DEV)); xyz.copy_(other_x.to(DEV))   # new inputs in the captured buffers
    graph.replay()
    torch.cuda.synchronize()
    fresh = rpn_handover.rpn_handover(scores, reg, xyz, cfg=cfg, mode="TRAIN")
    assert all(torch.equal(a, b) for a, b in zip(fresh, captured))
    assert not torch.equal(fresh.rois, eager.rois)


# ---- 5. switches -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["TRAIN", "TEST"])
def test_proposal_layer_fused_head_is_the_handover(mode):
    from epnet_amd import proposal_layer, rpn_handover
    cfg = handover_cfg()
    scores_h, reg_h, xyz_h = hc.scene_inputs(2048)
    scores, reg, xyz = scores_h.to(DEV), reg_h.to(DEV), xyz_h.to(DEV)
    layer = proposal_layer.ProposalLayer(mode, cfg=cfg, fused_head=True).to(DEV)
    rois, roi_scores = layer(scores, reg, xyz)
    want = rpn_handover.rpn_handover(scores, reg, xyz, cfg=cfg, mode=mode)
    assert torch.equal(rois, want.rois) and torch.equal(roi_scores, want.roi_scores_raw)
    # the default layer takes the stock path and lands within the decode tolerance of the same proposals
    stock = proposal_layer.ProposalLayer(mode, cfg=cfg).to(DEV)
    assert stock.fused_head is False
    hc.check(stock.decode(reg, xyz).cpu().view(-1, 7), want.proposals.cpu().double().view(-1, 7), torch.zeros(2 * 2048, dtype=torch.bool),
             "stock decode against the fused proposals")


def test_detection_layer_fused_decode():
    from epnet_amd import detection_layer, iou3d_cuda
    b, m = 2, 100
    cfg = hc.CONFIGS["rcnn"]
    rois_h, reg_h = hc.anchors(b * m, 7, seed=5), hc.regression_values(b * m, 46, 1.0, seed=5)
    cls_h = torch.randn((b * m, 1), generator=torch.Generator().manual_seed(6))
    rois, reg, cls = rois_h.view(b, m, 7).to(DEV), reg_h.to(DEV), cls_h.to(DEV)
    layer = detection_layer.DetectionLayer(detection_layer.default_cfg(), fused_decode=True).to(DEV)
    pred, raw, norm, det_b, det_s, det_c = layer(rois, cls, reg)
    ref = hc.reference64(cfg, rois_h, reg_h)
    hc.check(pred.cpu().view(-1, 7), ref, torch.zeros(b * m, dtype=torch.bool), "DetectionLayer(fused_decode=True)")
    ob, os_, oc = torch.empty_like(det_b), torch.empty_like(det_s), torch.empty_like(det_c)
    iou3d_cuda.rcnn_detections_gpu(pred, raw, norm, 0.2, 0.1, ob, os_, oc)
    assert torch.equal(det_b, ob) and torch.equal(det_s, os_) and torch.equal(det_c, oc) and int(det_c.sum()) > 0
    stock = detection_layer.DetectionLayer(detection_layer.default_cfg()).to(DEV)
    assert stock.fused_decode is False
    hc.check(stock(rois, cls, reg)[0].cpu().view(-1, 7), ref, torch.zeros(b * m, dtype=torch.bool), "DetectionLayer()")

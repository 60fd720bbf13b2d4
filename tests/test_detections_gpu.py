"""Second-stage inference on the GPU (-m gpu): epnet_roipool3d_canonical and epnet_rcnn_detections BIT FOR BIT against the numpy
restatements of tests/detections_restate.py (the same arithmetic of record, so equality, as for the other index-valued ops),
the reference's fixtures through the GPU layers (bounds of tests/test_detections.py), and the point of the feature: ROI pooling +
an RCNN head + DetectionLayer captured into ONE HIP graph and replayed on new batches. The cases of the two sweeps come from
detections_restate.detection_cases() / pooling_cases(); tests/test_detections.py asserts what they cover.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import detections_restate as R
from test_detections import run_detection_layer, run_pool_rois

pytestmark = pytest.mark.gpu

NAN = float("nan")


def run_detections(boxes, raw, norm, score_thresh, nms_thresh, stream=None):
    """-> (det_boxes3d, det_scores, det_count) on the device, outputs pre-filled with NaN / -1: every element must be written"""
    from epnet_amd import iou3d_cuda
    b, m = raw.shape
    det_b = torch.full((b, m, 7), NAN, device="cuda")
    det_s = torch.full((b, m), NAN, device="cuda")
    det_c = torch.full((b,), -1, dtype=torch.int32, device="cuda")
    if stream is None:
        iou3d_cuda.rcnn_detections_gpu(boxes, raw, norm, score_thresh, nms_thresh, det_b, det_s, det_c)
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            iou3d_cuda.rcnn_detections_gpu(boxes, raw, norm, score_thresh, nms_thresh, det_b, det_s, det_c)
        torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    return det_b, det_s, det_c


@pytest.mark.parametrize("b,m,score_family,box_family,nms_thresh,seed", R.detection_cases(),
                         ids=lambda v: str(v))
def test_detections_equal_the_restatement(hiplib, oracle, b, m, score_family, box_family, nms_thresh, seed):
    boxes, raw, norm = R.detection_inputs(b, m, score_family, box_family, seed)
    boxes, raw = boxes.cuda(), raw.cuda()
    norm = torch.sigmoid(raw) if norm is None else norm.cuda()
    stream = torch.cuda.Stream() if seed % 5 == 0 else None                    # every fifth case on a stream of its own
    det_b, det_s, det_c = run_detections(boxes, raw, norm, 0.2, nms_thresh, stream)
    # the restatement is fed the very norm_scores tensor the kernel read
    want_b, want_s, want_c = R.rcnn_detections(boxes.cpu().numpy(), raw.cpu().numpy(), norm.cpu().numpy(), 0.2, nms_thresh)
    np.testing.assert_array_equal(det_c.cpu().numpy(), want_c)
    np.testing.assert_array_equal(det_s.cpu().numpy(), want_s)                 # (NaN == NaN here: a NaN raw score is a value)
    np.testing.assert_array_equal(det_b.cpu().numpy(), want_b)


def test_too_many_rois_are_refused_and_nothing_is_written(hiplib):
    b, m = 2, 4097
    boxes = torch.zeros((b, m, 7), device="cuda")
    raw = torch.zeros((b, m), device="cuda")
    from epnet_amd import iou3d_cuda
    det_b = torch.full((b, m, 7), NAN, device="cuda")
    det_s = torch.full((b, m), NAN, device="cuda")
    det_c = torch.full((b,), -1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="rcnn_detections"):
        iou3d_cuda.rcnn_detections_gpu(boxes, raw, torch.sigmoid(raw), 0.2, 0.1, det_b, det_s, det_c)
    torch.cuda.synchronize()
    assert bool(torch.isnan(det_b).all()) and bool(torch.isnan(det_s).all()) and bool((det_c == -1).all())


@pytest.mark.parametrize("b,n,m,s,c,seed", R.pooling_cases(), ids=lambda v: str(v))
def test_canonical_pooling_equals_the_restatement(hiplib, oracle, b, n, m, s, c, seed):
    from epnet_amd import roipool3d_cuda, roipool3d_utils
    xyz, rois, feat = R.pooling_inputs(b, n, m, c, seed)
    d_xyz, d_rois, d_feat = xyz.cuda(), rois.cuda(), feat.cuda()
    pooled = torch.full((b, m, s, 3 + c), NAN, device="cuda")
    flag = torch.full((b, m), -1, dtype=torch.int32, device="cuda")
    roipool3d_cuda.forward_canonical(d_xyz, d_rois, d_feat, 0.2, pooled, flag)
    torch.cuda.synchronize()
    want, want_flag = R.roipool3d_canonical(xyz.numpy(), rois.numpy(), feat.numpy(), 0.2, s)
    got = pooled.cpu().numpy()
    np.testing.assert_array_equal(flag.cpu().numpy(), want_flag)
    assert not np.isnan(got).any()
    np.testing.assert_array_equal(got[..., 3:], want[..., 3:])
    # +0.0 and -0.0 both count as right in the xyz columns (an empty box at a zero coordinate): compared as values
    assert (got[..., 0:3] == want[..., 0:3]).all(), float(np.abs(got[..., 0:3] - want[..., 0:3]).max())
    # the allocating front end gives the same; its feature columns and flags are those of the existing op on the enlarged boxes
    pooled2, flag2 = roipool3d_utils.roipool3d_canonical_gpu(d_xyz, d_feat, d_rois, 0.2, sampled_pt_num=s)
    plain, plain_flag = roipool3d_utils.roipool3d_gpu(d_xyz, d_feat, d_rois, 0.2, sampled_pt_num=s)
    torch.cuda.synchronize()
    assert torch.equal(pooled2, pooled) and torch.equal(flag2, flag)
    assert torch.equal(pooled[..., 3:], plain[..., 3:]) and torch.equal(flag, plain_flag)
    if n >= 1000:
        assert 0 < int(flag.sum()) < flag.numel()                             # empty and non-empty boxes both occur


def test_pool_rois_matches_the_reference_gpu(hiplib):
    run_pool_rois("cuda")


def test_detection_layer_matches_the_reference_gpu(hiplib):
    run_detection_layer("cuda")


class Head(torch.nn.Module):
    """a small stand-in for the RCNN stage: per-ROI mean over the sampled points, then two fixed elementwise heads"""

    def __init__(self, channels):
        super().__init__()
        g = torch.Generator().manual_seed(9)
        self.register_buffer("w_cls", torch.randn((channels,), generator=g))
        self.register_buffer("w_reg", torch.randn((46,), generator=g))

    def forward(self, pts_input):
        mean = pts_input.mean(dim=1)                                           # (B*M, 3 + C)
        cls = torch.tanh(mean * self.w_cls).sum(dim=1, keepdim=True) * 2.0     # (B*M, 1)
        reg = torch.tanh(mean[:, 0:1] * self.w_reg) * 0.6                      # (B*M, 46)
        return cls, reg


def test_second_stage_captures_into_one_hip_graph(hiplib, oracle):
    """pool_rois + a stand-in RCNN head + DetectionLayer in ONE torch.cuda.graph (capture fails on any synchronisation), single
    stream; replayed on three different batches written into the static tensors, each replay equal to the eager result on that
    batch and to the restatements"""
    from epnet_amd import detection_layer as dl, synth
    d = "cuda"
    b, n, m, c, s = 2, 4096, 24, 6, 64
    cfg = dl.default_cfg()
    cfg.RCNN.NUM_POINTS = s
    layer = dl.DetectionLayer(cfg).to(d)
    head = Head(3 + 2 + c).to(d)

    def batch(seed):
        g = torch.Generator().manual_seed(seed)
        xyz = synth.scenes("kitti", b, n, seed=seed)
        rois = torch.stack([synth.proposal_boxes(m, seed=seed + k, num_objects=4)[0] for k in range(b)]).float()
        pick = torch.randint(0, n, (b, m // 2), generator=g)
        rois[:, :m // 2, 0:3] = torch.gather(xyz, 1, pick.unsqueeze(-1).expand(b, m // 2, 3)) + torch.tensor([0.0, 0.8, 0.0])
        rois[:, -2:, 0] += 400.0                                               # two empty boxes per scene
        return [xyz, torch.randn((b, n, c), generator=g), rois.contiguous(), (torch.rand((b, n), generator=g) > 0.5).float(),
                torch.rand((b, n), generator=g) * 70]

    static = [t.to(d) for t in batch(50)]

    def second_stage():
        with torch.no_grad():
            xyz, feats, rois, mask, depth = static
            pts_input, empty = dl.pool_rois(xyz, feats, rois, mask, pts_depth=depth, cfg=cfg)
            cls, reg = head(pts_input)
            return (pts_input, empty) + tuple(layer(rois, cls, reg))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            second_stage()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graph_out = second_stage()
    counts = []
    for seed in (60, 70, 80):
        for dst, src in zip(static, batch(seed)):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in graph_out]
        eager = second_stage()
        torch.cuda.synchronize()
        for name, a, e in zip(("pts_input", "empty", "pred", "raw", "norm", "det_boxes", "det_scores", "det_count"), replayed, eager):
            assert torch.equal(a, e), (seed, name)
        xyz, feats, rois, mask, depth = (t.cpu() for t in static)
        feat_in = torch.cat([mask.unsqueeze(2), (depth / 70.0 - 0.5).unsqueeze(2), feats], dim=2)
        want_p, want_f = R.roipool3d_canonical(xyz.numpy(), rois.numpy(), feat_in.numpy(), 0.2, s)
        np.testing.assert_array_equal(replayed[1].cpu().numpy(), want_f)
        assert (replayed[0].cpu().numpy() == want_p.reshape(-1, s, want_p.shape[-1])).all()
        want_b, want_s, want_c = R.rcnn_detections(replayed[2].cpu().numpy(), replayed[3].cpu().numpy(), replayed[4].cpu().numpy(), 0.2, 0.1)
        np.testing.assert_array_equal(replayed[7].cpu().numpy(), want_c)
        np.testing.assert_array_equal(replayed[6].cpu().numpy(), want_s)
        np.testing.assert_array_equal(replayed[5].cpu().numpy(), want_b)
        counts.append(tuple(want_c.tolist()))
        assert 0 < int(replayed[1].sum()) < replayed[1].numel()
    assert len(set(counts)) > 1 or any(0 < k < m for c_ in counts for k in c_)   # the batches are not three times the same answer
    assert any(k > 0 for c_ in counts for k in c_)


def test_bench_step_times_the_whole_detector_from_one_graph(hiplib):
    """`bench_step.py --infer --two-stage` in a child process: the RPN-stage line as before, then the whole detector's"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench_step.py"), "--infer", "--two-stage", "--batch", "1", "--points", "4096",
                          "--steps", "3", "--warmup", "2"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 2 and lines[0]["metric"].startswith("RPN-stage") and lines[1]["metric"].startswith("two-stage")
    res = lines[1]
    assert res["graph_equals_eager"] is True and lines[0]["graph_equals_eager"] is True
    assert res["rois_per_scene"] == 100 and res["scenes"] == 1 and len(res["detections"]) == 1 and 0 <= res["detections"][0] <= 100
    assert res["ms_eager"] > 0 and res["ms_hip_graph"] > 0

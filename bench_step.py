#!/usr/bin/env python3
"""bench_step.py -- BASELINE.json configs 3 and 4: training steps of the model AROUND the hot path at the yaml's shapes
(tools/cfgs/LI_Fusion_with_attention_use_ce_loss.yaml) on synthetic KITTI-shaped scenes.

    python bench_step.py --image --rpn-only [--batch 2]       # config 3: two-stream RPN (point + image stream, LI-Fusion) fwd+bwd
    python bench_step.py --image [--gpus N]                   # config 4: the whole rcnn_online step, 62.7 MB of gradients
    python bench_step.py --image [--rpn-only] --amp bf16      # either under torch.autocast("cuda", torch.bfloat16)
    python bench_step.py                                      # the point stream alone (round-1 figure)
    python bench_step.py --infer [--two-stage]                # inference latency: the RPN stage [and the whole detector]
    python bench_step.py --infer --two-stage --proposals fused   # the same with the one-call RPN hand-over (epnet_rpn_handover)
    python bench_step.py --infer --two-stage --image [--image-head points]   # the two-stream detector; points: the image head at the taps only
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 bench_step.py --gpus N   # scene-parallel, RCCL

What is timed (forward + backward + optimiser step -- SGD unless --optimizer says otherwise --, `--batch` scenes per GPU):
  RPN backbone   4 SA-MSG levels 16384>4096>1024>256>64 + 4 FP levels (lib/net/pointnet2_msg.py:126-196, point stream) and
                 the cls / reg heads (lib/net/rpn.py:23-52)
  proposals      ProposalLayer (decode, distance-based NMS, 512 proposals per scene)
  targets        ProposalTargetLayer (IoU, ROI sampling + augmentation, roipool3d 64 x 512 x 133, canonical transform);
                 --targets fused: the sync-free RCNNTargetLayer (epnet_rcnn_sample_rois + epnet_roipool3d_train)
  RCNN stage     3 SA levels over 64 ROIs x 512 points per scene (128 > 32 > group-all) and two FC heads
                 (lib/net/rcnn_net.py:43-93, without its loss bookkeeping)
Every geometry op is this package's HIP path; every dense layer (shared MLPs, batch norm, image convolutions, attention
fusion, heads, optimiser) is stock PyTorch-ROCm, as the north_star has it. With --image the backbone is the two-stream one
(epnet_amd/rpn_backbone.py = lib/net/pointnet2_msg.py: four strided conv blocks over a (B,3,384,1280) image ~N(0,1),
Feature_Gather at the four pyramid levels and at full resolution, attention fusion); pixel coordinates ~U[0,1280)xU[0,384).
Losses are placeholders (sums of squares) by default -- the step exercises autograd through every op of the hot path at the
real shapes, it does not train anything; `--loss reference` ends the step in the real RPN + RCNN losses (epnet_amd.loss_utils, one
fused call each) on labels built from the synthetic boxes, `--loss composed` in the same losses composed from stock torch calls. `ops_share` = HIP-event time inside this package's operators / the step's GPU time,
from an instrumented pass after the timed one. With N > 1 ranks the model is wrapped
in DistributedDataParallel: the gradient all-reduce over RCCL / xGMI is the step's only collective (scenes are sharded
by rank). One JSON line from rank 0.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SA_NPOINTS = [4096, 1024, 256, 64]
SA_RADIUS = [[0.1, 0.5], [0.5, 1.0], [1.0, 2.0], [2.0, 4.0]]
SA_NSAMPLE = [[16, 32], [16, 32], [16, 32], [16, 32]]
SA_MLPS = [[[16, 16, 32], [32, 32, 64]], [[64, 64, 128], [64, 96, 128]], [[128, 196, 256], [128, 196, 256]],
           [[256, 256, 512], [256, 384, 512]]]
FP_MLPS = [[128, 128], [256, 256], [512, 512], [512, 512]]
RCNN_NPOINTS, RCNN_RADIUS, RCNN_NSAMPLE = [128, 32, None], [0.2, 0.4, 100], [64, 64, 64]
RCNN_MLPS = [[128, 128, 128], [128, 128, 256], [256, 256, 512]]
PROPOSALS_DEFAULT = "composed"       # --proposals: the stock decoding + sort in front of epnet_rpn_proposals


def build_model(scale=1, rpn_channels=76, image=False, sampler="hip", loss="placeholder", image_head="dense", image_head_rows16=False,
                sa_tail="stock"):
    """the two-stage model; scale > 1 divides the pyramid's point counts (small test configurations); image: the
    two-stream backbone with LI-Fusion (configs 3 / 4) instead of the point stream alone; loss: "placeholder" (sums of squares),
    "reference" (the real losses, fused: epnet_amd.loss_utils) or "composed" (the real losses as the reference composes them from
    stock torch calls, with its mask indexing and .item() reads: bench_ops.composed_rpn_loss / composed_rcnn_loss); the real
    losses read the RPN labels from model.rpn_labels = rpn_labels(xyz, gt_boxes3d); image_head: the two-stream backbone's
    "dense" (default) or "points" (inference: the image head under the bilinear taps only, rpn_backbone.Pointnet2MSG); sa_tail:
    "stock" (default) or "fused" (inference: every SA level of both stages ends in pointnet2_utils.sa_tail)"""
    import torch
    import torch.nn as nn
    from epnet_amd import pytorch_utils as pt_utils, rpn_backbone
    from epnet_amd.pointnet2_modules import PointnetSAModule
    PYRAMID = os.environ.get("EPNET_SA_PYRAMID", "1") != "0"

    class RCNN(nn.Module):       # lib/net/rcnn_net.py:17-93 (xyz up-layer, merge, SA stack, heads), losses left out
        def __init__(self):
            super().__init__()
            self.xyz_up = pt_utils.SharedMLP([5, 128, 128], bn=False)          # xyz + mask + depth (:22-27)
            self.merge_down = pt_utils.SharedMLP([256, 128], bn=False)
            self.SA_modules = nn.ModuleList()
            cin = 128
            for k in range(len(RCNN_NPOINTS)):
                self.SA_modules.append(PointnetSAModule(npoint=RCNN_NPOINTS[k], radius=RCNN_RADIUS[k], nsample=RCNN_NSAMPLE[k],
                                                        mlp=[cin] + RCNN_MLPS[k], use_xyz=True, bn=False,
                                                        fused_tail=sa_tail == "fused"))
                cin = RCNN_MLPS[k][-1]
            self.cls = nn.Sequential(pt_utils.Conv1d(512, 512), pt_utils.Conv1d(512, 512), pt_utils.Conv1d(512, 1, activation=None))
            self.reg = nn.Sequential(pt_utils.Conv1d(512, 512), pt_utils.Conv1d(512, 512), pt_utils.Conv1d(512, 46, activation=None))

        def forward(self, pts, feats):
            """pts (R,512,3) canonical, feats (R,512,130) = [mask, depth, 128 rpn features] (:96-113)"""
            head = torch.cat((pts, feats[..., 0:2]), dim=2).transpose(1, 2).unsqueeze(3)
            merged = torch.cat((self.xyz_up(head), feats[..., 2:].transpose(1, 2).unsqueeze(3)), dim=1)
            f = self.merge_down(merged).squeeze(3)
            xyz = pts.contiguous()
            for sa in self.SA_modules:
                xyz, f, _ = sa(xyz, f.contiguous())
            return self.cls(f), self.reg(f)

    class TwoStage(nn.Module):
        def __init__(self):
            super().__init__()
            # lib/net/pointnet2_msg.py:126-259 (rpn.py:19: input_channels = 0, the yaml has USE_INTENSITY False)
            self.backbone = rpn_backbone.Pointnet2MSG(input_channels=0, config=rpn_backbone.BackboneConfig(li_fusion=image),
                                                      sampler=sampler, scale=scale, pyramid=PYRAMID, image_head=image_head,
                                                      image_head_rows16=image_head_rows16, sa_tail=sa_tail)
            self.two_stream = image
            self.rpn_cls = nn.Sequential(pt_utils.Conv1d(128, 128, bn=True), pt_utils.Conv1d(128, 1, activation=None))
            self.rpn_reg = nn.Sequential(pt_utils.Conv1d(128, 128, bn=True), pt_utils.Conv1d(128, rpn_channels, activation=None))
            self.rcnn = RCNN()
            self.layers = None   # (ProposalLayer, ProposalTargetLayer), set by the caller
            self.loss_mode = loss
            self.rpn_labels = None   # (cls_label (B,N), reg_label (B,N,7)) for the real losses, set by the caller

        def forward(self, xyz, gt_boxes3d, mark=None, image=None, xy=None, rpn_only=False):
            """one forward pass + placeholder loss (the whole step lives in forward so that DistributedDataParallel sees
            it); returns (loss, dict of outputs). image (B,3,H,W) / xy (B,N,2) pixel coordinates (normalised in place, as
            the reference does) for the two-stream backbone"""
            proposal_layer, target_layer = self.layers
            mark = mark if mark is not None else (lambda name: None)
            _, feats = self.backbone(xyz, image, xy) if self.two_stream else self.backbone(xyz)   # (B,128,N)
            rpn_cls = self.rpn_cls(feats).transpose(1, 2).contiguous()           # (B,N,1)
            rpn_reg = self.rpn_reg(feats).transpose(1, 2).contiguous()           # (B,N,76)
            mark("rpn")
            real = self.loss_mode != "placeholder"
            if real:                                                             # lib/net/train_functions.py:51-67
                if self.loss_mode == "reference":
                    from epnet_amd.loss_utils import rpn_loss, rcnn_loss
                else:
                    from bench_ops import composed_rpn_loss as rpn_loss, composed_rcnn_loss as rcnn_loss
                loss_rpn = rpn_loss(rpn_cls, rpn_reg, self.rpn_labels[0], self.rpn_labels[1])
            if rpn_only:                                                         # config 3: backbone + heads
                if real:
                    return loss_rpn.loss, {"rpn_cls": rpn_cls, "rpn_reg": rpn_reg, "rpn_loss": loss_rpn}
                return rpn_cls.pow(2).mean() + rpn_reg.pow(2).mean(), {"rpn_cls": rpn_cls, "rpn_reg": rpn_reg}
            with torch.no_grad():                                                # lib/net/point_rcnn.py:33-47
                scores = rpn_cls[:, :, 0].detach()
                rois, _ = proposal_layer(scores, rpn_reg.detach(), xyz)
                mark("proposals")
                seg_mask = (torch.sigmoid(scores) > 0.3).float()
                depth = torch.norm(xyz, p=2, dim=2)
                target = target_layer({"roi_boxes3d": rois, "gt_boxes3d": gt_boxes3d, "rpn_xyz": xyz,
                                       "rpn_features": feats.detach().permute(0, 2, 1).contiguous(), "seg_mask": seg_mask,
                                       "pts_depth": depth})
                mark("targets")
            rcnn_cls, rcnn_reg = self.rcnn(target["sampled_pts"], target["pts_feature"])
            mark("rcnn")
            if real:                                                             # lib/net/train_functions.py:69-88
                loss_rcnn = rcnn_loss(dict(target, rcnn_cls=rcnn_cls.view(rcnn_cls.shape[0], -1), rcnn_reg=rcnn_reg.view(rcnn_reg.shape[0], -1)))
                mark("losses")
                return loss_rpn.loss + loss_rcnn.loss, {"rois": rois, "target": target, "rcnn_cls": rcnn_cls, "rcnn_reg": rcnn_reg,
                                                        "rpn_cls": rpn_cls, "rpn_reg": rpn_reg, "rpn_loss": loss_rpn, "rcnn_loss": loss_rcnn}
            loss = rpn_cls.pow(2).mean() + rpn_reg.pow(2).mean() + rcnn_cls.pow(2).mean() + rcnn_reg.pow(2).mean()
            return loss, {"rois": rois, "target": target, "rcnn_cls": rcnn_cls, "rcnn_reg": rcnn_reg}

    return TwoStage()


def run_step(model, layers, xyz, gt_boxes3d, timer=None, image=None, xy=None, rpn_only=False):
    """one forward pass through `model` (plain or DistributedDataParallel-wrapped)"""
    (model.module if hasattr(model, "module") else model).layers = layers
    return model(xyz, gt_boxes3d, timer, image, None if xy is None else xy.clone(), rpn_only)


def rpn_labels(xyz, gt_boxes3d, inside=0.05, ignore=0.2):
    """per-point RPN labels as the reference's loader makes them on the host (lib/datasets/kitti_rcnn_dataset.py,
    generate_rpn_training_labels), here from the synthetic scenes' own boxes, on the device and outside every timed region:
    cls_label (B,N) 1 for a point in a ground-truth box, -1 in the box enlarged by `ignore` but not in it, else 0; reg_label
    (B,N,7) [centre - point, h, w, l, ry] for the labelled points, zero elsewhere. The synthetic object points lie ON the
    faces of their boxes, so a box counts as enlarged by `inside` already. xyz (B,N,3), gt_boxes3d (B,G,7) zero-padded"""
    import torch
    centre = gt_boxes3d[:, None, :, 0:3].clone()
    centre[..., 1] -= gt_boxes3d[:, None, :, 3] / 2
    d = xyz[:, :, None, :] - centre                                             # (B,N,G,3)
    ry = gt_boxes3d[:, None, :, 6]
    lx = d[..., 0] * torch.cos(ry) - d[..., 2] * torch.sin(ry)
    lz = d[..., 0] * torch.sin(ry) + d[..., 2] * torch.cos(ry)
    h, w, l = (gt_boxes3d[:, None, :, k] for k in (3, 4, 5))
    real = (h > 0)

    def within(extra):
        return real & (lx.abs() <= l / 2 + extra) & (lz.abs() <= w / 2 + extra) & (d[..., 1].abs() <= h / 2 + extra)
    fg_any, which = within(inside).int().max(dim=2)
    fg_any = fg_any > 0
    cls_label = torch.where(fg_any, 1, torch.where(within(ignore).any(dim=2), -1, 0)).long()
    pick = which[:, :, None, None].expand(-1, -1, 1, 3)
    reg = torch.cat([-torch.gather(d, 2, pick)[:, :, 0], torch.gather(gt_boxes3d[:, None].expand(-1, xyz.shape[1], -1, -1), 2,
                                                                        which[:, :, None, None].expand(-1, -1, 1, 7))[:, :, 0, 3:7]], dim=2)
    return cls_label.contiguous(), (reg * fg_any[:, :, None]).contiguous()


def synthetic_batch(batch, points, seed, device):
    import torch
    from epnet_amd import synth
    xyz = synth.scenes("kitti", batch, points, seed=seed).to(device)
    gts = torch.zeros((batch, 20, 7))
    for i in range(batch):
        gts[i, :12] = synth.object_boxes(12, seed + i)
    return xyz, gts.to(device)


def infer(args, model, proposal_layer, xyz, image=None, xy=None):
    """inference latency, eager launches against one HIP-graph replay: the RPN stage and, with --two-stage, the whole detector;
    image / xy: the two-stream backbone's inputs (--image)"""
    import contextlib
    import torch
    model.eval()
    two_stream = {"image": True, "image_head": args.image_head} if image is not None else {}
    two_stream["sa_tail"] = args.sa_tail
    # --amp: backbone, heads and the RCNN stage under torch.autocast; the proposal / detection layers and pool_rois make their own
    # float32 region. No loss, so float16 needs no scale here
    amp = (lambda: contextlib.nullcontext()) if args.amp == "off" else (
        lambda: torch.autocast("cuda", torch.float16 if args.amp == "fp16" else torch.bfloat16))
    dtype = "f32" if args.amp == "off" else "%s autocast (parameters f32)" % args.amp
    if image is not None:
        # the image stream's convolutions: at 2 scenes the dense library's default choice sums in an order that changes from run to
        # run, so two EAGER runs of the RPN stage already differ (graph_equals_eager false with either head, measured); as for the
        # RCNN heads below, its deterministic algorithms are asked for, for the comparison to mean something
        torch.backends.cudnn.deterministic = True
        two_stream["dense_layers_deterministic"] = True

    def rpn():
        # the backbone normalises xy in place: a fresh copy per call
        _, feats = model.backbone(xyz, image, xy.clone()) if image is not None else model.backbone(xyz)
        cls = model.rpn_cls(feats).transpose(1, 2).contiguous()
        reg = model.rpn_reg(feats).transpose(1, 2).contiguous()
        return feats, cls[:, :, 0].contiguous(), reg

    def stage():
        with torch.no_grad(), amp():
            _, scores, reg = rpn()
            return proposal_layer(scores, reg, xyz)

    def timed(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3

    def eager_and_graph(fn):
        """-> ms eager, ms per replay, graph == eager, the graph's output tensors"""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(max(3, args.warmup)):
                eager_out = fn()
        torch.cuda.current_stream().wait_stream(side)
        ms_eager = timed(fn, args.steps)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            graph_out = fn()
        graph.replay()
        torch.cuda.synchronize()
        same = all(torch.equal(a, b) for a, b in zip(eager_out, graph_out))
        return ms_eager, timed(graph.replay, args.steps), same, graph_out

    ms_eager, ms_graph, same, _ = eager_and_graph(stage)
    print(json.dumps({"metric": "RPN-stage inference latency (backbone + heads + proposal layer, eval mode)", "scenes": args.batch,
                      "points_per_scene": args.points, "ms_eager": round(ms_eager, 3), "ms_hip_graph": round(ms_graph, 3),
                      "graph_equals_eager": bool(same), "proposals": args.proposals, "dtype": dtype, "data": "synthetic",
                      **two_stream}), flush=True)
    if not args.two_stage:
        return
    # the whole detector (lib/net/point_rcnn.py:33-47 + the eval branch of lib/net/rcnn_net.py:138-164 + tools/eval_rcnn.py:555-583,
    # 663-683): the TEST proposal layer (100 ROIs per scene), canonical ROI pooling, the RCNN stage, decoding + threshold + NMS
    from epnet_amd import detection_layer as dl, proposal_layer as pl
    fused = args.proposals == "fused"
    test_layer = pl.ProposalLayer("TEST", cfg=proposal_layer.cfg).to(xyz.device)
    det_layer = dl.DetectionLayer(dl.default_cfg(), fused_decode=fused).to(xyz.device)
    # the RCNN heads are length-1 convolutions over 100 ROIs per scene: the dense library's default choice for that shape
    # accumulates in an order that changes from run to run (last bits), so two EAGER runs already differ; its deterministic
    # algorithms are asked for here, for the graph == eager comparison to mean something
    torch.backends.cudnn.deterministic = True

    def detector():
        with torch.no_grad(), amp():
            feats, scores, reg = rpn()
            if fused:                                                            # point_rcnn.py:44-52 in one call
                from epnet_amd import rpn_handover
                rois, _, seg_mask, depth = rpn_handover.rpn_handover(scores, reg, xyz, cfg=test_layer.cfg, mode="TEST")[:4]
            else:
                rois, _ = test_layer(scores, reg, xyz)
                seg_mask = (torch.sigmoid(scores) > 0.3).float()
                depth = torch.norm(xyz, p=2, dim=2)
            pts_input, _ = dl.pool_rois(xyz, feats.permute(0, 2, 1).contiguous(), rois, seg_mask, pts_depth=depth, cfg=det_layer.cfg)
            rcnn_cls, rcnn_reg = model.rcnn(pts_input[..., 0:3], pts_input[..., 3:])
            rcnn_cls = rcnn_cls.transpose(1, 2).contiguous().squeeze(dim=1)      # (B*M, 1), lib/net/rcnn_net.py:190
            rcnn_reg = rcnn_reg.transpose(1, 2).contiguous().squeeze(dim=1)      # (B*M, 46)
            return det_layer(rois, rcnn_cls, rcnn_reg)

    ms_eager, ms_graph, same, out = eager_and_graph(detector)
    counts = out[5].tolist()                                                     # of the last replay, read after the timed loop
    print(json.dumps({"metric": "two-stage inference latency (RPN stage + ROI pooling + RCNN stage + detections, eval mode)",
                      "scenes": args.batch, "points_per_scene": args.points, "rois_per_scene": int(out[0].shape[1]),
                      "ms_eager": round(ms_eager, 3), "ms_hip_graph": round(ms_graph, 3), "graph_equals_eager": bool(same),
                      "detections": counts, "dense_layers_deterministic": True, "proposals": args.proposals, "dtype": dtype,
                      "data": "synthetic", **two_stream}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2, help="scenes per GPU (16 over 8 GPUs in config 4)")
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--infer", action="store_true",
                    help="instead of the training step: inference latency of the RPN stage (backbone, heads, proposal layer) in "
                         "eval mode, eagerly and replayed from a HIP graph (nothing in the stage synchronises with the host)")
    ap.add_argument("--two-stage", action="store_true",
                    help="with --infer: after the RPN-stage line, the whole detector -- TEST proposal layer (100 ROIs per scene), "
                         "canonical ROI pooling, RCNN stage, decoding + score threshold + rotated NMS -- eagerly and as ONE HIP graph")
    ap.add_argument("--image", action="store_true",
                    help="two-stream backbone: (B,3,384,1280) image ~N(0,1), pixel coordinates ~U[0,1280)xU[0,384), LI-Fusion with "
                         "image attention (BASELINE configs 3 and 4; 15.7 M parameters = 62.7 MB of gradients)")
    ap.add_argument("--image-head", default="dense", choices=["dense", "points"],
                    help="with --image: the end of the image stream -- the full-resolution fusion map sampled at the points (default) "
                         "or, in inference, the head evaluated under the bilinear taps only (li_fusion.image_head_at_points); the "
                         "training steps run the dense lines either way")
    ap.add_argument("--sa-tail", default="stock", choices=["stock", "fused"],
                    help="with --infer: the end of every SA level's shared MLP -- the stock conv / batch norm / ReLU / max-pool lines, "
                         "or the last convolution with its folded batch norm, the ReLU and the pool from one kernel "
                         "(pointnet2_utils.sa_tail, float32 only); the JSON lines report which one ran")
    ap.add_argument("--rpn-only", action="store_true", help="config 3: forward + backward of backbone + RPN heads only")
    ap.add_argument("--sampler", default="hip", choices=["hip", "stock"],
                    help="point-to-pixel sampler: this package's Feature_Gather or stock torch.gather + grid_sample")
    ap.add_argument("--loss", default="placeholder", choices=["placeholder", "reference", "composed"],
                    help="the step's loss: sums of squares (default), the real RPN + RCNN losses fused (epnet_amd.loss_utils), or the "
                         "real losses composed from stock torch calls as the reference does, mask indexing and .item() reads included; "
                         "the RPN labels are built on the device outside the timed region")
    ap.add_argument("--targets", default="host", choices=["host", "fused"],
                    help="the RCNN target layer: the draw-for-draw restatement of the reference's host random streams (two read-backs "
                         "per step, default) or the sync-free epnet_amd.rcnn_target_layer.RCNNTargetLayer (device tables, two calls)")
    ap.add_argument("--optimizer", default="sgd", choices=["sgd", "composed", "fused"],
                    help="how the step ends: torch.optim.SGD with a fixed learning rate (default), the reference's adam_onecycle step "
                         "composed from stock torch calls (clip_grad_norm_, host one-cycle schedule, per-parameter decay, Adam: "
                         "bench_ops.ComposedAdamOneCycle), or epnet_amd.optim.FusedAdamOneCycle (three launches, no host scalar)")
    ap.add_argument("--proposals", default=PROPOSALS_DEFAULT, choices=["composed", "fused"],
                    help="between the RPN heads and the proposal kernels: the stock decoding, sort, mask and depth (default) or the "
                         "one-call hand-over (epnet_amd.rpn_handover: one decode launch, one order launch); the second stage's "
                         "decoding follows (DetectionLayer(fused_decode=...))")
    ap.add_argument("--inputs", default="arrays", choices=["arrays", "raw"],
                    help="where the step starts: from the (B,N,3) point arrays a loader would hand over (default), or, with --rpn-only, "
                         "from raw scans (synth.lidar_scan, 122 880 points each) through scan_layer.prepare_scans and "
                         "rpn_target_layer.augment_and_label on the device, fresh draws every step, no host synchronisation")
    ap.add_argument("--gt-aug", action="store_true",
                    help="with --inputs raw: GT-database augmentation of the point-only loader between the validity filter and the "
                         "sampling (gt_aug_layer.prepare_scans_gt_aug on a synthetic database of 200 objects, fresh draws every step, "
                         "no host synchronisation); a pasted object has no pixels, so the flag is refused together with --image")
    ap.add_argument("--amp", default="off", choices=["off", "bf16", "fp16"],
                    help="bf16: forward under torch.autocast('cuda', torch.bfloat16) -- dense layers and this package's SA / FP operators on "
                         "bfloat16 rows, parameters and their gradients float32. fp16: the same under torch.float16 with dynamic loss "
                         "scaling inside the optimiser step (--optimizer fused only: FusedAdamOneCycle(loss_scale='dynamic'), the loss "
                         "goes through scale_loss). With --infer: backbone, heads and RCNN stage under that autocast (no loss scale "
                         "involved), --image-head points on the 16-bit MFMA head (image_head_rows16=True)")
    ap.add_argument("--loss-scale", default="off", choices=["off", "guard"],
                    help="guard: with --optimizer fused under --amp off / bf16, a static loss scale of 1.0 -- the step is skipped on the "
                         "device when a gradient is not finite (--amp fp16 brings its own dynamic scale)")
    ap.add_argument("--gpus", type=int, default=1,
                    help="ranks (one per GPU); without a torch.distributed.run environment the ranks are started as child processes")
    ap.add_argument("--launch-check", action="store_true", help="rehearse the N-rank launch only (see bench.py)")
    ap.add_argument("--rehearsal", action="store_true",
                    help="allow EPNET_BENCH_DEVICE / EPNET_BENCH_BACKEND (all ranks on one device, gloo): see bench.py")
    args = ap.parse_args()
    if args.two_stage and not args.infer:
        ap.error("--two-stage belongs to --infer")
    if args.gt_aug and (args.image or args.inputs != "raw"):
        ap.error("--gt-aug belongs to the point-only loader: --rpn-only --inputs raw, without --image")
    if args.inputs == "raw" and (not args.rpn_only or args.image or args.infer):
        ap.error("--inputs raw starts the point-stream RPN step (--rpn-only, without --image) from raw scans")
    if ((args.amp == "fp16" and not args.infer) or args.loss_scale == "guard") and (args.optimizer != "fused" or args.infer):
        ap.error("--amp fp16 and --loss-scale guard are the fused optimiser's loss scaling: pass --optimizer fused")
    if args.amp == "fp16" and args.loss_scale == "guard":
        ap.error("--amp fp16 scales dynamically; --loss-scale guard belongs to --amp off / bf16")
    if args.sa_tail != "stock" and not args.infer:
        ap.error("--sa-tail fused is inference only: pass --infer")
    if args.image_head != "dense" and not args.image:
        ap.error("--image-head belongs to the two-stream backbone: pass --image")
    from epnet_amd import scene_shard
    code = scene_shard.launch_or_continue(args.gpus, os.path.abspath(__file__), sys.argv[1:])
    if code is not None:
        sys.exit(code)
    scene_shard.assert_world(args.gpus)
    if args.launch_check:
        import bench
        return bench.launch_check(args)
    if not args.rehearsal and ("EPNET_BENCH_DEVICE" in os.environ or "EPNET_BENCH_BACKEND" in os.environ):
        raise SystemExit("EPNET_BENCH_DEVICE / EPNET_BENCH_BACKEND rehearse the N-rank path on one device: pass --rehearsal")
    import numpy as np
    import torch
    import torch.distributed as dist
    from epnet_amd import proposal_layer as pl, proposal_target_layer as ptl

    world, rank, local = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    # EPNET_BENCH_DEVICE / EPNET_BENCH_BACKEND rehearse the N > 1 path on a one-GPU box (all ranks on one device, gloo)
    local = int(os.environ.get("EPNET_BENCH_DEVICE", local))
    backend = os.environ.get("EPNET_BENCH_BACKEND", "nccl")
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)
    torch.manual_seed(1 + rank)
    np.random.seed(1 + rank)
    model = build_model(image=args.image, sampler=args.sampler, loss=args.loss, image_head=args.image_head,
                        image_head_rows16=args.image_head == "points" and args.amp != "off", sa_tail=args.sa_tail).to(device)
    if world > 1:
        model = torch.nn.parallel.DistributedDataParallel(model, device_ids=[local], find_unused_parameters=False)
    total_steps = args.warmup + args.steps + 8                         # the instrumented pass takes up to 5 more
    if args.optimizer == "fused":
        from epnet_amd import optim
        loss_scale = "dynamic" if args.amp == "fp16" else 1.0 if args.loss_scale == "guard" else None
        opt = optim.FusedAdamOneCycle(model.module if hasattr(model, "module") else model, total_steps, loss_scale=loss_scale)
        zero_grad = opt.zero_grad                                      # nothing to do: the step leaves the gradients zero, in place
    elif args.optimizer == "composed":
        from bench_ops import ComposedAdamOneCycle
        opt = ComposedAdamOneCycle(model.parameters(), total_steps)
        zero_grad = opt.zero_grad
    else:
        opt = torch.optim.SGD(model.parameters(), lr=1e-4, momentum=0.9)
        zero_grad = lambda: opt.zero_grad(set_to_none=True)            # noqa: E731
    if args.targets == "fused":
        from epnet_amd import rcnn_target_layer as rtl
        layers = (pl.ProposalLayer("TRAIN", fused_head=args.proposals == "fused").to(device), rtl.RCNNTargetLayer())
    else:
        layers = (pl.ProposalLayer("TRAIN", fused_head=args.proposals == "fused").to(device), ptl.ProposalTargetLayer())
    xyz, gts = synthetic_batch(args.batch, args.points, 100 + 1000 * rank, device)   # every rank its own scenes
    image = xy = None
    if args.image:
        g = torch.Generator().manual_seed(200 + rank)
        image = torch.randn((args.batch, 3, 384, 1280), generator=g).to(device)                      # lib/datasets/kitti_dataset.py:54
        xy = (torch.rand((args.batch, args.points, 2), generator=g) * torch.tensor([1280.0, 384.0])).to(device)

    if args.infer:
        return infer(args, model.module if hasattr(model, "module") else model, layers[0], xyz, image, xy)
    raw = None
    if args.inputs == "raw":
        from epnet_amd import rpn_target_layer, scan_layer, synth
        scans, num_raw = scan_layer.collate_scans([synth.lidar_scan(122880 - 1500 * k, seed=300 + 1000 * rank + k) for k in range(args.batch)])
        cal = [synth.calibration(1000 * rank + k) for k in range(args.batch)]
        raw = {"scans": scans.to(device), "num_raw": num_raw.to(device), "cal": [torch.stack([c[j] for c in cal]).to(device) for j in range(4)],
               "alpha": torch.zeros(gts.shape[:2], device=device)}
        if args.gt_aug:
            from epnet_amd import gt_aug_layer
            raw.update(db=gt_aug_layer.GTDatabase.from_list(synth.gt_database(200, seed=500 + rank), device), cfg=gt_aug_layer.default_cfg(),
                       num_boxes=torch.full((args.batch,), 12, dtype=torch.int32, device=device),      # synthetic_batch fills 12 rows
                       plane=torch.tensor([[0.0, -1.0, 0.0, 1.65]] * args.batch, dtype=torch.float64, device=device))

    def step_inputs():
        """--inputs raw: this step's points from the raw scans, sampled, shuffled and augmented on the device"""
        if raw is None:
            return xyz, gts
        step_gts, step_alpha = gts, raw["alpha"]
        if args.gt_aug:
            tables = gt_aug_layer.draw_tables(args.batch, raw["scans"].shape[1], raw["db"], 8192, args.points, raw["cfg"], None, device)
            got = gt_aug_layer.prepare_scans_gt_aug(raw["scans"], raw["num_raw"], *raw["cal"], tables, raw["db"], gts, raw["num_boxes"], gts,
                                                    raw["alpha"], raw["num_boxes"], raw["plane"], npoints=args.points, extra_rows=8192,
                                                    cfg=raw["cfg"])
            step_gts, step_alpha = got["gt_boxes3d"], got["gt_alpha"]
        else:
            tables = scan_layer.draw_scan_tables(args.batch, raw["scans"].shape[1], args.points, None, device)
            got = scan_layer.prepare_scans(raw["scans"], raw["num_raw"], *raw["cal"], tables, npoints=args.points)
        aug = rpn_target_layer.draw_augmentation(args.batch, device=device)
        pts, boxes, cls_label, reg_label = rpn_target_layer.augment_and_label(got["pts_rect"], step_gts, step_alpha, aug)
        if args.loss != "placeholder":                     # the labels of THIS step's points
            (model.module if hasattr(model, "module") else model).rpn_labels = (cls_label, reg_label)
        return pts, boxes
    if args.loss != "placeholder":
        (model.module if hasattr(model, "module") else model).rpn_labels = rpn_labels(xyz, gts)

    phases = {}
    last_out = {}
    scaled = args.optimizer == "fused" and opt.scale is not None

    def one(timed):
        events = [("start", torch.cuda.Event(enable_timing=True))]
        events[0][1].record()

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            events.append((name, e))
        zero_grad()
        step_xyz, step_gts = step_inputs()
        if raw is not None and timed:
            mark("inputs")
        with torch.autocast("cuda", torch.float16 if args.amp == "fp16" else torch.bfloat16, enabled=args.amp != "off"):
            loss, out = run_step(model, layers, step_xyz, step_gts, mark if timed else None, image, xy, args.rpn_only)
        if timed:                                              # the line carries the terms of the last TIMED step
            last_out.update({k: v for k, v in out.items() if k in ("rpn_loss", "rcnn_loss")})
        (opt.scale_loss(loss) if scaled else loss).backward()
        mark("backward")
        opt.step()
        mark("optimizer")
        if timed:
            torch.cuda.synchronize()
            for (_, a), (name, b) in zip(events[:-1], events[1:]):
                phases[name] = phases.get(name, 0.0) + a.elapsed_time(b)
        return float(loss.detach()) if timed else None

    t_w = time.perf_counter()
    for k in range(args.warmup):
        one(False)
        if k == 0 and rank == 0:
            torch.cuda.synchronize()
            print("first step (kernel selection of the dense layers included): %.1f s" % (time.perf_counter() - t_w), file=sys.stderr, flush=True)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    last, per_step = None, []
    for _ in range(args.steps):
        t_step = time.perf_counter()
        last = one(True)
        per_step.append(time.perf_counter() - t_step)      # one(True) ends with a device synchronisation
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    elapsed_own = elapsed
    if world > 1:
        t = torch.tensor([elapsed], device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t)
    per_rank = scene_shard.gather_over_ranks({"ms_per_step": round(elapsed_own / args.steps * 1e3, 3),
                                              "device": scene_shard.device_identity(device)})
    # the gradient exchange on its own: one all-reduce of a buffer as large as all gradients (DDP sends the same bytes in buckets,
    # overlapped with backward -- this is the un-overlapped cost it hides)
    allreduce = None
    if world > 1:
        n_grad = sum(p.numel() for p in model.parameters() if p.requires_grad)
        flat = torch.zeros((n_grad,), dtype=torch.float32, device=device)
        for _ in range(2):
            dist.all_reduce(flat)
        a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a0.record()
        for _ in range(5):
            dist.all_reduce(flat)
        a1.record()
        torch.cuda.synchronize()
        ar_ms = a0.elapsed_time(a1) / 5
        allreduce = {"bytes": n_grad * 4, "ms_alone": round(ar_ms, 3), "backend": dist.get_backend(),
                     "bus_GBps": round(2 * (world - 1) / world * n_grad * 4 / (ar_ms * 1e-3) / 1e9, 2)}
        del flat
    # ---- share of the step spent inside this package's operators: an instrumented pass with a HIP event pair around every
    # call into the three extension stand-ins (on the stream the call launches on), against the GPU time of the same steps
    ops_share = None
    import contextlib
    import bench
    from epnet_amd import iou3d_cuda, pointnet2_cuda, roipool3d_cuda
    iou_names = [n for n in ("boxes_overlap_bev_gpu", "boxes_iou_bev_gpu", "boxes_iou3d_fused_gpu", "boxes_iou3d_pairs_gpu",
                             "aug_roi_by_noise_gpu", "rpn_proposals_gpu", "nms_device", "nms_normal_device", "rcnn_sample_rois_gpu")]
    timers = ([bench.OpTimer(torch, pointnet2_cuda), bench.OpTimer(torch, iou3d_cuda, iou_names),
               bench.OpTimer(torch, roipool3d_cuda, ["forward", "forward_train"])] if rank == 0 else [])
    reps = max(2, min(5, args.steps))
    with contextlib.ExitStack() as stack:       # (every rank takes the steps: the gradient all-reduce needs all of them)
        for t in timers:
            stack.enter_context(t)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            one(False)
        e1.record()
        torch.cuda.synchronize()
    if rank == 0:
        per_op = {}
        for t in timers:
            for name, _head, a, b_ in t.records:
                per_op[name] = per_op.get(name, 0.0) + a.elapsed_time(b_) / reps
        ops_ms = sum(per_op.values())
        step_gpu_ms = e0.elapsed_time(e1) / reps
        ops_share = {"ops_ms_per_step": round(ops_ms, 3), "instrumented_step_ms": round(step_gpu_ms, 3),
                     "share": round(ops_ms / step_gpu_ms, 4),
                     "per_op_ms": {k: round(v, 3) for k, v in sorted(per_op.items(), key=lambda kv: -kv[1])},
                     "note": "sum of HIP-event durations of every call into the pointnet2 / iou3d / roipool3d stand-ins "
                             "(calls on the side stream overlap the dense layers, so the share is of GPU work, not of wall time)"}
    if rank == 0:
        n_param = sum(p.numel() for p in model.parameters())
        what = ("two-stream RPN fwd+bwd (BASELINE config 3)" if (args.image and args.rpn_only) else
                "rcnn_online training step, two-stream model (BASELINE config 4)" if args.image else
                "RPN fwd+bwd, point stream only" if args.rpn_only else
                "rcnn_online point-stream training step (BASELINE config 4 without the image stream)")
        print(json.dumps({"metric": what, "n_gpus": world, "image_stream": bool(args.image), "rpn_only": bool(args.rpn_only),
                          "sampler": args.sampler, "targets": args.targets, "ops_share": ops_share,
                          "scenes_per_gpu": args.batch, "points_per_scene": args.points, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(elapsed / args.steps * 1e3, 3),
                          "ms_per_step_median": round(sorted(per_step)[len(per_step) // 2] * 1e3, 3),
                          "ms_per_step_max": round(max(per_step) * 1e3, 3),
                          "ms_per_step_all": [round(x * 1e3, 2) for x in per_step],
                          "scenes_per_s": round(world * args.batch * args.steps / elapsed, 2),
                          "phase_ms": {k: round(v / args.steps, 3) for k, v in phases.items()},
                          "parameters": n_param, "grad_allreduce_MB": round(n_param * 4 / 1e6, 1) if world > 1 else 0,
                          "grad_allreduce": allreduce, "devices_distinct": scene_shard.distinct_devices([r_["device"] for r_ in per_rank]),
                          "devices": [r_["device"] for r_ in per_rank], "rehearsal": bool(args.rehearsal),
                          "per_rank_ms_per_step": {"min": min(r_["ms_per_step"] for r_ in per_rank),
                                                   "max": max(r_["ms_per_step"] for r_ in per_rank)},
                          "loss": last, "data": "synthetic", "dtype": "f32" if args.amp == "off" else "%s autocast (parameters f32)" % args.amp, **({} if raw is None else {"inputs": "raw"}),
                          **({} if not args.gt_aug else {"gt_aug": True}),
                          **({} if args.optimizer == "sgd" else {"optimizer": args.optimizer}),
                          **({} if args.optimizer != "fused" else {"optimizer_stats": dict(zip(optim.optim_cuda.STATS_NAMES, opt.stats.tolist()))}),
                          **({} if not scaled else {"loss_scale": dict(opt.scaler_state_dict(), mode="dynamic" if args.amp == "fp16" else "guard")}),
                          **({} if args.loss == "placeholder" else {"loss_mode": args.loss, "loss_terms": {
                              n_: round(float(v), 6) for r_ in last_out.values() for n_, v in zip(r_.names, r_.terms.tolist())}}),
                          "note": "phase_ms from HIP events (%s); "
                                  % ("phases are host-serialised by the two syncs of the target layer" if args.targets == "host" else
                                     "the target layer does not synchronise with the host") +
                                  "dense layers are stock PyTorch-ROCm, geometry ops this package's HIP kernels"}))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

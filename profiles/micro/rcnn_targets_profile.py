#!/usr/bin/env python3
"""The RCNN target layer at `--scenes` x 512 ROIs x 20 box rows x 16384 points x 130 feature columns (R = 64, S = 512), `--iters`
calls after one warm-up call, for a profiler run of their own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/micro/rcnn_targets_profile.py --layer host
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/micro/rcnn_targets_profile.py --layer fused

--layer host: the existing ProposalTargetLayer (host random streams, two read-backs); --layer fused: RCNNTargetLayer
(epnet_rcnn_sample_rois + epnet_roipool3d_train, device tables). Prints the bytes the sampling call has to move."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layer", default="fused", choices=["host", "fused"])
    ap.add_argument("--scenes", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    from epnet_amd import proposal_target_layer as ptl, rcnn_target_layer as rtl, synth
    dev = torch.device("cuda:0")
    b, m, n, g_rows, c = args.scenes, 512, 16384, 20, 130
    g = torch.Generator().manual_seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    rl, gl = [], []
    for i in range(b):
        bx, _ = synth.proposal_boxes(m + 12, seed=200 + i, num_objects=12, jitter=0.4)
        gt = torch.zeros((g_rows, 7))
        gt[:12] = bx[m:]
        rl.append(bx[:m])
        gl.append(gt)
    layer_in = {"roi_boxes3d": torch.stack(rl).to(dev), "gt_boxes3d": torch.stack(gl).to(dev),
                "rpn_xyz": synth.scenes("kitti", b, n, seed=9).to(dev), "rpn_features": torch.randn((b, n, c - 2), generator=g).to(dev),
                "seg_mask": (torch.rand((b, n), generator=g) > 0.5).float().to(dev), "pts_depth": (torch.rand((b, n), generator=g) * 70).to(dev)}
    layer = ptl.ProposalTargetLayer() if args.layer == "host" else rtl.RCNNTargetLayer()
    for _ in range(1 + args.iters):
        out = layer(layer_in)
    torch.cuda.synchronize()
    r = 64
    print("layer %s, scenes %d, %d calls (1 warm-up): sampling inputs %d bytes (ROIs B*M*28, boxes B*G*gc*4, tables B*M*4 + B*R*4), "
          "sampling outputs %d bytes, IoU matrix %d bytes; foreground labels %d" % (
              args.layer, b, 1 + args.iters, b * (m * 28 + g_rows * 28 + m * 4 + r * 4), b * r * 60 + b * 24, b * m * g_rows * 4,
              int((out["cls_label"] == 1).sum())))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The losses of one training step (2 scenes: 32768 RPN rows x 76, 128 RCNN rows x 46), forward + backward, `--iters` times, for a
kernel trace of their own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/micro/loss_profile.py [--form fused|composed|sync_free]

fused = epnet_amd.loss_utils (csrc/loss.hip); composed / sync_free = the two stock-torch forms of bench_ops.py. Prints the host
time per iteration; the kernel counts and times are the profiler's."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", default="fused", choices=["fused", "composed", "sync_free"])
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    import torch
    import bench_ops
    import bench_step
    from epnet_amd import loss_utils
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    xyz, gts = bench_step.synthetic_batch(2, 16384, 300, dev)
    cls_label, reg_label = bench_step.rpn_labels(xyz, gts)
    rpn_cls = (torch.randn((2, 16384, 1), generator=g) * 1.5).to(dev).requires_grad_(True)
    rpn_reg = (torch.randn((2, 16384, 76), generator=g) * 0.5).to(dev).requires_grad_(True)
    u = torch.rand((128,), generator=g).to(dev)
    ret = {"rcnn_cls": (torch.randn((128, 1), generator=g) * 1.5).to(dev).requires_grad_(True),
           "rcnn_reg": (torch.randn((128, 46), generator=g) * 0.5).to(dev).requires_grad_(True),
           "cls_label": torch.where(u > 0.6, 1, torch.where(u < 0.45, 0, -1)).long(), "reg_valid_mask": (u > 0.55).long(),
           "gt_of_rois": torch.cat([(torch.rand((128, 3), generator=g) - 0.5) * 2, torch.tensor([1.5, 1.6, 3.9]) * (0.9 + 0.2 * torch.rand((128, 3), generator=g)),
                                    torch.rand((128, 1), generator=g) * 6.28], dim=1).to(dev)}

    def step():
        if args.form == "fused":
            a, b = loss_utils.rpn_loss(rpn_cls, rpn_reg, cls_label, reg_label), loss_utils.rcnn_loss(ret)
        else:
            sf = args.form == "sync_free"
            a = bench_ops.composed_rpn_loss(rpn_cls, rpn_reg, cls_label, reg_label, sync_free=sf)
            b = bench_ops.composed_rcnn_loss(ret, sync_free=sf)
        torch.autograd.grad(a.loss + b.loss, [rpn_cls, rpn_reg, ret["rcnn_cls"], ret["rcnn_reg"]])
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        step()
    torch.cuda.synchronize()
    print("%s: %.3f ms per iteration (host clock, %d iterations + 3 warm-up)" % (args.form, (time.perf_counter() - t0) / args.iters * 1e3, args.iters))


if __name__ == "__main__":
    main()

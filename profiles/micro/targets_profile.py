#!/usr/bin/env python3
"""The fused RPN training targets (csrc/targets.hip) at `--scenes` x 16384 points x 20 box rows, `--iters` times, for a profiler
run of their own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/micro/targets_profile.py
    rocprofv3 --pmc WRITE_SIZE --output-format csv -d OUT -- python3 profiles/micro/targets_profile.py --iters 2
    rocprofv3 --pmc FETCH_SIZE --output-format csv -d OUT -- python3 profiles/micro/targets_profile.py --iters 2

Prints the bytes the call has to write (points 12 + class 4 + row 28 per point, 28 per box row) and to read, to set against
the counters (WRITE_SIZE and FETCH_SIZE count kilobytes here)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    import torch
    import bench_step
    from epnet_amd import rpn_target_layer as rtl
    dev = torch.device("cuda:0")
    b, n = args.scenes, 16384
    xyz, gts = bench_step.synthetic_batch(b, n, 300, dev)
    g = gts.shape[1]
    alpha = torch.zeros((b, g), device=dev)
    aug = rtl.draw_augmentation(b, rtl.default_cfg(), torch.Generator(device=dev).manual_seed(9), device=dev)
    for _ in range(args.iters):
        out = rtl.augment_and_label(xyz, gts, alpha, aug)
    torch.cuda.synchronize()
    print("scenes %d: output bytes per call %d, input bytes per call %d; fg %d ignored %d" % (
        b, b * n * 44 + b * g * 28, b * n * 12 + b * g * 32 + b * 16, int((out[2] == 1).sum()), int((out[2] == -1).sum())))


if __name__ == "__main__":
    main()

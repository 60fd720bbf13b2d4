#!/usr/bin/env python3
"""det_grad_bench.py -- each deterministic gradient (include/epnet_ops.h "*_det", taken under torch.use_deterministic_algorithms)
against the default one, at bench_ops.py's shapes (16 scenes and 1), BASELINE config 5's group_points_grad and the LI-Fusion
sampler's shapes. One JSON line per op and shape: median ms of both paths and their ratio."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch
from epnet_amd import pointnet2_cuda as p2, synth

dev = torch.device("cuda:0")
i32 = torch.int32
g = torch.Generator().manual_seed(0)


def timeit(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def both(op, shape, fn):
    torch.use_deterministic_algorithms(False)
    ms_default = timeit(fn)
    torch.use_deterministic_algorithms(True)
    ms_det = timeit(fn)
    torch.use_deterministic_algorithms(False)
    print(json.dumps({"op": op, "shape": shape, "default_ms": round(ms_default, 4), "det_ms": round(ms_det, 4),
                      "ratio": round(ms_det / ms_default, 2)}), flush=True)


def ball_lists(bsz, n, m, ns, r, seed=11):
    pts = synth.scenes("kitti", bsz, n, seed=seed).to(dev)
    cidx = torch.empty((bsz, m), dtype=i32, device=dev)
    ctr = torch.empty((bsz, m, 3), device=dev)
    p2.sample_centres_wrapper(bsz, n, m, pts, p2.scene_index(pts), cidx, ctr)
    idx = torch.empty((bsz, m, ns), dtype=i32, device=dev)
    p2.ball_query_wrapper(bsz, n, m, r, ns, ctr, pts, idx)
    return pts, ctr, idx


for bsz in (16, 1):
    for c, m, n in ((256, 4096, 16384), (512, 1024, 4096)):
        unknown = synth.scenes("kitti", bsz, n, seed=7).to(dev)
        kidx = torch.empty((bsz, m), dtype=i32, device=dev)
        known = torch.empty((bsz, m, 3), device=dev)
        p2.sample_centres_wrapper(bsz, n, m, unknown, p2.scene_index(unknown), kidx, known)
        d2 = torch.empty((bsz, n, 3), device=dev); idx = torch.empty((bsz, n, 3), dtype=i32, device=dev)
        p2.three_nn_wrapper(bsz, n, m, unknown, known, d2, idx)
        w = torch.rand((bsz, n, 3), generator=g).to(dev); w = (w / w.sum(-1, keepdim=True)).contiguous()
        go = torch.randn((bsz, c, n), generator=g).to(dev)
        gp = torch.zeros((bsz, c, m), device=dev)
        both("three_interpolate_grad", {"B": bsz, "C": c, "n": n, "m": m},
             lambda: p2.three_interpolate_grad_wrapper(bsz, c, n, m, go, idx, w, gp))
    for c, n, m, ns, r in ((96, 4096, 1024, 32, 1.0), (32, 16384, 4096, 16, 0.5)):
        pts, ctr, idx = ball_lists(bsz, n, m, ns, r)
        go = torch.randn((bsz, c, m, ns), generator=g).to(dev)
        gp = torch.zeros((bsz, c, n), device=dev)
        shape = {"B": bsz, "C": c, "N": n, "M": m, "ns": ns}
        both("group_points_grad", shape, lambda: p2.group_points_grad_wrapper(bsz, c, n, m, ns, go, idx, gp))
        go3 = torch.randn((bsz, 3 + c, m, ns), generator=g).to(dev)
        both("group_concat_grad", shape, lambda: p2.group_concat_grad_wrapper(bsz, c, n, m, ns, go3, idx, gp, True))
        gw = torch.zeros((c, 3), device=dev)
        both("group_linear_grad_w", shape, lambda: p2.group_linear_grad_w_wrapper(bsz, c, n, m, ns, go, pts, ctr, idx, gw))
    for c, n, m in ((3, 16384, 4096), (64, 4096, 1024)):
        gidx = torch.randint(0, n, (bsz, m), generator=g, dtype=i32).to(dev)
        go = torch.randn((bsz, c, m), generator=g).to(dev)
        gp = torch.zeros((bsz, c, n), device=dev)
        both("gather_points_grad", {"B": bsz, "C": c, "N": n, "M": m}, lambda: p2.gather_points_grad_wrapper(bsz, c, n, m, go, gidx, gp))
    # LI-Fusion: the image feature maps of the four levels and the sampled points of each SA level
    for c, h, w, n in ((64, 192, 640, 4096), (128, 96, 320, 1024), (256, 48, 160, 256), (512, 24, 80, 64)):
        xy = (torch.rand((bsz, n, 2), generator=g) * 2 - 1).to(dev)
        go = torch.randn((bsz, c, n), generator=g).to(dev)
        gm = torch.zeros((bsz, c, h, w), device=dev)
        both("feature_gather_grad", {"B": bsz, "C": c, "H": h, "W": w, "n": n},
             lambda: p2.feature_gather_grad_wrapper(bsz, c, h, w, n, True, go, xy, gm))

# BASELINE config 5: 65536-point scenes, 16384 centres x 64 neighbours
for bsz in (1, 16):
    n, m, ns, c = 65536, 16384, 64, 64
    pts, ctr, idx = ball_lists(bsz, n, m, ns, 0.5, seed=9)
    go = torch.randn((bsz, c, m, ns), generator=g).to(dev)
    gp = torch.zeros((bsz, c, n), device=dev)
    both("group_points_grad", {"B": bsz, "C": c, "N": n, "M": m, "ns": ns, "config": 5},
         lambda: p2.group_points_grad_wrapper(bsz, c, n, m, ns, go, idx, gp))

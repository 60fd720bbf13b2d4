#!/usr/bin/env python3
"""The fused RPN inputs from raw scans (csrc/scan.hip) at `--scenes` x 122 880 raw points -> 16384, `--iters` times, and the
image normalisation of the same number of scenes, for a profiler run of their own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/micro/scan_profile.py

Prints the bytes the call has to move (20 per raw point: the row and its key; 44 per output row), to set against the kernel times."""
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
    from epnet_amd import scan_layer, synth
    dev = torch.device("cuda:0")
    b, p, n = args.scenes, 122880, 16384
    base = [synth.lidar_scan(p - 1500 * k, seed=60 + k) for k in range(8)]
    pts, num_raw = scan_layer.collate_scans([base[k % 8] for k in range(b)])
    pts, num_raw = pts.to(dev), num_raw.to(dev)
    cal = [synth.calibration(k % 8) for k in range(b)]
    V2C, R0, P2, shape = (torch.stack([c[j] for c in cal]).to(dev) for j in range(4))
    tables = scan_layer.draw_scan_tables(b, p, n, torch.Generator(device=dev).manual_seed(11), dev)
    img = torch.randint(0, 256, (min(b, 64), 375, 1242, 3), dtype=torch.uint8, device=dev)
    for _ in range(args.iters):
        out = scan_layer.prepare_scans(pts, num_raw, V2C, R0, P2, shape, tables, npoints=n)
        scan_layer.normalise_images(img)
    torch.cuda.synchronize()
    info = out["scene_info"].cpu()
    print("scenes %d: bytes per call %d (B*P*20 + B*N*44); valid %s far %s cases %s; image scenes %d" % (
        b, b * p * 20 + b * n * 44, info[:4, 1].tolist(), info[:4, 2].tolist(), sorted(set(info[:, 3].tolist())), img.shape[0]))


if __name__ == "__main__":
    main()

"""is the scene index of the level-1 centres the same bytes when it is built twice from the same input? (alone, and beside a gather)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from epnet_amd import pointnet2_cuda as ext, synth
b, n_src, n = 256, 16384, 4096
dev = "cuda:0"
xyz = synth.scenes("kitti", b, n_src, seed=3).to(dev)
g = torch.Generator().manual_seed(1)
idx = torch.stack([torch.randperm(n_src, generator=g)[:n] for _ in range(b)]).to(torch.int32).to(dev)
nbytes = ext.scene_index_bytes(b, n)
outs = []
big = torch.randn((64, 1 << 20), device=dev)
for rep in range(6):
    index = torch.zeros((nbytes,), dtype=torch.uint8, device=dev)
    new_xyz = torch.empty((b, n, 3), device=dev)
    if rep >= 3:   # something else on the device beside it
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for _ in range(4):
                big = big * 1.0001
    ext.scene_index_build_gathered_wrapper(b, n_src, n, xyz, idx, new_xyz, index)
    torch.cuda.synchronize()
    outs.append((index.cpu(), new_xyz.cpu()))
np_ = 4096
for rep in range(1, 6):
    same = torch.equal(outs[0][0], outs[rep][0])
    diff = (outs[0][0] != outs[rep][0]).view(-1)
    sorted_bytes = b * np_ * 16
    print("run %d against run 0: index identical %s; differing bytes %d (in the sorted rows %d, in the boxes %d); centres identical %s" % (
        rep, same, int(diff.sum()), int(diff[:sorted_bytes].sum()), int(diff[sorted_bytes:].sum()), torch.equal(outs[0][1], outs[rep][1])))
    if not same:
        rows = diff[:sorted_bytes].view(b, np_, 16).any(dim=2)
        print("   scenes with a differing row: %d of %d; rows: %d" % (int(rows.any(dim=1).sum()), b, int(rows.sum())))

"""The serving loop of the staged row gathers, which loads the index vector of the next pass before it serves the current one.

Every output is held bit for bit to torch.gather on the same device: the kernels copy. What the shapes are for:
  * the staged two-scale route (gather_rows_lds2_kernel) needs b * chunks >= 512, p0 + p1 >= 3072 and p % 4 == 0; the cases are
    the smallest that take it with one, two, four and eight row groups per workgroup (1, 4 and 8 have a serving loop of their
    own, two goes through the generic one), with a ragged last chunk, and with a scale that is exactly one pass of the workgroup
    (256 threads x 4 positions), where the load "behind the last pass" is the first thing that happens;
  * npoints = 67 makes p = 1072 and 2144: neither is a multiple of a pass, so the last pass of either scale is partial and the
    vector behind it is read from the clamped address;
  * the one-scale kernel (gather_rows_lds_kernel) at p = 2048 + 4 and with two tiles, quad-staged and row-major;
  * the last valid index vector of every row holds n - 1 and 0, and the index tensors have a canary on either side, so what a
    load behind the row would bring is no valid index of a neighbouring allocation.

And the centres that fps_wave_kernel (clouds of up to 1024 points: SA levels 3 and 4) writes itself instead of leaving them to a
gather kernel behind it: idx is the oracle's and new_xyz == xyz[idx] bit for bit, where the rounds run and where a known prefix makes
the first m points the samples, for one scene and for more scenes than the chip has compute units to give one each at once.
"""
import functools

import numpy as np
import pytest
import torch

from epnet_amd import pointnet2_cuda as ext

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PASS = 1024   # positions per pass of a workgroup


@pytest.fixture
def guarded():
    from conftest import GuardedAlloc
    g = GuardedAlloc()
    yield g
    torch.cuda.synchronize()
    g.check()


def make_idx(g, b, p, n, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    idx = g.alloc((b, p), torch.int32, DEV)
    idx.copy_(torch.randint(0, n, (b, p), generator=gen, device=DEV, dtype=torch.int32))
    idx[:, -4:] = torch.tensor([n - 1, 0, n - 1, 0], dtype=torch.int32, device=DEV)
    return idx


def make_feat(b, c, n, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn((b, c, n), generator=gen, device=DEV)


def assert_gathered(out, feat, idx):
    """out (b, c, p) == feat[b, c, idx[b, p]], a few channels at a time (the int64 index of torch.gather is twice the output)"""
    b, c, _ = feat.shape
    p = idx.shape[1]
    ix = idx.long().view(b, 1, p)
    for c0 in range(0, c, 64):
        c1 = min(c, c0 + 64)
        want = torch.gather(feat[:, c0:c1], 2, ix.expand(b, c1 - c0, p))
        assert torch.equal(out[:, c0:c1], want), ("channels", c0, c1)


TWO_SCALE = [
    # b, c, n, npoints                                       rows per workgroup, chunks
    pytest.param(256, 8, 4096, 67, id="one_group"),         # 4, 2
    pytest.param(256, 16, 2048, 67, id="two_groups"),       # 8, 2
    pytest.param(32, 256, 1024, 67, id="four_groups"),      # 16, 16
    pytest.param(32, 512, 256, 67, id="eight_groups"),      # 32, 16
    pytest.param(256, 20, 2048, 67, id="ragged_chunk"),     # 8, 3: the last chunk holds 4 rows, one group
    pytest.param(256, 24, 2048, 67, id="three_chunks"),     # 8, 3
    pytest.param(512, 8, 256, 64, id="one_pass"),           # 8, 1: p = 1024 + 2048
    pytest.param(256, 8, 4096, 320, id="one_group_whole_iterations"),   # p = 5120 + 10240: two-pass iterations, odd pass count
]


@pytest.mark.parametrize("b,c,n,npoints", TWO_SCALE)
def test_two_scale_gather(guarded, b, c, n, npoints):
    nsamples = (16, 32)
    feat = make_feat(b, c, n, 1)
    idxs = [make_idx(guarded, b, npoints * ns, n, 2 + k) for k, ns in enumerate(nsamples)]
    rows = min(c, 32, 65536 // (4 * n)) & ~3                  # the launcher's: 64 KB of LDS, whole groups of four rows
    assert b * -(-c // rows) >= 512 and sum(i.shape[1] for i in idxs) >= 3 * PASS, "the shape misses the staged two-scale route"
    outs = [guarded.alloc((b, c, npoints, ns), torch.float32, DEV) for ns in nsamples]
    for o in outs:
        o.fill_(float("nan"))
    ext.group_concat_multi_wrapper(b, c, n, npoints, list(nsamples), None, None, feat, idxs, outs, False)
    for o, i in zip(outs, idxs):
        assert_gathered(o.view(b, c, -1), feat, i)


ONE_SCALE = [
    # b, c, n, npoints, nsample
    pytest.param(2, 16, 1024, 513, 4, id="four_groups_p2052"),
    pytest.param(2, 8, 4096, 513, 4, id="one_group_p2052"),
    pytest.param(2, 8, 4096, 1250, 4, id="one_group_two_tiles"),    # tiles of 3072: a two-pass iteration and one pass more
    pytest.param(2, 8, 1024, 1250, 4, id="two_groups_two_tiles"),
    pytest.param(2, 9, 1024, 1250, 4, id="row_major_two_tiles"),
    pytest.param(2, 9, 1024, 513, 4, id="row_major_p2052"),
]


@pytest.mark.parametrize("b,c,n,npoints,nsample", ONE_SCALE)
def test_one_scale_gather(guarded, b, c, n, npoints, nsample):
    p = npoints * nsample
    feat = make_feat(b, c, n, 5)
    idx = make_idx(guarded, b, p, n, 6)
    out = guarded.alloc((b, c, npoints, nsample), torch.float32, DEV)
    out.fill_(float("nan"))
    ext.group_points_wrapper(b, c, n, npoints, nsample, feat, idx.view(b, npoints, nsample), out)
    assert_gathered(out.view(b, c, p), feat, idx)


@functools.lru_cache(maxsize=None)
def sampled_level(n, m):
    """130 clouds of n points that are furthest-point sequences themselves (the n samples of 4 n random points, in sampling
    order, as an SA level hands them to the next), and the oracle's m samples of each"""
    from oracle import oracle
    oracle.build()
    rng = np.random.default_rng(n)
    cloud = rng.uniform(-1, 1, (130, 4 * n, 3)).astype(np.float32)
    first = oracle.furthest_point_sampling(cloud, n)
    xyz = np.ascontiguousarray(np.take_along_axis(cloud, first[:, :, None].astype(np.int64), 1))
    return xyz, oracle.furthest_point_sampling(xyz, m)


@pytest.mark.parametrize("prefix", [False, True], ids=["rounds", "known_prefix"])
@pytest.mark.parametrize("b", [1, 130])
@pytest.mark.parametrize("n,m", [(1024, 256), (256, 64)])
def test_fps_wave_writes_centres(guarded, n, m, b, prefix):
    xyz_h, want = sampled_level(n, m)
    xyz = torch.from_numpy(xyz_h[:b]).to(DEV)
    idx = guarded.alloc((b, m), torch.int32, DEV)
    new_xyz = guarded.alloc((b, m, 3), torch.float32, DEV)
    idx.fill_(-1)
    new_xyz.fill_(float("nan"))
    if prefix:   # every other scene (the first one too) is known to be a sequence of n samples: its first m are the answer
        known = torch.zeros((b,), dtype=torch.int32, device=DEV)
        known[::2] = n
        out = guarded.alloc((b,), torch.int32, DEV)
        ext.sample_centres_wrapper(b, n, m, xyz, None, idx, new_xyz, prefix_in=known, prefix_out=out, prefix_cap=0)
    else:
        ext.sample_centres_wrapper(b, n, m, xyz, None, idx, new_xyz)
    assert np.array_equal(idx.cpu().numpy(), want[:b])
    assert torch.equal(new_xyz, torch.gather(xyz, 1, idx.long().view(b, m, 1).expand(b, m, 3)))

"""epnet_group_concat_multi on shapes like the last SA level (few centres, many channels, short rows) against the CPU oracle,
exact equality, on either side of every condition of the staged two-scale route (csrc/group.hip):

  * the positions of the two scales TOGETHER >= 3072 (three passes of a 256-thread workgroup at 4 positions per thread):
    per-scale positions 1024 / 2048 in every combination (sums 2048, 3072, 4096), and 3068 / 3072 / 3076;
  * b * chunks >= 512 workgroups, chunks = ceil(C / rows), rows = min(64 KB / (4 n), C, 32) rounded down to whole groups of
    four where C and n are multiples of four: 511 / 512 / 513 with one chunk per scene (C = 8, 12), the nearest counts on
    either side with 16, 17 and 32 chunks (C = 512, 516; n = 1024);
  * C % 4 == 0 and n % 4 == 0 for the four-rows-per-LDS-word staging (C = 516 with n = 255: neither);
  * with and without the coordinate rows.

Whatever route a shape takes, the tensors are those of the oracle: gathers are copies, the centred coordinates one fp32
subtraction in the oracle's order.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded(hiplib):
    assert torch.cuda.is_available()
    return hiplib


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check(oracle, b, c, n, m, nss, use_xyz, seed, scenes_per_compare=32):
    from epnet_amd import pointnet2_cuda as ext
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-20.0, 20.0, (b, n, 3)).astype(np.float32)
    centres = np.ascontiguousarray(xyz[:, rng.permutation(n)[:m]])
    feats = rng.standard_normal((b, c, n)).astype(np.float32)
    idxs = [rng.integers(0, n, (b, m, ns)).astype(np.int32) for ns in nss]
    for i in idxs:   # the ends of the rows are read
        i[:, 0, 0] = n - 1
        i[:, -1, -1] = 0
    ch0 = 3 if use_xyz else 0
    outs = [torch.full((b, ch0 + c, m, ns), float("nan"), device=DEV) for ns in nss]
    ext.group_concat_multi_wrapper(b, c, n, m, list(nss), dev(xyz), dev(centres), dev(feats), [dev(i) for i in idxs], outs, use_xyz)
    torch.cuda.synchronize()
    for idx, out in zip(idxs, outs):
        for s in range(0, b, scenes_per_compare):
            e = min(b, s + scenes_per_compare)
            parts = []
            if use_xyz:
                xyz_t = np.ascontiguousarray(xyz[s:e].transpose(0, 2, 1))
                parts.append(oracle.group_points(xyz_t, idx[s:e]) - centres[s:e].transpose(0, 2, 1)[..., None])
            parts.append(oracle.group_points(feats[s:e], idx[s:e]))
            np.testing.assert_array_equal(out[s:e].cpu().numpy(), np.concatenate(parts, axis=1))


POSITIONS = [  # (m, (ns0, ns1)): per-scale positions 1024 / 2048, sums below / at / above 3072
    (64, (16, 16)), (64, (16, 32)), (64, (32, 16)), (64, (32, 32)),
    (59, (16, 36)),   # 944 + 2124 = 3068
    (64, (12, 36)),   # 768 + 2304 = 3072: the smaller scale below one pass of the workgroup
    (769, (1, 3)),    # 769 + 2307 = 3076: neither scale a multiple of four positions
]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("use_xyz", [True, False])
@pytest.mark.parametrize("m,nss", POSITIONS)
@pytest.mark.parametrize("c,n", [(8, 256), (12, 256), (512, 256), (516, 256), (516, 255), (512, 1024), (12, 255), (8, 1024)])
def test_positions_of_both_scales_around_the_threshold(oracle, c, n, m, nss, use_xyz):
    """enough scenes for a full chip (b * chunks >= 512) at every C, so that the positions alone decide the route"""
    if m > n:
        m, nss = 255, (5, 8)   # n = 255 / 256: 1275 + 2040 positions, the first scale not a multiple of four
    chunks = {8: 1, 12: 1, 512: 16 if n <= 256 else 32, 516: 17}[c]
    b = -(-512 // chunks)
    _check(oracle, b, c, n, m, nss, use_xyz, seed=c * 7 + n + m + nss[0])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("use_xyz", [True, False])
@pytest.mark.parametrize("b,c,n", [
    (511, 8, 256), (512, 8, 256), (513, 8, 256),          # one chunk per scene: 511 / 512 / 513 workgroups
    (511, 12, 255), (512, 12, 255), (513, 12, 255),       # the same, rows staged one by one (n % 4 != 0)
    (511, 12, 1024), (512, 12, 1024), (513, 12, 1024),
    (31, 512, 256), (32, 512, 256), (33, 512, 256),       # 16 chunks: 496 / 512 / 528
    (30, 516, 256), (31, 516, 256),                       # 17 chunks: 510 / 527
    (30, 516, 255), (31, 516, 255),
    (15, 512, 1024), (16, 512, 1024), (17, 512, 1024),    # 32 chunks of 16 rows: 480 / 512 / 544
])
def test_scene_counts_around_a_full_chip(oracle, b, c, n, use_xyz):
    """the last level's 64 x (16 + 32) positions, scene counts on either side of b * chunks = 512"""
    _check(oracle, b, c, n, 64, (16, 32), use_xyz, seed=b + c + n)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("b", [1, 2, 256])
@pytest.mark.parametrize("use_xyz", [True, False])
def test_last_level_of_the_bench(oracle, b, use_xyz):
    """C = 512, 256 points -> 64 centres x (16 + 32) samples: the shape bench.py runs at 256 scenes, and small batches of it"""
    _check(oracle, b, 512, 256, 64, (16, 32), use_xyz, seed=4 + b)

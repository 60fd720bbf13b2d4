"""Parity tests proper: the HIP path (called through the extension stand-ins, i.e. through the C ABI)
against the CPU oracle on the same seeded inputs, against the committed golden fixtures, and -- at
BASELINE.json's full sizes -- through size-independent properties.

Bar: bit-exact for indices / masks / flags and for pure copies; <= 1e-5 for float sums whose order the
reference itself leaves unspecified (atomic scatter-adds) and for the trig-dependent rotated IoU.
"""
import numpy as np
import pytest
import torch

from conftest import golden
from epnet_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded(hiplib):
    assert torch.cuda.is_available()
    return hiplib


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def rand_cloud(b, n, seed, kind="kitti"):
    from epnet_amd import synth
    return synth.scenes(kind, b, n, seed=seed).numpy()


# ------------------------------------------------------------------------------------------------ FPS

@pytest.mark.parametrize("b,n,m,kind", [
    (2, 4096, 1024, "ubox"),     # BASELINE config 1 shape, x2 scenes
    (1, 16384, 4096, "kitti"),   # level 1 of the RPN pyramid (16 points / thread, register resident)
    (2, 16384, 512, "dup"),      # duplicated rows at full width
    (3, 1024, 256, "kitti"),     # level 3
    (4, 256, 64, "kitti"),       # level 4
    (8, 512, 128, "dup"),        # RCNN-stage shape (512-pt ROI clouds), ties from padding
    (2, 1000, 300, "kitti"),     # non power of two: reference block size 512, 2 points / thread
    (2, 100, 40, "ubox"),        # block size 64
    (3, 37, 20, "ubox"),         # reference block size 32 < one wave
    (2, 3, 3, "ubox"), (1, 2, 2, "ubox"), (2, 1, 1, "ubox"),
    (1, 5000, 1, "ubox"),        # m = 1: only index 0
])
def test_fps_matches_oracle(oracle, b, n, m, kind):
    from epnet_amd import pointnet2_utils as p2u
    xyz = rand_cloud(b, n, seed=100 + n, kind=kind)
    got = host(p2u.furthest_point_sample(dev(xyz), m))
    np.testing.assert_array_equal(got, oracle.furthest_point_sampling(xyz, m))


def test_fps_ties_all_equal_and_heavy_duplicates(oracle):
    from epnet_amd import pointnet2_utils as p2u
    ones = np.ones((2, 2048, 3), np.float32)
    np.testing.assert_array_equal(host(p2u.furthest_point_sample(dev(ones), 7)), oracle.furthest_point_sampling(ones, 7))
    # 16 distinct points repeated 128 times, more picks than distinct points
    rng = np.random.default_rng(5)
    base = rng.standard_normal((16, 3)).astype(np.float32)
    xyz = base[rng.integers(0, 16, size=(2, 2048))]
    np.testing.assert_array_equal(host(p2u.furthest_point_sample(dev(xyz), 100)), oracle.furthest_point_sampling(xyz, 100))
    # integer lattice: many exact distance ties between distinct points
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(8), indexing="ij"), -1).reshape(1, -1, 3).astype(np.float32)
    np.testing.assert_array_equal(host(p2u.furthest_point_sample(dev(g), 512)), oracle.furthest_point_sampling(g, 512))


def test_fps_running_distance_buffer_and_streaming_path(oracle):
    """temp is an in/out buffer of the extension (sampling.cpp:36-46); 16384 < n <= 65536 takes the big-scene
    kernel over a private index, n > 65536 the streaming kernel"""
    from epnet_amd import pointnet2_cuda as ext
    for n, m in ((4096, 200), (20000, 48), (70000, 24)):
        xyz = rand_cloud(2, n, seed=7, kind="kitti")
        temp = torch.full((2, n), 1e10, device=DEV)
        idx = torch.empty((2, m), dtype=torch.int32, device=DEV)
        ext.furthest_point_sampling_wrapper(2, n, m, dev(xyz), temp, idx)
        o_idx, o_temp = oracle.furthest_point_sampling(xyz, m, return_temp=True)
        np.testing.assert_array_equal(host(idx), o_idx)
        np.testing.assert_array_equal(host(temp), o_temp)


@pytest.mark.parametrize("n,m", [(700, 50), (4096, 300), (16384, 500), (20000, 60), (70000, 12)])
def test_fps_continues_from_given_running_distances(oracle, n, m):
    """temp is an IN/out buffer: a call that starts from arbitrary running distances (here: those another cloud
    left behind) must give the reference's picks -- every kernel family, indexed and not"""
    from epnet_amd import pointnet2_cuda as ext
    xyz = rand_cloud(2, n, seed=n + 5, kind="kitti")
    start = np.abs(np.random.default_rng(n).standard_normal((2, n))).astype(np.float32) * 30.0
    o_idx, o_temp = oracle.furthest_point_sampling(xyz, m, return_temp=True, temp=start)
    d_xyz = dev(xyz)
    for index in (None, ext.scene_index(d_xyz)):
        temp = dev(start)
        idx = torch.empty((2, m), dtype=torch.int32, device=DEV)
        if index is None:
            ext.furthest_point_sampling_wrapper(2, n, m, d_xyz, temp, idx)
        else:
            ext.furthest_point_sampling_indexed_wrapper(2, n, m, d_xyz, index, temp, idx)
        np.testing.assert_array_equal(host(idx), o_idx)
        np.testing.assert_array_equal(host(temp), o_temp)


def test_fps_golden_fixtures():
    from epnet_amd import pointnet2_utils as p2u
    fx = golden("pointnet2_cfg1.npz")
    np.testing.assert_array_equal(host(p2u.furthest_point_sample(dev(fx["xyz"]), 1024)), fx["fps_idx"])
    ft = golden("fps_ties.npz")
    np.testing.assert_array_equal(host(p2u.furthest_point_sample(dev(ft["dup_xyz"]), 1500)), ft["dup_idx"])
    np.testing.assert_array_equal(host(p2u.furthest_point_sample(dev(ft["odd_xyz"]), 300)), ft["odd_idx"])


@pytest.mark.parametrize("env,n,m,kind", [
    ({"EPNET_FPS_PRUNE": 0}, 16384, 2048, "kitti"),      # brute force over 16 waves x 16 slots instead of the pruned kernel
    ({"EPNET_FPS_PRUNE": 0}, 4096, 1024, "dup"),
    ({"EPNET_FPS_PRUNE": 0}, 3000, 700, "kitti"),
    ({"EPNET_FPS_PRUNE_MIN": 4096}, 4096, 512, "kitti"),  # pruning only above 4096 points
    ({"EPNET_FPS_PRUNE_MIN": 4096}, 8192, 512, "dup"),
    ({"EPNET_FPS_PWAVES": 8}, 4096, 1024, "dup"),         # wave counts of the self-sorting pruned kernel
    ({"EPNET_FPS_PWAVES": 4}, 16384, 1024, "kitti"),
    ({"EPNET_FPS_WAVES": 1}, 1024, 256, "dup"),           # wave counts of the register-resident brute-force kernel
    ({"EPNET_FPS_WAVES": 4}, 1024, 256, "kitti"),
    ({"EPNET_FPS_WAVES": 2}, 512, 128, "dup"),
])
def test_fps_tuning_variants_match_oracle(oracle, env, n, m, kind):
    """every kernel an EPNET_FPS_* override selects gives the oracle's indices, running distances and centres at shapes
    where the library's own choice is another kernel: nothing in the product library is out of the tests' reach"""
    from epnet_amd import pointnet2_cuda as ext
    with _lib.tuning(**env):
        b = 2
        xyz = rand_cloud(b, n, seed=500 + n + m, kind=kind)
        o_idx, o_temp = oracle.furthest_point_sampling(xyz, m, return_temp=True)
        d_xyz = dev(xyz)
        temp = torch.full((b, n), 1e10, device=DEV)
        idx = torch.full((b, m), -1, dtype=torch.int32, device=DEV)
        ext.furthest_point_sampling_wrapper(b, n, m, d_xyz, temp, idx)
        np.testing.assert_array_equal(host(idx), o_idx)
        np.testing.assert_array_equal(host(temp), o_temp)
        index = ext.scene_index(d_xyz)
        temp.fill_(1e10); idx.fill_(-1)
        ext.furthest_point_sampling_indexed_wrapper(b, n, m, d_xyz, index, temp, idx)
        np.testing.assert_array_equal(host(idx), o_idx)
        np.testing.assert_array_equal(host(temp), o_temp)
        idx.fill_(-1)
        centres = torch.full((b, m, 3), float("nan"), device=DEV)
        ext.sample_centres_wrapper(b, n, m, d_xyz, index, idx, centres)
        np.testing.assert_array_equal(host(idx), o_idx)
        np.testing.assert_array_equal(host(centres), np.take_along_axis(xyz, o_idx[:, :, None].astype(np.int64), axis=1))


def test_config1_fixture_on_the_gpu():
    """BASELINE config 1 end to end on the GPU against the committed fixture (captured from the reference's own Python
    surface): FPS, gather, both ball queries (r = 0.1: nearly empty balls, r = 2.0: saturated) and QueryAndGroup"""
    from epnet_amd import pointnet2_utils as p2u
    fx = golden("pointnet2_cfg1.npz")
    xyz = dev(fx["xyz"])
    for index in (None, p2u.scene_index(xyz)):
        fps = p2u.furthest_point_sample(xyz, 1024, index)
        np.testing.assert_array_equal(host(fps), fx["fps_idx"])
        new_xyz = p2u.gather_operation(xyz.transpose(1, 2).contiguous(), fps).transpose(1, 2).contiguous()
        np.testing.assert_array_equal(host(new_xyz), fx["new_xyz"])
        np.testing.assert_array_equal(host(p2u.ball_query(0.1, 32, xyz, new_xyz, index)), fx["ball_idx_r01"])
        np.testing.assert_array_equal(host(p2u.ball_query(2.0, 32, xyz, new_xyz, index)), fx["ball_idx_r20"])
        np.testing.assert_array_equal(host(p2u.QueryAndGroup(2.0, 32)(xyz, new_xyz, None, index)), fx["query_and_group_r20"])
    both = p2u.ball_query_multi([0.1, 2.0], [32, 32], xyz, dev(fx["new_xyz"]))
    np.testing.assert_array_equal(host(both[0]), fx["ball_idx_r01"])
    np.testing.assert_array_equal(host(both[1]), fx["ball_idx_r20"])
    idx2, centres = p2u.sample_and_gather(xyz, 1024, None)
    np.testing.assert_array_equal(host(idx2), fx["fps_idx"])
    np.testing.assert_array_equal(host(centres), fx["new_xyz"])


def test_fps_full_size_properties():
    """B = 16 scenes of 16384 points -> 4096: index 0 first, all indices distinct (the clouds have no
    duplicate rows), and the greedy max-min property holds for the sequence (checked in float64 on a
    prefix: each pick maximises the distance to the picks before it, up to fp32 rounding)."""
    from epnet_amd import pointnet2_utils as p2u
    xyz = rand_cloud(16, 16384, seed=50, kind="ubox")
    idx = host(p2u.furthest_point_sample(dev(xyz), 4096))
    assert (idx[:, 0] == 0).all() and idx.min() >= 0 and idx.max() < 16384
    for b in range(16):
        assert len(np.unique(idx[b])) == 4096
    p = xyz[3].astype(np.float64)
    d = np.full(16384, np.inf)
    for j in range(1, 64):
        d = np.minimum(d, ((p - p[idx[3, j - 1]]) ** 2).sum(1))
        assert d[idx[3, j]] >= d.max() * (1 - 1e-6)


@pytest.mark.parametrize("b,n,m,kind", [
    (2, 16384, 4096, "kitti"), (2, 16384, 300, "dup"), (2, 8192, 700, "kitti"), (3, 4096, 1024, "kitti"),
    (2, 2048, 512, "ubox"), (2, 1025, 64, "kitti"), (2, 1500, 1499, "dup"), (2, 10000, 33, "ubox"),
    (2, 1024, 256, "kitti"),     # indexed for the ball queries only: sampling takes the one-wave kernel
    (2, 900, 100, "kitti"),      # below the indexed range: index is None, plain path
    (1, 20000, 20, "kitti"),     # beyond the register file: bucket summaries in registers, points in the index
    (2, 30000, 700, "dup"), (1, 65536, 1500, "kitti"), (2, 16385, 300, "ubox"),
])
def test_fps_over_scene_index_matches_oracle(oracle, b, n, m, kind):
    """epnet_furthest_point_sampling_indexed: same indices AND running distances as the plain entry point"""
    from epnet_amd import pointnet2_cuda as ext
    xyz = rand_cloud(b, n, seed=300 + n, kind=kind)
    d_xyz = dev(xyz)
    index = ext.scene_index(d_xyz)
    assert (index is None) == (n < 1024)
    temp = torch.full((b, n), 1e10, device=DEV)
    idx = torch.empty((b, m), dtype=torch.int32, device=DEV)
    ext.furthest_point_sampling_indexed_wrapper(b, n, m, d_xyz, index, temp, idx)
    o_idx, o_temp = oracle.furthest_point_sampling(xyz, m, return_temp=True)
    np.testing.assert_array_equal(host(idx), o_idx)
    np.testing.assert_array_equal(host(temp), o_temp)


@pytest.mark.parametrize("b,n,m,kind", [
    (2, 16384, 4096, "kitti"), (2, 16384, 1500, "dup"), (2, 4096, 1024, "kitti"), (2, 2048, 2047, "ubox"),
    (2, 1024, 256, "kitti"), (3, 256, 64, "kitti"), (2, 40, 7, "ubox"), (1, 20000, 33, "kitti"), (2, 5000, 1, "ubox"),
])
def test_sample_and_gather_equals_fps_then_gather(oracle, b, n, m, kind):
    """epnet_sample_centres: the indices of FPS from a fresh state and exactly the rows they select"""
    from epnet_amd import pointnet2_utils as p2u
    xyz = rand_cloud(b, n, seed=900 + n, kind=kind)
    d_xyz = dev(xyz)
    o_idx = oracle.furthest_point_sampling(xyz, m)
    want = np.take_along_axis(xyz, o_idx[..., None].astype(np.int64), axis=1)
    for index in (p2u.scene_index(d_xyz), None):
        idx, new_xyz = p2u.sample_and_gather(d_xyz, m, index)
        np.testing.assert_array_equal(host(idx), o_idx)
        np.testing.assert_array_equal(host(new_xyz), want)


def test_fps_over_scene_index_ties(oracle):
    from epnet_amd import pointnet2_cuda as ext
    rng = np.random.default_rng(5)
    base = rng.standard_normal((16, 3)).astype(np.float32)
    lattice = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(8), indexing="ij"), -1).reshape(1, -1, 3)
    for xyz, m in ((np.ones((2, 2048, 3), np.float32), 7), (base[rng.integers(0, 16, size=(2, 4096))], 100),
                   (lattice.astype(np.float32), 512)):
        b, n = xyz.shape[:2]
        d_xyz = dev(xyz)
        temp = torch.full((b, n), 1e10, device=DEV)
        idx = torch.empty((b, m), dtype=torch.int32, device=DEV)
        ext.furthest_point_sampling_indexed_wrapper(b, n, m, d_xyz, ext.scene_index(d_xyz), temp, idx)
        np.testing.assert_array_equal(host(idx), oracle.furthest_point_sampling(xyz, m))


@pytest.mark.parametrize("b,n,m,scales,kind", [
    (2, 16384, 4096, ((0.1, 16), (0.5, 32)), "kitti"), (2, 4096, 1024, ((0.5, 16), (1.0, 32)), "kitti"),
    (2, 1024, 256, ((1.0, 16), (2.0, 32)), "kitti"), (1, 16384, 700, ((2.5, 64), (0.3, 8)), "kitti"),  # crowded + unsorted radii
    (2, 3000, 500, ((0.7, 5), (0.7, 9)), "ubox"), (1, 2048, 300, ((100.0, 40), (0.01, 3)), "dup"),
    (2, 4096, 128, ((0.5, 16), (1.0, 32), (2.0, 8)), "kitti"),   # three scales: one launch per scale
    (2, 500, 100, ((0.8, 16), (1.6, 32)), "kitti"),              # below the indexed range
    (1, 3000, 200, ((5.0, 100), (0.5, 3)), "ubox"),              # nsample beyond the 64-entry hit list
    (2, 2048, 1, ((1.0, 8), (2.0, 16)), "kitti"), (2, 2048, 3, ((1.0, 8), (2.0, 16)), "kitti"),   # odd tails of the pair kernel
])
@pytest.mark.parametrize("pair", [0, 1])   # one / two centres per wave (the library picks by launch size)
def test_ball_queries_of_an_msg_level_in_one_launch(oracle, b, n, m, scales, kind, pair):
    from epnet_amd import pointnet2_cuda as ext
    with _lib.tuning(EPNET_BQ_PAIR=pair):
        xyz = rand_cloud(b, n, seed=700 + n, kind=kind)
        centres = np.ascontiguousarray(xyz[:, :: max(1, n // m)][:, :m])
        d_xyz, d_c = dev(xyz), dev(centres)
        outs = [torch.full((b, m, ns), -5, dtype=torch.int32, device=DEV) for _r, ns in scales]
        ext.ball_query_multi_wrapper(b, n, m, [r for r, _ in scales], [ns for _, ns in scales], d_c, d_xyz, ext.scene_index(d_xyz), outs)
        for (r, ns), got in zip(scales, outs):
            np.testing.assert_array_equal(host(got), oracle.ball_query(r, ns, xyz, centres))


def test_one_scene_index_serves_sampling_and_both_ball_queries(oracle):
    """the SA-level call pattern: index once, then FPS + the two MSG ball queries"""
    from epnet_amd import pointnet2_cuda as ext
    b, n, m = 2, 16384, 4096
    xyz = rand_cloud(b, n, seed=77, kind="kitti")
    d_xyz = dev(xyz)
    index = torch.empty((ext._lib.lib().epnet_scene_index_bytes(b, n),), dtype=torch.uint8, device=DEV)
    ext.scene_index_build_wrapper(b, n, d_xyz, index)
    temp = torch.full((b, n), 1e10, device=DEV)
    fidx = torch.empty((b, m), dtype=torch.int32, device=DEV)
    ext.furthest_point_sampling_indexed_wrapper(b, n, m, d_xyz, index, temp, fidx)
    o_idx = oracle.furthest_point_sampling(xyz, m)
    np.testing.assert_array_equal(host(fidx), o_idx)
    new_xyz = np.ascontiguousarray(np.take_along_axis(xyz, o_idx[..., None].astype(np.int64), axis=1))
    for radius, ns in ((0.1, 16), (0.5, 32)):
        idx = torch.full((b, m, ns), -7, dtype=torch.int32, device=DEV)
        ext.ball_query_indexed_wrapper(b, n, m, radius, ns, dev(new_xyz), d_xyz, index, idx)
        np.testing.assert_array_equal(host(idx), oracle.ball_query(radius, ns, xyz, new_xyz))


# ------------------------------------------------------------------------------------------------ ball query

@pytest.mark.parametrize("b,n,m,radius,ns,kind", [
    (1, 4096, 1024, 0.1, 32, "ubox"), (1, 4096, 1024, 2.0, 32, "ubox"),
    (2, 16384, 4096, 0.1, 16, "kitti"), (2, 16384, 4096, 0.5, 32, "kitti"),
    (2, 4096, 1024, 0.5, 16, "kitti"), (2, 4096, 1024, 1.0, 32, "kitti"),
    (2, 1024, 256, 1.0, 16, "kitti"), (2, 1024, 256, 2.0, 32, "kitti"),
    (2, 256, 64, 2.0, 16, "kitti"), (2, 256, 64, 4.0, 32, "kitti"),
    (16, 512, 128, 0.2, 64, "kitti"), (16, 128, 32, 0.4, 64, "kitti"),   # RCNN stage
    (3, 1000, 77, 1.5, 5, "kitti"), (2, 2100, 9, 3.0, 70, "kitti"), (1, 63, 3, 50.0, 8, "ubox"),
    (1, 5000, 13, 100.0, 128, "ubox"),                                   # every ball saturates at once
    (1, 65536, 300, 0.5, 64, "kitti"), (1, 40000, 100, 0.8, 48, "kitti"),  # config-5 size: largest indexed path
])
@pytest.mark.parametrize("pair", [0, 1])
def test_ball_query_matches_oracle(oracle, b, n, m, radius, ns, kind, pair):
    from epnet_amd import pointnet2_utils as p2u
    with _lib.tuning(EPNET_BQ_PAIR=pair):
        xyz = rand_cloud(b, n, seed=200 + n + m, kind=kind)
        centres = np.ascontiguousarray(xyz[:, np.random.default_rng(n).permutation(n)[:m]])
        if kind == "ubox":
            centres[:, -1] = 1e4  # one empty ball per scene -> all-zero row
        got = host(p2u.ball_query(radius, ns, dev(xyz), dev(centres)))
        np.testing.assert_array_equal(got, oracle.ball_query(radius, ns, xyz, centres))


def test_ball_query_writes_every_slot_and_boundary_is_strict(oracle):
    from epnet_amd import pointnet2_cuda as ext
    xyz = np.zeros((1, 130, 3), np.float32)
    xyz[0, :, 0] = np.arange(130)
    centres = np.array([[[64.0, 0, 0], [1000.0, 0, 0]]], np.float32)
    idx = torch.full((1, 2, 6), -7, dtype=torch.int32, device=DEV)      # garbage in: must be overwritten
    ext.ball_query_wrapper(1, 130, 2, 2.0, 6, dev(centres), dev(xyz), idx)
    assert host(idx).tolist() == [[[63, 64, 65, 63, 63, 63], [0, 0, 0, 0, 0, 0]]]


@pytest.mark.parametrize("n,order", [(16384, "descending"), (16384, "ascending"), (16384, "random"), (2048, "descending"), (65536, "descending")])
@pytest.mark.parametrize("pair,stream", [(0, 0), (1, 0), (1, 1)])
def test_ball_query_crowded_lists_keep_the_smallest_indices(oracle, n, order, pair, stream):
    """balls that hold thousands of points. The streaming variant of the pair kernel (the library's choice above 16384 points,
    forced here on every size) cuts a hit list that runs full during the walk down to its nsample smallest ORIGINAL indices, again
    and again, with a threshold for what the list takes afterwards; the other kernels walk a second time through a bitmap.
    `descending`: the walk (cell order: along x) meets the largest indices first, so every cut replaces the whole list;
    `ascending`: the first cut already holds the answer; nsample 1 .. 64, and 100 (beyond a list: always the bitmap pass)"""
    from epnet_amd import pointnet2_cuda as ext
    with _lib.tuning(EPNET_BQ_PAIR=pair, EPNET_BQ_STREAM=stream):
        rng = np.random.default_rng(n)
        xyz = (rng.random((1, n, 3)) * np.array([40.0, 1.0, 1.0])).astype(np.float32)
        perm = {"ascending": np.argsort(xyz[0, :, 0]), "descending": np.argsort(-xyz[0, :, 0]), "random": rng.permutation(n)}[order]
        xyz = np.ascontiguousarray(xyz[:, perm])
        m = 37
        centres = np.ascontiguousarray(xyz[:, rng.permutation(n)[:m]])
        centres[0, -1] = (20.0, 0.5, 0.5)
        d_xyz, d_c = dev(xyz), dev(centres)
        index = ext.scene_index(d_xyz)
        scales = ((6.0, 64), (9.0, 1)), ((3.0, 5), (50.0, 33)), ((7.0, 100), (2.0, 64))
        for sc in scales:
            outs = [torch.full((1, m, ns), -5, dtype=torch.int32, device=DEV) for _r, ns in sc]
            ext.ball_query_multi_wrapper(1, n, m, [r for r, _ in sc], [ns for _, ns in sc], d_c, d_xyz, index, outs)
            for (r, ns), got in zip(sc, outs):
                want = oracle.ball_query(r, ns, xyz, centres)
                np.testing.assert_array_equal(host(got), want)
        hits = (np.linalg.norm(xyz[0][None] - centres[0][:, None], axis=-1) < 6.0).sum(1)
        assert hits.min() > (512 if n >= 16384 else 256)                   # every ball overflows the longest list of its kernel


def test_ball_query_indexed_and_direct_paths_agree(oracle):
    """epnet_ball_query (direct scan) and epnet_ball_query_ws (spatially indexed, caller scratch) are two
    entry points of the C ABI with bit-identical output; the workspace contract is checked too"""
    from epnet_amd import _lib
    l = _lib.lib()
    for b, n, m, radius, ns, kind in ((2, 4096, 513, 0.8, 24, "kitti"), (1, 16384, 1000, 0.3, 16, "dup"), (2, 3000, 77, 1.0, 40, "ubox")):
        xyz = rand_cloud(b, n, seed=31 + n, kind=kind)
        centres = np.ascontiguousarray(xyz[:, np.random.default_rng(3).permutation(n)[:m]])
        centres[:, 0] += 500.0  # an empty ball
        dx, dc = dev(xyz), dev(centres)
        want = oracle.ball_query(radius, ns, xyz, centres)
        direct = torch.full((b, m, ns), -3, dtype=torch.int32, device=DEV)
        assert l.epnet_ball_query(b, n, m, radius, ns, dc.data_ptr(), dx.data_ptr(), direct.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        nbytes = l.epnet_ball_query_workspace_bytes(b, n, m)
        assert nbytes > 0
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
        indexed = torch.full((b, m, ns), -3, dtype=torch.int32, device=DEV)
        stream = torch.cuda.current_stream().cuda_stream
        assert l.epnet_ball_query_ws(b, n, m, radius, ns, dc.data_ptr(), dx.data_ptr(), indexed.data_ptr(), ws.data_ptr(), nbytes, stream) == 0
        assert l.epnet_ball_query_ws(b, n, m, radius, ns, dc.data_ptr(), dx.data_ptr(), indexed.data_ptr(), ws.data_ptr(), nbytes - 16, stream) == -3  # ENOMEM
        np.testing.assert_array_equal(host(direct), want)
        np.testing.assert_array_equal(host(indexed), want)
    assert l.epnet_ball_query_workspace_bytes(4, 512, 128) == 0 and l.epnet_ball_query_workspace_bytes(1, 70000, 16384) == 0


def test_ball_query_full_size_property():
    """config 5 shape on a reduced batch: 65536 points, 16384 centres, nsample 64: every index lies in
    the ball or is the padding value, and the hits are strictly increasing."""
    from epnet_amd import pointnet2_utils as p2u
    xyz = rand_cloud(1, 65536, seed=9, kind="kitti")
    centres = np.ascontiguousarray(xyz[:, ::4])
    idx = host(p2u.ball_query(0.5, 64, dev(xyz), dev(centres)))[0]
    d2 = ((xyz[0][idx] - centres[0][:, None, :]) ** 2).sum(-1)
    assert (d2 < 0.25 + 1e-6).all()                      # every centre is a cloud point -> no empty ball
    first = idx[:, :1]
    inc = (np.diff(idx, axis=1) > 0) | (idx[:, 1:] == first)
    assert inc.all()


# ------------------------------------------------------------------------------------------------ gathers

@pytest.mark.parametrize("b,c,n,m,ns", [(2, 3, 4096, 1024, 16), (2, 96, 4096, 1024, 32), (1, 256, 1024, 256, 16),
                                        (2, 17, 333, 21, 5), (1, 1, 64, 7, 3), (4, 128, 512, 128, 64)])
def test_group_points_exact(oracle, b, c, n, m, ns):
    from epnet_amd import pointnet2_utils as p2u
    rng = np.random.default_rng(c * n)
    feats = rng.standard_normal((b, c, n)).astype(np.float32)
    idx = rng.integers(0, n, size=(b, m, ns)).astype(np.int32)
    np.testing.assert_array_equal(host(p2u.grouping_operation(dev(feats), dev(idx))), oracle.group_points(feats, idx))


@pytest.mark.parametrize("b,c,n,m", [(2, 3, 16384, 4096), (2, 3, 4096, 1024), (3, 5, 100, 33)])
def test_gather_points_exact(oracle, b, c, n, m):
    from epnet_amd import pointnet2_utils as p2u
    rng = np.random.default_rng(n + m)
    feats = rng.standard_normal((b, c, n)).astype(np.float32)
    idx = rng.integers(0, n, size=(b, m)).astype(np.int32)
    np.testing.assert_array_equal(host(p2u.gather_operation(dev(feats), dev(idx))), oracle.gather_points(feats, idx))


def test_group_full_size_against_torch():
    """level-2 feature grouping at B = 8 (C=96, N=4096, M=1024, ns=32): equals a torch.gather"""
    from epnet_amd import pointnet2_utils as p2u
    g = torch.Generator().manual_seed(3)
    feats = torch.randn((8, 96, 4096), generator=g).to(DEV)
    idx = torch.randint(0, 4096, (8, 1024, 32), generator=g, dtype=torch.int32).to(DEV)
    out = p2u.grouping_operation(feats, idx)
    ref = torch.gather(feats, 2, idx.view(8, 1, -1).expand(-1, 96, -1).long()).view(8, 96, 1024, 32)
    assert torch.equal(out, ref)


@pytest.mark.parametrize("b,c,n,m,ns", [(2, 96, 4096, 1024, 32), (2, 5, 333, 21, 5), (1, 3, 20000, 100, 8), (2, 256, 256, 64, 16)])
def test_group_points_grad(oracle, b, c, n, m, ns):
    from epnet_amd import pointnet2_cuda as ext
    rng = np.random.default_rng(7 * c + n)
    go = rng.standard_normal((b, c, m, ns)).astype(np.float32)
    idx = rng.integers(0, n, size=(b, m, ns)).astype(np.int32)
    grad = torch.zeros((b, c, n), device=DEV)
    ext.group_points_grad_wrapper(b, c, n, m, ns, dev(go), dev(idx), grad)
    np.testing.assert_allclose(host(grad), oracle.group_points_grad(go, idx, n), rtol=1e-5, atol=1e-5)


def _skewed_indices(rng, b, n, count, mode):
    """neighbour lists as uneven as real ones get (and worse)"""
    if mode == "uniform":
        return rng.integers(0, n, size=(b, count))
    if mode == "one":            # every entry to ONE target: a single run across all 1024 threads of the sum kernel
        return np.full((b, count), n // 3)
    if mode == "few":            # a handful of targets share everything
        return rng.choice(np.array([0, 1, n // 2, n - 1]), size=(b, count))
    if mode == "zipf":           # a few targets with thousands of entries, a long tail with one or none
        z = rng.zipf(1.3, size=(b, count))
        return np.minimum(z - 1, n - 1)
    if mode == "blocks":         # ball-query padding: one index repeated nsample times in a row
        return np.repeat(rng.integers(0, n, size=(b, (count + 31) // 32)), 32, axis=1)[:, :count]
    raise ValueError(mode)


@pytest.mark.parametrize("b,c,n,m,ns,mode", [
    (16, 96, 4096, 1024, 32, "blocks"),    # the level-2 shape: one 128 KB row per pass
    (3, 10, 4096, 1024, 32, "zipf"),
    (2, 7, 4096, 1024, 32, "one"),
    (2, 5, 4096, 1024, 32, "few"),
    (2, 96, 4096, 1024, 16, "uniform"),    # two rows per pass
    (5, 33, 1024, 256, 16, "zipf"),        # four / eight rows per pass, channel count not a multiple of it
    (130, 19, 512, 128, 64, "blocks"),     # RCNN shape, many scenes
    (2, 9, 333, 128, 8, "uniform"),        # target count not a multiple of 4: scalar write-back
    (2, 4, 1000, 1024, 4, "one"),          # exactly one chunk of entries, no padding
    (1, 3, 16384, 1025, 4, "zipf"),        # 4100 entries: 4092 padding entries of the dump target
    (2, 6, 50, 16, 4, "few"),              # 64 entries for 1024 threads: almost everything is padding
    (2, 16, 16384, 4096, 16, "blocks"),    # level-1 shapes: rows of 65536 / 131072 positions worked off in tiles of 20480
    (2, 5, 16384, 4096, 32, "zipf"),
    (1, 3, 9000, 5000, 20, "uniform"),     # 100000 positions, 9000 targets: tiles of 28672
])
def test_group_points_grad_uneven_lists(oracle, b, c, n, m, ns, mode):
    """the run-sum gradient (csrc/runsum.h) on neighbour lists of every shape: equal shares of the sorted entries per
    thread, runs handed across thread boundaries, the padding run, rows per pass from 1 to 8; accumulation INTO the buffer"""
    from epnet_amd import pointnet2_cuda as ext
    rng = np.random.default_rng(b * 131 + c)
    go = rng.standard_normal((b, c, m, ns)).astype(np.float32)
    idx = _skewed_indices(rng, b, n, m * ns, mode).reshape(b, m, ns).astype(np.int32)
    start = rng.standard_normal((b, c, n)).astype(np.float32)
    grad = dev(start)
    ext.group_points_grad_wrapper(b, c, n, m, ns, dev(go), dev(idx), grad)
    # float64 yardstick with a per-element bound from the list's sum of magnitudes: the order of a list's terms is free
    # (atomicAdd in the reference), so a list of 32768 terms may differ from the oracle's sequential fp32 sum by more than 1e-5
    want = np.zeros((b, c, n))
    mag = np.zeros((b, c, n))
    flat = idx.reshape(b, -1).astype(np.int64)
    for s_ in range(b):
        np.add.at(want[s_].T, flat[s_], go[s_].reshape(c, -1).T.astype(np.float64))
        np.add.at(mag[s_].T, flat[s_], np.abs(go[s_].reshape(c, -1).T).astype(np.float64))
    err = np.abs(host(grad).astype(np.float64) - (start + want))
    assert (err <= 1e-7 * mag + 1e-5 * np.maximum(1.0, np.abs(start + want))).all(), float(err.max())
    np.testing.assert_allclose(oracle.group_points_grad(go, idx, n), want, rtol=1e-3, atol=1e-2)   # the oracle agrees with the yardstick


@pytest.mark.parametrize("b,c,n,m,mode", [(16, 32, 16384, 4096, "zipf"), (2, 9, 16384, 4096, "one"), (3, 17, 4096, 1024, "uniform"),
                                          (2, 40, 1024, 256, "few"), (4, 6, 256, 64, "zipf"), (2, 3, 21844, 100, "uniform")])
def test_three_interpolate_grad_uneven_lists(oracle, b, c, n, m, mode):
    from epnet_amd import pointnet2_cuda as ext
    rng = np.random.default_rng(b * 17 + c)
    go = rng.standard_normal((b, c, n)).astype(np.float32)
    idx = _skewed_indices(rng, b, m, n * 3, mode).reshape(b, n, 3).astype(np.int32)
    w = rng.random((b, n, 3)).astype(np.float32)
    w /= w.sum(-1, keepdims=True)
    start = rng.standard_normal((b, c, m)).astype(np.float32)
    grad = dev(start)
    ext.three_interpolate_grad_wrapper(b, c, n, m, dev(go), dev(idx), dev(w), grad)
    terms = (go[:, :, :, None].astype(np.float64) * w[:, None, :, :].astype(np.float32).astype(np.float64)).reshape(b, c, n * 3)
    flat = idx.reshape(b, -1).astype(np.int64)
    want = np.zeros((b, c, m))
    mag = np.zeros((b, c, m))
    for s_ in range(b):
        np.add.at(want[s_].T, flat[s_], terms[s_].T)
        np.add.at(mag[s_].T, flat[s_], np.abs(terms[s_]).T)
    err = np.abs(host(grad).astype(np.float64) - (start + want))
    assert (err <= 2e-7 * mag + 1e-5 * np.maximum(1.0, np.abs(start + want))).all(), float(err.max())
    np.testing.assert_allclose(oracle.three_interpolate_grad(go, idx, w, m), want, rtol=1e-3, atol=1e-2)


def test_gather_points_grad_and_accumulation(oracle):
    from epnet_amd import pointnet2_cuda as ext
    rng = np.random.default_rng(11)
    go = rng.standard_normal((2, 3, 500)).astype(np.float32)
    idx = rng.integers(0, 2000, size=(2, 500)).astype(np.int32)
    grad = torch.ones((2, 3, 2000), device=DEV)  # the kernel accumulates INTO the buffer, like atomicAdd does
    ext.gather_points_grad_wrapper(2, 3, 2000, 500, dev(go), dev(idx), grad)
    np.testing.assert_allclose(host(grad), 1 + oracle.gather_points_grad(go, idx, 2000), rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------ interpolation

@pytest.mark.parametrize("b,n,m", [(2, 256, 64), (2, 1024, 256), (2, 4096, 1024), (1, 16384, 4096), (3, 77, 13), (2, 40, 5000),
                                   # known sets whose own index pads to an ODD multiple of 256 (2304, 2816, 3328, 3840): the staged
                                   # index build's last round of 512 is half a round (it once wrote a whole one: past the scene, and
                                   # for the last scene into the bucket boxes -- found by tests/test_gpu_sweep.py)
                                   (3, 4096, 2259), (2, 3000, 2816), (1, 5000, 3300), (2, 2000, 3840)])
def test_three_nn_matches_oracle(oracle, b, n, m):
    from epnet_amd import pointnet2_cuda as ext
    unknown = rand_cloud(b, n, seed=n, kind="kitti")
    known = np.ascontiguousarray(rand_cloud(b, max(m, 8), seed=n + 1, kind="kitti")[:, :m])
    d2 = torch.empty((b, n, 3), device=DEV)
    idx = torch.empty((b, n, 3), dtype=torch.int32, device=DEV)
    ext.three_nn_wrapper(b, n, m, dev(unknown), dev(known), d2, idx)
    o_d2, o_idx = oracle.three_nn(unknown, known)
    np.testing.assert_array_equal(host(idx), o_idx)
    np.testing.assert_array_equal(host(d2), o_d2)


def test_three_nn_ties_and_short_known(oracle):
    from epnet_amd import pointnet2_cuda as ext
    rng = np.random.default_rng(2)
    base = rng.standard_normal((6, 3)).astype(np.float32)
    known = base[rng.integers(0, 6, size=(2, 100))]            # heavy duplicates: distance ties everywhere
    unknown = rng.standard_normal((2, 50, 3)).astype(np.float32)
    for m in (100, 9, 2, 1):
        kn = np.ascontiguousarray(known[:, :m])
        d2 = torch.empty((2, 50, 3), device=DEV)
        idx = torch.empty((2, 50, 3), dtype=torch.int32, device=DEV)
        ext.three_nn_wrapper(2, 50, m, dev(unknown), dev(kn), d2, idx)
        o_d2, o_idx = oracle.three_nn(unknown, kn)
        np.testing.assert_array_equal(host(idx), o_idx)
        np.testing.assert_array_equal(host(d2), o_d2)            # inf in the unfilled slots when m < 3


def test_three_nn_indexed_and_direct_paths_agree(oracle):
    from epnet_amd import _lib
    l = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    for b, n, m, kind in ((2, 3000, 1024, "kitti"), (1, 500, 5000, "dup"), (2, 777, 600, "ubox")):
        unknown = rand_cloud(b, n, seed=61 + n, kind=kind)
        known = np.ascontiguousarray(rand_cloud(b, m, seed=62 + m, kind=kind))
        du, dk = dev(unknown), dev(known)
        o_d2, o_idx = oracle.three_nn(unknown, known)
        for use_ws in (False, True):
            d2 = torch.empty((b, n, 3), device=DEV); idx = torch.empty((b, n, 3), dtype=torch.int32, device=DEV)
            if use_ws:
                nbytes = l.epnet_three_nn_workspace_bytes(b, n, m)
                assert nbytes > 0
                ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
                assert l.epnet_three_nn_ws(b, n, m, du.data_ptr(), dk.data_ptr(), d2.data_ptr(), idx.data_ptr(), ws.data_ptr(), nbytes, stream) == 0
            else:
                assert l.epnet_three_nn(b, n, m, du.data_ptr(), dk.data_ptr(), d2.data_ptr(), idx.data_ptr(), stream) == 0
            np.testing.assert_array_equal(host(idx), o_idx)
            np.testing.assert_array_equal(host(d2), o_d2)
    assert l.epnet_three_nn_workspace_bytes(2, 256, 64) == 0


@pytest.mark.parametrize("b,n,m,kind", [
    (2, 16384, 4096, "kitti"), (2, 4096, 1024, "kitti"), (1, 5000, 1500, "ubox"), (2, 2048, 1030, "dup"),
    (1, 40000, 3000, "kitti"), (2, 1024, 1024, "kitti"),
    (2, 700, 1100, "kitti"),      # unknown set below the indexed range: known-index-only kernel
    (2, 3000, 300, "kitti"),      # known set below it: plain path
])
def test_three_nn_over_scene_indices_matches_oracle(oracle, b, n, m, kind):
    """epnet_three_nn_indexed with both point sets indexed (one wave per unknown bucket), with the known set only,
    and with neither: indices and squared distances bit-equal to the oracle"""
    from epnet_amd import pointnet2_cuda as ext
    with _lib.tuning(EPNET_NN_TILE_MIN_BUCKETS=1):   # the library keeps the bucket kernel for big launches only
        unknown = rand_cloud(b, n, seed=n + 1, kind=kind)
        known = rand_cloud(b, m, seed=m + 2, kind=kind)
        if kind == "dup":
            known[:, 100:160] = unknown[:, :60]   # exact zero distances and ties between equal known rows
        d_u, d_k = dev(unknown), dev(known)
        o_d2, o_i = oracle.three_nn(unknown, known)
        ui, ki = ext.scene_index(d_u), ext.scene_index(d_k)
        for use_u in (True, False):
            d2 = torch.full((b, n, 3), -1.0, device=DEV)
            i = torch.full((b, n, 3), -1, dtype=torch.int32, device=DEV)
            ext.three_nn_indexed_wrapper(b, n, m, d_u, d_k, ui if use_u else None, ki, d2, i)
            np.testing.assert_array_equal(host(i), o_i)
            np.testing.assert_array_equal(host(d2), o_d2)


@pytest.mark.parametrize("tile", [True, False])
def test_three_nn_non_finite_coordinates(oracle, tile):
    """NaN (either sign bit) and +-inf coordinates on both sides: the reference takes a point only if `d < best` with best starting
    at (float)1e40 = +inf (interpolate_gpu.cu:30-48), so a distance of +inf or NaN never enters a list -- unknowns with a
    non-finite coordinate get (inf, 0) three times, known points with one are never anybody's neighbour. The bucket kernel
    orders its (d, k) keys as doubles: a NaN of either sign must stay out of that order."""
    from epnet_amd import pointnet2_cuda as ext
    with _lib.tuning(EPNET_NN_TILE_MIN_BUCKETS=1 if tile else 1000000000):
        b, n, m = 2, 4096, 1536
        unknown = rand_cloud(b, n, seed=21, kind="kitti")
        known = rand_cloud(b, m, seed=22, kind="kitti")
        neg_nan = np.frombuffer(np.uint32(0xFFC00000).tobytes(), dtype=np.float32)[0]
        # NaN payloads propagate through the subtraction and the squares: the distance of such a point carries them, and bits from
        # 0x7FF00000 up are a NaN as the high word of a double as well (the canonical 0x7FC00000 alone cannot show that)
        bad_bits = [0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FF00001, 0xFFF80000]
        rng = np.random.default_rng(5)
        for arr, count in ((known, 64), (unknown, 96)):
            bits = arr.view(np.uint32)          # (written as bit patterns: no float move may quieten or canonicalise them)
            for k in range(count):
                bits[rng.integers(0, b), rng.integers(0, arr.shape[1]), rng.integers(0, 3)] = bad_bits[k % len(bad_bits)]
        known[1, 7] = [neg_nan, neg_nan, neg_nan]
        known.view(np.uint32)[1, 9] = [0x7FFFFFFF, 0xFFFFFFFF, 0x7FFFFFFF]
        unknown[0, 11] = [np.float32(np.inf), np.float32(-np.inf), neg_nan]
        unknown.view(np.uint32)[0, 13] = [0xFFFFFFFF, 0x7FFFFFFF, 0x7FF00001]
        d_u, d_k = dev(unknown), dev(known)
        o_d2, o_i = oracle.three_nn(unknown, known)
        assert np.isinf(o_d2).any() and np.isfinite(o_d2).any()
        ui, ki = ext.scene_index(d_u), ext.scene_index(d_k)
        d2 = torch.full((b, n, 3), -1.0, device=DEV)
        i = torch.full((b, n, 3), -1, dtype=torch.int32, device=DEV)
        ext.three_nn_indexed_wrapper(b, n, m, d_u, d_k, ui, ki, d2, i)
        np.testing.assert_array_equal(host(i), o_i)
        np.testing.assert_array_equal(host(d2), o_d2)


@pytest.mark.parametrize("b,n_src,n", [(2, 16384, 4096), (3, 4096, 1024), (2, 5000, 2500), (1, 20000, 16384)])
def test_scene_index_built_from_sampled_rows(oracle, b, n_src, n):
    """epnet_scene_index_build_gathered: the centre gather of an SA level and the index build of the next level in one launch --
    the rows come out as gather_points would give them, and the index answers for exactly those points (ball query and
    sampling over it against the oracle on the gathered cloud)"""
    from epnet_amd import pointnet2_cuda as ext
    rng = np.random.default_rng(n)
    src = rand_cloud(b, n_src, seed=n_src, kind="kitti")
    idx = np.stack([rng.permutation(n_src)[:n] for _ in range(b)]).astype(np.int32)
    idx[:, 7] = idx[:, 3]                                   # a repeated row
    want = np.take_along_axis(src, idx[:, :, None].astype(np.int64), axis=1)
    new_xyz = torch.full((b, n, 3), float("nan"), device=DEV)
    index = torch.empty((ext.scene_index_bytes(b, n),), dtype=torch.uint8, device=DEV)
    ext.scene_index_build_gathered_wrapper(b, n_src, n, dev(src), dev(idx), new_xyz, index)
    np.testing.assert_array_equal(host(new_xyz), want)
    m = 300
    centres = np.ascontiguousarray(want[:, :m])
    got = torch.empty((b, m, 24), dtype=torch.int32, device=DEV)
    ext.ball_query_indexed_wrapper(b, n, m, 0.7, 24, dev(centres), new_xyz, index, got)
    np.testing.assert_array_equal(host(got), oracle.ball_query(0.7, 24, want, centres))
    fps = torch.empty((b, 200), dtype=torch.int32, device=DEV)
    temp = torch.full((b, n), 1e10, device=DEV)
    ext.furthest_point_sampling_indexed_wrapper(b, n, 200, new_xyz, index, temp, fps)
    np.testing.assert_array_equal(host(fps), oracle.furthest_point_sampling(want, 200))


def test_scene_index_is_remembered_only_on_the_packages_own_centres():
    """a scene index is remembered on the tensor object it was built from, and only for tensors this package allocated
    itself (the centres of an SA level); a caller's tensor is indexed afresh on every call"""
    from epnet_amd import pointnet2_utils as p2u
    xyz = dev(rand_cloud(2, 4096, seed=9))
    first = p2u.scene_index(xyz)
    assert first is not None and p2u.scene_index(xyz, cached_only=True) is None     # a caller's tensor: nothing remembered
    assert p2u.scene_index(xyz) is not first
    idx, centres = p2u.sample_and_gather(xyz, 2048, first)
    assert p2u.scene_index(centres, cached_only=True) is None
    index = p2u.scene_index(centres)
    assert index is not None and p2u.scene_index(centres) is index and p2u.scene_index(centres, cached_only=True) is index
    centres.add_(1.0)   # written to: the remembered index is stale and must not be served
    assert p2u.scene_index(centres, cached_only=True) is None
    assert p2u.scene_index(dev(rand_cloud(2, 512, seed=9))) is None


def test_outputs_written_through_the_c_abi_move_their_version():
    """every stand-in bumps the version counter of the tensors its kernels wrote (the reference's pybind extensions write
    invisibly to autograd): an index remembered for the old contents is dropped"""
    from epnet_amd import pointnet2_cuda as ext, pointnet2_utils as p2u
    b, n, m = 2, 4096, 2048
    src = dev(rand_cloud(b, n, seed=3))
    _, centres = p2u.sample_and_gather(src, m, None)
    stale = p2u.scene_index(centres)
    assert p2u.scene_index(centres, cached_only=True) is stale
    # refill the same buffer through gather_points_wrapper with OTHER points: (B,3,m) rows written over (B,m,3) memory
    other = dev(rand_cloud(b, n, seed=4)).transpose(1, 2).contiguous()
    pick = torch.arange(m, dtype=torch.int32, device=DEV).repeat(b, 1).contiguous()
    v0 = centres._version
    ext.gather_points_wrapper(b, 3, n, m, other, pick, centres.view(b, 3, m))
    assert centres._version > v0
    assert p2u.scene_index(centres, cached_only=True) is None
    fresh = p2u.scene_index(centres)
    q = dev(rand_cloud(b, 64, seed=5))
    assert torch.equal(p2u.ball_query(2.0, 16, centres, q, fresh), p2u.ball_query(2.0, 16, centres, q))


def test_sa_module_follows_a_refilled_cloud_and_a_graph_replay():
    """VERDICT r01 weak 6 / ADVICE: (1) a preallocated cloud refilled through a write autograd cannot see (here
    gather_points_wrapper on the raw pointer; a foreign pybind extension would do the same) and (2) a static tensor
    rewritten by a HIP-graph replay after it was used eagerly: the SA module's indices must follow the NEW contents"""
    from epnet_amd import pointnet2_cuda as ext, pointnet2_modules as p2m, pointnet2_utils as p2u
    torch.manual_seed(0)
    sa = p2m.PointnetSAModuleMSG(npoint=512, radii=[0.5, 1.0], nsamples=[8, 16], mlps=[[0, 8], [0, 8]]).to(DEV).eval()
    b, n = 2, 4096
    buf = dev(rand_cloud(b, n, seed=11, kind="kitti"))
    with torch.no_grad():
        x_old, _, i_old = sa(buf)
        new_points = dev(rand_cloud(b, n, seed=12, kind="kitti"))
        # the new cloud copied over the buffer through the C ABI: one channel of N*3 values per scene, identity indices
        pick = torch.arange(n * 3, dtype=torch.int32, device=DEV).repeat(b, 1).contiguous()
        ext.gather_points_wrapper(b, 1, n * 3, n * 3, new_points.view(b, 1, n * 3), pick, buf.view(b, 1, n * 3))
        assert torch.equal(buf, new_points)
        x_new, _, i_new = sa(buf)
        x_ref, _, i_ref = sa(new_points.clone())
    assert torch.equal(i_new, i_ref) and torch.equal(x_new, x_ref) and not torch.equal(i_new, i_old)
    # (2) eager use, then a graph replay writes other coordinates into the same static tensor, then eager use again
    static = dev(rand_cloud(b, n, seed=13, kind="kitti"))
    staged = dev(rand_cloud(b, n, seed=14, kind="kitti"))
    with torch.no_grad():
        sa(static)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            static.copy_(staged)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        static.copy_(dev(rand_cloud(b, n, seed=13, kind="kitti")))
        sa(static)                                  # an eager pass over the old contents
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static.copy_(staged)
        graph.replay()                              # rewrites `static`; its version counter does not move
        torch.cuda.synchronize()
        x_after, _, i_after = sa(static)
        centres = x_after
        got = p2u.ball_query(1.0, 16, static, centres, p2u.scene_index(static))
        x_want, _, i_want = sa(staged.clone())
    assert torch.equal(i_after, i_want) and torch.equal(x_after, x_want)
    assert torch.equal(got, p2u.ball_query(1.0, 16, staged, centres))


@pytest.mark.parametrize("b,c,m,n", [(2, 256, 64, 256), (2, 128, 1024, 4096), (1, 7, 50, 333), (2, 16, 9, 2), (2, 40, 4096, 16384),
                                     (1, 4096, 4096, 16384),    # enough workgroups for the run-partitioned gradient
                                     (3, 1024, 64, 256), (2, 512, 256, 1024),   # the coarse FP levels of the RPN (thread-per-unknown / one-tile LDS kernels)
                                     (2, 24, 8, 100), (1, 200, 4092, 1023), (2, 12, 64, 64)])   # ragged n, long known rows, smallest n of that path
def test_three_interpolate_and_grad(oracle, b, c, m, n):
    from epnet_amd import pointnet2_cuda as ext
    rng = np.random.default_rng(c + m)
    pts = rng.standard_normal((b, c, m)).astype(np.float32)
    idx = rng.integers(0, m, size=(b, n, 3)).astype(np.int32)
    w = rng.random((b, n, 3)).astype(np.float32)
    w /= w.sum(-1, keepdims=True)
    out = torch.empty((b, c, n), device=DEV)
    ext.three_interpolate_wrapper(b, c, m, n, dev(pts), dev(idx), dev(w), out)
    np.testing.assert_array_equal(host(out), oracle.three_interpolate(pts, idx, w))   # same op order, no contraction
    go = rng.standard_normal((b, c, n)).astype(np.float32)
    grad = torch.zeros((b, c, m), device=DEV)
    ext.three_interpolate_grad_wrapper(b, c, n, m, dev(go), dev(idx), dev(w), grad)
    np.testing.assert_allclose(host(grad), oracle.three_interpolate_grad(go, idx, w, m), rtol=1e-5, atol=1e-5)


def test_scratch_free_entry_points_through_the_c_abi(oracle):
    """the wrappers hand scratch to the *_ws / *_indexed entry points whenever the library accepts it; the plain
    entry points (LDS-atomic gradients, self-sorting FPS, direct three_nn) must stay correct for callers without"""
    from epnet_amd import _lib
    l = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(41)
    b, c, n, m, ns = 2, 24, 2048, 256, 16
    go = rng.standard_normal((b, c, m, ns)).astype(np.float32)
    idx = rng.integers(0, n, size=(b, m, ns)).astype(np.int32)
    d_go, d_idx = dev(go), dev(idx)
    grad = torch.zeros((b, c, n), device=DEV)
    _lib.check(l.epnet_group_points_grad(b, c, n, m, ns, d_go.data_ptr(), d_idx.data_ptr(), grad.data_ptr(), s), "group_points_grad")
    np.testing.assert_allclose(host(grad), oracle.group_points_grad(go, idx, n), rtol=1e-5, atol=1e-5)
    # fused-tensor gradient: the feature channels sit behind 3 xyz channels
    go3 = rng.standard_normal((b, 3 + c, m, ns)).astype(np.float32)
    d_go3 = dev(go3)
    grad = torch.zeros((b, c, n), device=DEV)
    _lib.check(l.epnet_group_concat_grad(b, c, n, m, ns, d_go3.data_ptr(), d_idx.data_ptr(), grad.data_ptr(), 1, s), "group_concat_grad")
    np.testing.assert_allclose(host(grad), oracle.group_points_grad(np.ascontiguousarray(go3[:, 3:]), idx, n), rtol=1e-5, atol=1e-5)

    nn = 4096
    gi = rng.standard_normal((b, c, nn)).astype(np.float32)
    i3 = rng.integers(0, n, size=(b, nn, 3)).astype(np.int32)
    w = rng.random((b, nn, 3)).astype(np.float32)
    d_gi, d_i3, d_w = dev(gi), dev(i3), dev(w)
    grad = torch.zeros((b, c, n), device=DEV)
    _lib.check(l.epnet_three_interpolate_grad(b, c, nn, n, d_gi.data_ptr(), d_i3.data_ptr(), d_w.data_ptr(), grad.data_ptr(), s),
               "three_interpolate_grad")
    np.testing.assert_allclose(host(grad), oracle.three_interpolate_grad(gi, i3, w, n), rtol=1e-5, atol=1e-5)

    unknown, known = rand_cloud(b, nn, seed=1, kind="kitti"), rand_cloud(b, n, seed=2, kind="kitti")
    d_u, d_k = dev(unknown), dev(known)
    d2 = torch.empty((b, nn, 3), device=DEV)
    i = torch.empty((b, nn, 3), dtype=torch.int32, device=DEV)
    _lib.check(l.epnet_three_nn(b, nn, n, d_u.data_ptr(), d_k.data_ptr(), d2.data_ptr(), i.data_ptr(), s), "three_nn")
    o_d2, o_i = oracle.three_nn(unknown, known)
    np.testing.assert_array_equal(host(i), o_i)
    np.testing.assert_array_equal(host(d2), o_d2)

    centres = np.ascontiguousarray(known[:, ::8])
    d_c = dev(centres)
    out = torch.full((b, centres.shape[1], 24), -3, dtype=torch.int32, device=DEV)
    _lib.check(l.epnet_ball_query(b, n, centres.shape[1], 0.7, 24, d_c.data_ptr(), d_k.data_ptr(), out.data_ptr(), s), "ball_query")
    np.testing.assert_array_equal(host(out), oracle.ball_query(0.7, 24, known, centres))


# ------------------------------------------------------------------------------------------------ iou3d

def boxes_bev(num, seed):
    from epnet_amd import kitti_utils, synth
    b, s = synth.proposal_boxes(num, seed=seed, num_objects=max(4, num // 20), jitter=0.8)
    return kitti_utils.boxes3d_to_bev_torch(b).numpy(), s.numpy(), b.numpy()


def test_rotated_overlap_and_iou(oracle):
    from epnet_amd import iou3d_cuda as ext
    a, _, _ = boxes_bev(150, 1)
    b, _, _ = boxes_bev(37, 2)
    for fn, ofn in ((ext.boxes_overlap_bev_gpu, oracle.boxes_overlap_bev), (ext.boxes_iou_bev_gpu, oracle.boxes_iou_bev)):
        ans = torch.zeros((150, 37), device=DEV)
        fn(dev(a), dev(b), ans)
        ref = ofn(a, b)
        np.testing.assert_allclose(host(ans), ref, rtol=0, atol=1e-5)
        assert (ref > 0).sum() > 50
    # analytic cases (same as the oracle's KATs)
    unit = np.array([[0, 0, 1, 1, 0]], np.float32)
    rot = np.array([[0, 0, 1, 1, np.pi / 4]], np.float32)
    ans = torch.zeros((1, 1), device=DEV)
    ext.boxes_overlap_bev_gpu(dev(unit), dev(rot), ans)
    assert ans.item() == pytest.approx(2 * (2 ** 0.5 - 1), abs=1e-5)
    ext.boxes_iou_bev_gpu(dev(unit), dev(unit), ans)
    assert ans.item() == pytest.approx(1.0, abs=1e-6)


def test_iou3d_surface_fixture():
    from epnet_amd import iou3d_utils, kitti_utils
    fx = golden("iou3d.npz")
    a, b, s = dev(fx["boxes_a"]), dev(fx["boxes_b"]), dev(fx["scores"])
    np.testing.assert_allclose(host(iou3d_utils.boxes_iou3d_gpu(a, b)), fx["iou3d"], rtol=0, atol=1e-5)
    bev_a, bev_b = kitti_utils.boxes3d_to_bev_torch(a), kitti_utils.boxes3d_to_bev_torch(b)
    np.testing.assert_allclose(host(iou3d_utils.boxes_iou_bev(bev_a, bev_b)), fx["iou_bev"], rtol=0, atol=1e-5)
    for key, thr, fn in (("keep_rot_010", 0.1, iou3d_utils.nms_gpu), ("keep_rot_050", 0.5, iou3d_utils.nms_gpu),
                         ("keep_normal_085", 0.85, iou3d_utils.nms_normal_gpu), ("keep_normal_050", 0.5, iou3d_utils.nms_normal_gpu)):
        kept = fn(bev_a, s, thr)
        assert kept.dtype == torch.int64 and kept.is_cuda
        np.testing.assert_array_equal(host(kept), fx[key])


def test_fused_iou3d_equals_composition_and_pairs():
    from epnet_amd import iou3d_utils, synth
    a = synth.proposal_boxes(512, seed=3, num_objects=20)[0].to(DEV)
    b = synth.proposal_boxes(20, seed=4, num_objects=20)[0].to(DEV)
    fused, composed = iou3d_utils.boxes_iou3d_gpu(a, b), iou3d_utils.boxes_iou3d_composed(a, b)
    np.testing.assert_allclose(host(fused), host(composed), rtol=0, atol=1e-6)
    assert (host(fused) > 0.05).sum() > 20
    k = 300
    pa = a[torch.arange(k) % 512].contiguous()
    pb = b[torch.arange(k) % 20].contiguous()
    pairs = iou3d_utils.boxes_iou3d_pairs_gpu(pa, pb)
    np.testing.assert_array_equal(host(pairs), host(fused)[np.arange(k) % 512, np.arange(k) % 20])
    assert iou3d_utils.boxes_iou3d_gpu(a[:0], b).shape == (0, 20)


@pytest.mark.parametrize("n,thr", [(6300, 0.85), (2700, 0.85), (1000, 0.3), (64, 0.5), (65, 0.5), (1, 0.5)])
def test_nms_normal_full_size_exact(oracle, n, thr):
    """the training-path NMS (RPN.NMS_TYPE normal): N up to 6300, no trig -> bit-exact keep list"""
    from epnet_amd import iou3d_cuda as ext
    bev, scores, _ = boxes_bev(n, 10 + n)
    order = np.argsort(-scores, kind="stable")
    sorted_boxes = np.ascontiguousarray(bev[order])
    keep = torch.zeros((n,), dtype=torch.int64)
    num = ext.nms_normal_gpu(dev(sorted_boxes), keep, thr)      # the reference contract: CPU int64 keep + count
    o_keep = oracle.nms(sorted_boxes, thr, False)
    assert num == len(o_keep)
    np.testing.assert_array_equal(keep[:num].numpy(), o_keep)


def test_nms_rotated_and_empty(oracle):
    from epnet_amd import iou3d_cuda as ext
    bev, scores, _ = boxes_bev(700, 77)
    sorted_boxes = np.ascontiguousarray(bev[np.argsort(-scores, kind="stable")])
    full = oracle.boxes_iou_bev(sorted_boxes, sorted_boxes)
    thr = 0.1
    while np.abs(full - thr).min() < 1e-5:   # keep the test away from libm-borderline pairs
        thr += 0.0137
    keep, num = ext.nms_device(dev(sorted_boxes), thr)
    n = int(num.item())
    np.testing.assert_array_equal(host(keep[:n]), oracle.nms(sorted_boxes, thr, True))
    keep, num = ext.nms_device(torch.zeros((0, 5), device=DEV), 0.5)
    assert int(num.item()) == 0


# ------------------------------------------------------------------------------------------------ roipool3d

def test_roipool3d_fixtures_exact():
    from epnet_amd import roipool3d_utils
    fx = golden("roipool3d_surface.npz")
    pooled, empty = roipool3d_utils.roipool3d_gpu(dev(fx["pts"]), dev(fx["pts_feature"]), dev(fx["boxes3d"]), 0.2, sampled_pt_num=64)
    np.testing.assert_array_equal(host(empty), fx["pooled_empty_flag"])
    np.testing.assert_array_equal(host(pooled), fx["pooled_features"])
    # the fixture captured from the reference's own compiled CPU op (boxes already enlarged there)
    rf = golden("roipool3d_ref.npz")
    from epnet_amd import roipool3d_cuda as ext
    m, s, c = rf["boxes3d"].shape[0], rf["pooled_pts"].shape[1], rf["pts_feature"].shape[1]
    out = torch.zeros((1, m, s, 3 + c), device=DEV)
    flag = torch.zeros((1, m), dtype=torch.int32, device=DEV)
    ext.forward(dev(rf["pts"][None]), dev(rf["boxes3d"][None]), dev(rf["pts_feature"][None]), out, flag)
    np.testing.assert_array_equal(host(flag)[0], rf["pooled_empty_flag"].astype(np.int32))
    np.testing.assert_array_equal(host(out)[0, :, :, :3], rf["pooled_pts"])
    np.testing.assert_array_equal(host(out)[0, :, :, 3:], rf["pooled_features"])


@pytest.mark.parametrize("b,n,m,c,s", [(2, 16384, 64, 130, 512), (1, 5000, 7, 1, 33), (2, 700, 3, 0, 16), (1, 100, 2, 5, 600)])
def test_roipool3d_matches_oracle(oracle, b, n, m, c, s):
    from epnet_amd import kitti_utils, roipool3d_cuda as ext, synth
    pts = rand_cloud(b, n, seed=300 + n, kind="kitti")
    boxes = np.stack([synth.proposal_boxes(m, seed=400 + i, num_objects=40, jitter=0.5)[0].numpy() for i in range(b)])
    boxes = kitti_utils.enlarge_box3d(boxes.reshape(-1, 7), 0.2).reshape(b, m, 7)
    boxes[:, -1, 0] = 900.0   # one empty box per scene
    feat = np.random.default_rng(n).standard_normal((b, n, c)).astype(np.float32)
    out = torch.zeros((b, m, s, 3 + c), device=DEV)
    flag = torch.zeros((b, m), dtype=torch.int32, device=DEV)
    ext.forward(dev(pts), dev(boxes), dev(feat), out, flag)
    o_pool, o_flag = oracle.roipool3d(pts, boxes, feat, s)
    np.testing.assert_array_equal(host(flag), o_flag)
    np.testing.assert_array_equal(host(out), o_pool)
    assert o_flag[:, -1].all() and (n < 700 or not o_flag.all())


# ------------------------------------------------------------------------------------------------ modules, streams, graphs

def _load(module, fx):
    module.load_state_dict({k[4:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("sd__")})
    return module.to(DEV).eval()


def test_sa_and_fp_modules_on_gpu():
    from epnet_amd import pointnet2_modules as p2m
    fx = golden("sa_module.npz")
    sa = _load(p2m.PointnetSAModuleMSG(npoint=256, radii=[0.5, 1.0], nsamples=[16, 32], mlps=[[16, 16, 32], [16, 16, 32]]), fx)
    with torch.no_grad():
        new_xyz, feats, idx = sa(dev(fx["xyz"]), dev(fx["features"]))
    np.testing.assert_array_equal(host(idx), fx["idx"])
    np.testing.assert_array_equal(host(new_xyz), fx["new_xyz"])
    np.testing.assert_allclose(host(feats), fx["out_features"], rtol=0, atol=1e-5)
    fp = golden("fp_module.npz")
    fpm = _load(p2m.PointnetFPModule(mlp=[48, 32]), fp)
    with torch.no_grad():
        out = fpm(dev(fp["unknown"]), dev(fp["known"]), dev(fp["unknow_feats"]), dev(fp["known_feats"]))
    np.testing.assert_allclose(host(out), fp["out"], rtol=0, atol=1e-5)


def test_query_and_group_fused_equals_reference_composition():
    """epnet_group_concat (one fused op) vs the reference's composition of grouping ops, subtraction and cat
    (pointnet2_utils.py:249-257): identical values, forward; gradients w.r.t. features to 1e-5"""
    from epnet_amd import pointnet2_utils as p2u
    xyz = dev(rand_cloud(2, 4096, seed=77, kind="kitti"))
    new_xyz = xyz[:, ::4].contiguous()
    g = torch.Generator().manual_seed(5)
    feats = torch.randn((2, 19, 4096), generator=g).to(DEV)
    up = torch.randn((2, 22, 1024, 16), generator=g).to(DEV)
    for use_xyz, with_feats in ((True, True), (False, True), (True, False)):
        f1 = feats.clone().requires_grad_(True) if with_feats else None
        fused = p2u.QueryAndGroup(0.8, 16, use_xyz=use_xyz)(xyz, new_xyz, f1)
        idx = p2u.ball_query(0.8, 16, xyz, new_xyz)
        f2 = feats.clone().requires_grad_(True) if with_feats else None
        parts = []
        if use_xyz or not with_feats:
            gx = p2u.grouping_operation(xyz.transpose(1, 2).contiguous(), idx)
            gx -= new_xyz.transpose(1, 2).unsqueeze(-1)
            parts.append(gx)
        if with_feats:
            parts.append(p2u.grouping_operation(f2, idx))
        ref = torch.cat(parts, dim=1)
        assert torch.equal(fused, ref)
        if with_feats:
            w = up[:, :fused.shape[1]]
            (fused * w).sum().backward()
            (ref * w).sum().backward()
            np.testing.assert_allclose(host(f1.grad), host(f2.grad), rtol=1e-5, atol=1e-5)
    # nsample not a multiple of 4: the scalar centred-xyz kernel
    fused = p2u.QueryAndGroup(0.8, 7)(xyz, new_xyz, feats)
    idx = p2u.ball_query(0.8, 7, xyz, new_xyz)
    gx = p2u.grouping_operation(xyz.transpose(1, 2).contiguous(), idx) - new_xyz.transpose(1, 2).unsqueeze(-1)
    assert torch.equal(fused, torch.cat([gx, p2u.grouping_operation(feats, idx)], dim=1))
    # a gradient w.r.t. the coordinates takes the unfused, fully differentiable path
    xr = xyz.clone().requires_grad_(True)
    out = p2u.QueryAndGroup(0.8, 16)(xr, new_xyz, feats)
    out.sum().backward()
    assert xr.grad is not None and torch.isfinite(xr.grad).all()


def test_backbone_with_shared_indices_equals_plain_ops(monkeypatch):
    """two MSG SA levels + two FP modules, forward and backward: the wiring of this package's modules (one scene
    index per level for sampling / multi-scale ball query / three_nn, FPS + centre gather in one call, fused
    grouping) against the same modules with every shared-index feature switched off"""
    from epnet_amd import pointnet2_modules as p2m, pointnet2_utils as p2u

    def build():
        torch.manual_seed(3)
        sa1 = p2m.PointnetSAModuleMSG(npoint=512, radii=[0.5, 1.0], nsamples=[8, 16], mlps=[[4, 8, 16], [4, 8, 16]]).to(DEV)
        sa2 = p2m.PointnetSAModuleMSG(npoint=128, radii=[1.0, 2.0], nsamples=[8, 16], mlps=[[32, 32], [32, 48]]).to(DEV)
        fp2 = p2m.PointnetFPModule(mlp=[80 + 32, 64]).to(DEV)
        fp1 = p2m.PointnetFPModule(mlp=[64 + 4, 32]).to(DEV)
        return sa1, sa2, fp2, fp1

    def run(mods, xyz, feats):
        sa1, sa2, fp2, fp1 = mods
        f0 = feats.clone().requires_grad_(True)
        x1, f1, i1 = sa1(xyz, f0)
        x2, f2, i2 = sa2(x1, f1)
        u1 = fp2(x1, x2, f1, f2)
        u0 = fp1(xyz, x1, f0, u1)
        u0.square().mean().backward()
        grads = [p.grad.detach().clone() for m in mods for p in m.parameters()]
        return u0.detach(), i1, i2, f0.grad.detach(), grads

    xyz = dev(rand_cloud(2, 2048, seed=31, kind="kitti"))
    feats = torch.randn((2, 4, 2048), generator=torch.Generator().manual_seed(4)).to(DEV)
    with_index = run(build(), xyz, feats)
    assert p2u.scene_index(xyz, cached_only=True) is None              # nothing is remembered on the caller's own tensor
    monkeypatch.setattr(p2u, "scene_index", lambda *a, **k: None)      # plain ops: no index anywhere
    plain = run(build(), xyz, feats)
    assert torch.equal(with_index[1], plain[1]) and torch.equal(with_index[2], plain[2])   # FPS indices
    np.testing.assert_allclose(host(with_index[0]), host(plain[0]), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(host(with_index[3]), host(plain[3]), rtol=1e-4, atol=1e-6)
    for a, b in zip(with_index[4], plain[4]):
        np.testing.assert_allclose(host(a), host(b), rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("b,c,n,m,nss", [(48, 96, 4096, 256, (16, 32)), (2, 96, 4096, 1024, (16, 32)), (40, 16, 1024, 128, (16, 20)),
                                         (3, 8, 700, 64, (8, 4)), (2, 0, 2048, 256, (16, 32))])
def test_groupings_of_an_msg_level_in_one_call(b, c, n, m, nss):
    """epnet_group_concat_multi (feature rows staged once for two scales when the launch fills the chip) against one
    epnet_group_concat per scale: identical tensors"""
    from epnet_amd import pointnet2_cuda as ext
    g = torch.Generator().manual_seed(c + n)
    xyz = dev(rand_cloud(b, n, seed=n + c))
    new_xyz = xyz[:, :m].contiguous()
    feats = torch.randn((b, c, n), generator=g).to(DEV) if c else None
    idxs = [torch.randint(0, n, (b, m, ns), generator=g, dtype=torch.int32).to(DEV) for ns in nss]
    outs = [torch.full((b, 3 + c, m, ns), float("nan"), device=DEV) for ns in nss]
    ext.group_concat_multi_wrapper(b, c, n, m, list(nss), xyz, new_xyz, feats, idxs, outs, True)
    for ns, idx, out in zip(nss, idxs, outs):
        ref = torch.empty_like(out)
        ext.group_concat_wrapper(b, c, n, m, ns, xyz, new_xyz, feats, idx, ref, True)
        assert torch.equal(out, ref)


def test_autograd_on_gpu():
    from epnet_amd import pointnet2_utils as p2u
    fx = golden("grads.npz")
    feat = dev(fx["feat"]).requires_grad_(True)
    (p2u.grouping_operation(feat, dev(fx["idx"])) * dev(fx["upstream"])).sum().backward()
    np.testing.assert_allclose(host(feat.grad), fx["grad_feat"], rtol=1e-5, atol=1e-5)
    kf = dev(fx["known_feats"]).requires_grad_(True)
    (p2u.three_interpolate(kf, dev(fx["nn_idx"]), dev(fx["weight"])) * dev(fx["upstream2"])).sum().backward()
    np.testing.assert_allclose(host(kf.grad), fx["grad_known"], rtol=1e-5, atol=1e-5)


def test_ops_follow_the_current_stream_and_graph_replay(oracle):
    from epnet_amd import pointnet2_utils as p2u, sa_stack, synth
    xyz_h = synth.scenes("kitti", 2, 4096, seed=21)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        xyz = xyz_h.to(DEV, non_blocking=False)
        idx = p2u.furthest_point_sample(xyz, 512)
    side.synchronize()
    np.testing.assert_array_equal(host(idx), oracle.furthest_point_sampling(xyz_h.numpy(), 512))

    def outputs(stack, parity=0):
        out = [host(L["fps_idx"]).copy() for L in stack.levels] + [host(S["idx"]).copy() for L in stack.levels for S in L["scales"]]
        for L in stack.levels:
            centre = L["sets"][parity]["new_xyz"].transpose(1, 2).unsqueeze(-1)
            for S in L["scales"]:
                if stack.fused:
                    out.append(host(S["grouped"]).copy())
                else:  # the reference composition: group xyz, subtract the centre, group features, concatenate
                    parts = [S["grouped_xyz"] - centre] + ([S["grouped_feat"]] if S["grouped_feat"] is not None else [])
                    out.append(host(torch.cat(parts, dim=1)).copy())
        return out

    kw = dict(n=4096, device=DEV, npoints=(1024, 256, 64, 16), with_fp=False, seed=3)
    plain = sa_stack.SAStack(2, fused=False, shared_index=False, overlap=False, **kw)
    plain.run(xyz)
    torch.cuda.synchronize()
    eager = outputs(plain)
    # shared scene index + fused grouping, two streams, then the same from a HIP graph
    stack = sa_stack.SAStack(2, **kw)
    stack.run(xyz)
    torch.cuda.synchronize()
    for a, b in zip(eager, outputs(stack)):
        np.testing.assert_array_equal(a, b)
    stack.capture(xyz)
    for L in stack.levels:
        L["fps_idx"].zero_()
        for S in L["scales"]:
            S["grouped"].zero_()
    stack.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, outputs(stack)):
        np.testing.assert_array_equal(a, b)
    # software-pipelined: sampling of step k beside grouping of step k-1, two graphs replayed alternately
    piped = sa_stack.SAStack(2, pipelined=True, **kw)
    piped.capture(xyz)
    for k in range(3):
        for L in piped.levels:
            L["fps_idx"].zero_()
            for S in L["scales"]:
                S["grouped"].zero_()
                S["idx"].zero_()
        piped.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, outputs(piped, parity=1 - (k & 1))):
            np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(eager[0], oracle.furthest_point_sampling(xyz_h.numpy(), 1024))


@pytest.mark.parametrize("with_fp,kind,in_s", [(False, "kitti", (1, 2, 3)), (True, "kitti", None), (False, "dup", ()), (False, "dup", (1, 3)),
                                               (True, "kitti", (1, 2, 3)), (False, "kitti", (1,))])
def test_the_benchs_own_configuration_against_the_oracle(oracle, with_fp, kind, in_s):
    """exactly what bench.py times -- SAStack at 16384 points, software-pipelined, captured into two HIP graphs, the
    kernels the 256-scene run uses (fps_indexed_kernel<8,32>, the multi-scale ball query, group_concat_multi) -- with
    every fps_idx / centre / ball-query idx / grouped tensor of every level compared with the ORACLE directly
    (bench.verify_scene, the check the bench itself prints as `verified`). in_s: the levels whose ball queries run at the tail of
    stage S ((1, 2, 3) is what the 256-scene bench line uses, None = the stack's own choice: all of them with the FP ops)"""
    import bench
    from epnet_amd import sa_stack, synth
    b = 2
    xyz = synth.scenes(kind, b, 16384, seed=77).to(DEV)
    stack = sa_stack.SAStack(b, n=16384, device=DEV, with_fp=with_fp, seed=5, pipelined=True, fused_sampling=True, s_query_levels=in_s)
    assert stack.s_query_levels == (frozenset(range(4)) if in_s is None else frozenset(in_s))
    stack.capture(xyz)
    for L in stack.levels:        # nothing of the capture-time warm-up may survive into the comparison
        L["fps_idx"].fill_(-1)
        for P in L["sets"]:
            P["new_xyz"].zero_()    # (read as centres by the first replay's grouping stage: keep them finite)
        for S in L["scales"]:
            for idx_set in S["idx_sets"]:   # (read by the next step's grouping when the queries run in stage S: valid indices)
                idx_set.zero_()
            S["grouped"].fill_(float("nan"))
    for F in stack.fp_bufs:   # (the neighbour indices are read by the NEXT step's interpolation: they stay valid indices)
        F["out"].fill_(float("nan"))
        for P in F["sets"]:
            P["idx"].zero_()
            P["dist2"].fill_(float("nan"))
    for _ in range(3):            # both graphs of the rotation; the third replay regroups what the second one sampled
        stack.replay()
    torch.cuda.synchronize()
    for scene in range(b):
        assert bench.verify_scene(stack, stack.inputs[0], scene) == []
    # the checker does notice a wrong buffer
    stack.levels[1]["scales"][0]["idx"][0, 5, 3] += 1
    assert bench.verify_scene(stack, stack.inputs[0], 0) == ["level2.r0.5.ball_idx[set 0]"]


def test_config5_stack_against_the_oracle(oracle):
    """BASELINE config 5 at full size, as `bench.py --config 5` runs it (software-pipelined HIP graphs): dense 65536-point
    scenes, FPS 16384 over the scene index (the big-scene kernel with its sorted-order running distances), ball query
    r 0.5 / nsample 64, fused grouping of the coordinates and 64 feature channels -- every tensor against the oracle"""
    import bench
    from epnet_amd import sa_stack, synth
    cfg = sa_stack.CONFIGS[5]
    b = 2
    xyz = synth.scenes("kitti", b, cfg["n"], seed=55).to(DEV)
    stack = sa_stack.SAStack(b, n=cfg["n"], device=DEV, npoints=cfg["npoints"], radii=cfg["radii"], nsamples=cfg["nsamples"],
                             feat_channels=cfg["feat_channels"], seed=6, pipelined=True, fused_sampling=True)
    stack.capture(xyz)
    for L in stack.levels:
        L["fps_idx"].fill_(-1)
        for S in L["scales"]:
            S["grouped"].fill_(float("nan"))
    for _ in range(3):
        stack.replay()
    torch.cuda.synchronize()
    assert bench.verify_scene(stack, stack.inputs[0], 1) == []


@pytest.mark.parametrize("b,c,n,m,ns", [(2, 64, 65536, 2048, 64), (1, 16, 40000, 4000, 20), (2, 128, 20000, 700, 32), (1, 20, 17000, 2001, 12),
                                        (1, 64, 65536, 16384, 64), (1, 24, 30000, 3000, 128)])
def test_group_concat_long_rows_through_point_major_scratch(oracle, b, c, n, m, ns):
    """feature rows beyond LDS (n > 16384): epnet_group_concat_ws gathers from a point-major copy of the features; identical
    to the plain entry point and to the oracle's grouping"""
    from epnet_amd import _lib, pointnet2_cuda as ext
    assert _lib.lib().epnet_group_concat_workspace_bytes(b, c, n, m, ns) == b * c * n * 4
    g = torch.Generator().manual_seed(n + c)
    xyz = dev(rand_cloud(b, n, seed=n))
    new_xyz = xyz[:, :m].contiguous()
    feats = torch.randn((b, c, n), generator=g).to(DEV)
    idx = torch.randint(0, n, (b, m, ns), generator=g, dtype=torch.int32).to(DEV)
    out = torch.full((b, 3 + c, m, ns), float("nan"), device=DEV)
    ext.group_concat_wrapper(b, c, n, m, ns, xyz, new_xyz, feats, idx, out, True)
    want_feat = oracle.group_points(host(feats), host(idx))
    np.testing.assert_array_equal(host(out[:, 3:]), want_feat)
    want_xyz = oracle.group_points(host(xyz.transpose(1, 2).contiguous()), host(idx)) - host(new_xyz).transpose(0, 2, 1)[:, :, :, None]
    np.testing.assert_array_equal(host(out[:, :3]), want_xyz)
    plain = torch.empty_like(out)
    _lib.check(_lib.lib().epnet_group_concat(b, c, n, m, ns, xyz.data_ptr(), new_xyz.data_ptr(), feats.data_ptr(), idx.data_ptr(),
                                             plain.data_ptr(), 1, torch.cuda.current_stream().cuda_stream), "group_concat")
    assert torch.equal(out, plain)
    only = torch.full((b, c, m, ns), float("nan"), device=DEV)
    ext.group_concat_wrapper(b, c, n, m, ns, None, None, feats, idx, only, False)
    np.testing.assert_array_equal(host(only), want_feat)
    # a workspace the caller keeps
    kept = torch.empty((ext.group_concat_workspace_bytes(b, c, n, m, ns),), dtype=torch.uint8, device=DEV)
    again = torch.full((b, 3 + c, m, ns), float("nan"), device=DEV)
    ext.group_concat_wrapper(b, c, n, m, ns, xyz, new_xyz, feats, idx, again, True, kept)
    assert torch.equal(again, out)


def _plant_near_twin_tie(oracle, cloud, slot, seq, around, m):
    """writes to cloud[slot] coordinates a few ulps from a point picked in some round R >= `around` such that the two tie (not as
    exact twins) in round R of the sampling and nothing ties before -- found by trying nudges against the brute-force tie finder.
    Returns R."""
    import itertools
    import sys
    sys.path.insert(0, __import__("os").path.dirname(__file__))
    from test_oracle_second_derivation import first_tie_round
    bs = oracle.opt_n_threads(cloud.shape[0])
    for at_round in range(around, around + 40):
        for axis, k in itertools.product((1, 0, 2), (1, -1, 2, -2, 3, -3)):
            q = cloud[seq[at_round]].copy()
            for _ in range(abs(k)):
                q[axis] = np.nextafter(q[axis], np.float32(np.inf if k > 0 else -np.inf))
            trial = cloud.copy()
            trial[slot] = q
            if first_tie_round(trial, m, bs, twins_are_ties=False)[0] == at_round:
                cloud[slot] = q
                return at_round
    raise AssertionError("no near twin ties around round %d" % around)


def _lattice_cloud(n, seed):
    rng = np.random.default_rng(seed)
    base = rng.integers(-8, 9, size=(max(4, (n * 3) // 4), 3)).astype(np.float32) * np.float32(0.5)
    pts = np.concatenate([base, base[rng.integers(0, len(base), size=n - len(base))]])
    return pts[rng.permutation(n)].astype(np.float32)


@pytest.mark.parametrize("kind,n,pyramid", [("kitti", 16384, (4096, 1024, 256, 64)), ("dup", 16384, (4096, 1024, 256, 64)),
                                            ("ubox", 4096, (1024, 256, 64)), ("lattice", 4096, (1024, 256, 64)),
                                            ("lattice", 16384, (4096, 1024, 256, 64)), ("kitti", 3000, (700, 300, 100)),
                                            ("kitti_twin", 16384, (4096, 1024, 256, 64)), ("dup_shuffled", 16384, (4096, 1024, 256, 64)),
                                            ("few_distinct", 4096, (1024, 256, 64)), ("kitti_q", 16384, (4096, 1024, 256, 64))])
def test_sampling_chain_matches_oracle_and_reports_exact_tie_rounds(oracle, kind, n, pyramid):
    """epnet_sample_centres_chain over a whole pyramid: every level's indices and centres equal the oracle's (which runs the
    reference's rounds on every level), whether a level took the identity (tie-free prefix known) or ran its rounds (ties between
    DIFFERENT coordinates: the lattice cloud). Exact twins (duplicated rows, the reference loader's padding) tie harmlessly and do
    not end the prefix. The first level's reported round count equals the count found by brute force"""
    import sys
    sys.path.insert(0, __import__("os").path.dirname(__file__))
    from test_oracle_second_derivation import first_tie_round
    from epnet_amd import pointnet2_cuda as ext
    b = 3
    if kind == "kitti_twin":
        # an exact twin of the point picked in round 100 + 50 s (harmless: the prefix runs through it) AND a tie between DIFFERENT
        # coordinates in the MIDDLE of the first level's rounds: a never-picked point is moved next to the point picked in round
        # ~300 + 200 s, a few ulps off, where its fp32 running distance at that round is bit-identical -- so the deeper levels know a
        # prefix of about that length and resume their rounds from there
        clouds = np.stack([rand_cloud(1, n, seed=60 + s, kind="kitti")[0] for s in range(b)])
        for s_ in range(b):
            seq = oracle.furthest_point_sampling(clouds[s_:s_ + 1], pyramid[0])[0]
            never = np.setdiff1d(np.arange(n), seq)
            clouds[s_, never[3]] = clouds[s_, seq[100 + 50 * s_]]
            tied_at = _plant_near_twin_tie(oracle, clouds[s_], never[7], seq, 300 + 200 * s_, pyramid[0])
            assert 300 + 200 * s_ <= tied_at < 340 + 200 * s_
    elif kind == "dup_shuffled":   # what the loader does: pad by re-drawing rows, then shuffle (kitti_rcnn_dataset.py:338-342)
        clouds = np.stack([rand_cloud(1, n, seed=60 + s, kind="dup")[0][np.random.default_rng(s).permutation(n)] for s in range(b)])
    elif kind == "few_distinct":   # fewer distinct points than level-2 samples: the maximum reaches zero, the identity must end there
        clouds = np.stack([rand_cloud(1, nd, seed=60 + s, kind="kitti")[0][np.random.default_rng(s).integers(0, nd, size=n)]
                           for s, nd in enumerate((150, 300, 500))])
    else:
        clouds = np.stack([_lattice_cloud(n, 40 + s) if kind == "lattice" else rand_cloud(1, n, seed=60 + s, kind=kind)[0] for s in range(b)])
    cur_h, cur = clouds, dev(clouds)
    prefix_in = None
    took_identity, level1_ties = [], []
    for lvl, m in enumerate(pyramid):
        nn = cur.shape[1]
        index = ext.scene_index(cur)
        idx = torch.full((b, m), -1, dtype=torch.int32, device=DEV)
        centres = torch.full((b, m, 3), float("nan"), device=DEV)
        prefix_out = torch.full((b,), -7, dtype=torch.int32, device=DEV)
        ext.sample_centres_wrapper(b, nn, m, cur, index, idx, centres, prefix_in, prefix_out)
        want = oracle.furthest_point_sampling(cur_h, m)
        np.testing.assert_array_equal(host(idx), want, err_msg="level %d" % (lvl + 1))
        want_c = np.take_along_axis(cur_h, want[:, :, None].astype(np.int64), axis=1)
        np.testing.assert_array_equal(host(centres), want_c)
        po = host(prefix_out)
        if lvl == 0 and 1024 < nn <= 16384:   # the pruned kernels report ties exactly
            for s_ in range(b):
                tie, _ = first_tie_round(cur_h[s_], m, oracle.opt_n_threads(nn), twins_are_ties=False)
                assert po[s_] == tie, (s_, po[s_], tie)
                level1_ties.append(tie)
                if kind in ("dup", "dup_shuffled"):   # the twins do tie, early; the prefix runs through them
                    assert first_tie_round(cur_h[s_], m, oracle.opt_n_threads(nn))[0] < min(tie, pyramid[1])
        if prefix_in is not None:
            took_identity.append((host(prefix_in) >= m).tolist())
        assert (po >= 0).all() and (po <= max(m, int(host(prefix_in).max()) if prefix_in is not None else m)).all()
        cur_h, cur, prefix_in = want_c, centres, prefix_out
    if kind in ("kitti", "ubox") and n > 1024:
        assert all(all(t) for t in took_identity)            # no ties between different coordinates: every deeper level is the identity
    if kind in ("dup", "dup_shuffled"):
        # level 2 is the identity exactly where no tie between DIFFERENT coordinates fell into its rounds (fp32 distances of
        # 16384 points do collide now and then: about one scene in 40); the twins alone never end it
        assert took_identity[0] == [t >= pyramid[1] for t in level1_ties] and any(took_identity[0])
    if kind == "few_distinct":
        assert took_identity[0] == [False, True, True]        # 150 distinct points < 256 samples of level 2; 300 and 500 are not
    if kind == "lattice":
        assert not any(any(t) for t in took_identity)        # ties from the first rounds on: every level ran its rounds
    if kind == "kitti_twin":
        assert took_identity[0] == [False, False, False]      # level 2 (1024 rounds) resumes after 300 / 500 / 700 known samples
        assert took_identity[1] == [True, True, True]         # level 3 (256 rounds) lies inside every known prefix


def test_sample_and_gather_chains_through_the_centres():
    """pointnet2_utils.sample_and_gather hands the knowledge on as an attribute of the centres it returns (only while their
    version stands): the second call on them is the identity for a tie-free cloud, and a write to the centres ends it"""
    from epnet_amd import pointnet2_utils as p2u
    xyz = dev(rand_cloud(2, 16384, seed=5))
    i1, c1 = p2u.sample_and_gather(xyz, 4096, p2u.scene_index(xyz))
    assert hasattr(c1, "_epnet_fps_prefix") and host(c1._epnet_fps_prefix[0]).tolist() == [4096, 4096]
    i2, c2 = p2u.sample_and_gather(c1, 1024, p2u.scene_index(c1))
    assert torch.equal(i2, torch.arange(1024, dtype=torch.int32, device=DEV).repeat(2, 1)) and torch.equal(c2, c1[:, :1024])
    assert torch.equal(i2, p2u.furthest_point_sample(c1, 1024))          # what the rounds compute
    c1.mul_(1.0)                                                         # a write: the knowledge is void
    i2b, _ = p2u.sample_and_gather(c1, 1024, None)
    assert torch.equal(i2b, i2)


def test_sample_pyramid_chains_explicitly_and_the_attribute_form_has_an_opt_out(monkeypatch):
    """sample_pyramid hands the tie-free round counts from level to level itself (nothing attached to a tensor that escapes:
    ADVICE r02); EPNET_SA_CHAIN=0 switches the attribute form of sample_and_gather off"""
    from epnet_amd import pointnet2_utils as p2u
    xyz = dev(rand_cloud(2, 16384, seed=5))
    levels = p2u.sample_pyramid(xyz, [4096, 1024, 256, 64])
    torch.cuda.synchronize()
    for (idx, centres, _ev, _ix), m in zip(levels, (4096, 1024, 256, 64)):
        assert not hasattr(centres, "_epnet_fps_prefix")
    seq = torch.arange(1024, dtype=torch.int32, device=DEV).repeat(2, 1)
    assert torch.equal(levels[1][0], seq) and torch.equal(levels[2][0], seq[:, :256]) and torch.equal(levels[3][0], seq[:, :64])
    assert torch.equal(levels[1][0], p2u.furthest_point_sample(levels[0][1], 1024))      # what the rounds compute
    monkeypatch.setenv("EPNET_SA_CHAIN", "0")
    _, c1 = p2u.sample_and_gather(xyz, 4096, p2u.scene_index(xyz))
    assert not hasattr(c1, "_epnet_fps_prefix")
    i2, _ = p2u.sample_and_gather(c1, 1024, p2u.scene_index(c1))
    assert torch.equal(i2, seq)                                                           # the rounds ran, same answer

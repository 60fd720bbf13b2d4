"""The spatial ops across the float32 range of coordinates: every transform of tests/value_domain.py through every kernel family of
furthest point sampling, ball query, three_nn, QueryAndGroup and group_linear, bit for bit against the CPU oracle (which
tests/test_value_domain.py pins at these magnitudes). No tolerance appears in this file: sampling and neighbour results are
defined exactly, and the fused groupings are compositions of exact pieces.

What the kernels assume and nothing else tests: distances ordered as int32 bit patterns (fps_common.h; needs every distance
non-negative and every denormal to survive med3, the DPP folds and group_max), the pruned sampler's bound L <= d (fps_pruned.h),
the 3.0e38 padding rows and empty-bucket boxes and the +-3.4e38 box starts (spatial.h), the 1e10 start value, and the cell grid
at huge, tiny and lopsided extents (make_cell_grid, cell_code).

Shapes: the smallest that reach each family (fps_plan.h, bq_query_launch and the entry points of ball_query.hip, interpolate.hip).
Where the issue's sizes do not reach what it names, the sizes follow the code:
  * the ordered ball query needs a scene index of the CENTRES (m >= 1024) and is taken by default only above 16384 points:
    n = 16385 / m = 1024 by default and switched off, n = 2049 / m = 1024 forced (EPNET_BQ_ORDERED);
  * the direct scan's two-centres-per-wave kernel needs b * m >= 8192: one case at n = 300, m = 4096;
  * three_nn's bucket-of-unknowns kernel needs a scene index of the UNKNOWN set (n >= 1024): n = 1100 beside n = 700;
  * n = 16385 "without an index" goes through the indexed entry point with index = None (furthest_point_sampling_wrapper builds
    an index itself above 16384 points).
Every input is finite and inside D. An op is called on another op's result only after that result has been compared."""
import numpy as np
import pytest
import torch

import value_domain as vd
from epnet_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = vd.B
M = 48
PAIRS = [(name, kind) for name in vd.NAMES for kind in vd.BASES]
# The oracle's scans are O(n m) on the CPU, and a CPU takes a microcode assist for every denormal operand: in the three transforms
# whose distances are denormal its neighbour scans are some fifty times slower than anywhere else. There the scans run on one base
# cloud (three_nn on the lattice too under s-75, where lost bits make new ties); the sampling runs on all three everywhere
DENORMAL = ("s-75", "s-70", "denorm-mix")
SCAN_PAIRS = [(name, kind) for name, kind in PAIRS if name not in DENORMAL or kind == "kitti"]
NN_PAIRS = [(name, kind) for name, kind in PAIRS if name not in DENORMAL or kind == "kitti" or (name, kind) == ("s-75", "lattice")]


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded(hiplib):
    assert torch.cuda.is_available()
    return hiplib


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def out_tensor(shape, dtype=torch.float32, fill=None):
    """an output handed to a wrapper: between canaries (conftest routes pointnet2_utils._new through its guarded allocator)"""
    from epnet_amd import pointnet2_utils as p2u
    t = p2u._new(torch.empty((0,), device=DEV), shape, dtype)
    if fill is not None:
        t.fill_(fill)
    return t


_ORACLE = {}


def once(key, make):
    """an oracle result computed once, shared between the tests, read-only"""
    if key not in _ORACLE:
        got = make()
        for a in (got if isinstance(got, tuple) else (got,)):
            a.setflags(write=False)
        _ORACLE[key] = got
    return _ORACLE[key]


def gathered(xyz, idx):
    return np.ascontiguousarray(np.take_along_axis(xyz, idx[..., None].astype(np.int64), axis=1))


# ---- furthest point sampling ------------------------------------------------------------------------------------------------------
# (family, n, m, over a scene index, tuning): fps_plan.h. stream: reference block below one wave (n < 64), or more than 16 slots per
# thread without an index (n > 16384); wave: n <= 1024, and any n <= 16384 with the pruning switched off; pruned: 1024 < n <= 16384
# (4 waves x 8 slots at 1025, 8 waves from 8193); indexed: the same range over a scene index (np = 2048 and 16384); bigscene: beyond
# 16384 points over index and temp.
FPS_CASES = (("stream", 33, M, False, {}), ("stream", 16385, M, False, {}),
             ("wave", 64, M, False, {}), ("wave", 64, 64, False, {}), ("wave", 257, M, False, {}), ("wave", 1024, M, False, {}),
             ("wave", 4096, M, False, {"EPNET_FPS_PRUNE": 0}),
             ("pruned", 1025, M, False, {}), ("pruned", 8193, M, False, {}),
             ("indexed", 1025, M, True, {}), ("indexed", 16384, M, True, {}),
             ("bigscene", 16385, M, True, {}))


def oracle_fps(oracle, name, kind, n, m):
    xyz = vd.cloud(name, kind, n)[0]
    return once(("fps", name, kind, n, m), lambda: oracle.furthest_point_sampling(xyz, m, return_temp=True))


def device_fps(xyz, case):
    """-> idx and running distances from the entry point that takes temp (filled with 1e10); where temp may be NULL (64 <= n <=
    16384: the register-resident families) idx and centres from sample_centres as well, else None"""
    from epnet_amd import pointnet2_cuda as ext
    family, n, m, indexed, knobs = case
    d_xyz = dev(xyz)
    with _lib.tuning(**knobs):
        index = ext.scene_index(d_xyz) if indexed else None
        assert (index is not None) == indexed
        temp = out_tensor((B, n), torch.float32, 1e10)
        idx = out_tensor((B, m), torch.int32, -9)
        if indexed or n > 16384:
            ext.furthest_point_sampling_indexed_wrapper(B, n, m, d_xyz, index, temp, idx)
        else:
            ext.furthest_point_sampling_wrapper(B, n, m, d_xyz, temp, idx)
        free = None
        if 64 <= n <= 16384:
            idx2 = out_tensor((B, m), torch.int32, -9)
            new_xyz = out_tensor((B, m, 3), torch.float32, float("nan"))
            ext.sample_centres_wrapper(B, n, m, d_xyz, index, idx2, new_xyz)
            free = (host(idx2), host(new_xyz))
    return host(idx), host(temp), free


@pytest.mark.parametrize("name,kind", PAIRS)
def test_furthest_point_sampling(oracle, name, kind):
    for case in FPS_CASES:
        family, n, m, indexed, knobs = case
        what = "%s n = %d m = %d" % (family, n, m)
        xyz, _ = vd.cloud(name, kind, n)
        want, want_temp = oracle_fps(oracle, name, kind, n, m)
        idx, temp, free = device_fps(xyz, case)
        np.testing.assert_array_equal(idx, want, err_msg=what)
        np.testing.assert_array_equal(temp.view(np.int32), want_temp.view(np.int32), err_msg=what + " (running distances, bits)")
        if free is not None:
            np.testing.assert_array_equal(free[0], want, err_msg=what + " (temp = None)")
            np.testing.assert_array_equal(free[1].view(np.int32), gathered(xyz, want).view(np.int32), err_msg=what + " (centres)")
        if m == n:     # every point sampled: every running distance has reached zero, but for the last sample's (no round follows it)
            assert ((want_temp == 0).sum(axis=1) >= n - 1).all()


# (the large pyramid on the kitti cloud only: its oracle is the slowest in the file. With denormal distances, 16384 -> 4096 alone
# would keep the CPU busy for half a minute: those three transforms take 8193 -> 1024 -> 64, the smallest pyramid whose first
# level still runs eight waves over an index of 16384 rows and builds the next level's index in its epilogue)
PYRAMIDS = [(name, kind, 1025, (300, 64)) for name, kind in PAIRS] + \
           [(name, "kitti") + ((8193, (1024, 64)) if name in DENORMAL else (16384, (4096, 1024))) for name in vd.NAMES]


@pytest.mark.parametrize("name,kind,n,npoints", PYRAMIDS, ids=["%s-%s-%d" % p[:3] for p in PYRAMIDS])
def test_sampling_pyramid(oracle, name, kind, n, npoints):
    """every level equals furthest point sampling of the level above's centres, whether a level took the identity, replayed
    or ran its rounds (under s+20 and s-90 every early round is a tie: neither shortcut applies)"""
    from epnet_amd import pointnet2_utils as p2u
    xyz, _ = vd.cloud(name, kind, n)

    def levels_of():
        cur, out = xyz, []
        for m in npoints:
            want = oracle.furthest_point_sampling(cur, m)
            cur = gathered(cur, want)
            out += [want, cur]
        return tuple(out)
    ref = once(("pyramid", name, kind, n), levels_of)
    levels = p2u.sample_pyramid(dev(xyz), list(npoints))
    torch.cuda.synchronize()
    for k, (idx, new_xyz, _event, _index) in enumerate(levels):
        np.testing.assert_array_equal(host(idx), ref[2 * k], err_msg="level %d" % k)
        np.testing.assert_array_equal(host(new_xyz).view(np.int32), ref[2 * k + 1].view(np.int32), err_msg="level %d" % k)


# ---- ball query -------------------------------------------------------------------------------------------------------------------
BQ_N, BQ_M, BQ_NS = (300, 1024, 4097, 16385), 96, (1, 16, 65)


def in_range(idx, n, what):
    """an index taken from a padding row (-1) or from beyond the scene fails HERE, not in the kernel that would gather with it"""
    assert idx.min() >= 0 and idx.max() < n, (what, int(idx.min()), int(idx.max()))


def bq_routes(n, ns):
    """(label, over the caller's index, tuning) -- n < 1024: the direct scan alone. Else: the wrapper's own index, the direct scan
    (the indexed entry point without an index), and bq_query_launch one centre per wave, two per wave with the hit bitmap and, where
    nsample <= 64 lets it, two per wave with streamed lists"""
    if n < 1024:
        return (("direct", None, {}),)
    routes = [("own index", None, {}), ("direct", "none", {}), ("indexed, one per wave", "index", {"EPNET_BQ_PAIR": 0}),
              ("indexed, pair, bitmap", "index", {"EPNET_BQ_PAIR": 1, "EPNET_BQ_STREAM": 0})]
    if ns <= 64:
        routes.append(("indexed, pair, stream", "index", {"EPNET_BQ_PAIR": 1, "EPNET_BQ_STREAM": 1}))
    return tuple(routes)


def device_ball_query(route, n, m, radius, ns, d_c, d_xyz, index):
    from epnet_amd import pointnet2_cuda as ext
    _, over, knobs = route
    idx = out_tensor((B, m, ns), torch.int32, 0)       # (an empty ball keeps the zeros its tensor was created with)
    with _lib.tuning(**knobs):
        if over is None:
            ext.ball_query_wrapper(B, n, m, radius, ns, d_c, d_xyz, idx)
        else:
            ext.ball_query_indexed_wrapper(B, n, m, radius, ns, d_c, d_xyz, index if over == "index" else None, idx)
    return host(idx)


def oracle_bq(oracle, name, kind, n, m, k, ns):
    """-> radius k of the case, its centres, the oracle's lists"""
    xyz, r, c = vd.cloud(name, kind, n)[0], float(vd.radii(name, kind, n)[k]), vd.centres(name, kind, n, m)
    return r, c, once(("bq", name, kind, n, m, k, ns), lambda: oracle.ball_query(r, ns, xyz, c))


@pytest.mark.parametrize("n", BQ_N)
@pytest.mark.parametrize("name,kind", SCAN_PAIRS)
def test_ball_query(oracle, name, kind, n):
    from epnet_amd import pointnet2_cuda as ext
    xyz, _ = vd.cloud(name, kind, n)
    d_xyz = dev(xyz)
    index = ext.scene_index(d_xyz)
    assert (index is not None) == (n >= 1024)
    for k in range(3):
        for ns in BQ_NS:
            r, c, want = oracle_bq(oracle, name, kind, n, BQ_M, k, ns)
            d_c = dev(c)
            for route in bq_routes(n, ns):
                what = "n = %d radius[%d] = %r nsample = %d, %s" % (n, k, r, ns, route[0])
                got = device_ball_query(route, n, BQ_M, r, ns, d_c, d_xyz, index)
                in_range(got, n, what)
                np.testing.assert_array_equal(got, want, err_msg=what)
    if n != 300:
        return
    # n = 300 also carries the direct scan with two centres per wave (b * m >= 8192)
    m, ns = 4096, 16
    r, c, want = oracle_bq(oracle, name, kind, n, m, 1, ns)
    got = device_ball_query(("direct, two per wave", None, {}), n, m, r, ns, dev(c), dev(vd.cloud(name, kind, n)[0]), None)
    in_range(got, n, "direct, two per wave")
    np.testing.assert_array_equal(got, want)


# (n, m, noisy centres, values of EPNET_BQ_ORDERED, scales as (radius number, nsample)): forced at the smallest scene with an index
# (np = 4096), with every radius; by default and switched off just above 16384 points, where the centres are scene points and the
# radii the two larger ones (each ball holds its own centre at least: the oracle's scans end early)
ORDERED_CASES = ((2049, 1024, True, (1,), (((0, 16), (1, 32)), ((1, 65),), ((2, 16),))),
                 (16385, 1024, False, (-1, 0), (((1, 16), (2, 32)), ((2, 65),))))


@pytest.mark.parametrize("n,m,noisy,forces,scale_sets", ORDERED_CASES, ids=[str(c[0]) for c in ORDERED_CASES])
@pytest.mark.parametrize("name,kind", SCAN_PAIRS)
def test_ball_query_in_the_centres_order(oracle, name, kind, n, m, noisy, forces, scale_sets):
    """epnet_ball_query_ordered: the centres served in the order of their own scene index, one scale and the pyramid's pair of
    scales (16 and 32 samples: the specialised kernel), against one ball query per scale"""
    from epnet_amd import pointnet2_cuda as ext
    xyz, _ = vd.cloud(name, kind, n)
    rs = [float(r) for r in vd.radii(name, kind, n)]
    c = vd.centres(name, kind, n, m, noisy=noisy)
    d_xyz, d_c = dev(xyz), dev(c)
    index, ci = ext.scene_index(d_xyz), ext.scene_index(d_c)
    assert index is not None and ci is not None
    for scales in scale_sets:
        radii, nss = [rs[k] for k, _ in scales], [ns for _, ns in scales]
        want = [once(("bqo", name, kind, n, k, ns), lambda k=k, ns=ns: oracle.ball_query(rs[k], ns, xyz, c)) for k, ns in scales]
        for force in forces:
            for pair in (0, 1):
                what = "n = %d scales %r EPNET_BQ_ORDERED = %d EPNET_BQ_PAIR = %d" % (n, scales, force, pair)
                outs = [out_tensor((B, m, ns), torch.int32, 0) for ns in nss]
                with _lib.tuning(EPNET_BQ_ORDERED=force, EPNET_BQ_PAIR=pair):
                    ext.ball_query_ordered_wrapper(B, n, m, radii, nss, d_c, d_xyz, index, ci, outs)
                for got, w in zip(outs, want):
                    in_range(host(got), n, what)
                    np.testing.assert_array_equal(host(got), w, err_msg=what)


# ---- three_nn ---------------------------------------------------------------------------------------------------------------------
NN_N, NN_M = (700, 1100), (2, 300, 1100, 2259)


@pytest.mark.parametrize("n", NN_N)
@pytest.mark.parametrize("name,kind", NN_PAIRS)
def test_three_nn(oracle, name, kind, n):
    """plain entry: the direct scan (m < 512) and the entry's own index of the known set; indexed entry: over the known set's scene
    index (m >= 1024) a wave per unknown, and, over the unknown set's index as well (n >= 1024), a wave per bucket of unknowns"""
    from epnet_amd import pointnet2_cuda as ext
    unknown, _ = vd.cloud(name, kind, n)
    d_u = dev(unknown)
    ui = ext.scene_index(d_u)
    for m in NN_M:
        known = vd.known_set(unknown, m)
        d_k = dev(known)
        want_d, want_i = once(("nn", name, kind, n, m), lambda: oracle.three_nn(unknown, known))
        ki = ext.scene_index(d_k)
        routes = [("plain", None)] + [("indexed, EPNET_NN_TILE_MIN_BUCKETS = %d" % t, t) for t in (1, 10 ** 9)]
        for label, tile in routes:
            what = "n = %d m = %d, %s" % (n, m, label)
            d2 = out_tensor((B, n, 3), torch.float32, -1.0)
            i = out_tensor((B, n, 3), torch.int32, -9)
            if tile is None:
                ext.three_nn_wrapper(B, n, m, d_u, d_k, d2, i)
            else:
                with _lib.tuning(EPNET_NN_TILE_MIN_BUCKETS=tile):
                    ext.three_nn_indexed_wrapper(B, n, m, d_u, d_k, ui, ki, d2, i)
            np.testing.assert_array_equal(host(i), want_i, err_msg=what)
            np.testing.assert_array_equal(host(d2).view(np.int32), want_d.view(np.int32), err_msg=what + " (squared distances, bits)")


# ---- fused grouping ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", SCAN_PAIRS)
def test_query_and_group_and_group_linear(oracle, name, kind):
    """QueryAndGroup ([xyz - centre ; features] of the ball query's lists) and group_linear (the first shared-MLP layer folded into
    the grouping), composed from the oracle's pieces. The plain ball query of the case is compared first: a wrong neighbour list ends
    the test there, as a failed comparison, and never reaches a gather. group_linear's w_xyz is scaled by 2^-40 under s+60 (its
    products stay far from the top of the range); the oracle's result is required to be finite everywhere"""
    from epnet_amd import pointnet2_utils as p2u
    ns, m = 16, BQ_M
    for n in (1024, 4097):
        xyz, _ = vd.cloud(name, kind, n)
        c = vd.centres(name, kind, n, m)
        d_xyz, d_c = dev(xyz), dev(c)
        xyz_t = np.ascontiguousarray(xyz.transpose(0, 2, 1))
        rng = np.random.default_rng([n, 23])
        for k in range(3):
            r = float(vd.radii(name, kind, n)[k])
            want = once(("bq", name, kind, n, m, k, ns), lambda: oracle.ball_query(r, ns, xyz, c))
            got = host(p2u.ball_query(r, ns, d_xyz, d_c))
            in_range(got, n, "ball query")
            np.testing.assert_array_equal(got, want, err_msg="n = %d radius[%d]: the ball query" % (n, k))
            local = oracle.group_points(xyz_t, want) - c.transpose(0, 2, 1)[..., None]
            assert np.isfinite(local).all()
            for ch in (0, 19):
                feats = rng.standard_normal((B, ch, n)).astype(np.float32) if ch else None
                fused = p2u.QueryAndGroup(r, ns)(d_xyz, d_c, dev(feats) if ch else None)
                ref = np.concatenate([local, oracle.group_points(feats, want)], axis=1) if ch else local
                np.testing.assert_array_equal(host(fused).view(np.int32), ref.view(np.int32), err_msg="n = %d radius[%d] c = %d" % (n, k, ch))
            ch = 16
            z = rng.standard_normal((B, ch, n)).astype(np.float32)
            w_xyz = (rng.standard_normal((ch, 3)) * 0.3).astype(np.float32) * (vd.p2(-40) if name == "s+60" else np.float32(1))
            bias = rng.standard_normal((ch,)).astype(np.float32)
            ref = oracle.group_linear(xyz, c, z, want, w_xyz, bias)
            assert np.isfinite(ref).all()
            lin = p2u.group_linear(d_xyz, d_c, dev(z), dev(want), dev(w_xyz), dev(bias))
            np.testing.assert_array_equal(host(lin).view(np.int32), ref.view(np.int32), err_msg="n = %d radius[%d]: group_linear" % (n, k))


# ---- exact scalings (secondary: the oracle comparisons above are the test) -----------------------------------------------------------
@pytest.mark.parametrize("kind", vd.BASES)
@pytest.mark.parametrize("name", vd.EXACT)
def test_exact_scalings_scale_exactly(name, kind):
    """a power-of-two scaling that neither underflows nor clamps changes no index and multiplies every distance by scale^2, on the
    device as in the oracle: device results of the scaled cloud against device results of the base cloud"""
    from epnet_amd import pointnet2_cuda as ext
    for case in FPS_CASES:
        _, n, m, _, _ = case
        scaled, scale = vd.cloud(name, kind, n)
        idx0, temp0, _ = device_fps(vd.cloud("base", kind, n)[0], case)
        idx1, temp1, _ = device_fps(scaled, case)
        np.testing.assert_array_equal(idx1, idx0, err_msg=str(case))
        assert (temp0 < vd.START).all() and (temp1 < vd.START).all()      # nothing is left at, or clamped to, the start value
        np.testing.assert_array_equal(temp1, temp0 * (scale * scale), err_msg=str(case))
    n, m, ns = 4097, BQ_M, 16
    scaled, scale = vd.cloud(name, kind, n)
    for k in range(3):
        got = []
        for which in ("base", name):
            xyz, c, r = vd.cloud(which, kind, n)[0], vd.centres(which, kind, n, m), float(vd.radii(which, kind, n)[k])
            d_xyz = dev(xyz)
            got.append(device_ball_query(("indexed", "index", {"EPNET_BQ_PAIR": 0}), n, m, r, ns, dev(c), d_xyz, ext.scene_index(d_xyz)))
        np.testing.assert_array_equal(got[1], got[0], err_msg="ball query radius[%d]" % k)
    n, m = 1100, 1100
    res = []
    for unknown in (vd.cloud("base", kind, n)[0], vd.cloud(name, kind, n)[0]):
        d_u, d_k = dev(unknown), dev(vd.known_set(unknown, m))
        d2 = out_tensor((B, n, 3), torch.float32, -1.0)
        i = out_tensor((B, n, 3), torch.int32, -9)
        ext.three_nn_indexed_wrapper(B, n, m, d_u, d_k, ext.scene_index(d_u), ext.scene_index(d_k), d2, i)
        res.append((host(d2), host(i)))
    np.testing.assert_array_equal(res[1][1], res[0][1])
    np.testing.assert_array_equal(res[1][0], res[0][0] * (scale * scale))

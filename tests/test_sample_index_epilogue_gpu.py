"""epnet_sample_centres_chain_index: the sampling of a level, the gather of its centres and the scene index of those centres in
one call -- for 8192 < n <= 16384 and 1024 <= m <= 4096 in the epilogue of the 512-thread sampling kernel itself -- against the two
separate calls it replaces (epnet_sample_centres_chain, then epnet_scene_index_build_gathered).

Three scenes per case: a KITTI-like one, one padded with exact twins of its own rows, and a lattice whose equal distances tie
between DIFFERENT points in the first rounds (prefix_out < m), so that the next level takes the identity for some scenes and
replays its rounds for others, both from the index under test.

idx, new_xyz and prefix_out are compared bit for bit. The index is not: inside a grid cell the order of the points is the order in
which the LDS atomics of the histogram pass were served, which differs between two launches of the same kernel. What is fixed is
the cell of every point, so the sorted rows are compared after ordering them by (cell, original index), with the cell computed
here from the coordinates the way spatial.h does (and required to be non-decreasing along the rows as the kernel wrote them);
the bucket and quad boxes are compared with the boxes of the rows the index itself holds; and the consumers -- both ball queries
of the next level and its chained sampling -- run from the index under test and must equal the CPU oracle.

Shapes: 16384 -> 4096 is the workload's level 1; 8200 is the smallest cloud that reaches the 512-thread kernel, no multiple of 64,
with the smallest m that has an epilogue; 9000 -> 1500 has an index padded to 2048 with buckets of padding only.
"""
import functools

import numpy as np
import pytest
import torch

from epnet_amd import pointnet2_cuda as ext

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 3
f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded(hiplib):
    assert torch.cuda.is_available()
    return hiplib


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)   # (a copy: the shared references are read-only)


def host(t):
    return t.detach().cpu().numpy()


def lattice(n, seed):
    """points on a half-metre lattice, a quarter of them repeated: equal distances between different points from the first rounds on"""
    rng = np.random.default_rng(seed)
    base = rng.integers(-8, 9, size=(max(4, (n * 3) // 4), 3)).astype(f32) * f32(0.5)
    pts = np.concatenate([base, base[rng.integers(0, len(base), size=n - len(base))]])
    return pts[rng.permutation(n)].astype(f32)


@functools.lru_cache(maxsize=None)
def clouds(n, seed=0):
    from epnet_amd import synth
    # (three quarters of the dup scene are distinct points, the rest exact twins of some of them)
    c = np.stack([synth.cloud("kitti", n, seed + 70).numpy(), synth.dup_cloud(n, seed + 71, unique=(n * 3) // 4).numpy(),
                  lattice(n, seed + 72)])
    c.setflags(write=False)
    return c


_REF = {}


def reference(oracle, n, m, seed=0):
    """the oracle's samples and centres of clouds(n), computed once per shape and shared"""
    key = (n, m, seed)
    if key not in _REF:
        c = clouds(n, seed)
        idx = oracle.furthest_point_sampling(c, m)
        centres = np.take_along_axis(c, idx[:, :, None].astype(np.int64), axis=1)
        idx.setflags(write=False)
        centres.setflags(write=False)
        _REF[key] = (idx, centres)
    return _REF[key]


def next_shape(m):
    """the level below: a quarter of the centres, with the workload's radii for a cloud of that size"""
    return m // 4, ((0.5, 1.0) if m > 2048 else (1.0, 2.0)), (16, 32)


def separate(cloud_d, n, m, cap):
    """the two calls the new entry point replaces"""
    index = ext.scene_index(cloud_d)
    idx = torch.full((B, m), -1, dtype=torch.int32, device=DEV)
    new_xyz = torch.full((B, m, 3), float("nan"), device=DEV)
    prefix = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    nxt = torch.zeros((ext.scene_index_bytes(B, m),), dtype=torch.uint8, device=DEV)
    ext.sample_centres_wrapper(B, n, m, cloud_d, index, idx, None, None, prefix, cap)
    ext.scene_index_build_gathered_wrapper(B, n, m, cloud_d, idx, new_xyz, nxt)
    return idx, new_xyz, prefix, nxt


def fused(cloud_d, n, m, cap, outs=None):
    index = ext.scene_index(cloud_d)
    if outs is None:
        outs = (torch.full((B, m), -1, dtype=torch.int32, device=DEV), torch.full((B, m, 3), float("nan"), device=DEV),
                torch.full((B,), -7, dtype=torch.int32, device=DEV))
    idx, new_xyz, prefix = outs
    nxt = torch.zeros((ext.scene_index_bytes(B, m),), dtype=torch.uint8, device=DEV)
    ext.sample_centres_index_wrapper(B, n, m, cloud_d, index, idx, new_xyz, nxt, None, prefix, cap)
    return idx, new_xyz, prefix, nxt


# ---- the scene index on the host (spatial.h)

def index_np(m):
    np_ = 2048
    while np_ < m:
        np_ <<= 1
    return np_


def split_index(index, m):
    np_ = index_np(m)
    raw = host(index)
    a, b_ = B * np_ * 16, B * (np_ // 64) * 24
    rows = raw[:a].view(f32).reshape(B, np_, 4)
    boxes = raw[a:a + b_].view(f32).reshape(B, np_ // 64, 6)
    qboxes = raw[a + b_:a + b_ + B * (np_ // 256) * 24].view(f32).reshape(B, np_ // 256, 6)
    return rows, boxes, qboxes


def cell_codes(pts, max_bits):
    """make_cell_grid + cell_code of spatial.h in fp32, for the points of one scene"""
    lo = pts.min(axis=0).astype(f32)
    ext_ = (pts.max(axis=0).astype(f32) - lo).astype(f32)
    big = f32(ext_.max())
    cell = f32(big / f32(64)) if big > 0 else f32(1)
    bits = [0, 0, 0]
    for _ in range(8):
        total = 0
        for a in range(3):
            cells = int(f32(ext_[a] / cell)) + 1
            b_ = 0
            while (1 << b_) < cells and b_ < 6:
                b_ += 1
            bits[a] = b_
            total += b_
        if total <= max_bits:
            break
        cell = f32(cell * f32(1.26))
    inv = f32(f32(1) / cell)
    c = []
    for a in range(3):
        v = ((pts[:, a] - lo[a]).astype(f32) * inv).astype(f32).astype(np.int64)   # (int): towards zero; the values are >= 0
        c.append(np.clip(v, 0, (1 << bits[a]) - 1))
    code = np.zeros(len(pts), dtype=np.int64)
    pos = 0
    for b_ in range(6):
        for a in range(3):
            if b_ < bits[a]:
                code |= ((c[a] >> b_) & 1) << pos
                pos += 1
    return code


def canonical_rows(index, m, centres, max_bits):
    """the rows of an index ordered by (cell, original index), after checking that the index is one: every centre exactly once with
    its own coordinates, cells non-decreasing, padding behind, and boxes that are the boxes of the rows"""
    rows, boxes, qboxes = split_index(index, m)
    np_ = rows.shape[1]
    out = []
    for s in range(B):
        r = rows[s]
        w = r[:, 3].view(np.int32)
        assert (w[:m] >= 0).all() and (w[m:] == -1).all() and (r[m:, :3] == f32(3.0e38)).all(), "padding rows"
        assert np.array_equal(np.sort(w[:m]), np.arange(m)), "every centre exactly once"
        assert np.array_equal(r[:m, :3], centres[s][w[:m]]), "rows carry their point's coordinates"
        code = cell_codes(centres[s], max_bits)[w[:m]]
        assert (np.diff(code) >= 0).all(), "rows in cell order"
        out.append(r[:m][np.lexsort((w[:m], code))])
        real = (np.arange(np_) < m).reshape(np_ // 64, 64)
        pts = r[:, :3].reshape(np_ // 64, 64, 3)
        want = np.full((np_ // 64, 6), f32(3.0e38), dtype=f32)
        for k in range(np_ // 64):
            if real[k].any():
                p = pts[k][real[k]]
                want[k, 0::2], want[k, 1::2] = p.min(axis=0), p.max(axis=0)
        np.testing.assert_array_equal(boxes[s], want, err_msg="bucket boxes, scene %d" % s)
        wantq = np.full((np_ // 256, 6), f32(3.0e38), dtype=f32)
        for g in range(np_ // 256):
            part = want[4 * g:4 * g + 4]
            part = part[part[:, 0] < f32(3.0e38)]
            if len(part):
                wantq[g, 0::2], wantq[g, 1::2] = part[:, 0::2].min(axis=0), part[:, 1::2].max(axis=0)
        np.testing.assert_array_equal(qboxes[s], wantq, err_msg="quad boxes, scene %d" % s)
    return np.stack(out)


def check_consumers(oracle, m, new_xyz, prefix, nxt, centres):
    """both ball queries of the next level and its chained sampling, from the index under test, against the oracle"""
    m2, radii, nss = next_shape(m)
    idx2 = torch.full((B, m2), -1, dtype=torch.int32, device=DEV)
    centres2 = torch.full((B, m2, 3), float("nan"), device=DEV)
    prefix2 = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    ext.sample_centres_wrapper(B, m, m2, new_xyz, nxt, idx2, centres2, prefix, prefix2)
    want2 = oracle.furthest_point_sampling(np.asarray(centres), m2)
    np.testing.assert_array_equal(host(idx2), want2, err_msg="next level's sampling")
    want_c2 = np.take_along_axis(np.asarray(centres), want2[:, :, None].astype(np.int64), axis=1)
    np.testing.assert_array_equal(host(centres2), want_c2)
    outs = [torch.full((B, m2, ns), -1, dtype=torch.int32, device=DEV) for ns in nss]
    ext.ball_query_multi_wrapper(B, m, m2, list(radii), list(nss), centres2, new_xyz, nxt, outs)
    for r, ns, got in zip(radii, nss, outs):
        np.testing.assert_array_equal(host(got), oracle.ball_query(r, ns, np.asarray(centres), want_c2), err_msg="ball query r=%g" % r)
    return host(prefix)


@pytest.mark.parametrize("n,m", [(16384, 4096), (8200, 1024), (9000, 1500)])
def test_epilogue_equals_the_two_separate_calls(oracle, n, m):
    want_idx, want_c = reference(oracle, n, m)
    cloud_d = dev(clouds(n))
    cap = next_shape(m)[0]
    a_idx, a_xyz, a_pre, a_nxt = separate(cloud_d, n, m, cap)
    b_idx, b_xyz, b_pre, b_nxt = fused(cloud_d, n, m, cap)
    np.testing.assert_array_equal(host(a_idx), want_idx)
    assert torch.equal(b_idx, a_idx) and torch.equal(b_pre, a_pre)
    assert torch.equal(b_xyz.view(torch.int32), a_xyz.view(torch.int32))
    np.testing.assert_array_equal(host(b_xyz), want_c)
    bits = 12 if m <= 4096 else 14
    np.testing.assert_array_equal(canonical_rows(b_nxt, m, want_c, bits), canonical_rows(a_nxt, m, want_c, bits))
    pre = check_consumers(oracle, m, b_xyz, b_pre, b_nxt, want_c)
    # the lattice scene ties between different points inside the rounds the next level asks about; the KITTI-like one does not
    assert pre[2] < cap <= pre[0], pre


def test_outputs_off_a_16_byte_boundary(oracle):
    """idx, new_xyz and prefix_out 4, 8 and 12 bytes past a boundary (the separate route picks its gather by that alignment; the
    epilogue must not care), with canaries on either side of each"""
    import offset_alloc as oa
    n, m = 8200, 1024
    want_idx, want_c = reference(oracle, n, m)
    cap = next_shape(m)[0]
    cloud_d = dev(clouds(n))
    outs = (oa.output((B, m), torch.int32, 4), oa.output((B, m, 3), torch.float32, 8), oa.output((B,), torch.int32, 12))
    idx, new_xyz, prefix, nxt = fused(cloud_d, n, m, cap, outs)
    oa.check()
    assert oa.unwritten(idx) == 0 and oa.unwritten(new_xyz) == 0 and oa.unwritten(prefix) == 0
    np.testing.assert_array_equal(host(idx), want_idx)
    np.testing.assert_array_equal(host(new_xyz), want_c)
    a_idx, a_xyz, a_pre, a_nxt = separate(cloud_d, n, m, cap)
    assert torch.equal(prefix, a_pre)
    np.testing.assert_array_equal(canonical_rows(nxt, m, want_c, 12), canonical_rows(a_nxt, m, want_c, 12))
    check_consumers(oracle, m, new_xyz.contiguous(), prefix, nxt, want_c)


def test_captured_into_a_graph_and_replayed_on_two_inputs(oracle):
    n, m = 8200, 1024
    cap = next_shape(m)[0]
    static = dev(clouds(n, 0))
    index = torch.zeros((ext.scene_index_bytes(B, n),), dtype=torch.uint8, device=DEV)
    idx = torch.full((B, m), -1, dtype=torch.int32, device=DEV)
    new_xyz = torch.full((B, m, 3), float("nan"), device=DEV)
    prefix = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    nxt = torch.zeros((ext.scene_index_bytes(B, m),), dtype=torch.uint8, device=DEV)

    def step():
        ext.scene_index_build_wrapper(B, n, static, index)
        ext.sample_centres_index_wrapper(B, n, m, static, index, idx, new_xyz, nxt, None, prefix, cap)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for seed in (5, 0):   # two different inputs, the second one after the first has been through
        static.copy_(dev(clouds(n, seed)))
        for t in (idx, prefix):
            t.fill_(-3)
        new_xyz.fill_(float("nan"))
        nxt.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want_idx, want_c = reference(oracle, n, m, seed)
        np.testing.assert_array_equal(host(idx), want_idx)
        np.testing.assert_array_equal(host(new_xyz), want_c)
        a_idx, a_xyz, a_pre, a_nxt = separate(static, n, m, cap)
        assert torch.equal(prefix, a_pre)
        np.testing.assert_array_equal(canonical_rows(nxt, m, want_c, 12), canonical_rows(a_nxt, m, want_c, 12))
        check_consumers(oracle, m, new_xyz, prefix, nxt, want_c)


def test_shapes_without_an_epilogue_take_the_separate_route(oracle):
    """m = 8192 is more than the 512-thread workgroup holds (8 centres per thread), and a cloud of 4096 points runs the 256-thread
    kernel: the entry point issues the index build as a launch of its own, with the same results; a call without a next index is
    the existing entry point, which `separate` has used all along"""
    for n, m in ((16384, 8192), (4096, 1024)):
        want_idx, want_c = reference(oracle, n, m)
        cloud_d = dev(clouds(n))
        cap = next_shape(m)[0]
        a_idx, a_xyz, a_pre, a_nxt = separate(cloud_d, n, m, cap)
        b_idx, b_xyz, b_pre, b_nxt = fused(cloud_d, n, m, cap)
        np.testing.assert_array_equal(host(b_idx), want_idx)
        np.testing.assert_array_equal(host(b_xyz), want_c)
        assert torch.equal(b_idx, a_idx) and torch.equal(b_pre, a_pre) and torch.equal(b_xyz.view(torch.int32), a_xyz.view(torch.int32))
        bits = 12 if m <= 4096 else 14
        np.testing.assert_array_equal(canonical_rows(b_nxt, m, want_c, bits), canonical_rows(a_nxt, m, want_c, bits))
        check_consumers(oracle, m, b_xyz, b_pre, b_nxt, want_c)

"""The deterministic gradients on the device (include/epnet_ops.h, "*_det"). Under
torch.use_deterministic_algorithms(True) the stand-in wrappers take them, and their bits must equal the oracle's sequential loops
(the scatter-add ops, from a nonzero starting buffer) or the numpy restatement of the contract order (feature_gather_grad,
group_linear_grad_w) -- compared with np.array_equal, not to a tolerance. Also: autograd under the flag, four host threads on four
streams, and graph capture."""
import contextlib
import ctypes
import threading

import numpy as np
import pytest
import torch

import det_restate as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
i32 = torch.int32


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded(hiplib):
    assert torch.cuda.is_available()
    return hiplib


@contextlib.contextmanager
def deterministic(on=True):
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(on)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev)


def rng(seed):
    return np.random.default_rng(seed)


def same_bits(got, want):
    got = np.ascontiguousarray(got, np.float32)
    want = np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%d of %d elements differ, first at %s: %r vs %r" % (
        int(bad.sum()), bad.size, np.argwhere(bad)[0].tolist(), got[bad][0], want[bad][0])


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ---- the oracle's loops, from a given starting buffer ----------------------------------------------------------------------
def oracle_gather_grad(oracle, start, grad_out, idx):
    g = np.array(start, np.float32, copy=True)
    b, c, m = grad_out.shape
    oracle.lib().oracle_gather_points_grad(b, c, g.shape[2], m, _p(np.ascontiguousarray(grad_out, np.float32)),
                                           _p(np.ascontiguousarray(idx, np.int32)), _p(g))
    return g


def oracle_group_grad(oracle, start, grad_out, idx):
    g = np.array(start, np.float32, copy=True)
    b, c, m, ns = grad_out.shape
    oracle.lib().oracle_group_points_grad(b, c, g.shape[2], m, ns, _p(np.ascontiguousarray(grad_out, np.float32)),
                                          _p(np.ascontiguousarray(idx, np.int32)), _p(g))
    return g


def oracle_interp_grad(oracle, start, grad_out, idx, weight):
    g = np.array(start, np.float32, copy=True)
    b, c, n = grad_out.shape
    oracle.lib().oracle_three_interpolate_grad(b, c, n, g.shape[2], _p(np.ascontiguousarray(grad_out, np.float32)),
                                               _p(np.ascontiguousarray(idx, np.int32)),
                                               _p(np.ascontiguousarray(weight, np.float32)), _p(g))
    return g


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def unaligned(a):
    """a device copy of the float32 array `a` whose data pointer is 4 bytes past a 16-byte boundary"""
    flat = torch.empty((a.size + 4,), dtype=torch.float32, device=DEV)
    t = flat[1:1 + a.size].view(a.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def skewed_index(r, b, p, n, hot=None, pad_runs=0, ns=1):
    """indices with a ball-query-like skew: each group of ns repeats its first index from a random point on (padding), plus an
    optional hot target receiving `hot` entries"""
    idx = r.integers(0, n, size=(b, p), dtype=np.int64)
    if pad_runs:
        g = idx.reshape(b, p // ns, ns)
        cut = r.integers(1, ns + 1, size=(b, p // ns))
        mask = np.arange(ns)[None, None, :] >= cut[:, :, None]
        g[mask] = np.broadcast_to(g[:, :, :1], g.shape)[mask]
        idx = g.reshape(b, p)
    if hot:
        for bi in range(b):
            pos = r.choice(p, size=hot, replace=False)
            idx[bi, pos] = n // 2
    return idx.astype(np.int32)


# ---- 1. bit-exact against the oracle ---------------------------------------------------------------------------------------
GROUP_CASES = [
    # (b, c, n, npoints, nsample, extra)
    (16, 96, 4096, 1024, 32, {}),                       # bench level-2 shape at 16 scenes
    (16, 32, 16384, 4096, 16, {}),                      # bench level-1
    (2, 8, 16383, 1024, 16, {}),                        # n * 4 just below 64 KB (default: LDS atomics)
    (2, 8, 16385, 1024, 16, {}),                        # just above (default: global atomics), past runsum::kMaxTargets
    (2, 8, 16384, 1024, 16, {}),
    (3, 5, 1000, 1023, 3, {}),                          # p % 4 != 0, c % 8 != 0
    (2, 16, 4096, 4096, 32, {"tiles": True}),           # p = 131072: several run-sum tiles
    (2, 8, 4096, 1024, 32, {"unaligned": True}),        # grad_out 4 bytes off a 16-byte boundary
    (2, 8, 4096, 1024, 32, {"hot": 20000}),             # one target with 2e4 entries
    (2, 8, 4096, 1024, 64, {"pad": True}),              # heavy ball-query padding
    (1, 4, 65536, 16384, 64, {"pad": True}),            # config 5: n = 65536, 16384 x 64 entries
]


@pytest.mark.parametrize("case", GROUP_CASES, ids=lambda c: "b%d_c%d_n%d_m%d_ns%d%s" % (c[:5] + ("_" + "_".join(c[5]) if c[5] else "",)))
def test_group_points_grad_det_is_the_oracle(case, oracle):
    from epnet_amd import pointnet2_cuda as ext
    b, c, n, m, ns, extra = case
    r = rng(n + m + ns)
    idx = skewed_index(r, b, m * ns, n, hot=extra.get("hot"), pad_runs=extra.get("pad", False), ns=ns).reshape(b, m, ns)
    go = r.standard_normal((b, c, m, ns), dtype=np.float32)
    start = r.standard_normal((b, c, n), dtype=np.float32)
    gp = dev(start)
    g_dev = unaligned(go) if extra.get("unaligned") else dev(go)
    with deterministic():
        ext.group_points_grad_wrapper(b, c, n, m, ns, g_dev, dev(idx), gp)
    same_bits(gp.cpu().numpy(), oracle_group_grad(oracle, start, go, idx))


@pytest.mark.parametrize("b,c,n,m", [(16, 3, 16384, 4096), (16, 64, 4096, 1024), (2, 7, 20000, 1027)])
def test_gather_points_grad_det_is_the_oracle(b, c, n, m, oracle):
    from epnet_amd import pointnet2_cuda as ext
    r = rng(n + m)
    idx = r.integers(0, n, size=(b, m), dtype=np.int32)
    go = r.standard_normal((b, c, m), dtype=np.float32)
    start = r.standard_normal((b, c, n), dtype=np.float32)
    gp = dev(start)
    with deterministic():
        ext.gather_points_grad_wrapper(b, c, n, m, dev(go), dev(idx), gp)
    same_bits(gp.cpu().numpy(), oracle_gather_grad(oracle, start, go, idx))


def _three_nn_index(b, n, m, seed):
    from epnet_amd import pointnet2_utils as p2u, synth
    unknown = synth.scenes("kitti", b, n, seed=seed).to(DEV)
    known = synth.scenes("kitti", b, m, seed=seed + 1).to(DEV)
    _, idx = p2u.three_nn(unknown, known)
    return idx.cpu().numpy()


@pytest.mark.parametrize("b,c,n,m", [(16, 256, 16384, 4096), (16, 512, 4096, 1024), (1, 256, 16384, 4096), (2, 8, 8192, 16385),
                                     (2, 5, 1001, 64)])
def test_three_interpolate_grad_det_is_the_oracle(b, c, n, m, oracle):
    from epnet_amd import pointnet2_cuda as ext
    r = rng(n + m + c)
    idx = _three_nn_index(b, n, m, seed=n % 97)
    w = r.random((b, n, 3), dtype=np.float32)
    w = (w / w.sum(-1, keepdims=True)).astype(np.float32)
    go = r.standard_normal((b, c, n), dtype=np.float32)
    start = r.standard_normal((b, c, m), dtype=np.float32)
    gp = dev(start)
    with deterministic():
        ext.three_interpolate_grad_wrapper(b, c, n, m, unaligned(go) if c == 5 else dev(go), dev(idx), dev(w), gp)
    same_bits(gp.cpu().numpy(), oracle_interp_grad(oracle, start, go, idx, w))


@pytest.mark.parametrize("use_xyz", [True, False])
def test_group_concat_grad_det_two_scales_into_one_buffer(use_xyz, oracle):
    """_GroupConcatMulti.backward: two scales accumulate into one buffer = the oracle called twice"""
    from epnet_amd import pointnet2_cuda as ext
    b, c, n, m = 4, 24, 4096, 1024
    r = rng(5 + use_xyz)
    ch0 = 3 if use_xyz else 0
    start = r.standard_normal((b, c, n), dtype=np.float32)
    gp = dev(start)
    want = start
    with deterministic():
        for ns in (16, 32):
            idx = skewed_index(r, b, m * ns, n, pad_runs=True, ns=ns).reshape(b, m, ns)
            go = r.standard_normal((b, ch0 + c, m, ns), dtype=np.float32)
            ext.group_concat_grad_wrapper(b, c, n, m, ns, dev(go), dev(idx), gp, use_xyz)
            want = oracle_group_grad(oracle, want, go[:, ch0:], idx)
    same_bits(gp.cpu().numpy(), want)


@pytest.mark.parametrize("align_corners", [True, False])
@pytest.mark.parametrize("b,c,h,w,n", [(2, 64, 48, 160, 4096), (2, 512, 24, 80, 64), (1, 7, 5, 9, 333)])
def test_feature_gather_grad_det_is_the_restatement(b, c, h, w, n, align_corners):
    from epnet_amd import pointnet2_cuda as ext
    r = rng(h * w + n + align_corners)
    xy = r.uniform(-1.1, 1.1, size=(b, n, 2)).astype(np.float32)     # some points outside the map
    xy[:, : n // 8] = xy[:, :1]                                        # many points on one pixel: long runs
    xy[0, -1] = [np.inf, 0.5]
    go = r.standard_normal((b, c, n), dtype=np.float32)
    start = r.standard_normal((b, c, h, w), dtype=np.float32)
    gm = dev(start)
    with deterministic():
        ext.feature_gather_grad_wrapper(b, c, h, w, n, align_corners, dev(go), dev(xy), gm)
    same_bits(gm.cpu().numpy(), R.feature_gather_grad(start, go, xy, align_corners))


@pytest.mark.parametrize("b,c,n,m,ns", [(16, 64, 4096, 1024, 32), (3, 13, 1000, 333, 7), (1, 8, 16384, 4096, 64)])
def test_group_linear_grad_w_det_is_the_restatement(b, c, n, m, ns, oracle):
    from epnet_amd import pointnet2_cuda as ext, synth
    r = rng(c + m)
    xyz = synth.scenes("kitti", b, n, seed=3).numpy()
    new_xyz = xyz[:, r.choice(n, m, replace=False)]
    idx = skewed_index(r, b, m * ns, n, pad_runs=True, ns=ns).reshape(b, m, ns)
    go = r.standard_normal((b, c, m, ns), dtype=np.float32)
    start = r.standard_normal((c, 3), dtype=np.float32)
    gw = dev(start)
    with deterministic():
        ext.group_linear_grad_w_wrapper(b, c, n, m, ns, dev(go), dev(xyz), dev(new_xyz), dev(idx), gw)
    got = gw.cpu().numpy()
    same_bits(got, R.group_linear_grad_w(start, go, xyz, new_xyz, idx))
    d = xyz[np.arange(b)[:, None], idx.reshape(b, -1)].astype(np.float64) - np.repeat(new_xyz, ns, axis=1)
    exact = start + np.einsum("bcp,bpk->ck", go.reshape(b, c, -1).astype(np.float64), d)
    assert np.allclose(got, exact, rtol=1e-4, atol=1e-3)


def test_a_shape_the_det_path_cannot_run_raises_by_name():
    """b > 65535 scenes: EPNET_ELIMIT, raised as a RuntimeError that names the op -- never a silent atomic fallback"""
    from epnet_amd import pointnet2_cuda as ext
    b = 65536
    gp = torch.zeros((b, 1, 2), device=DEV)
    with deterministic(), pytest.raises(RuntimeError, match="group_points_grad"):
        ext.group_points_grad_wrapper(b, 1, 2, 1, 1, torch.ones((b, 1, 1, 1), device=DEV), torch.zeros((b, 1, 1), dtype=i32, device=DEV), gp)
    assert not bool(gp.any())


# ---- 2. autograd under the flag ----------------------------------------------------------------------------------------------
def _autograd_step(seed):
    from epnet_amd import li_fusion, pointnet2_utils as p2u, synth
    g = torch.Generator().manual_seed(seed)
    b, n, m = 2, 4096, 1024
    xyz = synth.scenes("kitti", b, n, seed=21).to(DEV)
    feat = torch.randn((b, 16, n), generator=g).to(DEV).requires_grad_(True)
    idx = p2u.furthest_point_sample(xyz, m)
    new_xyz = p2u.gather_operation(xyz.transpose(1, 2).contiguous(), idx).transpose(1, 2).contiguous()
    bq1, bq2 = p2u.ball_query(0.8, 16, xyz, new_xyz), p2u.ball_query(1.6, 32, xyz, new_xyz)
    sub = p2u.gather_operation(feat, idx)                                    # (b, 16, m)
    grouped = p2u.grouping_operation(feat, bq1)
    g1, g2 = p2u.group_concat_multi(xyz, new_xyz, feat, [bq1, bq2], use_xyz=True)
    dist, nn = p2u.three_nn(xyz, new_xyz)
    recip = 1.0 / (dist + 1e-8)
    wgt = (recip / recip.sum(dim=2, keepdim=True)).contiguous()
    interp = p2u.three_interpolate(sub, nn, wgt)                            # (b, 16, n)
    w_xyz = torch.randn((16, 3), generator=g).to(DEV).requires_grad_(True)
    lin = p2u.group_linear(xyz, new_xyz, feat, bq1, w_xyz)
    fmap = torch.randn((b, 16, 24, 80), generator=g).to(DEV).requires_grad_(True)
    xy = (torch.rand((b, n, 2), generator=g) * 2.2 - 1.1).to(DEV)
    sampled = li_fusion.Feature_Gather(fmap, xy)
    loss = ((grouped * grouped).sum() + (g1 * 0.5).sum() + (g2.sin()).sum() + (interp * interp).sum() + (lin.cos()).sum()
            + (sampled * sampled).sum())
    loss.backward()
    return [t.grad.detach().cpu().numpy() for t in (feat, w_xyz, fmap)]


def test_autograd_gradients_repeat_bit_for_bit_under_the_flag():
    with deterministic():
        a = _autograd_step(1)
        b = _autograd_step(1)
    for x, y in zip(a, b):
        same_bits(x, y)


def test_autograd_gradients_are_the_contract_values(oracle):
    """grouping_operation / gather_operation / three_interpolate / Feature_Gather through autograd equal the bit-exact expectations"""
    from epnet_amd import li_fusion, pointnet2_utils as p2u, synth
    r = rng(9)
    b, c, n, m, ns = 2, 16, 4096, 1024, 32
    xyz = synth.scenes("kitti", b, n, seed=22).to(DEV)
    feat_h = r.standard_normal((b, c, n), dtype=np.float32)
    idx = p2u.furthest_point_sample(xyz, m)
    new_xyz = p2u.gather_operation(xyz.transpose(1, 2).contiguous(), idx).transpose(1, 2).contiguous()
    bq = p2u.ball_query(1.0, ns, xyz, new_xyz)
    go_g = r.standard_normal((b, c, m, ns), dtype=np.float32)
    go_s = r.standard_normal((b, c, m), dtype=np.float32)
    with deterministic():
        feat = dev(feat_h).requires_grad_(True)
        (p2u.grouping_operation(feat, bq) * dev(go_g)).sum().backward()
        got_group = feat.grad.cpu().numpy()
        feat = dev(feat_h).requires_grad_(True)
        (p2u.gather_operation(feat, idx) * dev(go_s)).sum().backward()
        got_gather = feat.grad.cpu().numpy()
    zero = np.zeros((b, c, n), np.float32)
    # (x * go).sum() hands go to the op's backward: the gradient is the oracle's scatter of go
    same_bits(got_group, oracle_group_grad(oracle, zero, go_g, bq.cpu().numpy()))
    same_bits(got_gather, oracle_gather_grad(oracle, zero, go_s, idx.cpu().numpy()))

    dist, nn = p2u.three_nn(xyz, new_xyz)
    w = (1.0 / (dist + 1e-8)); w = (w / w.sum(dim=2, keepdim=True)).contiguous()
    sub_h = r.standard_normal((b, c, m), dtype=np.float32)
    go_i = r.standard_normal((b, c, n), dtype=np.float32)
    fmap_h = r.standard_normal((b, c, 24, 80), dtype=np.float32)
    xy_h = r.uniform(-1.1, 1.1, size=(b, n, 2)).astype(np.float32)
    go_f = r.standard_normal((b, c, n), dtype=np.float32)
    with deterministic():
        sub = dev(sub_h).requires_grad_(True)
        (p2u.three_interpolate(sub, nn, w) * dev(go_i)).sum().backward()
        fmap = dev(fmap_h).requires_grad_(True)
        (li_fusion.Feature_Gather(fmap, dev(xy_h)) * dev(go_f)).sum().backward()
    same_bits(sub.grad.cpu().numpy(), oracle_interp_grad(oracle, np.zeros((b, c, m), np.float32), go_i, nn.cpu().numpy(), w.cpu().numpy()))
    same_bits(fmap.grad.cpu().numpy(), R.feature_gather_grad(np.zeros_like(fmap_h), go_f, xy_h, True))


# ---- 3. four host threads on four streams ------------------------------------------------------------------------------------
def _det_jobs():
    from epnet_amd import pointnet2_cuda as ext
    r = rng(77)
    b, c, n, m = 2, 16, 4096, 1024
    idx_g = dev(skewed_index(r, b, m * 32, n, pad_runs=True, ns=32).reshape(b, m, 32))
    go_g = dev(r.standard_normal((b, c, m, 32), dtype=np.float32))
    idx_i = dev(_three_nn_index(b, n, m, seed=5))
    w = r.random((b, n, 3), dtype=np.float32); w = dev((w / w.sum(-1, keepdims=True)).astype(np.float32))
    go_i = dev(r.standard_normal((b, c, n), dtype=np.float32))
    xy = dev(r.uniform(-1.1, 1.1, size=(b, n, 2)).astype(np.float32))
    go_f = dev(r.standard_normal((b, 64, n), dtype=np.float32))
    xyz = dev(r.standard_normal((b, n, 3), dtype=np.float32))
    new_xyz = xyz[:, :m].contiguous()

    def group():
        out = torch.zeros((b, c, n), device=DEV)
        ext.group_points_grad_wrapper(b, c, n, m, 32, go_g, idx_g, out)
        return out

    def interp():
        out = torch.zeros((b, c, m), device=DEV)
        ext.three_interpolate_grad_wrapper(b, c, n, m, go_i, idx_i, w, out)
        return out

    def fgather():
        out = torch.zeros((b, 64, 48, 160), device=DEV)
        ext.feature_gather_grad_wrapper(b, 64, 48, 160, n, True, go_f, xy, out)
        return out

    def gw():
        out = torch.zeros((c, 3), device=DEV)
        ext.group_linear_grad_w_wrapper(b, c, n, m, 32, go_g, xyz, new_xyz, idx_g, out)
        return out
    return [group, interp, fgather, gw]


def test_four_threads_four_streams_equal_the_lone_runs():
    with deterministic():
        jobs = _det_jobs()
        alone = [j().cpu() for j in jobs]
        torch.cuda.synchronize()
        results, errors = [None] * 4, []

        def worker(k):
            try:
                torch.use_deterministic_algorithms(True)
                s = torch.cuda.Stream(device=DEV)
                outs = []
                with torch.cuda.stream(s):
                    for _ in range(8):
                        outs.append(jobs[k]())
                s.synchronize()
                results[k] = [o.cpu() for o in outs]
            except Exception as e:  # pragma: no cover - reported below
                errors.append(e)
        threads = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    assert not errors, errors
    for k in range(4):
        for o in results[k]:
            same_bits(o.numpy(), alone[k].numpy())


# ---- 4. graph capture ----------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_same_bits():
    with deterministic():
        jobs = _det_jobs()
        eager = [j().cpu() for j in jobs]
        s = torch.cuda.Stream(device=DEV)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for j in jobs:      # warm the caching allocator outside the capture
                j()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = [j() for j in jobs]
        graph.replay()
        torch.cuda.synchronize()
    for o, e in zip(outs, eager):
        same_bits(o.cpu().numpy(), e.numpy())

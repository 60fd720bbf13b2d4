"""The batch sizes the benchmark runs, checked scene by scene, and the batch-dimension boundaries of the ops underneath.

The rest of the suite is dense at small batches. Here:
  * config 2 (the headline) at B = 256, every scene of every tensor against the oracle, each of two resident batches in both
    pipeline roles;
  * config 5 at B = 256, whose grouped tensor holds 18e9 elements (8.4 x 2^31): the oracle on the scenes at the ends of the batch,
    of the point-major gather chunks and on every scene whose slice of an output straddles k * 2^31 elements or bytes; cheap
    device-side consistency checks (int64 gathers, index invariants) on all 256 scenes;
  * op level: the chunk boundaries of the point-major gather (launch_gather_rows_pm), one output past 2^31 elements without the
    stack, grid sizes around every residue of the workgroup count mod the 8 XCDs, and the documented scene-count limit (65535).

Indices and copies are compared for identity; float sums are held to tests/test_gpu_sweep.assert_scatter_sum's bound.
"""
import gc
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import test_gpu_sweep as sweep

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WORKERS = 16             # host threads for the per-scene oracle checks (ctypes releases the GIL while the oracle runs)
BATCH = 256              # bench.py's default batch (bench.py:103)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(autouse=True)
def _release_memory():
    """every case starts and ends with the caching allocator emptied: config 5 alone holds about 80 GB"""
    gc.collect()
    torch.cuda.empty_cache()
    yield
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture
def outputs():
    """the outputs handed to the wrappers, with a canary on either side (conftest.GuardedAlloc; the library's own allocations are
    guarded by conftest's autouse fixture). Also serves test_gpu_sweep's out_tensor() for the sweep bodies run from here."""
    from conftest import GuardedAlloc
    g = GuardedAlloc()
    sweep._CURRENT.append(g)
    yield g
    sweep._CURRENT.pop()
    torch.cuda.synchronize()
    g.check()


def out_tensor(g, shape, dtype=torch.float32, fill=None):
    t = g.alloc(shape, dtype, DEV)
    if fill is not None:
        t.fill_(fill)
    return t


def straddling_scenes(shape, itemsize):
    """scenes (leading dimension) of a contiguous tensor that hold the last element below, or the first element at or above, any
    multiple k >= 1 of 2^31 elements or of 2^31 bytes that the tensor reaches"""
    per_scene = int(np.prod(shape[1:], dtype=np.int64))
    total = int(shape[0]) * per_scene
    out = set()
    for unit in (1 << 31, (1 << 31) // itemsize):
        for k in range(1, (total - 1) // unit + 1):
            e = k * unit
            out.update({(e - 1) // per_scene, e // per_scene})
    return out


def test_straddling_scenes_of_the_config5_grouped_tensor():
    """(the set the config 5 test checks: scene 7 holds byte 2^31, 15 byte 2^32, 30 element 2^31)"""
    s = straddling_scenes((256, 67, 16384, 64), 4)
    assert {7, 15, 30} <= s and max(s) <= 255
    assert straddling_scenes((33, 64, 16384, 64), 4) >= {7, 8, 31, 32}       # (scene 32 starts exactly at element 2^31)
    assert straddling_scenes((4, 4), 4) == set()


def poison(stack):
    """nothing of the capture-time warm-up may survive into a comparison (as test_gpu_parity's test of the bench configuration)"""
    for L in stack.levels:
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


def bench_stack(cfg, with_fp=False):
    """SAStack as bench.py's time_stack builds it on its default line (pipelined, fused sampling, overlap, fused grouping,
    shared scene index, the default two stages), captured on two different resident batches and poisoned"""
    from epnet_amd import sa_stack, synth
    n = cfg["n"]
    batches = [synth.scenes("kitti", BATCH, n, seed=seed).to(DEV) for seed in (1000, 5000)]
    stack = sa_stack.SAStack(BATCH, n=n, device=DEV, with_fp=with_fp, seed=0, npoints=cfg["npoints"], radii=cfg["radii"],
                             nsamples=cfg["nsamples"], feat_channels=cfg["feat_channels"], overlap=True, fused=True,
                             shared_index=True, pipelined=True, fused_sampling=True, stages=2)
    assert stack.stages == 2 and stack.ring == 2
    stack.capture(*batches)
    del batches
    poison(stack)
    return stack


def roles(stack):
    """(batch the last step sampled, batch it grouped) for a two-stage pipelined stack (SAStack.owners, bench.verify_scene)"""
    s_par, g_par = stack.owners()
    return s_par, g_par, stack.inputs[s_par], stack.inputs[g_par]


def verify_scenes(stack, scenes, what):
    """bench.verify_scene on every scene of `scenes`, WORKERS at a time; the failure names each bad scene and its tensors"""
    import bench
    from oracle import oracle
    oracle.build()
    oracle.lib()
    torch.cuda.synchronize()
    _, _, cur, prev = roles(stack)
    with ThreadPoolExecutor(max_workers=WORKERS) as pool:
        results = list(pool.map(lambda s: (s, bench.verify_scene(stack, cur, s, prev_xyz=prev)), sorted(scenes)))
    bad = {s: names for s, names in results if names}
    assert not bad, "%s: %d of %d scenes differ from the oracle -- scene: tensors %s" % (what, len(bad), len(results), bad)


# ---- 1. config 2 at the bench's batch, every scene -----------------------------------------------------------------------------
@pytest.mark.parametrize("with_fp", [False, True])
def test_config2_every_scene_of_the_benchs_batch(oracle, with_fp):
    """bench.py's default line (B = 256, 16384 points, the RPN pyramid): three replays, then every scene of every tensor against
    the oracle; one more replay and the same again, so that each of the two resident batches is checked in both roles"""
    from epnet_amd import sa_stack
    stack = bench_stack(sa_stack.CONFIGS[2], with_fp=with_fp)
    for _ in range(3):
        stack.replay()
    verify_scenes(stack, range(BATCH), "config 2, with_fp=%s, after 3 replays" % with_fp)
    stack.replay()
    verify_scenes(stack, range(BATCH), "config 2, with_fp=%s, after 4 replays" % with_fp)


# ---- 2. config 5 at the bench's batch: the tensors past 2^31 ---------------------------------------------------------------------
def pm_chunk(c, n):
    """scenes per chunk of the point-major gather, as launch_gather_rows_pm computes it (epnet_amd/csrc/group.hip:565)"""
    return max(1, (64 << 20) // (c * n * 4))


def bad_scenes(ok, s0):
    """scene numbers of the False entries of a per-scene bool vector that starts at scene s0"""
    return [s0 + int(i) for i in torch.nonzero(~ok).flatten().tolist()]


def test_config5_at_the_benchs_batch(oracle):
    """sa_stack.CONFIGS[5] at B = 256 (bench.py --config 5): a 72 GB grouped tensor. The oracle on the boundary scenes and on every
    scene whose slice of an output straddles k * 2^31 elements or bytes; device-side consistency of all 256 scenes"""
    from epnet_amd import sa_stack
    cfg = sa_stack.CONFIGS[5]
    n, m, ns, c = cfg["n"], cfg["npoints"][0], cfg["nsamples"][0][0], cfg["feat_channels"][0]
    grouped_bytes = BATCH * (3 + c) * m * ns * 4
    # the grouped tensor, features + point-major workspace, two index sets, four clouds, and room for the checks
    need = grouped_bytes + BATCH * c * n * 4 * 2 + BATCH * m * ns * 4 * 2 + BATCH * n * 3 * 4 * 4 + (8 << 30)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip("config 5 at B = 256 needs %.1f GB of free device memory, %.1f GB are free" % (need / 1e9, free / 1e9))
    stack = bench_stack(cfg)
    for _ in range(3):
        stack.replay()
    torch.cuda.synchronize()
    L = stack.levels[0]
    S = L["scales"][0]
    s_par, g_par, cur, prev = roles(stack)
    assert S["grouped"].shape == (BATCH, 3 + c, m, ns) and S.get("workspace") is not None   # (the point-major path: group.hip:559)

    # the oracle on the boundary scenes: the batch's ends, the XCD map's eighths, the ends of several point-major chunks, and every
    # scene whose slice of an output tensor straddles a multiple of 2^31 elements or bytes (computed from the shapes)
    chunk = pm_chunk(c, n)
    scenes = {0, 1, 7, 8, 127, 128, BATCH - 2, BATCH - 1}
    for k in (1, 15, 16, BATCH // chunk - 1):
        scenes.update({k * chunk - 1, k * chunk})
    outputs_ = [L["fps_idx"], S["grouped"]] + [P["new_xyz"] for P in L["sets"]] + list(S["idx_sets"])
    straddle = set()
    for t in outputs_:
        straddle |= straddling_scenes(tuple(t.shape), t.element_size())
    assert {7, 15, 30} <= straddle
    verify_scenes(stack, scenes | straddle, "config 5 at B = %d" % BATCH)

    # device-side consistency of all 256 scenes, a few at a time: sampling, ball query and every grouped element
    idx_g = S["idx_sets"][g_par] if len(S["idx_sets"]) > 1 else S["idx"]     # the queries stage G grouped with
    centres_s, centres_g = L["sets"][s_par]["new_xyz"], L["sets"][g_par]["new_xyz"]
    failures = {}
    group = 4
    for s0 in range(0, BATCH, group):
        s1 = min(BATCH, s0 + group)
        g = s1 - s0
        f = L["fps_idx"][s0:s1].long()                                       # stage S: the batch `cur`
        srt = f.sort(dim=1).values
        ok_fps = (f[:, 0] == 0) & ((f >= 0) & (f < n)).all(1) & (srt[:, 1:] != srt[:, :-1]).all(1)
        want_c = torch.gather(cur[s0:s1], 1, f.clamp(0, n - 1).unsqueeze(-1).expand(-1, -1, 3))
        ok_centres = (centres_s[s0:s1] == want_c).flatten(1).all(1)
        q = idx_g[s0:s1].long()                                               # stage G: the batch `prev`
        ok_range = ((q >= 0) & (q < n)).flatten(1).all(1)
        # the reference's fill convention: the hits in scan order (strictly increasing), then the first hit repeated
        hits = 1 + (q[..., 1:] > q[..., :-1]).int().cumprod(-1).sum(-1, keepdim=True)
        padded = torch.arange(ns, device=DEV) >= hits
        ok_fill = (~padded | (q == q[..., :1])).flatten(1).all(1)
        qc = q.clamp(0, n - 1).reshape(g, 1, m * ns)
        got = S["grouped"][s0:s1].reshape(g, 3 + c, m * ns)
        want_f = torch.gather(L["features"][s0:s1], 2, qc.expand(-1, c, -1))
        ok_feat = (got[:, 3:] == want_f).flatten(1).all(1)
        del want_f
        rows = torch.gather(prev[s0:s1], 1, qc.reshape(g, m * ns, 1).expand(-1, -1, 3))
        want_x = (rows - centres_g[s0:s1].repeat_interleave(ns, dim=1)).transpose(1, 2)
        ok_xyz = (got[:, :3] == want_x).flatten(1).all(1)
        for name, ok in (("fps_idx", ok_fps), ("new_xyz = xyz[fps_idx]", ok_centres), ("ball_idx range", ok_range),
                         ("ball_idx fill", ok_fill), ("grouped features", ok_feat), ("grouped xyz - centre", ok_xyz)):
            for s in bad_scenes(ok, s0):
                failures.setdefault(s, []).append(name)
    assert not failures, "config 5 at B = %d, device-side checks -- scene: tensors %s" % (BATCH, failures)


# ---- 3. op-level boundaries of the batch dimension -------------------------------------------------------------------------------
def _pm_cases():
    out = []
    for c, n in ((64, 65536), (128, 32768), (16, 20000), (20, 17000)):
        k = pm_chunk(c, n)
        out += [(c, n, b) for b in (k - 1, k, k + 1, 2 * k + 1)]
    return out


@pytest.mark.parametrize("c,n,b", _pm_cases())
def test_point_major_gather_chunks(oracle, outputs, c, n, b):
    """launch_gather_rows_pm works through the batch in chunks of pm_chunk(c, n) scenes: batches one short of a chunk, one chunk,
    one past it and two chunks and one; group_concat (the point-major path) and group_points (launch_gather_rows, whose tiling
    depends on b) against the oracle, every scene"""
    from epnet_amd import pointnet2_cuda as ext
    ns = 16
    m = -(-n // ns)                                  # p = m * ns >= n: the point-major copy pays, the path is taken
    assert ext.group_concat_workspace_bytes(b, c, n, m, ns) == b * c * n * 4
    rng = np.random.default_rng(b * 7 + c)
    xyz = sweep.cloud("kitti", b, n, seed=b + n)
    new_xyz = np.ascontiguousarray(xyz[:, :m])
    feats = rng.standard_normal((b, c, n)).astype(np.float32)
    idx = rng.integers(0, n, size=(b, m, ns)).astype(np.int32)
    idx[:, 0, 0], idx[:, -1, -1] = n - 1, 0          # (the last and the first point of every scene)
    want_f = oracle.group_points(feats, idx)
    want_x = oracle.group_points(np.ascontiguousarray(xyz.transpose(0, 2, 1)), idx) - new_xyz.transpose(0, 2, 1)[..., None]
    d_feats, d_idx = dev(feats), dev(idx)
    out = out_tensor(outputs, (b, 3 + c, m, ns), fill=float("nan"))
    ext.group_concat_wrapper(b, c, n, m, ns, dev(xyz), dev(new_xyz), d_feats, d_idx, out, True)
    got = host(out)
    bad = [s for s in range(b) if not (np.array_equal(got[s, 3:], want_f[s]) and np.array_equal(got[s, :3], want_x[s]))]
    assert not bad, ("group_concat", c, n, b, "scenes", bad)
    only = out_tensor(outputs, (b, c, m, ns), fill=float("nan"))
    ext.group_points_wrapper(b, c, n, m, ns, d_feats, d_idx, only)
    got = host(only)
    bad = [s for s in range(b) if not np.array_equal(got[s], want_f[s])]
    assert not bad, ("group_points", c, n, b, "scenes", bad)


def test_group_points_output_past_2_to_the_31_elements(oracle, outputs):
    """group_points into a (33, 64, 16384, 64) output (2.2e9 elements, 8.9 GB) and its gradient from a grad_out of that shape:
    every scene against an int64 gather / a float64 index_add_ on the device, the straddling scenes and the last one against the
    oracle"""
    from epnet_amd import pointnet2_cuda as ext
    b, c, n, m, ns = 33, 64, 65536, 16384, 64
    p = m * ns
    assert b * c * p > 1 << 31
    g = torch.Generator(device=DEV).manual_seed(31)
    feats = torch.randn((b, c, n), generator=g, device=DEV)
    idx = torch.randint(0, n, (b, m, ns), generator=g, device=DEV, dtype=torch.int32)
    out = out_tensor(outputs, (b, c, m, ns), fill=float("nan"))
    ext.group_points_wrapper(b, c, n, m, ns, feats, idx, out)
    check = sorted(straddling_scenes((b, c, m, ns), 4) | {b - 1})
    bad = []
    for s in range(b):
        want = torch.gather(feats[s], 1, idx[s].reshape(1, p).long().expand(c, -1))
        if not torch.equal(out[s].reshape(c, p), want):
            bad.append(s)
    assert not bad, ("group_points vs int64 gather, scenes", bad)
    for s in check:
        np.testing.assert_array_equal(host(out[s:s + 1]), oracle.group_points(host(feats[s:s + 1]), host(idx[s:s + 1])),
                                      err_msg="group_points, scene %d" % s)
    del out
    torch.cuda.empty_cache()

    grad_out = torch.randn((b, c, m, ns), generator=g, device=DEV)
    grad = out_tensor(outputs, (b, c, n), fill=0.0)
    ext.group_points_grad_wrapper(b, c, n, m, ns, grad_out, idx, grad)
    bad = []
    for s in range(b):
        flat = idx[s].reshape(p).long()
        terms = grad_out[s].reshape(c, p).double()
        want = torch.zeros((c, n), dtype=torch.float64, device=DEV).index_add_(1, flat, terms)
        mag = torch.zeros((c, n), dtype=torch.float64, device=DEV).index_add_(1, flat, terms.abs())
        del terms
        err = (grad[s].double() - want).abs()
        # test_gpu_sweep.assert_scatter_sum's bound, evaluated on the device
        if not bool((err <= 2e-7 * mag + 1e-5 * want.abs().clamp(min=1.0)).all()):
            bad.append((s, float(err.max())))
    assert not bad, ("group_points_grad vs float64 index_add_, (scene, max error)", bad)
    for s in check:
        go = host(grad_out[s:s + 1])
        want = oracle.group_points_grad(go, host(idx[s:s + 1]), n)       # (the oracle's own fp32 sums: test_gpu_sweep's tolerance)
        np.testing.assert_allclose(host(grad[s:s + 1]), want, rtol=1e-3, atol=1e-2 * max(1.0, p / n / 30.0),
                                   err_msg="group_points_grad, scene %d" % s)


_RESIDUE_CASES = (0, 1, 3, 6, 7, 11, 12, 13, 17, 19, 20, 21, 28, 30, 31)   # sweep cases with c * ns <= 64: the oracle's share stays small


def _residue_cases():
    out = []
    for i, (b, n) in enumerate((b, n) for b in (255, 256, 257, 511, 1000) for n in (64, 257, 1024)):
        out.append((_RESIDUE_CASES[i], b, n, sweep.KINDS[i % len(sweep.KINDS)]))
    return out


@pytest.mark.parametrize("case,b,n,kind", _residue_cases())
def test_sa_level_and_fp_twin_at_large_batches(oracle, outputs, case, b, n, kind):
    """test_gpu_sweep.test_sweep_many_scenes (one SA level + its FP twin; every multi-workgroup kernel relabels its grid with
    common.h xcd_scene_map{,3}, a function of the whole grid) at batches larger than the sweep's, covering every residue of the
    workgroup count mod 8; every scene against the oracle"""
    sweep.test_sweep_many_scenes(oracle, case, b, n, kind)


# ---- the documented scene-count limit (launchers: `b > 65535` -> EPNET_ELIMIT) ---------------------------------------------------
_LIM_N, _LIM_C, _LIM_M, _LIM_NS = 8, 4, 2, 2     # a tiny scene; m * ns = 4 positions (the vector / sorted-scatter paths)


def _lim_inputs(b):
    rng = np.random.default_rng(65535)
    n, c, m, ns = _LIM_N, _LIM_C, _LIM_M, _LIM_NS
    xyz = rng.standard_normal((b, n, 3)).astype(np.float32)
    w = rng.random((b, n, 3)).astype(np.float32)
    return {"xyz": xyz, "new_xyz": np.ascontiguousarray(xyz[:, :m]), "feats": rng.standard_normal((b, c, n)).astype(np.float32),
            "idx": rng.integers(0, n, size=(b, m, ns)).astype(np.int32), "gi": rng.integers(0, n, size=(b, m)).astype(np.int32),
            "go": rng.standard_normal((b, 3 + c, m, ns)).astype(np.float32), "gm": rng.standard_normal((b, c, m)).astype(np.float32),
            "nn": rng.integers(0, m, size=(b, n, 3)).astype(np.int32), "w": w / w.sum(-1, keepdims=True),
            "gn": rng.standard_normal((b, c, n)).astype(np.float32), "wx": rng.standard_normal((c, 3)).astype(np.float32),
            "bias": rng.standard_normal((c,)).astype(np.float32), "fmap": rng.standard_normal((b, c, 3, 5)).astype(np.float32),
            "xy": (rng.random((b, n, 2)) * 2.4 - 1.2).astype(np.float32)}


def _grid_sample(fmap, xy):
    """the op the reference calls (bilinear, zero padding, align_corners=True), in the dtype of the feature map tensor"""
    import torch.nn.functional as F
    return F.grid_sample(fmap, torch.from_numpy(xy).to(fmap.dtype).unsqueeze(1), mode="bilinear", padding_mode="zeros",
                         align_corners=True).squeeze(2)


def _lim_case(name, b, g, x, o):
    """(call, outputs, check(scene)) of one wrapper at batch b; x = _lim_inputs(b), o = the oracle"""
    from epnet_amd import pointnet2_cuda as ext
    n, c, m, ns = _LIM_N, _LIM_C, _LIM_M, _LIM_NS
    d = {k: dev(v) for k, v in x.items()}
    sl = lambda a, s: a[s:s + 1]                           # noqa: E731
    if name == "group_points":
        out = out_tensor(g, (b, c, m, ns))
        return (lambda: ext.group_points_wrapper(b, c, n, m, ns, d["feats"], d["idx"], out), [out],
                lambda s: np.testing.assert_array_equal(host(sl(out, s)), o.group_points(sl(x["feats"], s), sl(x["idx"], s))))
    if name == "gather_points":
        out = out_tensor(g, (b, c, m))
        return (lambda: ext.gather_points_wrapper(b, c, n, m, d["feats"], d["gi"], out), [out],
                lambda s: np.testing.assert_array_equal(host(sl(out, s)), o.gather_points(sl(x["feats"], s), sl(x["gi"], s))))
    if name == "group_concat":
        out = out_tensor(g, (b, 3 + c, m, ns))

        def want(s):
            xt = np.ascontiguousarray(sl(x["xyz"], s).transpose(0, 2, 1))
            return np.concatenate([o.group_points(xt, sl(x["idx"], s)) - sl(x["new_xyz"], s).transpose(0, 2, 1)[..., None],
                                   o.group_points(sl(x["feats"], s), sl(x["idx"], s))], axis=1)
        return (lambda: ext.group_concat_wrapper(b, c, n, m, ns, d["xyz"], d["new_xyz"], d["feats"], d["idx"], out, True), [out],
                lambda s: np.testing.assert_array_equal(host(sl(out, s)), want(s)))
    if name in ("group_points_grad", "group_concat_grad"):
        grad = out_tensor(g, (b, c, n))
        if name == "group_points_grad":
            go = d["go"][:, 3:].contiguous()
            call = lambda: ext.group_points_grad_wrapper(b, c, n, m, ns, go, d["idx"], grad)        # noqa: E731
        else:
            call = lambda: ext.group_concat_grad_wrapper(b, c, n, m, ns, d["go"], d["idx"], grad, True)   # noqa: E731
        return (call, [grad], lambda s: sweep.assert_scatter_sum(host(sl(grad, s)), sl(x["go"], s)[:, 3:].reshape(1, c, -1),
                                                                 sl(x["idx"], s).reshape(1, -1).astype(np.int64), n))
    if name == "gather_points_grad":
        grad = out_tensor(g, (b, c, n))
        return (lambda: ext.gather_points_grad_wrapper(b, c, n, m, d["gm"], d["gi"], grad), [grad],
                lambda s: sweep.assert_scatter_sum(host(sl(grad, s)), sl(x["gm"], s), sl(x["gi"], s).astype(np.int64), n))
    if name == "group_linear":
        out = out_tensor(g, (b, c, m, ns))
        return (lambda: ext.group_linear_wrapper(b, c, n, m, ns, d["xyz"], d["new_xyz"], d["gn"], d["idx"], d["wx"], d["bias"], out),
                [out], lambda s: np.testing.assert_array_equal(
                    host(sl(out, s)), o.group_linear(sl(x["xyz"], s), sl(x["new_xyz"], s), sl(x["gn"], s), sl(x["idx"], s), x["wx"],
                                                     x["bias"])))
    if name == "group_linear_grad_w":
        gw = out_tensor(g, (c, 3))
        go = d["go"][:, 3:].contiguous()

        def check(s):          # a sum over ALL scenes: held to test_gpu_sweep.test_sweep_group_linear's bound once
            if s:
                return
            rel = x["xyz"].astype(np.float64)[np.arange(b)[:, None, None], x["idx"].astype(np.int64)] - x["new_xyz"][:, :, None, :]
            gof = x["go"][:, 3:].astype(np.float64)
            want = np.einsum("bcms,bmsk->ck", gof, rel)
            mag = np.einsum("bcms,bmsk->ck", np.abs(gof), np.abs(rel))
            assert (np.abs(host(gw) - want) <= 3e-7 * mag + 1e-5).all()
        return lambda: ext.group_linear_grad_w_wrapper(b, c, n, m, ns, go, d["xyz"], d["new_xyz"], d["idx"], gw), [gw], check
    if name == "three_interpolate":
        out = out_tensor(g, (b, c, n))
        return (lambda: ext.three_interpolate_wrapper(b, c, m, n, d["gm"], d["nn"], d["w"], out), [out],
                lambda s: np.testing.assert_array_equal(host(sl(out, s)), o.three_interpolate(sl(x["gm"], s), sl(x["nn"], s), sl(x["w"], s))))
    if name == "three_interpolate_grad":
        grad = out_tensor(g, (b, c, m))
        return (lambda: ext.three_interpolate_grad_wrapper(b, c, n, m, d["gn"], d["nn"], d["w"], grad), [grad],
                lambda s: sweep.assert_scatter_sum(host(sl(grad, s)), (sl(x["gn"], s)[:, :, :, None] * sl(x["w"], s)[:, None]).reshape(1, c, n * 3),
                                                   sl(x["nn"], s).reshape(1, -1).astype(np.int64), m))
    if name == "feature_gather":
        out = out_tensor(g, (b, c, n))
        return (lambda: ext.feature_gather_wrapper(b, c, 3, 5, n, n, True, d["fmap"], d["xy"], None, out, None), [out],
                lambda s: np.testing.assert_allclose(host(sl(out, s)), _grid_sample(torch.from_numpy(sl(x["fmap"], s)), sl(x["xy"], s)).numpy(),
                                                     rtol=1e-5, atol=1e-5))     # (test_gpu_sweep.test_sweep_feature_gather, align_corners)
    if name == "feature_gather_grad":
        grad = out_tensor(g, (b, c, 3, 5))

        def check(s):
            fm = torch.from_numpy(sl(x["fmap"], s)).double().requires_grad_(True)
            want, = torch.autograd.grad(_grid_sample(fm, sl(x["xy"], s)), fm, torch.from_numpy(sl(x["gn"], s)).double())
            scale = max(1.0, float(want.abs().max()))
            np.testing.assert_allclose(host(sl(grad, s)), want.numpy(), rtol=1e-4, atol=1e-4 * scale)
        return lambda: ext.feature_gather_grad_wrapper(b, c, 3, 5, n, True, d["gn"], d["xy"], grad), [grad], check
    raise ValueError(name)


_LIMIT_WRAPPERS = ("group_points", "gather_points", "group_concat", "group_points_grad", "gather_points_grad", "group_concat_grad",
                   "group_linear", "group_linear_grad_w", "three_interpolate", "three_interpolate_grad", "feature_gather",
                   "feature_gather_grad")


@pytest.mark.parametrize("name", _LIMIT_WRAPPERS)
def test_scene_count_limit(oracle, outputs, name):
    """b = 65535 (the largest grid dimension the launchers accept) works -- first, middle and last scene against the oracle --
    and b = 65536 raises RuntimeError before anything is launched: the output keeps what it held"""
    lim = 65535
    x = _lim_inputs(lim + 1)
    call, outs, check = _lim_case(name, lim, outputs, {k: v[:lim] if v.ndim > 1 and v.shape[0] == lim + 1 else v for k, v in x.items()},
                                  oracle)
    for t in outs:
        t.fill_(0.0 if name.endswith("grad") or name.endswith("grad_w") else float("nan"))
    call()
    torch.cuda.synchronize()
    for s in (0, lim // 2, lim - 1):
        check(s)
    call, outs, _ = _lim_case(name, lim + 1, outputs, x, oracle)
    for t in outs:
        t.fill_(7.25)
    with pytest.raises(RuntimeError, match="outside the supported range"):
        call()
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == 7.25).all()), (name, "an output was written past the limit")


# ---- the deterministic gradients (include/epnet_ops.h "*_det") at the bench's batch, past 2^31 and at the scene-count limit ----------
def _det_oracle():
    from oracle import oracle
    oracle.build()
    oracle.lib()
    return oracle


# (op, n targets, npoints / unknowns, nsample, channels): config 2's level 1 (16384 -> 4096 x 16 / 32) and level 2 (4096 -> 1024 x 32)
# groupings and its last FP module (16384 unknowns, 4096 known). Level 1 groups coordinates only in the bench, and the FP module's
# 256 channels would pass 4 GB of host copies: 17 / 9 / 65 channels there (>= 9 and no multiple of 8: partial fold rows)
_DET_BATCH = (("group_points_grad", 16384, 4096, 16, 17), ("group_points_grad", 16384, 4096, 32, 9),
              ("group_concat_grad", 16384, 4096, 16, 17), ("group_concat_grad", 16384, 4096, 32, 9),
              ("group_points_grad", 4096, 1024, 32, 96), ("group_concat_grad", 4096, 1024, 32, 96),
              ("three_interpolate_grad", 4096, 16384, 3, 65))


@pytest.mark.parametrize("op,n,m,ns,c", _DET_BATCH, ids=["%s_n%d_m%d_ns%d_c%d" % k for k in _DET_BATCH])
def test_det_gradients_at_the_benchs_batch(outputs, op, n, m, ns, c):
    """the deterministic gradients of config 2's shapes at B = 256 from a nonzero buffer, every scene bit for bit the oracle's loop"""
    from epnet_amd import pointnet2_cuda as ext
    from test_deterministic_gpu import deterministic, oracle_group_grad, oracle_interp_grad, same_bits
    o = _det_oracle()
    b = BATCH
    g = torch.Generator(device=DEV).manual_seed(m + ns + c)
    ch0 = 3 if op == "group_concat_grad" else 0
    start = torch.randn((b, c, n), generator=g, device=DEV)
    grad = out_tensor(outputs, (b, c, n))
    grad.copy_(start)
    if op == "three_interpolate_grad":
        idx = torch.randint(0, n, (b, m, 3), generator=g, device=DEV, dtype=torch.int32)
        w = torch.rand((b, m, 3), generator=g, device=DEV)
        w = (w / w.sum(-1, keepdim=True)).contiguous()
        go = torch.randn((b, c, m), generator=g, device=DEV)
        with deterministic():
            ext.three_interpolate_grad_wrapper(b, c, m, n, go, idx, w, grad)
    else:
        idx = torch.randint(0, n, (b, m, ns), generator=g, device=DEV, dtype=torch.int32)
        idx[:, :, ns // 2:] = idx[:, :, :1]                      # ball-query padding: the first hit repeated
        go = torch.randn((b, ch0 + c, m, ns), generator=g, device=DEV)
        with deterministic():
            if op == "group_points_grad":
                ext.group_points_grad_wrapper(b, c, n, m, ns, go, idx, grad)
            else:
                ext.group_concat_grad_wrapper(b, c, n, m, ns, go, idx, grad, True)
    torch.cuda.synchronize()
    got, s_h, go_h, idx_h = host(grad), host(start), host(go), host(idx)
    w_h = host(w) if op == "three_interpolate_grad" else None
    del go, start

    def scene(s):
        sl = slice(s, s + 1)
        if op == "three_interpolate_grad":
            want = oracle_interp_grad(o, s_h[sl], go_h[sl], idx_h[sl], w_h[sl])
        else:
            want = oracle_group_grad(o, s_h[sl], go_h[sl, ch0:], idx_h[sl])
        try:
            same_bits(got[sl], want)
        except AssertionError:
            return s
        return None
    with ThreadPoolExecutor(max_workers=WORKERS) as pool:
        bad = [s for s in pool.map(scene, range(b)) if s is not None]
    assert not bad, "%s at B = %d: %d scenes differ from the oracle's loop: %s" % (op, b, len(bad), bad)


def test_group_points_grad_det_past_2_to_the_31_elements(outputs):
    """the deterministic group_points_grad from the (33, 64, 16384, 64) grad_out of test_group_points_output_past_2_to_the_31_elements
    (2.2e9 elements): every scene against a float64 index_add_ on the device, the straddling scenes and both ends bit for bit"""
    from epnet_amd import pointnet2_cuda as ext
    from test_deterministic_gpu import deterministic, oracle_group_grad, same_bits
    o = _det_oracle()
    b, c, n, m, ns = 33, 64, 65536, 16384, 64
    p = m * ns
    assert b * c * p > 1 << 31
    g = torch.Generator(device=DEV).manual_seed(32)
    idx = torch.randint(0, n, (b, m, ns), generator=g, device=DEV, dtype=torch.int32)
    grad_out = torch.randn((b, c, m, ns), generator=g, device=DEV)
    start = torch.randn((b, c, n), generator=g, device=DEV)
    grad = out_tensor(outputs, (b, c, n))
    grad.copy_(start)
    with deterministic():
        ext.group_points_grad_wrapper(b, c, n, m, ns, grad_out, idx, grad)
    bad = []
    for s in range(b):
        flat = idx[s].reshape(p).long()
        terms = grad_out[s].reshape(c, p).double()
        want = start[s].double().index_add_(1, flat, terms)
        mag = start[s].double().abs().index_add_(1, flat, terms.abs())
        del terms
        err = (grad[s].double() - want).abs()
        if not bool((err <= 2e-7 * mag + 1e-5 * want.abs().clamp(min=1.0)).all()):      # test_gpu_sweep.assert_scatter_sum's bound
            bad.append((s, float(err.max())))
    assert not bad, ("group_points_grad (deterministic) vs float64 index_add_, (scene, max error)", bad)
    for s in sorted(straddling_scenes((b, c, m, ns), 4) | {0, b - 1}):
        sl = slice(s, s + 1)
        same_bits(host(grad[sl]), oracle_group_grad(o, host(start[sl]), host(grad_out[sl]), host(idx[sl])))


def _det_lim_case(name, b, g, x, o):
    """(call, outputs, check(scene)) of one deterministic gradient at batch b, from a nonzero buffer; the check is the contract,
    bit for bit (group_linear_grad_w: its sum over all scenes, once)"""
    import det_restate as R
    from epnet_amd import pointnet2_cuda as ext
    from test_deterministic_gpu import oracle_gather_grad, oracle_group_grad, oracle_interp_grad, same_bits
    n, c, m, ns = _LIM_N, _LIM_C, _LIM_M, _LIM_NS
    d = {k: dev(v) for k, v in x.items()}
    sl = lambda a, s: a[s:s + 1]                           # noqa: E731
    starts = {"group_linear_grad_w": x["wx"], "three_interpolate_grad": x["gm"], "feature_gather_grad": x["fmap"]}
    start = starts.get(name, x["feats"])
    out = out_tensor(g, start.shape)
    out.copy_(torch.from_numpy(start))

    def bits(want):
        return lambda s: same_bits(host(sl(out, s)), want(s))
    if name == "group_points_grad":
        go = d["go"][:, 3:].contiguous()
        return (lambda: ext.group_points_grad_wrapper(b, c, n, m, ns, go, d["idx"], out), [out],
                bits(lambda s: oracle_group_grad(o, sl(start, s), sl(x["go"], s)[:, 3:], sl(x["idx"], s))))
    if name == "group_concat_grad":
        return (lambda: ext.group_concat_grad_wrapper(b, c, n, m, ns, d["go"], d["idx"], out, True), [out],
                bits(lambda s: oracle_group_grad(o, sl(start, s), sl(x["go"], s)[:, 3:], sl(x["idx"], s))))
    if name == "gather_points_grad":
        return (lambda: ext.gather_points_grad_wrapper(b, c, n, m, d["gm"], d["gi"], out), [out],
                bits(lambda s: oracle_gather_grad(o, sl(start, s), sl(x["gm"], s), sl(x["gi"], s))))
    if name == "three_interpolate_grad":
        return (lambda: ext.three_interpolate_grad_wrapper(b, c, n, m, d["gn"], d["nn"], d["w"], out), [out],
                bits(lambda s: oracle_interp_grad(o, sl(start, s), sl(x["gn"], s), sl(x["nn"], s), sl(x["w"], s))))
    if name == "feature_gather_grad":
        return (lambda: ext.feature_gather_grad_wrapper(b, c, 3, 5, n, True, d["gn"], d["xy"], out), [out],
                bits(lambda s: R.feature_gather_grad(sl(start, s), sl(x["gn"], s), sl(x["xy"], s), True)))
    if name == "group_linear_grad_w":
        go = d["go"][:, 3:].contiguous()

        def check(s):
            if s == 0:
                same_bits(host(out), R.group_linear_grad_w(start, np.ascontiguousarray(x["go"][:, 3:]), x["xyz"], x["new_xyz"], x["idx"]))
        return lambda: ext.group_linear_grad_w_wrapper(b, c, n, m, ns, go, d["xyz"], d["new_xyz"], d["idx"], out), [out], check
    raise ValueError(name)


@pytest.mark.parametrize("name", ("gather_points_grad", "group_points_grad", "group_concat_grad", "three_interpolate_grad",
                                  "feature_gather_grad", "group_linear_grad_w"))
def test_scene_count_limit_det(outputs, name):
    """test_scene_count_limit under torch.use_deterministic_algorithms(True): b = 65535 runs its *_det entry point, scenes 0, 32767
    and 65534 are the contract's bits; b = 65536 raises a RuntimeError that names the op and leaves the output as it was"""
    from test_deterministic_gpu import deterministic
    o = _det_oracle()
    lim = 65535
    x = _lim_inputs(lim + 1)
    call, outs, check = _det_lim_case(name, lim, outputs, {k: v[:lim] if v.ndim > 1 and v.shape[0] == lim + 1 else v for k, v in x.items()}, o)
    with deterministic():
        call()
    torch.cuda.synchronize()
    for s in (0, lim // 2, lim - 1):
        check(s)
    call, outs, _ = _det_lim_case(name, lim + 1, outputs, x, o)
    for t in outs:
        t.fill_(7.25)
    with deterministic(), pytest.raises(RuntimeError, match=name):
        call()
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == 7.25).all()), (name, "an output was written past the limit")

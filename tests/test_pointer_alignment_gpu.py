"""Every kernel, and every branch inside one, that the library picks from a pointer's alignment, run with pointers OFF a 16-byte
boundary (tests/offset_alloc.py) at shapes where every length condition of the vector path holds.

Per dispatch site the op runs on the same values with all pointers aligned, with each listed pointer 4 bytes off alone, with all
of them 4 bytes off, with all of them 8 and 12 bytes off, and with every tensor of the call off its boundary. Asserted each time:

  a. the result equals the reference the op's own test uses, under that test's rule (exact equality for the copies, the pool,
     the integer outputs, the labels against their restatement and three_interpolate against the oracle; handover_cases.check
     for the decode; the loss sweep's bound rule for the box loss);
  b. the result has the bits of the all-aligned run. That also holds where (a) is a tolerance: the decode and the box loss stage
     their tile into LDS (vector or scalar loads, the same values in the same slots) and do all per-row arithmetic from there,
     so the two paths evaluate the same expression on the same numbers;
  c. the canaries around every tensor are intact and no output element still holds its sentinel.

The hardware tolerates misaligned vector access to global memory, so a vector path whose guard forgets a pointer does not
fault: it shows as a wrong value or a stray write, which (a) - (c) catch.

Which case reaches which fallback (kernels of their own show in profiles/pointer_alignment_kernel_stats.csv, branches do not):
  pool_max_row_kernel at a power-of-two nsample .......... test_pool_max, x + 4
  pool_max_grad_kernel at nsample % 4 == 0 ............... test_pool_max_grad, grad_x + 4
  gather_rows_scalar_kernel at p % 4 == 0 ................ test_row_gathers, idx + 4 / out + 4
  gather_rows_lds_kernel<false>, scalar staging branch ... test_row_gathers (c = 8, 12), points + 4
  gather_rows_lds_kernel<false>, vector staging branch ... test_row_gathers (c = 10), aligned
  group_xyz_centred_kernel at nsample % 4 == 0 ........... test_group_concat_coordinate_rows, idx + 4 / out + 4
  gather_rows_pm_kernel, non-wide write-back, full tiles . test_group_concat_point_major, out + 4
  epnet_group_concat_ws -> plain path .................... test_group_concat_point_major, workspace + 4
  gather_rows_lds2_kernel<false> (non-quad) .............. test_group_concat_multi, features + 4
  group_concat_multi, non-fused form ..................... test_group_concat_multi, idx[1] + 4 / out[0] + 4
  group_linear_lds_kernel, scalar staging branch ......... test_group_linear, z + 4
  group_linear_scalar_kernel at nsample % 4 == 0 ......... test_group_linear, idx + 4 / out + 4
  three_interpolate_lds_kernel, scalar staging branch .... test_three_interpolate (n = 1024), points + 4
  three_interpolate_kernel, scalar stores ................ test_three_interpolate (n = 8, 256, 1024), out + 4
  gather_centres_kernel at m % 4 == 0 .................... test_sample_centres, idx + 4 / new_xyz + 4
  rpn_targets_kernel<false> at n % 4 == 0 ................ test_rpn_targets, any pointer + 4
  decode_kernel, scalar staging loop ..................... test_decode*, pred_reg + 4
  box loss rows_kernel, p.vec == 0: zero fill, staging,
  write-back ............................................. test_box_loss*, pred_reg + 4 / grad_reg + 4
  image_normalise_kernel<false> at w % 4 == 0 ............ test_image_normalise, out + 4
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import handover_cases as hc
import loss_restate as lr
import offset_alloc as oa
import rpn_targets_restate as rts
import scan_restate as srs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, I32, I64, U8 = torch.float32, torch.int32, torch.int64, torch.uint8


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded(hiplib):
    assert torch.cuda.is_available()
    return hiplib


@pytest.fixture(autouse=True)
def _canaries_of_every_test():
    oa.forget()
    yield
    oa.check()


# ---- the runner ------------------------------------------------------------------------------------------------------------------
def variants(names):
    """(tag, {name: skew}): aligned; each pointer 4 bytes off alone; all of them 4 off; all 8 off; all 12 off"""
    yield "aligned", {}
    if len(names) > 1:
        for n in names:
            yield n + "+4", {n: 4}
    for skew in (4, 8, 12):
        yield "all+%d" % skew, {n: skew for n in names}


def run(inputs, outputs, call, skews, scratch=None):
    """inputs: name -> (array, dtype) or None; outputs: name -> (shape, dtype) or None; scratch: name -> bytes; call(tensors).
    -> name -> host array"""
    t = {k: oa.output((nbytes,), U8, skews.get(k, 0)) for k, nbytes in (scratch or {}).items()}
    for k, v in inputs.items():
        t[k] = None if v is None else oa.skewed(v[0], v[1], skews.get(k, 0))
    for k, v in outputs.items():
        t[k] = None if v is None else oa.output(v[0], v[1], skews.get(k, 0))
    assert all(t[k].data_ptr() % 16 == s for k, s in skews.items())
    call(t)
    oa.check()
    for k, v in inputs.items():        # the inputs are as they were
        if v is not None:
            want = v[0] if isinstance(v[0], torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v[0]))
            assert t[k].cpu().numpy().tobytes() == want.to(v[1]).numpy().tobytes(), ("an input changed", k)
    for k, v in outputs.items():
        if v is not None:
            assert oa.unwritten(t[k]) == 0, ("elements never written", k, oa.unwritten(t[k]))
    return {k: t[k].cpu().numpy() for k, v in outputs.items() if v is not None}


def sweep(inputs, outputs, call, names, reference, what, scratch=None):
    """all variants; reference(got, tag) asserts (a); (b) against the aligned run; (c) inside run(). Last, EVERY tensor of the
    call off its boundary, the pointers no guard looks at included (4 bytes; an int64 tensor 8, as a slice of one would be): a
    vector access nobody guards shows here"""
    base = None
    everything = {k: (8 if v[1] == I64 else 4) for k, v in list(inputs.items()) + list(outputs.items()) if v is not None}
    everything.update({k: 4 for k in (scratch or {})})
    for tag, skews in list(variants(names)) + [("everything+4", everything)]:
        got = run(inputs, outputs, call, skews, scratch)
        reference(got, (what, tag))
        if base is None:
            base = got
        for k in got:
            assert got[k].tobytes() == base[k].tobytes(), (what, tag, k, "differs from the aligned run")


def same(got, want, tag):
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, got.dtype, want.shape, want.dtype)
    np.testing.assert_array_equal(got, want, err_msg=str(tag))


def cloud(b, n, seed, kind="kitti"):
    from epnet_amd import synth
    return synth.scenes(kind, b, n, seed=seed).numpy()


# ---- the pool ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_arg", [True, False])
@pytest.mark.parametrize("ns", [4, 32, 256])
def test_pool_max(ns, with_arg):
    """37 rows (ten blocks of the row kernel; no multiple of the vector kernels' rows per pass); random values, the ties data of
    test_pool.py (ReLU zeros and repeated columns: the first position wins) with two planted ties, and one NaN row; reference:
    F.max_pool2d and the index it records"""
    from epnet_amd import pointnet2_cuda as ext
    from test_pool import data
    rows = 37
    for ties in (False, True):
        x = data((1, 1, rows, ns), 5, ties).clone()
        x[0, 0, 11, ns // 3] = float("nan")
        if ties:                        # and the row maximum twice, in different lanes of the row kernel where the row has them
            x[0, 0, 5, 1] = x[0, 0, 5, ns - 1] = 9.0
            x[0, 0, 6, ns - 2] = x[0, 0, 6, 2] = 9.0
        want, where = F.max_pool2d(x, kernel_size=[1, ns], return_indices=True)
        want_v, want_a = want.reshape(rows).numpy(), (where.reshape(rows) % ns).to(I32).numpy()
        assert np.isnan(want_v[11]) and want_a[11] == ns // 3
        if ties:
            assert int((x[0, 0] == want.reshape(rows, 1)).sum(dim=1).max()) > 1 and want_a[5] == 1 and want_a[6] == min(2, ns - 2)

        def reference(got, tag):
            same(got["out"], want_v, tag)
            if with_arg:
                same(got["arg"], want_a, tag)
        sweep({"x": (x.reshape(rows, ns), F32)}, {"out": ((rows,), F32), "arg": ((rows,), I32) if with_arg else None},
              lambda t: ext.pool_max_wrapper(rows, ns, t["x"], t["out"], t["arg"]), ["x"], reference, ("pool_max", ns, ties))


@pytest.mark.parametrize("ns", [4, 32, 256])
def test_pool_max_grad(oracle, ns):
    from epnet_amd import pointnet2_cuda as ext
    rows = 37
    rng = np.random.default_rng(ns)
    arg = rng.integers(0, ns, rows).astype(np.int32)
    arg[0], arg[1], arg[rows - 1] = 0, ns - 1, ns - 1
    g = rng.standard_normal(rows).astype(np.float32)
    want = oracle.pool_max_grad(g, arg, ns)
    sweep({"grad_out": (g, F32), "arg": (arg, I32)}, {"grad_x": ((rows, ns), F32)},
          lambda t: ext.pool_max_grad_wrapper(rows, ns, t["grad_out"], t["arg"], t["grad_x"]), ["grad_x"],
          lambda got, tag: same(got["grad_x"], want, tag), ("pool_max_grad", ns))


# ---- the row gathers ---------------------------------------------------------------------------------------------------------------
def gather_inputs(b, c, n, m, ns, seed):
    rng = np.random.default_rng(seed)
    feats = rng.standard_normal((b, c, n)).astype(np.float32)
    idx = rng.integers(0, n, (b, m, ns)).astype(np.int32)
    idx[:, 0, 0], idx[:, -1, -1] = n - 1, 0          # the ends of the rows are read
    return feats, idx


@pytest.mark.parametrize("c", [3, 8, 10, 12])
def test_row_gathers(oracle, c):
    """b = 2, n = 64, p = 2048 positions (the least the staged gather takes). c = 8, 12: four rows per LDS word; c = 10: rows
    staged one by one with 16-byte loads; c = 3: the few-channel kernel. group_points and gather_points share the launch."""
    from epnet_amd import pointnet2_cuda as ext
    b, n, m, ns = 2, 64, 128, 16
    feats, idx = gather_inputs(b, c, n, m, ns, seed=c)
    want = oracle.group_points(feats, idx)
    sweep({"points": (feats, F32), "idx": (idx, I32)}, {"out": ((b, c, m, ns), F32)},
          lambda t: ext.group_points_wrapper(b, c, n, m, ns, t["points"], t["idx"], t["out"]), ["points", "idx", "out"],
          lambda got, tag: same(got["out"], want, tag), ("group_points", c))
    flat = np.ascontiguousarray(idx.reshape(b, m * ns))
    want_flat = oracle.gather_points(feats, flat)
    sweep({"points": (feats, F32), "idx": (flat, I32)}, {"out": ((b, c, m * ns), F32)},
          lambda t: ext.gather_points_wrapper(b, c, n, m * ns, t["points"], t["idx"], t["out"]), ["points", "idx", "out"],
          lambda got, tag: same(got["out"], want_flat, tag), ("gather_points", c))


def concat_reference(oracle, xyz, centres, feats, idx):
    parts = [oracle.group_points(np.ascontiguousarray(xyz.transpose(0, 2, 1)), idx) - centres.transpose(0, 2, 1)[..., None]]
    if feats is not None:
        parts.append(oracle.group_points(feats, idx))
    return np.concatenate(parts, axis=1)


@pytest.mark.parametrize("c", [8, 12])
def test_group_concat_feature_rows(oracle, c):
    """the feature rows of group_concat land in a channel slice of the output (behind the three coordinate rows)"""
    from epnet_amd import pointnet2_cuda as ext
    b, n, m, ns = 2, 64, 128, 16
    feats, idx = gather_inputs(b, c, n, m, ns, seed=100 + c)
    xyz = cloud(b, n, seed=c)
    centres = np.ascontiguousarray(xyz[:, np.arange(m) % n])
    want = concat_reference(oracle, xyz, centres, feats, idx)
    sweep({"xyz": (xyz, F32), "new_xyz": (centres, F32), "features": (feats, F32), "idx": (idx, I32)}, {"out": ((b, 3 + c, m, ns), F32)},
          lambda t: ext.group_concat_wrapper(b, c, n, m, ns, t["xyz"], t["new_xyz"], t["features"], t["idx"], t["out"], True),
          ["features", "idx", "out"], lambda got, tag: same(got["out"], want, tag), ("group_concat", c))


def test_group_concat_coordinate_rows(oracle):
    from epnet_amd import pointnet2_cuda as ext
    b, n, m, ns = 2, 50, 9, 4
    rng = np.random.default_rng(9)
    xyz = cloud(b, n, seed=9)
    centres = np.ascontiguousarray(xyz[:, rng.permutation(n)[:m]])
    idx = rng.integers(0, n, (b, m, ns)).astype(np.int32)
    idx[:, 0, 0], idx[:, -1, -1] = n - 1, 0
    want = concat_reference(oracle, xyz, centres, None, idx)
    sweep({"xyz": (xyz, F32), "new_xyz": (centres, F32), "idx": (idx, I32)}, {"out": ((b, 3, m, ns), F32)},
          lambda t: ext.group_concat_wrapper(b, 0, n, m, ns, t["xyz"], t["new_xyz"], None, t["idx"], t["out"], True),
          ["idx", "out"], lambda got, tag: same(got["out"], want, tag), "group_concat coordinates")


def test_group_concat_point_major(oracle):
    """rows beyond LDS (n > 16384) through the caller's scratch: one scene, c = 16, p = 129 * 128 >= n positions, so that every
    tile of the point-major gather is full and its 16-byte write-back depends on `out` alone. A scratch pointer off the
    boundary sends the call down the plain path: the same bits."""
    from epnet_amd import pointnet2_cuda as ext
    b, c, n, m, ns = 1, 16, 16388, 129, 128
    nbytes = ext.group_concat_workspace_bytes(b, c, n, m, ns)
    assert nbytes == b * c * n * 4 and (m * ns) % 128 == 0 and m * ns >= n
    feats, idx = gather_inputs(b, c, n, m, ns, seed=16)
    xyz = cloud(b, n, seed=16)
    centres = np.ascontiguousarray(xyz[:, :m])
    want = concat_reference(oracle, xyz, centres, feats, idx)
    sweep({"xyz": (xyz, F32), "new_xyz": (centres, F32), "features": (feats, F32), "idx": (idx, I32)}, {"out": ((b, 3 + c, m, ns), F32)},
          lambda t: ext.group_concat_wrapper(b, c, n, m, ns, t["xyz"], t["new_xyz"], t["features"], t["idx"], t["out"], True, t["workspace"]),
          ["out", "workspace"], lambda got, tag: same(got["out"], want, tag), "group_concat through scratch", scratch={"workspace": nbytes})


def test_group_concat_multi(oracle):
    """two scales, c = 8, 64 x (16 + 32) = 3072 positions together (kGatherLds2MinPositions), 512 scenes of one row chunk each
    (the staged two-scale kernel wants a full chip). Skewed features: the staged kernel without the four-rows-per-word layout;
    a skewed idx[k] or out[k]: one plain group_concat per scale."""
    from epnet_amd import pointnet2_cuda as ext
    b, c, n, m, nss = 512, 8, 64, 64, (16, 32)
    rng = np.random.default_rng(3)
    xyz = rng.uniform(-20.0, 20.0, (b, n, 3)).astype(np.float32)
    centres = np.ascontiguousarray(xyz[:, rng.permutation(n)[:m]])
    feats = rng.standard_normal((b, c, n)).astype(np.float32)
    idxs = [rng.integers(0, n, (b, m, ns)).astype(np.int32) for ns in nss]
    for i in idxs:
        i[:, 0, 0], i[:, -1, -1] = n - 1, 0
    wants = [concat_reference(oracle, xyz, centres, feats, i) for i in idxs]

    def reference(got, tag):
        same(got["out0"], wants[0], tag)
        same(got["out1"], wants[1], tag)
    sweep({"xyz": (xyz, F32), "new_xyz": (centres, F32), "features": (feats, F32), "idx0": (idxs[0], I32), "idx1": (idxs[1], I32)},
          {"out0": ((b, 3 + c, m, nss[0]), F32), "out1": ((b, 3 + c, m, nss[1]), F32)},
          lambda t: ext.group_concat_multi_wrapper(b, c, n, m, list(nss), t["xyz"], t["new_xyz"], t["features"], [t["idx0"], t["idx1"]],
                                                   [t["out0"], t["out1"]], True),
          ["features", "idx1", "out0"], reference, "group_concat_multi")


def test_group_linear(oracle):
    from epnet_amd import pointnet2_cuda as ext
    b, c, n, m, ns = 2, 8, 64, 64, 16                  # p = 1024: the least the staged kernel takes
    rng = np.random.default_rng(8)
    z, idx = gather_inputs(b, c, n, m, ns, seed=8)
    xyz = cloud(b, n, seed=8)
    centres = np.ascontiguousarray(xyz[:, rng.permutation(n)[:m]])
    w = rng.standard_normal((c, 3)).astype(np.float32)
    bias = rng.standard_normal(c).astype(np.float32)
    for with_bias in (False, True):
        want = oracle.group_linear(xyz, centres, z, idx, w, bias if with_bias else None)
        sweep({"xyz": (xyz, F32), "new_xyz": (centres, F32), "z": (z, F32), "idx": (idx, I32), "w": (w, F32),
               "bias": (bias, F32) if with_bias else None}, {"out": ((b, c, m, ns), F32)},
              lambda t: ext.group_linear_wrapper(b, c, n, m, ns, t["xyz"], t["new_xyz"], t["z"], t["idx"], t["w"], t["bias"], t["out"]),
              ["z", "idx", "out"], lambda got, tag: same(got["out"], want, tag), ("group_linear", with_bias))


@pytest.mark.parametrize("n", [8, 256, 1024])
def test_three_interpolate(oracle, n):
    """c = 8, m = 64 known points. n = 1024: the staged kernels (four rows per LDS word, or row by row when `points` is off the
    boundary; the direct kernel when `out` is); n = 256: the coarse-level kernel; n = 8: the direct kernel, whose 16-byte store
    depends on `out`. Exact against the oracle: the same products and sums in the same order on every path (no contraction)."""
    from epnet_amd import pointnet2_cuda as ext
    b, c, m = 2, 8, 64
    rng = np.random.default_rng(n)
    pts = rng.standard_normal((b, c, m)).astype(np.float32)
    idx = rng.integers(0, m, (b, n, 3)).astype(np.int32)
    idx[:, 0, 0], idx[:, -1, -1] = m - 1, 0
    w = rng.random((b, n, 3)).astype(np.float32)
    want = oracle.three_interpolate(pts, idx, w)
    sweep({"points": (pts, F32), "idx": (idx, I32), "weight": (w, F32)}, {"out": ((b, c, n), F32)},
          lambda t: ext.three_interpolate_wrapper(b, c, m, n, t["points"], t["idx"], t["weight"], t["out"]),
          ["points", "out"], lambda got, tag: same(got["out"], want, tag), ("three_interpolate", n))


# ---- the centre gather -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,indexed", [(40, False), (64, False), (1000, False), (1025, False), (1025, True), (16385, False), (16385, True)])
def test_sample_centres(oracle, n, indexed):
    """m = 8 centres (m % 4 == 0). The smallest n of every sampling path: 40 (fewer points than a wave: the streaming kernel),
    64 and 1000 (fps_wave_kernel, which writes new_xyz itself), 1025 (the pruned kernel, or the indexed one over a scene index),
    16385 (the streaming kernel without an index, the big-scene kernel with one); all but fps_wave_kernel's end in the centre
    gather, whose four-centres-per-thread form depends on idx and new_xyz"""
    from epnet_amd import pointnet2_cuda as ext
    b, m = 2, 8
    xyz = cloud(b, n, seed=n)
    want_idx = oracle.furthest_point_sampling(xyz, m)
    want_xyz = np.take_along_axis(xyz, want_idx[:, :, None].astype(np.int64), axis=1)

    def call(t):
        index = ext.scene_index(t["xyz"]) if indexed else None
        assert (index is not None) == indexed
        ext.sample_centres_wrapper(b, n, m, t["xyz"], index, t["idx"], t["new_xyz"])

    def reference(got, tag):
        same(got["idx"], want_idx, tag)
        same(got["new_xyz"], want_xyz, tag)
    sweep({"xyz": (xyz, F32)}, {"idx": ((b, m), I32), "new_xyz": ((b, m, 3), F32)}, call, ["idx", "new_xyz"], reference, ("sample_centres", n, indexed))


# ---- the ops without a guard: black box ----------------------------------------------------------------------------------------------
def test_furthest_point_sampling_black_box(oracle):
    from epnet_amd import pointnet2_cuda as ext
    b, n, m = 2, 300, 20
    xyz = cloud(b, n, seed=1)
    want = oracle.furthest_point_sampling(xyz, m)
    sweep({"points": (xyz, F32)}, {"idx": ((b, m), I32)},
          lambda t: ext.furthest_point_sampling_wrapper(b, n, m, t["points"], oa.skewed(np.full((b, n), 1e10, np.float32), F32, t["points"].data_ptr() % 16), t["idx"]),
          ["points", "idx"], lambda got, tag: same(got["idx"], want, tag), "furthest_point_sampling")


@pytest.mark.parametrize("n", [500, 2048])
def test_ball_query_black_box(oracle, n):
    from epnet_amd import pointnet2_cuda as ext
    b, m, ns, radius = 2, 24, 12, 2.0
    xyz = cloud(b, n, seed=n)
    centres = np.ascontiguousarray(xyz[:, ::n // m][:, :m])
    want = oracle.ball_query(radius, ns, xyz, centres)
    sweep({"xyz": (xyz, F32), "new_xyz": (centres, F32)}, {"idx": ((b, m, ns), I32)},
          lambda t: ext.ball_query_wrapper(b, n, m, radius, ns, t["new_xyz"], t["xyz"], t["idx"]),
          ["xyz", "new_xyz", "idx"], lambda got, tag: same(got["idx"], want, tag), ("ball_query", n))


@pytest.mark.parametrize("m", [60, 600])
def test_three_nn_black_box(oracle, m):
    """m = 600: over the spatial index in scratch"""
    from epnet_amd import pointnet2_cuda as ext
    b, n = 2, 100
    unknown, known = cloud(b, n, seed=1), cloud(b, m, seed=2)
    want_d2, want_idx = oracle.three_nn(unknown, known)

    def reference(got, tag):
        same(got["idx"], want_idx, tag)
        same(got["dist2"], want_d2, tag)
    sweep({"unknown": (unknown, F32), "known": (known, F32)}, {"dist2": ((b, n, 3), F32), "idx": ((b, n, 3), I32)},
          lambda t: ext.three_nn_wrapper(b, n, m, t["unknown"], t["known"], t["dist2"], t["idx"]),
          ["unknown", "known", "dist2", "idx"], reference, ("three_nn", m))


# ---- the RPN training targets ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_aug", [False, True])
def test_rpn_targets(with_aug):
    """b = 2, n = 1028 (n % 4 == 0, one tile of 1024 points and four more), g = 3; the rule of test_rpn_targets_gpu.py: the
    augmentation within its bounds of the restatement, the labels of the kernel's own augmented values EQUAL on every point"""
    from epnet_amd import rpn_target_cuda
    from test_rpn_targets_gpu import draw_case
    b, n, g = 2, 1028, 3
    pts, gt, alpha, aug = draw_case(b, n, g, seed=77, with_aug=with_aug)
    on_face = rts.targets(pts, gt, alpha, aug)[4] <= rts.BAND
    assert on_face.mean() <= rts.SHARE or on_face.sum() <= 1
    pts[on_face] = np.array([300.0, 50.0, -200.0], np.float32)
    want_pts, want_gt = rts.targets(pts, gt, alpha, aug)[0:2] if with_aug else (pts, gt)

    def reference(got, tag):
        bad = []
        if with_aug:
            for i in range(b):
                bad += rts.augmentation_failures(i, got["pts_out"][i], got["gt_out"][i], want_pts[i], want_gt[i])
        else:
            same(got["pts_out"], pts, tag)
            same(got["gt_out"], gt, tag)
        made = [rts.labels(p, q, 0.2) for p, q in zip(got["pts_out"], got["gt_out"])]
        want_cls, want_reg, dist = (np.stack([o[k] for o in made]) for k in range(3))
        assert not (dist <= rts.BAND).any(), tag
        assert (want_cls == 1).any() and (want_cls == -1).any(), tag
        same(got["cls_label"], want_cls.astype(np.int32), tag)
        assert got["reg_label"].tobytes() == want_reg.tobytes(), (tag, "regression rows")
        assert not bad, (tag, bad)
    sweep({"pts": (pts, F32), "gt": (gt, F32), "alpha": (alpha, F32), "aug": (aug, F32) if with_aug else None},
          {"pts_out": ((b, n, 3), F32), "gt_out": ((b, g, 7), F32), "cls_label": ((b, n), I32), "reg_label": ((b, n, 7), F32)},
          lambda t: rpn_target_cuda.rpn_targets_gpu(t["pts"], t["gt"], t["alpha"], t["aug"], 0.2, t["pts_out"], t["gt_out"], t["cls_label"],
                                                    t["reg_label"]),
          ["pts", "pts_out", "cls_label", "reg_label"], reference, ("rpn_targets", with_aug))


# ---- the box loss ----------------------------------------------------------------------------------------------------------------------
def loss_case(stage, s, rows, seed):
    """the sweep's draw (test_loss_gpu.draw, settled off the kinks), with every row from 64 on made background: a wave with
    foreground rows stages, computes and writes its tile back, a wave without any only zero-fills"""
    import test_loss_gpu as tlg
    inp = tlg.draw(stage, s, rows, 0.5 if rows > 1 else 1.0, seed)
    if stage == "rcnn":
        inp["reg_mask"][64:] = 0
        inp["reg_mask"][0] = 1
    else:
        inp["cls_label"][64:] = np.minimum(inp["cls_label"][64:], 0)
        inp["cls_label"][0] = 1
    inp = tlg.settle(s, inp, seed)
    fg = (inp["reg_mask"] if stage == "rcnn" else inp["cls_label"]) > 0
    assert fg[:64].any() and not fg[64:].any()
    return inp


def loss_sweep(stage, s, rows, seed):
    import test_loss_gpu as tlg
    from epnet_amd import loss_cuda, loss_utils
    inp = loss_case(stage, s, rows, seed)
    c = lr.channels(s)
    assert inp["pred_reg"].shape == (rows, c)
    o64, o32 = lr.box_loss(s, dtype=np.float64, **inp), lr.box_loss(s, dtype=np.float32, **inp)
    anchor = loss_utils._anchor_on(torch.device(DEV), loss_utils.default_cfg())
    branch = inp["iou_branch"]

    def call(t):
        loss_cuda.box_loss_gpu(t["cls_logit"], t["pred_reg"], t["reg_label"], t["cls_label"], t["reg_mask"], t["iou_branch"], anchor,
                               s["loc_scope"], s["loc_bin_size"], s["num_head_bin"], s["ry_fine"], s["iou_type"], s["cls_type"], s["alpha"],
                               s["gamma"], s["fg_weight"], s["w_cls"], s["w_reg"], s["w_train"], s["ce_weight"], t["terms"], t["grad_cls"],
                               t["grad_reg"], t["grad_iou_branch"])

    def reference(got, tag):
        failures = []
        terms = got["terms"].astype(np.float64)
        for i, k in enumerate(lr.TERM_NAMES):
            bound = tlg.bound_rule(o64["terms"][k], o32["terms"][k])
            if not abs(terms[i] - float(o64["terms"][k])) <= bound:
                failures.append((k, terms[i], float(o64["terms"][k]), bound))
        for g in ("grad_cls", "grad_reg", "grad_iou_branch"):
            if g not in got:
                continue
            want = o64[g].reshape(got[g].shape)
            bound = tlg.bound_rule(want, o32[g].reshape(got[g].shape))
            diff = float(np.abs(got[g].astype(np.float64) - want).max())
            print("%s %s: max |diff| %.3e, bound %.3e" % (tag, g, diff, bound))
            if not diff <= bound:
                failures.append((g, diff, bound))
        assert not failures, (tag, failures)
        assert got["grad_reg"][0].any() and not got["grad_reg"][64:].any(), tag
    sweep({"cls_logit": (inp["cls_logit"], F32), "pred_reg": (inp["pred_reg"], F32), "reg_label": (inp["reg_label"], F32),
           "cls_label": (inp["cls_label"], I32), "reg_mask": None if inp["reg_mask"] is None else (inp["reg_mask"], I32),
           "iou_branch": None if branch is None else (branch, F32)},
          {"terms": ((24,), F32), "grad_cls": ((rows,), F32), "grad_reg": ((rows, c), F32),
           "grad_iou_branch": None if branch is None else ((rows,), F32)},
          call, ["pred_reg", "grad_reg"], reference, ("box_loss", stage, rows, c))


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("stage", ["rpn", "rcnn"])
def test_box_loss(stage, rows):
    """both stages at their own settings (76 and 46 channels). Against the float64 restatement under the sweep's bound rule
    (4 x the float32 restatement's own deviation, floor 1e-6 of the largest magnitude), and the bits of the aligned run"""
    loss_sweep(stage, lr.settings(stage, use_iou_branch=(stage == "rcnn")), rows, seed=rows * 31 + len(stage))


# c = 4 nb + 2 nh + 4 with nb even in 2 .. 32 and nh in 1 .. 32: even counts from 14 to 196
LOSS_CHANNELS = {14: (2, 1), 126: (28, 5), 128: (28, 6), 130: (28, 7), 196: (32, 32)}


@pytest.mark.parametrize("c", sorted(LOSS_CHANNELS))
def test_box_loss_staging_extremes(c):
    """the staging loop's (row, column) bookkeeping, dr = 256 / c, dc = 256 - dr * c, at the fewest and the most channels the
    argument rules allow and on either side of 128; rows 1, 63, 64 and 65"""
    nb, nh = LOSS_CHANNELS[c]
    for k, rows in enumerate((1, 63, 64, 65)):
        stage = ("rpn", "rcnn")[(k + c // 2) % 2]
        s = lr.settings(stage, loc_scope=nb * 0.25, loc_bin_size=0.5, num_head_bin=nh)
        assert lr.channels(s) == c
        loss_sweep(stage, s, rows, seed=c * 7 + rows)


# ---- the decode and the hand-over --------------------------------------------------------------------------------------------------------
def decode_sweep(name, rows, scale=1.0):
    from epnet_amd import handover_cuda
    cfg = hc.CONFIGS[name]
    anchor, reg = hc.case(name, rows, scale)
    ref, skip = hc.case_reference(name, rows, scale)
    kw = hc.decode_kwargs(cfg)

    def call(t):
        handover_cuda.decode_bbox_target_gpu(t["anchors"], t["pred_reg"], kw["loc_scope"], kw["loc_bin_size"], kw["num_head_bin"], hc.ANCHOR_SIZE,
                                             kw["get_xz_fine"], kw["get_y_by_bin"], kw["loc_y_scope"], kw["loc_y_bin_size"], kw["get_ry_fine"],
                                             kw["bbox_avg_by_bin"], kw["ry_with_bin"], False, t["boxes"])

    def reference(got, tag):
        boxes = torch.from_numpy(got["boxes"])
        if rows >= 1000:
            hc.check(boxes, ref, skip, str(tag))
        else:                           # too few rows for a share of rows left out: the tolerances alone, as test_decode_parity
            size, heading = hc.errors(boxes, ref, skip)
            print("%s: columns 0-5 at %.3f of the tolerance, heading error %.3e" % (tag, size, heading))
            assert boxes.shape == ref.shape and size == size and size <= 1.0 and heading <= hc.TOL, (tag, size, heading)
    sweep({"anchors": (anchor, F32), "pred_reg": (reg, F32)}, {"boxes": ((rows, 7), F32)}, call, ["pred_reg"], reference, ("decode", name, rows))
    return skip


@pytest.mark.parametrize("name", sorted(set(hc.CONFIGS) - set(hc.STAGING)))
def test_decode(name):
    left_out = total = 0
    for rows in (1, 63, 64, 65, 1000):
        left_out += int(decode_sweep(name, rows).sum())
        total += rows
    assert left_out <= 0.01 * total, (name, left_out, total)


@pytest.mark.parametrize("name", sorted(hc.STAGING))
def test_decode_staging_extremes(name):
    """10, 128, 129, 254 and 255 channels (handover_cases.STAGING), rows 1, 63, 64 and 65; no row is left out"""
    assert hc.channels(hc.CONFIGS[name]) == hc.STAGING[name] and not hc.CONFIGS[name]["ry_with_bin"]
    for rows in (1, 63, 64, 65):
        assert not bool(decode_sweep(name, rows).any())


def test_decode_refuses_256_channels():
    from epnet_amd import _lib, handover_cuda
    cfg = hc.TOO_WIDE
    assert hc.channels(cfg) == 256
    kw = hc.decode_kwargs(cfg)
    for skew in (0, 4):
        reg = oa.skewed(np.zeros((64, 256), np.float32), F32, skew)
        anchors, boxes = oa.skewed(np.zeros((64, 3), np.float32), F32, 0), oa.output((64, 7), F32, 0)
        with pytest.raises(_lib.EpnetError, match="decode_bbox_target.*supported range"):
            handover_cuda.decode_bbox_target_gpu(anchors, reg, kw["loc_scope"], kw["loc_bin_size"], kw["num_head_bin"], hc.ANCHOR_SIZE,
                                                 kw["get_xz_fine"], kw["get_y_by_bin"], kw["loc_y_scope"], kw["loc_y_bin_size"], kw["get_ry_fine"],
                                                 kw["bbox_avg_by_bin"], kw["ry_with_bin"], False, boxes)
        oa.check()
        assert oa.untouched(boxes)


def handover_call_args():
    from epnet_amd import proposal_layer, rpn_handover
    cfg = proposal_layer.default_cfg()
    cfg.TEST.RPN_DISTANCE_BASED_PROPOSE, cfg.RPN.NMS_TYPE = True, "normal"
    return rpn_handover.handover_args(cfg, "TEST")


def test_handover_end_to_end():
    """one hand-over at n = 2048 with rpn_reg off the boundary: order, proposals (the decode's tolerance against float64), and
    every output with the bits of the aligned run"""
    from epnet_amd import handover_cuda
    n = 2048
    scores, reg, xyz = hc.scene_inputs(n)
    args = handover_call_args()
    post = args["post_nms_top_n"]
    ref = hc.reference64(hc.CONFIGS["rpn_soft"], xyz.view(-1, 3), reg.view(-1, 76), y_to_bottom=True)

    def reference(got, tag):
        same(got["order"], hc.stable_order(scores).numpy(), tag)
        hc.check(torch.from_numpy(got["proposals"]).view(-1, 7), ref, torch.zeros(2 * n, dtype=torch.bool), str(tag))
        assert got["ret_count"].min() > 0 and got["ret_count"].max() <= post, tag
    sweep({"scores": (scores, F32), "rpn_reg": (reg, F32), "xyz": (xyz, F32)},
          {"ret_bbox3d": ((2, post, 7), F32), "ret_scores": ((2, post), F32), "ret_count": ((2,), I32), "seg_mask": ((2, n), F32),
           "pts_depth": ((2, n), F32), "proposals": ((2, n, 7), F32), "order": ((2, n), I64)},
          lambda t: handover_cuda.rpn_handover_gpu(t["scores"], t["rpn_reg"], t["xyz"], ret_bbox3d=t["ret_bbox3d"], ret_scores=t["ret_scores"],
                                                   ret_count=t["ret_count"], seg_mask=t["seg_mask"], pts_depth=t["pts_depth"],
                                                   proposals=t["proposals"], order=t["order"], **args),
          ["rpn_reg"], reference, "rpn_handover")


# ---- image normalisation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_scene", [False, True])
def test_image_normalise(per_scene):
    from epnet_amd import scan_cuda
    b, hw_in, hw_out = 2, (5, 21), (8, 16)             # w_out % 4 == 0; the image is wider and lower than the output
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (b,) + hw_in + (3,)).astype(np.uint8)
    shapes = np.array([[5, 21], [4, 9]], np.int32) if per_scene else None
    want = srs.image_normalise(img, shapes, hw_out)
    sweep({"img": (img, U8), "img_shape": None if shapes is None else (shapes, I32)}, {"out": ((b, 3) + hw_out, F32)},
          lambda t: scan_cuda.image_normalise_gpu(t["img"], t["img_shape"], srs.MEAN, srs.STD, t["out"]), ["out"],
          lambda got, tag: same(got["out"], want, tag), ("image_normalise", per_scene))


# ---- refusals stay refusals --------------------------------------------------------------------------------------------------------------
class _SkewedScratch:
    """stands in for `torch` inside a stand-in module: its uint8 scratch comes 4 bytes off a boundary, sentinel-filled"""

    def __init__(self):
        self.made = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *shape, dtype=torch.float32, device=None, **kw):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        if dtype == torch.uint8 and not kw:
            self.made.append(oa.output(shape, U8, 4, device))
            return self.made[-1]
        return torch.empty(shape, dtype=dtype, device=device, **kw)


def refused(outputs, scratch=()):
    oa.check()
    assert all(oa.untouched(t) for t in outputs), "an output of a refused call was written"
    assert all(oa.untouched(t) for t in scratch), "the scratch of a refused call was written"


def test_scan_prepare_refuses_a_skewed_scan():
    from epnet_amd import _lib, scan_cuda
    b, p, n = 1, 64, 16
    z = lambda shape, dtype=F32: oa.skewed(np.zeros(shape, np.float32), dtype, 0)  # noqa: E731
    outs = [oa.output(s, d, 0) for s, d in (((b, n, 3), F32), ((b, n), F32), ((b, n, 2), F32), ((b, n, 4), F32), ((b, n), I32), ((b, 6), I32))]
    with pytest.raises(_lib.EpnetError, match="scan_prepare"):
        scan_cuda.scan_prepare_gpu(oa.skewed(np.zeros((b, p, 4), np.float32), F32, 4), z((b,), I32), z((b, 3, 4)), z((b, 3, 3)), z((b, 3, 4)),
                                   z((b, 2), I32), z((b, p), I32), None, True, srs.SCOPE.reshape(-1), srs.NEAR, *outs)
    refused(outs)


def test_scene_index_refuses_a_skewed_buffer():
    from epnet_amd import _lib, pointnet2_cuda as ext
    b, n_src, n = 1, 2048, 1024
    nbytes = ext.scene_index_bytes(b, n)
    assert nbytes > 0
    xyz = oa.skewed(cloud(b, n_src, seed=1), F32, 0)
    index = oa.output((nbytes,), U8, 4)
    with pytest.raises(_lib.EpnetError, match="scene_index_build"):
        ext.scene_index_build_wrapper(b, n, xyz[:, :n].contiguous(), index)
    refused([], [index])
    idx = oa.skewed(np.arange(n, dtype=np.int32)[None] * 2, I32, 0)
    index, new_xyz = oa.output((nbytes,), U8, 4), oa.output((b, n, 3), F32, 0)
    with pytest.raises(_lib.EpnetError, match="scene_index_build_gathered"):
        ext.scene_index_build_gathered_wrapper(b, n_src, n, xyz, idx, new_xyz, index)
    refused([new_xyz], [index])


def test_three_nn_refuses_skewed_scratch(monkeypatch):
    from epnet_amd import _lib, pointnet2_cuda as ext
    b, n, m = 1, 8, 512                                 # 512 known points: the least that take the indexed kernel and its scratch
    assert _lib.lib().epnet_three_nn_workspace_bytes(b, n, m) > 0
    proxy = _SkewedScratch()
    monkeypatch.setattr(ext, "torch", proxy)
    dist2, idx = oa.output((b, n, 3), F32, 0), oa.output((b, n, 3), I32, 0)
    with pytest.raises(_lib.EpnetError, match="three_nn"):
        ext.three_nn_wrapper(b, n, m, oa.skewed(cloud(b, n, seed=1), F32, 0), oa.skewed(cloud(b, m, seed=2), F32, 0), dist2, idx)
    assert len(proxy.made) == 1
    refused([dist2, idx], proxy.made)


def test_box_loss_refuses_skewed_scratch():
    from epnet_amd import _lib, loss_cuda, loss_utils
    s = lr.settings("rpn")
    rows, c = 64, lr.channels(s)
    nbytes = _lib.lib().epnet_box_loss_workspace_bytes(rows, c)
    ws = oa.output((nbytes,), U8, 4)
    z = lambda shape, dtype=F32: oa.skewed(np.zeros(shape, np.float32), dtype, 0)  # noqa: E731
    outs = [oa.output((24,), F32, 0), oa.output((rows,), F32, 0), oa.output((rows, c), F32, 0)]
    anchor = loss_utils._anchor_on(torch.device(DEV), loss_utils.default_cfg())
    with pytest.raises(_lib.EpnetError, match="box_loss"):
        loss_cuda.box_loss_gpu(z((rows,)), z((rows, c)), z((rows, 7)), z((rows,), I32), None, None, anchor, s["loc_scope"], s["loc_bin_size"],
                               s["num_head_bin"], s["ry_fine"], s["iou_type"], s["cls_type"], s["alpha"], s["gamma"], s["fg_weight"], s["w_cls"],
                               s["w_reg"], s["w_train"], s["ce_weight"], *outs, None, ws=ws)
    refused(outs, [ws])


def test_handover_refuses_skewed_scratch(monkeypatch):
    from epnet_amd import _lib, handover_cuda
    n = 64
    args = handover_call_args()
    post = args["post_nms_top_n"]
    proxy = _SkewedScratch()
    monkeypatch.setattr(handover_cuda, "torch", proxy)
    z = lambda shape: oa.skewed(np.zeros(shape, np.float32), F32, 0)  # noqa: E731
    outs = [oa.output((1, post, 7), F32, 0), oa.output((1, post), F32, 0), oa.output((1,), I32, 0), oa.output((1, n), F32, 0),
            oa.output((1, n), F32, 0), oa.output((1, n, 7), F32, 0), oa.output((1, n), I64, 0)]
    with pytest.raises(_lib.EpnetError, match="rpn_handover"):
        handover_cuda.rpn_handover_gpu(z((1, n)), z((1, n, 76)), z((1, n, 3)), ret_bbox3d=outs[0], ret_scores=outs[1], ret_count=outs[2],
                                       seg_mask=outs[3], pts_depth=outs[4], proposals=outs[5], order=outs[6], **args)
    assert len(proxy.made) == 1
    refused(outs, proxy.made)


def test_deterministic_gradient_refuses_skewed_scratch():
    """the deterministic gradients want their scratch on a 256-byte boundary; no wrapper lets the caller pass it, so through
    the C ABI (as test_scratch_free_entry_points_through_the_c_abi in test_gpu_parity.py)"""
    from epnet_amd import _lib
    l = _lib.lib()
    b, c, n, m = 2, 4, 256, 512
    nbytes = l.epnet_gather_points_grad_det_workspace_bytes(b, n, m)
    assert nbytes > 0
    rng = np.random.default_rng(4)
    go = oa.skewed(rng.standard_normal((b, c, m)).astype(np.float32), F32, 0)
    idx = oa.skewed(rng.integers(0, n, (b, m)).astype(np.int32), I32, 0)
    grad, ws = oa.output((b, c, n), F32, 0), oa.output((nbytes + 256,), U8, 4)
    s = torch.cuda.current_stream().cuda_stream
    with pytest.raises(_lib.EpnetError, match="gather_points_grad"):
        _lib.check(l.epnet_gather_points_grad_det(b, c, n, m, go.data_ptr(), idx.data_ptr(), grad.data_ptr(), ws.data_ptr(), ws.numel(), s),
                   "gather_points_grad (deterministic)")
    refused([grad], [ws])

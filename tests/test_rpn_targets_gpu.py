"""The RPN training targets on the GPU (epnet_amd/rpn_target_layer.py over csrc/targets.hip).

Bounds. Against the reference (tests/golden/rpn_targets.npz) the fixture's own: augmented x, z within 1 fp32 ulp of
max(|x|, |z|), y and box columns 0..5 exact, ry within 1e-5; classes and regression rows EQUAL for every point farther than
1e-4 m from all faces, at most 0.5 % of a scene's points nearer. Against the float64 restatement (tests/rpn_targets_restate.py,
held to the reference in test_rpn_targets.py): the same for the augmentation; the labels are taken from the kernel's own
augmented values (the labels are defined on those) and are EQUAL on every point -- the seeded draws move the few points
within 1e-4 m of a face away, the decisive points stand 1e-3 m from their faces by construction. Between runs: bit-equal."""
import numpy as np
import pytest
import torch

import rpn_targets_restate as rs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F = np.float32


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def host(t):
    return t.detach().cpu().numpy()


def run(pts, gt, alpha=None, aug=None, extra=0.2):
    """through the public functions -> numpy (pts_out, gt_out, cls, reg); without aug the inputs stand for the augmented values"""
    from epnet_amd import rpn_target_layer as rtl
    if aug is None:
        cls, reg = rtl.rpn_training_labels(dev(pts), dev(gt), extra)
        return np.asarray(pts, F), np.asarray(gt, F), host(cls), host(reg)
    return tuple(host(t) for t in rtl.augment_and_label(dev(pts), dev(gt), dev(alpha), dev(aug), extra))


def labels_of(pts, gt, extra=0.2):
    out = [rs.labels(p, g, extra) for p, g in zip(pts, gt)]
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


# ---- the fixture ------------------------------------------------------------------------------------------------------------------
def test_kernel_against_the_reference(hiplib):
    scenes, extra = rs.fixture_scenes()
    bad = []
    for i, s in enumerate(scenes):
        pts, gt, cls, reg = run(s["pts"][None], s["gt"][None], s["alpha"][None], s["aug"][None], extra)
        bad += rs.augmentation_failures(i, pts[0], gt[0], s["ref_pts"], s["ref_gt"])
        # the labels of the reference's own augmented values against the reference's labels
        _, _, cls_r, reg_r = run(s["ref_pts"][None], s["ref_gt"][None], extra=extra)
        dist = rs.labels(s["ref_pts"], s["ref_gt"], extra)[2]
        print("scene %d: %.3f %% of %d points within %g m of a face" % (i, 100 * float((dist <= rs.BAND).mean()), len(dist), rs.BAND))
        bad += rs.label_failures((i, "labels of the reference's values"), cls_r[0], reg_r[0], s["ref_cls"], s["ref_reg"], dist)
        # the fused call's labels are those of its own augmented values: classes against the reference's, all against the restatement
        bad += rs.label_failures((i, "fused classes"), cls[0], s["ref_reg"], s["ref_cls"], s["ref_reg"], dist)
        want = rs.labels(pts[0], gt[0], extra)
        bad += rs.label_failures((i, "fused against the restatement"), cls[0], reg[0], want[0], want[1], want[2])
    assert not bad, bad


def test_fixture_scenes_as_one_batch(hiplib):
    """the five 1024-point scenes in one launch: every scene takes its own row of the table"""
    scenes, extra = rs.fixture_scenes()
    pick = [s for s in scenes if s["pts"].shape[0] == 1024]
    assert len(pick) >= 5
    stack = lambda k: np.stack([s[k] for s in pick])  # noqa: E731
    pts, gt, cls, reg = run(stack("pts"), stack("gt"), stack("alpha"), stack("aug"), extra)
    for i, s in enumerate(pick):
        one = run(s["pts"][None], s["gt"][None], s["alpha"][None], s["aug"][None], extra)
        for a, b in zip((pts, gt, cls, reg), one):
            assert a[i].tobytes() == b[0].tobytes()


# ---- decisive points: no band, no exclusions ----------------------------------------------------------------------------------------
def decisive_scene(ry, extra=0.2, step=1e-3):
    box = np.array([5.0, 1.5, 20.0, 1.5, 1.75, 4.0, ry], F)
    x, y, z, h, w, l, r = (float(v) for v in box)
    half = np.array([l / 2, h / 2, w / 2])
    local = [np.zeros(3)]
    for grow in (0.0, float(F(extra))):
        for axis in range(3):
            for side in (-1.0, 1.0):
                for d in (-step, step):
                    q = np.array([0.3, 0.2, -0.25])                       # off the other axes' centre, well inside
                    q[axis] = side * (half[axis] + grow + d)
                    local.append(q)
    q = np.array(local)
    c, s = np.cos(r), np.sin(r)
    pts = np.stack([x + q[:, 0] * c + q[:, 2] * s, y - h / 2 + q[:, 1], z - q[:, 0] * s + q[:, 2] * c], axis=1)
    return pts.astype(F), box[None]


def test_decisive_points(hiplib):
    rys = (0.0, np.pi / 2, -np.pi / 2, 0.7, 3.1)
    made = [decisive_scene(ry) for ry in rys]
    pts, gt = np.stack([m[0] for m in made]), np.stack([m[1] for m in made])
    assert pts.shape == (5, 25, 3)
    _, _, cls, reg = run(pts, gt)
    want_cls, want_reg, dist = labels_of(pts, gt)
    assert float(dist.min()) > 0.9e-3                                       # every point stands 1e-3 from its nearest face
    # inside / outside alternate face by face: 1 (centre), then per face of the box (1, -1), per face of the enlarged box (-1, 0)
    assert want_cls[0].tolist() == [1] + [1, -1] * 6 + [-1, 0] * 6
    assert np.array_equal(cls, want_cls) and cls.dtype == np.int32
    assert reg.tobytes() == want_reg.tobytes()
    assert np.array_equal(reg[:, :, 3:7][cls == 1], np.broadcast_to(gt[:, :, 3:7], (5, 25, 4))[cls == 1])
    assert not reg[cls != 1].any()


# ---- the order rule -----------------------------------------------------------------------------------------------------------------
def test_order_rule(hiplib):
    a = np.array([0, 1, 10, 1.5, 1.6, 4.0, 0.0], F)            # z in [9.2, 10.8]
    b = np.array([0, 1, 11.7, 1.5, 1.6, 4.0, 0.25], F)         # about z in [10.9, 12.5] at x = 0, its margin from 10.7
    c = np.array([0.5, 1.1, 10.4, 1.6, 1.7, 4.2, -0.4], F)     # overlaps a
    p = np.array([[0.0, 0.5, 10.0], [0.0, 0.5, 10.75], [0.2, 0.4, 10.2], [30.0, 0.5, 10.0]], F)
    ab, ba, ac, ca = (np.stack(v) for v in ((a, b), (b, a), (a, c), (c, a)))
    _, _, cls, reg = run(np.stack([p] * 4), np.stack([ab, ba, ac, ca]))
    want = labels_of(np.stack([p] * 4), np.stack([ab, ba, ac, ca]))
    assert np.array_equal(cls, want[0]) and reg.tobytes() == want[1].tobytes()
    centre_a = np.array([a[0], a[1] - a[3] / F(2), a[2]], F)
    # in box a and in box b's margin only: class -1 with a's row in order (a, b), class 1 in order (b, a)
    assert cls[0, 1] == -1 and np.array_equal(reg[0, 1], np.concatenate([centre_a - p[1], a[3:7]]))
    assert cls[1, 1] == 1 and np.array_equal(reg[1, 1], reg[0, 1])
    # in both a and c: the later box's row
    assert cls[2, 2] == 1 and np.array_equal(reg[2, 2, 3:7], c[3:7]) and cls[3, 2] == 1 and np.array_equal(reg[3, 2, 3:7], a[3:7])
    assert cls[:, 3].tolist() == [0, 0, 0, 0] and not reg[:, 3].any()


# ---- seeded shapes ------------------------------------------------------------------------------------------------------------------
def draw_case(b, n, g, seed, with_aug):
    """scenes with boxes, points in and around them, padding rows in the middle and at the end of the box list"""
    rng = np.random.default_rng(seed)
    gt = np.zeros((b, g, 7))
    if g:
        gt[..., 0], gt[..., 1], gt[..., 2] = rng.uniform(-20, 20, (b, g)), rng.uniform(1, 2, (b, g)), rng.uniform(8, 60, (b, g))
        gt[..., 3:6] = np.array([1.53, 1.63, 3.88]) * (1 + 0.08 * rng.normal(size=(b, g, 3)))
        gt[..., 6] = rng.uniform(-np.pi, np.pi, (b, g))
        for k in range(1, g, 2):                                            # overlapping pairs: the odd rows sit on their neighbour
            gt[:, k, 0:3] = gt[:, k - 1, 0:3] + rng.uniform(-1.2, 1.2, (b, 3)) * [1, 0.1, 1]
        real = np.ones(g, bool)
        if g >= 2:
            real[g - 1] = False                                             # padding at the end ...
        if g >= 7:
            real[[2, g // 2]] = False                                       # ... and in the middle
        gt[:, ~real] = 0
    gt = gt.astype(F)
    pts = np.stack([rng.uniform(-40, 40, (b, n)), rng.uniform(-1, 3, (b, n)), rng.uniform(0, 70, (b, n))], axis=2)
    if g:
        which = rng.integers(0, g, (b, n))
        bx = np.take_along_axis(gt.astype(np.float64), which[:, :, None], axis=1)
        half = np.stack([bx[..., 5] / 2, bx[..., 3] / 2, bx[..., 4] / 2], axis=2) + 0.5
        q = rng.uniform(-1, 1, (b, n, 3)) * half
        c, s = np.cos(bx[..., 6]), np.sin(bx[..., 6])
        local = np.stack([bx[..., 0] + q[..., 0] * c + q[..., 2] * s, bx[..., 1] - bx[..., 3] / 2 + q[..., 1],
                          bx[..., 2] - q[..., 0] * s + q[..., 2] * c], axis=2)
        near = (rng.uniform(size=(b, n)) < 0.7) & (bx[..., 3] > 0)
        pts[near] = local[near]
    alpha = (rng.uniform(-np.pi, np.pi, (b, g)) * (gt[..., 3] > 0)).astype(F)
    aug = None
    if with_aug:
        on = rng.uniform(size=(b, 3)) < 0.6
        on[0] = True
        aug = np.stack([on[:, 0], np.where(on[:, 0], rng.uniform(-np.pi / 18, np.pi / 18, b), 0), np.where(on[:, 1], rng.uniform(0.95, 1.05, b), 1),
                        on[:, 2]], axis=1).astype(F)
    return pts.astype(F), gt, alpha, aug


CASES = [(1, 1, 0, False), (2, 3, 1, True), (9, 4, 2, False), (1, 5, 7, True), (2, 255, 33, True), (9, 256, 70, False), (1, 257, 2, True),
         (2, 1023, 7, False), (1, 1025, 33, True), (2, 4099, 70, True), (1, 16384, 33, False), (2, 16384, 7, True), (257, 5, 2, True),
         (257, 256, 1, False), (9, 1025, 0, True), (9, 1024, 7, True)]


def test_cases_cover_the_shapes():
    assert {c[1] for c in CASES} >= {1, 3, 4, 5, 255, 256, 257, 1023, 1025, 4099, 16384}
    assert {c[2] for c in CASES} >= {0, 1, 2, 7, 33, 70} and {c[0] for c in CASES} >= {1, 2, 9, 257}


@pytest.mark.parametrize("b,n,g,with_aug", CASES)
def test_seeded_shapes_against_the_restatement(hiplib, b, n, g, with_aug):
    pts, gt, alpha, aug = draw_case(b, n, g, seed=b * 1000003 + n * 101 + g, with_aug=with_aug)
    # settle: a point within 1e-4 m of a face (after the augmentation) moves far away from every box
    first = rs.targets(pts, gt, alpha, aug)
    on_face = first[4] <= rs.BAND
    assert on_face.mean() <= rs.SHARE or on_face.sum() <= 1
    pts[on_face] = np.array([300.0, 50.0, -200.0], F)
    nan_at = None
    if n >= 4:
        nan_at = (b - 1, n // 2, 1)
        pts[nan_at] = np.nan                                                # one NaN coordinate: class 0, zero row, no fault
    pts_out, gt_out, cls, reg = run(pts, gt, alpha, aug)
    bad = []
    if with_aug:
        want_pts, want_gt = rs.targets(pts, gt, alpha, aug)[0:2]
        ok = ~np.isnan(want_pts).any(axis=2)
        assert np.array_equal(np.isnan(pts_out), np.isnan(want_pts))
        for i in range(b):
            bad += rs.augmentation_failures(i, pts_out[i][ok[i]], gt_out[i], want_pts[i][ok[i]], want_gt[i])
        if g:
            assert not gt_out[:, gt[0, :, 3] == 0].any()                    # padding rows stay zero
    want_cls, want_reg, dist = labels_of(pts_out, gt_out)
    assert not (dist <= rs.BAND).any()
    if not np.array_equal(cls, want_cls):
        bad.append(("classes", np.argwhere(cls != want_cls)[:5].tolist()))
    if reg.tobytes() != want_reg.tobytes():
        bad.append(("regression rows", np.argwhere(reg != want_reg)[:5].tolist()))
    if nan_at is not None:
        assert cls[nan_at[0], nan_at[1]] == 0 and not reg[nan_at[0], nan_at[1]].any()
    assert not bad, bad


def test_int64_labels_on_request(hiplib):
    from epnet_amd import rpn_target_layer as rtl
    pts, gt, _, _ = draw_case(2, 300, 3, seed=4, with_aug=False)
    c32, r32 = rtl.rpn_training_labels(dev(pts), dev(gt))
    c64, r64 = rtl.rpn_training_labels(dev(pts), dev(gt), dtype=torch.int64)
    assert c32.dtype == torch.int32 and c64.dtype == torch.int64 and torch.equal(c32.long(), c64) and torch.equal(r32, r64)
    assert (c32 == 1).any() and (c32 == -1).any()


# ---- limits -------------------------------------------------------------------------------------------------------------------------
def _raw(pts, gt, alpha, aug, outs, extra=0.2):
    from epnet_amd import rpn_target_cuda
    return rpn_target_cuda.rpn_targets_gpu(pts, gt, alpha, aug, extra, *outs)


def test_limits(hiplib):
    from epnet_amd import _lib
    fill = lambda shape, dtype=torch.float32: torch.full(shape, 7, dtype=dtype, device=DEV)  # noqa: E731
    b = 65536
    pts, gt, alpha, aug = (torch.zeros(s, device=DEV) for s in ((b, 1, 3), (b, 1, 7), (b, 1), (b, 4)))
    outs = [fill((b, 1, 3)), fill((b, 1, 7)), fill((b, 1), torch.int32), fill((b, 1, 7))]
    with pytest.raises(_lib.EpnetError, match="supported range"):
        _raw(pts, gt, alpha, aug, outs)
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)                          # nothing was written
    _raw(pts[:65535], gt[:65535], alpha[:65535], aug[:65535], outs)         # the largest batch runs
    torch.cuda.synchronize()
    assert bool((outs[2][:65535] == 0).all()) and bool((outs[2][65535:] == 7).all()) and bool((outs[0][65535:] == 7).all())
    # b or n of 0: a no-op
    for shape in ((0, 8), (2, 0)):
        outs = [fill((2, 8, 3)), fill((2, 2, 7)), fill((2, 8), torch.int32), fill((2, 8, 7))]
        bb, nn = shape
        _raw(torch.zeros((bb, nn, 3), device=DEV), torch.ones((bb, 2, 7), device=DEV), torch.zeros((bb, 2), device=DEV),
             torch.zeros((bb, 4), device=DEV), outs)
        torch.cuda.synchronize()
        assert all(bool((o == 7).all()) for o in outs)
    from epnet_amd import rpn_target_layer as rtl
    cls, reg = rtl.rpn_training_labels(torch.zeros((0, 8, 3), device=DEV), torch.zeros((0, 2, 7), device=DEV))
    assert cls.shape == (0, 8) and reg.shape == (0, 8, 7)
    with pytest.raises(RuntimeError, match="alias"):
        p = torch.zeros((1, 8, 3), device=DEV)
        _raw(p, torch.zeros((1, 1, 7), device=DEV), torch.zeros((1, 1), device=DEV), torch.zeros((1, 4), device=DEV),
             [p, fill((1, 1, 7)), fill((1, 8), torch.int32), fill((1, 8, 7))])


# ---- reproducibility ----------------------------------------------------------------------------------------------------------------
def test_runs_are_bit_equal(hiplib):
    """twice on one stream and once on a side stream"""
    from epnet_amd import rpn_target_layer as rtl
    pts, gt, alpha, aug = (dev(a) for a in draw_case(2, 16384, 20, seed=11, with_aug=True))
    a = rtl.augment_and_label(pts, gt, alpha, aug)
    b = rtl.augment_and_label(pts, gt, alpha, aug)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = rtl.augment_and_label(pts, gt, alpha, aug)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for x, y, z in zip(a, b, c):
        assert host(x).tobytes() == host(y).tobytes() == host(z).tobytes()
    assert (a[2] == 1).any() and (a[2] == -1).any() and a[3].abs().sum() > 0


# ---- one graph with the loss ----------------------------------------------------------------------------------------------------------
def test_targets_and_loss_in_one_graph(hiplib):
    """augment_and_label + rpn_loss forward and backward captured in ONE torch.cuda.graph (the capture fails on any
    synchronisation with the host), replayed after the static inputs were rewritten, against eager runs: bit-equal"""
    from epnet_amd import loss_utils, rpn_target_layer as rtl
    b, n, c = 2, 4096, 76
    first, second = draw_case(b, n, 9, seed=21, with_aug=True), draw_case(b, n, 9, seed=22, with_aug=True)
    g = torch.Generator(device=DEV).manual_seed(8)
    static = {"pts": dev(first[0]), "gt": dev(first[1]), "alpha": dev(first[2]), "aug": dev(first[3]),
              "cls": torch.randn((b, n, 1), generator=g, device=DEV).requires_grad_(True),
              "reg": torch.randn((b, n, c), generator=g, device=DEV).requires_grad_(True)}
    cfg = loss_utils.default_cfg()

    def step():
        pts, gt, cls_label, reg_label = rtl.augment_and_label(static["pts"], static["gt"], static["alpha"], static["aug"])
        out = loss_utils.rpn_loss(static["cls"], static["reg"], cls_label, reg_label, cfg)
        grads = torch.autograd.grad(out.loss, [static["cls"], static["reg"]])
        return [pts, gt, cls_label, reg_label, out.loss, out.terms] + list(grads)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    eager_first = step()
    assert all(torch.equal(x, y) for x, y in zip(eager_first, captured))
    assert float(captured[5][18]) > 0                                         # some foreground points reached the loss
    with torch.no_grad():
        for key, value in zip(("pts", "gt", "alpha", "aug"), second):
            static[key].copy_(dev(value))
    graph.replay()
    torch.cuda.synchronize()
    eager_second = step()
    assert all(torch.equal(x, y) for x, y in zip(eager_second, captured))
    assert not torch.equal(eager_second[5], eager_first[5]) and not torch.equal(eager_second[2], eager_first[2])

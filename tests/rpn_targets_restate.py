"""numpy restatement of the RPN training targets (include/epnet_ops.h, epnet_rpn_targets; reference:
lib/datasets/kitti_rcnn_dataset.py, data_augmentation :698-755 and generate_rpn_training_labels :547-576).

``augment`` follows the reference's arithmetic: the rotation in float64 from the float32 inputs, rounded once; the heading,
the scaling and the flip in float32. ``labels`` decides membership with FLOAT64 geometry (the yardstick of the kernel's
float32 predicate) and applies the order rule of the reference's loop: the class is decided by the last box whose enlarged
form holds the point, the regression row by the last box that holds it. It also returns each point's distance to the
nearest face of any box or enlarged box: only a point within rounding of a face may legitimately differ between a float32
and a float64 evaluation (or the reference's Delaunay test).
"""
import numpy as np

F = np.float32
PI = F(np.pi)


def augment(pts, gt, alpha, row):
    """pts (N,3), gt (G,7), alpha (G) float32, row = [rotate 0/1, angle, scale, flip 0/1] -> augmented (pts, gt), float32"""
    pts, gt, alpha = np.array(pts, F), np.array(gt, F).reshape(-1, 7), np.asarray(alpha, F).reshape(-1)
    rot, angle, scale, flip = bool(row[0]), float(F(row[1])), F(row[2]), bool(row[3])
    if rot:
        c, s = np.cos(angle), np.sin(angle)
        for a in (pts, gt):
            x, z = a[:, 0].astype(np.float64), a[:, 2].astype(np.float64)
            a[:, 0], a[:, 2] = (x * c - z * s).astype(F), (x * s + z * c).astype(F)
        beta = np.arctan2(gt[:, 2].astype(np.float64), gt[:, 0].astype(np.float64)).astype(F)
        gt[:, 6] = ((np.sign(beta) * PI) / F(2) + alpha) - beta
    pts = pts * scale
    gt[:, 0:6] = gt[:, 0:6] * scale
    if flip:
        pts[:, 0] = -pts[:, 0]
        gt[:, 0] = -gt[:, 0]
        gt[:, 6] = np.sign(gt[:, 6]) * PI - gt[:, 6]
    return pts, gt


def _surface_distance(q, half):
    """distance of local points q (N,3) to the surface of the box |q_i| <= half_i"""
    d = np.abs(q) - half
    outside = np.sqrt((np.maximum(d, 0.0) ** 2).sum(axis=1))
    inside = -d.max(axis=1)
    return np.where((d <= 0).all(axis=1), inside, outside)


def labels(pts, gt, extra_width=0.2):
    """pts (N,3), gt (G,7) float32 -> cls (N) int32, reg (N,7) float32, face_distance (N) float64 (inf without a box)"""
    pts, gt = np.asarray(pts, F), np.asarray(gt, F).reshape(-1, 7)
    n = pts.shape[0]
    cls, reg, dist = np.zeros(n, np.int32), np.zeros((n, 7), F), np.full(n, np.inf)
    e = float(F(extra_width))
    with np.errstate(invalid="ignore"):
        for k in range(gt.shape[0]):
            x, y, z, h, w, l, ry = (float(v) for v in gt[k])
            if not (h > 0 and w > 0 and l > 0):
                continue
            cy32 = gt[k, 1] - gt[k, 3] / F(2)
            d = pts.astype(np.float64) - np.array([x, y - h / 2, z])
            c, s = np.cos(ry), np.sin(ry)
            q = np.stack([d[:, 0] * c - d[:, 2] * s, d[:, 1], d[:, 0] * s + d[:, 2] * c], axis=1)
            half = np.array([l / 2, h / 2, w / 2])
            in_b = (np.abs(q) <= half).all(axis=1)
            in_e = (np.abs(q) <= half + e).all(axis=1)
            dist = np.fmin(dist, np.fmin(_surface_distance(q, half), _surface_distance(q, half + e)))
            cls[in_e] = np.where(in_b[in_e], 1, -1)
            centre = np.array([gt[k, 0], cy32, gt[k, 2]], F)
            reg[in_b, 0:3] = centre - pts[in_b]
            reg[in_b, 3:7] = gt[k, 3:7]
    return cls, reg, dist


def labels32(pts, gt, extra_width=0.2):
    """the kernel's documented definition (csrc/targets.hip), on box_faces.membership32: float32 in source order about the centre
    (x, y - h / 2 in float32, z), no 10 m gate, the enlarged box (h, w, l + 2e) about the same centre, a box with an extent that is
    not positive labels nothing, the last box decides, regression rows are centre - point as written
    -> cls (N) int32, reg (N,7) float32"""
    import box_faces as bf
    pts, gt = np.asarray(pts, F).reshape(-1, 3), np.asarray(gt, F).reshape(-1, 7)
    cls, reg = np.zeros(len(pts), np.int32), np.zeros((len(pts), 7), F)
    for b in gt:
        if not (b[3] > 0 and b[4] > 0 and b[5] > 0):
            continue
        cy = b[1] - b[3] / F(2)
        in_b = bf.membership32(pts, b, 0.0, gate=False, cy=cy)[0]
        in_e = bf.membership32(pts, b, extra_width, gate=False, cy=cy)[0]
        cls[in_e] = np.where(in_b[in_e], 1, -1)
        with np.errstate(invalid="ignore"):
            reg[in_b, 0:3] = np.array([b[0], cy, b[2]], F) - pts[in_b]
        reg[in_b, 3:7] = b[3:7]
    return cls, reg


def targets(pts, gt, alpha=None, aug=None, extra_width=0.2):
    """a batch: pts (B,N,3), gt (B,G,7), alpha (B,G), aug (B,4) or None -> (pts_out, gt_out, cls, reg, face_distance)"""
    pts, gt = np.asarray(pts, F), np.asarray(gt, F)
    out = []
    for i in range(pts.shape[0]):
        p, g = (pts[i].copy(), gt[i].copy()) if aug is None else augment(pts[i], gt[i], alpha[i], aug[i])
        out.append((p, g) + labels(p, g, extra_width))
    return tuple(np.stack([o[k] for o in out]) if out else np.zeros((0,)) for k in range(5))


# ---- the fixture (tests/golden/rpn_targets.npz, made by tests/golden/make_golden_rpn_targets.py) and its bounds ----------------
BAND = 1e-4          # metres around every face: 13 fp32 ulps at 80 m, the range of the scene
SHARE = 0.005        # of a scene's points may lie in the band (a condition on the inputs, not a tolerance)
RY_BOUND = 1e-5      # the parity definition's bound for trigonometry


def fixture_scenes():
    import os
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rpn_targets.npz"))
    scenes = []
    for i in range(int(fx["scenes"])):
        pre = "s%d__" % i
        scenes.append({k: fx[pre + k] for k in ("pts", "gt", "alpha", "aug", "ref_pts", "ref_gt", "ref_cls", "ref_reg")})
        scenes[-1]["ref_cls"] = scenes[-1]["ref_cls"].astype(np.int32)
    return scenes, float(fx["extra_width"])


def augmentation_failures(tag, pts, gt, ref_pts, ref_gt):
    """the fixture's bounds on augmented values: x and z within 1 fp32 ulp of max(|x|, |z|) (the reference's float64 product may
    be contracted differently by another BLAS), y exact; box columns 0..5 exact, ry within 1e-5"""
    bad = []
    ulp = np.spacing(np.maximum(np.abs(ref_pts[:, 0]), np.abs(ref_pts[:, 2])).astype(F)).astype(np.float64)
    for col in (0, 2):
        over = np.abs(pts[:, col].astype(np.float64) - ref_pts[:, col]) > ulp
        if over.any():
            bad.append((tag, "pts column %d" % col, int(over.sum())))
    if not np.array_equal(pts[:, 1], ref_pts[:, 1]):
        bad.append((tag, "pts y"))
    if not np.array_equal(gt[:, 0:6], ref_gt[:, 0:6]):
        bad.append((tag, "box columns 0..5", float(np.abs(gt[:, 0:6] - ref_gt[:, 0:6]).max())))
    if not (np.abs(gt[:, 6].astype(np.float64) - ref_gt[:, 6]) <= RY_BOUND).all():
        bad.append((tag, "ry", float(np.abs(gt[:, 6].astype(np.float64) - ref_gt[:, 6]).max())))
    return bad


def label_failures(tag, cls, reg, want_cls, want_reg, dist):
    """classes and regression rows equal for every point farther than BAND from all faces; at most SHARE of the points nearer"""
    keep = dist > BAND
    bad = []
    if (~keep).mean() > SHARE:
        bad.append((tag, "share of points on a face", float((~keep).mean())))
    if not np.array_equal(cls[keep], want_cls[keep]):
        bad.append((tag, "classes", int((cls[keep] != want_cls[keep]).sum())))
    if not np.array_equal(reg[keep], want_reg[keep]):
        bad.append((tag, "regression rows", int((reg[keep] != want_reg[keep]).any(axis=1).sum())))
    return bad

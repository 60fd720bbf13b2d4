"""TEST INFRASTRUCTURE (numpy only): the point-in-box predicate of the library in float32, and clouds whose points stand on the
faces of rotated boxes -- where a fused multiply-add, a `<` for a `<=`, a fast sincos or another order of the half extents
changes the decision.

``membership32`` is the ONE numpy statement of the predicate that roipool3d.hip (plain, canonical, training), targets.hip,
scan.hip's in_remove_box and host.cpp's pt_in_box promise: float32 in source order, every product and sum rounded on its own
(numpy fuses nothing), cos / sin correctly rounded through double, inclusive bounds. ``gt_aug_restate.pts_in_box`` and
``rpn_targets_restate.labels32`` rest on it. Two forms exist in the library and both are stated here:

  gate=True    pt_in_box3d (roipool3d, scan removal, the host ops): NOT(|dx| > 10 or |y - cy| > hh or |dz| > 10) and
               -hl <= x_rot <= hl and -hw <= z_rot <= hw. A NaN y passes the negated test, as in the reference.
  gate=False   the RPN targets: |x_rot| <= hl and |y - cy| <= hh and |z_rot| <= hw, no 10 m gate. A NaN fails.

``extra`` > 0 enlarges the extents as the kernels do, (l + 2e) * 0.5f; ``canonical`` also lowers the bottom, y + e
(kitti_utils.enlarge_box3d), where the RPN targets keep the centre of the box as given.

``face_points`` builds candidates on all six faces and steps them ulp by ulp across; ``classify`` marks the candidates on which a
decision hangs (an input-selection device, not a statement about a kernel); ``thin`` keeps whole step groups, the marked ones
first; the ``*_case`` functions are the inputs of tests/test_box_faces_gpu.py, whose fairness tests/test_box_faces.py asserts
without a kernel.
"""
import functools

import numpy as np

F, D = np.float32, np.float64
GATE = F(10.0)
STEPS = 3


# ---- the predicate ----------------------------------------------------------------------------------------------------------------
def enlarged(box, extra=0.0, canonical=False):
    """h, w, l + (float)(2 extra) in float32; canonical: y + (float)extra as well"""
    b = np.array(box, F).reshape(7)
    if extra:
        e = F(extra)
        b[3:6] = b[3:6] + F(2.0) * e
        if canonical:
            b[1] = b[1] + e
    return b


def box_terms(box, extra=0.0, canonical=False, cy=None):
    """-> dict of float32 cx, cy, cz, hh, hw, hl, cosa, sina; cy: given, or (float)((double)y - (double)h / 2.0)"""
    box = np.asarray(box, F).reshape(7)
    big = enlarged(box, extra, canonical)
    if cy is None:
        src = big if canonical else box
        cy = F(D(src[1]) - D(src[3]) / 2.0)
    return {"cx": box[0], "cy": F(cy), "cz": box[2], "hh": big[3] * F(0.5), "hw": big[4] * F(0.5), "hl": big[5] * F(0.5),
            "cosa": F(np.cos(D(box[6]))), "sina": F(np.sin(D(box[6])))}


def _decide(x_rot, z_rot, dx, dz, ay, t, gate):
    if gate:
        ok = ~((np.abs(dx) > GATE) | (ay > t["hh"]) | (np.abs(dz) > GATE))
        return ok & (x_rot >= -t["hl"]) & (x_rot <= t["hl"]) & (z_rot >= -t["hw"]) & (z_rot <= t["hw"])
    return (np.abs(x_rot) <= t["hl"]) & (ay <= t["hh"]) & (np.abs(z_rot) <= t["hw"])


def membership32(pts, box, extra=0.0, gate=True, canonical=False, cy=None):
    """pts (P,3), box (7) -> inside (P) bool, dict of the float32 intermediates (x_rot, z_rot, ay = |y - cy|, dx, dz) and terms"""
    t = box_terms(box, extra, canonical, cy)
    pts = np.asarray(pts, F).reshape(-1, 3)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dz, ay = x - t["cx"], z - t["cz"], np.abs(y - t["cy"])
        x_rot = dx * t["cosa"] + dz * (-t["sina"])
        z_rot = dx * t["sina"] + dz * t["cosa"]
        inside = _decide(x_rot, z_rot, dx, dz, ay, t, gate)
    assert x_rot.dtype == F and z_rot.dtype == F and ay.dtype == F
    return inside, dict(t, x_rot=x_rot, z_rot=z_rot, ay=ay, dx=dx, dz=dz)


def _fma(a, b, c):
    """fma(a, b, c) of float32 values: the product of two float32 values is exact in float64"""
    return (a.astype(D) * D(b) + c.astype(D)).astype(F)


def classify(pts, box, extra=0.0, gate=True, canonical=False, cy=None):
    """-> dict of (P) bool masks: inside; on_face (inside, and an intermediate EQUALS its bound: `<` for `<=` drops the point);
    contraction_sensitive (the decision changes when either product of x_rot or of z_rot is fused into the sum)"""
    inside, v = membership32(pts, box, extra, gate, canonical, cy)
    with np.errstate(invalid="ignore", over="ignore"):
        on = (np.abs(v["x_rot"]) == v["hl"]) | (np.abs(v["z_rot"]) == v["hw"]) | (v["ay"] == v["hh"])
        c, s, ns = v["cosa"], v["sina"], -v["sina"]
        sens = np.zeros(len(inside), bool)
        for xr in (_fma(v["dx"], c, v["dz"] * ns), _fma(v["dz"], ns, v["dx"] * c)):
            sens |= _decide(xr, v["z_rot"], v["dx"], v["dz"], v["ay"], v, gate) != inside
        for zr in (_fma(v["dx"], s, v["dz"] * c), _fma(v["dz"], c, v["dx"] * s)):
            sens |= _decide(v["x_rot"], zr, v["dx"], v["dz"], v["ay"], v, gate) != inside
    return {"inside": inside, "on_face": inside & on, "contraction_sensitive": sens}


# ---- points on the faces ----------------------------------------------------------------------------------------------------------
def _step(a, k):
    a = a.copy()
    for _ in range(abs(k)):
        a = np.nextafter(a, F(np.inf if k > 0 else -np.inf))
    return a


def face_points(box, per_face, steps, rng, extra=0.0, canonical=False, cy=None):
    """-> pts (P,3) float32, meta dict of (P) int arrays: face (0, 1 = -+l/2; 2, 3 = bottom / top in y; 4, 5 = -+w/2; -1 = the extra
    rows), group (one id per face point and its steps, -1 for the extra rows), step.

    per_face points on each of the six faces of the (enlarged) box, built in float64 and rounded to float32, each stepped
    -steps..steps ulps along one world axis (x or z on the vertical faces, see below; y on the y faces, in ulps of y or of the
    half height, whichever is larger). Extra rows: the centre, a far point,
    rows of NaN, +inf and -inf, a row whose y alone is NaN; for a box longer than 20 m, points at |x - cx| and |z - cz| of 10 and
    at the coordinate's next float whose distance exceeds 10, on either side."""
    t = box_terms(box, extra, canonical, cy)
    c, s = D(t["cosa"]), D(t["sina"])
    half = np.array([t["hl"], t["hh"], t["hw"]], D)
    centre = np.array([t["cx"], t["cy"], t["cz"]], D)
    rows, face, group, step = [], [], [], []
    for f in range(6):
        axis, side = f // 2, (-1.0, 1.0)[f % 2]
        q = rng.uniform(-0.9, 0.9, (per_face, 3)) * half
        q[:, axis] = side * half[axis]
        base = np.stack([centre[0] + q[:, 0] * c + q[:, 2] * s, centre[1] + q[:, 1], centre[2] - q[:, 0] * s + q[:, 2] * c], axis=1).astype(F)
        # x_rot = dx cos - dz sin, z_rot = dx sin + dz cos. A vertical face's points step along the world axis whose ulp moves the
        # face's coordinate most, |weight| * ulp(coordinate): the rounding of x and z displaces it by at most half of both
        # products, which is at most one such step (with equal magnitudes this is the axis the normal leans to)
        wx, wz = (abs(c), abs(s)) if axis == 0 else (abs(s), abs(c))
        along_x = wx * np.spacing(np.abs(base[:, 0])).astype(D) >= wz * np.spacing(np.abs(base[:, 2])).astype(D)
        ids = f * per_face + np.arange(per_face)
        for k in range(-steps, steps + 1):
            p = base.copy()
            if axis == 1:      # near y = 0 an ulp of y is far below an ulp of |y - cy|: there the step is an ulp of the bound
                unit = np.maximum(np.spacing(np.abs(base[:, 1])), np.spacing(t["hh"]))
                p[:, 1] = (base[:, 1].astype(D) + k * unit.astype(D)).astype(F)
            else:
                p[:, 0] = np.where(along_x, _step(base[:, 0], k), base[:, 0])
                p[:, 2] = np.where(along_x, base[:, 2], _step(base[:, 2], k))
            rows.append(p)
            face.append(np.full(per_face, f))
            group.append(ids)
            step.append(np.full(per_face, k))
    c32 = centre.astype(F)
    extra_rows = [c32, (centre + [300.0, 50.0, -200.0]).astype(F), np.full(3, np.nan, F), np.full(3, np.inf, F), np.full(3, -np.inf, F),
                  np.array([c32[0], np.nan, c32[2]], F)]
    if half[0] > 10.0:
        for col in (0, 2):
            for sign in (-1.0, 1.0):
                at, beyond = c32.copy(), c32.copy()
                at[col] = F(centre[col] + sign * 10.0)
                beyond[col] = at[col]
                while not abs(beyond[col] - c32[col]) > GATE:        # float32, as the kernels subtract
                    beyond[col] = np.nextafter(beyond[col], F(sign * np.inf))
                extra_rows += [at, beyond]
    k = len(extra_rows)
    rows.append(np.stack(extra_rows))
    pts = np.concatenate(rows).astype(F)
    meta = {"face": np.concatenate(face + [np.full(k, -1)]), "group": np.concatenate(group + [np.full(k, -1)]),
            "step": np.concatenate(step + [np.zeros(k, np.int64)])}
    return pts, meta


def thin(meta, marks, share, rng):
    """-> (P) bool: the extra rows and `share` whole step groups per face; on a face the groups with a
    contraction-sensitive point first (at most half the share), then those with a point on the face, then the others"""
    keep = meta["group"] < 0
    for f in range(6):
        of = meta["face"] == f
        ids = np.unique(meta["group"][of])
        sens = np.unique(meta["group"][of & marks["contraction_sensitive"]])
        on = np.setdiff1d(np.unique(meta["group"][of & marks["on_face"]]), sens)
        rest = np.setdiff1d(ids, np.concatenate([sens, on]))
        order = np.concatenate([rng.permutation(sens)[:(share + 1) // 2], rng.permutation(on), rng.permutation(rest)])
        keep |= np.isin(meta["group"], order[:share]) & of
    return keep


# ---- boxes ------------------------------------------------------------------------------------------------------------------------
def random_boxes(rng, m):
    """KITTI-like: x in [-30, 30], z in [5, 70] (and above 0.3 |x| + 2, in front of the sensor), l 3-5, w 1.4-2, h 1.3-2, any ry"""
    x = rng.uniform(-30, 30, m)
    z = np.array([rng.uniform(max(5.0, 0.3 * abs(v) + 2.0), 70.0) for v in x])
    return np.stack([x, rng.uniform(1.2, 2.0, m), z, rng.uniform(1.3, 2.0, m), rng.uniform(1.4, 2.0, m), rng.uniform(3.0, 5.0, m),
                     rng.uniform(-np.pi, np.pi, m)], axis=1).astype(F)


def box_set(rng, m):
    """-> boxes (K,7) float32, kinds (K): m "random" boxes; "aligned" ones with ry in {0, +-pi/2, pi} and one "turned" by
    2 pi + 0.3; a "dyadic" box (centre and extents exactly representable, so are its faces); two "gate" boxes with l = 24, along x
    and along z; a box with w = 0 and one with a negative l ("degenerate"); a "far" box that holds nothing (30 m
    and more from every point, yet within the 80 m of a scene: the bounds on the training mode's coordinates are those of that range)"""
    boxes, kinds = list(random_boxes(rng, m)), ["random"] * m
    for ry in (0.0, np.pi / 2, -np.pi / 2, np.pi, 2 * np.pi + 0.3):
        b = random_boxes(rng, 1)[0]
        b[6] = F(ry)
        boxes.append(b)
        kinds.append("aligned" if ry < 6 else "turned")
    boxes += [np.array([8.0, 1.0, 16.0, 1.5, 2.0, 4.0, 0.0], F), np.array([4.0, 1.5, 32.0, 1.5, 2.0, 24.0, 0.0], F),
              np.array([-16.0, 1.5, 48.0, 1.5, 2.0, 24.0, np.pi / 2], F)]
    kinds += ["dyadic", "gate", "gate"]
    flat, neg = random_boxes(rng, 2)
    flat[4], neg[5] = 0.0, -neg[5]
    boxes += [flat, neg, np.array([70.0, 1.5, -20.0, 1.5, 1.6, 4.0, 0.4], F)]
    kinds += ["degenerate", "degenerate", "far"]
    return np.stack(boxes).astype(F), kinds


# ---- clouds -----------------------------------------------------------------------------------------------------------------------
def candidates(boxes, rng, per_face=160, steps=STEPS, **form):
    """face_points of every box in `boxes` -> pts (P,3), meta with an extra key "box" (the row in `boxes`)"""
    pts, metas = [], []
    for k, box in enumerate(boxes):
        p, m = face_points(box, per_face, steps, rng, **{key: v for key, v in form.items() if key != "gate"})
        m["box"] = np.full(len(p), k)
        pts.append(p)
        metas.append(m)
    return np.concatenate(pts), {key: np.concatenate([m[key] for m in metas]) for key in metas[0]}


def marks_of(observed, boxes, meta, **form):
    """classify each candidate against its own box, on the values the predicate will see"""
    out = {key: np.zeros(len(observed), bool) for key in ("inside", "on_face", "contraction_sensitive")}
    for k, box in enumerate(boxes):
        mine = meta["box"] == k
        got = classify(observed[mine], box, **form)
        for key in out:
            out[key][mine] = got[key]
    return out


def thin_all(meta, marks, boxes, share, rng):
    keep = np.zeros(len(meta["box"]), bool)
    for k in range(len(boxes)):
        mine = np.nonzero(meta["box"] == k)[0]
        sub = {key: meta[key][mine] for key in meta}
        keep[mine] = thin(sub, {key: marks[key][mine] for key in marks}, share, rng)
    return keep


def conditions(marks, meta, kinds, gate):
    """the input conditions of a case, from the restatement alone -> dict of on_face, contraction_sensitive (counts), inside_share
    (of the face points) and faces_without_both (box, face) pairs of the boxes that must decide both ways within one ulp step"""
    on_a_face = meta["face"] >= 0
    missing = []
    for k, kind in enumerate(kinds):
        if kind in ("degenerate", "far"):
            continue
        for f in range(6):
            if kind == "gate" and gate and f < 2:
                continue                                  # the faces at +-12 m lie beyond the 10 m gate: nothing there is inside
            at = np.nonzero((meta["box"] == k) & (meta["face"] == f))[0]
            order = at[np.lexsort((meta["step"][at], meta["group"][at]))]
            same = meta["group"][order][1:] == meta["group"][order][:-1]
            if not (same & (marks["inside"][order][1:] != marks["inside"][order][:-1])).any():
                missing.append((k, f))
    return {"on_face": int(marks["on_face"].sum()), "contraction_sensitive": int(marks["contraction_sensitive"].sum()),
            "inside_share": float(marks["inside"][on_a_face].mean()), "faces_without_both": missing}


def case_conditions(scenes, gate):
    """the conditions of one GPU case: counts summed over its scenes (each with marks, meta, kinds)"""
    total = {"on_face": 0, "contraction_sensitive": 0, "inside": 0, "points": 0, "faces_without_both": []}
    for i, s in enumerate(scenes):
        c = conditions(s["marks"], s["meta"], s["kinds"], gate)
        on_a_face = s["meta"]["face"] >= 0
        total["on_face"] += c["on_face"]
        total["contraction_sensitive"] += c["contraction_sensitive"]
        total["inside"] += int(s["marks"]["inside"][on_a_face].sum())
        total["points"] += int(on_a_face.sum())
        total["faces_without_both"] += [(i,) + f for f in c["faces_without_both"]]
    total["inside_share"] = total["inside"] / total["points"]
    return total


def scenes_of(case):
    """a case that keeps per-scene lists under "marks", "meta", "kinds" -> list of per-scene dicts"""
    kinds = case["kinds"]
    return [{"marks": case["marks"][i], "meta": case["meta"][i], "kinds": kinds[i] if isinstance(kinds[0], list) else kinds}
            for i in range(len(case["marks"]))]


def check_conditions(c):
    assert c["on_face"] >= 100 and c["contraction_sensitive"] >= 30 and 0.3 <= c["inside_share"] <= 0.7 and not c["faces_without_both"], c


def scatter(face_pts, n, rng, filler):
    """the face points at seeded positions among n rows, `filler` (callable count -> (count,3)) in the others -> pts (n,3), rows"""
    assert len(face_pts) <= n, (len(face_pts), n)
    rows = np.sort(rng.permutation(n)[:len(face_pts)])
    pts = np.zeros((n, 3), F)
    rest = np.setdiff1d(np.arange(n), rows)
    pts[rest] = filler(len(rest))
    pts[rows] = face_pts
    return pts, rows


def scene_filler(rng, boxes):
    """points over the scene and (half of them) around the boxes' centres"""
    def make(count):
        p = np.stack([rng.uniform(-40, 40, count), rng.uniform(-1, 3, count), rng.uniform(0, 75, count)], axis=1)
        near = rng.uniform(size=count) < 0.5
        which = boxes[rng.integers(0, len(boxes), count)].astype(D)
        p[near] = (which[:, 0:3] - [0, 0.8, 0] + rng.uniform(-3, 3, (count, 3)) * [1, 0.4, 1])[near]
        return p.astype(F)
    return make


# ---- case: ROI pooling (plain: extra 0; canonical and training: the faces of the enlarged boxes) -------------------------------------
POOL_B, POOL_N, POOL_M_RANDOM = 2, 4000, 2
FEW = np.array([1.0, -16.0, 3.0, 1.5, 2.0, 4.0, 0.0], F)        # far above the cloud; two members, both ON a face: see pool_case


@functools.lru_cache(maxsize=None)
def pool_case(extra, seed=0):
    """-> dict: xyz (B,N,3), boxes (B,M,7), kinds, feat (B,N,1) = the row number, and per scene the face points' rows, meta and
    marks. The last box of a scene (FEW) holds exactly two points of the cloud, both on a face of its (enlarged) form."""
    form = dict(extra=extra, gate=True, canonical=extra > 0)
    out = {"xyz": [], "boxes": [], "rows": [], "meta": [], "marks": [], "extra": extra}
    for scene in range(POOL_B):
        rng = np.random.default_rng([seed, scene, int(round(extra * 10))])
        boxes, kinds = box_set(rng, POOL_M_RANDOM)
        live = [k for k, kind in enumerate(kinds) if kind != "far"]
        cand, meta = candidates(boxes[live], rng, **form)
        marks = marks_of(cand, boxes[live], meta, **form)
        keep = thin_all(meta, marks, live, 7, rng)
        few_pts, few_meta = face_points(FEW, 400, 0, rng, **{k: form[k] for k in ("extra", "canonical")})
        on_few = classify(few_pts, FEW, **form)["on_face"]               # cx + hl and cx - hl are float32 values for these extents
        on = [np.nonzero(on_few & (few_meta["face"] == f))[0][0] for f in (0, 1)]
        face_pts = np.concatenate([cand[keep], few_pts[on]])
        pts, rows = scatter(face_pts, POOL_N, rng, scene_filler(rng, boxes[live]))
        out["xyz"].append(pts)
        out["boxes"].append(np.concatenate([boxes, FEW[None]]))
        out["rows"].append(rows[:int(keep.sum())])
        out["meta"].append({key: meta[key][keep] for key in meta})
        out["marks"].append({key: marks[key][keep] for key in marks})
        out["kinds"] = [kinds[k] for k in live]
        out["live"] = live
    out["xyz"], out["boxes"] = np.stack(out["xyz"]), np.stack(out["boxes"])
    out["feat"] = np.broadcast_to(np.arange(POOL_N, dtype=F)[None, :, None], (POOL_B, POOL_N, 1)).copy()
    return out


# ---- case: RPN targets ----------------------------------------------------------------------------------------------------------------
RPN_G, RPN_N, RPN_B, RPN_EXTRA = (1, 64, 65, 130), (1023, 1024, 3001), 2, 0.2


def rpn_boxes(g, n, rng):
    """g rows: random boxes, every fourth one sitting on its predecessor (overlapping pairs, for the order rule), the box set's
    special boxes and two zero rows (padding) in between; -> boxes (g,7), the rows that get face points (on either side of the
    64-box chunk where g allows; the dyadic, gate and turned boxes too where n has the room), their kinds"""
    boxes = random_boxes(rng, g)
    for k in range(1, g, 4):
        boxes[k] = boxes[k - 1]
        boxes[k, 0:3] += np.array([0.4, 0.05, -0.3], F)
        boxes[k, 6] += F(0.1)
    special, kinds = box_set(rng, 0)
    slots = [k for k in range(2, g - 1) if k not in (62, 63, 64, 65)][:len(special) + 2]
    for slot, box in zip(slots, list(special) + [np.zeros(7, F), np.zeros(7, F)]):
        boxes[slot] = box
    faced = sorted({0, 1, 63, 64, g - 1} & set(range(g)))
    if n < 2000 and len(faced) > 4:
        faced.remove(1)
    faced_kinds = ["random"] * len(faced)
    for slot, kind in zip(slots, kinds):
        if kind in ("dyadic", "gate", "turned") and n >= 2000:
            faced.append(slot)
            faced_kinds.append(kind)
    return boxes, faced, faced_kinds


@functools.lru_cache(maxsize=None)
def rpn_case(g, n, with_aug, seed=0):
    """-> dict: pts (B,N,3), gt (B,G,7), alpha (B,G), aug (B,4) or None, and per scene the face points' rows, meta and marks. With
    an augmentation the face points are built on the restatement's augmented boxes, taken back through the inverse augmentation
    in float64 and rounded; the marks are taken on the restatement's augmented values of those (two forms per faced box: the box
    and the enlarged box, both about the targets' centre y - h / 2 in float32)"""
    import rpn_targets_restate as rs
    out = {"pts": [], "gt": [], "alpha": [], "aug": [], "rows": [], "meta": [], "marks": [], "kinds": []}
    for scene in range(RPN_B):
        rng = np.random.default_rng([seed, scene, g, n, int(with_aug)])
        gt, faced, faced_kinds = rpn_boxes(g, n, rng)
        alpha = (rng.uniform(-np.pi, np.pi, g) * (gt[:, 3] > 0)).astype(F)
        row = np.array([1, rng.uniform(-np.pi / 18, np.pi / 18), rng.uniform(0.95, 1.05), scene == 0], F) if with_aug else None
        gt_aug = rs.augment(np.zeros((0, 3), F), gt, alpha, row)[1] if with_aug else gt
        specs = [(k, dict(extra=e, gate=False, cy=gt_aug[k, 1] - gt_aug[k, 3] / F(2))) for e in (0.0, RPN_EXTRA) for k in faced]
        steps = STEPS + int(with_aug)                          # the round trip through the augmentation moves a point an ulp or two
        share = max(2, int((0.9 * n / len(specs) - 14) / (6 * (2 * steps + 1))))
        kept, metas, marks_all = [], [], []
        for i, (k, form) in enumerate(specs):
            p, m = face_points(gt_aug[k], 480, steps, rng, **{key: form[key] for key in ("extra", "cy")})
            m["box"] = np.full(len(p), i)
            src, seen = rpn_roundtrip(p, row) if with_aug else (p, p)
            mk = classify(seen, gt_aug[k], **form)
            keep = thin(m, mk, share, rng)
            kept.append(src[keep])
            metas.append({key: m[key][keep] for key in m})
            marks_all.append({key: mk[key][keep] for key in mk})
        pts, rows = scatter(np.concatenate(kept), n, rng, scene_filler(rng, gt[faced]))
        out["pts"].append(pts)
        out["gt"].append(gt)
        out["alpha"].append(alpha)
        out["aug"].append(row)
        out["rows"].append(rows)
        out["meta"].append({key: np.concatenate([m[key] for m in metas]) for key in metas[0]})
        out["marks"].append({key: np.concatenate([m[key] for m in marks_all]) for key in marks_all[0]})
        out["kinds"].append(faced_kinds * 2)
    for key in ("pts", "gt", "alpha"):
        out[key] = np.stack(out[key])
    out["aug"] = np.stack(out["aug"]) if with_aug else None
    return out


def rpn_roundtrip(p, row):
    """face points built in the augmented frame -> (the scene's input points: the inverse augmentation in float64, rounded;
    the restatement's augmented values of those)"""
    import rpn_targets_restate as rs
    with np.errstate(invalid="ignore", over="ignore"):
        q = p.astype(D)
        if row[3]:
            q[:, 0] = -q[:, 0]
        q = q / D(row[2])
        if row[0]:
            c, s = np.cos(D(row[1])), np.sin(D(row[1]))
            x, z = q[:, 0].copy(), q[:, 2].copy()
            q[:, 0], q[:, 2] = x * c + z * s, -x * s + z * c
    with np.errstate(invalid="ignore", over="ignore"):
        src = q.astype(F)
        return src, rs.augment(src, np.zeros((0, 7), F), np.zeros(0, F), row)[0]


# ---- case: scan removal ---------------------------------------------------------------------------------------------------------------
SCAN_P, SCAN_K, SCAN_N, SCAN_E = 3000, 3, 512, 16


def to_lidar(rect, V2C, R0):
    """the inverse of scan_restate's rectification, in float64 from the float32 calibration"""
    import scan_restate as sr
    m = sr.composite(V2C, R0, D)
    return (np.asarray(rect, D) - m[3]) @ np.linalg.inv(m[:3])


@functools.lru_cache(maxsize=None)
def scan_case(seed=0):
    """-> list of scenes (dicts): pts (P,4) lidar rows, calibration, remove_boxes (K,7) in the rectified frame, extra_pts, keys,
    slot_perm, and the face points' rows, meta, marks -- the marks taken on the rectified values scan_restate.classify gives"""
    import scan_restate as sr
    scenes = []
    for scene in range(2):
        rng = np.random.default_rng([seed, scene, 77])
        V2C, R0, P2, shape = sr.calib(scene + 3)
        z = rng.uniform(12, 34, SCAN_K)
        boxes = np.stack([rng.uniform(-0.15, 0.15, SCAN_K) * z, rng.uniform(1.4, 1.8, SCAN_K), z, rng.uniform(1.3, 1.6, SCAN_K), rng.uniform(1.4, 2.0, SCAN_K),
                          rng.uniform(3.0, 5.0, SCAN_K), rng.uniform(-np.pi, np.pi, SCAN_K)], axis=1).astype(F)
        cand, meta = candidates(boxes, rng, per_face=200)

        def rectified(rect):
            with np.errstate(invalid="ignore"):
                lidar = np.concatenate([to_lidar(rect, V2C, R0), rng.uniform(0, 1, (len(rect), 1))], axis=1).astype(F)
            return lidar, sr.classify(lidar, len(lidar), V2C, R0, P2, shape)
        lidar, (seen, _, valid, _) = rectified(cand)
        marks = marks_of(seen, boxes, meta)
        keep = thin_all(meta, marks, range(SCAN_K), 21, rng)
        finite = np.isfinite(cand).all(axis=1)
        assert valid[keep & finite & (meta["face"] >= 0)].all()
        count = SCAN_P - int(keep.sum())
        fz = rng.uniform(6, 60, count)
        fill = np.stack([rng.uniform(-0.2, 0.2, count) * fz, rng.uniform(0.0, 1.7, count), fz], axis=1)
        near = rng.uniform(size=count) < 0.4
        fill[near] = (boxes[rng.integers(0, SCAN_K, count), 0:3].astype(D) - [0, 0.7, 0] + rng.uniform(-2.5, 2.5, (count, 3)) * [1, 0.3, 1])[near]
        fill[::11, 2] = -fill[::11, 2]                                   # behind the camera: not valid
        pts = np.zeros((SCAN_P, 4), F)
        rows = np.sort(rng.permutation(SCAN_P)[:int(keep.sum())])
        pts[rows] = lidar[keep]
        pts[np.setdiff1d(np.arange(SCAN_P), rows)] = rectified(fill)[0]
        extra = np.concatenate([boxes[0, 0:3] + rng.uniform(-1, 1, (SCAN_E, 3)) * F(0.5), rng.uniform(0, 1, (SCAN_E, 1))], axis=1).astype(F)
        scenes.append({"pts": pts, "num_raw": SCAN_P - scene, "V2C": V2C, "R0": R0, "P2": P2, "img_shape": shape, "remove_boxes": boxes,
                       "extra_pts": extra, "num_extra": 5, "keys": rng.integers(-2 ** 31, 2 ** 31, SCAN_P + SCAN_E).astype(np.int32),
                       "slot_perm": rng.permutation(SCAN_N).astype(np.int32), "rows": rows, "meta": {key: meta[key][keep] for key in meta},
                       "marks": {key: marks[key][keep] for key in marks}, "kinds": ["random"] * SCAN_K})
    return scenes


# ---- case: one cloud for every family ---------------------------------------------------------------------------------------------------
CROSS_N, CROSS_M = 2048, 6


@functools.lru_cache(maxsize=None)
def cross_case(seed=0):
    """random boxes and their face points (no extra rows: finite, within 10 m of their box's centre), extra = 0, filler around"""
    rng = np.random.default_rng([seed, 99])
    boxes = random_boxes(rng, CROSS_M)
    boxes[:, 1] = np.minimum(boxes[:, 1], F(1.9))
    cand, meta = candidates(boxes, rng)
    marks = marks_of(cand, boxes, meta)
    keep = thin_all(meta, marks, range(CROSS_M), 7, rng) & (meta["group"] >= 0)

    def filler(count):
        which = boxes[rng.integers(0, CROSS_M, count)].astype(D)
        return (which[:, 0:3] - [0, 0.8, 0] + rng.uniform(-4, 4, (count, 3)) * [1, 0.3, 1]).astype(F)
    pts, rows = scatter(cand[keep], CROSS_N, rng, filler)
    return {"pts": pts, "boxes": boxes, "rows": rows, "meta": {key: meta[key][keep] for key in meta},
            "marks": {key: marks[key][keep] for key in marks}, "kinds": ["random"] * CROSS_M}

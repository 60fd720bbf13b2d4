"""Exact float64 geometry of rotated rectangles: the yardstick tests/test_exact_geometry*.py hold the oracle, the evaluator's
restatement and the device kernels to.

Nothing here is taken from the oracle's algorithm (oracle/epnet_oracle.c, box_overlap) or from the evaluator's
(tests/kitti_eval_restate.py, rotated_inter): no segment-crossing bookkeeping, no angle sort, no margins. The intersection of two
rectangles is the Sutherland-Hodgman clip of one against the four half-planes of the other, its area the shoelace sum, both in
float64 on corners computed in float64 from the float32 inputs. Only the corner CONVENTION is shared with the code under test,
because it defines which rectangle a row of numbers means:

  BEV form   (x1, y1, x2, y2, ry): the axis-aligned rectangle turned about its centre, (dx, dy) -> (dx cos + dy sin, -dx sin + dy cos)
             (rotate_around_center of the reference's iou3d kernel);
  eval form  (cx, cy, x_d, y_d, angle): the same turn of (+-x_d / 2, +-y_d / 2) about (cx, cy) (rbbox_to_corners of the reference's
             rotate_iou.py, `_corners` in tests/kitti_eval_restate.py).

A centre-form row (cx, cy, l, w, ry) is an eval-form box as it stands and `bev_of_centre` makes its BEV form.

The clip is vectorised over pairs: a polygon is a (P, 8, 2) array with a per-pair vertex count (a quadrilateral clipped by four
half-planes has at most eight vertices).
"""
import numpy as np

F32 = np.float32
MAX_VERTS = 8

# ---- the two measured bounds ------------------------------------------------------------------------------------------------------
# Largest |implementation - exact area| over the non-degenerate families below (N_PAIRS pairs each, seed FAMILY_SEED) and, for
# iou3d, the synthetic proposal sets, measured on the CPU by measure_iou3d / measure_proposals / measure_eval (python tests/exact_geometry.py prints the table).
# Each bound is four times the largest measured value, rounded up to one significant digit: room for the families' other seeds
# and for the 1e-5 between a device kernel and the oracle, and still two orders of magnitude below the error of a dropped or
# misordered polygon vertex (1e-2 or more for boxes of these sizes).
MEASURED_IOU3D = {"general": 2.057e-05, "parallel": 1.859e-05, "plus90": 2.047e-05, "nested_same": 2.146e-05, "nested_diff": 8.775e-06,
                  "near_angle": 5.582e-05, "aa_collinear": 1.431e-05, "aa_touching": 0.0, "far": 0.0,
                  "proposals_0.2": 1.984e-05, "proposals_0.8": 1.823e-05, "proposals_1.5": 2.588e-05}
MEASURED_EVAL = {"general": 1.558e-04, "parallel": 9.611e-05, "plus90": 2.433e-04, "nested_same": 1.346e-05, "nested_diff": 6.583e-06,
                 "aa_collinear": 8.345e-06, "aa_touching": 2.116e-06, "far": 0.0}
B_IOU3D = 3e-4        # 4 * 5.582e-05 = 2.23e-4, rounded up to one significant digit
B_EVAL = 1e-3         # 4 * 2.433e-04 = 9.73e-4, rounded up to one significant digit
FAMILY_SEED = 20260
N_PAIRS = 2000        # per family for the oracle
N_PAIRS_EVAL = 600    # per family for the restatement (a Python loop per pair)
FLOAT32_SLOP = 8 * 2.0 ** -24   # up to eight float32 roundings of a ratio that is at most 1


# ---- corners ----------------------------------------------------------------------------------------------------------------------
def _turn(dx, dy, cx, cy, angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.stack([dx * c[:, None] + dy * s[:, None] + cx[:, None], -dx * s[:, None] + dy * c[:, None] + cy[:, None]], axis=-1)


def corners_bev(boxes):
    """(n,5) [x1,y1,x2,y2,ry] -> (n,4,2) float64"""
    b = np.asarray(boxes, F32).astype(np.float64).reshape(-1, 5)
    cx, cy = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2
    x = np.stack([b[:, 0], b[:, 2], b[:, 2], b[:, 0]], axis=1) - cx[:, None]
    y = np.stack([b[:, 1], b[:, 1], b[:, 3], b[:, 3]], axis=1) - cy[:, None]
    return _turn(x, y, cx, cy, b[:, 4])


def corners_eval(boxes):
    """(n,5) [cx,cy,x_d,y_d,angle] (cast to float32 first, as the evaluator does) -> (n,4,2) float64"""
    b = np.asarray(boxes).astype(F32).astype(np.float64).reshape(-1, 5)
    hx, hy = b[:, 2] / 2, b[:, 3] / 2
    x = np.stack([-hx, -hx, hx, hx], axis=1)
    y = np.stack([-hy, hy, hy, -hy], axis=1)
    return _turn(x, y, b[:, 0], b[:, 1], b[:, 4])


# ---- polygon clip -----------------------------------------------------------------------------------------------------------------
def _signed_area(pts, count):
    p = pts.shape[0]
    rows = np.arange(p)
    total = np.zeros(p)
    for i in range(pts.shape[1]):
        live = i < count
        nxt = pts[rows, np.where(live, (i + 1) % np.maximum(count, 1), 0)]
        cur = pts[:, i]
        total += np.where(live, cur[:, 0] * nxt[:, 1] - nxt[:, 0] * cur[:, 1], 0.0)
    return total / 2


def intersection_area_corners(ca, cb):
    """ca, cb (P,4,2) float64 rectangles (either orientation) -> (P,) float64 area of their intersection"""
    ca, cb = np.asarray(ca, np.float64), np.asarray(cb, np.float64)
    p = ca.shape[0]
    rows = np.arange(p)
    four = np.full(p, 4)
    area_a, area_b = _signed_area(ca, four), _signed_area(cb, four)
    sign = np.where(area_b >= 0, 1.0, -1.0)                      # inside = left of a counter-clockwise edge
    pts = np.zeros((p, MAX_VERTS, 2))
    pts[:, :4] = ca
    count = four.copy()
    for e in range(4):
        a, b = cb[:, e], cb[:, (e + 1) % 4]
        ex, ey = (b - a)[:, 0], (b - a)[:, 1]
        dist = sign[:, None] * (ex[:, None] * (pts[:, :, 1] - a[:, 1, None]) - ey[:, None] * (pts[:, :, 0] - a[:, 0, None]))
        out = np.zeros_like(pts)
        n_out = np.zeros(p, np.int64)
        for i in range(MAX_VERTS):
            live = i < count
            j = np.where(live, (i + 1) % np.maximum(count, 1), 0)
            d0, d1 = dist[:, i], dist[rows, j]
            p0, p1 = pts[:, i], pts[rows, j]
            keep = live & (d0 >= 0)
            r = rows[keep]
            out[r, n_out[r]] = p0[r]
            n_out[r] += 1
            cross = live & ((d0 >= 0) != (d1 >= 0))
            r = rows[cross]
            t = d0[r] / (d0[r] - d1[r])
            out[r, n_out[r]] = p0[r] + t[:, None] * (p1[r] - p0[r])
            n_out[r] += 1
        pts, count = out, n_out
    area = np.abs(_signed_area(pts, count))
    return np.where((area_a == 0) | (area_b == 0), 0.0, area)   # a rectangle of no area shares none


def _pairs(fn, a, b):
    return intersection_area_corners(fn(a), fn(b))


def _matrix(fn, a, b):
    ca, cb = fn(a), fn(b)
    n, m = ca.shape[0], cb.shape[0]
    if n == 0 or m == 0:
        return np.zeros((n, m))
    return intersection_area_corners(np.repeat(ca, m, axis=0), np.tile(cb, (n, 1, 1))).reshape(n, m)


def overlap_bev_pairs(a, b):
    return _pairs(corners_bev, a, b)


def overlap_bev(a, b):
    """(n,5) x (m,5) BEV form -> (n,m) exact intersection areas"""
    return _matrix(corners_bev, a, b)


def overlap_eval_pairs(a, b):
    return _pairs(corners_eval, a, b)


def overlap_eval(a, b):
    return _matrix(corners_eval, a, b)


# ---- what the code under test derives from the area ------------------------------------------------------------------------------
def area_bev(boxes):
    b = np.asarray(boxes, F32).astype(np.float64).reshape(-1, 5)
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def iou_bev(a, b):
    ov = overlap_bev(a, b)
    return ov / (area_bev(a)[:, None] + area_bev(b)[None, :] - ov)


def bev_of_boxes3d(boxes):
    """(n,7) [x,y,z,h,w,l,ry] -> the float32 BEV rows the 3-D IoU hands to the rectangle overlap (x -+ l/2, z -+ w/2 in float32):
    the rounding of that conversion belongs to the box, the intersection of the resulting rectangles is what is exact"""
    x = np.asarray(boxes, F32).reshape(-1, 7)
    two = F32(2)
    return np.stack([x[:, 0] - x[:, 5] / two, x[:, 2] - x[:, 4] / two, x[:, 0] + x[:, 5] / two, x[:, 2] + x[:, 4] / two, x[:, 6]],
                    axis=1).astype(F32)


def _height_overlap(a_bottom, a_h, b_bottom, b_h):
    """y points down: a box spans [y - h, y]"""
    return np.maximum(np.minimum(a_bottom, b_bottom) - np.maximum(a_bottom - a_h, b_bottom - b_h), 0.0)


def iou3d(a, b, pairs=False):
    """(n,7) x (m,7) [x,y,z,h,w,l,ry], y = bottom centre -> (n,m) 3-D IoU (or (n,) of corresponding rows)"""
    a64, b64 = np.asarray(a, F32).astype(np.float64).reshape(-1, 7), np.asarray(b, F32).astype(np.float64).reshape(-1, 7)
    va, vb = a64[:, 3] * a64[:, 4] * a64[:, 5], b64[:, 3] * b64[:, 4] * b64[:, 5]
    if pairs:
        o3 = overlap_bev_pairs(bev_of_boxes3d(a), bev_of_boxes3d(b)) * _height_overlap(a64[:, 1], a64[:, 3], b64[:, 1], b64[:, 3])
        return o3 / (va + vb - o3)
    o3 = overlap_bev(bev_of_boxes3d(a), bev_of_boxes3d(b)) * _height_overlap(a64[:, 1, None], a64[:, 3, None], b64[None, :, 1],
                                                                               b64[None, :, 3])
    return o3 / (va[:, None] + vb[None, :] - o3)


def eval_bev(boxes, query_boxes, criterion=-1):
    """the evaluator's rotate_iou_gpu_eval: boxes (n,5), query_boxes (k,5) eval form -> (n,k); criterion -1 IoU, 0 over the query
    box's area, 1 over the row box's area, anything else the area itself"""
    b32, q32 = np.asarray(boxes).astype(F32).astype(np.float64), np.asarray(query_boxes).astype(F32).astype(np.float64)
    ai = overlap_eval(boxes, query_boxes)
    area_q, area_b = (q32[:, 2] * q32[:, 3])[None, :], (b32[:, 2] * b32[:, 3])[:, None]
    if criterion == -1:
        return ai / (area_q + area_b - ai)
    if criterion == 0:
        return ai / area_q
    if criterion == 1:
        return ai / area_b
    return ai


def eval_3d(boxes, qboxes):
    """the evaluator's d3_box_overlap: (n,7) x (k,7) float64 [x,y,z,l,h,w,ry] -> (n,k)"""
    b, q = np.asarray(boxes, np.float64).reshape(-1, 7), np.asarray(qboxes, np.float64).reshape(-1, 7)
    ai = overlap_eval(b[:, [0, 2, 3, 5, 6]], q[:, [0, 2, 3, 5, 6]])
    o3 = ai * _height_overlap(b[:, 1, None], b[:, 4, None], q[None, :, 1], q[None, :, 4])
    return o3 / ((b[:, 3] * b[:, 4] * b[:, 5])[:, None] + (q[:, 3] * q[:, 4] * q[:, 5])[None, :] - o3)


# ---- tolerances, derived from a bound on the AREA ----------------------------------------------------------------------------------
def ratio_tolerance(bound, smallest, height=1.0):
    """|o'/(sa+sb-o') - o/(sa+sb-o)| for |o' - o| <= bound * height. d/do [o/(s-o)] = s/(s-o)^2 with s = sa+sb, and the union
    u = s - o is at least max(sa, sb) >= s/2 because o <= min(sa, sb); so the slope is at most 2/u <= 2/smallest, where
    `smallest` is the smallest box area (volume) of the case; the computed o' may shrink u by the bound itself. FLOAT32_SLOP
    covers the float32 roundings of the products, the sum and the division on a ratio of at most 1."""
    err = bound * height
    return 2 * err / (smallest - err) + FLOAT32_SLOP


def part_tolerance(bound, smallest):
    """|o'/s - o/s| for the one-box criteria 0 / 1"""
    return bound / smallest + FLOAT32_SLOP


def iou_tolerance(a, b):
    """BEV IoU of BEV-form boxes: B_IOU3D * 2 / (smallest box area of the case)"""
    return ratio_tolerance(B_IOU3D, min(area_bev(a).min(), area_bev(b).min()))


def iou3d_tolerance(a7, b7, bound=None, columns=(3, 4, 5), height=3):
    """3-D IoU of 7-column boxes: the shared volume is the area times the height overlap, so it is off by at most the area's bound
    times the largest height overlap of the case (at most the smaller of the two largest heights); the smallest box is the
    smallest volume. `columns` are the three size columns, `height` the height's (the evaluator's order is l, h, w)."""
    a, b = np.asarray(a7, np.float64).reshape(-1, 7), np.asarray(b7, np.float64).reshape(-1, 7)
    tallest = min(a[:, height].max(), b[:, height].max())
    smallest = min(np.prod(a[:, columns], axis=1).min(), np.prod(b[:, columns], axis=1).min())
    return ratio_tolerance(B_IOU3D if bound is None else bound, smallest, tallest)


# ---- greedy NMS -------------------------------------------------------------------------------------------------------------------
def greedy_nms(iou, thresh):
    """boxes in score order, iou (n,n): keep a box unless a kept earlier one has iou > thresh with it -> kept positions"""
    n = iou.shape[0]
    dead = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if dead[i]:
            continue
        keep.append(i)
        dead[i + 1:] |= iou[i, i + 1:] > thresh
    return np.array(keep, np.int64)


# ---- box families -----------------------------------------------------------------------------------------------------------------
# centre form (cx, cy, l, w, ry) float32: centres x in [-40, 40], y in [0, 70], length 1..5, width 0.5..2.5, any angle
NON_DEGENERATE = ("general", "parallel", "plus90", "nested_same", "nested_diff", "near_angle", "aa_collinear", "aa_touching", "far")
DEGENERATE = ("identical", "plus180")
NON_DEGENERATE_EVAL = tuple(f for f in NON_DEGENERATE if f != "near_angle")    # the evaluator's intersection degenerates on it
DEGENERATE_EVAL = DEGENERATE + ("near_angle",)


def base_boxes(n, rng, clusters=0):
    if clusters:
        cen = np.stack([rng.uniform(-40, 40, clusters), rng.uniform(0, 70, clusters)], axis=1)[rng.randint(0, clusters, n)]
        cen = cen + rng.uniform(-1.5, 1.5, (n, 2))
    else:
        cen = np.stack([rng.uniform(-40, 40, n), rng.uniform(0, 70, n)], axis=1)
    return np.stack([cen[:, 0], cen[:, 1], rng.uniform(1, 5, n), rng.uniform(0.5, 2.5, n), rng.uniform(-np.pi, np.pi, n)], axis=1)


def _grid(v, step):
    return np.round(v / step) * step


def prepare(name, a, rng):
    """the first boxes of family `name` from base boxes: the nested families need room for an inner box of area >= 0.3, the
    axis-aligned ones sit on a 1/64 grid with sizes on a 1/32 grid (centre -+ size / 2 is then exact in float32, in both forms)"""
    a, n = a.copy(), a.shape[0]
    if name == "nested_same":
        a[:, 2], a[:, 3] = rng.uniform(2, 5, n), rng.uniform(1, 2.5, n)
    elif name == "nested_diff":
        a[:, 2], a[:, 3] = rng.uniform(2.5, 5, n), rng.uniform(1.5, 2.5, n)
    elif name.startswith("aa_"):
        a[:, 0:2], a[:, 2:4], a[:, 4] = _grid(a[:, 0:2], 1 / 64), _grid(a[:, 2:4], 1 / 32), 0.0
    elif name == "plus180":
        a = a.astype(F32).astype(np.float64)
    return a


def derive(name, a, rng):
    """the partner of every row of `a` (prepared float64 centre form) in family `name`; returns (a, b) float32"""
    n = a.shape[0]
    b = a.copy()

    def along(box, du, dv):   # a shift of (du, dv) in the box's own frame, in world coordinates
        c, s = np.cos(box[:, 4]), np.sin(box[:, 4])
        return np.stack([du * c + dv * s, -du * s + dv * c], axis=1)

    if name == "general":
        b[:, 0:2] += rng.uniform(-1.5, 1.5, (n, 2))
        b[:, 2], b[:, 3], b[:, 4] = rng.uniform(1, 5, n), rng.uniform(0.5, 2.5, n), rng.uniform(-np.pi, np.pi, n)
    elif name == "parallel":
        b[:, 0:2] += along(a, rng.uniform(-1, 1, n) * a[:, 2], rng.uniform(-1, 1, n) * a[:, 3])
        b[:, 2], b[:, 3] = rng.uniform(1, 5, n), rng.uniform(0.5, 2.5, n)
    elif name == "plus90":
        b[:, 2], b[:, 3] = rng.uniform(1, 5, n), rng.uniform(0.5, 2.5, n)
        b[:, 4] = a[:, 4] + np.pi / 2
    elif name == "nested_same":
        b[:, 2:4] = a[:, 2:4] * rng.uniform(0.5, 0.9, (n, 2))
        b[:, 0:2] += along(a, rng.uniform(-0.45, 0.45, n) * (a[:, 2] - b[:, 2]), rng.uniform(-0.45, 0.45, n) * (a[:, 3] - b[:, 3]))
    elif name == "nested_diff":
        radius = 0.45 * a[:, 3] * rng.uniform(0.7, 0.95, n)                        # b's half diagonal: inside a at any angle
        turn = rng.uniform(0.4, 1.0, n)
        b[:, 2], b[:, 3], b[:, 4] = 2 * radius * np.cos(turn), 2 * radius * np.sin(turn), rng.uniform(-np.pi, np.pi, n)
        room = 0.5 * a[:, 3] - radius
        b[:, 0:2] += along(a, rng.uniform(-0.9, 0.9, n) * room * 0.7, rng.uniform(-0.9, 0.9, n) * room * 0.7)
    elif name == "near_angle":
        b[:, 4] = a[:, 4] + rng.uniform(-1e-3, 1e-3, n)             # same centre and size: all four edge pairs nearly coincide
    elif name in ("aa_collinear", "aa_touching"):
        b[:, 2:4] = _grid(np.stack([rng.uniform(1, 5, n), rng.uniform(0.5, 2.5, n)], axis=1), 1 / 32)
        if name == "aa_collinear":   # lower edges on one line, overlapping in x
            b[:, 1] = a[:, 1] - a[:, 3] / 2 + b[:, 3] / 2
            b[:, 0] = a[:, 0] + _grid(rng.uniform(-0.4, 0.4, n) * (a[:, 2] + b[:, 2]), 1 / 64)
        else:                        # b's left edge on a's right edge, overlapping in y
            b[:, 0] = a[:, 0] + a[:, 2] / 2 + b[:, 2] / 2
            b[:, 1] = a[:, 1] + _grid(rng.uniform(-0.4, 0.4, n) * (a[:, 3] + b[:, 3]), 1 / 64)
    elif name == "far":
        far = rng.uniform(0, 2 * np.pi, n)
        b[:, 0:2] += (20 + rng.uniform(0, 20, n))[:, None] * np.stack([np.cos(far), np.sin(far)], axis=1)
        b[:, 2], b[:, 3], b[:, 4] = rng.uniform(1, 5, n), rng.uniform(0.5, 2.5, n), rng.uniform(-np.pi, np.pi, n)
    elif name == "identical":
        pass
    elif name == "plus180":
        b[:, 4] = (a[:, 4].astype(F32) + F32(np.pi)).astype(np.float64)
    else:
        raise KeyError(name)
    return a.astype(F32), b.astype(F32)


def _seed_of(name, seed):
    return seed + 1000 * (NON_DEGENERATE + DEGENERATE).index(name)


def family_pairs(name, n, seed=FAMILY_SEED):
    """-> (a, b): (n,5) float32 centre-form rows, pair i = (a[i], b[i])"""
    rng = np.random.RandomState(_seed_of(name, seed))
    return derive(name, prepare(name, base_boxes(n, rng), rng), rng)


def family_matrix(name, na, nb, seed=FAMILY_SEED):
    """-> (a (na,5), b (nb,5)) centre form: b[j] is the family partner of a[j % na]; the a's sit in a few clusters, so pairs off
    that diagonal overlap in general position as well"""
    rng = np.random.RandomState(_seed_of(name, seed) + 7)
    a0 = prepare(name, base_boxes(na, rng, clusters=max(2, na // 12)), rng)
    _, b = derive(name, a0[np.arange(nb) % na], rng)
    return a0.astype(F32), b


def bev_of_centre(c):
    """centre form -> BEV form, float32 (exact for the grid families)"""
    c = np.asarray(c, F32).reshape(-1, 5)
    two = F32(2)
    return np.stack([c[:, 0] - c[:, 2] / two, c[:, 1] - c[:, 3] / two, c[:, 0] + c[:, 2] / two, c[:, 1] + c[:, 3] / two, c[:, 4]],
                    axis=1).astype(F32)


def lift_boxes3d(c, rng, near=None):
    """centre form -> (n,7) float32 [x, y, z, h, w, l, ry] with heights 1..2.5 and bottoms 1..2.5; `near` (n,7): bottoms within
    0.8 of those rows' so that most heights overlap"""
    c = np.asarray(c, F32).reshape(-1, 5)
    n = c.shape[0]
    h = rng.uniform(1.0, 2.5, n)
    y = rng.uniform(1.0, 2.5, n) if near is None else near[:, 1] + rng.uniform(-0.8, 0.8, n)
    return np.stack([c[:, 0], y, c[:, 1], h, c[:, 3], c[:, 2], c[:, 4]], axis=1).astype(F32)


def eval_boxes3d(b7):
    """[x,y,z,h,w,l,ry] float32 -> the evaluator's float64 [x,y,z,l,h,w,ry]"""
    b7 = np.asarray(b7, np.float64).reshape(-1, 7)
    return np.ascontiguousarray(b7[:, [0, 1, 2, 5, 3, 4, 6]])


# ---- the inputs of the GPU tests, built here so that the CPU tests can check what those tests rely on ----------------------------
DEGENERATE_SEED_IOU3D = {"identical": 1, "plus180": 3}   # seeds at which the oracle's margin really fails on some pair
MATRIX_SHAPE = (67, 130)        # 64 b x 4 a per workgroup in the pairwise kernels: two b tiles, seventeen a tiles, both ragged
PAIRS_COUNT = 300               # 256 pairs per workgroup
NMS_STARTS = (0.1, 0.5, 0.7)
NMS_STEP, NMS_MOVES = 0.0137, 5
NMS_CASES = (("general", 130, 1), ("parallel", 130, 1), ("general", 300, 6), ("parallel", 300, 3))   # (family, n, seed)
RCNN_M, RCNN_G = 75, 12         # 256 // 12 = 21 ROIs per workgroup: 75 = 3 * 21 + 12
RCNN_VALID = (12, 7)            # scene 1 ends in five all-zero ground-truth rows
RCNN_SEED = 5
EVAL_FRAMES = ((70, 5), (9, 4), (0, 3), (33, 7), (130, 2))   # (rows = detections, cols = ground truths) per frame
EVAL_FRAMES_SMALL = ((12, 5), (9, 4), (0, 3), (20, 6))


def matrix_case(name, lifted=False):
    """-> BEV rows (a (67,5), b (130,5)) or, lifted, 7-column boxes"""
    a, b = family_matrix(name, *MATRIX_SHAPE)
    if not lifted:
        return bev_of_centre(a), bev_of_centre(b)
    rng = np.random.RandomState(_seed_of(name, FAMILY_SEED) + 11)
    a7 = lift_boxes3d(a, rng)
    return a7, lift_boxes3d(b, rng, near=a7[np.arange(b.shape[0]) % a.shape[0]])


def pairs_case(name, seed=FAMILY_SEED):
    """-> 7-column (a (300,7), b (300,7)), pair i = (a[i], b[i])"""
    a, b = family_pairs(name, PAIRS_COUNT, seed + 3)
    rng = np.random.RandomState(_seed_of(name, seed) + 13)
    a7 = lift_boxes3d(a, rng)
    return a7, lift_boxes3d(b, rng, near=a7)


def nms_case(name, n, seed):
    """n BEV boxes in score order: groups of four (a, the partner of a, the partner of that partner, a near copy of one of the
    three: IoU above 0.7) of family `name`, shuffled by a random score"""
    rng = np.random.RandomState(seed)
    k = (n + 3) // 4
    a = prepare(name, base_boxes(k, rng), rng)
    _, b = derive(name, a, rng)
    _, c = derive(name, b.astype(np.float64), rng)
    d = np.stack([a, b, c])[rng.randint(0, 3, k), np.arange(k)].astype(np.float64)
    d[:, 0:2] += rng.uniform(-0.1, 0.1, (k, 2))
    d[:, 2:4] *= rng.uniform(0.95, 1.05, (k, 2))
    d[:, 4] += rng.uniform(-0.03, 0.03, k)
    boxes = np.concatenate([a.astype(F32), b, c, d.astype(F32)])[:n]
    return bev_of_centre(boxes[np.argsort(-rng.rand(n), kind="stable")])


def clear_threshold(iou, start, tol):
    """the first of start, start + 0.0137, ... (five moves at most) further than tol from every entry of iou; None without one"""
    vals = iou[np.triu_indices(iou.shape[0], 1)]
    for move in range(NMS_MOVES + 1):
        t = start + move * NMS_STEP
        if np.abs(vals - t).min() > tol:
            return t
    return None


def rcnn_case(seed=RCNN_SEED):
    """-> rois (2,75,7), gt (2,12,7) float32: the ground truths in three clusters, every ROI a moved, resized, turned copy of one"""
    rng = np.random.RandomState(seed)
    rois, gts = np.zeros((2, RCNN_M, 7), F32), np.zeros((2, RCNN_G, 7), F32)
    for k, valid in enumerate(RCNN_VALID):
        g5 = base_boxes(valid, rng, clusters=3)
        g7 = lift_boxes3d(g5, rng)
        pick = rng.randint(0, valid, RCNN_M)
        r5 = g5[pick].copy()
        r5[:, 0:2] += rng.uniform(-0.6, 0.6, (RCNN_M, 2))
        r5[:, 2:4] *= rng.uniform(0.8, 1.2, (RCNN_M, 2))
        r5[:, 4] += np.where(np.arange(RCNN_M) % 2 == 0, rng.uniform(-0.3, 0.3, RCNN_M), rng.uniform(-np.pi, np.pi, RCNN_M))
        rois[k], gts[k, :valid] = lift_boxes3d(r5, rng, near=g7[pick]), g7
    return rois, gts


def eval_frames(name, sizes=EVAL_FRAMES, lifted=False, seed=FAMILY_SEED):
    """per frame (rows, cols) of family `name`: cols = the first boxes (ground truths), rows = partners (detections); float64 eval
    form (n,5), or lifted the evaluator's (n,7) [x,y,z,l,h,w,ry]"""
    rows, cols = [], []
    for f, (nr, nc) in enumerate(sizes):
        a, b = family_matrix(name, nc, nr, seed + 31 * (f + 1))
        if lifted:
            rng = np.random.RandomState(seed + 17 * (f + 1))
            a7 = lift_boxes3d(a, rng)
            b7 = lift_boxes3d(b, rng, near=a7[np.arange(nr) % nc])
            rows.append(eval_boxes3d(b7)); cols.append(eval_boxes3d(a7))
        else:
            rows.append(b.astype(np.float64)); cols.append(a.astype(np.float64))
    return rows, cols


# ---- measuring the bounds ---------------------------------------------------------------------------------------------------------
def round_up_one_digit(v):
    if v <= 0:
        return 0.0
    e = int(np.floor(np.log10(v)))
    m = np.ceil(v / 10.0 ** e - 1e-12)
    return float("%de%d" % (int(m), e))


def measure_iou3d(oracle, families=NON_DEGENERATE, n=N_PAIRS, seed=FAMILY_SEED):
    """-> {family: largest |oracle.boxes_overlap_bev - exact|} (+ the synthetic proposal sets)"""
    out = {}
    for name in families:
        a, b = (bev_of_centre(v) for v in family_pairs(name, n, seed))
        got = np.concatenate([np.diagonal(oracle.boxes_overlap_bev(a[k:k + 250], b[k:k + 250])) for k in range(0, n, 250)])
        out[name] = float(np.abs(got.astype(np.float64) - overlap_bev_pairs(a, b)).max())
    return out


def measure_proposals(oracle, jitters=(0.2, 0.8, 1.5), num=96):
    from epnet_amd import kitti_utils, synth
    out = {}
    for k, jitter in enumerate(jitters):
        boxes, _ = synth.proposal_boxes(num, seed=31 + k, num_objects=8, jitter=jitter)
        bev = kitti_utils.boxes3d_to_bev_torch(boxes).numpy()
        out["proposals_%g" % jitter] = float(np.abs(oracle.boxes_overlap_bev(bev, bev).astype(np.float64) - overlap_bev(bev, bev))[
            ~np.eye(num, dtype=bool)].max())
    return out


def restated_pairs(a, b):
    """kitti_eval_restate.rotated_inter(query = b[i], box = a[i]) per pair, float32"""
    import kitti_eval_restate as kr
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.array([kr.rotated_inter(b[i], a[i]) for i in range(a.shape[0])], F32)


def measure_eval(families=NON_DEGENERATE_EVAL, n=N_PAIRS_EVAL, seed=FAMILY_SEED):
    out = {}
    for name in families:
        a, b = family_pairs(name, n, seed)
        out[name] = float(np.abs(restated_pairs(a, b).astype(np.float64) - overlap_eval_pairs(a, b)).max())
    return out


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import oracle as _oracle
    _oracle.build()
    m3 = dict(measure_iou3d(_oracle), **measure_proposals(_oracle))
    me = measure_eval()
    for title, table in (("iou3d", m3), ("eval", me)):
        for key, val in table.items():
            print("%-6s %-16s %.3e" % (title, key, val))
        print("%-6s bound = %g" % (title, round_up_one_digit(4 * max(table.values()))))

"""TEST INFRASTRUCTURE: numpy restatement of the GT-database augmentation (include/epnet_ops.h: epnet_gt_aug_place,
epnet_gt_aug_points, epnet_scan_prepare_aug; reference: apply_gt_aug_to_one_scene, lib/datasets/kitti_rcnn_dataset.py:590-696).

Written from the contract in the header, one scene at a time: ``place`` is the loop of tries, ``object_points`` the accepted
objects' rows, ``prepare_aug`` the sampling over raw rows and extra rows (on scan_restate's classify and select). The overlap
decision is float64 on the float32 box values, the same expression as the kernel's for every pair (every pair whose heights
overlap is clipped, however far apart the boxes are); ``place`` also returns every ratio it compared with 1e-8, so that a test can
state how far its decisions are from the threshold.
"""
import os

import numpy as np

import box_faces as bf
import scan_restate as rs

F = np.float32
D = np.float64
TRIES, EASY_ABOVE = 100, 100
MAX_TRIES, MAX_EXISTING, MAX_ACCEPT = 128, 224, 32


# ---- the database -------------------------------------------------------------------------------------------------------------
def pack_database(objects):
    """the reference's list of dicts -> dict of boxes (D,7), alpha (D), npts (D), offsets (D+1), points (S,4), easy, hard"""
    boxes = np.stack([np.asarray(o["gt_box3d"], F).reshape(7) for o in objects])
    alpha = np.array([o["obj"].alpha if "obj" in o else o["alpha"] for o in objects], F)
    rows = [np.concatenate([np.asarray(o["points"], F).reshape(-1, 3), np.asarray(o["intensity"], F).reshape(-1, 1)], axis=1) for o in objects]
    npts = np.array([len(r) for r in rows], np.int32)
    offsets = np.concatenate([[0], np.cumsum(npts)]).astype(np.int32)
    return {"boxes": boxes, "alpha": alpha, "npts": npts, "offsets": offsets, "points": np.concatenate(rows, axis=0),
            "easy": np.nonzero(npts > EASY_ABOVE)[0].astype(np.int32), "hard": np.nonzero(npts <= EASY_ABOVE)[0].astype(np.int32)}


def synthetic_objects(count, seed, low=3, high=300, cone=False):
    """`count` car-sized objects at random places in (and a few outside) the scope, `low`..`high` points each, in the pickle's form;
    cone: most of them inside the camera's field of view (|x| < 0.3 z), where scan_restate.scene_with puts its valid points"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        x, z = rng.uniform(-44, 44), rng.uniform(-3, 74)
        if cone and k % 7 != 3:
            x = x / 44 * 0.3 * max(z, 5.0)
        box = np.array([x, rng.uniform(1.2, 2.0), z, rng.uniform(1.3, 1.9), rng.uniform(1.4, 1.9), rng.uniform(3.2, 4.6), rng.uniform(-np.pi, np.pi)], F)
        n = low + (k // 9) % 2 if k % 9 == 4 else int(rng.integers(low, high + 1))    # every ninth object: `low` points or one more
        local = np.stack([rng.uniform(-0.5, 0.5, n) * box[5], rng.uniform(0, 1, n) * box[3], rng.uniform(-0.5, 0.5, n) * box[4]], axis=1)
        c, s = np.cos(float(box[6])), np.sin(float(box[6]))
        pts = np.stack([box[0] + local[:, 0] * c + local[:, 2] * s, box[1] - local[:, 1], box[2] - local[:, 0] * s + local[:, 2] * c], axis=1)
        out.append({"gt_box3d": box, "points": pts.astype(F), "intensity": rng.uniform(0, 1, n).astype(F), "alpha": F(rng.uniform(-np.pi, np.pi))})
    return out


# ---- geometry -----------------------------------------------------------------------------------------------------------------
def make_rect(box):
    """box (7) float32 [x, y, z, h, w, l, ry] -> (x (4), z (4), y0, y1, area, solid): float64 from the float32 values"""
    box = np.asarray(box, F)
    x, y, z, h, w, l, ry = (D(v) for v in box)
    c, s, hl, hw = np.cos(ry), np.sin(ry), l / 2.0, w / 2.0
    dx, dz = np.array([hl, hl, -hl, -hl]), np.array([hw, -hw, -hw, hw])
    return ((x + dx * c) + dz * s, (z - dx * s) + dz * c, y - h, y, abs(w * l), bool(box[4] != 0 and box[5] != 0))


def clip_area(a, b):
    """area of the intersection of two rectangles: `a` clipped by the four half-planes of `b`, shoelace sum"""
    px, pz = list(a[0]), list(a[1])
    bx, bz = b[0], b[1]
    twice = 0.0
    for k in range(4):
        twice += bx[k] * bz[(k + 1) & 3] - bx[(k + 1) & 3] * bz[k]
    sign = 1.0 if twice >= 0.0 else -1.0
    for e in range(4):
        ax, az, ex, ez = bx[e], bz[e], bx[(e + 1) & 3] - bx[e], bz[(e + 1) & 3] - bz[e]
        qx, qz, n = [], [], len(px)
        for i in range(n):
            j = i + 1 if i + 1 < n else 0
            d0 = sign * (ex * (pz[i] - az) - ez * (px[i] - ax))
            d1 = sign * (ex * (pz[j] - az) - ez * (px[j] - ax))
            if d0 >= 0.0:
                qx.append(px[i]); qz.append(pz[i])
            if (d0 >= 0.0) != (d1 >= 0.0):
                t = d0 / (d0 - d1)
                qx.append(px[i] + t * (px[j] - px[i])); qz.append(pz[i] + t * (pz[j] - pz[i]))
        px, pz = qx[:8], qz[:8]
    total, n = 0.0, len(px)
    for i in range(n):
        j = i + 1 if i + 1 < n else 0
        total += px[i] * pz[j] - px[j] * pz[i]
    return abs(total / 2.0)


def overlap_ratio(cand, cur):
    """-> (shared height, overlap3d / union3d or None when the heights share nothing)"""
    h_overlap = min(cand[3], cur[3]) - max(cand[2], cur[2])
    if not h_overlap > 0.0:
        return h_overlap, None
    bottom = clip_area(cand, cur) if (cand[5] and cur[5]) else 0.0        # always clipped, as the kernel does: the same expression
    overlap3d = bottom * h_overlap
    union3d = (cand[4] * (cand[3] - cand[2]) + cur[4] * (cur[3] - cur[2])) - overlap3d
    with np.errstate(all="ignore"):
        return h_overlap, D(overlap3d) / D(union3d)


def enlarged(box):
    out = np.asarray(box, F).copy()
    out[4] += F(0.5); out[5] += F(0.5)
    return out


def in_scope(centre, scope):
    sc = np.asarray(scope, D).reshape(3, 2)
    return all(sc[j, 0] <= D(centre[j]) <= sc[j, 1] for j in range(3))


# ---- placement ----------------------------------------------------------------------------------------------------------------
def place(db, apply, extra_num, cand, all_boxes, gt_boxes, gt_alpha, plane, e, k_max=MAX_ACCEPT, g=None, reduce_by_range=True,
          scope=rs.SCOPE):
    """one scene. all_boxes (A,7), gt_boxes (G,7), gt_alpha (G): the live rows only; g: the capacity of the label rows in the
    outputs (default G). -> dict of the kernel's outputs for the scene, plus "ratios" (every ratio compared with 1e-8),
    "heights" (every shared height, also the negative ones = gaps) and "trace" (try, database row, outcome)"""
    all_boxes, gt_boxes, gt_alpha = np.asarray(all_boxes, F).reshape(-1, 7), np.asarray(gt_boxes, F).reshape(-1, 7), np.asarray(gt_alpha, F).reshape(-1)
    g = len(gt_boxes) if g is None else g
    pa, pb, pc, pd = (D(v) for v in np.asarray(plane, D))
    out = {"acc_db": np.full(k_max, -1, np.int32), "acc_box": np.zeros((k_max, 7), F), "acc_move": np.zeros(k_max, D),
           "acc_row0": np.zeros(k_max, np.int32), "remove_boxes": np.zeros((k_max, 7), F), "gt_out": np.zeros((g + k_max, 7), F),
           "alpha_out": np.zeros(g + k_max, F), "ratios": [], "heights": [], "trace": []}
    ng = len(gt_boxes)
    out["gt_out"][:ng], out["alpha_out"][:ng] = gt_boxes, gt_alpha
    tries = cnt = acc = rej_overlap = rej_capacity = rows = 0
    if apply:
        current = [make_rect(enlarged(bx)) for bx in all_boxes]
        extra = min(int(extra_num), k_max - 1)
        for t in range(len(cand)):
            if cnt > extra:
                break
            tries += 1
            d = int(cand[t])
            if d < 0 or d >= len(db["boxes"]):
                out["trace"].append((t, d, "no object")); continue
            box = db["boxes"][d].copy()
            if reduce_by_range and not in_scope(box[:3], scope):
                out["trace"].append((t, d, "range")); continue
            npts = int(db["npts"][d])
            if npts < 5:
                out["trace"].append((t, d, "few")); continue
            with np.errstate(all="ignore"):
                cur_height = ((-pd - pa * D(box[0])) - pc * D(box[2])) / pb
                move = D(box[1]) - cur_height
                box[1] = F(D(box[1]) - move)
            cnt += 1
            mine = make_rect(enlarged(box))
            hit = False
            for cur in current:
                h_overlap, ratio = overlap_ratio(mine, cur)
                out["heights"].append(h_overlap)
                if ratio is not None:
                    out["ratios"].append(ratio)
                    hit = hit or bool(ratio >= 1e-8)
            if hit:
                rej_overlap += 1
                out["trace"].append((t, d, "overlap")); continue
            if acc >= k_max or npts > e - rows:
                rej_capacity += 1
                out["trace"].append((t, d, "capacity")); continue
            current.append(mine)
            out["acc_db"][acc], out["acc_box"][acc], out["acc_move"][acc], out["acc_row0"][acc] = d, box, move, rows
            out["remove_boxes"][acc] = box
            out["remove_boxes"][acc, 3] += F(2.0)
            out["gt_out"][ng + acc], out["alpha_out"][ng + acc] = box, db["alpha"][d]
            out["trace"].append((t, d, "accept"))
            acc += 1
            rows += npts
    out["info"] = np.array([1 if apply else 0, int(extra_num), tries, cnt, acc, rej_overlap, rej_capacity, rows], np.int32)
    return out


def object_points(db, placed, e):
    """-> extra_pts (e,4): the accepted objects' rows one behind the other, lowered by their moves; zeros behind"""
    out = np.zeros((e, 4), F)
    for k in range(int(placed["info"][4])):
        d, row0 = int(placed["acc_db"][k]), int(placed["acc_row0"][k])
        rows = db["points"][db["offsets"][d]:db["offsets"][d + 1]].copy()
        rows[:, 1] = (rows[:, 1].astype(D) - placed["acc_move"][k]).astype(F)
        out[row0:row0 + len(rows)] = rows
    return out


# ---- the sampling ---------------------------------------------------------------------------------------------------------------
def pts_in_box(rect, box):
    """pt_in_box3d as epnet_roipool3d evaluates it: rect (P,3) float32, box (7) float32 -> (P) bool (box_faces.membership32, the
    one statement of the predicate)"""
    return bf.membership32(rect, box)[0]


def project(xyz, P2):
    """rectified (E,3) float32 -> (E,2) float32 pixel, the contract's order"""
    P2 = np.asarray(P2, F).reshape(3, 4)
    X, Y, Z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all="ignore"):
        pr = [((X * P2[r, 0] + Y * P2[r, 1]) + Z * P2[r, 2]) + P2[r, 3] for r in range(2)]
        return np.stack([pr[0] / Z, pr[1] / Z], axis=1).astype(F)


def prepare_aug(pts, num_raw, V2C, R0, P2, img_shape, extra_pts, num_extra, remove_boxes, num_remove, keys, slot_perm, n,
                reduce_by_range=True, scope=rs.SCOPE, near_depth=rs.NEAR):
    """one scene -> scan_restate.prepare's dict over [0, p) raw rows then [p, p + e) extra rows; scene_info has 8 entries"""
    pts, extra_pts = np.asarray(pts, F).reshape(-1, 4), np.asarray(extra_pts, F).reshape(-1, 4)
    p, e = len(pts), len(extra_pts)
    num_extra, num_remove = min(max(int(num_extra), 0), e), min(max(int(num_remove), 0), len(remove_boxes))
    rect, uv, valid, near = rs.classify(pts, num_raw, V2C, R0, P2, img_shape, reduce_by_range, scope, near_depth)
    inside = np.zeros(p, bool)
    for k in range(num_remove):
        inside |= pts_in_box(rect, remove_boxes[k])
    removed = int((valid & inside).sum())
    live = np.arange(e) < num_extra
    valid_all = np.concatenate([valid & ~inside, live])
    near_all = np.concatenate([near & ~inside, live & (extra_pts[:, 2] < F(near_depth))])
    rect_all = np.concatenate([rect, extra_pts[:, :3]])
    uv_all = np.concatenate([uv, project(extra_pts[:, :3], P2)])
    inten_all = np.concatenate([pts[:, 3], extra_pts[:, 3]]) - F(0.5)
    L, (V, Fc, case, r, q) = rs.select(valid_all, near_all, keys, n)
    out = {"pts_rect": np.zeros((n, 3), F), "pts_intensity": np.zeros(n, F), "pts_origin_xy": np.zeros((n, 2), F),
           "choice": np.full(n, -1, np.int32),
           "scene_info": np.array([min(max(int(num_raw), 0), p), V, Fc, case, r, q, removed, num_extra], np.int32)}
    if L is not None:
        slot = np.arange(n) if slot_perm is None else np.asarray(slot_perm, np.int64)
        out["pts_rect"][slot], out["pts_intensity"][slot], out["pts_origin_xy"][slot], out["choice"][slot] = rect_all[L], inten_all[L], uv_all[L], L
    out["pts_input"] = np.concatenate([out["pts_rect"], out["pts_intensity"][:, None]], axis=1)
    out["kept_raw"] = np.nonzero(valid & ~inside)[0]
    return out


PLACE_KEYS = ("acc_db", "acc_box", "acc_move", "acc_row0", "remove_boxes", "gt_out", "alpha_out", "info")


def whole(db, scene, tables, n, e, k_max=MAX_ACCEPT, g=None, **kw):
    """placement + points + sampling of one scene: scene = dict of pts, num_raw, V2C, R0, P2, img_shape, all_boxes, gt_boxes,
    gt_alpha, plane; tables = dict of apply, extra_num, cand, keys, slot_perm (this scene's rows)"""
    placed = place(db, tables["apply"], tables["extra_num"], tables["cand"], scene["all_boxes"], scene["gt_boxes"], scene["gt_alpha"],
                   scene["plane"], e, k_max, g, **kw)
    extra = object_points(db, placed, e)
    out = prepare_aug(scene["pts"], scene["num_raw"], scene["V2C"], scene["R0"], scene["P2"], scene["img_shape"], extra, placed["info"][7],
                      placed["remove_boxes"], placed["info"][4], tables["keys"], tables.get("slot_perm"), n, **kw)
    out.update({k: placed[k] for k in PLACE_KEYS})
    out["extra_pts"], out["ratios"], out["heights"], out["trace"] = extra, placed["ratios"], placed["heights"], placed["trace"]
    return out


def decisions_are_clear(ratios, heights):
    """no compared ratio in (0, 1e-5) and no shared height or gap below 1e-3: the decisions do not hang on the last bits"""
    return all(r == 0.0 or r >= 1e-5 for r in ratios) and all(abs(h) >= 1e-3 for h in heights)


def fixture():
    """tests/golden/gt_aug.npz -> (database objects, list of scene dicts with the reference's results)"""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gt_aug.npz"))
    objects = [{"gt_box3d": z["db_boxes"][k], "points": z["db_points"][z["db_offsets"][k]:z["db_offsets"][k + 1], :3],
                "intensity": z["db_points"][z["db_offsets"][k]:z["db_offsets"][k + 1], 3], "alpha": z["db_alpha"][k]}
               for k in range(len(z["db_boxes"]))]
    scenes = []
    for i in range(int(z["scenes"])):
        pre = "s%d__" % i
        scenes.append({k[len(pre):]: z[k] for k in z.files if k.startswith(pre)})
    return objects, scenes

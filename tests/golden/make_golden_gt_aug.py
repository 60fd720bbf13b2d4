"""Regenerates tests/golden/gt_aug.npz. Runs ONLY where the reference checkout is available; the fixture is plain data.

What runs is the REFERENCE'S OWN Python, imported unmodified through make_golden_rcnn.import_reference():
``KittiRCNNDataset.apply_gt_aug_to_one_scene`` (lib/datasets/kitti_rcnn_dataset.py:590-696) with ``kitti_utils.boxes3d_to_corners3d``
and ``get_iou3d`` and ``roipool3d_utils.pts_in_boxes3d_cpu`` (over the reference's own host op, compiled by oracle/build_ref.py),
called on ``object.__new__(KittiRCNNDataset)`` so that no dataset is needed on disk: ``gt_database`` is the [easy, hard] pair of
lists of :96-104 and ``get_road_plane`` an instance-level stand-in.

shapely is not installed here, and get_iou3d imports ``shapely.geometry.Polygon`` when it runs. A stand-in module of that name is
put into sys.modules: ``area`` is the shoelace sum, ``is_valid`` a non-zero area, ``intersection`` the float64 clip of one
polygon by the half-planes of the other (as tests/exact_geometry.py clips) -- the exact geometry shapely computes, on the float32
corners the reference hands over.

Randomness. While the reference method runs, ``np.random.rand`` and ``np.random.randint`` are served from the scene's tables:
``rand()`` returns p of the try, ``randint(0, len)`` returns floor(u * len) of the try, ``randint(10, GT_EXTRA_NUM)`` the scene's
extra_num. The reference code itself is untouched. Database objects are fresh copies per scene (the reference lowers obj.pos in
place, :656). The point features carry the row number in a spare column, so the rows the reference kept are read back from its
own result.

Conditions, asserted here: no compared box pair has a ratio in (0, 1e-5) -- by the restatement's float64 ratio and by the
reference's own iou3d -- or a vertical gap or overlap below 1e-3 m; every scan point within 1e-3 m of a face of a removal box or
of the 10 m gate (judged in float64) is removed from the scan before the reference runs, and the scan that runs is asserted to
hold none; no capacity rejection. The new rows of the reference's result are counted from the objects it says it accepted. Together the
scenes cover easy and hard picks, out-of-range and under-5-point candidates, overlap rejections against existing and against
accepted boxes, cnt ending the loop, the tries running out, apply = 0 and nothing accepted. Stored: inputs, tables and the
reference's outputs only.
"""
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import gt_aug_restate as gr  # noqa: E402
import scan_restate as rs  # noqa: E402
from make_golden_rcnn import import_reference  # noqa: E402

F = np.float32
T, E, P, D_OBJECTS = 100, 4096, 3000, 40
EYE_V2C = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(F)
EYE_R0 = np.eye(3, dtype=F)


# ---- the stand-in of shapely.geometry.Polygon -------------------------------------------------------------------------------------
def _shoelace(p):
    return 0.5 * float(np.sum(p[:, 0] * np.roll(p[:, 1], -1) - np.roll(p[:, 0], -1) * p[:, 1])) if len(p) >= 3 else 0.0


class Polygon:
    def __init__(self, points):
        self.p = np.asarray(points, np.float64).reshape(-1, 2)

    @property
    def area(self):
        return abs(_shoelace(self.p))

    @property
    def is_valid(self):
        return self.area > 0.0

    def intersection(self, other):
        sign = 1.0 if _shoelace(other.p) >= 0 else -1.0
        pts = [tuple(v) for v in self.p]
        m = len(other.p)
        for e in range(m):
            a, b = other.p[e], other.p[(e + 1) % m]
            ex, ey = b[0] - a[0], b[1] - a[1]
            out = []
            for i in range(len(pts)):
                p0, p1 = pts[i], pts[(i + 1) % len(pts)]
                d0 = sign * (ex * (p0[1] - a[1]) - ey * (p0[0] - a[0]))
                d1 = sign * (ex * (p1[1] - a[1]) - ey * (p1[0] - a[0]))
                if d0 >= 0:
                    out.append(p0)
                if (d0 >= 0) != (d1 >= 0):
                    t = d0 / (d0 - d1)
                    out.append((p0[0] + t * (p1[0] - p0[0]), p0[1] + t * (p1[1] - p0[1])))
            pts = out
        return Polygon(np.array(pts).reshape(-1, 2))


def install_shapely():
    if "shapely.geometry" in sys.modules:
        return
    top, geo = types.ModuleType("shapely"), types.ModuleType("shapely.geometry")
    geo.Polygon = Polygon
    top.geometry = geo
    sys.modules["shapely"], sys.modules["shapely.geometry"] = top, geo


# ---- the draws --------------------------------------------------------------------------------------------------------------------
class Draws:
    """np.random.rand and np.random.randint from the scene's tables while apply_gt_aug_to_one_scene runs"""

    def __init__(self, p, u, extra_num):
        self.p, self.u, self.extra_num, self.t, self.saved = p, u, extra_num, -1, None

    def rand(self, *shape):
        assert not shape
        self.t += 1
        return float(self.p[self.t])

    def randint(self, low, high=None, *a, **kw):
        if low == 10:
            return int(self.extra_num)
        assert low == 0
        return min(int(np.floor(float(self.u[self.t]) * high)), high - 1)

    def __enter__(self):
        self.saved = (np.random.rand, np.random.randint)
        np.random.rand, np.random.randint = self.rand, self.randint
        return self

    def __exit__(self, *exc):
        np.random.rand, np.random.randint = self.saved
        return False


class Obj:
    def __init__(self, box, alpha, npts):
        self.pos, self.alpha, self.npts = np.array(box[:3], F), float(alpha), int(npts)


def tables_for(rows, db, ratio, rng):
    """(p, u) that make the reference pick database row rows[t] at try t: p on the row's side of the ratio, u in the middle of
    the row's cell of its list"""
    p, u = np.zeros(len(rows), F), np.zeros(len(rows), F)
    for t, d in enumerate(rows):
        easy = d in db["easy"]
        lst = db["easy"] if easy else db["hard"]
        p[t] = rng.uniform(ratio + 0.01, 1.0) if easy else rng.uniform(0.0, ratio - 0.01)
        u[t] = (list(lst).index(d) + 0.5) / len(lst)
    return p, u


def cand_of(p, u, db, ratio):
    """draw_gt_aug_tables' rule in numpy"""
    pick = lambda lst: lst[np.minimum(np.floor(u * F(len(lst))).astype(np.int64), len(lst) - 1)]  # noqa: E731
    return np.where(p > F(ratio), pick(db["easy"]), pick(db["hard"])).astype(np.int32)


def near_a_face(pts, box, tol=1e-3):
    """scan points within tol of a face of the box or of the 10 m gate, in float64"""
    b = np.asarray(box, np.float64)
    x, y, z = (pts[:, j].astype(np.float64) for j in range(3))
    c, s = np.cos(b[6]), np.sin(b[6])
    xr, zr = (x - b[0]) * c - (z - b[2]) * s, (x - b[0]) * s + (z - b[2]) * c
    close = lambda v, at: np.abs(np.abs(v) - at) < tol  # noqa: E731
    return close(xr, b[5] / 2) | close(zr, b[4] / 2) | close(y - (b[1] - b[3] / 2), b[3] / 2) | close(x - b[0], 10.0) | close(z - b[2], 10.0)


def scene_points(rng, boxes, plane):
    """ground points over the scope and points in and around the given boxes, float32, in the rectified frame; intensity in column 3"""
    a, b, c, d = plane
    x, z = rng.uniform(-40, 40, P), rng.uniform(0.5, 70, P)
    y = (-d - a * x - c * z) / b - np.abs(rng.normal(0, 0.05, P))
    k = np.arange(P) % 3 == 0
    if len(boxes):
        pick = boxes[rng.integers(0, len(boxes), P)]
        x = np.where(k, pick[:, 0] + rng.uniform(-3, 3, P), x)
        z = np.where(k, pick[:, 2] + rng.uniform(-3, 3, P), z)
        y = np.where(k, pick[:, 1] - rng.uniform(-0.5, 4.0, P), y)
    return np.stack([x, y, z, rng.uniform(0, 1, P)], axis=1).astype(F)


def main():
    cfg = import_reference()[0]
    install_shapely()
    from oracle import build_ref
    sys.modules["roipool3d_cuda"].pts_in_boxes3d_cpu = build_ref.load().pts_in_boxes3d_cpu   # the reference's own host op, compiled
    from lib.datasets.kitti_rcnn_dataset import KittiRCNNDataset
    assert cfg.PC_REDUCE_BY_RANGE and np.array_equal(np.asarray(cfg.PC_AREA_SCOPE, np.float64), rs.SCOPE)
    ratio = float(cfg.GT_AUG_HARD_RATIO)
    assert ratio == 0.6 and cfg.GT_EXTRA_NUM == 15
    objects = gr.synthetic_objects(D_OBJECTS, seed=4100)
    db = gr.pack_database(objects)
    in_range = np.array([gr.in_scope(bx[:3], rs.SCOPE) for bx in db["boxes"]])
    good = np.nonzero(in_range & (db["npts"] >= 5))[0]
    bad = np.nonzero(~in_range | (db["npts"] < 5))[0]
    assert len(db["easy"]) >= 5 and len(db["hard"]) >= 5 and (~in_range).sum() >= 2 and (db["npts"] < 5).sum() >= 2 and len(good) >= 16
    P2, shape = rs.calib(0)[2:]
    out = {"scenes": np.int64(0), "db_boxes": db["boxes"], "db_alpha": db["alpha"], "db_offsets": db["offsets"], "db_points": db["points"],
           "V2C": EYE_V2C, "R0": EYE_R0, "P2": P2, "img_shape": shape, "T": np.int64(T), "E": np.int64(E)}
    # (kind, apply, extra_num, GT_AUG_RAND_NUM, existing boxes)
    kinds = [("cnt ends the loop", 1, 15, False, 12), ("the tries run out", 1, 15, False, 6), ("apply = 0", 0, 15, False, 5),
             ("nothing accepted", 1, 15, False, 8), ("ten extra, repeated objects", 1, 10, True, 1)]
    seen = set()
    for i, (kind, apply, extra_num, rand_num, existing) in enumerate(kinds):
        for attempt in range(200):
            rng = np.random.default_rng(4200 + 100 * i + attempt)
            plane = np.array([rng.uniform(-0.02, 0.02), -1.0, rng.uniform(-0.02, 0.02), rng.uniform(1.5, 1.8)], np.float64)
            plane /= np.linalg.norm(plane[:3])
            if kind == "the tries run out":
                rows = np.where(rng.uniform(size=T) < 0.93, rng.choice(bad, T), rng.choice(good, T))
            elif kind == "nothing accepted":
                rows = rng.choice(good[:existing], T)
            elif kind == "ten extra, repeated objects":
                rows = rng.choice(good[:14], T)
            else:
                rows = rng.choice(np.arange(D_OBJECTS), T)
            p_tab, u_tab = tables_for(rows, db, ratio, rng)
            cand = cand_of(p_tab, u_tab, db, ratio)
            assert np.array_equal(cand, rows)
            if kind == "nothing accepted":     # the existing boxes are the candidates themselves, on the road
                all_boxes = db["boxes"][good[:existing]].copy()
                all_boxes[:, 1] = [(-plane[3] - plane[0] * bx[0] - plane[2] * bx[2]) / plane[1] for bx in all_boxes]
            else:
                all_boxes = np.stack([o["gt_box3d"] for o in gr.synthetic_objects(existing, seed=4300 + 100 * i + attempt)]).reshape(-1, 7) \
                    if existing else np.zeros((0, 7), F)
                for bx in all_boxes:
                    bx[1] = F((-plane[3] - plane[0] * bx[0] - plane[2] * bx[2]) / plane[1] + rng.uniform(-0.1, 0.1))
            all_boxes = all_boxes.astype(F)
            num_gt = max(len(all_boxes) - 2, 0)           # the label rows: all but two of them (filtrate_objects drops some)
            gt_boxes, gt_alpha = all_boxes[:num_gt].copy(), rng.uniform(-3, 3, num_gt).astype(F)
            mine = gr.place(db, apply, extra_num, cand, all_boxes, gt_boxes, gt_alpha, plane, E)
            if gr.decisions_are_clear(mine["ratios"], mine["heights"]) and mine["info"][6] == 0:
                break
        else:
            raise AssertionError("no clear draw for scene %d" % i)
        pts = scene_points(rng, np.concatenate([all_boxes, mine["acc_box"][:mine["info"][4]]]), plane)
        unclear = np.zeros(len(pts), bool)
        for k in range(int(mine["info"][4])):
            unclear |= near_a_face(pts, mine["remove_boxes"][k])
        pts = pts[~unclear]
        assert not any(near_a_face(pts, mine["remove_boxes"][k]).any() for k in range(int(mine["info"][4])))     # the stated condition
        p = len(pts)

        ds = object.__new__(KittiRCNNDataset)
        fresh = [{"gt_box3d": o["gt_box3d"].copy(), "points": o["points"].copy(), "intensity": o["intensity"].copy(),
                  "rgb": np.zeros((len(o["points"]), 3), F), "obj": Obj(o["gt_box3d"], o["alpha"], len(o["points"]))} for o in objects]
        ds.gt_database = [[fresh[k] for k in db["easy"]], [fresh[k] for k in db["hard"]]]
        ds.get_road_plane = lambda sample_id: plane.copy()
        features = np.zeros((p, 4), np.float64)
        features[:, 0], features[:, 1] = pts[:, 3], np.arange(p)
        pre = "s%d__" % i
        cfg.GT_AUG_RAND_NUM = rand_num
        iou_seen = []
        import lib.utils.kitti_utils as ku
        real_iou = ku.get_iou3d

        def spy(*args, **kw):
            res = real_iou(*args, **kw)
            iou_seen.append(np.array(res, np.float64).reshape(-1))
            return res
        if apply:
            ku.get_iou3d = spy
            try:
                with Draws(p_tab, u_tab, extra_num) as draws:
                    flag, ref_pts, ref_feat, ref_boxes, ref_objs = ds.apply_gt_aug_to_one_scene(0, pts[:, :3].copy(), features, all_boxes.copy())
            finally:
                ku.get_iou3d = real_iou
                cfg.GT_AUG_RAND_NUM = False
            tries_used = draws.t + 1
            ref_ratios = np.concatenate(iou_seen) if iou_seen else np.zeros(0)
            assert not ((ref_ratios > 0) & (ref_ratios < 1e-5)).any()
        else:
            flag, tries_used = False, 0
        if not flag:
            ref_pts, ref_feat, ref_boxes, ref_alpha = pts[:, :3], features, np.zeros((0, 7), F), np.zeros(0, F)
        else:
            ref_alpha = np.array([o.alpha for o in ref_objs], F)
        # the new rows are the tail of what the reference returned: as many as the objects it says it accepted hold
        n_new = sum(o.npts for o in ref_objs) if flag else 0
        assert n_new == int(mine["info"][7])
        kept = np.asarray(ref_feat[:len(ref_feat) - n_new, 1], np.int64)
        assert np.array_equal(pts[kept, :3], ref_pts[:len(kept)]) and (np.diff(kept) > 0).all()
        accepted = int(mine["info"][4])
        assert len(ref_boxes) == accepted and int(mine["info"][2]) == tries_used, (i, len(ref_boxes), accepted, tries_used, mine["info"])
        outcomes = [tr[2] for tr in mine["trace"]]
        seen |= set(outcomes) | {kind}
        if accepted:
            seen |= {"easy" if d in db["easy"] else "hard" for d in mine["acc_db"][:accepted]}
            first_accept = outcomes.index("accept")
            if "overlap" in outcomes[:first_accept] or kind == "nothing accepted":
                seen.add("overlap with an existing box")
        if kind == "nothing accepted":
            assert accepted == 0 and "overlap" in outcomes
            seen.add("overlap with an existing box")
        if kind == "ten extra, repeated objects":
            accepted_before = [set(tr[1] for tr in mine["trace"][:j] if tr[2] == "accept") for j in range(len(outcomes))]
            assert "overlap" in outcomes and all(tr[1] in accepted_before[j] for j, tr in enumerate(mine["trace"]) if tr[2] == "overlap")
            seen.add("overlap with an accepted box")
        if kind == "cnt ends the loop":
            assert tries_used < T and mine["info"][3] == extra_num + 1
        if kind == "the tries run out":
            assert tries_used == T and mine["info"][3] <= extra_num
        for key, value in (("pts", pts), ("all_boxes", all_boxes), ("gt_boxes", gt_boxes), ("gt_alpha", gt_alpha), ("plane", plane),
                           ("apply", np.int32(apply)), ("extra_num", np.int32(extra_num)), ("p_table", p_tab), ("u_table", u_tab),
                           ("cand", cand), ("ref_flag", np.bool_(flag)), ("ref_tries", np.int64(tries_used)),
                           ("ref_extra_boxes", np.asarray(ref_boxes, F).reshape(-1, 7)), ("ref_extra_alpha", ref_alpha),
                           ("ref_new_pts", np.asarray(ref_pts[len(kept):], F)), ("ref_new_intensity", np.asarray(ref_feat[len(kept):, 0], F)),
                           ("ref_kept_rows", kept.astype(np.int32))):
            out[pre + key] = value
        out["scenes"] = np.int64(i + 1)
        print("scene %d (%s): p %d, tries %d, cnt %d, accepted %d, overlap %d, new points %d, removed %d; boxes bit-equal to the restatement: %s" % (
            i, kind, p, tries_used, mine["info"][3], accepted, mine["info"][5], n_new, p - len(kept),
            np.asarray(ref_boxes, F).reshape(-1, 7).tobytes() == mine["acc_box"][:accepted].tobytes()))
    want = {"easy", "hard", "range", "few", "overlap with an existing box", "overlap with an accepted box"} | {k[0] for k in kinds}
    assert want <= seen, want - seen
    path = os.path.join(HERE, "gt_aug.npz")
    np.savez_compressed(path, **out)
    print("wrote gt_aug.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

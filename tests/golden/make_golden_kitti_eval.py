"""Regenerates tests/golden/kitti_eval.npz. Runs ONLY in the build container (needs /root/reference); the fixture is plain data.

What runs is the REFERENCE'S OWN Python, imported unmodified from /root/reference: tools/kitti_object_eval_python/eval.py and
rotate_iou.py. numba is not installed, so a stand-in is put into sys.modules first: numba.jit and numba.cuda.jit are identity
decorators in both call forms, numba.float32 is np.float32, cuda.local.array(shape, dtype) is np.zeros(shape, np.float32), and
eval.rotate_iou_gpu_eval is a loop that casts to float32 and calls the reference's devRotateIoUEval(qbox, box, criterion) per
pair, in the argument order of rotate_iou_kernel_eval (rotate_iou.py:293). Under the interpreter the float32 device functions
accumulate a little differently from numba's typing, so the rotated values carry a 1e-5 bar, not bit equality.

Stored: the annos of two data sets as arrays, per-frame overlap blocks of the three metrics, clean_data's tables for class Car,
per (metric, difficulty, overlap row) the thresholds and the pr table, precision / recall / aos, the mAP arrays, the result
strings and ret_dicts. Condition, asserted here per frame (a frame is redrawn until it holds) and again by the test from the stored
overlaps: no overlap lies within 1e-4 of 0.7 / 0.5 / 0.25. A frame on which the reference's rotated intersection finds a ninth
polygon point (its arrays hold eight; under the interpreter that is an IndexError) is redrawn too; the count is stored.
"""
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))

REF = "/root/reference"
MARGIN = 1e-4
LEVELS = (0.7, 0.5, 0.25)
NAMES = ["Car", "Van", "Pedestrian", "Person_sitting", "Cyclist", "DontCare"]
FIELDS = ("truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y", "score")


def install_numba():
    def jit(*args, **kw):
        if len(args) == 1 and callable(args[0]) and not kw:
            return args[0]
        return lambda fn: fn

    numba = types.ModuleType("numba")
    cuda = types.ModuleType("numba.cuda")
    numba.jit = jit
    numba.float32 = np.float32
    numba.cuda = cuda
    cuda.jit = jit
    cuda.local = types.SimpleNamespace(array=lambda shape, dtype=None: np.zeros(shape, np.float32))
    cuda.shared = types.SimpleNamespace(array=lambda shape, dtype=None: np.zeros(shape, np.float32))
    sys.modules["numba"] = numba
    sys.modules["numba.cuda"] = cuda


def load_reference():
    install_numba()
    sys.path.insert(0, REF)
    import tools.kitti_object_eval_python.rotate_iou as rotate_iou
    import tools.kitti_object_eval_python.eval as ev

    def rotate_iou_gpu_eval(boxes, query_boxes, criterion=-1, device_id=0):
        boxes, query_boxes = boxes.astype(np.float32), query_boxes.astype(np.float32)
        iou = np.zeros((boxes.shape[0], query_boxes.shape[0]), np.float32)
        with np.errstate(all="ignore"):
            for n in range(boxes.shape[0]):
                for k in range(query_boxes.shape[0]):
                    iou[n, k] = rotate_iou.devRotateIoUEval(query_boxes[k], boxes[n], criterion)
        return iou

    ev.rotate_iou_gpu_eval = rotate_iou_gpu_eval
    return ev


# ---- the data sets ------------------------------------------------------------------------------------------------------------
DIMS = {"Car": (3.9, 1.5, 1.6), "Van": (5.0, 2.2, 1.9), "Pedestrian": (0.8, 1.8, 0.6), "Person_sitting": (0.8, 1.3, 0.6),
        "Cyclist": (1.8, 1.7, 0.6), "DontCare": (-1.0, -1.0, -1.0)}
RY_SPECIAL = [0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi, np.pi - 1e-3, -np.pi + 1e-3]
HEIGHTS = [20.0, 24.5, 25.5, 32.0, 39.5, 40.5, 60.0, 110.0]
TRUNCS = [0.0, 0.1, 0.14, 0.16, 0.29, 0.31, 0.49, 0.51]


def empty_anno(with_score):
    a = dict(name=[], truncated=[], occluded=[], alpha=[], bbox=[], dimensions=[], location=[], rotation_y=[])
    if with_score:
        a["score"] = []
    return a


def finish(a):
    out = {"name": np.array(a["name"], dtype="<U16")}
    out["truncated"] = np.array(a["truncated"], np.float64)
    out["occluded"] = np.array(a["occluded"], np.int64)
    out["alpha"] = np.array(a["alpha"], np.float64)
    out["bbox"] = np.array(a["bbox"], np.float64).reshape(-1, 4)
    out["dimensions"] = np.array(a["dimensions"], np.float64).reshape(-1, 3)
    out["location"] = np.array(a["location"], np.float64).reshape(-1, 3)
    out["rotation_y"] = np.array(a["rotation_y"], np.float64).reshape(-1)
    out["score"] = np.array(a.get("score", [0.0] * len(a["name"])), np.float64)
    return out


def add(a, name, trunc, occ, alpha, bbox, dims, loc, ry, score=None):
    a["name"].append(name)
    a["truncated"].append(trunc)
    a["occluded"].append(occ)
    a["alpha"].append(alpha)
    a["bbox"].append(list(bbox))
    a["dimensions"].append(list(dims))
    a["location"].append(list(loc))
    a["rotation_y"].append(ry)
    if score is not None:
        a["score"].append(score)


def r3(x):
    """three decimals, as a label file has them: keeps the fixture small and the values exactly representable in print"""
    return float(np.round(x, 3))


def draw_frame(rng, kind, names=NAMES):
    """kind: 'plain' | 'no_gt' | 'no_dt' | 'neither' | 'pairs' | 'ties'"""
    gt, dt = empty_anno(False), empty_anno(True)
    n_gt = 0 if kind in ("no_gt", "neither") else int(rng.integers(1 if kind in ("pairs", "ties") else 0, 9))
    for _ in range(n_gt):
        name = names[int(rng.integers(len(names)))]
        l, h, w = (r3(v * rng.uniform(0.85, 1.15)) if v > 0 else v for v in DIMS[name])
        loc = (r3(rng.uniform(-20, 20)), r3(rng.uniform(1.2, 2.0)), r3(rng.uniform(5, 60)))
        ry = float(RY_SPECIAL[int(rng.integers(len(RY_SPECIAL)))]) if rng.uniform() < 0.35 else r3(rng.uniform(-np.pi, np.pi))
        left, top = r3(rng.uniform(0, 1000)), r3(rng.uniform(100, 250))
        height = HEIGHTS[int(rng.integers(len(HEIGHTS)))]
        width = r3(height * rng.uniform(0.8, 2.2))
        occ = int(rng.choice([0, 0, 1, 2, 3])) if name != "DontCare" else -1
        trunc = TRUNCS[int(rng.integers(len(TRUNCS)))] if name != "DontCare" else -1.0
        alpha = r3(rng.uniform(-np.pi, np.pi)) if name != "DontCare" else -10.0
        if name == "DontCare":
            loc, ry = (-1000.0, -1000.0, -1000.0), -10.0
            width, height = r3(rng.uniform(40, 200)), r3(rng.uniform(30, 80))
        add(gt, name, trunc, occ, alpha, (left, top, r3(left + width), r3(top + height)), (l, h, w), loc, ry)
    if kind in ("no_dt", "neither"):
        return finish(gt), finish(dt)
    g = finish(gt)
    for i in range(n_gt):
        name = str(g["name"][i])
        box, dims, loc, ry = g["bbox"][i], g["dimensions"][i], g["location"][i], float(g["rotation_y"][i])
        if name == "DontCare":
            for _ in range(int(rng.integers(0, 3))):   # detections over a DontCare region: inside it, partly inside it
                wd, hd = (box[2] - box[0]) * rng.uniform(0.3, 0.9), max((box[3] - box[1]) * rng.uniform(0.5, 0.95), 26.0)
                x0 = box[0] + (box[2] - box[0] - wd) * rng.uniform(-0.3, 1.0)
                y0 = box[1] + (box[3] - box[1] - hd) * rng.uniform(0, 1.0)
                add(dt, "Car", 0.0, 0, r3(rng.uniform(-3, 3)), (r3(x0), r3(y0), r3(x0 + wd), r3(y0 + hd)), (3.9, 1.5, 1.6),
                    (r3(rng.uniform(-20, 20)), 1.6, r3(rng.uniform(60, 70))), r3(rng.uniform(-3, 3)), r3(rng.uniform(0.05, 0.9)))
            continue
        if rng.uniform() > 0.85:
            continue
        copies = 2 if rng.uniform() < 0.2 else 1   # the second copy of one ground truth becomes a false positive
        for c in range(copies):
            mode = rng.choice(["jitter", "jitter", "jitter", "identical", "edge", "nested", "far"]) if kind == "pairs" else "jitter"
            s = 0.03 if rng.uniform() < 0.6 else 0.12
            jb = [r3(v + rng.normal(0, s * (box[3] - box[1]))) for v in box]
            jd = [r3(v * (1 + rng.normal(0, s))) for v in dims]
            jl = [r3(v + rng.normal(0, s * 2)) for v in loc]
            jr = r3(ry + rng.normal(0, s))
            if mode == "identical":
                jb, jd, jl, jr = list(box), list(dims), list(loc), ry
            elif mode == "edge":      # shares an edge with the ground truth: shifted by exactly its length along its own axis
                jd, jr = list(dims), ry
                jl = [float(loc[0] + dims[0] * np.cos(ry)), float(loc[1]), float(loc[2] - dims[0] * np.sin(ry))]
                jb = [float(box[2]), float(box[1]), float(2 * box[2] - box[0]), float(box[3])]
            elif mode == "nested":
                jd, jl, jr = [r3(dims[0] * 0.5), r3(dims[1] * 0.8), r3(dims[2] * 0.5)], list(loc), ry
                jb = [r3(box[0] + 2), r3(box[1] + 2), r3(box[2] - 2), r3(box[3] - 2)]
            elif mode == "far":
                jl = [r3(loc[0] + 30), float(loc[1]), r3(loc[2] + 30)]
                jb = [r3(box[0] + 400), float(box[1]), r3(box[2] + 400), float(box[3])]
            dname = name if rng.uniform() < 0.9 else names[int(rng.integers(len(names) - 1))]
            add(dt, dname, 0.0, 0, r3(float(g["alpha"][i]) + rng.normal(0, 0.2)), jb, jd, jl, jr, r3(rng.uniform(0.02, 0.99)))
    for _ in range(int(rng.integers(0, 4))):   # pure false positives
        name = names[int(rng.integers(len(names) - 1))]
        l, h, w = DIMS[name]
        left, top, height = r3(rng.uniform(0, 1000)), r3(rng.uniform(100, 250)), HEIGHTS[int(rng.integers(len(HEIGHTS)))]
        add(dt, name, 0.0, 0, r3(rng.uniform(-3, 3)), (left, top, r3(left + height * 1.5), r3(top + height)), (l, h, w),
            (r3(rng.uniform(-20, 20)), 1.6, r3(rng.uniform(5, 60))), r3(rng.uniform(-3, 3)), r3(rng.uniform(0.02, 0.6)))
    if kind == "ties" and len(dt["score"]) >= 2:
        for k in range(len(dt["score"])):   # deliberately equal scores in one frame: two values only
            dt["score"][k] = 0.5 if k % 3 else 0.75
    return finish(gt), finish(dt)


def frame_blocks(ev, g, d):
    """the reference's three (dt, gt) blocks of one frame"""
    ov, _, _, _ = ev.calculate_iou_partly([d], [g], 0, 1)
    blocks = [ov[0]]
    for metric in (1, 2):
        ov, _, _, _ = ev.calculate_iou_partly([d], [g], metric, 1)
        blocks.append(ov[0])
    return blocks


def margin_ok(blocks):
    for b in blocks:
        v = np.asarray(b, np.float64).ravel()
        for lv in LEVELS:
            if v.size and np.abs(v - lv).min() < MARGIN:
                return False
    return True


def make_set(ev, rng, kinds, names=NAMES):
    gts, dts, blocks, redraw_margin, redraw_ninth = [], [], [], 0, 0
    for kind in kinds:
        while True:
            g, d = draw_frame(rng, kind, names)
            try:
                b = frame_blocks(ev, g, d)
            except IndexError:
                redraw_ninth += 1
                continue
            if not margin_ok(b):
                redraw_margin += 1
                continue
            break
        gts.append(g)
        dts.append(d)
        blocks.append(b)
    return gts, dts, blocks, redraw_margin, redraw_ninth


def pack_annos(prefix, annos, out):
    out[prefix + "_num"] = np.array([len(a["name"]) for a in annos], np.int32)
    out[prefix + "_name"] = np.array([NAMES.index(str(n)) for a in annos for n in a["name"]], np.int8)
    for f in FIELDS:
        out[prefix + "_" + f] = np.concatenate([a[f] for a in annos], axis=0)


def run_official(ev, gts, dts, classes):
    """get_official_eval_result with the thresholds and pr tables of every (metric, difficulty, overlap row) recorded"""
    records = []
    real_thr, real_fused, real_class = ev.get_thresholds, ev.fused_compute_statistics, ev.eval_class

    def thr(scores, num_gt, num_sample_pts=41):
        t = real_thr(scores, num_gt, num_sample_pts)
        records.append({"thresholds": np.array(t, np.float64), "pr": np.zeros((0, 4))})
        return t

    def fused(overlaps, pr, *a, **kw):
        real_fused(overlaps, pr, *a, **kw)
        records[-1]["pr"] = pr

    curves = []

    def eval_class(*a, **kw):
        ret = real_class(*a, **kw)
        curves.append(ret)
        return ret

    ev.get_thresholds, ev.fused_compute_statistics, ev.eval_class = thr, fused, eval_class
    try:
        with np.errstate(all="ignore"):
            result, ret = ev.get_official_eval_result(gts, dts, classes)
    finally:
        ev.get_thresholds, ev.fused_compute_statistics, ev.eval_class = real_thr, real_fused, real_class
    return result, ret, records, curves


def store_run(prefix, out, result, ret, records, curves, num_classes):
    out[prefix + "_result"] = np.array(result)
    out[prefix + "_ret"] = np.array([ret[k] for k in sorted(ret)], np.float64)
    out[prefix + "_ret_keys"] = np.array(sorted(ret))
    it = iter(records)
    for metric in range(3):
        for m in range(num_classes):
            for l in range(3):
                for k in range(2):
                    r = next(it)
                    key = "%s_m%d_c%d_d%d_k%d" % (prefix, metric, m, l, k)
                    out[key + "_thresholds"] = r["thresholds"]
                    out[key + "_pr"] = np.array(r["pr"], np.float64)
        for name in ("precision", "recall", "orientation"):
            out["%s_m%d_%s" % (prefix, metric, name)] = curves[metric][name]


def main():
    ev = load_reference()
    rng = np.random.default_rng(20240607)
    kinds = ["plain"] * 60
    for i, k in ((3, "no_gt"), (7, "no_dt"), (11, "neither"), (13, "ties"), (29, "ties")):
        kinds[i] = k
    for i in range(16, 26):
        kinds[i] = "pairs"
    out = {"names": np.array(NAMES)}
    gts, dts, blocks, rm, rn = make_set(ev, rng, kinds)
    pack_annos("a_gt", gts, out)
    pack_annos("a_dt", dts, out)
    for metric in range(3):
        out["a_overlaps_m%d" % metric] = np.concatenate([b[metric].astype(np.float64).ravel() for b in blocks])
    out["a_redraws"] = np.array([rm, rn], np.int32)
    for d in range(3):   # clean_data for Car
        rows = [ev.clean_data(g, t, 0, d) for g, t in zip(gts, dts)]
        out["a_ignored_gt_d%d" % d] = np.concatenate([np.array(r[1], np.int8) for r in rows])
        out["a_ignored_dt_d%d" % d] = np.concatenate([np.array(r[2], np.int8) for r in rows])
        out["a_num_valid_gt_d%d" % d] = np.array([r[0] for r in rows], np.int32)
        out["a_dc_num"] = np.array([len(r[3]) for r in rows], np.int32)
    result, ret, records, curves = run_official(ev, gts, dts, [0])
    store_run("a_car", out, result, ret, records, curves, 1)
    print(result)
    result, ret, records, curves = run_official(ev, gts, dts, [0, 1, 2])
    out["a_all_result"] = np.array(result)
    out["a_all_ret"] = np.array([ret[k] for k in sorted(ret)], np.float64)
    print(result)
    # the second set: Cyclist detections, no valid Cyclist ground truth (50 frames: the reference's split into 50 parts fails below that)
    no_cyc = [n for n in NAMES if n != "Cyclist"]
    gts2, dts2, blocks2, rm2, rn2 = make_set(ev, rng, (["plain"] * 7 + ["no_gt", "no_dt", "neither"]) * 5, no_cyc)
    for d in dts2:
        if len(d["name"]):
            d["name"][0] = "Cyclist"
    pack_annos("b_gt", gts2, out)
    pack_annos("b_dt", dts2, out)
    for metric in range(3):
        out["b_overlaps_m%d" % metric] = np.concatenate([b[metric].astype(np.float64).ravel() for b in blocks2])
    result, ret, records, curves = run_official(ev, gts2, dts2, [2])
    store_run("b_cyc", out, result, ret, records, curves, 1)
    print(result, "redraws (margin, ninth point):", rm, rn, rm2, rn2)
    path = os.path.join(HERE, "kitti_eval.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit("needs the reference checkout at " + REF)
    main()

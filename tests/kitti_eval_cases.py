"""What the two KITTI-evaluator test files share: tests/golden/kitti_eval.npz unpacked into the reference's anno dicts, and the
seeded data sets at the kernels' launch-geometry boundaries."""
import numpy as np

from conftest import golden

FIELDS = ("truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y", "score")
MARGIN = 1e-4          # ten times the value tolerance of the rotated overlaps
ROTATED_TOL = 1e-5
_cache = {}


def load():
    if "fx" not in _cache:
        _cache["fx"] = golden("kitti_eval.npz")
    return _cache["fx"]


def annos(fx, prefix):
    """the list of per-frame dicts, as get_label_annos returns them"""
    names = [str(n) for n in fx["names"]]
    num = fx[prefix + "_num"]
    off = np.concatenate([[0], np.cumsum(num)])
    out = []
    for f in range(len(num)):
        a, b = int(off[f]), int(off[f + 1])
        d = {"name": np.array([names[c] for c in fx[prefix + "_name"][a:b]], dtype="<U16")}
        for key in FIELDS:
            d[key] = np.array(fx[prefix + "_" + key][a:b])
        out.append(d)
    return out


def blocks(fx, key, gt_annos, dt_annos):
    """the stored flat overlaps of one metric as per-frame (dt, gt) blocks"""
    flat = fx[key]
    out, pos = [], 0
    for g, d in zip(gt_annos, dt_annos):
        n = len(d["name"]) * len(g["name"])
        out.append(flat[pos:pos + n].reshape(len(d["name"]), len(g["name"])))
        pos += n
    assert pos == flat.size
    return out


def similarity_bound(terms, total):
    """n * 2^-52 * sum: the freedom is the summation order and one rounding of cos per term"""
    return terms * 2.0 ** -52 * total


def generated(frames, dt_counts, gt_counts, dc_counts, seed):
    """a seeded data set with the given per-frame counts (cycled): Car / Van / Pedestrian ground truths, detections that are
    jittered copies of a ground truth or far away, DontCare rows on top. Nothing is redrawn: the callers' seeds were chosen
    so that the margin condition (no overlap within MARGIN of 0.7 / 0.5 / 0.25) holds where they assert it"""
    rng = np.random.default_rng(seed)
    gts, dts = [], []
    for f in range(frames):
        ng, nd, ndc = gt_counts[f % len(gt_counts)], dt_counts[f % len(dt_counts)], dc_counts[f % len(dc_counts)]
        g = {k: [] for k in ("name",) + FIELDS}
        for i in range(ng + ndc):
            dc = i >= ng
            h2 = float(rng.choice([22.0, 30.0, 45.0, 80.0]))
            left, top = float(np.round(rng.uniform(0, 1100), 2)), float(np.round(rng.uniform(100, 250), 2))
            g["name"].append("DontCare" if dc else str(rng.choice(["Car", "Car", "Car", "Van", "Pedestrian"])))
            g["truncated"].append(-1.0 if dc else float(rng.choice([0.0, 0.2, 0.4, 0.6])))
            g["occluded"].append(-1 if dc else int(rng.integers(0, 4)))
            g["alpha"].append(-10.0 if dc else float(np.round(rng.uniform(-3, 3), 2)))
            g["bbox"].append([left, top, left + (150.0 if dc else h2 * 1.6), top + (60.0 if dc else h2)])
            g["dimensions"].append([-1.0] * 3 if dc else [float(np.round(v * rng.uniform(0.9, 1.1), 2)) for v in (3.9, 1.5, 1.6)])
            g["location"].append([-1000.0] * 3 if dc else [float(np.round(rng.uniform(-30, 30), 2)), float(np.round(rng.uniform(1.3, 1.9), 2)),
                                                          float(np.round(rng.uniform(4, 70), 2))])
            g["rotation_y"].append(-10.0 if dc else float(np.round(rng.uniform(-np.pi, np.pi), 2)))
            g["score"].append(0.0)
        d = {k: [] for k in ("name",) + FIELDS}
        for j in range(nd):
            src = int(rng.integers(0, ng + ndc)) if (ng + ndc) and rng.uniform() < 0.7 else -1
            if src >= 0:
                s = float(rng.choice([0.02, 0.1]))
                box = [float(np.round(v + rng.normal(0, s * 20), 2)) for v in g["bbox"][src]]
                dims = [float(np.round(abs(v) * (1 + rng.normal(0, s)), 2)) for v in (g["dimensions"][src] if src < ng else (3.9, 1.5, 1.6))]
                loc = [float(np.round(v + rng.normal(0, s * 3), 2)) for v in (g["location"][src] if src < ng else (0.0, 1.6, 80.0))]
                ry = float(np.round((g["rotation_y"][src] if src < ng else 0.0) + rng.normal(0, s), 2))
            else:
                left, top, h2 = float(np.round(rng.uniform(0, 1100), 2)), float(np.round(rng.uniform(100, 250), 2)), float(rng.choice([22.0, 30.0, 45.0]))
                box, dims = [left, top, left + h2 * 1.5, top + h2], [3.9, 1.5, 1.6]
                loc, ry = [float(np.round(rng.uniform(-30, 30), 2)), 1.6, float(np.round(rng.uniform(4, 70), 2))], float(np.round(rng.uniform(-3, 3), 2))
            d["name"].append(str(rng.choice(["Car", "Car", "Car", "Car", "Pedestrian"])))
            d["truncated"].append(0.0)
            d["occluded"].append(0)
            d["alpha"].append(float(np.round(rng.uniform(-3, 3), 2)))
            d["bbox"].append(box)
            d["dimensions"].append(dims)
            d["location"].append(loc)
            d["rotation_y"].append(ry)
            d["score"].append(float(np.round(rng.uniform(0.01, 0.99), 2)))   # two decimals: equal scores do occur
        for a, lst in ((g, gts), (d, dts)):
            out = {"name": np.array(a["name"], dtype="<U16")}
            for key in FIELDS:
                out[key] = np.array(a[key], np.int64 if key == "occluded" else np.float64)
            for key, w in (("bbox", 4), ("dimensions", 3), ("location", 3)):
                out[key] = out[key].reshape(-1, w)
            lst.append(out)
    return gts, dts

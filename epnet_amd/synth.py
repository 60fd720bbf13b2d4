"""Synthetic KITTI-shaped inputs. No dataset is needed.

All generators are deterministic functions of an integer seed (``torch.Generator`` on the CPU) and
return contiguous fp32 CPU tensors; callers move them to the GPU.
"""
import math

import torch

# PC_AREA_SCOPE, reference lib/config.py:26-28: x in [-40,40], y in [-1,3], z in [0,70.4]
SCOPE = ((-40.0, 40.0), (-1.0, 3.0), (0.0, 70.4))
CLS_MEAN_SIZE = (1.52563191462, 1.62856739989, 3.88311640418)  # (h, w, l), reference yaml:19


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def ubox_cloud(n, seed=0):
    """uniform in the detection scope: the worst case for ball query (almost no early exits)"""
    g = _gen(seed)
    u = torch.rand((n, 3), generator=g, dtype=torch.float32)
    lo = torch.tensor([s[0] for s in SCOPE], dtype=torch.float32)
    hi = torch.tensor([s[1] for s in SCOPE], dtype=torch.float32)
    return (lo + u * (hi - lo)).contiguous()


def object_boxes(num, seed=0):
    """(num,7) [x, y(bottom), z, h, w, l, ry] car-sized boxes on the ground plane"""
    g = _gen(seed + 7919)
    r = torch.rand((num, 6), generator=g, dtype=torch.float32)
    rho = 5.0 + r[:, 0] * 55.0
    az = (r[:, 1] - 0.5) * math.radians(70.0)
    x, z = rho * torch.sin(az), rho * torch.cos(az)
    size = torch.tensor(CLS_MEAN_SIZE, dtype=torch.float32) * (0.8 + 0.4 * r[:, 2:5])
    ry = (r[:, 5] * 2 - 1) * math.pi
    y = torch.full((num,), 1.65, dtype=torch.float32)
    return torch.cat([x[:, None], y[:, None], z[:, None], size, ry[:, None]], dim=1).contiguous()


def kitti_like_cloud(n, seed=0, num_objects=40, return_boxes=False):
    """85 % ground returns (y = 1.65 + N(0, 0.03), range pdf ~ 1/rho on [2,70] m, azimuth +-40 deg) and
    15 % points on the surfaces of `num_objects` car-sized boxes; clipped to the scope; shuffled"""
    g = _gen(seed)
    n_obj = int(round(n * 0.15))
    n_gnd = n - n_obj
    u = torch.rand((n_gnd, 2), generator=g, dtype=torch.float32)
    rho = 2.0 * (35.0 ** u[:, 0])  # log-uniform on [2,70]  <=> pdf ~ 1/rho
    az = (u[:, 1] - 0.5) * math.radians(80.0)
    gy = 1.65 + 0.03 * torch.randn((n_gnd,), generator=g, dtype=torch.float32)
    ground = torch.stack([rho * torch.sin(az), gy, rho * torch.cos(az)], dim=1)

    boxes = object_boxes(num_objects, seed)
    which = torch.randint(0, num_objects, (n_obj,), generator=g)
    b = boxes[which]
    uvw = torch.rand((n_obj, 3), generator=g, dtype=torch.float32) - 0.5  # box frame, in [-.5,.5]
    face = torch.randint(0, 3, (n_obj,), generator=g)
    sign = torch.randint(0, 2, (n_obj,), generator=g).float() - 0.5
    uvw[torch.arange(n_obj), face] = sign  # snap one coordinate to a face
    lx, hy, wz = uvw[:, 0] * b[:, 5], uvw[:, 1] * b[:, 3], uvw[:, 2] * b[:, 4]
    c, s = torch.cos(b[:, 6]), torch.sin(b[:, 6])
    ox = b[:, 0] + lx * c + wz * s
    oz = b[:, 2] - lx * s + wz * c
    oy = b[:, 1] - b[:, 3] / 2 + hy
    obj = torch.stack([ox, oy, oz], dim=1)

    pts = torch.cat([ground, obj], dim=0)
    for d in range(3):
        pts[:, d].clamp_(SCOPE[d][0], SCOPE[d][1])
    pts = pts[torch.randperm(n, generator=g)].contiguous()
    return (pts, boxes) if return_boxes else pts


def dup_cloud(n, seed=0, unique=12000):
    """`unique` KITTI-like points padded to n by re-drawing existing rows, as the dataset pads short
    clouds (reference lib/datasets/kitti_rcnn_dataset.py:338-342): exercises FPS tie-breaks"""
    base = kitti_like_cloud(min(unique, n), seed)
    if n <= base.shape[0]:
        return base[:n].contiguous()
    g = _gen(seed + 104729)
    extra = torch.randint(0, base.shape[0], (n - base.shape[0],), generator=g)
    return torch.cat([base, base[extra]], dim=0).contiguous()


def kitti_q_cloud(n, seed=0):
    """KITTI-like coordinates rounded to 1e-3 m, the resolution velodyne .bin files carry: decimal-quantised coordinates
    make equal fp32 distances (FPS ties) far likelier than the continuous generator does"""
    return (torch.round(kitti_like_cloud(n, seed) * 1000.0) / 1000.0).contiguous()


KINDS = {"ubox": ubox_cloud, "kitti": kitti_like_cloud, "dup": dup_cloud, "kitti_q": kitti_q_cloud}


def cloud(kind, n, seed=0):
    return KINDS[kind](n, seed)


def scenes(kind, batch, n, seed=0):
    """(batch, n, 3) stack of independent scenes; scene i uses seed + i"""
    return torch.stack([KINDS[kind](n, seed + i) for i in range(batch)], dim=0).contiguous()


def proposal_boxes(num, seed=0, num_objects=40, jitter=1.0):
    """(num,7) boxes scattered around the scene's objects (for iou3d / roipool3d / NMS inputs) + scores"""
    g = _gen(seed + 15485863)
    obj = object_boxes(num_objects, seed)
    pick = obj[torch.randint(0, num_objects, (num,), generator=g)].clone()
    pick[:, [0, 2]] += (torch.rand((num, 2), generator=g) * 2 - 1) * jitter
    pick[:, 3:6] *= 0.8 + 0.4 * torch.rand((num, 3), generator=g)
    pick[:, 6] += (torch.rand((num,), generator=g) * 2 - 1) * 0.3
    scores = torch.rand((num,), generator=g, dtype=torch.float32)
    return pick.contiguous(), scores


def lidar_scan(p, seed=0):
    """(p,4) [x, y, z, intensity] in the velodyne frame (x forward, y left, z up), as a KITTI .bin scan holds them: ground
    returns and returns from upright surfaces over the WHOLE azimuth, ranges log-uniform on [3, 80] m, the sensor 1.73 m above
    the ground, coordinates rounded to 1e-3 m, intensity in [0, 1). Most points fail the camera-view test, as in a real scan
    (about 120 000 raw points give some 18 000 in view)."""
    g = _gen(seed + 32452843)
    u = torch.rand((p, 5), generator=g, dtype=torch.float32)
    rho = 3.0 * ((80.0 / 3.0) ** u[:, 0])
    az = (u[:, 1] * 2 - 1) * math.pi
    ground = u[:, 2] < 0.7
    z = torch.where(ground, -1.73 + 0.03 * torch.randn((p,), generator=g, dtype=torch.float32), -1.73 + 2.5 * u[:, 3])
    xyz = torch.stack([rho * torch.cos(az), rho * torch.sin(az), z], dim=1)
    xyz = torch.round(xyz * 1000.0) / 1000.0
    return torch.cat([xyz, u[:, 4:5]], dim=1).contiguous()


def gt_database(num, seed=0, min_points=3, max_points=600):
    """a GT database in the form tools/generate_gt_database.py pickles: a list of `num` dicts with 'gt_box3d' (7) float32 (car-sized,
    anywhere object_boxes puts them), 'points' (n,3) on the box's surfaces, 'intensity' (n) in [0, 1) and 'alpha'; n is
    log-uniform on [min_points, max_points], so that both the easy (more than 100 points) and the hard list are populated"""
    g = _gen(seed + 86028121)
    boxes = object_boxes(num, seed + 1)
    out = []
    for k in range(num):
        u = torch.rand((3,), generator=g, dtype=torch.float32)
        n = int(min_points * (max_points / float(min_points)) ** float(u[0]))
        r = torch.rand((n, 4), generator=g, dtype=torch.float32)
        h, w, l, ry = (float(v) for v in boxes[k, 3:7])
        local = torch.stack([(r[:, 0] - 0.5) * l, -r[:, 1] * h, (r[:, 2] - 0.5) * w], dim=1)
        c, s = math.cos(ry), math.sin(ry)
        pts = torch.stack([local[:, 0] * c + local[:, 2] * s, local[:, 1], -local[:, 0] * s + local[:, 2] * c], dim=1) + boxes[k, :3]
        out.append({"gt_box3d": boxes[k].numpy().copy(), "points": pts.contiguous().numpy(), "intensity": r[:, 3].contiguous().numpy(),
                    "alpha": float((u[1] * 2 - 1) * math.pi)})
    return out


def calibration(seed=0):
    """KITTI-typical calibration: V2C (3,4), R0 (3,3), P2 (3,4) fp32 and img_shape int32 [h, w] = [375, 1242]; the seed moves
    the principal point and the mounting by amounts of the size that differ between recording days"""
    g = _gen(seed + 49979687)
    d = torch.randn((4,), generator=g, dtype=torch.float64)
    V2C = torch.tensor([[7.533745e-03, -9.999714e-01, -6.166020e-04, -4.069766e-03],
                        [1.480249e-02, 7.280733e-04, -9.998902e-01, -7.631618e-02],
                        [9.998621e-01, 7.523790e-03, 1.480755e-02, -2.717806e-01]], dtype=torch.float64)
    V2C[:, 3] += 1e-3 * d[0:3]
    R0 = torch.tensor([[9.999239e-01, 9.837760e-03, -7.445048e-03], [-9.869795e-03, 9.999421e-01, -4.278459e-03],
                       [7.402527e-03, 4.351614e-03, 9.999631e-01]], dtype=torch.float64)
    P2 = torch.tensor([[7.215377e+02, 0.0, 6.095593e+02, 4.485728e+01], [0.0, 7.215377e+02, 1.728540e+02, 2.163791e-01],
                       [0.0, 0.0, 1.0, 2.745884e-03]], dtype=torch.float64)
    P2[0, 2] += 2.0 * d[3]
    return V2C.float().contiguous(), R0.float().contiguous(), P2.float().contiguous(), torch.tensor([375, 1242], dtype=torch.int32)


def kitti_eval_annos(frames, seed=0, mean_gt=6.0, mean_dt=10.0):
    """(gt_annos, dt_annos) for the AP evaluator (epnet_amd.kitti_eval), as get_label_annos returns them: numpy dicts, not
    tensors -- the evaluator's input is label files. Per frame about mean_gt ground truths (Car / Van / Pedestrian / Cyclist /
    DontCare, all occlusion levels, truncations and 2D heights either side of the difficulty limits) and about mean_dt
    detections: jittered copies of ground truths, duplicates, boxes over DontCare regions and pure false positives.
    KITTI val is 3769 frames."""
    import numpy as np
    rng = np.random.default_rng(seed)
    names = ["Car", "Car", "Car", "Van", "Pedestrian", "Cyclist", "DontCare"]
    dims_of = {"Car": (3.9, 1.5, 1.6), "Van": (5.0, 2.2, 1.9), "Pedestrian": (0.8, 1.8, 0.6), "Cyclist": (1.8, 1.7, 0.6)}
    keys = ("name", "truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y", "score")

    def pack(rows):
        out = {"name": np.array([r[0] for r in rows], dtype="<U16")}
        for i, (key, width) in enumerate((("truncated", 1), ("occluded", 1), ("alpha", 1), ("bbox", 4), ("dimensions", 3),
                                          ("location", 3), ("rotation_y", 1), ("score", 1)), start=1):
            a = np.array([r[i] for r in rows], np.int64 if key == "occluded" else np.float64)
            out[key] = a.reshape(-1, width) if width > 1 else a.reshape(-1)
        return out

    gts, dts = [], []
    for _ in range(frames):
        g, d = [], []
        for _ in range(int(rng.poisson(mean_gt))):
            name = names[int(rng.integers(len(names)))]
            left, top, height = rng.uniform(0, 1100), rng.uniform(120, 250), float(rng.choice([20.0, 30.0, 45.0, 70.0, 120.0]))
            box = [left, top, left + height * rng.uniform(0.6, 2.0), top + height]
            if name == "DontCare":
                g.append((name, -1.0, -1, -10.0, box, [-1.0] * 3, [-1000.0] * 3, -10.0, 0.0))
                continue
            l, h, w = (v * rng.uniform(0.85, 1.15) for v in dims_of[name])
            g.append((name, float(rng.choice([0.0, 0.1, 0.2, 0.4, 0.6])), int(rng.integers(0, 4)), rng.uniform(-math.pi, math.pi), box,
                      [l, h, w], [rng.uniform(-30, 30), rng.uniform(1.3, 1.9), rng.uniform(4, 70)], rng.uniform(-math.pi, math.pi), 0.0))
        share = mean_dt / max(mean_gt, 1.0)
        for row in g:
            for _ in range(int(rng.poisson(share * 0.8))):
                s = 0.03 if rng.uniform() < 0.7 else 0.15
                cls = "Car" if row[0] == "DontCare" else row[0]
                box = [v + rng.normal(0, s * 30) for v in row[4]]
                dims = [abs(v) * (1 + rng.normal(0, s)) for v in (row[5] if row[0] != "DontCare" else dims_of["Car"])]
                loc = [v + rng.normal(0, s * 3) for v in (row[6] if row[0] != "DontCare" else (0.0, 1.6, 75.0))]
                d.append((cls, 0.0, 0, row[3] + rng.normal(0, 0.2), box, dims, loc, row[7] + rng.normal(0, s), rng.uniform(0.05, 1.0)))
        for _ in range(int(rng.poisson(share * 0.2 * mean_gt))):
            left, top, height = rng.uniform(0, 1100), rng.uniform(120, 250), float(rng.choice([20.0, 30.0, 45.0]))
            d.append(("Car", 0.0, 0, rng.uniform(-3, 3), [left, top, left + height * 1.5, top + height], list(dims_of["Car"]),
                      [rng.uniform(-30, 30), 1.6, rng.uniform(4, 70)], rng.uniform(-3, 3), rng.uniform(0.05, 0.5)))
        gts.append(pack(g))
        dts.append(pack(d))
    assert keys == tuple(gts[0])
    return gts, dts

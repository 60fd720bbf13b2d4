"""Regenerates tests/golden/rpn_targets.npz. Runs ONLY where the reference checkout is available; the fixture is plain data.

What runs is the REFERENCE'S OWN Python, imported unmodified through make_golden_rcnn.import_reference():
``KittiRCNNDataset.data_augmentation`` and ``KittiRCNNDataset.generate_rpn_training_labels``
(lib/datasets/kitti_rcnn_dataset.py:698-755, :547-576), called on ``object.__new__(KittiRCNNDataset)`` so that no dataset is
needed on disk. While data_augmentation runs, ``np.random.rand`` / ``np.random.uniform`` are replaced by readers of the given
draws (the reference code itself is untouched). Every on/off combination of the three methods is one scene, plus a scene
without boxes.

As in the loader, the reference's methods see a scene's own boxes; the zero padding rows are added afterwards, as
collate_batch adds them. The scenes: overlapping pairs of boxes, headings near +-pi, one to five real boxes in six rows.
Points are drawn so that most fall in and just around the boxes (uniform in each box's frame, half extents + 0.5 m), the
rest over the scene's range. A scene with more than 0.5 % of its points within 1e-4 m of a face of a box or an enlarged box
is redrawn (the restatement measures it). Stored: inputs, draws and the reference's outputs only.
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import rpn_targets_restate as rs  # noqa: E402
from make_golden_rcnn import import_reference  # noqa: E402

F = np.float32
ROWS = 6
BAND, SHARE = 1e-4, 0.005
# (points, real boxes) per scene; scene i < 8 has methods (rotation, scaling, flip) = bits of i
SCENES = [(1024, 5), (1024, 2), (777, 3), (1024, 4), (1023, 5), (1024, 1), (1024, 3), (2048, 5), (256, 0)]


class Draws:
    """np.random.rand(3) -> 1 - aug_enable, np.random.uniform -> the angle, then the scale, while data_augmentation runs"""

    def __init__(self, on, angle, scale):
        self.on, self.values, self.saved = on, [("angle", angle), ("scale", scale)], None

    def rand(self, *shape):
        assert shape == (3,)
        return np.array([1.0 if o else 0.0 for o in self.on])       # aug_enable = 1 - rand: 0 (on) or 1 (off)

    def uniform(self, low, high):
        want = "angle" if low < 0 else "scale"
        name, v = next(p for p in self.values if p[0] == want)
        assert low <= v <= high, (name, low, v, high)
        return v

    def __enter__(self):
        self.saved = (np.random.rand, np.random.uniform)
        np.random.rand, np.random.uniform = self.rand, self.uniform
        return self

    def __exit__(self, *exc):
        np.random.rand, np.random.uniform = self.saved
        return False


def draw_scene(rng, n, real):
    gt = np.zeros((real, 7))
    for k in range(real):
        gt[k] = [rng.uniform(-20, 20), rng.uniform(1.0, 2.0), rng.uniform(8, 60), rng.normal(1.53, 0.1), rng.normal(1.63, 0.1),
                 rng.normal(3.88, 0.3), rng.uniform(-np.pi, np.pi)]
    if real >= 2:                                   # an overlapping pair: box 1 over a corner of box 0
        gt[1, 0:3] = gt[0, 0:3] + [0.9, 0.05, 1.1]
        gt[1, 6] = gt[0, 6] + 0.6
    if real >= 4:                                   # a second pair, the earlier box mostly inside the later one's margin
        gt[3, 0:3] = gt[2, 0:3] + [0.3, -0.1, 1.5]
        gt[3, 6] = gt[2, 6] - 1.2
    if real >= 3:
        gt[2, 6] = 3.1                              # headings near +-pi
    if real >= 5:
        gt[4, 6] = -3.12
    gt = gt.astype(F)
    pts = np.stack([rng.uniform(-40, 40, n), rng.uniform(-1, 3, n), rng.uniform(0, 70, n)], axis=1)
    if real:
        near = rng.uniform(size=n) < 0.75
        which = rng.integers(0, real, n)
        b = gt[which].astype(np.float64)
        half = np.stack([b[:, 5] / 2, b[:, 3] / 2, b[:, 4] / 2], axis=1) + 0.5
        q = rng.uniform(-1, 1, (n, 3)) * half
        c, s = np.cos(b[:, 6]), np.sin(b[:, 6])
        local = np.stack([b[:, 0] + q[:, 0] * c + q[:, 2] * s, b[:, 1] - b[:, 3] / 2 + q[:, 1], b[:, 2] - q[:, 0] * s + q[:, 2] * c], axis=1)
        pts[near] = local[near]
    alpha = rng.uniform(-np.pi, np.pi, real).astype(F)
    return pts.astype(F), gt, alpha


def main():
    cfg = import_reference()[0]
    from lib.datasets.kitti_rcnn_dataset import KittiRCNNDataset
    cfg.AUG_METHOD_LIST, cfg.AUG_METHOD_PROB, cfg.AUG_ROT_RANGE = ["rotation", "scaling", "flip"], [0.5, 0.5, 0.5], 18
    ds = object.__new__(KittiRCNNDataset)
    out = {"scenes": np.int64(len(SCENES)), "rows": np.int64(ROWS), "extra_width": np.float64(0.2)}
    for i, (n, real) in enumerate(SCENES):
        on = (bool(i & 1), bool(i & 2), bool(i & 4)) if i < 8 else (True, True, True)
        for attempt in range(50):
            rng = np.random.default_rng(9000 + 100 * i + attempt)
            pts, gt, alpha = draw_scene(rng, n, real)
            angle = float(F(rng.uniform(-np.pi / 18, np.pi / 18)))          # fp32 numbers: the device table holds fp32
            scale = float(F(rng.uniform(0.95, 1.05)))
            with Draws(on, angle, scale):
                aug_pts, aug_gt, method = ds.data_augmentation(pts.copy(), gt.copy(), alpha.copy())
            assert aug_pts.dtype == F and aug_gt.dtype == F and len(method) == sum(on), (aug_pts.dtype, aug_gt.dtype, method)
            cls, reg = KittiRCNNDataset.generate_rpn_training_labels(aug_pts, aug_gt)
            dist = rs.labels(aug_pts, aug_gt)[2]
            share = float((dist <= BAND).mean())
            if share <= SHARE:
                break
        else:
            raise AssertionError("scene %d: too many points on a face after 50 draws" % i)
        pad = lambda a: np.concatenate([a, np.zeros((ROWS - real,) + a.shape[1:], a.dtype)])  # noqa: E731
        pre = "s%d__" % i
        out[pre + "pts"], out[pre + "gt"], out[pre + "alpha"] = pts, pad(gt), pad(alpha)
        out[pre + "aug"] = np.array([on[0], angle if on[0] else 0.0, scale if on[1] else 1.0, on[2]], F)
        out[pre + "ref_pts"], out[pre + "ref_gt"] = aug_pts, pad(aug_gt)
        out[pre + "ref_cls"], out[pre + "ref_reg"] = cls.astype(np.int8), reg
        print("scene %d: %4d points, %d boxes, methods %s, fg %d, ignored %d, class -1 with a row %d, on a face %.3f %% (draw %d)" % (
            i, n, real, on, int((cls == 1).sum()), int((cls == -1).sum()), int(((cls == -1) & reg.any(axis=1)).sum()), 100 * share, attempt))
    path = os.path.join(HERE, "rpn_targets.npz")
    np.savez_compressed(path, **out)
    print("wrote rpn_targets.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

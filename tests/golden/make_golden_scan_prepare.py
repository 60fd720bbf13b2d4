"""Regenerates tests/golden/scan_prepare.npz. Runs ONLY where the reference checkout is available; the fixture is plain data.

What runs is the REFERENCE'S OWN Python, imported unmodified through make_golden_rcnn.import_reference():
``KittiRCNNDataset.get_rpn_with_li_fusion`` (lib/datasets/kitti_rcnn_dataset.py:281-367) with ``Calibration``
(lib/utils/calibration.py) and ``get_valid_flag``, called on ``object.__new__(KittiRCNNDataset)`` with ``mode = 'TEST'`` and
``random_select = True`` so that no dataset is needed on disk: ``get_calib``, ``get_lidar``, ``get_image_shape`` and
``get_image_rgb_with_normal`` are instance-level stand-ins that hand over the scene (Calibration accepts a dict).

Randomness. While the reference method runs, ``np.random.choice`` returns the r members with the smallest (unsigned key, row),
in row order, by the scene's table of keys -- one uniform r-subset, as choice(replace=False) draws -- and ``np.random.shuffle``
applies the stored ``slot_perm``: row slot_perm[j] receives entry j of the list in the contract's order (the forced points
first, then the subset; the reference concatenates the subset first when there are far points, which a shuffle is free to undo).
The reference code itself is untouched. Its ``choice`` indexes the rows that passed get_valid_flag; the fixture stores the raw
rows (through the flag the reference itself computed).

The scenes are synthetic full-azimuth scans, p <= 4096 and n <= 1024: case 0 without far points, case 0 with far points,
case 1 (V == n), case 2, and case 2 at V == n / 2. Every raw point within 1e-2 px of an image edge or within 1e-3 m of depth 0,
of a face of the scope or of z = 40 (judged in float64) is removed from the scan, so no decision of the float32 evaluation can
differ from the reference's. Stored: inputs, tables and the reference's outputs only.
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import scan_restate as rs  # noqa: E402
from make_golden_rcnn import import_reference  # noqa: E402

F = np.float32
# (raw points drawn, largest range, how n follows from V)
SCENES = [(4096, 38.0, lambda v: 256), (4096, 80.0, lambda v: 256), (3000, 80.0, lambda v: v), (2500, 80.0, lambda v: v + v // 3),
          (1501, 60.0, lambda v: 2 * v)]
WANT_CASES = [0, 0, 1, 2, 2]


class Draws:
    """np.random.choice and np.random.shuffle from the scene's tables while get_rpn_with_li_fusion runs"""

    def __init__(self, keys, slot_perm):
        self.keys, self.slot_perm, self.rows, self.pool, self.size, self.final, self.saved = keys, slot_perm, None, None, 0, None, None

    def flag(self, fn):
        def wrapped(*args):
            valid = fn(*args)
            self.rows = np.nonzero(valid)[0]
            return valid
        return wrapped

    def choice(self, a, size, replace=True):
        assert replace is False and self.rows is not None
        self.pool, self.size = np.array(a), int(size)
        return rs.smallest(a, self.keys[self.rows], size).astype(np.asarray(a).dtype)

    def shuffle(self, arr):
        rot = 0 if self.pool is None or np.array_equal(arr[:len(self.pool)], self.pool) else self.size
        ordered = np.roll(arr, -rot)                     # (subset, far) -> (far, subset)
        arr[self.slot_perm] = ordered
        self.final = self.rows[arr]

    def __enter__(self):
        self.saved = (np.random.choice, np.random.shuffle)
        np.random.choice, np.random.shuffle = self.choice, self.shuffle
        return self

    def __exit__(self, *exc):
        np.random.choice, np.random.shuffle = self.saved
        return False


def draw_scan(rng, p, far, V2C, R0, P2, shape):
    u = rng.uniform(size=(p, 5))
    rho = 3.0 * ((far / 3.0) ** u[:, 0])
    az = (u[:, 1] * 2 - 1) * np.pi
    z = np.where(u[:, 2] < 0.7, -1.73 + 0.03 * rng.normal(size=p), -1.73 + 2.5 * u[:, 3])
    pts = np.stack([rho * np.cos(az), rho * np.sin(az), z, u[:, 4]], axis=1).astype(F)
    rect, uv, depth = rs.transform64(pts, V2C, R0, P2)
    edge = np.minimum.reduce([np.abs(uv[:, 0]), np.abs(uv[:, 0] - shape[1]), np.abs(uv[:, 1]), np.abs(uv[:, 1] - shape[0])]) < 1e-2
    face = np.abs(depth) < 1e-3
    for j in range(3):
        face |= (np.abs(rect[:, j] - rs.SCOPE[j, 0]) < 1e-3) | (np.abs(rect[:, j] - rs.SCOPE[j, 1]) < 1e-3)
    face |= np.abs(rect[:, 2] - 40.0) < 1e-3
    return pts[~(edge | face)]


def main():
    cfg = import_reference()[0]
    from lib.datasets.kitti_rcnn_dataset import KittiRCNNDataset
    from lib.utils.calibration import Calibration
    assert cfg.PC_REDUCE_BY_RANGE and cfg.RPN.USE_INTENSITY and np.array_equal(np.asarray(cfg.PC_AREA_SCOPE, np.float64), rs.SCOPE)
    out = {"scenes": np.int64(len(SCENES))}
    for i, (p0, far, n_of) in enumerate(SCENES):
        rng = np.random.default_rng(7100 + i)
        V2C, R0, P2, shape = rs.calib(i)
        pts = draw_scan(rng, p0, far, V2C, R0, P2, shape)
        p = pts.shape[0]
        valid = rs.classify(pts, p, V2C, R0, P2, shape)[2]
        n = int(n_of(int(valid.sum())))
        assert 1 <= n <= 1024 and p <= 4096, (n, p)
        keys = rng.integers(-2 ** 31, 2 ** 31, p).astype(np.int32)
        keys[rng.integers(0, p, p // 8)] = keys[0]                      # some equal keys: the row decides
        slot_perm = rng.permutation(n).astype(np.int32)

        ds = object.__new__(KittiRCNNDataset)
        ds.sample_id_list, ds.mode, ds.random_select, ds.npoints = [0], "TEST", True, n
        ds.get_calib = lambda idx: Calibration({"P2": P2, "R0": R0, "Tr_velo2cam": V2C})
        ds.get_lidar = lambda idx: pts.copy()
        ds.get_image_shape = lambda idx: (int(shape[0]), int(shape[1]), 3)
        ds.get_image_rgb_with_normal = lambda idx: None
        draws = Draws(keys, slot_perm)
        ds.get_valid_flag = draws.flag(KittiRCNNDataset.get_valid_flag)
        with draws:
            info = ds.get_rpn_with_li_fusion(0)
        assert info["pts_rect"].dtype == F and info["pts_origin_xy"].dtype == F and info["pts_input"].shape == (n, 4)
        mine = rs.prepare(pts, p, V2C, R0, P2, shape, keys, slot_perm, n)
        V, Fc, case = (int(v) for v in mine["scene_info"][1:4])
        assert case == WANT_CASES[i], (i, case)
        assert (i != 0 or Fc == 0) and (i != 1 or Fc > 0) and (i != 4 or 2 * V == n)
        pre = "s%d__" % i
        for key, value in (("pts", pts), ("V2C", V2C), ("R0", R0), ("P2", P2), ("img_shape", shape), ("keys", keys), ("slot_perm", slot_perm),
                           ("n", np.int64(n)), ("ref_pts_rect", info["pts_rect"]), ("ref_pts_features", info["pts_features"]),
                           ("ref_pts_input", info["pts_input"]), ("ref_pts_origin_xy", info["pts_origin_xy"]),
                           ("ref_choice", draws.final.astype(np.int32))):
            out[pre + key] = value
        print("scene %d: p %d, n %d, valid %d, far %d, case %d, choice equal to the restatement: %s" % (
            i, p, n, V, Fc, case, np.array_equal(draws.final, mine["choice"])))
    path = os.path.join(HERE, "scan_prepare.npz")
    np.savez_compressed(path, **out)
    print("wrote scan_prepare.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""Regenerates tests/golden/roipool3d_ref_trials.npz. Runs ONLY in the build container (needs /root/reference); the fixture is
plain data.

What runs is the REFERENCE'S OWN compiled roipool3d CPU ops (lib/utils/roipool3d/src/roipool3d.cpp:97-195, built unmodified by
oracle/build_ref.py) on three seeded random scenes -- the cases tests/test_oracle_golden.py::test_oracle_vs_live_reference_build
checks the oracle against wherever it runs, and against the live build as well where that build is at hand.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import build_ref  # noqa: E402


def trials():
    """(pts (n,3), boxes (m,7), features (n,c), sampled points s) of the three cases"""
    rng = np.random.default_rng(3)
    for trial in range(3):
        n, m, c, s = 3000 + 500 * trial, 24, 4 + trial, 48
        pts = (rng.random((n, 3)) * [30, 4, 30] - [15, 1, 0]).astype(np.float32)
        boxes = np.stack([rng.uniform(-15, 15, m), rng.uniform(0, 3, m), rng.uniform(0, 30, m), rng.uniform(1, 3, m),
                          rng.uniform(1, 5, m), rng.uniform(2, 9, m), rng.uniform(-4, 4, m)], 1).astype(np.float32)
        feat = rng.standard_normal((n, c)).astype(np.float32)
        yield pts, boxes, feat, s


def run_reference(ref, pts, boxes, feat, s):
    """the reference ops on one case: (flags (m,n) int64, pooled points, pooled features, empty flags)"""
    m, c = boxes.shape[0], feat.shape[1]
    flag = torch.zeros((m, pts.shape[0]), dtype=torch.int64)
    ref.pts_in_boxes3d_cpu(flag, torch.from_numpy(pts), torch.from_numpy(boxes))
    pp, pf, ef = torch.zeros((m, s, 3)), torch.zeros((m, s, c)), torch.zeros(m, dtype=torch.int64)
    ref.roipool3d_cpu(torch.from_numpy(pts), torch.from_numpy(boxes), torch.from_numpy(feat), pp, pf, ef)
    return flag.numpy(), pp.numpy(), pf.numpy(), ef.numpy()


def main():
    ref = build_ref.load()
    assert ref is not None, "the reference build is not available here"
    out = {}
    for k, (pts, boxes, feat, s) in enumerate(trials()):
        flag, pp, pf, ef = run_reference(ref, pts, boxes, feat, s)
        out.update({"pts_%d" % k: pts, "boxes3d_%d" % k: boxes, "pts_feature_%d" % k: feat,
                    "pts_flag_%d" % k: np.packbits(flag.astype(np.uint8), axis=1), "pooled_pts_%d" % k: pp,
                    "pooled_features_%d" % k: pf, "pooled_empty_flag_%d" % k: ef})
    path = os.path.join(HERE, "roipool3d_ref_trials.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()

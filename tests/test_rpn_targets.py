"""The RPN training targets without a GPU: the numpy restatement (tests/rpn_targets_restate.py) against what the reference's own
data_augmentation and generate_rpn_training_labels returned (tests/golden/rpn_targets.npz), the library's export, the Python
surface's refusal of CPU tensors, and draw_augmentation's rules.

Bounds (set by the fixture's design, tests/rpn_targets_restate.py): classes and regression rows are EQUAL for every point farther
than 1e-4 m from all faces of all boxes and enlarged boxes (13 fp32 ulps at 80 m); at most 0.5 % of a scene's points may be
nearer (a condition on the inputs); augmented x, z within 1 fp32 ulp of max(|x|, |z|), y exact; box columns 0..5 exact, ry
within 1e-5."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rpn_targets_restate as rs

SCENES, EXTRA = rs.fixture_scenes()


def test_fixture_covers_what_it_should():
    methods = {tuple(bool(v) for v in (s["aug"][0], s["aug"][2] != 1, s["aug"][3])) for s in SCENES if s["gt"][:, 3].any()}
    assert len(methods) == 8                                                    # every on/off combination
    assert any(not s["gt"].any() for s in SCENES)                               # a scene without boxes
    assert any((s["gt"][:, 3] == 0).any() and s["gt"][:, 3].any() for s in SCENES)   # zero padding rows behind real ones
    assert any((np.abs(np.abs(s["ref_gt"][:, 6]) - np.pi) < 0.1).any() for s in SCENES)   # a heading near +-pi
    # a later box's margin over an earlier box's foreground: class -1 with a non-zero regression row
    assert sum(int(((s["ref_cls"] == -1) & s["ref_reg"].any(axis=1)).sum()) for s in SCENES) > 50
    assert all(s["pts"].shape[0] <= 2048 and s["gt"].shape[0] <= 6 for s in SCENES)


@pytest.mark.parametrize("i", range(len(SCENES)))
def test_restatement_against_the_reference(i):
    s = SCENES[i]
    pts, gt = rs.augment(s["pts"], s["gt"], s["alpha"], s["aug"])
    bad = rs.augmentation_failures(i, pts, gt, s["ref_pts"], s["ref_gt"])
    # the labels from the reference's own augmented values, so that the two checks do not lean on each other
    cls, reg, dist = rs.labels(s["ref_pts"], s["ref_gt"], EXTRA)
    print("scene %d: %d points, %.3f %% within %g m of a face" % (i, len(cls), 100 * float((dist <= rs.BAND).mean()), rs.BAND))
    bad += rs.label_failures(i, cls, reg, s["ref_cls"], s["ref_reg"], dist)
    assert not bad, bad


def test_restatement_order_rule():
    """a point in box 0 and only in the margin of box 1: class -1 with box 0's row in order (0, 1), class 1 in order (1, 0)"""
    a = np.array([0, 1, 10, 1.5, 1.6, 4.0, 0.0], np.float32)            # z in [9.2, 10.8]
    b = np.array([0, 1, 11.7, 1.5, 1.6, 4.0, 0.25], np.float32)         # about z in [10.9, 12.5] at x = 0, its margin from 10.7
    p = np.array([[0.0, 0.5, 10.0], [0.0, 0.5, 10.75]], np.float32)     # in a alone; in a and in b's margin only
    cls, reg, _ = rs.labels(p, np.stack([a, b]))
    assert cls.tolist() == [1, -1] and reg[1, 6] == 0.0 and reg[1, 2] == np.float32(10) - np.float32(10.75) and reg[1, 5] == 4.0
    cls, reg, _ = rs.labels(p, np.stack([b, a]))
    assert cls.tolist() == [1, 1] and reg[1, 2] == np.float32(10) - np.float32(10.75)


def test_library_exports_the_op_and_the_surface_refuses_cpu_tensors(hiplib):
    assert hasattr(hiplib, "epnet_rpn_targets")
    from epnet_amd import rpn_target_cuda, rpn_target_layer
    pts, gt = torch.zeros((1, 8, 3)), torch.zeros((1, 2, 7))
    with pytest.raises(RuntimeError, match="CUDAtensor"):
        rpn_target_layer.rpn_training_labels(pts, gt)
    with pytest.raises(RuntimeError, match="CUDAtensor"):
        rpn_target_layer.augment_and_label(pts, gt, torch.zeros((1, 2)), torch.zeros((1, 4)))
    with pytest.raises(RuntimeError, match="CUDAtensor"):
        rpn_target_cuda.rpn_targets_gpu(pts, gt, None, None, 0.2, None, None, torch.zeros((1, 8), dtype=torch.int32), torch.zeros((1, 8, 7)))


def _cfg(prob, methods=("rotation", "scaling", "flip"), rot_range=18):
    return SimpleNamespace(AUG_METHOD_LIST=list(methods), AUG_METHOD_PROB=list(prob), AUG_ROT_RANGE=rot_range)


def test_draw_augmentation_rules():
    from epnet_amd.rpn_target_layer import draw_augmentation
    g = torch.Generator().manual_seed(3)
    off = draw_augmentation(512, _cfg([0.0, 0.0, 0.0]), g, device="cpu")
    assert off.shape == (512, 4) and off.dtype == torch.float32
    assert torch.equal(off, torch.tensor([0.0, 0.0, 1.0, 0.0]).expand(512, 4))
    on = draw_augmentation(512, _cfg([1.0, 1.0, 1.0]), g, device="cpu")
    assert bool((on[:, 0] == 1).all()) and bool((on[:, 3] == 1).all())
    bound = math.pi / 18
    assert float(on[:, 1].abs().max()) <= bound and float(on[:, 1].min()) < -0.5 * bound and float(on[:, 1].max()) > 0.5 * bound
    assert float(on[:, 2].min()) >= 0.95 and float(on[:, 2].max()) <= 1.05 and float(on[:, 2].min()) < 0.96 and float(on[:, 2].max()) > 1.04
    half = draw_augmentation(4096, _cfg([0.5, 0.25, 0.75]), g, device="cpu")
    share = [float(half[:, 0].mean()), float((half[:, 2] != 1).float().mean()), float(half[:, 3].mean())]
    assert all(abs(s - p) < 0.04 for s, p in zip(share, (0.5, 0.25, 0.75))), share        # 4 sigma of a share of 4096 is 0.031
    assert bool((half[:, 1][half[:, 0] == 0] == 0).all())
    wide = draw_augmentation(512, _cfg([1.0, 1.0, 1.0], rot_range=6), g, device="cpu")
    assert bound < float(wide[:, 1].abs().max()) <= math.pi / 6
    for k, name in enumerate(("rotation", "scaling", "flip")):
        rest = [m for m in ("rotation", "scaling", "flip") if m != name]
        t = draw_augmentation(256, _cfg([1.0, 1.0, 1.0], rest), g, device="cpu")
        col = (t[:, 0], (t[:, 2] != 1).float(), t[:, 3])
        assert float(col[k].sum()) == 0 and all(float(col[j].mean()) > 0.99 for j in range(3) if j != k)
        assert name != "rotation" or float(t[:, 1].abs().max()) == 0


def test_draw_augmentation_reads_the_reference_config_when_loaded(monkeypatch):
    import sys
    import types
    from epnet_amd.rpn_target_layer import draw_augmentation
    mod = types.ModuleType("lib.config")
    mod.cfg = _cfg([0.0, 0.0, 1.0])
    monkeypatch.setitem(sys.modules, "lib.config", mod)
    t = draw_augmentation(64, generator=torch.Generator().manual_seed(1), device="cpu")
    assert float(t[:, 0].sum()) == 0 and bool((t[:, 2] == 1).all()) and float(t[:, 3].mean()) > 0.95

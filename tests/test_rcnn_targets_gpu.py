"""The sync-free RCNN training targets on the GPU (epnet_amd/rcnn_target_layer.py over csrc/rcnn_targets.hip and csrc/roipool3d.hip).

Bounds. The selection is compared BIT FOR BIT with the numpy restatement (tests/rcnn_targets_restate.py, held to the existing
layer in test_rcnn_targets.py) fed with the matrix of ``boxes_iou3d_gpu`` on the same inputs: both sides decide on the same floats,
so no ROI is excluded for sitting near a threshold. ``max_overlaps`` against the CPU oracle: the project's 1e-5. The pooled targets
against the reference's own results (tests/golden/proposal_target.npz) and against the float64 restatement: rtol 1e-5, atol 5e-5
(``check_forward``'s), the choice of rows, the flags and the labels exact. Between runs and streams: bit-equal."""
import numpy as np
import pytest
import torch

from conftest import golden

import rcnn_targets_restate as rs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F = np.float32
THRESH = dict(fg_thresh=0.55, bg_thresh=0.45, bg_thresh_lo=0.05, hard_bg_ratio=0.8)


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def host(t):
    return t.detach().cpu().numpy()


def cfg_of(per_image, aug_times=10, num_points=512):
    from epnet_amd import rcnn_target_layer as rtl
    cfg = rtl.default_cfg()
    cfg.RCNN.ROI_PER_IMAGE, cfg.RCNN.ROI_FG_AUG_TIMES, cfg.RCNN.NUM_POINTS = per_image, aug_times, num_points
    return cfg


# ---- scenes with a chosen mix of classes ------------------------------------------------------------------------------------------
# A ROI is its ground-truth box moved d metres along the box's own length axis (l = 3.9): IoU ~ (3.9 - d) / (3.9 + d)
SHIFT = {"fg": (0.0, 0.6), "mid": (1.22, 1.38), "hard": (1.7, 3.3), "easy": (4.5, 7.0)}
KINDS = {"both_many": dict(fg=0.6, hard=0.25, easy=0.15), "both_few": dict(fg=0.04, hard=0.5, easy=0.46), "fg_only": dict(fg=1.0),
         "bg_only": dict(hard=0.5, easy=0.5), "only_hard": dict(hard=1.0), "only_easy": dict(easy=1.0), "neither": dict(mid=1.0),
         "fg_and_mid": dict(fg=0.5, mid=0.5), "no_gt": dict(easy=1.0)}
CASE_OF = {"both_many": 0, "both_few": 0, "fg_only": 1, "bg_only": 2, "only_hard": 2, "only_easy": 2, "neither": 3, "fg_and_mid": 1, "no_gt": 2}


def make_scene(m, g, gc, kind, rng):
    """-> rois (m,7), gt (g,gc): real boxes 25 m apart with an interior zero row and trailing padding where g allows"""
    gt = np.zeros((g, gc))
    real = [0] if g < 3 else [k for k in range(g - max(1, g // 4)) if k != 1]      # row 1 zero (interior), the last quarter padding
    if kind != "no_gt":
        for k in real:
            gt[k, 0:7] = (-40 + 25.0 * (k % 4) + rng.uniform(-2, 2), rng.uniform(1.2, 2.0), 12 + 14.0 * (k // 4) + rng.uniform(-2, 2),
                          rng.uniform(1.4, 1.7), rng.uniform(1.5, 1.7), 3.9, rng.uniform(-np.pi, np.pi))
            if gc > 7:
                gt[k, 7:] = rng.randint(1, 4, gc - 7)
        if gc > 7 and g >= 3:
            gt[real[-1] + 1, 7] = 2.0                                             # a zero box whose class column counts it as a row (:105)
    mix = KINDS[kind]
    names = list(mix)
    counts = [int(round(mix[n] * m)) for n in names]
    counts[int(np.argmax(counts))] += m - sum(counts)
    if kind.startswith("both") and m >= 3:                                       # both kinds really present
        for i, n in enumerate(names):
            if counts[i] == 0:
                counts[i] += 1
                counts[int(np.argmax(counts))] -= 1
    classes = rng.permutation(np.repeat(names, counts))
    rois = np.zeros((m, 7))
    for i, c in enumerate(classes):
        box = gt[real[rng.randint(len(real))], 0:7] if kind != "no_gt" else np.array([0, 1.6, 20, 1.5, 1.6, 3.9, 0.2])
        d = rng.uniform(*SHIFT[c]) * (1 if rng.rand() < 0.5 else -1)
        rois[i] = box
        rois[i, 0] += d * np.cos(box[6])
        rois[i, 2] -= d * np.sin(box[6])
    return rois.astype(F), gt.astype(F)


def make_tables(b, m, r, rng, ties):
    fg_key, slot_u = rng.rand(b, m).astype(F), rng.rand(b, r).astype(F)
    if ties:
        fg_key = (np.floor(fg_key * 4) / 4).astype(F)                           # many equal keys: the order falls to the ROI index
        fg_key[:, ::7] = -0.0
        fg_key[:, 3::7] = 0.0
    slot_u[:, ::5] = 0.0                                                          # the ends of the range
    slot_u[:, 2::5] = F(1) - F(2.0 ** -24)
    return fg_key, slot_u


def gpu_matrix(rois, gt):
    """-> iou_of(scene, num_gt) over boxes_iou3d_gpu, the existing op, on the same inputs"""
    from epnet_amd import iou3d_utils

    def iou_of(k, num_gt):
        return host(iou3d_utils.boxes_iou3d_gpu(dev(rois[k]), dev(np.ascontiguousarray(gt[k, :num_gt, 0:7]))))
    return iou_of


def run_sampling(rois, gt, fg_key, slot_u, cfg, keep=None, noise=None):
    from epnet_amd import rcnn_target_layer as rtl
    tables = {"fg_key": dev(fg_key), "slot_u": dev(slot_u), "keep_draw": keep, "noise": noise}
    out = rtl.sample_rois(dev(rois), dev(gt), tables, cfg, details=True)
    torch.cuda.synchronize()
    return out


def identity_noise(k, t):
    if t == 0:
        return None, None
    return torch.ones((k, t), dtype=torch.uint8, device=DEV), torch.zeros((k, t, 7), device=DEV)


#        B  M    G   gc R    T   scene kinds                                              equal keys
CASES = [(1, 1, 1, 7, 1, 0, ("fg_only",), False),
         (1, 1, 1, 7, 16, 10, ("only_easy",), False),
         (3, 63, 8, 7, 16, 10, ("both_many", "bg_only", "fg_only"), False),
         (3, 64, 20, 8, 64, 1, ("both_few", "neither", "no_gt"), True),
         (5, 65, 8, 16, 100, 10, ("both_many", "only_hard", "only_easy", "fg_and_mid", "both_few"), True),
         (1, 128, 65, 7, 64, 0, ("both_many",), False),
         (3, 257, 20, 7, 16, 10, ("neither", "both_many", "no_gt"), True),
         (1, 512, 20, 7, 64, 10, ("both_many",), False),
         (3, 513, 65, 9, 100, 1, ("both_few", "both_many", "fg_only"), True),
         (5, 512, 1, 7, 1, 0, ("both_many", "bg_only", "fg_only", "neither", "no_gt"), False),
         (1, 4096, 8, 7, 1024, 10, ("both_many",), True),
         (3, 1100, 3, 7, 64, 64, ("both_many", "both_few", "only_hard"), False),
         (3, 65, 300, 7, 16, 10, ("both_many", "bg_only", "no_gt"), False)]           # G >= 256: one ROI per workgroup in the IoU phase


def test_cases_cover_the_shapes():
    assert {c[1] for c in CASES} >= {1, 63, 64, 65, 128, 257, 512, 513} and {c[2] for c in CASES} >= {1, 8, 20, 65, 300}
    assert {c[4] for c in CASES} >= {1, 16, 64, 100} and {c[0] for c in CASES} >= {1, 3, 5} and {c[5] for c in CASES} >= {0, 1, 10}
    assert any(c[1] < c[4] for c in CASES) and any(c[1] > c[4] for c in CASES)
    assert {k for c in CASES for k in c[6]} >= set(KINDS) and {c[3] for c in CASES} >= {7, 8, 16}


@pytest.mark.parametrize("b,m,g,gc,r,t,kinds,ties", CASES)
def test_selection_bit_for_bit(hiplib, b, m, g, gc, r, t, kinds, ties):
    rng = np.random.RandomState(1000 * m + 10 * g + r + t)
    scenes = [make_scene(m, g, gc, kind, rng) for kind in kinds]
    rois, gt = np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes])
    fg_key, slot_u = make_tables(b, m, r, rng, ties)
    cfg = cfg_of(r, t)
    fg_per_image = int(np.round(0.5 * r))
    keep, noise = identity_noise(b * r, t)
    got_rois, got_gt, got_iou, info, d = run_sampling(rois, gt, fg_key, slot_u, cfg, keep, noise)
    want = rs.sample(rois, gt, gpu_matrix(rois, gt), fg_key, slot_u, r, fg_per_image, aug_times=t, **THRESH)
    print("scene_info", host(info).tolist())
    assert host(info).tolist() == want["scene_info"].tolist()
    # the generator made the scenes it was asked for (a statement about the inputs)
    for k, kind in enumerate(kinds):
        expect = CASE_OF[kind] if m >= 3 or not kind.startswith("both") else want["scene_info"][k, 5]
        assert want["scene_info"][k, 5] == expect, (k, kind, want["scene_info"][k].tolist())
        assert (want["scene_info"][k, 0] == 0) == (kind == "no_gt")
    assert host(d["max_overlaps"]).tobytes() == want["max_overlaps"].tobytes()
    for key in ("gt_assignment", "src_inds", "tries"):
        assert host(d[key]).dtype == np.int32 and np.array_equal(host(d[key]), want[key]), key
    assert host(d["iou_src"]).tobytes() == want["iou_src"].tobytes()
    assert host(got_rois).tobytes() == want["batch_rois"].tobytes()             # identity noise: the gathered rows themselves
    assert host(got_gt).tobytes() == want["batch_gt_of_rois"].tobytes()
    assert host(got_iou).tobytes() == want["iou_src"].tobytes()
    fg_this = want["scene_info"][:, 4]
    tied = [k for k in range(b) if ties and want["scene_info"][k, 5] == 0 and fg_this[k] > 6]
    if tied:                                                                      # equal keys were really among the chosen ones
        assert any(len(set(fg_key[k][want["src_inds"][k][:fg_this[k]]].tolist())) < fg_this[k] for k in tied)


def test_outputs_without_the_optional_ones_are_the_same(hiplib):
    """the optional outputs live in the workspace when they are not asked for: same required outputs"""
    from epnet_amd import rcnn_target_layer as rtl
    rng = np.random.RandomState(5)
    rois, gt = (np.stack(v) for v in zip(*[make_scene(300, 8, 7, k, rng) for k in ("both_many", "both_few")]))
    fg_key, slot_u = make_tables(2, 300, 64, rng, False)
    cfg = cfg_of(64, 10)
    keep, noise = rtl.draw_aug_tables(2 * 64, 10, "multiple", DEV, torch.Generator(device=DEV).manual_seed(3))
    full = run_sampling(rois, gt, fg_key, slot_u, cfg, keep, noise)
    plain = rtl.sample_rois(dev(rois), dev(gt), {"fg_key": dev(fg_key), "slot_u": dev(slot_u), "keep_draw": keep, "noise": noise}, cfg)
    assert all(torch.equal(a, b) for a, b in zip(full[:4], plain))


# ---- the noise loop ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 10, 70])
def test_noise_loop_equals_the_batched_op(hiplib, t):
    """with real noise tables: batch_rois / batch_roi_iou = aug_roi_by_noise_batched on the gathered rows, bit for bit"""
    from epnet_amd import proposal_target_layer as ptl
    rng = np.random.RandomState(40 + t)
    kinds = ("both_many", "both_few", "fg_only")
    rois, gt = (np.stack(v) for v in zip(*[make_scene(200, 8, 7, k, rng) for k in kinds]))
    fg_key, slot_u = make_tables(3, 200, 64, rng, False)
    cfg = cfg_of(64, t)
    keep, noise = ptl.draw_aug_tables(3 * 64, t, "multiple", DEV, torch.Generator(device=DEV).manual_seed(t))
    got_rois, got_gt, got_iou, info, d = run_sampling(rois, gt, fg_key, slot_u, cfg, keep, noise)
    gathered = torch.gather(dev(rois), 1, d["src_inds"].long().unsqueeze(2).expand(-1, -1, 7)).contiguous().view(-1, 7)
    want_rois, want_iou = ptl.aug_roi_by_noise_batched(gathered, got_gt.view(-1, 7), d["iou_src"].view(-1), 0.55, keep, noise, d["tries"].view(-1))
    assert torch.equal(got_rois.view(-1, 7), want_rois) and torch.equal(got_iou.view(-1), want_iou)
    assert not torch.equal(got_iou, d["iou_src"]) and int((got_iou >= 0.55).sum()) > 0          # the loop did something


# ---- against the CPU oracle -------------------------------------------------------------------------------------------------------
def test_max_overlaps_against_the_oracle(hiplib, oracle):
    rng = np.random.RandomState(9)
    kinds = ("both_many", "both_few", "neither")
    rois, gt = (np.stack(v) for v in zip(*[make_scene(257, 20, 7, k, rng) for k in kinds]))
    fg_key, slot_u = make_tables(3, 257, 16, rng, False)
    d = run_sampling(rois, gt, fg_key, slot_u, cfg_of(16, 0))[4]
    for k in range(3):
        num_gt = rs.count_gt(gt[k])
        want = oracle.boxes_iou3d(rois[k], np.ascontiguousarray(gt[k, :num_gt, 0:7])).max(axis=1)
        np.testing.assert_allclose(host(d["max_overlaps"])[k], want, rtol=0, atol=1e-5)


# ---- epnet_roipool3d_train ----------------------------------------------------------------------------------------------------------
TOL = dict(rtol=1e-5, atol=5e-5)      # check_forward's (tests/test_proposal_target.py)


def small_cfg():
    from epnet_amd import rcnn_target_layer as rtl
    cfg = rtl.default_cfg()
    cfg.RCNN.NUM_POINTS, cfg.RCNN.ROI_PER_IMAGE = 32, 16
    return cfg


def test_train_pooling_against_the_reference(hiplib):
    """the golden's forward pass: its sampled rows and draws in, every fwd__out_ key out"""
    from epnet_amd import rcnn_target_layer as rtl
    fx = golden("proposal_target.npz")
    cfg = small_cfg()
    feat = torch.cat([dev(fx["fwd__in_seg_mask"]).unsqueeze(2), (dev(fx["fwd__in_pts_depth"]) / 70.0 - 0.5).unsqueeze(2),
                      dev(fx["fwd__in_rpn_features"])], dim=2)
    aug = rtl.aug_table_from_draws(*[dev(u) for u in fx["fwd__draws"]], cfg)
    out = rtl.pool_targets(dev(fx["fwd__in_rpn_xyz"]), feat, dev(fx["fwd__sampled_rois"]), dev(fx["fwd__sampled_gt"]),
                           dev(fx["fwd__sampled_iou"]), aug, cfg)
    out["gt_iou"] = dev(fx["fwd__sampled_iou"]).view(-1)
    out.pop("pooled_empty_flag")
    assert sorted(out) == sorted(k[len("fwd__out_"):] for k in fx.files if k.startswith("fwd__out_"))
    for key, val in out.items():
        want = fx["fwd__out_" + key]
        assert tuple(val.shape) == want.shape, key
        if val.dtype == torch.int32:
            np.testing.assert_array_equal(host(val), want, err_msg=key)
        else:
            print(key, "max abs difference %.3e" % float(np.abs(host(val).astype(np.float64) - want).max()))
            np.testing.assert_allclose(host(val), want, err_msg=key, **TOL)


def train_inputs(b, n, r, c, seed, with_aug):
    from detections_restate import pooling_inputs
    from epnet_amd import rcnn_target_layer as rtl
    xyz, rois, feat = pooling_inputs(b, n, r, c, seed)
    rng = np.random.RandomState(seed)
    rois, xyz = rois.numpy().copy(), xyz.numpy()
    rois[:, :, 6] = rng.uniform(0.2, 2.9, (b, r)) * np.where(rng.rand(b, r) < 0.5, -1, 1)     # clear of the mod 2 pi seam, see the docstring
    lim = np.maximum((rois[:, :, 2] - 0.5) / 0.2, 0)                                           # z > 0.2 |x|: atan2(z, x) keeps its sign under the rotation
    rois[:, :, 0] = np.clip(rois[:, :, 0], -lim, lim)
    rois[0, 0, 0:3] = (2.0, -30.0, 35.0)                                                       # an empty ROI in any case: far above the cloud
    gt = rois + rng.normal(size=rois.shape).astype(F) * np.array([0.3, 0.1, 0.3, 0.05, 0.05, 0.1, 0.2], F)
    gt[:, :, 6] = rng.uniform(-np.pi, np.pi, (b, r))
    iou = rng.rand(b, r).astype(F)
    iou[:, ::4] = np.array([0.45, 0.55, 0.6, 0.61], F)[rng.randint(0, 4, iou[:, ::4].shape)]   # on the thresholds: strict comparisons
    aug = None
    if with_aug:
        g = torch.Generator().manual_seed(seed)
        aug = rtl.aug_table_from_draws(*[torch.rand((b, r), generator=g) for _ in range(3)], rtl.default_cfg()).numpy()
    return xyz, feat.numpy(), rois.astype(F), gt.astype(F), iou, aug


@pytest.mark.parametrize("b,n,r,s,c,with_aug", [(1, 1, 3, 1, 1, True), (2, 64, 16, 32, 5, True), (2, 2048, 16, 512, 130, True), (3, 2048, 7, 32, 1, False),
                                                (1, 64, 5, 512, 130, False), (2, 2048, 64, 1, 5, True)])
def test_train_pooling_against_the_restatement(hiplib, b, n, r, s, c, with_aug):
    """ROI ry is drawn from +-[0.2, 2.9] and the rotation adds -angle in (0, pi / 18], a flip maps ry to sign(ry) pi - ry: the
    augmented ry stays at least 0.02 away from 0 and from +-pi, where a rounding of ry could change ry mod 2 pi by 2 pi"""
    from epnet_amd import rcnn_target_layer as rtl
    xyz, feat, rois, gt, iou, aug = train_inputs(b, n, r, c, 31 * n + s + c, with_aug)
    cfg = cfg_of(r, 10, s)
    out = rtl.pool_targets(dev(xyz), dev(feat), dev(rois), dev(gt), dev(iou), None if aug is None else dev(aug), cfg)
    torch.cuda.synchronize()
    want = rs.pool_train(xyz, feat, rois, gt, iou, aug, 0.2, 0.55, 0.6, 0.45, s, precise=True)
    flag = host(out["pooled_empty_flag"])
    assert flag.dtype == np.int32 and np.array_equal(flag, want["pooled_empty_flag"]) and flag[0, 0] == 1
    assert n < 64 or (flag == 0).sum() >= 2                                       # some ROIs hold points
    assert host(out["pts_feature"]).tobytes() == want["pts_feature"].tobytes()    # the choice of rows: exact copies
    for key in ("cls_label", "reg_valid_mask"):
        assert host(out[key]).dtype == np.int32 and np.array_equal(host(out[key]), want[key]), key
    assert (host(out["cls_label"])[flag.reshape(-1) == 1] == -1).all() and not host(out["mask_score"])[flag.reshape(-1) == 1].any()
    ry = want["roi_boxes3d"][:, 6]
    assert np.abs(ry).min() > 0.02 and np.abs(np.abs(ry) - np.pi).min() > 0.02
    for key in ("sampled_pts", "roi_boxes3d", "gt_of_rois", "mask_score"):
        got = host(out[key])
        assert got.shape == want[key].shape, key
        print(key, "max abs difference %.3e" % float(np.abs(got.astype(np.float64) - want[key]).max()))
        np.testing.assert_allclose(got, want[key], err_msg=key, **TOL)
    if aug is None:                                                               # no augmentation step: the boxes as given
        assert host(out["roi_boxes3d"]).tobytes() == rois.reshape(-1, 7).tobytes()


# ---- the whole layer --------------------------------------------------------------------------------------------------------------
def layer_inputs(b, m, n, seed):
    from epnet_amd import synth
    g = torch.Generator().manual_seed(seed)
    rois, gts = [], []
    for i in range(b):
        boxes, _ = synth.proposal_boxes(m + 12, seed=seed + i, num_objects=12, jitter=0.4)
        gt = torch.zeros((20, 7))
        gt[:12] = boxes[m:]
        rois.append(boxes[:m])
        gts.append(gt)
    return {"roi_boxes3d": torch.stack(rois).to(DEV), "gt_boxes3d": torch.stack(gts).to(DEV),
            "rpn_xyz": synth.scenes("kitti", b, n, seed=seed).to(DEV), "rpn_features": torch.randn((b, n, 128), generator=g).to(DEV),
            "seg_mask": (torch.rand((b, n), generator=g) > 0.5).float().to(DEV), "pts_depth": (torch.rand((b, n), generator=g) * 70).to(DEV)}


def fixed_tables(b, m, cfg, seed):
    """-> (tables, the three data_augmentation draws the aug table was made from)"""
    from epnet_amd import rcnn_target_layer as rtl
    g = torch.Generator(device=DEV).manual_seed(seed)
    tables = rtl.draw_sampling_tables(b, m, cfg, DEV, g)
    draws = [torch.rand((b, cfg.RCNN.ROI_PER_IMAGE), device=DEV, generator=g) for _ in range(3)]
    tables["aug"] = rtl.aug_table_from_draws(*draws, cfg)
    return tables, draws


def test_layer_equals_sampling_plus_the_existing_tail(hiplib):
    """RCNNTargetLayer with fixed tables = sample_rois, then the EXISTING layer's forward tail fed with the same draws"""
    from epnet_amd import proposal_target_layer as ptl, rcnn_target_layer as rtl
    b, m, n = 2, 512, 4096
    cfg = cfg_of(64, 10, 128)
    inputs = layer_inputs(b, m, n, 200)
    tables, draws = fixed_tables(b, m, cfg, 11)
    got = rtl.RCNNTargetLayer(cfg, label_dtype=torch.int64)(inputs, tables)
    got32 = rtl.RCNNTargetLayer(cfg)(inputs, tables)
    sampled = rtl.sample_rois(inputs["roi_boxes3d"], inputs["gt_boxes3d"], tables, cfg)
    old = ptl.ProposalTargetLayer(cfg)
    old.sample_rois_for_rcnn = lambda r, g: tuple(t.clone() for t in sampled[:3])
    real_da = old.data_augmentation
    old.data_augmentation = lambda p, r, g: real_da(p, r, g, draws)
    want = old(inputs)
    assert sorted(got) == sorted(list(want) + ["scene_info"])
    assert torch.equal(got["scene_info"], sampled[3]) and int(got["scene_info"][:, 1].min()) > 0
    for key, val in want.items():
        assert got[key].shape == val.shape and got[key].dtype == val.dtype, key
        if val.dtype == torch.int64:
            assert torch.equal(got[key], val), key
            assert got32[key].dtype == torch.int32 and torch.equal(got32[key].long(), val), key
        else:
            print(key, "max abs difference %.3e" % float((got[key] - val).abs().max()))
            np.testing.assert_allclose(host(got[key]), host(val), err_msg=key, **TOL)
            assert torch.equal(got32[key], got[key]), key
    assert set(got["cls_label"].unique().tolist()) == {-1, 0, 1} and int(got["reg_valid_mask"].sum()) > 0
    # without tables the layer draws its own: same shapes, another selection
    own = rtl.RCNNTargetLayer(cfg, generator=torch.Generator(device=DEV).manual_seed(1))(inputs)
    assert own["sampled_pts"].shape == got["sampled_pts"].shape and not torch.equal(own["roi_boxes3d"], got["roi_boxes3d"])


def test_runs_are_bit_equal(hiplib):
    """twice on one stream and once on a side stream"""
    from epnet_amd import rcnn_target_layer as rtl
    cfg = cfg_of(64, 10, 512)
    inputs = layer_inputs(2, 512, 16384, 300)
    tables, _ = fixed_tables(2, 512, cfg, 12)
    layer = rtl.RCNNTargetLayer(cfg)
    a, b = layer(inputs, tables), layer(inputs, tables)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = layer(inputs, tables)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for key in a:
        assert host(a[key]).tobytes() == host(b[key]).tobytes() == host(c[key]).tobytes(), key
    assert tuple(a["sampled_pts"].shape) == (128, 512, 3) and tuple(a["pts_feature"].shape) == (128, 512, 130)


# ---- one graph with the RCNN stage and its loss -----------------------------------------------------------------------------------------
def differing(xs, ys):
    """the names of the outputs (dicts of tensors with the same keys) that are not bit-equal, with the largest difference"""
    assert list(xs) == list(ys)
    return [(k, float((xs[k].float() - ys[k].float()).abs().max())) for k in xs if not torch.equal(xs[k], ys[k])]


@pytest.fixture()
def deterministic_gradients():
    """the library's default scatter-add gradients use float atomics (1e-5 against the oracle, not bit-reproducible); under
    torch's deterministic mode the stand-ins take the *_det entry points, whose bits depend on the inputs alone (INTEGRATION.md,
    "Reproducible gradients") -- what a bit-for-bit comparison of a backward pass needs"""
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(prev)


def test_targets_rcnn_stage_and_loss_in_one_graph(hiplib, deterministic_gradients):
    """RCNNTargetLayer.forward + the RCNN stage of bench_step's model + rcnn_loss, forward and backward, captured in ONE
    torch.cuda.graph on a single stream (the capture fails on any synchronisation with the host -- the existing layer's two
    read-backs cannot be captured), replayed after the static inputs and tables were rewritten, against eager runs: bit-equal"""
    import bench_step
    from epnet_amd import loss_utils, rcnn_target_layer as rtl
    torch.manual_seed(0)
    b, m, n = 2, 128, 2048
    cfg = cfg_of(16, 10, 512)
    model = bench_step.build_model(scale=8, loss="reference").to(DEV)
    rcnn = model.rcnn
    params = [p for p in rcnn.parameters() if p.requires_grad]
    static = layer_inputs(b, m, n, 400)
    tables, _ = fixed_tables(b, m, cfg, 13)
    second, second_tables = layer_inputs(b, m, n, 500), fixed_tables(b, m, cfg, 14)[0]
    layer = rtl.RCNNTargetLayer(cfg)
    loss_cfg = loss_utils.default_cfg()

    def step():
        with torch.no_grad():
            target = layer(static, tables)
        rcnn_cls, rcnn_reg = rcnn(target["sampled_pts"], target["pts_feature"])
        out = loss_utils.rcnn_loss(dict(target, rcnn_cls=rcnn_cls.view(rcnn_cls.shape[0], -1), rcnn_reg=rcnn_reg.view(rcnn_reg.shape[0], -1)), loss_cfg)
        grads = torch.autograd.grad(out.loss, params, allow_unused=True)
        named = {"target." + k: v for k, v in target.items()}
        named.update(rcnn_cls=rcnn_cls, rcnn_reg=rcnn_reg, loss=out.loss, terms=out.terms)
        named.update({"grad.%d" % i: g for i, g in enumerate(grads) if g is not None})
        return named
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    eager_first = {k: t.clone() for k, t in step().items()}
    print("outputs that differ between the replay and the eager run:", differing(eager_first, captured))
    grad_names = [k for k in captured if k.startswith("grad.")]
    assert len(grad_names) >= 10 and "target.scene_info" in captured and not differing(eager_first, captured)
    assert bool(torch.isfinite(captured["terms"]).all()) and all(bool(torch.isfinite(captured[k]).all()) for k in grad_names)
    assert float(eager_first[grad_names[0]].abs().sum()) > 0
    with torch.no_grad():
        for key in static:
            static[key].copy_(second[key])
        for key in tables:
            tables[key].copy_(second_tables[key])
    graph.replay()
    torch.cuda.synchronize()
    eager_second = step()
    print("after the rewrite:", differing(eager_second, captured))
    assert not differing(eager_second, captured)
    changed = [k for k, _ in differing(eager_second, eager_first)]
    assert "target.roi_boxes3d" in changed and "terms" in changed and grad_names[0] in changed          # the replay saw the new inputs


def test_layer_with_its_own_tables_does_not_synchronise(hiplib):
    """the default path, tables=None: drawing the tables and both calls run with torch's synchronisation check on 'error' (it
    raises on a blocking copy or a read-back), and the same call records into a graph"""
    from epnet_amd import rcnn_target_layer as rtl
    cfg = cfg_of(16, 10, 64)
    inputs = layer_inputs(2, 128, 2048, 700)
    layer = rtl.RCNNTargetLayer(cfg, generator=None)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        layer(inputs)                                                           # warm the allocator
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = layer(inputs)
        tables = rtl.draw_sampling_tables(2, 128, cfg, DEV)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert tuple(out["sampled_pts"].shape) == (32, 64, 3) and tables["noise"].shape == (32, 10, 7) and tables["aug"] is not None
    # the check does bite: a read-back raises under it
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            out["gt_iou"].sum().item()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = layer(inputs)
    graph.replay()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(captured["sampled_pts"]).all()) and set(captured["cls_label"].unique().tolist()) <= {-1, 0, 1}
    assert bool((captured["scene_info"][:, 0] == 12).all())


# ---- limits -------------------------------------------------------------------------------------------------------------------------
def test_limits_are_refused_before_any_launch(hiplib):
    from epnet_amd import _lib, iou3d_cuda, roipool3d_cuda
    fill = lambda shape, dtype=torch.float32: torch.full(shape, 7, dtype=dtype, device=DEV)  # noqa: E731
    i32 = torch.int32

    def call(b, m, g, gc, r, fg=None, **kw):
        outs = [fill((b, r, 7)), fill((b, r, 7)), fill((b, r)), fill((b, 6), i32)]
        opt = dict(src_inds=fill((b, r), i32), iou_src=fill((b, r)), tries=fill((b, r), i32), max_overlaps=fill((b, m)), gt_assignment=fill((b, m), i32))
        iou3d_cuda.rcnn_sample_rois_gpu(torch.zeros((b, m, 7), device=DEV), torch.zeros((b, g, gc), device=DEV), torch.zeros((b, m), device=DEV),
                                        torch.zeros((b, r), device=DEV), None, None, r // 2 if fg is None else fg, 0.55, 0.45, 0.05, 0.8, *outs, **opt, **kw)
        torch.cuda.synchronize()
        return outs + list(opt.values())
    for shape in ((1, 4097, 2, 7, 16), (1, 64, 2, 7, 1025), (65536, 1, 1, 7, 1)):
        with pytest.raises(_lib.EpnetError, match="supported range"):
            call(*shape)
    for shape, fg in (((1, 64, 2, 6, 16), None), ((1, 64, 2, 17, 16), None), ((1, 64, 2, 7, 16), 17)):
        with pytest.raises(_lib.EpnetError, match="invalid argument"):
            call(*shape, fg=fg)
    # a refused call writes nothing
    outs = [fill((1, 16, 7)), fill((1, 16, 7)), fill((1, 16)), fill((1, 6), i32)]
    with pytest.raises(_lib.EpnetError):
        iou3d_cuda.rcnn_sample_rois_gpu(torch.zeros((1, 4097, 7), device=DEV), torch.zeros((1, 2, 7), device=DEV), torch.zeros((1, 4097), device=DEV),
                                        torch.zeros((1, 16), device=DEV), None, None, 8, 0.55, 0.45, 0.05, 0.8, *outs)
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)
    # too small a workspace, straight at the C ABI
    l = _lib.lib()
    need = l.epnet_rcnn_sample_rois_workspace_bytes(1, 64, 2, 16)
    ws = fill((need,), torch.uint8)
    z = lambda *s: torch.zeros(s, device=DEV)  # noqa: E731
    ins = [z(1, 64, 7), z(1, 2, 7), z(1, 64), z(1, 16)]
    outs = [fill((1, 16, 7)), fill((1, 16, 7)), fill((1, 16)), fill((1, 6), i32)]
    args = [1, 64, 2, 7, 16, 8, 0.55, 0.45, 0.05, 0.8, 0] + [t.data_ptr() for t in ins] + [None, None, ws.data_ptr()]
    assert l.epnet_rcnn_sample_rois(*args, need - 1, *[t.data_ptr() for t in outs], None, None, None, None, None, None) == -3
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs) and bool((ws == 7).all())
    assert l.epnet_rcnn_sample_rois(*args, need, *[t.data_ptr() for t in outs], None, None, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert outs[3].tolist() == [[0, 0, 0, 64, 0, 2]] and not bool((outs[0] == 7).any())     # no ground truth: easy background, defined
    # the largest shapes run; b == 0 is a no-op
    big = call(1, 4096, 1, 16, 1024)
    assert big[3].tolist() == [[0, 0, 0, 4096, 0, 2]] and not any(bool((o == 7).any()) for o in big[:3] + big[4:])
    none = call(0, 64, 2, 7, 16)
    assert all(o.numel() == 0 or bool((o == 7).all()) for o in none)
    with pytest.raises(RuntimeError, match="alias slot_u"):
        u = z(1, 16)
        iou3d_cuda.rcnn_sample_rois_gpu(z(1, 16, 7), z(1, 2, 7), z(1, 16), u, None, None, 8, 0.55, 0.45, 0.05, 0.8, fill((1, 16, 7)), fill((1, 16, 7)), u,
                                        fill((1, 6), i32))
    with pytest.raises(RuntimeError, match="fg_key must be"):
        iou3d_cuda.rcnn_sample_rois_gpu(z(1, 16, 7), z(1, 2, 7), z(16), z(1, 16), None, None, 8, 0.55, 0.45, 0.05, 0.8, fill((1, 16, 7)), fill((1, 16, 7)),
                                        fill((1, 16)), fill((1, 6), i32))
    with pytest.raises(RuntimeError, match="alias"):
        r = z(1, 16, 7)
        iou3d_cuda.rcnn_sample_rois_gpu(r, z(1, 2, 7), z(1, 16), z(1, 16), None, None, 8, 0.55, 0.45, 0.05, 0.8, r, fill((1, 16, 7)), fill((1, 16)), fill((1, 6), i32))
    # the pooling: S beyond the LDS bound and B beyond the grid are refused, nothing written
    s_max = 150 * 1024 // 20
    for b, s in ((1, s_max + 1), (65536, 1)):
        outs = [fill((b * 1, s, 3)), fill((b * 1, s, 1)), fill((b, 7)), fill((b, 7)), fill((b,), i32), fill((b,), i32), fill((b,)), fill((b, 1), i32)]
        with pytest.raises(_lib.EpnetError, match="supported range"):
            roipool3d_cuda.forward_train(z(b, 4, 3), z(b, 4, 1), z(b, 1, 7), z(b, 1, 7), z(b, 1), None, 0.2, 0.55, 0.6, 0.45, *outs)
        torch.cuda.synchronize()
        assert all(bool((o == 7).all()) for o in outs)

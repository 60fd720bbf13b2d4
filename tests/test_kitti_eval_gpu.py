"""The KITTI AP evaluator on the GPU (epnet_amd/kitti_eval.py over csrc/kitti_eval.hip).

Bounds. Overlaps against the reference's run (tests/golden/kitti_eval.npz) and against the restatement: metric 0 bit-equal,
metrics 1 / 2 within 1e-5 absolute. The matching kernels are given the GPU's own overlaps and compared with the restatement's
literal loops on the same arrays: matched scores (NaN positions included) and tp / fp / fn equal, similarity within
n * 2^-52 * sum. End to end the nine ret_dict values are within 1e-9 of the reference's and the string is the same, which
rests on the margin condition (no overlap within 1e-4 of a min_overlap), asserted for every data set whose overlaps come from
two sources. Between runs and streams: bit-equal."""
import numpy as np
import pytest
import torch

import kitti_eval_cases as kc
import kitti_eval_restate as kr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FX = kc.load()
COMBOS = [(l, k) for l in range(3) for k in range(2)]   # difficulty x overlap row


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def offsets(counts, dtype=np.int32):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(dtype)


def gpu_blocks(gts, dts, metric):
    from epnet_amd import kitti_eval
    blocks, parted, n_dt, n_gt = kitti_eval.calculate_iou_partly(dts, gts, metric)   # eval.py:467: (dt, gt)
    assert parted is None and np.array_equal(n_dt, [len(d["name"]) for d in dts]) and np.array_equal(n_gt, [len(g["name"]) for g in gts])
    return blocks


def check_blocks(got, want, metric, what):
    worst = 0.0
    for f, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == np.float64, (what, f)
        if metric == 0:
            assert np.array_equal(a, b), (what, f)
        elif a.size:
            worst = max(worst, float(np.abs(a - b).max()))
    print("%s metric %d: max |diff| %.3e" % (what, metric, worst))
    assert worst <= kc.ROTATED_TOL, (what, metric, worst)


# ---- the packed device form of a data set, for direct calls of the two matching kernels -----------------------------------------
class Packed:
    def __init__(self, blocks, frames):
        """blocks: per-frame (dt, gt) overlaps; frames: per-frame dicts as kitti_eval_restate.prepare returns them, one list per
        difficulty"""
        self.frames, self.blocks = frames, blocks
        self.nd = [b.shape[0] for b in blocks]
        self.ng = [b.shape[1] for b in blocks]
        self.ndc = [len(fr["dc"]) for fr in frames[0]]
        f0 = frames[0]
        cat = lambda key, tail=(): np.concatenate([np.asarray(fr[key], np.float64).reshape((-1,) + tail) for fr in f0] + [np.zeros((0,) + tail)])  # noqa: E731
        self.gt_off, self.dt_off, self.dc_off = up(offsets(self.ng)), up(offsets(self.nd)), up(offsets(self.ndc))
        self.ov_off = up(offsets([a * b for a, b in zip(self.nd, self.ng)], np.int64))
        self.overlaps = up(np.concatenate([b.ravel() for b in blocks] + [np.zeros(0)]))
        self.dt_score, self.dt_alpha, self.gt_alpha = up(cat("dt_score")), up(cat("dt_alpha")), up(cat("gt_alpha"))
        self.dt_bbox, self.dc_bbox = up(cat("dt_bbox", (4,))), up(cat("dc", (4,)))
        self.ign_gt = up(np.stack([np.concatenate([fr["ignored_gt"] for fr in fl] + [np.zeros(0, np.int64)]) for fl in frames]).astype(np.int32))
        self.ign_dt = up(np.stack([np.concatenate([fr["ignored_dt"] for fr in fl] + [np.zeros(0, np.int64)]) for fl in frames]).astype(np.int32))
        self.total_gt, self.total_dt = sum(self.ng), sum(self.nd)

    def maxima(self):
        return max(self.ng + [0]), max(self.nd + [0]), max(self.ndc + [0])

    def match(self, combos, min_overlaps):
        from epnet_amd import kitti_eval_cuda, pointnet2_utils
        mg, md, _ = self.maxima()
        out = pointnet2_utils._new(self.overlaps, (len(combos), self.total_gt), torch.float64)
        kitti_eval_cuda.kitti_match_gpu(mg, md, [l for l, _ in combos], min_overlaps, self.gt_off, self.dt_off, self.ov_off, self.overlaps,
                                        self.dt_score, self.ign_gt, self.ign_dt, out)
        return out.cpu().numpy()

    def pr(self, combos, min_overlaps, thresholds, metric, compute_aos):
        """thresholds: one 1-d array per combination -> counts (C, T, 3), similarity (C, T)"""
        from epnet_amd import kitti_eval_cuda, pointnet2_utils
        mg, md, mdc = self.maxima()
        t = max(len(x) for x in thresholds)
        table = np.zeros((len(combos), t))
        for c, x in enumerate(thresholds):
            table[c, :len(x)] = x
        counts = pointnet2_utils._new(self.overlaps, (len(combos), t, 3), torch.int32)
        sims = pointnet2_utils._new(self.overlaps, (len(combos), t), torch.float64)
        kitti_eval_cuda.kitti_pr_gpu(mg, md, mdc, metric, compute_aos, [l for l, _ in combos], min_overlaps, [len(x) for x in thresholds],
                                     self.gt_off, self.dt_off, self.dc_off, self.ov_off, self.overlaps, self.dt_score, self.ign_gt,
                                     self.ign_dt, self.dt_bbox, self.dc_bbox, self.gt_alpha, self.dt_alpha, up(table), counts, sims)
        return counts.cpu().numpy(), sims.cpu().numpy()


def restated_match(p, l, min_overlap, metric):
    out = []
    for ov, fr in zip(p.blocks, p.frames[l]):
        r = kr.compute_statistics(ov, fr["gt_alpha"], fr["dt_alpha"], fr["dt_bbox"], fr["dt_score"], fr["ignored_gt"], fr["ignored_dt"],
                                  fr["dc"], metric, min_overlap, 0.0, False)
        out.append(r[5])
    return np.concatenate(out + [np.zeros(0)])


def restated_pr(p, l, min_overlap, thresholds, metric, compute_aos):
    pr, terms = np.zeros((len(thresholds), 4)), np.zeros(len(thresholds))
    for ov, fr in zip(p.blocks, p.frames[l]):
        for t, thresh in enumerate(thresholds):
            tp, fp, fn, sim, _, _, nt = kr.compute_statistics(ov, fr["gt_alpha"], fr["dt_alpha"], fr["dt_bbox"], fr["dt_score"],
                                                              fr["ignored_gt"], fr["ignored_dt"], fr["dc"], metric, min_overlap, thresh, True,
                                                              compute_aos)
            pr[t, :3] += (tp, fp, fn)
            if sim != -1:
                pr[t, 3] += sim
            terms[t] += nt
    return pr, terms


def check_matching(p, metric, min_overlaps, threshold_counts, combos=COMBOS):
    """pass 1 and pass 2 of a packed set against the literal loops, for each threshold count"""
    mins = [float(min_overlaps[k]) for _, k in combos]
    got = p.match(combos, mins)
    for c, (l, k) in enumerate(combos):
        want = restated_match(p, l, mins[c], metric)
        assert np.array_equal(np.isnan(got[c]), np.isnan(want)), ("sentinel positions", metric, l, k)
        assert np.array_equal(np.nan_to_num(got[c], nan=-1.0), np.nan_to_num(want, nan=-1.0)), ("matched scores", metric, l, k)
    scores = np.unique(p.dt_score.cpu().numpy())[::-1]
    for n in threshold_counts:   # thresholds that equal detection scores (eval.py:179 only ever sees such values)
        thr = scores[np.linspace(0, len(scores) - 1, n).astype(np.int64)] if n > 1 else scores[len(scores) // 2:len(scores) // 2 + 1]
        counts, sims = p.pr(combos, mins, [thr] * len(combos), metric, metric == 0)
        for c, (l, k) in enumerate(combos):
            want, terms = restated_pr(p, l, mins[c], thr, metric, metric == 0)
            assert np.array_equal(counts[c].astype(np.float64), want[:, :3]), ("tp/fp/fn", metric, l, k, n)
            bound = kc.similarity_bound(terms, want[:, 3])
            assert (np.abs(sims[c] - want[:, 3]) <= bound).all(), ("similarity", metric, l, k, n, sims[c] - want[:, 3], bound)


def packed_from_annos(gts, dts, blocks, current_class=0):
    return Packed(blocks, [kr.prepare(gts, dts, current_class, l)[0] for l in range(3)])


# ---- overlaps -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", ["a", "b"])
def test_overlaps_against_the_fixture_and_the_restatement(hiplib, prefix):
    gts, dts = kc.annos(FX, prefix + "_gt"), kc.annos(FX, prefix + "_dt")
    for metric in range(3):
        got = gpu_blocks(gts, dts, metric)
        check_blocks(got, kc.blocks(FX, "%s_overlaps_m%d" % (prefix, metric), gts, dts), metric, "reference " + prefix)
        check_blocks(got, kr.frame_overlaps(gts, dts, metric), metric, "restatement " + prefix)


# per-frame counts at the launch-geometry boundaries: a wave is 64 lanes, four waves share a frame's pairs
SMALL_DT = [63, 64, 65, 129, 0, 1, 2, 0, 5, 1, 3, 0]
SMALL_GT = [2, 1, 2, 1, 2, 0, 5, 0, 3, 1, 2, 1]
SMALL_DC = [0, 3, 0, 2, 1, 0, 4, 2, 0, 0, 1, 0]


def small_set(frames, seed):
    return kc.generated(frames, SMALL_DT if frames > 2 else SMALL_DT[2:], SMALL_GT if frames > 2 else SMALL_GT[2:],
                        SMALL_DC if frames > 2 else SMALL_DC[1:], seed)


@pytest.mark.parametrize("frames,seed", [(1, 11), (2, 12), (12, 13)])
def test_generated_sets_overlaps_and_matching(hiplib, frames, seed):
    gts, dts = small_set(frames, seed)
    mins = {0: (0.7, 0.5), 1: (0.7, 0.5), 2: (0.7, 0.25)}
    for metric in range(3):
        got = gpu_blocks(gts, dts, metric)
        want = kr.frame_overlaps(gts, dts, metric)
        assert kr.min_margin(want) >= kc.MARGIN and kr.min_margin(got) >= kc.MARGIN, "margin condition of the generated set"
        check_blocks(got, want, metric, "generated %d" % frames)
        check_matching(packed_from_annos(gts, dts, got), metric, mins[metric], (1, 41))


def test_many_frames_through_the_fixed_order_reduction(hiplib):
    """257 frames (four full rounds of the reducing wave's lanes and one more) of small counts"""
    gts, dts = kc.generated(257, [2, 0, 1, 3, 4], [1, 2, 0, 3], [0, 2, 0], 21)
    got = gpu_blocks(gts, dts, 0)
    check_blocks(got, kr.frame_overlaps(gts, dts, 0), 0, "generated 257")
    check_matching(packed_from_annos(gts, dts, got), 0, (0.7, 0.5), (1,))
    got1 = gpu_blocks(gts[:40], dts[:40], 1)
    want1 = kr.frame_overlaps(gts[:40], dts[:40], 1)
    assert kr.min_margin(want1) >= kc.MARGIN
    check_blocks(got1, want1, 1, "generated 257, first 40")
    check_matching(packed_from_annos(gts[:40], dts[:40], got1), 1, (0.7, 0.5), (41,), combos=[(1, 0), (2, 1)])


def test_largest_supported_frame(hiplib):
    """one frame of EPNET_KITTI_MAX_DT detections and MAX_GT ground-truth rows, 64 of them DontCare: the block equals the same pairs
    computed as many small frames (bit for bit), sampled pairs equal the restatement, and the matching kernels equal the loops"""
    from epnet_amd import kitti_eval_cuda as cu
    ndc = 64
    gts, dts = kc.generated(1, [cu.MAX_DT], [cu.MAX_GT - ndc], [ndc], 31)   # MAX_GT rows in all, 64 of them DontCare
    g, d = gts[0], dts[0]
    assert len(g["name"]) == cu.MAX_GT and len(d["name"]) == cu.MAX_DT and int((g["name"] == "DontCare").sum()) == ndc
    rng = np.random.default_rng(5)
    rows = lambda a, idx: {k: v[idx] for k, v in a.items()}  # noqa: E731
    for metric in range(3):
        big = gpu_blocks(gts, dts, metric)[0]
        # the same pairs as 16 frames of 64 detections each
        parts = gpu_blocks([g] * 16, [rows(d, slice(64 * i, 64 * i + 64)) for i in range(16)], metric)
        assert np.array_equal(big, np.concatenate(parts, 0))
        js, is_ = rng.integers(0, cu.MAX_DT, 40), rng.integers(0, cu.MAX_GT - ndc, 40)
        js[:4], is_[:4] = [0, cu.MAX_DT - 1, 0, cu.MAX_DT - 1], [0, 0, cu.MAX_GT - 1, cu.MAX_GT - 1]
        for j, i in zip(js, is_):
            want = kr.frame_overlaps([rows(g, slice(i, i + 1))], [rows(d, slice(j, j + 1))], metric)[0][0, 0]
            assert big[j, i] == want if metric == 0 else abs(big[j, i] - want) <= kc.ROTATED_TOL, (metric, j, i, big[j, i], want)
        if metric == 0:
            check_matching(packed_from_annos(gts, dts, [big]), 0, (0.7, 0.5), (1,), combos=[(1, 1)])


def test_dontcare_boxes_at_the_stated_maximum(hiplib):
    """EPNET_KITTI_MAX_DC DontCare boxes (all EPNET_KITTI_MAX_GT rows of the frame) under EPNET_KITTI_MAX_DT detections, most of
    them drawn over a DontCare region: every ground-truth row is of another class, so pass 2 is the false-positive count and
    the DontCare loop over all 256 boxes"""
    from epnet_amd import kitti_eval_cuda as cu
    assert cu.MAX_DC <= cu.MAX_GT   # DontCare boxes are ground-truth rows
    gts, dts = kc.generated(1, [cu.MAX_DT], [0], [cu.MAX_DC], 41)
    assert int((gts[0]["name"] == "DontCare").sum()) == cu.MAX_DC == len(gts[0]["name"]) and len(dts[0]["name"]) == cu.MAX_DT
    big = gpu_blocks(gts, dts, 0)
    check_blocks(big, kr.frame_overlaps(gts, dts, 0), 0, "256 DontCare")
    p = packed_from_annos(gts, dts, big)
    assert p.maxima() == (cu.MAX_GT, cu.MAX_DT, cu.MAX_DC)
    check_matching(p, 0, (0.7, 0.5), (1,), combos=[(1, 1)])
    plain = int((p.frames[1][0]["ignored_dt"] == 0).sum())
    with_dc, _ = p.pr([(1, 1)], [0.5], [np.array([0.0])], 0, False)
    without, _ = p.pr([(1, 1)], [0.5], [np.array([0.0])], 1, False)   # the other metrics have no DontCare pass
    assert tuple(without[0, 0]) == (0, plain, 0) and with_dc[0, 0, 1] < plain, (with_dc, without, plain)


# ---- edge cases of the matching rule, on hand-made overlaps --------------------------------------------------------------------
def hand_frame(ov, scores, ign_gt, ign_dt, dt_bbox=None, dc=None):
    ov = np.asarray(ov, np.float64)
    nd, ng = ov.shape
    fr = dict(ignored_gt=np.asarray(ign_gt, np.int64), ignored_dt=np.asarray(ign_dt, np.int64),
              dc=np.asarray(dc if dc is not None else np.zeros((0, 4)), np.float64).reshape(-1, 4), gt_alpha=np.linspace(-1, 1, ng),
              dt_alpha=np.linspace(-2, 2, nd), dt_bbox=np.asarray(dt_bbox if dt_bbox is not None else np.tile([0.0, 0.0, 10.0, 50.0], (nd, 1)), np.float64),
              dt_score=np.asarray(scores, np.float64))
    return ov, fr


def test_matching_edge_cases(hiplib):
    frames = []
    # 0: equal scores, the lowest index wins: gt 0 takes detection 1 (not 2), so gt 1, which only overlaps detection 2, still finds it
    frames.append(hand_frame([[0.9, 0.0], [0.9, 0.0], [0.9, 0.9]], [0.5, 0.8, 0.8], [0, 0], [0, 0, 0]))
    # 1: the same across lanes and mask slots: candidates 0, 64 and 65 with equal scores, 130 lower
    ov = np.zeros((131, 2)); ov[[0, 64, 65, 130], 0] = 0.9; ov[0, 1] = 0.8   # noqa: E702
    sc = np.full(131, 0.1); sc[[0, 64, 65]] = 0.6; sc[130] = 0.3             # noqa: E702
    frames.append(hand_frame(ov, sc, [0, 0], np.zeros(131)))
    # 2: only ignored_det == 1 candidates: the first one is taken, the ground truth is neither tp nor fn, no fp
    frames.append(hand_frame([[0.8], [0.9]], [0.7, 0.9], [0], [1, 1]))
    # 3: a detection matched to an ignored_gt == 1 row is neither tp nor fp; the second row is a plain tp
    frames.append(hand_frame([[0.9, 0.0], [0.0, 0.9]], [0.9, 0.6], [1, 0], [0, 0]))
    # 4: an ignored detection first, then a plain one with a lower overlap: the plain one wins (eval.py:210-216)
    frames.append(hand_frame([[0.95], [0.75], [0.85]], [0.9, 0.8, 0.8], [0], [1, 0, 0]))
    # 5: equal maximum overlaps in pass 2: the first index; a DontCare box covers the leftover detection
    frames.append(hand_frame([[0.8], [0.8], [0.1]], [0.4, 0.9, 0.9], [0], [0, 0, 0],
                             dt_bbox=[[0, 0, 10, 50], [0, 0, 10, 50], [100, 0, 110, 50]], dc=[[99, 0, 120, 60]]))
    # 6: ground truths of another class only (-1): sentinels everywhere, the detection is a false positive
    frames.append(hand_frame([[0.9, 0.9]], [0.9], [-1, -1], [0]))
    blocks = [f[0] for f in frames]
    p = Packed(blocks, [[f[1] for f in frames]])
    m = p.match([(0, 0)], [0.7])[0]
    nan = np.nan
    # frame 1, gt 1: its only candidate (detection 0) went to gt 0; frames 2 and 4: pass 1 goes by score, the best one is ignored
    want = [0.8, 0.8, 0.6, nan, nan, nan, 0.6, nan, 0.9, nan, nan]
    assert np.array_equal(np.isnan(m), np.isnan(want)) and np.array_equal(np.nan_to_num(m), np.nan_to_num(want)), m
    assert np.array_equal(np.nan_to_num(m, nan=-1), np.nan_to_num(restated_match(p, 0, 0.7, 0), nan=-1))
    # a threshold equal to a detection's score keeps that detection: 0.8 keeps both 0.8s of frame 0 and drops its 0.5
    for thr in ([0.8], [0.0], [0.9, 0.6, 0.3]):
        for metric in (0, 1):
            counts, sims = p.pr([(0, 0)], [0.7], [np.array(thr)], metric, True)
            want_pr, terms = restated_pr(p, 0, 0.7, thr, metric, True)
            assert np.array_equal(counts[0].astype(np.float64), want_pr[:, :3]), (thr, metric, counts[0], want_pr)
            assert (np.abs(sims[0] - want_pr[:, 3]) <= kc.similarity_bound(terms, want_pr[:, 3])).all()
    # frame by frame at threshold 0.8, metric 0 (tp, fp, fn)
    for f, expect in enumerate([(2, 0, 0), (0, 0, 2), (0, 0, 0), (0, 0, 1), (1, 1, 0), (1, 0, 0), (0, 1, 0)]):
        one = Packed([blocks[f]], [[frames[f][1]]])
        counts, _ = one.pr([(0, 0)], [0.7], [np.array([0.8])], 0, False)
        assert tuple(counts[0, 0]) == expect, (f, counts[0, 0], expect)


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_official_result_equals_the_reference(hiplib):
    from epnet_amd import kitti_eval
    gts, dts = kc.annos(FX, "a_gt"), kc.annos(FX, "a_dt")
    for m in range(3):
        assert kr.min_margin([FX["a_overlaps_m%d" % m]]) >= kc.MARGIN
    detail = {}
    result, ret = kitti_eval.get_official_eval_result(gts, dts, 0, device=DEV, _detail=detail)
    assert result == str(FX["a_car_result"])
    assert sorted(ret) == [str(k) for k in FX["a_car_ret_keys"]] and len(ret) == 9
    got = np.array([ret[k] for k in sorted(ret)])
    print("ret_dict max |diff| %.3e" % np.abs(got - FX["a_car_ret"]).max())
    assert np.abs(got - FX["a_car_ret"]).max() <= 1e-9
    for metric in range(3):
        for l, k in COMBOS:
            key = "a_car_m%d_c0_d%d_k%d" % (metric, l, k)
            assert np.array_equal(detail[metric][(0, l, k)]["thresholds"], FX[key + "_thresholds"]), key
            assert np.array_equal(detail[metric][(0, l, k)]["pr"][:, :3], FX[key + "_pr"][:, :3]), key
    result_all, ret_all = kitti_eval.get_official_eval_result(gts, dts, ["Car", "Pedestrian", "Cyclist"])
    assert result_all == str(FX["a_all_result"])
    assert np.abs(np.array([ret_all[k] for k in sorted(ret_all)]) - FX["a_all_ret"]).max() <= 1e-9
    gts_b, dts_b = kc.annos(FX, "b_gt"), kc.annos(FX, "b_dt")
    detail_b = {}
    result_b, ret_b = kitti_eval.get_official_eval_result(gts_b, dts_b, 2, _detail=detail_b)
    assert result_b == str(FX["b_cyc_result"]) and all(v == 0 for v in ret_b.values())
    assert all(detail_b[metric][(0, l, k)]["thresholds"].size == 0 for metric in range(3) for l, k in COMBOS)


def test_runs_and_streams_give_identical_bits(hiplib):
    from epnet_amd import kitti_eval
    gts, dts = kc.annos(FX, "a_gt"), kc.annos(FX, "a_dt")

    def run():
        detail = {}
        result, ret = kitti_eval.get_official_eval_result(gts, dts, 0, _detail=detail)
        arrays = [np.array([ret[k] for k in sorted(ret)])]
        for metric in range(3):
            arrays += [b for b in kitti_eval.calculate_iou_partly(dts, gts, metric)[0]]
            for l, k in COMBOS:
                arrays += [detail[metric][(0, l, k)]["thresholds"], detail[metric][(0, l, k)]["pr"]]
        return result, arrays

    first = run()
    second = run()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    for other in (second, third):
        assert other[0] == first[0] and len(other[1]) == len(first[1])
        for a, b in zip(first[1], other[1]):
            assert a.shape == b.shape and a.tobytes() == b.tobytes()


def test_rotate_iou_gpu_eval_and_the_dontcare_criterion(hiplib):
    """the served rotate_iou_gpu_eval(boxes, query_boxes, -1), and metric 0 with criterion 0 (eval.py:247) through the stand-in"""
    from epnet_amd import kitti_eval, kitti_eval_cuda, pointnet2_utils
    gts, dts = kc.annos(FX, "a_gt"), kc.annos(FX, "a_dt")
    f = int(np.argmax(FX["a_gt_num"] * FX["a_dt_num"]))
    db, gb = kr.metric_boxes(dts[f], 1), kr.metric_boxes(gts[f], 1)
    got = kitti_eval.rotate_iou_gpu_eval(db, gb, -1)
    want = kr.rotate_iou_eval(db, gb, -1)
    assert got.dtype == np.float32 and got.shape == want.shape and np.abs(got - want).max() <= kc.ROTATED_TOL
    assert kitti_eval.rotate_iou_gpu_eval(np.zeros((0, 5)), gb).shape == (0, len(gb))
    rows, cols = kr.metric_boxes(dts[f], 0), kr.metric_boxes(gts[f], 0)
    out = pointnet2_utils._new(up(rows), (rows.shape[0] * cols.shape[0],), torch.float64)
    for criterion in (0, 1, -1):
        kitti_eval_cuda.kitti_overlaps_gpu(0, criterion, len(rows), len(cols), up(offsets([len(rows)])), up(offsets([len(cols)])),
                                           up(offsets([len(rows) * len(cols)], np.int64)), up(rows), up(cols), out)
        assert np.array_equal(out.cpu().numpy().reshape(len(rows), len(cols)), kr.image_box_overlap(rows, cols, criterion)), criterion

"""The evaluation epoch on the GPU (-m gpu): epnet_eval_recall and epnet_kitti_records against the numpy restatements of
tests/eval_epoch_restate.py -- the same arithmetic of record, so equality; outputs pre-filled with NaN / -1 to prove that every
element is written -- the reference's fixture through the GPU layers, and the point of the feature: DetectionLayer + eval_batch
captured into ONE HIP graph and replayed on new batches. The IoU matrices the recall restatement takes come from boxes_iou3d_gpu
on the same device tensors: it sees the floats the kernel sees.
"""
import numpy as np
import pytest
import torch

import eval_epoch_restate as R
from test_eval_epoch import T, check_result, check_text_round_trip, gt_annos_of, run_epoch

pytestmark = pytest.mark.gpu

NAN = float("nan")


def device_iou(boxes, gt):
    """(b,m,7), (b,g,gc) device tensors -> (b,m,g) numpy, every gt ROW against every box through the package's boxes_iou3d_gpu"""
    from epnet_amd import iou3d_utils
    b, m, g = boxes.shape[0], boxes.shape[1], gt.shape[1]
    if g == 0:
        return np.zeros((b, m, 0), np.float32)
    return np.stack([iou3d_utils.boxes_iou3d_gpu(boxes[k].contiguous(), gt[k, :, :7].contiguous()).cpu().numpy() for k in range(b)])


def run_recall(pred, roi, gt, thresholds, seg, label, totals=None, stream=None):
    """-> the outputs on the device, pre-filled with NaN / -1"""
    from epnet_amd import iou3d_cuda
    b, m, g, nt = pred.shape[0], pred.shape[1], gt.shape[1], len(thresholds)
    stats = torch.full((b, 1 + 2 * nt), -1, dtype=torch.int32, device="cuda")
    seg_counts = None if seg is None else torch.full((3,), -1, dtype=torch.int64, device="cuda")
    gmp, gmr = torch.full((b, g), NAN, device="cuda"), torch.full((b, g), NAN, device="cuda")
    pmi = torch.full((b, m), NAN, device="cuda")

    def call():
        iou3d_cuda.eval_recall_gpu(pred, roi, gt, thresholds, seg, label, stats, seg_counts, totals, gmp, gmr, pmi)
    if stream is None:
        call()
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            call()
        torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    return stats, seg_counts, gmp, gmr, pmi


def check_recall(got, want, where):
    stats, seg_counts, gmp, gmr, pmi = got
    w_stats, w_seg, w_gmp, w_gmr, w_pmi = want
    np.testing.assert_array_equal(stats.cpu().numpy(), w_stats, err_msg=str(where))
    if w_seg is None:
        assert seg_counts is None
    else:
        np.testing.assert_array_equal(seg_counts.cpu().numpy(), w_seg, err_msg=str(where))
    np.testing.assert_array_equal(gmp.cpu().numpy(), w_gmp, err_msg=str(where))      # (NaN == NaN here: a NaN maximum is a value)
    np.testing.assert_array_equal(gmr.cpu().numpy(), w_gmr, err_msg=str(where))
    np.testing.assert_array_equal(pmi.cpu().numpy(), w_pmi, err_msg=str(where))


@pytest.mark.parametrize("b,m,g,gc,nt,n,with_roi,seed", R.recall_cases(), ids=lambda v: str(v))
def test_recall_equals_the_restatement(hiplib, b, m, g, gc, nt, n, with_roi, seed):
    pred, roi, gt, seg, label = R.recall_inputs(b, m, g, gc, n, seed)
    pred, roi, gt = pred.cuda(), (roi.cuda() if with_roi else None), gt.cuda()
    seg, label = (None, None) if seg is None else (seg.cuda(), label.cuda())
    iou_p = device_iou(pred, gt)
    iou_r = device_iou(roi, gt) if with_roi else None
    thresholds = [0.1, 0.3, 0.5, 0.7, 0.9, 0.2, 0.4, 0.6][:nt]
    # a threshold EQUAL to an occurring gt-max value pins the strict comparison
    base = R.eval_recall(iou_p, iou_r, gt.cpu().numpy(), thresholds)
    finite = base[2][np.isfinite(base[2]) & (base[2] > 0)]
    if finite.size:
        thresholds[-1] = float(finite[finite.size // 2])
    totals = torch.full((1 + 2 * nt,), 7, dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream() if seed % 5 == 0 else None                       # every fifth case on a stream of its own
    got = run_recall(pred, roi, gt, thresholds, seg, label, totals, stream)
    want = R.eval_recall(iou_p, iou_r, gt.cpu().numpy(), thresholds, None if seg is None else seg.cpu().numpy(),
                         None if label is None else label.cpu().numpy())
    check_recall(got, want, (b, m, g, seed))
    if finite.size:                                                               # the equal value is NOT recalled, the one below it is
        with np.errstate(invalid="ignore"):
            hit = int((base[2] > np.float32(thresholds[-1])).sum())
            assert int(want[0][:, nt].sum()) == hit < int((base[2] >= np.float32(thresholds[-1])).sum())
    got2 = run_recall(pred, roi, gt, thresholds, seg, label, totals)              # the running sums take two calls
    check_recall(got2, want, (b, m, g, seed, "second call"))
    np.testing.assert_array_equal(totals.cpu().numpy(), 7 + 2 * want[0].astype(np.int64).sum(0))
    fam = {(k + seed) % 5 for k in range(b)}
    if 4 in fam and g >= 1:
        assert (want[2] > 0.999).any()                                             # the gt identical to a box
    if 4 in fam and g >= 2 and m >= 4:
        # the pair with a NaN IoU: the NaN wins its column and its row, and the column is recalled at no threshold
        gmp, gmr, pmi = (t.cpu().numpy() for t in got[2:5])
        stats = got[0].cpu().numpy()
        for k in range(b):
            if (k + seed) % 5 != 4:
                continue
            num_gt = int(stats[k, 0])
            assert num_gt == g and np.isnan(gmp[k, g - 1]) and np.isnan(pmi[k, 1]) and not np.isnan(gmp[k, :g - 1]).any()
            assert not np.isnan(pmi[k, 2:]).any()         # (box 0, all NaN, meets the infinite row the same way)
            numbers = int((~np.isnan(gmp[k, :num_gt])).sum())
            assert numbers == g - 1 and (stats[k, 1:1 + nt] <= numbers).all()
            low = run_recall(pred, roi, gt, [-1.0], seg, label)[0].cpu().numpy()     # every number is above -1, a NaN is not
            assert low[k, 1] == numbers
            if with_roi:
                assert np.isnan(gmr[k, g - 1]) and low[k, 2] == int((~np.isnan(gmr[k, :num_gt])).sum()) == g - 1
    if 1 in fam:
        assert (want[0][:, 0] == 0).any()


def test_recall_family_coverage():
    cases = R.recall_cases()
    assert {c[1] for c in cases} == set(R.REC_M) and {c[2] for c in cases} >= set(R.REC_G) and {c[0] for c in cases} == set(R.REC_B)
    assert {c[3] for c in cases} == set(R.REC_GC) and {c[4] for c in cases} == set(R.REC_NT) and {c[5] for c in cases} == set(R.SEG_N)
    assert any(not c[6] for c in cases) and {(k + c[7]) % 5 for c in cases for k in range(c[0])} == {0, 1, 2, 3, 4}
    _, _, gt, _, _ = R.recall_inputs(5, 10, 20, 7, None, 3003)
    fams = [(k + 3003) % 5 for k in range(5)]
    k3 = fams.index(3)
    assert gt[k3, 19].any() and float(gt[k3, 19].sum()) == 0.0 and R.count_gt(gt[k3].numpy()) == 19      # the cancelling row is no box row
    k2 = fams.index(2)
    assert not gt[k2, 0].any() and R.count_gt(gt[k2].numpy()) == 19


def run_records(boxes, scores, count, p2, shape):
    from epnet_amd import iou3d_cuda
    b, m = scores.shape
    rec = torch.full((b, m, 13), NAN, dtype=torch.float64, device="cuda")
    cnt = torch.full((b,), -1, dtype=torch.int32, device="cuda")
    raw = torch.full((b, m, 4), NAN, device="cuda")
    val = torch.full((b, m), -1, dtype=torch.int32, device="cuda")
    iou3d_cuda.kitti_records_gpu(boxes, scores, count, p2, shape, rec, cnt, raw, val)
    torch.cuda.synchronize()
    return rec, cnt, raw, val


@pytest.mark.parametrize("b,m,mode,seed", R.records_cases(), ids=lambda v: str(v))
def test_records_equal_the_restatement(hiplib, b, m, mode, seed):
    boxes, scores, count, p2, shape = R.records_inputs(b, m, mode, seed)
    dev = [t if t is None else t.cuda() for t in (boxes, scores, count, p2, shape)]
    rec, cnt, raw, val = run_records(*dev)
    w_rec, w_cnt, w_raw, w_val = R.kitti_records(boxes.numpy(), scores.numpy(), None if count is None else count.numpy(), p2.numpy(),
                                                 shape.numpy())
    np.testing.assert_array_equal(val.cpu().numpy(), w_val)
    np.testing.assert_array_equal(cnt.cpu().numpy(), w_cnt)
    np.testing.assert_array_equal(raw.cpu().numpy(), w_raw)                       # NaN image coordinates of NaN boxes included
    np.testing.assert_array_equal(rec.cpu().numpy(), w_rec)
    if mode in ("full", "none") and m >= 100:
        assert 0 < w_val.sum() < w_val.size and np.isnan(w_raw).any()
        i = np.arange(m)
        assert (w_val[:, i % 8 == 3] == 0).all() and np.isfinite(w_raw[:, i % 8 == 3]).all()      # wider than 0.8 of the image
    if mode in ("full", "none") and m >= 128:                                     # the compaction order across wave boundaries
        assert w_val[:, [0, 63, 64, 127]].all()
        first = w_rec[0, :, 8:11]                                                  # x, y, z of the compacted rows, in input order
        src = boxes.numpy()[0][w_val[0] == 1][:, 0:3]
        np.testing.assert_array_equal(first[:w_cnt[0]], R.r4(src))
    # records without the optional outputs give the same
    from epnet_amd import iou3d_cuda
    rec2 = torch.full_like(rec, NAN)
    cnt2 = torch.full_like(cnt, -1)
    iou3d_cuda.kitti_records_gpu(dev[0], dev[1], dev[2], dev[3], dev[4], rec2, cnt2)
    torch.cuda.synchronize()
    assert torch.equal(cnt2, cnt) and np.array_equal(rec2.cpu().numpy(), rec.cpu().numpy())


def test_too_many_boxes_are_refused_and_nothing_is_written(hiplib):
    from epnet_amd import iou3d_cuda
    b, m = 2, 4097
    boxes, scores = torch.zeros((b, m, 7), device="cuda"), torch.zeros((b, m), device="cuda")
    p2, shape = T(np.stack([R.P2_KITTI] * b), "cuda"), T(np.array([R.IMG_KITTI] * b, np.int32), "cuda")
    rec = torch.full((b, m, 13), NAN, dtype=torch.float64, device="cuda")
    cnt = torch.full((b,), -1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="kitti_records"):
        iou3d_cuda.kitti_records_gpu(boxes, scores, None, p2, shape, rec, cnt)
    gt = torch.zeros((b, 4, 7), device="cuda")
    stats = torch.full((b, 19), -1, dtype=torch.int32, device="cuda")
    gmp = torch.full((b, 4), NAN, device="cuda")
    with pytest.raises(RuntimeError, match="eval_recall"):
        iou3d_cuda.eval_recall_gpu(boxes, None, gt, [0.1, 0.3, 0.5, 0.7, 0.9], None, None, stats, gt_max_pred=gmp)
    with pytest.raises(RuntimeError, match="eval_recall"):
        iou3d_cuda.eval_recall_gpu(boxes[:, :100].contiguous(), None, gt, [0.1] * 9, None, None, stats, gt_max_pred=gmp)
    torch.cuda.synchronize()
    assert bool(torch.isnan(rec).all()) and bool((cnt == -1).all()) and bool((stats == -1).all()) and bool(torch.isnan(gmp).all())


def test_epoch_matches_the_reference_gpu(hiplib, tmp_path):
    """the fixture through the kernels: the ret_dict entries bit for bit, the text round trip, and the AP evaluator fed with
    dt_annos() against the same call on the parsed files"""
    from epnet_amd import kitti_eval
    ep, fx = run_epoch("cuda")
    check_result(ep, fx)
    annos, parsed = check_text_round_trip(ep, fx, tmp_path)
    gts = gt_annos_of(fx)
    text_a, ap_a = kitti_eval.get_official_eval_result(gts, annos, 0)
    text_p, ap_p = kitti_eval.get_official_eval_result(gts, parsed, 0)
    assert text_a == text_p and ap_a == ap_p
    from epnet_amd import eval_epoch
    out = eval_epoch.eval_batch(*[T(fx[k][:2], "cuda") for k in ("pred_boxes3d", "rois", "det_boxes3d", "det_scores", "det_count",
                                                                 "gt_boxes3d", "P2", "img_shape")])
    np.testing.assert_array_equal(out.valid.cpu().numpy(), fx["valid"][:2])
    np.testing.assert_array_equal(out.gt_max_pred.cpu().numpy()[0, :9] > 0.7, fx["gt_max_iou"][0, :9] > 0.7)


def test_detector_and_evaluation_capture_into_one_hip_graph(hiplib, oracle):
    """DetectionLayer + eval_batch in ONE torch.cuda.graph (capture fails on any synchronisation); replayed on three new
    batches written into the static tensors, each replay equal to the eager result on that batch, bit for bit, and to the
    restatements"""
    from epnet_amd import detection_layer as dl, eval_epoch, synth
    d = "cuda"
    b, m, g, n = 2, 24, 6, 1000
    layer = dl.DetectionLayer(dl.default_cfg()).to(d)

    def batch(seed):
        gen = torch.Generator().manual_seed(seed)
        rois, gts = zip(*[R.scene_boxes(m, g, seed + 31 * k) for k in range(b)])
        gt = torch.stack(gts)
        gt[1, g - 1] = 0                                                        # a padding row
        cls = torch.randn((b * m, 1), generator=gen) * 2.0
        reg = (torch.randn((b * m, 46), generator=gen) * 0.3)
        seg = (torch.rand((b, n), generator=gen) < 0.4).int()
        label = torch.randint(-1, 2, (b, n), generator=gen).int()
        return [torch.stack(rois).contiguous(), cls, reg, gt.contiguous(), seg, label]

    p2, shape = T(np.stack([R.P2_KITTI] * b), d), T(np.array([R.IMG_KITTI] * b, np.int32), d)
    static = [t.to(d) for t in batch(50)]
    totals = torch.zeros((11,), dtype=torch.int64, device=d)

    def step():
        with torch.no_grad():
            rois, cls, reg, gt, seg, label = static
            pred, raw, norm, det_b, det_s, det_c = layer(rois, cls, reg)
            out = eval_epoch.eval_batch(pred, rois, det_b, det_s, det_c, gt, p2, shape, seg, label, totals=totals)
            return [pred, det_b, det_s, det_c, out.scene_stats, out.seg_counts, out.gt_max_pred, out.gt_max_roi, out.pred_max_iou,
                    out.records, out.rec_count, out.bbox_raw, out.valid]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graph_out = step()
    totals.zero_()
    expect_totals = np.zeros(11, np.int64)
    seen = []
    for seed in (60, 70, 80):
        for dst, src in zip(static, batch(seed)):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in graph_out]
        eager = step()
        torch.cuda.synchronize()
        for i, (a, e) in enumerate(zip(replayed, eager)):
            assert np.array_equal(a.cpu().numpy(), e.cpu().numpy(), equal_nan=True), (seed, i)
        rois, cls, reg, gt, seg, label = static
        pred = replayed[0]
        want = R.eval_recall(device_iou(pred, gt), device_iou(rois, gt), gt.cpu().numpy(), eval_epoch.THRESH_LIST, seg.cpu().numpy(),
                             label.cpu().numpy())
        for got, w in zip(replayed[4:9], want):
            np.testing.assert_array_equal(got.cpu().numpy(), w)
        w_rec = R.kitti_records(replayed[1].cpu().numpy(), replayed[2].cpu().numpy(), replayed[3].cpu().numpy(), p2.cpu().numpy(),
                                shape.cpu().numpy())
        for got, w in zip(replayed[9:13], w_rec):
            np.testing.assert_array_equal(got.cpu().numpy(), w)
        expect_totals += 2 * want[0].astype(np.int64).sum(0)                    # the replay and the eager call both add
        seen.append((tuple(want[0][:, 1].tolist()), tuple(w_rec[1].tolist())))      # recalled at 0.1, records per scene
    np.testing.assert_array_equal(totals.cpu().numpy(), expect_totals)
    assert len(set(seen)) > 1 and any(sum(s[1]) > 0 for s in seen) and any(sum(s[0]) > 0 for s in seen)

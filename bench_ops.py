#!/usr/bin/env python3
"""bench_ops.py -- per-operator timings of the hot-path rows that are not part of bench.py's SA stack:
iou3d (rotated overlap / IoU, both NMS flavours), roipool3d, three_nn / three_interpolate and the three
gradient ops, at the shapes of the reference's rcnn_online step. One JSON line per op:
median HIP-event time, algorithmic bytes (SURVEY.md 8d formulas) and the resulting GB/s.

    python bench_ops.py [--reps 20] [--stage2-only | --loss-only | --targets-only | --optim-only | --scan-only | --gt-aug-only | --handover-only |
                         --image-head-only | --sa-tail-only]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


# ---- the training losses composed from stock torch calls (the comparators of epnet_amd.loss_utils) ---------------------------------
# composed_*_loss(..., sync_free=False): the reference's structure (lib/net/train_functions.py:92-284 over lib/utils/loss_utils.py:
# 90-350) restated on this package's surface -- boolean-mask indexing of the foreground rows (a nonzero and a device-to-host read
# each), the host branch on fg_sum, scatter_ one-hots, cross_entropy / smooth_l1_loss means, and the .item() reads of the log.
# sync_free=True: the same loss as masked sums over ALL rows (no indexing, no read-back): the honest alternative to a kernel.
def _composed_box_loss(cfg, stage_cfg, names, cls_logit, pred_reg, reg_label, cls_label, reg_mask, iou_branch, ry_fine, w_cls, w_reg, w_train,
                       fg_weight, sync_free):
    import math
    import torch
    import torch.nn.functional as F
    from epnet_amd.loss_utils import LossReturn
    rows = cls_label.numel()
    x = cls_logit.reshape(-1)
    label = cls_label.reshape(-1)
    pred_reg, reg_label = pred_reg.reshape(rows, -1), reg_label.reshape(rows, 7)
    fg_mask = (label > 0) if reg_mask is None else (reg_mask.reshape(-1) > 0)
    log = {}
    # ---- classification
    if stage_cfg.LOSS_CLS == "SigmoidFocalLoss":
        target, pos, neg = (label > 0).float(), (label > 0).float(), (label == 0).float()
        weights = (pos + neg) / torch.clamp(pos.sum(), min=1.0)
        ce = torch.clamp(x, min=0) - x * target + torch.log1p(torch.exp(-torch.abs(x)))
        prob = torch.sigmoid(x)
        p_t = target * prob + (1 - target) * (1 - prob)
        alpha = stage_cfg.FOCAL_ALPHA[0]
        per = torch.pow(1.0 - p_t, stage_cfg.FOCAL_GAMMA) * (target * alpha + (1 - target) * (1 - alpha)) * ce * weights
        loss_cls, cls_pos, cls_neg = per.sum(), (per * pos).sum(), (per * neg).sum()
        if not sync_free:
            log["loss_cls_pos"], log["loss_cls_neg"] = cls_pos.item(), cls_neg.item()
    else:
        weight = torch.where(label > 0, float(fg_weight), 1.0)
        # the target is clamped: F.binary_cross_entropy refuses the -1 of an ignored row (a device-side assert)
        per = F.binary_cross_entropy(torch.sigmoid(x), (label > 0).float(), weight=weight, reduction="none")
        valid = (label >= 0).float()
        loss_cls = (per * valid).sum() / torch.clamp(valid.sum(), min=1.0)
        cls_pos = cls_neg = loss_cls * 0
    # ---- regression
    if sync_free:
        rw = fg_mask.float() / torch.clamp(fg_mask.float().sum(), min=1.0)     # a masked mean
        pr, lb, score, q = pred_reg, reg_label, torch.sigmoid(x), None if iou_branch is None else iou_branch.reshape(-1)
        fg_sum = None
    else:
        fg_sum = fg_mask.long().sum().item()
        if fg_sum != 0:
            pr, lb, score = pred_reg[fg_mask], reg_label[fg_mask], torch.sigmoid(x)[fg_mask]
            q = None if iou_branch is None else iou_branch.reshape(-1)[fg_mask]
            rw = None
    zero = loss_cls * 0
    parts = dict.fromkeys(("x_bin", "z_bin", "x_res", "z_res", "y_offset", "ry_bin", "ry_res", "size", "iou", "branch"), zero)
    if sync_free or fg_sum != 0:
        scope, bs, nh = stage_cfg.LOC_SCOPE, stage_cfg.LOC_BIN_SIZE, stage_cfg.NUM_HEAD_BIN
        nb = int(scope / bs) * 2
        anchor = _anchor(cfg, pr.device)

        def mean(v):
            return v.mean() if rw is None else (v * (rw if v.dim() == 1 else rw[:, None])).sum()

        def ce_mean(logits, target):
            return F.cross_entropy(logits, target) if rw is None else (F.cross_entropy(logits, target, reduction="none") * rw).sum()

        def sl1_mean(a, b):
            return F.smooth_l1_loss(a, b) if rw is None else mean(F.smooth_l1_loss(a, b, reduction="none"))

        def onehot(lab_, n):
            o = torch.zeros((lab_.size(0), n), device=lab_.device)
            o.scatter_(1, lab_.view(-1, 1), 1)
            return o
        x_shift = torch.clamp(lb[:, 0] + scope, 0, scope * 2 - 1e-3)
        z_shift = torch.clamp(lb[:, 2] + scope, 0, scope * 2 - 1e-3)
        x_bin, z_bin = (x_shift / bs).floor().long(), (z_shift / bs).floor().long()
        x_res = x_shift - (x_bin.float() * bs + bs / 2)
        z_res = z_shift - (z_bin.float() * bs + bs / 2)
        x_hot, z_hot = onehot(x_bin, nb), onehot(z_bin, nb)
        parts["x_bin"], parts["z_bin"] = ce_mean(pr[:, 0:nb], x_bin), ce_mean(pr[:, nb:2 * nb], z_bin)
        parts["x_res"] = sl1_mean((pr[:, 2 * nb:3 * nb] * x_hot).sum(dim=1), x_res / bs)
        parts["z_res"] = sl1_mean((pr[:, 3 * nb:4 * nb] * z_hot).sum(dim=1), z_res / bs)
        o_y = 4 * nb
        parts["y_offset"] = sl1_mean(pr[:, o_y:o_y + 1].sum(dim=1), lb[:, 1])
        ry = lb[:, 6]
        if ry_fine:
            apc = (math.pi / 2) / nh
            ry = ry % (2 * math.pi)
            opposite = (ry > math.pi * 0.5) & (ry < math.pi * 1.5)
            ry = torch.where(opposite, (ry + math.pi) % (2 * math.pi), ry)
            shift = torch.clamp((ry + math.pi * 0.5) % (2 * math.pi) - math.pi * 0.25, min=1e-3, max=math.pi * 0.5 - 1e-3)
        else:
            apc = (2 * math.pi) / nh
            shift = (ry % (2 * math.pi) + apc / 2) % (2 * math.pi)
        r_bin = (shift / apc).floor().long()
        r_res = (shift - (r_bin.float() * apc + apc / 2)) / (apc / 2)
        r_hot = onehot(r_bin, nh)
        o_rb, o_rr, o_sz = o_y + 1, o_y + 1 + nh, o_y + 1 + 2 * nh
        parts["ry_bin"] = ce_mean(pr[:, o_rb:o_rr], r_bin)
        parts["ry_res"] = sl1_mean((pr[:, o_rr:o_sz] * r_hot).sum(dim=1), r_res)
        size_norm = pr[:, o_sz:o_sz + 3]
        parts["size"] = sl1_mean(size_norm, (lb[:, 3:6] - anchor) / anchor) if rw is None else \
            (F.smooth_l1_loss(size_norm, (lb[:, 3:6] - anchor) / anchor, reduction="none") * rw[:, None]).sum() / 3
        # the consistency-enforcing IoU term
        pred_size = size_norm * anchor + anchor
        if cfg.TRAIN.IOU_LOSS_TYPE == "raw":
            pred_x, pred_z = (pr[:, 2 * nb:3 * nb] * x_hot).sum(dim=1) * bs, (pr[:, 3 * nb:4 * nb] * z_hot).sum(dim=1) * bs
            tar_x, tar_z = x_res, z_res
        else:
            centre = (torch.arange(nb, device=pr.device).float() * bs + bs / 2 - scope)
            pred_x = ((centre + pr[:, 2 * nb:3 * nb] * bs) * F.softmax(pr[:, 0:nb], 1)).sum(dim=1)
            pred_z = ((centre + pr[:, 3 * nb:4 * nb] * bs) * F.softmax(pr[:, nb:2 * nb], 1)).sum(dim=1)
            tar_x, tar_z = centre[x_bin] + x_res, centre[z_bin] + z_res
        pred_y = pr[:, o_y:o_y + 1].sum(dim=1)

        def overlap(pc, pe, tc, te):
            return torch.clamp(torch.min(pc + pe / 2, tc + te / 2) - torch.max(pc - pe / 2, tc - te / 2), min=1e-3)
        inter = overlap(pred_x, pred_size[:, 2], tar_x, lb[:, 5]) * overlap(pred_y, pred_size[:, 0], lb[:, 1], lb[:, 3]) * \
            overlap(pred_z, pred_size[:, 1], tar_z, lb[:, 4])
        pred_vol = torch.clamp(pred_size[:, 0] * pred_size[:, 1] * pred_size[:, 2], min=1e-3)
        iou = inter / (pred_vol + lb[:, 3] * lb[:, 4] * lb[:, 5] - inter)
        if q is not None:
            qc, tg = torch.clamp(q, 0.0001, 0.9999), torch.clamp(iou, 0.0001, 0.9999).detach()
            parts["branch"] = mean(-(tg * torch.log(qc) + (1 - tg) * torch.log(1 - qc)))
        parts["iou"] = mean(-torch.log(torch.clamp(score * iou, min=1e-4)))
        if not sync_free:
            for k in ("x_bin", "z_bin", "x_res", "z_res", "y_offset", "ry_bin", "ry_res"):
                log[k] = parts[k].item()                                        # reg_loss_dict's .item()s
    loss_loc = parts["x_bin"] + parts["z_bin"] + parts["x_res"] + parts["z_res"] + parts["y_offset"]
    loss_angle = parts["ry_bin"] + parts["ry_res"]
    loss_size, loss_iou = 3 * parts["size"], cfg.TRAIN.CE_WEIGHT * parts["iou"]
    loss_reg = loss_loc + loss_angle + loss_size + loss_iou + parts["branch"]
    loss = loss_cls * w_cls + loss_reg * w_reg
    total = loss * w_train
    pos_n, neg_n, valid_n = (label > 0).sum(), (label == 0).sum(), (label >= 0).sum()
    entries = [total, loss, loss_cls, cls_pos, cls_neg, loss_reg, loss_loc, loss_angle, loss_size, loss_iou, parts["x_bin"], parts["z_bin"],
               parts["x_res"], parts["z_res"], parts["y_offset"], parts["ry_bin"], parts["ry_res"], parts["branch"],
               fg_mask.sum(), pos_n, neg_n, valid_n, parts["size"], parts["iou"]]
    if not sync_free:                                                           # tb_dict / disp_dict: one .item() per entry
        for k, v in zip(names, entries):
            log[k] = v.item()
    terms = torch.stack([e.detach().float().reshape(()) for e in entries])
    return LossReturn(total, terms, names)


_anchors = {}


def _anchor(cfg, device):
    import torch
    if str(device) not in _anchors:
        _anchors[str(device)] = torch.from_numpy(cfg.CLS_MEAN_SIZE[0]).to(device)
    return _anchors[str(device)]


def composed_rpn_loss(rpn_cls, rpn_reg, rpn_cls_label, rpn_reg_label, cfg=None, sync_free=False):
    from epnet_amd import loss_utils
    cfg = cfg if cfg is not None else loss_utils.default_cfg()
    return _composed_box_loss(cfg, cfg.RPN, loss_utils.RPN_TERM_NAMES, rpn_cls, rpn_reg, rpn_reg_label, rpn_cls_label, None, None, False,
                              cfg.RPN.LOSS_WEIGHT[0], cfg.RPN.LOSS_WEIGHT[1], cfg.TRAIN.RPN_TRAIN_WEIGHT, cfg.RPN.FG_WEIGHT, sync_free)


def composed_rcnn_loss(ret_dict, cfg=None, sync_free=False):
    from epnet_amd import loss_utils
    cfg = cfg if cfg is not None else loss_utils.default_cfg()
    return _composed_box_loss(cfg, cfg.RCNN, loss_utils.RCNN_TERM_NAMES, ret_dict["rcnn_cls"], ret_dict["rcnn_reg"], ret_dict["gt_of_rois"],
                              ret_dict["cls_label"], ret_dict["reg_valid_mask"], ret_dict["rcnn_iou_branch"] if cfg.USE_IOU_BRANCH else None,
                              True, 1.0, 1.0, cfg.TRAIN.RCNN_TRAIN_WEIGHT, 1.0, sync_free)


def loss_rows(args, report, timeit_pair):
    """forward + backward of the fused losses against (i) the reference-shaped composition and (ii) the sync-free stock-torch form,
    at the RPN shapes (scenes x 16384 points x 76, labels from the synthetic scenes' ground-truth boxes) and the RCNN shapes
    (scenes x 64 ROIs x 46)"""
    import torch
    import bench_step
    from epnet_amd import loss_utils
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    for bsz in (1, 2, 16):
        xyz, gts = bench_step.synthetic_batch(bsz, 16384, 300, dev)
        cls_label, reg_label = bench_step.rpn_labels(xyz, gts)
        rpn_cls = (torch.randn((bsz, 16384, 1), generator=g) * 1.5).to(dev).requires_grad_(True)
        rpn_reg = (torch.randn((bsz, 16384, 76), generator=g) * 0.5).to(dev).requires_grad_(True)
        u = torch.rand((bsz * 64,), generator=g).to(dev)
        ret = {"rcnn_cls": (torch.randn((bsz * 64, 1), generator=g) * 1.5).to(dev).requires_grad_(True),
               "rcnn_reg": (torch.randn((bsz * 64, 46), generator=g) * 0.5).to(dev).requires_grad_(True),
               "cls_label": torch.where(u > 0.6, 1, torch.where(u < 0.45, 0, -1)).long(), "reg_valid_mask": (u > 0.55).long(),
               "gt_of_rois": torch.cat([(torch.rand((bsz * 64, 3), generator=g) - 0.5) * 2, torch.tensor([1.5, 1.6, 3.9]) * (0.9 + 0.2 * torch.rand((bsz * 64, 3), generator=g)),
                                        torch.rand((bsz * 64, 1), generator=g) * 6.28], dim=1).to(dev)}
        for stage, rows, c, leaves, fns in (
                ("rpn", bsz * 16384, 76, [rpn_cls, rpn_reg], [lambda sf=None: loss_utils.rpn_loss(rpn_cls, rpn_reg, cls_label, reg_label) if sf is None
                                                              else composed_rpn_loss(rpn_cls, rpn_reg, cls_label, reg_label, sync_free=sf)]),
                ("rcnn", bsz * 64, 46, [ret["rcnn_cls"], ret["rcnn_reg"]], [lambda sf=None: loss_utils.rcnn_loss(ret) if sf is None
                                                                            else composed_rcnn_loss(ret, sync_free=sf)])):
            fn = fns[0]

            def run(sf):
                out = fn(sf)
                torch.autograd.grad(out.loss, leaves, allow_unused=True)
                return out
            fused, ref_shaped, sync_free = (lambda: run(None)), (lambda: run(False)), (lambda: run(True))
            a, b, c_ = fused(), ref_shaped(), sync_free()
            close = bool(torch.allclose(a.terms, b.terms, rtol=1e-4, atol=1e-5) and torch.allclose(a.terms, c_.terms, rtol=1e-4, atol=1e-5))
            ms_ref, ms_fused = timeit_pair(ref_shaped, fused)
            ms_free, ms_fused2 = timeit_pair(sync_free, fused)
            report("%s_loss fwd+bwd" % stage, {"scenes": bsz, "rows": rows, "C": c, "fg": int(a.terms[18])}, ms_fused,
                   rows * (c * 8 + 7 * 4 + 4 + 8),
                   "one fused call + backward scaling; (i) reference-shaped composition (mask indexing, .item() reads): %.4f ms; (ii) sync-free "
                   "stock-torch form (masked sums): %.4f ms (fused in that pair: %.4f ms); same terms within 1e-4: %s"
                   % (ms_ref, ms_free, ms_fused2, close))


# ---- the optimiser step composed from stock torch calls (the comparator of epnet_amd.optim.FusedAdamOneCycle) -------------------------
class ComposedAdamOneCycle:
    """the reference's adam_onecycle step (tools/train_utils/train_utils.py:126-136) from stock torch calls: clip_grad_norm_, a
    host-side one-cycle schedule that sets lr and beta1 as Python floats, the true-weight-decay loop (one mul_ per trainable
    parameter) and torch.optim.Adam.step(); zero_grad() is stock (gradients become None)"""

    def __init__(self, params, total_steps, lr_max=0.002, moms=(0.95, 0.85), div_factor=10.0, pct_start=0.4, wd=0.001, beta2=0.99,
                 eps=1e-8, grad_norm_clip=1.0):
        import torch
        self.params = [p for p in params if p.requires_grad]
        self.total_steps, self.lr_max, self.moms, self.low = total_steps, lr_max, tuple(moms), lr_max / div_factor
        self.border, self.wd, self.beta2, self.clip, self.it = int(total_steps * pct_start), wd, beta2, grad_norm_clip, 0
        self.adam = torch.optim.Adam(self.params, lr=self.low, betas=(self.moms[0], beta2), eps=eps, weight_decay=0)
        self.last = None

    def schedule(self, it):
        import math
        it = min(it, self.total_steps - 1)

        def anneal(start, end, pct):
            return end + (start - end) / 2 * (math.cos(math.pi * pct) + 1)
        if it >= self.border:
            pct = (it - self.border) / (self.total_steps - self.border)
            return anneal(self.lr_max, self.low / 1e4, pct), anneal(self.moms[1], self.moms[0], pct)
        pct = it / self.border
        return anneal(self.low, self.lr_max, pct), anneal(self.moms[0], self.moms[1], pct)

    def zero_grad(self):
        self.adam.zero_grad()

    def step(self):
        import torch
        norm = torch.nn.utils.clip_grad_norm_(self.params, self.clip)
        lr, mom = self.schedule(self.it)
        self.it += 1
        for group in self.adam.param_groups:
            group["lr"], group["betas"] = lr, (mom, self.beta2)
        with torch.no_grad():
            for p in self.params:
                if p.requires_grad:
                    p.mul_(1 - self.wd * lr)
        self.adam.step()
        self.last = (norm, lr, mom)


def optim_rows(args, report):
    """one optimiser step over the two-stream model's parameter list (bench_step.build_model(image=True): 15.7 M parameters) with
    stored gradients: FusedAdamOneCycle (three launches) against ComposedAdamOneCycle, ALTERNATING inside one call; the gradients
    are put back outside the timed region (the fused step zeroes them, the composed clip scales them)"""
    import statistics
    import torch
    import bench_step
    from epnet_amd import optim
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model_f = bench_step.build_model(image=True).to(dev)
    model_c = bench_step.build_model(image=True).to(dev)
    model_c.load_state_dict(model_f.state_dict())
    steps = 2 * (3 + args.reps) + 1           # the pairs, then the bucket-view loop
    fused = optim.FusedAdamOneCycle(model_f, steps)
    params_f = fused.params
    name_of = {id(p): n for n, p in model_f.named_parameters()}
    by_name = dict(model_c.named_parameters())
    params_c = [by_name[name_of[id(p)]] for p in params_f]
    composed = ComposedAdamOneCycle(params_c, steps)
    g = torch.Generator(device=dev).manual_seed(1)
    master = [torch.randn(p.shape, generator=g, device=dev) * 1e-3 for p in params_f]
    for p, q, m in zip(params_f, params_c, master):
        p.grad, q.grad = m.clone(), m.clone()
    grads_f, grads_c = [p.grad for p in params_f], [q.grad for q in params_c]
    n = sum(p.numel() for p in params_f)

    def bucket_views():
        """move params_f's gradients into one flat bucket, each at element offset 1, 2 or 3 (mod 4)"""
        at, slots = 0, []
        for k, p in enumerate(params_f):
            at = (at + 3) // 4 * 4 + 1 + k % 3
            slots.append(at)
            at += p.numel()
        bucket = torch.zeros((at + 4,), device=dev)
        for p, slot in zip(params_f, slots):
            p.grad = bucket[slot:slot + p.numel()].view(p.shape)
        return [p.grad for p in params_f]
    if args.optim_side == "fused_views":
        grads_f = bucket_views()

    def refill():
        torch._foreach_copy_(grads_f, master)
        torch._foreach_copy_(grads_c, master)
        torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    sides = {"both": (True, True), "fused": (True, False), "fused_views": (True, False), "composed": (False, True)}[args.optim_side]
    tf, tc = [], []
    for k in range(3 + args.reps):
        refill()
        a = timed(fused.step) if sides[0] else 0.0
        b = timed(composed.step) if sides[1] else 0.0
        if k == 0 and all(sides):   # one step from the same state: the two forms differ in rounding order only
            diff = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(params_f, params_c))
        if k >= 3:
            tf.append(a); tc.append(b)
    stats = fused.stats.tolist()
    shape = {"tensors": len(params_f), "parameters": n, "reps": args.reps}
    if not all(sides):       # one side alone, for a kernel trace: its own op name, and no bytes claimed for the composition
        side_ms = statistics.median(tf) if sides[0] else statistics.median(tc)
        return report("adam_onecycle_step/%s_alone" % args.optim_side, shape, side_ms, n * 36 if sides[0] else 0,
                      "side %s only (for a kernel trace)" % args.optim_side)
    report("adam_onecycle_step", shape, statistics.median(tf), n * 36,
           "three launches, no host scalar; composed (clip_grad_norm_ + %d decay mul_ + stock Adam + host schedule): %.4f ms; fused lower in "
           "%d of %d alternating pairs; max |p_fused - p_composed| after the first step %.2e; total_norm %.6f coef %.6f; algorithmic bytes: "
           "4 (norm) + 16 read + 12 written + 4 (gradient zeroed) per parameter"
           % (len(params_c), statistics.median(tc), sum(a < b for a, b in zip(tf, tc)), len(tf), diff, stats[0], stats[1]))
    # the same step with every gradient a view at element offset 1, 2 or 3 (mod 4) of one flat bucket, as
    # DistributedDataParallel(gradient_as_bucket_view=True) lays them out: g goes through dword accesses, p / m / v stay 16-byte
    views = bucket_views()
    tv = []
    for k in range(3 + args.reps):           # the first step rebuilds the device tables; it is one of the three warm-up steps
        torch._foreach_copy_(views, master)
        torch.cuda.synchronize()
        ms = timed(fused.step)
        if k >= 3:
            tv.append(ms)
    report("adam_onecycle_step/bucket_views", shape, statistics.median(tv), n * 36,
           "the same step with every gradient a view at element offset 1, 2 or 3 (mod 4) of one flat bucket: g in dword accesses, "
           "p / m / v 16-byte; in a loop of its own after the pairs above (fused with gradient tensors of their own there: %.4f ms)"
           % statistics.median(tf))


def optim_scaled_rows(args, report):
    """the optimiser step with dynamic loss scaling on the same parameter list: FusedAdamOneCycle(loss_scale="dynamic") (three
    launches) against its stock composition -- what torch.amp.GradScaler runs around today's fused step, WITHOUT the host read of
    found_inf that GradScaler.step adds (so the comparator is sync-free too): found_inf and 1 / scale as GradScaler makes them,
    torch._amp_foreach_non_finite_check_and_unscale_, FusedAdamOneCycle.step(), torch._amp_update_scale_. ALTERNATING inside one
    call, the median of --reps per side, two passes; the gradients (finite, 65536 x those of optim_rows) are put back outside the
    timed region."""
    import statistics
    import torch
    import bench_step
    from epnet_amd import optim
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model_f = bench_step.build_model(image=True).to(dev)
    model_c = bench_step.build_model(image=True).to(dev)
    model_c.load_state_dict(model_f.state_dict())
    steps = 2 * (3 + args.reps)
    scaled = optim.FusedAdamOneCycle(model_f, steps, loss_scale="dynamic")
    plain = optim.FusedAdamOneCycle(model_c, steps)
    params_f, params_c = scaled.params, plain.params
    g = torch.Generator(device=dev).manual_seed(1)
    master = [torch.randn(p.shape, generator=g, device=dev) * (1e-3 * 65536.0) for p in params_f]
    for p, q, m in zip(params_f, params_c, master):
        p.grad, q.grad = m.clone(), m.clone()
    grads_f, grads_c = [p.grad for p in params_f], [q.grad for q in params_c]
    n = sum(p.numel() for p in params_f)
    scale = torch.full((1,), 65536.0, device=dev)
    tracker = torch.zeros((1,), dtype=torch.int32, device=dev)

    def composed_step():
        found = torch.full((), 0.0, dtype=torch.float32, device=dev)
        inv = scale.double().reciprocal().float()
        torch._amp_foreach_non_finite_check_and_unscale_(grads_c, found, inv)
        plain.step()
        torch._amp_update_scale_(scale, tracker, found, 2.0, 0.5, 2000)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    sides = {"scaled": (True, True), "scaled_fused": (True, False), "scaled_composed": (False, True)}[args.optim_side]
    passes, same = [], None
    for _ in range(2):
        tf, tc = [], []
        for k in range(3 + args.reps):
            torch._foreach_copy_(grads_f, master)
            torch._foreach_copy_(grads_c, master)
            torch.cuda.synchronize()
            a = timed(scaled.step) if sides[0] else 0.0
            b = timed(composed_step) if sides[1] else 0.0
            if same is None and all(sides):   # one step from the same state: defined to be the same bits
                same = all(torch.equal(p, q) for p, q in zip(params_f, params_c))
            if k >= 3:
                tf.append(a); tc.append(b)
        passes.append((tf, tc))
    shape = {"tensors": len(params_f), "parameters": n, "reps": args.reps}
    if not all(sides):
        side = [statistics.median(t[0] if sides[0] else t[1]) for t in passes]
        return report("adam_onecycle_step_scaled/%s_alone" % args.optim_side, shape, statistics.median(side), n * 36 if sides[0] else 0,
                      "side %s only (for a kernel trace); medians of the two passes: %s" % (args.optim_side, ["%.4f" % v for v in side]))

    def quartiles(t):
        q = statistics.quantiles(t, n=4)
        return q[0], q[2]
    rows, faster = [], True
    for tf, tc in passes:
        mf, mc = statistics.median(tf), statistics.median(tc)
        lo, hi = quartiles(tc)
        faster = faster and mf < mc - (hi - lo)
        rows.append("scaled %.4f ms (min %.4f max %.4f), composition %.4f ms (min %.4f, quartiles %.4f .. %.4f, max %.4f), scaled lower in "
                    "%d of %d pairs" % (mf, min(tf), max(tf), mc, min(tc), lo, hi, max(tc), sum(a < b for a, b in zip(tf, tc)), len(tf)))
    stats = scaled.stats.tolist()
    report("adam_onecycle_step_scaled", shape, statistics.median(passes[0][0] + passes[1][0]), n * 36,
           "three launches, nothing read back, against unscale (torch._amp_foreach_non_finite_check_and_unscale_, with found_inf and "
           "1 / scale made as GradScaler makes them) + the plain fused step + torch._amp_update_scale_, no host read of found_inf on "
           "either side; pass 1: %s; pass 2: %s; below the composition by more than its interquartile range in both passes: %s; "
           "parameters after the first step bit-equal: %s; scale %g, skipped %d, tracker %d (composition: scale %g, tracker %d)"
           % (rows[0], rows[1], faster, same, stats[6], int(stats[7]), int(scaled.scaler_state[0]), float(scale), int(tracker)))


def targets_rows(args, report, timeit_pair):
    """the fused RPN training targets (augmentation + labels, one launch: epnet_amd/rpn_target_layer.py) against the stock
    composition bench_step.rpn_labels (labels only, (B,N,G,3) temporaries), alternating inside one call, at 2 / 16 / 256 scenes x
    16384 points x 20 box rows (12 real). The composition runs in chunks of scenes if it runs out of memory."""
    import torch
    import bench_step
    from epnet_amd import rpn_target_layer as rtl
    dev = torch.device("cuda:0")
    n, peak = 16384, 8e12
    for bsz in (2, 16, 256):
        xyz, gts = bench_step.synthetic_batch(bsz, n, 300, dev)
        g = gts.shape[1]
        alpha = (torch.rand((bsz, g), generator=torch.Generator().manual_seed(7)) * 6.28 - 3.14).to(dev) * (gts[:, :, 3] > 0)
        aug = rtl.draw_augmentation(bsz, rtl.default_cfg(), torch.Generator(device=dev).manual_seed(9), device=dev)
        chunk = [bsz]

        def composed():
            return [bench_step.rpn_labels(xyz[i:i + chunk[0]], gts[i:i + chunk[0]]) for i in range(0, bsz, chunk[0])]

        def fused():
            return rtl.augment_and_label(xyz, gts, alpha, aug)

        def labels_only():
            return rtl.rpn_training_labels(xyz, gts)
        while True:
            try:
                want = composed()
                break
            except torch.OutOfMemoryError:
                want = None
                torch.cuda.empty_cache()
                chunk[0] = max(1, chunk[0] // 2)
        # how often the two rules give the same class on the unaugmented cloud (they are different rules: the synthetic object
        # points lie ON the faces, where the composition counts a box as enlarged by 0.05 already; see bench_step.rpn_labels)
        cls, reg = labels_only()
        agree = float((torch.cat([w[0] for w in want]).view(-1) == cls.view(-1).long()).float().mean())
        counts = {k: int((cls == v).sum()) for k, v in (("fg", 1), ("ignored", -1))}
        counts["ignored_with_row"] = int(((cls == -1) & (reg.abs().sum(dim=2) > 0)).sum())
        del want
        ms_c, ms_f = timeit_pair(composed, fused)
        ms_c2, ms_l = timeit_pair(composed, labels_only)
        nbytes = bsz * n * 56 + bsz * g * 56
        report("rpn_targets", dict({"scenes": bsz, "N": n, "G": g}, **counts), ms_f, nbytes,
               "augmentation + labels, one launch, no host sync: %.3f of the 8 TB/s peak over B*N*56 + B*G*56 bytes; labels alone "
               "(no aug table, 44 bytes per point): %.4f ms; stock composition bench_step.rpn_labels (labels only, another rule, in chunks "
               "of %d scenes): %.4f ms (%.4f ms in the second pair); same class on %.4f of the points"
               % (nbytes / (ms_f * 1e-3) / peak, ms_l, chunk[0], ms_c, ms_c2, agree))


def composed_scan_prepare(pts_lidar, num_raw, V2C, R0, P2, img_shape, npoints=16384):
    """the reference's first half of get_rpn_with_li_fusion (kitti_rcnn_dataset.py:281-356) composed from stock torch on the
    device, in its shape: a matmul per transform, the masks, then per scene nonzero / randperm with the read-backs their
    data-dependent sizes force. Its draws are torch's, so only counts and sets can be compared with the fused call."""
    import torch
    b, p = pts_lidar.shape[0], pts_lidar.shape[1]
    hom = torch.cat([pts_lidar[:, :, 0:3], torch.ones_like(pts_lidar[:, :, 0:1])], dim=2)
    rect = torch.bmm(hom, torch.bmm(V2C.transpose(1, 2), R0.transpose(1, 2)))
    hom2 = torch.bmm(torch.cat([rect, torch.ones_like(rect[:, :, 0:1])], dim=2), P2.transpose(1, 2))
    uv = hom2[:, :, 0:2] / rect[:, :, 2:3]
    depth = hom2[:, :, 2] - P2[:, 2, 3:4]
    hw = img_shape.to(rect.dtype)
    flag = (uv[:, :, 0] >= 0) & (uv[:, :, 0] < hw[:, 1:2]) & (uv[:, :, 1] >= 0) & (uv[:, :, 1] < hw[:, 0:1]) & (depth >= 0)
    flag &= (rect[:, :, 0] >= -40) & (rect[:, :, 0] <= 40) & (rect[:, :, 1] >= -1) & (rect[:, :, 1] <= 3) & (rect[:, :, 2] >= 0) & (rect[:, :, 2] <= 70.4)
    flag &= torch.arange(p, device=rect.device)[None, :] < num_raw[:, None]
    out = []
    for k in range(b):
        rows = flag[k].nonzero().view(-1)                                    # a read-back: the size depends on the data
        z = rect[k, rows, 2]
        if npoints < rows.numel():
            far, near = (z >= 40.0).nonzero().view(-1), (z < 40.0).nonzero().view(-1)
            pick = near[torch.randperm(near.numel(), device=rect.device)[:npoints - far.numel()]]
            choice = torch.cat([pick, far])
        else:
            choice = torch.arange(rows.numel(), device=rect.device)
            if npoints > rows.numel():
                choice = torch.cat([choice, choice[torch.randperm(rows.numel(), device=rect.device)[:npoints - rows.numel()]]])
        choice = rows[choice[torch.randperm(choice.numel(), device=rect.device)]]
        out.append((rect[k, choice], pts_lidar[k, choice, 3] - 0.5, uv[k, choice], choice))
    return (torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out]), torch.stack([o[2] for o in out]),
            torch.stack([o[3] for o in out]))


def scan_rows(args, report, timeit_pair):
    """the fused RPN inputs from raw scans (epnet_amd/scan_layer.py, four launches) against composed_scan_prepare, alternating
    inside one call, at 2 / 16 / 256 scenes of 122 880 raw points -> 16384; and normalise_images against .double() arithmetic
    plus .float() on the device"""
    import torch
    from epnet_amd import scan_layer, synth
    dev = torch.device("cuda:0")
    p, n, peak = 122880, 16384, 8e12
    base = [synth.lidar_scan(p - 1500 * k, seed=60 + k) for k in range(8)]
    for bsz in (2, 16, 256):
        pts, num_raw = scan_layer.collate_scans([base[k % 8] for k in range(bsz)])
        assert pts.shape[1] == p
        pts, num_raw = pts.to(dev), num_raw.to(dev)
        cal = [synth.calibration(k % 8) for k in range(bsz)]
        V2C, R0, P2, shape = (torch.stack([c[j] for c in cal]).to(dev) for j in range(4))
        tables = scan_layer.draw_scan_tables(bsz, p, n, torch.Generator(device=dev).manual_seed(11), dev)

        def fused():
            return scan_layer.prepare_scans(pts, num_raw, V2C, R0, P2, shape, tables, npoints=n)

        def fused_fresh_tables():
            return scan_layer.prepare_scans(pts, num_raw, V2C, R0, P2, shape, scan_layer.draw_scan_tables(bsz, p, n, None, dev), npoints=n)

        def composed():
            return composed_scan_prepare(pts, num_raw, V2C, R0, P2, shape, n)
        got, want = fused(), composed()
        info = got["scene_info"].cpu()
        # the two draw differently; what must agree: every far point is in both, and both pick valid points only
        same_far = all(torch.equal(torch.sort(got["choice"][k][got["pts_rect"][k, :, 2] >= 40].long())[0],
                                   torch.sort(want[3][k][want[0][k, :, 2] >= 40])[0]) for k in range(min(bsz, 4)))
        if not same_far:
            print("WARNING: scan_prepare at %d scenes: the fused call and the composition disagree on the far points" % bsz, file=sys.stderr, flush=True)
        ms_c, ms_f = timeit_pair(composed, fused)
        ms_c2, ms_t = timeit_pair(composed, fused_fresh_tables)
        nbytes = bsz * p * 20 + bsz * n * 44
        report("scan_prepare", {"scenes": bsz, "P": p, "N": n, "valid": info[:4, 1].tolist(), "far": info[:4, 2].tolist(),
                                "cases": sorted(set(info[:, 3].tolist())), "launches": 4}, ms_f, nbytes,
               "classify + plan + count + emit, no host sync: %.3f of the 8 TB/s peak over B*P*20 + B*N*44 bytes; with the tables drawn "
               "in the call (randint + rand + argsort): %.4f ms; stock composition (bmm, masks, per-scene nonzero / randperm with "
               "read-backs; its launches were not counted, by its statements about 12 + 8 per scene): %.4f ms (%.4f ms in the second pair); same far points in both: %s"
               % (nbytes / (ms_f * 1e-3) / peak, ms_t, ms_c, ms_c2, same_far))
    mean, std = torch.tensor(scan_layer.MEAN, dtype=torch.float64, device=dev), torch.tensor(scan_layer.STD, dtype=torch.float64, device=dev)
    for bsz in (2, 16, 64):
        img = torch.randint(0, 256, (bsz, 375, 1242, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(3))

        def fused_img():
            return scan_layer.normalise_images(img)

        def composed_img():
            back = torch.zeros((bsz, 384, 1280, 3), dtype=torch.float64, device=dev)
            back[:, :375, :1242] = (img.double() / 255.0 - mean) / std
            return back.float().permute(0, 3, 1, 2).contiguous()
        same = bool(torch.equal(fused_img(), composed_img()))
        if not same:
            print("WARNING: image_normalise at %d scenes: the fused call and the float64 composition differ" % bsz, file=sys.stderr, flush=True)
        ms_c, ms_f = timeit_pair(composed_img, fused_img)
        nbytes = bsz * (375 * 1242 * 3 + 3 * 384 * 1280 * 4)
        report("image_normalise", {"scenes": bsz, "in": [375, 1242], "out": [384, 1280], "launches": 1}, ms_f, nbytes,
               "8-bit image -> normalised NCHW fp32, one launch: %.3f of the 8 TB/s peak over the bytes read and written; float64 "
               "arithmetic on the device + .float() + permute: %.4f ms; same bits: %s" % (nbytes / (ms_f * 1e-3) / peak, ms_c, same))


def handover_rows(args, report, timeit_pair):
    """the one-call RPN hand-over (epnet_amd/rpn_handover.py: one decode launch, one order launch, then the proposal kernels)
    against the existing ProposalLayer.forward (stock decoding and sort in front of the same proposal kernels), alternating inside
    one call, at 1 / 2 / 16 / 256 scenes x 16384 x 76 with the TRAIN and the TEST budgets; then the two new kernels on their own
    against the stock ops they replace. The whole table is measured twice: the fused call counts as faster at a size only if its
    median is below the composition's in both runs AND the gap exceeds the difference between the composition's own two medians.
    --handover-side runs one side alone (what a kernel trace of launches per call needs)."""
    import torch
    from epnet_amd import bbox_transform, proposal_layer, rpn_handover, synth
    dev = torch.device("cuda:0")
    n, c, peak = 16384, 76, 8e12
    cfg = proposal_layer.default_cfg()
    base = synth.scenes("kitti", 8, n, seed=40)
    size = torch.from_numpy(cfg.CLS_MEAN_SIZE[0].copy()).to(dev)
    rows_out = {}
    sizes = [int(v) for v in args.handover_scenes.split(",")]
    for run in (1, 2) if args.handover_side == "both" else (1,):
        for bsz in sizes:
            gen = torch.Generator(device=dev).manual_seed(41 + bsz)
            xyz = base[[k % 8 for k in range(bsz)]].contiguous().to(dev)
            reg = torch.randn((bsz, n, c), generator=gen, device=dev).half().float()
            scores = torch.randn((bsz, n), generator=gen, device=dev) * 3
            for mode in ("TRAIN", "TEST"):
                stock = proposal_layer.ProposalLayer(mode, cfg=cfg).to(dev)

                def composed():
                    return stock(scores, reg, xyz)

                def composed_all():        # lib/net/point_rcnn.py:44-52 on the existing layer
                    rois, raw = stock(scores, reg, xyz)
                    return rois, raw, (torch.sigmoid(scores) > 0.3).float(), torch.norm(xyz, p=2, dim=2)

                def fused():
                    return rpn_handover.rpn_handover(scores, reg, xyz, cfg=cfg, mode=mode)
                if args.handover_side != "both":
                    fn = fused if args.handover_side == "fused" else composed
                    for _ in range(args.reps):
                        fn()
                    torch.cuda.synchronize()
                    continue
                got, want = fused(), composed()
                same_count = bool(torch.equal(got.roi_count, (want[1] != 0).sum(dim=1).int()))
                ms_c, ms_f = timeit_pair(composed, fused)
                ms_a, ms_f2 = timeit_pair(composed_all, fused)
                nbytes = bsz * n * ((c + 4) * 4 + 9 * 4 + 8)
                rows_out[(bsz, mode, run)] = (ms_c, ms_f)
                report("rpn_handover", {"scenes": bsz, "N": n, "C": c, "mode": mode, "run": run, "launches": 6}, ms_f, nbytes,
                       "decode + mask + depth (1 launch), order (1), bin / NMS mask / sweep / emit (4), no host sync; the existing "
                       "ProposalLayer.forward (stock decoding + torch.sort + the same proposal kernels): %.4f ms; that plus the stock "
                       "sigmoid / threshold / norm of point_rcnn.py:44-52: %.4f ms against %.4f ms in the same pair; kept counts equal: %s"
                       % (ms_c, ms_a, ms_f2, same_count))
            if args.handover_side != "both":
                continue
            # the two new kernels on their own
            flat_xyz, flat_reg = xyz.view(-1, 3), reg.view(-1, c)
            kw = dict(loc_scope=3.0, loc_bin_size=0.5, num_head_bin=12, get_xz_fine=True, get_y_by_bin=False, get_ry_fine=False,
                      bbox_avg_by_bin=True, ry_with_bin=False)
            ms_c, ms_f = timeit_pair(lambda: bbox_transform.decode_bbox_target(flat_xyz, flat_reg, anchor_size=size, **kw),
                                     lambda: rpn_handover.decode_boxes(flat_xyz, flat_reg, anchor_size=cfg.CLS_MEAN_SIZE[0], **kw))
            nbytes = bsz * n * ((c + 3) * 4 + 7 * 4)
            report("decode_bbox_target", {"rows": bsz * n, "C": c, "run": run, "launches": 1}, ms_f, nbytes,
                   "one launch: %.3f of the 8 TB/s peak over rows * (C + 3 + 7) * 4 bytes; stock bbox_transform.decode_bbox_target: %.4f ms"
                   % (nbytes / (ms_f * 1e-3) / peak, ms_c))
            ms_c, ms_f = timeit_pair(lambda: torch.sort(scores, dim=1, descending=True)[1], lambda: rpn_handover.score_order(scores))
            report("score_order", {"scenes": bsz, "N": n, "run": run, "launches": 1}, ms_f, bsz * n * 12,
                   "one workgroup per scene, keys sorted in LDS, stable; torch.sort(descending)[1]: %.4f ms" % ms_c)
    for bsz in sizes:
        for mode in ("TRAIN", "TEST"):
            if (bsz, mode, 1) not in rows_out:
                continue
            (c1, f1), (c2, f2) = rows_out[(bsz, mode, 1)], rows_out[(bsz, mode, 2)]
            spread = abs(c1 - c2)
            faster = f1 < c1 and f2 < c2 and min(c1 - f1, c2 - f2) > spread
            print(json.dumps({"op": "rpn_handover verdict", "scenes": bsz, "mode": mode, "composed_ms": [round(c1, 4), round(c2, 4)],
                              "fused_ms": [round(f1, 4), round(f2, 4)], "composed_spread_ms": round(spread, 4), "fused_is_faster": bool(faster)}),
                  flush=True)


def rcnn_targets_rows(args, report, timeit_pair):
    """the sync-free RCNN target layer (epnet_amd/rcnn_target_layer.py: epnet_rcnn_sample_rois + epnet_roipool3d_train, device
    tables) against the existing ProposalTargetLayer (host random streams, two read-backs), alternating inside one call, at
    1 / 2 / 16 scenes x 512 ROIs x 20 box rows (12 real) x 16384 points x 130 feature columns, R = 64, S = 512; then the two
    calls of the new layer on their own"""
    import torch
    from epnet_amd import proposal_target_layer as ptl, rcnn_target_layer as rtl, synth
    dev = torch.device("cuda:0")
    m, n, g_rows, r, s_num, c = 512, 16384, 20, 64, 512, 130
    g = torch.Generator().manual_seed(0)
    for bsz in (1, 2, 16):
        rl, gl = [], []
        for i in range(bsz):
            bx, _ = synth.proposal_boxes(m + 12, seed=200 + i, num_objects=12, jitter=0.4)
            gt = torch.zeros((g_rows, 7)); gt[:12] = bx[m:]
            rl.append(bx[:m]); gl.append(gt)
        layer_in = {"roi_boxes3d": torch.stack(rl).to(dev), "gt_boxes3d": torch.stack(gl).to(dev),
                    "rpn_xyz": synth.scenes("kitti", bsz, n, seed=9).to(dev), "rpn_features": torch.randn((bsz, n, c - 2), generator=g).to(dev),
                    "seg_mask": (torch.rand((bsz, n), generator=g) > 0.5).float().to(dev), "pts_depth": (torch.rand((bsz, n), generator=g) * 70).to(dev)}
        host_layer, fused_layer = ptl.ProposalTargetLayer(), rtl.RCNNTargetLayer()
        cfg = fused_layer.cfg
        ms_host, ms_fused = timeit_pair(lambda: host_layer(layer_in), lambda: fused_layer(layer_in))
        tables = rtl.draw_sampling_tables(bsz, m, cfg, dev)
        feat = torch.cat([layer_in["seg_mask"].unsqueeze(2), (layer_in["pts_depth"] / 70.0 - 0.5).unsqueeze(2), layer_in["rpn_features"]], dim=2)
        sampled = rtl.sample_rois(layer_in["roi_boxes3d"], layer_in["gt_boxes3d"], tables, cfg)
        ms_draw, ms_sample = timeit_pair(lambda: rtl.draw_sampling_tables(bsz, m, cfg, dev),
                                         lambda: rtl.sample_rois(layer_in["roi_boxes3d"], layer_in["gt_boxes3d"], tables, cfg))
        ms_cat, ms_pool = timeit_pair(lambda: torch.cat([layer_in["seg_mask"].unsqueeze(2), (layer_in["pts_depth"] / 70.0 - 0.5).unsqueeze(2),
                                                         layer_in["rpn_features"]], dim=2),
                                      lambda: rtl.pool_targets(layer_in["rpn_xyz"], feat, sampled[0], sampled[1], sampled[2], tables["aug"], cfg))
        info = sampled[3].tolist()
        sample_bytes = bsz * (m * 28 + g_rows * 7 * 4 + m * 4 + r * 4) + bsz * r * (28 + 28 + 4) + bsz * 24
        pool_bytes = bsz * (n * 12 + n * c * 4 + r * (28 * 2 + 4 + 12) + r * s_num * (3 + c) * 4 + r * (28 * 2 + 16))
        report("RCNNTargetLayer.forward", {"B": bsz, "proposals": m, "G": g_rows, "rois": r, "N": n, "C": c, "S": s_num,
                                           "fg_num": [row[1] for row in info]}, ms_fused, pool_bytes + sample_bytes,
               "device tables + epnet_rcnn_sample_rois + feature cat + epnet_roipool3d_train, no host sync; the existing ProposalTargetLayer "
               "(host random streams, two read-backs) in the same pair: %.4f ms; on their own: table draws %.4f ms, sample_rois %.4f ms "
               "(%d bytes of inputs, tables and outputs, noise tables and the IoU matrix aside), feature cat %.4f ms, pool_targets %.4f ms"
               % (ms_host, ms_draw, ms_sample, sample_bytes, ms_cat, ms_pool))


def rows16_rows(args, timeit_pair):
    """the native 16-bit kernels (csrc/rows16.hip) against their float32 twins -- unchanged code moving twice the feature bytes --
    and against the upcast composition (x.float() -> float32 op -> .to(T)), on the SA / FP level shapes of configs 3 and 4 at 2 and
    16 scenes. Every pair alternates inside one call, median of --reps by HIP events; native against twin twice (two passes)."""
    import torch
    from epnet_amd import pointnet2_cuda as p2
    dev, T, f32, i32 = torch.device("cuda:0"), torch.bfloat16, torch.float32, torch.int32
    g = torch.Generator(device=dev).manual_seed(0)
    PEAK = 8.0e12

    def line(op, shape, native, twin, upcast, nbytes, twin_bytes):
        spread = abs(twin[0] - twin[1])
        faster_twin = all(n < t - spread for n, t in zip(native, twin))
        best = min(native)
        print(json.dumps({"op": op + "_h", "dtype": "bf16", "shape": shape, "ms_native": [round(v, 4) for v in native],
                          "ms_f32_twin": [round(v, 4) for v in twin], "twin_spread_ms": round(spread, 4), "ms_upcast_composition": round(upcast[1], 4),
                          "ms_native_beside_upcast": round(upcast[0], 4), "algorithmic_bytes": nbytes, "twin_algorithmic_bytes": twin_bytes,
                          "share_of_8TBps": round(nbytes / (best * 1e-3) / PEAK, 3), "twin_share_of_8TBps": round(twin_bytes / (min(twin) * 1e-3) / PEAK, 3),
                          "faster_than_twin": bool(faster_twin), "faster_than_upcast": bool(upcast[0] < upcast[1])}), flush=True)

    for scenes in (2, 16):
        clouds = scenes * 64                               # ROIs of the RCNN stage
        # ---- group_linear: (b, c, n, npoint, ns) of the foldable levels (RPN levels 2-4, RCNN levels 1-2)
        for tag, (b, c, n, m, ns) in (("rpn2/16", (scenes, 64, 4096, 1024, 16)), ("rpn2/32", (scenes, 64, 4096, 1024, 32)),
                                      ("rpn3/32", (scenes, 128, 1024, 256, 32)), ("rpn4/32", (scenes, 256, 256, 64, 32)),
                                      ("rcnn1", (clouds, 128, 512, 128, 64)), ("rcnn2", (clouds, 128, 128, 32, 64))):
            xyz = torch.rand((b, n, 3), generator=g, device=dev)
            new_xyz = xyz[:, :m].contiguous()
            idx = torch.randint(0, n, (b, m, ns), generator=g, device=dev, dtype=i32)
            z32 = torch.randn((b, c, n), generator=g, device=dev)
            z16 = z32.to(T)
            w, bias = torch.randn((c, 3), generator=g, device=dev), torch.randn((c,), generator=g, device=dev)
            o16, o32 = torch.empty((b, c, m, ns), dtype=T, device=dev), torch.empty((b, c, m, ns), dtype=f32, device=dev)
            native = lambda: p2.group_linear_h_wrapper(b, c, n, m, ns, xyz, new_xyz, z16, idx, w, bias, o16)          # noqa: E731
            twin = lambda: p2.group_linear_wrapper(b, c, n, m, ns, xyz, new_xyz, z32, idx, w, bias, o32)                # noqa: E731

            def upcast():
                p2.group_linear_wrapper(b, c, n, m, ns, xyz, new_xyz, z16.float(), idx, w, bias, o32)
                return o32.to(T)
            a, bb = timeit_pair(native, twin), timeit_pair(native, twin)
            per = lambda e: b * (c * n * e + n * 12 + m * 12 + m * ns * 4 + c * m * ns * e)                             # noqa: E731
            line("group_linear", {"level": tag, "scenes": scenes, "b": b, "c": c, "n": n, "npoint": m, "ns": ns}, (a[0], bb[0]), (a[1], bb[1]),
                 timeit_pair(native, upcast), per(2), per(4))
            del z32, z16, o16, o32
        # ---- pool_max and its gradient: (rows, ns)
        for tag, (rows, ns) in (("rpn1/16", (scenes * 32 * 4096, 16)), ("rpn1/32", (scenes * 64 * 4096, 32)), ("rpn2/32", (scenes * 128 * 1024, 32)),
                                ("rcnn1", (clouds * 128 * 128, 64)), ("rcnn3", (clouds * 512, 32))):
            x32 = torch.randn((rows, ns), generator=g, device=dev)
            x16 = x32.to(T)
            o16, o32 = torch.empty((rows,), dtype=T, device=dev), torch.empty((rows,), dtype=f32, device=dev)
            arg = torch.empty((rows,), dtype=i32, device=dev)
            native = lambda: p2.pool_max_h_wrapper(rows, ns, x16, o16, arg)            # noqa: E731
            twin = lambda: p2.pool_max_wrapper(rows, ns, x32, o32, arg)                # noqa: E731

            def upcast():
                p2.pool_max_wrapper(rows, ns, x16.float(), o32, arg)
                return o32.to(T)
            a, bb = timeit_pair(native, twin), timeit_pair(native, twin)
            line("pool_max", {"level": tag, "scenes": scenes, "rows": rows, "ns": ns}, (a[0], bb[0]), (a[1], bb[1]), timeit_pair(native, upcast),
                 rows * (ns * 2 + 2 + 4), rows * (ns * 4 + 4 + 4))
            g16, g32 = torch.randn((rows,), generator=g, device=dev).to(T), torch.randn((rows,), generator=g, device=dev)
            native = lambda: p2.pool_max_grad_h_wrapper(rows, ns, g16, arg, x16)       # noqa: E731  (x16 / x32 reused as grad_x)
            twin = lambda: p2.pool_max_grad_wrapper(rows, ns, g32, arg, x32)           # noqa: E731

            def upcast():
                p2.pool_max_grad_wrapper(rows, ns, g16.float(), arg, x32)
                return x32.to(T)
            a, bb = timeit_pair(native, twin), timeit_pair(native, twin)
            line("pool_max_grad", {"level": tag, "scenes": scenes, "rows": rows, "ns": ns}, (a[0], bb[0]), (a[1], bb[1]),
                 timeit_pair(native, upcast), rows * (ns * 2 + 2 + 4), rows * (ns * 4 + 4 + 4))
            del x32, x16, o16, o32, g16, g32
        # ---- three_interpolate: (b, c, m, n) of the four FP levels
        for tag, (b, c, m, n) in (("fp1", (scenes, 256, 4096, 16384)), ("fp2", (scenes, 512, 1024, 4096)), ("fp3", (scenes, 512, 256, 1024)),
                                  ("fp4", (scenes, 1024, 64, 256))):
            p32 = torch.randn((b, c, m), generator=g, device=dev)
            p16 = p32.to(T)
            idx = torch.randint(0, m, (b, n, 3), generator=g, device=dev, dtype=i32)
            wt = torch.rand((b, n, 3), generator=g, device=dev)
            o16, o32 = torch.empty((b, c, n), dtype=T, device=dev), torch.empty((b, c, n), dtype=f32, device=dev)
            native = lambda: p2.three_interpolate_h_wrapper(b, c, m, n, p16, idx, wt, o16)      # noqa: E731
            twin = lambda: p2.three_interpolate_wrapper(b, c, m, n, p32, idx, wt, o32)          # noqa: E731

            def upcast():
                p2.three_interpolate_wrapper(b, c, m, n, p16.float(), idx, wt, o32)
                return o32.to(T)
            a, bb = timeit_pair(native, twin), timeit_pair(native, twin)
            per = lambda e: b * (c * m * e + n * 24 + c * n * e)                                   # noqa: E731
            line("three_interpolate", {"level": tag, "scenes": scenes, "b": b, "c": c, "m": m, "n": n}, (a[0], bb[0]), (a[1], bb[1]),
                 timeit_pair(native, upcast), per(2), per(4))
            del p32, p16, o16, o32


def kitti_eval_rows(args):
    """the AP evaluator (epnet_amd.kitti_eval) on a seeded synthetic set: median wall time of the whole get_official_eval_result
    (class Car) and of its phases, and the same set -- cut down to --kitti-eval-host-frames -- through the numpy restatement of
    the reference's loops (tests/kitti_eval_restate.py) on one host core. No reference figure exists: the reference evaluator
    is numba.cuda and cannot run on this hardware."""
    import statistics
    import time

    import torch
    from epnet_amd import kitti_eval, synth
    frames = args.kitti_eval_frames
    gts, dts = synth.kitti_eval_annos(frames, seed=3)
    shape = {"frames": frames, "gt": int(sum(len(a["name"]) for a in gts)), "dt": int(sum(len(a["name"]) for a in dts)), "class": "Car"}
    kitti_eval.get_official_eval_result(gts, dts, 0)   # warm-up
    whole = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        result, ret = kitti_eval.get_official_eval_result(gts, dts, 0)
        whole.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"op": "kitti_eval", "shape": shape, "ms": round(statistics.median(whole), 3), "reps": args.reps,
                      "note": "get_official_eval_result, wall time; Car 3d AP (moderate) %.4f" % ret["Car_3d_moderate"]}), flush=True)
    phases = {}
    for _ in range(args.reps):
        seconds = {}
        kitti_eval.get_official_eval_result(gts, dts, 0, _profile=seconds)
        for key, sec in seconds.items():
            phases.setdefault(key, []).append(sec * 1e3)
    for key in sorted(phases):
        print(json.dumps({"op": "kitti_eval/" + key, "shape": shape, "ms": round(statistics.median(phases[key]), 3), "reps": args.reps,
                          "note": "phase of get_official_eval_result, a device synchronisation either side"}), flush=True)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests"))
    import kitti_eval_restate
    n = min(frames, args.kitti_eval_host_frames)
    t0 = time.perf_counter()
    host_result, _ = kitti_eval_restate.get_official_eval_result(gts[:n], dts[:n], [0])
    host_ms = (time.perf_counter() - t0) * 1e3
    same = host_result == kitti_eval.get_official_eval_result(gts[:n], dts[:n], 0)[0]
    print(json.dumps({"op": "kitti_eval/numpy_restatement", "shape": {"frames": n, "gt": int(sum(len(a["name"]) for a in gts[:n])), "dt": int(sum(len(a["name"]) for a in dts[:n])),
                                "class": "Car"}, "ms": round(host_ms, 1), "reps": 1,
                      "note": "one host core, %d of %d frames; same result string as the GPU on these frames: %s" % (n, frames, same)}),
          flush=True)


def gt_aug_rows(args, report, timeit_pair):
    """GT-database augmentation (epnet_amd/gt_aug_layer.py: placement, points, sampling -- three calls, six launches) at 1 / 2 / 16 /
    256 scenes of 122 880 raw points -> 16384 on a synthetic database, the augmentation applied in every scene, alternating with
    scan_layer.prepare_scans on the same scans; and, for context only, the numpy restatement of one scene on one host core. Per-launch kernel times come from a run of
    this mode under a kernel trace (profiles/README.md), not from here."""
    import time
    import numpy as np
    import torch
    from epnet_amd import gt_aug_layer, scan_layer, synth
    dev = torch.device("cuda:0")
    p, n, e = 122880, 16384, 8192
    objects = synth.gt_database(200, seed=9)
    db = gt_aug_layer.GTDatabase.from_list(objects, dev)
    cfg = gt_aug_layer.default_cfg()
    base = [synth.lidar_scan(p - 1500 * k, seed=60 + k) for k in range(8)]
    scenes = [int(v) for v in args.gt_aug_scenes.split(",")]
    for bsz in scenes:
        pts, num_raw = scan_layer.collate_scans([base[k % 8] for k in range(bsz)])
        pts, num_raw = pts.to(dev), num_raw.to(dev)
        cal = [synth.calibration(k % 8) for k in range(bsz)]
        V2C, R0, P2, shape = (torch.stack([c[j] for c in cal]).to(dev) for j in range(4))
        gts = torch.zeros((bsz, 20, 7))
        for k in range(bsz):
            gts[k, :12] = synth.object_boxes(12, 40 + k % 8)
        gts, alpha = gts.to(dev), torch.zeros((bsz, 20), device=dev)
        count = torch.full((bsz,), 12, dtype=torch.int32, device=dev)
        plane = torch.tensor([[0.0, -1.0, 0.0, 1.65]] * bsz, dtype=torch.float64, device=dev)
        tables = gt_aug_layer.draw_tables(bsz, p, db, e, n, cfg, torch.Generator(device=dev).manual_seed(11), dev)
        tables["apply"] = torch.ones_like(tables["apply"])                 # every timed scene is augmented (GT_AUG_APPLY_PROB is not timed)
        plain_tables = {"keys": tables["keys"][:, :p].contiguous(), "slot_perm": tables["slot_perm"]}

        def fused():
            return gt_aug_layer.prepare_scans_gt_aug(pts, num_raw, V2C, R0, P2, shape, tables, db, gts, count, gts, alpha, count, plane,
                                                     npoints=n, extra_rows=e, cfg=cfg)

        def plain():
            return scan_layer.prepare_scans(pts, num_raw, V2C, R0, P2, shape, plain_tables, npoints=n)
        got = fused()
        info, scene_info = got["gt_aug_info"].cpu(), got["scene_info"].cpu()
        ms_p, ms_f = timeit_pair(plain, fused)
        row = {"scenes": bsz, "P": p, "E": e, "N": n, "objects": 200, "existing": 12, "launches": 6, "applied": int(info[:, 0].sum()),
               "accepted": info[:4, 4].tolist(), "overlap_rejections": info[:4, 5].tolist(), "capacity_rejections": int(info[:, 6].sum()),
               "extra_points": info[:4, 7].tolist(), "removed": scene_info[:4, 6].tolist()}
        if args.gt_aug_side == "fused":                                   # what a kernel trace of the launches per call needs
            for _ in range(args.reps):
                fused()
            torch.cuda.synchronize()
        report("prepare_scans_gt_aug", row, ms_f, bsz * (p * 20 + e * 36 + n * 44),
               "apply forced to 1 in every scene; placement + points + classify / plan / count / emit over P + E rows, no host sync; scan_layer.prepare_scans on the same "
               "scans, alternating: %.4f ms" % ms_p)
    if args.gt_aug_side == "fused":
        return
    # for context only: the restatement of ONE scene on one host core (numpy; the reference's own loop needs shapely and was not timed)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests"))
    import gt_aug_restate as gr
    host_db = gr.pack_database(objects)
    one = {k: v[0].cpu().numpy() for k, v in tables.items()}
    scene = dict(pts=pts[0].cpu().numpy(), num_raw=int(num_raw[0]), V2C=V2C[0].cpu().numpy(), R0=R0[0].cpu().numpy(), P2=P2[0].cpu().numpy(),
                 img_shape=shape[0].cpu().numpy(), all_boxes=gts[0, :12].cpu().numpy(), gt_boxes=gts[0, :12].cpu().numpy(),
                 gt_alpha=np.zeros(12, np.float32), plane=plane[0].cpu().numpy())
    assert int(one["apply"]) == 1                                          # the device rows above ran this scene with the same tables
    t0 = time.perf_counter()
    placed = gr.place(host_db, 1, one["extra_num"], one["cand"], scene["all_boxes"], scene["gt_boxes"], scene["gt_alpha"], scene["plane"], e)
    t1 = time.perf_counter()
    extra = gr.object_points(host_db, placed, e)
    out = gr.prepare_aug(scene["pts"], scene["num_raw"], scene["V2C"], scene["R0"], scene["P2"], scene["img_shape"], extra, placed["info"][7],
                         placed["remove_boxes"], placed["info"][4], one["keys"], one["slot_perm"], n)
    t2 = time.perf_counter()
    print(json.dumps({"op": "prepare_scans_gt_aug/numpy_restatement", "shape": {"scenes": 1, "P": p, "E": e, "N": n, "accepted": int(placed["info"][4]),
                                                                                "removed": int(out["scene_info"][6])},
                      "ms": round((t2 - t0) * 1e3, 1), "reps": 1,
                      "note": "one host core, one scene, for context only: the loop of tries %.1f ms (Python), points + removal + sampling %.1f ms "
                              "(numpy)" % ((t1 - t0) * 1e3, (t2 - t1) * 1e3)}), flush=True)


def image_head_rows(args, timeit_pair):
    """the end of the two-stream backbone alone at the yaml's widths, 384 x 1280, 16384 points per scene: the existing
    dense lines (DeConv x 4, concatenation, 1x1 convolution + batch norm + ReLU, Feature_Gather -- sampler="hip") against
    li_fusion.image_head_at_points, eval mode under no_grad. Alternating inside one call, median of --reps by HIP events, two
    passes; "faster" = below the dense side in both passes by more than the dense side's own spread between its passes. Peak
    allocated bytes of one call of each side, above what the inputs and weights hold."""
    import torch
    import torch.nn.functional as F
    from epnet_amd import li_fusion, rpn_backbone
    dev = torch.device("cuda:0")
    cfg = rpn_backbone.BackboneConfig()
    h, w, n = 384, 1280, 16384
    torch.manual_seed(0)
    deconvs = torch.nn.ModuleList([rpn_backbone.UpsampleDeConv(c, r, kernel_size=k, stride=k)
                                   for c, r, k in zip(cfg.img_channels[1:], cfg.deconv_reduce, cfg.deconv_kernels)])
    quarter = cfg.img_features_channel // 4
    conv, bn = torch.nn.Conv2d(sum(cfg.deconv_reduce), quarter, kernel_size=1), torch.nn.BatchNorm2d(quarter)
    with torch.no_grad():
        bn.running_mean.normal_(0.0, 0.3)
        bn.running_var.uniform_(0.5, 2.0)
    deconvs, conv, bn = deconvs.to(dev).eval(), conv.to(dev).eval(), bn.to(dev).eval()
    packed = li_fusion.pack_image_head(deconvs, conv, bn)
    g = torch.Generator().manual_seed(1)
    for bsz in [int(v) for v in args.image_head_scenes.split(",")]:
        maps = [torch.randn((bsz, c, h // k, w // k), generator=g).to(dev) for c, k in zip(cfg.img_channels[1:], cfg.deconv_kernels)]
        xy = (torch.rand((bsz, n, 2), generator=g) * 2.0 - 1.0).to(dev)
        assert li_fusion.supports_image_head_at_points(deconvs, conv, bn, maps)

        def dense():
            with torch.no_grad():
                up = torch.cat([deconvs[i](maps[i]) for i in range(len(deconvs))], dim=1)
                img_fusion = F.relu(bn(conv(up)))
                return li_fusion.Feature_Gather(img_fusion, xy)

        def points():
            return li_fusion.image_head_at_points(maps, packed, xy)

        def peak(fn):
            fn()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            held = torch.cuda.memory_allocated(dev)
            out = fn()
            torch.cuda.synchronize()
            top = torch.cuda.max_memory_allocated(dev) - held
            del out
            return int(top)

        shape = {"B": bsz, "N": n, "H": h, "W": w, "C": cfg.img_channels[1:], "R": cfg.deconv_reduce, "q": quarter}
        if args.amp != "off":
            # --amp: the dense lines under torch.autocast on 16-bit maps against the 16-bit points head on the same maps; the
            # float32 points head (on the same values as float32) beside them for the record
            low = torch.float16 if args.amp == "fp16" else torch.bfloat16
            maps32, maps = [m.to(low).float() for m in maps], [m.to(low) for m in maps]
            assert li_fusion.supports_image_head_at_points(deconvs, conv, bn, maps, rows16=True)
            dense32 = dense

            def dense():
                with torch.autocast("cuda", low):
                    return dense32()

            def points32():
                return li_fusion.image_head_at_points(maps32, packed, xy)
        if args.image_head_side != "both":
            fn = points if args.image_head_side == "points" else dense
            for _ in range(args.reps):
                fn()
            torch.cuda.synchronize()
            print(json.dumps({"op": "image_head/%s_alone" % args.image_head_side, "shape": shape, "calls": args.reps}), flush=True)
            continue
        if args.amp != "off":
            diff = float((dense().float() - points().float()).abs().max())
            diff32 = float((points32() - points().float()).abs().max())
            peak_d, peak_p, peak_p32 = peak(dense), peak(points), peak(points32)
            (d1, p1), (d2, p2) = timeit_pair(dense, points), timeit_pair(dense, points)
            (f1, _), (f2, _) = timeit_pair(points32, points), timeit_pair(points32, points)
            spread = abs(d1 - d2)
            faster = p1 < d1 and p2 < d2 and min(d1 - p1, d2 - p2) > spread
            print(json.dumps({"op": "image_head16", "amp": args.amp, "shape": shape, "ms_dense_autocast": [round(d1, 4), round(d2, 4)],
                              "ms_points16": [round(p1, 4), round(p2, 4)], "ms_points_f32": [round(f1, 4), round(f2, 4)],
                              "dense_spread_ms": round(spread, 4), "points16_is_faster": bool(faster), "peak_bytes_dense_autocast": peak_d,
                              "peak_bytes_points16": peak_p, "peak_bytes_points_f32": peak_p32, "max_abs_diff_dense_points16": diff,
                              "max_abs_diff_points_f32_points16": diff32, "reps": args.reps}), flush=True)
            del maps, maps32, xy
            torch.cuda.empty_cache()
            continue
        diff = float((dense() - points()).abs().max())
        peak_d, peak_p = peak(dense), peak(points)
        (d1, p1), (d2, p2) = timeit_pair(dense, points), timeit_pair(dense, points)
        spread = abs(d1 - d2)
        faster = p1 < d1 and p2 < d2 and min(d1 - p1, d2 - p2) > spread
        print(json.dumps({"op": "image_head", "shape": shape, "ms_dense": [round(d1, 4), round(d2, 4)], "ms_points": [round(p1, 4), round(p2, 4)],
                          "dense_spread_ms": round(spread, 4), "points_is_faster": bool(faster), "peak_bytes_dense": peak_d,
                          "peak_bytes_points": peak_p, "max_abs_diff": diff, "reps": args.reps}), flush=True)
        del maps, xy
        torch.cuda.empty_cache()


def sa_tail_rows(args, timeit_pair):
    """the end of every SA level's shared MLP alone, per level and scale of configs 3 / 4 (16384 points per scene, the
    yaml's widths) and of the RCNN stage's SA stack (100 ROIs per scene): the stock lines -- [batch norm,] ReLU of the unit before the
    last, then convolution, [batch norm,] ReLU and pool_max -- against pointnet2_utils.sa_tail on the same pre-activation, eval mode
    under no_grad. Alternating inside one call, median of --reps by HIP events, two passes; "faster" = below the stock side in both
    passes by more than the stock side's own spread between its passes. share_of_8TBps: (x + y + w bytes) / fused time / 8 TB/s."""
    import torch
    import bench_step
    from epnet_amd import pointnet2_utils as p2u, pytorch_utils as pt_utils, rpn_backbone
    dev = torch.device("cuda:0")
    cfg = rpn_backbone.BackboneConfig()
    rows, cin = [], 0
    for level in range(len(cfg.npoints)):
        for scale, (spec, ns) in enumerate(zip(cfg.mlps[level], cfg.nsample[level])):
            rows.append(("rpn level %d scale %d" % (level + 1, scale + 1), [cin + 3] + list(spec), cfg.use_bn, 1, cfg.npoints[level], ns))
        cin = sum(m[-1] for m in cfg.mlps[level])
    cin, rois = 128, 100
    for level, spec in enumerate(bench_step.RCNN_MLPS):
        group_all = bench_step.RCNN_NPOINTS[level] is None
        rows.append(("rcnn level %d" % (level + 1), [cin + 3] + list(spec), False, rois, 1 if group_all else bench_step.RCNN_NPOINTS[level],
                     bench_step.RCNN_NPOINTS[level - 1] if group_all else bench_step.RCNN_NSAMPLE[level]))
        cin = spec[-1]
    g = torch.Generator(device=dev).manual_seed(1)
    for bsz in [int(v) for v in args.sa_tail_scenes.split(",")]:
        for name, spec, bn, per_scene, p, ns in rows:
            torch.manual_seed(0)
            mlp = pt_utils.SharedMLP(list(spec), bn=bn)
            with torch.no_grad():
                for m in mlp.modules():
                    if isinstance(m, torch.nn.BatchNorm2d):
                        m.running_mean.normal_(0.0, 0.3)
                        m.running_var.uniform_(0.5, 2.0)
            mlp = mlp.to(dev).eval()
            packed = p2u.pack_sa_tail(mlp)
            flat = [layer for unit in mlp.children() for layer in unit.children()]
            tail = flat[len(flat) - packed.replaced:]
            b, k, c = bsz * per_scene, spec[-2], spec[-1]
            x = torch.randn((b, k, p, ns), generator=g, device=dev)    # up to 6.7 GB (RCNN level 1 at 16 scenes): drawn on the device

            def stock():
                with torch.no_grad():
                    h = x
                    for layer in tail:
                        h = layer(h)
                    return p2u.pool_max(h).squeeze(-1)

            def fused():
                return p2u.sa_tail(x, packed)

            shape = {"scenes": bsz, "B": b, "K": k, "C": c, "P": p, "S": ns, "bn": bool(bn)}
            if args.sa_tail_side != "both":
                fn = fused if args.sa_tail_side == "fused" else stock
                for _ in range(args.reps):
                    fn()
                torch.cuda.synchronize()
                print(json.dumps({"op": "sa_tail/%s_alone" % args.sa_tail_side, "row": name, "shape": shape, "calls": args.reps}), flush=True)
                continue
            y_f, y_s = fused(), stock()          # the fused side first: without a batch norm the stock ReLU works in place on x
            diff = float((y_f - y_s).abs().max())
            (s1, f1), (s2, f2) = timeit_pair(stock, fused), timeit_pair(stock, fused)
            spread = abs(s1 - s2)
            faster = f1 < s1 and f2 < s2 and min(s1 - f1, s2 - f2) > spread
            nbytes = 4 * (x.numel() + y_f.numel() + packed.w.numel())
            print(json.dumps({"op": "sa_tail", "row": name, "shape": shape, "ms_stock": [round(s1, 4), round(s2, 4)],
                              "ms_fused": [round(f1, 4), round(f2, 4)], "stock_spread_ms": round(spread, 4), "fused_is_faster": bool(faster),
                              "x_y_w_bytes": nbytes, "share_of_8TBps": round(nbytes / (min(f1, f2) * 1e-3) / 8e12, 4),
                              "max_abs_diff": diff, "reps": args.reps}), flush=True)
            del x
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--image-head-only", action="store_true",
                    help="only the two-stream backbone's image head: the dense lines against li_fusion.image_head_at_points")
    ap.add_argument("--image-head-side", default="both", choices=["both", "points", "dense"],
                    help="with --image-head-only: run one side alone, --reps calls per size (for a kernel trace)")
    ap.add_argument("--amp", default="off", choices=["off", "bf16", "fp16"],
                    help="with --image-head-only: 16-bit maps -- the dense lines under torch.autocast against the 16-bit points head "
                         "(li_fusion.image_head_at_points on float16 / bfloat16 maps), the float32 points head beside them")
    ap.add_argument("--image-head-scenes", default="1,2,16", help="with --image-head-only: the batch sizes, comma separated")
    ap.add_argument("--sa-tail-only", action="store_true",
                    help="only the end of every SA level's shared MLP: the stock convolution / batch norm / ReLU / pool_max lines against "
                         "pointnet2_utils.sa_tail, per level and scale of configs 3 / 4 and of the RCNN stage")
    ap.add_argument("--sa-tail-side", default="both", choices=["both", "fused", "stock"],
                    help="with --sa-tail-only: run one side alone, --reps calls per row (for a kernel trace)")
    ap.add_argument("--sa-tail-scenes", default="1,2,16", help="with --sa-tail-only: the batch sizes, comma separated")
    ap.add_argument("--gt-aug-only", action="store_true",
                    help="only GT-database augmentation: gt_aug_layer.prepare_scans_gt_aug against scan_layer.prepare_scans on the same scans")
    ap.add_argument("--gt-aug-side", default="both", choices=["both", "fused"],
                    help="with --gt-aug-only: fused = --reps more calls per size and no host restatement (for a kernel trace)")
    ap.add_argument("--gt-aug-scenes", default="1,2,16,256", help="with --gt-aug-only: the batch sizes, comma separated")
    ap.add_argument("--loss-only", action="store_true", help="only the training-loss rows (fused against the two stock-torch forms)")
    ap.add_argument("--targets-only", action="store_true", help="only the RPN training targets (fused against bench_step.rpn_labels)")
    ap.add_argument("--scan-only", action="store_true",
                    help="only the RPN inputs from raw scans (fused scan_layer.prepare_scans against composed_scan_prepare) and the image normalisation")
    ap.add_argument("--rcnn-targets-only", action="store_true",
                    help="only the RCNN training targets (the sync-free RCNNTargetLayer against the existing ProposalTargetLayer)")
    ap.add_argument("--stage2-only", action="store_true", help="only the second-stage inference pairs (roipool3d_canonical, rcnn_detections)")
    ap.add_argument("--handover-only", action="store_true",
                    help="only the RPN hand-over: rpn_handover against the existing ProposalLayer.forward, the whole table twice")
    ap.add_argument("--handover-side", default="both", choices=["both", "fused", "composed"],
                    help="with --handover-only: run one side alone, --reps calls per size (what a kernel trace of launches per call needs)")
    ap.add_argument("--handover-scenes", default="1,2,16,256", help="with --handover-only: the batch sizes, comma separated")
    ap.add_argument("--optim-only", action="store_true",
                    help="only the optimiser step: FusedAdamOneCycle against the stock-torch composition on the two-stream model's parameters")
    ap.add_argument("--optim-side", default="both", choices=["both", "fused", "fused_views", "composed", "scaled", "scaled_fused",
                                                             "scaled_composed"],
                    help="with --optim-only: run one side alone (what a kernel trace of launches per step needs); fused_views: the fused "
                         "side with every gradient a view at an odd offset of one bucket; scaled: the step with dynamic loss scaling "
                         "against its stock composition (unscale + the plain fused step + scale update), scaled_fused / "
                         "scaled_composed: one of those alone")
    ap.add_argument("--rows16-only", action="store_true",
                    help="only the native 16-bit SA / FP kernels against their float32 twins and the upcast composition (bf16)")
    ap.add_argument("--kitti-eval-only", action="store_true",
                    help="only the AP evaluator: get_official_eval_result and its phases on a synthetic set at KITTI-val scale")
    ap.add_argument("--kitti-eval-frames", type=int, default=3769, help="frames of the synthetic set (KITTI val: 3769)")
    ap.add_argument("--kitti-eval-host-frames", type=int, default=200, help="frames given to the numpy restatement on one host core")
    args = ap.parse_args()
    if args.kitti_eval_only:
        return kitti_eval_rows(args)
    import torch
    from epnet_amd import iou3d_cuda, iou3d_utils, kitti_utils, pointnet2_cuda as p2, roipool3d_cuda, synth

    dev = torch.device("cuda:0")
    f32, i32 = torch.float32, torch.int32

    def timeit(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts.sort()
        return ts[len(ts) // 2]

    def timeit_once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def report(op, shape, ms, nbytes, note=""):
        print(json.dumps({"op": op, "shape": shape, "ms": round(ms, 4), "algorithmic_bytes": nbytes,
                          "GBps": round(nbytes / (ms * 1e-3) / 1e9, 2), "note": note}), flush=True)

    def timeit_pair(fa, fb):
        """medians of two alternatives measured ALTERNATELY inside one call (same clocks, same cache state), warm-up first"""
        for _ in range(3):
            fa(); fb()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(args.reps):
            for fn, ts in ((fa, ta), (fb, tb)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record(); torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
        return sorted(ta)[len(ta) // 2], sorted(tb)[len(tb) // 2]

    g = torch.Generator().manual_seed(0)

    def stage2_infer():
        """second-stage inference: each fused op against the composition from the ops the package had before it -- the
        reference's own statements (lib/net/rcnn_net.py:152-162, tools/eval_rcnn.py:663-683) on this package's surface"""
        from epnet_amd import roipool3d_utils
        n, m, s, c = 16384, 100, 512, 130
        for bsz in (1, 2, 16):
            pts = synth.scenes("kitti", bsz, n, seed=5).to(dev)
            feat = torch.randn((bsz, n, c), generator=g).to(dev)
            rois = torch.stack([synth.proposal_boxes(m, seed=50 + i)[0] for i in range(bsz)]).to(dev)

            def composed():
                pooled, flag = roipool3d_utils.roipool3d_gpu(pts, feat, rois, 0.2, sampled_pt_num=s)
                pooled[:, :, :, 0:3] -= rois[:, :, 0:3].unsqueeze(dim=2)
                for k in range(bsz):
                    pooled[k, :, :, 0:3] = kitti_utils.rotate_pc_along_y_torch(pooled[k, :, :, 0:3], rois[k, :, 6])
                return pooled, flag

            def fused():
                return roipool3d_utils.roipool3d_canonical_gpu(pts, feat, rois, 0.2, sampled_pt_num=s)
            (pc, fc), (pf, ff) = composed(), fused()
            close = bool(torch.equal(fc, ff) and torch.equal(pc[..., 3:][fc == 0], pf[..., 3:][ff == 0])
                         and torch.allclose(pc[..., 0:3], pf[..., 0:3], rtol=0, atol=1e-4))
            ms_c, ms_f = timeit_pair(composed, fused)
            report("roipool3d_canonical", {"B": bsz, "N": n, "M": m, "S": s, "C": c}, ms_f,
                   bsz * (n * 12 + n * c * 4 + m * 28 + m * s * (3 + c) * 4 + m * 4),
                   "one launch, no zero-fill; composition (roipool3d_gpu + centre subtraction + per-scene rotation loop): %.4f ms; "
                   "same flags and features, xyz within 1e-4: %s; empty boxes: %d" % (ms_c, close, int(ff.sum())))
        for m in (100, 512):
            for bsz in (1, 2, 16):
                boxes = torch.stack([synth.proposal_boxes(m, seed=70 + i, num_objects=12)[0] for i in range(bsz)]).to(dev)
                raw = (torch.randn((bsz, m), generator=g) * 2).to(dev)
                norm = torch.sigmoid(raw)
                det_b = torch.empty((bsz, m, 7), device=dev)
                det_s = torch.empty((bsz, m), device=dev)
                det_c = torch.empty((bsz,), dtype=i32, device=dev)

                def composed():
                    inds = norm > 0.2
                    out = []
                    for k in range(bsz):
                        cur_inds = inds[k].view(-1)
                        if cur_inds.sum() == 0:
                            continue
                        sel_b, sel_s = boxes[k, cur_inds], raw[k, cur_inds]
                        keep_idx = iou3d_utils.nms_gpu(kitti_utils.boxes3d_to_bev_torch(sel_b), sel_s, 0.1).view(-1)
                        out.append((sel_b[keep_idx].cpu(), sel_s[keep_idx].cpu()))
                    return out

                def fused():
                    iou3d_cuda.rcnn_detections_gpu(boxes, raw, norm, 0.2, 0.1, det_b, det_s, det_c)

                def fused_read_back():
                    fused()
                    return det_b.cpu(), det_s.cpu(), det_c.cpu()
                want = composed()
                got_b, got_s, got_c = fused_read_back()
                same = got_c.tolist() == [w[1].numel() for w in want] and all(
                    torch.equal(got_b[k, :w[1].numel()], w[0]) and torch.equal(got_s[k, :w[1].numel()], w[1]) for k, w in enumerate(want))
                ms_c, ms_f = timeit_pair(composed, fused)
                ms_r = timeit(fused_read_back)
                report("rcnn_detections", {"B": bsz, "M": m, "score_thresh": 0.2, "nms_thresh": 0.1, "kept": got_c.tolist()}, ms_f,
                       bsz * (m * 28 + m * 8 + m * 32 + 4),
                       "select + batched rotated NMS + emit, no host sync; with one read-back of the three results: %.4f ms; composition "
                       "(per-scene loop over nms_gpu with its read-backs): %.4f ms; same result: %s" % (ms_r, ms_c, same))

    if args.stage2_only:
        return stage2_infer()
    if args.image_head_only:
        return image_head_rows(args, timeit_pair)
    if args.sa_tail_only:
        return sa_tail_rows(args, timeit_pair)
    if args.loss_only:
        return loss_rows(args, report, timeit_pair)
    if args.optim_only:
        return (optim_scaled_rows if args.optim_side.startswith("scaled") else optim_rows)(args, report)
    if args.targets_only:
        return targets_rows(args, report, timeit_pair)
    if args.rcnn_targets_only:
        return rcnn_targets_rows(args, report, timeit_pair)
    if args.scan_only:
        return scan_rows(args, report, timeit_pair)
    if args.gt_aug_only:
        return gt_aug_rows(args, report, timeit_pair)
    if args.handover_only:
        return handover_rows(args, report, timeit_pair)
    if args.rows16_only:
        return rows16_rows(args, timeit_pair)
    # ---- NMS at the proposal-layer sizes (RPN.NMS_TYPE normal, N <= 6300 / 2700, thresh 0.85) and eval rotated NMS
    for n, rot, thr in ((6300, False, 0.85), (2700, False, 0.85), (6300, True, 0.8), (512, True, 0.1), (100, True, 0.1)):
        boxes, scores = synth.proposal_boxes(n, seed=n, num_objects=40, jitter=1.5)
        bev, sc = kitti_utils.boxes3d_to_bev_torch(boxes).to(dev), scores.to(dev)
        fn = iou3d_utils.nms_gpu if rot else iou3d_utils.nms_normal_gpu
        kept = fn(bev, sc, thr)
        ms = timeit(lambda: fn(bev, sc, thr))
        srt = bev[sc.sort(0, descending=True)[1]].contiguous()
        dfn = iou3d_cuda.nms_device if rot else iou3d_cuda.nms_normal_device
        ms_dev = timeit(lambda: dfn(srt, thr))
        report("nms_gpu" if rot else "nms_normal_gpu", {"N": n, "thresh": thr, "kept": int(kept.numel())}, ms,
               n * 20 + n * ((n + 63) // 64) * 8, "surface call incl. sort + 4-byte count sync; mask+sweep kernels alone %.4f ms" % ms_dev)
    # ---- 3-D IoU of 512 ROIs x 20 GT boxes, and the 1x1 calls of aug_roi_by_noise
    a, _ = synth.proposal_boxes(512, seed=1)
    b, _ = synth.proposal_boxes(20, seed=2)
    a, b = a.to(dev), b.to(dev)
    report("boxes_iou3d_gpu", {"Na": 512, "Nb": 20}, timeit(lambda: iou3d_utils.boxes_iou3d_gpu(a, b)), 512 * 20 + 20 * 20 + 512 * 20 * 4, "incl. torch height/volume math")
    a1, b1 = a[:1].contiguous(), b[:1].contiguous()
    report("boxes_iou3d_gpu", {"Na": 1, "Nb": 1}, timeit(lambda: iou3d_utils.boxes_iou3d_gpu(a1, b1)), 44, "launch-latency bound")
    # ---- ROI augmentation: 2 scenes x 64 ROIs x up to 10 tries -- one launch against the reference's
    # host loop (proposal_target_layer.py:220-247: per try a single-pair IoU composed of ~15 launches and a device->host
    # read of the result), restated here on this package's own surface for timing
    from epnet_amd import proposal_target_layer as ptl
    k_rois, t_max = 128, 10
    boxes, _ = synth.proposal_boxes(2 * k_rois, seed=3, num_objects=16, jitter=0.6)
    rois0, gts0 = boxes[:k_rois].to(dev).contiguous(), boxes[k_rois:].to(dev).contiguous()
    src0 = torch.rand((k_rois,), generator=g).to(dev)
    tries = torch.tensor([t_max] * 32 + [1] * 32, dtype=i32).repeat(2).to(dev)

    def batched():
        keep, noise = ptl.draw_aug_tables(k_rois, t_max, "multiple", dev)
        return ptl.aug_roi_by_noise_batched(rois0.clone(), gts0, src0, 0.55, keep, noise, tries)

    def host_loop():
        keep, noise = ptl.draw_aug_tables(k_rois, t_max, "multiple", dev)
        keep_h = keep.cpu().numpy()
        out = rois0.clone()
        n_try = tries.cpu().numpy()
        launches = 0
        for k in range(k_rois):
            temp_iou, cnt, aug = 0.0, 0, out[k]
            while temp_iou < 0.55 and cnt < n_try[k]:
                nz = noise[k, cnt]
                aug = out[k] if keep_h[k, cnt] else torch.cat([out[k, 0:3] + nz[0:3], out[k, 3:6] * nz[3:6], out[k, 6:7] + nz[6:7]])
                temp_iou = float(iou3d_utils.boxes_iou3d_composed(aug.view(1, 7), gts0[k:k + 1])[0, 0])
                cnt += 1
                launches += 1
            out[k] = aug
        return launches
    ms_b = timeit(batched)
    n_pairs = host_loop()
    ms_h = timeit(host_loop) if args.reps <= 5 else sorted(timeit_once(host_loop) for _ in range(3))[1]
    report("aug_roi_by_noise", {"rois": k_rois, "aug_times": t_max, "fg": 64, "bg": 64}, ms_b, k_rois * (28 * 2 + 4 + 4 + t_max * 29 + 28 + 4),
           "tables drawn on the device + one launch; the reference's host loop over the same ROIs (%d single-pair IoU calls with a "
           "device->host read each): %.1f ms" % (n_pairs, ms_h))
    # ---- the whole target layer at BASELINE config 4's per-rank shapes (2 scenes x 512 proposals -> 64 ROIs, 16384 x 128 features)
    bsz, m, n = 2, 512, 16384
    rl, gl = [], []
    for i in range(bsz):
        bx, _ = synth.proposal_boxes(m + 12, seed=200 + i, num_objects=12, jitter=0.4)
        gt = torch.zeros((20, 7)); gt[:12] = bx[m:]
        rl.append(bx[:m]); gl.append(gt)
    layer_in = {"roi_boxes3d": torch.stack(rl).to(dev), "gt_boxes3d": torch.stack(gl).to(dev),
                "rpn_xyz": synth.scenes("kitti", bsz, n, seed=9).to(dev), "rpn_features": torch.randn((bsz, n, 128), generator=g).to(dev),
                "seg_mask": (torch.rand((bsz, n), generator=g) > 0.5).float().to(dev), "pts_depth": (torch.rand((bsz, n), generator=g) * 70).to(dev)}
    layer = ptl.ProposalTargetLayer()
    ms = timeit(lambda: layer(layer_in))
    report("ProposalTargetLayer.forward", {"B": bsz, "proposals": m, "rois": 64, "N": n, "C": 128}, ms,
           bsz * (n * 12 + n * 130 * 4 + 64 * 28 + 64 * 512 * 133 * 4 + 64 * 4),
           "IoU + sampling (2 host syncs) + batched augmentation + roipool3d + canonical transform + labels; bytes = the roipool3d figure")
    # ---- proposal layer at the training shapes: 2 scenes x 16384 points, pre 9000 / post 512, thresh 0.85
    from epnet_amd import proposal_layer as pl
    bsz, n = 2, 16384
    xyz_p = synth.scenes("kitti", bsz, n, seed=21).to(dev)
    reg_p = (torch.randn((bsz, n, 76), generator=g) * 0.5).to(dev)
    sc_p = torch.randn((bsz, n), generator=g).to(dev)
    for mode in ("TRAIN", "TEST"):
        layer_p = pl.ProposalLayer(mode).to(dev)
        mcfg = getattr(layer_p.cfg, mode)
        props = layer_p.decode(reg_p, xyz_p).contiguous()
        cnt = torch.zeros((bsz,), dtype=i32, device=dev)
        layer_p.propose(sc_p, props, cnt)

        def host_loop():   # the reference's per-scene structure (proposal_layer.py:40-54, 58-119) on this package's NMS surface
            order = torch.sort(sc_p, dim=1, descending=True)[1]
            ret = torch.zeros((bsz, mcfg.RPN_POST_NMS_TOP_N, 7), device=dev)
            pre = [0, int(mcfg.RPN_PRE_NMS_TOP_N * 0.7), mcfg.RPN_PRE_NMS_TOP_N - int(mcfg.RPN_PRE_NMS_TOP_N * 0.7)]
            post = [0, int(mcfg.RPN_POST_NMS_TOP_N * 0.7), mcfg.RPN_POST_NMS_TOP_N - int(mcfg.RPN_POST_NMS_TOP_N * 0.7)]
            for k in range(bsz):
                s_ord, p_ord = sc_p[k][order[k]], props[k][order[k]]
                dist, rng, outs = p_ord[:, 2], [0, 40.0, 80.0], []
                for i in (1, 2):
                    m = (dist > rng[i - 1]) & (dist <= rng[i])
                    cur_s, cur_p = s_ord[m][:pre[i]], p_ord[m][:pre[i]]
                    keep = iou3d_utils.nms_normal_gpu(kitti_utils.boxes3d_to_bev_torch(cur_p), cur_s, mcfg.RPN_NMS_THRESH)[:post[i]]
                    outs.append(cur_p[keep])
                allp = torch.cat(outs, 0)
                ret[k, :allp.size(0)] = allp
            return ret
        same = torch.equal(host_loop(), layer_p.propose(sc_p, props)[0])
        ms_dec = timeit(lambda: layer_p.decode(reg_p, xyz_p))
        ms_prop = timeit(lambda: layer_p.propose(sc_p, props))
        ms_host = timeit(host_loop)
        report("ProposalLayer.propose", {"B": bsz, "N": n, "mode": mode, "pre": mcfg.RPN_PRE_NMS_TOP_N, "post": mcfg.RPN_POST_NMS_TOP_N,
                                         "thresh": mcfg.RPN_NMS_THRESH, "kept": cnt.tolist()}, ms_prop,
               bsz * (n * 28 + n * 4 + n * 8 + mcfg.RPN_POST_NMS_TOP_N * 32),
               "sort + bin compaction + batched NMS + gather, no host sync; per-scene host loop on the same NMS kernels: %.3f ms "
               "(same result: %s); box decoding (stock tensor ops): %.3f ms" % (ms_host, same, ms_dec))
    # ---- LI-Fusion point-to-pixel sampler: the image pyramid of the yaml (LI_FUSION.IMG_CHANNELS) at 2 scenes
    import torch.nn.functional as F
    from epnet_amd.li_fusion import Feature_Gather
    for (c, h, w, n) in ((64, 192, 640, 4096), (128, 96, 320, 1024), (256, 48, 160, 256), (512, 24, 80, 64), (32, 384, 1280, 16384)):
        fmap = torch.randn((2, c, h, w), generator=g).to(dev)
        xy = (torch.rand((2, n, 2), generator=g) * 2 - 1).to(dev)
        ms_stock = timeit(lambda: F.grid_sample(fmap, xy.unsqueeze(1), mode="bilinear", padding_mode="zeros", align_corners=True))
        ms = timeit(lambda: Feature_Gather(fmap, xy))
        report("Feature_Gather", {"B": 2, "C": c, "H": h, "W": w, "N": n}, ms, 2 * (n * 8 + c * n * 4 * 4 + c * n * 4),
               "bytes = 4 taps read + 1 value written per (point, channel); stock grid_sample: %.4f ms" % ms_stock)
    # ---- roipool3d: (B,16384,3)+(B,16384,130) -> (B,64,512,133)
    for bsz, m in ((2, 64), (1, 100), (16, 64)):
        pts = synth.scenes("kitti", bsz, 16384, seed=5).to(dev)
        feat = torch.randn((bsz, 16384, 130), generator=g).to(dev)
        boxes = torch.stack([synth.proposal_boxes(m, seed=50 + i)[0] for i in range(bsz)]).to(dev)
        pooled = torch.zeros((bsz, m, 512, 133), dtype=f32, device=dev)
        flag = torch.zeros((bsz, m), dtype=i32, device=dev)
        big = kitti_utils.enlarge_box3d(boxes.view(-1, 7), 0.2).view(bsz, m, 7).contiguous()
        ms = timeit(lambda: roipool3d_cuda.forward(pts, big, feat, pooled, flag))
        n = 16384
        report("roipool3d forward", {"B": bsz, "N": n, "M": m, "S": 512, "C": 130}, ms,
               bsz * (n * 12 + n * 130 * 4 + m * 28 + m * 512 * 133 * 4 + m * 4), "empty boxes: %d" % int(flag.sum()))
    # ---- FP ops
    for bsz, (c, m, n) in ((16, (256, 4096, 16384)), (16, (512, 1024, 4096)), (1, (256, 4096, 16384))):
        unknown = synth.scenes("kitti", bsz, n, seed=7).to(dev)
        # as in an FP module: the known set is the FPS subset of the unknown one
        kidx = torch.empty((bsz, m), dtype=i32, device=dev)
        known = torch.empty((bsz, m, 3), device=dev)
        p2.sample_centres_wrapper(bsz, n, m, unknown, p2.scene_index(unknown), kidx, known)
        d2 = torch.empty((bsz, n, 3), device=dev); idx = torch.empty((bsz, n, 3), dtype=i32, device=dev)
        ms = timeit(lambda: p2.three_nn_wrapper(bsz, n, m, unknown, known, d2, idx))
        report("three_nn", {"B": bsz, "n": n, "m": m}, ms, bsz * (n * 12 + m * 12 + n * 24), "builds its own index of the known set")
        ui, ki = p2.scene_index(unknown), p2.scene_index(known)
        if ki is not None:
            ms = timeit(lambda: p2.three_nn_indexed_wrapper(bsz, n, m, unknown, known, ui, ki, d2, idx))
            report("three_nn", {"B": bsz, "n": n, "m": m}, ms, bsz * (n * 12 + m * 12 + n * 24), "over the scene indices of both point sets")
        feats = torch.randn((bsz, c, m), generator=g).to(dev)
        w = torch.rand((bsz, n, 3), generator=g).to(dev); w = (w / w.sum(-1, keepdim=True)).contiguous()
        out = torch.empty((bsz, c, n), device=dev)
        ms = timeit(lambda: p2.three_interpolate_wrapper(bsz, c, m, n, feats, idx, w, out))
        report("three_interpolate", {"B": bsz, "C": c, "m": m, "n": n}, ms, bsz * (c * m * 4 + n * 24 + c * n * 4))
        go = torch.randn((bsz, c, n), generator=g).to(dev); gp = torch.zeros((bsz, c, m), device=dev)
        ms = timeit(lambda: p2.three_interpolate_grad_wrapper(bsz, c, n, m, go, idx, w, gp))
        report("three_interpolate_grad", {"B": bsz, "C": c, "n": n, "m": m}, ms, bsz * (c * n * 4 + n * 24 + c * m * 4))
    # ---- grouping gradient (level 2: C=96, N=4096, M=1024, ns=32) on real ball-query neighbour lists
    for bsz in (16,):
        pts = synth.scenes("kitti", bsz, 4096, seed=11).to(dev)
        cidx = torch.empty((bsz, 1024), dtype=i32, device=dev)
        ctr = torch.empty((bsz, 1024, 3), device=dev)
        p2.sample_centres_wrapper(bsz, 4096, 1024, pts, p2.scene_index(pts), cidx, ctr)
        idx = torch.empty((bsz, 1024, 32), dtype=i32, device=dev)
        p2.ball_query_wrapper(bsz, 4096, 1024, 1.0, 32, ctr, pts, idx)
        go = torch.randn((bsz, 96, 1024, 32), generator=g).to(dev)
        gp = torch.zeros((bsz, 96, 4096), device=dev)
        ms = timeit(lambda: p2.group_points_grad_wrapper(bsz, 96, 4096, 1024, 32, go, idx, gp))
        report("group_points_grad", {"B": bsz, "C": 96, "N": 4096, "M": 1024, "ns": 32}, ms, bsz * (96 * 1024 * 32 * 4 + 1024 * 32 * 4 + 96 * 4096 * 4),
               "neighbour lists of ball_query(r=1.0) around FPS centres")
    # ---- BASELINE config 5: dense 65536-point scenes, one SA level with nsample = 64 (ball-query stress)
    for bsz in (1, 16):
        n, m, ns, c, radius = 65536, 16384, 64, 64, 0.5
        xyz = synth.scenes("kitti", bsz, n, seed=9).to(dev)
        index = torch.empty((p2.scene_index_bytes(bsz, n),), dtype=torch.uint8, device=dev)
        ms = timeit(lambda: p2.scene_index_build_wrapper(bsz, n, xyz, index))
        report("scene_index_build", {"B": bsz, "N": n}, ms, bsz * (n * 12 + n * 16), "this implementation's own structure")
        temp = torch.empty((bsz, n), device=dev); fidx = torch.empty((bsz, m), dtype=i32, device=dev)

        def fps():
            temp.fill_(1e10)
            p2.furthest_point_sampling_indexed_wrapper(bsz, n, m, xyz, index, temp, fidx)
        ms = timeit(fps) if bsz == 1 else timeit(fps)
        report("furthest_point_sampling", {"B": bsz, "N": n, "M": m}, ms, bsz * (n * 12 + m * 4), "big-scene kernel over the index")
        new_xyz = torch.gather(xyz, 1, fidx.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
        bq = torch.empty((bsz, m, ns), dtype=i32, device=dev)
        ms = timeit(lambda: p2.ball_query_indexed_wrapper(bsz, n, m, radius, ns, new_xyz, xyz, index, bq))
        report("ball_query", {"B": bsz, "N": n, "M": m, "r": radius, "ns": ns}, ms, bsz * (n * 12 + m * 12 + m * ns * 4))
        feats = torch.randn((bsz, c, n), generator=g).to(dev)
        grouped = torch.empty((bsz, 3 + c, m, ns), device=dev)
        ms = timeit(lambda: p2.group_concat_wrapper(bsz, c, n, m, ns, xyz, new_xyz, feats, bq, grouped, True))
        report("group_concat", {"B": bsz, "C": c, "N": n, "M": m, "ns": ns}, ms,
               bsz * (2 * m * ns * 4 + 3 * n * 4 + c * n * 4 + (3 + c) * m * ns * 4))
        gx = torch.empty((bsz, 3, m, ns), device=dev)
        ms = timeit(lambda: p2.group_concat_wrapper(bsz, 0, n, m, ns, xyz, new_xyz, None, bq, gx, True))
        report("group_concat", {"B": bsz, "C": 0, "N": n, "M": m, "ns": ns}, ms, bsz * (m * ns * 4 + 3 * n * 4 + 3 * m * ns * 4))
    stage2_infer()
    loss_rows(args, report, timeit_pair)


if __name__ == "__main__":
    main()

"""The RPN / RCNN training losses in this project's own words (numpy, float64 or float32): forward AND analytic gradients.

What is restated is lib/utils/loss_utils.py:79-87 (the logit cross-entropy of the focal loss), :90-350 (get_reg_loss) and the two
closures of lib/net/train_functions.py:92-284 (get_rpn_loss / get_rcnn_loss), as ONE function of rows:

    cls_logit (R)   pred_reg (R, C)   reg_label (R, 7) [dx, dy, dz, h, w, l, ry]   cls_label (R) in {-1, 0, > 0}
    reg_mask (R) or None (= cls_label > 0)   iou_branch (R) or None

with C = 4 nb + 1 + 2 nh + 3 laid out [x_bin nb | z_bin nb | x_res nb | z_res nb | y_offset | ry_bin nh | ry_res nh | size 3].
Every regression term is a SUM over the foreground rows divided by max(count, 1): no foreground row gives exactly 0 with zero
gradients and there is no branch on the count. `box_loss` returns the named terms, the gradients of terms['total'] with respect
to cls_logit, pred_reg and iou_branch, and per-row side information (labels, which clamps are active, distances from the kinks)
for the coverage tests and the fixture generator. The analytic gradients are checked against the reference's autograd in
tests/test_loss.py; nothing here is differentiated numerically.
"""
import numpy as np

TERM_NAMES = ["total", "loss", "loss_cls", "loss_cls_pos", "loss_cls_neg", "loss_reg", "loss_loc", "loss_angle", "loss_size", "loss_iou",
              "loss_x_bin", "loss_z_bin", "loss_x_res", "loss_z_res", "loss_y_offset", "loss_ry_bin", "loss_ry_res", "iou_branch_loss",
              "fg_sum", "cls_pos", "cls_neg", "cls_valid", "loss_size_unweighted", "loss_iou_unweighted"]

IOU_TYPES = ("raw", "cls_mask_with_bin")
CLS_TYPES = ("SigmoidFocalLoss", "BinaryCrossEntropy", "none")


def settings(stage, **over):
    """the values of tools/cfgs/LI_Fusion_with_attention_use_ce_loss.yaml for one stage"""
    s = dict(anchor=(1.52563191462, 1.62856739989, 3.88311640418), iou_type="cls_mask_with_bin", ce_weight=5.0, alpha=0.25, gamma=2.0,
             use_iou_branch=False, w_train=1.0, fg_weight=1.0, w_cls=1.0, w_reg=1.0)
    if stage == "rpn":
        s.update(loc_scope=3.0, loc_bin_size=0.5, num_head_bin=12, ry_fine=False, cls_type="SigmoidFocalLoss", fg_weight=15.0)
    else:
        s.update(loc_scope=1.5, loc_bin_size=0.5, num_head_bin=9, ry_fine=True, cls_type="BinaryCrossEntropy")
    s.update(over)
    return s


def channels(s):
    nb = int(s["loc_scope"] / s["loc_bin_size"]) * 2
    return 4 * nb + 1 + 2 * s["num_head_bin"] + 3


def _smooth_l1(d):
    a = np.abs(d)
    return np.where(a < 1, 0.5 * d * d, a - 0.5), np.where(a < 1, d, np.sign(d))


def _softmax_ce(logits, label):
    """-> per-row cross-entropy, softmax, d ce / d logits"""
    m = logits.max(axis=1, keepdims=True)
    e = np.exp(logits - m)
    se = e.sum(axis=1, keepdims=True)
    q = e / se
    rows = np.arange(logits.shape[0])
    ce = np.log(se[:, 0]) - (logits[rows, label] - m[:, 0])   # log_softmax's order: exact where the labelled logit is the largest
    g = q.copy()
    g[rows, label] -= 1
    return ce, q, g


def _relgap(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)


def heading_labels(ry, nh, fine, ft):
    """-> bin label, normalised residual label, and (fine only) whether the row took the 'opposite' flip"""
    two_pi = 2 * np.pi
    if fine:
        apc = (np.pi / 2) / nh
        ry = np.remainder(ry, two_pi).astype(ft)
        opposite = (ry > np.pi * 0.5) & (ry < np.pi * 1.5)
        ry = np.where(opposite, np.remainder(ry + np.pi, two_pi), ry).astype(ft)
        shift = np.remainder(ry + np.pi * 0.5, two_pi).astype(ft)
        shift = np.clip(shift - np.pi * 0.25, ft(1e-3), ft(np.pi * 0.5 - 1e-3)).astype(ft)
    else:
        apc = two_pi / nh
        opposite = np.zeros(ry.shape, bool)
        heading = np.remainder(ry, two_pi).astype(ft)
        shift = np.remainder(heading + apc / 2, two_pi).astype(ft)
    b = np.floor(shift / ft(apc)).astype(np.int64)
    res = shift - (b.astype(ft) * ft(apc) + ft(apc / 2))
    return b, (res / ft(apc / 2)).astype(ft), opposite


def box_loss(s, cls_logit, pred_reg, reg_label, cls_label, reg_mask=None, iou_branch=None, dtype=np.float64, fg_only=False):
    """fg_only (very large batches): pred_reg and reg_label hold the foreground rows only, in row order, and grad_reg comes back
    for those rows only (the background rows' gradient is zero)"""
    ft = np.dtype(dtype).type
    if s["iou_type"] not in IOU_TYPES or s["cls_type"] not in CLS_TYPES:
        raise ValueError("unknown loss type")
    scope, bs, nh = s["loc_scope"], s["loc_bin_size"], s["num_head_bin"]
    nb = int(scope / bs) * 2
    c = pred_reg.shape[1]
    assert c == 4 * nb + 1 + 2 * nh + 3, (c, nb, nh)
    x = np.asarray(cls_logit).reshape(-1).astype(ft)
    rows_n = x.shape[0]
    lab = np.asarray(cls_label).reshape(-1).astype(np.int64)
    mask = (lab > 0) if reg_mask is None else (np.asarray(reg_mask).reshape(-1) > 0)
    fg = np.nonzero(mask)[0]
    n_fg, n_pos, n_neg, n_valid = len(fg), int((lab > 0).sum()), int((lab == 0).sum()), int((lab >= 0).sum())
    w_train = ft(s["w_train"])
    w_cls, w_reg = ft(s["w_cls"]) * w_train, ft(s["w_reg"]) * w_train
    terms = {k: ft(0) for k in TERM_NAMES}
    terms.update(fg_sum=ft(n_fg), cls_pos=ft(n_pos), cls_neg=ft(n_neg), cls_valid=ft(n_valid))
    grad_cls = np.zeros(rows_n, ft)
    grad_reg = np.zeros((len(fg) if fg_only else rows_n, c), ft)
    grad_iou_branch = np.zeros(rows_n, ft)
    aux = {}

    # ---- classification, every row --------------------------------------------------------------------------------------
    p = 1 / (1 + np.exp(-x))
    t = (lab > 0).astype(ft)
    if s["cls_type"] == "SigmoidFocalLoss":
        w = ((lab >= 0).astype(ft)) / ft(max(n_pos, 1))
        ce = np.maximum(x, 0) - x * t + np.log1p(np.exp(-np.abs(x)))
        u = t * (1 - p) + (1 - t) * p                      # 1 - p_t
        gamma = ft(s["gamma"])
        mod = u * u if s["gamma"] == 2.0 else (np.power(u, gamma) if s["gamma"] else np.ones_like(u))
        dmod = 2 * u if s["gamma"] == 2.0 else (gamma * np.power(u, gamma - 1) if s["gamma"] else np.zeros_like(u))
        aw = t * ft(s["alpha"]) + (1 - t) * ft(1 - s["alpha"])
        per = mod * aw * ce * w
        terms["loss_cls"] = per.sum(dtype=ft)
        terms["loss_cls_pos"] = (per * (lab > 0)).sum(dtype=ft)
        terms["loss_cls_neg"] = (per * (lab == 0)).sum(dtype=ft)
        grad_cls += w_cls * aw * w * (dmod * (1 - 2 * t) * p * (1 - p) * ce + mod * (p - t))
    elif s["cls_type"] == "BinaryCrossEntropy":
        valid = (lab >= 0).astype(ft)
        w = np.where(lab > 0, ft(s["fg_weight"]), ft(1))
        with np.errstate(divide="ignore"):                  # F.binary_cross_entropy clamps its logs at -100
            per = -w * (t * np.maximum(np.log(p), -100) + (1 - t) * np.maximum(np.log(1 - p), -100))
        norm = ft(max(n_valid, 1))
        terms["loss_cls"] = (per * valid).sum(dtype=ft) / norm
        grad_cls += w_cls * valid / norm * w * (p - t) / np.maximum((1 - p) * p, ft(1e-12)) * (p * (1 - p))

    # ---- regression, the foreground rows -----------------------------------------------------------------------------------
    r = np.arange(n_fg)
    pr = (np.asarray(pred_reg) if fg_only else np.asarray(pred_reg)[fg]).astype(ft)
    lb = (np.asarray(reg_label).reshape(-1, 7) if fg_only else np.asarray(reg_label).reshape(rows_n, 7)[fg]).astype(ft)
    assert pr.shape[0] == n_fg and lb.shape[0] == n_fg
    anchor = np.asarray(s["anchor"], np.float32).astype(ft)   # MEAN_SIZE is a float32 tensor whatever the predictions are
    denom = ft(max(n_fg, 1))
    g = np.zeros((n_fg, c), ft)
    o_xb, o_zb, o_xr, o_zr, o_y = 0, nb, 2 * nb, 3 * nb, 4 * nb
    o_rb, o_rr, o_sz = 4 * nb + 1, 4 * nb + 1 + nh, 4 * nb + 1 + 2 * nh

    def loc_labels(off):
        shift = np.clip(off + ft(scope), ft(0), ft(scope * 2 - 1e-3)).astype(ft)
        b = np.floor(shift / ft(bs)).astype(np.int64)
        res = shift - (b.astype(ft) * ft(bs) + ft(bs / 2))
        return b, res.astype(ft), (res / ft(bs)).astype(ft)
    xb, x_res, x_resn = loc_labels(lb[:, 0])
    zb, z_res, z_resn = loc_labels(lb[:, 2])
    rb, r_resn, opposite = heading_labels(lb[:, 6], nh, s["ry_fine"], ft)
    aux.update(x_bin=xb, z_bin=zb, ry_bin=rb, opposite=opposite, fg_rows=fg)

    ce_x, q_x, g_x = _softmax_ce(pr[:, o_xb:o_xb + nb], xb)
    ce_z, q_z, g_z = _softmax_ce(pr[:, o_zb:o_zb + nb], zb)
    ce_r, _, g_r = _softmax_ce(pr[:, o_rb:o_rb + nh], rb)
    g[:, o_xb:o_xb + nb] += g_x
    g[:, o_zb:o_zb + nb] += g_z
    g[:, o_rb:o_rb + nh] += g_r
    sl_args = []

    def residual(col, target):
        d = pr[r, col] - target
        sl_args.append(d)
        v, dv = _smooth_l1(d)
        g[r, col] += dv
        return v
    l_xr = residual(o_xr + xb, x_resn)
    l_zr = residual(o_zr + zb, z_resn)
    l_y = residual(np.full(n_fg, o_y), lb[:, 1])
    l_rr = residual(o_rr + rb, r_resn)
    size_label = (lb[:, 3:6] - anchor) / anchor
    l_size = ft(0)
    for j in range(3):
        v = residual(np.full(n_fg, o_sz + j), size_label[:, j])
        l_size = l_size + v.sum(dtype=ft)                  # (a mean over 3 * fg elements times the caller's 3: d / d element = 1 / fg)

    def mean(v):
        return v.sum(dtype=ft) / denom
    terms.update(loss_x_bin=mean(ce_x), loss_z_bin=mean(ce_z), loss_x_res=mean(l_xr), loss_z_res=mean(l_zr), loss_y_offset=mean(l_y),
                 loss_ry_bin=mean(ce_r), loss_ry_res=mean(l_rr))
    terms["loss_size_unweighted"] = l_size / (ft(3) * denom)
    terms["loss_size"] = ft(3) * terms["loss_size_unweighted"]
    terms["loss_loc"] = terms["loss_x_bin"] + terms["loss_z_bin"] + terms["loss_x_res"] + terms["loss_z_res"] + terms["loss_y_offset"]
    terms["loss_angle"] = terms["loss_ry_bin"] + terms["loss_ry_res"]

    # ---- the consistency-enforcing (IoU) term: axis-aligned boxes in the bin frame ---------------------------------------
    size = pr[:, o_sz:o_sz + 3] * anchor + anchor          # h, w, l  (y, z, x extents)
    if s["iou_type"] == "raw":
        px, pz = pr[r, o_xr + xb] * ft(bs), pr[r, o_zr + zb] * ft(bs)
        tx, tz = x_res, z_res
    else:
        centre = (np.arange(nb).astype(ft) * ft(bs) + ft(bs / 2) - ft(scope)).astype(ft)
        ax, az = centre + pr[:, o_xr:o_xr + nb] * ft(bs), centre + pr[:, o_zr:o_zr + nb] * ft(bs)
        px, pz = (ax * q_x).sum(axis=1, dtype=ft), (az * q_z).sum(axis=1, dtype=ft)
        tx, tz = centre[xb] + x_res, centre[zb] + z_res
    py, ty = pr[:, o_y], lb[:, 1]
    rel = []

    def axis(pc, pe, tc, te):
        """-> clamped intersection, d / d centre, d / d extent, clamp active"""
        p_hi, t_hi, p_lo, t_lo = pc + pe / 2, tc + te / 2, pc - pe / 2, tc - te / 2
        raw = np.minimum(p_hi, t_hi) - np.maximum(p_lo, t_lo)
        rel.extend([_relgap(p_hi, t_hi), _relgap(p_lo, t_lo), _relgap(raw, 1e-3)])
        live = raw > ft(1e-3)
        hi_p, lo_p = (p_hi < t_hi).astype(ft), (p_lo > t_lo).astype(ft)
        return np.where(live, raw, ft(1e-3)).astype(ft), live * (hi_p - lo_p), live * (hi_p + lo_p) * ft(0.5), ~live
    ix, dix_c, dix_e, cl_x = axis(px, size[:, 2], tx, lb[:, 5])
    iy, diy_c, diy_e, cl_y = axis(py, size[:, 0], ty, lb[:, 3])
    iz, diz_c, diz_e, cl_z = axis(pz, size[:, 1], tz, lb[:, 4])
    inter = ix * iy * iz
    vol_raw = size[:, 0] * size[:, 1] * size[:, 2]
    vol_live = vol_raw > ft(1e-3)
    rel.append(_relgap(vol_raw, 1e-3))
    vol = np.where(vol_live, vol_raw, ft(1e-3)).astype(ft)
    t_vol = lb[:, 3] * lb[:, 4] * lb[:, 5]
    union = vol + t_vol - inter
    iou = inter / union
    score = p[fg]
    v = score * iou
    rel.append(_relgap(v, 1e-4))
    v_live = v > ft(1e-4)
    l_iou = -np.log(np.where(v_live, v, ft(1e-4)))
    ce_w = ft(s["ce_weight"])
    terms["loss_iou_unweighted"] = mean(l_iou)
    terms["loss_iou"] = ce_w * terms["loss_iou_unweighted"]
    g_inter = np.where(v_live, -(union + inter) / (inter * union), ft(0)) * ce_w
    g_vol = np.where(v_live, 1 / union, ft(0)) * ce_w
    g_cls_iou = np.where(v_live, -(1 - score), ft(0)) * ce_w
    g_ix, g_iy, g_iz = g_inter * iy * iz, g_inter * ix * iz, g_inter * ix * iy
    g_h = g_iy * diy_e + g_vol * vol_live * size[:, 1] * size[:, 2]
    g_w = g_iz * diz_e + g_vol * vol_live * size[:, 0] * size[:, 2]
    g_l = g_ix * dix_e + g_vol * vol_live * size[:, 0] * size[:, 1]
    g[:, o_sz + 0] += g_h * anchor[0]
    g[:, o_sz + 1] += g_w * anchor[1]
    g[:, o_sz + 2] += g_l * anchor[2]
    g[:, o_y] += g_iy * diy_c
    g_px, g_pz = g_ix * dix_c, g_iz * diz_c
    if s["iou_type"] == "raw":
        g[r, o_xr + xb] += g_px * ft(bs)
        g[r, o_zr + zb] += g_pz * ft(bs)
    else:
        g[:, o_xr:o_xr + nb] += (g_px * ft(bs))[:, None] * q_x
        g[:, o_zr:o_zr + nb] += (g_pz * ft(bs))[:, None] * q_z
        g[:, o_xb:o_xb + nb] += g_px[:, None] * q_x * (ax - px[:, None])
        g[:, o_zb:o_zb + nb] += g_pz[:, None] * q_z * (az - pz[:, None])
    aux.update(clamp_x=cl_x, clamp_y=cl_y, clamp_z=cl_z, clamp_volume=~vol_live, clamp_iou=~v_live, iou=iou)

    if s["use_iou_branch"]:
        q = np.asarray(iou_branch).reshape(-1)[fg].astype(ft)
        rel.extend([_relgap(q, 1e-4), _relgap(q, 0.9999)])
        inside = (q > ft(1e-4)) & (q < ft(0.9999))
        qc = np.clip(q, ft(1e-4), ft(0.9999)).astype(ft)
        tgt = np.clip(iou, ft(1e-4), ft(0.9999)).astype(ft)
        l_br = -(tgt * np.log(qc) + (1 - tgt) * np.log(1 - qc))
        terms["iou_branch_loss"] = mean(l_br)
        grad_iou_branch[fg] = w_reg / denom * np.where(inside, -(tgt / qc - (1 - tgt) / (1 - qc)), ft(0))

    terms["loss_reg"] = terms["loss_loc"] + terms["loss_angle"] + terms["loss_size"] + terms["loss_iou"] + terms["iou_branch_loss"]
    terms["loss"] = terms["loss_cls"] * ft(s["w_cls"]) + terms["loss_reg"] * ft(s["w_reg"])
    terms["total"] = terms["loss"] * w_train
    grad_reg[slice(None) if fg_only else fg] = g * (w_reg / denom)
    grad_cls[fg] += g_cls_iou * (w_reg / denom)
    sl = np.abs(np.abs(np.stack(sl_args, axis=1).astype(np.float64)) - 1).min(axis=1) if n_fg else np.zeros(0)
    aux.update(margin_smooth_l1=sl, margin_relative=np.stack(rel, axis=1).min(axis=1) if n_fg else np.zeros(0))
    terms = {k: ft(v) for k, v in terms.items()}
    return {"terms": terms, "grad_cls": grad_cls, "grad_reg": grad_reg, "grad_iou_branch": grad_iou_branch, "aux": aux}


def terms_vector(terms):
    return np.array([terms[k] for k in TERM_NAMES])

"""The fused training losses on the GPU (epnet_amd/loss_utils.py over csrc/loss.hip).

Bounds. Against the reference's float64 run (tests/golden/loss.npz): per compared tensor the bound the generator stored, 4 x the
deviation of the reference's own float32 run from its float64 run and not less than 1e-6 of the tensor's largest magnitude. In
the sweep, where there is no reference run, the same rule is evaluated by the restatement: yardstick = the float64 restatement
(held to the reference at 1e-9 in test_loss.py), bound = 4 x |float32 restatement - float64 restatement|, floor 1e-6 of the
largest magnitude. Between runs of the kernel on the same inputs: bit-equal."""
import numpy as np
import pytest
import torch

import loss_cases as lc
import loss_restate as lr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FX = lc.load()
NAMES = list(lc.CASES)


def cfg_of(s):
    """loss_utils.default_cfg() with a restatement settings dict written into it (both stages get the same values)"""
    from epnet_amd import loss_utils
    cfg = loss_utils.default_cfg()
    for st in (cfg.RPN, cfg.RCNN):
        st.LOC_SCOPE, st.LOC_BIN_SIZE, st.NUM_HEAD_BIN, st.LOSS_CLS = s["loc_scope"], s["loc_bin_size"], s["num_head_bin"], s["cls_type"]
        st.FOCAL_ALPHA, st.FOCAL_GAMMA = [s["alpha"], 1 - s["alpha"]], s["gamma"]
    cfg.RPN.FG_WEIGHT, cfg.RPN.LOSS_WEIGHT = s["fg_weight"], [s["w_cls"], s["w_reg"]]
    cfg.TRAIN.IOU_LOSS_TYPE, cfg.TRAIN.CE_WEIGHT, cfg.USE_IOU_BRANCH = s["iou_type"], s["ce_weight"], s["use_iou_branch"]
    cfg.TRAIN.RPN_TRAIN_WEIGHT = cfg.TRAIN.RCNN_TRAIN_WEIGHT = s["w_train"]
    return cfg


def run_public(stage, s, inp, backward=True, scale=None):
    """one loss through rpn_loss / rcnn_loss -> (LossReturn, leaves [cls, reg, branch or None])"""
    from epnet_amd import loss_utils
    rows = inp["cls_label"].shape[0]
    t = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dt)  # noqa: E731
    cls = t(inp["cls_logit"]).view(rows, 1).requires_grad_(True)
    reg = t(inp["pred_reg"]).requires_grad_(True)
    branch = None
    if stage == "rpn":
        split = 2 if rows % 2 == 0 else 1
        out = loss_utils.rpn_loss(cls.view(split, rows // split, 1), reg.view(split, rows // split, -1),
                                  t(inp["cls_label"], torch.int64).view(split, -1), t(inp["reg_label"]).view(split, -1, 7), cfg_of(s))
    else:
        ret = {"rcnn_cls": cls, "rcnn_reg": reg, "cls_label": t(inp["cls_label"], torch.int64), "gt_of_rois": t(inp["reg_label"]),
               "reg_valid_mask": t(inp["reg_mask"], torch.int64)}
        if s["use_iou_branch"]:
            branch = t(inp["iou_branch"]).view(rows, 1).requires_grad_(True)
            ret["rcnn_iou_branch"] = branch
        out = loss_utils.rcnn_loss(ret, cfg_of(s))
    if backward:
        (out.loss if scale is None else out.loss * scale).backward()
    return out, [cls, reg, branch]


@pytest.mark.parametrize("name", NAMES)
def test_fixture_cases_through_the_public_functions(hiplib, name):
    s, inp = lc.settings(name), lc.inputs(FX, name)
    out, leaves = run_public(lc.CASES[name][0], s, inp)
    terms = out.terms.cpu().numpy().astype(np.float64)
    assert float(out.loss) == float(np.float32(terms[0]))
    failures = []
    for key, term, want, bound in lc.reference_scalars(FX, name):
        got = terms[lr.TERM_NAMES.index(term)]
        print("%s %-18s got % .9e want % .9e |diff| %.2e bound %.2e" % (name, key, got, want, abs(got - want), bound))
        if not abs(got - want) <= bound:
            failures.append((key, got, want, bound))
    for g, leaf in zip(("grad_cls", "grad_reg", "grad_iou_branch"), leaves):
        k = name + "__" + g + "_f64"
        if k not in FX.files:
            assert leaf is None
            continue
        want, bound = FX[k], float(FX[name + "__" + g + "_bound"])
        got = leaf.grad.cpu().numpy().astype(np.float64).reshape(want.shape)
        diff = float(np.abs(got - want).max())
        print("%s %-18s max |diff| %.2e bound %.2e (max |want| %.2e)" % (name, g, diff, bound, float(np.abs(want).max())))
        if not diff <= bound:
            failures.append((g, diff, bound))
    assert not failures, failures


def draw(stage, s, rows, fg_share, seed, minus_one=True):
    """seeded inputs of the sweep: N(0,1) predictions (rounded to float16 numbers), labels as in the fixture's case (b)"""
    rng = np.random.default_rng(seed)
    c = lr.channels(s)
    u = rng.uniform(size=rows)
    if fg_share == "one":
        fg = np.zeros(rows, bool)
        fg[rows // 2] = True
    else:
        fg = u < fg_share
    other = rng.uniform(size=rows)
    cls_label = np.where(fg, 1, np.where((other > 0.9) & minus_one, -1, 0)).astype(np.int64)
    reg_mask = None
    if stage == "rcnn":
        reg_mask = fg.astype(np.int64)
        cls_label = np.where(fg & (other > 0.2), 1, np.where((other > 0.9) & minus_one, -1, 0)).astype(np.int64)
    scope = s["loc_scope"]
    lab = np.zeros((rows, 7))
    lab[:, 0], lab[:, 2] = rng.uniform(-scope, scope, rows) * 1.1, rng.uniform(-scope, scope, rows) * 1.1
    lab[:, 1] = rng.normal(0, 0.3, rows)
    lab[:, 3:6] = np.asarray(s["anchor"]) * (1 + 0.1 * rng.normal(size=(rows, 3)))
    lab[:, 6] = rng.uniform(-2 * np.pi, 3 * np.pi, rows)
    inp = {"cls_logit": (rng.normal(size=rows) * 1.5).astype(np.float32), "pred_reg": rng.normal(size=(rows, c)).astype(np.float16).astype(np.float32),
           "reg_label": lab.astype(np.float32), "cls_label": cls_label, "reg_mask": reg_mask, "iou_branch": None}
    if s["use_iou_branch"]:
        inp["iou_branch"] = rng.uniform(-0.1, 1.1, rows).astype(np.float32)
    return inp


def settle(s, inp, seed, fg_only=False):
    """the generator's rule for continuous draws: a foreground row within 1e-4 of a kink (a smooth-L1 argument at +-1, the two
    operands of a clamp / min / max within 1e-4 relative) is redrawn -- a float32 and a float64 evaluation may fall on different
    sides of a kink that is closer than rounding, and then differ by a whole term"""
    rng = np.random.default_rng(seed + 12345)
    c = inp["pred_reg"].shape[1]
    for _ in range(20):
        aux = lr.box_loss(s, dtype=np.float64, fg_only=fg_only, **inp)["aux"]
        bad = np.nonzero((aux["margin_smooth_l1"] < 1e-4) | (aux["margin_relative"] < 1e-4))[0]
        if not len(bad):
            return inp
        assert len(bad) <= max(1, 0.01 * len(aux["fg_rows"])) + 2
        inp["pred_reg"][bad if fg_only else aux["fg_rows"][bad]] = rng.normal(size=(len(bad), c)).astype(np.float16).astype(np.float32)
        if inp["iou_branch"] is not None:
            inp["iou_branch"][aux["fg_rows"][bad]] = rng.uniform(0.01, 0.99, len(bad)).astype(np.float32)
    raise AssertionError("rows on a kink after 20 redraws")


def bound_rule(r64, r32):
    r64, r32 = np.asarray(r64, np.float64), np.asarray(r32, np.float64)
    if r64.size == 0:
        return 0.0
    return max(4 * float(np.abs(r32 - r64).max()), 1e-6 * float(np.abs(r64).max()))


def check_against_restatement(stage, s, inp, tag):
    inp = settle(s, inp, seed=len(str(tag)))
    o64, o32 = lr.box_loss(s, dtype=np.float64, **inp), lr.box_loss(s, dtype=np.float32, **inp)
    out, leaves = run_public(stage, s, inp)
    terms = out.terms.cpu().numpy().astype(np.float64)
    failures = []
    for i, k in enumerate(lr.TERM_NAMES):
        b = bound_rule(o64["terms"][k], o32["terms"][k])
        if not abs(terms[i] - float(o64["terms"][k])) <= b:
            failures.append((tag, k, terms[i], float(o64["terms"][k]), b))
    for g, leaf in zip(("grad_cls", "grad_reg", "grad_iou_branch"), leaves):
        if leaf is None:
            continue
        want = o64[g].reshape(leaf.shape)
        b = bound_rule(want, o32[g].reshape(leaf.shape))
        diff = float(np.abs(leaf.grad.cpu().numpy().astype(np.float64) - want).max())
        if not diff <= b:
            failures.append((tag, g, diff, b))
    return failures


SWEEP_ROWS = (1, 63, 64, 65, 4097, 2 * 16384)
SWEEP_FG = (0.0, "one", 0.02, 0.5, 1.0)


@pytest.mark.parametrize("rows", SWEEP_ROWS)
def test_sweep_against_the_float64_restatement(hiplib, rows):
    """rows x foreground share x (nb, nh) x IoU type x heading mode x IoU branch x classification loss, labels with -1 rows: the
    configurations are dealt over the (rows, share) grid so that every value of every axis meets every row count"""
    failures, k = [], 0
    bins = ((2, 1), (6, 9), (12, 12), (12, 1), (2, 12), (6, 12), (12, 9), (2, 9), (6, 1))
    for fg_share in SWEEP_FG:
        for variant in range(4 if rows <= 4097 else 2):
            k += 1
            nb, nh = bins[(k + variant) % len(bins)]
            stage = "rcnn" if (k + variant // 2) % 2 else "rpn"
            s = lr.settings(stage, loc_scope=nb * 0.25, loc_bin_size=0.5, num_head_bin=nh, iou_type=lr.IOU_TYPES[variant % 2],
                            cls_type=("SigmoidFocalLoss", "BinaryCrossEntropy")[(k // 2 + variant) % 2],
                            use_iou_branch=(stage == "rcnn" and variant >= 1), w_train=1.0 if variant % 2 else 0.5)
            if stage == "rpn":
                s.update(w_cls=1.0 if variant < 2 else 2.0, w_reg=1.0 if variant < 2 else 0.5)
            inp = draw(stage, s, rows, fg_share, seed=rows * 131 + k * 7 + variant)
            failures += check_against_restatement(stage, s, inp, (rows, fg_share, stage, nb, nh, s["iou_type"], s["cls_type"], s["use_iou_branch"]))
    assert not failures, failures[:10]


def test_full_batch_rows(hiplib):
    """256 x 16384 rows (the batch bench.py runs), 2 % foreground: the restatement runs over the foreground rows on the host,
    the background rows' gradients are checked to be zero on the device; the row offsets pass 2^31 bytes"""
    from epnet_amd import loss_utils
    rows = 256 * 16384
    s = lr.settings("rpn")
    c = lr.channels(s)
    g = torch.Generator(device=DEV).manual_seed(5)
    reg = torch.randn((rows, c), generator=g, device=DEV).half().float()
    cls = (torch.randn((rows, 1), generator=g, device=DEV) * 1.5).requires_grad_(True)
    u = torch.rand((rows,), generator=g, device=DEV)
    label = torch.where(u < 0.02, 1, torch.where(u > 0.95, -1, 0)).long()
    fg = torch.nonzero(label > 0)[:, 0]
    lab = torch.zeros((rows, 7), device=DEV)
    small = draw("rpn", s, int(fg.numel()), 1.0, seed=9)
    lab[fg] = torch.from_numpy(small["reg_label"]).to(DEV)
    inp = {"cls_logit": cls.detach().cpu().numpy().reshape(-1), "pred_reg": reg[fg].cpu().numpy(), "reg_label": small["reg_label"],
           "cls_label": label.cpu().numpy(), "reg_mask": None, "iou_branch": None}
    inp = settle(s, inp, seed=9, fg_only=True)
    reg[fg] = torch.from_numpy(inp["pred_reg"]).to(DEV)
    reg.requires_grad_(True)
    out = loss_utils.rpn_loss(cls.view(256, 16384, 1), reg.view(256, 16384, c), label.view(256, 16384), lab.view(256, 16384, 7), cfg_of(s))
    out.loss.backward()
    assert float(reg.grad.abs().sum(dim=1)[label <= 0].max()) == 0.0
    o64, o32 = lr.box_loss(s, dtype=np.float64, fg_only=True, **inp), lr.box_loss(s, dtype=np.float32, fg_only=True, **inp)
    terms = out.terms.cpu().numpy().astype(np.float64)
    failures = []
    for i, k in enumerate(lr.TERM_NAMES):
        b = bound_rule(o64["terms"][k], o32["terms"][k])
        print("%-22s got % .9e want % .9e bound %.2e" % (k, terms[i], float(o64["terms"][k]), b))
        if not abs(terms[i] - float(o64["terms"][k])) <= b:
            failures.append((k, terms[i], float(o64["terms"][k]), b))
    for name, got, want, w32 in (("grad_reg", reg.grad[fg], o64["grad_reg"], o32["grad_reg"]), ("grad_cls", cls.grad.view(-1), o64["grad_cls"], o32["grad_cls"])):
        b = bound_rule(want, w32)
        diff = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
        print("%-22s max |diff| %.2e bound %.2e" % (name, diff, b))
        if not diff <= b:
            failures.append((name, diff, b))
    assert not failures, failures


@pytest.mark.parametrize("stage", ["rpn", "rcnn"])
def test_no_foreground_is_exactly_zero(hiplib, stage):
    name = stage + "_nofg"
    out, leaves = run_public(stage, lc.settings(name), lc.inputs(FX, name))
    terms = out.terms.cpu().numpy()
    assert not terms[5:18].any() and terms[22] == 0 and terms[23] == 0 and terms[18] == 0
    assert terms[0].tobytes() == terms[2].tobytes() and terms[1].tobytes() == terms[2].tobytes()      # total == classification loss
    assert float(out.loss) == float(terms[2])
    assert not leaves[1].grad.any() and leaves[0].grad.any()


def _raw_call(inp_dev, s, stream=None):
    """the stand-in itself on prepared device tensors -> (terms, grad_cls, grad_reg, grad_branch)"""
    from epnet_amd import loss_cuda, loss_utils
    cls, reg, lab, label, mask, branch = inp_dev
    rows, c = reg.shape
    terms, g_cls, g_reg = torch.empty(24, device=DEV), torch.empty(rows, device=DEV), torch.empty((rows, c), device=DEV)
    g_br = torch.empty(rows, device=DEV) if branch is not None else None
    anchor = loss_utils._anchor_on(DEV, loss_utils.default_cfg())

    def go():
        loss_cuda.box_loss_gpu(cls, reg, lab, label, mask, branch, anchor, s["loc_scope"], s["loc_bin_size"], s["num_head_bin"], s["ry_fine"],
                               s["iou_type"], s["cls_type"], s["alpha"], s["gamma"], s["fg_weight"], s["w_cls"], s["w_reg"], s["w_train"],
                               s["ce_weight"], terms, g_cls, g_reg, g_br)
    if stream is None:
        go()
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            go()
        torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    return [t.clone() for t in (terms, g_cls, g_reg)] + ([g_br.clone()] if g_br is not None else [])


@pytest.mark.parametrize("stage,rows", [("rpn", 2 * 16384), ("rcnn", 128), ("rpn", 4097)])
def test_runs_are_bit_equal(hiplib, stage, rows):
    """twice on one stream and once on a side stream: no float atomics, a fixed order of every sum"""
    s = lr.settings(stage, use_iou_branch=(stage == "rcnn"))
    inp = draw(stage, s, rows, 0.5 if stage == "rcnn" else 0.03, seed=77)
    t = lambda a, dt: None if a is None else torch.from_numpy(a).to(DEV).to(dt).contiguous()  # noqa: E731
    dev_in = (t(inp["cls_logit"], torch.float32), t(inp["pred_reg"], torch.float32), t(inp["reg_label"], torch.float32),
              t(inp["cls_label"], torch.int32), t(inp["reg_mask"], torch.int32), t(inp["iou_branch"], torch.float32))
    a, b, c = _raw_call(dev_in, s), _raw_call(dev_in, s), _raw_call(dev_in, s, torch.cuda.Stream())
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
        assert x.cpu().numpy().tobytes() == z.cpu().numpy().tobytes()
    assert a[2].abs().sum() > 0


@pytest.mark.parametrize("stage", ["rpn", "rcnn"])
def test_forward_and_backward_in_one_graph(hiplib, stage):
    """forward + backward of the public function captured in ONE torch.cuda.graph (the capture fails on any synchronisation with
    the host), replayed on new inputs, against the eager run on those inputs: bit-equal"""
    from epnet_amd import loss_utils
    rows = 2 * 4096 if stage == "rpn" else 128
    s = lr.settings(stage, use_iou_branch=(stage == "rcnn"))
    cfg = cfg_of(s)
    first, second = draw(stage, s, rows, 0.05 if stage == "rpn" else 0.5, seed=1), draw(stage, s, rows, 0.08 if stage == "rpn" else 0.4, seed=2)
    t = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dt)  # noqa: E731
    static = {"cls": t(first["cls_logit"]).view(rows, 1).requires_grad_(True), "reg": t(first["pred_reg"]).requires_grad_(True),
              "lab": t(first["reg_label"]), "label": t(first["cls_label"], torch.int64),
              "mask": None if first["reg_mask"] is None else t(first["reg_mask"], torch.int64),
              "branch": None if first["iou_branch"] is None else t(first["iou_branch"]).view(rows, 1).requires_grad_(True)}

    def step():
        if stage == "rpn":
            out = loss_utils.rpn_loss(static["cls"].view(2, -1, 1), static["reg"].view(2, rows // 2, -1), static["label"].view(2, -1),
                                      static["lab"].view(2, -1, 7), cfg)
        else:
            out = loss_utils.rcnn_loss({"rcnn_cls": static["cls"], "rcnn_reg": static["reg"], "cls_label": static["label"],
                                        "reg_valid_mask": static["mask"], "gt_of_rois": static["lab"], "rcnn_iou_branch": static["branch"]}, cfg)
        leaves = [static["cls"], static["reg"]] + ([static["branch"]] if static["branch"] is not None else [])
        grads = torch.autograd.grad(out.loss, leaves)
        return [out.loss, out.terms] + list(grads)
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
    eager_first = step()
    assert all(torch.equal(a, b) for a, b in zip(eager_first, captured))
    with torch.no_grad():
        static["cls"].copy_(t(second["cls_logit"]).view(rows, 1)); static["reg"].copy_(t(second["pred_reg"]))
        static["lab"].copy_(t(second["reg_label"])); static["label"].copy_(t(second["cls_label"], torch.int64))
        if static["mask"] is not None:
            static["mask"].copy_(t(second["reg_mask"], torch.int64))
        if static["branch"] is not None:
            static["branch"].copy_(t(second["iou_branch"]).view(rows, 1))
    graph.replay()
    torch.cuda.synchronize()
    eager_second = step()
    assert all(torch.equal(a, b) for a, b in zip(eager_second, captured))
    assert not torch.equal(eager_second[1], eager_first[1])


def test_backward_scales_by_the_incoming_gradient(hiplib):
    name = "rcnn_b_bin_branch"
    s, inp = lc.settings(name), lc.inputs(FX, name)
    _, plain = run_public("rcnn", s, inp)
    _, scaled = run_public("rcnn", s, inp, scale=0.25)
    for a, b in zip(plain, scaled):
        assert torch.equal(a.grad * 0.25, b.grad)


def test_dice_loss_stays_a_torch_expression_behind_the_same_surface(hiplib):
    name = "rpn_b_bin"
    s, inp = dict(lc.settings(name), cls_type="DiceLoss"), lc.inputs(FX, name)
    out, leaves = run_public("rpn", s, inp)
    none = lr.box_loss(dict(s, cls_type="none"), dtype=np.float64, **inp)
    p = 1 / (1 + np.exp(-inp["cls_logit"].astype(np.float64)))
    tgt, m = inp["cls_label"].astype(np.float64), (inp["cls_label"] != -1)
    dice = 1 - (np.minimum(p, tgt) * m).sum() / max((np.maximum(p, tgt) * m).sum(), 1.0)
    terms = out.terms.cpu().numpy()
    assert abs(terms[2] - dice) <= 1e-5 * abs(dice) and abs(float(out.loss) - (dice + float(none["terms"]["loss_reg"]))) <= 1e-5 * abs(float(out.loss))
    assert leaves[0].grad.abs().sum() > 0 and torch.isfinite(leaves[0].grad).all()


def test_masked_rows_of_the_rcnn_cross_entropy(hiplib):
    """-1 labels under BinaryCrossEntropy (no reference run exists for them, see test_loss.py): against the restatement"""
    s = lr.settings("rcnn")
    inp = draw("rcnn", s, 128, 0.5, seed=3, minus_one=True)
    assert (inp["cls_label"] == -1).any()
    assert not check_against_restatement("rcnn", s, inp, "masked")


def test_two_stage_step_with_the_real_losses(hiplib):
    """the two-stage model of bench_step.py at a reduced size takes one optimiser step with the real losses: finite terms,
    gradients on every parameter the placeholder loss reaches, and the loss of its own outputs equal to the restatement's"""
    import bench_step
    from epnet_amd import proposal_layer as pl, proposal_target_layer as ptl
    torch.manual_seed(0)
    np.random.seed(0)
    model = bench_step.build_model(scale=8, loss="reference").to(DEV)
    layers = (pl.ProposalLayer("TRAIN").to(DEV), ptl.ProposalTargetLayer())
    xyz, gts = bench_step.synthetic_batch(2, 2048, 7, DEV)
    model.rpn_labels = bench_step.rpn_labels(xyz, gts)
    opt = torch.optim.SGD(model.parameters(), lr=1e-4)
    opt.zero_grad(set_to_none=True)
    loss, out = bench_step.run_step(model, layers, xyz, gts)
    loss.backward()
    opt.step()
    for key in ("rpn_loss", "rcnn_loss"):
        assert torch.isfinite(out[key].terms).all(), (key, out[key].terms)
    assert float(out["rpn_loss"].terms[18]) > 0          # some points lie in a ground-truth box
    missing = [n for n, p in model.named_parameters() if p.grad is None]
    assert not missing, missing
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())
    first = next(p for n, p in model.named_parameters() if n.startswith("backbone.SA_modules.0") and n.endswith("conv.weight"))
    assert float(first.grad.abs().sum()) > 0
    # the losses of the step's own outputs against the restatement
    cls_label, reg_label = model.rpn_labels
    n = lambda t: t.detach().cpu().numpy()  # noqa: E731
    cases = (("rpn", lr.settings("rpn"), {"cls_logit": n(out["rpn_cls"]).reshape(-1), "pred_reg": n(out["rpn_reg"]).reshape(-1, 76),
                                          "reg_label": n(reg_label).reshape(-1, 7), "cls_label": n(cls_label).reshape(-1), "reg_mask": None,
                                          "iou_branch": None}, out["rpn_loss"]),
             ("rcnn", lr.settings("rcnn"), {"cls_logit": n(out["rcnn_cls"]).reshape(-1), "pred_reg": n(out["rcnn_reg"]).reshape(-1, 46),
                                            "reg_label": n(out["target"]["gt_of_rois"]).reshape(-1, 7), "cls_label": n(out["target"]["cls_label"]),
                                            "reg_mask": n(out["target"]["reg_valid_mask"]), "iou_branch": None}, out["rcnn_loss"]))
    failures = []
    for stage, s, inp, got in cases:
        o64, o32 = lr.box_loss(s, dtype=np.float64, **inp), lr.box_loss(s, dtype=np.float32, **inp)
        terms = got.terms.cpu().numpy().astype(np.float64)
        for i, k in enumerate(lr.TERM_NAMES):
            b = bound_rule(o64["terms"][k], o32["terms"][k])
            print("%s %-22s got % .9e want % .9e bound %.2e" % (stage, k, terms[i], float(o64["terms"][k]), b))
            if not abs(terms[i] - float(o64["terms"][k])) <= b:
                failures.append((stage, k, terms[i], float(o64["terms"][k]), b))
    assert not failures, failures
    assert abs(float(loss) - (float(out["rpn_loss"].loss) + float(out["rcnn_loss"].loss))) <= 1e-6 * abs(float(loss))


def test_bench_step_prints_its_line_with_the_real_losses(hiplib):
    import json
    import os
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(lc.HERE, "..", "bench_step.py"), "--loss", "reference", "--points", "2048", "--batch", "2",
                          "--steps", "2", "--warmup", "1"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().split("\n")[-1])
    assert line["loss_mode"] == "reference" and np.isfinite(line["loss"])
    assert set(line["loss_terms"]) >= {"rpn_loss", "rpn_loss_iou", "rcnn_loss", "rcnn_reg_fg"}
    assert all(np.isfinite(v) for v in line["loss_terms"].values())

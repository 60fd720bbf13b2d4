"""The fused optimiser on the GPU: epnet_adam_onecycle_step through epnet_amd.optim.FusedAdamOneCycle against the numpy
restatement (tests/optim_restate.py, bit for bit) and against the reference's own run (tests/golden/optim.npz).

Tensors: the fixture model's nine parameters plus sizes around the kernel's paths -- 1, 3, 4, 5 (below one 16-byte group),
chunk-1, chunk, chunk+1 (the full-chunk path and its neighbours) and 2 chunk + 3 (several workgroups and a tail).

Bounds. Against the restatement: p, exp_avg and exp_avg_sq equal bit for bit once it is given the device's clip coefficient --
the update is float32 in source order on both sides, and the only quantity summed in another order is the norm. total_norm:
1e-6 relative to the float64 sum (the kernels sum in float64; 1e-6 is far above its rounding and far below a dropped tensor).
Against the fixture: max(2 x the reference's own float32 error, 2^-23 max |p|) per step, as tests/test_optim.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import optim_cases as oc
import optim_restate as orr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = oc.load()
CHUNK = 4096
EXTRA = (1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
DEV = torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def initial(extra=EXTRA):
    """name -> float32 array: the fixture's parameters, then one tensor per extra size"""
    rng = np.random.default_rng(7)
    out = dict(oc.split(FX["p0"]))
    for k, n in enumerate(extra):
        out["extra%d" % k] = (rng.standard_normal(n) * 0.5).astype(np.float32)
    return out


def gradients(t, names, sizes):
    """name -> float32 array or None for step t: the fixture's (cycled past its 12 steps), the extras' drawn at the same scale"""
    rng = np.random.default_rng(100 + t)
    by_name = oc.split(FX["grads"][t % oc.STEPS], oc.GRAD_NAMES)
    scale = 450.0 if t % 3 == 2 else 0.45
    out = {}
    for n in names:
        if n.startswith("extra"):
            size = sizes[n]
            out[n] = (rng.standard_normal(size) * scale / 400).astype(np.float32)
        else:
            out[n] = by_name.get(n)
    return out


class Run:
    """an optimiser over a parameter list on the device; grads: 'separate' tensors or 'views' into one flat buffer at element
    offsets 1, 2, 3 (mod 4) in turn, the way DistributedDataParallel's gradient_as_bucket_view lays them out"""

    def __init__(self, extra=EXTRA, total_steps=oc.TOTAL_STEPS, zero_grads=True, grads="separate", frozen=True):
        from epnet_amd import optim
        self.p0 = initial(extra)
        self.names = list(self.p0)
        self.params = [torch.nn.Parameter(torch.from_numpy(self.p0[n].copy()).to(DEV)) for n in self.names]
        self.opt = optim.FusedAdamOneCycle(self.params, total_steps, wd=oc.WD, beta2=oc.BETA2, eps=oc.EPS, grad_norm_clip=oc.CLIP,
                                           zero_grads=zero_grads, **oc.SETTINGS)
        if frozen:
            self.params[self.names.index(oc.FROZEN)].requires_grad = False
        self.live = [n for n in self.names if not (frozen and n == oc.FROZEN)]
        self.layout = grads
        self.bucket = None
        self.t = 0

    def set_grads(self):
        g = gradients(self.t, self.names, {n: a.size for n, a in self.p0.items()})
        if self.layout == "views" and self.bucket is None:
            at, self.slots = 0, {}
            for k, n in enumerate(self.live):
                if g[n] is None:
                    continue
                at = (at + 3) // 4 * 4 + 1 + k % 3                 # offset = 1, 2 or 3 (mod 4 elements)
                self.slots[n] = at
                at += g[n].size
            self.bucket = torch.zeros((at + 4,), device=DEV)
        for n, p in zip(self.names, self.params):
            if n not in self.live or g[n] is None:
                continue
            new = torch.from_numpy(g[n]).to(DEV).view(p.shape)
            if p.grad is None:
                if self.layout == "views":
                    p.grad = self.bucket[self.slots[n]:self.slots[n] + p.numel()].view(p.shape)
                    assert p.grad.data_ptr() % 16 != 0
                    p.grad.copy_(new)
                else:
                    p.grad = new.clone()
            else:
                p.grad.copy_(new)
        return [g[n] for n in self.live]

    def step(self):
        grads = self.set_grads()
        self.opt.step()
        self.t += 1
        torch.cuda.synchronize()
        return grads

    def snapshot(self):
        p = {n: q.detach().cpu().numpy() for n, q in zip(self.names, self.params)}
        m = {n: self.opt._piece(self.opt.exp_avg, i).cpu().numpy() for i, n in enumerate(self.names)}
        v = {n: self.opt._piece(self.opt.exp_avg_sq, i).cpu().numpy() for i, n in enumerate(self.names)}
        return p, m, v, dict(zip(("total_norm", "coef", "lr", "mom", "step", "past_end"), self.opt.stats.tolist()))


def run_steps(run, steps):
    out, grads = [], []
    for _ in range(steps):
        grads.append(run.step())
        out.append(run.snapshot())
    return out, grads


_FOUR_STEPS = []


@pytest.fixture()
def four_steps(hiplib):
    """four steps (the third clips) of the fixture model + extras with separate gradient tensors, and the restatement of the
    same steps with the device's coefficients: computed once, by the first test that asks -- inside that test, a function-scoped
    fixture, so that the allocation canaries of tests/conftest.py are already around its state buffers and workspace --, then
    shared and never modified"""
    if not _FOUR_STEPS:
        run = Run()
        snaps, grads = run_steps(run, 4)
        want = list(orr.run([run.p0[n] for n in run.live], grads, oc.TOTAL_STEPS, wd=oc.WD, b2=oc.BETA2, eps=oc.EPS, clip=oc.CLIP,
                            coefs=[s[3]["coef"] for s in snaps], **oc.SETTINGS))
        _FOUR_STEPS.append((run, snaps, grads, want))
    return _FOUR_STEPS[0]


def test_kernels_equal_the_restatement_bit_for_bit(four_steps):
    run, snaps, grads, want = four_steps
    for t, ((p, m, v, stats), (wp, wm, wv, info)) in enumerate(zip(snaps, want)):
        rel = abs(stats["total_norm"] - info["total_norm"]) / info["total_norm"]
        print("step %d total_norm %.9f (float64 %.9f, rel %.1e) coef %.9g (restated %.9g) lr %.6e mom %.6f"
              % (t, stats["total_norm"], info["total_norm"], rel, stats["coef"], orr.clip_coef(info["total_norm"], oc.CLIP), stats["lr"], stats["mom"]))
        assert rel <= 1e-6
        assert np.float32(stats["coef"]) == orr.clip_coef(stats["total_norm"], oc.CLIP)   # the header's formula on the device's own norm
        assert (stats["coef"] < 1) == (t % 3 == 2)
        assert stats["lr"] == float(np.float32(info["lr"])) and stats["mom"] == float(np.float32(info["mom"]))
        assert stats["step"] == t and stats["past_end"] == 0
        for k, n in enumerate(run.live):
            assert same_bits(p[n].reshape(-1), wp[k].reshape(-1)), ("p", t, n, np.abs(p[n].reshape(-1) - wp[k].reshape(-1)).max())
            assert same_bits(m[n].reshape(-1), wm[k].reshape(-1)), ("exp_avg", t, n)
            assert same_bits(v[n].reshape(-1), wv[k].reshape(-1)), ("exp_avg_sq", t, n)
    assert int(run.opt.counter[0]) == 4


def test_missing_gradient_only_decays_and_frozen_parameter_is_untouched(four_steps):
    run, snaps, grads, want = four_steps
    p, m, v, _ = snaps[-1]
    decayed = run.p0[oc.NO_GRAD].copy()
    for t in range(4):
        lr, _mom = orr.one_cycle(t, oc.TOTAL_STEPS, **oc.SETTINGS)
        decayed = decayed * np.float32(1 - oc.WD * lr)
    assert same_bits(p[oc.NO_GRAD], decayed) and not np.array_equal(decayed, run.p0[oc.NO_GRAD])
    assert not m[oc.NO_GRAD].any() and not v[oc.NO_GRAD].any()
    assert same_bits(p[oc.FROZEN], run.p0[oc.FROZEN]) and not m[oc.FROZEN].any() and not v[oc.FROZEN].any()
    assert run.params[run.names.index(oc.NO_GRAD)].grad is None and run.params[run.names.index(oc.FROZEN)].grad is None
    assert m["fc.weight"].any() and v["extra7"].all()


def test_zero_grads_leaves_every_gradient_zero_at_the_same_address(hiplib):
    run = Run()
    run.step()
    where = {n: p.grad.data_ptr() for n, p in zip(run.names, run.params) if p.grad is not None}
    assert len(where) == len(run.live) - 1
    for _ in range(2):
        run.step()
        for n, p in zip(run.names, run.params):
            if p.grad is not None:
                assert p.grad.data_ptr() == where[n] and not bool(p.grad.any()), n
    run.opt.zero_grad()                                        # nothing to do, nothing moved
    assert {n: p.grad.data_ptr() for n, p in zip(run.names, run.params) if p.grad is not None} == where
    keep = Run(zero_grads=False)
    keep.step()
    assert all(bool(p.grad.any()) for p in keep.params if p.grad is not None)
    keep.opt.zero_grad()
    assert not any(bool(p.grad.any()) for p in keep.params if p.grad is not None)


def test_gradients_as_views_at_odd_offsets_give_the_same_bits(four_steps):
    _, snaps, _, _ = four_steps
    run = Run(grads="views")
    got, _ = run_steps(run, 4)
    assert sorted({run.slots[n] % 4 for n in run.slots}) == [1, 2, 3]
    for t in range(4):
        assert got[t][3] == snaps[t][3], (t, got[t][3], snaps[t][3])          # stats: the norm's bits do not depend on the layout
        for which in range(3):
            for n in run.names:
                assert same_bits(got[t][which][n], snaps[t][which][n]), (t, which, n)
    assert not bool(run.bucket.any())                          # zeroed in place, nothing written between the views


def test_two_runs_give_identical_bits(four_steps):
    _, snaps, _, _ = four_steps
    again, _ = run_steps(Run(), 4)
    for t in range(4):
        assert again[t][3] == snaps[t][3]
        for which in range(3):
            assert all(same_bits(again[t][which][n], snaps[t][which][n]) for n in snaps[t][which])


def test_within_twice_the_reference_float32_error_of_the_fixture(hiplib):
    run = Run(extra=())
    failures = []
    for t in range(oc.STEPS):
        run.step()
        p, _, _, stats = run.snapshot()
        err = float(np.abs(oc.join(p).astype(np.float64) - FX["p64"][t]).max())
        bound = max(2 * float(FX["err32"][t]), 2.0 ** -23 * float(np.abs(FX["p64"][t]).max()))
        rel = abs(stats["total_norm"] - FX["total_norm"][t]) / FX["total_norm"][t]
        print("step %2d err %.3e reference float32 err %.3e ratio %.2f bound %.3e norm rel %.1e" % (t, err, FX["err32"][t], err / FX["err32"][t], bound, rel))
        assert rel <= 1e-6 and stats["lr"] == float(np.float32(FX["lr"][t])) and stats["mom"] == float(np.float32(FX["mom"][t]))
        if not err <= bound:
            failures.append((t, err, bound))
    assert not failures, failures


def test_past_total_steps_the_last_row_is_used_and_flagged(hiplib):
    total = 5
    run = Run(extra=(5, CHUNK + 1), total_steps=total)
    snaps, grads = run_steps(run, 7)
    assert [s[3]["step"] for s in snaps] == [0, 1, 2, 3, 4, 4, 4] and [s[3]["past_end"] for s in snaps] == [0, 0, 0, 0, 0, 1, 1]
    assert snaps[5][3]["lr"] == snaps[4][3]["lr"] and int(run.opt.counter[0]) == 7
    want = list(orr.run([run.p0[n] for n in run.live], grads, total, wd=oc.WD, b2=oc.BETA2, eps=oc.EPS, clip=oc.CLIP,
                        coefs=[s[3]["coef"] for s in snaps], **oc.SETTINGS))
    for k, n in enumerate(run.live):
        assert same_bits(snaps[-1][0][n].reshape(-1), want[-1][0][k].reshape(-1)), n


def test_resume_from_a_state_dict_equals_a_straight_run(hiplib):
    straight, _ = run_steps(Run(), 12)
    first = Run()
    run_steps(first, 6)
    sd = first.opt.state_dict()
    assert float(sd["state"][0]["step"]) == 6 and oc.NAMES.index(oc.NO_GRAD) not in sd["state"]
    second = Run()
    with torch.no_grad():
        for p, q in zip(second.params, first.params):
            p.copy_(q)
    second.opt.load_state_dict(sd)
    second.t = 6
    resumed, _ = run_steps(second, 6)
    assert resumed[-1][3] == straight[-1][3] and resumed[-1][3]["step"] == 11
    for which in range(3):
        for n in second.names:
            assert same_bits(resumed[-1][which][n], straight[-1][which][n]), (which, n)


def test_a_changed_address_rebuilds_and_a_capture_refuses_to(hiplib, monkeypatch):
    run = Run(extra=(5,))
    run.step()
    p = run.params[0]
    p.grad = p.grad.clone()                                     # a new address: picked up by the next step, eagerly
    run.step()
    assert not bool(p.grad.any())
    p.grad = p.grad.clone()
    before = p.detach().clone()
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)        # what step() asks; no capture is begun
        with pytest.raises(RuntimeError, match="graph capture"):
            run.opt.step()
    torch.cuda.synchronize()
    assert torch.equal(p.detach(), before) and int(run.opt.counter[0]) == 2       # refused before any launch


def _training_pair():
    """two copies of the fixture model with a loss that reaches every parameter, and their optimisers"""
    from epnet_amd import optim
    out = []
    for _ in range(2):
        torch.manual_seed(3)
        model = oc.build_model().to(DEV)
        opt = optim.FusedAdamOneCycle(model, oc.TOTAL_STEPS, **oc.SETTINGS)
        out.append((model, opt))
    return out


def test_forward_backward_and_step_replay_from_one_graph(hiplib, monkeypatch, request):
    """forward + backward + step() of the fixture model captured in ONE torch.cuda.graph (bench_step's model has its own capture
    test of forward and backward, tests/test_rcnn_targets_gpu.py; its dense layers pick algorithms per call, which would make
    'K replays == K eager steps' a statement about them), replayed K times with a new batch each, against K eager steps"""
    (model_e, opt_e), (model_g, opt_g) = _training_pair()
    # bit-equal gradients from two runs of the dense layers need their deterministic algorithms (bench_step.infer asks for the
    # same): without them the batch-norm / convolution gradients differ in the last bits from run to run, eager or replayed
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    request.addfinalizer(lambda: torch.use_deterministic_algorithms(prev))
    gen = torch.Generator().manual_seed(11)
    batches = [torch.randn((4, 5, 33), generator=gen).to(DEV) for _ in range(3 + 5)]
    static = torch.empty_like(batches[0])

    def train_step(model, opt, x):
        y = model.bn2(model.conv2(torch.relu(model.bn1(model.conv1(x)))))      # (4, 3, 33)
        z = model.fc(y.mean(dim=(1, 2)).view(-1, 1))                           # (4, 1031)
        loss = (z * z).mean() + y.abs().mean() * 30
        loss.backward()
        opt.step()
        return loss
    warm, k_steps = 3, 5
    for k in range(warm + k_steps):
        train_step(model_e, opt_e, batches[k])
    steps_used = []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for k in range(warm):
            static.copy_(batches[k])
            train_step(model_g, opt_g, static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        train_step(model_g, opt_g, static)
    lrs, norms = [], []
    for k in range(warm, warm + k_steps):
        static.copy_(batches[k])
        graph.replay()
        torch.cuda.synchronize()
        stats = opt_g.stats.tolist()
        lrs.append(stats[2]); norms.append(stats[0]); steps_used.append(stats[4])
    print("learning rates of the replays:", lrs, "norms:", norms)
    assert len(set(lrs)) == k_steps and steps_used == [float(t) for t in range(warm, warm + k_steps)]
    assert int(opt_g.counter[0]) == int(opt_e.counter[0]) == warm + k_steps
    assert opt_g.stats.tolist() == opt_e.stats.tolist()
    for (n, p), q in zip(model_g.named_parameters(), model_e.parameters()):
        assert torch.equal(p, q), n
    assert torch.equal(opt_g.exp_avg, opt_e.exp_avg) and torch.equal(opt_g.exp_avg_sq, opt_e.exp_avg_sq)
    for b, c in zip(model_g.buffers(), model_e.buffers()):
        assert torch.equal(b, c)
    assert all(bool(torch.isfinite(p).all()) for p in model_g.parameters()) and norms[0] > 0


def _rcnn_inputs(b, m, n, seed, cfg):
    """static inputs and sampling tables of RCNNTargetLayer, as tests/test_rcnn_targets_gpu.py builds them"""
    from epnet_amd import rcnn_target_layer as rtl, synth
    g = torch.Generator().manual_seed(seed)
    rois, gts = [], []
    for i in range(b):
        boxes, _ = synth.proposal_boxes(m + 12, seed=seed + i, num_objects=12, jitter=0.4)
        gt = torch.zeros((20, 7))
        gt[:12] = boxes[m:]
        rois.append(boxes[:m])
        gts.append(gt)
    inputs = {"roi_boxes3d": torch.stack(rois).to(DEV), "gt_boxes3d": torch.stack(gts).to(DEV),
              "rpn_xyz": synth.scenes("kitti", b, n, seed=seed).to(DEV), "rpn_features": torch.randn((b, n, 128), generator=g).to(DEV),
              "seg_mask": (torch.rand((b, n), generator=g) > 0.5).float().to(DEV), "pts_depth": (torch.rand((b, n), generator=g) * 70).to(DEV)}
    gd = torch.Generator(device=DEV).manual_seed(seed)
    tables = rtl.draw_sampling_tables(b, m, cfg, DEV, gd)
    draws = [torch.rand((b, cfg.RCNN.ROI_PER_IMAGE), device=DEV, generator=gd) for _ in range(3)]
    tables["aug"] = rtl.aug_table_from_draws(*draws, cfg)
    return inputs, tables


def test_rcnn_stage_with_fused_targets_loss_and_step_replays_from_one_graph(hiplib):
    """the part of bench_step's model that tests/test_rcnn_targets_gpu.py shows to capture -- RCNNTargetLayer, the RCNN stage of
    build_model(scale=8), rcnn_loss, forward and backward -- now WITH the optimiser step in the same torch.cuda.graph: K replays on
    rewritten inputs and tables equal K eager steps bit for bit, each with its own learning rate. Deterministic gradients
    ("Reproducible gradients"), as there: the default scatter-add gradients use float atomics."""
    import copy
    import bench_step
    from epnet_amd import loss_utils, optim, rcnn_target_layer as rtl
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        torch.manual_seed(0)
        b, m, n, warm, k_steps = 2, 128, 2048, 2, 3
        cfg = rtl.default_cfg()
        cfg.RCNN.ROI_PER_IMAGE, cfg.RCNN.ROI_FG_AUG_TIMES, cfg.RCNN.NUM_POINTS = 16, 10, 512
        rcnn_e = bench_step.build_model(scale=8, loss="reference").to(DEV).rcnn
        rcnn_g = copy.deepcopy(rcnn_e)
        opt_e, opt_g = optim.FusedAdamOneCycle(rcnn_e, oc.TOTAL_STEPS), optim.FusedAdamOneCycle(rcnn_g, oc.TOTAL_STEPS)
        assert sum(p.numel() for p in opt_e.params) == sum(p.numel() for p in rcnn_e.parameters())
        layer, loss_cfg = rtl.RCNNTargetLayer(cfg), loss_utils.default_cfg()
        data = [_rcnn_inputs(b, m, n, 400 + 10 * k, cfg) for k in range(warm + k_steps)]
        static, static_tables = ({k: v.clone() for k, v in d.items()} for d in data[0])

        def train_step(rcnn, opt, inputs, tables):
            with torch.no_grad():
                target = layer(inputs, tables)
            rcnn_cls, rcnn_reg = rcnn(target["sampled_pts"], target["pts_feature"])
            out = loss_utils.rcnn_loss(dict(target, rcnn_cls=rcnn_cls.view(rcnn_cls.shape[0], -1), rcnn_reg=rcnn_reg.view(rcnn_reg.shape[0], -1)), loss_cfg)
            out.loss.backward()
            opt.step()
            return out.terms

        def rewrite(k):
            with torch.no_grad():
                for key in static:
                    static[key].copy_(data[k][0][key])
                for key in static_tables:
                    static_tables[key].copy_(data[k][1][key])
        for k in range(warm + k_steps):
            terms_e = train_step(rcnn_e, opt_e, *data[k]).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for k in range(warm):
                rewrite(k)
                train_step(rcnn_g, opt_g, static, static_tables)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            terms_g = train_step(rcnn_g, opt_g, static, static_tables)
        lrs = []
        for k in range(warm, warm + k_steps):
            rewrite(k)
            graph.replay()
            torch.cuda.synchronize()
            lrs.append(opt_g.stats[2].item())
        print("learning rates of the replays:", lrs, "stats", opt_g.stats.tolist())
        assert len(set(lrs)) == k_steps and opt_g.stats.tolist() == opt_e.stats.tolist() and opt_g.stats[0].item() > 0
        assert torch.equal(terms_g, terms_e)
        for (name, p), q in zip(rcnn_g.named_parameters(), rcnn_e.parameters()):
            assert torch.equal(p, q), name
        assert torch.equal(opt_g.exp_avg, opt_e.exp_avg) and torch.equal(opt_g.exp_avg_sq, opt_e.exp_avg_sq) and bool(opt_g.exp_avg_sq.any())
    finally:
        torch.use_deterministic_algorithms(prev)


def test_bench_step_with_the_fused_optimiser_prints_its_line(hiplib):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench_step.py"), "--optimizer", "fused", "--points", "2048", "--batch", "2",
                        "--steps", "2", "--warmup", "1"], cwd=ROOT, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    print(line["phase_ms"], line["optimizer_stats"])
    assert line["optimizer"] == "fused" and line["phase_ms"]["optimizer"] > 0
    assert line["optimizer_stats"]["past_end"] == 0 and line["optimizer_stats"]["total_norm"] > 0 and 0 < line["optimizer_stats"]["lr"] <= float(np.float32(0.002))
    assert np.isfinite(line["loss"])

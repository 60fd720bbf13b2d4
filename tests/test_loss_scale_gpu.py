"""Loss scaling and non-finite step skipping of the fused optimiser on the GPU: epnet_adam_onecycle_step_scaled through
``FusedAdamOneCycle(loss_scale=...)``.

The feature is defined as a composition of things that exist -- stock ``g * inv``, then epnet_adam_onecycle_step; stock
``torch._amp_update_scale_`` for the scale -- so every comparison here is bit for bit and there is no tolerance anywhere.

Tensors: the fixture model's nine parameters (tests/optim_cases.py: a frozen one, one without a gradient, fc.bias with 1031
elements on the short-chunk path) and two of 8197 elements -- two full 4096-element chunks and a tail of 5 --, ``big`` with a
gradient tensor of its own and ``bucket`` with a gradient that is a view at element offset 1 of a flat buffer."""
import numpy as np
import pytest
import torch

import loss_scale_restate as lsr
import optim_cases as oc

pytestmark = pytest.mark.gpu

FX = oc.load()
DEV = torch.device("cuda:0")
F = np.float32
BIG = 2 * 4096 + 5
NAMES = oc.NAMES + ("big", "bucket")
LIVE = tuple(n for n in NAMES if n != oc.FROZEN)
KW = dict(wd=oc.WD, beta2=oc.BETA2, eps=oc.EPS, grad_norm_clip=oc.CLIP, **oc.SETTINGS)
RESTATE_KW = dict(wd=oc.WD, b2=oc.BETA2, eps=oc.EPS, clip=oc.CLIP, **oc.SETTINGS)


def bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def same_bits(a, b):
    return np.size(a) == np.size(b) and np.array_equal(bits(a), bits(b))


def initial():
    rng = np.random.default_rng(7)
    out = dict(oc.split(FX["p0"]))
    for n in ("big", "bucket"):
        out[n] = (rng.standard_normal(BIG) * 0.5).astype(F)
    return out


def gradients(t, scale=1.0):
    """name -> float32 array (None: no gradient) of step t, every third one large enough to clip, times `scale` in float32"""
    rng = np.random.default_rng(100 + t)
    by_name = oc.split(FX["grads"][t % oc.STEPS], oc.GRAD_NAMES)
    size = 450.0 if t % 3 == 2 else 0.45
    out = {}
    for n in LIVE:
        g = (rng.standard_normal(BIG) * size / 400).astype(F) if n in ("big", "bucket") else by_name.get(n)
        out[n] = None if g is None else (np.asarray(g, F) * F(scale)).astype(F)
    return out


class Run:
    """an optimiser over the tensors above; step(grads) copies the gradients in (at fixed addresses) and steps"""

    def __init__(self, **kw):
        from epnet_amd import optim
        self.p0 = initial()
        self.params = [torch.nn.Parameter(torch.from_numpy(self.p0[n].copy()).to(DEV)) for n in NAMES]
        self.opt = optim.FusedAdamOneCycle(self.params, oc.TOTAL_STEPS, **dict(KW, **kw))
        self.params[NAMES.index(oc.FROZEN)].requires_grad = False
        self.flat = torch.zeros((BIG + 8,), device=DEV)

    def by_name(self, n):
        return self.params[NAMES.index(n)]

    def set_grads(self, grads, transform=None):
        for n in LIVE:
            if grads[n] is None:
                continue
            p = self.by_name(n)
            new = torch.from_numpy(np.ascontiguousarray(grads[n])).to(DEV).view(p.shape)
            if transform is not None:
                new = transform(new)
            if p.grad is None:
                if n == "bucket":
                    p.grad = self.flat[1:1 + BIG].view(p.shape)
                    assert p.grad.data_ptr() % 16 == 4
                else:
                    p.grad = torch.empty_like(new)
            p.grad.copy_(new)

    def step(self, grads, transform=None):
        self.set_grads(grads, transform)
        self.opt.step()
        torch.cuda.synchronize()
        return self.snapshot()

    def snapshot(self):
        opt = self.opt
        snap = {"p": {n: q.detach().cpu().numpy() for n, q in zip(NAMES, self.params)},
                "m": {n: opt._piece(opt.exp_avg, i).cpu().numpy() for i, n in enumerate(NAMES)},
                "v": {n: opt._piece(opt.exp_avg_sq, i).cpu().numpy() for i, n in enumerate(NAMES)},
                "stats": opt.stats.tolist(), "counter": int(opt.counter[0])}
        if opt.scale is not None:
            snap["scale"] = opt.scale.cpu().numpy()[0]
            snap["state"] = opt.scaler_state.tolist()
        return snap


def assert_same_state(a, b, what):
    for which in ("p", "m", "v"):
        for n in NAMES:
            assert same_bits(a[which][n], b[which][n]), (what, which, n)
    assert a["counter"] == b["counter"], what


def live_lists(by_name):
    return [by_name[n] for n in LIVE]


# ---- 1. the scaled entry equals stock g * inv followed by the existing entry ----------------------------------------------------
@pytest.mark.parametrize("scale", [65536.0, 1.0, 3.0, 2.0 ** -3])
def test_scaled_step_equals_stock_unscale_then_the_plain_step(hiplib, scale):
    scaled, plain = Run(loss_scale=scale, min_scale=min(1.0, scale)), Run()
    inv = torch.tensor(lsr.inverse(scale), device=DEV)                  # (float)(1.0 / (double)scale)
    assert float(inv) == float(F(1.0 / scale))
    fed, coefs, snaps = [], [], []
    for t in range(4):
        g = gradients(t, scale)
        a = scaled.step(g)
        b = plain.step(g, transform=lambda x: x * inv)                  # stock: one float32 multiply per element
        print("scale %g step %d stats %s" % (scale, t, a["stats"]))
        assert_same_state(a, b, (scale, t))
        assert a["stats"][:6] == b["stats"][:6] and a["counter"] == t + 1
        assert a["stats"][6] == scale and a["stats"][7] == 0 and b["stats"][6:] == [0.0, 0.0]
        assert same_bits(a["scale"], F(scale)) and a["state"] == [t + 1, 0]            # static: the scale does not move
        assert (a["stats"][1] < 1) == (t % 3 == 2)                      # the third step clips
        for n in LIVE:
            p = scaled.by_name(n)
            assert p.grad is None or not bool(p.grad.any()), n
        fed.append(live_lists(g)); coefs.append(a["stats"][1]); snaps.append(a)
    if scale == 3.0:                                                    # the premise: 3 * (1/3 rounded) is not the identity
        g = gradients(0, scale)["big"]
        assert not same_bits(g * lsr.inverse(scale), gradients(0)["big"])
    want = list(lsr.run(live_lists(scaled.p0), fed, oc.TOTAL_STEPS, scale, growth_interval=0, min_scale=min(1.0, scale), coefs=coefs,
                        **RESTATE_KW))
    for t, (wp, wm, wv, info) in enumerate(want):
        assert not info["skip"] and info["applied"] == t + 1
        assert abs(snaps[t]["stats"][0] - info["total_norm"]) <= 1e-6 * info["total_norm"]
        for k, n in enumerate(LIVE):
            assert same_bits(snaps[t]["p"][n], wp[k]) and same_bits(snaps[t]["m"][n], wm[k]) and same_bits(snaps[t]["v"][n], wv[k]), (t, n)


# ---- 2. a non-finite step is skipped -------------------------------------------------------------------------------------------
PLACES = [("big", 100), ("big", BIG - 2), ("bucket", BIG - 1), ("fc.bias", 1030)]


@pytest.mark.parametrize("value", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("name,at", PLACES, ids=["full_chunk", "tail", "view_last_element", "short_chunk"])
def test_a_non_finite_gradient_skips_the_step(hiplib, name, at, value):
    run = Run(loss_scale="dynamic", init_scale=1024.0, growth_interval=1000)
    before = run.step(gradients(0, 1024.0))
    assert before["counter"] == 1 and before["state"] == [1, 0]
    where = {n: run.by_name(n).grad.data_ptr() for n in LIVE if run.by_name(n).grad is not None}
    assert len(where) == len(LIVE) - 1 and run.by_name(oc.NO_GRAD).grad is None
    g = gradients(1, 1024.0)
    g[name] = g[name].copy()
    g[name].reshape(-1)[at] = value
    after = run.step(g)
    print(after["stats"], after["scale"], after["state"])
    assert_same_state(after, before, (name, at, value))                  # parameters, both moments, the counter
    assert same_bits(after["p"][oc.NO_GRAD], before["p"][oc.NO_GRAD])    # no decay either
    assert not same_bits(before["p"][oc.NO_GRAD], run.p0[oc.NO_GRAD])    # ... which the applied step did do
    for n, ptr in where.items():
        grad = run.by_name(n).grad
        assert grad.data_ptr() == ptr and not bool(grad.any()) and bool(torch.isfinite(grad).all()), n
    assert not bool(run.flat.any())                                      # nothing but zeros in and around the view
    assert same_bits(after["scale"], F(512.0)) and after["state"] == [0, 1]
    stats = after["stats"]
    assert not np.isfinite(stats[0]) and stats[1] == 0 and stats[6] == 1024.0 and stats[7] == 1
    assert stats[2:6] == [float(F(v)) for v in lsr.orr.one_cycle(1, oc.TOTAL_STEPS, **oc.SETTINGS)] + [1.0, 0.0]   # the row it would have used
    third = run.step(gradients(1, 512.0))                                # the next clean step is applied step 1, at the new scale
    assert third["counter"] == 2 and third["stats"][4] == 1 and third["stats"][6] == 512.0 and third["stats"][7] == 1
    assert third["state"] == [1, 1] and not same_bits(third["p"]["big"], before["p"]["big"])


def test_an_overflow_of_the_unscaled_gradient_skips_too(hiplib):
    run = Run(loss_scale=2.0 ** -3, min_scale=2.0 ** -3)
    before = run.step(gradients(0, 2.0 ** -3))
    g = gradients(1, 2.0 ** -3)
    g["fc.weight"] = g["fc.weight"].copy()
    g["fc.weight"].reshape(-1)[7] = 1e38                                # finite, but 8e38 is not
    assert np.isfinite(g["fc.weight"]).all() and not np.isfinite(lsr.unscale([g["fc.weight"]], 2.0 ** -3)[0]).all()
    after = run.step(g)
    assert_same_state(after, before, "overflow")
    assert after["stats"][0] == float("inf") and after["stats"][7] == 1 and after["state"] == [0, 1]
    assert same_bits(after["scale"], F(2.0 ** -3))                       # a static scale stays
    assert not bool(run.by_name("fc.weight").grad.any())


# ---- 3. the dynamic sequence against stock torch ------------------------------------------------------------------------------
def test_dynamic_sequence_equals_the_stock_composition(hiplib):
    """ten steps, growth_interval 3: clean x3, inf, clean x2, NaN, clean x3, against torch._amp_foreach_non_finite_check_and_unscale_
    + the plain fused step (left out when found_inf is set, as GradScaler.step does) + torch._amp_update_scale_"""
    bad = {3: float("inf"), 6: float("nan")}
    fused, stock = Run(loss_scale="dynamic", init_scale=65536.0, growth_interval=3), Run()
    scale = torch.full((1,), 65536.0, device=DEV)
    tracker = torch.zeros((1,), dtype=torch.int32, device=DEV)
    scales, fed = [], []
    for t in range(10):
        current = float(fused.opt.scale.item())
        assert current == float(scale.item())
        g = gradients(t, current)
        if t in bad:
            g["bucket"] = g["bucket"].copy()
            g["bucket"][4096 + t] = bad[t]
        a = fused.step(g)
        stock.set_grads(g)
        found = torch.zeros((1,), device=DEV)
        grads = [p.grad for p in stock.params if p.grad is not None]
        torch._amp_foreach_non_finite_check_and_unscale_(grads, found, scale.double().reciprocal().float())
        if float(found.item()) == 0:
            stock.opt.step()
        else:
            for x in grads:
                x.zero_()
        torch._amp_update_scale_(scale, tracker, found, 2.0, 0.5, 3)
        b = stock.snapshot()
        print("step %d scale %g -> %g tracker %d skipped %d" % (t, current, a["scale"], a["state"][0], a["state"][1]))
        assert same_bits(a["scale"], scale.cpu().numpy()[0]) and a["state"][0] == int(tracker.item()), t
        assert (float(found.item()) != 0) == (t in bad) and a["state"][1] == sum(1 for k in bad if k <= t)
        assert_same_state(a, b, t)
        scales.append(float(a["scale"])); fed.append(live_lists(g))
    assert scales == [65536.0, 65536.0, 131072.0, 65536.0, 65536.0, 65536.0, 32768.0, 32768.0, 32768.0, 65536.0]
    assert a["counter"] == 8 and a["stats"][7] == 2
    want = list(lsr.run(live_lists(fused.p0), fed, oc.TOTAL_STEPS, 65536.0, growth_interval=3, **RESTATE_KW))
    assert [float(w[3]["scale"]) for w in want] == scales and [w[3]["skip"] for w in want] == [t in bad for t in range(10)]
    assert want[-1][3]["applied"] == 8 and want[-1][3]["skipped"] == 2


# ---- 4. the guard ----------------------------------------------------------------------------------------------------------------
def test_a_static_scale_of_one_guards_against_a_nan_gradient(hiplib):
    guarded, plain = Run(loss_scale=1.0), Run()
    clean = gradients(0)
    first, first_plain = guarded.step(clean), plain.step(clean)
    assert_same_state(first, first_plain, "scale 1.0 is the plain step")
    g = gradients(1)
    g["conv2.weight"] = g["conv2.weight"].copy()
    g["conv2.weight"].reshape(-1)[2] = float("nan")
    after, after_plain = guarded.step(g), plain.step(g)
    assert_same_state(after, first, "guard")
    assert all(np.isfinite(after[w][n]).all() for w in ("p", "m", "v") for n in NAMES)
    assert after["stats"][7] == 1 and same_bits(after["scale"], F(1.0))
    # the premise: the plain step (a NaN norm gives coef 1) takes the NaN into the parameter and both moments, for good
    assert all(np.isnan(after_plain[w]["conv2.weight"].reshape(-1)[2]) for w in ("p", "m", "v"))
    assert after_plain["counter"] == 2 and np.isnan(after_plain["stats"][0])


# ---- 5. fp16 underflow: the reason the feature exists ---------------------------------------------------------------------------
def test_fp16_gradients_that_underflow_without_the_scale_train_with_it(hiplib, request):
    from epnet_amd import optim
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    request.addfinalizer(lambda: torch.use_deterministic_algorithms(prev))

    def stack():
        torch.manual_seed(5)
        return torch.nn.Sequential(torch.nn.Linear(24, 40), torch.nn.ReLU(), torch.nn.Linear(40, 8)).to(DEV)

    def loss_of(model, x):
        with torch.autocast("cuda", torch.float16):
            out = model(x)
        assert out.dtype == torch.float16
        # d loss / d out = 2e-8 rounds to zero in float16 (below half its smallest subnormal, 2^-25 = 3e-8); times 65536 it is
        # 1.3e-3, and everything behind it stays a normal float16 number
        return out.float().sum() * 2e-8
    gen = torch.Generator().manual_seed(6)
    xs = [torch.randn((16, 24), generator=gen).to(DEV) for _ in range(3)]
    unscaled = stack()
    loss_of(unscaled, xs[0]).backward()
    assert all(p.grad is not None and not bool(p.grad.any()) for p in unscaled.parameters())      # every gradient exactly zero
    fused, stock = stack(), stack()
    opt_f = optim.FusedAdamOneCycle(fused, oc.TOTAL_STEPS, loss_scale=65536.0, **oc.SETTINGS)
    opt_s = optim.FusedAdamOneCycle(stock, oc.TOTAL_STEPS, **oc.SETTINGS)
    for k, x in enumerate(xs):
        opt_f.scale_loss(loss_of(fused, x)).backward()
        assert all(bool(p.grad.any()) and p.grad.dtype == torch.float32 for p in fused.parameters()), k
        opt_f.step()
        (loss_of(stock, x) * 65536.0).backward()
        for p in stock.parameters():
            p.grad.div_(65536.0)
        opt_s.step()
    torch.cuda.synchronize()
    assert int(opt_f.counter[0]) == 3 and opt_f.stats.tolist()[6:] == [65536.0, 0.0]
    assert opt_f.stats.tolist()[:6] == opt_s.stats.tolist()[:6]
    start = stack()
    for (n, p), q, p0 in zip(fused.named_parameters(), stock.parameters(), start.parameters()):
        assert torch.equal(p, q) and not torch.equal(p, p0), n
    assert torch.equal(opt_f.exp_avg, opt_s.exp_avg) and torch.equal(opt_f.exp_avg_sq, opt_s.exp_avg_sq) and bool(opt_f.exp_avg_sq.any())


# ---- 6. forward, scale_loss, backward and step() from one graph ---------------------------------------------------------------
def test_scaled_training_step_replays_from_one_graph_and_skips_in_it(hiplib, monkeypatch, request):
    """the pattern of test_forward_backward_and_step_replay_from_one_graph (tests/test_optim_gpu.py) with a dynamic scale:
    one eager step, one capture, then a clean batch (the scale grows: growth_interval 2), one holding an infinity (skipped, the
    scale backs off) and a clean one, each replay against the eager run of the same batches"""
    from epnet_amd import optim
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    request.addfinalizer(lambda: torch.use_deterministic_algorithms(prev))
    pair = []
    for _ in range(2):
        torch.manual_seed(3)
        model = oc.build_model().to(DEV)
        pair.append((model, optim.FusedAdamOneCycle(model, oc.TOTAL_STEPS, loss_scale="dynamic", init_scale=1024.0, growth_interval=2,
                                                    **oc.SETTINGS)))
    (model_e, opt_e), (model_g, opt_g) = pair
    gen = torch.Generator().manual_seed(11)
    batches = [torch.randn((4, 5, 33), generator=gen).to(DEV) for _ in range(4)]
    batches[2][1, 2, 7] = float("inf")
    static = torch.empty_like(batches[0])

    def train_step(model, opt, x):
        y = model.bn2(model.conv2(torch.relu(model.bn1(model.conv1(x)))))      # (4, 3, 33)
        z = model.fc(y.mean(dim=(1, 2)).view(-1, 1))                           # (4, 1031)
        loss = (z * z).mean() + y.abs().mean() * 30
        opt.scale_loss(loss).backward()
        opt.step()

    def state(model, opt):
        torch.cuda.synchronize()
        return ([p.detach().clone() for p in model.parameters()], opt.exp_avg.clone(), opt.exp_avg_sq.clone(), int(opt.counter[0]),
                float(opt.scale.item()), opt.scaler_state.tolist(), opt.stats.tolist())
    eager = []
    for x in batches:
        train_step(model_e, opt_e, x)
        eager.append(state(model_e, opt_e))
    assert [e[3] for e in eager] == [1, 2, 2, 3] and [e[4] for e in eager] == [1024.0, 2048.0, 1024.0, 1024.0]
    assert [e[5] for e in eager] == [[1, 0], [0, 0], [0, 1], [1, 1]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        static.copy_(batches[0])
        train_step(model_g, opt_g, static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        train_step(model_g, opt_g, static)
    replayed = []
    for k in (1, 2, 3):
        static.copy_(batches[k])
        graph.replay()
        got, want = state(model_g, opt_g), eager[k]
        print("replay %d counter %d scale %g state %s norm %r" % (k, got[3], got[4], got[5], got[6][0]))
        for (n, _), p, q in zip(model_g.named_parameters(), got[0], want[0]):
            assert torch.equal(p, q), (k, n)
        assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), k
        assert got[3:6] == want[3:6], (k, got[3:6], want[3:6])
        assert got[6][1:] == want[6][1:] and (got[6][0] == want[6][0] or (np.isnan(got[6][0]) and np.isnan(want[6][0]))), k
        replayed.append(got)
    for p, q in zip(replayed[1][0], replayed[0][0]):                           # the skipped replay left the first one's bits
        assert torch.equal(p, q)
    assert not all(torch.equal(p, q) for p, q in zip(replayed[2][0], replayed[1][0]))
    assert all(bool(torch.isfinite(p).all()) for p in model_g.parameters())
    assert all(not bool(p.grad.any()) for p in model_g.parameters() if p.grad is not None)


# ---- 7. the workspace comes from the guarded allocator -----------------------------------------------------------------------------
def test_the_workspace_is_allocated_where_the_canaries_are(hiplib, monkeypatch):
    """tests/conftest.py has replaced pointnet2_utils._new by its canary allocator for this test; the scaled step's workspace
    (64 + 8 bytes per chunk, the plain step's size) must be asked of it, so that a write past it fails the test it happens in"""
    from epnet_amd import pointnet2_utils
    guarded, asked = pointnet2_utils._new, []

    def recording(like, shape, dtype=torch.float32, zero=False):
        asked.append((tuple(shape), dtype))
        return guarded(like, shape, dtype, zero)
    monkeypatch.setattr(pointnet2_utils, "_new", recording)
    run = Run(loss_scale="dynamic")
    run.step(gradients(0, 65536.0))
    chunks = sum(-(-a.size // 4096) for n, a in run.p0.items() if n in LIVE)
    assert ((64 + 8 * chunks,), torch.uint8) in asked, asked
    assert hiplib.epnet_adam_onecycle_workspace_bytes(chunks) == 64 + 8 * chunks

"""Loss scaling of the fused optimiser without a GPU: the scale's rule as tests/loss_scale_restate.py states it against stock
``torch._amp_update_scale_`` on CPU tensors (this torch has it there; the ``min_scale`` floor, which torch lacks, against values
worked out by hand), and the Python surface of ``FusedAdamOneCycle(loss_scale=...)``. The kernels' side is
tests/test_loss_scale_gpu.py."""
import numpy as np
import pytest
import torch

import loss_scale_restate as lsr
import optim_cases as oc

F = np.float32


def stock_sequence(init_scale, found, growth_factor, backoff_factor, growth_interval):
    scale, tracker = torch.tensor([init_scale], dtype=torch.float32), torch.zeros((1,), dtype=torch.int32)
    out = []
    for f in found:
        torch._amp_update_scale_(scale, tracker, torch.tensor([float(f)]), growth_factor, backoff_factor, growth_interval)
        out.append((scale.numpy()[0].copy(), int(tracker[0])))
    return out


def restated_sequence(init_scale, found, growth_factor, backoff_factor, growth_interval, min_scale=1e-30):
    scale, tracker, out = F(init_scale), 0, []
    for f in found:
        scale, tracker = lsr.update_scale(scale, tracker, bool(f), growth_factor, backoff_factor, growth_interval, min_scale)
        out.append((scale, tracker))
    return out


def same(a, b):
    return len(a) == len(b) and all(F(x[0]).tobytes() == F(y[0]).tobytes() and x[1] == y[1] for x, y in zip(a, b))


@pytest.mark.parametrize("init,found,gf,bf,interval", [
    (65536.0, [0, 0, 0, 0, 0, 0, 0], 2.0, 0.5, 3),                 # growth after exactly three clean steps, twice
    (65536.0, [0, 0, 1, 0, 0, 0, 0, 1, 1, 0], 2.0, 0.5, 3),        # a back-off resets the tracker
    (2.0 ** 127, [0, 0, 0], 2.0, 0.5, 1),                          # growth refused: the product is not finite
    (1000.0, [0, 1, 0, 0, 1, 0, 0, 0, 0, 1], 1.7, 0.3, 2),         # factors that are no float32 numbers: one rounding, from double
    (3.0, [1, 0, 0, 0, 0, 0, 1, 0], 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30, 1),
])
def test_scale_sequence_equals_stock_torch(init, found, gf, bf, interval):
    got, want = restated_sequence(init, found, gf, bf, interval), stock_sequence(init, found, gf, bf, interval)
    print(got, want)
    assert same(got, want)


def test_growth_happens_at_the_interval_and_not_before():
    seq = restated_sequence(4.0, [0] * 7, 2.0, 0.5, 3)
    assert [(float(s), t) for s, t in seq] == [(4, 1), (4, 2), (8, 0), (8, 1), (8, 2), (16, 0), (16, 1)]
    seq = restated_sequence(4.0, [0, 0, 1, 0, 0, 0], 2.0, 0.5, 3)
    assert [(float(s), t) for s, t in seq] == [(4, 1), (4, 2), (2, 0), (2, 1), (2, 2), (4, 0)]


def test_growth_is_refused_when_the_product_is_not_finite():
    """through run(), on zero gradients: a clean step each time, the scale stays 2^127 and the tracker returns to 0"""
    p = [np.ones(5, F)]
    steps = list(lsr.run(p, [[np.zeros(5, F)]] * 3, oc.TOTAL_STEPS, 2.0 ** 127, growth_interval=1, wd=oc.WD, b2=oc.BETA2, eps=oc.EPS,
                         clip=oc.CLIP, **oc.SETTINGS))
    assert [(float(s[3]["scale"]), s[3]["tracker"], s[3]["skip"]) for s in steps] == [(2.0 ** 127, 0, False)] * 3
    assert steps[-1][3]["applied"] == 3 and steps[-1][3]["skipped"] == 0


def test_min_scale_is_a_floor():
    """torch has no floor; by hand: 3 -> 1.5 -> max(0.75, 1) = 1 -> 1, and growth starts from the floor"""
    seq = restated_sequence(3.0, [1, 1, 1, 0, 0], 2.0, 0.5, 2, min_scale=1.0)
    assert [(float(s), t) for s, t in seq] == [(1.5, 0), (1.0, 0), (1.0, 0), (1.0, 1), (2.0, 0)]


def test_a_static_scale_never_moves():
    seq = restated_sequence(3.0, [0, 0, 1, 0, 1, 1, 0], 2.0, 0.5, 0, min_scale=1.0)
    assert all(F(s).tobytes() == F(3.0).tobytes() for s, _ in seq)
    assert [t for _, t in seq] == [1, 2, 0, 1, 0, 0, 1]                 # the tracker still counts clean steps since the last skip


def test_restated_run_skips_and_counts_applied_steps():
    """an infinity, a NaN and an overflow of g * inv skip: parameters and moments are the objects they were, the schedule's row
    is the applied steps'"""
    rng = np.random.default_rng(0)
    p = [rng.standard_normal(9).astype(F)]
    g = lambda: [rng.standard_normal(9).astype(F)]                     # noqa: E731
    bad_inf, bad_nan, big = g(), g(), [np.full(9, 1e38, F)]
    bad_inf[0][3], bad_nan[0][8] = np.inf, np.nan
    steps = list(lsr.run(p, [g(), bad_inf, g(), bad_nan, big, g()], oc.TOTAL_STEPS, 2.0 ** -3, growth_interval=0, min_scale=2.0 ** -3,
                         wd=oc.WD, b2=oc.BETA2, eps=oc.EPS, clip=oc.CLIP, **oc.SETTINGS))
    assert [s[3]["skip"] for s in steps] == [False, True, False, True, True, False]
    assert [s[3]["applied"] for s in steps] == [1, 1, 2, 2, 2, 3] and [s[3]["skipped"] for s in steps] == [0, 1, 1, 2, 3, 3]
    assert steps[1][0][0] is steps[0][0][0] and steps[4][1][0] is steps[2][1][0]
    assert [s[3]["step"] for s in steps if not s[3]["skip"]] == [0, 1, 2]


# ---- the Python surface (CPU parameters: nothing is launched) -------------------------------------------------------------------
def make(**kw):
    from epnet_amd import optim
    torch.manual_seed(0)
    model = oc.build_model()
    return model, optim.FusedAdamOneCycle(model, oc.TOTAL_STEPS, **kw)


def test_scale_loss_needs_a_scale_and_is_one_differentiable_multiply():
    _, opt = make()
    assert opt.scale is None
    with pytest.raises(RuntimeError, match="loss_scale=None"):
        opt.scale_loss(torch.ones(()))
    with pytest.raises(RuntimeError, match="loss_scale=None"):
        opt.scaler_state_dict()
    with pytest.raises(RuntimeError, match="loss_scale=None"):
        opt.load_scaler_state_dict({"scale": 2.0})
    _, opt = make(loss_scale="dynamic")
    assert opt.scale.dtype == torch.float32 and opt.scale.shape == (1,) and float(opt.scale) == 65536.0 and opt.growth_interval == 2000
    x = torch.tensor(0.5, requires_grad=True)
    opt.scale_loss(x * 3).backward()
    assert float(x.grad) == 3 * 65536.0
    _, opt = make(loss_scale=1.0)
    assert float(opt.scale) == 1.0 and opt.growth_interval == 0


@pytest.mark.parametrize("kw,match", [
    (dict(loss_scale="dynamic", growth_factor=0.5), "growth_factor"),
    (dict(loss_scale="dynamic", growth_factor=-2.0), "growth_factor"),
    (dict(loss_scale="dynamic", backoff_factor=1.5), "backoff_factor"),
    (dict(loss_scale="dynamic", backoff_factor=0.0), "backoff_factor"),
    (dict(loss_scale="dynamic", min_scale=0.0), "min_scale"),
    (dict(loss_scale="dynamic", min_scale=float("nan")), "min_scale"),
    (dict(loss_scale="dynamic", init_scale=0.5), "below min_scale"),
    (dict(loss_scale="dynamic", init_scale=float("inf")), "scale"),
    (dict(loss_scale="dynamic", growth_interval=0), "growth_interval"),
    (dict(loss_scale=0.0), "scale"),
    (dict(loss_scale=-1.0), "scale"),
    (dict(loss_scale="static"), "dynamic"),
])
def test_validation_errors_fire(kw, match):
    with pytest.raises(ValueError, match=match):
        make(**kw)


def test_scaler_state_dict_round_trips_and_reads_a_gradscaler_state():
    _, a = make(loss_scale="dynamic", growth_interval=7)
    sd = a.scaler_state_dict()
    assert sd == {"scale": 65536.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 7, "_growth_tracker": 0, "skipped": 0}
    assert set(torch.amp.GradScaler("cpu").state_dict()) <= set(sd)
    a.scale.fill_(512.0)
    a.scaler_state.copy_(torch.tensor([5, 3]))
    sd = a.scaler_state_dict()
    assert (sd["scale"], sd["_growth_tracker"], sd["skipped"]) == (512.0, 5, 3)
    _, b = make(loss_scale="dynamic", growth_interval=7)
    where = b.scale.data_ptr()
    b.load_scaler_state_dict(sd)
    assert b.scaler_state_dict() == sd and b.scale.data_ptr() == where       # in place: a captured graph keeps reading it
    b.load_scaler_state_dict({"scale": 1024.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000, "_growth_tracker": 11})
    got = b.scaler_state_dict()
    assert (got["scale"], got["_growth_tracker"], got["skipped"], got["growth_interval"]) == (1024.0, 11, 0, 7)
    with pytest.raises(ValueError):
        b.load_scaler_state_dict({"scale": 0.0})


def test_state_dict_keeps_its_format():
    _, plain = make()
    _, scaled = make(loss_scale="dynamic")
    a, b = plain.state_dict(), scaled.state_dict()
    assert sorted(a) == sorted(b) == ["param_groups", "state"] and a["state"] == b["state"] == {}
    assert [sorted(g) for g in a["param_groups"]] == [sorted(g) for g in b["param_groups"]]
    assert a["param_groups"] == b["param_groups"]
    scaled.load_state_dict(a)                                                # and reads the plain one's


def test_without_a_scale_the_scaled_binding_is_never_called(hiplib, monkeypatch):
    """loss_scale=None is today's call, argument for argument; a scale routes to the new binding with the optimiser's tensors"""
    from epnet_amd import optim_cuda
    calls = []
    monkeypatch.setattr(optim_cuda, "adam_onecycle_step_gpu", lambda *a, **k: calls.append(("plain", a, k)))
    monkeypatch.setattr(optim_cuda, "adam_onecycle_step_scaled_gpu", lambda *a, **k: calls.append(("scaled", a, k)))
    for kw, want, nargs in ((dict(), "plain", 13), (dict(loss_scale=1.0), "scaled", 19), (dict(loss_scale="dynamic"), "scaled", 19)):
        del calls[:]
        model, opt = make(**kw)
        for p in model.parameters():
            p.grad = torch.ones_like(p)
        opt.step()
        opt.step()
        assert [c[0] for c in calls] == [want, want], (kw, [c[0] for c in calls])
        args = calls[0][1]
        assert len(args) == nargs and not calls[0][2]
        assert args[3] is opt.rows and args[8] is opt.counter and args[11] is opt.stats and args[-1].dtype == torch.uint8
        if want == "scaled":
            assert args[12] is opt.scale and args[13] is opt.scaler_state
            assert args[14:18] == (2.0, 0.5, 0 if kw["loss_scale"] == 1.0 else 2000, 1.0)


def test_binding_table_declares_the_scaled_entry_next_to_the_plain_one():
    from epnet_amd import _lib, optim_cuda
    plain, scaled = _lib.SIGNATURES["epnet_adam_onecycle_step"], _lib.SIGNATURES["epnet_adam_onecycle_step_scaled"]
    assert scaled[0] is plain[0] and scaled[1][:15] == plain[1][:15] and scaled[1][-3:] == plain[1][-3:] and len(scaled[1]) == len(plain[1]) + 6
    assert optim_cuda.STATS_NAMES == ("total_norm", "coef", "lr", "mom", "step", "past_end")
    assert optim_cuda.SCALED_STATS_NAMES == ("scale", "skipped") and len(optim_cuda.STATS_NAMES + optim_cuda.SCALED_STATS_NAMES) == optim_cuda.STATS


def test_scaled_entry_validates_its_arguments_without_a_gpu(hiplib):
    import ctypes as C
    fake = C.c_void_p(4096)   # never dereferenced: the call returns before anything touches the device

    def call(gf=2.0, bf=0.5, interval=2000, min_scale=1.0, scale=fake, state=fake, tensors=3, chunks=5, ws=fake, ws_bytes=64 + 8 * 5):
        return hiplib.epnet_adam_onecycle_step_scaled(tensors, chunks, 4096, fake, fake, fake, 10, 1.0, 1e-8, 0.99, 1, fake, fake, fake, fake,
                                                      scale, state, gf, bf, interval, min_scale, ws, ws_bytes, None)
    einval, enomem = -1, -3
    for kw in (dict(gf=0.5), dict(gf=float("nan")), dict(gf=float("inf")), dict(bf=0.0), dict(bf=1.5), dict(bf=float("nan")), dict(interval=-1),
               dict(min_scale=0.0), dict(min_scale=-1.0), dict(min_scale=float("nan")), dict(min_scale=1e-60), dict(scale=None), dict(state=None)):
        assert call(**kw) == einval, kw
    assert call(ws=None) == enomem and call(ws_bytes=64 + 8 * 5 - 1) == enomem
    assert call(tensors=0, scale=None) == 0 and call(chunks=0) == 0           # nothing to do, nothing written

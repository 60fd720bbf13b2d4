"""The fused optimiser without a GPU: the schedule and the numpy restatement (tests/optim_restate.py) against the reference's own
run stored in tests/golden/optim.npz, the state dict's layout, the C ABI's argument checks and the refusal of host tensors.

Bound of a float32 evaluation against the reference's float64 run, per step: max(2 x the error of the reference's own float32
run at that step, 2^-23 x max |p|). The two float32 paths differ only in rounding order (torch's lerp_ / addcmul_ / addcdiv_
against the header's source order), so neither can be expected to be closer to float64 than the other; a wrong formula -- eps
inside the bias correction, decay after the update, an unclipped gradient, the wrong row -- is off by the size of an update,
three orders above (the fixture's `upd`)."""
import ctypes

import numpy as np
import pytest

import optim_cases as oc
import optim_restate as orr

FX = oc.load()


def bound(t):
    return max(2 * float(FX["err32"][t]), 2.0 ** -23 * float(np.abs(FX["p64"][t]).max()))


def fixture_grads(t):
    by_name = oc.split(FX["grads"][t], oc.GRAD_NAMES)
    return [by_name.get(n) for n in oc.NAMES]


def trainable(names=oc.NAMES):
    return [n for n in names if n != oc.FROZEN]


def test_one_cycle_table_equals_the_reference_schedule():
    from epnet_amd import optim
    lr, mom = optim.one_cycle_table(oc.TOTAL_STEPS, **oc.SETTINGS)
    assert lr.dtype == np.float64 and mom.dtype == np.float64 and len(lr) == oc.TOTAL_STEPS
    border = int(oc.TOTAL_STEPS * oc.SETTINGS["pct_start"])
    for t in (0, border - 1, border, oc.TOTAL_STEPS - 1):
        print("step %2d lr %.17g mom %.17g" % (t, lr[t], mom[t]))
    assert np.array_equal(lr, FX["schedule_lr"]) and np.array_equal(mom, FX["schedule_mom"])       # exactly, border and last step too
    assert np.array_equal(lr[:oc.STEPS], FX["lr"]) and np.array_equal(mom[:oc.STEPS], FX["mom"])  # what the training loop saw
    assert lr[border] == pytest.approx(oc.SETTINGS["lr_max"], rel=1e-15) and mom[border] == pytest.approx(oc.SETTINGS["moms"][1], rel=1e-15)
    for t in range(oc.TOTAL_STEPS):
        assert orr.one_cycle(t, oc.TOTAL_STEPS, **oc.SETTINGS) == (lr[t], mom[t])
    with pytest.raises(ValueError):
        optim.one_cycle_table(2, pct_start=0.4)     # the first phase would have no step: the reference divides by zero


def test_row_table_is_the_restatement_rows():
    from epnet_amd import optim
    lr, mom = optim.one_cycle_table(oc.TOTAL_STEPS, **oc.SETTINGS)
    rows = optim.schedule_rows(lr, mom, oc.WD, oc.BETA2)
    assert rows.dtype == np.float32 and rows.shape == (oc.TOTAL_STEPS, 8)
    for t in range(oc.TOTAL_STEPS):
        r = orr.row(t, lr[t], mom[t], oc.WD, oc.BETA2)
        want = [r[k] for k in ("decay", "b1", "omb1", "step_size", "bc2_sqrt", "lr", "mom")] + [np.float32(0)]
        assert rows[t].tolist() == [float(x) for x in want], t


def test_restatement_within_twice_the_reference_float32_error():
    names = trainable()
    p0 = oc.split(FX["p0"])
    grads = [[g for n, g in zip(oc.NAMES, fixture_grads(t)) if n != oc.FROZEN] for t in range(oc.STEPS)]
    failures = []
    steps = orr.run([p0[n] for n in names], grads, oc.TOTAL_STEPS, wd=oc.WD, b2=oc.BETA2, eps=oc.EPS, clip=oc.CLIP, **oc.SETTINGS)
    for t, (p, m, v, info) in enumerate(steps):
        got = dict(zip(names, p))
        got[oc.FROZEN] = p0[oc.FROZEN]
        err = float(np.abs(oc.join(got).astype(np.float64) - FX["p64"][t]).max())
        rel = abs(info["total_norm"] - float(FX["total_norm"][t])) / float(FX["total_norm"][t])
        print("step %2d coef %.6e err %.3e reference float32 err %.3e ratio %.2f bound %.3e update %.2e norm rel %.1e"
              % (t, info["coef"], err, FX["err32"][t], err / FX["err32"][t], bound(t), FX["upd"][t], rel))
        assert info["lr"] == FX["lr"][t] and info["mom"] == FX["mom"][t]
        assert rel < 1e-12
        assert (info["coef"] < 1) == (t % 3 == 2)
        if not err <= bound(t):
            failures.append((t, err, bound(t)))
    assert not failures, failures
    # the parameter without a gradient only decayed; the frozen one never moved in the reference either
    decay = np.prod([1 - oc.WD * l for l in FX["lr"]])
    assert np.allclose(got[oc.NO_GRAD], p0[oc.NO_GRAD] * decay, rtol=1e-6, atol=0)
    assert np.array_equal(oc.split(FX["p32"][-1])[oc.FROZEN], p0[oc.FROZEN])


def test_the_fixture_is_what_its_generator_says():
    assert FX["grads"].shape == (oc.STEPS, sum(oc.numel(n) for n in oc.GRAD_NAMES)) and FX["p64"].dtype == np.float64
    norms = np.sqrt((FX["grads"].astype(np.float64) ** 2).sum(axis=1))
    assert all((300 < n < 600) if t % 3 == 2 else (0.3 < n < 0.6) for t, n in enumerate(norms)), norms
    assert (FX["err32"] > 0).all() and (FX["err32"] < 1e-6).all() and (FX["upd"] > 100 * FX["err32"]).all()


def _optimizer(model=None):
    from epnet_amd import optim
    model = model or oc.build_model()
    opt = optim.FusedAdamOneCycle(model, oc.TOTAL_STEPS, wd=oc.WD, beta2=oc.BETA2, eps=oc.EPS, grad_norm_clip=oc.CLIP, **oc.SETTINGS)
    dict(model.named_parameters())[oc.FROZEN].requires_grad = False
    return model, opt


def test_state_dict_layout_is_the_reference_wrappers():
    import torch
    model, opt = _optimizer()
    name_of = {id(p): n for n, p in model.named_parameters()}
    assert [name_of[id(p)] for p in opt.params] == FX["order"].tolist()
    sd = opt.state_dict()
    assert [len(g["params"]) for g in sd["param_groups"]] == FX["groups"].tolist()
    assert [k for g in sd["param_groups"] for k in g["params"]] == list(range(len(oc.NAMES)))
    assert sd["state"] == {}                                         # nothing stepped yet, as a fresh torch optimiser
    stock = torch.optim.Adam([{"params": g} for g in opt.groups], betas=(0.9, oc.BETA2)).state_dict()
    assert set(stock["param_groups"][0]) - {"decoupled_weight_decay"} <= set(sd["param_groups"][0])
    # a reference checkpoint's optimizer_state: the fixture's moments of the float32 run after STEPS steps
    ref_state, at = {}, 0
    for k, n in enumerate(FX["order"].tolist()):
        if FX["has_state"][k]:
            size = oc.numel(n)
            ref_state[k] = {"step": torch.tensor(float(FX["step"])), "exp_avg": torch.from_numpy(FX["m32"][at:at + size].reshape(oc.SHAPES[n])),
                            "exp_avg_sq": torch.from_numpy(FX["v32"][at:at + size].reshape(oc.SHAPES[n]))}
            at += size
    opt.load_state_dict({"state": ref_state, "param_groups": stock["param_groups"]})
    assert int(opt.counter[0]) == int(FX["step"])
    back = opt.state_dict()
    assert sorted(back["state"]) == sorted(ref_state)
    for k, s in ref_state.items():                                   # the round trip is exact
        assert torch.equal(back["state"][k]["exp_avg"], s["exp_avg"]) and torch.equal(back["state"][k]["exp_avg_sq"], s["exp_avg_sq"])
        assert float(back["state"][k]["step"]) == float(FX["step"]) and back["state"][k]["exp_avg"].shape == s["exp_avg"].shape
    assert back["param_groups"][0]["lr"] == FX["lr"][oc.STEPS - 1] and back["param_groups"][0]["betas"] == (FX["mom"][oc.STEPS - 1], oc.BETA2)
    _, other = _optimizer()
    other.load_state_dict(back)
    again = other.state_dict()
    assert all(torch.equal(again["state"][k]["exp_avg_sq"], back["state"][k]["exp_avg_sq"]) for k in back["state"])
    with pytest.raises(ValueError):
        other.load_state_dict({"state": {}, "param_groups": [{"params": [0, 1]}, {"params": []}]})


def test_parameter_lists_go_to_group_zero():
    from epnet_amd import optim
    model = oc.build_model()
    opt = optim.FusedAdamOneCycle(model.parameters(), oc.TOTAL_STEPS)
    assert len(opt.groups[0]) == len(oc.NAMES) and opt.groups[1] == []
    with pytest.raises(ValueError):
        optim.FusedAdamOneCycle([], oc.TOTAL_STEPS)


# ---- the C ABI without a device ------------------------------------------------------------------------------------------
def _call(hiplib, tensors=3, chunks=5, max_numel=4096, ptr=4096, ws=4096, ws_bytes=1 << 20, total_steps=40, clip=1.0, eps=1e-8, b2=0.99,
          stats=4096):
    fake = ctypes.c_void_p(ptr) if ptr else None      # never dereferenced: every refusal comes before a launch
    return hiplib.epnet_adam_onecycle_step(tensors, chunks, max_numel, fake, fake, fake, total_steps, clip, eps, b2, 1, fake, fake, fake,
                                           ctypes.c_void_p(stats) if stats else None, ctypes.c_void_p(ws) if ws else None, ws_bytes, None)


def test_abi_refusals_without_a_device(hiplib):
    einval, enomem, elimit = -1, -3, -4
    assert _call(hiplib, tensors=0) == 0 and _call(hiplib, chunks=0) == 0            # zero tensors: nothing to do, nothing written
    assert _call(hiplib, tensors=0, chunks=0, ptr=0, ws=0, ws_bytes=0, stats=0) == 0
    assert _call(hiplib, tensors=-1) == einval and _call(hiplib, chunks=-1) == einval
    assert _call(hiplib, ptr=0) == einval and _call(hiplib, stats=0) == einval
    assert _call(hiplib, total_steps=0) == einval
    assert _call(hiplib, clip=0.0) == einval and _call(hiplib, clip=float("nan")) == einval
    assert _call(hiplib, eps=-1.0) == einval and _call(hiplib, b2=1.0) == einval
    assert _call(hiplib, max_numel=2 ** 31) == elimit and _call(hiplib, max_numel=2 ** 31 - 1, ws=0) == enomem
    assert _call(hiplib, chunks=2 ** 31) == elimit
    assert _call(hiplib, ws=0) == enomem and _call(hiplib, ws_bytes=64 + 5 * 8 - 1) == enomem
    assert _call(hiplib, ws=4104) == einval                                          # 16-byte alignment


def test_abi_workspace_formula(hiplib):
    """pinned: a caller that sized its scratch by the header's formula must not get EPNET_ENOMEM from a later library"""
    for chunks in (1, 2, 3996, 2 ** 31 - 1):
        assert hiplib.epnet_adam_onecycle_workspace_bytes(chunks) == 64 + 8 * chunks
    assert hiplib.epnet_adam_onecycle_workspace_bytes(0) == 0 and hiplib.epnet_adam_onecycle_workspace_bytes(-3) == 0


def test_host_tensors_are_refused(hiplib):
    import torch
    model, opt = _optimizer()
    for n, p in model.named_parameters():
        if n not in (oc.FROZEN, oc.NO_GRAD):
            p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in model.parameters()]
    with pytest.raises(RuntimeError, match="CUDAtensor"):
        opt.step()
    assert all(torch.equal(a, b) for a, b in zip(before, model.parameters()))

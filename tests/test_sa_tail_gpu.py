"""The fused SA tail on the device (include/epnet_ops.h: epnet_sa_tail_f32).

The kernel against tests/sa_tail_restate.py BIT FOR BIT (-0 == +0, NaN == NaN): one float32 fmaf chain over k ascending, the window
maximum, + bias, relu. Module level: the mean absolute error against the float64 module at most 1.5 x the stock float32
module's own (the margin of tests/test_image_head16_gpu.py); sampling outputs identical. Graph replay and offset pointers: bits."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import offset_alloc as oa
import sa_tail_restate as rs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

KS = [1, 2, 3, 16, 31, 32, 33, 96, 196, 384]
CS = [1, 31, 32, 33, 64, 130, 512]
SS = [1, 2, 16, 32, 64, 128]
PS = [1, 2, 31, 33, 64]
BS = [1, 3]
BUDGET = 2_000_000          # multiply-adds per case: the restatement stays fast


def _sweep():
    """a seeded mix of the lists above (not their product): every value of every list, both flags both ways, and every case
    within the budget (the largest (P, S, B) drawn that fits; K x C alone is at most 384 x 512 < BUDGET / 10)"""
    rng = np.random.default_rng(20240)
    cases = []
    for i in range(56):
        k, c = KS[i % len(KS)], CS[(i // 2 + i) % len(CS)]
        for _ in range(64):
            s, p, b = (int(rng.choice(v)) for v in (SS, PS, BS))
            if b * k * c * p * s <= BUDGET:
                break
        else:
            s, p, b = 1, 1, 1
        cases.append((k, c, s, p, b, bool(i & 1), bool(i & 2)))
    for values, col in ((KS, 0), (CS, 1), (SS, 2), (PS, 3), (BS, 4)):
        assert {case[col] for case in cases} == set(values), (col, values)
    assert {case[5:] for case in cases} == {(False, False), (False, True), (True, False), (True, True)}
    return cases


def _run(x, w, b, s_in, t_in, relu_in):
    from epnet_amd import pointnet2_utils as p2u
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    packed = p2u.SATail(t(w), t(b), t(s_in), t(t_in), relu_in, 0, None)
    y = p2u.sa_tail(t(x), packed)
    assert y.dtype == torch.float32 and tuple(y.shape) == (x.shape[0], w.shape[0], x.shape[2]) and not y.requires_grad
    return y.cpu().numpy()


def _check_bits(got, want, what):
    if not rs.bits_equal(got, want):
        bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
        first = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError("%s: %d of %d outputs differ from the fmaf chain, first at %s: %r against %r"
                             % (what, int(bad.sum()), bad.size, first, got[first], want[first]))


@pytest.mark.parametrize("k,c,s,p,b,affine,relu_in", _sweep())
def test_sweep_bit_for_bit(hiplib, k, c, s, p, b, affine, relu_in):
    rng = np.random.default_rng(k * 1000 + c * 10 + s + p)
    x, w, bias, s_in, t_in = rs.random_case(rng, b, k, c, p, s, affine)
    want = rs.restate(x, w, bias, s_in, t_in, relu_in)
    _check_bits(_run(x, w, bias, s_in, t_in, relu_in), want, "sweep")


def _model_triples():
    """(K, C, S, batch norm) of every level and scale of the RPN backbone and of the RCNN stage's SA stack"""
    import bench_step
    from epnet_amd import rpn_backbone
    cfg = rpn_backbone.BackboneConfig()
    triples = [(m[-2], m[-1], ns, True) for mlps, nss in zip(cfg.mlps, cfg.nsample) for m, ns in zip(mlps, nss)]
    for level, (m, ns) in enumerate(zip(bench_step.RCNN_MLPS, bench_step.RCNN_NSAMPLE)):
        group_all = bench_step.RCNN_NPOINTS[level] is None       # one window over the points of the level before
        triples.append((m[-2], m[-1], bench_step.RCNN_NPOINTS[level - 1] if group_all else ns, False))
    return sorted(set(triples))


@pytest.mark.parametrize("k,c,s,bn", _model_triples())
def test_model_shapes_bit_for_bit(hiplib, k, c, s, bn):
    """P <= 64, as many centres as 6 M multiply-adds allow (level 4: 384 x 512 x 32 per centre)"""
    p = max(1, min(64, 6_000_000 // (k * c * s)))
    rng = np.random.default_rng(k + c + s)
    x, w, bias, s_in, t_in = rs.random_case(rng, 1, k, c, p, s, bn)
    _check_bits(_run(x, w, bias, s_in, t_in, True), rs.restate(x, w, bias, s_in, t_in, True), "model shape P=%d" % p)


def test_no_bias_is_a_zero_bias(hiplib):
    rng = np.random.default_rng(3)
    x, w, _, _, _ = rs.random_case(rng, 2, 5, 7, 9, 4, False)
    _check_bits(_run(x, w, None, None, None, False), rs.restate(x, w, None), "no bias")


@pytest.mark.parametrize("k,c,s", [(3, 33, 16), (33, 5, 32), (1, 2, 1), (31, 64, 64), (5, 3, 4)])
def test_special_values_stay_in_their_window(hiplib, k, c, s):
    """+inf, -inf and NaN in one window each, in the LAST k (odd K: beside the zero padding of the MFMA's k-step) and in the last
    column of the window: +inf and NaN make exactly their own outputs non-finite, -inf loses the maximum; padding leaks nothing"""
    rng = np.random.default_rng(k + s)
    p = 7
    x, w, bias, _, _ = rs.random_case(rng, 2, k, c, p, s, False)
    w = np.abs(w) + np.float32(0.01)
    x[1, k - 1, 1, s - 1] = np.inf
    x[0, k - 1, 3, 0] = np.nan
    x[1, k - 1, 6, s - 1] = -np.inf
    got = _run(x, w, bias, None, None, False)
    _check_bits(got, rs.restate(x, w, bias), "special values")
    finite = np.isfinite(got)
    assert np.isposinf(got[1, :, 1]).all() and np.isnan(got[0, :, 3]).all()
    finite[1, :, 1] = finite[0, :, 3] = True
    assert finite.all()
    if s == 1:
        assert (got[1, :, 6] == 0).all()               # the window IS the -inf element
    # an infinite input scale: 0 * inf must not come out of the padding either (x' = fmaf(x, inf, 0) is +-inf or NaN everywhere)
    s_in, t_in = np.ones(k, np.float32), np.zeros(k, np.float32)
    s_in[k - 1] = np.inf
    x2 = np.abs(rs.random_case(rng, 1, k, c, p, s, False)[0]) + np.float32(1)
    got = _run(x2, w, bias, s_in, t_in, True)
    _check_bits(got, rs.restate(x2, w, bias, s_in, t_in, True), "infinite scale")
    assert np.isposinf(got).all()


def test_all_negative_windows_give_zero(hiplib):
    rng = np.random.default_rng(8)
    x, w, bias, _, _ = rs.random_case(rng, 2, 33, 40, 33, 16, False)
    x, w, bias = -np.abs(x) - np.float32(0.5), np.abs(w), -np.abs(bias)
    got = _run(x, w, bias, None, None, False)
    assert (got == 0).all() and rs.bits_equal(got, rs.restate(x, w, bias))


def test_unsupported_window_sizes_are_refused(hiplib):
    from epnet_amd import _lib, pointnet2_utils as p2u
    for s in (3, 48, 5, 24):
        x = torch.zeros((1, 4, 2, s), device=DEV)
        packed = p2u.SATail(torch.zeros((3, 4), device=DEV), torch.zeros(3, device=DEV), None, None, False, 0, None)
        with pytest.raises(_lib.EpnetError, match="outside"):
            p2u.sa_tail(x, packed)


# ---- offset pointers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,c,s,p", [(33, 64, 16, 33), (96, 130, 32, 5)])
def test_offset_pointers_give_the_same_bits(hiplib, k, c, s, p):
    from epnet_amd import pointnet2_cuda as ext
    oa.forget()
    rng = np.random.default_rng(k)
    x, w, bias, s_in, t_in = rs.random_case(rng, 2, k, c, p, s, True)
    outs = []
    for skew in ((0, 0, 0), (4, 0, 0), (0, 4, 0), (0, 0, 4), (4, 4, 4), (8, 12, 4)):
        tx, tw, ty = oa.skewed(x, skew_bytes=skew[0]), oa.skewed(w, skew_bytes=skew[1]), oa.output((2, c, p), skew_bytes=skew[2])
        tb, ts, tt = (oa.skewed(v, skew_bytes=skew[0]) for v in (bias, s_in, t_in))
        ext.sa_tail_wrapper(2, k, c, p, s, tx, tw, tb, ts, tt, True, ty)
        assert oa.unwritten(ty) == 0
        outs.append(ty.cpu().numpy())
    oa.check()
    want = rs.restate(x, w, bias, s_in, t_in, True)
    for got in outs:
        _check_bits(got, want, "offset pointers")


# ---- module level -------------------------------------------------------------------------------------------------------------
def _randomise(module, seed):
    g = torch.Generator().manual_seed(seed)
    for m in module.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.3)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.weight.data.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.bias.data.copy_(torch.randn(m.num_features, generator=g) * 0.2)


def _pair(make, seed=0):
    torch.manual_seed(seed)
    stock = make(False)
    _randomise(stock, seed + 1)
    fused = make(True)
    fused.load_state_dict(stock.state_dict())
    return stock.to(DEV).eval(), fused.to(DEV).eval()


def _cloud(b, n, c, seed):
    from epnet_amd import synth
    xyz = synth.scenes("kitti", b, n, seed=seed).to(DEV)
    feats = torch.randn((b, c, n), generator=torch.Generator().manual_seed(seed + 1)).to(DEV)
    return xyz, feats


def _float64_module(module, xyz, feats, new_xyz):
    """the level in float64 stock ops on the device: the module's own centres and ball queries, the grouped tensor by indexing, a
    float64 copy of every shared MLP, the maximum"""
    import copy
    from epnet_amd import pointnet2_utils as p2u
    outs = []
    for grouper, mlp in zip(module.groupers, module.mlps):
        if isinstance(grouper, p2u.GroupAll):
            grouped = torch.cat([xyz.transpose(1, 2).unsqueeze(2), feats.unsqueeze(2)], dim=1).double()
        else:
            idx = p2u.ball_query(grouper.radius, grouper.nsample, xyz, new_xyz).long()           # (B, P, S)
            b, p, s = idx.shape
            flat = idx.reshape(b, 1, p * s)
            gx = torch.gather(xyz.double().transpose(1, 2), 2, flat.expand(b, 3, p * s)).view(b, 3, p, s)
            gx = gx - new_xyz.double().transpose(1, 2).unsqueeze(-1)
            gf = torch.gather(feats.double(), 2, flat.expand(b, feats.shape[1], p * s)).view(b, -1, p, s)
            grouped = torch.cat([gx, gf], dim=1)
        outs.append(copy.deepcopy(mlp).double()(grouped).max(dim=3)[0])
    return torch.cat(outs, dim=1)


def _count_fused_calls(monkeypatch):
    from epnet_amd import pointnet2_utils as p2u
    calls, real = [], p2u.sa_tail

    def counted(x, packed):
        calls.append(tuple(x.shape))
        return real(x, packed)
    monkeypatch.setattr(p2u, "sa_tail", counted)
    return calls


def _module_case(monkeypatch, make, xyz, feats, scales, what):
    stock, fused = _pair(make)
    calls = _count_fused_calls(monkeypatch)
    with torch.no_grad():
        x_s, f_s, i_s = stock(xyz, feats)
        assert not calls
        x_f, f_f, i_f = fused(xyz, feats)
        assert len(calls) == scales, (what, calls)
        truth = _float64_module(stock, xyz, feats, x_s)
    if x_s is None:
        assert x_f is None and i_f is None and i_s is None
    else:
        assert torch.equal(x_s, x_f) and torch.equal(i_s, i_f)
    assert f_f.shape == f_s.shape and f_f.dtype == torch.float32
    e_fused, e_stock = (f_f.double() - truth).abs().mean().item(), (f_s.double() - truth).abs().mean().item()
    print("%s: mean |error| against the float64 module: fused %.4e, stock %.4e, ratio %.3f" % (what, e_fused, e_stock, e_fused / e_stock))
    assert truth.abs().max().item() > 0.1 and e_stock > 0
    assert e_fused <= 1.5 * e_stock, (what, e_fused, e_stock)
    return stock, fused


@pytest.mark.parametrize("fold", [True, False], ids=["folded first layer", "grouped"])
def test_msg_level_against_the_float64_module(hiplib, monkeypatch, fold):
    from epnet_amd.pointnet2_modules import PointnetSAModuleMSG

    def make(fused):
        m = PointnetSAModuleMSG(npoint=128, radii=[0.8, 1.6], nsamples=[16, 32], mlps=[[6, 16, 16, 32], [6, 32, 48, 64]],
                                fused_tail=fused)
        m.fold_first_layer = fold
        return m
    xyz, feats = _cloud(2, 1024, 6, 21)
    _module_case(monkeypatch, make, xyz, feats, 2, "MSG level, " + ("folded" if fold else "grouped"))


def test_group_all_level_against_the_float64_module(hiplib, monkeypatch):
    """the RCNN stage's last level: GroupAll, P = 1, S = 32, no batch norm"""
    from epnet_amd.pointnet2_modules import PointnetSAModule
    make = lambda fused: PointnetSAModule(mlp=[24, 32, 48, 64], bn=False, fused_tail=fused)
    xyz, feats = _cloud(6, 32, 24, 31)
    _module_case(monkeypatch, make, xyz, feats, 1, "GroupAll level")


@pytest.mark.parametrize("how", ["nsample 3 and 48", "train", "grad input", "autocast"])
def test_stock_bits_where_the_fused_tail_does_not_apply(hiplib, monkeypatch, how):
    from epnet_amd.pointnet2_modules import PointnetSAModuleMSG
    ns = [3, 48] if how.startswith("nsample") else [16, 32]
    make = lambda fused: PointnetSAModuleMSG(npoint=64, radii=[0.8, 1.6], nsamples=list(ns), mlps=[[6, 16, 32], [6, 16, 32]],
                                             fused_tail=fused)
    stock, fused = _pair(make)
    calls = _count_fused_calls(monkeypatch)
    xyz, feats = _cloud(2, 512, 6, 41)
    outs = []
    for m in (stock, fused):
        if how == "train":
            outs.append(m.train()(xyz, feats))
        elif how == "grad input":
            for p in m.parameters():
                p.requires_grad_(False)
            outs.append(m(xyz, feats.clone().requires_grad_(True)))
        elif how == "autocast":
            with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
                outs.append(m(xyz, feats))
        else:
            with torch.no_grad():
                outs.append(m(xyz, feats))
    assert not calls, (how, calls)
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    if how == "grad input":
        assert outs[1][1].requires_grad


def test_frozen_parameters_with_grad_enabled_take_the_fused_tail(hiplib, monkeypatch):
    from epnet_amd.pointnet2_modules import PointnetSAModule
    make = lambda fused: PointnetSAModule(npoint=32, radius=1.0, nsample=16, mlp=[6, 16, 32], fused_tail=fused)
    stock, fused = _pair(make)
    for p in fused.parameters():
        p.requires_grad_(False)
    calls = _count_fused_calls(monkeypatch)
    xyz, feats = _cloud(1, 256, 6, 51)
    out = fused(xyz, feats)                                    # grad enabled, nothing requires it
    assert len(calls) == 1 and not out[1].requires_grad


def test_backbone_graph_replay_equals_eager(hiplib, monkeypatch):
    from epnet_amd import rpn_backbone, synth
    torch.manual_seed(0)
    net = rpn_backbone.Pointnet2MSG(sa_tail="fused", scale=8, config=rpn_backbone.BackboneConfig(li_fusion=False)).to(DEV).eval()
    _randomise(net, 5)
    calls = _count_fused_calls(monkeypatch)
    xyz = synth.scenes("kitti", 1, 2048, seed=3).to(DEV)

    def stage():
        with torch.no_grad():
            return net(xyz)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            eager = stage()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert len(calls) == 2 * 8                                 # four levels, two scales each
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = stage()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, captured)) and eager[1].abs().max() > 0
    xyz.copy_(synth.scenes("kitti", 1, 2048, seed=4).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    fresh = stage()
    assert all(torch.equal(a, b) for a, b in zip(fresh, captured)) and not torch.equal(fresh[1], eager[1])

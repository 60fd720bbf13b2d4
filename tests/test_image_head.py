"""LI-Fusion's image head at the points only, everything that needs no GPU: the fold of
``li_fusion.pack_image_head`` + the per-tap rule (tests/image_head_restate.py) against the stock dense head in float64, the
pack's cache rule, ``supports_image_head_at_points``, and the backbone's fall-back to the dense lines."""
import inspect

import numpy as np
import pytest
import torch

import image_head_cases as cases
import image_head_restate as restate


@pytest.mark.parametrize("name", ["four", "two"])
def test_fold_and_per_tap_rule_equal_the_dense_head_in_float64(name):
    """the pack is rounded to float32 once (5e-8 measured); everything else is float64 on both sides"""
    from epnet_amd import li_fusion
    cfg = cases.CONFIGS[name]
    head = cases.make_head(cfg)
    maps, xy = cases.make_maps(cfg), cases.make_xy(cfg)
    with torch.no_grad():
        want = cases.dense_head(cases.head_to(head, dtype=torch.float64), [m.double() for m in maps], xy.double()).numpy()
    packed = li_fusion.pack_image_head(*head)
    assert packed.chans == cfg["chans"] and packed.kernels == cfg["kernels"] and packed.reduce == cfg["reduce"] and packed.q == cfg["q"]
    for wd, c, r, k in zip(packed.weights, cfg["chans"], cfg["reduce"], cfg["kernels"]):
        assert tuple(wd.shape) == (k, k, c, r) and wd.dtype == torch.float32 and wd.is_contiguous()
    assert tuple(packed.wf.shape) == (cfg["q"], sum(cfg["reduce"])) and tuple(packed.shift.shape) == (cfg["q"],)
    got = restate.image_head_at_points([m.numpy() for m in maps], [v.numpy() for v in packed.weights], cfg["kernels"],
                                       packed.wf.numpy(), packed.shift.numpy(), xy.numpy(), True, np.float64)
    assert got.shape == want.shape == (cfg["b"], cfg["q"], cfg["n"])
    assert np.abs(want).max() > 0.1                      # not a comparison of zeros
    assert (want[:, :, 2:4] == 0).all() and (got[:, :, 2:4] == 0).all()      # the two points outside the map
    worst = np.abs(got - want).max()
    print("fold + rule against the float64 dense head:", worst)
    assert worst <= 1e-6
    # and the float32 restatement stays inside the project's float tolerance of the same yardstick
    got32 = restate.image_head_at_points([m.numpy() for m in maps], [v.numpy() for v in packed.weights], cfg["kernels"],
                                         packed.wf.numpy(), packed.shift.numpy(), xy.numpy(), True, np.float32)
    assert got32.dtype == np.float32
    assert (np.abs(got32 - want) <= 1e-5 + 1e-5 * np.abs(want)).all()


def test_pack_is_rebuilt_only_when_a_source_changes():
    from epnet_amd import li_fusion
    head = cases.make_head(cases.CONFIGS["two"])
    deconvs, conv, bn = head
    first = li_fusion.pack_image_head(*head)
    assert li_fusion.pack_image_head(*head, previous=first) is first
    assert first.is_current(*head)
    with torch.no_grad():
        deconvs[1].weight.mul_(1.5)
    second = li_fusion.pack_image_head(*head, previous=first)
    assert second is not first and not first.is_current(*head)
    assert torch.equal(second.weights[1], first.weights[1] * 1.5) and torch.equal(second.weights[0], first.weights[0])
    assert li_fusion.pack_image_head(*head, previous=second) is second
    bn.running_var.add_(0.25)
    third = li_fusion.pack_image_head(*head, previous=second)
    assert third is not second and not torch.equal(third.wf, second.wf)
    assert li_fusion.pack_image_head(*head, previous=third) is third
    # load_state_dict copies in place: a new pack although the values are the same
    bn.load_state_dict(bn.state_dict())
    fourth = li_fusion.pack_image_head(*head, previous=third)
    assert fourth is not third and torch.equal(fourth.wf, third.wf) and torch.equal(fourth.shift, third.shift)


def test_supports_image_head_at_points():
    from epnet_amd import li_fusion
    from epnet_amd.rpn_backbone import UpsampleDeConv
    cfg = cases.CONFIGS["two"]
    deconvs, conv, bn = cases.make_head(cfg)
    maps = cases.make_maps(cfg)
    assert li_fusion.supports_image_head_at_points(deconvs, conv, bn, maps)
    # kernel != stride
    other = torch.nn.ModuleList([deconvs[0], UpsampleDeConv(7, 2, kernel_size=4, stride=2)])
    assert not li_fusion.supports_image_head_at_points(other, conv, bn, maps)
    # a kernel of 3
    three = torch.nn.ModuleList([deconvs[0], UpsampleDeConv(7, 2, kernel_size=3, stride=3)])
    assert not li_fusion.supports_image_head_at_points(three, conv, bn, [maps[0], torch.randn(3, 7, 4, 6)])
    with pytest.raises(RuntimeError):
        li_fusion.pack_image_head(three, conv, bn)
    # a full size that is no multiple of the largest kernel: 10 x 20 under kernels 2 and 4
    assert not li_fusion.supports_image_head_at_points(deconvs, conv, bn, [torch.randn(3, 5, 5, 10), torch.randn(3, 7, 2, 5)])
    assert not li_fusion.supports_image_head_at_points(deconvs, conv, bn, [torch.randn(3, 5, 5, 10), torch.randn(3, 7, 3, 5)])
    single = torch.nn.ModuleList([UpsampleDeConv(5, 5, kernel_size=4, stride=4)])
    conv1 = torch.nn.Conv2d(5, 5, 1)
    assert li_fusion.supports_image_head_at_points(single, conv1, bn, [torch.randn(1, 5, 3, 5)])
    # 16-bit maps
    for dtype in (torch.float16, torch.bfloat16):
        assert not li_fusion.supports_image_head_at_points(deconvs, conv, bn, [m.to(dtype) for m in maps])
    # a level count or channel count that does not match
    assert not li_fusion.supports_image_head_at_points(deconvs, conv, bn, maps[:1])
    assert not li_fusion.supports_image_head_at_points(deconvs, conv, bn, [maps[0], maps[1][:, :6]])


def test_image_head_at_points_rejects_cpu_tensors():
    from epnet_amd import li_fusion
    cfg = cases.CONFIGS["two"]
    head = cases.make_head(cfg)
    with pytest.raises(RuntimeError, match="CUDAtensor"):
        li_fusion.image_head_at_points(cases.make_maps(cfg), li_fusion.pack_image_head(*head), cases.make_xy(cfg))


def test_binding_table_mirrors_the_header():
    import ctypes
    from epnet_amd import _lib
    i, vp, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert _lib.SIGNATURES["epnet_image_head_points_workspace_bytes"] == (sz, [i] * 5 + [vp] * 3 + [i])
    assert _lib.SIGNATURES["epnet_image_head_points"] == (i, [i] * 5 + [vp] * 5 + [i] + [vp] * 3 + [i, vp, vp, sz, vp])


def test_shape_rules_of_the_entry_point_without_gpu(hiplib):
    """sizes and limits are answered before anything touches the device"""
    import ctypes as C
    ints = lambda *v: (C.c_int * len(v))(*v)
    size = hiplib.epnet_image_head_points_workspace_bytes
    rnd = lambda v: (v + 255) // 256 * 256
    chans, kernels, reduce = ints(5, 7), ints(2, 4), ints(3, 2)
    want = (rnd(3 * 5 * 6 * 10 * 4) + rnd(3 * 7 * 3 * 5 * 4) + rnd(4 * 3 * 70 * 5 * 4) + rnd(4 * 3 * 70 * 4) + rnd((256 + 256 + 257 + 257) * 4))
    assert size(3, 70, 12, 20, 2, chans, kernels, reduce, 5) == want
    assert size(0, 70, 12, 20, 2, chans, kernels, reduce, 5) == 0
    assert size(3, 70, 10, 20, 2, chans, kernels, reduce, 5) == 0            # 10 is no multiple of 4
    assert size(3, 70, 12, 20, 2, chans, ints(2, 3), reduce, 5) == 0
    fake = C.c_void_p(4096)           # never dereferenced
    ptrs = (C.c_void_p * 2)(4096, 4096)
    call = hiplib.epnet_image_head_points
    args = lambda h, kern, red, q, ws_bytes: (3, 70, h, 20, 2, chans, kern, red, ptrs, ptrs, q, fake, fake, fake, 1, fake, fake, ws_bytes, None)
    assert call(*args(10, kernels, reduce, 5, want)) == -1
    assert call(*args(12, ints(2, 3), reduce, 5, want)) == -1
    assert call(*args(12, kernels, ints(3, 238), 5, 1 << 30)) == -4           # sum R above 240
    assert call(*args(12, kernels, reduce, 121, 1 << 30)) == -4
    assert call(*args(12, kernels, reduce, 5, want - 1)) == -3                # one byte short: nothing is launched
    assert call(0, 70, 12, 20, 2, chans, kernels, reduce, None, None, 5, None, None, None, 1, None, None, 0, None) == 0


def test_default_image_head_is_dense():
    from epnet_amd.rpn_backbone import Pointnet2MSG
    assert inspect.signature(Pointnet2MSG.__init__).parameters["image_head"].default == "dense"
    with pytest.raises(AssertionError):
        Pointnet2MSG(input_channels=0, image_head="sparse")


def test_points_head_falls_back_to_the_dense_lines_on_cpu(monkeypatch, oracle):
    """CPU stand-ins (the harness of tests/test_two_stream.py): nothing is on the GPU, so "points" runs the dense lines -- bitwise
    the same output, the same state_dict keys, and the packed cache stays empty"""
    import oracle_ext
    from epnet_amd import pointnet2_cuda
    from epnet_amd.rpn_backbone import Pointnet2MSG
    from test_two_stream import load_small, small_config
    p2, _, _ = oracle_ext.make_modules()
    for name, fn in vars(p2).items():
        if callable(fn):
            monkeypatch.setattr(pointnet2_cuda, name, fn)
    dense, fx = load_small("stock")
    points = Pointnet2MSG(input_channels=0, config=small_config(), sampler="stock", image_head="points")
    assert list(points.state_dict().keys()) == list(dense.state_dict().keys())
    points.load_state_dict(dense.state_dict())
    pts, image, xy = torch.from_numpy(fx["pts"]), torch.from_numpy(fx["image"]), torch.from_numpy(fx["xy"])
    with torch.no_grad():
        _, want = dense.eval()(pts.clone(), image.clone(), xy.clone())
        _, got = points.eval()(pts.clone(), image.clone(), xy.clone())
    assert torch.equal(got, want) and points._packed_head is None

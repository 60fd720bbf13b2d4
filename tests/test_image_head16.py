"""The 16-bit image head at the points, the parts that need no device (include/epnet_ops.h:
epnet_image_head_points_h): ``PackedImageHead.rows16``, ``supports_image_head_at_points(rows16=)``, the binding, the entry point's
shape rules, the rule itself against its yardsticks (tests/image_head16_cases.py) and the backbone's switch on the CPU."""
import inspect

import pytest
import torch

import image_head_cases as cases
import image_head16_cases as cases16


def _pack(name, seed=0):
    from epnet_amd import li_fusion
    cfg = cases16.CONFIGS[name]
    head = cases.make_head(cfg, seed)
    return cfg, head, li_fusion.pack_image_head(*head)


@pytest.mark.parametrize("dtype", cases16.TYPES)
@pytest.mark.parametrize("name", ["four", "two", "real", "wide"])
def test_rows16_is_the_rounded_pack_in_the_documented_layout(name, dtype):
    cfg, head, packed = _pack(name)
    weights16, wf16 = packed.rows16(dtype)
    pad = lambda v, to: (v + to - 1) // to * to
    sum_r, q = sum(cfg["reduce"]), cfg["q"]
    for wd, got, c, r, k in zip(packed.weights, weights16, cfg["chans"], cfg["reduce"], cfg["kernels"]):
        assert got.dtype == dtype and got.is_contiguous() and tuple(got.shape) == (k, k, pad(r, 16) // 16, pad(c, 32) // 32, 4, 16, 8)
        # [py][px][nb][ks][kq][col][e] -> [py][px][ci = 32 ks + 8 kq + e][r = 16 nb + col]
        plain = got.permute(0, 1, 3, 4, 6, 2, 5).reshape(k, k, pad(c, 32), pad(r, 16))
        assert torch.equal(plain[:, :, :c, :r], wd.to(dtype))
        assert (plain[:, :, c:, :] == 0).all() and (plain[:, :, :, r:] == 0).all()
        assert not torch.signbit(plain[:, :, c:, :].float()).any() and not torch.signbit(plain[:, :, :, r:].float()).any()
    assert wf16.dtype == dtype and wf16.is_contiguous() and tuple(wf16.shape) == (pad(q, 16) // 16, pad(sum_r, 32) // 32, 4, 16, 8)
    plain = wf16.permute(0, 3, 1, 2, 4).reshape(pad(q, 16), pad(sum_r, 32))     # [qb][col] x [ks][kq][e]
    assert torch.equal(plain[:q, :sum_r], packed.wf.to(dtype))
    assert (plain[q:] == 0).all() and (plain[:, sum_r:] == 0).all()
    # the float32 fields stay what tests/test_image_head.py reads
    assert all(w.dtype == torch.float32 and tuple(w.shape) == (k, k, c, r)
               for w, c, r, k in zip(packed.weights, cfg["chans"], cfg["reduce"], cfg["kernels"]))
    assert packed.wf.dtype == torch.float32 and packed.shift.dtype == torch.float32


def test_rows16_is_built_once_per_dtype_and_rebuilt_with_the_pack():
    from epnet_amd import li_fusion
    cfg, head, packed = _pack("two")
    half = packed.rows16(torch.float16)
    assert packed.rows16(torch.float16) is half
    brain = packed.rows16(torch.bfloat16)
    assert packed.rows16(torch.bfloat16) is brain and packed.rows16(torch.float16) is half and brain is not half
    assert li_fusion.pack_image_head(*head, previous=packed) is packed and packed.rows16(torch.float16) is half
    with torch.no_grad():
        head[0][0].weight.mul_(2.0)
    again = li_fusion.pack_image_head(*head, previous=packed)
    assert again is not packed
    fresh = again.rows16(torch.float16)
    assert fresh is not half and torch.equal(fresh[0][0].float(), (half[0][0].float() * 2.0))
    with pytest.raises(RuntimeError):
        packed.rows16(torch.float32)


def test_supports_image_head_at_points_with_rows16():
    from epnet_amd import li_fusion
    cfg, (deconvs, conv, bn), _ = _pack("two")
    maps = cases.make_maps(cfg)
    assert "rows16" in inspect.signature(li_fusion.supports_image_head_at_points).parameters
    assert inspect.signature(li_fusion.supports_image_head_at_points).parameters["rows16"].default is False
    assert li_fusion.supports_image_head_at_points(deconvs, conv, bn, maps, rows16=True)          # float32 as before
    for dtype in cases16.TYPES:
        low = [m.to(dtype) for m in maps]
        assert not li_fusion.supports_image_head_at_points(deconvs, conv, bn, low)
        assert li_fusion.supports_image_head_at_points(deconvs, conv, bn, low, rows16=True)
        assert not li_fusion.supports_image_head_at_points(deconvs, conv, bn, [low[0], maps[1]], rows16=True)
        assert not li_fusion.supports_image_head_at_points(deconvs, conv, bn, [low[0], low[1][:, :6]], rows16=True)
    mixed = [maps[0].half(), maps[1].bfloat16()]
    assert not li_fusion.supports_image_head_at_points(deconvs, conv, bn, mixed, rows16=True)
    assert not li_fusion.supports_image_head_at_points(deconvs, conv, bn, [m.double() for m in maps], rows16=True)


def test_binding_table_mirrors_the_header(hiplib):
    import ctypes
    from epnet_amd import _lib
    i, vp, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert _lib.SIGNATURES["epnet_image_head_points_h_workspace_bytes"] == (sz, [i] * 5 + [vp] * 3 + [i])
    assert _lib.SIGNATURES["epnet_image_head_points_h"] == (i, [i] * 5 + [vp] * 3 + [i] + [vp] * 2 + [i] + [vp] * 3 + [i, vp, vp, sz, vp])
    assert hiplib.epnet_image_head_points_h_workspace_bytes and hiplib.epnet_image_head_points_h


@pytest.mark.parametrize("dtype", cases16.TYPES)
def test_image_head_at_points_rejects_cpu_tensors(dtype):
    from epnet_amd import li_fusion
    cfg, head, packed = _pack("two")
    with pytest.raises(RuntimeError, match="CUDAtensor"):
        li_fusion.image_head_at_points(cases16.maps_of(cfg, dtype), packed, cases.make_xy(cfg))
    maps = cases.make_maps(cfg)
    with pytest.raises(RuntimeError, match="one type"):
        li_fusion.image_head_at_points([maps[0].to(dtype), maps[1]], packed, cases.make_xy(cfg))


def test_shape_rules_of_the_entry_point_without_gpu(hiplib):
    """sizes, limits and the type code are answered before anything touches the device"""
    import ctypes as C
    ints = lambda *v: (C.c_int * len(v))(*v)
    size = hiplib.epnet_image_head_points_h_workspace_bytes
    rnd = lambda v: (v + 255) // 256 * 256
    chans, kernels, reduce = ints(5, 7), ints(2, 4), ints(3, 2)
    # the copies: 2 bytes, 5 and 7 channels padded to 32
    want = (rnd(3 * 32 * 6 * 10 * 2) + rnd(3 * 32 * 3 * 5 * 2) + rnd(4 * 3 * 70 * 5 * 4) + rnd(4 * 3 * 70 * 4) + rnd((256 + 256 + 257 + 257) * 4))
    assert size(3, 70, 12, 20, 2, chans, kernels, reduce, 5) == want
    assert size(0, 70, 12, 20, 2, chans, kernels, reduce, 5) == 0
    assert size(3, 70, 10, 20, 2, chans, kernels, reduce, 5) == 0            # 10 is no multiple of 4
    assert size(3, 70, 12, 20, 2, chans, ints(2, 3), reduce, 5) == 0
    assert size(3, 70, 12, 20, 2, chans, kernels, ints(3, 238), 5) == 0
    fake = C.c_void_p(4096)           # never dereferenced
    ptrs = (C.c_void_p * 2)(4096, 4096)
    call = hiplib.epnet_image_head_points_h
    args = lambda h, kern, red, q, ws_bytes, dtype=2, maps=ptrs, out=fake: (
        3, 70, h, 20, 2, chans, kern, red, dtype, maps, ptrs, q, fake, fake, fake, 1, out, fake, ws_bytes, None)
    assert call(*args(10, kernels, reduce, 5, want)) == -1
    assert call(*args(12, ints(2, 3), reduce, 5, want)) == -1
    assert call(*args(12, kernels, ints(3, 238), 5, 1 << 30)) == -4           # sum R = 241
    assert call(*args(12, kernels, reduce, 121, 1 << 30)) == -4
    assert call(*args(12, kernels, reduce, 5, want, dtype=0)) == -1
    assert call(*args(12, kernels, reduce, 5, want, dtype=3)) == -1
    assert call(*args(12, kernels, reduce, 5, want, out=None)) == -1
    assert call(*args(12, kernels, reduce, 5, want, maps=(C.c_void_p * 2)(4096, None))) == -1
    for dtype in (1, 2):
        assert call(*args(12, kernels, reduce, 5, want - 1, dtype=dtype)) == -3   # one byte short: nothing is launched
    assert call(0, 70, 12, 20, 2, chans, kernels, reduce, 1, None, None, 5, None, None, None, 1, None, None, 0, None) == 0


@pytest.mark.parametrize("dtype", cases16.TYPES)
@pytest.mark.parametrize("name", ["four", "two", "real"])
def test_the_rule_meets_its_bound_and_is_as_close_as_autocast(name, dtype):
    """the rule emulated in float64 with its two roundings: within the bound of R, and its mean absolute error against the true
    head at most 1.5 x that of the stock dense head under torch.autocast("cpu", T) (measured 0.78 - 1.19 when the rule was chosen)"""
    cfg, head, packed = _pack(name)
    maps, xy = cases16.maps_of(cfg, dtype), cases16.grid_xy(cfg)
    got = cases16.rule_emulated(packed, maps, xy, dtype)
    assert got.dtype == dtype
    worst = cases16.worst_of_bound(got, packed, maps, xy, cfg, dtype)
    truth = cases16.true_head(head, maps, xy)
    stock = cases16.autocast_head(head, maps, xy, dtype)
    e_rule, e_stock = (got.double() - truth).abs().mean().item(), (stock.double() - truth).abs().mean().item()
    print("%s %s: %.3f of the bound; mean |error| against the true head: rule %.3e, stock autocast %.3e, ratio %.3f"
          % (name, dtype, worst, e_rule, e_stock, e_rule / e_stock))
    assert worst <= 1.0
    assert truth.abs().max().item() > 0.1 and e_stock > 0
    assert e_rule <= 1.5 * e_stock


def test_rows16_switch_defaults_to_false():
    from epnet_amd.rpn_backbone import Pointnet2MSG
    assert inspect.signature(Pointnet2MSG.__init__).parameters["image_head_rows16"].default is False
    assert Pointnet2MSG(input_channels=0).image_head_rows16 is False


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_rows16_switch_changes_no_bit_on_the_cpu(monkeypatch, oracle, mode):
    """CPU stand-ins (the harness of tests/test_two_stream.py): nothing is on the GPU, so the switch runs the dense lines"""
    import oracle_ext
    from epnet_amd import pointnet2_cuda
    from epnet_amd.rpn_backbone import Pointnet2MSG
    from test_two_stream import load_small, small_config
    p2, _, _ = oracle_ext.make_modules()
    for name, fn in vars(p2).items():
        if callable(fn):
            monkeypatch.setattr(pointnet2_cuda, name, fn)
    dense, fx = load_small("stock")
    points = Pointnet2MSG(input_channels=0, config=small_config(), sampler="stock", image_head="points", image_head_rows16=True)
    assert list(points.state_dict().keys()) == list(dense.state_dict().keys())
    points.load_state_dict(dense.state_dict())
    pts, image, xy = torch.from_numpy(fx["pts"]), torch.from_numpy(fx["image"]), torch.from_numpy(fx["xy"])
    dense.train(mode == "train")
    points.train(mode == "train")
    with torch.no_grad():
        _, want = dense(pts.clone(), image.clone(), xy.clone())
        _, got = points(pts.clone(), image.clone(), xy.clone())
    assert torch.equal(got, want) and points._packed_head is None

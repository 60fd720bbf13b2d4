"""The 16-bit image head at the points on the device (include/epnet_ops.h: epnet_image_head_points_h).

Values: within ``(2 u + (K + 8) 2^-24) A`` of R, the rule without its inner rounding, both in stock float64 ops on the device
(tests/image_head16_cases.py, where the bound is derived); coordinates on a grid of 2^-10 so that the float32 tap weights are exact.
Against the stock dense head under autocast: the mean absolute error against the true (float64) head at most 1.5 x the stock one's.
Everything else is bitwise."""
import json
import os
import subprocess
import sys

import pytest
import torch

import image_head_cases as cases
import image_head16_cases as cases16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TYPES = pytest.mark.parametrize("dtype", cases16.TYPES, ids=["f16", "bf16"])


def _setup(name, dtype, b=None, n=None, xy=None, seed=0, cfg=None):
    from epnet_amd import li_fusion
    cfg = cases16.CONFIGS[name] if cfg is None else cfg
    head_dev = cases.head_to(cases.make_head(cfg, seed), device=DEV)
    maps = [m.to(DEV) for m in cases16.maps_of(cfg, dtype, b, seed + 1)]
    xy = (cases16.grid_xy(cfg, b, n, seed + 2) if xy is None else xy).to(DEV)
    return cfg, head_dev, li_fusion.pack_image_head(*head_dev), maps, xy


def _run(maps, packed, xy):
    from epnet_amd import li_fusion
    got = li_fusion.image_head_at_points(maps, packed, xy)
    assert got.dtype == maps[0].dtype and tuple(got.shape) == (xy.shape[0], packed.q, xy.shape[1])
    assert not got.requires_grad and got.grad_fn is None
    return got


def _check_values(cfg, packed, maps, xy, what):
    got = _run(maps, packed, xy)
    worst = cases16.worst_of_bound(got, packed, maps, xy, cfg, maps[0].dtype)
    print("%s %s: %.3f of the bound" % (what, maps[0].dtype, worst))
    assert worst <= 1.0, (what, worst)
    return got


@TYPES
@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 257])
@pytest.mark.parametrize("name", ["four", "two", "real", "wide"])
def test_values_within_the_bound_of_the_unrounded_rule(hiplib, name, n, dtype):
    cfg, head_dev, packed, maps, xy = _setup(name, dtype, n=n)
    got = _check_values(cfg, packed, maps, xy, "%s n=%d" % (name, n))
    if n >= 6:
        assert got.float().abs().max().item() > 0.1
        assert (got[:, :, 2:4] == 0).all()               # the two points outside the map


def _error_ratio(head_dev, packed, maps, xy, what):
    dtype = maps[0].dtype
    got = _run(maps, packed, xy)
    truth = cases16.true_head(head_dev, maps, xy)
    stock = cases16.autocast_head(head_dev, maps, xy, dtype)
    e_got, e_stock = (got.double() - truth).abs().mean().item(), (stock.double() - truth).abs().mean().item()
    print("%s %s: mean |error| against the true head: points %.4e, stock autocast %.4e, ratio %.3f" % (what, dtype, e_got, e_stock, e_got / e_stock))
    assert truth.abs().max().item() > 0.1 and e_stock > 0
    assert e_got <= 1.5 * e_stock, (what, e_got, e_stock)


@TYPES
def test_as_close_to_the_true_head_as_stock_autocast(hiplib, dtype):
    cfg, head_dev, packed, maps, xy = _setup("real", dtype)
    _error_ratio(head_dev, packed, maps, xy, "real")


@TYPES
def test_full_size_scene(hiplib, dtype):
    """1 scene, 384 x 1280, 16384 points, the yaml's widths: bin offsets and tile counts are only real here"""
    cfg = dict(cases.CONFIGS["real"], h=384, w=1280, b=1, n=16384)
    cfg, head_dev, packed, maps, xy = _setup(None, dtype, seed=3, cfg=cfg)
    _error_ratio(head_dev, packed, maps, xy, "full size")


@TYPES
@pytest.mark.parametrize("name", ["four", "real"])
def test_points_on_a_lattice_of_pitch_16(hiplib, name, dtype):
    """each of the four corners of every point falls into ONE phase bin, and many points share a pixel"""
    cfg = cases16.CONFIGS[name]
    g = torch.Generator().manual_seed(5)
    n = 257
    sites = torch.stack([torch.randint(0, cfg["w"] // 16, (2, n), generator=g) * 16.0,
                         torch.randint(0, cfg["h"] // 16, (2, n), generator=g) * 16.0], dim=2) + torch.tensor([0.25, 0.5])
    norm = lambda s: torch.stack([2.0 * s[..., 0] / (cfg["w"] - 1) - 1.0, 2.0 * s[..., 1] / (cfg["h"] - 1) - 1.0], dim=2)
    _, head_dev, packed, maps, xy = _setup(name, dtype, b=2, xy=torch.round(norm(sites) * 1024.0) / 1024.0)
    _check_values(cfg, packed, maps, xy, "%s lattice" % name)


@TYPES
@pytest.mark.parametrize("name", ["two", "wide"])
def test_every_point_on_the_same_pixel(hiplib, name, dtype):
    cfg = cases16.CONFIGS[name]
    xy = torch.round(torch.tensor(cases.pixel_centre(cfg, 9.3, 4.6)) * 1024.0).div(1024.0).repeat(2, 200, 1)
    _, head_dev, packed, maps, xy = _setup(name, dtype, b=2, xy=xy)
    got = _check_values(cfg, packed, maps, xy, "%s same pixel" % name)
    assert (got == got[:, :, :1]).all()


@TYPES
@pytest.mark.parametrize("name", ["two", "real"])
def test_every_point_outside_the_map_gives_exact_zeros(hiplib, name, dtype):
    g = torch.Generator().manual_seed(6)
    n = 130
    far = 1.0 + 4.0 / min(cases.CONFIGS[name]["h"], cases.CONFIGS[name]["w"]) + torch.rand((2, n, 2), generator=g)
    sign = torch.where(torch.rand((2, n, 2), generator=g) < 0.5, -1.0, 1.0)
    xy = far * sign
    xy[:, 0] = torch.tensor([float("nan"), 0.0])
    xy[:, 1] = torch.tensor([0.0, float("inf")])
    xy[:, 2] = torch.tensor([-3e38, 0.5])
    _, head_dev, packed, maps, xy = _setup(name, dtype, b=2, xy=xy)
    got = _run(maps, packed, xy)
    assert (got == 0).all() and not torch.signbit(got).any()


def _unread_pixels(cfg, maps, xy):
    """per level a (B, 1, hl, wl) mask of the pixels under no tap; the taps as the float32 kernels take them (exact on the grid)"""
    h, w = cfg["h"], cfg["w"]
    ix, iy = ((xy[..., 0] + 1.0) / 2.0) * (w - 1), ((xy[..., 1] + 1.0) / 2.0) * (h - 1)
    x0, y0 = torch.floor(ix).long(), torch.floor(iy).long()
    masks = []
    for m, k in zip(maps, cfg["kernels"]):
        read = torch.zeros((m.shape[0], m.shape[2], m.shape[3]), dtype=torch.bool, device=m.device)
        for dx in (0, 1):
            for dy in (0, 1):
                x, y = x0 + dx, y0 + dy
                ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
                bi = torch.arange(m.shape[0], device=m.device)[:, None].expand_as(x)
                read[bi[ok], (y[ok] // k), (x[ok] // k)] = True
        masks.append(~read[:, None])
    return masks


@TYPES
@pytest.mark.parametrize("name", ["four", "wide"])
def test_padding_and_unread_pixels_do_not_leak(hiplib, name, dtype):
    """every pixel no tap reads is NaN, then +inf: the same bits as with the clean maps (a zero of the padding times such a
    neighbour would be a NaN)"""
    cfg, head_dev, packed, maps, xy = _setup(name, dtype, n=40)
    clean = _run(maps, packed, xy)
    masks = _unread_pixels(cfg, maps, xy)
    assert masks[0].any()
    for poison in (float("nan"), float("inf")):
        dirty = [torch.where(mask, torch.full_like(m, poison), m) for m, mask in zip(maps, masks)]
        got = _run(dirty, packed, xy)
        assert torch.equal(got.view(torch.int16), clean.view(torch.int16)), poison


@TYPES
@pytest.mark.parametrize("name", ["four", "real"])
def test_bitwise_invariances(hiplib, name, dtype):
    """a tap's value depends on its pixel, its scene's maps and the weights alone"""
    cfg, head_dev, packed, maps, xy = _setup(name, dtype, b=3, n=257)
    bits = lambda t: t.view(torch.int16)
    first = _run(maps, packed, xy)
    assert torch.equal(bits(_run(maps, packed, xy)), bits(first))                                   # two runs
    perm = torch.randperm(257, generator=torch.Generator().manual_seed(7)).to(DEV)
    assert torch.equal(bits(_run(maps, packed, xy[:, perm].contiguous())), bits(first[:, :, perm].contiguous()))
    order = [2, 0, 1]                                                                                # scenes permuted
    assert torch.equal(bits(_run([m[order].contiguous() for m in maps], packed, xy[order].contiguous())), bits(first[order].contiguous()))
    for b in range(3):                                                                               # a scene alone
        alone = _run([m[b:b + 1].contiguous() for m in maps], packed, xy[b:b + 1].contiguous())
        assert torch.equal(bits(alone[0]), bits(first[b]))
    # fewer points, and extra points in front: other bins, other tiles, the same values
    assert torch.equal(bits(_run(maps, packed, xy[:, :100].contiguous())), bits(first[:, :, :100].contiguous()))
    extra = cases16.grid_xy(cfg, 3, 91, seed=33).to(DEV)
    more = _run(maps, packed, torch.cat([extra, xy], dim=1).contiguous())
    assert torch.equal(bits(more[:, :, 91:].contiguous()), bits(first))


def _offset_view(t, off):
    """the same values in a view that starts `off` elements into a larger buffer"""
    buf = torch.empty((t.numel() + 16,), dtype=t.dtype, device=t.device)
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + off * t.element_size()
    return view


@TYPES
@pytest.mark.parametrize("name", ["four", "real"])
def test_offset_pointers(hiplib, name, dtype):
    """maps and out at any 2-byte aligned address give the aligned call's bits; an unaligned pack is refused before a launch"""
    from epnet_amd import _lib, pointnet2_cuda
    cfg, head_dev, packed, maps, xy = _setup(name, dtype, n=257)
    want = _run(maps, packed, xy)
    for off in (1, 3):
        got = _run([_offset_view(m, off) for m in maps], packed, xy)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), off
    b, n, q = xy.shape[0], 257, cfg["q"]
    weights16, wf16 = packed.rows16(dtype)
    shapes = (b, n, cfg["h"], cfg["w"], cfg["chans"], cfg["kernels"], cfg["reduce"])
    for off in (1, 3):
        out_buf = torch.full((b * q * n + 16,), 7.0, dtype=dtype, device=DEV)
        out = out_buf[off:off + b * q * n].view(b, q, n)
        pointnet2_cuda.image_head_points_h_wrapper(*shapes, maps, weights16, q, wf16, packed.shift, xy, True, out)
        assert torch.equal(out.view(torch.int16), want.view(torch.int16))
        assert (out_buf[:off] == 7.0).all() and (out_buf[off + b * q * n:] == 7.0).all()
        out = torch.full((b, q, n), 7.0, dtype=dtype, device=DEV)
        with pytest.raises(_lib.EpnetError):
            pointnet2_cuda.image_head_points_h_wrapper(*shapes, maps, [_offset_view(v, off) for v in weights16], q, wf16, packed.shift,
                                                       xy, True, out)
        with pytest.raises(_lib.EpnetError):
            pointnet2_cuda.image_head_points_h_wrapper(*shapes, maps, weights16, q, _offset_view(wf16, off), packed.shift, xy, True, out)
        torch.cuda.synchronize()
        assert (out == 7.0).all()                                                                    # nothing was launched


@TYPES
@pytest.mark.parametrize("name", ["four", "real"])
def test_graph_capture_and_replay_on_new_contents(hiplib, name, dtype):
    from epnet_amd import li_fusion
    cfg, head_dev, packed, maps, xy = _setup(name, dtype, n=257)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        li_fusion.image_head_at_points(maps, packed, xy)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = li_fusion.image_head_at_points(maps, packed, xy)
    new_maps = [m.to(DEV) for m in cases16.maps_of(cfg, dtype, seed=21)]
    new_xy = cases16.grid_xy(cfg, n=257, seed=22).to(DEV)
    for m, v in zip(maps, new_maps):
        m.copy_(v)
    xy.copy_(new_xy)
    graph.replay()
    torch.cuda.synchronize()
    want = li_fusion.image_head_at_points(new_maps, packed, new_xy)
    assert torch.equal(out.view(torch.int16), want.view(torch.int16)) and out.float().abs().max().item() > 0.05


@TYPES
@pytest.mark.parametrize("name", ["two", "wide"])
def test_workspace_bounds(hiplib, name, dtype):
    """nothing is written outside workspace_bytes or out; one byte less is refused before anything is launched"""
    from epnet_amd import _lib, pointnet2_cuda
    cfg, head_dev, packed, maps, xy = _setup(name, dtype, n=257)
    b, n, h, w, q = xy.shape[0], 257, cfg["h"], cfg["w"], cfg["q"]
    want = _run(maps, packed, xy)
    ws_bytes = pointnet2_cuda.image_head_points_h_workspace_bytes(b, n, h, w, cfg["chans"], cfg["kernels"], cfg["reduce"], q)
    assert ws_bytes > 0 and ws_bytes % 256 == 0
    guard = 4096
    raw = torch.full((guard + ws_bytes + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    out_raw = torch.full((guard + b * q * n * 2 + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    out = out_raw[guard:guard + b * q * n * 2].view(dtype).view(b, q, n)
    weights16, wf16 = packed.rows16(dtype)
    args = (b, n, h, w, cfg["chans"], cfg["kernels"], cfg["reduce"], maps, weights16, q, wf16, packed.shift, xy, True, out)
    with pytest.raises(_lib.EpnetError, match="workspace"):
        pointnet2_cuda.image_head_points_h_wrapper(*args, workspace=raw[guard:guard + ws_bytes - 1])
    torch.cuda.synchronize()
    assert (raw == 0xA5).all() and (out_raw == 0xA5).all()                   # nothing was launched
    pointnet2_cuda.image_head_points_h_wrapper(*args, workspace=raw[guard:guard + ws_bytes])
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))
    for buf, size in ((raw, ws_bytes), (out_raw, b * q * n * 2)):
        assert (buf[:guard] == 0xA5).all() and (buf[guard + size:] == 0xA5).all()


# ---- the backbone ------------------------------------------------------------------------------------------------------------------
def _small_models(rows16):
    from epnet_amd.rpn_backbone import Pointnet2MSG
    from test_two_stream import load_small, small_config
    dense, fx = load_small("hip", DEV)
    points = Pointnet2MSG(input_channels=0, config=small_config(), sampler="hip", image_head="points", image_head_rows16=rows16).to(DEV)
    assert list(points.state_dict().keys()) == list(dense.state_dict().keys())
    points.load_state_dict(dense.state_dict())
    inputs = tuple(torch.from_numpy(fx[k]).to(DEV) for k in ("pts", "image", "xy"))
    return dense, points, inputs, torch.from_numpy(fx["probe"]).to(DEV)


@TYPES
def test_backbone_takes_the_16_bit_head_under_autocast(hiplib, dtype):
    from epnet_amd import li_fusion
    dense, points, (pts, image, xy), _ = _small_models(True)
    points.eval()
    caught, maps, conv_calls = [], [], []
    points.final_fusion_img_point.register_forward_hook(lambda mod, args, out: caught.append(args[1]))
    for block in points.Img_Block:
        block.register_forward_hook(lambda mod, args, out: maps.append(out))
    points.image_fusion_conv.register_forward_hook(lambda mod, args, out: conv_calls.append(tuple(out.shape)))
    xy_run = xy.clone()
    with torch.no_grad(), torch.autocast("cuda", dtype):
        _, feats = points(pts.clone(), image.clone(), xy_run)       # xy_run is normalised in place
    assert conv_calls == [] and len(caught) == 1 and len(maps) == 4 and all(m.dtype == dtype for m in maps)
    packed = points._packed_head
    assert packed is not None and dtype in packed._rows16
    assert caught[0].dtype == dtype and tuple(caught[0].shape) == (2, 4, 1024) and caught[0].float().abs().max().item() > 0
    assert torch.equal(caught[0].view(torch.int16), li_fusion.image_head_at_points(maps, packed, xy_run).view(torch.int16))
    # the head on the maps the model made against R. The model's coordinates are free float32 values; the bound is stated for
    # exact tap weights, so the comparison runs on the same coordinates moved onto the grid of 2^-10
    cfg = dict(chans=packed.chans, reduce=packed.reduce, kernels=packed.kernels, q=packed.q)
    snapped = (torch.round(xy_run * 1024.0) / 1024.0).contiguous()
    shifted = li_fusion.image_head_at_points(maps, packed, snapped)
    worst = cases16.worst_of_bound(shifted, packed, maps, snapped, cfg, dtype)
    print("backbone %s: %.3f of the bound" % (dtype, worst))
    assert worst <= 1.0


class _deterministic_dense_layers:
    """two runs of the same dense lines are compared bit for bit: the dense library's run-to-run choices (summation order of the
    image convolutions at 2 scenes, see bench_step.infer) are switched off for the comparison"""

    def __enter__(self):
        self.prev = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
                     torch.backends.cudnn.deterministic)
        torch.use_deterministic_algorithms(True, warn_only=True)
        torch.backends.cudnn.deterministic = True

    def __exit__(self, *exc):
        torch.use_deterministic_algorithms(self.prev[0], warn_only=self.prev[1])
        torch.backends.cudnn.deterministic = self.prev[2]
        return False


@TYPES
def test_backbone_without_the_switch_runs_the_dense_lines_under_autocast(hiplib, dtype):
    dense, points, (pts, image, xy), _ = _small_models(False)
    results = []
    with _deterministic_dense_layers():
        for model in (dense, points):
            model.eval()
            calls = []
            handle = model.image_fusion_conv.register_forward_hook(lambda mod, args, out: calls.append(tuple(out.shape)))
            with torch.no_grad(), torch.autocast("cuda", dtype):
                _, feats = model(pts.clone(), image.clone(), xy.clone())
            handle.remove()
            assert calls == [(2, 4, 32, 64)]
            results.append(feats)
    assert points._packed_head is None and torch.equal(results[0], results[1])


@TYPES
@pytest.mark.parametrize("mode", ["train", "eval with grad"])
def test_backbone_with_the_switch_runs_the_dense_lines_when_a_gradient_is_needed(hiplib, mode, dtype):
    dense, points, (pts, image, xy), probe = _small_models(True)
    results = []
    with _deterministic_dense_layers():
        for model in (dense, points):
            model.train(mode == "train")
            calls = []
            handle = model.image_fusion_conv.register_forward_hook(lambda mod, args, out: calls.append(tuple(out.shape)))
            img = image.clone().requires_grad_(True)
            with torch.autocast("cuda", dtype):
                _, feats = model(pts.clone(), img, xy.clone())
            (feats.float() * probe).sum().backward()
            handle.remove()
            assert calls == [(2, 4, 32, 64)]
            results.append((feats.detach(), img.grad.clone()))
    assert points._packed_head is None
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])


def test_bench_step_infer_under_autocast():
    """bench_step.py --infer under --amp bf16 opens the autocast region, says so, and its graph replays what eager computes"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench_step.py"), "--infer", "--image", "--two-stage", "--image-head", "points", "--amp", "bf16",
           "--points", "2048", "--batch", "2", "--steps", "2"]
    done = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    rows = [json.loads(line) for line in done.stdout.splitlines() if line.startswith("{")]
    print(done.stdout)
    assert len(rows) == 2
    for row in rows:
        assert "bf16" in row["dtype"] and "autocast" in row["dtype"]
    assert any(row.get("graph_equals_eager") is True for row in rows)
    assert all(row.get("graph_equals_eager", True) is True for row in rows)

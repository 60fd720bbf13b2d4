"""LI-Fusion's image head at the points only, on the device (include/epnet_ops.h: epnet_image_head_points).

Yardstick everywhere: the stock dense head -- the backbone's own three lines on ``stock_feature_gather`` -- in float64 on the
device. Tolerance: ``1e-5 + 1e-5 * |ref|``, the project's float tolerance; every value test also asserts that the stock float32
dense head stays within HALF of it on the same inputs, so the inputs are shown to be fair. "four" and "two" take the scalar
loads of ih_taps_kernel, "real" (the yaml's widths) and the small backbone fixture the 128-bit ones."""
import pytest
import torch

import image_head_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _setup(name, b=None, n=None, xy=None, seed=0):
    from epnet_amd import li_fusion
    cfg = cases.CONFIGS[name]
    head = cases.make_head(cfg, seed)
    maps = [m.to(DEV) for m in cases.make_maps(cfg, b, seed + 1)]
    xy = (cases.make_xy(cfg, b, n, seed + 2) if xy is None else xy).to(DEV)
    head_dev = cases.head_to(head, device=DEV)
    return cfg, head_dev, li_fusion.pack_image_head(*head_dev), maps, xy


def _check_values(head_dev, packed, maps, xy, what):
    """the points path within the tolerance of the float64 dense head, the float32 dense head within half of it"""
    from epnet_amd import li_fusion
    with torch.no_grad():
        ref = cases.dense_head(cases.head_to(head_dev, dtype=torch.float64), [m.double() for m in maps], xy.double())
        dense32 = cases.dense_head(head_dev, maps, xy)
    got = li_fusion.image_head_at_points(maps, packed, xy)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(ref.shape) and not got.requires_grad
    tol = 1e-5 + 1e-5 * ref.abs()
    e_got, e_dense = ((got.double() - ref).abs() / tol).max().item(), ((dense32.double() - ref).abs() / tol).max().item()
    print("%s: points path %.3f of the tolerance, float32 dense head %.3f" % (what, e_got, e_dense))
    assert e_dense <= 0.5, (what, e_dense)
    assert e_got <= 1.0, (what, e_got)
    return got, ref


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("name", ["four", "two", "real"])
def test_values_against_the_float64_dense_head(hiplib, name, n):
    cfg, head_dev, packed, maps, xy = _setup(name, n=n)
    got, ref = _check_values(head_dev, packed, maps, xy, "%s n=%d" % (name, n))
    if n >= 6:
        assert ref.abs().max().item() > 0.1
        assert (got[:, :, 2:4] == 0).all()               # the two points outside the map


@pytest.mark.parametrize("name", ["four", "real"])
def test_points_on_a_lattice_of_pitch_16(hiplib, name):
    """every point at the same offset from a pixel whose coordinates are multiples of 16: each of the four corners of every point
    falls into ONE phase bin (four bins take every tap, 252 are empty), and many points share a pixel"""
    cfg = cases.CONFIGS[name]
    g = torch.Generator().manual_seed(5)
    n = 257
    sites = torch.stack([torch.randint(0, cfg["w"] // 16, (2, n), generator=g) * 16.0,
                         torch.randint(0, cfg["h"] // 16, (2, n), generator=g) * 16.0], dim=2) + torch.tensor([0.25, 0.5])
    xy = torch.stack([2.0 * sites[..., 0] / (cfg["w"] - 1) - 1.0, 2.0 * sites[..., 1] / (cfg["h"] - 1) - 1.0], dim=2)
    _, head_dev, packed, maps, xy = _setup(name, b=2, xy=xy)
    _check_values(head_dev, packed, maps, xy, "%s lattice" % name)
    # and exactly on the lattice pixels' centres (one tap carries all the weight, up to the rounding of the coordinate)
    sites = sites - torch.tensor([0.25, 0.5])
    xy = torch.stack([2.0 * sites[..., 0] / (cfg["w"] - 1) - 1.0, 2.0 * sites[..., 1] / (cfg["h"] - 1) - 1.0], dim=2).to(DEV)
    _check_values(head_dev, packed, maps, xy, "%s lattice centres" % name)


@pytest.mark.parametrize("name", ["two", "real"])
def test_every_point_on_the_same_pixel(hiplib, name):
    cfg = cases.CONFIGS[name]
    xy = torch.tensor(cases.pixel_centre(cfg, 9.3, 4.6)).repeat(2, 200, 1)
    _, head_dev, packed, maps, xy = _setup(name, b=2, xy=xy)
    got, _ = _check_values(head_dev, packed, maps, xy, "%s same pixel" % name)
    assert (got == got[:, :, :1]).all()


@pytest.mark.parametrize("name", ["two", "real"])
def test_every_point_outside_the_map_gives_exact_zeros(hiplib, name):
    from epnet_amd import li_fusion
    g = torch.Generator().manual_seed(6)
    n = 130
    far = 1.0 + 4.0 / min(cases.CONFIGS[name]["h"], cases.CONFIGS[name]["w"]) + torch.rand((2, n, 2), generator=g)
    sign = torch.where(torch.rand((2, n, 2), generator=g) < 0.5, -1.0, 1.0)
    xy = far * sign
    xy[:, 0] = torch.tensor([float("nan"), 0.0])
    xy[:, 1] = torch.tensor([0.0, float("inf")])
    xy[:, 2] = torch.tensor([-3e38, 0.5])
    _, head_dev, packed, maps, xy = _setup(name, b=2, xy=xy)
    got = li_fusion.image_head_at_points(maps, packed, xy)
    assert (got == 0).all() and not torch.signbit(got).any()


def test_full_size_scene(hiplib):
    """1 scene, 384 x 1280, 16384 points, the yaml's widths: bin offsets and tile counts are only real here"""
    cfg = dict(cases.CONFIGS["real"], h=384, w=1280, b=1, n=16384)
    from epnet_amd import li_fusion
    head_dev = cases.head_to(cases.make_head(cfg, 3), device=DEV)
    maps = [m.to(DEV) for m in cases.make_maps(cfg, seed=4)]
    # coordinates on a grid of 2^-10: (x + 1) / 2 * 1279 then fits float32's 24 bits, so the float32 samplers' taps and weights are
    # exact. A free float32 coordinate is placed 1279 * 6e-8 = 8e-5 pixels off by that product, which moves ANY float32 sampler --
    # the stock one too -- seven tolerances from the float64 run at this width (measured: 7.07 for both); that is the
    # coordinate's rounding, not the head's, and the small maps above carry the free coordinates
    xy = (torch.round(cases.make_xy(cfg, seed=5) * 1024.0) / 1024.0).to(DEV)
    got, ref = _check_values(head_dev, li_fusion.pack_image_head(*head_dev), maps, xy, "full size")
    assert ref.abs().max().item() > 0.1


@pytest.mark.parametrize("name", ["four", "real"])
def test_bitwise_invariances(hiplib, name):
    """a tap's value depends on its pixel, its scene's maps and the weights alone"""
    from epnet_amd import li_fusion
    cfg, head_dev, packed, maps, xy = _setup(name, b=3, n=257)
    first = li_fusion.image_head_at_points(maps, packed, xy)
    assert torch.equal(li_fusion.image_head_at_points(maps, packed, xy), first)                  # two runs
    perm = torch.randperm(257, generator=torch.Generator().manual_seed(7)).to(DEV)
    assert torch.equal(li_fusion.image_head_at_points(maps, packed, xy[:, perm].contiguous()), first[:, :, perm])
    for b in range(3):                                                                           # a scene alone
        alone = li_fusion.image_head_at_points([m[b:b + 1].contiguous() for m in maps], packed, xy[b:b + 1].contiguous())
        assert torch.equal(alone[0], first[b])
    # fewer points: other bins, other tiles, the same values
    assert torch.equal(li_fusion.image_head_at_points(maps, packed, xy[:, :100].contiguous()), first[:, :, :100])


@pytest.mark.parametrize("name", ["four", "real"])
def test_graph_capture_and_replay_on_new_contents(hiplib, name):
    from epnet_amd import li_fusion
    cfg, head_dev, packed, maps, xy = _setup(name, n=257)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        li_fusion.image_head_at_points(maps, packed, xy)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = li_fusion.image_head_at_points(maps, packed, xy)
    new_maps = [m.to(DEV) for m in cases.make_maps(cfg, seed=21)]
    new_xy = cases.make_xy(cfg, n=257, seed=22).to(DEV)
    for m, v in zip(maps, new_maps):
        m.copy_(v)
    xy.copy_(new_xy)
    graph.replay()
    torch.cuda.synchronize()
    want = li_fusion.image_head_at_points(new_maps, packed, new_xy)
    assert torch.equal(out, want) and out.abs().max().item() > 0.05


@pytest.mark.parametrize("name", ["two", "real"])
def test_workspace_bounds(hiplib, name):
    """nothing is written outside workspace_bytes; one byte less is refused before anything is launched"""
    from epnet_amd import _lib, li_fusion, pointnet2_cuda
    cfg, head_dev, packed, maps, xy = _setup(name, n=257)
    b, n, h, w, q = xy.shape[0], 257, cfg["h"], cfg["w"], cfg["q"]
    want = li_fusion.image_head_at_points(maps, packed, xy)
    ws_bytes = pointnet2_cuda.image_head_points_workspace_bytes(b, n, h, w, cfg["chans"], cfg["kernels"], cfg["reduce"], q)
    assert ws_bytes > 0 and ws_bytes % 256 == 0
    guard = 4096
    raw = torch.full((guard + ws_bytes + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    out_raw = torch.full((guard + b * q * n * 4 + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    out = out_raw[guard:guard + b * q * n * 4].view(torch.float32).view(b, q, n)
    args = (b, n, h, w, cfg["chans"], cfg["kernels"], cfg["reduce"], maps, packed.weights, q, packed.wf, packed.shift, xy, True, out)
    with pytest.raises(_lib.EpnetError, match="workspace"):
        pointnet2_cuda.image_head_points_wrapper(*args, workspace=raw[guard:guard + ws_bytes - 1])
    torch.cuda.synchronize()
    assert (raw == 0xA5).all() and (out_raw == 0xA5).all()                   # nothing was launched
    pointnet2_cuda.image_head_points_wrapper(*args, workspace=raw[guard:guard + ws_bytes])
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    for buf, size in ((raw, ws_bytes), (out_raw, b * q * n * 4)):
        assert (buf[:guard] == 0xA5).all() and (buf[guard + size:] == 0xA5).all()


# ---- the backbone ------------------------------------------------------------------------------------------------------------------
def _small_models():
    from epnet_amd.rpn_backbone import Pointnet2MSG
    from test_two_stream import load_small, small_config
    dense, fx = load_small("hip", DEV)
    points = Pointnet2MSG(input_channels=0, config=small_config(), sampler="hip", image_head="points").to(DEV)
    assert list(points.state_dict().keys()) == list(dense.state_dict().keys())
    points.load_state_dict(dense.state_dict())
    inputs = tuple(torch.from_numpy(fx[k]).to(DEV) for k in ("pts", "image", "xy"))
    return dense, points, inputs, torch.from_numpy(fx["probe"]).to(DEV)


def _count_calls(module):
    calls = []
    handle = module.register_forward_hook(lambda mod, args, out: calls.append(tuple(out.shape)))
    return calls, handle


def test_backbone_takes_the_points_head_in_eval_mode_without_grad(hiplib):
    from epnet_amd import li_fusion
    dense, points, (pts, image, xy), _ = _small_models()
    points.eval()
    caught, maps = [], []
    points.final_fusion_img_point.register_forward_hook(lambda mod, args, out: caught.append(args[1]))
    for block in points.Img_Block:
        block.register_forward_hook(lambda mod, args, out: maps.append(out))
    conv_calls, _ = _count_calls(points.image_fusion_conv)
    xy_run = xy.clone()
    with torch.no_grad():
        _, feats = points(pts.clone(), image.clone(), xy_run)       # xy_run is normalised in place
    assert conv_calls == [] and len(caught) == 1 and len(maps) == 4
    assert points._packed_head is not None
    packed = li_fusion.pack_image_head(points.DeConv, points.image_fusion_conv, points.image_fusion_bn)
    assert torch.equal(caught[0], li_fusion.image_head_at_points(maps, packed, xy_run))
    assert tuple(caught[0].shape) == (2, 4, 1024) and caught[0].abs().max().item() > 0
    # the same pack serves the next call; and the whole model stays close to the dense one (the final fusion's two convolutions and
    # batch norms sit behind the head: ten times the float tolerance)
    before = points._packed_head
    with torch.no_grad():
        _, again = points(pts.clone(), image.clone(), xy.clone())
        _, want = dense.eval()(pts.clone(), image.clone(), xy.clone())
    assert points._packed_head is before and torch.equal(again, feats)
    torch.testing.assert_close(feats, want, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("mode", ["train", "eval with grad"])
def test_backbone_runs_the_dense_lines_when_a_gradient_is_needed(hiplib, mode):
    """bitwise the "dense" model: output and gradients (the project's deterministic gradients, so that two runs of the same
    code can be compared bit for bit)"""
    dense, points, (pts, image, xy), probe = _small_models()
    prev = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        results = []
        for model in (dense, points):
            model.train(mode == "train")
            conv_calls, handle = _count_calls(model.image_fusion_conv)
            img = image.clone().requires_grad_(True)
            _, feats = model(pts.clone(), img, xy.clone())
            (feats * probe).sum().backward()
            handle.remove()
            assert conv_calls == [(2, 4, 32, 64)]
            grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
            results.append((feats.detach(), img.grad.clone(), grads))
    finally:
        torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])
    (f_dense, gi_dense, gp_dense), (f_points, gi_points, gp_points) = results
    assert points._packed_head is None
    assert torch.equal(f_points, f_dense) and torch.equal(gi_points, gi_dense)
    assert sorted(gp_points) == sorted(gp_dense) and len(gp_dense) >= 10
    for k in gp_dense:
        assert torch.equal(gp_points[k], gp_dense[k]), k

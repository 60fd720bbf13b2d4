"""The RPN inputs from raw scans on the GPU (epnet_amd/scan_layer.py over csrc/scan.hip).

Bound: the kernel is BIT-EQUAL to the numpy restatement (tests/scan_restate.py, held to the reference in test_scan_prepare.py) in
every output -- the contract fixes every float32 operation and its order, and the selection is integer work. The seeded scenes
(scan_restate.scene_with) hold an exact number of valid and far points, so each case of the selection table is hit on purpose.
Image normalisation: bit-equal to the float64 numpy expression rounded once."""
import numpy as np
import pytest
import torch

import scan_restate as rs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F = np.float32
OUTS = ("pts_rect", "pts_intensity", "pts_origin_xy", "pts_input", "choice", "scene_info")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().cpu().numpy()


class Batch:
    """scenes of one length p: (pts (p,4), num_raw, V2C, R0, P2, shape) each, plus keys (b,p) and slot_perm (b,n) or None"""

    def __init__(self, scenes, n, keys, slot_perm):
        self.n, self.keys, self.slot_perm = n, np.ascontiguousarray(keys, np.int32), slot_perm
        self.pts = np.stack([s[0] for s in scenes]).astype(F)
        self.num_raw = np.array([s[1] for s in scenes], np.int32)
        self.V2C, self.R0, self.P2 = (np.stack([s[k] for s in scenes]).astype(F) for k in (2, 3, 4))
        self.shape = np.stack([s[5] for s in scenes]).astype(np.int32)

    def want(self, **kw):
        return rs.prepare_batch(self.pts, self.num_raw, self.V2C, self.R0, self.P2, self.shape, self.keys, self.slot_perm, self.n, **kw)

    def tensors(self):
        return [dev(a) for a in (self.pts, self.num_raw, self.V2C, self.R0, self.P2, self.shape)]

    def tables(self):
        return {"keys": dev(self.keys), "slot_perm": None if self.slot_perm is None else dev(self.slot_perm)}

    def run(self, cfg=None):
        from epnet_amd import scan_layer
        out = scan_layer.prepare_scans(*self.tensors(), self.tables(), npoints=self.n, cfg=cfg)
        got = {k: host(v) for k, v in out.items()}
        got["pts_intensity"] = got.pop("pts_features").reshape(len(self.pts), self.n)
        return got


def differences(got, want, keys=OUTS):
    bad = []
    for k in keys:
        if got[k].dtype != want[k].dtype or got[k].shape != want[k].shape:
            bad.append((k, got[k].dtype, got[k].shape, want[k].dtype, want[k].shape))
        elif got[k].tobytes() != want[k].tobytes():
            a, b = got[k].reshape(-1).view(np.int32), want[k].reshape(-1).view(np.int32)
            where = np.nonzero(a != b)[0]
            bad.append((k, len(where), np.unravel_index(where[:4], got[k].shape), got[k].reshape(-1)[where[:4]], want[k].reshape(-1)[where[:4]]))
    return bad


def scene(p, num_raw, far, near, seed):
    pts, V2C, R0, P2, shape = rs.scene_with(p, num_raw, far, near, seed)
    return pts, num_raw, V2C, R0, P2, shape


def draws(b, p, n, seed, perm=True):
    rng = np.random.default_rng(seed)
    keys = rng.integers(-2 ** 31, 2 ** 31, (b, p)).astype(np.int32)
    return keys, (np.stack([rng.permutation(n) for _ in range(b)]).astype(np.int32) if perm else None)


def counts_for(p, n, rng):
    """(num_raw, far, near) that fit p points and spread over the cases for n rows"""
    num_raw = int(rng.integers(0, p + 1))
    kind = int(rng.integers(0, 6))
    v = min(num_raw, {0: n + 1 + int(rng.integers(0, 2 * n + 2)), 1: n, 2: (n + 1) // 2 + int(rng.integers(0, max(n // 2, 1))),
                      3: int(rng.integers(1, max(n // 2, 2))), 4: 0, 5: 3 * n + 3}[kind])
    far = min(v, n + 1 + int(rng.integers(0, n + 1))) if kind == 5 else int(rng.integers(0, min(v, n) + 1))
    return num_raw, far, v - far


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------
def test_kernel_on_the_reference_scenes(hiplib):
    for i, s in enumerate(rs.fixture()):
        n = int(s["n"])
        one = Batch([(s["pts"], len(s["pts"]), s["V2C"], s["R0"], s["P2"], s["img_shape"])], n, s["keys"][None], s["slot_perm"][None])
        got = one.run()
        assert not differences(got, one.want()), i
        assert np.array_equal(got["choice"][0], s["ref_choice"])


# ---- shapes -----------------------------------------------------------------------------------------------------------------------------
P_SIZES, N_SIZES = (1, 63, 64, 65, 1023, 1025, 2049, 4099), (1, 16, 64, 1000)


@pytest.mark.parametrize("p", P_SIZES)
def test_shapes_against_the_restatement(hiplib, p):
    seen = set()
    for n in N_SIZES:
        rng = np.random.default_rng(p * 7919 + n)
        b = 6
        scenes = [scene(p, *counts_for(p, n, rng), seed=p * 131 + n * 17 + k) for k in range(b)]
        keys, perm = draws(b, p, n, seed=p + n, perm=n != 16)            # n == 16: without a shuffle
        keys[:, ::3] = keys[:, :1]                                        # many equal keys
        batch = Batch(scenes, n, keys, perm)
        want = batch.want()
        bad = differences(batch.run(), want)
        assert not bad, (p, n, bad)
        seen |= set(want["scene_info"][:, 3].tolist())
    assert 4 in seen and len(seen) >= (2 if p == 1 else 3), seen


def test_num_raw_of_0_1_p_minus_1_and_p_in_one_batch(hiplib):
    p, n = 2049, 64
    scenes = [scene(p, 0, 0, 0, 1), scene(p, 1, 0, 1, 2), scene(p, p - 1, 30, 200, 3), scene(p, p, 30, 200, 4)]
    # beyond the count every scene_with row looks valid; a count above p or below 0 is clamped
    more = [scene(p, p, 5, 40, 5), scene(p, 0, 0, 0, 6)]
    keys, perm = draws(6, p, n, seed=9)
    batch = Batch(scenes + more, n, keys, perm)
    batch.num_raw[4], batch.num_raw[5] = p + 1000, -3
    want = batch.want()
    assert want["scene_info"][:, 0].tolist() == [0, 1, p - 1, p, p, 0] and want["scene_info"][:, 3].tolist() == [4, 3, 0, 0, 2, 4]
    assert not differences(batch.run(), want)


CASE_COUNTS = {0: (4, 30), 5: (20, 5), 1: (6, 10), 2: (3, 9), 3: (1, 2), 4: (0, 0)}      # (far, near) for n = 16


@pytest.mark.parametrize("b", (1, 2, 257))
def test_all_cases_in_one_batch(hiplib, b):
    p, n = 130, 16
    order = [0, 5, 1, 2, 3, 4]
    scenes = [scene(p, p - (k % 3), *CASE_COUNTS[order[(k + b) % 6]], seed=100 + k) for k in range(b)]
    keys, perm = draws(b, p, n, seed=b)
    batch = Batch(scenes, n, keys, perm)
    want = batch.want()
    assert set(want["scene_info"][:, 3].tolist()) == (set(range(6)) if b >= 6 else {order[(k + b) % 6] for k in range(b)})
    assert not differences(batch.run(), want)


def test_boundaries_between_the_cases(hiplib):
    """F == n and F == n + 1; V == n - 1, V == n and V == n / 2 (and one below); V == 1 and V == 3 with n = 64"""
    p, n = 1025, 64
    counts = [(64, 100), (65, 100), (64, 0), (65, 0), (10, 53), (10, 54), (10, 55), (2, 30), (2, 29), (0, 1), (1, 0), (1, 2), (0, 3)]
    scenes = [scene(p, p, far, near, seed=300 + k) for k, (far, near) in enumerate(counts)]
    keys, perm = draws(len(counts), p, n, seed=77)
    batch = Batch(scenes, n, keys, perm)
    want = batch.want()
    assert want["scene_info"][:, 3].tolist() == [0, 5, 1, 5, 2, 1, 0, 2, 3, 3, 3, 3, 3]
    assert want["scene_info"][:, 4:6].tolist()[:4] == [[0, 1], [64, 0], [0, 1], [64, 0]]
    assert want["scene_info"][7:, 4:6].tolist() == [[32, 1], [2, 2], [0, 64], [0, 64], [1, 21], [1, 21]]
    assert not differences(batch.run(), want)


@pytest.mark.parametrize("kind", ("from 0..3", "all equal", "top byte only", "low byte only", "second byte only"))
def test_key_patterns(hiplib, kind):
    p, n, b = 4099, 1000, 3
    rng = np.random.default_rng(len(kind))
    base = int(rng.integers(0, 2 ** 32))
    raw = {"from 0..3": rng.integers(0, 4, (b, p)), "all equal": np.full((b, p), base),
           "top byte only": (base & 0x00FFFFFF) | (rng.integers(0, 256, (b, p)) << 24),
           "low byte only": (base & 0xFFFFFF00) | rng.integers(0, 256, (b, p)),
           "second byte only": (base & 0xFF00FFFF) | (rng.integers(0, 256, (b, p)) << 16)}[kind]
    keys = raw.astype(np.uint32).view(np.int32)
    scenes = [scene(p, p, 300, 2500, 400), scene(p, p - 7, 1200, 900, 401), scene(p, p, 0, 700, 402)]       # cases 0, 5, 2
    batch = Batch(scenes, n, keys, draws(b, p, n, seed=5)[1])
    want = batch.want()
    assert want["scene_info"][:, 3].tolist() == [0, 5, 2]
    assert not differences(batch.run(), want)


def test_known_answers_at_the_boundaries(hiplib):
    """the decisive rows of test_scan_prepare.toy_points through the kernel, with and without the scope"""
    from types import SimpleNamespace
    from test_scan_prepare import EYE_R0, EYE_V2C, TOY_P2, TOY_SHAPE, toy_scene
    pts, rows = toy_scene()
    p, n = 64, len(rows)
    padded = np.zeros((p, 4), F)
    padded[:len(pts)] = pts
    keys = np.zeros((1, p), np.int32)
    for reduce, col in ((True, 2), (False, 3)):
        cfg = SimpleNamespace(PC_REDUCE_BY_RANGE=reduce, PC_AREA_SCOPE=rs.SCOPE, RPN=SimpleNamespace(USE_INTENSITY=True))
        batch = Batch([(padded, len(pts), EYE_V2C, EYE_R0, TOY_P2, TOY_SHAPE)], n, keys, None)
        got = batch.run(cfg)
        assert not differences(got, batch.want(reduce_by_range=reduce))
        valid = sorted(set(got["choice"][0].tolist()))
        assert valid == [k for k, r in enumerate(rows) if r[col]], reduce


def test_without_pts_input_and_without_intensity(hiplib):
    from types import SimpleNamespace
    from epnet_amd import scan_layer
    p, n = 1023, 64
    batch = Batch([scene(p, p, 20, 300, 500), scene(p, p, 0, 40, 501)], n, *draws(2, p, n, seed=3))
    cfg = SimpleNamespace(PC_REDUCE_BY_RANGE=True, PC_AREA_SCOPE=rs.SCOPE.tolist(), RPN=SimpleNamespace(USE_INTENSITY=False))
    out = scan_layer.prepare_scans(*batch.tensors(), batch.tables(), npoints=n, cfg=cfg)
    assert out["pts_input"] is out["pts_rect"]                                  # :359-362
    got = {k: host(v) for k, v in out.items()}
    got["pts_intensity"] = got.pop("pts_features").reshape(2, n)
    assert not differences(got, batch.want(), ("pts_rect", "pts_intensity", "pts_origin_xy", "choice", "scene_info"))


def test_full_size(hiplib):
    """2 x 131072 raw points -> 16384: synthetic full-azimuth scans, 64 tiles per scene"""
    from epnet_amd import synth
    b, p, n = 2, 131072, 16384
    scans = [synth.lidar_scan(p - 5000 * k, seed=40 + k).numpy() for k in range(b)]
    cal = [tuple(t.numpy() for t in synth.calibration(k)) for k in range(b)]
    pts = np.zeros((b, p, 4), F)
    for k, s in enumerate(scans):
        pts[k, :len(s)] = s
    scenes = [(pts[k], len(scans[k])) + cal[k] for k in range(b)]
    batch = Batch(scenes, n, *draws(b, p, n, seed=12))
    want = batch.want()
    assert want["scene_info"][:, 3].tolist() == [0, 0] and (want["scene_info"][:, 2] > 0).all(), want["scene_info"]
    assert not differences(batch.run(), want)


# ---- limits -----------------------------------------------------------------------------------------------------------------------------
def test_limits(hiplib):
    from epnet_amd import _lib, scan_layer
    z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=DEV)  # noqa: E731
    args = lambda b, p: (z((b, p, 4)), z((b,), torch.int32), z((b, 3, 4)), z((b, 3, 3)), z((b, 3, 4)), z((b, 2), torch.int32))  # noqa: E731
    with pytest.raises(_lib.EpnetError, match="supported range"):
        scan_layer.prepare_scans(*args(1, 64), {"keys": z((1, 64), torch.int32), "slot_perm": None}, npoints=65537)
    with pytest.raises(_lib.EpnetError, match="supported range"):
        scan_layer.prepare_scans(*args(65536, 1), {"keys": z((65536, 1), torch.int32), "slot_perm": None}, npoints=1)
    out = scan_layer.prepare_scans(*args(65535, 1), {"keys": z((65535, 1), torch.int32), "slot_perm": None}, npoints=1)   # the largest batch
    assert bool((out["choice"] == -1).all()) and bool((out["scene_info"][:, 3] == 4).all())
    out = scan_layer.prepare_scans(*args(0, 64), {"keys": z((0, 64), torch.int32), "slot_perm": None}, npoints=16)
    assert out["pts_rect"].shape == (0, 16, 3)
    with pytest.raises(RuntimeError, match="slot_perm must be"):
        scan_layer.prepare_scans(*args(1, 64), {"keys": z((1, 64), torch.int32), "slot_perm": z((1, 8), torch.int32)}, npoints=16)


# ---- reproducibility, no synchronisation -----------------------------------------------------------------------------------------------
def mixed_batch(seed, b=4, p=4099, n=1000):
    counts = [(300, 2500), (1200, 900), (0, 700), (100, 200)]
    scenes = [scene(p, p - k, *counts[k % 4], seed=seed * 10 + k) for k in range(b)]
    return Batch(scenes, n, *draws(b, p, n, seed=seed))


def test_runs_are_bit_equal_and_need_no_sync(hiplib):
    """twice on one stream, once on a side stream, and once with every synchronising call an error"""
    from epnet_amd import scan_layer
    batch = mixed_batch(1)
    tensors, tables = batch.tensors(), batch.tables()
    img = torch.randint(0, 256, (2, 375, 1242, 3), dtype=torch.uint8, device=DEV)
    a = scan_layer.prepare_scans(*tensors, tables, npoints=batch.n)
    b = scan_layer.prepare_scans(*tensors, tables, npoints=batch.n)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = scan_layer.prepare_scans(*tensors, tables, npoints=batch.n)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        drawn = scan_layer.draw_scan_tables(4, 4099, batch.n, torch.Generator(device=DEV).manual_seed(3), DEV)
        d = scan_layer.prepare_scans(*tensors, tables, npoints=batch.n)
        scan_layer.prepare_scans(*tensors, drawn, npoints=batch.n)
        im = scan_layer.normalise_images(img)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for k in a:
        assert host(a[k]).tobytes() == host(b[k]).tobytes() == host(c[k]).tobytes() == host(d[k]).tobytes(), k
    assert im.shape == (2, 3, 384, 1280) and sorted(drawn["slot_perm"][0].tolist()) == list(range(batch.n))
    assert not differences({**{k: host(v) for k, v in a.items()}, "pts_intensity": host(a["pts_features"]).reshape(4, -1)}, batch.want())


def test_scans_targets_and_loss_in_one_graph(hiplib):
    """prepare_scans + augment_and_label + rpn_loss forward and backward captured in ONE torch.cuda.graph (the capture fails on
    any synchronisation with the host), replayed after in-place copies of new scans, counts and tables: equal to eager"""
    from epnet_amd import loss_utils, rpn_target_layer as rtl, scan_layer, synth
    first, second = mixed_batch(2), mixed_batch(3)
    b, n, c = 4, first.n, 76
    names = ("pts", "num_raw", "V2C", "R0", "P2", "shape")
    static = dict(zip(names, first.tensors()))
    static.update(first.tables())
    gt = torch.stack([synth.object_boxes(6, seed=k) for k in range(b)]).to(DEV)
    alpha = torch.zeros((b, 6), device=DEV)
    aug = rtl.draw_augmentation(b, generator=torch.Generator(device=DEV).manual_seed(4), device=DEV)
    g = torch.Generator(device=DEV).manual_seed(8)
    cls_in = torch.randn((b, n, 1), generator=g, device=DEV).requires_grad_(True)
    reg_in = torch.randn((b, n, c), generator=g, device=DEV).requires_grad_(True)
    cfg = loss_utils.default_cfg()

    def step():
        out = scan_layer.prepare_scans(*[static[k] for k in names], {"keys": static["keys"], "slot_perm": static["slot_perm"]}, npoints=n)
        pts, gt_aug, cls_label, reg_label = rtl.augment_and_label(out["pts_rect"], gt, alpha, aug)
        res = loss_utils.rpn_loss(cls_in, reg_in, cls_label, reg_label, cfg)
        grads = torch.autograd.grad(res.loss, [cls_in, reg_in])
        return [out["pts_rect"], out["pts_input"], out["pts_origin_xy"], out["choice"], out["scene_info"], pts, cls_label, res.loss, res.terms] + list(grads)
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
    assert all(torch.equal(x, y) for x, y in zip(eager_first, captured))
    with torch.no_grad():
        for key, value in zip(names, second.tensors()):
            static[key].copy_(value)
        for key, value in second.tables().items():
            static[key].copy_(value)
    graph.replay()
    torch.cuda.synchronize()
    eager_second = step()
    assert all(torch.equal(x, y) for x, y in zip(eager_second, captured))
    assert not torch.equal(eager_second[0], eager_first[0]) and not torch.equal(eager_second[3], eager_first[3])
    assert host(captured[3]).tobytes() == second.want()["choice"].tobytes()


# ---- image normalisation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw_in,hw_out,per_scene", [((375, 1242), (384, 1280), False), ((5, 7), (8, 16), False), ((5, 7), (6, 9), False),
                                                    ((376, 1242), (384, 1280), True), ((400, 1300), (384, 1280), False), ((9, 21), (8, 16), True)])
def test_image_normalisation(hiplib, hw_in, hw_out, per_scene):
    from epnet_amd import scan_layer
    rng = np.random.default_rng(hw_in[0] * hw_out[1])
    b = 3
    img = rng.integers(0, 256, (b,) + hw_in + (3,)).astype(np.uint8)
    img[0, 0, :256 if hw_in[1] >= 256 else hw_in[1], 0] = np.arange(256)[:hw_in[1]]          # every value of a byte where it fits
    shapes = None
    if per_scene:
        shapes = np.array([[hw_in[0], hw_in[1]], [hw_in[0] - 1, hw_in[1] - 2], [max(hw_in[0] - 6, 1), hw_in[1] // 2]], np.int32)
    got = host(scan_layer.normalise_images(dev(img), None if shapes is None else dev(shapes), out_hw=hw_out))
    want = rs.image_normalise(img, shapes, hw_out)
    assert got.dtype == F and got.shape == want.shape and got.tobytes() == want.tobytes()
    h, w = min(hw_in[0], hw_out[0]), min(hw_in[1], hw_out[1])
    assert got[0, :, :h, :w].all() and not got[0, :, h:].any() and not got[0, :, :, w:].any()      # scene 0: the image, then zero padding

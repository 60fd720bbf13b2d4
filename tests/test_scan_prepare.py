"""The RPN inputs from raw scans without a GPU: the numpy restatement (tests/scan_restate.py) against what the reference's own
get_rpn_with_li_fusion returned (tests/golden/scan_prepare.npz), known answers at the decision boundaries, the cases the
reference raises on, the distribution of the selection, the library's exports and limits, and the Python surface.

Bounds against the fixture: ``choice`` EQUAL in every row (the fixture holds no point within 1e-2 px of an image edge or 1e-3 m
of depth 0, a scope face or z = 40). Each float column is held to a float64 evaluation of the same formulas: the restatement may
be no farther from it than twice the reference's own largest distance in that column plus one float32 ulp of the column's
largest magnitude -- the reference's BLAS sums four to seven roundings in an order that is not known, hence the factor 2 (as in
test_two_stream.py)."""
import ctypes

import numpy as np
import pytest
import torch

import scan_restate as rs

F = np.float32
SCENES = rs.fixture()


def test_fixture_covers_what_it_should():
    infos = [rs.prepare(s["pts"], len(s["pts"]), s["V2C"], s["R0"], s["P2"], s["img_shape"], s["keys"], s["slot_perm"], int(s["n"]))["scene_info"]
             for s in SCENES]
    cases = [(int(i[3]), int(i[2]) > 0) for i in infos]
    assert (0, False) in cases and (0, True) in cases and any(c == 1 for c, _ in cases) and any(c == 2 for c, _ in cases)
    assert any(2 * int(i[1]) == int(s["n"]) for i, s in zip(infos, SCENES))                       # V == n / 2
    assert all(len(s["pts"]) <= 4096 and int(s["n"]) <= 1024 for s in SCENES)
    for s in SCENES:                                                                                 # equal keys among the rows
        assert len(np.unique(s["keys"])) < len(s["keys"])
        rect, uv, depth = rs.transform64(s["pts"], s["V2C"], s["R0"], s["P2"])
        h, w = (int(v) for v in s["img_shape"])
        assert np.minimum.reduce([np.abs(uv[:, 0]), np.abs(uv[:, 0] - w), np.abs(uv[:, 1]), np.abs(uv[:, 1] - h)]).min() >= 1e-2
        assert np.abs(depth).min() >= 1e-3 and np.abs(rect[:, 2] - 40.0).min() >= 1e-3
        assert all(np.abs(rect[:, j] - rs.SCOPE[j, e]).min() >= 1e-3 for j in range(3) for e in range(2))


@pytest.mark.parametrize("i", range(len(SCENES)))
def test_restatement_against_the_reference(i):
    s = SCENES[i]
    n = int(s["n"])
    mine = rs.prepare(s["pts"], len(s["pts"]), s["V2C"], s["R0"], s["P2"], s["img_shape"], s["keys"], s["slot_perm"], n)
    assert np.array_equal(mine["choice"], s["ref_choice"])
    rect64, uv64, _ = rs.transform64(s["pts"], s["V2C"], s["R0"], s["P2"])
    rows = s["ref_choice"]
    exact = {"pts_rect": rect64[rows], "pts_origin_xy": uv64[rows], "pts_intensity": s["pts"][rows, 3].astype(np.float64)[:, None] - 0.5}
    ref = {"pts_rect": s["ref_pts_rect"], "pts_origin_xy": s["ref_pts_origin_xy"], "pts_intensity": s["ref_pts_features"].reshape(n, 1)}
    got = {"pts_rect": mine["pts_rect"], "pts_origin_xy": mine["pts_origin_xy"], "pts_intensity": mine["pts_intensity"].reshape(n, 1)}
    bad = []
    for name in ("pts_rect", "pts_origin_xy", "pts_intensity"):
        assert ref[name].dtype == F and got[name].dtype == F
        for c in range(exact[name].shape[1]):
            e_ref = float(np.abs(ref[name][:, c].astype(np.float64) - exact[name][:, c]).max())
            e_mine = float(np.abs(got[name][:, c].astype(np.float64) - exact[name][:, c]).max())
            ulp = float(np.spacing(F(np.abs(exact[name][:, c]).max())))
            print("scene %d %s[%d]: reference %.3e, restatement %.3e, ulp %.3e" % (i, name, c, e_ref, e_mine, ulp))
            if not e_mine <= 2 * e_ref + ulp:
                bad.append((name, c, e_ref, e_mine, ulp))
    assert not bad, bad
    assert np.array_equal(mine["pts_input"][:, :3], mine["pts_rect"]) and np.array_equal(mine["pts_input"][:, 3], mine["pts_intensity"])
    assert np.array_equal(s["ref_pts_input"][:, :3], s["ref_pts_rect"])


# ---- known answers at the boundaries ------------------------------------------------------------------------------------------------
# u = X / Z + 2, v = Y / Z + 1, depth = X + Z; the rectified frame is the velodyne frame
EYE_V2C = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(F)
EYE_R0 = np.eye(3, dtype=F)
TOY_P2 = np.array([[1, 0, 2, 0], [0, 1, 1, 0], [1, 0, 1, 0]], F)
TOY_SHAPE = np.array([4, 8], np.int32)


def toy_points():
    """(name, row, valid with the scope, valid without)"""
    z704 = F(70.4)
    return [("plain", [1.0, 0.5, 2.0, 0.3], True, True),
            ("z == (float)70.4, above the double 70.4", [0.0, 0.0, z704, 0.1], False, True),
            ("z one ulp below (float)70.4", [0.0, 0.0, np.nextafter(z704, F(0)), 0.1], True, True),
            ("NaN x", [np.nan, 0.0, 2.0, 0.1], False, False),
            ("NaN intensity only", [1.0, 0.5, 2.0, np.nan], True, True),
            ("u == w", [12.0, 0.0, 2.0, 0.1], False, False),
            ("u one ulp below w", [np.nextafter(F(12.0), F(0)), 0.0, 2.0, 0.1], True, True),
            ("u == 0", [-2.0, 0.0, 1.0, 0.1], False, False),          # u = 0 is in the image, depth = -1 is not
            ("depth == 0", [-2.0, 0.0, 2.0, 0.1], True, True),        # u = 1
            ("depth below 0", [np.nextafter(F(-2.0), F(-3)), 0.0, 2.0, 0.1], False, False),
            ("v == h", [0.0, 6.0, 2.0, 0.1], False, False),
            ("y == 3, the scope's face", [0.0, 3.0, 2.0, 0.1], True, True),   # v = 2.5
            ("y above the scope", [0.0, np.nextafter(F(3.0), F(4)), 2.0, 0.1], False, True),
            ("z == 0", [0.0, 0.0, 0.0, 0.1], False, False),           # 0 / 0
            ("z == 40: far", [0.0, 0.0, 40.0, 0.1], True, True)]


def toy_scene():
    rows = toy_points()
    return np.array([r[1] for r in rows], F), rows


def test_known_answers_of_the_validity_rule():
    pts, rows = toy_scene()
    for reduce, col in ((True, 2), (False, 3)):
        rect, uv, valid, near = rs.classify(pts, len(pts), EYE_V2C, EYE_R0, TOY_P2, TOY_SHAPE, reduce_by_range=reduce)
        for k, r in enumerate(rows):
            assert bool(valid[k]) == r[col], (r[0], reduce)
    assert np.array_equal(rect[0], pts[0, :3]) and uv[0].tolist() == [2.5, 1.25]
    assert not near[len(rows) - 1] and valid[len(rows) - 1] and near[0]
    # rows at or beyond num_raw are invalid, num_raw is clamped
    assert not rs.classify(pts, 0, EYE_V2C, EYE_R0, TOY_P2, TOY_SHAPE)[2].any()
    assert rs.classify(pts, 1, EYE_V2C, EYE_R0, TOY_P2, TOY_SHAPE)[2].sum() == 1
    assert np.array_equal(rs.classify(pts, 10 ** 6, EYE_V2C, EYE_R0, TOY_P2, TOY_SHAPE, reduce_by_range=False)[2], valid)
    assert not rs.classify(pts, -5, EYE_V2C, EYE_R0, TOY_P2, TOY_SHAPE)[2].any()


def test_known_answers_of_the_selection():
    valid = np.ones(8, bool)
    near = np.array([1, 1, 1, 0, 1, 1, 1, 0], bool)                        # far: rows 3 and 7
    top = np.int32(-2 ** 31)                                                # 0x80000000: the LARGEST key when compared unsigned
    keys = np.array([5, top, 5, 0, 5, -1, 1, 0], np.int32)
    # case 0, n = 5: far (3, 7), then the 3 smallest near: key 1 (row 6), then the tie at 5 goes to rows 0 and 2, not 4
    L, info = rs.select(valid, near, keys, 5)
    assert L.tolist() == [3, 7, 0, 2, 6] and info == (8, 2, 0, 3, 1)
    L, info = rs.select(valid, near, keys, 7)                               # 5 near: all three 5s and the top-bit key, not 0xffffffff
    assert L.tolist() == [3, 7, 0, 1, 2, 4, 6] and info == (8, 2, 0, 5, 1)
    L, info = rs.select(valid, near, keys, 2)                               # F == n: no near point
    assert L.tolist() == [3, 7] and info == (8, 2, 0, 0, 1)
    L, info = rs.select(valid, near, keys, 1)                               # F == n + 1: case 5, the smallest far key, tie to row 3
    assert L.tolist() == [3] and info == (8, 2, 5, 1, 0)
    L, info = rs.select(valid, near, keys, 8)                               # case 1
    assert L.tolist() == list(range(8)) and info == (8, 2, 1, 0, 1)
    L, info = rs.select(valid, near, keys, 11)                              # case 2: all, then the 3 smallest of all
    assert L.tolist() == list(range(8)) + [3, 6, 7] and info == (8, 2, 2, 3, 1)
    L, info = rs.select(valid, near, keys, 16)                              # V == n / 2: case 2 with r = V
    assert L.tolist() == list(range(8)) * 2 and info == (8, 2, 2, 8, 1)


def test_cases_the_reference_raises_on():
    valid = np.array([0, 1, 0, 1, 1, 0], bool)
    keys = np.array([0, 9, 0, 3, 3, 0], np.int32)
    L, info = rs.select(valid, valid & False, keys, 8)                      # case 3: V = 3 < n / 2: two copies, then the 2 smallest
    assert L.tolist() == [1, 3, 4, 1, 3, 4, 3, 4] and info == (3, 3, 3, 2, 2)
    L, info = rs.select(valid, valid, keys, 9)
    assert L.tolist() == [1, 3, 4] * 3 and info == (3, 0, 3, 0, 3)
    L, info = rs.select(valid & False, valid & False, keys, 4)              # case 4
    assert L is None and info == (0, 0, 4, 0, 0)
    pts, V2C, R0, P2, shape = rs.scene_with(64, 60, 0, 0, seed=3)
    out = rs.prepare(pts, 60, V2C, R0, P2, shape, np.zeros(64, np.int32), None, 16)
    assert not out["pts_rect"].any() and not out["pts_input"].any() and not out["pts_origin_xy"].any() and (out["choice"] == -1).all()
    assert out["scene_info"].tolist() == [60, 0, 0, 4, 0, 0]
    pts, V2C, R0, P2, shape = rs.scene_with(64, 64, 20, 5, seed=4)          # case 5: 20 far points for 16 rows
    keys = np.arange(64, dtype=np.int32)[::-1].copy()
    out = rs.prepare(pts, 64, V2C, R0, P2, shape, keys, None, 16)
    assert out["scene_info"].tolist() == [64, 25, 20, 5, 16, 0]
    rect = rs.transform(pts, V2C, R0, P2)[0]
    assert (rect[out["choice"], 2] >= 40).all() and (np.diff(out["choice"]) > 0).all()
    assert np.array_equal(out["pts_rect"], rect[out["choice"]]) and np.array_equal(out["pts_intensity"], pts[out["choice"], 3] - F(0.5))


def test_selection_has_the_reference_distribution():
    """4000 scenes of p = 64, n = 16 with uniform keys: every far point is always chosen, every near point with the share
    (n - F) / near that a uniform subset gives, within 4 sigma of a binomial share of 4000"""
    rng = np.random.default_rng(17)
    p, n, scenes = 64, 16, 4000
    valid = np.zeros(p, bool)
    valid[rng.permutation(p)[:40]] = True
    far = np.zeros(p, bool)
    far[np.nonzero(valid)[0][:6]] = True
    near = valid & ~far
    count = np.zeros(p, np.int64)
    for _ in range(scenes):
        keys = rng.integers(-2 ** 31, 2 ** 31, p).astype(np.int32)
        L, info = rs.select(valid, near, keys, n)
        assert info == (40, 6, 0, 10, 1) and len(set(L.tolist())) == n
        count[L] += 1
    assert (count[far] == scenes).all() and not count[~valid].any()
    share = (n - 6) / 34.0
    sigma = np.sqrt(share * (1 - share) / scenes)
    got = count[near] / scenes
    print("near shares: %.4f .. %.4f around %.4f, 4 sigma = %.4f" % (got.min(), got.max(), share, 4 * sigma))
    assert np.abs(got - share).max() <= 4 * sigma


def test_image_restatement_is_the_reference_expression():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (1, 5, 7, 3)).astype(np.uint8)
    out = rs.image_normalise(img, None, (8, 16))
    im = img[0].astype(np.float64) / 255.0
    im -= [0.485, 0.456, 0.406]
    im /= [0.229, 0.224, 0.225]
    back = np.zeros((8, 16, 3))
    back[:5, :7] = im
    assert out.dtype == F and np.array_equal(out[0], back.astype(F).transpose(2, 0, 1))


# ---- the library and the Python surface -----------------------------------------------------------------------------------------------
def test_library_exports_and_limits_without_a_gpu(hiplib):
    for name in ("epnet_scan_prepare", "epnet_scan_prepare_workspace_bytes", "epnet_image_normalise"):
        assert hasattr(hiplib, name)
    tiles = lambda p: (p + 2047) // 2048  # noqa: E731
    for b, p, n in ((1, 1, 1), (2, 2049, 16), (3, 122880, 16384), (1, 1048576, 65536)):
        want = b * (tiles(p) * 32 * 16 + tiles(p) * 16 + 32)            # two mask words per 64 points, four counts per tile, the plan
        assert hiplib.epnet_scan_prepare_workspace_bytes(b, p, n) == want, (b, p, n)
    for b, p, n in ((0, 64, 16), (1, 0, 16), (1, 64, 0), (1, 1048577, 16), (1, 64, 65537), (65536, 64, 16)):
        assert hiplib.epnet_scan_prepare_workspace_bytes(b, p, n) == 0
    fake = ctypes.c_void_p(4096)          # never dereferenced: the calls return before anything touches the device
    scope = (ctypes.c_double * 6)(-40, 40, -1, 3, 0, 70.4)
    args = lambda b, p, n: (b, p, n, 1, ctypes.cast(scope, ctypes.c_void_p), 40.0) + (fake,) * 9 + (1 << 30,) + (fake,) * 6 + (None,)  # noqa: E731
    for b, p, n in ((1, 0, 16), (1, 64, 0), (1, 1048577, 16), (1, 64, 65537), (65536, 64, 16)):
        assert hiplib.epnet_scan_prepare(*args(b, p, n)) == -4, (b, p, n)
    assert hiplib.epnet_scan_prepare(*args(0, 64, 16)) == 0 and hiplib.epnet_scan_prepare(*args(-1, 64, 16)) == -1
    small = list(args(2, 4096, 16))
    small[15] = 100
    assert hiplib.epnet_scan_prepare(*small) == -3                         # workspace too small
    nul = list(args(2, 4096, 16))
    nul[6] = None
    assert hiplib.epnet_scan_prepare(*nul) == -1
    assert hiplib.epnet_image_normalise(0, 4, 4, 4, 4, None, None, None, None, None, None) == 0
    assert hiplib.epnet_image_normalise(1, 4, 4, 4, 4, None, None, None, None, None, None) == -1
    assert hiplib.epnet_image_normalise(65536, 4, 4, 4, 4, fake, None, fake, fake, fake, None) == -4


def test_surface_refuses_cpu_tensors(hiplib):
    from epnet_amd import scan_cuda, scan_layer
    pts, num = torch.zeros((1, 1024, 4)), torch.tensor([5], dtype=torch.int32)
    V2C, R0, P2, shape = torch.zeros((1, 3, 4)), torch.zeros((1, 3, 3)), torch.zeros((1, 3, 4)), torch.tensor([[375, 1242]], dtype=torch.int32)
    tables = scan_layer.draw_scan_tables(1, 1024, 16, torch.Generator().manual_seed(1), device="cpu")
    with pytest.raises(RuntimeError, match="CUDAtensor"):
        scan_layer.prepare_scans(pts, num, V2C, R0, P2, shape, tables, npoints=16)
    with pytest.raises(RuntimeError, match="CUDAtensor"):
        scan_layer.normalise_images(torch.zeros((1, 4, 4, 3), dtype=torch.uint8))
    outs = (torch.zeros((1, 16, 3)), torch.zeros((1, 16)), torch.zeros((1, 16, 2)), None, torch.zeros((1, 16), dtype=torch.int32),
            torch.zeros((1, 6), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="CUDAtensor"):
        scan_cuda.scan_prepare_gpu(pts, num, V2C, R0, P2, shape, tables["keys"], None, True, rs.SCOPE.reshape(-1), 40.0, *outs)
    with pytest.raises(RuntimeError, match="CUDAtensor"):
        scan_cuda.image_normalise_gpu(torch.zeros((1, 4, 4, 3), dtype=torch.uint8), None, rs.MEAN, rs.STD, torch.zeros((1, 3, 4, 4)))


def test_collate_and_tables():
    from epnet_amd import scan_layer, synth
    a, b = synth.lidar_scan(1500, seed=1), synth.lidar_scan(700, seed=2).numpy()
    pts, num = scan_layer.collate_scans([a, b])
    assert pts.shape == (2, 2048, 4) and pts.dtype == torch.float32 and num.tolist() == [1500, 700] and num.dtype == torch.int32
    assert torch.equal(pts[0, :1500], a) and not pts[0, 1500:].any() and np.array_equal(pts[1, :700].numpy(), b) and not pts[1, 700:].any()
    assert scan_layer.collate_scans([np.zeros((1024, 4), F)])[0].shape == (1, 1024, 4)
    t = scan_layer.draw_scan_tables(3, 2048, 64, torch.Generator().manual_seed(2), device="cpu")
    assert t["keys"].shape == (3, 2048) and t["keys"].dtype == torch.int32 and t["slot_perm"].shape == (3, 64) and t["slot_perm"].dtype == torch.int32
    assert bool((t["keys"] < 0).any()) and bool((t["keys"] > 0).any()) and int(t["keys"].abs().max()) > 2 ** 30     # the full 32 bits
    assert all(sorted(row.tolist()) == list(range(64)) for row in t["slot_perm"])
    assert not torch.equal(t["slot_perm"][0], t["slot_perm"][1])


def test_synthetic_scan_and_calibration():
    """lidar_scan covers the whole azimuth, so most points fail the view test; a share of a realistic size passes"""
    from epnet_amd import synth
    scan = synth.lidar_scan(20000, seed=3)
    assert scan.shape == (20000, 4) and scan.dtype == torch.float32 and torch.equal(scan, synth.lidar_scan(20000, seed=3))
    assert bool((scan[:, 0] < 0).any()) and bool((scan[:, 1] < 0).any()) and float(scan[:, 3].min()) >= 0 and float(scan[:, 3].max()) < 1
    V2C, R0, P2, shape = synth.calibration(0)
    assert V2C.shape == (3, 4) and R0.shape == (3, 3) and P2.shape == (3, 4) and shape.tolist() == [375, 1242] and shape.dtype == torch.int32
    assert not torch.equal(synth.calibration(1)[2], P2)
    valid, near = rs.classify(scan.numpy(), 20000, V2C.numpy(), R0.numpy(), P2.numpy(), shape.numpy())[2:4]
    share = float(valid.mean())
    assert 0.05 < share < 0.35, share
    assert 0 < int((valid & ~near).sum()) < int(valid.sum())


def test_prepare_reads_the_reference_config_when_loaded(monkeypatch):
    import sys
    import types
    from epnet_amd import scan_layer
    assert scan_layer._ambient_cfg().PC_REDUCE_BY_RANGE is True and scan_layer._ambient_cfg().RPN.USE_INTENSITY is True
    mod = types.ModuleType("lib.config")
    mod.cfg = types.SimpleNamespace(PC_REDUCE_BY_RANGE=False, PC_AREA_SCOPE=np.zeros((3, 2)), RPN=types.SimpleNamespace(USE_INTENSITY=False))
    monkeypatch.setitem(sys.modules, "lib.config", mod)
    assert scan_layer._ambient_cfg() is mod.cfg

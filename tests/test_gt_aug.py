"""GT-database augmentation without a GPU: the numpy restatement (tests/gt_aug_restate.py) against the reference's own
apply_gt_aug_to_one_scene (tests/golden/gt_aug.npz, made by tests/golden/make_golden_gt_aug.py), known answers of the loop, and
the library's exports, limits and size queries.

Bound: the restatement's decisions, placed boxes (their heights included) and object points are BIT-EQUAL to the reference's, and
it keeps the same raw rows. The placement is float64 rounded once where the reference stores into float32; the overlap decisions
of the fixture are at least 1e-5 (ratio) and 1e-3 m (height) away from their thresholds, so float64 on the float32 box values
decides as the reference's float32 corners do."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gt_aug_restate as gr
import scan_restate as rs

F = np.float32
PLANE = np.array([0.0, -1.0, 0.0, 1.65])


# ---- the fixture ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reference():
    objects, scenes = gr.fixture()
    return gr.pack_database(objects), scenes


def test_fixture_covers_the_stated_cases(reference):
    db, scenes = reference
    outcomes, picks = set(), set()
    for s in scenes:
        placed = gr.place(db, s["apply"], s["extra_num"], s["cand"], s["all_boxes"], s["gt_boxes"], s["gt_alpha"], s["plane"], 4096)
        assert gr.decisions_are_clear(placed["ratios"], placed["heights"]) and placed["info"][6] == 0
        outcomes |= {tr[2] for tr in placed["trace"]}
        picks |= {"easy" if d in db["easy"] else "hard" for d in placed["acc_db"][:placed["info"][4]]}
    assert outcomes == {"accept", "range", "few", "overlap"} and picks == {"easy", "hard"}
    info = [gr.place(db, s["apply"], s["extra_num"], s["cand"], s["all_boxes"], s["gt_boxes"], s["gt_alpha"], s["plane"], 4096)["info"] for s in scenes]
    assert any(i[2] < 100 and i[3] == i[1] + 1 for i in info), "cnt ends the loop"
    assert any(i[2] == 100 and i[3] <= i[1] for i in info), "the tries run out"
    assert any(i[0] == 0 for i in info) and any(i[0] == 1 and i[4] == 0 for i in info)


def test_restatement_against_the_reference(reference):
    db, scenes = reference
    for i, s in enumerate(scenes):
        placed = gr.place(db, s["apply"], s["extra_num"], s["cand"], s["all_boxes"], s["gt_boxes"], s["gt_alpha"], s["plane"], 4096)
        acc, ng = int(placed["info"][4]), len(s["gt_boxes"])
        assert bool(s["ref_flag"]) == (acc > 0) and int(placed["info"][2]) == int(s["ref_tries"]), i
        assert placed["acc_box"][:acc].tobytes() == s["ref_extra_boxes"].tobytes(), i
        assert placed["gt_out"][ng:ng + acc].tobytes() == s["ref_extra_boxes"].tobytes() and placed["gt_out"][:ng].tobytes() == s["gt_boxes"].tobytes()
        assert placed["alpha_out"][ng:ng + acc].tobytes() == s["ref_extra_alpha"].tobytes(), i
        extra = gr.object_points(db, placed, 4096)
        rows = int(placed["info"][7])
        assert rows == len(s["ref_new_pts"]) and extra[:rows, :3].tobytes() == s["ref_new_pts"].tobytes(), i
        assert extra[:rows, 3].tobytes() == s["ref_new_intensity"].tobytes() and not extra[rows:].any()
        inside = np.zeros(len(s["pts"]), bool)
        for k in range(acc):
            inside |= gr.pts_in_box(s["pts"][:, :3], placed["remove_boxes"][k])
        assert np.array_equal(np.nonzero(~inside)[0], s["ref_kept_rows"]), i


def test_sampling_keeps_the_references_rows(reference):
    """the whole chain of one fixture scene under the identity calibration: a chosen raw row is one the reference kept, a chosen
    extra row one of its new points"""
    db, scenes = reference
    z = np.load(gr.os.path.join(gr.os.path.dirname(gr.__file__), "golden", "gt_aug.npz"))
    s = scenes[0]
    p, n, e = len(s["pts"]), 512, 4096
    rng = np.random.default_rng(3)
    scene = dict(pts=s["pts"], num_raw=p, V2C=z["V2C"], R0=z["R0"], P2=z["P2"], img_shape=z["img_shape"], all_boxes=s["all_boxes"],
                 gt_boxes=s["gt_boxes"], gt_alpha=s["gt_alpha"], plane=s["plane"])
    tables = dict(apply=s["apply"], extra_num=s["extra_num"], cand=s["cand"], keys=rng.integers(-2 ** 31, 2 ** 31, p + e).astype(np.int32),
                  slot_perm=rng.permutation(n).astype(np.int32))
    out = gr.whole(db, scene, tables, n, e)
    raw = out["choice"][out["choice"] < p]
    new = out["choice"][out["choice"] >= p] - p
    assert len(raw) and len(new) and set(raw.tolist()) <= set(s["ref_kept_rows"].tolist()) and new.max() < len(s["ref_new_pts"])
    at = np.nonzero(out["choice"] >= p)[0]
    assert out["pts_rect"][at].tobytes() == s["ref_new_pts"][new].tobytes()
    assert out["pts_intensity"][at].tobytes() == (s["ref_new_intensity"][new] - F(0.5)).tobytes()
    assert out["scene_info"][6] > 0 and out["scene_info"][7] == len(s["ref_new_pts"])


# ---- known answers ----------------------------------------------------------------------------------------------------------------
def row_of_objects(count, npts=10, spacing=8.0):
    """objects 8 m apart along x at z = 30, y = 1.0, npts points each"""
    out = []
    for k in range(count):
        box = np.array([-36 + spacing * (k % 10), 1.0, 20 + 10 * (k // 10), 1.5, 1.6, 4.0, 0.0], F)
        out.append({"gt_box3d": box, "points": np.tile(box[:3], (npts, 1)).astype(F), "intensity": np.full(npts, 0.25, F), "alpha": F(k)})
    return out


def test_the_loop_counts_as_the_reference_does():
    """cnt rises on every candidate that passes the range and point checks, accepted or not; the loop ends on cnt > extra_num, so
    extra_num + 1 candidates are placed at most"""
    db = gr.pack_database(row_of_objects(20))
    none = np.zeros((0, 7), F)
    out = gr.place(db, 1, 3, np.arange(20), none, none, np.zeros(0, F), PLANE, 4096)
    assert out["info"].tolist() == [1, 3, 4, 4, 4, 0, 0, 40] and out["acc_db"][:5].tolist() == [0, 1, 2, 3, -1]
    out = gr.place(db, 1, 3, np.array([0, 0, 0, 1, 1, 2, 3]), none, none, np.zeros(0, F), PLANE, 4096)     # repeats overlap themselves
    assert out["info"].tolist() == [1, 3, 4, 4, 2, 2, 0, 20] and [t[2] for t in out["trace"]] == ["accept", "overlap", "overlap", "accept"]
    out = gr.place(db, 0, 3, np.arange(20), none, none, np.zeros(0, F), PLANE, 4096)
    assert out["info"].tolist() == [0, 3, 0, 0, 0, 0, 0, 0] and (out["acc_db"] == -1).all()
    out = gr.place(db, 1, 15, np.arange(5), none, none, np.zeros(0, F), PLANE, 4096)                       # the tries run out
    assert out["info"].tolist() == [1, 15, 5, 5, 5, 0, 0, 50]


def test_placement_and_enlargement_known_answers():
    db = gr.pack_database(row_of_objects(3))
    gt = np.array([[-36, 1.65, 20, 1.5, 1.6, 4.0, 0.3]], F)                # on object 0
    out = gr.place(db, 1, 15, np.array([0, 1]), gt, gt, np.array([0.5], F), PLANE, 4096, g=3)
    assert [t[2] for t in out["trace"]] == ["overlap", "accept"]
    assert out["acc_move"][0] == 1.0 - 1.65 and out["acc_box"][0].tolist() == [-28.0, F(1.65), 20.0, 1.5, F(1.6), 4.0, 0.0]
    assert out["remove_boxes"][0, 3] == 3.5 and out["remove_boxes"][0, 4] == F(1.6)
    assert out["gt_out"].shape == (3 + gr.MAX_ACCEPT, 7) and out["gt_out"][0].tolist() == gt[0].tolist() and out["gt_out"][1, 0] == -28.0
    assert out["alpha_out"][:3].tolist() == [0.5, 1.0, 0.0]
    pts = gr.object_points(db, out, 64)
    assert pts[:10, 1].tolist() == [F(1.65)] * 10 and pts[:10, 3].tolist() == [0.25] * 10 and not pts[10:].any()
    # 0.5 m of enlargement on both: two cars 2.0 m apart side by side (w 1.6) overlap, 2.2 m apart they do not
    for gap, want in ((2.0, "overlap"), (2.2, "accept")):
        side = np.array([[-28, 1.65, 20 + gap, 1.5, 1.6, 4.0, 0.0]], F)
        assert gr.place(db, 1, 15, np.array([1]), side, side[:0], np.zeros(0, F), PLANE, 4096)["trace"][0][2] == want
    # a box above the candidate shares no height; one with w == 0 shares no area
    above = np.array([[-28, -0.5, 20, 1.5, 1.6, 4.0, 0.0]], F)
    flat = np.array([[-28, 1.65, 20, 1.5, -0.5, 4.0, 0.0]], F)             # w + 0.5 == 0
    for box in (above, flat):
        assert gr.place(db, 1, 15, np.array([1]), box, box[:0], np.zeros(0, F), PLANE, 4096)["trace"][0][2] == "accept"


def test_empty_scene_accepts():
    """with no current box the candidate is accepted (the reference's max() of an empty array raises there)"""
    db = gr.pack_database(row_of_objects(2))
    none = np.zeros((0, 7), F)
    out = gr.place(db, 1, 15, np.array([1]), none, none, np.zeros(0, F), PLANE, 4096)
    assert out["info"].tolist() == [1, 15, 1, 1, 1, 0, 0, 10] and out["gt_out"][0, 0] == -28.0


def test_capacity_rule():
    """a candidate whose points do not fit in what is left of e is rejected after the overlap test and counted separately; a
    smaller one behind it still fits; a small k_max ends the loop early"""
    objs = row_of_objects(6)
    objs[2] = dict(objs[2], points=np.tile(objs[2]["gt_box3d"][:3], (30, 1)).astype(F), intensity=np.zeros(30, F))
    db = gr.pack_database(objs)
    none = np.zeros((0, 7), F)
    out = gr.place(db, 1, 15, np.array([0, 1, 2, 2, 3, 0]), none, none, np.zeros(0, F), PLANE, 35)
    assert [t[2] for t in out["trace"]] == ["accept", "accept", "capacity", "capacity", "accept", "overlap"]
    assert out["info"].tolist() == [1, 15, 6, 6, 3, 1, 2, 30] and out["acc_row0"][:3].tolist() == [0, 10, 20]
    out = gr.place(db, 1, 15, np.arange(6), none, none, np.zeros(0, F), PLANE, 4096, k_max=2)
    # extra_num is used as min(15, k_max - 1) = 1: the loop ends on cnt == 2, so the accepted list cannot outgrow k_max
    assert out["info"].tolist() == [1, 15, 2, 2, 2, 0, 0, 20]


def test_the_label_is_the_placed_box_on_every_use():
    """the reference lowers obj.pos in place (:656), so the label of a second use of one object in one worker drifts; here two
    scenes that use one object get the same label height as the reference's first use: the road's"""
    db = gr.pack_database(row_of_objects(1))
    none = np.zeros((0, 7), F)
    a = gr.place(db, 1, 15, np.array([0]), none, none, np.zeros(0, F), PLANE, 4096)
    b = gr.place(db, 1, 15, np.array([0]), none, none, np.zeros(0, F), np.array([0.0, -1.0, 0.0, 1.9]), 4096)
    assert a["gt_out"][0, 1] == F(1.65) and b["gt_out"][0, 1] == F(1.9) and db["boxes"][0, 1] == 1.0


# ---- the library without a GPU ----------------------------------------------------------------------------------------------------
def test_exports_limits_and_size_queries(hiplib):
    from epnet_amd import gt_aug_cuda
    assert hiplib.epnet_abi_version() == 1
    assert (gt_aug_cuda.MAX_TRIES, gt_aug_cuda.MAX_EXISTING, gt_aug_cuda.MAX_ACCEPT) == (gr.MAX_TRIES, gr.MAX_EXISTING, gr.MAX_ACCEPT) == (128, 224, 32)
    fake = ctypes.c_void_p(4096)         # never dereferenced: the calls return before anything touches the device
    scope = (ctypes.c_double * 6)(*rs.SCOPE.reshape(-1))
    sc = ctypes.cast(scope, ctypes.c_void_p)

    def place(b=1, t=100, a=12, g=8, k=32, e=4096, d=40, extra_max=15):
        return hiplib.epnet_gt_aug_place(b, t, a, g, k, e, d, extra_max, 1, sc, *([fake] * 20), None)
    elimit, einval = -4, -1
    assert place(t=129) == elimit and place(a=225) == elimit and place(k=33) == elimit and place(k=0) == elimit
    assert place(extra_max=32) == elimit and place(k=16, extra_max=16) == elimit and place(e=1048577) == elimit and place(d=0) == elimit
    assert place(b=65536) == elimit and place(b=-1) == einval and place(b=0) == 0
    assert hiplib.epnet_gt_aug_place(1, 100, 12, 8, 32, 4096, 40, 15, 1, sc, None, *([fake] * 19), None) == einval
    assert hiplib.epnet_gt_aug_points(1, 4096, 33, 40, 100, *([fake] * 7), None) == elimit
    assert hiplib.epnet_gt_aug_points(1, 4096, 32, 40, 100, None, *([fake] * 6), None) == einval
    assert hiplib.epnet_gt_aug_points(1, 0, 32, 40, 100, *([None] * 7), None) == 0
    # the workspace: epnet_scan_prepare's layout over p + e rows, three counts per tile instead of two
    size, size_aug = hiplib.epnet_scan_prepare_workspace_bytes, hiplib.epnet_scan_prepare_aug_workspace_bytes
    for b, p, e, n in ((1, 2048, 0, 64), (3, 4096, 4096, 1024), (2, 122880, 8192, 16384), (257, 100, 7, 16)):
        tiles = (p + e + 2047) // 2048
        assert size_aug(b, p, e, n) == size(b, p + e, n) + b * tiles * 4, (b, p, e, n)
    assert size_aug(1, 1048576, 1, 16) == 0 and size_aug(1, 1048575, 1, 16) > 0 and size_aug(1, 64, -1, 16) == 0 and size_aug(0, 64, 0, 16) == 0

    def sample(b=1, p=64, e=64, n=16, k=32, stride=8, ws=1 << 20):
        return hiplib.epnet_scan_prepare_aug(b, p, e, n, k, 1, sc, 40.0, *([fake] * 10), stride, fake, None, fake, ws, *([fake] * 6), None)
    assert sample(k=33) == elimit and sample(p=1048576) == elimit and sample(n=65537) == elimit and sample(stride=0) == einval
    assert sample(ws=8) == -3 and sample(b=0) == 0


def test_the_surface_refuses_cpu_tensors():
    from epnet_amd import gt_aug_layer
    db = gt_aug_layer.GTDatabase.from_list(gr.synthetic_objects(8, seed=1), device="cpu")
    assert db.boxes.shape == (8, 7) and db.offsets.tolist()[-1] == int(db.npts.sum()) == db.points.shape[0] - 1
    cfg = gt_aug_layer.default_cfg()
    tables = gt_aug_layer.draw_gt_aug_tables(2, db, cfg, torch.Generator().manual_seed(1), "cpu")
    boxes, count = torch.zeros((2, 4, 7)), torch.zeros((2,), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CUDAtensor"):
        gt_aug_layer.place_objects(db, tables, boxes, count, boxes, torch.zeros((2, 4)), count, torch.zeros((2, 4), dtype=torch.float64), cfg)
    tables.update(keys=torch.zeros((2, 64 + 4096), dtype=torch.int32), slot_perm=None)
    with pytest.raises(RuntimeError, match="CUDAtensor"):
        gt_aug_layer.prepare_scans_gt_aug(torch.zeros((2, 64, 4)), count, torch.zeros((2, 3, 4)), torch.zeros((2, 3, 3)), torch.zeros((2, 3, 4)),
                                          torch.zeros((2, 2), dtype=torch.int32), tables, db, boxes, count, boxes, torch.zeros((2, 4)), count,
                                          torch.zeros((2, 4), dtype=torch.float64), npoints=16, cfg=cfg)


def test_database_packing_matches_the_restatement():
    from epnet_amd import gt_aug_layer
    objects = gr.synthetic_objects(40, seed=2)
    db, want = gt_aug_layer.GTDatabase.from_list(objects, device="cpu"), gr.pack_database(objects)
    for name in ("boxes", "alpha", "npts", "offsets", "easy", "hard"):
        got = getattr(db, name).numpy()
        assert got.dtype == want[name].dtype and np.array_equal(got, want[name]), name
    assert np.array_equal(db.points.numpy()[:-1], want["points"]) and (db.num_objects, db.num_easy, db.num_hard) == (40, len(want["easy"]), len(want["hard"]))
    assert set(want["easy"].tolist()) == {k for k in range(40) if want["npts"][k] > 100}


@pytest.mark.parametrize("rand_num,ratio", [(False, 0.6), (True, 0.6), (True, 0.0), (False, 1.0)])
def test_the_tables_have_the_stated_ranges(rand_num, ratio):
    from epnet_amd import gt_aug_layer
    db = gt_aug_layer.GTDatabase.from_list(gr.synthetic_objects(40, seed=3), device="cpu")
    cfg = gt_aug_layer.default_cfg()
    cfg.GT_AUG_RAND_NUM, cfg.GT_AUG_HARD_RATIO, cfg.GT_AUG_APPLY_PROB = rand_num, ratio, 0.75
    t = gt_aug_layer.draw_gt_aug_tables(4000, db, cfg, torch.Generator().manual_seed(5), "cpu")
    assert t["apply"].dtype == t["extra_num"].dtype == t["cand"].dtype == torch.int32 and t["cand"].shape == (4000, 100)
    assert set(t["apply"].tolist()) == {0, 1} and abs(float(t["apply"].float().mean()) - 0.75) < 0.03
    assert set(t["extra_num"].tolist()) == ({10, 11, 12, 13, 14} if rand_num else {15})
    cand = t["cand"].numpy()
    assert set(np.unique(cand).tolist()) == (set(db.hard.tolist()) if ratio == 1.0 else set(range(40)))     # every row that can come, no other
    easy = np.isin(cand, db.easy.numpy()).mean()
    share = {0.6: 0.4, 0.0: db.num_easy / 40.0, 1.0: 0.0}[ratio]       # p > ratio picks easy; without a ratio every row alike
    assert abs(easy - share) < 0.01, (easy, share)
    again = gt_aug_layer.draw_gt_aug_tables(4000, db, cfg, torch.Generator().manual_seed(5), "cpu")
    assert all(torch.equal(t[k], again[k]) for k in t)
    cfg.GT_AUG_APPLY_PROB = 0.0
    assert not gt_aug_layer.draw_gt_aug_tables(50, db, cfg, torch.Generator().manual_seed(5), "cpu")["apply"].any()


def test_an_empty_list_gives_skipped_tries():
    from epnet_amd import gt_aug_layer
    db = gt_aug_layer.GTDatabase.from_list(gr.synthetic_objects(6, seed=1, low=5, high=50), device="cpu")     # no easy object
    assert db.num_easy == 0
    t = gt_aug_layer.draw_gt_aug_tables(200, db, gt_aug_layer.default_cfg(), torch.Generator().manual_seed(2), "cpu")
    cand = t["cand"].numpy()
    assert cand.min() == -1 and abs((cand == -1).mean() - 0.4) < 0.02
    out = gr.place(gr.pack_database(gr.synthetic_objects(6, seed=1, low=5, high=50)), 1, 15, np.array([-1, 99]), np.zeros((0, 7), F),
                   np.zeros((0, 7), F), np.zeros(0, F), PLANE, 4096)
    assert out["info"].tolist() == [1, 15, 2, 0, 0, 0, 0, 0]


def test_gt_aug_enabled_false_applies_to_no_scene():
    """GT_AUG_ENABLED is the reference's switch (:443): off, no scene is augmented and the other draws are what they were"""
    from epnet_amd import gt_aug_layer
    db = gt_aug_layer.GTDatabase.from_list(gr.synthetic_objects(12, seed=4), device="cpu")
    cfg = gt_aug_layer.default_cfg()
    cfg.GT_AUG_APPLY_PROB = 1.0
    on = gt_aug_layer.draw_gt_aug_tables(64, db, cfg, torch.Generator().manual_seed(9), "cpu")
    cfg.GT_AUG_ENABLED = False
    off = gt_aug_layer.draw_gt_aug_tables(64, db, cfg, torch.Generator().manual_seed(9), "cpu")
    assert bool(on["apply"].all()) and not bool(off["apply"].any()) and off["apply"].dtype == torch.int32
    assert torch.equal(on["cand"], off["cand"]) and torch.equal(on["extra_num"], off["extra_num"])


def test_cfg_keys_are_read_from_the_given_object():
    from epnet_amd import gt_aug_layer
    cfg = gt_aug_layer.default_cfg()
    assert all(hasattr(cfg, k) for k in gt_aug_layer.GT_AUG_KEYS) and cfg.GT_EXTRA_NUM == 15 and cfg.GT_AUG_HARD_RATIO == 0.6
    assert isinstance(cfg, SimpleNamespace) and cfg.PC_REDUCE_BY_RANGE

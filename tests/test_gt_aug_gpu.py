"""GT-database augmentation on the GPU (epnet_amd/gt_aug_layer.py over csrc/gtaug.hip and the AUG variant of csrc/scan.hip).

Bound: every output is BIT-EQUAL to the numpy restatement (tests/gt_aug_restate.py, held to the reference in test_gt_aug.py). The
placement is float64 arithmetic in a fixed order rounded once, the points and the sampling are the float32 contract of
epnet_scan_prepare plus pt_in_box3d, and the selection is integer work. The one thing that is not bit-defined is the float64
ratio of the overlap decision (cos and sin of the device library against numpy's); every seeded scene is therefore drawn until no
compared ratio lies in (0, 1e-5) and no shared height or gap is below 1e-3 m (gt_aug_restate.decisions_are_clear, the fixture's own
conditions), which leaves eleven decimal orders between a last-bit difference and a decision. The capacity case is held to the
restatement alone, as the contract says.

Shapes: b = 3, p = 4096, e = 4096, n = 1024, 40 objects of 3..300 points, at most 12 existing boxes, T = 100; the batch sizes
(1, 2, 257) run at p = 1100, n = 256."""
import numpy as np
import pytest
import torch

import gt_aug_restate as gr
import offset_alloc as oa
import scan_restate as rs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F = np.float32
T = 100
SCAN_KEYS = ("pts_rect", "pts_intensity", "pts_origin_xy", "pts_input", "choice", "scene_info")
ALL_KEYS = SCAN_KEYS + gr.PLACE_KEYS + ("extra_pts",)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().cpu().numpy()


OBJECTS = gr.synthetic_objects(40, seed=900, cone=True)     # in the field of view: their removal boxes hold scan points
DB = gr.pack_database(OBJECTS)


@pytest.fixture(scope="module")
def database(hiplib):
    from epnet_amd import gt_aug_layer
    return gt_aug_layer.GTDatabase.from_list(OBJECTS, DEV)


def cfg_with(extra_num=15, rand_num=False):
    from epnet_amd import gt_aug_layer
    cfg = gt_aug_layer.default_cfg()
    cfg.GT_EXTRA_NUM, cfg.GT_AUG_RAND_NUM = extra_num, rand_num
    return cfg


class Batch:
    """b seeded scenes: scan_restate.scene_with's scans (an exact number of valid and far points), `existing` boxes on the road of
    which all but two are label rows, a road plane and the tables; every scene is redrawn until its decisions are clear and,
    without `capacity`, until no candidate is rejected for want of point rows (the contract tested against the reference)"""

    def __init__(self, b, p, e, n, seed, existing=12, counts=(300, 2500), extra_num=15, apply=None, a_cap=None, g_cap=None, db=DB,
                 capacity=False):
        self.b, self.p, self.e, self.n, self.db = b, p, e, n, db
        most = existing if isinstance(existing, int) else max(existing)
        a_cap = a_cap if a_cap is not None else max(most, 1)
        g_cap = g_cap if g_cap is not None else max(most, 1)
        self.pts, self.cal = np.zeros((b, p, 4), F), []
        self.num_raw = np.zeros(b, np.int32)
        self.all_boxes, self.num_all = np.zeros((b, a_cap, 7), F), np.zeros(b, np.int32)
        self.gt, self.alpha, self.num_gt = np.zeros((b, g_cap, 7), F), np.zeros((b, g_cap), F), np.zeros(b, np.int32)
        self.plane = np.zeros((b, 4), np.float64)
        self.apply, self.extra_num, self.cand = np.zeros(b, np.int32), np.full(b, extra_num, np.int32), np.zeros((b, T), np.int32)
        self.keys, self.slot_perm = np.zeros((b, p + e), np.int32), np.zeros((b, n), np.int32)
        for k in range(b):
            far, near = counts[k % len(counts)] if isinstance(counts[0], tuple) else counts
            num_raw = p - (k % 3)
            pts, V2C, R0, P2, shape = rs.scene_with(p, num_raw, far, near, seed * 1000 + k)
            self.pts[k], self.num_raw[k] = pts, num_raw
            self.cal.append((V2C, R0, P2, shape))
            for attempt in range(50):
                rng = np.random.default_rng((seed * 1000 + k) * 50 + attempt)
                plane = np.array([rng.uniform(-0.02, 0.02), -1.0, rng.uniform(-0.02, 0.02), rng.uniform(1.5, 1.8)])
                count = existing if isinstance(existing, int) else existing[k % len(existing)]
                boxes = np.stack([o["gt_box3d"] for o in gr.synthetic_objects(count, seed=seed * 77 + k * 50 + attempt)]) if count else np.zeros((0, 7), F)
                for bx in boxes:
                    bx[1] = F((-plane[3] - plane[0] * bx[0] - plane[2] * bx[2]) / plane[1] + rng.uniform(-0.1, 0.1))
                cand = rng.integers(0, len(db["boxes"]), T).astype(np.int32)
                on = int(rng.uniform() < 0.8) if apply is None else int(apply[k % len(apply)])
                ng = max(count - 2, 0)
                placed = gr.place(db, on, extra_num, cand, boxes, boxes[:ng], np.zeros(ng, F), plane, e, g=g_cap)
                if gr.decisions_are_clear(placed["ratios"], placed["heights"]) and (capacity or placed["info"][6] == 0):
                    break
            else:
                raise AssertionError("no clear draw")
            self.all_boxes[k, :count], self.num_all[k] = boxes, count
            self.gt[k, :ng], self.alpha[k, :ng], self.num_gt[k] = boxes[:ng], rng.uniform(-3, 3, ng), ng
            self.plane[k], self.apply[k], self.cand[k] = plane, on, cand
            self.keys[k] = rng.integers(-2 ** 31, 2 ** 31, p + e)
            self.slot_perm[k] = rng.permutation(n)
        self._want = None

    def scene(self, k):
        V2C, R0, P2, shape = self.cal[k]
        return dict(pts=self.pts[k], num_raw=self.num_raw[k], V2C=V2C, R0=R0, P2=P2, img_shape=shape, all_boxes=self.all_boxes[k, :self.num_all[k]],
                    gt_boxes=self.gt[k, :self.num_gt[k]], gt_alpha=self.alpha[k, :self.num_gt[k]], plane=self.plane[k])

    def want(self):
        """computed once, shared, not modified"""
        if self._want is None:
            rows = [gr.whole(self.db, self.scene(k), dict(apply=self.apply[k], extra_num=self.extra_num[k], cand=self.cand[k], keys=self.keys[k],
                                                          slot_perm=self.slot_perm[k]), self.n, self.e, g=self.gt.shape[1]) for k in range(self.b)]
            self._want = {key: np.stack([r[key] for r in rows]) for key in ALL_KEYS}
        return self._want

    def tensors(self):
        cal = [dev(np.stack([c[j] for c in self.cal])) for j in range(4)]
        return [dev(self.pts), dev(self.num_raw)] + cal

    def tables(self):
        return {"apply": dev(self.apply), "extra_num": dev(self.extra_num), "cand": dev(self.cand), "keys": dev(self.keys), "slot_perm": dev(self.slot_perm)}

    def labels(self):
        return [dev(self.all_boxes), dev(self.num_all), dev(self.gt), dev(self.alpha), dev(self.num_gt), dev(self.plane)]

    def call(self, database, cfg=None, tensors=None, tables=None, labels=None):
        from epnet_amd import gt_aug_layer
        return gt_aug_layer.prepare_scans_gt_aug(*(tensors or self.tensors()), tables or self.tables(), database, *(labels or self.labels()),
                                                 npoints=self.n, extra_rows=self.e, cfg=cfg or cfg_with(int(self.extra_num.max())))

    def run(self, database, cfg=None):
        return flatten(self.call(database, cfg))


def flatten(out):
    got = {k: host(out[k]) for k in ("pts_rect", "pts_origin_xy", "pts_input", "choice", "scene_info", "extra_pts")}
    got["pts_intensity"] = host(out["pts_features"]).reshape(got["choice"].shape)
    got["gt_out"], got["alpha_out"], got["info"] = host(out["gt_boxes3d"]), host(out["gt_alpha"]), host(out["gt_aug_info"])
    for k in ("acc_db", "acc_box", "acc_move", "acc_row0", "remove_boxes"):
        got[k] = host(out["placed"][k])
    return got


def differences(got, want, keys=ALL_KEYS):
    bad = []
    for k in keys:
        if got[k].dtype != want[k].dtype or got[k].shape != want[k].shape:
            bad.append((k, got[k].dtype, got[k].shape, want[k].dtype, want[k].shape))
        elif got[k].tobytes() != want[k].tobytes():
            where = np.nonzero(got[k].reshape(-1) != want[k].reshape(-1))[0]
            bad.append((k, len(where), np.unravel_index(where[:4], got[k].shape), got[k].reshape(-1)[where[:4]], want[k].reshape(-1)[where[:4]]))
    return bad


@pytest.fixture(scope="module")
def main_batch():
    return Batch(3, 4096, 4096, 1024, seed=1, apply=(1, 1, 0))


# ---- against the reference's scenes and the restatement ---------------------------------------------------------------------------------
def test_kernels_on_the_reference_scenes(hiplib):
    """the fixture's scenes in one batch under the identity calibration: the restatement's bits, the reference's boxes and points,
    and only raw rows the reference kept"""
    from epnet_amd import gt_aug_layer
    objects, scenes = gr.fixture()
    db = gr.pack_database(objects)
    database = gt_aug_layer.GTDatabase.from_list(objects, DEV)
    z = np.load(gr.os.path.join(gr.os.path.dirname(gr.__file__), "golden", "gt_aug.npz"))
    b, p, e, n = len(scenes), 3072, 4096, 1024
    rng = np.random.default_rng(11)
    pts, num_raw = np.zeros((b, p, 4), F), np.array([len(s["pts"]) for s in scenes], np.int32)
    all_boxes, gt, alpha = np.zeros((b, 12, 7), F), np.zeros((b, 12, 7), F), np.zeros((b, 12), F)
    for k, s in enumerate(scenes):
        pts[k, :num_raw[k]] = s["pts"]
        all_boxes[k, :len(s["all_boxes"])], gt[k, :len(s["gt_boxes"])], alpha[k, :len(s["gt_boxes"])] = s["all_boxes"], s["gt_boxes"], s["gt_alpha"]
    num_all, num_gt = np.array([len(s["all_boxes"]) for s in scenes], np.int32), np.array([len(s["gt_boxes"]) for s in scenes], np.int32)
    keys, perm = rng.integers(-2 ** 31, 2 ** 31, (b, p + e)).astype(np.int32), np.stack([rng.permutation(n) for _ in range(b)]).astype(np.int32)
    rep = lambda a: dev(np.broadcast_to(a, (b,) + a.shape))  # noqa: E731
    tables = {"apply": dev(np.array([s["apply"] for s in scenes], np.int32)), "extra_num": dev(np.array([s["extra_num"] for s in scenes], np.int32)),
              "cand": dev(np.stack([s["cand"] for s in scenes])), "keys": dev(keys), "slot_perm": dev(perm)}
    out = gt_aug_layer.prepare_scans_gt_aug(dev(pts), dev(num_raw), rep(z["V2C"]), rep(z["R0"]), rep(z["P2"]), rep(z["img_shape"]), tables, database,
                                            dev(all_boxes), dev(num_all), dev(gt), dev(alpha), dev(num_gt), dev(np.stack([s["plane"] for s in scenes])),
                                            npoints=n, extra_rows=e, cfg=cfg_with())
    got = flatten(out)
    for k, s in enumerate(scenes):
        scene = dict(pts=pts[k], num_raw=num_raw[k], V2C=z["V2C"], R0=z["R0"], P2=z["P2"], img_shape=z["img_shape"], all_boxes=s["all_boxes"],
                     gt_boxes=s["gt_boxes"], gt_alpha=s["gt_alpha"], plane=s["plane"])
        want = gr.whole(db, scene, dict(apply=s["apply"], extra_num=s["extra_num"], cand=s["cand"], keys=keys[k], slot_perm=perm[k]), n, e, g=12)
        assert not differences({key: got[key][k] for key in ALL_KEYS}, want), k
        acc, rows = int(got["info"][k, 4]), int(got["info"][k, 7])
        assert got["acc_box"][k, :acc].tobytes() == s["ref_extra_boxes"].tobytes() and int(got["info"][k, 2]) == int(s["ref_tries"])
        assert got["extra_pts"][k, :rows, :3].tobytes() == s["ref_new_pts"].tobytes() and got["extra_pts"][k, :rows, 3].tobytes() == s["ref_new_intensity"].tobytes()
        raw = got["choice"][k][(got["choice"][k] >= 0) & (got["choice"][k] < p)]
        assert set(raw.tolist()) <= set(s["ref_kept_rows"].tolist())


def test_seeded_batch_against_the_restatement(database, main_batch):
    want = main_batch.want()
    assert want["info"][:, 0].tolist() == [1, 1, 0] and (want["info"][:2, 4] >= 3).all() and want["info"][:, 6].sum() == 0
    assert want["scene_info"][:2, 6].min() > 0 and (want["choice"] >= main_batch.p).any(), "points are removed and extra rows are chosen"
    assert not differences(main_batch.run(database), want)


@pytest.mark.parametrize("b", (1, 2, 257))
def test_batch_sizes(database, b):
    batch = Batch(b, 1100, 2048, 256, seed=10 + b, existing=(4, 0, 2), counts=[(40, 500), (10, 150), (0, 0), (300, 100)])
    want = batch.want()
    assert want["info"][:, 6].sum() == 0 and (b < 6 or {0, 2, 4} <= set(want["scene_info"][:, 3].tolist()))
    assert not differences(batch.run(database), want)


@pytest.mark.parametrize("num_all,extra_num", [(0, 10), (224, 10), (12, 31), (224, 31)])
def test_box_and_count_limits(database, num_all, extra_num):
    """no existing box and EPNET_GT_AUG_MAX_EXISTING of them; extra_num at its least and at k_max - 1"""
    batch = Batch(2, 1100, 4096, 256, seed=20 + num_all + extra_num, existing=num_all, counts=(40, 500), extra_num=extra_num, apply=(1,))
    want = batch.want()
    assert (want["info"][:, 3] >= 1).all() and want["info"][:, 6].sum() == 0
    if num_all == 0:
        assert (want["info"][:, 5] < want["info"][:, 3]).all()         # the first candidate meets no box and is accepted
    assert not differences(batch.run(database, cfg_with(extra_num)), want)


def test_limits_are_refused(database):
    from epnet_amd import _lib
    batch = Batch(1, 1100, 512, 64, seed=5, existing=2, counts=(10, 100))
    with pytest.raises(_lib.EpnetError, match="supported range"):
        batch.call(database, cfg_with(32))                             # extra_num must stay below k_max
    big = Batch(1, 1100, 512, 64, seed=5, existing=2, counts=(10, 100), a_cap=225)
    with pytest.raises(_lib.EpnetError, match="supported range"):
        big.call(database)
    tables = batch.tables()
    tables["cand"] = torch.zeros((1, 129), dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.EpnetError, match="supported range"):
        batch.call(database, tables=tables)


def test_point_capacity(database):
    """e = 300 rows: candidates that do not fit are rejected and counted apart, smaller ones behind them still fit (against the
    restatement only: the reference has no such limit)"""
    batch = Batch(3, 1100, 300, 256, seed=31, existing=3, counts=(40, 500), apply=(1,), capacity=True)
    want = batch.want()
    assert (want["info"][:, 6] > 0).all() and (want["info"][:, 7] <= 300).all() and (want["info"][:, 4] > 0).any()
    assert not differences(batch.run(database), want)


def test_no_extras_and_no_boxes_is_scan_prepare(database, main_batch):
    """e = 0 and no removal box: the bits of epnet_scan_prepare, by the stand-in directly and by the surface with apply = 0"""
    from epnet_amd import gt_aug_cuda, scan_layer
    b, p, n = main_batch.b, main_batch.p, main_batch.n
    tensors = main_batch.tensors()
    keys, perm = dev(main_batch.keys[:, :p]), dev(main_batch.slot_perm)
    plain = scan_layer.prepare_scans(*tensors, {"keys": keys, "slot_perm": perm}, npoints=n)
    z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=DEV)  # noqa: E731
    outs = [z((b, n, 3)), z((b, n, 1)), z((b, n, 2)), z((b, n, 4)), z((b, n), torch.int32), z((b, 8), torch.int32)]
    gt_aug_cuda.scan_prepare_aug_gpu(*tensors, z((b, 0, 4)), z((b, 0, 7)), z((b, 8), torch.int32), keys, perm, True, rs.SCOPE.reshape(-1), 40.0, *outs)
    names = ("pts_rect", "pts_features", "pts_origin_xy", "pts_input", "choice")
    assert all(torch.equal(plain[k], o) for k, o in zip(names, outs))
    assert torch.equal(plain["scene_info"], outs[5][:, :6]) and not outs[5][:, 6:].any()
    tables = main_batch.tables()
    tables["apply"] = torch.zeros_like(tables["apply"])
    for e in (0, 512):                                                  # nothing applied: the extra rows stay empty
        tables["keys"] = dev(main_batch.keys[:, :p + e])
        from epnet_amd import gt_aug_layer
        out = gt_aug_layer.prepare_scans_gt_aug(*tensors, tables, database, *main_batch.labels(), npoints=n, extra_rows=e, cfg=cfg_with())
        assert all(torch.equal(plain[k], out[k]) for k in names) and torch.equal(plain["scene_info"], out["scene_info"][:, :6])
        assert out["gt_aug_info"].tolist() == [[0, 15, 0, 0, 0, 0, 0, 0]] * b and not out["extra_pts"].any()
        assert torch.equal(out["gt_boxes3d"][:, :12], dev(main_batch.gt)) and not out["gt_boxes3d"][:, 12:].any()


def test_extras_push_a_scene_from_case_2_into_case_0(database):
    """900 valid raw points for n = 1024 is case 2 (every valid point, then 124 of them again); with the objects' rows there are
    more than n candidates and the scene is case 0: every far point and a subset of the near ones, extra rows among them"""
    batch = Batch(1, 4096, 4096, 1024, seed=41, existing=2, counts=(100, 800), apply=(1,))
    s, k = batch.scene(0), batch.keys[0]
    alone = rs.prepare(s["pts"], s["num_raw"], s["V2C"], s["R0"], s["P2"], s["img_shape"], k[:4096], batch.slot_perm[0], 1024)
    want = batch.want()
    assert alone["scene_info"][3] == 2 and want["scene_info"][0, 3] == 0 and want["scene_info"][0, 1] > 1024 > want["scene_info"][0, 1] - want["scene_info"][0, 7]
    assert not differences(batch.run(database), want)


# ---- known answers through the kernels ----------------------------------------------------------------------------------------------------
def test_known_answers_on_the_device(hiplib):
    """the hand-made cases of test_gt_aug.py through epnet_gt_aug_place and epnet_gt_aug_points themselves: the loop's counting,
    the empty scene, the capacity rule, the enlargement, a box above the candidate and one without width"""
    from epnet_amd import gt_aug_layer
    import test_gt_aug as cpu
    objs = cpu.row_of_objects(20)
    objs[2] = dict(objs[2], points=np.tile(objs[2]["gt_box3d"][:3], (30, 1)).astype(F), intensity=np.zeros(30, F))
    database = gt_aug_layer.GTDatabase.from_list(objs, DEV)
    side = lambda gap: [-28, 1.65, 20 + gap, 1.5, 1.6, 4.0, 0.0]  # noqa: E731
    # (tries, existing boxes, extra_num, extra rows) -> info
    cases = [(list(range(20)), [], 3, 4096, [1, 3, 4, 4, 4, 0, 0, 60]),
             ([0, 0, 0, 1, 1, 2, 3], [], 3, 4096, [1, 3, 4, 4, 2, 2, 0, 20]),
             ([1], [], 15, 4096, [1, 15, 1, 1, 1, 0, 0, 10]),
             ([0, 1, 2, 2, 3, 0], [], 15, 35, [1, 15, 6, 6, 3, 1, 2, 30]),
             ([1], [side(2.0)], 15, 4096, [1, 15, 1, 1, 0, 1, 0, 0]),
             ([1], [side(2.2)], 15, 4096, [1, 15, 1, 1, 1, 0, 0, 10]),
             ([1], [[-28, -0.5, 20, 1.5, 1.6, 4.0, 0.0]], 15, 4096, [1, 15, 1, 1, 1, 0, 0, 10]),
             ([1], [[-28, 1.65, 20, 1.5, -0.5, 4.0, 0.0]], 15, 4096, [1, 15, 1, 1, 1, 0, 0, 10])]
    for tries, boxes, extra_num, e, want in cases:
        cand = np.full((1, 8 if len(tries) <= 8 else 20), -1, np.int32)
        cand[0, :len(tries)] = tries
        all_boxes = np.zeros((1, 1, 7), F)
        if boxes:
            all_boxes[0, :len(boxes)] = boxes
        count = dev(np.array([len(boxes)], np.int32))
        tables = {"apply": dev(np.ones(1, np.int32)), "extra_num": dev(np.array([extra_num], np.int32)), "cand": dev(cand)}
        out = gt_aug_layer.place_objects(database, tables, dev(all_boxes), count, dev(all_boxes), dev(np.zeros((1, 1), F)), count,
                                         dev(cpu.PLANE[None]), cfg_with(extra_num), extra_rows=e)
        info = out["gt_aug_info"][0].tolist()
        info[2] = min(info[2], len(tries))                      # the padding tries (row -1) are skipped, not placed
        assert info == want, (tries, boxes, info)
    # the last accepted case: the placed box, its move, the removal box and its points
    assert out["acc_box"][0, 0].tolist() == [-28.0, float(F(1.65)), 20.0, 1.5, float(F(1.6)), 4.0, 0.0]
    assert float(out["acc_move"][0, 0]) == 1.0 - 1.65 and float(out["remove_boxes"][0, 0, 3]) == 3.5
    from epnet_amd import gt_aug_cuda
    pts = torch.full((1, 64, 4), 7.0, device=DEV)
    gt_aug_cuda.gt_aug_points_gpu(database.points, database.offsets, out["acc_db"], out["acc_move"], out["acc_row0"], out["gt_aug_info"], pts)
    assert host(pts)[0, :10].tolist() == [[-28.0, float(F(1.65)), 20.0, 0.25]] * 10 and not bool(pts[0, 10:].any())
    with pytest.raises(RuntimeError, match="db_offsets must hold"):
        gt_aug_cuda.gt_aug_points_gpu(database.points, database.offsets[:1], out["acc_db"], out["acc_move"], out["acc_row0"], out["gt_aug_info"], pts)
    with pytest.raises(RuntimeError, match="acc_move has"):
        gt_aug_cuda.gt_aug_points_gpu(database.points, database.offsets, out["acc_db"], out["acc_move"][:, :1].contiguous(), out["acc_row0"],
                                      out["gt_aug_info"], pts)
    assert host(pts)[0, :10].tolist() == [[-28.0, float(F(1.65)), 20.0, 0.25]] * 10          # a refused call writes nothing


def test_switched_off_is_prepare_scans(database, main_batch):
    """GT_AUG_ENABLED = False: the tables apply to no scene and the call gives prepare_scans' bits"""
    from epnet_amd import gt_aug_layer, scan_layer
    cfg = cfg_with()
    cfg.GT_AUG_ENABLED, cfg.GT_AUG_APPLY_PROB = False, 1.0
    tables = gt_aug_layer.draw_tables(main_batch.b, main_batch.p, database, main_batch.e, main_batch.n, cfg, torch.Generator(device=DEV).manual_seed(5), DEV)
    tensors = main_batch.tensors()
    out = main_batch.call(database, cfg, tensors=tensors, tables=tables)
    plain = scan_layer.prepare_scans(*tensors, {"keys": tables["keys"][:, :main_batch.p].contiguous(), "slot_perm": tables["slot_perm"]}, npoints=main_batch.n)
    assert all(torch.equal(plain[k], out[k]) for k in ("pts_rect", "pts_features", "pts_origin_xy", "pts_input", "choice"))
    assert not out["gt_aug_info"][:, 0].any() and not out["scene_info"][:, 6:].any()


# ---- reproducibility, no synchronisation, one graph -------------------------------------------------------------------------------------
def test_runs_are_bit_equal_and_need_no_sync(database, main_batch):
    from epnet_amd import gt_aug_layer
    tensors, tables, labels = main_batch.tensors(), main_batch.tables(), main_batch.labels()
    a = main_batch.call(database, tensors=tensors, tables=tables, labels=labels)
    b = main_batch.call(database, tensors=tensors, tables=tables, labels=labels)
    cfg = cfg_with(15, rand_num=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        c = main_batch.call(database, tensors=tensors, tables=tables, labels=labels)
        drawn = gt_aug_layer.draw_tables(main_batch.b, main_batch.p, database, main_batch.e, main_batch.n, cfg, torch.Generator(device=DEV).manual_seed(3), DEV)
        d = main_batch.call(database, cfg, tensors=tensors, tables=drawn, labels=labels)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    fa, fb, fc = flatten(a), flatten(b), flatten(c)
    assert all(fa[k].tobytes() == fb[k].tobytes() == fc[k].tobytes() for k in ALL_KEYS)
    assert not differences(fa, main_batch.want())
    info = host(d["gt_aug_info"])
    assert set(info[:, 1].tolist()) <= {10, 11, 12, 13, 14} and (info[:, 4] <= info[:, 3]).all() and drawn["keys"].shape == (3, 8192)
    assert int(drawn["cand"].min()) >= 0 and int(drawn["cand"].max()) < 40


def test_augmentation_targets_and_loss_in_one_graph(database, main_batch):
    """placement + points + sampling + augment_and_label + rpn_loss forward and backward captured in ONE torch.cuda.graph (the
    capture fails on any synchronisation with the host), replayed after in-place copies of a second batch: equal to eager"""
    from epnet_amd import loss_utils, rpn_target_layer as rtl
    second = Batch(3, 4096, 4096, 1024, seed=2, apply=(1, 0, 1))
    b, n, c = 3, main_batch.n, 76
    tensors, tables, labels = main_batch.tensors(), main_batch.tables(), main_batch.labels()
    aug = rtl.draw_augmentation(b, generator=torch.Generator(device=DEV).manual_seed(4), device=DEV)
    g = torch.Generator(device=DEV).manual_seed(8)
    cls_in = torch.randn((b, n, 1), generator=g, device=DEV).requires_grad_(True)
    reg_in = torch.randn((b, n, c), generator=g, device=DEV).requires_grad_(True)
    cfg, aug_cfg = loss_utils.default_cfg(), cfg_with()

    def step():
        out = main_batch.call(database, aug_cfg, tensors=tensors, tables=tables, labels=labels)
        pts, gt_aug, cls_label, reg_label = rtl.augment_and_label(out["pts_rect"], out["gt_boxes3d"], out["gt_alpha"], aug)
        res = loss_utils.rpn_loss(cls_in, reg_in, cls_label, reg_label, cfg)
        grads = torch.autograd.grad(res.loss, [cls_in, reg_in])
        return [out["pts_rect"], out["pts_input"], out["choice"], out["scene_info"], out["gt_boxes3d"], out["gt_aug_info"], out["extra_pts"], pts,
                gt_aug, cls_label, res.loss] + list(grads)
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
    assert int((captured[9] > 0).sum()) > 0, "foreground points, some of them in pasted objects"
    with torch.no_grad():
        for mine, other in ((tensors, second.tensors()), (labels, second.labels())):
            for dst, src in zip(mine, other):
                dst.copy_(src)
        for key, value in second.tables().items():
            tables[key].copy_(value)
    graph.replay()
    torch.cuda.synchronize()
    eager_second = step()
    assert all(torch.equal(x, y) for x, y in zip(eager_second, captured))
    assert not torch.equal(eager_second[0], eager_first[0]) and host(captured[2]).tobytes() == second.want()["choice"].tobytes()
    assert host(captured[5]).tobytes() == second.want()["info"].tobytes()


# ---- pointers off a 16-byte boundary ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skews", [{}, {"db_points": 4}, {"extra_pts": 4}, {"db_points": 4, "extra_pts": 4}, {"db_points": 8, "extra_pts": 8},
                                   {"db_points": 12, "extra_pts": 12}, {"db_points": 4, "extra_pts": 12, "rest": 4}],
                         ids=["aligned", "db_points+4", "extra_pts+4", "all+4", "all+8", "all+12", "every tensor"])
def test_points_kernel_with_offset_pointers(hiplib, skews):
    """epnet_gt_aug_points picks 16-byte row loads and stores from the alignment of db_points and extra_pts and scalar ones
    otherwise (points_kernel<false>): the same rows either way, no stray write, every element written"""
    from epnet_amd import gt_aug_cuda
    oa.forget()
    b, e, k_max = 3, 700, 32
    placed = [gr.place(DB, 1, 15, np.random.default_rng(60 + k).integers(0, 40, T), np.zeros((0, 7), F), np.zeros((0, 7), F), np.zeros(0, F),
                       np.array([0.0, -1.0, 0.0, 1.6 + 0.05 * k]), e) for k in range(b)]
    assert all(p["info"][4] >= 2 for p in placed) and any(p["info"][6] > 0 for p in placed)
    want = np.stack([gr.object_points(DB, p, e) for p in placed])
    rest = skews.get("rest", 0)
    stack = lambda key: np.stack([p[key] for p in placed])  # noqa: E731
    db_points = oa.skewed(DB["points"], torch.float32, skews.get("db_points", 0))
    offsets = oa.skewed(DB["offsets"], torch.int32, rest)
    acc_db, acc_row0, info = (oa.skewed(stack(key), torch.int32, rest) for key in ("acc_db", "acc_row0", "info"))
    acc_move = dev(stack("acc_move"))
    extra = oa.output((b, e, 4), torch.float32, skews.get("extra_pts", 0))
    assert db_points.data_ptr() % 16 == skews.get("db_points", 0) and extra.data_ptr() % 16 == skews.get("extra_pts", 0)
    gt_aug_cuda.gt_aug_points_gpu(db_points, offsets, acc_db, acc_move, acc_row0, info, extra)
    oa.check()
    assert oa.unwritten(extra) == 0 and host(extra).tobytes() == want.tobytes()


def test_every_tensor_of_the_placement_off_its_boundary(hiplib):
    """epnet_gt_aug_place selects nothing by alignment: with every float32 / int32 tensor 4 bytes and the float64 ones 8 bytes
    off a 16-byte boundary it gives the restatement's bits, writes every element and nothing else"""
    from epnet_amd import gt_aug_cuda
    oa.forget()
    batch = Batch(2, 64, 2048, 16, seed=71, existing=5, counts=(0, 0), apply=(1,))
    want = batch.want()
    b, k, g = 2, 32, batch.gt.shape[1]
    i32, f32 = torch.int32, torch.float32
    ins = [oa.skewed(a, t, 4) for a, t in ((DB["boxes"], f32), (DB["alpha"], f32), (DB["npts"], i32), (batch.apply, i32), (batch.extra_num, i32),
                                           (batch.cand, i32), (batch.all_boxes, f32), (batch.num_all, i32), (batch.gt, f32), (batch.alpha, f32),
                                           (batch.num_gt, i32))]
    plane = oa.skewed(batch.plane, torch.float64, 8)
    acc_move = oa.skewed(np.full((b, k), np.nan), torch.float64, 8)      # offset_alloc has no float64 sentinel: NaN marks an unwritten element
    outs = {"acc_db": oa.output((b, k), i32), "acc_box": oa.output((b, k, 7), f32), "acc_row0": oa.output((b, k), i32),
            "remove_boxes": oa.output((b, k, 7), f32), "gt_out": oa.output((b, g + k, 7), f32), "alpha_out": oa.output((b, g + k), f32),
            "info": oa.output((b, 8), i32)}
    gt_aug_cuda.gt_aug_place_gpu(*ins, plane, 15, batch.e, True, rs.SCOPE.reshape(-1), outs["acc_db"], outs["acc_box"], acc_move, outs["acc_row0"],
                                 outs["remove_boxes"], outs["gt_out"], outs["alpha_out"], outs["info"])
    oa.check()
    outs["acc_move"] = acc_move
    assert not bool(torch.isnan(acc_move).any()) and all(oa.unwritten(v) == 0 for key, v in outs.items() if key != "acc_move")
    assert not differences({key: host(v) for key, v in outs.items()}, want, gr.PLACE_KEYS)

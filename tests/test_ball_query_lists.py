"""The indexed ball query's hit lists at every length where the kernels change path, against the oracle's ball_query (the reference's
one-thread-per-centre scan, ball_query_gpu.cu:9-45) -- indices bit-exact, every slot written, nothing excluded.

The pair kernel keeps one hit list per centre for the two nested balls of an MSG level and emits the four lists of a wave in one
pass while both centres hold at most 32 hits; up to 64 a list is ordered on its own, beyond that the centre walks again through
the bitmap. The clouds here are PLANTED: around a chosen centre lie exactly c_in points inside the smaller radius and c_out more
inside the larger one, with c_in and c_out from VALUES (0, 1, every bound of a list +-1, every nsample of the scale pairs below
+-1, 200), far from everything else. Which original indices those points carry is decided from the walk order of the library's
own scene index (read back once per cloud): ascending, descending or shuffled against it, the smallest always in the last bucket
walked -- so "the first nsample in index order, padded with the first" is never what the walk meets first.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 3
R_IN, R_OUT = 0.3, 0.9
PITCH = 4.0          # between planted centres: no ball reaches a neighbour's points
M_TOTAL = 1030       # centres per scene: the planted ones first, then empty balls, then centres jittered around the clusters
VALUES = (0, 1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)
# neighbours (centres 2j, 2j + 1: one wave of the pair kernel) with one list on each side of a bound: 32 | 33, 64 | 65, 32 | 65, 65 | 0
NEIGHBOURS = (((32, 0), (16, 17)), ((33, 0), (0, 32)), ((64, 0), (1, 64)), ((2, 63), (32, 32)), ((32, 0), (65, 0)), ((65, 0), (0, 0)))
ORDERS = ("ascending", "descending", "shuffled")

SCALES = {
    "16+32": ((R_IN, 16), (R_OUT, 32)),          # the pyramid's pair
    "32+16 swapped": ((R_OUT, 32), (R_IN, 16)),
    "equal radii": ((R_OUT, 16), (R_OUT, 32)),
    "8+24": ((R_IN, 8), (R_OUT, 24)),
    "1+64": ((R_IN, 1), (R_OUT, 64)),
    "16+128": ((R_IN, 16), (R_OUT, 128)),        # an nsample above the 64-entry list
    "32+16 small ball": ((R_IN, 32), (R_OUT, 16)),
    "single": ((R_OUT, 32),),
}
MODES = {
    "pair": dict(EPNET_BQ_PAIR=1),
    "one centre per wave": dict(EPNET_BQ_PAIR=0),
    "streaming": dict(EPNET_BQ_PAIR=1, EPNET_BQ_STREAM=1),
}


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded(hiplib):
    assert torch.cuda.is_available()
    return hiplib


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _unit(rng, k):
    v = rng.normal(size=(k, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _plan(n, rng):
    """per scene: the list of (c_in, c_out) groups. Every value of VALUES occurs as c_in and as c_out over the B scenes, the
    NEIGHBOURS pairs stay adjacent (and start at an even centre), the rest of a scene's points goes to further random pairs"""
    need = [[(v, VALUES[(i * 7 + 3) % len(VALUES)])] for i, v in enumerate(VALUES)] + [list(p) for p in NEIGHBOURS]
    need.sort(key=lambda g: -sum(a + b for a, b in g))
    cap = n - 24                      # at least 24 background points per scene
    scenes, used = [[] for _ in range(B)], [0] * B
    for g in need:                    # largest first into the emptiest scene
        s = int(np.argmin(used))
        w = sum(a + b for a, b in g)
        assert used[s] + w <= cap, "the planted groups do not fit %d points" % n
        scenes[s].append(g)
        used[s] += w
    for s in range(B):
        while sum(len(g) for g in scenes[s]) < 120:
            g = [(int(rng.choice(VALUES[:18])), int(rng.choice(VALUES[:18])))]
            if used[s] + sum(g[0]) > cap:
                break
            scenes[s].append(g)
            used[s] += sum(g[0])
        order = rng.permutation(len(scenes[s]))
        pairs = [scenes[s][i] for i in order if len(scenes[s][i]) == 2]
        singles = [scenes[s][i] for i in order if len(scenes[s][i]) == 1]
        scenes[s] = [c for g in pairs for c in g] + [c for g in singles for c in g]   # pairs first: they start at even centres
    seen_in = {a for sc in scenes for a, _ in sc}
    seen_out = {b for sc in scenes for _, b in sc}
    assert seen_in >= set(VALUES) and seen_out >= set(VALUES)
    return scenes


def _walk_rank(geom):
    """position of every point in the sorted order of the library's scene index: (x, y, z, original index) rows, cell-sorted"""
    from epnet_amd import pointnet2_cuda as ext
    b, n = geom.shape[:2]
    index = ext.scene_index(dev(geom))
    torch.cuda.synchronize()
    np_ = 2048
    while np_ < n:
        np_ *= 2
    rows = index[:b * np_ * 16].cpu().numpy().view(np.int32).reshape(b, np_, 4)[..., 3]
    rank = np.empty((b, n), np.int64)
    for s in range(b):
        real = rows[s][rows[s] >= 0]
        assert np.array_equal(np.sort(real), np.arange(n))
        rank[s, real] = np.arange(n)
    return rank


_CLOUDS = {}


def _cloud(n):
    """xyz (B, n, 3), centres (B, M_TOTAL, 3), and what was planted: per scene (centre, c_in, c_out, order) rows"""
    if n in _CLOUDS:
        return _CLOUDS[n]
    rng = np.random.default_rng(7000 + n)
    plan = _plan(n, rng)
    geom = np.zeros((B, n, 3), np.float32)
    centres = np.zeros((B, M_TOTAL, 3), np.float32)
    members, planted = [], []
    for s in range(B):
        groups = plan[s]
        side = int(np.ceil(len(groups) ** (1.0 / 3.0)))
        pos = (np.stack(np.unravel_index(rng.permutation(side ** 3)[:len(groups)], (side,) * 3), axis=1) * PITCH).astype(np.float32)
        at, mem = 0, []
        for c, (c_in, c_out) in zip(pos, groups):
            k = c_in + c_out
            rad = np.concatenate([rng.uniform(0.05, 0.8, c_in) * R_IN, rng.uniform(1.3 * R_IN, 0.85 * R_OUT, c_out)])
            geom[s, at:at + k] = c + _unit(rng, k) * rad[:, None]
            mem.append(np.arange(at, at + k))
            at += k
        # background: off the grid diagonal, out of every ball's reach
        geom[s, at:] = pos[rng.integers(0, len(groups), n - at)] + np.float32(PITCH / 2) + rng.uniform(-0.3, 0.3, (n - at, 3))
        members.append(mem)
        g = len(groups)
        centres[s, :g] = pos
        empty = pos[rng.integers(0, g, 6)] + np.array([PITCH / 2, 0, 0], np.float32)       # no point of the cloud within R_OUT
        centres[s, g:g + 6] = empty
        rest = M_TOTAL - g - 6
        centres[s, g + 6:] = pos[rng.integers(0, g, rest)] + rng.normal(0, 0.4, (rest, 3))
        planted.append([(j, c_in, c_out, ORDERS[(j + s) % 3]) for j, (c_in, c_out) in enumerate(groups)])
    # which original indices the planted points carry, against the order the walk meets them in
    rank = _walk_rank(geom)
    xyz = np.empty_like(geom)
    for s in range(B):
        slot_of = np.full(n, -1, np.int64)
        free = rng.permutation(n)
        at = 0
        for mem, (_j, _ci, _co, order) in zip(members[s], planted[s]):
            k = len(mem)
            slots = np.sort(free[at:at + k])
            at += k
            if k == 0:
                continue
            by_walk = mem[np.argsort(rank[s, mem], kind="stable")]
            if order == "descending":
                slots = slots[::-1].copy()
            elif order == "shuffled":
                slots = rng.permutation(slots)
            low = int(np.argmin(slots))      # the smallest index goes to the point the walk meets last
            slots[low], slots[k - 1] = slots[k - 1], slots[low]
            slot_of[by_walk] = slots
        bg = np.nonzero(slot_of < 0)[0]
        slot_of[bg] = free[at:]
        assert np.array_equal(np.sort(slot_of), np.arange(n))
        xyz[s, slot_of] = geom[s]
    _CLOUDS[n] = (xyz, centres, planted)
    return _CLOUDS[n]


_WANT = {}


def _want(oracle, n, r, ns):
    key = (n, r, ns)
    if key not in _WANT:
        xyz, centres, _ = _cloud(n)
        _WANT[key] = oracle.ball_query(r, ns, xyz, centres)
        _WANT[key].setflags(write=False)
    return _WANT[key]


def _outs(m, scales):
    """idx tensors inside canaries: rows written past either end fail the case"""
    raws = [torch.full((B * m * ns + 512,), -5, dtype=torch.int32, device=DEV) for _r, ns in scales]
    return raws, [raw[256:256 + B * m * ns].view(B, m, ns) for raw, (_r, ns) in zip(raws, scales)]


def _check(oracle, n, m, scales, raws, outs, what):
    torch.cuda.synchronize()
    for raw, got, (r, ns) in zip(raws, outs, scales):
        assert bool((raw[:256] == -5).all()) and bool((raw[256 + B * m * ns:] == -5).all()), "%s: idx written out of bounds" % what
        np.testing.assert_array_equal(got.cpu().numpy(), _want(oracle, n, r, ns)[:, :m], err_msg="%s r=%g ns=%d" % (what, r, ns))


def _query(n, m, scales, mode):
    from epnet_amd import _lib, pointnet2_cuda as ext
    xyz, centres, _ = _cloud(n)
    d_xyz, d_c = dev(xyz), dev(centres[:, :m])
    index = ext.scene_index(d_xyz)
    raws, outs = _outs(m, scales)
    with _lib.tuning(**MODES[mode]):
        if len(scales) == 1:
            ext.ball_query_indexed_wrapper(B, n, m, scales[0][0], scales[0][1], d_c, d_xyz, index, outs[0])
        else:
            ext.ball_query_multi_wrapper(B, n, m, [r for r, _ in scales], [ns for _, ns in scales], d_c, d_xyz, index, outs)
    return raws, outs


def test_planted_counts_are_what_the_oracle_finds(oracle):
    """the clouds themselves: a planted centre has exactly c_in points inside R_IN and c_in + c_out inside R_OUT, the smallest
    index among them leads both rows, and the centres put between the clusters see nothing"""
    for n in (1024, 4096, 8192):
        xyz, centres, planted = _cloud(n)
        small, big = _want(oracle, n, R_IN, 400), _want(oracle, n, R_OUT, 400)
        for s in range(B):
            for j, c_in, c_out, _order in planted[s]:
                for row, k in ((small[s, j], c_in), (big[s, j], c_in + c_out)):
                    assert len(set(row.tolist())) == max(k, 1) and (k > 0 or not row.any())
                    assert (np.diff(row[:k]) > 0).all() and (row[k:] == row[0]).all()
            g = len(planted[s])
            assert not big[s, g:g + 6].any()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("scales", list(SCALES))
@pytest.mark.parametrize("n", [1024, 4096, 8192])   # one level of boxes (1 and 2 bitmap dwords per lane), two levels
def test_lists_match_oracle(oracle, n, scales, mode):
    sc = SCALES[scales]
    raws, outs = _query(n, M_TOTAL, sc, mode)
    _check(oracle, n, M_TOTAL, sc, raws, outs, "n=%d %s, %s" % (n, scales, mode))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("m", [1, 7, 257])
@pytest.mark.parametrize("n", [1024, 8192])
def test_odd_centre_counts(oracle, n, m, mode):
    """the last wave of a scene serves one centre: its second row is the next scene's first (or past the tensor)"""
    for scales in ("16+32", "8+24", "single"):
        sc = SCALES[scales]
        raws, outs = _query(n, m, sc, mode)
        _check(oracle, n, m, sc, raws, outs, "n=%d m=%d %s, %s" % (n, m, scales, mode))


@pytest.mark.parametrize("scales", ["16+32", "32+16 swapped", "1+64", "16+128", "single"])
@pytest.mark.parametrize("n", [1024, 4096, 8192])
def test_ordered_variant(oracle, n, scales):
    """epnet_ball_query_ordered: the two centres of a wave are neighbours in the centres' own index and their rows are not adjacent"""
    from epnet_amd import _lib, pointnet2_cuda as ext
    sc = SCALES[scales]
    xyz, centres, _ = _cloud(n)
    d_xyz, d_c = dev(xyz), dev(centres)
    index, centre_index = ext.scene_index(d_xyz), ext.scene_index(d_c)
    assert index is not None and centre_index is not None
    raws, outs = _outs(M_TOTAL, sc)
    with _lib.tuning(EPNET_BQ_ORDERED=1, EPNET_BQ_PAIR=1):
        ext.ball_query_ordered_wrapper(B, n, M_TOTAL, [r for r, _ in sc], [ns for _, ns in sc], d_c, d_xyz, index, centre_index, outs)
    _check(oracle, n, M_TOTAL, sc, raws, outs, "ordered n=%d %s" % (n, scales))

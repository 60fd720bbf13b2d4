"""A seeded sweep of the deterministic gradients (include/epnet_ops.h, "*_det") around the boundaries of
their own kernels, which tests/test_deterministic_gpu.py's hand-picked cases do not reach:
  * radix passes: one per byte of n - 1 targets (0 for n = 1, then 1 / 2 / 3 / 4 above 1, 256, 65536, 2^24);
  * sort tiles of 4096 entries and the scan of 256 * tiles counts in segments over 1024 threads;
  * fold rows of 8 channels; group_linear_grad_w's 4096-position tiles and 8-row chunks;
  * 1 to 257 scenes; index families that stress the sort (permutations, one hot target, sparse targets, ascending and
    descending order, targets that share their low byte, padding runs, indices outside [0, n)); sampler coordinates that give
    zero-weight taps, the map's edges, one ulp past them, far outside, infinite and NaN.
Every case starts from a buffer with -0.0 entries and large magnitudes, so that a skipped zero term or a reordered fold changes
bits. Each is checked bit for bit against the contract (the oracle's loops, or tests/det_restate.py) and against a float64
yardstick (test_gpu_sweep.assert_scatter_sum's bound), so that a kernel and a restatement wrong the same way cannot pass.
Also the model's two 3-pass sampler shapes (rpn_backbone.py: LI-Fusion level 1 and the final fusion).

The generator is seeded: the same cases every run (a failure names its case, which can be replayed alone with -k)."""
import numpy as np
import pytest
import torch

import det_restate as R
from conftest import GuardedAlloc
from test_deterministic_gpu import (deterministic, oracle_gather_grad, oracle_group_grad, oracle_interp_grad, same_bits,
                                    skewed_index, unaligned)
from test_gpu_sweep import assert_scatter_sum

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE = R.TILE
OPS = ("gather_points_grad", "group_points_grad", "group_concat_grad", "three_interpolate_grad", "feature_gather_grad",
       "group_linear_grad_w")
# targets n on both sides of every pass-count boundary (0 | 1 | 2 | 3 | 4 passes), and near 2^17
N_EDGES = (1, 2, 255, 256, 257, 65535, 65536, 65537, 131073, 1 << 24, (1 << 24) + 1)
PASS_BOUNDARIES = ((1, 2), (256, 257), (65536, 65537), (1 << 24, (1 << 24) + 1))
# entries per scene: one tile, the tile's edges, k tiles +- 1, tile counts whose 256 * tiles scan counts split unevenly over the
# 1024 scan threads (5, 7, 13 tiles), and about 10^6 (245 tiles)
P_EDGES = (1, 4095, 4096, 4097, 2 * TILE - 1, 2 * TILE + 1, 5 * TILE - 1, 7 * TILE + 1, 13 * TILE - 1, 1000003)
FAMILIES = ("uniform", "perm", "one", "sparse", "pad", "ascending", "descending", "low_byte", "out_of_range")
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1


def ceil_div(a, b):
    return -(-a // b)


def passes_of(n):
    """radix passes of the det sort for n targets (csrc/det.hip passes_of)"""
    return (int(n - 1).bit_length() + 7) // 8


# ---- the generator ---------------------------------------------------------------------------------------------------------------
# (n, p, c, b, family) before the op's own rounding of p; every op gets all of them (the boundaries), then seeded random ones
ANCHORS = (
    (1, 4097, 7, 2, "uniform"),                     # 0 passes, 2 tiles
    (2, 4095, 9, 3, "ascending"),                   # 1 pass, 1 tile
    (255, 1, 8, 1, "uniform"),
    (256, 4096, 17, 2, "descending"),
    (257, 2 * TILE + 1, 1, 17, "low_byte"),         # 2 passes, 3 tiles
    (65535, 5 * TILE - 1, 9, 2, "sparse"),          # 5 tiles: uneven scan segments
    (65536, 65536, 8, 1, "perm"),                   # every target hit once
    (65537, 7 * TILE + 1, 7, 1, "descending"),      # 3 passes
    (131073, 1000003, 1, 1, "uniform"),             # about 10^6 entries
    (1 << 24, 4097, 1, 1, "sparse"),                # 3 passes, the largest
    ((1 << 24) + 1, 4095, 1, 1, "out_of_range"),    # 4 passes
    ((1 << 24) + 1, 2 * TILE - 1, 2, 1, "low_byte"),
    (4096, 4097, 300, 1, "pad"),                    # >= 256 channels
    (1000, 1, 1, 255, "one"),                       # 255 - 257 scenes
    (3000, 4095, 9, 256, "uniform"),
    (777, 13 * TILE - 1, 9, 257, "out_of_range"),
    (20000, 13 * TILE - 1, 17, 3, "one"),           # one target receiving every entry of 13 tiles
    (300000, 2 * TILE + 1, 8, 2, "low_byte"),       # 3 passes, stability across them
)
C_CHOICES = (1, 7, 8, 9, 17, 33, 256)
B_CHOICES = (1, 2, 3, 17)


def _budget(op, n, p, c, b):
    """keeps the host-side contract and yardstick of one case small"""
    if n >= 1 << 22:
        b, c, p = 1, min(c, 2), min(p, 2 * TILE)
    if b >= 255:
        c, p, n = min(c, 9), min(p, 13 * TILE), min(n, 4096)
    while b * c * max(p, n) > 2e7 and c > 1:
        c = max(1, c // 2)
    while b * c * max(p, n) > 2e7 and b > 1:
        b = max(1, b // 2)
    if op == "group_linear_grad_w":
        while b * c * p > 4e6 and c > 1:
            c = max(1, c // 2)
        p = min(p, int(4e6) // (b * c))
    return n, p, c, b


def _shape(op, n, p):
    """(p, npoints, nsample) of an op for a wanted entry count p: group ops factor p = npoints * nsample, three_interpolate has
    3 entries per unknown, the sampler 4 per point (rounded up, so that a count past a tile boundary stays past it)"""
    if op in ("three_interpolate_grad", "feature_gather_grad"):
        k = 3 if op == "three_interpolate_grad" else 4
        npts = ceil_div(max(p, 1), k)
        return npts * k, npts, 1
    ns = next((d for d in (64, 32, 17, 16, 7, 5, 3) if p % d == 0 and p // d >= 1), 1)
    if op == "gather_points_grad":
        ns = 1
    return p, p // ns, ns


def _hw(n):
    """a map of h * w = n pixels, as square as n's divisors allow"""
    h = max(d for d in range(1, int(np.sqrt(n)) + 1) if n % d == 0) if n < 1 << 26 else 1
    return h, n // h


def _case_list(seed=29, random_per_op=10):
    rng = np.random.default_rng(seed)
    out = []
    for k_op, op in enumerate(OPS):
        specs = list(ANCHORS)
        for _ in range(random_per_op):
            specs.append((int(np.exp(rng.uniform(0, np.log(1 << 20)))), int(np.exp(rng.uniform(0, np.log(3e5)))),
                          int(rng.choice(C_CHOICES)), int(rng.choice(B_CHOICES)), FAMILIES[int(rng.integers(0, len(FAMILIES)))]))
        for j, (n, p, c, b, fam) in enumerate(specs):
            if op == "group_linear_grad_w" and fam == "out_of_range":
                fam = "uniform"                        # (its indices must be valid: they address xyz)
            if fam == "perm":
                p = n
            n, p, c, b = _budget(op, n, p, c, b)
            p, npts, ns = _shape(op, n, p)
            flag = bool((j + k_op) % 2)                # use_xyz / align_corners, where the op has one
            out.append(dict(i=len(out), op=op, n=n, p=p, npts=npts, ns=ns, c=c, b=b, family=fam, flag=flag,
                            unaligned=(j + k_op) % 4 == 3, seed=1000 + len(out)))
    return out


CASES = _case_list()


def case_id(cs):
    return "case%03d_%s_n%d_p%d_c%d_b%d_%s%s" % (cs["i"], cs["op"], cs["n"], cs["p"], cs["c"], cs["b"], cs["family"],
                                                  ("_flag" if cs["flag"] else "") + ("_unaligned" if cs["unaligned"] else ""))


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def index_family(r, fam, b, p, n, ns):
    """(b, p) int32 targets of one family"""
    if fam == "perm":                                     # (p rounded up to 3 or 4 entries a unit: the last few uniform)
        return np.stack([np.concatenate([r.permutation(n), r.integers(0, n, size=max(0, p - n))])[:p] for _ in range(b)]).astype(np.int32)
    if fam == "one":
        return np.repeat(r.integers(0, n, size=(b, 1)), p, axis=1).astype(np.int32)
    if fam == "sparse":                                   # a few hundred targets at most, the rest stay empty
        pool = r.integers(0, n, size=(b, min(n, 300)))
        return np.take_along_axis(pool, r.integers(0, pool.shape[1], size=(b, p)), axis=1).astype(np.int32)
    if fam == "pad":
        return skewed_index(r, b, p, n, pad_runs=ns > 1, ns=ns)
    idx = r.integers(0, n, size=(b, p)).astype(np.int64)
    if fam == "ascending":
        idx.sort(axis=1)
    elif fam == "descending":
        idx = -np.sort(-idx, axis=1)
    elif fam == "low_byte":                               # multiples of 256 plus one shared low byte per scene
        low = r.integers(0, min(n, 256), size=(b, 1))
        idx = np.minimum((idx // 256) * 256 + low, n - 1)
    elif fam == "out_of_range":
        bad = r.random((b, p)) < 0.01
        bad[:, 0] = True
        idx[bad] = r.choice(np.array([-1, n, INT_MAX, INT_MIN], np.int64), size=int(bad.sum()))
    return idx.astype(np.int32)


def start_buffer(r, b, c, n, flat, zero_targets=None):
    """a nonzero (b, c, n) starting buffer: -0.0 at a few targets (and at `zero_targets`, (b, n) bool), +-1e5 at a few targets
    that receive at most 64 entries (where the float64 bound still holds)"""
    s = r.standard_normal((b, c, n), dtype=np.float32)
    for bi in range(b):
        f = flat[bi]
        counts = np.bincount(f[(f >= 0) & (f < n)].astype(np.int64), minlength=n)
        big = (r.random(n) < 0.02) & (counts <= 64)
        s[bi][:, big] = np.float32(1e5) * np.sign(s[bi][:, big])
        neg0 = r.random(n) < 0.05
        if zero_targets is not None:
            neg0 |= zero_targets[bi]
        s[bi][:, neg0] = np.float32(-0.0)
    return s


def zero_term_targets(r, flat, n):
    """(b, n) bool: about 5% of the targets that some entry hits a few times (<= 8), whose terms the case makes +-0"""
    b = flat.shape[0]
    z = np.zeros((b, n), bool)
    for bi in range(b):
        f = flat[bi]
        counts = np.bincount(f[(f >= 0) & (f < n)].astype(np.int64), minlength=n)
        few = np.flatnonzero((counts > 0) & (counts <= 8))
        if len(few) >= 4:
            z[bi, r.choice(few, size=max(1, len(few) // 20), replace=False)] = True
    return z


def entry_mask(flat, targets_mask):
    """(b, p) bool: the entries whose target is marked in targets_mask (b, n)"""
    n = targets_mask.shape[1]
    ok = (flat >= 0) & (flat < n)
    out = np.zeros(flat.shape, bool)
    for bi in range(flat.shape[0]):
        out[bi, ok[bi]] = targets_mask[bi, flat[bi, ok[bi]].astype(np.int64)]
    return out


def sampler_xy(r, fam, b, npts, h, w, align_corners):
    """(b, npts, 2) float32: the bulk by family, then exact-pixel points (zero-weight in-bounds taps), the map's edges, one ulp
    past them, far outside / infinite / NaN"""
    f32 = np.float32
    xy = r.uniform(-1.1, 1.1, size=(b, npts, 2)).astype(f32)
    if fam == "sparse":
        xy = (r.uniform(-0.02, 0.02, size=(b, npts, 2)) + r.uniform(-0.9, 0.9, size=(b, 1, 2))).astype(f32)
    elif fam in ("ascending", "descending"):
        xy.sort(axis=1)
        if fam == "descending":
            xy = np.ascontiguousarray(xy[:, ::-1])
    # points on pixel positions: ix (iy) an exact integer for many of them, so that the taps at x0 + 1 (y0 + 1) weigh 0
    kx, ky = r.integers(0, w, size=(b, npts)), r.integers(0, h, size=(b, npts))
    if align_corners:
        ex = np.where(w > 1, 2.0 * kx / max(w - 1, 1) - 1.0, 0.0)
        ey = np.where(h > 1, 2.0 * ky / max(h - 1, 1) - 1.0, 0.0)
    else:
        ex, ey = (2.0 * kx + 1.0) / w - 1.0, (2.0 * ky + 1.0) / h - 1.0
    exact = r.random((b, npts)) < (0.6 if fam in ("perm", "pad", "low_byte") else 0.2)
    xy[..., 0] = np.where(exact & (r.random((b, npts)) < 0.7), ex, xy[..., 0])
    xy[..., 1] = np.where(exact & (r.random((b, npts)) < 0.7), ey, xy[..., 1])
    if fam == "one":                                       # many points on one pixel
        xy[:, : max(1, npts // 2)] = xy[:, :1]
    one_up, one_dn = np.nextafter(f32(1), f32(2)), np.nextafter(f32(-1), f32(-2))
    special = [(-1, -1), (1, 1), (-1, 1), (1, -1), (-1, 0.3), (0.3, 1), (0, 0), (one_up, 0.2), (one_dn, -0.4), (0.1, one_up),
               (-0.7, one_dn), (one_up, one_dn), (1e30, 0), (0, -1e30), (np.inf, 0.5), (-np.inf, -np.inf), (np.nan, 0.1),
               (0.2, np.nan)]
    for k, v in enumerate(special[: npts // 4]):
        xy[k % b, 1 + k] = v
    return np.ascontiguousarray(xy, f32)


# ---- the case runner -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def _lib_loaded(hiplib):
    assert torch.cuda.is_available()
    return hiplib


@pytest.fixture
def outputs():
    """the outputs handed to the wrappers, with a canary on either side (the library's own allocations, the det workspace among
    them, are guarded by conftest's autouse fixture)"""
    g = GuardedAlloc()
    yield g
    torch.cuda.synchronize()
    g.check()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def in_(a, cs):
    """a device input, 4 bytes off a 16-byte boundary on the cases that ask for it"""
    return unaligned(a) if cs["unaligned"] and a.dtype == np.float32 else dev(a)


def out_tensor(g, start):
    t = g.alloc(start.shape, torch.float32, DEV)
    t.copy_(torch.from_numpy(np.ascontiguousarray(start, np.float32)))
    return t


def yardstick(got, start, terms, flat, n):
    """assert_scatter_sum with the starting buffer as each target's first term, over the targets that some entry hits (the others
    are the starting buffer, bit for bit, by the contract check); entries outside [0, n) add nothing"""
    b, c = start.shape[:2]
    ok = (flat >= 0) & (flat < n)
    hit = np.unique(flat[ok]).astype(np.int64)
    if hit.size == 0:
        return
    pos = np.searchsorted(hit, np.where(ok, flat, hit[0]))
    terms = np.where(ok[:, None, :], terms, np.float32(0)).astype(np.float32)
    lead = np.broadcast_to(np.arange(hit.size, dtype=np.int64), (b, hit.size))
    s0 = start.reshape(b, c, n)[:, :, hit]
    assert_scatter_sum(got.reshape(b, c, n)[:, :, hit], np.concatenate([s0, terms], axis=2), np.concatenate([lead, pos], axis=1),
                       hit.size)


def run_scatter_case(cs, oracle, g):
    from epnet_amd import pointnet2_cuda as ext
    op, b, c, n, p, m, ns = cs["op"], cs["b"], cs["c"], cs["n"], cs["p"], cs["npts"], cs["ns"]
    r = np.random.default_rng(cs["seed"])
    flat = index_family(r, cs["family"], b, p, n, 3 if op == "three_interpolate_grad" else ns)
    oor = bool(((flat < 0) | (flat >= n)).any())
    zt = zero_term_targets(r, flat, n)
    zero_entries = entry_mask(flat, zt)
    start = start_buffer(r, b, c, n, flat, zt)
    if op == "three_interpolate_grad":
        idx = flat.reshape(b, m, 3)
        go = r.standard_normal((b, c, m), dtype=np.float32)
        w = r.random((b, m, 3), dtype=np.float32)
        w[r.random((b, m, 3)) < 0.02] = 0.0                # zero-weight entries: +-0 terms
        w = np.where(zero_entries.reshape(b, m, 3), np.float32(0), w).astype(np.float32)
        gp = out_tensor(g, start)
        with deterministic():
            ext.three_interpolate_grad_wrapper(b, c, m, n, in_(go, cs), dev(idx), in_(w, cs), gp)
        got = gp.cpu().numpy()
        same_bits(got, R.three_interpolate_grad(start, go, idx, w) if oor else oracle_interp_grad(oracle, start, go, idx, w))
        terms = (go[:, :, :, None] * w[:, None, :, :]).reshape(b, c, p)
        yardstick(got, start, terms, flat, n)
        return
    go = r.standard_normal((b, c, p), dtype=np.float32)
    go[:, :, r.random(p) < 0.01] = 0.0
    go = np.where(zero_entries[:, None, :], np.float32(0), go).astype(np.float32)   # +0 terms onto -0.0 targets
    gp = out_tensor(g, start)
    if op == "gather_points_grad":
        with deterministic():
            ext.gather_points_grad_wrapper(b, c, n, p, in_(go, cs), dev(flat), gp)
        want = R.gather_points_grad(start, go, flat) if oor else oracle_gather_grad(oracle, start, go, flat)
    else:
        idx = flat.reshape(b, m, ns)
        go4 = go.reshape(b, c, m, ns)
        with deterministic():
            if op == "group_points_grad":
                ext.group_points_grad_wrapper(b, c, n, m, ns, in_(go4, cs), dev(idx), gp)
            else:
                ch0 = 3 if cs["flag"] else 0
                full = np.full((b, ch0 + c, m, ns), np.float32(1e30))       # the xyz rows must not be read: huge if they are
                full[:, ch0:] = go4
                ext.group_concat_grad_wrapper(b, c, n, m, ns, in_(full, cs), dev(idx), gp, cs["flag"])
        want = R.group_points_grad(start, go4, idx) if oor else oracle_group_grad(oracle, start, go4, idx)
    got = gp.cpu().numpy()
    same_bits(got, want)
    yardstick(got, start, go, flat, n)


def run_sampler_case(cs, g):
    from epnet_amd import pointnet2_cuda as ext
    b, c, n, npts = cs["b"], cs["c"], cs["n"], cs["npts"]
    align = cs["flag"]
    h, w = _hw(n)
    r = np.random.default_rng(cs["seed"])
    xy = sampler_xy(r, cs["family"], b, npts, h, w, align)
    pix, wts = R.taps(xy, h, w, align)
    flat = pix.reshape(b, npts * 4)
    # -0.0 at the pixels that only zero-weight in-bounds taps reach: a tap skipped there leaves the sign bit set
    zero_only = np.zeros((b, n), bool)
    for bi in range(b):
        zero_only[bi, pix[bi][(pix[bi] >= 0) & (wts[bi] == 0)]] = True
        zero_only[bi, pix[bi][(pix[bi] >= 0) & (wts[bi] != 0)]] = False
    start = start_buffer(r, b, c, n, flat, zero_only)
    go = r.standard_normal((b, c, npts), dtype=np.float32)
    gm = out_tensor(g, start.reshape(b, c, h, w))
    with deterministic():
        ext.feature_gather_grad_wrapper(b, c, h, w, npts, align, in_(go, cs), in_(xy, cs), gm)
    got = gm.cpu().numpy()
    same_bits(got, R.feature_gather_grad(start.reshape(b, c, h, w), go, xy, align))
    terms = (go[:, :, :, None] * wts[:, None, :, :]).astype(np.float32).reshape(b, c, npts * 4)
    yardstick(got, start, terms, flat, n)


def run_linear_case(cs, g):
    from epnet_amd import pointnet2_cuda as ext, synth
    b, c, n, m, ns = cs["b"], cs["c"], cs["n"], cs["npts"], cs["ns"]
    r = np.random.default_rng(cs["seed"])
    xyz = synth.scenes("kitti", b, n, seed=cs["seed"]).numpy() if n <= 1 << 20 else r.uniform(-40, 40, size=(b, n, 3)).astype(np.float32)
    new_xyz = np.ascontiguousarray(xyz[:, r.integers(0, n, size=m)])
    idx = index_family(r, cs["family"], b, m * ns, n, ns).reshape(b, m, ns)
    go = r.standard_normal((b, c, m, ns), dtype=np.float32)
    go[:, :, r.random((m, ns)) < 0.01] = 0.0
    start = r.standard_normal((c, 3), dtype=np.float32)
    start[r.random((c, 3)) < 0.1] = -0.0
    start[r.random((c, 3)) < 0.05] = 1e4
    gw = out_tensor(g, start)
    with deterministic():
        ext.group_linear_grad_w_wrapper(b, c, n, m, ns, in_(go, cs), in_(xyz, cs), dev(new_xyz), dev(idx), gw)
    got = gw.cpu().numpy()
    same_bits(got, R.group_linear_grad_w(start, go, xyz, new_xyz, idx))
    # test_gpu_sweep.test_sweep_group_linear's bound against a float64 einsum, the starting buffer included
    rel = xyz.astype(np.float64)[np.arange(b)[:, None, None], idx.astype(np.int64)] - new_xyz[:, :, None, :].astype(np.float64)
    want = start + np.einsum("bcms,bmsk->ck", go.astype(np.float64), rel)
    mag = np.abs(start) + np.einsum("bcms,bmsk->ck", np.abs(go).astype(np.float64), np.abs(rel))
    assert (np.abs(got - want) <= 3e-7 * mag + 1e-5).all(), float(np.abs(got - want).max())


@pytest.mark.parametrize("cs", CASES, ids=case_id)
def test_det_sweep(cs, oracle, outputs):
    if cs["op"] == "feature_gather_grad":
        run_sampler_case(cs, outputs)
    elif cs["op"] == "group_linear_grad_w":
        run_linear_case(cs, outputs)
    else:
        run_scatter_case(cs, oracle, outputs)


# ---- empty problems ----------------------------------------------------------------------------------------------------------------
EMPTY = [(op, z) for op in OPS for z in ("b", "c", "p", "n") if not (z == "n" and op in ("feature_gather_grad", "group_linear_grad_w"))]


@pytest.mark.parametrize("op,zero", EMPTY, ids=["%s-%s0" % e for e in EMPTY])
def test_det_empty_problem_leaves_the_output_alone(op, zero, outputs):
    """b, c, the entries (npoints / unknowns / points) or the targets n = 0: the call succeeds and writes nothing"""
    from epnet_amd import pointnet2_cuda as ext
    d = dict(b=2, c=5, n=7, m=3, ns=2)
    d[{"p": "m"}.get(zero, zero)] = 0
    b, c, n, m, ns = d["b"], d["c"], d["n"], d["m"], d["ns"]
    r = np.random.default_rng(len(op) + ord(zero))

    def inp(*shape, ints=False):
        k = max(1, int(np.prod(shape)))
        return dev(r.integers(0, max(n, 1), size=k).astype(np.int32) if ints else r.standard_normal(k, dtype=np.float32))
    h, w = 3, 4
    size = {"group_linear_grad_w": c * 3, "feature_gather_grad": b * c * h * w}.get(op, b * c * n)
    fill = r.standard_normal(size + 64, dtype=np.float32)         # (more than the call may touch)
    fill[::5] = -0.0
    out = out_tensor(outputs, fill)
    with deterministic():
        if op == "gather_points_grad":
            ext.gather_points_grad_wrapper(b, c, n, m, inp(b, c, m), inp(b, m, ints=True), out)
        elif op == "group_points_grad":
            ext.group_points_grad_wrapper(b, c, n, m, ns, inp(b, c, m, ns), inp(b, m, ns, ints=True), out)
        elif op == "group_concat_grad":
            ext.group_concat_grad_wrapper(b, c, n, m, ns, inp(b, 3 + c, m, ns), inp(b, m, ns, ints=True), out, True)
        elif op == "three_interpolate_grad":          # (the entries are the unknowns m * 3 here, the targets n known points)
            ext.three_interpolate_grad_wrapper(b, c, m, n, inp(b, c, m), inp(b, m, 3, ints=True), inp(b, m, 3), out)
        elif op == "feature_gather_grad":
            ext.feature_gather_grad_wrapper(b, c, h, w, m, True, inp(b, c, m), inp(b, m, 2), out)
        else:
            ext.group_linear_grad_w_wrapper(b, c, max(n, 1), m, ns, inp(b, c, m, ns), inp(b, max(n, 1), 3), inp(b, m, 3),
                                            inp(b, m, ns, ints=True), out)
    same_bits(out.cpu().numpy(), fill)


# ---- the model's sampler shapes ----------------------------------------------------------------------------------------------------
IMAGE_SIZE = (1280, 384)          # (width, height): rpn_backbone.py normalises pixel coordinates by image_size - 1
MODEL_SHAPES = {
    # name: (channels, h, w, points picked through the FPS index or None): LI-Fusion level 1 samples Img_Block[0]'s half-size map
    # at the 4096 FPS points of the 16384; the final fusion samples the full-size map at all 16384 points
    "level1": (64, 192, 640, 4096),
    "final": (128, 384, 1280, None),
}
F64_CHANNELS = 16                 # (the float64 grid_sample yardstick on a slice of the channels: host memory)


def model_inputs(name, b=2, n_src=16384):
    """(xy (b, n_src, 2) normalised as rpn_backbone.py:189-190 does, fps_idx (b, m) int32 or None, the picked xy)"""
    from epnet_amd import pointnet2_utils as p2u, synth
    c, h, w, m = MODEL_SHAPES[name]
    g = torch.Generator().manual_seed(len(name))
    pix = torch.rand((b, n_src, 2), generator=g) * torch.tensor([IMAGE_SIZE[0] - 1.0, IMAGE_SIZE[1] - 1.0])
    pix[:, ::5] = pix[:, ::5].round()                                # whole pixels
    pix[:, 1::97] = pix[:, 1:2]                                      # many points on one pixel
    xy = pix.clone()
    xy[:, :, 0] = xy[:, :, 0] / (IMAGE_SIZE[0] - 1.0) * 2.0 - 1.0
    xy[:, :, 1] = xy[:, :, 1] / (IMAGE_SIZE[1] - 1.0) * 2.0 - 1.0
    if m is None:
        return xy, None, xy
    fps_idx = p2u.furthest_point_sample(synth.scenes("kitti", b, n_src, seed=41).to(DEV), m)
    picked = torch.gather(xy, 1, fps_idx.long().cpu().unsqueeze(-1).expand(-1, -1, 2))
    return xy, fps_idx, picked


def grid_sample_f64(start, go, xy, align_corners):
    """start + the float64 gradient of grid_sample (bilinear, zero padding) w.r.t. its map, for the first F64_CHANNELS channels"""
    import torch.nn.functional as F
    b, _, h, w = start.shape
    k = min(F64_CHANNELS, start.shape[1])
    fm = torch.zeros((b, k, h, w), dtype=torch.float64, requires_grad=True)
    out = F.grid_sample(fm, xy.double().unsqueeze(1), mode="bilinear", padding_mode="zeros", align_corners=align_corners)
    grad, = torch.autograd.grad(out, fm, torch.from_numpy(go[:, :k]).double().unsqueeze(2))
    return start[:, :k].astype(np.float64) + grad.numpy()


@pytest.mark.parametrize("align_corners", [True, False])
@pytest.mark.parametrize("name", list(MODEL_SHAPES))
def test_model_sampler_shapes(name, align_corners, outputs):
    """feature_gather_grad under the flag at the model's two sampler shapes (122 880 and 491 520 targets: 3 radix passes): bit
    for bit the restatement, and within test_gpu_sweep.test_sweep_feature_gather's bound of float64 grid_sample"""
    from epnet_amd import pointnet2_cuda as ext
    c, h, w, _ = MODEL_SHAPES[name]
    assert passes_of(h * w) == 3
    _, _, picked = model_inputs(name)
    b, n = picked.shape[:2]
    xy = np.ascontiguousarray(picked.numpy())
    r = np.random.default_rng(h + align_corners)
    go = r.standard_normal((b, c, n), dtype=np.float32)
    start = r.standard_normal((b, c, h, w), dtype=np.float32)
    start[:, :, ::3, ::7] = -0.0
    gm = out_tensor(outputs, start)
    with deterministic():
        ext.feature_gather_grad_wrapper(b, c, h, w, n, align_corners, dev(go), dev(xy), gm)
    got = gm.cpu().numpy()
    same_bits(got, R.feature_gather_grad(start, go, xy, align_corners))
    want = grid_sample_f64(start, go, picked, align_corners)
    scale = max(1.0, float(np.abs(want).max()))
    np.testing.assert_allclose(got[:, :want.shape[1]], want, rtol=1e-4, atol=(1e-4 if align_corners else 1e-3) * scale)


def test_level1_sampler_through_feature_gather_and_autograd():
    """li_fusion.Feature_Gather(fmap, xy, fps_idx) as LI-Fusion level 1 calls it: the backward scatters at the gathered xy"""
    from epnet_amd import li_fusion
    c, h, w, _ = MODEL_SHAPES["level1"]
    xy, fps_idx, picked = model_inputs("level1")
    b, n = picked.shape[:2]
    r = np.random.default_rng(5)
    fmap_h = r.standard_normal((b, c, h, w), dtype=np.float32)
    go = r.standard_normal((b, c, n), dtype=np.float32)
    with deterministic():
        fmap = dev(fmap_h).requires_grad_(True)
        out, got_xy = li_fusion.Feature_Gather(fmap, xy.to(DEV), fps_idx)
        (out * dev(go)).sum().backward()
    same_bits(got_xy.cpu().numpy(), picked.numpy())
    same_bits(fmap.grad.cpu().numpy(), R.feature_gather_grad(np.zeros_like(fmap_h), go, picked.numpy(), True))

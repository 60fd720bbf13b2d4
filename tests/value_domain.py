"""TEST INFRASTRUCTURE (numpy only): the input domain D of the spatial ops -- every finite float32 cloud with |coordinate| <= 2^62
-- as a table of transforms of three metre-scale base clouds, for tests/test_value_domain.py (the oracle against its closed forms,
here) and tests/test_value_domain_gpu.py (the kernels against the oracle).

Inside D a difference is at most 2^63 and a squared distance at most 3 * 2^126 < 2^128: the reference's arithmetic stays finite.
The lower end is open: denormal distances and distances that underflow to zero belong to D.

Base clouds (float32, seeded, b = 2): ``kitti`` and ``dup`` of epnet_amd.synth (dup: a quarter of the rows are re-drawn twins),
``lattice`` = quarter-metre grid points in random order (exact ties between distinct points).

A transform maps a base cloud to ``(xyz, scale)`` in float32; radii and box sizes of a case are multiplied by the same ``scale``
in float32 (``radii``). ``fps``: what the oracle's furthest point sampling of the transformed ``kitti`` cloud must show against the
base cloud's -- "equal" (same indices), "differs" (a regime of its own; a table that
quietly produced the base cloud again would pass everything) or None (not recorded). ``EXACT`` names the scalings that neither
underflow nor clamp: there every distance is the base cloud's times scale^2, bit for bit.

The issue that asked for this table named ``s+14`` the largest power of two at which no kitti distance reaches the 1e10 start
value. It is not: the largest squared distance of the kitti cloud is about 6400 = 2^12.6 and 1e10 = 2^33.2, so the largest such
power is 2^10, and that is what ``s+10`` is, with the claim asserted (``no_clamp``). ``s+14`` stays in the table as what it really is:
the far rounds clamp at 1e10 and tie, the near ones do not.
"""
import functools
from collections import namedtuple

import numpy as np

F = np.float32
B = 2
BASES = ("kitti", "dup", "lattice")
LIMIT = F(2.0 ** 62)        # D: |coordinate| <= LIMIT
START = F(1e10)             # the running distance every sampling starts from (pointnet2_utils.py:26)


def p2(k):
    """2^k as a float32 (exact for -149 <= k <= 127)"""
    v = F(2.0 ** k)
    assert v > 0 and np.isfinite(v)
    return v


# ---- base clouds ------------------------------------------------------------------------------------------------------------------
def _lattice(n, rng):
    side = int(np.ceil(n ** (1.0 / 3.0))) + 1
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 3).astype(F)
    return g[rng.permutation(len(g))[:n]] * F(0.25)


@functools.lru_cache(maxsize=None)
def base_cloud(kind, n, seed=1):
    """(B, n, 3) float32, read-only (shared between the tests)"""
    from epnet_amd import synth
    if kind == "kitti":
        xyz = synth.scenes("kitti", B, n, seed=seed).numpy()
    elif kind == "dup":
        xyz = np.stack([synth.dup_cloud(n, seed + i, unique=max(1, (n * 3) // 4)).numpy() for i in range(B)])
    elif kind == "lattice":
        rng = np.random.default_rng([seed, n])
        xyz = np.stack([_lattice(n, rng) for _ in range(B)])
    else:
        raise ValueError(kind)
    xyz = np.ascontiguousarray(xyz, F)
    assert xyz.shape == (B, n, 3)
    xyz.setflags(write=False)
    return xyz


def extent(kind, n, seed=1):
    """the largest side of the bounding box of scene 0 of the base cloud, float32"""
    return F(np.ptp(base_cloud(kind, n, seed)[0], axis=0).max())


# ---- transforms -------------------------------------------------------------------------------------------------------------------
Transform = namedtuple("Transform", "name fn fps reaches")


def _scale(k, clip=False):
    def fn(xyz):
        out = xyz * p2(k)
        if clip:
            out = np.clip(out, -LIMIT, LIMIT)
        return out, p2(k)
    return fn


def _shift(k, axes=(0, 1, 2), sign=1.0):
    def fn(xyz):
        out = xyz.copy()
        out[..., list(axes)] = out[..., list(axes)] + F(sign) * p2(k)
        return out, F(1.0)
    return fn


def _aniso(xyz):
    # (the scale of the radii follows the axis that carries every cell bit: a ball then still holds neighbours)
    return xyz * np.array([p2(40), p2(-30), F(1.0)], F), p2(40)


def _outliers(xyz):
    out = xyz.copy()
    out[:, ::500] = out[:, ::500] * p2(55)
    return out, F(1.0)


def _denorm_mix(xyz):
    # s-70, then the odd rows back by 2^70 (exact both ways): metre-scale rows among rows whose mutual distances are denormal. The
    # radii keep the scale of s-70, so r^2 is denormal too
    out = xyz * p2(-70)
    out[:, 1::2] = out[:, 1::2] * p2(70)
    return out, p2(-70)


TRANSFORMS = (
    Transform("s-90", _scale(-90), "differs", "every squared distance is 0: everything ties, r^2 = 0 and every ball is empty"),
    Transform("s-75", _scale(-75), "differs", "denormal distances with lost bits: new ties"),
    Transform("s-70", _scale(-70), "equal", "denormal distances (2^-140 .. 2^-127, low bits lost): still the base order on kitti"),
    Transform("s-40", _scale(-40), "equal", "exact scaling, tiny extents in the cell grid"),
    Transform("s+10", _scale(10), "equal", "the largest power of two at which no kitti distance reaches 1e10 (asserted): no clamp"),
    Transform("s+14", _scale(14), "differs", "distances beyond 1e10 clamp and tie, the nearer ones do not"),
    Transform("s+20", _scale(20), "differs", "every distance between distinct points clamps at 1e10: rank-only rounds"),
    Transform("s+60", _scale(60, clip=True), "differs", "the top of D, clipped to +-2^62: d up to 3 * 2^126"),
    Transform("t+17", _shift(17), None, "global-frame coordinates, quantised to 2^-6"),
    Transform("t+20", _shift(20), None, "quantised to 1/8: twins"),
    Transform("t+23", _shift(23), None, "quantised to 1: a lattice of twins and exact ties"),
    Transform("t+24", _shift(24), None, "quantised to 2"),
    Transform("t-24", _shift(24, axes=(0,), sign=-1.0), None, "a negative lower corner, quantisation on x alone"),
    Transform("aniso", _aniso, None, "x * 2^40, y * 2^-30: every cell bit on one axis, extent / cell is 0 on the others"),
    Transform("outliers", _outliers, None, "every 500th row * 2^55: the bulk in one cell, bucket boxes 2^60 wide, the outliers sampled first"),
    Transform("denorm-mix", _denorm_mix, None, "denormal and normal distances in one scene"),
)
NAMES = tuple(t.name for t in TRANSFORMS)
BASE = Transform("base", lambda xyz: (xyz.copy(), F(1.0)), None, "the metre-scale cloud itself: not a case, the other side of an exact scaling")
BY_NAME = {t.name: t for t in TRANSFORMS + (BASE,)}
EXACT = ("s-40", "s+10")    # neither underflow nor clamp: every op's indices equal the base cloud's, every distance is the base's times scale^2


@functools.lru_cache(maxsize=None)
def cloud(name, kind, n, seed=1):
    """-> (xyz (B, n, 3) float32 read-only, scale float32)"""
    xyz, scale = BY_NAME[name].fn(base_cloud(kind, n, seed))
    xyz = np.ascontiguousarray(xyz, F)
    assert xyz.dtype == F and xyz.shape == (B, n, 3)
    xyz.setflags(write=False)
    return xyz, F(scale)


def radii(name, kind, n, seed=1):
    """scale * {extent / 100, extent / 10, extent * 1.5} of the base cloud, every step in float32. Squared in float32 the first
    underflows to 0 (s-75, s-90), all are denormal (s-70, denorm-mix) or infinite (s+60, where only a padding row lies beyond)"""
    e, scale = extent(kind, n, seed), cloud(name, kind, n, seed)[1]
    out = tuple(scale * (e * F(f)) for f in (0.01, 0.1, 1.5))
    assert all(r.dtype == F and np.isfinite(r) for r in out)
    return out


def centres(name, kind, n, m, seed=1, noisy=True):
    """(B, m, 3) float32: m rows of the transformed scene (seeded), the second half of them moved by noise of a tenth of the
    scene's own extent per axis (an axis without extent stays), clipped into D"""
    xyz, _ = cloud(name, kind, n, seed)
    rng = np.random.default_rng([seed, n, m, 7])
    rows = rng.integers(0, n, size=m) if m > n else rng.permutation(n)[:m]
    c = np.array(xyz[:, rows])
    if noisy:
        with np.errstate(over="ignore"):
            span = np.ptp(xyz.astype(np.float64), axis=1, keepdims=True)
        noise = rng.normal(0.0, 0.1, (B, m, 3)) * span
        noise[:, :m // 2] = 0.0
        c = np.clip(c.astype(np.float64) + noise, -float(LIMIT), float(LIMIT)).astype(F)
    return np.ascontiguousarray(c, F)


def known_set(unknown, m, seed=1):
    """a known set of m rows for three_nn: rows of the unknown set itself (seeded), the first four of them copied from the unknown
    set's first rows and duplicated behind (exact zero distances, and ties between equal known rows), as tests/test_gpu_sweep.py"""
    n = unknown.shape[1]
    rng = np.random.default_rng([seed, n, m, 11])
    rows = rng.integers(0, n, size=m) if m > n else rng.permutation(n)[:m]
    known = np.array(unknown[:, rows])
    if m >= 8:
        known[:, :4] = unknown[:, :4]
        known[:, 4:8] = known[:, :4]
    return np.ascontiguousarray(known, F)


# ---- the table's own claims ---------------------------------------------------------------------------------------------------------
def d2_matrix(a, b):
    """(len(a), len(b)) squared distances in float32, dx*dx + dy*dy + dz*dz left to right, every step rounded on its own"""
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    with np.errstate(under="ignore"):
        d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == F
    return d


def in_domain(xyz):
    return bool(np.isfinite(xyz).all() and (np.abs(xyz) <= LIMIT).all())


def no_clamp(kind="kitti", n=2048, seed=1):
    """-> (largest squared distance of the base cloud, k): k is the largest power-of-two exponent with d2 * 2^(2k) < 1e10"""
    xyz = base_cloud(kind, n, seed)
    top = max(float(d2_matrix(s, s).max()) for s in xyz)
    k = 0
    while top * 4.0 ** (k + 1) < float(START):
        k += 1
    return top, k

"""The oracle itself across the float32 range of coordinates (tests/value_domain.py), before any kernel is judged against it: its
sequential scans against the closed forms of tests/test_oracle_second_derivation.py -- whole-array numpy float32 in the oracle's
expression order, dx*dx + dy*dy + dz*dz; the oracle is built with -ffp-contract=off -fno-fast-math, so denormals round as IEEE
says on both sides -- and the claims the case table makes about its own entries."""
import numpy as np
import pytest

import value_domain as vd
from test_oracle_second_derivation import ball_query_closed_form, fps_rank_rule, three_nn_closed_form

PAIRS = [(name, kind) for name in vd.NAMES for kind in vd.BASES]


def test_the_table_names_every_regime_once():
    assert len(set(vd.NAMES)) == len(vd.NAMES) == 16
    assert set(vd.EXACT) <= {t.name for t in vd.TRANSFORMS if t.fps == "equal"}
    for want in ("s-90", "s-75", "s-70", "s-40", "s+14", "s+20", "s+60", "t+17", "t+20", "t+23", "t+24", "t-24", "aniso", "outliers", "denorm-mix"):
        assert want in vd.NAMES


@pytest.mark.parametrize("name,kind", PAIRS)
def test_every_input_lies_in_the_domain(oracle, name, kind):
    """finite, |coordinate| <= 2^62, and every distance the oracle forms is finite: the whole matrix of a scene, and the running
    distances the oracle's own sampling leaves"""
    for n in (37, 1000):
        xyz, scale = vd.cloud(name, kind, n)
        assert vd.in_domain(xyz) and np.isfinite(scale) and scale > 0
        assert vd.in_domain(vd.centres(name, kind, n, 48))
        for s in xyz:
            assert np.isfinite(vd.d2_matrix(s, s)).all()
        _, temp = oracle.furthest_point_sampling(xyz, min(n, 48), return_temp=True)
        assert np.isfinite(temp).all() and (temp >= 0).all()
        assert all(np.isfinite(r) and r >= 0 for r in vd.radii(name, kind, n))


def test_the_top_of_the_domain_is_reached():
    xyz, _ = vd.cloud("s+60", "kitti", 1000)
    assert np.abs(xyz).max() == vd.LIMIT
    assert max(float(vd.d2_matrix(s, s).max()) for s in xyz) > 2.0 ** 124


def test_s10_is_the_largest_scaling_without_a_clamp():
    """what the table says of s+10 (and what it corrects about s+14): 2^10 keeps every squared distance of the kitti cloud below
    the 1e10 start value, 2^11 does not"""
    top, k = vd.no_clamp("kitti", 2048)
    assert k == 10, (top, k)
    for n in (1000, 4096):
        xyz, _ = vd.cloud("s+10", "kitti", n)
        assert max(float(vd.d2_matrix(s, s).max()) for s in xyz) < float(vd.START)
    xyz, _ = vd.cloud("s+14", "kitti", 1000)
    assert max(float(vd.d2_matrix(s, s).max()) for s in xyz) > float(vd.START)


def test_the_regimes_are_what_the_table_says(oracle):
    """the distances of each scaled kitti cloud, from the first sample: all zero (s-90), all denormal (s-75, s-70), all beyond 1e10
    except the twins' zeros (s+20); a mix of denormal and normal (denorm-mix); the shifted clouds lose rows to quantisation"""
    tiny = float(np.finfo(np.float32).tiny)

    def from_first(name):
        xyz, _ = vd.cloud(name, "kitti", 2048)
        return vd.d2_matrix(xyz[0][:1], xyz[0])[0]
    assert (from_first("s-90") == 0).all()
    for name in ("s-75", "s-70"):
        d = from_first(name)
        assert (d < tiny).all() and (d > 0).sum() > 2000
    d = from_first("s+20")
    assert ((d > float(vd.START)) | (d == 0)).all()
    d = from_first("denorm-mix")
    assert ((d > 0) & (d < tiny)).sum() > 500 and (d >= tiny).sum() > 500
    r = vd.radii("s-75", "kitti", 2048)
    assert r[0] * r[0] == 0 and 0 < r[1] * r[1] < tiny
    assert all(v * v == 0 for v in vd.radii("s-90", "kitti", 2048))
    with np.errstate(over="ignore"):
        assert np.isinf(vd.radii("s+60", "kitti", 2048)[2] * vd.radii("s+60", "kitti", 2048)[2])
    base = len(np.unique(vd.base_cloud("kitti", 2048)[0], axis=0))
    distinct = [len(np.unique(vd.cloud(name, "kitti", 2048)[0][0], axis=0)) for name in ("t+17", "t+20", "t+23", "t+24")]
    assert base >= distinct[0] >= distinct[1] > distinct[2] > distinct[3] > 100, (base, distinct)


@pytest.mark.parametrize("t", [t for t in vd.TRANSFORMS if t.fps], ids=lambda t: t.name)
def test_recorded_sampling_facts_hold(oracle, t):
    """"equal": the oracle samples the transformed kitti cloud as it samples the base cloud; "differs": it does not -- so a table
    whose transform did nothing cannot pass for one that did. EXACT entries: every base cloud, and the running distances are the
    base cloud's times scale^2 bit for bit"""
    n, m = 2048, 64
    base, base_temp = oracle.furthest_point_sampling(vd.base_cloud("kitti", n), m, return_temp=True)
    xyz, scale = vd.cloud(t.name, "kitti", n)
    got = oracle.furthest_point_sampling(xyz, m)
    assert np.array_equal(got, base) == (t.fps == "equal")
    if t.name in vd.EXACT:
        for kind in vd.BASES:
            for n in (1000, 4096):
                want, want_temp = oracle.furthest_point_sampling(vd.base_cloud(kind, n), 48, return_temp=True)
                got, got_temp = oracle.furthest_point_sampling(vd.cloud(t.name, kind, n)[0], 48, return_temp=True)
                np.testing.assert_array_equal(got, want)
                np.testing.assert_array_equal(got_temp, want_temp * (scale * scale))


@pytest.mark.parametrize("name,kind", PAIRS)
def test_sampling_oracle_equals_the_rank_rule(oracle, name, kind):
    for n in (37, 64, 1000, 4096):
        xyz, _ = vd.cloud(name, kind, n)
        m = min(n, 48)
        got, got_temp = oracle.furthest_point_sampling(xyz, m, return_temp=True)
        for s in range(vd.B):
            with np.errstate(under="ignore"):
                want, want_temp = fps_rank_rule(xyz[s], m, oracle.opt_n_threads(n))
            np.testing.assert_array_equal(got[s], want, err_msg="n = %d, scene %d" % (n, s))
            np.testing.assert_array_equal(got_temp[s], want_temp, err_msg="n = %d, scene %d" % (n, s))


@pytest.mark.parametrize("name,kind", PAIRS)
def test_ball_query_oracle_equals_the_closed_form(oracle, name, kind):
    n, m = 1000, 64
    xyz, _ = vd.cloud(name, kind, n)
    c = vd.centres(name, kind, n, m)
    for radius in vd.radii(name, kind, n):
        for ns in (1, 16):
            got = oracle.ball_query(float(radius), ns, xyz, c)
            assert ((got >= 0) & (got < n)).all()
            with np.errstate(under="ignore", over="ignore"):
                want = ball_query_closed_form(float(radius), ns, xyz, c)
            np.testing.assert_array_equal(got, want, err_msg="radius %r, nsample %d" % (radius, ns))


@pytest.mark.parametrize("name,kind", PAIRS)
def test_three_nn_oracle_equals_the_closed_form(oracle, name, kind):
    xyz, _ = vd.cloud(name, kind, 700)
    for m in (3, 300):
        known = vd.known_set(xyz, m)
        d2, idx = oracle.three_nn(xyz, known)
        with np.errstate(under="ignore"):
            want_d, want_i = three_nn_closed_form(xyz, known)
        np.testing.assert_array_equal(idx, want_i, err_msg="m = %d" % m)
        np.testing.assert_array_equal(d2, want_d, err_msg="m = %d" % m)
        assert np.isfinite(d2).all()

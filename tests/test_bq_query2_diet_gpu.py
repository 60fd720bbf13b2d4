"""The two-centre, shared-list ball query (bq_query2_kernel<D, 2, false, true>) at the pyramid's shapes, against the CPU oracle.

tests/test_ball_query_lists.py holds the list lengths at every bound, on clouds of 1024, 4096 and 8192 points. What it does not
reach: the one-level box pass at 2048 points, the two-level pass at 16384 (eight bitmap words per lane), and the pyramid's own
radius pairs on scene-like clouds, where the bucket-box pass sees lists of near quads of every length -- also none for one centre
of a wave and several for the other, the case in which a lane past its centre's list reads a slot of a list that was never
written in this round.

The built scene puts into one wave a centre that sees nothing and one with a long list, then a centre with more hits than the
larger nsample inside one grid cell (its first bucket), one above the 64-entry list (the bitmap walk) and one with three hits.
Indices are compared bit for bit.
"""
import numpy as np
import pytest
import torch

from epnet_amd import _lib, pointnet2_cuda as ext

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 2
PAIRS = {"0.1+0.5": (0.1, 0.5), "0.5+1": (0.5, 1.0), "1+2": (1.0, 2.0), "2+4": (2.0, 4.0)}   # the workload's four levels
NS = (16, 32)


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded(hiplib):
    assert torch.cuda.is_available()
    return hiplib


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def query(xyz, centres, radii):
    n, m = xyz.shape[1], centres.shape[1]
    d_xyz, d_c = dev(xyz), dev(centres)
    index = ext.scene_index(d_xyz)
    assert index is not None
    outs = [torch.full((B, m, ns), -1, dtype=torch.int32, device=DEV) for ns in NS]
    with _lib.tuning(EPNET_BQ_PAIR=1):   # two centres per wave, whatever the batch
        ext.ball_query_multi_wrapper(B, n, m, list(radii), list(NS), d_c, d_xyz, index, outs)
    return [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("kind", ["kitti", "ubox"])
@pytest.mark.parametrize("n,m", [(2048, 512), (4096, 1024), (16384, 4096)])
def test_pyramid_shapes_match_oracle(oracle, n, m, kind, pair):
    from epnet_amd import synth
    xyz = synth.scenes(kind, B, n, seed=n + 3).numpy()
    centres = np.ascontiguousarray(xyz[:, ::n // m][:, :m])
    radii = PAIRS[pair]
    for r, ns, got in zip(radii, NS, query(xyz, centres, radii)):
        np.testing.assert_array_equal(got, oracle.ball_query(r, ns, xyz, centres), err_msg="%s n=%d r=%g" % (kind, n, r))


def test_built_scene_of_uneven_lists(oracle):
    n, m = 16384, 64
    rng = np.random.default_rng(11)
    xyz = (rng.random((B, n, 3)).astype(np.float32) * np.float32(80.0)).astype(np.float32)   # sparse: about 0.03 points per unit cube
    centres = (rng.random((B, m, 3)).astype(np.float32) * np.float32(80.0)).astype(np.float32)
    r_in, r_out = 0.5, 1.0
    for s in range(B):
        spots = {1: 30, 2: 40, 4: 80, 5: 3, 7: 33, 6: 1}   # centre -> points planted inside the larger ball
        at = 100 + 1000 * s
        for c, k in spots.items():
            centres[s, c] = np.float32(5.0 + 9.0 * c)
            off = rng.normal(size=(k, 3)).astype(np.float32)
            off *= (rng.random((k, 1)).astype(np.float32) * np.float32(0.9)) / np.linalg.norm(off, axis=1, keepdims=True).astype(np.float32)
            # spread over the cloud's own order, so that index order and spatial order differ
            where = at + np.arange(k) * 37
            xyz[s, where] = centres[s, c] + off
            at += 50
        centres[s, 0] = np.float32(1000.0)   # sees nothing; shares its wave with centre 1
        centres[s, 3] = np.float32(-500.0)
    want_in, want_out = oracle.ball_query(r_in, NS[0], xyz, centres), oracle.ball_query(r_out, NS[1], xyz, centres)
    assert not want_out[:, 0].any() and not want_out[:, 3].any()                       # the empty lists
    assert all(len(set(want_out[s, 2].tolist())) == 32 and len(set(want_out[s, 1].tolist())) == 30 for s in range(B))
    got_in, got_out = query(xyz, centres, (r_in, r_out))
    np.testing.assert_array_equal(got_out, want_out)
    np.testing.assert_array_equal(got_in, want_in)

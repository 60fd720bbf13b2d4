"""One run of every branch of the sampling dispatch (epnet_amd/csrc/fps_plan.h carried out by fps_run in fps.hip): each kernel family
and each thing that follows it, at the smallest cloud that reaches it, against the CPU oracle -- idx and new_xyz bit for bit.

    n = 63      the stream kernel (reference block below one wave; running distances in memory)
    n = 64      one wave
    n = 1024    the wave kernel at its widest
    n = 1025    the pruned kernel; over a scene index the indexed kernel at np = 2048
    n = 8193    eight waves; with m = 1024 through sample_centres_index_wrapper the index epilogue, and with a prefix_in the two launches
    n = 16385   the bigscene kernel over index + temp; the stream kernel without an index

Two scenes per case. Scene 0 is reordered so that its first m points are its own furthest-point sequence: the chained cases hand
that knowledge in (prefix_in = [m, 0]), so that one scene takes the identity and the other runs its rounds; the other cases run the
rounds on both. Which kernel a shape gets is test_fps_plan.py's subject, on the CPU; the families named below are what it pins.
Every output sits between canaries. The next level's index is compared through the ball queries that read it (inside a grid cell
the order of its rows is not repeatable)."""
import functools

import numpy as np
import pytest
import torch

import offset_alloc as oa
from epnet_amd import pointnet2_cuda as ext

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 2


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded(hiplib):
    assert torch.cuda.is_available()
    return hiplib


_REF = {}


def reference(oracle, n, m):
    """the two scenes of a shape, the oracle's samples and their centres: computed once, shared, read-only"""
    if (n, m) not in _REF:
        from epnet_amd import synth
        c = np.stack([synth.cloud("kitti", n, 310 + k).numpy() for k in range(B)]).astype(np.float32)
        first = oracle.furthest_point_sampling(c[:1], min(m, n))[0].astype(np.int64)
        rest = np.setdiff1d(np.arange(n), first)
        c[0] = c[0][np.concatenate([first, rest])]
        idx = oracle.furthest_point_sampling(c, m)
        assert np.array_equal(idx[0, :min(m, n)], np.arange(min(m, n))), "scene 0 starts with its own furthest-point sequence"
        centres = np.take_along_axis(c, idx[:, :, None].astype(np.int64), axis=1)
        for a in (c, idx, centres):
            a.setflags(write=False)
        _REF[(n, m)] = (c, idx, centres)
    return _REF[(n, m)]


def run(oracle, route, n, m, indexed, chained, reports_ties=False):
    c, want_idx, want_c = reference(oracle, n, m)
    cloud = torch.from_numpy(np.array(c)).to(DEV)
    index = ext.scene_index(cloud) if indexed else None
    idx = oa.output((B, m), torch.int32, 0)
    prefix_in = torch.tensor([m, 0], dtype=torch.int32, device=DEV) if chained else None
    prefix_out = oa.output((B,), torch.int32, 0) if chained or route == "index" else None
    new_xyz = nxt = None
    if route == "fps":
        temp = torch.full((B, n), 1e10, device=DEV)
        if indexed:
            ext.furthest_point_sampling_indexed_wrapper(B, n, m, cloud, index, temp, idx)
        else:
            ext.furthest_point_sampling_wrapper(B, n, m, cloud, temp, idx)
    else:
        new_xyz = oa.output((B, m, 3), torch.float32, 0)
        if route == "centres":
            ext.sample_centres_wrapper(B, n, m, cloud, index, idx, new_xyz, prefix_in, prefix_out)
        else:
            nxt = torch.zeros((ext.scene_index_bytes(B, m),), dtype=torch.uint8, device=DEV)
            ext.sample_centres_index_wrapper(B, n, m, cloud, index, idx, new_xyz, nxt, prefix_in, prefix_out)
    oa.check()
    assert oa.unwritten(idx) == 0
    np.testing.assert_array_equal(idx.cpu().numpy(), want_idx)
    if new_xyz is not None:
        assert oa.unwritten(new_xyz) == 0
        np.testing.assert_array_equal(new_xyz.cpu().numpy().view(np.int32), want_c.view(np.int32))
    if prefix_out is not None:
        # a scene that took the identity passes its knowledge on; one that ran its rounds reports how many of them went without a
        # tie where the kernel can tell (the pruned families), else 0. What a count v claims: the first v centres are their own
        # furthest-point sequence
        got = prefix_out.cpu().tolist()
        for s in range(B):
            if chained and s == 0:
                assert got[s] == m
            elif not reports_ties:
                assert got[s] == 0
            else:
                assert 1 <= got[s] <= m, got
                np.testing.assert_array_equal(oracle.furthest_point_sampling(np.asarray(want_c[s:s + 1]), got[s])[0], np.arange(got[s]))
    if nxt is not None:   # the next level's index, through its readers
        m2 = 64
        centres2 = new_xyz[:, :m2].contiguous()
        outs = [torch.full((B, m2, ns), -1, dtype=torch.int32, device=DEV) for ns in (16, 32)]
        ext.ball_query_multi_wrapper(B, m, m2, [1.0, 2.0], [16, 32], centres2, new_xyz.contiguous(), nxt, outs)
        for r, ns, got in zip((1.0, 2.0), (16, 32), outs):
            np.testing.assert_array_equal(got.cpu().numpy(), oracle.ball_query(r, ns, np.asarray(want_c), np.asarray(want_c[:, :m2])),
                                          err_msg="ball query r=%g from the next index" % r)


#        route      n      m     index  chain  ties     what runs
CASES = [
    ("fps",     63,    8,    False, False, False),   # stream
    ("centres", 63,    8,    False, False, False),   # stream, gather
    ("centres", 63,    8,    False, True,  False),   # prefix kernel, stream, gather
    ("centres", 64,    8,    False, False, False),   # wave<1,1>, which writes the centres
    ("centres", 64,    8,    False, True,  False),   # wave with the prologue
    ("centres", 1024,  8,    True,  False, False),   # wave<8,2> (an index is not used at 1024 points)
    ("centres", 1025,  8,    False, False, True),    # pruned<4,8>, gather
    ("centres", 1025,  8,    False, True,  True),    # prefix kernel, pruned, gather
    ("centres", 1025,  8,    True,  False, True),    # indexed<4,8>, gather
    ("centres", 1025,  8,    True,  True,  True),    # indexed with the prologue, gather
    ("centres", 8193,  8,    False, False, True),    # pruned<8,32>
    ("centres", 8193,  8,    True,  False, True),    # indexed<8,32>
    ("index",   8193,  1024, True,  False, True),    # indexed<8,32> with the index epilogue
    ("index",   8193,  1024, True,  True,  True),    # a prefix_in: the gathered index build as a launch of its own
    ("fps",     16385, 8,    True,  False, False),   # bigscene
    ("centres", 16385, 8,    True,  True,  False),   # prefix kernel, bigscene, gather
    ("centres", 16385, 8,    False, False, False),   # stream, gather
]


@pytest.mark.parametrize("route,n,m,indexed,chained,reports_ties", CASES)
def test_every_branch_of_the_dispatch(oracle, route, n, m, indexed, chained, reports_ties):
    run(oracle, route, n, m, indexed, chained, reports_ties)

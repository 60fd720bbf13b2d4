"""The pipelined stack as the 256-scene benchmark line runs it since level 2's ball queries went back to stage G: the queries of
levels 3 and 4 at the tail of stage S, level 2's centres and index out of the level-1 sampling call. Every tensor of every level
against the oracle (bench.verify_scene), over two HIP graphs -- and the same with the centre gather inside the next level's
index-build dispatch (EPNET_SA_FUSE_GATHER=2), the sequence the step timings compare the sampling kernel's epilogue with."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded(hiplib):
    assert torch.cuda.is_available()
    return hiplib


@pytest.mark.parametrize("kind,fuse_gather", [("kitti", "1"), ("dup", "2")])
def test_levels_3_and_4_in_stage_s_against_the_oracle(oracle, monkeypatch, kind, fuse_gather):
    import bench
    from epnet_amd import sa_stack, synth
    monkeypatch.setenv("EPNET_SA_FUSE_GATHER", fuse_gather)
    b = 2
    xyz = synth.scenes(kind, b, 16384, seed=78).to(DEV)
    stack = sa_stack.SAStack(b, n=16384, device=DEV, seed=5, pipelined=True, fused_sampling=True, s_query_levels=(2, 3))
    assert stack.s_query_levels == frozenset({2, 3}) and stack.fuse_gather == int(fuse_gather)
    stack.capture(xyz)
    for L in stack.levels:        # nothing of the capture-time warm-up may survive into the comparison
        L["fps_idx"].fill_(-1)
        for P in L["sets"]:
            P["new_xyz"].zero_()
        for S in L["scales"]:
            for idx_set in S["idx_sets"]:
                idx_set.zero_()
            S["grouped"].fill_(float("nan"))
    for _ in range(3):            # both graphs of the rotation; the third replay regroups what the second one sampled
        stack.replay()
    torch.cuda.synchronize()
    for scene in range(b):
        assert bench.verify_scene(stack, stack.inputs[0], scene) == []


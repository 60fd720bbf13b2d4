"""bench.py's per-launch byte formulas add up to SURVEY.md section 8(d)'s per-scene figure (51 326 720 B for one
16384-point scene through the SA op stack), whichever way the stack issues its calls."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _calls(fused, multi):
    from epnet_amd import sa_stack
    calls = []
    n = 16384
    for lvl, m in enumerate(sa_stack.RPN_NPOINTS):
        c = sa_stack.RPN_FEAT_CHANNELS[lvl]
        calls.append(("furthest_point_sampling_indexed_wrapper", (1, n, m)))
        calls.append(("gather_points_wrapper", (1, 3, n, m)))
        radii, nss = sa_stack.RPN_RADII[lvl], sa_stack.RPN_NSAMPLES[lvl]
        if multi == "ordered":     # what the stack issues since round 3: the same bytes under the ordered entry point's name
            calls.append(("ball_query_ordered_wrapper", (1, n, m, list(radii), list(nss))))
        elif multi:
            calls.append(("ball_query_multi_wrapper", (1, n, m, list(radii), list(nss))))
        else:
            calls += [("ball_query_indexed_wrapper", (1, n, m, r, ns)) for r, ns in zip(radii, nss)]
        if fused == "multi":
            calls.append(("group_concat_multi_wrapper", (1, c, n, m, list(nss))))
            n = m
            continue
        for ns in nss:
            if fused:
                calls.append(("group_concat_wrapper", (1, c, n, m, ns)))
            else:
                calls.append(("group_points_wrapper", (1, 3, n, m, ns)))
                if c:
                    calls.append(("group_points_wrapper", (1, c, n, m, ns)))
        n = m
    return calls


def test_launch_bytes_sum_to_the_survey_figure():
    import bench
    from epnet_amd import sa_stack
    want = sa_stack.sa_algorithmic_bytes(16384)
    assert want["total"] == 51326720
    for fused in (False, True, "multi"):
        for multi in (False, True, "ordered"):
            total = sum(bench.op_family(name, head)[1] for name, head in _calls(fused, multi))
            assert total == want["total"], (fused, multi, total)


def test_scene_index_is_not_counted_as_algorithmic():
    import bench
    label, nbytes = bench.op_family("scene_index_build_wrapper", (1, 16384))
    assert label.startswith("scene_index") and nbytes > 0   # reported per launch, but not part of the stack total


def test_dominant_family_is_stable_when_sampling_and_grouping_trade_places():
    """roofline names the longest family of a step; within 10 % of the longest the one that moves the most bytes (the level-1
    sampling, a latency chain of 72 MB, and the grouping calls, 13 GB, are 2.09 - 2.22 ms each from run to run)"""
    import bench
    def fam(step_ms, launches, nbytes):
        return {"step_ms": step_ms, "launches_per_step": launches, "bytes_per_launch": nbytes, "avg_ms": step_ms / launches, "GBps": 0.0}
    k = {"fps N=16384 M=4096": fam(2.116, 1, 72_000_000), "group": fam(2.090, 4, 3_100_000_000), "ball_query x": fam(0.45, 1, 400_000_000)}
    assert bench.pick_dominant(k) == ("fps N=16384 M=4096", "group")
    k["group"] = fam(2.224, 4, 3_100_000_000)
    assert bench.pick_dominant(k) == ("group", "group")
    k["group"] = fam(1.2, 4, 3_100_000_000)                   # far behind: the longest family is named, whatever it moves
    assert bench.pick_dominant(k) == ("fps N=16384 M=4096", "fps N=16384 M=4096")


def test_dump_outputs_is_float32_bounded_and_repeatable(tmp_path):
    """--dump-outputs: every array as float32 .npy; the large ones replaced by the same seeded sample of their elements from run
    to run, the whole under the budget"""
    import numpy as np
    import torch
    import bench
    arrays = {"level1.centres": torch.arange(2 * 8 * 3, dtype=torch.float32).reshape(2, 8, 3),
              "level1.r0.1.ball_idx": torch.arange(4 * 1000 * 16, dtype=torch.int32).reshape(4, 1000, 16) % 16384,
              "level1.r0.1.grouped": torch.randn((4, 3, 1000, 16), generator=torch.Generator().manual_seed(0))}
    budget = 3 * 4 * 20000
    info = [bench.dump_outputs(arrays, str(tmp_path / d), budget=budget) for d in ("a", "b")]
    assert info[0] == info[1] and info[0]["level1.centres"]["sampled"] is None and info[0]["level1.r0.1.grouped"]["sampled"] == 20000
    total = 0
    for name, t in arrays.items():
        a, b = (np.load(str(tmp_path / d / (name + ".npy"))) for d in ("a", "b"))
        assert a.dtype == np.float32 and np.array_equal(a, b)
        total += a.nbytes
        if info[0][name]["sampled"] is None:
            assert np.array_equal(a, t.float().numpy())
        else:   # a sample of the array's own values, in the order of their positions
            assert a.size == info[0][name]["sampled"] and np.isin(a, t.float().numpy().ravel()).all()
    assert total <= budget

"""The deterministic gradients without a GPU: the C ABI declares, exports and binds every *_det entry point; the stand-in
wrappers pick them exactly when torch.use_deterministic_algorithms(True) is on; and the numpy restatements of the contract
orders (tests/det_restate.py), which the GPU tests hold the kernels to bit for bit, are themselves the oracle's loops and
grid_sample's gradient. The flag itself is only ever switched on in a child process (tests/det_dispatch_probe.py)."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import det_restate as R
from conftest import ROOT

DET_OPS = ["gather_points_grad", "group_points_grad", "group_concat_grad", "three_interpolate_grad", "feature_gather_grad",
           "group_linear_grad_w"]


# ---- the ABI ---------------------------------------------------------------------------------------------------------
def test_every_det_symbol_is_declared_exported_and_bound(hiplib):
    from epnet_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "epnet_ops.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for op in DET_OPS:
        for name in ("epnet_%s_det" % op, "epnet_%s_det_workspace_bytes" % op):
            assert re.search(r"\b%s\s*\(" % name, text), name
            assert hasattr(raw, name), name
            assert name in _lib.SIGNATURES, name
    assert hiplib.epnet_abi_version() == 1


def test_det_workspace_depends_on_shape_only(hiplib):
    l = hiplib
    q = {
        "gather_points_grad": lambda b: l.epnet_gather_points_grad_det_workspace_bytes(b, 4096, 1024),
        "group_points_grad": lambda b: l.epnet_group_points_grad_det_workspace_bytes(b, 65536, 16384, 64),
        "group_concat_grad": lambda b: l.epnet_group_concat_grad_det_workspace_bytes(b, 4096, 1024, 32),
        "three_interpolate_grad": lambda b: l.epnet_three_interpolate_grad_det_workspace_bytes(b, 16384, 4096),
        "feature_gather_grad": lambda b: l.epnet_feature_gather_grad_det_workspace_bytes(b, 48, 160, 4096),
        "group_linear_grad_w": lambda b: l.epnet_group_linear_grad_w_det_workspace_bytes(b, 64, 1024, 32),
    }
    for op, f in q.items():
        assert f(0) == 0, op
        assert 0 < f(1) < f(2) < f(16), op
        assert f(16) == f(16), op
    # empty problems need nothing, anything else something
    assert l.epnet_group_points_grad_det_workspace_bytes(4, 0, 16, 4) == 0
    assert l.epnet_group_points_grad_det_workspace_bytes(4, 16, 0, 4) == 0
    assert l.epnet_three_interpolate_grad_det_workspace_bytes(4, 0, 16) == 0
    assert l.epnet_feature_gather_grad_det_workspace_bytes(4, 0, 8, 16) == 0
    assert l.epnet_group_linear_grad_w_det_workspace_bytes(4, 0, 16, 4) == 0
    assert l.epnet_gather_points_grad_det_workspace_bytes(1, 1, 1) > 0
    # (no tuning value enters them)
    from epnet_amd import _lib
    before = q["group_points_grad"](3)
    with _lib.tuning(EPNET_BQ_PAIR=1, EPNET_NN_TILE_MIN_BUCKETS=0):
        assert q["group_points_grad"](3) == before


def test_det_entry_points_validate_without_a_gpu(hiplib):
    l = hiplib
    # empty problems are no-ops, null pointers and short workspaces are refused before any launch
    assert l.epnet_group_points_grad_det(0, 4, 16, 4, 4, None, None, None, None, 0, None) == 0
    assert l.epnet_group_points_grad_det(1, 4, 16, 4, 4, None, None, None, None, 0, None) == -1
    assert l.epnet_group_points_grad_det(1, 4, 16, 4, 4, 256, 256, 256, None, 0, None) == -3
    assert l.epnet_group_points_grad_det(-1, 4, 16, 4, 4, 256, 256, 256, 256, 1 << 20, None) == -1
    assert l.epnet_group_points_grad_det(65536, 1, 16, 1, 1, 256, 256, 256, 256, 1 << 40, None) == -4
    assert l.epnet_feature_gather_grad_det(1, 4, 8, 8, 16, 1, 256, 256, 256, None, 0, None) == -3
    assert l.epnet_group_linear_grad_w_det(1, 4, 16, 4, 4, 256, 256, 256, 256, 256, 256, 0, None) == -3


@pytest.mark.skipif(torch.cuda.is_available(), reason="hands the library placeholder pointers: only where no GPU could run them")
def test_every_det_limit_is_refused_before_a_launch(hiplib):
    """each EPNET_ELIMIT condition of each *_det entry point returns -4 with placeholder pointers and a workspace that passes every
    other check. Without a GPU a launch fails (-2, the first assertion), so -4 also shows that nothing was launched first"""
    l = hiplib
    P, WS = 256, 1 << 40                   # placeholder pointer (256-byte aligned), workspace size that is never short
    big_b, big_c = 65536, 8 * 65535 + 1    # b > 65535; ceil(c / 8) = 65536 fold rows / grad_w chunks
    calls = {
        "gather_points_grad": lambda b, c, n, m: l.epnet_gather_points_grad_det(b, c, n, m, P, P, P, P, WS, None),
        "group_points_grad": lambda b, c, n, m, ns=1: l.epnet_group_points_grad_det(b, c, n, m, ns, P, P, P, P, WS, None),
        "group_concat_grad": lambda b, c, n, m, ns=1: l.epnet_group_concat_grad_det(b, c, n, m, ns, P, P, P, 1, P, WS, None),
        "three_interpolate_grad": lambda b, c, n, m: l.epnet_three_interpolate_grad_det(b, c, n, m, P, P, P, P, P, WS, None),
        "feature_gather_grad": lambda b, c, h, w, n: l.epnet_feature_gather_grad_det(b, c, h, w, n, 1, P, P, P, P, WS, None),
        "group_linear_grad_w": lambda b, c, n, m, ns=1: l.epnet_group_linear_grad_w_det(b, c, n, m, ns, P, P, P, P, P, P, WS, None),
    }
    assert calls["group_points_grad"](1, 4, 16, 4, 4) == -2          # a shape inside the limits reaches its first launch
    refused = {
        "gather_points_grad": [(big_b, 1, 16, 4), (1, big_c, 16, 4)],
        "group_points_grad": [(big_b, 1, 16, 4), (1, big_c, 16, 4), (1, 1, 16, 65536, 32768)],
        "group_concat_grad": [(big_b, 1, 16, 4), (1, big_c, 16, 4), (1, 1, 16, 65536, 32768)],
        # 3 n entries: n = 715827883 -> 2^31 + 1
        "three_interpolate_grad": [(big_b, 1, 16, 4), (1, big_c, 16, 4), (1, 1, 715827883, 16)],
        # 4 n entries: n = 2^29 -> 2^31; h w = 65536 * 32768 = 2^31
        "feature_gather_grad": [(big_b, 1, 4, 4, 4), (1, big_c, 4, 4, 4), (1, 1, 4, 4, 1 << 29), (1, 1, 65536, 32768, 4)],
        "group_linear_grad_w": [(big_b, 1, 16, 4), (1, big_c, 16, 4), (1, 1, 16, 65536, 32768)],
    }
    assert set(refused) == set(DET_OPS)
    for op, shapes in refused.items():
        for shape in shapes:
            assert calls[op](*shape) == -4, (op, shape)
        # (the same calls one step inside the b and c limits get past the limit check)
        assert calls[op](*((65535,) + shapes[0][1:])) != -4, op
        assert calls[op](*((1, 8 * 65535) + shapes[1][2:])) != -4, op


# ---- the Python surface, against a recording stand-in for the library ----------------------------------------------------------
# torch.use_deterministic_algorithms is process-wide: the flag is switched on only in a child process (tests/det_dispatch_probe.py),
# so that nothing of it -- the flag, its NaN-filled allocations, the stand-in library -- reaches the other tests of this process.
@pytest.fixture(scope="module")
def dispatch():
    env = dict(os.environ)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "det_dispatch_probe.py")], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


TODAY = {
    "gather_points_grad": ["epnet_gather_points_grad"],
    "group_points_grad": ["epnet_group_points_grad_workspace_bytes", "epnet_group_points_grad_ws"],
    "group_concat_grad": ["epnet_group_points_grad_workspace_bytes", "epnet_group_concat_grad_ws"],
    "three_interpolate_grad": ["epnet_three_interpolate_grad_workspace_bytes", "epnet_three_interpolate_grad_ws"],
    "group_linear_grad_w": ["epnet_group_linear_grad_w"],
    "feature_gather_grad": ["epnet_feature_gather", "epnet_feature_gather_grad"],
}


@pytest.mark.parametrize("op", DET_OPS)
def test_wrappers_follow_torchs_deterministic_flag(op, dispatch):
    assert dispatch["initial_flag"] is False
    assert dispatch["off"][op] == TODAY[op]
    want = ["epnet_%s_det_workspace_bytes" % op, "epnet_%s_det" % op]
    if op == "feature_gather_grad":
        want = ["epnet_feature_gather"] + want
    assert dispatch["on"][op] == want


def test_a_refused_shape_raises_naming_the_op(dispatch):
    refused = dispatch["refused"]
    assert refused["raised"] is not None and "group_points_grad" in refused["raised"]
    assert "epnet_group_points_grad_det" in refused["calls"]
    assert not any(c.endswith("_ws") or c == "epnet_group_points_grad" for c in refused["calls"])


def test_this_process_never_had_the_flag_on():
    assert not torch.are_deterministic_algorithms_enabled()


# ---- the restatements -------------------------------------------------------------------------------------------------
def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("seed", [0, 1])
def test_scatter_restatements_are_the_oracle_loops(seed, oracle):
    r = np.random.default_rng(seed)
    b, c, n, m, ns = 3, 5, 97, 40, 8
    # skew: padding repeats and a hot target
    idx = r.integers(0, n, size=(b, m, ns)).astype(np.int32)
    idx[:, :, ns // 2:] = idx[:, :, :1]
    idx[:, ::3, 1] = 7
    go = r.standard_normal((b, c, m, ns), dtype=np.float32)
    start = r.standard_normal((b, c, n), dtype=np.float32)
    want = start.copy()
    oracle.lib().oracle_group_points_grad(b, c, n, m, ns, _p(go), _p(idx), _p(want))
    same_bits(R.group_points_grad(start, go, idx), want)

    gidx = np.ascontiguousarray(idx[:, :, 0])
    go2 = r.standard_normal((b, c, m), dtype=np.float32)
    want = start.copy()
    oracle.lib().oracle_gather_points_grad(b, c, n, m, _p(go2), _p(gidx), _p(want))
    same_bits(R.gather_points_grad(start, go2, gidx), want)

    nu = 300
    iidx = r.integers(0, m, size=(b, nu, 3)).astype(np.int32)
    iidx[:, ::2, 0] = 3
    w = r.random((b, nu, 3), dtype=np.float32)
    go3 = r.standard_normal((b, c, nu), dtype=np.float32)
    start3 = r.standard_normal((b, c, m), dtype=np.float32)
    want = start3.copy()
    oracle.lib().oracle_three_interpolate_grad(b, c, nu, m, _p(go3), _p(iidx), _p(w), _p(want))
    same_bits(R.three_interpolate_grad(start3, go3, iidx, w), want)


@pytest.mark.parametrize("align_corners", [True, False])
def test_taps_restatement_is_grid_samples_gradient(align_corners):
    import torch.nn.functional as F
    r = np.random.default_rng(3)
    b, c, h, w, n = 2, 4, 40, 64, 300     # (few points per pixel: the sums are short, so torch's own order hardly matters)
    xy = r.uniform(-1.2, 1.2, size=(b, n, 2)).astype(np.float32)
    go = r.standard_normal((b, c, n), dtype=np.float32)
    fmap = torch.zeros((b, c, h, w), dtype=torch.float32, requires_grad=True)
    out = F.grid_sample(fmap, torch.from_numpy(xy)[:, None], mode="bilinear", padding_mode="zeros", align_corners=align_corners)
    out.backward(torch.from_numpy(go)[:, :, None, :])
    got = R.feature_gather_grad(np.zeros((b, c, h, w), np.float32), go, xy, align_corners)
    # align_corners=False: torch's CPU kernel arrives at the unnormalised coordinate by other roundings than
    # ((x + 1) * W - 1) / 2, which moves a tap weight by a few ulps of the coordinate: 1e-5 relative there
    assert np.allclose(got, fmap.grad.numpy(), rtol=0 if align_corners else 1e-5, atol=1e-6)


def test_group_linear_order_restatement_is_the_sum():
    r = np.random.default_rng(4)
    b, c, n, m, ns = 2, 5, 300, 700, 7      # p = 4900: two tiles, the second one partial
    xyz = r.standard_normal((b, n, 3), dtype=np.float32)
    new_xyz = np.ascontiguousarray(np.resize(xyz[:, :50], (b, m, 3)), np.float32)
    idx = r.integers(0, n, size=(b, m, ns)).astype(np.int32)
    go = r.standard_normal((b, c, m, ns), dtype=np.float32)
    start = r.standard_normal((c, 3), dtype=np.float32)
    got = R.group_linear_grad_w(start, go, xyz, new_xyz, idx)
    d = xyz[np.arange(b)[:, None], idx.reshape(b, -1)].astype(np.float64) - np.repeat(new_xyz, ns, axis=1)
    exact = start + np.einsum("bcp,bpk->ck", go.reshape(b, c, -1).astype(np.float64), d)
    assert np.allclose(got, exact, rtol=1e-5, atol=1e-4)
    same_bits(got, R.group_linear_grad_w(start, go, xyz, new_xyz, idx))


# ---- the GPU sweep's generator (tests/test_deterministic_sweep.py) ---------------------------------------------------------------
def test_det_sweep_keeps_every_boundary():
    """for every op, the seeded case list has a case on either side of each radix pass-count boundary and of the 4096-entry sort
    tile, so that an edit of the generator cannot drop that coverage unnoticed"""
    import test_deterministic_sweep as S
    assert set(S.OPS) == set(DET_OPS)
    assert [S.passes_of(n) for n in (1, 2, 256, 257, 65536, 65537, 1 << 24, (1 << 24) + 1)] == [0, 1, 1, 2, 2, 3, 3, 4]
    assert [cs["i"] for cs in S.CASES] == list(range(len(S.CASES)))
    for op in DET_OPS:
        cases = [cs for cs in S.CASES if cs["op"] == op]
        ns = {cs["n"] for cs in cases}
        for lo, hi in S.PASS_BOUNDARIES:
            assert lo in ns and hi in ns, (op, lo, hi)
        assert {S.passes_of(n) for n in ns} >= {0, 1, 2, 3, 4}, op
        assert any(S.TILE - 4 <= cs["p"] <= S.TILE for cs in cases), op             # one full tile (3 n, 4 n: the nearest count)
        assert any(S.TILE < cs["p"] <= S.TILE + 4 for cs in cases), op              # ... and one entry past it
        assert any(cs["p"] >= 10 ** 6 for cs in cases) or op == "group_linear_grad_w", op
        assert {1, 7, 8, 9, 17} <= {cs["c"] for cs in cases} and max(cs["c"] for cs in cases) >= 256, op
        assert {1, 2, 3, 17} <= {cs["b"] for cs in cases} and {255, 256, 257} <= {cs["b"] for cs in cases}, op
        fams = {cs["family"] for cs in cases}
        assert fams >= set(S.FAMILIES) - ({"out_of_range"} if op == "group_linear_grad_w" else set()), (op, fams)
        for cs in cases:
            assert cs["p"] == cs["npts"] * {"three_interpolate_grad": 3, "feature_gather_grad": 4}.get(op, cs["ns"]), cs
        if op in ("group_concat_grad", "feature_gather_grad"):
            assert {cs["flag"] for cs in cases} == {True, False}, op

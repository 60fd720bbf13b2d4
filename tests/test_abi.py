"""The C-ABI library: loads without a GPU, exports every symbol include/epnet_ops.h declares, and the
Python binding table mirrors the header. No compute calls here (there is no GPU on the CPU runner)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


def header_functions():
    text = open(os.path.join(ROOT, "include", "epnet_ops.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(epnet_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_hot_path():
    names = header_functions()
    for must in ["epnet_furthest_point_sampling", "epnet_gather_points", "epnet_gather_points_grad", "epnet_ball_query",
                 "epnet_group_points", "epnet_group_points_grad", "epnet_three_nn", "epnet_three_interpolate",
                 "epnet_three_interpolate_grad", "epnet_boxes_overlap_bev", "epnet_boxes_iou_bev", "epnet_nms",
                 "epnet_nms_normal", "epnet_roipool3d", "epnet_pts_in_boxes3d_host", "epnet_roipool3d_host"]:
        assert must in names


def test_library_exports_every_declared_symbol(hiplib):
    from epnet_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in header_functions():
        assert hasattr(raw, name), "libepnet_hip.so lacks %s" % name
    assert sorted(_lib.SIGNATURES) == header_functions()
    assert hiplib.epnet_abi_version() == 1
    assert hiplib.epnet_strerror(0) == b"ok" and b"workspace" in hiplib.epnet_strerror(-3)


def test_argument_validation_without_gpu(hiplib):
    # negative sizes / NULL pointers are rejected before anything touches the device
    assert hiplib.epnet_ball_query(-1, 1, 1, 1.0, 1, None, None, None, None) == -1
    assert hiplib.epnet_furthest_point_sampling(1, 16, 4, None, None, None, None) == -1
    assert hiplib.epnet_group_points(1, 1, 1, 1, 1, None, None, None, None) == -1
    assert hiplib.epnet_nms_workspace_bytes(6300) == 6300 * 99 * 8 + 6300 * 80   # mask words + one 80-byte record per box
    assert hiplib.epnet_nms_workspace_bytes(0) == 0
    # positions to fill from an EMPTY cloud (n = 0): an error code, not a division by zero on the host
    import ctypes as C
    fake = C.c_void_p(4096)   # never dereferenced: the call must return before anything touches the device
    assert hiplib.epnet_group_points(1, 16, 0, 512, 8, fake, fake, fake, None) == -1
    assert hiplib.epnet_gather_points(1, 16, 0, 4096, fake, fake, fake, None) == -1
    assert hiplib.epnet_group_concat(1, 16, 0, 512, 8, fake, fake, fake, fake, fake, 1, None) == -1
    two = (C.c_int * 2)(8, 8)
    ptrs = (C.c_void_p * 2)(4096, 4096)
    assert hiplib.epnet_group_concat_multi(1, 16, 0, 512, 2, C.cast(two, C.c_void_p), fake, fake, fake, C.cast(ptrs, C.c_void_p),
                                           C.cast(ptrs, C.c_void_p), 1, None) == -1
    # empty problems are no-ops
    assert hiplib.epnet_ball_query(0, 10, 10, 1.0, 4, None, None, None, None) == 0
    assert hiplib.epnet_three_nn(1, 0, 5, None, None, None, None, None) == 0


# Workspace sizes of the box features, recorded from the library BEFORE their plans were rewritten on the shared carver
# (common.h): callers size and slice their buffers by these numbers, so a refactor must return every one of them unchanged.
# The models' own shapes (B = 2 / 16, M = 512, G = 20, R = 64 / 128, pre / post 9000 / 512), odd sizes, and the limits
# beyond which an entry point answers 0.
WORKSPACE_BYTES = {
    "epnet_rcnn_sample_rois_workspace_bytes": [
        ((2, 512, 20, 64), 91152), ((16, 512, 20, 128), 737344), ((1, 1, 1, 1), 96), ((3, 300, 7, 64), 33952),
        ((2, 4096, 33, 1024), 1163280), ((0, 512, 20, 64), 0), ((65536, 512, 20, 64), 0), ((2, 4097, 20, 64), 0),
        ((2, 512, 0, 64), 0), ((2, 512, 20, 1025), 0),
    ],
    "epnet_rpn_proposals_workspace_bytes": [
        ((2, 1, 9000, 512), 22824032), ((16, 1, 9000, 512), 182592256), ((2, 0, 9000, 512), 44640032),
        ((16, 0, 9000, 512), 357120256), ((1, 1, 9000, 100), 11412032), ((1, 0, 9000, 100), 22320032), ((3, 1, 37, 5), 18368),
        ((1, 1, 0, 0), 272), ((1, 0, 0, 0), 272), ((0, 1, 9000, 512), 0), ((2, 1, -1, 512), 0),
    ],
    "epnet_rpn_handover_workspace_bytes": [
        ((2, 16384, 1, 9000, 512), 24003680), ((16, 16384, 1, 9000, 512), 192029440), ((2, 16384, 0, 9000, 512), 45819680),
        ((1, 4099, 1, 9000, 100), 11559616), ((3, 333, 0, 37, 5), 62704), ((1, 1, 1, 0, 0), 320), ((0, 16384, 1, 9000, 512), 0),
        ((32768, 16, 1, 10, 10), 0), ((2, 16385, 1, 9000, 512), 0), ((2, 0, 1, 9000, 512), 0),
    ],
    "epnet_rcnn_detections_workspace_bytes": [
        ((2, 512), 180256), ((16, 512), 1441920), ((1, 100), 12832), ((1, 1), 192), ((3, 65), 25008), ((2, 4096), 5111840),
        ((0, 512), 0), ((2, 4097), 0), ((65536, 4), 0), ((2, 0), 0),
    ],
    "epnet_eval_recall_workspace_bytes": [
        ((2, 512, 20), 88384), ((16, 512, 20), 664064), ((1, 100, 0), 6144), ((1, 1, 1), 6176), ((3, 65, 7), 11792),
        ((2, 4096, 33), 1088016), ((0, 512, 20), 0), ((2, 4097, 20), 0), ((65536, 4, 4), 0), ((2, 512, -1), 0),
    ],
    "epnet_kitti_pr_workspace_bytes": [
        ((3769, 6, 41), 18543488), ((50, 3, 41), 123008), ((1, 1, 1), 32), ((7, 16, 64), 143360), ((5, 3, 3), 912),
        ((0, 3, 41), 0), ((3, 17, 41), 0), ((3, 3, 65), 0), ((3, 0, 41), 0),
    ],
    "epnet_nms_workspace_bytes": [
        ((6300,), 5493600), ((9000,), 10872000), ((512,), 73728), ((1,), 88), ((64,), 5632), ((65,), 6240), ((0,), 0), ((-5,), 0),
    ],
}


@pytest.mark.parametrize("name", sorted(WORKSPACE_BYTES))
def test_box_feature_workspace_sizes_are_pinned(hiplib, name):
    for args, expect in WORKSPACE_BYTES[name]:
        assert getattr(hiplib, name)(*args) == expect, (name, args)


def test_missing_library_is_loud(monkeypatch, tmp_path):
    from epnet_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.lib()


def test_cpu_tensors_are_rejected(hiplib):
    import torch
    from epnet_amd import pointnet2_utils, iou3d_utils
    xyz = torch.zeros((1, 8, 3))
    with pytest.raises(RuntimeError, match="CUDAtensor"):
        pointnet2_utils.ball_query(1.0, 4, xyz, xyz)
    with pytest.raises(RuntimeError, match="CUDAtensor"):
        iou3d_utils.boxes_iou_bev(torch.zeros((2, 5)), torch.zeros((2, 5)))


def test_host_ops_match_oracle_and_fixture(hiplib, oracle):
    """roipool3d's CPU entry points are host ops in the reference too (roipool3d.cpp:97-195)"""
    import numpy as np
    import torch
    from conftest import golden
    from epnet_amd import roipool3d_utils
    fx = golden("roipool3d_ref.npz")
    n = fx["pts"].shape[0]
    masks = roipool3d_utils.pts_in_boxes3d_cpu(torch.from_numpy(fx["pts"]), torch.from_numpy(fx["boxes3d"]))
    flags = np.unpackbits(fx["pts_flag"], axis=1)[:, :n].astype(bool)
    np.testing.assert_array_equal(torch.stack(masks).numpy(), flags)
    pp, pf, ef = roipool3d_utils.roipool_pc_cpu(torch.from_numpy(fx["pts"]), torch.from_numpy(fx["pts_feature"]),
                                               torch.from_numpy(fx["boxes3d"]), fx["pooled_pts"].shape[1])
    np.testing.assert_array_equal(pp.numpy(), fx["pooled_pts"])
    np.testing.assert_array_equal(pf.numpy(), fx["pooled_features"])
    np.testing.assert_array_equal(ef.numpy(), fx["pooled_empty_flag"])


def test_scene_index_size_is_the_documented_layout(hiplib):
    """epnet_scene_index_bytes (no GPU needed): per scene np float4 rows (np = the power of two >= max(n, 2048)), one box of 6
    floats per 64 and per 256 rows and, beyond 16384 points, np floats of sampling scratch (include/epnet_ops.h) -- a caller
    that sized the buffer by the formula of an older header would get EPNET_ENOMEM, so the formula is pinned here"""
    def want(b, n):
        if n < 1024 or n > 65536:
            return 0
        np_ = 2048
        while np_ < n:
            np_ *= 2
        return b * (np_ * 16 + (np_ // 64 + np_ // 256) * 24 + (np_ * 4 if n > 16384 else 0))
    for b, n in ((1, 1024), (3, 4096), (2, 16384), (2, 16385), (1, 40000), (4, 65536), (1, 1023), (1, 65537), (0, 4096)):
        assert hiplib.epnet_scene_index_bytes(b, n) == (want(b, n) if b > 0 else 0), (b, n)


def test_tuning_round_trip_and_restore(hiplib):
    """epnet_set_tuning / epnet_get_tuning: the kernel-selection overrides, -1 = the library's own choice"""
    from epnet_amd import _lib
    v = ctypes.c_int()
    for name, value in (("EPNET_BQ_PAIR", 1), ("EPNET_BQ_PAIR", 0), ("EPNET_FPS_PWAVES", 8), ("EPNET_FPS_WAVES", 16),
                        ("EPNET_FPS_PRUNE_MIN", 4096), ("EPNET_NN_TILE_MIN_BUCKETS", 1000000000)):
        assert hiplib.epnet_get_tuning(name.encode(), ctypes.byref(v)) == 0
        before = v.value
        assert hiplib.epnet_set_tuning(name.encode(), value) == 0
        assert hiplib.epnet_get_tuning(name.encode(), ctypes.byref(v)) == 0 and v.value == value
        assert hiplib.epnet_set_tuning(name.encode(), -1) == 0
        assert hiplib.epnet_get_tuning(name.encode(), ctypes.byref(v)) == 0 and v.value == -1
        assert hiplib.epnet_set_tuning(name.encode(), before) == 0
    with _lib.tuning(EPNET_BQ_STREAM=1, EPNET_FPS_PRUNE=0):
        assert hiplib.epnet_get_tuning(b"EPNET_BQ_STREAM", ctypes.byref(v)) == 0 and v.value == 1
        with pytest.raises(ZeroDivisionError):   # restored on the way out, also when the body raises
            with _lib.tuning(EPNET_BQ_STREAM=0):
                1 / 0
        assert hiplib.epnet_get_tuning(b"EPNET_BQ_STREAM", ctypes.byref(v)) == 0 and v.value == 1
    assert hiplib.epnet_get_tuning(b"EPNET_BQ_STREAM", ctypes.byref(v)) == 0 and v.value == -1
    assert hiplib.epnet_get_tuning(b"EPNET_FPS_PRUNE", ctypes.byref(v)) == 0 and v.value == -1


def test_tuning_rejects_unknown_names_and_values(hiplib):
    from epnet_amd import _lib
    v = ctypes.c_int(7)
    einval = -1
    for name in (b"EPNET_FPS_WIDE", b"EPNET_FPS_CTR", b"EPNET_FPS_BIG_WAVES", b"EPNET_BQ_PAD_KB", b"EPNET_GATHER_NO_QUAD",
                 b"EPNET_RUNSUM_TILE", b"EPNET_RUNSUM_PARTS", b"EPNET_BQ_PAIRS", b"bq_pair", b""):
        assert hiplib.epnet_set_tuning(name, 1) == einval, name
        assert hiplib.epnet_get_tuning(name, ctypes.byref(v)) == einval, name
    assert hiplib.epnet_set_tuning(None, 1) == einval and hiplib.epnet_get_tuning(b"EPNET_BQ_PAIR", None) == einval
    for name, value in (("EPNET_BQ_PAIR", 2), ("EPNET_BQ_STREAM", -2), ("EPNET_BQ_ORDERED", 5), ("EPNET_FPS_PRUNE", 2),
                        ("EPNET_FPS_PWAVES", 2), ("EPNET_FPS_PWAVES", 16), ("EPNET_FPS_WAVES", 3), ("EPNET_FPS_WAVES", 32),
                        ("EPNET_FPS_WAVES", 0), ("EPNET_FPS_PRUNE_MIN", -5), ("EPNET_NN_TILE_MIN_BUCKETS", -2)):
        assert hiplib.epnet_set_tuning(name.encode(), value) == einval, (name, value)
    assert v.value == 7   # nothing written on failure
    with pytest.raises(_lib.EpnetError, match="EPNET_FPS_WIDE"):
        with _lib.tuning(EPNET_FPS_WIDE=1):
            pass
    with pytest.raises(_lib.EpnetError, match="EPNET_BQ_PAIR"):
        with _lib.tuning(EPNET_BQ_STREAM=1, EPNET_BQ_PAIR=3):
            pass
    assert hiplib.epnet_get_tuning(b"EPNET_BQ_STREAM", ctypes.byref(v)) == 0 and v.value == -1   # the first one was undone


def test_tuning_is_seeded_from_the_environment_once(hiplib):
    """a process started with EPNET_BQ_PAIR=1 reads 1 back (what an A/B run of the unchanged bench.py relies on); a malformed
    or out-of-range value is ignored"""
    import subprocess
    import sys
    code = ("import ctypes; from epnet_amd import _lib; l = _lib.lib(); v = ctypes.c_int()\n"
            "for name in ('EPNET_BQ_PAIR', 'EPNET_FPS_PWAVES', 'EPNET_FPS_PRUNE_MIN', 'EPNET_BQ_STREAM'):\n"
            "    assert l.epnet_get_tuning(name.encode(), ctypes.byref(v)) == 0; print(name, v.value)\n")
    env = dict(os.environ, EPNET_BQ_PAIR="1", EPNET_FPS_PWAVES="2", EPNET_FPS_PRUNE_MIN="4096x")
    env.pop("EPNET_BQ_STREAM", None)
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split("\n")[:4] == ["EPNET_BQ_PAIR 1", "EPNET_FPS_PWAVES -1", "EPNET_FPS_PRUNE_MIN -1", "EPNET_BQ_STREAM -1"]


def test_library_reads_its_environment_in_one_place():
    """no launcher calls getenv: the kernel-selection overrides are read once, by the table's seeding function in host.cpp, so a
    workspace query and the launch it sizes cannot see different values, and a setenv elsewhere in the process cannot race a launch"""
    csrc = os.path.join(ROOT, "epnet_amd", "csrc")
    seen = {}
    for f in sorted(os.listdir(csrc)):
        text = open(os.path.join(csrc, f)).read()
        if "getenv" in text:
            seen[f] = text.count("getenv")
    assert seen == {"host.cpp": 1}, seen
    text = open(os.path.join(csrc, "host.cpp")).read()
    start = text.index("bool seed_from_env()")
    body_start = text.index("{", start)
    depth, i = 0, body_start
    while True:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        if depth == 0:
            break
        i += 1
    assert "getenv" in text[body_start:i]

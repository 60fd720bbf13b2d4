"""The training losses without a GPU: the numpy restatement (tests/loss_restate.py) against the reference's own run stored in
tests/golden/loss.npz, the fixture's coverage, the C ABI's argument checks and the Python surface's refusals.

Bounds. Restatement in float64 against the reference in float64: 1e-9 of the largest magnitude of the tensor compared -- both are
float64 evaluations of the same few hundred operations per row in another order, rounding is seven orders below and a wrong
column, a missing factor or a detached factor six orders above. Restatement in float32 against the reference in float64: the
bound the generator stored per tensor, 4 x the reference's own float32 deviation and not less than 1e-6 of the largest
magnitude -- the bound the kernel is held to on the GPU (test_loss_gpu.py), shown here to hold for an independent fp32
implementation."""
import ctypes
import os

import numpy as np
import pytest

import loss_cases as lc
import loss_restate as lr

FX = lc.load()
NAMES = list(lc.CASES)
GRADS = ("grad_cls", "grad_reg", "grad_iou_branch")


def compare(name, out, bound_of):
    """every scalar and every gradient of a case; bound_of(kind, key, reference float64 array) -> absolute bound"""
    failures = []
    for key, term, want, stored in lc.reference_scalars(FX, name):
        got = float(out["terms"][term])
        tol = bound_of("scalar", key, np.array([want]), stored)
        print("%s %-18s got % .9e want % .9e |diff| %.2e bound %.2e" % (name, key, got, want, abs(got - want), tol))
        if not abs(got - want) <= tol:
            failures.append((key, got, want, tol))
    for g in GRADS:
        k = name + "__" + g + "_f64"
        if k not in FX.files:
            continue
        want = FX[k]
        got = np.asarray(out[g], np.float64).reshape(want.shape)
        tol = bound_of("grad", g, want, float(FX[name + "__" + g + "_bound"]))
        diff = float(np.abs(got - want).max()) if want.size else 0.0
        print("%s %-18s max |diff| %.2e bound %.2e (max |want| %.2e)" % (name, g, diff, tol, float(np.abs(want).max())))
        if not diff <= tol:
            failures.append((g, diff, tol))
    assert not failures, failures


@pytest.mark.parametrize("name", NAMES)
def test_restatement_float64_equals_reference_float64(name):
    out = lr.box_loss(lc.settings(name), dtype=np.float64, **lc.inputs(FX, name))
    compare(name, out, lambda kind, key, want, stored: 1e-9 * float(np.abs(want).max()))


@pytest.mark.parametrize("name", NAMES)
def test_restatement_float32_within_stored_bounds(name):
    out = lr.box_loss(lc.settings(name), dtype=np.float32, **lc.inputs(FX, name))
    assert out["grad_reg"].dtype == np.float32 and out["terms"]["total"].dtype == np.float32
    compare(name, out, lambda kind, key, want, stored: stored)


def test_stored_bounds_follow_the_rule():
    """4 x the reference's float32 deviation, floor 1e-6 of the largest magnitude: recomputed from the two stored runs"""
    for name in NAMES:
        pre = name + "__"
        for g in GRADS:
            if pre + g + "_f64" not in FX.files:
                continue
            g64, g32 = FX[pre + g + "_f64"], FX[pre + g + "_f32"].astype(np.float64)
            want = max(4 * float(np.abs(g32 - g64).max()), 1e-6 * float(np.abs(g64).max())) if g64.size else 0.0
            assert float(FX[pre + g + "_bound"]) == want, (name, g)
        s64, s32 = FX[pre + "scalars_f64"], FX[pre + "scalars_f32"].astype(np.float64)
        np.testing.assert_array_equal(FX[pre + "scalars_bound"], np.maximum(4 * np.abs(s32 - s64), 1e-6 * np.abs(s64)))


def _reference_at_hand():
    from oracle import build_ref
    return build_ref.available()


@pytest.mark.skipif(not _reference_at_hand(), reason="the generator needs the reference checkout (build container only)")
def test_generator_reproduces_the_committed_fixture(tmp_path):
    """as test_oracle_golden.py does for its fixtures: the committed file is what the generator writes today (run in a child
    process: the generator replaces torch attributes while the reference runs). Names, inputs and counts bit for bit; what
    torch computed -- on another processor its vector math may round differently -- within 1e-9 of the largest magnitude for the
    float64 run, 1e-5 for the float32 run, and the bounds derived from their difference within a factor of 4"""
    import subprocess
    import sys
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import make_golden_loss as m; m.HERE = %r; m.main()"
            % (os.path.join(lc.HERE, "golden"), str(tmp_path)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    fresh = np.load(os.path.join(str(tmp_path), "loss.npz"))
    assert sorted(fresh.files) == sorted(FX.files)
    for k in FX.files:
        a, b = fresh[k], FX[k]
        if k.endswith("_f64") or k.endswith("_f32"):
            scale = float(np.abs(b).max()) if b.size else 0.0
            np.testing.assert_allclose(a, b, rtol=0, atol=(1e-9 if k.endswith("_f64") else 1e-5) * scale, err_msg=k)
        elif k.endswith("_bound"):
            a, b = np.atleast_1d(a), np.atleast_1d(b)
            assert ((a == 0) == (b == 0)).all() and (a[b > 0] <= 4 * b[b > 0]).all() and (b[b > 0] <= 4 * a[b > 0]).all(), k
        else:
            np.testing.assert_array_equal(a, b, err_msg=k)


def _aux(name, dtype=np.float64):
    return lr.box_loss(lc.settings(name), dtype=dtype, **lc.inputs(FX, name))["aux"]


def test_fixture_coverage():
    assert os.path.getsize(lc.FIXTURE) < 1 << 20
    for stage, rows in (("rpn", 512), ("rcnn", 128)):
        names = [n for n in NAMES if lc.CASES[n][0] == stage]
        s = lc.settings(names[0])
        nb, nh = int(s["loc_scope"] / s["loc_bin_size"]) * 2, s["num_head_bin"]
        seen = {"x_bin": set(), "z_bin": set(), "ry_bin": set()}
        flips = set()
        for n in names:
            assert FX[n + "__pred_reg_f16"].shape == (rows, lr.channels(s))
            aux = _aux(n)
            for k in seen:
                seen[k].update(int(v) for v in aux[k])
            flips.update(bool(v) for v in aux["opposite"])
            # the kink margins hold for every foreground row, and few rows had to be redrawn for that
            assert (aux["margin_smooth_l1"] >= 1e-4).all() and (aux["margin_relative"] >= 1e-4).all(), n
            assert int(FX[n + "__redrawn"]) <= 0.01 * rows, n
            # the labels do not depend on the precision
            a32 = _aux(n, np.float32)
            for k in ("x_bin", "z_bin", "ry_bin", "opposite"):
                np.testing.assert_array_equal(aux[k], a32[k])
        assert seen["x_bin"] == set(range(nb)) and seen["z_bin"] == set(range(nb)) and seen["ry_bin"] == set(range(nh)), (stage, seen)
        assert flips == ({False, True} if stage == "rcnn" else {False})
        clamps = ("clamp_x", "clamp_y", "clamp_z", "clamp_volume", "clamp_iou")
        for n in names:
            kind = lc.CASES[n][1]
            aux = _aux(n)
            if kind == "a":      # trained-like: boxes overlap, no clamp is active
                assert not any(aux[k].any() for k in clamps), n
            if kind == "b":      # N(0,1): every clamp active in some row
                assert all(aux[k].any() for k in clamps), (n, {k: int(aux[k].sum()) for k in clamps})
    # no foreground row, exactly one, both IoU types, the IoU branch on and off, both classification losses, -1 labels
    fg = {n: int(len(_aux(n)["fg_rows"])) for n in NAMES}
    assert fg["rpn_nofg"] == 0 and fg["rcnn_nofg"] == 0 and fg["rpn_onefg"] == 1 and fg["rcnn_onefg"] == 1
    for stage in ("rpn", "rcnn"):
        mine = [lc.CASES[n] for n in NAMES if lc.CASES[n][0] == stage]
        assert {c[2] for c in mine} == set(lr.IOU_TYPES) and {c[3] for c in mine} == {"SigmoidFocalLoss", "BinaryCrossEntropy"}
    assert {lc.CASES[n][4] for n in NAMES if lc.CASES[n][0] == "rcnn"} == {False, True}
    assert any((FX[n + "__cls_label"] == -1).any() for n in NAMES if lc.CASES[n][0] == "rpn")
    # the IoU branch's input clamps, both sides
    q = FX["rcnn_b_bin_branch__iou_branch"][_aux("rcnn_b_bin_branch")["fg_rows"]]
    assert (q < 1e-4).any() and (q > 0.9999).any()


def test_masked_rows_contribute_nothing():
    """the RCNN's BinaryCrossEntropy with -1 labels (the reference cannot be run on them under a current torch: it hands the -1 to
    F.binary_cross_entropy as a target): a masked row adds nothing to the loss and gets a zero gradient, and the mean is over
    the valid rows -- pinned on the restatement, which the kernel is compared with on the GPU"""
    name = "rcnn_b_bin"
    s, inp = lc.settings(name), lc.inputs(FX, name)
    full = lr.box_loss(s, **inp)
    masked = dict(inp, cls_label=inp["cls_label"].copy())
    drop = np.arange(0, 128, 5)
    masked["cls_label"][drop] = -1
    out = lr.box_loss(s, **masked)
    keep = np.setdiff1d(np.arange(128), drop)
    only = lr.box_loss(dict(s), **{k: (v[keep] if v is not None else None) for k, v in masked.items()})
    assert float(out["terms"]["cls_valid"]) == len(keep)
    np.testing.assert_allclose(float(out["terms"]["loss_cls"]), float(only["terms"]["loss_cls"]), rtol=1e-13)
    fg = set(int(v) for v in out["aux"]["fg_rows"])
    assert all(out["grad_cls"][r] == 0 for r in drop if r not in fg)
    assert float(out["terms"]["loss_cls"]) != float(full["terms"]["loss_cls"])


def test_no_foreground_is_exactly_zero():
    for name in ("rpn_nofg", "rcnn_nofg"):
        for dt in (np.float64, np.float32):
            out = lr.box_loss(lc.settings(name), dtype=dt, **lc.inputs(FX, name))
            t = out["terms"]
            assert all(t[k] == 0 for k in lr.TERM_NAMES[5:18]) and not out["grad_reg"].any()
            assert t["total"] == t["loss_cls"]


# ---- the C ABI without a device ------------------------------------------------------------------------------------------
def _call(hiplib, rows=128, c=46, scope=1.5, bin_size=0.5, nh=9, iou=1, cls=1, ptr=4096, ws=4096, ws_bytes=1 << 20, branch=(None, None), terms=4096):
    fake = ctypes.c_void_p(ptr) if ptr else None      # never dereferenced: every refusal comes before a launch
    return hiplib.epnet_box_loss(rows, c, scope, bin_size, nh, 1, iou, cls, 0.25, 2.0, 1.0, 1.0, 1.0, 1.0, 5.0, fake, fake, fake, fake, None,
                                 branch[0], fake, ctypes.c_void_p(terms) if terms else None, fake, fake, branch[1],
                                 ctypes.c_void_p(ws) if ws else None, ws_bytes, None)


def test_abi_refusals_without_a_device(hiplib):
    einval, enomem, elimit = -1, -3, -4
    assert _call(hiplib, rows=0) == 0                                       # an empty problem: nothing to do, nothing written
    assert _call(hiplib, rows=0, ptr=0, ws=0, ws_bytes=0, terms=0) == 0
    assert _call(hiplib, rows=-1) == einval
    assert _call(hiplib, ptr=0) == einval and _call(hiplib, terms=0) == einval
    assert _call(hiplib, c=45) == einval and _call(hiplib, c=76) == einval     # c != 4 nb + 1 + 2 nh + 3
    assert _call(hiplib, iou=2) == einval and _call(hiplib, iou=-1) == einval and _call(hiplib, cls=3) == einval
    assert _call(hiplib, branch=(ctypes.c_void_p(4096), None)) == einval      # the branch's input and gradient come together
    assert _call(hiplib, ws=0) == enomem and _call(hiplib, ws_bytes=4096 + 2 * 64 - 1) == enomem
    assert _call(hiplib, ws=4104) == einval                                    # 16-byte alignment
    assert _call(hiplib, c=4 * 34 + 1 + 18 + 3, scope=17.0, bin_size=1.0) == elimit
    assert _call(hiplib, scope=0.0) == einval and _call(hiplib, nh=0) == einval


def test_abi_workspace_formula(hiplib):
    """pinned: a caller that sized its scratch by the header's formula must not get EPNET_ENOMEM from a later library"""
    for rows, c in ((1, 46), (63, 46), (64, 76), (65, 76), (4097, 76), (2 * 16384, 76), (256 * 16384, 76)):
        assert hiplib.epnet_box_loss_workspace_bytes(rows, c) == 4096 + ((rows + 63) // 64) * 64, (rows, c)
    assert hiplib.epnet_box_loss_workspace_bytes(0, 76) == 0 and hiplib.epnet_box_loss_workspace_bytes(-5, 76) == 0


# ---- the Python surface --------------------------------------------------------------------------------------------------
def test_surface_refuses_cpu_tensors(hiplib):
    import torch
    from epnet_amd import loss_utils
    with pytest.raises(RuntimeError, match="CUDAtensor"):
        loss_utils.rpn_loss(torch.zeros((1, 8, 1)), torch.zeros((1, 8, 76)), torch.zeros((1, 8), dtype=torch.long), torch.zeros((1, 8, 7)))
    ret = {"rcnn_cls": torch.zeros((8, 1)), "rcnn_reg": torch.zeros((8, 46)), "cls_label": torch.zeros((8,), dtype=torch.long),
           "reg_valid_mask": torch.zeros((8,), dtype=torch.long), "gt_of_rois": torch.zeros((8, 7))}
    with pytest.raises(RuntimeError, match="CUDAtensor"):
        loss_utils.rcnn_loss(ret)


def test_surface_refuses_what_the_reference_cannot_run():
    import torch
    from epnet_amd import loss_utils
    z = torch.zeros((1, 8, 1))
    cfg = loss_utils.default_cfg()
    cfg.RPN.LOC_XZ_FINE = False
    with pytest.raises(NotImplementedError, match="x_res_l"):
        loss_utils.rpn_loss(z, z, z, z, cfg)
    cfg = loss_utils.default_cfg()
    cfg.RCNN.LOC_Y_BY_BIN = True
    with pytest.raises(NotImplementedError, match="y_offset_l"):
        loss_utils.rcnn_loss({}, cfg)
    cfg = loss_utils.default_cfg()
    cfg.RCNN.SIZE_RES_ON_ROI = True
    with pytest.raises(NotImplementedError, match="SIZE_RES_ON_ROI"):
        loss_utils.rcnn_loss({}, cfg)
    cfg = loss_utils.default_cfg()
    cfg.RCNN.LOSS_CLS = "CrossEntropy"
    with pytest.raises(NotImplementedError, match="CrossEntropy"):
        loss_utils.rcnn_loss({"rcnn_cls": z, "rcnn_reg": z, "gt_of_rois": z, "cls_label": z, "reg_valid_mask": z}, cfg)


def test_term_names_cover_the_reference_keys():
    """every key the reference's tb_dict / disp_dict / reg_loss_dict gets in any fixture case has a slot in `terms`"""
    from epnet_amd import loss_cuda, loss_utils
    assert loss_utils.TERM_NAMES == lr.TERM_NAMES and len(lr.TERM_NAMES) == loss_cuda.TERMS
    assert len(loss_utils.RPN_TERM_NAMES) == len(loss_utils.RCNN_TERM_NAMES) == loss_cuda.TERMS
    assert len(set(loss_utils.RPN_TERM_NAMES)) == loss_cuda.TERMS and len(set(loss_utils.RCNN_TERM_NAMES)) == loss_cuda.TERMS
    seen_rpn, seen_rcnn = set(), set()
    for name in NAMES:
        keys = set(str(k) for k in FX[name + "__tb_keys"]) | set(str(k) for k in FX[name + "__disp_keys"])
        # (a model_fn run logs both stages; with the RCNN's focal loss its pos / neg parts go under the RPN's keys)
        seen_rpn |= {k for k in keys if k.startswith("rpn")}
        seen_rcnn |= {k for k in keys if not k.startswith("rpn") and k != "loss"}
    assert len(seen_rpn) >= 10 and len(seen_rcnn) >= 20
    assert seen_rpn <= set(loss_utils.RPN_TERM_NAMES), seen_rpn - set(loss_utils.RPN_TERM_NAMES)
    known = set(loss_utils.RCNN_TERM_NAMES) | set(loss_utils.RCNN_KEY_ALIASES)
    assert seen_rcnn <= known, seen_rcnn - known
    assert set(loss_utils.RCNN_KEY_ALIASES.values()) <= set(loss_utils.RCNN_TERM_NAMES)
    # and the slot a key names is the slot the fixture comparison reads it from
    for keys, names, alias in ((lc.RPN_KEYS, loss_utils.RPN_TERM_NAMES, {}), (lc.RCNN_KEYS, loss_utils.RCNN_TERM_NAMES, loss_utils.RCNN_KEY_ALIASES)):
        for key, term in keys.items():
            slot = names[lr.TERM_NAMES.index(term)]
            if key in ("rpn_loss", "rcnn_loss"):      # the fixtures' train weights are 1: disp_dict's and tb_dict's value coincide
                continue
            assert alias.get(key, key) == slot, (key, term, slot)

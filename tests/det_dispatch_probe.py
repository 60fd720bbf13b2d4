"""Child-process probe for tests/test_deterministic_cpu.py: which C-ABI entry points the stand-in gradient wrappers call with
torch's deterministic flag off and on, recorded against a stand-in for the loaded library (no GPU needed).

torch.use_deterministic_algorithms is process-wide (and while it is on, every fresh CPU tensor is filled with NaN), so the flag
is only ever switched on here, in a process of its own: the test process never sees it. Prints one JSON object."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

from epnet_amd import _lib, li_fusion, pointnet2_cuda as ext  # noqa: E402

OPS = ["gather_points_grad", "group_points_grad", "group_concat_grad", "three_interpolate_grad", "feature_gather_grad",
       "group_linear_grad_w"]


class Recorder:
    def __init__(self):
        self.calls = []
        self.refuse = ()

    def __getattr__(self, name):
        if not name.startswith("epnet_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append(name)
            if name == "epnet_strerror":
                return b"problem size outside what the kernels support"
            if name == "epnet_last_hip_error":
                return b""
            if name in self.refuse:
                return -4
            return 4096 if name.endswith("workspace_bytes") else 0
        return fn


class _NoDevice:
    def __init__(self, t):
        pass

    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


def call(op):
    z = lambda *s: torch.zeros(s)
    zi = lambda *s: torch.zeros(s, dtype=torch.int32)
    if op == "gather_points_grad":
        ext.gather_points_grad_wrapper(2, 3, 16, 4, z(2, 3, 4), zi(2, 4), z(2, 3, 16))
    elif op == "group_points_grad":
        ext.group_points_grad_wrapper(2, 3, 16, 4, 2, z(2, 3, 4, 2), zi(2, 4, 2), z(2, 3, 16))
    elif op == "group_concat_grad":
        ext.group_concat_grad_wrapper(2, 3, 16, 4, 2, z(2, 6, 4, 2), zi(2, 4, 2), z(2, 3, 16), True)
    elif op == "three_interpolate_grad":
        ext.three_interpolate_grad_wrapper(2, 3, 16, 4, z(2, 3, 16), zi(2, 16, 3), z(2, 16, 3), z(2, 3, 4))
    elif op == "group_linear_grad_w":
        ext.group_linear_grad_w_wrapper(2, 3, 16, 4, 2, z(2, 3, 4, 2), z(2, 16, 3), z(2, 4, 3), zi(2, 4, 2), z(3, 3))
    elif op == "feature_gather_grad":   # through the LI-Fusion sampler's autograd Function
        fmap = z(2, 3, 5, 7).requires_grad_(True)
        li_fusion.Feature_Gather(fmap, z(2, 16, 2)).sum().backward()


def main():
    rec = Recorder()
    _lib.lib = lambda: rec
    ext.dev_ptr = lambda t, name, dtype: t.data_ptr()
    ext.on_device_of = _NoDevice
    result = {"initial_flag": torch.are_deterministic_algorithms_enabled(), "off": {}, "on": {}}
    for op in OPS:
        for mode in ("off", "on"):
            torch.use_deterministic_algorithms(mode == "on")
            rec.calls = []
            call(op)
            result[mode][op] = rec.calls
    # a shape the deterministic path refuses: a RuntimeError that names the op, and no default kernel behind it
    torch.use_deterministic_algorithms(True)
    rec.calls, rec.refuse = [], ("epnet_group_points_grad_det",)
    try:
        ext.group_points_grad_wrapper(2, 3, 16, 4, 2, torch.zeros(2, 3, 4, 2), torch.zeros((2, 4, 2), dtype=torch.int32),
                                      torch.zeros(2, 3, 16))
        result["refused"] = {"raised": None, "calls": rec.calls}
    except RuntimeError as e:
        result["refused"] = {"raised": str(e), "calls": rec.calls}
    torch.use_deterministic_algorithms(False)
    print(json.dumps(result))


if __name__ == "__main__":
    main()

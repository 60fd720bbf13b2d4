"""Tensor -> raw pointer plumbing shared by the three extension stand-ins."""
import torch


def _bad(name, why):
    raise RuntimeError("%s %s" % (name, why))


def dev_ptr(t, name, dtype):
    """device address of a contiguous GPU tensor of the given dtype (RuntimeError otherwise, as the
    reference's CHECK_CUDA / CHECK_CONTIGUOUS do -- e.g. lib/utils/iou3d/src/iou3d.cpp:7-9 -- plus a
    dtype check the reference lacks: there a wrong dtype is undefined behaviour)."""
    if not isinstance(t, torch.Tensor):
        _bad(name, "must be a torch.Tensor")
    if not t.is_cuda:
        _bad(name, "must be a CUDAtensor (epnet_amd has no CPU fallback)")
    if not t.is_contiguous():
        _bad(name, "must be contiguous")
    if t.dtype != dtype:
        _bad(name, "must have dtype %s, got %s" % (dtype, t.dtype))
    return t.data_ptr()


# the 16-bit feature types of torch.autocast and their codes in include/epnet_ops.h (EPNET_F16, EPNET_BF16)
ROWS16 = {torch.float16: 1, torch.bfloat16: 2}


def is_rows16(t):
    return isinstance(t, torch.Tensor) and t.dtype in ROWS16


def dev_ptr16(t, name, dtype):
    """dev_ptr for the 16-bit feature rows of the *_h entry points: `dtype` is one of ROWS16 (float64 and every other type
    raise exactly as dev_ptr does)"""
    if dtype not in ROWS16:
        _bad(name, "must have dtype torch.float32, torch.float16 or torch.bfloat16, got %s" % dtype)
    return dev_ptr(t, name, dtype)


def as_f32(t):
    """the one upcast at a boundary of the 16-bit path: a float16 / bfloat16 tensor becomes float32 (exact;
    autograd casts the gradient back to the tensor's own type), anything else -- float32, integers, None -- passes unchanged,
    so a float32 caller runs exactly what it ran before"""
    return t.float() if is_rows16(t) else t


def f32_region(fn):
    """decorator of a head-side entry point (losses, proposal / target / detection layers): its body is box geometry on the
    float32 tensors `as_f32` made, so an enclosing torch.autocast must not turn its matmuls into 16-bit ones. Outside autocast
    this changes nothing."""
    import functools

    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        with torch.autocast("cuda", enabled=False):
            return fn(*args, **kwargs)
    return wrapped


def host_ptr(t, name, dtype):
    if not isinstance(t, torch.Tensor):
        _bad(name, "must be a torch.Tensor")
    if t.is_cuda:
        _bad(name, "must be a CPU tensor")
    if not t.is_contiguous():
        _bad(name, "must be contiguous")
    if t.dtype != dtype:
        _bad(name, "must have dtype %s, got %s" % (dtype, t.dtype))
    return t.data_ptr()


def need(t, numel, name):
    if t.numel() < numel:
        _bad(name, "has %d elements, the call needs %d" % (t.numel(), numel))


def opt_ptr(t, name, dtype, count):
    """device address of an optional tensor (None -> NULL)"""
    if t is None:
        return None
    p = dev_ptr(t, name, dtype)
    need(t, count, name)
    return p


class on_device_of:
    """Makes the tensor's device current for the launch and yields its current HIP stream.

    The ops are called from several host threads with different current devices under
    nn.DataParallel (tools/train_rcnn.py:221-223), so device and stream are always derived from
    the tensor, never from global state."""

    __slots__ = ("dev", "prev")

    def __init__(self, t):
        self.dev = t.device.index
        self.prev = None

    def __enter__(self):
        cur = torch.cuda.current_device()
        if cur != self.dev:
            self.prev = cur
            torch.cuda.set_device(self.dev)
        return torch.cuda.current_stream(self.dev).cuda_stream

    def __exit__(self, *exc):
        if self.prev is not None:
            torch.cuda.set_device(self.prev)
        return False


def writes(*names):
    """decorator of an extension stand-in: the named arguments (tensors, lists of tensors or None) are OUTPUTS the kernels
    fill through ``data_ptr()``. The reference's pybind extensions write the same way, invisibly to autograd; here every
    output's version counter is moved after the launch, so that anything remembered about the old contents (autograd's
    saved-tensor check, pointnet2_utils.scene_index) is known to be stale."""
    import functools
    import inspect

    def deco(fn):
        params = list(inspect.signature(fn).parameters)
        slots = [(params.index(n), n) for n in names]

        @functools.wraps(fn)
        def wrapped(*args, **kwargs):
            result = fn(*args, **kwargs)
            for pos, name in slots:
                out = args[pos] if pos < len(args) else kwargs.get(name)
                if out is None:
                    continue
                torch._C._increment_version(tuple(out) if isinstance(out, (list, tuple)) else (out,))
            return result
        return wrapped
    return deco

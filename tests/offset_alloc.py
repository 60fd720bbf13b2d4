"""Guarded device tensors whose data pointer sits a chosen number of bytes past a 16-byte boundary.

Every tensor the other GPU tests make comes from torch's allocator or from ``conftest.GuardedAlloc``; both hand out 16-byte
aligned bodies, so the kernels and branches the library selects for a pointer OFF such a boundary never ran. ``skewed`` builds
the tensor as ``GuardedAlloc`` does -- a block of ``conftest.CANARY`` bytes, the body ``GUARD_BYTES`` in -- and then moves the
body ``skew_bytes`` further. A contiguous slice of a real tensor (``rcnn_reg[1:]``, ``xyz[1:]``, a view into a flat buffer) has
such a pointer, and ``_tensor.dev_ptr`` asks for contiguity alone.

``check()`` looks at the canaries of everything made since the last call, after a synchronize. Outputs are made with
``output()``: prefilled with a sentinel, so that an element the kernel left out shows (``unwritten``).
"""
import numpy as np
import torch

from conftest import CANARY, GUARD_BYTES

SKEWS = (0, 4, 8, 12)            # 4-byte types; 0 = the aligned tensor, guarded the same way
SENTINEL_F32 = -7.015625e30      # exact in float32; no case of the tests computes it
SENTINEL_I32 = -0x5A5A5A5B
SENTINEL_I64 = -0x5A5A5A5A5A5A5A5B
SENTINEL_U8 = 0x3C

_live = []


def _sentinel(dtype):
    return {torch.float32: SENTINEL_F32, torch.int32: SENTINEL_I32, torch.int64: SENTINEL_I64, torch.uint8: SENTINEL_U8}[dtype]


def skewed(array_or_shape, dtype=torch.float32, skew_bytes=4, device="cuda:0"):
    """a contiguous device tensor with ``data_ptr() % 16 == skew_bytes`` inside a block of canaries. ``array_or_shape``: a numpy
    array or a tensor (its values are copied in, converted to ``dtype``), or a shape (the body is filled with the sentinel)"""
    values = None
    if isinstance(array_or_shape, np.ndarray):
        values = torch.from_numpy(np.ascontiguousarray(array_or_shape))
    elif isinstance(array_or_shape, torch.Tensor):
        values = array_or_shape.detach()
    shape = tuple(values.shape) if values is not None else tuple(int(v) for v in (array_or_shape if isinstance(array_or_shape, (tuple, list, torch.Size)) else (array_or_shape,)))
    size = torch.empty((), dtype=dtype).element_size()
    assert skew_bytes in SKEWS and skew_bytes % size == 0, (skew_bytes, dtype)
    nbytes = int(np.prod(shape, dtype=np.int64)) * size
    pad = (-nbytes) % 16 + 16    # the canaries behind the body start on a boundary of their own, past any skew
    raw = torch.full((GUARD_BYTES + nbytes + pad + GUARD_BYTES,), CANARY, dtype=torch.uint8, device=device)
    assert raw.data_ptr() % 16 == 0
    start = GUARD_BYTES + skew_bytes
    body = torch.empty((0,), dtype=dtype, device=device).set_(raw.untyped_storage(), start // size, shape)
    assert body.is_contiguous() and body.data_ptr() % 16 == skew_bytes and body.data_ptr() == raw.data_ptr() + start
    if values is not None:
        body.copy_(values.to(dtype))
    else:
        body.fill_(_sentinel(dtype))
    _live.append((raw, start, nbytes, shape, dtype))
    return body


def output(shape, dtype=torch.float32, skew_bytes=4, device="cuda:0"):
    """an output tensor: the sentinel in every element"""
    return skewed(shape, dtype, skew_bytes, device)


def unwritten(t):
    """how many elements of an output still hold the sentinel"""
    if t.dtype == torch.float32:
        return int((t.view(torch.int32) == torch.tensor(SENTINEL_F32, dtype=torch.float32).view(torch.int32).item()).sum())
    return int((t == _sentinel(t.dtype)).sum())


def untouched(t):
    return unwritten(t) == t.numel()


def check():
    """the canaries of every tensor made since the last check; synchronizes first"""
    torch.cuda.synchronize()
    live = list(_live)
    del _live[:]
    for raw, start, nbytes, shape, dtype in live:
        head, tail = raw[:start], raw[start + nbytes:]
        assert bool((head == CANARY).all()), ("bytes written BEFORE a tensor", shape, dtype, start - GUARD_BYTES)
        assert bool((tail == CANARY).all()), ("bytes written PAST a tensor", shape, dtype, start - GUARD_BYTES, int((tail != CANARY).nonzero()[0]))


def forget():
    del _live[:]

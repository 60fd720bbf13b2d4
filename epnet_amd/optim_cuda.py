"""Stand-in of an extension module the reference does not have: its optimiser step is Python over stock torch
(tools/train_utils/train_utils.py:126-136, fastai_optim.py:132-149, learning_schedules_fastai.py:40-73).
``adam_onecycle_step_gpu`` is the one call of ``epnet_adam_onecycle_step`` (include/epnet_ops.h): clip, decay, Adam and the
schedule's row for the device counter's step, on the tensors' device and current stream, nothing read back.
"""
import torch

from . import _lib
from . import pointnet2_utils
from ._tensor import dev_ptr, need, on_device_of, writes

_F = torch.float32
_I = torch.int32
_L = torch.int64
_D = torch.float64

CHUNK = 4096  # EPNET_OPTIM_CHUNK
ROW = 8       # EPNET_OPTIM_ROW
STATS = 8     # EPNET_OPTIM_STATS
STATS_NAMES = ("total_norm", "coef", "lr", "mom", "step", "past_end")
SCALED_STATS_NAMES = ("scale", "skipped")  # stats[6], stats[7] of the scaled step (zeros after the plain one)


def workspace(like, chunks):
    """the call's scratch, from the package's allocation helper (the GPU tests put canaries around it)"""
    nbytes = _lib.lib().epnet_adam_onecycle_workspace_bytes(chunks)
    return pointnet2_utils._new(like, (max(nbytes, 16),), torch.uint8)


@writes("counter", "exp_avg", "exp_avg_sq", "stats")
def adam_onecycle_step_gpu(tensor_table, chunk_table, max_numel, rows, clip, eps, b2, zero_grads, counter, exp_avg, exp_avg_sq,
                           stats, ws=None):
    """tensor_table (T,4) int64 rows [param address, grad address or 0, numel, state offset]; chunk_table (C,2) int32 rows
    [tensor, first element]; rows (total_steps, 8) float32; counter (1) int64; exp_avg / exp_avg_sq: the flat float32 state;
    stats (8) float64. The parameters and gradients the table points at are written too: the caller moves their version
    counters (FusedAdamOneCycle.step does)."""
    if tensor_table.dim() != 2 or tensor_table.shape[1] != 4:
        raise RuntimeError("tensor_table must be (tensors, 4)")
    if chunk_table.dim() != 2 or chunk_table.shape[1] != 2:
        raise RuntimeError("chunk_table must be (chunks, 2)")
    if rows.dim() != 2 or rows.shape[1] != ROW or rows.shape[0] < 1:
        raise RuntimeError("rows must be (total_steps >= 1, %d)" % ROW)
    tensors, chunks, total_steps = tensor_table.shape[0], chunk_table.shape[0], rows.shape[0]
    pt, pc, pr = dev_ptr(tensor_table, "tensor_table", _L), dev_ptr(chunk_table, "chunk_table", _I), dev_ptr(rows, "rows", _F)
    pn, pm, pv = dev_ptr(counter, "counter", _L), dev_ptr(exp_avg, "exp_avg", _F), dev_ptr(exp_avg_sq, "exp_avg_sq", _F)
    ps = dev_ptr(stats, "stats", _D)
    need(counter, 1, "counter"); need(stats, STATS, "stats")
    if ws is None:
        ws = workspace(rows, chunks)
    pw = dev_ptr(ws, "workspace", torch.uint8)
    with on_device_of(rows) as s:
        _lib.check(_lib.lib().epnet_adam_onecycle_step(tensors, chunks, int(max_numel), pt, pc, pr, total_steps, float(clip), float(eps),
                                                       float(b2), int(bool(zero_grads)), pn, pm, pv, ps, pw, ws.numel(), s),
                   "adam_onecycle_step")
    return 1


@writes("counter", "exp_avg", "exp_avg_sq", "stats", "scale", "scaler_state")
def adam_onecycle_step_scaled_gpu(tensor_table, chunk_table, max_numel, rows, clip, eps, b2, zero_grads, counter, exp_avg, exp_avg_sq,
                                  stats, scale, scaler_state, growth_factor, backoff_factor, growth_interval, min_scale, ws=None):
    """``epnet_adam_onecycle_step_scaled``: the step above on gradients of ``loss * scale``, skipped when they are not finite.
    scale (1) float32; scaler_state (2) int64 [growth_tracker, skipped_total]; growth_interval 0 = a static scale. stats[6] is
    the scale the step used, stats[7] the steps skipped so far (SCALED_STATS_NAMES)."""
    if tensor_table.dim() != 2 or tensor_table.shape[1] != 4:
        raise RuntimeError("tensor_table must be (tensors, 4)")
    if chunk_table.dim() != 2 or chunk_table.shape[1] != 2:
        raise RuntimeError("chunk_table must be (chunks, 2)")
    if rows.dim() != 2 or rows.shape[1] != ROW or rows.shape[0] < 1:
        raise RuntimeError("rows must be (total_steps >= 1, %d)" % ROW)
    tensors, chunks, total_steps = tensor_table.shape[0], chunk_table.shape[0], rows.shape[0]
    pt, pc, pr = dev_ptr(tensor_table, "tensor_table", _L), dev_ptr(chunk_table, "chunk_table", _I), dev_ptr(rows, "rows", _F)
    pn, pm, pv = dev_ptr(counter, "counter", _L), dev_ptr(exp_avg, "exp_avg", _F), dev_ptr(exp_avg_sq, "exp_avg_sq", _F)
    ps, pk, pg = dev_ptr(stats, "stats", _D), dev_ptr(scale, "scale", _F), dev_ptr(scaler_state, "scaler_state", _L)
    need(counter, 1, "counter"); need(stats, STATS, "stats"); need(scale, 1, "scale"); need(scaler_state, 2, "scaler_state")
    if ws is None:
        ws = workspace(rows, chunks)
    pw = dev_ptr(ws, "workspace", torch.uint8)
    with on_device_of(rows) as s:
        _lib.check(_lib.lib().epnet_adam_onecycle_step_scaled(tensors, chunks, int(max_numel), pt, pc, pr, total_steps, float(clip),
                                                              float(eps), float(b2), int(bool(zero_grads)), pn, pm, pv, ps, pk, pg,
                                                              float(growth_factor), float(backoff_factor), int(growth_interval),
                                                              float(min_scale), pw, ws.numel(), s),
                   "adam_onecycle_step_scaled")
    return 1

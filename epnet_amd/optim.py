"""The reference's ``adam_onecycle`` training step as one fused, graph-capturable call.

The reference (tools/train_utils/train_utils.py:126-136) does four things per iteration: ``clip_grad_norm_`` (one ``.item()``
per parameter in the torch it pins), ``OneCycle.step(it)`` (learning_schedules_fastai.py:40-73: a new host-side ``lr`` and
``beta1``), the true-weight-decay loop of ``OptimWrapper.step`` (fastai_optim.py:132-149: one launch per tensor) and
``torch.optim.Adam.step``. ``FusedAdamOneCycle.step()`` is three launches of ``epnet_adam_onecycle_step``
(include/epnet_ops.h) with no host synchronisation and no host-side scalar: the step index lives in a device counter and
everything that depends on it in a row table uploaded once, so forward, backward and the step replay from one captured graph
with a new learning rate each time.

Differences from the reference, all stated in the header: Adam's bias corrections use the optimiser's one step counter (the
reference counts per parameter, which differs only for a parameter whose first gradient arrives late), and past ``total_steps``
the last row is used and ``stats`` flags it.
"""
import math

import numpy as np
import torch
from torch import nn

from . import _lib
from . import optim_cuda
from . import pointnet2_utils

_BN_TYPES = (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d)
_MAX_NUMEL = 2 ** 31 - 1


def one_cycle_table(total_steps, lr_max=0.002, moms=(0.95, 0.85), div_factor=10.0, pct_start=0.4):
    """float64 ``lr[t]`` and ``mom[t]``, t = 0 .. total_steps-1, as ``OneCycle.step(t)`` sets them: two half-cosine ramps that meet
    at ``border = int(total_steps * pct_start)``. Up to the border lr climbs from lr_max / div_factor to lr_max while the momentum
    falls from moms[0] to moms[1]; from the border on lr falls to lr_max / div_factor / 1e4 and the momentum climbs back. Evaluated
    scalar by scalar in the reference's order of operations, so the doubles are its doubles (tests/test_optim.py)."""
    total_steps = int(total_steps)
    border = int(total_steps * pct_start)
    if total_steps < 1 or not 0 < border < total_steps:
        raise ValueError("one_cycle_table: both phases need a step (total_steps %d, border %d)" % (total_steps, border))
    lr_low = lr_max / div_factor
    lr, mom = np.empty(total_steps, np.float64), np.empty(total_steps, np.float64)
    for t in range(total_steps):
        if t < border:
            ramp = np.cos(np.pi * (t / border)) + 1                         # 2 -> 0 over the phase
            lr_from, lr_to, mom_from, mom_to = lr_low, lr_max, moms[0], moms[1]
        else:
            ramp = np.cos(np.pi * ((t - border) / (total_steps - border))) + 1
            lr_from, lr_to, mom_from, mom_to = lr_max, lr_low / 1e4, moms[1], moms[0]
        lr[t] = lr_to + (lr_from - lr_to) / 2 * ramp
        mom[t] = mom_to + (mom_from - mom_to) / 2 * ramp
    return lr, mom


def schedule_rows(lr, mom, wd, beta2):
    """the (total_steps, 8) float32 row table of epnet_adam_onecycle_step: everything that depends on the step alone, in double,
    rounded once"""
    rows = np.zeros((len(lr), optim_cuda.ROW), np.float64)
    for t in range(len(lr)):
        l, b1 = float(lr[t]), float(mom[t])
        rows[t, :7] = (1 - wd * l, b1, 1 - b1, l / (1 - b1 ** (t + 1)), math.sqrt(1 - beta2 ** (t + 1)), l, b1)
    return rows.astype(np.float32)


def layer_groups(model):
    """the reference's two parameter groups (tools/train_rcnn.py:101-114 over fastai_optim.split_bn_bias): the model flattened to
    its leaf modules, group 0 the parameters of the leaves that are no BatchNorm, group 1 those of the BatchNorm leaves, each in
    module order without repeats, trainable ones only. As there, a parameter that a module WITH children holds directly is in no
    group."""
    groups = ([], [])
    seen = (set(), set())
    for leaf in model.modules():                       # depth first, in registration order: the flattened model's order
        if next(leaf.children(), None) is not None:
            continue
        which = 1 if isinstance(leaf, _BN_TYPES) else 0
        for p in leaf.parameters():
            if p.requires_grad and id(p) not in seen[which]:
                seen[which].add(id(p))
                groups[which].append(p)
    return groups


class FusedAdamOneCycle:
    """``OptimWrapper.create(partial(Adam, betas=(0.9, beta2)), ..., wd, true_wd=True, bn_wd=True)`` under ``OneCycle`` with
    ``clip_grad_norm_(parameters, grad_norm_clip)`` in front, the defaults being the yaml's. ``model_or_params``: a module (the
    reference's two groups, see layer_groups) or an iterable of parameters (all in group 0).

    ``step()`` takes the place of clip + scheduler step + optimizer step. A parameter whose ``requires_grad`` is False when it
    runs (RPN.FIXED, set after construction as the reference does) is skipped; one whose ``grad`` is None only decays. With
    ``zero_grads`` the kernel leaves every gradient zero, so the buffers persist, ``zero_grad()`` has nothing to do and
    backward accumulates into the same addresses -- what a graph capture needs.

    The device tables (where every parameter and gradient lives) are rebuilt only when an address, a ``requires_grad`` or the
    presence of a gradient changes: in practice once, at the first step. The rebuild copies two small tables to the device and
    is the only place that may synchronise; inside a graph capture it raises instead (run a step eagerly first).

    ``stats``: float64 (8) on the device -- total_norm, coef, lr, mom, the step used, 1 past ``total_steps`` -- as of the last
    step; read it whenever logging is due.

    ``loss_scale``: None (the default) is the plain step. ``"dynamic"`` is ``torch.amp.GradScaler``'s rule inside the same three
    launches (``epnet_adam_onecycle_step_scaled``): back-propagate ``opt.scale_loss(loss)``, and ``step()`` unscales the
    gradients as it reads them, skips the step when one of them is not finite (parameters, moments and the step counter stay,
    the gradients are still zeroed), multiplies the scale by ``backoff_factor`` (not below ``min_scale``) then, and by
    ``growth_factor`` after ``growth_interval`` applied steps in a row. A float is a static scale: it never moves, non-finite
    steps are still skipped; ``1.0`` is the guard for bfloat16 / float32 training. Nothing is read back: the scale (``opt.scale``),
    the growth tracker and the number of skipped steps live on the device, ``stats[6]`` is the scale the last step used and
    ``stats[7]`` the steps skipped so far. Parameters and gradients stay float32 (what ``torch.autocast`` gives); one scale
    serves all groups."""

    def __init__(self, model_or_params, total_steps, lr_max=0.002, moms=(0.95, 0.85), div_factor=10.0, pct_start=0.4, wd=0.001,
                 beta2=0.99, eps=1e-8, grad_norm_clip=1.0, zero_grads=True, loss_scale=None, init_scale=65536.0, growth_factor=2.0,
                 backoff_factor=0.5, growth_interval=2000, min_scale=1.0):
        if isinstance(model_or_params, nn.Module):
            groups = layer_groups(model_or_params)
        else:
            groups = ([p for p in model_or_params if p.requires_grad], [])
        self.groups = [list(g) for g in groups]
        self.params = self.groups[0] + self.groups[1]
        if not self.params:
            raise ValueError("FusedAdamOneCycle: no trainable parameter")
        if len({id(p) for p in self.params}) != len(self.params):
            raise ValueError("FusedAdamOneCycle: a parameter appears twice")
        self.device = self.params[0].device
        for p in self.params:
            if p.device != self.device:
                raise ValueError("FusedAdamOneCycle: parameters on %s and %s" % (self.device, p.device))
        self.total_steps, self.wd, self.beta2, self.eps = int(total_steps), float(wd), float(beta2), float(eps)
        self.grad_norm_clip, self.zero_grads = float(grad_norm_clip), bool(zero_grads)
        self.lr, self.mom = one_cycle_table(total_steps, lr_max, tuple(moms), div_factor, pct_start)
        self.rows = torch.from_numpy(schedule_rows(self.lr, self.mom, self.wd, self.beta2)).to(self.device)
        # state: two flat buffers, every tensor's piece starting at a multiple of 4 elements (16 bytes)
        self._offsets, total = [], 0
        for p in self.params:
            self._offsets.append(total)
            total += (p.numel() + 3) // 4 * 4
        like = self.params[0]
        self.exp_avg = pointnet2_utils._new(like, (max(total, 4),), torch.float32, zero=True)
        self.exp_avg_sq = pointnet2_utils._new(like, (max(total, 4),), torch.float32, zero=True)
        self._has_state = [False] * len(self.params)
        self.counter = torch.zeros((1,), dtype=torch.int64, device=self.device)
        self.stats = torch.zeros((optim_cuda.STATS,), dtype=torch.float64, device=self.device)
        self._signature = None
        self._tables = None
        self._init_scaler(loss_scale, init_scale, growth_factor, backoff_factor, growth_interval, min_scale)

    # ---- loss scaling -------------------------------------------------------------------------------------------------------
    def _init_scaler(self, loss_scale, init_scale, growth_factor, backoff_factor, growth_interval, min_scale):
        self.loss_scale = loss_scale
        self.scale = self.scaler_state = None
        if loss_scale is None:
            return
        if isinstance(loss_scale, str):
            if loss_scale != "dynamic":
                raise ValueError("FusedAdamOneCycle: loss_scale is None, \"dynamic\" or a number, got %r" % (loss_scale,))
            start, interval = float(init_scale), int(growth_interval)
            if interval < 1:
                raise ValueError("FusedAdamOneCycle: growth_interval must be at least 1 (got %r); a number as loss_scale is a "
                                 "static scale" % (growth_interval,))
        else:
            start, interval = float(loss_scale), 0
        growth_factor, backoff_factor, min_scale = float(growth_factor), float(backoff_factor), float(min_scale)
        fmax = float(np.finfo(np.float32).max)
        for name, value in (("growth_factor", growth_factor), ("backoff_factor", backoff_factor), ("min_scale", min_scale),
                            ("the scale", start)):
            if not 0 < value <= fmax:                   # also refuses NaN
                raise ValueError("FusedAdamOneCycle: %s must be positive and finite in float32, got %r" % (name, value))
        if growth_factor < 1:
            raise ValueError("FusedAdamOneCycle: growth_factor must be at least 1, got %r" % growth_factor)
        if backoff_factor > 1:
            raise ValueError("FusedAdamOneCycle: backoff_factor must be at most 1, got %r" % backoff_factor)
        if interval and start < min_scale:
            raise ValueError("FusedAdamOneCycle: init_scale %r is below min_scale %r" % (start, min_scale))
        self.growth_factor, self.backoff_factor, self.growth_interval, self.min_scale = growth_factor, backoff_factor, interval, min_scale
        self.scale = torch.full((1,), start, dtype=torch.float32, device=self.device)
        self.scaler_state = torch.zeros((2,), dtype=torch.int64, device=self.device)   # growth tracker, steps skipped

    def scale_loss(self, loss):
        """``loss * scale`` as one stock multiply by the device tensor: differentiable, capturable, nothing read back"""
        if self.scale is None:
            raise RuntimeError("FusedAdamOneCycle.scale_loss: this optimiser was built with loss_scale=None")
        return loss * self.scale

    def scaler_state_dict(self):
        """``torch.amp.GradScaler.state_dict()``'s keys plus ``skipped``; reads the device (synchronises)"""
        if self.scale is None:
            raise RuntimeError("FusedAdamOneCycle.scaler_state_dict: this optimiser was built with loss_scale=None")
        tracker, skipped = self.scaler_state.tolist()
        return {"scale": float(self.scale.item()), "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": int(tracker), "skipped": int(skipped)}

    def load_scaler_state_dict(self, state):
        """the scale and the growth tracker of ``scaler_state_dict()`` or of a ``GradScaler.state_dict()`` (``skipped`` is 0
        where missing). The factors and the interval stay the constructor's: whether the scale is static is not a checkpoint's
        to decide."""
        if self.scale is None:
            raise RuntimeError("FusedAdamOneCycle.load_scaler_state_dict: this optimiser was built with loss_scale=None")
        scale = float(state["scale"])
        if not 0 < scale <= float(np.finfo(np.float32).max):
            raise ValueError("load_scaler_state_dict: scale %r" % scale)
        self.scale.fill_(scale)
        self.scaler_state.copy_(torch.tensor([int(state.get("_growth_tracker", 0)), int(state.get("skipped", 0))], dtype=torch.int64))

    # ---- the tables ---------------------------------------------------------------------------------------------------------
    def _current_signature(self):
        sig = []
        for p in self.params:
            if not p.requires_grad:
                sig.append(None)
                continue
            g = p.grad
            sig.append((p.data_ptr(), None if g is None else g.data_ptr()))
        return sig

    def _check(self, t, what):
        if t.dtype != torch.float32 or t.layout != torch.strided or not t.is_contiguous() or t.device != self.device:
            raise RuntimeError("FusedAdamOneCycle: %s must be a contiguous float32 tensor on %s (got %s, %s, %s)"
                               % (what, self.device, t.dtype, t.layout, t.device))

    def _rebuild(self, sig):
        if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FusedAdamOneCycle: a parameter's or gradient's address, requires_grad or the presence of a gradient "
                               "changed inside a graph capture; run one step eagerly before capturing")
        table, live, stepped = [], [], []
        for i, (p, s) in enumerate(zip(self.params, sig)):
            if s is None or p.numel() == 0:
                continue
            self._check(p, "parameter %d" % i)
            g = p.grad
            if g is not None:
                self._check(g, "the gradient of parameter %d" % i)
                if g.numel() != p.numel():
                    raise RuntimeError("FusedAdamOneCycle: the gradient of parameter %d has another size" % i)
                stepped.append(i)
                live.append(g)
            table.append((s[0], s[1] or 0, p.numel(), self._offsets[i]))
            live.append(p)
        max_numel = max((row[2] for row in table), default=0)
        if max_numel > _MAX_NUMEL:
            _lib.check(-4, "adam_onecycle_step (a tensor of %d elements)" % max_numel)
        tt = np.array(table, np.int64).reshape(-1, 4)
        firsts = [np.arange(0, row[2], optim_cuda.CHUNK, dtype=np.int32) for row in table]
        ct = np.empty((sum(len(f) for f in firsts), 2), np.int32)
        at = 0
        for k, f in enumerate(firsts):
            ct[at:at + len(f), 0], ct[at:at + len(f), 1] = k, f
            at += len(f)
        ws = optim_cuda.workspace(self.rows, len(ct))
        self._tables = (torch.from_numpy(tt).to(self.device), torch.from_numpy(ct).to(self.device), max_numel, ws, tuple(live), tuple(stepped))
        self._signature = sig

    # ---- the optimiser's surface --------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self):
        sig = self._current_signature()
        if sig != self._signature:
            self._rebuild(sig)
        tt, ct, max_numel, ws, live, stepped = self._tables
        if tt.shape[0] == 0:
            return
        if self.scale is None:
            optim_cuda.adam_onecycle_step_gpu(tt, ct, max_numel, self.rows, self.grad_norm_clip, self.eps, self.beta2, self.zero_grads,
                                              self.counter, self.exp_avg, self.exp_avg_sq, self.stats, ws)
        else:
            optim_cuda.adam_onecycle_step_scaled_gpu(tt, ct, max_numel, self.rows, self.grad_norm_clip, self.eps, self.beta2,
                                                     self.zero_grads, self.counter, self.exp_avg, self.exp_avg_sq, self.stats,
                                                     self.scale, self.scaler_state, self.growth_factor, self.backoff_factor,
                                                     self.growth_interval, self.min_scale, ws)
        for i in stepped:                  # these now have moments (only once the launch went through)
            self._has_state[i] = True
        torch._C._increment_version(live)  # the kernels wrote the parameters (and zeroed the gradients) through raw pointers

    def zero_grad(self):
        """nothing to do once ``zero_grads`` holds the buffers at zero; otherwise zeroes them in place (addresses stay)"""
        if self.zero_grads:
            return
        for p in self.params:
            if p.grad is not None:
                p.grad.detach_()
                p.grad.zero_()

    def _piece(self, buf, i):
        p = self.params[i]
        return buf[self._offsets[i]:self._offsets[i] + p.numel()].view(p.shape)

    def state_dict(self):
        """``torch.optim.Adam.state_dict()``'s format with the reference wrapper's two groups (layer_groups), so that a reference
        checkpoint's ``optimizer_state`` and this one are interchangeable. Reads the device counter (synchronises)."""
        step = int(self.counter.item())
        at = min(max(step - 1, 0), self.total_steps - 1)
        state = {}
        for i in range(len(self.params)):
            if self._has_state[i] and step > 0:        # step 0 with state: every step so far was skipped (loss scaling)
                state[i] ={"step": torch.tensor(float(step)), "exp_avg": self._piece(self.exp_avg, i).clone(),
                            "exp_avg_sq": self._piece(self.exp_avg_sq, i).clone()}
        groups, first = [], 0
        for g in self.groups:
            groups.append({"lr": float(self.lr[at]), "betas": (float(self.mom[at]), self.beta2), "eps": self.eps, "weight_decay": 0,
                           "amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False,
                           "fused": None, "params": list(range(first, first + len(g)))})
            first += len(g)
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, state_dict):
        """moments and step count from a state dict of this class or of the reference's wrapper over the same model; the groups'
        hyper-parameters are the schedule's and are not read. Lossy in one respect: torch keeps a ``step`` per parameter, this
        class one counter, so a checkpoint whose parameters have DIFFERENT step counts (a parameter whose first gradient came
        late) is loaded with the largest of them for all, and saved again that way."""
        groups = state_dict["param_groups"]
        if [len(g["params"]) for g in groups] != [len(g) for g in self.groups]:
            raise ValueError("load_state_dict: groups of %s parameters, this optimiser has %s"
                             % ([len(g["params"]) for g in groups], [len(g) for g in self.groups]))
        order = [k for g in groups for k in g["params"]]
        steps = []
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        self._has_state = [False] * len(self.params)
        for i, key in enumerate(order):
            s = state_dict["state"].get(key)
            if s is None:
                continue
            p = self.params[i]
            if tuple(s["exp_avg"].shape) != tuple(p.shape):
                raise ValueError("load_state_dict: parameter %d is %s, its state %s" % (i, tuple(p.shape), tuple(s["exp_avg"].shape)))
            self._piece(self.exp_avg, i).copy_(s["exp_avg"])
            self._piece(self.exp_avg_sq, i).copy_(s["exp_avg_sq"])
            self._has_state[i] = True
            steps.append(int(float(s["step"])))
        self.counter.fill_(max(steps, default=0))
        self._signature = None

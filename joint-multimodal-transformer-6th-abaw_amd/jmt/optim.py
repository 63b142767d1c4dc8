"""Fused SGD and Adam over flat buffers (instantiator.py:32-46 semantics, config_file.json:73-82).

All trainable parameters are re-homed into ONE flat fp32 buffer, their gradients into another
(the buffer the RCCL all-reduce runs on), the momentum (Adam: both moments) into further ones;
one jmt_sgd_step / jmt_adam_step launch updates everything and rewrites the bf16/f16 compute
shadows of the weights in the same pass.  With the device state block (FusedSGD(device_lr=True),
FusedAdam) the learning rate is read on the device, so a captured step follows a schedule.
Parameters that never receive a gradient (the reference's unused `final_encoder`,
`gated_attention`) must not be passed: torch.optim.SGD skips them because their .grad is None,
so `used_parameters()` finds them with one probe backward."""
from __future__ import annotations

import math
import os
from typing import Iterable, List, Optional, Tuple

import torch

from . import _lib
from . import functional as F
from . import ops


def _bump_grad_gen(_p):
    F._grad_gen[0] += 1


def _state_block(lr: float, dev) -> torch.Tensor:
    """The device optimizer state of include/jmt.h: fp32[8] = lr, step, step_size, bc2_sqrt,
    clip coefficient, gradient norm, max_norm, 1 reserved."""
    return torch.tensor([lr, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float32, device=dev)


def _check_max_grad_norm(kind: str, max_grad_norm) -> Optional[float]:
    """None (no clipping), or the threshold as a float: > 0, float("inf") allowed (measure only)."""
    if max_grad_norm is None:
        return None
    x = float(max_grad_norm)
    if math.isnan(x) or x <= 0.0:
        raise ValueError(f"{kind}: max_grad_norm must be > 0 (float('inf') measures without "
                         f"clipping) or None, not {max_grad_norm!r}")
    return x


class _FlatOptimizer:
    """The flat-buffer layout the fused optimizers share: every parameter re-homed into one fp32
    buffer (each starting on a 64-element boundary, the padding zero), its .grad into a second,
    the 16-bit compute shadows into a third; the gradient-write bookkeeping behind
    fuse_zero_grad; the optional device state block (`state`) with set_lr / get_lr.

    fuse_zero_grad: the step kernel zeroes each gradient after reading it and the next
    zero_grad() issues nothing while no gradient has been written since — the training step of
    train.py:96-315 without a fill launch.  Off by default: torch's optimizer.step() leaves .grad
    readable until zero_grad().

    Contract of the skipped fill: "written since" is known from functional._grad_gen, which the
    HIP gradient writers (functional._grad_buffer) and torch autograd's accumulation into .grad
    (post-accumulate hooks) bump.  Anything else that writes into a .grad in place
    (p.grad.add_/copy_ by hand, a helper writing into the flat views) is invisible to it and the
    next backward would add onto the stale values: call zero_grad(force=True) after such a
    write, or set JMT_CHECK_ZERO_GRAD=1 to have every skipped fill verify (one reduction + host
    sync) that the gradients are in fact zero.

    max_grad_norm (FusedSGD(device_lr=True), FusedAdam): torch.nn.utils.clip_grad_norm_ (L2)
    folded into the step.  jmt_grad_norm (a read-only pass over the gradient buffer and a
    one-block fold, no floating-point atomics: bitwise reproducible) leaves the norm of the
    unscaled gradient, the coefficient min(1, max_norm / (norm + 1e-6)) and the per-parameter
    norms on the device, and the step kernel multiplies every gradient by the coefficient as it
    reads it (the *_clip entry points).  Nothing is read on the host and the step still captures
    into a hipGraph; set_max_grad_norm() is legal between replays, grad_norm() / clip_coef() /
    grad_norms() return device tensors.  None launches nothing and steps through the entry points
    without clipping."""

    state: Optional[torch.Tensor] = None
    max_grad_norm: Optional[float] = None
    _BUFFERS: tuple = ()          # names of the per-element state buffers (state_dict)

    def _init_flat(self, params: Iterable[torch.nn.Parameter], lr: float,
                   shadow_dtype: Optional[torch.dtype], fuse_zero_grad: bool):
        self.params: List[torch.nn.Parameter] = list(params)
        assert self.params, "no parameters"
        dev = self.params[0].device
        # every parameter starts on a 256-B boundary (16-B aligned MFMA operand loads)
        offs = []
        n = 0
        for p in self.params:
            offs.append(n)
            n += -(-p.numel() // 64) * 64
        self.numel = n
        self.lr = lr
        self.flat_p = torch.empty(n, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(n, dtype=torch.float32, device=dev)
        self.shadow = (torch.empty(n, dtype=shadow_dtype, device=dev)
                       if shadow_dtype not in (None, torch.float32) else None)
        self.flat_p.zero_()
        self.offsets = offs
        self._gviews = []
        with torch.no_grad():
            for p, off in zip(self.params, offs):
                k = p.numel()
                self.flat_p[off:off + k].copy_(p.detach().reshape(-1))
                p.data = self.flat_p[off:off + k].view_as(p)
                g = self.flat_g[off:off + k].view_as(p)
                p.grad = g
                self._gviews.append(g)
        if self.shadow is not None:
            ops.cast(self.flat_p, self.shadow.dtype, out=self.shadow)
        for p, off in zip(self.params, offs):
            F.register_shadow(p, self.shadow[off:off + p.numel()].view_as(p)
                              if self.shadow is not None else None)
        self.fuse_zero_grad = bool(fuse_zero_grad)
        # the gradients are known to be zero while nothing has written one since the last fill /
        # zeroing step (functional._grad_gen counts the HIP writers; torch autograd accumulation
        # into .grad is caught by the post-accumulate hooks)
        self._clean_gen = F._grad_gen[0]
        self._hooks = [p.register_post_accumulate_grad_hook(_bump_grad_gen) for p in self.params]

    def close(self):
        """Remove the gradient-write hooks this optimizer put on its parameters (also on garbage
        collection); the parameters keep their flat-buffer storage."""
        for h in getattr(self, "_hooks", ()):
            h.remove()
        self._hooks = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def zero_grad(self, set_to_none: bool = False, force: bool = False):
        """optimizer.zero_grad().  With fuse_zero_grad the step kernel already zeroed the
        gradients, so after a step (and no gradient write since) this issues nothing; force=True
        fills regardless (after an in-place .grad write the write counter cannot see)."""
        for p, g in zip(self.params, self._gviews):
            if p.grad is None or p.grad.data_ptr() != g.data_ptr():
                p.grad = g
                self._clean_gen = None
        if force or not self.fuse_zero_grad or self._clean_gen != F._grad_gen[0]:
            self.flat_g.zero_()
            self._clean_gen = F._grad_gen[0]
        elif os.environ.get("JMT_CHECK_ZERO_GRAD", "0") == "1":
            nz = int(torch.count_nonzero(self.flat_g))
            if nz:
                raise RuntimeError(f"{type(self).__name__}.zero_grad: {nz} gradient element(s) "
                                   "written outside the tracked writers since the fused zeroing "
                                   "step (see the fuse_zero_grad contract); call "
                                   "zero_grad(force=True)")

    def set_lr(self, lr: float):
        """Set the learning rate.  With the device state block this is a stream-ordered fill of
        state[0]: no host synchronisation, legal between replays of a captured step, and the
        replays that follow use the new value.  Without it (FusedSGD(device_lr=False)) only the
        host value changes: the lr is a kernel argument, so a graph captured earlier does NOT
        see it and keeps stepping at the lr it was captured with."""
        self.lr = float(lr)
        if self.state is not None:
            self.state[0:1].fill_(self.lr)

    def get_lr(self) -> float:
        """The learning rate last set (the host's copy: nothing is read from the device)."""
        return self.lr

    # ---------------------------------------------------------------- gradient-norm clipping
    def _init_clip(self, max_grad_norm: Optional[float]):
        """After the state block exists.  The segment table is the parameters' offsets: segment
        i = parameter i and the zero padding behind it."""
        self.max_grad_norm = max_grad_norm
        if max_grad_norm is None:
            return
        dev = self.flat_p.device
        self.state[6:7].fill_(max_grad_norm)
        self._seg_off = torch.tensor(self.offsets + [self.numel], dtype=torch.int64, device=dev)
        self._seg_norm = torch.zeros(len(self.params), dtype=torch.float32, device=dev)
        nbytes = int(_lib.load().jmt_grad_norm_scratch(self.numel, len(self.params)))
        if nbytes < 0:
            raise _lib.JMTError(f"jmt_grad_norm_scratch refuses {self.numel} elements in "
                                f"{len(self.params)} segments")
        self._norm_scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)

    def _grad_norm(self, grad_scale: float, amp_state: Optional[torch.Tensor]):
        """The norm launches of a clipped step: state[4] / state[5] and the per-parameter norms."""
        launch = lambda: _lib.call(
            "jmt_grad_norm", self.numel, self.flat_g.data_ptr(), self.state.data_ptr(),
            self._norm_scratch.data_ptr(), self._norm_scratch.numel() * 8,
            self._seg_off.data_ptr(), len(self.params), self._seg_norm.data_ptr(), grad_scale,
            self._ptr(amp_state), ops.stream())
        ops._hooked({"family": "grad_norm", "flops": 0.0, "bytes": 4.0 * self.numel}, launch)

    def _clipping(self) -> None:
        if self.max_grad_norm is None:
            raise RuntimeError(f"{type(self).__name__}: built without max_grad_norm (pass "
                               "float('inf') to measure the norm without clipping)")

    def set_max_grad_norm(self, max_grad_norm: float):
        """Set the clipping threshold: a stream-ordered fill of state[6], as set_lr is for
        state[0] (no host synchronisation, legal between replays of a captured step)."""
        self._clipping()
        self.max_grad_norm = _check_max_grad_norm(type(self).__name__, float(max_grad_norm))
        self.state[6:7].fill_(self.max_grad_norm)

    def grad_norm(self) -> torch.Tensor:
        """The last step's L2 norm of the unscaled gradient before clipping: a 0-dim view of the
        device state block (no synchronisation; read it when it is needed, e.g. once per epoch)."""
        self._clipping()
        return self.state[5]

    def clip_coef(self) -> torch.Tensor:
        """The last step's coefficient min(1, max_norm / (norm + 1e-6)), a 0-dim device view."""
        self._clipping()
        return self.state[4]

    def grad_norms(self) -> torch.Tensor:
        """The last step's per-parameter norms of the unscaled gradient, (len(params),) fp32 on
        the device, in `params` order."""
        self._clipping()
        return self._seg_norm

    def _ptr(self, t: Optional[torch.Tensor]):
        return t.data_ptr() if t is not None else None

    def _shadow_dt(self) -> int:
        return ops.dt(self.shadow) if self.shadow is not None else _lib.BF16

    def _step_bytes(self, arrays: int) -> float:
        """A step launch's traffic for the launch hook: `arrays` fp32 buffers read and written
        (the gradient written only with fuse_zero_grad) and the shadow written."""
        rw = 2 * arrays - (0 if self.fuse_zero_grad else 1)
        return float(self.numel) * (4 * rw + (2 if self.shadow is not None else 0))

    # ---------------------------------------------------------------- resume
    def _host_state(self) -> dict:
        return {}

    def _load_host_state(self, sd: dict):
        pass

    def state_dict(self) -> dict:
        """A flat dict: copies of the parameter buffer, the per-element state buffers and the
        device state block, plus the host-side scalars."""
        sd = {"kind": type(self).__name__, "numel": self.numel, "lr": self.lr,
              "flat_p": self.flat_p.clone(),
              "state": self.state.clone() if self.state is not None else None}
        for name in self._BUFFERS:
            t = getattr(self, name)
            sd[name] = t.clone() if t is not None else None
        sd.update(self._host_state())
        return sd

    @torch.no_grad()
    def load_state_dict(self, sd: dict):
        """Copy a state_dict() into this optimizer's own buffers (their addresses, and so a
        captured graph, stay valid) and rewrite the compute shadows."""
        if sd.get("kind") != type(self).__name__ or sd.get("numel") != self.numel:
            raise ValueError(f"{type(self).__name__}.load_state_dict: state of "
                             f"{sd.get('kind')} with {sd.get('numel')} elements does not fit "
                             f"{self.numel}")
        for name in self._BUFFERS + ("state",):
            mine, theirs = getattr(self, name), sd.get(name)
            if (mine is None) != (theirs is None):
                raise ValueError(f"{type(self).__name__}.load_state_dict: buffer {name!r} is "
                                 "present on one side only")
            if mine is not None:
                mine.copy_(theirs)
        if self.max_grad_norm is not None:        # this optimizer's threshold, not the file's
            self.state[6:7].fill_(self.max_grad_norm)
        self.flat_p.copy_(sd["flat_p"])
        if self.shadow is not None:
            ops.cast(self.flat_p, self.shadow.dtype, out=self.shadow)
        self.lr = float(sd["lr"])
        self._load_host_state(sd)


class FusedSGD(_FlatOptimizer):
    _BUFFERS = ("buf",)

    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float, momentum: float = 0.0,
                 dampening: float = 0.0, weight_decay: float = 0.0, nesterov: bool = False,
                 shadow_dtype: Optional[torch.dtype] = None, fuse_zero_grad: bool = False,
                 device_lr: bool = False, max_grad_norm: Optional[float] = None):
        """fuse_zero_grad, max_grad_norm: see _FlatOptimizer (jmt_sgd_step_zero; clipping needs
        device_lr=True, the coefficient lives in the device state block).

        device_lr: the learning rate lives in the device state block and the step goes through
        jmt_sgd_step_dev, so set_lr() (an lr scheduler) takes effect inside a captured graph.
        Off by default: the lr is then a kernel argument, fixed at capture."""
        max_grad_norm = _check_max_grad_norm("FusedSGD", max_grad_norm)
        if max_grad_norm is not None and not device_lr:
            raise ValueError("FusedSGD: max_grad_norm needs device_lr=True (the clip coefficient "
                             "is read from the device state block)")
        self._init_flat(params, lr, shadow_dtype, fuse_zero_grad)
        self.momentum, self.dampening = momentum, dampening
        self.weight_decay, self.nesterov = weight_decay, nesterov
        dev = self.flat_p.device
        self.buf = torch.zeros(self.numel, dtype=torch.float32, device=dev) if momentum else None
        self.state = _state_block(lr, dev) if device_lr else None
        self._init_clip(max_grad_norm)
        self.first = True

    def _host_state(self) -> dict:
        return {"first": self.first, "amp": getattr(self, "_amp", False)}

    def _load_host_state(self, sd: dict):
        self.first = bool(sd["first"])
        self._amp = bool(sd["amp"])

    def _step_dev(self, grad_scale: float, amp_state: Optional[torch.Tensor]):
        clip = self.max_grad_norm is not None
        if clip:
            self._grad_norm(grad_scale, amp_state)
        fn = "jmt_sgd_step_dev_clip" if clip else "jmt_sgd_step_dev"
        launch = lambda: _lib.call(
            fn, self.numel, self.flat_p.data_ptr(), self.flat_g.data_ptr(), self._ptr(self.buf),
            self.state.data_ptr(), self.momentum, self.dampening, self.weight_decay,
            int(self.nesterov), int(self.first), grad_scale, self._ptr(amp_state),
            int(self.fuse_zero_grad), self._ptr(self.shadow), self._shadow_dt(), ops.stream())
        ops._hooked({"family": fn[4:], "flops": 0.0, "bytes": self._step_bytes(3)}, launch)

    @torch.no_grad()
    def step_amp(self, amp_state: torch.Tensor):
        """One step driven by a GradScaler's device state (unscale, skip on overflow).  Whether
        the momentum buffer is initialised is then decided on the device (steps_taken), so plain
        step() calls cannot follow scaled ones."""
        self._amp = True
        if self.state is not None:
            self._step_dev(1.0, amp_state)
            self._clean_gen = F._grad_gen[0]
            return
        fn = "jmt_sgd_step_amp_zero" if self.fuse_zero_grad else "jmt_sgd_step_amp"
        _lib.call(fn, self.numel, self.flat_p.data_ptr(), self.flat_g.data_ptr(),
                  self.buf.data_ptr() if self.buf is not None else None, self.lr, self.momentum,
                  self.dampening, self.weight_decay, int(self.nesterov), int(self.first),
                  amp_state.data_ptr(),
                  self.shadow.data_ptr() if self.shadow is not None else None,
                  ops.dt(self.shadow) if self.shadow is not None else 1, ops.stream())
        self._clean_gen = F._grad_gen[0]

    @torch.no_grad()
    def step(self, grad_scale: float = 1.0):
        if getattr(self, "_amp", False):
            raise RuntimeError("FusedSGD: step() after GradScaler steps (first-step state is on "
                               "the device); keep using scaler.step(opt)")
        if self.state is not None:
            self._step_dev(grad_scale, None)
        else:
            ops.sgd_step(self.flat_p, self.flat_g, self.buf, self.lr, self.momentum,
                         self.dampening, self.weight_decay, self.nesterov, self.first, grad_scale,
                         self.shadow, zero_grad=self.fuse_zero_grad)
        self.first = False
        self._clean_gen = F._grad_gen[0]


class FusedAdam(_FlatOptimizer):
    """torch.optim.Adam (L2 weight decay; amsgrad optional) over the flat buffers, as
    instantiator.py:40-46 configures it.  The lr, the step count and both bias corrections live
    in the device state block: a step is two launches (jmt_opt_tick, jmt_adam_step), reads
    nothing from the device on the host, and captures into a hipGraph that follows set_lr()."""

    _BUFFERS = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")

    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float,
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, amsgrad: bool = False,
                 shadow_dtype: Optional[torch.dtype] = None, fuse_zero_grad: bool = False,
                 max_grad_norm: Optional[float] = None):
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"FusedAdam: betas {betas} must be in [0, 1)")
        max_grad_norm = _check_max_grad_norm("FusedAdam", max_grad_norm)
        self._init_flat(params, lr, shadow_dtype, fuse_zero_grad)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), eps
        self.weight_decay, self.amsgrad = weight_decay, bool(amsgrad)
        dev = self.flat_p.device
        self.exp_avg = torch.zeros(self.numel, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(self.numel, dtype=torch.float32, device=dev)
        self.max_exp_avg_sq = (torch.zeros(self.numel, dtype=torch.float32, device=dev)
                               if self.amsgrad else None)
        self.state = _state_block(lr, dev)
        self._init_clip(max_grad_norm)

    def _step(self, grad_scale: float, amp_state: Optional[torch.Tensor]):
        st, amp, s = self.state.data_ptr(), self._ptr(amp_state), ops.stream()
        clip = self.max_grad_norm is not None
        ops._hooked({"family": "opt_tick", "flops": 0.0, "bytes": 32.0}, lambda: _lib.call(
            "jmt_opt_tick", st, self.betas[0], self.betas[1], amp, s))
        if clip:
            self._grad_norm(grad_scale, amp_state)
        fn = "jmt_adam_step_clip" if clip else "jmt_adam_step"
        launch = lambda: _lib.call(
            fn, self.numel, self.flat_p.data_ptr(), self.flat_g.data_ptr(),
            self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self._ptr(self.max_exp_avg_sq),
            st, self.betas[0], self.betas[1], self.eps, self.weight_decay, grad_scale, amp,
            int(self.fuse_zero_grad), self._ptr(self.shadow), self._shadow_dt(), s)
        ops._hooked({"family": fn[4:], "flops": 0.0,
                     "bytes": self._step_bytes(5 if self.amsgrad else 4)}, launch)
        self._clean_gen = F._grad_gen[0]

    @torch.no_grad()
    def step_amp(self, amp_state: torch.Tensor):
        """One step driven by a GradScaler's device state: unscale by amp[1]; on found_inf
        neither the step count nor any buffer changes."""
        self._step(1.0, amp_state)

    @torch.no_grad()
    def step(self, grad_scale: float = 1.0):
        self._step(grad_scale, None)


class GradScaler:
    """torch.cuda.amp.GradScaler semantics (train.py:89,314-316) for FusedSGD / FusedAdam with the
    whole state on the device: `scaler.scale(loss).backward(); scaler.step(opt);
    scaler.update()` issue kernels only (no host synchronisation; the step stays capturable into
    a hipGraph)."""

    def __init__(self, init_scale: float = 2.0 ** 16, growth_factor: float = 2.0,
                 backoff_factor: float = 0.5, growth_interval: int = 2000, device=None):
        dev = torch.device(device) if device is not None else torch.device("cuda")
        self.growth_factor, self.backoff_factor = growth_factor, backoff_factor
        self.growth_interval = growth_interval
        self.state = torch.tensor([init_scale, 1.0 / init_scale, 0.0, 0.0, 0.0],
                                  dtype=torch.float32, device=dev)

    def scale(self, loss: torch.Tensor) -> torch.Tensor:
        return loss * self.state[0]

    def step(self, opt: "_FlatOptimizer"):
        _lib.call("jmt_amp_check", opt.numel, opt.flat_g.data_ptr(), self.state.data_ptr(),
                  ops.stream())
        opt.step_amp(self.state)

    def update(self):
        _lib.call("jmt_amp_update", self.state.data_ptr(), self.growth_factor,
                  self.backoff_factor, self.growth_interval, ops.stream())

    def get_scale(self) -> float:
        return float(self.state[0])


def used_parameters(model_fn, params: Iterable[torch.nn.Parameter]):
    """Run `model_fn()` (forward + backward), return the parameters that received a gradient."""
    params = list(params)
    for p in params:
        p.grad = None
    model_fn()
    used = [p for p in params if p.grad is not None]
    for p in params:
        p.grad = None
    return used

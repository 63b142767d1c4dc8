"""Learning-rate schedules of the reference's optimizer factory (instantiator.py:52-105), host
only: each step() computes the epoch's lr in Python floats from a closed form and hands it to
`opt.set_lr`.  With the device state block (jmt.optim.FusedAdam, FusedSGD(device_lr=True)) that
is one stream-ordered 4-byte fill, so a captured training step follows the schedule between
replays without re-capture.

    step       StepLR             base * gamma ** (epoch // step_size)
    mystep     MyStepLR           max(StepLR, min_lr)
    cosine     CosineAnnealingLR  eta_min + (base - eta_min) (1 + cos(pi epoch / T_max)) / 2
    mycosine   MyCosineLR         max(base * coef * (1 + cos((epoch - 1) pi / max_epochs)), min_lr)
    multistep  MultiStepLR        base * gamma ** (number of milestones <= epoch)

As with torch's schedulers, construction performs the initial step (epoch 0) and step() is
called once per epoch after the epoch's optimizer steps.  `opt` is anything with get_lr() and
set_lr(lr)."""
from __future__ import annotations

import bisect
import math
from typing import Iterable, List


class LRScheduler:
    """Shared base: base_lr is the optimizer's lr at construction, last_epoch the epoch whose lr
    is in force.  Subclasses give lr_at(epoch)."""

    def __init__(self, opt, last_epoch: int = -1):
        self.opt = opt
        self.base_lr = float(opt.get_lr())
        self.last_epoch = int(last_epoch)
        self._last_lr = self.base_lr
        self.step()

    def lr_at(self, epoch: int) -> float:
        raise NotImplementedError

    def step(self):
        self.last_epoch += 1
        self._last_lr = float(self.lr_at(self.last_epoch))
        self.opt.set_lr(self._last_lr)

    def get_last_lr(self) -> List[float]:
        return [self._last_lr]

    def state_dict(self) -> dict:
        return {k: v for k, v in self.__dict__.items() if k != "opt"}

    def load_state_dict(self, sd: dict):
        """Resume: restore the schedule's position and put its lr back into the optimizer."""
        self.__dict__.update(sd)
        self.opt.set_lr(self._last_lr)


class StepLR(LRScheduler):
    def __init__(self, opt, step_size: int, gamma: float = 0.1, last_epoch: int = -1):
        if int(step_size) < 1:
            raise ValueError(f"step_size must be >= 1, got {step_size}")
        self.step_size, self.gamma = int(step_size), float(gamma)
        super().__init__(opt, last_epoch)

    def lr_at(self, epoch: int) -> float:
        return self.base_lr * self.gamma ** (epoch // self.step_size)


class MyStepLR(StepLR):
    """StepLR that never goes below min_lr."""

    def __init__(self, opt, step_size: int, gamma: float = 0.1, last_epoch: int = -1,
                 min_lr: float = 1e-6):
        self.min_lr = float(min_lr)
        super().__init__(opt, step_size, gamma, last_epoch)

    def lr_at(self, epoch: int) -> float:
        return max(super().lr_at(epoch), self.min_lr)


class CosineAnnealingLR(LRScheduler):
    def __init__(self, opt, T_max: int, eta_min: float = 0.0, last_epoch: int = -1):
        if T_max <= 0:
            raise ValueError(f"T_max must be > 0, got {T_max}")
        self.T_max, self.eta_min = T_max, float(eta_min)
        super().__init__(opt, last_epoch)

    def lr_at(self, epoch: int) -> float:
        return self.eta_min + (self.base_lr - self.eta_min) * \
            (1.0 + math.cos(math.pi * epoch / self.T_max)) / 2.0


class MyCosineLR(LRScheduler):
    """Cosine evolution shifted by one epoch (it already moves the lr at epoch 0), clamped at
    min_lr."""

    def __init__(self, opt, coef: float, max_epochs: int, min_lr: float = 1e-9,
                 last_epoch: int = -1):
        if not isinstance(coef, float) or coef <= 0.0:
            raise ValueError(f"coef must be a float > 0, got {coef!r}")
        if max_epochs <= 0:
            raise ValueError(f"max_epochs must be > 0, got {max_epochs}")
        self.coef, self.max_epochs, self.min_lr = coef, float(max_epochs), float(min_lr)
        super().__init__(opt, last_epoch)

    def lr_at(self, epoch: int) -> float:
        return max(self.base_lr * self.coef *
                   (1.0 + math.cos((epoch - 1) * math.pi / self.max_epochs)), self.min_lr)


class MultiStepLR(LRScheduler):
    def __init__(self, opt, milestones: Iterable[int], gamma: float = 0.1, last_epoch: int = -1):
        self.milestones, self.gamma = sorted(int(m) for m in milestones), float(gamma)
        super().__init__(opt, last_epoch)

    def lr_at(self, epoch: int) -> float:
        return self.base_lr * self.gamma ** bisect.bisect_right(self.milestones, epoch)

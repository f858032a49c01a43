"""The learning-rate schedule of the retrieval model's training loop (reference train_decoder.py:151, 205:
`InverseSquareRootScheduler(optimizer, warmup_steps=10000)`, stepped once after every `optimizer.step()`).

The optimizer step number t (1, 2, ...) runs at

    lr(t) = base_lr                                  for t <= warmup_steps
    lr(t) = base_lr * sqrt(warmup_steps) / sqrt(t)   after that

where t = last_epoch + 1: the constructor leaves last_epoch at 0, every step() adds one.  Constructor, attribute names and
state dict are the reference's (`warmup_steps` next to what `LRScheduler` keeps), so the "scheduler" entry of a checkpoint
loads in either direction.

On any optimizer this is a host-side scheduler: step() writes `group["lr"]`.

On a `rqhip.optim.FlatAdamW` it also attaches the schedule to the optimizer, whose kernel (csrc/adamw.hip) then forms the
learning rate itself from a device counter `lr_step` that it advances with every optimizer step -- the part a captured
hipGraph needs, because a learning rate passed as a kernel argument replays the value of the capture.  The constructor and
load_state_dict() FILL that counter with last_epoch + 1 (no read-back); step() stays host-only and keeps `group["lr"]` as
the mirror for logging.

CONTRACT on a FlatAdamW: one scheduler.step() per optimizer.step(), a graph replay counting as an optimizer step -- the
reference's loop.  Then lr_step == last_epoch + 1 before every optimizer step, and the device's learning rate is the
mirror's (to the rounding of fp32).  A loop that steps the scheduler more or less often drifts from its mirror: the device
counter follows the optimizer steps.
"""
from torch.optim import Optimizer
from torch.optim.lr_scheduler import LRScheduler


class InverseSquareRootScheduler(LRScheduler):
    def __init__(self, optimizer: Optimizer, warmup_steps: int, last_epoch: int = -1):
        self.warmup_steps = warmup_steps
        super().__init__(optimizer, last_epoch)
        self._attach_device_schedule()

    def get_lr(self):
        t = self.last_epoch + 1
        if t <= self.warmup_steps:
            return list(self.base_lrs)
        decay = self.warmup_steps ** 0.5 / t ** 0.5
        return [base_lr * decay for base_lr in self.base_lrs]

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        self._attach_device_schedule()

    def _attach_device_schedule(self) -> None:
        """(nothing is kept on self: the state dict stays the reference's key set)"""
        attach = getattr(self.optimizer, "attach_schedule", None)
        if attach is not None:
            for gi in range(len(self.optimizer.param_groups)):
                attach(gi, self.warmup_steps, self.last_epoch + 1, self.base_lrs[gi])

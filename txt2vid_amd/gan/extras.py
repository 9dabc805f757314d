"""The seam between `train()` and the features that log or travel with the losses: AdaState, LeCamState, MatchState, LrSchedule, GradGuard carry
    slots                            [(name, fp32 device tensor, leading floats of it)] to read with the losses
    key                              the checkpoint key train() writes its `state_dict()` under, or None (CondGan.save_dict has ada's and lecam's)
    log_lines(iteration, values)     its lines of the log block; `values`: {name: [floats]} of every slot read so far"""
import torch

from .. import functional as TF

LOSSES = ('lD', 'lG', 'kl')          # the loss slots in front of the extras' (kl: conditioning augmentation only, else 0)


def training_extras(gan, optD, optG):
    """The extras of a run in the order of their log lines: ada, lecam, match, lr schedule, guard. Call it when train() starts."""
    sched, guard = optD.lr_sched and optD.lr_sched.sched, optD.grad_guard and optD.grad_guard.guard
    if sched is not None:
        sched.it0 = sched.counters()['D'] // sched.spi['D']       # its log counts on from where the device state stands now
    return [e for e in (gan.ada, getattr(gan, 'lecam', None), getattr(gan, 'match', None), sched, guard) if e is not None]


class Readout(object):
    """The losses and the extras' floats, read ONE iteration late through two pinned buffers with an event each: the host launches
    the next iteration while this one runs (a replay overwrites its loss scalars, hence the copies). One copy launch per slot: a
    kernel writing the pinned buffer in place. CPU: plain copies."""

    def __init__(self, extras, device):
        self.slots, off = [], 0                # (name, offset, floats, tensor or None: handed to `push`)
        for name, t, n in [(l, None, 1) for l in LOSSES] + [s for e in extras for s in e.slots]:
            self.slots.append((name, off, n, t))
            off += n
        self.width = -(-off // 4) * 4          # whole 16-byte rows
        self.cuda = torch.device(device).type == 'cuda'
        self.ring = [(torch.zeros(self.width).pin_memory() if self.cuda else torch.zeros(self.width),
                      torch.cuda.Event() if self.cuda else None) for _ in range(2)]
        self.prev = self.last = None           # the ring entries of the last two pushes

    def push(self, k, **losses):
        """Start the copies of iteration `k`: the loss tensors by slot name (None: stays 0) and every extra's."""
        hbuf, ev = self.ring[k & 1]
        for name, off, n, t in self.slots:
            t = losses.get(name, t)
            if t is None:
                continue
            if self.cuda:
                TF._copy2d(t, 0, n, hbuf, off, n, 1, n)
            else:
                hbuf[off:off + n].copy_(t.reshape(-1)[:n])
        if ev is not None:
            ev.record()
        self.prev, self.last = self.last, self.ring[k & 1]

    def pop(self):
        """{name: [floats]} of the push before the last one (waits for its event); None before there is one."""
        if self.prev is None:
            return None
        hbuf, ev = self.prev
        if ev is not None:
            ev.synchronize()
        return {name: hbuf[off:off + n].tolist() for name, off, n, t in self.slots}

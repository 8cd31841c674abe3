"""The zero arena: one buffer, cleared once per step, that every gradient accumulation target is a slice of."""
import torch

from . import capture


class _ZeroArena:
    """Zero-initialised f32 scratch for gradient accumulation targets (the `_acc` kernels add into
    their output).  One big buffer is cleared with ONE fill per step instead of one fill launch per
    gradient tensor (~1300 per step).  Slices stay valid until the next `recycle()`, which the
    optimizer's zero_grad() calls once the gradients have been consumed; until the first recycle()
    the arena is off and `zeros()` falls back to torch.zeros."""

    def __init__(self):
        self.buf = None
        self.off = 0
        self.high = 0
        self.active = False
        self.extra = []
        self.cap = 0

    def recycle(self, device):
        device = torch.device(device)
        need = max(self.high, 1 << 20)
        if self.buf is None or self.buf.device != device or self.buf.numel() < need:
            if self.buf is not None:
                capture.hold_or_ask("gradient arena", self.buf)     # (outgrown inside a capture that wrote slices of it)
            self.buf = torch.zeros(int(need * 1.25), dtype=torch.float32, device=device)
        elif self.off:
            self.buf[:self.off].zero_()
        self.off = 0
        self.high = 0
        self.extra = []
        self.active = True
        self.cap = self.buf.numel()

    def zeros(self, shape, device):
        # ~800 calls per step: one aten call (as_strided) instead of slice + view, no torch.device() construction
        nd = len(shape)
        if nd == 1:
            n = shape[0]
            stride = (1,)
        elif nd == 2:
            n = shape[0] * shape[1]
            stride = (shape[1], 1)
        else:
            n = 1
            stride = [1] * nd
            for i in range(nd - 1, -1, -1):
                stride[i] = n
                n *= shape[i]
        n_al = (n + 63) // 64 * 64           # keep every slice 256-byte aligned
        self.high += n_al
        buf = self.buf
        if not self.active or self.off + n_al > self.cap or (buf.device != device and buf.device != torch.device(device)):
            return torch.zeros(shape, dtype=torch.float32, device=device)
        out = buf.as_strided(shape, stride, self.off)
        self.off += n_al
        return out


ARENA = _ZeroArena()

# what every capture reads, held once per capture: the buffer whose slices a captured backward writes
capture.provide(lambda: (("gradient arena", ARENA.buf),))


def zeros_f32(shape, device):
    return ARENA.zeros(tuple(shape), device)

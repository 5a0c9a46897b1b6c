"""Tensors with guard rows for the tests of stand-alone entry points: the tensor handed to a kernel is the contiguous middle slice of
a larger one whose first and last ROWS rows hold a fixed pattern - NaN for floating-point types, 0x5A bytes for every other type (int64:
0x5A5A5A5A5A5A5A5A), the patterns of HumanoidSMPLIM._buffer.  A kernel that stores in front of or behind its rows changes the pattern.

`empty` gives an output (payload poisoned too), `of` an input or in/out state (payload = the array).  `arm()` records the guard rows as
they are; `check()` then compares them with that record bit for bit and no longer with the pattern, so a guard row may hold valid
numbers (`of(..., spill=k)`: the array's last k rows are the first k rows of the back guard - a launch k rows too wide stays inside the
test's own memory, and `check()` names what it wrote there).  A store of the bits already there is invisible to either mode.

`damaged()` is the finding as data: [(name, side)], side "in front of" or "behind"; `check()` raises GuardDamage, which carries it."""
import numpy as np
import torch

ROWS = 64
BYTE = 0x5A
FRONT, BEHIND = "in front of", "behind"


class GuardDamage(AssertionError):
    def __init__(self, message, damaged):
        super().__init__(message)
        self.damaged = damaged


class Guarded:
    def __init__(self, device):
        self.device = device
        self.held = []
        self.record = None

    def empty(self, name, shape, dtype=torch.float32):
        """[shape] on the device, every payload element NaN / 0x5A too: an element the kernel does not write is seen by the comparison."""
        lead = ROWS if len(shape) > 1 else ROWS * 64  # (1-d outputs: 64 x 64 elements on either side)
        full = torch.empty((shape[0] + 2 * lead,) + tuple(shape[1:]), dtype=dtype, device=self.device)
        if dtype.is_floating_point:
            full.fill_(float("nan"))
        else:
            full.view(torch.uint8).fill_(BYTE)
        self.held.append((name, full, lead))
        return full[lead:lead + shape[0]]

    def of(self, name, array, dtype=None, spill=0):
        """`array` (numpy or tensor) uploaded as the payload between the same guard rows; with spill = k the payload is all but the last
        k rows, and those k rows lie in the first k rows of the back guard (arm() before the launch)."""
        src = array.detach().cpu() if torch.is_tensor(array) else torch.as_tensor(np.ascontiguousarray(array))
        src = src.to(dtype=src.dtype if dtype is None else dtype)
        rows = src.shape[0] - spill
        assert src.dim() >= 1 and 0 <= spill <= ROWS and rows >= 0, (name, tuple(src.shape), spill)
        payload = self.empty(name, (rows,) + tuple(src.shape[1:]), src.dtype)
        _, full, lead = self.held[-1]
        full[lead:lead + src.shape[0]].copy_(src)
        return payload

    def wide(self, name, extra):
        """The payload of `name` together with the `extra` rows behind it (what `of(..., spill=extra)` put there)."""
        full, lead = next((full, lead) for n, full, lead in self.held if n == name)
        return full[lead:full.shape[0] - lead + extra]

    def _sides(self, full, lead):
        return ((FRONT, full[:lead]), (BEHIND, full[full.shape[0] - lead:]))

    def arm(self):
        """Record the guard rows of every tensor held so far as they are now: check() compares with the record, bit for bit."""
        self._sync()
        self.record = [tuple(rows.contiguous().view(torch.uint8).clone() for _, rows in self._sides(full, lead)) for _, full, lead in self.held]

    def _sync(self):
        if torch.device(self.device).type == "cuda":
            torch.cuda.synchronize()

    def _findings(self):
        self._sync()
        out = []
        for k, (name, full, lead) in enumerate(self.held):
            for j, (side, rows) in enumerate(self._sides(full, lead)):
                if self.record is not None and k < len(self.record):
                    bad = (rows.contiguous().view(torch.uint8) != self.record[k][j]).view(-1, full.element_size()).any(1)
                else:
                    bad = ~(torch.isnan(rows) if full.dtype.is_floating_point else rows.contiguous().view(torch.uint8) == BYTE)
                    bad = bad.reshape(-1, 1 if full.dtype.is_floating_point else full.element_size()).any(1)
                if bool(bad.any()):
                    out.append((name, side, int(bad.sum()), full.shape[0] - 2 * lead))
        return out

    def damaged(self):
        """[(name, side)] of every tensor with a changed guard element, in the order the tensors were made, front before behind."""
        return [(name, side) for name, side, _, _ in self._findings()]

    def check(self):
        found = self._findings()
        if found:
            raise GuardDamage("; ".join("%s: %d element(s) written %s its %d rows" % (name, count, side, rows) for name, side, count, rows in found), [(name, side) for name, side, _, _ in found])

"""Output tensors with guard rows for the tests of stand-alone entry points: the tensor handed to a kernel is the contiguous middle slice of
a larger one whose first and last ROWS rows hold a fixed pattern - NaN for floating-point types, 0x5A bytes for every other type (int64:
0x5A5A5A5A5A5A5A5A), the patterns of HumanoidSMPLIM._buffer.  A kernel that stores in front of or behind its rows changes the pattern."""
import torch

ROWS = 64
BYTE = 0x5A


class Guarded:
    def __init__(self, device):
        self.device = device
        self.held = []

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

    def check(self):
        torch.cuda.synchronize()
        for name, full, lead in self.held:
            for side, rows in (("in front of", full[:lead]), ("behind", full[full.shape[0] - lead:])):
                ok = torch.isnan(rows) if full.dtype.is_floating_point else rows.view(torch.uint8) == BYTE
                assert bool(ok.all()), "%s: %d element(s) written %s its %d rows" % (name, int((~ok).sum()), side, full.shape[0] - 2 * lead)

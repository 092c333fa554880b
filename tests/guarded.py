"""Guard bands around device buffers (helper of tests/test_containment_gpu.py; not a conftest).

torch's caching allocator rounds every tensor up to 512 bytes and carves tensors out of larger segments: a store a few elements or a
whole tile past the end of an output lands in padding or in a neighbour no test looks at again.  `Guarded` owns ONE uint8 device buffer
laid out [front guard | payload | back guard]:
  - the back guard starts at the byte after the payload's last byte - no rounding, no padding;
  - the front guard is a multiple of 256 bytes long, so the payload keeps the alignment torch's allocator gives every tensor;
  - each guard is at least max(1 MiB, 2 x payload bytes) - a condition, not a measurement: more than one misplaced 64-channel tile of the
    largest plane the containment module uses (64 x 17 x 33 x 4 B = 144 KB);
  - guards hold a byte pattern (0xA5 around what a kernel writes; 0x00 or 0xFF, the caller's choice, around what it reads), output
    payloads start as 0xFF bytes (NaN as floats, an impossible value as a pool's decision byte).
"""
import torch

GUARD_MIN = 1 << 20
PATTERN = 0xA5
POISON = 0xFF


def guard_bytes(payload_bytes):
    g = max(GUARD_MIN, 2 * int(payload_bytes))
    return (g + 255) // 256 * 256


class Guarded:
    def __init__(self, shape, dtype=torch.float32, fill=POISON, guard_fill=PATTERN, device="cuda"):
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        self.dtype = dtype
        self.guard_fill = int(guard_fill)
        numel = 1
        for s in self.shape:
            numel *= s
        self.nbytes = numel * torch.empty((), dtype=dtype).element_size()
        self.front = self.back = guard_bytes(self.nbytes)
        self.buf = torch.full((self.front + self.nbytes + self.back,), self.guard_fill, dtype=torch.uint8, device=device)
        self.payload_bytes = self.buf[self.front:self.front + self.nbytes]
        self.payload_bytes.fill_(int(fill))
        self.payload = self.payload_bytes.view(dtype).view(self.shape)
        assert self.payload.is_contiguous() and (self.nbytes == 0 or self.payload.data_ptr() == self.ptr())
        assert self.front % 256 == 0 and self.front >= max(GUARD_MIN, 2 * self.nbytes) and self.back >= max(GUARD_MIN, 2 * self.nbytes)

    @classmethod
    def of(cls, tensor, guard_fill=PATTERN, device="cuda"):
        """The same layout around a copy of `tensor` (an input, or an argument a kernel updates in place)."""
        g = cls(tensor.shape, tensor.dtype, fill=0, guard_fill=guard_fill, device=device)
        g.payload.copy_(tensor)
        return g

    def ptr(self):
        return self.buf.data_ptr() + self.front

    def bits(self):
        """The payload's bytes on the host (bit comparisons: NaN payloads compare by their bytes)."""
        return self.payload_bytes.cpu().clone()

    def damage(self):
        """None when both guards still hold their pattern (one device comparison per guard); else the first and last changed byte as
        offsets relative to the payload's END (0 = the byte right behind it; front-guard bytes are below -nbytes)."""
        spans = []
        for base, region in ((-self.nbytes - self.front, self.buf[:self.front]), (0, self.buf[self.front + self.nbytes:])):
            if not bool((region == self.guard_fill).all()):
                idx = (region != self.guard_fill).nonzero().flatten()
                spans.append((base + int(idx[0]), base + int(idx[-1]), int(idx.numel())))
        if not spans:
            return None
        return dict(first=min(s[0] for s in spans), last=max(s[1] for s in spans), changed=sum(s[2] for s in spans), payload_bytes=self.nbytes)

    def intact(self):
        return self.damage() is None

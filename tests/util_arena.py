"""A guarded device arena for the buffer-contract tests (tests/test_buffer_contract_gpu.py).

One uint8 device tensor filled with a POISON byte; `carve` hands out views of exactly the bytes asked for, at exactly
the alignment asked for, with a guard zone of poison in front of and behind every view.  `check` synchronises and
asserts that every guard byte still holds the poison: a kernel that stores one row, one vector or one element past a
buffer it was lent is reported with the buffer's name, the side and the first and last disturbed offsets.

Two poisons: 0xFF is NaN as fp16 / fp32 (and -1 as int8, 255 as uint8), 0x55 is a finite number in every type.  A float
kernel that READS a guard or scratch it never wrote and multiplies it by a zero weight turns 0xFF into NaN in its
output; an integer kernel shows the same defect as a difference between its results under the two poisons.

Guard width: at least 64 KiB on each side (one 128 x 256 fp16 output tile, the largest single tile a kernel of this
library stores); for scratch buffers at least the buffer's own size, capped at 8 MiB."""
import torch

POISONS = (0xFF, 0x55)
MIN_GUARD = 64 * 1024
MAX_SCRATCH_GUARD = 8 * 1024 * 1024
BASE_ALIGN = 4096


def _round_up(v, to):
    return (v + to - 1) // to * to


class Arena:
    def __init__(self, capacity, poison, device="cuda"):
        assert poison in POISONS
        self.poison = poison
        raw = torch.empty(capacity + 2 * BASE_ALIGN, dtype=torch.uint8, device=device)
        skip = (-raw.data_ptr()) % BASE_ALIGN
        self.buf = raw[skip:skip + capacity + BASE_ALIGN]
        self.buf.fill_(poison)
        self.cursor = 0
        self.views = []      # (name, start, nbytes, guard)

    def carve(self, nbytes, align, name, scratch=False):
        """uint8 view of exactly `nbytes` whose address is a multiple of `align` and of nothing larger (an odd
        multiple of it: 16 means 16, not 32), with poison guards on both sides."""
        nbytes = int(nbytes)
        assert nbytes > 0 and 1 <= align <= BASE_ALIGN // 2 and align & (align - 1) == 0
        guard = max(MIN_GUARD, min(nbytes, MAX_SCRATCH_GUARD)) if scratch else MIN_GUARD
        start = _round_up(self.cursor + guard, max(BASE_ALIGN, 2 * align)) + align
        end = start + nbytes + guard
        assert end <= self.buf.numel(), f"arena too small for {name}: {end} > {self.buf.numel()}"
        self.views.append((name, start, nbytes, guard))
        self.cursor = end
        view = self.buf[start:start + nbytes]
        assert view.data_ptr() % align == 0 and view.data_ptr() % (2 * align) != 0
        return view

    def empty(self, shape, dtype, align, name, scratch=False, channels_last=False):
        """Typed, shaped, contiguous tensor over a carved view, left holding the poison.  channels_last: `shape` is
        [N, C, H, W] and the memory is [N, H, W, C]."""
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        flat = self.carve(n * torch.empty((), dtype=dtype).element_size(), align, name, scratch).view(dtype)
        if channels_last:
            N, C, H, W = shape
            return flat.view(N, H, W, C).permute(0, 3, 1, 2)
        return flat.view(shape)

    def place(self, tensor, align, name, channels_last=False):
        """The contents of `tensor` (host or device) in a carved view of exactly its size."""
        out = self.empty(tensor.shape, tensor.dtype, align, name, channels_last=channels_last)
        out.copy_(tensor)
        return out

    def lender(self, align, log=None):
        """A stand-in for bevformer_tensorrt_amd.utils.workspace.lend: every request gets a fresh scratch view of
        EXACTLY nbytes at `align`, pre-filled with the poison.  `log` collects (tag, nbytes, view)."""
        def lend(tag, nbytes, device, stream_ptr):
            view = self.carve(nbytes, align, f"scratch:{tag}:{len(self.views)}", scratch=True)
            if log is not None:
                log.append((tag, int(nbytes), view))
            return view
        return lend

    def disturbed(self):
        """[(name, side, first offset, last offset, count)] of guard bytes that no longer hold the poison; offsets
        count from the buffer's end for 'behind' and back from its start for 'front' (0 = the adjacent byte)."""
        if self.buf.is_cuda:
            torch.cuda.synchronize()
        found = []
        for name, start, nbytes, guard in self.views:
            for side, lo, hi in (("front", start - guard, start), ("behind", start + nbytes, start + nbytes + guard)):
                bad = self.buf[lo:hi] != self.poison
                if bool(bad.any()):
                    idx = bad.nonzero().flatten()
                    first, last = int(idx[0]), int(idx[-1])
                    if side == "front":
                        first, last = hi - lo - 1 - last, hi - lo - 1 - first
                    found.append((name, side, first, last, int(idx.numel())))
        return found

    def check(self):
        found = self.disturbed()
        assert not found, "guard bytes overwritten: " + "; ".join(
            f"{name}: {count} bytes {side}, offsets {first}..{last}" for name, side, first, last, count in found)

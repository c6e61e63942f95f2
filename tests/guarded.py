"""Caller-owned buffers with the memory around them under watch.

The device-resident entry points read and write the caller's memory directly.  A plain torch.empty([n][O]) cannot show a
store past the last row (a caching allocator rounds sizes up: the store lands in slack or in a neighbour), a read past the
last row (the memory behind is zeros) or a kernel that only works where torch.empty happens to put a buffer.  guarded() puts
a buffer of exactly the payload's extent inside a larger allocation:

    | slack | head guard | payload (the view handed to the library) | tail guard | slack |
                         ^ byte_offset bytes past a 256-byte boundary

  * outputs (payload given as an element count): both guards AND the interior hold a sentinel no result can equal --
    float32: a NaN with a payload (the hardware's NaNs are 0x7fc00000 / 0xffc00000), compared as int32; int32: a negative
    constant (results are node indices).  check() asserts both guards intact and no sentinel left inside.
  * inputs (payload given as an array): the "guards" are poison a kernel must never let reach a result -- NaN around
    float rows, 1 / -128 bytes around byte masks, all-ones words around bit masks (`fill`) -- and check() asserts the WHOLE
    allocation is byte-identical to what it was.

Everything is compared where the tensor lives (torch.equal on int32 / uint8 views): nothing large travels to the host.
Guard sizes come from the kernels, not from taste (out_guard / in_guard below): the largest frame tile is 320 rows, the
widest node tile 256 nodes, so a kernel that stores a padded row of its last partial tile stays inside an output's guards;
a read that runs on past an input's last row meets poison for another 320 rows.  No buffer is placed against unmapped memory:
a read that never reaches a result is out of scope."""
import numpy as np
import torch

FRAME_TILE = 320   # the largest frame tile of any output kernel (fdnn_select.hpp)
NODE_TILE = 256    # the widest node tile: a padded row is the width rounded up to this
BOUNDARY = 256     # the view's base is byte_offset past a multiple of this
SLACK = 512        # bytes outside either guard, inside the allocation (nothing out there is watched)

NAN_SENTINEL = 0x7FC5A5A5        # float32 sentinel as int32: a quiet NaN with payload 0x05a5a5
INT_SENTINEL = -0x5A5A5A5B       # int32 sentinel


def out_guard(width):
    """Elements in each guard of an output [n][width]: one whole largest frame tile of padded rows."""
    return FRAME_TILE * (-(-int(width) // NODE_TILE) * NODE_TILE)


def in_guard(width):
    """(head, tail) elements of poison around an input [n][width]: one row in front, 320 rows behind."""
    return int(width), FRAME_TILE * int(width)


def _bits(dtype):
    """The integer dtype elements of `dtype` are compared in."""
    size = torch.empty((), dtype=dtype).element_size()
    return {1: torch.uint8, 4: torch.int32, 8: torch.int64}[size]


def _sentinel_tensor(dtype, fill):
    """One element of `dtype` holding the sentinel / poison, as a CPU tensor."""
    if fill is None:
        if dtype == torch.float32:
            return torch.tensor([NAN_SENTINEL], dtype=torch.int32).view(torch.float32)
        if dtype == torch.int32:
            return torch.tensor([INT_SENTINEL], dtype=torch.int32)
        raise ValueError(f"no default sentinel for {dtype}: pass fill")
    if isinstance(fill, float) and fill != fill:
        if dtype != torch.float32:
            raise ValueError("a NaN fill needs float32")
        return torch.tensor([NAN_SENTINEL], dtype=torch.int32).view(torch.float32)
    return torch.tensor([fill], dtype=dtype)


class Guarded:
    """What guarded() returns.  view: the payload's extent, 1-D, of `dtype` (hand view.data_ptr() / ptr to the library);
    whole: head guard + payload + tail guard as one 1-D tensor of `dtype` (payload from index `head` on); raw: the
    allocation as bytes."""

    def __init__(self, raw, start, count, dtype, head, tail, sentinel, is_input, name):
        size = sentinel.element_size()
        self.raw, self.dtype, self.head, self.tail, self.count, self.is_input, self.name = raw, dtype, head, tail, count, is_input, name
        self.whole = raw[start - head * size:start + (count + tail) * size].view(dtype)
        self.view = self.whole[head:head + count]
        self.ptr = self.view.data_ptr()
        self._sent = sentinel.to(raw.device).view(_bits(dtype))
        self._orig = None

    def freeze(self):
        """Inputs: remember the allocation's bytes (after the caller has filled the view)."""
        self._orig = self.raw.clone()
        return self

    def _first(self, bad):
        return int(torch.nonzero(bad)[0])

    def assert_untouched(self, what=""):
        """A call that was refused before any launch: an output still holds nothing but the sentinel, an input its bytes."""
        if self.is_input:
            return self.check(what)
        w = self.whole.view(_bits(self.dtype))
        if not torch.equal(w, self._sent.expand(w.numel())):
            at = self._first(w != self._sent) - self.head
            raise AssertionError(f"{what} {self.name}".strip() + f": written at element {at} of the view by a call that should have launched nothing")

    def check(self, what=""):
        tag = f"{what} {self.name}".strip()
        if self.is_input:
            if not torch.equal(self.raw, self._orig):
                at = self._first(self.raw != self._orig) - (self.view.data_ptr() - self.raw.data_ptr())
                raise AssertionError(f"{tag}: the input allocation changed at byte {at} of the view")
            return
        w = self.whole.view(_bits(self.dtype))
        head, body, tail = w[:self.head], w[self.head:self.head + self.count], w[self.head + self.count:]
        for part, label, base in ((head, "before", -self.head), (tail, "after", self.count)):
            if not torch.equal(part, self._sent.expand(part.numel())):
                at = self._first(part != self._sent) + base
                raise AssertionError(f"{tag}: write outside the buffer, {label} it, at element {at} of the view ({self.count} elements)")
        left = body == self._sent
        if bool(left.any()):
            raise AssertionError(f"{tag}: {int(left.sum())} elements of the buffer were never written, the first at {self._first(left)}")


def guarded(payload, dtype, head_elems, tail_elems, byte_offset=0, fill=None, device=None, name=""):
    """A view of exactly the payload's extent inside a larger allocation (module docstring).

    payload      an element count (an OUTPUT: interior filled with the sentinel) or a numpy array / torch tensor of `dtype`'s
                 element size (an INPUT: copied into the view, the surroundings poisoned with `fill`)
    head_elems,  elements of guard / poison before and after the view (out_guard, in_guard)
    tail_elems
    byte_offset  the view's base sits this many bytes past a 256-byte boundary; a multiple of the element size
    fill         the sentinel / poison value (None: the dtype's default; float('nan'): the NaN sentinel)"""
    is_input = not isinstance(payload, (int, np.integer))
    sentinel = _sentinel_tensor(dtype, fill)
    size = sentinel.element_size()
    if is_input:
        src = torch.from_numpy(np.ascontiguousarray(payload)) if isinstance(payload, np.ndarray) else payload.contiguous()
        if src.element_size() != size:
            raise ValueError(f"payload elements are {src.element_size()} bytes, {dtype} has {size}")
        count = src.numel()
        device = device if device is not None else src.device
    else:
        count = int(payload)
        device = device if device is not None else "cpu"
    if byte_offset < 0 or byte_offset >= BOUNDARY or byte_offset % size:
        raise ValueError(f"byte_offset must be a multiple of {size} in [0, {BOUNDARY})")
    head_b, body_b, tail_b = int(head_elems) * size, count * size, int(tail_elems) * size
    raw = torch.zeros(SLACK + head_b + BOUNDARY + body_b + tail_b + SLACK, dtype=torch.uint8, device=device)
    base = raw.data_ptr()
    start = SLACK + head_b
    start += (byte_offset - (base + start)) % BOUNDARY
    assert (base + start - byte_offset) % BOUNDARY == 0 and start - head_b >= SLACK and start + body_b + tail_b + SLACK <= raw.numel()
    g = Guarded(raw, start, count, dtype, int(head_elems), int(tail_elems), sentinel, is_input, name)
    g.whole.view(_bits(dtype))[:] = g._sent
    if is_input:
        g.view.view(_bits(dtype))[:] = src.reshape(-1).view(_bits(dtype)).to(raw.device)
        g.freeze()
    assert g.ptr == base + start and (g.ptr - byte_offset) % BOUNDARY == 0
    return g

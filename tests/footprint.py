"""Memory-footprint helpers: guarded outputs, poisoned operands, exact scratch.

A per-kernel test compares the tensor a launch returns with a reference.  These helpers check what a launch does OUTSIDE that
tensor and what it reads outside its operands: every buffer a case hands to a kernel is a strided view inside one larger
allocation (the arena) whose lead guard, trail guard and leading-dimension gaps hold a fixed bit pattern.

  guarded(shape, dtype, device, ld=...)  an output: guards / gaps hold the OUTPUT SENTINEL, a NaN bit pattern no kernel of the
                                         library produces (bf16 0xFFA5, fp32 0xFFA5A5A5, 0xFF bytes); the payload holds it too
                                         until the kernel writes it, so an element the kernel skips is visible as well
  poisoned(tensor, ld=...)               an operand: the same values, guards / gaps hold the INPUT POISON (bf16 0x7FC1, fp32
                                         0x7FC00001, 0xFF bytes for e4m3 bytes and scale words): a kernel that pulls a gap into
                                         a reduction or a product turns its result into NaN
  exact_scratch(nbytes, device)          a scratch buffer of exactly nbytes (16-byte aligned) between two guards; payload and
                                         guards hold 0xFF bytes (fp32 NaN), so scratch read before it is written shows up too
  assert_untouched(record)               every guard / gap byte still holds its pattern, compared BITWISE through an integer
                                         view (a NaN overwritten by another NaN is a touch); the message names the first touched
                                         byte offset and its region: lead guard, trail guard or the ld gap of row r

Guards are at least 64 KiB and at least 256 rows of the view on each side, so an overrun of a whole tile stays inside memory
the test owns: it is recorded, it does not fault.  Everything works on any torch device (tests/test_footprint_cpu.py plants
violations with CPU stand-in kernels).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch

GUARD_MIN_BYTES = 64 << 10
GUARD_MIN_ROWS = 256
_ALIGN = 256                      # guards are multiples of this, so the view keeps the allocation's alignment

# element size -> integer dtype of the bitwise view
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32}


def _signed(pattern: int, nbytes: int) -> int:
    bits = 8 * nbytes
    if nbytes == 1:
        return pattern                                   # uint8
    return pattern - (1 << bits) if pattern >= (1 << (bits - 1)) else pattern


def _esize(dtype: torch.dtype) -> int:
    return torch.empty((), dtype=dtype).element_size()


def out_sentinel(dtype: torch.dtype) -> int:
    """bit pattern of the output sentinel for one element of ``dtype``"""
    return {1: 0xFF, 2: 0xFFA5, 4: 0xFFA5A5A5}[_esize(dtype)]


def in_poison(dtype: torch.dtype) -> int:
    """bit pattern of the input poison: NaN for bf16 / fp32, 0xFF bytes for e4m3 bytes and integer (scale) words"""
    if dtype == torch.bfloat16:
        return 0x7FC1
    if dtype == torch.float32:
        return 0x7FC00001
    return {1: 0xFF, 2: 0xFFFF, 4: 0xFFFFFFFF}[_esize(dtype)]


@dataclass
class ArenaRecord:
    """where a view lies inside its arena (all offsets in bytes from the arena's first byte)"""
    name: str
    arena: torch.Tensor           # uint8 [total]
    pattern: int                  # element bit pattern of guards and gaps
    esize: int
    lead: int                     # bytes of the lead guard = offset of the view's first byte
    rows: int
    row_bytes: int                # ld * esize
    payload_bytes: int            # shape[-1] * esize
    trail: int                    # bytes of the trail guard

    @property
    def body(self) -> int:
        """bytes from the view's first byte to the start of the trail guard: the last row ends with its payload"""
        return (self.rows - 1) * self.row_bytes + self.payload_bytes if self.rows else 0

    @property
    def total(self) -> int:
        return self.lead + self.body + self.trail

    def region_of(self, offset: int) -> str:
        if offset < self.lead:
            return f"lead guard (byte {offset} of {self.lead}, {self.lead - offset} before the view)"
        if offset >= self.lead + self.body:
            return f"trail guard ({offset - self.lead - self.body} bytes past the view's end)"
        r, c = divmod(offset - self.lead, self.row_bytes)
        if c >= self.payload_bytes:
            return f"ld gap of row {r} (byte {c - self.payload_bytes} of the gap, column {c // self.esize})"
        return f"payload of row {r}"


def _round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def _guard_bytes(requested: Optional[int], row_bytes: int) -> int:
    g = max(GUARD_MIN_BYTES, GUARD_MIN_ROWS * row_bytes)
    if requested is not None:
        g = max(g, int(requested))
    return _round_up(g, _ALIGN)


def _fill(arena: torch.Tensor, pattern: int, esize: int) -> None:
    n = arena.numel() // esize * esize
    arena[:n].view(_INT_VIEW[esize]).fill_(_signed(pattern, esize))
    if n < arena.numel():                                  # (exact scratch of a size that is no multiple of the element)
        tail = torch.tensor([(pattern >> (8 * i)) & 0xFF for i in range(arena.numel() - n)], dtype=torch.uint8)
        arena[n:] = tail.to(arena.device)


def _arena(name: str, shape: Sequence[int], dtype: torch.dtype, device, ld: Optional[int], lead: Optional[int],
           trail: Optional[int], pattern: int) -> Tuple[torch.Tensor, ArenaRecord]:
    shape = tuple(int(s) for s in shape)
    assert len(shape) >= 1 and all(s > 0 for s in shape), shape
    es = _esize(dtype)
    cols = shape[-1]
    ld = cols if ld is None else int(ld)
    assert ld >= cols, f"{name}: ld {ld} < row length {cols}"
    rows = 1
    for s in shape[:-1]:
        rows *= s
    rec = ArenaRecord(name=name, arena=None, pattern=pattern, esize=es, lead=_guard_bytes(lead, ld * es), rows=rows,
                      row_bytes=ld * es, payload_bytes=cols * es, trail=_guard_bytes(trail, ld * es))
    total = _round_up(rec.total, es)
    rec.trail += total - rec.total
    rec.arena = torch.empty((total,), dtype=torch.uint8, device=device)
    _fill(rec.arena, pattern, es)
    strides = [1] * len(shape)
    if len(shape) >= 2:
        strides[-2] = ld
        for i in range(len(shape) - 3, -1, -1):
            strides[i] = strides[i + 1] * shape[i + 1]
    flat = rec.arena[rec.lead:rec.lead + _round_up(rec.body, es)].view(dtype)
    view = flat.as_strided(shape, strides)
    return view, rec


def guarded(shape, dtype, device, ld: Optional[int] = None, lead: Optional[int] = None, trail: Optional[int] = None,
            name: str = "out") -> Tuple[torch.Tensor, ArenaRecord]:
    """an output view of ``shape`` with row stride ``ld`` (elements, >= shape[-1]; leading dimensions are dense over the rows)
    inside a sentinel-filled arena; the payload starts out as sentinel too.  Returns (view, record)."""
    return _arena(name, shape, dtype, device, ld, lead, trail, out_sentinel(dtype))


def poisoned(tensor: torch.Tensor, ld: Optional[int] = None, lead: Optional[int] = None, trail: Optional[int] = None,
             name: str = "in", pattern: Optional[int] = None) -> Tuple[torch.Tensor, ArenaRecord]:
    """the values of ``tensor`` as a strided view inside an arena whose guards and ld gaps hold the input poison.
    ``pattern``: another fill (an in/out operand takes the output sentinel, which is a NaN as well)."""
    view, rec = _arena(name, tensor.shape, tensor.dtype, tensor.device, ld, lead, trail,
                       in_poison(tensor.dtype) if pattern is None else pattern)
    view.copy_(tensor)
    return view, rec


def exact_scratch(nbytes: int, device, lead: Optional[int] = None, trail: Optional[int] = None,
                  name: str = "scratch") -> Tuple[torch.Tensor, ArenaRecord]:
    """a uint8 view of exactly ``nbytes`` between two guards, 16-byte aligned (the guards are multiples of 256 bytes and the
    allocation itself is at least that aligned); payload and guards hold 0xFF bytes."""
    assert nbytes > 0
    view, rec = _arena(name, (int(nbytes),), torch.uint8, device, None, lead, trail, 0xFF)
    assert view.data_ptr() % 16 == 0, "exact_scratch: the allocation is not 16-byte aligned"
    return view, rec


def first_touched(rec: ArenaRecord) -> Optional[int]:
    """byte offset (from the arena's start) of the first guard / gap byte that no longer holds its pattern, or None"""
    a = rec.arena
    total = a.numel()
    pat = torch.tensor([(rec.pattern >> (8 * i)) & 0xFF for i in range(rec.esize)], dtype=torch.uint8, device=a.device)
    bad = a != pat.repeat(total // rec.esize)
    if rec.rows:
        body = bad[rec.lead:rec.lead + rec.body]
        full = (rec.rows - 1) * rec.row_bytes
        if full:
            body[:full].view(rec.rows - 1, rec.row_bytes)[:, :rec.payload_bytes] = False
        body[full:] = False                                            # the last row: payload only
    if not bool(bad.any()):
        return None
    return int(torch.nonzero(bad)[0, 0])


def assert_untouched(rec: ArenaRecord) -> None:
    off = first_touched(rec)
    if off is not None:
        got = int(rec.arena[off])
        want = (rec.pattern >> (8 * (off % rec.esize))) & 0xFF
        raise AssertionError(f"{rec.name}: byte {off} of the arena was touched ({got:#04x}, guard pattern {want:#04x}): "
                             f"{rec.region_of(off)}")


def bits(t: torch.Tensor) -> torch.Tensor:
    """the integer view a bitwise comparison uses (the tensor made dense first)"""
    return t.contiguous().view(_INT_VIEW[t.element_size()])


def bit_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def holds_sentinel(t: torch.Tensor) -> bool:
    """does any element of ``t`` hold the output sentinel of its dtype (a payload element the kernel did not write)?"""
    return bool((bits(t) == _signed(out_sentinel(t.dtype), t.element_size())).any())


def all_sentinel(t: torch.Tensor) -> bool:
    """does every element of ``t`` still hold the output sentinel (a part of an output the kernel must leave alone)?"""
    return bool((bits(t) == _signed(out_sentinel(t.dtype), t.element_size())).all())

"""Operands under the weakest memory contract a header allows, between guards the test owns.

A payload is placed inside ONE torch.uint8 allocation laid out as

    [ guard >= 64 KiB | pad | payload | guard >= 64 KiB ]

  * guard: 64 KiB = eight rows of 2048 f32, so an index of -1 or N times a row stride still lands in memory the test owns and is
    seen by intact(), instead of in somebody else's allocation.
  * pad: the payload starts at a 256-byte boundary plus `align`, so it has EXACTLY the alignment asked for and no more:
        align 16 (what a header calls 16-byte aligned: user, catalog, workspace, d_user)   base + 16
        align 8  (int64 operands: gt_index, exclude)                                       base + 8
        align 4  (everything else: f32 / int32 outputs, cat_inv_norm, index)               base + 4
    A fresh torch allocation is 512-byte aligned and would hide a kernel that quietly needs more than the header promises.
  * fill: the byte everything AROUND the payload holds (and the payload itself, when only a size is given):
        OUT  0x5A  outputs and their guards: 1.5e16 as f32, 1 515 870 810 as int32 -- no result looks like it, so all_written() can
                   tell an element the call never stored; also the surroundings of integer inputs (a stray index read there is huge
                   and positive, outside every catalogue)
        NAN  0xFF  the surroundings of floating-point inputs and one of the two workspace interiors: NaN as f32 and bf16, -1 in either
                   integer width.  A stale count read as -1 runs no loop and a stale index read as -1 lands in the guard, so a
                   read-before-write shows as a wrong answer, not as a wild address
        ZERO 0x00  the other workspace interior (what fresh device memory holds): a result that differs between the two interiors
                   was computed from bytes the call never wrote

Two-dimensional operands (the GEMM, attention and LoRA calls).  place(..., guard=bytes) widens both guards (rounded up to 64 KiB): a tile
kernel that overruns by a whole tile of rows is 256 row strides out, so callers pass guard_for(ld, element size) = max(64 KiB, 256 rows).
place(..., ld=elements) makes the payload the whole [rows, ld] base and hands out its [:, :width] view -- what the call sees; the pad
columns [width, ld) hold the arena's fill (0xFF beside floating-point inputs, 0x5A beside outputs) and pads_intact() tells whether every
one of them still does.  all_written() on a 16-bit output asks that no ELEMENT still reads 0x5A5A (1.5e16 as bf16): the caller picks
inputs whose results stay far below that and asserts so on its reference.

A plain helper module, no fixtures: tests/test_arena_host.py runs it on host tensors."""
import torch

GUARD = 64 * 1024
BASE = 256
OUT, NAN, ZERO = 0x5A, 0xFF, 0x00
OUT_WORD = 0x5A5A5A5A
OUT_HALF = 0x5A5A
ALIGNS = (4, 8, 16)


def guard_for(ld, element_size):
    """the guard of a 2-D operand with row stride ld (elements): a whole 256-row tile behind the last row, at least 64 KiB"""
    return max(GUARD, 256 * int(ld) * int(element_size))


def place(src, align, fill, *, device=None, interior=None, guard=GUARD, ld=None):
    """src: a tensor (its bytes become the payload; the view has its dtype and shape) or a number of bytes (a uint8 payload filled with
    `interior`, or with `fill` when interior is None).  Returns (whole, view): whole is the uint8 allocation, view the payload inside it
    at a 256-byte boundary + align.  The bytes of `whole` outside the payload hold `fill`; both guards have `guard` bytes rounded up to
    64 KiB.  ld (elements): src is a 2-D tensor or (rows, width, dtype); the payload is the [rows, ld] base, the view its [:, :width]
    columns -- a tensor's values, or `interior` / `fill` bytes -- and the pad columns hold `fill`."""
    if align not in ALIGNS:
        raise ValueError(f"align must be one of {ALIGNS}, got {align}")
    guard = (max(int(guard), 1) + GUARD - 1) // GUARD * GUARD
    is_tensor = isinstance(src, torch.Tensor)
    shape = None
    if ld is not None:
        rows, width, dtype = (src.shape[0], src.shape[1], src.dtype) if is_tensor else src
        if (is_tensor and src.dim() != 2) or ld < width:
            raise ValueError("a strided payload is 2-D with ld >= its width")
        esize = torch.empty((), dtype=dtype).element_size()
        if align % esize:
            raise ValueError(f"align {align} is below the natural alignment of {dtype}")
        device = src.device if (is_tensor and device is None) else device
        nbytes, shape = rows * ld * esize, (rows, width, dtype, ld)
    elif is_tensor:
        src = src.contiguous()
        device = src.device if device is None else device
        nbytes = src.numel() * src.element_size()
        if align % src.element_size():
            raise ValueError(f"align {align} is below the natural alignment of {src.dtype}")
    else:
        nbytes = int(src)
        if nbytes < 0:
            raise ValueError("nbytes must be >= 0")
    whole = torch.full((guard + BASE + align + nbytes + guard,), fill, dtype=torch.uint8, device=device)
    first = whole.data_ptr() + guard
    start = (first + BASE - 1) // BASE * BASE + align - whole.data_ptr()
    raw = whole[start:start + nbytes]
    if shape is not None:
        rows, width, dtype, ld = shape
        base = raw.view(dtype).view(rows, ld)
        view = base[:, :width]
        if is_tensor:
            view.copy_(src)
        elif interior is not None:
            raw.view(rows, ld * esize)[:, :width * esize] = interior
        whole.base, whole.width = base, width
    elif is_tensor:
        raw.copy_(src.reshape(-1).view(torch.uint8))
        view = raw.view(src.dtype).view(src.shape)
    else:
        if interior is not None:
            raw.fill_(interior)
        view = raw
    whole.arena = (start, nbytes, fill)
    assert view.data_ptr() == whole.data_ptr() + start and view.data_ptr() % BASE == align
    return whole, view


def typed(view, dtype, shape):
    """a uint8 payload seen as `dtype` of `shape` (the payload's alignment must allow the element size)"""
    return view.view(dtype).view(shape)


def intact(whole, view):
    """True when every byte of `whole` outside the payload `view` still holds the fill it was made with"""
    start, nbytes, fill = whole.arena
    size = whole.base.numel() * whole.base.element_size() if hasattr(whole, "base") else view.numel() * view.element_size()
    assert view.data_ptr() == whole.data_ptr() + start and size == nbytes, "not the view of this arena"
    return bool((whole[:start] == fill).all()) and bool((whole[start + nbytes:] == fill).all())


def pads_intact(whole):
    """True when every pad element (columns [width, ld) of a strided payload) still holds the fill; a dense payload has none"""
    if not hasattr(whole, "base"):
        return True
    start, nbytes, fill = whole.arena
    base = whole.base
    esize = base.element_size()
    rows, ld = base.shape
    raw = whole[start:start + nbytes].view(rows, ld * esize)
    return bool((raw[:, whole.width * esize:] == fill).all())


def all_written(view):
    """True when no element of the payload still holds the fill of an output nobody stored to: no 32-bit word 0x5A5A5A5A, and for a
    16-bit output (bf16) no ELEMENT 0x5A5A"""
    if view.element_size() == 2:
        return not bool((view.contiguous().view(torch.int16) == OUT_HALF).any())
    raw = view.contiguous().reshape(-1).view(torch.uint8)
    assert raw.numel() % 4 == 0, "outputs are made of 32-bit words"
    return not bool((raw.view(torch.int32) == OUT_WORD).any())


def untouched(whole):
    """True when every byte of the allocation, payload included, holds the fill (a refused call must leave its outputs alone)"""
    return bool((whole == whole.arena[2]).all())

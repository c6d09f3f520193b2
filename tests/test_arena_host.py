"""CPU: tests/arena.py on host tensors -- the guards report a one-byte write on either side of the payload, an unwritten word is
reported, and the pads give exactly the stated alignment (tests/test_gpu_catalog_memory.py relies on all three)."""
import pytest
import torch

from tests import arena


@pytest.mark.parametrize("align", arena.ALIGNS)
@pytest.mark.parametrize("nbytes", [4, 24, 1056, 4100])
def test_the_pad_gives_exactly_the_stated_alignment(align, nbytes):
    whole, view = arena.place(nbytes, align, arena.OUT)
    p = view.data_ptr()
    assert p % 256 == align                               # aligned to `align` and to nothing coarser
    assert p % align == 0 and p % (2 * align) != 0
    assert view.numel() == nbytes and whole.dtype == torch.uint8
    start = p - whole.data_ptr()
    assert start >= arena.GUARD and whole.numel() - (start + nbytes) >= arena.GUARD
    assert arena.intact(whole, view) and arena.untouched(whole)


def test_a_tensor_payload_keeps_its_bytes_dtype_and_shape():
    g = torch.Generator().manual_seed(0)
    for t, align, fill in ((torch.randn(17, 264, generator=g), 16, arena.NAN), (torch.randn(5, 8, generator=g).bfloat16(), 16, arena.NAN),
                           (torch.randint(-1, 99, (17, 9), generator=g), 8, arena.OUT),
                           (torch.randint(0, 99, (3, 5), generator=g, dtype=torch.int32), 4, arena.OUT)):
        whole, view = arena.place(t, align, fill)
        assert view.dtype == t.dtype and view.shape == t.shape and view.is_contiguous() and torch.equal(view, t)
        assert view.data_ptr() % 256 == align and arena.intact(whole, view)
        start, nbytes, _ = whole.arena
        assert bool((whole[:start] == fill).all()) and bool((whole[start + nbytes:] == fill).all())
    with pytest.raises(ValueError):
        arena.place(torch.zeros(3, dtype=torch.int64), 4, arena.OUT)         # below the natural alignment
    with pytest.raises(ValueError):
        arena.place(16, 32, arena.OUT)


def test_the_fills_read_as_the_module_says():
    _, v = arena.place(8, 4, arena.OUT)
    assert float(arena.typed(v, torch.float32, (2,))[0]) == pytest.approx(1.5e16, rel=0.05)
    assert int(arena.typed(v, torch.int32, (2,))[0]) == 1515870810 == arena.OUT_WORD
    _, v = arena.place(8, 8, arena.OUT, interior=arena.NAN)
    assert bool(torch.isnan(arena.typed(v, torch.float32, (2,))).all()) and bool(torch.isnan(arena.typed(v, torch.bfloat16, (4,))).all())
    assert arena.typed(v, torch.int32, (2,)).tolist() == [-1, -1] and arena.typed(v, torch.int64, (1,)).tolist() == [-1]
    _, v = arena.place(8, 16, arena.OUT, interior=arena.ZERO)
    assert arena.typed(v, torch.float32, (2,)).tolist() == [0.0, 0.0]


@pytest.mark.parametrize("align", arena.ALIGNS)
def test_a_one_byte_write_on_either_side_is_reported(align):
    for where in ("before", "after", "far_before", "far_after"):
        whole, view = arena.place(1056, align, arena.OUT)
        start, nbytes, _ = whole.arena
        at = {"before": start - 1, "after": start + nbytes, "far_before": 0, "far_after": whole.numel() - 1}[where]
        assert arena.intact(whole, view)
        whole[at] = 0x5B
        assert not arena.intact(whole, view), where
        assert not arena.untouched(whole)
    # a write INSIDE the payload is no guard violation
    whole, view = arena.place(1056, align, arena.OUT)
    view[0] = 1
    view[-1] = 1
    assert arena.intact(whole, view) and not arena.untouched(whole)


def test_an_unwritten_word_is_reported():
    whole, view = arena.place(4 * 40, 4, arena.OUT)
    out = arena.typed(view, torch.float32, (40,))
    assert not arena.all_written(out)
    out[:] = torch.arange(40, dtype=torch.float32)
    assert arena.all_written(out) and arena.all_written(view)
    for hole in (0, 17, 39):                                                     # first, middle and last word
        out[:] = torch.arange(40, dtype=torch.float32)
        arena.typed(view, torch.int32, (40,))[hole] = arena.OUT_WORD
        assert not arena.all_written(out), hole
    # three of the four bytes of a word written: the word no longer reads as the fill
    out[:] = torch.arange(40, dtype=torch.float32)
    view[4 * 5] = arena.OUT
    assert arena.all_written(out)
    ints = arena.typed(arena.place(4 * 6, 4, arena.OUT)[1], torch.int32, (2, 3))
    assert not arena.all_written(ints)
    ints[:] = -1
    assert arena.all_written(ints)


def test_the_guard_grows_to_what_is_asked_rounded_up_to_64_kib():
    for asked, got in ((1, arena.GUARD), (arena.GUARD, arena.GUARD), (arena.GUARD + 1, 2 * arena.GUARD), (256 * 4104 * 2, 33 * arena.GUARD)):
        whole, view = arena.place(1056, 16, arena.OUT, guard=asked)
        start, nbytes, _ = whole.arena
        assert got <= start < got + 2 * arena.BASE and got <= whole.numel() - (start + nbytes) < got + 2 * arena.BASE
        assert view.data_ptr() % 256 == 16 and arena.intact(whole, view)
        whole[got - 1] = 0                                                       # a byte a whole tile of rows before the payload
        assert not arena.intact(whole, view)
    assert arena.guard_for(2048, 4) == 256 * 2048 * 4 and arena.guard_for(8, 2) == arena.GUARD
    assert arena.place(8, 4, arena.OUT)[0].numel() == 2 * arena.GUARD + arena.BASE + 4 + 8      # the default is unchanged


@pytest.mark.parametrize("dtype,align", [(torch.bfloat16, 16), (torch.bfloat16, 8), (torch.float32, 4), (torch.float32, 16)])
def test_a_strided_payload_is_the_whole_base_and_its_pads_hold_the_fill(dtype, align):
    g = torch.Generator().manual_seed(1)
    t = torch.randint(-3, 4, (5, 24), generator=g).to(dtype)
    whole, view = arena.place(t, align, arena.NAN, ld=32)
    assert view.shape == (5, 24) and view.stride() == (32, 1) and view.dtype == dtype and torch.equal(view, t)
    assert view.data_ptr() % 256 == align and whole.base.shape == (5, 32) and whole.arena[1] == 5 * 32 * t.element_size()
    assert arena.intact(whole, view) and arena.pads_intact(whole)
    assert bool(torch.isnan(whole.base[:, 24:].float()).all())                   # 0xFF beside a floating-point input
    # an output: every element the fill, or `interior` inside the view and the fill in the pads
    whole, out = arena.place((5, 24, dtype), align, arena.OUT, ld=32)
    assert arena.untouched(whole) and arena.pads_intact(whole) and not arena.all_written(out)
    whole, out = arena.place((5, 24, dtype), align, arena.OUT, ld=32, interior=arena.NAN)
    assert bool(torch.isnan(out.float()).all()) and arena.pads_intact(whole) and arena.intact(whole, out)
    # one element written into the pad -- first pad column of the first row, last of the last row -- is reported, and is no guard violation
    for r, c in ((0, 24), (4, 31), (2, 27)):
        whole, out = arena.place((5, 24, dtype), align, arena.OUT, ld=32)
        out[:] = t
        assert arena.pads_intact(whole) and arena.all_written(out)
        whole.base[r, c] = 1.0
        assert not arena.pads_intact(whole) and arena.intact(whole, out)
    # a dense payload has no pads
    assert arena.pads_intact(arena.place(t, align, arena.NAN)[0])
    with pytest.raises(ValueError):
        arena.place(t, align, arena.NAN, ld=16)


def test_an_unwritten_16_bit_element_is_reported():
    whole, out = arena.place((3, 10, torch.bfloat16), 8, arena.OUT, ld=16)
    assert float(out[0, 0]) == pytest.approx(1.5e16, rel=0.05) and not arena.all_written(out)
    vals = torch.arange(30, dtype=torch.float32).reshape(3, 10).bfloat16()
    out[:] = vals
    assert arena.all_written(out)
    for r, c in ((0, 0), (1, 3), (2, 9)):                                       # ONE element of a 32-bit word left: the word check would miss it
        out[:] = vals
        out.view(torch.int16)[r, c] = arena.OUT_HALF
        assert not arena.all_written(out), (r, c)
    # a dense bf16 output of an odd element count (no whole 32-bit words) is taken element by element too
    _, raw = arena.place(2 * 7, 8, arena.OUT)
    odd = arena.typed(raw, torch.bfloat16, (7,))
    assert not arena.all_written(odd)
    odd[:] = 1.0
    assert arena.all_written(odd)

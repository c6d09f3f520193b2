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

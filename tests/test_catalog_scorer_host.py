"""CPU: the host side of the catalogue scorers and the bf16 catalogue -- the checks and the size query of ur_catalog_select_t's
catalog_bf16 / scorer fields through the raw library (fake non-null pointers: every call here returns before any launch), and
CatalogEvaluator(dtype=bf16) on the CPU device."""
import ctypes

import pytest
import torch

from unirec_amd import _lib, hip
from unirec_amd.evaluation import CatalogEvaluator

FAKE = 256          # non-null, 16-byte aligned, never dereferenced on the host


class _SelectABI16(ctypes.Structure):
    """ur_catalog_select_t as it was before catalog_bf16 / scorer: a caller that never heard of them.  The library reads two more
    int32 behind it, so the buffer below holds the struct plus zeroed room for them."""
    _fields_ = _lib.CatalogSelect._fields_[:-2]


def _select(**over):
    s = _lib.CatalogSelect()
    s.K, s.E = 10, 0
    s.topk_index = s.topk_score = FAKE
    for k, v in over.items():
        setattr(s, k, v)
    return s


def _call(lib, sel, B=4, N=5000, D=16):
    return lib.ur_catalog_scores(FAKE, FAKE, None, FAKE, FAKE, 0, B, N, D, ctypes.byref(sel), None)


def test_struct_mirror_ends_in_the_two_new_fields():
    names = [f[0] for f in _lib.CatalogSelect._fields_]
    assert names[-2:] == ["catalog_bf16", "scorer"] and names[-3] == "workspace_bytes"
    assert ctypes.sizeof(_lib.CatalogSelect) == ctypes.sizeof(_SelectABI16) + 8
    assert _lib.ABI_VERSION >= 17 and _lib.load().ur_version() == _lib.ABI_VERSION      # (the fields arrived with ABI 17)


@pytest.mark.parametrize("ws", [None, FAKE])
def test_bad_scorer_and_dtype_are_rejected_before_any_launch(ws):
    lib = _lib.load()
    need = _select()
    assert _call(lib, need) == 0
    for over in (dict(scorer=-1), dict(scorer=3), dict(catalog_bf16=-1), dict(catalog_bf16=2)):
        sel = _select(workspace=ws, workspace_bytes=need.workspace_bytes, **over)
        rc = _call(lib, sel)
        msg = lib.ur_last_error()
        assert rc < 0 and b"ur_catalog_scores" in msg and next(iter(over)).encode() in msg, (over, rc, msg)
    for scorer in (0, 1, 2):                                    # every valid pair passes the size query
        for bf in (0, 1):
            assert _call(lib, _select(scorer=scorer, catalog_bf16=bf)) == 0


@pytest.mark.parametrize("B,N,D,chunk_rows", [(4, 5000, 16, 0), (4, 5000, 16, 1024), (512, 4_000_000, 1024, 0), (17, 1300, 2048, 0)])
def test_size_query_with_zero_fields_is_the_old_one(B, N, D, chunk_rows):
    lib = _lib.load()
    # a struct that never touched the new fields: the ABI-16 layout inside a zeroed buffer of the new size
    buf = (ctypes.c_char * ctypes.sizeof(_lib.CatalogSelect))()
    old = _SelectABI16.from_buffer(buf)
    old.K, old.E, old.chunk_rows = 10, 0, chunk_rows
    old.topk_index = old.topk_score = FAKE
    rc = lib.ur_catalog_scores(FAKE, FAKE, None, FAKE, FAKE, 0, B, N, D, ctypes.cast(buf, ctypes.POINTER(_lib.CatalogSelect)), None)
    assert rc == 0 and old.workspace_bytes > 0
    zero = _select(chunk_rows=chunk_rows, scorer=0, catalog_bf16=0)
    assert _call(lib, zero, B=B, N=N, D=D) == 0 and zero.workspace_bytes == old.workspace_bytes
    vec = _select(chunk_rows=chunk_rows, scorer=1)
    assert _call(lib, vec, B=B, N=N, D=D) == 0 and vec.workspace_bytes == old.workspace_bytes
    for bf in (0, 1):
        mfma = _select(chunk_rows=chunk_rows, scorer=2, catalog_bf16=bf)
        assert _call(lib, mfma, B=B, N=N, D=D) == 0
        assert old.workspace_bytes <= mfma.workspace_bytes
        # whatever the MFMA scorer adds is no [B,N] buffer.  (Where one chunk holds the whole catalogue, rounded up to the 1024-score
        # tile, the chunk buffer alone is already B*N*4 or more; there the MFMA scorer must add nothing.)
        if old.workspace_bytes < B * N * 4:
            assert mfma.workspace_bytes < B * N * 4
        else:
            assert mfma.workspace_bytes == old.workspace_bytes


def test_scorer_names():
    assert hip.catalog_scorer_id(None) == 0 and hip.catalog_scorer_id("vector") == 1 and hip.catalog_scorer_id("mfma") == 2
    for bad in ("MFMA", "", "bf16", 2, 0, True):
        with pytest.raises(ValueError):
            hip.catalog_scorer_id(bad)


def test_bf16_evaluator_on_the_cpu_device(monkeypatch):
    g = torch.Generator().manual_seed(3)
    cat = torch.randn(37, 16, generator=g)
    ev = CatalogEvaluator(cat, device="cpu", dtype=torch.bfloat16)
    assert ev.catalog.dtype == torch.bfloat16 and ev.catalog.is_contiguous()
    assert torch.equal(ev.catalog, cat.to(torch.bfloat16)), "f32 input is rounded to nearest even, nothing else"
    assert torch.equal(CatalogEvaluator(cat.to(torch.bfloat16), device="cpu", dtype=torch.bfloat16).catalog, ev.catalog)
    assert CatalogEvaluator(cat, device="cpu").catalog.dtype == torch.float32, "the default stays f32"
    with pytest.raises(ValueError):
        CatalogEvaluator(cat, device="cpu", dtype=torch.float16)
    user = torch.randn(2, 16, generator=g)
    for call in (lambda: ev.evaluate(user, torch.tensor([0, 1])), lambda: ev.scores(user)):
        with pytest.raises(ValueError) as e:
            call()
        assert "retrieve()" in str(e.value)

    # an unknown scorer raises before the library is touched
    def no_library():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_library)
    for bad in ("tensor", "MFMA", 2):
        with pytest.raises(ValueError):
            ev.retrieve(user, k=3, scorer=bad)
        with pytest.raises(ValueError):
            hip.catalog_select(user, ev.catalog, 3, scorer=bad)

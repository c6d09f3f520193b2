"""CPU: the case tables of tests/train_memory_cases.py reach every kernel, tile, epilogue and mode the GEMM, attention and LoRA memory
modules promise to run -- asked of ur_gemm_plan, ur_attn_plan and ur_lora_plan themselves (no device, nothing is launched) on fake non-null
pointers of the alignment each row states.  A plan answer named in the requirement lists without a row fails here, and so does a row whose
stated plan is not the library's answer: a kernel added later cannot stay outside the memory modules unnoticed."""
import pytest

from tests import train_memory_cases as tm


def _names(table):
    names = [c["name"] for c in table]
    assert len(names) == len(set(names)), "row names are unique"
    return names


# ---- GEMM -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names(tm.GEMM_CASES))
def test_gemm_rows_state_the_librarys_plan(name):
    c = next(c for c in tm.GEMM_CASES if c["name"] == name)
    assert tm.gemm_plan_of(c) == c["plan"], name
    for i in range(len(c["grouped"] or [0])):
        ops = tm.gemm_operands(c, i if c["grouped"] else None)
        ptr = tm.fake_pointers(ops)
        for op in ops:
            assert ptr[op.name] % 256 == op.align and op.align in (4, 8, 16)
            assert op.ld is None or op.ld >= op.width
    if c["pers_mode"] == 0:
        assert tm.gemm_twin(c)["plan"][0] == "persistent"


def test_gemm_table_reaches_every_kernel():
    assert tm.missing(tm.gemm_required(), tm.GEMM_CASES) == []


def test_gemm_check_bites():
    """deleting any one row leaves a requirement unmet (a bit-identity pair loses its twin with the persistent row it mirrors)"""
    req = tm.gemm_required()
    for i, c in enumerate(tm.GEMM_CASES):
        cut = tm.GEMM_CASES[:i] + tm.GEMM_CASES[i + 1:]
        assert tm.missing(req, cut), f"deleting {c['name']} went unnoticed"
    assert tm.missing({**req, "a kernel nobody has written yet": lambda c: c["plan"][0] == "brand_new"}, tm.GEMM_CASES) == ["a kernel nobody has written yet"]


# ---- LoRA -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names(tm.LORA_CASES))
def test_lora_rows_state_the_librarys_plan(name):
    c = next(c for c in tm.LORA_CASES if c["name"] == name)
    if c["plan"] is not None:
        assert tm.lora_plan_of(c) == c["plan"], name


def test_lora_table_reaches_every_kernel():
    assert tm.missing(tm.lora_required(), tm.LORA_CASES) == []


def test_lora_check_bites():
    req = tm.lora_required()
    for i, c in enumerate(tm.LORA_CASES):
        assert tm.missing(req, tm.LORA_CASES[:i] + tm.LORA_CASES[i + 1:]), f"deleting {c['name']} went unnoticed"
    assert tm.missing({**req, "a kernel nobody has written yet": lambda c: (c["plan"] or ("",))[0] == "brand_new"}, tm.LORA_CASES)


# ---- attention --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names(tm.ATTN_CASES))
def test_attention_rows_state_the_librarys_plan(name):
    c = next(c for c in tm.ATTN_CASES if c["name"] == name)
    assert tm.attn_plan_of(c) == c["plan"], name


def test_attention_table_reaches_every_kernel():
    assert tm.missing(tm.attn_required(), tm.ATTN_CASES) == []


def test_attention_check_bites():
    req = tm.attn_required()
    for i, c in enumerate(tm.ATTN_CASES):
        assert tm.missing(req, tm.ATTN_CASES[:i] + tm.ATTN_CASES[i + 1:]), f"deleting {c['name']} went unnoticed"
    assert tm.missing({**req, "a kernel nobody has written yet": lambda c: c["plan"][0] == "brand_new"}, tm.ATTN_CASES)

"""CPU: which kernel every launch of ur_lora_project / ur_lora_reduce / ur_lora_bgrad takes, on which grid, with which token split and
workspace, as the library's one selection function answers it (ur_lora_plan -> hip.lora_plan; no device, nothing is launched).  The
smallest shapes on each side of every selection boundary, at explicit CU counts (256 and 8, so that the CU-dependent rules move); both
workspace queries are the plan's answer; the host-side restatements of a library rule (qwen3.lora_rank_rule's bits_t,
qwen3.lora_bits_t_sizes) are held to it; every case of tests/lora_cases.py reaches the kernel its label names; the query refuses what
the entry points refuse."""
import ctypes
import types

import pytest

from tests import lora_cases as L
from unirec_amd import _lib, hip, qwen3

ADDR = 4096      # an aligned non-null address: the query follows no pointer
CUS = (256, 8)
RANGES = [(0, 64), (64, 128), (192, 64)]      # column ranges, every width % 64 == 0


def plan(op, *a, cu_count=256, **k):
    return hip.lora_plan(op, *a, cu_count=cu_count, **k)


def kernel(op, *a, **k):
    return plan(op, *a, **k)["kernel"]


# =============================================================================================================================
# project
def test_project_ring_boundaries():
    """ring: rank 16, one adapter or column ranges, every width % 64 == 0 -- W = 64 is taken, 72 is not; ranks 8, 32, 64 and 2 .. 4
    adapters that share X never are; the CU count plays no part"""
    for cu in CUS:
        for masked in (False, True):
            assert plan("project", 300, 64, 16, 1, masked=masked, cu_count=cu) == dict(
                kernel="ring", masked=masked, nad_k=1, blocks=1, half=False, splits=1, tok_per_block=256, grid=(2, 1, 1),
                lds_bytes=plan("project", 1, 64, cu_count=cu)["lds_bytes"], workspace_bytes=0)
            assert kernel("project", 300, 72, 16, 1, masked=masked, cu_count=cu) == "staged"
        assert plan("project", 257, cols=RANGES, cu_count=cu)["grid"] == (2, 3, 1) and kernel("project", 257, cols=RANGES, cu_count=cu) == "ring"
        assert kernel("project", 257, cols=[(0, 64), (64, 72)], cu_count=cu) == "staged"
        for rank in (8, 32, 64):
            assert kernel("project", 300, 64, rank, 1, cu_count=cu) == "staged" and kernel("project", 300, rank=rank, cols=RANGES, cu_count=cu) == "staged"
        for nad in (2, 3, 4):
            assert kernel("project", 300, 64, 16, nad, cu_count=cu) == "staged"
    assert plan("project", 1, 64)["lds_bytes"] > 64 * 1024      # (the ring raises the kernel's dynamic-LDS limit)


@pytest.mark.parametrize("rank,blocks,half", [(8, 1, True), (16, 1, False), (32, 2, False), (64, 4, False)])
def test_project_staged_instantiation_and_grid(rank, blocks, half):
    """blocks / half per rank; adapters that share X run in one workgroup (nad_k = nad, grid y = 1), column ranges one adapter per
    workgroup row; 64 tokens per workgroup when nad_k * rank > 192 (four rank-64 adapters, and only they, among these ranks: 3 x 64 = 192 is not), else 128"""
    for nad in (1, 2, 3, 4):
        p = plan("project", 300, 72, rank, nad, masked=True)
        tok = 64 if nad * rank > 192 else 128
        assert (p["kernel"], p["masked"], p["blocks"], p["half"], p["lds_bytes"]) == ("staged", True, blocks, half, 0)
        assert (p["nad_k"], p["tok_per_block"], p["grid"]) == (nad, tok, (-(-300 // tok), 1, 1))
    p = plan("project", 300, rank=rank, cols=L.STAGED_COLS)
    assert (p["kernel"], p["nad_k"], p["tok_per_block"], p["grid"], p["blocks"], p["half"]) == ("staged", 1, 128, (3, 3, 1), blocks, half)
    assert {(nad, r) for nad in (1, 2, 3, 4) for r in hip.LORA_RANKS if plan("project", 64, 72, r, nad)["tok_per_block"] == 64} == {(4, 64)}


# =============================================================================================================================
# reduce
def test_reduce_ring_boundaries():
    """ring: rank 16, M % 128 == 0 (128 is taken; 127, 129 and 136 are not), every width % 64 == 0"""
    for cu in CUS:
        for nad in (1, 2, 3, 4):
            assert kernel("reduce", 128, 64, 16, nad, cu_count=cu) == "ring"
            for M in (127, 129, 136):
                assert kernel("reduce", M, 64, 16, nad, cu_count=cu) == "staged"
            assert kernel("reduce", 128, 72, 16, nad, cu_count=cu) == "staged"
        assert kernel("reduce", 128, cols=RANGES, cu_count=cu) == "ring" and kernel("reduce", 128, cols=[(0, 64), (64, 72)], cu_count=cu) == "staged"
        for rank in (8, 32, 64):
            assert kernel("reduce", 128, 64, rank, 1, cu_count=cu) == "staged" and kernel("reduce", 128, 64, rank, 3, masked=True, bits_t=True, cu_count=cu) == "staged"
    p = plan("reduce", 128, 64, 16, 3)
    assert (p["nad_k"], p["grid"], p["splits"], p["workspace_bytes"]) == (3, (1, 1, 1), 1, 0) and p["lds_bytes"] > 0
    assert plan("reduce", 128, cols=RANGES)["grid"] == (2, 1, 3) and plan("reduce", 128, cols=RANGES)["nad_k"] == 1


def test_reduce_masked_ring_needs_the_token_packed_flags():
    """a masked launch is ring only with drop_bits_t present, 16-byte aligned, bits_t_ld % 4 == 0 and >= width[0], bits_t_stride % 4 == 0;
    failing any one of these is no refusal: the register-staged kernel runs"""
    M, W = 256, 64
    assert kernel("reduce", M, W, 16, 2, masked=True, bits_t=True) == "ring" and plan("reduce", M, W, 16, 2, masked=True, bits_t=True)["masked"]
    assert kernel("reduce", M, W, 16, 2, masked=True) == "staged"
    for broken in (dict(drop_bits_t=ADDR + 4), dict(drop_bits_t=ADDR + 8), dict(bits_t_ld=W + 2), dict(bits_t_ld=W - 4), dict(bits_t_stride=W * 8 + 2)):
        p = plan("reduce", M, W, 16, 2, masked=True, bits_t=True, **broken)
        assert (p["kernel"], p["masked"]) == ("staged", True), broken
    assert kernel("reduce", M, W, 16, 2, masked=True, bits_t=True, bits_t_ld=W + 4, bits_t_stride=(W + 4) * 8) == "ring"
    assert kernel("reduce", M, W, 16, 2, drop_bits_t=ADDR + 4) == "ring"      # (no dropout: the token-packed flags are not looked at)


def test_reduce_splits():
    """M <= 128: one split, no slab sum, no workspace.  M = 300 (tests/lora_cases.reduce_staged): three splits of one 128-token tile.
    Never more than 256 splits.  The ring is sized for two rounds of its workgroups: 2 per CU, 4 per CU for adapters that share X"""
    for rank in hip.LORA_RANKS:
        for M in (1, 127, 128):
            p = plan("reduce", M, 72, rank, 2)
            assert (p["splits"], p["tok_per_block"], p["workspace_bytes"], p["grid"]) == (1, 128, 0, (2, 1, 1))
        p = plan("reduce", 300, 72, rank, 2)
        assert (p["splits"], p["tok_per_block"], p["grid"], p["workspace_bytes"]) == (3, 128, (2, 3, 1), 3 * 2 * rank * 72 * 4)
    # 2048 workgroups over the column blocks: 512 tiles and one column block ask for 2048 splits -> 256 of two tiles; 16 column blocks -> 128
    for cu in CUS:
        p = plan("reduce", 65536, 64, 8, 1, cu_count=cu)
        assert (p["kernel"], p["splits"], p["tok_per_block"], p["grid"]) == ("staged", 256, 256, (1, 256, 1))
        assert plan("reduce", 65536, 1024, 8, 1, cu_count=cu)["splits"] == 128
        assert plan("reduce", 128 * 257, 64, 8, 1, cu_count=cu)["splits"] == 129      # (257 tiles in splits of two)
    # ring, 64 tiles, one column block, 8 CUs: 2 x 8 splits for one adapter, 4 x 8 for adapters that share X, 2 x 8 / 2 column blocks for ranges
    assert plan("reduce", 8192, 64, 16, 1, cu_count=8)["splits"] == 16
    assert plan("reduce", 8192, 64, 16, 2, cu_count=8)["splits"] == 32 and plan("reduce", 8192, 64, 16, 2, cu_count=8)["tok_per_block"] == 256
    assert plan("reduce", 8192, cols=[(0, 64), (64, 64)], cu_count=8)["splits"] == 8
    assert [plan("reduce", 8192, 64, 16, nad, cu_count=256)["splits"] for nad in (1, 2)] == [64, 64]      # (256 CUs: every tile its own split)
    assert plan("reduce", 128 * 1024, 64, 16, 1, cu_count=304)["splits"] == 256


def _sweep_args():
    for rank in hip.LORA_RANKS:
        for M in (0, 1, 128, 300, 384, 1024, 4096, 65536):
            for W in (8, 64, 72, 200, 1024):
                for nad in (1, 2, 3, 4):
                    for masked, bits_t in ((False, False), (True, False), (True, True)):
                        yield hip.lora_plan_args(M, W, rank, nad, masked=masked, bits_t=bits_t)
            for cols in (RANGES, L.STAGED_COLS, L.RING_1024_COLS):
                yield hip.lora_plan_args(M, rank=rank, cols=cols, transposed=True)


def test_workspace_queries_are_the_plan():
    """ur_lora_reduce_workspace_bytes / ur_lora_bgrad_workspace_bytes == the plan's workspace_bytes at cu_count = 0 (what the launch uses);
    M = 0 answers kernel none with no workspace"""
    lib, n = _lib.load(), 0
    for a in _sweep_args():
        p = hip.lora_plan("reduce", a)
        assert p["workspace_bytes"] == lib.ur_lora_reduce_workspace_bytes(ctypes.byref(a))
        assert (p["workspace_bytes"] > 0) == (p["splits"] > 1) and (p["kernel"] == "none") == (a.M == 0)
        if not a.shared:
            p = hip.lora_plan("bgrad", a)
            assert p["workspace_bytes"] == lib.ur_lora_bgrad_workspace_bytes(ctypes.byref(a))
            assert (p["kernel"] == "none") == (a.M == 0) and (a.M == 0) == (p["workspace_bytes"] == 0)
        if a.M == 0:
            assert hip.lora_plan("project", a) == dict(kernel="none", masked=False, nad_k=0, blocks=0, half=False, splits=0, tok_per_block=0,
                                                       grid=(0, 0, 0), lds_bytes=0, workspace_bytes=0)
        n += 1
    assert n > 2000
    # the queries answer 0, not an error, where there is nothing to plan
    for bad in (dict(nad=0), dict(nad=5), dict(rank=24), dict(M=-1)):
        a = _args(**bad)
        assert lib.ur_lora_reduce_workspace_bytes(ctypes.byref(a)) == 0 and lib.ur_lora_bgrad_workspace_bytes(ctypes.byref(a)) == 0


# =============================================================================================================================
# bgrad
def test_bgrad_kernels():
    """register-staged: 512 tokens per block, 256 at rank 64; ring only at rank 16 with every width % 64 == 0; splits = grid x = the
    slabs, always summed; the workspace holds the slabs of the register-staged block count"""
    for cu in CUS:
        for rank, tok in ((8, 512), (16, 512), (32, 512), (64, 256)):
            p = plan("bgrad", 1000, rank=rank, cols=L.BGRAD_STAGED_COLS, cu_count=cu)
            assert (p["kernel"], p["tok_per_block"], p["splits"], p["grid"]) == ("staged", tok, -(-1000 // tok), (-(-1000 // tok), 2, 1))
            assert p["workspace_bytes"] == p["splits"] * rank * (72 + 64) * 4 and p["lds_bytes"] > 0
            assert (p["blocks"], p["half"], p["masked"], p["nad_k"]) == (max(rank // 16, 1), rank == 8, False, 1)
            assert kernel("bgrad", 1000, rank=rank, cols=RANGES, cu_count=cu) == ("ring" if rank == 16 else "staged")
    p = plan("bgrad", 1100, cols=RANGES)
    assert (p["kernel"], p["tok_per_block"], p["splits"], p["grid"], p["workspace_bytes"]) == ("ring", 512, 3, (3, 3, 1), 3 * 16 * 256 * 4)


@pytest.mark.parametrize("cu", [8, 256])
def test_bgrad_ring_1024_from_the_cu_count(cu):
    """ring1024 exactly when ceil(M / 1024) * nad >= cu_count: four adapters, the last M below and the first M at the boundary"""
    blocks = -(-cu // 4)
    below, at = (blocks - 1) * 1024, (blocks - 1) * 1024 + 1
    assert kernel("bgrad", below, cols=L.RING_1024_COLS, cu_count=cu) == "ring"
    p = plan("bgrad", at, cols=L.RING_1024_COLS, cu_count=cu)
    assert (p["kernel"], p["tok_per_block"], p["splits"], p["grid"]) == ("ring1024", 1024, blocks, (blocks, 4, 1))
    assert p["workspace_bytes"] == -(-at // 512) * 16 * 256 * 4      # (sized for the 512-token slabs)
    assert kernel("bgrad", at, cols=L.RING_1024_COLS, cu_count=cu + 1) == "ring"
    assert kernel("bgrad", at, rank=32, cols=L.RING_1024_COLS, cu_count=cu) == "staged"
    assert L.bgrad_ring_1024_rows(cu) == at + 37


# =============================================================================================================================
# host-side restatements of a library rule
def test_model_side_rules_are_the_plans():
    """qwen3.lora_rank_rule(r)["bits_t"] (all switches on) == "a ring-eligible masked reduce with token-packed flags answers ring";
    qwen3.lora_bits_t_sizes == the sizes at which it does, one value on each side of M % 128 and W % 64"""
    on = types.SimpleNamespace(merge_proj=True, fuse_norm_lora=True, fuse_swiglu_lora=True, bits_t=True)
    for r in hip.LORA_RANKS:
        for nad in (1, 3):
            assert qwen3.lora_rank_rule(r, on)["bits_t"] == (kernel("reduce", 128, 64, r, nad, masked=True, bits_t=True) == "ring")
    for M, W in ((128, 64), (256, 1024), (160, 64), (128, 96), (128, 72), (96, 64)):
        assert qwen3.lora_bits_t_sizes(M, W) == (kernel("reduce", M, W, 16, 3, masked=True, bits_t=True) == "ring"), (M, W)
    assert qwen3.lora_bits_t_sizes(M=256) and not qwen3.lora_bits_t_sizes(M=160) and qwen3.lora_bits_t_sizes(W=3072) and not qwen3.lora_bits_t_sizes(W=96)


# =============================================================================================================================
# refusals
OPS = ("project", "reduce", "bgrad")


def _args(ranges=False, masked=False, **fields):
    """valid arguments of 256 tokens (three column ranges, or two adapters that share 64 columns) with `fields` overwritten"""
    a = hip.lora_plan_args(256, cols=RANGES) if ranges else hip.lora_plan_args(256, 64, 16, 2, masked=masked)
    for name, v in fields.items():
        setattr(a, name, v)
    return a


def _refused(op, match, ranges=False, **fields):
    with pytest.raises(_lib.UniRecHipError, match=match):
        hip.lora_plan(op, _args(ranges or op == "bgrad", **fields), cu_count=256)


def test_the_query_refuses_what_the_entry_points_refuse():
    for op in OPS:
        who = f"ur_lora_{op}"
        for rank in (4, 24):
            _refused(op, rf"{who}: the LoRA kernels are built for the ranks 8, 16, 32 and 64 \(got {rank}\)", rank=rank)
        for nad in (0, 5):
            _refused(op, rf"{who}: M >= 0 and 1 <= nad <= 4 required \(M=256 nad={nad}\)", nad=nad)
        _refused(op, f"{who}: M >= 0 and 1 <= nad <= 4", M=-1)
        _refused(op, f"{who}: X must be 16-byte aligned", X=ADDR + 8)
        _refused(op, f"{who}: X must be 16-byte aligned", X=0)
        _refused(op, f"{who}: entry 1 column range", ranges=True, width=(ctypes.c_int * 4)(64, 60, 64, 0))
    for op in ("project", "bgrad"):
        who = f"ur_lora_{op}"
        _refused(op, rf"{who}: U\[1\] must be a 16-byte aligned", U=(ctypes.c_void_p * 4)(ADDR, ADDR + 8, ADDR, ADDR))
        _refused(op, f"{who}: P must be 8-byte aligned", P=ADDR + 4)
        _refused(op, f"{who}: P must be 8-byte aligned, ldp % 4 == 0, ldp >= rank nad", ldp=16)
    for op in ("reduce", "bgrad"):
        who = f"ur_lora_{op}"
        _refused(op, f"{who}: V must be a 16-byte aligned", V=ADDR + 8)
        _refused(op, f"{who}: V must be a 16-byte aligned", ldv=16)
        _refused(op, f"{who}: G must be 16-byte aligned", G=ADDR + 8)
    _refused("bgrad", "ur_lora_bgrad: adapters own column ranges of X \\(shared = 0\\), no dropout planes", shared=1)
    _refused("bgrad", "ur_lora_bgrad: dropout bit planes need adapters that share their input", drop_bits=ADDR, bits_ld=16, bits_stride=16 * 256)
    with pytest.raises(_lib.UniRecHipError, match="no dropout planes"):
        hip.lora_plan("bgrad", _args(masked=True))
    _refused("reduce", "ur_lora_reduce: dropout bit planes need adapters that share their input", ranges=True, drop_bits=ADDR, bits_ld=16, bits_stride=4096)
    _refused("project", "ur_lora_project: bit planes need 16-byte aligned rows", masked=True, drop_bits=ADDR + 8)
    for op in (3, -1):
        with pytest.raises(_lib.UniRecHipError, match=f"ur_lora_plan: unknown op {op}"):
            hip.lora_plan(op, 256, 64)
    with pytest.raises(_lib.UniRecHipError, match="ur_lora_plan: null plan or negative cu_count"):
        hip.lora_plan("reduce", 256, 64, cu_count=-1)
    lib, a = _lib.load(), hip.lora_plan_args(256, 64)
    assert lib.ur_lora_plan(0, ctypes.byref(a), 0, None) == -1 and lib.ur_lora_plan(0, None, 0, ctypes.byref(_lib.LoraPlanInfo())) == -1


# =============================================================================================================================
# every case of tests/lora_cases.py reaches the kernel its label names
def _generators():
    for rank in L.RANKS:
        for nad in (1, 2, 3, 4):
            yield "project", L.project_staged(rank, nad), {}
            yield "reduce", L.reduce_staged(rank, nad), {}
        yield "project", L.project_ranges(rank), {}
        yield "reduce", L.reduce_ranges(rank), {}
        yield "bgrad", L.bgrad_staged(rank), {}
    yield "project", L.project_ring(), {}
    for nad in (1, 2, 3, 4):
        yield "reduce", L.reduce_ring(nad), dict(bits_t=True)                  # (test_gpu_lora_f64 hands these the token-packed flags)
        yield "reduce", L.reduce_ring_fallback(nad), {}
    yield "reduce", L.reduce_ring_ranges(), {}
    yield "bgrad", L.bgrad_ring_512(), {}
    for cu in (8, 64):
        yield "bgrad", L.bgrad_ring_1024(cu), dict(cu_count=cu)


def test_every_case_reaches_the_kernel_its_label_names():
    """at 256 CUs (bgrad_ring_1024: at the CU count the case was built for), by the case's sizes, row stride and planes"""
    n, seen = 0, set()
    for op, cases, kw in _generators():
        for c in cases:
            assert c["path"].startswith(op + "/")
            got = L.plan_of(op, c, **{"cu_count": 256, **kw})
            assert got["kernel"] == L.kernel_of(c["path"]), (c["path"], c["M"], c["W"], c["rank"], c["nad"], got)
            assert got["masked"] == (c["keep"] is not None)
            seen.add((op, got["kernel"]))
            n += 1
    assert n > 2500
    assert seen == {("project", "staged"), ("project", "ring"), ("reduce", "staged"), ("reduce", "ring"), ("bgrad", "staged"), ("bgrad", "ring"), ("bgrad", "ring1024")}
    assert [L.kernel_of(p) for p in ("project/staged ranges", "reduce/staged (no bits_t)", "bgrad/ring 512", "bgrad/ring 1024")] == ["staged", "staged", "ring", "ring1024"]

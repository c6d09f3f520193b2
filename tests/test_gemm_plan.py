"""CPU: which kernel every launch of ur_gemm / ur_gemm_grouped takes, on which tile, with which epilogue instantiation and tile order,
as the library's one selection function answers it (ur_gemm_plan -> hip.gemm_plan; no device, nothing is launched).  The smallest shapes
on each side of every selection boundary under both ur_gemm_persistent_mode settings; every persistent instantiation is reached; the two
*_supported queries are the plan's answer; the host-side constants that restate a library rule (qwen3.PERS_GEMM_K2_MAX, the splits of
qformer._split_k_for) are held to it; the query refuses what the entry points refuse."""
import ctypes
import itertools

import pytest

from unirec_amd import _lib, hip

ADDR = 4096      # an aligned non-null address: the query follows no pointer
TN = dict(r_kcontig=False, s_kcontig=False, out_f32=True)      # token-major operands, f32 output: the weight-gradient products


class _mode:
    """with _mode(0): ...   -- ur_gemm_persistent_mode set and restored"""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.prev = hip.gemm_persistent_mode(self.mode)

    def __exit__(self, *exc):
        hip.gemm_persistent_mode(self.prev)
        return False


def _kernel(*a, **k):
    return hip.gemm_plan(*a, **k)["kernel"]


def _both_modes(*a, **k):
    """(kernel with the persistent kernel off, kernel with it on)"""
    out = []
    for mode in (0, 1):
        with _mode(mode):
            out.append(_kernel(*a, **k))
    return tuple(out)


TAKEN, NOT_TAKEN = ("generic", "persistent"), ("generic", "generic")


def test_persistent_size_boundaries():
    """2048 x 4096 x 256 is the smallest launch taken: 128 tiles, K = 4 K tiles.  112 tiles, K below 256 (192 is a multiple of 64), K off
    the 64 grid (288), M or N off the 256 grid and a row stride of C off the 8-element grid each leave it on the generic kernel; K = 320
    (5 K tiles) stays.  A C that is not 16-byte aligned is no launch at all."""
    assert _both_modes(2048, 4096, 256) == TAKEN
    assert hip.gemm_plan(2048, 4096, 256) == dict(kernel="persistent", tile=256, epi=0, mode=0, gcw=4, splits=1)
    assert _both_modes(1792, 4096, 256) == NOT_TAKEN and _both_modes(4096, 2048, 256) == TAKEN
    assert _both_modes(2048, 4096, 192) == NOT_TAKEN and _both_modes(2048, 4096, 288) == NOT_TAKEN
    assert _both_modes(2048, 4096, 320) == TAKEN
    assert _both_modes(2048 + 8, 4096, 256) == NOT_TAKEN and _both_modes(2048, 4096 + 8, 256) == NOT_TAKEN
    assert _both_modes(2048, 4096, 256, ldc=4096 + 4) == NOT_TAKEN and _both_modes(2048, 4096, 256, ldc=4096 + 8) == TAKEN
    with pytest.raises(_lib.UniRecHipError, match="16-byte aligned"):
        hip.gemm_plan(2048, 4096, 256, C=ADDR + 8)
    # K-strided operands, an f32 output and split_k stay off it
    for kw in (dict(r_kcontig=False), dict(s_kcontig=False), dict(out_f32=True), dict(out_f32=True, split_k=2)):
        assert _both_modes(2048, 4096, 256, **kw) == NOT_TAKEN, kw
    # the SwiGLU forward epilogue is the generic kernel's (a bias or residual beside the SwiGLU backward is no launch: ur_gemm refuses it)
    assert _both_modes(2048, 4096, 256, swiglu_gate=True, swiglu_act=True) == NOT_TAKEN
    assert _both_modes(2048, 4096, 256, swiglu_gu=True, swiglu_dgu=True) == TAKEN
    # the GELU epilogues alone
    assert _both_modes(2048, 4096, 256, gelu_out=True, bias=True) == TAKEN and _both_modes(2048, 4096, 256, gelu_grad_aux=True) == TAKEN
    for kw in (dict(gelu_out=True, gelu_grad_aux=True), dict(gelu_out=True, residual=True), dict(gelu_grad_aux=True, K2=16)):
        assert _both_modes(2048, 4096, 256, **kw) == NOT_TAKEN, kw


def test_second_k_range_boundary_is_the_hosts_constant():
    """qwen3.PERS_GEMM_K2_MAX is the library's rule: a second K range of that width rides in the persistent kernel's K stream, 8 more do not"""
    from unirec_amd.qwen3 import PERS_GEMM_K2_MAX
    assert PERS_GEMM_K2_MAX == 64
    assert _both_modes(2048, 4096, 256, PERS_GEMM_K2_MAX) == TAKEN
    assert hip.gemm_plan(2048, 4096, 256, PERS_GEMM_K2_MAX)["mode"] == 1
    assert _both_modes(2048, 4096, 256, PERS_GEMM_K2_MAX + 8) == NOT_TAKEN


def test_masked_launch_boundaries():
    """the masked LoRA epilogue of the persistent kernel is rank 16 only (also four adapters: K2 = 64, and past the unmasked K2 limit never),
    up to K = 8192"""
    assert _both_modes(2048, 4096, 256, 16, drop_rank=16) == TAKEN and hip.gemm_plan(2048, 4096, 256, 16, drop_rank=16)["mode"] == 2
    assert _both_modes(2048, 4096, 256, 64, drop_rank=16) == TAKEN
    assert _both_modes(2048, 4096, 256, 8, drop_rank=8) == NOT_TAKEN and _both_modes(2048, 4096, 256, 32, drop_rank=32) == NOT_TAKEN
    assert _both_modes(2048, 4096, 256, 128, drop_rank=32) == NOT_TAKEN
    assert _both_modes(2048, 4096, 8192, 16, drop_rank=16) == TAKEN and _both_modes(2048, 4096, 8256, 16, drop_rank=16) == NOT_TAKEN
    assert _both_modes(2048, 4096, 8256, 16) == TAKEN      # (the limit is the masked epilogue's)


QKR = dict(qkr_q=True, qkr_k=True, qkr_v=True, qkr_rstd=True, qkr_qw=True, qkr_kw=True, qkr_cos=True, qkr_sin=True, qkr_ldq=2048, qkr_ldk=1024,
           qkr_ldv=1024, qkr_S=256, qkr_nq_cols=2048, qkr_nk_cols=1024)
SWP = dict(swp_act=True, swp_ldact=2048, swp_I=2048)
EPILOGUES = {0: {}, 1: dict(swiglu_gu=True, swiglu_dgu=True), 2: dict(residual=True, bias=True), 3: QKR, 4: SWP, 5: dict(bias=True),
             6: dict(gelu_out=True), 7: dict(gelu_grad_aux=True)}
SECOND = {0: {}, 1: dict(K2=48), 2: dict(K2=16, drop_rank=16)}
PERS_INSTANCES = {(e, m) for e in (0, 1, 2, 5) for m in (0, 1, 2)} | {(3, 0), (3, 1), (4, 0), (4, 1), (6, 0), (7, 0)}


def test_every_persistent_instantiation_is_reached():
    """the 18 gemm_pers_kernel<EPI, MODE> of gemm_pers_launch, each by the arguments that select it; the other six combinations are either
    refused (the q/k-norm + RoPE and paired SwiGLU epilogues take no masked range) or run on the generic kernel (GELU with a second range)"""
    assert len(PERS_INSTANCES) == 18
    seen = set()
    for (e, ekw), (m, mkw) in itertools.product(EPILOGUES.items(), SECOND.items()):
        try:
            pl = hip.gemm_plan(2048, 4096, 256, **ekw, **mkw)
        except _lib.UniRecHipError:
            assert (e, m) in ((3, 2), (4, 2))
            continue
        if pl["kernel"] == "persistent":
            assert (pl["epi"], pl["mode"], pl["tile"], pl["splits"]) == (e, m, 256, 1), (e, m, pl)
            seen.add((e, m))
        else:
            assert pl["kernel"] == "generic" and e in (6, 7) and m > 0, (e, m, pl)
    assert seen == PERS_INSTANCES
    assert hip.gemm_plan(2048, 4096, 256, residual=True)["epi"] == 2


LAYOUTS = [(True, True), (True, False), (False, False), (False, True)]


@pytest.mark.parametrize("rk,sk", LAYOUTS)
def test_generic_tile_boundary(rk, sk):
    """256 x 256 from M, N >= 256 and 256 workgroups on -- 224 when both operands are K-strided -- at the shapes of
    tests/test_gpu_norm_f64.py:_big_tile_shape and at one tile row; K = 72 keeps the K-contiguous launches off the persistent kernel"""
    wgs = 224 if (not rk and not sk) else 256
    tile = lambda M, N, **kw: hip.gemm_plan(M, N, 72, r_kcontig=rk, s_kcontig=sk, **kw)      # noqa: E731
    big = (wgs // 2 - 1) * 256 + 8
    for mode in (0, 1):
        with _mode(mode):
            assert tile(264, big) == dict(kernel="generic", tile=256, epi=0, mode=0, gcw=0, splits=1)
            assert tile(264, big - 8)["tile"] == 128 and tile(248, big)["tile"] == 128 and tile(big, 248)["tile"] == 128
            assert tile(256, wgs * 256)["tile"] == 256 and tile(256, (wgs - 1) * 256)["tile"] == 128
            assert tile(256, (wgs - 1) * 256 + 8)["tile"] == 256
            # split_k multiplies the count (f32 output)
            assert tile(264, 520, out_f32=True, split_k=-(-wgs // 6))["tile"] == 256
            assert tile(264, 520, out_f32=True, split_k=-(-wgs // 6) - 1)["tile"] == 128


def test_generic_epilogue_instantiations():
    """EPI 1 / 2 = the SwiGLU backward / forward epilogue, on both tiles"""
    for M, N, t in ((264, 127 * 256 + 8, 256), (264, 520, 128)):
        assert hip.gemm_plan(M, N, 72, swiglu_gu=True, swiglu_dgu=True) == dict(kernel="generic", tile=t, epi=1, mode=0, gcw=0, splits=1)
        assert hip.gemm_plan(M, N, 72, swiglu_gate=True, swiglu_act=True, bias=True)["epi"] == 2
        assert hip.gemm_plan(M, N, 72, bias=True, residual=True, gelu_out=True, K2=72)["epi"] == 0


@pytest.mark.parametrize("gn,pers,generic", [(12, 0, 0), (16, 4, 4), (18, 0, 0), (20, 4, 4), (24, 6, 4), (30, 6, 0), (36, 6, 4), (48, 6, 4)])
def test_column_chunk_rules(gn, pers, generic):
    """gcw of both kernels by tile columns: from 16 columns on when they are a multiple of the width -- the persistent kernel's width is 6
    for multiples of 6 from 24 on, else 4; the generic kernel's is 4 -- and the tile rows of 8.  gm = 24 / 28 keeps every generic launch
    on the 256 tile (>= 288 workgroups) and every persistent one above 128 tiles."""
    N = gn * 256
    for gm, whole in ((24, True), (28, False)):
        M = gm * 256
        pl = hip.gemm_plan(M, N, 256)
        assert (pl["kernel"], pl["gcw"]) == ("persistent", pers if whole else 0), (gm, pl)
        with _mode(0):
            pl = hip.gemm_plan(M, N, 256)
        assert (pl["kernel"], pl["tile"], pl["gcw"]) == ("generic", 256, generic if whole else 0), (gm, pl)
        pl = hip.gemm_plan(M, N, 72, r_kcontig=False)
        assert (pl["kernel"], pl["tile"], pl["gcw"]) == ("generic", 256, generic if whole else 0), (gm, pl)
    # the 128 tile has no chunks: 16 x 16 tiles of 256 are one round (256 workgroups, chunks), 8 x 16 are 32 x 64 tiles of 128
    assert hip.gemm_plan(4096, 4096, 72)["gcw"] == 4 and hip.gemm_plan(2048, 4096, 72) == dict(kernel="generic", tile=128, epi=0, mode=0, gcw=0, splits=1)


def _group(shapes, K, split):
    return [hip.gemm_plan_args(M, N, K, split_k=split, **TN) for M, N in shapes]


def test_grouped_tile_boundary():
    """the eight 264 x 520 products of tests/test_gpu_dw_f64.py:test_grouped_big_tile_exact are 6 big tiles each: 144 at split 3 (the 256
    tile), 96 at split 2; eight products of 4 big tiles are 128 at split 4 and 96 at split 3; one product below 256 rows keeps the launch
    on the 128 tile"""
    for mode in (0, 1):
        with _mode(mode):
            assert hip.gemm_plan(_group([(264, 520)] * 8, 320, 3)) == dict(kernel="grouped", tile=256, epi=0, mode=0, gcw=0, splits=3)
            assert hip.gemm_plan(_group([(264, 520)] * 8, 320, 2)) == dict(kernel="grouped", tile=128, epi=0, mode=0, gcw=0, splits=2)
            assert hip.gemm_plan(_group([(512, 512)] * 8, 320, 4))["tile"] == 256 and hip.gemm_plan(_group([(512, 512)] * 8, 320, 3))["tile"] == 128
            assert hip.gemm_plan(_group([(264, 520)] * 7 + [(248, 520)], 320, 3))["tile"] == 128
            assert hip.gemm_plan(_group([(1024, 4096)], 320, 1)) == dict(kernel="grouped", tile=128, epi=0, mode=0, gcw=0, splits=1)
            assert hip.gemm_plan(_group([(1024, 4096)], 320, 2))["tile"] == 256


def test_supported_queries_are_the_plans_answer():
    """ur_gemm_qkrope_supported / ur_gemm_swiglu_paired_supported == "ur_gemm_plan accepts the arguments and answers persistent", over
    M x N x K x K2 x S in both modes"""
    lib, out = _lib.load(), _lib.GemmPlanInfo()
    PERSISTENT = hip.GEMM_KERNELS.index("persistent")
    n = {"qkr": 0, "swp": 0}
    grid = itertools.product((1024, 1792, 2048, 2056, 4096), (2048, 4096, 4104, 6144), (192, 256, 288, 1024), (0, 16, 48, 64, 72))
    for (M, N, K, K2), mode in itertools.product(grid, (0, 1)):
        with _mode(mode):
            cases = [("swp", hip.gemm_plan_args(M, N, K, K2, swp_act=True, swp_ldact=N // 2, swp_I=N // 2))]
            for S in (128, 256, 512):
                nq, nk = N // 2 // 256 * 256, N // 4 // 256 * 256
                cases.append(("qkr", hip.gemm_plan_args(M, N, K, K2, **dict(QKR, qkr_S=S, qkr_nq_cols=nq, qkr_nk_cols=nk, qkr_ldq=nq, qkr_ldk=nk,
                                                                             qkr_ldv=N - nq - nk))))
            for which, a in cases:
                fn = lib.ur_gemm_qkrope_supported if which == "qkr" else lib.ur_gemm_swiglu_paired_supported
                ok = lib.ur_gemm_plan(ctypes.byref(a), 0, ctypes.byref(out)) == 0 and out.kernel == PERSISTENT
                assert bool(fn(ctypes.byref(a))) == ok, (which, M, N, K, K2, mode, a.qkr_S)
                assert not ok or mode == 1
                n[which] += ok
    assert n["qkr"] > 0 and n["swp"] > 0
    # the Python wrappers, at the boundaries tests/test_gpu_gemm_persistent.py uses them at
    assert hip.gemm_qkrope_supported(2048, 4096, 1024, 48, 256, 2048, 1024) and not hip.gemm_qkrope_supported(1024, 4096, 1024, 0, 256, 2048, 1024)
    assert hip.gemm_swiglu_paired_supported(2048, 3072, 1024, 32) and not hip.gemm_swiglu_paired_supported(1024, 3072, 1024, 0)
    assert not hip.gemm_swiglu_paired_supported(2048, 3072 + 64, 1024, 32)      # I % 128


@pytest.mark.parametrize("out_rows,out_cols,red", [(768, 3072, 8192), (2304, 768, 8192), (2048, 1024, 32768), (1024, 4096, 32768),
                                                   (3072, 1024, 32768), (1024, 1024, 32768)])
def test_split_k_for_reaches_the_big_tile(out_rows, out_cols, red):
    """qformer._split_k_for is written around ur_gemm's 224 / 256-workgroup thresholds: at the shapes its comments cite, the split it
    picks puts the token reduction on the 256 x 256 tile"""
    from unirec_amd.qformer import _split_k_for
    split = _split_k_for(out_rows, out_cols, red)
    pl = hip.gemm_plan(out_rows, out_cols, red, split_k=split, **TN)
    assert (pl["kernel"], pl["tile"], pl["splits"]) == ("generic", 256, split), (split, pl)


def test_empty_launches_select_nothing():
    assert hip.gemm_plan(0, 4096, 256) == dict(kernel="none", tile=0, epi=0, mode=0, gcw=0, splits=0)
    assert _kernel(2048, 0, 256) == "none"


@pytest.mark.parametrize("args,kw,text", [
    ((-8, 4096, 256), {}, "negative dimension"),
    ((2048, 4096, 260), {}, "multiples of 8 for K-contiguous"),
    ((2048, 4096, 256), dict(split_k=2), "split_k needs f32 output"),
    ((2048, 4096, 256), dict(split_k=2, out_f32=True, ldc=4096 + 4), "split_k needs a dense output"),
    ((2048, 4096, 256, 24), dict(drop_rank=12), "masked LoRA epilogue"),
    ((2048, 4096, 256), dict(R=0), "null operand"),
    ((1024, 4096, 256), QKR, "q/k-norm \\+ RoPE epilogue is not available"),
    ((1024, 4096, 256), SWP, "paired SwiGLU forward epilogue is not available"),
    # the epilogue's f32 operands below the alignment the header states: refused by name, not as "not available"
    ((2048, 4096, 256), dict(QKR, qkr_cos=ADDR + 8), "qkr_qw, qkr_kw, qkr_cos and qkr_sin must be 16-byte aligned"),
    ((2048, 4096, 256), dict(QKR, qkr_kw=ADDR + 4), "qkr_qw, qkr_kw, qkr_cos and qkr_sin must be 16-byte aligned"),
    ((2048, 4096, 256), dict(QKR, qkr_rstd=ADDR + 2), "qkr_rstd must be 4-byte aligned"),
    ((2048, 4096, 256), dict(bias=ADDR + 8), "bias must be 16-byte aligned"),
])
def test_the_query_refuses_what_ur_gemm_refuses(args, kw, text):
    for mode in (0, 1):
        with _mode(mode), pytest.raises(_lib.UniRecHipError, match=text):
            hip.gemm_plan(*args, **kw)


def test_the_query_refuses_what_ur_gemm_grouped_refuses():
    with pytest.raises(_lib.UniRecHipError, match="1 .. 8 products"):
        hip.gemm_plan(_group([(264, 520)] * 9, 320, 1))
    with pytest.raises(_lib.UniRecHipError, match="token-major"):
        hip.gemm_plan([hip.gemm_plan_args(264, 520, 320)])
    g = _group([(264, 520)] * 2, 320, 2)
    g[1].ldc = 528
    with pytest.raises(_lib.UniRecHipError, match="dense output"):
        hip.gemm_plan(g)

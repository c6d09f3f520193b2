"""GPU: the weight-gradient token reductions (ur_gemm with split_k, ur_gemm_grouped) and the field projection of the item Q-Former head,
ELEMENT BY ELEMENT against float64 (tests/ref64.py, checked on the CPU in tests/test_ref64.py; inputs from tests/ew_cases.py).

Criteria (docs/lab_notes.md, "Element-wise float64 tests: AdamW, casts, field projection and split-K"):
  split-K, integer operands in [-3, 3]   bit-equal to the float64 product (every partial sum is an integer below 2^24: exact in any order), on
                         splits whose last run is short (K = 320 / 3, K = 1000 / 16) or EMPTY (K = 256 / 3: 4 tiles in runs of 2, 2, 0)
  ur_gemm_grouped        the same on both tile sizes, and bit for bit one ur_gemm per product where tile and split coincide (the small tile)
  unit-normal operands   K = 4096: ref64.assert_colsum_close with sum |term| = |dy|^T |x|, e32 = a float32 product on the CPU
  output stride          a column view of a wider f32 buffer: exact without split_k with every element outside the view untouched; with
                         split_k > 1 the call is refused (ldc == N is the documented contract) and nothing at all is written
  ur_field_projection_*  out: ref64.assert_f32_close; drec (bf16): 1 ulp + 2^-18 row max + 8 e32_row (ref64.assert_bf16_rows); dWf, dbf:
                         ref64.assert_colsum_close with their sum |term| -- on the Q = 32 fast path dWf receives 2^-9 sum |dout * rec| more, for
                         the bf16 rounding of dout in front of the MFMA (ref64.fproj_fast_dwf_terms); the generic path does not get it
Outputs are pre-filled with a sentinel and followed by guard elements that must keep their bits.  Every test prints its worst error / bound
("[ratio] kernel: x")."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import ew_cases, ref64  # noqa: E402
from unirec_amd import _lib, hip  # noqa: E402
from unirec_amd._lib import UniRecHipError, check  # noqa: E402

# entry point -> the primitive-level tests of this module that hold it against a reference (tests/test_abi_test_coverage.py)
COVERS = {
    "ur_gemm": ["test_gemm_splitk_short_and_empty_runs_exact", "test_output_stride_without_split_is_exact_and_with_split_is_refused"],
    "ur_gemm_grouped": ["test_grouped_small_tile_exact_and_equal_to_ur_gemm", "test_grouped_big_tile_exact", "test_grouped_unit_normal_operands",
                        "test_output_stride_without_split_is_exact_and_with_split_is_refused"],
    "ur_field_projection_fwd": ["test_field_projection_generic", "test_field_projection_fast", "test_field_projection_fast_forward_past_the_grid_cap",
                                "test_field_projection_misaligned_rec_takes_the_generic_kernels"],
    "ur_field_projection_bwd": ["test_field_projection_generic", "test_field_projection_fast", "test_field_projection_misaligned_rec_takes_the_generic_kernels",
                                "test_field_projection_refuses_bad_arguments_without_a_launch"],
}

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GUARD = 64
SENT32 = 0x4B4B4B4B                  # 13323083.0f, NaN-free: nothing here computes it
SENT16 = 0x4B4B
WORST = {}


def _note(kernel, ratio):
    WORST[kernel] = max(WORST.get(kernel, 0.0), float(ratio))
    print(f"[ratio] {kernel}: {float(ratio):.4f}")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _sentinel(shape, dtype=F32):
    """(the output of this shape, its flat backing buffer with GUARD more elements), all filled with the sentinel"""
    n = 1
    for s in shape:
        n *= s
    if dtype == F32:
        base = torch.full((n + GUARD,), SENT32, dtype=torch.int32, device=DEV).view(F32)
    else:
        base = torch.full((n + GUARD,), SENT16, dtype=torch.int16, device=DEV).view(BF16)
    return base[:n].view(*shape), base


def _guard_intact(base, n, what):
    sent = SENT32 if base.element_size() == 4 else SENT16
    assert (_bits(base)[n:] == sent).all(), f"{what}: elements behind the end were written"


def _all_written(out, what):
    sent = SENT32 if out.element_size() == 4 else SENT16
    assert not (_bits(out) == sent).any(), f"{what}: elements left unwritten"


def _tn(K, M, N, seed, pad=0, ints=True):
    """token-major operands (R [K, M], S [K, N], bf16 on the device; pad: a row stride above the row length) and their CPU copies"""
    g = _gen(seed)
    if ints:
        r, s = torch.randint(-3, 4, (K, M + pad), generator=g).to(BF16), torch.randint(-3, 4, (K, N + pad), generator=g).to(BF16)
    else:
        r, s = torch.randn(K, M + pad, generator=g).to(BF16), torch.randn(K, N + pad, generator=g).to(BF16)
    return r.to(DEV)[:, :M], s.to(DEV)[:, :N], r[:, :M], s[:, :N]


# ---- ur_gemm, split_k --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", [(8, 8), (136, 64), (264, 520)])
@pytest.mark.parametrize("K,split", [(256, 3), (320, 3), (1000, 16)])
def test_gemm_splitk_short_and_empty_runs_exact(K, split, M, N):
    runs = [b - a for a, b in ref64.splitk_slices(K, split)]
    assert len(runs) == split and {(256, 3): runs[-1] == 0, (320, 3): runs[-1] == 64, (1000, 16): runs[-1] == 40}[(K, split)]
    R, S, r, s = _tn(K, M, N, K + M)
    out, base = _sentinel((M, N))
    hip.gemm(R, S, r_kcontig=False, s_kcontig=False, out=out, split_k=split)
    torch.cuda.synchronize()
    _guard_intact(base, M * N, "split-K output")
    _note("gemm_kernel + splitk_reduce_kernel", ref64.assert_lora_exact(out, ref64.gemm_tn(r, s), f"K {K} / {split}, {M} x {N}"))


# ---- ur_gemm_grouped ---------------------------------------------------------------------------------------------------------------
def _grouped(shapes, K, split, seed, pad=0, ints=True, shared=False):
    """one grouped launch into sentinel outputs; returns [(R, S, r, s, out)] after checking the guards.  shared: every product reads the
    first product's operands (one reference for all of them)."""
    ops = []
    for i, (M, N) in enumerate(shapes):
        ops.append(ops[0] if shared and i else _tn(K, M, N, seed + i, pad, ints))
    outs = [_sentinel((M, N)) for M, N in shapes]
    hip.gemm_grouped([(o[0], o[1], out) for o, (out, _) in zip(ops, outs)], split_k=split)
    torch.cuda.synchronize()
    for (M, N), (out, base) in zip(shapes, outs):
        _guard_intact(base, M * N, f"grouped output {M} x {N}")
        _all_written(out, f"grouped output {M} x {N}")
    return [(*o, out) for o, (out, _) in zip(ops, outs)]


SMALL_TILE_SHAPES = [(64, 136), (136, 64), (264, 520), (8, 8)]


@pytest.mark.parametrize("split", [1, 3])
def test_grouped_small_tile_exact_and_equal_to_ur_gemm(split):
    """outputs below one big tile, edge tiles in both directions, a ragged last K tile, padded row strides of the inputs"""
    assert hip.gemm_plan([hip.gemm_plan_args(M, N, 1000, r_kcontig=False, s_kcontig=False, out_f32=True, split_k=split) for M, N in SMALL_TILE_SHAPES])["tile"] == 128
    for R, S, r, s, out in _grouped(SMALL_TILE_SHAPES, 1000, split, 100, pad=8):
        M, N = out.shape
        _note("gemm_grouped_kernel<128>", ref64.assert_lora_exact(out, ref64.gemm_tn(r, s), f"split {split}, {M} x {N}"))
        single = hip.gemm(R, S, r_kcontig=False, s_kcontig=False, out_f32=True, split_k=split)
        assert torch.equal(_bits(out), _bits(single)), f"split {split}, {M} x {N}: ur_gemm_grouped and ur_gemm differ"


@pytest.mark.parametrize("K", [320, 256])
def test_grouped_big_tile_exact(K):
    """eight products of 264 x 520: 6 big tiles each, 144 with the split (the 256 x 256 tile; 96 at split 2 would be the small one), edge tiles in both directions;
    K = 320 ends in a short run, K = 256 in an empty one"""
    shapes = [(264, 520)] * 8
    group = lambda split: [hip.gemm_plan_args(M, N, K, r_kcontig=False, s_kcontig=False, out_f32=True, split_k=split) for M, N in shapes]      # noqa: E731
    assert hip.gemm_plan(group(3))["tile"] == 256 and hip.gemm_plan(group(2))["tile"] == 128
    for R, S, r, s, out in _grouped(shapes, K, 3, 200 + K):
        _note("gemm_grouped_kernel<256>", ref64.assert_lora_exact(out, ref64.gemm_tn(r, s), f"K {K}"))


def test_grouped_unit_normal_operands():
    """K = 4096 at split 3 (runs of 22, 22, 20 tiles) on both tile sizes; the big-tile group shares one operand pair, so its eight results
    are also the same bits"""
    K, split = 4096, 3
    small = _grouped(SMALL_TILE_SHAPES, K, split, 300, pad=8, ints=False)
    big = _grouped([(264, 520)] * 8, K, split, 400, ints=False, shared=True)
    for name, group in (("gemm_grouped_kernel<128>", small), ("gemm_grouped_kernel<256>", big[:1])):
        for R, S, r, s, out in group:
            r64, s64 = r.to(F64), s.to(F64)
            ratio = ref64.assert_colsum_close(out, r64.t() @ s64, r.float().t() @ s.float(), r64.abs().t() @ s64.abs(), f"{name} {tuple(out.shape)}")
            _note(name + " (unit-normal)", ratio)
    for R, S, r, s, out in small:
        single = hip.gemm(R, S, r_kcontig=False, s_kcontig=False, out_f32=True, split_k=split)
        assert torch.equal(_bits(out), _bits(single)), f"{tuple(out.shape)}: ur_gemm_grouped and ur_gemm differ"
    for *_, out in big[1:]:
        assert torch.equal(_bits(out), _bits(big[0][-1])), "a product's result depends on its place in the grid"


# ---- output stride -----------------------------------------------------------------------------------------------------------------
def _strided_out(M, N):
    """out = backing[1:-1, 8:8 + N] of a sentinel-filled f32 [M + 2, N + 16]: one guard row above and below, 8 guard columns on either side
    (so a slab-sized write from out's first element ends inside the backing tensor)"""
    backing = torch.full((M + 2, N + 16), SENT32, dtype=torch.int32, device=DEV).view(F32)
    return backing[1:-1, 8:8 + N], backing


def _outside_intact(backing, N, what):
    b = _bits(backing)
    assert (b[0] == SENT32).all() and (b[-1] == SENT32).all() and (b[:, :8] == SENT32).all() and (b[:, 8 + N:] == SENT32).all(), \
        f"{what}: elements outside the output view were written"


@pytest.mark.parametrize("M,N", [(136, 64), (264, 520)])
def test_output_stride_without_split_is_exact_and_with_split_is_refused(M, N):
    K = 320
    R, S, r, s = _tn(K, M, N, 500 + M)
    exact = ref64.gemm_tn(r, s)
    for name, run in (("ur_gemm", lambda o, k: hip.gemm(R, S, r_kcontig=False, s_kcontig=False, out=o, split_k=k)),
                      ("ur_gemm_grouped", lambda o, k: hip.gemm_grouped([(R, S, o)], split_k=k))):
        out, backing = _strided_out(M, N)
        assert out.stride(0) == N + 16 and out.data_ptr() % 16 == 0
        run(out, 1)
        torch.cuda.synchronize()
        ref64.assert_lora_exact(out, exact, f"{name}, ldc = N + 16")
        _outside_intact(backing, N, name)
        out, backing = _strided_out(M, N)
        with pytest.raises((UniRecHipError, ValueError), match="ldc == N"):
            run(out, 2)
        torch.cuda.synchronize()
        assert (_bits(backing) == SENT32).all(), f"{name}: a refused split-K call wrote"
    _note("output stride", 0.0)


# ---- field projection ----------------------------------------------------------------------------------------------------------------
def _fproj_fwd(rec, Wf, bf):
    B, Q, E = rec.shape
    F_ = Wf.shape[0]
    out, base = _sentinel((B, F_, E))
    check(_lib.load().ur_field_projection_fwd(rec.data_ptr(), Wf.data_ptr(), bf.data_ptr(), out.data_ptr(), B, Q, F_, E, hip._stream()), "ur_field_projection_fwd")
    torch.cuda.synchronize()
    _guard_intact(base, B * F_ * E, "field projection out")
    return out


def _fproj_bwd(dout, rec, Wf):
    B, Q, E = rec.shape
    F_ = Wf.shape[0]
    (drec, b0), (dWf, b1), (dbf, b2) = _sentinel((B, Q, E), BF16), _sentinel((F_, Q)), _sentinel((F_,))
    ws, n = hip._heads_ws(Q, F_, rec.device)
    check(_lib.load().ur_field_projection_bwd(dout.data_ptr(), rec.data_ptr(), Wf.data_ptr(), drec.data_ptr(), dWf.data_ptr(), dbf.data_ptr(), B, Q, F_, E,
                                              ws.data_ptr(), n, hip._stream()), "ur_field_projection_bwd")
    torch.cuda.synchronize()
    for b, k, name in ((b0, B * Q * E, "drec"), (b1, F_ * Q, "dWf"), (b2, F_, "dbf")):
        _guard_intact(b, k, f"field projection {name}")
    return drec, dWf, dbf


def _fproj_case(B, Q, F_, E, seed, fast, misalign=False):
    rec, Wf, bf, dout = ew_cases.fproj_inputs(B, Q, F_, E, seed)
    if misalign:                                             # rec one element into its buffer: 2 bytes off every vector alignment
        buf = torch.zeros(rec.numel() + 8, dtype=BF16, device=DEV)
        buf[1:1 + rec.numel()] = rec.reshape(-1).to(DEV)
        rec_d = buf[1:1 + rec.numel()].view(B, Q, E)
        assert rec_d.data_ptr() % 16 == 2
    else:
        rec_d = rec.to(DEV)
    Wd, bd, dd = Wf.to(DEV), bf.to(DEV), dout.to(DEV)
    what = f"({B}, {Q}, {F_}, {E})"
    kind = "32" if fast else ""
    out = _fproj_fwd(rec_d, Wd, bd)
    _note(f"fproj_fwd{kind}_kernel", ref64.assert_f32_close(out, ref64.field_projection_fwd(rec, Wf, bf), ref64.field_projection_fwd(rec, Wf, bf, dtype=F32),
                                                            what=f"out {what}"))
    drec, dWf, dbf = _fproj_bwd(dd, rec_d, Wd)
    r64, r32 = ref64.field_projection_bwd(dout, rec, Wf), ref64.field_projection_bwd(dout, rec, Wf, dtype=F32)
    _note(f"fproj_bwd{kind}_kernel drec", ref64.assert_bf16_rows(drec, r64[0], r32[0], f"drec {what}"))
    aW = ref64.fproj_fast_dwf_terms(r64[3]) if fast else r64[3]
    _note(f"fproj_bwd{kind}_kernel dWf", ref64.assert_colsum_close(dWf, r64[1], r32[1], aW, f"dWf {what}"))
    _note(f"fproj_bwd{kind}_kernel dbf", ref64.assert_colsum_close(dbf, r64[2], r32[2], r64[4], f"dbf {what}"))
    again = _fproj_bwd(dd, rec_d, Wd)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((drec, dWf, dbf), again)), f"{what}: the backward is not reproducible"
    return rec, Wf, bf, dout, rec_d, Wd


@pytest.mark.parametrize("B,Q,F_,E", ew_cases.FPROJ_GENERIC)
def test_field_projection_generic(B, Q, F_, E):
    """B * E = 76,800 is past the backward's 256 workgroups (the grid-stride loop with the `ok` guards around wave_sum), 537,600 past the
    forward's 2048; (3, 64, 32, 100) are the MAXQ / MAXF limits with E % 4 != 0; Q = 32 with F = 17 > FPAD stays generic"""
    assert not (Q == 32 and F_ <= 16)
    _fproj_case(B, Q, F_, E, 600 + B, fast=False)


@pytest.mark.parametrize("B,Q,F_,E", ew_cases.FPROJ_FAST)
def test_field_projection_fast(B, Q, F_, E):
    """the reference's shape; B above the 256 workgroups with F = FPAD and the smallest E the backward takes; a single field"""
    assert Q == 32 and F_ <= 16 and E % 128 == 0
    rec, Wf, bf, dout, rec_d, Wd = _fproj_case(B, Q, F_, E, 700 + B, fast=True)
    # a dout that is exact in bf16 loses nothing in front of the MFMA: the plain criterion, without the operand-rounding term
    dq = dout.to(BF16).float()
    _, dWf, dbf = _fproj_bwd(dq.to(DEV), rec_d, Wd)
    r64, r32 = ref64.field_projection_bwd(dq, rec, Wf), ref64.field_projection_bwd(dq, rec, Wf, dtype=F32)
    _note("fproj_bwd32_kernel dWf (bf16-exact dout)", ref64.assert_colsum_close(dWf, r64[1], r32[1], r64[3], f"dWf, bf16-exact dout ({B}, {Q}, {F_}, {E})"))
    ref64.assert_colsum_close(dbf, r64[2], r32[2], r64[4], "dbf, bf16-exact dout")


def test_field_projection_misaligned_rec_takes_the_generic_kernels():
    """Q = 32, F = 14, E = 256 would be the fast path; rec 2 bytes off falls back -- and is held WITHOUT the fast path's operand-rounding term"""
    _fproj_case(5, 32, 14, 256, 800, fast=False, misalign=True)


def test_field_projection_fast_forward_past_the_grid_cap():
    """B * E / 4 = 1,051,392 threads of work against 4096 workgroups of 256: rec is a 37-row block tiled 111 times (an odd period: a stride error
    cannot land on an equal row), the reference is formed once for the block and every repeat must carry the first repeat's bits"""
    reps, blk, Q, F_, E = 111, 37, 32, 1, 1024
    B = reps * blk
    assert B * E > 4096 * 256 * 4
    rec, Wf, bf, _ = ew_cases.fproj_inputs(blk, Q, F_, E, 900)
    out = _fproj_fwd(rec.to(DEV).repeat(reps, 1, 1), Wf.to(DEV), bf.to(DEV)).view(reps, blk, F_, E)
    _note("fproj_fwd32_kernel", ref64.assert_f32_close(out[0], ref64.field_projection_fwd(rec, Wf, bf), ref64.field_projection_fwd(rec, Wf, bf, dtype=F32),
                                                       what="out, first repeat"))
    same = (_bits(out) == _bits(out[0])[None]).reshape(reps, -1).all(dim=1)
    assert same.all(), f"repeats {(~same).nonzero().reshape(-1).tolist()[:8]} differ from the first"


def test_field_projection_refuses_bad_arguments_without_a_launch():
    lib = _lib.load()
    B, E = 4, 64
    rec = torch.zeros(B * 65 * E, dtype=BF16, device=DEV)
    W, bf = torch.zeros(33 * 65, device=DEV), torch.zeros(33, device=DEV)
    dout = torch.zeros(B * 33 * E, device=DEV)
    (out, ob), (drec, rb), (dWf, wb), (dbf, bb) = _sentinel((B * 33 * E,)), _sentinel((B * 65 * E,), BF16), _sentinel((33 * 65,)), _sentinel((33,))
    ws, n = hip._heads_ws(64, 32, rec.device)
    st = hip._stream()
    for Q, F_ in ((65, 32), (64, 33), (0, 8), (8, 0)):
        assert lib.ur_field_projection_fwd(rec.data_ptr(), W.data_ptr(), bf.data_ptr(), out.data_ptr(), B, Q, F_, E, st) < 0
        assert b"ur_field_projection_fwd" in lib.ur_last_error()
        assert lib.ur_field_projection_bwd(dout.data_ptr(), rec.data_ptr(), W.data_ptr(), drec.data_ptr(), dWf.data_ptr(), dbf.data_ptr(), B, Q, F_, E,
                                           ws.data_ptr(), n, st) < 0
        assert b"ur_field_projection_bwd" in lib.ur_last_error()
    need = lib.ur_heads_workspace_bytes(64, 32)
    assert need == 256 * (64 * 32 + 32) * 4
    assert lib.ur_field_projection_bwd(dout.data_ptr(), rec.data_ptr(), W.data_ptr(), drec.data_ptr(), dWf.data_ptr(), dbf.data_ptr(), B, 64, 32, E,
                                       ws.data_ptr(), need - 1, st) < 0
    assert b"workspace too small" in lib.ur_last_error()
    assert lib.ur_field_projection_bwd(dout.data_ptr(), rec.data_ptr(), W.data_ptr(), drec.data_ptr(), dWf.data_ptr(), dbf.data_ptr(), B, 64, 32, E,
                                       0, need, st) < 0
    torch.cuda.synchronize()
    for b in (ob, rb, wb, bb):
        sent = SENT32 if b.element_size() == 4 else SENT16
        assert (_bits(b) == sent).all(), "a refused call wrote"

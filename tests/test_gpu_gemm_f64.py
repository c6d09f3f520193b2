"""GPU: the fused epilogues of the Qwen3 decoder's GEMMs, ELEMENT BY ELEMENT against float64 (tests/ref64.py, checked on the CPU in
tests/test_ref64.py): q/k-norm + RoPE of the merged q|k|v launch (csrc/gemm_pers.hip EPI 3), the paired SwiGLU forward of the merged gate|up
launch (EPI 4) and the generic swiglu_fwd= epilogue, the SwiGLU backward of the down-projection's dX launch (EPI 1, generic and persistent,
plain / with the LoRA pair in the K stream / with the masked rank-16 term), and the LoRA second K range at widths that are no multiple of 16.

Exact-product family.  Integer-valued R, S in [-3, 3], K = 256 or 320, an integer LoRA pair in [-1, 1]: |acc| < 2^24, the accumulator is
exact in any order and only the epilogue rounds.  acc is formed in float64 ON THE DEVICE (torch matmul), and the references and criteria of
this module stay there too (ref64.assert_ulp_ratio: assert_within_ulps without the trip to the CPU; outputs are 8 .. 35 M elements).
Random-operand family.  Gaussian bf16 operands at K = 1024, one case per epilogue: the float64 formula over the float64 product, with the
8 e32 of assert_lora_bf16 -- e32 = the same formula over a float32 product formed on the CPU.

Criteria (docs/lab_notes.md, "Element-wise float64 tests: the decoder's GEMM epilogues"):
  EPI 3 q_r / k_r   |got - ref64| <= 1 bf16 ulp + 2^-18 head-row max |ref64| + 8 e32_row, ref64 = the float64 formula over the kernel's OWN
                    table row at the row's position, e32_row = head-row max |float32 emulation, angle recurrence included, - ref64|
                    (ref64.qkrope_bound; the margin is shown on the emulation alone in test_margins_beyond_one_ulp_are_what_float32_costs)
  EPI 3 v           the correctly rounded exact product, bit for bit;  rstd: ref64.assert_f32_close with scale |rstd|
  EPI 4 / fwd       gate | up (up) bit-equal to the correctly rounded exact product; act within 1 bf16 ulp, no floor, of silu(gate BITS) * up BITS
  EPI 1             d_up within 1 bf16 ulp, no floor; d_gate within 1 ulp + 2^-18 |d(act) * up|   (test_swiglu_shapes' criterion), d(act) the
                    UNROUNDED float64 product (+ masked term: ref64.lora_masked_epilogue)
  second K range    bit-equal to the correctly rounded exact value on both kernels
No element is exempt.  Every output is pre-filled with the 0x4B4B sentinel (a NaN pattern where every finite bf16 is a legitimate output) and must be written and finite where it belongs and untouched in
the pad columns of a wider row stride; a second call must be bit-identical.  Keep flags come from oracle/dropout_ref.lora_keep only, after
the planes handed to the kernel were compared with the twin's words.  Every case asserts the kernel it means to test is the one that runs:
hip.gemm_qkrope_supported / gemm_swiglu_paired_supported, and for EPI 1 and the second K range the library's own selection for the launch's
arguments (hip.gemm_plan) under gemm_persistent_mode(1) and (0).  Every test prints its worst error / bound ("[ratio] kernel: x")."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dropout_ref  # noqa: E402
from tests import ref64  # noqa: E402
from unirec_amd import hip  # noqa: E402

# entry point -> the primitive-level tests of this module that hold it against a reference (tests/test_abi_test_coverage.py)
COVERS = {
    "ur_gemm": ["test_qkrope_epilogue_exact_products", "test_paired_swiglu_forward_exact_products", "test_swiglu_backward_epilogue_generic",
                "test_swiglu_backward_epilogue_persistent", "test_second_k_range_widths_off_the_16_grid"],
    "ur_gemm_qkrope_supported": ["test_qkrope_epilogue_exact_products", "test_qkrope_support_answers"],
    "ur_qkrope_perm": ["test_qkrope_perm_is_the_paired_order", "test_qkrope_epilogue_exact_products"],
    "ur_gemm_swiglu_paired_supported": ["test_paired_swiglu_forward_exact_products"],
}

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENTINEL = 0x4B4B                    # a finite bf16 bit pattern (13303808.0) nothing here computes ...
SENTINEL_NAN = 0x7FA5                # ... except the launches over EVERY finite bf16 (gate = 0x4B4B is one of them): a NaN pattern no arithmetic produces
EPS = 1e-6
THETA = 1e6
WORST = {}


def _note(kernel, ratio):
    WORST[kernel] = max(WORST.get(kernel, 0.0), float(ratio))
    print(f"[ratio] {kernel}: {float(ratio):.4f}")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(shape, seed, lo=-3, hi=3):
    """integer-valued float64 on the device"""
    return torch.randint(lo, hi + 1, shape, generator=_gen(seed)).to(DEV).to(F64)


def _bits16(t):
    return t.contiguous().view(torch.int16)


def _sentinel_bf16(M, n, pad=8, pattern=SENTINEL):
    """(the [M, n] output view, its [M, n + pad] base) filled with the sentinel pattern"""
    base = torch.full((M, n + pad), pattern, dtype=torch.int16, device=DEV).view(BF16)
    return base[:, :n], base


def _written(out, base, what, finite=True, pattern=SENTINEL):
    """every element of the view written (and finite; finite=False: no NaN -- infinities are the criterion's business), the pad columns of
    the wider row untouched"""
    n = out.shape[1]
    assert not (_bits16(out) == pattern).any(), f"{what}: elements left unwritten"
    if finite:
        assert torch.isfinite(out.float()).all(), f"{what}: non-finite outputs"
    else:
        assert not torch.isnan(out.float()).any(), f"{what}: NaN outputs"
    assert (_bits16(base[:, n:]) == pattern).all(), f"{what}: pad columns of the wider row were written"


def _wide(t, pad=8, off=0):
    """device copy of t [M, W] as a column view of a buffer `pad` columns wider (ld != width)"""
    base = torch.zeros((t.shape[0], t.shape[1] + pad), dtype=BF16, device=DEV)
    base[:, off:off + t.shape[1]] = t.to(BF16)
    return base[:, off:off + t.shape[1]]


def _exact_bits(got, exact64, what):
    """got (bf16, device) carries the bits of the exact float64 value rounded ONCE (both zeros count as +0): ref64.assert_lora_exact on the device"""
    want = ref64._bf16_of_exact(exact64)
    g = torch.where(got == 0, torch.zeros_like(got), got)
    w = torch.where(want == 0, torch.zeros_like(want), want)
    off = _bits16(g) != _bits16(w)
    if off.any():
        i = tuple(int(v) for v in off.nonzero()[0])
        raise AssertionError(f"{what}: {int(off.sum())} of {off.numel()} elements differ from the correctly rounded exact value; first at {i}: "
                             f"got {got[i].item()!r}, exact {exact64[i].item()!r}")
    return 0.0


def _check_may_overflow(got, ref, ulps, floor, what):
    """test_gpu_head_primitives._check_may_overflow on the device: the criterion, except where the float64 reference leaves bfloat16's range --
    there the output must be the infinity of the right sign (or the largest finite value inside the last half ulp)"""
    got, ref = got.to(F64), ref.to(F64)
    over = ref.abs() > ref64.BF16_MAX
    sure = ref.abs() > ref64.BF16_MAX + 2.0 ** 120
    assert (got[sure] == torch.sign(ref[sure]) * float("inf")).all(), f"{what}: overflow must give the signed infinity"
    edge = over & ~sure
    assert ((got[edge].abs() >= ref64.BF16_MAX) & (torch.sign(got[edge]) == torch.sign(ref[edge]))).all(), f"{what}: wrong value at the edge of the range"
    fl = torch.as_tensor(floor, dtype=F64, device=ref.device).expand_as(ref)
    z = torch.zeros_like(ref)
    return ref64.assert_ulp_ratio(torch.where(over, z, got), torch.where(over, z, ref), ulps, torch.where(over, z, fl), what)


def _all_finite_bf16():
    bits = torch.arange(0, 65536, dtype=torch.int32)
    bits = bits[(bits & 0x7F80) != 0x7F80]                        # drop inf / NaN: 65 280 values, zeros and subnormals included
    assert bits.numel() == 65280
    return bits.to(torch.int16).view(BF16)


UPS = [0.0, 2.0 ** -100, -(2.0 ** -100), 1.0, -2.5, 0.0078125 * 3, 3.0e4, -3.0e4]       # tests/test_gpu_head_primitives.py
DACTS = [1.0, -0.5, 2.0 ** -9 * 3, 100.0]


class _mode:
    """with _mode(1): ...   -- ur_gemm_persistent_mode set and restored"""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.prev = hip.gemm_persistent_mode(self.mode)

    def __exit__(self, *exc):
        hip.gemm_persistent_mode(self.prev)
        return False


def _persistent_takes(M, N, K, K2=0, **launch):
    """the library's own selection (hip.gemm_plan: ur_gemm_plan) for the K-contiguous bf16 [M, N] launch under test -- launch: its epilogue
    operands, row strides and alpha, as hip.gemm_plan_args takes them -- under the CURRENT ur_gemm_persistent_mode"""
    return hip.gemm_plan(M, N, K, K2, **launch)["kernel"] == "persistent"


def _swiglu_bwd_launch(I, ld=None, **more):
    """the SwiGLU backward epilogue's arguments as hip.gemm passes them: gu / dgu rows of ld (default 2 I) elements, C = dgu"""
    ld = 2 * I if ld is None else ld
    return dict(swiglu_gu=True, swiglu_dgu=True, swiglu_ldgu=ld, swiglu_lddgu=ld, ldc=ld, **more)


_TABLES = {}


def _tables(S):
    if S not in _TABLES:
        _TABLES[S] = hip.rope_table(S, 128, THETA, DEV)           # the kernel's own f32 rows (test_rope_table holds them)
        torch.cuda.synchronize()
    return _TABLES[S]


def _norm_weights(seed):
    qw = (1.0 + 0.1 * torch.randn(128, generator=_gen(seed))).to(DEV)
    kw = (1.0 + 0.1 * torch.randn(128, generator=_gen(seed + 1))).to(DEV)
    assert not torch.equal(qw, kw)
    return qw, kw


def _paired_rows(W, nqk_heads):
    """weight rows of the q / k heads in the paired order of the fused launch: W_paired[h * 128 + c] = W[h * 128 + perm[c]]"""
    perm = hip.qkrope_perm(128)
    rows = torch.cat([(torch.arange(nqk_heads)[:, None] * 128 + perm[None, :]).reshape(-1), torch.arange(nqk_heads * 128, W.shape[0])])
    return W[rows.to(W.device)].contiguous()


# =============================================================================================================================
# EPI 3: q/k-norm + RoPE of the merged q|k|v launch
def test_qkrope_perm_is_the_paired_order():
    """hip.qkrope_perm(128) is a permutation of 0 .. 127, and tile columns c and c + 16 of a 32-column group hold features d and d + 64
    (ur_qkrope_perm: ((c >> 4) & 1) * 64 + ((c >> 5) & 3) * 16 + (c & 15))"""
    perm = hip.qkrope_perm(128)
    assert perm.shape == (128,) and sorted(perm.tolist()) == list(range(128))
    for c in range(128):
        assert int(perm[c]) == ((c >> 4) & 1) * 64 + ((c >> 5) & 3) * 16 + (c & 15)
        if (c & 31) < 16:
            assert int(perm[c]) < 64 and int(perm[c + 16]) == int(perm[c]) + 64
    with pytest.raises(ValueError):
        hip.qkrope_perm(64)


def test_qkrope_support_answers():
    """ur_gemm_qkrope_supported answers 0 for S = 128, S = 384, an odd head count on q, k or v, 127 tiles, alpha != 1 and a bias, and 1 for
    the neighbouring launches that differ in that one respect"""
    q = lambda *a, **k: hip.gemm_qkrope_supported(*a, DEV, **k)      # noqa: E731    (M, N, K, K2, S, nq_cols, nk_cols)
    assert q(2048, 4096, 256, 0, 256, 2048, 1024) and q(2304, 4096, 256, 0, 768, 2048, 1024)
    assert not q(2048, 4096, 256, 0, 128, 2048, 1024), "S = 128"
    assert not q(2304, 4096, 256, 0, 384, 2048, 1024), "S = 384"
    assert not q(2048, 4096, 256, 0, 256, 1920, 1024), "15 q heads (and 9 v heads)"
    assert not q(2048, 4096, 256, 0, 256, 2048, 896), "7 k heads (and 9 v heads)"
    assert not q(2048, 4096, 256, 0, 256, 2048 + 128, 1024 + 128), "17 q and 9 k heads"
    assert q(128 * 256, 256, 256, 0, 256, 256, 0) and not q(127 * 256, 256, 256, 0, 256, 256, 0), "127 tiles"
    assert not q(2048, 4096, 256, 0, 256, 2048, 1024, alpha=0.5), "alpha != 1"
    assert not q(2048, 4096, 256, 0, 256, 2048, 1024, bias=torch.zeros(4096, device=DEV)), "a bias"


#            M      S     nq    nk    N     K
QKR_SHAPES = {
    "a": (2048, 2048, 2048, 1024, 4096, 256),      # the 0.6B shape: positions up to 2047, gcw = 4 column chunks
    "b": (2048, 256, 2048, 1024, 4096, 256),       # pos0 = 0 in every tile, every tile wraps
    "c": (2048, 512, 2048, 1024, 4096, 256),       # pos0 in {0, 256}
    "d": (11008, 256, 256, 256, 768, 256),         # gn = 3, no column chunks, 129 tiles
    "e": (8448, 256, 2048, 1024, 4096, 320),       # 528 tiles: workgroups walk 2 and 3 tiles, an odd K-tile count
}


def _hold_qkrope(tag, out, acc, acc32, qw, kw, S, nq, nk, v_check):
    """q_r / k_r / rstd of `out` against the float64 formula over acc (acc32: what the float32 emulation starts from); returns the worst
    |q_r - formula| / ulp and the ratio against the BARE bound (no e32 term), for the lab notes"""
    cos, sin = _tables(S)
    q1, k1, v1, rstd = out
    ref = ref64.qkrope_epilogue(acc, qw, kw, cos, sin, S, nq, nk, EPS)
    un = ref64.qkrope_emulated(acc32, qw, kw, cos, sin, S, nq, nk, EPS, rounded=False)
    ulps = bare = 0.0
    for got, r, u, n in ((q1, ref[0], un[0], "q_r"), (k1, ref[1], un[1], "k_r")):
        _note(f"gemm EPI 3 {n}", ref64.assert_ulp_ratio(got, r, 1, ref64.qkrope_bound(r, u), f"{tag} {n}"))
        bare = max(bare, ref64.ulp_ratio(got, r, 1, ref64.qkrope_bound(r))[0])
        if n == "q_r":
            ulps = float(((got.to(F64) - r).abs() / ref64.bf16_ulp(r)).max())
        rm = r.abs().reshape(r.shape[0], -1, 128).amax(-1)
        e = (u - r).abs().reshape(r.shape[0], -1, 128).amax(-1)
        print(f"[info] {tag} {n}: e32_row / row max at most {float((e[rm > 0] / rm[rm > 0]).max()):.3e}")
    v_check(v1, ref[2])
    r32 = ref64.qkrope_epilogue(acc32, qw, kw, cos, sin, S, nq, nk, EPS, dtype=F32)[3]
    col = lambda t: t.reshape(-1, 1).cpu()      # noqa: E731
    _note("gemm EPI 3 rstd", ref64.assert_f32_close(col(rstd), col(ref[3]), col(r32), scale=ref[3].abs().reshape(-1).cpu(), what=f"{tag} rstd"))
    print(f"[info] {tag}: worst |q_r - formula over the row's own table row| = {ulps:.3f} bf16 ulp; {bare:.3f} x the bound WITHOUT the e32 term")
    return ulps, bare


def _run_qkrope(tag, R, Wn, t, Bn, M, S, nq, nk, N, K2):
    """one launch pair (second call bit-identical) into column views of wider sentinel buffers; returns the first call's outputs"""
    qw, kw = _norm_weights(1100)
    cos, sin = _tables(S)
    nh = (nq + nk) // 128
    assert hip.gemm_qkrope_supported(M, N, R.shape[1], K2, S, nq, nk, DEV), f"{tag}: the launch would not carry the epilogue"
    Wp = _paired_rows(Wn.to(BF16), nh)
    R2 = None if t is None else _wide(t, pad=16, off=8)
    S2 = None if Bn is None else _wide(_paired_rows(Bn.to(BF16), nh), pad=8)
    Rb = R.to(BF16).contiguous()
    res = []
    for _ in range(2):
        (q, qb), (k, kb), (v, vb) = _sentinel_bf16(M, nq), _sentinel_bf16(M, nk), _sentinel_bf16(M, N - nq - nk)
        rstd = torch.full((M, nh), float("nan"), device=DEV)
        got = hip.gemm_qkv_rope(Rb, Wp, qw, kw, cos, sin, S, nq, nk, EPS, R2=R2, S2=S2, out=(q, k, v, rstd))
        assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, (q, k, v, rstd)))
        for o, b, n in ((q, qb, "q_r"), (k, kb, "k_r"), (v, vb, "v")):
            _written(o, b, f"{tag} {n}")
        assert torch.isfinite(rstd).all(), f"{tag}: rstd unwritten (NaN pre-fill) or non-finite"
        res.append((q, k, v, rstd))
    for a, b in zip(res[0][:3], res[1][:3]):
        assert torch.equal(_bits16(a), _bits16(b)), f"{tag}: a second call differs"
    assert torch.equal(res[0][3], res[1][3]), f"{tag}: rstd of a second call differs"
    return res[0], qw, kw


@pytest.mark.parametrize("K2", [0, 48, 24])
@pytest.mark.parametrize("case", list(QKR_SHAPES))
def test_qkrope_epilogue_exact_products(case, K2):
    """shapes (a) .. (e) x {no LoRA pair, K2 = 48, K2 = 24 (the merged q|k|v launches of ranks 16 and 8)}; one all-zero activation row per
    batch (output 0, rstd = 1 / sqrt(eps)); norm weights 1 + 0.1 randn that differ between q and k; weights (and the LoRA B operand) in the
    paired row order; every output a column view of a wider sentinel buffer, t / B column views too"""
    M, S, nq, nk, N, K = QKR_SHAPES[case]
    tag = f"EPI 3 ({case}) M{M} S{S} N{N} K{K} K2 {K2}"
    R, Wn = _ints((M, K), 1101), _ints((N, K), 1102)
    R[5::S] = 0.0
    t = Bn = None
    acc = R @ Wn.t()
    if K2:
        t, Bn = _ints((M, K2), 1103, -1, 1), _ints((N, K2), 1104, -1, 1)
        t[5::S] = 0.0
        acc = acc + t @ Bn.t()
    assert float(acc.abs().max()) < 2.0 ** 24
    out, qw, kw = _run_qkrope(tag, R, Wn, t, Bn, M, S, nq, nk, N, K2)
    _hold_qkrope(tag, out, acc, acc, qw, kw, S, nq, nk, lambda v, r: _note("gemm EPI 3 v (exact)", _exact_bits(v, r, f"{tag} v")))
    zero = torch.arange(5, M, S, device=DEV)
    assert (out[0][zero] == 0).all() and (out[1][zero] == 0).all() and (out[2][zero] == 0).all(), f"{tag}: the all-zero rows"
    assert float((out[3][zero].to(F64) - EPS ** -0.5).abs().max()) <= 2.0 ** -20 * EPS ** -0.5, f"{tag}: rstd of the all-zero rows is not 1 / sqrt(eps)"


def _randn_bf16(shape, seed, std=1.0):
    return (torch.randn(shape, generator=_gen(seed)) * std).to(BF16)


def _products(Rb, Sb):
    """(float64 product on the device, float32 product formed on the CPU, sum |term| in float64) of CPU bf16 operands"""
    a64 = Rb.to(DEV).to(F64) @ Sb.to(DEV).to(F64).t()
    a32 = (Rb.float() @ Sb.float().t()).to(DEV)
    ab = Rb.to(DEV).to(F64).abs() @ Sb.to(DEV).to(F64).abs().t()
    return a64, a32, ab


def test_qkrope_epilogue_random_operands():
    """shape (a) with Gaussian bf16 operands at K = 1024: the float64 formula over the float64 product; e32_row from the emulation over a
    float32 CPU product; v within 1 ulp + 2^-20 sum |term| + 8 |acc32 - acc64| (assert_lora_bf16)"""
    M, S, nq, nk, N, _ = QKR_SHAPES["a"]
    K = 1024
    tag = f"EPI 3 random M{M} S{S} N{N} K{K}"
    Rb, Wb = _randn_bf16((M, K), 1110), _randn_bf16((N, K), 1111, 0.05)
    acc, acc32, ab = _products(Rb, Wb)
    out, qw, kw = _run_qkrope(tag, Rb.to(DEV), Wb.to(DEV), None, None, M, S, nq, nk, N, 0)
    vs = slice(nq + nk, N)
    _hold_qkrope(tag, out, acc, acc32, qw, kw, S, nq, nk,
                 lambda v, r: _note("gemm EPI 3 v", ref64.assert_ulp_ratio(v, r, 1, 2.0 ** -20 * ab[:, vs] + 8.0 * (acc32[:, vs].to(F64) - r).abs(), f"{tag} v")))


# =============================================================================================================================
# EPI 4: the paired SwiGLU forward of the merged gate|up launch; the generic swiglu_fwd= epilogue
def _run_paired(tag, Rb, Wn, t, Bn, M, I, K2, pattern=SENTINEL):
    """Rb [M, K] bf16 device, Wn [2 I, K] natural order (gate rows | up rows): (gu, act) of the first of two bit-identical calls"""
    rows = hip.swiglu_pair_rows(I).to(DEV)
    assert hip.gemm_swiglu_paired_supported(M, I, Rb.shape[1], K2, DEV), f"{tag}: the launch would not carry the epilogue"
    Wp = Wn.to(BF16)[rows].contiguous()
    R2 = None if t is None else _wide(t, pad=16, off=8)
    S2 = None if Bn is None else _wide(Bn[rows], pad=8)
    res = []
    for _ in range(2):
        (gu, gub), (act, actb) = _sentinel_bf16(M, 2 * I, pattern=pattern), _sentinel_bf16(M, I, pattern=pattern)
        hip.gemm(Rb, Wp, out=gu, R2=R2, S2=S2, swiglu_paired=act)
        res.append((gu, gub, act, actb))
    assert torch.equal(_bits16(res[0][0]), _bits16(res[1][0])) and torch.equal(_bits16(res[0][2]), _bits16(res[1][2])), f"{tag}: a second call differs"
    return res[0]


@pytest.mark.parametrize("M,I,K2", [(2048, 2048, 0), (2048, 2048, 32), (2048, 2048, 16), (2048, 2048, 8), (32768, 128, 0), (11008, 384, 0)])
def test_paired_swiglu_forward_exact_products(M, I, K2):
    """gate | up BIT-equal to the correctly rounded exact product, act within 1 bf16 ulp (no floor) of silu(gate bits) * (up bits);
    I = 128: gn = 1, I = 384: gn = 3; the LoRA pair of ranks 16 (merged gate|up: K2 = 32), 8 and a single rank-8 adapter"""
    K = 256
    tag = f"EPI 4 M{M} I{I} K{K} K2 {K2}"
    R, Wn = _ints((M, K), 1201), _ints((2 * I, K), 1202)
    acc = R @ Wn.t()
    t = Bn = None
    if K2:
        t, Bn = _ints((M, K2), 1203, -1, 1), _ints((2 * I, K2), 1204, -1, 1)
        acc = acc + t @ Bn.t()
    gu, gub, act, actb = _run_paired(tag, R.to(BF16).contiguous(), Wn, t, Bn, M, I, K2)
    _written(gu, gub, f"{tag} gate|up")
    _written(act, actb, f"{tag} act")
    _, want_act = ref64.swiglu_fwd_epilogue(acc)
    _note("gemm EPI 4 gate|up (exact)", _exact_bits(gu, acc, f"{tag} gate|up"))
    _note("gemm EPI 4 act", ref64.assert_ulp_ratio(act, want_act, 1, 0.0, f"{tag} act"))


def test_paired_swiglu_forward_over_every_finite_bf16():
    """ONE launch of 510 tiles (I = 65280 = 510 x 128, M = 256, K = 256): S[gate n, 0] = x_n for every finite bf16, R[m, 0] = +-1, and
    S[up n, 1] = 1, R[m, 1] = UPS[m % 8]: gate = +-x_n and up = UPS[m % 8] exactly"""
    x = _all_finite_bf16()
    I, M, K = x.numel(), 256, 256
    tag = "EPI 4 over all bf16 gates"
    Wn = torch.zeros(2 * I, K, dtype=BF16)
    Wn[:I, 0] = x
    Wn[I:, 1] = 1.0
    sign = torch.tensor([1.0, -1.0]).repeat_interleave(8).repeat(M // 16)
    ups = torch.tensor(UPS).to(BF16).repeat(M // 8)
    R = torch.zeros(M, K, dtype=BF16)
    R[:, 0], R[:, 1] = sign.to(BF16), ups
    acc = torch.cat([sign.to(F64)[:, None] * x.to(F64)[None, :], ups.to(F64)[:, None].expand(M, I)], 1).to(DEV)
    gu, gub, act, actb = _run_paired(tag, R.to(DEV), Wn.to(DEV), None, None, M, I, 0, pattern=SENTINEL_NAN)
    _written(gu, gub, f"{tag} gate|up", pattern=SENTINEL_NAN)
    _written(act, actb, f"{tag} act", finite=False, pattern=SENTINEL_NAN)      # silu(+-3e38) * 3e4 overflows: held by _check_may_overflow
    _note("gemm EPI 4 gate|up (exact)", _exact_bits(gu, acc, f"{tag} gate|up"))
    _note("gemm EPI 4 act (all bf16)", _check_may_overflow(act, ref64.swiglu_fwd_epilogue(acc)[1], 1, 0.0, f"{tag} act"))


@pytest.mark.parametrize("M,I,K", [(300, 256, 128), (16384, 1024, 64), (1000, 516, 72)])
def test_generic_swiglu_forward_epilogue_exact_products(M, I, K):
    """the generic swiglu_fwd= epilogue at test_gemm_swiglu_forward_epilogue's three shapes: up bit-equal to the rounded exact product, act
    within 1 bf16 ulp (no floor) of silu(gate) * (up bits); gate | up column halves of one buffer where I % 8 == 0"""
    tag = f"swiglu_fwd= M{M} I{I} K{K}"
    R, Wn = _ints((M, K), 1211), _ints((I, K), 1212)
    acc = R @ Wn.t()
    gate = _randn_bf16((M, I), 1213, 2.0).to(DEV)
    with _mode(0):
        res = []
        for _ in range(2):
            act, actb = _sentinel_bf16(M, I, pad=8 if I % 8 == 0 else 4)
            if I % 8 == 0:
                gu = torch.full((M, 2 * I + 8), SENTINEL, dtype=torch.int16, device=DEV).view(BF16)
                gu[:, :I] = gate
                g_in, up, upb = gu[:, :I], gu[:, I:2 * I], gu
            else:               # (column halves of one buffer would leave the up half 8-byte aligned only: separate tensors)
                g_in = gate
                up, upb = _sentinel_bf16(M, I, pad=4)
            hip.gemm(R.to(BF16).contiguous(), Wn.to(BF16).contiguous(), out=up, swiglu_fwd=(g_in, act))
            res.append((up, upb, act, actb))
    up, upb, act, actb = res[0]
    assert not (_bits16(up) == SENTINEL).any() and (_bits16(upb[:, -4:]) == SENTINEL).all(), f"{tag}: up unwritten or its pad written"
    _written(act, actb, f"{tag} act")
    assert torch.equal(_bits16(up), _bits16(res[1][0])) and torch.equal(_bits16(act), _bits16(res[1][2])), f"{tag}: a second call differs"
    _note("gemm swiglu_fwd= up (exact)", _exact_bits(up, acc, f"{tag} up"))
    _note("gemm swiglu_fwd= act", ref64.assert_ulp_ratio(act, ref64.swiglu_fwd(gate, up), 1, 0.0, f"{tag} act"))


def test_paired_swiglu_forward_random_operands():
    """M 2048, I 2048 at K = 1024, Gaussian bf16 operands: gate | up within 1 ulp + 2^-20 sum |term| + 8 |acc32 - acc64| of the float64
    product, act within 1 ulp (no floor) of silu(gate BITS WRITTEN) * (up bits written)"""
    M, I, K = 2048, 2048, 1024
    tag = f"EPI 4 random M{M} I{I} K{K}"
    Rb, Wb = _randn_bf16((M, K), 1220), _randn_bf16((2 * I, K), 1221, 0.05)
    acc, acc32, ab = _products(Rb, Wb)
    gu, gub, act, actb = _run_paired(tag, Rb.to(DEV), Wb.to(DEV), None, None, M, I, 0)
    _written(gu, gub, f"{tag} gate|up")
    _written(act, actb, f"{tag} act")
    _note("gemm EPI 4 gate|up", ref64.assert_ulp_ratio(gu, acc, 1, 2.0 ** -20 * ab + 8.0 * (acc32.to(F64) - acc).abs(), f"{tag} gate|up"))
    _note("gemm EPI 4 act", ref64.assert_ulp_ratio(act, ref64.swiglu_fwd(gu[:, :I], gu[:, I:]), 1, 0.0, f"{tag} act"))


# =============================================================================================================================
# EPI 1: the SwiGLU backward of the down-projection's dX launch
def _special_gates():
    """0, +-2^-100, -1.28 +- two ulps (where silu' cancels), +-30, +-100, +-3e4, +-1: 16 values"""
    c = torch.tensor([-1.28]).to(BF16).view(torch.int16)
    near = torch.cat([c + d for d in (-2, -1, 0, 1, 2)]).view(BF16).float()
    return torch.cat([torch.tensor([0.0, 2.0 ** -100, -(2.0 ** -100)]), near, torch.tensor([30.0, -30.0, 100.0, -100.0, 3e4, -3e4, 1.0, -1.0])]).to(BF16)


def _gu(M, I, seed):
    """random bf16 of scale 2 with a band of special gates: gate columns 0 .. 15 (I >= 16), and the same values as the LAST 16 gate columns"""
    gu = _randn_bf16((M, 2 * I), seed, 2.0)
    sp = _special_gates()
    gu[:, :16] = sp
    gu[:, I - 16:I] = sp.flip(0)
    return gu


def _drop_planes(seed, p, M, N):
    """(device planes, keep [M, N] float64 on the device) of one adapter: keep from the numpy twin ONLY, the planes compared with its words"""
    W = -(-N // 8) * 8
    bits = hip.lora_dropout_bits(seed, p, M, W, 1, DEV)
    words = torch.from_numpy(dropout_ref.lora_words(seed, p, M, W, 1).view(np.int32))
    assert torch.equal(bits.cpu().contiguous().view(torch.int32), words), "planes differ from the numpy twin"
    keep = torch.from_numpy(dropout_ref.lora_keep(seed, p, M, W, 1)[0, :, :N].astype(np.float64)).to(DEV)
    return bits, keep


SWB_FORMS = ["plain", "lora", "masked"]


def _swiglu_bwd_case(tag, M, I, K, form, persistent, views):
    """dX = dy W^T (+ tb A / + keep / (1 - p) (tb A)) handed to the SwiGLU backward in the epilogue: d_gate | d_up against
    ref64.swiglu_bwd_epilogue of the UNROUNDED exact d(act)"""
    r, p = 16, 0.5
    dy, Wn = _ints((M, K), 1301), _ints((I, K), 1302)
    gu = _gu(M, I, 1303).to(DEV)
    dact = dy @ Wn.t()
    kw = {}
    if form != "plain":
        tb, A = _ints((M, r), 1304, -1, 1), _ints((r, I), 1305, -1, 1)
        R2, S2 = tb.to(BF16).contiguous(), hip.transpose_bf16(A.to(BF16).contiguous())
        kw = dict(R2=_wide(R2, pad=8) if views else R2, S2=S2)
        if form == "masked":
            bits, keep = _drop_planes(77 + M, p, M, I)
            kw["drop"] = (bits, p, r)
            dact = ref64.lora_masked_epilogue(dy, Wn, tb, A, keep[None], p, r)
        else:
            dact = dact + tb @ A
    K2 = 0 if form == "plain" else r
    pad = 8 if I % 8 == 0 else 4
    launch = _swiglu_bwd_launch(I, 2 * I + pad if views else None, drop_rank=r if form == "masked" else 0)
    if K2 and views:
        launch["ldr2"] = r + 8
    with _mode(1):
        takes = _persistent_takes(M, I, K, K2, **launch)
    with _mode(0):
        assert not _persistent_takes(M, I, K, K2, **launch)
    assert takes == persistent, f"{tag}: the launch is {'not ' if persistent else ''}taken by the persistent kernel"
    gin = gu
    if views:
        base = torch.zeros((M, 2 * I + pad), dtype=BF16, device=DEV)
        base[:, :2 * I] = gu
        gin = base[:, :2 * I]
    dyb, Wb = dy.to(BF16).contiguous(), Wn.to(BF16).contiguous()
    res = []
    with _mode(1 if persistent else 0):
        for _ in range(2):
            if views:
                dgu, dgub = _sentinel_bf16(M, 2 * I, pad=pad)
            else:
                dgub = torch.full((M, 2 * I), SENTINEL, dtype=torch.int16, device=DEV).view(BF16)
                dgu = dgub
            out = hip.gemm(dyb, Wb, swiglu_bwd=(gin, dgu), **kw)
            assert out.data_ptr() == dgu.data_ptr()
            res.append((dgu, dgub))
    dgu, dgub = res[0]
    _written(dgu, dgub, tag)
    assert torch.equal(_bits16(dgu), _bits16(res[1][0])), f"{tag}: a second call differs"
    gate, up = gu[:, :I], gu[:, I:]
    rg, ru = ref64.swiglu_bwd_epilogue(dact, gate, up)
    name = f"gemm EPI 1 {'persistent' if persistent else 'generic'} {form}"
    _note(name + " d_gate", ref64.assert_ulp_ratio(dgu[:, :I], rg, 1, 2.0 ** -18 * (dact * up.to(F64)).abs(), f"{tag} d_gate"))
    _note(name + " d_up", ref64.assert_ulp_ratio(dgu[:, I:], ru, 1, 0.0, f"{tag} d_up"))


def _big_tile_shape():
    """tests/test_gpu_norm_f64.py: the smallest K-contiguous launch of gemm.hip's 256 x 256 configuration that stays off the persistent kernel"""
    M, I, K = 264, (256 // 2 - 1) * 256 + 8, 72
    pl = hip.gemm_plan(M, I, K, **_swiglu_bwd_launch(I))
    assert (pl["kernel"], pl["tile"], pl["epi"]) == ("generic", 256, 1) and hip.gemm_plan(M, I - 256, K, **_swiglu_bwd_launch(I - 256))["tile"] == 128
    return M, I, K


@pytest.mark.parametrize("form", SWB_FORMS)
@pytest.mark.parametrize("shape", [(300, 256, 128), (1000, 516, 72), "big"])
def test_swiglu_backward_epilogue_generic(shape, form):
    """(300, 256, 128); (1000, 516, 72): 8-byte pieces, edge tiles, I % 8 != 0; the smallest 256 x 256-tile launch off the persistent
    kernel.  gu / dgu are column views of wider buffers at the first and the last shape"""
    M, I, K = _big_tile_shape() if shape == "big" else shape
    _swiglu_bwd_case(f"EPI 1 generic {form} M{M} I{I} K{K}", M, I, K, form, persistent=False, views=shape != (1000, 516, 72))


@pytest.mark.parametrize("form", SWB_FORMS)
@pytest.mark.parametrize("M,I,K", [(2048, 4096, 256), (8448, 4096, 320)])
def test_swiglu_backward_epilogue_persistent(M, I, K, form):
    """128 tiles at the shortest K stream, and 528 tiles (workgroups walk 2 and 3 tiles, an odd K-tile count); gu / dgu column views of
    wider buffers at the first"""
    _swiglu_bwd_case(f"EPI 1 persistent {form} M{M} I{I} K{K}", M, I, K, form, persistent=True, views=M == 2048)


def test_swiglu_backward_epilogue_over_every_finite_bf16():
    """ONE persistent launch of 255 tiles (I = 65280, M = 256, K = 256): gate[m, n] = x_n for every finite bf16, d(act) = DACTS[m % 4]
    exactly (R[m, 0] = DACTS[m % 4], S[n, 0] = 1), up = UPS[(m / 4) % 8]"""
    x = _all_finite_bf16()
    I, M, K = x.numel(), 256, 256
    tag = "EPI 1 over all bf16 gates"
    d = torch.tensor(DACTS).to(BF16).repeat(M // 4)
    ups = torch.tensor(UPS).to(BF16).repeat_interleave(4).repeat(M // 32)
    R = torch.zeros(M, K, dtype=BF16)
    R[:, 0] = d
    Wn = torch.zeros(I, K, dtype=BF16)
    Wn[:, 0] = 1.0
    gu = torch.cat([x[None, :].expand(M, I), ups[:, None].expand(M, I)], 1).contiguous().to(DEV)
    dact = d.to(F64)[:, None].expand(M, I).to(DEV)
    with _mode(1):
        assert _persistent_takes(M, I, K, **_swiglu_bwd_launch(I))
        dgu, dgub = _sentinel_bf16(M, 2 * I, pattern=SENTINEL_NAN)
        hip.gemm(R.to(DEV), Wn.to(DEV), swiglu_bwd=(gu, dgu))
        again, _ = _sentinel_bf16(M, 2 * I, pattern=SENTINEL_NAN)
        hip.gemm(R.to(DEV), Wn.to(DEV), swiglu_bwd=(gu, again))
    _written(dgu, dgub, tag, finite=False, pattern=SENTINEL_NAN)    # d_up = 100 * 3e38 * s overflows: held by _check_may_overflow
    assert torch.equal(_bits16(dgu), _bits16(again)), f"{tag}: a second call differs"
    rg, ru = ref64.swiglu_bwd_epilogue(dact, gu[:, :I], gu[:, I:])
    scale = (dact * gu[:, I:].to(F64)).abs()
    _note("gemm EPI 1 persistent d_gate (all bf16)", _check_may_overflow(dgu[:, :I], rg, 1, 2.0 ** -18 * scale, f"{tag} d_gate"))
    _note("gemm EPI 1 persistent d_up (all bf16)", _check_may_overflow(dgu[:, I:], ru, 1, 0.0, f"{tag} d_up"))


def test_swiglu_backward_epilogue_random_operands():
    """M 2048, I 4096 at K = 1024 on the persistent kernel, Gaussian bf16 operands: the float64 formula over the float64 product; beside the
    criterion of the exact family each output is granted what the float32 accumulation costs, as assert_lora_bf16 grants it: 2^-20 sum |term|
    of d(act) seen through the output's factor, + 8 |formula over a float32 CPU product - ref64|"""
    M, I, K = 2048, 4096, 1024
    tag = f"EPI 1 random M{M} I{I} K{K}"
    dyb, Wb = _randn_bf16((M, K), 1320), _randn_bf16((I, K), 1321, 0.05)
    dact, d32, ab = _products(dyb, Wb)
    gu = _gu(M, I, 1322).to(DEV)
    gate, up = gu[:, :I], gu[:, I:]
    with _mode(1):
        assert _persistent_takes(M, I, K, **_swiglu_bwd_launch(I))
        dgu, dgub = _sentinel_bf16(M, 2 * I)
        hip.gemm(dyb.to(DEV), Wb.to(DEV), swiglu_bwd=(gu, dgu))
    _written(dgu, dgub, tag)
    rg, ru = ref64.swiglu_bwd_epilogue(dact, gate, up)
    fg, fu = ref64.swiglu_bwd_epilogue(torch.ones_like(dact), gate, up)          # the outputs' factors of d(act)
    g32, u32 = ref64.swiglu_bwd_epilogue(d32, gate, up)                          # the formula over the float32 product
    fl_g = 2.0 ** -18 * (dact * up.to(F64)).abs() + 2.0 ** -20 * ab * fg.abs() + 8.0 * (g32 - rg).abs()
    fl_u = 2.0 ** -20 * ab * fu.abs() + 8.0 * (u32 - ru).abs()
    _note("gemm EPI 1 persistent random d_gate", ref64.assert_ulp_ratio(dgu[:, :I], rg, 1, fl_g, f"{tag} d_gate"))
    _note("gemm EPI 1 persistent random d_up", ref64.assert_ulp_ratio(dgu[:, I:], ru, 1, fl_u, f"{tag} d_up"))


# =============================================================================================================================
# the LoRA second K range at widths off the 16-element grid
@pytest.mark.parametrize("K2", [8, 24, 40, 56])
def test_second_k_range_widths_off_the_16_grid(K2):
    """test_persistent_second_k_range's exact case at K2 = 8 (rank 8), 24 (merged q|k|v of rank 8), 40, 56: row strides of t / B that are no
    multiple of 16 elements and the zero-word fetch INSIDE a 16-element group; bit equality to the rounded exact value on both kernels"""
    M, N, K = 8192, 4096, 512
    R, Sm = _ints((M, K), 1401, -2, 2), _ints((N, K), 1402, -2, 2)
    R2, S2 = _ints((M, K2), 1403, -1, 1), _ints((N, K2), 1404, -1, 1)
    exact = (R @ Sm.t() + R2 @ S2.t()) / 16
    args = [x.to(BF16).contiguous() for x in (R, Sm, R2, S2)]
    assert args[2].stride(0) == K2 and args[3].stride(0) == K2
    for mode, name in ((0, "generic"), (1, "persistent")):
        with _mode(mode):
            assert _persistent_takes(M, N, K, K2, alpha=1.0 / 16) == bool(mode)
            out, base = _sentinel_bf16(M, N)
            hip.gemm(args[0], args[1], R2=args[2], S2=args[3], alpha=1.0 / 16, out=out)
        _written(out, base, f"K2 {K2} {name}")
        _note(f"gemm second K range {name} (exact)", _exact_bits(out, exact, f"second K range K2 {K2} {name}"))


def test_zz_worst_ratio_table():
    """prints the worst observed error / bound per kernel and path over the tests of this module that ran before it (docs/lab_notes.md)"""
    print("\n[table] worst error / bound per kernel and path")
    for k in sorted(WORST):
        print(f"[table] {k:50s} {WORST[k]:.4f}")

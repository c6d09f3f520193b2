"""GPU: the LoRA adapter kernels and their dropout flags, ELEMENT BY ELEMENT against float64 (tests/ref64.py, checked on the CPU in
tests/test_ref64.py), on every dispatch path of csrc/lora.hip plus ur_gemm's masked rank-r epilogue.  Before each launch of
ur_lora_project / _reduce / _bgrad the library is asked (hip.lora_plan, for the very tensors of the launch, on this device) which kernel
it takes: the one the case's label names.

Flags.  ur_lora_dropout_bits is compared BYTE FOR BYTE with the numpy twin oracle/dropout_ref.lora_words (layout and zero padding words
included), hip.lora_bits_to_keep with dropout_ref.lora_keep, ur_lora_bits_transpose with a numpy repack.  Every keep mask the kernel
tests use comes from dropout_ref.lora_keep, and each of those tests first asserts that the planes it hands to the kernel equal the twin's.

Criteria (docs/lab_notes.md, "Element-wise float64 tests: LoRA kernels and their dropout flags"):
  bf16 outputs t / tb / C     |got - ref64| <= 1 bf16 ulp(ref64) + 2^-20 * |alpha| sum |term| + 8 * |ref32 - ref64|   (ref64.assert_lora_bf16)
  f32 outputs dA / dB         |got - ref64| <= 8 * |ref32 - ref64| + 2^-20 * sum |term|                             (ref64.assert_colsum_close)
  exact family                small-integer inputs, power-of-two alpha, p = 0.5: every f32 partial sum is exact in any order and the
                              output equals the correctly rounded exact value BIT FOR BIT                            (ref64.assert_lora_exact)
ref32 = the same formula in float32 torch on the CPU.  No element is exempt.  Every output is pre-filled with a sentinel and must be
written and finite where it belongs and untouched in the pad columns of a wider row stride; a second call must be bit-identical.
The fused kernels' projection is referred to the h / act BITS THE KERNEL WROTE (the MFMA operand is that bf16 value), after those bits
were held to their own criterion.  Every test prints its worst error / bound ("[ratio] kernel: x")."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dropout_ref  # noqa: E402
from tests import lora_cases, norm_cases, ref64  # noqa: E402
from unirec_amd import hip  # noqa: E402

# entry point -> the primitive-level tests of this module that hold it against a reference (tests/test_abi_test_coverage.py)
COVERS = {
    "ur_lora_dropout_bits": ["test_flag_bytes_equal_the_numpy_twin", "test_flag_bytes_second_grid_slice"],
    "ur_lora_bits_transpose": ["test_token_packed_flags_equal_a_numpy_repack"],
    "ur_lora_project": ["test_project_register_staged", "test_project_column_ranges", "test_project_ring"],
    "ur_lora_reduce": ["test_reduce_register_staged", "test_reduce_ring", "test_reduce_column_ranges_transposed"],
    "ur_lora_bgrad": ["test_bgrad_register_staged", "test_bgrad_ring_512", "test_bgrad_ring_1024"],
    "ur_rmsnorm_lora_fwd": ["test_fused_rmsnorm_lora_projection"],
    "ur_swiglu_lora_fwd": ["test_fused_swiglu_lora_projection"],
    "ur_gemm": ["test_masked_gemm_epilogue_generic"],
}

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENTINEL = 0x4B4B                    # a finite bf16 bit pattern (13303808.0) nothing here computes
WORST = {}


def _note(kernel, ratio):
    WORST[kernel] = max(WORST.get(kernel, 0.0), float(ratio))
    print(f"[ratio] {kernel}: {float(ratio):.4f}")


# =============================================================================================================================
# flags
def _words_of(bits):
    """uint32 [nad, M, ld / 4] view of the device planes' raw bytes, on the CPU"""
    return bits.cpu().contiguous().view(torch.int32)


def _twin_words(seed, p, M, W, nad, row0=0):
    return torch.from_numpy(dropout_ref.lora_words(seed, p, M, W, nad, row0).view(np.int32))


SEED_HI = (0x9E37 << 32) | 0x0123_4567
FLAG_P = [0.1, 0.25, 0.3, 0.5, 2.0 ** -15, 0.99999]


@pytest.mark.parametrize("p", FLAG_P)
@pytest.mark.parametrize("W", [8, 40, 128, 136, 1024, 3072])
def test_flag_bytes_equal_the_numpy_twin(W, p):
    """raw bytes and the library's unpacker, M in {1, 33, 300}, 1 .. 4 planes, seeds with and without a high word, row0 in {0, 77, 2^33}"""
    for M, nad, seed, row0 in ((1, 1, 5, 0), (33, 2, SEED_HI, 77), (300, 3, 12345, 2 ** 33), (33, 4, SEED_HI + 1, 0)):
        if W == 3072 and M == 300 and p not in (0.1, 0.5):
            continue                                       # (the twin's cost, not the kernel's: two thresholds at the largest shape)
        bits = torch.full((nad, M, hip.lora_bits_ld(W)), 0xA5, dtype=torch.uint8, device=DEV)
        hip.lora_dropout_bits(seed, p, M, W, nad, DEV, out=bits, row0=row0)
        assert dropout_ref.lora_bits_ld(W) == hip.lora_bits_ld(W)
        assert torch.equal(_words_of(bits), _twin_words(seed, p, M, W, nad, row0)), f"W{W} p{p} M{M} nad{nad}"
        keep = torch.from_numpy(dropout_ref.lora_keep(seed, p, M, W, nad, row0))
        assert torch.equal(hip.lora_bits_to_keep(bits, W).cpu(), keep)


def test_flag_bytes_second_grid_slice():
    """W = 8, M = 2^20 + 5: rows past 2^20 belong to the second blockIdx.y slice"""
    M, W, p, seed = 2 ** 20 + 5, 8, 0.3, SEED_HI
    bits = hip.lora_dropout_bits(seed, p, M, W, 1, DEV)
    assert torch.equal(_words_of(bits), _twin_words(seed, p, M, W, 1))


@pytest.mark.parametrize("W", [8, 40, 64, 136, 202])
@pytest.mark.parametrize("M,nad", [(32, 1), (128, 3), (416, 4)])
def test_token_packed_flags_equal_a_numpy_repack(M, nad, W):
    if W % 8:
        W_bits = (W + 7) // 8 * 8                          # the planes of a [M, 208] input; the token-packed copy is asked for W = 202 columns
    else:
        W_bits = W
    seed, p = 31 + W, 0.3
    bits = hip.lora_dropout_bits(seed, p, M, W_bits, nad, DEV)
    words = dropout_ref.lora_words(seed, p, M, W_bits, nad)
    assert torch.equal(_words_of(bits), torch.from_numpy(words.view(np.int32)))
    ldt = hip.lora_bits_t_ld(W)
    out = torch.full((nad, M // 32, ldt), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    bt = hip.lora_bits_transpose(bits, W, out=out)
    want = dropout_ref.lora_words_transposed(words, W)
    assert want.shape == (nad, M // 32, ldt)
    assert torch.equal(bt.cpu(), torch.from_numpy(want.view(np.int32)))


# =============================================================================================================================
# helpers of the kernel tests
def _bits16(t):
    return t.contiguous().view(torch.int16)


def _wide(t, pad=8):
    """device copy of a CPU [M, W] tensor as a view of a tensor `pad` columns wider (ld != width)"""
    base = torch.zeros((t.shape[0], t.shape[1] + pad), dtype=t.dtype, device=DEV)
    base[:, :t.shape[1]] = t.to(DEV)
    return base[:, :t.shape[1]]


def _planes(c, W=None):
    """the device planes of case c -- drawn by ur_lora_dropout_bits with the case's seed, p and row0 and compared with the numpy twin's
    words before any kernel sees them (c['keep'] is the twin's unpacking of the same words) -- or None"""
    if c["keep"] is None:
        return None
    W = c["W"] if W is None else W
    bits = hip.lora_dropout_bits(c["seed"], c["p"], c["M"], W, c["nad"], DEV, row0=c["row0"])
    assert torch.equal(_words_of(bits), _twin_words(c["seed"], c["p"], c["M"], W, c["nad"], c["row0"])), "planes differ from the numpy twin"
    return bits


def _sentinel_bf16(M, n, pad=4):
    """(the [M, n] output view, its [M, n + pad] base) filled with SENTINEL"""
    base = torch.full((M, n + pad), SENTINEL, dtype=torch.int16, device=DEV).view(BF16)
    return base[:, :n], base


def _written(out, base, what):
    """every element of the view written and finite, the pad columns of the wider row untouched"""
    n = out.shape[1]
    assert not (_bits16(out) == SENTINEL).any(), f"{what}: elements left unwritten"
    assert torch.isfinite(out.float()).all(), f"{what}: non-finite outputs"
    assert (_bits16(base[:, n:]) == SENTINEL).all(), f"{what}: pad columns of the wider row were written"


def _hold_bf16(name, c, got, ref, what):
    """ref(dtype=..., absolute=...) -> the reference of the output `got` (device bf16)"""
    r64 = ref()
    if c["family"] == "exact":
        _note(name + " (exact)", ref64.assert_lora_exact(got.cpu(), r64, what))
    else:
        _note(name, ref64.assert_lora_bf16(got.cpu(), r64, ref(dtype=F32), ref(absolute=True), what))


def _hold_f32(name, c, got, ref, what):
    r64 = ref()
    g = got.detach().cpu().reshape(-1)
    assert torch.isfinite(g).all(), f"{what}: unwritten (NaN pre-fill) or non-finite outputs"
    if c["family"] == "exact":
        _note(name + " (exact)", ref64.assert_lora_exact(g, r64, what))
    else:
        _note(name, ref64.assert_colsum_close(g, r64, ref(dtype=F32), ref(absolute=True), what))


def _tag(c):
    return f"{c['path']} {c['family']} r{c['rank']} nad{c['nad']} M{c['M']} W{c['W']} p{c['p']} row0 {c['row0']}" + (f" cols{c['cols']}" if c["cols"] else "")


def _takes(op, args, c):
    """the library's own answer (hip.lora_plan on this device) for the LoraArgs of the launch under test is the kernel c's label names"""
    plan = hip.lora_plan(op, args)
    assert plan["kernel"] == lora_cases.kernel_of(c["path"]), f"{_tag(c)}: the launch takes {plan}"


def _run_project(c):
    what = _tag(c)
    X, U, bits = _wide(c["X"]), [u.to(DEV) for u in c["U"]], _planes(c)
    out, base = _sentinel_bf16(c["M"], c["rank"] * c["nad"])
    _takes("project", hip.lora_project_args(X, U, cols=c["cols"], alpha=c["alpha"], bits=bits, out=out)[0], c)
    hip.lora_project(X, U, cols=c["cols"], alpha=c["alpha"], bits=bits, out=out)
    _written(out, base, what)
    _hold_bf16("lora_project " + c["path"], c, out, lambda **k: ref64.lora_project(c["X"], c["U"], c["keep"], c["alpha"], c["cols"], **k), what)
    again, _ = _sentinel_bf16(c["M"], c["rank"] * c["nad"])
    hip.lora_project(X, U, cols=c["cols"], alpha=c["alpha"], bits=bits, out=again)
    assert torch.equal(_bits16(out), _bits16(again)), f"{what}: a second call differs"


def _run_reduce(c, with_bits_t=False):
    what = _tag(c)
    X, V, bits = _wide(c["X"]), _wide(c["V"]), _planes(c)
    transposed = bool(c.get("transposed", False))
    bt = None
    if with_bits_t and bits is not None:
        bt = hip.lora_bits_transpose(bits, c["W"])
        want = dropout_ref.lora_words_transposed(dropout_ref.lora_words(c["seed"], c["p"], c["M"], c["W"], c["nad"], c["row0"]), c["W"])
        assert torch.equal(bt.cpu(), torch.from_numpy(want.view(np.int32))), f"{what}: token-packed planes differ from the numpy repack"
    n = c["rank"] * sum(w for _, w in (c["cols"] or [(0, c["W"])] * c["nad"]))
    kw = dict(cols=c["cols"], nad=c["nad"], alpha=c["alpha"], bits=bits, transposed=transposed, bits_t=bt)
    outs = []
    for _ in range(2):
        out = torch.full((n,), float("nan"), device=DEV)
        if not outs:
            _takes("reduce", hip.lora_reduce_args(X, V, out, **kw), c)
        hip.lora_reduce(X, V, out, **kw)
        outs.append(out)
    _hold_f32("lora_reduce " + c["path"], c, outs[0],
              lambda **k: ref64.lora_reduce(c["X"], c["V"], c["rank"], c["nad"], c["keep"], c["alpha"], c["cols"], transposed, **k), what)
    assert torch.equal(outs[0], outs[1]), f"{what}: a second call differs"
    return outs[0]


def _run_bgrad(c):
    what = _tag(c)
    dy, t, Bt = _wide(c["X"]), _wide(c["V"]), [u.to(DEV) for u in c["U"]]
    n = c["rank"] * sum(w for _, w in c["cols"])
    res = []
    for _ in range(2):
        out, base = _sentinel_bf16(c["M"], c["rank"] * c["nad"])
        gB = torch.full((n,), float("nan"), device=DEV)
        if not res:
            _takes("bgrad", hip.lora_bgrad_args(dy, t, Bt, c["cols"], gB, alpha=c["alpha"], out=out)[0], c)
        hip.lora_bgrad(dy, t, Bt, c["cols"], gB, alpha=c["alpha"], out=out)
        _written(out, base, what)
        res.append((out, gB))
    ref = lambda i: (lambda **k: ref64.lora_bgrad(c["X"], c["V"], c["U"], c["cols"], c["alpha"], **k)[i])      # noqa: E731
    _hold_bf16("lora_bgrad tb " + c["path"], c, res[0][0], ref(0), what + " tb")
    _hold_f32("lora_bgrad dB " + c["path"], c, res[0][1], ref(1), what + " dB")
    assert torch.equal(_bits16(res[0][0]), _bits16(res[1][0])) and torch.equal(res[0][1], res[1][1]), f"{what}: a second call differs"


# =============================================================================================================================
# ur_lora_project
@pytest.mark.parametrize("nad", [1, 2, 3, 4])
@pytest.mark.parametrize("rank", lora_cases.RANKS)
def test_project_register_staged(rank, nad):
    """ranks 8 .. 64 x 1 .. 4 adapters that share X (4 x rank 32: one LDS slot; 4 x rank 64: 64 tokens per workgroup), masked and not,
    M in {1, 31, 129, 257}, W in {8, 120, 128, 136, 392}, ld != width, both families"""
    for c in lora_cases.project_staged(rank, nad):
        _run_project(c)


@pytest.mark.parametrize("rank", lora_cases.RANKS)
def test_project_column_ranges(rank):
    """adapters that own column ranges of X (no range starts at 0, a ragged width): one row of workgroups per adapter"""
    for c in lora_cases.project_ranges(rank):
        _run_project(c)


def test_project_ring():
    """rank 16, one adapter or column ranges with every width % 64 == 0 (a range that does not start at 0), W in {64, 192, 1024},
    M in {1, 255, 256, 257, 513}, masked and not"""
    for c in lora_cases.project_ring():
        _run_project(c)


# =============================================================================================================================
# ur_lora_reduce
@pytest.mark.parametrize("nad", [1, 2, 3, 4])
@pytest.mark.parametrize("rank", lora_cases.RANKS)
def test_reduce_register_staged(rank, nad):
    """M in {1, 37, 127, 129, 300} (one split .. three), W in {8, 64, 72, 200}, masked and not, both families"""
    for c in lora_cases.reduce_staged(rank, nad):
        _run_reduce(c)


@pytest.mark.parametrize("rank", lora_cases.RANKS)
def test_reduce_column_ranges_transposed(rank):
    for c in lora_cases.reduce_ranges(rank):
        _run_reduce(c)


@pytest.mark.parametrize("nad", [1, 2, 3, 4])
def test_reduce_ring(nad):
    """rank 16, M in {128, 384, 1024}, W in {64, 192}: masked with the token-packed flags and unmasked; and the ring-eligible shape that
    comes with bits but without bits_t, which must run the register-staged kernel (same flags: the same sums up to the order)"""
    for c in lora_cases.reduce_ring(nad):
        _run_reduce(c, with_bits_t=True)
    for c in lora_cases.reduce_ring_fallback(nad):
        _run_reduce(c, with_bits_t=False)
    if nad == 1:
        for c in lora_cases.reduce_ring_ranges():
            _run_reduce(c)


# =============================================================================================================================
# ur_lora_bgrad
@pytest.mark.parametrize("rank", lora_cases.RANKS)
def test_bgrad_register_staged(rank):
    """every rank, one width of 72, M = the kernel's tokens per block (the plan's tok_per_block) - 1, + 0, + 1"""
    for c in lora_cases.bgrad_staged(rank):
        _run_bgrad(c)


def test_bgrad_ring_512():
    for c in lora_cases.bgrad_ring_512():
        _run_bgrad(c)


def test_bgrad_ring_1024():
    """four 64-wide adapters, M = the smallest row count that gives every CU a 1024-token block, + 37"""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    for c in lora_cases.bgrad_ring_1024(cu):
        assert -(-c["M"] // 1024) * 4 >= cu > -(-(c["M"] - 38) // 1024) * 4
        _run_bgrad(c)


# =============================================================================================================================
# fused kernels: the projection of the h / act bits the kernel wrote
RMS_EPS = 1e-6


@pytest.mark.parametrize("nad,p", [(2, 0.0), (3, 0.0), (2, 0.1), (3, 0.3)])
@pytest.mark.parametrize("M", [1, 63, 65, 200])
def test_fused_rmsnorm_lora_projection(M, nad, p):
    D = 1024
    c = lora_cases.fused_case(M, D, nad, p, seed=900 + M + nad, row0=(0, lora_cases.ROW0_BIG)[M % 2])
    c["path"] = "rmsnorm_lora_fwd"
    what = _tag(c)
    x, w = norm_cases.rows(M, D, 40 + M), norm_cases.norm_weight(D, 41 + M)
    U, bits = [u.to(DEV) for u in c["U"]], _planes(c)
    t, base = _sentinel_bf16(M, 16 * nad)
    h, rstd, _ = hip.rmsnorm_lora_fwd(x.to(DEV), w.to(DEV), RMS_EPS, U, alpha=c["alpha"], bits=bits, t_out=t)
    _written(t, base, what + " t")
    r64, r32 = ref64.rmsnorm_fwd(x, w, RMS_EPS), ref64.rmsnorm_fwd(x, w, RMS_EPS, dtype=F32)
    _note("rmsnorm_lora_fwd h", ref64.assert_bf16_rows(h.cpu(), r64[0], r32[0], what + " h"))
    hs = h.cpu()
    assert t.shape == (M, 16 * nad)
    _note("rmsnorm_lora_fwd t", ref64.assert_lora_bf16(t.cpu(), ref64.rms_lora_t(hs, c["U"], c["keep"], c["alpha"]),
                                                        ref64.rms_lora_t(hs, c["U"], c["keep"], c["alpha"], dtype=F32),
                                                        ref64.rms_lora_t(hs, c["U"], c["keep"], c["alpha"], absolute=True), what + " t"))
    h2, _, t2 = hip.rmsnorm_lora_fwd(x.to(DEV), w.to(DEV), RMS_EPS, U, alpha=c["alpha"], bits=bits)
    assert torch.equal(_bits16(t), _bits16(t2)) and torch.equal(_bits16(h), _bits16(h2)), f"{what}: a second call differs"


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("I", [128, 384])
@pytest.mark.parametrize("M", [1, 127, 129, 300])
def test_fused_swiglu_lora_projection(M, I, p):
    c = lora_cases.fused_case(M, I, 1, p, seed=950 + M + I, row0=(0, 77)[M % 2])
    c["path"] = "swiglu_lora_fwd"
    what = _tag(c)
    gu = (torch.randn((M, 2 * I), generator=lora_cases.gen(60 + M + I)) * 2.0).to(BF16)
    U, bits = c["U"][0].to(DEV), _planes(c)
    t, base = _sentinel_bf16(M, 16)
    act, _ = hip.swiglu_lora_fwd(gu.to(DEV), I, U, alpha=c["alpha"], bits=bits, t_out=t)
    _written(t, base, what + " t")
    a64 = ref64.swiglu_fwd(gu[:, :I], gu[:, I:])
    _note("swiglu_lora_fwd act", ref64.assert_within_ulps(act.cpu(), a64, 1, 0.0, what + " act"))
    ac = act.cpu()
    args = (ac, c["U"][0], c["keep"], c["alpha"])
    assert t.shape == (M, 16)
    _note("swiglu_lora_fwd t", ref64.assert_lora_bf16(t.cpu(), ref64.swiglu_lora_t(*args), ref64.swiglu_lora_t(*args, dtype=F32),
                                                       ref64.swiglu_lora_t(*args, absolute=True), what + " t"))
    act2, t2 = hip.swiglu_lora_fwd(gu.to(DEV), I, U, alpha=c["alpha"], bits=bits)
    assert torch.equal(_bits16(t), _bits16(t2)) and torch.equal(_bits16(act), _bits16(act2)), f"{what}: a second call differs"


# =============================================================================================================================
# ur_gemm: the masked rank-r epilogue on the generic launch
@pytest.mark.parametrize("nad", [1, 2, 3])
@pytest.mark.parametrize("rank", lora_cases.RANKS)
def test_masked_gemm_epilogue_generic(rank, nad):
    """C = R S^T + sum_a keep_a / (1 - p) (tb_a A_a): N in {136, 264}, M in {1, 200}, K = 64; exact at p = 0.5, random at p = 0.1"""
    for c in lora_cases.epilogue_cases(rank, nad):
        what = f"{c['path']} {c['family']} r{rank} nad{nad} M{c['M']} N{c['N']} p{c['p']} row0 {c['row0']}"
        bits = _planes(c, W=c["N"])
        R, S, tb = c["R"].to(DEV), c["S"].to(DEV), c["tb"].to(DEV)
        S2 = hip.transpose_bf16(c["A"].to(DEV))
        outs = []
        for _ in range(2):
            out, base = _sentinel_bf16(c["M"], c["N"], pad=8)
            hip.gemm(R, S, R2=tb, S2=S2, drop=(bits, c["p"], rank), out=out)
            _written(out, base, what)
            outs.append(out)
        _hold_bf16("gemm masked epilogue", c, outs[0],
                   lambda **k: ref64.lora_masked_epilogue(c["R"], c["S"], c["tb"], c["A"], c["keep"], c["p"], rank, **k), what)
        assert torch.equal(_bits16(outs[0]), _bits16(outs[1])), f"{what}: a second call differs"


def test_zz_worst_ratio_table():
    """prints the worst observed error / bound per kernel and path over the tests of this module that ran before it (docs/lab_notes.md)"""
    print("\n[table] worst error / bound per kernel and path")
    for k in sorted(WORST):
        print(f"[table] {k:50s} {WORST[k]:.4f}")

"""GPU: the head, RoPE, pool and data primitives of include/unirec_hip.h, ELEMENT BY ELEMENT against the float64 references of
tests/ref64.py (themselves checked on the CPU in tests/test_ref64.py), at the shapes and edges where each kernel branches.

Criteria (tests/ref64.py; derivations in docs/lab_notes.md, "Element-wise float64 tests"):
  bf16 outputs computed in f32 and rounded once   |got - ref| <= 1 bf16 ulp + 2^-18 * (row max |ref|, or the named product scale)
  f32 outputs                                      per row  max |got - ref| <= 8 * e32 + 2^-20 * scale, e32 = what the same formula costs in
                                                   float32 torch on the CPU
  integer-valued sums, gathers, ranks, top-K       exact
No element is exempt.  Every test prints its worst error / bound ("[ratio] kernel: x"); test_zz_worst_ratio_table prints the table.

Not specified by the header and therefore not tested: NaN scores in ur_mrr_rank / ur_rank_of_index / ur_topk, and gt_index outside
[0, N) in ur_rank_of_index.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import ref64  # noqa: E402
from unirec_amd import _lib, hip  # noqa: E402

# entry point -> the primitive-level tests of this module that hold it against a reference (tests/test_abi_test_coverage.py)
COVERS = {
    "ur_rope_table": ["test_rope_table"],
    "ur_qknorm_rope_fwd": ["test_qknorm_rope_fwd", "test_qknorm_rope_grid_stride"],
    "ur_qknorm_rope_bwd": ["test_qknorm_rope_bwd", "test_qknorm_rope_grid_stride"],
    "ur_qknorm_rope_bwd_roped": ["test_qknorm_rope_bwd_roped"],
    "ur_qknorm_rope_bwd_roped_k": ["test_qknorm_rope_bwd_roped_k"],
    "ur_embed_inject_fwd": ["test_embed_inject_fwd_and_bwd"],
    "ur_inject_bwd": ["test_embed_inject_fwd_and_bwd", "test_inject_rejects_wide_rows"],
    "ur_mean_pool_fwd": ["test_mean_pool_fwd"],
    "ur_mean_pool_bwd": ["test_mean_pool_bwd"],
    "ur_user_sequence_assemble": ["test_user_sequence_assemble"],
    "ur_dropout_keep": ["test_user_sequence_assemble"],
    "ur_cosine_scores": ["test_cosine_scores"],
    "ur_catalog_scores": ["test_catalog_scores"],
    "ur_infonce_fwd_bwd": ["test_infonce_fwd_bwd"],
    "ur_mrr_rank": ["test_ranks_and_topk_are_exact"],
    "ur_rank_of_index": ["test_ranks_and_topk_are_exact"],
    "ur_topk": ["test_ranks_and_topk_are_exact"],
    "ur_recon_stats": ["test_recon_stats_and_grad"],
    "ur_recon_grad": ["test_recon_stats_and_grad"],
    "ur_triplet_margin": ["test_triplet_margin"],
    "ur_mse_loss": ["test_mse_loss"],
    "ur_gelu_bwd": ["test_gelu_bwd_exhaustive"],
    "ur_swiglu_fwd": ["test_swiglu_exhaustive", "test_swiglu_shapes"],
    "ur_swiglu_bwd": ["test_swiglu_exhaustive", "test_swiglu_shapes"],
    "ur_context_mlp1": ["test_context_mlp1"],
}

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENTINEL = 0x4B4B                    # a finite bf16 bit pattern nothing computes by accident
WORST = {}


def _note(kernel, ratio):
    WORST[kernel] = max(WORST.get(kernel, 0.0), float(ratio))
    print(f"[ratio] {kernel}: {float(ratio):.4f}")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=_gen(seed)) * scale


def _ints(shape, seed, lo=-3, hi=4):
    return torch.randint(lo, hi, shape, generator=_gen(seed)).float()


def _norm_weight(hd, seed):
    """+-[0.25, 4], log-uniform, a third of them negative: far from the 1.0 every model-level test runs with"""
    g = _gen(seed)
    mag = torch.exp2(torch.rand(hd, generator=g) * 4.0 - 2.0)
    sign = torch.where(torch.rand(hd, generator=g) < 1.0 / 3.0, -1.0, 1.0)
    return (mag * sign).float()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _sentinel(shape):
    return torch.full(shape, SENTINEL, dtype=torch.int16, device=DEV).view(BF16)


def _rejected(fn, who):
    """fn() must fail with a NEGATIVE return code (argument check, nothing launched) and a message naming the entry point"""
    with pytest.raises(_lib.UniRecHipError) as e:
        fn()
    msg = str(e.value)
    assert "rc=-" in msg and who in msg.split("):", 1)[-1], msg


# =============================================================================================================================
# RoPE table
@pytest.mark.parametrize("theta", [1e4, 1e6])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("S", [1, 257, 4096])
def test_rope_table(S, hd, theta):
    """|err| <= pos * 2^-21 + 2^-22: ~8 f32 ulps of accumulated relative error in the angle (powf, reciprocal, product) times the angle
    (<= pos), plus the rounding of cos / sin themselves."""
    cos, sin = hip.rope_table(S, hd, theta, DEV)
    rc, rs = ref64.rope_table(S, hd, theta)
    bound = torch.arange(S, dtype=F64)[:, None] * 2.0 ** -21 + 2.0 ** -22
    worst = 0.0
    for name, got, ref in (("cos", cos, rc), ("sin", sin, rs)):
        got = got.cpu().to(F64)
        assert got.shape == ref.shape and torch.isfinite(got).all()
        ratio = (got - ref).abs() / bound
        i = tuple(int(v) for v in torch.unravel_index(ratio.argmax(), ratio.shape))
        assert ratio[i] <= 1.0, f"{name}[{i}]: got {got[i].item()!r}, reference {ref[i].item()!r}, {ratio[i].item():.2f} x the bound; " \
                                f"{int((ratio > 1).sum())} offenders"
        worst = max(worst, float(ratio.max()))
    _note("rope_table", worst)


# =============================================================================================================================
# q/k RMSNorm + RoPE from the raw projection
HEADS = [(16, 8), (3, 2), (1, 1), (0, 3), (5, 1)]           # nq + nkv = 0, 1, 2, 3 mod 4 and the k heads alone
TOKENS = [(1, 1), (15, 4), (16, 16), (33, 7), (33, 1), (1000, 333)]      # (M, S): S not dividing M, S = 1
EPS = 1e-6


def _rope_case(M, S, nq, nkv, hd, seed):
    """raw = a column slice of a wider buffer (ldraw > packed width)"""
    ncols = (nq + 2 * nkv) * hd
    wide = _randn((M, ncols + 24), seed, 3.0).to(BF16).to(DEV)
    raw = wide[:, 8:8 + ncols]
    qw, kw = _norm_weight(hd, seed + 1), _norm_weight(hd, seed + 2)
    cos, sin = hip.rope_table(S, hd, 1e6, DEV)
    return raw, qw, kw, cos, sin


def _split_heads(q, k, M, nq, nkv, hd):
    return torch.cat([q.reshape(M, nq, hd), k.reshape(M, nkv, hd)], dim=1)


def _check_rope_fwd(M, S, nq, nkv, hd, seed=100):
    raw, qw, kw, cos, sin = _rope_case(M, S, nq, nkv, hd, seed)
    q, k = hip.qknorm_rope_fwd(raw, qw.to(DEV), kw.to(DEV), cos, sin, S, nq, nkv, hd, EPS)
    got = _split_heads(q.cpu(), k.cpu(), M, nq, nkv, hd)
    ref = ref64.qknorm_rope_fwd(raw.cpu(), qw, kw, cos.cpu(), sin.cpu(), S, nq, nkv, hd, float(torch.tensor(EPS, dtype=F32)))
    _note(f"qknorm_rope_fwd hd{hd}", ref64.assert_within_ulps(got, ref, 1, 2.0 ** -18 * ref64.rowmax(ref), f"rope fwd M{M} S{S} {nq}+{nkv} hd{hd}"))


def _check_rope_bwd(M, S, nq, nkv, hd, seed=200):
    raw, qw, kw, cos, sin = _rope_case(M, S, nq, nkv, hd, seed)
    nh, ncols = nq + nkv, (nq + 2 * nkv) * hd
    dq = _randn((M, nq * hd), seed + 3).to(BF16).to(DEV)
    dk = _randn((M, nkv * hd), seed + 4).to(BF16).to(DEV)
    if nq == 0:
        dq = dk                                                  # (never read: any valid pointer)
    wide = _sentinel((M, ncols + 16))
    draw = wide[:, 8:8 + ncols]
    hip.qknorm_rope_bwd(dq, dk, raw, qw.to(DEV), kw.to(DEV), cos, sin, draw, S, nq, nkv, hd, EPS)
    out = wide.cpu()
    dout = _split_heads(dq.cpu()[:, :nq * hd], dk.cpu(), M, nq, nkv, hd)
    ref = ref64.qknorm_rope_bwd(dout, raw.cpu(), qw, kw, cos.cpu(), sin.cpu(), S, nq, nkv, hd, float(torch.tensor(EPS, dtype=F32)))
    got = out[:, 8:8 + nh * hd].reshape(M, nh, hd)
    _note(f"qknorm_rope_bwd hd{hd}", ref64.assert_within_ulps(got, ref, 1, 2.0 ** -18 * ref64.rowmax(ref), f"rope bwd M{M} S{S} {nq}+{nkv} hd{hd}"))
    untouched = torch.cat([out[:, :8], out[:, 8 + nh * hd:]], dim=1)
    assert (_bits(untouched) == SENTINEL).all(), "the v columns / padding of dqkv_raw were written"


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("M,S", TOKENS)
@pytest.mark.parametrize("nq,nkv", HEADS)
def test_qknorm_rope_fwd(nq, nkv, M, S, hd):
    _check_rope_fwd(M, S, nq, nkv, hd)


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("M,S", TOKENS)
@pytest.mark.parametrize("nq,nkv", HEADS)
def test_qknorm_rope_bwd(nq, nkv, M, S, hd):
    _check_rope_bwd(M, S, nq, nkv, hd)


@pytest.mark.parametrize("hd,M,nq,nkv", [(128, 65536 + 16 + 3, 1, 1), (128, 65536 + 16 + 3, 0, 3), (64, 2 * 65536 + 32 + 3, 1, 1)])
def test_qknorm_rope_grid_stride(hd, M, nq, nkv):
    """more than 4096 workgroups of 256 / (hd / 8) tokens: the kernel strides over its grid"""
    assert (M + 256 // (hd // 8) - 1) // (256 // (hd // 8)) > 4096
    _check_rope_fwd(M, 4096, nq, nkv, hd, seed=300)
    _check_rope_bwd(M, 4096, nq, nkv, hd, seed=310)


# ---- the same backward from the ROPED output + 1 / rms (the forward ran as the q|k|v GEMM's epilogue) -----------------------
def _roped_case(M, S, nq, nkv, seed):
    hd = 128
    raw, qw, kw, cos, sin = _rope_case(M, S, nq, nkv, hd, seed)
    q_r, k_r = hip.qknorm_rope_fwd(raw, qw.to(DEV), kw.to(DEV), cos, sin, S, nq, nkv, hd, EPS)
    eps = float(torch.tensor(EPS, dtype=F32))
    rstd = ref64.qknorm_rope_rstd(raw.cpu(), nq, nkv, hd, eps).to(F32)            # float64 from the raw rows, cast to f32
    return raw, qw, kw, cos, sin, q_r, k_r, rstd, eps


def _check_roped(got, dout, roped, rstd, raw, qw, kw, cos, sin, S, nq, nkv, eps, what):
    """against the float64 formula over the kernel's own inputs (1 ulp), and against the TRUE gradient of the raw projection: the kernel
    reconstructs x^ from bf16-rounded outputs, which costs e_rt = |formula(bf16 roped, f32 rstd) - true| per row, measured here"""
    hd = 128
    true = ref64.qknorm_rope_bwd(dout, raw.cpu(), qw, kw, cos.cpu(), sin.cpu(), S, nq, nkv, hd, eps)
    recon = ref64.qknorm_rope_bwd_from_roped(dout, roped, rstd, qw, kw, cos.cpu(), sin.cpu(), S, nq, nkv, hd)
    e_rt = (recon - true).abs().amax(dim=-1, keepdim=True)
    _note(what, ref64.assert_within_ulps(got, recon, 1, 2.0 ** -18 * ref64.rowmax(recon), what + " vs the formula over its inputs"))
    _note(what + " (true gradient)", ref64.assert_within_ulps(got, true, 1, 2.0 * e_rt + 2.0 ** -18 * ref64.rowmax(true), what + " vs the true gradient"))
    rel = float((e_rt / ref64.rowmax(true).clamp_min(1e-300)).max())
    print(f"[e_rt] {what}: max e_rt / rowmax = {rel:.3e}")
    WORST["e_rt / rowmax (" + what + ")"] = max(WORST.get("e_rt / rowmax (" + what + ")", 0.0), rel)


BIG = (65536 + 16 + 3, 4096)                                     # the grid-stride size runs with one small head count only


@pytest.mark.parametrize("nq,nkv,M,S", [(nq, nkv, M, S) for nq, nkv in HEADS if nq > 0 for M, S in TOKENS] + [(1, 1) + BIG])
def test_qknorm_rope_bwd_roped(nq, nkv, M, S):
    hd, nh = 128, nq + nkv
    raw, qw, kw, cos, sin, q_r, k_r, rstd, eps = _roped_case(M, S, nq, nkv, 400)
    dq = _randn((M, nq * hd), 403).to(BF16).to(DEV)
    dk = _randn((M, nkv * hd), 404).to(BF16).to(DEV)
    ncols = (nq + 2 * nkv) * hd
    wide = _sentinel((M, ncols + 16))
    hip.qknorm_rope_bwd_roped(dq, dk, q_r, k_r, rstd.to(DEV), qw.to(DEV), kw.to(DEV), cos, sin, wide[:, 8:8 + ncols], S, nq, nkv, hd)
    out = wide.cpu()
    dout = _split_heads(dq.cpu(), dk.cpu(), M, nq, nkv, hd)
    roped = _split_heads(q_r.cpu(), k_r.cpu(), M, nq, nkv, hd)
    _check_roped(out[:, 8:8 + nh * hd].reshape(M, nh, hd), dout, roped, rstd, raw, qw, kw, cos, sin, S, nq, nkv, eps, "qknorm_rope_bwd_roped")
    untouched = torch.cat([out[:, :8], out[:, 8 + nh * hd:]], dim=1)
    assert (_bits(untouched) == SENTINEL).all(), "the v columns / padding of dqkv_raw were written"


@pytest.mark.parametrize("nq,nkv,M,S", [(nq, nkv, M, S) for nq, nkv in HEADS for M, S in TOKENS] + [(1, 1) + BIG])
def test_qknorm_rope_bwd_roped_k(nq, nkv, M, S):
    """the k heads alone: row constants at rstd[m, h0 + h] with h0 > 0 and a row stride wider than nkv; k_roped and dk_raw strided"""
    hd = 128
    raw, qw, kw, cos, sin, q_r, k_r, rstd, eps = _roped_case(M, S, nq, nkv, 500)
    h0 = nq + 2                                                  # the k constants sit behind the q heads' and two unused columns
    rs_wide = torch.full((M, nq + nkv + 5), float("nan"))
    rs_wide[:, h0:h0 + nkv] = rstd[:, nq:]
    k_wide = _sentinel((M, nkv * hd + 16))
    k_wide[:, 8:8 + nkv * hd] = k_r
    dk = _randn((M, nkv * hd), 504).to(BF16).to(DEV)
    out_wide = _sentinel((M, nkv * hd + 24))
    hip.qknorm_rope_bwd_roped_k(dk, k_wide[:, 8:8 + nkv * hd], rs_wide.to(DEV), h0, kw.to(DEV), cos, sin, out_wide[:, 16:16 + nkv * hd], S, nkv, hd)
    out = out_wide.cpu()
    # reference: the k heads are heads nq.. of the full problem; evaluate it with nq = 0 over the k columns
    raw_k = raw.cpu()[:, nq * hd:(nq + nkv) * hd]
    dout = dk.cpu().reshape(M, nkv, hd)
    _check_roped(out[:, 16:16 + nkv * hd].reshape(M, nkv, hd), dout, k_r.cpu().reshape(M, nkv, hd), rstd[:, nq:], raw_k, kw, kw, cos, sin, S, 0, nkv, eps,
                 "qknorm_rope_bwd_roped_k")
    untouched = torch.cat([out[:, :16], out[:, 16 + nkv * hd:]], dim=1)
    assert (_bits(untouched) == SENTINEL).all(), "columns outside dk_raw were written"


# =============================================================================================================================
# embedding gather + token injection
def _inject_ids(B, S, T, first, seed):
    """ordinary ids everywhere, then per sample: token 2 at positions 0 and S - 1, token 1 in 256-position chunks 0 and 2 (none in chunk 1),
    token 0 at up to 300 other positions, tokens 3 .. T - 1 never (truncated away).  S < 8: token 0 at position 0 only."""
    g = _gen(seed)
    ids = torch.randint(0, first, (B, S), generator=g)
    for b in range(B):
        if S < 8:
            ids[b, 0] = first
            continue
        reserved = {0, 5, 700, S - 1}
        free = [int(p) for p in torch.randperm(S, generator=g) if int(p) not in reserved]
        ids[b, free[:min(300, len(free) // 2)]] = first
        if T >= 2:
            ids[b, 5] = first + 1
            if S > 700:
                ids[b, 700] = first + 1
        if T >= 3:
            ids[b, 0] = ids[b, S - 1] = first + 2
    return ids


@pytest.mark.parametrize("B,S,D,T", [(2, 1, 8, 1), (3, 255, 1024, 5), (2, 256, 2048, 5), (2, 257, 2056, 6), (2, 2048, 4096, 5), (9, 2048, 8, 7),
                                     (2, 300, 64, 0)])
def test_embed_inject_fwd_and_bwd(B, S, D, T):
    """forward bit-exact (B * S > 16384 rows takes the grid stride); backward = bf16(exact integer sum) bit for bit: D > 2048 uses the
    second accumulator set, a token present 300 times, matches in different 256-position chunks, truncated tokens exactly zero"""
    first, extra = 64, 8
    V = first + T + extra
    ids = _inject_ids(B, S, max(T, 1), first, 600 + S)
    embed = _randn((V, D), 601).to(BF16)
    tokens = _randn((B, T, D), 602).to(BF16) if T else None
    out = hip.embed_inject_fwd(embed.to(DEV), ids.to(DEV), None if tokens is None else tokens.to(DEV), first).cpu()
    ref = embed[ids]                                             # [B, S, D]
    if T:
        rel = ids - first
        special = (rel >= 0) & (rel < T)
        bidx = torch.arange(B)[:, None].expand(B, S)
        ref = torch.where(special[..., None], tokens[bidx, rel.clamp(0, T - 1)], ref)
        assert special[:, 0].all() or T < 3
    assert torch.equal(_bits(out), _bits(ref)), "embed_inject_fwd is not a bit-exact gather"
    if not T:
        return
    dx = _ints((B, S, D), 603).to(BF16)
    dtok = hip.inject_bwd(dx.to(DEV), ids.to(DEV), first, T).cpu()
    want = torch.zeros(B, T, D, dtype=F64)
    for t in range(T):
        want[:, t] = (dx.to(F64) * (ids == first + t)[..., None]).sum(1)
    assert float(want.abs().max()) < 2 ** 24                     # the f32 sum is exact; the output rounds once
    assert torch.equal(_bits(dtok), _bits(want.to(F32).to(BF16))), f"max err {(dtok.to(F64) - want).abs().max()}"
    assert T < 4 or (_bits(dtok[:, 3:]) == 0).all(), "a truncated token must receive an exactly zero gradient"
    if S >= 900:
        assert int((ids == first).sum(1).min()) == 300


def test_inject_rejects_wide_rows():
    B, S, D, T = 1, 4, 4104, 2
    dx = torch.zeros((B, S, D), dtype=BF16, device=DEV)
    ids = torch.zeros((B, S), dtype=torch.int64, device=DEV)
    _rejected(lambda: hip.inject_bwd(dx, ids, 64, T), "ur_inject_bwd")


# =============================================================================================================================
# mean pool
POOL = [(B, S, D) for S in (1, 2, 15, 16, 17, 100, 2048) for D in (8, 520, 1024) for B in (1, 3, 64) if B * S * D <= 2 ** 25]


@pytest.mark.parametrize("B,S,D", POOL)
def test_mean_pool_fwd(B, S, D):
    """integer inputs: the f32 sum is exact, so the f32 output is within 2 f32 ulps of sum / S (the kernel multiplies by a rounded 1 / S)
    and the bf16 output within 1 bf16 ulp; S < 16 leaves slices of the first stage empty"""
    x = _ints((B, S, D), 700).to(BF16)
    ref = x.to(F32).sum(1).to(F64) / S
    mode = (B + S + D // 8) % 3                                   # f32 only / bf16 only / both
    o32, o16 = hip.mean_pool_fwd(x.to(DEV), out_f32=mode != 1, out_bf16=mode != 0)
    assert (o32 is None) == (mode == 1) and (o16 is None) == (mode == 0)
    if o32 is not None:
        err = (o32.cpu().to(F64) - ref).abs()
        bound = 2.0 * ref64.f32_ulp(ref)
        assert (err <= bound).all(), f"f32 mean: worst {float((err / bound).max()):.2f} x 2 ulp at {int((err / bound).argmax())}"
        _note("mean_pool_fwd f32 (x 2 f32 ulp)", float((err / bound).max()))
    if o16 is not None:
        _note("mean_pool_fwd bf16", ref64.assert_within_ulps(o16.cpu(), ref, 1, 0.0, f"pool fwd bf16 B{B} S{S} D{D}"))


@pytest.mark.parametrize("from_bf16", [False, True])
@pytest.mark.parametrize("B,S,D", POOL + [(3, 2048, 1024)])
def test_mean_pool_bwd(B, S, D, from_bf16):
    """dx = dout / S broadcast over S; (3, 2048, 1024) has B * S * D / 8 > 2048 * 256 and strides over the grid"""
    dout = _randn((B, D), 710)
    dout = dout.to(BF16) if from_bf16 else dout
    dx = hip.mean_pool_bwd(dout.to(DEV), S).cpu()
    ref = (dout.to(F64) / S)[:, None, :].expand(B, S, D)
    _note("mean_pool_bwd", ref64.assert_within_ulps(dx, ref, 1, 2.0 ** -18 * ref64.rowmax(ref), f"pool bwd B{B} S{S} D{D}"))


# =============================================================================================================================
# user-sequence assembly
@pytest.mark.parametrize("p,batch0", [(0.0, 0), (0.1, 0), (0.1, 2)])
@pytest.mark.parametrize("L,Qi,H", [(50, 32, 768), (100, 32, 768), (3, 1, 8), (7, 4, 264)])
def test_user_sequence_assemble(L, Qi, H, p, batch0):
    """values against the float64 PE: 1 bf16 ulp + pos * 2^-19 (__expf's argument rounding ~2^-20.8 relative in the frequency, the
    product's ~2^-21, x 2 margin, times the angle <= pos); padding rows exactly zero, mask exactly 0 / 1; with dropout the kept elements
    are ref / (1 - p), the dropped ones exactly 0, at the counters of ur_dropout_keep"""
    B, seed = 5, 77
    tok = _randn((B, L, Qi, H), 800).to(BF16)
    ctx = _randn((B, L, H), 801).to(BF16)
    lens = torch.tensor([0, 1, L, int(torch.randint(1, L + 1, (1,), generator=_gen(802))), L + 3], dtype=torch.int32)      # (longer than L: all valid)
    out, mask = hip.user_sequence_assemble(tok.to(DEV), ctx.to(DEV), lens.to(DEV), p, seed, drop_batch0=batch0)
    keep = None
    if p > 0:
        n = B * L * Qi * H
        keep = hip.dropout_keep(seed, p, batch0 * L * Qi * H, n, DEV).cpu().reshape(B, L * Qi, H)
        assert 0.85 < float(keep.float().mean()) < 0.95
    ref, rmask = ref64.user_sequence_assemble(tok, ctx, lens, keep=keep, p=p)
    assert torch.equal(mask.cpu().to(F64), rmask), "mask must be exactly 0 / 1 by length"
    out = out.cpu()
    pos_floor = (torch.arange(L * Qi, dtype=F64) * 2.0 ** -19 / (1.0 - p))[None, :, None]
    _note("user_sequence_assemble", ref64.assert_within_ulps(out, ref, 1, pos_floor.expand_as(ref) * (ref != 0), f"assemble L{L} Qi{Qi} H{H} p{p}"))
    zero = ref == 0                                               # padding rows and dropped elements: exactly zero, not merely small
    assert (_bits(out)[zero] & 0x7FFF == 0).all()
    assert (out[0] == 0).all() and (out[1, Qi:] == 0).all()


# =============================================================================================================================
# cosine scores / catalogue scores
def _with_zero_rows(x, rows):
    for r in rows:
        if r < x.shape[0]:
            x[r] = 0
    return x


@pytest.mark.parametrize("B,N,D", [(1, 0, 4), (16, 1, 48), (17, 3, 1024), (37, 4, 1028), (16, 5, 2048), (37, 5003, 48), (2, 100003, 4),
                                   (1, 100003, 48), (17, 257, 2048)])
def test_cosine_scores(B, N, D):
    user = _with_zero_rows(_randn((B, D), 900), [B - 1] if B > 1 else [])
    pos = _randn((B, D), 901)
    neg = _randn((B, N, D), 902)
    if N > 2:
        neg[0, 1] = 0                                             # a zero candidate: score 0, finite
    s, inv = hip.cosine_scores(user.to(DEV), pos.to(DEV), neg.to(DEV))
    ref, ref32 = ref64.cosine_scores(user, pos, neg), ref64.cosine_scores(user, pos, neg, dtype=F32)
    _note("cosine_scores", ref64.assert_f32_close(s.cpu(), ref, ref32, what=f"cosine B{B} N{N} D{D}"))
    if B > 1:
        assert (s.cpu()[B - 1] == 0).all()
    if N > 2:
        assert float(s.cpu()[0, 2]) == 0.0
    cand = torch.cat([pos[:, None], neg], 1)
    iref = 1.0 / cand.to(F64).norm(dim=-1).clamp_min(1e-12)
    iref32 = 1.0 / cand.norm(dim=-1).clamp_min(1e-12)
    _note("cosine_scores inv_norm", ref64.assert_f32_close(inv.cpu()[..., None], iref[..., None], iref32[..., None], what="cand_inv_norm"))


@pytest.mark.parametrize("B,N,D", [(1, 1, 4), (16, 3, 48), (17, 4, 1024), (37, 5, 1028), (17, 5003, 2048), (3, 100003, 48), (16, 100003, 4),
                                   (37, 1001, 1024)])
def test_catalog_scores(B, N, D):
    """the last partial block of 16 users (B = 17, 37), rows per block rounded to 4 (N = 1, 3, 5, 5003, 100003)"""
    user = _with_zero_rows(_randn((B, D), 910), [B - 1] if B > 1 else [])
    cat = _with_zero_rows(_randn((N, D), 911), [2])
    s, cinv = hip.catalog_scores(user.to(DEV), cat.to(DEV))
    ref, ref32 = ref64.catalog_scores(user, cat), ref64.catalog_scores(user, cat, dtype=F32)
    _note("catalog_scores", ref64.assert_f32_close(s.cpu(), ref, ref32, what=f"catalog B{B} N{N} D{D}"))
    if B > 1:
        assert (s.cpu()[B - 1] == 0).all()
    if N > 2:
        assert (s.cpu()[:, 2] == 0).all()
    s2, cinv2 = hip.catalog_scores(user.to(DEV), cat.to(DEV), cat_inv_norm=cinv)
    assert cinv2 is cinv and torch.equal(s2.view(torch.int32), s.view(torch.int32)), "the cat_inv_norm reuse path changed the scores"


def test_catalog_scores_rejects_wide_rows():
    user, cat = torch.zeros((2, 2052), device=DEV), torch.zeros((3, 2052), device=DEV)
    _rejected(lambda: hip.catalog_scores(user, cat), "ur_catalog_scores")


# =============================================================================================================================
# InfoNCE
TAU = float(torch.tensor(0.07, dtype=F32))


@pytest.mark.parametrize("B,N,D,mask_mode,tau,gscale", [
    (1, 0, 4, "none", 0.07, 1.0), (2, 1, 4, "random", 0.07, 1.0), (64, 14, 1024, "none", 0.07, 0.25), (65, 15, 1028, "random", 0.07, 1.0),
    (130, 16, 4, "one", 1.0, 1.0), (2, 255, 2048, "none", 0.01, 3.0), (2, 256, 1028, "random", 0.07, 1.0), (1, 257, 1024, "all_invalid", 0.07, 1.0),
    (65, 1000, 1028, "random", 0.07, 1.0), (2, 10000, 1024, "none", 0.07, 1.0), (2, 10000, 4, "random", 0.01, 1.0), (130, 257, 2048, "one", 0.07, 2.0),
    (64, 16, 1024, "all_invalid", 0.01, 1.0), (2, 15, 2048, "none", 1.0, 1.0)])
def test_infonce_fwd_bwd(B, N, D, mask_mode, tau, gscale):
    """loss and d_user against torch.autograd through the float64 head (one dropped candidate of 10001 moves the loss by ~1e-4);
    N + 1 < 16 leaves backward chunks empty, D > 1024 strides the feature axis, B > 64 strides the 64-lane batch mean"""
    tau = float(torch.tensor(tau, dtype=F32))                     # the value the kernel receives
    user, pos, neg = _randn((B, D), 1000), _randn((B, D), 1001), _randn((B, N, D), 1002)
    g = _gen(1003)
    mask = {"none": None, "random": torch.rand((B, N), generator=g) > 0.3, "all_invalid": torch.zeros((B, N), dtype=torch.bool),
            "one": torch.zeros((B, N), dtype=torch.bool)}[mask_mode]
    if mask_mode == "one":
        mask[torch.arange(B), torch.randint(0, N, (B,), generator=g)] = True
    u, p_, n_ = user.to(DEV), pos.to(DEV), neg.to(DEV)
    m_ = None if mask is None else mask.to(torch.uint8).to(DEV)
    s, inv = hip.cosine_scores(u, p_, n_)
    loss, du = hip.infonce_fwd_bwd(u, p_, n_, m_, s, inv, temperature=tau, grad_scale=gscale)
    loss_ng, du_ng = hip.infonce_fwd_bwd(u, p_, n_, m_, s, inv, temperature=tau, grad_scale=gscale, need_grad=False)
    assert du_ng is None and torch.equal(loss_ng.view(torch.int32), loss.view(torch.int32)), "need_grad=False changed the loss"
    l64, du64 = ref64.infonce(user, pos, neg, mask, tau, gscale)
    l32, du32 = ref64.infonce(user, pos, neg, mask, tau, gscale, dtype=F32)
    what = f"infonce B{B} N{N} D{D} {mask_mode} tau{tau:g}"
    _note("infonce loss", ref64.assert_f32_close(loss.cpu().reshape(()), l64, l32, scale=abs(float(l64)) + 1.0, what=what + " loss"))
    # rows without a valid negative: the exact gradient is 0 and so is e32, which would allow nothing.  The kernel forms z_0 - lse with a
    # fused multiply-subtract whose residue is up to half an f32 ulp of z = s / tau (|z| <= 1 / tau): |p_0 - 1| <= 2^-24 / tau, the
    # weight (p_0 - 1) / tau, the direction |c^_0 - u^ s_0| <= 1, the chain rule 1 / ||u||, the mean 1 / B; x 4 for exp / log roundings
    dead = torch.ones(B, dtype=torch.bool) if N == 0 else (torch.zeros(B, dtype=torch.bool) if mask is None else ~mask.any(1))
    if (~dead).any():
        _note("infonce d_user", ref64.assert_f32_close(du.cpu()[~dead], du64[~dead], du32[~dead], what=what + " d_user"))
    if dead.any():
        bound = 2.0 ** -22 * gscale / (B * user.double().norm(dim=-1)[dead] * tau * tau)
        err = du.cpu().double()[dead].abs().amax(-1)
        assert torch.isfinite(err).all() and (err <= bound).all(), f"{what}: d_user of a sample without valid negatives: {float((err / bound).max()):.3f} x the bound"
        assert float(du64[dead].abs().max()) < 1e-12
        _note("infonce d_user (no valid negative)", float((err / bound).max()))
    print(f"[e32] {what}: loss e32 {abs(float(l32) - float(l64)):.3e}, d_user max e32 / rowmax "
          f"{float(((du32.to(F64) - du64).abs().amax(-1) / du64.abs().amax(-1).clamp_min(1e-300)).max()):.3e}")
    if mask_mode == "all_invalid" or N == 0:
        assert abs(float(l64)) < 1e-12


# =============================================================================================================================
# ranks and top-K: exact
def _rank_scores(B, C, seed):
    """rows of small integers (ties everywhere), then special rows: all equal; equal maxima at j and j + 256 (the thread stride) and in
    different waves (j, j + 64, j + 200); +inf; -inf runs; all -inf"""
    g = _gen(seed)
    s = torch.randint(-4, 5, (B, C), generator=g).float()
    s[1 % B] = 2.0
    if C > 256:
        s[2 % B, 0] = s[2 % B, 256] = 9.0
    if C > 200:
        s[3 % B, 10] = s[3 % B, 74] = s[3 % B, 210] = 7.0
    if B > 4:
        s[4, C // 2] = float("inf")
        s[4, : C // 3] = float("-inf")
    if B > 5:
        s[5] = float("-inf")
    if B > 6:
        s[6] = s[6] + torch.rand(C, generator=g)                  # a row without ties
    return s


@pytest.mark.parametrize("C", [1, 2, 256, 257, 1001, 100003])
def test_ranks_and_topk_are_exact(C):
    B = 8
    s = _rank_scores(B, C, 1100 + C)
    sd = s.to(DEV)
    for K in sorted({1, min(10, C), C if C <= 1001 else 10}):
        idx, val = hip.topk(sd, K)
        ridx, rval = ref64.topk(s, K)
        assert torch.equal(idx.cpu().to(torch.int64), ridx), f"top-{K} of C = {C}: rows {(idx.cpu() != ridx).any(1).nonzero().flatten().tolist()} differ"
        assert torch.equal(val.cpu().view(torch.int32), s.gather(1, ridx).view(torch.int32)), "val_out != scores.gather(idx_out)"
    assert torch.equal(hip.topk(sd, min(4, C))[0].cpu()[1 % B].to(torch.int64), torch.arange(min(4, C)))       # all equal: 0 .. K-1
    # MRR rank over [positive | negatives]: ties go to the positive, a masked negative above the positive is not counted
    N = C - 1
    g = _gen(1200 + C)
    for mask in (None, torch.rand((B, N), generator=g) > 0.5):
        s2 = s.clone()
        if N >= 3:
            s2[0, 0], s2[0, 1], s2[0, 2], s2[0, 3] = 1.0, 5.0, 5.0, 1.0      # two negatives above, one tie
            if mask is not None:
                mask[0, 0], mask[0, 1] = False, True                          # the first is masked away
        m_ = None if mask is None else mask.to(torch.uint8).to(DEV)
        r = hip.mrr_rank(s2.to(DEV), m_).cpu().to(torch.int64)
        assert torch.equal(r, ref64.mrr_rank(s2, mask)), f"mrr_rank C = {C}"
        assert int(r[1 % B]) == 1 or B == 1                                   # all equal: rank 1
    # rank of a catalogue column
    gt = torch.randint(0, C, (B,), generator=g)
    if C > 256:
        gt[2] = 256                                                           # one of the equal maxima: rank 1
    r = hip.rank_of_index(sd, gt).cpu().to(torch.int64)
    assert torch.equal(r, ref64.rank_of_index(s, gt))
    if C > 256:
        assert int(r[2]) == 1


# =============================================================================================================================
# reconstruction statistics / gradient, triplet margin, MSE
def _scalar_close(got, r64, r32, what):
    """a vector of independent scalars: each its own row with scale |ref| + 1"""
    got, r64, r32 = got.reshape(-1, 1), r64.reshape(-1, 1), r32.reshape(-1, 1)
    return ref64.assert_f32_close(got, r64, r32, scale=r64.abs().reshape(-1) + 1.0, what=what)


@pytest.mark.parametrize("E", [1, 100, 1024])
@pytest.mark.parametrize("rows", [1, 3, 5, 1024, 1025, 4100])
def test_recon_stats_and_grad(rows, E):
    """rows > 1024 takes the grid stride (256 workgroups x 4 waves); a zero rec row takes the cosine eps path"""
    rec, x = _randn((rows, E), 1300), _randn((rows, E), 1301)
    rec[0] = 0
    g = _gen(1302 + rows)
    mode = (rows + E) % 3
    mask = [torch.ones(rows), (torch.rand(rows, generator=g) > 0.4).float(), torch.zeros(rows)][mode]
    mask[0] = 1.0                                                 # the zero rec row counts (mode 2: it is the single valid row)
    sums = hip.recon_stats(rec.to(DEV), x.to(DEV), mask.to(DEV))
    r64, r32 = ref64.recon_stats(rec, x, mask), ref64.recon_stats(rec, x, mask, dtype=F32)
    _note("recon_stats", _scalar_close(sums.cpu(), r64, r32, f"recon_stats rows{rows} E{E}"))
    assert float(sums[1]) == float(mask.sum())
    d = hip.recon_grad(rec.to(DEV), x.to(DEV), mask.to(DEV), sums, 0.7).cpu()
    _note("recon_grad", ref64.assert_f32_close(d, ref64.recon_grad(rec, x, mask, 0.7), ref64.recon_grad(rec, x, mask, 0.7, dtype=F32),
                                               what=f"recon_grad rows{rows} E{E}"))
    assert (d[mask == 0] == 0).all()


@pytest.mark.parametrize("E", [1, 100, 1024])
@pytest.mark.parametrize("B", [1, 5, 4097])
def test_triplet_margin(B, E):
    """B > 4096 takes the grid stride; rows whose margin is inactive get an exactly zero gradient; anchor == positive; coef != 1"""
    a, p, n = _randn((B, E), 1400), _randn((B, E), 1401), _randn((B, E), 1402)
    if B > 1:
        a[1] = p[1]
    margin, coef = 0.5, 1.5
    l_rows = ((a.double() - p.double() + 1e-6) ** 2).sum(-1).sqrt() - ((a.double() - n.double() + 1e-6) ** 2).sum(-1).sqrt() + margin
    near = l_rows.abs() < 1e-4                                    # f32 and f64 may disagree about which side of the hinge such a row is on
    a[near] = p[near]                                             # (anchor == positive: firmly active)
    l_rows = ((a.double() - p.double() + 1e-6) ** 2).sum(-1).sqrt() - ((a.double() - n.double() + 1e-6) ** 2).sum(-1).sqrt() + margin
    assert (l_rows.abs() >= 1e-4).all()
    loss, da = hip.triplet_margin(a.to(DEV), p.to(DEV), n.to(DEV), margin, coef)
    l64, d64 = ref64.triplet_margin(a, p, n, margin, coef)
    l32, d32 = ref64.triplet_margin(a, p, n, margin, coef, dtype=F32)
    what = f"triplet B{B} E{E}"
    _note("triplet_margin loss", ref64.assert_f32_close(loss.cpu().reshape(()), l64, l32, scale=abs(float(l64)) + 1.0, what=what + " loss"))
    _note("triplet_margin d_anchor", ref64.assert_f32_close(da.cpu(), d64, d32, what=what + " d_anchor"))
    inactive = d64.abs().amax(-1) == 0
    assert (da.cpu()[inactive] == 0).all()
    if B > 1000:
        assert inactive.any() and not inactive.all()
    loss_ng, da_ng = hip.triplet_margin(a.to(DEV), p.to(DEV), n.to(DEV), margin, coef, need_grad=False)
    assert da_ng is None and torch.equal(loss_ng.view(torch.int32), loss.view(torch.int32))


@pytest.mark.parametrize("n", [1, 7, 65536, 65536 * 256 + 3])
def test_mse_loss(n):
    """n > 65536 strides the 256-workgroup sum; the gradient strides above 2048 * 256 elements"""
    a, b = _randn((n,), 1500), _randn((n,), 1501)
    loss, da = hip.mse_loss(a.to(DEV), b.to(DEV), coef=0.3)
    l64, d64 = ref64.mse(a, b, 0.3)
    l32, d32 = ref64.mse(a, b, 0.3, dtype=F32)
    _note("mse_loss loss", ref64.assert_f32_close(loss.cpu().reshape(()), l64, l32, scale=abs(float(l64)) + 1.0, what=f"mse n{n} loss"))
    _note("mse_loss d_a", ref64.assert_f32_close(da.cpu()[:, None], d64[:, None], d32[:, None], what=f"mse n{n} d_a"))
    loss_ng, da_ng = hip.mse_loss(a.to(DEV), b.to(DEV), coef=0.3, need_grad=False)
    assert da_ng is None and torch.equal(loss_ng.view(torch.int32), loss.view(torch.int32))


# =============================================================================================================================
# GELU' and SwiGLU: exhaustive over bfloat16
def _all_finite_bf16():
    bits = torch.arange(0, 65536, dtype=torch.int32)
    bits = bits[(bits & 0x7F80) != 0x7F80]                        # drop inf / NaN: 65 280 values, zeros and subnormals included
    assert bits.numel() == 65280
    return bits.to(torch.int16).view(BF16)


def _check_may_overflow(got, ref, ulps, floor, what):
    """assert_within_ulps, except where the float64 reference leaves bfloat16's range: there the output must be the infinity of the right
    sign (either that or the largest finite value inside the last half ulp, where the rounding goes either way)"""
    got, ref = got.to(F64), ref.to(F64)
    over = ref.abs() > ref64.BF16_MAX
    sure = ref.abs() > ref64.BF16_MAX + 2.0 ** 120               # beyond the largest finite value + 1 ulp: certainly rounds to infinity
    assert (got[sure] == torch.sign(ref[sure]) * float("inf")).all(), f"{what}: overflow must give the signed infinity"
    edge = over & ~sure
    assert ((got[edge].abs() >= ref64.BF16_MAX) & (torch.sign(got[edge]) == torch.sign(ref[edge]))).all(), f"{what}: wrong value at the edge of the range"
    fl = torch.as_tensor(floor, dtype=F64).expand_as(ref)
    return ref64.assert_within_ulps(torch.where(over, torch.zeros_like(got), got), torch.where(over, torch.zeros_like(ref), ref), ulps,
                                    torch.where(over, torch.zeros_like(fl), fl), what)


@pytest.mark.parametrize("random_dy", [False, True])
def test_gelu_bwd_exhaustive(random_dy):
    """every finite bf16 u: dx = dy * (Phi(u) + u phi(u)) within 1 ulp + 2^-18 |dy| -- the hardware exp2 behind the fitted Phi runs HERE
    (tests/test_gelu_cdf.py pins the coefficients by CPU emulation only)"""
    u = _all_finite_bf16()
    dy = _randn((u.numel(),), 1600, 2.0).to(BF16) if random_dy else torch.ones(u.numel(), dtype=BF16)
    dx = hip.gelu_bwd(dy.to(DEV), u.to(DEV)).cpu()
    ref = dy.to(F64) * ref64.gelu_grad(u)
    _note("gelu_bwd", ref64.assert_within_ulps(dx, ref, 1, 2.0 ** -18 * dy.to(F64).abs(), "gelu_bwd over all bf16"))


UPS = [0.0, 2.0 ** -100, -(2.0 ** -100), 1.0, -2.5, 0.0078125 * 3, 3.0e4, -3.0e4]       # 0, +-tiny, +-large
DACTS = [1.0, -0.5, 2.0 ** -9 * 3, 100.0]


def test_swiglu_exhaustive():
    """every finite bf16 gate x 8 up values (x 4 dact values for the backward): 1 ulp, no floor for the forward and for d_up, 2^-18 |dact * up|
    for d_gate (silu' = s (1 + g (1 - s)) cancels around g = -1.28)"""
    gate = _all_finite_bf16()
    I = gate.numel()
    ups = torch.tensor(UPS).to(BF16)
    gu = torch.cat([gate[None, :].expand(len(UPS), I), ups[:, None].expand(len(UPS), I)], dim=1).contiguous()       # [8, 2 I]
    act = hip.swiglu_fwd(gu.to(DEV), I).cpu()
    ref = ref64.swiglu_fwd(gu[:, :I], gu[:, I:])
    _note("swiglu_fwd", _check_may_overflow(act, ref, 1, 0.0, "swiglu_fwd over all bf16 gates"))
    gu4 = gu.repeat(len(DACTS), 1)                                                         # [32, 2 I]: row = dact index * 8 + up index
    dact = torch.tensor(DACTS).to(BF16).repeat_interleave(len(UPS))[:, None].expand(len(DACTS) * len(UPS), I).contiguous()
    dgu = hip.swiglu_bwd(dact.to(DEV), gu4.to(DEV), I).cpu()
    rg, ru = ref64.swiglu_bwd(dact, gu4[:, :I], gu4[:, I:])
    scale = (dact.to(F64) * gu4[:, I:].to(F64)).abs()
    _note("swiglu_bwd d_gate", _check_may_overflow(dgu[:, :I], rg, 1, 2.0 ** -18 * scale, "swiglu_bwd d_gate over all bf16 gates"))
    _note("swiglu_bwd d_up", _check_may_overflow(dgu[:, I:], ru, 1, 0.0, "swiglu_bwd d_up over all bf16 gates"))


@pytest.mark.parametrize("M,I", [(1, 8), (33, 96), (4133, 3072)])
def test_swiglu_shapes(M, I):
    gu = _randn((M, 2 * I), 1700, 2.0).to(BF16)
    dact = _randn((M, I), 1701).to(BF16)
    act = hip.swiglu_fwd(gu.to(DEV), I).cpu()
    _note("swiglu_fwd", ref64.assert_within_ulps(act, ref64.swiglu_fwd(gu[:, :I], gu[:, I:]), 1, 0.0, f"swiglu_fwd {M}x{I}"))
    dgu = hip.swiglu_bwd(dact.to(DEV), gu.to(DEV), I).cpu()
    rg, ru = ref64.swiglu_bwd(dact, gu[:, :I], gu[:, I:])
    _note("swiglu_bwd d_gate", ref64.assert_within_ulps(dgu[:, :I], rg, 1, 2.0 ** -18 * (dact.to(F64) * gu[:, I:].to(F64)).abs(), f"swiglu_bwd d_gate {M}x{I}"))
    _note("swiglu_bwd d_up", ref64.assert_within_ulps(dgu[:, I:], ru, 1, 0.0, f"swiglu_bwd d_up {M}x{I}"))


# =============================================================================================================================
# event-context encoders, first layer
def _timestamps(n, seed):
    day, year = 86400.0, 31557600.0
    head = torch.tensor([0.0, -1.0, -day, -3.0 * day - 5.0, -year - 17.0, day * 19000, day * 7 * 2800, year * 50, year, 1.7e9, 1.7e9 + 12345.0, 1.0, 43200.0])
    g = _gen(seed)
    rest = torch.cat([1.7e9 + torch.rand(max(n, 16), generator=g) * 1.0e8, -torch.rand(16, generator=g) * 1.0e9, torch.rand(16, generator=g) * 1.0e5])
    return torch.cat([head, rest[torch.randperm(rest.numel(), generator=g)]])[:n].float().contiguous()


def _coords(n, seed):
    head = torch.tensor([[90.0, 0.0], [-90.0, 0.0], [90.0, 180.0], [-90.0, -180.0], [0.0, 180.0], [0.0, -180.0], [0.0, 0.0], [45.0, 90.0], [12.5, -179.999]])
    g = _gen(seed)
    rest = torch.stack([torch.rand(max(n, 16), generator=g) * 180.0 - 90.0, torch.rand(max(n, 16), generator=g) * 360.0 - 180.0], -1)
    return torch.cat([head, rest])[:n].float().contiguous()


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n,H2", [(1, 8), (1, 100), (1, 1536), (70000, 8), (70000, 100), (3000, 1536)])
def test_context_mlp1(n, H2, kind):
    """float64 Linear + GELU over the features computed by the float32 recipe in the reference's operation order (they are f32-chaotic at
    real timestamps).  1 bf16 ulp + sum_f |W1[j][f]| * 2 * f32_ulp(angle_f): an angle may round one f32 ulp differently, sin / cos are
    1-Lipschitz.  n = 70000 is more workgroups than a 16-bit grid index holds."""
    nf = 9 if kind == 0 else 3
    x = _timestamps(n, 1800) if kind == 0 else _coords(n, 1801)
    feat, ang = ref64.timestamp_features(x) if kind == 0 else ref64.geo_features(x)
    W1, b1 = _randn((H2, nf), 1802, 0.5), _randn((H2,), 1803, 0.5)
    out = hip.context_mlp1(x.to(DEV), kind, W1.to(DEV), b1.to(DEV)).cpu()
    ref = ref64.context_mlp1(feat, W1, b1)
    floor = (2.0 * ref64.f32_ulp(ang)) @ W1.to(F64).abs().t()
    _note(f"context_mlp1 kind {kind}", ref64.assert_within_ulps(out, ref, 1, floor, f"context_mlp1 kind{kind} n{n} H2 {H2}"))


# =============================================================================================================================
# argument checks: a negative code and a message, nothing launched
def test_argument_checks_reject_without_launching():
    lib = _lib.load()
    st = hip._stream()
    f = lambda *shape: torch.zeros(shape, device=DEV)                         # noqa: E731
    h = lambda *shape: torch.zeros(shape, dtype=BF16, device=DEV)             # noqa: E731
    ids = torch.zeros((2, 4), dtype=torch.int64, device=DEV)
    # D % 8 / % 4
    _rejected(lambda: hip.mean_pool_fwd(h(2, 4, 12)), "ur_mean_pool_fwd")
    _rejected(lambda: hip.mean_pool_bwd(f(2, 12), 4), "ur_mean_pool_bwd")
    _rejected(lambda: hip.embed_inject_fwd(h(8, 12), ids, None, 4), "ur_embed_inject_fwd")
    _rejected(lambda: hip.inject_bwd(h(2, 4, 12), ids, 4, 2), "ur_inject_bwd")
    _rejected(lambda: hip.user_sequence_assemble(h(1, 2, 2, 12), h(1, 2, 12), torch.ones(1, dtype=torch.int32, device=DEV)), "ur_user_sequence_assemble")
    _rejected(lambda: hip.cosine_scores(f(2, 6), f(2, 6), f(2, 3, 6)), "ur_cosine_scores")
    _rejected(lambda: hip.catalog_scores(f(2, 6), f(3, 6)), "ur_catalog_scores")
    _rejected(lambda: hip.gelu_bwd(h(12), h(12)), "ur_gelu_bwd")
    _rejected(lambda: hip.swiglu_fwd(h(2, 24), 12), "ur_swiglu_fwd")
    _rejected(lambda: hip.swiglu_bwd(h(2, 12), h(2, 24), 12), "ur_swiglu_bwd")
    _rejected(lambda: hip.qknorm_rope_fwd(h(4, 4 * 32), f(32), f(32), f(4, 16), f(4, 16), 4, 2, 1, 32, 1e-6), "ur_qknorm_rope_fwd")
    # top-K with K > C
    _rejected(lambda: hip.topk(f(2, 5), 6), "ur_topk")
    # a workspace one byte short
    B, N, D = 3, 5, 8
    user, pos, neg = f(B, D) + 1, f(B, D) + 1, f(B, N, D) + 1
    s, inv = hip.cosine_scores(user, pos, neg)
    loss = torch.full((1,), 123.0, device=DEV)
    wsb = int(lib.ur_infonce_workspace_bytes(B, N, D))
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    rc = lib.ur_infonce_fwd_bwd(user.data_ptr(), pos.data_ptr(), neg.data_ptr(), 0, s.data_ptr(), inv.data_ptr(), 0.07, 1.0, loss.data_ptr(), 0, B, N, D,
                                ws.data_ptr(), wsb - 1, st)
    assert rc < 0 and b"ur_infonce_fwd_bwd" in lib.ur_last_error() and float(loss) == 123.0
    assert lib.ur_infonce_fwd_bwd(user.data_ptr(), pos.data_ptr(), neg.data_ptr(), 0, s.data_ptr(), inv.data_ptr(), 0.07, 1.0, loss.data_ptr(), 0, B, N, D,
                                  ws.data_ptr(), wsb, st) == 0 and float(loss) != 123.0
    x = h(2, 4, 16) + 1
    o32 = torch.full((2, 16), 123.0, device=DEV)
    wsb = int(lib.ur_mean_pool_workspace_bytes(2, 16))
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    rc = lib.ur_mean_pool_fwd(x.data_ptr(), o32.data_ptr(), 0, 2, 4, 16, ws.data_ptr(), wsb - 1, st)
    assert rc < 0 and b"ur_mean_pool_fwd" in lib.ur_last_error() and (o32 == 123.0).all()
    assert lib.ur_mean_pool_fwd(x.data_ptr(), o32.data_ptr(), 0, 2, 4, 16, ws.data_ptr(), wsb, st) == 0 and (o32 == 1.0).all()
    # an operand 2 bytes off a 16-byte boundary
    flat = h(4096)
    off = flat[1:1 + 64]                                                       # data_ptr + 2
    assert off.data_ptr() % 16 == 2
    _rejected(lambda: hip.gelu_bwd(h(64), off), "ur_gelu_bwd")
    _rejected(lambda: hip.swiglu_fwd(off.view(2, 32), 16), "ur_swiglu_fwd")
    _rejected(lambda: hip.swiglu_bwd(off[:32].view(2, 16), h(2, 32), 16), "ur_swiglu_bwd")
    _rejected(lambda: hip.mean_pool_fwd(off.view(1, 4, 16)), "ur_mean_pool_fwd")
    _rejected(lambda: hip.embed_inject_fwd(flat[1:1 + 8 * 16].view(8, 16), ids, None, 4), "ur_embed_inject_fwd")
    _rejected(lambda: hip.inject_bwd(flat[1:1 + 2 * 4 * 16].view(2, 4, 16), ids, 4, 2), "ur_inject_bwd")
    raw_off = flat[1:1 + 4 * 256].view(4, 256)
    tab = f(4, 32)
    _rejected(lambda: hip.qknorm_rope_fwd(raw_off, f(64), f(64), tab, tab, 4, 2, 1, 64, 1e-6), "ur_qknorm_rope_fwd")
    fflat = f(4096)
    foff = fflat[1:1 + 64]                                                     # f32: + 4 bytes, still off the 16-byte boundary
    _rejected(lambda: hip.cosine_scores(foff.view(2, 32), f(2, 32), f(2, 3, 32)), "ur_cosine_scores")
    _rejected(lambda: hip.catalog_scores(foff.view(2, 32), f(3, 32)), "ur_catalog_scores")
    torch.cuda.synchronize()


def test_zz_worst_ratio_table():
    """prints the worst observed error / bound per kernel over the tests of this module that ran before it (docs/lab_notes.md)"""
    print("\n[table] worst error / bound per kernel")
    for k in sorted(WORST):
        print(f"[table] {k:45s} {WORST[k]:.4f}")
    assert all(math.isfinite(v) for v in WORST.values())

"""GPU: LayerNorm, RMSNorm (also fused with the LoRA down projection), the batch reductions and the epilogues of ur_gemm, ELEMENT BY
ELEMENT against the float64 references of tests/ref64.py (checked on the CPU in tests/test_ref64.py), at the shapes where each kernel
branches: every NCH instantiation, a partly filled last 512-column chunk, H = 8, one row, and more rows than the grid-stride caps of
csrc/norm.hip (16384 / 2048 / 32768 rows for ln_fwd / ln_bwd / rms_*).

Criteria (tests/ref64.py; docs/lab_notes.md, "Element-wise float64 tests: norm, reduction and GEMM epilogue kernels"):
  bf16 outputs of the norm kernels   |got - ref| <= 1 bf16 ulp + 2^-18 * row max |ref| + 8 * e32_row        (assert_bf16_rows; the row
                                     maximum of a dropout-masked output is that of the unmasked row / (1 - p))
  mean, rstd (f32)                   per row 8 * e32 + 2^-20 * scale                                         (assert_f32_close)
  dgamma, dbeta, dbias, reductions   per column 8 * e32_col + 2^-20 * sum_m |term|; integer inputs exact     (assert_colsum_close)
  z_save                             bit-equal to bf16(y + residual); 1 ulp + 8 * e32_row under pre-dropout; a dropped element = the residual's bits
  GEMM epilogue, exact products      C: 1 ulp + 2^-20 (|alpha acc| + |bias| + |res|)                       (assert_gemm_c)
                                     gelu_out against gelu of the C bits written: 1 ulp where |gelu| > 1e-6, 1e-6 absolute below
                                                                                                             (assert_gelu_close)
                                     gelu' mode: 1 ulp + 2^-18 |alpha acc + bias + res|, the value the factor multiplies, as
                                     test_gelu_bwd_exhaustive's 2^-18 |dy|                                   (assert_gemm_gelu_grad)
                                     f32: 2^-22 (|alpha acc| + |bias|)                                       (assert_gemm_f32)
e32 = |the same formula in float32 torch on the CPU - the float64 value|.  Keep flags come from oracle/dropout_ref.hidden_keep (numpy).
No element is exempt.  Every test prints its worst error / bound ("[ratio] kernel: x"); test_zz_worst_ratio_table prints the table.

The reference normalises the z the kernel SAVED, after that z has been held to its own criterion: LN(z) of the rounded z is the
documented function (forward and backward see the same z), and under pre-dropout the f32 product y * 1 / (1 - p) may legitimately round
z one ulp away from the float64 value.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dropout_ref  # noqa: E402
from tests import norm_cases, ref64  # noqa: E402
from unirec_amd import _lib, hip  # noqa: E402

# entry point -> the primitive-level tests of this module that hold it against a reference (tests/test_abi_test_coverage.py)
COVERS = {
    "ur_layernorm_fwd": ["test_layernorm", "test_layernorm_modes", "test_layernorm_fwd_grid_stride", "test_norm_argument_checks_and_empty_launches"],
    "ur_layernorm_bwd": ["test_layernorm", "test_layernorm_modes", "test_layernorm_bwd_grid_stride", "test_norm_argument_checks_and_empty_launches"],
    "ur_layernorm_bwd_reduce": ["test_layernorm", "test_layernorm_modes", "test_layernorm_bwd_grid_stride"],
    "ur_rmsnorm_fwd": ["test_rmsnorm", "test_rmsnorm_grid_stride"],
    "ur_rmsnorm_bwd": ["test_rmsnorm", "test_rmsnorm_grid_stride"],
    "ur_rmsnorm_lora_fwd": ["test_fused_rmsnorm_lora_norm_half"],
    "ur_batch_reduce": ["test_batch_reduce", "test_batch_reduce_wide_rows_many_batches_exact"],
    "ur_gemm": ["test_gemm_epilogues_exact_products", "test_gemm_gelu_epilogues_over_every_finite_bf16"],
}

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENTINEL = 0x4B4B                    # a finite bf16 bit pattern nothing computes by accident
LN_EPS, RMS_EPS = 1e-12, 1e-6
WORST = {}


def _note(kernel, ratio):
    WORST[kernel] = max(WORST.get(kernel, 0.0), float(ratio))
    print(f"[ratio] {kernel}: {float(ratio):.4f}")


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=norm_cases.gen(seed)) * scale


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _rejected(fn, who):
    """fn() must fail with a NEGATIVE return code (argument check, nothing launched) and a message naming the entry point"""
    with pytest.raises(_lib.UniRecHipError) as e:
        fn()
    msg = str(e.value)
    assert "rc=-" in msg and who in msg.split("):", 1)[-1], msg


def _keep(M, H, p, seed, row0):
    """[M, H] float64 0 / 1 from the numpy generator, or None"""
    if not p:
        return None
    return torch.from_numpy(dropout_ref.hidden_keep(seed, p, M, H, row0).astype(np.float64))


def _col(t):
    return t.reshape(-1, 1)


# =============================================================================================================================
# LayerNorm
LN_H = [8, 512, 520, 768, 1024, 1032, 1544, 2048]
SEED_PRE, SEED_POST = 0x1234_5678_9ABC, 77


def _ln_inputs(M, H, y_rows, with_res, seed):
    y = norm_cases.rows(y_rows, H, seed)
    res = norm_cases.residual_rows(M, H, seed + 1) if with_res else None
    gamma, beta = norm_cases.norm_weight(H, seed + 2), _randn((H,), seed + 3)
    dout = _randn((M, H), seed + 4).to(BF16)
    return y, res, gamma, beta, dout


def _ln_forward_checks(tag, y, res, gamma, beta, M, H, y_rows, p_pre, p_post, row0):
    """launches the forward, holds z / out / mean / rstd, returns what the backward needs"""
    kpre, kpost = _keep(M, H, p_pre, SEED_PRE, row0), _keep(M, H, p_post, SEED_POST, row0)
    yd, rd, gd, bd = y.to(DEV), (res.to(DEV) if res is not None else None), gamma.to(DEV), beta.to(DEV)
    kw = dict(residual=rd, p_pre=p_pre, seed_pre=SEED_PRE, p_post=p_post, seed_post=SEED_POST, M=M, drop_row0=row0)
    out, z, mean, rstd = hip.layernorm_fwd(yd, gd, bd, LN_EPS, save_z=True, **kw)
    out_nz, z_none, mean_nz, rstd_nz = hip.layernorm_fwd(yd, gd, bd, LN_EPS, save_z=False, **kw)
    assert z_none is None and _same_bits(out, out_nz), f"{tag}: save_z=False changes the output bits"
    assert torch.equal(mean.view(torch.int32), mean_nz.view(torch.int32)) and torch.equal(rstd.view(torch.int32), rstd_nz.view(torch.int32))
    zc = z.cpu()
    # z_save
    if not p_pre:
        z32 = ref64.layernorm_fwd(y, res, gamma, beta, LN_EPS, y_rows=y_rows, M=M, dtype=F32)[0].to(BF16)
        assert _same_bits(zc, z32), f"{tag}: z_save is not bf16(y + residual)"
    else:
        # 1 ulp + 8 * e32_row: y / (1 - p) + residual can cancel EXACTLY (40.5 / 0.9 - 45) where the f32 product is 2^-24 of its terms off
        z_exact, z_f32 = ref64.layernorm_z(y, res, kpre, p_pre, y_rows, M), ref64.layernorm_z(y, res, kpre, p_pre, y_rows, M, dtype=F32)
        _note("layernorm_fwd z_save (pre-dropout)", ref64.assert_bf16_rows(zc, z_exact, z_f32, f"{tag} z_save", floor=0.0))
        dropped = kpre == 0
        want = res if res is not None else torch.zeros(M, H, dtype=BF16)
        assert torch.equal(zc.to(F64)[dropped], want.to(F64)[dropped]), f"{tag}: a dropped element's z is not the residual"
        if res is not None:
            assert torch.equal(_bits(zc)[dropped], _bits(want)[dropped]), f"{tag}: a dropped element's z is not the residual bit for bit"
    # out, mean, rstd of the z the kernel saved
    r64 = ref64.layernorm_of_z(zc.to(F64), gamma, beta, LN_EPS, kpost, p_post)
    r32 = ref64.layernorm_of_z(zc.to(F64), gamma, beta, LN_EPS, kpost, p_post, dtype=F32)
    unmasked = ref64.rowmax(ref64.layernorm_of_z(zc.to(F64), gamma, beta, LN_EPS)[0]) / (1.0 - p_post) if p_post else None
    _note("layernorm_fwd out", ref64.assert_bf16_rows(out.cpu(), r64[0], r32[0], f"{tag} out", scale=unmasked))
    _note("layernorm_fwd mean", ref64.assert_f32_close(_col(mean.cpu()), _col(r64[1]), _col(r32[1]), scale=zc.to(F64).abs().amax(-1), what=f"{tag} mean"))
    _note("layernorm_fwd rstd", ref64.assert_f32_close(_col(rstd.cpu()), _col(r64[2]), _col(r32[2]), what=f"{tag} rstd"))
    return out, z, mean, rstd, kpre, kpost, gd


def _ln_backward_checks(tag, dout, z, mean, rstd, gamma, gd, M, H, p_pre, p_post, row0, kpre, kpost, need_dy=True):
    """one-call path and defer_reduce + finish(): dz, dy, dgamma, dbeta, dbias"""
    zc = z.cpu()
    dd = dout.to(DEV)
    kw = dict(p_pre=p_pre, seed_pre=SEED_PRE, p_post=p_post, seed_post=SEED_POST, need_dy=need_dy, drop_row0=row0)
    nan = lambda: torch.full((H,), float("nan"), device=DEV)          # noqa: E731
    dg, db, dbias = nan(), nan(), (nan() if need_dy else None)
    dz, dy = hip.layernorm_bwd(dd, z, mean, rstd, gd, dg, db, dbias, **kw)
    dg2, db2, dbias2 = nan(), nan(), (nan() if need_dy else None)
    dz2, dy2, finish = hip.layernorm_bwd(dd, z, mean, rstd, gd, dg2, db2, dbias2, defer_reduce=True, **kw)
    torch.cuda.synchronize()
    assert torch.isnan(dg2).all() and torch.isnan(db2).all(), f"{tag}: the deferred path wrote a parameter gradient before finish()"
    finish()
    assert _same_bits(dz, dz2) and _same_bits(dy, dy2), f"{tag}: the deferred path changes dz / dy bits"
    if not p_pre or not need_dy:
        assert dy.data_ptr() == dz.data_ptr()
    r64 = ref64.layernorm_bwd(dout, zc, gamma, LN_EPS, kpre, p_pre, kpost, p_post)
    r32 = ref64.layernorm_bwd(dout, zc, gamma, LN_EPS, kpre, p_pre, kpost, p_post, dtype=F32)
    _note("layernorm_bwd dz", ref64.assert_bf16_rows(dz.cpu(), r64[0], r32[0], f"{tag} dz"))
    if need_dy:
        unmasked = ref64.rowmax(r64[0]) / (1.0 - p_pre) if p_pre else None          # dy = dz with elements masked away: the row scale is dz's
        _note("layernorm_bwd dy", ref64.assert_bf16_rows(dy.cpu(), r64[1], r32[1], f"{tag} dy", scale=unmasked))
    tg, tb = ref64.layernorm_bwd_terms(dout, zc, LN_EPS, kpost, p_post)
    for path, g_, b_, s_ in (("one call", dg, db, dbias), ("deferred", dg2, db2, dbias2)):
        _note("layernorm_bwd dgamma", ref64.assert_colsum_close(g_.cpu(), r64[2], r32[2], tg, f"{tag} dgamma ({path})"))
        _note("layernorm_bwd dbeta", ref64.assert_colsum_close(b_.cpu(), r64[3], r32[3], tb, f"{tag} dbeta ({path})"))
        if s_ is not None:
            own = dy.cpu().to(F64)
            _note("layernorm_bwd dbias", ref64.assert_colsum_close(s_.cpu(), own.sum(0), own.sum(0), own.abs().sum(0), f"{tag} dbias ({path})"))


def _ln_case(M, H, *, with_res=True, y_rows=None, p_pre=0.0, p_post=0.0, row0=0, need_dy=True, backward=True, seed=100):
    y_rows = M if y_rows is None else y_rows
    tag = f"layernorm M{M} H{H} y_rows{y_rows} res{int(with_res)} p_pre{p_pre} p_post{p_post} row0 {row0}"
    y, res, gamma, beta, dout = _ln_inputs(M, H, y_rows, with_res, seed + H)
    out, z, mean, rstd, kpre, kpost, gd = _ln_forward_checks(tag, y, res, gamma, beta, M, H, y_rows, p_pre, p_post, row0)
    e = norm_cases.equal_row(M)
    if e >= 0 and y_rows == M and not p_pre and not p_post:
        # variance 0, eps carries it: the output IS beta
        assert torch.equal(out[e].cpu(), beta.to(BF16)), f"{tag}: the all-equal row does not come out as beta"
        assert float(mean[e]) == norm_cases.EQUAL_VALUE + (1.0 if with_res else 0.0) and abs(float(rstd[e]) * math.sqrt(LN_EPS) - 1.0) < 2.0 ** -20
    if backward:
        _ln_backward_checks(tag, dout, z, mean, rstd, gamma, gd, M, H, p_pre, p_post, row0, kpre, kpost, need_dy)


@pytest.mark.parametrize("M", [1, 5, 257])
@pytest.mark.parametrize("H", LN_H)
def test_layernorm(M, H):
    """forward, backward and the deferred reduction with a residual, every NCH instantiation (H <= 512, <= 1024, above), a partly
    filled last chunk (520, 1032, 1544), H = 8, and one / five / 257 rows (64 blocks of four rows and one of one)"""
    _ln_case(M, H)


@pytest.mark.parametrize("H", [8, 1032])
def test_layernorm_bwd_grid_stride(H):
    """2048 + 5 rows: the first row count at which ln_bwd_kernel's row loop strides, and all 512 partial rows of the column sums in use
    (what ur_layernorm_bwd_reduce walks)"""
    _ln_case(2048 + 5, H, seed=200)


def _sentinel_bf16(M, H):
    return torch.full((M, H), SENTINEL, dtype=torch.int16, device=DEV).view(BF16)


def _periodic(t, M):
    return t[torch.arange(M) % t.shape[0]].contiguous()


@pytest.mark.parametrize("H", [8, 1032])
def test_layernorm_fwd_grid_stride(H):
    """16384 + 7 rows: ln_fwd_kernel's row loop strides from 16384 rows on.  The inputs repeat with period 521 rows (a prime: a row and
    its repeats fall on different waves and blocks); the reference is evaluated once per distinct row.  Rows that come out bit-identical
    to their first occurrence are held through it; any other row is held against the reference on its own.  The outputs are filled with a
    sentinel (NaN for mean / rstd) before the launch, so a row the kernel never wrote is one of those."""
    M, P = 16384 + 7, 521
    y, res, gamma, beta, _ = _ln_inputs(P, H, P, True, 300 + H)
    yd, rd = _periodic(y, M).to(DEV), _periodic(res, M).to(DEV)
    out, z = _sentinel_bf16(M, H), _sentinel_bf16(M, H)                      # an unwritten row keeps the sentinel and is held on its own below
    mean, rstd = torch.full((M,), float("nan"), device=DEV), torch.full((M,), float("nan"), device=DEV)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    _lib.check(_lib.load().ur_layernorm_fwd(yd.data_ptr(), M, rd.data_ptr(), gd.data_ptr(), bd.data_ptr(), out.data_ptr(), z.data_ptr(), mean.data_ptr(),
                                            rstd.data_ptr(), M, H, LN_EPS, 0.0, 0, 0.0, 0, 0, hip._stream()), "ur_layernorm_fwd")
    tag = f"layernorm_fwd M{M} H{H}"
    z32 = ref64.layernorm_fwd(y, res, gamma, beta, LN_EPS, dtype=F32)[0].to(BF16)
    assert _same_bits(z.cpu(), _periodic(z32, M)), f"{tag}: z_save is not bf16(y + residual)"
    r64 = ref64.layernorm_of_z(z32.to(F64), gamma, beta, LN_EPS)
    r32 = ref64.layernorm_of_z(z32.to(F64), gamma, beta, LN_EPS, dtype=F32)
    oc, mc, rc = out.cpu(), mean.cpu(), rstd.cpu()
    assert torch.isfinite(mc).all() and torch.isfinite(rc).all(), f"{tag}: rows of mean / rstd were never written"
    same = (_bits(oc) == _bits(_periodic(oc[:P], M))).all(-1) & (mc == _periodic(mc[:P], M)) & (rc == _periodic(rc[:P], M))
    rows = torch.cat([torch.arange(P), (~same).nonzero().flatten()]).unique()
    print(f"[info] {tag}: {int((~same).sum())} rows differ from their first occurrence")
    src = rows % P
    _note("layernorm_fwd out", ref64.assert_bf16_rows(oc[rows], r64[0][src], r32[0][src], f"{tag} out"))
    _note("layernorm_fwd mean", ref64.assert_f32_close(_col(mc[rows]), _col(r64[1][src]), _col(r32[1][src]), scale=z32.to(F64).abs().amax(-1)[src], what=f"{tag} mean"))
    _note("layernorm_fwd rstd", ref64.assert_f32_close(_col(rc[rows]), _col(r64[2][src]), _col(r32[2][src]), what=f"{tag} rstd"))


LN_MODES = [
    dict(with_res=False),                                                         # plain
    dict(with_res=False, y_rows=32),                                              # broadcast, 256 % 32 == 0 (M is set to 256 below)
    dict(with_res=True, y_rows=7),                                                # broadcast, M % y_rows != 0
    dict(with_res=True, p_pre=0.1, row0=0),
    dict(with_res=True, p_pre=0.5, row0=40),
    dict(with_res=False, p_pre=0.5, row0=40),
    dict(with_res=True, p_post=0.1, row0=40),
    dict(with_res=False, p_post=0.5, row0=0),
    dict(with_res=True, p_pre=0.1, p_post=0.5, row0=40),
    dict(with_res=True, p_pre=0.5, p_post=0.1, row0=0, y_rows=7),
    dict(with_res=True, need_dy=False),
    dict(with_res=True, p_pre=0.1, row0=40, need_dy=False),
]


@pytest.mark.parametrize("mode", range(len(LN_MODES)))
@pytest.mark.parametrize("H", [8, 520, 1544])
def test_layernorm_modes(H, mode):
    kw = dict(LN_MODES[mode])
    M = 256 if kw.get("y_rows") == 32 else 257
    _ln_case(M, H, seed=400 + mode, **kw)


def test_norm_argument_checks_and_empty_launches():
    """rejections carry a negative code and launch nothing; M = 0 returns 0 and writes no row"""
    lib = _lib.load()
    st = hip._stream()
    f = lambda *shape: torch.zeros(shape, device=DEV)                         # noqa: E731
    h = lambda *shape: torch.zeros(shape, dtype=BF16, device=DEV)             # noqa: E731
    for H in (12, 2056):
        _rejected(lambda: hip.layernorm_fwd(h(2, H), f(H), f(H), LN_EPS), "ur_layernorm_fwd")
        _rejected(lambda: hip.layernorm_bwd(h(2, H), h(2, H), f(2), f(2), f(H), f(H), f(H)), "ur_layernorm_bwd")
        _rejected(lambda: hip.rmsnorm_fwd(h(2, H), f(H), RMS_EPS), "ur_rmsnorm_fwd")
        _rejected(lambda: hip.rmsnorm_bwd(h(2, H), h(2, H), f(H), f(2)), "ur_rmsnorm_bwd")
    H = 16
    _rejected(lambda: hip.layernorm_fwd(h(2, H), f(H), f(H), LN_EPS, p_pre=1.0), "ur_layernorm_fwd")
    _rejected(lambda: hip.layernorm_fwd(h(2, H), f(H), f(H), LN_EPS, p_post=1.0), "ur_layernorm_fwd")
    _rejected(lambda: hip.layernorm_bwd(h(2, H), h(2, H), f(2), f(2), f(H), f(H), f(H), p_pre=1.0), "ur_layernorm_bwd")
    _rejected(lambda: hip.batch_reduce(h(3, 12), 3, 1, 12), "ur_batch_reduce")
    # a workspace one byte short; dy aliasing dz under pre-dropout (the header allows the alias for p_pre == 0 only)
    M = 4
    sent = lambda: torch.full((M, H), SENTINEL, dtype=torch.int16, device=DEV).view(BF16)        # noqa: E731
    dout, z, mean, rstd, gamma = h(M, H) + 1, h(M, H), f(M), f(M) + 1, f(H) + 1
    dz, dy, dg, db = sent(), sent(), torch.full((H,), 123.0, device=DEV), torch.full((H,), 123.0, device=DEV)
    wsb = int(lib.ur_layernorm_bwd_workspace_bytes(H))
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    bwd = lambda dz_, dy_, M_, p_pre, nbytes: lib.ur_layernorm_bwd(dout.data_ptr(), z.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),   # noqa: E731
                                                                   dz_.data_ptr(), dy_.data_ptr(), dg.data_ptr(), db.data_ptr(), 0, M_, H, p_pre, 1, 0.0, 2, 0,
                                                                   ws.data_ptr(), nbytes, st)
    assert bwd(dz, dy, M, 0.0, wsb - 1) < 0 and b"ur_layernorm_bwd" in lib.ur_last_error()
    assert bwd(dz, dz, M, 0.5, wsb) < 0 and b"ur_layernorm_bwd" in lib.ur_last_error()
    torch.cuda.synchronize()
    assert (_bits(dz) == SENTINEL).all() and (_bits(dy) == SENTINEL).all() and (dg == 123.0).all() and (db == 123.0).all()
    # M = 0
    assert bwd(dz, dy, 0, 0.0, wsb) == 0
    out, zs, mu, rs = sent(), sent(), f(M) + 123.0, f(M) + 123.0
    assert lib.ur_layernorm_fwd(dout.data_ptr(), 1, 0, gamma.data_ptr(), gamma.data_ptr(), out.data_ptr(), zs.data_ptr(), mu.data_ptr(), rs.data_ptr(),
                                0, H, LN_EPS, 0.0, 0, 0.0, 0, 0, st) == 0
    assert lib.ur_rmsnorm_fwd(dout.data_ptr(), gamma.data_ptr(), out.data_ptr(), rs.data_ptr(), 0, H, RMS_EPS, st) == 0
    assert lib.ur_rmsnorm_bwd(dout.data_ptr(), dout.data_ptr(), gamma.data_ptr(), rstd.data_ptr(), 0, zs.data_ptr(), 0, H, st) == 0
    torch.cuda.synchronize()
    for t in (dz, dy, out, zs):
        assert (_bits(t) == SENTINEL).all()
    assert (mu == 123.0).all() and (rs == 123.0).all()
    assert (dg == 0).all() and (db == 0).all()         # ur_layernorm_bwd with M = 0 (header): dgamma / dbeta become the empty sum, no row is written
    assert bwd(dz, dy, M, 0.0, wsb) == 0                                       # the same arguments are accepted once nothing is wrong
    torch.cuda.synchronize()
    assert not (_bits(dz) == SENTINEL).any()


# =============================================================================================================================
# RMSNorm
RMS_D = [8, 128, 520, 1024, 1032, 1544, 2048]


def _rms_inputs(M, D, seed):
    x = norm_cases.rows(M, D, seed)
    e = norm_cases.equal_row(M)
    if e >= 0:
        x[e] = 0.0                                                             # the zero row
    w = norm_cases.norm_weight(D, seed + 1)
    dout, add = _randn((M, D), seed + 2).to(BF16), _randn((M, D), seed + 3).to(BF16)
    return x, w, dout, add


def _rms_refs(x, w, dout, add):
    f = [ref64.rmsnorm_fwd(x, w, RMS_EPS, dtype=dt) for dt in (F64, F32)]
    b_add = [ref64.rmsnorm_bwd(dout, x, w, RMS_EPS, add, dtype=dt) for dt in (F64, F32)]
    b = [ref64.rmsnorm_bwd(dout, x, w, RMS_EPS, None, dtype=dt) for dt in (F64, F32)]
    return f, b_add, b


@pytest.mark.parametrize("M", [1, 7, 513])
@pytest.mark.parametrize("D", RMS_D)
def test_rmsnorm(M, D):
    """forward and backward, with and without `add`, every NCH instantiation (D > 1024 runs NCH = 4), partly filled last chunks,
    D = 8.  The zero row: rstd = eps^-1/2, out = 0, and -- xhat being 0 -- dx = add + rstd * dout * w."""
    tag = f"rmsnorm M{M} D{D}"
    x, w, dout, add = _rms_inputs(M, D, 500 + D)
    f, b_add, b = _rms_refs(x, w, dout, add)
    xd, wd, dd = x.to(DEV), w.to(DEV), dout.to(DEV)
    out, rstd = hip.rmsnorm_fwd(xd, wd, RMS_EPS)
    _note("rmsnorm_fwd out", ref64.assert_bf16_rows(out.cpu(), f[0][0], f[1][0], f"{tag} out"))
    _note("rmsnorm_fwd rstd", ref64.assert_f32_close(_col(rstd.cpu()), _col(f[0][1]), _col(f[1][1]), what=f"{tag} rstd"))
    e = norm_cases.equal_row(M)
    if e >= 0:
        assert (out[e] == 0).all() and abs(float(rstd[e]) * math.sqrt(RMS_EPS) - 1.0) < 2.0 ** -20
    dx_add = hip.rmsnorm_bwd(dd, xd, wd, rstd, add=add.to(DEV))
    dx = hip.rmsnorm_bwd(dd, xd, wd, rstd)
    _note("rmsnorm_bwd dx (add)", ref64.assert_bf16_rows(dx_add.cpu(), b_add[0], b_add[1], f"{tag} dx with add"))
    _note("rmsnorm_bwd dx", ref64.assert_bf16_rows(dx.cpu(), b[0], b[1], f"{tag} dx"))


@pytest.mark.parametrize("D", [8, 1032])
def test_rmsnorm_grid_stride(D):
    """32768 + 7 rows: rms_fwd_kernel / rms_bwd_kernel stride from 32768 rows on.  Periodic inputs as in test_layernorm_fwd_grid_stride."""
    M, P = 32768 + 7, 521
    tag = f"rmsnorm M{M} D{D}"
    x, w, dout, add = _rms_inputs(P, D, 600 + D)
    f, b_add, _ = _rms_refs(x, w, dout, add)
    xd, wd = _periodic(x, M).to(DEV), w.to(DEV)
    out, dx, rstd = _sentinel_bf16(M, D), _sentinel_bf16(M, D), torch.full((M,), float("nan"), device=DEV)     # as in the LayerNorm stride test
    dd, ad = _periodic(dout, M).to(DEV), _periodic(add, M).to(DEV)
    lib, st = _lib.load(), hip._stream()
    _lib.check(lib.ur_rmsnorm_fwd(xd.data_ptr(), wd.data_ptr(), out.data_ptr(), rstd.data_ptr(), M, D, RMS_EPS, st), "ur_rmsnorm_fwd")
    _lib.check(lib.ur_rmsnorm_bwd(dd.data_ptr(), xd.data_ptr(), wd.data_ptr(), rstd.data_ptr(), ad.data_ptr(), dx.data_ptr(), M, D, st), "ur_rmsnorm_bwd")
    oc, rc, dc = out.cpu(), rstd.cpu(), dx.cpu()
    assert torch.isfinite(rc).all(), f"{tag}: {int((~torch.isfinite(rc)).sum())} rows of rstd were never written"
    same = (_bits(oc) == _bits(_periodic(oc[:P], M))).all(-1) & (rc == _periodic(rc[:P], M)) & (_bits(dc) == _bits(_periodic(dc[:P], M))).all(-1)
    rows = torch.cat([torch.arange(P), (~same).nonzero().flatten()]).unique()
    print(f"[info] {tag}: {int((~same).sum())} rows differ from their first occurrence")
    src = rows % P
    _note("rmsnorm_fwd out", ref64.assert_bf16_rows(oc[rows], f[0][0][src], f[1][0][src], f"{tag} out"))
    _note("rmsnorm_fwd rstd", ref64.assert_f32_close(_col(rc[rows]), _col(f[0][1][src]), _col(f[1][1][src]), what=f"{tag} rstd"))
    _note("rmsnorm_bwd dx (add)", ref64.assert_bf16_rows(dc[rows], b_add[0][src], b_add[1][src], f"{tag} dx with add"))


@pytest.mark.parametrize("nad,p", [(2, 0.0), (3, 0.0), (2, 0.1), (3, 0.1)])
@pytest.mark.parametrize("M", [1, 64, 1000, 4133])
def test_fused_rmsnorm_lora_norm_half(M, nad, p):
    """h and rstd of ur_rmsnorm_lora_fwd against the float64 RMSNorm (the projection t keeps its test in tests/test_gpu_primitives.py)"""
    D = 1024
    tag = f"rmsnorm_lora_fwd M{M} nad{nad} p{p}"
    x, w, _, _ = _rms_inputs(M, D, 700 + M)
    U = [_randn((16, D), 710 + a, 0.05).to(BF16).to(DEV) for a in range(nad)]
    bits = hip.lora_dropout_bits(1234, p, M, D, nad, DEV) if p > 0 else None
    h, rstd, _ = hip.rmsnorm_lora_fwd(x.to(DEV), w.to(DEV), RMS_EPS, U, alpha=2.0 / (1.0 - p), bits=bits)
    r64, r32 = ref64.rmsnorm_fwd(x, w, RMS_EPS), ref64.rmsnorm_fwd(x, w, RMS_EPS, dtype=F32)
    _note("rmsnorm_lora_fwd h", ref64.assert_bf16_rows(h.cpu(), r64[0], r32[0], f"{tag} h"))
    _note("rmsnorm_lora_fwd rstd", ref64.assert_f32_close(_col(rstd.cpu()), _col(r64[1]), _col(r32[1]), what=f"{tag} rstd"))


# =============================================================================================================================
# batch reduce / column sums
BR_NB = [0, 1, 3, 37, 63, 64, 65, 1000, 2053, 4099]
BR_ROWS_H = [(1, 8), (1, 136), (4, 64), (32, 1024)]


def _br_run(x, nb, rows, H):
    xd = x.to(DEV) if nb > 0 else torch.zeros((rows, H), dtype=BF16, device=DEV)           # nb == 0 still needs a valid pointer
    out = torch.full((rows, H), float("nan"), device=DEV)
    if rows == 1 and nb > 0:
        return hip.colsum(xd.view(nb, H), out=out.view(H)).view(1, H).cpu()
    return hip.batch_reduce(xd, nb, rows, H, out=out).cpu()


# (32 x 1024 at nb = 2053 and 4099 -- 67 M and 134 M elements -- is held by test_batch_reduce_wide_rows_many_batches_exact)
BR_CASES = [(nb, rows, H) for rows, H in BR_ROWS_H for nb in BR_NB if not (rows * H == 32 * 1024 and nb > 1000)]


@pytest.mark.parametrize("nb,rows,H", BR_CASES)
def test_batch_reduce(nb, rows, H):
    """every slice shape of batch_reduce_stage1: one row per slice (nb <= 64), the unrolled loop with each remainder (nb = 2053 at
    rows * H <= 256: 33 rows per slice = 8 trips of four + 1; 1000 and 4099 likewise), short and empty last slices; rows = 1 goes
    through hip.colsum.  Random inputs within 2^-20 * sum_b |in| per element, integer-valued inputs exact."""
    tag = f"batch_reduce nb{nb} rows{rows} H{H}"
    scale = torch.exp2(torch.randint(-6, 7, (rows * H,), generator=norm_cases.gen(800))).reshape(1, H * rows)
    x = (_randn((nb, rows * H), 801 + nb) * scale).to(BF16).reshape(nb * rows, H)
    r = ref64.batch_reduce(x, nb, rows, H)
    a = ref64.batch_reduce(x.to(F64).abs(), nb, rows, H)
    _note("batch_reduce", ref64.assert_colsum_close(_br_run(x, nb, rows, H), r, r, a, tag))
    xi = torch.randint(-3, 4, (nb * rows, H), generator=norm_cases.gen(802 + nb)).to(BF16)
    assert torch.equal(_br_run(xi, nb, rows, H).to(F64), ref64.batch_reduce(xi, nb, rows, H)), f"{tag}: integer-valued inputs must sum exactly"


@pytest.mark.parametrize("nb", [2053, 4099])
def test_batch_reduce_wide_rows_many_batches_exact(nb):
    """rows * H = 32 x 1024 at the two largest batch counts (64 slices of 33 resp. 65 rows, the last ones short): integer-valued
    inputs, which must come out exact (a float64 reference of 134 M random elements would take longer than the rest of the module)"""
    rows, H = 32, 1024
    xi = torch.randint(-3, 4, (nb, rows * H), generator=norm_cases.gen(810 + nb), dtype=torch.int8)
    want = xi.sum(0, dtype=torch.int64).reshape(rows, H)
    out = hip.batch_reduce(xi.to(DEV).to(BF16).reshape(nb * rows, H), nb, rows, H).cpu()
    assert torch.equal(out.to(torch.int64), want) and torch.equal(out, want.float())
    _note("batch_reduce", 0.0)


# =============================================================================================================================
# GEMM epilogues on exact products
LAYOUTS = [(True, True), (True, False), (False, False), (False, True)]


def _big_tile_shape(rk, sk):
    """the smallest (M, N) every layout accepts for which the library takes the generic kernel's 256 x 256 configuration (hip.gemm_plan holds
    it: one tile column less is the 128 tile): 2 x 128 tiles, 2 x 112 when both operands are K-strided -- with M, N multiples of 8
    (K-strided operands) and not of 256, which also keeps the launch off the persistent kernel"""
    wgs = 224 if (not rk and not sk) else 256
    M, N, K = 264, (wgs // 2 - 1) * 256 + 8, 72
    pl = hip.gemm_plan(M, N, K, r_kcontig=rk, s_kcontig=sk)
    assert (pl["kernel"], pl["tile"]) == ("generic", 256) and hip.gemm_plan(M, N - 256, K, r_kcontig=rk, s_kcontig=sk)["tile"] == 128
    return M, N, K


PERS_SHAPE = (2048, 4096, 256)      # 128 tiles of 256 x 256, K a multiple of 64 from 256 on, K-contiguous operands: the persistent kernel (gemm_pers.hip)
GEMM_SHAPES = [(8, 8, 8), (200, 136, 72), (200, 132, 72), (130, 260, 200), "big"]
GEMM_CASES = [(s, rk, sk) for s in GEMM_SHAPES for rk, sk in LAYOUTS
              if s == "big" or ((rk or s[0] % 8 == 0) and (sk or s[1] % 8 == 0))]          # a K-strided operand needs its contiguous dim % 8 == 0
GEMM_CASES.append((PERS_SHAPE, True, True))
_GEMM_INPUTS = {}


def _gemm_inputs(M, N, K):
    key = (M, N, K)
    if key not in _GEMM_INPUTS:
        _GEMM_INPUTS.clear()                                                   # one shape at a time: the big one is 8.6 M elements per tensor
        g = norm_cases.gen(900 + M + N)
        Rm = torch.randint(-3, 4, (M, K), generator=g).float()
        Sm = torch.randint(-3, 4, (N, K), generator=g).float()
        acc = (Rm @ Sm.t()).to(F64)                                            # |acc| <= 9 K < 2^24: exact in float32
        bias = torch.randn(N, generator=g)
        res = torch.randn(M, N, generator=g).to(BF16)
        aux = (torch.randn(M, N, generator=g) * 1.5).to(BF16)
        _GEMM_INPUTS[key] = (Rm, Sm, acc, bias, res, aux)
    return _GEMM_INPUTS[key]


@pytest.mark.parametrize("shape,rk,sk", GEMM_CASES)
def test_gemm_epilogues_exact_products(shape, rk, sk):
    """integer-valued R, S in [-3, 3], K <= 256: the accumulator is exact, only the epilogue rounds.  v = (alpha acc + bias + res) *
    gelu'(aux); C = bf16(v); gelu_out = bf16(gelu(C)).  The shapes of the issue run on the generic kernel (gemm_body.hip.h); PERS_SHAPE is
    the smallest launch the persistent kernel takes, whose GELU epilogues (residual-free: EPI 6 / 7) are code of their own."""
    M, N, K = _big_tile_shape(rk, sk) if shape == "big" else shape
    if shape == PERS_SHAPE:
        takes = lambda **kw: hip.gemm_plan(M, N, K, **kw)      # noqa: E731
        assert takes(bias=True)["kernel"] == "persistent" and not hip.gemm_plan(M - 256, N, K, bias=True)["kernel"] == "persistent"
        assert (takes(bias=True, gelu_out=True)["epi"], takes(bias=True, gelu_grad_aux=True)["epi"]) == (6, 7)
    tag = f"gemm {M}x{N}x{K} rk{int(rk)} sk{int(sk)}"
    Rm, Sm, acc, bias, res, aux = _gemm_inputs(M, N, K)
    R = (Rm if rk else Rm.t()).contiguous().to(BF16).to(DEV)
    S = (Sm if sk else Sm.t()).contiguous().to(BF16).to(DEV)
    bd, rd, ad = bias.to(DEV), res.to(DEV), aux.to(DEV)
    run = lambda **kw: hip.gemm(R, S, r_kcontig=rk, s_kcontig=sk, **kw)        # noqa: E731
    def check_c(C, alpha, b_, r_, what):
        _note("gemm epilogue C", ref64.assert_gemm_c(C.cpu(), acc, alpha, b_, r_, f"{tag} {what}"))

    def check_gelu(C, g, what):
        _note("gemm epilogue gelu_out", ref64.assert_gelu_close(g.cpu(), C.cpu(), f"{tag} {what}: gelu_out against gelu of the C written"))

    def check_grad(C, alpha, b_, r_, what):
        _note("gemm epilogue gelu' mode", ref64.assert_gemm_gelu_grad(C.cpu(), acc, alpha, b_, r_, aux, f"{tag} {what}, * gelu'(aux)"))

    g = torch.empty((M, N), dtype=BF16, device=DEV)
    C = run(alpha=0.5, bias=bd, residual=rd, gelu_out=g)
    check_c(C, 0.5, bias, res, "alpha 0.5 + bias + residual + gelu_out")
    check_gelu(C, g, "alpha 0.5 + bias + residual")
    for alpha in (1.0, 0.5):
        check_grad(run(alpha=alpha, bias=bd, gelu_grad_aux=ad), alpha, bias, None, f"alpha {alpha} + bias")
    _note("gemm epilogue f32", ref64.assert_gemm_f32(run(alpha=0.5, bias=bd, out_f32=True).cpu(), acc, 0.5, bias, f"{tag} f32 + bias"))
    check_c(run(alpha=0.5, bias=bd), 0.5, bias, None, "alpha 0.5 + bias")           # the plain path (a bias alone)
    C = run(alpha=1.0, bias=bd, gelu_out=g)
    check_c(C, 1.0, bias, None, "alpha 1 + bias + gelu_out")
    check_gelu(C, g, "alpha 1 + bias")
    check_c(run(alpha=1.0, residual=rd), 1.0, None, res, "alpha 1 + residual")
    check_grad(run(alpha=1.0, bias=bd, residual=rd, gelu_grad_aux=ad), 1.0, bias, res, "alpha 1 + bias + residual")
    assert torch.equal(run(out_f32=True).cpu().to(F64), acc), f"{tag}: the plain f32 product is not exact"


def _all_finite_bf16():
    bits = torch.arange(0, 65536, dtype=torch.int32)
    bits = bits[(bits & 0x7F80) != 0x7F80]                        # drop inf / NaN: 65 280 values, zeros and subnormals included
    assert bits.numel() == 65280
    return bits.to(torch.int16).view(BF16)


BF16_MIN_SUBNORMAL = 2.0 ** -133


def test_gemm_gelu_epilogues_over_every_finite_bf16():
    """K = 8, S[n, 0] = x_n for every finite bf16, R[m, 0] = +-1: acc = +-x_n exactly, so gelu_out = bf16(gelu(+-x_n)) runs the fitted Phi
    and the hardware exp2 over every input -- the forward exists only as this epilogue (tests/test_gelu_cdf.py emulates it on the CPU).
    1 bf16 ulp where |gelu(x)| > 1e-6 (there test_gelu_cdf.py demands the exact bf16 of the emulation), |err| <= 1e-6 below (either zero
    included where the float64 value lies below the smallest bf16 subnormal).  The same launch shape with gelu_grad_aux = x and acc = dy_m repeats
    test_gelu_bwd_exhaustive for the epilogue path."""
    x = _all_finite_bf16()
    N, M, K = x.numel(), 8, 8
    S = torch.zeros(N, K, dtype=BF16)
    S[:, 0] = x
    sign = torch.tensor([1.0, -1.0] * (M // 2))
    R = torch.zeros(M, K, dtype=BF16)
    R[:, 0] = sign.to(BF16)
    g = torch.empty((M, N), dtype=BF16, device=DEV)
    C = hip.gemm(R.to(DEV), S.to(DEV), gelu_out=g)
    arg = sign.to(F64)[:, None] * x.to(F64)[None, :]
    assert torch.equal(C.cpu().to(F64), arg), "C is not the exact product"
    got, ref = g.cpu().to(F64), ref64.gelu(arg)
    big = ref.abs() > ref64.GELU_TAIL
    _note("gemm epilogue gelu_out (all bf16)", ref64.assert_gelu_close(g.cpu(), C.cpu(), "gelu_out over all bf16"))
    # x so negative that the float64 value lies below the smallest bf16 subnormal: the reference rounds to -0, either zero is right, and
    # what the linear continuation of the fit leaves there instead is held by the 1e-6 above
    under = (ref.abs() < BF16_MIN_SUBNORMAL) & (arg < -1.0)
    print(f"[info] gelu_out where gelu(x) underflows bf16: {int((got[under] == 0).sum())} of {int(under.sum())} outputs are a zero, largest |output| {float(got[under].abs().max()):.3e}")
    nearest = ref[0].to(BF16).to(F64)
    off = int(((got[0] != nearest) & big[0]).sum())
    assert off <= 225, f"{off} inputs with |gelu(x)| > 1e-6 miss the nearest bf16: more than the 225 the CPU emulation counts over ALL inputs"
    print(f"[info] gelu_out over all bf16: {off} of {int(big[0].sum())} inputs with |gelu(x)| > 1e-6 are not the nearest bf16 of the float64 value (all within 1 ulp)")
    # gelu'(x) as the epilogue: acc = dy_m exactly
    dy = torch.cat([torch.ones(1), _randn((M - 1,), 950, 2.0)]).to(BF16)
    R2 = torch.zeros(M, K, dtype=BF16)
    R2[:, 0] = dy
    S2 = torch.zeros(N, K, dtype=BF16)
    S2[:, 0] = 1.0
    aux = x[None, :].expand(M, N).contiguous()
    C2 = hip.gemm(R2.to(DEV), S2.to(DEV), gelu_grad_aux=aux.to(DEV))
    ref2 = dy.to(F64)[:, None] * ref64.gelu_grad(x)[None, :]
    _note("gemm epilogue gelu' (all bf16)", ref64.assert_within_ulps(C2.cpu(), ref2, 1, 2.0 ** -18 * dy.to(F64).abs()[:, None], "gelu' epilogue over all bf16"))


def test_zz_worst_ratio_table():
    """prints the worst observed error / bound per kernel over the tests of this module that ran before it (docs/lab_notes.md)"""
    print("\n[table] worst error / bound per kernel")
    for k in sorted(WORST):
        print(f"[table] {k:45s} {WORST[k]:.4f}")

"""GPU: the pooling family (include/unirec_hip_pool.h: ur_pool_norm_fwd / ur_pool_norm_bwd, both modes) ELEMENT BY ELEMENT against the
float64 restatement of tests/pool_ref.py (checked on the CPU in tests/test_pool_host.py), at the smallest shapes at which the kernels can
go wrong: D 8 (one 16-byte vector), 264 (33 vectors: a partly filled wave), 1024 (the product's width; two chunks per lane), 2048 (the
limit; four chunks); S 1, 7, 40, 17 (one more than the sixteen forward slices: two positions per slice, the last used slice half
filled, seven empty), 35 (2 x 16 + 3: three positions per slice, one per wave) and 200 (thirteen per slice: a wave takes a pair of rows
per trip and goes round twice); B 1 and 3; and B 5, S 1000, D 64 -- 5000 rows against the 4096 the backward's grid covers at once.

Criteria (no element is exempt; each test prints its worst error / bound as "[ratio] ..."):
  forward    |got - ref64| <= N f32 ulps of T = sum_s |c_s y_sd|, N = tests/pool_ref.fwd_ulps: the count of roundings of the kernels' own
             operation order, per sample (4 NCH + 8 for every y; the masked mean adds min(n - 1, its adds) + 1).  It is a worst-case count;
             on the samples with one valid token, where nothing averages out, the measured error reaches 0.23 of it (docs/lab_notes.md §32).
  backward   the form tests/test_gpu_norm_f64.py applies to ur_rmsnorm_bwd on the same rows (ref64.assert_bf16_rows): 1 bf16 ulp +
             2^-18 * row max |ref64| + 8 * e32_row, with ref64 = c_s * (the RMSNorm backward of g): the row scale carries c_s.
  exact      rows of +/-1 with w = 1 and eps = 0 (rstd = 1 exactly): LAST returns the selected row bit for bit, MASKED_MEAN over a
             power-of-two count the exact quotient, the backward under an integer g orthogonal to every row c * g exactly.
  masked rows filled with NaN / Inf bit patterns change no output bit, and their dx is +0 bitwise; two calls give the same bits; a NULL
  mask and an explicit all-ones mask give the same bits; every refusal returns before any launch (the outputs keep a sentinel)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import pool_ref, ref64  # noqa: E402
from unirec_amd import _lib, hip  # noqa: E402

# entry point of include/unirec_hip_pool.h -> its float64 tests (tests/test_pool_host.py holds this dict to the header)
COVERS = {
    "ur_pool_norm_workspace_bytes": ["test_forward_and_backward_against_float64"],
    "ur_pool_norm_fwd": ["test_forward_and_backward_against_float64", "test_more_rows_than_the_backward_grid_against_float64"],
    "ur_pool_norm_bwd": ["test_forward_and_backward_against_float64", "test_more_rows_than_the_backward_grid_against_float64"],
}

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPS = 1e-6
SENTINEL = 0x4B4B                    # a finite bf16 bit pattern nothing computes by accident
WORST = {}


def _note(kernel, ratio):
    WORST[kernel] = max(WORST.get(kernel, 0.0), float(ratio))
    print(f"[ratio] {kernel}: {float(ratio):.4f}")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits16(t):
    return t.contiguous().view(torch.int16)


def _bits32(t):
    return t.contiguous().view(torch.int32)


def _masks(B, S, seed):
    """name -> uint8 [B,S] or None.  Every kind the header speaks of; `empty` has one all-zero sample among valid ones (the middle one;
    the only one at B = 1)."""
    g = _gen(seed)
    pos = torch.arange(S).expand(B, S)
    npad = torch.tensor([min(S - 1, b * max(1, S // 3) + (1 if S > 1 else 0)) for b in range(B)])[:, None]
    holes = (torch.rand(B, S, generator=g) < 0.6).to(torch.uint8)
    holes[:, int(torch.randint(0, S, (1,), generator=g))] = 1
    empty = holes.clone()
    empty[B // 2] = 0
    one = lambda s: (pos == s).to(torch.uint8)      # noqa: E731
    return {"null": None, "ones": torch.ones(B, S, dtype=torch.uint8), "left": (pos >= npad).to(torch.uint8),
            "right": (pos < S - npad).to(torch.uint8), "holes": holes * 3, "first_only": one(0), "last_only": one(S - 1), "empty": empty}


def _inputs(B, S, D, seed):
    g = _gen(seed)
    x = (torch.randn(B, S, D, generator=g) * (0.5 + 2.0 * torch.rand(B, S, 1, generator=g))).to(BF16)
    w = (1.0 + 0.1 * torch.randn(D, generator=g)).to(F32)
    dp = torch.randn(B, D, generator=g).to(F32)
    return x, w, dp


def _poison(x, c):
    """x with every row of pooling weight 0 overwritten by NaN / Inf / -Inf bit patterns"""
    bad = torch.tensor([0x7FC0, 0x7F80, 0xFF80, 0x7FFF], dtype=torch.int32).to(torch.int16)
    xb = _bits16(x).clone()
    dead = (c == 0)
    fill = bad[torch.arange(x.shape[2]) % 4].expand_as(xb)
    xb = torch.where(dead[..., None], fill, xb)
    return xb.view(BF16)


def _n_valid(mask, B, S):
    return torch.full((B,), S) if mask is None else (mask != 0).sum(1)


def _check_forward(tag, x, w, mask, mode, out):
    B, S, D = x.shape
    p64, T = pool_ref.pool_norm_fwd(x, w, EPS, mask, mode)
    bound = pool_ref.fwd_bound(T, D, S, mode, _n_valid(mask, B, S))
    o = out.cpu().to(F64)
    assert torch.isfinite(o).all(), f"{tag}: non-finite output"
    err = (o - p64).abs()
    off = err > bound
    assert not off.any(), f"{tag}: {int(off.sum())} of {err.numel()} elements exceed the bound; worst error / bound {float((err / bound).max()):.3f}"
    empty = _n_valid(mask, B, S) == 0
    assert (_bits32(out.cpu())[empty] == 0).all(), f"{tag}: a sample without a valid position must give +0"
    return float((err / bound).max())


def _check_backward(tag, dp, x, w, mask, mode, dx):
    B, S, D = x.shape
    r64, r32 = (pool_ref.pool_norm_bwd(dp, x, w, EPS, mask, mode, dtype=dt) for dt in (F64, F32))
    c = pool_ref.pool_weights(mask, B, S, mode)
    dxc = dx.cpu()
    assert (_bits16(dxc)[c == 0] == 0).all(), f"{tag}: rows of pooling weight 0 must be +0 bitwise"
    return ref64.assert_bf16_rows(dxc.view(B * S, D), r64.view(B * S, D), r32.view(B * S, D), f"{tag} dx")


def _raw_fwd_exact_workspace(x, w, mask, mode):
    """ur_pool_norm_fwd through the raw library with a workspace of EXACTLY the queried size inside a larger sentinel buffer"""
    lib = _lib.load()
    B, S, D = x.shape
    m = hip.POOL_MODES[mode]
    need = int(lib.ur_pool_norm_workspace_bytes(B, D, m))
    guard = 256
    buf = torch.full((need + 2 * guard,), 0x5A, dtype=torch.uint8, device=DEV)
    out = torch.empty((B, D), dtype=F32, device=DEV)
    _lib.check(lib.ur_pool_norm_fwd(x.data_ptr(), w.data_ptr(), 0 if mask is None else mask.data_ptr(), out.data_ptr(), B, S, D, EPS, m,
                                    buf.data_ptr() + guard, need, hip._stream()), "ur_pool_norm_fwd")
    b = buf.cpu()
    assert (b[:guard] == 0x5A).all() and (b[guard + need:] == 0x5A).all(), "the forward wrote outside the workspace it asked for"
    return out


@pytest.mark.parametrize("S", [1, 7, 40, 17, 35, 200])
@pytest.mark.parametrize("D", [8, 264, 1024, 2048])
def test_forward_and_backward_against_float64(D, S):
    for B in (1, 3):
        x, w, dp = _inputs(B, S, D, 1000 * D + 10 * S + B)
        xd, wd, dd = x.to(DEV), w.to(DEV), dp.to(DEV)
        for mode in pool_ref.MODES:
            keep = {}
            for name, mask in _masks(B, S, D + S + B).items():
                tag = f"pool_norm {mode} B{B} S{S} D{D} mask={name}"
                md = None if mask is None else mask.to(DEV)
                out = hip.pool_norm_fwd(xd, wd, EPS, md, mode)
                dx = hip.pool_norm_bwd(dd, xd, wd, EPS, md, mode)
                _note(f"pool_norm_fwd {mode}", _check_forward(tag, x, w, mask, mode, out))
                _note(f"pool_norm_bwd {mode}", _check_backward(tag, dp, x, w, mask, mode, dx))
                # determinism: a second call gives the same bits
                assert torch.equal(_bits32(hip.pool_norm_fwd(xd, wd, EPS, md, mode)), _bits32(out)), f"{tag}: forward bits differ between calls"
                assert torch.equal(_bits16(hip.pool_norm_bwd(dd, xd, wd, EPS, md, mode)), _bits16(dx)), f"{tag}: backward bits differ between calls"
                # rows of pooling weight 0 are never loaded
                c = pool_ref.pool_weights(mask, B, S, mode)
                if (c == 0).any():
                    xp = _poison(x, c).to(DEV)
                    assert torch.equal(_bits32(hip.pool_norm_fwd(xp, wd, EPS, md, mode)), _bits32(out)), f"{tag}: NaN / Inf in masked rows changed the output"
                    assert torch.equal(_bits16(hip.pool_norm_bwd(dd, xp, wd, EPS, md, mode)), _bits16(dx)), f"{tag}: NaN / Inf in masked rows changed dx"
                if name == "holes":
                    assert torch.equal(_bits32(_raw_fwd_exact_workspace(xd, wd, md, mode)), _bits32(out)), f"{tag}: exact-size workspace"
                keep[name] = (out, dx)
            for k in (0, 1):
                assert torch.equal(keep["null"][k], keep["ones"][k]), f"{mode} B{B} S{S} D{D}: NULL and all-ones masks give different bits"


def test_more_rows_than_the_backward_grid_against_float64():
    """B 5, S 1000, D 64: 5000 rows, the backward's grid (1024 blocks of four waves) covers 4096 at once -- the rows beyond are reached
    by the stride; the forward runs 63 positions per slice.  Left padding, sample 3 empty."""
    B, S, D = 5, 1000, 64
    x, w, dp = _inputs(B, S, D, 77)
    pos = torch.arange(S).expand(B, S)
    mask = (pos >= torch.tensor([0, 100, 517, S, 999])[:, None]).to(torch.uint8)
    xd, wd, dd, md = x.to(DEV), w.to(DEV), dp.to(DEV), mask.to(DEV)
    for mode in pool_ref.MODES:
        for name, m, mdev in (("left", mask, md), ("null", None, None)):
            tag = f"pool_norm {mode} B{B} S{S} D{D} mask={name}"
            dx = torch.full((B, S, D), 0, dtype=torch.int16, device=DEV).fill_(SENTINEL).view(BF16)
            lib = _lib.load()
            need = int(lib.ur_pool_norm_workspace_bytes(B, D, hip.POOL_MODES[mode]))
            ws = torch.empty(need, dtype=torch.uint8, device=DEV)
            _lib.check(lib.ur_pool_norm_bwd(dd.data_ptr(), xd.data_ptr(), wd.data_ptr(), 0 if mdev is None else mdev.data_ptr(), dx.data_ptr(),
                                            B, S, D, EPS, hip.POOL_MODES[mode], ws.data_ptr(), need, hip._stream()), "ur_pool_norm_bwd")
            assert not (_bits16(dx.cpu()) == SENTINEL).all(-1).any(), f"{tag}: a row of dx was never written"
            _note(f"pool_norm_bwd {mode}", _check_backward(tag, dp, x, w, m, mode, dx))
            _note(f"pool_norm_fwd {mode}", _check_forward(tag, x, w, m, mode, hip.pool_norm_fwd(xd, wd, EPS, mdev, mode)))


@pytest.mark.parametrize("D", [8, 264, 1024])
def test_exact_cases(D):
    """rows of +/-1, w = 1, eps = 0: rstd = rsqrt(D / D + 0) = 1 exactly, y = x.  Columns come in equal pairs (x[2j] = x[2j+1]) and
    g = (k_0, -k_0, k_1, -k_1, ..) with small integers k: g is orthogonal to every row, so dx = c * g exactly."""
    B, S = 3, 40
    g = _gen(D)
    half = (torch.randint(0, 2, (B, S, D // 2), generator=g) * 2 - 1).to(F32)
    x = torch.repeat_interleave(half, 2, dim=2).to(BF16)
    k = torch.randint(-8, 9, (B, D // 2), generator=g).to(F32)
    dp = torch.stack([k, -k], dim=2).reshape(B, D)
    w = torch.ones(D)
    mask = torch.zeros(B, S, dtype=torch.uint8)
    for b, n in enumerate((8, 16, 32)):                                   # power-of-two counts at scattered positions, holes included
        mask[b, torch.randperm(S, generator=g)[:n]] = 1
    xd, wd, dd, md = x.to(DEV), w.to(DEV), dp.to(DEV), mask.to(DEV)
    last = torch.stack([x[b, int(mask[b].nonzero().max())] for b in range(B)]).to(F32)
    out = hip.pool_norm_fwd(xd, wd, 0.0, md, "last").cpu()
    assert torch.equal(_bits32(out), _bits32(last)), "LAST must return the selected row bit for bit"
    mean = torch.stack([x[b][mask[b] != 0].to(F64).sum(0) / int(mask[b].sum()) for b in range(B)])
    out = hip.pool_norm_fwd(xd, wd, 0.0, md, "masked_mean").cpu()
    assert torch.equal(out.to(F64), mean), "MASKED_MEAN over a power-of-two count must return the exact quotient"
    for mode in pool_ref.MODES:
        c = pool_ref.pool_weights(mask, B, S, mode)
        want = (c[..., None] * dp.to(F64)[:, None, :])
        assert torch.equal(want.to(BF16).to(F64), want)                   # (representable: nothing is rounded in the expectation)
        dx = hip.pool_norm_bwd(dd, xd, wd, 0.0, md, mode).cpu()
        assert torch.equal(dx.to(F64), want), f"{mode}: dx must be c * g exactly"
        assert (_bits16(dx)[c == 0] == 0).all()
    # the same without a mask: 32 rows of S = 32 (a power of two), the last row
    x32 = xd[:, :32].contiguous()
    out = hip.pool_norm_fwd(x32, wd, 0.0, None, "masked_mean").cpu()
    assert torch.equal(out.to(F64), x[:, :32].to(F64).sum(1) / 32)
    assert torch.equal(_bits32(hip.pool_norm_fwd(x32, wd, 0.0, None, "last").cpu()), _bits32(x[:, 31].to(F32)))


def test_refusals_launch_nothing():
    """every refusal of the header through the raw library on device buffers: a negative return, a message naming the entry point, and
    the outputs still hold their sentinel afterwards"""
    lib, st = _lib.load(), hip._stream()
    B, S, D = 3, 40, 256
    x, w, dp = (t.to(DEV) for t in _inputs(B, S, D, 5))
    mask = torch.ones(B, S, dtype=torch.uint8, device=DEV)
    out = torch.full((B, D), 12345.0, dtype=F32, device=DEV)
    dx = torch.full((B, S, D), 0, dtype=torch.int16, device=DEV).fill_(SENTINEL)
    spare = torch.zeros(64, dtype=torch.uint8, device=DEV)

    def calls(mode, **over):
        need = int(lib.ur_pool_norm_workspace_bytes(B, D, mode)) if mode in (1, 2) else 1 << 20
        ws = torch.full((max(need, 16) + 16,), 0x5A, dtype=torch.uint8, device=DEV)
        a = dict(x=x.data_ptr(), w=w.data_ptr(), mask=mask.data_ptr(), out=out.data_ptr(), dx=dx.data_ptr(), g=dp.data_ptr(), ws=ws.data_ptr(),
                 wsb=need, B=B, S=S, D=D, eps=EPS)
        a.update(over)
        rf = lib.ur_pool_norm_fwd(a["x"], a["w"], a["mask"], a["out"], a["B"], a["S"], a["D"], a["eps"], mode, a["ws"], a["wsb"], st)
        mf = lib.ur_last_error()
        rb = lib.ur_pool_norm_bwd(a["g"], a["x"], a["w"], a["mask"], a["dx"], a["B"], a["S"], a["D"], a["eps"], mode, a["ws"], a["wsb"], st)
        mb = lib.ur_last_error()
        assert rf < 0 and b"ur_pool_norm_fwd" in mf, (mode, over, rf, mf)
        assert rb < 0 and b"ur_pool_norm_bwd" in mb, (mode, over, rb, mb)
        torch.cuda.synchronize()
        assert (ws == 0x5A).all(), (mode, over, "the workspace was written")

    for mode in (1, 2):
        for name in ("x", "w", "ws"):
            calls(mode, **{name: None})
            calls(mode, **{name: spare.data_ptr() + 8})                    # misaligned
        calls(mode, out=None, dx=None)
        calls(mode, out=out.data_ptr() + 4, dx=dx.data_ptr() + 2)
        calls(mode, g=None, out=None)
        calls(mode, D=12)
        calls(mode, D=2056)
        calls(mode, S=0)
        calls(mode, S=-1)
        calls(mode, B=-2)
        calls(mode, eps=-1.0)
        calls(mode, wsb=int(lib.ur_pool_norm_workspace_bytes(B, D, mode)) - 1)      # one byte short
    for mode in (0, 3, 7):
        calls(mode)
    torch.cuda.synchronize()
    assert (out == 12345.0).all() and (dx == SENTINEL).all(), "a refused call wrote to its output"
    # B == 0: 0, nothing written
    need = int(lib.ur_pool_norm_workspace_bytes(B, D, 1))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert lib.ur_pool_norm_fwd(x.data_ptr(), w.data_ptr(), None, out.data_ptr(), 0, S, D, EPS, 1, ws.data_ptr(), need, st) == 0
    assert lib.ur_pool_norm_bwd(dp.data_ptr(), x.data_ptr(), w.data_ptr(), None, dx.data_ptr(), 0, S, D, EPS, 2, ws.data_ptr(), need, st) == 0
    torch.cuda.synchronize()
    assert (out == 12345.0).all() and (dx == SENTINEL).all()
    with pytest.raises(ValueError, match="mode"):
        hip.pool_norm_fwd(x, w, EPS, mask, "mean")


def test_zz_worst_ratio_table():
    """prints the worst observed error / bound per kernel and mode over the tests of this module that ran before it (docs/lab_notes.md §32)"""
    print("\n[table] worst error / bound per kernel")
    for k in sorted(WORST):
        print(f"[table]   {k}: {WORST[k]:.4f}")

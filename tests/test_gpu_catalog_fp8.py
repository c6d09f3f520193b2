"""GPU: the FP8 catalogue family (include/unirec_fp8.h) against tests/catalog_fp8_ref.py and against what exists.

  quantise   codes, scale and inv equal the reference IN EVERY BIT: f32 and bf16 sources with ld > D, planted rows (zeros; a exactly
             448 2^-j and the next float above; one large element among tiny ones: subnormal codes, underflow to 0 and -0; a = 2^-70, the
             clamp), and one row pinned at a = 448 holding every e4m3 value, every midpoint and their f32 neighbours, both signs.
  re-rank    index and score bits equal hip.catalog_deep_rerank(user, codes.float(), ...).
  scores     all scores, read through a call with K = N, against float64(q . c) float64(iu8) float64(inv) with the planes the first
             test holds to their bits.  The bound is derived, not measured: products of two e4m3 values are exact in f32; what rounds is
             at most D f32 additions in some order and two multiplies, so
                 |err| <= ((D + 2) 2^-23 sum_d |q_bd c_nd|) iu8 inv + 2^-22 |s|
             (the unit 2^-23 is twice the rounding unit: it covers an accumulator that truncates).  The worst err / bound is printed
             (run with -s; docs/lab_notes.md records it), and beside it the error of hip.catalog_coarse_deep_select on the same operands
             -- codes and quantised users are exact in bf16, so the bf16 kernel computes the same quantity.  Where the derived bound is
             missed the issue's fallback applies: 4 x that bf16 kernel's worst error on the same operands.
             MEASURED on an MI355X: the derived bound holds at every shape, worst err / bound 0.038 (D = 16), 0.012 (48), 0.0007 (1024,
             1056), 0.0001 (2048); |err| <= 8.8e-8.  The scorer widens the codes and runs v_mfma_f32_16x16x32_bf16.  Its first form ran
             v_mfma_f32_16x16x32_fp8_fp8 on the bytes and FAILED this test: worst err / bound 34.2 at D = 16 and 5.5 at D = 48 (|err| up to
             6.6e-5 against the bf16 kernel's 6.1e-8), and the fallback missed at every width -- that instruction aligns the 32 products
             of a step to the largest and truncates them near 2^-14 of it (448 * 448 + x y returned 200704 + 8 for x y = 12 and 200704
             for every x y < 8).  test_scores_of_subnormal_and_small_codes_against_float64 holds the widening itself: rows of the codes
             nearest zero, where a flushed subnormal or another e4m3 dialect would show at full size.
  select     a pure function of the scores: N = 3077 at chunk_rows = 1024 (four chunks, the last short) against
             tests/catalog_coarse_ref.select on scores rebuilt from 1024-row slices, exactly; planted copies of the ground truth give
             rank 1 (the diagonal launch has the chunk pass's bits); identical rows tie to the lowest indices; two calls, the same bits.
  end to end Fp8CatalogEvaluator.retrieve_two_stage against the reference re-rank of its own stage-1 list, against the exact
             retrieval over the dequantised catalogue on a constructed case, and the rerank_with= route.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import catalog_coarse_ref as cref  # noqa: E402
from tests import catalog_fp8_ref as ref  # noqa: E402
from unirec_amd import _lib, hip  # noqa: E402
from unirec_amd.evaluation import CatalogEvaluator, Fp8CatalogEvaluator  # noqa: E402

DEV = "cuda"
F32, BF16, I32, I64, U8 = torch.float32, torch.bfloat16, torch.int32, torch.int64, torch.uint8

COVERS = {
    "ur_catalog_fp8_quantize": ["test_quantize_bits", "test_quantize_every_value_and_midpoint"],
    "ur_catalog_fp8_select": ["test_scores_against_float64", "test_select_is_a_pure_function_of_the_scores"],
    "ur_catalog_fp8_rerank": ["test_rerank_bits"],
}


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- quantise ----------------------------------------------------------------------------------------------------------------------------
def _planted(kind, D, dtype, g):
    """one row [D] f32 of the planted kinds; every value is exact in `dtype`"""
    eps = 2.0 ** -23 if dtype is F32 else 2.0 ** -7
    small = (torch.rand(D, generator=g) - 0.5).to(dtype).float()
    if kind == 0:                                     # all zeros
        return torch.zeros(D)
    if kind in (1, 2, 3, 4):                          # a exactly 448 2^-j (j = 3, 12), and the next float above it
        j = 3 if kind < 3 else 12
        a = 448.0 * 2.0 ** -j * (1.0 if kind in (1, 3) else 1.0 + eps)
        row = small * a
        row[D // 2] = -a
        return row.to(dtype).float()
    if kind == 5:                                     # one large element among tiny ones: a = 1, e = 8; subnormal codes, underflow, -0
        tiny = torch.tensor([2.0 ** -17, -2.0 ** -17, 3 * 2.0 ** -18, -3 * 2.0 ** -18, 2.0 ** -18, -2.0 ** -18, 2.0 ** -19, -2.0 ** -19,
                             2.0 ** -30, -2.0 ** -30, 5 * 2.0 ** -19, -7 * 2.0 ** -17, 2.0 ** -14, 9 * 2.0 ** -18, 0.0, -0.0])
        row = tiny.repeat((D + 15) // 16)[:D].clone()
        row[3] = 1.0
        return row
    tiny = torch.tensor([2.0 ** -70, -2.0 ** -71, 1.5 * 2.0 ** -73, -2.0 ** -74, 2.0 ** -75, -2.0 ** -75, 3 * 2.0 ** -76, 2.0 ** -90])
    return tiny.repeat((D + 7) // 8)[:D].clone()      # a = 2^-70: e would be 78, the clamp gives 64 and x 2^64 <= 2^-6


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("N", [1, 17, 1025])
@pytest.mark.parametrize("D", [16, 48, 1024, 2048])
def test_quantize_bits(D, N, dtype):
    g = _gen(1000 * D + N)
    ld = D + (24 if dtype is BF16 else 12)
    mag = torch.exp2(torch.randint(-20, 20, (N, 1), generator=g).float())
    src = (torch.randn(N, ld, generator=g) * mag).to(dtype)
    for i in range(7):                               # the planted rows (with N == 1, the kind moves with D)
        n = (i * 3) % N if N > 1 else 0
        kind = i if N > 1 else (D // 16) % 7
        src[n, :D] = _planted(kind, D, dtype, g).to(dtype)
    codes, scale, inv = hip.catalog_fp8_quantize(src.to(DEV)[:, :D])
    torch.cuda.synchronize()
    rc, rs, ri = ref.quantize(src[:, :D])
    assert codes.dtype == U8 and codes.shape == (N, D) and np.array_equal(codes.cpu().numpy(), rc)
    assert np.array_equal(scale.cpu().numpy().view(np.uint32), rs.view(np.uint32))
    assert np.array_equal(inv.cpu().numpy().view(np.uint32), ri.view(np.uint32))
    # decoding is exact
    deq = (codes.view(torch.float8_e4m3fn).float() * scale[:, None]).cpu()
    assert np.array_equal(deq.numpy(), ref.dequantize(rc, rs))
    # out=: the same bits into a slice of a larger catalogue
    big = (torch.zeros(N + 2, D, dtype=U8, device=DEV), torch.zeros(N + 2, device=DEV), torch.zeros(N + 2, device=DEV))
    got = hip.catalog_fp8_quantize(src.to(DEV)[:, :D], out=tuple(t[1:N + 1] for t in big))
    assert torch.equal(got[0], codes) and torch.equal(_bits(got[1]), _bits(scale)) and torch.equal(_bits(got[2]), _bits(inv))
    assert int(big[0][0].sum()) == 0 and int(big[0][-1].sum()) == 0


def test_quantize_every_value_and_midpoint():
    """one row of D = 2048 pinned at a = 448 (e = 0, so the row's elements are what is rounded): every representable e4m3 value, every
    midpoint between neighbours and the f32 neighbours of each on both sides, both signs"""
    vals = np.sort(ref.DECODE[:127].astype(np.float64))                                  # 0 .. 448, the 127 non-negative finite values
    pts = np.concatenate([vals, (vals[1:] + vals[:-1]) / 2]).astype(np.float32)          # midpoints are exact in f32
    b = pts.view(np.uint32).astype(np.int64)
    top = int(np.float32(448.0).view(np.uint32))
    near = np.concatenate([np.clip(b + k, 0, top) for k in (-1, 0, 1)]).astype(np.uint32).view(np.float32)
    both = np.unique(np.concatenate([near, -near]).view(np.uint32)).view(np.float32)     # (-0 and +0 are both kept: distinct bits)
    assert 1400 <= both.size <= 2047, both.size
    row = np.zeros(2048, dtype=np.float32)
    row[0] = 448.0
    row[1:1 + both.size] = both
    src = torch.from_numpy(row)[None]
    codes, scale, inv = hip.catalog_fp8_quantize(src.to(DEV))
    rc, rs, ri = ref.quantize(src)
    assert float(scale[0]) == 1.0 and rs[0] == 1.0
    assert np.array_equal(codes.cpu().numpy(), rc), np.nonzero(codes.cpu().numpy() != rc)
    assert np.array_equal(inv.cpu().numpy().view(np.uint32), ri.view(np.uint32))
    # the row reaches every finite code of either sign
    assert set(np.unique(rc).tolist()) == set(range(0, 127)) | set(range(128, 255))


# ---- re-rank -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [16, 1024, 2048])
@pytest.mark.parametrize("K_in", [1, 128, 129, 1024])
def test_rerank_bits(K_in, D):
    g = _gen(7 * D + K_in)
    B, N = 5, 1500
    cat = torch.randn(N, D, generator=g) * torch.exp2(torch.randint(-6, 6, (N, 1), generator=g).float())
    user = torch.randn(B, D, generator=g).to(DEV)
    codes, scale, inv = hip.catalog_fp8_quantize(cat.to(DEV))
    index = torch.randint(0, N, (B, K_in), generator=g).to(I32)
    if K_in > 4:
        index[:, 1] = -1                               # empty slots: -1, N and beyond
        index[1, 2] = N
        index[2, 3] = 2 ** 31 - 1
        index[:, 4] = index[:, 0]                      # a duplicated index is scored and listed twice
    else:
        index[1, 0] = -1
    index = index.to(DEV)
    wide = codes.view(torch.float8_e4m3fn).float()
    for k in sorted({1, K_in, (K_in + 1) // 2}):
        idx, val = hip.catalog_fp8_rerank(user, codes, index, inv, k)
        widx, wval, _ = hip.catalog_deep_rerank(user, wide, index, k, inv.clone())
        assert idx.shape == (B, k) and torch.equal(idx, widx) and torch.equal(_bits(val), _bits(wval)), (K_in, D, k)
    # the plane the quantiser wrote is the one the exact path computes for codes.float()
    _, _, own = hip.catalog_deep_rerank(user, wide, index, 1)
    assert torch.equal(_bits(own), _bits(inv))
    again = hip.catalog_fp8_rerank(user, codes.view(torch.float8_e4m3fn), index, inv, K_in)
    first = hip.catalog_fp8_rerank(user, codes, index, inv, K_in)
    assert torch.equal(again[0], first[0]) and torch.equal(_bits(again[1]), _bits(first[1]))


# ---- scores against float64 ----------------------------------------------------------------------------------------------------------------
def _all_scores(user, codes, inv, **kw):
    """f32 [B, N] on the host: every score of a catalogue of at most 1024 rows, read through a call with K = N"""
    N = codes.shape[0]
    idx, val, _ = hip.catalog_fp8_select(user, codes, N, inv, **kw)
    idx, val = idx.cpu().long(), val.cpu()
    assert bool((idx.sort(dim=1).values == torch.arange(N)[None]).all()), "a call with K = N lists every row once"
    return torch.zeros_like(val).scatter_(1, idx, val)


_WORST = {}


@pytest.mark.parametrize("D", [16, 48, 1024, 1056, 2048])
@pytest.mark.parametrize("N", [1, 255, 1024])
@pytest.mark.parametrize("B", [1, 17, 65])
def test_scores_against_float64(B, N, D):
    if D == 2048 and B == 65:
        B = 33                                         # the wide kernel stages 32 users: 33 is its ragged second group
    g = _gen(B * 100000 + N * 10 + D)
    cat = torch.randn(N, D, generator=g) * torch.exp2(torch.randint(-8, 8, (N, 1), generator=g).float())
    user = torch.randn(B, D, generator=g)
    if N > 4:
        cat[3] = user[0] * 0.37                        # a near-parallel pair (cosine near 1) and an orthogonal-ish rest
        cat[4, D // 2:] = 0
    codes, _, inv = hip.catalog_fp8_quantize(cat.to(DEV))
    q, _, iu8 = hip.catalog_fp8_quantize(user.to(DEV))                    # the planes test_quantize_bits holds to their bits
    s8 = _all_scores(user.to(DEV), codes, inv).numpy().astype(np.float64)
    s64, bound = ref.scores64(q.cpu().numpy(), iu8.cpu().numpy(), codes.cpu().numpy(), inv.cpu().numpy())
    err = np.abs(s8 - s64)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    # for the record: the bf16-MFMA kernel on the same operands (code values are exact in bf16)
    qb, cb = q.view(torch.float8_e4m3fn).to(BF16).float(), codes.view(torch.float8_e4m3fn).to(BF16)
    bi, bv, _, _ = hip.catalog_coarse_deep_select(qb, cb, N)
    s16 = torch.zeros(B, N).scatter_(1, bi.cpu().long(), bv.cpu()).numpy().astype(np.float64)
    err16 = np.abs(s16 - s64)
    _WORST[(B, N, D)] = worst
    print(f"fp8 scores B={B} N={N} D={D}: worst err/bound {worst:.4f}, max |err| fp8 {err.max():.3e}, bf16 kernel {err16.max():.3e}, "
          f"bf16 err/bound {float((err16 / np.maximum(bound, 1e-300)).max()):.4f}; overall worst so far {max(_WORST.values()):.4f}")
    # the derived bound; where the instruction misses it, the project's rule for coarse scores: 4 x the bf16 kernel's worst error on the
    # same operands, measured above
    assert (err <= bound).all() or err.max() <= 4.0 * err16.max(), (B, N, D, worst, float(err.max()), float(err16.max()))


def test_scores_of_subnormal_and_small_codes_against_float64():
    """rows made of the 30 codes nearest zero only (subnormals m 2^-9 and the first binade, both signs) against users of large elements:
    every product is of the same order, so a code the scorer widened wrongly -- a flushed subnormal, another e4m3 dialect -- shows in
    the score at full size; and rows holding every finite code, for the rest of the table"""
    g = _gen(21)
    B, N, D = 17, 255, 48
    small = torch.tensor([c for c in range(1, 16)] + [0x80 + c for c in range(1, 16)], dtype=U8)
    codes = small[torch.randint(0, small.numel(), (N, D), generator=g)]
    every = torch.tensor([c for c in range(256) if c & 0x7f != 0x7f], dtype=U8)
    codes[200:] = every[torch.randint(0, every.numel(), (N - 200, D), generator=g)]
    user = (torch.randint(0, 2, (B, D), generator=g) * 2 - 1).float() * (224.0 + 32.0 * torch.randint(0, 8, (B, D), generator=g))
    user[:, 0] = 448.0                                 # e = 0: the users are their own codes
    cdev = codes.to(DEV)
    inv = torch.from_numpy(ref.row_inv_norm(ref.decode(codes.numpy()))).to(DEV)
    q, scale, iu8 = hip.catalog_fp8_quantize(user.to(DEV))
    assert bool((scale == 1).all()) and np.array_equal(ref.decode(q.cpu().numpy()), user.numpy())
    s8 = _all_scores(user.to(DEV), cdev, inv).numpy().astype(np.float64)
    s64, bound = ref.scores64(q.cpu().numpy(), iu8.cpu().numpy(), codes.numpy(), inv.cpu().numpy())
    err = np.abs(s8 - s64)
    print(f"small codes: worst err/bound {float((err / bound).max()):.4f}, largest |s| {np.abs(s64).max():.3f}")
    assert np.abs(s64[:, :200]).max() > 0.2 and (err <= bound).all()


# ---- select is a pure function of the scores ---------------------------------------------------------------------------------------------
_SEL = {}


def _select_case():
    if _SEL:
        return _SEL
    g = _gen(77)
    B, N, D, E = 6, 3077, 48, 3
    cat = torch.randn(N, D, generator=g)
    gt = torch.tensor([1500, 7, 3076, 2048, 1023, 602])                      # the last one lies inside the run of identical rows
    user = cat[gt] + 0.05 * torch.randn(B, D, generator=g)
    for b, (lo, hi) in enumerate(((3, 2900), (0, 1024), (5, 1025), (2047, 3075), (10, 2049))):      # copies below and above, in other chunks
        cat[lo] = cat[gt[b]]
        cat[hi] = cat[gt[b]]
    cat[600:606] = cat[602]                            # six identical rows: user 5's ground truth and five copies
    exclude = torch.tensor([[-1, 4, 2900], [-1, -1, 7], [5, 6, 3076], [1, 2, 3], [-1, -1, -1], [-1, -1, -1]], dtype=I64)      # rows 1, 2 name their own gt
    codes, _, inv = hip.catalog_fp8_quantize(cat.to(DEV))
    u = user.to(DEV)
    scores = torch.empty(B, N)
    for c0 in range(0, N, 1024):                       # rebuilt from 1024-row slices, each read with K = its length
        c1 = min(N, c0 + 1024)
        scores[:, c0:c1] = _all_scores(u, codes[c0:c1].contiguous(), inv[c0:c1].contiguous())
    _SEL.update(B=B, N=N, D=D, E=E, user=u, codes=codes, inv=inv, gt=gt, exclude=exclude, scores=scores.numpy().astype(np.float64))
    return _SEL


@pytest.mark.parametrize("K", [1, 128, 129, 1000])
def test_select_is_a_pure_function_of_the_scores(K):
    c = _select_case()
    for E in (0, 3):
        ex = c["exclude"] if E else None
        for with_gt in (True, False):
            gt = c["gt"] if with_gt else None
            widx, wval, wrank = cref.select(c["scores"], K, None if gt is None else gt.numpy(), None if ex is None else ex.numpy())
            for segments in (0, 1, 8):
                idx, val, rank = hip.catalog_fp8_select(c["user"], c["codes"], K, c["inv"], gt_index=gt, exclude=None if ex is None else ex.to(DEV),
                                                        chunk_rows=1024, segments=segments)
                what = (K, E, with_gt, segments)
                assert np.array_equal(idx.cpu().numpy(), widx), what
                assert np.array_equal(val.cpu().numpy().astype(np.float64), wval), what
                if with_gt:
                    assert np.array_equal(rank.cpu().numpy(), wrank), what
                    # the copies of a user's ground truth tie with it bit for bit: nothing lies strictly above it
                    assert (rank.cpu().numpy() == 1).all(), (what, rank)
                else:
                    assert rank is None
                # identical rows tie to the lowest indices: user 5's list opens with 600, 601, ..
                assert idx[5, :min(K, 6)].tolist() == list(range(600, 600 + min(K, 6))), what
                again = hip.catalog_fp8_select(c["user"], c["codes"], K, c["inv"], gt_index=gt, exclude=None if ex is None else ex.to(DEV),
                                               chunk_rows=1024, segments=segments)
                assert torch.equal(again[0], idx) and torch.equal(_bits(again[1]), _bits(val)), what
    assert all(len(set(c["scores"][b, 600:606].tolist())) == 1 for b in range(c["B"]))       # identical rows, one score: a function of the pair
    # the library's own chunking and one chunk of everything give the same lists
    one = hip.catalog_fp8_select(c["user"], c["codes"], K, c["inv"], gt_index=c["gt"], chunk_rows=4096)
    own = hip.catalog_fp8_select(c["user"], c["codes"], K, c["inv"], gt_index=c["gt"])
    assert torch.equal(one[0], own[0]) and torch.equal(_bits(one[1]), _bits(own[1])) and torch.equal(one[2], own[2])


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def test_retrieve_two_stage_equals_the_reference_rerank_of_its_own_shortlist():
    g = _gen(5)
    B, N, D, k, S = 9, 3000, 64, 20, 300
    cat = torch.randn(N, D, generator=g)
    user = torch.randn(B, D, generator=g)
    gt = torch.randint(0, N, (B,), generator=g)
    ev = Fp8CatalogEvaluator(cat, device=DEV, block_rows=701)                 # five blocks, the last short
    whole = Fp8CatalogEvaluator(cat.to(DEV), device=DEV)
    assert torch.equal(ev.codes, whole.codes) and torch.equal(_bits(ev.scale), _bits(whole.scale)) and torch.equal(_bits(ev.inv), _bits(whole.inv))
    # exactly N D bytes of codes and no other tensor of size N x D
    held = {n: t for n, t in vars(ev).items() if isinstance(t, torch.Tensor)}
    assert sorted(held) == ["codes", "inv", "scale"] and ev.codes.numel() * ev.codes.element_size() == N * D
    assert all(t.numel() == N for n, t in held.items() if n != "codes")
    out = ev.retrieve_two_stage(user, k=k, shortlist=S, gt_index=gt, exclude=[[1, 2]] * B, ks=(1, 10), chunk_rows=1024)
    assert out["rank_is_coarse"] is True and out["catalog_dtype"] == "fp8_e4m3" and set(out["hit_at"]) == {1, 10}
    u = user.to(DEV)
    ex = torch.tensor([[1, 2]] * B, dtype=I64, device=DEV)
    short, _, rank = hip.catalog_fp8_select(u, ev.codes, S, ev.inv, gt_index=gt.to(DEV), exclude=ex, chunk_rows=1024)
    assert torch.equal(out["rank"], rank)
    s64 = ref.exact_scores64(user, ev.codes.cpu().numpy())
    ridx, rval = cref.rerank(s64, short.cpu().numpy(), k)
    bound = (D // 64 + 16) * 2.0 ** -24                # the exact chain: a lane's fmaf chain, six tree levels, two multiplies; |cosine| <= 1
    idx, val = out["topk_index"].cpu().numpy(), out["topk_score"].cpu().numpy().astype(np.float64)
    assert np.abs(val - np.take_along_axis(s64, idx.astype(np.int64), 1)).max() <= bound
    gaps_ok = np.array([np.all(np.abs(np.diff(rval[b])) > 2 * bound) for b in range(B)])
    assert gaps_ok.sum() >= B - 1 and (idx[gaps_ok] == ridx[gaps_ok]).all()
    # from_codes recomputes the norm plane; dequantized() is exact
    again = Fp8CatalogEvaluator.from_codes(ev.codes, ev.scale)
    assert torch.equal(_bits(again.inv), _bits(ev.inv))
    assert np.array_equal(ev.dequantized().cpu().numpy(), ref.dequantize(ev.codes.cpu().numpy(), ev.scale.cpu().numpy()))
    assert torch.equal(ev.dequantized([5, 0, 2999]), ev.dequantized()[[5, 0, 2999]])
    # CatalogEvaluator.quantized(): the same catalogue
    assert torch.equal(CatalogEvaluator(cat, device=DEV).quantized().codes, ev.codes)


def test_constructed_catalogue_matches_the_exact_retrieval_and_rerank_with():
    g = _gen(11)
    B, N, D, k = 12, 4000, 1024, 4
    cat = torch.randn(N, D, generator=g)
    base = torch.unique(torch.randint(0, N // 8, (B,), generator=g)) * 8     # distinct rows 8 apart; the near-copies follow each
    B = base.numel()
    for b in range(B):
        for j in range(1, k):
            cat[int(base[b]) + j] = cat[base[b]] + (0.15 * j) * torch.randn(D, generator=g)
    user = cat[base] + 0.05 * torch.randn(B, D, generator=g)
    ev = Fp8CatalogEvaluator(cat, device=DEV)
    deq = ev.dequantized()
    # before any retrieval: in float64, every user's k-th and (k + 1)-th exact scores over the quantised catalogue lie > 0.25 apart
    s64 = cref.exact_scores(user, deq.cpu())
    top = torch.sort(s64, dim=1, descending=True).values
    gap = (top[:, k - 1] - top[:, k]).numpy()
    print(f"constructed catalogue: smallest gap between the k-th and (k+1)-th exact scores {gap.min():.4f}")
    assert (gap > 0.25).all(), gap
    out = ev.retrieve_two_stage(user, k=k)
    exact = CatalogEvaluator(deq, device=DEV).retrieve(user, k)
    assert torch.equal(out["topk_index"], exact["topk_index"]) and torch.equal(_bits(out["topk_score"]), _bits(exact["topk_score"]))
    # rerank_with=: that evaluator's own re-rank of the same shortlist
    full = CatalogEvaluator(cat, device=DEV, dtype=BF16)
    routed = ev.retrieve_two_stage(user, k=k, shortlist=200, rerank_with=full)
    short, _, _ = hip.catalog_fp8_select(user.to(DEV), ev.codes, 200, ev.inv)
    widx, wval, _ = hip.catalog_deep_rerank(user.to(DEV), full.catalog, short, k)
    assert torch.equal(routed["topk_index"], widx) and torch.equal(_bits(routed["topk_score"]), _bits(wval))
    assert routed["catalog_dtype"] == "fp8_e4m3" and "rank" not in routed


# ---- wrappers ----------------------------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_by_entry_point_and_field():
    u = torch.zeros(2, 32, device=DEV)
    codes = torch.zeros(10, 32, dtype=U8, device=DEV)
    inv = torch.ones(10, device=DEV)
    index = torch.zeros(2, 5, dtype=I32, device=DEV)
    for K in (0, 1025):
        with pytest.raises(_lib.UniRecHipError, match="ur_catalog_fp8_select: K must be"):
            hip.catalog_fp8_select(u, codes, K, inv)
    with pytest.raises(_lib.UniRecHipError, match="ur_catalog_fp8_select: chunk_rows"):
        hip.catalog_fp8_select(u, codes, 4, inv, chunk_rows=1000)
    with pytest.raises(_lib.UniRecHipError, match="ur_catalog_fp8_select: segments"):
        hip.catalog_fp8_select(u, codes, 4, inv, segments=17)
    with pytest.raises(ValueError, match="catalog_fp8_select: codes must be uint8"):
        hip.catalog_fp8_select(u, codes.float(), 4, inv)
    with pytest.raises(ValueError, match="catalog_fp8_select: cat_inv_norm must be f32 of shape"):
        hip.catalog_fp8_select(u, codes, 4, None)
    with pytest.raises(ValueError, match="catalog_fp8_select: user .* must share D"):
        hip.catalog_fp8_select(u[:, :16].contiguous(), codes, 4, inv)
    with pytest.raises(ValueError, match="catalog_fp8_select: D must be a multiple of 16"):
        hip.catalog_fp8_select(torch.zeros(2, 24, device=DEV), torch.zeros(10, 24, dtype=U8, device=DEV), 4, inv)
    with pytest.raises(ValueError, match="catalog_fp8_select: gt_index must have shape"):
        hip.catalog_fp8_select(u, codes, 4, inv, gt_index=torch.zeros(3, dtype=I64))
    for k in (0, 6):
        with pytest.raises(_lib.UniRecHipError, match="ur_catalog_fp8_rerank: k must be"):
            hip.catalog_fp8_rerank(u, codes, index, inv, k)
    with pytest.raises(_lib.UniRecHipError, match="ur_catalog_fp8_rerank: K_in must be"):
        hip.catalog_fp8_rerank(u, codes, torch.zeros(2, 1025, dtype=I32, device=DEV), inv)
    with pytest.raises(ValueError, match="catalog_fp8_rerank: index must be"):
        hip.catalog_fp8_rerank(u, codes, index[:1], inv)
    with pytest.raises(ValueError, match="catalog_fp8_rerank: cat_inv_norm"):
        hip.catalog_fp8_rerank(u, codes, index, inv[:5])
    with pytest.raises(_lib.UniRecHipError, match="ur_catalog_fp8_quantize: D must be"):
        hip.catalog_fp8_quantize(torch.zeros(2, 4096, device=DEV))
    with pytest.raises(ValueError, match="catalog_fp8_quantize: src must be .* multiple of 16"):
        hip.catalog_fp8_quantize(torch.zeros(2, 24, device=DEV))
    with pytest.raises(ValueError, match="catalog_fp8_quantize: src must be f32 or bf16"):
        hip.catalog_fp8_quantize(torch.zeros(2, 32, device=DEV, dtype=torch.float16))
    with pytest.raises(ValueError, match="catalog_fp8_quantize: src must have unit stride"):
        hip.catalog_fp8_quantize(torch.zeros(2, 64, device=DEV)[:, ::2])
    with pytest.raises(ValueError, match="catalog_fp8_quantize: out must be"):
        hip.catalog_fp8_quantize(torch.zeros(2, 32, device=DEV), out=(codes, inv, inv))
    # an empty catalogue and an empty batch are no-ops with the documented outputs
    idx, val, rank = hip.catalog_fp8_select(u, codes[:0], 3, inv[:0], gt_index=torch.zeros(2, dtype=I64))
    assert bool((idx == -1).all()) and bool(torch.isneginf(val).all()) and rank.tolist() == [1, 1]
    idx, val, _ = hip.catalog_fp8_select(u[:0], codes, 3, inv)
    assert idx.shape == (0, 3) and val.shape == (0, 3)

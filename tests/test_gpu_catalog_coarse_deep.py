"""GPU: the long two-stage retrieval family (include/unirec_hip_coarse_deep.h).

Coarse-deep select.  The outputs are a pure function of the coarse scores, so they are held EXACTLY: the whole coarse score matrix of a
case is rebuilt with the older entry point alone -- hip.catalog_coarse_select(user, cat[j:j+128], 128) on consecutive 128-row slices
returns every row of its slice, and the coarse score of a pair does not depend on where the row sits -- the rebuilt matrix is first held
to hip.catalog_coarse_select(K = 128) on the whole catalogue (lists, bits, rank), and then np.lexsort on its bits is the reference for
every K up to 1024: indices, score bits and rank by torch.equal, whatever chunk_rows, segments, the norms' readiness or gt_index.
The scores themselves are held to float64 within the bound of tests/test_gpu_catalog_coarse.py, max(4 x yardstick, 8 f32 ulps of the
largest |s64|), the yardstick now hip.catalog_deep_select(u~.float(), cat, K, scorer="vector") on the same case.  Run with -s for the table.

Deep re-rank.  Index and score bits against hip.catalog_scores on the same pairs under the total order; the float64 bound
(2 (D / 64 + 6) + 6) 2^-24 of the existing re-rank test; for K_in <= 128 every bit of hip.catalog_rerank.

End to end.  retrieve_two_stage(k, S) equals the exact retrieve(k) wherever the float64 reference separates the k-th from the (S + 1)-th
exact score by more than 2^-7, and equals retrieve(k, shortlist=S) tensor for tensor where that call exists (S <= 128)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import catalog_coarse_ref as cref  # noqa: E402
from tests import ref64  # noqa: E402
from tests.test_gpu_catalog_coarse import _bits, _case, _gathered_error, _rerank_case, _retrieve_case, _same  # noqa: E402
from unirec_amd import _lib, hip  # noqa: E402
from unirec_amd.evaluation import CatalogEvaluator  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16

COVERS = {
    "ur_catalog_coarse_deep_select": ["test_coarse_deep_select_equals_the_order_of_the_rebuilt_coarse_scores",
                                      "test_coarse_deep_select_equals_coarse_select_up_to_128"],
    "ur_catalog_deep_rerank": ["test_deep_rerank_against_float64_and_the_exact_scorer_bits"],
}

# (B, N, D, E): fewer candidates than K (1, 17 rows); N around the 1024-score tile with one and several chunks at chunk_rows = 1024; B
# around the coarse scorer's user group (64; 32 for D > 1024); D with a short last K step (8, 24, 40, 264) and full steps only (1024, 2048)
SHAPES = [(1, 1, 8, 0), (17, 17, 40, 0), (15, 1023, 24, 1), (63, 1025, 40, 1), (64, 2049, 1024, 0), (65, 5003, 264, 9), (31, 2049, 2048, 1),
          (33, 1500, 2048, 9)]
KS = (1, 128, 129, 300, 1000, 1024)


@functools.lru_cache(maxsize=None)
def _rebuilt(B, N, D, E):
    """(case, S): S f32 [B,N] on the host, the coarse scores of the case read back through hip.catalog_coarse_select on 128-row slices
    (no exclusion: every row of a slice is in its list).  Nothing of the new code runs here."""
    c = _case(B, N, D, E)
    S = np.full((B, N), np.nan, dtype=np.float32)
    rows = np.arange(B)[:, None]
    for j in range(0, N, 128):
        piece = c["cat"][j:j + 128]
        assert piece.is_contiguous() and piece.data_ptr() % 16 == 0
        idx, val, _, _ = hip.catalog_coarse_select(c["user"], piece, 128)
        idx, val = idx.cpu().numpy(), val.cpu().numpy()
        n = piece.shape[0]
        assert (np.sort(idx[:, :n], axis=1) == np.arange(n)[None, :]).all() and (idx[:, n:] == -1).all()
        S[rows, j + idx[:, :n]] = val[:, :n]
    assert np.isfinite(S).all()
    return c, S


def _reference(c, S, K, with_gt):
    """(index int32 [B,K], score f32 [B,K], rank int32 [B] or None): np.lexsort on the bits of S under the list and rank rules"""
    B, N = S.shape
    gt = c["gt"].numpy() if with_gt else None
    keep = c["keep"] if with_gt or c["ex"] is None else cref.keep_mask(B, N, None, c["ex"].numpy())
    idx = np.full((B, K), -1, dtype=np.int32)
    val = np.full((B, K), -np.inf, dtype=np.float32)
    rank = np.zeros((B,), dtype=np.int32) if with_gt else None
    for b in range(B):
        cand = np.nonzero(keep[b])[0]
        o = cand[np.lexsort((cand, -S[b, cand].astype(np.float64)))][:K]
        idx[b, :len(o)] = o
        val[b, :len(o)] = S[b, o]
        if with_gt:
            others = cand[cand != gt[b]]
            rank[b] = 1 + int((S[b, others] > S[b, gt[b]]).sum())
    return torch.from_numpy(idx), torch.from_numpy(val), None if rank is None else torch.from_numpy(rank)


def _equal(got, want, what):
    assert torch.equal(got[0].cpu(), want[0]), (what, "indices")
    assert torch.equal(_bits(got[1]).cpu(), _bits(want[1])), (what, "score bits")
    assert (got[2] is None and want[2] is None) or torch.equal(got[2].cpu(), want[2]), (what, "rank")


@functools.lru_cache(maxsize=None)
def _checked(B, N, D, E):
    """_rebuilt, with the premise checked first so that a wrong reconstruction cannot pass as a wrong feature: its stable top-128 and its
    rank must be those of hip.catalog_coarse_select(K = 128) on the whole catalogue"""
    c, S = _rebuilt(B, N, D, E)
    for with_gt in (True, False):
        old = hip.catalog_coarse_select(c["user"], c["cat"], 128, gt_index=c["gt"] if with_gt else None, exclude=c["packed"])
        _equal(old[:3], _reference(c, S, 128, with_gt), ("premise", B, N, D, E, with_gt))
    return c, S


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("B,N,D,E", SHAPES)
def test_coarse_deep_select_equals_the_order_of_the_rebuilt_coarse_scores(B, N, D, E, K):
    c, S = _checked(B, N, D, E)
    want = {g: _reference(c, S, K, g) for g in (True, False)}
    cinv = hip.catalog_coarse_select(c["user"], c["cat"], 1)[3]
    for with_gt in (True, False):
        gt = c["gt"] if with_gt else None
        for chunk_rows in (None, 1024):
            for segments in (None, 1, 3, 16):
                got = hip.catalog_coarse_deep_select(c["user"], c["cat"], K, cat_inv_norm=cinv, gt_index=gt, exclude=c["packed"],
                                                     chunk_rows=chunk_rows, segments=segments)
                assert got[0].dtype == torch.int32 and got[1].dtype == F32 and got[0].shape == (B, K) and got[3] is cinv
                _equal(got[:3], want[with_gt], (B, N, D, E, K, with_gt, chunk_rows, segments))
        # the norms not ready: the library writes the same norms and gives the same bits; and a second call repeats them
        fresh = hip.catalog_coarse_deep_select(c["user"], c["cat"], K, gt_index=gt, exclude=c["packed"])
        assert torch.equal(_bits(fresh[3]), _bits(cinv))
        _equal(fresh[:3], want[with_gt], (B, N, D, E, K, with_gt, "norms not ready"))
        assert _same(fresh, hip.catalog_coarse_deep_select(c["user"], c["cat"], K, gt_index=gt, exclude=c["packed"]))


@pytest.mark.parametrize("B,N,D,E", SHAPES)
def test_coarse_deep_select_equals_coarse_select_up_to_128(B, N, D, E):
    c = _case(B, N, D, E)
    for K in (1, 10, 128):
        for gt in (c["gt"], None):
            old = hip.catalog_coarse_select(c["user"], c["cat"], K, gt_index=gt, exclude=c["packed"])
            for chunk_rows, segments in ((None, None), (1024, 3)):
                new = hip.catalog_coarse_deep_select(c["user"], c["cat"], K, gt_index=gt, exclude=c["packed"], chunk_rows=chunk_rows,
                                                     segments=segments)
                assert _same(old, new) and torch.equal(_bits(old[3]), _bits(new[3])), (K, gt is None, chunk_rows, segments)


def _rising_rows(N, D):
    """[N, D] bf16 rows whose cosine with u = (+-1 on the first D / 2 components, 0 after) rises strictly with the row, by more than 1e-4
    per row in float64: row = a u + b v, v = +-1 on the other half, (a, b) integers of at most 8 bits -- every row, every product and
    every partial sum is exact in bf16 / f32, so the coarse scores differ from float64 by the norms' few f32 roundings alone"""
    h = D // 2
    g = torch.Generator().manual_seed(N + D)
    u = torch.zeros(D)
    v = torch.zeros(D)
    u[:h] = torch.randint(0, 2, (h,), generator=g).float() * 2 - 1
    v[h:] = torch.randint(0, 2, (D - h,), generator=g).float() * 2 - 1
    a, b = np.meshgrid(np.arange(-256, 257), np.arange(0, 257), indexing="ij")
    a, b = a.reshape(-1), b.reshape(-1)
    ok = np.gcd(a, b) == 1
    a, b = a[ok], b[ok]
    cos = a * np.sqrt(h) / np.sqrt(a.astype(np.float64) ** 2 * h + b.astype(np.float64) ** 2 * (D - h))
    o = np.argsort(cos, kind="stable")
    pick, last = [], -2.0
    for i in o:
        if cos[i] - last > 1.5e-4:
            pick.append(i)
            last = cos[i]
    assert len(pick) >= N, (len(pick), N)
    pick = np.array(pick)[np.floor(np.linspace(0, len(pick) - 1, N)).astype(np.int64)]      # (a step >= 1: strictly increasing)
    rows = torch.from_numpy(a[pick]).float()[:, None] * u[None, :] + torch.from_numpy(b[pick]).float()[:, None] * v[None, :]
    cat = rows.to(BF16)
    assert torch.equal(cat.float(), rows)
    return u[None, :].contiguous(), cat


@pytest.mark.parametrize("chunk_rows", [None, 1024])
def test_a_rising_score_fills_the_survivor_buffer_and_the_list_is_the_last_rows(chunk_rows):
    """the worst case of the deferred merge: every score passes the stale threshold, tile after tile, in one workgroup per user"""
    N, D, K = 5003, 264, 1024
    user, cat = _rising_rows(N, D)
    s64 = cref.coarse_scores(user, cat).numpy()[0]
    assert np.diff(s64).min() > 1e-4, "precondition: the float64 coarse cosine rises by more than 1e-4 per row"
    gt = torch.tensor([N - 7])
    idx, val, rank, _ = hip.catalog_coarse_deep_select(user.to(DEV), cat.to(DEV), K, gt_index=gt, chunk_rows=chunk_rows, segments=1)
    assert idx[0].cpu().tolist() == list(range(N - 1, N - 1 - K, -1))
    assert int(rank[0]) == 7
    assert np.abs(val[0].cpu().numpy().astype(np.float64) - s64[::-1][:K]).max() <= 1e-6


@pytest.mark.parametrize("D", [264, 2048])
def test_identical_rows_tie_to_the_lowest_indices_and_rank_one(D):
    K, N, B = 1024, 2049, 33
    g = torch.Generator().manual_seed(D + K)
    user = torch.randn(B, D, generator=g).to(DEV)
    cat = torch.randn(1, D, generator=g).to(BF16).repeat(N, 1).contiguous().to(DEV)
    gt = torch.randint(0, N, (B,), generator=g)
    for chunk_rows, segments in ((None, None), (1024, 1), (1024, 16)):
        idx, val, rank, _ = hip.catalog_coarse_deep_select(user, cat, K, gt_index=gt, chunk_rows=chunk_rows, segments=segments)
        assert torch.equal(idx.cpu(), torch.arange(K, dtype=torch.int32).repeat(B, 1))
        assert torch.equal(_bits(val), _bits(val[:, :1]).repeat(1, K)) and bool(torch.isfinite(val).all())
        assert torch.equal(rank.cpu(), torch.ones(B, dtype=torch.int32)), rank


@pytest.mark.parametrize("chunk_rows", [None, 1024])
def test_everything_but_the_ground_truth_excluded(chunk_rows):
    c = _case(17, 1300, 40)
    ex = torch.stack([torch.tensor([n for n in range(1300) if n != int(g)]) for g in c["gt"]]).to(DEV)
    idx, val, rank, _ = hip.catalog_coarse_deep_select(c["user"], c["cat"], 300, gt_index=c["gt"], exclude=ex, chunk_rows=chunk_rows)
    assert torch.equal(idx[:, 0].cpu(), c["gt"].to(torch.int32)) and bool((idx[:, 1:] == -1).all())
    assert bool(torch.isneginf(val[:, 1:]).all()) and bool(torch.isfinite(val[:, 0]).all())
    assert torch.equal(rank.cpu(), torch.ones(17, dtype=torch.int32))
    old = hip.catalog_coarse_select(c["user"], c["cat"], 1, gt_index=c["gt"], exclude=ex)
    assert torch.equal(_bits(val[:, :1]), _bits(old[1]))


@pytest.mark.parametrize("K", [300, 1024])
@pytest.mark.parametrize("B,N,D,E", SHAPES)
def test_coarse_deep_scores_against_float64(B, N, D, E, K):
    c = _case(B, N, D, E)
    idx, val, _, cinv = hip.catalog_coarse_deep_select(c["user"], c["cat"], K, gt_index=c["gt"], exclude=c["packed"])
    yi, yv, _, _ = hip.catalog_deep_select(c["user"].to(BF16).float(), c["cat"], K, cat_inv_norm=cinv, gt_index=c["gt"], exclude=c["packed"],
                                           scorer="vector")
    yard = _gathered_error(yi, yv, c["s64"])
    e = max(4.0 * yard, 8.0 * float(ref64.f32_ulp(float(np.abs(c["s64"]).max()))))
    measured = _gathered_error(idx, val, c["s64"])
    print(f"\ncoarse-deep B {B:3d} N {N:5d} D {D:5d} K {K:4d} E {E}: measured {measured:.3e}  yardstick {yard:.3e}  bound {e:.3e}  "
          f"ratio {measured / e:.3f}")
    assert measured <= e, (measured, yard, e)


# ---- the deep re-rank ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,N,D,K_in", [(1, 1, 8, 1), (17, 1023, 264, 10), (33, 2049, 1024, 129), (5, 5003, 2048, 1000), (3, 40, 24, 1024),
                                        (64, 5003, 1024, 1024)])
def test_deep_rerank_against_float64_and_the_exact_scorer_bits(B, N, D, K_in, dtype):
    user, cat, index = _rerank_case(B, N, D, K_in, dtype)
    S, cinv = hip.catalog_scores(user, cat.float())                  # the plain f32 call: catalog_scores_kernel, untouched
    S_host, idx_host = S.cpu().numpy(), index.cpu().numpy()
    s64 = cref.exact_scores(user, cat).numpy()
    bound = (2 * (D / 64 + 6) + 6) * 2.0 ** -24                      # the bound of the existing re-rank test, same chain
    for k in sorted({K_in, 1, min(128, K_in)}, reverse=True):
        idx, val, out_cinv = hip.catalog_deep_rerank(user, cat, index, k)
        assert idx.shape == (B, k) and idx.dtype == torch.int32 and val.dtype == F32
        assert torch.equal(_bits(out_cinv), _bits(cinv))
        idx_np, val_np = idx.cpu().numpy(), val.cpu().numpy()
        for b in range(B):
            row = idx_host[b][(idx_host[b] >= 0) & (idx_host[b] < N)]                # (duplicates stay: scored and listed twice)
            o = row[cref.order(S_host[b, row], row)][:k]                             # the total order on the exact scorer's bits
            assert idx_np[b, :len(o)].tolist() == o.tolist(), (b, k)
            assert (val_np[b, :len(o)].view(np.int32) == S_host[b, o].view(np.int32)).all(), (b, k, "score bits")
            assert (idx_np[b, len(o):] == -1).all() and np.isneginf(val_np[b, len(o):]).all()
            assert np.abs(val_np[b, :len(o)].astype(np.float64) - s64[b, o]).max(initial=0.0) <= bound
        again = hip.catalog_deep_rerank(user, cat, index, k, cat_inv_norm=cinv)
        assert again[2] is cinv and torch.equal(again[0], idx) and torch.equal(_bits(again[1]), _bits(val))
        if K_in <= 128:                                              # the short entry point's bits, every one
            old = hip.catalog_rerank(user, cat, index, k, cat_inv_norm=cinv)
            assert torch.equal(old[0], idx) and torch.equal(_bits(old[1]), _bits(val))
    if N > 12 and K_in >= 10:                                        # the tied rows 4 .. 9 came out next to each other, in index order
        idx, val, _ = hip.catalog_deep_rerank(user, cat, index)
        for b in range(B):
            row = idx[b].cpu().tolist()
            tied = sorted(n for n in row if 4 <= n <= 9)
            at = row.index(tied[0])
            assert set(tied) == {4, 5, 6, 7, 8, 9} and row[at:at + len(tied)] == tied
            assert len(set(_bits(val[b, at:at + len(tied)]).cpu().tolist())) == 1


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("K_in", [1, 10, 128])
def test_deep_rerank_equals_rerank_up_to_128(K_in, dtype):
    user, cat, index = _rerank_case(33, 2049, 1024, K_in, dtype)
    for k in sorted({K_in, 1}):
        old, new = hip.catalog_rerank(user, cat, index, k), hip.catalog_deep_rerank(user, cat, index, k)
        assert torch.equal(old[0], new[0]) and torch.equal(_bits(old[1]), _bits(new[1])) and torch.equal(_bits(old[2]), _bits(new[2]))


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,D", [(17, 5003, 264), (33, 2049, 1024)])
def test_retrieve_two_stage_equals_the_exact_retrieve(B, N, D):
    user, cat, gt = _retrieve_case(B, N, D)
    top = np.sort(cref.exact_scores(user, cat).numpy(), axis=1)[:, ::-1]
    ev = CatalogEvaluator(cat, device=DEV, dtype=BF16)
    for k, S in ((10, 129), (200, 1024), (500, 1024), (129, 1024)):
        assert ((top[:, k - 1] - top[:, S]) > 2.0 ** -7).all(), f"precondition: the exact {k}th score clears the exact {S + 1}th by more than 2^-7"
        exact = ev.retrieve(user, k=k, gt_index=gt)
        two = ev.retrieve_two_stage(user, k=k, shortlist=S, gt_index=gt)
        assert torch.equal(two["topk_index"], exact["topk_index"]) and torch.equal(_bits(two["topk_score"]), _bits(exact["topk_score"])), (k, S)
        assert two["rank_is_coarse"] is True and "rank_is_coarse" not in exact
        assert two["rank"].dtype == torch.int32 and 0.0 < two["mrr"] <= 1.0 and set(two["hit_at"]) == {k} and set(two["ndcg_at"]) == {k}
        assert torch.equal(two["rank"], hip.catalog_coarse_deep_select(user.to(DEV), ev.catalog, S, gt_index=gt)[2])
        chunked = ev.retrieve_two_stage(user, k=k, shortlist=S, chunk_rows=1024)
        assert "rank" not in chunked and torch.equal(chunked["topk_index"], exact["topk_index"])
        assert torch.equal(_bits(chunked["topk_score"]), _bits(exact["topk_score"]))
    # where retrieve(k, shortlist=S) exists, the same dict tensor for tensor
    for k, S in ((10, 128), (10, 10)):
        old = ev.retrieve(user, k=k, gt_index=gt, shortlist=S, ks=(1, k))
        new = ev.retrieve_two_stage(user, k=k, shortlist=S, gt_index=gt, ks=(1, k))
        assert sorted(old) == sorted(new)
        for key in old:
            if isinstance(old[key], torch.Tensor):
                assert old[key].dtype == new[key].dtype and torch.equal(_bits(old[key]), _bits(new[key])), (k, S, key)
            else:
                assert old[key] == new[key], (k, S, key)
    # a truncated evaluator holds a contiguous copy: the call runs on it as on any other, and returns the exact scorer's bits
    t = ev.truncated(D // 2 // 8 * 8)
    d = t.catalog.shape[1]
    t_two = t.retrieve_two_stage(user[:, :d], k=200, shortlist=1024)
    S_t = hip.catalog_scores(user[:, :d].contiguous().to(DEV), t.catalog.float())[0]
    assert torch.equal(_bits(t_two["topk_score"]), _bits(torch.gather(S_t, 1, t_two["topk_index"].long())))
    assert bool((t_two["topk_score"][:, :-1] >= t_two["topk_score"][:, 1:]).all())


def test_deep_rerank_restores_the_exact_order_of_planted_near_copies():
    """the planted case of tests/test_gpu_catalog_coarse.py -- twenty near-copies of user 0's best item whose exact cosines lie
    1e-5 .. 2e-5 apart, which rounding the user to bf16 moves past each other -- through a shortlist of 1024"""
    D, N = 264, 2049
    g = torch.Generator().manual_seed(11)
    user = torch.randn(5, D, generator=g)
    cat = torch.randn(N, D, generator=g)
    u0 = user[0] / user[0].norm()
    base = 0.9 * u0 + (1 - 0.81) ** 0.5 * torch.nn.functional.normalize(torch.randn(D, generator=g), dim=0)
    cand = (base[None, :] + 0.2 * torch.randn(8000, D, generator=g) / D ** 0.5).to(BF16)
    se = cref.exact_scores(user[:1], cand)[0].numpy()
    o, pick = np.argsort(-se), []
    for i in o:
        gap = se[pick[-1]] - se[i] if pick else 1.2e-5
        if gap >= 1e-5:
            pick = pick + [i] if gap <= 2e-5 else [i]
        if len(pick) == 20:
            break
    assert len(pick) == 20
    where = torch.randperm(N, generator=g)[:20]
    cat = cat.to(BF16)
    cat[where] = cand[np.array(pick)]
    s_exact, s_coarse = cref.exact_scores(user, cat).numpy(), cref.coarse_scores(user, cat).numpy()
    want = where.numpy()                                               # planted in descending exact order
    assert (np.argsort(-s_exact[0])[:20] == want).all() and np.diff(s_exact[0, want]).max() <= -1e-5
    assert np.diff(s_coarse[0, want]).max() > 1e-5, "precondition: the coarse reference inverts a neighbouring pair by more than 1e-5"
    ev = CatalogEvaluator(cat, device=DEV, dtype=BF16)
    coarse = hip.catalog_coarse_deep_select(user.to(DEV), ev.catalog, 1024)[0]
    assert coarse[0, :20].cpu().tolist() != want.tolist() and sorted(coarse[0, :20].cpu().tolist()) == sorted(want.tolist())
    two, exact = ev.retrieve_two_stage(user, k=20, shortlist=1024), ev.retrieve(user, k=20)
    assert two["topk_index"][0].cpu().tolist() == want.tolist()
    assert torch.equal(two["topk_index"][0], exact["topk_index"][0]) and torch.equal(_bits(two["topk_score"][0]), _bits(exact["topk_score"][0]))


# ---- refusals through the wrappers --------------------------------------------------------------------------------------------------
def test_wrappers_refuse_by_entry_point_and_field():
    c = _case(15, 1023, 24, 1)
    user, cat = c["user"], c["cat"]
    index = torch.zeros(15, 300, dtype=torch.int32, device=DEV)
    sel, rer = hip.catalog_coarse_deep_select, hip.catalog_deep_rerank
    with pytest.raises(_lib.UniRecHipError, match="catalog_coarse_deep_select: user.*no CPU fallback"):
        sel(user.cpu(), cat, 10)
    with pytest.raises(_lib.UniRecHipError, match="catalog_deep_rerank: index.*no CPU fallback"):
        rer(user, cat, index.cpu())
    wide = torch.zeros(1023, 48, dtype=BF16, device=DEV)
    with pytest.raises(ValueError, match="catalog_coarse_deep_select: catalog.*contiguous"):
        sel(user, wide[:, :24], 10)
    with pytest.raises(ValueError, match="catalog_deep_rerank: catalog.*contiguous"):
        rer(user, wide[:, :24], index)
    with pytest.raises(ValueError, match="catalog_coarse_deep_select.*bf16 catalogue"):
        sel(user, cat.float(), 10)
    for K in (0, 1025):
        with pytest.raises(_lib.UniRecHipError, match="ur_catalog_coarse_deep_select: K must be"):
            sel(user, cat, K)
    with pytest.raises(_lib.UniRecHipError, match="ur_catalog_coarse_deep_select: chunk_rows"):
        sel(user, cat, 300, chunk_rows=1000)
    with pytest.raises(_lib.UniRecHipError, match="ur_catalog_coarse_deep_select: segments"):
        sel(user, cat, 300, segments=17)
    with pytest.raises(_lib.UniRecHipError, match="ur_catalog_deep_rerank: K_in must be"):
        rer(user, cat, torch.zeros(15, 1025, dtype=torch.int32, device=DEV))
    for k in (301, 0):
        with pytest.raises(_lib.UniRecHipError, match="ur_catalog_deep_rerank: k must be"):
            rer(user, cat, index, k)
    with pytest.raises(ValueError, match=r"catalog_deep_rerank: index must be \[15, K'\]"):
        rer(user, cat, index[:7].contiguous())
    # the short entry points keep their limits
    with pytest.raises(_lib.UniRecHipError, match="ur_catalog_coarse_select: K must be"):
        hip.catalog_coarse_select(user, cat, 129)
    with pytest.raises(_lib.UniRecHipError, match="ur_catalog_rerank: K_in must be"):
        hip.catalog_rerank(user, cat, torch.zeros(15, 129, dtype=torch.int32, device=DEV))

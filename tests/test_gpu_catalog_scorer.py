"""GPU: the two catalogue scorers (vector, f32 MFMA) on f32 and bf16 catalogues, held EXACTLY -- indices, score bits, ranks and
cat_inv_norm bits -- to the plain f32 path on Cf (the catalogue itself, or its exact .float() when it is stored as bf16) plus numpy:

    S    = hip.catalog_scores(user, Cf) on the host
    list = the non-excluded items in np.argsort(-S, kind="stable") order, cut to K, padded with (-1, -inf)
    rank = 1 + #{non-excluded n : S[n] > S[gt]}

The plain call runs catalog_scores_kernel on f32 and is never touched by the scorer or the dtype under test.  No tolerance anywhere:
an MFMA chain or a sum tree in another order, a pad that is not a real zero or a wrong bf16 widening changes last bits, and the
adversarial catalogue below is built so that last bits decide the order and the counts."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from unirec_amd import hip  # noqa: E402
from unirec_amd.evaluation import CatalogEvaluator, pack_exclude  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
SCORERS = ("vector", "mfma")
DTYPES = (F32, BF16)
combos = pytest.mark.parametrize("scorer,dtype", [(s, d) for s in SCORERS for d in DTYPES],
                                 ids=[f"{s}-{'f32' if d is F32 else 'bf16'}" for s in SCORERS for d in DTYPES])


def _reference(S, K, gt=None, exclude=None):
    """numpy lists / ranks from the plain call's scores; exclude = per-user iterables of indices (negative = empty slot)"""
    B, N = S.shape
    idx = np.full((B, K), -1, dtype=np.int32)
    val = np.full((B, K), -np.inf, dtype=np.float32)
    rank = np.zeros((B,), dtype=np.int32)
    for b in range(B):
        keep = np.ones(N, dtype=bool)
        if exclude is not None:
            for n in exclude[b]:
                n = int(n)
                if 0 <= n < N and (gt is None or n != int(gt[b])):
                    keep[n] = False
        cand = np.nonzero(keep)[0]
        order = np.argsort(-S[b, cand], kind="stable")[:K]
        idx[b, :len(order)] = cand[order]
        val[b, :len(order)] = S[b, cand[order]]
        if gt is not None:
            rank[b] = 1 + int((S[b, cand] > S[b, int(gt[b])]).sum())
    return torch.from_numpy(idx), torch.from_numpy(val), torch.from_numpy(rank)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _plain(user, C):
    """(S on the host, cat_inv_norm) of the plain f32 call on Cf"""
    Cf = C if C.dtype == F32 else C.float()
    S, cinv = hip.catalog_scores(user, Cf)
    assert not bool(torch.isnan(S).any())
    return S.cpu().numpy(), cinv


def _stored(cat, dtype):
    if dtype is F32:
        return cat
    C = cat.to(BF16)
    bits = C.view(torch.int16)
    assert C.numel() < 1000 or bool((bits & 1).any()), "random bf16 values use the whole mantissa: nothing fits fewer bits"
    return C


def _check(got, ref, cinv_ref=None):
    idx, val, rank, cinv = got
    ridx, rval, rrank = ref
    assert idx.dtype == torch.int32 and val.dtype == F32
    assert torch.equal(idx.cpu(), ridx), (idx.cpu(), ridx)
    assert _same_bits(val.cpu(), rval), (val.cpu(), rval)
    if rank is not None:
        assert rank.dtype == torch.int32 and torch.equal(rank.cpu(), rrank), (rank.cpu(), rrank)
    if cinv_ref is not None:
        assert _same_bits(cinv, cinv_ref)


# 1: shapes ---------------------------------------------------------------------------------------------------------------------
# D = 4: only chain 0 exists; 48: chains 0-11; 260: chain 0 has two pieces and every other chain one (the end of a chain);
# 33 users: two ragged user tiles of the MFMA kernel; 2048: its 16-user form; N with chunk_rows 1024: several chunks, the last ragged
SHAPES = [(1, 1, 4, 1), (5, 1000, 48, 10), (3, 2100, 260, 10), (33, 5003, 1024, 10), (130, 2049, 64, 128), (17, 1300, 2048, 128)]


@functools.lru_cache(maxsize=None)
def _case(B, N, D, dtype):
    g = torch.Generator().manual_seed(B + 3 * N + 7 * D)
    user = torch.randn(B, D, generator=g).to(DEV)
    C = _stored(torch.randn(N, D, generator=g).to(DEV), dtype)
    gt = torch.randint(0, N, (B,), generator=g)
    S, cinv = _plain(user, C)
    return user, C, gt, S, cinv


@combos
@pytest.mark.parametrize("B,N,D,K", SHAPES)
def test_shapes(B, N, D, K, scorer, dtype):
    user, C, gt, S, cinv_ref = _case(B, N, D, dtype)
    chunk_rows = 1024 if N > 1024 else None
    ref = _reference(S, K, gt)
    got = hip.catalog_select(user, C, K, gt_index=gt, chunk_rows=chunk_rows, scorer=scorer)          # cat_inv_norm not ready
    _check(got, ref, cinv_ref)
    again = hip.catalog_select(user, C, K, cat_inv_norm=got[3], gt_index=gt, chunk_rows=chunk_rows, scorer=scorer)   # ready
    assert again[3] is got[3]
    _check(again, ref, cinv_ref)
    lists = hip.catalog_select(user, C, K, cat_inv_norm=cinv_ref, chunk_rows=chunk_rows, scorer=scorer)      # no ground truth
    assert lists[2] is None
    _check(lists, _reference(S, K))


# 2: every score of a catalogue, at different places inside a row tile ----------------------------------------------------------
@combos
@pytest.mark.parametrize("offset", [0, 1, 31, 33])
def test_every_score_in_windows(offset, scorer, dtype):
    B, N, D, K = 4, 100, 1024, 100
    user, big, _, _, _ = _case(B, 140, D, dtype)
    C = big[offset:offset + N]
    assert C.is_contiguous() and C.data_ptr() % 16 == 0
    S, cinv_ref = _plain(user, C)
    gt = torch.tensor([0, 99, 50, 31])
    got = hip.catalog_select(user, C, K, gt_index=gt, scorer=scorer)
    _check(got, _reference(S, K, gt), cinv_ref)
    assert sorted(got[0][0].tolist()) == list(range(N)), "K = N: the list holds every item, so every score was compared"


# 3: adversarial rows: only an exact bit match orders and counts right ----------------------------------------------------------
TIED = (0, 1023, 1024, 2500)                 # identical rows either side of a chunk boundary and in three chunks
SCALED = tuple(10 + 9 * j for j in range(300))       # 10 .. 2701: positive scalings of one row, over three chunks
NEAR = tuple(range(2710, 2800))              # that row plus 1e-4 noise
ZERO_ROWS = (2900, 2901, 2902)
SUBNORMAL_ROW, TINY_ROW, HUGE_ROW = 2910, 2920, 2921
ADV = (8, 3000, 1024, 10)


@functools.lru_cache(maxsize=None)
def _adversarial(dtype):
    B, N, D, K = ADV
    g = torch.Generator().manual_seed(23)
    cat = torch.randn(N, D, generator=g)
    v, c0 = torch.randn(D, generator=g), torch.randn(D, generator=g)
    for j, n in enumerate(SCALED):
        cat[n] = c0 * float(0.37 + 1.9 * torch.rand((), generator=g))
    for n in NEAR:
        cat[n] = c0 + 1e-4 * torch.randn(D, generator=g)
    for n in TIED:
        cat[n] = v
    for n in ZERO_ROWS:
        cat[n] = 0.0
    cat[SUBNORMAL_ROW, ::7] = 1e-40                                   # f32 subnormals (bf16 keeps them subnormal)
    cat[SUBNORMAL_ROW, 3::7] = -3e-41
    cat[TINY_ROW] = 1e-20 * torch.randn(D, generator=g)              # squares near 1e-40
    cat[HUGE_ROW, 5::128] = 1e18 * torch.randn(D // 128, generator=g)  # eight squares near 1e36: their sum stays finite
    user = torch.randn(B, D, generator=g)
    user[0], user[1], user[2] = v, 0.0, c0
    user[3] = c0 * 0.731 + 1e-5 * torch.randn(D, generator=g)
    user[5, ::5] = 1e-40
    user[5, 2::5] = -2e-39
    user = user.to(DEV)
    C = _stored(cat.to(DEV), dtype)
    S, cinv = _plain(user, C)
    assert np.isfinite(S).all()
    assert len({S[0, n].tobytes() for n in TIED}) == 1
    near_equal = S[2, list(SCALED)]
    assert float(near_equal.max() - near_equal.min()) < 1e-5 and float(near_equal.min()) > 0.99, "equal cosines up to the last bits"
    assert (S[1] == 0).all() and (S[:, list(ZERO_ROWS)] == 0).all()
    return user, C, S, cinv


@combos
def test_adversarial_rows(scorer, dtype):
    B, N, D, K = ADV
    user, C, S, cinv_ref = _adversarial(dtype)
    ev = CatalogEvaluator(C, device=DEV, dtype=dtype)
    assert ev.catalog.data_ptr() == C.data_ptr(), "the catalogue is kept as it is stored: no copy, no f32 image"
    cinv = None
    for g_ in TIED:                                    # each of the tied items as ground truth: nothing is strictly above it
        gt = torch.tensor([g_, 5, SCALED[150], SCALED[7], ZERO_ROWS[1], SUBNORMAL_ROW, TINY_ROW, HUGE_ROW])
        out = ev.retrieve(user, k=K, gt_index=gt, chunk_rows=1024, scorer=scorer)
        _check((out["topk_index"], out["topk_score"], out["rank"], ev._inv), _reference(S, K, gt), cinv_ref)
        assert cinv is None or ev._inv is cinv
        cinv = ev._inv
        assert out["topk_index"][0, :4].tolist() == list(TIED) and int(out["rank"][0]) == 1
        assert out["topk_index"][1].tolist() == list(range(K)) and int(out["rank"][1]) == 1          # the all-zero user
    # K = 128 over the 390 near-equal scores of users 2 and 3: their order is in the last bits
    got = hip.catalog_select(user, C, 128, cat_inv_norm=cinv_ref, gt_index=gt, chunk_rows=1024, scorer=scorer)
    _check(got, _reference(S, 128, gt))
    assert set(got[0][2].tolist()) <= set(SCALED) | set(NEAR)


@combos
def test_adversarial_exclusion(scorer, dtype):
    B, N, D, K = ADV
    user, C, S, cinv_ref = _adversarial(dtype)
    order = np.argsort(-S, kind="stable")
    gt = torch.tensor([1024, 5, int(order[2, 4]), int(order[3, 5]), 17, 18, 19, 20])
    exclude = [[] for _ in range(B)]                                           # user 1: an empty row
    exclude[0] = [0]                                                           # the top-1 item (the first of the tied four)
    exclude[2] = [int(order[2, 0]), int(gt[2]), int(order[2, 9])]              # holds the user's own ground truth
    exclude[3] = [int(order[3, 0])]                                            # the top-1 item, above the ground truth
    exclude[4] = order[4, :40].tolist() + [int(order[4, 3])]                   # 41 entries, one a duplicate; shorter rows are padded
    exclude[6] = [N, N + 7, 2 ** 40] + order[6, :3].tolist()                   # indices the catalogue does not have match nothing
    exclude[7] = list(SCALED[:30])
    packed = pack_exclude(exclude)
    assert packed.shape[1] == 41 and bool((packed[0] < 0).any()) and int(packed[1].max()) < 0
    ev = CatalogEvaluator(C, device=DEV, dtype=dtype)
    out = ev.retrieve(user, k=K, gt_index=gt, exclude=exclude, chunk_rows=1024, scorer=scorer)
    _check((out["topk_index"], out["topk_score"], out["rank"], ev._inv), _reference(S, K, gt, exclude), cinv_ref)
    assert out["topk_index"][0, :3].tolist() == [1023, 1024, 2500] and int(out["rank"][0]) == 1
    assert int(gt[2]) in out["topk_index"][2].tolist() and exclude[3][0] not in out["topk_index"][3].tolist()
    assert not set(out["topk_index"][7].tolist()) & set(SCALED[:30])


# 4: the same call twice ------------------------------------------------------------------------------------------------------
@combos
def test_repeat_run_is_identical(scorer, dtype):
    user, C, gt, S, cinv_ref = _case(33, 5003, 1024, dtype)
    a = hip.catalog_select(user, C, 10, gt_index=gt, chunk_rows=1024, scorer=scorer)
    b = hip.catalog_select(user, C, 10, gt_index=gt, chunk_rows=1024, scorer=scorer)
    assert torch.equal(a[0], b[0]) and _same_bits(a[1], b[1]) and torch.equal(a[2], b[2]) and _same_bits(a[3], b[3])


# 5: a resident bf16 catalogue: no [B,N] tensor and no f32 copy ------------------------------------------------------------------
def test_bf16_catalogue_no_b_times_n_allocation_and_no_f32_copy():
    B, N, D, K = 64, 200_000, 1024, 10
    g = torch.Generator(device=DEV).manual_seed(5)
    C = torch.randn(N, D, generator=g, device=DEV).to(BF16)
    user = torch.randn(B, D, generator=g, device=DEV)
    gt = torch.randint(0, N, (B,), generator=g, device=DEV)
    S, cinv_ref = _plain(user, C)                       # (the f32 copy of the reference is gone when _plain returns)
    ref = _reference(S, K, gt.cpu())
    ev = CatalogEvaluator(C, device=DEV, dtype=BF16)
    assert ev.catalog.data_ptr() == C.data_ptr()
    for scorer in SCORERS:
        ev.retrieve(user, k=K, gt_index=gt, chunk_rows=8192, scorer=scorer)      # warm-up: norms cached, workspace grown
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = ev.retrieve(user, k=K, gt_index=gt, chunk_rows=8192, scorer=scorer)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        print(f"[alloc] {scorer}: retrieve peak above the level before the call: {peak} bytes; B*N = {B * N} bytes; "
              f"catalogue bf16 {C.numel() * 2} bytes, as f32 {C.numel() * 4} bytes")
        assert peak < B * N, (peak, B * N)
        assert hip.workspace(0, user.device, "catalog_select").numel() < B * N
        _check((out["topk_index"], out["topk_score"], out["rank"], ev._inv), ref, cinv_ref)      # 25 chunks, the last one ragged

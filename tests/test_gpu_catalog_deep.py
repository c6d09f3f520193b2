"""GPU: long exact retrieval lists (ur_catalog_deep_select, hip.catalog_deep_select, CatalogEvaluator.retrieve(k > 128)) held EXACTLY
-- indices, ranks and score bits -- to the reference of tests/test_gpu_catalog_select.py:

    S    = hip.catalog_scores(user, catalog) on the host           (the f32 scores the streaming call must reproduce bit for bit)
    list = the non-excluded items in np.argsort(-S, kind="stable") order, cut to K, padded with (-1, -inf)
    rank = 1 + #{non-excluded n : S[n] > S[gt]}

Never the new kernel itself.  There are no tolerances: the scores are the same f32 values, so torch.equal on everything.  The shapes are
the smallest at which each mechanism can go wrong: K either side of 128 / 256 / 1024, N either side of K, of one tile (1024) and of two,
5003 rows in five chunks with a ragged last one, 1, 2, 5 and 16 workgroups per user (more than the catalogue has tiles included)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from unirec_amd import _lib, hip  # noqa: E402
from unirec_amd.evaluation import CatalogEvaluator, pack_exclude  # noqa: E402

COVERS = {"ur_catalog_deep_select": ["test_boundaries_of_k_n_and_chunks", "test_segments_do_not_show", "test_exclusion", "test_ties",
                                     "test_adversarial_order_for_the_deferred_merge", "test_equals_select_mode_up_to_128"]}

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16


@functools.lru_cache(maxsize=None)
def _case(B, N, D, seed=0):
    """(user, catalogue, S on the host, gt) of one shape: built once, shared by the tests, never modified"""
    g = torch.Generator().manual_seed(1000 * seed + B + N + D)
    user = torch.randn(B, D, generator=g).to(DEV)
    cat = torch.randn(N, D, generator=g).to(DEV)
    gt = torch.randint(0, N, (B,), generator=g)
    S = hip.catalog_scores(user, cat)[0].cpu().numpy()
    return user, cat, S, gt


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
    return torch.from_numpy(idx), torch.from_numpy(val), (torch.from_numpy(rank) if gt is not None else None)


def _same_bits(a, b):
    return torch.equal(a, b) and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _check(out, ref):
    """out: what hip.catalog_deep_select / hip.catalog_select return; ref: _reference's triple (or another call's output)"""
    idx, val, rank = out[0], out[1], out[2]
    assert idx.dtype == torch.int32 and val.dtype == F32
    assert torch.equal(idx.cpu(), ref[0].cpu()), (idx.cpu(), ref[0].cpu())
    assert _same_bits(val.cpu(), ref[1].cpu())
    assert (rank is None) == (ref[2] is None)
    if rank is not None:
        assert rank.dtype == torch.int32 and torch.equal(rank.cpu(), ref[2].cpu()), (rank.cpu(), ref[2].cpu())


# 1 ---------------------------------------------------------------------------------------------------------------------------
# every K with N either side of it, of one tile and of two; 5003 with chunk_rows 1024: five chunks, the last one ragged.  B and D rotate
# through (1, 5, 17, 37) x (8, 48) so that every value meets every K; D = 1024 and 2048 once each (the MFMA scorer is the default at 1024).
KS = (129, 256, 257, 1023, 1024)
BOUNDARY = [(K, N, (1, 5, 17, 37)[(i + j) % 4], (8, 48)[(i + j // 4) % 2])
            for i, K in enumerate(KS) for j, N in enumerate(dict.fromkeys((1, K - 1, K, K + 1, 1025, 2049, 5003)))]
BOUNDARY += [(257, 2049, 17, 1024), (1024, 1025, 5, 2048)]


@pytest.mark.parametrize("K,N,B,D", BOUNDARY)
def test_boundaries_of_k_n_and_chunks(K, N, B, D):
    user, cat, S, gt = _case(B, N, D)
    with_gt, lists = _reference(S, K, gt), _reference(S, K)
    for chunk_rows in (None, 1024):
        _check(hip.catalog_deep_select(user, cat, K, gt_index=gt, chunk_rows=chunk_rows), with_gt)
        _check(hip.catalog_deep_select(user, cat, K, chunk_rows=chunk_rows), lists)
    if N < K:
        out = hip.catalog_deep_select(user, cat, K)
        assert bool((out[0][:, N:] == -1).all()) and bool(torch.isneginf(out[1][:, N:]).all()) and bool((out[0][:, :N] >= 0).all())


# the number of workgroups per user must not show: the library's choice (8 at these B, capped by the tiles of a chunk), 1, 2, 5 and 16;
# with chunk_rows 1024 a chunk is one tile, so all but one segment are empty in every chunk; 16 at N = 5003 is more than there are tiles
@pytest.mark.parametrize("K,N,B,D", [(129, 5003, 5, 48), (1024, 5003, 17, 8), (257, 2049, 37, 48), (1024, 1025, 1, 8)])
def test_segments_do_not_show(K, N, B, D):
    user, cat, S, gt = _case(B, N, D)
    ref = _reference(S, K, gt)
    for segments in (None, 1, 2, 5, 16):
        for chunk_rows in (None, 1024, 2048):
            _check(hip.catalog_deep_select(user, cat, K, gt_index=gt, chunk_rows=chunk_rows, segments=segments), ref)


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 9])
@pytest.mark.parametrize("chunk_rows", [None, 1024])
def test_exclusion(E, chunk_rows):
    B, N, D, K = 17, 5003, 48, 300
    user, cat, S, gt0 = _case(B, N, D)
    order = np.argsort(-S, kind="stable")
    g = torch.Generator().manual_seed(11 + E)
    gt = gt0.clone()
    ex = torch.full((B, E), -1, dtype=torch.int64)                            # negative padding everywhere nothing is written below
    for b in range(B):
        gt[b] = int(order[b, b * 20])                                          # inside the list for most users, at its head for user 0
    for b in range(1, B):
        n_own = 1 + (b % E)
        picks = order[b, torch.randperm(K + 50, generator=g)[:n_own].numpy()]  # items of the list and just behind it
        ex[b, :n_own] = torch.from_numpy(picks.astype(np.int64))
    ex[3, 0] = gt[3]                                                           # a row that holds the user's own ground truth: it stays
    ex[4, -1] = ex[4, 0]                                                       # a duplicate (E = 1: the same slot)
    lists = [row.tolist() for row in ex]
    packed = pack_exclude(ex)
    assert packed.shape == (B, E) and bool((packed[0] < 0).all())
    ref = _reference(S, K, gt, lists)
    _check(hip.catalog_deep_select(user, cat, K, gt_index=gt, exclude=packed.to(DEV), chunk_rows=chunk_rows), ref)
    assert int(gt[3]) in ref[0][3].tolist()
    # shuffled, unsorted lists through retrieve's pack_exclude
    ev = CatalogEvaluator(cat, device=DEV)
    out = ev.retrieve(user, k=K, gt_index=gt, exclude=ex[:, torch.randperm(E, generator=g)].to(DEV), chunk_rows=chunk_rows)
    _check((out["topk_index"], out["topk_score"], out["rank"]), ref)
    out = ev.retrieve(user, k=K, gt_index=gt, exclude=[list(reversed(r)) for r in lists], chunk_rows=chunk_rows)
    _check((out["topk_index"], out["topk_score"], out["rank"]), ref)


def test_exclusion_leaves_fewer_than_k():
    B, N, D, K = 5, 300, 8, 257
    user, cat, S, gt = _case(B, N, D)
    keep = 100                                                                  # 200 of the 300 items excluded: 100 or 101 candidates
    lists = [[n for n in range(N) if (n * 7 + b) % 3 != 0] for b in range(B)]
    ref = _reference(S, K, gt, lists)
    out = hip.catalog_deep_select(user, cat, K, gt_index=gt, exclude=pack_exclude(lists).to(DEV))
    _check(out, ref)
    assert bool((out[0][:, keep + 1:] == -1).all()) and bool(torch.isneginf(out[1][:, keep + 1:]).all()) and bool((out[0][:, :keep] >= 0).all())


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["identical", "sixteen"])
def test_ties(which):
    g = torch.Generator().manual_seed(5)
    D = 48
    if which == "identical":                                                   # 2049 identical rows: the order is the index alone
        N, Ks = 2049, (129, 1024)
        cat = torch.randn(1, D, generator=g).expand(N, D).contiguous().to(DEV)
    else:                                                                      # 16 distinct rows repeated: ties across tiles, chunks, segments
        N, Ks = 5003, (1024,)
        cat = torch.randn(16, D, generator=g).repeat(313, 1)[:N].contiguous().to(DEV)
    user = torch.randn(3, D, generator=g).to(DEV)
    S = hip.catalog_scores(user, cat)[0].cpu().numpy()
    assert len({S[0, n].tobytes() for n in range(0, N, 16)}) == 1
    for K in Ks:
        for gt in (torch.tensor([0, 1024, N - 1]), torch.tensor([1023, 2048, 17])):
            ref = _reference(S, K, gt)
            for chunk_rows, segments in ((None, None), (1024, None), (None, 1), (2048, 2)):
                out = hip.catalog_deep_select(user, cat, K, gt_index=gt, chunk_rows=chunk_rows, segments=segments)
                _check(out, ref)
                if which == "identical":
                    assert out[0][0].tolist() == list(range(K)) and out[2].tolist() == [1, 1, 1]
                    assert len(set(out[1][0].view(torch.int32).tolist())) == 1


# 4 ---------------------------------------------------------------------------------------------------------------------------
# row n = (a_n, 1, 0, ...) with a_n strictly increasing; users +e0 and -e0: one user's score rises with every row -- every score of every
# tile passes the threshold, the case that overruns a survivor buffer sized from the average -- and the other's falls with every row:
# nothing passes after the first K
@pytest.mark.parametrize("chunk_rows", [None, 1024])
def test_adversarial_order_for_the_deferred_merge(chunk_rows):
    B, N, D, K = 2, 5003, 8, 1024
    cat = torch.zeros(N, D)
    cat[:, 0] = torch.linspace(-3.0, 3.0, N)
    cat[:, 1] = 1.0
    user = torch.zeros(B, D)
    user[0, 0], user[1, 0] = 1.0, -1.0
    user, cat = user.to(DEV), cat.to(DEV)
    S = hip.catalog_scores(user, cat)[0].cpu().numpy()
    assert bool((np.diff(S[0]) > 0).all()) and bool((np.diff(S[1]) < 0).all())
    gt = torch.tensor([2500, 2500])
    ref = _reference(S, K, gt)
    assert ref[0][0].tolist() == list(range(N - 1, N - 1 - K, -1)) and ref[0][1].tolist() == list(range(K))
    for segments in (None, 1, 2):
        _check(hip.catalog_deep_select(user, cat, K, gt_index=gt, chunk_rows=chunk_rows, segments=segments), ref)
    _check(hip.catalog_deep_select(user, cat, 129, gt_index=gt, chunk_rows=chunk_rows, segments=1), _reference(S, 129, gt))


# 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 10, 128])
def test_equals_select_mode_up_to_128(K):
    for N, B, D in dict.fromkeys(c[1:] for c in BOUNDARY):                     # every shape of test 1
        user, cat, S, gt = _case(B, N, D)
        for chunk_rows in (None, 1024):
            old = hip.catalog_select(user, cat, K, gt_index=gt, chunk_rows=chunk_rows)
            _check(hip.catalog_deep_select(user, cat, K, gt_index=gt, chunk_rows=chunk_rows), old)
            _check(old, _reference(S, K, gt))


def test_bf16_catalogue_gives_what_its_float_copy_gives():
    user, cat, S, gt = _case(17, 5003, 48)
    cb = cat.to(BF16)
    for K in (129, 1024):
        a = hip.catalog_deep_select(user, cb, K, gt_index=gt)
        b = hip.catalog_deep_select(user, cb.float(), K, gt_index=gt)
        _check(a, b)
        assert _same_bits(a[3], b[3])
        Sb = hip.catalog_scores(user, cb.float())[0].cpu().numpy()
        _check(a, _reference(Sb, K, gt))


@pytest.mark.parametrize("B", [17, 33])                                        # one and two 32-user tiles of the MFMA scorer
def test_scorers_give_the_same_bits_and_two_calls_too(B):
    N, D, K = 2049, 1024, 300
    user, cat, S, gt = _case(B, N, D)
    ref = _reference(S, K, gt)
    for catalog in (cat, cat.to(BF16)):
        want = ref if catalog is cat else None
        outs = [hip.catalog_deep_select(user, catalog, K, gt_index=gt, scorer=sc) for sc in ("vector", "mfma", None, "mfma")]
        for o in outs:
            _check(o, want or outs[0])


def test_retrieve_above_128():
    B, N, D, K = 17, 5003, 48, 300
    user, cat, S, gt = _case(B, N, D)
    ev = CatalogEvaluator(cat, device=DEV)
    ref = _reference(S, K, gt)
    out = ev.retrieve(user, k=K, gt_index=gt, ks=(10, 300, 1000))
    _check((out["topk_index"], out["topk_score"], out["rank"]), ref)
    r = ref[2].to(torch.float64)
    assert abs(out["mrr"] - float((1.0 / r).mean())) <= 1e-15
    assert set(out["hit_at"]) == set(out["ndcg_at"]) == {10, 300, 1000}
    for k in (10, 300, 1000):
        assert abs(out["hit_at"][k] - float((r <= k).to(torch.float64).mean())) <= 1e-15
        assert abs(out["ndcg_at"][k] - float(torch.where(r <= k, 1.0 / torch.log2(1.0 + r), torch.zeros_like(r)).mean())) <= 1e-14
    lists = ev.retrieve(user, k=1024, chunk_rows=1024)
    assert set(lists) == {"topk_index", "topk_score"}
    _check((lists["topk_index"], lists["topk_score"], None), _reference(S, 1024))
    # the short lists still come from select mode, and it still stops at 128
    old = ev.retrieve(user, k=128, gt_index=gt)
    _check((old["topk_index"], old["topk_score"], old["rank"]), _reference(S, 128, gt))
    with pytest.raises(_lib.UniRecHipError, match="ur_catalog_scores"):
        hip.catalog_select(user, cat, 129)


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_wrapper_rejects_host_and_non_contiguous_tensors():
    user, cat, S, gt = _case(5, 1025, 48)
    bad = (_lib.UniRecHipError, ValueError, TypeError)
    with pytest.raises(bad):
        hip.catalog_deep_select(user.cpu(), cat, 300)
    with pytest.raises(bad):
        hip.catalog_deep_select(user, cat.cpu(), 300)
    with pytest.raises(bad):
        hip.catalog_deep_select(user.t().contiguous().t(), cat, 300)
    with pytest.raises(bad):
        hip.catalog_deep_select(user, cat[:, ::2], 300)
    with pytest.raises(bad):
        hip.catalog_deep_select(user, cat, 300, exclude=torch.zeros(5, 4, dtype=torch.int64))            # a host tensor
    with pytest.raises(bad):
        hip.catalog_deep_select(user, cat, 300, exclude=torch.zeros(5, 4, dtype=torch.int32, device=DEV))
    for kw, word in ((dict(K=0), "K must be"), (dict(K=1025), "K must be"), (dict(K=300, chunk_rows=1000), "chunk_rows")):   # the library's own checks
        with pytest.raises(_lib.UniRecHipError) as e:
            hip.catalog_deep_select(user, cat, **kw)
        assert "rc=-" in str(e.value) and "ur_catalog_deep_select" in str(e.value) and word in str(e.value)

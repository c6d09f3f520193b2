"""GPU: streaming catalogue retrieval (ur_catalog_scores with a ur_catalog_select_t, hip.catalog_select, CatalogEvaluator.retrieve)
held EXACTLY -- indices, ranks and score bits -- to the plain path plus numpy:

    S    = hip.catalog_scores(user, catalog) on the host           (the f32 scores the streaming mode must reproduce bit for bit)
    list = the non-excluded items in np.argsort(-S, kind="stable") order, cut to K, padded with (-1, -inf)
    rank = 1 + #{non-excluded n : S[n] > S[gt]}

Never the new kernel itself.  There are no tolerances: the scores are the same f32 values, so torch.equal on everything."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from unirec_amd import _lib, hip  # noqa: E402
from unirec_amd.evaluation import CatalogEvaluator, pack_exclude  # noqa: E402

DEV = "cuda"
F32 = torch.float32


@functools.lru_cache(maxsize=None)
def _case(B, N, D, seed=0):
    """(user, catalogue, evaluator, S on the host, gt) of one shape: built once, shared by the tests, never modified"""
    g = torch.Generator().manual_seed(1000 * seed + B + N + D)
    user = torch.randn(B, D, generator=g).to(DEV)
    cat = torch.randn(N, D, generator=g).to(DEV)
    gt = torch.randint(0, N, (B,), generator=g)
    ev = CatalogEvaluator(cat, device=DEV)
    S = ev.scores(user).cpu().numpy()
    return user, cat, ev, S, gt


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
    return torch.equal(a, b) and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _check(out, ref, with_rank=True):
    idx, val, rank = ref
    assert out["topk_index"].dtype == torch.int32 and out["topk_score"].dtype == F32
    assert torch.equal(out["topk_index"].cpu(), idx), (out["topk_index"].cpu(), idx)
    assert _same_bits(out["topk_score"].cpu(), val)
    if with_rank:
        assert out["rank"].dtype == torch.int32 and torch.equal(out["rank"].cpu(), rank), (out["rank"].cpu(), rank)


# 1 ---------------------------------------------------------------------------------------------------------------------------
# (5003 with chunk_rows 1024: five chunks, the last one ragged; 1025: a second tile of one score; K = 128 > one wave, = the limit)
@pytest.mark.parametrize("B,N,D,K,chunk_rows", [
    (1, 1, 4, 1, None), (5, 1000, 48, 10, None), (17, 5003, 1024, 10, None), (37, 1025, 2048, 128, None), (3, 129, 16, 128, None),
    (1, 1, 4, 1, 1024), (5, 1000, 48, 10, 1024), (17, 5003, 1024, 10, 1024)])
def test_retrieve_equals_evaluate(B, N, D, K, chunk_rows):
    user, cat, ev, S, gt = _case(B, N, D)
    want = ev.evaluate(user, gt, k=K)
    out = ev.retrieve(user, k=K, gt_index=gt, ks=(1, K, 1000), chunk_rows=chunk_rows)
    assert torch.equal(out["topk_index"], want["topk_index"])
    assert _same_bits(out["topk_score"], want["topk_score"])
    assert torch.equal(out["rank"], want["rank"])
    _check(out, _reference(S, K, gt))
    # float64 means of the same ranks: mrr and hit@K are evaluate()'s numbers
    assert abs(out["mrr"] - want["mrr"]) <= 1e-15 and abs(out["hit_at"][K] - want["hit_at_k"]) <= 1e-15
    r = want["rank"].cpu().to(torch.float64)
    assert set(out["hit_at"]) == set(out["ndcg_at"]) == {1, K, 1000}
    for k in (1, K, 1000):
        assert abs(out["hit_at"][k] - float((r <= k).to(torch.float64).mean())) <= 1e-15
        assert abs(out["ndcg_at"][k] - float(torch.where(r <= k, 1.0 / torch.log2(1.0 + r), torch.zeros_like(r)).mean())) <= 1e-14
    # without gt_index: the lists alone
    lists = ev.retrieve(user, k=K, chunk_rows=chunk_rows)
    assert set(lists) == {"topk_index", "topk_score"}
    _check(lists, _reference(S, K), with_rank=False)


# 2 ---------------------------------------------------------------------------------------------------------------------------
def test_fewer_candidates_than_k():
    user, cat, ev, S, gt = _case(2, 3, 8)
    out = ev.retrieve(user, k=10, gt_index=gt)
    _check(out, _reference(S, 10, gt))
    assert bool((out["topk_index"][:, 3:] == -1).all()) and bool(torch.isneginf(out["topk_score"][:, 3:]).all())
    assert bool((out["topk_index"][:, :3] >= 0).all())

    user, cat, ev, S, gt = _case(2, 12, 8)
    gt = torch.tensor([11, 0])
    exclude = [[0, 3, 4, 7, 9], [1, 2, 5, 6, 10]]
    out = ev.retrieve(user, k=10, gt_index=gt, exclude=exclude)
    _check(out, _reference(S, 10, gt, exclude))
    assert bool((out["topk_index"][:, 7:] == -1).all()) and bool(torch.isneginf(out["topk_score"][:, 7:]).all())
    for b in range(2):
        assert sorted(out["topk_index"][b, :7].tolist()) == sorted(set(range(12)) - set(exclude[b]))


# 3 ---------------------------------------------------------------------------------------------------------------------------
TIED = (0, 1023, 1024, 2500)        # either side of the 1024-score tile boundary and, with chunk_rows 1024, in three chunks


@functools.lru_cache(maxsize=None)
def _tie_case():
    N, D = 3000, 48
    g = torch.Generator().manual_seed(7)
    cat = torch.randn(N, D, generator=g)
    v = torch.randn(D, generator=g)
    for n in TIED:
        cat[n] = v                  # identical bits, so identical scores
    user = torch.stack([v, torch.zeros(D), torch.randn(D, generator=g)]).to(DEV)
    ev = CatalogEvaluator(cat.to(DEV), device=DEV)
    return user, ev, ev.scores(user).cpu().numpy()


@pytest.mark.parametrize("chunk_rows", [None, 1024])
def test_ties_go_to_the_lowest_index(chunk_rows):
    user, ev, S = _tie_case()
    K = 10
    assert len({S[0, n].tobytes() for n in TIED}) == 1
    for g_ in TIED:                                   # each of the tied items as ground truth: nothing is strictly above it
        gt = torch.tensor([g_, 5, 6])
        out = ev.retrieve(user, k=K, gt_index=gt, chunk_rows=chunk_rows)
        _check(out, _reference(S, K, gt))
        assert out["topk_index"][0, :4].tolist() == list(TIED)
        assert int(out["rank"][0]) == 1
        # an all-zero user: every cosine is 0, so the list is the first K indices and every item has rank 1
        assert out["topk_index"][1].tolist() == list(range(K)) and int(out["rank"][1]) == 1
    gt = torch.tensor([1024, 5, 6])
    exclude = [[0], [0, 2], []]
    out = ev.retrieve(user, k=K, gt_index=gt, exclude=exclude, chunk_rows=chunk_rows)
    _check(out, _reference(S, K, gt, exclude))
    assert out["topk_index"][0, :3].tolist() == [1023, 1024, 2500]
    assert out["topk_index"][1].tolist() == [1] + list(range(3, K + 2))


# 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_rows", [None, 1024])
def test_exclusion(chunk_rows):
    B, N, D, K = 17, 5003, 48, 10
    user, cat, ev, S, gt0 = _case(B, N, D)
    order = np.argsort(-S, kind="stable")
    gt = gt0.clone()
    g = torch.Generator().manual_seed(11)
    exclude = [[] for _ in range(B)]
    exclude[1] = [int(order[1, 2])]                                            # one entry (the third best item)
    fifty = torch.randperm(N, generator=g)[:49].tolist()
    exclude[2] = fifty + [fifty[0]]                                            # 50 entries, one a duplicate; padded below
    gt[3] = int(order[3, 4])
    exclude[3] = [int(order[3, 0]), int(gt[3]), int(order[3, 9])]              # holds the user's own ground truth
    gt[4] = int(order[4, 5])                                                   # scored below the top-1 item ...
    exclude[4] = [int(order[4, 0])]                                            # ... which is excluded
    for b in range(5, B):                                                      # the rest: their best items and random ones, 0 .. 200 entries
        n_rand = int(torch.randint(0, 200, (1,), generator=g))
        exclude[b] = order[b, :b].tolist() + torch.randint(0, N, (n_rand,), generator=g).tolist()
    exclude[16] = exclude[16] + [N, N + 7, 2 ** 40]                            # indices the catalogue does not have match nothing
    packed = pack_exclude(exclude)
    assert packed.shape[1] >= 50 and bool((packed[2] < 0).any()) and packed[0].max() < 0

    plain = ev.retrieve(user, k=K, gt_index=gt, chunk_rows=chunk_rows)
    out = ev.retrieve(user, k=K, gt_index=gt, exclude=exclude, chunk_rows=chunk_rows)
    _check(out, _reference(S, K, gt, exclude))
    _check(plain, _reference(S, K, gt))
    # the same through the padded-tensor form, in any column order
    shuffled = packed[:, torch.randperm(packed.shape[1], generator=g)]
    _check(ev.retrieve(user, k=K, gt_index=gt, exclude=shuffled.to(DEV), chunk_rows=chunk_rows), _reference(S, K, gt, exclude))

    assert torch.equal(out["topk_index"][0], plain["topk_index"][0]) and int(out["rank"][0]) == int(plain["rank"][0])
    assert exclude[1][0] not in out["topk_index"][1].tolist() and exclude[1][0] in plain["topk_index"][1].tolist()
    # the ground truth stays although its row lists it; of the two other entries only the one above it moves the rank
    assert int(gt[3]) in out["topk_index"][3].tolist() and int(plain["rank"][3]) == 5 and int(out["rank"][3]) == 4
    # the top-1 item vanishes and the ground truth below it gains one place
    assert exclude[4][0] == int(plain["topk_index"][4, 0]) and exclude[4][0] not in out["topk_index"][4].tolist()
    assert int(plain["rank"][4]) == 6 and int(out["rank"][4]) == 5
    assert torch.equal(out["topk_index"][4, :K - 1], plain["topk_index"][4, 1:])


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_no_b_times_n_allocation():
    B, N, D, K = 64, 200_000, 16, 10
    user, cat, ev, S, gt = _case(B, N, D)
    gt_dev = gt.to(DEV)
    ev.retrieve(user, k=K, gt_index=gt_dev, chunk_rows=8192)                  # warm-up: norms cached, workspace grown
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = ev.retrieve(user, k=K, gt_index=gt_dev, chunk_rows=8192)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"[alloc] retrieve peak above the level before the call: {peak} bytes; B*N = {B * N} bytes; scores [B,N] f32 = {4 * B * N} bytes")
    assert peak < B * N, (peak, B * N)
    ws = hip.workspace(0, user.device, "catalog_select")
    assert ws.numel() < B * N, "the cached scratch (chunk [64, 8192] f32 + 64 reference scores) is no [B,N] buffer either"
    _check(out, _reference(S, K, gt))                                          # 25 chunks, the last one ragged


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_cat_inv_norm_reuse_and_norm_outputs():
    B, N, D, K = 17, 5003, 48, 10
    user, cat, ev, S, gt = _case(B, N, D)
    _, cinv_plain = hip.catalog_scores(user, cat)
    idx, val, rank, cinv = hip.catalog_select(user, cat, K, gt_index=gt)
    assert _same_bits(cinv, cinv_plain)
    idx2, val2, rank2, cinv2 = hip.catalog_select(user, cat, K, cat_inv_norm=cinv, gt_index=gt)
    assert cinv2 is cinv and torch.equal(idx2, idx) and _same_bits(val2, val) and torch.equal(rank2, rank)
    _check({"topk_index": idx, "topk_score": val, "rank": rank}, _reference(S, K, gt))
    # a caller's norms are USED, not recomputed: doubled norms double every score (a power of two: exact) and change nothing else
    idx3, val3, rank3, _ = hip.catalog_select(user, cat, K, cat_inv_norm=cinv * 2, gt_index=gt)
    assert torch.equal(idx3, idx) and _same_bits(val3, val * 2) and torch.equal(rank3, rank)

    # user_inv_norm / cat_inv_norm as the raw call writes them, plain against select mode
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    scores = torch.empty(B, N, device=DEV)
    uinv_a, cinv_a = torch.full((B,), -1.0, device=DEV), torch.full((N,), -1.0, device=DEV)
    uinv_b, cinv_b = torch.full((B,), -2.0, device=DEV), torch.full((N,), -2.0, device=DEV)
    _lib.check(lib.ur_catalog_scores(user.data_ptr(), cat.data_ptr(), scores.data_ptr(), uinv_a.data_ptr(), cinv_a.data_ptr(), 0, B, N, D,
                                     None, st), "ur_catalog_scores")
    sel = _lib.CatalogSelect()
    ti, ts = torch.empty(B, K, dtype=torch.int32, device=DEV), torch.empty(B, K, device=DEV)
    sel.K, sel.topk_index, sel.topk_score = K, ti.data_ptr(), ts.data_ptr()
    args = (user.data_ptr(), cat.data_ptr(), None, uinv_b.data_ptr(), cinv_b.data_ptr(), 0, B, N, D)
    _lib.check(lib.ur_catalog_scores(*args, ctypes.byref(sel), st), "ur_catalog_scores")
    ws = torch.empty(sel.workspace_bytes, dtype=torch.uint8, device=DEV)
    sel.workspace = ws.data_ptr()
    _lib.check(lib.ur_catalog_scores(*args, ctypes.byref(sel), st), "ur_catalog_scores")
    torch.cuda.synchronize()
    assert _same_bits(uinv_a, uinv_b) and _same_bits(cinv_a, cinv_b)
    assert torch.equal(scores.cpu(), torch.from_numpy(S)) and torch.equal(ti, idx) and _same_bits(ts, val)


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_wrapper_rejects_host_and_non_contiguous_tensors():
    user, cat, ev, S, gt = _case(5, 1000, 48)
    bad = (_lib.UniRecHipError, ValueError, TypeError)
    with pytest.raises(bad):
        hip.catalog_select(user.cpu(), cat, 10)
    with pytest.raises(bad):
        hip.catalog_select(user, cat.cpu(), 10)
    with pytest.raises(bad):
        hip.catalog_select(user.t().contiguous().t(), cat, 10)
    with pytest.raises(bad):
        hip.catalog_select(user, cat[:, ::2], 10)
    with pytest.raises(bad):
        hip.catalog_select(user, cat, 10, exclude=torch.zeros(5, 4, dtype=torch.int64))            # a host tensor
    with pytest.raises(bad):
        hip.catalog_select(user, cat, 10, exclude=torch.zeros(5, 4, dtype=torch.int32, device=DEV))
    for kw in (dict(K=0), dict(K=129), dict(K=10, chunk_rows=1000)):                               # the library's own checks
        with pytest.raises(_lib.UniRecHipError) as e:
            hip.catalog_select(user, cat, **kw)
        assert "rc=-" in str(e.value) and "ur_catalog_scores" in str(e.value)

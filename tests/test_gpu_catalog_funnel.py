"""GPU: the funnel retrieval family (include/unirec_hip_funnel.h) -- prefixes of the resident [N,D] catalogue read in place.

Every reference is code that existed before this family, run on contiguous copies of the prefix: the norms hip.catalog_coarse_select /
hip.catalog_select write for cat[:, :d].contiguous(), hip.catalog_coarse_deep_select and hip.catalog_deep_rerank on the copies.  All
comparisons are on bits (torch.equal): the contract is equality, not a tolerance.  In every case the catalogue's components past the
prefix are random and of full size -- what a kernel reads past `dim` shows in the scores.

End to end.  retrieve_funnel equals the hand composition of the three hip calls tensor for tensor, and on a catalogue with a decaying
spectrum it returns retrieve(k)'s lists and score bits for every user whom a float64 reference separates: every item of the float64
top-k at dims[-1] clears the stage's (S_i + 1)-th float64 score by 2^-7 at stage 0 (the coarse error) and by 2^-16 at the re-rank
stages (far above the exact scorer's f32 error)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import catalog_coarse_ref as cref  # noqa: E402
from tests.test_gpu_catalog_coarse import _bits, _case, _rerank_case, _same  # noqa: E402
from unirec_amd import _lib, hip  # noqa: E402
from unirec_amd.evaluation import CatalogEvaluator  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16

COVERS = {
    "ur_catalog_prefix_norms": ["test_prefix_norms_equal_the_norms_of_the_contiguous_slices"],
    "ur_catalog_funnel_select": ["test_funnel_select_equals_coarse_deep_select_on_the_contiguous_copies",
                                 "test_a_spike_behind_the_prefix_does_not_move_a_score"],
    "ur_catalog_funnel_rerank": ["test_funnel_rerank_equals_deep_rerank_on_the_contiguous_slices"],
}


# ---- the norms ------------------------------------------------------------------------------------------------------------------------
def _old_norms(cat, d):
    """the inverse norms an older entry point writes for the contiguous slice cat[:, :d]"""
    piece = cat[:, :d].contiguous()
    user = torch.ones(1, d, device=DEV)
    if cat.dtype == BF16:
        return hip.catalog_coarse_select(user, piece, 1)[3]
    return hip.catalog_select(user, piece, 1)[3]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("D,dims", [(16, (8,)), (264, (8, 40, 264)), (1024, (64, 256, 1024)), (2048, (1032, 2048)), (2048, (64, 256, 1024)),
                                    (72, (8, 16, 24, 32, 40, 48, 56, 64))])
def test_prefix_norms_equal_the_norms_of_the_contiguous_slices(D, dims, dtype):
    N = 1027
    g = torch.Generator().manual_seed(D + len(dims))
    cat = torch.randn(N, D, generator=g)
    cat[3, :dims[0]] = 0.0                       # a row whose narrowest prefix is all zero: the 1e-12 clamp
    cat[5] = 0.0                                 # and one that is zero throughout
    cat = cat.to(dtype).to(DEV)
    inv = hip.catalog_prefix_norms(cat, dims)
    assert inv.shape == (len(dims), N) and inv.dtype == F32
    for l, d in enumerate(dims):
        assert torch.equal(_bits(inv[l]), _bits(_old_norms(cat, d))), (D, dims, d)
    assert float(inv[0, 3]) == float(inv[-1, 5]) and 0.99e12 < float(inv[0, 3]) < 1.01e12 and bool(torch.isfinite(inv).all())
    assert torch.equal(_bits(inv), _bits(hip.catalog_prefix_norms(cat, dims)))
    if dtype == F32:                              # an f32 catalogue takes multiples of 4
        odd = tuple(sorted({4, 12, D - 4}))
        inv4 = hip.catalog_prefix_norms(cat, odd)
        for l, d in enumerate(odd):
            assert torch.equal(_bits(inv4[l]), _bits(_old_norms(cat, d))), (D, odd, d)


# ---- the select -----------------------------------------------------------------------------------------------------------------------
# (B, N, D, d, E): the smallest case; a short last K step with live data behind it (d = 40: one full step and 8 of 32 elements); B just
# past and exactly a 64-user group; one past 128 users; the four-chain rule (d > 1024) with a short step; d = D
SHAPES = [(1, 1, 16, 8, 0), (17, 17, 72, 40, 0), (63, 1025, 264, 40, 1), (65, 5003, 264, 64, 9), (64, 2049, 1024, 256, 0),
          (129, 1500, 1024, 512, 1), (33, 1500, 2048, 1032, 9), (31, 2049, 2048, 2048, 1)]
KS = (1, 129, 1024)


def _all_equal(got, want, what):
    assert torch.equal(got[0], want[0]), (what, "indices")
    assert torch.equal(_bits(got[1]), _bits(want[1])), (what, "score bits")
    assert (got[2] is None and want[2] is None) or torch.equal(got[2], want[2]), (what, "rank")
    assert torch.equal(_bits(got[3]), _bits(want[3])), (what, "norms")


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("B,N,D,d,E", SHAPES)
def test_funnel_select_equals_coarse_deep_select_on_the_contiguous_copies(B, N, D, d, E, K):
    c = _case(B, N, D, E)
    user, cat = c["user"], c["cat"]
    u_d, cat_d = user[:, :d].contiguous(), cat[:, :d].contiguous()
    if d < D:
        assert float(cat[:, d:].float().abs().min()) > 0.0, "the components behind the prefix are live"
    for with_gt in (True, False):
        gt = c["gt"] if with_gt else None
        want = hip.catalog_coarse_deep_select(u_d, cat_d, K, gt_index=gt, exclude=c["packed"])
        cinv = want[3]
        for chunk_rows in (None, 1024):
            for segments in (None, 1, 3):
                got = hip.catalog_funnel_select(user, cat, d, K, cat_inv_norm=cinv, gt_index=gt, exclude=c["packed"], chunk_rows=chunk_rows,
                                                segments=segments)
                assert got[0].dtype == torch.int32 and got[1].dtype == F32 and got[0].shape == (B, K) and got[3] is cinv
                _all_equal(got, want, (B, N, D, d, E, K, with_gt, chunk_rows, segments))
        # the norms not ready: the call writes the prefix's plane with the same bits; and a second call repeats every bit
        fresh = hip.catalog_funnel_select(user, cat, d, K, gt_index=gt, exclude=c["packed"])
        _all_equal(fresh, want, (B, N, D, d, E, K, with_gt, "norms not ready"))
        again = hip.catalog_funnel_select(user, cat, d, K, gt_index=gt, exclude=c["packed"])
        assert _same(fresh, again) and torch.equal(_bits(fresh[3]), _bits(again[3]))
        if d == D:                                # the same call on the same, uncopied tensors
            _all_equal(fresh, hip.catalog_coarse_deep_select(user, cat, K, gt_index=gt, exclude=c["packed"]), "d == D")


@pytest.mark.parametrize("B,N,D,d", [(17, 17, 72, 40), (63, 1025, 264, 40), (33, 1500, 2048, 1032)])
def test_a_spike_behind_the_prefix_does_not_move_a_score(B, N, D, d):
    """1e30 in column d of every catalogue row and of every user: the K step that ends short is masked by dim, so no score, list entry,
    rank or norm moves by a bit"""
    c = _case(B, N, D, 0)
    user, cat = c["user"].clone(), c["cat"].clone()
    plain = hip.catalog_funnel_select(user, cat, d, 129, gt_index=c["gt"])
    cat[:, d] = 1e30
    user[:, d] = 1e30
    assert bool(torch.isfinite(cat[:, d].float()).all()) and float(cat[0, d]) > 1e29
    spiked = hip.catalog_funnel_select(user, cat, d, 129, gt_index=c["gt"])
    _all_equal(spiked, plain, "spike")
    _all_equal(spiked, hip.catalog_coarse_deep_select(user[:, :d].contiguous(), cat[:, :d].contiguous(), 129, gt_index=c["gt"]), "spike, copies")
    # an infinity there as well: it is not an input of the call (a product with the staged zero padding would be a NaN)
    cat[:, d] = float("inf")
    user[:, d] = float("inf")
    _all_equal(hip.catalog_funnel_select(user, cat, d, 129, gt_index=c["gt"]), plain, "infinity behind the prefix")
    short = hip.catalog_funnel_select(user, cat, d, 129, gt_index=c["gt"])[0]
    idx, val, _ = hip.catalog_funnel_rerank(user, cat, short, d, 10)
    want = hip.catalog_deep_rerank(user[:, :d].contiguous(), cat[:, :d].contiguous(), short, 10)
    assert torch.equal(idx, want[0]) and torch.equal(_bits(val), _bits(want[1]))
    assert bool(torch.isfinite(val[:, 0]).all())


# ---- the re-rank ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("K_in", [1, 128, 129, 1000])
@pytest.mark.parametrize("B,N,D", [(5, 300, 264), (3, 2049, 1024)])
def test_funnel_rerank_equals_deep_rerank_on_the_contiguous_slices(B, N, D, K_in, dtype):
    """_rerank_case: random indices (duplicated, K_in = 1000 of 300 rows certainly), empty slots (-1) and indices past N"""
    user, cat, index = _rerank_case(B, N, D, K_in, dtype)
    widths = (8, 40, 256, D) + ((12,) if dtype == F32 else ())
    for d in widths:
        u_d, cat_d = user[:, :d].contiguous(), cat[:, :d].contiguous()
        for k in sorted({K_in, max(1, K_in - 1), max(1, K_in // 3)}):
            want = hip.catalog_deep_rerank(u_d, cat_d, index, k)
            got = hip.catalog_funnel_rerank(user, cat, index, d, k)
            assert got[0].shape == (B, k) and got[0].dtype == torch.int32 and got[1].dtype == F32
            assert torch.equal(got[0], want[0]) and torch.equal(_bits(got[1]), _bits(want[1])), (d, k)
            assert torch.equal(_bits(got[2]), _bits(want[2])), (d, k, "norms")
            again = hip.catalog_funnel_rerank(user, cat, index, d, k, cat_inv_norm=want[2])
            assert again[2] is want[2] and torch.equal(again[0], got[0]) and torch.equal(_bits(again[1]), _bits(got[1]))
        if d == D:                                # that call's bits on the same buffers
            same = hip.catalog_deep_rerank(user, cat, index)
            got = hip.catalog_funnel_rerank(user, cat, index, D)
            assert torch.equal(got[0], same[0]) and torch.equal(_bits(got[1]), _bits(same[1])) and torch.equal(_bits(got[2]), _bits(same[2]))


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _decaying_case(B, N, D, dims):
    """standard normal rows, the components in [dims[i-1], dims[i]) scaled by 2^(-3 i), rounded to bf16; user b = row gt_b + 0.5 x noise
    of the same scaling.  Returns (user f32 [B,D], cat bf16 [N,D], gt, {d: float64 cosines [B,N] of the first d components})"""
    g = torch.Generator().manual_seed(B + N + D + sum(dims))
    scale = torch.ones(D)
    for i in range(1, len(dims)):
        scale[dims[i - 1]:dims[i]] = 2.0 ** (-3 * i)
    cat = (torch.randn(N, D, generator=g) * scale).to(BF16)
    gt = torch.randint(0, N, (B,), generator=g)
    user = cat[gt].float() + 0.5 * torch.randn(B, D, generator=g) * scale
    s64 = {d: cref.exact_scores(user[:, :d].contiguous(), cat[:, :d].contiguous()).numpy() for d in dims}
    return user, cat, gt, s64


def _separated(s64, dims, k, shortlists):
    """bool [B]: every item of the float64 top-k at dims[-1] clears the (S_i + 1)-th float64 score of stage i by the stage's margin"""
    final = s64[dims[-1]]
    topk = np.argsort(-final, axis=1, kind="stable")[:, :k]
    ok = np.ones(final.shape[0], dtype=bool)
    for i, S in enumerate(shortlists):
        s = s64[dims[i]]
        if S >= s.shape[1]:
            continue
        edge = -np.sort(-s, axis=1)[:, S]
        margin = 2.0 ** -7 if i == 0 else 2.0 ** -16
        ok &= (np.take_along_axis(s, topk, axis=1) - edge[:, None] > margin).all(axis=1)
    return ok


@pytest.mark.parametrize("B,N,D,dims,k,shortlists", [(65, 5003, 264, (64, 264), 10, (128,)), (65, 5003, 264, (64, 128, 264), 10, (512, 128)),
                                                     (33, 3000, 1024, (64, 256, 1024), 10, (1024, 128)), (64, 5003, 264, (64, 264), 100, (300,))])
def test_retrieve_funnel_equals_the_hand_composition_and_the_exact_retrieve(B, N, D, dims, k, shortlists):
    user, cat, gt, s64 = _decaying_case(B, N, D, dims)
    ev = CatalogEvaluator(cat, device=DEV, dtype=BF16)
    out = ev.retrieve_funnel(user, k=k, dims=dims, shortlists=shortlists, gt_index=gt, ks=(1, k))
    # the hand composition of the three calls, tensor for tensor
    u = user.to(DEV)
    inv = hip.catalog_prefix_norms(ev.catalog, dims)
    idx, _, rank, _ = hip.catalog_funnel_select(u, ev.catalog, dims[0], shortlists[0], inv[0], gt_index=gt)
    for i in range(1, len(dims)):
        idx, val, _ = hip.catalog_funnel_rerank(u, ev.catalog, idx, dims[i], (shortlists[1:] + (k,))[i - 1], inv[i])
    assert torch.equal(out["topk_index"], idx) and torch.equal(_bits(out["topk_score"]), _bits(val)) and torch.equal(out["rank"], rank)
    assert out["rank_is_coarse"] is True and out["rank_dim"] == dims[0] and out["topk_index"].shape == (B, k)
    assert 0.0 < out["mrr"] <= 1.0 and set(out["hit_at"]) == {1, k} and set(out["ndcg_at"]) == {1, k}
    assert sorted(ev._prefix_inv) == sorted(d for d in dims if d != D) and torch.equal(_bits(ev._inv), _bits(inv[-1]))
    for i, d in enumerate(dims[:-1]):
        assert torch.equal(_bits(ev._prefix_inv[d]), _bits(inv[i]))
    # a second call asks for no norms and repeats every bit; without gt_index there is no rank
    planes = {d: p.data_ptr() for d, p in ev._prefix_inv.items()}
    again = ev.retrieve_funnel(user, k=k, dims=dims, shortlists=shortlists, chunk_rows=1024)
    assert sorted(again) == ["topk_index", "topk_score"] and {d: p.data_ptr() for d, p in ev._prefix_inv.items()} == planes
    assert torch.equal(again["topk_index"], out["topk_index"]) and torch.equal(_bits(again["topk_score"]), _bits(out["topk_score"]))
    # against the exact retrieve(k), on the users the float64 reference separates
    sep = _separated(s64, dims, k, shortlists)
    print(f"\nfunnel B {B} N {N} D {D} dims {dims} k {k} shortlists {shortlists}: separated {int(sep.sum())} of {B}")
    assert sep.mean() >= 0.75, (int(sep.sum()), B)
    exact = ev.retrieve(user, k=k)
    rows = torch.from_numpy(np.nonzero(sep)[0]).to(DEV)
    assert torch.equal(out["topk_index"][rows], exact["topk_index"][rows])
    assert torch.equal(_bits(out["topk_score"][rows]), _bits(exact["topk_score"][rows]))
    # the older paths on the same evaluator are untouched by the planes the funnel keeps
    two = ev.retrieve_two_stage(user, k=k, shortlist=shortlists[0])
    assert torch.equal(two["topk_index"][rows], exact["topk_index"][rows])


# ---- refusals through the wrappers ----------------------------------------------------------------------------------------------------
def test_wrappers_refuse_by_entry_point_and_field():
    c = _case(15, 1023, 24, 1)
    user, cat = c["user"], c["cat"]
    index = torch.zeros(15, 300, dtype=torch.int32, device=DEV)
    sel, rer, norms = hip.catalog_funnel_select, hip.catalog_funnel_rerank, hip.catalog_prefix_norms
    with pytest.raises(_lib.UniRecHipError, match="catalog_funnel_select: user.*no CPU fallback"):
        sel(user.cpu(), cat, 8, 10)
    with pytest.raises(ValueError, match="catalog_funnel_select.*bf16 catalogue"):
        sel(user, cat.float(), 8, 10)
    with pytest.raises(ValueError, match="catalog_funnel_select.*prefix dim = 32"):
        sel(user, cat, 32, 10)
    with pytest.raises(_lib.UniRecHipError, match="ur_catalog_funnel_select: dim must be"):
        sel(user, cat, 12, 10)
    for K in (0, 1025):
        with pytest.raises(_lib.UniRecHipError, match="ur_catalog_funnel_select: K must be"):
            sel(user, cat, 8, K)
    with pytest.raises(_lib.UniRecHipError, match="ur_catalog_funnel_select: chunk_rows"):
        sel(user, cat, 8, 300, chunk_rows=1000)
    with pytest.raises(_lib.UniRecHipError, match="ur_catalog_funnel_select: segments"):
        sel(user, cat, 8, 300, segments=17)
    with pytest.raises(_lib.UniRecHipError, match="ur_catalog_funnel_rerank: K_in must be"):
        rer(user, cat, torch.zeros(15, 1025, dtype=torch.int32, device=DEV), 8)
    for k in (301, 0):
        with pytest.raises(_lib.UniRecHipError, match="ur_catalog_funnel_rerank: k must be"):
            rer(user, cat, index, 8, k)
    with pytest.raises(_lib.UniRecHipError, match="ur_catalog_funnel_rerank: dim must be"):
        rer(user, cat, index, 12)                                   # a bf16 catalogue takes multiples of 8
    with pytest.raises(ValueError, match=r"catalog_funnel_rerank: index must be \[15, K'\]"):
        rer(user, cat, index[:7].contiguous(), 8)
    with pytest.raises(ValueError, match="multiple of 8 for a bf16 catalogue"):
        norms(cat, (4, 8))
    with pytest.raises(ValueError, match="strictly ascending"):
        norms(cat, (16, 8))
    with pytest.raises(ValueError, match="at most the catalogue width 24"):
        norms(cat, (8, 32))
    assert norms(cat.float(), (4, 8)).shape == (2, 1023)

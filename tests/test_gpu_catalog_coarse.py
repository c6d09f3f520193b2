"""GPU: the two-stage retrieval family (include/unirec_hip_coarse.h) against the float64 restatement tests/catalog_coarse_ref.py.

Coarse scores.  Every returned coarse score is held to s64 = the float64 cosine of the bf16-rounded user with the row, within

    e = max(4 x yardstick, 8 f32 ulps of the largest |s64| of the case)

where the yardstick is the worst error, against the same s64, of the existing hip.catalog_select(u~.float(), catalog, scorer="vector")
on the same case: the exact scorer computes the same mathematical quantity by another, equally long f32 summation of the same exact
products, so its own error is the measure of what an f32 sum of this length costs (the project's usual margin of 4).  Run with -s for
the measured / yardstick / bound table.

Lists.  Random catalogues are not separated enough for index equality at K' = 128, so a list is held to a band: sorted on its own
bits, no duplicate, nothing excluded, nothing out of range; every kept item NOT returned has s64 <= (the list's last score) + e; every
returned item has s64 >= tau - 2 e, tau the K'-th largest s64 of the kept items.  So that the band cannot hide a dropped item the test
first asserts, on the reference alone, that at least 90 % of the users have no other item within 2 e of tau.  The rank lies between
1 + #{s64 > ref64 + 2 e} and 1 + #{s64 >= ref64 - 2 e} over the kept n != g, and for at least 90 % of the users the two ends agree.

Exact properties (torch.equal): repeatability, chunk_rows, the position of a user in the batch, a catalogue of identical rows, everything
but the ground truth excluded.  Re-rank: the score bits of hip.catalog_scores on the same pairs and the total order on those bits.
End to end: retrieve(k, shortlist) equals retrieve(k) where the float64 reference separates the k-th from the (shortlist + 1)-th score
by more than 2^-7, twice the worst change of a cosine under bf16 rounding of one side."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import catalog_coarse_ref as cref  # noqa: E402
from tests import ref64  # noqa: E402
from unirec_amd import hip  # noqa: E402
from unirec_amd.evaluation import CatalogEvaluator, pack_exclude  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16

COVERS = {
    "ur_catalog_coarse_select": ["test_coarse_select_against_float64"],
    "ur_catalog_rerank": ["test_rerank_against_float64_and_the_exact_scorer_bits"],
}


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    """the same lists, score bits and ranks"""
    return torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1])) and \
        ((a[2] is None and b[2] is None) or torch.equal(a[2], b[2]))


def _exclude_rows(B, N, E, gt, g):
    """[B,E] int64: random seen items, a few empty slots, and in some rows the user's own ground truth (which must stay)"""
    if E == 0:
        return None
    ex = torch.randint(0, N, (B, E), generator=g)
    ex[::3, 0] = -1
    ex[1::2, E - 1] = gt[1::2]
    return ex


@functools.lru_cache(maxsize=None)
def _case(B, N, D, E=0, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + B + 3 * N + 7 * D + 11 * E)
    user = torch.randn(B, D, generator=g)
    cat = torch.randn(N, D, generator=g).to(BF16)
    gt = torch.randint(0, N, (B,), generator=g)
    ex = _exclude_rows(B, N, E, gt, g)
    s64 = cref.coarse_scores(user, cat).numpy()
    packed = None if ex is None else pack_exclude(ex, B).to(DEV)
    return dict(B=B, N=N, D=D, user=user.to(DEV), cat=cat.to(DEV), gt=gt, ex=ex, packed=packed, s64=s64,
                keep=cref.keep_mask(B, N, gt.numpy(), None if ex is None else ex.numpy()))


def _gathered_error(idx, val, s64):
    """worst |val - s64[b, idx]| over the filled slots of lists idx / val [B,K]"""
    idx, val = idx.cpu().numpy(), val.cpu().numpy().astype(np.float64)
    worst = 0.0
    for b in range(idx.shape[0]):
        m = idx[b] >= 0
        if m.any():
            worst = max(worst, float(np.abs(val[b, m] - s64[b, idx[b, m]]).max()))
    return worst


def _bound(c, K, exclude="case"):
    """(e, yardstick): the existing vector scorer on the rounded users, same case, same exclusion, same reference"""
    ub = c["user"].to(BF16).float()
    exclude = c["packed"] if isinstance(exclude, str) else exclude
    yi, yv, _, _ = hip.catalog_select(ub, c["cat"], K, gt_index=c["gt"], exclude=exclude, scorer="vector")
    yard = _gathered_error(yi, yv, c["s64"])
    floor = 8.0 * float(ref64.f32_ulp(float(np.abs(c["s64"]).max())))
    return max(4.0 * yard, floor), yard


def _hold_band(c, K, idx, val, rank, e, what=""):
    """the band test of the module docstring on lists idx / val [B,K] and on rank"""
    B, N, s64, keep, gt = c["B"], c["N"], c["s64"], c["keep"], c["gt"].numpy()
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    clear = clear_rank = 0
    for b in range(B):
        kept = np.nonzero(keep[b])[0]
        n_fill = min(K, len(kept))
        row, sc = idx[b], val[b]
        assert (row[:n_fill] >= 0).all() and (row[:n_fill] < N).all() and (row[n_fill:] == -1).all(), (what, b, row)
        assert np.isneginf(sc[n_fill:]).all()
        assert len(set(row[:n_fill].tolist())) == n_fill, (what, b, "duplicate")
        assert keep[b, row[:n_fill]].all(), (what, b, "an excluded item was returned")
        o = cref.order(sc[:n_fill], row[:n_fill])
        assert (o == np.arange(n_fill)).all(), (what, b, "not sorted under the total order on its own bits")
        if len(kept) > K:
            top = np.sort(s64[b, kept])[::-1]
            tau = top[K - 1]
            clear += int((np.abs(s64[b, kept] - tau) <= 2 * e).sum() == 1)
            rest = np.setdiff1d(kept, row)
            assert (s64[b, rest] <= float(sc[K - 1]) + e).all(), (what, b, "a better item was left out")
            assert (s64[b, row] >= tau - 2 * e).all(), (what, b, "a returned item lies below the band")
        else:
            clear += 1
            assert sorted(row[:n_fill].tolist()) == kept.tolist()
        if rank is not None:
            others = kept[kept != gt[b]]
            lo = 1 + int((s64[b, others] > s64[b, gt[b]] + 2 * e).sum())
            hi = 1 + int((s64[b, others] >= s64[b, gt[b]] - 2 * e).sum())
            clear_rank += int(lo == hi)
            assert lo <= int(rank[b]) <= hi, (what, b, lo, int(rank[b]), hi)
    assert clear >= 0.9 * B, f"{what}: precondition: only {clear} of {B} users have tau alone in its 2e band; change the seed"
    if rank is not None:
        assert clear_rank >= 0.9 * B, f"{what}: precondition: only {clear_rank} of {B} users have a single-valued rank band; change the seed"


# (B, N, D, K', E): B around the user group (64; 32 for D > 1024) and 1 / 15 / 17 / 33; N below K', around the 1024-row selection tile and
# the 256-row workgroup step, several chunks at chunk_rows = 1024; D: one K step that ends short (8, 24), full steps plus a short one (40,
# 264), full steps only (1024, 2048: the 32-user form).  The last entry is the seed: 0 unless the reference-only precondition of the band
# test (which depends on nothing but the seed and e) left less than 5 % of room at e = 4e-7
SHAPES = [
    (1, 1, 8, 1, 0, 0), (15, 15, 24, 10, 1, 0), (17, 17, 40, 128, 0, 0), (33, 1023, 264, 10, 9, 0), (63, 1025, 40, 128, 1, 0),
    (64, 2049, 1024, 10, 0, 0), (65, 5003, 264, 128, 9, 0), (17, 5003, 1024, 128, 0, 4), (1, 5003, 8, 1, 9, 0), (15, 2049, 24, 128, 0, 0),
    (31, 2049, 2048, 10, 1, 0), (32, 1025, 2048, 128, 0, 1), (33, 1023, 2048, 1, 9, 0), (17, 1, 1024, 10, 0, 0), (33, 15, 2048, 128, 1, 0),
]


@pytest.mark.parametrize("B,N,D,K,E,seed", SHAPES)
def test_coarse_select_against_float64(B, N, D, K, E, seed):
    c = _case(B, N, D, E, seed)
    got = hip.catalog_coarse_select(c["user"], c["cat"], K, gt_index=c["gt"], exclude=c["packed"])          # cat_inv_norm not ready
    idx, val, rank, cinv = got
    assert idx.dtype == torch.int32 and val.dtype == F32 and rank.dtype == torch.int32 and idx.shape == (B, K)
    e, yard = _bound(c, K)
    measured = _gathered_error(idx, val, c["s64"])
    print(f"\ncoarse B {B:3d} N {N:5d} D {D:5d} K' {K:4d} E {E}: measured {measured:.3e}  yardstick {yard:.3e}  bound {e:.3e}  "
          f"ratio {measured / e:.3f}")
    assert measured <= e, (measured, yard, e)
    _hold_band(c, K, idx, val, rank.cpu().numpy(), e, what=f"B{B} N{N} D{D} K{K} E{E}")
    # the catalogue norms are the exact scorer's for a bf16 catalogue, bit for bit
    want_cinv = hip.catalog_select(c["user"], c["cat"], 1, scorer="vector")[3]
    assert torch.equal(_bits(cinv), _bits(want_cinv))
    # two calls, norms ready or not: the same bits; chunk_rows = 1024 and the default: the same lists, scores and ranks
    again = hip.catalog_coarse_select(c["user"], c["cat"], K, cat_inv_norm=cinv, gt_index=c["gt"], exclude=c["packed"])
    assert again[3] is cinv and _same(got, again)
    chunked = hip.catalog_coarse_select(c["user"], c["cat"], K, cat_inv_norm=cinv, gt_index=c["gt"], exclude=c["packed"], chunk_rows=1024)
    assert _same(got, chunked)
    # without a ground truth: no rank; the same lists, unless an exclusion row held the ground truth (then that item leaves as well)
    lists = hip.catalog_coarse_select(c["user"], c["cat"], K, cat_inv_norm=cinv, exclude=c["packed"], chunk_rows=1024)
    assert lists[2] is None
    if E == 0:
        assert torch.equal(lists[0], idx) and torch.equal(_bits(lists[1]), _bits(val))
    else:
        assert _gathered_error(lists[0], lists[1], c["s64"]) <= e
        _hold_band(dict(c, keep=cref.keep_mask(B, N, None, c["ex"].numpy())), K, lists[0], lists[1], None, e, what="no ground truth")


@pytest.mark.parametrize("N,D,K", [(2049, 264, 10), (1025, 2048, 128)])
def test_a_user_scores_the_same_alone_and_anywhere_in_a_batch(N, D, K):
    c = _case(33, N, D, 9)
    batch = hip.catalog_coarse_select(c["user"], c["cat"], K, gt_index=c["gt"], exclude=c["packed"])
    for b in range(33):
        alone = hip.catalog_coarse_select(c["user"][b:b + 1].contiguous(), c["cat"], K, cat_inv_norm=batch[3], gt_index=c["gt"][b:b + 1],
                                          exclude=c["packed"][b:b + 1].contiguous())
        assert _same(alone, (batch[0][b:b + 1], batch[1][b:b + 1], batch[2][b:b + 1])), b
    # ... and at another position, among other users
    perm = torch.randperm(33, generator=torch.Generator().manual_seed(3))
    moved = hip.catalog_coarse_select(c["user"][perm.to(DEV)].contiguous(), c["cat"], K, cat_inv_norm=batch[3], gt_index=c["gt"][perm],
                                      exclude=c["packed"][perm.to(DEV)].contiguous())
    assert _same(moved, (batch[0][perm.to(DEV)], batch[1][perm.to(DEV)], batch[2][perm.to(DEV)]))


@pytest.mark.parametrize("D", [264, 1024, 2048])
@pytest.mark.parametrize("K", [10, 128])
def test_identical_rows_tie_to_the_lowest_indices_and_rank_one(D, K):
    """2049 copies of one row: the chain must not depend on where a row sits in a tile, a workgroup or a chunk, and the ground truth's
    reference score must have the bits a chunk holds for it"""
    g = torch.Generator().manual_seed(D + K)
    user = torch.randn(33, D, generator=g).to(DEV)
    cat = torch.randn(1, D, generator=g).to(BF16).repeat(2049, 1).contiguous().to(DEV)
    gt = torch.randint(0, 2049, (33,), generator=g)
    for chunk_rows in (None, 1024):
        idx, val, rank, _ = hip.catalog_coarse_select(user, cat, K, gt_index=gt, chunk_rows=chunk_rows)
        assert torch.equal(idx.cpu(), torch.arange(K, dtype=torch.int32).repeat(33, 1))
        assert torch.equal(_bits(val), _bits(val[:, :1]).repeat(1, K)) and bool(torch.isfinite(val).all())
        assert torch.equal(rank.cpu(), torch.ones(33, dtype=torch.int32)), rank


@pytest.mark.parametrize("chunk_rows", [None, 1024])
def test_everything_but_the_ground_truth_excluded(chunk_rows):
    c = _case(17, 1300, 40)
    ex = torch.stack([torch.tensor([n for n in range(1300) if n != int(g)]) for g in c["gt"]]).to(DEV)
    idx, val, rank, _ = hip.catalog_coarse_select(c["user"], c["cat"], 10, gt_index=c["gt"], exclude=ex, chunk_rows=chunk_rows)
    assert torch.equal(idx[:, 0].cpu(), c["gt"].to(torch.int32)) and bool((idx[:, 1:] == -1).all())
    assert bool(torch.isneginf(val[:, 1:]).all()) and bool(torch.isfinite(val[:, 0]).all())
    assert torch.equal(rank.cpu(), torch.ones(17, dtype=torch.int32))
    e, _ = _bound(c, 10, ex)
    assert _gathered_error(idx, val, c["s64"]) <= e


# ---- the re-rank --------------------------------------------------------------------------------------------------------------------
def _rerank_case(B, N, D, K_in, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + B + N + D + K_in)
    user = torch.randn(B, D, generator=g)
    cat = torch.randn(N, D, generator=g)
    if N > 12:
        cat[5:10] = cat[4]                                           # exact ties: six copies of one row at the indices 4 .. 9
    cat = cat.to(dtype)
    index = torch.randint(0, N, (B, K_in), generator=g, dtype=torch.int32)
    if N > 12 and K_in >= 10:
        for b in range(B):
            pos = torch.randperm(K_in, generator=g)[:9]
            index[b, pos[:6]] = torch.tensor([9, 4, 7, 5, 8, 6], dtype=torch.int32)      # the tied rows, out of order
            index[b, pos[6:8]] = -1                                  # empty slots in the middle
            index[b, pos[8]] = N + b                                 # out of range: an empty slot as well
    else:
        index[0, 0] = N
    return user.to(DEV), cat.to(DEV), index.to(DEV)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,N,D,K_in", [(1, 1, 8, 1), (17, 1023, 264, 10), (33, 2049, 1024, 128), (5, 300, 2048, 128), (3, 40, 24, 128)])
def test_rerank_against_float64_and_the_exact_scorer_bits(B, N, D, K_in, dtype):
    user, cat, index = _rerank_case(B, N, D, K_in, dtype)
    S, cinv = hip.catalog_scores(user, cat.float())                  # the plain f32 call: catalog_scores_kernel, untouched
    S_host, idx_host = S.cpu().numpy(), index.cpu().numpy()
    s64 = cref.exact_scores(user, cat).numpy()
    # the f32 chain against float64: a lane's D / 64 fmafs, 6 tree levels, the two norms (the same sums) and a few multiplies, each
    # 2^-24 relative to the sum of the |products|, which Cauchy-Schwarz keeps at or below 1 after the two norms
    bound = (2 * (D / 64 + 6) + 6) * 2.0 ** -24
    for k in (K_in, 1):
        idx, val, out_cinv = hip.catalog_rerank(user, cat, index, k)
        assert idx.shape == (B, k) and idx.dtype == torch.int32 and val.dtype == F32
        assert torch.equal(_bits(out_cinv), _bits(cinv))
        idx_np, val_np = idx.cpu().numpy(), val.cpu().numpy()
        for b in range(B):
            row = idx_host[b][(idx_host[b] >= 0) & (idx_host[b] < N)]
            o = row[cref.order(S_host[b, row], row)][:k]                             # the total order on the exact scorer's bits
            assert idx_np[b, :len(o)].tolist() == o.tolist(), (b, k)
            assert (val_np[b, :len(o)].view(np.int32) == S_host[b, o].view(np.int32)).all(), (b, k, "score bits")
            assert (idx_np[b, len(o):] == -1).all() and np.isneginf(val_np[b, len(o):]).all()
            assert np.abs(val_np[b, :len(o)].astype(np.float64) - s64[b, o]).max(initial=0.0) <= bound
        # the float64 restatement gives the same lists wherever its own scores are separated by more than twice the bound
        ridx, rval = cref.rerank(s64, idx_host, k)
        gaps_ok = np.array([np.all(np.abs(np.diff(rval[b][np.isfinite(rval[b])])) > 2 * bound) for b in range(B)])
        assert (idx_np[gaps_ok] == ridx[gaps_ok]).all()
        again = hip.catalog_rerank(user, cat, index, k, cat_inv_norm=cinv)
        assert again[2] is cinv and torch.equal(again[0], idx) and torch.equal(_bits(again[1]), _bits(val))
    if N > 12 and K_in >= 10:                                        # the tied rows 4 .. 9 came out next to each other, in index order
        idx, val, _ = hip.catalog_rerank(user, cat, index)
        for b in range(B):
            row = idx[b].cpu().tolist()
            tied = sorted(n for n in row if 4 <= n <= 9)
            at = row.index(tied[0])
            assert set(tied) == {4, 5, 6, 7, 8, 9} and row[at:at + len(tied)] == tied
            assert len(set(_bits(val[b, at:at + len(tied)]).cpu().tolist())) == 1


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _retrieve_case(B, N, D):
    g = torch.Generator().manual_seed(B + N + D)
    user = torch.randn(B, D, generator=g)
    cat = torch.randn(N, D, generator=g).to(BF16)
    gt = torch.randint(0, N, (B,), generator=g)
    return user, cat, gt


@pytest.mark.parametrize("B,N,D", [(17, 5003, 264), (33, 2049, 1024)])
def test_retrieve_with_a_shortlist_equals_the_exact_retrieve(B, N, D):
    user, cat, gt = _retrieve_case(B, N, D)
    top = np.sort(cref.exact_scores(user, cat).numpy(), axis=1)[:, ::-1]
    assert ((top[:, 9] - top[:, 128]) > 2.0 ** -7).all(), "precondition: the exact 10th score clears the exact 129th by more than 2^-7"
    ev = CatalogEvaluator(cat, device=DEV, dtype=BF16)
    exact = ev.retrieve(user, k=10, gt_index=gt)
    two = ev.retrieve(user, k=10, gt_index=gt, shortlist=128)
    assert torch.equal(two["topk_index"], exact["topk_index"]) and torch.equal(_bits(two["topk_score"]), _bits(exact["topk_score"]))
    assert two["rank_is_coarse"] is True and "rank_is_coarse" not in exact
    assert two["rank"].dtype == torch.int32 and 0.0 < two["mrr"] <= 1.0 and set(two["hit_at"]) == {10}
    # the coarse rank is the rank of the shortlist pass itself
    assert torch.equal(two["rank"], hip.catalog_coarse_select(user.to(DEV), ev.catalog, 128, gt_index=gt)[2])
    chunked = ev.retrieve(user, k=10, shortlist=128, chunk_rows=1024)
    assert "rank" not in chunked and torch.equal(chunked["topk_index"], exact["topk_index"])
    # shortlist = k: still the exact scores of what is returned, in the exact order of those items
    same = ev.retrieve(user, k=10, shortlist=10)
    S = hip.catalog_scores(user.to(DEV), ev.catalog.float())[0]
    assert torch.equal(_bits(same["topk_score"]), _bits(torch.gather(S, 1, same["topk_index"].long())))
    # a truncated evaluator holds a contiguous copy: the two-stage path runs on it as on any other
    t = ev.truncated(D // 2 // 8 * 8)
    d = t.catalog.shape[1]
    t_two = t.retrieve(user[:, :d], k=10, shortlist=128)
    S_t = hip.catalog_scores(user[:, :d].contiguous().to(DEV), t.catalog.float())[0]
    assert torch.equal(_bits(t_two["topk_score"]), _bits(torch.gather(S_t, 1, t_two["topk_index"].long())))


def test_rerank_restores_the_exact_order_of_planted_near_copies():
    """twenty near-copies of user 0's best item whose exact cosines lie 1e-5 .. 2e-5 apart: rounding the user to bf16 moves some of
    them past each other (by up to 4e-5 on the reference), the re-rank puts them back"""
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
    coarse = hip.catalog_coarse_select(user.to(DEV), ev.catalog, 128)[0]
    assert coarse[0, :20].cpu().tolist() != want.tolist() and sorted(coarse[0, :20].cpu().tolist()) == sorted(want.tolist())
    two, exact = ev.retrieve(user, k=20, shortlist=128), ev.retrieve(user, k=20)
    assert two["topk_index"][0].cpu().tolist() == want.tolist()
    assert torch.equal(two["topk_index"][0], exact["topk_index"][0]) and torch.equal(_bits(two["topk_score"][0]), _bits(exact["topk_score"][0]))


# ---- mining -------------------------------------------------------------------------------------------------------------------------
def test_coarse_mining_is_valid_under_the_band():
    from unirec_amd.negatives import CatalogCandidates
    c = _case(17, 5003, 264, 9, 3)
    hard_skip, num_hard = 3, 12
    K = hard_skip + num_hard
    cc = CatalogCandidates(CatalogEvaluator(c["cat"], device=DEV, dtype=BF16), num_hard=num_hard, hard_skip=hard_skip, coarse=True)
    mined = cc.mine(c["user"], c["gt"], c["ex"])
    assert mined.shape == (17, num_hard) and mined.dtype == torch.int64
    idx, val, _, _ = hip.catalog_coarse_select(c["user"], c["cat"], K, gt_index=c["gt"], exclude=c["packed"])
    e, _ = _bound(c, K)
    _hold_band(c, K, idx, val, None, e, what="mining")               # the whole coarse list is valid under the band ...
    tail = idx[:, hard_skip:].to(torch.int64).cpu()                   # ... and the mined set is its ranks hard_skip + 1 .., the positive masked
    assert torch.equal(mined.cpu(), torch.where(tail == c["gt"][:, None], torch.full_like(tail, -1), tail))
    for b in range(17):
        row = [n for n in mined[b].cpu().tolist() if n >= 0]
        assert len(row) >= num_hard - 1 and len(set(row)) == len(row) and int(c["gt"][b]) not in row and c["keep"][b, row].all()
    # not the exact miner's path: that one still runs, untouched, and agrees wherever the band is clear
    plain = CatalogCandidates(cc.evaluator, num_hard=num_hard, hard_skip=hard_skip).mine(c["user"], c["gt"], c["ex"])
    assert plain.shape == mined.shape


def test_candidates_with_coarse_mining_run_a_joint_step():
    import types
    from tests.test_gpu_grad_clip import _inputs, _joint
    from tests.test_gpu_negatives import _catalogue, _index_batch
    from unirec_amd.joint import JointTrainer
    from unirec_amd.negatives import CatalogCandidates
    case, model = _joint()
    batch = _inputs(case)
    cat, pos_index, neg_index = _catalogue(batch, BF16, extra=200)
    assert cat.shape[1] % 8 == 0
    B, Pe = neg_index.shape
    seen = [[int(pos_index[0]), 3, 30]] + [[] for _ in range(B - 1)]
    cc = CatalogCandidates(cat, num_random=8, num_hard=4, hard_skip=1, seed=3, coarse=True)
    args = types.SimpleNamespace(learning_rate=1e-3, warmup_steps=0, max_steps=4, max_grad_norm=1.0, weight_decay=0.01, logging_steps=0)
    tr = JointTrainer(model, args, negatives=cc)
    before = [p.master.clone() for p in tr.packs]
    loss = tr.training_step(_index_batch(batch, pos_index, neg_index, seen_item_index=seen))
    assert torch.isfinite(loss) and any(not torch.equal(p.master, b) for p, b in zip(tr.packs, before)), "the step moves the weights"
    index, mask = cc.last_index, cc.last_mask
    assert index.shape == (B, Pe + 8 + 4)
    mined = index[:, Pe + 8:]
    assert bool((mask[:, Pe + 8:] == (mined >= 0).to(torch.uint8)).all()) and bool((mined >= 0).any())
    for b in range(B):
        row = [n for n in mined[b].cpu().tolist() if n >= 0]
        assert len(set(row)) == len(row) and int(pos_index[b]) not in row and not set(row) & set(seen[b])

"""GPU: catalogue rows past 2^32 bytes and 2^31 elements.  The ABI takes N up to INT32_MAX, the benchmarked shape (1 M x 1024 f32) ends five
per cent below 2^32 bytes, and no other test touches a row whose offset does not fit 32 bits.  This is an ADDRESSING test: a wrong row
gives a cosine of 0.02 where 0.9 is expected, so nothing here needs a new tolerance.

The catalogue: ONE bf16 tensor of N = 2^20 + 1025 = 1 049 601 rows, D = 2048 -- 4.30e9 bytes, 2.15e9 elements; every row with index
>= 2^20 lies beyond both limits.  Built once per module on the device (torch.randn in bf16) and freed at the end.  The f32
instantiations share the templated index arithmetic and get no 8.6 GB catalogue of their own; the one f32-only entry point, the plain
ur_catalog_scores, reads THE SAME MEMORY as an f32 catalogue [N, 1024] (two bf16 elements per f32: finite, ordinary values), whose rows
>= 2^20 start at or past 2^32 bytes.

Three users; twelve planted rows dealt round-robin, planted row j = bf16(a_j u_b + sqrt(1 - a_j^2) noise), b = j mod 3, a_j = 0.95 -
0.03 j.  The noise is made orthogonal to u_b and as long as u_b, separately on the components [0, 256) and [256, 2048), so the float64
cosine is a_j at full width AND on the 256-wide prefix the funnel reads, up to the bf16 rounding of the row.  The indices: 0, 1023, 1024,
2^20 - 1, 2^20, 2^20 + 1, 2^20 + 1023 = N - 2, 2^20 + 1024 = N - 1 (at this N the last two of the issue's list coincide with the two
before them) and four more past 2^20: 2^20 + 31, + 512, + 513, + 1000.  chunk_rows = 65536 puts a chunk start exactly on 2^20; the
default makes one chunk of the whole catalogue.

Preconditions, asserted on references alone (not measurements of the code under test): the float64 cosines of the planted rows with
their users (host, 12 rows) are pairwise >= 2^-6 apart and each user's lowest is >= 0.5, at full width and on the prefix; the largest
cosine of any user with a non-planted row, by torch's own matmul on the device in chunks of 65 536 rows, is below 0.25 (about 5.3 /
sqrt(2048) = 0.12 is expected) -- on the 256-wide prefix below 0.45 (5.3 / sqrt(256) = 0.33; the lowest planted cosine is 0.62).  The
CPU test below checks the full-width figure on a stand-in of 3 x 100 000 random rows.

Assertions: the first four entries of every user's list are its planted rows in a-order (select, deep, coarse, coarse-deep, funnel;
K = 4, and 129 where the entry point takes it); with gt_index a planted row the rank is 1 + the user's planted rows above it; the exact
scorers return, for planted rows, the bits of hip.catalog_scores(user, the 12 rows copied out) (the window test of
test_gpu_catalog_scorer establishes that a row's place does not change its bits); the plain call's planted columns and its columns
2^20 - 2048 .. N (the catalogue ends before 2^20 + 2048) have the bits of the call on compact copies; prefix norms and the three re-ranks on rows >= 2^20 equal the
same call on a compact copy of the last 2049 rows with remapped indices; coarse scores at planted rows are within 2^-7 of float64 (the
figure tests/test_gpu_catalog_coarse.py gives for bf16 rounding of one side; loose on purpose).

Out of scope: ur_catalog_softmax and ur_catalog_mrl_softmax at this size.  No yardstick for their bounds exists at a million candidates
without an 8.6 GB f32 copy.  Their scoring launches take `catalog + c0 * D` and `cat_inv_norm + c0` exactly as select mode does (the same
catalog_score_chunk / launch functions), and their gradient kernel reads `cp + (long)n * cld`, 64-bit.

Offset expressions of the family and their types are tabled in docs/lab_notes.md; none is 32-bit."""
import pytest
import torch

from unirec_amd import hip

gpu = pytest.mark.gpu

COVERS = {
    "ur_catalog_scores": ["test_plain_scores_past_4gib", "test_exact_selects_past_4gib"],
    "ur_catalog_deep_select": ["test_exact_selects_past_4gib"],
    "ur_catalog_coarse_select": ["test_coarse_selects_past_4gib"],
    "ur_catalog_coarse_deep_select": ["test_coarse_selects_past_4gib"],
    "ur_catalog_funnel_select": ["test_coarse_selects_past_4gib"],
    "ur_catalog_prefix_norms": ["test_prefix_norms_past_4gib"],
    "ur_catalog_rerank": ["test_reranks_past_4gib"],
    "ur_catalog_deep_rerank": ["test_reranks_past_4gib"],
    "ur_catalog_funnel_rerank": ["test_reranks_past_4gib"],
}

DEV = "cuda"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
M = 1 << 20
N, D, B, PREFIX = M + 1025, 2048, 3, 256
PLANTED = (0, 1023, 1024, M - 1, M, M + 1, M + 1023, M + 1024, M + 31, M + 512, M + 513, M + 1000)
ALPHA = tuple(0.95 - 0.03 * j for j in range(len(PLANTED)))
CHUNKS = (65536, None)
SEP, FLOOR, CEIL, CEIL_PREFIX = 2.0 ** -6, 0.5, 0.25, 0.45
assert N * D * 2 > 1 << 32 and N * D > 1 << 31 and M * D * 2 == 1 << 32 and len(set(PLANTED)) == 12 and max(PLANTED) == N - 1


def _users_and_planted():
    """(user f32 [3, D], rows bf16 [12, D]) on the host"""
    g = torch.Generator().manual_seed(4096)
    user = torch.randn(B, D, generator=g)
    rows = []
    for j, a in enumerate(ALPHA):
        u = user[j % B].double()
        noise = torch.randn(D, generator=g).double()
        for lo, hi in ((0, PREFIX), (PREFIX, D)):          # orthogonal to u and as long as u, on the prefix and behind it
            ub, nb = u[lo:hi], noise[lo:hi]
            nb = nb - (nb @ ub) / (ub @ ub) * ub
            noise[lo:hi] = nb * ub.norm() / nb.norm()
        rows.append((a * u + (1.0 - a * a) ** 0.5 * noise).to(F32).to(BF16))
    return user, torch.stack(rows)


def _cos64(user, rows, d):
    u, r = user[:, :d].double(), rows[:, :d].double()
    return (u / u.norm(dim=1, keepdim=True)) @ (r / r.norm(dim=1, keepdim=True)).T          # [3, 12]


def _mine(b):
    """the positions in PLANTED of user b's rows, best first"""
    return [j for j in range(len(PLANTED)) if j % B == b]


def _max_cosine(user, rows, d, skip=()):
    """the largest cosine of any user with any of `rows` (bf16 or f32, on the users' device) on the first d components, the rows whose
    index is in `skip` left out: torch's matmul in f32, 65 536 rows at a time"""
    uh = torch.nn.functional.normalize(user[:, :d].float(), dim=1)
    worst = -1.0
    for r0 in range(0, rows.shape[0], 65536):
        piece = rows[r0:r0 + 65536, :d].float()
        cos = torch.nn.functional.normalize(piece, dim=1) @ uh.T
        for n in skip:
            if r0 <= n < r0 + piece.shape[0]:
                cos[n - r0] = -1.0
        worst = max(worst, float(cos.max()))
    return worst


def test_random_rows_stay_far_below_the_planted_ones():
    """CPU stand-in for the device precondition: 3 x 100 000 random bf16 rows, none within 0.25 of a user"""
    user, rows = _users_and_planted()
    g = torch.Generator().manual_seed(5)
    worst = max(_max_cosine(user, torch.randn(20000, D, generator=g).to(BF16), D) for _ in range(5))
    assert worst < CEIL, worst
    for d in (D, PREFIX):                                   # and the planted rows are where the module says, on the host alone
        c = _cos64(user, rows, d)
        own = torch.tensor([float(c[j % B, j]) for j in range(len(PLANTED))])
        assert float((own - torch.tensor(ALPHA)).abs().max()) < 2.0 ** -9, (d, own)
        assert float(torch.pdist(own[:, None]).min()) >= SEP and float(own.min()) >= FLOOR


@pytest.fixture(scope="module")
def big():
    """the catalogue, the users, the compact copies and the float64 cosines; the preconditions are asserted here, once"""
    import time
    torch.cuda.synchronize()
    t0 = time.time()
    user_h, rows_h = _users_and_planted()
    cat = torch.randn(N, D, dtype=BF16, device=DEV, generator=torch.Generator(device=DEV).manual_seed(20))
    at = torch.tensor(PLANTED, device=DEV)
    cat[at] = rows_h.to(DEV)
    torch.cuda.synchronize()
    print(f"\n[4gib] catalogue {tuple(cat.shape)} bf16, {cat.numel() * 2 / 1e9:.2f} GB, built in {time.time() - t0:.2f} s")
    user = user_h.to(DEV)
    c = dict(cat=cat, user=user, user_h=user_h, rows_h=rows_h, cos={d: _cos64(user_h, rows_h, d) for d in (D, PREFIX)})
    for d, ceil in ((D, CEIL), (PREFIX, CEIL_PREFIX)):
        own = torch.tensor([float(c["cos"][d][j % B, j]) for j in range(len(PLANTED))])
        assert float(torch.pdist(own[:, None]).min()) >= SEP, (d, own)
        assert all(float(own[_mine(b)].min()) >= FLOOR for b in range(B))
        for b in range(B):                                  # ... and a user's own rows stand in a-order
            assert own[_mine(b)].tolist() == sorted(own[_mine(b)].tolist(), reverse=True)
        worst = _max_cosine(user, cat, d, skip=PLANTED)
        print(f"[4gib] largest cosine with a non-planted row on [:{d}]: {worst:.4f} (ceiling {ceil})")
        assert worst < ceil, (d, worst)
        others = max(float(c["cos"][d][b, j]) for b in range(B) for j in range(len(PLANTED)) if j % B != b)
        assert others < ceil, (d, others)                   # another user's planted rows are orthogonal to this one, up to chance
    torch.cuda.synchronize()
    print(f"[4gib] preconditions hold; fixture ready after {time.time() - t0:.2f} s")
    yield c
    del c, cat
    torch.cuda.empty_cache()


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _want_lists(b):
    return [PLANTED[j] for j in _mine(b)]


def _gt_and_rank():
    """gt_index: user b's planted row at position b + 1 of its own a-order -> rank b + 2"""
    gt = torch.tensor([_want_lists(b)[b + 1] for b in range(B)])
    return gt, torch.tensor([b + 2 for b in range(B)], dtype=torch.int32)


def _lists_hold(idx, rank, want_rank, what):
    for b in range(B):
        assert idx[b, :4].cpu().tolist() == _want_lists(b), (what, b, idx[b, :4].cpu().tolist(), _want_lists(b))
    assert torch.equal(rank.cpu(), want_rank), (what, rank.cpu(), want_rank)


@gpu
@pytest.mark.parametrize("scorer", ["vector", "mfma"])
def test_exact_selects_past_4gib(big, scorer):
    user, cat = big["user"], big["cat"]
    compact = cat[torch.tensor(PLANTED, device=DEV)].float().contiguous()
    S = hip.catalog_scores(user, compact)[0]                                   # [3, 12]: the bits every exact scorer must return
    gt, want_rank = _gt_and_rank()
    cinv = None
    for chunk_rows in CHUNKS:
        calls = [("select K 4", lambda: hip.catalog_select(user, cat, 4, cat_inv_norm=cinv, gt_index=gt, chunk_rows=chunk_rows, scorer=scorer)),
                 ("deep K 4", lambda: hip.catalog_deep_select(user, cat, 4, cat_inv_norm=cinv, gt_index=gt, chunk_rows=chunk_rows, scorer=scorer)),
                 ("deep K 129", lambda: hip.catalog_deep_select(user, cat, 129, cat_inv_norm=cinv, gt_index=gt, chunk_rows=chunk_rows,
                                                                scorer=scorer))]
        for what, call in calls:
            idx, val, rank, cinv = call()                                          # (the first call computes the norms of all N rows)
            _lists_hold(idx, rank, want_rank, (what, scorer, chunk_rows))
            for b in range(B):
                assert torch.equal(_bits(val[b, :4]), _bits(S[b, _mine(b)])), (what, scorer, chunk_rows, b, "score bits")
    # the norms of rows past 2^20 are those of the compact copy
    tail = hip.catalog_select(user, cat[M - 1024:].clone(), 1)[3]
    assert torch.equal(_bits(cinv[M - 1024:]), _bits(tail))


@gpu
def test_coarse_selects_past_4gib(big):
    user, cat, cos = big["user"], big["cat"], big["cos"]
    gt, want_rank = _gt_and_rank()
    for chunk_rows in CHUNKS:
        calls = [("coarse K 4", D, lambda: hip.catalog_coarse_select(user, cat, 4, gt_index=gt, chunk_rows=chunk_rows)),
                 ("coarse-deep K 4", D, lambda: hip.catalog_coarse_deep_select(user, cat, 4, gt_index=gt, chunk_rows=chunk_rows)),
                 ("coarse-deep K 129", D, lambda: hip.catalog_coarse_deep_select(user, cat, 129, gt_index=gt, chunk_rows=chunk_rows)),
                 ("funnel K 4", PREFIX, lambda: hip.catalog_funnel_select(user, cat, PREFIX, 4, gt_index=gt, chunk_rows=chunk_rows)),
                 ("funnel K 129", PREFIX, lambda: hip.catalog_funnel_select(user, cat, PREFIX, 129, gt_index=gt, chunk_rows=chunk_rows))]
        for what, d, call in calls:
            idx, val, rank, _ = call()
            _lists_hold(idx, rank, want_rank, (what, chunk_rows))
            for b in range(B):
                err = float((val[b, :4].double().cpu() - cos[d][b, _mine(b)]).abs().max())
                assert err <= 2.0 ** -7, (what, chunk_rows, b, err)


@gpu
def test_plain_scores_past_4gib(big):
    """the f32-only plain call on the same memory seen as f32 [N, 1024]: row n starts at byte 4096 n, rows >= 2^20 at or past 2^32"""
    catf = big["cat"].view(F32)
    assert catf.shape == (N, D // 2) and catf.data_ptr() == big["cat"].data_ptr() and bool(torch.isfinite(catf[M - 2048:]).all())
    user = big["user"][:, :D // 2].contiguous()
    S, cinv = hip.catalog_scores(user, catf)
    assert S.shape == (B, N) and bool(torch.isfinite(S).all())
    at = torch.tensor(PLANTED, device=DEV)
    planted, pinv = hip.catalog_scores(user, catf[at].contiguous())
    assert torch.equal(_bits(S[:, at]), _bits(planted)) and torch.equal(_bits(cinv[at]), _bits(pinv))
    w0, w1 = M - 2048, min(N, M + 2048)                       # (the catalogue ends 1025 rows past 2^20)
    window, winv = hip.catalog_scores(user, catf[w0:w1].clone())
    assert window.shape == (B, w1 - w0)
    assert torch.equal(_bits(S[:, w0:w1]), _bits(window)) and torch.equal(_bits(cinv[w0:w1]), _bits(winv))
    # the rows differ, so equal bits are not an accident of a repeated row: (nearly) every column of the window has its own score
    assert len(set(_bits(window[0]).tolist())) > 0.99 * (w1 - w0)


@gpu
def test_prefix_norms_past_4gib(big):
    cat, dims = big["cat"], (PREFIX, D)
    inv = hip.catalog_prefix_norms(cat, dims)
    tail = hip.catalog_prefix_norms(cat[N - 2049:].clone(), dims)
    assert inv.shape == (2, N) and torch.equal(_bits(inv[:, N - 2049:]), _bits(tail))
    r = cat[N - 2049:].double()
    for l, d in enumerate(dims):                            # and the compact call is right: float64, the f32 chain's few roundings
        i64 = 1.0 / r[:, :d].norm(dim=1)
        assert float(((tail[l].double() - i64).abs() / i64).max()) <= (4 * (d // 256) + 8) * 2.0 ** -24


@gpu
def test_reranks_past_4gib(big):
    """index lists of planted and nearby rows past 2^20 against the same call on a compact copy of the last 2049 rows"""
    user, cat = big["user"], big["cat"]
    s0 = N - 2049
    compact = cat[s0:].clone()
    g = torch.Generator().manual_seed(77)
    past = [n for n in PLANTED if n >= M]
    near = sorted({min(N - 1, max(M, n + o)) for n in past for o in (-2, -1, 1, 2)} - set(past))
    for K_in, calls in ((128, [("rerank", lambda c, i: hip.catalog_rerank(user, c, i, 10))]),
                        (129, [("deep rerank", lambda c, i: hip.catalog_deep_rerank(user, c, i, 10)),
                               ("funnel rerank", lambda c, i: hip.catalog_funnel_rerank(user, c, i, PREFIX, 10))])):
        rows = []
        for b in range(B):
            fixed = past + near
            rest = (M + torch.randperm(1025, generator=g)).tolist()
            rest = [n for n in rest if n not in fixed][:K_in - len(fixed)]
            rows.append(torch.tensor(fixed + rest)[torch.randperm(K_in, generator=g)])
        index = torch.stack(rows).to(torch.int32).to(DEV)
        assert index.shape == (B, K_in) and int(index.min()) >= M and int(index.max()) == N - 1
        for what, call in calls:
            idx, val, cinv = call(cat, index)
            widx, wval, winv = call(compact, index - s0)
            assert torch.equal(idx, widx + s0), what
            assert torch.equal(_bits(val), _bits(wval)), what
            assert torch.equal(_bits(cinv[s0:]), _bits(winv)), what
            if what != "funnel rerank":                     # the exact full-width order puts the user's own planted rows past 2^20 first
                for b in range(B):
                    mine = [n for n in _want_lists(b) if n >= M]
                    assert idx[b, :len(mine)].cpu().tolist() == mine, (what, b)

"""GPU: the Matryoshka catalogue softmax (ur_catalog_mrl_softmax / hip.catalog_mrl_softmax / CatalogSoftmaxLoss(matryoshka_dims=...) /
the trainers' keywords).

What is held, at equal explicit chunk_rows, is BITS: plane k of one call on the resident [N,D] catalogue against hip.catalog_softmax on
the contiguous copies user[:, :d_k], catalog[:, :d_k] -- row_loss, lse, the plane's loss, the norm plane; with one-hot weights the loss
and d_user[:, :d_k] too, with d_user[:, d_k:] == 0; with general weights d_user and loss against the ascending-k fma combine of the sliced
calls' results, formed on the host (float64 product of two f32 factors is exact, one rounding to f32: an fma).  Neither the scorer nor
the catalogue's storage type shows, two calls agree, K = 1 is hip.catalog_softmax on the same buffers, and what lies behind a prefix in
a row reaches no result of that plane.

With chunk_rows left to the library the chunk and split sizes differ from the sliced call's, so there each plane is held to the float64
restatement tests/catalog_softmax_ref.py on the slice, under the bounds of tests/test_gpu_catalog_softmax.py (restated in _bounds below:
4x the measured error of the InfoNCE kernels on the same candidates, never below 8 f32 ulps of the quantity's magnitude -- that file's
docstring derives the magnitudes); loss and d_user are held to the weighted float64 sum under sum_k weights[k] * bound_k.
Every figure is printed before it is asserted (run with -s)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.catalog_softmax_ref import catalog_softmax_ref  # noqa: E402
from unirec_amd import hip  # noqa: E402
from unirec_amd.evaluation import pack_exclude  # noqa: E402

DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
ULP8 = 8 * 2.0 ** -23
GRAD_SCALE = 0.5
WEIGHTS = (0.75, 0.0, 1.5, 0.3, 2.0)            # general weights, with a plane of weight 0 among them; the first K are taken
PRODUCT = (64, 128, 256, 512, 1024)

COVERS = {
    "ur_catalog_mrl_softmax": ["test_bits_against_the_sliced_calls", "test_one_plane_is_the_plain_call", "test_live_data_behind_the_prefix",
                               "test_default_chunk_rows_against_float64", "test_forward_only", "test_everything_but_the_ground_truth_excluded"],
}

# B: either side of the 16-user group of the vector scorer and of the 32-user group of the MFMA scorer and the gradient product; N with
# chunk_rows = 1024: one row, either side of a chunk, several chunks with a one-row and a ragged last chunk; dims: a prefix inside the
# first 256-element piece, on and just past a piece boundary, the product's widths, the wide D > 1024 path, the single plane; E:
# exclusion rows with the ground truth, duplicates and -1 in them.  Thinned by hand so that every value and every pair (dtype, scorer)
# occurs.  (All dims are multiples of 8: a bf16 catalogue takes them.)
GRID = [
    (1, 1, (8, 16), 0, 0.07, F32, "vector"),
    (16, 1023, (8, 256, 264), 1, 1.0, BF16, "mfma"),
    (17, 1025, PRODUCT, 9, 0.01, F32, "mfma"),
    (33, 2049, (248, 1032), 9, 0.07, BF16, "vector"),
    (1, 5003, (264,), 1, 0.01, F32, "mfma"),
    (16, 5003, (8, 16), 9, 1.0, BF16, "mfma"),
    (17, 1, (8, 256, 264), 0, 0.07, BF16, "vector"),
    (33, 1023, PRODUCT, 0, 0.07, BF16, "mfma"),
    (1, 1025, (248, 1032), 1, 1.0, F32, "mfma"),
    (16, 2049, (264,), 9, 0.07, BF16, "vector"),
    (33, 5003, (8, 256, 264), 1, 0.01, F32, "vector"),
    (17, 2049, PRODUCT, 1, 1.0, F32, "vector"),
    (33, 1025, (248, 1032), 0, 0.01, F32, "vector"),
]


def _id(c):
    return f"B{c[0]}-N{c[1]}-d{'_'.join(map(str, c[2]))}-E{c[3]}-tau{c[4]}-{'f32' if c[5] is F32 else 'bf16'}-{c[6]}"


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), what


def _exclude_rows(B, N, E, gt, g):
    """[B,E] int64 with, per row: the user's own ground truth (even rows), a duplicated entry, -1 padding, random rows"""
    if E == 0:
        return None
    ex = torch.randint(0, N, (B, E), generator=g)
    ex[0::2, 0] = gt[0::2]
    if E > 2:
        ex[:, 1] = ex[:, 2]
        ex[:, E - 1] = -1
        ex[1::2, 3] = -1
    return ex


@functools.lru_cache(maxsize=None)
def _case(B, N, D, E, dtype):
    g = torch.Generator().manual_seed(B + 3 * N + 7 * D + 11 * E)
    user = torch.randn(B, D, generator=g).to(DEV)
    C = torch.randn(N, D, generator=g).to(DEV).to(dtype)
    gt = torch.randint(0, N, (B,), generator=g)
    raw = _exclude_rows(B, N, E, gt, g)
    ex = pack_exclude(raw, B)
    return user, C, gt, raw, None if ex is None else ex.to(DEV)


def _sliced(user, C, gt, ex, dims, tau, **kw):
    """hip.catalog_softmax on the contiguous slices, one call per plane: [(loss, row_loss, lse, d_user, cat_inv_norm)]"""
    return [hip.catalog_softmax(user[:, :d].contiguous(), C[:, :d].contiguous(), gt, tau, exclude=ex, grad_scale=GRAD_SCALE, **kw) for d in dims]


def _fma(w, x, acc):
    """f32 fmaf(w, x, acc) elementwise on the host: the float64 product of two f32 numbers is exact; one rounding to f32"""
    return (torch.tensor(w, dtype=F32).double() * x.double() + acc.double()).to(F32)


def _combine(weights, planes, dims, B, D):
    """(loss [1], d_user [B,D]) of the header's definition from the sliced calls: fmaf from 0 in ascending k, weight 0 skipped"""
    loss, du = torch.zeros(1), torch.zeros(B, D)
    for w, p, d in zip(weights, planes, dims):
        if w > 0:
            loss = _fma(w, p[0].cpu(), loss)
            du[:, :d] = _fma(w, p[3].cpu(), du[:, :d])
    return loss, du


@pytest.mark.parametrize("B,N,dims,E,tau,dtype,scorer", GRID, ids=[_id(c) for c in GRID])
def test_bits_against_the_sliced_calls(B, N, dims, E, tau, dtype, scorer):
    D, K = dims[-1], len(dims)
    user, C, gt, _, ex = _case(B, N, D, E, dtype)
    call = lambda weights, cat=C, **kw: hip.catalog_mrl_softmax(user, cat, gt, dims, weights, tau, exclude=ex, grad_scale=GRAD_SCALE,      # noqa: E731
                                                                **{"chunk_rows": 1024, "scorer": scorer, **kw})
    planes = _sliced(user, C, gt, ex, dims, tau, chunk_rows=1024, scorer=scorer)
    weights = WEIGHTS[:K]
    got = call(weights)
    loss, plane_loss, row_loss, lse, d_user, norms = got
    assert loss.shape == (1,) and plane_loss.shape == (K,) and row_loss.shape == (K, B) and lse.shape == (K, B)
    assert d_user.shape == (B, D) and norms.shape == (K, N)
    for k, p in enumerate(planes):                                                           # 1: every plane, bit for bit
        _same(row_loss[k], p[1], f"row_loss of plane {k}")
        _same(lse[k], p[2], f"lse of plane {k}")
        _same(norms[k], p[4], f"cat_inv_norm of plane {k}")
        _same(plane_loss[k:k + 1], p[0], f"plane_loss of plane {k}")
    want_loss, want_du = _combine(weights, planes, dims, B, D)                               # general weights: the fma combine
    assert torch.equal(loss.cpu(), want_loss) and torch.equal(d_user.cpu(), want_du)
    for k, p in enumerate(planes):                                                           # one-hot weights: that call's loss and gradient
        hot = call(tuple(float(j == k) for j in range(K)), cat_inv_norms=norms)
        assert torch.equal(hot[0], p[0]) and torch.equal(hot[4][:, :dims[k]], p[3]), f"one-hot at plane {k}"
        assert not bool(hot[4][:, dims[k]:].any()), f"d_user past plane {k}'s width"
        for a, b in zip(hot[1:4], got[1:4]):
            _same(a, b, "the weights reach no plane's own outputs")
    other = call(weights, scorer="mfma" if scorer == "vector" else "vector", cat_inv_norms=norms)      # 2: the scorer never shows
    for a, b in zip(got, other):
        _same(a, b, "scorer")
    if dtype is BF16:                                                                        # 2: nor does the storage type
        for a, b in zip(got, call(weights, cat=C.float())):
            _same(a, b, "bf16 against its f32 copy")
    for a, b in zip(got, call(weights)):                                                     # 3: two calls
        _same(a, b, "two calls")
    for t in got:
        assert bool(torch.isfinite(t).all())


@pytest.mark.parametrize("B,N,D,E,tau,dtype,scorer", [(17, 2049, 264, 9, 0.07, F32, "mfma"), (33, 1025, 1024, 1, 0.01, BF16, "vector"),
                                                       (16, 1023, 1032, 0, 1.0, BF16, "mfma")])
def test_one_plane_is_the_plain_call(B, N, D, E, tau, dtype, scorer):
    """3: K = 1, dims = (D,), weights = (1,): every output of hip.catalog_softmax on the same buffers"""
    user, C, gt, _, ex = _case(B, N, D, E, dtype)
    plain = hip.catalog_softmax(user, C, gt, tau, exclude=ex, chunk_rows=1024, scorer=scorer, grad_scale=GRAD_SCALE)
    got = hip.catalog_mrl_softmax(user, C, gt, (D,), (1.0,), tau, exclude=ex, chunk_rows=1024, scorer=scorer, grad_scale=GRAD_SCALE)
    _same(got[0], plain[0], "loss")
    _same(got[1], plain[0], "plane_loss")
    _same(got[2][0], plain[1], "row_loss")
    _same(got[3][0], plain[2], "lse")
    _same(got[4], plain[3], "d_user")
    _same(got[5][0], plain[4], "cat_inv_norm")
    fed = hip.catalog_mrl_softmax(user, C, gt, (D,), None, tau, cat_inv_norms=plain[4][None].contiguous(), exclude=ex, chunk_rows=1024,
                                  scorer=scorer, grad_scale=GRAD_SCALE)                      # the plain call's norms, weights left to the default
    for a, b in zip(fed, got):
        _same(a, b, "norms brought by the caller")


@pytest.mark.parametrize("dims,k,dtype,scorer", [((8, 256, 264), 0, F32, "mfma"), ((8, 256, 264), 1, BF16, "vector"), ((248, 1032), 0, BF16, "mfma"),
                                                  (PRODUCT, 2, F32, "vector")])
def test_live_data_behind_the_prefix(dims, k, dtype, scorer):
    """4: with the weights one-hot at plane k, other finite values behind d_k in every user and catalogue row change no bit of the
    loss, of plane k's outputs or of d_user"""
    B, N, D, E, tau = 17, 2049, dims[-1], 9, 0.07
    user, C, gt, _, ex = _case(B, N, D, E, dtype)
    hot = tuple(float(j == k) for j in range(len(dims)))
    call = lambda u, c: hip.catalog_mrl_softmax(u, c, gt, dims, hot, tau, exclude=ex, chunk_rows=1024, scorer=scorer, grad_scale=GRAD_SCALE)      # noqa: E731
    before = call(user, C)
    g = torch.Generator().manual_seed(99)
    user2, C2 = user.clone(), C.clone()
    user2[:, dims[k]:] = (37.0 * torch.randn(B, D - dims[k], generator=g)).to(DEV)
    C2[:, dims[k]:] = (1e3 * torch.randn(N, D - dims[k], generator=g)).to(DEV).to(dtype)
    assert not torch.equal(user2, user) and not torch.equal(C2, C)
    after = call(user2, C2)
    _same(after[0], before[0], "loss")
    _same(after[4], before[4], "d_user")
    for i, what in ((1, "plane_loss"), (2, "row_loss"), (3, "lse"), (5, "cat_inv_norm")):
        _same(after[i][:k + 1], before[i][:k + 1], what)                                     # (the planes up to k lie inside the prefix)
    assert not torch.equal(after[2][-1], before[2][-1]), "the widest plane does read the new values"


def _bounds(user, C, gt, tau, ref, grad_scale):
    """tests/test_gpu_catalog_softmax.py's bounds, restated: the error of hip.cosine_scores + hip.infonce_fwd_bwd against the same float64
    reference on the identical candidate set (per user: the positive = catalogue row g_b, the N rows as negatives masked to the kept
    ones without g_b); a bound is 4x that error and never below 8 f32 ulps of the quantity's magnitude"""
    B, N = ref["keep"].shape
    Cf = C.float()
    rows, dus = [], []
    for b in range(B):
        gb = int(gt[b])
        u, pos, neg = user[b:b + 1].contiguous(), Cf[gb:gb + 1], Cf[None]
        mask = ref["keep"][b].clone()
        mask[gb] = False
        mask = mask.to(torch.uint8)[None].contiguous().to(DEV)
        scores, inv = hip.cosine_scores(u, pos, neg)
        loss, du = hip.infonce_fwd_bwd(u, pos, neg, mask, scores, inv, tau, grad_scale / B)
        rows.append(loss.double().cpu())
        dus.append(du.double().cpu())
    rows, dus = torch.cat(rows), torch.cat(dus)
    err_row = float((rows - ref["row_loss"]).abs().max())
    err_loss = abs(float(rows.mean() - ref["loss"]))
    err_du = float((dus - ref["d_user"]).abs().max())
    z = ref["scores"].abs() * ref["keep"] / float(torch.tensor(tau, dtype=F32))
    mag_l = max(float(ref["lse"].abs().max()), float(z.max()))
    u64, c64 = user.double().cpu(), Cf.double().cpu()[gt]
    iu = 1.0 / u64.norm(dim=1).clamp_min(1e-12)
    chat = c64 / c64.norm(dim=1, keepdim=True).clamp_min(1e-12)
    mag_du = max(float(ref["d_user"].abs().max()), grad_scale / (B * tau) * float((iu * chat.abs().max(dim=1).values).max()))
    return {"err": {"loss": err_loss, "row_loss": err_row, "lse": err_row, "d_user": err_du},
            "bound": {"loss": max(4 * err_loss, ULP8 * mag_l), "row_loss": max(4 * err_row, ULP8 * mag_l),
                      "lse": max(4 * err_row, ULP8 * mag_l), "d_user": max(4 * err_du, ULP8 * mag_du)}}


def _hold_planes(tag, got, user, C, gt, raw, dims, weights, tau, grad_scale):
    """every plane against the float64 restatement on its slice, then loss and d_user against the weighted float64 sum"""
    loss, plane_loss, row_loss, lse, d_user, _ = got
    B, D = user.shape
    want_loss, want_du = torch.zeros((), dtype=F64), torch.zeros(B, D, dtype=F64)
    bound_loss = bound_du = 0.0
    for k, d in enumerate(dims):
        u, c = user[:, :d].contiguous(), C[:, :d].contiguous()
        ref = catalog_softmax_ref(u, c, gt, tau, raw, grad_scale)
        bounds = _bounds(u, c, gt, tau, ref, grad_scale)
        errs = {"loss": abs(float(plane_loss[k].double().cpu() - ref["loss"])),
                "row_loss": float((row_loss[k].double().cpu() - ref["row_loss"]).abs().max()),
                "lse": float((lse[k].double().cpu() - ref["lse"]).abs().max())}
        for q, e in errs.items():
            print(f"{tag} plane {k} (d {d}) {q}: error {e:.3e}  InfoNCE kernels {bounds['err'][q]:.3e}  bound {bounds['bound'][q]:.3e}")
        for q, e in errs.items():
            assert e <= bounds["bound"][q], (tag, k, q, e, bounds["bound"][q])
        w = float(torch.tensor(weights[k], dtype=F32))
        want_loss += w * ref["loss"]
        want_du[:, :d] += w * ref["d_user"]
        bound_loss += w * bounds["bound"]["loss"]
        bound_du += w * bounds["bound"]["d_user"]
    e_loss = abs(float(loss.double().cpu()[0] - want_loss))
    print(f"{tag} loss: error {e_loss:.3e}  bound {bound_loss:.3e}")
    assert e_loss <= bound_loss
    if d_user is not None:
        e_du = float((d_user.double().cpu() - want_du).abs().max())
        print(f"{tag} d_user: error {e_du:.3e}  bound {bound_du:.3e}")
        assert e_du <= bound_du
    for t in got[:5]:
        assert t is None or bool(torch.isfinite(t).all())


@pytest.mark.parametrize("B,N,dims,E,tau,dtype,scorer", [(17, 5003, (8, 256, 264), 9, 0.07, F32, None), (16, 2049, PRODUCT, 1, 0.01, BF16, None),
                                                          (33, 5003, (248, 1032), 0, 1.0, BF16, "vector")], ids=["f32-264", "bf16-product", "bf16-wide"])
def test_default_chunk_rows_against_float64(B, N, dims, E, tau, dtype, scorer):
    """5: chunk_rows (and here the scorer) left to the library: the chunk is the whole catalogue rounded up, so segments and splits are
    not the sliced call's -- each plane, the loss and d_user against float64"""
    user, C, gt, raw, ex = _case(B, N, dims[-1], E, dtype)
    weights = WEIGHTS[:len(dims)]
    got = hip.catalog_mrl_softmax(user, C, gt, dims, weights, tau, exclude=ex, scorer=scorer, grad_scale=GRAD_SCALE)
    _hold_planes("chunk default", got, user, C, gt, raw, dims, weights, tau, GRAD_SCALE)
    for a, b in zip(got, hip.catalog_mrl_softmax(user, C, gt, dims, weights, tau, exclude=ex, scorer=scorer, grad_scale=GRAD_SCALE)):
        _same(a, b, "two calls")


def test_forward_only():
    """6: need_grad=False gives the same forward bits, no d_user, and a smaller workspace"""
    B, N, dims, tau = 17, 2049, (8, 256, 264), 0.07
    user, C, gt, _, ex = _case(B, N, dims[-1], 9, F32)
    for key in [k for k in hip._ws_cache if k[1] == "catalog_mrl_softmax"]:                   # (grow-only: start from no buffer)
        del hip._ws_cache[key]
    fwd = hip.catalog_mrl_softmax(user, C, gt, dims, None, tau, exclude=ex, chunk_rows=1024, need_grad=False)
    assert fwd[4] is None
    forward_bytes = hip.workspace(1, user.device, "catalog_mrl_softmax").numel()
    full = hip.catalog_mrl_softmax(user, C, gt, dims, None, tau, exclude=ex, chunk_rows=1024)
    for i in (0, 1, 2, 3, 5):
        _same(fwd[i], full[i], "forward outputs")
    assert full[4].shape == (B, dims[-1])
    assert hip.workspace(1, user.device, "catalog_mrl_softmax").numel() > forward_bytes, "the gradient pass needs the per-plane slabs on top"


@pytest.mark.parametrize("dtype,scorer", [(F32, "vector"), (BF16, "mfma")], ids=["f32-vector", "bf16-mfma"])
def test_everything_but_the_ground_truth_excluded(dtype, scorer):
    """7: every row but the ground truth is excluded: each plane's sum has one term, so its row_loss is exactly 0, and d_user is exactly 0"""
    B, N, dims, tau = 3, 1500, (8, 256, 264), 0.07
    g = torch.Generator().manual_seed(4)
    user, C = torch.randn(B, 264, generator=g).to(DEV), torch.randn(N, 264, generator=g).to(DEV).to(dtype)
    gt = torch.tensor([0, 1499, 1024])
    ex = pack_exclude(torch.arange(N)[None].expand(B, N).contiguous(), B).to(DEV)
    got = hip.catalog_mrl_softmax(user, C, gt, dims, (1.0, 0.5, 2.0), tau, exclude=ex, chunk_rows=1024, scorer=scorer)
    print("row_loss", got[2].cpu().tolist(), "max |d_user|", float(got[4].abs().max()))
    assert not bool(got[2].any()) and not bool(got[1].any()) and not bool(got[0].any()) and not bool(got[4].any())
    assert bool(torch.isfinite(got[3]).all())


def test_loss_module_autograd():
    """8: CatalogSoftmaxLoss(matryoshka_dims=...) is an autograd function over the call; its norm planes are the evaluator's, the ones
    retrieve_funnel over the same widths searches with; without dims it is the plain loss, bit for bit"""
    from unirec_amd.evaluation import CatalogEvaluator
    from unirec_amd.joint import CatalogSoftmaxLoss
    B, N, dims, tau = 17, 2049, (8, 256, 264), 0.07
    weights = (0.75, 0.0, 1.5)
    user, C, gt, _, ex = _case(B, N, dims[-1], 9, BF16)
    ev = CatalogEvaluator(C, dtype=BF16)
    fn = CatalogSoftmaxLoss(ev, tau, None, 1024, matryoshka_dims=dims, matryoshka_weights=weights)
    u = user.clone().requires_grad_(True)
    loss = fn(u, gt, exclude=ex)
    (loss * 3.0).backward()
    want = hip.catalog_mrl_softmax(user, C, gt, dims, weights, tau, exclude=ex, chunk_rows=1024)
    assert loss.shape == () and torch.equal(loss.detach().view(1), want[0])
    _same(fn.last_plane_loss, want[1], "last_plane_loss")
    _same(fn.last_row_loss, want[2], "last_row_loss [K,B]")
    _same(fn.last_lse, want[3], "last_lse [K,B]")
    assert torch.equal(u.grad, want[4] * 3.0), "backward = the call's d_user times the upstream gradient"
    planes = hip.catalog_prefix_norms(C, dims)
    assert sorted(ev._prefix_inv) == [8, 256] and ev._inv is not None
    for k, d in enumerate(dims):
        _same(ev._inv if d == dims[-1] else ev._prefix_inv[d], planes[k], "the evaluator holds the plane of every width")
        _same(want[5][k], planes[k], "and the call computes the same plane")
    kept = fn._planes
    fn(user, gt, exclude=ex)
    assert fn._planes is kept, "the planes are stacked once"
    r = ev.retrieve_funnel(user, k=5, dims=dims, gt_index=gt, chunk_rows=1024)                # the funnel finds every plane in place
    assert sorted(ev._prefix_inv) == [8, 256] and r["topk_index"].shape == (B, 5)
    # without dims: today's path
    ev2 = CatalogEvaluator(C, dtype=BF16)
    plain = CatalogSoftmaxLoss(ev2, tau, None, 1024)
    u2 = user.clone().requires_grad_(True)
    plain(u2, gt, exclude=ex).backward()
    ref = hip.catalog_softmax(user, C, gt, tau, exclude=ex, chunk_rows=1024)
    assert plain.last_plane_loss is None and plain.last_row_loss.shape == (B,)
    _same(plain.last_row_loss, ref[1], "plain row_loss")
    _same(u2.grad, ref[3], "plain gradient")


def _args(**over):
    import types
    kw = dict(learning_rate=1e-3, warmup_steps=0, max_steps=4, max_grad_norm=1.0, weight_decay=0.01, logging_steps=1)
    kw.update(over)
    return types.SimpleNamespace(**kw)


def test_trainer_step():
    """8: a JointTrainer(loss="catalog_softmax", matryoshka_dims=...) step on the model of test_gpu_catalog_softmax's trainer test: its
    loss is the call's on the step's own user embeddings; the same trainer without dims gives the plain loss's bits"""
    from tests.test_gpu_grad_clip import _inputs, _joint
    from tests.test_gpu_negatives import _catalogue
    from unirec_amd.joint import JointTrainer, MultiModalTrainer
    from unirec_amd.negatives import CatalogCandidates
    case, model = _joint()
    full = _inputs(case)
    cat, pos_index, _ = _catalogue(full)
    D = cat.shape[1]
    dims, weights, tau = (8, D // 4, D), (1.0, 0.5, 2.0), 0.07
    batch = {k: v for k, v in full.items() if k not in ("positive_item_embeddings", "negative_item_embeddings", "negative_masks")}
    batch["positive_item_index"] = pos_index
    tr = JointTrainer(model, _args(), temperature=tau, negatives=CatalogCandidates(cat), loss="catalog_softmax", matryoshka_dims=dims,
                      matryoshka_weights=weights)
    plain = MultiModalTrainer(tau, CatalogCandidates(cat), loss="catalog_softmax")          # (JointTrainer's loss_fn, without a second optimizer)
    model.eval()
    with torch.no_grad():
        loss, user = tr.compute_loss(model, batch, return_outputs=True)
        u = user.float().contiguous()
        want = hip.catalog_mrl_softmax(u, cat, pos_index, dims, weights, tau)
        fn = tr.loss_fn.catalog_softmax_loss
        assert torch.equal(loss.view(1), want[0])
        _same(fn.last_plane_loss, want[1], "plane_loss")
        _same(fn.last_row_loss, want[2], "row_loss")
        loss_plain, user_plain = plain.compute_loss(model, batch, return_outputs=True)
        ref = hip.catalog_softmax(u, cat, pos_index, tau)
        assert torch.equal(_bits(user_plain), _bits(user)) and torch.equal(loss_plain.view(1), ref[0]), "without dims: today's bits"
        _same(plain.catalog_softmax_loss.last_row_loss, ref[1], "today's row_loss")
        assert plain.catalog_softmax_loss.last_plane_loss is None
    before = [p.master.clone() for p in tr.packs]
    out = tr.training_step(batch)
    assert out.shape == () and bool(torch.isfinite(out))
    assert tr.state.global_step == 1 and float(tr.optimizer.last_grad_norm) > 0
    assert any(not torch.equal(p.master, b) for p, b in zip(tr.packs, before)), "the parameters moved"
    assert all(bool(torch.isfinite(p.master).all()) for p in tr.packs)
    rec = tr.state.log_history[-1]
    assert len(rec["plane_loss"]) == 3 and all(v > 0 for v in rec["plane_loss"]), "the log carries the per-prefix losses"

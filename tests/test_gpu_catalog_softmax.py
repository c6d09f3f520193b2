"""GPU: the full-catalogue softmax loss (ur_catalog_softmax / hip.catalog_softmax / CatalogSoftmaxLoss / the trainers' loss keyword)
against the float64 restatement in tests/catalog_softmax_ref.py.

Tolerance.  Nothing here is a chosen constant: each case measures the error of the InfoNCE kernels this loss stands beside
(hip.cosine_scores + hip.infonce_fwd_bwd) against the SAME float64 reference on the IDENTICAL candidate set -- per user, the
positive = catalogue row g_b and the N catalogue rows as negatives, masked to the rows the user keeps and with row g_b itself masked
out (one positive plus the N - 1 other rows; calling it a user at a time makes `neg` a [1,N,D] view of the catalogue and yields the
per-user loss, which the batched call does not return).  The bound of a quantity is 4x that error (the chunk fold adds one rescale per
chunk and sums in another order), and never below 8 f32 ulps of the quantity's magnitude:
  loss, row_loss, lse: magnitude = max(|lse|, max |z_bn| over the kept rows) -- lse is a maximum of z plus a logarithm, and row_loss
      a difference of two such numbers, so their rounding is in ulps of the largest |z| even when the value itself is near 0;
      lse has no counterpart in the InfoNCE call and takes row_loss's measured error (row_loss = lse - z_g);
      the loss's measured error is that of the float64 mean of the InfoNCE per-user losses;
  d_user: errors are absolute maxima over [B,D], i.e. relative to max |d_user| on both sides of the comparison; magnitude =
      max(max |d_user|, grad_scale / (B tau) * max_b(iu_b * max_d |c^_g_b,d|)) -- the second is the term w_g c^_g before the
      "- 1" of the ground truth cancels against exp(z_g - lse), which rounds in ulps of 1 / tau however small the difference is
      (with every other row excluded the difference is exactly 0 and so is the reference, up to 1e-16).
Every figure is printed before it is asserted (run with -s); docs/lab_notes.md section 29 records them."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.catalog_softmax_ref import catalog_softmax_ref  # noqa: E402
from unirec_amd import hip  # noqa: E402
from unirec_amd.evaluation import pack_exclude  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
ULP8 = 8 * 2.0 ** -23

COVERS = {
    "ur_catalog_softmax": ["test_grid_against_float64", "test_everything_but_the_ground_truth_excluded", "test_forward_only"],
}

# B: both sides of the 16-user block; N with chunk_rows = 1024: one row, two, an exact chunk and either side of it, several chunks with
# a one-row and a ragged last chunk; D: one piece, a ragged column tile (264 = 256 + 8), the product width; E: exclusion rows with the
# ground truth, duplicates and -1 padding in them.  Thinned by hand so that every value and every pair (dtype, scorer) occurs.
GRID = [
    (1, 1, 4, 0, 0.07, F32, "vector"),
    (16, 2, 264, 1, 1.0, BF16, "mfma"),
    (17, 1023, 1024, 9, 0.01, F32, "mfma"),
    (1, 1024, 264, 9, 0.07, BF16, "vector"),
    (16, 1025, 4, 0, 0.01, F32, "mfma"),
    (17, 2049, 264, 1, 0.07, BF16, "vector"),
    (16, 5003, 1024, 9, 1.0, F32, "vector"),
    (17, 5003, 4, 1, 0.01, BF16, "mfma"),
    (1, 2049, 1024, 0, 1.0, F32, "mfma"),
    (17, 1, 1024, 0, 1.0, BF16, "vector"),
    (1, 2, 4, 9, 0.01, F32, "vector"),
    (16, 1023, 4, 1, 0.07, BF16, "mfma"),
    (17, 1025, 1024, 9, 0.07, BF16, "mfma"),
    (1, 1024, 1024, 1, 0.01, F32, "mfma"),
]
GRAD_SCALE = 0.5


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


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
def _case(B, N, D, E, tau, dtype):
    g = torch.Generator().manual_seed(B + 3 * N + 7 * D + 11 * E)
    user = torch.randn(B, D, generator=g).to(DEV)
    C = torch.randn(N, D, generator=g).to(DEV).to(dtype)
    gt = torch.randint(0, N, (B,), generator=g)
    raw = _exclude_rows(B, N, E, gt, g)
    ex = pack_exclude(raw, B)
    ref = catalog_softmax_ref(user, C, gt, tau, raw, GRAD_SCALE)
    return user, C, gt, None if ex is None else ex.to(DEV), ref, _bounds(user, C, gt, tau, ref, GRAD_SCALE)


def _bounds(user, C, gt, tau, ref, grad_scale):
    """The measured error of the InfoNCE kernels on the same candidates and the bounds derived from it (module docstring)."""
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


def _errors(got, ref):
    loss, row_loss, lse, d_user = got[:4]
    out = {"loss": abs(float(loss.double().cpu()[0] - ref["loss"])),
           "row_loss": float((row_loss.double().cpu() - ref["row_loss"]).abs().max()),
           "lse": float((lse.double().cpu() - ref["lse"]).abs().max())}
    if d_user is not None:
        out["d_user"] = float((d_user.double().cpu() - ref["d_user"]).abs().max())
    return out


def _hold(tag, got, ref, bounds):
    errs = _errors(got, ref)
    for q, e in errs.items():
        print(f"{tag} {q}: error {e:.3e}  InfoNCE kernels {bounds['err'][q]:.3e}  bound {bounds['bound'][q]:.3e}")
    for q, e in errs.items():
        assert e <= bounds["bound"][q], (tag, q, e, bounds["bound"][q])
    for t in got[:4]:
        assert t is None or bool(torch.isfinite(t).all())


@pytest.mark.parametrize("B,N,D,E,tau,dtype,scorer", GRID,
                         ids=[f"B{c[0]}-N{c[1]}-D{c[2]}-E{c[3]}-tau{c[4]}-{'f32' if c[5] is F32 else 'bf16'}-{c[6]}" for c in GRID])
def test_grid_against_float64(B, N, D, E, tau, dtype, scorer):
    user, C, gt, ex, ref, bounds = _case(B, N, D, E, tau, dtype)
    call = lambda cat=C, **kw: hip.catalog_softmax(user, cat, gt, tau, exclude=ex, grad_scale=GRAD_SCALE,      # noqa: E731
                                                   **{"chunk_rows": 1024, "scorer": scorer, **kw})
    got = call()
    assert got[0].shape == (1,) and got[1].shape == (B,) and got[2].shape == (B,) and got[3].shape == (B, D) and got[4].shape == (N,)
    _hold("chunk 1024", got, ref, bounds)                                                    # 1
    other = call(scorer="mfma" if scorer == "vector" else "vector", cat_inv_norm=got[4])     # 2: the scorer never shows
    for a, b in zip(got[:4], other[:4]):
        assert torch.equal(_bits(a), _bits(b))
    if dtype is BF16:                                                                        # 2: nor does the storage type
        wide = call(cat=C.float())
        for a, b in zip(got, wide):
            assert torch.equal(_bits(a), _bits(b))
    again = call()                                                                           # 3
    for a, b in zip(got, again):
        assert torch.equal(_bits(a), _bits(b))
    _hold("chunk default", call(chunk_rows=None), ref, bounds)                               # 4


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_everything_but_the_ground_truth_excluded(dtype):
    """5: the sum has one term: row_loss = 0 and d_user = 0 within the bounds (N = 1 is in the grid)"""
    B, N, D, tau = 3, 1500, 264, 0.07
    g = torch.Generator().manual_seed(4)
    user, C = torch.randn(B, D, generator=g).to(DEV), torch.randn(N, D, generator=g).to(DEV).to(dtype)
    gt = torch.tensor([0, 1499, 1024])
    raw = torch.arange(N)[None].expand(B, N).contiguous()
    ref = catalog_softmax_ref(user, C, gt, tau, raw, 1.0)
    assert float(ref["row_loss"].abs().max()) <= 1e-12 and float(ref["d_user"].abs().max()) <= 1e-12
    bounds = _bounds(user, C, gt, tau, ref, 1.0)
    for scorer in ("vector", "mfma"):
        got = hip.catalog_softmax(user, C, gt, tau, exclude=pack_exclude(raw, B).to(DEV), chunk_rows=1024, scorer=scorer)
        _hold(f"all excluded, {scorer}", got, ref, bounds)
        zero = torch.zeros(())
        print("row_loss", got[1].cpu().tolist(), "max |d_user|", float(got[3].abs().max()))
        assert float((got[1].double().cpu() - zero).abs().max()) <= bounds["bound"]["row_loss"]
        assert float((got[3].double().cpu() - zero).abs().max()) <= bounds["bound"]["d_user"]


def test_forward_only():
    """6: need_grad=False gives the same loss bits and runs no second pass: the workspace is the smaller one and its chunk buffer still
    holds the last chunk's raw scores (the second pass overwrites them with weights)."""
    B, N, D, tau = 5, 2500, 264, 0.07
    user, C, gt, ex, ref, bounds = _case(B, N, D, 9, tau, F32)
    for key in [k for k in hip._ws_cache if k[1] == "catalog_softmax"]:                      # (grow-only: start from no buffer)
        del hip._ws_cache[key]
    fwd = hip.catalog_softmax(user, C, gt, tau, exclude=ex, chunk_rows=1024, scorer="vector", need_grad=False)
    assert fwd[3] is None
    _hold("forward only", fwd, ref, bounds)
    ws = hip.workspace(1, user.device, "catalog_softmax")
    forward_bytes = ws.numel()
    last = N - 2048                                                                          # rows 2048 .. 2499 are the last chunk
    S, _ = hip.catalog_scores(user, C)
    held = ws[:B * last * 4].view(F32).view(B, last).clone()
    assert torch.equal(_bits(held), _bits(S[:, 2048:]))
    full = hip.catalog_softmax(user, C, gt, tau, exclude=ex, chunk_rows=1024, scorer="vector", grad_scale=GRAD_SCALE)
    for a, b in zip(fwd[:3], full[:3]):
        assert torch.equal(_bits(a), _bits(b))
    ws2 = hip.workspace(1, user.device, "catalog_softmax")
    assert ws2.numel() > forward_bytes, "the gradient pass needs the partial [B,D] slabs on top"
    assert not torch.equal(_bits(ws2[:B * last * 4].view(F32).view(B, last)), _bits(S[:, 2048:])), "pass 2 leaves weights in the chunk buffer"
    _hold("with the gradient", full, ref, bounds)


def test_loss_module_autograd():
    """CatalogSoftmaxLoss: an autograd function over hip.catalog_softmax; the catalogue norms are computed once and shared with the evaluator"""
    from unirec_amd.evaluation import CatalogEvaluator
    from unirec_amd.joint import CatalogSoftmaxLoss
    B, N, D, tau = 5, 2500, 264, 0.07
    user, C, gt, ex, ref, bounds = _case(B, N, D, 9, tau, F32)
    ev = CatalogEvaluator(C)
    fn = CatalogSoftmaxLoss(ev, tau, chunk_rows=1024)
    u = user.clone().requires_grad_(True)
    loss = fn(u, gt, exclude=ex)
    assert loss.shape == () and ev._inv is not None
    inv = ev._inv
    (loss * GRAD_SCALE).backward()
    _hold("module", (loss.detach().view(1), fn.last_row_loss, fn.last_lse, u.grad), ref, bounds)
    loss2 = fn(user, gt, exclude=[[int(i) for i in r if i >= 0] for r in ex.cpu()])          # ragged lists, cached norms
    assert ev._inv is inv and torch.equal(_bits(loss2), _bits(loss))
    r = ev.retrieve(user, k=5, gt_index=gt, chunk_rows=1024)                                  # the evaluator goes on using the same norms
    assert ev._inv is inv and r["rank"].shape == (B,)


def _args(**over):
    import types
    kw = dict(learning_rate=1e-3, warmup_steps=0, max_steps=4, max_grad_norm=1.0, weight_decay=0.01, logging_steps=0)      # (no warm-up: the first step's rate is not 0)
    kw.update(over)
    return types.SimpleNamespace(**kw)


def test_trainer_step():
    """7: one JointTrainer(loss="catalog_softmax") step on the golden joint case over test_gpu_negatives' catalogue"""
    from tests.test_gpu_grad_clip import _inputs, _joint
    from tests.test_gpu_negatives import _catalogue
    from unirec_amd.joint import JointTrainer
    from unirec_amd.negatives import CatalogCandidates
    case, model = _joint()
    full = _inputs(case)
    cat, pos_index, _ = _catalogue(full)
    batch = {k: v for k, v in full.items() if k not in ("positive_item_embeddings", "negative_item_embeddings", "negative_masks")}
    batch["positive_item_index"] = pos_index
    tau = 0.07
    tr = JointTrainer(model, _args(), temperature=tau, negatives=CatalogCandidates(cat), loss="catalog_softmax")
    with pytest.raises(ValueError, match="negative_masks"):
        tr.compute_loss(model, dict(batch, negative_masks=full["negative_masks"]))
    model.eval()
    with torch.no_grad():
        loss, user = tr.compute_loss(model, batch, return_outputs=True)
        B, N = user.shape[0], cat.shape[0]
        ref = catalog_softmax_ref(user.float(), cat, pos_index, tau)
        fn = tr.loss_fn.catalog_softmax_loss
        _hold("trainer", (loss.view(1), fn.last_row_loss, fn.last_lse, None), ref, _bounds(user.float().contiguous(), cat, pos_index.cpu(), tau, ref, 1.0))
        # the items a user has seen leave the sum: here the best-scoring other rows, so the loss must fall
        S = ref["scores"].clone()
        S[torch.arange(B), pos_index.cpu()] = -2.0
        seen = S.topk(7, dim=1).indices
        seen[:, 0] = pos_index.cpu()                                                         # (the positive itself is never dropped)
        loss_seen, user2 = tr.compute_loss(model, dict(batch, seen_item_index=seen.to(DEV)), return_outputs=True)
        assert torch.equal(_bits(user2), _bits(user))
        ref_seen = catalog_softmax_ref(user.float(), cat, pos_index, tau, seen)
        _hold("trainer, seen", (loss_seen.view(1), fn.last_row_loss, fn.last_lse, None), ref_seen,
              _bounds(user.float().contiguous(), cat, pos_index.cpu(), tau, ref_seen, 1.0))
        assert float(loss_seen) < float(loss) and float(ref_seen["loss"]) < float(ref["loss"])
    before = [p.master.clone() for p in tr.packs]
    out = tr.training_step(dict(batch, seen_item_index=seen.to(DEV)))
    assert out.shape == () and bool(torch.isfinite(out))
    assert tr.state.global_step == 1 and float(tr.optimizer.last_grad_norm) > 0
    assert any(not torch.equal(p.master, b) for p, b in zip(tr.packs, before)), "the parameters moved"
    assert all(bool(torch.isfinite(p.master).all()) for p in tr.packs)

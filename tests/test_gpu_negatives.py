"""GPU: candidates by index -- the widening gather (bf16 rows to f32 rows, bit for bit), mining against the plain catalogue scores,
and the joint step on an index batch against the same step on the embedding batch gathered with torch."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. the widening gather
@pytest.mark.parametrize("D", [8, 264, 1024])
def test_widening_gather_bit_for_bit(D):
    from unirec_amd import hip
    n_src = 37
    g = torch.Generator().manual_seed(D)
    src = torch.randn(n_src, D, generator=g).to(BF16).to(DEV)
    shapes = [(1,), (5,), (1027,), (3, 7)]
    for shape in shapes:
        idx = torch.randint(-1, n_src + 1, shape, generator=g)          # -1 and n_src are drawn too; duplicates come by themselves
        flat = idx.view(-1)
        edge = torch.tensor([0, n_src - 1, -1, n_src, 0])
        flat[:min(flat.numel(), 5)] = edge[:min(flat.numel(), 5)]        # [1]: index 0; the others: every edge and a duplicate
        if shape == (1,):
            cases = [idx, torch.tensor([n_src - 1]), torch.tensor([-1]), torch.tensor([n_src])]
        else:
            cases = [idx]
        for ix in cases:
            ix = ix.to(DEV)
            out = hip.gather_rows(src, ix, out_dtype=F32)
            assert out.dtype == F32 and out.shape == tuple(ix.shape) + (D,)
            valid = (ix >= 0) & (ix < n_src)
            want = torch.where(valid[..., None], src[ix.clamp(0, n_src - 1)].float(), torch.zeros((), device=DEV))
            assert torch.equal(_bits(out), _bits(want)), (D, shape)
    assert hip.gather_rows(src, torch.empty(0, dtype=torch.int64, device=DEV), out_dtype=F32).shape == (0, D)


def test_widening_gather_keeps_every_bit_pattern():
    from unirec_amd import hip
    pat = torch.arange(65536, dtype=torch.int32).to(torch.int16)         # wraps: every 16-bit pattern once (NaN payloads, inf, subnormals, -0)
    src = pat.view(BF16).view(8192, 8).to(DEV)
    perm = torch.randperm(8192, generator=torch.Generator().manual_seed(0)).to(DEV)
    out = hip.gather_rows(src, perm, out_dtype=F32)
    want = ((src.view(torch.int16)[perm].to(torch.int64) & 0xFFFF) << 16).to(torch.int32)      # the narrowing wraps: the same 32 bits
    assert torch.equal(_bits(out), want)
    assert torch.unique(_bits(out)).numel() == 65536


def test_widening_gather_refuses_odd_rows():
    from unirec_amd import hip
    src = torch.zeros(4, 12, dtype=BF16, device=DEV)
    with pytest.raises(Exception) as e:
        hip.gather_rows(src, torch.tensor([0], device=DEV), out_dtype=F32)
    assert "ur_gather_rows" in str(e.value)


# ---- 2. mining against the plain scores
def _mining_case(B, N, D, seed):
    g = torch.Generator().manual_seed(seed)
    cat = torch.randn(N, D, generator=g)
    cat[N // 2] = cat[3]                                                 # two items with equal scores: the lower index comes first
    user = torch.randn(B, D, generator=g)
    gt = torch.randint(0, N, (B,), generator=g)
    return cat, user, gt


def _expected(scores, gt, exclude, hard_skip, num_hard):
    """positions hard_skip .. hard_skip + num_hard of each user's non-excluded items (the ground truth is never excluded) ordered by
    (score descending, index ascending), the ground truth then removed."""
    s = scores.cpu().numpy()
    out = []
    for b in range(s.shape[0]):
        seen = set(exclude[b]) - {int(gt[b])} if exclude is not None else set()
        order = np.lexsort((np.arange(s.shape[1]), -s[b].astype(np.float64)))
        order = [int(n) for n in order if int(n) not in seen]
        out.append([n for n in order[hard_skip:hard_skip + num_hard] if n != int(gt[b])])
    return out


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("hard_skip", [0, 5])
@pytest.mark.parametrize("shape", [(3, 129, 16, 128), (5, 5003, 48, 12)])
def test_mining_against_plain_scores(shape, hard_skip, dtype):
    """(3, 129, 16): hard_skip + num_hard = 128 and, with the exclusions, fewer candidates than that.  (5, 5003, 48): a list of 12
    folded over five chunks of 1024 rows (CatalogCandidates.chunk_rows)."""
    from unirec_amd import hip
    from unirec_amd.negatives import CatalogCandidates
    B, N, D, K = shape
    num_hard = K - hard_skip
    cat, user, gt = _mining_case(B, N, D, seed=N + hard_skip)
    cat = cat.to(dtype).to(DEV)
    user = user.to(DEV)
    scores, _ = hip.catalog_scores(user, cat.float())                     # a bf16 catalogue scores as its f32 copy, bit for bit
    top = torch.argsort(scores, dim=1, descending=True)[:, :8].cpu()
    exclude = [sorted({int(gt[b])} | {int(top[b, j]) for j in (0, 2, 3)} | {(7 * b + j) % N for j in range(b)}) for b in range(B)]
    cc = CatalogCandidates(cat, num_hard=num_hard, hard_skip=hard_skip)
    if N > 1024:
        cc.chunk_rows = 1024
    for ex in (None, exclude):
        mined = cc.mine(user.clone().requires_grad_(True), gt, ex)
        assert mined.dtype == torch.int64 and mined.shape == (B, num_hard) and mined.device == cat.device
        want = _expected(scores, gt, ex, hard_skip, num_hard)
        for b in range(B):
            row = mined[b].tolist()
            valid = [n for n in row if n >= 0]
            assert valid == want[b], (b, ex is not None)
            assert int(gt[b]) not in valid
            if ex is not None:
                assert not set(valid) & (set(ex[b]) - {int(gt[b])})
            # the tail of a short list is -1; elsewhere only the ground truth's own place is
            n_cand = N - (len(set(ex[b]) - {int(gt[b])}) if ex is not None else 0)
            filled = max(0, min(num_hard, n_cand - hard_skip))
            assert all(n == -1 for n in row[filled:]) and sum(n == -1 for n in row[:filled]) <= 1
    if N == 129:
        assert filled < num_hard, "the first shape must come out short"
    # a tensor of seen items padded with -1 is the same exclusion
    E = max(len(r) for r in exclude)
    padded = torch.tensor([r + [-1] * (E - len(r)) for r in exclude])
    assert torch.equal(cc.mine(user, gt, padded), cc.mine(user, gt, exclude))


# ---- 3. / 4. the loss and the step on an index batch
def _joint_case():
    from tests.test_gpu_grad_clip import _inputs, _joint
    case, model = _joint()
    return case, model, _inputs(case)


def _catalogue(batch, dtype=F32, extra=25):
    """A catalogue of the case's positives and negatives (then `extra` random rows) and the index batch over it."""
    pos, neg = batch["positive_item_embeddings"], batch["negative_item_embeddings"]
    B, P, D = neg.shape
    g = torch.Generator().manual_seed(5)
    rows = [neg.reshape(B * P, D), pos] + ([torch.randn(extra, D, generator=g).to(DEV)] if extra else [])
    cat = torch.cat(rows).to(dtype).contiguous()
    neg_index = torch.arange(B * P, device=DEV).view(B, P)
    pos_index = B * P + torch.arange(B, device=DEV)
    return cat, pos_index, neg_index


def _index_batch(batch, pos_index, neg_index, **more):
    out = {k: v for k, v in batch.items() if k not in ("positive_item_embeddings", "negative_item_embeddings")}
    out.update(positive_item_index=pos_index, negative_item_index=neg_index, **more)
    return out


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_loss_identity(dtype):
    from tests.golden import cases
    from tests.test_gpu_grad_clip import _inputs
    from unirec_amd.joint import InfoNCELoss
    from unirec_amd.negatives import CatalogCandidates
    case = cases.ALL["joint_left"]
    batch = _inputs(case)
    cat, pos_index, neg_index = _catalogue(batch, dtype)
    neg_index = neg_index.clone()
    neg_index[1, 2] = -1                                                  # a padded column
    nmask = batch["negative_masks"]
    user = torch.randn(case["B"], case["D"], generator=torch.Generator().manual_seed(9)).to(DEV)
    cc = CatalogCandidates(cat)
    ua, ub = user.clone().requires_grad_(True), user.clone().requires_grad_(True)
    pos, neg, mask, index = cc.candidates(ua, pos_index, neg_index, nmask)
    assert pos.dtype == F32 and neg.dtype == F32 and mask.dtype == torch.uint8 and index.dtype == torch.int64
    want_mask = ((neg_index >= 0) & (nmask != 0)).to(torch.uint8)
    assert torch.equal(mask, want_mask) and torch.equal(index, torch.where(want_mask.bool(), neg_index, torch.full_like(neg_index, -1)))
    assert cc.last_index is index and cc.last_mask is mask
    loss_fn = InfoNCELoss(0.07)
    la = loss_fn(ua, pos, neg, mask)
    la.backward()
    tneg = torch.where(want_mask.bool()[..., None], cat[neg_index.clamp(min=0)].float(), torch.zeros((), device=DEV))
    lb = loss_fn(ub, cat[pos_index].float(), tneg, want_mask)
    lb.backward()
    assert torch.isfinite(la) and torch.equal(_bits(la.detach()), _bits(lb.detach()))
    assert torch.equal(_bits(ua.grad), _bits(ub.grad)) and float(ua.grad.abs().max()) > 0


def _args(**over):
    kw = dict(learning_rate=1e-3, warmup_steps=1, max_steps=4, max_grad_norm=1.0, weight_decay=0.01, logging_steps=0)
    kw.update(over)
    return types.SimpleNamespace(**kw)


def test_trainer_identity():
    from unirec_amd.joint import JointTrainer
    from unirec_amd.negatives import CatalogCandidates
    case, ma, batch = _joint_case()
    _, mb, _ = _joint_case()
    cat, pos_index, neg_index = _catalogue(batch)
    ibatch = _index_batch(batch, pos_index, neg_index)
    ebatch = dict(batch, positive_item_embeddings=cat[pos_index], negative_item_embeddings=cat[neg_index])
    ta = JointTrainer(ma, _args(), negatives=CatalogCandidates(cat))
    tb = JointTrainer(mb, _args())
    before = [p.master.clone() for p in ta.packs]
    for step in range(2):
        la, lb = ta.training_step(ibatch), tb.training_step(ebatch)
        assert torch.isfinite(la) and torch.equal(_bits(la), _bits(lb)), step
        for pa, pb in zip(ta.packs, tb.packs):
            assert torch.equal(pa.master, pb.master), step
    assert any(not torch.equal(p.master, b) for p, b in zip(ta.packs, before))
    # a trainer that holds a catalogue takes an embedding batch exactly as one that holds none
    lc = ta.training_step(ebatch)
    ld = tb.training_step(ebatch)
    assert torch.equal(_bits(lc), _bits(ld))


# ---- 5. random and mined negatives in the step
def test_random_and_mined_negatives_in_the_step():
    from unirec_amd import hip
    from unirec_amd.joint import JointTrainer
    from unirec_amd.negatives import CatalogCandidates
    runs = []
    for _ in range(2):
        case, model, batch = _joint_case()
        cat, pos_index, neg_index = _catalogue(batch, BF16, extra=200)
        N, B, Pe = cat.shape[0], neg_index.shape[0], neg_index.shape[1]
        seen = [[int(pos_index[0]), 3, 30], [], [int(neg_index[2, 0]), 100, 101, 150]]
        ibatch = _index_batch(batch, pos_index, neg_index, seen_item_index=seen)
        cc = CatalogCandidates(cat, num_random=8, num_hard=4, hard_skip=1, seed=3)
        tr = JointTrainer(model, _args(warmup_steps=0), negatives=cc)       # no warm-up: the first step's rate is not zero
        before = [p.master.clone() for p in tr.packs]
        seen_user, inner = [], tr.loss_fn.compute_loss

        def spy(model, inputs, return_outputs=False, **kw):                      # the step's own user embeddings, dropout as it draws it
            loss, user = inner(model, inputs, return_outputs=True, **kw)
            seen_user.append(user.detach().clone())
            return (loss, user) if return_outputs else loss
        tr.loss_fn.compute_loss = spy
        loss = tr.training_step(ibatch)
        user, index0, mask0 = seen_user[0], cc.last_index.clone(), cc.last_mask.clone()
        assert torch.isfinite(loss)
        assert any(not torch.equal(p.master, b) for p, b in zip(tr.packs, before)), "the step moves the weights"
        runs.append((loss, index0, mask0))
        # the mask rule against this step's own user embeddings
        assert index0.shape == (B, Pe + 8 + 4)
        scores, _ = hip.catalog_scores(user.detach().float().contiguous(), cat.float())
        want_mined = _expected(scores, pos_index.tolist(), seen, 1, 4)
        rand = cc.sample(B, 0, 0)
        nmask = batch["negative_masks"]
        for b in range(B):
            row, m = index0[b].tolist(), mask0[b].tolist()
            mined = row[Pe + 8:]
            assert [n for n in mined if n >= 0] == want_mined[b], b
            assert m[Pe + 8:] == [int(n >= 0) for n in mined]
            for j in range(Pe):
                ok = int(neg_index[b, j]) >= 0 and int(nmask[b, j]) != 0
                assert m[j] == int(ok) and row[j] == (int(neg_index[b, j]) if ok else -1)
            for j, r in enumerate(rand[b].tolist()):
                ok = r != int(pos_index[b]) and r not in seen[b] and r not in mined
                assert m[Pe + j] == int(ok) and row[Pe + j] == (r if ok else -1), (b, j)
            assert 0 <= min(rand[b].tolist()) and max(rand[b].tolist()) < N
        # the next step draws other random negatives
        tr.training_step(ibatch)
        assert not torch.equal(cc.sample(B, 1, 0), rand)
        assert torch.equal(torch.where(cc.last_mask[:, Pe:Pe + 8].bool(), cc.sample(B, 1, 0), torch.full_like(rand, -1)), cc.last_index[:, Pe:Pe + 8])
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])


# ---- 6. shard invariance
def test_shard_invariance():
    from unirec_amd.negatives import CatalogCandidates
    g = torch.Generator().manual_seed(21)
    N, D, B = 300, 64, 6
    cat = torch.randn(N, D, generator=g).to(BF16).to(DEV)
    user = torch.randn(B, D, generator=g).to(DEV)
    pos_index = torch.randint(0, N, (B,), generator=g).to(DEV)
    neg_index = torch.randint(-1, N, (B, 3), generator=g).to(DEV)
    seen = [[int(pos_index[b]), b, 2 * b + 50] for b in range(B)]
    cc = CatalogCandidates(cat, num_random=40, num_hard=5, hard_skip=2, seed=1)
    pos, neg, mask, index = cc.candidates(user, pos_index, neg_index, exclude=seen, step=7, first_sample=0)
    assert neg.shape == (B, 48, D)
    parts = [cc.candidates(user[lo:lo + 3], pos_index[lo:lo + 3], neg_index[lo:lo + 3], exclude=seen[lo:lo + 3], step=7, first_sample=lo)
             for lo in (0, 3)]
    for k, whole in enumerate((pos, neg, mask, index)):
        assert torch.equal(whole, torch.cat([p[k] for p in parts])), k
    # keyed on the global sample index: the second shard with first_sample 0 would draw the first shard's random negatives
    again = cc.candidates(user[3:], pos_index[3:], neg_index[3:], exclude=seen[3:], step=7, first_sample=0)
    assert not torch.equal(again[3], parts[1][3])
    # the gathered rows are the catalogue's, widened; masked columns are zero rows
    want = torch.where((index >= 0)[..., None], cat[index.clamp(min=0)].float(), torch.zeros((), device=DEV))
    assert torch.equal(_bits(neg), _bits(want)) and torch.equal(mask, (index >= 0).to(torch.uint8))

"""GPU: the Matryoshka loss through the joint surface (InfoNCELoss / MultiModalTrainer / JointTrainer with matryoshka_dims, mrr_ranks and
MRREvaluator.ranks_from_embeddings with dims, CatalogEvaluator.truncated) on the smallest joint model the joint tests build
(tests/golden/cases.py joint_left: B 3, 7 negatives, D 256).  The kernels themselves are held to float64 in tests/test_gpu_mrl_f64.py."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import mrl_ref, ref64  # noqa: E402
from tests.test_gpu_negatives import _catalogue, _index_batch, _joint_case  # noqa: E402

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
DIMS = (32, 64, 128, 256)
WEIGHTS = (0.5, 0.0, 2.0, 1.0)
TAU = 0.07


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _args(**over):
    kw = dict(learning_rate=1e-3, warmup_steps=0, max_steps=4, max_grad_norm=1.0, weight_decay=0.01, logging_steps=1)
    kw.update(over)
    return types.SimpleNamespace(**kw)


def _loss_and_user_grad(trainer, model, batch):
    """(loss, the user embeddings of the forward, the gradient that reaches them, the LoRA pack's gradient)"""
    seen = {}
    loss, user = trainer.compute_loss(model, batch, return_outputs=True)
    user.register_hook(lambda g: seen.setdefault("g", g.detach().clone()))
    loss.backward()                                             # (a fresh model: its packs' gradients start at zero)
    pack = model.base_model._ensure_pack(user.device)
    return loss.detach(), user.detach(), seen["g"], pack.grad.clone()


def test_default_path_is_unchanged():
    from unirec_amd.joint import MultiModalTrainer
    case, ma, batch = _joint_case()
    _, mb, _ = _joint_case()
    la, ua, ga, pa = _loss_and_user_grad(MultiModalTrainer(), ma, batch)
    lb, ub, gb, pb = _loss_and_user_grad(MultiModalTrainer(matryoshka_dims=None, matryoshka_weights=None), mb, batch)
    assert torch.isfinite(la) and torch.equal(_bits(la), _bits(lb)) and torch.equal(_bits(ua), _bits(ub))
    assert torch.equal(_bits(ga), _bits(gb)) and torch.equal(_bits(pa), _bits(pb)) and float(pa.abs().max()) > 0


def test_loss_with_dims_against_float64_and_the_gradient_that_reaches_the_user_embeddings():
    from unirec_amd import hip
    from unirec_amd.joint import MultiModalTrainer
    case, model, batch = _joint_case()
    tr = MultiModalTrainer(TAU, matryoshka_dims=DIMS, matryoshka_weights=WEIGHTS)
    seen = {}
    loss, user = tr.compute_loss(model, batch, return_outputs=True)
    user.register_hook(lambda g: seen.setdefault("g", g.detach().clone()))
    (loss * 3.0).backward()                                     # an upstream scalar that is not 1
    planes = tr.infonce_loss.last_plane_loss
    assert planes.shape == (len(DIMS),) and planes.is_cuda
    u = user.detach().float().cpu()
    pos, neg, mask = (batch[k].cpu() for k in ("positive_item_embeddings", "negative_item_embeddings", "negative_masks"))
    tau32 = float(torch.tensor(TAU, dtype=F32))
    l64, pl64, _ = mrl_ref.infonce(u, pos, neg, mask, DIMS, WEIGHTS, tau32)
    l32, pl32, _ = mrl_ref.infonce(u, pos, neg, mask, DIMS, WEIGHTS, tau32, dtype=F32)
    ref64.assert_f32_close(loss.detach().cpu().reshape(()), l64, l32, scale=abs(float(l64)) + 1.0, what="matryoshka loss of the joint model")
    for k in range(len(DIMS)):
        ref64.assert_f32_close(planes[k].cpu().reshape(()), pl64[k], pl32[k], scale=abs(float(pl64[k])) + 1.0, what=f"plane_loss[{k}]")
    # the gradient at the user embeddings = the kernel's d_user on those embeddings, times the upstream scalar
    ud = user.detach().float().contiguous()
    _, _, du, _, _ = hip.mrl_infonce(ud, batch["positive_item_embeddings"].float().contiguous(), batch["negative_item_embeddings"].float().contiguous(),
                                     batch["negative_masks"].to(torch.uint8).contiguous(), DIMS, WEIGHTS, TAU, 1.0)
    assert seen["g"].shape == du.shape and torch.equal(_bits(seen["g"].float()), _bits(du * 3.0)) and float(du.abs().max()) > 0


def test_index_batch_gives_the_embedding_batch_loss():
    from unirec_amd.joint import MultiModalTrainer
    from unirec_amd.negatives import CatalogCandidates
    case, ma, batch = _joint_case()
    _, mb, _ = _joint_case()
    cat, pos_index, neg_index = _catalogue(batch)
    ibatch = _index_batch(batch, pos_index, neg_index)
    ebatch = dict(batch, positive_item_embeddings=cat[pos_index], negative_item_embeddings=cat[neg_index])
    ta = MultiModalTrainer(TAU, negatives=CatalogCandidates(cat), matryoshka_dims=DIMS, matryoshka_weights=WEIGHTS)
    tb = MultiModalTrainer(TAU, matryoshka_dims=DIMS, matryoshka_weights=WEIGHTS)
    la, _, ga, pa = _loss_and_user_grad(ta, ma, ibatch)
    lb, _, gb, pb = _loss_and_user_grad(tb, mb, ebatch)
    assert torch.isfinite(la) and torch.equal(_bits(la), _bits(lb)) and torch.equal(_bits(ga), _bits(gb)) and torch.equal(_bits(pa), _bits(pb))
    assert torch.equal(_bits(ta.infonce_loss.last_plane_loss), _bits(tb.infonce_loss.last_plane_loss))
    # and it is not the plain loss
    lc, _, _, _ = _loss_and_user_grad(MultiModalTrainer(TAU), _joint_case()[1], ebatch)
    assert not torch.equal(_bits(la), _bits(lc))


def test_joint_trainer_step_logs_plane_loss_and_moves_the_adapters():
    from unirec_amd.joint import JointTrainer
    case, model, batch = _joint_case()
    tr = JointTrainer(model, _args(), matryoshka_dims=DIMS, matryoshka_weights=WEIGHTS)
    before = tr.lpack.master.clone()
    loss = tr.training_step(batch)
    assert torch.isfinite(loss) and not torch.equal(tr.lpack.master, before), "the step moves the LoRA parameters"
    rec = tr.state.log_history[-1]
    assert rec["step"] == 1 and len(rec["plane_loss"]) == len(DIMS) and all(v == v and v > 0 for v in rec["plane_loss"])
    planes = tr.loss_fn.infonce_loss.last_plane_loss.cpu().tolist()
    assert rec["plane_loss"] == pytest.approx(planes, rel=1e-6)
    assert rec["loss"] == pytest.approx(sum(w * p for w, p in zip(WEIGHTS, planes)), rel=1e-5)
    # a trainer without dims logs what it always logged
    _, m2, _ = _joint_case()
    t2 = JointTrainer(m2, _args())
    t2.training_step(batch)
    assert "plane_loss" not in t2.state.log_history[-1]


def test_ranks_per_prefix_equal_the_ranks_on_slices():
    from unirec_amd.evaluation import MRREvaluator
    from unirec_amd.joint import mrr_ranks
    g = torch.Generator().manual_seed(21)
    B, N, D = 6, 41, 256
    u, p, n = torch.randn(B, D, generator=g).to(DEV), torch.randn(B, D, generator=g).to(DEV), torch.randn(B, N, D, generator=g).to(DEV)
    m = (torch.rand(B, N, generator=g) > 0.3).to(DEV)
    scores, ranks = mrr_ranks(u, p, n, m, dims=DIMS)
    assert scores.shape == (len(DIMS), B, N + 1) and ranks.shape == (len(DIMS), B) and ranks.dtype == torch.int32
    for k, d in enumerate(DIMS):
        sk, rk = mrr_ranks(u[:, :d], p[:, :d], n[..., :d], m)
        assert torch.equal(_bits(scores[k]), _bits(sk)) and torch.equal(ranks[k], rk), d
    assert len({tuple(r.tolist()) for r in ranks}) > 1, "the prefixes rank differently on random vectors"
    ragged = [n[b, :N - 3 * b] for b in range(B)]
    rr = MRREvaluator.ranks_from_embeddings(u, p, ragged, dims=DIMS)
    for k, d in enumerate(DIMS):
        assert torch.equal(rr[k], MRREvaluator.ranks_from_embeddings(u[:, :d], p[:, :d], [x[:, :d] for x in ragged])), d


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_truncated_evaluator_is_a_fresh_evaluator_over_the_prefix(dtype):
    from unirec_amd.evaluation import CatalogEvaluator
    g = torch.Generator().manual_seed(22)
    Ncat, D, B, k = 3000, 512, 5, 10
    cat = torch.randn(Ncat, D, generator=g)
    u = torch.randn(B, D, generator=g).to(DEV)
    gt = torch.randint(0, Ncat, (B,), generator=g)
    ev = CatalogEvaluator(cat, dtype=dtype)
    ev.retrieve(u, k)                                           # the wide evaluator has its norms: the narrow one must not inherit them
    tr = ev.truncated(256)
    fresh = CatalogEvaluator(ev.catalog[:, :256].contiguous(), dtype=dtype)
    assert tr._inv is None and tr.catalog.shape == (Ncat, 256) and tr.catalog.dtype == dtype and tr.catalog.is_contiguous()
    a = tr.retrieve(u[:, :256], k, gt_index=gt, exclude=[[1, 2], [], [5], [], [7, 8, 9]])
    b = fresh.retrieve(u[:, :256].contiguous(), k, gt_index=gt, exclude=[[1, 2], [], [5], [], [7, 8, 9]])
    assert torch.equal(a["topk_index"], b["topk_index"]) and torch.equal(_bits(a["topk_score"]), _bits(b["topk_score"]))
    assert torch.equal(a["rank"], b["rank"]) and a["mrr"] == b["mrr"]
    assert not torch.equal(a["topk_index"], ev.retrieve(u, k)["topk_index"])
    if dtype == torch.float32:
        ea, eb = tr.evaluate(u[:, :256], gt, k), fresh.evaluate(u[:, :256].contiguous(), gt, k)
        assert torch.equal(ea["rank"], eb["rank"]) and torch.equal(ea["topk_index"], eb["topk_index"]) and torch.equal(_bits(ea["topk_score"]), _bits(eb["topk_score"]))

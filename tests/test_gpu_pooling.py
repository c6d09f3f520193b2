"""GPU, model level: the pooling rules "masked_mean" and "last" through Qwen3LoRAModel / MultiModalQwenEmbedding, held to
tests/parity_utils.OUT_REL (outputs) and GRAD_REL (gradients):
  * the fixture tests/golden/pool_tiny.npz (transformers.Qwen3Model + the reference's own last_token_pool; the masked mean is the
    generator's: that rule is pinned by the oracle alone): pooled vectors and the gradient with respect to inputs_embeds, both rules,
    both padding sides, on a model without adapters;
  * joint_left / joint_right with the item Q-Former, injection, adapters and InfoNCE against the oracle composition with
    tests/pool_ref.pool in place of .mean(dim=1): user embeddings, query_embeddings.grad, EVERY LoRA A / B gradient;
  * padding invariance: the same batch with 16 more pad columns gives the same embeddings under both rules (the float32 oracle alone
    moves by 5e-7 there; under "mean" by 0.2 / 0.43);
  * merged and unmerged evaluation under "last" agree; pooling="mean" and an absent keyword give identical bits;
  * a JointTrainer step under "last" runs and launches neither mean_pool_fwd nor mean_pool_bwd."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import qformer_ref as R  # noqa: E402
from oracle import qwen3_ref as Q  # noqa: E402
from oracle import weights as W  # noqa: E402
from tests import pool_ref  # noqa: E402
from tests.golden import cases  # noqa: E402
from tests.parity_utils import GRAD_REL, OUT_REL, assert_close, load_generated, load_golden, rel_err  # noqa: E402
from tests.test_gpu_joint import _qwen_cfg  # noqa: E402

DEV = "cuda"
JOINT = ("joint_left", "joint_right")
MODES = pool_ref.MODES


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _build_joint(case, use_lora, pooling=None, lora_seed=None):
    """tests/test_gpu_joint._build_joint with the pooling keyword"""
    from unirec_amd.joint import MultiModalQwenEmbedding
    from unirec_amd.qformer_model import QFormerForItemRepresentation
    c = case["cfg"]
    qc = cases.qwen_cfg(case)
    cfg = R.QFormerCfg(c["H"], c["L"], c["nh"], c["I"], c["Q"], c["E"], 2)
    qf = QFormerForItemRepresentation(hidden_size=c["H"], num_hidden_layers=c["L"], num_attention_heads=c["nh"], intermediate_size=c["I"],
                                      num_query_tokens=c["Q"], field_embedding_dim=c["E"], num_fields=c["F"], dropout=0.0)
    qf = load_generated(qf, R.item_qformer_shapes(cfg, c["F"]), case["seed"])
    hc = _qwen_cfg(qc, use_lora)
    hc.vocab_size = case["first_special_id"]
    kw = {} if pooling is None else {"pooling": pooling}
    m = MultiModalQwenEmbedding(qformer_model=qf, use_lora=use_lora, qwen_config=hc, num_history_items=case["hist"],
                                num_query_tokens_per_item=c["Q"], **kw)
    sd = {k: torch.from_numpy(v) for k, v in W.fill_state_dict(Q.qwen3_shapes(qc, lora=False), case["seed"] + 1).items()}
    missing, unexpected = m.base_model.load_state_dict(sd, strict=False)
    assert not unexpected
    if use_lora:
        lsd = {k: torch.from_numpy(v) for k, v in W.fill_state_dict(
            {k: s for k, s in Q.qwen3_shapes(qc, lora=True).items() if ".lora_" in k}, lora_seed).items()}
        m.base_model.load_state_dict(lsd, strict=False)
    return m.to(DEV).train(), qf


def _more_padding(case, extra=16):
    """the batch of `case` with `extra` more pad columns on its padding side"""
    ids, am, hfe, ham, pos, neg, nmask = cases.joint_inputs(case)
    B = ids.shape[0]
    pad_i, pad_m = np.zeros((B, extra), dtype=ids.dtype), np.zeros((B, extra), dtype=am.dtype)
    if case["pad_side"] == "left":
        return np.concatenate([pad_i, ids], 1), np.concatenate([pad_m, am], 1), hfe, ham
    return np.concatenate([ids, pad_i], 1), np.concatenate([am, pad_m], 1), hfe, ham


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("side", sorted(pool_ref.POOL_CASES))
def test_pooled_vectors_and_input_gradient_match_the_fixture(side, mode):
    """The decoder alone (use_lora=False).  inputs_embeds enters as injected tokens -- position s of every sample holds the special id
    s, so the whole input is the [B,S,D] token tensor and its gradient is the gradient with respect to inputs_embeds."""
    from unirec_amd.qwen3 import Qwen3LoRAModel
    case = pool_ref.POOL_CASES[side]
    g = load_golden("pool_tiny")
    qc = cases.qwen_cfg(case)
    hc = _qwen_cfg(qc, False)
    hc.pooling = mode
    m = load_generated(Qwen3LoRAModel(hc, use_lora=False), Q.qwen3_shapes(qc, lora=False), case["seed"] + 1)
    assert m.pooling == mode
    x, am, r = pool_ref.pool_case_inputs(side)
    B, S, D = x.shape
    ids = torch.arange(S, device=DEV).expand(B, S).contiguous()
    tok = _t(x).to(torch.bfloat16).requires_grad_(True)
    pooled = m.forward_pooled(ids, _t(am), tok, 0)
    (pooled * _t(r)).sum().backward()
    print(side, mode)
    assert_close(pooled, g[f"{side}/{mode}/pooled"], OUT_REL, "pooled")
    assert_close(tok.grad, g[f"{side}/{mode}/grad_inputs_embeds"], GRAD_REL, "grad_inputs_embeds")
    assert float(tok.grad[_t(am) == 0].abs().max()) == 0.0, "padding receives no gradient"


# ---- the joint model against the oracle composition ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_joint(name, mode):
    """(user [B,D], d query_embeddings, {lora name: grad}) of the float32 oracle with pool_ref.pool in place of .mean(dim=1); computed
    once per (case, rule) and left unchanged"""
    case = cases.ALL[name]
    c, qc = case["cfg"], cases.qwen_cfg(case)
    cfg = R.QFormerCfg(c["H"], c["L"], c["nh"], c["I"], c["Q"], c["E"], 2)
    PQ = {k: torch.from_numpy(v).requires_grad_(True) for k, v in W.fill_state_dict(R.item_qformer_shapes(cfg, c["F"]), case["seed"]).items()}
    PW = {k: torch.from_numpy(v) for k, v in W.fill_state_dict(Q.qwen3_shapes(qc, lora=False), case["seed"] + 1).items()}
    lsh = {k: s for k, s in Q.qwen3_shapes(qc, lora=True).items() if ".lora_" in k}
    PL = {k: torch.from_numpy(v).requires_grad_(True) for k, v in W.fill_state_dict(lsh, case["seed"] + 2).items()}
    ids, am, hfe, ham, pos, neg, nmask = cases.joint_inputs(case)
    B, hist = case["B"], case["hist"]
    out = R.item_qformer_forward(PQ, cfg, torch.from_numpy(hfe).view(B * hist, c["F"], c["E"]), torch.from_numpy(ham).view(B * hist, c["F"]))
    toks = out["query_outputs"].view(B, hist, c["Q"], c["H"])
    P = {**PW, **PL}
    text = Q.inject_tokens(P["embed_tokens.weight"][torch.from_numpy(ids)], torch.from_numpy(ids), toks, case["first_special_id"])
    h = Q.qwen3_forward(P, qc, text, torch.from_numpy(am))
    user = pool_ref.pool(h, torch.from_numpy(am), mode)
    loss = Q.infonce_loss(user, torch.from_numpy(pos), torch.from_numpy(neg), torch.from_numpy(nmask))
    loss.backward()
    return user.detach().numpy(), float(loss.detach()), PQ["query_embeddings"].grad.numpy(), {k: v.grad.numpy() for k, v in PL.items()}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", JOINT)
def test_joint_with_lora_matches_oracle_with_pool_ref(name, mode):
    from unirec_amd.joint import InfoNCELoss
    case = cases.ALL[name]
    m, qf = _build_joint(case, use_lora=True, pooling=mode, lora_seed=case["seed"] + 2)
    ids, am, hfe, ham, pos, neg, nmask = cases.joint_inputs(case)
    user = m(_t(ids), _t(am), _t(hfe), _t(ham))
    loss = InfoNCELoss()(user, _t(pos), _t(neg), _t(nmask))
    loss.backward()
    ou, ol, dq, dl = _oracle_joint(name, mode)
    print(name, mode)
    assert_close(user, ou, OUT_REL, "user_embeddings")
    assert_close(loss, np.asarray(ol), OUT_REL, "loss")
    assert_close(dict(qf.named_parameters())["query_embeddings"].grad, dq, GRAD_REL, "grad/query_embeddings")
    named = dict(m.base_model.named_parameters())
    assert len(dl) == 2 * 7 * 2
    for k in sorted(dl):
        assert_close(named[k].grad, dl[k], GRAD_REL, "grad/" + k)
    assert named["layers.0.self_attn.q_proj.weight"].grad is None      # base weights are frozen


@pytest.mark.parametrize("name", JOINT)
def test_embeddings_do_not_depend_on_the_padded_length(name):
    """S 48 -> 64 on the case's padding side: both rules within OUT_REL (the measured values are printed; the float32 oracle moves by
    <= 5e-7), on every plan an evaluation takes here: adapters, merged operands, no adapters.  The default rule does move -- by more
    than OUT_REL, which is what the new rules are for."""
    case = cases.ALL[name]
    ids, am, hfe, ham = cases.joint_inputs(case)[:4]
    ids2, am2, _, _ = _more_padding(case)
    assert ids2.shape[1] == ids.shape[1] + 16
    for use_lora in (True, False):
        for mode in MODES + ("mean",):
            m, _ = _build_joint(case, use_lora=use_lora, pooling=mode, lora_seed=case["seed"] + 2)
            m.eval()
            plans = ("adapters", "merged") if use_lora else ("no adapters",)
            for plan in plans:
                if plan == "merged":
                    m.merge_adapter()
                with torch.no_grad():
                    u48 = m(_t(ids), _t(am), _t(hfe), _t(ham)).cpu().numpy()
                    u64 = m(_t(ids2), _t(am2), _t(hfe), _t(ham)).cpu().numpy()
                e = rel_err(u64, u48)
                print(f"  {name} {mode} ({plan}): relative change of the embeddings under 16 more pad columns = {e:.3e}")
                if mode == "mean":
                    assert e > OUT_REL, "the default rule is expected to depend on the padded length"
                else:
                    assert e <= OUT_REL, f"{name} {mode} ({plan}): {e:.3e} > {OUT_REL}"


def test_merged_and_unmerged_evaluation_agree_under_last():
    case = cases.ALL["joint_left"]
    m, _ = _build_joint(case, use_lora=True, pooling="last", lora_seed=case["seed"] + 2)
    m.eval()
    ids, am, hfe, ham = cases.joint_inputs(case)[:4]
    with torch.no_grad():
        u0 = m(_t(ids), _t(am), _t(hfe), _t(ham))
        m.merge_adapter()
        u1 = m(_t(ids), _t(am), _t(hfe), _t(ham))
        m.unmerge_adapter()
        u2 = m(_t(ids), _t(am), _t(hfe), _t(ham))
    assert_close(u1, u0.cpu().numpy(), OUT_REL, "merged against unmerged user_embeddings")
    assert torch.equal(u0, u2)
    assert_close(u0, _oracle_joint("joint_left", "last")[0], OUT_REL, "user_embeddings (eval)")


def test_mean_keyword_and_absent_keyword_give_identical_bits(monkeypatch):
    """the default rule is today's code path: the same launches (mean_pool_fwd / mean_pool_bwd, never pool_norm_*) and the same bits"""
    from unirec_amd import hip
    from unirec_amd.joint import InfoNCELoss
    calls = []
    for fn in ("mean_pool_fwd", "mean_pool_bwd", "pool_norm_fwd", "pool_norm_bwd"):
        monkeypatch.setattr(hip, fn, (lambda f, n: lambda *a, **k: (calls.append(n), f(*a, **k))[1])(getattr(hip, fn), fn))
    case = cases.ALL["joint_left"]
    ids, am, hfe, ham, pos, neg, nmask = cases.joint_inputs(case)
    res = []
    for pooling in (None, "mean"):
        m, qf = _build_joint(case, use_lora=True, pooling=pooling, lora_seed=case["seed"] + 2)
        assert m.base_model.pooling == "mean"
        user = m(_t(ids), _t(am), _t(hfe), _t(ham))
        InfoNCELoss()(user, _t(pos), _t(neg), _t(nmask)).backward()
        res.append((user.detach().clone(), {k: p.grad.detach().clone() for k, p in m.base_model.named_parameters() if p.grad is not None},
                    qf.query_embeddings.grad.detach().clone()))
    assert "pool_norm_fwd" not in calls and "pool_norm_bwd" not in calls
    assert "mean_pool_fwd" in calls and "mean_pool_bwd" in calls
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][2], res[1][2])
    assert res[0][1].keys() == res[1][1].keys() and len(res[0][1]) == 2 * 7 * 2
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k


def test_joint_trainer_step_under_last_launches_no_mean_pool(tmp_path, monkeypatch):
    from transformers import TrainingArguments
    from tests.test_gpu_grad_clip import _inputs as joint_batch
    from unirec_amd import hip
    from unirec_amd.joint import JointTrainer
    calls = []
    for fn in ("mean_pool_fwd", "mean_pool_bwd", "pool_norm_fwd", "pool_norm_bwd"):
        monkeypatch.setattr(hip, fn, (lambda f, n: lambda *a, **k: (calls.append(n), f(*a, **k))[1])(getattr(hip, fn), fn))
    case = dict(cases.ALL["joint_left"], drop_one_special=False)
    model, _ = _build_joint(case, use_lora=True, pooling="last", lora_seed=case["seed"] + 2)
    tr = JointTrainer(model, TrainingArguments(output_dir=str(tmp_path), learning_rate=1e-4, max_steps=2, report_to=[]))
    batch = joint_batch(case)
    before = {n: p.detach().clone() for n, p in model.base_model.lora_named_parameters()}
    l0 = tr.training_step(batch)
    l1 = tr.training_step(batch)
    assert bool(torch.isfinite(l0)) and bool(torch.isfinite(l1))
    # the item Q-Former pools its query tokens with mean_pool_* only in its own heads, which the joint step does not run
    assert calls.count("pool_norm_fwd") == 2 and calls.count("pool_norm_bwd") == 2, calls
    assert "mean_pool_fwd" not in calls and "mean_pool_bwd" not in calls, calls
    assert any(not torch.equal(p.detach(), before[n]) for n, p in model.base_model.lora_named_parameters()), "the step moved no adapter"

"""GPU parity: Qwen3(+LoRA) decoder, token injection, mean-pool, InfoNCE and MRR on the HIP path vs
golden vectors produced by the installed transformers Qwen3Model + the reference's joint module."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import qformer_ref as R  # noqa: E402
from oracle import qwen3_ref as Q  # noqa: E402
from oracle import weights as W  # noqa: E402
from tests.golden import cases  # noqa: E402
from tests.parity_utils import GRAD_REL, OUT_REL, assert_close, grad_scale, load_generated, load_golden  # noqa: E402

DEV = "cuda"
JOINT = [n for n, c in cases.ALL.items() if c["kind"] == "joint"]
QWEN = [n for n, c in cases.ALL.items() if c["kind"] == "qwen"]


def _qwen_cfg(qc, lora):
    from unirec_amd.qwen3 import Qwen3Config
    return Qwen3Config(vocab_size=qc.vocab_size, hidden_size=qc.hidden_size, intermediate_size=qc.intermediate_size,
                       num_hidden_layers=qc.num_hidden_layers, num_attention_heads=qc.num_attention_heads,
                       num_key_value_heads=qc.num_key_value_heads, head_dim=qc.head_dim, rms_norm_eps=qc.rms_norm_eps,
                       rope_theta=qc.rope_theta, lora_r=qc.lora_r, lora_alpha=qc.lora_alpha, lora_dropout=0.0)


def _build_joint(case, use_lora, lora_seed=None):
    from unirec_amd.joint import MultiModalQwenEmbedding
    from unirec_amd.qformer_model import QFormerForItemRepresentation
    c = case["cfg"]
    qc = cases.qwen_cfg(case)
    cfg = R.QFormerCfg(c["H"], c["L"], c["nh"], c["I"], c["Q"], c["E"], 2)
    qf = QFormerForItemRepresentation(hidden_size=c["H"], num_hidden_layers=c["L"], num_attention_heads=c["nh"],
                                      intermediate_size=c["I"], num_query_tokens=c["Q"], field_embedding_dim=c["E"],
                                      num_fields=c["F"], dropout=0.0)
    qf = load_generated(qf, R.item_qformer_shapes(cfg, c["F"]), case["seed"])
    hc = _qwen_cfg(qc, use_lora)
    hc.vocab_size = case["first_special_id"]        # specials are appended after the base vocabulary
    m = MultiModalQwenEmbedding(qformer_model=qf, use_lora=use_lora, qwen_config=hc, num_history_items=case["hist"],
                                num_query_tokens_per_item=c["Q"])
    assert m.first_special_id == case["first_special_id"]
    shapes = Q.qwen3_shapes(qc, lora=False)
    sd = {k: torch.from_numpy(v) for k, v in W.fill_state_dict(shapes, case["seed"] + 1).items()}
    missing, unexpected = m.base_model.load_state_dict(sd, strict=False)
    assert not unexpected
    if use_lora:
        lsd = {k: torch.from_numpy(v) for k, v in W.fill_state_dict(
            {k: s for k, s in Q.qwen3_shapes(qc, lora=True).items() if ".lora_" in k}, lora_seed).items()}
        m.base_model.load_state_dict(lsd, strict=False)
    return m.to(DEV).train(), qf


@pytest.mark.parametrize("name", QWEN)
def test_qwen3_decoder_matches_transformers(name):
    from unirec_amd.qwen3 import Qwen3LoRAModel
    case = cases.ALL[name]
    g = load_golden(name)
    qc = cases.qwen_cfg(case)
    m = Qwen3LoRAModel(_qwen_cfg(qc, False), use_lora=False)
    m = load_generated(m, Q.qwen3_shapes(qc, lora=False), case["seed"] + 1)
    x, am = cases.qwen_inputs(case)
    # feed inputs_embeds through the embedding table: vocabulary = the B*S input rows
    B, S, D = x.shape
    m.embed_tokens.weight = torch.nn.Parameter(torch.from_numpy(x.reshape(B * S, D)).to(DEV), requires_grad=False)
    m.config.vocab_size = B * S
    ids = torch.arange(B * S, device=DEV).view(B, S)
    pooled = m.forward_pooled(ids, torch.from_numpy(am).to(DEV))
    want = g["sdpa/last_hidden_state"].mean(axis=1)
    print(name)
    assert_close(pooled, want, OUT_REL, "mean-pooled last_hidden_state (sdpa semantics)")


@pytest.mark.parametrize("name", JOINT)
def test_joint_matches_reference(name):
    from unirec_amd.joint import InfoNCELoss, mrr_ranks
    case = cases.ALL[name]
    c = case["cfg"]
    g = {k[5:]: v for k, v in load_golden(name).items() if k.startswith("sdpa/")}
    m, qf = _build_joint(case, use_lora=False)
    ids, am, hfe, ham, pos, neg, nmask = cases.joint_inputs(case)
    t = lambda a: torch.from_numpy(a).to(DEV)
    user = m(t(ids), t(am), t(hfe), t(ham))
    print(name)
    assert_close(user, g["user_embeddings"], OUT_REL, "user_embeddings")
    loss = InfoNCELoss()(user, t(pos), t(neg), t(nmask))
    assert_close(loss, g["loss"], OUT_REL, "infonce loss")
    scores, rank = mrr_ranks(user, t(pos), t(neg))
    assert rank.cpu().tolist() == g["ranks"].tolist()
    loss.backward()
    named = dict(qf.named_parameters())
    # Ill-conditioned gradients: with Q = 2 the layer-0 self-attention softmax runs over two nearly identical keys, and
    # every item sees the SAME learned queries, so the bf16 rounding of P / o is one coherent draw over the whole batch:
    # the query / key weight gradients come out 50x smaller than their neighbours (norm 3e-3 against 0.2) and carry
    # 0.7 - 3 % error for either attention kernel depending on the weight seed (tools/lab/tiny_attn_joint_err.py; 7 %
    # for this fixture's seed).  Their error is held against 5 % of the query-table gradient's norm instead of their own.
    ill = 0.05 * float(np.linalg.norm(g["grad/query_embeddings"]))
    ILL_KEYS = ("qformer.encoder.layer.0.attention.self.query.weight", "qformer.encoder.layer.0.attention.self.key.bias")
    gs = grad_scale(g, cases.item_grad_keys(c, heads=False))
    for k in cases.item_grad_keys(c, heads=False):
        assert_close(cases.trim_like(named[k].grad.float().cpu().numpy()), g["grad/" + k], GRAD_REL * 1.5, "grad/" + k, floor=1e-6,
                     abs_scale=ill if k in ILL_KEYS else 0.0, ref_scale=gs)
    assert named["item_representation_head.weight"].grad is None      # unused heads stay untouched (as in the reference)


@pytest.mark.parametrize("name", JOINT)
def test_joint_with_lora_matches_oracle(name):
    """LoRA has no importable reference here (peft absent: parity unpinned); check against the oracle's
    restatement of the published formula, including dA / dB."""
    from unirec_amd.joint import InfoNCELoss
    case = cases.ALL[name]
    c = case["cfg"]
    qc = cases.qwen_cfg(case)
    m, qf = _build_joint(case, use_lora=True, lora_seed=case["seed"] + 2)
    ids, am, hfe, ham, pos, neg, nmask = cases.joint_inputs(case)
    t = lambda a: torch.from_numpy(a).to(DEV)
    user = m(t(ids), t(am), t(hfe), t(ham))
    loss = InfoNCELoss()(user, t(pos), t(neg), t(nmask))
    loss.backward()
    # oracle
    cfg = R.QFormerCfg(c["H"], c["L"], c["nh"], c["I"], c["Q"], c["E"], 2)
    PQ = {k: torch.from_numpy(v).requires_grad_(True) for k, v in W.fill_state_dict(R.item_qformer_shapes(cfg, c["F"]), case["seed"]).items()}
    PW = {k: torch.from_numpy(v) for k, v in W.fill_state_dict(Q.qwen3_shapes(qc, lora=False), case["seed"] + 1).items()}
    lsh = {k: s for k, s in Q.qwen3_shapes(qc, lora=True).items() if ".lora_" in k}
    PL = {k: torch.from_numpy(v).requires_grad_(True) for k, v in W.fill_state_dict(lsh, case["seed"] + 2).items()}
    B, hist = case["B"], case["hist"]
    out = R.item_qformer_forward(PQ, cfg, torch.from_numpy(hfe).view(B * hist, c["F"], c["E"]), torch.from_numpy(ham).view(B * hist, c["F"]))
    toks = out["query_outputs"].view(B, hist, c["Q"], c["H"])
    ou = Q.joint_forward({**PW, **PL}, qc, torch.from_numpy(ids), torch.from_numpy(am), toks, case["first_special_id"])
    ol = Q.infonce_loss(ou, torch.from_numpy(pos), torch.from_numpy(neg), torch.from_numpy(nmask))
    ol.backward()
    print(name, "(LoRA)")
    assert_close(user, ou.detach().numpy(), OUT_REL, "user_embeddings")
    assert_close(loss, ol.detach().numpy(), OUT_REL, "loss")
    named = dict(m.base_model.named_parameters())
    for k in ("layers.0.self_attn.q_proj.lora_A.weight", "layers.0.self_attn.k_proj.lora_B.weight", "layers.0.self_attn.v_proj.lora_A.weight",
              "layers.1.self_attn.o_proj.lora_B.weight", "layers.1.mlp.gate_proj.lora_A.weight", "layers.0.mlp.up_proj.lora_B.weight",
              "layers.1.mlp.down_proj.lora_A.weight", "layers.1.mlp.down_proj.lora_B.weight"):
        assert_close(named[k].grad, PL[k].grad.numpy(), GRAD_REL * 1.5, "grad/" + k)
    assert_close(dict(qf.named_parameters())["query_embeddings"].grad, PQ["query_embeddings"].grad.numpy(), GRAD_REL * 1.5, "grad/query_embeddings")
    assert named["layers.0.self_attn.q_proj.weight"].grad is None      # base weights are frozen


def test_merged_projection_launches_are_bit_identical(monkeypatch):
    """q|k|v and gate|up leave as ONE GEMM launch each, their LoRA term as a block-diagonal second K range (exact zeros off the
    diagonal): the pooled output and every LoRA gradient must equal the per-adapter launches bit for bit."""
    from unirec_amd.joint import InfoNCELoss
    from unirec_amd.switches import switches
    case = cases.ALL[JOINT[0]]
    ids, am, hfe, ham, pos, neg, nmask = cases.joint_inputs(case)
    t = lambda a: torch.from_numpy(a).to(DEV)
    res = []
    for merged in (True, False):
        monkeypatch.setattr(switches, "merge_proj", merged)
        m, qf = _build_joint(case, use_lora=True, lora_seed=case["seed"] + 2)
        user = m(t(ids), t(am), t(hfe), t(ham))
        InfoNCELoss()(user, t(pos), t(neg), t(nmask)).backward()
        grads = {k: p.grad.detach().clone() for k, p in m.base_model.named_parameters() if p.grad is not None}
        res.append((user.detach().clone(), grads))
    assert torch.equal(res[0][0], res[1][0])
    assert res[0][1].keys() == res[1][1].keys() and len(res[0][1]) > 0
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k


@pytest.mark.parametrize("name", JOINT[:1])
def test_joint_with_lora_dropout_matches_oracle(name):
    """LoRA dropout (reference :121-131, lora_dropout=0.1; peft: one nn.Dropout per adapter on the adapter's
    input).  The HIP path draws its masks from a counter-based generator (ur_lora_dropout_bits); the test regenerates
    exactly those bit planes from the layer's seed and feeds the unpacked masks to the oracle, so the arithmetic -- forward, dA with the masked input,
    dB, and the masked gradient into the adapter input -- is checked element for element; the mask statistics
    are checked separately."""
    _check_lora_dropout(cases.ALL[name], name, 0.25)


def test_joint_with_lora_dropout_mid_size_matches_oracle():
    """The same check where the step's own kernels run: the 0.6B layer shape (D 1024, 16 / 8 heads of 128, I 3072), M = 32 x 512 =
    16384 tokens -- the 256x256 projection GEMM with its masked rank-16 epilogue (64 x 4 tiles), the merged q|k|v / gate|up launches,
    the fused RMSNorm / SwiGLU + adapter passes (D = 1024, r = 16) -- at the reference's lora_dropout = 0.1."""
    _check_lora_dropout(dict(cases.MID["joint_mid"], B=32), "joint_mid B=32", 0.1)


def _check_lora_dropout(case, name, pdrop):
    from unirec_amd import hip
    from unirec_amd.joint import InfoNCELoss
    c = case["cfg"]
    qc = cases.qwen_cfg(case)
    m, qf = _build_joint(case, use_lora=True, lora_seed=case["seed"] + 2)
    bm = m.base_model
    bm.config.lora_dropout = pdrop
    bm.lora_seed, bm._lora_step = 77, 5
    ids, am, hfe, ham, pos, neg, nmask = cases.joint_inputs(case)
    t = lambda a: torch.from_numpy(a).to(DEV)
    user = m(t(ids), t(am), t(hfe), t(ham))
    loss = InfoNCELoss()(user, t(pos), t(neg), t(nmask))
    loss.backward()
    assert bm._lora_step == 6
    # the masks the kernels used
    B, S = ids.shape
    M, D, I, NQ = B * S, qc.hidden_size, qc.intermediate_size, qc.num_attention_heads * qc.head_dim
    groups = {0: (("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"), D), 1: (("self_attn.o_proj",), NQ),
              2: (("mlp.gate_proj", "mlp.up_proj"), D), 3: (("mlp.down_proj",), I)}
    masks, kept = {}, []
    for i in range(qc.num_hidden_layers):
        for g, (names, width) in groups.items():
            seed = bm.lora_dropout_seed(5, i, g)
            keep = hip.lora_bits_to_keep(hip.lora_dropout_bits(seed, pdrop, M, width, len(names), DEV), width).cpu()
            for slot, nm in enumerate(names):
                mk = keep[slot].view(B, S, width)
                masks[f"layers.{i}.{nm}"] = mk
                kept.append(mk.float().mean().item())
    assert abs(sum(kept) / len(kept) - (1 - pdrop)) < 0.01, kept
    assert not torch.equal(masks["layers.0.self_attn.q_proj"], masks["layers.0.self_attn.k_proj"])      # one mask per adapter
    # oracle with the same masks
    qc.lora_dropout = pdrop
    cfg = R.QFormerCfg(c["H"], c["L"], c["nh"], c["I"], c["Q"], c["E"], 2)
    PQ = {k: torch.from_numpy(v).requires_grad_(True) for k, v in W.fill_state_dict(R.item_qformer_shapes(cfg, c["F"]), case["seed"]).items()}
    PW = {k: torch.from_numpy(v) for k, v in W.fill_state_dict(Q.qwen3_shapes(qc, lora=False), case["seed"] + 1).items()}
    lsh = {k: s_ for k, s_ in Q.qwen3_shapes(qc, lora=True).items() if ".lora_" in k}
    PL = {k: torch.from_numpy(v).requires_grad_(True) for k, v in W.fill_state_dict(lsh, case["seed"] + 2).items()}
    hist = case["hist"]
    out = R.item_qformer_forward(PQ, cfg, torch.from_numpy(hfe).view(B * hist, c["F"], c["E"]), torch.from_numpy(ham).view(B * hist, c["F"]))
    toks = out["query_outputs"].view(B, hist, c["Q"], c["H"])
    ou = Q.joint_forward({**PW, **PL}, qc, torch.from_numpy(ids), torch.from_numpy(am), toks, case["first_special_id"], lora_masks=masks)
    ol = Q.infonce_loss(ou, torch.from_numpy(pos), torch.from_numpy(neg), torch.from_numpy(nmask))
    ol.backward()
    print(name, "(LoRA dropout)")
    assert_close(user, ou.detach().numpy(), OUT_REL, "user_embeddings")
    assert_close(loss, ol.detach().numpy(), OUT_REL, "loss")
    named = dict(bm.named_parameters())
    for k in ("layers.0.self_attn.q_proj.lora_A.weight", "layers.0.self_attn.k_proj.lora_A.weight", "layers.0.self_attn.v_proj.lora_B.weight",
              "layers.1.self_attn.o_proj.lora_A.weight", "layers.1.mlp.gate_proj.lora_A.weight", "layers.0.mlp.up_proj.lora_A.weight",
              "layers.1.mlp.down_proj.lora_A.weight", "layers.0.mlp.down_proj.lora_B.weight"):
        assert_close(named[k].grad, PL[k].grad.numpy(), GRAD_REL * 1.5, "grad/" + k)
    # the gradient that reaches the Q-Former went through every masked adapter-input gradient (ur_gemm drop_bits)
    assert_close(dict(qf.named_parameters())["query_embeddings"].grad, PQ["query_embeddings"].grad.numpy(), GRAD_REL * 1.5, "grad/query_embeddings")
    # eval mode: no dropout, and the step counter does not move
    m.eval()
    with torch.no_grad():
        u0 = m(t(ids), t(am), t(hfe), t(ham))
    qc.lora_dropout = 0.0
    ou0 = Q.joint_forward({**PW, **PL}, qc, torch.from_numpy(ids), torch.from_numpy(am), toks.detach(), case["first_special_id"])
    assert_close(u0, ou0.detach().numpy(), OUT_REL, "user_embeddings(eval)")
    assert bm._lora_step == 6


def test_topk_and_ranks_are_exact():
    from unirec_amd import hip
    g = torch.Generator().manual_seed(0)
    s = torch.randn(5, 1001, generator=g)
    s[0, 7] = s[0, 3]                    # a tie: lowest index first
    sd = s.to(DEV)
    idx, val = hip.topk(sd, 10)
    want = Q.topk_indices(s, 10)
    assert idx.cpu().tolist() == want.tolist()
    rank = hip.mrr_rank(sd)
    assert rank.cpu().tolist() == (1 + (s[:, 1:] > s[:, :1]).sum(1)).tolist()


def test_inject_handles_repeated_and_missing_tokens():
    from unirec_amd import hip
    B, S, D, T, first = 2, 300, 64, 3, 50
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, first, (B, S), generator=g)
    ids[0, 5] = first; ids[0, 290] = first; ids[0, 17] = first + 2      # token 0 twice, token 1 missing
    ids[1, 0] = first + 1
    emb = torch.randn(first + T, D, generator=g).to(DEV).to(torch.bfloat16)
    tok = torch.randn(B, T, D, generator=g).to(DEV).to(torch.bfloat16)
    idsd = ids.to(DEV)
    out = hip.embed_inject_fwd(emb, idsd, tok, first)
    want = emb[idsd]
    want[0, 5] = tok[0, 0]; want[0, 290] = tok[0, 0]; want[0, 17] = tok[0, 2]; want[1, 0] = tok[1, 1]
    assert torch.equal(out, want)
    dx = torch.randn(B, S, D, generator=g).to(DEV).to(torch.bfloat16)
    dt = hip.inject_bwd(dx, idsd, first, T)
    assert torch.equal(dt[0, 0], (dx[0, 5].float() + dx[0, 290].float()).to(torch.bfloat16))
    assert torch.equal(dt[0, 2], dx[0, 17]) and torch.equal(dt[1, 1], dx[1, 0])
    assert float(dt[0, 1].abs().max()) == 0 and float(dt[1, 0].abs().max()) == 0


def test_user_tokens_into_qwen3_matches_oracle_composition():
    """U4 (no reference code): UserQFormer query tokens injected after the history tokens; checked against
    the oracle's composition of its pinned pieces (user Q-Former, injection, Qwen3, pool, InfoNCE)."""
    from unirec_amd.joint import InfoNCELoss, MultiModalQwenEmbedding
    from unirec_amd.qformer_model import QFormerForItemRepresentation
    from unirec_amd.user_qformer import UserQFormer
    case = cases.ALL["joint_right"]
    c = case["cfg"]
    qc = cases.qwen_cfg(case)
    D, hist, Qi, B, S = qc.hidden_size, case["hist"], c["Q"], case["B"], case["S"]
    NU, T, Eu = 8, 24, 192
    cfg = R.QFormerCfg(c["H"], c["L"], c["nh"], c["I"], c["Q"], c["E"], 2)
    ucfg = R.QFormerCfg(D, 2, D // 64, 512, NU, Eu, 1)
    qf = load_generated(QFormerForItemRepresentation(hidden_size=c["H"], num_hidden_layers=c["L"], num_attention_heads=c["nh"],
                                                     intermediate_size=c["I"], num_query_tokens=c["Q"], field_embedding_dim=c["E"],
                                                     num_fields=c["F"], dropout=0.0), R.item_qformer_shapes(cfg, c["F"]), 5)
    uq = load_generated(UserQFormer(hidden_size=D, num_hidden_layers=2, num_attention_heads=D // 64, intermediate_size=512,
                                    num_query_tokens=NU, input_embedding_dim=Eu, num_item_tokens_to_predict=2, dropout=0.0),
                        R.user_qformer_shapes(ucfg, 2), 6)
    hc = _qwen_cfg(qc, False)
    hc.vocab_size = case["first_special_id"]
    m = MultiModalQwenEmbedding(qformer_model=qf, use_lora=False, qwen_config=hc, num_history_items=hist, num_query_tokens_per_item=Qi,
                                user_qformer=uq)
    sdw = {k: torch.from_numpy(v) for k, v in W.fill_state_dict(Q.qwen3_shapes(qc, lora=False), 7).items()}
    emb = torch.from_numpy(W.normal("emb", (case["first_special_id"] + hist * Qi + NU, D), 7, std=0.02))
    sdw["embed_tokens.weight"] = emb
    m.base_model.load_state_dict(sdw, strict=False)
    m = m.to(DEV).train()
    ids, am, hfe, ham, pos, neg, nmask = cases.joint_inputs(case)
    first_u = case["first_special_id"] + hist * Qi
    for b in range(B):                                    # put each user special once into the real region
        real = [p for p in np.nonzero(am[b])[0] if ids[b, p] < case["first_special_id"]][:NU]
        for k, p in enumerate(real):
            ids[b, p] = first_u + k
    ut = W.normal("ut", (B, T, Eu), 8, std=0.8)
    um = np.ones((B, T), dtype=np.float32); um[1, 15:] = 0; ut[1, 15:] = 0
    t = lambda a: torch.from_numpy(a).to(DEV)
    user = m(t(ids), t(am), t(hfe), t(ham), user_sequence_tokens=t(ut), user_attention_mask=t(um))
    loss = InfoNCELoss()(user, t(pos), t(neg), t(nmask))
    loss.backward()
    # oracle composition
    PQ = {k: torch.from_numpy(v).requires_grad_(True) for k, v in W.fill_state_dict(R.item_qformer_shapes(cfg, c["F"]), 5).items()}
    PU = {k: torch.from_numpy(v).requires_grad_(True) for k, v in W.fill_state_dict(R.user_qformer_shapes(ucfg, 2), 6).items()}
    PW = {k: v for k, v in sdw.items()}
    it = R.item_qformer_forward(PQ, cfg, torch.from_numpy(hfe).view(B * hist, c["F"], c["E"]), torch.from_numpy(ham).view(B * hist, c["F"]))
    _, uqo = R.user_qformer_forward(PU, ucfg, torch.from_numpy(ut), torch.from_numpy(um), 2)
    toks = torch.cat([it["query_outputs"].view(B, hist * Qi, D), uqo], dim=1).view(B, 1, hist * Qi + NU, D)
    ou = Q.joint_forward(PW, qc, torch.from_numpy(ids), torch.from_numpy(am), toks, case["first_special_id"])
    ol = Q.infonce_loss(ou, torch.from_numpy(pos), torch.from_numpy(neg), torch.from_numpy(nmask))
    ol.backward()
    print("U4")
    assert_close(user, ou.detach().numpy(), OUT_REL, "user_embeddings")
    assert_close(loss, ol.detach().numpy(), OUT_REL, "loss")
    assert_close(uq.query_embeddings.grad, PU["query_embeddings"].grad.numpy(), GRAD_REL * 1.5, "grad/user query_embeddings")
    assert_close(qf.query_embeddings.grad, PQ["query_embeddings"].grad.numpy(), GRAD_REL * 1.5, "grad/item query_embeddings")


def test_user_sequence_assembly_matches_oracle():
    """U0: tokens + context + sinusoidal PE over the flat index + right padding / mask in one kernel."""
    from unirec_amd.user_sequence_encoder import UserSequenceAssembler
    B, L, Qi, H = 3, 7, 4, 128
    tok = W.normal("tok", (B, L, Qi, H), 1, std=0.8)
    ctx = W.normal("ctx", (B, L, H), 2, std=0.3)
    lens = np.array([7, 3, 1], dtype=np.int64)
    asm = UserSequenceAssembler(embedding_dim=H, num_query_tokens=Qi)
    out, mask = asm.encode_user_sequences(torch.from_numpy(tok).to(DEV), torch.from_numpy(ctx).to(DEV), torch.from_numpy(lens).to(DEV))
    assert out.shape == (B, L * Qi, H) and mask.shape == (B, L * Qi)
    for b in range(B):
        n = int(lens[b])
        tb = torch.from_numpy(tok[b, :n]).to(torch.bfloat16).float()
        cb = torch.from_numpy(ctx[b, :n]).to(torch.bfloat16).float()
        want = R.assemble_user_sequence(tb, cb)
        got = out[b, :n * Qi].float().cpu()
        assert torch.allclose(got, want, rtol=1e-2, atol=2e-2), (b, (got - want).abs().max())
        assert float(out[b, n * Qi:].abs().max()) == 0.0 if n < L else True
        assert mask[b].cpu().tolist() == [1.0] * (n * Qi) + [0.0] * ((L - n) * Qi)

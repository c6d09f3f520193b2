"""GPU: LoRA on chosen projections and layers (peft's target_modules / layers_to_transform / use_rslora).

Primitive.  ur_rmsnorm_lora_fwd with ONE adapter (rms_lora_kernel<1>: a q|k|v or gate|up group that holds a single adapter) is held to
float64 element by element exactly as tests/test_gpu_lora_f64.py::test_fused_rmsnorm_lora_projection holds two and three adapters: the
same cases generator, references and criteria (ref64.assert_bf16_rows for h, ref64.assert_lora_bf16 for t), no new bound.

Decoder step.  The shapes, inputs, weights and bounds of tests/test_gpu_lora_ranks.py (OUT_REL for the pooled output, GRAD_REL * 1.5 for
every adapter gradient and the item-token gradient), LoRA dropout 0.1 ON, against the CPU oracle whose weights simply lack the absent
adapters.  The masks are NOT taken from the model: the test draws them by the canonical rule -- the mask of module m of layer i is plane
slot(m) of lora_dropout_bits(lora_dropout_seed(step, i, group(m)), p, M, W, len(group)), slot = the module's position in its group -- so a
model that handed a kernel the wrong plane (the mask of another module) would miss the gradient bound by far (dA moves by ~45 %)."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import qwen3_ref as Q  # noqa: E402
from tests import lora_cases, norm_cases, ref64  # noqa: E402
from tests.parity_utils import GRAD_REL, OUT_REL, assert_close  # noqa: E402
from tests.test_gpu_lora_f64 import RMS_EPS, _bits16, _note, _planes, _sentinel_bf16, _tag, _written  # noqa: E402
from tests.test_gpu_lora_ranks import GROUPS, PDROP, SEED, SHAPES, STEP, T, _inputs, _oracle_cfg, _weights  # noqa: E402

DEV = "cuda"
F32 = torch.float32
ALL7 = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
ATTN = ("q_proj", "k_proj", "v_proj", "o_proj")


# ---- primitive: one adapter ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("M", [1, 63, 65, 200])
def test_fused_rmsnorm_lora_projection_one_adapter(M, p):
    from unirec_amd import hip
    D, nad = 1024, 1
    c = lora_cases.fused_case(M, D, nad, p, seed=900 + M + nad, row0=(0, lora_cases.ROW0_BIG)[M % 2])
    c["path"] = "rmsnorm_lora_fwd"
    what = _tag(c)
    x, w = norm_cases.rows(M, D, 40 + M), norm_cases.norm_weight(D, 41 + M)
    U, bits = [u.to(DEV) for u in c["U"]], _planes(c)
    t, base = _sentinel_bf16(M, 16 * nad)
    h, rstd, _ = hip.rmsnorm_lora_fwd(x.to(DEV), w.to(DEV), RMS_EPS, U, alpha=c["alpha"], bits=bits, t_out=t)
    _written(t, base, what + " t")
    r64, r32 = ref64.rmsnorm_fwd(x, w, RMS_EPS), ref64.rmsnorm_fwd(x, w, RMS_EPS, dtype=F32)
    _note("rmsnorm_lora_fwd<1> h", ref64.assert_bf16_rows(h.cpu(), r64[0], r32[0], what + " h"))
    hs = h.cpu()
    assert t.shape == (M, 16 * nad)
    _note("rmsnorm_lora_fwd<1> t", ref64.assert_lora_bf16(t.cpu(), ref64.rms_lora_t(hs, c["U"], c["keep"], c["alpha"]),
                                                           ref64.rms_lora_t(hs, c["U"], c["keep"], c["alpha"], dtype=F32),
                                                           ref64.rms_lora_t(hs, c["U"], c["keep"], c["alpha"], absolute=True), what + " t"))
    h2, _, t2 = hip.rmsnorm_lora_fwd(x.to(DEV), w.to(DEV), RMS_EPS, U, alpha=c["alpha"], bits=bits)
    assert torch.equal(_bits16(t), _bits16(t2)) and torch.equal(_bits16(h), _bits16(h2)), f"{what}: a second call differs"


def test_one_adapter_reads_the_plane_it_is_given():
    """The plane of slot 1 of a three-plane stream, handed over as the view bits[1:2], gives the t of a one-plane call on a copy of it."""
    from unirec_amd import hip
    M, D = 130, 1024
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M, D, generator=g).to(torch.bfloat16).to(DEV)
    w = (1.0 + 0.1 * torch.randn(D, generator=g)).to(DEV)
    U = [(torch.randn(16, D, generator=g) * 0.1).to(torch.bfloat16).to(DEV)]
    bits = hip.lora_dropout_bits(99, 0.3, M, D, 3, DEV)
    _, _, t_view = hip.rmsnorm_lora_fwd(x, w, RMS_EPS, U, alpha=1.0, bits=bits[1:2])
    _, _, t_copy = hip.rmsnorm_lora_fwd(x, w, RMS_EPS, U, alpha=1.0, bits=bits[1:2].clone())
    _, _, t_other = hip.rmsnorm_lora_fwd(x, w, RMS_EPS, U, alpha=1.0, bits=bits[0:1])
    assert torch.equal(_bits16(t_view), _bits16(t_copy))
    assert not torch.equal(_bits16(t_view), _bits16(t_other))


# ---- decoder step against the oracle -----------------------------------------------------------------------------------------
def _present(targets, layers):
    """dotted module names that carry an adapter: 'layers.{i}.self_attn.q_proj', ..."""
    return [f"layers.{i}.{nm}" for i in (range(2) if layers is None else layers) for names, _ in GROUPS for nm in names
            if nm.rsplit(".", 1)[-1] in targets]


def _oracle_weights(shape, r, targets, layers):
    """the all-seven weights of tests/test_gpu_lora_ranks.py without the tensors of the absent adapters (same values for the rest)"""
    keep = set(_present(targets, layers))
    return {k: v for k, v in _weights(_oracle_cfg(shape, r)).items() if ".lora_" not in k or k.rsplit(".lora_", 1)[0] in keep}


def _product(shape, r, targets, layers=None, rslora=False):
    from unirec_amd.qwen3 import Qwen3Config, Qwen3LoRAModel
    s = SHAPES[shape]
    m = Qwen3LoRAModel(Qwen3Config(vocab_size=128, hidden_size=s["D"], intermediate_size=s["I"], num_hidden_layers=2,
                                   num_attention_heads=s["nq"], num_key_value_heads=s["nkv"], head_dim=128, lora_r=r, lora_alpha=2.0 * r,
                                   lora_dropout=PDROP, lora_target_modules=None if targets is None else list(targets),
                                   lora_layers_to_transform=layers, use_rslora=rslora))
    m.reset_parameters(lora_b_std=0.05)
    missing, unexpected = m.load_state_dict(_oracle_weights(shape, r, ALL7 if targets is None else targets, layers), strict=False)
    assert not unexpected and not missing
    m = m.to(DEV).train()
    m.lora_seed = SEED
    return m


def _canonical_masks(m, shape, present):
    """plane slot(module) of the group's generator stream, whatever else is present (m is used for its seed function only)"""
    from unirec_amd import hip
    s = SHAPES[shape]
    B, S = s["B"], s["S"]
    width = {"D": s["D"], "NQ": s["nq"] * 128, "I": s["I"]}
    masks = {}
    for i in range(2):
        for g, (names, wkey) in enumerate(GROUPS):
            wd = width[wkey]
            keep = hip.lora_bits_to_keep(hip.lora_dropout_bits(m.lora_dropout_seed(STEP, i, g), PDROP, B * S, wd, len(names), DEV), wd).cpu()
            for slot, nm in enumerate(names):
                if f"layers.{i}.{nm}" in present:
                    masks[f"layers.{i}.{nm}"] = keep[slot].view(B, S, wd)
    return masks


@functools.lru_cache(maxsize=None)
def _oracle(shape, r, targets, layers, rslora, train):
    qc = _oracle_cfg(shape, r)
    if rslora:
        qc.lora_alpha = qc.lora_alpha * math.sqrt(r)          # the oracle's scale is lora_alpha / r
    P = _oracle_weights(shape, r, targets, layers)
    ids, am, tok, gvec, first = _inputs(shape)
    B = ids.shape[0]
    if not train:
        with torch.no_grad():
            return Q.joint_forward(P, qc, ids, am, tok.float().view(B, 1, T, -1), first).numpy(), None, None
    masks = _canonical_masks(_product(shape, r, targets, layers, rslora), shape, set(_present(targets, layers)))
    lora = {k: v.requires_grad_(True) for k, v in P.items() if ".lora_" in k}
    toks = tok.float().view(B, 1, T, -1).requires_grad_(True)
    ou = Q.joint_forward(P, qc, ids, am, toks, first, lora_masks=masks)
    (ou * gvec).sum().backward()
    return ou.detach().numpy(), {k: v.grad.numpy() for k, v in lora.items()}, toks.grad.view(B, T, -1).numpy()


def _step_meets_the_oracle(shape, r, targets, layers=None, rslora=False, prefetch=True):
    lt = None if layers is None else tuple(layers)
    ou, gl, gt = _oracle(shape, r, tuple(targets), lt, rslora, True)
    m = _product(shape, r, targets, layers, rslora)
    m._lora_step = STEP
    ids, am, tok, gvec, first = _inputs(shape)
    ids, am = ids.to(DEV), am.to(DEV)
    tok = tok.to(DEV).requires_grad_(True)
    if prefetch:
        m.prefetch_lora_bits(ids.numel(), ids.device)
    pooled = m.forward_pooled(ids, am, tok, first)
    pooled.backward(gvec.to(DEV))
    torch.cuda.synchronize()
    what = f"{shape} r={r} {'+'.join(targets)} layers={layers} rslora={rslora}"
    assert_close(pooled, ou, OUT_REL, f"[{what}] pooled")
    named = dict(m.named_parameters())
    present = _present(targets, layers)
    # exactly peft's trainable set: a parameter that does not exist has no gradient -- absent, not a zero tensor
    lora_names = sorted(k for k in named if ".lora_" in k)
    assert lora_names == sorted(f"{p}.lora_{ab}.weight" for p in present for ab in "AB") == sorted(gl)
    assert sorted(n for n, _ in m.lora_named_parameters()) == lora_names and sorted(m.pack.names) == lora_names
    assert sorted(k for k, v in named.items() if v.grad is not None) == lora_names
    for k in sorted(gl):
        assert_close(named[k].grad, gl[k], GRAD_REL * 1.5, f"[{what}] grad/{k}")
    assert_close(tok.grad, gt, GRAD_REL * 1.5, f"[{what}] grad/item_tokens")
    return m, ids


@pytest.mark.parametrize("targets", [("q_proj", "v_proj"), ("k_proj",), ("o_proj", "down_proj")], ids="+".join)
def test_big_decoder_step_meets_the_oracle(targets):
    """2 layers of the 0.6B shape, B 8 x S 512, r = 16: q+v (planes 0 and 2 of the q|k|v stream as a strided view), k alone (the
    one-adapter fused RMSNorm kernel inside the model, plane 1), o+down (no adapter in q|k|v and gate|up: both merged launches bare)."""
    m, ids = _step_meets_the_oracle("big", 16, targets)
    plan = m._plan(ids.numel(), ids.shape[1], ids.device, m._pack, m._frozen)
    assert plan.merged and plan.fuse_norm and plan.fuse_rope and plan.swiglu == "pair"


@pytest.mark.parametrize("r,targets", [(16, ("gate_proj",)), (8, ("q_proj", "v_proj")), (32, ("q_proj", "v_proj")), (64, ATTN)],
                         ids=lambda v: "+".join(v) if isinstance(v, tuple) else str(v))
def test_small_decoder_step_meets_the_oracle(r, targets):
    """hidden 256, 2/1 heads, I 384, B 2 x S 128: generic tiles, partial token blocks; planes drawn in the forward (no prefetch)"""
    _step_meets_the_oracle("small", r, targets, prefetch=False)


def test_small_decoder_layers_to_transform_train_and_eval():
    """adapters on q and v of layer 1 only: layer 0 runs as the adapter-free model does; then eval under no_grad"""
    m, ids = _step_meets_the_oracle("small", 16, ("q_proj", "v_proj"), layers=[1], prefetch=True)
    assert m.adapter_modules == ((), ("self_attn.q_proj", "self_attn.v_proj"))
    ou, _, _ = _oracle("small", 16, ("q_proj", "v_proj"), (1,), False, False)
    _, am, tok, _, first = _inputs("small")
    m.eval()
    with torch.no_grad():
        pooled = m.forward_pooled(ids, am.to(DEV), tok.to(DEV), first)
    torch.cuda.synchronize()
    assert_close(pooled, ou, OUT_REL, "[small q+v layer 1] pooled (eval)")


def test_small_decoder_rslora_all_seven():
    """use_rslora: the scale is lora_alpha / sqrt(r); the oracle (scale lora_alpha / r) gets lora_alpha * sqrt(r)"""
    m, _ = _step_meets_the_oracle("small", 16, ALL7, rslora=True, prefetch=False)
    assert m._lora_scale() == 32.0 / 4.0


# ---- plan ------------------------------------------------------------------------------------------------------------------------
def test_plans_of_q_and_v():
    from unirec_amd.qwen3 import _Plan
    s = SHAPES["big"]
    M, S = s["B"] * s["S"], s["S"]

    def plan_of(r, targets):
        m = _product("big", r, targets)
        return m._plan(M, S, torch.device(DEV), m._ensure_pack(DEV), m._ensure_frozen(DEV))
    assert plan_of(16, ("q_proj", "v_proj")) == _Plan(merged=True, fuse_norm=True, fuse_rope=True, swiglu="pair", pad_att=True, bits_one_event=False,
                                                      mlp_recompute="pair", rope_bwd_in_dq=True, rope_k_in_dkv=True, bits_t=True)
    # rank 32 on q and v: the merged launch's second K range is 2 * 32 = 64 columns, one K tile
    assert plan_of(32, ("q_proj", "v_proj")) == _Plan(merged=True, fuse_norm=False, fuse_rope=True, swiglu="pair", pad_att=True, bits_one_event=False,
                                                      mlp_recompute="pair", rope_bwd_in_dq=True, rope_k_in_dkv=True, bits_t=False)
    assert plan_of(32, None).merged is False and plan_of(32, ALL7).merged is False


# ---- the default is untouched ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["small", "big"])
def test_explicit_seven_equals_the_default_bit_for_bit(shape):
    outs = []
    for targets in (None, ALL7):
        m = _product(shape, 16, targets)
        m._lora_step = STEP
        ids, am, tok, gvec, first = _inputs(shape)
        ids, am = ids.to(DEV), am.to(DEV)
        tok = tok.to(DEV).requires_grad_(True)
        m.prefetch_lora_bits(ids.numel(), ids.device)
        pooled = m.forward_pooled(ids, am, tok, first)
        pooled.backward(gvec.to(DEV))
        torch.cuda.synchronize()
        outs.append((pooled.detach(), tok.grad, {n: p.grad for n, p in m.lora_named_parameters()}))
    (p0, t0, g0), (p1, t1, g1) = outs
    assert torch.equal(p0, p1) and torch.equal(t0, t1)
    assert list(g0) == list(g1) and len(g0) == 2 * 7 * 2
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n

"""GPU: merged adapters -- ur_lora_merge element by element against float64 (tests/lora_merge_ref.py: the bound is derived there), the
merged forward against the CPU oracle on the shapes of tests/test_gpu_lora_targets.py, the exactness of unmerge, merge_and_unload, the
refusal of training while merged, and the export a plain ``transformers`` Qwen3Model loads."""
import functools
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import qwen3_ref as Q  # noqa: E402
from tests.lora_merge_ref import lora_merge_ref, merge_inputs, merge_terms  # noqa: E402
from tests.parity_utils import OUT_REL, assert_close, rel_err  # noqa: E402
from tests.test_gpu_lora_ranks import SEED, SHAPES, STEP, _inputs  # noqa: E402
from tests.test_gpu_lora_targets import ALL7, _oracle, _oracle_weights, _product  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
QV, OD = ("q_proj", "v_proj"), ("o_proj", "down_proj")

# entry point of include/unirec_hip_adapter.h -> its float64 tests (tests/test_lora_merge_host.py holds this dict to the header)
COVERS = {"ur_lora_merge": ["test_merge_kernel_matches_float64_element_by_element"]}


# ---- 5. the kernel ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _kernel_case(O, I, r):
    W, A, B = merge_inputs(O, I, r, seed=1000 + O + 3 * I + r)
    return W, A, B, merge_terms(W, A, B)


def _padded(t, pad, fill):
    """(buffer [rows, cols + pad] filled with `fill`, its [rows, cols] view holding t): a row stride larger than the width"""
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf, buf[:, :t.shape[1]]


def _held(got, ref, bound, what):
    err = (got.detach().cpu().double() - ref).abs()
    bad = err > bound
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"  {what}: worst |got - ref| / bound = {ratio:.3f}, worst |got - ref| = {float(err.max()):.3e}")
    if bool(bad.any()):
        o, i = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements miss the bound; first [{o},{i}]: got {float(got[o, i]):.9g}, "
                             f"ref {float(ref[o, i]):.17g}, bound {float(bound[o, i]):.3e}")


@pytest.mark.parametrize("O,I,r", [(8, 8, 8), (24, 40, 16), (136, 264, 32), (1024, 1024, 16), (3072, 1024, 64), (1024, 3072, 8)])
def test_merge_kernel_matches_float64_element_by_element(O, I, r):
    from unirec_amd import hip
    W, A, B, terms = _kernel_case(O, I, r)
    Ad, Bd = A.to(DEV), B.to(DEV)
    for scale in (2.0, -0.75):
        ref, b32, b16 = lora_merge_ref(W, A, B, scale, terms)
        what = f"[{O}x{I} r={r} scale={scale}]"
        # out_f32 alone: W and the output with row strides larger than the width (W's a multiple of 4, the output's of 4 as well)
        wbuf, wv = _padded(W, 4, 3.0)
        obuf, ov = _padded(torch.zeros(O, I), 12, 7.0)
        o32, none = hip.lora_merge(wv, Ad, Bd, scale, out_f32=ov)
        assert none is None and o32 is ov
        _held(ov, ref, b32, what + " f32 alone")
        assert bool((obuf[:, I:] == 7.0).all()) and torch.equal(wbuf[:, :I].cpu(), W) and bool((wbuf[:, I:] == 3.0).all()), what + ": padding or W written"
        # out_bf16 alone, padded rows
        hbuf, hv = _padded(torch.zeros(O, I, dtype=BF16), 8, 7.0)
        hip.lora_merge(wv, Ad, Bd, scale, out_bf16=hv)
        _held(hv, ref, b16, what + " bf16 alone")
        assert bool((hbuf[:, I:] == 7.0).all()), what + ": bf16 padding written"
        # both, dense; twice: equal bits; the bf16 output is the rounding of the f32 one
        Wd = W.to(DEV)
        d32, d16 = hip.lora_merge(Wd, Ad, Bd, scale, out_f32=torch.empty(O, I, device=DEV), out_bf16=torch.empty(O, I, dtype=BF16, device=DEV))
        e32, e16 = hip.lora_merge(Wd, Ad, Bd, scale, out_f32=torch.empty(O, I, device=DEV), out_bf16=torch.empty(O, I, dtype=BF16, device=DEV))
        _held(d32, ref, b32, what + " f32 of both")
        _held(d16, ref, b16, what + " bf16 of both")
        assert torch.equal(d32.view(torch.int32), e32.view(torch.int32)) and torch.equal(d16.view(torch.int16), e16.view(torch.int16)), what + ": a second call differs"
        assert torch.equal(d32.view(torch.int32), ov.contiguous().view(torch.int32)) and torch.equal(d16.view(torch.int16), hv.contiguous().view(torch.int16)), \
            what + ": the result depends on the strides or on which outputs are asked for"
        assert torch.equal(d16.view(torch.int16), d32.to(BF16).view(torch.int16)), what + ": out_bf16 is not the round-to-nearest-even of out_f32"
        # in place on a padded W, with the bf16 output beside it
        ibuf, iv = _padded(W, 8, 3.0)
        i32, i16 = hip.lora_merge(iv, Ad, Bd, scale, out_f32=iv, out_bf16=torch.empty(O, I, dtype=BF16, device=DEV))
        assert i32 is iv
        _held(iv, ref, b32, what + " in place")
        assert torch.equal(iv.contiguous().view(torch.int32), d32.view(torch.int32)) and torch.equal(i16.view(torch.int16), d16.view(torch.int16)), what + ": in place differs"
        assert bool((ibuf[:, I:] == 3.0).all()), what + ": in place wrote the padding"
    # the default: a new dense f32 tensor
    n32, _ = hip.lora_merge(W.to(DEV), Ad, Bd, -0.75)
    assert torch.equal(n32.view(torch.int32), d32.view(torch.int32))


def test_merge_kernel_empty_and_refused():
    from unirec_amd import _lib, hip
    out, _ = hip.lora_merge(torch.empty(0, 16, device=DEV), torch.zeros(8, 16, device=DEV), torch.empty(0, 8, device=DEV), 1.0)
    assert out.shape == (0, 16)
    W = torch.zeros(16, 16, device=DEV)
    with pytest.raises(_lib.UniRecHipError, match="ur_lora_merge.*out_bf16 aliases"):
        hip.lora_merge(W, torch.zeros(8, 16, device=DEV), torch.zeros(16, 8, device=DEV), 1.0, out_bf16=W.view(BF16)[:, :16])
    with pytest.raises(ValueError, match="rank"):
        hip.lora_merge(W, torch.zeros(24, 16, device=DEV), torch.zeros(16, 24, device=DEV), 1.0)


# ---- 6. / 7. the merged forward against the oracle --------------------------------------------------------------------------------------
def _eval_inputs(shape):
    ids, am, tok, gvec, first = _inputs(shape)
    return ids.to(DEV), am.to(DEV), tok.to(DEV), gvec.to(DEV), first


def _merged_meets_the_oracle(shape, r, targets, layers=None, rslora=False):
    ou, _, _ = _oracle(shape, r, tuple(targets), None if layers is None else tuple(layers), rslora, False)
    m = _product(shape, r, targets, None if layers is None else list(layers), rslora).eval()
    ids, am, tok, _, first = _eval_inputs(shape)
    seen = []
    real_plan = m._plan
    m._plan = lambda *a: seen.append((a[3], real_plan(*a))) or seen[-1][1]
    with torch.no_grad():
        un = m.forward_pooled(ids, am, tok, first)
        m.merge_adapter()
        assert m.merged and m._merged["bytes"] > 0
        me = m.forward_pooled(ids, am, tok, first)
        m.unmerge_adapter()
        un2 = m.forward_pooled(ids, am, tok, first)
    torch.cuda.synchronize()
    what = f"{shape} r={r} {'+'.join(targets)} layers={layers} rslora={rslora}"
    print(f"  [{what}] rel err against the oracle: merged {rel_err(me.float().cpu().numpy(), ou):.3e}, unmerged {rel_err(un.float().cpu().numpy(), ou):.3e}")
    assert_close(me, ou, OUT_REL, f"[{what}] merged pooled")
    assert torch.equal(un, un2), f"[{what}]: the forward after unmerge_adapter() is not the forward before merge_adapter()"
    (p0, plan0), (p1, plan1), (p2, plan2) = seen
    assert p0 is not None and p1 is None and p2 is p0, "the merged forward runs without the parameter pack"
    assert plan0 == plan2
    return m, plan1


@pytest.mark.parametrize("targets", [ALL7, QV, OD], ids="+".join)
@pytest.mark.parametrize("r", [8, 16, 64])
def test_merged_forward_meets_the_oracle(r, targets):
    _merged_meets_the_oracle("small", r, targets)


def test_merged_forward_layers_to_transform():
    m, _ = _merged_meets_the_oracle("small", 16, QV, layers=[1])
    m.merge_adapter()
    base, fz = m._ensure_frozen(m.embed_tokens.weight.device), m._merged["fz"]
    assert fz["layers"][0] is base["layers"][0], "a layer without adapters keeps its operands"
    l1, b1 = fz["layers"][1], base["layers"][1]
    assert l1["qkv"] is not b1["qkv"] and l1["qkvT"] is not b1["qkvT"] and all(l1[k] is b1[k] for k in ("o", "oT", "gu", "guT", "guP", "d", "dT"))
    NQ, NKV = 256, 128
    assert not torch.equal(l1["qkv"][:NQ], b1["qkv"][:NQ]) and torch.equal(l1["qkv"][NQ:NQ + NKV], b1["qkv"][NQ:NQ + NKV]), "k_proj carries no adapter"
    assert torch.equal(l1["qkvT"], l1["qkv"].t()) and (l1["qkvP"] is None or torch.equal(l1["qkvP"], l1["qkv"][m._qk_row_perm(DEV)]))


def test_merged_forward_rslora():
    m, _ = _merged_meets_the_oracle("small", 16, ALL7, rslora=True)
    assert m._lora_scale() == 32.0 / 4.0


def test_merged_operands_follow_the_adapters():
    """the cache key holds the adapters' state: a changed adapter between two merges (torch's in-place update, or the fused optimizer's
    raw write announced by mark_dirty) gives new operands; an unchanged one keeps them"""
    m = _product("small", 16, QV).eval()
    m.merge_adapter()
    fz0 = m._merged["fz"]
    m.merge_adapter()
    assert m._merged["fz"] is fz0
    q0 = fz0["layers"][0]["qkv"].clone()
    with torch.no_grad():
        m.layers[0].self_attn.q_proj.lora_B.weight.mul_(2.0)
    m.merge_adapter()
    assert m._merged["fz"] is not fz0 and not torch.equal(m._merged["fz"]["layers"][0]["qkv"], q0)
    ids, am, tok, _, first = _eval_inputs("small")
    with torch.no_grad():
        m.forward_pooled(ids, am, tok, first)
    m.unmerge_adapter()
    with torch.no_grad():
        m.forward_pooled(ids, am, tok, first)           # builds the pack
    m.merge_adapter()
    fz1 = m._merged["fz"]
    m.pack.w32("layers.0.self_attn.q_proj.lora_B.weight").data.mul_(0.5)      # raw write into the master, as the fused AdamW does
    m.pack.mark_dirty()
    m.merge_adapter()
    assert m._merged["fz"] is not fz1 and torch.equal(m._merged["fz"]["layers"][0]["qkv"], q0)      # (x 2, x 0.5: exact)


def test_big_merged_forward_takes_the_adapter_free_plan():
    """2 layers of the 0.6B shape, B 8 x S 512, r 16, all seven: the persistent GEMM and its fused q/k-norm + RoPE epilogue on merged
    operands; the plan is the one a model without adapters gets"""
    from unirec_amd.qwen3 import Qwen3Config, Qwen3LoRAModel, _Plan
    m, plan = _merged_meets_the_oracle("big", 16, ALL7)
    s = SHAPES["big"]
    bare = Qwen3LoRAModel(Qwen3Config(vocab_size=128, hidden_size=s["D"], intermediate_size=s["I"], num_hidden_layers=1, num_attention_heads=s["nq"],
                                      num_key_value_heads=s["nkv"], head_dim=128), use_lora=False).to(DEV)
    want = bare._plan(s["B"] * s["S"], s["S"], torch.device(DEV), None, bare._ensure_frozen(DEV))
    assert plan == want, (plan, want)
    assert isinstance(plan, _Plan) and plan.merged and plan.fuse_rope and not plan.fuse_norm and plan.mlp_recompute == "plain"


def test_disable_adapter_runs_the_base_model():
    """inside disable_adapter() the forward is the base model's (the oracle without any adapter tensor), merged or not; outside it nothing
    has changed"""
    from tests.test_gpu_lora_ranks import T, _oracle_cfg
    m = _product("small", 16, ALL7).eval()
    ids, am, tok, _, first = _eval_inputs("small")
    P = {k: v for k, v in _oracle_weights("small", 16, ALL7, None).items() if ".lora_" not in k}
    ids_c, am_c, tok_c, _, _ = _inputs("small")
    with torch.no_grad():
        base = Q.joint_forward(P, _oracle_cfg("small", 16), ids_c, am_c, tok_c.float().view(ids_c.shape[0], 1, T, -1), first).numpy()
        on = m.forward_pooled(ids, am, tok, first)
        with m.disable_adapter():
            off = m.forward_pooled(ids, am, tok, first)
        m.merge_adapter()
        with m.disable_adapter():
            off_merged = m.forward_pooled(ids, am, tok, first)
        assert m.merged
        m.unmerge_adapter()
        on2 = m.forward_pooled(ids, am, tok, first)
    assert_close(off, base, OUT_REL, "[small] disable_adapter(): the base model")
    assert torch.equal(off, off_merged) and torch.equal(on, on2) and not torch.equal(on, off)


# ---- 8. round trip: a training step, merge, eval, unmerge, the same training step ----------------------------------------------------
def test_training_step_is_bit_equal_after_merge_and_unmerge():
    m = _product("small", 16, ALL7)
    ids, am, tok, gvec, first = _eval_inputs("small")

    def step():
        m.train()
        m._lora_step = STEP
        for p in m.parameters():
            p.grad = None
        if m.pack is not None:
            m.pack.clear_grads()
        t = tok.clone().requires_grad_(True)
        pooled = m.forward_pooled(ids, am, t, first)
        pooled.backward(gvec)
        torch.cuda.synchronize()
        return pooled.detach().clone(), t.grad.clone(), {n: p.grad.detach().clone() for n, p in m.lora_named_parameters()}
    assert m.lora_seed == SEED and m._drop_p() > 0.0
    p0, t0, g0 = step()
    m.eval()
    m.merge_adapter()
    with torch.no_grad():
        m.forward_pooled(ids, am, tok, first)
    m.unmerge_adapter()
    p1, t1, g1 = step()
    assert torch.equal(p0, p1) and torch.equal(t0, t1)
    assert list(g0) == list(g1) and len(g0) == 2 * 7 * 2
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


# ---- 9. refusals; merge_and_unload -----------------------------------------------------------------------------------------------------
def test_training_forward_while_merged_is_refused():
    m = _product("small", 16, QV)
    ids, am, tok, _, first = _eval_inputs("small")
    m.merge_adapter()
    m.train()
    with pytest.raises(RuntimeError, match="unmerge_adapter"):
        m.forward_pooled(ids, am, tok, first)
    m.prefetch_lora_bits(ids.numel(), ids.device)
    assert m._bits_pre is None, "prefetch_lora_bits is a no-op while merged"
    with torch.no_grad():                          # (train mode without grad: an evaluation forward, no dropout on merged operands)
        a = m.forward_pooled(ids, am, tok, first)
    m.eval()
    t = tok.clone().requires_grad_(True)           # eval mode with grad: the backward runs on the merged transposes
    b = m.forward_pooled(ids, am, t, first)
    b.sum().backward()
    assert torch.equal(a, b.detach()) and t.grad is not None and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0
    assert all(p.grad is None for _, p in m.lora_named_parameters())


def test_joint_trainer_on_a_merged_model_is_refused(tmp_path):
    from transformers import TrainingArguments
    from tests.test_gpu_grad_clip import _inputs as joint_batch
    from tests.test_gpu_grad_clip import _joint
    from unirec_amd.joint import JointTrainer
    case, model = _joint()
    tr = JointTrainer(model, TrainingArguments(output_dir=str(tmp_path), learning_rate=1e-4, max_steps=2, report_to=[]))
    batch = joint_batch(case)
    model.merge_adapter()
    with pytest.raises(RuntimeError, match="unmerge_adapter"):
        tr.training_step(batch)
    model.unmerge_adapter()
    assert bool(torch.isfinite(tr.training_step(batch)))


def test_merge_and_unload_equals_a_fresh_model_without_adapters():
    from unirec_amd.qwen3 import Qwen3Config, Qwen3LoRAModel
    m = _product("small", 16, ALL7).eval()
    ids, am, tok, _, first = _eval_inputs("small")
    ou, _, _ = _oracle("small", 16, ALL7, None, False, False)
    lora = {n: p.detach().clone() for n, p in m.lora_named_parameters()}
    base = {n: p.detach().clone() for n, p in m.named_parameters() if ".lora_" not in n}
    assert m.merge_and_unload() is m
    assert not m.use_lora and m.pack is None and m._frozen is None
    sd = m.state_dict()
    s = SHAPES["small"]
    qc = Q.Qwen3Cfg(hidden_size=s["D"], num_hidden_layers=2, num_attention_heads=s["nq"], num_key_value_heads=s["nkv"], head_dim=128,
                    intermediate_size=s["I"], vocab_size=128)
    assert {k: tuple(v.shape) for k, v in sd.items()} == Q.qwen3_shapes(qc, lora=False)
    for n, w in base.items():                      # the masters: the float64 merge under the kernel's bound; the rest untouched
        a = lora.get(n.replace(".weight", ".lora_A.weight"))
        if a is None:
            assert torch.equal(sd[n], w), n
            continue
        ref, b32, _ = lora_merge_ref(w.cpu(), a.cpu(), lora[n.replace(".weight", ".lora_B.weight")].cpu(), 2.0)
        _held(sd[n], ref, b32, n)
    with torch.no_grad():
        got = m.forward_pooled(ids, am, tok, first)
    fresh = Qwen3LoRAModel(Qwen3Config(vocab_size=128, hidden_size=s["D"], intermediate_size=s["I"], num_hidden_layers=2, num_attention_heads=s["nq"],
                                       num_key_value_heads=s["nkv"], head_dim=128), use_lora=False)
    fresh.load_state_dict({k: v.cpu() for k, v in sd.items()})
    fresh = fresh.to(DEV).eval()
    with torch.no_grad():
        want = fresh.forward_pooled(ids, am, tok, first)
    assert torch.equal(got, want)
    assert_close(got, ou, OUT_REL, "[small] merge_and_unload pooled")


# ---- 10. export -------------------------------------------------------------------------------------------------------------------------
class _QF(torch.nn.Module):
    """stands in for the item Q-Former: a config with the hidden size and a state dict (the decoder is what these tests export)"""

    def __init__(self, hidden, value=0.0):
        super().__init__()
        self.config = type("C", (), {"hidden_size": hidden})()
        self.w = torch.nn.Parameter(torch.full((4,), float(value)))


def _joint_small(r=16, targets=ALL7):
    """MultiModalQwenEmbedding around the `small` decoder of the tests above: the vocabulary is 120 + the 8 special tokens the tokenizer
    adds (resize_token_embeddings), the weights are the oracle's"""
    from unirec_amd.joint import HistoryTokenTable, MultiModalQwenEmbedding
    from unirec_amd.qwen3 import Qwen3Config
    s = SHAPES["small"]
    cfg = Qwen3Config(vocab_size=120, hidden_size=s["D"], intermediate_size=s["I"], num_hidden_layers=2, num_attention_heads=s["nq"],
                      num_key_value_heads=s["nkv"], head_dim=128, lora_r=r, lora_alpha=2.0 * r, lora_dropout=0.1, lora_target_modules=list(targets))
    kw = dict(qwen_config=cfg, num_history_items=4, num_query_tokens_per_item=2, tokenizer=HistoryTokenTable(120, 4, 2))
    mm = MultiModalQwenEmbedding(qformer_model=_QF(s["D"], 1.5), **kw)
    assert mm.base_model.embed_tokens.weight.shape[0] == 128 and mm.first_special_id == 120
    missing, unexpected = mm.base_model.load_state_dict(_oracle_weights("small", r, targets, None), strict=False)
    assert not missing and not unexpected
    return mm.to(DEV).eval(), kw


def test_merged_export_loads_in_transformers(tmp_path):
    from safetensors.torch import load_file
    from transformers import Qwen3Model
    from tests.test_gpu_lora_ranks import T
    from tests.test_oracle_golden import _close
    mm, _ = _joint_small()
    ids, am, tok, _, first = _inputs("small")
    assert first == mm.first_special_id
    before = {n: p.detach().clone() for n, p in mm.base_model.named_parameters()}
    mm.save_pretrained(str(tmp_path), merged=True)
    assert sorted(os.listdir(tmp_path)) == ["config.json", "history_tokens.json", "model.safetensors", "model_config.json", "qformer_model.bin"]
    assert mm.use_lora and mm.base_model.use_lora and not mm.base_model.merged
    for n, p in mm.base_model.named_parameters():
        assert torch.equal(p, before[n]), f"{n}: save_pretrained(merged=True) modified the live model"
    # the tensors: HF keys, f32, the float64 merge under the kernel's bound; embed_tokens with its added rows
    sd = load_file(os.path.join(tmp_path, "model.safetensors"))
    s = SHAPES["small"]
    qc = Q.Qwen3Cfg(hidden_size=s["D"], num_hidden_layers=2, num_attention_heads=s["nq"], num_key_value_heads=s["nkv"], head_dim=128,
                    intermediate_size=s["I"], vocab_size=128)
    assert {k: tuple(v.shape) for k, v in sd.items()} == Q.qwen3_shapes(qc, lora=False) and all(v.dtype == F32 for v in sd.values())
    for n, w in sd.items():
        a = before.get(n.replace(".weight", ".lora_A.weight"))
        if a is None or ".lora_" in n:
            assert torch.equal(w, before[n].cpu()), n
            continue
        ref, b32, _ = lora_merge_ref(before[n].cpu(), a.cpu(), before[n.replace(".weight", ".lora_B.weight")].cpu(), 2.0)
        _held(w, ref, b32, n)
    # plain transformers on the CPU in f32 against the unmerged f32 oracle: two f32 evaluations of one function
    hf = Qwen3Model.from_pretrained(str(tmp_path), local_files_only=True, dtype=F32, attn_implementation="sdpa").eval()
    assert hf.embed_tokens.weight.shape[0] == 128
    B = ids.shape[0]
    with torch.no_grad():
        x = Q.inject_tokens(hf.embed_tokens(ids), ids, tok.float().view(B, 1, T, -1), first)
        got = hf(inputs_embeds=x, attention_mask=am).last_hidden_state.mean(dim=1)
    ou, _, _ = _oracle("small", 16, ALL7, None, False, False)
    print(f"  transformers on the merged export against the unmerged oracle: rel err {rel_err(got.numpy(), ou):.3e}")
    _close(got.numpy(), ou, rtol=1e-3, atol=1e-5, what="pooled")              # tests/test_oracle_golden.py::test_joint's tolerance for this tensor
    # a lower-precision export
    mm.save_pretrained(str(tmp_path / "bf16"), merged=True, dtype=BF16)
    assert all(v.dtype == BF16 for v in load_file(os.path.join(tmp_path, "bf16", "model.safetensors")).values())
    assert json.load(open(os.path.join(tmp_path, "bf16", "config.json")))["dtype"] == "bfloat16"


def test_save_and_from_pretrained_round_trip(tmp_path):
    from unirec_amd.joint import MultiModalQwenEmbedding
    mm, kw = _joint_small(16, QV)
    ids, am, tok, _, first = _eval_inputs("small")
    with torch.no_grad():
        want = mm.base_model.forward_pooled(ids, am, tok, first)
    # merged=False: the files and adapter keys of before
    d = tmp_path / "adapters"
    mm.save_pretrained(str(d))
    assert sorted(os.listdir(d)) == ["adapter_config.json", "adapter_model.bin", "history_tokens.json", "model_config.json", "qformer_model.bin"]
    keys = sorted(torch.load(os.path.join(d, "adapter_model.bin")))
    assert keys == sorted(f"base_model.model.layers.{i}.self_attn.{p}.lora_{ab}.weight" for i in range(2) for p in QV for ab in "AB")
    base = {k: v for k, v in _oracle_weights("small", 16, QV, None).items() if ".lora_" not in k}
    qf = _QF(256)
    back = MultiModalQwenEmbedding.from_pretrained(str(d), qf, base_state_dict=base, **dict(kw, qwen_config=_fresh_cfg(kw["qwen_config"])))
    assert back.use_lora and back.base_model.adapter_modules == mm.base_model.adapter_modules and float(qf.w.detach()[0]) == 1.5
    back = back.to(DEV).eval()
    with torch.no_grad():
        got = back.base_model.forward_pooled(ids, am, tok, first)
    assert torch.equal(got, want), "from_pretrained does not reproduce the saved model's eval forward bit for bit"
    # the merged directory read back: a model without adapters that computes what merge_and_unload() leaves
    dm = tmp_path / "merged"
    mm.save_pretrained(str(dm), merged=True)
    loaded = MultiModalQwenEmbedding.from_pretrained(str(dm), _QF(256), num_history_items=4, num_query_tokens_per_item=2).to(DEV).eval()
    assert not loaded.use_lora and loaded.first_special_id == 120 and loaded.base_model.embed_tokens.weight.shape[0] == 128
    mm.merge_and_unload()
    assert not mm.use_lora
    with torch.no_grad():
        a, b = loaded.base_model.forward_pooled(ids, am, tok, first), mm.base_model.forward_pooled(ids, am, tok, first)
    assert torch.equal(a, b)
    assert_close(a, want.float().cpu().numpy(), OUT_REL, "merged against unmerged")


def _fresh_cfg(cfg):
    from unirec_amd.qwen3 import Qwen3Config
    return Qwen3Config(vocab_size=120, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size, num_hidden_layers=cfg.num_hidden_layers,
                       num_attention_heads=cfg.num_attention_heads, num_key_value_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim)

"""GPU: every launch of a decoder training step held to float64, LINK BY LINK (tests/layer_links.py; docs/lab_notes.md section 31).

All cases run the 0.6B layer shape -- D 1024, 16 / 8 heads of 128, I 3072 -- with 2 layers and random weights (oracle.weights), left
padding on one sample and a fully valid one, injected item tokens (inject_bwd is a station) and a shard offset (row0 != 0).
  1  the product's plan: all seven adapters, r 16, dropout 0.1, at the smallest (B, S) whose _plan equals the benchmark shape's field by
     field (asserted), with and without prefetched bit planes
  2  the other plan: B 3 x S 200, q and v adapters on layer 1 only, r 8, rsLoRA, recompute_mlp, no kept RMSNorm outputs
  3  stale operands: the masters moved in place, a second step, merge_adapter() + an eval forward, unmerge_adapter() + a third step
  4  every adapter gradient and the injected-token gradient end to end against the oracle at GRAD_REL * 1.5
Every case prints each station's worst error / bound ("[ratio] station: x", run with -s) and its wall time."""
import time
from dataclasses import fields

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import qwen3_ref as Q  # noqa: E402
from oracle import weights as W  # noqa: E402
from tests import attn_cases, layer_links as LL  # noqa: E402
from tests.parity_utils import GRAD_REL, assert_close  # noqa: E402
from unirec_amd import hip  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
FIRST, T = 500, 4                     # base vocabulary; injected item tokens
SHAPES = sorted(((b, s) for b in (2, 4, 8, 16, 32, 64) for s in (256, 512, 1024, 2048)), key=lambda bs: (bs[0] * bs[1], bs[1]))
_CACHE = {}


def _config(**kw):
    from unirec_amd.qwen3 import Qwen3Config
    kw = dict(dict(lora_r=16, lora_alpha=32.0, lora_dropout=0.1), **kw)
    return Qwen3Config(vocab_size=FIRST + T, hidden_size=1024, intermediate_size=3072, num_hidden_layers=2, num_attention_heads=16,
                       num_key_value_heads=8, head_dim=128, **kw)


def _build(seed=31, **kw):
    from unirec_amd.qwen3 import Qwen3LoRAModel
    c = _config(**kw)
    m = Qwen3LoRAModel(c)
    qc = Q.Qwen3Cfg(vocab_size=c.vocab_size, num_hidden_layers=2, lora_r=c.lora_r, lora_alpha=c.lora_alpha)
    gen = W.fill_state_dict(Q.qwen3_shapes(qc, lora=True), seed)
    own = m.state_dict()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in gen.items() if k in own}, strict=True)
    m = m.to(DEV).train()
    m.lora_seed, m._lora_step, m.sample_offset = 4242, 7, 3
    return m, qc, gen


def _inputs(B, S, seed=5):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, FIRST, (B, S), generator=g)
    mask = torch.ones((B, S), dtype=torch.uint8)
    mask[0, :37] = 0                                          # left padding on sample 0; the others fully valid
    for b in range(B):
        for t in range(T - 1):                                # token T - 1 never appears: its gradient is exactly zero
            ids[b, 40 + 17 * t + b] = FIRST + t
    ids[1, S - 1] = FIRST                                     # token 0 twice in sample 1
    tok = torch.randn((B, T, 1024), generator=g).to(BF16)
    d_pooled = torch.randn((B, 1024), generator=g)
    return tok.to(DEV), ids.to(DEV), mask.to(DEV), FIRST, d_pooled.to(DEV)


def _bits_fn(seed, p, M, Wd, planes, row0):
    return hip.lora_dropout_bits(seed, p, M, Wd, planes, DEV, row0=row0)


def _tables_fn(S, hd, theta):
    return hip.rope_table(S, hd, theta, DEV)                  # the kernel's own rows (tests/test_gpu_head_primitives.py holds them)


def _check(m, st, inp, what, weights=None, live=True):
    B, S = inp[1].shape
    qkr = attn_cases.qk_round_for(128, True, S, S, B=B, nq=16, nkv=8) is not None
    t0 = time.perf_counter()
    print(f"\n[case] {what}: B {B} x S {S}, {len(st.tape)} launches, plan {st.plan}")
    ratios = LL.check_step(st, LL.ModelDef(m, DEV, weights=weights, live=live), inp if st.backward else inp[:4] + (None,), _bits_fn, _tables_fn, qk_rounded=qkr)
    print(f"[time] {what}: checker {time.perf_counter() - t0:.1f} s; worst error / bound {max(ratios.values()):.4f} at {max(ratios, key=ratios.get)}")
    return ratios


def _product_shape(m):
    """the smallest (B, S) whose plan is the benchmark shape's (B 64 x S 2048): the _plan queries launch nothing"""
    fz, pack = m._operands(torch.device(DEV, torch.cuda.current_device()))
    bench = m._plan(64 * 2048, 2048, torch.device(DEV), pack, fz)
    for B, S in SHAPES:
        if m._plan(B * S, S, torch.device(DEV), pack, fz) == bench:
            return B, S, bench
    raise AssertionError("no shape up to B 64 x S 2048 has the benchmark's plan")


def _same_plan(plan, bench):
    for f in fields(bench):
        assert getattr(plan, f.name) == getattr(bench, f.name), f"plan.{f.name} = {getattr(plan, f.name)!r}, at the benchmark's shape {getattr(bench, f.name)!r}"


# ---- 1: the product's plan ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefetch", [False, True], ids=["planes drawn in the step", "prefetched planes"])
def test_product_plan_every_link(monkeypatch, prefetch):
    t0 = time.perf_counter()
    m, qc, gen = _build()
    B, S, bench = _product_shape(m)
    print(f"\n[shape] smallest shape with the benchmark's plan: B {B} x S {S}; candidates from B 2 x S 256")
    assert bench.merged and bench.fuse_norm and bench.fuse_rope and bench.swiglu == "pair" and bench.rope_bwd_in_dq and bench.bits_t, bench
    inp = _inputs(B, S)
    st = LL.run_step(m, monkeypatch, *inp, prefetch=prefetch)
    _same_plan(st.plan, bench)
    assert st.prefetched == prefetch and st.pdrop == 0.1 and m.first_sample(B) * S != 0
    ratios = _check(m, st, inp, f"1 product plan, {'prefetched' if prefetch else 'drawn'} planes")
    assert sum(k.startswith("grad ") for k in ratios) == 14 * 2 and "d_tok" in ratios
    assert sum(".bits_t_" in k for k in ratios) == 2 * 4, "token-packed planes of every group of both layers"
    if not prefetch:
        _CACHE["case1"] = (m, qc, gen, inp, st)
    print(f"[time] case 1 ({'prefetched' if prefetch else 'drawn'}): {time.perf_counter() - t0:.1f} s")


# ---- 2: the other plan --------------------------------------------------------------------------------------------------------------
def test_other_plan_every_link(monkeypatch):
    t0 = time.perf_counter()
    m, qc, gen = _build(lora_r=8, use_rslora=True, lora_target_modules=("q_proj", "v_proj"), lora_layers_to_transform=[1])
    m.recompute_mlp, m.keep_norm_outputs = True, False
    B, S = 3, 200
    inp = _inputs(B, S)
    st = LL.run_step(m, monkeypatch, *inp)
    _, _, bench = _product_shape(_build()[0])
    flipped = [f.name for f in fields(bench) if getattr(st.plan, f.name) != getattr(bench, f.name)]
    print(f"\n[plan] {st.plan}\n[plan] differs from case 1's in: {flipped}")
    for f in ("fuse_norm", "fuse_rope", "swiglu", "mlp_recompute", "rope_bwd_in_dq", "bits_t"):
        assert f in flipped, f"the configuration is meant to flip plan.{f}"
    assert st.recomputed == [True, True] and st.kept_norms == [False, False] and (B * S) % 128 != 0
    ratios = _check(m, st, inp, "2 other plan")
    assert sum(k.startswith("grad ") for k in ratios) == 4 and "L0.t_qkv" not in ratios and "L1.t_qkv" in ratios and "L1.t_o" not in ratios
    assert "L0.gu (recomputed)" in ratios and "L1.h (recomputed)" in ratios and "L1.dq" in ratios
    print(f"[time] case 2: {time.perf_counter() - t0:.1f} s")


# ---- 3: stale operands --------------------------------------------------------------------------------------------------------------
def _t_stations(st):
    return [r.ret[2] if r.name == "rmsnorm_lora_fwd" else (r.ret[1] if r.name == "swiglu_lora_fwd" else r.ret)
            for r in st.tape if r.name in ("rmsnorm_lora_fwd", "swiglu_lora_fwd", "lora_project")]


def test_stale_operands(monkeypatch):
    t0 = time.perf_counter()
    m, qc, gen = _build()
    B, S, bench = _product_shape(m)
    inp = _inputs(B, S)
    first = LL.run_step(m, monkeypatch, *inp)                 # (case 1 holds this step's links)
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():                                     # an optimizer's step: every master moves in place by its own magnitude
        for n, p in m.named_parameters():
            if ".lora_" in n:
                p.add_((torch.randn(p.shape, generator=g) * float(p.std())).to(DEV))
    m._lora_step = first.lora_step                            # the same masks again: t_* may differ through the adapters alone
    second = LL.run_step(m, monkeypatch, *inp)
    _same_plan(second.plan, bench)
    _check(m, second, inp, "3 second step on moved masters")
    ta, tb = _t_stations(first), _t_stations(second)
    assert len(ta) == len(tb) == 2 * 4 and all(not torch.equal(a, b) for a, b in zip(ta, tb)), "t_* must move with the adapters"
    m.eval()
    m.merge_adapter()
    merged = LL.run_step(m, monkeypatch, *inp[:4])
    assert not merged.live and merged.pdrop == 0.0
    ratios = _check(m, merged, inp, "3 eval forward on merged operands", weights=m.merged_state_dict(), live=False)
    assert not any(".t_" in k for k in ratios)
    m.unmerge_adapter()
    m.train()
    third = LL.run_step(m, monkeypatch, *inp)
    _same_plan(third.plan, bench)
    assert third.lora_step == second.lora_step + 1
    _check(m, third, inp, "3 third step after unmerge_adapter()")
    print(f"[time] case 3: {time.perf_counter() - t0:.1f} s")


# ---- 4: every adapter gradient end to end --------------------------------------------------------------------------------------------
def test_every_adapter_gradient_against_the_oracle(monkeypatch):
    """what links cannot show: that the links listed are all there is.  The oracle (oracle.qwen3_ref.joint_forward, float32 CPU, the
    regenerated keep masks) differentiates the whole stack; ALL 14 x layers LoRA gradients and the injected-token gradient are held
    at the GRAD_REL * 1.5 of tests/test_gpu_joint.py"""
    t0 = time.perf_counter()
    if "case1" not in _CACHE:
        m, qc, gen = _build()
        B, S, _ = _product_shape(m)
        inp = _inputs(B, S)
        _CACHE["case1"] = (m, qc, gen, inp, LL.run_step(m, monkeypatch, *inp))
    m, qc, gen, inp, st = _CACHE["case1"]
    tok, ids, mask, first, d_pooled = inp
    B, S = ids.shape
    M, p = B * S, st.pdrop
    masks = {}
    for i in range(2):
        for g, (_, projs) in enumerate(LL.GROUPS):
            width = (1024, 2048, 1024, 3072)[g]
            bits = hip.lora_dropout_bits(m.lora_dropout_seed(st.lora_step, i, g), p, M, width, len(projs), DEV, row0=m.first_sample(B) * S)
            keep = hip.lora_bits_to_keep(bits, width).cpu()
            for slot, pn in enumerate(projs):
                masks[f"layers.{i}.{LL._MODULE[pn]}.{pn}"] = keep[slot].view(B, S, width)
    qc.lora_dropout = p
    P = {k: torch.from_numpy(v) for k, v in gen.items()}
    for k in P:
        if ".lora_" in k:
            P[k].requires_grad_(True)
    toks = tok.cpu().float().view(B, 1, T, 1024).requires_grad_(True)
    pooled = Q.joint_forward(P, qc, ids.cpu(), mask.cpu(), toks, first, lora_masks=masks)
    (pooled * d_pooled.cpu()).sum().backward()
    names = [k for k in P if ".lora_" in k]
    assert len(names) == 14 * 2 and set(names) == set(st.grads)
    for k in names:
        assert_close(st.grads[k], P[k].grad.numpy(), GRAD_REL * 1.5, "grad/" + k)
    assert_close(st.d_tok, toks.grad.view(B, T, 1024).numpy(), GRAD_REL * 1.5, "grad/injected tokens")
    assert float(st.d_tok[:, T - 1].float().abs().max()) == 0.0, "a token that appears nowhere receives an exactly zero gradient"
    print(f"[time] case 4: {time.perf_counter() - t0:.1f} s")

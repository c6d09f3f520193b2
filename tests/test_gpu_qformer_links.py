"""GPU: every launch of a Q-Former step held to float64, LINK BY LINK (tests/qformer_links.py; docs/lab_notes.md section 35).

All cases: random weights (oracle.weights), sample_offset != 0, model._step preset to a nonzero value, E != H, one fully valid sample,
ragged key masks, one very short history; the item cases also one FULLY masked sample.  Shapes are the smallest at which each decision
in the code is taken; every case asserts, with queries that launch nothing, that the decisions it claims are in force.
  1  item plan (C2's decisions): grouped dW at split_k 2 with a ragged last K slice, GENERIC attention, K | V bias by the post-loop colsum,
     side stream active
  2  the joint step's item plan: Q 2, TINY attention forward and backward, grouped dW at split 1
  3  user plan (C3's decisions): FEWQ dK/dV writing kv_colsum, the hoisted K | V dW on _split_k_for's long-reduction branch, _UserHeadFn
     with the split-K f32 dX + cast
  4  the other user plan: T 96, B 3 -- no grouped launch, single split-K dW, generic dK/dV, K | V bias from colsum
  5  prefix (grad_items, against forward_triplet itself), gradient checkpointing, stale operands, the eval forward
  6  free-standing BertModel: per-sample and [1, Q, H] query embeddings, encoder states with gradient
  7  stream ordering: cases 1 and 3 untaped through the public autograd path, bit for bit
  8  end to end against oracle.qformer_train_ref with the regenerated keep masks
Every case prints each station's worst error / bound ("[ratio] station: x", run with -s) and its wall time."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dropout_ref  # noqa: E402
from oracle import qformer_ref as R  # noqa: E402
from oracle import qformer_train_ref as RT  # noqa: E402
from oracle import weights as W  # noqa: E402
from tests import qformer_links as QL  # noqa: E402
from tests import ref64  # noqa: E402
from tests.parity_utils import GRAD_REL, OUT_REL, assert_close, load_generated  # noqa: E402
from unirec_amd import _lib, hip  # noqa: E402
from unirec_amd.qformer import _split_k_for  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
_CACHE = {}


class GpuMasks:
    """keep masks from the kernels' own generators (tests/test_gpu_norm_f64.py and test_gpu_attention_f64.py hold them against the oracle)"""

    def hidden(self, seed, p, rows, H, row0):
        return hip.dropout_keep(seed, p, row0 * H, rows * H, DEV).view(rows, H).cpu()

    def attn(self, seed, p, B, nh, Sq, Sk, b0):
        return hip.attn_dropout_keep(seed, p, b0 * nh * Sq, B * nh * Sq, Sk, DEV).view(B, nh, Sq, Sk).cpu()


def _mask(B, T, fully_masked=None, seed=3):
    g = torch.Generator().manual_seed(seed)
    mask = torch.ones((B, T), dtype=torch.int64)
    for b in range(1, B):
        mask[b, int(torch.randint(1, T, (1,), generator=g)):] = 0            # ragged; sample 0 stays fully valid
    mask[1, 2:] = 0                                                        # one very short history
    if fully_masked is not None:
        mask[fully_masked] = 0
    return mask


def _item(H, nh, I, L, Q, F_, E, p, B, Bg=None, seed=41, offset=3, step=5):
    from unirec_amd.qformer_utils import QFormerForItemRepresentation
    m = QFormerForItemRepresentation(hidden_size=H, num_hidden_layers=L, num_attention_heads=nh, intermediate_size=I, num_query_tokens=Q,
                                     field_embedding_dim=E, num_fields=F_, dropout=p)
    cfg = R.QFormerCfg(H, L, nh, I, Q, E, 2)
    m = load_generated(m, R.item_qformer_shapes(cfg, F_), seed).train()
    m.qformer.sample_offset, m.qformer._step = offset, step
    g = torch.Generator().manual_seed(seed + 1)
    inputs = dict(enc=torch.randn((B, F_, E), generator=g).to(DEV), mask=_mask(B, F_, 2).to(DEV), grad_items=Bg)
    nb = B if Bg is None else Bg
    d_out = dict(query_outputs=torch.randn((nb, Q, H), generator=g).to(DEV), item=torch.randn((nb, E), generator=g).to(DEV),
                 rec=torch.randn((nb, F_, E), generator=g).to(DEV))
    return m, inputs, d_out, cfg


def _user(H, nh, I, L, Q, T, E, n_pred, p, B, seed=51, offset=2, step=8):
    from unirec_amd.user_qformer import UserQFormer
    m = UserQFormer(hidden_size=H, num_hidden_layers=L, num_attention_heads=nh, intermediate_size=I, num_query_tokens=Q, input_embedding_dim=E,
                    num_item_tokens_to_predict=n_pred, dropout=p)
    cfg = R.QFormerCfg(H, L, nh, I, Q, E, 1)
    m = load_generated(m, R.user_qformer_shapes(cfg, n_pred), seed).train()
    m.qformer.sample_offset, m.qformer._step = offset, step
    g = torch.Generator().manual_seed(seed + 1)
    inputs = dict(enc=torch.randn((B, T, E), generator=g).to(DEV), mask=_mask(B, T).to(DEV))
    return m, inputs, torch.randn((B, n_pred * E), generator=g).to(DEV), cfg


def _check(m, st, inputs, d_out, what):
    t0 = time.perf_counter()
    print(f"\n[case] {what}: {len(st.tape)} launches, forward {st.info}")
    ratios = QL.check_step(st, QL.ModelDef(m, DEV), inputs, GpuMasks(), d_out)
    worst = max(ratios, key=ratios.get)
    print(f"[time] {what}: checker {time.perf_counter() - t0:.1f} s; worst error / bound {ratios[worst]:.4f} at {worst}")
    fam = {}
    for k, v in ratios.items():
        f = k.split(" ")[0] if k.startswith(("grad ", "buffer ")) else k.split(".")[-1].split(" ")[0]
        fam[f] = max(fam.get(f, 0.0), v)
    print("[families] " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(fam.items())))
    return ratios


def _attn_plans(st):
    """[(attn_bwd record, the plan of its launch)] from the library's own contexts: sizes, strides and flags as the step passed them (the
    gradient buffers have the layout of their forward operands); hip.attn_plan launches nothing"""
    ctx_of = {}
    for n, c in st.ctxs:
        ctx_of.setdefault(n, c)
    out = []
    for r in st.tape:
        if r.name != "attn_bwd":
            continue
        c = ctx_of[r.args[0].n]
        g = _lib.AttnBwdArgs()
        g.lddo, g.lddq, g.lddk, g.lddv = c.args.nq * c.args.head_dim, c.args.ldq, c.args.ldk, c.args.ldv
        if r.kwargs.get("kv_colsum") is not None:
            g.kv_colsum = 4096
        out.append((r, c, hip.attn_plan(c, g)))
    return out


def _decisions(st, M, L, ncross_layers):
    plans = _attn_plans(st)
    cross = [(r, c, p) for r, c, p in plans if c.args.key_mask]
    self_ = [(r, c, p) for r, c, p in plans if not c.args.key_mask]
    assert len(cross) == ncross_layers and len(self_) == L
    return self_, cross


def _live_grads_present(m, st):
    live = [n for n, _ in m.live_named_parameters()]
    assert all(st.grads[n] is not None for n in live) and all(st.grads[n] is None for n in st.grads if n not in live) and len(live) < len(st.grads)
    return live


# ---- 1: the item plan -------------------------------------------------------------------------------------------------------------------
def test_item_plan_every_link(monkeypatch):
    t0 = time.perf_counter()
    H, nh, I, L, Q, F_, E, B = 256, 4, 512, 3, 32, 14, 192, 131
    m, inputs, d_out, cfg = _item(H, nh, I, L, Q, F_, E, 0.2, B)
    M = B * Q
    st = QL.run_step(m, monkeypatch, inputs, d_out)
    assert st.info["step_seed"] == 6 and st.info["row0"] == 3 * Q and st.info["p_h"] == st.info["p_a"] == 0.2 and not st.info["ckpt"]
    assert m.qformer._seed(1, 2, 6) == dropout_ref.site_seed(m.qformer.seed, 6, 1, 2)
    # decisions: grouped dW at split >= 2 with a ragged last K slice; generic attention; K | V bias by colsum; side stream
    assert M >= 4096 and M % ref64.GEMM_BK != 0 and st.grouped and st.side
    grouped = [r for r in st.tape if r.name == "gemm_grouped"]
    assert len(grouped) == L, "one grouped launch per layer"
    for r in grouped:
        t256 = sum(-(-o.shape[0] // 256) * -(-o.shape[1] // 256) for _, _, o in r.args[0])
        sp = max(1, min(256 // t256, M // 2048))
        assert sp >= 2 and r.kwargs["split_k"] == sp
        k0, k1 = ref64.splitk_slices(M, sp)[-1]
        assert 0 < k1 - k0 and (k1 - k0) % ref64.GEMM_BK != 0, "the last K slice is ragged"
    self_, cross = _decisions(st, M, L, 2)
    for r, c, p in self_ + cross:
        print(f"[plan] attention {c.args.Sq} x {c.args.Sk}: {p}")
        assert p["fwd"] == "generic" and p["dq"] == "generic" and p["dkv"] not in ("fewq", "tiny", "none"), p
        assert not hip.attn_bwd_kv_colsum_supported(c) and r.kwargs.get("kv_colsum") is None
    assert (cross[0][1].args.Sq, cross[0][1].args.Sk) == (32, 14) and (self_[0][1].args.Sq, self_[0][1].args.Sk) == (32, 32)
    kvcs = [r for r in st.tape if r.name == "colsum" and r.args[0].shape == (B * F_, 4 * H)]
    assert len(kvcs) == 1, "the K | V bias gradients come through ONE post-loop colsum"
    ratios = _check(m, st, inputs, d_out, "1 item plan")
    live = _live_grads_present(m, st)
    assert sum(k.startswith("grad ") for k in ratios) == len(live) == 7 + 2 + 16 * L + 10 * 2, len(live)
    assert "L1.qc" not in ratios and "L0.c.dk" in ratios and "L2.c.dv" in ratios and "hd.rec" in ratios
    _CACHE["case1"] = (m, inputs, d_out, st)
    print(f"[time] case 1: {time.perf_counter() - t0:.1f} s")


# ---- 2: the joint step's item plan --------------------------------------------------------------------------------------------------------
def test_joint_item_plan_every_link(monkeypatch):
    t0 = time.perf_counter()
    H, nh, I, L, Q, F_, E, B = 128, 2, 256, 2, 2, 14, 96, 150
    m, inputs, d_out, cfg = _item(H, nh, I, L, Q, F_, E, 0.2, B)
    st = QL.run_step(m, monkeypatch, inputs, d_out)
    M = B * Q
    assert 256 <= M < 2048 and st.grouped and st.side
    grouped = [r for r in st.tape if r.name == "gemm_grouped"]
    assert len(grouped) == L and all(r.kwargs["split_k"] == 1 for r in grouped) and max(1, min(256, M // 2048)) == 1
    self_, cross = _decisions(st, M, L, 1)
    for r, c, p in self_ + cross:
        print(f"[plan] attention {c.args.Sq} x {c.args.Sk}: {p}")
        assert p["fwd"] == p["dq"] == p["dkv"] == "tiny", p
    ratios = _check(m, st, inputs, d_out, "2 joint's item plan")
    assert sum(k.startswith("grad ") for k in ratios) == len(_live_grads_present(m, st))
    print(f"[time] case 2: {time.perf_counter() - t0:.1f} s")


# ---- 3: the user plan ----------------------------------------------------------------------------------------------------------------------
def _user_case3():
    return _user(128, 2, 256, 2, 64, 320, 96, 43, 0.1, 64)


def test_user_plan_every_link(monkeypatch):
    t0 = time.perf_counter()
    m, inputs, d_out, cfg = _user_case3()
    H, Q, T, B, E, n_pred = 128, 64, 320, 64, 96, 43
    st = QL.run_step(m, monkeypatch, inputs, d_out)
    M, Me = B * Q, B * T
    assert Me >= 16384 and n_pred * E >= 4096 and st.side and st.grouped and st.info["step_seed"] == 9
    self_, cross = _decisions(st, M, 2, 2)
    for r, c, p in cross:
        print(f"[plan] cross attention {c.args.Sq} x {c.args.Sk}: {p}")
        assert p["dkv"] == "fewq" and hip.attn_bwd_kv_colsum_supported(c) and r.kwargs.get("kv_colsum") is not None, p
    assert not any(r.name == "colsum" and r.args[0].shape[0] == Me for r in st.tape), "no second pass over dK | dV"
    # the hoisted K | V weight gradient: alone (its token count is not the layers'), on _split_k_for's long-reduction branch
    kv = [r for r in st.tape if r.name == "gemm" and r.kwargs.get("out") is not None and tuple(r.kwargs["out"].shape) == (4 * H, E)]
    assert len(kv) == 1 and Me != M and kv[0].kwargs["split_k"] == _split_k_for(4 * H, E, Me)
    t256 = ((4 * H + 255) // 256) * ((E + 255) // 256)
    assert _split_k_for(4 * H, E, Me) == min(64, -(-256 // t256)) == 64 and _split_k_for(4 * H, E, 16383) == 63, "the long-reduction branch (red >= 16384)"
    assert any(r.name == "gemm" and r.kwargs.get("out_f32") and r.kwargs.get("split_k", 1) == 2 for r in st.tape), "the head's split-K f32 dX"
    ratios = _check(m, st, inputs, d_out, "3 user plan")
    assert "uh.dln32" in ratios and "uh.dln" in ratios and "L1.c.dk" in ratios
    assert sum(k.startswith("grad ") for k in ratios) == len(_live_grads_present(m, st))
    _CACHE["case3"] = (m, inputs, d_out, st)
    print(f"[time] case 3: {time.perf_counter() - t0:.1f} s")


# ---- 4: the other user plan -----------------------------------------------------------------------------------------------------------------
def test_other_user_plan_every_link(monkeypatch):
    t0 = time.perf_counter()
    H, Q, T, B, E, n_pred = 128, 64, 96, 3, 96, 4
    m, inputs, d_out, cfg = _user(H, 2, 256, 2, Q, T, E, n_pred, 0.1, B)
    st = QL.run_step(m, monkeypatch, inputs, d_out)
    M, Me = B * Q, B * T
    assert M < 256 and not st.grouped and st.side and not any(r.name == "gemm_grouped" for r in st.tape), "no grouped launch"
    self_, cross = _decisions(st, M, 2, 2)
    for r, c, p in cross:
        print(f"[plan] cross attention {c.args.Sq} x {c.args.Sk}: {p}")
        assert p["dkv"] != "fewq" and not hip.attn_bwd_kv_colsum_supported(c) and r.kwargs.get("kv_colsum") is None, p
    assert sum(r.name == "colsum" and tuple(r.args[0].shape) == (Me, 4 * H) for r in st.tape) == 1, "K | V bias from the post-loop colsum"
    dws = [r for r in st.tape if r.name == "gemm" and r.kwargs.get("out") is not None and r.kwargs["out"].dtype == F32 and "split_k" in r.kwargs]
    assert len(dws) == 2 * 6 + 1, "every weight gradient of the encoder is a single split-K product"
    for r in dws:
        o = r.kwargs["out"]
        red = r.args[0].shape[0]
        assert red < 16384 and r.kwargs["split_k"] == _split_k_for(o.shape[0], o.shape[1], red) == int(max(1, min(max(1, 512 // (-(-o.shape[0] // 128) * -(-o.shape[1] // 128))), red // 256, 64))), \
            "_split_k_for's first branch"
    assert n_pred * E // 2048 <= 1, "the head's dX is one bf16 product"
    ratios = _check(m, st, inputs, d_out, "4 other user plan")
    assert "uh.dln32" not in ratios and "uh.dln" in ratios
    assert sum(k.startswith("grad ") for k in ratios) == len(_live_grads_present(m, st))
    print(f"[time] case 4: {time.perf_counter() - t0:.1f} s")


# ---- 5: prefix, checkpointing, stale operands, eval --------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int16 if a.dtype == BF16 else torch.int32), b.contiguous().view(torch.int16 if b.dtype == BF16 else torch.int32))


def test_prefix_checkpointing_stale_operands_eval(monkeypatch):
    t0 = time.perf_counter()
    H, nh, I, L, Q, F_, E, B, Bg = 128, 2, 256, 3, 8, 14, 96, 12, 5
    m, inputs, d_out, cfg = _item(H, nh, I, L, Q, F_, E, 0.2, B, Bg)
    # prefix: the backward's stations cover the leading Bg samples only
    st = QL.run_step(m, monkeypatch, inputs, d_out)
    assert st.info["Bg"] == Bg < st.info["B"] == B
    r1 = _check(m, st, inputs, d_out, "5 prefix (grad_items)")
    assert "hd.others.item" in r1
    # ... and it is what forward_triplet + autograd compute, bit for bit
    m.qformer._step = st.step_before
    m._pack.clear_grads()
    out, other = m.forward_triplet(inputs["enc"][:Bg], inputs["mask"][:Bg], inputs["enc"][Bg:], inputs["mask"][Bg:])
    torch.autograd.backward([out["query_outputs"], out["item_representation"], out["reconstructed_fields"]], [d_out["query_outputs"], d_out["item"], d_out["rec"]])
    torch.cuda.synchronize()
    assert _same_bits(out["item_representation"].detach(), st.out["item"]) and _same_bits(other, st.out["other_item"]) and _same_bits(out["reconstructed_fields"].detach(), st.out["rec"])
    for n, p in m.named_parameters():
        assert (p.grad is None) == (st.grads[n] is None) and (p.grad is None or _same_bits(p.grad, st.grads[n])), f"forward_triplet's {n}.grad differs from the taped step's"
    # checkpointing: the re-run stations are bit-equal to the first run's, and the links hold
    m.qformer.config.gradient_checkpointing = True
    m.qformer._step = st.step_before
    ck = QL.run_step(m, monkeypatch, inputs, d_out)
    assert ck.info["ckpt"]
    r2 = _check(m, ck, inputs, d_out, "5 gradient checkpointing")
    assert all(f"L{i}.rerun" in r2 for i in range(L)) and "L0.s.z (re-run)" in r2
    for n in st.grads:
        assert (st.grads[n] is None) == (ck.grads[n] is None) and (st.grads[n] is None or _same_bits(st.grads[n], ck.grads[n])), f"checkpointing changes {n}.grad"
    m.qformer.config.gradient_checkpointing = False
    # stale operands: every master moves in place by its own magnitude; the shadow cast and the transposes must follow state_dict()
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.add_((torch.randn(p.shape, generator=g) * float(p.std())).to(DEV))
    m.qformer._step = st.step_before
    second = QL.run_step(m, monkeypatch, inputs, d_out)
    r3 = _check(m, second, inputs, d_out, "5 second step on moved masters")
    assert any(k.startswith("prep.shadow") for k in r3) and "prep.transposes" in r3
    tr = lambda s: next(r for r in s.tape if r.name == "batched_transpose").ret      # noqa: E731
    assert all(not torch.equal(a, b) for a, b in zip(tr(st), tr(second))), "every transposed weight must move with its master"
    # eval: no-grad forward, nothing kept, zero dropout
    m.eval()
    ev_in = dict(inputs, grad_items=None)
    with torch.no_grad():
        ev = QL.run_step(m, monkeypatch, ev_in, None, keep=False)
    assert ev.info["p_h"] == ev.info["p_a"] == 0.0 and not ev.backward
    r4 = _check(m, ev, ev_in, None, "5 eval forward")
    assert "L0.s.z" not in r4 and "L0.s.out" in r4 and not any(k.startswith("prep.shadow") for k in r4)
    print(f"[time] case 5: {time.perf_counter() - t0:.1f} s")


# ---- 6: the free-standing BertModel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ["per sample", "one table"])
def test_free_standing_bert_model(monkeypatch, rows):
    from unirec_amd.qformer import BertConfig, BertModel
    t0 = time.perf_counter()
    H, nh, I, L, Q, T, E, B = 128, 2, 256, 2, 8, 20, 96, 6
    c = BertConfig(hidden_size=H, num_hidden_layers=L, num_attention_heads=nh, intermediate_size=I, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1,
                   add_cross_attention=True, query_length=Q, encoder_width=E, cross_attention_freq=2)
    m = BertModel(c)
    m = load_generated(m, R.qformer_live_shapes(R.QFormerCfg(H, L, nh, I, Q, E, 2), prefix=""), 61).train()
    m.sample_offset, m._step = 4, 3
    g = torch.Generator().manual_seed(62)
    inputs = dict(enc=torch.randn((B, T, E), generator=g).to(DEV), mask=_mask(B, T, 2).to(DEV), enc_needs_grad=True,
                  query_embeds=torch.randn((B if rows == "per sample" else 1, Q, H), generator=g).to(DEV))
    d = torch.randn((B, Q, H), generator=g).to(DEV)
    st = QL.run_step(m, monkeypatch, inputs, d)
    ratios = _check(m, st, inputs, d, f"6 BertModel, {rows}")
    assert "d_qe" in ratios and "d_enc" in ratios and "d_enc16" in ratios
    assert tuple(st.d_qe.shape) == tuple(inputs["query_embeds"].shape) and tuple(st.d_enc.shape) == (B, T, E)
    assert any(r.name == "batch_reduce" for r in st.tape) == (rows == "one table")
    assert len(next(r for r in st.tape if r.name == "batched_transpose").ret) == 4 * L + 2 + 1, "the extra transposed group of the encoder states' dX"
    # ... and through the public autograd path, bit for bit
    m._step = st.step_before
    qe, enc = inputs["query_embeds"].clone().requires_grad_(True), inputs["enc"].clone().requires_grad_(True)
    out = m(query_embeds=qe.expand(B, -1, -1) if rows == "one table" else qe, encoder_hidden_states=enc, encoder_attention_mask=inputs["mask"]).last_hidden_state
    out.backward(d)
    torch.cuda.synchronize()
    assert _same_bits(out.detach(), st.out["last_hidden_state"]) and _same_bits(enc.grad, st.d_enc) and _same_bits(qe.grad, st.d_qe)
    print(f"[time] case 6 ({rows}): {time.perf_counter() - t0:.1f} s")


# ---- 7: stream ordering ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["case1", "case3"])
def test_untaped_step_equals_the_taped_step(monkeypatch, case):
    """The tape synchronizes after every launch: a taped step cannot see a missing join() / off_chain dependency.  The same step through
    the public modules and autograd, side stream and all, must give the same bits."""
    t0 = time.perf_counter()
    if case not in _CACHE:
        m, inputs, d_out, cfg = _item(256, 4, 512, 3, 32, 14, 192, 0.2, 131) if case == "case1" else _user_case3()
        _CACHE[case] = (m, inputs, d_out, QL.run_step(m, monkeypatch, inputs, d_out))
    m, inputs, d_out, st = _CACHE[case]
    assert st.side, "the side stream carries this step's reductions"
    m.qformer._step = st.step_before
    m._pack.clear_grads()
    if case == "case1":
        out = m(inputs["enc"], inputs["mask"])
        torch.autograd.backward([out["query_outputs"], out["item_representation"], out["reconstructed_fields"]], [d_out["query_outputs"], d_out["item"], d_out["rec"]])
        got = {"query_outputs": out["query_outputs"], "item": out["item_representation"], "rec": out["reconstructed_fields"]}
    else:
        pred = m(inputs["enc"], inputs["mask"])
        pred.backward(d_out.view(pred.shape))
        got = {"flat": pred.view(pred.shape[0], -1)}
    torch.cuda.synchronize()
    assert m.qformer._step == st.info["step_seed"]
    for k, v in got.items():
        assert _same_bits(v.detach(), st.out[k]), f"untaped {k} differs from the taped step's"
    off = [n for n, p in m.named_parameters() if (p.grad is None) != (st.grads[n] is None) or (p.grad is not None and not _same_bits(p.grad, st.grads[n]))]
    assert not off, f"untaped gradients differ from the taped step's: {off[:6]}"
    print(f"[time] case 7 ({case}): {time.perf_counter() - t0:.1f} s")


# ---- 8: end to end ----------------------------------------------------------------------------------------------------------------------------
def test_every_gradient_against_the_oracle(monkeypatch):
    """what links cannot show: that the links listed are all there is.  oracle.qformer_train_ref differentiates the whole item model
    with the regenerated keep masks; every live gradient at GRAD_REL, the three outputs at OUT_REL."""
    t0 = time.perf_counter()
    H, nh, I, L, Q, F_, E, B, p = 256, 4, 512, 3, 32, 14, 192, 9, 0.2
    m, inputs, d_out, cfg = _item(H, nh, I, L, Q, F_, E, p, B)
    st = QL.run_step(m, monkeypatch, inputs, d_out)
    bert = m.qformer
    masks = dropout_ref.qformer_masks(bert.seed, st.info["step_seed"], p, B, Q, F_, H, nh, L, 2, b0=st.info["b0"])
    P = {k: torch.from_numpy(v).requires_grad_(True) for k, v in W.fill_state_dict(R.item_qformer_shapes(cfg, F_), 41).items()}
    oo = RT.item_qformer_forward_train(P, cfg, inputs["enc"].cpu(), inputs["mask"].cpu(), masks, p)
    for k, o in (("query_outputs", "query_outputs"), ("item_representation", "item"), ("reconstructed_fields", "rec")):
        assert_close(st.out[o], oo[k].detach().numpy(), OUT_REL, k)
    ((oo["query_outputs"] * d_out["query_outputs"].cpu()).sum() + (oo["item_representation"] * d_out["item"].cpu()).sum()
     + (oo["reconstructed_fields"] * d_out["rec"].cpu()).sum()).backward()
    live = _live_grads_present(m, st)
    scale = max(float(P[n].grad.norm()) for n in live)          # (the key biases' gradients are analytically zero: softmax rows sum to 1)
    for n in live:
        assert_close(st.grads[n], P[n].grad.numpy(), GRAD_REL, "grad/" + n, floor=1e-6, ref_scale=scale)
    print(f"[time] case 8: {time.perf_counter() - t0:.1f} s")

"""CPU: the link checker of tests/qformer_links.py bites.

The REAL BertModel._forward_impl / _layer_forward / _backward_impl and the real _ItemHeadsFn / _UserHeadFn run on the CPU over FakeHip, a
float32 stand-in for unirec_amd.hip: every entry point the Q-Former calls, evaluated with tests/ref64.py's restatements at dtype=F32 (or
the same formula in float32 torch) and rounded to bf16 wherever the path stores bf16; keep masks from oracle.dropout_ref.  The tape it
leaves has the format of a GPU tape.  The clean tapes must pass; each MUTANT -- one deliberate glue bug, injected in the stand-in or by
monkeypatching here, never in product code -- must be rejected AT ITS OWN LINK and nowhere upstream of it.

  item   H 128 / 2 heads, I 256, 3 layers (cross attention in 0 and 2), Q 8, F 5, E 96, B 5 of which grad_items 3 (forward_triplet's
         prefix), gradient checkpointing, sample_offset 2; sample 0 fully valid, ragged masks, sample 2 FULLY masked
  user   2 layers with cross attention in each, Q 8, T 256 (the few-query dK/dV kernel's rule: kv_colsum is fused), B 2, n_pred 2"""
import types

import pytest
import torch

from oracle import dropout_ref
from tests import layer_links as LL
from tests import qformer_links as QL
from tests import ref64

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
H, NH, I = 128, 2, 256


def _bf(x):
    return x.to(BF16)


def _hk(seed, p, rows, width, row0):
    return torch.from_numpy(dropout_ref.hidden_keep(seed, p, rows, width, row0).copy()) if p > 0.0 else None


class FakeHip:
    """unirec_amd.hip's entry points as the Q-Former calls them, in float32 torch on the CPU.  mutant: the name of ONE deliberate bug."""
    GEMM_MAX_GROUPS = 8
    _lib = types.SimpleNamespace(UniRecHipError=RuntimeError)

    def __init__(self, mutant=None):
        self.mutant, self.n, self.mem = mutant, {}, {}
        outer = self

        class BatchedTranspose:
            def __init__(self, sources):
                self.sources = sources
                self.first = None

            def run(self):
                out = [s.t().contiguous() for s in self.sources]
                if self.first is None:
                    self.first = out
                return self.first if outer.mutant == "transposes_not_rerun" else out
        self.BatchedTranspose = BatchedTranspose

    def _count(self, what):
        self.n[what] = self.n.get(what, 0) + 1
        return self.n[what] - 1

    def _is(self, mutant, k):
        """count the call under `mutant`; True when this is call k and the mutant is the one asked for"""
        return self._count(mutant) == k and self.mutant == mutant

    # ---- casts, element-wise
    def cast_f32_to_bf16(self, src, dst=None):
        if dst is None:
            return src.to(BF16)
        dst.copy_(src.to(BF16))
        return dst

    def cast_bf16_to_f32(self, src, dst=None):
        return src.to(F32)

    def add_bf16(self, a, b, out=None):
        return _bf(a.float() + b.float())

    def gelu_bwd(self, dy, u):
        return _bf(dy.float() * ref64.gelu_grad_f32(u))

    # ---- LayerNorm
    def layernorm_fwd(self, y, gamma, beta, eps, residual=None, save_z=True, p_pre=0.0, seed_pre=0, p_post=0.0, seed_post=0, M=None, drop_row0=0):
        W = y.shape[-1]
        y2 = y.reshape(-1, W)
        M = y2.shape[0] if M is None else M
        z = _bf(ref64.layernorm_z(y2, residual, _hk(seed_pre, p_pre, M, W, drop_row0), p_pre, y2.shape[0], M, dtype=F32))
        out, mean, rstd, _ = ref64.layernorm_of_z(z, gamma, beta, eps, _hk(seed_post, p_post, M, W, drop_row0), p_post, dtype=F32)
        return _bf(out), (z if save_z else None), mean, rstd

    def layernorm_bwd(self, dout, z, mean, rstd, gamma, dgamma, dbeta, dbias=None, p_pre=0.0, seed_pre=0, p_post=0.0, seed_post=0, need_dy=True,
                      drop_row0=0, defer_reduce=False):
        M, W = z.shape
        if p_pre > 0.0:                                                   # (the layers' sites; the embedding's is post-dropout)
            if self._is("ln_bwd_wrong_site_seed", 0):
                seed_pre -= 1
            if self._is("drop_row0_omitted", 1):
                drop_row0 = 0
        d = dout.float()
        kpost = _hk(seed_post, p_post, M, W, drop_row0)
        if kpost is not None:
            d = d * kpost.float() / (1.0 - p_post)
        xh = (z.float() - mean[:, None]) * rstd[:, None]
        g = d * gamma.float()
        dz = rstd[:, None] * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
        kpre = _hk(seed_pre, p_pre, M, W, drop_row0)
        dz16 = _bf(dz)
        dy16 = dz16 if (kpre is None or not need_dy) else _bf(dz * kpre.float() / (1.0 - p_pre))

        def finish():
            dgamma.copy_((d * xh).sum(0))
            dbeta.copy_(d.sum(0))
            if dbias is not None:
                dbias.copy_(dy16.float().sum(0))
        if defer_reduce:
            finish.scratch = torch.zeros(1)
            return dz16, dy16, finish
        finish()
        return dz16, dy16

    # ---- GEMMs
    def gemm(self, R, S, *, r_kcontig=True, s_kcontig=True, out=None, out_f32=False, bias=None, residual=None, gelu_out=None, gelu_grad_aux=None,
             split_k=1):
        k = self._count("gemm")
        if k == 0 and self.mutant == "kv_weight_order_swapped":          # (the first GEMM is the hoisted K | V projection) v0 | k0 | ... in
            S = torch.cat([S[H:2 * H], S[:H], S[2 * H:]], 0)             # the weight list, k | v in the views
        if residual is not None and self._is("dx_residual_dropped", 0):
            residual = None
        Rm = R.float() if r_kcontig else R.float().t()
        Sm = S.float() if s_kcontig else S.float().t()
        v = Rm @ Sm.t()
        if bias is not None:
            v = v + bias.float()
        if residual is not None:
            v = v + residual.float()
        if gelu_grad_aux is not None:
            v = v * ref64.gelu_grad_f32(gelu_grad_aux)
        if out_f32 or (out is not None and out.dtype == F32):
            if out is None:
                return v
            out.copy_(v.reshape(out.shape))
            return out
        C = _bf(v)
        if out is not None:
            out.copy_(C)
            C = out
        if gelu_out is not None:
            gelu_out.copy_(_bf(ref64.gelu(C.to(F64)).float()))
        if k == 0:
            self.mem["kv_all"] = C
        return C

    def gemm_grouped(self, products, split_k=1):
        outs = [o for _, _, o in products]
        if self.mutant == "grouped_output_misbound" and self._count("grouped") == 0:
            j = next(j for j in range(len(outs) - 1) if outs[j].shape == outs[j + 1].shape)          # two neighbours of one shape
            outs[j], outs[j + 1] = outs[j + 1], outs[j]
        for (R, S, _), o in zip(products, outs):
            o.copy_(R.float().t() @ S.float())

    def colsum(self, x, out=None):
        s = x.float().sum(0)
        if x.shape[1] == 3 * H and self._is("qkv_bias_order", 0):
            s = torch.cat([s[:H], s[2 * H:], s[H:2 * H]])
        if self.mutant == "kv_bias_colsum_skipped" and x.shape[1] % (2 * H) == 0 and x.shape[0] == self.mem.get("Me"):
            return out                                                   # (dK | dV of every cross layer: rows = B * T)
        if out is None:
            return s
        out.copy_(s)
        return out

    def batch_reduce(self, x, nb, rows, W, out=None):
        if self.mutant == "batch_reduce_nb_rows_exchanged":
            s = x.float().reshape(rows, nb, W).sum(1)
        else:
            s = x.float().reshape(nb, rows, W).sum(0)
        if out is None:
            return s
        out.copy_(s.reshape(out.shape))
        return out

    # ---- attention
    def attn_fwd(self, q, k, v, *, causal, key_mask=None, dropout_p=0.0, seed=0, drop_batch0=0):
        B, Sq, nh, _ = q.shape
        if key_mask is None and self._is("drop_batch0_omitted", 0):
            drop_batch0 = 0
        if key_mask is not None:
            self.mem["Me"] = B * k.shape[1]
            if self._is("cross_reads_other_slot", 0):
                kv = self.mem["kv_all"].view(B, k.shape[1], -1, 2, nh, q.shape[-1])[:, :, 1]
                k, v = kv[:, :, 0], kv[:, :, 1]
        a = dict(B=B, p=dropout_p, seed=seed, b0=drop_batch0, causal=causal)
        o = _bf(ref64.attention_fwd(q, k, v, key_mask, causal, q.shape[-1] ** -0.5, self._akeep(a, q, k), dropout_p, dtype=F32)[0]).contiguous()
        return o, types.SimpleNamespace(args=a, keep=(q, k, v, key_mask), o=o, stats=None)

    @staticmethod
    def _akeep(a, q, k):
        if a["p"] <= 0.0:
            return None
        return torch.from_numpy(dropout_ref.attn_keep(a["seed"], a["p"], a["B"], q.shape[2], q.shape[1], k.shape[1], a["b0"]).copy())

    def attn_ctx_prefix(self, ctx, Bg):
        return types.SimpleNamespace(args=dict(ctx.args, B=int(Bg)), keep=ctx.keep, o=ctx.o, stats=None)

    def attn_bwd_kv_colsum_supported(self, ctx):
        q, k, v, _ = ctx.keep               # the header's rule for the few-query dK/dV kernel: head_dim 64, non-causal, nq == nkv, <= 64 queries, >= 256 keys
        return q.shape[-1] == 64 and not ctx.args["causal"] and q.shape[2] == k.shape[2] and q.shape[1] <= 64 and k.shape[1] >= 256

    def attn_bwd(self, ctx, dout, dq=None, dk=None, dv=None, kv_colsum=None):
        a = ctx.args
        B = a["B"]
        q, k, v, mask = (None if t is None else t[:B] for t in ctx.keep)
        g = ref64.attention_bwd(q, k, v, mask, a["causal"], q.shape[-1] ** -0.5, dout, self._akeep(a, q, k), a["p"], dtype=F32)
        for dst, src in zip((dq, dk, dv), g):
            dst.copy_(_bf(src))
        if kv_colsum is not None and self.mutant == "kv_colsum_of_the_f32_accumulators":          # (no bug: what the few-query kernel does)
            kv_colsum.copy_(torch.cat([t.float().reshape(-1, t.shape[2] * t.shape[3]).sum(0) for t in g[1:]]))
        elif kv_colsum is not None:
            kv_colsum.copy_(torch.cat([dk.float().reshape(-1, dk.shape[2] * dk.shape[3]).sum(0), dv.float().reshape(-1, dv.shape[2] * dv.shape[3]).sum(0)]))
        return dq, dk, dv

    # ---- heads
    def mean_pool_fwd(self, x, out_f32=True, out_bf16=False):
        m = x.float().mean(1)
        return (m if out_f32 else None), (_bf(m) if out_bf16 else None)

    def mean_pool_bwd(self, dout, S_):
        return _bf((dout.float() / S_)[:, None, :].expand(dout.shape[0], S_, dout.shape[1])).contiguous()

    def field_projection_fwd(self, rec16, Wf, bf):
        return ref64.field_projection_fwd(rec16, Wf, bf, dtype=F32)

    def field_projection_bwd(self, dout, rec16, Wf, dWf, dbf):
        r = ref64.field_projection_bwd(dout, rec16, Wf, dtype=F32)
        dWf.copy_(r[1])
        dbf.copy_(r[2])
        return _bf(r[0]).contiguous()


# =================================================================================================================================
def _masks(B, T, fully_masked):
    g = torch.Generator().manual_seed(3)
    mask = torch.ones((B, T), dtype=torch.int64)
    for b in range(1, B):
        mask[b, int(torch.randint(1, T, (1,), generator=g)):] = 0            # ragged; sample 0 stays fully valid
    mask[1, 2:] = 0                                                        # one very short history
    if fully_masked is not None:
        mask[fully_masked] = 0
    return mask


def _randomize(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.3 if p.dim() == 1 else 0.08) + (1.0 if "LayerNorm.weight" in n or n.endswith("2.weight") else 0.0))


def _item(p, ckpt=True, B=5, Bg=3, Q=8, F_=5, E=96):
    from unirec_amd.qformer_utils import QFormerForItemRepresentation
    torch.manual_seed(11)
    m = QFormerForItemRepresentation(hidden_size=H, num_hidden_layers=3, num_attention_heads=NH, intermediate_size=I, num_query_tokens=Q,
                                     field_embedding_dim=E, num_fields=F_, dropout=p)
    _randomize(m, 12)
    m.train()
    m.qformer.config.gradient_checkpointing = ckpt
    m.qformer.sample_offset, m.qformer._step = 2, 6
    g = torch.Generator().manual_seed(13)
    inputs = dict(enc=torch.randn((B, F_, E), generator=g), mask=_masks(B, F_, 2), grad_items=Bg)
    nb = B if Bg is None else Bg
    d_out = dict(query_outputs=torch.randn((nb, Q, H), generator=g), item=torch.randn((nb, E), generator=g), rec=torch.randn((nb, F_, E), generator=g))
    return m, inputs, d_out


def _user(p, B=2, Q=8, T=256, E=96, n_pred=2):
    from unirec_amd.user_qformer import UserQFormer
    torch.manual_seed(21)
    m = UserQFormer(hidden_size=H, num_hidden_layers=2, num_attention_heads=NH, intermediate_size=I, num_query_tokens=Q, input_embedding_dim=E,
                    num_item_tokens_to_predict=n_pred, dropout=p)
    _randomize(m, 22)
    m.train()
    m.qformer.sample_offset, m.qformer._step = 3, 4
    g = torch.Generator().manual_seed(23)
    inputs = dict(enc=torch.randn((B, T, E), generator=g), mask=_masks(B, T, None))
    return m, inputs, torch.randn((B, n_pred * E), generator=g)


def _run(build, monkeypatch, mutant=None, **kw):
    m, inputs, d_out = build
    fake = FakeHip(mutant)
    st = QL.run_step(m, monkeypatch, inputs, d_out, hipmod=fake, **kw)
    return m, inputs, d_out, st


def _check(m, inputs, d_out, st):
    return QL.check_step(st, QL.ModelDef(m, "cpu"), inputs, QL.HostMasks(), d_out, verbose=False)


def _first_failure(m, inputs, d_out, st):
    with pytest.raises(QL.LinkFailures) as e:
        _check(m, inputs, d_out, st)
    return list(e.value.failed)


# ---- clean tapes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.2, 0.0], ids=["dropout", "no dropout"])
def test_clean_item_tape_passes(monkeypatch, p):
    m, inputs, d_out, st = _run(_item(p), monkeypatch)
    assert st.info["Bg"] == 3 < st.info["B"] == 5 and st.info["ckpt"] and st.info["step_seed"] == 7 and st.info["row0"] == 2 * 8
    ratios = _check(m, inputs, d_out, st)
    live = [n for n, _ in m.live_named_parameters()]
    assert sum(k.startswith("grad ") for k in ratios) == len(live) and all(st.grads[n] is not None for n in live)
    assert all(st.grads[n] is None for n, _ in m.named_parameters() if n not in live) and len(live) < len(st.grads)
    assert "L1.qc" not in ratios and "L0.qc (re-run)" in ratios and "L2.rerun" in ratios and "hd.others.item" in ratios
    assert ("L0.s.dy" in ratios) == (p > 0.0)


@pytest.mark.parametrize("p", [0.1, 0.0], ids=["dropout", "no dropout"])
def test_clean_user_tape_passes(monkeypatch, p):
    m, inputs, d_out, st = _run(_user(p), monkeypatch)
    ratios = _check(m, inputs, d_out, st)
    assert sum(1 for r in st.tape if r.name == "attn_bwd" and r.kwargs.get("kv_colsum") is not None) == 2, "kv_colsum fused in both cross layers"
    assert "L1.c.dk" in ratios and "uh.da" in ratios and "L0.s.z" in ratios
    assert sum(k.startswith("grad ") for k in ratios) == len(m.live_named_parameters())


def test_clean_eval_forward_passes(monkeypatch):
    m, inputs, _ = _item(0.2, ckpt=False)
    m.eval()
    inputs["grad_items"] = None
    with torch.no_grad():
        st = QL.run_step(m, monkeypatch, inputs, None, hipmod=FakeHip(), keep=False)
    assert st.info["p_h"] == 0.0 and not st.backward
    ratios = QL.check_step(st, QL.ModelDef(m, "cpu"), inputs, QL.HostMasks(), None, verbose=False)
    assert "L0.s.out" in ratios and "L0.s.z" not in ratios and not any(k.startswith("grad ") for k in ratios)


def test_clean_bert_tape_passes(monkeypatch):
    """the free-standing BertModel: per-sample query embeddings (the cast path) and [1, Q, H] (batch_reduce), encoder states with gradient"""
    from unirec_amd.qformer import BertModel
    m0, inputs, d_out = _item(0.2, ckpt=False)
    bert = BertModel(m0.qformer.config)
    _randomize(bert, 31)
    bert.train()
    bert.sample_offset, bert._step = 1, 9
    g = torch.Generator().manual_seed(32)
    for rows in (5, 1):
        inp = dict(enc=inputs["enc"], mask=inputs["mask"], query_embeds=torch.randn((rows, 8, H), generator=g), enc_needs_grad=True)
        d = torch.randn((5, 8, H), generator=g)
        st = QL.run_step(bert, monkeypatch, inp, d, hipmod=FakeHip())
        ratios = QL.check_step(st, QL.ModelDef(bert, "cpu"), inp, QL.HostMasks(), d, verbose=False)
        assert "d_qe" in ratios and "d_enc" in ratios and "d_enc16" in ratios and st.d_qe.shape[0] == rows and st.d_enc.shape == inputs["enc"].shape


# ---- mutants ----------------------------------------------------------------------------------------------------------------------------
ITEM_MUTANTS = {                                             # mutant -> the link that must reject it (first in tape order)
    "cross_reads_other_slot": "L0.c.att",
    "kv_weight_order_swapped": "kv_all",
    "ln_bwd_wrong_site_seed": "L2.f.dy",
    "drop_row0_omitted": "L2.c.dy",
    "drop_batch0_omitted": "L0.s.att",
    "kv_bias_colsum_skipped": "grad qformer.encoder.layer.0.crossattention.self.key.bias",
    "dx_residual_dropped": "L2.dxc",
    "qkv_bias_order": "grad qformer.encoder.layer.2.attention.self.key.bias",
    "batch_reduce_nb_rows_exchanged": "grad query_embeddings",
}


@pytest.mark.parametrize("mutant", sorted(ITEM_MUTANTS))
def test_item_mutant_is_rejected_at_its_own_link(monkeypatch, mutant):
    m, inputs, d_out, st = _run(_item(0.2), monkeypatch, mutant)
    failed = _first_failure(m, inputs, d_out, st)
    assert failed[0] == ITEM_MUTANTS[mutant], failed[:5]


def test_dout_not_cut_to_the_leading_rows_is_rejected(monkeypatch):
    """the backward walks ANOTHER Bg rows of the incoming gradient than the leading ones"""
    m, inputs, d_out = _item(0.2)
    orig = m.qformer._backward_impl
    monkeypatch.setattr(m.qformer, "_backward_impl", lambda S, dout, *a: orig(S, torch.cat([dout[2:], dout[:2]]), *a))
    st = QL.run_step(m, monkeypatch, inputs, d_out, hipmod=FakeHip())
    failed = _first_failure(m, inputs, d_out, st)
    assert failed[0] == "L2.f.dz", failed[:5]


def test_stale_transposes_are_rejected(monkeypatch):
    """BatchedTranspose.run() not re-run after the masters moved: the first step passes, the second is rejected at the transposes"""
    build = _item(0.2)
    m, inputs, d_out = build
    fake = FakeHip("transposes_not_rerun")
    first = QL.run_step(m, monkeypatch, inputs, d_out, hipmod=fake)
    _check(m, inputs, d_out, first)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(2.0)
    second = QL.run_step(m, monkeypatch, inputs, d_out, hipmod=fake)
    assert any(r.name == "cast_f32_to_bf16" and len(r.args) == 2 for r in second.tape), "the masters moved: the shadow cast is on the tape"
    failed = _first_failure(m, inputs, d_out, second)
    assert failed[0] == "prep.transposes", failed[:5]
    fake.mutant = None
    third = QL.run_step(m, monkeypatch, inputs, d_out, hipmod=fake)
    assert not any(k.startswith("prep.shadow") for k in _check(m, inputs, d_out, third)), "the masters did not move again: no shadow cast"


def test_kv_bias_colsum_also_run_when_fused_is_rejected(monkeypatch):
    """the post-loop colsum over dK | dV although the attention backward wrote kv_colsum: a launch the configuration does not prescribe"""
    m, inputs, d_out, st = _run(_user(0.1), monkeypatch)
    at = max(i for i, r in enumerate(st.tape) if r.name == "gemm" and r.kwargs.get("out") is not None and r.kwargs["out"].dtype == F32) + 1
    extra = LL.Rec("colsum", (torch.zeros(4, 4 * H, dtype=BF16),), {"out": torch.zeros(4 * H)}, torch.zeros(4 * H))
    st.tape = st.tape[:at] + [extra] + st.tape[at:]
    with pytest.raises(QL.TapeError, match="colsum"):
        _check(m, inputs, d_out, st)


def test_grouped_output_bound_to_the_wrong_parameter_is_rejected(monkeypatch):
    """the grouped weight-gradient launch on the CPU: the incoming gradient says it lives on the device, the side stream is switched off"""
    from unirec_amd.switches import switches

    class SaysCuda(torch.Tensor):
        is_cuda = True
    monkeypatch.setattr(switches, "qf_dw_stream", False)
    for mutant in (None, "grouped_output_misbound"):
        m, inputs, d_out = _item(0.2, ckpt=False, B=32, Bg=None)
        orig = m.qformer._backward_impl
        monkeypatch.setattr(m.qformer, "_backward_impl", lambda S, dout, *a, orig=orig: orig(S, dout.as_subclass(SaysCuda), *a))
        st = QL.run_step(m, monkeypatch, inputs, d_out, hipmod=FakeHip(mutant))
        assert sum(r.name == "gemm_grouped" for r in st.tape) == 3
        st.grouped = True
        if mutant is None:
            _check(m, inputs, d_out, st)
        else:                                        # layer 2's first neighbours of one shape: crossattention.output.dense and .self.query
            failed = _first_failure(m, inputs, d_out, st)
            assert failed[0] == "grad qformer.encoder.layer.2.crossattention.output.dense.weight", failed[:5]


def test_kv_colsum_is_held_as_its_primitive_test_holds_it(monkeypatch):
    """The few-query dK/dV kernel sums its float32 accumulators before the bf16 store.  Such sums pass the link (the summed attention
    bound of tests/test_gpu_attention_f64.py), and are NOT the column sums of the stored bf16 dK | dV: assert_colsum_close over the
    stored values, the criterion of the post-loop colsum, rejects them."""
    m, inputs, d_out, st = _run(_user(0.1), monkeypatch, "kv_colsum_of_the_f32_accumulators")
    _check(m, inputs, d_out, st)
    r = next(r for r in st.tape if r.name == "attn_bwd" and r.kwargs.get("kv_colsum") is not None)
    stored = torch.cat([r.kwargs[k].reshape(-1, H) for k in ("dk", "dv")], 1).to(F64)
    with pytest.raises(AssertionError):
        ref64.assert_colsum_close(r.kwargs["kv_colsum"], stored.sum(0), stored.sum(0), stored.abs().sum(0), "sums of the stored values")


# ---- tape integrity ---------------------------------------------------------------------------------------------------------------------
def test_unknown_entry_point_is_a_tape_error():
    with pytest.raises(QL.TapeError, match="rmsnorm_fwd"):
        QL.QTape(types.SimpleNamespace(rmsnorm_fwd=lambda *a: None)).rmsnorm_fwd


def test_unconsumed_launch_and_missing_station_are_tape_errors(monkeypatch):
    m, inputs, d_out, st = _run(_user(0.0), monkeypatch)
    tape = list(st.tape)
    st.tape = tape + [LL.Rec("colsum", (torch.zeros(2, 8, dtype=BF16),), {}, torch.zeros(8))]
    with pytest.raises(QL.TapeError, match="consumed by no link"):
        _check(m, inputs, d_out, st)
    st.tape = tape[:-1]
    with pytest.raises(QL.TapeError, match="missing"):
        _check(m, inputs, d_out, st)
    k = next(i for i, r in enumerate(tape) if r.name == "attn_fwd")
    st.tape = tape[:k] + tape[k + 1:]
    with pytest.raises(QL.TapeError, match="attn_fwd is expected"):
        _check(m, inputs, d_out, st)


# ---- the criterion of the f32 products --------------------------------------------------------------------------------------------------
def test_f32_product_floor_needs_the_emulation_term():
    """assert_gemm_f32's 2^-22 |acc| is stated for EXACT products.  A constructed dW whose terms cancel (x, then -x, then a small rest):
    the float32 accumulation of the bf16 products, in the order given, misses that floor by orders of magnitude, while 8 |v32 - v64| +
    2^-20 sum |term| -- what tests/test_gpu_dw_f64.py holds the same kernels to on unit-normal operands -- contains it, and still
    rejects a dropped term."""
    g = torch.Generator().manual_seed(5)
    K, M, N = 512, 8, 8
    dy = _bf(torch.randn((K, M), generator=g))
    x = _bf(torch.randn((K, N), generator=g))
    dy[K // 2:K - 2] = dy[:K // 2 - 2]
    x[K // 2:K - 2] = -x[:K // 2 - 2]                                       # every product appears twice with opposite signs
    r64 = dy.to(F64).t() @ x.to(F64)
    acc = torch.zeros((M, N), dtype=F32)
    for k in range(0, K, 32):                                              # float32 partial sums, K tile by K tile
        acc = acc + dy[k:k + 32].float().t() @ x[k:k + 32].float()
    with pytest.raises(AssertionError):
        ref64.assert_gemm_f32(acc, r64, 1.0, what="exact-product floor")
    ab = dy.to(F64).abs().t() @ x.to(F64).abs()
    r32 = dy.float().t() @ x.float()
    QL._sum_f32(acc, r64, r32, ab, "the emulation's term")
    with pytest.raises(AssertionError):
        QL._sum_f32(acc - dy[0].float()[:, None] * x[0].float()[None, :], r64, r32, ab, "a dropped term")

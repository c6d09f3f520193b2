"""CPU: the link checker of tests/layer_links.py bites.

The REAL Qwen3LoRAModel._forward_impl / _backward_impl run on the CPU over FakeHip, a float32 stand-in for unirec_amd.hip: every entry point
the decoder calls, evaluated with tests/ref64.py's restatements at dtype=F32 (or the same formula in float32 torch) and rounded to bf16
wherever the path stores bf16.  The tape it leaves has exactly the format of a GPU tape, so the checker is exercised as the GPU test uses
it.  The clean tape must pass under every plan the reduced layer reaches; each MUTANT -- one deliberate glue bug inside one launch, whose
wrong output then flows on through the real glue -- must be rejected AT ITS OWN LINK and nowhere else.

Reduced layer: D 128, two heads of 64 over one kv head, I 256, r 8, 2 layers, B 2 x S 24, left padding on sample 0, dropout 0.25, rsLoRA,
injected tokens, a shard offset (row0 != 0)."""
import math
import types

import numpy as np
import pytest
import torch

from oracle import dropout_ref
from tests import layer_links as LL
from tests import ref64

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
B, S, D, NH, NKV, HD, I, R, LAYERS, T, P = 2, 24, 128, 2, 1, 64, 256, 8, 2, 3, 0.25
FIRST = 40                                                    # first special id: the base vocabulary


def _bf(x):
    return x.to(BF16)


class FakeHip:
    """unirec_amd.hip's entry points as the decoder calls them, in float32 torch on the CPU.  mutant: the name of ONE deliberate bug."""
    LORA_RANKS = (8, 16, 32, 64)
    _lib = types.SimpleNamespace(UniRecHipError=RuntimeError)

    def __init__(self, mutant=None, paired=True):
        self.mutant, self.paired, self.n = mutant, paired, {}
        self.mem = {}

    def _count(self, what):
        self.n[what] = self.n.get(what, 0) + 1
        return self.n[what] - 1

    def _is(self, mutant, what, k):
        """count the call under `what`; True when this is call k and the mutant is the one asked for"""
        return self._count(mutant + "/" + what) == k and self.mutant == mutant

    # ---- host answers
    def gemm_swiglu_paired_supported(self, M, I_, K, K2, device=None):
        return self.paired

    def gemm_qkrope_supported(self, *a, **k):
        return False

    def swiglu_pair_rows(self, I_):
        from unirec_amd.hip import swiglu_pair_rows
        return swiglu_pair_rows(I_)

    def lora_bits_ld(self, W):
        return dropout_ref.lora_bits_ld(W)

    # ---- operand preparation
    def cast_f32_to_bf16(self, src, dst=None):
        if dst is None:
            return src.to(BF16)
        dst.copy_(src.to(BF16))
        return dst

    def rope_table(self, S_, hd, theta, device):
        return ref64.rope_table_f32(S_, hd, theta)

    class BatchedTranspose:
        def __init__(self, sources):
            self.sources = sources

        def run(self):
            return [s.t().contiguous() for s in self.sources]

    # ---- dropout planes
    def lora_dropout_bits(self, seed, p, M, W, nad, device, out=None, row0=0):
        if self._is("row0_off_by_one_sample", "bits", 0):
            row0 += S
        words = dropout_ref.lora_words(seed, p, M, W, nad, row0)
        bits = torch.from_numpy(words.view(np.uint8).reshape(nad, M, -1).copy())
        if out is not None:
            out.copy_(bits)
            return out
        return bits

    def _keep(self, bits, W):
        from unirec_amd.hip import lora_bits_to_keep
        return None if bits is None else lora_bits_to_keep(bits, W)

    # ---- forward
    def embed_inject_fwd(self, embed, ids, tok, first):
        out = embed[ids]
        if tok is not None:
            rel = ids - first
            sp = (rel >= 0) & (rel < tok.shape[1])
            out = torch.where(sp[..., None], tok[torch.arange(ids.shape[0])[:, None].expand_as(ids), rel.clamp(0, tok.shape[1] - 1)], out)
        self.mem["x0"] = out.reshape(-1, out.shape[-1])
        return out

    def rmsnorm_fwd(self, x, w, eps):
        out, rstd = ref64.rmsnorm_fwd(x.float(), w, eps, dtype=F32)
        if self._count("rmsnorm_fwd") == 0:
            self.mem["h0"] = _bf(out)
        return _bf(out), rstd

    def lora_project(self, X, U, cols=None, alpha=1.0, bits=None, out=None):
        k = self._count("lora_project")
        keep = self._keep(bits, X.shape[1])
        if self.mutant == "t_o_scale_twice" and k == 1:
            alpha = alpha * self.mem["scale"]
        if self.mutant == "t_gu_without_inverse_keep" and k == 2:
            alpha = alpha * (1.0 - P)
        if self.mutant == "plain_scale_under_rslora" and k == 0:
            alpha = alpha / math.sqrt(R)                                  # alpha / r instead of alpha / sqrt(r)
        if self.mutant == "v_reads_k_plane" and k == 0:
            keep = keep.clone()
            keep[2] = keep[1]
        return _bf(ref64.lora_project(X, U, keep, alpha, cols, dtype=F32))

    def gemm(self, Rm, Sm, *, out=None, alpha=1.0, residual=None, R2=None, S2=None, drop=None, swiglu_bwd=None, swiglu_fwd=None,
             swiglu_paired=None):
        if R2 is not None and residual is None and swiglu_bwd is None and drop is None and out is not None:
            k = self._count("fwd_second_range")
            if k == 0:
                self.mem["S2_first"] = S2
            if self.mutant == "layer1_uses_layer0_B" and k == 2:          # (q|k|v and gate|up of layer 0, then q|k|v of layer 1)
                S2 = self.mem["S2_first"]
        if residual is not None:
            k = self._count("residual")
            if self.mutant == "o_residual_from_h" and k == 0:
                residual = self.mem["h0"]
            if self.mutant == "down_residual_from_x" and k == 1:
                residual = self.mem["x0"]
        acc = Rm.float() @ Sm.float().t()
        if R2 is not None:
            if drop is None:
                acc = acc + R2.float() @ S2.float().t()
            else:
                bits, p, rank = drop
                keep = self._keep(bits, Sm.shape[0]).float()
                for a in range(R2.shape[1] // rank):
                    sl = slice(a * rank, (a + 1) * rank)
                    acc = acc + keep[a] / (1.0 - p) * (R2[:, sl].float() @ S2[:, sl].float().t())
        if swiglu_bwd is not None:
            gu, dgu = swiglu_bwd
            n = acc.shape[1]
            dg, du = ref64.swiglu_bwd(acc, gu[:, :n], gu[:, n:])
            dgu.copy_(torch.cat([_bf(dg.float()), _bf(du.float())], 1))
            return dgu
        if swiglu_paired is not None:                                     # the weight rows came interleaved: back to gate | up
            nat = torch.empty_like(acc)
            nat[:, self.swiglu_pair_rows(acc.shape[1] // 2)] = acc
            acc = nat
        v = alpha * acc
        if residual is not None:
            v = v + residual.float()
        C = _bf(v)
        if out is None:
            out = C
        else:
            out.copy_(C)
        if swiglu_paired is not None:
            n = C.shape[1] // 2
            swiglu_paired.copy_(_bf(ref64.swiglu_fwd(C[:, :n], C[:, n:]).float()))
        if swiglu_fwd is not None:
            gate, act = swiglu_fwd
            act.copy_(_bf(ref64.swiglu_fwd(gate, C).float()))
        return out

    def qknorm_rope_fwd(self, qkv, qw, kw, cos, sin, S_, nq, nkv, hd, eps):
        k = self._count("qknorm_rope_fwd")
        if self.mutant == "q_norm_weight_on_k_heads" and k == 0:
            kw = qw
        if self.mutant == "rope_position_not_wrapped" and k == 0:         # position m instead of m % S: only sample 1 is wrong
            S_ = qkv.shape[0]
            cos, sin = ref64.rope_table_f32(S_, hd, self.mem["theta"])
        o = _bf(ref64.qknorm_rope_fwd(qkv, qw, kw, cos, sin, S_, nq, nkv, hd, eps, dtype=F32)).reshape(qkv.shape[0], -1)
        return o[:, :nq * hd].contiguous(), o[:, nq * hd:].contiguous()

    def attn_fwd(self, q, k, v, *, causal, key_mask=None, out=None):
        mask = key_mask
        if self._is("key_mask_of_one_sample_ignored", "attn_fwd", 0):
            mask = key_mask.clone()
            mask[0] = 1
        o = _bf(ref64.attention_fwd(q, k, v, mask, causal, q.shape[-1] ** -0.5, dtype=F32)[0]).contiguous()
        if out is not None:
            out.copy_(o)
            o = out
        ctx = types.SimpleNamespace(args=None, keep=(q, k, v, key_mask), o=o, stats=None)
        return o, ctx

    def swiglu_fwd(self, gu, I_, out=None):
        act = _bf(ref64.swiglu_fwd(gu[:, :I_], gu[:, I_:]).float())
        if out is None:
            return act
        out.copy_(act)
        return out

    def mean_pool_fwd(self, x):
        return x.float().mean(1), None

    # ---- backward
    def mean_pool_bwd(self, dout, S_):
        return _bf((dout.float() / S_)[:, None, :].expand(dout.shape[0], S_, dout.shape[1])).contiguous()

    def rmsnorm_bwd(self, dout, x, w, rstd, add=None):
        if self._is("dx2_without_add", "rmsnorm_bwd", 1):                 # (0: the final norm, 1: dx2 of layer 1, 2: dx_out of layer 1)
            add = None
        xh = x.float() * rstd[:, None]
        g = dout.float() * w.float()
        dx = rstd[:, None] * (g - xh * (g * xh).mean(-1, keepdim=True))
        return _bf(dx if add is None else dx + add.float())

    def lora_bgrad(self, dy, t, Bt, cols, gB, alpha=1.0, out=None):
        k = self._count("lora_bgrad")
        if self.mutant == "tb_without_scale" and k == 0:
            alpha = 1.0
        tb, dB = ref64.lora_bgrad(dy, t, Bt, cols, alpha, dtype=F32)
        gB.view(-1).copy_(dB)
        if self.mutant == "dB_of_k_and_v_swapped" and k == 3:             # (layer 1: down, gate|up, o, then q|k|v)
            (ck, nk), (cv, nv) = cols[1], cols[2]
            kk, vv = gB[ck:ck + nk].clone(), gB[cv:cv + nv].clone()
            gB[ck:ck + nk], gB[cv:cv + nv] = vv, kk
        return _bf(tb)

    def lora_reduce(self, X, V, out, cols=None, nad=None, alpha=1.0, bits=None, transposed=False, bits_t=None):
        if self._is("dA_without_mask", "lora_reduce", 0):
            bits = None
        r = out.numel() // (X.shape[1] * int(nad))
        out.view(-1).copy_(ref64.lora_reduce(X, V, r, int(nad), self._keep(bits, X.shape[1]), alpha, cols, transposed, dtype=F32))
        return out

    def attn_bwd(self, ctx, dout, dq=None, dk=None, dv=None):
        q, k, v, mask = ctx.keep
        g = ref64.attention_bwd(q, k, v, mask, True, q.shape[-1] ** -0.5, dout, dtype=F32)
        for dst, src in zip((dq, dk, dv), g):
            dst.copy_(_bf(src))
        if self._is("dqkv_v_columns_from_dk", "attn_bwd", 0):
            dv.copy_(dk)
        return dq, dk, dv

    def qknorm_rope_bwd(self, dq, dk, qkv, qw, kw, cos, sin, dqkv, S_, nq, nkv, hd, eps):
        M = dq.shape[0]
        dout = torch.cat([dq.reshape(M, nq, hd), dk.reshape(M, nkv, hd)], 1)
        g = ref64.qknorm_rope_bwd(dout, qkv, qw, kw, cos, sin, S_, nq, nkv, hd, eps)
        dqkv[:, :(nq + nkv) * hd] = _bf(g.float()).reshape(M, -1)

    def inject_bwd(self, dx, ids, first, T_):
        sel = torch.stack([(ids == first + t) for t in range(T_)], 1).float()
        return _bf(sel @ dx.float())


def _model(**cfg):
    from unirec_amd.qwen3 import Qwen3Config, Qwen3LoRAModel
    torch.manual_seed(1234)
    c = Qwen3Config(vocab_size=FIRST + T, hidden_size=D, intermediate_size=I, num_hidden_layers=LAYERS, num_attention_heads=NH,
                    num_key_value_heads=NKV, head_dim=HD, lora_r=R, lora_alpha=32.0, lora_dropout=P, use_rslora=True, initializer_range=0.05, **cfg)
    m = Qwen3LoRAModel(c)
    m.reset_parameters(lora_b_std=0.05)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("norm.weight") or n.endswith("layernorm.weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape))
    m.lora_seed, m._lora_step, m.sample_offset = 99, 3, 5
    return m.train()


def _inputs():
    g = torch.Generator().manual_seed(77)
    ids = torch.randint(0, FIRST, (B, S), generator=g)
    mask = torch.ones((B, S), dtype=torch.uint8)
    mask[0, :7] = 0                                           # left padding on sample 0, sample 1 fully valid
    ids[0, 9], ids[0, 20], ids[1, 2], ids[1, 3], ids[1, 11] = FIRST, FIRST, FIRST + 1, FIRST + 2, FIRST + 1
    tok = torch.randn((B, T, D), generator=g).to(BF16)
    d_pooled = torch.randn((B, D), generator=g)
    return tok, ids, mask, FIRST, d_pooled


def _bits_fn(seed, p, M, W, planes, row0):
    return torch.from_numpy(dropout_ref.lora_words(seed, p, M, W, planes, row0).view(np.uint8).reshape(planes, M, -1).copy())


def _tables_fn(S_, hd, theta):
    return ref64.rope_table_f32(S_, hd, theta)


def _step(monkeypatch, mutant=None, paired=True, backward=True, model=None, **cfg):
    import unirec_amd.packing as packing
    fake = FakeHip(mutant, paired)
    monkeypatch.setattr(packing, "hip", fake)
    m = _model(**cfg) if model is None else model
    fake.mem.update(scale=m._lora_scale(), theta=float(m.config.rope_theta))
    inp = _inputs()
    st = LL.run_step(m, monkeypatch, inp[0], inp[1], inp[2], inp[3], inp[4] if backward else None, hipmod=fake)
    return m, st, (inp if backward else inp[:4] + (None,))


def _check(m, st, inp, **kw):
    return LL.check_step(st, LL.ModelDef(m, "cpu"), inp, _bits_fn, _tables_fn, verbose=False, **kw)


# ---- the clean tape ---------------------------------------------------------------------------------------------------------------
PLANS = {"merged + paired SwiGLU": dict(paired=True), "merged, SwiGLU alone": dict(paired=False),
         "per projection + SwiGLU in the up launch": dict(paired=False, merge_proj=False, swiglu_fwd_fused=True),
         "per projection, SwiGLU alone": dict(paired=False, merge_proj=False)}


@pytest.mark.parametrize("plan", list(PLANS))
def test_clean_tape_passes(monkeypatch, plan):
    from unirec_amd.switches import switches
    kw = dict(PLANS[plan])
    for f in ("merge_proj", "swiglu_fwd_fused"):
        if f in kw:
            monkeypatch.setattr(switches, f, kw.pop(f))
    m, st, inp = _step(monkeypatch, **kw)
    want = {"merged + paired SwiGLU": (True, "pair"), "merged, SwiGLU alone": (True, "alone"),
            "per projection + SwiGLU in the up launch": (False, "up"), "per projection, SwiGLU alone": (False, "alone")}[plan]
    assert (st.plan.merged, st.plan.swiglu) == want and not st.plan.fuse_rope and not st.plan.rope_bwd_in_dq
    ratios = _check(m, st, inp)
    assert sum(k.startswith("grad ") for k in ratios) == 14 * LAYERS and "d_tok" in ratios and "L1.dqkv.v" in ratios
    assert max(ratios.values()) <= 1.0


def test_clean_tape_passes_with_recomputation_and_a_partial_placement(monkeypatch):
    """q and v adapters on layer 1 only; gate|up, act and both RMSNorm outputs rebuilt in the backward"""
    import unirec_amd.packing as packing
    monkeypatch.setattr(packing, "hip", FakeHip())
    m = _model(lora_target_modules=("q_proj", "v_proj"), lora_layers_to_transform=[1])
    m.recompute_mlp, m.keep_norm_outputs = True, False
    m, st, inp = _step(monkeypatch, model=m)
    assert st.recomputed == [True, True] and st.kept_norms == [False, False]
    ratios = _check(m, st, inp)
    assert sum(k.startswith("grad ") for k in ratios) == 4 and "L0.t_qkv" not in ratios and "L1.gu (recomputed)" in ratios


def test_clean_forward_alone_passes(monkeypatch):
    m, st, inp = _step(monkeypatch, backward=False)
    ratios = _check(m, st, inp)
    assert "L1.att" in ratios and not any(k.startswith("grad ") for k in ratios)


# ---- mutants ----------------------------------------------------------------------------------------------------------------------
def _g(i, proj, ab):
    return f"grad layers.{i}.{LL._MODULE[proj]}.{proj}.lora_{ab}.weight"


# mutant -> the links that must fail, the FIRST of them first (None: exactly that one link)
MUTANTS = {
    "o_residual_from_h": ["L0.x2"],
    "down_residual_from_x": ["L0.x3"],
    "t_o_scale_twice": ["L0.t_o"],
    "t_gu_without_inverse_keep": ["L0.t_gu"],
    "plain_scale_under_rslora": ["L0.t_qkv"],
    "v_reads_k_plane": ["L0.t_qkv"],
    # the planes ARE the station; what was computed under them (t, dA, the masked dX) disagrees with the regenerated masks as well
    "row0_off_by_one_sample": ["L0.bits_qkv", "L0.t_qkv", _g(0, "q_proj", "A"), _g(0, "k_proj", "A"), _g(0, "v_proj", "A"), "L0.dh"],
    "q_norm_weight_on_k_heads": ["L0.k_r"],
    "rope_position_not_wrapped": ["L0.q_r", "L0.k_r"],               # one launch makes both
    "key_mask_of_one_sample_ignored": ["L0.att"],
    "dx2_without_add": ["L1.dx2"],
    "dqkv_v_columns_from_dk": ["L1.dv"],
    "tb_without_scale": ["L1.tb_d"],
    "dA_without_mask": [_g(1, "down_proj", "A")],
    "dB_of_k_and_v_swapped": [_g(1, "k_proj", "B"), _g(1, "v_proj", "B")],
    "layer1_uses_layer0_B": ["L1.qkv"],
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutant_is_rejected_at_its_link(monkeypatch, mutant):
    m, st, inp = _step(monkeypatch, mutant=mutant)
    with pytest.raises(LL.LinkFailures) as e:
        _check(m, st, inp)
    failed = list(e.value.failed)
    assert failed[0] == MUTANTS[mutant][0], failed
    assert set(failed) == set(MUTANTS[mutant]), failed


def test_rope_mutant_touches_the_second_sample_only(monkeypatch):
    """the glue error the pooled comparison cannot see: rows of sample 0 carry their right positions"""
    m, st, inp = _step(monkeypatch, mutant="rope_position_not_wrapped")
    clean = _step(monkeypatch)[1]
    a = [r for r in st.tape if r.name == "qknorm_rope_fwd"][0].ret[0]
    b = [r for r in clean.tape if r.name == "qknorm_rope_fwd"][0].ret[0]
    assert torch.equal(a[:S], b[:S]) and not torch.equal(a[S:], b[S:])


def test_a_launch_no_link_consumes_is_refused(monkeypatch):
    m, st, inp = _step(monkeypatch)
    extra = [r for r in st.tape if r.name == "swiglu_fwd"] or [r for r in st.tape if r.name == "lora_project"]
    st.tape.append(extra[0])
    with pytest.raises(LL.TapeError, match="consumed by no link"):
        _check(m, st, inp)
    st.tape.pop()
    k = [n for n, r in enumerate(st.tape) if r.name == "rmsnorm_bwd"][1]
    st.tape.insert(k, st.tape[k])                             # the same launch twice in the middle of the backward
    with pytest.raises(LL.TapeError, match="is expected"):
        _check(m, st, inp)


def test_an_unknown_entry_point_is_refused():
    tape = LL.Tape(types.SimpleNamespace(new_fused_kernel=lambda *a: None, gemm=lambda *a: None))
    tape.gemm
    with pytest.raises(LL.TapeError, match="does not know"):
        tape.new_fused_kernel


def test_a_missing_station_is_refused(monkeypatch):
    m, st, inp = _step(monkeypatch)
    k = [n for n, r in enumerate(st.tape) if r.name == "lora_project"][1]         # t_o of layer 0 never taped
    del st.tape[k]
    with pytest.raises(LL.TapeError, match="L0.t_o"):
        _check(m, st, inp)
    m, st, inp = _step(monkeypatch)
    name = "layers.1.mlp.up_proj.lora_B.weight"
    del st.grads[name]                                         # a gradient nobody published
    with pytest.raises(LL.TapeError, match=name):
        _check(m, st, inp)
    m, st, inp = _step(monkeypatch)
    del st.tape[-1]                                            # the injected-token gradient
    with pytest.raises(LL.TapeError, match="tape ends"):
        _check(m, st, inp)


def test_exact_product_floor_has_no_term_for_float32_accumulation():
    """Why the projections are held with the accumulation term of the random-operand family (2^-20 sum |term| + 8 |v32 - v64|) beside
    assert_gemm_c's bound: on Gaussian operands a float32 accumulation misses assert_gemm_c -- whose floor, 2^-20 |acc|, is stated for
    EXACT products -- on elements whose terms cancel, and ONLY there; with the term it passes, and an operand scaled by 1 + 2^-6 (four
    bf16 ulps of every output) still fails."""
    g = torch.Generator().manual_seed(5)
    Rm, Sm = torch.randn((256, 1024), generator=g).to(BF16), (0.05 * torch.randn((512, 1024), generator=g)).to(BF16)
    a64, a32 = Rm.to(F64) @ Sm.to(F64).t(), Rm.float() @ Sm.float().t()
    ab = Rm.to(F64).abs() @ Sm.to(F64).abs().t()
    C = a32.to(BF16)
    with pytest.raises(AssertionError):
        ref64.assert_gemm_c(C, a64, 1.0)
    err = (C.to(F64) - a64).abs()
    off = err > ref64.bf16_ulp(a64) + 2.0 ** -20 * a64.abs()
    assert 0 < int(off.sum()) < off.numel() // 100
    assert float((a64.abs() / ab)[off].max()) < 2.0 ** -8, "the offenders are the cancelling elements"
    assert float(err[off].max()) <= float((ref64.bf16_ulp(a64) + 8.0 * (a32.to(F64) - a64).abs())[off].max())
    assert LL._lora_bf16(C, a64, a32, ab, "float32 accumulation") <= 1.0
    C2 = (Rm.float() @ (Sm.float() * (1 + 2.0 ** -6)).t()).to(BF16)
    with pytest.raises(AssertionError):
        LL._lora_bf16(C2, a64, a32, ab, "a scaled operand")

"""The decoder layer held LINK BY LINK: every launch of one training step of unirec_amd.qwen3.Qwen3LoRAModel (_forward_impl /
_backward_impl) against the float64 restatement of the operation it is meant to perform (tests/ref64.py), fed with the HIP path's OWN
stored inputs -- no error is propagated across links, so every criterion is the one the primitive tests hold the same kernel to.

Two parts (docs/lab_notes.md section 31):
  Tape        a recording proxy for the name ``hip`` in unirec_amd.qwen3's namespace: function name, clones of every tensor argument AFTER
              the call (outputs written through out=, add=, dqkv= ... carry their values then) and clones of every result.
  check_step  walks the tape in the order the plan in force prescribes, names the outputs (stations), and holds every station against
              a reference built from the MODEL'S DEFINITION (state_dict() rounded to bf16 by torch's CPU conversion, the config's
              lora_alpha / r / use_rslora / eps / theta, keep masks regenerated from lora_dropout_seed, ref64.attention_allowed) and the
              stored activations at the link's input stations.  It never reads fz, the pack, _bcomb, _lora_transposes, _qk_row_perm or a
              scalar argument on the tape: those are the glue under test.  Every launch must be consumed by a link and the stations
              checked must be the stations the plan promises; anything else is a TapeError.
tests/test_layer_links_host.py runs the REAL _forward_impl / _backward_impl on the CPU over a float32 stand-in for the library (ref64's
restatements at dtype=F32, rounded to bf16 wherever the path stores bf16) and shows that the checker passes the clean tape and rejects
deliberate glue bugs at their own links; tests/test_gpu_layer_links.py holds the HIP path.

Criteria (all from tests/ref64.py; no constant is new):
  RMSNorm fwd / bwd                       assert_bf16_rows' bound: 1 bf16 ulp + 2^-18 row max + 8 e32_row
  projections (second K range, residual)  1 bf16 ulp + 2^-20 (sum |term| + |residual|) + 8 |v32 - v64|: assert_gemm_c's bound with the
                                          accumulation term test_gpu_gemm_f64's random-operand family grants the same kernels
                                          (assert_gemm_c itself is stated for EXACT products: its floor 2^-20 |acc| vanishes where
                                          Gaussian terms cancel, and float32 accumulation does not -- test_layer_links_host shows it)
  t_*, tb_*, masked dX                    assert_lora_bf16 with the absolute-term sums
  fused q/k-norm + RoPE                   qkrope_bound (with the float32 emulation's e32); stand-alone pass: 1 ulp + 2^-18 head-row max
  attention                               attention_bounds / assert_attn_bound
  SwiGLU                                  act: 1 ulp, no floor, of silu(gate BITS) * up BITS; dgate | dup as test_swiglu_backward_epilogue_random_operands
  dA / dB                                 assert_colsum_close with their absolute-term sums
  embed / inject, bit planes              bit equality;  mean pool: assert_f32_close (fwd), 1 ulp + 2^-18 row max (bwd)
"""
import math

import numpy as np
import torch

from oracle import dropout_ref
from tests import ref64

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GROUPS = (("qkv", ("q_proj", "k_proj", "v_proj")), ("o", ("o_proj",)), ("gu", ("gate_proj", "up_proj")), ("d", ("down_proj",)))
_MODULE = {"q_proj": "self_attn", "k_proj": "self_attn", "v_proj": "self_attn", "o_proj": "self_attn", "gate_proj": "mlp",
           "up_proj": "mlp", "down_proj": "mlp"}


class TapeError(AssertionError):
    """the tape does not have the shape the plan prescribes: an unknown / extra / missing launch or station"""


class LinkFailures(AssertionError):
    """one or more links exceeded their criterion: .failed = {link name: message} in tape order"""

    def __init__(self, failed, ratios):
        self.failed, self.ratios = failed, ratios
        super().__init__("links off their criterion:\n" + "\n".join(f"  [{k}] {v}" for k, v in failed.items()))


# =================================================================================================================================
# the tape
HOST = {"gemm_qkrope_supported", "gemm_swiglu_paired_supported", "qkrope_perm", "swiglu_pair_rows", "lora_bits_ld", "lora_bits_t_ld",
        "lora_bits_to_keep", "gemm_plan", "attn_plan"}                                   # answered on the host: nothing is launched
PREP = {"cast_f32_to_bf16", "rope_table", "lora_merge"}                                  # operand preparation (first step / after a merge)
STEP = {"embed_inject_fwd", "rmsnorm_fwd", "rmsnorm_lora_fwd", "lora_project", "lora_dropout_bits", "lora_bits_transpose", "gemm",
        "gemm_qkv_rope", "qknorm_rope_fwd", "attn_fwd", "swiglu_fwd", "swiglu_lora_fwd", "mean_pool_fwd", "mean_pool_bwd", "rmsnorm_bwd",
        "lora_bgrad", "lora_reduce", "attn_bwd", "qknorm_rope_bwd", "qknorm_rope_bwd_roped", "qknorm_rope_bwd_roped_k", "inject_bwd"}


class Rec:
    __slots__ = ("name", "args", "kwargs", "ret")

    def __init__(self, name, args, kwargs, ret):
        self.name, self.args, self.kwargs, self.ret = name, args, kwargs, ret

    def __repr__(self):
        return f"<{self.name}>"


class _Ctx:
    """stands for an attention context on the tape: .n = index of the attn_fwd record that made it"""

    def __init__(self, n):
        self.n = n


class _TapedTranspose:
    """hip.BatchedTranspose whose run() goes on the tape (the model keeps the object across steps: run_step re-binds it)"""

    def __init__(self, tape, inner):
        self.tape, self.inner = tape, inner

    def run(self):
        out = self.inner.run()
        self.tape._record("batched_transpose", (list(self.inner.sources),), {}, list(out))
        return out


class Tape:
    """Proxy for the module ``unirec_amd.hip`` (or a stand-in with the same entry points): forwards every call and records the launches."""

    def __init__(self, real, host=None, prep=None, step=None):
        """host / prep / step: the entry-point sets of the link map in force (default: the decoder's, HOST / PREP / STEP)"""
        self.__dict__.update(_real=real, recs=[], _ctxs=[], _host=HOST if host is None else host, _prep=PREP if prep is None else prep,
                             _step=STEP if step is None else step)

    def _snap(self, v):
        if isinstance(v, torch.Tensor):
            return v.detach().clone()
        if isinstance(v, (tuple, list)):
            return type(v)(self._snap(e) for e in v)
        if all(hasattr(v, a) for a in ("args", "keep", "o", "stats")):                   # hip.AttnCtx
            for n, c in self._ctxs:
                if c is v:
                    return _Ctx(n)
            self._ctxs.append((len(self.recs), v))                                        # (kept alive: identities stay unique)
            return _Ctx(len(self.recs))
        return v

    def _record(self, name, a, k, ret):
        if torch.cuda.is_available():
            torch.cuda.synchronize()                                                      # side-stream writers (prefetched planes) included
        self.recs.append(Rec(name, self._snap(a), {n: self._snap(v) for n, v in k.items()}, self._snap(ret)))

    def __getattr__(self, name):
        attr = getattr(self._real, name)
        if name == "BatchedTranspose":
            return lambda sources: _TapedTranspose(self, attr(sources))
        if name in self._host or not callable(attr) or isinstance(attr, type) or name.startswith("_"):
            return attr
        if name not in self._step and name not in self._prep:
            raise TapeError(f"hip.{name}: a launch the link map does not know")

        def call(*a, **k):
            ret = attr(*a, **k)
            self._record(name, a, k, ret)
            return ret
        return call


class Step:
    """one taped step: the tape, what the forward said about itself (plan, dropout step, what it kept), and the step's results"""


def run_step(model, monkeypatch, tok, ids, mask_u8, first, d_pooled=None, prefetch=False, hipmod=None):
    """One step through model._forward_impl / _backward_impl, as _JointFn drives them, with the recording proxy installed around it.
    d_pooled None: the forward alone (keep=True).  prefetch: the bit planes are generated ahead by prefetch_lora_bits (on the tape too)."""
    import unirec_amd.qwen3 as qmod
    real = qmod.hip if hipmod is None else hipmod
    tape = Tape(real)
    st = Step()
    B, S = ids.shape
    lt = getattr(model, "_lt", None)
    if lt is not None:                                   # the cached A^T / B^T launcher of an earlier step: its run() belongs on THIS tape
        model._lt = (lt[0], lt[1], _TapedTranspose(tape, lt[2].inner if isinstance(lt[2], _TapedTranspose) else lt[2]))
    with monkeypatch.context() as mp:
        mp.setattr(qmod, "hip", tape)
        if prefetch:
            model.prefetch_lora_bits(B * S, ids.device, row0=model.first_sample(B) * S)
        st.prefetched = model._bits_pre is not None
        st.packed = sorted(model._bits_pre["packed"]) if st.prefetched else []
        pooled, saved = model._forward_impl(tok, ids, mask_u8, first, keep=True)
        st.plan, st.pdrop, st.lora_step = saved["plan"], saved["pdrop"], saved["step"]
        st.live = saved["pack"] is not None
        st.recomputed = [bool(L.get("mlp_recompute")) for L in saved["layers"]]
        st.kept_norms = ["h" in L for L in saved["layers"]]
        st.pooled, st.d_tok = pooled.detach().clone(), None
        st.backward = d_pooled is not None
        if st.backward:
            d_tok = model._backward_impl(saved, d_pooled)
            st.d_tok = None if d_tok is None else d_tok.detach().clone()
    lt = getattr(model, "_lt", None)
    if lt is not None and isinstance(lt[2], _TapedTranspose):
        model._lt = (lt[0], lt[1], lt[2].inner)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    st.tape = tape.recs
    st.grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if ".lora_" in n and p.grad is not None} if st.backward else {}
    st.B, st.S, st.T = B, S, tok.shape[1]
    return st


# =================================================================================================================================
# the model's definition
class ModelDef:
    """What the references may know: the config, state_dict() (rounded to bf16 by torch's CPU conversion), the dropout seed function and
    the shard's first sample.  weights: a HF-layout state dict to use INSTEAD of the model's (merged weights); live=False: no adapter runs."""

    def __init__(self, model, dev, weights=None, live=True):
        from unirec_amd.qwen3 import normalize_lora_layers, normalize_lora_targets
        c = self.c = model.config
        self.dev = torch.device(dev)
        sd = {k: v.detach().to("cpu", F32) for k, v in (model.state_dict() if weights is None else weights).items()}
        self.sd = sd
        self.live = bool(live and model.use_lora)
        targets = normalize_lora_targets(c.lora_target_modules) if self.live else ()
        layers = set(normalize_lora_layers(c.lora_layers_to_transform, c.num_hidden_layers)) if self.live else set()
        self.on = [tuple(t for t in targets) if i in layers else () for i in range(c.num_hidden_layers)]
        self.r = int(c.lora_r)
        self.s = 0.0 if not self.live else (c.lora_alpha / math.sqrt(c.lora_r) if c.use_rslora else c.lora_alpha / c.lora_r)
        self.eps, self.theta = c.rms_norm_eps, float(c.rope_theta)
        self.D, self.I, self.hd = c.hidden_size, c.intermediate_size, c.head_dim
        self.nq, self.nkv = c.num_attention_heads, c.num_key_value_heads
        self.NQ, self.NKV = self.nq * self.hd, self.nkv * self.hd
        self.seed_of = model.lora_dropout_seed
        self.first_sample = model.first_sample
        self._cache = {}

    def w16(self, key):
        """the tensor `key` of the state dict as the bf16 GEMM operand, on the compute device"""
        if key not in self._cache:
            self._cache[key] = self.sd[key].to(BF16).to(self.dev)
        return self._cache[key]

    def f32(self, key):
        return self.sd[key].to(self.dev)

    def W(self, i, proj):
        return self.w16(f"layers.{i}.{_MODULE[proj]}.{proj}.weight")

    def A(self, i, proj):
        return self.w16(f"layers.{i}.{_MODULE[proj]}.{proj}.lora_A.weight")

    def Bm(self, i, proj):
        return self.w16(f"layers.{i}.{_MODULE[proj]}.{proj}.lora_B.weight")

    def pname(self, i, proj, ab):
        return f"layers.{i}.{_MODULE[proj]}.{proj}.lora_{ab}.weight"

    def group(self, i, g):
        """(input width, [(projection, slot, first output column, width)] of the PRESENT adapters, all (projection, col, width))"""
        widths = {"q_proj": self.NQ, "k_proj": self.NKV, "v_proj": self.NKV, "o_proj": self.D, "gate_proj": self.I, "up_proj": self.I,
                  "down_proj": self.D}
        win = (self.D, self.NQ, self.D, self.I)[g]
        allp, col = [], 0
        for p in GROUPS[g][1]:
            allp.append((p, col, widths[p]))
            col += widths[p]
        present = [(p, j, c0, n) for j, (p, c0, n) in enumerate(allp) if p in self.on[i]]
        return win, present, allp


# =================================================================================================================================
# criteria on the compute device (the formulas of ref64.assert_lora_bf16 / assert_bf16_rows, evaluated where the tensors live, as
# tests/test_gpu_gemm_f64.py does with ref64.assert_ulp_ratio)
def _lora_bf16(got, r64, r32, ab, what):
    return ref64.assert_ulp_ratio(got.to(r64.device), r64, 1, 2.0 ** -20 * ab + 8.0 * (r32.to(F64) - r64).abs(), what)


def _bf16_rows(got, r64, r32, what):
    e32 = (r32.to(F64) - r64).abs().amax(-1, keepdim=True)
    return ref64.assert_ulp_ratio(got.to(r64.device), r64, 1, 2.0 ** -18 * r64.abs().amax(-1, keepdim=True) + 8.0 * e32, what)


def _head_rows(got, r64, hd, what, extra=0.0):
    """the stand-alone q/k-norm + RoPE kernels' criterion: 1 bf16 ulp + 2^-18 max |ref| of the HEAD row (+ extra)"""
    M = r64.shape[0]
    fl = 2.0 ** -18 * r64.reshape(M, -1, hd).abs().amax(-1, keepdim=True).expand(M, r64.shape[1] // hd, hd).reshape(M, -1)
    return ref64.assert_ulp_ratio(got.to(r64.device), r64, 1, fl + extra, what)


def _bits_equal(got, want, what):
    g, w = got.detach().cpu(), want.detach().cpu()
    assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {tuple(g.shape)} {g.dtype} vs {tuple(w.shape)} {w.dtype}"
    if g.dtype in (BF16, F32):
        g, w = g.contiguous().view(torch.int16 if g.dtype == BF16 else torch.int32), w.contiguous().view(torch.int16 if w.dtype == BF16 else torch.int32)
    off = g != w
    assert not off.any(), f"{what}: {int(off.sum())} of {off.numel()} elements differ, first at {tuple(int(v) for v in off.nonzero()[0])}"
    return 0.0


# =================================================================================================================================
# the checker
class _Walk:
    def __init__(self, step, mdef, inputs, bits_fn, tables_fn, qk_rounded):
        self.st, self.m, self.inp = step, mdef, inputs
        self.bits_fn, self.tables_fn, self.qk_rounded = bits_fn, tables_fn, qk_rounded
        self.recs, self.pos = step.tape, 0
        self.failed, self.ratios, self.checked = {}, {}, []
        self.dev = mdef.dev
        self._keep = {}
        self.S, self.B, self.M = step.S, step.B, step.B * step.S
        self.row0 = mdef.first_sample(step.B) * step.S
        self.cos, self.sin = (t.to(self.dev) for t in tables_fn(step.S, mdef.hd, mdef.theta))

    # ---- plumbing
    def hold(self, link, fn):
        """one station: fn() returns the worst error / bound or raises AssertionError"""
        self.checked.append(link)
        try:
            self.ratios[link] = float(fn())
        except TapeError:
            raise
        except AssertionError as e:
            self.failed[link] = str(e).split("\n")[0][:400]

    def prep(self):
        """operand preparation on the tape (first step: the bf16 operands, the RoPE table; every backward: A^T / B^T): each is held to
        what it must be given ITS OWN source, the projections' references then show whether the right operand reached the launch"""
        while self.pos < len(self.recs) and (self.recs[self.pos].name in PREP or self.recs[self.pos].name == "batched_transpose"):
            r, n = self.recs[self.pos], self.pos
            self.pos += 1
            if r.name == "cast_f32_to_bf16":
                self.hold(f"prep.cast#{n}", lambda: _bits_equal(r.ret, r.args[0].to("cpu").to(BF16), "cast_f32_to_bf16"))
            elif r.name == "rope_table":
                self.hold(f"prep.rope_table#{n}", lambda: max(_bits_equal(r.ret[0], self.cos.to(F32), "cos"), _bits_equal(r.ret[1], self.sin.to(F32), "sin")))
            elif r.name == "batched_transpose":
                self.hold(f"prep.transposes#{n}", lambda: max([_bits_equal(o, s.t().contiguous(), "A^T / B^T") for s, o in zip(r.args[0], r.ret)] + [0.0]))
            else:
                self.hold(f"prep.{r.name}#{n}", lambda: 0.0)

    def take(self, name, why):
        self.prep()
        if self.pos >= len(self.recs):
            raise TapeError(f"{why}: the tape ends where hip.{name} is expected (a station is missing)")
        r = self.recs[self.pos]
        if r.name != name:
            raise TapeError(f"{why}: launch {self.pos} is hip.{r.name} where hip.{name} is expected")
        self.pos += 1
        return r

    def d64(self, t):
        return t.to(self.dev).to(F64)

    def keep(self, i, g):
        """uint8 [planes, M, W] on the CPU: the keep flags of group g of layer i regenerated from the model's seed function; None at p = 0"""
        if self.st.pdrop <= 0.0:
            return None
        if (i, g) not in self._keep:
            win, present, _ = self.m.group(i, g)
            planes = present[-1][1] + 1
            bits = self.bits_fn(self.m.seed_of(self.st.lora_step, i, g), self.st.pdrop, self.M, win, planes, self.row0)
            from unirec_amd.hip import lora_bits_to_keep
            self._keep[(i, g)] = (bits.cpu(), lora_bits_to_keep(bits, win).cpu())
        return self._keep[(i, g)]

    def keeps(self, i, g):
        """[present adapters, M, W] keep flags (CPU uint8) or None"""
        if not self.m.group(i, g)[1]:
            return None
        k = self.keep(i, g)
        if k is None:
            return None
        _, present, _ = self.m.group(i, g)
        return k[1][[j for _, j, _, _ in present]]

    def bits_station(self, i, g, rec, tag):
        self.hold(f"L{i}.bits_{GROUPS[g][0]}{tag}", lambda: _bits_equal(rec.ret, self.keep(i, g)[0], f"planes of layer {i} group {g}"))

    def drawn(self, i, g):
        return self.st.pdrop > 0.0 and not self.st.prefetched and bool(self.m.group(i, g)[1])

    # ---- reference pieces
    def prod(self, R, S):
        """(float64 product, float32 product, sum |term|) of R [M, K] and S [N, K] on the compute device"""
        R64, S64 = self.d64(R), self.d64(S)
        return R64 @ S64.t(), (R.to(self.dev).to(F32) @ S.to(self.dev).to(F32).t()), R64.abs() @ S64.abs().t()

    def projection(self, i, g, xin, t, residual=None):
        """v = x W^T + sum_a t_a B_a^T (+ residual) of group g of layer i over ALL its output columns: (v64, v32, sum |term| + |res|)"""
        _, present, allp = self.m.group(i, g)
        W = torch.cat([self.m.W(i, p) for p, _, _ in allp], 0)
        a64, a32, ab = self.prod(xin, W)
        for k, (p, _, c0, n) in enumerate(present):
            b64, b32, bb = self.prod(t[:, k * self.m.r:(k + 1) * self.m.r], self.m.Bm(i, p))
            a64[:, c0:c0 + n] += b64
            a32[:, c0:c0 + n] += b32
            ab[:, c0:c0 + n] += bb
        if residual is not None:
            a64, a32, ab = a64 + self.d64(residual), a32 + residual.to(self.dev).to(F32), ab + self.d64(residual).abs()
        return a64, a32, ab

    def t_link(self, link, i, g, xin, got):
        _, present, _ = self.m.group(i, g)
        U = [self.m.A(i, p).cpu() for p, _, _, _ in present]
        alpha = self.m.s / (1.0 - self.st.pdrop)
        kw = dict(keep=self.keeps(i, g), alpha=alpha)
        x = xin.cpu()
        self.hold(link, lambda: ref64.assert_lora_bf16(got.cpu(), ref64.lora_project(x, U, **kw), ref64.lora_project(x, U, dtype=F32, **kw),
                                                       ref64.lora_project(x, U, absolute=True, **kw), link))

    def norm_link(self, pre, x, wkey, h, rstd):
        w = self.m.f32(wkey)
        r64, r32 = ref64.rmsnorm_fwd(self.d64(x), w, self.m.eps, dtype=F64), ref64.rmsnorm_fwd(x.to(self.dev).to(F32), w, self.m.eps, dtype=F32)
        self.hold(pre, lambda: _bf16_rows(h, r64[0], r32[0], pre))
        if rstd is not None:
            col = lambda t: t.reshape(-1, 1).cpu()      # noqa: E731
            self.hold(pre + ".rstd", lambda: ref64.assert_f32_close(col(rstd), col(r64[1]), col(r32[1]), what=pre + " rstd"))

    def norm_bwd_link(self, link, dout, x, wkey, add, got):
        w = self.sd_cpu(wkey)
        r = [ref64.rmsnorm_bwd(dout.cpu(), x.cpu(), w, self.m.eps, None if add is None else add.cpu(), dtype=dt) for dt in (F64, F32)]
        self.hold(link, lambda: ref64.assert_bf16_rows(got.cpu(), r[0], r[1], link))

    def sd_cpu(self, key):
        return self.m.sd[key]

    def act_link(self, link, gu, act):
        I = self.m.I
        self.hold(link, lambda: ref64.assert_ulp_ratio(act.to(self.dev), ref64.swiglu_fwd(gu[:, :I].to(self.dev), gu[:, I:].to(self.dev)), 1, 0.0, link))

    # ---- forward
    def group_launches(self, i, g, why, merged_kw=None):
        """the projection launch(es) of group g: one (merged, or no adapter in the group) or one per projection; returns (records, out [M, N])"""
        _, present, allp = self.m.group(i, g)
        if self.st.plan.merged or not present:
            r = self.take("gemm", why)
            return [r], r.kwargs["out"]
        rs = [self.take("gemm", f"{why} ({p})") for p, _, _ in allp]
        return rs, torch.cat([r.kwargs["out"] for r in rs], 1)

    def mlp_up(self, i, h2, t_gu, sw, pre):
        """gate|up (+ act where the launch makes it): (gu, act or None)"""
        if sw == "pair":
            r = self.take("gemm", f"L{i}.gu (paired)")
            gu, act = r.kwargs["out"], r.kwargs.get("swiglu_paired")
            if act is None:
                raise TapeError(f"L{i}.gu: the plan says 'pair' and the launch carries no act")
        else:
            rs, gu = self.group_launches(i, 2, f"L{i}.gu")
            act = rs[-1].kwargs["swiglu_fwd"][1] if (sw == "up" and rs[-1].kwargs.get("swiglu_fwd") is not None) else None
            if sw == "up" and act is None:
                raise TapeError(f"L{i}.gu: the plan says 'up' and the up launch carries no act")
        v64, v32, ab = self.projection(i, 2, h2, t_gu)
        self.hold(f"L{i}.gu{pre}", lambda: _lora_bf16(gu, v64, v32, ab, f"L{i}.gu"))
        return gu, act

    def layer_swiglu(self, i):
        sw = self.st.plan.swiglu if self.m.live else "alone"
        _, pgu, _ = self.m.group(i, 2)
        if (sw == "up" and not pgu) or (sw == "lora" and not self.m.group(i, 3)[1]):
            sw = "alone"
        return sw

    def forward(self):
        m, st, plan = self.m, self.st, self.st.plan
        B, S, M, NQ, NKV, hd, I = self.B, self.S, self.M, m.NQ, m.NKV, m.hd, m.I
        tok, ids, mask, first = self.inp[:4]
        self.L = []
        if st.prefetched:
            for i in range(m.c.num_hidden_layers):
                for g in range(4):
                    if m.group(i, g)[1]:
                        self.bits_station(i, g, self.take("lora_dropout_bits", f"prefetched planes L{i} group {g}"), "")
            for (i, g) in st.packed:
                r = self.take("lora_bits_transpose", f"token-packed planes L{i} group {g}")
                self.bits_t_station(i, g, r, full=True)
        # ---- embedding + injection
        x = self.take("embed_inject_fwd", "x").ret.view(M, m.D)
        emb = m.w16("embed_tokens.weight").cpu()
        want = emb[ids.cpu()]
        if st.T:
            rel = ids.cpu() - first
            sp = (rel >= 0) & (rel < st.T)
            want = torch.where(sp[..., None], tok.cpu()[torch.arange(B)[:, None].expand(B, S), rel.clamp(0, st.T - 1)], want)
        self.hold("x", lambda: _bits_equal(x.view(B, S, -1), want, "embed + inject"))
        for i in range(m.c.num_hidden_layers):
            L = {"x": x}
            h, t_qkv = self.norm_and_t(i, 0, x, "h", "t_qkv")
            if plan.fuse_rope:
                q_r, k_r, v, rstd_qk = self.take("gemm_qkv_rope", f"L{i}.q_r").ret
                a64, a32, ab = self.projection(i, 0, h, t_qkv)
                qn, kn = m.f32(f"layers.{i}.self_attn.q_norm.weight"), m.f32(f"layers.{i}.self_attn.k_norm.weight")
                ref = ref64.qkrope_epilogue(a64, qn, kn, self.cos, self.sin, S, NQ, NKV, m.eps)
                un = ref64.qkrope_emulated(a32, qn, kn, self.cos, self.sin, S, NQ, NKV, m.eps, rounded=False)
                self.hold(f"L{i}.q_r", lambda: ref64.assert_ulp_ratio(q_r.to(self.dev), ref[0], 1, ref64.qkrope_bound(ref[0], un[0]), f"L{i}.q_r"))
                self.hold(f"L{i}.k_r", lambda: ref64.assert_ulp_ratio(k_r.to(self.dev), ref[1], 1, ref64.qkrope_bound(ref[1], un[1]), f"L{i}.k_r"))
                vs = slice(NQ + NKV, NQ + 2 * NKV)
                self.hold(f"L{i}.v", lambda: _lora_bf16(v, a64[:, vs], a32[:, vs], ab[:, vs], f"L{i}.v"))
                r32 = ref64.qkrope_epilogue(a32, qn, kn, self.cos, self.sin, S, NQ, NKV, m.eps, dtype=F32)[3]
                col = lambda t: t.reshape(-1, 1).cpu()      # noqa: E731
                self.hold(f"L{i}.rstd_qk", lambda: ref64.assert_f32_close(col(rstd_qk), col(ref[3]), col(r32), scale=ref[3].abs().reshape(-1).cpu(), what=f"L{i}.rstd_qk"))
                L.update(rstd_qk=rstd_qk)
            else:
                _, qkv = self.group_launches(i, 0, f"L{i}.qkv")
                v64, v32, ab = self.projection(i, 0, h, t_qkv)
                self.hold(f"L{i}.qkv", lambda: _lora_bf16(qkv, v64, v32, ab, f"L{i}.qkv"))
                q_r, k_r = self.take("qknorm_rope_fwd", f"L{i}.q_r").ret
                qn, kn = self.sd_cpu(f"layers.{i}.self_attn.q_norm.weight"), self.sd_cpu(f"layers.{i}.self_attn.k_norm.weight")
                ref = ref64.qknorm_rope_fwd(qkv.cpu(), qn, kn, self.cos.cpu(), self.sin.cpu(), S, m.nq, m.nkv, hd, m.eps).reshape(M, -1)
                self.hold(f"L{i}.q_r", lambda: _head_rows(q_r.cpu(), ref[:, :NQ], hd, f"L{i}.q_r"))
                self.hold(f"L{i}.k_r", lambda: _head_rows(k_r.cpu(), ref[:, NQ:], hd, f"L{i}.k_r"))
                v = qkv[:, NQ + NKV:]
                L.update(qkv=qkv)
            r = self.take("attn_fwd", f"L{i}.att")
            att = r.ret[0].reshape(M, NQ)
            L.update(q_r=q_r, k_r=k_r, v=v, att=att, ctx=r.ret[1].n, h=h, t_qkv=t_qkv)
            if not st.backward:
                self.attention_links(i, L, None)
            t_o = None
            if m.group(i, 1)[1]:
                if self.drawn(i, 1):
                    self.bits_station(i, 1, self.take("lora_dropout_bits", f"L{i}.t_o"), "")
                t_o = self.take("lora_project", f"L{i}.t_o").ret
                self.t_link(f"L{i}.t_o", i, 1, att, t_o)
            x2 = self.take("gemm", f"L{i}.x2").ret
            v64, v32, ab = self.projection(i, 1, att, t_o, residual=x)
            self.hold(f"L{i}.x2", lambda v64=v64, v32=v32, ab=ab: _lora_bf16(x2, v64, v32, ab, f"L{i}.x2"))
            h2, t_gu = self.norm_and_t(i, 2, x2, "h2", "t_gu")
            sw = self.layer_swiglu(i)
            gu, act = self.mlp_up(i, h2, t_gu, sw, "")
            t_d = None
            if sw == "lora":
                if self.drawn(i, 3):
                    self.bits_station(i, 3, self.take("lora_dropout_bits", f"L{i}.t_d"), "")
                act, t_d = self.take("swiglu_lora_fwd", f"L{i}.act").ret
            elif sw == "alone":
                act = self.take("swiglu_fwd", f"L{i}.act").ret
            self.act_link(f"L{i}.act", gu, act)
            if m.group(i, 3)[1]:
                if sw != "lora":
                    if self.drawn(i, 3):
                        self.bits_station(i, 3, self.take("lora_dropout_bits", f"L{i}.t_d"), "")
                    t_d = self.take("lora_project", f"L{i}.t_d").ret
                self.t_link(f"L{i}.t_d", i, 3, act, t_d)
            x3 = self.take("gemm", f"L{i}.x3").ret
            v64, v32, ab = self.projection(i, 3, act, t_d, residual=x2)
            self.hold(f"L{i}.x3", lambda v64=v64, v32=v32, ab=ab: _lora_bf16(x3, v64, v32, ab, f"L{i}.x3"))
            L.update(t_o=t_o, x2=x2, h2=h2, t_gu=t_gu, gu=gu, act=act, t_d=t_d, sw=sw)
            self.L.append(L)
            x = x3
        self.xf = x
        last, _ = self.take("rmsnorm_fwd", "last").ret
        self.norm_link("last", x, "norm.weight", last, None)
        pooled = self.take("mean_pool_fwd", "pooled").ret[0]
        l64 = last.cpu().to(F64).view(B, S, -1)
        self.hold("pooled", lambda: ref64.assert_f32_close(pooled.cpu(), l64.mean(1), last.cpu().to(F32).view(B, S, -1).mean(1), what="pooled"))
        self.hold("pooled (returned)", lambda: _bits_equal(st.pooled, pooled, "the step's result is the mean pool's output"))

    def norm_and_t(self, i, g, x, hname, tname):
        """RMSNorm (+ the t of group g, which reads its output) -> (h, t or None)"""
        has = bool(self.m.group(i, g)[1])
        if self.st.plan.fuse_norm and has:
            if self.drawn(i, g):
                self.bits_station(i, g, self.take("lora_dropout_bits", f"L{i}.{tname}"), "")
            h, rstd, t = self.take("rmsnorm_lora_fwd", f"L{i}.{hname}").ret
        else:
            h, rstd = self.take("rmsnorm_fwd", f"L{i}.{hname}").ret
            t = None
            if has:
                if self.drawn(i, g):
                    self.bits_station(i, g, self.take("lora_dropout_bits", f"L{i}.{tname}"), "")
                t = self.take("lora_project", f"L{i}.{tname}").ret
        self.norm_link(f"L{i}.{hname}", x, f"layers.{i}.{'input_layernorm' if g == 0 else 'post_attention_layernorm'}.weight", h, rstd)
        if has:
            self.t_link(f"L{i}.{tname}", i, g, h, t)
        return h, t

    # ---- attention (forward and backward links share one float64 evaluation)
    def attention_links(self, i, L, datt, got_bwd=None):
        m, B, S = self.m, self.B, self.S
        v4 = lambda t, n: t.cpu().reshape(B, S, n, m.hd)      # noqa: E731
        q, k, v = v4(L["q_r"], m.nq), v4(L["k_r"], m.nkv), v4(L["v"], m.nkv)
        mask = self.inp[2]
        mask = None if mask is None else mask.cpu()
        scale = m.hd ** -0.5
        dout = torch.zeros_like(q) if datt is None else v4(datt, m.nq)
        A = ref64.attention_bounds(q, k, v, mask, True, scale, dout, qk_rounded=self.qk_rounded)
        o = ref64.attention_fwd(q, k, v, mask, True, scale)[0]
        self.hold(f"L{i}.att", lambda: ref64.assert_attn_bound(v4(L["att"], m.nq), o, A["o"], f"L{i}.att"))
        if datt is None:
            return None
        ref = dict(zip(("dq", "dk", "dv"), ref64.attention_bwd(q, k, v, mask, True, scale, dout)))
        for n, heads in (("dq", m.nq), ("dk", m.nkv), ("dv", m.nkv)):
            if got_bwd.get(n) is not None:
                self.hold(f"L{i}.{n}", lambda n=n, heads=heads: ref64.assert_attn_bound(v4(got_bwd[n], heads), ref[n], A[n], f"L{i}.{n}"))
        return ref, A

    def roped_bwd(self, link, dout64, A, roped, rstd, wkey, heads, got):
        """the q/k-norm + RoPE backward from the roped outputs over `heads` heads that share the weight `wkey`.  A None: dout64 is a STORED
        bf16 station and the criterion is the stand-alone kernel's (1 ulp + 2^-18 head-row max of the formula over its inputs).  A given:
        the launch fuses the attention backward with it, dout64 is the float64 attention gradient and the attention's bound A (an
        element-wise bound on its error) is carried through the same LINEAR map with absolute values: |d dx| <= rstd (|R^T| A |w| +
        |x^| mean(|R^T| A |w| |x^|)), R^T the rotation's transpose -- added to the stand-alone criterion."""
        M, S, hd = self.M, self.S, self.m.hd
        w = self.sd_cpu(wkey)
        cos, sin = self.cos.cpu(), self.sin.cpu()
        rp, rs = roped.cpu().reshape(M, heads, hd), rstd.cpu().to(F64)
        recon = ref64.qknorm_rope_bwd_from_roped(dout64.reshape(M, heads, hd), rp, rs, w, w, cos, sin, S, 0, heads, hd).reshape(M, -1)
        extra = 0.0
        if A is not None:
            c, s = ref64._cs_rows(cos, sin, M, S, F64)
            a = A.reshape(M, heads, hd).to(F64)
            g = (a * c.abs() + torch.cat([a[..., hd // 2:], a[..., :hd // 2]], -1) * s.abs()) * w.to(F64).abs()
            xh = (ref64._unrotate(rp.to(F64), c, s) / w.to(F64)).abs()
            extra = ((ref64.U_BF16 + ref64.F32_SLACK) * rs[..., None] * (g + xh * (g * xh).mean(-1, keepdim=True))).reshape(M, -1)
        self.hold(link, lambda: _head_rows(got.cpu(), recon, hd, link, extra))

    def bits_t_station(self, i, g, rec, full=False):
        """token-packed planes against the numpy repack of the regenerated row planes"""
        win = self.m.group(i, g)[0]
        bits = self.keep(i, g)[0]
        if not full:
            bits = bits[[j for _, j, _, _ in self.m.group(i, g)[1]]]
        words = bits.contiguous().numpy().view(np.uint32)
        want = torch.from_numpy(dropout_ref.lora_words_transposed(words, win).view(np.int32))
        self.hold(f"L{i}.bits_t_{GROUPS[g][0]}", lambda: _bits_equal(rec.ret, want, f"token-packed planes of layer {i} group {g}"))

    # ---- backward
    def proj_bwd(self, i, g, dy, xin, t, link, tbname, swiglu_gu=None):
        """the adapters' gradients of group g (tb, dB, dA) and dX = dy W + sum_a keep_a / (1 - p) (tb_a A_a): returns the launch's output"""
        m, st, r = self.m, self.st, self.m.r
        win, present, allp = m.group(i, g)
        Wt = torch.cat([m.W(i, p) for p, _, _ in allp], 0).t()                 # [in, out]: S of dX = dy S^T
        tb = None
        if present:
            cols = [(c0, n) for _, _, c0, n in present]
            rec = self.take("lora_bgrad", f"L{i}.{tbname}")
            tb, gB = rec.ret, rec.args[4]
            Bt = [m.Bm(i, p).t().cpu() for p, _, _, _ in present]
            dyc, tc = dy.cpu(), t.cpu()
            ref = [ref64.lora_bgrad(dyc, tc, Bt, cols, alpha=m.s, **kw) for kw in ({}, {"dtype": F32}, {"absolute": True})]
            self.hold(f"L{i}.{tbname}", lambda: ref64.assert_lora_bf16(tb.cpu(), ref[0][0], ref[1][0], ref[2][0], f"L{i}.{tbname}"))
            self.grad_links(i, present, "B", gB, [x[1] for x in ref])
            keeps = self.keeps(i, g)
            if keeps is not None and not st.prefetched_packed(i, g) and st.plan.bits_t and win % 64 == 0:
                self.bits_t_station(i, g, self.take("lora_bits_transpose", f"L{i}.bits_t_{GROUPS[g][0]}"))
            rec = self.take("lora_reduce", f"L{i}.dA of {GROUPS[g][0]}")
            kw = dict(keep=keeps, alpha=1.0 / (1.0 - st.pdrop))
            xc, tbc = xin.cpu(), tb.cpu()
            ref = [ref64.lora_reduce(xc, tbc, r, len(present), **kw, **k2) for k2 in ({}, {"dtype": F32}, {"absolute": True})]
            self.grad_links(i, present, "A", rec.args[2], ref)
        out = self.take("gemm", link).ret
        A = torch.cat([m.A(i, p) for p, _, _, _ in present], 0) if present else torch.zeros((0, win), dtype=BF16, device=self.dev)
        tbd = tb.to(self.dev) if present else torch.zeros((self.M, 0), dtype=BF16, device=self.dev)
        keeps = self.keeps(i, g)
        kd = [torch.ones((), dtype=F64, device=self.dev)] * len(present) if keeps is None else keeps.to(self.dev)
        e = [ref64.lora_masked_epilogue(dy.to(self.dev), Wt, tbd, A, kd, st.pdrop, r, **kw) for kw in ({}, {"dtype": F32}, {"absolute": True})]
        if swiglu_gu is None:
            self.hold(link, lambda: _lora_bf16(out, e[0], e[1], e[2], link))
        else:
            I = m.I
            gate, up = swiglu_gu[:, :I].to(self.dev), swiglu_gu[:, I:].to(self.dev)
            rg, ru = ref64.swiglu_bwd_epilogue(e[0], gate, up)
            fg, fu = ref64.swiglu_bwd_epilogue(torch.ones_like(e[0]), gate, up)
            g32, u32 = ref64.swiglu_bwd_epilogue(e[1], gate, up)
            fl_g = 2.0 ** -18 * (e[0] * up.to(F64)).abs() + 2.0 ** -20 * e[2] * fg.abs() + 8.0 * (g32 - rg).abs()
            fl_u = 2.0 ** -20 * e[2] * fu.abs() + 8.0 * (u32 - ru).abs()
            self.hold(link + ".gate", lambda: ref64.assert_ulp_ratio(out[:, :I].to(self.dev), rg, 1, fl_g, link + " d_gate"))
            self.hold(link + ".up", lambda: ref64.assert_ulp_ratio(out[:, I:].to(self.dev), ru, 1, fl_u, link + " d_up"))
        return out, tb

    def grad_links(self, i, present, ab, taped, ref):
        """dA / dB of the group's present adapters: the published p.grad of every parameter against its slice of the flattened float64
        reduction, and the launch's own output buffer bit-equal to the published gradients laid end to end"""
        off, pub = 0, []
        for p, _, _, _ in present:
            name = self.m.pname(i, p, ab)
            g = self.st.grads.get(name)
            if g is None:
                raise TapeError(f"grad {name}: no gradient was published (a station is missing)")
            n = g.numel()
            sl = slice(off, off + n)
            off += n
            pub.append(g.reshape(-1))
            self.hold(f"grad {name}", lambda g=g, sl=sl, name=name: ref64.assert_colsum_close(g.reshape(-1).cpu(), ref[0][sl], ref[1][sl], ref[2][sl], name))
        self.hold(f"L{i}.d{ab} buffer ({present[0][0]}..)", lambda: _bits_equal(taped.reshape(-1), torch.cat(pub), "the launch's output vs the published gradients"))

    def backward(self):
        m, st, plan = self.m, self.st, self.st.plan
        B, S, M, NQ, NKV, hd, I = self.B, self.S, self.M, m.NQ, m.NKV, m.hd, m.I
        d_pooled = self.inp[4]
        dlast = self.take("mean_pool_bwd", "dlast").ret.view(M, -1)
        ref = (d_pooled.cpu().to(F64) / S)[:, None, :].expand(B, S, m.D).reshape(M, -1)
        self.hold("dlast", lambda: ref64.assert_within_ulps(dlast.cpu(), ref, 1, 2.0 ** -18 * ref64.rowmax(ref), "dlast"))
        dx = self.take("rmsnorm_bwd", "dx_in").ret
        self.norm_bwd_link("dx_in", dlast, self.xf, "norm.weight", None, dx)
        for i in reversed(range(m.c.num_hidden_layers)):
            L = self.L[i]
            x, x2 = L["x"], L["x2"]
            gu, act, h2 = L["gu"], L["act"], L["h2"]
            if not st.kept_norms[i]:
                h2 = self.take("rmsnorm_fwd", f"L{i}.h2 (recomputed)").ret[0]
                self.norm_link(f"L{i}.h2 (recomputed)", x2, f"layers.{i}.post_attention_layernorm.weight", h2, None)
            if st.recomputed[i]:
                gu, act = self.mlp_up(i, h2, L["t_gu"], "pair" if plan.mlp_recompute == "pair" else "merged", " (recomputed)")
                if act is None:
                    act = self.take("swiglu_fwd", f"L{i}.act (recomputed)").kwargs["out"]
                self.act_link(f"L{i}.act (recomputed)", gu, act)
            dgu, _ = self.proj_bwd(i, 3, dx, act, L["t_d"], f"L{i}.dgu", "tb_d", swiglu_gu=gu)
            dh2, _ = self.proj_bwd(i, 2, dgu, h2, L["t_gu"], f"L{i}.dh2", "tb_gu")
            dx2 = self.take("rmsnorm_bwd", f"L{i}.dx2").ret
            self.norm_bwd_link(f"L{i}.dx2", dh2, x2, f"layers.{i}.post_attention_layernorm.weight", dx, dx2)
            datt, _ = self.proj_bwd(i, 1, dx2, L["att"], L["t_o"], f"L{i}.datt", "tb_o")
            rec = self.take("attn_bwd", f"L{i}.dq")
            if not isinstance(rec.args[0], _Ctx) or rec.args[0].n != L["ctx"]:
                raise TapeError(f"L{i}: the attention backward runs on another launch's context")
            kw = rec.kwargs
            qnk, knk = f"layers.{i}.self_attn.q_norm.weight", f"layers.{i}.self_attn.k_norm.weight"
            if not plan.rope_bwd_in_dq:
                got = {"dq": kw["dq"], "dk": kw["dk"], "dv": kw["dv"]}
                self.attention_links(i, L, datt, got)
                dq_r, dk_r, dv = (got[n].reshape(M, -1) for n in ("dq", "dk", "dv"))
                dout = torch.cat([dq_r, dk_r], 1).cpu().to(F64)
                if plan.fuse_rope:
                    dqkv = self.take("qknorm_rope_bwd_roped", f"L{i}.dqkv").args[9]
                    self.roped_bwd(f"L{i}.dqkv.q", dout[:, :NQ], None, L["q_r"], L["rstd_qk"][:, :m.nq], qnk, m.nq, dqkv[:, :NQ])
                    self.roped_bwd(f"L{i}.dqkv.k", dout[:, NQ:], None, L["k_r"], L["rstd_qk"][:, m.nq:], knk, m.nkv, dqkv[:, NQ:NQ + NKV])
                else:
                    dqkv = self.take("qknorm_rope_bwd", f"L{i}.dqkv").args[7]
                    r64 = ref64.qknorm_rope_bwd(dout.reshape(M, -1, hd), L["qkv"].cpu(), self.sd_cpu(qnk), self.sd_cpu(knk), self.cos.cpu(), self.sin.cpu(),
                                                S, m.nq, m.nkv, hd, m.eps).reshape(M, -1)
                    self.hold(f"L{i}.dqkv.q", lambda: _head_rows(dqkv[:, :NQ].cpu(), r64[:, :NQ], hd, f"L{i}.dqkv.q"))
                    self.hold(f"L{i}.dqkv.k", lambda: _head_rows(dqkv[:, NQ:NQ + NKV].cpu(), r64[:, NQ:], hd, f"L{i}.dqkv.k"))
                self.hold(f"L{i}.dqkv.v", lambda: _bits_equal(dqkv[:, NQ + NKV:], dv, "the v columns of dqkv are the attention's dv"))
            elif plan.fuse_rope:
                if kw.get("rope_q") is None or (plan.rope_k_in_dkv and kw.get("rope_k") is None):
                    raise TapeError(f"L{i}: the plan carries the RoPE backward in the attention backward and the launch does not")
                dq_raw = kw["rope_q"][-1]
                got = {"dv": kw["dv"]} if plan.rope_k_in_dkv else {"dv": kw["dv"], "dk": kw["dk"]}
                ref, A = self.attention_links(i, L, datt, got)
                flat = lambda t: t.reshape(M, -1)      # noqa: E731
                self.roped_bwd(f"L{i}.dqkv.q", flat(ref["dq"]), flat(A["dq"]), L["q_r"], L["rstd_qk"][:, :m.nq], qnk, m.nq, dq_raw)
                if plan.rope_k_in_dkv:
                    dk_raw = kw["rope_k"][-1]
                    self.roped_bwd(f"L{i}.dqkv.k", flat(ref["dk"]), flat(A["dk"]), L["k_r"], L["rstd_qk"][:, m.nq:], knk, m.nkv, dk_raw)
                else:
                    dk_raw = self.take("qknorm_rope_bwd_roped_k", f"L{i}.dqkv.k").args[7]
                    self.roped_bwd(f"L{i}.dqkv.k", flat(kw["dk"]).cpu().to(F64), None, L["k_r"], L["rstd_qk"][:, m.nq:], knk, m.nkv, dk_raw)
                dqkv = torch.cat([dq_raw, dk_raw, kw["dv"].reshape(M, -1)], 1)
            else:
                raise TapeError("the q heads' RoPE backward inside the dQ kernel FROM THE RAW projection (switches.rope_bwd_fused = True) is not mapped")
            h = L["h"]
            if not st.kept_norms[i]:
                h = self.take("rmsnorm_fwd", f"L{i}.h (recomputed)").ret[0]
                self.norm_link(f"L{i}.h (recomputed)", x, f"layers.{i}.input_layernorm.weight", h, None)
            dh, _ = self.proj_bwd(i, 0, dqkv, h, L["t_qkv"], f"L{i}.dh", "tb_qkv")
            dx = self.take("rmsnorm_bwd", f"L{i}.dx_out").ret
            self.norm_bwd_link(f"L{i}.dx_out", dh, x, f"layers.{i}.input_layernorm.weight", dx2, dx)
        if st.T:
            d_tok = self.take("inject_bwd", "d_tok").ret
            ids, first = self.inp[1].cpu(), self.inp[3]
            dx3 = dx.cpu().view(B, S, -1)
            sel = torch.stack([(ids == first + t) for t in range(st.T)], 1).to(F64)             # [B, T, S]
            r64, r32, ab = sel @ dx3.to(F64), (sel.to(F32) @ dx3.to(F32)), sel @ dx3.to(F64).abs()
            self.hold("d_tok", lambda: ref64.assert_lora_bf16(d_tok.cpu(), r64, r32, ab, "d_tok"))
            self.hold("d_tok (returned)", lambda: _bits_equal(st.d_tok, d_tok, "the step's result is inject_bwd's output"))
        extra = set(st.grads) - {k[5:] for k in self.checked if k.startswith("grad ")}
        if extra:
            raise TapeError(f"gradients were published that no link produced: {sorted(extra)[:4]}")


def expected_stations(step, mdef):
    """the stations the plan in force promises (prep.*, bits planes and the (returned) identities aside), written from the plan alone"""
    plan, out = step.plan, ["x", "last", "pooled"]
    for i in range(mdef.c.num_hidden_layers):
        has = [bool(mdef.group(i, g)[1]) for g in range(4)]
        out += [f"L{i}.{n}" for n in ("h", "h.rstd", "q_r", "k_r", "att", "x2", "h2", "h2.rstd", "gu", "act", "x3")]
        out += [f"L{i}.v", f"L{i}.rstd_qk"] if plan.fuse_rope else [f"L{i}.qkv"]
        out += [f"L{i}.t_{GROUPS[g][0]}" for g in range(4) if has[g]]
        if not step.backward:
            continue
        out += [f"L{i}.{n}" for n in ("dgu.gate", "dgu.up", "dh2", "dx2", "datt", "dv", "dqkv.q", "dqkv.k", "dh", "dx_out")]
        out += [f"L{i}.tb_{GROUPS[g][0]}" for g in range(4) if has[g]]
        out += [f"grad {mdef.pname(i, p, ab)}" for p in mdef.on[i] for ab in "AB"]
        if not plan.rope_bwd_in_dq:
            out += [f"L{i}.dq", f"L{i}.dk", f"L{i}.dqkv.v"]
        elif not plan.rope_k_in_dkv:
            out += [f"L{i}.dk"]
        if not step.kept_norms[i]:
            out += [f"L{i}.h (recomputed)", f"L{i}.h2 (recomputed)"]
        if step.recomputed[i]:
            out += [f"L{i}.gu (recomputed)", f"L{i}.act (recomputed)"]
    if step.backward:
        out += ["dlast", "dx_in"] + (["d_tok"] if step.T else [])
    return set(out)


def _aux(name):
    return name.startswith("prep.") or ".bits_" in name or name.endswith("(returned)") or " buffer (" in name


def check_step(step, mdef, inputs, bits_fn, tables_fn, qk_rounded=False, verbose=True):
    """Hold every station of a taped step.  inputs = (tok bf16 [B, T, D], ids, mask_u8 or None, first_special_id, d_pooled f32 or None);
    bits_fn(seed, p, M, W, planes, row0) -> the dropped-flag planes uint8 [planes, M, ld]; tables_fn(S, hd, theta) -> (cos, sin) f32.
    Returns {station: worst error / bound}; raises TapeError (shape of the tape) or LinkFailures (.failed in tape order)."""
    step.prefetched_packed = lambda i, g: step.prefetched and (i, g) in step.packed
    w = _Walk(step, mdef, inputs, bits_fn, tables_fn, qk_rounded)
    w.forward()
    if step.backward:
        w.backward()
    w.prep()
    if w.pos != len(w.recs):
        raise TapeError(f"launch {w.pos} of {len(w.recs)} (hip.{w.recs[w.pos].name}) is consumed by no link")
    got, want = {k for k in w.checked if not _aux(k)}, expected_stations(step, mdef)
    if got != want:
        raise TapeError(f"stations checked != stations the plan promises: missing {sorted(want - got)[:6]}, unexpected {sorted(got - want)[:6]}")
    if verbose:
        for k in w.checked:
            print(f"[ratio] {k}: {w.ratios.get(k, float('nan')):.4f}" + ("   <-- FAILED" if k in w.failed else ""))
    if w.failed:
        raise LinkFailures(w.failed, w.ratios)
    return w.ratios

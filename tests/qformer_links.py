"""The Q-Former held LINK BY LINK: every launch of one step of unirec_amd.qformer.BertModel (_forward_impl / _layer_forward / _backward_impl)
and of the wrappers' head functions (_ItemHeadsFn, _UserHeadFn) against the float64 restatement of the operation it is meant to perform
(tests/ref64.py), fed with the HIP path's OWN stored inputs -- no error is propagated across links.  The machinery is tests/layer_links.py's
(Tape, Rec, _Ctx, _TapedTranspose, TapeError, LinkFailures and the device-side criterion helpers); docs/lab_notes.md section 35.

  QTape       the recording proxy for the name ``hip`` in unirec_amd.qformer, .qformer_utils, .user_qformer and .packing (the master -> bf16
              shadow cast of ParamPack.refresh_shadow is operand preparation and is on the tape).  layernorm_bwd(defer_reduce=True): the
              returned finish() is wrapped, its effect on dgamma / dbeta / dbias is a record of its own ("ln_finish").  attn_ctx_prefix is
              answered on the host; the context it returns stands for the forward launch of the context it was cut from.
  run_step    drives a QFormerForItemRepresentation, a UserQFormer or a free-standing BertModel the way their autograd nodes do.
  check_step  walks the tape in the order the code prescribes for the configuration in force, names every output (station) and holds it
              against a reference built from the MODEL'S DEFINITION: state_dict() rounded to bf16 by torch's CPU conversion, the config
              (H, nh, I, eps, cross_attention_freq, dropout probabilities), model._seed as a function, the shard's first sample, and the
              stored activations at the link's input stations.  It never reads the pack, fused16 / fused32 / fusedg, _wt, the layout of
              kv_all as the model sees it, or a scalar / seed argument on the tape: those are the glue under test.  The FUSED orders
              (q|k|v, k0|v0|k1|v1 ..., the transposes' list) are the reference's own.  Every launch is consumed by exactly one link, the
              stations checked are the ones the configuration promises (expected_stations), and every live parameter's published .grad
              is bit-equal to exactly one gradient station; dead parameters have grad None.

Criteria (all from tests/ref64.py; no constant is new):
  LayerNorm fwd                 z_save bit-equal to bf16(y + residual), under pre-dropout 1 ulp + 8 e32_row with the dropped elements the
                                residual's bits; out: assert_bf16_rows (1 ulp + 2^-18 row max + 8 e32_row, the unmasked row's scale under
                                post-dropout); mean, rstd: assert_f32_close -- as tests/test_gpu_norm_f64.py.  A first run that saves no z
                                under pre-dropout (gradient checkpointing) is held through its re-run: bit-equal outputs, the re-run's links
  LayerNorm bwd                 dz, dy: assert_bf16_rows; dgamma / dbeta / dbias: assert_colsum_close with their absolute-term sums
  bf16-output GEMMs             layer_links' projection bound: 1 bf16 ulp + 2^-20 (sum |term| + |bias| + |residual|) + 8 |v32 - v64|;
                                gelu_out: assert_gelu_close of the stored C; gelu_grad_aux: assert_gemm_gelu_grad's bound (1 ulp +
                                2^-18 |pre| + 2^-20 mag |gelu'|) with the same float32-emulation term 8 |pre32 - pre64| |gelu'|
  f32-output GEMMs, every dW    assert_colsum_close's bound, 8 |v32 - v64| + 2^-20 sum |term|, evaluated on the compute device: the criterion
                                test_gpu_dw_f64.py holds ur_gemm / ur_gemm_grouped to on unit-normal operands.  assert_gemm_f32's
                                2^-22 |acc| is stated for EXACT products; its floor vanishes where Gaussian terms cancel and float32
                                accumulation does not (tests/test_qformer_links_host.py constructs the example, as test_layer_links_host
                                does for assert_gemm_c): the term comes from the float32 emulation, not from a fitted constant
  attention fwd / dQ / dK / dV  attention_bounds / assert_attn_bound (key mask, regenerated keep masks)
  colsum, batch_reduce          assert_colsum_close with absolute-term sums (the terms are given exactly: ref32 = ref64)
  kv_colsum                     the float64 column sums of the float64 dK | dV within the summed attention bound A, as
                                test_few_query_dkv_and_kv_colsum (test_gpu_attention_f64.py) holds it: the few-query kernel sums its float32
                                accumulators BEFORE the bf16 store, so the sums of the STORED dK | dV (assert_colsum_close over them, as the
                                post-loop colsum is held) are another quantity -- tests/test_qformer_links_host.py shows it
  casts, add_bf16, transposes   bit equality; a transpose station equals the bf16 state-dict weight(s) transposed, in the reference's order
  mean_pool_fwd (bf16)          assert_bf16_rows;  mean_pool_bwd: 1 ulp + 2^-18 row max;  gelu_bwd: 1 ulp + 2^-18 |dy|
  field_projection_*            out: assert_f32_close; drec: assert_bf16_rows; dWf / dbf: assert_colsum_close (fproj_fast_dwf_terms where the
                                Q = 32, F <= 16, E % 128 == 0 kernel runs) -- as tests/test_gpu_dw_f64.py
"""
import types

import torch

from tests import layer_links as LL
from tests import ref64
from tests.layer_links import LinkFailures, TapeError, _bits_equal, _lora_bf16  # noqa: F401

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64

HOST = {"attn_ctx_prefix", "attn_bwd_kv_colsum_supported", "gemm_plan", "gemm_plan_args", "attn_plan", "dropout_keep", "attn_dropout_keep",
        "GEMM_MAX_GROUPS"}
STEP = {"layernorm_fwd", "layernorm_bwd", "gemm", "gemm_grouped", "attn_fwd", "attn_bwd", "colsum", "batch_reduce", "cast_f32_to_bf16",
        "cast_bf16_to_f32", "add_bf16", "mean_pool_fwd", "mean_pool_bwd", "field_projection_fwd", "field_projection_bwd", "gelu_bwd"}
MODULES = ("unirec_amd.qformer", "unirec_amd.qformer_utils", "unirec_amd.user_qformer", "unirec_amd.packing")
EMB_LAYER, EMB_SITE = 1023, 0                    # the embedding LayerNorm's dropout site (oracle/dropout_ref.py restates it)


class QTape(LL.Tape):
    def __init__(self, real):
        super().__init__(real, host=HOST, prep=set(), step=STEP)

    def __getattr__(self, name):
        if name == "attn_ctx_prefix":
            real = getattr(self._real, name)

            def prefix(ctx, Bg):
                new = real(ctx, Bg)
                self._snap(ctx)
                self._ctxs.append((next(n for n, c in self._ctxs if c is ctx), new))       # stands for the same forward launch
                return new
            return prefix
        if name == "layernorm_bwd":
            real = getattr(self._real, name)

            def call(*a, **k):
                ret = real(*a, **k)
                if not k.get("defer_reduce"):
                    self._record(name, a, k, ret)
                    return ret
                dz, dy, fin = ret
                self._record(name, a, k, (dz, dy))
                sums = (a[5], a[6], a[7] if len(a) > 7 else k.get("dbias"))

                def finish():
                    fin()
                    self._record("ln_finish", sums, {}, None)
                finish.scratch = fin.scratch
                return dz, dy, finish
            return call
        return super().__getattr__(name)


# =================================================================================================================================
# one step
def _kind(model):
    return "item" if hasattr(model, "item_representation_head") else ("user" if hasattr(model, "prediction_head") else "bert")


def run_step(model, monkeypatch, inputs, d_out=None, hipmod=None, taped=True, keep=True):
    """One step of `model`, driven as its autograd nodes drive it, with the recording proxy installed around it (taped=False: the same
    calls on the library itself -- the side stream's ordering is then the code's own).
    inputs: dict(enc [B, T, E], mask [B, T] or None, grad_items (item; None = all), query_embeds (free-standing BertModel),
    enc_needs_grad (BertModel)).  d_out: item dict(query_outputs f32 [Bg, Q, H], item f32 [Bg, E], rec f32 [Bg, F, E]); user f32
    [B, n_pred * E]; BertModel f32 [B, Q, H]; None: the forward alone.  keep=False: the no-grad forward (nothing is saved)."""
    import importlib
    import unirec_amd.qformer as qmod
    from unirec_amd.qformer_utils import _ItemHeadsFn
    from unirec_amd.switches import switches
    from unirec_amd.user_qformer import _UserHeadFn
    kind = _kind(model)
    bert = model if kind == "bert" else model.qformer
    real = qmod.hip if hipmod is None else hipmod
    tape = QTape(real) if taped else real
    st = LL.Step()
    st.kind, st.backward, st.keep, st.wt = kind, d_out is not None, keep, bool(switches.qf_wt)
    enc, mask = inputs["enc"], inputs.get("mask")
    B = enc.shape[0]
    qe = model.query_embeddings.detach() if kind != "bert" else inputs["query_embeds"].detach()
    mask_u8 = None if mask is None else (mask != 0).to(torch.uint8).contiguous()
    Bg = inputs.get("grad_items")
    pack = model._ensure_pack(enc.device)
    pack.clear_grads()
    for p in model.parameters():
        p.grad = None
    wt = getattr(bert, "_wt", None)
    rebound = wt is not None and taped
    if rebound:                                          # the cached W^T launcher of an earlier step: its run() belongs on THIS tape
        inner = wt[3].inner if isinstance(wt[3], LL._TapedTranspose) else wt[3]
        bert._wt = wt[:3] + (LL._TapedTranspose(tape, inner),)
    fake = lambda: types.SimpleNamespace(set_materialize_grads=lambda b: None)      # noqa: E731
    with monkeypatch.context() as mp:
        for mod in MODULES:
            mp.setattr(importlib.import_module(mod), "hip", tape)
        step_before = bert._step
        h, S = bert._forward_impl(qe, enc.detach(), mask_u8, B, keep=keep, grad_items=None if (Bg is None or Bg == B) else int(Bg))
        p_h, p_a = bert._drop()
        b0 = int(bert.sample_offset) if bert.sample_offset is not None else int(bert.dp_rank) * B
        st.info = dict(B=B, Bg=B, ckpt=False, step_seed=bert._step, row0=b0 * qe.shape[1], b0=b0, p_h=p_h, p_a=p_a) if S is None else \
            {k: S[k] for k in ("B", "Bg", "ckpt", "step_seed", "row0", "b0", "p_h", "p_a")}
        st.step_before = step_before
        st.side = bool(st.backward and switches.qf_dw_stream and enc.is_cuda and st.info["Bg"] * qe.shape[1] <= qmod._DW_SIDE_MAX_ROWS)
        st.grouped = bool(st.backward and switches.qf_dw_grouped and enc.is_cuda and st.info["Bg"] * qe.shape[1] >= 256)
        nb = st.info["Bg"]
        st.out = {"h": h.detach().clone()}
        st.d_qe = st.d_enc = None
        if kind == "item":
            ctx = fake()
            item, rec = _ItemHeadsFn.forward(ctx, model, h[:nb])
            st.out.update(item=item.detach().clone(), rec=rec.detach().clone())
            if nb < B:
                st.out["other_item"] = _ItemHeadsFn.forward(fake(), model, h[nb:].detach())[0].detach().clone()
            st.out["query_outputs"] = tape.cast_bf16_to_f32(h[:nb]).detach().clone()
            if st.backward:
                dh = _ItemHeadsFn.backward(ctx, d_out["item"], d_out["rec"])[1]
                dq16 = tape.cast_f32_to_bf16(d_out["query_outputs"].contiguous())
                dsum = dq16 + dh                                                   # autograd's own accumulation of the two bf16 gradients of h
                if nb < B:
                    dsum = torch.cat([dsum, torch.zeros((B - nb,) + tuple(dsum.shape[1:]), dtype=BF16, device=dsum.device)])
                bert._backward_impl(S, dsum, False, "query_embeddings")
        elif kind == "user":
            ctx = fake()
            flat = _UserHeadFn.forward(ctx, model, h)
            st.out["flat"] = flat.detach().clone()
            if st.backward:
                dh = _UserHeadFn.backward(ctx, d_out)[1]
                bert._backward_impl(S, dh, False, "query_embeddings")
        else:
            st.out["last_hidden_state"] = tape.cast_bf16_to_f32(h).detach().clone()
            if st.backward:
                d16 = tape.cast_f32_to_bf16(d_out.contiguous())
                d_qe, d_enc = bert._backward_impl(S, d16, bool(inputs.get("enc_needs_grad")), None)
                st.d_qe = None if d_qe is None else d_qe.detach().clone()
                st.d_enc = None if d_enc is None else d_enc.detach().clone()
    wt = getattr(bert, "_wt", None)
    if wt is not None and isinstance(wt[3], LL._TapedTranspose):
        bert._wt = wt[:3] + (wt[3].inner,)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    st.tape = tape.recs if taped else []
    st.ctxs = list(tape._ctxs) if taped else []          # (index of the attn_fwd record, the library's own context): for hip.attn_plan queries
    st.grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}
    return st


# =================================================================================================================================
# the model's definition
class ModelDef:
    """What the references may know: the config, state_dict() (weights rounded to bf16 by torch's CPU conversion), model._seed and the names
    of the live parameters."""

    def __init__(self, model, dev):
        self.kind = _kind(model)
        bert = model if self.kind == "bert" else model.qformer
        c = self.c = bert.config
        self.pre = "" if self.kind == "bert" else "qformer."
        self.dev = torch.device(dev)
        self.sd = {k: v.detach().to("cpu", F32) for k, v in model.state_dict().items()}
        self.H, self.nh, self.I, self.eps, self.L = c.hidden_size, c.num_attention_heads, c.intermediate_size, c.layer_norm_eps, c.num_hidden_layers
        self.dh, self.E = self.H // self.nh, c.encoder_width
        self.cross = [bool(c.add_cross_attention and i % c.cross_attention_freq == 0) for i in range(self.L)]
        self.seed_of = bert._seed
        self.live = [n for n, _ in model.live_named_parameters()]
        self.names = [n for n, _ in model.named_parameters()]
        self.head_eps = model.prediction_head[2].eps if self.kind == "user" else None
        self._cache = {}

    def w16(self, *keys):
        """the weights `keys` of the state dict, stacked in this order, as the bf16 GEMM operand on the compute device"""
        if keys not in self._cache:
            self._cache[keys] = torch.cat([self.sd[k].to(BF16) for k in keys], 0).to(self.dev)
        return self._cache[keys]

    def f32(self, *keys):
        return torch.cat([self.sd[k] for k in keys], 0)

    def lp(self, i):
        return f"{self.pre}encoder.layer.{i}."


class HostMasks:
    """keep masks from oracle.dropout_ref (CPU)"""

    def hidden(self, seed, p, rows, H, row0):
        from oracle import dropout_ref
        return torch.from_numpy(dropout_ref.hidden_keep(seed, p, rows, H, row0).copy())

    def attn(self, seed, p, B, nh, Sq, Sk, b0):
        from oracle import dropout_ref
        return torch.from_numpy(dropout_ref.attn_keep(seed, p, B, nh, Sq, Sk, b0).copy())


# =================================================================================================================================
# criteria on the compute device
def _sum_f32(got, r64, r32, ab, what):
    """ref64.assert_colsum_close's bound where the tensors live: |got - ref64| <= 8 |ref32 - ref64| + 2^-20 sum |term|; the worst ratio"""
    g = got.to(r64.device).to(F64).reshape(r64.shape)
    assert torch.isfinite(g).all(), f"{what}: non-finite outputs"
    err, bound = (g - r64).abs(), 8.0 * (r32.to(F64) - r64).abs() + 2.0 ** -20 * ab
    off = err > bound
    if off.any():
        i = tuple(int(v) for v in off.nonzero()[0])
        raise AssertionError(f"{what}: {int(off.sum())} of {err.numel()} sums exceed 8 e32 + 2^-20 sum |term|; first at {i}: got {g[i].item()!r}, "
                             f"reference {r64[i].item()!r}, error {err[i].item():.3e}, allowed {bound[i].item():.3e}")
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0


def _col(t):
    return t.detach().cpu().reshape(-1, 1)


def _same(a, b, what):
    return _bits_equal(a.contiguous(), b.contiguous(), what)


# =================================================================================================================================
# the checker
class _Walk:
    def __init__(self, step, mdef, inputs, masks, d_out):
        self.st, self.m, self.inp, self.masks, self.d_out = step, mdef, inputs, masks, d_out
        self.recs, self.pos = step.tape, 0
        self.failed, self.ratios, self.checked = {}, {}, []
        self.dev = mdef.dev
        self.gst = {}                                                        # gradient stations: parameter name -> the launch's output
        I = step.info
        self.B, self.Bg, self.p_h, self.p_a, self.row0, self.b0, self.step_seed = I["B"], I["Bg"], I["p_h"], I["p_a"], I["row0"], I["b0"], I["step_seed"]
        self.ckpt, self.tag = I["ckpt"], ""

    # ---- plumbing
    def hold(self, link, fn):
        link += self.tag                                                     # " (re-run)" while a checkpointed layer is rebuilt
        self.checked.append(link)
        try:
            self.ratios[link] = float(fn())
        except TapeError:
            raise
        except AssertionError as e:
            self.failed[link] = str(e).split("\n")[0][:400]

    def take(self, name, why):
        if self.pos >= len(self.recs):
            raise TapeError(f"{why}: the tape ends where hip.{name} is expected (a station is missing)")
        r = self.recs[self.pos]
        if r.name != name:
            raise TapeError(f"{why}: launch {self.pos} is hip.{r.name} where hip.{name} is expected")
        self.pos += 1
        return r

    def peek(self):
        return self.recs[self.pos].name if self.pos < len(self.recs) else None

    def d64(self, t):
        return t.to(self.dev).to(F64)

    def seed(self, layer, site):
        return self.m.seed_of(layer, site, self.step_seed)

    def hkeep(self, layer, site, rows, p):
        return self.masks.hidden(self.seed(layer, site), p, rows, self.m.H, self.row0) if p > 0.0 else None

    # ---- GEMM references
    def prod(self, R, S, bias=None, residual=None):
        """(v64, v32, sum |term|) of R [M, K] S[N, K]^T (+ bias [N]) (+ residual [M, N]) on the compute device"""
        R64, S64 = self.d64(R), self.d64(S)
        v64, v32, ab = R64 @ S64.t(), R.to(self.dev).to(F32) @ S.to(self.dev).to(F32).t(), R64.abs() @ S64.abs().t()
        if bias is not None:
            b = bias.to(self.dev)
            v64, v32, ab = v64 + b.to(F64), v32 + b.to(F32), ab + b.to(F64).abs()
        if residual is not None:
            r = residual.to(self.dev)
            v64, v32, ab = v64 + r.to(F64), v32 + r.to(F32), ab + r.to(F64).abs()
        return v64, v32, ab

    def proj(self, link, got, R, S, bias=None, residual=None):
        v = self.prod(R, S, bias, residual)
        self.hold(link, lambda: _lora_bf16(got, v[0], v[1], v[2], link))

    def tn(self, dy, x):
        """(v64, v32, sum |term|) of dy^T x over the token axis: dy [K, M], x [K, N]"""
        return self.prod(dy.t(), x.t())

    def grads(self, names, taped, r, crit=None):
        """the published .grad of the parameters `names` (the REFERENCE's order) against their rows of the reduction r = (r64, r32, sum
        |term|) -- or by crit(grad, rows, name) --, and the launch's own output bit-equal to the published gradients laid end to end (the
        gradient station)"""
        off, pub = 0, []
        for n in names:
            g = self.st.grads.get(n)
            if g is None:
                raise TapeError(f"grad {n}: no gradient was published (a station is missing)")
            rows = g.shape[0]
            sl = slice(off, off + rows)
            off += rows
            pub.append(g.reshape(-1))
            if n in self.gst:
                raise TapeError(f"grad {n}: a second gradient station")
            self.gst[n] = True
            self.hold(f"grad {n}", (lambda g=g, sl=sl, n=n: _sum_f32(g, r[0][sl], r[1][sl], r[2][sl], n)) if crit is None else (lambda g=g, sl=sl, n=n: crit(g, sl, n)))
        self.hold(f"buffer ({names[0]} ..)", lambda: _same(taped.reshape(-1), torch.cat(pub), "the launch's output vs the published gradients"))

    def colsum_ref(self, x):
        x64 = self.d64(x)
        return x64.sum(0), x64.sum(0), x64.abs().sum(0)

    # ---- LayerNorm
    def ln_fwd(self, pre, rec, y, res, gkey, bkey, eps, keep, p, post=False, M=None):
        """returns (out, z station or None): z None where the launch saved none and the reference cannot restate it bit for bit"""
        out, z, mean, rstd = rec.ret
        kpre, p_pre, kpost, p_post = (None, 0.0, keep, p) if post else (keep, p, None, 0.0)
        yc, rc = y.cpu(), None if res is None else res.cpu()
        y_rows = yc.shape[0]
        M = y_rows if M is None else M
        gamma, beta = self.m.sd[gkey], self.m.sd[bkey]
        if z is not None:
            if not p_pre:
                want = ref64.layernorm_z(yc, rc, None, 0.0, y_rows, M, dtype=F32).to(BF16)
                self.hold(pre + ".z", lambda: _same(z.cpu(), want, pre + " z_save = bf16(y + residual)"))
            else:
                ze, zf = ref64.layernorm_z(yc, rc, kpre, p_pre, y_rows, M), ref64.layernorm_z(yc, rc, kpre, p_pre, y_rows, M, dtype=F32)

                def zcheck():
                    ratio = ref64.assert_bf16_rows(z.cpu(), ze, zf, pre + " z_save", floor=0.0)
                    dropped = kpre == 0
                    want = rc if rc is not None else torch.zeros(M, yc.shape[1], dtype=BF16)
                    # (value equality: a residual of -0 -- a post-dropout zero of the embedding LayerNorm -- plus the dropped +0 is +0)
                    assert torch.equal(z.cpu().to(F64)[dropped], want.to(F64)[dropped]), pre + ": a dropped element's z is not the residual"
                    return ratio
                self.hold(pre + ".z", zcheck)
            zc = z.cpu()
        elif not p_pre:
            zc = ref64.layernorm_z(yc, rc, None, 0.0, y_rows, M, dtype=F32).to(BF16)
        else:
            return out, None                                                  # (held through the re-run: see the module docstring)
        r64 = ref64.layernorm_of_z(zc.to(F64), gamma, beta, eps, kpost, p_post)
        r32 = ref64.layernorm_of_z(zc.to(F64), gamma, beta, eps, kpost, p_post, dtype=F32)
        unmasked = ref64.rowmax(ref64.layernorm_of_z(zc.to(F64), gamma, beta, eps)[0]) / (1.0 - p_post) if p_post else None
        self.hold(pre + ".out", lambda: ref64.assert_bf16_rows(out.cpu(), r64[0], r32[0], pre + " out", scale=unmasked))
        self.hold(pre + ".mean", lambda: ref64.assert_f32_close(_col(mean), _col(r64[1]), _col(r32[1]), scale=zc.to(F64).abs().amax(-1), what=pre + " mean"))
        self.hold(pre + ".rstd", lambda: ref64.assert_f32_close(_col(rstd), _col(r64[2]), _col(r32[2]), what=pre + " rstd"))
        return out, zc

    def ln_bwd(self, pre, dout, z, gkey, eps, keep, p, names, post=False, need_dy=True, deferred=False):
        """names = (gamma, beta, bias or None): the parameters whose gradients the launch (or its finish()) writes.  Returns (dz, dy)."""
        rec = self.take("layernorm_bwd", pre)
        dz, dy = rec.ret[0], rec.ret[1]
        if deferred:
            sums = self.take("ln_finish", pre + " finish()").args
        else:
            sums = (rec.args[5], rec.args[6], rec.args[7] if len(rec.args) > 7 else rec.kwargs.get("dbias"))
        kpre, p_pre, kpost, p_post = (None, 0.0, keep, p) if post else (keep, p, None, 0.0)
        gamma = self.m.sd[gkey]
        dc, zc = dout.cpu(), z.cpu()
        r64 = ref64.layernorm_bwd(dc, zc, gamma, eps, kpre, p_pre, kpost, p_post)
        r32 = ref64.layernorm_bwd(dc, zc, gamma, eps, kpre, p_pre, kpost, p_post, dtype=F32)
        self.hold(pre + ".dz", lambda: ref64.assert_bf16_rows(dz.cpu(), r64[0], r32[0], pre + " dz"))
        if need_dy and p_pre:
            unmasked = ref64.rowmax(r64[0]) / (1.0 - p_pre)
            self.hold(pre + ".dy", lambda: ref64.assert_bf16_rows(dy.cpu(), r64[1], r32[1], pre + " dy", scale=unmasked))
        tg, tb = ref64.layernorm_bwd_terms(dc, zc, eps, kpost, p_post)
        self.grads([names[0]], sums[0], (r64[2], r32[2], tg))
        self.grads([names[1]], sums[1], (r64[3], r32[3], tb))
        if names[2] is not None:
            if sums[2] is None:
                raise TapeError(f"{pre}: the launch carries no dbias")
            own = dy.cpu().to(F64)
            self.grads([names[2]], sums[2], (own.sum(0), own.sum(0), own.abs().sum(0)))
        return dz, dy

    # ---- attention
    def attention(self, pre, q, k, v, mask, seed_site, o_got, dout=None, got=None):
        """q [B, Sq, nh, dh], k / v [B, Sk, nh, dh] stations; forward (dout None) or backward (got = dict of dq / dk / dv)"""
        m = self.m
        B, Sq, Sk = q.shape[0], q.shape[1], k.shape[1]
        keep = self.masks.attn(self.seed(*seed_site), self.p_a, B, m.nh, Sq, Sk, self.b0) if self.p_a > 0.0 else None
        q, k, v = q.cpu(), k.cpu(), v.cpu()
        mask = None if mask is None else mask[:B].cpu()
        scale = m.dh ** -0.5
        d = torch.zeros_like(q) if dout is None else dout.cpu().reshape(q.shape)
        A = ref64.attention_bounds(q, k, v, mask, False, scale, d, keep, self.p_a)
        if dout is None:
            o = ref64.attention_fwd(q, k, v, mask, False, scale, keep, self.p_a)[0]
            self.hold(pre + ".att", lambda: ref64.assert_attn_bound(o_got.cpu().reshape(o.shape), o, A["o"], pre + " att"))
            return
        ref = dict(zip(("dq", "dk", "dv"), ref64.attention_bwd(q, k, v, mask, False, scale, d, keep, self.p_a)))
        for n in ("dq", "dk", "dv"):
            self.hold(f"{pre}.{n}", lambda n=n: ref64.assert_attn_bound(got[n].cpu().reshape(ref[n].shape), ref[n], A[n], f"{pre} {n}"))
        return ref, A

    # ---- forward
    def shadow(self):
        r = self.recs[self.pos] if self.pos < len(self.recs) else None
        if r is not None and r.name == "cast_f32_to_bf16" and len(r.args) == 2 and r.args[1] is not None:
            self.pos += 1
            self.hold(f"prep.shadow#{self.pos - 1}", lambda: _same(r.ret.cpu(), r.args[0].cpu().to(BF16), "the bf16 shadow of the masters"))
            return True
        return False

    def cast16(self, link, src):
        r = self.take("cast_f32_to_bf16", link)
        self.hold(link, lambda: _same(r.ret.cpu(), ref64.cast_f32_to_bf16(src).reshape(r.ret.shape), link))
        return r.ret

    def forward(self):
        m, st = self.m, self.st
        enc, mask = self.inp["enc"], self.inp.get("mask")
        self.mask = None if mask is None else (mask != 0).to(torch.uint8)
        B, H = self.B, m.H
        qe = m.sd["query_embeddings"] if m.kind != "bert" else self.inp["query_embeds"].detach().cpu()
        self.Q, self.T = qe.shape[1], enc.shape[1]
        self.qe_rows = qe.shape[0] * qe.shape[1]
        self.had_shadow = self.shadow()
        qe16 = self.cast16("qe16", qe).view(-1, H) if qe.dtype == F32 else qe.reshape(-1, H)
        self.enc16 = (self.cast16("enc16", enc) if enc.dtype == F32 else enc).reshape(B * self.T, -1)
        M = B * self.Q
        keep = self.hkeep(EMB_LAYER, EMB_SITE, M, self.p_h)
        rec = self.take("layernorm_fwd", "emb")
        x, self.z0 = self.ln_fwd("emb", rec, qe16, None, m.pre + "embeddings.LayerNorm.weight", m.pre + "embeddings.LayerNorm.bias", m.eps, keep, self.p_h,
                                 post=True, M=M)
        self.kv = None
        cl = [i for i in range(m.L) if m.cross[i]]
        if cl:                                # the hoisted K | V of every cross layer, in the reference's order k | v per layer, layer by layer
            got = self.take("gemm", "kv_all").ret
            keys = [f"{m.lp(i)}crossattention.self.{n}." for i in cl for n in ("key", "value")]
            self.proj("kv_all", got, self.enc16, m.w16(*[k + "weight" for k in keys]), m.f32(*[k + "bias" for k in keys]))
            self.kv = {i: (got[:, 2 * j * H:(2 * j + 1) * H], got[:, (2 * j + 1) * H:(2 * j + 2) * H]) for j, i in enumerate(cl)}
        self.Ls = []
        for i in range(m.L):
            L = self.layer_fwd(i, x, B)
            self.Ls.append(L)
            x = L["x3"]
        self.hold("h (returned)", lambda: _same(st.out["h"].reshape(M, H), x, "the encoder's result is the last layer's output"))
        self.h = x
        if m.kind == "item":
            self.hf = self.item_heads_fwd(x[:self.Bg * self.Q], self.Bg, "hd")
            self.hold("item (returned)", lambda: _same(st.out["item"], self.hf["item"], "item_representation"))
            self.hold("rec (returned)", lambda: _same(st.out["rec"], self.hf["rec"], "reconstructed_fields"))
            if self.Bg < B:
                o = self.item_heads_fwd(x[self.Bg * self.Q:], B - self.Bg, "hd.others")
                self.hold("other_item (returned)", lambda: _same(st.out["other_item"], o["item"], "the others' item_representation"))
            r = self.take("cast_bf16_to_f32", "query_outputs")
            self.hold("query_outputs", lambda: _same(r.ret.reshape(-1, H), x[:self.Bg * self.Q].to(F32), "query_outputs = f32(h)"))
        elif m.kind == "user":
            self.hf = self.user_head_fwd(x)
            self.hold("flat (returned)", lambda: _same(st.out["flat"], self.hf["flat"], "the prediction"))
        else:
            r = self.take("cast_bf16_to_f32", "last_hidden_state")
            self.hold("last_hidden_state", lambda: _same(r.ret.reshape(-1, H), x.to(F32), "last_hidden_state = f32(h)"))

    def layer_fwd(self, i, x, B):
        """one layer on the leading B samples' rows x [B * Q, H]: its launches' outputs as stations"""
        m = self.m
        H, nh, dh, Q, T, eps = m.H, m.nh, m.dh, self.Q, self.T, m.eps
        M = B * Q
        lp = m.lp(i)
        a = lp + "attention."
        n = lambda s: f"L{i}.{s}"       # noqa: E731
        L = {"x": x}
        qkv = self.take("gemm", n("qkv")).ret
        self.proj(n("qkv"), qkv, x, m.w16(*[a + f"self.{k}.weight" for k in ("query", "key", "value")]),
                  m.f32(*[a + f"self.{k}.bias" for k in ("query", "key", "value")]))
        q5 = qkv.reshape(B, Q, 3, nh, dh)
        r = self.take("attn_fwd", n("s.att"))
        att, L["s.ctx"] = r.ret[0], r.ret[1].n
        self.attention(n("s"), q5[:, :, 0], q5[:, :, 1], q5[:, :, 2], None, (i, 1), att)
        y = self.take("gemm", n("s.y")).ret
        self.proj(n("s.y"), y, att.reshape(M, H), m.w16(a + "output.dense.weight"), m.f32(a + "output.dense.bias"))
        rec = self.take("layernorm_fwd", n("s"))
        x1, z1 = self.ln_fwd(n("s"), rec, y, x, a + "output.LayerNorm.weight", a + "output.LayerNorm.bias", eps, self.hkeep(i, 2, M, self.p_h), self.p_h)
        L.update(qkv=qkv, att=att, y=y, x1=x1, z1=z1)
        xc = x1
        if m.cross[i]:
            c = lp + "crossattention."
            qc = self.take("gemm", n("qc")).ret
            self.proj(n("qc"), qc, x1, m.w16(c + "self.query.weight"), m.f32(c + "self.query.bias"))
            k, v = (t[:B * T].reshape(B, T, nh, dh) for t in self.kv[i])
            r = self.take("attn_fwd", n("c.att"))
            att2, L["c.ctx"] = r.ret[0], r.ret[1].n
            self.attention(n("c"), qc.reshape(B, Q, nh, dh), k, v, self.mask, (i, 3), att2)
            y2 = self.take("gemm", n("c.y")).ret
            self.proj(n("c.y"), y2, att2.reshape(M, H), m.w16(c + "output.dense.weight"), m.f32(c + "output.dense.bias"))
            rec = self.take("layernorm_fwd", n("c"))
            x2, z2 = self.ln_fwd(n("c"), rec, y2, x1, c + "output.LayerNorm.weight", c + "output.LayerNorm.bias", eps, self.hkeep(i, 4, M, self.p_h), self.p_h)
            L.update(qc=qc, att2=att2, y2=y2, x2=x2, z2=z2)
            xc = x2
        f1, f2 = lp + "intermediate_query.dense.", lp + "output_query."
        r = self.take("gemm", n("u"))
        u, hbuf = r.ret, r.kwargs.get("gelu_out")
        if hbuf is None:
            raise TapeError(f"{n('u')}: the launch carries no gelu_out")
        self.proj(n("u"), u, xc, m.w16(f1 + "weight"), m.f32(f1 + "bias"))
        self.hold(n("gelu"), lambda: ref64.assert_gelu_close(hbuf.cpu(), u.cpu(), n("gelu")))
        y3 = self.take("gemm", n("f.y")).ret
        self.proj(n("f.y"), y3, hbuf, m.w16(f2 + "dense.weight"), m.f32(f2 + "dense.bias"))
        rec = self.take("layernorm_fwd", n("f"))
        x3, z3 = self.ln_fwd(n("f"), rec, y3, xc, f2 + "LayerNorm.weight", f2 + "LayerNorm.bias", eps, self.hkeep(i, 5, M, self.p_h), self.p_h)
        L.update(xc=xc, u=u, hbuf=hbuf, y3=y3, x3=x3, z3=z3)
        return L

    # ---- heads
    def item_heads_fwd(self, h, nb, pre):
        m = self.m
        H, Q, E = m.H, self.Q, m.E
        pooled = self.take("mean_pool_fwd", pre + ".pooled").ret[1]
        h3 = h.cpu().reshape(nb, Q, H)
        self.hold(pre + ".pooled", lambda: ref64.assert_bf16_rows(pooled.cpu(), h3.to(F64).mean(1), h3.to(F32).mean(1), pre + " pooled"))
        item = self.take("gemm", pre + ".item").ret
        v = self.prod(pooled, m.w16("item_representation_head.weight"), m.f32("item_representation_head.bias"))
        self.hold(pre + ".item", lambda: _sum_f32(item, v[0], v[1], v[2], pre + " item"))
        rec_q = self.take("gemm", pre + ".rec_q").ret
        self.proj(pre + ".rec_q", rec_q, h, m.w16("reconstruction_head.weight"), m.f32("reconstruction_head.bias"))
        rec = self.take("field_projection_fwd", pre + ".rec").ret
        Wf, bf = m.sd["field_projection.weight"], m.sd["field_projection.bias"]
        rq = rec_q.cpu().reshape(nb, Q, E)
        flat = lambda t: t.reshape(-1, E)     # noqa: E731
        self.hold(pre + ".rec", lambda: ref64.assert_f32_close(flat(rec.cpu()), flat(ref64.field_projection_fwd(rq, Wf, bf)),
                                                               flat(ref64.field_projection_fwd(rq, Wf, bf, dtype=F32)), what=pre + " rec"))
        return dict(h=h, pooled=pooled, item=item, rec_q=rec_q, rec=rec)

    def item_heads_bwd(self):
        m, hf = self.m, self.hf
        H, Q, E, nb = m.H, self.Q, m.E, self.Bg
        h = hf["h"]
        d_item, d_rec = self.d_out["item"], self.d_out["rec"]
        r = self.take("field_projection_bwd", "hd.drq")
        drq = r.ret.reshape(nb * Q, E)
        Wf = m.sd["field_projection.weight"]
        rq = hf["rec_q"].cpu().reshape(nb, Q, E)
        r64, r32 = ref64.field_projection_bwd(d_rec.cpu(), rq, Wf), ref64.field_projection_bwd(d_rec.cpu(), rq, Wf, dtype=F32)
        self.hold("hd.drq", lambda: ref64.assert_bf16_rows(drq.cpu(), r64[0].reshape(-1, E), r32[0].reshape(-1, E), "hd drq"))
        fast = Q == 32 and Wf.shape[0] <= 16 and E % 128 == 0            # the MFMA kernel's shapes (tests/test_gpu_dw_f64.py)
        self.grads(["field_projection.weight"], r.args[3], (r64[1], r32[1], ref64.fproj_fast_dwf_terms(r64[3]) if fast else r64[3]))
        self.grads(["field_projection.bias"], r.args[4], (r64[2], r32[2], r64[4]))
        self.grads(["reconstruction_head.weight"], self.take("gemm", "grad reconstruction_head.weight").kwargs["out"], self.tn(drq, h))
        self.grads(["reconstruction_head.bias"], self.take("colsum", "grad reconstruction_head.bias").kwargs["out"], self.colsum_ref(drq))
        dh = self.take("gemm", "hd.dh_rec").ret
        self.proj("hd.dh_rec", dh, drq, m.w16("reconstruction_head.weight").t())
        d16 = self.cast16("hd.d16", d_item)
        self.grads(["item_representation_head.weight"], self.take("gemm", "grad item_representation_head.weight").kwargs["out"], self.tn(d16, hf["pooled"]))
        self.grads(["item_representation_head.bias"], self.take("colsum", "grad item_representation_head.bias").kwargs["out"], self.colsum_ref(d16))
        dpool = self.take("gemm", "hd.dpool").ret
        self.proj("hd.dpool", dpool, d16, m.w16("item_representation_head.weight").t())
        dh2 = self.take("mean_pool_bwd", "hd.dh_pool").ret.reshape(nb * Q, H)
        self.pool_bwd("hd.dh_pool", dh2, dpool, nb)
        both = self.take("add_bf16", "hd.dh").ret
        self.hold("hd.dh", lambda: _same(both.cpu().reshape(-1, H), ref64.add_bf16(dh, dh2)[0], "hd dh = dh_rec + dh_pool"))
        dq16 = self.cast16("dq16", self.d_out["query_outputs"]).reshape(-1, H)
        return dq16 + both.reshape(-1, H).to(dq16.device)

    def pool_bwd(self, link, got, dpool, nb):
        ref = (dpool.cpu().to(F64) / self.Q)[:, None, :].expand(nb, self.Q, self.m.H).reshape(nb * self.Q, -1)
        self.hold(link, lambda: ref64.assert_within_ulps(got.cpu(), ref, 1, 2.0 ** -18 * ref64.rowmax(ref), link))

    def user_head_fwd(self, h):
        m = self.m
        H, Q, B = m.H, self.Q, self.B
        u16 = self.take("mean_pool_fwd", "uh.u16").ret[1]
        h3 = h.cpu().reshape(B, Q, H)
        self.hold("uh.u16", lambda: ref64.assert_bf16_rows(u16.cpu(), h3.to(F64).mean(1), h3.to(F32).mean(1), "uh u16"))
        r = self.take("gemm", "uh.a")
        a, g = r.ret, r.kwargs.get("gelu_out")
        if g is None:
            raise TapeError("uh.a: the launch carries no gelu_out")
        self.proj("uh.a", a, u16, m.w16("prediction_head.0.weight"), m.f32("prediction_head.0.bias"))
        self.hold("uh.gelu", lambda: ref64.assert_gelu_close(g.cpu(), a.cpu(), "uh gelu"))
        rec = self.take("layernorm_fwd", "uh.ln")
        ln, _ = self.ln_fwd("uh.ln", rec, g, None, "prediction_head.2.weight", "prediction_head.2.bias", m.head_eps, None, 0.0)
        flat = self.take("gemm", "uh.flat").ret
        v = self.prod(ln, m.w16("prediction_head.3.weight"), m.f32("prediction_head.3.bias"))
        self.hold("uh.flat", lambda: _sum_f32(flat, v[0], v[1], v[2], "uh flat"))
        return dict(u16=u16, a=a, g=g, ln=ln, flat=flat)

    def user_head_bwd(self):
        m, hf = self.m, self.hf
        W3 = m.w16("prediction_head.3.weight")
        d16 = self.cast16("uh.d16", self.d_out)
        self.grads(["prediction_head.3.weight"], self.take("gemm", "grad prediction_head.3.weight").kwargs["out"], self.tn(d16, hf["ln"]))
        self.grads(["prediction_head.3.bias"], self.take("colsum", "grad prediction_head.3.bias").kwargs["out"], self.colsum_ref(d16))
        r = self.take("gemm", "uh.dln")
        if W3.shape[0] // 2048 > 1:                                        # the split-K f32 dX and its cast
            v = self.prod(d16, W3.t())
            self.hold("uh.dln32", lambda: _sum_f32(r.ret, v[0], v[1], v[2], "uh dln (f32, split-K)"))
            dln = self.cast16("uh.dln", r.ret)
        else:
            dln = r.ret
            self.proj("uh.dln", dln, d16, W3.t())
        dz, _ = self.ln_bwd("uh.ln", dln, hf["g"], "prediction_head.2.weight", m.head_eps, None, 0.0, ("prediction_head.2.weight", "prediction_head.2.bias", None),
                            need_dy=False)
        da = self.take("gelu_bwd", "uh.da").ret
        ref = dz.cpu().to(F64) * ref64.gelu_grad(hf["a"].cpu())
        self.hold("uh.da", lambda: ref64.assert_within_ulps(da.cpu(), ref, 1, 2.0 ** -18 * dz.cpu().to(F64).abs(), "uh da"))
        self.grads(["prediction_head.0.weight"], self.take("gemm", "grad prediction_head.0.weight").kwargs["out"], self.tn(da, hf["u16"]))
        self.grads(["prediction_head.0.bias"], self.take("colsum", "grad prediction_head.0.bias").kwargs["out"], self.colsum_ref(da))
        du = self.take("gemm", "uh.du").ret
        self.proj("uh.du", du, da, m.w16("prediction_head.0.weight").t())
        dh = self.take("mean_pool_bwd", "uh.dh").ret.reshape(self.B * self.Q, m.H)
        self.pool_bwd("uh.dh", dh, du, self.B)
        return dh

    # ---- backward
    def dW(self, names, dy, x):
        """the gradient of one weight (or several adjacent ones, in the reference's order): alone, or with the layer's grouped launch"""
        if self.st.grouped and dy.shape[0] == self.Mg and dy.shape[1] % 8 == 0 and x.shape[1] % 8 == 0:
            self.pending.append((names, dy, x))
            return
        self.grads(names, self.take("gemm", f"grad {names[0]}").kwargs["out"], self.tn(dy, x))

    def flush(self, why):
        if not self.pending:
            return
        prods = self.take("gemm_grouped", f"{why}: the grouped weight gradients").args[0]
        if len(prods) != len(self.pending):
            raise TapeError(f"{why}: the grouped launch carries {len(prods)} products where {len(self.pending)} weight gradients are due")
        for (names, dy, x), prod in zip(self.pending, prods):
            self.grads(names, prod[2], self.tn(dy, x))
        self.pending = []

    def dX(self, link, dy, keys, residual=None):
        got = self.take("gemm", link).ret
        self.proj(link, got, dy, self.m.w16(*keys).t(), None, residual)
        return got

    def backward(self):
        m, st = self.m, self.st
        H, nh, dh, Q, T, eps, Bg = m.H, m.nh, m.dh, self.Q, self.T, m.eps, self.Bg
        Mg = self.Mg = Bg * Q
        self.pending = []
        if m.kind == "item":
            dx = self.item_heads_bwd()
        elif m.kind == "user":
            dx = self.user_head_bwd()
        else:
            dx = self.cast16("dout16", self.d_out).reshape(Mg, H)
        with_enc = bool(self.inp.get("enc_needs_grad"))
        cl = [i for i in range(m.L) if m.cross[i]]
        if st.wt:                                  # W^T of every weight a dX reads, in the reference's order
            r = self.take("batched_transpose", "the weight transposes")
            want = []
            for i in range(m.L):
                lp = m.lp(i)
                a = lp + "attention."
                want += [[a + f"self.{k}.weight" for k in ("query", "key", "value")], [a + "output.dense.weight"], [lp + "intermediate_query.dense.weight"],
                         [lp + "output_query.dense.weight"]]
                if m.cross[i]:
                    want += [[lp + "crossattention.self.query.weight"], [lp + "crossattention.output.dense.weight"]]
                if i == 0 and with_enc and cl:
                    want += [[f"{m.lp(j)}crossattention.self.{k}.weight" for j in cl for k in ("key", "value")]]
            if len(r.ret) != len(want):
                raise TapeError(f"the transposes: {len(r.ret)} outputs where the reference lists {len(want)}")
            self.hold("prep.transposes", lambda: max(_same(o.cpu(), m.w16(*k).t().cpu(), f"W^T of {k[0]}") for o, k in zip(r.ret, want)))
        mask = self.mask
        dkv = {}
        fused_cs = None
        for i in reversed(range(m.L)):
            L = self.Ls[i]
            if self.ckpt:
                first = L
                self.tag = " (re-run)"
                L = self.layer_fwd(i, first["x"][:Mg], Bg)
                self.tag = ""
                keys = [k for k in L if not k.endswith("ctx") and not k.startswith("z") and L[k] is not None]
                self.hold(f"L{i}.rerun", lambda: max(_same(L[k], first[k][:L[k].shape[0]], f"L{i} re-run {k}") for k in keys))
            elif Bg < self.B:
                L = {k: (v if k.endswith("ctx") or v is None else v[:(Bg if v.dim() == 4 else Mg)]) for k, v in L.items()}
            lp = m.lp(i)
            n = lambda s: f"L{i}.{s}"       # noqa: E731
            f1, f2 = lp + "intermediate_query.dense.", lp + "output_query."
            dz3, dy3 = self.ln_bwd(n("f"), dx, L["z3"], f2 + "LayerNorm.weight", eps, self.hkeep(i, 5, Mg, self.p_h), self.p_h,
                                   (f2 + "LayerNorm.weight", f2 + "LayerNorm.bias", f2 + "dense.bias"), deferred=st.side)
            self.dW([f2 + "dense.weight"], dy3, L["hbuf"])
            du = self.take("gemm", n("du")).ret
            pre64, pre32, ab = self.prod(dy3, m.w16(f2 + "dense.weight").t())
            gp = ref64.gelu_grad(L["u"].cpu()).to(self.dev)
            fl = 2.0 ** -18 * pre64.abs() + (2.0 ** -20 * ab + 8.0 * (pre32.to(F64) - pre64).abs()) * gp.abs()
            self.hold(n("du"), lambda: ref64.assert_ulp_ratio(du.to(self.dev), pre64 * gp, 1, fl, n("du")))
            self.grads([f1 + "bias"], self.take("colsum", f"grad {f1}bias").kwargs["out"], self.colsum_ref(du))
            self.dW([f1 + "weight"], du, L["xc"])
            dx = self.dX(n("dxc"), du, [f1 + "weight"], residual=dz3)
            if m.cross[i]:
                c = lp + "crossattention."
                dz2, dy2 = self.ln_bwd(n("c"), dx, L["z2"], c + "output.LayerNorm.weight", eps, self.hkeep(i, 4, Mg, self.p_h), self.p_h,
                                       (c + "output.LayerNorm.weight", c + "output.LayerNorm.bias", c + "output.dense.bias"), deferred=st.side)
                self.dW([c + "output.dense.weight"], dy2, L["att2"].reshape(Mg, H))
                dctx2 = self.dX(n("c.dctx"), dy2, [c + "output.dense.weight"])
                r = self.take("attn_bwd", n("c.dq"))
                if not isinstance(r.args[0], LL._Ctx) or r.args[0].n != L["c.ctx"]:
                    raise TapeError(f"L{i}: the cross-attention backward runs on another launch's context")
                k, v = (t[:Bg * T].reshape(Bg, T, nh, dh) for t in self.kv[i])
                got = {"dq": r.kwargs["dq"], "dk": r.kwargs["dk"], "dv": r.kwargs["dv"]}
                ref, A = self.attention(n("c"), L["qc"].reshape(Bg, Q, nh, dh), k, v, mask, (i, 3), None, dctx2, got)
                dkv[i] = (got["dk"].reshape(Bg * T, H), got["dv"].reshape(Bg * T, H))
                cs = r.kwargs.get("kv_colsum")
                if fused_cs is None:
                    fused_cs = cs is not None
                if fused_cs != (cs is not None):
                    raise TapeError(f"L{i}: kv_colsum is written by some cross layers' attention backward and not by others")
                if cs is not None:           # the few-query kernel sums its float32 dK | dV BEFORE the bf16 store: the float64 column sums of
                    # the float64 dK / dV within the summed A, as test_few_query_dkv_and_kv_colsum holds it (test_qformer_links_host shows
                    # that the sums of the STORED values are another quantity)
                    want, bound = (torch.cat([t[k_].sum(dim=(0, 1)).reshape(-1) for k_ in ("dk", "dv")]) for t in (ref, A))
                    self.grads([c + "self.key.bias", c + "self.value.bias"], cs, None,
                               crit=lambda g, sl, name: ref64.assert_attn_bound(g.cpu(), want[sl], bound[sl], name))
                dqc = got["dq"].reshape(Mg, H)
                self.dW([c + "self.query.weight"], dqc, L["x1"])
                self.grads([c + "self.query.bias"], self.take("colsum", f"grad {c}self.query.bias").kwargs["out"], self.colsum_ref(dqc))
                dx = self.dX(n("dx1"), dqc, [c + "self.query.weight"], residual=dz2)
            a = lp + "attention."
            dz1, dy1 = self.ln_bwd(n("s"), dx, L["z1"], a + "output.LayerNorm.weight", eps, self.hkeep(i, 2, Mg, self.p_h), self.p_h,
                                   (a + "output.LayerNorm.weight", a + "output.LayerNorm.bias", a + "output.dense.bias"), deferred=st.side)
            self.dW([a + "output.dense.weight"], dy1, L["att"].reshape(Mg, H))
            dctx = self.dX(n("s.dctx"), dy1, [a + "output.dense.weight"])
            r = self.take("attn_bwd", n("s.dq"))
            if not isinstance(r.args[0], LL._Ctx) or r.args[0].n != L["s.ctx"]:
                raise TapeError(f"L{i}: the self-attention backward runs on another launch's context")
            q5 = L["qkv"].reshape(Bg, Q, 3, nh, dh)
            got = {"dq": r.kwargs["dq"], "dk": r.kwargs["dk"], "dv": r.kwargs["dv"]}
            self.attention(n("s"), q5[:, :, 0], q5[:, :, 1], q5[:, :, 2], None, (i, 1), None, dctx, got)
            dqkv = torch.cat([got[k].reshape(Mg, H) for k in ("dq", "dk", "dv")], 1)              # the reference's order: q | k | v
            qkvw = [a + f"self.{k}.weight" for k in ("query", "key", "value")]
            self.dW(qkvw, dqkv, L["x"])
            self.grads([a + f"self.{k}.bias" for k in ("query", "key", "value")], self.take("colsum", f"grad {a}self.*.bias").kwargs["out"], self.colsum_ref(dqkv))
            dx = self.dX(n("dx0"), dqkv, qkvw, residual=dz1)
            self.flush(f"L{i}")
        if cl:
            kvw = [f"{m.lp(j)}crossattention.self.{k}.weight" for j in cl for k in ("key", "value")]
            kvb = [f"{m.lp(j)}crossattention.self.{k}.bias" for j in cl for k in ("key", "value")]
            dkv_all = torch.cat([t for j in cl for t in dkv[j]], 1)                                # the reference's order again
            self.dW(kvw, dkv_all, self.enc16[:Bg * T])
            if not fused_cs:
                self.grads(kvb, self.take("colsum", "grad of the K | V biases").kwargs["out"], self.colsum_ref(dkv_all))
            if with_enc:
                d_enc16 = self.dX("d_enc16", dkv_all, kvw)
        z0 = self.z0[:Mg]
        dz0, _ = self.ln_bwd("emb", dx, z0, m.pre + "embeddings.LayerNorm.weight", eps, self.hkeep(EMB_LAYER, EMB_SITE, Mg, self.p_h), self.p_h,
                             (m.pre + "embeddings.LayerNorm.weight", m.pre + "embeddings.LayerNorm.bias", None), post=True, need_dy=False)
        rows = self.qe_rows
        if m.kind != "bert":
            r = self.take("batch_reduce", "grad query_embeddings")
            ref = ref64.batch_reduce(dz0.cpu(), Mg // rows, rows, H), ref64.batch_reduce(dz0.cpu().to(F64).abs(), Mg // rows, rows, H)
            self.grads(["query_embeddings"], r.kwargs["out"], (ref[0].reshape(1, rows, H), ref[0].reshape(1, rows, H), ref[1].reshape(1, rows, H)))
        elif rows == Mg:
            r = self.take("cast_bf16_to_f32", "d_qe")
            self.hold("d_qe", lambda: _same(r.ret.reshape(Mg, H), dz0.to(F32), "d_qe = f32(dz0)"))
            self.hold("d_qe (returned)", lambda: _same(st.d_qe.reshape(Mg, H), r.ret.reshape(Mg, H), "the step's d_qe"))
        else:
            r = self.take("batch_reduce", "d_qe")
            ref = ref64.batch_reduce(dz0.cpu(), Mg // rows, rows, H), ref64.batch_reduce(dz0.cpu().to(F64).abs(), Mg // rows, rows, H)
            self.hold("d_qe", lambda: ref64.assert_colsum_close(r.ret.cpu().reshape(rows, H), ref[0], ref[0], ref[1], "d_qe"))
            self.hold("d_qe (returned)", lambda: _same(st.d_qe.reshape(rows, H), r.ret.reshape(rows, H), "the step's d_qe"))
        if cl and with_enc:
            r = self.take("cast_bf16_to_f32", "d_enc")
            self.hold("d_enc", lambda: _same(r.ret.reshape(d_enc16.shape), d_enc16.to(F32), "d_enc = f32(d_enc16)"))
            self.hold("d_enc (returned)", lambda: _same(st.d_enc.reshape(d_enc16.shape), r.ret.reshape(d_enc16.shape), "the step's d_enc"))
        self.flush("after the loop")
        # ---- every live parameter's published gradient is one gradient station; the dead ones have none
        live = set(m.live)
        if set(self.gst) != live:
            raise TapeError(f"gradient stations != live parameters: missing {sorted(live - set(self.gst))[:4]}, unexpected {sorted(set(self.gst) - live)[:4]}")
        stray = [n for n in m.names if n not in live and st.grads.get(n) is not None]
        if stray:
            raise TapeError(f"dead parameters carry a gradient: {stray[:4]}")


def expected_stations(step, mdef, inputs):
    """the stations the configuration promises (prep.*, buffers and the (returned) identities aside), written from the configuration alone"""
    I, m = step.info, mdef
    p, ckpt, bwd, train_z = I["p_h"] > 0.0, I["ckpt"], step.backward, step.keep and not I["ckpt"]
    f32_in = lambda t: t.dtype == F32       # noqa: E731
    out = []
    if m.kind != "bert" or f32_in(inputs["query_embeds"]):
        out.append("qe16")
    if f32_in(inputs["enc"]):
        out.append("enc16")

    def ln(pre, z, full=True):
        return ([pre + ".z"] if z else []) + ([pre + ".out", pre + ".mean", pre + ".rstd"] if full else [])

    def layer(i, tag, z):
        full = z or not p
        o = [f"L{i}.qkv", f"L{i}.s.att", f"L{i}.s.y", f"L{i}.u", f"L{i}.gelu", f"L{i}.f.y"] + ln(f"L{i}.s", z, full) + ln(f"L{i}.f", z, full)
        if m.cross[i]:
            o += [f"L{i}.qc", f"L{i}.c.att", f"L{i}.c.y"] + ln(f"L{i}.c", z, full)
        return [s + tag for s in o]
    out += ln("emb", step.keep)
    if any(m.cross):
        out.append("kv_all")
    for i in range(m.L):
        out += layer(i, "", train_z)
    if m.kind == "item":
        out += ["hd.pooled", "hd.item", "hd.rec_q", "hd.rec", "query_outputs"]
        if I["Bg"] < I["B"]:
            out += ["hd.others.pooled", "hd.others.item", "hd.others.rec_q", "hd.others.rec"]
    elif m.kind == "user":
        out += ["uh.u16", "uh.a", "uh.gelu", "uh.ln.out", "uh.ln.mean", "uh.ln.rstd", "uh.flat"]
    else:
        out.append("last_hidden_state")
    if not bwd:
        return set(out)
    out += [f"grad {n}" for n in m.live]
    if m.kind == "item":
        out += ["hd.drq", "hd.dh_rec", "hd.d16", "hd.dpool", "hd.dh_pool", "hd.dh", "dq16"]
    elif m.kind == "user":
        out += ["uh.d16", "uh.dln", "uh.ln.dz", "uh.da", "uh.du", "uh.dh"] + (["uh.dln32"] if m.sd["prediction_head.3.weight"].shape[0] // 2048 > 1 else [])
    else:
        out += ["dout16", "d_qe"] + (["d_enc16", "d_enc"] if inputs.get("enc_needs_grad") and any(m.cross) else [])
    dy = [".dz"] + ([".dy"] if p else [])
    for i in range(m.L):
        if ckpt:
            out += layer(i, " (re-run)", True) + [f"L{i}.rerun"]
        out += [f"L{i}.f{s}" for s in dy] + [f"L{i}.du", f"L{i}.dxc"] + [f"L{i}.s{s}" for s in dy] + [f"L{i}.s.dctx", f"L{i}.s.dq", f"L{i}.s.dk", f"L{i}.s.dv", f"L{i}.dx0"]
        if m.cross[i]:
            out += [f"L{i}.c{s}" for s in dy] + [f"L{i}.c.dctx", f"L{i}.c.dq", f"L{i}.c.dk", f"L{i}.c.dv", f"L{i}.dx1"]
    out.append("emb.dz")
    return set(out)


def _aux(name):
    return name.startswith("prep.") or name.endswith("(returned)") or name.startswith("buffer (")


def check_step(step, mdef, inputs, masks, d_out=None, verbose=True):
    """Hold every station of a taped step.  inputs / d_out: what run_step was given; masks: .hidden(seed, p, rows, H, row0) -> uint8 [rows, H],
    .attn(seed, p, B, nh, Sq, Sk, b0) -> uint8 [B, nh, Sq, Sk] (CPU tensors).  Returns {station: worst error / bound}; raises TapeError (the
    shape of the tape) or LinkFailures (.failed in tape order)."""
    w = _Walk(step, mdef, inputs, masks, d_out)
    w.forward()
    if step.backward:
        w.backward()
    if w.pos != len(w.recs):
        raise TapeError(f"launch {w.pos} of {len(w.recs)} (hip.{w.recs[w.pos].name}) is consumed by no link")
    got, want = {k for k in w.checked if not _aux(k)}, expected_stations(step, mdef, inputs)
    if got != want or len(got) != len([k for k in w.checked if not _aux(k)]):
        raise TapeError(f"stations checked != stations the configuration promises: missing {sorted(want - got)[:6]}, unexpected {sorted(got - want)[:6]}")
    if verbose:
        for k in w.checked:
            print(f"[ratio] {k}: {w.ratios.get(k, float('nan')):.4f}" + ("   <-- FAILED" if k in w.failed else ""))
    if w.failed:
        raise LinkFailures(w.failed, w.ratios)
    return w.ratios

"""Float64 restatements of the head, RoPE, pool, data, attention, norm, reduction, GEMM-epilogue, LoRA, optimizer, cast, field-projection
and split-K primitives of include/unirec_hip.h, and the element-wise criteria the GPU tests hold the kernels to (tests/test_gpu_head_primitives.py,
tests/test_gpu_attention_f64.py, tests/test_gpu_norm_f64.py, tests/test_gpu_lora_f64.py, tests/test_gpu_gemm_f64.py,
tests/test_gpu_elementwise_f64.py, tests/test_gpu_dw_f64.py).  Plain torch: no fixtures, no device code
(the fused-GEMM-epilogue section at the end runs on its inputs' device, everything else on the CPU).

Every reference is written from the formula in the header comment of its entry point and is itself checked against an
independent implementation in tests/test_ref64.py.  All functions take / return CPU tensors; inputs of any float dtype are
promoted to float64 first (``dtype=torch.float32`` re-evaluates the SAME formula in float32: the yardstick of assert_f32_close).
"""
import math

import torch

F64 = torch.float64
BF16_MAX = float(torch.finfo(torch.bfloat16).max)
_BF16_MIN_NORMAL_EXP = -126


# ---- criteria --------------------------------------------------------------------------------------------------------------
def bf16_ulp(ref64):
    """2 ** (floor(log2 |ref|) - 7): the spacing of bfloat16 (8 significant bits) at |ref|, floored at the smallest normal."""
    a = torch.as_tensor(ref64, dtype=F64).abs()
    _, e = torch.frexp(a)                                        # a = m * 2^e, m in [0.5, 1): floor(log2 a) = e - 1
    e = torch.where(a == 0, torch.full_like(e, _BF16_MIN_NORMAL_EXP), e - 1).clamp_min(_BF16_MIN_NORMAL_EXP)
    return torch.ldexp(torch.ones_like(a), e - 7)


def f32_ulp(x):
    """Spacing of float32 at |x| (floored at the smallest normal)."""
    a = torch.as_tensor(x, dtype=F64).abs()
    _, e = torch.frexp(a)
    e = torch.where(a == 0, torch.full_like(e, -126), e - 1).clamp_min(-126)
    return torch.ldexp(torch.ones_like(a), e - 23)


def _cpu64(t):
    return torch.as_tensor(t).detach().to("cpu").to(F64)


def assert_within_ulps(got, ref64, ulps, floor=0.0, what=""):
    """EVERY element: |got - ref| <= ulps * bf16_ulp(ref) + floor (floor broadcasts against ref: a per-row scale), everything finite.
    Returns the worst |err| / bound (for the lab-note table)."""
    g, r = _cpu64(got), _cpu64(ref64)
    assert g.shape == r.shape, f"{what}: shape {tuple(g.shape)} vs reference {tuple(r.shape)}"
    assert torch.isfinite(r).all(), f"{what}: the reference itself is not finite"
    if g.numel() == 0:
        return 0.0
    bad = ~torch.isfinite(g)
    if bad.any():
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} non-finite outputs, first at {i}: got {g[i].item()}, reference {r[i].item()}")
    fl = torch.as_tensor(floor, dtype=F64)
    ulp = bf16_ulp(r)
    err = (g - r).abs()
    bound = (ulps * ulp + fl).expand_as(err)
    off = err > bound
    if off.any():
        ratio = torch.where(off, err / ulp, torch.zeros_like(err))
        flat = int(ratio.argmax())
        i = tuple(int(v) for v in torch.unravel_index(torch.tensor(flat), err.shape))
        raise AssertionError(f"{what}: {int(off.sum())} of {err.numel()} elements exceed {ulps} bf16 ulp + floor; worst at index {i}: "
                             f"got {g[i].item()!r}, reference {r[i].item()!r}, error {err[i].item():.3e} = {ratio[i].item():.2f} ulp "
                             f"(allowed {bound[i].item():.3e})")
    return float((err / bound.clamp_min(1e-300)).max())


def assert_f32_close(got, ref64, ref32, scale=None, what=""):
    """f32 outputs.  ref32 is the SAME reference formula evaluated in float32 torch on the CPU; e32 = per-row max |ref32 - ref64|
    is what plain f32 arithmetic costs on this input.  Per row (last axis; a 0-d / 1-element tensor is one row):
        max |got - ref64| <= 8 * e32 + 2 ** -20 * scale,      scale = row max |ref64| unless given (|loss| + 1 for scalars).
    Returns the worst row's error / bound."""
    g, r, r32 = _cpu64(got), _cpu64(ref64), _cpu64(ref32)
    assert g.shape == r.shape == r32.shape, f"{what}: shapes {tuple(g.shape)} / {tuple(r.shape)} / {tuple(r32.shape)}"
    assert torch.isfinite(r).all(), f"{what}: the reference itself is not finite"
    if g.numel() == 0:
        return 0.0
    bad = ~torch.isfinite(g)
    if bad.any():
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} non-finite outputs, first at {i}: got {g[i].item()}, reference {r[i].item()}")
    if g.dim() == 0:
        g, r, r32 = g.reshape(1), r.reshape(1), r32.reshape(1)
    e32 = (r32 - r).abs().amax(dim=-1)
    sc = r.abs().amax(dim=-1) if scale is None else torch.as_tensor(scale, dtype=F64).expand_as(e32)
    bound = 8.0 * e32 + 2.0 ** -20 * sc
    err = (g - r).abs()
    rowerr = err.amax(dim=-1)
    off = rowerr > bound
    if off.any():
        excess = torch.where(off, rowerr - bound, torch.zeros_like(rowerr))
        row = tuple(int(v) for v in torch.unravel_index(excess.argmax(), rowerr.shape))
        col = int(err[row].argmax())
        i = row + (col,)
        raise AssertionError(f"{what}: {int(off.sum())} of {rowerr.numel()} rows exceed 8 * e32 + 2^-20 * scale; worst at index {i}: "
                             f"got {g[i].item()!r}, reference {r[i].item()!r}, error {err[i].item():.3e}, allowed {bound[row].item():.3e} "
                             f"(e32 {e32[row].item():.3e}, scale {sc[row].item():.3e})")
    ok = bound > 0
    return float((rowerr[ok] / bound[ok]).max()) if ok.any() else 0.0


def rowmax(ref64, dim=-1):
    return _cpu64(ref64).abs().amax(dim=dim, keepdim=True)


# ---- Qwen3 q/k RMSNorm + RoPE (modeling_qwen3.py:59-64, 107-170) -----------------------------------------------------------
def rope_table(S, head_dim, theta, dtype=F64):
    """cos / sin [S, head_dim / 2]: inv_freq_i = theta ** (-2 i / head_dim), angle = pos * inv_freq_i."""
    i = torch.arange(head_dim // 2, dtype=dtype)
    inv = torch.as_tensor(theta, dtype=dtype) ** (-(2.0 * i) / head_dim)
    ang = torch.arange(S, dtype=dtype)[:, None] * inv[None, :]
    return torch.cos(ang), torch.sin(ang)


def _rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat([-x[..., h:], x[..., :h]], dim=-1)


def _unrotate(y, c, s):
    """R^T y of the rotation R x = x c + rotate_half(x) s (c, s duplicated over both halves)."""
    return y * c - _rotate_half(y) * s


def _cs_rows(cos_tab, sin_tab, M, S, dtype):
    pos = torch.arange(M) % S
    c = cos_tab.to(dtype)[pos]
    s = sin_tab.to(dtype)[pos]
    return torch.cat([c, c], -1)[:, None, :], torch.cat([s, s], -1)[:, None, :]


def _head_weights(qw, kw, nq, nkv, dtype):
    return torch.cat([qw.to(dtype)[None].expand(nq, -1), kw.to(dtype)[None].expand(nkv, -1)], 0)      # [nq + nkv, hd]


def qknorm_rope_fwd(raw, qw, kw, cos_tab, sin_tab, S, nq, nkv, hd, eps, dtype=F64):
    """raw [M, >= (nq + nkv) * hd] (q heads | k heads | ...), token m at position m % S, the TABLES AS GIVEN (the kernel's f32 ones, so
    table error is not rope error): out[m, h] = RoPE(w_h * x / sqrt(mean(x^2) + eps)).  Returns [M, nq + nkv, hd]."""
    M = raw.shape[0]
    x = raw[:, :(nq + nkv) * hd].to(dtype).reshape(M, nq + nkv, hd)
    w = _head_weights(qw, kw, nq, nkv, dtype)
    xn = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * w
    c, s = _cs_rows(cos_tab, sin_tab, M, S, dtype)
    return xn * c + _rotate_half(xn) * s


def qknorm_rope_rstd(raw, nq, nkv, hd, eps):
    M = raw.shape[0]
    x = raw[:, :(nq + nkv) * hd].to(F64).reshape(M, nq + nkv, hd)
    return torch.rsqrt((x * x).mean(-1) + eps)                    # [M, nq + nkv]


def qknorm_rope_bwd(dout, raw, qw, kw, cos_tab, sin_tab, S, nq, nkv, hd, eps):
    """Gradient of the raw projection: torch.autograd through the float64 forward.  dout [M, nq + nkv, hd]; returns the same shape."""
    x = raw[:, :(nq + nkv) * hd].to(F64).clone().requires_grad_(True)
    out = qknorm_rope_fwd(x, qw, kw, cos_tab, sin_tab, S, nq, nkv, hd, eps)
    (g,) = torch.autograd.grad(out, x, dout.to(F64))
    return g.reshape(out.shape)


def qknorm_rope_bwd_from_roped(dout, roped, rstd, qw, kw, cos_tab, sin_tab, S, nq, nkv, hd):
    """The same gradient written out, from what the fused forward keeps: the ROPED output o and 1 / rms.
        xn = R^T o,  x^ = xn / w,  g = (R^T dout) * w,  dx = rstd * (g - x^ * mean(g * x^)).
    dout, roped [M, nq + nkv, hd]; rstd [M, nq + nkv]."""
    M = dout.shape[0]
    w = _head_weights(qw, kw, nq, nkv, F64)
    c, s = _cs_rows(cos_tab, sin_tab, M, S, F64)
    xh = _unrotate(roped.to(F64), c, s) / w
    g = _unrotate(dout.to(F64), c, s) * w
    t = (g * xh).mean(-1, keepdim=True)
    return rstd.to(F64)[..., None] * (g - xh * t)


# ---- user-sequence assembly (models/user_sequence_encoder.py:16-33, 128-142) -----------------------------------------------
def sinusoidal_pe(length, H, dtype=F64):
    """PE over the FLAT index: even d -> sin(pos * w_d), odd d -> cos(pos * w_{d-1}), w_d = exp(-d * ln(1e4) / H)."""
    pos = torch.arange(length, dtype=dtype)[:, None]
    d = torch.arange(0, H, 2, dtype=dtype)
    w = torch.exp(d * (-math.log(10000.0) / H))
    pe = torch.zeros(length, H, dtype=dtype)
    pe[:, 0::2] = torch.sin(pos * w)
    pe[:, 1::2] = torch.cos(pos * w)
    return pe


def user_sequence_assemble(tokens, ctx, lengths, keep=None, p=0.0):
    """tokens [B, L, Qi, H], ctx [B, L, H], lengths [B]; keep [B, L*Qi, H] (0 / 1) or None.
    out[b, l*Qi + j] = (tokens + ctx + PE[l*Qi + j]) * keep / (1 - p) for l < len[b], else 0; mask = l < len[b]."""
    B, L, Qi, H = tokens.shape
    x = (tokens.to(F64) + ctx.to(F64)[:, :, None, :]).reshape(B, L * Qi, H) + sinusoidal_pe(L * Qi, H)[None]
    valid = (torch.arange(L)[None, :] < lengths.to(torch.int64)[:, None]).repeat_interleave(Qi, dim=1)       # [B, L*Qi]
    if keep is not None:
        x = x * keep.to(F64).reshape(B, L * Qi, H) / (1.0 - p)
    return x * valid[..., None].to(F64), valid.to(F64)


# ---- ranking head (train_item_individual_token_joint.py:331-352, 392-419) --------------------------------------------------
def _normalize(x, eps=1e-12):
    return x / x.norm(dim=-1, keepdim=True).clamp_min(eps)


def cosine_scores(user, pos, neg, dtype=F64):
    """scores [B, 1 + N]: column 0 = cos(user, pos), 1 + n = cos(user, neg_n); F.normalize eps 1e-12."""
    u = _normalize(user.to(dtype))
    cand = torch.cat([pos.to(dtype)[:, None, :], neg.to(dtype)], dim=1)
    return torch.einsum("bd,bnd->bn", u, _normalize(cand))


def catalog_scores(user, catalog, dtype=F64):
    return _normalize(user.to(dtype)) @ _normalize(catalog.to(dtype)).t()


def infonce(user, pos, neg, neg_mask, tau, grad_scale=1.0, dtype=F64):
    """loss = mean_b(-s_b0 / tau + logsumexp over {0} U valid negatives of s / tau); d_user = grad_scale * dloss / duser (autograd)."""
    u = user.to(dtype).clone().requires_grad_(True)
    z = cosine_scores(u, pos, neg, dtype) / tau
    if neg_mask is not None:
        valid = torch.cat([torch.ones(z.shape[0], 1, dtype=torch.bool), neg_mask.bool()], dim=1)
        z = z.masked_fill(~valid, float("-inf"))
    loss = (torch.logsumexp(z, dim=1) - z[:, 0]).mean()
    (du,) = torch.autograd.grad(loss, u)
    return loss.detach(), du * grad_scale


def mrr_rank(scores, neg_mask=None):
    """1 + #{valid n : s[1 + n] > s[0]} (the positive wins ties)."""
    gt = scores[:, 1:] > scores[:, :1]
    if neg_mask is not None:
        gt = gt & neg_mask.bool()
    return 1 + gt.sum(dim=1)


def rank_of_index(scores, gt_index):
    ref = scores.gather(1, gt_index.to(torch.int64)[:, None])
    return 1 + (scores > ref).sum(dim=1)


def topk(scores, K):
    """Descending top-K, lowest index first among equal scores: K rounds of 'first position of the maximum'."""
    s = scores.clone().to(F64)
    B, C = s.shape
    taken = torch.zeros(B, C, dtype=torch.bool)
    idx = torch.empty(B, K, dtype=torch.int64)
    rows = torch.arange(B)
    for k in range(K):
        # -inf scores must stay selectable: mask by `taken`, not by value
        cur = torch.where(taken, torch.full_like(s, float("-inf")), s)
        best = cur.amax(dim=1, keepdim=True)
        cand = (cur == best) & ~taken
        i = torch.where(cand, torch.arange(C)[None, :].expand(B, C), torch.full((B, C), C)).amin(dim=1)
        idx[:, k] = i
        taken[rows, i] = True
    return idx, scores.gather(1, idx)


# ---- Q-Former heads / losses (training/item_qformer_training.py:49-56, evaluation/evaluate_item_qformer.py:75-92) ----------
def recon_stats(rec, x, mask, dtype=F64):
    """sums3 = (sum mask * (rec - x)^2, sum mask, sum over valid rows of cos(x_row, rec_row)); rec, x [rows, E], mask [rows]."""
    rec, x, m = rec.to(dtype), x.to(dtype), mask.to(dtype)
    se = (((rec - x) ** 2).sum(-1) * m).sum()
    cos = (rec * x).sum(-1) / (x.norm(dim=-1).clamp_min(1e-12) * rec.norm(dim=-1).clamp_min(1e-12))
    return torch.stack([se, m.sum(), (cos * (m != 0).to(dtype)).sum()])


def recon_grad(rec, x, mask, coef, dtype=F64):
    """d_rec = coef * 2 * mask * (rec - x) / sum(mask)."""
    rec, x, m = rec.to(dtype), x.to(dtype), mask.to(dtype)
    return (2.0 * coef / m.sum()) * m[:, None] * (rec - x)


def triplet_margin(a, p, n, margin, coef, dtype=F64):
    """TripletMarginLoss(margin, p=2, eps=1e-6 ADDED TO THE DIFFERENCE, mean); returns (loss, coef * dloss / danchor)."""
    a = a.to(dtype).clone().requires_grad_(True)
    dp = ((a - p.to(dtype) + 1e-6) ** 2).sum(-1).sqrt()
    dn = ((a - n.to(dtype) + 1e-6) ** 2).sum(-1).sqrt()
    loss = (dp - dn + margin).clamp_min(0.0).mean()
    (da,) = torch.autograd.grad(loss, a)
    return loss.detach(), coef * da


def mse(a, b, coef, dtype=F64):
    """nn.MSELoss (mean over all elements); returns (loss, coef * 2 (a - b) / n)."""
    a, b = a.to(dtype), b.to(dtype)
    d = a - b
    return (d * d).mean(), (2.0 * coef / d.numel()) * d


# ---- element-wise --------------------------------------------------------------------------------------------------------
def gelu_grad(u):
    """d/du [u * Phi(u)] = Phi(u) + u * phi(u), Phi through erfc so the negative tail keeps its relative accuracy."""
    u = u.to(F64)
    cdf = 0.5 * torch.special.erfc(-u / math.sqrt(2.0))
    return cdf + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def gelu(u):
    u = u.to(F64)
    return u * 0.5 * torch.special.erfc(-u / math.sqrt(2.0))


def _sigmoid64(g):
    # 1 / (1 + exp(-g)) without overflow on either side
    e = torch.exp(-g.abs())
    return torch.where(g >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def swiglu_fwd(gate, up):
    g, u = gate.to(F64), up.to(F64)
    return g * _sigmoid64(g) * u


def swiglu_bwd(dact, gate, up):
    """(dgate, dup): dgate = dact * up * silu'(gate), silu'(g) = s (1 + g (1 - s)); dup = dact * silu(gate)."""
    d, g, u = dact.to(F64), gate.to(F64), up.to(F64)
    s = _sigmoid64(g)
    one_minus_s = _sigmoid64(-g)
    return d * u * s * (1.0 + g * one_minus_s), d * g * s


# ---- event-context encoders, first layer (models/mwne.py:525-565, 586-607) -------------------------------------------------
def timestamp_features(ts):
    """9 features, EVERY STEP IN FLOAT32 in the reference's operation order (the phases are f32-chaotic at real timestamps: a float64
    evaluation would be a different function).  Returns (features f32 [n, 9], angles f32 [n, 9]) -- angle_f is the argument of the
    sin / cos behind feature f (0 for the secular feature), which the tolerance of ur_context_mlp1 is stated in."""
    f32 = torch.float32
    x = ts.to(f32).reshape(-1)
    year, day, two_pi = torch.tensor(31557600.0, dtype=f32), torch.tensor(86400.0, dtype=f32), torch.tensor(2.0 * math.pi, dtype=f32)
    a_day = two_pi * (torch.remainder(x, day) / day)
    a_week = two_pi * (((x / day) + 4.0) / 7.0)
    year_phase = torch.remainder(x, year) / year
    a_year = two_pi * year_phase
    a_month = two_pi * (year_phase * 12.0)
    feats = [x / year]
    angles = [torch.zeros_like(x)]
    for a in (a_day, a_week, a_year, a_month):
        feats += [torch.sin(a), torch.cos(a)]
        angles += [a, a]
    return torch.stack(feats, -1), torch.stack(angles, -1)


def geo_features(coords):
    """(lat, lon) degrees [n, 2] -> unit-sphere (x, y, z), float32 as the reference; angle slack per feature = |lat| + |lon| for x, y
    (|d(cos a cos b)| <= |da| + |db|) and |lat| for z, returned as a pseudo-angle whose f32 ulp bounds the features' legitimate spread."""
    f32 = torch.float32
    c = coords.to(f32)
    d2r = torch.tensor(math.pi / 180.0, dtype=f32)
    lat, lon = c[:, 0] * d2r, c[:, 1] * d2r
    feats = torch.stack([torch.cos(lat) * torch.cos(lon), torch.cos(lat) * torch.sin(lon), torch.sin(lat)], -1)
    both = torch.maximum(lat.abs(), lon.abs()) * 2.0
    return feats, torch.stack([both, both, lat.abs()], -1)


def context_mlp1(feat, W1, b1):
    """gelu(b1 + W1 feat) in float64 over the given features: [n, H2]."""
    return gelu(feat.to(F64) @ W1.to(F64).t() + b1.to(F64))


# ---- fused attention (include/unirec_hip.h: ur_attn_fwd / ur_attn_bwd) -----------------------------------------------------
# Tensors use the ABI's layout: q, o, dout, dq [B, Sq, nq, hd]; k, v, dk, dv [B, Sk, nkv, hd]; key_mask [B, Sk] (1 = attend) or None;
# keep [B, nq, Sq, Sk] (0 / 1: oracle/dropout_ref.attn_keep) or None.  Probabilities / bounds on logits are [B, nq, Sq, Sk].
U_BF16 = 2.0 ** -8                  # bf16 unit roundoff as the bounds use it: the spacing of 8 significant bits (round-to-nearest costs half)
F32_SLACK = 2.0 ** -20              # what assert_f32_close grants f32 arithmetic
F32_MIN = float(torch.finfo(torch.float32).min)
LOG2E = 1.4426950408889634


def _bf(x):
    """round to bfloat16 (nearest even), keep the dtype"""
    return x.to(torch.bfloat16).to(x.dtype)


def _bh(x, dtype):
    return torch.as_tensor(x).detach().to("cpu").to(dtype).permute(0, 2, 1, 3)           # [B, heads, S, hd]


def _kv_to_q(x, rep):
    return x.repeat_interleave(rep, dim=1)                       # kv head of query head h = h // rep


def _q_to_kv(x, rep):
    B, nq, S, D = x.shape
    return x.reshape(B, nq // rep, rep, S, D).sum(2)             # dk / dv of a kv head: the sum over its query heads


def attention_allowed(key_mask, causal, B, Sq, Sk):
    """(ok [B, 1, Sq, Sk] bool: the keys a row's softmax runs over, live [B, 1, Sq]: rows with at least one allowed key).
    Non-causal (additive finfo(float32).min): a row without an allowed key is the uniform softmax over ALL Sk keys -- ok is all True there.
    Causal (SDPA): allowed = causal AND key mask; a row without an allowed key stays empty (o = 0, zero gradients)."""
    ok = torch.ones(B, 1, Sq, Sk, dtype=torch.bool)
    if key_mask is not None:
        ok = ok & torch.as_tensor(key_mask).cpu().bool()[:, None, None, :]
    if causal:
        ok = ok & torch.tril(torch.ones(Sq, Sk, dtype=torch.bool))[None, None]
    live = ok.any(-1)
    if not causal:
        ok = ok | ~live[..., None]
    return ok, live


def _attn_probs(qh, kh, ok, live, causal, scale):
    """P [B, nq, Sq, Sk] and lse [B, nq, Sq] of the masked, scaled logits (kh already expanded to the query heads).  A non-causal row
    without an allowed key has every logit EQUAL (finfo.min absorbs the score): uniform, lse = finfo.min + ln Sk."""
    s = (qh @ kh.transpose(-1, -2)) * scale
    if not causal:
        s = torch.where(live[..., None], s, torch.zeros_like(s))
    s = s.masked_fill(~ok, float("-inf"))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    P = torch.where(l > 0, e / l.clamp_min(1e-300), torch.zeros_like(e))
    lse = (m + torch.log(l)).squeeze(-1)
    if not causal:
        lse = torch.where(live.expand_as(lse), lse, torch.full_like(lse, F32_MIN) + math.log(s.shape[-1]))
    return P, lse


def _keep_scale(keep, p, dtype):
    if keep is None:
        return None
    return torch.as_tensor(keep).cpu().to(dtype) / (1.0 - p)


def attention_fwd(q, k, v, key_mask, causal, scale, keep=None, p=0.0, dtype=F64):
    """(o [B, Sq, nq, hd], P [B, nq, Sq, Sk] BEFORE dropout, lse [B, nq, Sq] = ln sum exp of the allowed scaled logits;
    -inf on a causal row without an allowed key).  o = (P * keep / (1 - p)) V."""
    qh, kh, vh = _bh(q, dtype), _bh(k, dtype), _bh(v, dtype)
    rep = qh.shape[1] // kh.shape[1]
    ok, live = attention_allowed(key_mask, causal, qh.shape[0], qh.shape[2], kh.shape[2])
    P, lse = _attn_probs(qh, _kv_to_q(kh, rep), ok, live, causal, scale)
    ks = _keep_scale(keep, p, dtype)
    Pt = P if ks is None else P * ks
    return (Pt @ _kv_to_q(vh, rep)).permute(0, 2, 1, 3), P, lse


def attention_bwd(q, k, v, key_mask, causal, scale, dout, keep=None, p=0.0, dtype=F64):
    """(dq, dk, dv) written out: dP = dO V^T (masked / scaled like P under dropout), delta = rowsum(dO * O), dS = P * (dP - delta),
    dQ = scale dS K, dK = scale dS^T Q, dV = (P keep / (1 - p))^T dO; dk / dv of a kv head sum over its query heads."""
    qh, kh, vh, doh = _bh(q, dtype), _bh(k, dtype), _bh(v, dtype), _bh(dout, dtype)
    rep = qh.shape[1] // kh.shape[1]
    kq, vq = _kv_to_q(kh, rep), _kv_to_q(vh, rep)
    ok, live = attention_allowed(key_mask, causal, qh.shape[0], qh.shape[2], kh.shape[2])
    P, _ = _attn_probs(qh, kq, ok, live, causal, scale)
    ks = _keep_scale(keep, p, dtype)
    Pt = P if ks is None else P * ks
    o = Pt @ vq
    dP = doh @ vq.transpose(-1, -2)
    if ks is not None:
        dP = dP * ks
    delta = (doh * o).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    dq = scale * (dS @ kq)
    dk = _q_to_kv(scale * (dS.transpose(-1, -2) @ qh), rep)
    dv = _q_to_kv(Pt.transpose(-1, -2) @ doh, rep)
    return dq.permute(0, 2, 1, 3), dk.permute(0, 2, 1, 3), dv.permute(0, 2, 1, 3)


def attention_bounds(q, k, v, key_mask, causal, scale, dout, keep=None, p=0.0, qk_rounded=False):
    """The magnitudes A of the a-priori running-error bound |got - ref| <= (U_BF16 + F32_SLACK) * A, one term per point where the
    kernel path rounds to bf16 (docs/lab_notes.md, "Element-wise float64 tests: attention"), from the float64 reference's own
    quantities:
        A_o  = Pt |V| + |o|                                     (Pt = P keep / (1 - p) rounded for the PV product; o rounded at the store)
        A_dv = Pt^T |dO| + |dv|
        A_dS = P (2 |dPt - delta| + rowsum(|dO| (|o| + A_o)))    (dS rounded for its two products; delta is formed from the bf16 o)
        A_dq = scale A_dS |K| + |dq|,   A_dk = scale A_dS^T |Q| + |dk|
    qk_rounded (the generated causal head_dim-128 kernels round q * scale * log2 e, resp. k * scale * log2 e, to bf16 once more): every
    logit moves by at most u * E, E = scale |q| . |k|, hence P by at most u * A_P, A_P = P (E + rowsum(P E)) to first order, and lse by
    at most u * rowsum(P E); A_o, A_dv and A_dS receive the A_P term.  Returns a dict of A_o, A_dq, A_dk, A_dv (ABI layout) and
    A_lse [B, nq, Sq]."""
    qh, kh, vh, doh = _bh(q, F64), _bh(k, F64), _bh(v, F64), _bh(dout, F64)
    rep = qh.shape[1] // kh.shape[1]
    kq, vq = _kv_to_q(kh, rep), _kv_to_q(vh, rep)
    ok, live = attention_allowed(key_mask, causal, qh.shape[0], qh.shape[2], kh.shape[2])
    P, _ = _attn_probs(qh, kq, ok, live, causal, scale)
    ks = _keep_scale(keep, p, F64)
    Pt = P if ks is None else P * ks
    o = Pt @ vq
    dP = doh @ vq.transpose(-1, -2)
    if ks is not None:
        dP = dP * ks
    delta = (doh * o).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    dq = scale * (dS @ kq)
    dk = _q_to_kv(scale * (dS.transpose(-1, -2) @ qh), rep)
    dv = _q_to_kv(Pt.transpose(-1, -2) @ doh, rep)
    A_o = Pt @ vq.abs() + o.abs()
    A_dv_q = Pt.transpose(-1, -2) @ doh.abs()
    A_lse = torch.zeros(P.shape[:-1], dtype=F64)
    A_P = None
    if qk_rounded:
        E = scale * (qh.abs() @ kq.abs().transpose(-1, -2))
        PE = (P * E).sum(-1, keepdim=True)
        A_P = P * (E + PE)
        A_lse = PE.squeeze(-1)
        A_o = A_o + A_P @ vq.abs()
        A_dv_q = A_dv_q + A_P.transpose(-1, -2) @ doh.abs()
    A_dS = P * (2.0 * (dP - delta).abs() + (doh.abs() * (o.abs() + A_o)).sum(-1, keepdim=True))
    if A_P is not None:
        A_dS = A_dS + A_P * (dP - delta).abs()
    A_dq = scale * (A_dS @ kq.abs()) + dq.abs()
    A_dk = _q_to_kv(scale * (A_dS.transpose(-1, -2) @ qh.abs()), rep) + dk.abs()
    A_dv = _q_to_kv(A_dv_q, rep) + dv.abs()
    perm = lambda t: t.permute(0, 2, 1, 3)                       # noqa: E731
    return {"o": perm(A_o), "dq": perm(A_dq), "dk": perm(A_dk), "dv": perm(A_dv), "lse": A_lse}


ATTN_MUTANTS = ("drop_key_tile", "diagonal_shift", "kv_head_mod", "no_delta", "bwd_no_drop_scale", "masked_row_zero")


def attention_emulated(q, k, v, key_mask, causal, scale, dout, keep=None, p=0.0, qk_round=None, mutant=None):
    """The kernels' arithmetic restated in float32 torch with a bf16 rounding at every point the bound lists: (o, dq, dk, dv), bf16
    values in float64.  Its error against the float64 reference is the yardstick of the Frobenius criterion -- never the kernel's own.
        o  = bf((bf(Et) V) / l), Et = exp(s - row max) keep / (1 - p),  delta = rowsum(dO * o),  dS = P (dPt - delta),
        dq = bf(bf(scale dS) K),  dk = bf(scale bf(dS)^T Q),  dv = bf(bf(Pt)^T dO)
    qk_round: None (generic kernels); "fwd" (generated forward, generic backward: only lse carries the rounded q);
    "all" (generated forward + dQ round q * scale * log2 e, generated dK/dV rounds k * scale * log2 e, all normalised by the forward's lse).
    mutant: one of ATTN_MUTANTS -- a DELIBERATE bug, for tests/test_ref64.py to show that the criteria bite (keep-flag swaps need no hook:
    feed other flags)."""
    assert mutant is None or mutant in ATTN_MUTANTS, mutant
    f32 = torch.float32
    qh, kh, vh, doh = _bh(q, f32), _bh(k, f32), _bh(v, f32), _bh(dout, f32)
    B, nq, Sq, D = qh.shape
    nkv, Sk = kh.shape[1], kh.shape[2]
    rep = nq // nkv
    if mutant == "kv_head_mod":
        idx = torch.arange(nq) % nkv
        kq, vq = kh[:, idx], vh[:, idx]
    else:
        kq, vq = _kv_to_q(kh, rep), _kv_to_q(vh, rep)
    ok, live = attention_allowed(key_mask, causal, B, Sq, Sk)
    if mutant == "drop_key_tile" and Sk > 64:                   # the last 64-key tile is never swept
        ok = ok.clone()
        ok[..., ((Sk - 1) // 64) * 64:] = False
    if mutant == "diagonal_shift" and causal:                   # key <= query - 1
        ok = ok & torch.tril(torch.ones(Sq, Sk, dtype=torch.bool), diagonal=-1)[None, None]
    if mutant == "masked_row_zero" and not causal and key_mask is not None:
        ok = ok & torch.as_tensor(key_mask).cpu().bool()[:, None, None, :]
    c = scale * LOG2E

    def probs(qs, ks_, lse=None):
        s = qs @ ks_.transpose(-1, -2)
        if not causal:
            s = torch.where(live[..., None], s, torch.zeros_like(s))
        s = s.masked_fill(~ok, float("-inf"))
        if lse is None:
            m = s.amax(-1, keepdim=True)
            m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
            l = torch.exp(s - m).sum(-1, keepdim=True)
            lse = torch.where(l > 0, m + torch.log(l), torch.full_like(m, float("inf")))
        return torch.exp(s - lse), lse, s

    q_r, k_r = _bf(qh * c) / LOG2E, _bf(kq * c) / LOG2E          # natural-log logits from the re-rounded operand
    if qk_round is None:
        P, lse, s_f = probs(qh * scale, kq)
        P_dq = P_dkv = P
    else:
        P, lse, s_f = probs(q_r, kq)
        P_dq = P if qk_round == "all" else probs(qh * scale, kq, lse)[0]
        P_dkv = probs(qh, k_r, lse)[0] if qk_round == "all" else P_dq
    # the forward rounds the UNNORMALISED probabilities exp(s - row max) (the maximum itself stays exactly 1) and divides by l at the store
    m_f = s_f.amax(-1, keepdim=True)
    m_f = torch.where(torch.isfinite(m_f), m_f, torch.zeros_like(m_f))
    e_f = torch.exp(s_f - m_f)
    l_f = e_f.sum(-1, keepdim=True)
    inv_f = torch.where(l_f > 0, 1.0 / l_f.clamp_min(1e-30), torch.zeros_like(l_f))
    ks = _keep_scale(keep, p, f32)
    one = torch.ones((), dtype=f32)
    fs, bs = (one if ks is None else ks), (one if ks is None else ks)
    if mutant == "bwd_no_drop_scale" and ks is not None:
        bs = ks * (1.0 - p)
    o = _bf((_bf(e_f * fs) @ vq) * inv_f)
    dP = doh @ vq.transpose(-1, -2)
    delta = (doh * o).sum(-1, keepdim=True)
    if mutant == "no_delta":
        delta = torch.zeros_like(delta)
    dq = _bf(_bf(scale * P_dq * (dP * bs - delta)) @ kq)
    dS = _bf(P_dkv * (dP * bs - delta))
    dk_q = scale * (dS.transpose(-1, -2) @ qh)
    dv_q = _bf(P_dkv * bs).transpose(-1, -2) @ doh
    if mutant == "kv_head_mod":
        dk = torch.zeros_like(kh).index_add_(1, idx, dk_q)
        dv = torch.zeros_like(vh).index_add_(1, idx, dv_q)
    else:
        dk, dv = _q_to_kv(dk_q, rep), _q_to_kv(dv_q, rep)
    return tuple(_bf(t).permute(0, 2, 1, 3).to(F64) for t in (o, dq, dk, dv))


def attention_emulated_tiled(q, k, v, key_mask, causal, scale, dout, keep=None, p=0.0, tile=64, defer=6.0):
    """A second, independently built correct emulation, for measuring how far two correct implementations lie apart in the Frobenius
    criterion's norm (the margin 3): keys swept in tiles with an online softmax, the running maximum moved only when it grows by more
    than 2^defer (probabilities above 1 in between), UNNORMALISED probabilities rounded for the PV product and o normalised at the end,
    delta from the unrounded o, the dS scale applied after the dK product and before the dQ one, partial sums per tile."""
    f32 = torch.float32
    qh, kh, vh, doh = _bh(q, f32), _bh(k, f32), _bh(v, f32), _bh(dout, f32)
    B, nq, Sq, D = qh.shape
    nkv, Sk = kh.shape[1], kh.shape[2]
    rep = nq // nkv
    kq, vq = _kv_to_q(kh, rep), _kv_to_q(vh, rep)
    ok, live = attention_allowed(key_mask, causal, B, Sq, Sk)
    ks = _keep_scale(keep, p, f32)
    s = (qh @ kq.transpose(-1, -2)) * scale
    if not causal:
        s = torch.where(live[..., None], s, torch.zeros_like(s))
    s = s.masked_fill(~ok, float("-inf"))
    m = torch.full((B, nq, Sq, 1), float("-inf"), dtype=f32)
    l = torch.zeros((B, nq, Sq, 1), dtype=f32)
    acc = torch.zeros((B, nq, Sq, D), dtype=f32)
    for k0 in range(0, Sk, tile):
        st = s[..., k0:k0 + tile]
        mx = st.amax(-1, keepdim=True)
        grow = ~(mx <= m + defer * math.log(2.0))
        mnew = torch.where(grow, torch.maximum(m, mx), m)
        mu = torch.where(torch.isfinite(mnew), mnew, torch.zeros_like(mnew))
        alpha = torch.exp(torch.where(torch.isfinite(m), m, torch.full_like(m, -1e30)) - mu).clamp_max(1.0)
        alpha = torch.where(torch.isfinite(m), alpha, torch.zeros_like(alpha))
        l, acc, m = l * alpha, acc * alpha, mnew
        e = torch.exp(st - mu)
        l = l + e.sum(-1, keepdim=True)
        if ks is not None:
            e = e * ks[..., k0:k0 + tile]
        acc = acc + _bf(e) @ vq[:, :, k0:k0 + tile]
    inv = torch.where(l > 0, 1.0 / l.clamp_min(1e-30), torch.zeros_like(l))
    o32 = acc * inv
    o = _bf(o32)
    mu = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    delta = (doh * o32).sum(-1, keepdim=True)
    dq = torch.zeros_like(qh)
    dk_q = torch.zeros((B, nq, Sk, D), dtype=f32)
    dv_q = torch.zeros((B, nq, Sk, D), dtype=f32)
    for k0 in range(0, Sk, tile):
        sl = slice(k0, k0 + tile)
        P = torch.exp(s[..., sl] - mu) * inv
        dP = doh @ vq[:, :, sl].transpose(-1, -2)
        Pt = P
        if ks is not None:
            dP, Pt = dP * ks[..., sl], P * ks[..., sl]
        dS = _bf(P * (dP - delta))
        dq = dq + dS @ kq[:, :, sl]
        dk_q[:, :, sl] = dS.transpose(-1, -2) @ qh
        dv_q[:, :, sl] = _bf(Pt).transpose(-1, -2) @ doh
    dq = dq * scale
    dk, dv = _q_to_kv(dk_q * scale, rep), _q_to_kv(dv_q, rep)
    return tuple(_bf(t).permute(0, 2, 1, 3).to(F64) for t in (o, dq, dk, dv))


def attn_bound_ratio(got, ref64, A):
    """max over EVERY element of |got - ref| / ((U_BF16 + F32_SLACK) * A); 0 / 0 counts as 0, x / 0 as inf."""
    g, r, a = _cpu64(got), _cpu64(ref64), _cpu64(A)
    err, bound = (g - r).abs(), (U_BF16 + F32_SLACK) * a
    ratio = torch.where(err <= bound, err / bound.clamp_min(1e-300), torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.full_like(err, float("inf"))))
    ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)
    return ratio


def assert_attn_bound(got, ref64, A, what=""):
    """EVERY element: |got - ref| <= U_BF16 * A + F32_SLACK * A, everything finite.  Returns the worst error / bound."""
    g, r = _cpu64(got), _cpu64(ref64)
    assert g.shape == r.shape == tuple(A.shape), f"{what}: shapes {tuple(g.shape)} / {tuple(r.shape)} / {tuple(A.shape)}"
    assert torch.isfinite(r).all() and torch.isfinite(_cpu64(A)).all(), f"{what}: the reference itself is not finite"
    if g.numel() == 0:
        return 0.0
    bad = ~torch.isfinite(g)
    if bad.any():
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} non-finite outputs, first at {i}: got {g[i].item()}, reference {r[i].item()}")
    ratio = attn_bound_ratio(g, r, A)
    off = ratio > 1.0
    if off.any():
        i = tuple(int(v) for v in torch.unravel_index(ratio.argmax(), ratio.shape))
        raise AssertionError(f"{what}: {int(off.sum())} of {ratio.numel()} elements exceed (2^-8 + 2^-20) * A; worst at index {i}: got {g[i].item()!r}, "
                             f"reference {r[i].item()!r}, error {abs(g[i].item() - r[i].item()):.3e} = {ratio[i].item():.2f} x the bound (A {_cpu64(A)[i].item():.3e})")
    return float(ratio.max())


def attn_frob_ratio(got, ref64, emul, A, margin=3.0):
    """per (batch, head) slice of an ABI-layout tensor [B, S, heads, hd]: ||got - ref||_F / (margin * ||emul - ref||_F + F32_SLACK * ||A||_F)"""
    g, r, e, a = _cpu64(got), _cpu64(ref64), _cpu64(emul), _cpu64(A)
    nrm = lambda t: t.pow(2).sum(dim=(1, 3)).sqrt()               # noqa: E731
    err, bound = nrm(g - r), margin * nrm(e - r) + F32_SLACK * nrm(a)
    return torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))


def assert_attn_frob(got, ref64, emul, A, what="", margin=3.0):
    """Every (batch, head) slice: ||got - ref||_F <= 3 * ||emul - ref||_F + 2^-20 * ||A||_F.  Returns the worst ratio."""
    g = _cpu64(got)
    if g.numel() == 0:
        return 0.0
    assert torch.isfinite(g).all(), f"{what}: non-finite outputs"
    ratio = attn_frob_ratio(g, ref64, emul, A, margin)
    off = ratio > 1.0
    if off.any():
        i = tuple(int(v) for v in torch.unravel_index(ratio.argmax(), ratio.shape))
        raise AssertionError(f"{what}: {int(off.sum())} of {ratio.numel()} (batch, head) slices exceed {margin} x the emulation's Frobenius error; "
                             f"worst at (batch, head) {i}: {ratio[i].item():.2f} x the bound")
    return float(ratio.max())


# ---- LayerNorm / RMSNorm / batch reduce / GEMM epilogue (include/unirec_hip.h: ur_layernorm_*, ur_rmsnorm_*, ur_batch_reduce, ur_gemm) ---
def assert_bf16_rows(got, ref64, ref32, what="", scale=None, floor=2.0 ** -18):
    """bf16 outputs of the row-normalising kernels.  EVERY element:
        |got - ref64| <= 1 bf16 ulp(ref64) + 2^-18 * row max |ref64| + 8 * e32_row,   e32_row = row max |ref32 - ref64|,
    ref32 the SAME two-pass formula in float32 torch on the CPU (the yardstick of assert_f32_close).  The e32 term is there for rows whose
    mean dwarfs their spread (docs/lab_notes.md, "Element-wise float64 tests: norm, reduction and GEMM epilogue kernels"); on centred rows
    it is far below the first two.  scale [rows, 1]: the row scale of the floor where it is not the row maximum of ref64 itself -- the
    UNMASKED row of a dropout-masked output, whose cancellation error does not shrink when the mask removes the row's large elements.
    floor = 0: 1 ulp + 8 * e32_row alone (z_save under pre-dropout).  Everything finite.  Returns the worst error / bound."""
    r, r32 = _cpu64(ref64), _cpu64(ref32)
    assert r.shape == r32.shape, f"{what}: shapes {tuple(r.shape)} / {tuple(r32.shape)}"
    assert torch.isfinite(r32).all(), f"{what}: the float32 re-evaluation of the reference is not finite"
    if r.numel() == 0:
        return assert_within_ulps(got, r, 1, 0.0, what)
    e32 = (r32 - r).abs().amax(dim=-1, keepdim=True)
    sc = r.abs().amax(dim=-1, keepdim=True) if scale is None else _cpu64(scale).reshape(-1, 1)
    return assert_within_ulps(got, r, 1, floor * sc + 8.0 * e32, what)


GELU_TAIL = 1e-6                    # |gelu(x)| at or below this: the fitted Phi of common.hip.h (and float32 erf itself) is held absolutely


def assert_gelu_close(got, x, what=""):
    """gelu outputs (bf16) of the bf16 inputs x: 1 bf16 ulp of the float64 value wherever |gelu(x)| > 1e-6 -- the region in which
    tests/test_gelu_cdf.py demands the exact bf16 of the emulation --, |error| <= 1e-6 below it (x < -5 and |x| < 2e-6: float32
    0.5 x (1 + erf(x / sqrt 2)) returns -0 for every x <= -5.6, docs/lab_notes.md).  Returns the worst error / bound."""
    g, r = _cpu64(got), gelu(_cpu64(x))
    big = r.abs() > GELU_TAIL
    z = torch.zeros_like(r)
    ratio = assert_within_ulps(torch.where(big, g, z), torch.where(big, r, z), 1, 0.0, what)
    assert torch.isfinite(g).all(), f"{what}: non-finite outputs"
    err = torch.where(big, z, (g - r).abs())
    if (err > GELU_TAIL).any():
        i = tuple(int(v) for v in torch.unravel_index(err.argmax(), err.shape))
        raise AssertionError(f"{what}: {int((err > GELU_TAIL).sum())} outputs with |gelu(x)| <= 1e-6 are off by more than 1e-6; worst at {i}: "
                             f"got {g[i].item()!r}, reference {r[i].item()!r}")
    return max(ratio, float(err.max()) / GELU_TAIL)


def assert_colsum_close(got, ref64, ref32, abs_terms, what=""):
    """f32 column sums over M rows (dgamma, dbeta, dbias, ur_batch_reduce).  EVERY column:
        |got - ref64| <= 8 * |ref32 - ref64| + 2^-20 * sum_m |term|      (abs_terms = that sum per column; ref32 = ref64 where the terms are given
    exactly and only the summation rounds).  Everything finite.  Returns the worst error / bound (0 / 0 counts as 0)."""
    g, r, r32, a = _cpu64(got), _cpu64(ref64), _cpu64(ref32), _cpu64(abs_terms)
    assert g.shape == r.shape == r32.shape == a.shape, f"{what}: shapes {tuple(g.shape)} / {tuple(r.shape)} / {tuple(r32.shape)} / {tuple(a.shape)}"
    assert torch.isfinite(r).all() and torch.isfinite(r32).all(), f"{what}: the reference itself is not finite"
    if g.numel() == 0:
        return 0.0
    bad = ~torch.isfinite(g)
    if bad.any():
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} non-finite outputs, first at {i}: got {g[i].item()}, reference {r[i].item()}")
    err, bound = (g - r).abs(), 8.0 * (r32 - r).abs() + 2.0 ** -20 * a
    off = err > bound
    if off.any():
        excess = torch.where(off, err - bound, torch.zeros_like(err))
        i = tuple(int(v) for v in torch.unravel_index(excess.argmax(), err.shape))
        raise AssertionError(f"{what}: {int(off.sum())} of {err.numel()} sums exceed 8 * e32 + 2^-20 * sum |term|; worst at index {i}: got {g[i].item()!r}, "
                             f"reference {r[i].item()!r}, error {err[i].item():.3e}, allowed {bound[i].item():.3e} (sum |term| {a[i].item():.3e})")
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300)).max())


def _drop_scale(keep, p, dtype):
    if keep is None:
        return None
    return torch.as_tensor(keep).to(dtype) / torch.as_tensor(1.0 - p, dtype=dtype)


def layernorm_z(y, residual=None, keep_pre=None, p_pre=0.0, y_rows=None, M=None, dtype=F64):
    """z = y[m % y_rows] * keep_pre / (1 - p_pre) + residual, UNROUNDED: [M, H]."""
    y = torch.as_tensor(y).detach().cpu()
    y = y.reshape(-1, y.shape[-1]).to(dtype)
    y_rows = y.shape[0] if y_rows is None else int(y_rows)
    M = y_rows if M is None else int(M)
    z = y[torch.arange(M) % y_rows]
    s = _drop_scale(keep_pre, p_pre, dtype)
    if s is not None:
        z = z * s
    if residual is not None:
        z = z + torch.as_tensor(residual).detach().cpu().to(dtype)
    return z


def layernorm_of_z(z, gamma, beta, eps, keep_post=None, p_post=0.0, dtype=F64):
    """(out, mean, rstd, xhat) of the given z, two-pass: mean, then the mean of the squared deviations."""
    z = z.to(dtype)
    mean = z.mean(-1, keepdim=True)
    d = z - mean
    rstd = torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)
    xhat = d * rstd
    out = xhat * gamma.to(dtype) + beta.to(dtype)
    s = _drop_scale(keep_post, p_post, dtype)
    if s is not None:
        out = out * s
    return out, mean.squeeze(-1), rstd.squeeze(-1), xhat


def layernorm_fwd(y, residual, gamma, beta, eps, keep_pre=None, p_pre=0.0, keep_post=None, p_post=0.0, y_rows=None, M=None, dtype=F64):
    """(z, out, mean, rstd): z = bf16(dropout_pre(y) + residual) -- the value the kernel saves --, out = dropout_post(LN(z) * gamma + beta)
    of that ROUNDED z, as the kernel normalises it by design (forward and backward see the same z).  keep_* [M, H] 0 / 1
    (oracle/dropout_ref.hidden_keep) or None."""
    z = _bf(layernorm_z(y, residual, keep_pre, p_pre, y_rows, M, dtype))
    out, mean, rstd, _ = layernorm_of_z(z, gamma, beta, eps, keep_post, p_post, dtype)
    return z, out, mean, rstd


def layernorm_bwd(dout, z, gamma, eps, keep_pre=None, p_pre=0.0, keep_post=None, p_post=0.0, dtype=F64):
    """(dz, dy, dgamma, dbeta): torch.autograd through the forward from z; dy = dz * keep_pre / (1 - p_pre)."""
    zz = torch.as_tensor(z).detach().cpu().to(dtype).clone().requires_grad_(True)
    g = gamma.detach().cpu().to(dtype).clone().requires_grad_(True)
    b = torch.zeros_like(g).requires_grad_(True)
    out, _, _, _ = layernorm_of_z(zz, g, b, eps, keep_post, p_post, dtype)
    dz, dg, db = torch.autograd.grad(out, (zz, g, b), torch.as_tensor(dout).detach().cpu().to(dtype))
    s = _drop_scale(keep_pre, p_pre, dtype)
    return dz, (dz if s is None else dz * s), dg, db


def layernorm_bwd_terms(dout, z, eps, keep_post=None, p_post=0.0):
    """(sum_m |dout' * xhat|, sum_m |dout'|) per column, dout' = dout * keep_post / (1 - p_post): what the dgamma / dbeta sums run over."""
    zz = torch.as_tensor(z).detach().cpu().to(F64)
    d = torch.as_tensor(dout).detach().cpu().to(F64)
    s = _drop_scale(keep_post, p_post, F64)
    if s is not None:
        d = d * s
    xhat = layernorm_of_z(zz, torch.ones(zz.shape[-1], dtype=F64), torch.zeros(zz.shape[-1], dtype=F64), eps)[3]
    return (d * xhat).abs().sum(0), d.abs().sum(0)


def rmsnorm_fwd(x, w, eps, dtype=F64):
    """(out, rstd): out = w * (x * rsqrt(mean(x^2) + eps))."""
    x = torch.as_tensor(x).to(dtype)
    rstd = torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    return w.to(dtype) * (x * rstd), rstd.squeeze(-1)


def rmsnorm_bwd(dout, x, w, eps, add=None, dtype=F64):
    """dx = add + d out / d x (weights frozen): torch.autograd through the forward."""
    xx = torch.as_tensor(x).detach().cpu().to(dtype).clone().requires_grad_(True)
    out, _ = rmsnorm_fwd(xx, w.detach().cpu(), eps, dtype)
    (dx,) = torch.autograd.grad(out, xx, torch.as_tensor(dout).detach().cpu().to(dtype))
    return dx if add is None else dx + torch.as_tensor(add).detach().cpu().to(dtype)


def batch_reduce(x, nb, rows, H, dtype=F64):
    """out[r][h] = sum_{b < nb} in[b * rows + r][h]: [rows, H]."""
    return torch.as_tensor(x).detach().cpu().to(dtype).reshape(nb, rows, H).sum(0)


def gemm_epilogue(acc, alpha=1.0, bias=None, residual=None, aux=None, dtype=F64):
    """v = (alpha * acc + bias[n] + residual[m][n]) * gelu'(aux[m][n]) of the EXACT product acc [M, N]; the kernel stores C = bf16(v) and
    gelu_out = bf16(gelu(C)) (ur_gemm_args)."""
    v = torch.as_tensor(alpha, dtype=dtype) * acc.to(dtype)
    if bias is not None:
        v = v + bias.to(dtype)[None, :]
    if residual is not None:
        v = v + residual.to(dtype)
    if aux is not None:
        v = v * gelu_grad(aux).to(dtype)
    return v


def gelu_grad_f32(u):
    """gelu'(u) = Phi(u) + u phi(u) with every step in float32 torch, Phi = 0.5 (1 + erf(u / sqrt 2)) as the reference model's own GELU forms
    it: absolutely accurate (about 1e-7), not relatively -- below u = -5 it is a difference of two numbers of 1e-7 and smaller"""
    f32 = torch.float32
    u = torch.as_tensor(u).to(f32)
    cdf = 0.5 * (1.0 + torch.erf(u * torch.tensor(1.0 / math.sqrt(2.0), dtype=f32)))
    return cdf + u * (torch.exp(-0.5 * u * u) * torch.tensor(1.0 / math.sqrt(2.0 * math.pi), dtype=f32))


def _ratio(err, bound):
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0


def assert_gemm_c(C, acc, alpha, bias=None, residual=None, what=""):
    """bf16 C of an exact product without the gelu' factor: 1 bf16 ulp + 2^-20 (|alpha acc| + |bias| + |res|) around v = alpha acc + bias + res
    (three float32 roundings of terms of those magnitudes).  Returns the worst error / bound."""
    v = gemm_epilogue(acc, alpha, bias, residual)
    mag = (alpha * acc.to(F64)).abs()
    if bias is not None:
        mag = mag + bias.to(F64).abs()[None, :]
    if residual is not None:
        mag = mag + residual.to(F64).abs()
    return assert_within_ulps(C, v, 1, 2.0 ** -20 * mag, what)


def assert_gemm_gelu_grad(C, acc, alpha, bias, residual, aux, what=""):
    """bf16 C = bf16(pre * gelu'(aux)), pre = alpha acc + bias + res: 1 bf16 ulp + 2^-18 |pre| + 2^-20 (|alpha acc| + |bias| + |res|) |gelu'(aux)|
    -- the floor of test_gelu_bwd_exhaustive (2^-18 |dy|), pre being what the factor multiplies, and the floor assert_gemm_c grants pre.  gelu' = Phi + u phi is held ABSOLUTELY by float32 arithmetic (gelu_grad_f32: below
    u = -5 it is the difference of two numbers of 1e-7; tests/test_ref64.py shows the float32 evaluation missing 2^-18 |pre gelu'| there and
    meeting 2^-18 |pre|).  Returns the worst error / bound."""
    v, pre = gemm_epilogue(acc, alpha, bias, residual, aux), gemm_epilogue(acc, alpha, bias, residual)
    mag = (alpha * acc.to(F64)).abs()
    if bias is not None:
        mag = mag + bias.to(F64).abs()[None, :]
    if residual is not None:
        mag = mag + residual.to(F64).abs()
    # + assert_gemm_c's floor of pre itself, seen through the factor: alpha acc + bias + res may cancel (three float32 roundings of its terms)
    return assert_within_ulps(C, v, 1, 2.0 ** -18 * pre.abs() + 2.0 ** -20 * mag * gelu_grad(aux).abs(), what)


def assert_gemm_f32(C32, acc, alpha, bias=None, what=""):
    """f32 output: |got - (alpha acc + bias)| <= 2^-22 (|alpha acc| + |bias|), everything finite.  Returns the worst error / bound."""
    g, v = _cpu64(C32), gemm_epilogue(acc, alpha, bias)
    assert torch.isfinite(g).all(), f"{what}: non-finite outputs"
    bound = 2.0 ** -22 * ((alpha * acc.to(F64)).abs() + (bias.to(F64).abs()[None, :] if bias is not None else 0.0))
    err = (g - v).abs()
    assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} elements exceed 2^-22 (|alpha acc| + |bias|), worst {_ratio(err, bound):.2f} x"
    return _ratio(err, bound)


NORM_MUTANTS = ("one_pass_variance", "no_m1", "gelu_unrounded", "bias_after_gelu_grad")


def norm_emulated(z, gamma, beta, eps, dout, mutant=None):
    """The LayerNorm kernels' arithmetic in float32 torch, outputs rounded to bf16: (out, dz).  mutant: 'one_pass_variance' (var = E[z^2] -
    mean^2 in the forward) or 'no_m1' (the backward loses the mean of dout * gamma) -- DELIBERATE bugs, for tests/test_ref64.py."""
    assert mutant in (None, "one_pass_variance", "no_m1"), mutant
    f32 = torch.float32
    z, g, b, d = z.to(f32), gamma.to(f32), beta.to(f32), dout.to(f32)
    mean = z.mean(-1, keepdim=True)
    if mutant == "one_pass_variance":
        var = (z * z).mean(-1, keepdim=True) - mean * mean
    else:
        var = ((z - mean) ** 2).mean(-1, keepdim=True)
    rs = torch.rsqrt(var + eps)
    xh = (z - mean) * rs
    out = xh * g + b
    go = d * g
    m1 = go.mean(-1, keepdim=True) if mutant != "no_m1" else torch.zeros_like(mean)
    m2 = (go * xh).mean(-1, keepdim=True)
    dz = rs * (go - m1 - xh * m2)
    return _bf(out).to(F64), _bf(dz).to(F64)


def gemm_epilogue_emulated(acc, alpha, bias, residual, aux, mutant=None):
    """The GEMM epilogue in float32 torch (gelu' too: gelu_grad_f32): (C, gelu_out) as bf16 values in float64.  mutant: 'gelu_unrounded' (gelu_out from v instead of
    bf16(v)) or 'bias_after_gelu_grad' (v = (alpha acc + res) * gelu'(aux) + bias)."""
    assert mutant in (None, "gelu_unrounded", "bias_after_gelu_grad"), mutant
    f32 = torch.float32
    v = acc.to(f32) * alpha
    fac = gelu_grad_f32(aux) if aux is not None else None
    if mutant == "bias_after_gelu_grad":
        if residual is not None:
            v = v + residual.to(f32)
        if fac is not None:
            v = v * fac
        if bias is not None:
            v = v + bias.to(f32)[None, :]
    else:
        if bias is not None:
            v = v + bias.to(f32)[None, :]
        if residual is not None:
            v = v + residual.to(f32)
        if fac is not None:
            v = v * fac
    C = _bf(v)
    g = gelu(v if mutant == "gelu_unrounded" else C).to(f32)
    return C.to(F64), _bf(g).to(F64)


# ---- LoRA adapter kernels (include/unirec_hip.h: ur_lora_project / ur_lora_reduce / ur_lora_bgrad, ur_gemm's masked epilogue,
#      ur_rmsnorm_lora_fwd, ur_swiglu_lora_fwd; formulas: header comment of csrc/lora.hip) -------------------------------------------
# X [M, W] bf16; U: list of [r, width_a]; V [M, r nad]; keep [nad, M, W] 0 / 1 or None; cols None (the adapters share all of X) or
# [(c0, width)] (adapter a owns that range).  dtype=torch.float32 re-evaluates the same formula in float32 (the e32 yardstick);
# absolute=True returns sum |term| (with |alpha|), the magnitude the accumulation term of the criteria scales with.
def _lora_cols(X, nad, cols):
    return [(0, X.shape[1])] * nad if cols is None else list(cols)


def _lora_x(X, keep, a, c0, w, dtype):
    xa = torch.as_tensor(X).detach().cpu()[:, c0:c0 + w].to(dtype)
    return xa if keep is None else xa * torch.as_tensor(keep[a]).to(dtype)


def _scaled(t, alpha, dtype, absolute):
    return t * torch.as_tensor(abs(alpha) if absolute else alpha, dtype=dtype)


def lora_project(X, U, keep=None, alpha=1.0, cols=None, dtype=F64, absolute=False):
    """P[m, r a + j] = alpha * sum_w keep_a(m, w) X[m, c0_a + w] U_a[j, w]: [M, r nad]."""
    outs = []
    for a, (c0, w) in enumerate(_lora_cols(X, len(U), cols)):
        xa, ua = _lora_x(X, keep, a, c0, w, dtype), U[a].detach().cpu().to(dtype)
        outs.append(xa.abs() @ ua.abs().t() if absolute else xa @ ua.t())
    return _scaled(torch.cat(outs, 1), alpha, dtype, absolute)


def lora_reduce(X, V, rank, nad, keep=None, alpha=1.0, cols=None, transposed=False, dtype=F64, absolute=False):
    """G_a[j, w] = alpha * sum_m V[m, r a + j] keep_a(m, w) X[m, c0_a + w], the dense output FLATTENED: entry a after entry a - 1, each
    [r, width_a] or, transposed, [width_a, r]."""
    v = torch.as_tensor(V).detach().cpu().to(dtype)
    outs = []
    for a, (c0, w) in enumerate(_lora_cols(X, nad, cols)):
        xa, va = _lora_x(X, keep, a, c0, w, dtype), v[:, rank * a:rank * (a + 1)]
        g = va.abs().t() @ xa.abs() if absolute else va.t() @ xa
        outs.append((g.t() if transposed else g).reshape(-1))
    return _scaled(torch.cat(outs), alpha, dtype, absolute)


def lora_bgrad(dy, t, Bt, cols, alpha=1.0, dtype=F64, absolute=False):
    """(tb [M, r nad] = alpha * dy_a B_a, dB flattened: entry a = dy_a^T t_a [width_a, r]) -- alpha scales tb only."""
    r = Bt[0].shape[0]
    tb = lora_project(dy, Bt, None, alpha, cols, dtype, absolute)
    dB = lora_reduce(dy, t, r, len(cols), None, 1.0, cols, True, dtype, absolute)
    return tb, dB


def lora_masked_epilogue(R, S, tb, A, keep, p, rank, dtype=F64, absolute=False):
    """C = R S^T + sum_a keep_a / (1 - p) * (tb_a A_a): [M, N]; A [r nad, N], adapter a = rows r a .. of A and columns r a .. of tb."""
    c = lambda t: torch.as_tensor(t).detach().to(dtype)      # noqa: E731    (on the inputs' device: tests/test_gpu_gemm_f64.py keeps them on the GPU)
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)
    R, S, tb, A = ab(c(R)), ab(c(S)), ab(c(tb)), ab(c(A))
    out = R @ S.t()
    inv = torch.as_tensor(1.0, dtype=dtype) / torch.as_tensor(1.0 - p, dtype=dtype)
    for a in range(A.shape[0] // rank):
        out = out + c(keep[a]) * inv * (tb[:, rank * a:rank * (a + 1)] @ A[rank * a:rank * (a + 1)])
    return out


def rms_lora_t(h_saved, U, keep=None, alpha=1.0, dtype=F64, absolute=False):
    """The LoRA half of ur_rmsnorm_lora_fwd.  rms_lora_kernel packs h = w * (x * rstd) to bf16 (pack_bf2) ONCE, stores those bits as H and
    feeds the SAME packed registers (after drop_apply) to the MFMA as its column operand: t is the projection of the h BITS THE KERNEL WROTE,
    t[m, 16 a + j] = alpha * sum_c keep_a(m, c) h[m, c] A_a[j, c].  h_saved: the kernel's H output (held to the RMSNorm criterion first)."""
    return lora_project(h_saved, U, keep, alpha, None, dtype, absolute)


def swiglu_lora_t(act_saved, U, keep=None, alpha=1.0, dtype=F64, absolute=False):
    """The LoRA half of ur_swiglu_lora_fwd.  swiglu_lora_kernel packs act = silu(gate) * up to bf16 once, stores those bits as ACT and
    feeds the same registers (after drop_apply) to the MFMA: t[m, j] = alpha * sum_c keep(m, c) act[m, c] A[j, c] over the act BITS WRITTEN."""
    return lora_project(act_saved, [U], keep, alpha, None, dtype, absolute)


def assert_lora_bf16(got, ref64, ref32, abs_terms, what=""):
    """bf16 outputs t / tb / C.  EVERY element: |got - ref64| <= 1 bf16 ulp(ref64) + 2^-20 * abs_terms + 8 * |ref32 - ref64|, abs_terms =
    |alpha| sum |term| of that element (the accumulation term of assert_gemm_c / assert_colsum_close).  Returns the worst error / bound."""
    r, r32, a = _cpu64(ref64), _cpu64(ref32), _cpu64(abs_terms)
    assert r.shape == r32.shape == a.shape, f"{what}: shapes {tuple(r.shape)} / {tuple(r32.shape)} / {tuple(a.shape)}"
    assert torch.isfinite(r32).all(), f"{what}: the float32 re-evaluation of the reference is not finite"
    return assert_within_ulps(got, r, 1, 2.0 ** -20 * a + 8.0 * (r32 - r).abs(), what)


def assert_lora_exact(got, ref64, what=""):
    """The exact family: every element of `got` (bf16 or f32) carries the bits of the exact value rounded ONCE to its type.  The exact value
    zero has no sign (float64 torch returns -0.0 for a lone product -3 * 0; an accumulator that starts at +0 returns +0.0): both zeros are
    written +0 before the bits are compared.  Returns 0."""
    g = torch.as_tensor(got).detach().cpu()
    want = _cpu64(ref64).to(torch.float32).to(g.dtype)             # integers below 2^24 scaled by a power of two: exact in float32
    assert want.to(F64).ne(_cpu64(ref64)).sum() == 0 or g.dtype == torch.bfloat16, f"{what}: the exact value does not fit float32"
    g, want = torch.where(g == 0, torch.zeros_like(g), g), torch.where(want == 0, torch.zeros_like(want), want)
    assert g.shape == want.shape, f"{what}: shape {tuple(g.shape)} vs reference {tuple(want.shape)}"
    view = torch.int16 if g.dtype == torch.bfloat16 else torch.int32
    off = g.contiguous().view(view) != want.contiguous().view(view)
    if off.any():
        i = tuple(int(v) for v in off.nonzero()[0])
        raise AssertionError(f"{what}: {int(off.sum())} of {off.numel()} elements differ from the correctly rounded exact value; first at index {i}: "
                             f"got {g[i].item()!r}, exact {_cpu64(ref64)[i].item()!r} -> {want[i].item()!r}")
    return 0.0


LORA_MUTANTS = ("tail_chunk_skipped", "plane_of_block", "pair_order", "no_drop_scale", "row0_ignored", "half_rank_neighbour",
                "last_token_block_dropped", "col0_ignored")
_PAIR_ELEM = (0, 2, 4, 6, 1, 3, 5, 7)


def _acc32(parts, order):
    """f32 sum of a list of f32 tensors: 'chunks' = one after the other, 'tree' = pairwise"""
    parts = list(parts)
    if not parts:
        return None
    if order == "chunks":
        s = parts[0]
        for t in parts[1:]:
            s = s + t
        return s
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
    return parts[0]


def lora_mutant_applies(kind, c, mutant):
    """whether `mutant` changes what lora_emulated computes for launch `kind` of case c (a mutant that is invisible at a shape needs another)"""
    masked, cols = c.get("keep") is not None, c.get("cols")
    r, nad, M = c["rank"], c["nad"], c["M"]
    if mutant == "tail_chunk_skipped":
        return kind in ("project", "bgrad") and any(w % 128 for _, w in _lora_cols(c["X"], nad, cols))
    if mutant == "plane_of_block":
        return kind in ("project", "reduce", "epilogue") and masked and r >= 32 and nad >= 2
    if mutant == "pair_order":
        return masked
    if mutant == "no_drop_scale":
        return kind == "epilogue"
    if mutant == "row0_ignored":
        return masked and c["row0"] != 0
    if mutant == "half_rank_neighbour":
        return kind == "project" and masked and r == 8 and nad >= 2
    if mutant == "last_token_block_dropped":
        return kind != "epilogue" and M % 128 != 0
    if mutant == "col0_ignored":
        return kind in ("project", "reduce", "bgrad") and cols is not None and any(c0 for c0, _ in cols)
    raise AssertionError(mutant)


def lora_emulated(kind, c, order="chunks", mutant=None):
    """The kernels' arithmetic restated in float32 torch: exact bf16 x bf16 products, float32 partial sums over pieces of the reduction axis
    added in `order` ('chunks': pieces of 128 columns / tokens one after the other, the register-staged kernels' own order; 'tree': pieces of
    32 summed pairwise), ONE rounding to bf16 for t / tb / C.  kind: 'project' -> P; 'reduce' -> flattened G (c['transposed']); 'bgrad' ->
    (tb, dB); 'epilogue' -> C (c of lora_cases.epilogue_case).  Returns float64 tensors.
    mutant: one of LORA_MUTANTS -- a DELIBERATE bug, for tests/test_ref64.py to show that the criteria bite:
      tail_chunk_skipped        the columns past the last full 128 are ignored (project, tb of bgrad)
      plane_of_block            16-row block b of a rank-32 / 64 launch uses plane b (mod nad) instead of plane b / NB
      pair_order                flag bit i of a byte is applied to element c + i instead of c + 2 i (i < 4) / c + 2 (i - 4) + 1
      no_drop_scale             the masked epilogue adds keep * (tb A) without 1 / (1 - p)
      row0_ignored              the planes are drawn for rows 0 .. M - 1 instead of row0 ..
      half_rank_neighbour       rank 8: the upper half of adapter a's block is not zero but live, and its 16-wide result lands on adapter
                                a + 1's columns -- adapter a + 1's t is computed under plane a
      last_token_block_dropped  the rows of the last, partly filled 128-token block are not computed (row outputs stay 0, sums lose them)
      col0_ignored              an adapter's column range starts at column 0"""
    assert mutant is None or mutant in LORA_MUTANTS, mutant
    assert order in ("chunks", "tree")
    f32 = torch.float32
    step = 128 if order == "chunks" else 32
    rank, nad, M = c["rank"], c["nad"], c["M"]
    keep = c.get("keep")
    if keep is not None:
        if mutant == "row0_ignored":
            import numpy as np
            from oracle import dropout_ref
            keep = torch.from_numpy(dropout_ref.lora_keep(c["seed"], c["p"], M, keep.shape[-1], nad, 0).astype(np.float64))
        if mutant == "pair_order":
            W_ = keep.shape[-1]
            idx = torch.arange(W_)
            keep = keep[..., (idx // 8) * 8 + torch.tensor(_PAIR_ELEM)[idx % 8]]
        keep = keep.to(f32)
    mlive = M if mutant != "last_token_block_dropped" else (M // 128) * 128

    def plane(a, nb):
        if keep is None:
            return None
        if mutant == "plane_of_block":
            return keep[(a * (rank // 16) + nb) % nad]
        if mutant == "half_rank_neighbour" and a > 0:
            return keep[a - 1]
        return keep[a]

    def blocks(a):             # (first rank row, rows, plane) of adapter a's 16-row blocks (one 8-row block at rank 8)
        return [(16 * nb, min(16, rank), plane(a, nb)) for nb in range(max(1, rank // 16))]

    def xcols(X, a, cols_):
        c0, w = _lora_cols(X, nad, cols_)[a]
        if mutant == "col0_ignored":
            c0 = 0
        return X.detach().cpu()[:, c0:c0 + w].to(f32), w

    def project(X, U, alpha, cols_):
        out = torch.zeros(M, rank * nad, dtype=f32)
        for a in range(nad):
            xa, w = xcols(X, a, cols_)
            wl = (w // 128) * 128 if mutant == "tail_chunk_skipped" else w
            for j0, nj, kp in blocks(a):
                xm = xa if kp is None else xa * kp
                u = U[a].detach().cpu().to(f32)[j0:j0 + nj]
                s = _acc32([xm[:, k:min(k + step, wl)] @ u[:, k:min(k + step, wl)].t() for k in range(0, wl, step)], order)
                if s is not None:
                    out[:mlive, rank * a + j0:rank * a + j0 + nj] = (s * torch.tensor(alpha, dtype=f32))[:mlive]
        return _bf(out).to(F64)

    def reduce(X, V, alpha, cols_, transposed):
        v = V.detach().cpu().to(f32)
        outs = []
        for a in range(nad):
            xa, w = xcols(X, a, cols_)
            g = torch.zeros(rank, w, dtype=f32)
            for j0, nj, kp in blocks(a):
                xm = xa if kp is None else xa * kp
                va = v[:, rank * a + j0:rank * a + j0 + nj]
                s = _acc32([va[t0:min(t0 + step, mlive)].t() @ xm[t0:min(t0 + step, mlive)] for t0 in range(0, mlive, step)], order)
                if s is not None:
                    g[j0:j0 + nj] = s * torch.tensor(alpha, dtype=f32)
            outs.append((g.t() if transposed else g).reshape(-1))
        return torch.cat(outs).to(F64)

    if kind == "project":
        return project(c["X"], c["U"], c["alpha"], c["cols"])
    if kind == "reduce":
        return reduce(c["X"], c["V"], c["alpha"], c["cols"], bool(c.get("transposed", c["cols"] is not None)))
    if kind == "bgrad":
        return project(c["X"], c["U"], c["alpha"], c["cols"]), reduce(c["X"], c["V"], 1.0, c["cols"], True)
    assert kind == "epilogue", kind
    R, S, tb, A = (c[k].detach().cpu().to(f32) for k in ("R", "S", "tb", "A"))
    K = R.shape[1]
    acc = _acc32([R[:, k:k + step] @ S[:, k:k + step].t() for k in range(0, K, step)], order)
    inv = torch.tensor(1.0, dtype=f32) if mutant == "no_drop_scale" else torch.tensor(1.0, dtype=f32) / torch.tensor(1.0 - c["p"], dtype=f32)
    for a in range(nad):
        for j0, nj, kp in blocks(a):
            sl = slice(rank * a + j0, rank * a + j0 + nj)
            acc = acc + kp * ((tb[:, sl] @ A[sl]) * inv)
    return _bf(acc).to(F64)


# ---- the decoder's fused GEMM epilogues (csrc/gemm_pers.hip EPI 3 / 4 / 1, gemm_body.hip.h EPI 1 / 2; ur_gemm_args.qkr_*, swp_*, swiglu_*) ---
# Device-agnostic: these run on whatever device their inputs live on (the GPU tests keep 8 .. 35 M element outputs there); every
# product acc is given in the NATURAL feature order (the paired weight-row order of the launches is the tests' business).
def ulp_ratio(got, ref64, ulps=1, floor=0.0):
    """(worst |got - ref| / (ulps * bf16_ulp(ref) + floor), number of elements above 1, number of non-finite outputs) without leaving the
    inputs' device -- assert_within_ulps' criterion for outputs too large to walk on the CPU.  0 / 0 counts as 0."""
    g, r = got.to(F64), ref64.to(F64)
    assert g.shape == r.shape, f"shape {tuple(g.shape)} vs reference {tuple(r.shape)}"
    assert torch.isfinite(r).all(), "the reference itself is not finite"
    err = (g - r).abs()
    bound = ulps * bf16_ulp(r) + torch.as_tensor(floor, dtype=F64, device=r.device)
    bad = ~torch.isfinite(g)
    ratio = torch.where(bad | (err == 0), torch.zeros_like(err), err / bound)
    return float(ratio.max()) if ratio.numel() else 0.0, int((ratio > 1.0).sum()), int(bad.sum())


def assert_ulp_ratio(got, ref64, ulps=1, floor=0.0, what=""):
    """assert_within_ulps on the inputs' device: EVERY element finite and within ulps * bf16_ulp(ref) + floor.  Returns the worst ratio."""
    worst, off, bad = ulp_ratio(got, ref64, ulps, floor)
    assert bad == 0, f"{what}: {bad} non-finite outputs"
    if off:
        g, r = got.to(F64), ref64.to(F64)
        exc = ((g - r).abs() / (ulps * bf16_ulp(r) + torch.as_tensor(floor, dtype=F64, device=r.device)))
        i = tuple(int(v) for v in torch.unravel_index(exc.argmax(), exc.shape))
        raise AssertionError(f"{what}: {off} of {g.numel()} elements exceed {ulps} bf16 ulp + floor; worst at index {i}: got {g[i].item()!r}, "
                             f"reference {r[i].item()!r}, error {abs(g[i].item() - r[i].item()):.3e} = {worst:.2f} x the bound")
    return worst


def rope_table_f32(S, head_dim, theta):
    """The table as ur_rope_table forms it (qwen_ops.hip): inv_freq and the ANGLE pos * inv_freq in float32, cos / sin of that float32 angle
    correctly rounded.  The angle's rounding (half an ulp of up to 4095 rad: 1.2e-4) is what makes table row p + 16 differ from table
    row p advanced by table row 16."""
    f32 = torch.float32
    half = head_dim // 2
    inv = 1.0 / torch.pow(torch.tensor(theta, dtype=f32), (2 * torch.arange(half)).to(f32) / float(2 * half))
    ang = (torch.arange(S).to(f32)[:, None] * inv[None, :]).to(F64)
    return torch.cos(ang).to(f32), torch.sin(ang).to(f32)


def qkrope_epilogue(acc, qw, kw, cos_tab, sin_tab, S, nq_cols, nk_cols, eps, dtype=F64):
    """q/k-norm + RoPE as the epilogue of the merged q|k|v launch (ur_gemm_args.qkr_*; Qwen3Attention): acc [M, N] = the product, columns
    q heads | k heads | v in natural feature order, 128-wide heads, token m at position m % S.  Per head rstd = 1 / sqrt(mean(acc^2) + eps),
    x = acc * rstd * w, rotate-half RoPE with the table rows AS GIVEN (qknorm_rope_fwd's formula); v = the plain projection.
    Returns (q_r [M, nq_cols], k_r [M, nk_cols], v [M, N - nq_cols - nk_cols], rstd [M, (nq_cols + nk_cols) / 128])."""
    hd = 128
    nq, nk = nq_cols // hd, nk_cols // hd
    M = acc.shape[0]
    a = acc.to(dtype)
    x = a[:, :nq_cols + nk_cols].reshape(M, nq + nk, hd)
    rstd = torch.rsqrt((x * x).mean(-1) + eps)
    out = qknorm_rope_fwd(a, qw, kw, cos_tab, sin_tab, S, nq, nk, hd, eps, dtype).reshape(M, nq_cols + nk_cols)
    return out[:, :nq_cols], out[:, nq_cols:], a[:, nq_cols + nk_cols:], rstd


def swiglu_bwd_epilogue(dact64, gate, up):
    """SwiGLU backward as the epilogue of the down-projection's dX launch (swiglu_bwd=): swiglu_bwd on the UNROUNDED d(act) -- the
    epilogue keeps the product in f32 and never rounds it to bf16, which the stand-alone kernel's input is.  (dgate, dup)."""
    return swiglu_bwd(dact64.to(F64), gate, up)


def _bf16_of_exact(acc):
    """bf16 of a product that float32 holds exactly (|acc| < 2^24 integers): ONE rounding"""
    a32 = acc.to(torch.float32)
    assert bool((a32.to(F64) == acc.to(F64)).all()), "the product is not exact in float32: bf16 through float32 would round twice"
    return a32.to(torch.bfloat16)


def swiglu_fwd_epilogue(acc_gate_up):
    """SwiGLU forward as the epilogue of the merged gate|up launch (swiglu_paired=) and of the up projection (swiglu_fwd=): acc [M, 2 I] =
    the exact product, gate | up.  Returns (gu = bf16(acc) -- what the launch stores for the backward --, act = silu(gate BITS) * (up
    BITS) in float64)."""
    gu = _bf16_of_exact(acc_gate_up)
    I = gu.shape[1] // 2
    return gu, swiglu_fwd(gu[:, :I], gu[:, I:])


GEMM_EPI_MUTANTS = ("pos_not_wrapped", "step80_as_16", "rstd_neighbour_head", "k_weight_on_q", "eps_dropped", "partner_sign",
                    "dgate_from_rounded_dact", "dup_uses_sigmoid_only", "gate_up_halves_swapped", "masked_term_unscaled")


def qkrope_emulated(acc, qw, kw, cos_tab, sin_tab, S, nq_cols, nk_cols, eps, mutant=None, recurrence=True, rounded=True):
    """EPI 3 of csrc/gemm_pers.hip in float32 torch, outputs rounded to bf16 (rstd stays f32): the same four outputs as qkrope_epilogue, in
    float64.  Per 256-row tile and row-in-16 l15 the kernel loads ONE table row per wave group wr (position pos0 + 64 wr + l15, pos0 =
    m0 % S) and advances cos / sin by the angle-addition theorem with table rows 16 and 80: + 16 three times, + 80 (from row block 3 of
    the first row half to block 0 of the second), + 16 three times.  rstd = f32 rsqrt(sum / 128 + eps), x = (acc * rstd) * w,
    o = xa c - xb s | xb c + xa s.  recurrence=False reads every row's own table row instead (what the stand-alone kernel does);
    rounded=False returns q_r / k_r BEFORE the rounding to bf16 (the e32 yardstick of qkrope_bound: what float32 costs, not what bf16 does).
    mutant (DELIBERATE bugs, tests/test_ref64.py): pos_not_wrapped (pos0 = m0: the tables must then have M rows), step80_as_16,
    rstd_neighbour_head (the two heads of a 256-column tile swap their row constants), k_weight_on_q, eps_dropped, partner_sign."""
    assert mutant in (None, "pos_not_wrapped", "step80_as_16", "rstd_neighbour_head", "k_weight_on_q", "eps_dropped", "partner_sign"), mutant
    f32 = torch.float32
    hd = 128
    nh = (nq_cols + nk_cols) // hd
    nq = nq_cols // hd
    M = acc.shape[0]
    assert M % 256 == 0 and S % 256 == 0 and nq_cols % 256 == 0 and nk_cols % 256 == 0
    dev = acc.device
    a = acc.to(f32)
    x = a[:, :nq_cols + nk_cols].reshape(M, nh, hd)
    ct, st = cos_tab.to(f32), sin_tab.to(f32)
    # ---- cos / sin of every row, as the kernel gets them
    m = torch.arange(M, device=dev)
    m0 = (m // 256) * 256
    pos0 = m0 if mutant == "pos_not_wrapped" else m0 % S
    r = m % 256
    if recurrence:
        wr, l15, j = (r >> 6) & 1, r & 15, (r >> 7) * 4 + ((r >> 4) & 3)
        base = pos0 + wr * 64 + l15
        c, s = ct[base], st[base]                                   # [M, 64]: the row the lane loaded
        for step in range(7):
            t = 16 if (step != 3 or mutant == "step80_as_16") else 80
            dc, ds = ct[t][None, :], st[t][None, :]
            cn, sn = c * dc - s * ds, s * dc + c * ds
            live = (j > step)[:, None]
            c, s = torch.where(live, cn, c), torch.where(live, sn, s)
    else:
        c, s = ct[pos0 + r], st[pos0 + r]
    # ---- row constants
    ss = (x * x).sum(-1)
    rs = torch.rsqrt(ss * torch.tensor(1.0 / 128.0, dtype=f32) + (0.0 if mutant == "eps_dropped" else torch.tensor(eps, dtype=f32)))
    rs_used = rs.reshape(M, nh // 2, 2).flip(-1).reshape(M, nh) if mutant == "rstd_neighbour_head" else rs
    w = torch.cat([(kw if mutant == "k_weight_on_q" else qw).to(f32)[None].expand(nq, -1), kw.to(f32)[None].expand(nh - nq, -1)], 0)
    xn = (x * rs_used[..., None]) * w[None]
    xa, xb = xn[..., :64], xn[..., 64:]
    c, s = c[:, None, :], s[:, None, :]
    o0 = xa * c - xb * s
    o1 = (xb * c - xa * s) if mutant == "partner_sign" else (xb * c + xa * s)
    out = torch.cat([o0, o1], -1)
    out = (_bf(out) if rounded else out).to(F64).reshape(M, nq_cols + nk_cols)
    return out[:, :nq_cols], out[:, nq_cols:], _bf(a[:, nq_cols + nk_cols:]).to(F64), rs_used.to(F64)


def _sigmoid32(g):
    return 1.0 / (1.0 + torch.exp(-g))


def swiglu_bwd_epilogue_emulated(acc, gate, up, masked=None, mutant=None):
    """EPI 1 (both GEMM kernels) in float32 torch: d = acc (+ keep / (1 - p) * (tb A), masked = (tb, A [r, N], keep [M, N], p)) stays f32;
    dgate = d u (s (1 + g (1 - s))), dup = d (g s), each rounded once to bf16.  Returns (dgate, dup) in float64.
    mutant: dgate_from_rounded_dact (d is rounded to bf16 first: the two-kernel path, a LEGITIMATE result), dup_uses_sigmoid_only
    (dup = d s), gate_up_halves_swapped (the gate is read from the up half and the up from the gate half), masked_term_unscaled (the
    1 / (1 - p) factor is lost)."""
    assert mutant in (None, "dgate_from_rounded_dact", "dup_uses_sigmoid_only", "gate_up_halves_swapped", "masked_term_unscaled"), mutant
    f32 = torch.float32
    d = acc.to(f32)
    if masked is not None:
        tb, A, keep, p = masked
        inv = torch.tensor(1.0, dtype=f32) if mutant == "masked_term_unscaled" else torch.tensor(1.0, dtype=f32) / torch.tensor(1.0 - p, dtype=f32)
        d = d + keep.to(f32) * ((tb.to(f32) @ A.to(f32)) * inv)
    if mutant == "dgate_from_rounded_dact":
        d = _bf(d).to(f32)
    g, u = gate.to(f32), up.to(f32)
    if mutant == "gate_up_halves_swapped":
        g, u = u, g
    sg = _sigmoid32(g)
    dup = d * sg if mutant == "dup_uses_sigmoid_only" else d * (g * sg)
    dgate = d * u * (sg * (1.0 + g * (1.0 - sg)))
    return _bf(dgate).to(F64), _bf(dup).to(F64)


def swiglu_fwd_epilogue_emulated(acc_gate_up, mutant=None):
    """EPI 4 / the generic swiglu_fwd= epilogue in float32 torch: gu = bf16(acc), act = bf16(silu(gate bits) * up bits).  (gu bf16, act
    float64).  mutant: gate_up_halves_swapped (act = silu(up) * gate)."""
    assert mutant in (None, "gate_up_halves_swapped"), mutant
    f32 = torch.float32
    gu = acc_gate_up.to(f32).to(torch.bfloat16)
    I = gu.shape[1] // 2
    g, u = gu[:, :I].to(f32), gu[:, I:].to(f32)
    if mutant == "gate_up_halves_swapped":
        g, u = u, g
    return gu, _bf((g * _sigmoid32(g)) * u).to(F64)


def qkrope_bound(ref64, emul=None):
    """The floor of the EPI 3 criterion beside 1 bf16 ulp: 2^-18 * row max |ref| per HEAD row (the stand-alone kernel's bound), + 8 *
    e32_row where an emulation is given, e32_row = the head row's max |emulation - ref64| -- what the float32 recipe, its angle recurrence
    over the FLOAT32 table included, costs on this input (tests/test_ref64.py: test_margins_beyond_one_ulp_are_what_float32_costs).
    ref64 [M, heads * 128] -> floor of the same shape."""
    M = ref64.shape[0]
    r = ref64.to(F64).reshape(M, -1, 128)
    fl = 2.0 ** -18 * r.abs().amax(-1, keepdim=True)
    if emul is not None:
        fl = fl + 8.0 * (emul.to(F64).reshape(M, -1, 128) - r).abs().amax(-1, keepdim=True)
    return fl.expand_as(r).reshape(M, -1)


# ---- AdamW, casts, bf16 add, field projection, split-K token reductions (include/unirec_hip.h: ur_adamw_step*, ur_cast_*, ur_add_bf16,
# ur_field_projection_*, ur_gemm / ur_gemm_grouped with split_k) ---------------------------------------------------------------------
ADAMW_MUTANTS = ("bias_correction_step_minus_1", "l2_decay_in_gradient", "eps_inside_sqrt", "grad_scale_not_on_v", "tail_unstepped")
FPROJ_MUTANTS = ("bias_per_q", "position_skipped", "w_transposed")
SPLITK_MUTANTS = ("slice_dropped", "slice_twice")
GEMM_BK = 64                        # K depth of one tile of csrc/gemm.hip: ur_gemm cuts K into split_k runs of ceil(tiles / split_k) tiles


def _f32_scalar(x, dtype):
    """a `float` argument of the ABI: the float32 value the kernel receives, in the evaluation's dtype"""
    return torch.tensor(float(x), dtype=torch.float32).to(dtype)


def adamw_step(p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale, coef=1.0, dtype=F64, mutant=None):
    """torch.optim.AdamW's step (decoupled decay) as the header states it, on flat vectors; returns (p, m, v):
        gr = g * (grad_scale * coef);  p *= 1 - lr * wd;  m = b1 m + (1 - b1) gr;  v = b2 v + (1 - b2) gr^2;
        p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps).
    The hyperparameters enter as the float32 values the ABI passes.  mutant: one of ADAMW_MUTANTS, a DELIBERATE bug."""
    assert mutant is None or mutant in ADAMW_MUTANTS, mutant
    c = lambda t: torch.as_tensor(t).detach().cpu().to(dtype).reshape(-1)      # noqa: E731
    p0, g0, m0, v0 = c(p), c(g), c(m), c(v)
    lr_, b1_, b2_, eps_, wd_ = (_f32_scalar(x, dtype) for x in (lr, b1, b2, eps, wd))
    gs = _f32_scalar(grad_scale, dtype) * _f32_scalar(coef, dtype)
    one = torch.ones((), dtype=dtype)
    t = float(step - 1 if mutant == "bias_correction_step_minus_1" else step)
    bc1, bc2 = one - b1_ ** t, one - b2_ ** t
    gr = g0 * gs
    if mutant == "l2_decay_in_gradient":
        gr = gr + wd_ * p0
        pn = p0
    else:
        pn = p0 * (one - lr_ * wd_)
    mn = b1_ * m0 + (one - b1_) * gr
    gv = g0 if mutant == "grad_scale_not_on_v" else gr
    vn = b2_ * v0 + (one - b2_) * gv * gv
    if mutant == "eps_inside_sqrt":
        denom = torch.sqrt(vn / bc2 + eps_)
    else:
        denom = torch.sqrt(vn) / torch.sqrt(bc2) + eps_
    pn = pn - (lr_ / bc1) * (mn / denom)
    if mutant == "tail_unstepped":
        k = (p0.numel() // 4) * 4
        pn[k:], mn[k:], vn[k:] = p0[k:], m0[k:], v0[k:]
    return pn, mn, vn


def rows_of(t, width=64):
    """a flat vector as rows of `width` elements (zero-padded): the rows of assert_f32_close, so that one large element sets the bound of its
    own 64 neighbours only"""
    t = torch.as_tensor(t).detach().cpu().reshape(-1)
    pad = (-t.numel()) % width
    if pad:
        t = torch.cat([t, torch.zeros(pad, dtype=t.dtype)])
    return t.reshape(-1, width)


def cast_f32_to_bf16(x):
    """torch's own CPU conversion (round to nearest even; NaN stays NaN, overflow gives the signed infinity)"""
    return torch.as_tensor(x).detach().cpu().to(torch.float32).to(torch.bfloat16)


def assert_bf16_bits(got, want, what=""):
    """bf16 `got` carries the bits of `want`, except that every NaN equals every NaN (the payload is not specified).  Returns 0."""
    g, w = torch.as_tensor(got).detach().cpu(), torch.as_tensor(want).detach().cpu()
    assert g.dtype == w.dtype == torch.bfloat16 and g.shape == w.shape, f"{what}: {g.dtype} {tuple(g.shape)} vs {w.dtype} {tuple(w.shape)}"
    gn, wn = torch.isnan(g), torch.isnan(w)
    off = (gn != wn) | (~gn & (g.contiguous().view(torch.int16) != w.contiguous().view(torch.int16)))
    if off.any():
        i = tuple(int(v) for v in off.nonzero()[0])
        raise AssertionError(f"{what}: {int(off.sum())} of {off.numel()} elements differ; first at index {i}: got {g[i].item()!r} "
                             f"(0x{int(g.contiguous().view(torch.int16)[i]) & 0xffff:04x}), expected {w[i].item()!r} (0x{int(w.contiguous().view(torch.int16)[i]) & 0xffff:04x})")
    return 0.0


def add_bf16(a, b):
    """(bf16(float32(a) + float32(b)) -- the kernel's documented rounding: the float32 sum of two bf16 values, rounded once more --, the
    float64 sum)"""
    a, b = torch.as_tensor(a).detach().cpu(), torch.as_tensor(b).detach().cpu()
    return (a.to(torch.float32) + b.to(torch.float32)).to(torch.bfloat16), a.to(F64) + b.to(F64)


def field_projection_fwd(rec, Wf, bf, dtype=F64, mutant=None):
    """out[b, f, e] = sum_q Wf[f, q] rec[b, q, e] + bf[f]: [B, F, E]."""
    assert mutant is None or mutant in FPROJ_MUTANTS, mutant
    r, w, b = (torch.as_tensor(t).detach().cpu().to(dtype) for t in (rec, Wf, bf))
    if mutant == "w_transposed":                                 # the F * Q words read as [Q, F]
        w = w.reshape(-1).reshape(w.shape[1], w.shape[0]).t()
    out = torch.einsum("fq,bqe->bfe", w, r)
    return out + b[None, :, None] * (w.shape[1] if mutant == "bias_per_q" else 1)


def field_projection_bwd(dout, rec, Wf, dtype=F64, mutant=None):
    """(drec [B, Q, E] = sum_f Wf[f, q] dout[b, f, e];  dWf [F, Q] = sum_{b, e} dout[b, f, e] rec[b, q, e];  dbf [F] = sum_{b, e} dout[b, f, e];
    sum |dout * rec| [F, Q];  sum |dout| [F]) -- the last two are the abs_terms of assert_colsum_close."""
    assert mutant is None or mutant in FPROJ_MUTANTS, mutant
    d, r, w = (torch.as_tensor(t).detach().cpu().to(dtype) for t in (dout, rec, Wf))
    wd = w.reshape(-1).reshape(w.shape[1], w.shape[0]).t() if mutant == "w_transposed" else w
    drec = torch.einsum("fq,bfe->bqe", wd, d)
    dk = d
    if mutant == "position_skipped":                             # the last (b, e) position never reaches the weight gradient
        dk = d.clone()
        dk[-1, :, -1] = 0
    dWf = torch.einsum("bfe,bqe->fq", dk, r)
    return drec, dWf, d.sum(dim=(0, 2)), torch.einsum("bfe,bqe->fq", d.abs(), r.abs()), d.abs().sum(dim=(0, 2))


FPROJ_OPERAND_ROUNDING = 2.0 ** -9  # fproj_bwd32_kernel rounds dout to bf16 (half a unit of 8 significant bits) in front of the MFMA


def fproj_fast_dwf_terms(abs_terms):
    """abs_terms of assert_colsum_close for the Q = 32 fast path's dWf: the bound 8 e32 + 2^-20 sum |term| + 2^-9 sum |term|, the last
    for the bf16 rounding of the dout operand, written as one sum |term| scaled by 1 + 2^11 (as assert_lora_bf16 passes its own)."""
    return _cpu64(abs_terms) * (1.0 + FPROJ_OPERAND_ROUNDING * 2.0 ** 20)


def splitk_slices(K, split_k, bk=GEMM_BK):
    """[(k0, k1)] of the split_k runs ur_gemm / ur_gemm_grouped cut the token axis into: ceil(ceil(K / bk) / split_k) tiles each; trailing
    runs may be short or EMPTY (k0 >= k1)."""
    per = -(-(-(-K // bk)) // max(1, split_k)) * bk
    return [(min(K, z * per), min(K, (z + 1) * per)) for z in range(max(1, split_k))]


def gemm_tn(R, S, split_k=1, dtype=F64, mutant=None):
    """Token-major product out[m, n] = sum_k R[k, m] S[k, n] (dW = dY^T X), summed run by run as the split-K slabs are; R [K, M], S [K, N]."""
    assert mutant is None or mutant in SPLITK_MUTANTS, mutant
    r, s = torch.as_tensor(R).detach().cpu().to(dtype), torch.as_tensor(S).detach().cpu().to(dtype)
    runs = [(k0, k1) for k0, k1 in splitk_slices(r.shape[0], split_k) if k1 > k0]
    if mutant == "slice_dropped":
        runs = runs[:-1]
    if mutant == "slice_twice":
        runs = runs + runs[:1]
    out = torch.zeros(r.shape[1], s.shape[1], dtype=dtype)
    for k0, k1 in runs:
        out = out + r[k0:k1].t() @ s[k0:k1]
    return out


def assert_adamw_close(got, p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale, coef=1.0, coef32=None, what=""):
    """got = (p, m, v) after one step, each held by assert_f32_close in rows of 64 against adamw_step in float64, with the same formula in
    float32 as the yardstick (coef32: the float32 evaluation's own clip coefficient where the coefficient is itself computed).  Returns the
    worst error / bound of the three."""
    r64 = adamw_step(p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale, coef)
    r32 = adamw_step(p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale, coef if coef32 is None else coef32, dtype=torch.float32)
    worst = 0.0
    for name, x, a, b in zip(("param", "exp_avg", "exp_avg_sq"), got, r64, r32):
        assert torch.as_tensor(x).numel() == a.numel(), f"{what}: {name}: {torch.as_tensor(x).numel()} elements vs {a.numel()}"
        worst = max(worst, assert_f32_close(rows_of(x), rows_of(a), rows_of(b), what=f"{what}: {name}"))
    return worst

"""The inputs of tests/test_gpu_attention_f64.py and what they are held to, as plain CPU code: the GPU module runs the kernels on
these cases, tests/test_ref64.py checks on the CPU that the emulation meets the hard bound on every one of them.  No device execution;
asks the built library which kernels a shape takes (hip.attn_plan).

A case is a dict (see case()); inputs() builds its seeded bf16 tensors, reference() the float64 results, criteria() the bound magnitudes
A and the emulation, hold() applies both criteria and the stats check to what a kernel returned."""
import contextlib
import functools
import zlib

import torch

from oracle import dropout_ref
from tests import ref64
from unirec_amd import _lib, hip

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
HEADS = ((1, 1), (3, 3), (4, 2), (4, 1))              # (nq, nkv): GQA ratios 1, 1, 2, 4


def case(name, B, Sq, Sk, nq, nkv, hd, causal, mask="none", p=0.0, dseed=0, drop_batch0=0, values="randn", scale=None, modes=()):
    """mask: "none" | "rand" (70 % kept, key 0 kept) | "full" (rand + one fully masked sample) | "left" (left padding of 3 b + 1 keys) |
    "ragged" (a valid prefix per sample, one fully masked sample when B > 1) | a tuple of per-sample specs ("none",) / ("pad", n) / ("hole", key).
    values: "randn" | "std4" (q, k at std 4: near one-hot) | "equal_keys" (exactly uniform) | "dout0" | "v0".
    modes: ((mode name, value), ...) for ur_attn_mode, e.g. (("C128", 0),)."""
    return dict(name=name, B=B, Sq=Sq, Sk=Sk, nq=nq, nkv=nkv, hd=hd, causal=bool(causal), mask=mask, p=float(p), dseed=int(dseed),
                drop_batch0=int(drop_batch0), values=values, scale=float(scale if scale is not None else hd ** -0.5), modes=tuple(modes))


def _input_key(c):
    return tuple((k, c[k]) for k in sorted(c) if k not in ("name", "modes"))


MODE_KEYS = {"TINY": hip.ATTN_MODE_TINY, "C128": hip.ATTN_MODE_C128, "DKV_PERSIST": hip.ATTN_MODE_DKV_PERSIST, "FEWQ": hip.ATTN_MODE_FEWQ}


def plan_args(B, Sq, Sk, nq, nkv, hd, causal, p=0.0, scale=None):
    """(AttnArgs, AttnBwdArgs) of a dense call as far as hip.attn_plan reads them: sizes, strides and flags, no pointer"""
    a, g = _lib.AttnArgs(), _lib.AttnBwdArgs()
    a.B, a.Sq, a.Sk, a.nq, a.nkv, a.head_dim, a.causal = B, Sq, Sk, nq, nkv, hd, int(causal)
    a.ldq = a.ldo = g.lddo = g.lddq = nq * hd
    a.ldk = a.ldv = g.lddk = g.lddv = nkv * hd
    a.scale, a.dropout_p = float(scale if scale is not None else hd ** -0.5), float(p)
    return a, g


@contextlib.contextmanager
def plan_modes(modes):
    """the ur_attn_mode words ((mode name, value), ...) set, every other word as it stands; all restored on exit"""
    with contextlib.ExitStack() as st:
        for k, v in modes:
            st.enter_context(hip.attn_mode_set(MODE_KEYS[k], v))
        yield


def plan_of(a, g=None, modes=()):
    """hip.attn_plan under the ur_attn_mode words `modes`"""
    with plan_modes(modes):
        return hip.attn_plan(a, g)


def plan(c):
    """the kernels case c takes under its own modes"""
    return plan_of(*plan_args(c["B"], c["Sq"], c["Sk"], c["nq"], c["nkv"], c["hd"], c["causal"], c["p"], c["scale"]), modes=c["modes"])


def _qk_round_of(pl):
    """Which launches run on the generated causal head_dim-128 kernels, i.e. round q * scale * log2 e (k * scale * log2 e in dK/dV) to
    bf16 once more: None, "fwd" (forward only) or "all" (the backward pair as well)."""
    if pl["fwd"] != "c128":
        assert pl["dq"] != "c128" and pl["dkv"] != "c128", pl
        return None
    return "all" if pl["dq"] == "c128" else "fwd"


def qk_round_for(hd, causal, Sq, Sk, c128_mode=None, B=1, nq=1, nkv=1):
    """_qk_round_of what the library selects for a dense call of this shape; c128_mode None: UR_ATTN_MODE_C128 as it stands"""
    return _qk_round_of(plan_of(*plan_args(B, Sq, Sk, nq, nkv, hd, causal), modes=() if c128_mode is None else (("C128", c128_mode),)))


def qk_round(c):
    return _qk_round_of(plan(c))


def _mask(c, g):
    B, Sk, m = c["B"], c["Sk"], c["mask"]
    if m == "none":
        return None
    km = torch.ones((B, Sk), dtype=torch.uint8)
    if isinstance(m, tuple):
        for b in range(B):
            spec = m[b % len(m)]
            if spec[0] == "pad":
                km[b, :min(spec[1], Sk)] = 0
            elif spec[0] == "hole":
                km[b, spec[1]] = 0
        return km
    if m in ("rand", "full"):
        km = (torch.rand((B, Sk), generator=g) < 0.7).to(torch.uint8)
        km[:, 0] = 1
        if m == "full":
            km[min(1, B - 1)] = 0
    elif m == "left":
        for b in range(1, B):
            km[b, :min(Sk - 1, 3 * b + 1)] = 0
    elif m == "ragged":
        lens = torch.randint(max(1, Sk // 2), Sk + 1, (B,), generator=g)
        km = (torch.arange(Sk)[None, :] < lens[:, None]).to(torch.uint8)
        if B > 1:
            km[1] = 0
    else:
        raise ValueError(m)
    return km


@functools.lru_cache(maxsize=8)
def _inputs(key):
    c = dict(key)
    g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    B, Sq, Sk, nq, nkv, hd = c["B"], c["Sq"], c["Sk"], c["nq"], c["nkv"], c["hd"]
    std = 4.0 if c["values"] == "std4" else 1.0
    q = (torch.randn((B, Sq, nq, hd), generator=g) * std).to(BF16)
    k = (torch.randn((B, Sk, nkv, hd), generator=g) * std).to(BF16)
    v = torch.randn((B, Sk, nkv, hd), generator=g).to(BF16)
    dout = torch.randn((B, Sq, nq, hd), generator=g).to(BF16)
    if c["values"] == "equal_keys":
        k = k[:, :1].expand(B, Sk, nkv, hd).contiguous()
    if c["values"] == "dout0":
        dout = torch.zeros_like(dout)
    if c["values"] == "v0":
        v = torch.zeros_like(v)
    km = _mask(c, g)
    keep = None
    if c["p"] > 0:
        keep = torch.from_numpy(dropout_ref.attn_keep(c["dseed"], c["p"], B, nq, Sq, Sk, c["drop_batch0"]))
    return dict(q=q, k=k, v=v, dout=dout, key_mask=km, keep=keep)


def inputs(c):
    """q, k, v, dout (bf16, CPU), key_mask (uint8 [B, Sk] or None), keep (uint8 [B, nq, Sq, Sk] from oracle/dropout_ref.attn_keep, or None)"""
    return _inputs(_input_key(c))


def reference_of(q, k, v, dout, key_mask, causal, scale, keep=None, p=0.0):
    """float64 from the exact bf16 values: o, lse, lse32 (the same formula in float32), live, dq, dk, dv"""
    o, _, lse = ref64.attention_fwd(q, k, v, key_mask, causal, scale, keep, p)
    lse32 = ref64.attention_fwd(q, k, v, key_mask, causal, scale, keep, p, dtype=F32)[2]
    dq, dk, dv = ref64.attention_bwd(q, k, v, key_mask, causal, scale, dout, keep, p)
    live = ref64.attention_allowed(key_mask, causal, q.shape[0], q.shape[1], k.shape[1])[1].expand(lse.shape)
    return dict(o=o, lse=lse, lse32=lse32, live=live, dq=dq, dk=dk, dv=dv)


def criteria_of(q, k, v, dout, key_mask, causal, scale, keep=None, p=0.0, qk_round=None):
    """(A: the bound magnitudes, emul: the emulation's o, dq, dk, dv)"""
    A = ref64.attention_bounds(q, k, v, key_mask, causal, scale, dout, keep, p, qk_rounded=qk_round is not None)
    e = ref64.attention_emulated(q, k, v, key_mask, causal, scale, dout, keep, p, qk_round=qk_round)
    return A, dict(zip(("o", "dq", "dk", "dv"), e))


@functools.lru_cache(maxsize=4)
def _reference(key):
    c, x = dict(key), _inputs(key)
    return reference_of(x["q"], x["k"], x["v"], x["dout"], x["key_mask"], c["causal"], c["scale"], x["keep"], c["p"])


@functools.lru_cache(maxsize=4)
def _criteria(key, qkr):
    c, x = dict(key), _inputs(key)
    return criteria_of(x["q"], x["k"], x["v"], x["dout"], x["key_mask"], c["causal"], c["scale"], x["keep"], c["p"], qkr)


def reference(c):
    return _reference(_input_key(c))


def criteria(c):
    return _criteria(_input_key(c), qk_round(c))


def hold(ref, A, emul, got, what, stats=None):
    """Both criteria on every output in `got` (a dict with any of o, dq, dk, dv -- tensors of the ABI layout, any device) and, with stats
    [B, nq, Sq, 2] = (m, 1 / l), the check of m + ln l against the float64 lse.  Returns {"<output> bound" / "<output> frob" / "lse": worst ratio}."""
    out = {}
    for n in ("o", "dq", "dk", "dv"):
        if n in got:
            out[n + " bound"] = ref64.assert_attn_bound(got[n], ref[n], A[n], f"{what} {n}")
            out[n + " frob"] = ref64.assert_attn_frob(got[n], ref[n], emul[n], A[n], f"{what} {n}")
    if stats is not None:
        out["lse"] = hold_stats(ref, A, stats, what)
    return out


def hold_stats(ref, A, stats, what):
    """m + ln l against lse on the rows with an allowed key: assert_f32_close (8 * e32 + 2^-20 * row max |lse|), plus u * A_lse where the
    generated forward re-rounds q (A_lse = 0 otherwise); finite everywhere -- (m, 1 / l) itself is not unique (deferred maximum)."""
    st = stats.detach().cpu().to(F64)
    assert torch.isfinite(st).all(), f"{what}: non-finite stats"
    if st.numel() == 0:
        return 0.0
    live, lse = ref["live"], ref["lse"]
    assert (st[..., 1][live] > 0).all(), f"{what}: 1 / l <= 0 on a row with an allowed key"
    got = torch.where(live, st[..., 0] - torch.log(st[..., 1].clamp_min(1e-300)), torch.zeros_like(lse))
    want = torch.where(live, lse, torch.zeros_like(lse))
    want32 = torch.where(live, ref["lse32"].to(F64), torch.zeros_like(lse))
    if float(A["lse"].abs().max()) == 0.0:
        return ref64.assert_f32_close(got, want, want32, what=what + " m + ln l")
    e32 = (want32 - want).abs().amax(-1, keepdim=True)
    bound = 8.0 * e32 + ref64.F32_SLACK * want.abs().amax(-1, keepdim=True) + ref64.U_BF16 * A["lse"]
    err = (got - want).abs()
    off = err > bound
    if off.any():
        i = tuple(int(t) for t in torch.unravel_index((err / bound).argmax(), err.shape))
        raise AssertionError(f"{what} m + ln l: {int(off.sum())} rows exceed the bound; worst at (b, h, q) {i}: got {got[i].item()!r}, "
                             f"reference {want[i].item()!r}, allowed {bound[i].item():.3e}")
    return float((err / bound).max())


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def generic_cases():
    """every <head_dim, causal, NW> of the compiler-scheduled kernels: the smallest shapes on each side of 32 / 64 queries (NW 1 / 2 / 4),
    ragged last tiles, more than one key tile; every GQA ratio; B 1 and 3; every mask kind"""
    out = []
    nc_masks, c_masks = ("none", "rand", "full"), ("none", "rand", "left")
    i = 0
    for hd in (64, 128):
        for (Sq, Sk) in ((1, 1), (3, 65), (32, 64), (33, 63), (64, 129), (65, 64), (100, 257)):
            for (nq, nkv) in HEADS:
                B, m = (1, 3)[i % 2], nc_masks[i % 3]
                # hd 64, rep 1, <= 4 x <= 16 would be the tiny kernels' shape: held to the MFMA kernels here, to the tiny ones in tiny_cases()
                modes = (("TINY", 0),) if hd == 64 and nq == nkv and Sq <= 4 and Sk <= 16 else ()
                out.append(case(f"nc hd{hd} {Sq}x{Sk} {nq}:{nkv} B{B} {m}", B, Sq, Sk, nq, nkv, hd, False, m, modes=modes))
                i += 1
        for S in (1, 2, 33, 64, 65, 127):
            for (nq, nkv) in HEADS:
                B, m = (1, 3)[i % 2], c_masks[i % 3]
                out.append(case(f"c hd{hd} S{S} {nq}:{nkv} B{B} {m}", B, S, S, nq, nkv, hd, True, m))
                i += 1
    for S in (128, 192, 384):           # the compiler-scheduled causal head_dim-128 kernels and attn_bwd_dkv2_kernel<true>
        for (nq, nkv) in HEADS:
            B, m = (1, 3)[i % 2], c_masks[i % 3]
            out.append(case(f"c hd128 S{S} {nq}:{nkv} B{B} {m} C128=0", B, S, S, nq, nkv, 128, True, m, modes=(("C128", 0),)))
            i += 1
    return out


def c128_cases():
    """the generated causal head_dim-128 kernels: one, two and three 256-row items (S 128, 384, 640), the generated forward feeding the
    generic backward (S 192, 576), rep 1 / 2 / 4, and the masks their tile skipping branches on"""
    out = []
    for S in (128, 384, 640, 192, 576):
        sets = ((("none",), ("pad", 64), ("pad", 128)), (("pad", S - 1), ("hole", 63), ("hole", 64)), (("hole", 65), ("none",), ("pad", 64)))
        for j, (nq, nkv) in enumerate(((2, 2), (4, 2), (4, 1))):
            for s, mset in enumerate(sets):
                if S in (192, 576) and s != j:           # the mixed path: one mask set per GQA ratio
                    continue
                out.append(case(f"c128 S{S} {nq}:{nkv} masks{s}", 3, S, S, nq, nkv, 128, True, mset))
    return out


def fewq_cases():
    """attn_bwd_dkv_fewq_kernel (hd 64, rep 1, <= 64 queries, >= 256 keys): one chunk with a ragged last block (256, 257), two chunks
    with a ragged last chunk (520); few (batch, head) pairs so that the launch chunks; with the kernel on and off"""
    out = []
    for (Sq, Sk, B, nq, m) in ((64, 256, 1, 2, "none"), (33, 257, 2, 1, "ragged"), (40, 520, 1, 2, "rand"), (64, 520, 2, 2, "ragged")):
        for fewq in (1, 0):
            out.append(case(f"fewq {Sq}x{Sk} B{B} nq{nq} {m} FEWQ={fewq}", B, Sq, Sk, nq, nq, 64, False, m, modes=(("FEWQ", fewq),)))
    return out


def tiny_cases():
    """attn_tiny_fwd / bwd kernels (<= 4 queries x <= 16 keys, hd 64, rep 1): pair counts that do not fill a wave (4 pairs) or a
    workgroup (16); with the kernels on (3) and off (0: the MFMA kernels on the same inputs)"""
    out = []
    for (Sq, Sk, B, nq, m) in ((1, 1, 1, 1, "none"), (2, 14, 3, 3, "full"), (4, 16, 5, 1, "rand"), (3, 5, 2, 3, "full")):
        for tiny in (3, 0):
            out.append(case(f"tiny {Sq}x{Sk} B{B} nq{nq} {m} TINY={tiny}", B, Sq, Sk, nq, nq, 64, False, m, modes=(("TINY", tiny),)))
    return out


def dropout_cases():
    """non-causal probability dropout against the float64 reference under the kernels' own keep flags (oracle/dropout_ref.attn_keep):
    odd Sk (one word decides keys 2 kp and 2 kp + 1), drop_batch0 0 / 3, a seed above 2^63, ragged masks with a fully masked sample
    (uniform softmax, then dropped), (33, 65) at hd 128 (attn_bwd_dkv_kernel<128, false, 4>), a few-query and a tiny shape"""
    big = (1 << 63) + 0x9E3779B97F4A7C15 % (1 << 62)
    return [
        case("drop hd64 40x71 p.1", 2, 40, 71, 2, 2, 64, False, "ragged", p=0.1, dseed=11, drop_batch0=0),
        case("drop hd64 64x129 p.5 b0=3", 3, 64, 129, 3, 3, 64, False, "ragged", p=0.5, dseed=big, drop_batch0=3),
        case("drop hd64 65x33 p.5 gqa", 1, 65, 33, 4, 2, 64, False, "rand", p=0.5, dseed=12, drop_batch0=3),
        case("drop hd128 33x65 p.1", 2, 33, 65, 2, 2, 128, False, "ragged", p=0.1, dseed=big + 1, drop_batch0=0),
        case("drop hd128 33x65 p.5 gqa b0=3", 2, 33, 65, 4, 1, 128, False, "none", p=0.5, dseed=13, drop_batch0=3),
        case("drop hd128 20x31 p.5", 3, 20, 31, 1, 1, 128, False, "full", p=0.5, dseed=14),
        case("drop fewq 33x257 p.1", 2, 33, 257, 2, 2, 64, False, "ragged", p=0.1, dseed=big + 2, drop_batch0=3),
        case("drop fewq 33x257 p.1 FEWQ=0", 2, 33, 257, 2, 2, 64, False, "ragged", p=0.1, dseed=big + 2, drop_batch0=3, modes=(("FEWQ", 0),)),
        case("drop tiny 2x13 p.5", 3, 2, 13, 3, 3, 64, False, "full", p=0.5, dseed=15, drop_batch0=3),
        case("drop tiny 2x13 p.5 TINY=0", 3, 2, 13, 3, 3, 64, False, "full", p=0.5, dseed=15, drop_batch0=3, modes=(("TINY", 0),)),
        case("drop tiny 4x16 p.1", 2, 4, 16, 1, 1, 64, False, "rand", p=0.1, dseed=big + 3),
    ]


def value_cases():
    """near one-hot and exactly uniform softmax, exactly zero gradients, a zero v, scale far from hd ** -0.5"""
    out = []
    for hd, causal, Sq, Sk in ((64, False, 33, 65), (128, True, 65, 65), (64, False, 3, 5)):
        tag = f"hd{hd} {'c' if causal else 'nc'} {Sq}x{Sk}"
        out.append(case(f"values std4 {tag}", 2, Sq, Sk, 4, 2, hd, causal, "rand", values="std4"))
        out.append(case(f"values equal_keys {tag}", 2, Sq, Sk, 2, 2, hd, causal, "none", values="equal_keys"))
        out.append(case(f"values dout0 {tag}", 2, Sq, Sk, 2, 2, hd, causal, "rand", values="dout0"))
        out.append(case(f"values v0 {tag}", 2, Sq, Sk, 2, 2, hd, causal, "rand", values="v0"))
        for sc in (0.05, 1.0):
            out.append(case(f"values scale{sc} {tag}", 2, Sq, Sk, 2, 2, hd, causal, "rand", scale=sc))
    out.append(case("values scale0.05 c128 S128", 1, 128, 128, 2, 1, 128, True, "none", scale=0.05))
    out.append(case("values scale1.0 hd64 tiny 2x14", 2, 2, 14, 2, 2, 64, False, "rand", scale=1.0))
    return out


def layout_cases():
    """strided operands and outputs (see test_strided_outputs_leave_their_gaps_untouched): both mask semantics, the generic, generated,
    few-query and tiny kernels"""
    return [
        case("layout nc hd64 33x65", 2, 33, 65, 2, 2, 64, False, "rand"),
        case("layout nc hd128 65x40", 2, 65, 40, 4, 2, 128, False, "full"),
        case("layout c hd64 65", 2, 65, 65, 2, 1, 64, True, "left"),
        case("layout c hd128 130", 2, 130, 130, 4, 2, 128, True, "rand"),
        case("layout c128 S128", 2, 128, 128, 4, 2, 128, True, (("none",), ("pad", 64))),
        case("layout c hd128 S128 C128=0", 2, 128, 128, 4, 2, 128, True, (("none",), ("pad", 64)), modes=(("C128", 0),)),
        case("layout fewq 33x257", 1, 33, 257, 2, 2, 64, False, "ragged"),
        case("layout tiny 2x14", 3, 2, 14, 3, 3, 64, False, "full"),
    ]


def all_cases():
    return generic_cases() + c128_cases() + fewq_cases() + tiny_cases() + dropout_cases() + value_cases() + layout_cases()

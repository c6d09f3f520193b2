"""GPU: ur_attn_fwd / ur_attn_bwd, ELEMENT BY ELEMENT against the float64 reference of tests/ref64.py (attention section; itself checked
on the CPU in tests/test_ref64.py), on every kernel behind the dispatcher of unirec_amd/csrc/attn.hip and at the shapes where each branches.
The cases live in tests/attn_cases.py (plain CPU code, so the CPU suite can check the criteria on the very same inputs).

Criteria (derivations and the per-kernel list of rounding points: docs/lab_notes.md, "Element-wise float64 tests: attention"):
  hard bound, every element of o, dq, dk, dv    |got - ref| <= 2^-8 * A + 2^-20 * A, A = the reference's formula with every summand replaced by its
                                                magnitude, one term per point where the kernel path rounds to bf16 (ref64.attention_bounds)
  sharp criterion, every (batch, head) slice    ||got - ref||_F <= 3 * ||emul - ref||_F + 2^-20 * ||A||_F, emul = the same arithmetic in torch on the
                                                CPU with bf16 roundings at those points (ref64.attention_emulated) -- never the kernel's own error
  stats                                         m + ln l against the float64 lse through assert_f32_close on rows with an allowed key (+ 2^-8 * A_lse
                                                where the generated forward re-rounds q); finite everywhere
  dropout                                       the reference runs under the kernels' own keep flags, restated on the CPU (oracle/dropout_ref.attn_keep)
  gaps of strided outputs, refused calls        bit for bit the sentinel
No element is exempt.  Every test prints its worst ratios ("[ratio] ..."); test_zz_worst_ratio_table prints the table.

Not held here (see the issue that added this module): the persistent dK/dV walk (> 256 key blocks; bit-identical to the per-block launch in
tests/test_gpu_switches.py) and the rope_q / rope_k fused stores (against kernels that tests/test_gpu_head_primitives.py holds to float64).
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dropout_ref  # noqa: E402
from tests import attn_cases as ac  # noqa: E402
from tests import ref64  # noqa: E402
from unirec_amd import _lib, hip  # noqa: E402
from unirec_amd._lib import AttnArgs, AttnBwdArgs  # noqa: E402

# entry point -> the primitive-level tests of this module that hold it against a reference (tests/test_abi_test_coverage.py)
COVERS = {
    "ur_attn_fwd": ["test_generic_kernels", "test_generated_causal_hd128_kernels", "test_tiny_kernels", "test_dropout_against_the_reference",
                    "test_values", "test_strided_outputs_leave_their_gaps_untouched", "test_forward_alone_accepts_a_4_element_output_stride",
                    "test_empty_batch_writes_nothing", "test_argument_checks_reject_without_launching"],
    "ur_attn_bwd": ["test_generic_kernels", "test_generated_causal_hd128_kernels", "test_few_query_dkv_and_kv_colsum", "test_tiny_kernels",
                    "test_dropout_against_the_reference", "test_values", "test_strided_outputs_leave_their_gaps_untouched",
                    "test_empty_batch_writes_nothing", "test_argument_checks_reject_without_launching"],
    "ur_attn_dropout_keep": ["test_dropout_against_the_reference"],
}

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENTINEL = 0x4B4B                    # a finite bf16 bit pattern nothing computes by accident
WORST = {}


def _note(kernel, ratio):
    WORST[kernel] = max(WORST.get(kernel, 0.0), float(ratio))
    print(f"[ratio] {kernel}: {float(ratio):.4f}")


def _note_all(family, ratios):
    for what, r in ratios.items():
        _note(f"{family} {what}", r)


_modes = ac.plan_modes      # with _modes(case["modes"]): every ur_attn_mode word of the case set, all restored on exit


def _ids(cases):
    return [c["name"] for c in cases]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _dev(x):
    return {n: (None if t is None else t.to(DEV)) for n, t in x.items()}


def _fwd_bwd(c, d, out=None, grads=(None, None, None), kv_colsum=None, backward=True):
    with _modes(c["modes"]):
        o, ctx = hip.attn_fwd(d["q"], d["k"], d["v"], causal=c["causal"], key_mask=d["key_mask"], scale=c["scale"], dropout_p=c["p"],
                              seed=c["dseed"], drop_batch0=c["drop_batch0"], out=out)
        got = {"o": o}
        if backward:
            got["dq"], got["dk"], got["dv"] = hip.attn_bwd(ctx, d["dout"], dq=grads[0], dk=grads[1], dv=grads[2], kv_colsum=kv_colsum)
        torch.cuda.synchronize()
    return got, ctx


def _check(c, family):
    """forward + backward of one case on contiguous operands, both criteria on o, dq, dk, dv and the stats check"""
    d = _dev(ac.inputs(c))
    got, ctx = _fwd_bwd(c, d)
    A, emul = ac.criteria(c)
    _note_all(family, ac.hold(ac.reference(c), A, emul, got, c["name"], stats=ctx.stats))
    return got, ctx


# =============================================================================================================================
@pytest.mark.parametrize("c", ac.generic_cases(), ids=_ids(ac.generic_cases()))
def test_generic_kernels(c):
    """attn_fwd_kernel / attn_bwd_dq_kernel / attn_bwd_dkv_kernel<hd, causal, NW> for every instantiation, and attn_bwd_dkv2_kernel (hd 128
    without dropout)"""
    _check(c, f"generic hd{c['hd']} {'causal' if c['causal'] else 'non-causal'}")


@pytest.mark.parametrize("c", ac.c128_cases(), ids=_ids(ac.c128_cases()))
def test_generated_causal_hd128_kernels(c):
    """attn_fwd_c128_kernel, attn_bwd_dq_c128_kernel, attn_bwd_dkv_c128_kernel (S % 128 == 0) and the generated forward feeding the generic
    backward (S = 192, 576)"""
    assert ac.qk_round(c) == ("all" if c["Sk"] % 128 == 0 else "fwd")
    _check(c, "generated c128" if c["Sk"] % 128 == 0 else "generated fwd + generic bwd")


@pytest.mark.parametrize("c", ac.fewq_cases(), ids=_ids(ac.fewq_cases()))
def test_few_query_dkv_and_kv_colsum(c):
    """attn_bwd_dkv_fewq_kernel (chunked launch) and, on the same inputs, attn_bwd_dkv_kernel; then kv_colsum (which forces one chunk) against
    the float64 column sums of the float64 dK / dV, within the summed A"""
    on = dict(c["modes"])["FEWQ"] == 1
    _, ctx = _check(c, "few-query dkv" if on else "few-query shape, generic dkv")
    with _modes(c["modes"]):
        assert hip.attn_bwd_kv_colsum_supported(ctx) == on
        if not on:
            return
        nq, hd = c["nq"], c["hd"]
        colsum = torch.full((2 * nq * hd,), float("nan"), device=DEV)
        d = _dev(ac.inputs(c))
        dq, dk, dv = hip.attn_bwd(ctx, d["dout"], kv_colsum=colsum)
        torch.cuda.synchronize()
    ref, (A, emul) = ac.reference(c), ac.criteria(c)
    _note_all("few-query dkv (one chunk)", ac.hold(ref, A, emul, {"dq": dq, "dk": dk, "dv": dv}, c["name"] + " with kv_colsum"))
    want = torch.cat([ref["dk"].sum(dim=(0, 1)).reshape(-1), ref["dv"].sum(dim=(0, 1)).reshape(-1)])
    bound = torch.cat([A["dk"].sum(dim=(0, 1)).reshape(-1), A["dv"].sum(dim=(0, 1)).reshape(-1)])
    _note("kv_colsum bound", ref64.assert_attn_bound(colsum, want, bound, c["name"] + " kv_colsum"))


@pytest.mark.parametrize("c", ac.tiny_cases(), ids=_ids(ac.tiny_cases()))
def test_tiny_kernels(c):
    """attn_tiny_fwd_kernel / attn_tiny_bwd_kernel<2 | 4>, and the MFMA kernels on the same inputs"""
    _check(c, "tiny" if dict(c["modes"])["TINY"] == 3 else "tiny shape, MFMA kernels")


@pytest.mark.parametrize("c", ac.dropout_cases(), ids=_ids(ac.dropout_cases()))
def test_dropout_against_the_reference(c):
    """probability dropout, forward and backward, against the float64 reference under the keep flags of oracle/dropout_ref.attn_keep -- and
    ur_attn_dropout_keep exports exactly those flags"""
    x = ac.inputs(c)
    B, nq, Sq, Sk = c["B"], c["nq"], c["Sq"], c["Sk"]
    dev_keep = hip.attn_dropout_keep(c["dseed"], c["p"], c["drop_batch0"] * nq * Sq, B * nq * Sq, Sk, DEV).cpu().reshape(B, nq, Sq, Sk)
    assert torch.equal(dev_keep, x["keep"])
    _check(c, f"dropout hd{c['hd']}")


@pytest.mark.parametrize("c", ac.value_cases(), ids=_ids(ac.value_cases()))
def test_values(c):
    got, _ = _check(c, "values")
    if c["values"] == "dout0":
        assert all(float(got[n].float().abs().max()) == 0.0 for n in ("dq", "dk", "dv"))
    if c["values"] == "v0":
        assert float(got["o"].float().abs().max()) == 0.0 and float(got["dq"].float().abs().max()) == 0.0 and float(got["dk"].float().abs().max()) == 0.0


# =============================================================================================================================
# layout
def _strided(t, pad, fill=None, offset=0):
    """a copy of t [B, S, heads, hd] as a view with token stride heads * hd + pad into a fresh buffer, `offset` elements past its base;
    returns (view, buffer).  fill None: the gaps hold other random data (inputs); else the sentinel pattern (outputs)."""
    B, S, H, D = t.shape
    ld = H * D + pad
    if fill is None:
        buf = torch.randn(B * S * ld + offset, device=DEV).to(BF16)
    else:
        buf = torch.full((B * S * ld + offset,), fill, dtype=torch.int16, device=DEV).view(BF16)
    view = buf[offset:].view(B, S, ld)[..., :H * D].view(B, S, H, D)
    if fill is None:
        view.copy_(t)
    return view, buf


def _gaps_untouched(view, buf, before, what):
    """every element of buf outside view still holds its bits"""
    mask = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    B, S, H, D = view.shape
    off = (view.data_ptr() - buf.data_ptr()) // 2
    mask[off:].view(B, S, -1)[..., :H * D] = False
    assert torch.equal(_bits(buf)[mask], before[mask]), f"{what}: a gap element of the strided output was written"


@pytest.mark.parametrize("grad_pad,grad_offset", [(8, 0), (4, 4)], ids=["ld+8", "ld+4, 8-byte base"])
@pytest.mark.parametrize("c", ac.layout_cases(), ids=_ids(ac.layout_cases()))
def test_strided_outputs_leave_their_gaps_untouched(c, grad_pad, grad_offset):
    """q, k, v, dout each with its own token stride; o (token stride heads * hd + 8), dq, dk, dv (+ 8, or + 4 from a base that is 8- but not
    16-byte aligned) as views into sentinel-filled buffers: both criteria on the results, every gap element keeps the sentinel bits"""
    x = _dev(ac.inputs(c))
    d = dict(x)
    for n, pad in (("q", 8), ("k", 16), ("v", 24), ("dout", 32)):
        d[n], _ = _strided(x[n], pad)
    o, obuf = _strided(x["q"], 8, SENTINEL)
    gr = [_strided(x[n], grad_pad, SENTINEL, grad_offset) for n in ("q", "k", "v")]
    assert all(g[0].data_ptr() % 16 == 2 * grad_offset for g in gr)
    before = [_bits(b).clone() for b in [obuf] + [g[1] for g in gr]]
    got, ctx = _fwd_bwd(c, d, out=o, grads=tuple(g[0] for g in gr))
    assert got["o"].data_ptr() == o.data_ptr() and all(got[n].data_ptr() == g[0].data_ptr() for n, g in zip(("dq", "dk", "dv"), gr))
    A, emul = ac.criteria(c)
    _note_all("strided", ac.hold(ac.reference(c), A, emul, got, c["name"], stats=ctx.stats))
    for (view, buf), b0, n in zip([(o, obuf)] + gr, before, ("o", "dq", "dk", "dv")):
        _gaps_untouched(view, buf, b0, f"{c['name']} {n}")


@pytest.mark.parametrize("c", ac.layout_cases(), ids=_ids(ac.layout_cases()))
def test_forward_alone_accepts_a_4_element_output_stride(c):
    """ur_attn_fwd takes ldo % 4 == 0 (every second row of o is then 8-, not 16-byte aligned); ur_attn_bwd needs ldo % 8 == 0 and refuses
    that context"""
    d = _dev(ac.inputs(c))
    o, obuf = _strided(d["q"], 4, SENTINEL)
    before = _bits(obuf).clone()
    got, ctx = _fwd_bwd(c, d, out=o, backward=False)
    A, emul = ac.criteria(c)
    _note_all("strided", ac.hold(ac.reference(c), A, emul, got, c["name"] + " ldo + 4", stats=ctx.stats))
    _gaps_untouched(o, obuf, before, c["name"] + " o")
    grads = [torch.full(d[n].shape, SENTINEL, dtype=torch.int16, device=DEV).view(BF16) for n in ("q", "k", "v")]
    with _modes(c["modes"]), pytest.raises(_lib.UniRecHipError, match="rc=-"):
        hip.attn_bwd(ctx, d["dout"], dq=grads[0], dk=grads[1], dv=grads[2])
    torch.cuda.synchronize()
    assert all(bool((_bits(g) == SENTINEL).all()) for g in grads)


# =============================================================================================================================
# arguments
def _raw_case():
    """a valid non-causal call (B 2, 33 x 40, 4 : 2 heads, hd 64) as raw argument structs over sentinel-filled outputs"""
    B, Sq, Sk, nq, nkv, hd = 2, 33, 40, 4, 2, 64
    t = lambda *s: torch.randn(s, device=DEV).to(BF16)          # noqa: E731
    sent = lambda *s: torch.full(s, SENTINEL, dtype=torch.int16, device=DEV).view(BF16)          # noqa: E731
    keepalive = dict(q=t(B, Sq, nq, hd), k=t(B, Sk, nkv, hd), v=t(B, Sk, nkv, hd), dout=t(B, Sq, nq, hd), o=sent(B, Sq, nq, hd),
                     dq=sent(B, Sq, nq, hd), dk=sent(B, Sk, nkv, hd), dv=sent(B, Sk, nkv, hd),
                     stats=torch.full((B, nq, Sq, 2), 123.0, device=DEV),
                     delta=torch.full((int(_lib.load().ur_attn_bwd_workspace_floats(B, nq, Sq)),), 123.0, device=DEV),
                     colsum=torch.full((2 * nq * hd,), 123.0, device=DEV), colsum_ws=torch.full((2 * B * nq * hd,), 123.0, device=DEV))
    a = AttnArgs()
    a.q, a.k, a.v, a.o, a.stats = (keepalive[n].data_ptr() for n in ("q", "k", "v", "o", "stats"))
    a.ldq, a.ldk, a.ldv, a.ldo = nq * hd, nkv * hd, nkv * hd, nq * hd
    a.key_mask = 0
    a.B, a.Sq, a.Sk, a.nq, a.nkv, a.head_dim = B, Sq, Sk, nq, nkv, hd
    a.causal, a.scale, a.dropout_p, a.seed, a.drop_batch0 = 0, hd ** -0.5, 0.0, 0, 0
    g = AttnBwdArgs()
    g.dout, g.dq, g.dk, g.dv = (keepalive[n].data_ptr() for n in ("dout", "dq", "dk", "dv"))
    g.lddo, g.lddq, g.lddk, g.lddv = nq * hd, nq * hd, nkv * hd, nkv * hd
    g.delta = keepalive["delta"].data_ptr()
    return a, g, keepalive


def _untouched(keep):
    torch.cuda.synchronize()
    return (all(bool((_bits(keep[n]) == SENTINEL).all()) for n in ("o", "dq", "dk", "dv"))
            and all(bool((keep[n] == 123.0).all()) for n in ("stats", "delta", "colsum", "colsum_ws")))


def _with(struct, **fields):
    s = type(struct).from_buffer_copy(struct)
    for k, v in fields.items():
        setattr(s, k, v)
    return s


def test_empty_batch_writes_nothing():
    lib, st = _lib.load(), hip._stream()
    a, g, keep = _raw_case()
    a0 = _with(a, B=0)
    assert lib.ur_attn_fwd(ctypes.byref(a0), st) == 0
    assert lib.ur_attn_bwd(ctypes.byref(a0), ctypes.byref(g), st) == 0
    assert _untouched(keep)
    # and the same structs with B = 2 do run
    assert lib.ur_attn_fwd(ctypes.byref(a), st) == 0 and lib.ur_attn_bwd(ctypes.byref(a), ctypes.byref(g), st) == 0
    torch.cuda.synchronize()
    assert not any(bool((_bits(keep[n]) == SENTINEL).any()) for n in ("o", "dq", "dk", "dv")) and not bool((keep["stats"] == 123.0).any())


def test_argument_checks_reject_without_launching():
    """every UR_REQUIRE of fill / ur_attn_fwd / ur_attn_bwd: a negative code, a message that names the entry point, nothing launched (all
    outputs, the stats and the workspace keep their sentinel)"""
    lib, st = _lib.load(), hip._stream()
    a, g, keep = _raw_case()
    nq, nkv, hd = a.nq, a.nkv, a.head_dim

    def refused(a_, g_=None, fwd=True, bwd=True):
        if fwd:
            rc = lib.ur_attn_fwd(ctypes.byref(a_), st)
            assert rc < 0 and b"ur_attn" in lib.ur_last_error(), (rc, lib.ur_last_error())
        if bwd:
            rc = lib.ur_attn_bwd(ctypes.byref(a_), ctypes.byref(g if g_ is None else g_), st)
            assert rc < 0 and b"ur_attn" in lib.ur_last_error(), (rc, lib.ur_last_error())
        assert _untouched(keep)

    refused(_with(a, head_dim=96))
    refused(_with(a, nq=3))                                    # 3 % 2 != 0
    refused(_with(a, causal=1))                                # Sq 33 != Sk 40
    refused(_with(a, causal=1, Sk=a.Sq, dropout_p=0.1))        # causal with dropout
    refused(_with(a, dropout_p=1.0))
    refused(_with(a, scale=0.0))
    refused(_with(a, Sk=8193))
    refused(_with(a, ldq=nq * hd - 8))                         # strides below heads * hd
    refused(_with(a, ldk=nkv * hd - 8))
    refused(_with(a, ldv=nkv * hd - 8))
    refused(_with(a, ldq=nq * hd + 4))                         # q / k / v rows: 16 bytes
    refused(_with(a, q=a.q + 8))
    refused(_with(a, k=a.k + 2))
    refused(_with(a, v=a.v + 4))
    refused(_with(a, q=0))
    refused(_with(a, stats=0))
    refused(_with(a, stats=a.stats + 2))                       # the f32 planes: 4 bytes
    # the output of the forward: 16-byte base, ldo % 4, ldo >= heads * hd (the backward only reads o: 16-byte rows)
    refused(_with(a, o=a.o + 8))
    refused(_with(a, ldo=nq * hd + 2))
    refused(_with(a, ldo=nq * hd - 8), bwd=False)
    refused(_with(a, o=0))
    refused(_with(a, ldo=nq * hd + 4), fwd=False)
    # the backward's own operands
    refused(a, _with(g, dout=g.dout + 8), fwd=False)
    refused(a, _with(g, lddo=nq * hd + 4), fwd=False)
    refused(a, _with(g, dq=g.dq + 4), fwd=False)               # gradients: 8-byte base, ld % 4
    refused(a, _with(g, dk=g.dk + 2), fwd=False)
    refused(a, _with(g, dv=g.dv + 4), fwd=False)
    refused(a, _with(g, lddq=nq * hd + 2), fwd=False)
    refused(a, _with(g, lddk=nkv * hd + 2), fwd=False)
    refused(a, _with(g, lddv=nkv * hd + 6), fwd=False)
    refused(a, _with(g, dq=0), fwd=False)
    refused(a, _with(g, delta=0), fwd=False)
    refused(a, _with(g, delta=g.delta + 2), fwd=False)
    refused(a, _with(g, kv_colsum=keep["colsum"].data_ptr() + 2, kv_colsum_ws=keep["colsum_ws"].data_ptr()), fwd=False)
    refused(a, _with(g, kv_colsum=keep["colsum"].data_ptr(), kv_colsum_ws=keep["colsum_ws"].data_ptr() + 2), fwd=False)
    refused(a, _with(g, rope_rstd=keep["stats"].data_ptr() + 2), fwd=False)
    # kv_colsum where the few-query kernel does not run (40 keys), and without its scratch
    assert lib.ur_attn_bwd_kv_colsum_floats(ctypes.byref(a)) == 0
    refused(a, _with(g, kv_colsum=keep["colsum"].data_ptr(), kv_colsum_ws=keep["colsum_ws"].data_ptr()), fwd=False)
    # the fused q-norm / RoPE backward is causal head_dim-128 only
    refused(a, _with(g, rope_q_raw=a.q), fwd=False)
    # ... and the unchanged structs are accepted
    assert lib.ur_attn_fwd(ctypes.byref(a), st) == 0 and lib.ur_attn_bwd(ctypes.byref(a), ctypes.byref(g), st) == 0
    torch.cuda.synchronize()


def test_dropout_reference_flags_are_the_documented_rows():
    """the dropout row of (b, h, q) is ((drop_batch0 + b) * nq + h) * Sq + q: samples 3 .. 4 of a 5-sample call draw what samples 0 .. 1 of a
    call with drop_batch0 = 3 draw (oracle/dropout_ref.attn_keep, the flags the reference of this module runs under)"""
    full = dropout_ref.attn_keep(77, 0.3, 5, 3, 4, 9, 0)
    assert (full[3:] == dropout_ref.attn_keep(77, 0.3, 2, 3, 4, 9, 3)).all()


def test_zz_worst_ratio_table():
    """prints the worst observed error / bound per kernel family over the tests of this module that ran before it (docs/lab_notes.md)"""
    print("\n[table] worst ratio per kernel family: hard bound (error / ((2^-8 + 2^-20) A)), Frobenius (error / (3 emul + 2^-20 A)), lse")
    for k in sorted(WORST):
        print(f"[table] {k:60s} {WORST[k]:.4f}")
    assert all(math.isfinite(v) for v in WORST.values())

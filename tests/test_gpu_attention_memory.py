"""GPU: WHERE ur_attn_fwd and ur_attn_bwd read and write.  tests/test_gpu_attention_f64.py holds the values on fresh 512-byte-aligned torch
tensors, with `delta` a torch.empty; here every row of tests/train_memory_cases.py's attention table
(tests/test_train_memory_cases_host.py shows that it reaches every kernel of ur_attn_plan, both UR_ATTN_MODE_DKV_PERSIST settings and the
three rope_* forms) goes through the raw C ABI -- ur_attn_fwd, then ur_attn_bwd on the o and stats it wrote -- with every pointer placed
by tests/arena.py:

  * at a 256-byte boundary + exactly what the header promises: 16 for q, k, v, o, dout, rope_q_raw, rope_dq_raw, rope_k, rope_dk_raw, the
    norm weights and the cos / sin tables; 8 for dq, dk, dv (dk 16 where rope_k runs the stand-alone k kernel); 4 for stats, delta, kv_colsum, kv_colsum_ws, rope_rstd and key_mask (whose
    bytes are read one at a time: the arena's smallest step);
  * q, k, v, o, dout as [B * S, heads * hd] views of rows 8 elements wider, dq, dk, dv 4 wider (0xFF = NaN in the pad of an input, 0x5A
    in the pad of an output) between guards of max(64 KiB, 256 rows): a row fetched behind the last token of the last batch row, the
    next-block prefetches of the dK/dV kernels and a whole-tile store behind dk land in memory the test owns;
  * `delta` at exactly ur_attn_bwd_workspace_floats words and kv_colsum_ws at exactly ur_attn_bwd_kv_colsum_floats, their interiors 0xFF
    in one run and 0x00 in another.

Every row asserts the contract of tests/memory_harness.py: (1) rc == 0 from both calls; (2) every guard and pad column intact, every input
unchanged; (3) every element of o, stats, dq, dk, dv (kv_colsum, rope_dq_raw, rope_dk_raw) written -- and what the header says is NOT
written is the fill bit for bit: dq under rope_q_raw, dk where the generated store writes rope_dk_raw, and the two dropout key planes of
`delta` when dropout_p == 0 (they hold the interior of the run, 0xFF or 0x00); (4) bit equality with hip.attn_fwd / hip.attn_bwd on
ordinary tensors; (5) both criteria and the stats check of tests/attn_cases.py (hold: the hard bound and the Frobenius criterion of
test_gpu_attention_f64) -- the rope_* outputs against the two-kernel path within the bounds tests/test_gpu_attention.py holds them to,
kv_colsum within the summed A of test_few_query_dkv_and_kv_colsum; (6) the 0xFF run, the 0x00 run and a run whose outputs were pre-filled
0xFF agree in every output bit.  The attention calls take no sized workspace: (7) does not apply.  No tolerance is new.  Every row sets
its ur_attn_mode words through tests/attn_cases.py:plan_modes, which restores them on exit.

Workspace regions of `delta` (nrows = B * nq * Sq words each; read off attn.hip; the poison confirms the reading, it does not replace it):

  plane 0  -rowsum(dO * O)       written by the dQ launch (attn_bwd_dq_kernel, attn_bwd_dq_c128_kernel, attn_tiny_bwd_kernel is the whole
  plane 1  -LSE / scale            backward and uses neither): every row q < Sq of every (b, h) -- ws[srow], ws[nrows + srow] under `qok`
           (-LSE log2 e on the     read by the dK/dV launch: attn_bwd_dkv_kernel / dkv2 at p.delta[sbase + min(.., Sq - 1)] (clamped INSIDE
           generated pair)         the (b, h) plane), the LDS-DMA fetches of attn_bwd_dkv_kernel and the generated kernel at
                                   p.delta + sbase + rd.  For the last (b, h) of a ragged query tile rd runs past plane 1 into
  plane 2, 3  dropout row keys     the key planes: written by the dQ launch only under dropout (p.rowkeys[srow], [nrows + srow]), read by
                                   dK/dV only under dropout.  Without dropout they keep the caller's bytes; what a fetch past plane 1
                                   brings from there belongs to query rows >= Sq, which every reader discards by position (a select on
                                   the row index, no multiply-by-zero): the 0xFF and 0x00 runs agree in every bit
  8 queue words (+ 8 pad)        zeroed by the dQ launch (blockIdx.x == 0, tid < 8 of attn_bwd_dq_c128_kernel) before the persistent dK/dV
                                   launch of the same call draws from them with atomicAdd; no other kernel touches them
  kv_colsum_ws [B][2][nq][hd]    written by attn_bwd_dkv_fewq_kernel (one workgroup per (b, h) with kv_colsum: every word), read by
                                   kv_colsum_reduce_kernel

Alignments written into include/unirec_hip.h together with this module, each now refused by name before any launch: stats 4, delta 4,
kv_colsum / kv_colsum_ws 4, rope_rstd 4 (every access is one 32-bit word, the LDS-DMA fetches included); key_mask has none (bytes).

Findings.  No guard byte, pad column or poisoned word reaches an output.  One refusal came too late: with rope_k on a shape off the
generated pair (row rope-k-192) ur_attn_bwd took dk at the 8 bytes the header promises, ran dQ and dK/dV, and only then
ur_qknorm_rope_bwd_roped_k refused dk ("alignment / stride": it reads dk in 16-byte pieces) -- rc < 0 with dq, dk and dv already written.
Fixed in attn.hip: that path now asks for a 16-byte aligned dk beside the dense one, before anything is launched; the header says so.
Nothing else in unirec_amd/csrc had to change beyond the refusals above.  Wall time on the MI355X: 20 tests in 5.3 s (the module alone,
one process)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import arena, ref64  # noqa: E402
from tests import attn_cases as ac  # noqa: E402
from tests import memory_harness as mh  # noqa: E402
from tests import train_memory_cases as tm  # noqa: E402
from unirec_amd import _lib, hip  # noqa: E402

COVERS = {
    "ur_attn_fwd": ["test_attention_memory", "test_planes_below_their_alignment_are_refused_by_name"],
    "ur_attn_bwd": ["test_attention_memory", "test_planes_below_their_alignment_are_refused_by_name"],
}

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
EPS, THETA = 1e-6, 1e6


def _row(name):
    return next(c for c in tm.ATTN_CASES if c["name"] == name)


def _ac_case(c):
    return ac.case(c["name"], c["B"], c["Sq"], c["Sk"], c["nq"], c["nkv"], c["hd"], c["causal"], c["mask"], p=c["p"], dseed=tm.ATTN_SEED,
                   drop_batch0=tm.ATTN_BATCH0, modes=c["modes"])


def _rope_inputs(c):
    """what the rope_* forms read beside the attention's own operands: a raw q projection, 1 / rms per (token, head), the norm weights, the
    tables.  Any values do: the fused store and the two-kernel path it is held to read the same ones."""
    g = torch.Generator().manual_seed(77 + c["Sq"])
    M, nq, nkv, hd = c["B"] * c["Sq"], c["nq"], c["nkv"], c["hd"]
    cos, sin = hip.rope_table(c["Sq"], hd, THETA, DEV)
    return dict(raw=torch.randn((M, (nq + 2 * nkv) * hd), generator=g).to(BF16).to(DEV), rstd=(0.5 + torch.rand((M, nq + nkv), generator=g)).to(DEV),
                qw=(1.0 + 0.1 * torch.randn(hd, generator=g)).to(DEV), kw=(1.0 + 0.1 * torch.randn(hd, generator=g)).to(DEV), cos=cos, sin=sin)


def _build(c, misalign=None):
    lib, case = _lib.load(), _ac_case(c)
    x = ac.inputs(case)
    B, Sq, Sk, nq, nkv, hd = c["B"], c["Sq"], c["Sk"], c["nq"], c["nkv"], c["hd"]
    NQ, NKV, ld = nq * hd, nkv * hd, tm.attn_lds(c)
    r = _rope_inputs(c) if c["rope"] else None
    fused_k = c["rope"] == "rstd_k" and c["plan"][2] == "c128"
    nrows = B * nq * Sq
    off = lambda name: (8 if name == "dk" else 2) if name == misalign else 0      # noqa: E731
    dense_dk = c["rope"] == "rstd_k" and not fused_k      # the stand-alone k kernel reads dk: dense rows, 16 bytes

    def launch(P):
        ptr = {}
        for n, rows, w in (("q", B * Sq, NQ), ("k", B * Sk, NKV), ("v", B * Sk, NKV), ("dout", B * Sq, NQ)):
            ptr[n] = P.inp(n, x[n].reshape(rows, w), 16, ld=ld[n]).data_ptr()
        if x["key_mask"] is not None:
            ptr["key_mask"] = P.inp("key_mask", x["key_mask"], 4).data_ptr()
        ptr["o"] = P.out("o", (B * Sq, NQ), BF16, 16, ld=ld["o"]).data_ptr()
        ptr["stats"] = P.out("stats", (B, nq, Sq, 2), F32, 4).data_ptr() - off("stats")
        ptr["dq"] = P.out("dq", (B * Sq, NQ), BF16, 8, ld=ld["dq"], written=c["rope"] is None).data_ptr()
        ptr["dk"] = P.out("dk", (B * Sk, NKV), BF16, 16 if dense_dk else 8, ld=ld["dk"], written=not fused_k).data_ptr() - off("dk")
        ptr["dv"] = P.out("dv", (B * Sk, NKV), BF16, 8, ld=ld["dv"]).data_ptr()
        words = int(lib.ur_attn_bwd_workspace_floats(B, nq, Sq))
        assert words == 4 * nrows + 16
        P.delta = P.ws("delta", 4 * words, 4)
        ptr["delta"] = P.delta.data_ptr() - off("delta")
        if c["rope"]:
            ptr["rope_q_weight"], ptr["rope_cos"], ptr["rope_sin"] = (P.inp(n, r[k], 16).data_ptr() for n, k in (("rope_q_weight", "qw"), ("rope_cos", "cos"), ("rope_sin", "sin")))
            ptr["rope_dq_raw"] = P.out("rope_dq_raw", (B * Sq, NQ), BF16, 16, ld=NQ + tm.PAD).data_ptr()
            if c["rope"] == "raw":
                ptr["rope_q_raw"] = P.inp("rope_q_raw", r["raw"][:, :NQ], 16, ld=NQ + tm.PAD).data_ptr()
            else:
                ptr["rope_q_raw"] = ptr["q"]
                ptr["rope_rstd"] = P.inp("rope_rstd", r["rstd"], 4).data_ptr() - off("rope_rstd")
            if c["rope"] == "rstd_k":
                ptr["rope_k"] = ptr["k"]
                ptr["rope_k_weight"] = P.inp("rope_k_weight", r["kw"], 16).data_ptr()
                ptr["rope_dk_raw"] = P.out("rope_dk_raw", (B * Sk, NKV), BF16, 16, ld=NKV + tm.PAD).data_ptr()
        a, g = tm.attn_structs(c, ptr)
        if c["rope"]:
            g.rope_ldraw, g.rope_lddraw, g.rope_eps = (NQ + tm.PAD if c["rope"] == "raw" else ld["q"]), NQ + tm.PAD, EPS
            if c["rope"] != "raw":
                g.rope_rstd_ld, g.rope_rstd_h0 = nq + nkv, 0
            if c["rope"] == "rstd_k":
                g.rope_ldk, g.rope_rstd_hk0, g.rope_lddkraw = ld["k"], nq, NKV + tm.PAD
        with ac.plan_modes(c["modes"]):
            pl = hip.attn_plan(a, g)
            assert (pl["fwd"], pl["dq"], pl["dkv"], pl["nw_q"], pl["nw_k"]) == c["plan"], pl
            if c["colsum"]:
                nws = int(lib.ur_attn_bwd_kv_colsum_floats(ctypes.byref(a)))
                assert nws == 2 * B * nq * hd
                g.kv_colsum = P.out("kv_colsum", (2 * nq * hd,), F32, 4).data_ptr() - off("kv_colsum")
                g.kv_colsum_ws = P.ws("kv_colsum_ws", 4 * nws, 4).data_ptr()
            rc = lib.ur_attn_fwd(ctypes.byref(a), hip._stream())
            return rc if rc else lib.ur_attn_bwd(ctypes.byref(a), ctypes.byref(g), hip._stream())

    d = {n: (None if t is None else t.to(DEV)) for n, t in x.items()}

    def wrapped(**kw):
        with ac.plan_modes(c["modes"]):
            o, ctx = hip.attn_fwd(d["q"], d["k"], d["v"], causal=c["causal"], key_mask=d["key_mask"], scale=case["scale"], dropout_p=c["p"], seed=tm.ATTN_SEED,
                                  drop_batch0=tm.ATTN_BATCH0)
            dq, dk, dv = hip.attn_bwd(ctx, d["dout"], **kw)
            torch.cuda.synchronize()
        return o, ctx, dq, dk, dv

    two = lambda t, w: t.reshape(-1, w)      # noqa: E731

    def wrapper():
        kw, out = {}, {}
        if c["colsum"]:
            out["kv_colsum"] = kw["kv_colsum"] = torch.empty((2 * nq * hd,), dtype=F32, device=DEV)
        if c["rope"]:
            out["rope_dq_raw"] = torch.empty((B * Sq, NQ), dtype=BF16, device=DEV)
            kw["rope_q"] = (r["raw"][:, :NQ] if c["rope"] == "raw" else two(d["q"], NQ), r["qw"], r["cos"], r["sin"], EPS, out["rope_dq_raw"])
            if c["rope"] != "raw":
                kw["rope_rstd"] = (r["rstd"], 0)
            if c["rope"] == "rstd_k":
                out["rope_dk_raw"] = torch.empty((B * Sk, NKV), dtype=BF16, device=DEV)
                kw["rope_k"] = (two(d["k"], NKV), r["kw"], nq, out["rope_dk_raw"])
        o, ctx, dq, dk, dv = wrapped(**kw)
        out.update(o=two(o, NQ), stats=ctx.stats, dv=two(dv, NKV))
        if dq is not None:
            out["dq"] = two(dq, NQ)
        if not fused_k:
            out["dk"] = two(dk, NKV)
        return out

    def reference(outs):
        ref, (A, emul) = ac.reference(case), ac.criteria(case)
        four = dict(o=(B, Sq, nq, hd), dq=(B, Sq, nq, hd), dk=(B, Sk, nkv, hd), dv=(B, Sk, nkv, hd))
        got = {n: outs[n].reshape(four[n]) for n in four if n in outs}
        ac.hold(ref, A, emul, got, c["name"], stats=outs["stats"])
        if c["colsum"]:
            want = torch.cat([ref["dk"].sum(dim=(0, 1)).reshape(-1), ref["dv"].sum(dim=(0, 1)).reshape(-1)])
            bound = torch.cat([A["dk"].sum(dim=(0, 1)).reshape(-1), A["dv"].sum(dim=(0, 1)).reshape(-1)])
            ref64.assert_attn_bound(outs["kv_colsum"], want, bound, c["name"] + " kv_colsum")
        if c["rope"]:
            # the two-kernel path on the same inputs, within what tests/test_gpu_attention.py holds the fused stores to
            _, _, dq, dk, _ = wrapped()
            d0 = torch.zeros_like(r["raw"])
            if c["rope"] == "raw":
                hip.qknorm_rope_bwd(two(dq, NQ), two(dk, NKV), r["raw"], r["qw"], r["kw"], r["cos"], r["sin"], d0, Sq, nq, nkv, hd, EPS)
            else:
                hip.qknorm_rope_bwd_roped(two(dq, NQ), two(dk, NKV), two(d["q"], NQ), two(d["k"], NKV), r["rstd"], r["qw"], r["kw"], r["cos"], r["sin"], d0, Sq, nq, nkv, hd)
            torch.cuda.synchronize()
            pairs = [(d0[:, :NQ].float(), outs["rope_dq_raw"].float(), False)]
            if c["rope"] == "rstd_k":
                pairs.append((d0[:, NQ:NQ + NKV].float(), outs["rope_dk_raw"].float(), not fused_k))
            for want, got_, same in pairs:
                assert torch.isfinite(got_).all() and want.abs().max() > 0
                assert (want - got_).abs().max() <= 2e-2 * want.abs().max() and (want - got_).norm() / want.norm() < 3e-3
                assert not same or torch.equal(want, got_), "the stand-alone k kernel inside the call is the two-kernel path bit for bit"

    def key_planes_kept(P):
        """(3): without dropout the two key planes of `delta` are not written"""
        planes = P.delta[4 * 2 * nrows:4 * 4 * nrows]
        return bool((planes == P.interior).all())
    return launch, wrapper, reference, key_planes_kept


@pytest.mark.parametrize("name", [c["name"] for c in tm.ATTN_CASES])
def test_attention_memory(name):
    c = _row(name)
    assert tm.attn_plan_of(c) == c["plan"]
    launch, wrapper, reference, key_planes_kept = _build(c)
    runs = []

    def recorded(P):
        runs.append(P)
        return launch(P)
    mh.memory_contract(f"ur_attn[{name}]", recorded, wrapper, reference, sized=False, poisons=True)
    assert len(runs) == 3
    if c["p"] == 0:
        assert all(key_planes_kept(P) for P in runs), f"{name}: the dropout key planes of delta were written without dropout"


def test_planes_below_their_alignment_are_refused_by_name():
    """stats, delta, kv_colsum and rope_rstd at a 256-byte boundary + 2, and dk at + 8 where rope_k runs the stand-alone k kernel, which reads
    it in 16-byte pieces: a negative return that names the field, before any launch -- every output and workspace still holds its fill
    (with stats misplaced the forward already refuses; otherwise the forward has run)"""
    for name, field in (("generic-31x40-masked-row", "stats"), ("generic-31x40-masked-row", "delta"), ("fewq-33x257-colsum", "kv_colsum"),
                        ("rope-rstd-192", "rope_rstd"), ("rope-k-192", "dk")):
        launch = _build(_row(name), misalign=field)[0]
        P = mh.Placer(arena.OUT, arena.OUT)
        P.finish(launch(P))
        if field == "stats":
            mh.refused_untouched(P, f"{name}: {field} + 2", field)
        else:      # (the forward has run: o and stats are written, the backward's outputs and workspaces are not)
            assert P.rc < 0 and field in P.error, (P.rc, P.error)
            for n in ("dq", "dk", "dv", "delta") + (("kv_colsum", "kv_colsum_ws") if field == "kv_colsum" else ()):
                assert arena.untouched(P.arenas[n][0]), f"{name}: a refused backward wrote {n}"


def test_the_checks_bite():
    """without touching a kernel: a dk element left at the fill, a byte behind the last row of v changed, and an element written into the
    pad of dq each fail the placement checks of a run that passed them"""
    c = _row("generic-31x40-masked-row")
    launch = _build(c)[0]

    def run():
        P = mh.Placer()
        P.finish(launch(P))
        assert P.rc == 0
        mh.check_placement(P, "untampered")
        return P
    P = run()
    P.outputs["dk"].view(torch.int16)[c["B"] * c["Sk"] - 1, 5] = arena.OUT_HALF
    with pytest.raises(AssertionError, match="nobody stored"):
        mh.check_placement(P, "hole")
    P = run()
    whole = P.arenas["v"][0]
    whole[whole.arena[0] + whole.arena[1]] = 0
    with pytest.raises(AssertionError, match="guard of v"):
        mh.check_placement(P, "guard")
    P = run()
    P.arenas["dq"][0].base[0, c["nq"] * c["hd"]] = 1.0
    with pytest.raises(AssertionError, match="pad column of dq"):
        mh.check_placement(P, "pad")

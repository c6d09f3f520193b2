"""GPU: WHERE ur_lora_project, ur_lora_reduce, ur_lora_bgrad, ur_rmsnorm_lora_fwd and ur_swiglu_lora_fwd read and write.
tests/test_gpu_lora_f64.py holds the values on fresh 512-byte-aligned torch tensors and the recycled hip.workspace() buffer; here every row
of tests/train_memory_cases.py's LoRA table (tests/test_train_memory_cases_host.py shows that it reaches every kernel of ur_lora_plan)
goes through the raw C ABI with every pointer placed by tests/arena.py:

  * at a 256-byte boundary + exactly what the header promises: 16 for X, every U, V, G, drop_bits, drop_bits_t, the workspaces, and x, w,
    out, gu, act of the fused forwards; 8 for P; 4 for rstd;
  * X, U, V and P as [:, :width] views of rows 8 (P: 4) elements wider -- 0xFF = NaN in the pad of an input, 0x5A in the pad of P --
    between guards of max(64 KiB, 256 rows): the rows the LDS-DMA rings fetch ahead of the last token (M = 257 against 256 tokens per
    workgroup, 513 against 512) land in memory the test owns;
  * the slab workspaces at exactly the queried size, their interior 0xFF in one run and 0x00 in another.

Every row asserts the contract of tests/memory_harness.py: (1) rc == 0; (2) every guard and pad column intact, every input unchanged;
(3) every element of P, G, out, act and rstd written (no bf16 element 0x5A5A, no f32 word 0x5A5A5A5A); (4) bit equality with
hip.lora_project / lora_reduce / lora_bgrad / rmsnorm_lora_fwd / swiglu_lora_fwd on ordinary tensors; (5) the criteria of
tests/test_gpu_lora_f64.py -- the exact family of tests/lora_cases.py (small integers, alpha 2, p 0.5) against ref64.assert_lora_exact,
the fused forwards against assert_bf16_rows / assert_within_ulps / assert_lora_bf16 of the h / act bits written; (6) the 0xFF run, the
0x00 run and a run whose outputs were pre-filled 0xFF agree in every output bit; (7) a slab workspace one byte short is refused with
rc < 0 and "workspace" in ur_last_error, every output byte still the fill.  No tolerance is new.

Workspace regions (read off lora.hip; the poison confirms the reading, it does not replace it):

  ur_lora_reduce, splits > 1     slabs [splits][total] f32, total = rank * sum of widths
      written by   lora_reduce_kernel / lora_reduce_ring_kernel: workgroup (column block x, split y, adapter z) stores its 64-column
                   piece of slab y -- a split whose token range is ragged or empty still stores (zeros)
      read by      slab_sum_kernel: total / 4 float4 of each of pl.splits slabs, in slab order, into G
      splits == 1 asks for no workspace: the kernel stores G itself
  ur_lora_bgrad                  slabs [ceil(M / staged tokens per block)][total] f32 -- sized for the STAGED block count
      written by   lora_bgrad_kernel / lora_bgrad_ring_kernel<2 | 4>: block x stores slab x, x < grid x = ceil(M / tok_per_block)
      read by      slab_sum_kernel with splits = that grid x: RING (512 tokens) and RING1024 run fewer blocks than the workspace has
                   slabs, and the sum reads only the slabs that ran -- the 0xFF interior of the slabs behind them reaches no output
  ur_lora_project and the fused forwards take no workspace.

Alignments written into include/unirec_hip.h together with this module: the workspaces of ur_lora_reduce / ur_lora_bgrad 16 (already
checked, under the words "workspace too small"), drop_bits 16 with bits_stride a multiple of 16, drop_bits_t 16 for the ring (anything
less selects the register-staged kernel, as ur_lora_plan documents), x / w / out of ur_rmsnorm_lora_fwd and gu / act of
ur_swiglu_lora_fwd 16, rstd 4 (now checked).

Findings: none; nothing in unirec_amd/csrc had to change for this module beyond the rstd check.  Wall time on the MI355X: 29 tests in
2.5 s (the module alone, one process)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import arena, lora_cases, norm_cases, ref64  # noqa: E402
from tests import memory_harness as mh  # noqa: E402
from tests import train_memory_cases as tm  # noqa: E402
from tests.test_gpu_lora_f64 import RMS_EPS, _planes  # noqa: E402
from unirec_amd import _lib, hip  # noqa: E402

COVERS = {
    "ur_lora_project": ["test_lora_memory"],
    "ur_lora_reduce": ["test_lora_memory"],
    "ur_lora_bgrad": ["test_lora_memory"],
    "ur_rmsnorm_lora_fwd": ["test_lora_memory", "test_rstd_below_its_alignment_is_refused_by_name"],
    "ur_swiglu_lora_fwd": ["test_lora_memory"],
}

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


def _row(name):
    return next(c for c in tm.LORA_CASES if c["name"] == name)


def _inputs(row):
    """the exact-family case of tests/lora_cases.py for a table row, its planes on the device (compared with the numpy twin)"""
    c = lora_cases.case("exact", row["M"], row["W"], row["rank"], row["nad"], p=lora_cases.EXACT_P if row["masked"] else 0.0, cols=row["cols"],
                        seed=4000 + sum(ord(ch) for ch in row["name"]), row0=77 if row["masked"] else 0)
    c["bits"] = _planes(c)
    c["bits_t"] = hip.lora_bits_transpose(c["bits"], row["W"]) if row["bits_t"] else None
    return c


def _place_common(P, row, c):
    W, r, nad = row["W"], row["rank"], row["nad"]
    X = P.inp("X", c["X"], 16, ld=W + tm.PAD)
    bits = None if c["bits"] is None else P.inp("drop_bits", c["bits"], 16)
    return X, bits, r, nad


def _project(row):
    lib, c = _lib.load(), _inputs(row)

    def launch(P):
        X, bits, r, nad = _place_common(P, row, c)
        U = [P.inp(f"U{e}", u, 16, ld=u.shape[1] + tm.PAD) for e, u in enumerate(c["U"])]
        out = P.out("P", (row["M"], r * nad), BF16, 8, ld=r * nad + 4)
        a, _ = hip.lora_project_args(X, U, cols=row["cols"], alpha=c["alpha"], bits=bits, out=out)
        assert hip.lora_plan("project", a)["kernel"] == row["plan"][0]
        return lib.ur_lora_project(ctypes.byref(a), hip._stream())

    def wrapper():
        return dict(P=hip.lora_project(c["X"].to(DEV), [u.to(DEV) for u in c["U"]], cols=row["cols"], alpha=c["alpha"], bits=c["bits"]))

    def reference(outs):
        ref64.assert_lora_exact(outs["P"].cpu(), ref64.lora_project(c["X"], c["U"], c["keep"], c["alpha"], row["cols"]), row["name"])
    return launch, wrapper, reference, False


def _total(row):
    return row["rank"] * sum(w for _, w in (row["cols"] or [(0, row["W"])] * row["nad"]))


def _reduce(row):
    lib, c = _lib.load(), _inputs(row)
    kw = dict(cols=row["cols"], nad=row["nad"], alpha=c["alpha"], transposed=row["transposed"])
    sized = row["plan"][2] > 1

    def launch(P):
        X, bits, r, nad = _place_common(P, row, c)
        V = P.inp("V", c["V"], 16, ld=r * nad + tm.PAD)
        bt = None if c["bits_t"] is None else P.inp("drop_bits_t", c["bits_t"], 16)
        G = P.out("G", (_total(row),), F32, 16)
        a = hip.lora_reduce_args(X, V, G, bits=bits, bits_t=bt, **kw)
        pl = hip.lora_plan("reduce", a)
        assert pl["kernel"] == row["plan"][0] and (pl["splits"] > 1) == sized, pl
        need = int(lib.ur_lora_reduce_workspace_bytes(ctypes.byref(a)))
        assert need == pl["workspace_bytes"] and (need > 0) == sized
        ws = P.ws("workspace", need).data_ptr() if need else 0
        return lib.ur_lora_reduce(ctypes.byref(a), ws, need - P.short if need else 0, hip._stream())

    def wrapper():
        out = torch.empty((_total(row),), dtype=F32, device=DEV)
        return dict(G=hip.lora_reduce(c["X"].to(DEV), c["V"].to(DEV), out, bits=c["bits"], bits_t=c["bits_t"], **kw))

    def reference(outs):
        ref = ref64.lora_reduce(c["X"], c["V"], row["rank"], row["nad"], c["keep"], c["alpha"], row["cols"], row["transposed"])
        ref64.assert_lora_exact(outs["G"].cpu().reshape(-1), ref, row["name"])
    return launch, wrapper, reference, sized


def _bgrad(row):
    lib, c = _lib.load(), _inputs(row)
    r, nad = row["rank"], row["nad"]

    def launch(P):
        dy = P.inp("X", c["X"], 16, ld=row["W"] + tm.PAD)
        t = P.inp("V", c["V"], 16, ld=r * nad + tm.PAD)
        Bt = [P.inp(f"U{e}", u, 16, ld=u.shape[1] + tm.PAD) for e, u in enumerate(c["U"])]
        out = P.out("P", (row["M"], r * nad), BF16, 8, ld=r * nad + 4)
        gB = P.out("G", (_total(row),), F32, 16)
        a, _ = hip.lora_bgrad_args(dy, t, Bt, row["cols"], gB, alpha=c["alpha"], out=out)
        pl = hip.lora_plan("bgrad", a)
        assert (pl["kernel"], pl["tok_per_block"]) == row["plan"][:2], pl
        need = int(lib.ur_lora_bgrad_workspace_bytes(ctypes.byref(a)))
        assert need == pl["workspace_bytes"] and need >= pl["splits"] * _total(row) * 4
        ws = P.ws("workspace", need).data_ptr()
        return lib.ur_lora_bgrad(ctypes.byref(a), ws, need - P.short, hip._stream())

    def wrapper():
        gB = torch.empty((_total(row),), dtype=F32, device=DEV)
        tb = hip.lora_bgrad(c["X"].to(DEV), c["V"].to(DEV), [u.to(DEV) for u in c["U"]], row["cols"], gB, alpha=c["alpha"])
        return dict(P=tb, G=gB)

    def reference(outs):
        tb, dB = ref64.lora_bgrad(c["X"], c["V"], c["U"], row["cols"], c["alpha"])
        ref64.assert_lora_exact(outs["P"].cpu(), tb, row["name"] + " tb")
        ref64.assert_lora_exact(outs["G"].cpu().reshape(-1), dB, row["name"] + " dB")
    return launch, wrapper, reference, True


def _fused_case(row, p=0.1):
    c = lora_cases.fused_case(row["M"], row["W"], row["nad"], p, seed=4100 + row["M"] + row["nad"], row0=77)
    c["bits"] = _planes(c)
    return c


def _rmsnorm(row, rstd_off=0):
    lib, c = _lib.load(), _fused_case(row)
    M, D, nad = row["M"], row["W"], row["nad"]
    x, w = norm_cases.rows(M, D, 40 + M), norm_cases.norm_weight(D, 41 + M)

    def launch(P):
        xd, wd = P.inp("x", x, 16), P.inp("w", w, 16)
        U = [P.inp(f"U{e}", u, 16, ld=D + tm.PAD) for e, u in enumerate(c["U"])]
        bits = P.inp("drop_bits", c["bits"], 16)
        out, rstd = P.out("out", (M, D), BF16, 16), P.out("rstd", (M,), F32, 4)
        t = P.out("P", (M, 16 * nad), BF16, 8, ld=16 * nad + 4)
        a = hip._lora_fill(out, [(0, D)] * nad, True, bits, c["alpha"], 16, [(u.data_ptr(), u.stride(0)) for u in U], (t.data_ptr(), t.stride(0)))
        return lib.ur_rmsnorm_lora_fwd(xd.data_ptr(), wd.data_ptr(), out.data_ptr(), rstd.data_ptr() - rstd_off, M, D, RMS_EPS, ctypes.byref(a), hip._stream())

    def wrapper():
        h, rstd, t = hip.rmsnorm_lora_fwd(x.to(DEV), w.to(DEV), RMS_EPS, [u.to(DEV) for u in c["U"]], alpha=c["alpha"], bits=c["bits"])
        return dict(out=h, rstd=rstd, P=t)

    def reference(outs):
        r64, r32 = ref64.rmsnorm_fwd(x, w, RMS_EPS), ref64.rmsnorm_fwd(x, w, RMS_EPS, dtype=F32)
        ref64.assert_bf16_rows(outs["out"].cpu(), r64[0], r32[0], row["name"] + " h")
        ref64.assert_f32_close(outs["rstd"].cpu().reshape(-1, 1), r64[1].reshape(-1, 1), r32[1].reshape(-1, 1), what=row["name"] + " rstd")
        hs = outs["out"].cpu()
        args = (hs, c["U"], c["keep"], c["alpha"])
        ref64.assert_lora_bf16(outs["P"].cpu(), ref64.rms_lora_t(*args), ref64.rms_lora_t(*args, dtype=F32), ref64.rms_lora_t(*args, absolute=True),
                               row["name"] + " t")
    return launch, wrapper, reference, False


def _swiglu(row):
    lib, c = _lib.load(), _fused_case(row)
    M, I = row["M"], row["W"]
    gu = (torch.randn((M, 2 * I), generator=lora_cases.gen(60 + M + I)) * 2.0).to(BF16)

    def launch(P):
        gd = P.inp("gu", gu, 16)
        U = P.inp("U0", c["U"][0], 16, ld=I + tm.PAD)
        bits = P.inp("drop_bits", c["bits"], 16)
        act = P.out("act", (M, I), BF16, 16)
        t = P.out("P", (M, 16), BF16, 8, ld=16 + 4)
        a = hip._lora_fill(act, [(0, I)], True, bits, c["alpha"], 16, [(U.data_ptr(), U.stride(0))], (t.data_ptr(), t.stride(0)))
        return lib.ur_swiglu_lora_fwd(gd.data_ptr(), act.data_ptr(), M, I, ctypes.byref(a), hip._stream())

    def wrapper():
        act, t = hip.swiglu_lora_fwd(gu.to(DEV), I, c["U"][0].to(DEV), alpha=c["alpha"], bits=c["bits"])
        return dict(act=act, P=t)

    def reference(outs):
        ref64.assert_within_ulps(outs["act"].cpu(), ref64.swiglu_fwd(gu[:, :I], gu[:, I:]), 1, 0.0, row["name"] + " act")
        args = (outs["act"].cpu(), c["U"][0], c["keep"], c["alpha"])
        ref64.assert_lora_bf16(outs["P"].cpu(), ref64.swiglu_lora_t(*args), ref64.swiglu_lora_t(*args, dtype=F32), ref64.swiglu_lora_t(*args, absolute=True),
                               row["name"] + " t")
    return launch, wrapper, reference, False


_BUILD = dict(project=_project, reduce=_reduce, bgrad=_bgrad, rmsnorm=_rmsnorm, swiglu=_swiglu)


@pytest.mark.parametrize("name", [c["name"] for c in tm.LORA_CASES])
def test_lora_memory(name):
    row = _row(name)
    if row["plan"] is not None and row["name"] != "bgrad-ring1024":
        assert tm.lora_plan_of(row) == row["plan"]
    if row["name"] == "bgrad-ring1024":
        assert torch.cuda.get_device_properties(0).multi_processor_count == tm.CU, "the table is written for the MI355X's 256 compute units"
    launch, wrapper, reference, sized = _BUILD[row["op"]](row)
    mh.memory_contract(f"ur_lora[{name}]", launch, wrapper, reference, sized=sized, poisons=sized)


def test_rstd_below_its_alignment_is_refused_by_name():
    """rstd of ur_rmsnorm_lora_fwd at a 256-byte boundary + 2: a negative return that names it, nothing written"""
    launch = _rmsnorm(_row("rmsnorm-lora"), rstd_off=2)[0]
    P = mh.Placer(arena.OUT, arena.OUT)
    mh.refused_untouched(P.finish(launch(P)), "rstd + 2", "rstd")


def test_a_slab_left_at_the_fill_is_reported():
    """without touching a kernel: one word of G, and one element of P, put back to the fill fail the placement check of a run that passed"""
    launch = _bgrad(_row("bgrad-staged-r16"))[0]
    for name in ("G", "P"):
        P = mh.Placer()
        P.finish(launch(P))
        assert P.rc == 0
        mh.check_placement(P, "untampered")
        if name == "G":
            P.outputs["G"].view(torch.int32)[5] = arena.OUT_WORD
        else:
            P.outputs["P"].view(torch.int16)[512, 3] = arena.OUT_HALF          # a row of the ragged last block
        with pytest.raises(AssertionError, match="nobody stored"):
            mh.check_placement(P, name)

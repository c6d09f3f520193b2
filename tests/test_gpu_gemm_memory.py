"""GPU: WHERE ur_gemm and ur_gemm_grouped read and write.  tests/test_gpu_gemm_f64.py, test_gpu_norm_f64.py and test_gpu_dw_f64.py hold the
values on fresh 512-byte-aligned torch tensors and the recycled hip.workspace() buffer; here every row of tests/train_memory_cases.py's
GEMM table (tests/test_train_memory_cases_host.py shows that it reaches every kernel, tile, epilogue and mode) goes through the raw C ABI
with every pointer placed by tests/arena.py:

  * at a 256-byte boundary + exactly what the header promises: 16 for R, S, R2, S2, C, bias, drop_bits, the split_k workspace, the epilogue
    operands of the persistent kernel and qkr_qw / qkr_kw / qkr_cos / qkr_sin; 8 for swiglu_gu / swiglu_dgu / swiglu_gate / swiglu_act on
    the generic kernel; 4 for qkr_rstd;
  * every 2-D operand a [:, :width] view of rows of width + 8 elements (0xFF = NaN in the pad of an input, 0x5A in the pad of an output)
    between guards of max(64 KiB, 256 rows): a row fetched behind the last row of R or S, the overhang of the last K step (K = 72: 56
    elements) and a store one tile behind C land in memory the test owns;
  * the split_k workspace at exactly the queried size, its interior 0xFF in one run and 0x00 in another.

Every row asserts: (1) rc == 0; (2) every guard and every pad column of every input, output and workspace intact, every input unchanged;
(3) every output element the header says is written no longer holds 0x5A (no bf16 element 0x5A5A, no f32 word 0x5A5A5A5A -- the wrapper's
result has none either), and C under swiglu_gu and qkr_q, which the header says is not written, is the fill bit for bit; (4) the outputs
equal, bit for bit, what hip.gemm / hip.gemm_qkv_rope / hip.gemm_grouped return for the same arguments on ordinary tensors; (5) they pass
the reference check of the entry point's own float64 module on integer operands (ref64.assert_gemm_c / assert_gemm_f32 /
assert_gemm_gelu_grad / assert_gelu_close, _exact_bits, _hold_qkrope and the SwiGLU criteria of test_gpu_gemm_f64, assert_lora_exact over
gemm_tn of test_gpu_dw_f64); (6) the 0xFF run, the 0x00 run and a run whose OUTPUTS were pre-filled 0xFF agree in every output bit;
(7) a split_k workspace one byte short is refused with rc < 0 and "workspace" in ur_last_error, every output byte still the fill.  The
bit-identity pairs run the persistent rows' launches under ur_gemm_persistent_mode(0) and equal them bit for bit.  No tolerance is new.

Workspace regions (read off gemm.hip and gemm_body.hip.h; the poison confirms the reading, it does not replace it):

  ur_gemm, split_k > 1      slabs [splits][M][ldc] f32 (ldc == N)
      written by   gemm_kernel: workgroup (tile, split z) stores its whole tile of slab z -- also a split whose K run is empty stores
                   zeros -- so every element [z][m][n], m < M, n < N, is stored before the combine
      read by      splitk_reduce_kernel: total4 = M * ldc / 4 float4 of each of the `splits` slabs, summed in slab order into C
  ur_gemm_grouped, split_k > 1   per product i, slabs [splits][M_i][ldc_i] one after another
      written by   gemm_grouped_kernel, as above per product
      read by      splitk_reduce_grouped_kernel: blockIdx.y = product, its own total4 and slab stride
  split_k <= 1 takes no workspace; C is written once and never read (the run with 0xFF-filled outputs equals the others).

Alignments written into include/unirec_hip.h together with this module: bias 16 (float4 loads), drop_bits 16, qkr_qw / qkr_kw /
qkr_cos / qkr_sin 16 (float4 loads; refused by name now, where they used to answer "not available"), qkr_rstd 4, the split_k workspace 16
(refused by name now), the SwiGLU operands 8 on the generic kernel.

Findings: no guard byte, pad column or poisoned word reaches an output; nothing in unirec_amd/csrc had to change for this module beyond
the two refusals above.  Wall time on the MI355X: 41 tests in 9.3 s (the module alone, one process)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import arena, ref64  # noqa: E402
from tests import memory_harness as mh  # noqa: E402
from tests import train_memory_cases as tm  # noqa: E402
from tests.test_gpu_gemm_f64 import (_drop_planes, _exact_bits, _gu, _hold_qkrope, _ints, _norm_weights, _paired_rows, _randn_bf16,  # noqa: E402
                                     _tables)
from unirec_amd import _lib, hip  # noqa: E402

COVERS = {
    "ur_gemm": ["test_gemm_memory", "test_alignment_below_the_contract_is_refused_by_name"],
    "ur_gemm_grouped": ["test_gemm_memory"],
}

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


class _mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.prev = hip.gemm_persistent_mode(self.mode)

    def __exit__(self, *exc):
        hip.gemm_persistent_mode(self.prev)
        return False


def _seed(c):
    return 5000 + sum(ord(ch) for ch in c["name"])


def _tensors(c):
    """{operand name: the input tensor (device)} of a ur_gemm row, and what its references need (float64, device)"""
    M, N, K, K2, e, s = c["M"], c["N"], c["K"], c["K2"], c["epi"], _seed(c)
    R, Wn = _ints((M, K), s), _ints((N, K), s + 1)
    acc = R @ Wn.t()
    t = {}
    x = dict(acc=acc)
    Sm = Wn
    nqk = (N // 2 + N // 4) // 128
    rows = hip.swiglu_pair_rows(N // 2).to(DEV) if "swp" in e else None
    if "qkr" in e:
        Sm = _paired_rows(Wn, nqk)
    if rows is not None:
        Sm = Wn[rows]
    t["R"] = (R if c["rk"] else R.t()).contiguous().to(BF16)
    t["S"] = (Sm if c["sk"] else Sm.t()).contiguous().to(BF16)
    if K2:
        tb, Bn = _ints((M, K2), s + 2, -1, 1), _ints((N, K2), s + 3, -1, 1)
        B2 = _paired_rows(Bn, nqk) if "qkr" in e else (Bn[rows] if rows is not None else Bn)
        t["R2"] = (tb if c["rk"] else tb.t()).contiguous().to(BF16)
        t["S2"] = (B2 if c["sk"] else B2.t()).contiguous().to(BF16)
        if c["drop_rank"]:
            bits, keep = _drop_planes(s + 4, tm.DROP_P, M, N)
            t["drop_bits"] = bits.reshape(M, -1)
            x["bits"] = bits
            x["acc"] = ref64.lora_masked_epilogue(R, Wn, tb, Bn.t().contiguous(), keep[None], tm.DROP_P, c["drop_rank"])
        else:
            x["acc"] = acc + tb @ Bn.t()
    assert float(x["acc"].abs().max()) < 2.0 ** 24
    if "bias" in e:
        t["bias"] = torch.randn(N, generator=torch.Generator().manual_seed(s + 5)).to(DEV)
    if "residual" in e:
        t["residual"] = _randn_bf16((M, N), s + 6).to(DEV)
    if "gelu_grad_aux" in e:
        t["gelu_grad_aux"] = _randn_bf16((M, N), s + 7, 1.5).to(DEV)
    if "swiglu_gu" in e:
        t["swiglu_gu"] = _gu(M, N, s + 8).to(DEV)
    if "swiglu_gate" in e:
        t["swiglu_gate"] = _randn_bf16((M, N), s + 9, 2.0).to(DEV)
    if "qkr" in e:
        t["qkr_qw"], t["qkr_kw"] = _norm_weights(s + 10)
        t["qkr_cos"], t["qkr_sin"] = _tables(tm.QKR_S)
    return t, x


def _launch_one(c, t):
    """launch(P) of a ur_gemm row over the input tensors t"""
    lib = _lib.load()

    def launch(P):
        ptr = {}
        for op in tm.gemm_operands(c):
            dt = mh.DTYPES[op.dtype]
            if op.out:
                v = P.out(op.name, (op.rows, op.width), dt, op.align, ld=op.ld, written=op.written)
            elif op.ld is None:
                v = P.inp(op.name, t[op.name], op.align)
            else:
                v = P.inp(op.name, t[op.name], op.align, ld=op.ld)
            assert tuple(v.shape)[-1] == op.width and v.dtype == dt, op
            ptr[op.name] = v.data_ptr()
        a = tm.gemm_struct(c, ptr)
        need = int(lib.ur_gemm_workspace_bytes(ctypes.byref(a)))
        assert (need > 0) == (c["split"] > 1)
        ws = P.ws("workspace", need).data_ptr() if need else 0
        with _mode(c["pers_mode"]):
            return lib.ur_gemm(ctypes.byref(a), ws, need - P.short if need else 0, hip._stream())
    return launch


def _wrapper_one(c, t, x):
    e = c["epi"]

    def wrapper():
        M, N = c["M"], c["N"]
        with _mode(c["pers_mode"]):
            if "qkr" in e:
                q, k, v, rstd = hip.gemm_qkv_rope(t["R"], t["S"], t["qkr_qw"], t["qkr_kw"], t["qkr_cos"], t["qkr_sin"], tm.QKR_S, N // 2, N // 4, tm.QKR_EPS,
                                                  R2=t.get("R2"), S2=t.get("S2"))
                return dict(qkr_q=q, qkr_k=k, qkr_v=v, qkr_rstd=rstd)
            kw = dict(r_kcontig=c["rk"], s_kcontig=c["sk"], out_f32=c["f32"], alpha=c["alpha"], bias=t.get("bias"), residual=t.get("residual"),
                      gelu_grad_aux=t.get("gelu_grad_aux"), R2=t.get("R2"), S2=t.get("S2"), split_k=c["split"])
            if c["drop_rank"]:
                kw["drop"] = (x["bits"], tm.DROP_P, c["drop_rank"])
            out = {}
            if "gelu_out" in e:
                out["gelu_out"] = kw["gelu_out"] = torch.empty((M, N), dtype=BF16, device=DEV)
            if "swiglu_gu" in e:
                dgu = torch.empty((M, 2 * N), dtype=BF16, device=DEV)
                hip.gemm(t["R"], t["S"], swiglu_bwd=(t["swiglu_gu"], dgu), **kw)
                return dict(swiglu_dgu=dgu)
            if "swiglu_gate" in e:
                out["swiglu_act"] = torch.empty((M, N), dtype=BF16, device=DEV)
                kw["swiglu_fwd"] = (t["swiglu_gate"], out["swiglu_act"])
            if "swp" in e:
                out["swp_act"] = kw["swiglu_paired"] = torch.empty((M, N // 2), dtype=BF16, device=DEV)
            out["C"] = hip.gemm(t["R"], t["S"], **kw)
            torch.cuda.synchronize()
            return out
    return wrapper


def _reference_one(c, t, x):
    e, acc, tag = c["epi"], x["acc"], c["name"]
    cpu = lambda v: None if v is None else v.cpu()      # noqa: E731

    def reference(outs):
        N = c["N"]
        if "qkr" in e:
            out = (outs["qkr_q"], outs["qkr_k"], outs["qkr_v"], outs["qkr_rstd"])
            _hold_qkrope(tag, out, acc, acc, t["qkr_qw"], t["qkr_kw"], tm.QKR_S, N // 2, N // 4, lambda v, r: _exact_bits(v, r, f"{tag} v"))
        elif "swp" in e:
            _exact_bits(outs["C"], acc, f"{tag} gate|up")
            ref64.assert_ulp_ratio(outs["swp_act"], ref64.swiglu_fwd_epilogue(acc)[1], 1, 0.0, f"{tag} act")
        elif "swiglu_gu" in e:
            gate, up = t["swiglu_gu"][:, :N], t["swiglu_gu"][:, N:]
            rg, ru = ref64.swiglu_bwd_epilogue(acc, gate, up)
            ref64.assert_ulp_ratio(outs["swiglu_dgu"][:, :N], rg, 1, 2.0 ** -18 * (acc * up.to(F64)).abs(), f"{tag} d_gate")
            ref64.assert_ulp_ratio(outs["swiglu_dgu"][:, N:], ru, 1, 0.0, f"{tag} d_up")
        elif "swiglu_gate" in e:
            _exact_bits(outs["C"], acc, f"{tag} up")
            ref64.assert_ulp_ratio(outs["swiglu_act"], ref64.swiglu_fwd(t["swiglu_gate"], outs["C"]), 1, 0.0, f"{tag} act")
        elif c["f32"] and c["split"] > 1:
            assert torch.equal(outs["C"].to(F64), acc), f"{tag}: the split-K product of integers is not exact"
        elif c["f32"]:
            ref64.assert_gemm_f32(outs["C"].cpu(), acc.cpu(), c["alpha"], cpu(t.get("bias")), tag)
        elif "gelu_grad_aux" in e:
            ref64.assert_gemm_gelu_grad(outs["C"].cpu(), acc.cpu(), c["alpha"], cpu(t.get("bias")), None, t["gelu_grad_aux"].cpu(), tag)
        elif not ({"bias", "residual"} & e) and c["alpha"] == 1.0:
            _exact_bits(outs["C"], acc, tag)
        else:
            ref64.assert_gemm_c(outs["C"].cpu(), acc.cpu(), c["alpha"], cpu(t.get("bias")), cpu(t.get("residual")), tag)
        if "gelu_out" in e:
            ref64.assert_gelu_close(outs["gelu_out"].cpu(), outs["C"].cpu(), f"{tag}: gelu_out against gelu of the C written")
    return reference


def _grouped(c):
    """(launch, wrapper, reference) of a ur_gemm_grouped row"""
    lib = _lib.load()
    n, K = len(c["grouped"]), c["K"]
    ops = []
    for i, (M, N) in enumerate(c["grouped"]):
        ops.append((_ints((K, M), _seed(c) + 2 * i).to(BF16), _ints((K, N), _seed(c) + 2 * i + 1).to(BF16)))

    def launch(P):
        arr = (_lib.GemmArgs * n)()
        for i in range(n):
            ptr = {}
            for op in tm.gemm_operands(c, i):
                if op.out:
                    ptr[op.name] = P.out(op.name, (op.rows, op.width), F32, op.align, ld=op.ld).data_ptr()
                else:
                    ptr[op.name] = P.inp(op.name, ops[i][0 if op.field == "R" else 1], op.align, ld=op.ld).data_ptr()
            arr[i] = tm.gemm_struct(c, ptr, i)
        need = int(lib.ur_gemm_grouped_workspace_bytes(arr, n))
        assert (need > 0) == (c["split"] > 1)
        ws = P.ws("workspace", need).data_ptr() if need else 0
        return lib.ur_gemm_grouped(arr, n, ws, need - P.short if need else 0, hip._stream())

    def wrapper():
        outs = [torch.empty((M, N), dtype=F32, device=DEV) for M, N in c["grouped"]]
        hip.gemm_grouped([(r, s, o) for (r, s), o in zip(ops, outs)], split_k=c["split"])
        torch.cuda.synchronize()
        return {f"C{i}": o for i, o in enumerate(outs)}

    def reference(outs):
        for i, (r, s) in enumerate(ops):
            ref64.assert_lora_exact(outs[f"C{i}"], ref64.gemm_tn(r.cpu(), s.cpu()), f"{c['name']} product {i}")
    return launch, wrapper, reference


def _case(name):
    return next(c for c in tm.GEMM_CASES if c["name"] == name)


@pytest.mark.parametrize("name", [c["name"] for c in tm.GEMM_CASES])
def test_gemm_memory(name):
    c = _case(name)
    assert tm.gemm_plan_of(c) == c["plan"], "the row runs the kernel it names"
    if c["grouped"]:
        launch, wrapper, reference = _grouped(c)
    else:
        t, x = _tensors(c)
        launch, wrapper, reference = _launch_one(c, t), _wrapper_one(c, t, x), _reference_one(c, t, x)
    outs = mh.memory_contract(f"ur_gemm[{name}]", launch, wrapper, reference, sized=c["split"] > 1, poisons=c["split"] > 1)
    if c["pers_mode"] == 0:
        twin = tm.gemm_twin(c)
        assert tm.gemm_plan_of(twin)[0] == "persistent"
        want = _wrapper_one(twin, t, x)()
        for n, v in want.items():
            assert mh.same_bits(v, outs[n]), f"{name}: {n} differs between the generic and the persistent kernel"


def test_alignment_below_the_contract_is_refused_by_name():
    """every pointer the header gives an alignment, placed one step below it (a 256-byte boundary + half the alignment): a negative return
    that names the field, before any launch -- every output and the workspace still hold their fill"""
    lib = _lib.load()
    for name, field, word in (("g128-rksk-f32", "bias", "bias"), ("g128-split", "workspace", "workspace"), ("pers-e3-m0", "qkr_cos", "qkr_cos"),
                              ("pers-e3-m0", "qkr_qw", "qkr_qw"), ("pers-e3-m0", "qkr_rstd", "qkr_rstd"), ("g128-masked-r8", "drop_bits", "bit planes"),
                              ("g128-swiglu-bwd", "swiglu_gu", "8-byte aligned"), ("g128-rksk-bf16", "R", "16-byte aligned")):
        c = _case(name)
        t, _ = _tensors(c)

        def launch(P, c=c, t=t, field=field):
            ptr = {}
            for op in tm.gemm_operands(c):
                dt = mh.DTYPES[op.dtype]
                v = (P.out(op.name, (op.rows, op.width), dt, op.align, ld=op.ld) if op.out else
                     P.inp(op.name, t[op.name], op.align, ld=op.ld) if op.ld is not None else P.inp(op.name, t[op.name], op.align))
                ptr[op.name] = v.data_ptr() - (op.align // 2 if op.name == field else 0)      # (never followed: the call is refused)
            a = tm.gemm_struct(c, ptr)
            need = int(lib.ur_gemm_workspace_bytes(ctypes.byref(a)))
            ws = P.ws("workspace", need + 16).data_ptr() + (8 if field == "workspace" else 0) if need else 0
            return lib.ur_gemm(ctypes.byref(a), ws, need, hip._stream())
        P = mh.Placer(arena.OUT, arena.OUT)
        mh.refused_untouched(P.finish(launch(P)), f"{name}: {field} below its alignment", word)


def test_the_checks_bite():
    """without touching a kernel: one element written into a pad, one guard byte changed, and one output word left at the fill each fail
    the placement checks of a run that passed them"""
    c = _case("g128-rksk-bf16")
    t, _ = _tensors(c)

    def run():
        P = mh.Placer()
        P.finish(_launch_one(c, t)(P))
        assert P.rc == 0
        mh.check_placement(P, "untampered")
        return P
    P = run()
    whole, view = P.arenas["C"]
    whole.base[3, c["N"]] = 1.0                                                  # the first pad column of a row of C
    with pytest.raises(AssertionError, match="pad column of C"):
        mh.check_placement(P, "pad")
    P = run()
    whole, view = P.arenas["S"]
    whole[whole.arena[0] + whole.arena[1]] = 0                                   # the first byte behind the last row of S
    with pytest.raises(AssertionError, match="guard of S"):
        mh.check_placement(P, "guard")
    P = run()
    P.outputs["C"].view(torch.int16)[c["M"] - 1, c["N"] - 1] = arena.OUT_HALF   # the last element, as if the ragged tile had skipped it
    with pytest.raises(AssertionError, match="nobody stored"):
        mh.check_placement(P, "hole")
    P = run()
    P.arenas["R"][1][0, 0] = 9.0
    with pytest.raises(AssertionError, match="input R was written"):
        mh.check_placement(P, "input")

"""The cases of tests/test_gpu_gemm_memory.py, tests/test_gpu_attention_memory.py and tests/test_gpu_lora_memory.py: one table per family,
importable without a GPU.  tests/test_train_memory_cases_host.py asks ur_gemm_plan / ur_attn_plan / ur_lora_plan for every row (fake
non-null pointers of the stated alignment) and holds the tables to the list of kernels, tiles, epilogues and modes they must reach.

Every row is the smallest shape its kernel takes with the last tile ragged in every dimension the kernel lets be ragged; every 2-D operand
has a row stride of its width + 8 elements (a fetch that overhangs the row lands in pad, not in the next row) unless the entry point wants
it dense.  `operands` lists, per row, every pointer of the call: its struct field, shape, type, the alignment the header promises and
whether the header says the call writes it."""
from unirec_amd import _lib, hip

PAD = 8
FAKE = 1 << 20      # a 256-byte boundary: fake pointers are FAKE * k + align, as tests/arena.py places the real ones


class Op:
    """one pointer of a call: name (key of the case's tensors), field / ldfield (struct members, None = a positional argument), rows x width
    of dtype ("bf16", "f32", "u8", "i32"), ld (elements; None = dense, 1-D), align, out (the call writes it), written (the header says so)"""

    def __init__(self, name, rows, width, dtype, align, *, field=None, ldfield=None, ld=None, out=False, written=True):
        self.name, self.rows, self.width, self.dtype, self.align = name, int(rows), int(width), dtype, align
        self.field, self.ldfield, self.ld, self.out, self.written = field if field is not None else name, ldfield, ld, out, written

    def __repr__(self):
        return f"Op({self.name} [{self.rows}, {self.width}] {self.dtype} +{self.align}{' out' if self.out else ''})"


def fake_pointers(ops):
    """{name: a non-null address at a 256-byte boundary + the operand's alignment}"""
    return {op.name: FAKE * (i + 1) + op.align for i, op in enumerate(ops)}


# =====================================================================================================================================
# GEMM
def G(name, M, N, K, plan, *, rk=True, sk=True, f32=False, split=1, K2=0, alpha=1.0, drop_rank=0, pers_mode=1, **epi):
    """epi: bias / residual / gelu_out / gelu_grad_aux / swiglu_gu / swiglu_gate / qkr / swp = True.  plan: (kernel, tile, epi, mode, gcw,
    splits) as ur_gemm_plan must answer under ur_gemm_persistent_mode(pers_mode)."""
    return dict(name=name, M=M, N=N, K=K, rk=rk, sk=sk, f32=f32, split=split, K2=K2, alpha=alpha, drop_rank=drop_rank, pers_mode=pers_mode,
                epi={k for k, v in epi.items() if v}, plan=plan, grouped=None)


def GG(name, shapes, K, split, tile):
    return dict(name=name, grouped=list(shapes), K=K, split=split, pers_mode=1, plan=("grouped", tile, 0, 0, 0, split), f32=True, epi=set(),
                K2=0, drop_rank=0, rk=False, sk=False, alpha=1.0)


PERS = (2048, 4096, 256)      # 128 tiles of 256 x 256, four K tiles: the least the persistent kernel takes (gm 8, gn 16: column chunks of 4)
PERS6 = (2048, 6144, 256)     # gn 24: column chunks of 6
_EPI = {0: {}, 1: dict(swiglu_gu=True), 2: dict(residual=True, bias=True), 3: dict(qkr=True), 4: dict(swp=True), 5: dict(bias=True),
        6: dict(gelu_out=True, bias=True), 7: dict(gelu_grad_aux=True, bias=True)}
_SECOND = {0: {}, 1: dict(K2=48), 2: dict(K2=16, drop_rank=16)}
PERS_INSTANCES = sorted({(e, m) for e in (0, 1, 2, 5) for m in (0, 1, 2)} | {(3, 0), (3, 1), (4, 0), (4, 1), (6, 0), (7, 0)})

GEMM_CASES = []
for _rk, _sk in ((True, True), (True, False), (False, False), (False, True)):
    _M, _N = (130 if _rk else 136), (132 if _sk else 136)
    _t = f"r{'k' if _rk else 'm'}s{'k' if _sk else 'n'}"
    # two tiles in both directions, the last 2 .. 8 wide; K = 72 leaves the second 64-wide K step 56 short
    GEMM_CASES.append(G(f"g128-{_t}-bf16", _M, _N, 72, ("generic", 128, 0, 0, 0, 1), rk=_rk, sk=_sk, alpha=0.5, bias=True, residual=True))
    GEMM_CASES.append(G(f"g128-{_t}-f32", _M, _N, 72, ("generic", 128, 0, 0, 0, 1), rk=_rk, sk=_sk, f32=True, alpha=0.5, bias=True))
GEMM_CASES += [
    G("g128-swiglu-bwd", 130, 132, 72, ("generic", 128, 1, 0, 0, 1), swiglu_gu=True),
    G("g128-swiglu-fwd", 130, 132, 72, ("generic", 128, 2, 0, 0, 1), swiglu_gate=True),
    G("g128-split", 130, 132, 136, ("generic", 128, 0, 0, 0, 2), f32=True, split=2),
    G("g128-masked-r8", 130, 136, 72, ("generic", 128, 0, 0, 0, 1), K2=8, drop_rank=8),
    # f32: 2 x 3 big tiles x 43 splits = 258 workgroups; the last split is 8 of K = 42 * 64 + 8
    G("g256-split", 264, 520, 42 * 64 + 8, ("generic", 256, 0, 0, 0, 43), f32=True, split=43),
    # bf16: 16 x 16 tiles, the last row and column tile 8 wide: 256 workgroups, tile rows a multiple of 8 and columns of 4 -> chunks of 4
    G("g256-gcw4", 15 * 256 + 8, 15 * 256 + 8, 72, ("generic", 256, 0, 0, 4, 1)),
]
for _e, _m in PERS_INSTANCES:
    _M, _N, _K = PERS6 if (_e, _m) == (0, 0) else PERS
    GEMM_CASES.append(G(f"pers-e{_e}-m{_m}", _M, _N, _K, ("persistent", 256, _e, _m, 6 if (_e, _m) == (0, 0) else 4, 1), **_EPI[_e], **_SECOND[_m]))
# the bit-identity pairs: the same launch with the persistent kernel switched off (128 workgroups of the big tile: the 128 tile)
for _m in (0, 1, 2):
    GEMM_CASES.append(G(f"pair-e2-m{_m}", *PERS, ("generic", 128, 0, 0, 0, 1), pers_mode=0, **_EPI[2], **_SECOND[_m]))
GEMM_CASES += [
    GG("grouped128", [(136, 264), (264, 136)], 72, 1, 128),
    GG("grouped128-split", [(136, 264), (264, 136)], 136, 2, 128),
    GG("grouped256", [(776, 1032)] * 8, 72, 1, 256),           # 4 x 5 big tiles each, 160 in all, the last row and column tile 8 wide
    GG("grouped256-split", [(264, 520)] * 8, 320, 3, 256),     # 6 big tiles each, 144 with the split; K = 320 ends in a short run
]


def gemm_twin(c):
    """the row of a bit-identity pair under ur_gemm_persistent_mode(1)"""
    assert c["pers_mode"] == 0
    return next(t for t in GEMM_CASES if t["pers_mode"] == 1 and not t["grouped"] and (t["M"], t["N"], t["K"], t["K2"], t["drop_rank"], t["epi"]) ==
                (c["M"], c["N"], c["K"], c["K2"], c["drop_rank"], c["epi"]))


def gemm_operands(c, i=None):
    """the pointers of ur_gemm for row c (of product i of a grouped row).  Alignments: 16 for every base the header calls 16-byte aligned
    (R, S, R2, S2, C, the epilogue operands of the persistent kernel, bias, drop_bits, the q/k-norm weights and tables); 8 for the SwiGLU
    operands of the generic kernel; 4 for qkr_rstd."""
    if c["grouped"]:
        M, N = c["grouped"][i]
        K = c["K"]
        return [Op(f"R{i}", K, M, "bf16", 16, field="R", ldfield="ldr", ld=M + PAD), Op(f"S{i}", K, N, "bf16", 16, field="S", ldfield="lds", ld=N + PAD),
                Op(f"C{i}", M, N, "f32", 16, field="C", ldfield="ldc", ld=N if c["split"] > 1 else N + PAD, out=True)]
    M, N, K, K2, e = c["M"], c["N"], c["K"], c["K2"], c["epi"]
    two = lambda name, rows, width, **kw: Op(name, rows, width, "bf16", kw.pop("align", 16), ld=width + PAD, **kw)      # noqa: E731
    r_shape = lambda k: (M, k) if c["rk"] else (k, M)      # noqa: E731
    s_shape = lambda k: (N, k) if c["sk"] else (k, N)      # noqa: E731
    ops = [two("R", *r_shape(K), ldfield="ldr"), two("S", *s_shape(K), ldfield="lds")]
    if K2:
        ops += [two("R2", *r_shape(K2), ldfield="ldr2"), two("S2", *s_shape(K2), ldfield="lds2")]
    c_written = not ({"swiglu_gu", "qkr"} & e)
    ops.append(Op("C", M, N, "f32" if c["f32"] else "bf16", 16, ldfield="ldc", ld=N if c["split"] > 1 else N + PAD, out=True, written=c_written))
    sw = 16 if c["plan"][0] == "persistent" else 8
    if "bias" in e:
        ops.append(Op("bias", 1, N, "f32", 16))
    if "residual" in e:
        ops.append(two("residual", M, N, ldfield="ldres"))
    if "gelu_out" in e:
        ops.append(two("gelu_out", M, N, ldfield="ldg", out=True))
    if "gelu_grad_aux" in e:
        ops.append(two("gelu_grad_aux", M, N, ldfield="ldaux"))
    if "swiglu_gu" in e:
        ops += [two("swiglu_gu", M, 2 * N, ldfield="swiglu_ldgu", align=sw), two("swiglu_dgu", M, 2 * N, ldfield="swiglu_lddgu", align=sw, out=True)]
    if "swiglu_gate" in e:
        ops += [two("swiglu_gate", M, N, ldfield="swiglu_ldgate", align=sw), two("swiglu_act", M, N, ldfield="swiglu_ldact", align=sw, out=True)]
    if c["drop_rank"]:
        nad = K2 // c["drop_rank"]
        ops.append(Op("drop_bits", nad * M, (N + 127) // 128 * 16, "u8", 16))
    if "qkr" in e:
        nq, nk = N // 2, N // 4
        ops += [two("qkr_q", M, nq, ldfield="qkr_ldq", out=True), two("qkr_k", M, nk, ldfield="qkr_ldk", out=True),
                two("qkr_v", M, N - nq - nk, ldfield="qkr_ldv", out=True), Op("qkr_rstd", M, (nq + nk) // 128, "f32", 4, out=True),
                Op("qkr_qw", 1, 128, "f32", 16), Op("qkr_kw", 1, 128, "f32", 16), Op("qkr_cos", QKR_S, 64, "f32", 16), Op("qkr_sin", QKR_S, 64, "f32", 16)]
    if "swp" in e:
        ops.append(two("swp_act", M, N // 2, ldfield="swp_ldact", out=True))
    return ops


QKR_S, QKR_EPS, DROP_P = 256, 1e-6, 0.5


def gemm_struct(c, ptr, i=None):
    """the ur_gemm_args of row c (product i) with the addresses ptr[name]"""
    a = _lib.GemmArgs()
    ops = gemm_operands(c, i)
    for op in ops:
        setattr(a, op.field, ptr[op.name])
        if op.ldfield:
            setattr(a, op.ldfield, op.ld)
    if c["grouped"]:
        a.M, a.N = c["grouped"][i]
    else:
        a.M, a.N, a.K2 = c["M"], c["N"], c["K2"]
    a.K, a.r_kcontig, a.s_kcontig, a.c_f32, a.alpha, a.split_k = c["K"], int(c["rk"]), int(c["sk"]), int(c["f32"]), c["alpha"], c["split"]
    if "swiglu_gu" in c["epi"]:
        a.swiglu_I = c["N"]
    if c["drop_rank"]:
        ld = (c["N"] + 127) // 128 * 16
        a.drop_bits_ld, a.drop_bits_stride, a.drop_rank, a.drop_p = ld, ld * c["M"], c["drop_rank"], DROP_P
    if "qkr" in c["epi"]:
        a.qkr_S, a.qkr_nq_cols, a.qkr_nk_cols, a.qkr_eps = QKR_S, c["N"] // 2, c["N"] // 4, QKR_EPS
    if "swp" in c["epi"]:
        a.swp_I = c["N"] // 2
    return a


def gemm_plan_of(c):
    """ur_gemm_plan's answer for row c on fake pointers, under the row's ur_gemm_persistent_mode: (kernel, tile, epi, mode, gcw, splits)"""
    prev = hip.gemm_persistent_mode(c["pers_mode"])
    try:
        if c["grouped"]:
            arg = [gemm_struct(c, fake_pointers(gemm_operands(c, i)), i) for i in range(len(c["grouped"]))]
        else:
            arg = gemm_struct(c, fake_pointers(gemm_operands(c)))
        pl = hip.gemm_plan(arg)
    finally:
        hip.gemm_persistent_mode(prev)
    return (pl["kernel"], pl["tile"], pl["epi"], pl["mode"], pl["gcw"], pl["splits"])


def gemm_required():
    """{what the table must reach: predicate over a row}"""
    p = lambda c: c["plan"]      # noqa: E731
    plain = lambda c: not c["grouped"] and c["split"] == 1 and not c["drop_rank"] and p(c)[2] == 0      # noqa: E731
    req = {}
    for rk, sk in ((True, True), (True, False), (False, False), (False, True)):
        for f32 in (False, True):
            req[f"generic tile 128, r_kcontig {int(rk)}, s_kcontig {int(sk)}, {'f32' if f32 else 'bf16'} output"] = (
                lambda c, rk=rk, sk=sk, f32=f32: plain(c) and p(c)[:2] == ("generic", 128) and (c["rk"], c["sk"], c["f32"]) == (rk, sk, f32) and c["pers_mode"] == 1)
    for gcw in (0, 4):
        req[f"generic tile 256, gcw {gcw}"] = lambda c, gcw=gcw: p(c)[:2] == ("generic", 256) and p(c)[4] == gcw
    for e in (0, 1, 2):
        req[f"generic epi {e}"] = lambda c, e=e: p(c)[0] == "generic" and p(c)[2] == e
    for t in (128, 256):
        req[f"generic split_k > 1, tile {t}"] = lambda c, t=t: p(c)[:2] == ("generic", t) and p(c)[5] > 1
    for e, m in PERS_INSTANCES:
        req[f"persistent epi {e} mode {m}"] = lambda c, e=e, m=m: p(c)[0] == "persistent" and p(c)[2:4] == (e, m)
    for gcw in (4, 6):
        req[f"persistent gcw {gcw}"] = lambda c, gcw=gcw: p(c)[0] == "persistent" and p(c)[4] == gcw
    for t in (128, 256):
        for s in (False, True):
            req[f"grouped tile {t}, split_k {'> 1' if s else '1'}"] = lambda c, t=t, s=s: p(c)[:2] == ("grouped", t) and (p(c)[5] > 1) == s
    req["masked-LoRA epilogue on the generic kernel at a rank other than 16"] = lambda c: p(c)[0] == "generic" and c["drop_rank"] not in (0, 16)
    for m in (0, 1, 2):
        req[f"ur_gemm_persistent_mode(0) twin of a persistent launch, second-range mode {m}"] = (
            lambda c, m=m: c["pers_mode"] == 0 and p(c)[0] == "generic" and gemm_twin(c)["plan"][0] == "persistent" and gemm_twin(c)["plan"][3] == m)
    return req


def missing(required, table):
    """the requirements no row of `table` meets"""
    return [what for what, pred in required.items() if not any(pred(c) for c in table)]


# =====================================================================================================================================
# LoRA
CU = 256      # the MI355X's compute units: what ur_lora_plan is asked with (the splits of the reduce and the RING1024 rule depend on it)
STAGED_COLS = [(8, 72), (80, 8), (88, 64)]              # a ragged width, the minimum width, no range starts at 0 (tests/lora_cases.py)
RING_COLS = [(0, 64), (64, 128), (192, 64)]
BGRAD_STAGED_COLS = [(8, 72), (80, 64)]
RING_1024_COLS = [(0, 64), (64, 64), (128, 64), (192, 64)]


def L(name, op, M, W, rank, nad, plan, *, cols=None, masked=False, bits_t=False, transposed=False):
    """plan: (kernel, tok_per_block, splits) as ur_lora_plan must answer at CU compute units; op "rmsnorm" / "swiglu": the fused forwards
    (no plan: one kernel each)"""
    return dict(name=name, op=op, M=M, W=W, rank=rank, nad=nad, cols=cols, masked=masked, bits_t=bits_t, transposed=transposed, plan=plan)


def _ring1024_rows():
    """the row count tests/test_gpu_lora_f64.py:test_bgrad_ring_1024 uses: the first row of the block that gives every CU one, + 37"""
    return (CU // 4 - 1) * 1024 + 1 + 37


LORA_CASES = []
for _r in (8, 16, 32, 64):
    # M = 130: two 128-token blocks, the second 2 tokens; W = 72: a 64-column piece and a ragged one
    LORA_CASES.append(L(f"project-staged-r{_r}-n1", "project", 130, 72, _r, 1, ("staged", 128, 1), masked=_r in (8, 32)))
    LORA_CASES.append(L(f"project-staged-r{_r}-n3", "project", 130, 72, _r, 3, ("staged", 128, 1), masked=_r in (16, 64)))
LORA_CASES += [
    L("project-staged-r64-n4", "project", 130, 72, 64, 4, ("staged", 64, 1), masked=True),            # 16 blocks of U: 64 tokens per workgroup
    L("project-ring", "project", 257, 64, 16, 1, ("ring", 256, 1), masked=True),                      # 257 against the ring's 256 tokens
    L("project-ring-ranges", "project", 257, 256, 16, 3, ("ring", 256, 1), cols=RING_COLS),
    L("reduce-staged-1", "reduce", 122, 72, 16, 1, ("staged", 128, 1)),
    L("reduce-staged-1-masked", "reduce", 122, 72, 32, 3, ("staged", 128, 1), masked=True),
    L("reduce-staged-n", "reduce", 130, 72, 8, 3, ("staged", 128, 2)),
    L("reduce-staged-n-masked", "reduce", 130, 72, 16, 1, ("staged", 128, 2), masked=True),
    L("reduce-staged-T", "reduce", 130, 152, 64, 3, ("staged", 128, 2), cols=STAGED_COLS, transposed=True),
    L("reduce-ring-1", "reduce", 128, 64, 16, 1, ("ring", 128, 1)),
    L("reduce-ring-1-masked", "reduce", 128, 64, 16, 3, ("ring", 128, 1), masked=True, bits_t=True),
    L("reduce-ring-n", "reduce", 256, 64, 16, 3, ("ring", 128, 2)),
    L("reduce-ring-n-masked", "reduce", 256, 64, 16, 1, ("ring", 128, 2), masked=True, bits_t=True),
    L("reduce-ring-T", "reduce", 256, 256, 16, 3, ("ring", 128, 2), cols=RING_COLS, transposed=True),
    L("bgrad-staged-r16", "bgrad", 513, 144, 16, 2, ("staged", 512, 2), cols=BGRAD_STAGED_COLS),
    L("bgrad-staged-r64", "bgrad", 257, 144, 64, 2, ("staged", 256, 2), cols=BGRAD_STAGED_COLS),
    L("bgrad-ring", "bgrad", 513, 256, 16, 3, ("ring", 512, 2), cols=RING_COLS),
    L("bgrad-ring1024", "bgrad", _ring1024_rows(), 256, 16, 4, ("ring1024", 1024, CU // 4), cols=RING_1024_COLS),
    L("rmsnorm-lora", "rmsnorm", 130, 1024, 16, 3, None, masked=True),
    L("swiglu-lora", "swiglu", 130, 128, 16, 1, None, masked=True),
]


def lora_plan_of(c):
    """ur_lora_plan's answer for row c at CU compute units, on fake pointers of the stated alignment: X, U, V, G, the bit planes 16, P 8"""
    a = hip.lora_plan_args(c["M"], c["W"], c["rank"], c["nad"], cols=c["cols"], masked=c["masked"], bits_t=c["bits_t"], transposed=c["transposed"], pad=PAD,
                           X=FAKE + 16, P=2 * FAKE + 8, V=3 * FAKE + 16, G=4 * FAKE + 16)
    if c["masked"]:
        a.drop_bits = 5 * FAKE + 16
    if c["bits_t"]:
        a.drop_bits_t = 6 * FAKE + 16
    for e in range(c["nad"]):
        a.U[e] = (7 + e) * FAKE + 16
    pl = hip.lora_plan(c["op"], a, cu_count=CU)
    assert pl["masked"] == (c["masked"] and c["op"] != "bgrad")
    return (pl["kernel"], pl["tok_per_block"], pl["splits"])


def lora_required():
    planned = lambda c, op: c["op"] == op and c["plan"] is not None      # noqa: E731
    req = {}
    for r in (8, 16, 32, 64):
        for n in (1, 3):
            req[f"project STAGED rank {r}, {n} adapter(s) that share X"] = (
                lambda c, r=r, n=n: planned(c, "project") and c["plan"][0] == "staged" and (c["rank"], c["nad"]) == (r, n) and c["cols"] is None)
    for t in (64, 128):
        req[f"project STAGED, {t} tokens per workgroup"] = lambda c, t=t: planned(c, "project") and c["plan"][:2] == ("staged", t)
    req["project RING"] = lambda c: planned(c, "project") and c["plan"][0] == "ring" and c["cols"] is None
    req["project RING over column ranges"] = lambda c: planned(c, "project") and c["plan"][0] == "ring" and c["cols"] is not None
    for k in ("staged", "ring"):
        for many in (False, True):
            for masked in (False, True):
                req[f"reduce {k.upper()}, splits {'> 1' if many else '== 1'}, {'masked' if masked else 'no dropout'}"] = (
                    lambda c, k=k, many=many, masked=masked: planned(c, "reduce") and c["plan"][0] == k and (c["plan"][2] > 1) == many and
                    c["masked"] == masked and not c["transposed"])
        req[f"reduce {k.upper()}, g_transposed 1"] = lambda c, k=k: planned(c, "reduce") and c["plan"][0] == k and c["transposed"]
    req["reduce g_transposed 0"] = lambda c: planned(c, "reduce") and not c["transposed"]
    req["bgrad STAGED"] = lambda c: planned(c, "bgrad") and c["plan"][0] == "staged" and c["rank"] != 64
    req["bgrad STAGED rank 64"] = lambda c: planned(c, "bgrad") and c["plan"][0] == "staged" and c["rank"] == 64
    req["bgrad RING"] = lambda c: planned(c, "bgrad") and c["plan"][0] == "ring"
    req["bgrad RING1024"] = lambda c: planned(c, "bgrad") and c["plan"][0] == "ring1024"
    req["ur_rmsnorm_lora_fwd"] = lambda c: c["op"] == "rmsnorm"
    req["ur_swiglu_lora_fwd"] = lambda c: c["op"] == "swiglu"
    return req


# =====================================================================================================================================
# attention
def A(name, Sq, Sk, nq, nkv, hd, causal, mask, plan, *, p=0.0, modes=(), colsum=False, rope=None, B=2):
    """plan: (fwd, dq, dkv, nw_q, nw_k) as ur_attn_plan must answer under `modes`.  rope: None | "raw" (rope_q_raw = the raw projection) |
    "rstd" (rope_rstd: the roped q) | "rstd_k" (rope_k as well).  mask: a mask kind of tests/attn_cases.py."""
    return dict(name=name, B=B, Sq=Sq, Sk=Sk, nq=nq, nkv=nkv, hd=hd, causal=causal, mask=mask, p=p, modes=tuple(modes), colsum=colsum, rope=rope, plan=plan)


G3, PADS = ("generic",) * 3, (("none",), ("pad", 64))
ATTN_CASES = [
    # Sq = 31, 63, 70 (1, 2, 4 waves of queries) against Sk = 40, 77, 130 (2, 4, 4 waves of keys), and 31 keys for the one-wave dK/dV kernel
    A("generic-31x40-masked-row", 31, 40, 2, 2, 64, False, "full", G3 + (1, 2)),
    A("generic-63x77-hd128-dropout", 63, 77, 2, 2, 128, False, "ragged", G3 + (2, 4), p=0.1),
    A("generic-70x130-dropout", 70, 130, 4, 2, 64, False, "rand", G3 + (4, 4), p=0.5),
    A("generic-70x31", 70, 31, 2, 2, 64, False, "none", G3 + (4, 1)),
    A("generic-causal-gqa-70", 70, 70, 4, 2, 64, True, "left", G3 + (4, 4)),
    A("tiny-3x13", 3, 13, 3, 3, 64, False, "full", ("tiny",) * 3 + (1, 1)),
    A("tiny-3x13-dropout", 3, 13, 3, 3, 64, False, "full", ("tiny",) * 3 + (1, 1), p=0.5),
    A("c128-128-gqa", 128, 128, 4, 2, 128, True, PADS, ("c128",) * 3 + (4, 4)),
    # 2 x 136 (batch, kv head) groups of one 128-key block each: a multiple of 8 above the 256 compute units -- the persistent walk
    A("c128-128-walk", 128, 128, 136, 136, 128, True, PADS, ("c128",) * 3 + (4, 4), modes=(("DKV_PERSIST", 1),)),
    A("c128-128-blocks", 128, 128, 136, 136, 128, True, PADS, ("c128",) * 3 + (4, 4), modes=(("DKV_PERSIST", 0),)),
    A("c128-forward-192", 192, 192, 4, 2, 128, True, "left", ("c128", "generic", "dkv2", 4, 4)),
    A("fewq-33x257-colsum", 33, 257, 2, 2, 64, False, "ragged", ("generic", "generic", "fewq", 2, 4), colsum=True),
    A("fewq-33x257-dropout", 33, 257, 2, 2, 64, False, "ragged", ("generic", "generic", "fewq", 2, 4), p=0.1),
    A("dkv2-31x130", 31, 130, 2, 2, 128, False, "rand", ("generic", "generic", "dkv2", 1, 4)),
    A("rope-raw-70", 70, 70, 4, 2, 128, True, "left", ("generic", "generic", "dkv2", 4, 4), rope="raw"),
    A("rope-rstd-192", 192, 192, 4, 2, 128, True, "left", ("c128", "generic", "dkv2", 4, 4), rope="rstd"),
    A("rope-k-128", 128, 128, 4, 2, 128, True, PADS, ("c128",) * 3 + (4, 4), rope="rstd_k"),
    A("rope-k-192", 192, 192, 4, 2, 128, True, "left", ("c128", "generic", "dkv2", 4, 4), rope="rstd_k"),
]


def attn_lds(c):
    """token strides (elements) of q, k, v, o, dout (16-byte rows: + 8) and of dq, dk, dv (8-byte rows: + 4; dk dense where rope_k runs the
    stand-alone kernel, which wants it so)"""
    NQ, NKV = c["nq"] * c["hd"], c["nkv"] * c["hd"]
    dense_dk = c["rope"] == "rstd_k" and c["plan"][2] != "c128"
    return dict(q=NQ + PAD, k=NKV + PAD, v=NKV + PAD, o=NQ + PAD, dout=NQ + PAD, dq=NQ + 4, dk=NKV if dense_dk else NKV + 4, dv=NKV + 4)


def attn_structs(c, ptr=None):
    """(ur_attn_args, ur_attn_bwd_args) of row c: sizes, strides and flags; ptr {field: address} fills pointers (ur_attn_plan reads none)"""
    a, g = _lib.AttnArgs(), _lib.AttnBwdArgs()
    ld = attn_lds(c)
    a.B, a.Sq, a.Sk, a.nq, a.nkv, a.head_dim, a.causal = c["B"], c["Sq"], c["Sk"], c["nq"], c["nkv"], c["hd"], int(c["causal"])
    a.ldq, a.ldk, a.ldv, a.ldo = ld["q"], ld["k"], ld["v"], ld["o"]
    g.lddo, g.lddq, g.lddk, g.lddv = ld["dout"], ld["dq"], ld["dk"], ld["dv"]
    a.scale, a.dropout_p, a.seed, a.drop_batch0 = c["hd"] ** -0.5, c["p"], ATTN_SEED, ATTN_BATCH0
    for k, v in (ptr or {}).items():
        setattr(a if hasattr(a, k) else g, k, v)
    return a, g


ATTN_SEED, ATTN_BATCH0 = 11, 3


def attn_plan_of(c):
    from tests import attn_cases as ac
    a, g = attn_structs(c, dict(q=FAKE + 16, k=2 * FAKE + 16, v=3 * FAKE + 16, o=4 * FAKE + 16, stats=5 * FAKE + 4, dout=6 * FAKE + 16, dq=7 * FAKE + 8,
                                dk=8 * FAKE + 8, dv=9 * FAKE + 8, delta=10 * FAKE + 4))
    if c["colsum"]:
        g.kv_colsum, g.kv_colsum_ws = 11 * FAKE + 4, 12 * FAKE + 4
    pl = ac.plan_of(a, g, c["modes"])
    return (pl["fwd"], pl["dq"], pl["dkv"], pl["nw_q"], pl["nw_k"])


def attn_walks(c):
    """the generated dK/dV launch of row c is the persistent walk on CU compute units (attn.hip launch_dkv: mode on, (batch, kv head) groups
    a multiple of 8, more key blocks than compute units)"""
    blocks = -(-c["Sk"] // 128) * c["nkv"] * c["B"]
    return c["plan"][2] == "c128" and dict(c["modes"]).get("DKV_PERSIST", 1) != 0 and (c["nkv"] * c["B"]) % 8 == 0 and blocks > CU


def attn_required():
    p = lambda c: c["plan"]      # noqa: E731
    plain = lambda c: c["rope"] is None      # noqa: E731
    req = {}
    for nw in (1, 2, 4):
        req[f"forward GENERIC, nw_q {nw}"] = lambda c, nw=nw: p(c)[0] == "generic" and p(c)[3] == nw
        req[f"dK/dV GENERIC, nw_k {nw}"] = lambda c, nw=nw: p(c)[2] == "generic" and p(c)[4] == nw
    for k in ("tiny", "c128"):
        req[f"forward {k.upper()}"] = lambda c, k=k: p(c)[0] == k
    for k in ("tiny", "c128", "generic"):
        req[f"dQ {k.upper()}"] = lambda c, k=k: p(c)[1] == k
    for k in ("tiny", "c128", "dkv2"):
        req[f"dK/dV {k.upper()}"] = lambda c, k=k: p(c)[2] == k and plain(c)
    req["dK/dV FEWQ with kv_colsum"] = lambda c: p(c)[2] == "fewq" and c["colsum"]
    req["dK/dV DKV2, non-causal"] = lambda c: p(c)[2] == "dkv2" and not c["causal"]
    req["forward C128 feeding the generic dQ and DKV2"] = lambda c: p(c)[:3] == ("c128", "generic", "dkv2") and plain(c)
    req["UR_ATTN_MODE_DKV_PERSIST 1: the persistent walk"] = lambda c: attn_walks(c)
    req["UR_ATTN_MODE_DKV_PERSIST 0 on the same launch"] = (
        lambda c: p(c)[2] == "c128" and dict(c["modes"]).get("DKV_PERSIST") == 0 and attn_walks(dict(c, modes=())))
    req["dropout on: generic head_dim 64"] = lambda c: c["p"] > 0 and p(c)[:3] == G3 and c["hd"] == 64
    req["dropout on: generic head_dim 128"] = lambda c: c["p"] > 0 and p(c)[:3] == G3 and c["hd"] == 128
    req["dropout on: tiny"] = lambda c: c["p"] > 0 and p(c)[0] == "tiny"
    req["dropout on: few-query dK/dV"] = lambda c: c["p"] > 0 and p(c)[2] == "fewq"
    req["dropout off: tiny"] = lambda c: c["p"] == 0 and p(c)[0] == "tiny"
    req["causal with GQA 4:2, generic kernels"] = lambda c: c["causal"] and (c["nq"], c["nkv"]) == (4, 2) and p(c)[:3] == G3 and plain(c)
    req["causal with GQA 4:2, generated pair"] = lambda c: c["causal"] and (c["nq"], c["nkv"]) == (4, 2) and p(c)[:3] == ("c128",) * 3 and plain(c)
    req["a key mask with one fully masked row"] = lambda c: c["mask"] == "full" and p(c)[:3] == G3
    req["one wave of keys against four of queries"] = lambda c: p(c)[3:] == (4, 1)
    req["rope_q_raw: the raw projection"] = lambda c: c["rope"] == "raw"
    req["rope_rstd: the roped q"] = lambda c: c["rope"] == "rstd"
    req["rope_k on the generated pair"] = lambda c: c["rope"] == "rstd_k" and p(c)[2] == "c128"
    req["rope_k off the generated pair"] = lambda c: c["rope"] == "rstd_k" and p(c)[2] != "c128"
    return req

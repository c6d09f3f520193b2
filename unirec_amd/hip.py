"""Tensor-level wrappers over the C ABI (include/unirec_hip.h and the family headers beside it).

PyTorch is plumbing here: it owns device memory and the current HIP stream; every computation is a
call into libunirec_hip.so with raw ``data_ptr()``s.  All functions require CUDA(HIP) tensors and
raise on anything else -- there is no eager fallback.
"""
import ctypes

import torch

from . import _lib
from ._lib import AttnArgs, AttnBwdArgs, AttnPlanInfo, CatalogSelect, GemmArgs, GemmPlanInfo, LoraArgs, LoraPlanInfo, check

BF16 = torch.bfloat16
F32 = torch.float32


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_get_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """The current HIP stream of the current device as an integer handle.  (torch.cuda.current_stream() builds a Stream object per
    call: 2.7 us, on every one of the ~870 launches of an item-stage step; the raw query is 0.3 us.)"""
    if _raw_stream is not None and _get_device is not None:
        return _raw_stream(_get_device())
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


def _need(t, dtype, name):
    if not t.is_cuda:
        raise _lib.UniRecHipError(f"{name}: expected a device tensor (the UniRec HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous tensor")


_ws_cache = {}

# Optional live kernel timing (bench.py roofline leg): when PROFILE is a list, every ur_gemm launch is
# bracketed by HIP events recorded on the launching (current) stream and logged with its shape.
PROFILE = None
PROFILE_STREAM = None   # bench.py: list of (event0, event1, family, algorithmic bytes) around the HBM-bound launches wrapped by _stream_family
PROFILE_ATTN = None     # bench.py: list of (event0, event1, 'fwd' | 'bwd', B, Sq, Sk, nq, head_dim, causal) around every attention launch


def _stream_family(family, nbytes):
    """Decorator for a wrapper of an HBM-bound launch: when PROFILE_STREAM is a list (bench.py's roofline leg) HIP events on the
    launching stream bracket the call and (events, family, ALGORITHMIC bytes = every operand read / written once) is appended.
    nbytes(result, *args, **kwargs) -> bytes."""
    import functools

    def deco(fn):
        @functools.wraps(fn)
        def wrapped(*a, **k):
            if PROFILE_STREAM is None:
                return fn(*a, **k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **k)
            e1.record()
            PROFILE_STREAM.append((e0, e1, family, int(nbytes(r, *a, **k))))
            return r
        return wrapped
    return deco


def _nb(*ts):
    return sum(t.numel() * t.element_size() for t in ts if t is not None and hasattr(t, "numel"))


def workspace(nbytes, device, tag="default"):
    """Grow-only scratch buffer per (device, tag, STREAM); owned by the caller side (torch allocator).  Per stream since round 6: launches of
    one family run on two streams at once (the Q-Formers' weight-gradient reductions on their side stream beside the dX chain), and a scratch
    buffer shared across streams would be a race (the C3 full-size determinism test caught exactly that)."""
    key = (device, tag, _stream() if device.type == "cuda" else 0)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


# ------------------------------------------------------------------------------------------------
GEMM_MAX_GROUPS = 8
GEMM_KERNELS = ("none", "generic", "persistent", "grouped")      # index = UR_GEMM_KERNEL_* (include/unirec_hip.h)
_ADDR = 4096      # an aligned non-null address: what the selection queries put where a launch has a tensor (they follow no pointer)


def _operand(t, what, shape=None):
    if t.dtype != BF16 or not t.is_cuda or t.dim() != 2 or t.stride(1) != 1 or (shape is not None and tuple(t.shape) != shape[0]):
        raise ValueError(f"{what} must be a {'2-D bf16' if shape is None else 'bf16 ' + shape[1]} device tensor with unit inner stride")


def _gemm_args(R, ldr, S, lds, C, ldc, M, N, K, r_kcontig=1, s_kcontig=1, c_f32=0, alpha=1.0, split_k=1, pair2=None):
    """The operand and output fields of a GemmArgs from addresses and row strides; pair2 = (R2, ldr2, S2, lds2, K2)."""
    a = GemmArgs()
    a.R, a.ldr, a.r_kcontig = R, ldr, int(r_kcontig)
    a.S, a.lds, a.s_kcontig = S, lds, int(s_kcontig)
    a.C, a.ldc, a.c_f32 = C, ldc, int(c_f32)
    a.M, a.N, a.K, a.alpha, a.split_k = M, N, K, float(alpha), int(split_k)
    if pair2 is not None:
        a.R2, a.ldr2, a.S2, a.lds2, a.K2 = pair2
    return a


def _pair2(R2, S2, r_kcontig=True):
    return None if R2 is None else (R2.data_ptr(), R2.stride(0), S2.data_ptr(), S2.stride(0), R2.shape[1] if r_kcontig else R2.shape[0])


def _launch(fn, what, args, entry):
    """check(fn(*args, stream)); when PROFILE is a list (bench.py's roofline leg) HIP events on the launching stream bracket the call
    and (e0, e1, *entry()) is appended."""
    if PROFILE is None:
        return check(fn(*args, _stream()), what)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(fn(*args, _stream()), what)
    e1.record()
    PROFILE.append((e0, e1, *entry()))


def gemm(R, S, *, r_kcontig=True, s_kcontig=True, M=None, N=None, K=None, out=None, out_f32=False, alpha=1.0,
         bias=None, residual=None, gelu_out=None, gelu_grad_aux=None, R2=None, S2=None, split_k=1, drop=None,
         swiglu_bwd=None, swiglu_fwd=None, swiglu_paired=None):
    """C[M,N] = alpha*(R(m,k) S(n,k) + R2 S2) + epilogue.  R/S are 2-D bf16 (row stride = stride(0)).
    drop = (bits, p, rank): masked LoRA epilogue (bits = hip.lora_dropout_bits planes of the adapters' shared input),
    swiglu_bwd = (gu, dgu): the result is d(act) of SwiGLU; dgate | dup are written to dgu [M, 2N] and no C is produced
    (returns dgu).  swiglu_fwd = (gate, act): C is up(x) as usual and act[M, N] = silu(gate) * C is written beside it.
    swiglu_paired = act [M, N/2]: the merged gate|up projection with 128-row interleaved weight rows (swiglu_pair_rows); C is
    gate | up in the standard order and act = silu(gate) * up leaves beside it (persistent kernel only: gemm_swiglu_paired_supported).
    See ur_gemm_args in include/unirec_hip.h."""
    lib = _lib.load()
    _operand(R, "gemm: R")
    _operand(S, "gemm: S")
    if M is None:
        M = R.shape[0] if r_kcontig else R.shape[1]
    if N is None:
        N = S.shape[0] if s_kcontig else S.shape[1]
    if K is None:
        K = R.shape[1] if r_kcontig else R.shape[0]
    Ks = S.shape[1] if s_kcontig else S.shape[0]
    if Ks != K:
        raise ValueError(f"gemm: K mismatch R:{K} S:{Ks}")
    if swiglu_bwd is not None:
        gu_, dgu_ = swiglu_bwd
        _operand(gu_, "gemm: swiglu_bwd gu", ((M, 2 * N), "[M, 2N]"))
        _operand(dgu_, "gemm: swiglu_bwd dgu", ((M, 2 * N), "[M, 2N]"))
        out = dgu_            # C is not written in this mode; any valid bf16 pointer with ldc >= N
    if out is None:
        out = torch.empty((M, N), dtype=F32 if out_f32 else BF16, device=R.device)
    f32 = int(out.dtype == F32)
    a = _gemm_args(R.data_ptr(), R.stride(0), S.data_ptr(), S.stride(0), out.data_ptr(), out.stride(0), M, N, K, r_kcontig, s_kcontig, f32,
                   alpha, split_k, _pair2(R2, S2, r_kcontig))
    a.bias = _p(bias)
    if residual is not None:
        a.residual, a.ldres = residual.data_ptr(), residual.stride(0)
    if gelu_out is not None:
        a.gelu_out, a.ldg = gelu_out.data_ptr(), gelu_out.stride(0)
    if gelu_grad_aux is not None:
        a.gelu_grad_aux, a.ldaux = gelu_grad_aux.data_ptr(), gelu_grad_aux.stride(0)
    if swiglu_bwd is not None:
        a.swiglu_gu, a.swiglu_ldgu = gu_.data_ptr(), gu_.stride(0)
        a.swiglu_dgu, a.swiglu_lddgu, a.swiglu_I = dgu_.data_ptr(), dgu_.stride(0), N
    if swiglu_fwd is not None:
        gate_, act_ = swiglu_fwd
        _operand(gate_, "gemm: swiglu_fwd gate", ((M, N), "[M, N]"))
        _operand(act_, "gemm: swiglu_fwd act", ((M, N), "[M, N]"))
        a.swiglu_gate, a.swiglu_ldgate, a.swiglu_act, a.swiglu_ldact = gate_.data_ptr(), gate_.stride(0), act_.data_ptr(), act_.stride(0)
    if swiglu_paired is not None:
        _operand(swiglu_paired, "gemm: swiglu_paired act", ((M, N // 2), "[M, N/2]"))
        a.swp_act, a.swp_ldact, a.swp_I = swiglu_paired.data_ptr(), swiglu_paired.stride(0), N // 2
    if drop is not None:
        bits, pdrop, rank = drop
        a.drop_bits, a.drop_bits_ld, a.drop_bits_stride = bits.data_ptr(), bits.stride(1), bits.stride(0)
        a.drop_p, a.drop_rank = float(pdrop), int(rank)
    ws, wsb = 0, 0
    if split_k > 1:
        wsb = lib.ur_gemm_workspace_bytes(ctypes.byref(a))
        ws = workspace(wsb, R.device, "gemm").data_ptr()
    _launch(lib.ur_gemm, "ur_gemm", (ctypes.byref(a), ws, wsb),
            lambda: (int(r_kcontig), int(s_kcontig), f32, M, N, K + int(a.K2), int(split_k),
                     1 if swiglu_bwd is not None else (2 if swiglu_fwd is not None else (4 if swiglu_paired is not None else 0))))
    return out


def qkrope_perm(head_dim=128):
    """Feature stored at tile column c of a head under the paired row order of the fused q|k|v + q/k-norm + RoPE launch
    (ur_qkrope_perm, include/unirec_hip.h): index tensor `perm` with W_paired[h * 128 + c] = W[h * 128 + perm[c]]."""
    if head_dim != 128:
        raise ValueError("the fused q/k-norm + RoPE epilogue is built for head_dim 128")
    lib = _lib.load()
    return torch.tensor([lib.ur_qkrope_perm(c) for c in range(128)], dtype=torch.long)


def swiglu_pair_rows(I):
    """Row order of the merged gate|up weight (and of its LoRA B operand) for the paired SwiGLU epilogue: blocks of 128 gate rows
    alternate with the 128 up rows of the same features -- index tensor `rows` with W_paired = W[rows], W = [gate; up] [2 I, K]."""
    t = torch.arange(I // 128)[:, None, None] * 128 + torch.arange(128)[None, None, :]          # [I/128, 1, 128]
    return torch.cat([t, t + I], dim=1).reshape(-1)


def gemm_grouped(products, split_k=1):
    """ur_gemm_grouped: products = [(R [K, M], S [K, N], out f32 [M, N]), ...] (1..8 token-major pairs: out_i = R_i^T S_i over the shared
    token axis K) as ONE launch -- the weight gradients of one Q-Former layer.  Every out_i is written (split_k > 1: through the
    per-stream workspace and one grouped reduction)."""
    lib = _lib.load()
    n = len(products)
    if not 1 <= n <= GEMM_MAX_GROUPS:
        raise ValueError(f"gemm_grouped: 1 .. {GEMM_MAX_GROUPS} products per launch (got {n})")
    arr = (GemmArgs * n)()
    for i, (R, S, out) in enumerate(products):
        _operand(R, "gemm_grouped: R")
        _operand(S, "gemm_grouped: S")
        if R.shape[0] != S.shape[0]:
            raise ValueError(f"gemm_grouped: token counts differ ({R.shape[0]} vs {S.shape[0]})")
        if not out.is_cuda:
            raise _lib.UniRecHipError("gemm_grouped: out: expected a device tensor (the UniRec HIP path has no CPU fallback)")
        # (a row stride above the row length is the library's to judge: ur_gemm_grouped takes it without split_k and refuses it with)
        if out.dtype != F32 or out.dim() != 2 or tuple(out.shape) != (R.shape[1], S.shape[1]) or out.stride(1) != 1:
            raise ValueError(f"gemm_grouped: out must be f32 [{R.shape[1]}, {S.shape[1]}] with unit inner stride, got {out.dtype} {tuple(out.shape)}")
        arr[i] = _gemm_args(R.data_ptr(), R.stride(0), S.data_ptr(), S.stride(0), out.data_ptr(), out.stride(0), R.shape[1], S.shape[1], R.shape[0],
                            0, 0, 1, 1.0, split_k)
    ws, wsb = 0, 0
    if split_k > 1:
        wsb = lib.ur_gemm_grouped_workspace_bytes(arr, n)
        ws = workspace(wsb, products[0][0].device, "gemm_grouped").data_ptr()

    def entry():
        # (one entry for the launch: M = the products' output rows summed at the widest N -- FLOP-exact only for equal N; see flops below)
        fl = sum(2.0 * R.shape[0] * R.shape[1] * S.shape[1] for R, S, _ in products)
        K = products[0][0].shape[0]
        N = max(S.shape[1] for _, S, _ in products)
        return 0, 0, 1, int(round(fl / (2.0 * K * N))), N, K, int(split_k), 0
    _launch(lib.ur_gemm_grouped, "ur_gemm_grouped", (arr, n, ws, wsb), entry)


def gemm_plan_args(M, N, K, K2=0, *, r_kcontig=True, s_kcontig=True, out_f32=False, split_k=1, alpha=1.0, ldc=None, drop_rank=0, **ptrs):
    """A GemmArgs of these sizes for the selection queries: dense rows, and _ADDR in C and in every pointer field named in ptrs
    (bias=True, swiglu_gu=True, ...; C=address sets another one)."""
    pair2 = (_ADDR, K2 if r_kcontig else M, _ADDR, K2 if s_kcontig else N, K2) if K2 else None
    a = _gemm_args(_ADDR, K if r_kcontig else M, _ADDR, K if s_kcontig else N, _ADDR, N if ldc is None else ldc, M, N, K, r_kcontig, s_kcontig,
                   out_f32, alpha, split_k, pair2)
    a.ldres = a.ldg = a.ldaux = a.swiglu_ldgate = a.swiglu_ldact = a.swiglu_I = N
    a.swiglu_ldgu = a.swiglu_lddgu = 2 * N
    if drop_rank:
        a.drop_bits, a.drop_bits_ld, a.drop_bits_stride, a.drop_rank, a.drop_p = _ADDR, (N + 127) // 128 * 16, (N + 127) // 128 * 16 * M, drop_rank, 0.5
    for name, v in ptrs.items():
        setattr(a, name, _ADDR if v is True else int(v))
    return a


def gemm_plan(a, *sizes, **flags):
    """Which kernel ur_gemm / ur_gemm_grouped launches and how, under the current gemm_persistent_mode (ur_gemm_plan): a dict with
    kernel (a name from GEMM_KERNELS), tile, epi, mode, gcw and splits.  a: a GemmArgs (ur_gemm), a sequence of them (ur_gemm_grouped),
    or M followed by N, K[, K2] and the keywords of gemm_plan_args.  No tensor and no device is needed.  Raises UniRecHipError where the
    entry point would refuse the arguments."""
    if isinstance(a, int):
        a = gemm_plan_args(a, *sizes, **flags)
    count = 0 if isinstance(a, GemmArgs) else len(a)
    out = GemmPlanInfo()
    check(_lib.load().ur_gemm_plan((GemmArgs * count)(*a) if count else ctypes.byref(a), count, ctypes.byref(out)), "ur_gemm_plan")
    return dict(kernel=GEMM_KERNELS[out.kernel], tile=int(out.tile), epi=int(out.epi), mode=int(out.mode), gcw=int(out.gcw), splits=int(out.splits))


def gemm_swiglu_paired_supported(M, I, K, K2, device=None):
    """True when the merged gate|up projection of these sizes can carry the SwiGLU forward in its epilogue (`device` is not needed)."""
    a = gemm_plan_args(M, 2 * I, K, K2, swp_act=True, swp_ldact=I, swp_I=I)
    return bool(_lib.load().ur_gemm_swiglu_paired_supported(ctypes.byref(a)))


def gemm_qkrope_supported(M, N, K, K2, Sseq, nq_cols, nk_cols, device=None, alpha=1.0, bias=None):
    """True when the q|k|v projection of these sizes can carry q/k-norm + RoPE in its epilogue (ur_gemm_qkrope_supported); alpha / bias
    (f32 [N]) fill the fields of ur_gemm_args the epilogue does not take, for which the answer is no.  `device` is not needed."""
    a = gemm_plan_args(M, N, K, K2, alpha=alpha, bias=bias is not None, qkr_q=True, qkr_k=True, qkr_v=True, qkr_rstd=True, qkr_qw=True, qkr_kw=True,
                   qkr_cos=True, qkr_sin=True, qkr_ldq=nq_cols, qkr_ldk=nk_cols, qkr_ldv=N - nq_cols - nk_cols, qkr_S=Sseq, qkr_nq_cols=nq_cols,
                   qkr_nk_cols=nk_cols)
    return bool(_lib.load().ur_gemm_qkrope_supported(ctypes.byref(a)))


def gemm_qkv_rope(R, S, qw, kw, cos, sin, Sseq, nq_cols, nk_cols, eps, R2=None, S2=None, out=None):
    """The merged q|k|v projection with q/k-norm + RoPE in its epilogue (ur_gemm_args.qkr_*): R [M,K] activations, S [N,K]
    weights whose q / k head rows are in the paired order (qkrope_perm), optional LoRA pair (S2 rows paired likewise).
    Returns (q_r [M,nq_cols], k_r [M,nk_cols], v [M,N-nq-nk], rstd [M,(nq+nk)/128]); the raw q, k are never stored.
    out = (q, k, v, rstd): write there instead -- q / k / v bf16 of those shapes with unit inner stride and ANY row stride >= the width
    (column views of wider buffers: qkr_ldq / ldk / ldv), rstd contiguous f32."""
    lib = _lib.load()
    M, N, K = R.shape[0], S.shape[0], R.shape[1]
    dev = R.device
    shapes = ((M, nq_cols), (M, nk_cols), (M, N - nq_cols - nk_cols), (M, (nq_cols + nk_cols) // 128))
    if out is None:
        outs = tuple(torch.empty(sh, dtype=F32 if i == 3 else BF16, device=dev) for i, sh in enumerate(shapes))
    else:
        outs = tuple(out)
        if len(outs) != 4:
            raise ValueError("gemm_qkv_rope: out must be (q, k, v, rstd)")
        for i, (t, sh, nm) in enumerate(zip(outs, shapes, ("q", "k", "v", "rstd"))):
            if t.dtype != (F32 if i == 3 else BF16) or not t.is_cuda or tuple(t.shape) != sh or t.stride(1) != 1 or (i == 3 and not t.is_contiguous()):
                raise ValueError(f"gemm_qkv_rope: out {nm} must be a {'contiguous f32' if i == 3 else 'bf16'} {sh} device tensor with unit inner stride")
    q, k, v, rstd = outs
    # (C is not written in this mode: any valid pointer)
    a = _gemm_args(R.data_ptr(), R.stride(0), S.data_ptr(), S.stride(0), q.data_ptr(), q.stride(0), M, N, K, pair2=_pair2(R2, S2))
    a.qkr_q, a.qkr_ldq, a.qkr_k, a.qkr_ldk, a.qkr_v, a.qkr_ldv = q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0)
    a.qkr_rstd, a.qkr_qw, a.qkr_kw, a.qkr_cos, a.qkr_sin = rstd.data_ptr(), qw.data_ptr(), kw.data_ptr(), cos.data_ptr(), sin.data_ptr()
    a.qkr_S, a.qkr_nq_cols, a.qkr_nk_cols, a.qkr_eps = int(Sseq), int(nq_cols), int(nk_cols), float(eps)
    _launch(lib.ur_gemm, "ur_gemm(qkrope)", (ctypes.byref(a), 0, 0), lambda: (1, 1, 0, M, N, K + int(a.K2), 1, 3))
    return outs


@_stream_family("qknorm_rope_bwd", lambda r, dq_out, dk_out, q_r, k_r, rstd, qw, kw, cos, sin, dqkv_raw, S, nq, nkv, hd:
                3 * (_nb(k_r) if dq_out is None else _nb(q_r, k_r)))      # gradient in, roped output in, raw gradient out
def qknorm_rope_bwd_roped(dq_out, dk_out, q_r, k_r, rstd, qw, kw, cos, sin, dqkv_raw, S, nq, nkv, hd):
    """Backward of the fused q|k|v epilogue: dq|dk raw into dqkv_raw[:, :(nq+nkv)*hd] from the ROPED forward outputs + rstd."""
    lib = _lib.load()
    M = q_r.shape[0]
    check(lib.ur_qknorm_rope_bwd_roped(dq_out.data_ptr(), dk_out.data_ptr(), q_r.data_ptr(), q_r.stride(0), k_r.data_ptr(), k_r.stride(0),
                                       rstd.data_ptr(), qw.data_ptr(), kw.data_ptr(), cos.data_ptr(), sin.data_ptr(), dqkv_raw.data_ptr(),
                                       dqkv_raw.stride(0), M, S, nq, nkv, hd, _stream()), "ur_qknorm_rope_bwd_roped")
    return dqkv_raw


@_stream_family("qknorm_rope_bwd", lambda r, dk_out, k_r, rstd, h0, kw, cos, sin, dk_raw, S, nkv, hd: 3 * _nb(dk_out))      # gradient in, roped k in, raw gradient out
def qknorm_rope_bwd_roped_k(dk_out, k_r, rstd, h0, kw, cos, sin, dk_raw, S, nkv, hd):
    """The k heads of qknorm_rope_bwd_roped alone (the q heads rode in the dQ kernel: attn_bwd(..., rope_rstd=...)): dk_raw [M, >= nkv*hd]
    view receives the gradient of the raw k projection; 1 / rms of (m, k head h) = rstd[m, h0 + h]."""
    lib = _lib.load()
    M = k_r.shape[0]
    check(lib.ur_qknorm_rope_bwd_roped_k(dk_out.data_ptr(), k_r.data_ptr(), k_r.stride(0), rstd.data_ptr(), rstd.stride(0), int(h0), kw.data_ptr(),
                                         cos.data_ptr(), sin.data_ptr(), dk_raw.data_ptr(), dk_raw.stride(0), M, S, nkv, hd, _stream()),
          "ur_qknorm_rope_bwd_roped_k")
    return dk_raw


ATTN_MODE_TINY, ATTN_MODE_C128, ATTN_MODE_DKV_PERSIST, ATTN_MODE_FEWQ = 0, 1, 2, 3      # include/unirec_hip.h: UR_ATTN_MODE_*
ATTN_KERNELS = ("none", "generic", "tiny", "c128", None, "dkv2", "fewq")                 # index = UR_ATTN_KERNEL_* (4: retired id)


def attn_mode(key, value):
    """Kernel selection of the attention entry points (ur_attn_mode, include/unirec_hip.h): sets the process-wide word `key` and returns
    the previous value; value -1 = default, -2 = query only."""
    prev = int(_lib.load().ur_attn_mode(int(key), int(value)))
    if prev < 0:
        raise ValueError(f"ur_attn_mode: unknown key {key}")
    return prev


class attn_mode_set:
    """with hip.attn_mode_set(hip.ATTN_MODE_C128, 0): ...   -- the word is restored on exit (tests, A/B timing)"""

    def __init__(self, key, value):
        self.key, self.value = key, value

    def __enter__(self):
        self.prev = attn_mode(self.key, self.value)
        return self

    def __exit__(self, *exc):
        attn_mode(self.key, self.prev)
        return False


def gemm_persistent_mode(mode):
    """0 = generic GEMM kernel only, 1 = persistent kernel where eligible, -1 = default; returns the previous setting
    (ur_gemm_persistent_mode, include/unirec_hip.h)."""
    return int(_lib.load().ur_gemm_persistent_mode(int(mode)))


# ---- LoRA adapter products (ranks 8, 16, 32, 64): include/unirec_hip.h, csrc/lora.hip ---------------
LORA_RANKS = (8, 16, 32, 64)      # what ur_lora_project / ur_lora_reduce / ur_lora_bgrad are built for


def _lora_rank(r, who):
    if int(r) not in LORA_RANKS:
        raise ValueError(f"{who}: LoRA rank {int(r)} is not supported (supported ranks: {', '.join(map(str, LORA_RANKS))})")
    return int(r)


def lora_bits_ld(W):
    return int(_lib.load().ur_lora_bits_ld(int(W)))


def lora_bits_t_ld(W):
    return int(_lib.load().ur_lora_bits_t_ld(int(W)))


@_stream_family("lora_bits", lambda r, *a, **k: _nb(r))
def lora_dropout_bits(seed, p, M, W, nad, device, out=None, row0=0):
    """Dropped-flag bit planes uint8 [nad, M, ur_lora_bits_ld(W)] of nad adapters that share an [M, W] input.  row0: rows that
    precede row 0 in the global minibatch (a data-parallel rank draws the flags of ITS rows)."""
    lib = _lib.load()
    ld = int(lib.ur_lora_bits_ld(int(W)))
    bits = torch.empty((nad, M, ld), dtype=torch.uint8, device=device) if out is None else out
    check(lib.ur_lora_dropout_bits(int(seed), float(p), int(M), int(W), int(nad), bits.data_ptr(), ld, bits.stride(0), int(row0), _stream()),
          "ur_lora_dropout_bits")
    return bits


def lora_bits_transpose(bits, W, out=None):
    """Token-packed copy int32 [nad, M / 32, ur_lora_bits_t_ld(W)] of the dropped-flag planes (ur_lora_bits_transpose): what the token
    reduction (lora_reduce(..., bits_t=...)) masks its transposed fragments with.  M % 32 == 0."""
    lib = _lib.load()
    nad, M, ld = bits.shape
    if M % 32:
        raise ValueError("lora_bits_transpose: M must be a multiple of 32")
    ldt = int(lib.ur_lora_bits_t_ld(int(W)))
    bt = torch.empty((nad, M // 32, ldt), dtype=torch.int32, device=bits.device) if out is None else out
    check(lib.ur_lora_bits_transpose(bits.data_ptr(), ld, bits.stride(0), int(M), int(W), int(nad), bt.data_ptr(), ldt, bt.stride(0), _stream()),
          "ur_lora_bits_transpose")
    return bt


def lora_bits_to_keep(bits, W):
    """Unpack bit planes into keep masks uint8 [nad, M, W] (1 = kept) -- test / inspection helper (torch ops)."""
    nad, M, ld = bits.shape
    b = bits.to(torch.int32)
    pos = torch.tensor([0, 4, 1, 5, 2, 6, 3, 7], device=bits.device, dtype=torch.int32)     # element e of a byte -> bit
    dropped = (b.unsqueeze(-1) >> pos) & 1
    return (1 - dropped).reshape(nad, M, ld * 8)[:, :, :W].to(torch.uint8)


def _lora_fill(X, cols, shared, bits, alpha, rank, U=(), P=None, V=None, G=None, transposed=False, bits_t=None):
    """The LoraArgs of a launch -- what lora_project, lora_reduce, lora_bgrad, the fused kernels and lora_plan_args all fill.  X: the 2-D
    bf16 device tensor, or (address, ld, M) for the selection query; bits: the planes' tensor, or (address, ld, plane stride); U: a
    sequence of (address, ld); P, V: (address, ld); G: an address; bits_t: (address, ld, plane stride)."""
    a = LoraArgs()
    if isinstance(X, tuple):
        a.X, a.ldx, a.M = X
    elif X.dtype != BF16 or not X.is_cuda or X.dim() != 2 or X.stride(1) != 1:
        raise ValueError("lora: X must be a 2-D bf16 device tensor with unit inner stride")
    else:
        a.X, a.ldx, a.M = X.data_ptr(), X.stride(0), X.shape[0]
    a.nad, a.rank, a.shared = len(cols), int(rank), int(shared)
    for e, (c0, w) in enumerate(cols):
        a.col0[e], a.width[e] = int(c0), int(w)
    if bits is not None:
        a.drop_bits, a.bits_ld, a.bits_stride = bits if isinstance(bits, tuple) else (bits.data_ptr(), bits.stride(1), bits.stride(0))
    if bits_t is not None:
        a.drop_bits_t, a.bits_t_ld, a.bits_t_stride = bits_t
    a.alpha = float(alpha)
    for e, (u, ldu) in enumerate(U):
        a.U[e], a.ldu[e] = u, ldu
    if P is not None:
        a.P, a.ldp = P
    if V is not None:
        a.V, a.ldv = V
    if G is not None:
        a.G, a.g_transposed = G, int(transposed)
    return a


LORA_OPS = ("project", "reduce", "bgrad")                        # index = UR_LORA_OP_* (include/unirec_hip.h)
LORA_KERNELS = ("none", "staged", "ring", "ring1024")            # index = UR_LORA_KERNEL_*


def lora_plan_args(M, W=None, rank=16, nad=1, *, cols=None, masked=False, bits_t=False, transposed=False, pad=0, alpha=1.0, **fields):
    """A LoraArgs of these sizes for the selection query: nad adapters that share an [M, W] input, or cols=[(c0, width), ...] column
    ranges; dense rows (+ pad columns) and _ADDR wherever a launch has a tensor -- X, every U, P, V, G, and the dropout planes with
    masked / bits_t.  fields: LoraArgs fields set last (drop_bits_t=_ADDR + 4, bits_t_ld=..., shared=1 ...)."""
    shared = cols is None
    if shared:
        cols = [(0, W)] * nad
    ldx = max(c0 + w for c0, w in cols) + pad if cols else pad
    Wb = cols[0][1] if cols else 0
    ld, ldt = (Wb + 127) // 128 * 16, (Wb + 3) // 4 * 4          # ur_lora_bits_ld, ur_lora_bits_t_ld of the shared input
    a = _lora_fill((_ADDR, ldx, M), cols, shared, (_ADDR, ld, ld * M) if masked else None, alpha, rank,
                   U=[(_ADDR, w) for _, w in cols], P=(_ADDR, rank * len(cols)), V=(_ADDR, rank * len(cols)),
                   G=_ADDR, transposed=transposed, bits_t=(_ADDR, ldt, ldt * ((M + 31) // 32)) if masked and bits_t else None)
    for name, v in fields.items():
        setattr(a, name, v)
    return a


def lora_plan(op, a, *sizes, cu_count=0, **kw):
    """Which kernel ur_lora_project / ur_lora_reduce / ur_lora_bgrad (op: a name from LORA_OPS) launches and how (ur_lora_plan): a dict
    with kernel (a name from LORA_KERNELS), masked, nad_k, blocks, half, splits, tok_per_block, grid, lds_bytes and workspace_bytes.
    a: a LoraArgs, or M followed by the arguments of lora_plan_args.  cu_count = 0: the current device's (256 without one).  No tensor
    and no device is needed.  Raises UniRecHipError where the entry point would refuse the arguments."""
    if not isinstance(a, LoraArgs):
        a = lora_plan_args(a, *sizes, **kw)
    out = LoraPlanInfo()
    check(_lib.load().ur_lora_plan(LORA_OPS.index(op) if op in LORA_OPS else int(op), ctypes.byref(a), int(cu_count), ctypes.byref(out)), "ur_lora_plan")
    return dict(kernel=LORA_KERNELS[out.kernel], masked=bool(out.masked), nad_k=int(out.nad_k), blocks=int(out.blocks), half=bool(out.half),
                splits=int(out.splits), tok_per_block=int(out.tok_per_block), grid=(int(out.grid_x), int(out.grid_y), int(out.grid_z)),
                lds_bytes=int(out.lds_bytes), workspace_bytes=int(out.workspace_bytes))


def _cols_bytes(X, cols):
    return X.shape[0] * 2 * (X.shape[1] if cols is None else sum(w for _, w in cols))


def lora_project_args(X, U, cols=None, alpha=1.0, bits=None, out=None):
    """(the LoraArgs of lora_project for these tensors, out) -- what the launch passes and what lora_plan("project", ...) is asked with"""
    shared = cols is None
    if shared:
        cols = [(0, X.shape[1])] * len(U)
    r = _lora_rank(U[0].shape[0], "lora_project")
    for e, u in enumerate(U):
        if u.dtype != BF16 or u.dim() != 2 or u.shape[0] != r or u.stride(1) != 1 or u.shape[1] != cols[e][1]:
            raise ValueError(f"lora_project: U[a] must be bf16 [{r}, width_a]")
    if out is None:
        out = torch.empty((X.shape[0], r * len(U)), dtype=BF16, device=X.device)
    return _lora_fill(X, cols, shared, bits, alpha, r, [(u.data_ptr(), u.stride(0)) for u in U], (out.data_ptr(), out.stride(0))), out


@_stream_family("lora_project", lambda r, X, U, cols=None, alpha=1.0, bits=None, out=None: _cols_bytes(X, cols) + _nb(r) + (_nb(bits) if bits is not None else 0))
def lora_project(X, U, cols=None, alpha=1.0, bits=None, out=None):
    """P[m, r a+j] = alpha * sum_w keep_a(m,w) X[m, c0_a+w] U_a[j,w].  U: list of bf16 [r, width_a] matrices, r = U[0].shape[0]
    in LORA_RANKS.  cols=None: the adapters share all of X's columns (optionally with dropout bit planes `bits`);
    cols=[(c0, width), ...]: adapter a owns that column range of X."""
    a, out = lora_project_args(X, U, cols, alpha, bits, out)
    check(_lib.load().ur_lora_project(ctypes.byref(a), _stream()), "ur_lora_project")
    return out


@_stream_family("swiglu_lora", lambda r, gu, I, U, alpha=1.0, bits=None, t_out=None: _nb(gu) + _nb(*r) + (_nb(bits) if bits is not None else 0))
def swiglu_lora_fwd(gu, I, U, alpha=1.0, bits=None, t_out=None):
    """SwiGLU forward + the down_proj adapter's down projection in one pass over gu [M, 2I]: -> (act bf16 [M, I], t bf16 [M, 16]).
    t_out: write t there (a bf16 [M, 16] view; its row stride may be wider)."""
    lib = _lib.load()
    _need(gu, BF16, "gu")
    M = gu.shape[0]
    act = torch.empty((M, I), dtype=BF16, device=gu.device)
    if U.dtype != BF16 or U.shape[0] != 16 or U.stride(1) != 1 or U.shape[1] != I:
        raise ValueError("swiglu_lora_fwd: U must be bf16 [16, I]")
    t = torch.empty((M, 16), dtype=BF16, device=gu.device) if t_out is None else t_out
    a = _lora_fill(act, [(0, I)], True, bits, alpha, 16, [(U.data_ptr(), U.stride(0))], (t.data_ptr(), t.stride(0)))
    check(lib.ur_swiglu_lora_fwd(gu.data_ptr(), act.data_ptr(), M, I, ctypes.byref(a), _stream()), "ur_swiglu_lora_fwd")
    return act, t


@_stream_family("rms_lora", lambda r, x, w, eps, U, alpha=1.0, bits=None, t_out=None: _nb(x) + _nb(*r) + (_nb(bits) if bits is not None else 0))
def rmsnorm_lora_fwd(x, w, eps, U, alpha=1.0, bits=None, t_out=None):
    """RMSNorm forward + the down projection of the 1 to 3 adapters that read the normalised activation, one pass over x:
    -> (h bf16 like x, rstd f32 [M], t bf16 [M, 16 len(U)]).  D must be 1024.  t_out: write t there (a bf16 [M, 16 len(U)] view; its
    row stride may be wider)."""
    lib = _lib.load()
    _need(x, BF16, "x")
    if not 1 <= len(U) <= 3:
        raise ValueError(f"rmsnorm_lora_fwd: 1 to 3 adapters share the normalised input (got {len(U)})")
    D = x.shape[-1]
    M = x.numel() // D
    out = torch.empty_like(x)
    rstd = torch.empty((M,), dtype=F32, device=x.device)
    for u in U:
        if u.dtype != BF16 or u.shape[0] != 16 or u.stride(1) != 1 or u.shape[1] != D:
            raise ValueError("rmsnorm_lora_fwd: U[a] must be bf16 [16, D]")
    t = torch.empty((M, 16 * len(U)), dtype=BF16, device=x.device) if t_out is None else t_out
    a = _lora_fill(out.view(M, D), [(0, D)] * len(U), True, bits, alpha, 16, [(u.data_ptr(), u.stride(0)) for u in U], (t.data_ptr(), t.stride(0)))
    check(lib.ur_rmsnorm_lora_fwd(x.data_ptr(), w.data_ptr(), out.data_ptr(), rstd.data_ptr(), M, D, eps, ctypes.byref(a), _stream()),
          "ur_rmsnorm_lora_fwd")
    return out, rstd, t


def _reduce_rank(out, X, cols, nad):
    """rank of a token reduction = rows of its dense output per input column"""
    wsum = sum(w for _, w in cols) if cols is not None else X.shape[1] * int(nad)
    return out.numel() // max(wsum, 1)


def lora_reduce_args(X, V, out, cols=None, nad=None, alpha=1.0, bits=None, transposed=False, bits_t=None):
    """the LoraArgs of lora_reduce for these tensors -- what the launch passes and what lora_plan("reduce", ...) is asked with"""
    shared = cols is None
    r = _reduce_rank(out, X, cols, nad)
    if shared:
        cols = [(0, X.shape[1])] * int(nad)
    if out.numel() != r * sum(w for _, w in cols):
        raise ValueError("lora_reduce: out has the wrong size")
    r = _lora_rank(r, "lora_reduce")
    if V.dtype != BF16 or V.stride(1) != 1 or V.shape[0] != X.shape[0] or V.shape[1] < r * len(cols):
        raise ValueError(f"lora_reduce: V must be bf16 [M, >= {r} nad]")
    _need(out, F32, "out")
    if bits is None or bits_t is None:
        bt = None
    elif bits_t.dtype != torch.int32 or bits_t.dim() != 3 or bits_t.shape[0] != bits.shape[0] or bits_t.shape[1] * 32 != X.shape[0] or bits_t.stride(2) != 1:
        raise ValueError("lora_reduce: bits_t must be the int32 [nad, M / 32, ld] tensor of lora_bits_transpose")
    else:
        bt = (bits_t.data_ptr(), bits_t.stride(1), bits_t.stride(0))
    return _lora_fill(X, cols, shared, bits, alpha, r, V=(V.data_ptr(), V.stride(0)), G=out.data_ptr(), transposed=transposed, bits_t=bt)


@_stream_family("lora_reduce", lambda r, X, V, out, cols=None, nad=None, alpha=1.0, bits=None, transposed=False, bits_t=None:
                _cols_bytes(X, cols) + X.shape[0] * 2 * _reduce_rank(out, X, cols, nad) * (len(cols) if cols is not None else int(nad)) + (_nb(bits) if bits is not None else 0))
def lora_reduce(X, V, out, cols=None, nad=None, alpha=1.0, bits=None, transposed=False, bits_t=None):
    """G_a[j,w] = alpha * sum_m V[m,r a+j] keep_a(m,w) X[m, c0_a+w] into the dense f32 tensor `out`
    ([r nad, W] for shared columns, or [sum width, r] with transposed=True for per-adapter column ranges); the rank r in LORA_RANKS is
    what the size of `out` says.  bits_t: lora_bits_transpose(bits, W) -- with it a rank-16 launch streams X through the LDS-DMA ring
    kernel (the other ranks run the register-staged kernel either way)."""
    lib = _lib.load()
    a = lora_reduce_args(X, V, out, cols, nad, alpha, bits, transposed, bits_t)
    wsb = lib.ur_lora_reduce_workspace_bytes(ctypes.byref(a))
    ws = workspace(wsb, X.device, "lora").data_ptr() if wsb else 0
    check(lib.ur_lora_reduce(ctypes.byref(a), ws, wsb, _stream()), "ur_lora_reduce")
    return out


def layernorm_fwd(y, gamma, beta, eps, residual=None, save_z=True, p_pre=0.0, seed_pre=0, p_post=0.0, seed_post=0,
                  M=None, drop_row0=0):
    """Returns (out, z, mean, rstd).  y may have fewer rows than M (row m reads y[m % y.shape[0]]).  drop_row0: rows that
    precede this launch's row 0 in the global minibatch (dropout masks keyed on the global element index)."""
    lib = _lib.load()
    _need(y, BF16, "y")
    H = y.shape[-1]
    y_rows = y.numel() // H
    if M is None:
        M = y_rows
    dev = y.device
    out = torch.empty((M, H), dtype=BF16, device=dev)
    z = torch.empty((M, H), dtype=BF16, device=dev) if save_z else None
    mean = torch.empty((M,), dtype=F32, device=dev)
    rstd = torch.empty((M,), dtype=F32, device=dev)
    check(lib.ur_layernorm_fwd(y.data_ptr(), y_rows, _p(residual), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), _p(z),
                               mean.data_ptr(), rstd.data_ptr(), M, H, eps, p_pre, seed_pre, p_post, seed_post, int(drop_row0), _stream()),
          "ur_layernorm_fwd")
    return out, z, mean, rstd


def layernorm_bwd(dout, z, mean, rstd, gamma, dgamma, dbeta, dbias=None, p_pre=0.0, seed_pre=0, p_post=0.0, seed_post=0,
                  need_dy=True, drop_row0=0, defer_reduce=False):
    """Returns (dz, dy); dgamma/dbeta/dbias (f32 [H]) are overwritten in place.
    defer_reduce=True: returns (dz, dy, finish) -- the call stops at the per-block partial sums (a scratch tensor of its own) and
    finish() launches their reduction into dgamma / dbeta / dbias on the stream that is current WHEN IT IS CALLED (ordering against this
    call is the caller's: qformer.py runs it on its side stream behind an event)."""
    lib = _lib.load()
    M, H = z.shape
    dz = torch.empty_like(z)
    dy = dz if (p_pre == 0.0 or not need_dy) else torch.empty_like(z)
    wsb = lib.ur_layernorm_bwd_workspace_bytes(H)
    if defer_reduce:
        ws = torch.empty(int(wsb), dtype=torch.uint8, device=z.device)
        check(lib.ur_layernorm_bwd(dout.data_ptr(), z.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                   dz.data_ptr(), dy.data_ptr() if need_dy else 0, 0, 0, 0,
                                   M, H, p_pre, seed_pre, p_post, seed_post, int(drop_row0), ws.data_ptr(), wsb, _stream()), "ur_layernorm_bwd")

        def finish():
            check(lib.ur_layernorm_bwd_reduce(ws.data_ptr(), M, H, dgamma.data_ptr(), dbeta.data_ptr(), _p(dbias), _stream()), "ur_layernorm_bwd_reduce")
        finish.scratch = ws
        return dz, dy, finish
    ws = workspace(wsb, z.device, "ln")
    check(lib.ur_layernorm_bwd(dout.data_ptr(), z.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                               dz.data_ptr(), dy.data_ptr() if need_dy else 0, dgamma.data_ptr(), dbeta.data_ptr(), _p(dbias),
                               M, H, p_pre, seed_pre, p_post, seed_post, int(drop_row0), ws.data_ptr(), wsb, _stream()), "ur_layernorm_bwd")
    return dz, dy


def batch_reduce(x, nb, rows, H, out=None):
    lib = _lib.load()
    _need(x, BF16, "x")
    if out is None:
        out = torch.empty((rows, H), dtype=F32, device=x.device)
    wsb = lib.ur_batch_reduce_workspace_bytes(nb, rows, H)
    ws = workspace(wsb, x.device, "br")
    check(lib.ur_batch_reduce(x.data_ptr(), out.data_ptr(), nb, rows, H, ws.data_ptr(), wsb, _stream()), "ur_batch_reduce")
    return out


def colsum(x2d, out=None):
    """f32 column sums of a contiguous bf16 [M,N] (bias gradients)."""
    M, N = x2d.shape
    o = batch_reduce(x2d, M, 1, N, out=None if out is None else out.view(1, N))
    return o.view(N)


def rmsnorm_fwd(x, w, eps):
    lib = _lib.load()
    _need(x, BF16, "x")
    D = x.shape[-1]
    M = x.numel() // D
    out = torch.empty_like(x)
    rstd = torch.empty((M,), dtype=F32, device=x.device)
    check(lib.ur_rmsnorm_fwd(x.data_ptr(), w.data_ptr(), out.data_ptr(), rstd.data_ptr(), M, D, eps, _stream()), "ur_rmsnorm_fwd")
    return out, rstd


@_stream_family("rms_bwd", lambda r, dout, x, w, rstd, add=None: _nb(dout, x, r, add))
def rmsnorm_bwd(dout, x, w, rstd, add=None):
    lib = _lib.load()
    D = x.shape[-1]
    M = x.numel() // D
    dx = torch.empty_like(x)
    check(lib.ur_rmsnorm_bwd(dout.data_ptr(), x.data_ptr(), w.data_ptr(), rstd.data_ptr(), _p(add), dx.data_ptr(), M, D, _stream()),
          "ur_rmsnorm_bwd")
    return dx


class AttnCtx:
    """What ur_attn_bwd needs from the forward (argument struct + the tensors it points into)."""
    __slots__ = ("args", "keep", "o", "stats")


def attn_ctx_prefix(ctx, Bg):
    """The forward context restricted to its first Bg samples (a backward over the leading rows of a larger forward): same pointers
    and strides -- batch b of every operand sits at b * (tokens * stride) -- with B = Bg."""
    a = AttnArgs.from_buffer_copy(ctx.args)
    a.B = int(Bg)
    c = AttnCtx()
    c.args, c.keep, c.o, c.stats = a, ctx.keep, ctx.o, ctx.stats
    return c


def _tok_stride(t):
    # [B,S,heads,hd] view (possibly a slice of a fused projection buffer): elements between tokens
    if t.stride(3) != 1 or t.stride(2) != t.shape[3] or t.stride(0) != t.shape[1] * t.stride(1):
        raise ValueError("attention operand must be [B,S,heads,hd] with dense heads and uniform token stride")
    return t.stride(1)


def attn_fwd(q, k, v, *, causal, key_mask=None, scale=None, dropout_p=0.0, seed=0, out=None, drop_batch0=0):
    """q [B,Sq,nq,hd], k/v [B,Sk,nkv,hd] bf16 (strided views allowed).  key_mask uint8 [B,Sk] or None.
    Returns (o [B,Sq,nq,hd] contiguous, ctx)."""
    lib = _lib.load()
    B, Sq, nq, hd = q.shape
    Sk, nkv = k.shape[1], k.shape[2]
    if out is None:
        out = torch.empty((B, Sq, nq, hd), dtype=BF16, device=q.device)
    stats = torch.empty((B, nq, Sq, 2), dtype=F32, device=q.device)
    if key_mask is not None and (key_mask.dtype != torch.uint8 or not key_mask.is_contiguous()):
        raise TypeError("key_mask must be a contiguous uint8 [B,Sk] tensor")
    a = AttnArgs()
    a.q, a.k, a.v, a.o, a.stats = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), stats.data_ptr()
    a.ldq, a.ldk, a.ldv, a.ldo = _tok_stride(q), _tok_stride(k), _tok_stride(v), _tok_stride(out)
    a.key_mask = _p(key_mask)
    a.B, a.Sq, a.Sk, a.nq, a.nkv, a.head_dim = B, Sq, Sk, nq, nkv, hd
    a.causal = int(causal)
    a.scale = float(scale if scale is not None else hd ** -0.5)
    a.dropout_p, a.seed, a.drop_batch0 = float(dropout_p), int(seed), int(drop_batch0)
    if PROFILE_ATTN is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(lib.ur_attn_fwd(ctypes.byref(a), _stream()), "ur_attn_fwd")
        e1.record()
        PROFILE_ATTN.append((e0, e1, "fwd", B, Sq, Sk, nq, hd, int(causal)))
    else:
        check(lib.ur_attn_fwd(ctypes.byref(a), _stream()), "ur_attn_fwd")
    ctx = AttnCtx()
    ctx.args, ctx.keep, ctx.o, ctx.stats = a, (q, k, v, key_mask), out, stats
    return out, ctx


def attn_bwd_kv_colsum_supported(ctx):
    """True when attn_bwd(ctx, ..., kv_colsum=) can also produce the column sums of dK | dV (the few-query dK/dV kernel's shapes)."""
    return int(_lib.load().ur_attn_bwd_kv_colsum_floats(ctypes.byref(ctx.args))) > 0


def attn_plan(ctx_or_args, bwd=None):
    """Which kernels attn_fwd / attn_bwd take for these arguments under the current attn_mode words (ur_attn_plan): a dict with
    fwd, dq, dkv (names from ATTN_KERNELS), lse_log2 and nw_q, nw_k (waves per workgroup of the generic kernels).  ctx_or_args: an AttnCtx or an AttnArgs (only sizes, strides and flags are read:
    no tensor and no device is needed); bwd: an AttnBwdArgs (lddo and whether kv_colsum is set are read), None = the forward only
    (dq = dkv = "none").  Raises UniRecHipError where the entry points would refuse the arguments."""
    a = ctx_or_args.args if isinstance(ctx_or_args, AttnCtx) else ctx_or_args
    out = AttnPlanInfo()
    check(_lib.load().ur_attn_plan(ctypes.byref(a), None if bwd is None else ctypes.byref(bwd), ctypes.byref(out)), "ur_attn_plan")
    return dict(fwd=ATTN_KERNELS[out.fwd], dq=ATTN_KERNELS[out.dq], dkv=ATTN_KERNELS[out.dkv], lse_log2=int(out.lse_log2),
                nw_q=int(out.nw_q), nw_k=int(out.nw_k))


def attn_bwd(ctx, dout, dq=None, dk=None, dv=None, rope_q=None, rope_rstd=None, rope_k=None, kv_colsum=None):
    """dout [B,Sq,nq,hd] -> (dq, dk, dv); outputs may be strided views into a fused gradient buffer.
    rope_q = (q_raw [M, >= nq*hd] view, q_norm_weight f32 [hd], cos, sin, eps, dq_raw [M, >= nq*hd] view): the dQ kernel carries
    the q-norm + RoPE backward and writes the gradient of the RAW q projection into dq_raw; no dq is produced (returns None).
    rope_rstd = (rstd f32 [M, nh], first q head's column): the forward ran q-norm + RoPE in the q|k|v GEMM epilogue -- rope_q[0]
    is then the ROPED q (the attention's own q) and 1 / rms comes from rstd (ur_attn_bwd_args.rope_rstd).
    rope_k = (k_r [M, >= nkv*hd] view, k_norm_weight, first k head's column of rstd, dk_raw [M, >= nkv*hd] view) with rope_rstd: the
    k heads' backward too (in the dK/dV kernel's store where the generated kernel runs, else by the stand-alone kernel inside the call;
    dk is scratch then).
    kv_colsum = f32 [2 * nq * hd] (contiguous): also receives [column sums of dK | of dV] over all keys and batch rows -- the K | V
    projections' bias gradients -- when attn_bwd_kv_colsum_supported(ctx)."""
    lib = _lib.load()
    q, k, v, _ = ctx.keep
    if dq is None and rope_q is None:
        dq = torch.empty(q.shape, dtype=BF16, device=q.device)
    if dk is None:
        dk = torch.empty(k.shape, dtype=BF16, device=q.device)
    if dv is None:
        dv = torch.empty(v.shape, dtype=BF16, device=q.device)
    a = ctx.args
    # workspace: the row constants (-rowsum(dO*O), -LSE/scale) + the call's own work-queue words (the library owns no device state)
    delta = torch.empty((int(lib.ur_attn_bwd_workspace_floats(a.B, a.nq, a.Sq)),), dtype=F32, device=q.device)
    g = AttnBwdArgs()
    g.dout, g.dq, g.dk, g.dv = dout.data_ptr(), (0 if dq is None else dq.data_ptr()), dk.data_ptr(), dv.data_ptr()
    g.lddo, g.lddq, g.lddk, g.lddv = _tok_stride(dout), (0 if dq is None else _tok_stride(dq)), _tok_stride(dk), _tok_stride(dv)
    if rope_q is not None:
        q_raw, qw, cos, sin, eps, dq_raw = rope_q
        g.rope_q_raw, g.rope_ldraw, g.rope_q_weight = q_raw.data_ptr(), q_raw.stride(0), qw.data_ptr()
        g.rope_cos, g.rope_sin, g.rope_eps = cos.data_ptr(), sin.data_ptr(), float(eps)
        g.rope_dq_raw, g.rope_lddraw = dq_raw.data_ptr(), dq_raw.stride(0)
        if rope_rstd is not None:
            rstd, h0 = rope_rstd
            _need(rstd, F32, "rope_rstd")
            g.rope_rstd, g.rope_rstd_ld, g.rope_rstd_h0 = rstd.data_ptr(), rstd.stride(0), int(h0)
            if rope_k is not None:
                k_r, kw, hk0, dk_raw = rope_k
                g.rope_k, g.rope_ldk, g.rope_k_weight, g.rope_rstd_hk0 = k_r.data_ptr(), k_r.stride(0), kw.data_ptr(), int(hk0)
                g.rope_dk_raw, g.rope_lddkraw = dk_raw.data_ptr(), dk_raw.stride(0)
    g.delta = delta.data_ptr()
    if kv_colsum is not None:
        nws = int(lib.ur_attn_bwd_kv_colsum_floats(ctypes.byref(a)))
        if nws <= 0:
            raise ValueError("attn_bwd: kv_colsum is not available for this shape (attn_bwd_kv_colsum_supported)")
        _need(kv_colsum, F32, "kv_colsum")
        if kv_colsum.numel() != 2 * a.nq * a.head_dim or not kv_colsum.is_contiguous():
            raise ValueError("attn_bwd: kv_colsum must be a contiguous f32 tensor of 2 * nq * head_dim elements")
        cws = torch.empty((nws,), dtype=F32, device=q.device)
        g.kv_colsum, g.kv_colsum_ws = kv_colsum.data_ptr(), cws.data_ptr()
    if PROFILE_ATTN is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(lib.ur_attn_bwd(ctypes.byref(a), ctypes.byref(g), _stream()), "ur_attn_bwd")
        e1.record()
        PROFILE_ATTN.append((e0, e1, "bwd", a.B, a.Sq, a.Sk, a.nq, a.head_dim, a.causal))
    else:
        check(lib.ur_attn_bwd(ctypes.byref(a), ctypes.byref(g), _stream()), "ur_attn_bwd")
    return dq, dk, dv


def dropout_keep(seed, p, idx0, n, device):
    """uint8 [n]: keep flags of elements idx0 .. idx0 + n - 1 of the dropout stream `seed` (ur_dropout_keep) -- test / inspection
    helper: hidden dropout counters are (drop_row0 + row) * H + col (attention probabilities: attn_dropout_keep)."""
    lib = _lib.load()
    out = torch.empty((int(n),), dtype=torch.uint8, device=device)
    check(lib.ur_dropout_keep(int(seed), float(p), int(idx0), int(n), out.data_ptr(), _stream()), "ur_dropout_keep")
    return out


def attn_dropout_keep(seed, p, row0, nrows, Sk, device):
    """uint8 [nrows, Sk]: keep flags of the attention-probability dropout for the rows row0 .. (ur_attn_dropout_keep); a row is
    ((drop_batch0 + b) * heads + h) * Sq + query -- test / inspection helper."""
    lib = _lib.load()
    out = torch.empty((int(nrows), int(Sk)), dtype=torch.uint8, device=device)
    check(lib.ur_attn_dropout_keep(int(seed), float(p), int(row0), int(nrows), int(Sk), out.data_ptr(), _stream()), "ur_attn_dropout_keep")
    return out


def cast_f32_to_bf16(src, dst=None):
    lib = _lib.load()
    _need(src, F32, "src")
    if dst is None:
        dst = torch.empty(src.shape, dtype=BF16, device=src.device)
    check(lib.ur_cast_f32_to_bf16(src.data_ptr(), dst.data_ptr(), src.numel(), _stream()), "ur_cast_f32_to_bf16")
    return dst


def cast_bf16_to_f32(src, dst=None):
    lib = _lib.load()
    _need(src, BF16, "src")
    if dst is None:
        dst = torch.empty(src.shape, dtype=F32, device=src.device)
    check(lib.ur_cast_bf16_to_f32(src.data_ptr(), dst.data_ptr(), src.numel(), _stream()), "ur_cast_bf16_to_f32")
    return dst


def lora_merge(W, A, B, scale, out_f32=None, out_bf16=None):
    """out = W + scale * B A from the f32 masters in one pass over W (ur_lora_merge, include/unirec_hip_adapter.h): W f32 [out, in]
    (rows may be strided), A f32 [r, in], B f32 [out, r], r one of LORA_RANKS.  out_f32 / out_bf16: [out, in] tensors to write (rows may be
    strided); out_f32 may be W itself (the merge in place).  With neither given a new f32 tensor is made.  Returns (out_f32, out_bf16)."""
    if W.dim() != 2 or A.dim() != 2 or B.dim() != 2 or A.shape[1] != W.shape[1] or B.shape != (W.shape[0], A.shape[0]):
        raise ValueError(f"lora_merge: W [out,in], A [r,in], B [out,r] expected, got {tuple(W.shape)}, {tuple(A.shape)}, {tuple(B.shape)}")
    _lora_rank(A.shape[0], "lora_merge")
    _need(A, F32, "A")
    _need(B, F32, "B")
    lib = _lib.load()
    if out_f32 is None and out_bf16 is None:
        out_f32 = torch.empty(W.shape, dtype=F32, device=W.device)
    a = _lib.LoraMerge()
    for t, dtype, name in ((W, F32, "W"), (out_f32, F32, "out_f32"), (out_bf16, BF16, "out_bf16")):
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.UniRecHipError(f"lora_merge: {name} must be a device tensor (the UniRec HIP path has no CPU fallback)")
        if t.dtype != dtype or t.shape != W.shape or (t.shape[1] > 1 and t.stride(1) != 1):
            raise ValueError(f"lora_merge: {name} must be {dtype} {tuple(W.shape)} with unit column stride")
    a.W, a.ldw, a.A, a.B = W.data_ptr(), W.stride(0), A.data_ptr(), B.data_ptr()
    a.rank, a.scale = A.shape[0], float(scale)
    a.out_rows, a.in_cols = W.shape
    if out_f32 is not None:
        a.out_f32, a.ld_f32 = out_f32.data_ptr(), out_f32.stride(0)
    if out_bf16 is not None:
        a.out_bf16, a.ld_bf16 = out_bf16.data_ptr(), out_bf16.stride(0)
    check(lib.ur_lora_merge(ctypes.byref(a), _stream()), "ur_lora_merge")
    return out_f32, out_bf16


class BatchedTranspose:
    """Many small bf16 transposes as ONE launch (ur_transpose_bf16_batched).  Built once over persistent source tensors
    (views of a parameter pack's bf16 shadow); run() refreshes every destination; out[i] is the transposed view."""

    def __init__(self, sources):
        import numpy as np
        dev = sources[0].device
        total = sum(t.numel() for t in sources)
        self.buf = torch.empty(total, dtype=BF16, device=dev)
        self.out, rec, off, tile = [], np.zeros((len(sources), 4), dtype=np.int64), 0, 0
        for i, t in enumerate(sources):
            if t.dim() != 2 or not t.is_contiguous() or t.dtype != BF16:
                raise ValueError("BatchedTranspose: contiguous 2-D bf16 sources only")
            rows, cols = t.shape
            d = self.buf[off:off + rows * cols].view(cols, rows)
            off += rows * cols
            self.out.append(d)
            ntx = (cols + 31) // 32
            rec[i] = (t.data_ptr(), d.data_ptr(), rows | (cols << 32), tile | (ntx << 32))
            tile += ntx * ((rows + 31) // 32)
        self.sources = sources                       # keeps the storages alive
        self.n, self.tiles = len(sources), tile
        self.desc = torch.from_numpy(rec).to(dev)
        self.key = tuple(t.data_ptr() for t in sources)

    def run(self):
        check(_lib.load().ur_transpose_bf16_batched(self.desc.data_ptr(), self.n, self.tiles, _stream()), "ur_transpose_bf16_batched")
        return self.out


def transpose_bf16(src, dst=None):
    lib = _lib.load()
    _need(src, BF16, "src")
    rows, cols = src.shape
    if dst is None:
        dst = torch.empty((cols, rows), dtype=BF16, device=src.device)
    check(lib.ur_transpose_bf16(src.data_ptr(), dst.data_ptr(), rows, cols, _stream()), "ur_transpose_bf16")
    return dst


def add_bf16(a, b, out=None):
    lib = _lib.load()
    if out is None:
        out = torch.empty_like(a)
    check(lib.ur_add_bf16(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _stream()), "ur_add_bf16")
    return out


def swiglu_fwd(gu, I, out=None):
    lib = _lib.load()
    M = gu.numel() // (2 * I)
    act = torch.empty((M, I), dtype=BF16, device=gu.device) if out is None else out
    assert act.is_contiguous() and act.numel() == M * I and act.dtype == BF16
    check(lib.ur_swiglu_fwd(gu.data_ptr(), act.data_ptr(), M, I, _stream()), "ur_swiglu_fwd")
    return act


def swiglu_bwd(dact, gu, I):
    lib = _lib.load()
    M = gu.numel() // (2 * I)
    dgu = torch.empty_like(gu)
    check(lib.ur_swiglu_bwd(dact.data_ptr(), gu.data_ptr(), dgu.data_ptr(), M, I, _stream()), "ur_swiglu_bwd")
    return dgu


@_stream_family("adamw", lambda r, param, grad, exp_avg, exp_avg_sq, *a, **k: 2 * _nb(param, exp_avg, exp_avg_sq) + _nb(grad))
def adamw_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, coef=None):
    """coef: None (ur_adamw_step) or a 0-d f32 device tensor, the clip coefficient of grad_norm_clip: the gradient is scaled by
    grad_scale * coef on the device (ur_adamw_step_dev, no host read)."""
    lib = _lib.load()
    if coef is None:
        check(lib.ur_adamw_step(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), param.numel(), lr,
                                beta1, beta2, eps, weight_decay, step, grad_scale, _stream()), "ur_adamw_step")
    else:
        _need(coef, F32, "adamw_step(coef)")
        check(lib.ur_adamw_step_dev(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), param.numel(), lr,
                                    beta1, beta2, eps, weight_decay, step, grad_scale, coef.data_ptr(), _stream()), "ur_adamw_step_dev")


def grad_norm_partials(ranges):
    """partial slots ur_grad_norm_clip needs for these ranges (UR_NORM_BLOCK_ELEMS elements per slot)"""
    return sum(-(-r.numel() // _lib.NORM_BLOCK_ELEMS) for r in ranges)


@_stream_family("grad_norm", lambda r, ranges, *a, **k: _nb(*ranges))
def grad_norm_clip(ranges, grad_scale, max_norm, out_norm, out_coef):
    """torch.nn.utils.clip_grad_norm_'s global L2 norm and clip coefficient over a list of contiguous f32 device tensors (the live
    gradient spans), without touching them: out_norm = ||all ranges|| * grad_scale, out_coef = min(max_norm / (norm + 1e-6), 1),
    both 0-d f32 device tensors written on the current stream (no host sync).  Deterministic (fixed split, no atomics)."""
    lib = _lib.load()
    _need(out_norm, F32, "grad_norm_clip(out_norm)")
    _need(out_coef, F32, "grad_norm_clip(out_coef)")
    for r in ranges:
        _need(r, F32, "grad_norm_clip(range)")
    arr = (_lib.F32Range * max(1, len(ranges)))()
    for i, r in enumerate(ranges):
        arr[i].ptr, arr[i].n = r.data_ptr(), r.numel()
    nparts = grad_norm_partials(ranges)
    ws = workspace(4 * max(1, nparts), out_norm.device, tag="grad_norm")
    check(lib.ur_grad_norm_clip(arr, len(ranges), ws.data_ptr(), nparts, grad_scale, max_norm, out_norm.data_ptr(), out_coef.data_ptr(),
                                _stream()), "ur_grad_norm_clip")


# ---- Qwen3-side ops ------------------------------------------------------------------------------
def rope_table(S, head_dim, theta, device):
    lib = _lib.load()
    cos = torch.empty((S, head_dim // 2), dtype=F32, device=device)
    sin = torch.empty((S, head_dim // 2), dtype=F32, device=device)
    check(lib.ur_rope_table(cos.data_ptr(), sin.data_ptr(), S, head_dim, theta, _stream()), "ur_rope_table")
    return cos, sin


def qknorm_rope_fwd(qkv_raw, qw, kw, cos, sin, S, nq, nkv, hd, eps):
    """qkv_raw [M,(nq+2nkv)*hd] -> (q_out [M,nq*hd], k_out [M,nkv*hd])."""
    lib = _lib.load()
    M = qkv_raw.shape[0]
    q_out = torch.empty((M, nq * hd), dtype=BF16, device=qkv_raw.device)
    k_out = torch.empty((M, nkv * hd), dtype=BF16, device=qkv_raw.device)
    check(lib.ur_qknorm_rope_fwd(qkv_raw.data_ptr(), qkv_raw.stride(0), qw.data_ptr(), kw.data_ptr(), cos.data_ptr(), sin.data_ptr(),
                                 q_out.data_ptr(), k_out.data_ptr(), M, S, nq, nkv, hd, eps, _stream()), "ur_qknorm_rope_fwd")
    return q_out, k_out


def qknorm_rope_bwd(dq_out, dk_out, qkv_raw, qw, kw, cos, sin, dqkv_raw, S, nq, nkv, hd, eps):
    lib = _lib.load()
    M = qkv_raw.shape[0]
    check(lib.ur_qknorm_rope_bwd(dq_out.data_ptr(), dk_out.data_ptr(), qkv_raw.data_ptr(), qkv_raw.stride(0), qw.data_ptr(), kw.data_ptr(),
                                 cos.data_ptr(), sin.data_ptr(), dqkv_raw.data_ptr(), dqkv_raw.stride(0), M, S, nq, nkv, hd, eps,
                                 _stream()), "ur_qknorm_rope_bwd")
    return dqkv_raw


def embed_inject_fwd(embed, input_ids, item_tokens, first_special_id):
    """embed [V,D] bf16, input_ids int64 [B,S], item_tokens [B,T,D] bf16 or None -> [B,S,D] bf16."""
    lib = _lib.load()
    _need(embed, BF16, "embed")
    _need(input_ids, torch.int64, "input_ids")
    B, S = input_ids.shape
    V, D = embed.shape
    T = 0 if item_tokens is None else item_tokens.shape[1]
    out = torch.empty((B, S, D), dtype=BF16, device=embed.device)
    check(lib.ur_embed_inject_fwd(embed.data_ptr(), V, input_ids.data_ptr(), _p(item_tokens), first_special_id, T, out.data_ptr(),
                                  B, S, D, _stream()), "ur_embed_inject_fwd")
    return out


def inject_bwd(dx, input_ids, first_special_id, T):
    lib = _lib.load()
    B, S, D = dx.shape
    d_tok = torch.empty((B, T, D), dtype=BF16, device=dx.device)
    check(lib.ur_inject_bwd(dx.data_ptr(), input_ids.data_ptr(), first_special_id, T, d_tok.data_ptr(), B, S, D, _stream()),
          "ur_inject_bwd")
    return d_tok


def mean_pool_fwd(x, out_f32=True, out_bf16=False):
    """x [B,S,D] bf16 -> (f32 [B,D] or None, bf16 [B,D] or None)."""
    lib = _lib.load()
    _need(x, BF16, "x")
    B, S, D = x.shape
    o32 = torch.empty((B, D), dtype=F32, device=x.device) if out_f32 else None
    o16 = torch.empty((B, D), dtype=BF16, device=x.device) if out_bf16 else None
    wsb = lib.ur_mean_pool_workspace_bytes(B, D)
    ws = workspace(wsb, x.device, "pool")
    check(lib.ur_mean_pool_fwd(x.data_ptr(), _p(o32), _p(o16), B, S, D, ws.data_ptr(), wsb, _stream()), "ur_mean_pool_fwd")
    return o32, o16


def mean_pool_bwd(dout, S):
    """dout [B,D] (f32 or bf16) -> dx [B,S,D] bf16 = dout / S broadcast."""
    lib = _lib.load()
    B, D = dout.shape
    dx = torch.empty((B, S, D), dtype=BF16, device=dout.device)
    d32 = dout.data_ptr() if dout.dtype == F32 else 0
    d16 = dout.data_ptr() if dout.dtype == BF16 else 0
    check(lib.ur_mean_pool_bwd(d32, d16, dx.data_ptr(), B, S, D, _stream()), "ur_mean_pool_bwd")
    return dx


# ---- mask-aware pooling fused with the final RMSNorm (include/unirec_hip_pool.h) -------------------
POOL_MODES = {"masked_mean": _lib.POOL_MASKED_MEAN, "last": _lib.POOL_LAST}
POOLINGS = ("mean",) + tuple(POOL_MODES)      # "mean": rmsnorm_fwd + mean_pool_fwd over all S positions (the default rule)


def _pool_norm_args(x, w, mask, mode):
    if mode not in POOL_MODES:
        raise ValueError(f"pool_norm: mode must be one of {', '.join(POOL_MODES)} (got {mode!r})")
    _need(x, BF16, "x")
    _need(w, F32, "w")
    if x.dim() != 3 or tuple(w.shape) != (x.shape[2],):
        raise ValueError(f"pool_norm: x [B,S,D] and w [D] expected, got {tuple(x.shape)} and {tuple(w.shape)}")
    if mask is not None:
        _need(mask, torch.uint8, "mask")
        if tuple(mask.shape) != tuple(x.shape[:2]):
            raise ValueError(f"pool_norm: mask must be [B,S] = {tuple(x.shape[:2])}, got {tuple(mask.shape)}")
    lib = _lib.load()
    B, S, D = x.shape
    wsb = lib.ur_pool_norm_workspace_bytes(B, D, POOL_MODES[mode])
    if wsb < 0:
        check(-1, "ur_pool_norm_workspace_bytes")
    return lib, B, S, D, wsb, workspace(wsb, x.device, "pool_norm")


def pool_norm_fwd(x, w, eps, mask=None, mode="masked_mean"):
    """x [B,S,D] bf16 (the last layer's output), w [D] f32 (final norm weight), mask [B,S] uint8 or None (all valid) -> pooled f32 [B,D]:
    RMSNorm and the pooling rule `mode` in one pass; masked rows are not read."""
    lib, B, S, D, wsb, ws = _pool_norm_args(x, w, mask, mode)
    out = torch.empty((B, D), dtype=F32, device=x.device)
    check(lib.ur_pool_norm_fwd(x.data_ptr(), w.data_ptr(), _p(mask), out.data_ptr(), B, S, D, eps, POOL_MODES[mode], ws.data_ptr(), wsb,
                               _stream()), "ur_pool_norm_fwd")
    return out


def pool_norm_bwd(d_pooled, x, w, eps, mask=None, mode="masked_mean"):
    """d_pooled f32 [B,D] -> dx bf16 [B,S,D], the gradient of pool_norm_fwd with respect to x (every row written; +0 where the pooling
    weight is 0)."""
    lib, B, S, D, wsb, ws = _pool_norm_args(x, w, mask, mode)
    _need(d_pooled, F32, "d_pooled")
    if tuple(d_pooled.shape) != (B, D):
        raise ValueError(f"pool_norm_bwd: d_pooled must be [B,D] = {(B, D)}, got {tuple(d_pooled.shape)}")
    dx = torch.empty_like(x)
    check(lib.ur_pool_norm_bwd(d_pooled.data_ptr(), x.data_ptr(), w.data_ptr(), _p(mask), dx.data_ptr(), B, S, D, eps, POOL_MODES[mode],
                               ws.data_ptr(), wsb, _stream()), "ur_pool_norm_bwd")
    return dx


# ---- ranking head --------------------------------------------------------------------------------
@_stream_family("J6_candidate_scores", lambda r, user, pos, neg: _nb(user, pos, neg) + _nb(*r))
def cosine_scores(user, pos, neg):
    """user [B,D], pos [B,D], neg [B,N,D] f32 -> (scores [B,1+N], cand_inv_norm [B,1+N])."""
    lib = _lib.load()
    for t, n in ((user, "user"), (pos, "pos"), (neg, "neg")):
        _need(t, F32, n)
    B, D = user.shape
    N = neg.shape[1]
    scores = torch.empty((B, N + 1), dtype=F32, device=user.device)
    inv = torch.empty((B, N + 1), dtype=F32, device=user.device)
    check(lib.ur_cosine_scores(user.data_ptr(), pos.data_ptr(), neg.data_ptr(), scores.data_ptr(), inv.data_ptr(), B, N, D, _stream()),
          "ur_cosine_scores")
    return scores, inv


def infonce_fwd_bwd(user, pos, neg, neg_mask, scores, inv, temperature=0.07, grad_scale=1.0, need_grad=True):
    """Returns (loss [1] f32, d_user [B,D] f32 or None)."""
    lib = _lib.load()
    B, D = user.shape
    N = neg.shape[1]
    loss = torch.empty((1,), dtype=F32, device=user.device)
    du = torch.empty((B, D), dtype=F32, device=user.device) if need_grad else None
    wsb = lib.ur_infonce_workspace_bytes(B, N, D)
    ws = workspace(wsb, user.device, "infonce")
    check(lib.ur_infonce_fwd_bwd(user.data_ptr(), pos.data_ptr(), neg.data_ptr(), _p(neg_mask), scores.data_ptr(), inv.data_ptr(),
                                 temperature, grad_scale, loss.data_ptr(), _p(du), B, N, D, ws.data_ptr(), wsb, _stream()),
          "ur_infonce_fwd_bwd")
    return loss, du


def mrr_rank(scores, neg_mask=None):
    lib = _lib.load()
    B, C = scores.shape
    rank = torch.empty((B,), dtype=torch.int32, device=scores.device)
    check(lib.ur_mrr_rank(scores.data_ptr(), _p(neg_mask), rank.data_ptr(), B, C - 1, _stream()), "ur_mrr_rank")
    return rank


# ---- Matryoshka head (include/unirec_hip_mrl.h): csrc/mrl.hip --------------------------------------------------------------------
MRL_MAX_DIMS = _lib.MRL_MAX_DIMS


def mrl_dims(dims, name="dims", D=None):
    """The checks ur_mrl_* make on the prefix widths, on the host: 1..MRL_MAX_DIMS integers, positive multiples of 4, strictly ascending,
    the last equal to D when D is given.  Returns them as a tuple of ints; a ValueError names `name`."""
    try:
        out = tuple(dims)
    except TypeError:
        raise ValueError(f"{name} must be a sequence of 1 to {MRL_MAX_DIMS} integers, got {dims!r}") from None
    if not 1 <= len(out) <= MRL_MAX_DIMS or any(isinstance(d, bool) or not isinstance(d, int) for d in out):
        raise ValueError(f"{name} must hold 1 to {MRL_MAX_DIMS} integers, got {dims!r}")
    if any(d <= 0 or d % 4 for d in out):
        raise ValueError(f"{name}: every entry must be a positive multiple of 4, got {out}")
    if any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError(f"{name} must be strictly ascending, got {out}")
    if D is not None and out[-1] != int(D):
        raise ValueError(f"{name}: the last entry must be the embedding width {int(D)}, got {out}")
    return out


def mrl_weights(weights, K, name="weights"):
    """None -> all ones (Matryoshka's default); else K finite weights >= 0 with at least one positive, as a tuple of floats."""
    import math
    if weights is None:
        return (1.0,) * K
    try:
        out = tuple(float(w) for w in weights)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a sequence of {K} numbers, got {weights!r}") from None
    if len(out) != K:
        raise ValueError(f"{name} must hold one weight per prefix ({K}), got {len(out)}")
    if any(not math.isfinite(w) or w < 0 for w in out):
        raise ValueError(f"{name}: every weight must be finite and >= 0, got {out}")
    if not any(w > 0 for w in out):
        raise ValueError(f"{name}: at least one weight must be positive, got {out}")
    return out


def _mrl_operands(user, pos, neg, dims, what):
    for t, n in ((user, "user"), (pos, "pos"), (neg, "neg")):
        _need(t, F32, n)
    if user.dim() != 2 or pos.shape != user.shape or neg.dim() != 3 or neg.shape[0] != user.shape[0] or neg.shape[2] != user.shape[1]:
        raise ValueError(f"{what}: need user [B,D], pos [B,D], neg [B,N,D], got {tuple(user.shape)}, {tuple(pos.shape)}, {tuple(neg.shape)}")
    B, D = user.shape
    return B, neg.shape[1], D, mrl_dims(dims, "dims", D)


@_stream_family("J6_candidate_scores", lambda r, user, pos, neg, dims: _nb(user, pos, neg) + _nb(*r))
def mrl_scores(user, pos, neg, dims):
    """user [B,D], pos [B,D], neg [B,N,D] f32 -> (scores [K,B,1+N], cand_inv_norm [K,B,1+N]): plane k holds cosine_scores' bits on the
    first dims[k] components, and the candidates are read once for all planes (ur_mrl_scores)."""
    B, N, D, dims = _mrl_operands(user, pos, neg, dims, "mrl_scores")
    lib = _lib.load()
    K = len(dims)
    scores = torch.empty((K, B, N + 1), dtype=F32, device=user.device)
    inv = torch.empty((K, B, N + 1), dtype=F32, device=user.device)
    a = _lib.MrlScores()
    a.user, a.pos, a.neg = user.data_ptr(), pos.data_ptr(), neg.data_ptr()
    a.B, a.N, a.D, a.K = B, N, D, K
    a.dims[:K] = dims
    a.scores, a.cand_inv_norm = scores.data_ptr(), inv.data_ptr()
    check(lib.ur_mrl_scores(ctypes.byref(a), _stream()), "ur_mrl_scores")
    return scores, inv


def mrl_infonce(user, pos, neg, neg_mask, dims, weights=None, temperature=0.07, grad_scale=1.0, need_grad=True):
    """The InfoNCE loss on every prefix dims[k] of the embeddings and its weighted sum (ur_mrl_infonce): one pass over the candidates
    for all the score planes, one more for the whole gradient.  weights: None = all ones.
    Returns (loss f32 [1], plane_loss f32 [K], d_user f32 [B,D] or None, scores [K,B,1+N], cand_inv_norm [K,B,1+N])."""
    B, N, D, dims = _mrl_operands(user, pos, neg, dims, "mrl_infonce")
    K = len(dims)
    weights = mrl_weights(weights, K)
    if neg_mask is not None:
        _need(neg_mask, torch.uint8, "neg_mask")
        if tuple(neg_mask.shape) != (B, N):
            raise ValueError(f"mrl_infonce: neg_mask must be [B,N] = {(B, N)}, got {tuple(neg_mask.shape)}")
    lib = _lib.load()
    dev = user.device
    scores = torch.empty((K, B, N + 1), dtype=F32, device=dev)
    inv = torch.empty((K, B, N + 1), dtype=F32, device=dev)
    plane_loss = torch.empty((K,), dtype=F32, device=dev)
    loss = torch.empty((1,), dtype=F32, device=dev)
    du = torch.empty((B, D), dtype=F32, device=dev) if need_grad else None
    a = _lib.MrlInfoNCE()
    a.user, a.pos, a.neg, a.neg_mask = user.data_ptr(), pos.data_ptr(), neg.data_ptr(), _p(neg_mask) or None
    a.B, a.N, a.D, a.K = B, N, D, K
    a.dims[:K] = dims
    a.weights[:K] = weights
    a.temperature, a.grad_scale = float(temperature), float(grad_scale)
    a.scores, a.cand_inv_norm, a.plane_loss, a.loss, a.d_user = scores.data_ptr(), inv.data_ptr(), plane_loss.data_ptr(), loss.data_ptr(), _p(du) or None
    check(lib.ur_mrl_infonce(ctypes.byref(a), _stream()), "ur_mrl_infonce")        # size query: workspace is NULL
    wsb = a.workspace_bytes
    ws = workspace(wsb, dev, "mrl_infonce")
    a.workspace = ws.data_ptr()
    check(lib.ur_mrl_infonce(ctypes.byref(a), _stream()), "ur_mrl_infonce")
    return loss, plane_loss, du, scores, inv


def topk(scores, K):
    lib = _lib.load()
    _need(scores, F32, "scores")
    B, C = scores.shape
    idx = torch.empty((B, K), dtype=torch.int32, device=scores.device)
    val = torch.empty((B, K), dtype=F32, device=scores.device)
    ws = workspace(B * C, scores.device, "topk")
    check(lib.ur_topk(scores.data_ptr(), B, C, K, idx.data_ptr(), val.data_ptr(), ws.data_ptr(), B * C, _stream()), "ur_topk")
    return idx, val


# ---- data path: csrc/catalog.hip ----------------------------------
_KIND = {torch.uint8: 0, BF16: 1, F32: 2}


def gather_rows(src, idx, out_dtype=None):
    """out[i] = src[idx[i]] over the leading axis (idx int64, any shape; negative / out-of-range -> zero row).
    f32 sources may be gathered straight to bf16, and bf16 sources straight to f32 (out_dtype=torch.float32: the exact widening, every
    bit pattern kept; rows of a multiple of 8 elements).  Returns idx.shape + src.shape[1:]."""
    lib = _lib.load()
    if not src.is_cuda or not src.is_contiguous() or src.dtype not in _KIND:
        raise ValueError("gather_rows: src must be a contiguous uint8 / bf16 / f32 device tensor")
    out_dtype = src.dtype if out_dtype is None else out_dtype
    idx = idx.to(device=src.device, dtype=torch.int64).contiguous()
    row = 1
    for s_ in src.shape[1:]:
        row *= s_
    out = torch.empty(tuple(idx.shape) + tuple(src.shape[1:]), dtype=out_dtype, device=src.device)
    check(lib.ur_gather_rows(src.data_ptr(), _KIND[src.dtype], out.data_ptr(), _KIND[out_dtype], idx.data_ptr(), row, idx.numel(),
                             src.shape[0], _stream()), "ur_gather_rows")
    return out


def catalog_scores(user, catalog, cat_inv_norm=None):
    """cosine scores [B,N] of user [B,D] f32 against a shared catalogue [N,D] f32; returns (scores, cat_inv_norm)
    so repeated calls over the same catalogue skip its norm pass."""
    lib = _lib.load()
    _need(user, F32, "user")
    _need(catalog, F32, "catalog")
    B, D = user.shape
    N = catalog.shape[0]
    scores = torch.empty((B, N), dtype=F32, device=user.device)
    uinv = torch.empty((B,), dtype=F32, device=user.device)
    ready = cat_inv_norm is not None
    if not ready:
        cat_inv_norm = torch.empty((N,), dtype=F32, device=user.device)
    check(lib.ur_catalog_scores(user.data_ptr(), catalog.data_ptr(), scores.data_ptr(), uinv.data_ptr(), cat_inv_norm.data_ptr(),
                                int(ready), B, N, D, None, _stream()), "ur_catalog_scores")
    return scores, cat_inv_norm


CATALOG_TOPK_MAX = 128      # UR_CATALOG_TOPK_MAX


CATALOG_SCORERS = {None: 0, "vector": 1, "mfma": 2}      # ur_catalog_select_t.scorer (UR_CATALOG_SCORER_*)


def catalog_scorer_id(scorer):
    """None | "vector" | "mfma" -> the value of ur_catalog_select_t.scorer; anything else is a ValueError."""
    if not (scorer is None or isinstance(scorer, str)) or scorer not in CATALOG_SCORERS:
        raise ValueError(f"catalog scorer must be None, 'vector' or 'mfma', got {scorer!r}")
    return CATALOG_SCORERS[scorer]


# What the five catalogue wrappers below share.  `who` is the wrapper's own name, in every message.
def _catalog_norm(cat_inv_norm, N, dev, who, planes=None):
    """(cat_inv_norm, cat_norm_ready): the caller's inverse norms [N] f32 ([planes,N] for a call on prefixes), or a buffer for the
    library to fill"""
    shape = (N,) if planes is None else (planes, N)
    if cat_inv_norm is None:
        return torch.empty(shape, dtype=F32, device=dev), 0
    if cat_inv_norm.dtype != F32 or cat_inv_norm.shape != shape:
        raise ValueError(f"{who}: cat_inv_norm must be f32 of shape {list(shape)}, got {cat_inv_norm.dtype} {tuple(cat_inv_norm.shape)}")
    _need(cat_inv_norm, F32, "cat_inv_norm")
    return cat_inv_norm, 1


def _catalog_operands(who, user, catalog, cat_inv_norm, planes=None):
    """The operand checks: catalog's dtype, user [B,D] f32 and catalog [N,D] sharing D, cat_inv_norm [N] f32 ([planes,N] when given) --
    the shapes first, as ValueErrors, so that a call which would be read out of bounds is refused whatever else is wrong with it -- then
    device and contiguity.
    Returns (B, N, D, device, cat_inv_norm, cat_norm_ready)."""
    if catalog.dtype not in (F32, BF16):
        raise ValueError(f"{who}: catalog must be f32 or bf16, got {catalog.dtype}")
    if user.dim() != 2 or catalog.dim() != 2 or catalog.shape[1] != user.shape[1]:
        raise ValueError(f"{who}: user [B,D] and catalog [N,D] must share D, got {tuple(user.shape)} and {tuple(catalog.shape)}")
    (B, D), N = user.shape, catalog.shape[0]
    cat_inv_norm, ready = _catalog_norm(cat_inv_norm, N, user.device, who, planes)
    _need(user, F32, f"{who}: user")
    _need(catalog, catalog.dtype, f"{who}: catalog")
    return B, N, D, user.device, cat_inv_norm, ready


def _catalog_lists(a, B, K, dev):
    """the output lists [B,K] of a call, entered into its argument struct"""
    idx = torch.empty((B, max(K, 0)), dtype=torch.int32, device=dev)
    val = torch.empty((B, max(K, 0)), dtype=F32, device=dev)
    a.topk_index, a.topk_score = idx.data_ptr(), val.data_ptr()
    return idx, val


def _catalog_filters(who, a, B, dev, gt_index, exclude, want_rank=True):
    """gt_index [B] (with the rank output it asks for, unless want_rank is False) and exclude [B,E], entered into the argument struct.
    Returns (gt, rank): gt is the tensor the struct points to and must outlive the call."""
    gt = rank = None
    if gt_index is not None:
        gt = gt_index.to(device=dev, dtype=torch.int64).contiguous()
        if gt.shape != (B,):
            raise ValueError(f"{who}: gt_index must have shape [{B}], got {tuple(gt.shape)}")
        a.gt_index = gt.data_ptr()
        if want_rank:
            rank = torch.empty((B,), dtype=torch.int32, device=dev)
            a.rank = rank.data_ptr()
    if exclude is not None:
        _need(exclude, torch.int64, "exclude")
        if exclude.dim() != 2 or exclude.shape[0] != B:
            raise ValueError(f"{who}: exclude must be [{B}, E], got {tuple(exclude.shape)}")
        a.E = exclude.shape[1]
        a.exclude = exclude.data_ptr() if a.E else None
    return gt, rank


def _catalog_call(entry, a, dev, tag, *args):
    """entry(*args, &a, stream) twice: the size query (a.workspace is NULL), then the call with workspace(tag)"""
    fn = getattr(_lib.load(), entry)

    def call():
        check(fn(*args, ctypes.byref(a), _stream()), entry)
    call()
    a.workspace = workspace(a.workspace_bytes, dev, tag).data_ptr()
    call()


def catalog_select(user, catalog, K, cat_inv_norm=None, gt_index=None, exclude=None, chunk_rows=None, scorer=None):
    """Streaming retrieval over a shared catalogue [N,D] f32 or bf16 (ur_catalog_scores with a ur_catalog_select_t): the K best items per
    user of user [B,D] f32 under catalog_scores' own f32 scores, descending, lowest index first among equal scores; no [B,N] tensor
    exists.  A bf16 catalogue is widened exactly as it is read and gives what catalog.float() gives, bit for bit.
    gt_index int64 [B]: also the 1-based rank of that item (1 + the number of strictly greater scores).  exclude int64 [B,E], rows
    sorted ascending with negative entries as empty slots: those items are left out of the list and of the count, except the user's
    own gt_index.  chunk_rows: catalogue rows scored per chunk (a multiple of 1024; None = the library's choice).
    scorer: the kernel that scores a chunk, "vector" or "mfma" (f32 matrix cores); both give the same bits, None = the library's choice.
    Returns (topk_index int32 [B,K], topk_score f32 [B,K], rank int32 [B] or None, cat_inv_norm); with fewer than K candidates the
    tail of a row is index -1, score -inf."""
    scorer_id = catalog_scorer_id(scorer)
    B, N, D, dev, cat_inv_norm, ready = _catalog_operands("catalog_select", user, catalog, cat_inv_norm)
    sel = CatalogSelect()
    sel.K, sel.chunk_rows = int(K), int(chunk_rows or 0)
    sel.catalog_bf16, sel.scorer = int(catalog.dtype == BF16), scorer_id
    idx, val = _catalog_lists(sel, B, sel.K, dev)
    gt, rank = _catalog_filters("catalog_select", sel, B, dev, gt_index, exclude)
    uinv = torch.empty((B,), dtype=F32, device=dev)
    _catalog_call("ur_catalog_scores", sel, dev, "catalog_select",
                  user.data_ptr(), catalog.data_ptr(), None, uinv.data_ptr(), cat_inv_norm.data_ptr(), ready, B, N, D)
    return idx, val, rank, cat_inv_norm


CATALOG_DEEP_TOPK_MAX = _lib.CATALOG_DEEP_TOPK_MAX      # UR_CATALOG_DEEP_TOPK_MAX


def catalog_deep_select(user, catalog, K, cat_inv_norm=None, gt_index=None, exclude=None, chunk_rows=None, scorer=None, segments=None):
    """catalog_select with lists of up to CATALOG_DEEP_TOPK_MAX = 1024 items (ur_catalog_deep_select, include/unirec_hip_deep.h): the
    same f32 scores bit for bit, the same total order (score descending, lowest index first), the same gt_index / rank, exclude,
    chunk_rows and scorer arguments and the same (-1, -inf) tail; for K <= 128 the same outputs in every bit.  The selection kernel
    defers its merges and several workgroups share a user's chunk row; neither shows in the result.
    segments: for tests -- the number of workgroups per user (1 .. 16) instead of the library's choice from B and the CU count; the
    outputs do not depend on it.
    Returns (topk_index int32 [B,K], topk_score f32 [B,K], rank int32 [B] or None, cat_inv_norm)."""
    scorer_id = catalog_scorer_id(scorer)
    a = _lib.CatalogDeep()
    a.B, a.N, a.D, dev, cat_inv_norm, a.cat_norm_ready = _catalog_operands("catalog_deep_select", user, catalog, cat_inv_norm)
    a.user, a.catalog, a.cat_inv_norm = user.data_ptr(), catalog.data_ptr(), cat_inv_norm.data_ptr()
    a.catalog_bf16, a.scorer = int(catalog.dtype == BF16), scorer_id
    a.K, a.chunk_rows, a.segments = int(K), int(chunk_rows or 0), int(segments or 0)
    idx, val = _catalog_lists(a, a.B, a.K, dev)
    gt, rank = _catalog_filters("catalog_deep_select", a, a.B, dev, gt_index, exclude)
    _catalog_call("ur_catalog_deep_select", a, dev, "catalog_deep")
    return idx, val, rank, cat_inv_norm


COARSE_USER_GROUP = _lib.COARSE_USER_GROUP      # users a workgroup of the coarse scorer stages (half of it when D > 1024)


def catalog_coarse_select(user, catalog, K, cat_inv_norm=None, gt_index=None, exclude=None, chunk_rows=None):
    """The APPROXIMATE shortlist pass over a bf16 catalogue [N,D] (ur_catalog_coarse_select, include/unirec_hip_coarse.h): catalog_select
    with the chunks scored on the bf16 matrix cores.  The coarse score of (b, n) is the cosine of user b ROUNDED to bf16 with row n, summed
    in f32 by v_mfma_f32_16x16x32_bf16 -- what catalog_select(user.bfloat16().float(), catalog) computes in f32 chains, up to the order of
    the sum.  Lists (K <= 128), total order, gt_index / rank, exclude, chunk_rows and the (-1, -inf) tail are catalog_select's; the scores
    and the rank are coarse ones.  D must be a multiple of 8 and the catalogue bf16 (``CatalogEvaluator(dtype=torch.bfloat16)``).
    Returns (topk_index int32 [B,K], topk_score f32 [B,K], rank int32 [B] or None, cat_inv_norm)."""
    if catalog.dtype != BF16:
        raise ValueError(f"catalog_coarse_select: the coarse scorer reads a bf16 catalogue (CatalogEvaluator(dtype=torch.bfloat16)), got {catalog.dtype}")
    a = _lib.CatalogCoarse()
    a.B, a.N, a.D, dev, cat_inv_norm, a.cat_norm_ready = _catalog_operands("catalog_coarse_select", user, catalog, cat_inv_norm)
    a.user, a.catalog, a.cat_inv_norm, a.catalog_bf16 = user.data_ptr(), catalog.data_ptr(), cat_inv_norm.data_ptr(), 1
    a.K, a.chunk_rows = int(K), int(chunk_rows or 0)
    idx, val = _catalog_lists(a, a.B, a.K, dev)
    gt, rank = _catalog_filters("catalog_coarse_select", a, a.B, dev, gt_index, exclude)
    _catalog_call("ur_catalog_coarse_select", a, dev, "catalog_coarse")
    return idx, val, rank, cat_inv_norm


def catalog_rerank(user, catalog, index, k=None, cat_inv_norm=None):
    """The EXACT scores of a shortlist (ur_catalog_rerank): index int32 [B,K'] into catalog [N,D] f32 or bf16, an entry outside [0,N)
    (-1) an empty slot.  Every pair is scored by catalog_scores' own f32 chain -- the bits catalog_scores / catalog_select give for it --
    and each row is sorted under their total order (score descending, index ascending); the first k (default K') are returned, empty
    slots at the tail as (-1, -inf).  Returns (topk_index int32 [B,k], topk_score f32 [B,k], cat_inv_norm)."""
    a = _lib.CatalogRerank()
    a.B, a.N, a.D, dev, cat_inv_norm, a.cat_norm_ready = _catalog_operands("catalog_rerank", user, catalog, cat_inv_norm)
    a.user, a.catalog, a.cat_inv_norm = user.data_ptr(), catalog.data_ptr(), cat_inv_norm.data_ptr()
    a.catalog_bf16 = int(catalog.dtype == BF16)
    _need(index, torch.int32, "index")
    if index.dim() != 2 or index.shape[0] != a.B:
        raise ValueError(f"catalog_rerank: index must be [{a.B}, K'], got {tuple(index.shape)}")
    a.index, a.K_in = index.data_ptr(), index.shape[1]
    a.k = index.shape[1] if k is None else int(k)
    idx, val = _catalog_lists(a, a.B, a.k, dev)
    _catalog_call("ur_catalog_rerank", a, dev, "catalog_rerank")
    return idx, val, cat_inv_norm


def catalog_coarse_deep_select(user, catalog, K, cat_inv_norm=None, gt_index=None, exclude=None, chunk_rows=None, segments=None):
    """catalog_coarse_select with lists of up to CATALOG_DEEP_TOPK_MAX = 1024 items (ur_catalog_coarse_deep_select,
    include/unirec_hip_coarse_deep.h): the same APPROXIMATE coarse scores bit for bit -- the same cast, norms and bf16-MFMA launches --
    folded by the selection kernels of catalog_deep_select.  Total order, gt_index / rank, exclude, chunk_rows and the (-1, -inf) tail
    are catalog_coarse_select's; for K <= 128 so is every output bit, and for larger K the first 128 entries and the rank are those of
    K = 128.  D must be a multiple of 8 and the catalogue bf16.
    segments: for tests -- the number of workgroups per user (1 .. 16) instead of the library's choice; the outputs do not depend on it.
    Returns (topk_index int32 [B,K], topk_score f32 [B,K], rank int32 [B] or None, cat_inv_norm)."""
    if catalog.dtype != BF16:
        raise ValueError("catalog_coarse_deep_select: the coarse scorer reads a bf16 catalogue (CatalogEvaluator(dtype=torch.bfloat16)), "
                         f"got {catalog.dtype}")
    a = _lib.CatalogCoarseDeep()
    a.B, a.N, a.D, dev, cat_inv_norm, a.cat_norm_ready = _catalog_operands("catalog_coarse_deep_select", user, catalog, cat_inv_norm)
    a.user, a.catalog, a.cat_inv_norm, a.catalog_bf16 = user.data_ptr(), catalog.data_ptr(), cat_inv_norm.data_ptr(), 1
    a.K, a.chunk_rows, a.segments = int(K), int(chunk_rows or 0), int(segments or 0)
    idx, val = _catalog_lists(a, a.B, a.K, dev)
    gt, rank = _catalog_filters("catalog_coarse_deep_select", a, a.B, dev, gt_index, exclude)
    _catalog_call("ur_catalog_coarse_deep_select", a, dev, "catalog_coarse_deep")
    return idx, val, rank, cat_inv_norm


def catalog_deep_rerank(user, catalog, index, k=None, cat_inv_norm=None):
    """catalog_rerank for shortlists of up to CATALOG_DEEP_TOPK_MAX = 1024 items (ur_catalog_deep_rerank,
    include/unirec_hip_coarse_deep.h): index int32 [B,K'] into catalog [N,D] f32 or bf16, an entry outside [0,N) an empty slot.  Every
    pair is scored by catalog_scores' own f32 chain, one wave per pair in a launch of its own, and each row is sorted under the total
    order (score descending, index ascending); the first k (default K') are returned, empty slots at the tail as (-1, -inf).  For
    K' <= 128 the outputs equal catalog_rerank's in every bit.  Returns (topk_index int32 [B,k], topk_score f32 [B,k], cat_inv_norm)."""
    a = _lib.CatalogDeepRerank()
    a.B, a.N, a.D, dev, cat_inv_norm, a.cat_norm_ready = _catalog_operands("catalog_deep_rerank", user, catalog, cat_inv_norm)
    a.user, a.catalog, a.cat_inv_norm = user.data_ptr(), catalog.data_ptr(), cat_inv_norm.data_ptr()
    a.catalog_bf16 = int(catalog.dtype == BF16)
    _need(index, torch.int32, "catalog_deep_rerank: index")
    if index.dim() != 2 or index.shape[0] != a.B:
        raise ValueError(f"catalog_deep_rerank: index must be [{a.B}, K'], got {tuple(index.shape)}")
    a.index, a.K_in = index.data_ptr(), index.shape[1]
    a.k = index.shape[1] if k is None else int(k)
    idx, val = _catalog_lists(a, a.B, a.k, dev)
    _catalog_call("ur_catalog_deep_rerank", a, dev, "catalog_deep_rerank")
    return idx, val, cat_inv_norm


def _funnel_operands(who, user, catalog, dim, cat_inv_norm):
    """The operand checks of the funnel wrappers: user [B,Du] f32 and catalog [N,Dc] f32 or bf16, both taken whole -- only their first
    `dim` components are read, with the row strides Du and Dc, and no copy is made -- and cat_inv_norm [N] f32, the plane of this prefix.
    Returns (B, N, dim, ld, ldu, device, cat_inv_norm, cat_norm_ready)."""
    if catalog.dtype not in (F32, BF16):
        raise ValueError(f"{who}: catalog must be f32 or bf16, got {catalog.dtype}")
    if isinstance(dim, bool) or not isinstance(dim, int):
        raise ValueError(f"{who}: dim must be an int, got {dim!r}")
    if user.dim() != 2 or catalog.dim() != 2 or not 0 < dim <= min(user.shape[1], catalog.shape[1]):
        raise ValueError(f"{who}: user [B,Du] and catalog [N,Dc] must both hold the prefix dim = {dim}, got {tuple(user.shape)} and "
                         f"{tuple(catalog.shape)}")
    B, N = user.shape[0], catalog.shape[0]
    cat_inv_norm, ready = _catalog_norm(cat_inv_norm, N, user.device, who)
    _need(user, F32, f"{who}: user")
    _need(catalog, catalog.dtype, f"{who}: catalog")
    return B, N, dim, catalog.shape[1], user.shape[1], user.device, cat_inv_norm, ready


def catalog_prefix_norms(catalog, dims):
    """The inverse norms of len(dims) prefixes of every row of catalog [N,D] f32 or bf16 (ur_catalog_prefix_norms,
    include/unirec_hip_funnel.h) -> inv f32 [L,N]: plane l holds, bit for bit, the cat_inv_norm the catalogue wrappers compute on the
    contiguous slice catalog[:, :dims[l]].  The catalogue is read once, in place, for all planes.  dims: what mrl_dims accepts (1 to
    MRL_MAX_DIMS ascending multiples of 4), multiples of 8 for a bf16 catalogue, the last at most D."""
    who = "catalog_prefix_norms"
    dims = mrl_dims(dims, "dims")
    if catalog.dtype not in (F32, BF16):
        raise ValueError(f"{who}: catalog must be f32 or bf16, got {catalog.dtype}")
    if catalog.dim() != 2:
        raise ValueError(f"{who}: catalog must be [N,D], got {tuple(catalog.shape)}")
    if catalog.dtype == BF16 and any(d % 8 for d in dims):
        raise ValueError(f"dims: every entry must be a multiple of 8 for a bf16 catalogue, got {dims}")
    if dims[-1] > catalog.shape[1]:
        raise ValueError(f"dims: the last entry must be at most the catalogue width {catalog.shape[1]}, got {dims}")
    _need(catalog, catalog.dtype, f"{who}: catalog")
    N, L = catalog.shape[0], len(dims)
    inv = torch.empty((L, N), dtype=F32, device=catalog.device)
    a = _lib.CatalogPrefixNorms()
    a.catalog, a.catalog_bf16, a.N, a.ld, a.L, a.inv = catalog.data_ptr(), int(catalog.dtype == BF16), N, catalog.shape[1], L, inv.data_ptr()
    a.dims[:L] = dims
    check(_lib.load().ur_catalog_prefix_norms(ctypes.byref(a), _stream()), "ur_catalog_prefix_norms")
    return inv


def catalog_funnel_select(user, catalog, dim, K, cat_inv_norm=None, gt_index=None, exclude=None, chunk_rows=None, segments=None):
    """catalog_coarse_deep_select on the first `dim` components of user [B,Du] f32 and of a bf16 catalog [N,Dc], read in place
    (ur_catalog_funnel_select, include/unirec_hip_funnel.h): the tensors are taken whole and their row strides passed, no [N,dim] copy
    exists.  Every output equals, in every bit, catalog_coarse_deep_select(user[:, :dim].contiguous(), catalog[:, :dim].contiguous(), K,
    ...)'s: the APPROXIMATE coarse scores of the prefix, the lists, the rank and the norms.  cat_inv_norm is the [N] plane of THIS prefix
    (a row of catalog_prefix_norms), in, or computed and returned.  dim: a multiple of 8.
    segments: for tests, as in catalog_coarse_deep_select.
    Returns (topk_index int32 [B,K], topk_score f32 [B,K], rank int32 [B] or None, cat_inv_norm)."""
    if catalog.dtype != BF16:
        raise ValueError("catalog_funnel_select: the coarse scorer reads a bf16 catalogue (CatalogEvaluator(dtype=torch.bfloat16)), "
                         f"got {catalog.dtype}")
    a = _lib.CatalogFunnelSelect()
    a.B, a.N, a.dim, a.ld, a.ldu, dev, cat_inv_norm, a.cat_norm_ready = _funnel_operands("catalog_funnel_select", user, catalog, dim, cat_inv_norm)
    a.user, a.catalog, a.cat_inv_norm, a.catalog_bf16 = user.data_ptr(), catalog.data_ptr(), cat_inv_norm.data_ptr(), 1
    a.K, a.chunk_rows, a.segments = int(K), int(chunk_rows or 0), int(segments or 0)
    idx, val = _catalog_lists(a, a.B, a.K, dev)
    gt, rank = _catalog_filters("catalog_funnel_select", a, a.B, dev, gt_index, exclude)
    _catalog_call("ur_catalog_funnel_select", a, dev, "catalog_funnel_select")
    return idx, val, rank, cat_inv_norm


def catalog_funnel_rerank(user, catalog, index, dim, k=None, cat_inv_norm=None):
    """catalog_deep_rerank on the first `dim` components of user [B,Du] f32 and catalog [N,Dc] f32 or bf16, read in place
    (ur_catalog_funnel_rerank, include/unirec_hip_funnel.h): index int32 [B,K'] with K' <= 1024, an entry outside [0,N) an empty slot; the
    index and score bits are catalog_deep_rerank's on the contiguous slices, and with dim == Du == Dc that call's on the same tensors.
    cat_inv_norm is the [N] plane of THIS prefix.  Returns (topk_index int32 [B,k], topk_score f32 [B,k], cat_inv_norm)."""
    a = _lib.CatalogFunnelRerank()
    a.B, a.N, a.dim, a.ld, a.ldu, dev, cat_inv_norm, a.cat_norm_ready = _funnel_operands("catalog_funnel_rerank", user, catalog, dim, cat_inv_norm)
    a.user, a.catalog, a.cat_inv_norm = user.data_ptr(), catalog.data_ptr(), cat_inv_norm.data_ptr()
    a.catalog_bf16 = int(catalog.dtype == BF16)
    _need(index, torch.int32, "catalog_funnel_rerank: index")
    if index.dim() != 2 or index.shape[0] != a.B:
        raise ValueError(f"catalog_funnel_rerank: index must be [{a.B}, K'], got {tuple(index.shape)}")
    a.index, a.K_in = index.data_ptr(), index.shape[1]
    a.k = index.shape[1] if k is None else int(k)
    idx, val = _catalog_lists(a, a.B, a.k, dev)
    _catalog_call("ur_catalog_funnel_rerank", a, dev, "catalog_funnel_rerank")
    return idx, val, cat_inv_norm


FP8_CODES = torch.uint8      # the codes of an fp8 catalogue: e4m3fn bit patterns (codes.view(torch.float8_e4m3fn) is torch's view of them)


def _fp8_operands(who, user, codes, cat_inv_norm):
    """The operand checks of the fp8 wrappers: user [B,D] f32 and codes [N,D] uint8 (or float8_e4m3fn, the same bytes) sharing D, D a
    multiple of 16, cat_inv_norm [N] f32 -- always given: it is the plane catalog_fp8_quantize wrote.  Shapes first, as ValueErrors.
    Returns (B, N, D, device, codes as uint8)."""
    if codes.dtype == torch.float8_e4m3fn:
        codes = codes.view(FP8_CODES)
    if codes.dtype != FP8_CODES:
        raise ValueError(f"{who}: codes must be uint8 or float8_e4m3fn (OCP e4m3fn bit patterns), got {codes.dtype}")
    if user.dim() != 2 or codes.dim() != 2 or codes.shape[1] != user.shape[1]:
        raise ValueError(f"{who}: user [B,D] and codes [N,D] must share D, got {tuple(user.shape)} and {tuple(codes.shape)}")
    (B, D), N = user.shape, codes.shape[0]
    if D % 16:
        raise ValueError(f"{who}: D must be a multiple of 16, got {D}")
    if cat_inv_norm is None or cat_inv_norm.dtype != F32 or cat_inv_norm.shape != (N,):
        got = None if cat_inv_norm is None else (cat_inv_norm.dtype, tuple(cat_inv_norm.shape))
        raise ValueError(f"{who}: cat_inv_norm must be f32 of shape [{N}] (the inv plane of catalog_fp8_quantize), got {got}")
    _need(user, F32, f"{who}: user")
    _need(codes, FP8_CODES, f"{who}: codes")
    _need(cat_inv_norm, F32, f"{who}: cat_inv_norm")
    return B, N, D, user.device, codes


def catalog_fp8_quantize(src, out=None):
    """Rows of src [N,D] f32 or bf16 -> an fp8 catalogue (ur_catalog_fp8_quantize, include/unirec_fp8.h): codes uint8 [N,D], one OCP
    e4m3fn bit pattern per element; scale f32 [N], the power of two 2^-e of the row (e the largest exponent with max|x| 2^e <= 448);
    inv f32 [N], the inverse norm of the row's code values with the bits the row-norm kernel gives codes.float().  Rounding is to
    nearest even into the subnormals with signed zeros, the header's rule in integer arithmetic: the codes are those of
    (src * 2^e).to(torch.float8_e4m3fn) on the CPU.  codes.float() * scale[:, None] decodes exactly.  src may be a view whose rows are
    further apart than D (stride(1) == 1, a row stride that is a multiple of 4); D a multiple of 16, at most 2048.
    out: (codes, scale, inv) to write into, for quantising a catalogue a block of rows at a time.  Returns (codes, scale, inv)."""
    who = "catalog_fp8_quantize"
    if src.dtype not in (F32, BF16):
        raise ValueError(f"{who}: src must be f32 or bf16, got {src.dtype}")
    if src.dim() != 2 or src.shape[1] == 0 or src.shape[1] % 16:
        raise ValueError(f"{who}: src must be [N,D] with D a positive multiple of 16, got {tuple(src.shape)}")
    N, D = src.shape
    ld = src.stride(0) if N > 1 else D
    if src.stride(1) != 1 or ld < D or ld % 4:
        raise ValueError(f"{who}: src must have unit stride along D and a row stride >= D that is a multiple of 4, got strides {src.stride()}")
    if not src.is_cuda:
        raise _lib.UniRecHipError(f"{who}: src: expected a device tensor (the UniRec HIP path has no CPU fallback)")
    dev = src.device
    if out is None:
        out = (torch.empty((N, D), dtype=FP8_CODES, device=dev), torch.empty((N,), dtype=F32, device=dev), torch.empty((N,), dtype=F32, device=dev))
    codes, scale, inv = out
    if codes.shape != (N, D) or scale.shape != (N,) or inv.shape != (N,):
        raise ValueError(f"{who}: out must be (codes [{N},{D}], scale [{N}], inv [{N}]), got {tuple(codes.shape)}, {tuple(scale.shape)}, "
                         f"{tuple(inv.shape)}")
    _need(codes, FP8_CODES, f"{who}: codes")
    _need(scale, F32, f"{who}: scale")
    _need(inv, F32, f"{who}: inv")
    a = _lib.CatalogFp8Quantize()
    a.src, a.src_bf16, a.N, a.D, a.ld = src.data_ptr(), int(src.dtype == BF16), N, D, ld
    a.codes, a.scale, a.inv = codes.data_ptr(), scale.data_ptr(), inv.data_ptr()
    check(_lib.load().ur_catalog_fp8_quantize(ctypes.byref(a), _stream()), "ur_catalog_fp8_quantize")
    return codes, scale, inv


def catalog_fp8_select(user, codes, K, cat_inv_norm, gt_index=None, exclude=None, chunk_rows=None, segments=None):
    """catalog_coarse_deep_select over an fp8 catalogue (ur_catalog_fp8_select, include/unirec_fp8.h): the K <= 1024 best items per user
    of user [B,D] f32 under the APPROXIMATE score s8 -- the users are quantised by catalog_fp8_quantize's rule and the cosine of the two
    code rows is summed in f32 by v_mfma_f32_16x16x32_bf16 on the codes widened in registers (exact products; the error is the order of
    the sum; the fp8 MFMA truncates its products and is not used).  codes uint8 [N,D] and
    cat_inv_norm [N] are catalog_fp8_quantize's codes and inv; the row scales play no part in a cosine.  Total order, gt_index / rank,
    exclude, chunk_rows, segments and the (-1, -inf) tail are catalog_coarse_deep_select's (the same selection kernels).
    Returns (topk_index int32 [B,K], topk_score f32 [B,K], rank int32 [B] or None)."""
    a = _lib.CatalogFp8Select()
    a.B, a.N, a.D, dev, codes = _fp8_operands("catalog_fp8_select", user, codes, cat_inv_norm)
    a.user, a.codes, a.cat_inv_norm = user.data_ptr(), codes.data_ptr(), cat_inv_norm.data_ptr()
    a.K, a.chunk_rows, a.segments = int(K), int(chunk_rows or 0), int(segments or 0)
    idx, val = _catalog_lists(a, a.B, a.K, dev)
    gt, rank = _catalog_filters("catalog_fp8_select", a, a.B, dev, gt_index, exclude)
    _catalog_call("ur_catalog_fp8_select", a, dev, "catalog_fp8_select")
    return idx, val, rank


def catalog_fp8_rerank(user, codes, index, cat_inv_norm, k=None):
    """catalog_deep_rerank over an fp8 catalogue (ur_catalog_fp8_rerank, include/unirec_fp8.h): index int32 [B,K'] with K' <= 1024 into
    codes uint8 [N,D], an entry outside [0,N) an empty slot.  Every pair is scored EXACTLY against the quantised row -- the codes are
    widened as they are read and meet the unrounded f32 user in catalog_scores' own chain -- so the index and score bits are those of
    catalog_deep_rerank(user, codes.float(), index, k, cat_inv_norm).  Returns (topk_index int32 [B,k], topk_score f32 [B,k])."""
    a = _lib.CatalogFp8Rerank()
    a.B, a.N, a.D, dev, codes = _fp8_operands("catalog_fp8_rerank", user, codes, cat_inv_norm)
    a.user, a.codes, a.cat_inv_norm = user.data_ptr(), codes.data_ptr(), cat_inv_norm.data_ptr()
    _need(index, torch.int32, "catalog_fp8_rerank: index")
    if index.dim() != 2 or index.shape[0] != a.B:
        raise ValueError(f"catalog_fp8_rerank: index must be [{a.B}, K'], got {tuple(index.shape)}")
    a.index, a.K_in = index.data_ptr(), index.shape[1]
    a.k = index.shape[1] if k is None else int(k)
    idx, val = _catalog_lists(a, a.B, a.k, dev)
    _catalog_call("ur_catalog_fp8_rerank", a, dev, "catalog_fp8_rerank")
    return idx, val


def catalog_softmax(user, catalog, gt_index, temperature, cat_inv_norm=None, exclude=None, chunk_rows=None, scorer=None, grad_scale=1.0,
                    need_grad=True):
    """The softmax loss over the whole catalogue [N,D] f32 or bf16 (ur_catalog_softmax, include/unirec_hip_loss.h): cross-entropy of
    catalogue row gt_index[b] against every row under catalog_select's own f32 cosine scores divided by `temperature`, streamed in
    chunks (no [B,N] tensor), and grad_scale * d loss / d user.  exclude int64 [B,E], rows sorted ascending with negative entries as empty
    slots: those items leave the sum, except the user's own gt_index.  chunk_rows, scorer: as for catalog_select (the result's bits do
    not depend on the scorer).  need_grad=False runs the forward pass alone.
    Returns (loss f32 [1], row_loss f32 [B], lse f32 [B], d_user f32 [B,D] or None, cat_inv_norm)."""
    scorer_id = catalog_scorer_id(scorer)
    a = _lib.CatalogSoftmax()
    a.B, a.N, a.D, dev, cat_inv_norm, a.cat_norm_ready = _catalog_operands("catalog_softmax", user, catalog, cat_inv_norm)
    a.user, a.catalog, a.cat_inv_norm = user.data_ptr(), catalog.data_ptr(), cat_inv_norm.data_ptr()
    a.catalog_bf16, a.scorer = int(catalog.dtype == BF16), scorer_id
    a.temperature, a.grad_scale, a.chunk_rows = float(temperature), float(grad_scale), int(chunk_rows or 0)
    gt, _ = _catalog_filters("catalog_softmax", a, a.B, dev, gt_index, exclude, want_rank=False)
    loss = torch.empty((1,), dtype=F32, device=dev)
    row_loss = torch.empty((a.B,), dtype=F32, device=dev)
    lse = torch.empty((a.B,), dtype=F32, device=dev)
    d_user = torch.empty((a.B, a.D), dtype=F32, device=dev) if need_grad else None
    a.loss, a.row_loss, a.lse, a.d_user = loss.data_ptr(), row_loss.data_ptr(), lse.data_ptr(), _p(d_user) or None
    _catalog_call("ur_catalog_softmax", a, dev, "catalog_softmax")
    return loss, row_loss, lse, d_user, cat_inv_norm


def catalog_mrl_softmax(user, catalog, gt_index, dims, weights, temperature, cat_inv_norms=None, exclude=None, chunk_rows=None, scorer=None,
                        grad_scale=1.0, need_grad=True):
    """The Matryoshka form of catalog_softmax (ur_catalog_mrl_softmax, include/unirec_hip_mrl_loss.h): catalog_softmax on every prefix
    dims[k] of user [B,D] f32 and catalog [N,D] f32 or bf16, both read in place -- no [N,d_k] copy -- and the weighted sum
    loss = sum_k weights[k] * plane_loss[k] with its gradient.  dims: what mrl_dims accepts, the last one D, multiples of 8 for a bf16
    catalogue; weights: None = all ones, a zero weight keeps the plane's outputs and leaves both sums.  At equal explicit chunk_rows plane
    k's row_loss, lse, plane_loss and norms are, bit for bit, catalog_softmax's on the contiguous slices user[:, :d_k], catalog[:, :d_k].
    cat_inv_norms: f32 [K,N], plane k the norms of prefix dims[k] (catalog_prefix_norms(catalog, dims)), in, or computed and returned.
    gt_index, exclude, temperature, chunk_rows, scorer, grad_scale, need_grad: as for catalog_softmax, shared by all planes.
    Returns (loss f32 [1], plane_loss f32 [K], row_loss f32 [K,B], lse f32 [K,B], d_user f32 [B,D] or None, cat_inv_norms)."""
    who = "catalog_mrl_softmax"
    scorer_id = catalog_scorer_id(scorer)
    dims = mrl_dims(dims, "dims", user.shape[1] if user.dim() == 2 else None)      # (a user that is not [B,D] is refused below)
    K = len(dims)
    weights = mrl_weights(weights, K)
    if catalog.dtype == BF16 and any(d % 8 for d in dims):
        raise ValueError(f"dims: every entry must be a multiple of 8 for a bf16 catalogue, got {dims}")
    a = _lib.CatalogMrlSoftmax()
    a.B, a.N, a.D, dev, cat_inv_norms, a.cat_norm_ready = _catalog_operands(who, user, catalog, cat_inv_norms, planes=K)
    a.user, a.catalog, a.cat_inv_norm = user.data_ptr(), catalog.data_ptr(), cat_inv_norms.data_ptr()
    a.catalog_bf16, a.scorer = int(catalog.dtype == BF16), scorer_id
    a.temperature, a.grad_scale, a.chunk_rows = float(temperature), float(grad_scale), int(chunk_rows or 0)
    a.K = K
    a.dims[:K] = dims
    a.weights[:K] = weights
    gt, _ = _catalog_filters(who, a, a.B, dev, gt_index, exclude, want_rank=False)
    if gt is None:
        raise ValueError(f"{who}: gt_index is needed")
    loss = torch.empty((1,), dtype=F32, device=dev)
    plane_loss = torch.empty((K,), dtype=F32, device=dev)
    row_loss = torch.empty((K, a.B), dtype=F32, device=dev)
    lse = torch.empty((K, a.B), dtype=F32, device=dev)
    d_user = torch.empty((a.B, a.D), dtype=F32, device=dev) if need_grad else None
    a.loss, a.plane_loss, a.row_loss, a.lse, a.d_user = loss.data_ptr(), plane_loss.data_ptr(), row_loss.data_ptr(), lse.data_ptr(), _p(d_user) or None
    _catalog_call("ur_catalog_mrl_softmax", a, dev, who)
    return loss, plane_loss, row_loss, lse, d_user, cat_inv_norms


def rank_of_index(scores, gt_index):
    """1-based rank of column gt_index[b] in the descending order of scores[b] (ties go to the ground truth)."""
    lib = _lib.load()
    _need(scores, F32, "scores")
    B, N = scores.shape
    gt = gt_index.to(device=scores.device, dtype=torch.int64).contiguous()
    rank = torch.empty((B,), dtype=torch.int32, device=scores.device)
    check(lib.ur_rank_of_index(scores.data_ptr(), gt.data_ptr(), rank.data_ptr(), B, N, _stream()), "ur_rank_of_index")
    return rank


def lora_bgrad_args(dy, t, Bt, cols, gB, alpha=1.0, out=None):
    """(the LoraArgs of lora_bgrad for these tensors, out) -- what the launch passes and what lora_plan("bgrad", ...) is asked with"""
    r = _lora_rank(Bt[0].shape[0], "lora_bgrad")
    for e, u in enumerate(Bt):
        if u.dtype != BF16 or u.dim() != 2 or u.shape[0] != r or u.stride(1) != 1 or u.shape[1] != cols[e][1]:
            raise ValueError(f"lora_bgrad: Bt[a] must be bf16 [{r}, width_a]")
    if t.dtype != BF16 or t.stride(1) != 1 or t.shape[0] != dy.shape[0] or t.shape[1] < r * len(cols):
        raise ValueError(f"lora_bgrad: t must be bf16 [M, >= {r} nad]")
    _need(gB, F32, "gB")
    if gB.numel() != r * sum(w for _, w in cols):
        raise ValueError("lora_bgrad: gB has the wrong size")
    if out is None:
        out = torch.empty((dy.shape[0], r * len(cols)), dtype=BF16, device=dy.device)
    return _lora_fill(dy, cols, False, None, alpha, r, [(u.data_ptr(), u.stride(0)) for u in Bt], (out.data_ptr(), out.stride(0)), (t.data_ptr(), t.stride(0)),
                      gB.data_ptr(), True), out


@_stream_family("lora_bgrad", lambda r, dy, t, Bt, cols, gB, alpha=1.0, out=None: _cols_bytes(dy, cols) + 2 * dy.shape[0] * 2 * Bt[0].shape[0] * len(cols))
def lora_bgrad(dy, t, Bt, cols, gB, alpha=1.0, out=None):
    """One pass over dy: returns tb [M, r nad] = alpha * dy_a B_a (Bt: list of B_a^T [r, width_a], r in LORA_RANKS) and fills
    gB [sum width, r] f32 with dB_a = dy_a^T t_a (adapter a owns columns cols[a] of dy, t holds t_a at columns r a)."""
    lib = _lib.load()
    a, out = lora_bgrad_args(dy, t, Bt, cols, gB, alpha, out)
    wsb = lib.ur_lora_bgrad_workspace_bytes(ctypes.byref(a))
    ws = workspace(wsb, dy.device, "lora").data_ptr() if wsb else 0
    check(lib.ur_lora_bgrad(ctypes.byref(a), ws, wsb, _stream()), "ur_lora_bgrad")
    return out


def context_mlp1(x, kind, W1, b1):
    """bf16 [n, 2H] = gelu(W1 feat(x) + b1); kind 0: x = f32 timestamps [n]; kind 1: x = f32 (lat, lon) [n,2]."""
    lib = _lib.load()
    _need(x, F32, "x")
    _need(W1, F32, "W1")
    _need(b1, F32, "b1")
    n = x.shape[0]
    out = torch.empty((n, W1.shape[0]), dtype=BF16, device=x.device)
    check(lib.ur_context_mlp1(x.data_ptr(), int(kind), W1.data_ptr(), b1.data_ptr(), out.data_ptr(), n, W1.shape[0], _stream()), "ur_context_mlp1")
    return out


# ---- heads / losses ------------------------------------------------------------------------------
def gelu_bwd(dy, u):
    lib = _lib.load()
    dx = torch.empty_like(u)
    check(lib.ur_gelu_bwd(dy.data_ptr(), u.data_ptr(), dx.data_ptr(), u.numel(), _stream()), "ur_gelu_bwd")
    return dx


def _heads_ws(Q, F, device):
    lib = _lib.load()
    n = max(lib.ur_heads_workspace_bytes(Q, F), 4096 * 4)
    return workspace(n, device, "heads"), n


def field_projection_fwd(rec16, Wf, bf):
    """rec16 [B,Q,E] bf16, Wf [F,Q] f32, bf [F] f32 -> [B,F,E] f32."""
    lib = _lib.load()
    B, Q, E = rec16.shape
    F_ = Wf.shape[0]
    out = torch.empty((B, F_, E), dtype=F32, device=rec16.device)
    check(lib.ur_field_projection_fwd(rec16.data_ptr(), Wf.data_ptr(), bf.data_ptr(), out.data_ptr(), B, Q, F_, E, _stream()),
          "ur_field_projection_fwd")
    return out


def field_projection_bwd(dout, rec16, Wf, dWf, dbf):
    lib = _lib.load()
    B, Q, E = rec16.shape
    F_ = Wf.shape[0]
    drec = torch.empty_like(rec16)
    ws, n = _heads_ws(Q, F_, rec16.device)
    check(lib.ur_field_projection_bwd(dout.data_ptr(), rec16.data_ptr(), Wf.data_ptr(), drec.data_ptr(), dWf.data_ptr(), dbf.data_ptr(),
                                      B, Q, F_, E, ws.data_ptr(), n, _stream()), "ur_field_projection_bwd")
    return drec


def recon_stats(rec, x, mask):
    """f32 [rows,E] x2 + f32 mask [rows] -> sums3 = (sum mask*se, sum mask, sum cos over valid rows)."""
    lib = _lib.load()
    E = rec.shape[-1]
    rows = rec.numel() // E
    sums = torch.empty((3,), dtype=F32, device=rec.device)
    ws, n = _heads_ws(1, 1, rec.device)
    check(lib.ur_recon_stats(rec.data_ptr(), x.data_ptr(), mask.data_ptr(), sums.data_ptr(), rows, E, ws.data_ptr(), n, _stream()),
          "ur_recon_stats")
    return sums


def recon_grad(rec, x, mask, sums, coef):
    lib = _lib.load()
    E = rec.shape[-1]
    rows = rec.numel() // E
    d = torch.empty_like(rec)
    check(lib.ur_recon_grad(rec.data_ptr(), x.data_ptr(), mask.data_ptr(), sums.data_ptr(), coef, d.data_ptr(), rows, E, _stream()),
          "ur_recon_grad")
    return d


def triplet_margin(anchor, pos, neg, margin, coef, need_grad=True):
    lib = _lib.load()
    B, E = anchor.shape
    loss = torch.empty((1,), dtype=F32, device=anchor.device)
    da = torch.empty_like(anchor) if need_grad else None
    ws, n = _heads_ws(1, 1, anchor.device)
    if n < 4 * B:
        ws, n = workspace(4 * B, anchor.device, "heads"), 4 * B
    check(lib.ur_triplet_margin(anchor.data_ptr(), pos.data_ptr(), neg.data_ptr(), margin, coef, loss.data_ptr(), _p(da), B, E,
                                ws.data_ptr(), n, _stream()), "ur_triplet_margin")
    return loss, da


def mse_loss(a, b, coef=1.0, need_grad=True):
    lib = _lib.load()
    loss = torch.empty((1,), dtype=F32, device=a.device)
    da = torch.empty_like(a) if need_grad else None
    ws, n = _heads_ws(1, 1, a.device)
    check(lib.ur_mse_loss(a.data_ptr(), b.data_ptr(), a.numel(), coef, loss.data_ptr(), _p(da), ws.data_ptr(), n, _stream()),
          "ur_mse_loss")
    return loss, da


def user_sequence_assemble(item_tokens, context, lengths, dropout_p=0.0, seed=0, drop_batch0=0):
    """item_tokens [B,L,Qi,H] bf16, context [B,L,H] bf16, lengths int32 [B] -> (out [B,L*Qi,H] bf16, mask [B,L*Qi] f32)."""
    lib = _lib.load()
    _need(item_tokens, BF16, "item_tokens")
    _need(context, BF16, "context")
    _need(lengths, torch.int32, "lengths")
    B, L, Qi, H = item_tokens.shape
    out = torch.empty((B, L * Qi, H), dtype=BF16, device=item_tokens.device)
    mask = torch.empty((B, L * Qi), dtype=F32, device=item_tokens.device)
    check(lib.ur_user_sequence_assemble(item_tokens.data_ptr(), context.data_ptr(), lengths.data_ptr(), out.data_ptr(), mask.data_ptr(),
                                        B, L, Qi, H, dropout_p, seed, int(drop_batch0), _stream()), "ur_user_sequence_assemble")
    return out, mask

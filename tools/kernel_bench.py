#!/usr/bin/env python3
"""Micro-benchmarks of the individual hot kernels (attention fwd/bwd, projection GEMMs) at the C4
shapes; used under rocprofv3 (--kernel-trace / --pmc) when tuning.  Usage:
    python tools/kernel_bench.py attn|gemm|lora [--B 8] [--iters 5]
    python tools/kernel_bench.py catalog --B 512 --N 1000000 --K 100 [--D 1024] [--rounds 3] [--chunks]
    python tools/kernel_bench.py catalog --B 512 --N 1000000 --K 100 --scorer vector mfma --catalog-dtype bf16
    python tools/kernel_bench.py catalog --K 1000 --dtypes f32 bf16 --users 512 64 [--N 1000000] [--D 1024] [--rounds 5] [--segments 1 4 16]
    python tools/kernel_bench.py catalog --shortlist 128 --catalog-dtype bf16 [--N 1000000] [--D 1024] [--rounds 3]
    python tools/kernel_bench.py catalog --two-stage-shortlist 1024 --K 1000 --catalog-dtype bf16 [--users 512 64] [--rounds 5]
    python tools/kernel_bench.py catalog --funnel-dims 256 1024 --funnel-shortlists 1024 --K 1000 [--users 512 64] [--rounds 5]
    python tools/kernel_bench.py catalog --fp8 --K 1000 --two-stage-shortlist 1024 [--users 512 64] [--rounds 5]
    python tools/kernel_bench.py negatives --B 64 --P 1000 --N 1000000 --K 128 [--catalog-dtype f32|bf16] [--rounds 3]
    python tools/kernel_bench.py catalog_softmax --users 64 512 --dtypes f32 bf16 --N 1000000 [--D 1024] [--rounds 5]
    python tools/kernel_bench.py catalog_mrl_softmax --users 64 512 --dtypes f32 bf16 --dims 64,128,256,512,1024 [--N 1000000] [--rounds 5]
    python tools/kernel_bench.py merge --B 64 --S 2048 [--layers 28] [--rank 16] [--rounds 5] [--iters 2]
    python tools/kernel_bench.py pool --B 64 --S 2048 [--D 1024] [--rounds 5] [--iters 20]
    python tools/kernel_bench.py mrl --B 64 --N 999 --D 1024 --dims 64,128,256,512,1024 [--rounds 5] [--iters 20]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from unirec_amd import hip


def timeit(fn, iters):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def attn(args):
    B, S, nq, nkv, hd = args.B, args.S, 16, 8, 128
    g = torch.Generator().manual_seed(0)
    qkv = (torch.randn(B, S, (nq + 2 * nkv) * hd, generator=g)).cuda().to(torch.bfloat16)
    q = qkv[..., :nq * hd].view(B, S, nq, hd); k = qkv[..., nq * hd:(nq + nkv) * hd].view(B, S, nkv, hd); v = qkv[..., (nq + nkv) * hd:].view(B, S, nkv, hd)
    dout = torch.randn(B, S, nq, hd, generator=g).cuda().to(torch.bfloat16)
    fl = 4 * B * nq * S * S * hd / 2
    o, ctx = hip.attn_fwd(q, k, v, causal=True)
    t = timeit(lambda: hip.attn_fwd(q, k, v, causal=True), args.iters)
    print(f"attn fwd  B={B} S={S}: {t:.3f} ms  {fl / t / 1e9:.1f} TFLOP/s")
    t = timeit(lambda: hip.attn_bwd(ctx, dout), args.iters)
    print(f"attn bwd  B={B} S={S}: {t:.3f} ms  {2.5 * fl / t / 1e9:.1f} TFLOP/s (2.5x fwd flops; 3.5x executed)")


def gemm(args):
    M = args.B * args.S
    g = torch.Generator().manual_seed(0)
    for (N, K, rk, sk, name) in [(2048, 1024, True, True, "q_proj fwd"), (3072, 1024, True, True, "gate fwd"), (1024, 3072, True, True, "down fwd"),
                                 (1024, 4096, True, False, "dX qkv"), (3072, 1024, True, False, "dX down"), (1024, 6144, True, False, "dX gate|up")]:
        R = torch.randn(M, K, generator=g).cuda().to(torch.bfloat16)
        S_ = (torch.randn(N, K, generator=g) if sk else torch.randn(K, N, generator=g)).cuda().to(torch.bfloat16) * 0.05
        out = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        t = timeit(lambda: hip.gemm(R, S_, r_kcontig=rk, s_kcontig=sk, out=out), args.iters)
        line = f"gemm {name:12s} M={M} N={N} K={K}: {t:.3f} ms  {2 * M * N * K / t / 1e9:.1f} TFLOP/s"
        if args.lib:       # reference point only (the product never calls it): the vendor library GEMM torch dispatches to
            Sm = S_ if sk else S_.t()
            tl = timeit(lambda: torch.matmul(R, Sm.t(), out=out), args.iters)
            line += f"   | torch.matmul (hipBLASLt / rocBLAS): {tl:.3f} ms  {2 * M * N * K / tl / 1e9:.1f} TFLOP/s"
        print(line)


def dw(args):
    """Token-reduction (dW) GEMM of the user Q-Former's K|V projection at C3: out[2048,1024] = dKV^T X over 819200
    tokens; token-major operands (K-strided, as the backward has them) against pre-transposed K-contiguous ones."""
    Kt, Mo, No = 512 * 1600, 2048, 1024
    g = torch.Generator().manual_seed(0)
    dy = torch.randn(Kt, Mo, generator=g).cuda().to(torch.bfloat16)
    x = torch.randn(Kt, No, generator=g).cuda().to(torch.bfloat16)
    out = torch.empty(Mo, No, device="cuda")
    fl = 2.0 * Kt * Mo * No
    for sp in (4, 8, 16):
        t = timeit(lambda: hip.gemm(dy, x, r_kcontig=False, s_kcontig=False, out=out, split_k=sp), args.iters)
        print(f"dW token-major  split {sp:2d}: {t:.3f} ms  {fl / t / 1e9:.1f} TFLOP/s")
    ref = out.clone()
    dyT, xT = dy.t().contiguous(), x.t().contiguous()
    for sp in (8, 16):
        t = timeit(lambda: hip.gemm(dyT, xT, r_kcontig=True, s_kcontig=True, out=out, split_k=sp), args.iters)
        print(f"dW transposed   split {sp:2d}: {t:.3f} ms  {fl / t / 1e9:.1f} TFLOP/s   max|diff| vs token-major {float((out - ref).abs().max()):.3e}")
    t = timeit(lambda: hip.transpose_bf16(dy), args.iters)
    print(f"transpose [819200,2048] bf16: {t:.3f} ms")


def xattn(args):
    """User Q-Former cross-attention at C3: 64 queries x 1600 keys, B*heads = 512*16, ragged key mask, p = 0.1."""
    B, nh, Sq, Sk = 512, 16, 64, 1600
    g = torch.Generator().manual_seed(0)
    q = (torch.randn(B, Sq, nh, 64, generator=g) * 0.5).cuda().to(torch.bfloat16)
    kv = (torch.randn(B, Sk, 2, nh, 64, generator=g) * 0.5).cuda().to(torch.bfloat16)
    lens = torch.randint(Sk // 2, Sk + 1, (B,), generator=g)
    km = (torch.arange(Sk)[None, :] < lens[:, None]).to(torch.uint8).cuda()
    dout = torch.randn(B, Sq, nh, 64, generator=g).cuda().to(torch.bfloat16)
    dkv = torch.empty_like(kv)
    for pd in (0.1, 0.0):
        o, ctx = hip.attn_fwd(q, kv[:, :, 0], kv[:, :, 1], causal=False, key_mask=km, dropout_p=pd, seed=3)
        t = timeit(lambda: hip.attn_fwd(q, kv[:, :, 0], kv[:, :, 1], causal=False, key_mask=km, dropout_p=pd, seed=3), args.iters)
        print(f"xattn fwd p={pd}: {t:.3f} ms")
        for sw in ("0", "1"):
            with hip.attn_mode_set(hip.ATTN_MODE_FEWQ, int(sw)):
                t = timeit(lambda: hip.attn_bwd(ctx, dout, dk=dkv[:, :, 0], dv=dkv[:, :, 1]), args.iters)
            print(f"xattn bwd (dq + dkv) p={pd} ur_attn_mode(FEWQ, {sw}): {t:.3f} ms")


def gemm_merge(args):
    """One projection launch over q|k|v (N = 4096) or gate|up (N = 6144) against the separate launches the decoder issues
    today (one per LoRA adapter): what merging them behind a block-diagonal second K range would buy."""
    M, K = args.B * args.S, 1024
    g = torch.Generator().manual_seed(0)
    R = torch.randn(M, K, generator=g).cuda().to(torch.bfloat16)
    for name, parts in (("q|k|v", (2048, 1024, 1024)), ("gate|up", (3072, 3072))):
        N = sum(parts)
        W = (torch.randn(N, K, generator=g) * 0.05).cuda().to(torch.bfloat16)
        out = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        def separate():
            c = 0
            for n in parts:
                hip.gemm(R, W[c:c + n], out=out[:, c:c + n]); c += n
        t1 = timeit(separate, args.iters)
        t2 = timeit(lambda: hip.gemm(R, W, out=out), args.iters)
        print(f"gemm {name:8s} N={N}: separate launches {t1:.3f} ms | one launch {t2:.3f} ms  ({2 * M * N * K / t2 / 1e9:.0f} TFLOP/s)")


STEP_SHAPES = [(4096, 1024, True, "q|k|v fwd"), (1024, 2048, True, "o_proj fwd"), (6144, 1024, True, "gate|up fwd"), (1024, 3072, True, "down fwd"),
               (1024, 4096, False, "dX q|k|v"), (2048, 1024, False, "dX o_proj"), (1024, 6144, False, "dX gate|up")]


def gemm_step(args):
    """The K-contiguous 256x256 projection launches the C4 step actually issues (merged q|k|v and gate|up), ONE launch each
    in a fixed order after one warm-up round -- for the rocprofv3 --pmc passes (tools/gemm_pmc.py maps dispatch order to shape).
    dX launches read the frozen weights' transposed copies, i.e. they are K-contiguous [N,K] operands as well."""
    M = args.B * args.S
    g = torch.Generator().manual_seed(0)
    ops = []
    for (N, K, fwd, name) in STEP_SHAPES:
        R = torch.randn(M, K, generator=g).cuda().to(torch.bfloat16)
        W = (torch.randn(N, K, generator=g) * 0.05).cuda().to(torch.bfloat16)
        ops.append((R, W, torch.empty(M, N, dtype=torch.bfloat16, device="cuda"), name, N, K))
    for rnd in range(2):          # round 0 = warm-up, round 1 = the measured dispatches (the last 7 gemm_kernel dispatches)
        for (R, W, out, name, N, K) in ops:
            hip.gemm(R, W, out=out)
        torch.cuda.synchronize()
    for (R, W, out, name, N, K) in ops:
        t = timeit(lambda: hip.gemm(R, W, out=out), args.iters)
        print(f"gemm {name:12s} M={M} N={N} K={K}: {t:.3f} ms  {2 * M * N * K / t / 1e9:.1f} TFLOP/s")


def rmslora(args):
    """RMSNorm forward + lora_project as two kernels against the fused ur_rmsnorm_lora_fwd (q|k|v: 3 adapters, gate|up: 2)."""
    M, D = args.B * args.S, 1024
    g = torch.Generator().manual_seed(0)
    x = torch.randn(M, D, generator=g).cuda().to(torch.bfloat16)
    w = torch.ones(D).cuda()
    for nad in (3, 2):
        U = [(torch.randn(16, D, generator=g) * 0.05).cuda().to(torch.bfloat16) for _ in range(nad)]
        bits = hip.lora_dropout_bits(1, 0.1, M, D, nad, "cuda")
        t_n = timeit(lambda: hip.rmsnorm_fwd(x, w, 1e-6), args.iters)
        h, _ = hip.rmsnorm_fwd(x, w, 1e-6)
        t_p = timeit(lambda: hip.lora_project(h, U, alpha=2.2, bits=bits), args.iters)
        t_f = timeit(lambda: hip.rmsnorm_lora_fwd(x, w, 1e-6, U, alpha=2.2, bits=bits), args.iters)
        gb = 2.0 * M * D * 2 / 1e9
        print(f"nad={nad}: rmsnorm {t_n * 1e3:.1f} us + project {t_p * 1e3:.1f} us = {(t_n + t_p) * 1e3:.1f} us | fused {t_f * 1e3:.1f} us "
              f"({gb / t_f:.2f} TB/s on x + h)")


def swilora(args):
    """SwiGLU forward + the down adapter's lora_project as two kernels against the fused ur_swiglu_lora_fwd."""
    M, I = args.B * args.S, 3072
    g = torch.Generator().manual_seed(0)
    gu = torch.randn(M, 2 * I, generator=g).cuda().to(torch.bfloat16)
    U = (torch.randn(16, I, generator=g) * 0.05).cuda().to(torch.bfloat16)
    bits = hip.lora_dropout_bits(1, 0.1, M, I, 1, "cuda")
    t_s = timeit(lambda: hip.swiglu_fwd(gu, I), args.iters)
    act = hip.swiglu_fwd(gu, I)
    t_p = timeit(lambda: hip.lora_project(act, [U], alpha=2.2, bits=bits), args.iters)
    t_f = timeit(lambda: hip.swiglu_lora_fwd(gu, I, U, alpha=2.2, bits=bits), args.iters)
    gb = 3.0 * M * I * 2 / 1e9
    print(f"swiglu {t_s * 1e3:.1f} us + project {t_p * 1e3:.1f} us = {(t_s + t_p) * 1e3:.1f} us | fused {t_f * 1e3:.1f} us ({gb / t_f:.2f} TB/s on gate|up + act)")


def gemm_lora(args):
    """What the LoRA term costs inside the projection GEMMs: plain / + second K range (forward: t B^T, K2 = 16) /
    + masked rank-16 epilogue (dX under LoRA dropout)."""
    M, r = args.B * args.S, 16
    g = torch.Generator().manual_seed(0)
    for (N, K, nad, name) in [(2048, 1024, 1, "q fwd"), (3072, 1024, 1, "gate fwd"), (1024, 3072, 1, "down fwd"),
                              (1024, 4096, 3, "dX qkv"), (3072, 1024, 1, "dX down"), (1024, 6144, 2, "dX gate|up")]:
        R = torch.randn(M, K, generator=g).cuda().to(torch.bfloat16)
        S_ = (torch.randn(N, K, generator=g) * 0.05).cuda().to(torch.bfloat16)
        t = torch.randn(M, nad * r, generator=g).cuda().to(torch.bfloat16)
        Bm = (torch.randn(N, nad * r, generator=g) * 0.05).cuda().to(torch.bfloat16)
        bits = hip.lora_dropout_bits(1, 0.1, M, N, nad, "cuda")
        out = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        t0 = timeit(lambda: hip.gemm(R, S_, out=out), args.iters)
        t1 = timeit(lambda: hip.gemm(R, S_, out=out, R2=t, S2=Bm), args.iters)
        t2 = timeit(lambda: hip.gemm(R, S_, out=out, R2=t, S2=Bm, drop=(bits, 0.1, r)), args.iters)
        print(f"gemm {name:12s} N={N} K={K}: plain {t0:.3f} ms | + K2={nad * r} range {t1:.3f} ms | + masked epilogue ({nad} adapters) {t2:.3f} ms")


def rope(args):
    """q/k-norm + RoPE forward / backward over the raw q|k|v projection (16 q + 8 kv heads of 128): TB/s of raw q|k in + q_r|k_r out."""
    M, S, nq, nkv, hd = args.B * args.S, args.S, 16, 8, 128
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(M, (nq + 2 * nkv) * hd, generator=g).cuda().to(torch.bfloat16)
    qn, kn = torch.ones(hd).cuda(), torch.ones(hd).cuda()
    cos, sin = hip.rope_table(S, hd, 1e6, "cuda")
    t = timeit(lambda: hip.qknorm_rope_fwd(qkv, qn, kn, cos, sin, S, nq, nkv, hd, 1e-6), args.iters)
    nb = 2.0 * M * (nq + nkv) * hd * 2
    print(f"qknorm_rope fwd: {t * 1e3:.1f} us  {nb / t / 1e9:.2f} TB/s (raw q|k read + q_r|k_r written)")
    q_r, k_r = hip.qknorm_rope_fwd(qkv, qn, kn, cos, sin, S, nq, nkv, hd, 1e-6)
    dqkv = torch.empty_like(qkv)
    t = timeit(lambda: hip.qknorm_rope_bwd(q_r, k_r, qkv, qn, kn, cos, sin, dqkv, S, nq, nkv, hd, 1e-6), args.iters)
    print(f"qknorm_rope bwd: {t * 1e3:.1f} us  {1.5 * nb / t / 1e9:.2f} TB/s (dq_r|dk_r + raw q|k read, dq|dk raw written)")
    rstd = torch.rsqrt(qkv[:, :(nq + nkv) * hd].float().view(M, nq + nkv, hd).pow(2).mean(-1) + 1e-6)
    t = timeit(lambda: hip.qknorm_rope_bwd_roped(q_r, k_r, q_r, k_r, rstd, qn, kn, cos, sin, dqkv, S, nq, nkv, hd), args.iters)
    print(f"qknorm_rope bwd from the roped outputs: {t * 1e3:.1f} us  {1.5 * nb / t / 1e9:.2f} TB/s")


# the adapter groups of a decoder layer: (name, input width, output widths)
LORA_GROUPS = (("q|k|v", 1024, (2048, 1024, 1024)), ("o", 2048, (1024,)), ("gate|up", 1024, (3072, 3072)), ("down", 3072, (1024,)))


def lora(args):
    """The LoRA side kernels at the C4 shapes (M = B*S tokens; --B 64 is C4), per adapter group and per rank of --ranks: the forward
    projection t = drop(x) A^T, the backward's one pass over dy (tb and dB) and its token reduction dA = tb^T drop(x), with the GB/s
    of the activation each streams (its bytes do not depend on the rank) and the time relative to rank 16 of the same run."""
    M = args.B * args.S
    ranks = [int(r) for r in args.ranks.split(",")]
    g = torch.Generator().manual_seed(0)
    ms = timeit(lambda: hip.lora_dropout_bits(1, 0.1, M, 1024, 3, "cuda"), args.iters)
    print(f"lora bits   3 planes of [M,1024]: {ms * 1e3:7.1f} us  {3 * M * 1024 / 8 / ms / 1e6:7.1f} GB/s   (M = {M}; the planes do not depend on the rank)")
    times = {}
    for gname, win, outs in LORA_GROUPS:
        nad, wout = len(outs), sum(outs)
        x = torch.randn(M, win, generator=g).cuda().to(torch.bfloat16)
        dy = torch.randn(M, wout, generator=g).cuda().to(torch.bfloat16)
        bits = hip.lora_dropout_bits(1, 0.1, M, win, nad, "cuda")
        bits_t = hip.lora_bits_transpose(bits, win)
        cols = [(sum(outs[:j]), n) for j, n in enumerate(outs)]
        for r in ranks:
            A = [(torch.randn(r, win, generator=g) * 0.1).cuda().to(torch.bfloat16) for _ in range(nad)]
            Bt = [(torch.randn(r, n, generator=g) * 0.1).cuda().to(torch.bfloat16) for n in outs]
            t = torch.randn(M, nad * r, generator=g).cuda().to(torch.bfloat16)
            gA, gB = torch.empty(nad * r, win, device="cuda"), torch.empty(wout, r, device="cuda")
            for kname, fn, nbytes in (
                    ("project t  = drop(x) A^T", lambda: hip.lora_project(x, A, alpha=1.1, bits=bits), x.numel() * 2),
                    ("bgrad   tb and dB, one pass", lambda: hip.lora_bgrad(dy, t, Bt, cols, gB), dy.numel() * 2),
                    ("reduce  dA = tb^T drop(x)", lambda: hip.lora_reduce(x, t, gA, nad=nad, alpha=1.1, bits=bits, bits_t=bits_t if r == 16 else None), x.numel() * 2)):
                ms = timeit(fn, args.iters)
                times[(gname, kname, r)] = ms
                rel = f"  x{ms / times[(gname, kname, 16)]:.2f} of rank 16" if (gname, kname, 16) in times else ""
                print(f"lora {gname:8s} r={r:2d} {kname:28s}: {ms * 1e3:7.1f} us  {nbytes / ms / 1e6:7.1f} GB/s{rel}")
        del x, dy, bits, bits_t
    if 16 in ranks:
        for r in ranks:
            tot = sum(v for (gn, kn, rr), v in times.items() if rr == r)
            print(f"lora all groups r={r:2d}: {tot * 1e3:7.1f} us per layer (forward projections + backward streams)  x{tot / sum(v for (gn, kn, rr), v in times.items() if rr == 16):.2f} of rank 16")


def catalog(args):
    """Full-catalogue evaluation: CatalogEvaluator.evaluate() (scores [B,N] + rank_of_index + topk, three kernels) against the streaming
    retrieve() on the same random catalogue and users, alternating --rounds times after one call of each; wall time of the whole call (both
    end in a host read of the metrics) and the peak allocation of a call above the level before it, scratch buffers included.
    --chunks adds retrieve() at half and at double the default rows per chunk.
    --scorer vector mfma times retrieve() once per named scorer instead (alternating in this process, the library's own choice last);
    --catalog-dtype bf16 keeps the catalogue in bf16, where evaluate() does not exist and the first scorer named is the reference."""
    from unirec_amd.evaluation import CatalogEvaluator
    if args.funnel_dims:
        return catalog_funnel(args)
    if args.fp8:
        return catalog_fp8(args)
    if args.two_stage_shortlist:
        return catalog_two_stage(args)
    if args.shortlist:
        return catalog_shortlist(args)
    if args.K > hip.CATALOG_TOPK_MAX:
        return catalog_deep(args)
    B, N, K, D = args.B, args.N, args.K, args.D
    bf16 = args.catalog_dtype == "bf16"
    g = torch.Generator(device="cuda").manual_seed(0)
    cat = torch.randn(N, D, generator=g, device="cuda")
    if bf16:
        cat = cat.to(torch.bfloat16)
    user = torch.randn(B, D, generator=g, device="cuda")
    gt = torch.randint(0, N, (B,), generator=g, device="cuda")
    ev = CatalogEvaluator(cat, dtype=cat.dtype)
    ev.retrieve(user[:1], k=1)                                # the catalogue norms: cached by every path, outside every figure below
    n_up = (N + 1023) // 1024 * 1024
    rows = max(1024, min((64 << 20) // (4 * B) // 1024 * 1024, n_up))           # the library's default (catalog_chunk_rows)
    variants = [] if bf16 else [("evaluate", lambda: ev.evaluate(user, gt, k=K))]
    if args.scorer:
        variants += [(f"retrieve scorer={sc}", lambda sc=sc: ev.retrieve(user, k=K, gt_index=gt, scorer=sc)) for sc in args.scorer]
        variants.append(("retrieve scorer=None (library)", lambda: ev.retrieve(user, k=K, gt_index=gt)))
    else:
        variants.append((f"retrieve (chunk_rows default = {rows})", lambda: ev.retrieve(user, k=K, gt_index=gt)))
    if args.chunks:
        for r in (max(1024, rows // 2 // 1024 * 1024), min(rows * 2, n_up)):
            variants.append((f"retrieve chunk_rows={r}", lambda r=r: ev.retrieve(user, k=K, gt_index=gt, chunk_rows=r)))
    print(f"catalog B={B} N={N} D={D} K={K}: catalogue {args.catalog_dtype} {cat.numel() * cat.element_size() / 2**20:.0f} MiB, "
          f"scores [B,N] f32 {B * N * 4 / 2**20:.0f} MiB, chunk_rows default = {rows}")
    peaks, outs, times = {}, {}, {name: [] for name, _ in variants}
    for name, fn in variants:                                 # first call of each: warm-up, peak allocation with cold scratch, results
        hip._ws_cache.clear()
        torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        outs[name] = fn()
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base
    ref = outs[variants[0][0]]
    for name, _ in variants[1:]:
        o = outs[name]
        same = torch.equal(o["topk_index"], ref["topk_index"]) and torch.equal(o["topk_score"], ref["topk_score"]) and torch.equal(o["rank"], ref["rank"])
        print(f"{name}: lists, scores and ranks equal those of {variants[0][0]}: {same}")
        assert same
    del outs
    for name, fn in variants:                                 # scratch of every variant warm again
        fn()
    for _ in range(args.rounds):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    for name, _ in variants:
        t = sorted(times[name])
        print(f"{name:44s}: median {t[len(t) // 2]:9.2f} ms  min {t[0]:9.2f}  max {t[-1]:9.2f}  (spread {t[-1] - t[0]:.2f} over {len(t)} alternating rounds)"
              f"  peak allocation {peaks[name] / 2**20:9.2f} MiB")


def catalog_deep(args):
    """Long lists (--K above 128, hip.catalog_deep_select) beside the existing call at K = 128, per catalogue dtype (--dtypes, default
    --catalog-dtype) and user count (--users, default 512 and 64), alternating --rounds times in this process after one call of each:
      (a) retrieve(k=128), the existing selection kernel;  (b) hip.catalog_deep_select at K = 128 (held equal to (a) in every bit);
      (c) retrieve(k=--K);  and, with --segments, (c) with that many workgroups per user forced.
    Wall time of the whole call ((a) and (c) end in a host read of the metrics), (c) / (a) and (b) / (a), the number of workgroups per user
    the library chooses, the workspace its size query reports and the peak allocation of (c) against a [B,N] f32 matrix."""
    import ctypes
    from unirec_amd import _lib
    from unirec_amd.evaluation import CatalogEvaluator
    N, D, K = args.N, args.D, args.K
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    g = torch.Generator(device="cuda").manual_seed(0)
    cat32 = torch.randn(N, D, generator=g, device="cuda")
    for dtype in (args.dtypes or [args.catalog_dtype]):
        ev = CatalogEvaluator(cat32, dtype=torch.bfloat16 if dtype == "bf16" else torch.float32)
        for B in (args.users or [512, 64]):
            user = torch.randn(B, D, generator=g, device="cuda")
            gt = torch.randint(0, N, (B,), generator=g, device="cuda")
            ev.retrieve(user[:1], k=1)                        # the catalogue norms: cached by every path, outside every figure below
            rows = max(1024, min((64 << 20) // (4 * B) // 1024 * 1024, (N + 1023) // 1024 * 1024))
            G = max(1, min(4 * cus // B, 1024 // B, 8, rows // 1024))          # deep_segments of unirec_amd/csrc/catalog_deep.hip.h
            q = _lib.CatalogDeep()
            q.B, q.N, q.D, q.K = B, N, D, K
            _lib.check(_lib.load().ur_catalog_deep_select(ctypes.byref(q), None), "ur_catalog_deep_select")
            variants = [("(a) retrieve(k=128)", lambda: ev.retrieve(user, k=128, gt_index=gt)),
                        ("(b) catalog_deep_select K=128", lambda: hip.catalog_deep_select(user, ev.catalog, 128, ev._inv, gt_index=gt)),
                        (f"(c) retrieve(k={K})", lambda: ev.retrieve(user, k=K, gt_index=gt))]
            variants += [(f"    catalog_deep_select K={K} segments={s}", lambda s=s: hip.catalog_deep_select(user, ev.catalog, K, ev._inv, gt_index=gt, segments=s))
                         for s in (args.segments or [])]
            a_out, b_out = variants[0][1](), variants[1][1]()
            same = torch.equal(b_out[0], a_out["topk_index"]) and torch.equal(b_out[1], a_out["topk_score"]) and torch.equal(b_out[2], a_out["rank"])
            assert same, "catalog_deep_select at K = 128 differs from retrieve(k=128)"
            hip._ws_cache.clear()
            torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            c_out = variants[2][1]()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            assert torch.equal(c_out["topk_index"][:, :128], a_out["topk_index"]) and torch.equal(c_out["rank"], a_out["rank"])
            for name, fn in variants:                         # scratch of every variant warm again
                fn()
            times = {name: [] for name, _ in variants}
            for _ in range(args.rounds):
                for name, fn in variants:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) * 1e3)
            print(f"catalog deep: B={B} N={N} D={D} catalogue {dtype}, chunk_rows default = {rows}, {cus} CUs, workgroups per user G = {G}; "
                  f"(b) equals (a) in every bit: {same}; the first 128 of (c) and its ranks equal (a)")
            print(f"  workspace (size query, K={K}): {q.workspace_bytes / 2**20:.2f} MiB; peak allocation of (c): {peak / 2**20:.2f} MiB; "
                  f"scores [B,N] f32: {B * N * 4 / 2**20:.0f} MiB")
            med = {}
            for name, _ in variants:
                t = sorted(times[name])
                med[name] = t[len(t) // 2]
                print(f"  {name:44s}: median {med[name]:9.2f} ms  min {t[0]:9.2f}  max {t[-1]:9.2f}  (spread {t[-1] - t[0]:.2f} over {len(t)} alternating rounds)")
            a, b, c = (v[0] for v in variants[:3])
            print(f"  (c) / (a) = {med[c] / med[a]:.2f}  ((c) - (a) = {med[c] - med[a]:.2f} ms);  (b) / (a) = {med[b] / med[a]:.2f}")
        del ev


def catalog_shortlist(args):
    """The two-stage retrieve(k, shortlist=--shortlist) against the exact retrieve(k) (scorer=None) on the same bf16 catalogue, alternating
    --rounds times in this process after one call of each, at (B, K) = (512, 100) and (64, 10): wall time of the whole call (each ends in a
    host read of the metrics), the ratio of the medians, the recall of the two-stage list against the exact one, and the two stages of the
    two-stage call timed on their own (hip.catalog_coarse_select, hip.catalog_rerank: the split that says which stage holds the time)."""
    from unirec_amd.evaluation import CatalogEvaluator
    N, D, S = args.N, args.D, args.shortlist
    if args.catalog_dtype != "bf16":
        raise SystemExit("catalog --shortlist: the coarse scorer reads a bf16 catalogue; add --catalog-dtype bf16")
    g = torch.Generator(device="cuda").manual_seed(0)
    cat = torch.randn(N, D, generator=g, device="cuda").to(torch.bfloat16)
    ev = CatalogEvaluator(cat, dtype=cat.dtype)
    del cat
    print(f"catalog --shortlist {S}: N={N} D={D}, catalogue bf16 {N * D * 2 / 2**20:.0f} MiB, {args.rounds} alternating rounds")
    for B, K in ((512, 100), (64, 10)):
        user = torch.randn(B, D, generator=g, device="cuda")
        gt = torch.randint(0, N, (B,), generator=g, device="cuda")
        ev.retrieve(user[:1], k=1)                            # the catalogue norms: cached by every path, outside every figure below
        variants = [("exact retrieve (scorer=None)", lambda: ev.retrieve(user, k=K, gt_index=gt)),
                    (f"two-stage retrieve (shortlist={S})", lambda: ev.retrieve(user, k=K, gt_index=gt, shortlist=S)),
                    ("  coarse select alone", lambda: hip.catalog_coarse_select(user, ev.catalog, S, ev._inv, gt_index=gt)),
                    ("  re-rank alone", None)]
        short = hip.catalog_coarse_select(user, ev.catalog, S, ev._inv, gt_index=gt)[0]
        variants[3] = (variants[3][0], lambda: hip.catalog_rerank(user, ev.catalog, short, K, ev._inv))
        outs = {name: fn() for name, fn in variants[:2]}      # warm-up and results
        for name, fn in variants[2:]:
            fn()
        exact, two = outs[variants[0][0]], outs[variants[1][0]]
        hit = (two["topk_index"][:, :, None] == exact["topk_index"][:, None, :]).any(2).float().mean().item()
        same = (two["topk_index"] == exact["topk_index"]).all(1).float().mean().item()
        rank_off = ((two["rank"] - exact["rank"]).abs().double() / exact["rank"].double()).median().item()
        times = {name: [] for name, _ in variants}
        for _ in range(args.rounds):
            for name, fn in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
        print(f"B={B} K={K}: recall@{K} of the two-stage list against the exact one {hit:.6f}; users whose whole list is identical {same:.4f}; "
              f"median |coarse rank - exact rank| / exact rank {rank_off:.2e}")
        med = {}
        for name, _ in variants:
            t = sorted(times[name])
            med[name] = t[len(t) // 2]
            print(f"  {name:40s}: median {med[name]:9.2f} ms  min {t[0]:9.2f}  max {t[-1]:9.2f}  (spread {t[-1] - t[0]:.2f} over {len(t)} alternating rounds)")
        a, b = variants[0][0], variants[1][0]
        gap = med[a] - med[b]
        spread = max(max(times[a]) - min(times[a]), max(times[b]) - min(times[b]))
        print(f"  exact / two-stage = {med[a] / med[b]:.2f}x  (difference {gap:.2f} ms against a spread of {spread:.2f} ms: "
              f"{'faster by more than the spread' if gap > spread else 'NOT faster by more than the spread'})")


def catalog_two_stage(args):
    """CatalogEvaluator.retrieve_two_stage(k=--K, shortlist=--two-stage-shortlist) against the exact retrieve(k=--K) on the same bf16
    catalogue, per user count (--users, default 512 and 64), alternating --rounds times in this process after one call of each; with a
    shortlist of at most 128 the older retrieve(k, shortlist=) alternates as a third contender.  Wall time of the whole call (each ends in
    a host read of the metrics), the ratio of the medians against the alternation's spread, the recall of the two-stage list against the
    exact one and the share of users whose whole list is identical, the two stages timed on their own (hip.catalog_coarse_deep_select,
    hip.catalog_deep_rerank), the workspaces the size queries report and the peak allocation of the two-stage call."""
    import ctypes
    from unirec_amd import _lib
    from unirec_amd.evaluation import CatalogEvaluator
    N, D, S, K = args.N, args.D, args.two_stage_shortlist, args.K
    if args.catalog_dtype != "bf16":
        raise SystemExit("catalog --two-stage-shortlist: the coarse scorer reads a bf16 catalogue; add --catalog-dtype bf16")
    g = torch.Generator(device="cuda").manual_seed(0)
    cat = torch.randn(N, D, generator=g, device="cuda").to(torch.bfloat16)
    ev = CatalogEvaluator(cat, dtype=cat.dtype)
    del cat
    print(f"catalog --two-stage-shortlist {S} --K {K}: N={N} D={D}, catalogue bf16 {N * D * 2 / 2**20:.0f} MiB, {args.rounds} alternating rounds")
    for B in (args.users or [512, 64]):
        user = torch.randn(B, D, generator=g, device="cuda")
        gt = torch.randint(0, N, (B,), generator=g, device="cuda")
        ev.retrieve(user[:1], k=1)                            # the catalogue norms: cached by every path, outside every figure below
        exact_name, two_name = f"exact retrieve(k={K})", f"retrieve_two_stage(k={K}, shortlist={S})"
        variants = [(exact_name, lambda: ev.retrieve(user, k=K, gt_index=gt)),
                    (two_name, lambda: ev.retrieve_two_stage(user, k=K, shortlist=S, gt_index=gt))]
        if S <= hip.CATALOG_TOPK_MAX:
            variants.append((f"retrieve(k={K}, shortlist={S})", lambda: ev.retrieve(user, k=K, gt_index=gt, shortlist=S)))
        short = hip.catalog_coarse_deep_select(user, ev.catalog, S, ev._inv, gt_index=gt)[0]
        variants += [("  coarse-deep select alone", lambda: hip.catalog_coarse_deep_select(user, ev.catalog, S, ev._inv, gt_index=gt)),
                     ("  deep re-rank alone", lambda: hip.catalog_deep_rerank(user, ev.catalog, short, K, ev._inv))]
        exact = variants[0][1]()
        hip._ws_cache.clear()
        torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        two = variants[1][1]()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        for name, fn in variants:                             # scratch of every variant warm again
            fn()
        hit = (two["topk_index"][:, :, None] == exact["topk_index"][:, None, :]).any(2).float().mean().item()
        same = (two["topk_index"] == exact["topk_index"]).all(1).float().mean().item()
        bits = torch.equal(two["topk_score"].view(torch.int32)[two["topk_index"] == exact["topk_index"]],
                           exact["topk_score"].view(torch.int32)[two["topk_index"] == exact["topk_index"]])
        qs, qr = _lib.CatalogCoarseDeep(), _lib.CatalogDeepRerank()
        qs.B, qs.N, qs.D, qs.K, qs.catalog_bf16 = B, N, D, S, 1
        qr.B, qr.N, qr.D, qr.K_in, qr.k, qr.catalog_bf16 = B, N, D, S, K, 1
        _lib.check(_lib.load().ur_catalog_coarse_deep_select(ctypes.byref(qs), None), "ur_catalog_coarse_deep_select")
        _lib.check(_lib.load().ur_catalog_deep_rerank(ctypes.byref(qr), None), "ur_catalog_deep_rerank")
        times = {name: [] for name, _ in variants}
        for _ in range(args.rounds):
            for name, fn in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
        print(f"B={B} K={K} shortlist={S}: recall@{K} of the two-stage list against the exact one {hit:.6f}; users whose whole list is identical "
              f"{same:.4f}; score bits equal where the items agree: {bits}")
        print(f"  workspace (size queries): select {qs.workspace_bytes / 2**20:.2f} MiB, re-rank {qr.workspace_bytes / 2**20:.2f} MiB; peak allocation "
              f"of the two-stage call {peak / 2**20:.2f} MiB; scores [B,N] f32 would be {B * N * 4 / 2**20:.0f} MiB")
        med = {}
        for name, _ in variants:
            t = sorted(times[name])
            med[name] = t[len(t) // 2]
            print(f"  {name:44s}: median {med[name]:9.2f} ms  min {t[0]:9.2f}  max {t[-1]:9.2f}  (spread {t[-1] - t[0]:.2f} over {len(t)} alternating rounds)")
        for a in [v[0] for v in variants[:-2] if v[0] != two_name]:
            gap = med[a] - med[two_name]
            spread = max(max(times[a]) - min(times[a]), max(times[two_name]) - min(times[two_name]))
            print(f"  {a.strip()} / two-stage = {med[a] / med[two_name]:.2f}x  (difference {gap:.2f} ms against a spread of {spread:.2f} ms: "
                  f"{'faster by more than the spread' if gap > spread else 'NOT faster by more than the spread'})")


def catalog_fp8(args):
    """Fp8CatalogEvaluator.retrieve_two_stage(k=--K, shortlist=--two-stage-shortlist) against CatalogEvaluator.retrieve_two_stage on the
    bf16 catalogue it was quantised from, per user count (--users, default 512 and 64), alternating --rounds times in one process after
    one call of each.  Wall time of the whole call, the stages timed on their own (the per-kernel split: hip.catalog_fp8_select /
    hip.catalog_coarse_deep_select, hip.catalog_fp8_rerank / hip.catalog_deep_rerank), the resident bytes of either catalogue, the
    workspaces the size queries report, the peak allocation of a call, and the recall@K of both lists against the exact bf16 retrieve(k)
    on two synthetic catalogues: standard normal rows, and rows whose later components decay (_decaying_catalogue)."""
    import ctypes
    from unirec_amd import _lib
    from unirec_amd.evaluation import CatalogEvaluator
    N, D, K = args.N, args.D, args.K
    S = args.two_stage_shortlist or min(1024, max(128, 2 * K))
    g = torch.Generator(device="cuda").manual_seed(0)
    ev = CatalogEvaluator(torch.randn(N, D, generator=g, device="cuda").to(torch.bfloat16), dtype=torch.bfloat16)
    f8 = ev.quantized()
    held = sum(t.numel() * t.element_size() for t in (f8.codes, f8.scale, f8.inv))
    print(f"catalog --fp8 --K {K} --two-stage-shortlist {S}: N={N} D={D}; resident bytes: bf16 catalogue {N * D * 2 / 2**20:.0f} MiB + norms "
          f"{N * 4 / 2**20:.1f} MiB, fp8 codes {f8.codes.numel() / 2**20:.0f} MiB + scale and inv {2 * N * 4 / 2**20:.1f} MiB "
          f"(held: {held / 2**20:.1f} MiB); {args.rounds} alternating rounds")
    for B in (args.users or [512, 64]):
        user = torch.randn(B, D, generator=g, device="cuda")
        gt = torch.randint(0, N, (B,), generator=g, device="cuda")
        ev.retrieve(user[:1], k=1)                            # the bf16 catalogue's norms, outside every figure below
        bf_name, f8_name = f"bf16 retrieve_two_stage(k={K}, shortlist={S})", f"fp8  retrieve_two_stage(k={K}, shortlist={S})"
        short16 = hip.catalog_coarse_deep_select(user, ev.catalog, S, ev._inv, gt_index=gt)[0]
        short8 = hip.catalog_fp8_select(user, f8.codes, S, f8.inv, gt_index=gt)[0]
        variants = [(bf_name, lambda: ev.retrieve_two_stage(user, k=K, shortlist=S, gt_index=gt)),
                    (f8_name, lambda: f8.retrieve_two_stage(user, k=K, shortlist=S, gt_index=gt)),
                    ("  bf16 coarse-deep select alone", lambda: hip.catalog_coarse_deep_select(user, ev.catalog, S, ev._inv, gt_index=gt)),
                    ("  fp8 select alone", lambda: hip.catalog_fp8_select(user, f8.codes, S, f8.inv, gt_index=gt)),
                    ("  bf16 deep re-rank alone", lambda: hip.catalog_deep_rerank(user, ev.catalog, short16, K, ev._inv)),
                    ("  fp8 re-rank alone", lambda: hip.catalog_fp8_rerank(user, f8.codes, short8, f8.inv, K))]
        peaks = {}
        for name, fn in variants[:2]:
            fn()
            hip._ws_cache.clear()
            torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            peaks[name] = torch.cuda.max_memory_allocated() - base
        for name, fn in variants:                             # scratch of every variant warm again
            fn()
        q8, q16 = _lib.CatalogFp8Select(), _lib.CatalogCoarseDeep()
        q8.B, q8.N, q8.D, q8.K = B, N, D, S
        q16.B, q16.N, q16.D, q16.K, q16.catalog_bf16 = B, N, D, S, 1
        _lib.check(_lib.load().ur_catalog_fp8_select(ctypes.byref(q8), None), "ur_catalog_fp8_select")
        _lib.check(_lib.load().ur_catalog_coarse_deep_select(ctypes.byref(q16), None), "ur_catalog_coarse_deep_select")
        times = {name: [] for name, _ in variants}
        for _ in range(args.rounds):
            for name, fn in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
        print(f"B={B} K={K} shortlist={S}: select workspace (size queries) fp8 {q8.workspace_bytes / 2**20:.2f} MiB, bf16 "
              f"{q16.workspace_bytes / 2**20:.2f} MiB; peak allocation of a call fp8 {peaks[f8_name] / 2**20:.2f} MiB, bf16 {peaks[bf_name] / 2**20:.2f} MiB")
        med = {}
        for name, _ in variants:
            t = sorted(times[name])
            med[name] = t[len(t) // 2]
            print(f"  {name:52s}: median {med[name]:9.2f} ms  min {t[0]:9.2f}  max {t[-1]:9.2f}  (spread {t[-1] - t[0]:.2f} over {len(t)} alternating rounds)")
        spread = max(max(times[n]) - min(times[n]) for n in (bf_name, f8_name))
        print(f"  bf16 / fp8 = {med[bf_name] / med[f8_name]:.3f}x (difference {med[bf_name] - med[f8_name]:.2f} ms against a spread of {spread:.2f} ms)")
    # recall of both two-stage lists against the exact bf16 retrieve(k), on the random catalogue and on one whose later components decay
    del short16, short8
    Bq = min(64, (args.users or [64])[-1])
    for label in ("random", "decaying"):
        if label == "decaying":
            del ev, f8
            cat, scale = _decaying_catalogue(N, D, (D // 4, D // 2, D), g)
            ev = CatalogEvaluator(cat, dtype=torch.bfloat16)
            del cat
            f8 = ev.quantized()
        u = torch.randn(Bq, D, generator=g, device="cuda")
        if label == "decaying":
            u = u * scale
        exact = ev.retrieve(u, k=K)["topk_index"]
        for name, e in (("bf16", ev), ("fp8", f8)):
            got = e.retrieve_two_stage(u, k=K, shortlist=S)["topk_index"]
            hit = (got[:, :, None] == exact[:, None, :]).any(2).float().mean().item()
            same = (got == exact).all(1).float().mean().item()
            print(f"  recall@{K} of the {name} two-stage list (shortlist {S}) against the exact bf16 retrieve(k), {label} catalogue, {Bq} users: "
                  f"{hit:.6f}; users whose whole list is identical {same:.4f}")


def _decaying_catalogue(N, D, dims, g):
    """standard normal rows whose components in [dims[i-1], dims[i]) are scaled by 2^(-3 i), bf16: a stand-in for a Matryoshka-trained
    embedding, whose leading components carry most of a cosine"""
    scale = torch.ones(D, device="cuda")
    for i in range(1, len(dims)):
        scale[dims[i - 1]:dims[i]] = 2.0 ** (-3 * i)
    return (torch.randn(N, D, generator=g, device="cuda") * scale).to(torch.bfloat16), scale


def catalog_funnel(args):
    """CatalogEvaluator.retrieve_funnel(k=--K, dims=--funnel-dims, shortlists=--funnel-shortlists) on a bf16 catalogue, per user count
    (--users, default 512 and 64), the contenders alternating --rounds times in this process after one call of each:
      (a) retrieve_two_stage(k, shortlists[0]) at the full width, the yardstick;
      (b) retrieve_funnel: every stage reads its prefix of the resident catalogue in place;
      (c) the hand composition through truncated(dims[0]): the stage-0 select on a contiguous [N, dims[0]] copy, then (b)'s re-rank stages --
          the same arithmetic, so (b) against (c) is what the strided read costs.
    Then the stages on their own, the scorer's share of the catalogue bytes per second, the workspaces and the peak allocation of (b), and
    recall@k of (b) against the exact retrieve(k) on a decaying-spectrum catalogue and on a flat random one (the timings run on the
    decaying one; the arithmetic does not depend on the values)."""
    import ctypes
    from unirec_amd import _lib
    from unirec_amd.evaluation import CatalogEvaluator, ranking_metrics
    N, D, K = args.N, args.D, args.K
    dims, S = tuple(args.funnel_dims), tuple(args.funnel_shortlists or ())
    S = S or None
    g = torch.Generator(device="cuda").manual_seed(0)
    cat, scale = _decaying_catalogue(N, D, dims, g)
    ev = CatalogEvaluator(cat, dtype=cat.dtype)
    del cat
    flat = CatalogEvaluator(torch.randn(N, D, generator=g, device="cuda").to(torch.bfloat16), dtype=torch.bfloat16)
    copy = ev.truncated(dims[0])                              # (c)'s contiguous [N, dims[0]] copy
    print(f"catalog --funnel-dims {' '.join(map(str, dims))} --funnel-shortlists {S} --K {K}: N={N} D={D}, catalogue bf16 "
          f"{N * D * 2 / 2**20:.0f} MiB, the truncated copy of (c) {N * dims[0] * 2 / 2**20:.0f} MiB, {args.rounds} alternating rounds")
    for B in (args.users or [512, 64]):
        gt = torch.randint(0, N, (B,), generator=g, device="cuda")
        user = ev.catalog[gt].float() + 0.5 * torch.randn(B, D, generator=g, device="cuda") * scale
        flat_user = flat.catalog[gt].float() + 0.5 * torch.randn(B, D, generator=g, device="cuda")
        ev.retrieve(user[:1], k=1)                            # the norms of every path, outside every figure below
        fun = ev.retrieve_funnel(user, k=K, dims=dims, shortlists=S, gt_index=gt)
        S_used = S or (min(1024, max(128, 2 * K)),) * (len(dims) - 1)
        inv = ev._prefix_norms(dims)
        u0 = user[:, :dims[0]].contiguous()
        copy.retrieve(u0[:1], k=1)
        keep = S_used[1:] + (K,)

        def hand():
            idx, _, rank, _ = hip.catalog_coarse_deep_select(u0, copy.catalog, S_used[0], copy._inv, gt_index=gt)
            for d, n in zip(dims[1:], keep):
                idx, val, _ = hip.catalog_funnel_rerank(user, ev.catalog, idx, d, n, inv[d])
            return idx, val, ranking_metrics(rank, (K,)).cpu().tolist()      # (the metrics and the host read the evaluator's calls end in)

        def reranks(idx):
            for d, n in zip(dims[1:], keep):
                idx, val, _ = hip.catalog_funnel_rerank(user, ev.catalog, idx, d, n, inv[d])
            return idx, val
        a_name, b_name, c_name = f"(a) retrieve_two_stage(k={K}, shortlist={S_used[0]})", f"(b) retrieve_funnel(k={K}, dims={dims})", \
            f"(c) select on truncated({dims[0]}) + (b)'s re-ranks"
        short = hip.catalog_funnel_select(user, ev.catalog, dims[0], S_used[0], inv[dims[0]], gt_index=gt)[0]
        variants = [(a_name, lambda: ev.retrieve_two_stage(user, k=K, shortlist=S_used[0], gt_index=gt)),
                    (b_name, lambda: ev.retrieve_funnel(user, k=K, dims=dims, shortlists=S, gt_index=gt)),
                    (c_name, hand),
                    (f"  coarse-deep select alone, D = {D}", lambda: hip.catalog_coarse_deep_select(user, ev.catalog, S_used[0], ev._inv, gt_index=gt)),
                    (f"  funnel select alone, dim = {dims[0]} of {D}", lambda: hip.catalog_funnel_select(user, ev.catalog, dims[0], S_used[0],
                                                                                                       inv[dims[0]], gt_index=gt)),
                    (f"  coarse-deep select alone, the [N, {dims[0]}] copy", lambda: hip.catalog_coarse_deep_select(u0, copy.catalog, S_used[0],
                                                                                                                 copy._inv, gt_index=gt)),
                    ("  the funnel's re-rank stages alone", lambda: reranks(short))]
        h = hand()
        assert torch.equal(h[0], fun["topk_index"]) and torch.equal(h[1].view(torch.int32), fun["topk_score"].view(torch.int32)), \
            "(b) and (c) are the same arithmetic"
        hip._ws_cache.clear()
        torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        variants[1][1]()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        for name, fn in variants:                             # scratch of every variant warm again
            fn()
        recall = {}
        for label, e, u in (("decaying spectrum", ev, user), ("flat random", flat, flat_user)):
            exact = e.retrieve(u, k=K)["topk_index"]
            got = e.retrieve_funnel(u, k=K, dims=dims, shortlists=S)["topk_index"]
            recall[label] = ((got[:, :, None] == exact[:, None, :]).any(2).float().mean().item(), (got == exact).all(1).float().mean().item())
        qs, qr = _lib.CatalogFunnelSelect(), _lib.CatalogFunnelRerank()
        qs.B, qs.N, qs.dim, qs.ld, qs.ldu, qs.K, qs.catalog_bf16 = B, N, dims[0], D, D, S_used[0], 1
        qr.B, qr.N, qr.dim, qr.ld, qr.ldu, qr.K_in, qr.k, qr.catalog_bf16 = B, N, dims[1], D, D, S_used[0], keep[0], 1
        _lib.check(_lib.load().ur_catalog_funnel_select(ctypes.byref(qs), None), "ur_catalog_funnel_select")
        _lib.check(_lib.load().ur_catalog_funnel_rerank(ctypes.byref(qr), None), "ur_catalog_funnel_rerank")
        times = {name: [] for name, _ in variants}
        for _ in range(args.rounds):
            for name, fn in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
        print(f"B={B} K={K} dims={dims} shortlists={S_used}:")
        for label, (hit, same) in recall.items():
            print(f"  recall@{K} of the funnel against the exact retrieve(k), {label} catalogue: {hit:.6f}; users whose whole list is identical {same:.4f}")
        print(f"  workspace (size queries): select {qs.workspace_bytes / 2**20:.2f} MiB, first re-rank {qr.workspace_bytes / 2**20:.2f} MiB; peak "
              f"allocation of the funnel call {peak / 2**20:.2f} MiB; scores [B,N] f32 would be {B * N * 4 / 2**20:.0f} MiB, a truncated copy "
              f"{N * dims[0] * 2 / 2**20:.0f} MiB")
        med = {}
        for name, _ in variants:
            t = sorted(times[name])
            med[name] = t[len(t) // 2]
            print(f"  {name:54s}: median {med[name]:9.2f} ms  min {t[0]:9.2f}  max {t[-1]:9.2f}  (spread {t[-1] - t[0]:.2f} over {len(t)} alternating rounds)")
        for x, y, what in ((a_name, b_name, "(a) / (b)"), (c_name, b_name, "(c) / (b)")):
            gap = med[x] - med[y]
            spread = max(max(times[x]) - min(times[x]), max(times[y]) - min(times[y]))
            verdict = "(b) faster by more than the spread" if gap > spread else "(b) slower by more than the spread" if -gap > spread else \
                "inside the spread"
            print(f"  {what} = {med[x] / med[y]:.2f}x  (difference {gap:.2f} ms against a spread of {spread:.2f} ms: {verdict})")


def negatives(args):
    """Candidates by index (unirec_amd.negatives.CatalogCandidates) on a random catalogue, every group alternating --rounds times in this
    process after one call of each:
      (a) the widening gather of [B,P] rows from the bf16 copy of the catalogue (hip.gather_rows to f32, one kernel) against the two-pass
          form it replaces (gather_rows to bf16, then .float()); ms and GB/s of the bytes each form moves per element (6 against 10);
      (b) mine(): the K hardest items of B users over the N-row catalogue (--catalog-dtype);
      (c) candidates() as a whole: P/2 explicit + P/2 random + K mined columns, seen items, both gathers."""
    from unirec_amd.negatives import CatalogCandidates
    B, P, N, K, D = args.B, args.P, args.N, args.K, args.D
    g = torch.Generator(device="cuda").manual_seed(0)
    cat = torch.randn(N, D, generator=g, device="cuda")
    cat16 = cat.to(torch.bfloat16)
    if args.catalog_dtype == "bf16":
        cat = cat16
    user = torch.randn(B, D, generator=g, device="cuda")
    pos = torch.randint(0, N, (B,), generator=g, device="cuda")
    idx = torch.randint(0, N, (B, P), generator=g, device="cuda")
    seen = torch.randint(0, N, (B, 50), generator=g, device="cuda")
    miner = CatalogCandidates(cat, num_hard=K)
    whole = CatalogCandidates(miner.evaluator, num_random=P - P // 2, num_hard=K, seed=1)
    one = lambda: hip.gather_rows(cat16, idx, out_dtype=torch.float32)
    two = lambda: hip.gather_rows(cat16, idx).float()
    assert torch.equal(one().view(torch.int32), two().view(torch.int32))
    el = B * P * D
    groups = [[("gather bf16 -> f32, one kernel", one, 6 * el), ("gather bf16 -> bf16, then .float()", two, 10 * el)],
              [(f"mine() K={K}", lambda: miner.mine(user, pos, seen), 0)],
              [(f"candidates() {P // 2} explicit + {P - P // 2} random + {K} mined", lambda: whole.candidates(user, pos, idx[:, :P // 2], exclude=seen, step=3), 0)]]
    print(f"negatives B={B} P={P} N={N} D={D} K={K}: catalogue {args.catalog_dtype} {cat.numel() * cat.element_size() / 2**20:.0f} MiB, "
          f"gathered [B,P,D] f32 {el * 4 / 2**20:.0f} MiB")
    for group in groups:
        times = {name: [] for name, _, _ in group}
        for name, fn, _ in group:                                 # warm-up: scratch buffers, the catalogue norms
            fn(); fn()
        for _ in range(args.rounds):
            for name, fn, _ in group:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3 / args.iters)
        for name, _, nbytes in group:
            t = sorted(times[name])
            rate = f"  {nbytes / t[len(t) // 2] / 1e6:8.1f} GB/s" if nbytes else ""
            print(f"{name:60s}: median {t[len(t) // 2]:9.3f} ms  min {t[0]:9.3f}  max {t[-1]:9.3f}  ({len(t)} alternating rounds of {args.iters} calls){rate}")


def catalog_softmax(args):
    """The full-catalogue softmax loss (hip.catalog_softmax) forward only and forward + backward, alternating --rounds times in this process
    with one streaming retrieval pass (hip.catalog_select, K = 128, rank included) at the same shape -- the code that loss was built beside,
    on the same box.  Per (--users, --dtypes) pair: device-event time of each call, its ratio to the retrieval pass, and what the
    algorithm needs over that time: catalogue bytes per sweep (1 sweep forward, 3 with the backward: score, score again, gradient
    product; retrieval: 1) against the HBM read ceiling, and 2 B N D FLOP per sweep against the f32-MFMA peak."""
    N, D = args.N, args.D
    g = torch.Generator(device="cuda").manual_seed(0)
    cat32 = torch.randn(N, D, generator=g, device="cuda")
    for dtype in (args.dtypes or [args.catalog_dtype]):
        cat = cat32 if dtype == "f32" else cat32.to(torch.bfloat16)
        for B in (args.users or [args.B]):
            user = torch.randn(B, D, generator=g, device="cuda")
            gt = torch.randint(0, N, (B,), generator=g, device="cuda")
            seen = torch.sort(torch.randint(0, N, (B, 50), generator=g, device="cuda"), dim=1).values.contiguous()
            inv = hip.catalog_select(user[:1].contiguous(), cat, 1)[3]             # the catalogue norms: cached by every caller
            variants = [("retrieve K=128", lambda: hip.catalog_select(user, cat, 128, inv, gt_index=gt, exclude=seen), 1),
                        ("softmax forward", lambda: hip.catalog_softmax(user, cat, gt, 0.07, inv, exclude=seen, need_grad=False), 1),
                        ("softmax forward + backward", lambda: hip.catalog_softmax(user, cat, gt, 0.07, inv, exclude=seen), 3)]
            times = {name: [] for name, _, _ in variants}
            for name, fn, _ in variants:                                          # warm-up: code objects, scratch buffers
                fn(); fn()
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for name, fn, _ in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.iters):
                        fn()
                    e1.record(); torch.cuda.synchronize()
                    times[name].append(e0.elapsed_time(e1) / args.iters)
            cat_bytes, flop = cat.numel() * cat.element_size(), 2.0 * B * N * D
            med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
            print(f"catalog_softmax B={B} N={N} D={D} catalogue {dtype} ({cat_bytes / 2**30:.2f} GiB), exclude [B,50], {args.rounds} alternating rounds of {args.iters} calls")
            for name, _, sweeps in variants:
                t = sorted(times[name])
                print(f"  {name:28s}: median {med[name]:8.3f} ms  min {t[0]:8.3f}  max {t[-1]:8.3f}  x{med[name] / med['retrieve K=128']:5.2f} of a retrieval pass"
                      f"  {sweeps} sweep(s): {sweeps * cat_bytes / med[name] / 1e9:6.2f} TB/s of catalogue  {sweeps * flop / med[name] / 1e9:7.1f} TFLOP/s f32")
            del user
        del cat


def catalog_mrl_softmax(args):
    """The Matryoshka catalogue softmax (hip.catalog_mrl_softmax, prefixes --dims of a [--N, --D] catalogue read in place) against the only
    way to the same numbers without it, alternating --rounds times in this process (device events around --iters calls; medians), per
    (--users, --dtypes) pair, every call with its norm planes ready, exclude [B,50]:
      (a) hip.catalog_mrl_softmax, forward and forward + backward (and the forward with each scorer forced);
      (b) K hip.catalog_softmax calls on contiguous slices, slices ready, and again with the slices made inside the timed region;
      (c) one plain hip.catalog_softmax at --D;
      (d) peak device allocation of one cold call of (a) against (b) with its slices (workspace included, the resident catalogue not)."""
    N, D = args.N, args.D
    dims = tuple(int(d) for d in args.dims.split(","))
    tau = 0.07
    g = torch.Generator(device="cuda").manual_seed(0)
    cat32 = torch.randn(N, D, generator=g, device="cuda")

    def peak(fn, tags):
        for key in [k for k in hip._ws_cache if k[1] in tags]:
            del hip._ws_cache[key]
        torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn(); torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    for dtype in (args.dtypes or [args.catalog_dtype]):
        cat = cat32 if dtype == "f32" else cat32.to(torch.bfloat16)
        planes = hip.catalog_prefix_norms(cat, dims)
        for B in (args.users or [args.B]):
            user = torch.randn(B, D, generator=g, device="cuda")
            gt = torch.randint(0, N, (B,), generator=g, device="cuda")
            seen = torch.sort(torch.randint(0, N, (B, 50), generator=g, device="cuda"), dim=1).values.contiguous()

            def mrl_call(**kw):
                return hip.catalog_mrl_softmax(user, cat, gt, dims, None, tau, planes, exclude=seen, **kw)

            def sliced(ready=None, **kw):                                          # (slices made here live one at a time)
                out = []
                for k, d in enumerate(dims):
                    u, c = ready[k] if ready else (user[:, :d].contiguous(), cat[:, :d].contiguous())
                    out.append(hip.catalog_softmax(u, c, gt, tau, planes[k], exclude=seen, **kw)[:4])
                return out

            mem_a = peak(mrl_call, ("catalog_mrl_softmax",))
            mem_b = peak(sliced, ("catalog_softmax",))
            ready = [(user[:, :d].contiguous(), cat[:, :d].contiguous()) for d in dims]
            slice_bytes = sum(c.numel() * c.element_size() for _, c in ready)
            variants = [("(a) mrl forward", lambda: mrl_call(need_grad=False)),
                        ("(a) mrl forward + backward", mrl_call),
                        ("(a) mrl forward, vector scorer", lambda: mrl_call(need_grad=False, scorer="vector")),
                        ("(a) mrl forward, mfma scorer", lambda: mrl_call(need_grad=False, scorer="mfma")),
                        ("(b) K sliced forward, slices ready", lambda: sliced(ready, need_grad=False)),
                        ("(b) K sliced forward + backward, slices ready", lambda: sliced(ready)),
                        ("(b) K sliced forward + backward, slices made", sliced),
                        ("(c) plain forward at D", lambda: hip.catalog_softmax(user, cat, gt, tau, planes[-1], exclude=seen, need_grad=False)),
                        ("(c) plain forward + backward at D", lambda: hip.catalog_softmax(user, cat, gt, tau, planes[-1], exclude=seen))]
            times = {name: [] for name, _ in variants}
            for _, fn in variants:
                fn(); fn()
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for name, fn in variants:
                    times[name].append(timeit(fn, args.iters))
            loss = float(mrl_call(need_grad=False)[0])
            want = sum(float(r[0]) for r in sliced(ready, need_grad=False))
            med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
            print(f"catalog_mrl_softmax B={B} N={N} D={D} dims={dims} (sum d_k / D = {sum(dims) / D:.3f}) catalogue {dtype} "
                  f"({cat.numel() * cat.element_size() / 2**30:.2f} GiB, slices {slice_bytes / 2**30:.2f} GiB), exclude [B,50], {args.rounds} alternating "
                  f"rounds of {args.iters} calls; loss {loss:.6f} against {want:.6f} from the sliced calls")
            for name, _ in variants:
                t = sorted(times[name])
                print(f"  {name:46s}: median {med[name]:9.3f} ms  min {t[0]:9.3f}  max {t[-1]:9.3f}")
            for a, others in (("(a) mrl forward", ("(b) K sliced forward, slices ready", "(c) plain forward at D")),
                              ("(a) mrl forward + backward", ("(b) K sliced forward + backward, slices ready", "(b) K sliced forward + backward, slices made",
                                                              "(c) plain forward + backward at D"))):
                for o in others:
                    print(f"  {a} / {o}: {med[a] / med[o]:.3f}")
            print(f"  (d) peak allocation of a cold call: (a) {mem_a / 2**20:.1f} MiB, (b) with its slices {mem_b / 2**20:.1f} MiB")
            del user, ready
        del cat, planes


def merge(args):
    """Merged adapters (Qwen3LoRAModel.merge_adapter): the evaluation forward of the decoder (--layers of the 0.6B shape, rank --rank on all
    seven projections, B x S tokens, no_grad, eval mode) with the adapters merged and unmerged, alternating --rounds times in this process
    (device events around --iters forwards); merge_adapter() itself for the whole model (host clock around a synchronised call, the cache
    dropped before each) with the bytes of bf16 operands it adds and the HBM traffic the kernel needs (W read once in f32, the bf16
    output written once); and the two pooled outputs' relative difference."""
    from unirec_amd.qwen3 import Qwen3Config, Qwen3LoRAModel
    B, S, L, r = args.B, args.S, args.layers, args.rank
    torch.manual_seed(0)
    m = Qwen3LoRAModel(Qwen3Config(vocab_size=4096, num_hidden_layers=L, lora_r=r, lora_alpha=2.0 * r))
    m.reset_parameters(lora_b_std=0.02)
    m = m.to("cuda").eval()
    g = torch.Generator(device="cuda").manual_seed(1)
    ids = torch.randint(0, 4096, (B, S), generator=g, device="cuda")
    am = torch.ones(B, S, dtype=torch.long, device="cuda")
    am[:, :S // 8] = 0

    def forward():
        with torch.no_grad():
            return m.forward_pooled(ids, am)
    outs, times = {}, {"unmerged": [], "merged": []}
    merge_ms = []
    for _ in range(3):                                   # merge_adapter() from nothing, three times (the first loads the code object)
        m.unmerge_adapter()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.merge_adapter()
        torch.cuda.synchronize()
        merge_ms.append((time.perf_counter() - t0) * 1e3)
    added = m._merged["bytes"]
    w_elems = sum(p.weight.numel() for _, _, _, _, p in m._adapted_projections())
    for form in ("unmerged", "merged"):                  # warm-up of both forms: code objects, the pack, the frozen operands
        m.merge_adapter() if form == "merged" else m.unmerge_adapter()
        outs[form] = forward()
        forward()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for form in ("unmerged", "merged"):
            m.merge_adapter() if form == "merged" else m.unmerge_adapter()
            torch.cuda.synchronize()
            times[form].append(timeit(forward, args.iters))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    diff = float((outs["merged"] - outs["unmerged"]).norm() / outs["unmerged"].norm())
    print(f"merge B={B} S={S} layers={L} rank={r} all seven projections, eval forward under no_grad, {args.rounds} alternating rounds of {args.iters} forwards")
    for form in ("unmerged", "merged"):
        t = sorted(times[form])
        print(f"  forward {form:9s}: median {med[form]:9.3f} ms  min {t[0]:9.3f}  max {t[-1]:9.3f}")
    print(f"  merged / unmerged: {med['merged'] / med['unmerged']:.4f}   (pooled outputs differ by {diff:.3e} relative)")
    t = sorted(merge_ms[1:])
    print(f"  merge_adapter() whole model: {t[0]:.2f} .. {t[-1]:.2f} ms (first call {merge_ms[0]:.2f} ms), adds {added / 2**20:.1f} MiB of bf16 operands; "
          f"the kernel's own traffic {w_elems * 6 / 2**20:.1f} MiB (f32 W in, bf16 out) = {w_elems * 6 / (t[0] * 1e-3) / 1e12:.3f} TB/s over the whole call")


def pool(args):
    """Pooling rules at the decoder's output (B x S rows of --D bf16, left padding with 10 % masked, as the benchmark pads): the pair the
    default rule launches -- rmsnorm_fwd + mean_pool_fwd, mean_pool_bwd + rmsnorm_bwd -- against pool_norm_fwd / pool_norm_bwd under
    both mask-aware rules, alternating --rounds times in this process (device events around --iters calls; medians).  Each time is
    also given as a share of the 6.3 TB/s read ceiling for the bytes that path MUST move: the pair reads x, writes and re-reads the
    normalised rows (forward) or writes and re-reads the broadcast gradient (backward); masked_mean reads only the valid rows; last
    reads B rows; every backward writes all of dx."""
    B, S, D = args.B, args.S, args.D
    eps, peak = 1e-6, 6.3e12
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(B, S, D, generator=g, device="cuda").to(torch.bfloat16)
    w = 1.0 + 0.1 * torch.randn(D, generator=g, device="cuda")
    dp = torch.randn(B, D, generator=g, device="cuda")
    mask = torch.ones(B, S, dtype=torch.uint8, device="cuda")
    mask[:, :S // 10] = 0
    valid = int(mask.sum())
    row = D * 2
    rstd = hip.rmsnorm_fwd(x.view(B * S, D), w, eps)[1]
    paths = {
        "fwd mean (rmsnorm_fwd + mean_pool_fwd)": (lambda: hip.mean_pool_fwd(hip.rmsnorm_fwd(x.view(B * S, D), w, eps)[0].view(B, S, D)), 3 * B * S * row),
        "fwd masked_mean (pool_norm_fwd)": (lambda: hip.pool_norm_fwd(x, w, eps, mask, "masked_mean"), valid * row),
        "fwd last (pool_norm_fwd)": (lambda: hip.pool_norm_fwd(x, w, eps, mask, "last"), B * row),
        "bwd mean (mean_pool_bwd + rmsnorm_bwd)": (lambda: hip.rmsnorm_bwd(hip.mean_pool_bwd(dp, S).view(B * S, D), x.view(B * S, D), w, rstd), 4 * B * S * row),
        "bwd masked_mean (pool_norm_bwd)": (lambda: hip.pool_norm_bwd(dp, x, w, eps, mask, "masked_mean"), (valid + B * S) * row),
        "bwd last (pool_norm_bwd)": (lambda: hip.pool_norm_bwd(dp, x, w, eps, mask, "last"), (B + B * S) * row),
    }
    times = {k: [] for k in paths}
    for fn, _ in paths.values():
        fn(); fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, (fn, _) in paths.items():
            times[k].append(timeit(fn, args.iters))
    print(f"pool B={B} S={S} D={D} left padding, {B * S - valid} of {B * S} rows masked; {args.rounds} alternating rounds of {args.iters} calls, device events")
    med = {}
    for k, (_, nbytes) in paths.items():
        t = sorted(times[k])
        med[k] = t[len(t) // 2]
        print(f"  {k:42s}: median {med[k] * 1e3:9.1f} us  min {t[0] * 1e3:9.1f}  max {t[-1] * 1e3:9.1f}   {nbytes / 2**20:8.1f} MiB must move = "
              f"{nbytes / (med[k] * 1e-3) / 1e12:6.3f} TB/s = {100 * nbytes / (med[k] * 1e-3) / peak:5.1f} % of 6.3 TB/s")
    for d in ("fwd", "bwd"):
        base = next(v for k, v in med.items() if k.startswith(d + " mean"))
        for k, v in med.items():
            if k.startswith(d) and not k.startswith(d + " mean"):
                print(f"  {k} / the pair it replaces: {v / base:.3f}")


def mrl(args):
    """Matryoshka InfoNCE at the joint step's candidate shape (--B users, --N negatives each, --D wide, prefixes --dims), scores + loss +
    backward, alternating --rounds times in this process (device events around --iters calls; medians):
      (a) hip.mrl_infonce: one pass over the candidates for all score planes, one for the whole gradient;
      (b) per prefix, cosine_scores + infonce_fwd_bwd on slices made contiguous INSIDE the timed region (what a nested loss costs today);
      (c) the same with the slices prepared outside it (the kernels alone);
      (d) cosine_scores + infonce_fwd_bwd at --D only: the single-plane loss, the floor.
    Each time is also given against the bytes that path must read of the candidates (f32), at the 6.3 TB/s read ceiling."""
    B, N, D = args.B, args.N, args.D
    dims = tuple(int(d) for d in args.dims.split(","))
    peak, tau = 6.3e12, 0.07
    g = torch.Generator(device="cuda").manual_seed(0)
    user, pos = torch.randn(B, D, generator=g, device="cuda"), torch.randn(B, D, generator=g, device="cuda")
    neg = torch.randn(B, N, D, generator=g, device="cuda")
    cand = B * (N + 1) * 4                                   # bytes of one candidate column

    def pair(u, p, n):
        s, inv = hip.cosine_scores(u, p, n)
        return hip.infonce_fwd_bwd(u, p, n, None, s, inv, tau, 1.0)

    def sliced():
        return [pair(user[:, :d].contiguous(), pos[:, :d].contiguous(), neg[..., :d].contiguous()) for d in dims]

    ready = [(user[:, :d].contiguous(), pos[:, :d].contiguous(), neg[..., :d].contiguous()) for d in dims]
    paths = {
        "(a) mrl_infonce, fused": (lambda: hip.mrl_infonce(user, pos, neg, None, dims, None, tau, 1.0), 2 * cand * D),
        "(b) K sliced pairs, slices made inside": (sliced, 4 * cand * sum(dims)),      # copy in + out, then two reads
        "(c) K sliced pairs, slices ready": (lambda: [pair(*t) for t in ready], 2 * cand * sum(dims)),
        "(d) single plane at D (the floor)": (lambda: pair(user, pos, neg), 2 * cand * D),
    }
    # the results must not differ: every plane and the one-hot gradients are the sliced kernels' bits (tests/test_gpu_mrl_f64.py); here
    # the all-ones total against the sum of the sliced losses
    loss = hip.mrl_infonce(user, pos, neg, None, dims, None, tau, 1.0)[0]
    want = sum(float(l) for l, _ in sliced())
    times = {k: [] for k in paths}
    for fn, _ in paths.values():
        fn(); fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, (fn, _) in paths.items():
            times[k].append(timeit(fn, args.iters))
    print(f"mrl B={B} N={N} D={D} dims={dims} (sum d_k / D = {sum(dims) / D:.3f}), candidates {cand * D / 2**20:.1f} MiB f32; {args.rounds} alternating "
          f"rounds of {args.iters} calls, device events; loss {float(loss):.6f} against {want:.6f} from the sliced pairs")
    med = {}
    for k, (_, nbytes) in paths.items():
        t = sorted(times[k])
        med[k] = t[len(t) // 2]
        print(f"  {k:40s}: median {med[k] * 1e3:9.1f} us  min {t[0] * 1e3:9.1f}  max {t[-1] * 1e3:9.1f}   candidate bytes moved {nbytes / 2**20:8.1f} MiB = "
              f"{nbytes / (med[k] * 1e-3) / 1e12:6.3f} TB/s = {100 * nbytes / (med[k] * 1e-3) / peak:5.1f} % of 6.3 TB/s")
    a = med["(a) mrl_infonce, fused"]
    for k, v in med.items():
        if not k.startswith("(a)"):
            print(f"  (a) / {k}: {a / v:.3f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["attn", "gemm", "lora", "rope", "dw", "xattn", "gemm_lora", "gemm_merge", "gemm_step", "rmslora", "swilora", "catalog", "negatives", "catalog_softmax", "catalog_mrl_softmax", "merge", "pool", "mrl"])
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--S", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--ranks", default="16,8,32,64", help="lora: the ranks to time, comma separated (rank 16 first gives every other rank its ratio)")
    ap.add_argument("--N", type=int, default=1_000_000, help="catalog: items")
    ap.add_argument("--K", type=int, default=10, help="catalog: list length")
    ap.add_argument("--D", type=int, default=1024, help="catalog: embedding width")
    ap.add_argument("--rounds", type=int, default=3, help="catalog: alternating timed rounds")
    ap.add_argument("--chunks", action="store_true", help="catalog: also time retrieve() at half and double the default rows per chunk")
    ap.add_argument("--scorer", nargs="+", choices=["vector", "mfma"], help="catalog: time retrieve() with each of these scorers, alternating")
    ap.add_argument("--shortlist", type=int, default=0, help="catalog: time retrieve(shortlist=...) against the exact retrieve() at (512, 100) and (64, 10)")
    ap.add_argument("--two-stage-shortlist", type=int, default=0,
                    help="catalog: time retrieve_two_stage(k=--K, shortlist=...) against the exact retrieve(k=--K) per --users (default 512 and 64)")
    ap.add_argument("--fp8", action="store_true",
                    help="catalog: time Fp8CatalogEvaluator.retrieve_two_stage(k=--K, shortlist=--two-stage-shortlist) against the bf16 "
                         "retrieve_two_stage per --users (default 512 and 64), with resident bytes, peak allocation and recall")
    ap.add_argument("--segments", type=int, nargs="+", help="catalog with --K above 128: also time the long-list call with each of these workgroup counts per user forced")
    ap.add_argument("--funnel-dims", type=int, nargs="+",
                    help="catalog: time retrieve_funnel(k=--K, dims=...) against retrieve_two_stage at the full width and against the hand "
                         "composition through truncated(dims[0]), per --users (default 512 and 64); the catalogue is bf16")
    ap.add_argument("--funnel-shortlists", type=int, nargs="+", help="catalog --funnel-dims: the shortlists (default: retrieve_funnel's own)")
    ap.add_argument("--catalog-dtype", choices=["f32", "bf16"], default="f32", help="catalog: the dtype the catalogue is stored in")
    ap.add_argument("--users", type=int, nargs="+", help="catalog_softmax: the user counts to time (default: --B)")
    ap.add_argument("--dtypes", nargs="+", choices=["f32", "bf16"], help="catalog_softmax: the catalogue dtypes to time (default: --catalog-dtype)")
    ap.add_argument("--P", type=int, default=1000, help="negatives: candidate columns per user")
    ap.add_argument("--layers", type=int, default=28, help="merge: decoder layers")
    ap.add_argument("--rank", type=int, default=16, help="merge: LoRA rank")
    ap.add_argument("--dims", default="64,128,256,512,1024", help="mrl: the nested prefix widths, comma separated, the last one --D")
    ap.add_argument("--lib", action="store_true", help="gemm: also time torch.matmul on the same operands (reference point)")
    a = ap.parse_args()
    {"attn": attn, "gemm": gemm, "lora": lora, "rope": rope, "dw": dw, "xattn": xattn, "gemm_lora": gemm_lora, "gemm_merge": gemm_merge, "gemm_step": gemm_step, "rmslora": rmslora, "swilora": swilora,
     "catalog": catalog, "negatives": negatives, "catalog_softmax": catalog_softmax, "catalog_mrl_softmax": catalog_mrl_softmax, "merge": merge, "pool": pool, "mrl": mrl}[a.what](a)

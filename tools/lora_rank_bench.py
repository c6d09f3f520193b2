#!/usr/bin/env python3
"""Decoder training step per LoRA rank (default: the C4 shape, B 64 x S 2048, 28 layers of Qwen3-0.6B, lora_dropout 0.1).

For every rank of --ranks, in ONE process: a Qwen3LoRAModel with random weights, warm-up steps, then --steps steps (prefetch of the
dropout planes, forward, backward) timed with device events; and, in isolation, the four masked dX GEMMs of a layer's backward
(frozen W^T + the adapters' masked rank-r epilogue), times the layer count, with their share of the step: for ranks other than 16
they run on the generic GEMM kernel, for rank 16 on the persistent one.  Prints one JSON line; --out writes it to a file too.
--targets times placements (peft's target_modules): placements separated by ';', the projections of one by ',', `all` = all seven --
every rank of --ranks runs once per placement, rows carry "targets" and "step_vs_all" (the isolated dX GEMMs are the all-seven
launches and are timed for `all` only).
    python tools/lora_rank_bench.py [--ranks 16,8,32,64] [--B 64] [--S 2048] [--layers 28] [--steps 10] [--warmup 3] [--out FILE]
                                    [--targets "all;q_proj,v_proj;q_proj,k_proj,v_proj,o_proj"]"""
import argparse
import gc
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from unirec_amd import hip
from unirec_amd.qwen3 import Qwen3Config, Qwen3LoRAModel

BF16 = torch.bfloat16


def events_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def dx_gemms_ms(M, cfg, r, p, iters):
    """the four dX launches of one layer's backward under LoRA dropout: {group: ms}"""
    D, I = cfg.hidden_size, cfg.intermediate_size
    NQ, NKV = cfg.num_attention_heads * cfg.head_dim, cfg.num_key_value_heads * cfg.head_dim
    g = torch.Generator().manual_seed(0)
    out = {}
    for name, N, K, nad in (("down", I, D, 1), ("gate|up", D, 2 * I, 2), ("o", NQ, D, 1), ("q|k|v", D, NQ + 2 * NKV, 3)):
        dy = torch.randn(M, K, generator=g).cuda().to(BF16)
        WT = (torch.randn(N, K, generator=g) * 0.05).cuda().to(BF16)
        tb = torch.randn(M, nad * r, generator=g).cuda().to(BF16)
        AT = (torch.randn(N, nad * r, generator=g) * 0.05).cuda().to(BF16)
        bits = hip.lora_dropout_bits(1, p, M, N, nad, "cuda")
        res = torch.empty(M, N, dtype=BF16, device="cuda")
        fn = lambda: hip.gemm(dy, WT, out=res, R2=tb, S2=AT, drop=(bits, p, r))
        fn()
        out[name] = events_ms(fn, iters)
        del dy, WT, tb, AT, bits, res
    return out


def step_ms(args, r, targets=None):
    """targets: the projections that carry an adapter (None: all seven)"""
    cfg = Qwen3Config(vocab_size=4096, num_hidden_layers=args.layers, lora_r=r, lora_alpha=2.0 * r, lora_dropout=args.dropout,
                      lora_target_modules=targets)
    torch.manual_seed(0)
    m = Qwen3LoRAModel(cfg)
    m.reset_parameters(lora_b_std=0.02)
    m = m.cuda().train()
    B, S, T = args.B, args.S, 20
    first = cfg.vocab_size - T
    ids = torch.randint(1, first, (B, S), device="cuda")
    ids[:, S // 2:S // 2 + T] = first + torch.arange(T, device="cuda")
    am = torch.ones((B, S), dtype=torch.int64, device="cuda")
    tok = (torch.randn(B, T, cfg.hidden_size, device="cuda") * 0.05).to(BF16).requires_grad_(True)
    gvec = torch.randn(B, cfg.hidden_size, device="cuda")

    def step():
        m.prefetch_lora_bits(B * S, ids.device)
        m.forward_pooled(ids, am, tok, first).backward(gvec)
        tok.grad = None

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    ms = events_ms(step, args.steps)
    plan = m._plan(B * S, S, ids.device, m._pack, m._frozen)
    dx = dx_gemms_ms(B * S, cfg, r, args.dropout, 5) if targets is None else {}
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    params = [(n, p.detach()) for n, p in m.lora_named_parameters()]
    del m, tok, ids, am
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    dx_step = args.layers * sum(dx.values())
    if targets is not None:
        return {"rank": r, "targets": list(targets), "step_ms": round(ms, 2), "seq_per_s": round(B / ms * 1e3, 2), "peak_GiB": round(peak, 1),
                "trainable_params": sum(p.numel() for _, p in params),
                "plan": {"merged": plan.merged, "fuse_norm": plan.fuse_norm, "fuse_rope": plan.fuse_rope, "swiglu": plan.swiglu, "bits_t": plan.bits_t}}
    return {"rank": r, "step_ms": round(ms, 2), "seq_per_s": round(B / ms * 1e3, 2), "peak_GiB": round(peak, 1),
            "plan": {"merged": plan.merged, "fuse_norm": plan.fuse_norm, "fuse_rope": plan.fuse_rope, "swiglu": plan.swiglu, "bits_t": plan.bits_t},
            "dx_gemm_ms_per_layer": {k: round(v, 3) for k, v in dx.items()}, "dx_gemm_ms_per_step": round(dx_step, 2),
            "dx_gemm_share_of_step": round(dx_step / ms, 3)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", default="16,8,32,64")
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--S", type=int, default=2048)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--targets", default=None, help="placements separated by ';', projections by ',', 'all' = all seven")
    a = ap.parse_args()
    if a.targets:
        from unirec_amd.qwen3 import LORA_TARGETS
        places = [LORA_TARGETS if t.strip() == "all" else tuple(x.strip() for x in t.split(",")) for t in a.targets.split(";")]
        rows = [step_ms(a, int(r), list(t)) for r in a.ranks.split(",") for t in places]
        for x in rows:
            base = next((y for y in rows if y["rank"] == x["rank"] and tuple(y["targets"]) == LORA_TARGETS), None)
            x["step_vs_all"] = round(x["step_ms"] / base["step_ms"], 3) if base else None
    else:
        rows = [step_ms(a, int(r)) for r in a.ranks.split(",")]
        base = next((x for x in rows if x["rank"] == 16), None)
        for x in rows:
            x["step_vs_rank16"] = round(x["step_ms"] / base["step_ms"], 3) if base else None
    res = {"what": "decoder training step per LoRA rank" + (" and placement" if a.targets else ""), "B": a.B, "S": a.S, "layers": a.layers, "dropout": a.dropout, "steps": a.steps,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "ranks": rows}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")

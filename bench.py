#!/usr/bin/env python3
"""bench.py -- headline benchmark of the UniRec MI355X hot path.

Metric (BASELINE.json): user-sequences/sec of the JOINT training step (item Q-Former on the
history -> token injection -> Qwen3-Embedding-0.6B-shaped decoder + LoRA r=16 -> mean pool -> InfoNCE
over the candidate pool; forward + backward + gradient all-reduce + AdamW), hist=50, Q_item=2,
S=2048, pool 1000, batch 64 per GPU (configs[3] = C4; weak scaling: per-GPU batch fixed).
A "step" = one such pass over one batch of synthetic inputs that are already resident in HBM.

  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \\
        bench.py --gpus N --steps K --warmup W

Rank 0 prints ONE JSON line (contract in the task statement).  A plain run sets up, warms up, times the K steps and
prints the headline (`metric`, `value`, `unit`, `ms_per_step`, `loss`, `param_checksum`, `comm`, ...), nothing more.
`--full` adds what takes runs or passes of its own: `roofline` (dominant kernel = the bf16 MFMA projection GEMM, timed
live with HIP events on its launch stream inside the timed region), `attention` and the HBM-bound families (a separate
pass of events after it), `cpu_baseline` (the oracle's joint step timed on the host cores on a bounded sample; N=1 only)
and, for the default shapes, the per-stage lines (`stages`: C1, C2, C3, C5).

`--dump-outputs DIR` writes what the last timed step computed as DIR/<name>.npy (float32 / float64, a few tens of MB at
most): the loss, the user embeddings and a fixed, seeded sample of the trainable parameters after the optimizer step and
of their gradients.  The inputs are seeded, so equal arguments give equal inputs from run to run.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")      # (unirec_amd/__init__.py: kernel arguments in device memory; before HIP initialises)

import torch


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64, help="user sequences per GPU (C4: 64)")
    ap.add_argument("--hist", type=int, default=50)
    ap.add_argument("--seq", type=int, default=2048)
    ap.add_argument("--pool", type=int, default=1000)
    ap.add_argument("--layers", type=int, default=28, help="Qwen3 layers (28 = the named model; fewer is a debug run)")
    ap.add_argument("--workload", choices=["joint", "item", "user", "item_c1"], default="joint",
                    help="joint = C4 headline (default); item = C2 item Q-Former step; user = C3 user Q-Former step; item_c1 = C1 tiny item Q-Former eval forward")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-baseline-only", action="store_true", help="(internal) run the CPU oracle leg and print its JSON")
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--cpu-budget", type=float, default=100.0, help="seconds of oracle work the cpu_baseline leg may start (warm-up 1 + best of 3 inside it)")
    ap.add_argument("--user-tokens", action="store_true",
                    help="C5 / U4: also run the User Q-Former over hist*32 cached item tokens and inject its 64 query tokens")
    ap.add_argument("--micro-batches", type=int, default=1,
                    help="split the per-GPU batch into this many micro-batches inside one optimizer step (gradient accumulation; "
                         "C5: --batch 64 --micro-batches 2 keeps S=4096 within 288 GB)")
    ap.add_argument("--no-stages", dest="stages", action="store_false",
                    help="joint workload: skip the item (C2) / user (C3) stage measurements that follow the headline in the same process")
    ap.add_argument("--stage-steps", type=int, default=10)
    ap.add_argument("--no-c5-stage", dest="c5_stage", action="store_false",
                    help="joint workload: skip the C5 line (hist 100, S 4096, pool 10000, user tokens, B 64; 1 warm-up + 2 steps) that follows the stages")
    ap.add_argument("--c5-stage-multi", action="store_true",
                    help="run the C5 line on a multi-rank launch as well (default: single-GPU runs only -- it fills 260 of 288 GB per rank, and a rank "
                         "that runs out of memory there would take the headline line of the scaling run with it)")
    ap.add_argument("--c5-cpu-budget", type=float, default=45.0, help="seconds of oracle work the C5 cpu_baseline leg may start")
    ap.add_argument("--cpu-runs", type=int, default=3, help="(internal) timed repeats of the cpu_baseline leg after its warm-up (0: the cold run is the sample)")
    ap.add_argument("--stage-cpu-budget", type=float, default=25.0, help="seconds of oracle work per stage cpu_baseline leg")
    ap.add_argument("--recompute-mlp", action="store_true",
                    help="drop gate|up and act after each layer's forward and rebuild them in the backward (memory for time: "
                         "the C5 shape --user-tokens --hist 100 --seq 4096 --batch 64 then runs as ONE launch)")
    ap.add_argument("--recompute-mlp-layers", type=int, default=0,
                    help="like --recompute-mlp for decoder layers 0 .. N-1 only (the C5 line keeps as many layers' gate|up / act as 288 GB allow)")
    ap.add_argument("--no-dropout", action="store_true")
    ap.add_argument("--comm-bf16", action="store_true",
                    help="multi-GPU, opt-in: the item Q-Former's gradient buckets cross xGMI as bf16 (dp.GradBuckets wire_dtype); default f32")
    ap.add_argument("--lora-dropout", type=float, default=0.1, help="LoRA adapter dropout (reference lora_dropout=0.1)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: roofline / attention / HBM-family events, the CPU oracle "
                         "baseline and the per-stage lines (the --no-* switches above act on these)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (float32 / float64)")
    return ap.parse_args()


# ---- synthetic inputs ----------------------------------------------------------
def make_batch(B, hist, S, pool, F, E, D, Qi, vocab, first_special, seed, device, n_user=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(B, hist, F, E, generator=g)
    x = x / x.norm(dim=-1, keepdim=True)
    x[:, :, 1, E - 256:] = 0.0                                   # CLIP field: 768 dims zero-padded to 1024
    hmask = (torch.rand(B, hist, F, generator=g) < 0.8).long()
    hmask[..., 0] = 1
    hlen = torch.randint(hist // 2, hist + 1, (B,), generator=g)
    for b in range(B):
        hmask[b, hlen[b]:] = 0                                   # padded history slots: fully masked zeros
    x = x * hmask[..., None]
    ids = torch.randint(0, vocab, (B, S), generator=g)
    am = torch.ones(B, S, dtype=torch.long)
    npad = (torch.rand(B, generator=g) * 0.2 * S).long()
    nsp = hist * Qi + n_user                                     # history specials, then the user-query specials (U4)
    stride = max(1, (S - int(npad.max()) - 8) // nsp)
    for b in range(B):
        am[b, :npad[b]] = 0                                      # left padding (~10 % of positions)
        pos = npad[b] + 4 + torch.arange(nsp) * stride
        ids[b, pos] = first_special + torch.arange(nsp)          # each special token exactly once
    posv = torch.randn(B, D, generator=g)
    posv = posv / posv.norm(dim=-1, keepdim=True)
    neg = torch.randn(B, pool - 1, D, generator=g)
    neg = neg / neg.norm(dim=-1, keepdim=True)
    out = dict(input_ids=ids.to(device), attention_mask=am.to(device), history_field_embeddings=x.to(device),
               history_attention_mask=hmask.to(device), positive_item_embeddings=posv.to(device),
               negative_item_embeddings=neg.to(device), negative_masks=None, user_sequence_tokens=None, user_attention_mask=None)
    if n_user > 0:       # C3-shaped user sequence: hist x 32 cached item query tokens, ragged with the history length
        T = hist * 32
        ut = (torch.randn(B, T, D, generator=g) * 0.8).to(torch.bfloat16)
        um = (torch.arange(T)[None, :] < (hlen * 32)[:, None]).float()
        out["user_sequence_tokens"] = (ut * um[..., None].to(torch.bfloat16)).to(device)
        out["user_attention_mask"] = um.to(device)
    return out


def build(args, device):
    from unirec_amd.joint import MultiModalQwenEmbedding
    from unirec_amd.qformer_utils import QFormerForItemRepresentation
    from unirec_amd.qwen3 import Qwen3Config
    torch.manual_seed(1234)
    Qi, F, E, D = 2, 14, 1024, 1024
    p = 0.0 if args.no_dropout else 0.2
    qf = QFormerForItemRepresentation(hidden_size=D, num_hidden_layers=12, num_attention_heads=16, intermediate_size=4096,
                                      num_query_tokens=Qi, field_embedding_dim=E, num_fields=F, dropout=p)
    cfg = Qwen3Config(num_hidden_layers=args.layers, lora_dropout=0.0 if args.no_dropout else args.lora_dropout)    # reference: :121-131
    uq = None
    if getattr(args, "user_tokens", False):
        from unirec_amd.user_qformer import UserQFormer
        uq = UserQFormer(dropout=0.0 if args.no_dropout else 0.1)
    model = MultiModalQwenEmbedding(qformer_model=qf, use_lora=True, qwen_config=cfg, num_history_items=args.hist,
                                    num_query_tokens_per_item=Qi, user_qformer=uq)
    model.base_model.reset_parameters(lora_b_std=0.01)           # exercise the LoRA path
    model = model.to(device).train()
    return model, qf, cfg, (Qi, F, E, D)


def flops_per_step(args, B, cfg, dims):
    """Algorithmic FLOPs of one joint step on one GPU (SURVEY.md §8(d) formulas)."""
    Qi, F, E, D = dims
    S, hist = args.seq, args.hist
    H, I_q, L_q = 1024, 4096, 12
    items = B * hist
    per_layer = items * Qi * (8 * H * H + 4 * Qi * H + 4 * H * I_q)
    cross = 4 * items * Qi * H * H + 4 * items * F * E * H + 4 * items * Qi * F * H
    qf_fwd = L_q * per_layer + 6 * cross
    nq, nkv, hd, I = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim, cfg.intermediate_size
    w = D * (nq + 2 * nkv) * hd + nq * hd * D + 3 * D * I
    tok = B * S
    gemm_fwd = cfg.num_hidden_layers * 2 * w * tok
    attn_fwd = cfg.num_hidden_layers * (4 * B * nq * S * S * hd) / 2
    lora_fwd = cfg.num_hidden_layers * 2 * tok * cfg.lora_r * (2 * D * 4 + (nq + 2 * nkv) * hd + nq * hd + 3 * I + I)
    qwen = (gemm_fwd + lora_fwd) * 2 + attn_fwd * 3.5     # bwd: dX only for frozen weights (+LoRA dA/dB); attention bwd = 2.5x fwd
    return qf_fwd * 3 + qwen


def attn_executed_ratio(am, S, kt=64):
    """Executed / algorithmic MFMA work of the causal head_dim-128 attention launches for the 0/1 attention mask `am` [B, S]
    (csrc/attn.hip: attn_fwd_c128_kernel, attn_bwd_dq_c128_kernel, attn_bwd_dkv_c128_kernel; S a multiple of 128).
    Forward and dQ: a wave owns 64 queries and sweeps the 64-key tiles from the sequence's first tile holding a valid key up to
    its diagonal tile; per tile 72 MFMAs forward (S, P V and the 8 row-sum products: 2.25 contractions of 64 x 64 pairs) and 96
    for dQ (3 contractions); the diagonal tile skips the quarter above the diagonal.  dK/dV: a workgroup owns 128 keys -- skipped
    whole when none is valid -- and every wave sweeps all 64-query tiles from the block's first query to S, 4 contractions.
    Algorithmic: S^2 / 2 query-key pairs per head x 2 contractions forward, 5 backward (bench convention: 2.5 x forward)."""
    valid = am.to("cpu").bool()
    B = valid.shape[0]
    ntiles = S // kt
    pairs_q = pairs_k = 0.0
    for b in range(B):
        nz = torch.nonzero(valid[b])
        t0 = (int(nz[0]) // kt) if nz.numel() else ntiles
        for w in range(S // 64):                       # wave w of the sequence: queries 64 w .. 64 w + 63, diagonal tile w
            tiles = max(0, w + 1 - t0)
            if tiles > 0:
                pairs_q += (tiles - 0.25) * kt * 64
        for kb in range(S // 128):
            if bool(valid[b, kb * 128:(kb + 1) * 128].any()):
                pairs_k += ((S - kb * 128) // kt) * kt * 128
    alg = B * S * S / 2.0
    return {"fwd": 2.25 * pairs_q / (2.0 * alg), "bwd": (3.0 * pairs_q + 4.0 * pairs_k) / (5.0 * alg)}


def device_peaks():
    """Peaks READ FROM THE DEVICE beside the datasheet ones: bf16 dense MFMA = CUs x max shader clock x 4096 FLOP per CU
    and clock (4 SIMDs x one v_mfma_f32_32x32x16_bf16 = 32768 FLOP per 32 cycles).  CU count from the HIP device properties, the
    maximum shader clock from `rocminfo` (torch does not expose it on ROCm), else from sysfs pp_dpm_sclk."""
    out = {"mfma_bf16_TFLOPs_spec": 2500.0, "hbm_GBps_spec": 8000.0}
    try:
        cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
        mhz, src = 0.0, None
        try:
            import re
            import subprocess
            txt = subprocess.run(["rocminfo"], capture_output=True, text=True, timeout=30).stdout
            for blk in txt.split("Agent ")[1:]:
                if "Device Type:             GPU" in blk or re.search(r"Device Type:\s+GPU", blk):
                    m = re.search(r"Max Clock Freq\. \(MHz\):\s+(\d+)", blk)
                    if m:
                        mhz, src = float(m.group(1)), "rocminfo"
                        break
        except Exception:                       # noqa: BLE001
            pass
        if not mhz:
            import glob
            for f in glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk"):
                vals = [float(x.split(":")[1].lower().replace("mhz", "").replace("*", "").strip()) for x in open(f).read().strip().splitlines() if ":" in x]
                if vals:
                    mhz, src = max(vals), "pp_dpm_sclk"
                    break
        out.update({"compute_units": cus, "max_shader_clock_MHz": mhz or None, "clock_source": src,
                    "mfma_bf16_TFLOPs_device": round(cus * mhz * 1e6 * 4096 / 1e12, 1) if mhz else None})
    except Exception as e:                      # noqa: BLE001 -- the line must still print
        out["error"] = str(e)
    return out


def _cpu_threads(args):
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    threads = max(1, min(args.cpu_threads, avail))     # more threads than this thrash on the small fp32 ops
    torch.set_num_threads(threads)
    return threads


def _best_of(step, budget_s, runs=3):
    """warm-up 1 + best of 3, inside a time budget (a run that would overshoot the budget is not started)."""
    t_start = time.time()
    t0 = time.time(); step(); warm = time.time() - t0
    if runs <= 0:
        return warm, f"1 run (cold, {warm:.1f} s; bounded sample: no repeats asked for)"
    times = []
    for _ in range(runs):
        if times and time.time() - t_start + min(times) > budget_s:
            break
        if not times and time.time() - t_start + warm > budget_s:
            break
        t0 = time.time(); step(); times.append(time.time() - t0)
    if not times:
        return warm, f"1 run (cold, {warm:.1f} s; the budget of {budget_s:.0f} s left no room for timed repeats)"
    return min(times), f"warm-up 1 + best of {len(times)} ({min(times):.2f} s; warm-up {warm:.1f} s)"


def cpu_baseline(args, cfg, dims):
    """Oracle joint step (fwd+bwd, fp32) on the host cores, B=1 sequence of the same workload."""
    from oracle import qformer_ref as R, qwen3_ref as Q, weights as W
    Qi, F, E, D = dims
    threads = _cpu_threads(args)
    qcfg = R.QFormerCfg(D, 12, 16, 4096, Qi, E, 2)
    wc = Q.Qwen3Cfg(hidden_size=D, num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                    num_key_value_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim, intermediate_size=cfg.intermediate_size,
                    vocab_size=4096 + args.hist * Qi, rope_theta=cfg.rope_theta, lora_r=cfg.lora_r, lora_alpha=cfg.lora_alpha)
    g = torch.Generator().manual_seed(0)
    PQ = {k: (torch.randn(s, generator=g) * 0.02).requires_grad_(True) for k, s in R.item_qformer_shapes(qcfg, F).items()}
    PW = {}
    for k, s in Q.qwen3_shapes(wc, lora=True).items():
        t = torch.randn(s, generator=g) * 0.02
        if "norm" in k:
            t = torch.ones(s)
        PW[k] = t.requires_grad_(".lora_" in k)
    first = 4096
    n_user = 64 if args.user_tokens else 0
    ucfg, PU = None, {}
    if n_user:           # C5 / U4: the User Q-Former (reference default: L4 Q64 H1024 I4096) over hist x 32 cached item tokens, its 64 query tokens injected
        ucfg = R.QFormerCfg(D, 4, 16, 4096, n_user, D, 1)
        PU = {k: (torch.randn(s, generator=g) * 0.02).requires_grad_(True) for k, s in R.user_qformer_shapes(ucfg, 32).items()}
        PW["embed_tokens.weight"] = torch.randn(first + args.hist * Qi + n_user, D, generator=g) * 0.02
    b = make_batch(1, args.hist, args.seq, args.pool, F, E, D, Qi, first, first, 7, "cpu", n_user=n_user)

    def step():
        for t in list(PQ.values()) + list(PW.values()) + list(PU.values()):
            t.grad = None
        out = R.item_qformer_forward(PQ, qcfg, b["history_field_embeddings"].view(args.hist, F, E), b["history_attention_mask"].view(args.hist, F))
        toks = out["query_outputs"].view(1, args.hist, Qi, D)
        if n_user:
            _, uqo = R.user_qformer_forward(PU, ucfg, b["user_sequence_tokens"].float(), b["user_attention_mask"], 32)
            toks = torch.cat([toks.view(1, args.hist * Qi, D), uqo], dim=1).view(1, 1, args.hist * Qi + n_user, D)
        u = Q.joint_forward(PW, wc, b["input_ids"], b["attention_mask"], toks, first)
        loss = Q.infonce_loss(u, b["positive_item_embeddings"], b["negative_item_embeddings"])
        loss.backward()
    dt, how = _best_of(step, args.cpu_budget, runs=args.cpu_runs)
    return {"value": round(1.0 / dt, 5), "unit": "user-sequences/sec", "cores": threads, "kind": "port",
            "sample": f"1 user-sequence (hist={args.hist}, S={args.seq}, pool={args.pool}, {cfg.num_hidden_layers} layers" + (", User Q-Former over hist x 32 tokens + 64 user tokens" if n_user else "") + "), "
                      f"oracle fp32 fwd+bwd, {how}"}


def cpu_baseline_stage(args):
    """Oracle item (C2) / user (C3) Q-Former step, fwd+bwd fp32 on the host cores, on a reduced batch of the same shapes
    (C3 at B=32; C2 at B=64), dropout off (the oracle has no dropout path; its cost is negligible on the CPU)."""
    from oracle import qformer_ref as R
    threads = _cpu_threads(args)
    g = torch.Generator().manual_seed(0)
    if args.workload == "item_c1":
        # BASELINE configs[0] exactly: the evaluate_item_qformer.py path (evaluation/evaluate_item_qformer.py:66-104), eval forward + masked MSE + cosine
        B, F, E = 16, 8, 256
        cfg = R.QFormerCfg(256, 2, 4, 1024, 4, E, 2)
        P = {k: torch.randn(s, generator=g) * 0.02 for k, s in R.item_qformer_shapes(cfg, F).items()}
        x = torch.randn(B, F, E, generator=g); x = x / x.norm(dim=-1, keepdim=True)
        mk = (torch.rand(B, F, generator=g) < 0.8).long(); mk[:, 0] = 1
        x = x * mk[..., None]
        reps = 200

        def step():
            with torch.no_grad():
                for _ in range(reps):
                    out = R.item_qformer_forward(P, cfg, x, mk)
                    R.eval_reconstruction(out["reconstructed_fields"], x, mk)
        dt, how = _best_of(step, args.cpu_budget)
        return {"value": round(B * reps / dt, 1), "unit": "items/sec", "latency_us": round(dt / reps * 1e6, 1), "cores": threads, "kind": "port",
                "sample": f"{reps} eval forwards of {B} items (C1: L2 Q4 H256 nh4 I1024 F8 E256) + masked MSE / cosine, oracle fp32, {how}"}
    if args.workload == "item":
        B, F = 64, 14
        cfg = R.QFormerCfg(768, 12, 12, 3072, 32, 1024, 2)
        P = {k: (torch.randn(s, generator=g) * 0.02).requires_grad_(True) for k, s in R.item_qformer_shapes(cfg, F).items()}

        def fields(n):
            x = torch.randn(n, F, 1024, generator=g); x = x / x.norm(dim=-1, keepdim=True)
            mk = (torch.rand(n, F, generator=g) < 0.8).long(); mk[:, 0] = 1
            return x * mk[..., None], mk
        (xa, ma), (xpn, mpn) = fields(B), fields(2 * B)

        def step():      # training/item_qformer_training.py:117-131: anchor with grad, positives / negatives without
            for t in P.values():
                t.grad = None
            out = R.item_qformer_forward(P, cfg, xa, ma)
            with torch.no_grad():
                rep = R.item_qformer_forward(P, cfg, xpn, mpn)["item_representation"]
            R.qformer_loss(out, xa, ma, rep[:B], rep[B:])[0].backward()
        unit, what = "items/sec", f"{B} items (C2 shapes L12 Q32 H768 F14; anchor fwd+bwd + positives|negatives no-grad fwd)"
    else:
        B, T = 16, args.hist * 32
        cfg = R.QFormerCfg(1024, 4, 16, 4096, 64, 1024, 1)
        P = {k: (torch.randn(s, generator=g) * 0.02).requires_grad_(True) for k, s in R.user_qformer_shapes(cfg, 32).items()}
        x = torch.randn(B, T, 1024, generator=g) * 0.8
        lens = torch.randint(T // 2, T + 1, (B,), generator=g)
        mask = (torch.arange(T)[None, :] < lens[:, None]).float()
        x = x * mask[..., None]
        tgt = torch.randn(B, 32, 1024, generator=g) * 0.8

        def step():      # training/user_qformer_training.py:203-214
            for t in P.values():
                t.grad = None
            torch.nn.functional.mse_loss(R.user_qformer_forward(P, cfg, x, mask, 32)[0], tgt).backward()
        unit, what = "user-sequences/sec", f"{B} user sequences (C3 shapes L4 Q64 H1024, T={T})"
    dt, how = _best_of(step, args.cpu_budget)
    return {"value": round(B / dt, 3), "unit": unit, "cores": threads, "kind": "port", "sample": f"{what}, oracle fp32, {how}"}


def cpu_baseline_subprocess(args):
    """Run the oracle leg in a child process with a hard time bound (a GPU-initialised process must not
    exec; a child is fine) so the default bench always finishes within minutes."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-baseline-only", "--workload", args.workload, "--hist", str(args.hist),
           "--seq", str(args.seq), "--pool", str(args.pool), "--layers", str(args.layers), "--cpu-threads", str(args.cpu_threads),
           "--cpu-budget", str(args.cpu_budget), "--cpu-runs", str(getattr(args, "cpu_runs", 3))] + (["--user-tokens"] if getattr(args, "user_tokens", False) else [])
    unit = {"item": "items/sec", "item_c1": "items/sec"}.get(args.workload, "user-sequences/sec")
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.cpu_budget + 150, env={**os.environ, "HIP_VISIBLE_DEVICES": ""})
        line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
        return json.loads(line)
    except Exception as e:       # timeout / failure: report it, never hide it
        return {"value": None, "unit": unit, "cores": args.cpu_threads, "kind": "port",
                "sample": f"oracle leg did not finish within {args.cpu_budget + 150} s ({type(e).__name__})"}


# ---- per-stage workloads (BASELINE configs[1], configs[2]); reported with their own metric names ----
def run_stage(args):
    from unirec_amd import dp
    rank, world, local = dp.init_from_env()
    _check_world(args, world)
    device = torch.device("cuda", local % max(1, torch.cuda.device_count()))      # (modulo: gloo rehearsal of N ranks on one GPU)
    torch.cuda.set_device(device)
    out = measure_stage(args, rank, world, device)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        dp.close_native_comms()
        torch.distributed.destroy_process_group()


def measure_stage(args, rank, world, device):
    """One stage workload (args.workload = item | user) on an initialised device / process group -> the stage's JSON object
    (rank 0; None elsewhere).  Also called by the joint bench for the `stages` entry of its line."""
    from unirec_amd import dp
    from unirec_amd.losses import QFormerLoss, mse_loss
    from unirec_amd.optim import FusedAdamW
    from unirec_amd import hip
    torch.manual_seed(1234)
    g = torch.Generator().manual_seed(1234 + rank)
    p = 0.0 if args.no_dropout else None
    if args.workload == "item_c1":
        return measure_item_c1(args, rank, world, device, g)
    if args.workload == "item":
        from unirec_amd.qformer_utils import QFormerForItemRepresentation
        B = args.batch if args.batch != 64 else 256
        m = QFormerForItemRepresentation(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                                         num_query_tokens=32, field_embedding_dim=1024, num_fields=14,
                                         dropout=0.2 if p is None else p).to(device).train()
        def fields():
            x = torch.randn(B, 14, 1024, generator=g); x = x / x.norm(dim=-1, keepdim=True)
            mk = (torch.rand(B, 14, generator=g) < 0.8).long(); mk[:, 0] = 1
            return (x * mk[..., None]).to(device), mk.to(device)
        (xa, ma), (xp, mp), (xn, mn) = fields(), fields(), fields()
        xpn, mpn = torch.cat([xp, xn]), torch.cat([mp, mn])
        loss_fn = QFormerLoss(data_parallel=True)       # the masked MSE divides by the all-reduced sum of the mask
        dp.set_dp_rank(rank, m)                # dropout masks keyed on the global sample index: same seeds, counters offset by rank * B
        pack = m._ensure_pack(device)
        opt = FusedAdamW([pack], lr=1e-4)
        bk = dp.GradBuckets(pack.grad, [0, pack.numel])
        merged = os.environ.get("UNIREC_ITEM_MERGED", "1") != "0"      # 0: anchor forward + one no-grad forward of positives | negatives
        def step():          # training/item_qformer_training.py:117-131: anchor with grad, pos/neg without
            opt.zero_grad()
            if merged:       # samples are independent: anchor | positives | negatives share ONE forward of 3B items, the backward walks the anchor rows
                out, rep = m.forward_triplet(xa, ma, xpn, mpn); pr, nr = rep[:B], rep[B:]
            else:
                out = m(xa, ma)
                with torch.no_grad():
                    dp.set_sample_offset(rank * 2 * B, m)      # its own counters: rank r's 2B rows of the ranks' concatenated pos|neg forwards
                    rep = m(xpn, mpn)["item_representation"]; pr, nr = rep[:B], rep[B:]
                    dp.set_sample_offset(None, m)
            loss, _, _ = loss_fn(out, {"field_embeddings": xa}, pr, nr, ma)
            loss.backward(); bk.ready_all(); bk.wait(); opt.step(grad_scale=1.0 / world)
            return loss
        unit, metric = "items/sec", ("items/sec item Q-Former triplet step (C2: L12 Q32 H768 F14, one forward of anchor|positives|negatives, backward over the anchor rows, AdamW)" if merged else
                        "items/sec item Q-Former triplet step (C2: L12 Q32 H768 F14, anchor fwd+bwd, positives|negatives in one no-grad fwd, AdamW)")
        flops = 2 * 8.0e12 / 256 * B / 2          # 8.0 TFLOP per 256-item triplet step
    else:
        from unirec_amd.user_qformer import UserQFormer
        B = args.batch if args.batch != 64 else 512
        T = args.hist * 32
        m = UserQFormer(dropout=0.1 if p is None else p).to(device).train()
        x = (torch.randn(B, T, 1024, generator=g) * 0.8).to(device).to(torch.bfloat16)
        lens = torch.randint(T // 2, T + 1, (B,), generator=g)
        mask = (torch.arange(T)[None, :] < lens[:, None]).float().to(device)
        x = x * mask[..., None].to(torch.bfloat16)
        # fraction of the T keys a launch actually sweeps (ragged histories: the forward / dQ kernels stop at the last 64-key tile that holds a
        # valid key, the few-query dK/dV kernel skips 32-key blocks without one) -- `GB_per_s_swept` of the cross-attention entries below
        swept_frac = float((((lens + 63) // 64) * 64).clamp(max=T).double().mean() / T)
        tgt = (torch.randn(B, 32, 1024, generator=g) * 0.8).to(device)
        dp.set_dp_rank(rank, m)                # dropout masks keyed on the global sample index: same seeds, counters offset by rank * B
        pack = m._ensure_pack(device)
        opt = FusedAdamW([pack], lr=1e-4)
        bk = dp.GradBuckets(pack.grad, [0, pack.numel])
        def step():          # training/user_qformer_training.py:203-214
            opt.zero_grad()
            loss = mse_loss(m(x, mask), tgt)
            loss.backward(); bk.ready_all(); bk.wait(); opt.step(grad_scale=1.0 / world)
            return loss
        unit, metric = "user-sequences/sec", f"user-sequences/sec user Q-Former step (C3: L4 Q64 H1024, T={T}, fwd+bwd+AdamW)"
        flops = 55.6e12 / 512 * B * (T / 1600.0)
    dist_on = torch.distributed.is_available() and torch.distributed.is_initialized()

    def sync():
        if dist_on:
            torch.distributed.barrier()
        torch.cuda.synchronize()
    for _ in range(args.warmup):
        step()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    t_host = time.perf_counter() - t0          # the host has issued every launch of the timed steps (nothing synchronises inside a step)
    sync()
    dt = time.perf_counter() - t0
    if dist_on:
        t = torch.tensor([dt], device=device, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t.item())
    if getattr(args, "dump_outputs", None) and rank == 0:
        dump_outputs(args.dump_outputs, {"loss": loss, "params_sample": pack_sample(pack.master), "grad_sample": pack_sample(pack.grad)})

    def line(**full):
        """The stage's line (rank 0), with the --full measurements (`full`) inside."""
        return {"metric": metric, "value": round(world * B * args.steps / dt, 2), "unit": unit, "n_gpus": world, "steps": args.steps,
                "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 2), "host_issue_ms_per_step": round(t_host / args.steps * 1e3, 2),
                "higher_is_better": True, "scaling": "weak",
                "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
                "config": {"workload": args.workload, "per_gpu_batch": B, "global_batch": B * world, "dropout": "off" if args.no_dropout else "on",
                           "parallelism": f"dp{world}"},
                "step_tflops_per_gpu": round(flops / (dt / args.steps) / 1e12, 1), "loss": round(float(loss.detach()), 5),
                "max_mem_gb": round(torch.cuda.max_memory_allocated() / 2**30, 1), **full, "comm": _comm_info(world)}

    if not args.full:
        return line() if rank == 0 else None
    # roofline leg: HIP events around every GEMM launch, in a SEPARATE pass of the same step right after the timed region -- a stage step
    # is ~270 GEMM launches of 20-100 us, and two event objects + records per launch cost the timed loop 5-20 % on a slow host core
    # (the C4 line keeps its events inside the timed region: 1190 launches per 430 ms)
    nprof = max(1, min(args.steps, 10))
    hip.PROFILE = []
    for _ in range(nprof):
        step()
    sync()
    prof, hip.PROFILE = hip.PROFILE, None
    # ... and one more pass with events around every attention launch, aggregated per SHAPE (so the few-query cross-attention launches
    # -- the north-star's small-Q / large-KV kernel -- read separately from the self-attention ones)
    hip.PROFILE_ATTN = []
    for _ in range(min(nprof, 3)):
        step()
    sync()
    aprof, hip.PROFILE_ATTN = hip.PROFILE_ATTN, None
    if rank == 0:
        # roofline of the dominant kernel family of the stage: every MFMA GEMM launch of the timed region (projections,
        # dX, token-reduction dW), HIP events on the launching stream
        g_ms = sum(e0.elapsed_time(e1) for (e0, e1, *_r) in prof)
        g_fl = sum(2.0 * M * N * K for (_e0, _e1, _rk, _sk, _f32, M, N, K, _sp, _epi) in prof)
        if os.environ.get("UNIREC_GEMM_SHAPES") == "1":       # lab: the stage's GEMM launches aggregated by shape, on stderr
            import collections
            agg = collections.defaultdict(lambda: [0, 0.0])
            for (e0, e1, rk, sk, f32, M, N, K, sp, epi) in prof:
                agg[(M, N, K, rk, sk, f32, sp, epi)][0] += 1; agg[(M, N, K, rk, sk, f32, sp, epi)][1] += e0.elapsed_time(e1)
            for k, (n, ms) in sorted(agg.items(), key=lambda kv: -kv[1][1])[:30]:
                print(f"M={k[0]:7d} N={k[1]:5d} K={k[2]:7d} rk={int(k[3])} sk={int(k[4])} f32={int(k[5])} split={k[6]:3d} epi={k[7]}: {n // nprof:4d}/step x "
                      f"{ms / n * 1e3:7.1f} us = {ms / nprof:6.2f} ms/step  {2.0 * k[0] * k[1] * k[2] * n / ms / 1e9:7.1f} TFLOP/s", file=sys.stderr)
        ach = g_fl / (g_ms * 1e-3) / 1e12 if g_ms > 0 else 0.0
        roof = {"bound": "mfma", "achieved": round(ach, 1), "peak": 2500.0, "unit": "TFLOP/s", "frac": round(ach / 2500.0, 4), "traffic": None, "peak_device": device_peaks(),
                "kernel": "gemm_kernel<...> (all MFMA GEMM launches of the stage)", "launches": len(prof),
                "avg_launch_ms": round(g_ms / max(len(prof), 1), 4), "gemm_ms_per_step": round(g_ms / nprof, 2),
                "events": f"separate pass of {nprof} steps right after the timed region (same process, same inputs)",
                "step_frac_of_peak": round(flops / (dt / args.steps) / 2.5e15, 4)}
        # attention launches by shape: K | V (and dK | dV) bytes once per pass against the HBM peak (forward / dQ read K | V; the backward
        # launch = dQ + dK/dV reads K | V twice and writes dK | dV once)
        ashape = {}
        for (e0, e1, kind, aB, aSq, aSk, anq, ahd, acausal) in aprof:
            v = ashape.setdefault((kind, aSq, aSk), [0.0, 0, aB, anq, ahd])
            v[0] += e0.elapsed_time(e1); v[1] += 1
        attn_shapes = {}
        for (kind, aSq, aSk), (ms, n, aB, anq, ahd) in sorted(ashape.items()):
            kvb = 2.0 * aB * aSk * anq * ahd * 2           # K | V bytes of one pass (bf16; one kv head per query head in the Q-Formers)
            nbytes = kvb if kind == "fwd" else 3.0 * kvb   # bwd: K | V twice + dK | dV once (the masked key tail is not read: an upper bound)
            attn_shapes[f"{kind}_q{aSq}_k{aSk}"] = {"launches_per_step": n // max(1, min(nprof, 3)), "avg_launch_us": round(ms / n * 1e3, 1),
                                                    "GB_per_s_upper": round(nbytes / (ms / n) / 1e6, 1)}
            if args.workload == "user" and aSk == T:      # the ragged cross-attention: bytes of the key tiles the kernels sweep (valid histories, mean swept_frac of T)
                attn_shapes[f"{kind}_q{aSq}_k{aSk}"].update({"GB_per_s_swept": round(nbytes * swept_frac / (ms / n) / 1e6, 1), "swept_frac": round(swept_frac, 4),
                                                           "hbm_fraction_swept": round(nbytes * swept_frac / (ms / n) / 1e6 / 8000.0, 4)})
        roof["attention_by_shape"] = attn_shapes
        out = line(roofline=roof)
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline_subprocess(args)
        else:
            out["cpu_baseline_note"] = "the CPU oracle leg runs on rank 0 of the N=1 line only"
        return out
    return None


def measure_item_c1(args, rank, world, device, g):
    """BASELINE configs[0] (C1) on the GPU: the evaluate_item_qformer.py path -- eval-mode forward of the tiny item Q-Former (L2 Q4 H256 nh4
    I1024 F8 E256) over a batch of 16 cached field embeddings + the masked MSE / cosine sums (ur_recon_stats) INSIDE the timed call
    (evaluation/evaluate_item_qformer.py:66-104).  A forward is ~40 launches of a few microseconds: the line reports the latency of one call
    as issued launch by launch and, when the capture succeeds, as ONE hipGraph replay (the launch-bound inner loop the graph is for)."""
    from unirec_amd import hip
    from unirec_amd.qformer_utils import QFormerForItemRepresentation
    B, F, E = 16, 8, 256
    m = QFormerForItemRepresentation(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=1024, num_query_tokens=4,
                                     field_embedding_dim=E, num_fields=F, dropout=0.2).to(device).eval()
    x = torch.randn(B, F, E, generator=g); x = x / x.norm(dim=-1, keepdim=True)
    mk = (torch.rand(B, F, generator=g) < 0.8).long(); mk[:, 0] = 1
    x = (x * mk[..., None]).to(device)
    mk = mk.to(device)
    mkf = mk.float()

    def call():
        with torch.no_grad():
            out = m(x, mk)
            return hip.recon_stats(out["reconstructed_fields"].contiguous(), x, mkf)

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n, r
    reps = 200
    for _ in range(10):
        call()
    dt, sums = timed(call, reps)
    graph = {"captured": False}
    try:                         # one hipGraph replay per call (stream capture on a side stream; allocations come from the graph's private pool)
        if world > 1:            # (a process group's watchdog thread may touch the device during a global-mode capture: the single-rank line carries the graph number)
            raise RuntimeError("hipGraph capture is measured on the single-rank line only")
        gr = torch.cuda.CUDAGraph()
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            for _ in range(3):
                call()
        torch.cuda.current_stream().wait_stream(st)
        with torch.cuda.graph(gr, stream=st):
            gsums = call()
        for _ in range(10):
            gr.replay()
        dtg, _ = timed(gr.replay, reps)
        same = bool(torch.equal(gsums, sums))
        graph = {"captured": True, "latency_us": round(dtg * 1e6, 1), "items_per_s": round(B / dtg, 1), "bit_identical_to_the_launch_by_launch_call": same}
    except Exception as e:       # noqa: BLE001 -- the launch-by-launch number stands on its own
        graph = {"captured": False, "error": f"{type(e).__name__}: {str(e)[:160]}"}
    if rank != 0:
        return None
    if getattr(args, "dump_outputs", None):
        dump_outputs(args.dump_outputs, {"recon_stats": sums.double()})
    sums = sums.float().cpu().tolist()
    # bytes one call has to move: the live bf16 weights once + the field embeddings + the reconstruction read back by the metric kernel
    live = sum(p_.numel() for n_, p_ in m.named_parameters() if n_ in m._ensure_pack(device).params)
    nbytes = 2.0 * live + 4.0 * B * F * E * 3
    best = min(dt, graph.get("latency_us", 1e30) * 1e-6)
    roof = {"bound": "hbm", "achieved": round(nbytes / best / 1e9, 2), "peak": 8000.0, "unit": "GB/s", "frac": round(nbytes / best / 1e9 / 8000.0, 6), "traffic": None,
            "note": f"latency-bound: {nbytes / 1e6:.2f} MB of weights + inputs per call; the call is a chain of ~40 dependent launches over 64 query rows, not a stream"}
    out = {"metric": "items/sec item Q-Former eval forward + reconstruction metrics (C1: L2 Q4 H256 nh4 I1024 F8 E256, batch 16; evaluate_item_qformer.py path)",
           "value": round(world * B / best, 1), "unit": "items/sec", "n_gpus": world, "steps": reps, "warmup": 10, "ms_per_step": round(best * 1e3, 4),
           "latency_us": {"launch_by_launch": round(dt * 1e6, 1), "hip_graph": graph.get("latency_us")}, "hip_graph": graph,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
           "config": {"workload": "item_c1", "per_gpu_batch": B, "mode": "eval (dropout off)", "eval_mse": round(sums[0] / max(sums[1], 1.0), 6), "eval_cos_mean": round(sums[2] / max(sums[1], 1.0), 6)},
           "max_mem_gb": round(torch.cuda.max_memory_allocated() / 2**30, 2), "roofline": roof}
    if args.full and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline_subprocess(args)
    return out


def _check_world(args, world):
    """--gpus N must be the number of ranks that actually run (a silent 1-rank run would report a 1-GPU number as N)."""
    if world != args.gpus and os.environ.get("UNIREC_DP_FORCE") != "1":
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; launch with\n  python -m torch.distributed.run --nnodes=1 "
                         f"--nproc-per-node {args.gpus} --master-addr 127.0.0.1 --master-port 29500 bench.py --gpus {args.gpus} ...\n"
                         f"(or plain `python bench.py --gpus {args.gpus}`, which starts the ranks itself)")


def _comm_info(world):
    """What the gradient all-reduce actually ran on: backend and number of ranks of the initialised process group."""
    d = torch.distributed
    if d.is_available() and d.is_initialized():
        be = d.get_backend()
        from unirec_amd import dp as _dp
        if _dp._native:          # the buckets went through the library's own communicator (default for multi-rank RCCL runs; UNIREC_DP_COMM=torch opts out)
            c = next(iter(_dp._native.values()))
            return {"backend": "rccl (native ur_comm_*; rendezvous over torch.distributed " + be + ")", "ranks": c.world, "allreduce_launches": c.launches}
        return {"backend": "rccl (torch.distributed nccl)" if be == "nccl" else be, "ranks": d.get_world_size()}
    return {"backend": None, "ranks": 1}


# ---- --dump-outputs: what the last timed step computed, for an output-for-output comparison of two builds ----------------
DUMP_SAMPLE = 1 << 20          # elements kept of a flat parameter / gradient pack larger than this (a fixed, seeded sample)
DUMP_LIMIT = 64 << 20          # bytes one dump may write


def pack_sample(t, seed=0):
    """The flat tensor t whole when it holds at most DUMP_SAMPLE elements, else DUMP_SAMPLE of its elements at sorted indices
    drawn (with replacement) from a CPU generator seeded with `seed`: a pack of the same size is sampled at the same indices."""
    t = t.detach().reshape(-1)
    if t.numel() <= DUMP_SAMPLE:
        return t
    idx = torch.randint(0, t.numel(), (DUMP_SAMPLE,), generator=torch.Generator().manual_seed(seed)).sort().values
    return t[idx.to(t.device)]


def dump_outputs(path, arrays):
    """name -> tensor, written as path/<name>.npy: float64 for scalars and float64 tensors, float32 for everything else."""
    import numpy as np
    host = {k: (t.detach().double() if t.numel() == 1 or t.dtype == torch.float64 else t.detach().float()).cpu().numpy()
            for k, t in arrays.items()}
    nbytes = sum(a.nbytes for a in host.values())
    if nbytes > DUMP_LIMIT:
        raise SystemExit(f"bench.py: --dump-outputs would write {nbytes} bytes (limit {DUMP_LIMIT})")
    os.makedirs(path, exist_ok=True)
    for k, a in host.items():
        np.save(os.path.join(path, k + ".npy"), a)


def main():
    args = parse()
    if args.cpu_baseline_only:
        if args.workload != "joint":
            print(json.dumps(cpu_baseline_stage(args)), flush=True)
            return
        from unirec_amd.qwen3 import Qwen3Config
        print(json.dumps(cpu_baseline(args, Qwen3Config(num_hidden_layers=args.layers), (2, 14, 1024, 1024))), flush=True)
        return
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: this process has not touched the GPU (no HIP call so far) -- start the N ranks
        # as CHILD processes under torch.distributed.run, relay their output (rank 0 prints the JSON line) and leave with
        # the launcher's exit code.  Never re-exec: the parent just waits.
        from unirec_amd import dp
        raise SystemExit(dp.launch_ranks(args.gpus, os.path.abspath(__file__), sys.argv[1:]))
    if args.workload != "joint":
        return run_stage(args)
    from unirec_amd import dp
    rank, world, local = dp.init_from_env()
    _check_world(args, world)
    device = torch.device("cuda", local % max(1, torch.cuda.device_count()))      # (modulo: gloo rehearsal of N ranks on one GPU)
    torch.cuda.set_device(device)
    out = measure_joint(args, rank, world, device)
    if out is False:
        return
    dist_on = torch.distributed.is_available() and torch.distributed.is_initialized()
    import gc
    # ---- per-stage lines (BASELINE configs[0], [1], [2], [4]), measured in this same process after the headline; every rank
    # takes part (the stages all-reduce their gradient packs like the joint step); --full only
    stages = {}
    if args.full and args.stages and args.batch == 64 and args.hist == 50 and args.seq == 2048 and not args.user_tokens and args.layers == 28:
        gc.collect(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        for wl, key in (("item_c1", "item_c1"), ("item", "item_c2"), ("user", "user_c3")):
            sa = argparse.Namespace(**{**vars(args), "workload": wl, "steps": args.stage_steps, "warmup": 3, "cpu_budget": args.stage_cpu_budget,
                                       "dump_outputs": None})
            so = measure_stage(sa, rank, world, device)
            if rank == 0:
                stages[key] = {k: so[k] for k in ("metric", "value", "unit", "steps", "ms_per_step", "latency_us", "host_issue_ms_per_step", "step_tflops_per_gpu", "max_mem_gb", "config", "roofline", "hip_graph") if k in so}
                if "cpu_baseline" in so:
                    stages[key]["cpu_baseline"] = so["cpu_baseline"]
            gc.collect(); torch.cuda.empty_cache()
        if args.c5_stage and (world == 1 or args.c5_stage_multi):
            # BASELINE configs[4] (C5): the C4 step with hist 100, S 4096, pool 10000 and the User Q-Former's 64 tokens (U4), B 64 as ONE launch
            # (recompute_mlp keeps it inside 288 GB); 1 warm-up + 2 timed steps, its own roofline / attention / cpu_baseline on a bounded sample
            torch.cuda.reset_peak_memory_stats()
            # gate|up / act of the LAST 14 layers are kept (4.8 GB each at 262144 tokens: ~262 GB of 288), the first 14 rebuilt in the backward;
            # should the allocator refuse, the line falls back to rebuilding all 28 (201.8 GB) and says so in config.recompute_mlp
            ca = argparse.Namespace(**{**vars(args), "hist": 100, "seq": 4096, "pool": 10000, "user_tokens": True, "recompute_mlp": False, "recompute_mlp_layers": int(os.environ.get("UNIREC_BENCH_C5_REBUILD_LAYERS", "14" if world == 1 else "20")),      # (multi-rank: room for the communicator's buffers; no fallback there)
                                       "steps": 2, "warmup": 1, "micro_batches": 1, "cpu_budget": args.c5_cpu_budget, "cpu_runs": 1, "dump_outputs": None})
            refused = False
            try:
                so = measure_joint(ca, rank, world, device, side_steps=1)
            except torch.cuda.OutOfMemoryError:
                if world > 1:
                    raise                      # (ranks must not diverge: a multi-rank run states its own budget)
                refused = True                 # (retry OUTSIDE the handler: the exception's traceback keeps the failed attempt's model and activations alive)
            if refused:
                gc.collect(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
                ca.recompute_mlp, ca.recompute_mlp_layers = True, 0
                so = measure_joint(ca, rank, world, device, side_steps=1)
            if rank == 0 and so:
                stages["joint_c5"] = {k: so[k] for k in ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "step_tflops_per_gpu", "loss", "max_mem_gb", "config", "roofline", "attention", "comm",
                                                         "cpu_baseline") if k in so}
            gc.collect(); torch.cuda.empty_cache()
    if rank == 0:
        if stages:
            out["stages"] = stages
        print(json.dumps(out), flush=True)
    if dist_on:
        dp.close_native_comms()
        torch.distributed.destroy_process_group()


def measure_joint(args, rank, world, device, side_steps=3):
    """One joint workload (C4 by default; C5 with --user-tokens --hist 100 --seq 4096 --pool 10000) on an initialised device / process group
    -> the line's JSON object (rank 0), None on the other ranks, False when a lab switch already printed its own line."""
    from unirec_amd import dp, hip
    from unirec_amd.joint import InfoNCELoss
    from unirec_amd.optim import FusedAdamW
    model, qf, cfg, dims = build(args, device)
    Qi, F, E, D = dims
    B = args.batch
    n_user = model.num_user_query_tokens
    batch = make_batch(B, args.hist, args.seq, args.pool, F, E, D, Qi, model.first_special_id, model.first_special_id,
                       1234 + rank, device, n_user=n_user)
    loss_fn = InfoNCELoss(0.07)
    qw = model.base_model
    qw.recompute_mlp = bool(args.recompute_mlp) or qw.recompute_mlp
    if getattr(args, "recompute_mlp_layers", 0) > 0 and not args.recompute_mlp:
        qw.recompute_mlp = int(args.recompute_mlp_layers)
    dp.set_dp_rank(rank, model, qf)                # dropout / LoRA-dropout masks keyed on the global sample index (same seeds on every rank)
    qpack, lpack = qf._ensure_pack(device), qw._ensure_pack(device)
    packs = [qpack, lpack]
    ubk = upack = None
    if model.user_qformer is not None:
        upack = model.user_qformer._ensure_pack(device)
        packs.append(upack)
        ubk = dp.GradBuckets(upack.grad, [0, upack.numel])      # the user Q-Former's gradients: one bucket after the backward
    opt = FusedAdamW(packs, lr=1e-4, weight_decay=0.01)

    # ---- gradient buckets in backward-completion order (LoRA 27..0, Q-Former 11..0, query table) ----
    lgrp, qgrp = 7, 1          # LoRA: 4 buckets of 7 layers (10 MB each); Q-Former: one bucket per layer (60 MB f32): the exposed tail is the small query-table bucket
    l_pre, q_pre = [f"layers.{i}." for i in range(cfg.num_hidden_layers)], [f"qformer.encoder.layer.{i}." for i in range(12)]
    lb = dp.layer_boundaries(lpack, l_pre, lgrp)
    qb = dp.layer_boundaries(qpack, q_pre, qgrp)           # [query table + embedding LN | hoisted cross-attention K|V of all layers | layer 0 | ... | layer 11 | heads]
    # --comm-bf16 (opt-in): the item Q-Former's buckets travel as bf16 (its f32 gradients become final in the last milliseconds of the backward)
    lbk, qbk = dp.GradBuckets(lpack.grad, lb), dp.GradBuckets(qpack.grad, qb, wire_dtype=torch.bfloat16 if args.comm_bf16 else None)
    qw.grad_ready_hook = dp.bucket_hook(lpack, lbk, l_pre, lgrp)
    qf.qformer.grad_ready_hook = dp.bucket_hook(qpack, qbk, q_pre, qgrp)      # -2: the hoisted K|V gradients leave from their own hook, -1: the query table

    comm_on, waits = bool(lbk.enabled or qbk.enabled), []
    nmb = max(1, args.micro_batches)
    if B % nmb:
        raise SystemExit(f"--batch {B} is not a multiple of --micro-batches {nmb}")
    mb = B // nmb
    dump = getattr(args, "dump_outputs", None)
    users = []                  # --dump-outputs: the user embeddings of the latest step, one entry per micro-batch

    def step():
        opt.zero_grad()
        total = None
        del users[:]
        for k in range(nmb):
            sl = slice(k * mb, (k + 1) * mb)
            last = k == nmb - 1
            for bk in (lbk, qbk, ubk):
                if bk is not None:
                    bk.begin_micro_batch(last)
            if nmb > 1:         # dropout counters follow the GLOBAL sample index: rank r's micro-batch k starts at r * B + k * mb
                dp.set_sample_offset(rank * B + k * mb, model, qf, model.user_qformer)
            ut, um = batch["user_sequence_tokens"], batch["user_attention_mask"]
            user = model(batch["input_ids"][sl], batch["attention_mask"][sl], batch["history_field_embeddings"][sl],
                         batch["history_attention_mask"][sl], None if ut is None else ut[sl], None if um is None else um[sl])
            if dump:
                users.append(user.detach())
            nm = batch["negative_masks"]
            loss = loss_fn(user, batch["positive_item_embeddings"][sl], batch["negative_item_embeddings"][sl], None if nm is None else nm[sl])
            if nmb > 1:
                loss = loss / nmb               # mean over the whole batch = mean of the micro-batch means
            loss.backward()
            if ubk is not None:
                ubk.ready_all()
            total = loss.detach() if total is None else total + loss.detach()
        # the step stream now WAITS for the bucket all-reduces still in flight on the communicator's side stream: HIP events around the waits
        # time what the backward did not cover (`comm.exposed_wait_ms_per_step`; two records per step, only when a process group is up)
        if comm_on:
            w0, w1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            w0.record()
        if ubk is not None:
            ubk.wait()
        lbk.wait(); qbk.wait()
        if comm_on:
            w1.record()
            waits.append((w0, w1))
        opt.step(grad_scale=1.0 / world)
        return total

    dist_on = torch.distributed.is_available() and torch.distributed.is_initialized()    # world > 1 (or UNIREC_DP_FORCE=1)

    def sync():
        if dist_on:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    sync()
    # --full, inside the timed region: HIP events around the launches of the DOMINANT family only (the projection GEMMs: `roofline`).  The
    # events of the attention launches and of the HBM-bound families (1000+ more per step; every timed record is a barrier packet, together
    # 4-6 ms of a 425 ms step: same-box A/B with UNIREC_BENCH_EVENTS=0) run in a separate pass of the same step after the timed region.
    # A plain run records no events at all.
    ev_in_loop = os.environ.get("UNIREC_BENCH_EVENTS", "1") != "0"      # lab: 0 = no HIP events inside the timed region at all
    if ev_in_loop and args.full:
        hip.PROFILE = []
    del waits[:]
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    sync()
    dt = time.perf_counter() - t0
    comm_extra = {}
    if comm_on:
        nb = [bk for bk in (lbk, qbk, ubk) if bk is not None]
        comm_extra = {"exposed_wait_ms_per_step": round(sum(a.elapsed_time(b) for a, b in waits) / max(len(waits), 1), 3),
                      "buckets": {"lora": lbk.n, "item_qformer": qbk.n, **({"user_qformer": ubk.n} if ubk is not None else {})},
                      "bytes_per_step": int(sum((2 if bk.wire_on else 4) * sum(max(0, bk.bounds[i + 1] - bk.bounds[i]) for i in range(bk.n)) for bk in nb)),
                      "wire": {"lora": "f32", "item_qformer": "bf16" if qbk.wire_on else "f32"},
                      "exposed_wait_note": "HIP events on the step stream around GradBuckets.wait() of every pack: the time the stream stalls on bucket tickets the backward did not cover (0 when the all-reduces hide)"}
    del waits[:]
    if not ev_in_loop:
        print(json.dumps({"ms_per_step_without_events": round(dt / args.steps * 1e3, 2)}), flush=True)
        return False
    prof, hip.PROFILE = hip.PROFILE, None
    if dist_on:
        t = torch.tensor([dt], device=device, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t.item())
    lossv = float(loss.item())
    if not math.isfinite(lossv):
        raise SystemExit("non-finite loss")
    # what the timed steps left in the trainable parameters (f64 sums of the flat fp32 masters): equal runs give equal digits,
    # and under data parallelism every rank must print the same ones (tests/test_gpu_dp_rccl.py)
    checksum = {"lora": float(lpack.master.double().abs().sum().item()), "qformer": float(qpack.master.double().abs().sum().item())}
    if dump and rank == 0:      # before the side pass below steps the model again
        arrays = {"loss": loss, "user_embeddings": torch.cat(users)}
        for name, pack in (("lora", lpack), ("qformer", qpack), ("user_qformer", upack)):
            if pack is not None:
                arrays[f"{name}_params_sample"] = pack_sample(pack.master)
                arrays[f"{name}_grad_sample"] = pack_sample(pack.grad)
        dump_outputs(dump, arrays)

    def headline(**full):
        """The line's object (rank 0): the headline and what the timed steps left, with the --full measurements (`full`) inside."""
        return {"metric": f"user-sequences/sec joint fwd+bwd (Qwen3-0.6B+LoRA, hist={args.hist})", "value": round(world * B * args.steps / dt, 3),
                "unit": "user-sequences/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": round(dt / args.steps * 1e3, 2), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                "dtype": "bf16", "data": "synthetic",
                "config": {"workload": ("C5-shaped joint step with the User Q-Former's 64 tokens (U4): " if n_user else "C4 joint step: ") +
                                       f"item Q-Former(L12,H1024,Q2,F14) on {B}x{args.hist} items -> inject -> "
                                       f"Qwen3-0.6B-shaped({cfg.num_hidden_layers}L)+LoRA r16 -> mean-pool -> InfoNCE pool {args.pool}; "
                                       f"fwd+bwd+allreduce+AdamW", "per_gpu_batch": B, "global_batch": B * world, "seq_len": args.seq,
                           "hist": args.hist, "pool": args.pool, "dropout": 0.0 if args.no_dropout else 0.2, "lora_dropout": 0.0 if args.no_dropout else args.lora_dropout,
                           "micro_batches": nmb, "recompute_mlp": (qw.recompute_mlp if isinstance(qw.recompute_mlp, bool) else f"layers 0..{int(qw.recompute_mlp) - 1}"), "parallelism": f"dp{world}", "random_init": True},
                "step_tflops_per_gpu": round(flops_per_step(args, B, cfg, dims) / (dt / args.steps) / 1e12, 1), "loss": round(lossv, 4),
                "max_mem_gb": round(torch.cuda.max_memory_allocated() / 2**30, 1), **full, "comm": {**_comm_info(world), **comm_extra}, "param_checksum": checksum}

    if not args.full:
        qw.grad_ready_hook = None             # (the hooks hold the buckets: drop the cycle so the packs can be freed)
        qf.qformer.grad_ready_hook = None
        return headline() if rank == 0 else None
    # the side pass: attention and HBM-bound family events (all ranks run it: the step holds collectives)
    nside = max(1, min(args.steps, side_steps))
    hip.PROFILE_ATTN, hip.PROFILE_STREAM = [], []
    for _ in range(nside):
        step()
    sync()
    aprof, hip.PROFILE_ATTN = hip.PROFILE_ATTN, None
    sprof, hip.PROFILE_STREAM = hip.PROFILE_STREAM, None

    if rank == 0:
        # ---- roofline of the dominant kernel: forward projection GEMM gemm_kernel<RK=1,SK=1,bf16> -----
        tot_ms, tot_fl, n = 0.0, 0.0, 0
        pl_ms, pl_fl, pl_n = 0.0, 0.0, 0
        x1_ms, x1_fl = 0.0, 0.0
        all_ms, all_fl = 0.0, 0.0
        for (e0, e1, rk, sk, f32, M, N, K, split, epi) in prof:
            ms = e0.elapsed_time(e1)
            all_ms += ms; all_fl += 2.0 * M * N * K
            # The family of rounds 1-2: every K-contiguous bf16 projection launch on 256x256 tiles (forward q|k|v, o, gate|up, down
            # and the frozen-weight dX launches), whatever rides in its epilogue now -- q/k-norm + RoPE (3) and the SwiGLU forward (4)
            # are counted with their GEMM FLOPs only, so fusing work into a launch can only LOWER this number.  Round 5 (VERDICT round 4,
            # item 2): the down-projection dX launch that carries the SwiGLU backward (1: 3.2 GB of gate|up / dgate|dup traffic ride on
            # it, 0.28 of peak) is INSIDE `frac` too; `frac_without_swiglu_backward` is the number of rounds 1-4.
            # Tile rule = csrc/gemm.hip launch() / csrc/gemm_pers.hip gemm_pers_eligible().
            tiles = (-(-M // 256)) * (-(-N // 256)) * max(split, 1)
            if epi in (0, 1, 3, 4) and rk and sk and not f32 and M >= 256 and N >= 256 and tiles >= (128 if epi else 256):
                tot_ms += ms; tot_fl += 2.0 * M * N * K; n += 1
                if epi == 1:
                    x1_ms += ms; x1_fl += 2.0 * M * N * K
                if epi == 0:
                    pl_ms += ms; pl_fl += 2.0 * M * N * K; pl_n += 1
        ach = tot_fl / (tot_ms * 1e-3) / 1e12 if tot_ms > 0 else 0.0
        e1_ms = sum(e0.elapsed_time(e1) for (e0, e1, rk, sk, f32, M, N, K, split, epi) in prof if epi == 1)
        e1_fl = sum(2.0 * M * N * K for (e0, e1, rk, sk, f32, M, N, K, split, epi) in prof if epi == 1)
        e1_n = sum(1 for r_ in prof if r_[9] == 1)
        peaks = device_peaks()
        # HBM-bound families (hbm_fraction = algorithmic bytes / (time x peak bandwidth)), HIP events around every launch
        fam = {}
        for (e0, e1, family, nbytes) in sprof:
            f_ = fam.setdefault(family, [0.0, 0, 0])
            f_[0] += e0.elapsed_time(e1); f_[1] += nbytes; f_[2] += 1
        streams = {k: {"launches": v[2], "ms_per_step": round(v[0] / nside, 3), "GB_per_s": round(v[1] / max(v[0], 1e-9) / 1e6, 1),
                       "hbm_fraction": round(v[1] / max(v[0], 1e-9) / 1e6 / peaks["hbm_GBps_spec"], 4)} for k, v in sorted(fam.items())}
        if "lora_bits" in streams:
            # the flag planes (and their token-packed copies) of step n + 1 are generated on a SIDE stream under step n's Q-Former backward:
            # kernel time beside the step, not in it (profiles/r4_ab_step.txt)
            streams["lora_bits"]["side_stream"] = True
        streams["_sum_on_the_step_stream_ms"] = round(sum(v["ms_per_step"] for k, v in streams.items() if isinstance(v, dict) and not v.get("side_stream")
                                                          and k not in ("adamw", "J6_candidate_scores")), 2)
        # HBM-side bytes of one launch from the separate rocprofv3 --pmc passes (profiles/r2_gemm_pmc.json: FETCH_SIZE x2 +
        # WRITE_SIZE, the MI355X_MICROARCH corrections); bench.py itself cannot collect PMC counters.  Reported for the
        # largest launch of the family, the merged gate|up forward (M=131072, N=6144, K=1024).
        traffic, tnote = None, "no PMC summary found"
        try:
            pm = json.load(open(os.path.join(ROOT, "profiles", "r6_gemm_pmc.json")))["launches"]["gate|up fwd"]
            if B * args.seq == pm["M"]:
                traffic = pm["hbm_bytes"]
                tnote = (f"gate|up forward launch (N=6144, K=1024): fabric reads {pm['fabric_read_bytes']} (x{pm['read_ratio']} of A+W; FETCH_SIZE "
                         f"counts Infinity-Cache hits too) + writes {pm['write_bytes']} vs algorithmic {pm['algorithmic_bytes']} (x{pm['ratio']}); "
                         f"profiles/r6_gemm_pmc.json")
        except Exception:
            pass
        roof = {"bound": "mfma", "achieved": round(ach, 1), "peak": 2500.0, "unit": "TFLOP/s", "frac": round(ach / 2500.0, 4),
                "traffic": traffic, "peak_device": peaks,
                "swiglu_backward_launch": {"launches": e1_n, "avg_launch_ms": round(e1_ms / max(e1_n, 1), 4), "tflops": round(e1_fl / max(e1_ms, 1e-9) / 1e9, 1),
                                           "frac": round(e1_fl / max(e1_ms, 1e-9) / 1e9 / 2500.0, 4),
                                           "note": "gemm_pers_kernel<1, 2>: the down-projection dX launch that carries the SwiGLU backward in its epilogue (inside `frac` since round 5)"},
                "frac_without_swiglu_backward": round((tot_fl - x1_fl) / max(tot_ms - x1_ms, 1e-9) / 1e9 / 2500.0, 4),
                "frac_definition": "rounds 5+: every 256x256 K-contiguous projection launch INCLUDING the one that carries the SwiGLU backward (EPI 1); compare with BENCH_r01..r04 through frac_without_swiglu_backward",
                "hbm_bound_families": streams, "kernel": "gemm_pers_kernel<EPI 0|1|2|3|4|5, MODE> (every launch of the C4 step since the gate|up dX launch moved to it; other shapes: gemm_kernel<true,true,false,256,256,2,4,0>) (K-contiguous 256x256 projection GEMM: forward + "
                          "frozen-weight dX incl. the launch that carries the SwiGLU backward; the persistent kernel takes the launches csrc/gemm_pers.hip:gemm_pers_eligible "
                          "accepts; launches with a q/k-norm + RoPE, SwiGLU-forward or SwiGLU-backward epilogue are counted with their GEMM FLOPs only)",
                "plain_epilogue_launches": {"launches": pl_n, "avg_launch_ms": round(pl_ms / max(pl_n, 1), 4),
                                            "tflops": round(pl_fl / max(pl_ms, 1e-9) / 1e9, 1), "frac": round(pl_fl / max(pl_ms, 1e-9) / 1e9 / 2500.0, 4)},
                "traffic_note": tnote,
                "launches": n, "avg_launch_ms": round(tot_ms / max(n, 1), 4),
                "all_gemm_tflops": round(all_fl / (all_ms * 1e-3) / 1e12, 1) if all_ms > 0 else 0.0,
                "all_gemm_ms_per_step": round(all_ms / args.steps, 2),
                # the datasheet peak is a 2.4 GHz / zero-data number: a register-only v_mfma_f32_16x16x32_bf16 stream with random
                # operands sustains 2.05 PFLOP/s at this part's 1400 W cap, and this kernel runs at that cap
                "sustained_mfma_peak": 2050.0, "frac_of_sustained": round(ach / 2050.0, 4),
                "sustained_note": "tools/lab/mfma_power_lab.hip, profiles/r2_mfma_power_lab.txt, profiles/r2_power_gemm_step.txt"}
        # the causal attention family of the decoder (second-largest group of the step), HIP events around every launch; FLOPs are the
        # ALGORITHMIC dense-causal ones (forward 4 B nq S^2 hd / 2, backward 2.5x): left padding only makes the kernels skip work
        att = {"fwd": [0.0, 0.0, 0], "bwd": [0.0, 0.0, 0]}
        for (e0, e1, kind, aB, aSq, aSk, anq, ahd, acausal) in aprof:
            if acausal and ahd == 128:
                f = 4.0 * aB * anq * aSq * aSk * ahd / 2 * (1.0 if kind == "fwd" else 2.5)
                att[kind][0] += e0.elapsed_time(e1); att[kind][1] += f; att[kind][2] += 1
        attn = {k: {"launches": v[2], "avg_launch_ms": round(v[0] / max(v[2], 1), 4), "ms_per_step": round(v[0] / nside, 2),
                    "tflops": round(v[1] / max(v[0], 1e-9) / 1e9, 1), "frac_of_peak": round(v[1] / max(v[0], 1e-9) / 1e9 / 2500.0, 4)} for k, v in att.items()}
        # ... and on the EXECUTED FLOPs: what the kernels issue for this batch's masks (whole 64-key tiles incl. the masked half of
        # the diagonal ones, minus the leading all-padding key tiles they skip) -- the honest MFMA utilisation of the kernels
        ex = attn_executed_ratio(batch["attention_mask"], args.seq)
        for k in ("fwd", "bwd"):
            attn[k]["executed_over_algorithmic"] = round(ex[k], 4)
            attn[k]["frac_of_peak_executed"] = round(attn[k]["frac_of_peak"] * ex[k], 4)
        attn["events"] = streams["_events"] = f"separate pass of {nside} steps right after the timed region (same process, same batch)"
        attn["kernels"] = ("attn_fwd_c128_kernel; attn_bwd_dq_c128_kernel + attn_bwd_dkv_c128_kernel (one ur_attn_bwd call): main loops "
                           "generated by tools/asmgen (one wave per SIMD, hand-scheduled); executed_over_algorithmic counts the MFMAs they issue: "
                           "forward incl. the row-sum products, backward 7 contractions for the 5 algorithmic ones (S and dP in both kernels)")
        out = headline(roofline=roof, attention=attn)
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline_subprocess(args)
        elif world > 1:
            out["cpu_baseline_note"] = "the CPU oracle leg runs on rank 0 of the N=1 line only"
    qw.grad_ready_hook = None                 # (the hooks hold the buckets: drop the cycle so the packs can be freed before the next workload)
    qf.qformer.grad_ready_hook = None
    return out if rank == 0 else None


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What gradient-norm clipping costs the C4 joint step (one GPU).  Builds the C4 joint model as bench.py does, runs one backward
to find the live gradient spans (item Q-Former + LoRA packs), then times with HIP events (warm-up, median of --reps):
  * the norm + coef launches (ur_grad_norm_clip) over those spans,
  * the AdamW launches of FusedAdamW.step over the same runs: ur_adamw_step against ur_adamw_step_dev, alternating,
and prints TB/s of the bytes swept (norm: the gradients read once; AdamW: gradient read + parameter / moments read and written).
--step-ab N adds an alternating same-process A/B of N pairs of C4 JointTrainer.training_step with max_grad_norm 1.0 against off.
One JSON line on stdout.  Usage: python tools/clip_bench.py [--reps 30] [--step-ab 6] [--batch 64]"""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--step-ab", type=int, default=6, help="pairs of C4 training steps, clipped / unclipped, alternating (0: skip)")
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    import bench
    from unirec_amd import hip
    from unirec_amd.joint import JointTrainer
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    argv, sys.argv = sys.argv, sys.argv[:1]
    try:
        args = bench.parse()                 # bench.py's defaults: the C4 joint workload
    finally:
        sys.argv = argv
    args.batch = a.batch
    model, qf, cfg, dims = bench.build(args, dev)
    Qi, F, E, D = dims
    batch = bench.make_batch(a.batch, args.hist, args.seq, args.pool, F, E, D, Qi, model.first_special_id, model.first_special_id, 1234, dev)
    targs = types.SimpleNamespace(learning_rate=1e-4, warmup_steps=0, max_grad_norm=1.0, lr_scheduler_type="constant", weight_decay=0.0,
                                  logging_steps=0)
    tr = JointTrainer(model, targs, num_training_steps=1000)
    inputs = {k: batch[k] for k in ("input_ids", "attention_mask", "history_field_embeddings", "history_attention_mask",
                                    "positive_item_embeddings", "negative_item_embeddings", "negative_masks")}
    tr.training_step(inputs)                 # one real step: the live sets of the joint backward
    torch.cuda.synchronize()
    opt = tr.optimizer
    spans = [opt.packs[k].grad[lo:hi] for k, lo, hi in opt.grad_spans()]
    nbytes = sum(s.numel() * 4 for s in spans)
    norm, coef = torch.zeros((), device=dev), torch.ones((), device=dev)
    t_norm = timed(lambda: hip.grad_norm_clip(spans, 1.0, 1.0, norm, coef), a.reps)

    runs = []
    for pack, (m, v), steps in zip(opt.packs, opt.state, opt.steps):
        for lo, hi, t in pack.live_ranges(key=steps.__getitem__):
            runs.append((pack.master[lo:hi], pack.grad[lo:hi], m[lo:hi], v[lo:hi], t))
    adam_bytes = sum(7 * r[0].numel() * 4 for r in runs)          # p, m, v read + written, g read
    one = torch.ones((), device=dev)

    def adam(c):
        for p, g, m, v, t in runs:
            hip.adamw_step(p, g, m, v, 1e-4, 0.9, 0.999, 1e-8, 0.0, t, 1.0, coef=c)
    t_host, t_dev = [], []
    for _ in range(a.reps):          # alternating A / B, one launch set each
        t_host += timed(lambda: adam(None), 1, warmup=1)
        t_dev += timed(lambda: adam(one), 1, warmup=1)
    med = statistics.median
    out = {"tool": "clip_bench", "spans": len(spans), "span_bytes": nbytes, "adamw_runs": len(runs), "reps": a.reps,
           "norm_ms": med(t_norm), "norm_tb_s": nbytes / med(t_norm) / 1e9, "norm_ms_min": min(t_norm),
           "adamw_ms": med(t_host), "adamw_tb_s": adam_bytes / med(t_host) / 1e9,
           "adamw_dev_ms": med(t_dev), "adamw_dev_tb_s": adam_bytes / med(t_dev) / 1e9,
           "adamw_dev_over_adamw": med(t_dev) / med(t_host)}
    if a.step_ab > 0:
        on, off = [], []
        for _ in range(2):
            tr.training_step(inputs)
        for _ in range(a.step_ab):
            for clip, acc in ((1.0, on), (None, off)):
                opt.max_grad_norm = clip
                acc += timed(lambda: tr.training_step(inputs), 1, warmup=0)
        out.update({"step_ab_pairs": a.step_ab, "step_clip_ms": med(on), "step_noclip_ms": med(off),
                    "step_clip_minus_noclip_ms": med(on) - med(off), "step_clip_ms_all": on, "step_noclip_ms_all": off})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

"""One rank of the clipped JointTrainer step under data parallelism (tests/test_gpu_grad_clip.py starts one or two of these as
child processes on cuda:0, backend gloo).  The joint model (item Q-Former -> injection -> Qwen3 + LoRA -> InfoNCE, dropout 0.1
everywhere: masks keyed on the global sample index) takes one JointTrainer step on this rank's shard of a global batch.
Usage: python tests/clip_dp_worker.py <outdir> <global_batch>   (RANK / WORLD_SIZE / MASTER_* from the env)"""
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch


def run(outdir, Bg):
    import numpy as np
    from tests.golden import cases
    from tests.test_gpu_joint import _build_joint
    from unirec_amd import dp
    from unirec_amd.joint import JointTrainer
    rank, world, _ = dp.init_from_env()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    case = dict(cases.ALL["joint_left"], B=Bg, drop_one_special=False)
    m, qf = _build_joint(case, use_lora=True, lora_seed=case["seed"] + 2)
    m.base_model.config.lora_dropout = 0.1
    qf.qformer.config.hidden_dropout_prob = 0.1
    qf.qformer.config.attention_probs_dropout_prob = 0.1
    max_grad_norm = 1e-3          # far under the gradient's norm: the clip bites
    args = types.SimpleNamespace(learning_rate=1e-4, max_grad_norm=max_grad_norm, lr_scheduler_type="constant", weight_decay=0.01,
                                 logging_steps=1)
    tr = JointTrainer(m, args, num_training_steps=1)
    ids, am, hfe, ham, pos, neg, nmask = cases.joint_inputs(case)
    lo, hi = dp.shard_range(Bg, rank, world)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[lo:hi])).to(dev)
    batch = {"input_ids": t(ids), "attention_mask": t(am), "history_field_embeddings": t(hfe), "history_attention_mask": t(ham),
             "positive_item_embeddings": t(pos), "negative_item_embeddings": t(neg), "negative_masks": t(nmask)}
    tr.training_step(batch)
    torch.cuda.synchronize()
    names = {"qformer": tr.qpack, "lora": tr.lpack}
    out = {"master": {k: p.master.cpu() for k, p in names.items()},
           "exp_avg": {k: tr.optimizer.state[tr.packs.index(p)][0].cpu() for k, p in names.items()},
           "grad_norm": tr.state.log_history[-1]["grad_norm"], "max_grad_norm": max_grad_norm, "n": hi - lo, "world": world}
    torch.save(out, os.path.join(outdir, f"rank{rank}.pt"))
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    run(sys.argv[1], int(sys.argv[2]))

"""CPU: the host side of the joint step's gradient clipping and schedule -- argument checks of ur_grad_norm_clip /
ur_adamw_step_dev (they precede any launch), the schedules against transformers.get_scheduler, the TrainingArguments ->
JointTrainer mapping, HF's weight-decay rule on the packs, the live-span builder, and loading a state saved before clipping."""
import types

import pytest
import torch

from unirec_amd import _lib

# fake device addresses: every call below fails a host-side check before it could launch
P, MIS = 1 << 20, (1 << 20) + 4


def _ranges(*pairs):
    arr = (_lib.F32Range * max(1, len(pairs)))()
    for i, (p, n) in enumerate(pairs):
        arr[i].ptr, arr[i].n = p, n
    return arr


def _err():
    return _lib.load().ur_last_error()


def test_grad_norm_clip_rejects_bad_arguments():
    lib = _lib.load()
    ok = _ranges((P, 100))
    assert lib.ur_grad_norm_clip(ok, -1, P, 1, 1.0, 1.0, P, P + 4, None) < 0 and b"n_ranges" in _err()
    assert lib.ur_grad_norm_clip(ok, (1 << 20) + 1, P, 1, 1.0, 1.0, P, P + 4, None) < 0 and b"n_ranges" in _err()
    assert lib.ur_grad_norm_clip(None, 2, P, 1, 1.0, 1.0, P, P + 4, None) < 0 and b"null ranges" in _err()
    assert lib.ur_grad_norm_clip(ok, 1, P, 1, 1.0, 0.0, P, P + 4, None) < 0 and b"max_norm" in _err()
    assert lib.ur_grad_norm_clip(ok, 1, P, 1, 1.0, -1.0, P, P + 4, None) < 0 and b"max_norm" in _err()
    assert lib.ur_grad_norm_clip(ok, 1, P, 1, 1.0, float("nan"), P, P + 4, None) < 0 and b"max_norm" in _err()
    assert lib.ur_grad_norm_clip(ok, 1, P, 1, 1.0, 1.0, None, P + 4, None) < 0 and b"out_norm" in _err()
    assert lib.ur_grad_norm_clip(ok, 1, P, 1, 1.0, 1.0, P, P + 2, None) < 0 and b"misaligned" in _err()
    assert lib.ur_grad_norm_clip(_ranges((MIS, 100)), 1, P, 1, 1.0, 1.0, P, P + 4, None) < 0 and b"range 0" in _err()
    assert lib.ur_grad_norm_clip(_ranges((P, 8), (None, 8)), 2, P, 2, 1.0, 1.0, P, P + 4, None) < 0 and b"range 1" in _err()
    assert lib.ur_grad_norm_clip(_ranges((P, -1)), 1, P, 1, 1.0, 1.0, P, P + 4, None) < 0 and b"negative" in _err()
    # partial slots: ceil(n / UR_NORM_BLOCK_ELEMS) per range
    big = _ranges((P, _lib.NORM_BLOCK_ELEMS + 1), (P, 3))
    assert lib.ur_grad_norm_clip(big, 2, P, 2, 1.0, 1.0, P, P + 4, None) < 0 and b"need 3" in _err()
    assert lib.ur_grad_norm_clip(big, 2, None, 3, 1.0, 1.0, P, P + 4, None) < 0 and b"partials" in _err()


def test_adamw_step_dev_rejects_bad_arguments():
    lib = _lib.load()
    args = lambda param=P, coef=P, step=1, n=64: (param, P, P, P, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, step, 1.0, coef, None)
    assert lib.ur_adamw_step_dev(*args(coef=None)) < 0 and b"coef" in _err()
    assert lib.ur_adamw_step_dev(*args(coef=P + 2)) < 0 and b"coef" in _err()
    assert lib.ur_adamw_step_dev(*args(param=MIS)) < 0 and b"misaligned" in _err()
    assert lib.ur_adamw_step_dev(*args(step=0)) < 0 and b"step >= 1" in _err()
    assert lib.ur_adamw_step_dev(*args(n=-4)) < 0 and b"n >= 0" in _err()
    assert lib.ur_adamw_step_dev(*args(param=None)) < 0 and b"null" in _err()


@pytest.mark.parametrize("name,warmup,total", [("linear", 3, 6), ("linear", 20, 100), ("linear", 0, 7), ("cosine", 3, 11),
                                               ("cosine", 0, 9), ("constant", 0, 5), ("constant", 4, 5),
                                               ("constant_with_warmup", 3, 8), ("constant_with_warmup", 0, 4)])
def test_schedules_equal_transformers(name, warmup, total):
    from transformers import get_scheduler as hf_get_scheduler
    from unirec_amd.optim import get_scheduler
    p = torch.nn.Parameter(torch.zeros(1))
    topt = torch.optim.AdamW([p], lr=1e-4)
    hf = hf_get_scheduler(name, topt, num_warmup_steps=warmup, num_training_steps=total)
    opt = types.SimpleNamespace(lr=1e-4)
    ours = get_scheduler(name, opt, num_warmup_steps=warmup, num_training_steps=total)
    for step in range(total + 3):
        assert ours.get_last_lr() == hf.get_last_lr(), (step, ours.get_last_lr(), hf.get_last_lr())
        assert opt.lr == topt.param_groups[0]["lr"], step
        topt.step()                     # (no gradient: a no-op that keeps torch's scheduler-order warning away)
        hf.step()
        ours.step()
    # resume: a fresh schedule loaded from the state continues where the first one is
    opt2 = types.SimpleNamespace(lr=1e-4)
    again = get_scheduler(name, opt2, num_warmup_steps=warmup, num_training_steps=total)
    again.load_state_dict(ours.state_dict())
    assert again.get_last_lr() == ours.get_last_lr() and opt2.lr == opt.lr


def test_linear_warmup_matches_the_documented_values():
    from unirec_amd.optim import get_scheduler
    opt = types.SimpleNamespace(lr=1e-4)
    s = get_scheduler("linear", opt, num_warmup_steps=3, num_training_steps=6)
    seen = []
    for _ in range(7):
        seen.append(opt.lr)
        s.step()
    assert seen[0] == 0.0 and seen[3] == 1e-4 and seen[6] == 0.0
    assert seen == pytest.approx([0, 1e-4 / 3, 2e-4 / 3, 1e-4, 2e-4 / 3, 1e-4 / 3, 0], abs=1e-12)


def _tiny_joint():
    from unirec_amd.joint import MultiModalQwenEmbedding
    from unirec_amd.qformer_utils import QFormerForItemRepresentation
    from unirec_amd.qwen3 import Qwen3Config
    torch.manual_seed(0)
    qf = QFormerForItemRepresentation(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512,
                                      num_query_tokens=2, field_embedding_dim=256, num_fields=4)
    cfg = Qwen3Config(vocab_size=100, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, head_dim=64)
    return MultiModalQwenEmbedding(qformer_model=qf, qwen_config=cfg, num_history_items=2, num_query_tokens_per_item=2)


def test_training_arguments_map_onto_the_joint_trainer(tmp_path):
    from transformers import TrainingArguments
    from unirec_amd.joint import JointTrainer, TrainingConfig
    m = _tiny_joint()
    # the reference's main() (training/train_item_individual_token_joint.py:755-773; fp16 has no meaning on the HIP path)
    ref = TrainingArguments(output_dir=str(tmp_path), per_device_train_batch_size=16, gradient_accumulation_steps=1, num_train_epochs=500,
                            learning_rate=1e-4, logging_steps=10, warmup_steps=20, max_grad_norm=1.0, report_to=[])
    tr = JointTrainer(m, ref, num_training_steps=1000)
    c = tr.config
    assert (c.learning_rate, c.betas, c.eps, c.weight_decay, c.max_grad_norm) == (1e-4, (0.9, 0.999), 1e-8, 0.0, 1.0)
    assert (c.lr_scheduler_type, c.warmup_steps, c.num_training_steps, c.logging_steps) == ("linear", 20, 1000, 10)
    opt = tr.optimizer
    assert opt.max_grad_norm == 1.0 and opt.weight_decay == 0.0 and opt.no_decay == frozenset() and opt.lr == 0.0   # HF: lr * 0 / 20
    assert [p for p in tr.packs] == [m.qformer_model.pack, m.base_model.pack]
    assert tr.lr_scheduler.num_warmup_steps == 20 and tr.lr_scheduler.base_lr == 1e-4
    # TrainingArguments defaults; max_steps wins over num_training_steps; a warm-up ratio; clipping off with max_grad_norm <= 0
    d = TrainingArguments(output_dir=str(tmp_path), report_to=[])
    c = TrainingConfig(d, num_training_steps=40)
    assert (c.learning_rate, c.betas, c.eps, c.weight_decay) == (d.learning_rate, (d.adam_beta1, d.adam_beta2), d.adam_epsilon, d.weight_decay)
    assert (c.max_grad_norm, c.lr_scheduler_type, c.warmup_steps, c.num_training_steps, c.logging_steps) == (1.0, "linear", 0, 40, 500)
    c = TrainingConfig(TrainingArguments(output_dir=str(tmp_path), max_steps=50, warmup_steps=0.1, max_grad_norm=0.0,
                                         lr_scheduler_type="cosine", weight_decay=0.01, report_to=[]), num_training_steps=999)
    assert (c.num_training_steps, c.warmup_steps, c.max_grad_norm, c.lr_scheduler_type, c.weight_decay) == (50, 5, None, "cosine", 0.01)
    # any object with TrainingArguments' attribute names
    c = TrainingConfig(types.SimpleNamespace(learning_rate=3e-4, warmup_steps=2, max_grad_norm=0.5, lr_scheduler_type="constant_with_warmup"))
    assert (c.learning_rate, c.warmup_steps, c.max_grad_norm, c.lr_scheduler_type, c.num_training_steps) == (3e-4, 2, 0.5, "constant_with_warmup", None)
    with pytest.raises(ValueError, match="gradient_accumulation_steps"):
        TrainingConfig(TrainingArguments(output_dir=str(tmp_path), gradient_accumulation_steps=4, report_to=[]), num_training_steps=10)


def test_no_decay_names_follow_hf_trainer(tmp_path):
    from transformers import Trainer, TrainingArguments
    from unirec_amd.joint import JointTrainer
    m = _tiny_joint()
    tr = JointTrainer(m, TrainingArguments(output_dir=str(tmp_path), weight_decay=0.01, report_to=[]), num_training_steps=10)
    decay = set(Trainer.get_decay_parameter_names(None, m))
    model_name = {id(p): n for n, p in m.named_parameters()}
    checked = 0
    for pack in tr.packs:
        for n in pack.names:
            assert (n in tr.no_decay) == (model_name[id(pack.params[n])] not in decay), n
            checked += 1
    assert checked > 0 and tr.no_decay and tr.optimizer.no_decay == frozenset(tr.no_decay)
    assert any(n.endswith("LayerNorm.weight") for n in tr.no_decay) and not any(".lora_" in n for n in tr.no_decay)


def _cpu_pack():
    from unirec_amd.packing import ParamPack
    sizes = [("a", (8,)), ("b", (2, 8)), ("c", (3,)), ("d", (16,)), ("e", (5,)), ("f", (8,))]
    named = [(n, torch.nn.Parameter(torch.randn(*s))) for n, s in sizes]
    return ParamPack(named, "cpu")


def test_live_spans_merge_adjacent_tensors_and_drop_stale_ones():
    from unirec_amd.optim import FusedAdamW
    pk = _cpu_pack()
    # offsets: a 0..8, b 8..24, c 24..27 (padded to 32), d 32..48, e 48..53 (padded to 56), f 56..64
    pk.publish_grads(["a", "b", "c", "d", "f"])
    assert pk.live_spans() == [(0, 27), (32, 48), (56, 64)]
    opt = FusedAdamW([pk], max_grad_norm=1.0)
    pk.params["d"].grad = None                     # reset by someone else: torch.optim.AdamW would not step it
    assert opt.grad_spans() == [(0, 0, 27), (0, 56, 64)]
    assert "d" not in pk.live
    pk.publish_grads(["e"])
    assert opt.grad_spans() == [(0, 0, 27), (0, 48, 53), (0, 56, 64)]


def test_state_dict_round_trip_and_a_state_saved_before_clipping_loads():
    from unirec_amd.optim import FusedAdamW
    pk = _cpu_pack()
    opt = FusedAdamW([pk], lr=1e-3, weight_decay=0.01, max_grad_norm=0.5, no_decay=["c", "e"])
    opt.state[0][0].fill_(0.25)
    sd = opt.state_dict()
    assert sd["max_grad_norm"] == 0.5 and sd["no_decay"] == ["c", "e"]
    old = {k: v for k, v in sd.items() if k not in ("max_grad_norm", "no_decay")}       # what the optimizer saved before
    fresh = FusedAdamW([pk], max_grad_norm=2.0, no_decay=["a"])
    fresh.load_state_dict(old)
    assert fresh.max_grad_norm == 2.0 and fresh.no_decay == frozenset(["a"]) and fresh.lr == 1e-3
    assert torch.equal(fresh.state[0][0], opt.state[0][0])
    fresh.load_state_dict(sd)
    assert fresh.max_grad_norm == 0.5 and fresh.no_decay == frozenset(["c", "e"])
    with pytest.raises(ValueError):
        FusedAdamW([pk], max_grad_norm=0.0)
    assert FusedAdamW([pk]).last_grad_norm is None

"""CPU: what the host decides about the LoRA rank -- the supported set at construction, the shapes the adapters and their peft
export take, and the rank-dependent launch rule of Qwen3LoRAModel._plan (a pure function of rank and switches)."""
from types import SimpleNamespace

import pytest


def _tiny(**kw):
    from unirec_amd.qwen3 import Qwen3Config
    return Qwen3Config(vocab_size=64, hidden_size=64, intermediate_size=96, num_hidden_layers=2, num_attention_heads=2,
                       num_key_value_heads=1, head_dim=32, **kw)


@pytest.mark.parametrize("r", [12, 128, 4, 24])
def test_unsupported_rank_fails_at_construction(r):
    from unirec_amd.qwen3 import Qwen3LoRAModel
    with pytest.raises(ValueError, match="8, 16, 32, 64"):
        Qwen3LoRAModel(_tiny(lora_r=r))
    Qwen3LoRAModel(_tiny(lora_r=r), use_lora=False)          # no adapters: the rank is not looked at


@pytest.mark.parametrize("r", [8, 16, 32, 64])
def test_supported_ranks_build_with_peft_shapes(r):
    from unirec_amd.joint import MultiModalQwenEmbedding
    m = MultiModalQwenEmbedding(lora_config={"r": r, "lora_alpha": 2 * r, "lora_dropout": 0.1}, qwen_config=_tiny(),
                                num_history_items=2, num_query_tokens_per_item=2)
    c = m.base_model.config
    assert (c.lora_r, c.lora_alpha, c.lora_dropout) == (r, 2 * r, 0.1)
    sd = m.base_model.peft_state_dict()
    assert len(sd) == 2 * 7 * 2
    dims = {"self_attn.q_proj": (64, 64), "self_attn.k_proj": (32, 64), "self_attn.v_proj": (32, 64), "self_attn.o_proj": (64, 64),
            "mlp.gate_proj": (96, 64), "mlp.up_proj": (96, 64), "mlp.down_proj": (64, 96)}
    for i in range(2):
        for proj, (out, inp) in dims.items():
            assert tuple(sd[f"base_model.model.layers.{i}.{proj}.lora_A.weight"].shape) == (r, inp)
            assert tuple(sd[f"base_model.model.layers.{i}.{proj}.lora_B.weight"].shape) == (out, r)
    # the trainable set and the parameter pack's order follow from the shapes alone
    names = [n for n, _ in m.base_model.lora_named_parameters()]
    assert len(names) == len(sd) and all(("base_model.model." + n) in sd for n in names)


def test_rank_rule_table():
    """merged: the merged q|k|v launch's second K range (3 r) fits the persistent GEMM's one K tile of 64; the fused norm / SwiGLU +
    adapter kernels and the token-packed flags (ring kernel of the token reduction) are rank 16."""
    from unirec_amd.qwen3 import PERS_GEMM_K2_MAX, lora_rank_rule
    from unirec_amd.switches import Switches
    assert PERS_GEMM_K2_MAX == 64
    on = Switches()
    assert lora_rank_rule(8, on) == {"merged": True, "fuse_norm": False, "swiglu_lora": False, "bits_t": False}
    assert lora_rank_rule(16, on) == {"merged": True, "fuse_norm": True, "swiglu_lora": True, "bits_t": True}
    assert lora_rank_rule(32, on) == {"merged": False, "fuse_norm": False, "swiglu_lora": False, "bits_t": False}
    assert lora_rank_rule(64, on) == {"merged": False, "fuse_norm": False, "swiglu_lora": False, "bits_t": False}
    # a pure function of (rank, switches): any object with the four fields will do, and a switch that is off stays off at rank 16
    off = SimpleNamespace(merge_proj=False, fuse_norm_lora=False, fuse_swiglu_lora=False, bits_t=False)
    for r in (8, 16, 32, 64):
        assert lora_rank_rule(r, off) == {"merged": False, "fuse_norm": False, "swiglu_lora": False, "bits_t": False}
    one = SimpleNamespace(merge_proj=True, fuse_norm_lora=False, fuse_swiglu_lora=True, bits_t=False)
    assert lora_rank_rule(16, one) == {"merged": True, "fuse_norm": False, "swiglu_lora": True, "bits_t": False}


def test_wrappers_refuse_other_ranks_before_any_launch():
    """hip.lora_project / lora_bgrad read the rank from the operands and name the supported set (no device needed to get there)"""
    from unirec_amd import hip
    assert hip.LORA_RANKS == (8, 16, 32, 64)
    with pytest.raises(ValueError, match="8, 16, 32, 64"):
        hip._lora_rank(12, "test")
    assert [hip._lora_rank(r, "test") for r in hip.LORA_RANKS] == [8, 16, 32, 64]

"""CPU: what the host decides about the LoRA placement -- how a peft.LoraConfig-like object or dict is read (every field honoured or
refused by name), the parameters a placement builds and exports, adapter_config.json, the rank-stabilised scale, and the data-parallel
bucket layout over a pack in which some layers own nothing."""
import json
from types import SimpleNamespace

import pytest
import torch

ALL7 = ["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"]
DIMS = {"self_attn.q_proj": (64, 64), "self_attn.k_proj": (32, 64), "self_attn.v_proj": (32, 64), "self_attn.o_proj": (64, 64),
        "mlp.gate_proj": (96, 64), "mlp.up_proj": (96, 64), "mlp.down_proj": (64, 96)}


def _tiny(**kw):
    """the tiny config of tests/test_lora_ranks_host.py"""
    from unirec_amd.qwen3 import Qwen3Config
    return Qwen3Config(vocab_size=64, hidden_size=64, intermediate_size=96, num_hidden_layers=2, num_attention_heads=2,
                       num_key_value_heads=1, head_dim=32, **kw)


def _both(d):
    """a config as a dict and as an object with attributes"""
    return [d, SimpleNamespace(**d)]


def _model(lora_config, **kw):
    from unirec_amd.joint import MultiModalQwenEmbedding
    return MultiModalQwenEmbedding(lora_config=lora_config, qwen_config=_tiny(**kw), num_history_items=2, num_query_tokens_per_item=2)


# ---- parsing ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec,want", [(["q_proj", "v_proj"], ["q_proj", "v_proj"]), (("v_proj", "q_proj"), ["q_proj", "v_proj"]),
                                       ({"k_proj"}, ["k_proj"]), (["self_attn.q_proj", "mlp.up_proj"], ["q_proj", "up_proj"]),
                                       ("all-linear", ALL7), (None, None), (list(reversed(ALL7)), ALL7)])
def test_target_modules_are_read(spec, want):
    for lc in _both({"r": 16, "target_modules": spec}):
        m = _model(lc)
        assert m.base_model.config.lora_target_modules == want
        short = ALL7 if want is None else want
        assert all(tuple(p.rsplit(".", 1)[-1] for p in mods) == tuple(short) for mods in m.base_model.adapter_modules)


@pytest.mark.parametrize("spec,match", [("q_proj", "regular expression"), (".*_proj", "regular expression"), (["q_proj", "lm_head"], "lm_head"),
                                        (["attn.q_proj"], "attn.q_proj"), ([], "empty"), (set(), "empty"), (7, "target_modules")])
def test_target_modules_are_refused(spec, match):
    for lc in _both({"target_modules": spec}):
        with pytest.raises(ValueError, match=match):
            _model(lc)


@pytest.mark.parametrize("spec,want", [(1, [1]), ([1], [1]), ([1, 0], [0, 1]), ((0,), [0]), (None, None)])
def test_layers_to_transform_are_read(spec, want):
    for lc in _both({"target_modules": ["q_proj"], "layers_to_transform": spec}):
        m = _model(lc)
        assert m.base_model.config.lora_layers_to_transform == want
        on = range(2) if want is None else want
        assert [bool(mods) for mods in m.base_model.adapter_modules] == [i in on for i in range(2)]


@pytest.mark.parametrize("spec", [2, -1, [0, 2], [0.0], "1", [], True])
def test_layers_to_transform_out_of_range_is_refused(spec):
    for lc in _both({"layers_to_transform": spec}):
        with pytest.raises(ValueError, match="layers_to_transform"):
            _model(lc)


@pytest.mark.parametrize("field,bad,inert", [("rank_pattern", {"q_proj": 8}, [{}, None]), ("alpha_pattern", {"q_proj": 4.0}, [{}, None]),
                                             ("bias", "all", ["none"]), ("bias", "lora_only", ["none"]), ("use_dora", True, [False]),
                                             ("fan_in_fan_out", True, [False]), ("modules_to_save", ["norm"], [None, []]),
                                             ("layers_pattern", "layers", [None, [], ""]), ("exclude_modules", ["o_proj"], [None, [], set()])])
def test_fields_without_an_implementation_are_refused_by_name(field, bad, inert):
    for lc in _both({"r": 8, field: bad}):
        with pytest.raises(ValueError, match=field):
            _model(lc)
    for v in inert:
        for lc in _both({"r": 8, field: v}):
            assert _model(lc).base_model.config.lora_r == 8
    assert _model({"r": 8}).base_model.config.lora_r == 8            # an absent field is never an error


def test_a_full_peft_style_config_with_inert_values_is_accepted():
    lc = SimpleNamespace(r=8, lora_alpha=16, lora_dropout=0.05, target_modules={"q_proj", "v_proj"}, layers_to_transform=None, use_rslora=False,
                         rank_pattern={}, alpha_pattern={}, bias="none", use_dora=False, fan_in_fan_out=False, modules_to_save=None,
                         layers_pattern=None, exclude_modules=None, task_type="FEATURE_EXTRACTION", inference_mode=False, init_lora_weights=True)
    c = _model(lc).base_model.config
    assert (c.lora_r, c.lora_alpha, c.lora_dropout, c.lora_target_modules, c.lora_layers_to_transform, c.use_rslora) == (8, 16, 0.05, ["q_proj", "v_proj"], None, False)


# ---- what a placement builds -----------------------------------------------------------------------------------------------------
def test_q_and_v_build_peft_trainable_set():
    for lc in _both({"r": 16, "lora_alpha": 32, "target_modules": ["q_proj", "v_proj"]}):
        m = _model(lc).base_model
        sd = m.peft_state_dict()
        assert len(sd) == 2 * 2 * 2
        for i in range(2):
            for proj in ("self_attn.q_proj", "self_attn.v_proj"):
                out, inp = DIMS[proj]
                assert tuple(sd[f"base_model.model.layers.{i}.{proj}.lora_A.weight"].shape) == (16, inp)
                assert tuple(sd[f"base_model.model.layers.{i}.{proj}.lora_B.weight"].shape) == (out, 16)
        names = [n for n, _ in m.lora_named_parameters()]
        assert sorted("base_model.model." + n for n in names) == sorted(sd)
        assert sorted(n for n in m.state_dict() if ".lora_" in n) == sorted(names)
        assert m.adapter_modules == (("self_attn.q_proj", "self_attn.v_proj"),) * 2
        assert not hasattr(m.layers[0].self_attn.k_proj, "lora_A") and hasattr(m.layers[0].self_attn.q_proj, "lora_A")


def test_layers_to_transform_builds_that_layer_only():
    m = _model({"r": 16, "target_modules": ["q_proj", "v_proj"], "layers_to_transform": [1]}).base_model
    sd = m.peft_state_dict()
    assert len(sd) == 4 and all(k.startswith("base_model.model.layers.1.") for k in sd)
    assert m.adapter_modules == ((), ("self_attn.q_proj", "self_attn.v_proj"))


def test_explicit_seven_is_the_default_layout():
    """same parameter names, pack order and offsets as lora_config=None"""
    from unirec_amd.packing import ParamPack
    a, b = _model(None).base_model, _model({"target_modules": list(ALL7)}).base_model
    na, nb = [n for n, _ in a.lora_named_parameters()], [n for n, _ in b.lora_named_parameters()]
    assert na == nb and len(na) == 2 * 7 * 2
    assert list(a.state_dict()) == list(b.state_dict())
    pa, pb = ParamPack(a.lora_named_parameters(), "cpu"), ParamPack(b.lora_named_parameters(), "cpu")
    assert pa.names == pb.names and pa.offsets == pb.offsets and pa.numel == pb.numel
    assert a.adapter_modules == b.adapter_modules == (tuple(DIMS),) * 2
    assert a._place == b._place and all(pl.view is None for layer in a._place for pl in layer)


def test_plane_views_are_the_modules_slots():
    """the present adapters' planes inside the group's generator stream: q+v = planes 0 and 2 (stride 2), k alone = plane 1, up = plane 1"""
    m = _model({"target_modules": ["q_proj", "v_proj", "up_proj"]}).base_model
    qkv, o, gu, d = m._place[0]
    assert (qkv.planes, qkv.view, qkv.cols) == (3, slice(0, 3, 2), ((0, 64), (96, 32)))
    assert (gu.planes, gu.view, gu.cols) == (2, slice(1, 2, 1), ((96, 96),))
    assert (o.planes, d.planes) == (0, 0)
    k = _model({"target_modules": ["k_proj"]}).base_model._place[1][0]
    assert (k.planes, k.view, k.cols) == (2, slice(1, 2, 1), ((64, 32),))
    qk = _model({"target_modules": ["q_proj", "k_proj"]}).base_model._place[0][0]
    assert (qk.planes, qk.view) == (2, None)


def test_rank_rule_with_an_adapter_count():
    from unirec_amd.qwen3 import lora_rank_rule
    from unirec_amd.switches import Switches
    on = Switches()
    assert lora_rank_rule(32, on)["merged"] is False and lora_rank_rule(32, on, 3)["merged"] is False
    assert lora_rank_rule(32, on, 2)["merged"] is True               # rank 32 on q and v: 64 <= 64
    assert lora_rank_rule(64, on, 1)["merged"] is True and lora_rank_rule(64, on, 2)["merged"] is False
    assert lora_rank_rule(64, on, 0)["merged"] is True               # no adapter in q|k|v or gate|up at all
    assert lora_rank_rule(16, on, 1) == lora_rank_rule(16, on)


def test_rslora_scale():
    for r in (8, 16, 64):
        plain = _model({"r": r, "lora_alpha": 32.0}).base_model
        rs = _model({"r": r, "lora_alpha": 32.0, "use_rslora": True}).base_model
        assert plain._lora_scale() == 32.0 / r and plain.config.use_rslora is False
        assert rs._lora_scale() == 32.0 / r ** 0.5 and rs.config.use_rslora is True


def test_adapter_config_round_trip(tmp_path):
    from unirec_amd.joint import MultiModalQwenEmbedding, apply_lora_config
    lc = {"r": 8, "lora_alpha": 24, "lora_dropout": 0.05, "target_modules": ["v_proj", "q_proj"], "layers_to_transform": [1], "use_rslora": True}
    qf = torch.nn.Linear(2, 2)                      # stands in for the Q-Former: save_pretrained stores its state_dict
    qf.config = SimpleNamespace(hidden_size=64)
    m = MultiModalQwenEmbedding(base_model_name="Qwen/Qwen3-Embedding-0.6B", lora_config=lc, qwen_config=_tiny(), num_history_items=2,
                                num_query_tokens_per_item=2, qformer_model=qf)
    m.save_pretrained(str(tmp_path))
    with open(tmp_path / "adapter_config.json") as f:
        saved = json.load(f)
    assert saved == {"peft_type": "LORA", "task_type": "FEATURE_EXTRACTION", "base_model_name_or_path": "Qwen/Qwen3-Embedding-0.6B", "r": 8,
                     "lora_alpha": 24, "lora_dropout": 0.05, "target_modules": ["q_proj", "v_proj"], "layers_to_transform": [1],
                     "use_rslora": True, "bias": "none", "inference_mode": True}
    # the file read back as a lora_config builds the same placement, and adapter_model.bin holds exactly its tensors
    back = apply_lora_config(_tiny(), saved)
    c = m.base_model.config
    assert (back.lora_r, back.lora_alpha, back.lora_dropout, back.lora_target_modules, back.lora_layers_to_transform, back.use_rslora) == \
        (c.lora_r, c.lora_alpha, c.lora_dropout, c.lora_target_modules, c.lora_layers_to_transform, c.use_rslora)
    again = _model(saved).base_model
    assert again.adapter_modules == m.base_model.adapter_modules
    sd = torch.load(tmp_path / "adapter_model.bin")
    assert sorted(sd) == sorted(again.peft_state_dict())


# ---- data-parallel buckets over a pack with adapter-free layers --------------------------------------------------------------------
class _StubPack:
    """ParamPack's layout fields (tests/test_dp_gloo.py: _FakePack)"""

    def __init__(self, named_shapes):
        self.names, self.offsets, self.params = [], {}, {}
        off = 0
        for n, shp in named_shapes:
            self.names.append(n)
            self.offsets[n] = off
            self.params[n] = torch.zeros(shp)
            off += (self.params[n].numel() + 7) // 8 * 8
        self.numel = off


class _Rec:
    def __init__(self, bounds):
        self.bounds, self.sent, self.signalled = bounds, [], []

    def ready(self, i):
        self.sent.append((i, tuple(self.signalled)))


def _lora_pack(layers):
    shapes = []
    for i in layers:
        shapes += [(f"layers.{i}.q.lora_A", (16, 64)), (f"layers.{i}.q.lora_B", (64, 16))]      # 2048 elements per layer
    return _StubPack(shapes)


def _run_hook(pack, pre, grp):
    from unirec_amd import dp
    b = dp.layer_boundaries(pack, pre, grp)
    rec = _Rec(b)
    hook = dp.bucket_hook(pack, rec, pre, grp)
    for sig in reversed(range(len(pre))):            # Qwen3LoRAModel.backward: layers L-1 .. 0, nothing else
        rec.signalled.append(sig)
        hook(sig)
    return b, rec, hook


def _contract(pack, pre, b, rec):
    # every gradient element lies in exactly one bucket
    assert b[0] == 0 and b[-1] == pack.numel and all(lo < hi for lo, hi in zip(b, b[1:]))
    # every bucket is sent exactly once per backward
    assert sorted(i for i, _ in rec.sent) == list(range(len(b) - 1))
    # no bucket is sent before the last layer that writes into it has signalled
    for i, seen in rec.sent:
        writers = {k for k, p in enumerate(pre) for n in pack.names if n.startswith(p) and b[i] <= pack.offsets[n] < b[i + 1]}
        assert writers and writers <= set(seen), (i, writers, seen)


def test_buckets_with_adapter_free_layers():
    pre = [f"layers.{i}." for i in range(6)]
    pack = _lora_pack([1, 2, 4, 5])                  # layers 0 and 3 of 6 own nothing
    b, rec, hook = _run_hook(pack, pre, 2)
    assert b == [0, 2048, 4096, 8192]                # {1}, {2}, {4, 5}: a group's bucket starts at its lowest layer that owns anything
    assert [i for i, _ in rec.sent] == [2, 1, 0]
    assert [seen[-1] for _, seen in rec.sent] == [4, 2, 1]      # sent when the lowest adapted layer of the group signals
    assert hook.lead_by_layer and hook.first_of == {1: 0, 2: 1, 4: 2}
    _contract(pack, pre, b, rec)
    for grp in (1, 3, 7):
        b, rec, hook = _run_hook(pack, pre, grp)
        _contract(pack, pre, b, rec)
    assert _run_hook(pack, pre, 7)[0] == [0, 8192]
    assert _run_hook(pack, pre, 1)[0] == [0, 2048, 4096, 6144, 8192]
    # a whole group without adapters: no bucket for it, its signals are no-ops
    pack = _lora_pack([0, 1, 4])
    b, rec, hook = _run_hook(pack, pre, 2)
    assert b == [0, 4096, 6144] and [i for i, _ in rec.sent] == [1, 0] and [seen[-1] for _, seen in rec.sent] == [4, 0]
    _contract(pack, pre, b, rec)
    # only the top layer
    b, rec, hook = _run_hook(_lora_pack([5]), pre, 2)
    assert b == [0, 2048] and [(i, seen[-1]) for i, seen in rec.sent] == [(0, 5)]


def test_buckets_of_the_all_layers_pack_are_unchanged():
    """the layout and send order every earlier version produced for a pack in which each layer owns a range"""
    pre = [f"layers.{i}." for i in range(6)]
    pack = _lora_pack(range(6))
    b, rec, hook = _run_hook(pack, pre, 2)
    assert b == [0, 4096, 8192, 12288]
    assert [(i, seen[-1]) for i, seen in rec.sent] == [(2, 4), (1, 2), (0, 0)]
    assert hook.first_of == {0: 0, 2: 1, 4: 2} and hook.lead_by_layer and hook.hoisted_bucket is None
    _contract(pack, pre, b, rec)
    b, rec, hook = _run_hook(pack, pre, 4)
    assert b == [0, 8192, 12288] and [(i, seen[-1]) for i, seen in rec.sent] == [(1, 4), (0, 0)]
    b, rec, hook = _run_hook(pack, pre, 1)
    assert b == [0, 2048, 4096, 6144, 8192, 10240, 12288] and [i for i, _ in rec.sent] == [5, 4, 3, 2, 1, 0]

"""CPU: the host side of merged adapters -- the three rules include/unirec_hip_adapter.h is held to (declared <=> exported <=> bound, the
struct mirror in the header's field order, a float64 test named for every entry point through the COVERS dict of
tests/test_gpu_lora_merge.py), every refusal of ur_lora_merge through the raw library (fake non-null pointers: each call returns before
any launch), the float64 reference against torch, and the Python-level refusals and bookkeeping that need no device."""
import ast
import ctypes
import json
import os
import re

import pytest
import torch

from oracle import qwen3_ref as Q
from tests.lora_merge_ref import bf16_half_ulp, lora_merge_ref, merge_inputs
from unirec_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "unirec_hip_adapter.h")
GPU_TESTS = "tests/test_gpu_lora_merge.py"
FAKE = 1 << 20          # non-null, 16-byte aligned, never dereferenced on the host
MB = 1 << 24            # distance between the fake operands: no two of them overlap


# ---- the header: declared <=> exported <=> bound, struct mirror, a float64 test per entry point -------------------------------------
def _declared(header=HEADER):
    src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ur_[a-z0-9_]+)\s*\(", src)))


def test_adapter_header_symbols_are_bound_and_exported():
    names = _declared()
    assert names == ["ur_lora_merge"]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in unirec_hip_adapter.h but not exported by libunirec_hip.so"
        assert n in _lib.ADAPTER_SIGNATURES, f"{n} declared in unirec_hip_adapter.h but not bound in unirec_amd/_lib.py"
    assert not set(_lib.ADAPTER_SIGNATURES) - set(names), "bound but not declared in the adapter header"
    assert not set(_lib.ADAPTER_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.LOSS_SIGNATURES)), "a name belongs to one header"
    for other in ("unirec_hip.h", "unirec_hip_loss.h"):
        assert not set(names) & set(_declared(os.path.join(ROOT, "include", other))), f"{other} declares an adapter entry point"
    loaded = _lib.load()
    for n in names:
        assert getattr(loaded, n).argtypes == _lib.ADAPTER_SIGNATURES[n][1], f"load() did not bind {n}"
    assert _lib.ABI_VERSION >= 21 and loaded.ur_version() == _lib.ABI_VERSION      # (the adapter header arrived with ABI 21)


def test_struct_mirror_matches_the_header_field_order():
    body = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = body[body.index("typedef struct {") + len("typedef struct {"):body.index("} ur_lora_merge_t;")]
    fields = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in _lib.LoraMerge._fields_]


def test_every_adapter_entry_point_has_a_float64_test():
    with open(os.path.join(ROOT, GPU_TESTS)) as f:
        tree = ast.parse(f.read())
    covers = None
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "COVERS" for t in node.targets):
            covers = ast.literal_eval(node.value)
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    assert isinstance(covers, dict), f"{GPU_TESTS} has no top-level COVERS dict"
    assert sorted(covers) == _declared(), "COVERS lists exactly the entry points of unirec_hip_adapter.h"
    for entry, names in covers.items():
        assert names, f"COVERS[{entry!r}] names no test"
        for name in names:
            assert name in tests and "float64" in name, f"COVERS[{entry!r}] names {name}: no such float64 test"


# ---- ur_lora_merge: every refusal, without a GPU -------------------------------------------------------------------------------------
def _args(**over):
    a = _lib.LoraMerge()
    a.W, a.A, a.B, a.out_f32, a.out_bf16 = FAKE, FAKE + MB, FAKE + 2 * MB, FAKE + 3 * MB, FAKE + 4 * MB
    a.out_rows, a.in_cols, a.rank, a.scale = 64, 128, 16, 2.0
    a.ldw = a.ld_f32 = a.ld_bf16 = 128
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_invalid_arguments_are_rejected_without_a_gpu():
    lib = _lib.load()

    def rejected(word, **over):
        a = _args(**over)
        rc = lib.ur_lora_merge(ctypes.byref(a), None)
        msg = lib.ur_last_error()
        assert rc < 0 and b"ur_lora_merge" in msg and word in msg, (over, rc, msg)

    assert lib.ur_lora_merge(None, None) < 0 and b"ur_lora_merge" in lib.ur_last_error()
    for name in ("W", "A", "B"):
        rejected(b"null", **{name: None})
        rejected(b"aligned", **{name: FAKE + 5 * MB + 4})
    rejected(b"aligned", out_f32=FAKE + 3 * MB + 8)
    rejected(b"aligned", out_bf16=FAKE + 4 * MB + 2)
    for r in (0, 4, 12, 24, 128, -16):
        rejected(b"rank", rank=r)
    rejected(b"both outputs", out_f32=None, out_bf16=None)
    # out_bf16 on top of an input (W 64 x 128 f32 = 32 KiB, A 16 x 128 f32 = 8 KiB, B 64 x 16 f32 = 4 KiB): at its start, inside it, across its end
    for base, nbytes in ((FAKE, 64 * 128 * 4), (FAKE + MB, 16 * 128 * 4), (FAKE + 2 * MB, 64 * 16 * 4)):
        for at in (base, base + nbytes // 2, base + nbytes - 16, base - 64 * 128 * 2 + 16):
            rejected(b"out_bf16 aliases", out_bf16=at)
    rejected(b"out_bf16 aliases", out_bf16=FAKE + 3 * MB)                      # ... and on top of the other output
    rejected(b"out_f32", out_f32=FAKE + MB)                                   # out_f32 on A
    rejected(b"out_f32", out_f32=FAKE + 128 * 4)                              # out_f32 inside W without being W
    rejected(b"out_f32", out_f32=FAKE, ld_f32=256, ldw=128)                   # W's pointer under another row stride
    # sizes and strides
    rejected(b"multiples of 8", out_rows=60)
    rejected(b"multiples of 8", in_cols=100, ldw=104, ld_f32=104, ld_bf16=104)
    rejected(b"multiples of 8", out_rows=-8)
    rejected(b"ldw", ldw=120)
    rejected(b"ldw", ldw=130)
    rejected(b"ld_f32", ld_f32=64)
    rejected(b"ld_bf16", ld_bf16=132)
    # nothing to do: 0, nothing launched (and nothing written: there is no device here)
    for over in (dict(out_rows=0), dict(in_cols=0), dict(out_rows=0, W=None, out_f32=None, out_bf16=None)):
        assert lib.ur_lora_merge(ctypes.byref(_args(**over)), None) == 0


def test_wrapper_refuses_host_tensors_and_bad_shapes():
    from unirec_amd import hip
    W, A, B = torch.zeros(16, 24), torch.zeros(8, 24), torch.zeros(16, 8)
    with pytest.raises(_lib.UniRecHipError, match="no CPU fallback"):
        hip.lora_merge(W, A, B, 1.0)
    with pytest.raises(ValueError, match="W \\[out,in\\]"):
        hip.lora_merge(W, A, torch.zeros(8, 8), 1.0)


# ---- the float64 reference -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("O,I,r,scale", [(8, 8, 8, 2.0), (24, 40, 16, -0.5), (136, 264, 64, 8.0)])
def test_reference_matches_torch_float64(O, I, r, scale):
    W, A, B = merge_inputs(O, I, r, seed=O + r)
    assert float(A[1].abs().max()) == 0.0 and float(B[:, 2].abs().max()) == 0.0
    assert int((W == 0).sum()) > 0 or O * I < 100
    mags = torch.cat([t[t != 0].abs().flatten() for t in (W, A, B)])
    assert float(mags.min()) >= 2.0 ** -20.01 and float(mags.max()) <= 2.0 ** 8.01
    ref, b32, b16 = lora_merge_ref(W, A, B, scale)
    want = W.double() + scale * B.double() @ A.double()
    assert float((ref - want).abs().max()) <= 1e-13 * float(want.abs().max())
    assert ref.dtype == torch.float64 and bool((b32 >= 0).all()) and bool((b16 >= b32).all())
    # an f32 evaluation in the kernel's order sits inside the f32 bound, its bf16 rounding inside the bf16 bound
    acc = torch.zeros(O, I)
    for k in range(r):
        acc = torch.addcmul(acc, B[:, k:k + 1], A[k:k + 1, :])      # (mul + add: two roundings where the kernel has one; the bound still holds them at these sizes)
    got = W + scale * acc
    assert bool(((got.double() - ref).abs() <= 3 * b32 + 1e-300).all())
    assert bool(((got.bfloat16().double() - ref).abs() <= 3 * b32 + bf16_half_ulp(ref) * 1.01 + 1e-300).all())


def test_bf16_half_ulp():
    x = torch.tensor([0.0, 1.0, 1.5, 2.0, 255.0, 2.0 ** -130, -3.0], dtype=torch.float64)
    assert bf16_half_ulp(x).tolist() == [0.0, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -1, 2.0 ** -134, 2.0 ** -7]


# ---- Python-level refusals and bookkeeping that need no device ---------------------------------------------------------------------
class _QF(torch.nn.Module):
    """stands in for the item Q-Former: a config with the hidden size and a state dict"""

    def __init__(self, hidden):
        super().__init__()
        self.config = type("C", (), {"hidden_size": hidden})()
        self.w = torch.nn.Parameter(torch.arange(4.0))


def _cfg(**over):
    from unirec_amd.qwen3 import Qwen3Config
    kw = dict(vocab_size=120, hidden_size=256, intermediate_size=384, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
              head_dim=128, lora_r=16, lora_alpha=32.0, lora_dropout=0.1)
    kw.update(over)
    return Qwen3Config(**kw)


def _model(cfg=None, **kw):
    from unirec_amd.joint import HistoryTokenTable, MultiModalQwenEmbedding
    return MultiModalQwenEmbedding(qformer_model=_QF(256), qwen_config=cfg or _cfg(), num_history_items=4, num_query_tokens_per_item=2,
                                   tokenizer=HistoryTokenTable(120, 4, 2), **kw)


def test_from_pretrained_refuses_adapter_fields_by_name(tmp_path):
    from unirec_amd.joint import HistoryTokenTable, MultiModalQwenEmbedding
    m = _model(_cfg(lora_target_modules=["q_proj", "v_proj"]))
    m.save_pretrained(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["adapter_config.json", "adapter_model.bin", "history_tokens.json", "model_config.json", "qformer_model.bin"]
    kw = dict(qwen_config=_cfg(), num_history_items=4, num_query_tokens_per_item=2, tokenizer=HistoryTokenTable(120, 4, 2))
    back = MultiModalQwenEmbedding.from_pretrained(str(tmp_path), _QF(256), **kw)      # round trip on the host: placement and values
    assert back.base_model.adapter_modules == m.base_model.adapter_modules == (("self_attn.q_proj", "self_attn.v_proj"),) * 2
    for (n0, p0), (n1, p1) in zip(m.base_model.lora_named_parameters(), back.base_model.lora_named_parameters()):
        assert n0 == n1 and torch.equal(p0, p1)
    path = os.path.join(tmp_path, "adapter_config.json")
    good = json.load(open(path))
    for field, value in (("use_dora", True), ("rank_pattern", {"q_proj": 8}), ("bias", "all"), ("modules_to_save", ["norm"])):
        json.dump(dict(good, **{field: value}), open(path, "w"))
        with pytest.raises(ValueError, match=field):
            MultiModalQwenEmbedding.from_pretrained(str(tmp_path), _QF(256), **kw)
    json.dump(dict(good, target_modules=["q_proj", "lm_head"]), open(path, "w"))
    with pytest.raises(ValueError, match="lm_head"):
        MultiModalQwenEmbedding.from_pretrained(str(tmp_path), _QF(256), **kw)
    json.dump(good, open(path, "w"))
    # a tensor that does not fit the placement: named
    sd = torch.load(os.path.join(tmp_path, "adapter_model.bin"))
    extra = "base_model.model.layers.0.self_attn.k_proj.lora_A.weight"
    with pytest.raises(KeyError, match="k_proj.lora_A"):
        m.load_adapter(dict(sd, **{extra: torch.zeros(16, 256)}))
    some = next(iter(sd))
    with pytest.raises(KeyError, match="missing"):
        m.load_adapter({k: v for k, v in sd.items() if k != some})
    with pytest.raises(ValueError, match="shape"):
        m.load_adapter(dict(sd, **{some: torch.zeros(3, 3)}))
    # a directory whose adapters are not this model's
    with pytest.raises(ValueError, match="target_modules"):
        _model().load_adapter(str(tmp_path))
    assert m.load_adapter(str(tmp_path)) is m


def test_unload_leaves_the_hf_key_set(monkeypatch):
    """merge_and_unload with the kernel mocked (W + s B A by torch, on the host): the bookkeeping -- adapters gone, use_lora off, caches
    dropped, exactly the HF Qwen3Model keys -- and the values the in-place call is asked for."""
    from unirec_amd import hip
    calls = []

    def fake_merge(W, A, B, scale, out_f32=None, out_bf16=None):
        assert out_f32 is W and out_bf16 is None, "merge_and_unload merges in place on the f32 master"
        calls.append(tuple(W.shape))
        W.add_(scale * (B.double() @ A.double()).float())
        return W, None
    monkeypatch.setattr(hip, "lora_merge", fake_merge)
    cfg = _cfg(lora_target_modules=["q_proj", "down_proj"], lora_layers_to_transform=[1], use_rslora=True)
    m = _model(cfg)
    bm = m.base_model
    bm.reset_parameters(lora_b_std=0.05)
    before = {k: v.clone() for k, v in bm.state_dict().items()}
    bm._frozen = {"key": "stale"}
    assert m.merge_and_unload() is m and m.use_lora is False and bm.use_lora is False
    assert calls == [(256, 256), (256, 384)]
    assert bm._frozen is None and bm._pack is None and bm._merged is None and bm.adapter_modules == ((), ())
    after = bm.state_dict()
    qc = Q.Qwen3Cfg(hidden_size=256, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, head_dim=128, intermediate_size=384,
                    vocab_size=128)
    assert {k: tuple(v.shape) for k, v in after.items()} == Q.qwen3_shapes(qc, lora=False)
    s = 32.0 / 4.0          # rsLoRA: lora_alpha / sqrt(r)
    for k, v in after.items():
        a, b = (before.get(k.replace(".weight", f".lora_{x}.weight")) for x in "AB")
        want = before[k] if a is None else before[k] + s * (b.double() @ a.double()).float()
        assert torch.equal(v, want), k
    assert bm.merge_and_unload() is bm and len(calls) == 2                     # nothing left to merge
    bm.merge_adapter()                                                         # no adapters: nothing to do, on any device
    assert not bm.merged


def test_training_while_merged_is_refused_before_anything_runs(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded")
    m = _model()
    bm = m.base_model
    bm._merged = {"key": None, "fz": None, "bytes": 0}                         # (what merge_adapter() leaves behind)
    monkeypatch.setattr(_lib, "load", no_library)
    ids = torch.zeros(2, 8, dtype=torch.long)
    m.train()
    for call in (lambda: m(ids), lambda: bm.forward_pooled(ids)):
        with pytest.raises(RuntimeError, match="unmerge_adapter"):
            call()
    bm.prefetch_lora_bits(16, "cpu")                                          # a no-op while merged: no library, no device
    assert bm._bits_pre is None and bm._drop_p() == 0.0
    m.unmerge_adapter()
    assert not bm.merged and bm._drop_p() == pytest.approx(0.1)
    with bm.disable_adapter():
        assert bm._drop_p() == 0.0 and not bm._lora_live()
    assert bm._lora_live()


def test_hf_config_and_checkpoint_files(tmp_path):
    """the merged export's files from host tensors: transformers reads config.json back into the decoder's shape, and the safetensors
    file holds the keys and dtype asked for; an adapter tensor is refused by name"""
    from safetensors.torch import load_file
    from unirec_amd.joint import hf_qwen3_config_dict, write_hf_checkpoint
    cfg = _cfg(vocab_size=128)
    qc = Q.Qwen3Cfg(hidden_size=256, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, head_dim=128, intermediate_size=384,
                    vocab_size=128)
    sd = {k: torch.full(shp, 0.5) for k, shp in Q.qwen3_shapes(qc, lora=False).items()}
    write_hf_checkpoint(str(tmp_path), cfg, sd, torch.bfloat16)
    back = load_file(os.path.join(tmp_path, "model.safetensors"))
    assert sorted(back) == sorted(sd) and all(v.dtype == torch.bfloat16 for v in back.values())
    with pytest.raises(ValueError, match="lora_A"):
        write_hf_checkpoint(str(tmp_path), cfg, dict(sd, **{"layers.0.mlp.up_proj.lora_A.weight": torch.zeros(16, 256)}))
    import transformers
    hc = transformers.AutoConfig.from_pretrained(str(tmp_path), local_files_only=True)
    d = hf_qwen3_config_dict(cfg, torch.bfloat16)
    for k in ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "num_key_value_heads", "head_dim",
              "rms_norm_eps", "tie_word_embeddings"):
        assert getattr(hc, k) == d[k], k
    rope = getattr(hc, "rope_parameters", None) or {"rope_theta": getattr(hc, "rope_theta", None)}
    assert rope["rope_theta"] == cfg.rope_theta

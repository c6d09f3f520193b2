"""CPU: the host side of the pooling modes -- the rules include/unirec_hip_pool.h is held to (declared <=> exported <=> bound, a name in
one header only, a float64 test named for every entry point through the COVERS dict of tests/test_gpu_pool_f64.py; the family passes no
struct, so there is no mirror to check), every refusal of the three entry points through the raw library (fake non-null pointers: each
call returns before any launch), the float64 reference (tests/pool_ref.py) against autograd and against the fixture
tests/golden/pool_tiny.npz composed with the oracle's decoder, and the Python-level plumbing of the `pooling` field."""
import ast
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle import qwen3_ref as Q
from oracle import weights as W
from tests import pool_ref
from tests.golden import cases
from tests.test_oracle_golden import _close
from unirec_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "unirec_hip_pool.h")
GPU_TESTS = "tests/test_gpu_pool_f64.py"
FAKE = 1 << 20          # non-null, 16-byte aligned, never dereferenced on the host
MB = 1 << 24
MM, LAST = _lib.POOL_MASKED_MEAN, _lib.POOL_LAST


# ---- the header: declared <=> exported <=> bound, a float64 test per entry point -------------------------------------------------------
def _declared(header=HEADER):
    src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ur_[a-z0-9_]+)\s*\(", src)))


def test_pool_header_symbols_are_bound_and_exported():
    names = _declared()
    assert names == ["ur_pool_norm_bwd", "ur_pool_norm_fwd", "ur_pool_norm_workspace_bytes"]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in unirec_hip_pool.h but not exported by libunirec_hip.so"
        assert n in _lib.POOL_SIGNATURES, f"{n} declared in unirec_hip_pool.h but not bound in unirec_amd/_lib.py"
    assert not set(_lib.POOL_SIGNATURES) - set(names), "bound but not declared in the pooling header"
    others = set(_lib.SIGNATURES) | set(_lib.LOSS_SIGNATURES) | set(_lib.ADAPTER_SIGNATURES)
    assert not set(_lib.POOL_SIGNATURES) & others, "a name belongs to one header"
    for other in ("unirec_hip.h", "unirec_hip_loss.h", "unirec_hip_adapter.h"):
        assert not set(names) & set(_declared(os.path.join(ROOT, "include", other))), f"{other} declares a pooling entry point"
    loaded = _lib.load()
    for n in names:
        assert getattr(loaded, n).argtypes == _lib.POOL_SIGNATURES[n][1], f"load() did not bind {n}"
        assert getattr(loaded, n).restype == _lib.POOL_SIGNATURES[n][0]
    assert _lib.ABI_VERSION >= 22 and loaded.ur_version() == _lib.ABI_VERSION      # (the pooling header arrived with ABI 22)


def test_header_constants_match_the_binding():
    src = open(HEADER).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (UR_POOL_[A-Z_]+) (\d+)", src)}
    assert consts == {"UR_POOL_MASKED_MEAN": MM, "UR_POOL_LAST": LAST, "UR_POOL_NORM_SLICES": _lib.POOL_NORM_SLICES}
    assert pool_ref.SLICES == _lib.POOL_NORM_SLICES
    assert "typedef struct" not in src          # no struct crosses this family's ABI: nothing to mirror in ctypes


def test_every_pool_entry_point_has_a_float64_test():
    with open(os.path.join(ROOT, GPU_TESTS)) as f:
        tree = ast.parse(f.read())
    covers = None
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "COVERS" for t in node.targets):
            covers = ast.literal_eval(node.value)
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    assert isinstance(covers, dict), f"{GPU_TESTS} has no top-level COVERS dict"
    assert sorted(covers) == _declared(), "COVERS lists exactly the entry points of unirec_hip_pool.h"
    for entry, names in covers.items():
        assert names, f"COVERS[{entry!r}] names no test"
        for name in names:
            assert name in tests and "float64" in name, f"COVERS[{entry!r}] names {name}: no such float64 test"


# ---- every refusal, without a GPU -------------------------------------------------------------------------------------------------------
def _call(lib, which, **over):
    B, S, D, mode = (over.get(k, v) for k, v in (("B", 3), ("S", 40), ("D", 256), ("mode", MM)))
    a = dict(x=FAKE, w=FAKE + MB, mask=FAKE + 2 * MB + 1, out=FAKE + 3 * MB, g=FAKE + 4 * MB, ws=FAKE + 5 * MB, eps=1e-6,
             wsb=max(int(lib.ur_pool_norm_workspace_bytes(B, D, mode)), 0), B=B, S=S, D=D, mode=mode)
    a.update(over)
    if which == "fwd":
        return lib.ur_pool_norm_fwd(a["x"], a["w"], a["mask"], a["out"], a["B"], a["S"], a["D"], a["eps"], a["mode"], a["ws"], a["wsb"], None)
    return lib.ur_pool_norm_bwd(a["g"], a["x"], a["w"], a["mask"], a["out"], a["B"], a["S"], a["D"], a["eps"], a["mode"], a["ws"], a["wsb"], None)


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_invalid_arguments_are_rejected_without_a_gpu(which):
    lib = _lib.load()
    who = f"ur_pool_norm_{which}".encode()

    def rejected(word, **over):
        rc = _call(lib, which, **over)
        msg = lib.ur_last_error()
        assert rc < 0 and who in msg and word in msg, (over, rc, msg)

    for name in ("x", "w", "out") + (("g",) if which == "bwd" else ()):
        rejected(b"null", **{name: None})
        rejected(b"aligned", **{name: FAKE + 6 * MB + 8})
    rejected(b"D %", D=12)
    rejected(b"D %", D=2056)
    rejected(b"D %", D=0)
    rejected(b"S > 0", S=0)
    rejected(b"S > 0", S=-3)
    rejected(b"S > 0", B=-1)
    rejected(b"eps", eps=-1e-6)
    rejected(b"eps", eps=float("nan"))
    for mode in (0, 3, -1):
        rejected(b"mode", mode=mode)
    for mode in (MM, LAST):
        need = int(lib.ur_pool_norm_workspace_bytes(3, 256, mode))
        assert need == (3 * 16 * 257 * 4 if mode == MM else 3 * 4)
        rejected(b"workspace too small", mode=mode, wsb=need - 1)          # one byte short
        rejected(b"workspace", mode=mode, ws=None)
        rejected(b"workspace", mode=mode, ws=FAKE + 5 * MB + 4)
    # nothing to do: 0, nothing launched (and nothing written: there is no device here) -- even with no buffers at all
    assert _call(lib, which, B=0) == 0
    assert _call(lib, which, B=0, x=None, w=None, out=None, g=None, ws=None, wsb=0) == 0


def test_workspace_query_refuses_what_the_calls_refuse():
    lib = _lib.load()
    for B, D, mode in ((-1, 256, MM), (3, 12, MM), (3, 4096, LAST), (3, 256, 0), (3, 0, LAST)):
        assert lib.ur_pool_norm_workspace_bytes(B, D, mode) == -1 and b"ur_pool_norm_workspace_bytes" in lib.ur_last_error()
    assert lib.ur_pool_norm_workspace_bytes(0, 8, MM) == 0


def test_wrapper_refuses_host_tensors_and_bad_arguments():
    from unirec_amd import hip
    x, w = torch.zeros(2, 5, 16, dtype=torch.bfloat16), torch.ones(16)
    with pytest.raises(ValueError, match="mode"):
        hip.pool_norm_fwd(x, w, 1e-6, None, "mean")
    with pytest.raises(_lib.UniRecHipError, match="no CPU fallback"):
        hip.pool_norm_fwd(x, w, 1e-6, None, "last")
    with pytest.raises(_lib.UniRecHipError, match="no CPU fallback"):
        hip.pool_norm_bwd(torch.zeros(2, 16), x, w, 1e-6, None, "masked_mean")


# ---- the float64 reference --------------------------------------------------------------------------------------------------------------
def _masks(B, S):
    g = torch.Generator().manual_seed(B * 100 + S)
    holes = (torch.rand(B, S, generator=g) < 0.6).to(torch.uint8)
    holes[0] = 0                                     # an all-zero sample among valid ones
    if B > 1:
        holes[1, S // 2] = 1
    return {"none": None, "holes": holes}


@pytest.mark.parametrize("mode", pool_ref.MODES)
@pytest.mark.parametrize("B,S,D", [(1, 1, 8), (3, 7, 24), (2, 33, 40)])
def test_reference_matches_autograd(mode, B, S, D):
    g = torch.Generator().manual_seed(S)
    x = torch.randn(B, S, D, generator=g, dtype=torch.float64)
    w = torch.rand(D, generator=g, dtype=torch.float64) + 0.5
    dp = torch.randn(B, D, generator=g, dtype=torch.float64)
    for name, mask in _masks(B, S).items():
        c = pool_ref.pool_weights(mask, B, S, mode)
        valid = torch.ones(B, S, dtype=torch.bool) if mask is None else mask != 0
        assert bool(((c != 0) <= valid).all()) and torch.allclose(c.sum(1), valid.any(1).double())
        if mode == "last":
            for b in range(B):
                nz = valid[b].nonzero().flatten()
                assert c[b].nonzero().flatten().tolist() == ([int(nz[-1])] if len(nz) else [])
        xx = x.clone().requires_grad_(True)
        y = Q.rms_norm(xx, w, 1e-6)
        want = (y * c[..., None]).sum(1)
        (dx_want,) = torch.autograd.grad(want, xx, dp)
        pooled, T = pool_ref.pool_norm_fwd(x, w, 1e-6, mask, mode)
        assert torch.allclose(pooled, want, rtol=1e-12, atol=1e-14) and bool((T >= pooled.abs() - 1e-14).all())
        assert torch.allclose(pool_ref.pool(y.detach(), mask, mode), want, rtol=1e-12, atol=1e-14)
        assert torch.allclose(pool_ref.pool_norm_bwd(dp, x, w, 1e-6, mask, mode), dx_want, rtol=1e-10, atol=1e-13)
        # rows with c = 0 never enter a product: NaN / Inf there change nothing
        xn = x.clone()
        xn[(c == 0)] = float("nan")
        if (c == 0).any():
            b0, s0 = (c == 0).nonzero()[0].tolist()
            xn[b0, s0, 0] = float("inf")
        assert torch.equal(pool_ref.pool_norm_fwd(xn, w, 1e-6, mask, mode)[0], pooled)
        assert torch.equal(pool_ref.pool_norm_bwd(dp, xn, w, 1e-6, mask, mode), pool_ref.pool_norm_bwd(dp, x, w, 1e-6, mask, mode))
        if mask is not None:
            assert float(pooled[0].abs().max()) == 0.0 and float(pool_ref.pool_norm_bwd(dp, x, w, 1e-6, mask, mode)[0].abs().max()) == 0.0


def test_forward_ulp_count():
    """the count of tests/pool_ref.fwd_ulps at the shapes the GPU test runs, by hand"""
    assert [pool_ref.nch(D) for D in (8, 264, 512, 520, 1024, 1032, 2048)] == [1, 1, 1, 2, 2, 4, 4]
    assert pool_ref.fwd_ulps(1024, 2048, "last", 2000) == 16 and pool_ref.fwd_ulps(2048, 40, "last", 1) == 24
    assert pool_ref.fwd_ulps(8, 40, "masked_mean", 1) == 12
    assert pool_ref.fwd_ulps(8, 40, "masked_mean", 4) == 12 + 3 + 1
    assert pool_ref.fwd_ulps(8, 40, "masked_mean", 40) == 12 + (0 + 3 + 15) + 1            # ceil(40 / 16) = 3 rows per slice: one per wave
    assert pool_ref.fwd_ulps(1024, 2048, "masked_mean", 2048) == 16 + (31 + 3 + 15) + 1


@pytest.mark.parametrize("side", sorted(pool_ref.POOL_CASES))
@pytest.mark.parametrize("mode", pool_ref.MODES)
def test_oracle_with_pool_ref_matches_the_fixture(golden_dir, side, mode):
    """oracle.qwen3_ref.qwen3_forward composed with pool_ref.pool against what transformers.Qwen3Model and the reference's own
    last_token_pool (masked mean: the generator's) produced; the tolerance of tests/test_oracle_golden.py::test_qwen3_decoder"""
    case = pool_ref.POOL_CASES[side]
    g = dict(np.load(os.path.join(golden_dir, "pool_tiny.npz")))
    qc = cases.qwen_cfg(case)
    P = {k: torch.from_numpy(v) for k, v in W.fill_state_dict(Q.qwen3_shapes(qc, lora=False), case["seed"] + 1).items()}
    x, am, r = pool_ref.pool_case_inputs(side)
    assert am.shape == (3, 40) and (am[:, -1 if side == "left" else 0] == 1).all() and am.sum() < am.size
    xt = torch.from_numpy(x).requires_grad_(True)
    h = Q.qwen3_forward(P, qc, xt, torch.from_numpy(am), fully_masked="zero")
    pooled = pool_ref.pool(h, torch.from_numpy(am), mode)
    (pooled * torch.from_numpy(r)).sum().backward()
    _close(pooled.detach().numpy(), g[f"{side}/{mode}/pooled"], rtol=1e-3, atol=1e-4, what="pooled")
    _close(xt.grad.numpy(), g[f"{side}/{mode}/grad_inputs_embeds"], rtol=1e-3, atol=1e-7, what="grad_inputs_embeds")
    assert float(np.abs(g[f"{side}/{mode}/grad_inputs_embeds"][am == 0]).max()) == 0.0      # padding receives no gradient


def test_fixture_holds_outputs_only(golden_dir):
    g = np.load(os.path.join(golden_dir, "pool_tiny.npz"))
    assert sorted(g.files) == sorted(f"{s}/{m}/{k}" for s in pool_ref.POOL_CASES for m in pool_ref.MODES for k in ("pooled", "grad_inputs_embeds"))
    assert os.path.getsize(os.path.join(golden_dir, "pool_tiny.npz")) < (1 << 20)


# ---- the `pooling` field: refusals and the model_config.json round trip, on the host ------------------------------------------------------
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


def test_bogus_pooling_is_refused_by_name(monkeypatch):
    from unirec_amd.qwen3 import Qwen3Config, Qwen3LoRAModel

    def no_library():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_library)                         # before any device work
    for bad in ("bogus", "MEAN", "cls", 1, ""):
        with pytest.raises(ValueError, match="pooling"):
            _model(pooling=bad)
        with pytest.raises(ValueError, match="pooling"):
            Qwen3Config(pooling=bad)
    cfg = _cfg()
    cfg.pooling = "bogus"                                                  # set behind the constructor's back
    with pytest.raises(ValueError, match="pooling"):
        Qwen3LoRAModel(cfg)


def test_pooling_defaults_and_keyword():
    from unirec_amd.qwen3 import Qwen3Config
    assert Qwen3Config().pooling == "mean" and _model().base_model.pooling == "mean"
    assert _model(_cfg(pooling="last")).base_model.pooling == "last"                          # None keeps the config's value
    assert _model(_cfg(pooling="last"), pooling="masked_mean").base_model.pooling == "masked_mean"
    old = _cfg()
    del old.pooling                                                        # a config object from before the field
    assert _model(old).base_model.pooling == "mean"


@pytest.mark.parametrize("pooling", ["mean", "masked_mean", "last"])
def test_model_config_round_trip_on_the_host(tmp_path, pooling):
    from unirec_amd.joint import HistoryTokenTable, MultiModalQwenEmbedding
    m = _model(pooling=pooling)
    m.save_pretrained(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["adapter_config.json", "adapter_model.bin", "history_tokens.json", "model_config.json", "qformer_model.bin"]
    saved = json.load(open(os.path.join(tmp_path, "model_config.json")))
    assert saved == {"hidden_size": 256, "use_lora": True, "pooling": pooling}
    kw = dict(num_history_items=4, num_query_tokens_per_item=2, tokenizer=HistoryTokenTable(120, 4, 2))
    back = MultiModalQwenEmbedding.from_pretrained(str(tmp_path), _QF(256), qwen_config=_cfg(), **kw)
    assert back.base_model.pooling == pooling and back.base_model.config.pooling == pooling
    # a constructor keyword wins
    assert MultiModalQwenEmbedding.from_pretrained(str(tmp_path), _QF(256), qwen_config=_cfg(), pooling="last", **kw).base_model.pooling == "last"
    # a directory from before the field pools as it always did
    json.dump({"hidden_size": 256, "use_lora": True}, open(os.path.join(tmp_path, "model_config.json"), "w"))
    assert MultiModalQwenEmbedding.from_pretrained(str(tmp_path), _QF(256), qwen_config=_cfg(), **kw).base_model.pooling == "mean"
    json.dump({"hidden_size": 256, "use_lora": True, "pooling": "bogus"}, open(os.path.join(tmp_path, "model_config.json"), "w"))
    with pytest.raises(ValueError, match="pooling"):
        MultiModalQwenEmbedding.from_pretrained(str(tmp_path), _QF(256), qwen_config=_cfg(), **kw)

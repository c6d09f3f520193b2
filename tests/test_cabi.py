"""CPU: the C-ABI library builds, loads and exports exactly what include/unirec_hip.h declares
(no compute calls -- there is no GPU here)."""
import ctypes
import os
import re

from unirec_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "unirec_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ur_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_are_bound_and_exported():
    names = _declared()
    assert "ur_gemm" in names and "ur_version" in names
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in unirec_hip.h but not exported by libunirec_hip.so"
        assert n in _lib.SIGNATURES, f"{n} declared in unirec_hip.h but not bound in unirec_amd/_lib.py"
    extra = set(_lib.SIGNATURES) - set(names)
    assert not extra, f"bound but not declared in the header: {extra}"


def test_loader_binds_and_reports_version():
    lib = _lib.load()
    assert lib.ur_version() == _lib.ABI_VERSION
    assert isinstance(lib.ur_last_error(), bytes)


def test_the_library_sources_read_no_environment_variable():
    """include/unirec_hip.h: "The library reads no environment variable" -- however unirec_amd/csrc is built"""
    csrc = os.path.join(ROOT, "unirec_amd", "csrc")
    files = [os.path.join(d, f) for d, _, fs in os.walk(csrc) for f in fs]
    assert len(files) > 10
    hits = [os.path.relpath(f, ROOT) for f in files if b"getenv" in open(f, "rb").read()]
    assert not hits, f"getenv in the library sources: {hits}"


def test_invalid_arguments_are_rejected_without_a_gpu():
    """Argument validation happens on the host before any launch, so it is testable here."""
    lib = _lib.load()
    a = _lib.GemmArgs()
    a.M, a.N, a.K = 8, 8, 12          # K not a multiple of 8
    a.R = a.S = a.C = 256
    a.ldr = a.lds = 16
    a.ldc = 8
    a.r_kcontig = a.s_kcontig = 1
    rc = lib.ur_gemm(ctypes.byref(a), None, 0, None)
    assert rc < 0 and b"multiples of 8" in lib.ur_last_error()
    assert lib.ur_layernorm_fwd(None, 1, None, None, None, None, None, None, None, 4, 12, 1e-5, 0.0, 0, 0.0, 0, 0, None) < 0
    # communicator entry points: argument checks precede any RCCL / HIP call
    h = ctypes.c_void_p()
    assert lib.ur_comm_init(ctypes.byref(h), 3, 2, ctypes.create_string_buffer(128), 0) < 0 and b"outside a world" in lib.ur_last_error()
    assert lib.ur_comm_allreduce_async(None, None, 4, 0, None) < 0 and b"not a communicator" in lib.ur_last_error()
    assert lib.ur_comm_wait(None, None) < 0
    assert lib.ur_comm_destroy(None) == 0


def test_pointers_below_the_stated_alignment_are_refused_by_name_without_a_gpu():
    """the alignments include/unirec_hip.h states for the f32 planes, scratch and workspaces of ur_attn_fwd / ur_attn_bwd, ur_gemm and
    ur_rmsnorm_lora_fwd: a pointer below them is a negative return that names it, before any HIP call (fake addresses, never followed)"""
    lib, P = _lib.load(), 1 << 20
    a, g = _lib.AttnArgs(), _lib.AttnBwdArgs()
    a.q, a.k, a.v, a.o, a.stats = P, 2 * P, 3 * P, 4 * P, 5 * P + 2
    a.B, a.Sq, a.Sk, a.nq, a.nkv, a.head_dim, a.scale = 2, 33, 40, 2, 2, 64, 0.125
    a.ldq = a.ldk = a.ldv = a.ldo = g.lddo = g.lddq = g.lddk = g.lddv = 128
    assert lib.ur_attn_fwd(ctypes.byref(a), None) < 0 and b"stats must be 4-byte aligned" in lib.ur_last_error()
    a.stats = 5 * P + 4
    g.dout, g.dq, g.dk, g.dv, g.delta = 6 * P, 7 * P + 8, 8 * P + 8, 9 * P + 8, 10 * P + 2
    assert lib.ur_attn_bwd(ctypes.byref(a), ctypes.byref(g), None) < 0 and b"delta must be 4-byte aligned" in lib.ur_last_error()
    g.delta, g.kv_colsum, g.kv_colsum_ws = 10 * P + 4, 11 * P + 2, 12 * P + 4
    assert lib.ur_attn_bwd(ctypes.byref(a), ctypes.byref(g), None) < 0 and b"kv_colsum and kv_colsum_ws must be 4-byte aligned" in lib.ur_last_error()
    g.kv_colsum, g.kv_colsum_ws, g.rope_rstd = 0, 0, 13 * P + 2
    assert lib.ur_attn_bwd(ctypes.byref(a), ctypes.byref(g), None) < 0 and b"rope_rstd must be 4-byte aligned" in lib.ur_last_error()
    m = _lib.GemmArgs()
    m.M, m.N, m.K, m.R, m.S, m.C = 136, 136, 136, P, 2 * P, 3 * P
    m.ldr = m.lds = m.ldc = 136
    m.c_f32, m.split_k, m.alpha = 1, 2, 1.0
    need = lib.ur_gemm_workspace_bytes(ctypes.byref(m))
    assert need == 2 * 136 * 136 * 4
    assert lib.ur_gemm(ctypes.byref(m), 4 * P + 8, need, None) < 0 and b"workspace must be 16-byte aligned" in lib.ur_last_error()
    assert lib.ur_gemm(ctypes.byref(m), 4 * P, need - 1, None) < 0 and b"workspace too small" in lib.ur_last_error()
    assert lib.ur_gemm_grouped(ctypes.byref(m), 1, 4 * P + 8, need, None) < 0 and b"workspace must be 16-byte aligned" in lib.ur_last_error()
    r = _lib.LoraArgs()
    r.nad, r.rank, r.shared = 1, 16, 1
    assert lib.ur_rmsnorm_lora_fwd(P, 2 * P, 3 * P, 4 * P + 2, 8, 1024, 1e-6, ctypes.byref(r), None) < 0 and b"rstd must be 4-byte aligned" in lib.ur_last_error()


def test_product_path_has_no_oracle_import():
    """The oracle is test infrastructure: nothing under unirec_amd/ may import it."""
    pkg = os.path.join(ROOT, "unirec_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith(".py"):
                txt = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M), os.path.join(dp, f)


def test_live_and_dead_parameter_split_matches_the_reference_probe():
    """dead = word/position embeddings + the per-layer TEXT FFN; attention.output / crossattention.output
    are live (a substring match once froze them by accident)."""
    import torch
    from unirec_amd.qformer import _dead
    from unirec_amd.qformer_utils import QFormerForItemRepresentation
    with torch.device("meta"):
        m = QFormerForItemRepresentation(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=1024,
                                         num_query_tokens=4, field_embedding_dim=256, num_fields=8)
    live = {n for n, _ in m.live_named_parameters()}
    named = dict(m.named_parameters())
    assert all(_dead(n) == (n not in live) for n in named)
    # C1 live / dead parameter counts probed on the reference: 1 976 360 / 8 996 864
    assert sum(named[n].numel() for n in live) == 1976360 and sum(p.numel() for n, p in named.items() if n not in live) == 8996864

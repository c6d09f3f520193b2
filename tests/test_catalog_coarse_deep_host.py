"""CPU: the host side of the long two-stage retrieval family -- the rules include/unirec_hip_coarse_deep.h is held to (declared <=>
exported <=> bound, a name in one header only, the ctypes mirrors of its structs field for field, both entry points named in the COVERS
dict of tests/test_gpu_catalog_coarse_deep.py), every refusal of the two entry points and their size queries through the raw library
(fake non-null pointers: each call returns before any launch), the two workspace plans under the host sanitizers, and the route
CatalogEvaluator.retrieve_two_stage takes with every device call out of reach."""
import ast
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from unirec_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "unirec_hip_coarse_deep.h")
GPU_TESTS = "tests/test_gpu_catalog_coarse_deep.py"
OTHER_HEADERS = ("unirec_hip.h", "unirec_hip_loss.h", "unirec_hip_adapter.h", "unirec_hip_pool.h", "unirec_hip_mrl.h", "unirec_hip_coarse.h",
                 "unirec_hip_deep.h")
SELECT, RERANK = "ur_catalog_coarse_deep_select", "ur_catalog_deep_rerank"
FAKE = 1 << 20          # non-null, 16-byte aligned, never dereferenced on the host
MB = 1 << 24
F32, BF16 = torch.float32, torch.bfloat16


# ---- the header: declared <=> exported <=> bound, the struct mirrors, a test per entry point ---------------------------------------------
def _source(header=HEADER):
    return re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)


def _declared(header=HEADER):
    return sorted(set(re.findall(r"\b(ur_[a-z0-9_]+)\s*\(", _source(header))))


def test_coarse_deep_header_symbols_are_bound_and_exported():
    names = _declared()
    assert names == sorted([SELECT, RERANK])
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        assert hasattr(lib, name), f"{name} declared in unirec_hip_coarse_deep.h but not exported by libunirec_hip.so"
    assert sorted(_lib.COARSE_DEEP_SIGNATURES) == names, "declared <=> bound in unirec_amd/_lib.py"
    others = set(_lib.SIGNATURES) | set(_lib.LOSS_SIGNATURES) | set(_lib.ADAPTER_SIGNATURES) | set(_lib.POOL_SIGNATURES) | \
        set(_lib.MRL_SIGNATURES) | set(_lib.COARSE_SIGNATURES) | set(_lib.DEEP_SIGNATURES)
    assert not set(_lib.COARSE_DEEP_SIGNATURES) & others, "a name belongs to one header"
    for other in OTHER_HEADERS:
        assert not set(names) & set(_declared(os.path.join(ROOT, "include", other))), f"{other} declares an entry point of this family"
    loaded = _lib.load()
    for name in names:
        assert getattr(loaded, name).argtypes == _lib.COARSE_DEEP_SIGNATURES[name][1], f"load() did not bind {name}"
        assert getattr(loaded, name).restype == _lib.COARSE_DEEP_SIGNATURES[name][0]
    assert _lib.ABI_VERSION >= 27 and loaded.ur_version() == _lib.ABI_VERSION      # (this header arrived with ABI 27)
    # the older families keep exactly their entry points
    assert sorted(_lib.COARSE_SIGNATURES) == ["ur_catalog_coarse_select", "ur_catalog_rerank"]
    assert sorted(_lib.DEEP_SIGNATURES) == ["ur_catalog_deep_select"]


_CTYPE = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}


def _header_structs():
    """{typedef name: [(field name, ctypes type)]} of every struct the header declares, read from its text"""
    out = {}
    for body, name in re.findall(r"typedef struct \{(.*?)\}\s*(\w+);", _source(), flags=re.S):
        fields = []
        for decl in (d.strip() for d in body.split(";")):
            if not decl:
                continue
            m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)", decl)
            assert m, f"{name}: cannot read the field declaration {decl!r}"
            ctype, star, field = m.groups()
            fields.append((field, ctypes.c_void_p if star else _CTYPE[ctype]))
        out[name] = fields
    return out


def test_struct_mirrors_match_the_header_field_for_field():
    structs = _header_structs()
    assert sorted(structs) == ["ur_catalog_coarse_deep_t", "ur_catalog_deep_rerank_t"]
    for typedef, got in (("ur_catalog_coarse_deep_t", _lib.CatalogCoarseDeep), ("ur_catalog_deep_rerank_t", _lib.CatalogDeepRerank)):
        fields = structs[typedef]
        want = type("FromHeader", (ctypes.Structure,), {"_fields_": fields})
        assert [f[0] for f in got._fields_] == [f[0] for f in fields], f"{typedef}: field names and order"
        assert ctypes.sizeof(got) == ctypes.sizeof(want)
        for (name, t), (_, tw) in zip(got._fields_, fields):
            assert getattr(got, name).offset == getattr(want, name).offset, (typedef, name)
            assert t is tw, f"{typedef}.{name}: {t} against the header's {tw}"
    # ur_catalog_coarse_t's fields in their order, plus segments before the workspace (as in ur_catalog_deep_t); ur_catalog_rerank_t's
    coarse = [f[0] for f in _lib.CatalogCoarse._fields_]
    at = coarse.index("workspace")
    assert [f[0] for f in _lib.CatalogCoarseDeep._fields_] == coarse[:at] + ["segments"] + coarse[at:]
    deep = [f[0] for f in _lib.CatalogDeep._fields_]
    assert deep[deep.index("segments") + 1] == "workspace"
    assert [f[0] for f in _lib.CatalogDeepRerank._fields_] == [f[0] for f in _lib.CatalogRerank._fields_]


def test_both_entry_points_are_listed_in_the_gpu_file():
    with open(os.path.join(ROOT, GPU_TESTS)) as f:
        tree = ast.parse(f.read())
    covers = None
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "COVERS" for t in node.targets):
            covers = ast.literal_eval(node.value)
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    assert isinstance(covers, dict), f"{GPU_TESTS} has no top-level COVERS dict"
    assert sorted(covers) == _declared(), "COVERS lists exactly the two entry points of unirec_hip_coarse_deep.h"
    for entry in covers:
        assert covers[entry] and all(name in tests for name in covers[entry]), covers


# ---- every refusal, without a GPU --------------------------------------------------------------------------------------------------------
_SELECT_PTRS = ("user", "catalog", "cat_inv_norm", "topk_index", "topk_score", "gt_index", "rank", "exclude", "workspace")
_RERANK_PTRS = ("user", "catalog", "cat_inv_norm", "index", "topk_index", "topk_score", "workspace")


def _args(cls, fn, ptrs, sizes, query, over):
    """a valid argument struct over fake pointers with `over` applied; the workspace is sized by the size query of the call's own sizes
    (query=True) unless `workspace_bytes` is given"""
    a = cls()
    names = [f[0] for f in a._fields_]
    for i, n in enumerate(ptrs):
        setattr(a, n, FAKE + i * MB)
    for k, v in sizes.items():
        setattr(a, k, v)
    for k, v in over.items():
        assert k in names, k
        setattr(a, k, v)
    if query and "workspace_bytes" not in over:
        q = cls()
        ctypes.memmove(ctypes.byref(q), ctypes.byref(a), ctypes.sizeof(a))
        q.workspace = None
        a.workspace_bytes = q.workspace_bytes if fn(ctypes.byref(q), None) == 0 else 1 << 40
    return a


def _select_args(lib=None, **over):
    """B 3, N 2000, D 40, K 300, E 5, chunk_rows 1024, bf16"""
    return _args(_lib.CatalogCoarseDeep, lib and lib.ur_catalog_coarse_deep_select, _SELECT_PTRS,
                 dict(B=3, N=2000, D=40, K=300, E=5, chunk_rows=1024, catalog_bf16=1), lib is not None, over)


def _rerank_args(lib=None, **over):
    """B 3, N 2000, D 40, K_in 300, k 200, f32"""
    return _args(_lib.CatalogDeepRerank, lib and lib.ur_catalog_deep_rerank, _RERANK_PTRS, dict(B=3, N=2000, D=40, K_in=300, k=200),
                 lib is not None, over)


def test_select_refuses_invalid_arguments_without_a_gpu():
    lib = _lib.load()
    fn = lib.ur_catalog_coarse_deep_select

    def rejected(word, **over):
        rc = fn(ctypes.byref(_select_args(lib, **over)), None)
        msg = lib.ur_last_error()
        assert rc < 0 and SELECT.encode() in msg and word in msg, (over, rc, msg)

    assert fn(None, None) < 0 and SELECT.encode() in lib.ur_last_error()
    rejected(b"B >= 0", B=-1)
    rejected(b"N", N=-1)
    rejected(b"N", N=1 << 31)
    for D in (0, 4, 12, 2056, -8, 41, 4096):
        rejected(b"D must be", D=D)
    for K in (0, -1, 1025):
        rejected(b"K must be", K=K)
    rejected(b"chunk_rows", chunk_rows=1000)
    rejected(b"chunk_rows", chunk_rows=-1024)
    rejected(b"exclude", exclude=None)                                   # E = 5 with a null exclude
    rejected(b"gt_index and rank", rank=None)
    rejected(b"gt_index and rank", gt_index=None)
    for flag in (0, 2, -1):                                              # an f32 catalogue is refused by name
        rejected(b"catalog_bf16", catalog_bf16=flag)
    for segments in (-1, 17):
        rejected(b"segments", segments=segments)
    for name in ("topk_index", "topk_score", "user", "catalog", "cat_inv_norm"):
        rejected(b"null", **{name: None})
    for name in ("user", "catalog"):
        rejected(b"aligned", **{name: FAKE + 20 * MB + 8})
    need = _select_args(lib).workspace_bytes
    assert need > 0
    rejected(b"workspace", workspace_bytes=need - 1)
    rejected(b"workspace", workspace=FAKE + 21 * MB + 4)
    # the limits themselves pass every check up to the pointers, with B == 0
    for over in (dict(K=1024), dict(K=1), dict(K=128), dict(K=129), dict(D=8), dict(D=2048), dict(segments=16), dict(N=0)):
        assert fn(ctypes.byref(_select_args(lib, B=0, **over)), None) == 0, (over, lib.ur_last_error())
    none = {n: None for n in _SELECT_PTRS if n not in ("workspace", "exclude", "gt_index", "rank")}
    assert fn(ctypes.byref(_select_args(lib, B=0, **none)), None) == 0, lib.ur_last_error()


def test_rerank_refuses_invalid_arguments_without_a_gpu():
    lib = _lib.load()
    fn = lib.ur_catalog_deep_rerank

    def rejected(word, **over):
        rc = fn(ctypes.byref(_rerank_args(lib, **over)), None)
        msg = lib.ur_last_error()
        assert rc < 0 and RERANK.encode() in msg and word in msg, (over, rc, msg)

    assert fn(None, None) < 0 and RERANK.encode() in lib.ur_last_error()
    rejected(b"B >= 0", B=-1)
    rejected(b"N", N=0)
    rejected(b"N", N=1 << 31)
    for D in (0, 6, 2052, -4, 41):
        rejected(b"D must be", D=D)
    rejected(b"D must be", D=12, catalog_bf16=1)                         # a bf16 catalogue takes multiples of 8
    for K_in in (0, -1, 1025):
        rejected(b"K_in must be", K_in=K_in, k=1)
    for k in (0, -1, 301):
        rejected(b"k must be", k=k)
    for flag in (2, -1):
        rejected(b"catalog_bf16", catalog_bf16=flag)
    for name in ("index", "topk_index", "topk_score", "user", "catalog", "cat_inv_norm"):
        rejected(b"null", **{name: None})
    for name in ("user", "catalog"):
        rejected(b"aligned", **{name: FAKE + 20 * MB + 8})
    need = _rerank_args(lib).workspace_bytes
    assert need > 0
    rejected(b"workspace", workspace_bytes=need - 1)
    rejected(b"workspace", workspace=FAKE + 21 * MB + 4)
    for over in (dict(K_in=1024, k=1024), dict(K_in=1, k=1), dict(K_in=129, k=129), dict(D=4), dict(D=2048, catalog_bf16=1), dict(D=12)):
        assert fn(ctypes.byref(_rerank_args(lib, B=0, **over)), None) == 0, (over, lib.ur_last_error())
    # the short entry point keeps its limit
    a = _lib.CatalogRerank()
    ctypes.memmove(ctypes.byref(a), ctypes.byref(_rerank_args(None, K_in=129, k=1)), ctypes.sizeof(a))
    assert lib.ur_catalog_rerank(ctypes.byref(a), None) < 0 and b"K_in must be" in lib.ur_last_error()


def _pad16(n):
    return (n + 15) // 16 * 16


def _select_need(lib, **over):
    a = _select_args(None, **over)
    a.workspace, a.workspace_bytes = None, -1
    assert lib.ur_catalog_coarse_deep_select(ctypes.byref(a), None) == 0, lib.ur_last_error()
    return a.workspace_bytes


def _rerank_need(lib, **over):
    a = _rerank_args(None, **over)
    a.workspace, a.workspace_bytes = None, -1
    assert lib.ur_catalog_deep_rerank(ctypes.byref(a), None) == 0, lib.ur_last_error()
    return a.workspace_bytes


def test_size_queries_equal_the_documented_workspaces_and_do_not_launch():
    lib = _lib.load()
    # u~ [B,D] bf16 | iu~ [B] | ref [B] | chunk [B, rows] f32 | list scores, list indices [B, Gw, K] | counts [B, Gw];
    # Gw = min(max(1024 / B, 1), 8) unless segments names it; rows = chunk_rows or the 64 MB rule, never more than N rounded up to 1024
    def want(B, D, rows, K, gw):
        return max(16, _pad16(B * D * 2) + 2 * _pad16(B * 4) + _pad16(B * rows * 4) + 2 * _pad16(B * gw * K * 4) + _pad16(B * gw * 4))
    assert _select_need(lib) == want(3, 40, 1024, 300, 8)
    assert _select_need(lib, chunk_rows=0) == want(3, 40, 2048, 300, 8)
    assert _select_need(lib, segments=1) == want(3, 40, 1024, 300, 1) and _select_need(lib, segments=16) == want(3, 40, 1024, 300, 16)
    big = _select_need(lib, B=512, N=1 << 30, D=1024, K=1024, chunk_rows=0)
    assert big == want(512, 1024, (64 << 20) // (4 * 512), 1024, 2) == (1 << 20) + 2 * 2048 + (64 << 20) + 2 * (4 << 20) + 4096
    assert _select_need(lib, B=512, N=1 << 20, D=1024, K=1024, chunk_rows=0) == big                 # nothing of size B x N
    assert _select_need(lib, B=64, N=1 << 20, D=1024, K=1000, chunk_rows=0) == want(64, 1024, 1 << 18, 1000, 8)
    assert _select_need(lib, B=2000, N=1 << 20, D=8, K=129, chunk_rows=2048) == want(2000, 8, 2048, 129, 1)
    assert _select_need(lib, B=0) == 16
    # the query needs no pointer at all (and no device), and still refuses what the call refuses, leaving workspace_bytes alone
    a = _select_args(None, E=0, **{n: None for n in _SELECT_PTRS if n != "exclude"})
    a.workspace_bytes = -1
    assert lib.ur_catalog_coarse_deep_select(ctypes.byref(a), None) == 0 and a.workspace_bytes == _select_need(lib, E=0)
    for over, word in ((dict(D=4), b"D must be"), (dict(K=1025), b"K must be"), (dict(K=0), b"K must be"), (dict(catalog_bf16=0), b"catalog_bf16"),
                       (dict(chunk_rows=1000), b"chunk_rows"), (dict(segments=17), b"segments")):
        a = _select_args(None, workspace=None, **over)
        a.workspace_bytes = 123
        assert lib.ur_catalog_coarse_deep_select(ctypes.byref(a), None) < 0 and word in lib.ur_last_error() and a.workspace_bytes == 123
    # the re-rank: iu [B] | scores [B, K_in]
    assert _rerank_need(lib) == _pad16(3 * 4) + _pad16(3 * 300 * 4)
    assert _rerank_need(lib, B=512, K_in=1024, k=1000, N=1 << 20, D=1024) == 2048 + (2 << 20)
    assert _rerank_need(lib, B=5, K_in=1, k=1) == 32 + 32 and _rerank_need(lib, B=0) == 16
    a = _rerank_args(None, **{n: None for n in _RERANK_PTRS})
    a.workspace_bytes = -1
    assert lib.ur_catalog_deep_rerank(ctypes.byref(a), None) == 0 and a.workspace_bytes == _rerank_need(lib)
    for over, word in ((dict(D=6), b"D must be"), (dict(K_in=1025), b"K_in must be"), (dict(k=301), b"k must be"), (dict(N=0), b"N")):
        a = _rerank_args(None, workspace=None, **over)
        a.workspace_bytes = 123
        assert lib.ur_catalog_deep_rerank(ctypes.byref(a), None) < 0 and word in lib.ur_last_error() and a.workspace_bytes == 123


def test_coarse_deep_workspace_layouts_under_the_host_sanitizers(tmp_path):
    """tests/host/catalog_coarse_deep_layout_check.cpp: the two plans over a grid of B, N, D, K and segments -- regions aligned, disjoint
    and inside the size the query answers, the size the closed form -- as a stand-alone host program under AddressSanitizer and UBSan"""
    # the sanitizer runtimes are linked statically: a dynamic one insists on being the first library the process loads
    gxx, clang = shutil.which("g++"), shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    cxx = [gxx, "-static-libasan", "-static-libubsan"] if gxx else [clang, "-static-libsan"]
    exe = str(tmp_path / "catalog_coarse_deep_layout_check")
    subprocess.run(cxx + ["-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                          "-I", os.path.join(ROOT, "unirec_amd", "csrc"),
                          os.path.join(ROOT, "tests", "host", "catalog_coarse_deep_layout_check.cpp"), "-o", exe], check=True)
    # (the program allocates nothing it does not free at exit; the leak pass needs ptrace, which a sandbox may not grant)
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0 and run.stdout.split() == ["ok", "8640"], (run.returncode, run.stdout, run.stderr)


# ---- the route retrieve_two_stage takes, with every device call out of reach -----------------------------------------------------------
class Reached(Exception):
    pass


@pytest.fixture
def routes(monkeypatch):
    """every launch wrapper an evaluator could reach raises Reached(name, arguments); loading the library fails if touched"""
    from unirec_amd import hip

    def raiser(name):
        def touched(*a, **k):
            raise Reached(name, a, k)
        return touched
    for name in ("catalog_deep_select", "catalog_select", "catalog_coarse_select", "catalog_rerank", "catalog_scores", "catalog_softmax",
                 "catalog_coarse_deep_select", "catalog_deep_rerank"):
        monkeypatch.setattr(hip, name, raiser(name))
    monkeypatch.setattr(_lib, "load", raiser("_lib.load"))


def _evaluator(dtype=F32):
    from unirec_amd.evaluation import CatalogEvaluator
    return CatalogEvaluator(torch.arange(200 * 16, dtype=F32).reshape(200, 16).sin(), device="cpu", dtype=dtype)


def test_retrieve_two_stage_accepts_and_refuses_by_k_and_shortlist(routes):
    u = torch.ones(2, 16)
    ev = _evaluator(BF16)
    # accepted: the coarse-deep select is reached with the shortlist as its K, whatever the size
    for kw, S in ((dict(k=10, shortlist=10), 10), (dict(k=10, shortlist=128), 128), (dict(k=10, shortlist=129), 129),
                  (dict(k=200, shortlist=1024), 1024), (dict(k=1024, shortlist=1024), 1024), (dict(k=1, shortlist=1), 1),
                  (dict(), 128), (dict(k=64), 128), (dict(k=65), 130), (dict(k=500), 1000), (dict(k=513), 1024), (dict(k=1024), 1024),
                  (dict(k=300, exclude=[[1, 2], [5]], gt_index=torch.tensor([3, 4]), chunk_rows=1024), 600)):
        with pytest.raises(Reached) as hit:
            ev.retrieve_two_stage(u, **kw)
        name, args, kwargs = hit.value.args
        assert name == "catalog_coarse_deep_select" and args[2] == S, (kw, name, args[2:])
        assert kwargs["chunk_rows"] == kw.get("chunk_rows") and (kwargs["gt_index"] is None) == ("gt_index" not in kw)
    # refused before any device call: ints only, no bools, 1 <= k <= shortlist <= 1024
    for kw in (dict(k=0), dict(k=-1), dict(k=1025), dict(k=10.0), dict(k="10"), dict(k=True), dict(k=None),
               dict(k=10, shortlist=9), dict(k=10, shortlist=1025), dict(k=10, shortlist=128.0), dict(k=10, shortlist=True),
               dict(k=1, shortlist=0), dict(k=200, shortlist=128)):
        with pytest.raises(ValueError, match="retrieve_two_stage: (k|shortlist) must be an int in"):
            ev.retrieve_two_stage(u, **kw)
    # an f32 catalogue: the message retrieve(shortlist=) gives
    with pytest.raises(ValueError) as two:
        _evaluator(F32).retrieve_two_stage(u, k=10, shortlist=300)
    with pytest.raises(ValueError) as old:
        _evaluator(F32).retrieve(u, k=10, shortlist=100)
    assert str(two.value) == str(old.value) and "bf16 catalogue" in str(two.value)
    assert "NOT a tuned value" in type(ev).retrieve_two_stage.__doc__


def test_the_second_stage_is_the_deep_rerank_with_k(monkeypatch):
    from unirec_amd import hip
    calls = []

    def select(u, cat, K, inv, gt_index=None, exclude=None, chunk_rows=None):
        calls.append(("select", K))
        rank = None if gt_index is None else torch.ones(u.shape[0], dtype=torch.int32)
        return torch.zeros(u.shape[0], K, dtype=torch.int32), None, rank, "norms"

    def rerank(u, cat, index, k, inv):
        calls.append(("rerank", tuple(index.shape), k, inv))
        return index[:, :k], torch.zeros(u.shape[0], k), inv
    monkeypatch.setattr(hip, "catalog_coarse_deep_select", select)
    monkeypatch.setattr(hip, "catalog_deep_rerank", rerank)
    ev = _evaluator(BF16)
    out = ev.retrieve_two_stage(torch.ones(2, 16), k=200, shortlist=700, gt_index=[3, 4], ks=(1, 10))
    assert calls == [("select", 700), ("rerank", (2, 700), 200, "norms")] and ev._inv == "norms"
    assert out["topk_index"].shape == (2, 200) and out["rank_is_coarse"] is True and out["mrr"] == 1.0
    assert out["hit_at"] == {1: 1.0, 10: 1.0} and set(out["ndcg_at"]) == {1, 10}
    out = ev.retrieve_two_stage(torch.ones(2, 16), k=5)
    assert sorted(out) == ["topk_index", "topk_score"] and calls[-2:] == [("select", 128), ("rerank", (2, 128), 5, "norms")]


def test_retrieve_keeps_its_routes_and_refusals(routes):
    u = torch.ones(2, 16)
    for dtype in (F32, BF16):
        ev = _evaluator(dtype)
        for kw, name in ((dict(k=129), "catalog_deep_select"), (dict(k=1024), "catalog_deep_select"), (dict(k=128), "catalog_select"),
                         (dict(), "catalog_select")):
            with pytest.raises(Reached) as hit:
                ev.retrieve(u, **kw)
            assert hit.value.args[0] == name
        with pytest.raises(ValueError, match=r"\bk\b.*1024"):
            ev.retrieve(u, k=1025)
    ev = _evaluator(BF16)
    for kw in (dict(k=10, shortlist=129), dict(k=200, shortlist=128), dict(k=10, shortlist=9)):
        with pytest.raises(ValueError, match="shortlist must be an int in"):
            ev.retrieve(u, **kw)
    with pytest.raises(Reached) as hit:
        ev.retrieve(u, k=10, shortlist=128)
    assert hit.value.args[0] == "catalog_coarse_select"


def test_wrappers_refuse_before_the_library():
    from unirec_amd import hip
    u = torch.zeros(2, 16)
    with pytest.raises(_lib.UniRecHipError, match="no CPU fallback"):
        hip.catalog_coarse_deep_select(u, torch.zeros(5, 16, dtype=BF16), 300)
    with pytest.raises(ValueError, match="catalog_coarse_deep_select.*bf16 catalogue"):
        hip.catalog_coarse_deep_select(u, torch.zeros(5, 16), 300)
    with pytest.raises(_lib.UniRecHipError, match="no CPU fallback"):
        hip.catalog_deep_rerank(u, torch.zeros(5, 16), torch.zeros(2, 300, dtype=torch.int32))
    with pytest.raises(ValueError, match="catalog_deep_rerank.*f32 or bf16"):
        hip.catalog_deep_rerank(u, torch.zeros(5, 16, dtype=torch.float16), torch.zeros(2, 300, dtype=torch.int32))
    with pytest.raises(ValueError, match="catalog_deep_rerank.*share D"):
        hip.catalog_deep_rerank(u, torch.zeros(5, 12), torch.zeros(2, 300, dtype=torch.int32))

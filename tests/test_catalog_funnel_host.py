"""CPU: the host side of the funnel retrieval family -- the rules include/unirec_hip_funnel.h is held to (declared <=> exported <=>
bound, a name in one header only, the ctypes mirrors of its structs field for field, the three entry points named in the COVERS dict of
tests/test_gpu_catalog_funnel.py), every refusal of the three entry points and of the two size queries through the raw library (fake
non-null pointers: each call returns before any launch), the size queries against the closed forms the header documents, the two
workspace plans under the host sanitizers, and the route CatalogEvaluator.retrieve_funnel takes with every device call out of reach."""
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
HEADER = os.path.join(ROOT, "include", "unirec_hip_funnel.h")
GPU_TESTS = "tests/test_gpu_catalog_funnel.py"
OTHER_HEADERS = ("unirec_hip.h", "unirec_hip_loss.h", "unirec_hip_adapter.h", "unirec_hip_pool.h", "unirec_hip_mrl.h", "unirec_hip_coarse.h",
                 "unirec_hip_deep.h", "unirec_hip_coarse_deep.h")
NORMS, SELECT, RERANK = "ur_catalog_prefix_norms", "ur_catalog_funnel_select", "ur_catalog_funnel_rerank"
FAKE = 1 << 20          # non-null, 16-byte aligned, never dereferenced on the host
MB = 1 << 24
F32, BF16 = torch.float32, torch.bfloat16


# ---- the header: declared <=> exported <=> bound, the struct mirrors, a test per entry point ---------------------------------------------
def _source(header=HEADER):
    return re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)


def _declared(header=HEADER):
    return sorted(set(re.findall(r"\b(ur_[a-z0-9_]+)\s*\(", _source(header))))


def test_funnel_header_symbols_are_bound_and_exported():
    names = _declared()
    assert names == sorted([NORMS, SELECT, RERANK])
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        assert hasattr(lib, name), f"{name} declared in unirec_hip_funnel.h but not exported by libunirec_hip.so"
    assert sorted(_lib.FUNNEL_SIGNATURES) == names, "declared <=> bound in unirec_amd/_lib.py"
    others = set(_lib.SIGNATURES) | set(_lib.LOSS_SIGNATURES) | set(_lib.ADAPTER_SIGNATURES) | set(_lib.POOL_SIGNATURES) | \
        set(_lib.MRL_SIGNATURES) | set(_lib.COARSE_SIGNATURES) | set(_lib.DEEP_SIGNATURES) | set(_lib.COARSE_DEEP_SIGNATURES)
    assert not set(_lib.FUNNEL_SIGNATURES) & others, "a name belongs to one header"
    for other in OTHER_HEADERS:
        assert not set(names) & set(_declared(os.path.join(ROOT, "include", other))), f"{other} declares an entry point of this family"
    loaded = _lib.load()
    for name in names:
        assert getattr(loaded, name).argtypes == _lib.FUNNEL_SIGNATURES[name][1], f"load() did not bind {name}"
        assert getattr(loaded, name).restype == _lib.FUNNEL_SIGNATURES[name][0]
    assert _lib.ABI_VERSION >= 28 and loaded.ur_version() == _lib.ABI_VERSION      # (this header arrived with ABI 28)
    # the older families keep exactly their entry points
    assert sorted(_lib.COARSE_SIGNATURES) == ["ur_catalog_coarse_select", "ur_catalog_rerank"]
    assert sorted(_lib.DEEP_SIGNATURES) == ["ur_catalog_deep_select"]
    assert sorted(_lib.COARSE_DEEP_SIGNATURES) == ["ur_catalog_coarse_deep_select", "ur_catalog_deep_rerank"]
    # the constants of the header
    defines = dict(re.findall(r"#define (UR_FUNNEL_\w+) (\d+)", _source()))
    assert defines == {"UR_FUNNEL_MAX_DIMS": str(_lib.FUNNEL_MAX_DIMS), "UR_FUNNEL_USER_GROUP": str(_lib.FUNNEL_USER_GROUP)}
    assert _lib.FUNNEL_MAX_DIMS == _lib.MRL_MAX_DIMS


_CTYPE = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}


def _header_structs():
    """{typedef name: [(field name, ctypes type)]} of every struct the header declares, read from its text (arrays sized by a #define)"""
    src = _source()
    defines = {k: int(v) for k, v in re.findall(r"#define (\w+) (\d+)", src)}
    out = {}
    for body, name in re.findall(r"typedef struct \{(.*?)\}\s*(\w+);", src, flags=re.S):
        fields = []
        for decl in (d.strip() for d in body.split(";")):
            if not decl:
                continue
            m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)(?:\[(\w+)\])?", decl)
            assert m, f"{name}: cannot read the field declaration {decl!r}"
            ctype, star, field, count = m.groups()
            t = ctypes.c_void_p if star else _CTYPE[ctype]
            fields.append((field, t * defines[count] if count else t))
        out[name] = fields
    return out


def test_struct_mirrors_match_the_header_field_for_field():
    structs = _header_structs()
    assert sorted(structs) == ["ur_catalog_funnel_rerank_t", "ur_catalog_funnel_select_t", "ur_catalog_prefix_norms_t"]
    for typedef, got in (("ur_catalog_prefix_norms_t", _lib.CatalogPrefixNorms), ("ur_catalog_funnel_select_t", _lib.CatalogFunnelSelect),
                         ("ur_catalog_funnel_rerank_t", _lib.CatalogFunnelRerank)):
        fields = structs[typedef]
        want = type("FromHeader", (ctypes.Structure,), {"_fields_": fields})
        assert [f[0] for f in got._fields_] == [f[0] for f in fields], f"{typedef}: field names and order"
        assert ctypes.sizeof(got) == ctypes.sizeof(want)
        for (name, t), (_, tw) in zip(got._fields_, fields):
            assert getattr(got, name).offset == getattr(want, name).offset, (typedef, name)
            same_array = hasattr(t, "_length_") and hasattr(tw, "_length_") and t._length_ == tw._length_ and t._type_ is tw._type_
            assert t is tw or same_array, f"{typedef}.{name}: {t} against the header's {tw}"

    # the fields of ur_catalog_coarse_deep_t / ur_catalog_deep_rerank_t, with dim, ld and ldu in place of D
    def swapped(cls):
        names = [f[0] for f in cls._fields_]
        at = names.index("D")
        return names[:at] + ["dim", "ld", "ldu"] + names[at + 1:]
    assert [f[0] for f in _lib.CatalogFunnelSelect._fields_] == swapped(_lib.CatalogCoarseDeep)
    assert [f[0] for f in _lib.CatalogFunnelRerank._fields_] == swapped(_lib.CatalogDeepRerank)


def test_the_three_entry_points_are_listed_in_the_gpu_file():
    with open(os.path.join(ROOT, GPU_TESTS)) as f:
        tree = ast.parse(f.read())
    covers = None
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "COVERS" for t in node.targets):
            covers = ast.literal_eval(node.value)
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    assert isinstance(covers, dict), f"{GPU_TESTS} has no top-level COVERS dict"
    assert sorted(covers) == _declared(), "COVERS lists exactly the three entry points of unirec_hip_funnel.h"
    for entry in covers:
        assert covers[entry] and all(name in tests for name in covers[entry]), covers


# ---- every refusal, without a GPU --------------------------------------------------------------------------------------------------------
_SELECT_PTRS = ("user", "catalog", "cat_inv_norm", "topk_index", "topk_score", "gt_index", "rank", "exclude", "workspace")
_RERANK_PTRS = ("user", "catalog", "cat_inv_norm", "index", "topk_index", "topk_score", "workspace")
_NORMS_PTRS = ("catalog", "inv")


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
        if k == "dims":
            a.dims[:len(v)] = v
        else:
            setattr(a, k, v)
    if query and "workspace_bytes" not in over:
        q = cls()
        ctypes.memmove(ctypes.byref(q), ctypes.byref(a), ctypes.sizeof(a))
        q.workspace = None
        a.workspace_bytes = q.workspace_bytes if fn(ctypes.byref(q), None) == 0 else 1 << 40
    return a


def _select_args(lib=None, **over):
    """B 3, N 2000, dim 40 of ld 72 and ldu 48, K 300, E 5, chunk_rows 1024, bf16"""
    return _args(_lib.CatalogFunnelSelect, lib and lib.ur_catalog_funnel_select, _SELECT_PTRS,
                 dict(B=3, N=2000, dim=40, ld=72, ldu=48, K=300, E=5, chunk_rows=1024, catalog_bf16=1), lib is not None, over)


def _rerank_args(lib=None, **over):
    """B 3, N 2000, dim 40 of ld 72 and ldu 48, K_in 300, k 200, f32"""
    return _args(_lib.CatalogFunnelRerank, lib and lib.ur_catalog_funnel_rerank, _RERANK_PTRS,
                 dict(B=3, N=2000, dim=40, ld=72, ldu=48, K_in=300, k=200), lib is not None, over)


def _norms_args(**over):
    """N 2000, ld 72, dims (8, 40, 72), f32"""
    over.setdefault("dims", (8, 40, 72))
    return _args(_lib.CatalogPrefixNorms, None, _NORMS_PTRS, dict(N=2000, ld=72, L=3), False, over)


def test_prefix_norms_refuses_invalid_arguments_without_a_gpu():
    lib = _lib.load()
    fn = lib.ur_catalog_prefix_norms

    def rejected(word, **over):
        rc = fn(ctypes.byref(_norms_args(**over)), None)
        msg = lib.ur_last_error()
        assert rc < 0 and NORMS.encode() in msg and word in msg, (over, rc, msg)

    assert fn(None, None) < 0 and NORMS.encode() in lib.ur_last_error()
    for flag in (2, -1):
        rejected(b"catalog_bf16", catalog_bf16=flag)
    rejected(b"N", N=-1)
    rejected(b"N", N=1 << 31)
    for L in (0, -1, 9):                                                 # L out of 1 .. UR_FUNNEL_MAX_DIMS
        rejected(b"L must be", L=L)
    for ld in (0, -72, 70):
        rejected(b"ld must be", ld=ld)
    rejected(b"ld must be", ld=76, catalog_bf16=1)                       # a bf16 row stride takes multiples of 8
    rejected(b"dims[0]", dims=(0, 40, 72))
    rejected(b"dims[1]", dims=(8, 42, 72))
    rejected(b"dims[0]", dims=(-8, 40, 72))
    rejected(b"dims[1]", dims=(8, 12, 72), catalog_bf16=1)               # multiples of 8 for a bf16 catalogue
    rejected(b"strictly ascending", dims=(8, 8, 72))                     # dims not ascending
    rejected(b"strictly ascending", dims=(40, 8, 72))
    rejected(b"exceeds ld", dims=(8, 40, 76))                            # a prefix wider than the row
    rejected(b"dims[0]", dims=(2052,), L=1, ld=4096)                     # past 2048
    for name in _NORMS_PTRS:
        rejected(b"null", **{name: None})
    rejected(b"aligned", catalog=FAKE + 8)
    # with N == 0 the limits themselves pass every check and nothing is launched; entries past L are ignored
    for over in (dict(L=1, dims=(72, 0, 0)), dict(L=8, ld=2048, dims=(8, 16, 24, 32, 40, 48, 56, 2048)), dict(dims=(4, 12, 20)),
                 dict(catalog_bf16=1, dims=(8, 16, 24)), dict(L=2, dims=(8, 40, 1)), dict(catalog=None, inv=None)):
        assert fn(ctypes.byref(_norms_args(N=0, **over)), None) == 0, (over, lib.ur_last_error())


def test_select_refuses_invalid_arguments_without_a_gpu():
    lib = _lib.load()
    fn = lib.ur_catalog_funnel_select

    def rejected(word, **over):
        rc = fn(ctypes.byref(_select_args(lib, **over)), None)
        msg = lib.ur_last_error()
        assert rc < 0 and SELECT.encode() in msg and word in msg, (over, rc, msg)

    assert fn(None, None) < 0 and SELECT.encode() in lib.ur_last_error()
    rejected(b"B >= 0", B=-1)
    rejected(b"N", N=-1)
    rejected(b"N", N=1 << 31)
    for dim in (0, 4, 12, -8, 41):
        rejected(b"dim must be", dim=dim)
    rejected(b"dim must be", dim=2056, ld=4096, ldu=4096)
    rejected(b"ld must be at least dim", dim=80)                         # dim > ld
    rejected(b"ld must be at least dim", ld=32)
    rejected(b"ldu must be at least dim", dim=56)                        # dim > ldu (ldu = 48, ld = 72)
    rejected(b"ldu must be at least dim", ldu=36)
    rejected(b"ld must be a multiple of 8", ld=76)                       # ld % 8
    rejected(b"ldu must be a multiple of 4", ldu=42)
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
    for over in (dict(K=1024), dict(K=1), dict(K=129), dict(dim=8), dict(dim=2048, ld=2048, ldu=2048), dict(dim=72, ldu=72), dict(dim=48),
                 dict(ld=40, ldu=40), dict(ldu=44), dict(segments=16), dict(N=0)):
        assert fn(ctypes.byref(_select_args(lib, B=0, **over)), None) == 0, (over, lib.ur_last_error())
    none = {n: None for n in _SELECT_PTRS if n not in ("workspace", "exclude", "gt_index", "rank")}
    assert fn(ctypes.byref(_select_args(lib, B=0, **none)), None) == 0, lib.ur_last_error()


def test_rerank_refuses_invalid_arguments_without_a_gpu():
    lib = _lib.load()
    fn = lib.ur_catalog_funnel_rerank

    def rejected(word, **over):
        rc = fn(ctypes.byref(_rerank_args(lib, **over)), None)
        msg = lib.ur_last_error()
        assert rc < 0 and RERANK.encode() in msg and word in msg, (over, rc, msg)

    assert fn(None, None) < 0 and RERANK.encode() in lib.ur_last_error()
    rejected(b"B >= 0", B=-1)
    rejected(b"N", N=0)
    rejected(b"N", N=1 << 31)
    for dim in (0, 6, -4, 41):
        rejected(b"dim must be", dim=dim)
    rejected(b"dim must be", dim=2052, ld=4096, ldu=4096)
    rejected(b"dim must be", dim=12, catalog_bf16=1)                     # a bf16 catalogue takes multiples of 8
    rejected(b"ld must be", dim=76)                                      # dim > ld
    rejected(b"ld must be", ld=36)
    rejected(b"ld must be", ld=74)
    rejected(b"ld must be", ld=76, catalog_bf16=1)                       # a bf16 row stride takes multiples of 8
    rejected(b"ldu must be", dim=52)                                     # dim > ldu
    rejected(b"ldu must be", ldu=42)
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
    for over in (dict(K_in=1024, k=1024), dict(K_in=1, k=1), dict(K_in=129, k=129), dict(dim=4), dict(dim=2048, ld=2048, ldu=2048, catalog_bf16=1),
                 dict(dim=12), dict(ld=76), dict(dim=48), dict(ld=40, ldu=40)):
        assert fn(ctypes.byref(_rerank_args(lib, B=0, **over)), None) == 0, (over, lib.ur_last_error())


def _pad16(n):
    return (n + 15) // 16 * 16


def _select_need(lib, **over):
    a = _select_args(None, **over)
    a.workspace, a.workspace_bytes = None, -1
    assert lib.ur_catalog_funnel_select(ctypes.byref(a), None) == 0, lib.ur_last_error()
    return a.workspace_bytes


def _rerank_need(lib, **over):
    a = _rerank_args(None, **over)
    a.workspace, a.workspace_bytes = None, -1
    assert lib.ur_catalog_funnel_rerank(ctypes.byref(a), None) == 0, lib.ur_last_error()
    return a.workspace_bytes


def test_size_queries_equal_the_documented_workspaces_and_do_not_launch():
    lib = _lib.load()
    # u~ [B,dim] bf16 | iu~ [B] | ref [B] | chunk [B, rows] f32 | list scores, list indices [B, Gw, K] | counts [B, Gw];
    # Gw = min(max(1024 / B, 1), 8) unless segments names it; rows = chunk_rows or the 64 MB rule, never more than N rounded up to 1024
    def want(B, dim, rows, K, gw):
        return max(16, _pad16(B * dim * 2) + 2 * _pad16(B * 4) + _pad16(B * rows * 4) + 2 * _pad16(B * gw * K * 4) + _pad16(B * gw * 4))
    assert _select_need(lib) == want(3, 40, 1024, 300, 8)
    assert _select_need(lib, chunk_rows=0) == want(3, 40, 2048, 300, 8)
    assert _select_need(lib, segments=1) == want(3, 40, 1024, 300, 1) and _select_need(lib, segments=16) == want(3, 40, 1024, 300, 16)
    # neither stride sizes anything: the catalogue is read in place and the staged user prefix is contiguous
    assert _select_need(lib, ld=2048, ldu=1024) == _select_need(lib) == _select_need(lib, ld=40, ldu=40)
    big = _select_need(lib, B=512, N=1 << 20, dim=256, ld=1024, ldu=1024, K=1024, chunk_rows=0)
    assert big == want(512, 256, (64 << 20) // (4 * 512), 1024, 2) == (1 << 18) + 2 * 2048 + (64 << 20) + 2 * (4 << 20) + 4096
    assert _select_need(lib, B=512, N=1 << 30, dim=256, ld=1024, ldu=1024, K=1024, chunk_rows=0) == big          # nothing of size B x N
    assert big < (1 << 20) * 256 * 2 / 4                                                                   # and no [N, dim] copy
    assert _select_need(lib, B=64, N=1 << 20, dim=256, ld=1024, ldu=1024, K=1000, chunk_rows=0) == want(64, 256, 1 << 18, 1000, 8)
    assert _select_need(lib, B=0) == 16
    # the query needs no pointer at all (and no device), and still refuses what the call refuses, leaving workspace_bytes alone
    a = _select_args(None, E=0, **{n: None for n in _SELECT_PTRS if n != "exclude"})
    a.workspace_bytes = -1
    assert lib.ur_catalog_funnel_select(ctypes.byref(a), None) == 0 and a.workspace_bytes == _select_need(lib, E=0)
    for over, word in ((dict(dim=4), b"dim must be"), (dict(dim=80), b"ld must be at least"), (dict(dim=56), b"ldu must be at least"),
                       (dict(ld=76), b"ld must be a multiple of 8"), (dict(K=1025), b"K must be"), (dict(K=0), b"K must be"),
                       (dict(catalog_bf16=0), b"catalog_bf16"), (dict(chunk_rows=1000), b"chunk_rows"), (dict(segments=17), b"segments")):
        a = _select_args(None, workspace=None, **over)
        a.workspace_bytes = 123
        assert lib.ur_catalog_funnel_select(ctypes.byref(a), None) < 0 and word in lib.ur_last_error() and a.workspace_bytes == 123
    # the re-rank: iu [B] | scores [B, K_in]
    assert _rerank_need(lib) == _pad16(3 * 4) + _pad16(3 * 300 * 4)
    assert _rerank_need(lib, B=512, K_in=1024, k=1000, N=1 << 20, dim=256, ld=1024, ldu=1024) == 2048 + (2 << 20)
    assert _rerank_need(lib, B=5, K_in=1, k=1) == 32 + 32 and _rerank_need(lib, B=0) == 16
    a = _rerank_args(None, **{n: None for n in _RERANK_PTRS})
    a.workspace_bytes = -1
    assert lib.ur_catalog_funnel_rerank(ctypes.byref(a), None) == 0 and a.workspace_bytes == _rerank_need(lib)
    for over, word in ((dict(dim=6), b"dim must be"), (dict(dim=76), b"ld must be"), (dict(dim=52), b"ldu must be"), (dict(K_in=1025), b"K_in must be"),
                       (dict(k=301), b"k must be"), (dict(N=0), b"N")):
        a = _rerank_args(None, workspace=None, **over)
        a.workspace_bytes = 123
        assert lib.ur_catalog_funnel_rerank(ctypes.byref(a), None) < 0 and word in lib.ur_last_error() and a.workspace_bytes == 123


def test_funnel_workspace_layouts_under_the_host_sanitizers(tmp_path):
    """tests/host/catalog_funnel_layout_check.cpp: the two plans over a grid of B, N, dim, K and segments -- regions aligned, disjoint and
    inside the size the query answers, the size the closed form -- as a stand-alone host program under AddressSanitizer and UBSan"""
    # the sanitizer runtimes are linked statically: a dynamic one insists on being the first library the process loads
    gxx, clang = shutil.which("g++"), shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    cxx = [gxx, "-static-libasan", "-static-libubsan"] if gxx else [clang, "-static-libsan"]
    exe = str(tmp_path / "catalog_funnel_layout_check")
    subprocess.run(cxx + ["-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                          "-I", os.path.join(ROOT, "unirec_amd", "csrc"),
                          os.path.join(ROOT, "tests", "host", "catalog_funnel_layout_check.cpp"), "-o", exe], check=True)
    # (the program allocates nothing it does not free at exit; the leak pass needs ptrace, which a sandbox may not grant)
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0 and run.stdout.split() == ["ok", "12600"], (run.returncode, run.stdout, run.stderr)


# ---- the route retrieve_funnel takes, with every device call out of reach --------------------------------------------------------------
class Reached(Exception):
    pass


_WRAPPERS = ("catalog_deep_select", "catalog_select", "catalog_coarse_select", "catalog_rerank", "catalog_scores", "catalog_softmax",
             "catalog_coarse_deep_select", "catalog_deep_rerank", "catalog_prefix_norms", "catalog_funnel_select", "catalog_funnel_rerank")


@pytest.fixture
def routes(monkeypatch):
    """every launch wrapper an evaluator could reach raises Reached(name, arguments); loading the library fails if touched"""
    from unirec_amd import hip

    def raiser(name):
        def touched(*a, **k):
            raise Reached(name, a, k)
        return touched
    for name in _WRAPPERS:
        monkeypatch.setattr(hip, name, raiser(name))
    monkeypatch.setattr(_lib, "load", raiser("_lib.load"))


def _evaluator(dtype=F32, D=64):
    from unirec_amd.evaluation import CatalogEvaluator
    return CatalogEvaluator(torch.arange(200 * D, dtype=F32).reshape(200, D).sin(), device="cpu", dtype=dtype)


@pytest.fixture
def stages(monkeypatch):
    """the three funnel wrappers replaced by recorders that return tensors of the right shapes; the others stay out of reach"""
    from unirec_amd import hip
    calls = []

    def norms(cat, dims):
        calls.append(("norms", tuple(dims)))
        return torch.stack([torch.full((cat.shape[0],), float(d)) for d in dims])

    def select(u, cat, dim, K, inv, gt_index=None, exclude=None, chunk_rows=None):
        calls.append(("select", dim, K, float(inv[0]), gt_index is not None, exclude is not None, chunk_rows))
        rank = None if gt_index is None else torch.ones(u.shape[0], dtype=torch.int32)
        return torch.zeros(u.shape[0], K, dtype=torch.int32), None, rank, inv

    def rerank(u, cat, index, dim, k, inv):
        calls.append(("rerank", dim, tuple(index.shape), k, float(inv[0])))
        return index[:, :k], torch.zeros(u.shape[0], k), inv
    monkeypatch.setattr(hip, "catalog_prefix_norms", norms)
    monkeypatch.setattr(hip, "catalog_funnel_select", select)
    monkeypatch.setattr(hip, "catalog_funnel_rerank", rerank)
    for name in _WRAPPERS[:8]:
        monkeypatch.setattr(hip, name, lambda *a, _n=name, **k: (_ for _ in ()).throw(Reached(_n)))
    return calls


def test_retrieve_funnel_routes_stage_by_stage(stages):
    calls = stages
    ev = _evaluator(BF16)
    u = torch.ones(2, 64)
    out = ev.retrieve_funnel(u, k=5, dims=(8, 32, 64), shortlists=(700, 200), gt_index=[3, 4], exclude=[[1, 2], [5]], ks=(1, 10), chunk_rows=1024)
    # one norm call for the three widths; stage 0 the select at dims[0] with K = shortlists[0], carrying gt_index, exclude and chunk_rows;
    # then the re-ranks at dims[1] down to shortlists[1] and at dims[2] down to k, each with its own plane
    assert calls == [("norms", (8, 32, 64)), ("select", 8, 700, 8.0, True, True, 1024), ("rerank", 32, (2, 700), 200, 32.0),
                     ("rerank", 64, (2, 200), 5, 64.0)]
    assert out["topk_index"].shape == (2, 5) and out["rank_is_coarse"] is True and out["rank_dim"] == 8 and out["mrr"] == 1.0
    assert out["hit_at"] == {1: 1.0, 10: 1.0} and set(out["ndcg_at"]) == {1, 10}
    assert sorted(ev._prefix_inv) == [8, 32] and float(ev._inv[0]) == 64.0            # the plane of width D is the evaluator's own
    # the planes are requested once per dim: a second call asks for nothing, a new width for itself alone
    del calls[:]
    out = ev.retrieve_funnel(u, k=5, dims=(8, 64))
    assert calls == [("select", 8, 128, 8.0, False, False, None), ("rerank", 64, (2, 128), 5, 64.0)]
    assert sorted(out) == ["topk_index", "topk_score"]
    del calls[:]
    ev.retrieve_funnel(u, k=5, dims=(8, 16, 32, 64))
    assert calls[0] == ("norms", (16,)) and [c[0] for c in calls[1:]] == ["select", "rerank", "rerank", "rerank"]
    # norms that retrieve() left behind are the plane of width D
    ev = _evaluator(BF16)
    ev._inv = torch.full((200,), -1.0)
    del calls[:]
    ev.retrieve_funnel(u, k=5, dims=(8, 64))
    assert calls == [("norms", (8,)), ("select", 8, 128, 8.0, False, False, None), ("rerank", 64, (2, 128), 5, -1.0)]
    # the last width may stop short of D
    del calls[:]
    ev.retrieve_funnel(u, k=3, dims=(16, 32), shortlists=[10])
    assert calls == [("norms", (16, 32)), ("select", 16, 10, 16.0, False, False, None), ("rerank", 32, (2, 10), 3, 32.0)]


def test_retrieve_funnel_default_shortlists(stages):
    calls = stages
    ev = _evaluator(BF16)
    u = torch.ones(2, 64)
    for k, S in ((1, 128), (10, 128), (64, 128), (65, 130), (500, 1000), (513, 1024), (1024, 1024)):
        del calls[:]
        ev.retrieve_funnel(u, k=k, dims=(8, 32, 64))
        got = [c for c in calls if c[0] != "norms"]
        assert got == [("select", 8, S, 8.0, False, False, None), ("rerank", 32, (2, S), S, 32.0), ("rerank", 64, (2, S), k, 64.0)], (k, got)
    assert "NOT a tuned value" in type(ev).retrieve_funnel.__doc__


def test_retrieve_funnel_refuses_before_any_device_call(routes):
    u = torch.ones(2, 64)
    ev = _evaluator(BF16)
    for kw in (dict(k=0), dict(k=-1), dict(k=1025), dict(k=10.0), dict(k="10"), dict(k=True), dict(k=None)):
        with pytest.raises(ValueError, match="retrieve_funnel: k must be an int in"):
            ev.retrieve_funnel(u, dims=(8, 64), **kw)
    for dims in (None, (64,), (8, 8, 64), (32, 8), (8, 72), (8, 12, 64), (4, 64), (8.0, 64), (True, 64), "ab", 8, (0, 64),
                 (8, 16, 24, 32, 40, 48, 56, 60, 64)):
        with pytest.raises(ValueError, match="retrieve_funnel: dims"):
            ev.retrieve_funnel(u, k=5, dims=dims)
    for sl in ((), (128, 128), (4,), (1025,), (128.0,), (True,), 128, ("128",)):
        with pytest.raises(ValueError, match="retrieve_funnel: shortlists"):
            ev.retrieve_funnel(u, k=5, dims=(8, 64), shortlists=sl)
    for sl in ((100, 200), (4, 4), (200,), (200, 100, 50)):
        with pytest.raises(ValueError, match="retrieve_funnel: shortlists"):
            ev.retrieve_funnel(u, k=5, dims=(8, 32, 64), shortlists=sl)
    # an f32 catalogue: the message retrieve_two_stage gives
    with pytest.raises(ValueError) as funnel:
        _evaluator(F32).retrieve_funnel(u, k=10, dims=(8, 64))
    with pytest.raises(ValueError) as two:
        _evaluator(F32).retrieve_two_stage(u, k=10, shortlist=300)
    assert str(funnel.value) == str(two.value) and "bf16 catalogue" in str(funnel.value)
    # accepted arguments reach the norms first
    with pytest.raises(Reached) as hit:
        ev.retrieve_funnel(u, k=5, dims=(8, 64), shortlists=(5,))
    assert hit.value.args[0] == "catalog_prefix_norms" and hit.value.args[1][1] == (8, 64)


def test_the_older_evaluator_paths_keep_their_routes(routes):
    u = torch.ones(2, 64)
    for dtype in (F32, BF16):
        ev = _evaluator(dtype)
        for kw, name in ((dict(k=129), "catalog_deep_select"), (dict(k=1024), "catalog_deep_select"), (dict(k=128), "catalog_select"),
                         (dict(), "catalog_select")):
            with pytest.raises(Reached) as hit:
                ev.retrieve(u, **kw)
            assert hit.value.args[0] == name
    ev = _evaluator(BF16)
    with pytest.raises(Reached) as hit:
        ev.retrieve(u, k=10, shortlist=128)
    assert hit.value.args[0] == "catalog_coarse_select"
    with pytest.raises(Reached) as hit:
        ev.retrieve_two_stage(u, k=10, shortlist=300)
    assert hit.value.args[0] == "catalog_coarse_deep_select" and hit.value.args[1][2] == 300
    t = ev.truncated(32)                              # still a contiguous copy with norms of its own
    assert t.catalog.shape == (200, 32) and t.catalog.is_contiguous() and t._inv is None and t._prefix_inv == {}
    assert t.catalog.data_ptr() != ev.catalog.data_ptr()
    with pytest.raises(Reached) as hit:
        t.retrieve_two_stage(u[:, :32], k=10)
    assert hit.value.args[0] == "catalog_coarse_deep_select" and hit.value.args[1][1] is t.catalog


def test_wrappers_refuse_before_the_library():
    from unirec_amd import hip
    u = torch.zeros(2, 16)
    index = torch.zeros(2, 300, dtype=torch.int32)
    with pytest.raises(_lib.UniRecHipError, match="no CPU fallback"):
        hip.catalog_funnel_select(u, torch.zeros(5, 16, dtype=BF16), 8, 300)
    with pytest.raises(ValueError, match="catalog_funnel_select.*bf16 catalogue"):
        hip.catalog_funnel_select(u, torch.zeros(5, 16), 8, 300)
    with pytest.raises(ValueError, match="catalog_funnel_select.*prefix dim = 24"):
        hip.catalog_funnel_select(u, torch.zeros(5, 32, dtype=BF16), 24, 300)
    with pytest.raises(ValueError, match="catalog_funnel_select: dim must be an int"):
        hip.catalog_funnel_select(u, torch.zeros(5, 32, dtype=BF16), 8.0, 300)
    with pytest.raises(_lib.UniRecHipError, match="no CPU fallback"):
        hip.catalog_funnel_rerank(u, torch.zeros(5, 16), index, 8)
    with pytest.raises(ValueError, match="catalog_funnel_rerank.*f32 or bf16"):
        hip.catalog_funnel_rerank(u, torch.zeros(5, 16, dtype=torch.float16), index, 8)
    with pytest.raises(ValueError, match="catalog_funnel_rerank.*prefix dim = 24"):
        hip.catalog_funnel_rerank(u, torch.zeros(5, 32), index, 24)
    with pytest.raises(_lib.UniRecHipError, match="no CPU fallback"):
        hip.catalog_prefix_norms(torch.zeros(5, 16), (4, 8))
    with pytest.raises(ValueError, match="multiple of 8 for a bf16 catalogue"):
        hip.catalog_prefix_norms(torch.zeros(5, 16, dtype=BF16), (4, 8))
    for dims in ((8, 4), (8, 8), (), (0, 8), (6,), (8.0,), tuple(range(4, 40, 4))):
        with pytest.raises(ValueError, match="dims"):
            hip.catalog_prefix_norms(torch.zeros(5, 16), dims)
    with pytest.raises(ValueError, match="at most the catalogue width 16"):
        hip.catalog_prefix_norms(torch.zeros(5, 16), (8, 20))

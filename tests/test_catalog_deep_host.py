"""CPU: the host side of the long-list retrieval family -- the rules include/unirec_hip_deep.h is held to (declared <=> exported <=>
bound, a name in one header only, the ctypes mirror of its struct field for field, the entry point named in the COVERS dict of
tests/test_gpu_catalog_deep.py), every refusal of the entry point and its size query through the raw library (fake non-null pointers:
each call returns before any launch), and the route CatalogEvaluator.retrieve(k=...) takes with every device call out of reach."""
import ast
import ctypes
import os
import re

import pytest
import torch

from unirec_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "unirec_hip_deep.h")
GPU_TESTS = "tests/test_gpu_catalog_deep.py"
OTHER_HEADERS = ("unirec_hip.h", "unirec_hip_loss.h", "unirec_hip_adapter.h", "unirec_hip_pool.h", "unirec_hip_mrl.h", "unirec_hip_coarse.h")
ENTRY = "ur_catalog_deep_select"
FAKE = 1 << 20          # non-null, 16-byte aligned, never dereferenced on the host
MB = 1 << 24
F32, BF16 = torch.float32, torch.bfloat16


# ---- the header: declared <=> exported <=> bound, the struct mirror, a test per entry point ----------------------------------------------
def _source(header=HEADER):
    return re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)


def _declared(header=HEADER):
    return sorted(set(re.findall(r"\b(ur_[a-z0-9_]+)\s*\(", _source(header))))


def test_deep_header_symbols_are_bound_and_exported():
    names = _declared()
    assert names == [ENTRY]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, ENTRY), f"{ENTRY} declared in unirec_hip_deep.h but not exported by libunirec_hip.so"
    assert sorted(_lib.DEEP_SIGNATURES) == names, "declared <=> bound in unirec_amd/_lib.py"
    others = set(_lib.SIGNATURES) | set(_lib.LOSS_SIGNATURES) | set(_lib.ADAPTER_SIGNATURES) | set(_lib.POOL_SIGNATURES) | \
        set(_lib.MRL_SIGNATURES) | set(_lib.COARSE_SIGNATURES)
    assert not set(_lib.DEEP_SIGNATURES) & others, "a name belongs to one header"
    for other in OTHER_HEADERS:
        assert ENTRY not in _declared(os.path.join(ROOT, "include", other)), f"{other} declares the deep entry point"
    loaded = _lib.load()
    assert getattr(loaded, ENTRY).argtypes == _lib.DEEP_SIGNATURES[ENTRY][1], f"load() did not bind {ENTRY}"
    assert getattr(loaded, ENTRY).restype == _lib.DEEP_SIGNATURES[ENTRY][0]
    assert _lib.ABI_VERSION >= 26 and loaded.ur_version() == _lib.ABI_VERSION      # (the deep header arrived with ABI 26)


def test_header_constants_match_the_binding():
    from unirec_amd import hip
    consts = {k: int(v) for k, v in re.findall(r"#define (UR_CATALOG_DEEP_[A-Z_]+) (\d+)", open(HEADER).read())}
    assert consts == {"UR_CATALOG_DEEP_TOPK_MAX": _lib.CATALOG_DEEP_TOPK_MAX, "UR_CATALOG_DEEP_SEGMENTS_MAX": _lib.CATALOG_DEEP_SEGMENTS_MAX}
    assert consts["UR_CATALOG_DEEP_TOPK_MAX"] == hip.CATALOG_DEEP_TOPK_MAX == 1024
    assert hip.CATALOG_TOPK_MAX == 128                                          # the old limit stands beside it


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


def test_struct_mirror_matches_the_header_field_for_field():
    structs = _header_structs()
    assert sorted(structs) == ["ur_catalog_deep_t"]
    fields = structs["ur_catalog_deep_t"]
    want = type("FromHeader", (ctypes.Structure,), {"_fields_": fields})
    got = _lib.CatalogDeep
    assert [f[0] for f in got._fields_] == [f[0] for f in fields], "field names and order"
    assert ctypes.sizeof(got) == ctypes.sizeof(want)
    for (name, t), (_, tw) in zip(got._fields_, fields):
        assert getattr(got, name).offset == getattr(want, name).offset, name
        assert t is tw, f"{name}: {t} against the header's {tw}"
    # what ur_catalog_coarse_t carries, plus scorer (and the test-only segments)
    assert set(f[0] for f in _lib.CatalogCoarse._fields_) | {"scorer", "segments"} == set(f[0] for f in fields)


def test_the_entry_point_is_listed_in_the_gpu_file():
    with open(os.path.join(ROOT, GPU_TESTS)) as f:
        tree = ast.parse(f.read())
    covers = None
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "COVERS" for t in node.targets):
            covers = ast.literal_eval(node.value)
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    assert isinstance(covers, dict), f"{GPU_TESTS} has no top-level COVERS dict"
    assert sorted(covers) == _declared(), "COVERS lists exactly the entry point of unirec_hip_deep.h"
    assert covers[ENTRY] and all(name in tests for name in covers[ENTRY]), covers


# ---- every refusal, without a GPU --------------------------------------------------------------------------------------------------------
_PTRS = ("user", "catalog", "cat_inv_norm", "topk_index", "topk_score", "gt_index", "rank", "exclude", "workspace")


def _args(lib=None, **over):
    """a valid argument struct over fake pointers (B 3, N 2000, D 40, K 300), with `over` applied; the workspace is sized by the size
    query of the call's own sizes unless `workspace_bytes` is given"""
    a = _lib.CatalogDeep()
    names = [f[0] for f in a._fields_]
    for i, n in enumerate(_PTRS):
        setattr(a, n, FAKE + i * MB)
    a.B, a.N, a.D, a.K, a.E, a.chunk_rows = 3, 2000, 40, 300, 5, 1024
    explicit_ws = "workspace_bytes" in over
    for k, v in over.items():
        assert k in names, k
        setattr(a, k, v)
    if lib is not None and not explicit_ws:
        q = _lib.CatalogDeep()
        ctypes.memmove(ctypes.byref(q), ctypes.byref(a), ctypes.sizeof(a))
        q.workspace = None
        a.workspace_bytes = q.workspace_bytes if lib.ur_catalog_deep_select(ctypes.byref(q), None) == 0 else 1 << 40
    return a


def test_invalid_arguments_are_rejected_without_a_gpu():
    lib = _lib.load()
    fn = lib.ur_catalog_deep_select

    def rejected(word, **over):
        rc = fn(ctypes.byref(_args(lib, **over)), None)
        msg = lib.ur_last_error()
        assert rc < 0 and ENTRY.encode() in msg and word in msg, (over, rc, msg)

    assert fn(None, None) < 0 and ENTRY.encode() in lib.ur_last_error()
    rejected(b"B >= 0", B=-1)
    rejected(b"N", N=-1)
    rejected(b"N", N=1 << 31)
    for D in (0, 6, 2052, -4, 41, 4096):
        rejected(b"D must be", D=D)
    for K in (0, -1, 1025):
        rejected(b"K must be", K=K)
    rejected(b"chunk_rows", chunk_rows=1000)
    rejected(b"chunk_rows", chunk_rows=-1024)
    rejected(b"exclude", exclude=None)                                   # E = 5 with a null exclude
    rejected(b"gt_index and rank", rank=None)
    rejected(b"gt_index and rank", gt_index=None)
    for flag in (2, -1):
        rejected(b"catalog_bf16", catalog_bf16=flag)
    for scorer in (3, -1):
        rejected(b"scorer", scorer=scorer)
    for segments in (-1, 17):
        rejected(b"segments", segments=segments)
    for name in ("topk_index", "topk_score", "user", "catalog", "cat_inv_norm"):
        rejected(b"null", **{name: None})
    for name in ("user", "catalog"):
        rejected(b"aligned", **{name: FAKE + 20 * MB + 8})
    need = _args(lib).workspace_bytes
    assert need > 0
    rejected(b"workspace", workspace_bytes=need - 1)
    rejected(b"workspace", workspace=FAKE + 21 * MB + 4)
    # the limits themselves pass every check up to the pointers: K = 1024, D = 4 and 2048, both dtypes and every scorer, with B == 0
    for over in (dict(K=1024), dict(K=1), dict(D=4), dict(D=2048), dict(catalog_bf16=1, scorer=2), dict(scorer=1), dict(segments=16)):
        assert fn(ctypes.byref(_args(lib, B=0, **over)), None) == 0, (over, lib.ur_last_error())
    # nothing to do: 0, nothing launched -- even with no buffers at all
    none = {n: None for n in _PTRS if n not in ("workspace", "exclude", "gt_index", "rank")}
    assert fn(ctypes.byref(_args(lib, B=0, **none)), None) == 0, lib.ur_last_error()


def _need(lib, **over):
    a = _args(None, **over)
    a.workspace, a.workspace_bytes = None, -1
    assert lib.ur_catalog_deep_select(ctypes.byref(a), None) == 0, lib.ur_last_error()
    return a.workspace_bytes


def _pad16(n):
    return (n + 15) // 16 * 16


def test_size_query_holds_nothing_of_size_b_times_n_and_does_not_launch():
    lib = _lib.load()
    # chunk [B, rows] f32 | ref [B] | 1/|u| [B] | list scores, list indices [B, Gw, K] | counts [B, Gw]; Gw = min(max(1024 / B, 1), 8)
    # unless segments names it; rows = chunk_rows or the 64 MB rule, never more than N rounded up to 1024
    def want(B, rows, K, gw):
        return max(16, _pad16(B * rows * 4) + 2 * _pad16(B * 4) + 2 * _pad16(B * gw * K * 4) + _pad16(B * gw * 4))
    assert _need(lib) == want(3, 1024, 300, 8)
    assert _need(lib, chunk_rows=0) == want(3, 2048, 300, 8)
    assert _need(lib, segments=1) == want(3, 1024, 300, 1) and _need(lib, segments=16) == want(3, 1024, 300, 16)
    big = _need(lib, B=512, N=1 << 30, D=1024, K=1024, chunk_rows=0)
    assert big == want(512, (64 << 20) // (4 * 512), 1024, 2) == (64 << 20) + 2 * 2048 + 2 * (4 << 20) + 4096     # 72 MB for 2^39 scores
    assert _need(lib, B=512, N=1 << 20, D=1024, K=1024, chunk_rows=0) == big                                       # N is not in it
    assert _need(lib, B=64, N=1 << 20, D=1024, K=1000, chunk_rows=0) == want(64, 1 << 18, 1000, 8)
    assert _need(lib, B=2000, N=1 << 20, D=8, K=129, chunk_rows=2048) == want(2000, 2048, 129, 1)
    assert _need(lib, B=0) == 16
    # the query needs no pointer at all (and no device: this machine may have none), and still refuses what the call refuses
    a = _args(None, E=0, **{n: None for n in _PTRS if n != "exclude"})
    a.workspace_bytes = -1
    assert lib.ur_catalog_deep_select(ctypes.byref(a), None) == 0 and a.workspace_bytes == _need(lib, E=0)
    for over, word in ((dict(D=6), b"D must be"), (dict(K=1025), b"K must be"), (dict(K=0), b"K must be"), (dict(catalog_bf16=2), b"catalog_bf16"),
                       (dict(scorer=3), b"scorer"), (dict(chunk_rows=1000), b"chunk_rows"), (dict(segments=17), b"segments")):
        a = _args(None, workspace=None, **over)
        a.workspace_bytes = 123
        assert lib.ur_catalog_deep_select(ctypes.byref(a), None) < 0 and word in lib.ur_last_error() and a.workspace_bytes == 123


# ---- the route retrieve(k=...) takes, with every device call out of reach ------------------------------------------------------------------
class Reached(Exception):
    pass


@pytest.fixture
def routes(monkeypatch):
    """every launch wrapper retrieve() could reach raises Reached(its name); loading the library fails if touched"""
    from unirec_amd import hip

    def raiser(name):
        def touched(*a, **k):
            raise Reached(name)
        return touched
    for name in ("catalog_deep_select", "catalog_select", "catalog_coarse_select", "catalog_rerank", "catalog_scores", "catalog_softmax"):
        monkeypatch.setattr(hip, name, raiser(name))
    monkeypatch.setattr(_lib, "load", raiser("_lib.load"))


def _evaluator(dtype=F32):
    from unirec_amd.evaluation import CatalogEvaluator
    return CatalogEvaluator(torch.arange(200 * 16, dtype=F32).reshape(200, 16).sin(), device="cpu", dtype=dtype)


def test_retrieve_routes_by_k(routes):
    u = torch.ones(2, 16)
    for dtype in (F32, BF16):
        ev = _evaluator(dtype)
        for kw in (dict(k=129), dict(k=1024), dict(k=300, exclude=[[1, 2], [5]], gt_index=torch.tensor([3, 4])), dict(k=1000, scorer="mfma")):
            with pytest.raises(Reached, match="^catalog_deep_select$"):
                ev.retrieve(u, **kw)
        for kw in (dict(k=128), dict(k=1), dict(), dict(k=10, exclude=[[1, 2], [5]], gt_index=torch.tensor([3, 4]))):
            with pytest.raises(Reached, match="^catalog_select$"):
                ev.retrieve(u, **kw)
        for bad in (0, -1, 1025, 200.0, "200", True, None, (200,)):
            with pytest.raises(ValueError, match=r"\bk\b.*1024"):                  # names k and the limit; no device call (not Reached)
                ev.retrieve(u, k=bad)
    # a shortlist lies in [k, 128]: k > 128 with one is refused by the shortlist rule, and the two-stage route is where it was
    ev = _evaluator(BF16)
    with pytest.raises(ValueError, match="shortlist must be an int in"):
        ev.retrieve(u, k=200, shortlist=128)
    with pytest.raises(Reached, match="^catalog_coarse_select$"):
        ev.retrieve(u, k=10, shortlist=128)


def test_wrapper_refuses_before_the_library():
    from unirec_amd import hip
    u = torch.zeros(2, 16)
    with pytest.raises(_lib.UniRecHipError, match="no CPU fallback"):
        hip.catalog_deep_select(u, torch.zeros(5, 16), 300)
    with pytest.raises(ValueError, match="f32 or bf16"):
        hip.catalog_deep_select(u, torch.zeros(5, 16, dtype=torch.float16), 300)
    with pytest.raises(ValueError, match="scorer"):
        hip.catalog_deep_select(u, torch.zeros(5, 16), 300, scorer="bf16")

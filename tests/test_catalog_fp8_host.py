"""CPU: the host side of the FP8 catalogue family -- the rules include/unirec_fp8.h is held to (declared <=> exported <=> bound, a name
in one header only, the ctypes mirrors of its structs field for field, the three entry points named in the COVERS dict of
tests/test_gpu_catalog_fp8.py: the rule of tests/test_abi_test_coverage.py, which globs include/unirec_hip*.h, applied to this header),
every refusal of the three entry points and of the two size queries through the raw library (fake non-null pointers: each call returns
before any launch), the size queries against the closed forms the header documents, the reference tests/catalog_fp8_ref.py on its own
(decode table against torch's view, encode(decode(c)) == c, the frexp rule against a search at the boundary mantissas), the workspace
plans and the codec under the host sanitizers, and the route Fp8CatalogEvaluator takes with every device call out of reach."""
import ast
import ctypes
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import catalog_fp8_ref as ref
from unirec_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "unirec_fp8.h")
GPU_TESTS = "tests/test_gpu_catalog_fp8.py"
QUANTIZE, SELECT, RERANK = "ur_catalog_fp8_quantize", "ur_catalog_fp8_select", "ur_catalog_fp8_rerank"
FAKE = 1 << 20          # non-null, 16-byte aligned, never dereferenced on the host
MB = 1 << 24
F32, BF16 = torch.float32, torch.bfloat16


# ---- the header: declared <=> exported <=> bound, the struct mirrors, a test per entry point ---------------------------------------------
def _source(header=HEADER):
    return re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)


def _declared(header=HEADER):
    return sorted(set(re.findall(r"\b(ur_[a-z0-9_]+)\s*\(", _source(header))))


def test_fp8_header_symbols_are_bound_and_exported():
    names = _declared()
    assert names == sorted([QUANTIZE, SELECT, RERANK])
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        assert hasattr(lib, name), f"{name} declared in unirec_fp8.h but not exported by libunirec_hip.so"
    assert sorted(_lib.FP8_SIGNATURES) == names, "declared <=> bound in unirec_amd/_lib.py"
    others = set(_lib.SIGNATURES) | set(_lib.LOSS_SIGNATURES) | set(_lib.ADAPTER_SIGNATURES) | set(_lib.POOL_SIGNATURES) | \
        set(_lib.MRL_SIGNATURES) | set(_lib.COARSE_SIGNATURES) | set(_lib.DEEP_SIGNATURES) | set(_lib.COARSE_DEEP_SIGNATURES) | \
        set(_lib.FUNNEL_SIGNATURES) | set(_lib.MRL_LOSS_SIGNATURES)
    assert not set(_lib.FP8_SIGNATURES) & others, "a name belongs to one header"
    older = sorted(glob.glob(os.path.join(ROOT, "include", "unirec_hip*.h")))
    assert len(older) >= 10 and HEADER not in older
    for other in older:
        assert not set(names) & set(_declared(other)), f"{other} declares an entry point of this family"
    loaded = _lib.load()
    for name in names:
        assert getattr(loaded, name).argtypes == _lib.FP8_SIGNATURES[name][1], f"load() did not bind {name}"
        assert getattr(loaded, name).restype == _lib.FP8_SIGNATURES[name][0]
    assert _lib.ABI_VERSION >= 30 and loaded.ur_version() == _lib.ABI_VERSION      # (this header arrived with ABI 30)
    # the older retrieval families keep exactly their entry points
    assert sorted(_lib.COARSE_DEEP_SIGNATURES) == ["ur_catalog_coarse_deep_select", "ur_catalog_deep_rerank"]
    assert sorted(_lib.FUNNEL_SIGNATURES) == ["ur_catalog_funnel_rerank", "ur_catalog_funnel_select", "ur_catalog_prefix_norms"]
    defines = dict(re.findall(r"#define (UR_FP8_\w+) (\d+)", _source()))
    assert defines == {"UR_FP8_USER_GROUP": str(_lib.FP8_USER_GROUP)}


_CTYPE = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "uint8_t": ctypes.c_uint8}


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
    assert sorted(structs) == ["ur_catalog_fp8_quantize_t", "ur_catalog_fp8_rerank_t", "ur_catalog_fp8_select_t"]
    for typedef, got in (("ur_catalog_fp8_quantize_t", _lib.CatalogFp8Quantize), ("ur_catalog_fp8_select_t", _lib.CatalogFp8Select),
                         ("ur_catalog_fp8_rerank_t", _lib.CatalogFp8Rerank)):
        fields = structs[typedef]
        want = type("FromHeader", (ctypes.Structure,), {"_fields_": fields})
        assert [f[0] for f in got._fields_] == [f[0] for f in fields], f"{typedef}: field names and order"
        assert ctypes.sizeof(got) == ctypes.sizeof(want)
        for (name, t), (_, tw) in zip(got._fields_, fields):
            assert getattr(got, name).offset == getattr(want, name).offset, (typedef, name)
            assert t is tw, f"{typedef}.{name}: {t} against the header's {tw}"

    # the fields of ur_catalog_coarse_deep_t / ur_catalog_deep_rerank_t with codes for catalog and without the two flags: the norm plane
    # is always an input here
    def fp8_form(cls):
        return ["codes" if n == "catalog" else n for n, _ in cls._fields_ if n not in ("catalog_bf16", "cat_norm_ready")]
    assert [f[0] for f in _lib.CatalogFp8Select._fields_] == fp8_form(_lib.CatalogCoarseDeep)
    assert [f[0] for f in _lib.CatalogFp8Rerank._fields_] == fp8_form(_lib.CatalogDeepRerank)


def test_the_three_entry_points_are_listed_in_the_gpu_file():
    with open(os.path.join(ROOT, GPU_TESTS)) as f:
        tree = ast.parse(f.read())
    covers = None
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "COVERS" for t in node.targets):
            covers = ast.literal_eval(node.value)
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    assert isinstance(covers, dict), f"{GPU_TESTS} has no top-level COVERS dict"
    assert sorted(covers) == _declared(), "COVERS lists exactly the three entry points of unirec_fp8.h"
    for entry in covers:
        assert covers[entry] and all(name in tests for name in covers[entry]), covers


# ---- every refusal, without a GPU --------------------------------------------------------------------------------------------------------
_QUANTIZE_PTRS = ("src", "codes", "scale", "inv")
_SELECT_PTRS = ("user", "codes", "cat_inv_norm", "topk_index", "topk_score", "gt_index", "rank", "exclude", "workspace")
_RERANK_PTRS = ("user", "codes", "cat_inv_norm", "index", "topk_index", "topk_score", "workspace")


def _args(cls, fn, ptrs, sizes, query, over):
    """a valid argument struct over fake pointers with `over` applied; the workspace is sized by the size query of the call's own sizes
    (query=True) unless `workspace_bytes` is given"""
    a = cls()
    names = [f[0] for f in a._fields_]
    for i, n in enumerate(ptrs):
        setattr(a, n, FAKE + i * MB)
    for k, v in {**sizes, **over}.items():
        assert k in names, k
        setattr(a, k, v)
    if query and "workspace_bytes" not in over:
        q = cls()
        ctypes.memmove(ctypes.byref(q), ctypes.byref(a), ctypes.sizeof(a))
        q.workspace = None
        a.workspace_bytes = q.workspace_bytes if fn(ctypes.byref(q), None) == 0 else 1 << 40
    return a


def _quantize_args(**over):
    """N 2000, D 48 of ld 60, f32"""
    return _args(_lib.CatalogFp8Quantize, None, _QUANTIZE_PTRS, dict(N=2000, D=48, ld=60), False, over)


def _select_args(lib=None, **over):
    """B 3, N 2000, D 48, K 300, E 5, chunk_rows 1024"""
    return _args(_lib.CatalogFp8Select, lib and lib.ur_catalog_fp8_select, _SELECT_PTRS,
                 dict(B=3, N=2000, D=48, K=300, E=5, chunk_rows=1024), lib is not None, over)


def _rerank_args(lib=None, **over):
    """B 3, N 2000, D 48, K_in 300, k 200"""
    return _args(_lib.CatalogFp8Rerank, lib and lib.ur_catalog_fp8_rerank, _RERANK_PTRS, dict(B=3, N=2000, D=48, K_in=300, k=200),
                 lib is not None, over)


def test_quantize_refuses_invalid_arguments_without_a_gpu():
    lib = _lib.load()
    fn = lib.ur_catalog_fp8_quantize

    def rejected(word, **over):
        rc = fn(ctypes.byref(_quantize_args(**over)), None)
        msg = lib.ur_last_error()
        assert rc < 0 and QUANTIZE.encode() in msg and word in msg, (over, rc, msg)

    assert fn(None, None) < 0 and QUANTIZE.encode() in lib.ur_last_error()
    for flag in (2, -1):
        rejected(b"src_bf16", src_bf16=flag)
    rejected(b"N", N=-1)
    rejected(b"N", N=1 << 31)
    for D in (0, 8, 24, -16, 2064):
        rejected(b"D must be", D=D, ld=4096)
    for ld in (0, 44, 50, -60):
        rejected(b"ld must be", ld=ld)
    for name in _QUANTIZE_PTRS:
        rejected(b"null", **{name: None})
    for name in ("src", "codes"):
        rejected(b"aligned", **{name: FAKE + 20 * MB + 8})
    # with N == 0 the limits themselves pass every check and nothing is launched
    for over in (dict(D=16, ld=16), dict(D=2048, ld=2048), dict(ld=48), dict(src_bf16=1), dict(src=None, codes=None, scale=None, inv=None)):
        assert fn(ctypes.byref(_quantize_args(N=0, **over)), None) == 0, (over, lib.ur_last_error())


def test_select_refuses_invalid_arguments_without_a_gpu():
    lib = _lib.load()
    fn = lib.ur_catalog_fp8_select

    def rejected(word, **over):
        rc = fn(ctypes.byref(_select_args(lib, **over)), None)
        msg = lib.ur_last_error()
        assert rc < 0 and SELECT.encode() in msg and word in msg, (over, rc, msg)

    assert fn(None, None) < 0 and SELECT.encode() in lib.ur_last_error()
    rejected(b"B >= 0", B=-1)
    rejected(b"N", N=-1)
    rejected(b"N", N=1 << 31)
    for D in (0, 8, 24, 40, -16, 2064):
        rejected(b"D must be a positive multiple of 16", D=D)
    for K in (0, -1, 1025):
        rejected(b"K must be", K=K)
    rejected(b"chunk_rows", chunk_rows=1000)
    rejected(b"chunk_rows", chunk_rows=-1024)
    rejected(b"exclude", exclude=None)                                   # E = 5 with a null exclude
    rejected(b"gt_index and rank", rank=None)
    rejected(b"gt_index and rank", gt_index=None)
    for segments in (-1, 17):
        rejected(b"segments", segments=segments)
    for name in ("topk_index", "topk_score", "user", "codes", "cat_inv_norm"):
        rejected(b"null", **{name: None})
    for name in ("user", "codes"):
        rejected(b"aligned", **{name: FAKE + 20 * MB + 8})
    need = _select_args(lib).workspace_bytes
    assert need > 0
    rejected(b"workspace", workspace_bytes=need - 1)
    rejected(b"workspace", workspace=FAKE + 21 * MB + 4)
    # the limits themselves pass every check up to the pointers, with B == 0
    for over in (dict(K=1024), dict(K=1), dict(K=129), dict(D=16), dict(D=2048), dict(segments=16), dict(N=0)):
        assert fn(ctypes.byref(_select_args(lib, B=0, **over)), None) == 0, (over, lib.ur_last_error())
    none = {n: None for n in _SELECT_PTRS if n not in ("workspace", "exclude", "gt_index", "rank")}
    assert fn(ctypes.byref(_select_args(lib, B=0, **none)), None) == 0, lib.ur_last_error()


def test_rerank_refuses_invalid_arguments_without_a_gpu():
    lib = _lib.load()
    fn = lib.ur_catalog_fp8_rerank

    def rejected(word, **over):
        rc = fn(ctypes.byref(_rerank_args(lib, **over)), None)
        msg = lib.ur_last_error()
        assert rc < 0 and RERANK.encode() in msg and word in msg, (over, rc, msg)

    assert fn(None, None) < 0 and RERANK.encode() in lib.ur_last_error()
    rejected(b"B >= 0", B=-1)
    rejected(b"N", N=0)
    rejected(b"N", N=1 << 31)
    for D in (0, 8, 24, -16, 2064):
        rejected(b"D must be", D=D)
    for K_in in (0, -1, 1025):
        rejected(b"K_in must be", K_in=K_in, k=1)
    for k in (0, -1, 301):
        rejected(b"k must be", k=k)
    for name in ("index", "topk_index", "topk_score", "user", "codes", "cat_inv_norm"):
        rejected(b"null", **{name: None})
    for name in ("user", "codes"):
        rejected(b"aligned", **{name: FAKE + 20 * MB + 8})
    need = _rerank_args(lib).workspace_bytes
    assert need > 0
    rejected(b"workspace", workspace_bytes=need - 1)
    rejected(b"workspace", workspace=FAKE + 21 * MB + 4)
    for over in (dict(K_in=1024, k=1024), dict(K_in=1, k=1), dict(K_in=129, k=129), dict(D=16), dict(D=2048)):
        assert fn(ctypes.byref(_rerank_args(lib, B=0, **over)), None) == 0, (over, lib.ur_last_error())


def _pad16(n):
    return (n + 15) // 16 * 16


def _select_need(lib, **over):
    a = _select_args(None, **over)
    a.workspace, a.workspace_bytes = None, -1
    assert lib.ur_catalog_fp8_select(ctypes.byref(a), None) == 0, lib.ur_last_error()
    return a.workspace_bytes


def _rerank_need(lib, **over):
    a = _rerank_args(None, **over)
    a.workspace, a.workspace_bytes = None, -1
    assert lib.ur_catalog_fp8_rerank(ctypes.byref(a), None) == 0, lib.ur_last_error()
    return a.workspace_bytes


def test_size_queries_equal_the_documented_workspaces_and_do_not_launch():
    lib = _lib.load()
    # q [B,D] bytes | iu8 [B] | user scales [B] | ref [B] | chunk [B, rows] f32 | list scores, list indices [B, Gw, K] | counts [B, Gw];
    # Gw = min(max(1024 / B, 1), 8) unless segments names it; rows = chunk_rows or the 64 MB rule, never more than N rounded up to 1024
    def want(B, D, rows, K, gw):
        return max(16, _pad16(B * D) + 3 * _pad16(B * 4) + _pad16(B * rows * 4) + 2 * _pad16(B * gw * K * 4) + _pad16(B * gw * 4))
    assert _select_need(lib) == want(3, 48, 1024, 300, 8)
    assert _select_need(lib, chunk_rows=0) == want(3, 48, 2048, 300, 8)
    assert _select_need(lib, segments=1) == want(3, 48, 1024, 300, 1) and _select_need(lib, segments=16) == want(3, 48, 1024, 300, 16)
    big = _select_need(lib, B=512, N=1 << 20, D=1024, K=1024, chunk_rows=0)
    assert big == want(512, 1024, (64 << 20) // (4 * 512), 1024, 2) == (1 << 19) + 3 * 2048 + (64 << 20) + 2 * (4 << 20) + 4096
    assert _select_need(lib, B=512, N=1 << 30, D=1024, K=1024, chunk_rows=0) == big                            # nothing of size B x N
    # the staged users take half the bytes of the bf16 form
    a = _lib.CatalogCoarseDeep()
    a.B, a.N, a.D, a.K, a.catalog_bf16 = 512, 1 << 20, 1024, 1024, 1
    assert lib.ur_catalog_coarse_deep_select(ctypes.byref(a), None) == 0 and a.workspace_bytes - big == (1 << 19) - 2048
    assert _select_need(lib, B=64, N=1 << 20, D=256, K=1000, chunk_rows=0) == want(64, 256, 1 << 18, 1000, 8)
    assert _select_need(lib, B=0) == 16
    # the query needs no pointer at all (and no device), and still refuses what the call refuses, leaving workspace_bytes alone
    a = _select_args(None, E=0, **{n: None for n in _SELECT_PTRS if n != "exclude"})
    a.workspace_bytes = -1
    assert lib.ur_catalog_fp8_select(ctypes.byref(a), None) == 0 and a.workspace_bytes == _select_need(lib, E=0)
    for over, word in ((dict(D=8), b"D must be"), (dict(K=1025), b"K must be"), (dict(K=0), b"K must be"), (dict(chunk_rows=1000), b"chunk_rows"),
                       (dict(segments=17), b"segments")):
        a = _select_args(None, workspace=None, **over)
        a.workspace_bytes = 123
        assert lib.ur_catalog_fp8_select(ctypes.byref(a), None) < 0 and word in lib.ur_last_error() and a.workspace_bytes == 123
    # the re-rank: iu [B] | scores [B, K_in]
    assert _rerank_need(lib) == _pad16(3 * 4) + _pad16(3 * 300 * 4)
    assert _rerank_need(lib, B=512, K_in=1024, k=1000, N=1 << 20, D=1024) == 2048 + (2 << 20)
    assert _rerank_need(lib, B=5, K_in=1, k=1) == 32 + 32 and _rerank_need(lib, B=0) == 16
    a = _rerank_args(None, **{n: None for n in _RERANK_PTRS})
    a.workspace_bytes = -1
    assert lib.ur_catalog_fp8_rerank(ctypes.byref(a), None) == 0 and a.workspace_bytes == _rerank_need(lib)
    for over, word in ((dict(D=24), b"D must be"), (dict(K_in=1025), b"K_in must be"), (dict(k=301), b"k must be"), (dict(N=0), b"N")):
        a = _rerank_args(None, workspace=None, **over)
        a.workspace_bytes = 123
        assert lib.ur_catalog_fp8_rerank(ctypes.byref(a), None) < 0 and word in lib.ur_last_error() and a.workspace_bytes == 123


def test_fp8_workspace_layouts_and_codec_under_the_host_sanitizers(tmp_path):
    """tests/host/catalog_fp8_layout_check.cpp: the two plans over a grid of B, N, D, K and segments -- regions aligned, disjoint and
    inside the size the query answers, the size the closed form -- and the integer codec the kernels run (every code there and back,
    every tie to the even code, the row exponent at the boundary mantissas), as a stand-alone host program under AddressSanitizer and
    UBSan"""
    # the sanitizer runtimes are linked statically: a dynamic one insists on being the first library the process loads
    gxx, clang = shutil.which("g++"), shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    cxx = [gxx, "-static-libasan", "-static-libubsan"] if gxx else [clang, "-static-libsan"]
    exe = str(tmp_path / "catalog_fp8_layout_check")
    subprocess.run(cxx + ["-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                          "-I", os.path.join(ROOT, "unirec_amd", "csrc"),
                          os.path.join(ROOT, "tests", "host", "catalog_fp8_layout_check.cpp"), "-o", exe], check=True)
    # (the program allocates nothing it does not free at exit; the leak pass needs ptrace, which a sandbox may not grant)
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0 and run.stdout.split() == ["ok", "12600"], (run.returncode, run.stdout, run.stderr)


# ---- the reference holds up on its own -----------------------------------------------------------------------------------------------------
def test_decode_table_equals_torchs_view_of_all_256_codes():
    mine = ref.decode_table()
    theirs = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(F32).numpy()
    nan = np.isnan(theirs)
    assert np.nonzero(nan)[0].tolist() == [0x7f, 0xff] and np.array_equal(np.isnan(mine), nan)
    assert np.array_equal(mine[~nan].view(np.uint32), theirs[~nan].view(np.uint32))          # bits: -0 is code 0x80
    assert mine[0x7e] == 448.0 and mine[0x01] == 2.0 ** -9 and mine[0x08] == 2.0 ** -6 and np.signbit(mine[0x80])


def test_encoding_a_decoded_code_gives_the_same_code():
    codes = np.array([c for c in range(256) if c & 0x7f != 0x7f], dtype=np.uint8)
    assert np.array_equal(ref.encode(ref.decode(codes)), codes)
    # ties go to the even code, into the subnormals, and the sign of a zero stays
    assert ref.encode(np.float32([2.0 ** -10, 3 * 2.0 ** -10, -2.0 ** -10, 2.0 ** -11, 0.0, -0.0, 1.0625, 1.1875])).tolist() == \
        [0, 2, 0x80, 0, 0, 0x80, 0x38, 0x3a]
    # quantising a decoded catalogue at e = 0 returns it
    rows = ref.decode(codes)[None].repeat(2, 0)[:, :240].copy()
    rows[:, 0] = 448.0
    c, s, _ = ref.quantize(torch.from_numpy(rows))
    assert np.array_equal(ref.decode(c), rows) and s.tolist() == [1.0, 1.0]


def test_the_frexp_rule_is_the_largest_exponent_at_the_boundary_mantissas():
    up, down = np.float32(np.inf), np.float32(0)
    for x in range(-60, 60):
        for m in (np.float32(0.5), np.nextafter(np.float32(0.5), up), np.nextafter(np.float32(0.875), down), np.float32(0.875),
                  np.nextafter(np.float32(0.875), up), np.nextafter(np.float32(1.0), down)):
            a = np.float32(np.ldexp(m, x))
            assert int(ref.row_exponent(a)) == ref.row_exponent_by_search(a), (m, x)
    assert int(ref.row_exponent(np.float32(448.0))) == 0 and int(ref.row_exponent(np.nextafter(np.float32(448.0), up))) == -1
    assert ref.row_exponent(np.float32([0.0, np.inf, np.nan, 2.0 ** -70, 2.0 ** 100, 1e-45])).tolist() == [0, 0, 0, 64, -64, 64]
    # the norm chain: against float64 within the chain's rounding, and exact where every partial sum is a small integer
    rows = np.ones((3, 48), dtype=np.float32)
    assert ref.row_inv_norm(rows).tolist() == [np.float32(1.0) / np.sqrt(np.float32(48.0))] * 3
    g = np.random.default_rng(0).standard_normal((5, 1056)).astype(np.float32)
    want = 1.0 / np.sqrt((g.astype(np.float64) ** 2).sum(1))
    assert np.abs(ref.row_inv_norm(g) / want - 1).max() < 32 * 2.0 ** -24
    assert ref.row_inv_norm(np.zeros((1, 16), dtype=np.float32))[0] == np.float32(1.0) / np.float32(1e-12)


# ---- the route Fp8CatalogEvaluator takes, with every device call out of reach -------------------------------------------------------------
class Reached(Exception):
    pass


_WRAPPERS = ("catalog_deep_select", "catalog_select", "catalog_coarse_select", "catalog_rerank", "catalog_scores", "catalog_softmax",
             "catalog_coarse_deep_select", "catalog_deep_rerank", "catalog_prefix_norms", "catalog_funnel_select", "catalog_funnel_rerank",
             "catalog_fp8_quantize", "catalog_fp8_select", "catalog_fp8_rerank")


@pytest.fixture
def stages(monkeypatch):
    """the fp8 wrappers and the deep re-rank replaced by recorders that work on host tensors (the quantiser by the reference); every other
    wrapper raises Reached, and loading the library fails if touched"""
    from unirec_amd import hip
    calls = []

    def quantize(src, out=None):
        calls.append(("quantize", tuple(src.shape), src.dtype, src.device.type))
        c, s, i = (torch.from_numpy(x) for x in ref.quantize(src))
        if out is None:
            return c, s, i
        out[0].copy_(c), out[1].copy_(s), out[2].copy_(i)
        return out

    def select(u, codes, K, inv, gt_index=None, exclude=None, chunk_rows=None, segments=None):
        calls.append(("select", tuple(codes.shape), codes.dtype, K, gt_index is not None, exclude is not None, chunk_rows))
        rank = None if gt_index is None else torch.ones(u.shape[0], dtype=torch.int32)
        return torch.zeros(u.shape[0], K, dtype=torch.int32), None, rank

    def rerank(u, codes, index, inv, k=None):
        calls.append(("rerank", tuple(index.shape), k, inv is not None))
        return index[:, :k], torch.zeros(u.shape[0], k)

    def deep_rerank(u, cat, index, k=None, cat_inv_norm=None):
        calls.append(("deep_rerank", cat.dtype, tuple(index.shape), k))
        return index[:, :k], torch.zeros(u.shape[0], k), torch.ones(cat.shape[0])
    for name in _WRAPPERS:
        monkeypatch.setattr(hip, name, lambda *a, _n=name, **k: (_ for _ in ()).throw(Reached(_n)))
    monkeypatch.setattr(hip, "catalog_fp8_quantize", quantize)
    monkeypatch.setattr(hip, "catalog_fp8_select", select)
    monkeypatch.setattr(hip, "catalog_fp8_rerank", rerank)
    monkeypatch.setattr(hip, "catalog_deep_rerank", deep_rerank)
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(Reached("_lib.load")))
    return calls


def _catalog(N=200, D=64, dtype=F32):
    return torch.arange(N * D, dtype=F32).reshape(N, D).sin().to(dtype)


def test_the_evaluator_quantises_block_by_block_and_holds_one_byte_per_element(stages):
    from unirec_amd.evaluation import CatalogEvaluator, Fp8CatalogEvaluator
    calls = stages
    cat = _catalog()
    ev = Fp8CatalogEvaluator(cat, item_ids=range(200), device="cpu", block_rows=64)
    assert calls == [("quantize", (64, 64), F32, "cpu")] * 3 + [("quantize", (8, 64), F32, "cpu")]
    rc, rs, ri = ref.quantize(cat)
    assert np.array_equal(ev.codes.numpy(), rc) and np.array_equal(ev.scale.numpy(), rs) and np.array_equal(ev.inv.numpy(), ri)
    held = {n: t for n, t in vars(ev).items() if isinstance(t, torch.Tensor)}
    assert sorted(held) == ["codes", "inv", "scale"] and ev.codes.dtype == torch.uint8 and ev.codes.numel() == 200 * 64
    assert ev.item_ids[:2] == ["0", "1"]
    # dequantized() is the exact decoding and stays close to the source: half a step of the top binade of a row is 2^-4 of its maximum
    deq = ev.dequantized()
    assert np.array_equal(deq.numpy(), ref.dequantize(rc, rs)) and float((deq - cat).abs().max()) <= 2.0 ** -4
    assert torch.equal(ev.dequantized([3, 1]), deq[[3, 1]])
    # a bf16 source is taken as it is; None picks blocks by bytes; quantized() hands the evaluator's own tensor over
    del calls[:]
    Fp8CatalogEvaluator(_catalog(dtype=BF16), device="cpu")
    assert calls == [("quantize", (200, 64), BF16, "cpu")]
    del calls[:]
    q = CatalogEvaluator(cat, device="cpu", dtype=BF16).quantized(block_rows=150)
    assert calls == [("quantize", (150, 64), BF16, "cpu"), ("quantize", (50, 64), BF16, "cpu")] and q.codes.shape == (200, 64)
    for bad in (torch.zeros(5, 24), torch.zeros(5), torch.zeros(5, 4096), torch.zeros(5, 0)):
        with pytest.raises(ValueError, match="Fp8CatalogEvaluator: catalog must be"):
            Fp8CatalogEvaluator(bad, device="cpu")
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="Fp8CatalogEvaluator: block_rows"):
            Fp8CatalogEvaluator(cat, device="cpu", block_rows=bad)
    with pytest.raises(ValueError, match="from_codes: codes must be"):
        Fp8CatalogEvaluator.from_codes(torch.zeros(5, 32), torch.ones(5))
    with pytest.raises(ValueError, match="from_codes: scale must be"):
        Fp8CatalogEvaluator.from_codes(torch.zeros(5, 32, dtype=torch.uint8), torch.ones(4))
    with pytest.raises(Reached) as hit:                                     # the norms come from the row-norm kernel
        Fp8CatalogEvaluator.from_codes(ev.codes, ev.scale)
    assert hit.value.args[0] == "catalog_prefix_norms"


def test_retrieve_two_stage_routes_and_refuses(stages):
    from unirec_amd.evaluation import CatalogEvaluator, Fp8CatalogEvaluator
    calls = stages
    ev = Fp8CatalogEvaluator(_catalog(), device="cpu")
    u = torch.ones(2, 64)
    del calls[:]
    out = ev.retrieve_two_stage(u, k=5, shortlist=700, gt_index=[3, 4], exclude=[[1, 2], [5]], ks=(1, 10), chunk_rows=1024)
    assert calls == [("select", (200, 64), torch.uint8, 700, True, True, 1024), ("rerank", (2, 700), 5, True)]
    assert out["topk_index"].shape == (2, 5) and out["rank_is_coarse"] is True and out["catalog_dtype"] == "fp8_e4m3" and out["mrr"] == 1.0
    assert out["hit_at"] == {1: 1.0, 10: 1.0} and set(out["ndcg_at"]) == {1, 10}
    del calls[:]
    out = ev.retrieve_two_stage(u, k=5)
    assert calls == [("select", (200, 64), torch.uint8, 128, False, False, None), ("rerank", (2, 128), 5, True)]
    assert sorted(out) == ["catalog_dtype", "rank_is_coarse", "topk_index", "topk_score"]
    # the default shortlist is CatalogEvaluator.retrieve_two_stage's
    for k, S in ((1, 128), (64, 128), (65, 130), (500, 1000), (513, 1024), (1024, 1024)):
        del calls[:]
        ev.retrieve_two_stage(u, k=k)
        assert calls[0][3] == S and calls[1] == ("rerank", (2, S), k, True)
    assert "NOT a tuned value" in Fp8CatalogEvaluator.retrieve_two_stage.__doc__
    # rerank_with: that evaluator's deep re-rank of the same shortlist
    full = CatalogEvaluator(_catalog(), device="cpu", dtype=BF16)
    del calls[:]
    out = ev.retrieve_two_stage(u, k=5, shortlist=300, rerank_with=full)
    assert calls == [("select", (200, 64), torch.uint8, 300, False, False, None), ("deep_rerank", BF16, (2, 300), 5)]
    assert out["catalog_dtype"] == "fp8_e4m3" and full._inv is not None
    # the refusals of CatalogEvaluator.retrieve_two_stage, in its words, before any device call
    del calls[:]
    for kw in (dict(k=0), dict(k=-1), dict(k=1025), dict(k=10.0), dict(k="10"), dict(k=True), dict(k=None)):
        with pytest.raises(ValueError, match=r"retrieve_two_stage: k must be an int in \[1, 1024\]"):
            ev.retrieve_two_stage(u, **kw)
    for sl in (4, 1025, 128.0, True, "128"):
        with pytest.raises(ValueError, match=r"retrieve_two_stage: shortlist must be an int in \[k, 1024\]"):
            ev.retrieve_two_stage(u, k=5, shortlist=sl)
    for other in (CatalogEvaluator(_catalog(N=100), device="cpu"), CatalogEvaluator(_catalog(D=32), device="cpu"), ev, torch.zeros(200, 64)):
        with pytest.raises(ValueError, match="retrieve_two_stage: rerank_with must be a CatalogEvaluator over the same"):
            ev.retrieve_two_stage(u, k=5, rerank_with=other)
    assert calls == []
    bf = CatalogEvaluator(_catalog(), device="cpu", dtype=BF16)
    with pytest.raises(ValueError) as mine:
        ev.retrieve_two_stage(u, k=0)
    with pytest.raises(ValueError) as theirs:
        bf.retrieve_two_stage(u, k=0)
    assert str(mine.value) == str(theirs.value)


def test_the_older_evaluator_paths_keep_their_routes(stages):
    from unirec_amd.evaluation import CatalogEvaluator
    u = torch.ones(2, 64)
    ev = CatalogEvaluator(_catalog(), device="cpu", dtype=BF16)
    for call, name in ((lambda: ev.retrieve(u, k=10), "catalog_select"), (lambda: ev.retrieve(u, k=200), "catalog_deep_select"),
                       (lambda: ev.retrieve(u, k=10, shortlist=128), "catalog_coarse_select"),
                       (lambda: ev.retrieve_two_stage(u, k=10, shortlist=300), "catalog_coarse_deep_select"),
                       (lambda: ev.retrieve_funnel(u, k=5, dims=(8, 64)), "catalog_prefix_norms")):
        with pytest.raises(Reached) as hit:
            call()
        assert hit.value.args[0] == name


def test_wrappers_refuse_before_the_library():
    from unirec_amd import hip
    u = torch.zeros(2, 32)
    codes = torch.zeros(5, 32, dtype=torch.uint8)
    inv = torch.ones(5)
    index = torch.zeros(2, 300, dtype=torch.int32)
    with pytest.raises(_lib.UniRecHipError, match="no CPU fallback"):
        hip.catalog_fp8_select(u, codes, 300, inv)
    with pytest.raises(_lib.UniRecHipError, match="no CPU fallback"):
        hip.catalog_fp8_rerank(u, codes.view(torch.float8_e4m3fn), index, inv)
    with pytest.raises(_lib.UniRecHipError, match="no CPU fallback"):
        hip.catalog_fp8_quantize(torch.zeros(5, 32))
    with pytest.raises(ValueError, match="catalog_fp8_select: codes must be uint8 or float8_e4m3fn"):
        hip.catalog_fp8_select(u, codes.to(BF16), 300, inv)
    with pytest.raises(ValueError, match="catalog_fp8_select: user .* and codes .* must share D"):
        hip.catalog_fp8_select(torch.zeros(2, 16), codes, 300, inv)
    with pytest.raises(ValueError, match="catalog_fp8_rerank: D must be a multiple of 16"):
        hip.catalog_fp8_rerank(torch.zeros(2, 24), torch.zeros(5, 24, dtype=torch.uint8), index, inv)
    for bad in (None, torch.ones(4), torch.ones(5, dtype=torch.float64)):
        with pytest.raises(ValueError, match="catalog_fp8_select: cat_inv_norm must be f32 of shape"):
            hip.catalog_fp8_select(u, codes, 300, bad)
    with pytest.raises(ValueError, match="catalog_fp8_quantize: src must be f32 or bf16"):
        hip.catalog_fp8_quantize(torch.zeros(5, 32, dtype=torch.float64))
    with pytest.raises(ValueError, match="catalog_fp8_quantize: src must be .* multiple of 16"):
        hip.catalog_fp8_quantize(torch.zeros(5, 40))
    with pytest.raises(ValueError, match="catalog_fp8_quantize: src must have unit stride"):
        hip.catalog_fp8_quantize(torch.zeros(5, 34)[:, :32])

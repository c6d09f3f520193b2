"""CPU: the host side of the Matryoshka catalogue softmax -- the rules include/unirec_hip_mrl_loss.h is held to (declared <=> exported
<=> bound, a name in one header only, the ctypes mirror of its struct field for field, the entry point named in the COVERS dict of
tests/test_gpu_catalog_mrl_softmax.py), every refusal of ur_catalog_mrl_softmax through the raw library (fake non-null pointers: each call
returns before any launch), the size query against the layout the header documents, that layout under the host sanitizers, and what the
loss module and the trainers accept and refuse before the library is touched."""
import ast
import ctypes
import os
import re
import shutil
import subprocess
import types

import pytest
import torch

from unirec_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "unirec_hip_mrl_loss.h")
GPU_TESTS = "tests/test_gpu_catalog_mrl_softmax.py"
OTHER_HEADERS = ("unirec_hip.h", "unirec_hip_loss.h", "unirec_hip_adapter.h", "unirec_hip_pool.h", "unirec_hip_mrl.h", "unirec_hip_coarse.h",
                 "unirec_hip_deep.h", "unirec_hip_coarse_deep.h", "unirec_hip_funnel.h")
ENTRY = "ur_catalog_mrl_softmax"
FAKE = 1 << 20          # non-null, 16-byte aligned, never dereferenced on the host
MB = 1 << 24
SEGS = 16               # CSM_SEGS: workgroups per user's chunk row
F32, BF16 = torch.float32, torch.bfloat16


# ---- the header: declared <=> exported <=> bound, the struct mirror, a test for the entry point ------------------------------------------
def _source(header=HEADER):
    return re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)


def _declared(header=HEADER):
    return sorted(set(re.findall(r"\b(ur_[a-z0-9_]+)\s*\(", _source(header))))


def test_mrl_loss_header_symbols_are_bound_and_exported():
    names = _declared()
    assert names == [ENTRY]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, ENTRY), f"{ENTRY} declared in unirec_hip_mrl_loss.h but not exported by libunirec_hip.so"
    assert sorted(_lib.MRL_LOSS_SIGNATURES) == names, "declared <=> bound in unirec_amd/_lib.py"
    others = set(_lib.SIGNATURES) | set(_lib.LOSS_SIGNATURES) | set(_lib.ADAPTER_SIGNATURES) | set(_lib.POOL_SIGNATURES) | \
        set(_lib.MRL_SIGNATURES) | set(_lib.COARSE_SIGNATURES) | set(_lib.DEEP_SIGNATURES) | set(_lib.COARSE_DEEP_SIGNATURES) | \
        set(_lib.FUNNEL_SIGNATURES)
    assert not set(_lib.MRL_LOSS_SIGNATURES) & others, "a name belongs to one header"
    for other in OTHER_HEADERS:
        assert ENTRY not in _declared(os.path.join(ROOT, "include", other)), f"{other} declares the entry point of this family"
    loaded = _lib.load()
    assert getattr(loaded, ENTRY).argtypes == _lib.MRL_LOSS_SIGNATURES[ENTRY][1], f"load() did not bind {ENTRY}"
    assert getattr(loaded, ENTRY).restype == _lib.MRL_LOSS_SIGNATURES[ENTRY][0]
    assert _lib.ABI_VERSION >= 29 and loaded.ur_version() == _lib.ABI_VERSION      # (this header arrived with ABI 29)
    # the older families keep exactly their entry points
    assert sorted(_lib.LOSS_SIGNATURES) == ["ur_catalog_softmax"] and sorted(_lib.MRL_SIGNATURES) == ["ur_mrl_infonce", "ur_mrl_scores"]
    assert sorted(_lib.FUNNEL_SIGNATURES) == ["ur_catalog_funnel_rerank", "ur_catalog_funnel_select", "ur_catalog_prefix_norms"]


_CTYPE = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}


def test_struct_mirror_matches_the_header_field_for_field():
    src = _source()
    found = re.findall(r"typedef struct \{(.*?)\}\s*(\w+);", src, flags=re.S)
    assert [name for _, name in found] == ["ur_catalog_mrl_softmax_t"]
    # the arrays are sized by UR_MRL_MAX_DIMS of include/unirec_hip_mrl.h, which this header includes
    defines = {k: int(v) for k, v in re.findall(r"#define (\w+) (\d+)", _source(os.path.join(ROOT, "include", "unirec_hip_mrl.h")))}
    assert defines["UR_MRL_MAX_DIMS"] == _lib.MRL_MAX_DIMS and '#include "unirec_hip_mrl.h"' in src
    fields = []
    for decl in (d.strip() for d in found[0][0].split(";")):
        if not decl:
            continue
        m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)(?:\[(\w+)\])?", decl)
        assert m, f"cannot read the field declaration {decl!r}"
        ctype, star, field, count = m.groups()
        t = ctypes.c_void_p if star else _CTYPE[ctype]
        fields.append((field, t * defines[count] if count else t))
    got = _lib.CatalogMrlSoftmax
    want = type("FromHeader", (ctypes.Structure,), {"_fields_": fields})
    assert [f[0] for f in got._fields_] == [f[0] for f in fields], "field names and order"
    assert ctypes.sizeof(got) == ctypes.sizeof(want)
    for (name, t), (_, tw) in zip(got._fields_, fields):
        assert getattr(got, name).offset == getattr(want, name).offset, name
        same_array = hasattr(t, "_length_") and hasattr(tw, "_length_") and t._length_ == tw._length_ and t._type_ is tw._type_
        assert t is tw or same_array, f"{name}: {t} against the header's {tw}"
    # the fields of ur_catalog_softmax_t, with K, dims, weights and plane_loss added in front of loss
    plain = [f[0] for f in _lib.CatalogSoftmax._fields_]
    at = plain.index("loss")
    assert [f[0] for f in got._fields_] == plain[:at] + ["K", "dims", "weights", "plane_loss"] + plain[at:]


def test_the_entry_point_is_listed_in_the_gpu_file():
    with open(os.path.join(ROOT, GPU_TESTS)) as f:
        tree = ast.parse(f.read())
    covers = None
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "COVERS" for t in node.targets):
            covers = ast.literal_eval(node.value)
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    assert isinstance(covers, dict), f"{GPU_TESTS} has no top-level COVERS dict"
    assert sorted(covers) == _declared(), "COVERS lists exactly the entry point of unirec_hip_mrl_loss.h"
    assert covers[ENTRY] and all(name in tests for name in covers[ENTRY]), covers


# ---- every refusal, without a GPU --------------------------------------------------------------------------------------------------------
_PTRS = ("user", "catalog", "cat_inv_norm", "gt_index", "exclude", "plane_loss", "loss", "row_loss", "lse", "d_user", "workspace")


def _args(lib=None, **over):
    """a valid argument struct over fake pointers with `over` applied: B 3, N 2000, D 72, dims (8, 40, 72), weights (1, 0, 2), E 5,
    chunk_rows 1024, f32; with `lib` the workspace is sized by the call's own size query unless workspace_bytes is given"""
    a = _lib.CatalogMrlSoftmax()
    names = [f[0] for f in a._fields_]
    for i, n in enumerate(_PTRS):
        setattr(a, n, FAKE + i * MB)
    sizes = dict(B=3, N=2000, D=72, K=3, E=5, chunk_rows=1024, temperature=0.07, grad_scale=1.0)
    over.setdefault("dims", (8, 40, 72))
    over.setdefault("weights", (1.0, 0.0, 2.0))
    for k, v in {**sizes, **over}.items():
        assert k in names, k
        if k in ("dims", "weights"):
            getattr(a, k)[:len(v)] = v
        else:
            setattr(a, k, v)
    if lib is not None and "workspace_bytes" not in over:
        q = _lib.CatalogMrlSoftmax()
        ctypes.memmove(ctypes.byref(q), ctypes.byref(a), ctypes.sizeof(a))
        q.workspace = None
        a.workspace_bytes = q.workspace_bytes if lib.ur_catalog_mrl_softmax(ctypes.byref(q), None) == 0 else 1 << 40
    return a


def test_refuses_invalid_arguments_without_a_gpu():
    lib = _lib.load()
    fn = lib.ur_catalog_mrl_softmax

    def rejected(word, **over):
        for query in (False, True):                                      # a size query checks the sizes too
            a = _args(lib, **over)
            if query:
                a.workspace = None
            rc = fn(ctypes.byref(a), None)
            msg = lib.ur_last_error()
            assert rc < 0 and ENTRY.encode() in msg and word in msg, (over, rc, msg)

    assert fn(None, None) < 0 and ENTRY.encode() in lib.ur_last_error()
    rejected(b"B >= 0", B=-1)
    rejected(b"N", N=0)
    rejected(b"N", N=1 << 31)
    for K in (0, -1, 9):                                                 # K out of 1 .. UR_MRL_MAX_DIMS
        rejected(b"K must be", K=K)
    rejected(b"strictly ascending", dims=(8, 8, 72))                     # dims not ascending
    rejected(b"strictly ascending", dims=(40, 8, 72))
    rejected(b"dims[1]", dims=(8, 42, 72))                               # not a multiple of 4
    rejected(b"dims[0]", dims=(0, 40, 72))
    rejected(b"dims[0]", dims=(-8, 40, 72))
    rejected(b"dims[1]", dims=(8, 12, 72), catalog_bf16=1)               # multiples of 8 for a bf16 catalogue
    rejected(b"dims[2]", dims=(8, 40, 76), D=76, catalog_bf16=1)
    rejected(b"last of dims", dims=(8, 40, 64))                          # last != D
    rejected(b"last of dims", dims=(8, 40, 76))
    rejected(b"last of dims", K=2)
    rejected(b"weights[1]", weights=(1.0, -1.0, 1.0))
    rejected(b"weights[0]", weights=(float("nan"), 1.0, 1.0))
    rejected(b"weights[2]", weights=(1.0, 1.0, float("inf")))
    rejected(b"at least one positive", weights=(0.0, 0.0, 0.0))
    rejected(b"temperature", temperature=0.0)
    rejected(b"temperature", temperature=-0.07)
    rejected(b"temperature", temperature=float("nan"))
    rejected(b"chunk_rows", chunk_rows=1000)
    rejected(b"chunk_rows", chunk_rows=-1024)
    rejected(b"exclude", exclude=None)                                   # E = 5 with a null exclude
    rejected(b"exclude", E=-1)
    rejected(b"scorer", scorer=3)
    rejected(b"scorer", scorer=-1)
    rejected(b"catalog_bf16", catalog_bf16=2)
    rejected(b"D", D=2052, dims=(8, 40, 2052))
    rejected(b"D", D=70, dims=(8, 40, 70))

    def refused_call(word, **over):
        rc = fn(ctypes.byref(_args(lib, **over)), None)
        msg = lib.ur_last_error()
        assert rc < 0 and ENTRY.encode() in msg and word in msg, (over, rc, msg)
    for name in ("user", "catalog", "cat_inv_norm", "gt_index", "plane_loss", "loss", "row_loss", "lse"):
        refused_call(b"null", **{name: None})
    for name in ("user", "catalog", "d_user"):                           # misaligned pointers
        refused_call(b"aligned", **{name: FAKE + 20 * MB + 8})
    need = _args(lib).workspace_bytes
    assert 0 < need < 1 << 40
    refused_call(b"workspace", workspace_bytes=need - 1)                 # a workspace one byte short
    refused_call(b"workspace", workspace=FAKE + 21 * MB + 4)
    # the limits themselves pass every check up to the pointers, with B == 0; entries past K are ignored
    for over in (dict(K=1, dims=(72,), weights=(1.0,)), dict(K=8, D=2048, dims=(8, 16, 24, 32, 40, 48, 56, 2048), weights=(0.0,) * 7 + (1e-30,)),
                 dict(D=12, dims=(4, 8, 12)), dict(catalog_bf16=1, dims=(8, 16, 72)), dict(K=2, dims=(8, 72, 1), weights=(1.0, 1.0, -1.0)),
                 dict(d_user=None), dict(E=0, exclude=None), dict(N=1), dict(N=(1 << 31) - 1), dict(chunk_rows=0), dict(scorer=1), dict(scorer=2)):
        assert fn(ctypes.byref(_args(lib, B=0, **over)), None) == 0, (over, lib.ur_last_error())
    none = {n: None for n in _PTRS if n not in ("workspace", "exclude")}
    assert fn(ctypes.byref(_args(lib, B=0, **none)), None) == 0, lib.ur_last_error()


# ---- the size query: the documented layout, restated ---------------------------------------------------------------------------------------
def _pad16(n):
    return (n + 15) // 16 * 16


def _splits(B, D, rows):
    """the row splits of the gradient product (include/unirec_hip_loss.h's plan): ~1024 workgroups, no split shorter than 64 rows"""
    tiles = ((max(B, 1) + 31) // 32) * ((D + 255) // 256)
    s = max(1, min(1024 // tiles, (rows + 63) // 64))
    rps = ((rows + s - 1) // s + 3) // 4 * 4
    return (rows + rps - 1) // rps


def _want(B, N, dims, chunk_rows, grad):
    K = len(dims)
    n_up = (N + 1023) // 1024 * 1024
    rows = chunk_rows or (64 << 20) // (4 * max(B, 1) * K) // 1024 * 1024
    rows = max(min(rows, n_up), 1024)
    need = _pad16(K * B * rows * 4) + 2 * _pad16(K * B * 4) + 3 * _pad16(K * B * SEGS * 4)
    if grad:
        need += sum(_pad16(_splits(B, d, rows) * B * d * 4) for d in dims)
    return max(need, 16)


def _need(lib, B, N, dims, chunk_rows, grad, **over):
    a = _args(None, **{**dict(B=B, N=N, D=dims[-1], K=len(dims), dims=dims, weights=(1.0,) * len(dims), chunk_rows=chunk_rows), **over})
    if not grad:
        a.d_user = None
    a.workspace, a.workspace_bytes = None, -1
    assert lib.ur_catalog_mrl_softmax(ctypes.byref(a), None) == 0, lib.ur_last_error()
    return a.workspace_bytes


def test_size_query_equals_the_documented_workspace_and_does_not_launch():
    lib = _lib.load()
    for B, N, dims, chunk_rows in ((3, 2000, (8, 40, 72), 1024), (3, 2000, (8, 40, 72), 0), (1, 1, (264,), 1024), (33, 5003, (8, 256, 264), 1024),
                                   (17, 5003, (248, 1032), 2048), (64, 1 << 20, (64, 128, 256, 512, 1024), 0),
                                   (512, 1 << 20, (64, 128, 256, 512, 1024), 0), (512, 1 << 20, (64, 128, 256, 512, 1024), 8192),
                                   (2000, 1 << 20, (4, 8, 12, 16, 20, 24, 28, 2048), 0)):
        for grad in (False, True):
            assert _need(lib, B, N, dims, chunk_rows, grad) == _want(B, N, dims, chunk_rows, grad), (B, N, dims, chunk_rows, grad)
    dims = (64, 128, 256, 512, 1024)
    # left to the library, the five planes share the 64 MB: a fifth of the rows of the plain call, and forward only is smaller
    fwd = _need(lib, 512, 1 << 20, dims, 0, False)
    assert fwd == _pad16(5 * 512 * 6144 * 4) + 2 * _pad16(5 * 512 * 4) + 3 * _pad16(5 * 512 * SEGS * 4) and fwd < (64 << 20) + (1 << 20)
    assert fwd < _need(lib, 512, 1 << 20, dims, 0, True)
    # nothing of size B x N and nothing of size N x d: the size does not grow with N
    assert _need(lib, 512, 1 << 30, dims, 0, True) == _need(lib, 512, 1 << 20, dims, 0, True) < (1 << 20) * 64 * 4
    # K = 1 at explicit rows: the plain call's workspace
    plain = _lib.CatalogSoftmax()
    plain.B, plain.N, plain.D, plain.chunk_rows, plain.temperature, plain.d_user = 33, 5003, 264, 1024, 0.07, FAKE
    assert lib.ur_catalog_softmax(ctypes.byref(plain), None) == 0 and plain.workspace_bytes == _need(lib, 33, 5003, (264,), 1024, True)
    # neither the scorer, the catalogue type, the weights nor E size anything
    base = _need(lib, 3, 2000, (8, 40, 72), 1024, True)
    for over in (dict(scorer=1), dict(scorer=2), dict(catalog_bf16=1), dict(E=0, exclude=None), dict(weights=(0.0, 0.0, 5.0))):
        assert _need(lib, 3, 2000, (8, 40, 72), 1024, True, **over) == base
    assert _need(lib, 0, 2000, (8, 40, 72), 1024, True) == 16
    # the query needs no pointer at all (and no device), and a refused query leaves workspace_bytes alone
    a = _args(None, E=0, **{n: None for n in _PTRS})
    a.workspace_bytes = -1
    assert lib.ur_catalog_mrl_softmax(ctypes.byref(a), None) == 0 and a.workspace_bytes == _want(3, 2000, (8, 40, 72), 1024, False)
    for over, word in ((dict(K=9), b"K must be"), (dict(dims=(8, 8, 72)), b"strictly ascending"), (dict(dims=(8, 42, 72)), b"dims[1]"),
                       (dict(dims=(8, 40, 64)), b"last of dims"), (dict(weights=(0.0, 0.0, 0.0)), b"at least one positive"),
                       (dict(weights=(1.0, -2.0, 1.0)), b"weights[1]"), (dict(temperature=0.0), b"temperature"), (dict(chunk_rows=1000), b"chunk_rows"),
                       (dict(exclude=None), b"exclude"), (dict(catalog_bf16=1, dims=(8, 12, 72)), b"dims[1]")):
        a = _args(None, workspace=None, **over)
        a.workspace_bytes = 123
        assert lib.ur_catalog_mrl_softmax(ctypes.byref(a), None) < 0 and word in lib.ur_last_error() and a.workspace_bytes == 123, over


def test_workspace_layout_under_the_host_sanitizers(tmp_path):
    """tests/host/catalog_mrl_softmax_layout_check.cpp: the plan over a grid of B, N, dims, chunk_rows and forward / backward -- regions
    aligned, disjoint and inside the size the query answers, the size the closed form, every plane's segment size and row splits those of
    the plain call's plan on the slice -- as a stand-alone host program under AddressSanitizer and UBSan"""
    # the sanitizer runtimes are linked statically: a dynamic one insists on being the first library the process loads
    gxx, clang = shutil.which("g++"), shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    cxx = [gxx, "-static-libasan", "-static-libubsan"] if gxx else [clang, "-static-libsan"]
    exe = str(tmp_path / "catalog_mrl_softmax_layout_check")
    subprocess.run(cxx + ["-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                          "-I", os.path.join(ROOT, "unirec_amd", "csrc"),
                          os.path.join(ROOT, "tests", "host", "catalog_mrl_softmax_layout_check.cpp"), "-o", exe], check=True)
    # (the program allocates nothing it does not free at exit; the leak pass needs ptrace, which a sandbox may not grant)
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0 and run.stdout.split() == ["ok", "3072"], (run.returncode, run.stdout, run.stderr)


# ---- the loss module, the trainers and the wrapper: before the library, the model or the device is touched ---------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", touched)


def test_loss_module_takes_matryoshka_dims(no_library):
    from unirec_amd.evaluation import CatalogEvaluator
    from unirec_amd.joint import CatalogSoftmaxLoss
    cat = torch.randn(30, 32, generator=torch.Generator().manual_seed(1))
    ev = CatalogEvaluator(cat, device="cpu")
    plain = CatalogSoftmaxLoss(ev)
    assert plain.matryoshka_dims is None and plain.matryoshka_weights is None and plain.last_plane_loss is None
    ok = CatalogSoftmaxLoss(ev, 0.07, None, None, matryoshka_dims=[4, 12, 32])
    assert ok.matryoshka_dims == (4, 12, 32) and ok.matryoshka_weights == (1.0, 1.0, 1.0) and ok.evaluator is ev
    assert ok.last_plane_loss is None and ok.last_lse is None and ok.last_row_loss is None
    assert CatalogSoftmaxLoss(ev, matryoshka_dims=(32,), matryoshka_weights=[2]).matryoshka_weights == (2.0,)
    assert CatalogSoftmaxLoss(cat.to(BF16), matryoshka_dims=(8, 32), matryoshka_weights=(0.0, 1.0)).matryoshka_weights == (0.0, 1.0)
    with pytest.raises(ValueError, match="matryoshka_weights needs matryoshka_dims"):
        CatalogSoftmaxLoss(ev, matryoshka_weights=(1.0, 1.0))
    with pytest.raises(ValueError, match="matryoshka_dims: the last entry must be the embedding width 32"):
        CatalogSoftmaxLoss(ev, matryoshka_dims=(4, 12, 16))
    with pytest.raises(ValueError, match="matryoshka_dims.*multiple of 8 for a bf16 catalogue"):
        CatalogSoftmaxLoss(cat.to(BF16), matryoshka_dims=(4, 32))
    for bad in ((), (4, 6, 32), (0, 32), (8, 8, 32), (16, 8, 32), tuple(range(4, 40, 4)), (4.0, 32), "32", 32, (True, 32)):
        with pytest.raises(ValueError, match="matryoshka_dims"):
            CatalogSoftmaxLoss(ev, matryoshka_dims=bad)
    for bad in ((1.0, -1.0, 1.0), (1.0, float("nan"), 1.0), (0.0, 0.0, 0.0), (1.0, 1.0), "abc", 1.0):
        with pytest.raises(ValueError, match="matryoshka_weights"):
            CatalogSoftmaxLoss(ev, matryoshka_dims=(4, 12, 32), matryoshka_weights=bad)


def test_trainers_take_matryoshka_dims_with_the_catalogue_softmax(no_library):
    from unirec_amd.joint import CatalogSoftmaxLoss, JointTrainer, MultiModalTrainer
    from unirec_amd.negatives import CatalogCandidates
    cat = torch.randn(30, 32, generator=torch.Generator().manual_seed(1))
    args = types.SimpleNamespace(learning_rate=1e-3, max_steps=2)
    tr = MultiModalTrainer(0.07, CatalogCandidates(cat), loss="catalog_softmax", matryoshka_dims=(4, 12, 32), matryoshka_weights=(1.0, 0.0, 0.5))
    assert isinstance(tr.catalog_softmax_loss, CatalogSoftmaxLoss) and tr.catalog_softmax_loss.evaluator is tr.negatives.evaluator
    assert tr.catalog_softmax_loss.matryoshka_dims == (4, 12, 32) and tr.catalog_softmax_loss.matryoshka_weights == (1.0, 0.0, 0.5)
    assert MultiModalTrainer(0.07, CatalogCandidates(cat), loss="catalog_softmax").catalog_softmax_loss.matryoshka_dims is None
    for make in (lambda **kw: MultiModalTrainer(0.07, **kw), lambda **kw: JointTrainer(None, args, **kw)):
        # no catalogue: the refusal names the loss and the dims, in that order
        with pytest.raises(ValueError, match="catalog_softmax.*matryoshka_dims.*negatives"):
            make(loss="catalog_softmax", matryoshka_dims=(4, 12, 32))
        with pytest.raises(ValueError, match="negatives"):
            make(loss="catalog_softmax")
        # the other refusals keep their text
        with pytest.raises(ValueError, match="num_random and negatives.num_hard must be 0"):
            make(negatives=CatalogCandidates(cat, num_random=4), loss="catalog_softmax", matryoshka_dims=(4, 12, 32))
        with pytest.raises(ValueError, match="num_random and negatives.num_hard must be 0"):
            make(negatives=CatalogCandidates(cat, num_hard=2), loss="catalog_softmax", matryoshka_dims=(4, 12, 32))
        with pytest.raises(ValueError, match="matryoshka_dims: the last entry must be the embedding width 32"):
            make(negatives=CatalogCandidates(cat), loss="catalog_softmax", matryoshka_dims=(4, 12, 16))
        with pytest.raises(ValueError, match="matryoshka_weights needs matryoshka_dims"):
            make(negatives=CatalogCandidates(cat), loss="catalog_softmax", matryoshka_weights=(1.0, 1.0))
        with pytest.raises(ValueError, match="matryoshka_weights"):
            make(negatives=CatalogCandidates(cat), loss="catalog_softmax", matryoshka_dims=(4, 12, 32), matryoshka_weights=(1.0, -1.0, 1.0))
    coarse = CatalogCandidates(cat.to(BF16))
    coarse.coarse = True
    with pytest.raises(ValueError, match="has no coarse form"):
        MultiModalTrainer(0.07, coarse, loss="catalog_softmax", matryoshka_dims=(8, 32))

    def model(**kw):
        raise AssertionError("the model ran")
    base = {"input_ids": None, "attention_mask": None, "history_field_embeddings": None, "history_attention_mask": None}
    with pytest.raises(ValueError, match="positive_item_index"):
        tr.compute_loss(model, dict(base))
    for key in ("negative_item_index", "negative_masks", "positive_item_embeddings", "negative_item_embeddings"):
        with pytest.raises(ValueError, match=f"must not carry {key}"):
            tr.compute_loss(model, dict(base, positive_item_index=torch.tensor([1]), **{key: torch.zeros(1)}))


def test_wrapper_refuses_before_the_library():
    from unirec_amd import hip
    u, cat, gt = torch.zeros(2, 16), torch.zeros(5, 16), torch.tensor([0, 1])
    with pytest.raises(_lib.UniRecHipError, match="no CPU fallback"):
        hip.catalog_mrl_softmax(u, cat, gt, (8, 16), None, 0.07)
    with pytest.raises(ValueError, match="catalog_mrl_softmax.*f32 or bf16"):
        hip.catalog_mrl_softmax(u, cat.to(torch.float16), gt, (8, 16), None, 0.07)
    with pytest.raises(ValueError, match="catalog_mrl_softmax.*must share D"):
        hip.catalog_mrl_softmax(u, torch.zeros(5, 32), gt, (8, 16), None, 0.07)
    with pytest.raises(ValueError, match="dims: the last entry must be the embedding width 16"):
        hip.catalog_mrl_softmax(u, cat, gt, (4, 8), None, 0.07)
    with pytest.raises(ValueError, match="multiple of 8 for a bf16 catalogue"):
        hip.catalog_mrl_softmax(u, cat.to(BF16), gt, (4, 16), None, 0.07)
    for dims in ((16, 8), (8, 8, 16), (), (0, 16), (6, 16), (8.0, 16), tuple(range(4, 40, 4))):
        with pytest.raises(ValueError, match="dims"):
            hip.catalog_mrl_softmax(u, cat, gt, dims, None, 0.07)
    for weights in ((1.0,), (1.0, -1.0), (0.0, 0.0), (1.0, float("nan"))):
        with pytest.raises(ValueError, match="weights"):
            hip.catalog_mrl_softmax(u, cat, gt, (8, 16), weights, 0.07)
    with pytest.raises(ValueError, match=r"cat_inv_norm must be f32 of shape \[2, 5\]"):
        hip.catalog_mrl_softmax(u, cat, gt, (8, 16), None, 0.07, cat_inv_norms=torch.zeros(5))
    with pytest.raises(ValueError, match="scorer"):
        hip.catalog_mrl_softmax(u, cat, gt, (8, 16), None, 0.07, scorer="MFMA")

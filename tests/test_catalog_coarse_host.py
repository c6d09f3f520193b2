"""CPU: the host side of the two-stage retrieval family -- the rules include/unirec_hip_coarse.h is held to (declared <=> exported <=>
bound, a name in one header only, the ctypes mirrors of its two structs field for field, a float64 test named for every entry point
through the COVERS dict of tests/test_gpu_catalog_coarse.py), every refusal of the two entry points and their size queries through the raw
library (fake non-null pointers: each call returns before any launch), the Python-level refusals of `shortlist` and `coarse` with the
library out of reach, and the float64 reference (tests/catalog_coarse_ref.py) against a direct float64 torch expression."""
import ast
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import catalog_coarse_ref as cref
from unirec_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "unirec_hip_coarse.h")
GPU_TESTS = "tests/test_gpu_catalog_coarse.py"
OTHER_HEADERS = ("unirec_hip.h", "unirec_hip_loss.h", "unirec_hip_adapter.h", "unirec_hip_pool.h", "unirec_hip_mrl.h")
FAKE = 1 << 20          # non-null, 16-byte aligned, never dereferenced on the host
MB = 1 << 24
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
ENTRY = {"coarse": "ur_catalog_coarse_select", "rerank": "ur_catalog_rerank"}


# ---- the header: declared <=> exported <=> bound, struct mirrors, a float64 test per entry point ----------------------------------------
def _source(header=HEADER):
    return re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)


def _declared(header=HEADER):
    return sorted(set(re.findall(r"\b(ur_[a-z0-9_]+)\s*\(", _source(header))))


def test_coarse_header_symbols_are_bound_and_exported():
    names = _declared()
    assert names == ["ur_catalog_coarse_select", "ur_catalog_rerank"]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in unirec_hip_coarse.h but not exported by libunirec_hip.so"
        assert n in _lib.COARSE_SIGNATURES, f"{n} declared in unirec_hip_coarse.h but not bound in unirec_amd/_lib.py"
    assert not set(_lib.COARSE_SIGNATURES) - set(names), "bound but not declared in the coarse header"
    others = set(_lib.SIGNATURES) | set(_lib.LOSS_SIGNATURES) | set(_lib.ADAPTER_SIGNATURES) | set(_lib.POOL_SIGNATURES) | set(_lib.MRL_SIGNATURES)
    assert not set(_lib.COARSE_SIGNATURES) & others, "a name belongs to one header"
    for other in OTHER_HEADERS:
        assert not set(names) & set(_declared(os.path.join(ROOT, "include", other))), f"{other} declares a coarse entry point"
    loaded = _lib.load()
    for n in names:
        assert getattr(loaded, n).argtypes == _lib.COARSE_SIGNATURES[n][1], f"load() did not bind {n}"
        assert getattr(loaded, n).restype == _lib.COARSE_SIGNATURES[n][0]
    assert _lib.ABI_VERSION >= 25 and loaded.ur_version() == _lib.ABI_VERSION      # (the coarse header arrived with ABI 25)


def test_header_constants_match_the_binding():
    consts = {k: int(v) for k, v in re.findall(r"#define (UR_COARSE_[A-Z_]+) (\d+)", open(HEADER).read())}
    assert consts == {"UR_COARSE_USER_GROUP": _lib.COARSE_USER_GROUP}
    from unirec_amd import hip
    assert hip.COARSE_USER_GROUP == _lib.COARSE_USER_GROUP == 64


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


@pytest.mark.parametrize("cname,mirror", [("ur_catalog_coarse_t", "CatalogCoarse"), ("ur_catalog_rerank_t", "CatalogRerank")])
def test_struct_mirrors_match_the_header_field_for_field(cname, mirror):
    structs = _header_structs()
    assert sorted(structs) == ["ur_catalog_coarse_t", "ur_catalog_rerank_t"]
    want = type("FromHeader", (ctypes.Structure,), {"_fields_": structs[cname]})
    got = getattr(_lib, mirror)
    assert [f[0] for f in got._fields_] == [f[0] for f in structs[cname]], "field names and order"
    assert ctypes.sizeof(got) == ctypes.sizeof(want)
    for (name, t), (_, tw) in zip(got._fields_, structs[cname]):
        assert getattr(got, name).offset == getattr(want, name).offset, name
        assert t is tw, f"{name}: {t} against the header's {tw}"


def test_every_coarse_entry_point_has_a_float64_test():
    with open(os.path.join(ROOT, GPU_TESTS)) as f:
        tree = ast.parse(f.read())
    covers = None
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "COVERS" for t in node.targets):
            covers = ast.literal_eval(node.value)
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    assert isinstance(covers, dict), f"{GPU_TESTS} has no top-level COVERS dict"
    assert sorted(covers) == _declared(), "COVERS lists exactly the entry points of unirec_hip_coarse.h"
    for entry, names in covers.items():
        assert names, f"COVERS[{entry!r}] names no test"
        for name in names:
            assert name in tests and "float64" in name, f"COVERS[{entry!r}] names {name}: no such float64 test"


# ---- every refusal, without a GPU -------------------------------------------------------------------------------------------------------
_PTRS = ("user", "catalog", "cat_inv_norm", "topk_index", "topk_score", "gt_index", "rank", "exclude", "index", "workspace")


def _args(which, lib=None, **over):
    """a valid argument struct over fake pointers (B 3, N 2000, D 40), with `over` applied; the workspace is sized by the size query of
    the call's own sizes unless `workspace_bytes` is given"""
    a = _lib.CatalogCoarse() if which == "coarse" else _lib.CatalogRerank()
    names = [f[0] for f in a._fields_]
    for i, n in enumerate(p for p in _PTRS if p in names):
        setattr(a, n, FAKE + i * MB)
    a.B, a.N, a.D = 3, 2000, 40
    if which == "coarse":
        a.catalog_bf16, a.K, a.E, a.chunk_rows = 1, 10, 5, 1024
    else:
        a.catalog_bf16, a.K_in, a.k = 0, 16, 10
    explicit_ws = "workspace_bytes" in over
    for k, v in over.items():
        assert k in names, k
        setattr(a, k, v)
    if lib is not None and not explicit_ws:
        q = type(a)()
        ctypes.memmove(ctypes.byref(q), ctypes.byref(a), ctypes.sizeof(a))
        q.workspace = None
        a.workspace_bytes = q.workspace_bytes if getattr(lib, ENTRY[which])(ctypes.byref(q), None) == 0 else 1 << 40
    return a


@pytest.mark.parametrize("which", ["coarse", "rerank"])
def test_invalid_arguments_are_rejected_without_a_gpu(which):
    lib = _lib.load()
    fn = getattr(lib, ENTRY[which])
    who = ENTRY[which].encode()

    def rejected(word, **over):
        rc = fn(ctypes.byref(_args(which, lib, **over)), None)
        msg = lib.ur_last_error()
        assert rc < 0 and who in msg and word in msg, (over, rc, msg)

    assert fn(None, None) < 0 and who in lib.ur_last_error()
    rejected(b"B >= 0", B=-1)
    rejected(b"N", N=-1)
    rejected(b"N", N=1 << 31)
    # D: not a multiple of 8 (4 for the re-rank of an f32 catalogue), zero, negative, too wide
    for D in (0, -8, 2056, 4096) + ((4, 12, 36, 41) if which == "coarse" else (2, 6, 41)):
        rejected(b"D must be", D=D)
    if which == "coarse":
        for K in (0, -1, 129):
            rejected(b"K must be", K=K)
        for flag in (0, 2, -1):                                   # an f32 catalogue, or a flag that is no dtype at all
            rejected(b"catalog_bf16", catalog_bf16=flag)
        rejected(b"chunk_rows", chunk_rows=1000)
        rejected(b"chunk_rows", chunk_rows=-1024)
        rejected(b"exclude", exclude=None)
        rejected(b"gt_index and rank", rank=None)
        rejected(b"gt_index and rank", gt_index=None)
        outputs, inputs = ("topk_index", "topk_score"), ("user", "catalog", "cat_inv_norm")
    else:
        for K_in in (0, -1, 129):
            rejected(b"K_in must be", K_in=K_in, k=1)
        for k in (0, -1, 17):                                     # k > K'
            rejected(b"k must be", k=k)
        for flag in (2, -1):
            rejected(b"catalog_bf16", catalog_bf16=flag)
        rejected(b"D must be", catalog_bf16=1, D=36)              # a bf16 row of 36 elements is not 16-byte pieces
        rejected(b"N", N=0)
        outputs, inputs = ("topk_index", "topk_score", "index"), ("user", "catalog", "cat_inv_norm")
    for name in outputs + inputs:
        rejected(b"null", **{name: None})
    for name in ("user", "catalog"):
        rejected(b"aligned", **{name: FAKE + 20 * MB + 8})
    # a short workspace (one byte), a misaligned one
    need = _args(which, lib).workspace_bytes
    assert need > 0
    rejected(b"workspace", workspace_bytes=need - 1)
    rejected(b"workspace", workspace=FAKE + 21 * MB + 4)
    # nothing to do: 0, nothing launched -- even with no buffers at all
    none = {n: None for n in _PTRS if n in [f[0] for f in _args(which)._fields_] and n not in ("workspace", "exclude", "gt_index", "rank")}
    a = _args(which, lib, B=0, **none)
    assert fn(ctypes.byref(a), None) == 0, lib.ur_last_error()


def _need(lib, which, **over):
    a = _args(which, None, **over)
    a.workspace, a.workspace_bytes = None, -1
    assert getattr(lib, ENTRY[which])(ctypes.byref(a), None) == 0, lib.ur_last_error()
    return a.workspace_bytes


def _pad16(n):
    return (n + 15) // 16 * 16


def test_size_query_holds_nothing_of_size_b_times_n():
    lib = _lib.load()
    # u~ [B,D] bf16 | iu~ [B] | ref [B] | chunk [B, rows] f32, rows = chunk_rows or the 64 MB rule, never more than N rounded up to 1024
    assert _need(lib, "coarse") == _pad16(3 * 40 * 2) + 2 * _pad16(3 * 4) + 3 * 1024 * 4
    assert _need(lib, "coarse", chunk_rows=0) == _pad16(3 * 40 * 2) + 2 * _pad16(3 * 4) + 3 * 2048 * 4
    big = _need(lib, "coarse", B=512, N=1 << 30, D=1024, chunk_rows=0)
    assert big == 512 * 1024 * 2 + 2 * 512 * 4 + (64 << 20)                     # 65 MB for B x N = 2^39 scores
    assert _need(lib, "coarse", B=512, N=1 << 20, D=1024, chunk_rows=0) == big    # N is not in it
    assert _need(lib, "coarse", B=512, N=1 << 30, D=1024, chunk_rows=2048) == 512 * 1024 * 2 + 2 * 512 * 4 + 512 * 2048 * 4
    assert _need(lib, "coarse", B=0) == 16
    # the re-rank: the users' inverse norms, nothing else
    assert _need(lib, "rerank") == 16 and _need(lib, "rerank", B=512, N=1 << 30) == 2048
    # the query needs no pointer at all, and still refuses what the call refuses
    for which in ("coarse", "rerank"):
        fn = getattr(lib, ENTRY[which])
        a = _args(which, None, **{n: None for n in _PTRS if n in [f[0] for f in _args(which)._fields_] and n != "exclude"}, **({"E": 0} if which == "coarse" else {}))
        a.workspace_bytes = -1
        assert fn(ctypes.byref(a), None) == 0 and a.workspace_bytes == _need(lib, which, **({"E": 0} if which == "coarse" else {}))
        for over, word in ((dict(D=12 if which == "coarse" else 6), b"D must be"),) + \
                ((((dict(K=129), b"K must be"), (dict(catalog_bf16=0), b"catalog_bf16"))) if which == "coarse" else ((dict(k=17), b"k must be"),)):
            a = _args(which, None, workspace=None, **over)
            a.workspace_bytes = 123
            assert fn(ctypes.byref(a), None) < 0 and word in lib.ur_last_error() and a.workspace_bytes == 123


# ---- Python-level refusals: all before the library is loaded ----------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """loading the library fails if touched, and so does every launch wrapper the two-stage surface could reach"""
    from unirec_amd import hip

    def touched(*a, **k):
        raise AssertionError("a device call was made")
    for name in ("catalog_coarse_select", "catalog_rerank", "catalog_select", "catalog_scores", "catalog_softmax"):
        monkeypatch.setattr(hip, name, touched)
    monkeypatch.setattr(_lib, "load", touched)


def _evaluator(dtype):
    from unirec_amd.evaluation import CatalogEvaluator
    return CatalogEvaluator(torch.arange(200 * 16, dtype=F32).reshape(200, 16).sin(), device="cpu", dtype=dtype)


def test_retrieve_refuses_by_name(no_device):
    u = torch.ones(2, 16)
    ev = _evaluator(BF16)
    for scorer in ("vector", "mfma"):
        with pytest.raises(ValueError, match="scorer"):
            ev.retrieve(u, k=10, shortlist=64, scorer=scorer)
    with pytest.raises(ValueError, match=r"shortlist.*dtype=torch\.bfloat16"):
        _evaluator(F32).retrieve(u, k=10, shortlist=64)
    for bad in (9, 0, -1, 129, 64.0, "64", True, (64,)):
        with pytest.raises(ValueError, match="shortlist"):
            ev.retrieve(u, k=10, shortlist=bad)
    with pytest.raises(ValueError, match="shortlist"):
        ev.retrieve(u, k=0, shortlist=64)
    with pytest.raises(ValueError, match="scorer"):                 # the old refusal of an unknown scorer is untouched
        ev.retrieve(u, k=10, scorer="bf16")
    # accepted forms reach the device call: k == shortlist, the ends of the range
    for k, shortlist in ((10, 10), (1, 128), (128, 128)):
        with pytest.raises(AssertionError, match="device call"):
            ev.retrieve(u, k=k, shortlist=shortlist)
    with pytest.raises(AssertionError, match="device call"):
        ev.truncated(8).retrieve(u[:, :8], k=10, shortlist=64)


def test_candidates_and_trainer_refuse_by_name(no_device):
    from unirec_amd.joint import MultiModalTrainer
    from unirec_amd.negatives import CatalogCandidates
    with pytest.raises(ValueError, match=r"coarse.*dtype=torch\.bfloat16"):
        CatalogCandidates(_evaluator(F32), num_hard=4, coarse=True)
    with pytest.raises(ValueError, match=r"coarse.*dtype=torch\.bfloat16"):
        CatalogCandidates(torch.zeros(5, 16), num_hard=4, coarse=True)
    with pytest.raises(ValueError, match="scorer"):
        CatalogCandidates(_evaluator(BF16), num_hard=4, coarse=True, scorer="mfma")
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="coarse"):
            CatalogCandidates(_evaluator(BF16), num_hard=4, coarse=bad)
    ok = CatalogCandidates(_evaluator(BF16), num_hard=4, hard_skip=2, coarse=True)
    assert ok.coarse is True and CatalogCandidates(_evaluator(BF16), num_hard=4).coarse is False
    with pytest.raises(ValueError, match="catalog_softmax.*coarse"):
        MultiModalTrainer(0.07, negatives=CatalogCandidates(_evaluator(BF16), coarse=True), loss="catalog_softmax")
    assert MultiModalTrainer(0.07, negatives=ok).negatives is ok


def test_wrappers_refuse_host_tensors_and_an_f32_catalogue():
    from unirec_amd import hip
    u, idx = torch.zeros(2, 16), torch.zeros(2, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"dtype=torch\.bfloat16"):
        hip.catalog_coarse_select(u, torch.zeros(5, 16), 4)
    with pytest.raises(_lib.UniRecHipError, match="no CPU fallback"):
        hip.catalog_coarse_select(u, torch.zeros(5, 16, dtype=BF16), 4)
    with pytest.raises(_lib.UniRecHipError, match="no CPU fallback"):
        hip.catalog_rerank(u, torch.zeros(5, 16), idx)
    with pytest.raises(ValueError, match="f32 or bf16"):
        hip.catalog_rerank(u, torch.zeros(5, 16, dtype=torch.float16), idx)


# ---- the float64 reference against a direct float64 torch expression ---------------------------------------------------------------------
@pytest.mark.parametrize("B,N,D,K,E", [(3, 50, 24, 10, 0), (5, 7, 8, 10, 3), (4, 300, 264, 128, 9)])
def test_reference_matches_a_direct_float64_expression(B, N, D, K, E):
    g = torch.Generator().manual_seed(B + N + D)
    user = torch.randn(B, D, generator=g)
    cat = torch.randn(N, D, generator=g).to(BF16)
    gt = torch.randint(0, N, (B,), generator=g)
    ex = torch.randint(-2, N, (B, E), generator=g) if E else None
    ub = user.to(BF16)
    assert torch.equal(cref.round_bf16(user), ub.to(F64))
    direct = torch.nn.functional.cosine_similarity(ub.to(F64)[:, None, :], cat.to(F64)[None, :, :], dim=2, eps=1e-12)
    s = cref.coarse_scores(user, cat)
    assert s.dtype == F64 and float((s - direct).abs().max()) < 1e-14
    exact = torch.nn.functional.cosine_similarity(user.to(F64)[:, None, :], cat.to(F64)[None, :, :], dim=2, eps=1e-12)
    assert float((cref.exact_scores(user, cat) - exact).abs().max()) < 1e-14
    # rounding one side to bf16 moves a cosine by less than 2^-8 (here: far less)
    assert float((s - exact).abs().max()) < 2.0 ** -8
    idx, val, rank = cref.select(s, K, gt, None if ex is None else ex.tolist())
    for b in range(B):
        kept = [n for n in range(N) if ex is None or n == int(gt[b]) or n not in set(ex[b].tolist())]
        want = sorted(kept, key=lambda n: (-float(s[b, n]), n))[:K]
        assert idx[b, :len(want)].tolist() == want and (idx[b, len(want):] == -1).all() and np.isneginf(val[b, len(want):]).all()
        assert np.array_equal(val[b, :len(want)], s[b, want].numpy())
        assert rank[b] == 1 + sum(1 for n in kept if n != int(gt[b]) and float(s[b, n]) > float(s[b, gt[b]]))
    lists = cref.select(s, K)
    assert lists[2] is None and (lists[0][:, 0] == s.argmax(1).numpy()).all()


def test_reference_rerank_rule():
    s = torch.tensor([[0.5, 0.25, 0.5, -1.0, 0.75]], dtype=F64)
    idx, val = cref.rerank(s, np.array([[3, -1, 2, 0, 9, 4, 2]]), 7)
    assert idx.tolist() == [[4, 0, 2, 2, 3, -1, -1]]                # ties by index, a duplicate twice, empty slots last
    assert val[0, :5].tolist() == [0.75, 0.5, 0.5, 0.5, -1.0] and np.isneginf(val[0, 5:]).all()
    assert cref.rerank(s, np.array([[3, -1, 2, 0, 9, 4, 2]]), 1)[0].tolist() == [[4]]

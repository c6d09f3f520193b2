"""CPU: the host side of the Matryoshka family -- the rules include/unirec_hip_mrl.h is held to (declared <=> exported <=> bound, a name
in one header only, the ctypes mirrors of its two structs field for field, a float64 test named for every entry point through the COVERS
dict of tests/test_gpu_mrl_f64.py), every refusal of the two entry points and the size query through the raw library (fake non-null
pointers: each call returns before any launch), the float64 reference (tests/mrl_ref.py) against the fixture tests/golden/mrl_tiny.npz
written by the reference's own InfoNCELoss on slices, and the Python-level refusals of the `matryoshka_dims` / `matryoshka_weights`
keywords, `mrr_ranks(dims=...)` and `CatalogEvaluator.truncated`."""
import ast
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import mrl_ref, ref64
from unirec_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "unirec_hip_mrl.h")
GPU_TESTS = "tests/test_gpu_mrl_f64.py"
OTHER_HEADERS = ("unirec_hip.h", "unirec_hip_loss.h", "unirec_hip_adapter.h", "unirec_hip_pool.h")
FAKE = 1 << 20          # non-null, 16-byte aligned, never dereferenced on the host
MB = 1 << 24
F64, F32 = torch.float64, torch.float32


# ---- the header: declared <=> exported <=> bound, struct mirrors, a float64 test per entry point ----------------------------------------
def _source(header=HEADER):
    return re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)


def _declared(header=HEADER):
    return sorted(set(re.findall(r"\b(ur_[a-z0-9_]+)\s*\(", _source(header))))


def test_mrl_header_symbols_are_bound_and_exported():
    names = _declared()
    assert names == ["ur_mrl_infonce", "ur_mrl_scores"]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in unirec_hip_mrl.h but not exported by libunirec_hip.so"
        assert n in _lib.MRL_SIGNATURES, f"{n} declared in unirec_hip_mrl.h but not bound in unirec_amd/_lib.py"
    assert not set(_lib.MRL_SIGNATURES) - set(names), "bound but not declared in the Matryoshka header"
    others = set(_lib.SIGNATURES) | set(_lib.LOSS_SIGNATURES) | set(_lib.ADAPTER_SIGNATURES) | set(_lib.POOL_SIGNATURES)
    assert not set(_lib.MRL_SIGNATURES) & others, "a name belongs to one header"
    for other in OTHER_HEADERS:
        assert not set(names) & set(_declared(os.path.join(ROOT, "include", other))), f"{other} declares a Matryoshka entry point"
    loaded = _lib.load()
    for n in names:
        assert getattr(loaded, n).argtypes == _lib.MRL_SIGNATURES[n][1], f"load() did not bind {n}"
        assert getattr(loaded, n).restype == _lib.MRL_SIGNATURES[n][0]
    assert _lib.ABI_VERSION >= 24 and loaded.ur_version() == _lib.ABI_VERSION      # (the Matryoshka header arrived with ABI 24)


def test_header_constants_match_the_binding():
    consts = {k: int(v) for k, v in re.findall(r"#define (UR_MRL_[A-Z_]+) (\d+)", open(HEADER).read())}
    assert consts == {"UR_MRL_MAX_DIMS": _lib.MRL_MAX_DIMS, "UR_MRL_BWD_CHUNKS": _lib.MRL_BWD_CHUNKS}
    from unirec_amd import hip
    assert hip.MRL_MAX_DIMS == _lib.MRL_MAX_DIMS == 8


_CTYPE = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}


def _header_structs():
    """{typedef name: [(field name, ctypes type)]} of every struct the header declares, read from its text"""
    consts = {k: int(v) for k, v in re.findall(r"#define (UR_MRL_[A-Z_]+) (\d+)", open(HEADER).read())}
    out = {}
    for body, name in re.findall(r"typedef struct \{(.*?)\}\s*(\w+);", _source(), flags=re.S):
        fields = []
        for decl in (d.strip() for d in body.split(";")):
            if not decl:
                continue
            m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)(?:\[(\w+)\])?", decl)
            assert m, f"{name}: cannot read the field declaration {decl!r}"
            ctype, star, field, dim = m.groups()
            t = ctypes.c_void_p if star else _CTYPE[ctype]
            if dim:
                t = t * (consts[dim] if dim in consts else int(dim))
            fields.append((field, t))
        out[name] = fields
    return out


@pytest.mark.parametrize("cname,mirror", [("ur_mrl_scores_t", "MrlScores"), ("ur_mrl_infonce_t", "MrlInfoNCE")])
def test_struct_mirrors_match_the_header_field_for_field(cname, mirror):
    structs = _header_structs()
    assert sorted(structs) == ["ur_mrl_infonce_t", "ur_mrl_scores_t"]
    want = type("FromHeader", (ctypes.Structure,), {"_fields_": structs[cname]})
    got = getattr(_lib, mirror)
    assert [f[0] for f in got._fields_] == [f[0] for f in structs[cname]], "field names and order"
    assert ctypes.sizeof(got) == ctypes.sizeof(want)
    for (name, t), (_, tw) in zip(got._fields_, structs[cname]):
        assert ctypes.sizeof(t) == ctypes.sizeof(tw) and getattr(got, name).offset == getattr(want, name).offset, name
        assert (t is ctypes.c_void_p) == (tw is ctypes.c_void_p), f"{name}: pointer against value"
        if t is not ctypes.c_void_p:
            assert t is tw or (issubclass(t, ctypes.Array) and t._type_ is tw._type_ and t._length_ == tw._length_), name


def test_every_mrl_entry_point_has_a_float64_test():
    with open(os.path.join(ROOT, GPU_TESTS)) as f:
        tree = ast.parse(f.read())
    covers = None
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "COVERS" for t in node.targets):
            covers = ast.literal_eval(node.value)
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    assert isinstance(covers, dict), f"{GPU_TESTS} has no top-level COVERS dict"
    assert sorted(covers) == _declared(), "COVERS lists exactly the entry points of unirec_hip_mrl.h"
    for entry, names in covers.items():
        assert names, f"COVERS[{entry!r}] names no test"
        for name in names:
            assert name in tests and "float64" in name, f"COVERS[{entry!r}] names {name}: no such float64 test"


# ---- every refusal, without a GPU -------------------------------------------------------------------------------------------------------
_PTRS = ("user", "pos", "neg", "neg_mask", "scores", "cand_inv_norm", "plane_loss", "loss", "d_user", "workspace")


def _args(which, lib=None, **over):
    """a valid argument struct over fake pointers (B 3, N 7, dims 4 12 32), with `over` applied; the workspace is sized by the size query
    of the call's own sizes unless `workspace_bytes` is given"""
    a = _lib.MrlScores() if which == "scores" else _lib.MrlInfoNCE()
    dims = list(over.pop("dims", (4, 12, 32)))
    a.K = over.pop("K", len(dims))
    a.dims[:len(dims)] = dims
    a.B, a.N, a.D = over.pop("B", 3), over.pop("N", 7), over.pop("D", dims[-1] if dims else 0)
    names = [f[0] for f in a._fields_]
    for i, n in enumerate(p for p in _PTRS if p in names):
        setattr(a, n, FAKE + i * MB)
    if which == "infonce":
        w = list(over.pop("weights", (1.0,) * len(dims)))
        a.weights[:len(w)] = w
        a.temperature, a.grad_scale = over.pop("temperature", 0.07), 1.0
        if lib is not None and "workspace_bytes" not in over:
            q = _args("infonce", None, dims=dims, K=a.K, B=a.B, N=a.N, D=a.D, weights=w, temperature=0.07)
            q.workspace = None
            a.workspace_bytes = q.workspace_bytes if lib.ur_mrl_infonce(ctypes.byref(q), None) == 0 else 0
    for k, v in over.items():
        assert k in names, k
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("which", ["scores", "infonce"])
def test_invalid_arguments_are_rejected_without_a_gpu(which):
    lib = _lib.load()
    fn = getattr(lib, f"ur_mrl_{which}")
    who = f"ur_mrl_{which}".encode()

    def rejected(word, **over):
        rc = fn(ctypes.byref(_args(which, lib, **over)), None)
        msg = lib.ur_last_error()
        assert rc < 0 and who in msg and word in msg, (over, rc, msg)

    assert fn(None, None) < 0 and who in lib.ur_last_error()
    # K outside 1..8
    rejected(b"K", K=0)
    rejected(b"K", K=-1)
    rejected(b"K", K=9)
    # a dim that is not a positive multiple of 4, not ascending, or last != D
    rejected(b"dims", dims=(4, 13, 32))
    rejected(b"dims", dims=(0, 12, 32), D=32)
    rejected(b"dims", dims=(-4, 12, 32), D=32)
    rejected(b"dims", dims=(2, 12, 32))
    rejected(b"dims", dims=(12, 12, 32))
    rejected(b"dims", dims=(16, 12, 32))
    rejected(b"dims", dims=(4, 12, 32), D=36)
    rejected(b"dims", dims=(4, 12, 32), D=28)
    rejected(b"B >= 0", B=-1)
    rejected(b"N >= 0", N=-1)
    # misaligned or null pointers
    for name in ("user", "pos", "neg", "scores", "cand_inv_norm") + (("plane_loss", "loss") if which == "infonce" else ()):
        rejected(b"null", **{name: None})
    for name in ("user", "pos", "neg"):
        rejected(b"aligned", **{name: FAKE + 20 * MB + 8})
    if which == "infonce":
        # a negative, non-finite or all-zero weight vector
        rejected(b"weights", weights=(1.0, -0.5, 1.0))
        rejected(b"weights", weights=(1.0, float("nan"), 1.0))
        rejected(b"weights", weights=(1.0, float("inf"), 1.0))
        rejected(b"weights", weights=(0.0, 0.0, 0.0))
        # temperature <= 0
        rejected(b"temperature", temperature=0.0)
        rejected(b"temperature", temperature=-0.07)
        rejected(b"temperature", temperature=float("nan"))
        # a short workspace (one byte), a misaligned one, a misaligned d_user
        need = _args(which, lib).workspace_bytes
        assert need > 0
        rejected(b"workspace", workspace_bytes=need - 1)
        rejected(b"workspace", workspace=FAKE + 21 * MB + 4)
        rejected(b"d_user", d_user=FAKE + 22 * MB + 4)
    # nothing to do: 0, nothing launched -- even with no buffers at all
    assert fn(ctypes.byref(_args(which, lib, B=0)), None) == 0
    none = {n: None for n in _PTRS if n in [f[0] for f in _args(which)._fields_] and n != "workspace"}
    a = _args(which, lib, B=0, **none)
    if which == "infonce":
        a.workspace = FAKE
    assert fn(ctypes.byref(a), None) == 0, lib.ur_last_error()
    # N == 0 is legal and needs no neg; it is refused only further on, by nothing (the fake pointers are never followed: B = 0)
    assert fn(ctypes.byref(_args(which, lib, B=0, N=0, neg=None)), None) == 0


def _need(lib, **over):
    a = _args("infonce", None, **over)
    a.workspace, a.workspace_bytes = None, -1
    assert lib.ur_mrl_infonce(ctypes.byref(a), None) == 0, lib.ur_last_error()
    return a.workspace_bytes


def test_size_query_fills_workspace_bytes_and_grows():
    lib = _lib.load()
    # row losses [K][pad4(B)] + w pad4(K * B * (N + 1)) + partial sums [B][16][sum d_k], floats
    assert _need(lib) == 4 * (3 * 4 + 72 + 3 * 16 * 48)
    base = _need(lib)
    assert _need(lib, B=4) > base and _need(lib, N=8) > base
    assert _need(lib, dims=(4, 16, 32)) > base and _need(lib, dims=(4, 12, 20, 32)) > base
    assert _need(lib, dims=(32,)) == 4 * (4 + 24 + 3 * 16 * 32)
    assert _need(lib, B=0) == 0
    # the query needs no pointer at all, and still refuses what the call refuses
    a = _args("infonce", None, **{n: None for n in _PTRS})
    assert lib.ur_mrl_infonce(ctypes.byref(a), None) == 0 and a.workspace_bytes == base
    for over, word in ((dict(K=9), b"K"), (dict(dims=(4, 10, 32)), b"dims"), (dict(weights=(0.0, 0.0, 0.0)), b"weights"),
                       (dict(temperature=0.0), b"temperature")):
        a = _args("infonce", None, workspace=None, **over)
        a.workspace_bytes = 123
        assert lib.ur_mrl_infonce(ctypes.byref(a), None) < 0 and word in lib.ur_last_error() and a.workspace_bytes == 123


# ---- the float64 reference against the reference's own loss on slices --------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(mrl_ref.MRL_CASES))
def test_reference_reproduces_the_fixture(golden_dir, case):
    """f32 arithmetic of the reference's InfoNCELoss against float64: 1e-6 relative"""
    g = mrl_ref.load_fixture(golden_dir)
    user, pos, neg, mask = mrl_ref.mrl_case_inputs(case)
    c = mrl_ref.MRL_CASES[case]
    assert user.shape == (c["B"], c["D"]) and neg.shape == (c["B"], c["N"], c["D"]) and (mask is None) == (not c["mask"])
    if mask is not None:
        assert bool(mask.any(1).all()) and not bool(mask.all())
    for wname, weights in mrl_ref.MRL_WEIGHTS.items():
        loss, plane, du = mrl_ref.infonce(user, pos, neg, mask, mrl_ref.MRL_DIMS, weights, mrl_ref.MRL_TAU)
        np.testing.assert_allclose(plane.numpy(), g[f"{case}/plane_loss"], rtol=1e-6, atol=0)
        np.testing.assert_allclose(float(loss), float(g[f"{case}/{wname}/loss"]), rtol=1e-6, atol=0)
        want = g[f"{case}/{wname}/d_user"]
        np.testing.assert_allclose(du.numpy(), want, rtol=0, atol=1e-6 * float(np.abs(want).max()))
        if weights[1] == 0.0 and weights[2] != 0:          # the zero-weight plane left the gradient: columns 4..11 are plane 2's alone
            _, _, du2 = mrl_ref.infonce(user, pos, neg, mask, mrl_ref.MRL_DIMS, (0.0, 0.0, weights[2]), mrl_ref.MRL_TAU)
            assert torch.equal(du[:, 4:], du2[:, 4:])


def test_fixture_holds_outputs_only(golden_dir):
    g = np.load(os.path.join(golden_dir, "mrl_tiny.npz"))
    assert sorted(g.files) == mrl_ref.fixture_keys()
    assert os.path.getsize(os.path.join(golden_dir, "mrl_tiny.npz")) < 16 * 1024


def test_single_plane_reference_is_the_heads_reference():
    user, pos, neg, mask = mrl_ref.mrl_case_inputs("masked")
    D = user.shape[1]
    for dtype in (F64, F32):
        loss, plane, du = mrl_ref.infonce(user, pos, neg, mask, (D,), (1.0,), 0.07, 0.5, dtype)
        l1, du1 = ref64.infonce(user, pos, neg, mask, 0.07, 0.5, dtype)
        assert torch.equal(loss, l1) and torch.equal(plane[0], l1) and torch.equal(du, du1)
        assert torch.equal(mrl_ref.scores(user, pos, neg, (D,), dtype)[0], ref64.cosine_scores(user, pos, neg, dtype))
    s = mrl_ref.scores(user, pos, neg, mrl_ref.MRL_DIMS)
    assert s.shape == (3, 3, 8)
    assert torch.equal(mrl_ref.ranks(s, mask), torch.stack([ref64.mrr_rank(s[k], mask) for k in range(3)]))


# ---- Python-level refusals: all before any device call -----------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """every launch wrapper the Matryoshka surface could reach fails if touched, and so does loading the library"""
    from unirec_amd import hip

    def touched(*a, **k):
        raise AssertionError("a device call was made")
    for name in ("mrl_scores", "mrl_infonce", "cosine_scores", "infonce_fwd_bwd", "mrr_rank", "catalog_softmax", "catalog_select", "catalog_scores"):
        monkeypatch.setattr(hip, name, touched)
    monkeypatch.setattr(_lib, "load", touched)


BAD_DIMS = [(), (4, 6, 32), (0, 32), (-4, 32), (8, 8, 32), (16, 8, 32), tuple(range(4, 40, 4)), (4.0, 32), "32", 32, (True, 32)]
BAD_WEIGHTS = [(1.0, -1.0, 1.0), (1.0, float("nan"), 1.0), (1.0, float("inf"), 1.0), (0.0, 0.0, 0.0), (1.0, 1.0), (1.0, 1.0, 1.0, 1.0), "abc", 1.0]


def test_loss_keywords_are_refused_by_name(no_device):
    from unirec_amd.joint import InfoNCELoss, JointTrainer, MultiModalTrainer
    for make in (lambda **k: InfoNCELoss(0.07, **k), lambda **k: MultiModalTrainer(0.07, **k),
                 lambda **k: JointTrainer(None, None, **k)):
        for bad in BAD_DIMS:
            with pytest.raises(ValueError, match="matryoshka_dims"):
                make(matryoshka_dims=bad)
        for bad in BAD_WEIGHTS:
            with pytest.raises(ValueError, match="matryoshka_weights"):
                make(matryoshka_dims=(4, 12, 32), matryoshka_weights=bad)
        with pytest.raises(ValueError, match="matryoshka_weights"):
            make(matryoshka_weights=(1.0, 1.0))                       # weights without dims
    for make in (lambda **k: MultiModalTrainer(0.07, **k), lambda **k: JointTrainer(None, None, **k)):
        with pytest.raises(ValueError, match="catalog_softmax.*matryoshka_dims"):
            make(loss="catalog_softmax", matryoshka_dims=(4, 12, 32))
    with pytest.raises(ValueError, match="temperature"):
        InfoNCELoss(0.0, matryoshka_dims=(4, 32))
    # accepted: the defaults, the normalised forms
    assert InfoNCELoss().matryoshka_dims is None and MultiModalTrainer().infonce_loss.matryoshka_dims is None
    ok = InfoNCELoss(0.07, matryoshka_dims=[4, 12, 32])
    assert ok.matryoshka_dims == (4, 12, 32) and ok.matryoshka_weights == (1.0, 1.0, 1.0) and ok.last_plane_loss is None
    assert MultiModalTrainer(matryoshka_dims=(4, 32), matryoshka_weights=[0, 2]).infonce_loss.matryoshka_weights == (0.0, 2.0)


def test_last_dim_is_checked_against_the_embeddings_at_the_first_call(no_device):
    from unirec_amd.joint import InfoNCELoss, mrr_ranks
    from unirec_amd.evaluation import MRREvaluator
    u, p, n = torch.zeros(2, 16), torch.zeros(2, 16), torch.zeros(2, 3, 16)
    with pytest.raises(ValueError, match="matryoshka_dims"):
        InfoNCELoss(0.07, matryoshka_dims=(4, 12, 32))(u, p, n)
    with pytest.raises(ValueError, match="dims"):
        mrr_ranks(u, p, n, dims=(4, 32))
    with pytest.raises(ValueError, match="dims"):
        mrr_ranks(u, p, n, dims=(4, 6, 16))
    with pytest.raises(ValueError, match="dims"):
        MRREvaluator.ranks_from_embeddings(u, p, [n[0], n[1]], dims=(8, 12))


def test_truncated_refuses_a_bad_dim_by_name(no_device):
    from unirec_amd.evaluation import CatalogEvaluator
    ev = CatalogEvaluator(torch.arange(5 * 16, dtype=torch.float32).reshape(5, 16), item_ids=list("abcde"), device="cpu")
    for bad in (0, -4, 6, 20, 8.0, True, None):
        with pytest.raises(ValueError, match="dim"):
            ev.truncated(bad)
    for dtype in (torch.float32, torch.bfloat16):
        ev = CatalogEvaluator(torch.arange(5 * 16, dtype=torch.float32).reshape(5, 16), item_ids=list("abcde"), device="cpu", dtype=dtype)
        t = ev.truncated(8)
        assert t.catalog.shape == (5, 8) and t.catalog.is_contiguous() and t.catalog.dtype == dtype and t._inv is None
        assert torch.equal(t.catalog, ev.catalog[:, :8]) and t.item_ids == ev.item_ids
        assert t.catalog.data_ptr() != ev.catalog.data_ptr()
        assert ev.truncated(16).catalog.shape == (5, 16)


def test_wrappers_refuse_host_tensors_and_bad_arguments():
    from unirec_amd import hip
    u, p, n = torch.zeros(2, 16), torch.zeros(2, 16), torch.zeros(2, 3, 16)
    with pytest.raises(_lib.UniRecHipError, match="no CPU fallback"):
        hip.mrl_scores(u, p, n, (4, 16))
    with pytest.raises(_lib.UniRecHipError, match="no CPU fallback"):
        hip.mrl_infonce(u, p, n, None, (4, 16))
    assert hip.mrl_dims([4, 16], D=16) == (4, 16) and hip.mrl_weights(None, 3) == (1.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="dims"):
        hip.mrl_dims((4, 16), D=32)

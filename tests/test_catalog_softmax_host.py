"""CPU: the host side of the full-catalogue softmax loss -- the float64 reference against torch autograd, the three rules
include/unirec_hip_loss.h is held to (declared <=> exported <=> bound, and a float64 test named for every entry point), the argument
checks and the size query of ur_catalog_softmax through the raw library (fake non-null pointers: every call here returns before any
launch), and the trainers' refusals."""
import ast
import ctypes
import os
import re
import types

import pytest
import torch

from tests.catalog_softmax_ref import autograd_ref, catalog_softmax_ref
from unirec_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 256          # non-null, 16-byte aligned, never dereferenced on the host
GPU_TESTS = "tests/test_gpu_catalog_softmax.py"


# ---- the reference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,D,tau,E", [(1, 1, 4, 0.07, 0), (3, 50, 8, 1.0, 0), (5, 300, 16, 0.07, 4), (4, 200, 12, 0.01, 9)])
def test_reference_matches_float64_autograd(B, N, D, tau, E):
    g = torch.Generator().manual_seed(B + 7 * N)
    user, cat = torch.randn(B, D, generator=g), torch.randn(N, D, generator=g)
    gt = torch.randint(0, N, (B,), generator=g)
    exclude = None
    if E:
        exclude = torch.randint(-1, N, (B, E), generator=g)
        exclude[:, 0] = gt                   # the user's own ground truth: never dropped
        exclude[:, 1] = exclude[:, 2]        # a duplicate
    ref = catalog_softmax_ref(user, cat, gt, tau, exclude, grad_scale=0.5)
    loss, du = autograd_ref(user, cat, gt, tau, exclude, grad_scale=0.5)
    assert abs(float(ref["loss"] - loss)) <= 1e-13 * max(1.0, abs(float(loss)))
    scale = float(du.abs().max())
    assert float((ref["d_user"] - du).abs().max()) <= 1e-12 * max(scale, 1e-300), (float((ref["d_user"] - du).abs().max()), scale)
    assert bool(ref["keep"].gather(1, gt[:, None]).all())
    if N == 1:
        assert float(ref["loss"]) == 0.0 and scale <= 1e-12
    if E:
        assert int((~ref["keep"]).sum()) > 0
        full = catalog_softmax_ref(user, cat, gt, tau, None, grad_scale=0.5)
        assert float(full["loss"]) >= float(ref["loss"]), "dropping rows shrinks the sum"
        assert tau < 0.07 or float(full["loss"]) > float(ref["loss"])      # (at tau = 0.01 the dropped terms may lie below 1e-16 of it)


def test_reference_widens_bf16_exactly():
    g = torch.Generator().manual_seed(2)
    user, cat = torch.randn(3, 8, generator=g), torch.randn(40, 8, generator=g).to(torch.bfloat16)
    gt = torch.tensor([0, 39, 7])
    a, b = catalog_softmax_ref(user, cat, gt, 0.07), catalog_softmax_ref(user, cat.float(), gt, 0.07)
    assert torch.equal(a["row_loss"], b["row_loss"]) and torch.equal(a["d_user"], b["d_user"])


# ---- the header: declared <=> exported <=> bound, and a float64 test per entry point -----------------------------------------------
def _declared():
    src = open(os.path.join(ROOT, "include", "unirec_hip_loss.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ur_[a-z0-9_]+)\s*\(", src)))


def test_loss_header_symbols_are_bound_and_exported():
    names = _declared()
    assert "ur_catalog_softmax" in names
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in unirec_hip_loss.h but not exported by libunirec_hip.so"
        assert n in _lib.LOSS_SIGNATURES, f"{n} declared in unirec_hip_loss.h but not bound in unirec_amd/_lib.py"
    extra = set(_lib.LOSS_SIGNATURES) - set(names)
    assert not extra, f"bound but not declared in the loss header: {extra}"
    assert not set(_lib.LOSS_SIGNATURES) & set(_lib.SIGNATURES), "a name belongs to one header"
    loaded = _lib.load()
    for n in names:
        assert getattr(loaded, n).argtypes == _lib.LOSS_SIGNATURES[n][1], f"load() did not bind {n}"
    assert _lib.ABI_VERSION >= 20 and loaded.ur_version() == _lib.ABI_VERSION      # (the loss header arrived with ABI 20)


def test_every_loss_entry_point_has_a_float64_test():
    with open(os.path.join(ROOT, GPU_TESTS)) as f:
        tree = ast.parse(f.read())
    covers = None
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "COVERS" for t in node.targets):
            covers = ast.literal_eval(node.value)
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    assert isinstance(covers, dict), f"{GPU_TESTS} has no top-level COVERS dict"
    assert sorted(covers) == _declared(), "COVERS lists exactly the entry points of unirec_hip_loss.h"
    for entry, names in covers.items():
        assert names, f"COVERS[{entry!r}] names no test"
        for name in names:
            assert name in tests, f"COVERS[{entry!r}] names {name}, which does not exist"


def test_struct_mirror_matches_the_header_field_order():
    src = open(os.path.join(ROOT, "include", "unirec_hip_loss.h")).read()
    body = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    body = body[body.index("typedef struct {") + len("typedef struct {"):body.index("} ur_catalog_softmax_t;")]
    fields = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in _lib.CatalogSoftmax._fields_]


# ---- ur_catalog_softmax: checks and size query --------------------------------------------------------------------------------------
def _args(**over):
    a = _lib.CatalogSoftmax()
    a.user = a.catalog = a.cat_inv_norm = a.gt_index = a.loss = a.row_loss = a.lse = a.d_user = FAKE
    a.B, a.N, a.D = 4, 5000, 16
    a.temperature, a.grad_scale = 0.07, 1.0
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _query(lib, **over):
    a = _args(**over)
    assert lib.ur_catalog_softmax(ctypes.byref(a), None) == 0, lib.ur_last_error()
    return a.workspace_bytes


def test_argument_checks_reject_before_any_launch():
    lib = _lib.load()
    need = _query(lib)
    assert need > 0

    def rejected(word, **over):
        for ws in (dict(), dict(workspace=FAKE, workspace_bytes=need)):      # a size query checks the sizes too
            a = _args(**ws, **over)
            rc = lib.ur_catalog_softmax(ctypes.byref(a), None)
            msg = lib.ur_last_error()
            assert rc < 0 and b"ur_catalog_softmax" in msg and word in msg, (over, rc, msg)

    rejected(b"temperature", temperature=0.0)
    rejected(b"temperature", temperature=-0.07)
    rejected(b"temperature", temperature=float("nan"))
    rejected(b"chunk_rows", chunk_rows=1000)
    rejected(b"chunk_rows", chunk_rows=-1024)
    rejected(b"scorer", scorer=3)
    rejected(b"scorer", scorer=-1)
    rejected(b"catalog_bf16", catalog_bf16=2)
    rejected(b"catalog_bf16", catalog_bf16=-1)
    rejected(b"exclude", E=3)                                                # E > 0 with exclude NULL
    rejected(b"exclude", E=-1, exclude=FAKE)
    rejected(b"D", D=6)
    rejected(b"D", D=2052)
    rejected(b"N", N=2 ** 31)
    rejected(b"N", N=0)
    # with a workspace: one byte short, misaligned, a null operand
    for over, word in ((dict(workspace=FAKE, workspace_bytes=need - 1), b"workspace"), (dict(workspace=FAKE + 4, workspace_bytes=need + 64), b"workspace"),
                       (dict(workspace=FAKE, workspace_bytes=need, gt_index=None), b"null"), (dict(workspace=FAKE, workspace_bytes=need, lse=None), b"null"),
                       (dict(workspace=FAKE, workspace_bytes=need, user=FAKE + 4), b"aligned")):
        a = _args(**over)
        rc = lib.ur_catalog_softmax(ctypes.byref(a), None)
        assert rc < 0 and b"ur_catalog_softmax" in lib.ur_last_error() and word in lib.ur_last_error(), (over, rc, lib.ur_last_error())
    # inside the limits: the size queries succeed
    for over in (dict(N=2 ** 31 - 1), dict(N=1), dict(D=2048), dict(D=4), dict(chunk_rows=1024), dict(E=3, exclude=FAKE), dict(d_user=None)):
        assert _query(lib, **over) > 0
    for scorer in (0, 1, 2):
        for bf in (0, 1):
            assert _query(lib, scorer=scorer, catalog_bf16=bf) == need, "the scorer and the catalogue type do not size the workspace"
    assert lib.ur_catalog_softmax(None, None) < 0
    # B == 0 with a workspace: nothing to do, nothing launched
    a = _args(B=0, workspace=FAKE, workspace_bytes=1 << 20)
    assert lib.ur_catalog_softmax(ctypes.byref(a), None) == 0


def test_size_query():
    lib = _lib.load()
    a = _args(workspace_bytes=-7)
    assert lib.ur_catalog_softmax(ctypes.byref(a), None) == 0 and a.workspace_bytes > 0
    # the chunk buffer of select mode (the catalogue rounded up to the 1024-score tile, per user) and then some; no pass 2, no slabs
    fwd = _query(lib, d_user=None)
    assert 4 * 5120 * 4 <= fwd < 4 * 5120 * 4 + 4096
    assert _query(lib) > fwd
    assert 4 * 1024 * 4 <= _query(lib, d_user=None, chunk_rows=1024) < 4 * 1024 * 4 + 4096
    # at catalogue scale the size does not grow with N, and it is no [B,N] buffer
    B, D = 512, 1024
    big4, big8 = _query(lib, B=B, N=4_000_000, D=D), _query(lib, B=B, N=8_000_000, D=D)
    assert big4 == big8
    assert big4 < B * 4_000_000 * 4
    assert big4 <= 256 << 20, "chunk buffer near 64 MB plus the partial [B,D] slabs"
    for Bx in (16, 64):
        assert _query(lib, B=Bx, N=4_000_000, D=D) == _query(lib, B=Bx, N=8_000_000, D=D) < Bx * 4_000_000 * 4


# ---- the trainers' refusals: before the library, the model or the device is touched ---------------------------------------------------
def _no_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_library)


def test_trainer_refusals(monkeypatch):
    from unirec_amd.joint import CatalogSoftmaxLoss, JointTrainer, MultiModalTrainer
    from unirec_amd.negatives import CatalogCandidates
    _no_library(monkeypatch)
    cat = torch.randn(30, 8, generator=torch.Generator().manual_seed(1))
    args = types.SimpleNamespace(learning_rate=1e-3, max_steps=2)
    for make in (lambda **kw: MultiModalTrainer(0.07, **kw), lambda **kw: JointTrainer(None, args, **kw)):
        with pytest.raises(ValueError, match="negatives"):
            make(loss="catalog_softmax")
        with pytest.raises(ValueError, match="num_random"):
            make(negatives=CatalogCandidates(cat, num_random=4), loss="catalog_softmax")
        with pytest.raises(ValueError, match="num_hard"):
            make(negatives=CatalogCandidates(cat, num_hard=2), loss="catalog_softmax")
        with pytest.raises(ValueError, match="softmax_over_everything"):
            make(negatives=CatalogCandidates(cat), loss="softmax_over_everything")
    tr = MultiModalTrainer(0.07, CatalogCandidates(cat), loss="catalog_softmax")
    assert isinstance(tr.catalog_softmax_loss, CatalogSoftmaxLoss) and tr.catalog_softmax_loss.evaluator is tr.negatives.evaluator

    def model(**kw):
        raise AssertionError("the model ran")
    base = {"input_ids": None, "attention_mask": None, "history_field_embeddings": None, "history_attention_mask": None}
    with pytest.raises(ValueError, match="positive_item_index"):
        tr.compute_loss(model, dict(base))
    for key in ("negative_item_index", "negative_masks", "positive_item_embeddings", "negative_item_embeddings"):
        with pytest.raises(ValueError, match=key):
            tr.compute_loss(model, dict(base, positive_item_index=torch.tensor([1]), **{key: torch.zeros(1)}))
    # the default stays InfoNCE, with or without a catalogue
    assert MultiModalTrainer().loss == "infonce" and MultiModalTrainer(0.07, CatalogCandidates(cat)).catalog_softmax_loss is None


def test_loss_module_arguments(monkeypatch):
    from unirec_amd.evaluation import CatalogEvaluator
    from unirec_amd.joint import CatalogSoftmaxLoss
    _no_library(monkeypatch)
    cat = torch.randn(30, 8, generator=torch.Generator().manual_seed(1))
    ev = CatalogEvaluator(cat, device="cpu")
    assert CatalogSoftmaxLoss(ev).evaluator is ev and CatalogSoftmaxLoss(ev).temperature == 0.07
    assert CatalogSoftmaxLoss(cat.to(torch.bfloat16)).catalog.dtype == torch.bfloat16
    for bad in (dict(scorer="MFMA"), dict(temperature=0.0), dict(temperature=-1.0)):
        with pytest.raises(ValueError):
            CatalogSoftmaxLoss(cat, **bad)
    with pytest.raises(ValueError):
        CatalogSoftmaxLoss(cat.to(torch.float16))
    with pytest.raises(ValueError):
        CatalogSoftmaxLoss(cat[0])

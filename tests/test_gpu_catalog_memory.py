"""GPU: WHERE the catalogue entry points read and write.  Their own test modules hold the values on fresh, 512-byte-aligned torch
allocations and zeroed or recycled workspaces; here every call goes through the raw C ABI with every pointer placed by tests/arena.py:

  * at the weakest alignment its header allows (user, catalog, workspace, d_user: a 256-byte boundary + 16; int64 operands + 8; everything
    else + 4 -- so cat_inv_norm + c0, the output lists and the rank are 4-byte aligned and nothing more);
  * between two 64 KiB guards: 0x5A around outputs and integer inputs, 0xFF (NaN) around floating-point inputs, so a row read behind the
    last catalogue row or the last user is a NaN in a score, and a store one row past a list is a changed guard byte;
  * with the workspace at exactly the queried size, its interior 0xFF in one run and 0x00 in another.

Every case asserts: (1) rc == 0; (2) every guard of every output, input and workspace intact, and the inputs themselves unchanged;
(3) every output element the header says is written no longer holds 0x5A5A5A5A -- rank, cat_inv_norm when it was not ready,
user_inv_norm, lse, row_loss and plane_loss included; (4) the outputs equal, bit for bit, what the hip.* wrapper returns for the same
arguments on ordinary tensors; (5) they pass the reference check of the entry point's own test module (the numpy lists of
test_gpu_catalog_select / test_gpu_catalog_deep on the plain call's scores, the float64 band of test_gpu_catalog_coarse, _hold with
_bounds of test_gpu_catalog_softmax, _hold_planes of test_gpu_catalog_mrl_softmax) -- (4) alone would compare the code with itself;
(6) the 0xFF run and the 0x00 run agree in every bit of every output; (7) a workspace one byte short, and one at a 256-byte boundary
+ 8, is refused with rc < 0 and "workspace" in ur_last_error, every output byte still 0x5A.  No tolerance is new: (4) and (6) are bit
equalities and (5) reuses bounds those modules derive.

Workspace regions: written before read, and by which launch (read off catalog_layout.hip.h and the kernels that take the offsets; the
poison confirms the reading, it does not replace it).  "first" is the flag of the first chunk of a stream.

  select_layout (ur_catalog_scores, select mode)
    chunk [B][rows]        catalog_scores_kernel / catalog_scores_mfma_kernel store [B][len] (ld = len) of every chunk before
                           catalog_select_kernel reads row[n], n < len; the tail of a short last chunk is never read
    ref [B]                catalog_gt_score_kernel (prologue), only with gt_index; read by catalog_select_kernel only with gt_index
    (outputs as state)     topk_score / topk_index / rank are the running state: catalog_select_kernel reads them only when !first
  deep_layout (ur_catalog_deep_select)
    chunk, ref             as above; the reader is catalog_deep_sweep_kernel
    inv_u [B]              row_inv_norm_kernel (prologue) before the scoring launches read it
    list_score/index       catalog_deep_sweep_kernel loads them only when !first; on the first chunk EVERY workgroup (b, g) -- one without
      [B][gw][K]           rows included, it does not take the early return -- starts from empty lists and stores all K entries of its slot.
                           The launch uses G <= gw slots per user with stride G; catalog_deep_merge_kernel reads the same G slots.
    count [B][gw]          catalog_deep_sweep_kernel: (first ? 0 : count) + ..., only with gt_index; the merge reads it only with rank
  coarse_layout / coarse_deep_layout / funnel_select_layout
    user~ [B][D] bf16      ur_cast_f32_to_bf16 (cast_prefix_kernel for the funnel) writes all B D elements before the norm and the scorer
    inv_u [B]              row_inv_norm_kernel<bf16> on user~
    ref [B]                the diagonal launch of catalog_scores_bf16_kernel (gt != NULL) stores ref[b] for every b < B, only with gt_index
    chunk                  catalog_scores_bf16(_prefix)_kernel, [B][len] with ld = len, before the selection kernel
    lists, counts          as deep_layout
  ur_catalog_rerank        inv_u [B]: row_inv_norm_kernel before catalog_rerank_kernel
  deep_rerank_layout / funnel_rerank_layout
    inv_u [B]              row_inv_norm_kernel / row_prefix_inv_norm_kernel
    score [B][K_in]        catalog_deep_rerank_score_kernel stores every (b, slot), -inf for an empty slot; the sort kernel reads a score
                           only for an index inside [0, N)
  catalog_softmax_layout / catalog_mrl_softmax_layout (per plane)
    chunk                  the scoring launch of each pass before the fold / weight kernel; the weight kernel rewrites [b][n], n < len, in
                           place before catalog_softmax_grad_kernel reads the same range
    inv_u, ref             prologue (row_inv_norm / row_prefix_inv_norm, catalog_gt_score(_prefix)_kernel); gt_index is mandatory
    m_run, l_run           catalog_softmax_fold_kernel: first ? (-inf, 0) : slot, for segments with and without rows
      [B][CSM_SEGS]
    t_run [B][CSM_SEGS]    catalog_softmax_weight_kernel: first ? 0 : slot, likewise (pass 2 only)
    slabs [nsplit][B][D]   catalog_softmax_grad_kernel: on the first chunk every split -- one without rows stores zeros -- STORES all B x D of its
                           slab; later chunks add.  catalog_softmax_duser_kernel / catalog_mrl_duser_kernel read nsplit slabs.  Without
                           d_user the region has size 0 and pass 2 does not run.
  ur_catalog_prefix_norms and the plain ur_catalog_scores take no workspace.

No region is read before it is written, so nothing in unirec_amd/csrc had to change for this module."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import arena  # noqa: E402
from tests import catalog_coarse_ref as cref  # noqa: E402
from tests import ref64  # noqa: E402
from tests.catalog_softmax_ref import catalog_softmax_ref  # noqa: E402
from tests.test_gpu_catalog_coarse import _bound, _case as _coarse_case, _gathered_error, _hold_band, _rerank_case  # noqa: E402
from tests.test_gpu_catalog_deep import _reference as _deep_reference  # noqa: E402
from tests.test_gpu_catalog_mrl_softmax import _hold_planes  # noqa: E402
from tests.test_gpu_catalog_select import _reference as _select_reference  # noqa: E402
from tests.test_gpu_catalog_softmax import _bounds, _hold  # noqa: E402
from unirec_amd import _lib, hip  # noqa: E402
from unirec_amd.evaluation import pack_exclude  # noqa: E402

DEV = "cuda"
F32, BF16, I32, I64 = torch.float32, torch.bfloat16, torch.int32, torch.int64
B0, N0, D0, E0, CHUNK = 17, 2049, 264, 9, 1024          # a ragged user block, a ragged K step, three chunks with a one-row last chunk
TAU, GRAD_SCALE = 0.07, 0.5
ALIGN16 = ("user", "catalog", "d_user")                 # what the headers call 16-byte aligned (and the workspace)

COVERS = {
    "ur_catalog_scores": ["test_plain_scores", "test_select_mode"],
    "ur_catalog_deep_select": ["test_deep_select"],
    "ur_catalog_coarse_select": ["test_coarse_select"],
    "ur_catalog_coarse_deep_select": ["test_coarse_deep_select"],
    "ur_catalog_rerank": ["test_rerank"],
    "ur_catalog_deep_rerank": ["test_deep_rerank"],
    "ur_catalog_prefix_norms": ["test_prefix_norms"],
    "ur_catalog_funnel_select": ["test_funnel_select"],
    "ur_catalog_funnel_rerank": ["test_funnel_rerank"],
    "ur_catalog_softmax": ["test_softmax"],
    "ur_catalog_mrl_softmax": ["test_mrl_softmax"],
}


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _name(dtype):
    return "f32" if dtype is F32 else "bf16"


def _norm_bound(d):
    """relative error of an inverse row norm over d components against float64: a lane's chain is 4 roundings deep per 256-element piece
    (square, the sum inside the piece, the accumulation), then six tree levels, the root and the division, each 2^-24 relative on a sum
    of non-negative terms"""
    return (4 * ((d + 255) // 256) + 6 + 2) * 2.0 ** -24


def _norms_hold(inv, rows, d):
    i64 = 1.0 / rows[:, :d].double().norm(dim=1).clamp_min(1e-12)
    assert float(((inv.double() - i64).abs() / i64).max()) <= _norm_bound(d), d


# ---- one raw call with every pointer in an arena --------------------------------------------------------------------------------------
class Run:
    """rc, the error text and the arenas {name: (whole, view)} of one raw call; `inputs` keeps what was placed, to see it unchanged"""

    def __init__(self):
        self.rc, self.error, self.arenas, self.inputs, self.outputs, self.need = None, "", {}, {}, {}, 0


def _run(spec, interior=arena.NAN, short=0, ws_align=16):
    """spec: entry, struct (class), scalars {field: value}, arrays {field: values}, inputs {name: tensor}, outputs {name: (shape, dtype)},
    call(lib, ptr, a) -> rc, workspace (bool).  The size query first; then the call with the workspace at exactly the queried size less
    `short` bytes, at a 256-byte boundary + ws_align."""
    lib = _lib.load()
    r = Run()
    a = spec["struct"]()
    for k, v in spec["scalars"].items():
        setattr(a, k, v)
    for k, v in spec.get("arrays", {}).items():
        getattr(a, k)[:len(v)] = list(v)
    ptr = {}
    for name, t in spec["inputs"].items():
        align = 16 if name in ALIGN16 else 8 if t.dtype == I64 else 4
        fill = arena.NAN if t.is_floating_point() else arena.OUT
        whole, view = arena.place(t.to(DEV), align, fill)
        r.arenas[name], r.inputs[name], ptr[name] = (whole, view), t.to(DEV).clone(), view.data_ptr()
    for name, (shape, dtype) in spec["outputs"].items():
        nbytes = 4 * int(np.prod(shape))
        whole, raw = arena.place(nbytes, 16 if name in ALIGN16 else 4, arena.OUT, device=DEV)
        view = arena.typed(raw, dtype, tuple(shape))
        r.arenas[name], r.outputs[name], ptr[name] = (whole, view), view, view.data_ptr()
    fields = {f[0] for f in a._fields_}
    for name, p in ptr.items():
        if name in fields:
            setattr(a, name, p)
    stream = hip._stream()
    if spec.get("workspace", True):
        a.workspace, a.workspace_bytes = None, 0
        assert spec["call"](lib, ptr, a, stream) == 0, lib.ur_last_error()
        r.need = int(a.workspace_bytes)
        assert r.need >= 16
        whole, view = arena.place(r.need - short, ws_align, arena.OUT, device=DEV, interior=interior)
        r.arenas["workspace"] = (whole, view)
        a.workspace, a.workspace_bytes = view.data_ptr(), r.need - short
    r.rc = spec["call"](lib, ptr, a, stream)
    torch.cuda.synchronize()
    r.error = lib.ur_last_error().decode("utf-8", "replace") if r.rc != 0 else ""
    return r


def _struct_call(entry):
    return lambda lib, ptr, a, stream: getattr(lib, entry)(ctypes.byref(a), stream)


def _memory_contract(spec, wrapper, reference):
    """assertions 1 - 7 of the module docstring.  wrapper() -> {output name: tensor} from the hip.* wrapper on ordinary tensors;
    reference(outs) asserts the entry point's own reference check on {output name: tensor}."""
    runs = [_run(spec, interior) for interior in ((arena.NAN, arena.ZERO) if spec.get("workspace", True) else (arena.NAN,))]
    for r in runs:
        assert r.rc == 0, (r.rc, r.error)                                                                      # 1
        for name, (whole, view) in r.arenas.items():                                                           # 2
            assert arena.intact(whole, view), f"{spec['entry']}: a guard of {name} was written"
        for name, t in r.inputs.items():
            assert torch.equal(r.arenas[name][1].reshape(-1).view(torch.uint8), t.reshape(-1).view(torch.uint8)), f"input {name} was written"
        for name, view in r.outputs.items():                                                                   # 3
            assert arena.all_written(view), f"{spec['entry']}: {name} keeps elements nobody stored"
    outs = {name: view.clone() for name, view in runs[0].outputs.items()}
    for r in runs[1:]:                                                                                          # 6
        for name, view in r.outputs.items():
            assert torch.equal(_bits(view), _bits(outs[name])), f"{spec['entry']}: {name} depends on what the workspace held"
    want = wrapper()                                                                                            # 4
    assert set(want) <= set(outs) and want, "the wrapper's outputs are outputs of the raw call"
    for name, t in want.items():
        assert t.shape == outs[name].shape and t.dtype == outs[name].dtype, name
        assert torch.equal(_bits(t), _bits(outs[name])), f"{spec['entry']}: {name} differs from the wrapper's"
    reference(outs)                                                                                             # 5
    if spec.get("workspace", True):                                                                             # 7
        for kw in (dict(short=1), dict(ws_align=8)):
            r = _run(spec, arena.OUT, **kw)
            assert r.rc < 0 and "workspace" in r.error, (kw, r.rc, r.error)
            for name, (whole, view) in r.arenas.items():
                if name in r.outputs or name == "workspace":
                    assert arena.untouched(whole), f"{spec['entry']}: a refused call wrote {name}"
                else:
                    assert arena.intact(whole, view), name
    return outs


# ---- the exact selects ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _exact_case(B, N, D, dtype):
    """user, catalogue, gt, the exclusion rows (raw lists and packed), and S = the plain call's scores on the host"""
    g = torch.Generator().manual_seed(7 + B + 3 * N + 7 * D)
    user = torch.randn(B, D, generator=g).to(DEV)
    cat = torch.randn(N, D, generator=g).to(dtype).to(DEV)
    gt = torch.randint(0, N, (B,), generator=g)
    raw = torch.randint(0, N, (B, E0), generator=g)
    raw[::3, 0] = -1
    raw[1::2, E0 - 1] = gt[1::2]
    S = hip.catalog_scores(user, cat.float())[0].cpu().numpy()
    return dict(user=user, cat=cat, gt=gt, raw=raw, packed=pack_exclude(raw, B).to(DEV), S=S)


def _lists_reference(reference, c, K):
    def check(outs):
        idx, val, rank = reference(c["S"], K, c["gt"].numpy(), c["raw"].numpy())
        assert torch.equal(outs["topk_index"].cpu(), idx)
        assert torch.equal(_bits(outs["topk_score"]), _bits(val))
        assert torch.equal(outs["rank"].cpu(), rank)
        if "cat_inv_norm" in outs:
            _norms_hold(outs["cat_inv_norm"], c["cat"], c["cat"].shape[1])
    return check


def _select_io(c, B, N, K):
    return (dict(user=c["user"], catalog=c["cat"], gt_index=c["gt"], exclude=c["packed"]),
            dict(topk_index=((B, K), I32), topk_score=((B, K), F32), rank=((B,), I32), cat_inv_norm=((N,), F32)))


def test_plain_scores():
    """ur_catalog_scores without a select struct: [B, N] scores, both norm outputs; no workspace.  Reference: float64 cosines within the
    bound tests/test_gpu_catalog_coarse.py derives for this f32 chain."""
    for B in (B0, 33):
        c = _exact_case(B, N0, D0, F32)
        spec = dict(entry="ur_catalog_scores", struct=_lib.CatalogSelect, scalars={}, workspace=False,
                    inputs=dict(user=c["user"], catalog=c["cat"]),
                    outputs=dict(scores=((B, N0), F32), user_inv_norm=((B,), F32), cat_inv_norm=((N0,), F32)),
                    call=lambda lib, ptr, a, stream, B=B: lib.ur_catalog_scores(ptr["user"], ptr["catalog"], ptr["scores"], ptr["user_inv_norm"],
                                                                               ptr["cat_inv_norm"], 0, B, N0, D0, None, stream))

        def wrapper(c=c):
            S, cinv = hip.catalog_scores(c["user"], c["cat"])
            return dict(scores=S, cat_inv_norm=cinv)

        def reference(outs, c=c):
            s64 = cref.exact_scores(c["user"].cpu(), c["cat"].cpu())
            assert float((outs["scores"].double().cpu() - s64).abs().max()) <= (2 * (D0 / 64 + 6) + 6) * 2.0 ** -24
            _norms_hold(outs["user_inv_norm"], c["user"], D0)
        _memory_contract(spec, wrapper, reference)


@pytest.mark.parametrize("B,K,dtype,scorer", [(17, 10, F32, "vector"), (17, 128, BF16, "mfma"), (17, 10, BF16, "vector"), (17, 128, F32, "mfma"),
                                              (33, 128, F32, "mfma"), (33, 10, BF16, "mfma")],
                         ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_select_mode(B, K, dtype, scorer):
    c = _exact_case(B, N0, D0, dtype)
    inputs, outputs = _select_io(c, B, N0, K)
    outputs["user_inv_norm"] = ((B,), F32)
    spec = dict(entry="ur_catalog_scores", struct=_lib.CatalogSelect, inputs=inputs, outputs=outputs,
                scalars=dict(K=K, E=E0, chunk_rows=CHUNK, catalog_bf16=int(dtype is BF16), scorer=hip.catalog_scorer_id(scorer)),
                call=lambda lib, ptr, a, stream: lib.ur_catalog_scores(ptr["user"], ptr["catalog"], None, ptr["user_inv_norm"], ptr["cat_inv_norm"],
                                                                       0, B, N0, D0, ctypes.byref(a), stream))

    def wrapper():
        idx, val, rank, cinv = hip.catalog_select(c["user"], c["cat"], K, gt_index=c["gt"], exclude=c["packed"], chunk_rows=CHUNK, scorer=scorer)
        return dict(topk_index=idx, topk_score=val, rank=rank, cat_inv_norm=cinv)
    _memory_contract(spec, wrapper, _lists_reference(_select_reference, c, K))


@pytest.mark.parametrize("K,segments,dtype,scorer", [(129, 1, F32, "vector"), (1000, 3, BF16, "mfma"), (129, 3, BF16, "vector"), (1000, 1, F32, "mfma")],
                         ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_deep_select(K, segments, dtype, scorer):
    c = _exact_case(B0, N0, D0, dtype)
    inputs, outputs = _select_io(c, B0, N0, K)
    spec = dict(entry="ur_catalog_deep_select", struct=_lib.CatalogDeep, inputs=inputs, outputs=outputs, call=_struct_call("ur_catalog_deep_select"),
                scalars=dict(B=B0, N=N0, D=D0, K=K, E=E0, chunk_rows=CHUNK, segments=segments, catalog_bf16=int(dtype is BF16),
                             scorer=hip.catalog_scorer_id(scorer), cat_norm_ready=0))

    def wrapper():
        idx, val, rank, cinv = hip.catalog_deep_select(c["user"], c["cat"], K, gt_index=c["gt"], exclude=c["packed"], chunk_rows=CHUNK,
                                                       scorer=scorer, segments=segments)
        return dict(topk_index=idx, topk_score=val, rank=rank, cat_inv_norm=cinv)
    _memory_contract(spec, wrapper, _lists_reference(_deep_reference, c, K))


# ---- the coarse selects -----------------------------------------------------------------------------------------------------------------
COARSE_SHAPES = [(65, 2049, 264), (33, 1025, 2048)]      # a 64-user group plus one; the 32-user form of D > 1024


def _band_e(c, K):
    """the bound of the band: test_gpu_catalog_coarse._bound up to 128 entries; above, test_coarse_deep_scores_against_float64's -- the
    same yardstick (the exact vector scorer on the rounded users against the same float64 scores) from the long-list entry point"""
    if K <= hip.CATALOG_TOPK_MAX:
        return _bound(c, K)[0]
    yi, yv, _, _ = hip.catalog_deep_select(c["user"].to(BF16).float(), c["cat"], K, gt_index=c["gt"], exclude=c["packed"], scorer="vector")
    return max(4.0 * _gathered_error(yi, yv, c["s64"]), 8.0 * float(ref64.f32_ulp(float(np.abs(c["s64"]).max()))))


def _band_reference(c, K):
    def check(outs):
        e = _band_e(c, K)
        assert _gathered_error(outs["topk_index"], outs["topk_score"], c["s64"]) <= e
        _hold_band(c, K, outs["topk_index"], outs["topk_score"], outs["rank"].cpu().numpy(), e, what="placed")
    return check


def _coarse_io(c, K, ready=None):
    B, N = c["B"], c["N"]
    inputs = dict(user=c["user"], catalog=c["cat"], gt_index=c["gt"], exclude=c["packed"])
    outputs = dict(topk_index=((B, K), I32), topk_score=((B, K), F32), rank=((B,), I32))
    if ready is None:
        outputs["cat_inv_norm"] = ((N,), F32)
    else:
        inputs["cat_inv_norm"] = ready
    return inputs, outputs


@pytest.mark.parametrize("B,N,D", COARSE_SHAPES)
def test_coarse_select(B, N, D):
    c, K = _coarse_case(B, N, D, E0), 128
    inputs, outputs = _coarse_io(c, K)
    spec = dict(entry="ur_catalog_coarse_select", struct=_lib.CatalogCoarse, inputs=inputs, outputs=outputs, call=_struct_call("ur_catalog_coarse_select"),
                scalars=dict(B=B, N=N, D=D, K=K, E=E0, chunk_rows=CHUNK, catalog_bf16=1, cat_norm_ready=0))

    def wrapper():
        idx, val, rank, cinv = hip.catalog_coarse_select(c["user"], c["cat"], K, gt_index=c["gt"], exclude=c["packed"], chunk_rows=CHUNK)
        return dict(topk_index=idx, topk_score=val, rank=rank, cat_inv_norm=cinv)
    _memory_contract(spec, wrapper, _band_reference(c, K))


@pytest.mark.parametrize("K,segments", [(128, 0), (300, 3)])
@pytest.mark.parametrize("B,N,D", COARSE_SHAPES)
def test_coarse_deep_select(B, N, D, K, segments):
    c = _coarse_case(B, N, D, E0)
    inputs, outputs = _coarse_io(c, K)
    spec = dict(entry="ur_catalog_coarse_deep_select", struct=_lib.CatalogCoarseDeep, inputs=inputs, outputs=outputs,
                call=_struct_call("ur_catalog_coarse_deep_select"),
                scalars=dict(B=B, N=N, D=D, K=K, E=E0, chunk_rows=CHUNK, segments=segments, catalog_bf16=1, cat_norm_ready=0))

    def wrapper():
        idx, val, rank, cinv = hip.catalog_coarse_deep_select(c["user"], c["cat"], K, gt_index=c["gt"], exclude=c["packed"], chunk_rows=CHUNK,
                                                              segments=segments)
        return dict(topk_index=idx, topk_score=val, rank=rank, cat_inv_norm=cinv)
    _memory_contract(spec, wrapper, _band_reference(c, K))


FUNNEL_DIM = 40                                          # one full K step and 8 of 32 elements, live data behind it: ld = ldu = 264


@pytest.mark.parametrize("K,segments,ready", [(128, 0, False), (300, 3, True)])
def test_funnel_select(K, segments, ready):
    """the prefix [:40] of the rows of the (65, 2049, 264) case, read in place; the band is taken on the contiguous slices"""
    B, N, D = COARSE_SHAPES[0]
    full = _coarse_case(B, N, D, E0)
    c = dict(full, D=FUNNEL_DIM, user=full["user"][:, :FUNNEL_DIM].contiguous(), cat=full["cat"][:, :FUNNEL_DIM].contiguous(),
             s64=cref.coarse_scores(full["user"][:, :FUNNEL_DIM].cpu(), full["cat"][:, :FUNNEL_DIM].cpu()).numpy())
    norms = hip.catalog_prefix_norms(full["cat"], (FUNNEL_DIM,))[0].contiguous() if ready else None
    inputs, outputs = _coarse_io(full, K, norms)
    spec = dict(entry="ur_catalog_funnel_select", struct=_lib.CatalogFunnelSelect, inputs=inputs, outputs=outputs,
                call=_struct_call("ur_catalog_funnel_select"),
                scalars=dict(B=B, N=N, dim=FUNNEL_DIM, ld=D, ldu=D, K=K, E=E0, chunk_rows=CHUNK, segments=segments, catalog_bf16=1,
                             cat_norm_ready=int(ready)))

    def wrapper():
        idx, val, rank, cinv = hip.catalog_funnel_select(full["user"], full["cat"], FUNNEL_DIM, K, cat_inv_norm=norms, gt_index=full["gt"],
                                                         exclude=full["packed"], chunk_rows=CHUNK, segments=segments)
        out = dict(topk_index=idx, topk_score=val, rank=rank)
        return out if ready else dict(out, cat_inv_norm=cinv)
    _memory_contract(spec, wrapper, _band_reference(c, K))


# ---- the re-ranks and the norms ---------------------------------------------------------------------------------------------------------
def _rerank_reference(user, cat, index, k, D):
    """tests/test_gpu_catalog_coarse.py's criteria: the total order on the plain call's score bits, those bits, the float64 bound of the
    chain"""
    def check(outs):
        N = cat.shape[0]
        S = hip.catalog_scores(user, cat.float())[0].cpu().numpy()
        s64 = cref.exact_scores(user.cpu(), cat.cpu()).numpy()
        bound = (2 * (D / 64 + 6) + 6) * 2.0 ** -24
        idx_np, val_np, idx_host = outs["topk_index"].cpu().numpy(), outs["topk_score"].cpu().numpy(), index.cpu().numpy()
        for b in range(user.shape[0]):
            row = idx_host[b][(idx_host[b] >= 0) & (idx_host[b] < N)]
            o = row[cref.order(S[b, row], row)][:k]
            assert idx_np[b, :len(o)].tolist() == o.tolist(), b
            assert (val_np[b, :len(o)].view(np.int32) == S[b, o].view(np.int32)).all(), (b, "score bits")
            assert (idx_np[b, len(o):] == -1).all() and np.isneginf(val_np[b, len(o):]).all()
            assert np.abs(val_np[b, :len(o)].astype(np.float64) - s64[b, o]).max(initial=0.0) <= bound
        _norms_hold(outs["cat_inv_norm"], cat, D)
    return check


def _rerank_spec(entry, struct, user, cat, index, k, dtype, **dims):
    B, K_in, N = user.shape[0], index.shape[1], cat.shape[0]
    return dict(entry=entry, struct=struct, call=_struct_call(entry), inputs=dict(user=user, catalog=cat, index=index),
                outputs=dict(topk_index=((B, k), I32), topk_score=((B, k), F32), cat_inv_norm=((N,), F32)),
                scalars=dict(B=B, N=N, K_in=K_in, k=k, catalog_bf16=int(dtype is BF16), cat_norm_ready=0, **dims))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
def test_rerank(dtype):
    user, cat, index = _rerank_case(B0, N0, D0, 128, dtype)
    spec = _rerank_spec("ur_catalog_rerank", _lib.CatalogRerank, user, cat, index, 10, dtype, D=D0)

    def wrapper():
        idx, val, cinv = hip.catalog_rerank(user, cat, index, 10)
        return dict(topk_index=idx, topk_score=val, cat_inv_norm=cinv)
    _memory_contract(spec, wrapper, _rerank_reference(user, cat, index, 10, D0))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
@pytest.mark.parametrize("K_in", [128, 129])
def test_deep_rerank(K_in, dtype):
    user, cat, index = _rerank_case(B0, N0, D0, K_in, dtype)
    spec = _rerank_spec("ur_catalog_deep_rerank", _lib.CatalogDeepRerank, user, cat, index, 10, dtype, D=D0)

    def wrapper():
        idx, val, cinv = hip.catalog_deep_rerank(user, cat, index, 10)
        return dict(topk_index=idx, topk_score=val, cat_inv_norm=cinv)
    _memory_contract(spec, wrapper, _rerank_reference(user, cat, index, 10, D0))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
@pytest.mark.parametrize("K_in", [128, 129])
def test_funnel_rerank(K_in, dtype):
    user, cat, index = _rerank_case(B0, N0, D0, K_in, dtype)
    spec = _rerank_spec("ur_catalog_funnel_rerank", _lib.CatalogFunnelRerank, user, cat, index, 10, dtype, dim=FUNNEL_DIM, ld=D0, ldu=D0)

    def wrapper():
        idx, val, cinv = hip.catalog_funnel_rerank(user, cat, index, FUNNEL_DIM, 10)
        return dict(topk_index=idx, topk_score=val, cat_inv_norm=cinv)
    u_d, c_d = user[:, :FUNNEL_DIM].contiguous(), cat[:, :FUNNEL_DIM].contiguous()
    _memory_contract(spec, wrapper, _rerank_reference(u_d, c_d, index, 10, FUNNEL_DIM))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
def test_prefix_norms(dtype):
    N, ld, dims = 1025, 264, (8, 40, 264)
    g = torch.Generator().manual_seed(ld + len(dims))
    cat = torch.randn(N, ld, generator=g)
    cat[3, :dims[0]] = 0.0                                 # a row whose narrowest prefix is all zero: the 1e-12 clamp
    cat = cat.to(dtype).to(DEV)
    spec = dict(entry="ur_catalog_prefix_norms", struct=_lib.CatalogPrefixNorms, call=_struct_call("ur_catalog_prefix_norms"), workspace=False,
                inputs=dict(catalog=cat), outputs=dict(inv=((len(dims), N), F32)), arrays=dict(dims=dims),
                scalars=dict(catalog_bf16=int(dtype is BF16), N=N, ld=ld, L=len(dims)))

    def reference(outs):
        for l, d in enumerate(dims):
            _norms_hold(outs["inv"][l], cat, d)
        assert 0.99e12 < float(outs["inv"][0, 3]) < 1.01e12
    _memory_contract(spec, lambda: dict(inv=hip.catalog_prefix_norms(cat, dims)), reference)


# ---- the losses -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _loss_case(B, N, D, dtype):
    g = torch.Generator().manual_seed(B + 3 * N + 7 * D + 11 * E0)
    user = torch.randn(B, D, generator=g).to(DEV)
    C = torch.randn(N, D, generator=g).to(DEV).to(dtype)
    gt = torch.randint(0, N, (B,), generator=g)
    raw = torch.randint(0, N, (B, E0), generator=g)
    raw[0::2, 0] = gt[0::2]                               # the user's own ground truth, a duplicated entry, -1 padding
    raw[:, 1] = raw[:, 2]
    raw[:, E0 - 1] = -1
    raw[1::2, 3] = -1
    return user, C, gt, raw, pack_exclude(raw, B).to(DEV)


@pytest.mark.parametrize("dtype,scorer,grad", [(F32, "vector", True), (BF16, "mfma", True), (F32, "mfma", False), (BF16, "vector", False)],
                         ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_softmax(dtype, scorer, grad):
    user, C, gt, raw, ex = _loss_case(B0, N0, D0, dtype)
    outputs = dict(loss=((1,), F32), row_loss=((B0,), F32), lse=((B0,), F32), cat_inv_norm=((N0,), F32))
    if grad:
        outputs["d_user"] = ((B0, D0), F32)
    spec = dict(entry="ur_catalog_softmax", struct=_lib.CatalogSoftmax, call=_struct_call("ur_catalog_softmax"),
                inputs=dict(user=user, catalog=C, gt_index=gt, exclude=ex), outputs=outputs,
                scalars=dict(B=B0, N=N0, D=D0, E=E0, chunk_rows=CHUNK, catalog_bf16=int(dtype is BF16), scorer=hip.catalog_scorer_id(scorer),
                             cat_norm_ready=0, temperature=TAU, grad_scale=GRAD_SCALE))

    def wrapper():
        loss, row_loss, lse, d_user, cinv = hip.catalog_softmax(user, C, gt, TAU, exclude=ex, chunk_rows=CHUNK, scorer=scorer,
                                                                grad_scale=GRAD_SCALE, need_grad=grad)
        out = dict(loss=loss, row_loss=row_loss, lse=lse, cat_inv_norm=cinv)
        return dict(out, d_user=d_user) if grad else out

    def reference(outs):
        ref = catalog_softmax_ref(user, C, gt, TAU, raw, GRAD_SCALE)
        _hold("placed", (outs["loss"], outs["row_loss"], outs["lse"], outs.get("d_user")), ref, _bounds(user, C, gt, TAU, ref, GRAD_SCALE))
    _memory_contract(spec, wrapper, reference)


MRL_WEIGHTS = (0.75, 0.0, 1.5)                          # general weights, a plane of weight 0 among them


@pytest.mark.parametrize("B,dims,dtype,scorer,grad", [(17, (8, 256, 264), F32, "vector", True), (17, (8, 256, 264), BF16, "mfma", True),
                                                      (17, (8, 256, 264), F32, "mfma", False), (17, (8, 256, 264), BF16, "vector", False),
                                                      (16, (64, 256, 1024), F32, "mfma", True), (16, (64, 256, 1024), BF16, "mfma", True)],
                         ids=lambda v: _name(v) if isinstance(v, torch.dtype) else "_".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_mrl_softmax(B, dims, dtype, scorer, grad):
    """(8, 256, 264): a prefix inside the first piece, on a piece boundary, the ragged width; (64, 256, 1024) with the MFMA scorer: the
    three-plane group kernel"""
    D, K = dims[-1], len(dims)
    user, C, gt, raw, ex = _loss_case(B, N0, D, dtype)
    outputs = dict(loss=((1,), F32), plane_loss=((K,), F32), row_loss=((K, B), F32), lse=((K, B), F32), cat_inv_norm=((K, N0), F32))
    if grad:
        outputs["d_user"] = ((B, D), F32)
    spec = dict(entry="ur_catalog_mrl_softmax", struct=_lib.CatalogMrlSoftmax, call=_struct_call("ur_catalog_mrl_softmax"),
                inputs=dict(user=user, catalog=C, gt_index=gt, exclude=ex), outputs=outputs, arrays=dict(dims=dims, weights=MRL_WEIGHTS),
                scalars=dict(B=B, N=N0, D=D, E=E0, K=K, chunk_rows=CHUNK, catalog_bf16=int(dtype is BF16), scorer=hip.catalog_scorer_id(scorer),
                             cat_norm_ready=0, temperature=TAU, grad_scale=GRAD_SCALE))

    def wrapper():
        loss, plane_loss, row_loss, lse, d_user, norms = hip.catalog_mrl_softmax(user, C, gt, dims, MRL_WEIGHTS, TAU, exclude=ex, chunk_rows=CHUNK,
                                                                                 scorer=scorer, grad_scale=GRAD_SCALE, need_grad=grad)
        out = dict(loss=loss, plane_loss=plane_loss, row_loss=row_loss, lse=lse, cat_inv_norm=norms)
        return dict(out, d_user=d_user) if grad else out

    def reference(outs):
        got = (outs["loss"], outs["plane_loss"], outs["row_loss"], outs["lse"], outs.get("d_user"), outs["cat_inv_norm"])
        _hold_planes("placed", got, user, C, gt, raw, dims, MRL_WEIGHTS, TAU, GRAD_SCALE)
    _memory_contract(spec, wrapper, reference)

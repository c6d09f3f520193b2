"""GPU: WHERE the three entry points of include/unirec_fp8.h read and write, as tests/test_gpu_catalog_memory.py asks of the older
catalogue calls.  Every call goes through the raw C ABI with every pointer placed by tests/arena.py:

  * at the weakest alignment the header allows (src, user, codes, workspace: a 256-byte boundary + 16; int64 operands + 8; everything else
    -- scale, inv, cat_inv_norm, index, the output lists, the rank -- + 4);
  * between two 64 KiB guards: 0x5A around outputs and integer inputs, 0xFF around floating-point inputs and around the codes (NaN as f32,
    the NaN code as e4m3), so a row read behind the last one is a NaN in a score and a store past an output is a changed guard byte;
  * with the workspace at exactly the queried size, its interior 0xFF in one run and 0x00 in another.

Every case asserts: rc == 0; every guard intact and every input unchanged; no output word still 0x5A5A5A5A; the outputs equal, bit for
bit, what the hip.* wrapper returns on ordinary tensors, and pass the reference check of tests/test_gpu_catalog_fp8.py (the quantiser's
bits, catalog_coarse_ref.select on the scores rebuilt slice by slice, hip.catalog_deep_rerank on codes.float()); the two poisons agree
in every bit; a workspace one byte short, and one at a 256-byte boundary + 8, is refused with "workspace" in ur_last_error and every
output byte still 0x5A.

Workspace regions (fp8_select_layout, catalog_layout.hip.h): q [B][D], iu8 [B] and the user scales [B] are written by
catalog_fp8_quantize_kernel (every row b < B, every element) before the scorer stages them; ref [B] by the diagonal launch, only with
gt_index; chunk [B][len] by catalog_scores_fp8_kernel before the sweep reads row[n], n < len; lists and counts as in deep_layout.  The
re-rank: iu [B] by row_inv_norm_kernel, score [B][K_in] by catalog_fp8_rerank_score_kernel for every (b, slot).  No region is read
before it is written."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import arena  # noqa: E402
from tests import catalog_coarse_ref as cref  # noqa: E402
from tests import catalog_fp8_ref as ref  # noqa: E402
from tests.test_gpu_catalog_fp8 import _all_scores  # noqa: E402
from unirec_amd import _lib, hip  # noqa: E402

DEV = "cuda"
F32, BF16, I32, I64, U8 = torch.float32, torch.bfloat16, torch.int32, torch.int64, torch.uint8
B0, N0, D0, E0, CHUNK = 17, 2049, 272, 9, 1024          # a ragged user block, a ragged K pair, three chunks with a one-row last chunk
ALIGN16 = ("src", "user", "codes")

COVERS = {
    "ur_catalog_fp8_quantize": ["test_quantize"],
    "ur_catalog_fp8_select": ["test_select"],
    "ur_catalog_fp8_rerank": ["test_rerank"],
}


def _bits(t):
    t = t.detach().contiguous()
    return (t if t.dtype == U8 else t.view(I32)).cpu()


class Run:
    def __init__(self):
        self.rc, self.error, self.arenas, self.inputs, self.outputs, self.need = None, "", {}, {}, {}, 0


def _run(entry, struct, scalars, inputs, outputs, workspace=True, interior=arena.NAN, short=0, ws_align=16):
    """one raw call: inputs {field: tensor}, outputs {field: (shape, dtype)}; the size query first, then the call with the workspace at
    exactly the queried size less `short` bytes, at a 256-byte boundary + ws_align"""
    lib = _lib.load()
    fn = getattr(lib, entry)
    r = Run()
    a = struct()
    for k, v in scalars.items():
        setattr(a, k, v)
    for name, t in inputs.items():
        align = 16 if name in ALIGN16 else 8 if t.dtype == I64 else 4
        fill = arena.NAN if (t.is_floating_point() or t.dtype == U8) else arena.OUT
        whole, view = arena.place(t.to(DEV), align, fill)
        r.arenas[name], r.inputs[name] = (whole, view), t.to(DEV).clone()
        setattr(a, name, view.data_ptr())
    for name, (shape, dtype) in outputs.items():
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        whole, raw = arena.place(nbytes, 16 if name in ALIGN16 else 4, arena.OUT, device=DEV)
        view = arena.typed(raw, dtype, tuple(shape))
        r.arenas[name], r.outputs[name] = (whole, view), view
        setattr(a, name, view.data_ptr())
    stream = hip._stream()
    if workspace:
        a.workspace, a.workspace_bytes = None, 0
        assert fn(ctypes.byref(a), stream) == 0, lib.ur_last_error()
        r.need = int(a.workspace_bytes)
        assert r.need >= 16
        whole, view = arena.place(r.need - short, ws_align, arena.OUT, device=DEV, interior=interior)
        r.arenas["workspace"] = (whole, view)
        a.workspace, a.workspace_bytes = view.data_ptr(), r.need - short
    r.rc = fn(ctypes.byref(a), stream)
    torch.cuda.synchronize()
    r.error = lib.ur_last_error().decode("utf-8", "replace") if r.rc != 0 else ""
    return r


def _memory_contract(spec, wrapper, reference):
    """the assertions of the module docstring.  wrapper() -> {output name: tensor} on ordinary tensors; reference(outs) asserts the entry
    point's reference check on {output name: tensor}"""
    ws = spec.get("workspace", True)
    runs = [_run(**spec, interior=interior) for interior in ((arena.NAN, arena.ZERO) if ws else (arena.NAN,))]
    for r in runs:
        assert r.rc == 0, (r.rc, r.error)
        for name, (whole, view) in r.arenas.items():
            assert arena.intact(whole, view), f"{spec['entry']}: a guard of {name} was written"
        for name, t in r.inputs.items():
            assert torch.equal(r.arenas[name][1].reshape(-1).view(U8), t.reshape(-1).view(U8)), f"input {name} was written"
        for name, view in r.outputs.items():
            assert arena.all_written(view), f"{spec['entry']}: {name} keeps elements nobody stored"
    outs = {name: view.clone() for name, view in runs[0].outputs.items()}
    for r in runs[1:]:
        for name, view in r.outputs.items():
            assert torch.equal(_bits(view), _bits(outs[name])), f"{spec['entry']}: {name} depends on what the workspace held"
    want = wrapper()
    assert set(want) <= set(outs) and want
    for name, t in want.items():
        assert t.shape == outs[name].shape and t.dtype == outs[name].dtype, name
        assert torch.equal(_bits(t), _bits(outs[name])), f"{spec['entry']}: {name} differs from the wrapper's"
    reference(outs)
    if ws:
        for kw in (dict(short=1), dict(ws_align=8)):
            r = _run(**spec, interior=arena.OUT, **kw)
            assert r.rc < 0 and "workspace" in r.error, (kw, r.rc, r.error)
            for name, (whole, view) in r.arenas.items():
                if name in r.outputs or name == "workspace":
                    assert arena.untouched(whole), f"{spec['entry']}: a refused call wrote {name}"


def _operands(seed=3):
    g = torch.Generator().manual_seed(seed)
    cat = torch.randn(N0, D0, generator=g) * torch.exp2(torch.randint(-5, 5, (N0, 1), generator=g).float())
    user = torch.randn(B0, D0, generator=g)
    gt = torch.randint(0, N0, (B0,), generator=g)
    gt[0], gt[1] = N0 - 1, 0                                     # the one-row last chunk and the first row
    user[:4] = cat[gt[:4]] + 0.05 * torch.randn(4, D0, generator=g)
    exclude = torch.sort(torch.randint(-3, N0, (B0, E0), generator=g).clamp_min(-1), dim=1).values
    codes, scale, inv = hip.catalog_fp8_quantize(cat.to(DEV))
    return cat, user, gt, exclude, codes, scale, inv


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_quantize(dtype):
    g = torch.Generator().manual_seed(9)
    N, D, ld = 1027, D0, D0 + 20
    src = (torch.randn(N, ld, generator=g) * torch.exp2(torch.randint(-9, 9, (N, 1), generator=g).float())).to(dtype)
    src[5, :D] = 0
    spec = dict(entry="ur_catalog_fp8_quantize", struct=_lib.CatalogFp8Quantize, scalars=dict(src_bf16=int(dtype is BF16), N=N, D=D, ld=ld),
                inputs=dict(src=src), outputs=dict(codes=((N, D), U8), scale=((N,), F32), inv=((N,), F32)), workspace=False)

    def wrapper():
        return dict(zip(("codes", "scale", "inv"), hip.catalog_fp8_quantize(src.to(DEV)[:, :D])))

    def reference(outs):
        rc, rs, ri = ref.quantize(src[:, :D])
        assert np.array_equal(outs["codes"].cpu().numpy(), rc)
        assert np.array_equal(outs["scale"].cpu().numpy().view(np.uint32), rs.view(np.uint32))
        assert np.array_equal(outs["inv"].cpu().numpy().view(np.uint32), ri.view(np.uint32))
    _memory_contract(spec, wrapper, reference)


@pytest.mark.parametrize("with_gt", [True, False], ids=["gt", "nogt"])
def test_select(with_gt):
    cat, user, gt, exclude, codes, scale, inv = _operands()
    K = 300
    inputs = dict(user=user, codes=codes.cpu(), cat_inv_norm=inv.cpu(), exclude=exclude)
    outputs = dict(topk_index=((B0, K), I32), topk_score=((B0, K), F32))
    if with_gt:
        inputs["gt_index"] = gt
        outputs["rank"] = ((B0,), I32)
    spec = dict(entry="ur_catalog_fp8_select", struct=_lib.CatalogFp8Select, scalars=dict(B=B0, N=N0, D=D0, K=K, E=E0, chunk_rows=CHUNK),
                inputs=inputs, outputs=outputs)

    def wrapper():
        idx, val, rank = hip.catalog_fp8_select(user.to(DEV), codes, K, inv, gt_index=gt if with_gt else None, exclude=exclude.to(DEV),
                                                chunk_rows=CHUNK)
        out = dict(topk_index=idx, topk_score=val)
        if with_gt:
            out["rank"] = rank
        return out

    def reference(outs):
        scores = torch.empty(B0, N0)
        for c0 in range(0, N0, 1024):
            c1 = min(N0, c0 + 1024)
            scores[:, c0:c1] = _all_scores(user.to(DEV), codes[c0:c1].contiguous(), inv[c0:c1].contiguous())
        widx, wval, wrank = cref.select(scores.numpy().astype(np.float64), K, gt.numpy() if with_gt else None, exclude.numpy())
        assert np.array_equal(outs["topk_index"].cpu().numpy(), widx)
        assert np.array_equal(outs["topk_score"].cpu().numpy().astype(np.float64), wval)
        if with_gt:
            assert np.array_equal(outs["rank"].cpu().numpy(), wrank) and (wrank[:4] == 1).all()
    _memory_contract(spec, wrapper, reference)


def test_rerank():
    cat, user, gt, exclude, codes, scale, inv = _operands()
    g = torch.Generator().manual_seed(4)
    K_in, k = 300, 200
    index = torch.randint(0, N0, (B0, K_in), generator=g).to(I32)
    index[:, 3], index[2, 5], index[:, 7], index[0, 0] = -1, N0, index[:, 6], N0 - 1
    spec = dict(entry="ur_catalog_fp8_rerank", struct=_lib.CatalogFp8Rerank, scalars=dict(B=B0, N=N0, D=D0, K_in=K_in, k=k),
                inputs=dict(user=user, codes=codes.cpu(), cat_inv_norm=inv.cpu(), index=index),
                outputs=dict(topk_index=((B0, k), I32), topk_score=((B0, k), F32)))

    def wrapper():
        idx, val = hip.catalog_fp8_rerank(user.to(DEV), codes, index.to(DEV), inv, k)
        return dict(topk_index=idx, topk_score=val)

    def reference(outs):
        widx, wval, _ = hip.catalog_deep_rerank(user.to(DEV), codes.view(torch.float8_e4m3fn).float(), index.to(DEV), k, inv.clone())
        assert torch.equal(outs["topk_index"], widx) and torch.equal(_bits(outs["topk_score"]), _bits(wval))
    _memory_contract(spec, wrapper, reference)

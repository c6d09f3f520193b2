"""GPU: the LoRA adapter kernels at the ranks 8, 32 and 64 (rank 16 has tests/test_gpu_primitives.py), dropout included.

Primitives (ur_lora_project / ur_lora_reduce / ur_lora_bgrad and ur_gemm's masked epilogue) are held against float64 products of the
SAME bf16 inputs with the kernels' own flags (hip.lora_bits_to_keep), at the bounds the rank-16 tests use: the arithmetic is the same
-- exact bf16 x bf16 products, f32 accumulation, one bf16 rounding for P:
    bf16 outputs t / tb      max|err| <= 6e-3 * max|want| + 1e-3
    f32 outputs dA / dB      max|err| <= 1e-4 * max|want| + 2e-3
    masked GEMM epilogue     max|err| <= 2e-2 * max|want| + 2e-2
Shapes are the smallest that reach each edge: a lone row, row counts that are no multiple of 16 / of the 128-token block, the minimum
width, a tail of the 128-column chunk, several chunks, column ranges with ld != width, one and three adapters.

The decoder step (2 layers of the 0.6B shape at M = 4096, where the projections reach the persistent GEMM; and a small decoder whose
launches are all generic tiles and partial token blocks) is held against the CPU oracle with LoRA dropout ON and the kernels' own
masks, at the bounds tests/test_gpu_switches.py uses for the same comparison at rank 16; rank 16 runs through the same test as the
control, and its launch plan is asserted literally."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import qwen3_ref as Q  # noqa: E402
from oracle import weights as W  # noqa: E402
from tests.parity_utils import GRAD_REL, OUT_REL, assert_close  # noqa: E402

DEV = "cuda"
RANKS = [8, 32, 64]
BF = torch.bfloat16


def _bf(t):
    return t.to(DEV).to(BF)


def _check(got, want, rel, ab, what):
    err = (got.double() - want).abs().max().item()
    bound = rel * want.abs().max().item() + ab
    print(f"  {what}: max|err| = {err:.3e} (bound {bound:.3e})")
    assert torch.isfinite(got).all(), what
    assert err <= bound, f"{what}: max|err| {err:.3e} > {bound:.3e}"


def _t_bound(got, want, what):
    _check(got, want, 6e-3, 1e-3, what)


def _g_bound(got, want, what):
    _check(got, want, 1e-4, 2e-3, what)


# ---- primitives ------------------------------------------------------------------------------------
@pytest.mark.parametrize("W_", [8, 136, 1024])
@pytest.mark.parametrize("M", [1, 37, 300])
@pytest.mark.parametrize("r", RANKS)
def test_project_shared_input(r, M, W_):
    """t = dropout_a(x) A_a^T for one and three adapters that share x, with and without bit planes; deterministic."""
    from unirec_amd import hip
    g = torch.Generator().manual_seed(1000 * r + M + W_)
    x = _bf(torch.randn(M, W_ + 8, generator=g))[:, :W_]                    # ld != width
    for nad in (1, 3):
        A = [_bf(torch.randn(r, W_, generator=g) * 0.2) for _ in range(nad)]
        if nad == 3:
            A[1] = A[0]                                                      # same U, another plane
        for p in (0.0, 0.3):
            bits = hip.lora_dropout_bits(11 + nad, p, M, W_, nad, DEV) if p > 0 else None
            keep = hip.lora_bits_to_keep(bits, W_).double() if p > 0 else torch.ones((nad, M, W_), dtype=torch.float64, device=DEV)
            got = hip.lora_project(x, A, alpha=1.0 / (1 - p), bits=bits)
            assert got.shape == (M, nad * r)
            want = torch.cat([(x.double() * keep[a] / (1 - p)) @ A[a].double().t() for a in range(nad)], 1)
            _t_bound(got, want, f"project r={r} M={M} W={W_} nad={nad} p={p}")
            assert torch.equal(got, hip.lora_project(x, A, alpha=1.0 / (1 - p), bits=bits))
            if nad == 3 and p > 0 and M * W_ >= 4096:
                assert not torch.equal(got[:, :r], got[:, r:2 * r])          # one plane per adapter
            if nad == 3 and p == 0:
                assert torch.equal(got[:, :r], got[:, r:2 * r])


@pytest.mark.parametrize("M", [200, 4100])
@pytest.mark.parametrize("r", RANKS)
def test_project_and_reduce_over_column_ranges(r, M):
    """Adapters that own column ranges of one activation (shared = 0): tb_a = s * dy_a B_a and dB_a = dy_a^T t_a (transposed dense
    output); the activation is a view of a wider tensor."""
    from unirec_amd import hip
    g = torch.Generator().manual_seed(5 + r)
    cols, Wt = [(0, 256), (256, 128), (384, 72)], 456
    dy = _bf(torch.randn(M, Wt + 8, generator=g))[:, :Wt]
    B = [_bf(torch.randn(n, r, generator=g) * 0.2) for _, n in cols]
    t = _bf(torch.randn(M, 3 * r, generator=g))
    Bt = [hip.transpose_bf16(b) for b in B]
    tb = hip.lora_project(dy, Bt, cols=cols, alpha=2.0)
    want = torch.cat([2.0 * dy[:, c0:c0 + n].double() @ B[a].double() for a, (c0, n) in enumerate(cols)], 1)
    _t_bound(tb, want, f"project/cols r={r} M={M}")
    assert torch.equal(tb, hip.lora_project(dy, Bt, cols=cols, alpha=2.0))
    gB = torch.full((Wt, r), float("nan"), device=DEV)
    hip.lora_reduce(dy, t, gB, cols=cols, transposed=True)
    want = torch.cat([dy[:, c0:c0 + n].double().t() @ t[:, a * r:(a + 1) * r].double() for a, (c0, n) in enumerate(cols)], 0)
    _g_bound(gB, want, f"reduce/cols (dB) r={r} M={M}")
    again = torch.empty_like(gB)
    hip.lora_reduce(dy, t, again, cols=cols, transposed=True)
    assert torch.equal(gB, again)


@pytest.mark.parametrize("W_", [128, 200])
@pytest.mark.parametrize("M", [37, 300, 1111, 1024])
@pytest.mark.parametrize("r", RANKS)
def test_reduce_shared_input(r, M, W_):
    """dA_a = tb_a^T dropout_a(x), masked and not, one and three adapters; deterministic.  M = 1024 (a multiple of 128, widths of 64):
    the launch the rank-16 ring kernel would take -- with the token-packed flags supplied the register-staged kernel still runs (asserted
    on the library's own answer, hip.lora_plan, for the very tensors of the launch)."""
    from unirec_amd import hip
    g = torch.Generator().manual_seed(7 * r + M + W_)
    x = _bf(torch.randn(M, W_ + 8, generator=g))[:, :W_]
    for nad in (1, 3):
        tb = _bf(torch.randn(M, nad * r, generator=g))
        for p in (0.0, 0.3):
            bits = hip.lora_dropout_bits(77 + nad, p, M, W_, nad, DEV) if p > 0 else None
            keep = hip.lora_bits_to_keep(bits, W_).double() if p > 0 else torch.ones((nad, M, W_), dtype=torch.float64, device=DEV)
            want = torch.cat([tb[:, a * r:(a + 1) * r].double().t() @ (x.double() * keep[a] / (1 - p)) for a in range(nad)], 0)
            gA = torch.full((nad * r, W_), float("nan"), device=DEV)
            hip.lora_reduce(x, tb, gA, nad=nad, alpha=1.0 / (1 - p), bits=bits)
            _g_bound(gA, want, f"reduce r={r} M={M} W={W_} nad={nad} p={p}")
            again = torch.empty_like(gA)
            hip.lora_reduce(x, tb, again, nad=nad, alpha=1.0 / (1 - p), bits=bits)
            assert torch.equal(gA, again)
            if p > 0 and M % 128 == 0:
                bt = hip.lora_bits_transpose(bits, W_)
                with_t = torch.full_like(gA, float("nan"))
                plan = hip.lora_plan("reduce", hip.lora_reduce_args(x, tb, with_t, nad=nad, alpha=1.0 / (1 - p), bits=bits, bits_t=bt))
                assert plan["kernel"] == "staged" and plan["masked"], plan
                hip.lora_reduce(x, tb, with_t, nad=nad, alpha=1.0 / (1 - p), bits=bits, bits_t=bt)
                _g_bound(with_t, want, f"reduce with bits_t r={r} M={M} W={W_} nad={nad}")
                assert torch.equal(with_t, gA)                              # the same kernel: bits_t is not consumed


@pytest.mark.parametrize("cols", [[(0, 64)], [(0, 128), (128, 64), (256, 192)], [(64, 256), (320, 128)]], ids=["1x64", "3", "2off"])
@pytest.mark.parametrize("M", [200, 1024, 4100])
@pytest.mark.parametrize("r", RANKS)
def test_bgrad(r, M, cols):
    """tb = s * dy_a B_a and dB_a = dy_a^T t_a from one pass over dy; ragged token counts, ranges that do not start at 0; deterministic."""
    from unirec_amd import hip
    g = torch.Generator().manual_seed(M + r)
    Wt = max(c0 + n for c0, n in cols)
    dy = _bf(torch.randn(M, Wt + 8, generator=g))[:, :Wt]
    B = [_bf(torch.randn(n, r, generator=g) * 0.2) for _, n in cols]
    Bt = [hip.transpose_bf16(b) for b in B]
    t = _bf(torch.randn(M, len(cols) * r, generator=g))
    ntot = sum(n for _, n in cols)
    gB = torch.full((ntot, r), float("nan"), device=DEV)
    tb = hip.lora_bgrad(dy, t, Bt, cols, gB, alpha=0.5)
    assert tb.shape == (M, len(cols) * r)
    want_tb = torch.cat([0.5 * dy[:, c0:c0 + n].double() @ B[a].double() for a, (c0, n) in enumerate(cols)], 1)
    want_gB = torch.cat([dy[:, c0:c0 + n].double().t() @ t[:, a * r:(a + 1) * r].double() for a, (c0, n) in enumerate(cols)], 0)
    _t_bound(tb, want_tb, f"bgrad tb r={r} M={M}")
    _g_bound(gB, want_gB, f"bgrad dB r={r} M={M}")
    gB2 = torch.empty_like(gB)
    tb2 = hip.lora_bgrad(dy, t, Bt, cols, gB2, alpha=0.5)
    assert torch.equal(gB, gB2) and torch.equal(tb, tb2)


@pytest.mark.parametrize("r", RANKS)
def test_row_products_do_not_depend_on_the_row_position(r):
    """t (ur_lora_project, one adapter and three that share x, with dropout) and tb (ur_lora_bgrad) of rows [lo, hi) computed alone
    equal the slice of the full launch bit for bit: shard and micro-batch invariance of the model rest on it."""
    from unirec_amd import hip
    g = torch.Generator().manual_seed(21 + r)
    M, K = 4096, 2048
    x = _bf(torch.randn(M, K, generator=g))
    for nad in (1, 3):
        A = [_bf(torch.randn(r, K, generator=g) * 0.2) for _ in range(nad)]
        bits = hip.lora_dropout_bits(5, 0.1, M, K, nad, DEV)
        full = hip.lora_project(x, A, alpha=1.1, bits=bits)
        for lo, hi in ((1024, 2048), (2304, 4096)):
            part = hip.lora_project(x[lo:hi], A, alpha=1.1, bits=bits[:, lo:hi])
            assert torch.equal(part, full[lo:hi])
    cols = [(0, 1024), (1024, 512), (1536, 512)]
    Bt = [_bf(torch.randn(r, n, generator=g) * 0.2) for _, n in cols]
    t = _bf(torch.randn(M, 3 * r, generator=g))
    gB = torch.empty(K, r, device=DEV)
    tb = hip.lora_bgrad(x, t, Bt, cols, gB)
    for lo, hi in ((1024, 2048), (2304, 4096)):
        tbp = hip.lora_bgrad(x[lo:hi], t[lo:hi], Bt, cols, torch.empty_like(gB))
        assert torch.equal(tbp, tb[lo:hi])


@pytest.mark.parametrize("K", [128, 200])
@pytest.mark.parametrize("M", [300, 520])
@pytest.mark.parametrize("r", RANKS)
def test_masked_gemm_epilogue(r, M, K):
    """dx = dy W + sum_a mask_a * (tb_a A_a) / (1 - p): ur_gemm's masked rank-r epilogue, one and three adapters (rank 64 x 3: K2 = 192)."""
    from unirec_amd import hip
    g = torch.Generator().manual_seed(3 + r + M + K)
    p, Nout = 0.3, 136
    dy = _bf(torch.randn(M, Nout, generator=g))
    WT = _bf(torch.randn(K, Nout, generator=g) * 0.1)                       # [in, out] = transposed weight
    for nad in (1, 3):
        A = _bf(torch.randn(nad * r, K, generator=g) * 0.2)
        tb = _bf(torch.randn(M, nad * r, generator=g))
        bits = hip.lora_dropout_bits(1234 + nad, p, M, K, nad, DEV)
        keep = hip.lora_bits_to_keep(bits, K).double()
        got = hip.gemm(dy, WT, R2=tb, S2=hip.transpose_bf16(A), drop=(bits, p, r))
        want = dy.double() @ WT.double().t()
        for a in range(nad):
            want = want + keep[a] / (1 - p) * (tb[:, a * r:(a + 1) * r].double() @ A[a * r:(a + 1) * r].double())
        _check(got, want, 2e-2, 2e-2, f"masked epilogue r={r} M={M} K={K} nad={nad}")
        assert torch.equal(got, hip.gemm(dy, WT, R2=tb, S2=hip.transpose_bf16(A), drop=(bits, p, r)))


def test_unsupported_rank_is_refused_with_the_supported_set():
    from unirec_amd import hip
    x = _bf(torch.randn(64, 128))
    with pytest.raises(ValueError, match="8, 16, 32, 64"):
        hip.lora_project(x, [_bf(torch.randn(24, 128))])


# ---- decoder step against the oracle -------------------------------------------------------------------
PDROP, STEP, SEED, WSEED, T = 0.1, 5, 77, 31, 8
SHAPES = {"big": dict(D=1024, I=3072, nq=16, nkv=8, B=8, S=512), "small": dict(D=256, I=384, nq=2, nkv=1, B=2, S=128)}
GROUPS = ((("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"), "D"), (("self_attn.o_proj",), "NQ"),
          (("mlp.gate_proj", "mlp.up_proj"), "D"), (("mlp.down_proj",), "I"))


def _oracle_cfg(shape, r):
    s = SHAPES[shape]
    return Q.Qwen3Cfg(hidden_size=s["D"], num_hidden_layers=2, num_attention_heads=s["nq"], num_key_value_heads=s["nkv"], head_dim=128,
                      intermediate_size=s["I"], vocab_size=128, lora_r=r, lora_alpha=2.0 * r, lora_dropout=PDROP)


def _weights(qc):
    """oracle.weights tensors for both sides; lora_B ~ N(0, 0.05) so that the adapter path carries weight"""
    rule = lambda k, shp: W.normal(k, shp, WSEED, std=0.05) if k.endswith("lora_B.weight") else None
    return {k: torch.from_numpy(v) for k, v in W.fill_state_dict(Q.qwen3_shapes(qc, lora=True), WSEED, rules=rule).items()}


def _inputs(shape):
    s = SHAPES[shape]
    B, S, D = s["B"], s["S"], s["D"]
    rng = np.random.default_rng(9)
    first = 128 - T
    ids = rng.integers(1, first, size=(B, S))
    am = np.ones((B, S), dtype=np.int64)
    pad = S // 8
    ids[:, :pad], am[:, :pad] = 0, 0                                         # left padding
    for b in range(B):
        ids[b, rng.choice(np.arange(pad, S), size=T, replace=False)] = first + np.arange(T)
    tok = torch.from_numpy(rng.standard_normal((B, T, D)).astype(np.float32) * 0.05).to(BF)
    gvec = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32))
    return torch.from_numpy(ids), torch.from_numpy(am), tok, gvec, first


def _product(shape, r):
    from unirec_amd.qwen3 import Qwen3Config, Qwen3LoRAModel
    s = SHAPES[shape]
    m = Qwen3LoRAModel(Qwen3Config(vocab_size=128, hidden_size=s["D"], intermediate_size=s["I"], num_hidden_layers=2,
                                   num_attention_heads=s["nq"], num_key_value_heads=s["nkv"], head_dim=128,
                                   lora_r=r, lora_alpha=2.0 * r, lora_dropout=PDROP))
    m.reset_parameters(lora_b_std=0.05)
    missing, unexpected = m.load_state_dict(_weights(_oracle_cfg(shape, r)), strict=False)
    assert not unexpected and not missing
    m = m.to(DEV).train()
    m.lora_seed = SEED
    return m


def _masks(m, shape):
    from unirec_amd import hip
    s = SHAPES[shape]
    B, S = s["B"], s["S"]
    width = {"D": s["D"], "NQ": s["nq"] * 128, "I": s["I"]}
    masks = {}
    for i in range(2):
        for g, (names, wkey) in enumerate(GROUPS):
            wd = width[wkey]
            keep = hip.lora_bits_to_keep(hip.lora_dropout_bits(m.lora_dropout_seed(STEP, i, g), PDROP, B * S, wd, len(names), DEV), wd).cpu()
            for slot, nm in enumerate(names):
                masks[f"layers.{i}.{nm}"] = keep[slot].view(B, S, wd)
    return masks


@functools.lru_cache(maxsize=None)
def _oracle(shape, r, train):
    """(pooled, LoRA gradients, token gradient) of the oracle; train: with the kernels' masks of (SEED, STEP), else no dropout, no backward"""
    qc = _oracle_cfg(shape, r)
    P = _weights(qc)
    ids, am, tok, gvec, first = _inputs(shape)
    B = ids.shape[0]
    if not train:
        with torch.no_grad():
            return Q.joint_forward(P, qc, ids, am, tok.float().view(B, 1, T, -1), first).numpy(), None, None
    masks = _masks(_product(shape, r), shape)
    lora = {k: v.requires_grad_(True) for k, v in P.items() if ".lora_" in k}
    toks = tok.float().view(B, 1, T, -1).requires_grad_(True)
    ou = Q.joint_forward(P, qc, ids, am, toks, first, lora_masks=masks)
    (ou * gvec).sum().backward()
    return ou.detach().numpy(), {k: v.grad.numpy() for k, v in lora.items()}, toks.grad.view(B, T, -1).numpy()


def _decoder_step_meets_the_oracle(shape, r, prefetch):
    ou, gl, gt = _oracle(shape, r, True)
    m = _product(shape, r)
    m._lora_step = STEP
    ids, am, tok, gvec, first = _inputs(shape)
    ids, am = ids.to(DEV), am.to(DEV)
    tok = tok.to(DEV).requires_grad_(True)
    if prefetch:          # the planes of the step made on the side stream, as MultiModalQwenEmbedding.forward does
        m.prefetch_lora_bits(ids.numel(), ids.device)
    pooled = m.forward_pooled(ids, am, tok, first)
    pooled.backward(gvec.to(DEV))
    torch.cuda.synchronize()
    what = f"{shape} r={r}"
    assert_close(pooled, ou, OUT_REL, f"[{what}] pooled")
    named = dict(m.named_parameters())
    assert len(gl) == 2 * 7 * 2
    for k in sorted(gl):
        assert tuple(named[k].shape) == ((r, named[k].shape[1]) if "lora_A" in k else (named[k].shape[0], r))
        assert_close(named[k].grad, gl[k], GRAD_REL * 1.5, f"[{what}] grad/{k}")
    assert_close(tok.grad, gt, GRAD_REL * 1.5, f"[{what}] grad/item_tokens")
    return m, ids


@pytest.mark.parametrize("r", RANKS)
def test_decoder_step_with_dropout_meets_the_oracle(r):
    """2 layers of the 0.6B shape, B 8 x S 512 (M = 4096: the projections reach the persistent GEMM), left padding, dropout 0.1."""
    _decoder_step_meets_the_oracle("big", r, prefetch=True)


def test_decoder_step_rank_16_control_and_its_plan():
    """The same step at rank 16, and the launch plan rank 16 has always had at this shape."""
    m, ids = _decoder_step_meets_the_oracle("big", 16, prefetch=True)
    plan = m._plan(ids.numel(), ids.shape[1], ids.device, m._pack, m._frozen)
    assert plan.merged is True
    assert plan.fuse_norm is True
    assert plan.fuse_rope is True
    assert plan.swiglu == "pair"
    assert plan.bits_t is True


@pytest.mark.parametrize("r", RANKS)
def test_small_decoder_train_and_eval(r):
    """hidden 256, 2/1 heads, I 384, B 2 x S 128: every launch a generic tile, every token block partial.  Train mode with dropout
    against the oracle with the kernels' masks; eval mode under no_grad against the oracle without masks."""
    m, ids = _decoder_step_meets_the_oracle("small", r, prefetch=False)
    ou, _, _ = _oracle("small", r, False)
    _, am, tok, _, first = _inputs("small")
    m.eval()
    with torch.no_grad():
        pooled = m.forward_pooled(ids, am.to(DEV), tok.to(DEV), first)
    torch.cuda.synchronize()
    assert_close(pooled, ou, OUT_REL, f"[small r={r}] pooled (eval)")

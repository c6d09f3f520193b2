"""Inputs of the LoRA kernel tests, shared by tests/test_ref64.py (CPU: the criteria accept two summation orders and reject every mutant)
and tests/test_gpu_lora_f64.py (GPU).  Plain torch on the CPU, seeded generators, bf16 values returned as bf16 tensors.

Two families:
  exact    small integers (|x| <= 8, |u|, |v| <= 4; random, so no two columns or tokens are interchangeable), alpha = 2, dropout p = 0.5
           (1 / (1 - p) = 2): every product and every f32 partial sum is an integer below 2^24 (terms of at most 32 each, times 2: up to
           2^18 of them; the launches here have at most 4096, except the 1024-token-block path of ur_lora_bgrad, whose smallest launch is
           one block per CU), exact in ANY summation order -- the kernel must return the correctly rounded exact value bit for bit.
  random   bf16 normals (U at 0.2), p in {0.1, 0.3}, alpha = 1.5 / (1 - p).
Keep masks are oracle/dropout_ref.lora_keep(seed, p, M, W, nad, row0) -- numpy, never the library's unpacker."""
import itertools

import numpy as np
import torch

from oracle import dropout_ref
from unirec_amd import hip

BF16 = torch.bfloat16
FAMILIES = ("exact", "random")
EXACT_P, EXACT_ALPHA, RANDOM_S = 0.5, 2.0, 1.5
MAX_EXACT_TERMS = 2 ** 18            # 2^18 terms * 32 * alpha 2 = 2^24


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(shape, bound, g):
    return torch.randint(-bound, bound + 1, shape, generator=g).to(BF16)


def values(family, shape, g, bound=8, scale=1.0):
    """bf16 tensor of the family: integers in [-bound, bound], or normals at `scale`"""
    return _ints(shape, bound, g) if family == "exact" else (torch.randn(shape, generator=g) * scale).to(BF16)


def case(family, M, W, rank, nad, p=0.0, cols=None, seed=0, row0=0, pad=8):
    """One launch's inputs as a dict.  cols=None: nad adapters share the [M, W] input X (a view of a tensor `pad` columns wider: ld !=
    width), with one keep plane each when p > 0.  cols=[(c0, width), ...]: adapter a owns that column range of X [M, W] (no dropout).
        X [M, W]; U: list of [rank, width_a] (A_a, or B_a^T); V [M, rank nad] (tb, or t); alpha; p; keep [nad, M, W] float64 or None;
        seed, row0: what the planes were drawn with."""
    assert family in FAMILIES and (cols is None or p == 0.0)
    assert family != "exact" or p in (0.0, EXACT_P)
    g = gen(1000003 * seed + 7919 * M + 31 * W + rank + 17 * nad + (1 if family == "exact" else 0))
    X = values(family, (M, W + pad), g)[:, :W]
    widths = [W] * nad if cols is None else [w for _, w in cols]
    assert len(widths) == nad and (family != "exact" or max(max(widths), M) <= MAX_EXACT_TERMS)
    U = [values(family, (rank, w), g, bound=4, scale=0.2) for w in widths]
    V = values(family, (M, rank * nad), g, bound=4)
    alpha = EXACT_ALPHA if family == "exact" else RANDOM_S / (1.0 - p)
    keep = None
    if p > 0.0:
        keep = torch.from_numpy(dropout_ref.lora_keep(seed, p, M, W, nad, row0).astype(np.float64))
    return dict(family=family, M=M, W=W, rank=rank, nad=nad, p=p, cols=cols, seed=seed, row0=row0, X=X, U=U, V=V, alpha=alpha, keep=keep)


def epilogue_case(family, M, N, K, rank, nad, p, seed=0, row0=0):
    """ur_gemm's masked rank-r epilogue: C [M, N] = R S^T + sum_a keep_a / (1 - p) * (tb_a A_a).  R [M, K], S [N, K], tb [M, rank nad],
    A [rank nad, N] (adapter a: rows rank a ..), keep [nad, M, N]."""
    assert family in FAMILIES and (family != "exact" or p == EXACT_P)
    g = gen(7 * seed + 13 * M + N + 101 * rank + nad)
    R = values(family, (M, K), g)
    S = values(family, (N, K), g, bound=4, scale=0.1)
    tb = values(family, (M, rank * nad), g, bound=4)
    A = values(family, (rank * nad, N), g, bound=4, scale=0.2)
    keep = torch.from_numpy(dropout_ref.lora_keep(seed, p, M, N, nad, row0).astype(np.float64))
    return dict(family=family, M=M, N=N, K=K, rank=rank, nad=nad, p=p, seed=seed, row0=row0, R=R, S=S, tb=tb, A=A, keep=keep)


# ---- the launches of tests/test_gpu_lora_f64.py, path by path (csrc/lora.hip: the dispatch of ur_lora_project / _reduce / _bgrad) -----
# A case's "path" label is "<op>/<kernel> ...".  Where a list depends on a rule of the dispatch it ASKS the library (hip.lora_plan: the
# selection function the launches read; no device needed) instead of restating the rule; tests/test_lora_plan.py holds every case of
# every list to the kernel its label names.
RANKS = (8, 16, 32, 64)
ROW0_BIG = 2 ** 33 + 11
STAGED_COLS = [(8, 72), (80, 8), (88, 64)]              # a ragged width, the minimum width, no range starts at 0


def _families(masked, i):
    """(family, p) pairs of launch number i: the exact family at p = 0.5, the random one at 0.1 / 0.3 in turn"""
    return (("exact", EXACT_P if masked else 0.0), ("random", (0.1, 0.3)[i % 2] if masked else 0.0))


def _shared(path, rank, nad, Ms, Ws, masks=(False, True), skip=None):
    i = 0
    for M in Ms:
        for W in Ws:
            if skip is not None and skip(M, W):
                continue
            for masked in masks:
                i += 1
                for family, p in _families(masked, i):
                    c = case(family, M, W, rank, nad, p=p, seed=100 * i + rank + nad, row0=(0, 77, ROW0_BIG)[i % 3])
                    c["path"] = path
                    yield c


def _ranges(path, rank, cols, Ms, transposed=True):
    W = max(c0 + w for c0, w in cols)
    for i, M in enumerate(Ms):
        for family in FAMILIES:
            c = case(family, M, W, rank, len(cols), cols=cols, seed=300 + i + rank)
            c["path"], c["transposed"] = path, transposed
            yield c


def project_staged(rank, nad):
    """register-staged kernel: every rank, 1 .. 4 adapters that share X; a lone rank-16 adapter stays on it through W % 64 != 0"""
    ring = lambda M, W: hip.lora_plan("project", M, W, rank, nad)["kernel"] == "ring"      # noqa: E731
    return _shared("project/staged", rank, nad, (1, 31, 129, 257), (8, 120, 128, 136, 392), skip=ring)


def project_ranges(rank):
    """register-staged kernel over column ranges (one workgroup row per adapter): tb of a merged projection at a ragged width"""
    return _ranges("project/staged ranges", rank, STAGED_COLS, (31, 257))


RING_COLS = [(64, 128), (192, 64), (256, 192)]          # every width % 64 == 0, the first range does not start at 0


def project_ring():
    """LDS-DMA ring kernel: one rank-16 adapter (masked and not), or rank-16 column ranges with every width % 64 == 0"""
    yield from _shared("project/ring", 16, 1, (1, 255, 256, 257, 513), (64, 192, 1024))
    yield from _ranges("project/ring ranges", 16, RING_COLS, (1, 255, 256, 257, 513))


def reduce_staged(rank, nad):
    """register-staged kernel: M <= 128 runs without the slab sum, M = 300 runs three splits; no M here is a multiple of 128"""
    return _shared("reduce/staged", rank, nad, (1, 37, 127, 129, 300), (8, 64, 72, 200))


def reduce_ranges(rank):
    """the transposed output over column ranges (dB of a merged projection), register-staged"""
    return _ranges("reduce/staged ranges", rank, STAGED_COLS, (37, 300))


def reduce_ring_fallback(nad):
    """a ring-eligible shape (rank 16, M % 128 == 0, W % 64 == 0) given bits but NO token-packed bits: the register-staged kernel"""
    return _shared("reduce/staged (no bits_t)", 16, nad, (256,), (64,), masks=(True,))


def reduce_ring(nad):
    """LDS-DMA ring kernel: rank 16, M % 128 == 0, W % 64 == 0; masked launches come with the token-packed flags"""
    return _shared("reduce/ring", 16, nad, (128, 384, 1024), (64, 192))


def reduce_ring_ranges():
    return _ranges("reduce/ring ranges", 16, [(0, 64), (64, 128), (192, 64)], (128, 384))


BGRAD_STAGED_COLS = [(8, 72), (80, 64)]                 # one width of 72: the ragged width keeps rank 16 on the register-staged kernel


def bgrad_staged(rank):
    t = hip.lora_plan("bgrad", 1, rank=rank, cols=BGRAD_STAGED_COLS)["tok_per_block"]      # tokens per block of the register-staged kernel
    return _ranges("bgrad/staged", rank, BGRAD_STAGED_COLS, (t - 1, t, t + 1))


def bgrad_ring_512():
    return _ranges("bgrad/ring 512", 16, [(64, 128), (192, 64)], (1, 511, 513, 1100))


RING_1024_COLS = [(0, 64), (64, 64), (128, 64), (192, 64)]


def bgrad_ring_1024_rows(cu_count):
    """the first row of the smallest number of 1024-token blocks at which a device of cu_count CUs runs the 1024-token kernel, plus 37"""
    first = lambda blocks: (blocks - 1) * 1024 + 1      # noqa: E731
    blocks = next(b for b in itertools.count(1) if hip.lora_plan("bgrad", first(b), cols=RING_1024_COLS, cu_count=cu_count)["kernel"] == "ring1024")
    return first(blocks) + 37


def bgrad_ring_1024(cu_count):
    return _ranges("bgrad/ring 1024", 16, RING_1024_COLS, (bgrad_ring_1024_rows(cu_count),))


def plan_of(op, c, cu_count=0, **kw):
    """the library's answer for case c by its sizes (lora_plan_args: dense rows, masked launches with their planes)"""
    return hip.lora_plan(op, c["M"], c["W"], c["rank"], c["nad"], cols=c["cols"], masked=c["keep"] is not None, pad=8, cu_count=cu_count, **kw)


def kernel_of(path):
    """the kernel (hip.LORA_KERNELS) a path label names: '<op>/staged ...', '<op>/ring ...', 'bgrad/ring 1024'"""
    word = path.split("/")[1]
    return "ring1024" if word.startswith("ring 1024") else word.split()[0]


def epilogue_cases(rank, nad):
    i = 0
    for N in (136, 264):
        for M in (1, 200):
            i += 1
            for family, p in (("exact", EXACT_P), ("random", 0.1)):
                c = epilogue_case(family, M, N, 64, rank, nad, p, seed=500 + i + rank + nad, row0=(0, ROW0_BIG)[i % 2])
                c["path"] = "gemm masked epilogue"
                yield c


def fused_case(M, W, nad, p, seed, row0=0):
    """adapter weights, alpha and keep planes of a fused launch (random family: the projected operand is the kernel's own h / act)"""
    g = gen(seed)
    U = [values("random", (16, W), g, scale=0.05) for _ in range(nad)]
    keep = torch.from_numpy(dropout_ref.lora_keep(seed, p, M, W, nad, row0).astype(np.float64)) if p > 0 else None
    return dict(family="random", M=M, W=W, rank=16, nad=nad, p=p, cols=None, seed=seed, row0=row0, U=U, alpha=RANDOM_S / (1.0 - p), keep=keep)

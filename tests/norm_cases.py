"""Inputs of the norm / reduction / GEMM-epilogue tests, shared by tests/test_ref64.py (CPU: the criteria bite) and
tests/test_gpu_norm_f64.py (GPU).  Plain torch on the CPU, seeded generators, bf16 values returned as bf16 tensors."""
import torch

BF16 = torch.bfloat16
KINDS = ("scale 1e-3", "scale 1", "scale 300", "mean 100 std 1", "mean 1000 std 8")
EQUAL_VALUE = 3.0                    # the all-equal row: H * 3 and every partial sum are exact in float32, so mean == 3 and z - mean == 0 exactly


def gen(seed):
    return torch.Generator().manual_seed(seed)


def norm_weight(n, seed):
    """+-[0.25, 4], log-uniform, a third of them negative (as _norm_weight of tests/test_gpu_head_primitives.py)"""
    g = gen(seed)
    mag = torch.exp2(torch.rand(n, generator=g) * 4.0 - 2.0)
    sign = torch.where(torch.rand(n, generator=g) < 1.0 / 3.0, -1.0, 1.0)
    return (mag * sign).float()


def row_kind(r, H):
    return (r + H // 8) % len(KINDS)


def equal_row(M):
    """index of the all-equal row, or -1 (M < 5: every row is needed for the five kinds of data)"""
    return M // 2 if M >= 5 else -1


def rows(M, H, seed, kinds=None):
    """[M, H] bf16: row r is of kind row_kind(r, H) -- centred randn at scale 1e-3 / 1 / 300, or offset rows at mean 100 / std 1 and
    mean 1000 / std 8 -- and row equal_row(M) holds EQUAL_VALUE everywhere.  kinds: restrict to these kind indices."""
    g = gen(seed)
    x = torch.randn(M, H, generator=g)
    k = torch.tensor([row_kind(r, H) for r in range(M)])
    if kinds is not None:
        k = torch.tensor(list(kinds))[k % len(kinds)]
    scale = torch.tensor([1e-3, 1.0, 300.0, 1.0, 8.0])[k][:, None]
    shift = torch.tensor([0.0, 0.0, 0.0, 100.0, 1000.0])[k][:, None]
    x = x * scale + shift
    e = equal_row(M)
    if e >= 0:
        x[e] = EQUAL_VALUE
    return x.to(BF16)


def residual_rows(M, H, seed):
    """[M, H] bf16 residual: a quarter of the row's spread, so z = y + residual keeps the row's kind; 1.0 on the all-equal row"""
    g = gen(seed)
    k = torch.tensor([row_kind(r, H) for r in range(M)])
    scale = torch.tensor([1e-3, 1.0, 300.0, 1.0, 8.0])[k][:, None]
    x = torch.randn(M, H, generator=g) * scale * 0.25
    e = equal_row(M)
    if e >= 0:
        x[e] = 1.0
    return x.to(BF16)

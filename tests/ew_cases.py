"""Inputs shared by tests/test_ref64.py (CPU: the references and that the criteria bite) and tests/test_gpu_elementwise_f64.py /
tests/test_gpu_dw_f64.py (GPU: the kernels).  Plain torch on the CPU, no device code."""
import numpy as np
import torch

F32 = torch.float32

# ur_adamw_step: 4 elements per thread, at most 2048 workgroups of 256 threads -- a vector beyond 2,097,152 elements enters the grid-stride
# loop.  The large size runs three more full rounds of one workgroup and a 3-element tail; the small ones are the tail alone (3), one vector
# (4), vector + tail (7) and a prime (1021).
ADAMW_STRIDE = 2048 * 256 * 4
ADAMW_SIZES = (3, 4, 7, 1021, ADAMW_STRIDE + 4 * 256 * 3 + 3)
ADAMW_STEPS = (1, 2, 10, 100000)          # 100000: b1^t underflows to 0, b2^t to a float32 subnormal
ADAMW_HYPER = dict(b1=0.9, b2=0.999, eps=1e-8)
ADAMW_GRAD_SCALE = 1.0 / 3.0              # not a power of two: a scale applied once where it belongs twice shows

# the casts and ur_add_bf16: 8 elements per thread
CAST_STRIDE = 2048 * 256 * 8
CAST_SIZES = (1, 7, 8, 9, CAST_STRIDE + 8 * 256 * 2 + 5)
ADD_SIZE = CAST_STRIDE + 8 * 256 * 2
CAST_LOW_HALVES = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def adamw_inputs(n, step, seed):
    """(p, g, m, v) float32 [n].  |p| <= 0.1 against a step of about lr: the update is at least as large as the parameter.  The gradient's
    magnitude is ONE power of ten per 64-element row (the rows of ref64.rows_of), 1e-12 .. 1e3 over the rows, mantissa 0.5 .. 1, random
    sign; one element in eight is an exact zero, and half of those have m = v = 0 too (v stays 0: the denominator is eps alone).  The saved
    moments are what step - 1 steps over gradients of the row's scale leave behind: m of that scale times 1 - b1^(step - 1), v of its square
    times 1 - b2^(step - 1) -- zero at step 1."""
    g_ = _gen(seed)
    rows = -(-n // 64)
    expo = (torch.arange(rows) * 7 + seed) % 16 - 12
    scale = (10.0 ** expo.to(torch.float64)).repeat_interleave(64)[:n]
    u = lambda: torch.rand(n, generator=g_, dtype=torch.float64)      # noqa: E731
    sign = torch.where(u() < 0.5, -1.0, 1.0)
    g = sign * scale * (0.5 + 0.5 * u())
    p = (u() * 2 - 1) * 0.1
    m = scale * (u() * 2 - 1) * (1.0 - ADAMW_HYPER["b1"] ** (step - 1))
    v = scale * scale * (0.25 + 0.75 * u()) * (1.0 - ADAMW_HYPER["b2"] ** (step - 1))
    zero = u() < 0.125
    cold = zero & (u() < 0.5)
    g = torch.where(zero, torch.zeros_like(g), g)
    m = torch.where(cold, torch.zeros_like(m), m)
    v = torch.where(cold, torch.zeros_like(v), v)
    return p.to(F32), g.to(F32), m.to(F32), v.to(F32)


def cast_patterns():
    """float32 [6 * 65536]: every upper half 0x0000 .. 0xffff over each of CAST_LOW_HALVES -- exact values, ties towards both parities, the
    carry into the exponent, overflow to infinity, subnormals, both zeros, the infinities and NaNs of every upper half."""
    hi = np.arange(65536, dtype=np.uint32)
    words = np.concatenate([(hi << 16) | np.uint32(lo) for lo in CAST_LOW_HALVES])
    return torch.from_numpy(words.view(np.float32).copy())


def bf16_patterns():
    """bfloat16 [65536]: every bit pattern"""
    return torch.from_numpy(np.arange(65536, dtype=np.uint16).view(np.int16).copy()).view(torch.bfloat16)


def add_operands(n, seed):
    """(a, b) bfloat16 [n]: b's exponent lies 0 .. 20 below a's (cycling over the elements), random mantissas and signs -- sums that cancel,
    sums that carry, and addends below half an ulp of the other"""
    g_ = _gen(seed)
    mant = lambda: 1.0 + torch.randint(0, 128, (n,), generator=g_).to(F32) / 128.0          # noqa: E731   (exact in bf16, below 2)
    sign = lambda: torch.where(torch.rand(n, generator=g_) < 0.5, -1.0, 1.0)                 # noqa: E731
    ea = torch.randint(-8, 9, (n,), generator=g_).to(F32)
    a = sign() * mant() * 2.0 ** ea
    b = sign() * mant() * 2.0 ** (ea - (torch.arange(n) % 21).to(F32))
    return a.to(torch.bfloat16), b.to(torch.bfloat16)


# ur_field_projection_*: (B, Q, F, E); FPROJ_FAST are the shapes the Q = 32 kernels (fproj_fwd32_kernel / fproj_bwd32_kernel) take
FPROJ_GENERIC = ((300, 4, 8, 256), (2100, 4, 8, 256), (3, 64, 32, 100), (5, 32, 17, 256))
FPROJ_FAST = ((5, 32, 14, 256), (300, 32, 16, 128), (7, 32, 1, 384))


def fproj_inputs(B, Q, F, E, seed):
    """(rec bf16 [B, Q, E], Wf f32 [F, Q], bf f32 [F], dout f32 [B, F, E])"""
    g_ = _gen(seed)
    rec = torch.randn(B, Q, E, generator=g_).to(torch.bfloat16)
    Wf = torch.randn(F, Q, generator=g_) * 0.3
    bf = torch.randn(F, generator=g_)
    dout = torch.randn(B, F, E, generator=g_)
    return rec, Wf, bf, dout
